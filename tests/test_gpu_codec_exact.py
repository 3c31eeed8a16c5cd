"""The streaming tokenizer chains (acoustic decoder -> semantic encoder, one frame per call, conv histories per utterance slot)
at the real channel widths, in the two exact modes, every frame of every slot against the fp32 CPU oracle.

xsplit 3 runs the per-slot paths with exact fp32 activations; xsplit 2 takes the kernel families of the timed bf16 mode (tile
and 16-row GEMV forms, slot batching, fused block1d at C = 32 / 64 / 128, row-tiled norm + conv at 256 / 512, channel-sliced at
1024, the T = 1 PRO_NORMDW GEMV stage at 2048) with two-term activations.  The bounds (codec_exact.B*) are a few 1e-5 to 1e-4,
and test_codec_fault_sensitivity_cpu.py shows that a wrong history row anywhere in either net moves an output by at least four
times as much -- which the 5e-2 of the bf16-mode test at these widths (test_gpu_fullsize.py) cannot see.

The runners return every figure; the tests print the worst and then assert, so a measuring script can call the runners alone.
"""
import contextlib

import pytest
import torch

import codec_exact as ce

pytestmark = pytest.mark.gpu

SEED = 0
DEPTHS = {"REAL": ce.REAL, "MIXED": ce.MIXED}

# (slots of the batched call, slots on the one-utterance path, slots of a second batched call without a semantic output) per
# frame.  Slot 1 mirrors slot 0's inputs on the one-utterance path throughout (the pair check); slot 2 alternates between the
# two paths; slot 3 is reset before frame 2; frame 1 carries all 8 rows, out of order and with the last slot; frame 3 is n = 1;
# [9, 0, 3] and [2, 0] come back, so their second call replays a captured graph (as every one-utterance call after a slot's
# first); slots 4 and 5 are never encoded again after their decode-only call.  29 slot-frames.
PLAN = [
    ([9, 0, 3], [1, 2], []),
    ([9, 0, 2, 3, 4, 5, 6, 7], [1], []),
    ([9, 0, 3], [1, 2], []),
    ([0], [1], []),
    ([2, 0], [1], []),
    ([2, 0], [1], [5, 4]),
]
PLAN_RESET = {2: [3]}                # frame -> slots reset before it
PLAN_REAL = [([0, 1, 2], [], [])] * 4


class Store:
    """the synthetic weights per depth list and the oracle's outputs per (depths, plan, seed), each computed once"""

    def __init__(self):
        self._weights, self._oracle = {}, {}

    def weights(self, name):
        if name not in self._weights:
            self._weights[name] = ce.codec_weights(DEPTHS[name])
        return self._weights[name]

    def oracle(self, name, tag, plan, resets, seed):
        """(frame, slot) -> (audio, semantic or None)"""
        key = (name, tag, seed)
        if key not in self._oracle:
            ac_w, sem_w = self.weights(name)
            cc, sc = ce.codec_cfgs(DEPTHS[name])
            chains, ref = {}, {}
            for t, ((batch, single, nosem), lat) in enumerate(zip(plan, plan_latents(plan, seed))):
                for s in resets.get(t, []):
                    chains[s].reset()
                for s in batch + single + nosem:
                    ch = chains.setdefault(s, ce.OracleChain(ac_w, sem_w, cc, sc))
                    ref[(t, s)] = ch.step(lat[s], sem=s not in nosem)
            self._oracle[key] = ref
        return self._oracle[key]

    @contextlib.contextmanager
    def engine(self, xsplit, name, n_slots, use_graph):
        eng = ce.build_codec_engine(xsplit, DEPTHS[name], n_slots, use_graph, weights=self.weights(name))[0]
        try:
            yield eng
        finally:
            eng.close()


@pytest.fixture(scope="module")
def store():
    return Store()


def plan_latents(plan, seed):
    """frame -> {slot: latent [64]}: every slot its own stream, slot 1 a copy of slot 0's"""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for batch, single, nosem in plan:
        lat = {s: torch.randn(64, generator=g) * 0.7 for s in sorted(set(batch + single + nosem))}
        if 1 in single and 0 in lat:
            lat[1] = lat[0].clone()
        out.append(lat)
    return out


# ------------------------------------------------------------------------------------------------------------ runners
def run_one_slot(store, eng, name, seed):
    """Six frames on slot 1 through codec_decode + semantic_encode with a reset after frame 3, then two frames on the untouched
    slot 0.  -> [(label, audio rel-L2, semantic rel-L2)]"""
    plan = [([], [1], [])] * 6 + [([], [0], [])] * 2
    # slot 1's mirror rule does not apply here: plan_latents copies slot 0 only where both are in a frame
    ref = store.oracle(name, "one_slot", plan, {4: [1]}, seed)
    lats = plan_latents(plan, seed)
    lat_d, audio, sem = eng.new(1, 64), eng.new(3200), eng.new(128)
    figs = []
    for t, (_, single, _) in enumerate(plan):
        s = single[0]
        with torch.cuda.stream(eng.stream):
            lat_d.copy_(lats[t][s][None])
            if t == 4:
                eng.codec_reset(1)
            eng.codec_decode(s, lat_d, audio)
            eng.semantic_encode(s, audio, sem)
        eng.sync()
        ra, rs = ref[(t, s)]
        figs.append((f"frame {t} slot {s}", ce.rel_l2(audio, ra), ce.rel_l2(sem, rs)))
    return figs


def run_plan(store, eng, name, tag, plan, resets, seed):
    """-> ([(label, audio rel-L2, semantic rel-L2 or None)] against the oracle, [(label, audio, semantic)] batched slot 0 against
    one-utterance slot 1)"""
    ref = store.oracle(name, tag, plan, resets, seed)
    lats = plan_latents(plan, seed)
    lat_b, audio_b, sem_b = eng.new(8, 64), eng.new(8, 3200), eng.new(8, 128)
    lat_n, audio_n = eng.new(8, 64), eng.new(8, 3200)
    one = {}                                        # one-utterance path: fixed buffers per slot, so its graphs replay
    figs, pair = [], []
    for t, (batch, single, nosem) in enumerate(plan):
        lat = lats[t]
        with torch.cuda.stream(eng.stream):
            lat_b[:len(batch)].copy_(torch.stack([lat[s] for s in batch]))
            if nosem:
                lat_n[:len(nosem)].copy_(torch.stack([lat[s] for s in nosem]))
            for s in single:
                if s not in one:
                    one[s] = (eng.new(1, 64), eng.new(3200), eng.new(128))
                one[s][0].copy_(lat[s][None])
            for s in resets.get(t, []):
                eng.codec_reset(s)
            eng.codec_chain_batch(batch, lat_b[:len(batch)], audio_b[:len(batch)], sem_b[:len(batch)])
            if nosem:
                eng.codec_chain_batch(nosem, lat_n[:len(nosem)], audio_n[:len(nosem)], None)
            for s in single:
                eng.codec_decode(s, one[s][0], one[s][1])
                eng.semantic_encode(s, one[s][1], one[s][2])
        eng.sync()
        outs = {s: (audio_b[j].cpu(), sem_b[j].cpu()) for j, s in enumerate(batch)}
        outs.update({s: (audio_n[j].cpu(), None) for j, s in enumerate(nosem)})
        outs.update({s: (one[s][1].cpu(), one[s][2].cpu()) for s in single})
        for s, (a, se) in sorted(outs.items()):
            ra, rs = ref[(t, s)]
            figs.append((f"frame {t} slot {s}", ce.rel_l2(a, ra), None if se is None else ce.rel_l2(se, rs)))
        if 0 in batch and 1 in single:
            pair.append((f"frame {t}", ce.rel_l2(outs[0][0], outs[1][0]), ce.rel_l2(outs[0][1], outs[1][1])))
    return figs, pair


def worst(figs):
    return max(f[1] for f in figs), max(f[2] for f in figs if f[2] is not None)


def hold(figs, b_audio, b_sem):
    bad = [f for f in figs if not f[1] <= b_audio or (f[2] is not None and not f[2] <= b_sem)]     # a NaN is a miss
    assert not bad, (bad, b_audio, b_sem)


# -------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ["REAL", "MIXED"])
@pytest.mark.parametrize("xs", [2, 3])
def test_streaming_chain_one_slot(store, xs, name):
    with store.engine(xs, name, 2, False) as eng:
        figs = run_one_slot(store, eng, name, SEED)
    wa, ws = worst(figs)
    print(f"streaming_chain_one_slot[xsplit {xs}, {name}]: audio vs oracle {wa:.2e}, semantic vs oracle {ws:.2e}")
    hold(figs, *((ce.B2_AUDIO, ce.B2_SEM) if xs == 2 else (ce.B3_AUDIO, ce.B3_SEM)))


@pytest.mark.parametrize("mode", ["full", "heavy"])
def test_chain_batch_exact(store, mode, monkeypatch):
    """mode "full": every stage of both nets slot-batched (the default); "heavy": only the T <= 8 stages, the rest per utterance
    on forked graph branches (VVHIP_BATCH_CODEC=heavy, read when the engine is created)"""
    if mode == "heavy":
        monkeypatch.setenv("VVHIP_BATCH_CODEC", "heavy")
    else:
        monkeypatch.delenv("VVHIP_BATCH_CODEC", raising=False)
    assert sum(len(b) + len(s) + len(n) for b, s, n in PLAN) <= 30
    with store.engine(2, "MIXED", 10, True) as eng:
        figs, pair = run_plan(store, eng, "MIXED", "plan", PLAN, PLAN_RESET, SEED)
    wa, ws = worst(figs)
    wp = max(max(p[1], p[2]) for p in pair)
    print(f"chain_batch_exact[{mode}]: audio vs oracle {wa:.2e}, semantic vs oracle {ws:.2e}, batched vs single {wp:.2e}")
    hold(figs, ce.B2_AUDIO, ce.B2_SEM)
    assert len(pair) == len(PLAN)
    hold(pair, ce.B2_PAIR, ce.B2_PAIR)


def test_chain_batch_real_depths(store, monkeypatch):
    """the shipped block counts (3-3-3-3-3-3-8) once through the slot-batched path: three slots, four frames"""
    monkeypatch.delenv("VVHIP_BATCH_CODEC", raising=False)
    with store.engine(2, "REAL", 3, True) as eng:
        figs, _ = run_plan(store, eng, "REAL", "real", PLAN_REAL, {}, SEED)
    wa, ws = worst(figs)
    print(f"chain_batch_real_depths: audio vs oracle {wa:.2e}, semantic vs oracle {ws:.2e}")
    hold(figs, ce.B2_AUDIO, ce.B2_SEM)
