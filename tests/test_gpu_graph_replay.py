"""Every captured hipGraph against an eager engine, across the calls that change engine state.

graphed_run (csrc/engine.hip) runs a key eagerly at its first sight, captures it at the second and replays it after; a replay repeats
every scalar argument and every pointer of the captured launches.  It is right only if whatever can change between two calls is read
from device memory, named in the key, or dropped by the call that changes it (the table in DESIGN.md section 3 and above graphed() in
csrc/engine_ctx.h).  Each test here takes one cell of that table: two engines that differ only in use_graph are given the same calls
in the same order -- resets, setters and uploads included, since the tokenizer history and the KV cache evolve from call to call --
every call is issued three times with the same tensors (eager, captured, replayed) and every output of every call is compared with
torch.equal.  Bit for bit is the project's claim, not a tolerance: the decode kernels sum in a fixed order without atomics (headers of
gemv16p.hip and gemm.hip, vv_attn_merge2_kernel); the one flag-based hand-off, the prefill GEMM's K-split, is not reached here.

"Would a stale replay pass?" is closed by a precondition on the EAGER engine alone: its outputs before and after the change differ by
rel-L2 > 1e-1.  When the graph engine misses, the message says whether its output equals its own pre-change output bit for bit -- the
signature of a stale replay.

Geometry: the "gqa" LM of test_gpu_kernels.LM_CASES (hidden 256, 4 / 2 heads, 3 layers), max_ctx 1280, 16 rows, 8 slots, the
synthetic tokenizers of build_small, a 2-layer head of width 256, 5 solver steps.  Every tensor handed to an engine stays allocated
until the module ends: graph keys hold addresses, and an address the allocator hands out twice would make one test's first sight
another test's replay.  vv_stat(1) counts cached graphs; the counts asserted per test are in the docstrings."""
import pytest
import torch

import lm_shapes as ls
import synth
from gpu_util import build_small, rel_err
from oracle import codec

pytestmark = pytest.mark.gpu

H, N_STEPS = 256, 5
FACTORS = (0.2, -0.05)
# first call after a reset against oracle/codec.py, the bounds of the tests that hold these paths already:
#   xsplit 3  test_codec_decode_stream_reset / test_semantic_encode_stream (each net on the input the engine's net saw)
#   xsplit 1  test_codec_chain_batch_at_real_widths (the encoder on the oracle's audio)
ORACLE_TOL = {3: 2e-4, 1: 5e-2}

_pairs, _keep, _sights = {}, [], {}


def _pair(xs, monkeypatch, heavy=False):
    """(graph Small, eager Small) -- equal but for use_graph; VVHIP_BATCH_CODEC is read when an engine is created"""
    key = (xs, heavy)
    if key not in _pairs:
        from test_gpu_kernels import LM_CASES
        if heavy:
            monkeypatch.setenv("VVHIP_BATCH_CODEC", "heavy")
        else:
            monkeypatch.delenv("VVHIP_BATCH_CODEC", raising=False)
        mk = lambda graph: build_small(LM_CASES[ls.REPLAY_ENGINE[0]], xsplit=xs, use_graph=graph, n_slots=8, max_ctx=1280,
                                       max_rows=ls.REPLAY_ENGINE[1], head_layers=2)
        _pairs[key] = (mk(True), mk(False))
    return _pairs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for pair in _pairs.values():
        for s in pair:
            s.eng.close()
    _pairs.clear()
    _keep.clear()
    _sights.clear()


def _new(eng, *shape):
    t = eng.new(*shape)
    _keep.append(t)
    return t


def _dev(eng, t):
    out = _new(eng, *t.shape)
    _put(eng, out, t)
    return out


def _put(eng, buf, host):
    """new values into the SAME device buffer, ordered on the engine stream"""
    with torch.cuda.stream(eng.stream):
        buf.copy_(host.to(eng.device, torch.float32))


def _graphs(eng):
    return eng.stat(1)


def _clean(pair):
    """every test ends here: no capture fell back to an eager run, no captured graph holds a memset / memcpy node"""
    g = pair[0].eng
    g.sync()
    pair[1].eng.sync()
    assert g.stat(4) == 0, g.stat(4)
    assert g.stat(5) == 0, g.stat(5)


def _same(got, want, own_before, what):
    """got (graph engine) == want (eager engine) bit for bit; a miss says whether got is the graph engine's own pre-change output"""
    if torch.equal(got, want):
        return
    if own_before is None:
        tail = "no state change precedes this call"
    elif own_before.shape == got.shape and torch.equal(got, own_before):
        tail = "it EQUALS the graph engine's own pre-change output bit for bit: a stale replay"
    else:
        tail = "it does not equal the graph engine's own pre-change output"
    pytest.fail(f"{what}: the graph engine differs from the eager engine, rel-L2 {rel_err(got, want):.3e}; {tail}")


def _moved(after, before, what):
    """the precondition, on the eager engine: the change moves the result by more than 1e-1"""
    e = rel_err(after, before)
    assert e > 1e-1, f"{what}: the eager engine's output moved by {e:.3e} only -- a stale replay could pass"


# ------------------------------------------------------------------------------------------------ (a) tokenizer graphs, speech factors
def _latents(n, seed=6100):
    return torch.randn(n, 64, generator=torch.Generator().manual_seed(seed)) * 0.7


_oracle_audio = {}


def _first_frame_oracle(s, xs, lat_row, scaling, bias, audio, sem, what):
    """one slot's first frame after a reset against the oracle's streaming nets on empty state"""
    key = (tuple(lat_row.tolist()), scaling, bias)
    if key not in _oracle_audio:
        x = lat_row if scaling is None else lat_row / scaling - bias
        with torch.no_grad():
            _oracle_audio[key] = codec.decoder_forward(s.ac_w, x[None, :, None], s.cc.ratios, s.cc.dec_depths, {}, s.cc.eps)[0, 0]
    ra = _oracle_audio[key]
    ea = rel_err(audio, ra)
    print(f"[{what}] audio vs oracle {ea:.3e} (bound {ORACLE_TOL[xs]:.0e})")
    assert ea <= ORACLE_TOL[xs], (what, ea)
    if sem is not None:
        src = ra if xs == 1 else audio.cpu()
        with torch.no_grad():
            rs = codec.encoder_forward(s.sem_w, src[None, None], s.sc.ratios, s.sc.enc_depths, {}, s.sc.eps)[0, :, 0]
        es = rel_err(sem, rs)
        print(f"[{what}] semantic vs oracle {es:.3e} (bound {ORACLE_TOL[xs]:.0e})")
        assert es <= ORACLE_TOL[xs], (what, es)


class _Codec:
    """one engine's buffers for a slot set and the three tokenizer entry points over them"""

    def __init__(self, eng, slots, lat):
        self.eng, self.slots, n = eng, list(slots), len(slots)
        self.lat, self.audio, self.sem = _dev(eng, lat[:n]), _new(eng, n, 3200), _new(eng, n, 128)

    def reset(self):
        with torch.cuda.stream(self.eng.stream):
            for sl in self.slots:
                self.eng.codec_reset(sl)

    def call(self, family):
        e = self.eng
        with torch.cuda.stream(e.stream):
            if family == "dec":
                for j, sl in enumerate(self.slots):
                    e.codec_decode(sl, self.lat[j:j + 1], self.audio[j])
                    e.semantic_encode(sl, self.audio[j], self.sem[j])
            else:
                e.codec_chain_batch(self.slots, self.lat, self.audio, self.sem, apply_speech_factors=family == "chain")
        e.sync()
        return self.audio.cpu(), self.sem.cpu()


# the forked-branch mode changes the batched chain only: codec_decode and the one-utterance chain have one form
A_CASES = [(xs, slots, heavy, family) for xs in (1, 3) for slots, heavy in (((0,), False), ((0, 1), False), ((0, 1), True))
           for family in (("chain",) if heavy else ("chain", "dec", "chain-raw"))]
A_IDS = [f"{fam}-xs{xs}-slots{''.join(map(str, sl))}{'-heavy' if hv else ''}" for xs, sl, hv, fam in A_CASES]


@pytest.mark.parametrize("xs,slots,heavy,family", A_CASES, ids=A_IDS)
def test_speech_factors_reach_the_tokenizer_replays(xs, slots, heavy, family, monkeypatch):
    """Factors (1.0, 0.0), then (0.2, -0.05), then (1.0, 0.0) again; after each setter a reset of the slots and three calls on one
    latent tensor.  "chain": vv_codec_chain_batch with semantic output (slots [0]: the one-utterance path; [0, 1]: the slot-batched
    path, vv_affine_slots; heavy: forked graph branches); "dec": vv_codec_decode + vv_semantic_encode per slot, the dec: and senc:
    families; "chain-raw": the chain with apply_speech_factors=False.  1 / scaling and -bias are computed on the host inside the
    captured body and passed by value, so the setter must drop every graph that applied them and no other.  vv_stat(1), at the second
    call of a phase and unchanged at the third:
      chain      +1 in every phase, -1 at each setter
      dec        +2 per slot in the first phase (dec: and senc:), then -1 per slot at each setter (senc: holds no factor and stays)
                 and +1 per slot in the phase after it
      chain-raw  +1 in the first phase and nothing after: its graph holds no factor, stays cached, and gives the same outputs
                 in every phase"""
    pair = _pair(xs, monkeypatch, heavy)
    lat = _latents(len(slots))
    runs = [_Codec(s.eng, slots, lat) for s in pair]
    n = len(slots)
    cache0, drop = {"chain": (1, 1), "dec": (2 * n, n), "chain-raw": (1, 0)}[family]      # graphs of the first phase; dropped by a setter
    geng = pair[0].eng
    applied = family != "chain-raw"
    phases = ((1.0, 0.0), FACTORS, (1.0, 0.0))
    before = None                      # previous phase: per call (graph outputs, eager outputs)
    for ph, (scaling, bias) in enumerate(phases):
        for s, r in zip(pair, runs):
            s.eng.sync()
            s.eng.set_speech_factors(scaling, bias)
            r.reset()
        base = _graphs(geng)
        now = []
        for call in range(3):
            got, want = runs[0].call(family), runs[1].call(family)
            what = f"{A_IDS[A_CASES.index((xs, slots, heavy, family))]} factors ({scaling}, {bias}) call {call}"
            for k, (a, b) in enumerate(zip(got, want)):
                assert bool(torch.isfinite(b).all()), what
                if before is not None and applied:
                    _moved(b, before[call][1][k], what)
                if before is not None and not applied:
                    assert torch.equal(b, before[call][1][k]), f"{what}: the setter changed a chain that does not apply the factors"
                _same(a, b, before[call][0][k] if before is not None else None, what)
            if call == 0:
                for j in range(len(slots)):
                    _first_frame_oracle(pair[1], xs, lat[j], scaling if applied else None, bias, want[0][j], want[1][j], what + f" row {j}")
            if call >= 1:
                assert _graphs(geng) == base + (cache0 if ph == 0 else drop), (what, _graphs(geng), base, cache0, drop)
            now.append((got, want))
        if ph > 0:
            assert base == cached - drop, f"{family}: the setter dropped {cached - base} graph(s), {drop} hold the old factors"
        cached = _graphs(geng)
        before = now
    _clean(pair)


# ------------------------------------------------------------------------------------------------ (b) one key per slot order
@pytest.mark.parametrize("xs", [1, 3])
def test_chain_graphs_are_keyed_by_slot_order(xs, monkeypatch):
    """The same three tensors for every call; slot lists [0, 1], [1, 0], [1], [0, 1] in rotation, three rounds, new latent rows
    each call.  The slot list is a key field (the captured launches hold the slots' buffers): three graphs in all, and in every
    replay row j is slot slots[j]'s next frame -- equal to the eager engine, and held to the oracle's stream of that slot."""
    pair = _pair(xs, monkeypatch)
    lat0 = _latents(2, 6200)
    runs = [_Codec(s.eng, (0, 1), lat0) for s in pair]
    for s, r in zip(pair, runs):
        s.eng.sync()
        s.eng.set_speech_factors(*FACTORS)
        r.reset()
    geng = pair[0].eng
    g0 = _graphs(geng)
    st_dec, st_sem = {0: {}, 1: {}}, {0: {}, 1: {}}
    s = pair[1]
    sights, expect = {}, g0
    for rnd in range(3):
        for i, slots in enumerate(([0, 1], [1, 0], [1], [0, 1])):
            n = len(slots)
            lat = _latents(n, 6210 + 10 * rnd + i)
            outs = []
            for r in runs:
                _put(r.eng, r.lat[:n], lat)
                with torch.cuda.stream(r.eng.stream):
                    r.eng.codec_chain_batch(slots, r.lat[:n], r.audio[:n], r.sem[:n])
                r.eng.sync()
                outs.append((r.audio[:n].cpu(), r.sem[:n].cpu()))
            what = f"xs{xs} round {rnd} slots {slots}"
            sights[tuple(slots)] = sights.get(tuple(slots), 0) + 1
            expect += sights[tuple(slots)] == 2
            assert _graphs(geng) == expect, (what, _graphs(geng), expect)
            (ga, gs), (ea, es) = outs
            _same(ga, ea, None, what + " audio")
            _same(gs, es, None, what + " semantic")
            for j, sl in enumerate(slots):
                x = lat[j] / FACTORS[0] - FACTORS[1]
                with torch.no_grad():
                    ra = codec.decoder_forward(s.ac_w, x[None, :, None], s.cc.ratios, s.cc.dec_depths, st_dec[sl], s.cc.eps)[0, 0]
                    src = ra if xs == 1 else ea[j]                # as ORACLE_TOL says: the protocol of the test each bound is from
                    rs = codec.encoder_forward(s.sem_w, src[None, None], s.sc.ratios, s.sc.enc_depths, st_sem[sl], s.sc.eps)[0, :, 0]
                tol = ORACLE_TOL[xs]
                assert rel_err(ea[j], ra) <= tol and rel_err(es[j], rs) <= tol, (what, j, rel_err(ea[j], ra), rel_err(es[j], rs))
            if n == 2:
                _moved(ea[0], ea[1], what + ": the two slots' rows")      # a row handed to the wrong slot would show
    assert _graphs(geng) == g0 + 3
    _clean(pair)


# ------------------------------------------------------------------------------------------------ (c) samp: / sde: and the schedule
class _Sampler:
    def __init__(self, eng, n, seed, cond_std=3.0):
        g = synth.Gen(seed)
        self.eng, self.n = eng, n
        self.cond = _dev(eng, torch.cat([g.normal((n, H), cond_std, mat=False), g.normal((n, H), cond_std, mat=False)]))
        self.noise = _dev(eng, g.normal((n, 64), 1.0, mat=False))
        self.sn = _dev(eng, g.normal((N_STEPS, n, 64), 1.0, mat=False))
        self.out = _new(eng, n, 64)

    def call(self, cfg, sde=False):
        e = self.eng
        with torch.cuda.stream(e.stream):
            e.diffusion_sample(self.n, self.cond, self.noise, cfg, self.out, step_noise=self.sn if sde else None)
        e.sync()
        return self.out.cpu()


def _fresh_schedule(pair):
    """5 deterministic steps, installed anew: a schedule drops the sampler graphs of the WHOLE engine, so a test that counts them
    starts from none (the engines are shared by the module)"""
    for s in pair:
        s.eng.sync()
        s.eng.set_num_steps(2 * N_STEPS)
        s.eng.set_num_steps(N_STEPS)
    return _graphs(pair[0].eng)


def _three_calls(pair, runs, base, before, what, **kw):
    """three calls on both engines; one graph at the second, none at the third -> [(graph output, eager output)]"""
    geng, now = pair[0].eng, []
    for call in range(3):
        got, want = runs[0].call(**kw), runs[1].call(**kw)
        assert bool(torch.isfinite(want).all()), what
        if before is not None:
            _moved(want, before[call][1], f"{what} call {call}")
        _same(got, want, before[call][0] if before is not None else None, f"{what} call {call}")
        if call >= 1:
            assert _graphs(geng) == base + 1, (what, call, _graphs(geng), base)
        now.append((got, want))
    return now


C_CFG = 3.0


@pytest.mark.parametrize("n", [1, 3, 8])
def test_sampler_graphs_follow_the_schedule(n, monkeypatch):
    """vv_diffusion_sample / _sde with a scalar cfg_scale, xsplit 1, n = 1, 3, 8: 2, 6 and 16 head rows -- the GEMV layers with the
    seam, and the packed 16-row forms vv_head_plan chooses.  A captured sample_body holds the step count, the table offsets and the
    per-step buffers a longer schedule reallocates; none is a key field, so set_schedule must drop samp: and sde: graphs.
    5 steps, 10 steps, 5 steps; then at 5 steps dpmsolver++ -> sde-dpmsolver++ -> dpmsolver++ (sde_on flips: the wrong entry point
    raises, the right one matches the eager engine on its first, second and third call).  Every setter drops one graph, every phase
    caches one (vv_stat(1): +1 at the second call, +0 at the third; +1 over the whole test, 5 captures).
    Precondition: the solver switch moves the result by ~1; halving the step moves it by the solver's discretisation error, 0.15 - 0.2
    on the fp32 CPU oracle (oracle/dpm.py) at conditions of std 3 and cfg_scale 3.0, the inputs used here (0.09 - 0.15 at std 1
    and 1.3, too close to the 1e-1 this file asks for)."""
    from vibevoice_amd.engine import EngineError
    pair = _pair(1, monkeypatch)
    runs = [_Sampler(s.eng, n, 5202 + n) for s in pair]
    geng = pair[0].eng

    def schedule(steps, solver):
        for s in pair:
            s.eng.sync()
            s.eng.set_num_steps(steps, algorithm_type=solver)
        return _graphs(geng)
    try:
        g0 = _fresh_schedule(pair)
        prev, cached = None, None
        for steps in (N_STEPS, 2 * N_STEPS, N_STEPS):
            base = schedule(steps, "dpmsolver++")
            if cached is not None:
                assert base == cached - 1, f"n={n}: a schedule of {steps} steps left the samp: graph of the previous one cached"
            prev = _three_calls(pair, runs, base, prev, f"n={n} {steps} steps", cfg=C_CFG)
            cached = _graphs(geng)
        for solver in ("sde-dpmsolver++", "dpmsolver++"):
            sde = solver.startswith("sde")
            base = schedule(N_STEPS, solver)
            assert base == cached - 1, f"n={n}: the switch to {solver} left the previous solver's graph cached"
            for r in runs:                                     # the entry point of the other solver: refused, nothing cached
                with pytest.raises(EngineError, match="deterministic" if not sde else "stochastic"):
                    r.call(cfg=C_CFG, sde=not sde)
            assert _graphs(geng) == base
            prev = _three_calls(pair, runs, base, prev, f"n={n} {solver}", cfg=C_CFG, sde=sde)
            cached = _graphs(geng)
        assert cached == g0 + 1
    finally:
        for s in pair:
            s.eng.sync()
            s.eng.set_num_steps(N_STEPS)
    _clean(pair)


# ------------------------------------------------------------------------------------------------ (d) replays after an upload
def _fresh(orig, seed):
    """a fresh bf16-representable draw with the shape, mean and spread of `orig`"""
    o = orig.float()
    return synth.bf16_round(torch.randn(o.shape, generator=torch.Generator().manual_seed(seed)) * o.std() + o.mean())


def upload_set(s):
    """engine name -> new value: one parameter of each kind vv_upload distinguishes, in each family a cached graph reads"""
    d = s.lmcfg.head_dim
    inv_freq = 1.0 / (s.lmcfg.theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
    wobble = 0.5 + torch.rand(inv_freq.shape, generator=torch.Generator().manual_seed(6300))
    src = {"lm.layers.1.mlp.down_proj.weight": s.lm_w["layers.1.mlp.down_proj.weight"],                         # packed LM matrix
           "lm.layers.0.input_layernorm.weight": s.lm_w["layers.0.input_layernorm.weight"],                     # LM norm vector
           "lm.layers.0.self_attn.q_proj.bias": s.lm_w["layers.0.self_attn.q_proj.bias"],                       # a third of the QKV bias
           "head.layers.0.ffn.gate_proj.weight": s.head_w["layers.0.ffn.gate_proj.weight"],                     # head layer matrix
           "head.t_embedder.mlp.0.weight": s.head_w["t_embedder.mlp.0.weight"],                                 # the table set_schedule derives
           "dec.stages.0.1.ffn.linear2.weight": s.ac_w["decoder.stages.0.1.ffn.linear2.weight"],                # codec pointwise matrix
           "dec.stages.0.0.mixer.conv.conv.conv.weight": s.ac_w["decoder.stages.0.0.mixer.conv.conv.conv.weight"]}   # depthwise filter
    new = {k: _fresh(v, 6301 + i) for i, (k, v) in enumerate(src.items())}
    new["lm.rope.inv_freq"] = synth.bf16_round(inv_freq * wobble)           # the (cos, sin) table is rebuilt in place
    return new


def test_replays_after_an_upload(monkeypatch):
    """Four graphs cached on an xsplit-1 engine: lm: with 2 decode rows (three steps), lm: with a 3-row span of one cache (the
    split + merge route, whose rope/append reads inv_freq itself), samp: (n = 1) and chain: (slot 0).  Then Engine.upload replaces
    eight parameters on both engines, one of each kind vv_upload distinguishes (upload_set).  Uploads are in place -- no pointer of a
    captured launch moves -- so no lm: or chain: graph may be dropped (vv_stat(1) stays at +4); the t-embedder upload makes
    Engine.upload forget the step count, and the re-issued set_num_steps drops the samp: graph (+3), which the next calls capture
    again (+4).  Three more calls of each family at the same positions: equal to the eager engine, and moved by the new weights."""
    pair = _pair(1, monkeypatch)
    s0 = pair[1]
    cfg = s0.lmcfg
    gk = torch.Generator().manual_seed(6400)
    lens = (10, 40)
    kv = [tuple(torch.randn(cfg.layers, cfg.kv_heads, n, cfg.head_dim, generator=gk).to(torch.bfloat16) for _ in "kv") for n in lens + (20,)]
    g = synth.Gen(6401)
    x2h, x3h = g.normal((2, H), 1.0, mat=False), g.normal((ls.REPLAY_SPAN, H), 1.0, mat=False)
    lat = _latents(1, 6402)
    sides = []
    for s in pair:
        e = s.eng
        e.sync()
        e.set_speech_factors(*FACTORS)
        with torch.cuda.stream(e.stream):
            for c, (k, v) in enumerate(kv):
                for layer in range(cfg.layers):
                    e.kv_import_at(c, layer, 0, k[layer].to(e.device), v[layer].to(e.device))
        sides.append(dict(eng=e, x2=_dev(e, x2h), h2=_new(e, 2, H), x3=_dev(e, x3h), h3=_new(e, ls.REPLAY_SPAN, H),
                          samp=_Sampler(e, 1, 6403, cond_std=1.0), codec=_Codec(e, (0,), lat)))
    geng = pair[0].eng

    def round_of_calls(b):
        """three calls of each family -> per call [decode rows, span rows, latents, audio, semantic]"""
        e, outs = b["eng"], []
        b["codec"].reset()
        for step in range(3):
            with torch.cuda.stream(e.stream):
                e.lm_forward([(c, n + step) for c, n in enumerate(lens)], b["x2"], b["h2"])
                e.lm_forward_span(2, 20, ls.REPLAY_SPAN, b["x3"], b["h3"])
            e.sync()
            outs.append([b["h2"].cpu(), b["h3"].cpu(), b["samp"].call(1.3), *b["codec"].call("chain")])
        return outs
    names = ("lm: 2 decode rows", "lm: 3-row span", "samp:", "chain: audio", "chain: semantic")
    g0 = _fresh_schedule(pair)
    pre = [round_of_calls(b) for b in sides]
    for step in range(3):
        for k, nm in enumerate(names):
            _same(pre[0][step][k], pre[1][step][k], None, f"before the upload, call {step}, {nm}")
    assert _graphs(geng) == g0 + 4, (_graphs(geng), g0)
    new = upload_set(s0)
    for s in pair:
        e = s.eng
        e.sync()
        exp = e.expected_weights()
        for name, t in new.items():
            assert exp[name] == t.numel(), name
            e.upload(name, t)
    assert _graphs(geng) == g0 + 4, "an upload dropped a graph: uploads are in place, every captured pointer is still right"
    for s in pair:
        s.eng.set_num_steps(N_STEPS)                    # Engine.upload("head. ...") forgot the step count: the table is rebuilt
    assert _graphs(geng) == g0 + 3, "the re-issued schedule must drop the samp: graph"
    try:
        post = [round_of_calls(b) for b in sides]
        for step in range(3):
            for k, nm in enumerate(names):
                what = f"after the upload, call {step}, {nm}"
                _moved(post[1][step][k], pre[1][step][k], what)
                _same(post[0][step][k], post[1][step][k], pre[0][step][k], what)
        assert _graphs(geng) == g0 + 4, (_graphs(geng), g0)
    finally:
        old = {"lm." + k: v for k, v in s0.lm_w.items()}
        old.update({"head." + k: v for k, v in s0.head_w.items()})
        old.update({"dec." + k[len("decoder."):]: v for k, v in s0.ac_w.items() if k.startswith("decoder.")})
        d = cfg.head_dim
        old["lm.rope.inv_freq"] = 1.0 / (cfg.theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
        for s in pair:                                  # the engines are shared by the module: the other tests' weights come back
            s.eng.sync()
            for name in new:
                s.eng.upload(name, old[name])
            s.eng.set_num_steps(N_STEPS)
    _clean(pair)


# ------------------------------------------------------------------------------------------------ (e) lm: and the row table
REPLAY_GRAPHS = {"one": 2, "short+long": 2, "block-edge": 1, "6": 1, "16": 1}      # on keys no earlier case has shown the engine
_lm_bufs = {}


def _lm_buffers(eng, n_rows):
    """ONE x / hidden buffer per engine and row count: the cases with two rows share a key"""
    key = (id(eng), n_rows)
    if key not in _lm_bufs:
        _lm_bufs[key] = (_new(eng, n_rows, H), _new(eng, n_rows, H))
    return _lm_bufs[key]


@pytest.mark.parametrize("case", list(ls.REPLAY_ROWS))
@pytest.mark.parametrize("xs", [1, 3])
def test_lm_replays_follow_the_row_table(xs, case, monkeypatch):
    """Decode rows on a graph engine with one x / hidden buffer per row count: the rows' caches and positions are read from the row
    table on the device, the split count of the attention is a key field (tests/lm_shapes.py REPLAY_ROWS / REPLAY_SPLITS;
    test_pass_plan_cpu.py asserts the routes and the split count of every step).  Caches hold random bf16 K/V up to each starting
    length; x is rewritten in place before every step.  Every step equals the eager engine bit for bit, and a key is captured at its
    second sight, never again: vv_stat(1) is followed call by call, and on a fresh engine rises by REPLAY_GRAPHS[case] --
      one         2: positions 1021 .. 1023 of cache 0 (one split), 1024 .. 1027 (two splits, the merge kernel joins the graph), then
                  positions 0 .. 2 of cache 1 with the same buffers replay the one-split graph
      short+long  2: a row at 5 beside one crossing 1024 -- the short row rides in a two-split launch, the merge kernel skips it
      block-edge  1 (0 after short+long: the same key): rows crossing positions 32 and 64, the block edge of the V layout and of the
                  owner split
      6, 16       1 each: the packed batch route in the bf16 mode, the attention writing the packed o-projection operand in the graph"""
    pair = _pair(xs, monkeypatch)
    cfg = pair[1].lmcfg
    steps, splits = ls.REPLAY_ROWS[case], ls.REPLAY_SPLITS[case]
    n_rows = len(steps[0])
    starts = {}
    for rows in steps:
        for c, p in rows:
            starts.setdefault(c, p)
    gk = torch.Generator().manual_seed(6500 + n_rows)
    kv = {c: tuple(torch.randn(cfg.layers, cfg.kv_heads, n, cfg.head_dim, generator=gk).to(torch.bfloat16) for _ in "kv")
          for c, n in starts.items() if n > 0}
    for s in pair:
        e = s.eng
        e.sync()
        with torch.cuda.stream(e.stream):
            for c, (k, v) in kv.items():
                for layer in range(cfg.layers):
                    e.kv_import_at(c, layer, 0, k[layer].to(e.device), v[layer].to(e.device))
    geng = pair[0].eng
    sights = _sights.setdefault(id(geng), {})
    fresh = not any((n_rows, S) in sights for S in set(splits))
    g0 = expect = _graphs(geng)
    g = synth.Gen(6510 + n_rows)
    prev = None
    for step, (rows, S) in enumerate(zip(steps, splits)):
        xh = g.normal((n_rows, H), 1.0, mat=False)
        outs = []
        for s in pair:
            e = s.eng
            x, hid = _lm_buffers(e, n_rows)
            _put(e, x, xh)
            with torch.cuda.stream(e.stream):
                e.lm_forward(rows, x, hid)
            e.sync()
            outs.append(hid.cpu())
        what = f"xs{xs} {case} step {step} rows {rows[:2]}{'...' if n_rows > 2 else ''}"
        sights[(n_rows, S)] = sights.get((n_rows, S), 0) + 1
        expect += sights[(n_rows, S)] == 2
        assert _graphs(geng) == expect, (what, _graphs(geng), expect)
        assert bool(torch.isfinite(outs[1]).all()), what
        if prev is not None:
            _moved(outs[1], prev[1], what)
        _same(outs[0], outs[1], prev[0] if prev is not None else None, what)
        prev = outs
    if fresh:
        assert expect - g0 == REPLAY_GRAPHS[case], (case, expect - g0)
    _clean(pair)


# ------------------------------------------------------------------------------------------------ (f) warmup(), then the real factors
def test_warmup_before_the_speech_factors_leaves_no_stale_graph(monkeypatch):
    """A model whose speech factors are unset (NaN) is warmed up: warmup() installs (1.0, 0.0) in the engine and generates three
    frames, so the tokenizer chain's graph reaches its second sight and is captured dividing by 1.0; then set_speech_factors installs
    the real factors (load_state_dict does the same), and a one-utterance forced generate() with four diffusion frames runs on the
    buffers the warm-up used.  It must match the oracle loop (run_both / check of test_gpu_generate.py) and, bit for bit, the same
    generate() on a second model that never warmed up.  The first GPU run of warmup() in the suite."""
    import test_gpu_generate as tg
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference as Model
    forced = [[tg.D, tg.D, tg.D, tg.D, tg.X]]
    warm = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=512, use_graph=True)
    cold = build_small(synth.LMCfg(), xsplit=3, n_slots=1, max_ctx=512, use_graph=True)
    try:
        seen = {}
        plain = Model.set_speech_factors

        def warm_up_first(self, scaling, bias):
            """run_both's model, at the point where it installs the factors: still NaN there, so warmup() runs unscaled"""
            assert self._scaling != self._scaling
            self.warmup(voice_frames=2)
            assert self._scaling != self._scaling, "warmup() must leave the model's factors unset"
            seen["graphs"] = self.engine.stat(1)
            plain(self, scaling, bias)
        with monkeypatch.context() as mp:
            mp.setattr(Model, "set_speech_factors", warm_up_first)
            ow, hw = tg.run_both(warm, 1, forced, with_speech=True)
        assert seen["graphs"] > 0, "warmup() cached no graph: the sequence under test did not happen"
        oc, hc = tg.run_both(cold, 1, forced, with_speech=True)
        assert hc[0].speech_outputs[0].shape[-1] == 4 * 3200
        tg.check(oc, hc)
        aw, ac = hw[0].speech_outputs[0].float().cpu(), hc[0].speech_outputs[0].float().cpu()
        stale = "" if torch.equal(aw, ac) else f"; warmed-up model vs fresh model, waveform rel-L2 {rel_err(aw, ac):.3e}"
        try:
            tg.check(ow, hw)
        except AssertionError as err:
            raise AssertionError(f"generate() after warmup() + set_speech_factors misses the oracle ({err}){stale}") from err
        assert torch.equal(hw[0].sequences.cpu(), hc[0].sequences.cpu())
        assert torch.equal(aw, ac), stale
        assert len(hw[1].latents) == len(hc[1].latents) == 4
        for a, b in zip(hw[1].latents, hc[1].latents):
            assert torch.equal(a.cpu(), b.cpu()), rel_err(a, b)
        for s in (warm, cold):
            s.eng.sync()
            assert s.eng.stat(1) > 0 and s.eng.stat(4) == 0 and s.eng.stat(5) == 0
    finally:
        warm.eng.close()
        cold.eng.close()
