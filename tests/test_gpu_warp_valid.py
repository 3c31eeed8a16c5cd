"""vv_lm_warp_valid (csrc/warp.hip: the full-vocabulary logits processors evaluated for the valid ids only) against tests/warp_ref.py --
bit-equal scores, identical removals and survivor counts -- and generate() with the processors on the device against the torch path.

Inputs stay BOUNDARY_MARGIN away from the top-p / min-p thresholds (asserted on every case): the kernel sums its masses as fp32
partials combined in fp64, warp_ref in fp64, torch in fp32 in sort order; AT a threshold the three need not agree."""
import types

import numpy as np
import pytest
import torch

import synth
import warp_ref as wr
from gpu_util import build_small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one small engine per vocabulary size, built on first use"""
    made = {}

    def get(V):
        if V not in made:
            made[V] = build_small(synth.LMCfg(vocab=V), xsplit=3, n_slots=2, max_ctx=256, tied=True).eng
        return made[V]
    yield get
    for e in made.values():
        e.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def launch(eng, logits, seen, valid, pad=1024, **kw):
    """logits [n, V] fp32 / seen [n, V] bool (numpy) -> (out [n, n_valid], survivors [n]) from the kernel.  The logits scratch
    continues with `pad` NaNs behind n * V and `out` is NaN before the call: nothing of either may show up in the result, and the
    kernel may not write behind its n * n_valid block."""
    n, V = logits.shape
    nv = len(valid)
    eng.set_valid_tokens(valid)
    with torch.cuda.stream(eng.stream):
        lg = torch.full((n * V + pad,), float("nan"), dtype=torch.float32, device=eng.device)
        lg[:n * V] = torch.from_numpy(logits.reshape(-1)).to(eng.device)
        sn = None
        if seen is not None:
            sn = torch.full((n * V + pad,), 1, dtype=torch.uint8, device=eng.device)
            sn[:n * V] = torch.from_numpy(seen.reshape(-1).astype(np.uint8)).to(eng.device)
        out = torch.full((n * nv + 16,), float("nan"), dtype=torch.float32, device=eng.device)
        surv = torch.full((n + 4,), -7, dtype=torch.int32, device=eng.device)
        eng.lm_warp_valid(n, lg, sn, out, surv, **kw)
    eng.sync()
    out, surv = out.cpu().numpy(), surv.cpu().numpy()
    assert np.isnan(out[n * nv:]).all() and (surv[n:] == -7).all()
    return out[:n * nv].reshape(n, nv), surv[:n]


def check(eng, logits, seen, valid, **kw):
    want, dist, want_surv = wr.warp_ref_rows(logits, seen, valid, **kw)
    assert dist.min() > wr.BOUNDARY_MARGIN, (kw, float(dist.min()))       # the precondition, on this test's own inputs
    got, surv = launch(eng, logits, seen if kw.get("repetition_penalty", 1.0) != 1.0 else None, valid, **kw)
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    assert np.array_equal(_bits(got), _bits(want)), (kw, got, want)
    assert np.array_equal(surv, want_surv), (kw, surv, want_surv)
    return got, want


def processor_sets(V):
    k = 5 if V < 2000 else 50
    return {
        "penalty": dict(do_sample=True, repetition_penalty=1.3),
        "temperature": dict(do_sample=True, temperature=0.7),
        "top_k": dict(do_sample=True, top_k=k),
        "top_p": dict(do_sample=True, top_p=0.9),
        "min_p": dict(do_sample=True, min_p=0.05),
        "top_k+top_p": dict(do_sample=True, top_k=k, top_p=0.9),
        "all": dict(do_sample=True, repetition_penalty=1.3, temperature=1.5, top_k=4 * k, top_p=0.99, min_p=0.002),
        "top_k>=V": dict(do_sample=True, top_k=V + 7, top_p=0.5),
        "top_k=1": dict(do_sample=True, top_k=1, min_p=0.3),
        "greedy+penalty": dict(do_sample=False, repetition_penalty=1.3, temperature=0.7, top_k=k, top_p=0.5, min_p=0.3),
    }


@pytest.mark.parametrize("V", [320, 1031, 4099])
def test_kernel_equals_the_reduction_form(engines, V):
    """every processor set at n = 5 rows, 4 valid ids.  V = 1031 and 4099 are odd: rows 1.. start off a 16-byte boundary and end in a
    tail; 4099 gives every thread more than one element (1024 threads x float4) and is prime."""
    eng = engines(V)
    removed = kept = 0
    for i, (name, kw) in enumerate(processor_sets(V).items()):
        logits, seen, valid = wr.make_case(100 * V + i, V, n_valid=4, scale=(1.0, 3.0, 6.0)[i % 3], n=5)
        got, _ = check(eng, logits, seen, valid, **kw)
        removed += int(np.isneginf(got).sum())
        kept += int(np.isfinite(got).sum())
    assert removed >= 10 and kept >= 10


@pytest.mark.parametrize("n,n_valid", [(1, 1), (1, 16), (16, 1), (16, 16), (5, 16), (16, 4)])
def test_kernel_row_and_valid_counts(engines, n, n_valid):
    eng = engines(1031)
    sets = processor_sets(1031)
    for i, name in enumerate(("all", "top_k+top_p", "top_k", "greedy+penalty")):
        logits, seen, valid = wr.make_case(5000 + 100 * n + 10 * n_valid + i, 1031, n_valid=n_valid, scale=3.0, n=n)
        check(eng, logits, seen, valid, **sets[name])


def test_kernel_at_the_real_vocabulary(engines):
    """V = 152064, n = 2 (1.2 MB of logits): the four select / mass passes at 149 elements per thread"""
    V = 152064
    logits, seen, valid = wr.make_case(77, V, n_valid=5, scale=3.0, n=2)
    got, _ = check(engines(V), logits, seen, valid, **processor_sets(V)["all"])
    assert np.isneginf(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("k,kept", [(5, (True, False, False)), (10, (True, False, False)), (12, (True, True, False)),
                                    (20, (True, True, False)), (21, (True, True, True))])
def test_kernel_top_k_boundary_on_ties(engines, k, kept):
    l, valid = wr.tie_case(320)
    got, _ = check(engines(320), l, None, valid, do_sample=True, top_k=k)
    assert tuple(np.isfinite(got[0])) == kept


def test_rows_do_not_interact_and_runs_repeat(engines):
    """row r of an n = 16 call equals the n = 1 call on that row, bit for bit; two runs of one call are bit-identical"""
    eng = engines(1031)
    kw = processor_sets(1031)["all"]
    logits, seen, valid = wr.make_case(424242, 1031, n_valid=7, scale=3.0, n=16)
    got, _ = check(eng, logits, seen, valid, **kw)
    again, _ = launch(eng, logits, seen, valid, **kw)
    assert np.array_equal(_bits(got), _bits(again))
    for r in range(16):
        one, surv = launch(eng, logits[r:r + 1], seen[r:r + 1], valid, **kw)
        assert np.array_equal(_bits(one[0]), _bits(got[r])), r
        assert surv[0] == np.isfinite(got[r]).sum()


def test_poisoned_tail_and_output(engines):
    """the logits scratch behind n * V and `out` before the call hold NaN, the seen bytes behind n * V are set: nothing non-finite
    appears except the -inf of removed tokens (launch() also checks that nothing behind the result block was written)"""
    eng = engines(4099)
    for name in ("all", "top_p", "top_k", "greedy+penalty"):
        logits, seen, valid = wr.make_case(31337, 4099, n_valid=6, scale=3.0, n=3)
        got, surv = launch(eng, logits, seen, valid, pad=8192, **{**processor_sets(4099)[name], "repetition_penalty": 1.3})
        assert (np.isfinite(got) | np.isneginf(got)).all(), name
        assert np.array_equal(surv, np.isfinite(got).sum(axis=1))


def test_refusals(engines):
    """each bad argument raises EngineError with its text, before any launch"""
    from vibevoice_amd.engine import EngineError
    eng = engines(320)
    V = 320
    eng.set_valid_tokens([3, 5, 7])
    lg, out = eng.new(17 * V), eng.new(17 * 16)
    sn, surv = eng.new(17 * V, dtype=torch.uint8), eng.new(17, dtype=torch.int32)
    before = eng.stat(0)                     # launches enqueued through this context
    for n, seen, kw, text in [
            (0, None, {}, r"n must be in \[1,16\]"),
            (17, None, {}, r"n must be in \[1,16\]"),
            (1, sn, dict(repetition_penalty=0.0), "repetition_penalty"),
            (1, sn, dict(repetition_penalty=-1.0), "repetition_penalty"),
            (1, None, dict(temperature=0.0, do_sample=True), "temperature"),
            (1, None, dict(top_k=-1, do_sample=True), "top_k"),
            (1, None, dict(top_p=1.5, do_sample=True), "top_p"),
            (1, None, dict(top_p=-0.1, do_sample=True), "top_p"),
            (1, None, dict(min_p=1.5, do_sample=True), "min_p"),
            (1, None, dict(min_p=-0.5, do_sample=True), "min_p"),
            (1, None, dict(repetition_penalty=1.2), "seen mask")]:
        with pytest.raises(EngineError, match=text):
            eng.lm_warp_valid(n, lg, seen, out, surv, **kw)
    eng.sync()
    assert not out.any() and not surv.any()                       # nothing ran
    assert eng.stat(0) == before
    # a context whose valid ids were never set
    fresh = eng.fork()
    try:
        with pytest.raises(EngineError, match="vv_set_valid_tokens"):
            fresh.lm_warp_valid(1, lg, None, out, surv)
    finally:
        fresh.close()
    # and the context still works
    eng.lm_warp_valid(1, lg, None, out, surv)
    eng.sync()
    assert int(surv[0]) == 3 and eng.stat(0) == before + 1


# ---------------------------------------------------------------------------------------------------------------- generate()
TOK = types.SimpleNamespace(speech_start_id=301, speech_end_id=302, speech_diffusion_id=303, eos_token_id=304, bos_token_id=None,
                            pad_token_id=305)
VALID_COLS = slice(301, 305)


@pytest.fixture(scope="module")
def sm():
    s = build_small(synth.LMCfg(), xsplit=3, n_slots=2, max_ctx=512)
    yield s
    s.eng.close()


def _generate(s, on_device, gen_cfg, lift, seed, record=None, max_new_tokens=10):
    """seeded generate() of a left-padded batch of two on the small engine.  lift: four values added to the valid columns of the full
    logits (the synthetic lm_head ranks them far below its top 5 of 320; both paths see the same lifted logits).  record: a list that
    receives (logits, seen, valid, kwargs) of every vv_lm_warp_valid call."""
    from test_gpu_generate import make_inputs
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = s.eng
    V = s.lmcfg.vocab
    ids, mask, sim, st, smk = make_inputs(s, 2, True, 61)
    g = synth.Gen(62)
    pre = (g.normal((2,), 1.0, mat=False), g.normal((2, 3, 64), 1.0, mat=False))
    bank = {}

    def noise_fn(step, n2):
        if (step, n2) not in bank:
            bank[(step, n2)] = synth.Gen(61 * 1000 + step).normal((n2, 64), 1.0, mat=False)
        return bank[(step, n2)]
    cfgd = {"decoder_config": {"max_position_embeddings": s.lmcfg.max_pos}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
            "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
    m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
    m.set_speech_factors(s.scaling, s.bias)
    m.set_ddpm_inference_steps(5)
    assert m.warp_on_device is True
    m.warp_on_device = on_device
    plain_full, plain_warp = eng.lm_logits_full, eng.lm_warp_valid

    def lm_logits_full(n, hidden, out):
        plain_full(n, hidden, out)
        out[:n * V].view(n, V)[:, VALID_COLS] += torch.tensor(lift, dtype=torch.float32, device=out.device)

    def lm_warp_valid(n, logits, seen, out, survivors, **kw):
        if record is not None:
            record.append((logits[:n * V].view(n, V).cpu().numpy().copy(),
                           None if seen is None else (seen[:n * V].view(n, V).cpu().numpy() != 0), list(eng._valid_ids), dict(kw)))
        plain_warp(n, logits, seen, out, survivors, **kw)
    eng.lm_logits_full, eng.lm_warp_valid = lm_logits_full, lm_warp_valid
    try:
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        return m.generate(input_ids=ids, attention_mask=mask, speech_tensors=st, speech_masks=smk, speech_input_mask=sim, cfg_scale=1.3,
                          tokenizer=TOK, max_new_tokens=max_new_tokens, generation_config=gen_cfg, _noise_fn=noise_fn, _prefill_noise=pre,
                          show_progress_bar=False)
    finally:
        del eng.lm_logits_full, eng.lm_warp_valid


@pytest.mark.parametrize("gen_cfg,lift", [
    ({"do_sample": True, "top_k": 5, "top_p": 0.9, "min_p": 0.01, "repetition_penalty": 1.2, "temperature": 0.8}, [4.0, 4.0, 4.0, 4.0]),
    ({"do_sample": False, "repetition_penalty": 1.3}, [4.0, 4.0, 4.0, 0.0])],       # greedy: <eos> not lifted, or the run ends at once
    ids=["sampled", "greedy-penalty"])
def test_generate_on_the_device_equals_the_torch_path(sm, gen_cfg, lift):
    """warp_on_device True against False, seeded, batch 2, _noise_fn fixed: equal sequences and bit-equal speech_outputs (the
    multinomial call is the same call on the same scores).  First, on the scores recorded at every step of the device run: no
    valid token within BOUNDARY_MARGIN of a filter threshold."""
    rec = []
    dev = _generate(sm, True, gen_cfg, lift=lift, seed=5, record=rec)
    assert rec
    for logits, seen, valid, kw in rec:
        _, dist, _ = wr.warp_ref_rows(logits, seen, valid, **kw)
        assert dist.min() > wr.BOUNDARY_MARGIN, float(dist.min())
    host = _generate(sm, False, gen_cfg, lift=lift, seed=5)
    assert dev.sequences.shape[1] - 21 >= 4                       # more than a step or two was compared
    assert torch.equal(dev.sequences.cpu(), host.sequences.cpu()), (dev.sequences.tolist(), host.sequences.tolist())
    for a, b in zip(dev.speech_outputs, host.speech_outputs):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "torch"])
def test_generate_reports_a_row_without_valid_tokens_on_both_paths(sm, on_device):
    """top_k = 1 on rows whose maximum is not a valid id (the synthetic lm_head, nothing lifted): every valid token is removed"""
    with pytest.raises(RuntimeError, match="removed every valid speech token"):
        _generate(sm, on_device, {"do_sample": True, "top_k": 1}, lift=[0.0] * 4, seed=5)
    sm.eng.sync()
