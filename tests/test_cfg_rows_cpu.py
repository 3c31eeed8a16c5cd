"""CPU tests of the per-request guidance scale in the host loops (generate / generate_continuous / the queued batch).

The numeric stages run through an oracle-backed fake engine whose sampler takes the per-row vector and hands it to
oracle.dpm.sample_speech_tokens as [n, 1]; what is under test is the host code: which scale travels with which condition row
when rows retire, get admitted and diffuse in subsets, the validation, and that a call with one scale keeps the float path."""
import pytest
import torch

import fake_engine
from oracle import dpm, head
from oracle import generate as ogen
from test_dropin_cpu import TOK, _requests
from test_oracle_golden import _oracle_small

OTOK = ogen.TokenIds(speech_start_id=TOK.speech_start_id, speech_end_id=TOK.speech_end_id, speech_diffusion_id=TOK.speech_diffusion_id,
                     eos_token_id=TOK.eos_token_id, bos_token_id=None, pad_token_id=TOK.pad_token_id)
CFGD = {"decoder_config": {"max_position_embeddings": 4096}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
        "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
SCALES = [1.0, 3.0, 0.0, 1.3]


class RowsFakeEngine(fake_engine.FakeEngine):
    """FakeEngine whose sampler accepts the per-row vector: every call is recorded as (n, cfg_scale as passed (a tensor is copied),
    the n positive condition rows)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.sampler_calls = []

    def diffusion_sample(self, n, cond, noise, cfg_scale, latent_out, step_noise=None):
        om = self.om
        if isinstance(cfg_scale, torch.Tensor):
            assert cfg_scale.shape == (n,) and cfg_scale.dtype == torch.float32
            self.sampler_calls.append((n, cfg_scale.clone(), cond[:n].clone()))
            cfg = cfg_scale.clone()[:, None]
        else:
            assert isinstance(cfg_scale, float)
            self.sampler_calls.append((n, cfg_scale, cond[:n].clone()))
            cfg = cfg_scale
        nz = torch.cat([noise[:n], noise[:n]])
        lat = dpm.sample_speech_tokens(lambda x, t, c: head.head_forward(om.head_w, x, t, c, om.head_layers, om.head_eps),
                                       cond[:n].clone(), cond[n:2 * n].clone(), cfg, self.n_steps, nz, om.t_cast_dtype)
        latent_out[:n] = lat
        self.calls["samples"] += 1


def _model(n_slots, eng_cls=RowsFakeEngine):
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    eng = eng_cls(_oracle_small(), n_slots=n_slots)
    m = VibeVoiceForConditionalGenerationInference(CFGD, eng, model_dtype=torch.float32)
    m.set_speech_factors(0.2, -0.05)
    m.set_ddpm_inference_steps(5)
    m.concurrent_codecs = False
    return m, eng


def _oracle_alone(r, cfg, trace=None):
    return ogen.oracle_generate(_oracle_small(), OTOK, r["input_ids"], r["attention_mask"], cfg_scale=cfg, num_steps=5,
                                noise_fn=r["_noise_fn"], forced_tokens=[r["_forced_tokens"]], trace=trace)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def _same_as_oracle(out, ref):
    oseq, oaud, omax = ref
    assert torch.equal(out.sequences.cpu(), oseq)
    assert torch.equal(out.reach_max_step_sample.cpu(), omax)
    assert out.speech_outputs[0] is not None and oaud[0] is not None
    assert out.speech_outputs[0].shape[-1] == oaud[0].shape[-1]
    assert _rel(out.speech_outputs[0][0], oaud[0][0]) <= 1e-5, _rel(out.speech_outputs[0][0], oaud[0][0])


def test_the_scales_are_told_apart_by_the_oracle():
    """precondition of everything below: one request under two of the scales gives waveforms more than 1e-1 apart"""
    r = _requests(4, 3)[0]
    a, b = _oracle_alone(r, 1.0), _oracle_alone(r, 3.0)
    assert _rel(a[1][0][0], b[1][0][0]) > 1e-1


def test_queue_rows_keep_their_own_scale(monkeypatch):
    """4 requests with distinct scales through 2 slots: forced plans of different lengths make rows retire and get admitted at
    different steps, <speech_end> steps leave a subset of the rows diffusing.  At every sampler call entry j of the vector is the
    scale of the utterance whose condition is row j, and every request ends as the oracle loop gives it alone under its own scale."""
    reqs = [dict(r, cfg_scale=c) for r, c in zip(_requests(4, 3), SCALES)]
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(2)
        outs = m.generate_continuous(reqs, tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=7.0)
    assert m.last_stats["max_in_flight"] == 2 and len(m.last_stats["admissions"]) == 4
    # whose condition is row j: the oracle loop on a request alone (under its own scale) goes through the positive hidden states the
    # request has in the queue, up to BLAS blocking -- so every recorded condition row is matched to the nearest of those rows
    solo_rows = []
    for i, (r, c, o) in enumerate(zip(reqs, SCALES, outs)):
        tr = ogen.Trace()
        _same_as_oracle(o, _oracle_alone(r, c, trace=tr))
        solo_rows += [(i, h[0]) for h in tr.pos_hidden]
    bank = torch.stack([row for _, row in solo_rows])
    sizes = set()
    for n, cs, cond in eng.sampler_calls:
        assert isinstance(cs, torch.Tensor), "a queue with mixed scales passes the vector"
        sizes.add(n)
        for j in range(n):
            d = (bank - cond[j]).norm(dim=1) / cond[j].norm()
            k = int(d.argmin())
            assert float(d[k]) <= 1e-4, float(d[k])
            assert float(cs[j]) == torch.tensor(SCALES[solo_rows[k][0]], dtype=torch.float32).item(), (j, cs.tolist(), solo_rows[k][0])
    assert sizes == {1, 2}, sizes           # full passes and passes where only a subset of the rows in flight diffuses


def test_generate_takes_one_scale_per_row(monkeypatch):
    """generate(cfg_scale=[...]) on a lock-step batch of 2, as list, tuple and tensor; equal values keep the float path"""
    reqs = _requests(2, 5)
    L = max(r["input_ids"].shape[1] for r in reqs)
    ids = torch.full((2, L), TOK.pad_token_id, dtype=torch.long)
    mask = torch.zeros((2, L), dtype=torch.long)
    for b, r in enumerate(reqs):
        n = r["input_ids"].shape[1]
        ids[b, L - n:] = r["input_ids"][0]
        mask[b, L - n:] = 1
    forced = [r["_forced_tokens"] for r in reqs]
    bank = {s: torch.cat([reqs[0]["_noise_fn"](s, 2)[:1], reqs[1]["_noise_fn"](s, 2)[:1]]) for s in range(16)}
    noise_fn = lambda step, n2: torch.cat([bank[step], bank[step]])[:n2]
    ref = ogen.oracle_generate(_oracle_small(), OTOK, ids, mask, cfg_scale=1.3, num_steps=5,
                               noise_fn=noise_fn, forced_tokens=forced)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        kw = dict(input_ids=ids, attention_mask=mask, tokenizer=TOK, generation_config={"do_sample": False}, _forced_tokens=forced,
                  _noise_fn=noise_fn, show_progress_bar=False)
        m, eng = _model(2)
        same = m.generate(cfg_scale=[1.3, 1.3], **kw)
        assert eng.sampler_calls and all(isinstance(cs, float) and cs == 1.3 for _, cs, _ in eng.sampler_calls)   # equal scales: the float
        assert torch.equal(same.sequences.cpu(), ref[0])
        for b in range(2):
            assert _rel(same.speech_outputs[b][0], ref[1][b][0]) <= 1e-5
        for form in ([1.0, 3.0], torch.tensor([1.0, 3.0]), (1.0, 3.0)):
            m, eng = _model(2)
            mixed = m.generate(cfg_scale=form, **kw)
            assert all(isinstance(cs, torch.Tensor) for _, cs, _ in eng.sampler_calls)
            assert any(n == 2 and cs.tolist() == [1.0, 3.0] for n, cs, _ in eng.sampler_calls)
            for b, c in enumerate([1.0, 3.0]):
                # row b of the mixed batch == row b of the oracle's batch under that one scale (rows do not interact)
                one = ogen.oracle_generate(_oracle_small(), OTOK, ids, mask, cfg_scale=c, num_steps=5,
                                           noise_fn=noise_fn, forced_tokens=forced)
                assert torch.equal(mixed.sequences.cpu()[b], one[0][b])
                assert _rel(mixed.speech_outputs[b][0], one[1][b][0]) <= 1e-5


def test_queued_batch_forwards_the_rows_scales(monkeypatch):
    """a batch above the engine's slots is decoded through the queue: _generate_queued puts each row's scale into its request"""
    reqs = _requests(3, 9)
    L = reqs[0]["input_ids"].shape[1]
    ids = torch.cat([reqs[0]["input_ids"]] * 3)
    mask = torch.ones_like(ids)
    forced = [reqs[0]["_forced_tokens"]] * 3
    scales = [1.0, 3.0, 0.0]
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(2)
        out = m.generate(input_ids=ids, attention_mask=mask, tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=scales,
                         _forced_tokens=forced, _noise_fn=reqs[0]["_noise_fn"], show_progress_bar=False)
    assert L == ids.shape[1] and len(out.speech_outputs) == 3
    for b, c in enumerate(scales):
        oseq, oaud, _ = _oracle_alone(reqs[0], c)
        assert torch.equal(out.sequences.cpu()[b, :oseq.shape[1]], oseq[0])
        assert _rel(out.speech_outputs[b][0], oaud[0][0]) <= 1e-5
    # the same prompt, plan and noise under three scales: the three waveforms differ
    assert _rel(out.speech_outputs[0][0], out.speech_outputs[1][0]) > 1e-1


def test_equal_scales_hand_the_engine_a_float(monkeypatch):
    """requests that all carry the same scale (as keys, or none and the call's argument) run today's path: a Python float"""
    base = _requests(3, 3)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        for reqs, call, want in (([dict(r, cfg_scale=2.0) for r in base], 1.0, 2.0), (base, 1.3, 1.3),
                                 ([dict(base[0], cfg_scale=1.3), base[1], base[2]], 1.3, 1.3)):
            m, eng = _model(2)
            m.generate_continuous(reqs, tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=call)
            assert eng.sampler_calls and all(isinstance(cs, float) and cs == want for _, cs, _ in eng.sampler_calls)
        # the stock fake engine (float only) still serves such a call: nothing but the float reaches it
        m, eng = _model(2, eng_cls=fake_engine.FakeEngine)
        m.generate_continuous(base, tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=1.3)


class _NoPrefill(RowsFakeEngine):
    def lm_forward(self, *a, **k):
        raise AssertionError("validation comes before any prefill")

    def embed(self, *a, **k):
        raise AssertionError("validation comes before any prefill")


@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [1.0, float("nan")], [float("inf"), 1.0], float("nan"), "1.3", [1.0, "2"],
                                 [1.0, None], None, [1.0, 2j], torch.ones(2, 1), torch.tensor([1.0, float("inf")]), [[1.0, 2.0]], [True, 1.0]])
def test_generate_refuses_a_bad_scale_before_any_prefill(monkeypatch, bad):
    reqs = _requests(2, 5)
    ids = torch.cat([reqs[0]["input_ids"], reqs[0]["input_ids"]])
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(2, eng_cls=_NoPrefill)
        with pytest.raises(ValueError, match="cfg_scale"):
            m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=TOK, cfg_scale=bad, show_progress_bar=False)
        m1, _ = _model(1, eng_cls=_NoPrefill)          # the queued path validates as early
        with pytest.raises(ValueError, match="cfg_scale"):
            m1.generate(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=TOK, cfg_scale=bad, show_progress_bar=False)


@pytest.mark.parametrize("bad", [float("nan"), float("-inf"), "3", [1.0, 2.0], 1j, torch.ones(2)])
def test_queue_refuses_a_bad_request_scale_before_any_prefill(monkeypatch, bad):
    base = _requests(3, 3)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
        m, eng = _model(2, eng_cls=_NoPrefill)
        reqs = [base[0], base[1], dict(base[2], cfg_scale=bad)]          # the LAST request is the bad one: nothing may start before it is seen
        with pytest.raises(ValueError, match="cfg_scale"):
            m.generate_continuous(reqs, tokenizer=TOK, cfg_scale=1.3)
        with pytest.raises(ValueError, match="cfg_scale"):
            m.generate_interleaved(reqs, lanes=2, tokenizer=TOK, cfg_scale=1.3)
        with pytest.raises(ValueError, match="cfg_scale"):
            m.generate_continuous(base, tokenizer=TOK, cfg_scale=bad)      # the call's default is held to the same rules


def test_numbers_of_every_real_kind_are_accepted():
    import numpy as np
    from vibevoice_amd.modeling import _cfg_scale_values
    assert _cfg_scale_values(2, 3, "t") == [2.0, 2.0, 2.0]
    assert _cfg_scale_values(np.float32(1.5), 2, "t") == [1.5, 1.5]
    assert _cfg_scale_values(torch.tensor(1.5), 2, "t") == [1.5, 1.5]
    assert _cfg_scale_values(np.array([1.0, 0.0]), 2, "t") == [1.0, 0.0]
    assert _cfg_scale_values([np.float64(1.0), 3, torch.tensor(0.5)], 3, "t") == [1.0, 3.0, 0.5]
    assert _cfg_scale_values(torch.tensor([1, 2]), 2, "t") == [1.0, 2.0]
