"""CPU tests of the per-request seed in the host loops: generate / generate_continuous / generate_interleaved / the queued batch and
the streaming class, through the oracle-backed fake engines (no noise_rows entry: the model falls back to vibevoice_amd/noise.py on
the host).  Under test: which counters travel with which request when rows are admitted, retire, diffuse in subsets and guess wrong,
that a request's draws are the same in any company, and that a call without a seed leaves the torch generators' path alone."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

import fake_engine
from test_dropin_cpu import TOK, _requests
from test_oracle_golden import G as GOLD, _oracle_small, _oracle_streaming_small
from vibevoice_amd import modeling, noise

CFGD = {"decoder_config": {"max_position_embeddings": 4096}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
        "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
D, E, S, X = TOK.speech_diffusion_id, TOK.speech_end_id, TOK.speech_start_id, TOK.eos_token_id
VALID = [S, E, D, X]                   # the order _session hands the engine (no bos id)
SEED_A = 0x9e3779b97f4a7c15
GREEDY = {"do_sample": False}


@pytest.fixture(autouse=True)
def _one_blas_thread():
    """exact comparisons of two runs of the same arithmetic: the CPU BLAS's summation order depends on its thread count and timing"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _trace():
    return types.SimpleNamespace(pos_hidden=[], neg_hidden=[], latents=[], semantic=[], next_embeds=[], tokens=[], logits=[], noise=[])


def _model(n_slots=2):
    eng = fake_engine.FakeEngine(_oracle_small(), n_slots=n_slots)
    assert not hasattr(eng, "noise_rows")
    m = modeling.VibeVoiceForConditionalGenerationInference(CFGD, eng, model_dtype=torch.float32)
    m.set_speech_factors(0.2, -0.05)
    m.set_ddpm_inference_steps(5)
    m.concurrent_codecs = False
    return m, eng


def _reqs(n, seed, seeds):
    """the forced-plan requests of test_dropin_cpu without their injected noise, each with its own seed (None: no "seed" key)"""
    out = []
    for r, sd in zip(_requests(n, seed), seeds):
        r = {k: v for k, v in r.items() if k != "_noise_fn"}
        if sd is not None:
            r["seed"] = sd
        out.append(r)
    return out


def _alone(m, r, trace=None, gen_cfg=GREEDY, **kw):
    forced = {"_forced_tokens": [r["_forced_tokens"]]} if "_forced_tokens" in r else {}
    return m.generate(input_ids=r["input_ids"], attention_mask=r["attention_mask"], cfg_scale=1.3, tokenizer=TOK, generation_config=gen_cfg,
                      show_progress_bar=False, seed=r.get("seed"), _trace=trace, **forced, **kw)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def _start_noise(seed, t):
    return noise.normals(seed, t, 1, noise.STREAM_START, 1, 0, 64)[0, 0]


def _noise_of(trace, idx):
    return [(t, row) for i, t, row in trace.noise if i == idx]


def _check_noise(trace, idx, seed, n_frames):
    got = _noise_of(trace, idx)
    assert [t for t, _ in got] == list(range(n_frames)), [t for t, _ in got]
    for t, row in got:
        assert torch.equal(row, _start_noise(seed, t)), t


def test_a_seeded_request_is_repeatable_in_any_company(monkeypatch):
    """Request A (seed s, a forced plan with a <speech_end> / <speech_start> turn) alone through generate(), first and last of three
    seeded requests through two slots of generate_continuous(), through one slot, and through generate_interleaved(lanes=2): the start
    noise of its t-th accepted latent is noise.normals(s, t, ...) bit for bit every time, its waveform agrees with the run alone within
    the 1e-5 of the queued-vs-alone tests (the CPU BLAS blocks a 2-row matmul differently) and exactly through one slot.  (Exactly:
    against the run alone on an engine in the same state -- the oracle-backed tokenizers treat a slot's zeroed conv history and an
    absent one with different, equivalent arithmetic, 6e-7 apart, so the request that comes last through one slot is compared with
    the second of two runs alone on one engine.)"""
    b, a, c = _reqs(3, 3, [11, SEED_A, 2 ** 64 - 1])      # A: the 8-token plan D E S D D D D X
    n_frames = a["_forced_tokens"].count(D)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(torch.cuda, "set_device", lambda *x, **k: None)
        m, _ = _model(1)
        tr = _trace()
        solo = _alone(m, a, tr)
        solo_used_slot = _alone(m, a)
        assert _rel(solo_used_slot.speech_outputs[0], solo.speech_outputs[0]) <= 1e-5
        _check_noise(tr, 0, SEED_A, n_frames)
        assert solo.speech_outputs[0].shape[-1] == n_frames * 3200
        for order, ia in (([a, b, c], 0), ([b, c, a], 2)):
            m, _ = _model(2)
            tr = _trace()
            outs = m.generate_continuous(order, tokenizer=TOK, generation_config=GREEDY, cfg_scale=1.3, _trace=tr)
            assert m.last_stats["max_in_flight"] == 2
            _check_noise(tr, ia, SEED_A, n_frames)
            for i, r in enumerate(order):                  # the others draw from their own seeds
                _check_noise(tr, i, r["seed"], r["_forced_tokens"].count(D))
            assert torch.equal(outs[ia].sequences.cpu(), solo.sequences.cpu())
            assert _rel(outs[ia].speech_outputs[0], solo.speech_outputs[0]) <= 1e-5
            m, _ = _model(2)
            one = m.generate_continuous(order, tokenizer=TOK, generation_config=GREEDY, cfg_scale=1.3, max_concurrent=1)
            assert torch.equal(one[ia].speech_outputs[0], (solo if ia == 0 else solo_used_slot).speech_outputs[0])
        m, _ = _model(2)
        lanes = m.generate_interleaved([b, c, a, dict(b, seed=5)], lanes=2, tokenizer=TOK, generation_config=GREEDY, cfg_scale=1.3)
        assert m.last_stats["lanes"] == 2
        m.close_lanes()
        assert torch.equal(lanes[2].sequences.cpu(), solo.sequences.cpu())
        assert _rel(lanes[2].speech_outputs[0], solo.speech_outputs[0]) <= 1e-5
        # another seed is another take
        m, _ = _model(1)
        other = _alone(m, dict(a, seed=SEED_A + 1))
        assert _rel(other.speech_outputs[0], solo.speech_outputs[0]) > 1e-2


def _replay(rows, seed, temperature=1.0):
    """tokens from the recorded per-step score rows of ONE request: u = noise.uniform(seed, k), inverse CDF of the float64 softmax"""
    toks = []
    for k, row in enumerate(rows):
        sc = (row / temperature).numpy() if temperature != 1.0 else row.numpy()
        toks.append(VALID[noise.choose(sc, noise.uniform(seed, k))])
        if toks[-1] == X:
            break
    return toks


@pytest.mark.parametrize("gen_cfg", [{"do_sample": True, "top_k": 0}, {"do_sample": True, "top_k": 0, "temperature": 0.7},
                                     {"do_sample": True, "top_k": 300, "temperature": 0.9, "repetition_penalty": 1.1}])
def test_sampled_tokens_come_from_the_requests_own_uniforms(monkeypatch, gen_cfg):
    """do_sample: the k-th token of a seeded request is the inverse CDF of the float64 softmax over its valid-id scores at
    u = noise.uniform(seed, k) -- replayed here from the traced logits (plain / temperature) or from the processors' output (top-k of
    the whole vocabulary + repetition penalty) --
    and the same alone and queued behind other sampled requests; the torch generators are not touched."""
    base = _reqs(3, 21, [28, 3, 4])           # seed 28: six tokens under all three settings, frames among them
    for r in base:
        del r["_forced_tokens"]
    a = base[0]
    warp = "repetition_penalty" in gen_cfg
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(1)
        seen = []
        if warp:
            plain = m._full_vocab_scores
            m._full_vocab_scores = lambda hidden, order, S: seen.append(plain(hidden, order, S)) or seen[-1]
        tr = _trace()
        torch.manual_seed(1)
        state = torch.get_rng_state()
        solo = _alone(m, a, tr, gen_cfg=gen_cfg, max_new_tokens=12)
        assert torch.equal(torch.get_rng_state(), state)
        got = solo.sequences[0, a["input_ids"].shape[1]:].tolist()
        if warp:
            rows = [s[0, torch.tensor(VALID)] for s in seen]
            want = _replay(rows, 28)
        else:
            want = _replay([lg[0] for lg in tr.logits], 28, float(gen_cfg.get("temperature", 1.0)))
        assert got[:len(want)] == want and len(want) >= 4 and D in want, (got, want)
        assert all(t == X for t in got[len(want):])
        m, eng = _model(2)
        outs = m.generate_continuous([base[1], base[2], a], tokenizer=TOK, generation_config=gen_cfg, cfg_scale=1.3, max_new_tokens=12)
        assert outs[2].sequences[0, a["input_ids"].shape[1]:].tolist() == got[:len(want)]


def test_wrong_speculative_guesses_spend_nothing(monkeypatch):
    """A plan with <speech_end> right after a frame and a new <speech_start>, twice: the sampler is enqueued speculatively behind the LM
    pass and its latent discarded when the row does not diffuse.  t counts ACCEPTED latents only, so the later frames' noise is the
    reference's for their t."""
    plan = [D, E, S, D, E, S, D, D, X]
    r = dict(_reqs(1, 5, [77])[0], _forced_tokens=plan)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(1)
        m.speculate_sampling = True
        tr = _trace()
        out = _alone(m, r, tr)
        _check_noise(tr, 0, 77, 4)
        assert eng.calls["samples"] > 4, eng.calls          # guesses were made and thrown away
        m2, eng2 = _model(1)
        m2.speculate_sampling = False
        out2 = _alone(m2, r)
        assert eng2.calls["samples"] == 4
        assert torch.equal(out.speech_outputs[0], out2.speech_outputs[0])


def test_the_stochastic_solver_draws_its_step_noise_from_streams_1_to_n(monkeypatch):
    """sde-dpmsolver++ (installed through the noise_scheduler.from_config surface, as the gradio demo does): the variance noise of
    solver step i of the frame with counter t is noise.normals(s, t, 1, 1 + i, ...), for accepted and discarded sampler calls alike,
    and speculation stays on."""
    s = 2 ** 64 - 1
    plan = [D, D, E, S, D, X]
    r = dict(_reqs(1, 5, [s])[0], _forced_tokens=plan)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, eng = _model(1)
        sched = m.model.noise_scheduler
        m.model.noise_scheduler = sched.from_config(sched.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
        m.set_ddpm_inference_steps(5)
        calls = []
        plain = eng.diffusion_sample

        def rec(n, cond, nz, cfg_scale, latent_out, step_noise=None):
            calls.append((nz[:n].clone(), step_noise[:, :n].clone()))
            return plain(n, cond, nz, cfg_scale, latent_out, step_noise=step_noise)
        eng.diffusion_sample = rec
        tr = _trace()
        torch.manual_seed(2)
        state = torch.get_rng_state()
        _alone(m, r, tr)
        assert torch.equal(torch.get_rng_state(), state)
    _check_noise(tr, 0, s, 3)
    assert len(calls) > 3                                   # speculative calls among them
    seen_t = set()
    for nz, sn in calls:
        t = next(t for t in range(4) if torch.equal(nz[0], _start_noise(s, t)))
        seen_t.add(t)
        assert sn.shape == (5, 1, 64)
        assert torch.equal(sn[:, 0], noise.normals(s, t, 1, 1, 5, 0, 64)[:, 0])
        for i in range(5):
            assert torch.equal(sn[i, 0], noise.normals(s, t, 1, 1 + i, 1, 0, 64)[0, 0])
    assert seen_t >= {0, 1, 2}


def test_mixed_calls_and_argument_handling(monkeypatch):
    a, b, c = _reqs(3, 3, [SEED_A, None, 12])
    with fake_engine.cpu_cuda_shims(monkeypatch):
        # a mixed call: the unseeded request's seed is ONE randint on the CPU generator, nothing else is drawn from it
        m, _ = _model(2)
        tr = _trace()
        torch.manual_seed(5)
        m.generate_continuous([a, b, c], tokenizer=TOK, generation_config=GREEDY, cfg_scale=1.3, _trace=tr)
        after = torch.get_rng_state()
        torch.manual_seed(5)
        derived = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
        assert torch.equal(torch.get_rng_state(), after)
        _check_noise(tr, 1, derived, b["_forced_tokens"].count(D))
        _check_noise(tr, 0, SEED_A, a["_forced_tokens"].count(D))
        _check_noise(tr, 2, 12, c["_forced_tokens"].count(D))
        # no seed anywhere: the torch path, draw for draw.  The plan D D X alone costs randn(2, 64) at step 0, a speculative draw that
        # is kept at step 1 and one that is undone at step 2: two draws of [2, 64] on the CPU generator
        m, _ = _model(1)
        short = dict(b, _forced_tokens=[D, D, X])
        tr = _trace()
        torch.manual_seed(9)
        _alone(m, short, tr)
        after = torch.get_rng_state()
        torch.manual_seed(9)
        draws = [torch.randn(2, 64) for _ in range(2)]
        assert torch.equal(torch.get_rng_state(), after)
        assert [t for _, t, _ in tr.noise] == [0, 1]
        for (_, t, row), d in zip(tr.noise, draws):
            assert torch.equal(row, d[0])
        # one int for two rows is refused; a list takes one entry per row
        ids = torch.cat([a["input_ids"][:, :9], a["input_ids"][:, :9]])
        kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=TOK, generation_config=GREEDY, show_progress_bar=False,
                  _forced_tokens=[[D, X], [D, D, X]])
        m, _ = _model(2)
        with pytest.raises(ValueError, match="one seed per row"):
            m.generate(seed=7, **kw)
        with pytest.raises(ValueError, match="seed"):
            m.generate(seed=[7], **kw)
        with pytest.raises(ValueError, match="seed"):
            m.generate(seed=[7, -1], **kw)
        with pytest.raises(ValueError, match="seed"):
            m.generate_continuous([a, dict(b, seed=1.5)], tokenizer=TOK, generation_config=GREEDY)
        # a lock-step batch: every row draws from its own seed; a row's noise does not depend on its batch index
        tr = _trace()
        m.generate(seed=[7, 8], _trace=tr, **kw)
        _check_noise(tr, 0, 7, 1)
        _check_noise(tr, 1, 8, 2)
        tr = _trace()
        m.generate(seed=[8, 7], _trace=tr, **kw)
        _check_noise(tr, 0, 8, 1)
        _check_noise(tr, 1, 7, 2)


def test_an_all_seeded_queued_batch_raises_no_rng_order_warning(monkeypatch):
    """three rows on a two-slot engine go through the queue: the one-time UserWarning about draws consumed in queue order is for calls
    that draw from the shared generators -- not raised when every row carries a seed, still raised when one does not"""
    r = _reqs(1, 9, [None])[0]
    ids = torch.cat([r["input_ids"]] * 3)
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=TOK, generation_config=GREEDY, show_progress_bar=False,
              _forced_tokens=[[D, D, X]] * 3)
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(modeling, "_WARNED_QUEUED_RNG", False)
        m, _ = _model(2)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out = m.generate(seed=[1, 2, 1], **kw)
        assert not [w for w in rec if issubclass(w.category, UserWarning)], [str(w.message) for w in rec]
        assert _rel(out.speech_outputs[2], out.speech_outputs[0]) <= 1e-5         # the same request and seed, admitted at another time
        assert _rel(out.speech_outputs[1], out.speech_outputs[0]) > 1e-2
        with pytest.warns(UserWarning, match="queue order"):
            m.generate(seed=[1, None, 1], **kw)


def test_voice_draws_follow_the_seed_and_the_speaker_index(monkeypatch):
    """the voice-sample latents of a seeded request: r2 = stream 0x80000001 (t = frame, aux = speaker), r1 = normal 0 of quad 0 of
    stream 0x80000002 (aux = speaker), both std_dist_type branches; the torch generators are not touched"""
    wav = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 3 * 3200)).astype(np.float32)) * 0.1
    masks = torch.ones(2, 3, dtype=torch.bool)
    s = 31337
    with fake_engine.cpu_cuda_shims(monkeypatch):
        m, _ = _model(1)
        mean, _ = m._process_speech_inputs(wav, masks, prefill_noise=(torch.zeros(2), torch.zeros(2, 3, 64)))
        torch.manual_seed(4)
        state = torch.get_rng_state()
        feats, emb = m._process_speech_inputs(wav, masks, seeds=[(s, 0), (s, 1)])
        assert torch.equal(torch.get_rng_state(), state)
        r1 = torch.stack([noise.normals(s, 0, 1, noise.STREAM_VOICE_SCALE, 1, k, 4)[0, 0, 0] for k in range(2)])
        r2 = torch.cat([noise.normals(s, 0, 3, noise.STREAM_VOICE, 1, k, 64) for k in range(2)])
        lat = mean / 0.2 + 0.05 + (r1 * (0.5 / 0.8))[:, None, None] * r2
        assert torch.allclose(feats, (lat - 0.05) * 0.2, rtol=1e-5, atol=1e-6)
        assert emb.shape[0] == 6
        # the second speaker alone under index 1 draws what it drew as the second of two
        f1, _ = m._process_speech_inputs(wav[1:], masks[1:], seeds=[(s, 1)])
        assert torch.allclose(f1[0], feats[1], rtol=1e-5, atol=1e-6)
        m.std_dist_type = "fix"
        ffix, _ = m._process_speech_inputs(wav, masks, seeds=[(s, 0), (s, 1)])
        assert torch.allclose(ffix, (mean / 0.2 + 0.05 + 0.5 * r2 - 0.05) * 0.2, rtol=1e-5, atol=1e-6)


def test_streaming_class_takes_a_seed(monkeypatch):
    """generate(seed=s) of the streaming class: two runs agree exactly, another seed is another take, the CPU generator is not touched"""
    from vibevoice_amd.modeling_streaming import VibeVoiceStreamingForConditionalGenerationInference
    z = np.load(os.path.join(GOLD, "streaming_text3_cap20.npz"))

    def branch(tag):
        n = int(z[f"{tag}_layers"])
        kv = [(torch.from_numpy(z[f"{tag}_k{li}"])[None], torch.from_numpy(z[f"{tag}_v{li}"])[None]) for li in range(n)]
        hid = torch.zeros(1, kv[0][0].shape[2], 128)
        hid[0, -1] = torch.from_numpy(z[f"{tag}_last"])
        return types.SimpleNamespace(past_key_values=kv, last_hidden_state=hid)
    pre = {"lm": branch("lm"), "tts_lm": branch("tts"), "neg_lm": None, "neg_tts_lm": branch("neg_tts")}
    with fake_engine.cpu_cuda_shims(monkeypatch):
        eng = fake_engine.FakeStreamingEngine(_oracle_streaming_small(eos_bias=None), 1, 2)
        cfgd = {"decoder_config": {"max_position_embeddings": 512}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                "tts_backbone_num_hidden_layers": 2}
        m = VibeVoiceStreamingForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
        m.set_speech_factors(0.2, -0.05)
        m.set_ddpm_inference_steps(5)
        outs, first = [], []
        plain = eng.diffusion_sample

        def rec(n, cond, nz, cfg_scale, latent_out):
            first.append(nz[0].clone())
            return plain(n, cond, nz, cfg_scale, latent_out)
        eng.diffusion_sample = rec
        torch.manual_seed(6)
        state = torch.get_rng_state()
        for sd in (39, 40, 40, 41):          # (the first run leaves the decoder's conv history zeroed instead of absent: see above)
            eng.caches = {0: eng.om.lm.new_cache(), 1: eng.om.tts_lm.new_cache(), 2: eng.om.tts_lm.new_cache()}
            n0 = len(first)
            outs.append(m.generate(tts_text_ids=torch.from_numpy(z["text"])[None], all_prefilled_outputs=pre, cfg_scale=1.5,
                                   max_new_tokens=int(z["max_new"]), seed=sd))
            for f, nz in enumerate(first[n0:]):
                assert torch.equal(nz, _start_noise(sd, f))
        assert torch.equal(torch.get_rng_state(), state)
        with pytest.raises(ValueError, match="seed"):
            m.generate(tts_text_ids=torch.from_numpy(z["text"])[None], all_prefilled_outputs=pre, seed=-3)
    assert outs[0].speech_outputs[0].numel() > 0
    assert torch.equal(outs[1].speech_outputs[0], outs[2].speech_outputs[0])
    assert _rel(outs[3].speech_outputs[0], outs[1].speech_outputs[0]) > 1e-2
