"""CPU tests of the prompt-prefix path (model.build_prompt_prefix, PromptPrefix, generate(prompt_prefix=...)): the product's host code --
which rows reuse how many positions, which voice samples are still encoded, what is refused -- over tests/fake_engine's oracle
arithmetic, with snapshot / restore implemented over the fake's own caches."""
import os

import numpy as np
import pytest
import torch

import fake_engine
from test_dropin_cpu import TOK, checkpoint_dir, tiny_reference_state_dict  # noqa: F401  (checkpoint_dir: fixture)
from test_oracle_golden import G as GOLD


class _SnapshotMixin:
    """Engine.kv_snapshot / kv_restore over the fake's oracle caches (k / v lists of [kvh, L, d]); counts encoder calls."""
    encoder_calls = 0

    def _set_geometry(self, layers, kv_heads, head_dim):
        self.cfg.lm_layers, self.cfg.lm_kv_heads, self.cfg.lm_head_dim = layers, kv_heads, head_dim

    def kv_snapshot(self, cache, n_pos):
        c = self.caches[cache]
        assert c.length >= n_pos
        return [t[:, :n_pos].clone() for t in c.k], [t[:, :n_pos].clone() for t in c.v]

    def kv_restore(self, cache, n_pos, k, v):
        assert n_pos <= self.max_ctx and all(t.shape[1] == n_pos for t in k)
        c = self.caches.setdefault(cache, self.om.lm.new_cache())
        c.k, c.v, c.length = [t.clone() for t in k], [t.clone() for t in v], n_pos

    def acoustic_encode(self, *a, **kw):
        self.encoder_calls += 1
        return super().acoustic_encode(*a, **kw)


class PrefixFakeEngine(_SnapshotMixin, fake_engine.LoadableFakeEngine):
    def __init__(self, ecfg, device=None):
        super().__init__(ecfg, device)
        self._set_geometry(ecfg.lm_layers, ecfg.lm_kv_heads, ecfg.lm_head_dim)


@pytest.fixture()
def model(monkeypatch, checkpoint_dir):  # noqa: F811
    from vibevoice_amd import modeling
    with fake_engine.cpu_cuda_shims(monkeypatch):
        monkeypatch.setattr(modeling, "Engine", PrefixFakeEngine)
        m = modeling.VibeVoiceForConditionalGenerationInference.from_pretrained(checkpoint_dir, torch_dtype=torch.float32, device_map="cuda")
        m.eval()
        m.set_ddpm_inference_steps(num_steps=5)
        yield m


def _inputs(z, rows=None):
    d = {k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "speech_tensors", "speech_masks", "speech_input_mask")}
    if rows is not None:                      # one batch row with its own voice sample (one sample per row in these files)
        d = {k: v[rows:rows + 1] for k, v in d.items()}
    return d


def _rel(a, b):
    return float((a.float().reshape(-1) - b.float().reshape(-1)).norm() / b.float().norm())


# ---------------------------------------------------------------- 1. reference goldens through the prefixed path
@pytest.mark.parametrize("name", ["generate_sampled_b1", "generate_norefresh_b1"])
def test_reference_golden_reproduced_through_a_prompt_prefix(model, name):
    """The goldens test_dropin_cpu.py replays unprefixed (recorded from the reference's own generate(), seeded), here as
    build_prompt_prefix + generate(prompt_prefix=...): seeded the same way, the prefix build takes the voice latents' two draws the
    reference's prefill takes, generate() then continues on the same generator -- sequences identical, waveform rel-L2 <= 1e-4 (that
    file's bound).  generate() itself does not touch the acoustic encoder and runs the LM over the prompt's tail only."""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    inputs = _inputs(z)
    forced = [z["forced"][0][:int(z["forced_len"][0])].tolist()] if z["forced"].size else None
    kw = dict(cfg_scale=1.3, tokenizer=TOK, verbose=False, is_prefill=True, show_progress_bar=False)
    if name == "generate_sampled_b1":
        kw.update(max_new_tokens=14, generation_config={"do_sample": True, "top_k": 0})
    else:
        kw.update(max_new_tokens=None, generation_config={"do_sample": False}, refresh_negative=False, _forced_tokens=forced)
    torch.manual_seed(int(z["seed"]))
    prefix = model.build_prompt_prefix(**inputs)
    assert prefix.n_pos == 5 and prefix.speech_pos == [3, 4] and prefix.ids == z["input_ids"][0][:5].tolist()
    assert model.engine.encoder_calls == 1
    out = model.generate(**inputs, prompt_prefix=prefix, **kw)
    assert model.engine.encoder_calls == 1                         # the voice sample was not encoded again
    assert model.last_stats["prefix_rows_reused"] == 5 and model.last_stats["prompt_rows_computed"] == 21 - 5
    assert torch.equal(out.sequences.cpu(), torch.from_numpy(z["sequences"]))
    assert torch.equal(out.reach_max_step_sample.cpu(), torch.from_numpy(z["reach_max"]))
    ref = torch.from_numpy(z["audio_0"])
    got = out.speech_outputs[0].reshape(-1)
    assert got.shape == ref.shape and _rel(got, ref) <= 1e-4
    # the voice inputs may be left out altogether: the prefix carries them
    torch.manual_seed(int(z["seed"]))
    model.build_prompt_prefix(**inputs)                            # same generator state as above
    out2 = model.generate(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"], prompt_prefix=prefix, **kw)
    assert torch.equal(out2.sequences.cpu(), out.sequences.cpu()) and _rel(out2.speech_outputs[0], out.speech_outputs[0]) <= 1e-6


# ---------------------------------------------------------------- 2. the host rules
def _b2_case():
    z = np.load(os.path.join(GOLD, "generate_norefresh_b2.npz"))
    forced = [z["forced"][b][:int(z["forced_len"][b])].tolist() for b in range(2)]
    g = torch.Generator().manual_seed(11)
    noise = (torch.randn(2, generator=g), torch.randn(2, 3, 64, generator=g))
    return z, forced, noise


def _run(model, inputs, forced, noise, **kw):
    torch.manual_seed(5)                                           # the diffusion noise of the loop
    return model.generate(**inputs, max_new_tokens=None, cfg_scale=1.3, tokenizer=TOK, generation_config={"do_sample": False}, verbose=False,
                          is_prefill=True, _forced_tokens=forced, _prefill_noise=noise, show_progress_bar=False, **kw)


def _same(a, b, rows):
    assert torch.equal(a.sequences.cpu(), b.sequences.cpu()) and torch.equal(a.reach_max_step_sample.cpu(), b.reach_max_step_sample.cpu())
    for r in range(rows):
        # one connector / LM call over fewer rows: the CPU BLAS blocks it differently (test_dropin_cpu's continuous-admission bound)
        assert a.speech_outputs[r].shape == b.speech_outputs[r].shape and _rel(a.speech_outputs[r], b.speech_outputs[r]) <= 1e-5


def _row_prefix(model, z, b, noise, **kw):
    return model.build_prompt_prefix(**_inputs(z, b), _prefill_noise=(noise[0][b:b + 1], noise[1][b:b + 1]), **kw)


def test_batch_of_two_list_single_and_none(model):
    """B = 2, a left-padded row among them: a list with one prefix per row, a list with None for a row (that row's voice sample is
    still encoded, and only it), and the lengths of the lists are checked."""
    z, forced, noise = _b2_case()
    base = _run(model, _inputs(z), forced, noise)
    assert model.last_stats["prefix_rows_reused"] == 0 and model.last_stats["prompt_rows_computed"] == 21 + 17
    p0, p1 = _row_prefix(model, z, 0, noise), _row_prefix(model, z, 1, noise)
    assert (p0.n_pos, p0.speech_pos) == (5, [3, 4]) and (p1.n_pos, p1.speech_pos) == (6, [3, 4, 5])      # unpadded positions
    n_enc = model.engine.encoder_calls
    out = _run(model, _inputs(z), forced, noise, prompt_prefix=[p0, p1])
    assert model.engine.encoder_calls == n_enc
    assert model.last_stats["prefix_rows_reused"] == 5 + 6 and model.last_stats["prompt_rows_computed"] == 16 + 11
    _same(out, base, 2)
    out = _run(model, _inputs(z), forced, noise, prompt_prefix=[p0, None])
    assert model.engine.encoder_calls == n_enc + 1                 # row 1's sample only
    assert model.last_stats["prefix_rows_reused"] == 5 and model.last_stats["prompt_rows_computed"] == 16 + 17
    _same(out, base, 2)
    with pytest.raises(ValueError, match="entries for 2 rows"):
        _run(model, _inputs(z), forced, noise, prompt_prefix=[p0])
    # one PromptPrefix for every row: row 1 does not start with it, and says where
    with pytest.raises(ValueError, match="position"):
        _run(model, _inputs(z), forced, noise, prompt_prefix=p0)
    one = _run(model, _inputs(z, 0), forced[:1], (noise[0][:1], noise[1][:1]), prompt_prefix=p0)      # single prefix, single row
    assert model.last_stats["prefix_rows_reused"] == 5
    assert torch.equal(one.sequences[0, :21 + len(forced[0])].cpu(), base.sequences[0, :21 + len(forced[0])].cpu())


def test_prompt_that_is_the_prefix_keeps_one_row_for_the_lm(model):
    z, forced, noise = _b2_case()
    inputs, nz = _inputs(z, 0), (noise[0][:1], noise[1][:1])
    base = _run(model, inputs, forced[:1], nz)
    whole = model.build_prompt_prefix(**inputs, _prefill_noise=nz, n_prefix=21)
    assert whole.n_pos == 21
    out = _run(model, inputs, forced[:1], nz, prompt_prefix=whole)
    assert model.last_stats["prefix_rows_reused"] == 20 and model.last_stats["prompt_rows_computed"] == 1
    _same(out, base, 1)


def test_row_with_speech_positions_beyond_the_prefix_is_prefilled_in_full(model):
    z, forced, noise = _b2_case()
    inputs, nz = _inputs(z, 0), (noise[0][:1], noise[1][:1])
    base = _run(model, inputs, forced[:1], nz)
    short = model.build_prompt_prefix(**inputs, _prefill_noise=nz, n_prefix=4)          # ends inside the voice block [3, 4]
    assert short.speech_pos == [3]
    n_enc = model.engine.encoder_calls
    out = _run(model, inputs, forced[:1], nz, prompt_prefix=short)
    assert model.engine.encoder_calls == n_enc + 1
    assert model.last_stats["prefix_rows_reused"] == 0 and model.last_stats["prompt_rows_computed"] == 21
    _same(out, base, 1)
    # a text-only prefix in front of the voice block is the same case
    text = model.build_prompt_prefix(inputs["input_ids"], n_prefix=3)
    _same(_run(model, inputs, forced[:1], nz, prompt_prefix=text), base, 1)
    assert model.last_stats["prefix_rows_reused"] == 0
    with pytest.raises(ValueError, match="n_prefix is required"):
        model.build_prompt_prefix(inputs["input_ids"])


def test_mismatch_and_stale_prefixes_are_refused(model):
    z, forced, noise = _b2_case()
    inputs, nz = _inputs(z, 0), (noise[0][:1], noise[1][:1])
    p = model.build_prompt_prefix(**inputs, _prefill_noise=nz)
    bad = dict(inputs)
    bad["input_ids"] = inputs["input_ids"].clone()
    bad["input_ids"][0, 2] += 1
    with pytest.raises(ValueError, match="position 2"):
        _run(model, bad, forced[:1], nz, prompt_prefix=p)
    bad = dict(inputs)
    bad["speech_input_mask"] = inputs["speech_input_mask"].clone()
    bad["speech_input_mask"][0, 3] = False                          # the same ids, another voice block
    with pytest.raises(ValueError, match="position 3"):
        _run(model, bad, forced[:1], nz, prompt_prefix=p)
    with pytest.raises(TypeError):
        _run(model, inputs, forced[:1], nz, prompt_prefix="voice-a")
    # parameters change -> every prefix built before is refused, by each of the three ways in
    e0 = model.weights_epoch
    sd = tiny_reference_state_dict()
    key = "model.language_model.layers.0.self_attn.q_proj.weight"
    model.load_state_dict({key: sd[key]}, strict=False)
    assert model.weights_epoch == e0 + 1
    with pytest.raises(RuntimeError, match="stale"):
        _run(model, inputs, forced[:1], nz, prompt_prefix=p)
    model.model.language_model.load_state_dict({key[len("model.language_model."):]: sd[key]}, strict=False)
    model.upload("lm.layers.0.self_attn.q_proj.weight", sd[key])
    assert model.weights_epoch == e0 + 3
    p2 = model.build_prompt_prefix(**inputs, _prefill_noise=nz)    # rebuilt under the current weights: accepted again
    _run(model, inputs, forced[:1], nz, prompt_prefix=p2)
    assert model.last_stats["prefix_rows_reused"] == 5


def test_request_dict_key_of_generate_continuous(model):
    """More requests than slots in flight: a prefix is restored into a slot another request has just left."""
    z, forced, noise = _b2_case()
    reqs = []
    for i in range(4):
        b = i % 2
        r = _inputs(z, b)
        r.update(_forced_tokens=forced[b], _prefill_noise=(noise[0][b:b + 1], noise[1][b:b + 1]))
        reqs.append(r)
    kw = dict(tokenizer=TOK, generation_config={"do_sample": False}, cfg_scale=1.3, max_concurrent=2)
    model.concurrent_codecs = False
    torch.manual_seed(9)
    base = model.generate_continuous(reqs, **kw)
    assert model.last_stats["prefix_rows_reused"] == 0
    pf = [_row_prefix(model, z, b, noise) for b in range(2)]
    n_enc = model.engine.encoder_calls
    torch.manual_seed(9)
    outs = model.generate_continuous([dict(r, prompt_prefix=pf[i % 2]) if i != 1 else r for i, r in enumerate(reqs)], **kw)
    assert model.engine.encoder_calls == n_enc + 1                  # request 1 carries no prefix
    assert model.last_stats["prefix_rows_reused"] == 5 + 5 + 6 and model.last_stats["prompt_rows_computed"] == 16 + 17 + 16 + 11
    assert [a[1] for a in model.last_stats["admissions"]] == [0, 1, 2, 3] and model.last_stats["max_in_flight"] == 2
    for a, b in zip(outs, base):
        _same(a, b, 1)
