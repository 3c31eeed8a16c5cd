"""tests/warp_ref.py (the full-vocabulary logits processors as reductions, what vv_lm_warp_valid evaluates) against transformers' own
classes, and the host loop's device path (seen-set bookkeeping, row order) on the fake engine."""
import itertools
import os

import numpy as np
import pytest
import torch

import warp_ref as wr

pytest.importorskip("transformers")

TOP_K = (0, 1, 5, 50, 200, "V", "V+7")
TOP_P = (1.0, 0.5, 0.9, 0.99)
MIN_P = (0.0, 0.002, 0.05, 0.3)
PEN = (1.0, 1.3)
TEMP = (1.0, 0.7, 1.5)
PER_V = 44            # combinations drawn per vocabulary size: 3 x 44 rows x 4 valid tokens = 528 tokens


def _hf(l, seen, valid, pen, temp, top_k, top_p, min_p, stages=None):
    """the five transformers classes in HF's order on one row; stages (optional dict) records, per filter, the valid tokens' finite
    pattern before / after it"""
    from transformers.generation.logits_process import (MinPLogitsWarper, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    sc = torch.from_numpy(l)[None].clone()
    if pen != 1.0:
        sc = RepetitionPenaltyLogitsProcessor(pen)(torch.from_numpy(np.nonzero(seen)[0])[None], sc)
    if temp != 1.0:
        sc = TemperatureLogitsWarper(temp)(None, sc)
    for name, proc in (("top_k", TopKLogitsWarper(top_k) if top_k > 0 else None), ("top_p", TopPLogitsWarper(top_p) if top_p < 1.0 else None),
                       ("min_p", MinPLogitsWarper(min_p) if min_p > 0.0 else None)):
        if proc is None:
            continue
        before = torch.isfinite(sc[0, valid])
        sc = proc(None, sc)
        if stages is not None:
            after = torch.isfinite(sc[0, valid])
            stages.setdefault(name, [False, False])
            stages[name][0] |= bool((before & ~after).any())
            stages[name][1] |= bool((before & after).any())
    return sc[0, valid].numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def grid():
    """(V, case, settings) rows: PER_V combinations per vocabulary size, drawn once with a fixed seed from the full product"""
    combos = list(itertools.product(TOP_K, TOP_P, MIN_P, PEN, TEMP))
    rows = []
    for vi, V in enumerate((320, 1031, 152064)):
        g = np.random.default_rng(1000 + vi)
        for ci, c in enumerate(g.choice(len(combos), size=PER_V, replace=False)):
            tk, tp, mp, pen, temp = combos[int(c)]
            tk = V if tk == "V" else V + 7 if tk == "V+7" else tk
            logits, seen, valid = wr.make_case(7000 + 100 * vi + ci, V, n_valid=4, scale=(1.0, 3.0, 6.0)[ci % 3])
            rows.append((V, logits[0], seen[0], valid, dict(repetition_penalty=pen, temperature=temp, top_k=tk, top_p=tp, min_p=mp)))
    return rows


def test_reduction_form_equals_the_transformers_classes_on_the_grid(grid):
    """Surviving scores bit-equal, removals identical, for 528 valid tokens; every filter both removes and keeps a valid token somewhere
    in the grid; no token within BOUNDARY_MARGIN of a filter boundary (torch sums its masses in fp32 in sort order: at the
    boundary itself the two need not agree, so the inputs stay away from it)."""
    stages, n_tok, min_dist = {}, 0, np.inf
    for V, l, seen, valid, kw in grid:
        got, dist = wr.warp_ref(l, seen, valid, do_sample=True, **kw)
        want = _hf(l, seen, valid, kw["repetition_penalty"], kw["temperature"], kw["top_k"], kw["top_p"], kw["min_p"], stages)
        assert np.array_equal(_bits(got), _bits(want)), (V, kw, got, want)
        min_dist = min(min_dist, float(dist.min()))
        n_tok += len(valid)
    assert n_tok == 528
    assert min_dist > wr.BOUNDARY_MARGIN, min_dist
    for name in ("top_k", "top_p", "min_p"):
        assert stages[name] == [True, True], (name, stages[name])


@pytest.mark.parametrize("k,kept", [(5, (True, False, False)), (10, (True, False, False)), (12, (True, True, False)),
                                    (20, (True, True, False)), (21, (True, True, True))])
def test_top_k_boundary_on_ties(k, kept):
    """values 5 x 10, 3 x 10, 0 x 44: HF removes s < (k-th largest value), so a tie at the boundary survives as a whole"""
    l, valid = wr.tie_case()
    got, _ = wr.warp_ref(l[0], None, valid, do_sample=True, top_k=k)
    want = _hf(l[0], None, valid, 1.0, 1.0, k, 1.0, 0.0)
    assert np.array_equal(_bits(got), _bits(want))
    assert tuple(np.isfinite(got)) == kept


def test_greedy_with_a_penalty_is_the_penalised_score():
    logits, seen, valid = wr.make_case(3, 1031, n_valid=5, scale=3.0)
    got, dist = wr.warp_ref(logits[0], seen[0], valid, do_sample=False, repetition_penalty=1.3, temperature=0.7, top_k=5, top_p=0.5)
    want = _hf(logits[0], seen[0], valid, 1.3, 1.0, 0, 1.0, 0.0)
    assert np.array_equal(_bits(got), _bits(want)) and np.isinf(dist).all()
    assert (got != logits[0][valid]).any()                       # a valid id was in the seen set


@pytest.mark.parametrize("seed", [2, 6])
def test_host_loop_device_path_equals_the_torch_path(monkeypatch, seed):
    """generate(do_sample=True, top_k=50, top_p=0.9, repetition_penalty=1.1), seeded, on the fake engine with a stub lm_warp_valid
    built from warp_ref: the same sequences as the same call with warp_on_device = False.  Pins what the host loop hands the entry:
    the seen sets (prompt ids, the pad id rule, the tokens generated since the last step), the row order, the scalars.  The small
    oracle model's valid ids rank far below its top 50 of 320, so its full logits get the four valid columns lifted by 3 (both runs);
    seed 2 ends row 0 early and seed 6 row 1: the surviving row then sits at another position of the call than its slot."""
    import types as _types
    import fake_engine
    from test_oracle_golden import G as GOLD, _oracle_small
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference
    z = np.load(os.path.join(GOLD, "generate_sampled_warped_b2.npz"))
    B = z["input_ids"].shape[0]
    gen_cfg = {"do_sample": True, "top_k": 50, "top_p": 0.9, "repetition_penalty": 1.1}
    calls = []

    def run(on_device):
        with fake_engine.cpu_cuda_shims(monkeypatch):
            eng = fake_engine.FakeEngine(_oracle_small(), n_slots=B)

            def lm_warp_valid(n, logits, seen, out, survivors, **kw):
                V, nv = eng.cfg.lm_vocab, len(eng.valid)
                assert 1 <= n <= 16 and logits.dtype == torch.float32 and out.dtype == torch.float32 and survivors.dtype == torch.int32
                assert seen is not None and seen.dtype == torch.uint8
                L = logits.reshape(-1)[:n * V].view(n, V).numpy()
                sn = seen.reshape(-1)[:n * V].view(n, V).numpy() != 0
                o, _, sv = wr.warp_ref_rows(L, sn, eng.valid, **kw)
                out.reshape(-1)[:n * nv].copy_(torch.from_numpy(o).reshape(-1))
                survivors[:n].copy_(torch.from_numpy(sv))
                calls.append((n, sn.sum(axis=1).tolist(), dict(kw)))
            eng.lm_warp_valid = lm_warp_valid
            plain_full = eng.lm_logits_full

            def lm_logits_full(n, hidden, out):
                plain_full(n, hidden, out)
                out.reshape(-1)[:n * eng.cfg.lm_vocab].view(n, -1)[:, 301:305] += 3.0
            eng.lm_logits_full = lm_logits_full
            cfgd = {"decoder_config": {"max_position_embeddings": 4096}, "diffusion_head_config": {"ddpm_num_inference_steps": 5},
                    "acoustic_tokenizer_config": {"fix_std": 0.5, "std_dist_type": "gaussian"}}
            m = VibeVoiceForConditionalGenerationInference(cfgd, eng, model_dtype=torch.float32)
            assert m.warp_on_device is True                      # the default
            m.warp_on_device = on_device
            m.set_speech_factors(0.2, -0.05)
            m.set_ddpm_inference_steps(5)
            tok = _types.SimpleNamespace(speech_start_id=301, speech_end_id=302, speech_diffusion_id=303, eos_token_id=304,
                                         bos_token_id=None, pad_token_id=305)
            torch.manual_seed(seed)
            return m.generate(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
                              speech_tensors=torch.from_numpy(z["speech_tensors"]), speech_masks=torch.from_numpy(z["speech_masks"]),
                              speech_input_mask=torch.from_numpy(z["speech_input_mask"]), cfg_scale=1.3, tokenizer=tok,
                              max_new_tokens=12, generation_config=gen_cfg, show_progress_bar=False)
    host = run(False)
    assert not calls
    dev = run(True)
    assert calls and all(kw == dict(repetition_penalty=1.1, temperature=1.0, do_sample=True, top_k=50, top_p=0.9, min_p=0.0)
                         for _, _, kw in calls)
    assert any(n == B for n, _, _ in calls) and any(n == 1 for n, _, _ in calls)
    # a seen set holds at least the row's prompt and never shrinks while the batch is whole
    whole = [c[1] for c in calls if c[0] == B]
    assert all(min(c) >= 8 for c in whole) and all(y >= x for p, q in zip(whole, whole[1:]) for x, y in zip(p, q))
    assert torch.equal(dev.sequences, host.sequences), (dev.sequences.tolist(), host.sequences.tolist())
    for a, b in zip(dev.speech_outputs, host.speech_outputs):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
