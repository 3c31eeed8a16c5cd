#!/usr/bin/env python
"""The token-choice stage of sampled decoding with the full-vocabulary logits processors as torch ops (warp_on_device = False,
modeling.py::_full_vocab_scores) and as one kernel (warp_on_device = True, vv_lm_warp_valid): A/B on one engine in one process.

Stage = what the host loop runs per LM step between the hidden state and the [n, n_valid] scores the draw is taken from:
vv_lm_logits_full, the seen-set update, the processors, the valid columns, the check that a valid token survived (a host wait in
both arms).  Shapes: the 7B language model's lm_head (V = 152064, H = 3584; ONE decoder layer -- the stage does not touch the
layers), synthetic seeded weights, n = 1 and n = 8 rows, generation_config {"top_k": 50, "top_p": 0.9, "repetition_penalty": 1.1}
with do_sample.  The hidden rows are one seeded vector and the valid ids are that row's four highest logits, so both arms keep a
valid token at every step; every iteration appends one token to each row's history (the seen sets grow as in a real run).

The arms alternate iteration by iteration (torch, device, lm_logits_full alone) after a warm-up of all three; every iteration is
bracketed by a pair of device events on the engine's stream.  Reported per arm: median and p90 of the per-iteration times.

    python tools/warp_valid_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/warp_valid_ab.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

GEN_CFG = {"top_k": 50, "top_p": 0.9, "repetition_penalty": 1.1}


def build_model(device, n_slots):
    from vibevoice_amd import synthetic
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.engine import Engine, map_param_name
    from vibevoice_amd.modeling import VibeVoiceForConditionalGenerationInference, engine_config_from_reference
    cfg = copy.deepcopy(CONFIGS["7b"])
    cfg["decoder_config"]["num_hidden_layers"] = 1
    ecfg = engine_config_from_reference(cfg, n_slots=n_slots, max_ctx=256, use_graph=False, max_rows=16)
    eng = Engine(ecfg, device)
    exp = eng.expected_weights()
    gen = torch.Generator(device=device)
    gen.manual_seed(0)
    for k, shape in synthetic.param_shapes(cfg).items():
        name = map_param_name(k)
        if name in exp:
            eng.upload(name, synthetic.random_tensor(k, shape, gen, device, torch.bfloat16))
    miss = eng.missing_weights()
    if miss:
        raise SystemExit(f"engine parameters not provided: {miss[:5]}")
    model = VibeVoiceForConditionalGenerationInference(cfg, eng, model_dtype=torch.bfloat16)
    return model, cfg


def summarise(us):
    s = sorted(us)
    return {"median_us": round(statistics.median(s), 2), "p90_us": round(s[min(len(s) - 1, int(0.9 * len(s)))], 2), "iterations": len(s)}


def measure(model, n, iters, warmup):
    from vibevoice_amd.modeling import _Session
    e = model.engine
    V, H = e.cfg.lm_vocab, e.cfg.lm_hidden
    g = torch.Generator().manual_seed(11)
    with torch.cuda.stream(e.stream):
        hid = (torch.randn(1, H, generator=g) * 2.0).repeat(n, 1).to(e.device)
        scratch = torch.empty(16 * V, dtype=torch.float32, device=e.device)
        e.lm_logits_full(1, hid[:1], scratch)
        valid = torch.topk(scratch[:V], 4).indices.tolist()
    e.sync()
    e.set_valid_tokens(valid)
    vt = torch.tensor(valid, dtype=torch.long, device=e.device)
    hist = torch.randint(0, V, (n, 64 + warmup + iters), generator=g).tolist()
    S = _Session(warp=dict(top_k=GEN_CFG["top_k"], top_p=GEN_CFG["top_p"], min_p=0.0, repetition_penalty=GEN_CFG["repetition_penalty"]),
                 do_sample=True, temperature=1.0, pad_id=None, nv=len(valid))
    order = [types.SimpleNamespace(idx=i, slot=i, ids=hist[i][:64], tokens=[], seq_len0=64, init_len=64, finished=False) for i in range(n)]

    def arm_torch():
        lg = model._full_vocab_scores(hid, order, S)[:, vt]
        if not bool(torch.isfinite(lg).any(dim=-1).all()):
            raise SystemExit("torch arm: a row lost every valid token")
        return lg

    def arm_device():
        lg = model._warp_valid_scores(hid, order, S)
        if int(model._warp_surv[:n].min()) < 1:
            raise SystemExit("device arm: a row lost every valid token")
        return lg

    def arm_logits():
        e.lm_logits_full(n, hid, scratch)
    arms = {"torch": arm_torch, "device": arm_device, "lm_logits_full": arm_logits}
    us = {k: [] for k in arms}
    agree = True
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(e.stream):
        for it in range(warmup + iters):
            for i, u in enumerate(order):
                u.tokens.append(hist[i][64 + it])
            got = {}
            for name, fn in arms.items():
                ev0.record(e.stream)
                got[name] = fn()
                ev1.record(e.stream)
                ev1.synchronize()
                if it >= warmup:
                    us[name].append(ev0.elapsed_time(ev1) * 1e3)
            a, b = got["torch"].float().cpu(), got["device"].float().cpu()
            fin = torch.isfinite(a)
            agree = agree and bool(torch.equal(fin, torch.isfinite(b))) and bool(torch.allclose(a[fin], b[fin], rtol=1e-6, atol=0))
    e.sync()
    res = {k: summarise(v) for k, v in us.items()}
    res["arms_agree"] = agree
    res["device_faster"] = bool(res["device"]["median_us"] < res["torch"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_valid_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/warp_valid_ab.py measures on the GPU; none found")
    device = torch.device("cuda", 0)
    rows = [int(r) for r in args.rows.split(",") if r]
    model, cfg = build_model(device, max(rows))
    out = {"tool": "tools/warp_valid_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "lm_vocab": model.engine.cfg.lm_vocab, "lm_hidden": model.engine.cfg.lm_hidden, "generation_config": dict(GEN_CFG, do_sample=True),
           "stage": "lm_logits_full -> seen-set update -> processors -> [n, n_valid] scores -> survivor check (host wait)",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process",
           "warmup": args.warmup, "rows": {}}
    try:
        for n in rows:
            out["rows"][str(n)] = measure(model, n, args.iters, args.warmup)
            print(json.dumps({"n": n, **{k: v for k, v in out["rows"][str(n)].items()}}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        model.engine.close()


if __name__ == "__main__":
    main()
