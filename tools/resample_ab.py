#!/usr/bin/env python
"""The device time a streamer's put() spends in front of its D2H copy, with and without a sample rate: A/B on one engine in one
process.

  pcm16            Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine) today
  resample_pcm16   Resampler.push(..., pcm16=True) on the same batch (vv_resample_rows, one launch, the 16-bit conversion included):
                   AudioStreamer(pcm16=engine, sample_rate=R)
for R = 48000 (L / M = 2 / 1, 64 taps) and R = 8000 (1 / 3, 192 taps), n = 1 and n = 8 rows of one 3200-sample frame.  The stage
touches no weight, so none is uploaded and the language model is cut to one layer.

The arms alternate iteration by iteration after a warm-up of both; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
added device time of the resampling put over the plain one, and that figure against 1 % of the README's 1.5B-shapes frame (3.07 ms).
No threshold is enforced: the file records what was measured.

    python tools/resample_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/resample_ab.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FRAME_MS_1P5B = 3.07
HOP = 3200


def build_engine(device):
    from vibevoice_amd.configs import CONFIGS
    from vibevoice_amd.engine import Engine
    from vibevoice_amd.modeling import engine_config_from_reference
    cfg = copy.deepcopy(CONFIGS["1.5b"])
    cfg["decoder_config"]["num_hidden_layers"] = 1
    return Engine(engine_config_from_reference(cfg, n_slots=1, max_ctx=256, use_graph=False, max_rows=16), device)


def summarise(us):
    s = sorted(us)
    return {"median_us": round(statistics.median(s), 2), "p90_us": round(s[min(len(s) - 1, int(0.9 * len(s)))], 2), "iterations": len(s)}


def measure(eng, rate, n, iters, warmup):
    rs = eng.resampler(24000, rate, n)
    try:
        g = torch.Generator().manual_seed(rate + n)
        x = (torch.rand(n, HOP, generator=g) * 2.0 - 1.0).to(eng.device)
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out = torch.empty((n, rs.max_out(HOP)), dtype=torch.int16, device=eng.device)
        ids = list(range(n))
        arms = {"empty": lambda: None,
                "pcm16": lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream),
                "resample_pcm16": lambda: rs.push(x, ids, out=out, pcm16=True, stream=eng.stream)}
        us = {k: [] for k in arms}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(eng.stream):
            for it in range(warmup + iters):
                for name, fn in arms.items():
                    ev0.record(eng.stream)
                    fn()
                    ev1.record(eng.stream)
                    ev1.synchronize()
                    if it >= warmup:
                        us[name].append(ev0.elapsed_time(ev1) * 1e3)
        eng.sync()
        res = {k: summarise(v) for k, v in us.items()}
        added = round(res["resample_pcm16"]["median_us"] - res["pcm16"]["median_us"], 2)
        return {"L": rs.L, "M": rs.M, "taps": rs.T, "outputs_per_put_and_row": rs.counts(0, HOP), "device_events": res,
                "added_device_us_per_put": added, "limit_us_1pct_of_1p5b_frame": round(FRAME_MS_1P5B * 10.0, 2),
                "within_limit": bool(added < FRAME_MS_1P5B * 10.0)}
    finally:
        rs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/resample_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone",
           "warmup": args.warmup, "cases": {}}
    try:
        for rate in (48000, 8000):
            for n in [int(r) for r in args.rows.split(",") if r]:
                key = f"24000to{rate}_n{n}"
                out["cases"][key] = measure(eng, rate, n, args.iters, args.warmup)
                print(json.dumps({"case": key, **out["cases"][key]}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
