#!/usr/bin/env python
"""The device time a streamer's put() spends in its conversion stage in front of the D2H copy, with and without an output level: A/B on
one engine in one process, the method of tools/resample_ab.py.

  pcm16            Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine)
  level_pcm16      Level.push(..., pcm16=True) on the same batch at 24 kHz (vv_level_rows, one launch, the 16-bit conversion included):
                   AudioStreamer(pcm16=engine, ceiling_db=-1)
  resample_pcm16   Resampler.push(..., pcm16=True) on the same batch, 24 -> 48 kHz (vv_resample_rows): AudioStreamer(pcm16=engine,
                   sample_rate=48000), the other stage that ends a chain, for scale
for n = 1 and n = 8 rows of one 3200-sample frame.  The stages touch no weight, so none is uploaded and the language model is cut to
one layer.

The arms alternate iteration by iteration after a warm-up of all; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
added device time of the level put over the plain one, and whether it costs more than the resampling put.  No threshold is enforced:
the file records what was measured.

    python tools/level_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/level_ab.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from resample_ab import FRAME_MS_1P5B, HOP, build_engine, summarise  # noqa: E402


def measure(eng, n, iters, warmup):
    lv, rs = eng.level(n, rate=24000, ceiling_db=-1.0), eng.resampler(24000, 48000, n)
    try:
        g = torch.Generator().manual_seed(n)
        x = ((torch.rand(n, HOP, generator=g) * 2.0 - 1.0) * 1.5).to(eng.device)          # a third of it beyond the ceiling
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out_lv = torch.empty((n, lv.max_out(HOP)), dtype=torch.int16, device=eng.device)
        out_rs = torch.empty((n, rs.max_out(HOP)), dtype=torch.int16, device=eng.device)
        ids = list(range(n))
        arms = {"empty": lambda: None,
                "pcm16": lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream),
                "level_pcm16": lambda: lv.push(x, ids, 0.0, out=out_lv, pcm16=True, stream=eng.stream),
                "resample_pcm16": lambda: rs.push(x, ids, out=out_rs, pcm16=True, stream=eng.stream)}
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
        added = round(res["level_pcm16"]["median_us"] - res["pcm16"]["median_us"], 2)
        return {"A": lv.A, "H": lv.H, "staged_samples_per_row": lv.H + 3 * lv.A - 3 + HOP, "device_events": res,
                "added_device_us_per_put": added, "resample_added_device_us_per_put": round(res["resample_pcm16"]["median_us"] - res["pcm16"]["median_us"], 2),
                "level_costs_more_than_resample": bool(res["level_pcm16"]["median_us"] > res["resample_pcm16"]["median_us"]),
                "one_pct_of_1p5b_frame_us": round(FRAME_MS_1P5B * 10.0, 2)}
    finally:
        lv.close()
        rs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/level_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/level_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone",
           "warmup": args.warmup, "cases": {}}
    try:
        for n in [int(r) for r in args.rows.split(",") if r]:
            key = f"24000_n{n}"
            out["cases"][key] = measure(eng, n, args.iters, args.warmup)
            print(json.dumps({"case": key, **out["cases"][key]}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
