#!/usr/bin/env python
"""The device time a streamer's put() spends in front of its D2H copy, with and without a speed: A/B on one engine in one process,
by the method of tools/resample_ab.py.

  pcm16         Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine) today
  tempo_pcm16   Tempo.push(..., pcm16=True) on the same batch (vv_tempo_rows, one launch, the 16-bit conversion included):
                AudioStreamer(pcm16=engine, speed=S)
for S = 0.5, 1.25 and 2.0 (27, 11 and 7 blocks of 240 output samples per 3200-sample frame, walked one after the other), n = 1 and
n = 8 rows of one frame.  The streams run on from iteration to iteration, as a streamer's do.  The stage touches no weight, so none is
uploaded and the language model is cut to one layer.

The arms alternate iteration by iteration after a warm-up of both; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
added device time of the stretching put over the plain one, that figure against the README's frame times, and the stretching put
against the resampling put's recorded median (profiles/resample_ab.json, 24000to48000_n8).  No threshold is enforced: the file records
what was measured.

    python tools/tempo_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/tempo_ab.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from resample_ab import HOP, build_engine, summarise  # noqa: E402

FRAME_MS = {"1.5b_shapes_n1": 1.59, "1.5b_shapes": 3.07, "7b_shapes": 8.0}


def measure(eng, speed, n, iters, warmup):
    from vibevoice_amd import tempo as T
    tp = eng.tempo(n)
    try:
        g = torch.Generator().manual_seed(int(speed * 100) + n)
        x = ((torch.rand(n, HOP, generator=g) * 2.0 - 1.0) * 0.5).to(eng.device)
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out = torch.empty((n, tp.max_out(HOP)), dtype=torch.int16, device=eng.device)
        ids = list(range(n))
        emitted = []
        arms = {"empty": lambda: None,
                "pcm16": lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream),
                "tempo_pcm16": lambda: emitted.append(tp.push(x, ids, speed, out=out, pcm16=True, stream=eng.stream)[1][0])}
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
        added = round(res["tempo_pcm16"]["median_us"] - res["pcm16"]["median_us"], 2)
        P, Q = T.ratio(speed)
        blocks = sorted(set(e // T.HS for e in emitted[warmup:]))
        return {"P": P, "Q": Q, "blocks_per_put_and_row": blocks, "device_events": res, "added_device_us_per_put": added,
                "added_percent_of_frame": {k: round(added / (ms * 10.0), 2) for k, ms in FRAME_MS.items()}}
    finally:
        tp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/tempo_ab.py measures on the GPU; none found")
    with open(os.path.join(ROOT, "profiles", "resample_ab.json")) as f:
        rs_us = json.load(f)["cases"]["24000to48000_n8"]["device_events"]["resample_pcm16"]["median_us"]
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/tempo_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone",
           "warmup": args.warmup, "frame_ms": FRAME_MS, "resample_put_median_us_n8_48k": rs_us, "cases": {}}
    try:
        for speed in (0.5, 1.25, 2.0):
            for n in [int(r) for r in args.rows.split(",") if r]:
                key = f"speed{speed}_n{n}"
                out["cases"][key] = measure(eng, speed, n, args.iters, args.warmup)
                out["cases"][key]["times_the_resample_put"] = round(out["cases"][key]["device_events"]["tempo_pcm16"]["median_us"] / rs_us, 2)
                print(json.dumps({"case": key, **out["cases"][key]}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
