#!/usr/bin/env python
"""The device time a streamer's put() spends in its last stages in front of the D2H copy, with and without the pause stage: A/B on one
engine in one process, the method of tools/level_ab.py.

  pcm16              Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine)
  level_pcm16        Level.push(..., pcm16=True) on the same batch at 24 kHz (vv_level_rows): AudioStreamer(pcm16=engine, ceiling_db=-1)
  pause_pcm16        Pause.push(..., pcm16=True) on the same batch (vv_pause_rows, one launch, the 16-bit conversion included):
                     AudioStreamer(pcm16=engine, max_pause_ms=100, max_lead_ms=20)
  level_pause_pcm16  Level.push to fp32, then Pause.push(..., pcm16=True) on what it emitted: both arguments together
for n = 1 and n = 8 rows of one 3200-sample frame.  The frame is [4 quiet segments | 2 loud | 3 quiet | 2 loud | 2 quiet and a third]:
under a lead cap of 20 ms (2 segments) the first run is held, cut and joined, under the cap of 100 ms the others pass as they arrive and
the last third of a segment waits, so the copy plan does all its kinds of work.  The pause streams are reset before every timed push (outside the event pair): the
lead cap applies to a stream's first run only, and every iteration then does the same work.  The stages touch no weight, so none is
uploaded and the language model is cut to one layer.

The arms alternate iteration by iteration after a warm-up of all; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
added device time of the pause put over the plain one and over the level put of the same run.  No threshold is enforced: the file
records what was measured.

    python tools/pause_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/pause_ab.json]
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

PAUSE_MS, LEAD_MS, SEG = 100, 20, 240


def frame(n):
    """[n, 3200]: quiet 4 | loud 2 | quiet 3 | loud 2 | quiet 2 1/3 segments, -70 and -20 dBFS noise"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, HOP, generator=g)
    gain = torch.full((HOP,), 10.0 ** (-70.0 / 20.0))
    for a, b in ((4, 6), (9, 11)):
        gain[a * SEG:b * SEG] = 10.0 ** (-20.0 / 20.0)
    return (x * gain).clamp(-1.0, 1.0)


def measure(eng, n, iters, warmup):
    lv, lv2 = eng.level(n, rate=24000, ceiling_db=-1.0), eng.level(n, rate=24000, ceiling_db=-1.0)
    ps, ps2 = eng.pause(n, rate=24000), eng.pause(n, rate=24000)
    try:
        x = frame(n).to(eng.device)
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out_lv = torch.empty((n, lv.max_out(HOP)), dtype=torch.int16, device=eng.device)
        mid = torch.empty((n, lv2.max_out(HOP)), dtype=torch.float32, device=eng.device)
        out_ps = torch.empty((n, ps.max_out(lv2.max_out(HOP))), dtype=torch.int16, device=eng.device)
        ids = list(range(n))

        def pause_alone():
            return ps.push(x, ids, PAUSE_MS, LEAD_MS, out=out_ps, pcm16=True, stream=eng.stream)

        def level_pause():
            _, cnt = lv2.push(x, ids, 0.0, out=mid, stream=eng.stream)
            return ps2.push(mid, ids, PAUSE_MS, LEAD_MS, out=out_ps, pcm16=True, n_in=cnt, stream=eng.stream)
        arms = {"empty": (None, lambda: None),
                "pcm16": (None, lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream)),
                "level_pcm16": (None, lambda: lv.push(x, ids, 0.0, out=out_lv, pcm16=True, stream=eng.stream)),
                "pause_pcm16": (ps, pause_alone),
                "level_pause_pcm16": (ps2, level_pause)}
        us = {k: [] for k in arms}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        emitted = None
        with torch.cuda.stream(eng.stream):
            for it in range(warmup + iters):
                for name, (fresh, fn) in arms.items():
                    if fresh is not None:
                        fresh.reset(stream=eng.stream)         # in front of the event pair: not timed
                    ev0.record(eng.stream)
                    r = fn()
                    ev1.record(eng.stream)
                    ev1.synchronize()
                    if it >= warmup:
                        us[name].append(ev0.elapsed_time(ev1) * 1e3)
                    if name == "pause_pcm16" and it == warmup + iters - 1:
                        emitted = r[1].cpu().tolist()
        eng.sync()
        res = {k: summarise(v) for k, v in us.items()}
        med = {k: v["median_us"] for k, v in res.items()}
        return {"seg": ps.seg, "max_pause_ms": PAUSE_MS, "max_lead_ms": LEAD_MS, "samples_in_per_row": HOP, "samples_out_per_row": emitted,
                "samples_dropped_per_row": ps.dropped(stream=eng.stream), "device_events": res,
                "pause_added_device_us_per_put_over_pcm16": round(med["pause_pcm16"] - med["pcm16"], 2),
                "pause_minus_level_put_us": round(med["pause_pcm16"] - med["level_pcm16"], 2),
                "level_pause_added_device_us_per_put_over_level": round(med["level_pause_pcm16"] - med["level_pcm16"], 2),
                "pause_costs_more_than_level": bool(med["pause_pcm16"] > med["level_pcm16"]),
                "one_pct_of_1p5b_frame_us": round(FRAME_MS_1P5B * 10.0, 2)}
    finally:
        for s in (lv, lv2, ps, ps2):
            s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pause_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/pause_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/pause_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone; the pause streams are reset in front of each pair",
           "warmup": args.warmup, "iters": args.iters, "cases": {}}
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
