#!/usr/bin/env python
"""The device time a streamer's put() spends in its stage chain in front of the D2H copy, with and without the loudness leveller: A/B on
one engine in one process, the method of tools/level_ab.py.

  pcm16                 Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine)
  level_pcm16           Level.push(..., pcm16=True) on the same batch (vv_level_rows): AudioStreamer(pcm16=engine, ceiling_db=-1)
  loudness              Loudness.push on the same batch alone (vv_loud_rows: the FIR launch over tiles x rows, then the apply launch)
  loudness_level_pcm16  Loudness.push into an fp32 temporary, then Level.push(..., pcm16=True) of that:
                        AudioStreamer(pcm16=engine, loudness_lufs=-16)
for n = 1 and n = 8 rows of one 3200-sample frame.  The stages touch no weight, so none is uploaded and the language model is cut to
one layer.

The arms alternate iteration by iteration after a warm-up of all; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
device time the leveller adds to a put() against the conversion alone and against the level stage of the same run, and that as a share
of the 1.59, 3.07 and 8.0 ms frames.  No threshold is enforced: the file records what was measured.

    python tools/loudness_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--out profiles/loudness_ab.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from resample_ab import HOP, build_engine, summarise  # noqa: E402

FRAMES_MS = (1.59, 3.07, 8.0)


def measure(eng, n, iters, warmup):
    lv, lv2, ld, ld2 = eng.level(n, rate=24000, ceiling_db=-1.0), eng.level(n, rate=24000, ceiling_db=-1.0), eng.loudness(n), eng.loudness(n)
    try:
        g = torch.Generator().manual_seed(n)
        x = (torch.randn(n, HOP, generator=g) * 0.1).to(eng.device)                   # about -20 LUFS: every segment counts, the gain moves
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out_lv = torch.empty((n, lv.max_out(HOP)), dtype=torch.int16, device=eng.device)
        out_lv2 = torch.empty((n, lv2.max_out(HOP)), dtype=torch.int16, device=eng.device)
        tmp = torch.empty((n, HOP), dtype=torch.float32, device=eng.device)
        tmp2 = torch.empty((n, HOP), dtype=torch.float32, device=eng.device)
        ids = list(range(n))

        def chain():
            ld2.push(x, ids, -16.0, out=tmp2, stream=eng.stream)
            lv2.push(tmp2, ids, 0.0, out=out_lv2, pcm16=True, stream=eng.stream)
        arms = {"empty": lambda: None,
                "pcm16": lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream),
                "level_pcm16": lambda: lv.push(x, ids, 0.0, out=out_lv, pcm16=True, stream=eng.stream),
                "loudness": lambda: ld.push(x, ids, -16.0, out=tmp, stream=eng.stream),
                "loudness_level_pcm16": chain}
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
        med = {k: v["median_us"] for k, v in res.items()}
        over_pcm, over_level = round(med["loudness_level_pcm16"] - med["pcm16"], 2), round(med["loudness_level_pcm16"] - med["level_pcm16"], 2)
        return {"fir_workgroups": n * (HOP // 320), "fma_per_put": n * HOP * 2400, "device_events": res,
                "added_device_us_per_put_over_pcm16": over_pcm, "added_device_us_per_put_over_level": over_level,
                "added_over_level_share_of_frame_pct": {f"{ms}ms": round(over_level / (ms * 10.0), 2) for ms in FRAMES_MS},
                "added_over_pcm16_share_of_frame_pct": {f"{ms}ms": round(over_pcm / (ms * 10.0), 2) for ms in FRAMES_MS},
                "costs_less_than_the_tempo_put_at_its_worst_485us": bool(med["loudness"] < 485.0)}
    finally:
        for st in (lv, lv2, ld, ld2):
            st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/loudness_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/loudness_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "launch_form": "time-tiled: vv_loud_fir_rows_kernel over (10 tiles of 320 samples x rows), then vv_loud_apply_rows_kernel, one "
                          "workgroup per row (against one FIR workgroup per row: tools/experiments/loudness_row_form)",
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
