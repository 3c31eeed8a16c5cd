#!/usr/bin/env python
"""The device time a streamer's put() spends in front of the D2H copy when the pitch is shifted: A/B on one engine in one process, the
method of tools/level_ab.py.

  pcm16               Engine.audio_to_pcm16 on the [n, 3200] chunk batch (vv_audio_to_pcm16): AudioStreamer(pcm16=engine)
  tempo_pcm16         Tempo.push(..., pcm16=True) on the same batch at speed Q / P (vv_tempo_rows, the 16-bit conversion included): what
                      the tempo stage in front of the pitch stage costs by itself
  tempo_pitch_pcm16   Tempo.push(...) as fp32, then Pitch.push(..., pcm16=True) on what it emitted (vv_tempo_rows + vv_pitch_rows):
                      AudioStreamer(pcm16=engine, pitch=s)
for s = -12, -3, +3 and +12 semitones (P / Q = 1/2, 37/44, 44/37, 2/1) and n = 1 and n = 8 rows of one 3200-sample frame.  The streams
run on from iteration to iteration, as a streamer's do.  The stages touch no weight, so none is uploaded and the language model is cut
to one layer.

The arms alternate iteration by iteration after a warm-up of all; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90; per case the
added device time of the shifted put over the plain one and the share of it that is the pitch stage's.  No threshold is enforced: the
file records what was measured.

    python tools/pitch_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--semitones -12,-3,3,12] [--out profiles/pitch_ab.json]
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


def measure(eng, n, semis, iters, warmup):
    from vibevoice_amd import pitch as _pt
    P, Q = _pt.ratio(semis)
    speed = _pt.tempo_speed(1.0, semis)
    alone, front, pt = eng.tempo(n), eng.tempo(n), eng.pitch(n)
    try:
        g = torch.Generator().manual_seed(n)
        x = ((torch.rand(n, HOP, generator=g) * 2.0 - 1.0) * 0.9).to(eng.device)
        pcm = torch.empty((n, HOP), dtype=torch.int16, device=eng.device)
        out_tp = torch.empty((n, alone.max_out(HOP)), dtype=torch.int16, device=eng.device)
        mid = torch.empty((n, front.max_out(HOP)), dtype=torch.float32, device=eng.device)
        out_pt = torch.empty((n, pt.max_out(mid.shape[1])), dtype=torch.int16, device=eng.device)
        ids = list(range(n))
        emitted = []

        def chain():
            _, cnt = front.push(x, ids, speed, out=mid, stream=eng.stream)
            _, got = pt.push(mid, ids, semis, out=out_pt, pcm16=True, n_in=cnt, stream=eng.stream)
            emitted.append(got[0])
        arms = {"empty": lambda: None,
                "pcm16": lambda: eng.audio_to_pcm16(x, pcm, stream=eng.stream),
                "tempo_pcm16": lambda: alone.push(x, ids, speed, out=out_tp, pcm16=True, stream=eng.stream),
                "tempo_pitch_pcm16": chain}
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
        return {"semitones": semis, "P": P, "Q": Q, "tempo_speed": speed, "taps_per_output": 2 * _pt.taps(P, Q) + 1,
                "samples_per_put_mean": round(sum(emitted) / len(emitted), 1), "device_events": res,
                "added_device_us_per_put": round(med["tempo_pitch_pcm16"] - med["pcm16"], 2),
                "tempo_added_device_us_per_put": round(med["tempo_pcm16"] - med["pcm16"], 2),
                "pitch_stage_device_us_per_put": round(med["tempo_pitch_pcm16"] - med["tempo_pcm16"], 2),
                "one_pct_of_1p5b_frame_us": round(FRAME_MS_1P5B * 10.0, 2)}
    finally:
        alone.close()
        front.close()
        pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--semitones", default="-12,-3,3,12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/pitch_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/pitch_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone",
           "warmup": args.warmup, "cases": {}}
    try:
        for n in [int(r) for r in args.rows.split(",") if r]:
            for semis in [float(s) for s in args.semitones.split(",") if s]:
                key = f"{semis:+g}_n{n}"
                out["cases"][key] = measure(eng, n, semis, args.iters, args.warmup)
                print(json.dumps({"case": key, **out["cases"][key]}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
