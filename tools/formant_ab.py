#!/usr/bin/env python
"""The device time a streamer's put() spends in front of the D2H copy when the formants are warped: A/B on one engine in one process, the
method of tools/pitch_ab.py.

  pitch                Tempo.push(...) as fp32 at speed Q / P, then Pitch.push(..., pcm16=True) (vv_tempo_rows + vv_pitch_rows):
                       AudioStreamer(pcm16=engine, pitch=+3)
  pitch_formant0       Tempo.push, Formant.push at Q / P, Pitch.push, all fp32, then Level.push(..., pcm16=True) (the level stage the
                       warp brings with it): AudioStreamer(pcm16=engine, pitch=+3, formant=0.0)
  formant              Formant.push at ratio(+3) as fp32, then Level.push(..., pcm16=True): AudioStreamer(pcm16=engine, formant=+3)
  formant_push         Formant.push alone (vv_formant_rows: the frame launch and the sum launch)
  level_pcm16          Level.push(..., pcm16=True) alone on the [n, 3200] batch, for the share of the two arms above that is the level's
for n = 1 and n = 8 rows of one 3200-sample frame.  The streams run on from iteration to iteration, as a streamer's do.  The stages touch
no weight, so none is uploaded and the language model is cut to one layer.

The arms alternate iteration by iteration after a warm-up of all; every iteration is bracketed by a pair of device events on the
engine's stream (an empty pair is measured the same way and reported beside them).  Reported per arm: median and p90, and the medians
as a share of a 1.59 / 3.07 / 8.0 ms frame.  No threshold is enforced: the file records what was measured.

    python tools/formant_ab.py [--iters 200] [--warmup 20] [--rows 1,8] [--semitones 3] [--out profiles/formant_ab.json]
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


def measure(eng, n, semis, iters, warmup):
    from vibevoice_amd import formant as _fm
    from vibevoice_amd import pitch as _pt
    speed = _pt.tempo_speed(1.0, semis)
    keep, alone = _fm.fraction(0.0, semis), _fm.warp_of(semis)
    tp_a, pt_a = eng.tempo(n), eng.pitch(n)
    tp_b, fm_b, pt_b, lv_b = eng.tempo(n), eng.formant(n), eng.pitch(n), eng.level(n)
    fm_c, lv_c, fm_d, lv_e = eng.formant(n), eng.level(n), eng.formant(n), eng.level(n)
    stages = [tp_a, pt_a, tp_b, fm_b, pt_b, lv_b, fm_c, lv_c, fm_d, lv_e]
    try:
        g = torch.Generator().manual_seed(n)
        x = ((torch.rand(n, HOP, generator=g) * 2.0 - 1.0) * 0.9).to(eng.device)
        ids = list(range(n))
        dev = eng.device

        def buf(cols, dt=torch.float32):
            return torch.empty((n, cols), dtype=dt, device=dev)
        a_mid = buf(tp_a.max_out(HOP))
        a_out = buf(pt_a.max_out(a_mid.shape[1]), torch.int16)
        b_tp = buf(tp_b.max_out(HOP))
        b_fm = buf(fm_b.max_out(b_tp.shape[1]))
        b_pt = buf(pt_b.max_out(b_fm.shape[1]))
        b_out = buf(lv_b.max_out(b_pt.shape[1]), torch.int16)
        c_fm = buf(fm_c.max_out(HOP))
        c_out = buf(lv_c.max_out(c_fm.shape[1]), torch.int16)
        d_fm = buf(fm_d.max_out(HOP))
        e_out = buf(lv_e.max_out(HOP), torch.int16)
        emitted = []

        def pitch():
            _, cnt = tp_a.push(x, ids, speed, out=a_mid, stream=eng.stream)
            pt_a.push(a_mid, ids, semis, out=a_out, pcm16=True, n_in=cnt, stream=eng.stream)

        def pitch_formant0():
            _, cnt = tp_b.push(x, ids, speed, out=b_tp, stream=eng.stream)
            _, cnt = fm_b.push(b_tp, ids, fractions=keep, out=b_fm, n_in=cnt, stream=eng.stream)
            _, cnt = pt_b.push(b_fm, ids, semis, out=b_pt, n_in=cnt, stream=eng.stream)
            _, got = lv_b.push(b_pt, ids, 0.0, out=b_out, pcm16=True, n_in=cnt, stream=eng.stream)
            emitted.append(got[0])

        def formant():
            _, cnt = fm_c.push(x, ids, fractions=alone, out=c_fm, stream=eng.stream)
            lv_c.push(c_fm, ids, 0.0, out=c_out, pcm16=True, n_in=cnt, stream=eng.stream)
        arms = {"empty": lambda: None,
                "pitch": pitch,
                "pitch_formant0": pitch_formant0,
                "formant": formant,
                "formant_push": lambda: fm_d.push(x, ids, fractions=alone, out=d_fm, stream=eng.stream),
                "level_pcm16": lambda: lv_e.push(x, ids, 0.0, out=e_out, pcm16=True, stream=eng.stream)}
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
        return {"semitones": semis, "pitch_ratio": list(_pt.ratio(semis)), "warp_kept": list(keep), "warp_alone": list(alone),
                "frames_per_put": (HOP + _fm.H - 1) // _fm.H, "samples_per_put_mean": round(sum(emitted) / len(emitted), 1),
                "device_events": res,
                "formant_added_to_pitch_put_us": round(med["pitch_formant0"] - med["pitch"], 2),
                "formant_stage_device_us_per_put": round(med["formant_push"] - med["empty"], 2),
                "share_of_frame_pct": {k: {f"{ms:g}ms": round(v / (ms * 10.0), 2) for ms in FRAMES_MS} for k, v in med.items() if k != "empty"}}
    finally:
        for s in stages:
            s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--semitones", default="3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formant_ab.json"))
    args = ap.parse_args()
    from vibevoice_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("tools/formant_ab.py measures on the GPU; none found")
    eng = build_engine(torch.device("cuda", 0))
    out = {"tool": "tools/formant_ab.py", "library_build": build.binary_id(), "device": torch.cuda.get_device_name(0),
           "stage": "what put() runs on the producing stream in front of the D2H copy, for one [n, 3200] fp32 chunk batch -> int16",
           "timing": "one device-event pair per iteration on the engine stream; arms alternate iteration by iteration in one process; "
                     "'empty' is the event pair alone",
           "warmup": args.warmup, "iters": args.iters, "cases": {}}
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
