"""What the bounds of test_gpu_codec_exact.py are worth: every state fault of codec_exact.fault_list(), injected into the
CPU oracle's streaming chain, must move an output by at least 4x the bound the GPU tests hold that output to.

MIXED depths at the real widths, four frames, the fault applied to the carried state before each of frames 1..3.  A fault's
signature is the worst per-frame rel-L2 against the clean run, on the audio and on the semantic vector.  Frame 0 is common to
all runs, so the faulted runs start from a copy of the clean state after frame 0; a semantic-encoder fault leaves the audio
alone, so those runs reuse the clean audio.

Every fault clears both the xsplit 3 and the xsplit 2 bounds, so no fault is exempt from either: the smallest signatures are
3.3e-3 on the audio and 2.8e-3 on the semantic vector (newest history row of a C = 32 block lost), the loosest bounds 4e-5 and
6e-5.
"""
import copy

import pytest
import torch

import codec_exact as ce
from oracle import codec

N_FRAMES = 4


def _latents():
    g = torch.Generator().manual_seed(11)
    return [torch.randn(64, generator=g) * 0.7 for _ in range(N_FRAMES)]


def _run(chain, lats, fault=None, audio=None, start=0):
    """-> per-frame (audio, semantic) from frame `start` on.  audio: the clean run's audio (semantic-net faults skip the decoder)."""
    out = []
    for t in range(start, N_FRAMES):
        if fault is not None and t >= 1:
            ce.apply(fault, chain.dec if fault[1] == "dec" else chain.sem)
        with torch.no_grad():
            if audio is None:
                x = lats[t] / ce.SCALING - ce.BIAS
                a = codec.decoder_forward(chain.ac_w, x[None, :, None], chain.cc.ratios, chain.cc.dec_depths, chain.dec, chain.cc.eps)[0, 0]
            else:
                a = audio[t]
            s = codec.encoder_forward(chain.sem_w, a[None, None], chain.sc.ratios, chain.sc.enc_depths, chain.sem, chain.sc.eps)[0, :, 0]
        out.append((a, s))
    return out


@pytest.fixture(scope="module")
def clean():
    ac_w, sem_w = ce.codec_weights(ce.MIXED)
    cc, sc = ce.codec_cfgs(ce.MIXED)
    lats = _latents()
    chain = ce.OracleChain(ac_w, sem_w, cc, sc)
    # frame 0, then a snapshot of the carried state, then frames 1..3
    x = lats[0] / ce.SCALING - ce.BIAS
    with torch.no_grad():
        a0 = codec.decoder_forward(ac_w, x[None, :, None], cc.ratios, cc.dec_depths, chain.dec, cc.eps)[0, 0]
        s0 = codec.encoder_forward(sem_w, a0[None, None], sc.ratios, sc.enc_depths, chain.sem, sc.eps)[0, :, 0]
    snap = (copy.deepcopy(chain.dec), copy.deepcopy(chain.sem))
    rest = _run(chain, lats, start=1)
    return chain, lats, snap, [(a0, s0)] + rest


def _from_snapshot(clean):
    chain, _, snap, _ = clean
    c = ce.OracleChain(chain.ac_w, chain.sem_w, chain.cc, chain.sc)
    c.dec, c.sem = copy.deepcopy(snap[0]), copy.deepcopy(snap[1])
    return c


def test_clean_oracle_is_repeatable(clean):
    """the clean oracle run twice, from scratch, is bit-identical (the signatures below are differences of two such runs)"""
    chain, lats, _, ref = clean
    again = _run(ce.OracleChain(chain.ac_w, chain.sem_w, chain.cc, chain.sc), lats)
    for (a, s), (ra, rs) in zip(again, ref):
        assert torch.equal(a, ra) and torch.equal(s, rs)
    # ... and so is a run resumed from the frame-0 snapshot, which is what the faulted runs do
    resumed = _run(_from_snapshot(clean), lats, start=1)
    for (a, s), (ra, rs) in zip(resumed, ref[1:]):
        assert torch.equal(a, ra) and torch.equal(s, rs)


def test_every_fault_clears_the_gpu_bounds(clean):
    _, lats, _, ref = clean
    clean_audio = [a for a, _ in ref]
    weak, sig_a, sig_s = [], [], []
    for fault in ce.fault_list(ce.MIXED):
        got = _run(_from_snapshot(clean), lats, fault, audio=clean_audio if fault[1] == "sem" else None, start=1)
        sa = max(ce.rel_l2(a, ra) for (a, _), (ra, _) in zip(got, ref[1:]))
        ss = max(ce.rel_l2(s, rs) for (_, s), (_, rs) in zip(got, ref[1:]))
        print(f"fault {fault[0]:28s} audio {sa:.2e}  semantic {ss:.2e}")
        ok3 = sa >= 4 * ce.B3_AUDIO or ss >= 4 * ce.B3_SEM
        ok2 = sa >= 4 * ce.B2_AUDIO or ss >= 4 * ce.B2_SEM
        if not (ok3 and ok2):
            weak.append((fault[0], sa, ss, ok3, ok2))
        sig_s.append(ss)
        if fault[1] == "dec":                   # a semantic-encoder fault cannot reach the audio
            sig_a.append(sa)
    assert not weak, weak
    # no bound above a quarter of the smallest signature of its output
    print(f"smallest signature: audio {min(sig_a):.2e}, semantic {min(sig_s):.2e}")
    assert 4 * max(ce.B3_AUDIO, ce.B2_AUDIO) <= min(sig_a)
    assert 4 * max(ce.B3_SEM, ce.B2_SEM) <= min(sig_s)
    assert min(ce.B3_AUDIO, ce.B3_SEM, ce.B2_AUDIO, ce.B2_SEM, ce.B2_PAIR) >= 1e-5      # the oracle's own rounding is ~1e-6
