"""What the formant tests share (test_formant_cpu.py, test_gpu_formant.py): the resonator signals and the envelope read-out."""
import functools

import numpy as np
from scipy.signal import lfilter

RATE = 24000
FORMANTS, BANDWIDTH, AMPS = (700.0, 1500.0, 2600.0), 200.0, (1.0, 0.5, 0.3)


def resonate(excitation):
    """the excitation through three two-pole resonators (pole radius exp(-pi bw / rate)), summed, scaled to peak 0.5"""
    r = np.exp(-np.pi * BANDWIDTH / RATE)
    y = np.zeros(excitation.shape[0])
    for f, a in zip(FORMANTS, AMPS):
        y += a * lfilter([1.0], [1.0, -2.0 * r * np.cos(2.0 * np.pi * f / RATE), r * r], excitation)
    return y * (0.5 / np.abs(y).max())


@functools.lru_cache(maxsize=1)
def vowel():
    """48000 samples of noise through the resonators (read-only)"""
    v = resonate(np.random.default_rng(0).standard_normal(48000))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=1)
def pulses():
    """48000 samples of a pulse train of period 218 through the resonators (read-only)"""
    e = np.zeros(48000)
    e[::218] = 1.0
    v = resonate(e)
    v.setflags(write=False)
    return v


def peaks(x, rate=RATE):
    """The envelope's local maxima in Hz: the power of 2048-point Hann frames at hop 512, in dB, its mean over the frames, smoothed by
    a Gaussian of sigma 120 Hz, maxima between 200 and 5500 Hz within 35 dB of the largest.  The mean is taken of the dB values: that
    reading gives the figures the feature's prototype recorded (656 / 1559 / 2695 Hz for vowel(), 1008 / 2320 / 4031 at 3/2).  The dB
    of the mean power reads the second maximum at 1547 and, at 2/3, the first at 410 against 437.5: 6.25 % off."""
    x = np.asarray(x, dtype=np.float64)
    n = 2048
    fr = np.lib.stride_tricks.sliding_window_view(x, n)[::512] * np.hanning(n + 1)[:n]
    db = (10.0 * np.log10(np.abs(np.fft.rfft(fr, axis=1)) ** 2 + 1e-300)).mean(axis=0)
    hz = rate / n
    t = np.arange(-int(5 * 120.0 / hz), int(5 * 120.0 / hz) + 1) * hz
    g = np.exp(-0.5 * (t / 120.0) ** 2)
    pad = g.shape[0] // 2
    sm = np.convolve(np.pad(db, pad, mode="edge"), g / g.sum(), mode="valid")
    f = np.arange(sm.shape[0]) * hz
    top = sm[(f >= 200.0) & (f <= 5500.0)].max()
    return [float(f[k]) for k in range(1, sm.shape[0] - 1)
            if sm[k] > sm[k - 1] and sm[k] >= sm[k + 1] and 200.0 <= f[k] <= 5500.0 and sm[k] >= top - 35.0]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
