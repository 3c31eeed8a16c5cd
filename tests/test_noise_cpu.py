"""vibevoice_amd/noise.py, the counter-based generator of seeded requests (Philox4x32-10 + Box-Muller): known answers, the exactness of
the uniform, the moments and independence of the normals, and the argument rules."""
import math

import numpy as np
import pytest
import torch

from vibevoice_amd import noise

N = 1 << 20


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter, key, want", [
    ([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, want):
    """Random123's known-answer vectors"""
    assert _hex(noise.philox4x32(np.array(counter, dtype=np.uint64), key)) == want
    # vectorised: the same block inside a batch of counters
    batch = np.array([[1, 2, 3, 4], counter, [5, 6, 7, 8]], dtype=np.uint64)
    assert _hex(noise.philox4x32(batch, key)[1]) == want


def test_the_uniform_is_exact_in_fp32_and_inside_the_open_interval():
    x = np.array([0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffe00, 0xffffffff], dtype=np.uint32)
    x = np.concatenate([x, np.random.default_rng(1).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
    u = noise._u(x)
    assert u.dtype == np.float64
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # exactly representable
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24 and (u > 0).all() and (u < 1).all()
    for t in (0, 1, 2 ** 32 - 1):
        v = noise.uniform(12345, t)
        assert 0.0 < v < 1.0 and float(np.float32(v)) == v
    x0 = noise.philox4x32(np.array([0, 7, noise.STREAM_TOKEN, 0], dtype=np.uint64), (12345, 0))[0]
    assert noise.uniform(12345, 7) == ((int(x0) >> 9) + 0.5) * 2.0 ** -23


def _corr(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return abs(float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std())))


def test_moments_of_the_normals():
    z = noise.normals(0x0123456789abcdef, 0, 1, 0, 1, 0, N)
    assert z.shape == (1, 1, N) and z.dtype == torch.float32
    z = z.double().reshape(-1)
    mean, var = float(z.mean()), float(z.var())
    kurt = float(((z - mean) ** 4).mean() / var ** 2 - 3.0)
    assert abs(mean) <= 5 / math.sqrt(N), mean
    assert abs(var - 1) <= 5 * math.sqrt(2 / N), var
    assert abs(kurt) <= 5 * math.sqrt(24 / N), kurt
    assert float(z.abs().max()) <= 5.7681
    assert math.isclose(math.sqrt(48 * math.log(2)), 5.7681, abs_tol=5e-5)


def test_streams_seeds_and_counters_are_uncorrelated():
    s = 0xfeedfacecafebeef
    bound = 5 / math.sqrt(N)
    two = noise.normals(s, 0, 1, 0, 2, 0, N)                       # two streams of one key
    assert _corr(two[0], two[1]) <= bound
    assert _corr(two[0], noise.normals(s + 1, 0, 1, 0, 1, 0, N)) <= bound
    tt = noise.normals(s, 41, 2, 0, 1, 0, N)                       # t and t + 1
    assert _corr(tt[0, 0], tt[0, 1]) <= bound
    assert _corr(two[0], noise.normals(s, 0, 1, 0, 1, 3, N)) <= bound       # aux


def test_layout_of_normals():
    """[n_streams, n_t, width]: every entry is the single-stream, single-t call; element j = normal j % 4 of quad j // 4"""
    s = 99
    blk = noise.normals(s, 5, 3, 2, 4, 1, 68)
    assert blk.shape == (4, 3, 68)
    for a in range(4):
        for f in range(3):
            assert torch.equal(blk[a, f], noise.normals(s, 5 + f, 1, 2 + a, 1, 1, 68)[0, 0])
    assert torch.equal(noise.normals(s, 5, 1, 2, 1, 1, 6)[0, 0], blk[0, 0, :6])       # a width that is no multiple of 4: a prefix
    x = noise.philox4x32(np.array([3, 5, 2, 1], dtype=np.uint64), (s, 0))
    u0, u1 = noise._u(x[0]), noise._u(x[1])
    r = np.sqrt(-2.0 * np.log(u0))
    assert float(blk[0, 0, 12]) == float(np.float32(r * np.cos((2.0 * np.pi) * u1)))
    assert float(blk[0, 0, 13]) == float(np.float32(r * np.sin((2.0 * np.pi) * u1)))


def test_seed_range():
    for ok in (0, 2 ** 64 - 1, np.int64(5)):
        noise.normals(ok, 0, 1, 0, 1, 0, 4)
        noise.uniform(ok, 0)
    for bad in (-1, 2 ** 64, 1.5, "3", None, True):
        with pytest.raises(ValueError):
            noise.normals(bad, 0, 1, 0, 1, 0, 4)
        with pytest.raises(ValueError):
            noise.uniform(bad, 0)
    hi = noise.normals(2 ** 64 - 1, 0, 1, 0, 1, 0, 64)
    assert not torch.equal(hi, noise.normals(2 ** 32 - 1, 0, 1, 0, 1, 0, 64))         # the high half of the seed is part of the key


def test_the_counter_word_t_wraps():
    s = 7
    two = noise.normals(s, 2 ** 32 - 1, 2, 0, 1, 0, 64)
    assert torch.equal(two[0, 0], noise.normals(s, 2 ** 32 - 1, 1, 0, 1, 0, 64)[0, 0])
    assert torch.equal(two[0, 1], noise.normals(s, 0, 1, 0, 1, 0, 64)[0, 0])
    assert noise.uniform(s, 2 ** 32) == noise.uniform(s, 0)


def test_choose_is_the_inverse_cdf_of_the_float64_softmax():
    sc = np.array([0.0, -np.inf, math.log(3.0), -np.inf], dtype=np.float32)      # p = [1/4, 0, 3/4, 0]
    assert noise.choose(sc, 0.1) == 0 and noise.choose(sc, 0.2499) == 0
    assert noise.choose(sc, 0.2501) == 2 and noise.choose(sc, 0.999999) == 2
    assert noise.choose(sc, 1.0) == 2                                # no running sum exceeds u: the last index with p > 0
    with pytest.raises(ValueError):
        noise.choose(np.full(4, -np.inf), 0.5)
