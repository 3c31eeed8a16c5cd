"""The W13 format from its definition alone (vibevoice_amd/w13.py): no device, no library.

  * pack -> unpack is the identity for every normal tensor the GPU tests use, and none of their tile rows falls back: a cap of 0,
    asserted here, so that test_gpu_w13.py cannot pass by comparing the bf16 route with itself;
  * planted elements are flagged exactly as the rule says, per tile row;
  * the byte layout, element by element, against the sentences of the module's docstring written out one element at a time."""
import numpy as np
import pytest

import w13_cases as WC
from vibevoice_amd import w13

CASES = WC.normal_cases()


@pytest.mark.parametrize("label,w", CASES, ids=[c[0] for c in CASES])
def test_normal_tensors_round_trip_without_fallback(label, w):
    b = WC.bits(w)
    N, K = b.shape
    planes, emax, ok = w13.pack(b)
    assert planes.shape == (N // 16, K // 128, w13.GROUP_BYTES) and planes.dtype == np.uint8
    assert int((ok == 0).sum()) == 0, f"{label}: {int((ok == 0).sum())} tile rows fall back"
    assert np.array_equal(w13.unpack(planes, emax, N, K), b)
    assert len(w13.twin(b)) == w13.twin_bytes(N, K) == N * K * 13 // 8 + (2 * (N // 16) + 4) * 4


def _planted(value, row=20, col=70):
    b = WC.bits(WC.weights(32, 256, 5))
    b[row, col] = value
    return b


def test_zeros_of_both_signs_are_kept():
    for z in (0x0000, 0x8000):
        b = _planted(z)
        planes, emax, ok = w13.pack(b)
        assert ok.tolist() == [1, 1]
        assert w13.unpack(planes, emax, 32, 256)[20, 70] == z


def test_the_span_is_29_binades_under_the_tile_rows_maximum():
    b = WC.bits(WC.weights(32, 256, 5))
    top = b[16:32].reshape(-1)[np.argmax((b[16:32].reshape(-1) >> 7) & 0xFF)]
    for binades, good in ((29, True), (30, False), (31, False)):
        c = b.copy()
        c[20, 70] = WC.under(top, binades)
        rep, emax = w13.representable(c)
        assert bool(rep[20, 70]) == good and int(rep.sum()) == rep.size - (0 if good else 1)
        planes, em2, ok = w13.pack(c)
        assert ok.tolist() == [1, 1 if good else 0]          # the other tile row is untouched
        back = w13.unpack(planes, em2, 32, 256)
        want = c.copy()
        if not good:
            want[20, 70] = c[20, 70] & 0x8000                # stored as a zero of its sign
        assert np.array_equal(back, want)


@pytest.mark.parametrize("value", [WC.DENORMAL, WC.DENORMAL | 0x8000, WC.INF, WC.INF | 0x8000, WC.NAN], ids=["denormal", "-denormal", "inf", "-inf", "nan"])
def test_denormals_and_non_finite_values_are_not_representable(value):
    b = _planted(value)
    rep, emax = w13.representable(b)
    assert not rep[20, 70]
    _, _, ok = w13.pack(b)
    assert ok.tolist() == [1, 0]
    if value & 0x7F80 == 0x7F80:      # Emax = 255: nothing but the zeros of that tile row has a code
        assert int(emax[1]) == 255 and not rep[16:32][(b[16:32] & 0x7FFF) != 0].any()
    else:
        assert int(rep[16:32].sum()) == 16 * 256 - 1


def test_shapes_without_whole_groups_are_refused():
    for N, K in ((32, 96), (24, 128), (16, 130)):
        assert not w13.shape_ok(N, K)
        with pytest.raises(ValueError):
            w13.pack(np.zeros((N, K), dtype=np.uint16))


def test_layout_element_by_element():
    b = WC.bits(WC.weights(48, 384, 9))
    planes, emax, _ = w13.pack(b)
    tw = w13.twin(b)
    assert np.array_equal(tw[:planes.size], planes.reshape(-1))
    tail = tw[planes.size:].view(np.uint32)
    assert np.array_equal(tail[:3], emax) and tail[3:7].tolist() == [1, 1, 1, 1] and tail[7:].tolist() == [0, 0, 0]
    rng = np.random.default_rng(3)
    for n, k in zip(rng.integers(0, 48, 200), rng.integers(0, 384, 200)):
        n, k = int(n), int(k)
        v = int(b[n, k])
        s, E, m = v >> 15, (v >> 7) & 0xFF, v & 0x7F
        tile, group = n // 16, k // 128
        kt, kk = (k % 128) // 32, k % 32
        lane, e = (kk // 8) * 16 + n % 16, kk % 8
        idx = kt * 8 + e
        g = planes[tile, group]
        hb = int(g[(idx // 16) * 1024 + lane * 16 + idx % 16])
        c = E - int(emax[tile]) + 30 if v & 0x7FFF else 0
        assert hb == (s << 7 | c << 2 | m >> 5)
        string = int.from_bytes(bytes(g[2048 + lane * 16:2048 + lane * 16 + 16]) + bytes(g[3072 + lane * 4:3072 + lane * 4 + 4]), "little")
        assert (string >> (10 * (idx // 2) + 5 * (idx % 2))) & 31 == m & 31
    assert np.array_equal(w13.fragments(b)[2, 5, 17], b[32 + 1, 5 * 32 + 8:5 * 32 + 16])
