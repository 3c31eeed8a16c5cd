"""tests/gemv16p_ref.py (the fp64 reference of the batch-decode packed GEMV) held to its written definitions and to tests/gemv_ref.py,
on the CPU: the tile layout element by element against the index formula, and the RS / SH / PK additions against the prologues that
test_gemv_ref_cpu.py already ties to the oracle -- so the reference the GPU cases compare with cannot drift from that one."""
import struct

import numpy as np
import pytest
import torch

import gemv16p_ref as P
import gemv_ref as R
import synth


def _bf16_bits(v):
    """the bf16 bit pattern of a float that is exactly representable"""
    return struct.unpack("<I", struct.pack("<f", float(v)))[0] >> 16


@pytest.mark.parametrize("T,K", [(16, 64), (5, 40), (1, 32)])
def test_tile_layout_element_by_element(T, K):
    x = synth.Gen(3 + T + K).normal((T, K), 1.0, mat=True)          # bf16 values: the rounding is not what is tested here
    raw = P.pack16_tile(x)
    assert raw.dtype == torch.uint8 and raw.numel() == P.tile_bytes(K) == ((K + 31) // 32) * 1024
    b = raw.numpy().tobytes()
    seen = np.zeros(len(b), dtype=bool)
    for t in range(16):
        for k in range(K):
            off = (((k >> 5) * 64 + (t & 15) + 16 * ((k & 31) >> 3)) * 16) + (k & 7) * 2
            want = _bf16_bits(x[t, k]) if t < T else 0
            assert struct.unpack_from("<H", b, off)[0] == want, (t, k)
            seen[off:off + 2] = True
    assert not any(b[i] for i in np.nonzero(~seen)[0]), "bytes of no element (columns past K) are not zero"


def test_tile_round_trip_and_rounding():
    g = synth.Gen(17)
    for T, K in ((16, 96), (7, 160), (3, 36)):
        x = g.normal((T, K), 1.0, mat=False)
        back = P.unpack16_tile(P.pack16_tile(x), K)
        assert torch.equal(back[:T], R.bf16r(x)) and not bool(back[T:].any())
        assert torch.equal(P.pack16_tile(back[:T]), P.pack16_tile(x))


def test_rs_from_partials_is_pro_rms():
    """the row scale from per-tile partial sums of squares of x, applied to W . bf16(x * nw), is gemv_ref's RMS prologue"""
    g = synth.Gen(23)
    T, K, N, eps = 5, 96, 20, 1e-5
    x, nw = g.normal((T, K), 1.0, mat=False), g.vec(K, 0.1, 1.0)
    W = R.weights(g.normal((N, K), 0.1))
    part = torch.zeros(K // 16, 16, dtype=torch.float64)
    part[:, :T] = P.ssq_partials(x)
    got = R.product(P.operands(P.pack16_tile(x * nw), K, T, ssq_in=part, eps=eps), W)
    want = R.product(R.pro_rms(x, nw, eps, 1), W)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


def test_rs_sh_is_pro_rms_mod():
    g = synth.Gen(29)
    T, K, N, eps = 6, 64, 12, 1e-5
    x, nw = g.normal((T, K), 1.0, mat=False), g.vec(K, 0.1, 1.0)
    sc, sh = g.normal((T, K), 0.3, mat=False), g.normal((T, K), 0.3, mat=False)
    W = R.weights(g.normal((N, K), 0.1))
    part = torch.zeros(K // 16, 16, dtype=torch.float64)
    part[:, :T] = P.ssq_partials(x)
    got = R.product(P.operands(P.pack16_tile((x * nw) * (1.0 + sc)), K, T, ssq_in=part, eps=eps, xs=P.pack16_tile(sh)), W)
    want = R.product(R.pro_rms_mod(x, nw, sc, sh, eps, 1), W)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


def test_partials_do_not_depend_on_their_split():
    """RS is defined on the sum over tiles: any split of the same totals gives the same scale"""
    g = synth.Gen(31)
    tot = g.uniform((16,), 10.0, 90.0).double()
    a = torch.stack([tot * 0.25, tot * 0.5, tot * 0.25])
    assert torch.allclose(P.rs_from_partials(a, 64, 1e-5), P.rs_from_partials(tot[None], 64, 1e-5), rtol=1e-14, atol=0)
    assert torch.allclose(P.rs_from_partials(tot[None], 64, 1e-5)[:, 0], 1.0 / torch.sqrt(tot / 64 + 1e-5), rtol=1e-14, atol=0)


def test_pk_feeds_the_next_rms():
    """PK's outputs are the next projection's RS operands: bf16(y * nw) and the partials of y reproduce pro_rms(y, nw)"""
    g = synth.Gen(37)
    T, N, N2, eps = 4, 64, 8, 1e-5
    y, nw = g.normal((T, N), 1.0, mat=False), g.vec(N, 0.1, 1.0)
    W = R.weights(g.normal((N2, N), 0.1))
    rows = P.pk_rows(y, nw)
    assert torch.equal(rows, R.bf16r(y * nw))
    part = torch.zeros(N // 16, 16, dtype=torch.float64)
    part[:, :T] = P.ssq_partials(y)
    got = R.product(P.operands(P.pack16_tile(rows), N, T, ssq_in=part, eps=eps), W)
    want = R.product(R.pro_rms(y, nw, eps, 1), W)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


def test_pack16_value_is_the_modulated_norm():
    g = synth.Gen(41)
    T, K, eps = 3, 64, 1e-5
    x, nw = g.normal((T, K), 1.0, mat=False), g.vec(K, 0.1, 1.0)
    sc, sh = g.normal((T, K), 0.3, mat=False), g.normal((T, K), 0.3, mat=False)
    main, shift = P.pack16_value(x, nw, eps, sc, sh)
    A, rs, S = R.pro_rms_mod(x, nw, sc, sh, eps, None)
    want = rs * A + S
    assert float(((main + shift) - want).abs().max() / want.abs().max()) <= 1e-6      # A is formed in fp32 there
    main1, shift1 = P.pack16_value(x, None, eps)
    assert not bool(shift1.any())
    assert torch.allclose(main1.pow(2).mean(-1), x.double().pow(2).mean(-1) / (x.double().pow(2).mean(-1) + eps), rtol=1e-12, atol=0)


def test_ulp_bf16():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 1e-3])
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -17], dtype=torch.float64)
    assert torch.equal(P.ulp_bf16(v), want)
    x = synth.Gen(43).normal((1000,), 1.0, mat=False)
    assert bool(((R.bf16r(x) - x).abs().double() <= P.ulp_bf16(x) / 2).all())
