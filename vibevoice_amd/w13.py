"""W13: a lossless 13-bit storage of bf16 weight matrices, defined by bits.  csrc/vv_w13.h decodes the same format on the device
(vv_w13_unpack, the one decoder of the pack kernel's round trip, the test expansion and the decode GEMV's W13 forms) and
csrc/w13.hip packs it; this module needs no GPU and is what those kernels are tested against.

Why it is exact.  A bf16 value is sign (1) | exponent field E (8) | mantissa (7).  Within one tile row -- 16 output features x all K --
the exponents of trained weights span a few binades, so E is stored as a 5-bit code relative to the row's largest exponent Emax:

    representable:  +-0 (E = 0, mantissa 0; the sign is kept), or  Emax - 29 <= E <= Emax  with  1 <= E  and  Emax <= 254
    code c = E - Emax + 30 in 1..30, 0 for zero

Denormals (E = 0, mantissa != 0), values more than 29 binades under the row's maximum, Inf and NaN (E = 255, which makes Emax 255)
are not representable; a matrix with one such element keeps its bf16 launch as a whole.  Codes 1..30 are the normal range of an
e5m2 byte, so the high byte  sign << 7 | c << 2 | mantissa >> 5  is decoded by the hardware's e5m2 -> bf16 conversion with the
scale 2^(Emax - 142), and the low field  mantissa & 31  is or-ed under the result.  A non-representable element is stored as a zero
of its sign.  The device judges representability by decoding what it packed and comparing bits; ok() below states the same rule.

Layout.  The matrix [N][K] (N % 16 == 0, K % 128 == 0) is cut as the packed bf16 format is (csrc/vv_common.h): tile rows of 16
features, k-tiles of 32, 64 lanes per k-tile, lane l holding W[n0 + l % 16][k0 + (l // 16) * 8 + 0..7].  Four k-tiles are one group; a
lane's 32 elements of a group (element = k-tile * 8 + e) take 52 bytes in four planes, each plane contiguous over the 64 lanes:

    bytes [0, 1024)     lane * 16 + i     high byte of element i,       i = 0..15
    bytes [1024, 2048)  lane * 16 + i     high byte of element 16 + i
    bytes [2048, 3072)  lane * 16 ...     bits 0..127 of the lane's low string, little endian
    bytes [3072, 3328)  lane * 4 ...      bits 128..159 of it

The low string holds, for pair j = 0..15 (elements 2j, 2j + 1: one 32-bit word of a fragment), the 10 bits
lo[2j] | lo[2j + 1] << 5 at bit 10 j.  Groups are ordered [tile row][group].  Behind the planes: one uint32 Emax per tile row, one
uint32 ok per tile row (1 = every element of the row came back bit for bit), and one word that is the AND of those (then three of
padding): twin_bytes(N, K) in all, 13 / 16 of the bf16 bytes plus those words.
"""
import numpy as np

GROUP_BYTES = 3328
SPAN = 29                      # binades under Emax that still have a code


def shape_ok(N, K):
    return N > 0 and K > 0 and N % 16 == 0 and K % 128 == 0


def plane_bytes(N, K):
    return (N // 16) * (K // 128) * GROUP_BYTES


def twin_bytes(N, K):
    return plane_bytes(N, K) + (2 * (N // 16) + 4) * 4


def _lanes(w):
    """[N][K] -> [tile rows][groups][64 lanes][32 elements], the order of the layout above"""
    N, K = w.shape
    a = w.reshape(N // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 64, 8)
    return a.reshape(N // 16, K // 128, 4, 64, 8).transpose(0, 1, 3, 2, 4).reshape(N // 16, K // 128, 64, 32)


def _unlanes(a, N, K):
    b = a.reshape(N // 16, K // 128, 64, 4, 8).transpose(0, 1, 3, 2, 4).reshape(N // 16, K // 32, 4, 16, 8)
    return b.transpose(0, 3, 1, 2, 4).reshape(N, K)


def representable(bits):
    """bits: uint16 [N][K] bf16 patterns.  -> (bool [N][K], Emax uint32 [N // 16])"""
    bits = np.asarray(bits, dtype=np.uint16)
    N, K = bits.shape
    if not shape_ok(N, K):
        raise ValueError(f"W13 needs N % 16 == 0 and K % 128 == 0, got {N} x {K}")
    E = ((bits >> 7) & 0xFF).astype(np.int32)
    zero = (bits & 0x7FFF) == 0
    emax = E.reshape(N // 16, 16 * K).max(axis=1)
    em = np.repeat(emax, 16)[:, None]
    rep = zero | ((E >= 1) & (E + SPAN >= em) & (em <= 254))
    return rep, emax.astype(np.uint32)


def pack(bits):
    """bits: uint16 [N][K].  -> (planes uint8 [N // 16][K // 128][3328], Emax uint32 [N // 16], ok uint32 [N // 16])"""
    bits = np.asarray(bits, dtype=np.uint16)
    N, K = bits.shape
    rep, emax = representable(bits)
    s = (bits >> 15).astype(np.uint32)
    E = ((bits >> 7) & 0xFF).astype(np.uint32)
    m = (bits & 0x7F).astype(np.uint32)
    live = rep & ((bits & 0x7FFF) != 0)
    em = np.repeat(emax, 16)[:, None]
    c = np.where(live, E + 30 - em, 0).astype(np.uint32)
    hb = ((s << 7) | (c << 2) | np.where(live, m >> 5, 0)).astype(np.uint8)
    lo = np.where(live, m & 31, 0).astype(np.uint32)
    hb, lo = _lanes(hb), _lanes(lo)                                   # [T][G][64][32]
    x = lo[..., 0::2] | (lo[..., 1::2] << 5)                           # [T][G][64][16] ten bits per pair
    string = ((x[..., None] >> np.arange(10, dtype=np.uint32)) & 1).astype(np.uint8).reshape(*x.shape[:3], 160)
    low = np.packbits(string, axis=-1, bitorder="little")             # [T][G][64][20]
    T, G = hb.shape[:2]
    planes = np.empty((T, G, GROUP_BYTES), dtype=np.uint8)
    planes[..., 0:1024] = hb[..., :16].reshape(T, G, 1024)
    planes[..., 1024:2048] = hb[..., 16:].reshape(T, G, 1024)
    planes[..., 2048:3072] = low[..., :16].reshape(T, G, 1024)
    planes[..., 3072:3328] = low[..., 16:].reshape(T, G, 256)
    ok = rep.reshape(N // 16, 16 * K).all(axis=1).astype(np.uint32)
    return planes, emax, ok


def twin(bits):
    """the whole device buffer of a matrix, twin_bytes(N, K) bytes"""
    planes, emax, ok = pack(bits)
    tail = np.zeros(2 * len(emax) + 4, dtype=np.uint32)
    tail[:len(emax)] = emax
    tail[len(emax):2 * len(emax)] = ok
    tail[2 * len(emax)] = int(ok.all())
    return np.concatenate([planes.reshape(-1), tail.view(np.uint8)])


def unpack(planes, emax, N, K):
    """-> uint16 [N][K]: the value every stored element decodes to (a non-representable one: a zero of its sign)"""
    T, G = N // 16, K // 128
    planes = np.asarray(planes, dtype=np.uint8).reshape(T, G, GROUP_BYTES)
    hb = np.concatenate([planes[..., 0:1024].reshape(T, G, 64, 16), planes[..., 1024:2048].reshape(T, G, 64, 16)], axis=-1).astype(np.uint32)
    low = np.concatenate([planes[..., 2048:3072].reshape(T, G, 64, 16), planes[..., 3072:3328].reshape(T, G, 64, 4)], axis=-1)
    string = np.unpackbits(low, axis=-1, bitorder="little").reshape(T, G, 64, 32, 5).astype(np.uint32)
    lo = (string << np.arange(5, dtype=np.uint32)).sum(axis=-1)
    s, c, mh = hb >> 7, (hb >> 2) & 31, hb & 3
    em = np.asarray(emax, dtype=np.uint32).reshape(T, 1, 1, 1)
    E = np.where(c > 0, c + em - 30, 0)
    out = np.where(c > 0, (s << 15) | (E << 7) | (mh << 5) | lo, s << 15).astype(np.uint16)
    return _unlanes(out, N, K)


def fragments(bits):
    """uint16 [N][K] -> the packed bf16 format of csrc/vv_common.h as uint16 [N // 16][K // 32][64][8]"""
    bits = np.asarray(bits, dtype=np.uint16)
    N, K = bits.shape
    return bits.reshape(N // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 64, 8).copy()
