"""Counter-based random numbers of a seeded request (Philox4x32-10): the normative definition.

Every random number a request with a `seed` consumes is a pure function of (seed, the request's own counters, a stream id); nothing
is drawn from a shared, stateful generator, so what a request gets does not depend on the requests it shares the engine with.
csrc/noise.hip (vv_noise_rows) evaluates the same function on the device in fp32 for the per-frame draws; this module is the host
form: the cold draws, engines without the entry, and the reference the kernel is held to.

    key      (seed & 0xffffffff, seed >> 32),   0 <= seed < 2**64
    counter  (q, t, stream, aux), all uint32; t wraps modulo 2**32

    stream                 t                                             aux
    0          solver start noise          latents the request has ACCEPTED so far       0
    1 + i      variance noise, solver step i (sde-dpmsolver++)   as stream 0              0
    0x80000000 token choice                tokens the request has chosen before this one 0
    0x80000001 voice latent noise (r2)     voice frame index                             speaker index within the request
    0x80000002 voice per-speaker scale (r1)   0                                          speaker (normal 0 of quad 0 only)

Normals: element j of a row uses q = j // 4 and normal j % 4 of that block's output (x0, x1, x2, x3):
    u(x) = ((x >> 9) + 0.5) * 2**-23            exact in fp32, never 0 or 1
    r = sqrt(-2 ln u(x0)),  z0 = r cospi(2 u(x1)),  z1 = r sinpi(2 u(x1));  z2, z3 the same from (x2, x3)
so |z| <= sqrt(48 ln 2) = 5.7681.  The uniform of the token stream is u(x0) of counter (0, t, 0x80000000, 0).
This is a surface of its own: it does not reproduce the reference's torch RNG streams.
"""
import numpy as np
import torch

STREAM_START = 0                  # + 1 + i: variance noise of solver step i
STREAM_TOKEN = 0x80000000
STREAM_VOICE = 0x80000001
STREAM_VOICE_SCALE = 0x80000002

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def check_seed(seed, what="seed"):
    """a Python int in [0, 2**64); anything else raises ValueError"""
    if isinstance(seed, (bool, float)) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{what} = {seed!r}: a seed is an int with 0 <= seed < 2**64")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what} = {seed}: a seed is an int with 0 <= seed < 2**64")
    return seed


def philox4x32(counter, key):
    """Philox4x32-10.  counter: uint32 [..., 4], key: two uint32 words (scalars or arrays broadcastable to counter[..., 0]) ->
    uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(_MASK)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0 = np.asarray(key[0], dtype=np.uint64) & np.uint64(_MASK)
    k1 = np.asarray(key[1], dtype=np.uint64) & np.uint64(_MASK)
    m, sh = np.uint64(_MASK), np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & m
            k1 = (k1 + np.uint64(_W1)) & m
        p0 = c0 * np.uint64(_M0)                   # 32 x 32 -> 64 bits, exact in uint64
        p1 = c2 * np.uint64(_M1)
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m, (p0 >> sh) ^ c3 ^ k1, p0 & m
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _u(x):
    """uint32 -> float64 holding ((x >> 9) + 0.5) * 2**-23, a value fp32 represents exactly"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * (2.0 ** -23)


def normals(seed, t0, n_t, stream0, n_streams, aux, width) -> torch.Tensor:
    """fp32 [n_streams, n_t, width]: stream ids stream0 .. stream0 + n_streams - 1, counter words t = t0 .. t0 + n_t - 1 (mod 2**32);
    evaluated in float64 and rounded once"""
    seed = check_seed(seed)
    n_t, n_streams, width = int(n_t), int(n_streams), int(width)
    if n_t < 1 or n_streams < 1 or width < 1:
        raise ValueError(f"normals: n_t = {n_t}, n_streams = {n_streams}, width = {width} must be positive")
    nq = (width + 3) // 4
    ctr = np.empty((n_streams, n_t, nq, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nq, dtype=np.uint64)[None, None, :]
    ctr[..., 1] = ((int(t0) + np.arange(n_t, dtype=np.uint64)) & np.uint64(_MASK))[None, :, None]
    ctr[..., 2] = ((int(stream0) + np.arange(n_streams, dtype=np.uint64)) & np.uint64(_MASK))[:, None, None]
    ctr[..., 3] = int(aux) & _MASK
    x = philox4x32(ctr, (seed & _MASK, seed >> 32))
    z = np.empty((n_streams, n_t, nq, 4), dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(_u(x[..., a])))
        ang = (2.0 * np.pi) * _u(x[..., a + 1])
        z[..., a] = r * np.cos(ang)
        z[..., a + 1] = r * np.sin(ang)
    return torch.from_numpy(z.reshape(n_streams, n_t, nq * 4)[..., :width].astype(np.float32))


def uniform(seed, t) -> float:
    """the token stream's uniform in (0, 1) for the t-th token a request chooses"""
    seed = check_seed(seed)
    x = philox4x32(np.array([0, int(t) & _MASK, STREAM_TOKEN, 0], dtype=np.uint64), (seed & _MASK, seed >> 32))
    return float(_u(x[0]))


def choose(scores, u) -> int:
    """Index into one row of valid-id scores (already temperature-scaled, -inf = removed): p = float64 softmax, the first index whose
    running sum exceeds u, else the last index with p > 0.  ValueError when the row holds no finite score."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    fin = np.isfinite(s)
    if not fin.any():
        raise ValueError("no finite score")
    e = np.where(fin, np.exp(np.where(fin, s, 0.0) - s[fin].max()), 0.0)
    p = e / e.sum()
    hit = np.nonzero(np.cumsum(p) > u)[0]
    return int(hit[0]) if hit.size else int(np.nonzero(p > 0)[0][-1])
