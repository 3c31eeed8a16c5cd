"""The reference's full-vocabulary logits processors in reduction form, for the valid ids only (tests only).

HF's processors in front of the valid-token constraint -- repetition penalty, then with do_sample temperature, top-k, top-p, min-p
(min_tokens_to_keep = 1) -- reduce, for a token v that is read back, to a few reductions over the row: with s the penalised /
tempered fp32 scores, m = max s, e = exp(s - m),

    top-k   v survives iff #{j : s[j] > s[v]} < k, k = min(top_k, V);  T = {j : s[j] >= tau}, tau the k-th largest value
    top-p   v is removed iff A[v] <= (1 - top_p) Z,  Z = sum_{j in T} e[j],  A[v] = sum_{j in T, s[j] <= s[v]} e[j]
    min-p   v is removed iff exp(s[v] - m) < min_p
    the row's maximum is never removed by top-p / min-p.

Scores in fp32 (numpy's IEEE multiply / divide: what torch computes on the CPU), masses in fp64.  test_warp_ref_cpu.py holds this form
to transformers' own classes; test_gpu_warp_valid.py holds vv_lm_warp_valid to this form.
"""
import numpy as np

BOUNDARY_MARGIN = 1e-4      # 10 x the ~1e-5 relative error of summing <= 152K fp32 terms as ~150-term fp32 partials combined in fp64


def scores_f32(l, seen, repetition_penalty=1.0, temperature=1.0, do_sample=True):
    """RepetitionPenaltyLogitsProcessor + TemperatureLogitsWarper on one fp32 row"""
    s = np.asarray(l, dtype=np.float32).copy()
    if repetition_penalty != 1.0:
        pen = np.float32(repetition_penalty)
        s = np.where(np.asarray(seen, dtype=bool), np.where(s < 0, s * pen, s / pen), s).astype(np.float32)
    if do_sample and temperature != 1.0:
        s = (s / np.float32(temperature)).astype(np.float32)
    return s


def warp_ref(l, seen, valid, *, repetition_penalty=1.0, temperature=1.0, do_sample=True, top_k=0, top_p=1.0, min_p=0.0):
    """One row.  l [V] fp32, seen [V] bool (or None), valid: the ids read back.  Returns (out [n_valid] fp32: the processed score or
    -inf, dist [n_valid] fp64: the distance of each token to the nearest boundary of an active filter that decides about it --
    |A/Z - (1 - top_p)| for top-p, |exp(s - m) - min_p| / min_p for min-p; inf where none does)."""
    V = len(l)
    s = scores_f32(l, seen if seen is not None else np.zeros(V, bool), repetition_penalty, temperature, do_sample)
    valid = [int(v) for v in valid]
    sv = s[valid]
    out = sv.copy()
    dist = np.full(len(valid), np.inf)
    if not do_sample:
        return out, dist
    keep = np.ones(len(valid), bool)
    in_T = np.ones(V, bool)
    k = min(int(top_k), V) if top_k > 0 else 0
    if k > 0:
        keep &= np.array([(s > x).sum() < k for x in sv])
        tau = np.partition(s, V - k)[V - k]                  # the k-th largest value
        in_T = s >= tau
    m = s.max()
    e = np.exp(s.astype(np.float64) - np.float64(m))
    if top_p < 1.0:
        Z = e[in_T].sum()
        for i, x in enumerate(sv):
            if not keep[i] or x == m:
                continue
            A = e[in_T & (s <= x)].sum()
            dist[i] = min(dist[i], abs(A / Z - (1.0 - top_p)))
            if A <= (1.0 - top_p) * Z:
                keep[i] = False
    if min_p > 0.0:
        for i, x in enumerate(sv):
            if not keep[i] or x == m:
                continue
            r = np.exp(np.float64(x) - np.float64(m))
            dist[i] = min(dist[i], abs(r - min_p) / min_p)
            if r < min_p:
                keep[i] = False
    out[~keep] = -np.inf
    return out, dist


def warp_ref_rows(logits, seen, valid, **kw):
    """[n, V] rows -> (out [n, n_valid] fp32, dist [n, n_valid], survivors [n] int32)"""
    outs, dists = zip(*[warp_ref(logits[r], None if seen is None else seen[r], valid, **kw) for r in range(len(logits))])
    out = np.stack(outs).astype(np.float32)
    return out, np.stack(dists), np.isfinite(out).sum(axis=1).astype(np.int32)


def make_case(seed, V, n_valid=4, scale=1.0, n=1):
    """n rows of normal fp32 logits at `scale`; n_valid ids (shared by the rows, as the engine holds them) lifted to 1..4 sigma in a
    per-row order with a little jitter, so that the filters cut BETWEEN them; a seen set per row (5 % of the ids) that holds at least
    one valid id.  Returns (logits [n, V] fp32, seen [n, V] bool, valid list)."""
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((n, V)) * scale).astype(np.float32)
    valid = sorted(int(v) for v in g.choice(V, size=n_valid, replace=False))
    seen = g.random((n, V)) < 0.05
    for r in range(n):
        lift = np.linspace(1.0, 4.0, n_valid) + g.uniform(-0.1, 0.1, n_valid)
        logits[r, valid] = (g.permutation(lift) * scale).astype(np.float32)
        seen[r, valid] = False
        seen[r, valid[int(g.integers(n_valid))]] = True
        if n_valid > 1:
            seen[r, valid[int(g.integers(n_valid))]] = True
    return logits, seen, valid


def tie_case(V=64):
    """the top-k boundary on ties: values 5 x 10, 3 x 10, 0 x (V - 20) (V = 64: 0 x 44), shuffled; valid ids: one of each value.
    k = 5, 10 keep only the 5s; k = 12, 20 keep the 5s and ALL the 3s (HF removes s < k-th value); k = 21 keeps everything."""
    g = np.random.default_rng(5)
    vals = np.array([5.0] * 10 + [3.0] * 10 + [0.0] * (V - 20), dtype=np.float32)
    l = vals[g.permutation(V)]
    valid = [int(np.nonzero(l == x)[0][0]) for x in (5.0, 3.0, 0.0)]
    return l[None, :].copy(), valid
