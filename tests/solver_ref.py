"""Table-driven DPM-Solver++ sampler in fp32 torch (tests only): what csrc/solver.hip computes per solver step, written out
with torch tensors so the CPU tests can hold vibevoice_amd.schedule.make_general_table to the reference scheduler's recorded
steps (tests/golden/solver_family.npz) and the GPU tests can hold the general sampler to the oracle's head.

One table row {a, s, cs, c0, c1, c2, cn, 0} per step:
    x0 = a z - s v
    z' = cs z + c0 x0 + c1 (x0 - m1) + c2 (m1 - m2) + cn noise          (m1, m2: the two previous x0)
Terms whose coefficient is zero are skipped, so a first-order row is the reference's first-order expression term by term.
"""
import torch

from vibevoice_amd import schedule


def step(row, z, v, m1=None, m2=None, noise=None):
    """-> (x0, z') of one table row; v: the (guided) v-prediction, m1 / m2: the previous two x0 (None: not yet there)"""
    a, s, cs, c0, c1, c2, cn = (float(x) for x in row[:7])
    x0 = a * z - s * v
    zn = cs * z + c0 * x0
    if c1 != 0.0:
        zn = zn + c1 * (x0 - m1)
    if c2 != 0.0:
        zn = zn + c2 * (m1 - m2)
    if cn != 0.0:
        zn = zn + cn * noise
    return x0, zn


def stochastic(config):
    return schedule.solver_settings(config)["algorithm_type"] == "sde-dpmsolver++"


def sample(head_fn, config, n_steps, cond, neg_cond, cfg_scale, noise, t_cast_bf16=False, step_noise=None):
    """sample_speech_tokens under `config`: head_fn(noisy [2n, L], t [2n], cond [2n, H]) -> [2n, L]; noise [n, L];
    cfg_scale a float or a tensor [n] (one scale per utterance row); step_noise [N, n, L] for a stochastic configuration."""
    tv, coef = schedule.make_general_table(config, n_steps, t_cast_bf16)
    assert (step_noise is not None) == stochastic(config)
    n = noise.shape[0]
    cfg = cfg_scale.reshape(n, 1).to(torch.float32) if isinstance(cfg_scale, torch.Tensor) else float(cfg_scale)
    condition = torch.cat([cond, neg_cond], dim=0)
    z = noise.to(torch.float32).clone()
    m1 = m2 = None
    for i in range(len(tv)):
        t = torch.full((2 * n,), float(tv[i]), dtype=torch.float32)
        eps = head_fn(torch.cat([z, z], dim=0), t, condition).to(torch.float32)
        v = eps[n:] + cfg * (eps[:n] - eps[n:])
        x0, z = step(coef[i], z, v, m1, m2, None if step_noise is None else step_noise[i].to(torch.float32))
        m1, m2 = x0, m1
    return z
