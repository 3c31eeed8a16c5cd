"""tests/fake_engine's CPU engine with the general solver table: set_num_steps takes solver=, and a general configuration is
sampled through tests/solver_ref (the table-driven sampler held to the reference's recorded steps) over the oracle's head.
Shipped configurations keep the parent class's path.  The calls are logged for the routing tests."""
import torch

import fake_engine
import solver_ref
from oracle import head


class SolverFakeEngine(fake_engine.LoadableFakeEngine):
    def __init__(self, ecfg, device=None):
        super().__init__(ecfg, device)
        self.solver = None
        self.log = []           # ("set_num_steps", n, kwargs) / ("sample", n, rows of step noise or None)

    def set_num_steps(self, n, t_cast_bf16=False, algorithm_type="dpmsolver++", **kw):
        self.log.append(("set_num_steps", n, dict(kw, algorithm_type=algorithm_type)))
        assert set(kw) <= {"solver"}
        self.solver = kw.get("solver")
        self.t_cast_bf16 = t_cast_bf16
        super().set_num_steps(n, t_cast_bf16, algorithm_type)

    def general_config(self):
        return dict(self.solver, algorithm_type=self.algorithm_type)

    def diffusion_sample(self, n, cond, noise, cfg_scale, latent_out, step_noise=None):
        self.log.append(("sample", n, None if step_noise is None else tuple(step_noise.shape)))
        if self.solver is None:
            return super().diffusion_sample(n, cond, noise, cfg_scale, latent_out, step_noise=step_noise)
        om = self.om
        latent_out[:n] = solver_ref.sample(lambda x, t, c: head.head_forward(om.head_w, x, t, c, om.head_layers, om.head_eps),
                                           self.general_config(), self.n_steps, cond[:n].clone(), cond[n:2 * n].clone(), cfg_scale,
                                           noise[:n], t_cast_bf16=self.t_cast_bf16, step_noise=step_noise)
        self.calls["samples"] += 1
