"""Seeded synthetic weights/configs shared by the golden generator and the tests.

Everything is drawn from numpy's PCG64 `default_rng(seed)` so that
tests/golden/make_golden.py (build container, has /root/reference) and the
tests (CPU here, GPU box) see bit-identical weights without shipping them.
The golden files store a checksum of the weights they were generated with.

All matrix-shaped weights are rounded to bf16-representable values: the HIP
engine stores matrices as bf16, the oracle/reference compute in fp32 on the
*same* values, so parity tests measure arithmetic, not weight quantisation.
Zero-initialised layers of the reference (diffusion-head adaLN / final linear,
modular_vibevoice_diffusion_head.py:246-252) and the 1e-6 layer scales are
re-randomised -- otherwise outputs are identically 0 and tests are vacuous
(SURVEY.md 7(f)).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


class Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def normal(self, shape, std=1.0, mat=True):
        a = torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32) * np.float32(std))
        return bf16_round(a) if mat else a

    def uniform(self, shape, lo, hi):
        return torch.from_numpy(self.rng.uniform(lo, hi, shape).astype(np.float32))

    def linear(self, out_f, in_f, gain=1.0):
        return self.normal((out_f, in_f), gain / np.sqrt(in_f))

    def vec(self, n, std=0.1, mean=0.0):
        return torch.from_numpy((self.rng.standard_normal(n) * std + mean).astype(np.float32))


def checksum(w: dict) -> np.ndarray:
    s = 0.0
    s2 = 0.0
    for k in sorted(w):
        v = w[k].double()
        s += float(v.sum())
        s2 += float((v * v).sum())
    return np.array([s, s2], dtype=np.float64)


# ----------------------------------------------------------------------------
@dataclass
class HeadCfg:
    hidden: int = 64
    layers: int = 2
    ffn_ratio: float = 3.0
    latent: int = 64
    eps: float = 1e-5


def head_weights(cfg: HeadCfg, seed=1):
    g = Gen(seed)
    H, Fd = cfg.hidden, int(cfg.hidden * cfg.ffn_ratio)
    w = {
        "noisy_images_proj.weight": g.linear(H, cfg.latent),
        "cond_proj.weight": g.linear(H, H),
        "t_embedder.mlp.0.weight": g.linear(H, 256),
        "t_embedder.mlp.2.weight": g.linear(H, H),
        "final_layer.adaLN_modulation.1.weight": g.linear(2 * H, H, 0.5),
        "final_layer.linear.weight": g.linear(cfg.latent, H),
    }
    for i in range(cfg.layers):
        p = f"layers.{i}."
        w[p + "norm.weight"] = g.vec(H, 0.1, 1.0)
        w[p + "adaLN_modulation.1.weight"] = g.linear(3 * H, H, 0.5)
        w[p + "ffn.gate_proj.weight"] = g.linear(Fd, H)
        w[p + "ffn.up_proj.weight"] = g.linear(Fd, H)
        w[p + "ffn.down_proj.weight"] = g.linear(H, Fd)
    return w


# ----------------------------------------------------------------------------
@dataclass
class CodecCfg:
    n_filters: int = 4
    vae_dim: int = 64
    ratios: List[int] = field(default_factory=lambda: [8, 5, 5, 4, 2, 2])
    enc_depths: List[int] = field(default_factory=lambda: [1, 1, 1, 1, 1, 1, 2])
    eps: float = 1e-5

    @property
    def dec_depths(self):
        return list(reversed(self.enc_depths))

    @property
    def depth_str(self):
        return "-".join(str(d) for d in self.enc_depths)


def _block_weights(g, w, p, C):
    w[p + "norm.weight"] = g.vec(C, 0.1, 1.0)
    w[p + "ffn_norm.weight"] = g.vec(C, 0.1, 1.0)
    w[p + "gamma"] = g.uniform((C,), 0.3, 0.9)
    w[p + "ffn_gamma"] = g.uniform((C,), 0.3, 0.9)
    w[p + "mixer.conv.conv.conv.weight"] = g.normal((C, 1, 7), 1.0 / np.sqrt(7.0), mat=False)
    w[p + "mixer.conv.conv.conv.bias"] = g.vec(C, 0.1)
    w[p + "ffn.linear1.weight"] = g.linear(4 * C, C)
    w[p + "ffn.linear1.bias"] = g.vec(4 * C, 0.1)
    w[p + "ffn.linear2.weight"] = g.linear(C, 4 * C)
    w[p + "ffn.linear2.bias"] = g.vec(C, 0.1)


def encoder_weights(cfg: CodecCfg, seed=2, prefix="encoder."):
    g = Gen(seed)
    w = {}
    rr = list(reversed(cfg.ratios))
    nf = cfg.n_filters
    w[prefix + "downsample_layers.0.0.conv.conv.weight"] = g.normal((nf, 1, 7), 1.0 / np.sqrt(7.0))
    w[prefix + "downsample_layers.0.0.conv.conv.bias"] = g.vec(nf, 0.1)
    for i, r in enumerate(rr):
        cin, cout = nf * 2 ** i, nf * 2 ** (i + 1)
        w[prefix + f"downsample_layers.{i+1}.0.conv.conv.weight"] = g.normal((cout, cin, 2 * r), 1.0 / np.sqrt(cin * 2 * r))
        w[prefix + f"downsample_layers.{i+1}.0.conv.conv.bias"] = g.vec(cout, 0.1)
    for i, d in enumerate(cfg.enc_depths):
        C = nf * 2 ** i
        for j in range(d):
            _block_weights(g, w, prefix + f"stages.{i}.{j}.", C)
    Cl = nf * 2 ** (len(cfg.enc_depths) - 1)
    w[prefix + "head.conv.conv.weight"] = g.normal((cfg.vae_dim, Cl, 7), 1.0 / np.sqrt(Cl * 7))
    w[prefix + "head.conv.conv.bias"] = g.vec(cfg.vae_dim, 0.1)
    return w


def decoder_weights(cfg: CodecCfg, seed=3, prefix="decoder."):
    g = Gen(seed)
    w = {}
    nf = cfg.n_filters
    nd = len(cfg.dec_depths)
    C0 = nf * 2 ** (nd - 1)
    w[prefix + "upsample_layers.0.0.conv.conv.weight"] = g.normal((C0, cfg.vae_dim, 7), 1.0 / np.sqrt(cfg.vae_dim * 7))
    w[prefix + "upsample_layers.0.0.conv.conv.bias"] = g.vec(C0, 0.1)
    for i, r in enumerate(cfg.ratios):
        cin, cout = nf * 2 ** (nd - 1 - i), nf * 2 ** (nd - 2 - i)
        # ConvTranspose1d weight is [in, out, k]
        w[prefix + f"upsample_layers.{i+1}.0.convtr.convtr.weight"] = g.normal((cin, cout, 2 * r), 1.0 / np.sqrt(cin * 2))
        w[prefix + f"upsample_layers.{i+1}.0.convtr.convtr.bias"] = g.vec(cout, 0.1)
    for i, d in enumerate(cfg.dec_depths):
        C = nf * 2 ** (nd - 1 - i)
        for j in range(d):
            _block_weights(g, w, prefix + f"stages.{i}.{j}.", C)
    w[prefix + "head.conv.conv.weight"] = g.normal((1, nf, 7), 1.0 / np.sqrt(nf * 7))
    w[prefix + "head.conv.conv.bias"] = g.vec(1, 0.1)
    return w


def connector_weights(in_dim, H, seed=4):
    g = Gen(seed)
    return {
        "fc1.weight": g.linear(H, in_dim), "fc1.bias": g.vec(H, 0.1),
        "norm.weight": g.vec(H, 0.1, 1.0),
        "fc2.weight": g.linear(H, H), "fc2.bias": g.vec(H, 0.1),
    }


# ----------------------------------------------------------------------------
@dataclass
class LMCfg:
    hidden: int = 128
    layers: int = 2
    heads: int = 2
    kv_heads: int = 1
    inter: int = 256
    vocab: int = 320
    theta: float = 1e6
    eps: float = 1e-6
    max_pos: int = 4096
    head_dim_override: Optional[int] = None     # explicit head dim (heads * head_dim != hidden); None = hidden // heads

    @property
    def head_dim(self):
        return self.head_dim_override or self.hidden // self.heads


def lm_weights(cfg: LMCfg, seed=5):
    g = Gen(seed)
    H, d = cfg.hidden, cfg.head_dim
    w = {"embed_tokens.weight": g.normal((cfg.vocab, H), 1.0), "norm.weight": g.vec(H, 0.1, 1.0)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        w[p + "input_layernorm.weight"] = g.vec(H, 0.1, 1.0)
        w[p + "post_attention_layernorm.weight"] = g.vec(H, 0.1, 1.0)
        w[p + "self_attn.q_proj.weight"] = g.linear(cfg.heads * d, H)
        w[p + "self_attn.q_proj.bias"] = g.vec(cfg.heads * d, 0.2)
        w[p + "self_attn.k_proj.weight"] = g.linear(cfg.kv_heads * d, H)
        w[p + "self_attn.k_proj.bias"] = g.vec(cfg.kv_heads * d, 0.2)
        w[p + "self_attn.v_proj.weight"] = g.linear(cfg.kv_heads * d, H)
        w[p + "self_attn.v_proj.bias"] = g.vec(cfg.kv_heads * d, 0.2)
        w[p + "self_attn.o_proj.weight"] = g.linear(H, cfg.heads * d)
        w[p + "mlp.gate_proj.weight"] = g.linear(cfg.inter, H)
        w[p + "mlp.up_proj.weight"] = g.linear(cfg.inter, H)
        w[p + "mlp.down_proj.weight"] = g.linear(H, cfg.inter)
    return w


def lm_head_weight(cfg: LMCfg, seed=6):
    return Gen(seed).linear(cfg.vocab, cfg.hidden)
