"""The seeded tensors of the W13 tests (test_w13_cpu.py, test_gpu_w13.py): bf16 weight matrices as bit patterns, and the planted
elements the format must refuse.  test_w13_cpu.py asserts that none of the normal tensors has a tile row that falls back, so that no GPU
test can pass by comparing the bf16 route with itself."""
import numpy as np
import torch

import synth

PACK_SHAPES = ((32, 128), (32, 256), (32, 384))      # one, two, three groups per tile row: fewer groups than the pack kernel has waves
WIDTHS = ((256, 768), (384, 1152))                   # head width H, FFN width I of the GEMV and sampler cases
HEAD_LAYERS = 4                                      # 12 gate / up / down matrices


def weights(N, K, seed):
    """a normal matrix at the usual 1 / sqrt(K) scale, rounded to bf16 (round to nearest even, as the upload rounds)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) / np.sqrt(K)).to(torch.bfloat16)


def bits(w):
    """bf16 tensor -> uint16 [N][K]"""
    return w.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(b):
    return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)


def head_matrices(H, I):
    """the gate / up / down matrices of the synthetic head at these widths, as the engine stores them: {name: bf16 [N][K]}"""
    w = synth.head_weights(synth.HeadCfg(hidden=H, layers=HEAD_LAYERS, ffn_ratio=I / H))
    return {k: v.to(torch.bfloat16) for k, v in w.items() if ".ffn." in k}


def reupload_down(H, I):
    """the new values of layers.2's down projection in the sampler test"""
    return weights(H, I, 7700 + H)


def gemv_weights(H, I):
    return {"gate": weights(I, H, 100 + H), "up": weights(I, H, 200 + H), "down": weights(H, I, 300 + H)}


def normal_cases():
    """every normal tensor a GPU test packs: (label, bf16 [N][K])"""
    out = [(f"pack {N}x{K}", weights(N, K, 40 + K)) for N, K in PACK_SHAPES]
    for H, I in WIDTHS:
        out += [(f"gemv {k} {H}/{I}", v) for k, v in gemv_weights(H, I).items()]
        out += [(f"head {k} {H}/{I}", v) for k, v in head_matrices(H, I).items()]
        out.append((f"reupload down {H}/{I}", reupload_down(H, I)))
    return out


# bf16 patterns the format refuses, planted into an otherwise normal tile row
DENORMAL, INF, NAN = 0x0001, 0x7F80, 0x7FC1


def under(b, binades):
    """the pattern `binades` binades under the pattern b (same sign and mantissa)"""
    return int(b) - (binades << 7)
