"""Shared pieces of the exact-mode tests of the streaming tokenizer chains at the real channel widths
(test_gpu_codec_exact.py on the GPU, test_codec_fault_sensitivity_cpu.py on the CPU).

The chains (acoustic decoder -> semantic encoder, one frame per call, conv histories carried per utterance slot) run at
n_filters = 32, i.e. C = 32 .. 2048, in the two exact modes and are compared frame by frame with the fp32 CPU oracle
(oracle/codec.py):
  xsplit 3  exact fp32 activations, per-slot paths only;
  xsplit 2  the kernel families of the timed bf16 mode (MFMA tile form, 16-row GEMV form, slot batching, fused block1d,
            row-tiled / channel-sliced norm + conv, the T = 1 PRO_NORMDW GEMV stage) with two-term activations.

The fault list is what gives the bounds below their meaning: every entry perturbs one piece of carried state of the
ORACLE (a conv history zeroed, rolled by a row, its newest row zeroed); test_codec_fault_sensitivity_cpu.py asserts that
each of them moves an output by at least 4x the bound the GPU tests hold that output to.
"""
import torch

import synth

# encoder order (C = 32, 64, 128, 256, 512, 1024, 2048); the decoder runs the reversed list
REAL = [3, 3, 3, 3, 3, 3, 8]        # the shipped 1.5B / 7B tokenizers
MIXED = [2, 1, 2, 1, 2, 1, 2]       # with REAL: every stage kind once with an odd and once with an even block count
SCALING, BIAS = 0.2, -0.05

# Bounds: worst per-frame rel-L2 against the fp32 oracle over all frames and slots of test_gpu_codec_exact.py.  Each is 4x the
# worst value measured on an MI355X over three input seeds (0, 1, 2), rounded up to one significant digit, and never below
# 1e-5: the oracle's own rounding (fp32 against float64 at these shapes) is 1.1e-6 on the audio and 1.4e-6 on the semantic
# vector.  The three seeds lie within 1.25x of each other for every figure.  The smallest fault signature
# (test_codec_fault_sensitivity_cpu.py, MIXED depths) is 3.3e-3 on the audio and 2.8e-3 on the semantic vector, 70x and 46x
# the loosest bound of its output.
B3_AUDIO = 1e-5     # xsplit 3: measured 1.68e-6 (REAL), 1.49e-6 (MIXED); 4x = 6.7e-6, lifted to the 1e-5 floor
B3_SEM = 2e-5       # xsplit 3: measured 2.88e-6 (REAL), 2.44e-6 (MIXED); 4x = 1.2e-5
B2_AUDIO = 4e-5     # xsplit 2: measured 8.28e-6 one slot (REAL), 8.17e-6 slot-batched REAL, 8.08e-6 the 8-row plan; 4x = 3.3e-5
B2_SEM = 6e-5       # xsplit 2: measured 1.32e-5 slot-batched REAL, 1.25e-5 the 8-row plan, 1.22e-5 one slot; 4x = 5.3e-5
B2_PAIR = 6e-5      # xsplit 2, slot-batched slot against the one-utterance path on equal inputs: measured 1.40e-5; 4x = 5.6e-5


def codec_cfgs(depths):
    return (synth.CodecCfg(n_filters=32, enc_depths=list(depths)),
            synth.CodecCfg(n_filters=32, vae_dim=128, enc_depths=list(depths)))


def codec_weights(depths):
    """(acoustic decoder weights, semantic encoder weights), seeds as gpu_util.build_small"""
    cc, sc = codec_cfgs(depths)
    return synth.decoder_weights(cc, 3), synth.encoder_weights(sc, 7)


def build_codec_engine(xsplit, depths, n_slots, use_graph, weights=None):
    """An Engine as gpu_util.build_small builds it -- smallest LM, two head layers -- but with both streaming tokenizers at the real
    widths and `depths` blocks per stage.  No acoustic encoder: the streaming chain does not run it.
    Returns (engine, acoustic decoder weights, semantic encoder weights, acoustic cfg, semantic cfg)."""
    from vibevoice_amd.engine import Engine, EngineConfig
    lmcfg = synth.LMCfg()
    H = lmcfg.hidden
    hc = synth.HeadCfg(hidden=H, layers=2)
    cc, sc = codec_cfgs(depths)
    ac_w, sem_w = weights if weights is not None else codec_weights(depths)
    lm_w = synth.lm_weights(lmcfg)
    ecfg = EngineConfig(lm_hidden=H, lm_layers=lmcfg.layers, lm_heads=lmcfg.heads, lm_kv_heads=lmcfg.kv_heads,
                        lm_head_dim=lmcfg.head_dim, lm_inter=lmcfg.inter, lm_vocab=lmcfg.vocab, lm_eps=lmcfg.eps, rope_theta=lmcfg.theta,
                        head_layers=hc.layers, head_ffn_ratio=hc.ffn_ratio, head_eps=hc.eps,
                        n_filters=cc.n_filters, ratios=cc.ratios, enc_depths=cc.enc_depths, sem_dim=128, has_acoustic_encoder=False,
                        codec_eps=cc.eps, n_slots=n_slots, max_ctx=64, xsplit=xsplit, use_graph=use_graph, max_rows=16, enc_frames=1)
    eng = Engine(ecfg)
    sd = {"lm." + k: v for k, v in lm_w.items()}
    sd["lm_head.weight"] = synth.lm_head_weight(lmcfg)
    sd.update({"head." + k: v for k, v in synth.head_weights(hc).items()})
    sd.update({"dec." + k[len("decoder."):]: v for k, v in ac_w.items()})
    sd.update({"senc." + k[len("encoder."):]: v for k, v in sem_w.items()})
    sd.update({"ac_conn." + k: v for k, v in synth.connector_weights(64, H, 4).items()})
    sd.update({"sem_conn." + k: v for k, v in synth.connector_weights(128, H, 8).items()})
    eng.load_state_dict(sd, mapped=True, strict=True)
    eng.set_speech_factors(SCALING, BIAS)
    return eng, ac_w, sem_w, cc, sc


class OracleChain:
    """One utterance's streaming decoder -> semantic encoder on the CPU oracle."""

    def __init__(self, ac_w, sem_w, cc, sc):
        self.ac_w, self.sem_w, self.cc, self.sc = ac_w, sem_w, cc, sc
        self.dec, self.sem = {}, {}

    def step(self, latent, sem=True):
        """latent [64] as the engine takes it (speech factors not yet undone) -> (audio [3200], semantic [128] or None)"""
        from oracle import codec
        x = latent / SCALING - BIAS
        with torch.no_grad():
            a = codec.decoder_forward(self.ac_w, x[None, :, None], self.cc.ratios, self.cc.dec_depths, self.dec, self.cc.eps)[0, 0]
            s = codec.encoder_forward(self.sem_w, a[None, None], self.sc.ratios, self.sc.enc_depths, self.sem, self.sc.eps)[0, :, 0] if sem else None
        return a, s

    def reset(self):
        from oracle import codec
        codec.zero_state(self.dec)
        codec.zero_state(self.sem)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


# ---------------------------------------------------------------------------------------------------------------- faults
def _zero(t):
    return torch.zeros_like(t)


def _roll(t):
    return torch.roll(t, 1, dims=2)


def _newest(t):
    t = t.clone()
    t[:, :, -1] = 0
    return t


OPS = {"zero": _zero, "roll": _roll, "newest": _newest}


def _dec_block(depths, stage, block):
    """state-key substring of the decoder's stage `stage` (decoder order: stage 0 is C = 2048), block clamped to the stage's last"""
    d = list(reversed(depths))[stage]
    return f"decoder.stages.{stage}.{min(block, d - 1)}.mixer"


def _sem_block(depths, stage, block):
    return f"encoder.stages.{stage}.{min(block, depths[stage] - 1)}.mixer"


def fault_list(depths):
    """(name, net, state-key substring, operation): net "dec" / "sem" is the oracle state dict the key lives in.  First the ten
    faults the bounds were sized against (block indices are those of the REAL depths, clamped to the last block of a shorter
    stage), then zero / roll / newest-row-zero on one block of every stage kind of each net: T = 1 GEMV stage (C = 2048),
    channel-sliced norm + conv (1024), row-tiled norm + conv (512, 256), fused block kernel (128, 32; C = 64 is among the ten)."""
    f = [
        ("dec s0 b0 zero", "dec", _dec_block(depths, 0, 0), "zero"),
        ("dec s0 last newest", "dec", _dec_block(depths, 0, 7), "newest"),
        ("dec s3 b1 roll", "dec", _dec_block(depths, 3, 1), "roll"),
        ("dec s6 b2 zero", "dec", _dec_block(depths, 6, 2), "zero"),
        ("dec s5 b0 zero", "dec", _dec_block(depths, 5, 0), "zero"),
        ("dec upsample 4 zero", "dec", "decoder.upsample_layers.4.0.convtr.convtr.", "zero"),
        ("dec head zero", "dec", "decoder.head", "zero"),
        ("sem s6 b3 zero", "sem", _sem_block(depths, 6, 3), "zero"),
        ("sem s0 b1 zero", "sem", _sem_block(depths, 0, 1), "zero"),
        ("sem downsample 3 zero", "sem", "encoder.downsample_layers.3.0.conv.conv.", "zero"),
    ]
    # decoder stage i has C = 2048 >> i, encoder stage i has C = 32 << i
    for kind, ds, es in (("gemv2048", 0, 6), ("sliced1024", 1, 5), ("rows512", 2, 4), ("rows256", 3, 3), ("fused128", 4, 2), ("fused32", 6, 0)):
        for op in OPS:
            f.append((f"dec {kind} {op}", "dec", _dec_block(depths, ds, 1), op))
            f.append((f"sem {kind} {op}", "sem", _sem_block(depths, es, 1), op))
    seen, out = set(), []
    for name, net, key, op in f:
        if (net, key, op) not in seen:
            seen.add((net, key, op))
            out.append((name, net, key, op))
    return out


def apply(fault, state_dict):
    """Applies one entry of fault_list() to an oracle state dict (of the net the entry names), in place."""
    _, _, key, op = fault
    hit = [k for k in state_dict if key in k]
    if len(hit) != 1:
        raise KeyError(f"fault {fault[0]!r}: {key!r} matches {hit} in the state")
    state_dict[hit[0]] = OPS[op](state_dict[hit[0]])
