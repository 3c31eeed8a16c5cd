"""Thin Python wrapper over the libvvhip.so C ABI (include/vvhip.h).

PyTorch is used here only for device memory (tensors whose data_ptr() is handed
to the engine) and for the HIP stream; every arithmetic op of the hot path runs
inside libvvhip.so.  There is no fallback path: constructing an Engine without
the shared library or without a GPU raises.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import schedule as _schedule


@dataclass
class EngineConfig:
    # Qwen2 decoder
    lm_hidden: int
    lm_layers: int
    lm_heads: int
    lm_kv_heads: int
    lm_inter: int
    lm_vocab: int
    lm_head_dim: Optional[int] = None
    lm_eps: float = 1e-6
    rope_theta: float = 1e6
    # diffusion head
    head_layers: int = 4
    head_ffn_ratio: float = 3.0
    latent_dim: int = 64
    head_eps: float = 1e-5
    # tokenizers
    n_filters: int = 32
    ratios: Sequence[int] = (8, 5, 5, 4, 2, 2)
    enc_depths: Sequence[int] = (3, 3, 3, 3, 3, 3, 8)
    sem_dim: int = 128
    has_acoustic_encoder: bool = True
    codec_eps: float = 1e-5
    # runtime
    n_slots: int = 1
    max_ctx: int = 4096
    max_rows: int = 16
    xsplit: int = 2
    attn_splits: int = 128      # upper bound on flash-decoding splits; a launch uses one per 1024 positions of its longest row,
                                 # capped so that a launch of long rows aims at about 256 workgroups (csrc/pass_plan.h)
    enc_frames: int = 75         # voice-prompt frames per acoustic-encoder pass: one pass per 10-s speaker prompt (any pass size gives the
                                 # same result, tests/test_gpu_shipped.py; 0.042 s at 5 frames per pass -> 0.027 s at 75 for two speakers)
    use_graph: bool = True
    tts_layers: int = 0          # Streaming-0.5B: the last tts_layers of lm_layers form the TTS LM

    def __post_init__(self):
        if self.lm_head_dim is None:
            self.lm_head_dim = self.lm_hidden // self.lm_heads

    @property
    def head_ffn(self):
        return int(self.lm_hidden * self.head_ffn_ratio)

    @property
    def hop(self):
        return int(np.prod(self.ratios))


# reference state_dict prefix -> engine parameter prefix
PREFIX_MAP = (
    ("model.language_model.", "lm."),
    ("model.prediction_head.", "head."),
    ("model.acoustic_tokenizer.decoder.", "dec."),
    ("model.acoustic_tokenizer.encoder.", "aenc."),
    ("model.semantic_tokenizer.encoder.", "senc."),
    ("model.acoustic_connector.", "ac_conn."),
    ("model.semantic_connector.", "sem_conn."),
    ("lm_head.", "lm_head."),
)


def map_param_name(ref_key: str) -> Optional[str]:
    for a, b in PREFIX_MAP:
        if ref_key.startswith(a):
            return b + ref_key[len(a):]
    return None


class EngineError(RuntimeError):
    pass


class Engine:
    def __init__(self, cfg: EngineConfig, device: Optional[torch.device] = None, share_from: Optional["Engine"] = None):
        """share_from: another Engine of the same model on the same device whose weights are fully uploaded -- this engine then reads
        THOSE weights (vv_create_shared) and owns only its runtime state (KV caches, activations, tokenizer state, graphs) and its
        stream; uploads / LoRA merges go through the owner.  See Engine.fork()."""
        if not torch.cuda.is_available():
            raise EngineError("vibevoice_amd.Engine needs an AMD GPU (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:                 # device_map="cuda" (demo/inference_from_file.py:303): the current device
            self.device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        c = _lib.VVConfig()
        for f in ("lm_hidden", "lm_layers", "lm_heads", "lm_kv_heads", "lm_head_dim", "lm_inter", "lm_vocab",
                  "lm_eps", "head_layers", "latent_dim", "head_eps", "n_filters", "sem_dim", "codec_eps",
                  "n_slots", "max_ctx", "max_rows", "xsplit", "attn_splits", "enc_frames"):
            setattr(c, f, getattr(cfg, f))
        c.head_ffn = cfg.head_ffn
        c.n_ratios = len(cfg.ratios)
        for i, r in enumerate(cfg.ratios):
            c.ratios[i] = int(r)
        c.n_stages = len(cfg.enc_depths)
        for i, d in enumerate(cfg.enc_depths):
            c.enc_depths[i] = int(d)
        c.has_acoustic_encoder = int(cfg.has_acoustic_encoder)
        c.use_graph = int(cfg.use_graph)
        c.tts_layers = int(cfg.tts_layers)
        self._ctx = C.c_void_p()
        # a dedicated non-default stream: hipGraph capture is illegal on the null stream
        self.stream = torch.cuda.Stream(device=self.device)
        self.shared_from = share_from
        self.max_ctx = (cfg.max_ctx + 127) // 128 * 128
        self._n_steps = None
        self.general_solver, self.stochastic, self.n_solver_steps = False, False, 0      # what set_num_steps leaves
        if share_from is not None:
            if share_from.device != self.device:
                raise EngineError("a shared engine lives on its owner's device")
            rc = self.lib.vv_create_shared(C.byref(c), share_from._ctx, C.byref(self._ctx))
            if rc != 0:
                msg = self._err()
                if self._ctx:
                    self.lib.vv_destroy(self._ctx)
                    self._ctx = C.c_void_p()
                raise EngineError("vv_create_shared failed: " + msg)
            self._loaded = set(share_from._loaded)
            return
        rc = self.lib.vv_create(C.byref(c), C.byref(self._ctx))
        if rc != 0:
            raise EngineError("vv_create failed: " + self._err())
        self._loaded = set()
        # HF Qwen2RotaryEmbedding inv_freq, computed exactly as transformers does
        d = cfg.lm_head_dim
        inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
        self.upload("lm.rope.inv_freq", inv_freq)

    def fork(self, **runtime) -> "Engine":
        """A second engine over this engine's weights (one copy in HBM) with its own runtime state and stream; runtime: n_slots, max_ctx,
        max_rows, attn_splits, use_graph overrides.  Two engines driven from two host threads interleave two independent utterance
        batches on the GPU: each chain's launch boundaries are filled by the other's kernels."""
        import dataclasses
        owner = self.shared_from or self
        return Engine(dataclasses.replace(self.cfg, **runtime), self.device, share_from=owner)

    # ------------------------------------------------------------------ plumbing
    def _err(self):
        s = self.lib.vv_last_error(self._ctx)
        return s.decode() if s else "?"

    def _chk(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what} failed: {self._err()}")

    @property
    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    def close(self):
        if self._ctx:
            self.lib.vv_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        """wait for the engine stream, then surface asynchronous device-side errors (vv_check: the prefill GEMM's K-split
        hand-off reports a lost producer through a host word instead of hanging)"""
        self.stream.synchronize()
        if self._ctx:
            self._chk(self.lib.vv_check(self._ctx, self._s), "vv_check")
            self._warn_capture_fallbacks()
            n = int(self.lib.vv_stat(self._ctx, 5))
            if n:
                # an invariant of the library, checked where every generate() ends: a memset node of a replayed hipGraph was seen to
                # fill with stale words on this runtime, so captured sequences hold kernel launches only
                raise RuntimeError(f"vibevoice_amd: {n} memset / memcpy node(s) inside this engine's captured hipGraphs -- a copy or fill "
                                   "was enqueued with hipMemsetAsync / hipMemcpyAsync inside a captured sequence; use the library's copy "
                                   "and fill kernels (csrc/misc.hip: vv_copy_launch, vv_zero_launch)")

    def _warn_capture_fallbacks(self):
        """One warning per engine the first time a stream capture did not close and its work ran eagerly instead (vv_stat(ctx, 4) > 0):
        the step is still correct, but that launch sequence will be enqueued kernel by kernel from now on -- a serving process that
        lost its graphs should hear about it.  The known cause is a device-wide synchronize (torch.cuda.synchronize(),
        hipDeviceSynchronize) in ANOTHER host thread while this engine was capturing: synchronize streams or events instead."""
        if getattr(self, "_fallback_warned", False) or not self._ctx:
            return
        n = int(self.lib.vv_stat(self._ctx, 4))
        if n > 0:
            self._fallback_warned = True
            import warnings
            warnings.warn(f"vibevoice_amd: {n} hipGraph capture(s) of this engine did not close and ran eagerly instead -- those launch sequences "
                          "stay un-graphed (slower steps, same results).  Usual cause: another host thread called a device-wide synchronize "
                          "(torch.cuda.synchronize()) during the capture; synchronize streams or events in a process that generates.",
                          RuntimeWarning, stacklevel=3)

    def new(self, *shape, dtype=torch.float32):
        """zero tensor whose fill is ordered on the engine stream"""
        with torch.cuda.stream(self.stream):
            return torch.zeros(*shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ parameters
    def expected_weights(self) -> Dict[str, int]:
        out = {}
        buf = C.create_string_buffer(256)
        n = C.c_int64()
        ld = C.c_int()
        for i in range(self.lib.vv_num_weights(self._ctx)):
            self._chk(self.lib.vv_weight_info(self._ctx, i, buf, 256, C.byref(n), C.byref(ld)), "vv_weight_info")
            out[buf.value.decode()] = n.value
        return out

    def missing_weights(self) -> List[str]:
        miss = []
        buf = C.create_string_buffer(256)
        n = C.c_int64()
        ld = C.c_int()
        for i in range(self.lib.vv_num_weights(self._ctx)):
            self.lib.vv_weight_info(self._ctx, i, buf, 256, C.byref(n), C.byref(ld))
            if not ld.value:
                miss.append(buf.value.decode())
        return miss

    def upload(self, name: str, t: torch.Tensor):
        """t: fp32 or bf16 tensor on any device (host tensors are staged)."""
        t = t.detach()
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.to(torch.float32)
        t = t.contiguous()
        # the tensor must exist before the library reads it (vv_upload works on the null stream).  The producing stream only: a
        # device-wide synchronize from one host thread invalidates a stream capture another thread's context has open (lanes)
        torch.cuda.current_stream(self.device).synchronize()
        rc = self.lib.vv_upload(self._ctx, name.encode(), C.c_void_p(t.data_ptr()),
                                1 if t.dtype == torch.bfloat16 else 0, t.numel())
        self._chk(rc, f"vv_upload({name})")
        self._loaded.add(name)
        # state the engine DERIVES from parameters must follow them (load_state_dict on a live model, LoRA merges): the
        # timestep-embedding table comes from head.t_embedder, the packed valid-token rows from lm_head / embed_tokens
        if name.startswith("head."):
            self._n_steps = None
        if name in ("lm.embed_tokens.weight", "lm_head.weight") and getattr(self, "_valid_ids", None):
            self.set_valid_tokens(self._valid_ids)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], mapped=False, strict=True):
        """sd keyed by reference names (model.language_model....) unless mapped=True."""
        exp = self.expected_weights()
        for k, v in sd.items():
            name = k if mapped else map_param_name(k)
            if name is None or name not in exp:
                continue
            self.upload(name, v)
        if strict:
            miss = self.missing_weights()
            if miss:
                raise EngineError(f"{len(miss)} parameters were not provided, e.g. {miss[:5]}")

    def set_speech_factors(self, scaling: float, bias: float):
        self._chk(self.lib.vv_set_speech_factors(self._ctx, float(scaling), float(bias)), "vv_set_speech_factors")

    def set_valid_tokens(self, ids: Sequence[int]):
        arr = (C.c_int * len(ids))(*[int(i) for i in ids])
        self._chk(self.lib.vv_set_valid_tokens(self._ctx, arr, len(ids)), "vv_set_valid_tokens")
        self.n_valid = len(ids)
        self._valid_ids = [int(i) for i in ids]

    def set_num_steps(self, n_steps: int, t_cast_bf16: bool = False, algorithm_type: str = "dpmsolver++", solver: Optional[dict] = None):
        """Solver table for N steps.  algorithm_type: "dpmsolver++" (the model classes' scheduler) or "sde-dpmsolver++" (what
        demo/gradio_demo.py:142-146 installs); the stochastic one is sampled with diffusion_sample(..., step_noise=...).
        solver: the non-default sampling-time settings of the reference scheduler (schedule.SAMPLING_KEYS: solver_order,
        solver_type, lower_order_final, euler_at_final, final_sigmas_type, timestep_spacing, steps_offset, lambda_min_clipped) as a
        dict.  Settings equal to a shipped configuration -- None, an empty dict, defaults spelled out -- keep the shipped table and
        sampler; anything else installs the general table (schedule.make_general_table) and diffusion_sample routes to the general
        sampler.  n_solver_steps is then what the reference's set_timesteps(n_steps) yields."""
        cfg = dict(solver or {}, algorithm_type=str(algorithm_type))
        unknown = sorted(set(cfg) - set(_schedule.SAMPLING_KEYS))
        if unknown:
            raise ValueError(f"set_num_steps: {unknown} are not sampling-time settings {_schedule.SAMPLING_KEYS}")
        general = not _schedule.is_shipped(cfg)
        key = (int(n_steps), bool(t_cast_bf16), str(algorithm_type)) + ((tuple(sorted(_schedule.solver_settings(cfg).items())),) if general else ())
        if self._n_steps == key:
            return
        if general:
            tv, coef = _schedule.make_general_table(cfg, n_steps, t_cast_bf16)
            stochastic = algorithm_type == "sde-dpmsolver++"
        else:
            tv, coef = _schedule.make_table(n_steps, t_cast_bf16, algorithm_type)
            stochastic = coef.shape[1] == 6
        name = "vv_set_schedule_general" if general else "vv_set_schedule_sde" if stochastic else "vv_set_schedule"
        fp = C.POINTER(C.c_float)
        self._chk(getattr(self.lib, name)(self._ctx, len(tv), tv.ctypes.data_as(fp), np.ascontiguousarray(coef).ctypes.data_as(fp),
                                          *((int(stochastic),) if general else ()), self._s), name)
        self._n_steps = key
        self.n_solver_steps = len(tv)
        self.stochastic = stochastic
        self.general_solver = general

    # ------------------------------------------------------------------ ops
    @staticmethod
    def _p(t: Optional[torch.Tensor]):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()

    @staticmethod
    def _rows(rows):
        """(cache, pos) pairs -> a VVRow array without a per-row Python loop (a 10,922-row prompt chunk is one call)"""
        a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
        return (_lib.VVRow * a.shape[0]).from_buffer(a), a

    def lm_forward(self, rows: Sequence[tuple], x_in: torch.Tensor, hidden_out: torch.Tensor):
        arr, keep = self._rows(rows)
        self._chk(self.lib.vv_lm_forward(self._ctx, self._s, len(arr), arr, self._p(x_in), self._p(hidden_out)), "vv_lm_forward")

    def lm_forward_span(self, cache: int, pos0: int, n: int, x_in: torch.Tensor, hidden_out: torch.Tensor):
        """n consecutive positions pos0 .. pos0+n-1 of one cache (a prompt chunk)"""
        a = np.empty((n, 2), dtype=np.int32)
        a[:, 0] = cache
        a[:, 1] = np.arange(pos0, pos0 + n, dtype=np.int32)
        arr = (_lib.VVRow * n).from_buffer(a)
        self._chk(self.lib.vv_lm_forward(self._ctx, self._s, n, arr, self._p(x_in), self._p(hidden_out)), "vv_lm_forward")

    def lm_forward_range(self, rows: Sequence[tuple], x_in: torch.Tensor, hidden_out: torch.Tensor, l0: int, l1: int,
                         final_norm: bool):
        arr, keep = self._rows(rows)
        n = len(arr)
        self._chk(self.lib.vv_lm_forward_range(self._ctx, self._s, n, arr, self._p(x_in), self._p(hidden_out),
                                               int(l0), int(l1), int(final_norm)), "vv_lm_forward_range")

    def kv_import(self, cache: int, layer: int, k: torch.Tensor, v: torch.Tensor):
        """k, v: [kv_heads, n_pos, head_dim] (keys already rotated), fp32 or bf16, on the engine device."""
        assert k.shape == v.shape and k.dim() == 3
        k = k.contiguous()
        v = v.contiguous()
        if k.dtype not in (torch.float32, torch.bfloat16):
            k, v = k.float(), v.float()
        self._chk(self.lib.vv_kv_import(self._ctx, self._s, cache, layer, k.shape[1], self._p(k), self._p(v),
                                        1 if k.dtype == torch.bfloat16 else 0), "vv_kv_import")

    def kv_move(self, cache: int, src_pos: int, dst_pos: int):
        """cached position src_pos copied onto dst_pos, every layer of `cache` (keys keep their rotation)"""
        self._chk(self.lib.vv_kv_move(self._ctx, self._s, int(cache), int(src_pos), int(dst_pos)), "vv_kv_move")

    def kv_import_at(self, cache: int, layer: int, pos0: int, k: torch.Tensor, v: torch.Tensor):
        """k, v: [kv_heads, n_pos, head_dim] -> cache positions [pos0, pos0 + n_pos)."""
        assert k.shape == v.shape and k.dim() == 3
        k = k.contiguous()
        v = v.contiguous()
        if k.dtype not in (torch.float32, torch.bfloat16):
            k, v = k.float(), v.float()
        self._chk(self.lib.vv_kv_import_at(self._ctx, self._s, cache, layer, int(pos0), k.shape[1], self._p(k), self._p(v),
                                           1 if k.dtype == torch.bfloat16 else 0), "vv_kv_import_at")

    def kv_export(self, cache: int, layer: int, pos0: int, n_pos: int, dtype=torch.bfloat16):
        """positions [pos0, pos0 + n_pos) of one layer of `cache` in HF layout: (k, v), each [kv_heads, n_pos, head_dim] (keys as
        cached, rotated), fp32 or bf16 -- the exact inverse of kv_import_at."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise EngineError(f"kv_export: dtype {dtype} (torch.float32 or torch.bfloat16)")
        with torch.cuda.stream(self.stream):
            k = torch.empty(self.cfg.lm_kv_heads, max(0, int(n_pos)), self.cfg.lm_head_dim, dtype=dtype, device=self.device)
            v = torch.empty_like(k)
        self._chk(self.lib.vv_kv_export(self._ctx, self._s, int(cache), int(layer), int(pos0), int(n_pos), self._p(k), self._p(v),
                                        1 if dtype == torch.bfloat16 else 0), "vv_kv_export")
        return k, v

    def kv_snapshot_numel(self, n_pos: int) -> int:
        """bf16 elements of ONE of the two snapshot buffers (K or V) for n_pos positions"""
        nb = int(self.lib.vv_kv_snapshot_bytes(self._ctx, int(n_pos)))
        if nb < 0:
            raise EngineError(f"vv_kv_snapshot_bytes failed: {self._err()}")
        return nb // 2

    def kv_snapshot(self, cache: int, n_pos: int):
        """positions [0, n_pos) of every layer of `cache` as two compact bf16 device tensors (k, v), each
        [layers, kv_heads, ceil32(n_pos) * head_dim] in the cache's tile layouts; slots past n_pos are zero.  Independent of max_ctx:
        any engine over the same model (a fork() with another max_ctx) restores it."""
        n = self.kv_snapshot_numel(n_pos)
        per_head = n // (self.cfg.lm_layers * self.cfg.lm_kv_heads)
        with torch.cuda.stream(self.stream):
            k = torch.empty(self.cfg.lm_layers, self.cfg.lm_kv_heads, per_head, dtype=torch.bfloat16, device=self.device)
            v = torch.empty_like(k)
        self._chk(self.lib.vv_kv_snapshot(self._ctx, self._s, int(cache), int(n_pos), self._p(k), self._p(v)), "vv_kv_snapshot")
        return k, v

    def kv_restore(self, cache: int, n_pos: int, k: torch.Tensor, v: torch.Tensor):
        """the inverse of kv_snapshot, into positions [0, ceil32(n_pos)) of `cache`, every layer; append behind n_pos afterwards"""
        n = self.kv_snapshot_numel(n_pos)
        for t in (k, v):
            if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.numel() != n or t.device != self.device:
                raise EngineError(f"kv_restore: a snapshot of {n_pos} positions is a contiguous bf16 tensor of {n} elements on {self.device}")
        self._chk(self.lib.vv_kv_restore(self._ctx, self._s, int(cache), int(n_pos), self._p(k), self._p(v)), "vv_kv_restore")

    def add_type_embedding(self, n: int, x: torch.Tensor, type_id: int, out: torch.Tensor):
        self._chk(self.lib.vv_add_type_embedding(self._ctx, self._s, n, self._p(x), int(type_id), self._p(out)),
                  "vv_add_type_embedding")

    def eos_logit(self, n: int, hidden: torch.Tensor, out: torch.Tensor):
        self._chk(self.lib.vv_eos_logit(self._ctx, self._s, n, self._p(hidden), self._p(out)), "vv_eos_logit")

    @property
    def embed_chunk(self) -> int:
        """token ids one vv_embed call takes: max(64, max_rows)"""
        return max(64, int(self.cfg.max_rows))

    def embed(self, ids: Sequence[int], out: torch.Tensor):
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        arr = (C.c_int * a.shape[0]).from_buffer(a)
        self._chk(self.lib.vv_embed(self._ctx, self._s, a.shape[0], arr, self._p(out)), "vv_embed")

    def lm_logits(self, n: int, hidden: torch.Tensor, logits_out: torch.Tensor):
        self._chk(self.lib.vv_lm_logits(self._ctx, self._s, n, self._p(hidden), self._p(logits_out)), "vv_lm_logits")

    def lm_logits_full(self, n: int, hidden: torch.Tensor, logits_out: torch.Tensor):
        """logits over the whole vocabulary, [n, lm_vocab] fp32 (the full-vocabulary logits processors' input)"""
        assert logits_out.dtype == torch.float32 and logits_out.is_contiguous() and logits_out.numel() >= n * self.cfg.lm_vocab
        self._chk(self.lib.vv_lm_logits_full(self._ctx, self._s, n, self._p(hidden), self._p(logits_out)), "vv_lm_logits_full")

    def lm_warp_valid(self, n: int, logits: torch.Tensor, seen: Optional[torch.Tensor], out: torch.Tensor, survivors: torch.Tensor, *,
                      repetition_penalty: float = 1.0, temperature: float = 1.0, do_sample: bool = False, top_k: int = 0,
                      top_p: float = 1.0, min_p: float = 0.0):
        """The full-vocabulary logits processors + the valid-id constraint for n <= 16 rows of lm_logits_full's output (read only):
        out[:n * n_valid] = the processed scores of the valid ids, -inf where a filter removed one; survivors[:n] = finite entries per
        row.  seen: [n, lm_vocab] uint8, non-zero where the id is in the row's input_ids (None when repetition_penalty == 1)."""
        V = self.cfg.lm_vocab
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= n * V
        assert seen is None or (seen.dtype == torch.uint8 and seen.is_contiguous() and seen.numel() >= n * V)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n * max(1, getattr(self, "n_valid", 0) or 0)
        assert survivors.dtype == torch.int32 and survivors.is_contiguous() and survivors.numel() >= n
        self._chk(self.lib.vv_lm_warp_valid(self._ctx, self._s, int(n), self._p(logits), self._p(seen), float(repetition_penalty),
                                            float(temperature), int(bool(do_sample)), int(top_k), float(top_p), float(min_p),
                                            self._p(out), self._p(survivors)), "vv_lm_warp_valid")

    def noise_rows(self, keys: Sequence[tuple], stream0: int, n_streams: int, n_t: int, width: int, out: torch.Tensor):
        """The normals of seeded requests (vibevoice_amd/noise.py), on the device: out[s][r][f][j] for stream ids stream0 + s
        (s < n_streams), rows r = keys[r] = (seed, t0, aux), counter words t = t0 + f (f < n_t), j < width.  out: contiguous fp32 on
        the engine device with at least n_streams * len(keys) * n_t * width elements; nothing else is written."""
        from . import noise as _noise
        n = len(keys)
        arr = (_lib.VVNoiseKey * max(1, n))()
        for i, (seed, t0, aux) in enumerate(keys):
            seed = _noise.check_seed(seed)
            arr[i].seed_lo, arr[i].seed_hi, arr[i].t0, arr[i].aux = seed & 0xffffffff, seed >> 32, int(t0) & 0xffffffff, int(aux) & 0xffffffff
        if out is not None:
            if out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
                raise ValueError(f"noise_rows: out is a contiguous fp32 tensor on {self.device}")
            if n >= 1 and n_streams >= 1 and n_t >= 1 and width >= 1 and out.numel() < int(n_streams) * n * int(n_t) * int(width):
                raise ValueError(f"noise_rows: out holds {out.numel()} elements, {int(n_streams) * n * int(n_t) * int(width)} are written")
        self._chk(self.lib.vv_noise_rows(self._ctx, self._s, n, arr, int(stream0) & 0xffffffff, int(n_streams), int(n_t), int(width),
                                         self._p(out)), "vv_noise_rows")

    def diffusion_sample(self, n: int, cond: torch.Tensor, noise: torch.Tensor, cfg_scale, latent_out: torch.Tensor,
                         step_noise: Optional[torch.Tensor] = None):
        """step_noise [n_steps, n, latent] fp32 (contiguous, on the device): the per-step variance noise of the stochastic solver.
        cfg_scale: one float for every row, or a 1-D fp32 device tensor of n guidance scales, one per utterance row.  The kernels read
        the tensor at run time and the graph is keyed by its address: rewrite the same buffer between calls and nothing is re-captured."""
        rows = isinstance(cfg_scale, torch.Tensor)
        if rows and (cfg_scale.dim() != 1 or cfg_scale.shape[0] != n or cfg_scale.dtype != torch.float32 or cfg_scale.device != self.device
                     or not cfg_scale.is_contiguous()):
            raise ValueError(f"diffusion_sample: a per-row cfg_scale is a contiguous 1-D fp32 tensor of n = {n} entries on {self.device}")
        if step_noise is not None:      # every entry point reads n_solver_steps rows of n latents
            assert step_noise.dtype == torch.float32 and step_noise.is_contiguous() and step_noise.shape[1] == n
            assert step_noise.shape[0] >= self.n_solver_steps
        head, sn, out = (self._ctx, self._s, n, self._p(cond), self._p(noise)), self._p(step_noise), self._p(latent_out)
        if self.general_solver:         # routed by the installed table (set_num_steps(..., solver=...))
            name, args = "vv_diffusion_sample_general", (sn, 0.0 if rows else float(cfg_scale), self._p(cfg_scale) if rows else C.c_void_p(), out)
        elif rows:
            name, args = "vv_diffusion_sample_rows", (sn, self._p(cfg_scale), out)
        elif step_noise is None:
            name, args = "vv_diffusion_sample", (float(cfg_scale), out)
        else:
            name, args = "vv_diffusion_sample_sde", (sn, float(cfg_scale), out)
        self._chk(getattr(self.lib, name)(*head, *args), name)

    def head_forward(self, noisy: torch.Tensor, t: float, cond: torch.Tensor, out: torch.Tensor):
        n = noisy.shape[0]
        tarr = (C.c_float * n)(*([float(t)] * n))
        self._chk(self.lib.vv_head_forward(self._ctx, self._s, n, self._p(noisy), tarr, self._p(cond), self._p(out)),
                  "vv_head_forward")

    def _sp(self, stream):
        """hipStream_t of an optional torch stream (default: the engine's own stream)"""
        return self._s if stream is None else C.c_void_p(stream.cuda_stream)

    def codec_decode(self, slot: int, latent: torch.Tensor, audio_out: torch.Tensor, apply_speech_factors=True, stream=None):
        self._chk(self.lib.vv_codec_decode(self._ctx, self._sp(stream), slot, 1, self._p(latent), self._p(audio_out),
                                           int(apply_speech_factors)), "vv_codec_decode")

    def semantic_encode(self, slot: int, audio: torch.Tensor, sem_out: torch.Tensor, stream=None):
        self._chk(self.lib.vv_semantic_encode(self._ctx, self._sp(stream), slot, 1, self._p(audio), self._p(sem_out)),
                  "vv_semantic_encode")

    def codec_chain_batch(self, slots, latent: torch.Tensor, audio_out: torch.Tensor, sem_out=None, apply_speech_factors=True):
        """One frame of len(slots) utterances through the acoustic decoder and (sem_out given) the semantic encoder: row j of
        latent [n, latent] / audio_out [n, hop] / sem_out [n, sem_dim] belongs to streaming slot slots[j].  The reference
        decodes / re-encodes the step's diffusion rows as one batch (modeling_vibevoice_inference.py:636-672); here the
        weight-heavy stages of both nets read their weights once for the whole batch."""
        n = len(slots)
        assert latent.is_contiguous() and audio_out.is_contiguous() and (sem_out is None or sem_out.is_contiguous())
        arr = (C.c_int * n)(*[int(s) for s in slots])
        self._chk(self.lib.vv_codec_chain_batch(self._ctx, self._s, n, arr, self._p(latent), self._p(audio_out),
                                                self._p(sem_out) if sem_out is not None else None, int(apply_speech_factors)),
                  "vv_codec_chain_batch")

    def acoustic_encode(self, frames: int, wav: torch.Tensor, mean_out: torch.Tensor, valid_samples: Optional[int] = None):
        """wav [frames * hop] -> mean_out [frames, latent].  valid_samples: real signal length when it does not fill the last frame (wav is
        zero beyond it): the reference's per-conv-layer right padding is reproduced (vv_acoustic_encode_ragged)."""
        if valid_samples is None or valid_samples >= frames * self.cfg.hop:
            self._chk(self.lib.vv_acoustic_encode(self._ctx, self._s, frames, self._p(wav), self._p(mean_out)), "vv_acoustic_encode")
        else:
            self._chk(self.lib.vv_acoustic_encode_ragged(self._ctx, self._s, frames, int(valid_samples), self._p(wav), self._p(mean_out)),
                      "vv_acoustic_encode_ragged")

    def set_enc_pass_frames(self, frames_per_pass: int):
        """frames per voice-prompt encoder pass, 1..cfg.enc_frames"""
        self._chk(self.lib.vv_set_enc_pass_frames(self._ctx, int(frames_per_pass)), "vv_set_enc_pass_frames")

    def audio_to_pcm16(self, audio: torch.Tensor, pcm_out: torch.Tensor, stream=None):
        """audio [n, samples] fp32 (contiguous) -> pcm_out [n, samples] int16, per-chunk peak normalisation as the reference's
        convert_to_16_bit_wav (demo/gradio_demo.py:1058-1073)."""
        n, samples = audio.shape
        assert audio.is_contiguous() and pcm_out.is_contiguous() and pcm_out.dtype == torch.int16 and audio.dtype == torch.float32
        self._chk(self.lib.vv_audio_to_pcm16(self._ctx, self._sp(stream), n, samples, self._p(audio), self._p(pcm_out)),
                  "vv_audio_to_pcm16")

    # ------------------------------------------------------------------ streaming row stages and their whole-signal forms
    _STAGE_USED = {"resampler": "_rs_used", "tempo": "_tp_used", "pitch": "_pt_used", "formant": "_fm_used", "level": "_lv_used", "loudness": "_ld_used",
                   "pause": "_ps_used"}

    def _take_stage_slot(self, kind, make):
        """make(k) for the first free k of this engine's four `kind` configurations; the stage's close() gives k back"""
        used = self.__dict__.setdefault(self._STAGE_USED[kind], [None] * 4)
        for k in range(len(used)):
            if used[k] is None:
                used[k] = s = make(k)
                return s
        raise EngineError(f"Engine.{kind}: all 4 {kind} configurations of this engine are in use; close() one")

    def _whole(self, what, audio, n_out, run, stream, aux_cols=0):
        """Whole signals through a stateless kernel: audio [samples] or [n, samples] as contiguous fp32 rows on the engine's device,
        run(hipStream_t, rows, samples, x, out, aux) per 65535 rows (the grid's limit), out and the int32 aux (aux_cols > 0) offset to
        the tile's first row -> (out [..., n_out] fp32, aux [n, aux_cols] or None)"""
        x = audio.detach().to(device=self.device, dtype=torch.float32)
        if x.dim() not in (1, 2):
            raise ValueError(f"Engine.{what}: audio is [samples] or [n, samples], got {tuple(audio.shape)}")
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        n, n_in = x2.shape
        out = torch.empty((n, n_out), dtype=torch.float32, device=self.device)
        aux = torch.zeros((n, aux_cols), dtype=torch.int32, device=self.device) if aux_cols else None
        if n and n_in:
            st = self._sp(stream if stream is not None else torch.cuda.current_stream(self.device))
            for i0 in range(0, n, 65535):
                run(st, min(65535, n - i0), n_in, x2[i0:], out[i0:], aux[i0:] if aux is not None else None)
        return out.reshape(x.shape[:-1] + (n_out,)), aux

    # audio at another sample rate (resample.py, csrc/resample.hip)
    def resampler(self, src_rate: int, dst_rate: int, n_streams: int) -> "Resampler":
        """A streaming resampler src_rate -> dst_rate with n_streams independent streams, in one of this engine's four resampler
        configurations (close() it to give the configuration back)."""
        return self._take_stage_slot("resampler", lambda k: Resampler(self, k, src_rate, dst_rate, n_streams))

    def resample(self, audio: torch.Tensor, src_rate: int, dst_rate: int, stream=None) -> torch.Tensor:
        """Whole signals at another rate: audio [samples] or [n, samples] (any float dtype, any device) -> fp32 on the engine's device,
        ceil(samples * dst / src) samples each, the definition of vibevoice_amd/resample.py.  Stateless; runs on `stream` (default:
        the current torch stream of the device, the one that produced a device tensor)."""
        from . import resample as _rs
        L, M, T, coef = _rs.design(src_rate, dst_rate)
        n_out = _rs.total_out(int(audio.shape[-1]), L, M) if audio.dim() else 0

        def run(st, nn, n_in, x, out, _):
            cache = self.__dict__.setdefault("_rs_coef", {})
            cd = cache.get((L, M, T))
            if cd is None:
                cd = cache[(L, M, T)] = torch.from_numpy(np.array(coef)).to(self.device)
            self._chk(self.lib.vv_resample_once(self._ctx, st, L, M, T, self._p(cd), nn, n_in, self._p(x), n_in, self._p(out), n_out), "vv_resample_once")
        return self._whole("resample", audio, n_out, run, stream)[0]

    # speaking rate (tempo.py, csrc/tempo.hip)
    def tempo(self, n_streams: int) -> "Tempo":
        """A streaming tempo change with n_streams independent streams, each at its own speed, in one of this engine's four tempo
        configurations (close() it to give the configuration back)."""
        return self._take_stage_slot("tempo", lambda k: Tempo(self, k, n_streams))

    def _tempo_window(self):
        from . import tempo as _tp
        w = self.__dict__.get("_tp_window")
        if w is None:
            w = self.__dict__["_tp_window"] = torch.from_numpy(np.array(_tp.window())).to(self.device)
        return w

    def time_stretch(self, audio: torch.Tensor, speed: float, stream=None, return_offsets: bool = False):
        """Whole signals at another speaking rate, the pitch kept: audio [samples] or [n, samples] (24 kHz, any float dtype, any
        device) -> fp32 on the engine's device, ceil(samples * Q / P) samples each for speed = P / Q in [0.5, 2.0], the definition of
        vibevoice_amd/tempo.py.  Stateless; runs on `stream` (default: the current torch stream of the device).  return_offsets:
        -> (out, offsets), offsets int32 [..., blocks]: the offset the search chose for each block of 240 output samples."""
        from . import tempo as _tp
        P, Q = _tp.ratio(speed)
        n_out = _tp.total_out(int(audio.shape[-1]), P, Q) if audio.dim() else 0
        nblk = -(-n_out // _tp.HS)

        def run(st, nn, n_in, x, out, offs):
            self._chk(self.lib.vv_tempo_once(self._ctx, st, self._p(self._tempo_window()), P, Q, nn, n_in, self._p(x), n_in, self._p(out), n_out,
                                             self._p(offs) if offs is not None else None, max(nblk, 1)), "vv_tempo_once")
        out, offs = self._whole("time_stretch", audio, n_out, run, stream, aux_cols=max(nblk, 1) if return_offsets else 0)
        return (out, offs[:, :nblk].reshape(out.shape[:-1] + (nblk,))) if return_offsets else out

    # pitch (pitch.py, csrc/pitch.hip)
    def pitch(self, n_streams: int) -> "Pitch":
        """A streaming variable-ratio resampler with n_streams independent streams, each at the ratio of its own shift in semitones,
        in one of this engine's four pitch configurations (close() it to give the configuration back).  Behind a tempo stage at
        speed Q / P it moves the pitch and keeps the duration."""
        return self._take_stage_slot("pitch", lambda k: Pitch(self, k, n_streams))

    def _pitch_table(self):
        from . import pitch as _pt
        h = self.__dict__.get("_pt_table")
        if h is None:
            h = self.__dict__["_pt_table"] = torch.from_numpy(np.array(_pt.table())).to(self.device)
        return h

    def pitch_shift(self, audio: torch.Tensor, semitones, speed: float = 1.0, stream=None, formant=None) -> torch.Tensor:
        """Whole signals at another pitch: audio [samples] or [n, samples] (24 kHz, any float dtype, any device) -> fp32 on the engine's
        device, moved by `semitones` in [-12, +12] and played at `speed`: time_stretch() at speed * Q / P (none where that is exactly
        1), then pitch_resample() at P / Q = ratio(semitones), the definition of vibevoice_amd/pitch.py (shift_ref):
        ceil(ceil(n Qt / Pt) Q / P) samples.  formant=None: a resampling shifter, the formants move with the pitch.  formant=F (semitones
        in [-12, +12]): formant_warp() at ratio(F) * Q / P between the two (vibevoice_amd/formant.py), so the formants end up F semitones
        from the untouched voice's -- 0.0 keeps them.  A combined speed outside [0.5, 2.0] is refused, and so is a warp outside [1/2, 2].
        Stateless; runs on `stream` (default: the current torch stream of the device)."""
        from . import pitch as _pt
        from . import tempo as _tp
        P, Q = _pt.ratio(semitones)
        v = _pt.tempo_speed(speed, semitones)
        ab = None
        if formant is not None:
            from . import formant as _fm
            ab = _fm.fraction(formant, semitones)
        if _tp.ratio(v) != (1, 1):
            audio = self.time_stretch(audio, v, stream=stream)
        if ab is not None and ab != (1, 1):
            audio = self.formant_warp(audio, fractions=ab, stream=stream)
        if P == Q:
            return audio.detach().to(device=self.device, dtype=torch.float32)
        out, counts = self.pitch_resample(audio, semitones, stream=stream)
        return out[..., :counts[0]] if counts else out

    def pitch_resample(self, audio: torch.Tensor, semitones, stream=None):
        """The pitch stage alone over whole signals: audio [samples] or [n, samples] -> (out fp32 [..., max(counts)], counts): row i
        resampled at P / Q = ratio(semitones[i]) (or one value for all rows), counts[i] = ceil(samples * Q / P) samples of it (what lies
        behind them is not written).  Pitch and duration both change by the ratio.  Stateless; one launch per 16 rows, each row at its own ratio."""
        from . import pitch as _pt
        rows = int(audio.numel() // audio.shape[-1]) if audio.dim() and audio.shape[-1] else 0
        semis = [semitones] * rows if not hasattr(semitones, "__len__") else list(semitones)
        if len(semis) != rows:
            raise ValueError(f"Engine.pitch_resample: semitones names one value, or one per row ({rows}), got {len(semis)}")
        pq = [_pt.ratio(s) for s in semis]
        counts = [_pt.total_out(int(audio.shape[-1]), P, Q) for P, Q in pq]
        n_out = max(counts, default=0)

        def run(st, nn, n_in, x, out, _):
            h = self._pitch_table()
            i0 = rows - int(x.shape[0])                        # _whole hands over the tile's first row onwards
            flat = [v for P, Q in pq[i0:i0 + nn] for v in (P, Q)]
            self._chk(self.lib.vv_pitch_once(self._ctx, st, self._p(h), int(h.shape[0]), _pt.R, nn, (C.c_int * (2 * nn))(*flat), n_in, self._p(x),
                                             n_in, self._p(out), n_out), "vv_pitch_once")
        return self._whole("pitch_resample", audio, n_out, run, stream)[0], counts

    # formants (formant.py, csrc/formant.hip)
    def formant(self, n_streams: int) -> "Formant":
        """A streaming spectral-envelope warp with n_streams independent streams, each at its own fraction A / B, in one of this
        engine's four formant configurations (close() it to give the configuration back).  Alone it moves the formants and keeps the
        pitch; in front of a pitch stage at P / Q, at Q / P, it keeps the formants where they were."""
        return self._take_stage_slot("formant", lambda k: Formant(self, k, n_streams))

    def _formant_table(self):
        from . import formant as _fm
        t = self.__dict__.get("_fm_table")
        if t is None:
            t = self.__dict__["_fm_table"] = torch.from_numpy(np.array(_fm.twiddles())).to(self.device)
        return t

    def formant_warp(self, audio: torch.Tensor, semitones=None, stream=None, fractions=None) -> torch.Tensor:
        """Whole signals with their formants moved and their pitch kept: audio [samples] or [n, samples] (24 kHz, any float dtype, any
        device) -> fp32 on the engine's device, as many samples, the definition of vibevoice_amd/formant.py.  semitones in [-12, +12]: one
        value, or one per row (the warp is pitch.ratio of it); fractions: the warp (A, B) itself, or one per row, in place of semitones.
        A row at 1 / 1 is copied.  Stateless; two launches per 16 rows, each row at its own warp, on `stream` (default: the current
        torch stream of the device)."""
        from . import formant as _fm
        rows = int(audio.numel() // audio.shape[-1]) if audio.dim() and audio.shape[-1] else 0
        ab = _fm_fractions(_fm, "Engine.formant_warp", rows, semitones, fractions)
        n_out = int(audio.shape[-1]) if audio.dim() else 0
        ts = stream if stream is not None else torch.cuda.current_stream(self.device)

        def run(st, nn, n_in, x, out, _):
            tw = self._formant_table()
            i0 = rows - int(x.shape[0])                        # _whole hands over the tile's first row onwards
            flat = [v for A, B in ab[i0:i0 + nn] for v in (A, B)]
            floats = min(nn, 16) * (-(-n_in // _fm.H) + 3) * _fm.N
            with torch.cuda.stream(ts):                        # the frames between the two launches: this stream's
                scratch = torch.empty(floats, dtype=torch.float32, device=self.device)
            self._chk(self.lib.vv_formant_once(self._ctx, st, self._p(tw), nn, (C.c_int * (2 * nn))(*flat), n_in, self._p(x), n_in, self._p(out),
                                               n_out, self._p(scratch), floats), "vv_formant_once")
        return self._whole("formant_warp", audio, n_out, run, stream)[0]

    # output level (level.py, csrc/level.hip)
    def level(self, n_streams: int, rate: int = 24000, ceiling_db: float = -1.0) -> "Level":
        """A streaming gain and look-ahead peak limiter at `rate` Hz under the ceiling `ceiling_db`, with n_streams independent streams,
        each at its own volume, in one of this engine's four level configurations (close() it to give the configuration back)."""
        return self._take_stage_slot("level", lambda k: Level(self, k, n_streams, rate, ceiling_db))

    def apply_level(self, audio: torch.Tensor, volume_db: float = 0.0, ceiling_db: float = -1.0, rate: int = 24000, stream=None) -> torch.Tensor:
        """Whole signals at another level: audio [samples] or [n, samples] (at `rate` Hz, any float dtype, any device) -> fp32 on the
        engine's device, as many samples: volume_db of gain, then a look-ahead peak limiter that keeps every sample within ceiling_db
        of full scale (5 ms of look-ahead and ramp, 50 ms of hold), the definition of vibevoice_amd/level.py.  A signal that never
        reaches the ceiling comes back as fl(gain * x) bit for bit.  Stateless; runs on `stream` (default: the current torch stream
        of the device)."""
        from . import level as _lv
        A, H = _lv.params(rate)
        g, c = float(_lv.gain_of(volume_db)), float(_lv.ceiling_of(ceiling_db))
        n_out = int(audio.shape[-1]) if audio.dim() else 0

        def run(st, nn, n_in, x, out, _):
            self._chk(self.lib.vv_level_once(self._ctx, st, A, H, g, c, nn, n_in, self._p(x), n_in, self._p(out), n_out), "vv_level_once")
        return self._whole("apply_level", audio, n_out, run, stream)[0]

    # loudness (loudness.py, csrc/loudness.hip)
    def loudness(self, n_streams: int) -> "Loudness":
        """A streaming adaptive leveller at 24 kHz with n_streams independent streams, each with its own target, in one of this engine's
        four loudness configurations (close() it to give the configuration back)."""
        return self._take_stage_slot("loudness", lambda k: Loudness(self, k, n_streams))

    def _loud_taps(self):
        from . import loudness as _ld
        w = self.__dict__.get("_ld_taps")
        if w is None:
            w = self.__dict__["_ld_taps"] = torch.from_numpy(_ld.taps().astype(np.float64)).to(self.device)
        return w

    def segment_energies(self, audio: torch.Tensor, stream=None, fine: bool = False) -> torch.Tensor:
        """The K-weighted energy of every complete 100 ms segment: audio [samples] or [n, samples] (24 kHz, any float dtype, any device)
        -> int64 [..., samples // 2400] on the engine's device, E / (2400 * 2**32) a segment's mean square: the definition of
        vibevoice_amd/loudness.py, integer for integer.  fine: F, the same sums at 16 times the resolution, F / (2400 * 2**40) the
        mean square (what measure_loudness reads).  Stateless; runs on `stream` (default: the device's current torch stream)."""
        from . import loudness as _ld
        x = audio.detach().to(device=self.device, dtype=torch.float32)
        if x.dim() not in (1, 2):
            raise ValueError(f"Engine.segment_energies: audio is [samples] or [n, samples], got {tuple(audio.shape)}")
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        n, n_in = x2.shape
        n_seg = n_in // _ld.S
        E = torch.empty((n, n_seg), dtype=torch.int64, device=self.device)
        if n and n_seg:
            st = self._sp(stream if stream is not None else torch.cuda.current_stream(self.device))
            for i0 in range(0, n, 65535):
                e = (None, 0, self._p(E[i0:]), n_seg) if fine else (self._p(E[i0:]), n_seg, None, 0)
                self._chk(self.lib.vv_loud_energy(self._ctx, st, self._p(self._loud_taps()), min(65535, n - i0), n_in, self._p(x2[i0:]), n_in, *e),
                          "vv_loud_energy")
        return E.reshape(x.shape[:-1] + (n_seg,))

    def measure_loudness(self, audio: torch.Tensor, stream=None) -> torch.Tensor:
        """The ITU-R BS.1770-4 loudness in LUFS of audio [samples] or [n, samples] at 24 kHz -> a float64 CPU tensor, one value per row
        (a scalar tensor for a 1-D signal); -inf for a signal with no 400 ms block over -70 LUFS or shorter than 400 ms.  The device
        delivers the segment energies, the gating runs on the host over a few numbers per second of audio (this call waits for them)."""
        from . import loudness as _ld
        F = self.segment_energies(audio, stream, fine=True)
        n_rows = int(np.prod(F.shape[:-1]))                         # explicit: a signal under one segment has rows of no energies
        rows = F.reshape(n_rows, F.shape[-1]).cpu().tolist()        # the copy waits for the producing stream
        return torch.tensor([_ld.gated(r, fine=True) for r in rows], dtype=torch.float64).reshape(F.shape[:-1])

    def apply_loudness(self, audio: torch.Tensor, target_lufs: float = -16.0, start_db: float = 0.0, max_boost_db: float = 12.0,
                       return_gain: bool = False, stream=None):
        """Whole signals through the adaptive leveller: audio [samples] or [n, samples] (24 kHz, any float dtype, any device) -> fp32 on
        the engine's device, as many samples, brought towards target_lufs (-36 .. -10) by a gain that follows the loudness of the last
        three seconds of speech (and of the last 400 ms where that is louder), starts at start_db (-24 .. +24) and stays within
        [-24 dB, max_boost_db]: the definition of vibevoice_amd/loudness.py, bit for bit.  No limiter: a boost can pass full scale, run
        apply_level behind it.  return_gain: -> (out, gain), the gain of every sample.  Stateless; runs on `stream`."""
        from . import loudness as _ld
        t, g0, wmax = float(_ld.target_of(target_lufs)), float(_ld.start_of(start_db)), float(_ld.boost_of(max_boost_db))
        n_out = int(audio.shape[-1]) if audio.dim() else 0
        n_seg = max(n_out // _ld.S, 1)
        gains = []

        def run(st, nn, n_in, x, out, _):
            E = torch.empty((nn, n_seg), dtype=torch.int64, device=self.device)
            g = torch.empty((nn, n_out), dtype=torch.float32, device=self.device) if return_gain else None
            gains.append(g)
            self._chk(self.lib.vv_loud_once(self._ctx, st, self._p(self._loud_taps()), t, g0, wmax, nn, n_in, self._p(x), n_in, self._p(out), n_out,
                                            self._p(g) if g is not None else None, n_out, self._p(E), n_seg), "vv_loud_once")
        out = self._whole("apply_loudness", audio, n_out, run, stream)[0]
        if not return_gain:
            return out
        g = torch.cat(gains) if gains else torch.empty((0, n_out), dtype=torch.float32, device=self.device)
        return out, g.reshape(out.shape)

    # pauses (pause.py, csrc/pause.hip)
    def pause(self, n_streams: int, rate: int = 24000) -> "Pause":
        """A streaming pause shortener at `rate` Hz (8000 .. 48000) with n_streams independent streams, each with its own caps and
        threshold, in one of this engine's four pause configurations (close() it to give the configuration back)."""
        return self._take_stage_slot("pause", lambda k: Pause(self, k, n_streams, rate))

    def _pause_weights(self, rate):
        from . import pause as _ps
        cache = self.__dict__.setdefault("_ps_weights", {})
        wt = cache.get(int(rate))
        if wt is None:
            wt = cache[int(rate)] = torch.from_numpy(np.concatenate(_ps.weights(rate))).to(self.device)
        return wt

    def shorten_pauses(self, audio: torch.Tensor, max_pause_ms=None, max_lead_ms=None, threshold_db: float = -50.0, rate: int = 24000,
                       stream=None):
        """Whole signals with their silences capped: audio [samples] or [n, samples] (at `rate` Hz, any float dtype, any device) ->
        (a list of 1-D fp32 tensors on the engine's device, one per signal and of its own length, and the samples each dropped, a list
        of ints): quiet runs (10 ms segments below threshold_db, -80 .. -20) longer than max_pause_ms (100 .. 5000; None: no cap) keep
        their beginning and their end around a 10 ms cross-fade, the run in front of the first loud segment is capped at max_lead_ms
        (0 .. 5000; None: max_pause_ms applies): the definition of vibevoice_amd/pause.py, bit for bit.  A signal with no run above its
        cap comes back as it is.  Stateless; runs on `stream` (default: the device's current torch stream) and waits for it: the
        lengths depend on the data."""
        from . import pause as _ps
        seg, th = _ps.seg_of(rate), _ps.theta(rate, threshold_db)
        Cc, C0 = _ps.caps(rate, max_pause_ms, max_lead_ms)
        n_out = int(audio.shape[-1]) if audio.dim() else 0
        ts = stream if stream is not None else torch.cuda.current_stream(self.device)

        def run(st, nn, n_in, x, out, aux):
            with torch.cuda.stream(ts):                        # the streams' samples during the launch: this stream's
                scratch = torch.empty(nn * _ps.STATE_FLOATS, dtype=torch.float32, device=self.device)
            self._chk(self.lib.vv_pause_once(self._ctx, st, self._p(self._pause_weights(rate)), seg, Cc, C0, th, nn, n_in, self._p(x), n_in,
                                             self._p(out), n_out, self._p(scratch), scratch.numel(), self._p(aux)), "vv_pause_once")
        out, aux = self._whole("shorten_pauses", audio, n_out, run, ts, aux_cols=2)
        rows = out.reshape(-1, n_out)
        if not n_out:
            return [rows[i] for i in range(rows.shape[0])], [0] * rows.shape[0]
        ts.synchronize()
        cnt = aux.cpu().tolist()
        return [rows[i, :cnt[i][0]] for i in range(rows.shape[0])], [int(c[1]) for c in cnt]

    def codec_reset(self, slot: int):
        self._chk(self.lib.vv_codec_reset(self._ctx, self._s, slot), "vv_codec_reset")

    def connect(self, n: int, latent: torch.Tensor, sem: Optional[torch.Tensor], out: torch.Tensor):
        self._chk(self.lib.vv_connect(self._ctx, self._s, n, self._p(latent), self._p(sem), self._p(out)), "vv_connect")

    def profile_begin(self):
        self._chk(self.lib.vv_profile_begin(self._ctx), "vv_profile_begin")

    def profile_end(self):
        n, ms, by = (C.c_int64 * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
        self._chk(self.lib.vv_profile_end(self._ctx, n, ms, by), "vv_profile_end")
        return (n[0], ms[0], by[0]), (n[1], ms[1], by[1])

    def profile_replay(self, reps=3, family=0):
        """(launches, total_ms, bytes) of the recorded launches of one kernel family replayed as one dependent hipGraph chain:
        family 0 = vv_gemv_kernel, 1 = vv_gemv16p_kernel (batch decode), 2 = decode attention (fused kernel + merge)."""
        n, ms, by = C.c_int64(), C.c_double(), C.c_double()
        self._chk(self.lib.vv_profile_replay_family(self._ctx, self._s, int(family), int(reps), C.byref(n), C.byref(ms), C.byref(by)),
                  "vv_profile_replay_family")
        return n.value, ms.value, by.value

    def stat(self, what=0):
        return int(self.lib.vv_stat(self._ctx, what))

    # ------------------------------------------------------------------ low level (tests / microbench)
    def pack_matrix(self, w: torch.Tensor) -> torch.Tensor:
        N, K = w.shape
        out = torch.empty(int(self.lib.vv_packed_bytes(N, K)), dtype=torch.uint8, device=self.device)
        w = w.to(self.device, torch.float32).contiguous()
        with torch.cuda.stream(self.stream):
            rc = self.lib.vv_pack_matrix(self._s, self._p(w), self._p(out), N, K)
        if rc != 0:
            raise EngineError("vv_pack_matrix failed")
        self.sync()
        return out

    def w13_pack(self, packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
        """The W13 twin (vibevoice_amd/w13.py) of a pack_matrix output, packed and checked on the device: uint8 [vv_w13_twin_bytes]."""
        self._shape_ints("w13_pack", N=N, K=K)
        nbytes = int(self.lib.vv_w13_twin_bytes(N, K))
        if nbytes == 0:
            raise ValueError(f"w13_pack: N = {N} must be a multiple of 16 and K = {K} of 128")
        self._dev_tensor("w13_pack", "packed", packed, int(self.lib.vv_packed_bytes(N, K)), torch.uint8)
        twin = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._after_producer()
        rc = self.lib.vv_w13_pack_matrix(self._s, C.c_void_p(packed.data_ptr()), C.c_void_p(twin.data_ptr()), N, K)
        if rc != 0:
            raise EngineError(f"vv_w13_pack_matrix failed ({rc})")
        return twin

    def w13_unpack(self, twin: torch.Tensor, N: int, K: int) -> torch.Tensor:
        """A twin expanded back to packed bf16 fragments by the device decoder: uint8 [vv_packed_bytes]."""
        self._shape_ints("w13_unpack", N=N, K=K)
        nbytes = int(self.lib.vv_w13_twin_bytes(N, K))
        if nbytes == 0:
            raise ValueError(f"w13_unpack: N = {N} must be a multiple of 16 and K = {K} of 128")
        self._dev_tensor("w13_unpack", "twin", twin, nbytes, torch.uint8)
        out = torch.zeros(int(self.lib.vv_packed_bytes(N, K)), dtype=torch.uint8, device=self.device)
        self._after_producer()
        rc = self.lib.vv_w13_unpack_matrix(self._s, C.c_void_p(twin.data_ptr()), C.c_void_p(out.data_ptr()), N, K)
        if rc != 0:
            raise EngineError(f"vv_w13_unpack_matrix failed ({rc})")
        return out

    # ------------------------------------------------------------------ device-resident LoRA adapters
    MERGE_DTYPES = ("float32", "bfloat16")

    def _dev_tensor(self, what, name, t, numel, dtype=torch.float32, unaligned_ok=False):
        """an operand is checked BEFORE the call: a wrong argument must fail here, not as an out-of-bounds access on the GPU"""
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{what}: {name} is not a tensor on {self.device}")
        if t.dtype != dtype:
            raise ValueError(f"{what}: {name} is {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous")
        if t.data_ptr() % 16 and not unaligned_ok:
            raise ValueError(f"{what}: {name} is not 16-byte aligned")
        if t.numel() < numel:
            raise ValueError(f"{what}: {name} holds {t.numel()} elements, the launch addresses {numel}")

    @staticmethod
    def _shape_ints(what, **ints):
        for k, v in ints.items():
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1 or v >= (1 << 30):
                raise ValueError(f"{what}: {k} = {v!r} is not an int in [1, 2^30)")

    def _delta_flag(self, what, merge_dtype):
        if merge_dtype not in self.MERGE_DTYPES:
            raise ValueError(f"{what}: merge_dtype must be one of {self.MERGE_DTYPES}, got {merge_dtype!r}")
        return 1 if merge_dtype == "bfloat16" else 0

    def _raw_err(self):
        s = self.lib.vv_last_error(None)
        return s.decode() if s else "?"

    def _mat_shape(self, name):
        """(N, K) of a plain linear matrix parameter as the engine packs it, or None (unknown name, another kind: the library
        refuses those with its own text)"""
        tab = self.__dict__.setdefault("_mat_shapes", {})
        if name not in tab:
            n, k = C.c_int(), C.c_int()
            tab[name] = (n.value, k.value) if self.lib.vv_weight_shape(self._ctx, name.encode(), C.byref(n), C.byref(k)) == 0 else None
        return tab[name]

    def _after_producer(self):
        """operands made on the caller's current torch stream (fills, copies, .to(device)) are complete before the engine stream reads
        or overwrites them: an event wait on the device, no host synchronisation"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def unpack_matrix(self, packed: torch.Tensor, N: int, K: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The inverse of pack_matrix: packed bf16 tiles of a linear [N, K] matrix -> row-major fp32 (exact).  out: an [N, K] fp32
        tensor to write into (every element is written); default: a new one.  Asynchronous on the engine stream."""
        self._shape_ints("unpack_matrix", N=N, K=K)
        self._dev_tensor("unpack_matrix", "packed", packed, int(self.lib.vv_packed_bytes(N, K)), torch.uint8)
        if out is None:
            with torch.cuda.stream(self.stream):
                out = torch.empty(N, K, dtype=torch.float32, device=self.device)
        self._dev_tensor("unpack_matrix", "out", out, N * K)
        self._after_producer()
        if self.lib.vv_unpack_matrix(self._s, self._p(packed), self._p(out), int(N), int(K)) != 0:
            raise EngineError("vv_unpack_matrix failed: " + self._raw_err())
        return out

    def lora_merge_raw(self, base_packed: torch.Tensor, dst_packed: torch.Tensor, N: int, K: int, a: torch.Tensor, b: torch.Tensor,
                       scale: float, merge_dtype: str = "float32", unaligned_ok=()):
        """One launch of the LoRA merge kernel on raw buffers: dst_packed = bf16(base_packed + scale * b @ a) in the packed layout
        (a [r, K], b [N, r] fp32; dst_packed may be base_packed).  merge_dtype as lora.merge_lora.  Every tensor is checked before
        the call (unaligned_ok names operands whose alignment check is left to the library).  Asynchronous: the caller syncs."""
        what = "lora_merge_raw"
        self._shape_ints(what, N=N, K=K)
        flag = self._delta_flag(what, merge_dtype)
        if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dim() != 2 or b.dim() != 2:
            raise ValueError(f"{what}: a and b are 2-D tensors")
        r = int(a.shape[0])
        if tuple(a.shape) != (r, K) or tuple(b.shape) != (N, r):
            raise ValueError(f"{what}: a {tuple(a.shape)} / b {tuple(b.shape)} do not factor an [{N}, {K}] matrix")
        nb = int(self.lib.vv_packed_bytes(N, K))
        self._dev_tensor(what, "base_packed", base_packed, nb, torch.uint8, "base_packed" in unaligned_ok)
        self._dev_tensor(what, "dst_packed", dst_packed, nb, torch.uint8, "dst_packed" in unaligned_ok)
        self._dev_tensor(what, "a", a, r * K, unaligned_ok="a" in unaligned_ok)
        self._dev_tensor(what, "b", b, N * r, unaligned_ok="b" in unaligned_ok)
        self._after_producer()
        if self.lib.vv_lora_merge_raw(self._s, self._p(base_packed), self._p(dst_packed), int(N), int(K), self._p(a), self._p(b), r,
                                      float(scale), flag) != 0:
            raise EngineError("vv_lora_merge_raw failed: " + self._raw_err())

    def weight_read(self, name: str, shape: Sequence[int]) -> torch.Tensor:
        """A plain linear parameter as it is NOW (base, or base + the merged adapter): row-major fp32 `shape` = [N, K], exact (the
        storage is bf16).  The caller states the shape (the reference checkpoint's); it is checked against the engine's (vv_weight_shape)."""
        nk = self._mat_shape(name)
        if nk is not None and tuple(int(v) for v in shape) != nk:
            raise ValueError(f"weight_read({name}): shape {tuple(shape)}, the parameter is {nk}")
        with torch.cuda.stream(self.stream):
            out = torch.empty(*[int(v) for v in shape], dtype=torch.float32, device=self.device)
        self._chk(self.lib.vv_weight_read(self._ctx, self._s, name.encode(), self._p(out)), f"vv_weight_read({name})")
        return out

    def lora_merge(self, name: str, a: torch.Tensor, b: torch.Tensor, scale: float, merge_dtype: str = "float32", unaligned_ok=()):
        """active(name) = bf16(base + scale * b @ a), in place in the packed weights (a [r, K], b [N, r] fp32 on the engine device).
        The first merge of a parameter snapshots its base; a merge is never cumulative.  Eager on the engine stream; the caller
        syncs and keeps a and b alive until then.  Cached hipGraphs stay valid (no pointer changes)."""
        what = f"lora_merge({name})"
        flag = self._delta_flag(what, merge_dtype)
        if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"{what}: a [r, K] and b [N, r] are 2-D tensors with one r")
        r, K, N = int(a.shape[0]), int(a.shape[1]), int(b.shape[0])
        nk = self._mat_shape(name)
        if nk is not None and (N, K) != nk:          # the library takes N and K from its registry: a and b must cover them
            raise ValueError(f"{what}: b @ a is [{N}, {K}], the parameter is {list(nk)}")
        self._dev_tensor(what, "a", a, r * K, unaligned_ok="a" in unaligned_ok)
        self._dev_tensor(what, "b", b, N * r, unaligned_ok="b" in unaligned_ok)
        self._after_producer()
        self._chk(self.lib.vv_lora_merge(self._ctx, self._s, name.encode(), self._p(a), self._p(b), r, float(scale), flag),
                  f"vv_lora_merge({name})")
        if name.startswith("head."):
            self._n_steps = None             # as upload(): the timestep-embedding table is derived from head.t_embedder

    def lora_reset(self, name: Optional[str] = None):
        """The base snapshot copied back over the parameter (None: every merged parameter); a parameter never merged is left alone."""
        self._chk(self.lib.vv_lora_reset(self._ctx, self._s, name.encode() if name is not None else None), f"vv_lora_reset({name})")
        if name is None or name.startswith("head."):
            self._n_steps = None

    def gemm3_raw(self, wp, x, y, N, K, epi=0, w2p=None, nw=None, eps=1e-6, bias=None, ksplit=True):
        """the prefill GEMM (prefill.hip) on fp32 rows x [T, K] -> y [T, N]; ksplit=False computes every tile whole"""
        T = x.shape[0]
        xp = torch.zeros(int(self.lib.vv_packed_bytes(T, K)), dtype=torch.uint8, device=self.device)
        yp = torch.zeros(int(self.lib.vv_packed_bytes(T, N)), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        rc = self.lib.vv_gemm3_raw(self._ctx if ksplit else None, self._s, self._p(wp), self._p(w2p), self._p(x), T, N, K, epi, self._p(nw), float(eps),
                                   self._p(bias), self._p(y), self._p(xp), self._p(yp))
        if rc != 0:
            raise EngineError(f"vv_gemm3_raw failed ({rc})")
        self.sync()

    def gemm_raw(self, wp, x, y, N, K, T=None, ldx=None, ldy=None, pro=0, epi=0, w2p=None, nw=None, eps=1e-6,
                 bias=None, nscale=None, xsplit=None, ksplit=0, nontemporal=0):
        T = x.shape[0] if T is None else T
        rc = self.lib.vv_gemm_raw(self._s, self._p(wp), self._p(w2p), self._p(x), self._p(y), T, N, K,
                                  ldx or K, ldy or N, pro, epi, self._p(nw), float(eps), self._p(bias),
                                  self._p(nscale), xsplit or self.cfg.xsplit, ksplit, nontemporal)
        if rc != 0:
            raise EngineError(f"vv_gemm_raw failed ({rc})")

    # prologue / epilogue ids of csrc/vv_common.h
    PRO_NONE, PRO_RMS, PRO_RMS_MOD, PRO_ADD_SILU, PRO_NORMDW = 0, 1, 2, 3, 4
    EPI_STORE, EPI_BIAS, EPI_BIAS_GELU, EPI_SWIGLU, EPI_RESID, EPI_GATED_RESID, EPI_CFG_DPM = 0, 1, 2, 3, 4, 5, 6

    def gemv_case(self, wp, x, y, T, N, K, *, ldx=None, ldy=None, pro=0, epi=0, w2p=None, nw=None, eps=1e-6, bias=None, nscale=None,
                  mod_scale=None, mod_shift=None, ld_mod=0, addvec=None, x_row_mod=0, add_rows_per_vec=0, gate=None, ld_gate=0,
                  z=None, x0p=None, coef=None, cfg=0.0, n_cfg=0, sde_noise=None, cfg_rows=None,
                  kgrid=0, yparts=None, xa=None, n_xa=0, ya=None, n_ya=0, part_stride=0,
                  sl_n=0, sl_T=0, sl_x=0, sl_y=0, sl_id=(),
                  dw_hist=None, dw_w=None, dw_b=None, dw_gamma=None, dw_nw=None, dw_xout=None, dw_hnew=None,
                  xsplit=None, unaligned_ok=(), w13_form=None, twin=None, twin2=None):
        """One launch of the decode GEMV kernel (vv_gemv_case), or a refusal.  Returns the form the launcher chose,
        (XS, MR, WPB, PARTS, SL), or None when nothing was launched (the kernel's eligibility check or its launcher refused).

        Every tensor is checked BEFORE the call -- device, dtype (fp32; packed weights uint8), contiguity, 16-byte alignment and a
        size that covers every address the kernel can form from T, N, K and the strides -- and a mismatch raises ValueError: a
        wrong argument must fail here, not as an out-of-bounds access on the GPU.  unaligned_ok names tensors whose alignment
        check is waived, for callers that test the refusal of a misaligned operand (their size is still checked).
        Asynchronous: the caller syncs.

        w13_form = (mr, wpb): the launch is that W13 form (vv_w13_gemv_case), over the twins (w13_pack outputs; twin2 for SwiGLU's second
        matrix) or, with twin None, the same form over the bf16 fragments; returns the form asked for, None on a refusal."""
        ldx = K if ldx is None else ldx
        ldy = N if ldy is None else ldy
        xs = self.cfg.xsplit if xsplit is None else xsplit
        ints = dict(T=T, N=N, K=K, ldx=ldx, ldy=ldy, pro=pro, epi=epi, ld_mod=ld_mod, x_row_mod=x_row_mod, add_rows_per_vec=add_rows_per_vec,
                    ld_gate=ld_gate, n_cfg=n_cfg, kgrid=kgrid, n_xa=n_xa, n_ya=n_ya, part_stride=part_stride, sl_n=sl_n, sl_T=sl_T,
                    sl_x=sl_x, sl_y=sl_y, xsplit=xs)
        for k, v in ints.items():
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0 or v >= (1 << 30):
                raise ValueError(f"gemv_case: {k} = {v!r} is not an int in [0, 2^30)")
        if T < 1 or N < 1 or K < 1:
            raise ValueError(f"gemv_case: T, N, K = {T}, {N}, {K} must be positive")
        if xs not in (1, 2, 3):
            raise ValueError(f"gemv_case: xsplit = {xs}")
        if not 0 <= pro <= 4 or not 0 <= epi <= 6:
            raise ValueError(f"gemv_case: pro = {pro}, epi = {epi}")
        if ldx < K or ldy < N:
            raise ValueError(f"gemv_case: ldx = {ldx} < K = {K} or ldy = {ldy} < N = {N}")
        sl_id = [int(v) for v in sl_id]
        if sl_n > 8 or len(sl_id) < sl_n or len(sl_id) > 8 or any(v < 0 or v >= (1 << 20) for v in sl_id):
            raise ValueError(f"gemv_case: sl_n = {sl_n}, sl_id = {sl_id}")
        if sl_n > 0 and (sl_T < 1 or T != sl_n * sl_T):
            raise ValueError(f"gemv_case: T = {T} is not sl_n * sl_T = {sl_n} * {sl_T}")
        if sl_n == 0 and (sl_T or sl_x or sl_y or sl_id):
            raise ValueError("gemv_case: slot fields without sl_n")

        def need(name, t, numel, dtype=torch.float32, required=True):
            if t is None:
                if required:
                    raise ValueError(f"gemv_case: {name} is required here")
                return
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise ValueError(f"gemv_case: {name} is not a tensor on {self.device}")
            if t.dtype != dtype:
                raise ValueError(f"gemv_case: {name} is {t.dtype}, expected {dtype}")
            if not t.is_contiguous():
                raise ValueError(f"gemv_case: {name} is not contiguous")
            if t.data_ptr() % 16 and name not in unaligned_ok:
                raise ValueError(f"gemv_case: {name} is not 16-byte aligned")
            if t.numel() < numel:
                raise ValueError(f"gemv_case: {name} holds {t.numel()} elements, the launch addresses {numel}")

        def extent(rows, ld, width, slot_stride):
            """elements from the base pointer to the end of the last addressable row"""
            if sl_n > 0 and slot_stride > 0:
                return max(sl_id[:sl_n]) * slot_stride + (sl_T - 1) * ld + width
            return (rows - 1) * ld + width
        x_rows = x_row_mod if x_row_mod > 0 else T
        x_need = extent(x_rows, ldx, K, sl_x)
        y_need = extent(T, ldy, N, sl_y)
        wbytes = int(self.lib.vv_packed_bytes(N, K))
        need("wp", wp, wbytes, torch.uint8)
        need("w2p", w2p, wbytes, torch.uint8, required=epi == self.EPI_SWIGLU)
        if w13_form is None and (twin is not None or twin2 is not None):
            raise ValueError("gemv_case: twins without w13_form")
        if twin is not None or twin2 is not None:
            tbytes = int(self.lib.vv_w13_twin_bytes(N, K))
            if tbytes == 0:
                raise ValueError(f"gemv_case: no W13 twin for N = {N}, K = {K}")
            need("twin", twin, tbytes, torch.uint8)
            need("twin2", twin2, tbytes, torch.uint8, required=epi == self.EPI_SWIGLU)
        need("x", x, x_need)
        need("y", y, y_need, required=epi != self.EPI_CFG_DPM)
        need("nw", nw, K, required=False)
        need("bias", bias, N, required=False)
        need("nscale", nscale, N, required=False)
        is_mod = pro == self.PRO_RMS_MOD
        if is_mod and ld_mod < K:
            raise ValueError(f"gemv_case: ld_mod = {ld_mod} < K = {K}")
        need("mod_scale", mod_scale, (T - 1) * ld_mod + K, required=is_mod)
        need("mod_shift", mod_shift, (T - 1) * ld_mod + K, required=is_mod)
        n_vec = (T - 1) // add_rows_per_vec + 1 if add_rows_per_vec > 0 else 1
        need("addvec", addvec, n_vec * K, required=pro == self.PRO_ADD_SILU)
        is_gated = epi == self.EPI_GATED_RESID
        if is_gated and ld_gate < N:
            raise ValueError(f"gemv_case: ld_gate = {ld_gate} < N = {N}")
        need("gate", gate, (T - 1) * ld_gate + N, required=is_gated)
        is_cfg = epi == self.EPI_CFG_DPM
        if is_cfg and n_cfg < 1:
            raise ValueError("gemv_case: the CFG epilogue needs n_cfg >= 1")
        need("z", z, 2 * n_cfg * N, required=is_cfg)       # dense [2 n_cfg][N]: the epilogue addresses them by n_cfg, not by T or ldy
        need("x0p", x0p, n_cfg * N, required=is_cfg)
        need("coef", coef, 6, required=is_cfg)
        need("sde_noise", sde_noise, n_cfg * N, required=False)
        need("cfg_rows", cfg_rows, n_cfg, required=False)
        if (kgrid > 1 or n_xa or n_ya) and part_stride < max(x_need if n_xa else 0, y_need if (kgrid > 1 or n_ya) else 0):
            raise ValueError(f"gemv_case: part_stride = {part_stride} is smaller than one part tensor")
        need("yparts", yparts, (kgrid - 2) * part_stride + y_need if kgrid > 1 else 0, required=kgrid > 1)
        need("xa", xa, (max(n_xa, 2) - 1) * part_stride + x_need, required=n_xa > 0)
        need("ya", ya, (max(n_ya, 2) - 1) * part_stride + y_need, required=n_ya > 0)
        is_dw = pro == self.PRO_NORMDW
        for name, t, rows in (("dw_hist", dw_hist, 6), ("dw_w", dw_w, 7), ("dw_b", dw_b, 1), ("dw_gamma", dw_gamma, 1), ("dw_nw", dw_nw, 1),
                              ("dw_xout", dw_xout, 1), ("dw_hnew", dw_hnew, 1)):
            need(name, t, rows * K, required=is_dw)

        a = _lib.VVGemvCase()
        p = lambda t: t.data_ptr() if t is not None else None
        a.W, a.W2, a.X, a.Y = p(wp), p(w2p), p(x), p(y)
        a.T, a.N, a.K, a.ldx, a.ldy, a.pro, a.epi = T, N, K, ldx, ldy, pro, epi
        a.nw, a.eps, a.bias, a.nscale = p(nw), float(eps), p(bias), p(nscale)
        a.mod_scale, a.mod_shift, a.ld_mod = p(mod_scale), p(mod_shift), ld_mod
        a.addvec, a.x_row_mod, a.add_rows_per_vec = p(addvec), x_row_mod, add_rows_per_vec
        a.gate, a.ld_gate = p(gate), ld_gate
        a.z, a.x0p, a.coef, a.cfg, a.n_cfg, a.sde_noise = p(z), p(x0p), p(coef), float(cfg), n_cfg, p(sde_noise)
        a.kgrid, a.yparts, a.xa, a.n_xa, a.ya, a.n_ya, a.part_stride = kgrid, p(yparts), p(xa), n_xa, p(ya), n_ya, part_stride
        a.sl_n, a.sl_T, a.sl_x, a.sl_y = sl_n, sl_T, sl_x, sl_y
        for j, v in enumerate(sl_id):
            a.sl_id[j] = v
        a.dw_hist, a.dw_w, a.dw_b, a.dw_gamma, a.dw_nw = p(dw_hist), p(dw_w), p(dw_b), p(dw_gamma), p(dw_nw)
        a.dw_xout, a.dw_hnew = p(dw_xout), p(dw_hnew)
        a.cfg_rows = p(cfg_rows)
        if w13_form is not None:
            mr, wpb = (int(v) for v in w13_form)
            if xs != 1 or T > mr:
                raise ValueError(f"gemv_case: the W13 form ({mr}, {wpb}) takes xsplit 1 and T <= {mr}")
            rc = self.lib.vv_w13_gemv_case(self._s, C.byref(a), p(twin), p(twin2), mr, wpb)
            if rc == _lib.GEMV_REFUSED:
                return None
            if rc != 0:
                raise EngineError(f"vv_w13_gemv_case failed ({rc})")
            return (1, mr, wpb, 0, 0)
        form = (C.c_int * 5)()
        rc = self.lib.vv_gemv_case(self._s, C.byref(a), xs, form)
        if rc == _lib.GEMV_REFUSED:
            return None
        if rc != 0:
            raise EngineError(f"vv_gemv_case failed ({rc})")
        return tuple(form)

    def _case_need(self, who, name, t, numel, dtype=torch.float32, required=False):
        """the operand check of the one-launch test entries: device, dtype, contiguity, 16-byte alignment, at least numel elements"""
        if t is None:
            if required:
                raise ValueError(f"{who}: {name} is required here")
            return
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{who}: {name} is not a tensor on {self.device}")
        if t.dtype != dtype:
            raise ValueError(f"{who}: {name} is {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} is not contiguous")
        if t.data_ptr() % 16:
            raise ValueError(f"{who}: {name} is not 16-byte aligned")
        if t.numel() < numel:
            raise ValueError(f"{who}: {name} holds {t.numel()} elements, the launch addresses {numel}")

    @staticmethod
    def _case_ints(who, **ints):
        for k, v in ints.items():
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0 or v >= (1 << 30):
                raise ValueError(f"{who}: {k} = {v!r} is not an int in [0, 2^30)")

    FLAG_RS, FLAG_SH, FLAG_PK = 1, 2, 4      # vv_gemv16p_case's flags

    def gemv16p_case(self, wp, xp, T, N, K, *, epi=0, flags=0, w2p=None, y=None, yp=None, bias=None, gate=None, ldy=None, ld_gate=0,
                     ssq_in=None, ssq_tiles=0, eps=1e-6, xs=None, pk_nw=None, pk_sc=None, ld_pk=0, ssq_out=None,
                     z=None, x0p=None, coef=None, cfg=0.0, n_cfg=0, sde_noise=None, cfg_rows=None):
        """One launch of the batch-decode packed GEMV (vv_gemv16p_case), or a refusal.  Returns the waves per workgroup the launcher
        chose (4 or 8), or None when nothing was launched.  xp / xs: one packed 16-row activation tile each (uint8, ceil(K / 32) KiB);
        yp: one such tile of the N output features; fp32 everywhere else.

        As in gemv_case every tensor is checked BEFORE the call -- device, dtype, contiguity, 16-byte alignment and a size that covers
        every address the kernel can form -- and a mismatch raises ValueError.  An operand the launcher itself insists on (ssq_in
        with RS, xs with SH, ...) may be None: that is its refusal to give.  Asynchronous: the caller syncs."""
        who = "gemv16p_case"
        ldy = N if ldy is None else ldy
        self._case_ints(who, T=T, N=N, K=K, epi=epi, flags=flags, ldy=ldy, ld_gate=ld_gate, ssq_tiles=ssq_tiles, ld_pk=ld_pk, n_cfg=n_cfg)
        if N < 1 or K < 1 or T > 64:
            raise ValueError(f"{who}: T, N, K = {T}, {N}, {K}")
        if not 0 <= epi <= 6 or not 0 <= flags <= 7:
            raise ValueError(f"{who}: epi = {epi}, flags = {flags}")
        need = lambda *a, **k: self._case_need(who, *a, **k)
        k_tiles, n4 = (K + 31) // 32, 4 * ((N + 3) // 4)
        rows = lambda ld: max(T - 1, 0) * ld + n4             # the last row's last float4
        wbytes = int(self.lib.vv_packed_bytes(N, K))
        need("wp", wp, wbytes, torch.uint8, required=True)
        need("w2p", w2p, wbytes, torch.uint8, required=epi == self.EPI_SWIGLU)
        need("xp", xp, k_tiles * 1024, torch.uint8, required=True)
        need("xs", xs, k_tiles * 1024, torch.uint8)
        if y is not None and ldy < n4:
            raise ValueError(f"{who}: ldy = {ldy} < N = {N}")
        need("y", y, rows(ldy))
        need("yp", yp, ((N + 31) // 32) * 1024, torch.uint8)
        need("bias", bias, n4)
        if gate is not None and ld_gate < n4:
            raise ValueError(f"{who}: ld_gate = {ld_gate} < N = {N}")
        need("gate", gate, rows(ld_gate))
        if ssq_in is not None and ssq_tiles < 1:
            raise ValueError(f"{who}: ssq_in with ssq_tiles = {ssq_tiles}")
        need("ssq_in", ssq_in, ssq_tiles * 16)
        need("pk_nw", pk_nw, n4)
        if pk_sc is not None and ld_pk < n4:
            raise ValueError(f"{who}: ld_pk = {ld_pk} < N = {N}")
        need("pk_sc", pk_sc, rows(ld_pk))
        need("ssq_out", ssq_out, ((N + 15) // 16) * 16)
        need("z", z, 2 * n_cfg * N)                          # dense [2 n_cfg][N]: addressed by n_cfg, not by T or ldy
        need("x0p", x0p, n_cfg * N)
        need("coef", coef, 6)
        need("sde_noise", sde_noise, n_cfg * N)
        need("cfg_rows", cfg_rows, n_cfg)

        a = _lib.VVGemv16pCase()
        p = lambda t: t.data_ptr() if t is not None else None
        a.W, a.W2, a.Xp, a.Y, a.Yp, a.bias, a.gate = p(wp), p(w2p), p(xp), p(y), p(yp), p(bias), p(gate)
        a.T, a.N, a.K, a.ldy, a.ld_gate = T, N, K, ldy, ld_gate
        a.ssq_in, a.ssq_tiles, a.eps, a.Xs = p(ssq_in), ssq_tiles, float(eps), p(xs)
        a.pk_nw, a.pk_sc, a.ld_pk, a.ssq_out = p(pk_nw), p(pk_sc), ld_pk, p(ssq_out)
        a.z, a.x0p, a.coef, a.cfg, a.n_cfg, a.sde_noise, a.cfg_rows = p(z), p(x0p), p(coef), float(cfg), n_cfg, p(sde_noise), p(cfg_rows)
        wpb = C.c_int(0)
        rc = self.lib.vv_gemv16p_case(self._s, C.byref(a), epi, flags, C.byref(wpb))
        if rc == _lib.GEMV_REFUSED:
            return None
        if rc != 0:
            raise EngineError(f"vv_gemv16p_case failed ({rc})")
        return wpb.value

    def pack16_case(self, x, xp, T, K, *, mode=1, ldx=None, nw=None, eps=1e-6, sc=None, sh=None, ld_mod=0, unaligned_ld_ok=False):
        """One launch of vv_pack16_kernel (vv_pack16_case): rows x [T][ldx] fp32 -> the packed 16-row tile xp (uint8, K / 32 KiB), or a
        refusal (None).  Returns 4, the kernel's waves per workgroup.  Operands are checked as in gemv16p_case; unaligned_ld_ok waives
        the multiple-of-4 check of ldx for a caller that tests the launcher's refusal of it (sizes are still checked)."""
        who = "pack16_case"
        ldx = K if ldx is None else ldx
        self._case_ints(who, T=T, K=K, mode=mode, ldx=ldx, ld_mod=ld_mod)
        if K < 32 or T > 64:
            raise ValueError(f"{who}: T, K = {T}, {K}")
        if ldx < K or (ldx % 4 and not unaligned_ld_ok):
            raise ValueError(f"{who}: ldx = {ldx}")
        need = lambda *a, **k: self._case_need(who, *a, **k)
        need("x", x, max(T - 1, 0) * ldx + K, required=True)
        need("xp", xp, ((K + 31) // 32) * 1024, torch.uint8, required=True)
        need("nw", nw, K)
        if (sc is not None or sh is not None) and (ld_mod < K or ld_mod % 4):
            raise ValueError(f"{who}: ld_mod = {ld_mod}")
        need("sc", sc, max(T - 1, 0) * ld_mod + K)
        need("sh", sh, max(T - 1, 0) * ld_mod + K)
        p = lambda t: t.data_ptr() if t is not None else None
        rc = self.lib.vv_pack16_case(self._s, p(x), ldx, mode, p(nw), float(eps), p(sc), p(sh), ld_mod, p(xp), T, K)
        if rc == _lib.GEMV_REFUSED:
            return None
        if rc != 0:
            raise EngineError(f"vv_pack16_case failed ({rc})")
        return 4

    def pack16_tiles_case(self, x, xp, T, K, n_tiles, *, ldx=None, stride_outer=0, n_inner=1, stride_inner=0, tile_bytes=None):
        """One launch of vv_pack16_tiles_kernel (vv_pack16_tiles_case): n_tiles row blocks [T][ldx] of x, block j at float offset
        (j // n_inner) * stride_outer + (j % n_inner) * stride_inner, -> plain bf16 packed tiles at xp + j * tile_bytes; None on a
        refusal, else 4 (waves per workgroup).  Operands are checked as in gemv16p_case."""
        who = "pack16_tiles_case"
        ldx = K if ldx is None else ldx
        tb = ((K + 31) // 32) * 1024
        tile_bytes = tb if tile_bytes is None else tile_bytes
        self._case_ints(who, T=T, K=K, n_tiles=n_tiles, ldx=ldx, stride_outer=stride_outer, n_inner=n_inner, stride_inner=stride_inner,
                        tile_bytes=tile_bytes)
        if K < 32 or T > 64 or n_tiles < 1 or n_inner < 1 or ldx < K or tile_bytes < tb:
            raise ValueError(f"{who}: T, K, n_tiles, n_inner, ldx, tile_bytes = {T}, {K}, {n_tiles}, {n_inner}, {ldx}, {tile_bytes}")
        last = max(((j // n_inner) * stride_outer + (j % n_inner) * stride_inner) for j in range(n_tiles))
        need = lambda *a, **k: self._case_need(who, *a, **k)
        need("x", x, last + max(T - 1, 0) * ldx + K, required=True)
        need("xp", xp, (n_tiles - 1) * tile_bytes + tb, torch.uint8, required=True)
        rc = self.lib.vv_pack16_tiles_case(self._s, x.data_ptr(), ldx, stride_outer, n_inner, stride_inner, xp.data_ptr(), tile_bytes, T, K, n_tiles)
        if rc == _lib.GEMV_REFUSED:
            return None
        if rc != 0:
            raise EngineError(f"vv_pack16_tiles_case failed ({rc})")
        return 4


class TempoCapacityError(EngineError):
    """A Tempo.push row that brings more input, or emits more output, than one launch takes per row; nothing ran, no state changed:
    push it in pieces."""


class _RowStage:
    """What the streaming row stages share (Loudness, Tempo, Formant, Pitch, Resampler, Level, Pause): n_streams chunk-continuous streams
    in one of the engine's configurations, pushed up to 16 rows a launch.  A stage supplies KIND (Engine._STAGE_USED), its row struct ROW
    and how push() fills it, its C entry points ROWS_FN / RESET_FN, counts(), max_out() and take().  Pause alone has no counts(): what
    it emits depends on the data, its push() launches itself and returns the counts as a device tensor."""
    KIND = ROW = ROWS_FN = RESET_FN = None
    NO_ROWS = ()                                          # the launches of a push that names no stream

    def __init__(self, engine: Engine, slot: int, n_streams: int):
        self.engine, self.slot, self.n_streams = engine, slot, int(n_streams)
        self.total = [0] * self.n_streams                 # input samples each stream has taken (the C side keeps the same figures)

    def take(self, ids: Sequence[int], remaining: Sequence[int], flush: bool = False) -> int:
        """input samples per row the next push accepts from rows that still have remaining[i] for stream ids[i]: a longer chunk goes in
        pieces of this width (host integers)"""
        raise NotImplementedError

    def _args(self, audio, stream_ids, flush, n_in, **more):
        """push()'s arguments checked and spread over the rows -> (ids, samples, n_in per row, flush per row, *more per row)"""
        e, name = self.engine, type(self).__name__
        ids = [int(i) for i in stream_ids]
        n = len(ids)
        samples = 0 if audio is None else int(audio.shape[-1])
        if audio is not None:
            if audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_contiguous() or audio.device != e.device or audio.shape[0] < n:
                raise ValueError(f"{name}.push: audio is a contiguous fp32 [n >= {n}, samples] tensor on {e.device}")
        nin = [samples] * n if n_in is None else [int(v) for v in n_in]
        fl = [bool(flush)] * n if isinstance(flush, (bool, int)) else [bool(v) for v in flush]
        rest = [[v] * n if not hasattr(v, "__len__") else list(v) for v in more.values()]
        if any(len(v) != n for v in [nin, fl] + rest):
            names = ["n_in", "flush"] + list(more)
            raise ValueError(f"{name}.push: {', '.join(names[:-1])} and {names[-1]} name one value per row")
        return (ids, samples, nin, fl, *rest)

    def _out(self, out, n, nin, pcm16):
        """push()'s output rows: the caller's, checked, or new ones of max_out() columns"""
        e, dt = self.engine, torch.int16 if pcm16 else torch.float32
        if out is None:
            return torch.empty((max(n, 1), self.max_out(max(nin, default=0))), dtype=dt, device=e.device)
        if out.dim() != 2 or out.dtype != dt or not out.is_contiguous() or out.device != e.device or out.shape[0] < n:
            raise ValueError(f"{type(self).__name__}.push: out is a contiguous {dt} [n >= {n}, capacity] tensor on {e.device}")
        return out

    def _refused(self, rc):
        self.engine._chk(rc, self.ROWS_FN)

    def _launch(self, audio, samples, ids, nin, rows, out, pcm16, stream, extra=lambda i0: (), took=lambda i: None):
        """One ROWS_FN launch per 16 rows on `stream` (default: the device's current torch stream), the pointers offset to the launch's
        first row; extra(i0): the stage's further arguments; took(i) after the launch that took row i -> the rows' counts"""
        e, n, cap = self.engine, len(ids), int(out.shape[1])
        st = e._sp(stream if stream is not None else torch.cuda.current_stream(e.device))
        cnts = (C.c_int * max(n, 1))()
        for i0 in range(0, n, 16) or self.NO_ROWS:
            nn = min(16, n - i0)
            a = C.c_void_p(audio.data_ptr() + i0 * samples * 4) if audio is not None else C.c_void_p()
            o = C.c_void_p(out.data_ptr() + i0 * cap * out.element_size())
            self._refused(getattr(e.lib, self.ROWS_FN)(e._ctx, st, self.slot, nn, C.cast(C.byref(rows, i0 * C.sizeof(self.ROW)), C.POINTER(self.ROW)),
                                                       a, samples, o, cap, int(pcm16), C.cast(C.byref(cnts, i0 * 4), C.POINTER(C.c_int)), *extra(i0)))
            for i in range(i0, i0 + nn):
                self.total[ids[i]] += nin[i]
                took(i)
        return [int(cnts[i]) for i in range(n)]

    def reset(self, ids: Optional[Sequence[int]] = None, stream=None):
        """streams `ids` (default: all) back to their first sample: history zeroed on `stream`, totals 0, flush marks cleared"""
        e = self.engine
        st = e._sp(stream if stream is not None else torch.cuda.current_stream(e.device))
        arr = None if ids is None else (C.c_int * max(1, len(ids)))(*[int(i) for i in ids])
        e._chk(getattr(e.lib, self.RESET_FN)(e._ctx, st, self.slot, 0 if ids is None else len(ids), arr), self.RESET_FN)
        for i in range(self.n_streams) if ids is None else ids:
            self._cleared(int(i))

    def _cleared(self, stream_id):
        self.total[stream_id] = 0

    def close(self):
        """give the engine's configuration back (its device buffers are released when the configuration is set again or the engine closes)"""
        used = getattr(self.engine, Engine._STAGE_USED[self.KIND], None)
        if used is not None and used[self.slot] is self:
            used[self.slot] = None


class Tempo(_RowStage):
    """One streaming tempo configuration of an engine (Engine.tempo): n_streams chunk-continuous streams at 24 kHz, each at the speed
    of its first push until its reset (which clears the speed with the rest).  What a stream delivers does not depend on how its input
    was cut into pushes (vibevoice_amd/tempo.py): the concatenation of its pushes and its flush equals Engine.time_stretch() of the
    concatenated input, bit for bit in float mode, ceil(n * Q / P) samples.  delay_samples: the input samples (640, 26.7 ms) a stream
    holds back at most until its next push; max_in: the input samples one row of a push may bring."""
    KIND, ROW, ROWS_FN, RESET_FN = "tempo", _lib.VVTempoRow, "vv_tempo_rows", "vv_tempo_reset"

    def __init__(self, engine: Engine, slot: int, n_streams: int):
        from . import tempo as _tp
        super().__init__(engine, slot, n_streams)
        self.delay_samples, self.max_in = _tp.delay_samples(), 7680
        self.ratio = [None] * self.n_streams              # (P, Q) of each stream, None before its first push
        w = np.ascontiguousarray(_tp.window())
        engine._chk(engine.lib.vv_tempo_set(engine._ctx, slot, C.c_void_p(w.ctypes.data), self.n_streams, engine._s), "vv_tempo_set")

    def counts(self, stream_id: int, n_in: int, speed=None, flush: bool = False) -> int:
        """samples a push of n_in samples to stream_id would emit now (host integers, no device sync); speed: for its first push"""
        from . import tempo as _tp
        P, Q = self.ratio[stream_id] or _tp.ratio(speed)
        return _tp.counts(P, Q, self.total[stream_id], n_in, flush)[1]

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits at any speed, the flush included: a stream has emitted every
        block that starts 880 input samples or more before its total, and a signal of n samples yields at most 2 n"""
        return 2 * (int(n_in) + 880) + 1

    def take(self, ids, remaining, flush=False):
        return min(self.max_in, max(remaining))

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], speeds, flush=False, out: Optional[torch.Tensor] = None,
             n_in=None, stream=None, pcm16: bool = False, return_offsets: bool = False):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) at speeds[i] (or one speed for all rows; a stream keeps the speed of its first push); n_in: samples
        of each row that count (default: all), flush: bool or one per row -- a stream's last push, after which it takes no more until
        reset().  -> (out, counts): out[i, :counts[i]] is what row i emitted, fp32, or int16 under pcm16 (the arithmetic of
        Engine.audio_to_pcm16 over the row's stretched chunk, in the same launch).  out: a contiguous [>= n, capacity] tensor of that
        dtype to write into (default: a new one of max_out(samples) columns).  return_offsets: -> (out, counts, offsets), offsets
        int32 [n, blocks]: the offset chosen for each block of 240 samples a row emitted.  One launch per 16 rows on `stream`
        (default: the device's current torch stream); the counts are host integers, nothing waits for the device.  A row beyond the
        launch's capacity raises TempoCapacityError before anything ran."""
        from . import tempo as _tp
        ids, samples, nin, fl, sp = self._args(audio, stream_ids, flush, n_in, speeds=speeds)
        pq = [_tp.ratio(v) for v in sp]
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        ld_off = -(-int(out.shape[1]) // _tp.HS)
        offs = torch.zeros((max(n, 1), ld_off), dtype=torch.int32, device=out.device) if return_offsets else None
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush, rows[i].P, rows[i].Q = ids[i], nin[i], int(fl[i]), pq[i][0], pq[i][1]
        res = self._launch(audio, samples, ids, nin, rows, out, pcm16, stream,
                           extra=lambda i0: (C.c_void_p(offs.data_ptr() + i0 * ld_off * 4) if offs is not None else C.c_void_p(), ld_off),
                           took=lambda i: self.ratio.__setitem__(ids[i], pq[i]))
        return (out, res, offs) if return_offsets else (out, res)

    def _refused(self, rc):
        if rc == _lib.TEMPO_OVER_CAPACITY:
            raise TempoCapacityError(f"Tempo.push: {self.engine._err()}")
        super()._refused(rc)

    def _cleared(self, stream_id):
        self.total[stream_id], self.ratio[stream_id] = 0, None


class Pitch(_RowStage):
    """One streaming pitch configuration of an engine (Engine.pitch): n_streams chunk-continuous variable-ratio resamplers at 24 kHz, each
    at the ratio P / Q of the shift of its first push until its reset (which clears the ratio with the rest); the rows of one launch run
    at different ratios.  What a stream delivers does not depend on how its input was cut into pushes (vibevoice_amd/pitch.py): the
    concatenation of its pushes and its flush equals Engine.pitch_resample() of the concatenated input, bit for bit in float mode,
    ceil(n * Q / P) samples; a stream at 0 semitones passes bit for bit.  Pitch AND duration change by the ratio: behind a tempo stage at
    speed Q / P (AudioStreamer(pitch=...)) the duration stays.  delay_samples: the input samples (64, 2.7 ms) a stream holds back at
    most until its next push; max_in: the input samples one row of a push may bring."""
    KIND, ROW, ROWS_FN, RESET_FN = "pitch", _lib.VVPitchRow, "vv_pitch_rows", "vv_pitch_reset"
    NO_ROWS = (0,)                                        # one launch, which vv_pitch_rows refuses by name

    def __init__(self, engine: Engine, slot: int, n_streams: int):
        from . import pitch as _pt
        super().__init__(engine, slot, n_streams)
        self.delay_samples, self.max_in = _pt.MAX_TN, _pt.MAX_IN
        self.ratio = [None] * self.n_streams              # (P, Q) of each stream, None before its first push
        h = np.ascontiguousarray(_pt.table())
        engine._chk(engine.lib.vv_pitch_set(engine._ctx, slot, C.c_void_p(h.ctypes.data), int(h.shape[0]), _pt.R, self.n_streams, engine._s),
                    "vv_pitch_set")

    def _pq(self, stream_id, semitones):
        from . import pitch as _pt
        return self.ratio[stream_id] or _pt.ratio(semitones)

    def counts(self, stream_id: int, n_in: int, semitones=None, flush: bool = False) -> int:
        """samples a push of n_in samples to stream_id would emit now (host integers, no device sync); semitones: for its first push"""
        from . import pitch as _pt
        P, Q = self._pq(stream_id, semitones)
        return _pt.counts(P, Q, self.total[stream_id], n_in, flush)[1]

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits at any ratio, the flush included: at most 64 held samples join the
        chunk, and n samples yield at most 2 n"""
        return 2 * (int(n_in) + self.delay_samples) + 1

    def take(self, ids, remaining, flush=False, semitones=None):
        """semitones: one per row, for the streams that have had no push yet (without it such a stream counts as an octave down, the
        ratio that emits most)"""
        from . import pitch as _pt
        semis = [-12.0] * len(ids) if semitones is None else semitones
        return _pt.push_width([self._pq(i, s) for i, s in zip(ids, semis)], [self.total[i] for i in ids], remaining, flush)

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], semitones, flush=False, out: Optional[torch.Tensor] = None,
             n_in=None, stream=None, pcm16: bool = False):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) at the ratio of semitones[i] (or one shift for all rows; a stream keeps the ratio of its first push);
        n_in: samples of each row that count (default: all), flush: bool or one per row -- a stream's last push, after which it takes no
        more until reset().  -> (out, counts): out[i, :counts[i]] is what row i emitted, fp32, or int16 under pcm16 (the arithmetic of
        Engine.audio_to_pcm16 over the row's resampled chunk, in the same launch).  out: a contiguous [>= n, capacity] tensor of that
        dtype to write into (default: a new one of max_out(samples) columns).  One launch per 16 rows on `stream` (default: the
        device's current torch stream); the counts are host integers, nothing waits for the device.  A row of more than max_in
        samples, or one that emits more than 8192, is refused: push it in pieces of take()."""
        from . import pitch as _pt
        ids, samples, nin, fl, semis = self._args(audio, stream_ids, flush, n_in, semitones=semitones)
        pq = [_pt.ratio(v) for v in semis]
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush, rows[i].P, rows[i].Q = ids[i], nin[i], int(fl[i]), pq[i][0], pq[i][1]
        return out, self._launch(audio, samples, ids, nin, rows, out, pcm16, stream, took=lambda i: self.ratio.__setitem__(ids[i], pq[i]))

    def _cleared(self, stream_id):
        self.total[stream_id], self.ratio[stream_id] = 0, None


def _fm_fractions(_fm, who, n, semitones, fractions):
    """the warps (A, B) of n rows from semitones (one value or one per row) or from fractions ((A, B) or one pair per row)"""
    if fractions is not None:
        ab = [tuple(fractions)] * n if not hasattr(fractions[0], "__len__") else [tuple(v) for v in fractions]
        name = "fractions"
    else:
        ab = [semitones] * n if not hasattr(semitones, "__len__") else list(semitones)
        name = "semitones"
    if len(ab) != n:
        raise ValueError(f"{who}: {name} names one value, or one per row ({n}), got {len(ab)}")
    return [_fm.check(*v) for v in ab] if fractions is not None else [_fm.warp_of(v) for v in ab]


class Formant(_RowStage):
    """One streaming formant configuration of an engine (Engine.formant): n_streams chunk-continuous spectral-envelope warps at 24 kHz,
    each at the fraction A / B of its first push until its reset (which clears the fraction with the rest); the rows of one launch run at
    different fractions.  What a stream delivers does not depend on how its input was cut into pushes (vibevoice_amd/formant.py): the
    concatenation of its pushes and its flush equals Engine.formant_warp() of the concatenated input, bit for bit, as many samples; a
    stream at 1 / 1 passes bit for bit.  The pushes of one configuration are ordered on one stream.  delay_samples: the input samples
    (1023, 42.6 ms) a stream holds back at most until its next push; max_in: the input samples one row of a push may bring."""
    KIND, ROW, ROWS_FN, RESET_FN = "formant", _lib.VVFormantRow, "vv_formant_rows", "vv_formant_reset"
    NO_ROWS = (0,)                                        # one launch, which vv_formant_rows refuses by name

    def __init__(self, engine: Engine, slot: int, n_streams: int):
        from . import formant as _fm
        super().__init__(engine, slot, n_streams)
        self.delay_samples, self.max_in = _fm.DELAY, _fm.MAX_IN
        self.ratio = [None] * self.n_streams              # (A, B) of each stream, None before its first push
        t = np.ascontiguousarray(_fm.twiddles())
        engine._chk(engine.lib.vv_formant_set(engine._ctx, slot, C.c_void_p(t.ctypes.data), self.n_streams, engine._s), "vv_formant_set")

    def counts(self, stream_id: int, n_in: int, semitones=None, flush: bool = False, fraction=None) -> int:
        """samples a push of n_in samples to stream_id would emit now (host integers, no device sync); semitones or fraction = (A, B):
        for its first push"""
        from . import formant as _fm
        A, B = self.ratio[stream_id] or (_fm.check(*fraction) if fraction is not None else _fm.warp_of(semitones))
        return _fm.counts(self.total[stream_id], n_in, flush, A, B)[1]

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits, the flush included: at most 1023 held samples join the chunk"""
        return int(n_in) + self.delay_samples

    def take(self, ids, remaining, flush=False):
        from . import formant as _fm
        return _fm.push_width(remaining)

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], semitones=None, flush=False, out: Optional[torch.Tensor] = None,
             n_in=None, stream=None, pcm16: bool = False, fractions=None):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) at the warp of semitones[i] (or one shift for all rows), or at fractions[i] = (A, B) (or one pair for all
        rows) in their place; a stream keeps the fraction of its first push.  n_in: samples of each row that count (default: all),
        flush: bool or one per row -- a stream's last push, after which it takes no more until reset().  -> (out, counts):
        out[i, :counts[i]] is what row i emitted, fp32 (pcm16 is refused by name: a level stage follows this one).  out: a contiguous
        fp32 [>= n, capacity] tensor to write into (default: a new one of max_out(samples) columns).  Two launches per 16 rows on `stream`
        (default: the device's current torch stream); the counts are host integers, nothing waits for the device.  A row of more than
        max_in samples is refused: push it in pieces of take()."""
        from . import formant as _fm
        ids, samples, nin, fl = self._args(audio, stream_ids, flush, n_in)
        ab = _fm_fractions(_fm, "Formant.push", len(ids), semitones, fractions)
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush, rows[i].A, rows[i].B = ids[i], nin[i], int(fl[i]), ab[i][0], ab[i][1]
        return out, self._launch(audio, samples, ids, nin, rows, out, pcm16, stream, took=lambda i: self.ratio.__setitem__(ids[i], ab[i]))

    def _cleared(self, stream_id):
        self.total[stream_id], self.ratio[stream_id] = 0, None


class Resampler(_RowStage):
    """One streaming resampler configuration of an engine (Engine.resampler): n_streams chunk-continuous streams src_rate -> dst_rate.
    What a stream delivers does not depend on how its input was cut into pushes (vibevoice_amd/resample.py): the concatenation of its
    pushes and its flush equals Engine.resample() of the concatenated input, bit for bit in float mode, ceil(n * L / M) samples.
    taps: filter taps per output sample; delay_samples: the input samples (taps / 2) a stream holds back until its next push."""
    KIND, ROW, ROWS_FN, RESET_FN = "resampler", _lib.VVResampleRow, "vv_resample_rows", "vv_resampler_reset"
    NO_ROWS = (0,)                                        # one launch, which vv_resample_rows refuses by name (Tempo.push returns no counts)

    def __init__(self, engine: Engine, slot: int, src_rate: int, dst_rate: int, n_streams: int):
        from . import resample as _rs
        super().__init__(engine, slot, n_streams)
        self.src_rate, self.dst_rate = int(src_rate), int(dst_rate)
        self.L, self.M, self.T, coef = _rs.design(src_rate, dst_rate)
        self.taps, self.delay_samples = self.T, _rs.delay_samples(self.T)
        c = np.ascontiguousarray(coef)
        engine._chk(engine.lib.vv_resampler_set(engine._ctx, slot, self.L, self.M, self.T, C.c_void_p(c.ctypes.data), self.n_streams,
                                                engine._s), "vv_resampler_set")

    def counts(self, stream_id: int, n_in: int, flush: bool = False) -> int:
        """samples a push of n_in samples to stream_id would emit now (host integers, no device sync)"""
        from . import resample as _rs
        return _rs.counts(self.L, self.M, self.T, self.total[stream_id], n_in, flush)[1]

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits, the flush included"""
        return -((-(int(n_in) + self.delay_samples + 1) * self.L) // self.M) + 1

    def take(self, ids, remaining, flush=False):
        from . import resample as _rs
        return _rs.push_width(self.L, self.M, self.T, [self.total[i] for i in ids], remaining, flush)

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], flush=False, out: Optional[torch.Tensor] = None,
             pcm16: bool = False, n_in=None, stream=None):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct); n_in: samples of each row that count (default: all), flush: bool or one per row -- a stream's last
        push, after which it takes no more until reset().  -> (out, counts): out[i, :counts[i]] is what row i emitted, fp32, or int16
        under pcm16 (the arithmetic of Engine.audio_to_pcm16 over the row's resampled chunk, in the same launch).  out: a contiguous
        [>= n, capacity] tensor of that dtype to write into (default: a new one of max_out(samples) columns).  One launch per 16 rows
        on `stream` (default: the device's current torch stream); the counts are host integers, nothing waits for the device."""
        ids, samples, nin, fl = self._args(audio, stream_ids, flush, n_in)
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush = ids[i], nin[i], int(fl[i])
        return out, self._launch(audio, samples, ids, nin, rows, out, pcm16, stream)


class Level(_RowStage):
    """One streaming level configuration of an engine (Engine.level): n_streams chunk-continuous streams at `rate` Hz under one ceiling,
    each at the volume of its first push until its reset (which clears the volume with the rest).  What a stream delivers does not
    depend on how its input was cut into pushes (vibevoice_amd/level.py): the concatenation of its pushes and its flush equals
    Engine.apply_level() of the concatenated input, bit for bit in float mode, as many samples.  delay_samples: the input samples
    (A - 1, 5 ms less one) a stream holds back until its next push; max_in: the input samples one row of a push may bring."""
    KIND, ROW, ROWS_FN, RESET_FN = "level", _lib.VVLevelRow, "vv_level_rows", "vv_level_reset"
    NO_ROWS = (0,)                                        # one launch, which vv_level_rows refuses by name

    def __init__(self, engine: Engine, slot: int, n_streams: int, rate: int = 24000, ceiling_db: float = -1.0):
        from . import level as _lv
        super().__init__(engine, slot, n_streams)
        self.rate, self.ceiling_db = int(rate), float(ceiling_db)
        self.A, self.H = _lv.params(rate)
        self.ceiling = float(_lv.ceiling_of(ceiling_db))
        self.delay_samples, self.max_in = _lv.delay_samples(self.A), _lv.push_width(self.A, self.H)
        engine._chk(engine.lib.vv_level_set(engine._ctx, slot, self.A, self.H, self.ceiling, self.n_streams, engine._s), "vv_level_set")

    def counts(self, stream_id: int, n_in: int, flush: bool = False) -> int:
        """samples a push of n_in samples to stream_id would emit now (host integers, no device sync)"""
        from . import level as _lv
        return _lv.counts(self.A, self.total[stream_id], n_in, flush)[1]

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits, the flush included"""
        return int(n_in) + self.delay_samples

    def take(self, ids, remaining, flush=False):
        return min(self.max_in, max(remaining))

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], volumes_db=0.0, flush=False, out: Optional[torch.Tensor] = None,
             n_in=None, stream=None, pcm16: bool = False):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) at volumes_db[i] (or one volume for all rows; a stream keeps the volume of its first push); n_in:
        samples of each row that count (default: all), flush: bool or one per row -- a stream's last push, after which it takes no
        more until reset().  -> (out, counts): out[i, :counts[i]] is what row i emitted, fp32, or int16 under pcm16 (the arithmetic of
        Engine.audio_to_pcm16 over the row's own output, in the same launch; its rescale never fires, the peak is within the
        ceiling).  out: a contiguous [>= n, capacity] tensor of that dtype to write into (default: a new one of max_out(samples)
        columns).  One launch per 16 rows on `stream` (default: the device's current torch stream); the counts are host integers,
        nothing waits for the device.  A row of more than max_in samples is refused: push it in pieces of take()."""
        from . import level as _lv
        ids, samples, nin, fl, vols = self._args(audio, stream_ids, flush, n_in, volumes_db=volumes_db)
        gains = [float(_lv.gain_of(v)) for v in vols]
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush, rows[i].gain = ids[i], nin[i], int(fl[i]), gains[i]
        return out, self._launch(audio, samples, ids, nin, rows, out, pcm16, stream)


class Pause(_RowStage):
    """One streaming pause configuration of an engine (Engine.pause): n_streams chunk-continuous streams at `rate` Hz, each with the caps
    and the threshold of its first push until its reset (which clears them with the rest).  What a stream delivers does not depend on how
    its input was cut into pushes (vibevoice_amd/pause.py): the concatenation of its pushes and its flush equals pause.shorten() of the
    concatenated input, bit for bit in float mode.  The one stage whose counts depend on the data: push() returns them as a DEVICE
    tensor, and total[] counts input samples only.  delay_samples: the input samples (seg - 1, under 10 ms) that wait for their segment
    to fill; silence, never speech, waits longer (up to ten segments).  max_in: the input samples one row of a push may bring."""
    KIND, ROW, ROWS_FN, RESET_FN = "pause", _lib.VVPauseRow, "vv_pause_rows", "vv_pause_reset"

    def __init__(self, engine: Engine, slot: int, n_streams: int, rate: int = 24000):
        from . import pause as _ps
        super().__init__(engine, slot, n_streams)
        self.seg, self.rate = _ps.seg_of(rate), int(rate)   # refuses a rate outside 8 .. 48 kHz, by name
        self.delay_samples, self.max_in = self.seg - 1, _ps.MAX_IN
        wt = np.ascontiguousarray(np.concatenate(_ps.weights(rate)))
        engine._chk(engine.lib.vv_pause_set(engine._ctx, slot, self.seg, C.c_void_p(wt.ctypes.data), self.n_streams, engine._s), "vv_pause_set")

    def max_out(self, n_in: int) -> int:
        """upper bound of what any push of up to n_in samples emits, the flush included: the open segment and ten held ones with it"""
        from . import pause as _ps
        return _ps.max_out(n_in, self.rate)

    def take(self, ids, remaining, flush=False):
        return min(self.max_in, max(remaining))

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], max_pause_ms=None, max_lead_ms=None, threshold_db=-50.0,
             flush=False, out: Optional[torch.Tensor] = None, n_in=None, stream=None, pcm16: bool = False):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) under max_pause_ms[i], max_lead_ms[i] (None: no cap / max_pause_ms applies) and threshold_db[i] (or
        one value for all rows; a stream keeps the parameters of its first push); n_in: samples of each row that count (default: all),
        flush: bool or one per row -- a stream's last push, after which it takes no more until reset().  -> (out, counts_dev):
        out[i, :counts_dev[i]] is what row i emitted, fp32, or int16 under pcm16 (the arithmetic of Engine.audio_to_pcm16 over the
        row's own emitted samples, in the same launch); counts_dev: int32 [n] on the device, written by the launch -- the host does
        not know them, and reading them waits for `stream`.  out: a contiguous [>= n, capacity >= max_out(samples)] tensor of that
        dtype to write into (default: a new one).  One launch per 16 rows on `stream` (default: the device's current torch stream);
        nothing waits for the device.  A row of more than max_in samples is refused: push it in pieces of take()."""
        from . import pause as _ps
        ids, samples, nin, fl, mp, ml, th = self._args(audio, stream_ids, flush, n_in, max_pause_ms=max_pause_ms, max_lead_ms=max_lead_ms,
                                                       threshold_db=threshold_db)
        par = [_ps.caps(self.rate, a, b) + (_ps.theta(self.rate, c),) for a, b, c in zip(mp, ml, th)]
        e, n, out = self.engine, len(ids), self._out(out, len(ids), nin, pcm16)
        ts = stream if stream is not None else torch.cuda.current_stream(e.device)
        with torch.cuda.stream(ts):
            cnts = torch.zeros(max(n, 1), dtype=torch.int32, device=e.device)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush, rows[i].seg = ids[i], nin[i], int(fl[i]), self.seg
            rows[i].C, rows[i].C0, rows[i].theta = par[i]
        cap = int(out.shape[1])
        for i0 in range(0, n, 16) or (0,):                   # no rows: one launch, which vv_pause_rows refuses by name
            nn = min(16, n - i0)
            a = C.c_void_p(audio.data_ptr() + i0 * samples * 4) if audio is not None else C.c_void_p()
            o = C.c_void_p(out.data_ptr() + i0 * cap * out.element_size())
            self._refused(e.lib.vv_pause_rows(e._ctx, e._sp(ts), self.slot, nn, C.cast(C.byref(rows, i0 * C.sizeof(self.ROW)), C.POINTER(self.ROW)),
                                              a, samples, o, cap, int(pcm16), C.c_void_p(cnts.data_ptr() + i0 * 4)))
            for i in range(i0, i0 + nn):
                self.total[ids[i]] += nin[i]
        return out, cnts[:n]

    def totals(self, ids: Optional[Sequence[int]] = None, stream=None):
        """(taken, emitted, dropped) samples of streams `ids` (default: all), read from the device: this call WAITS for `stream`
        (default: the device's current torch stream), the one the pushes ran on"""
        e = self.engine
        ids = list(range(self.n_streams)) if ids is None else [int(i) for i in ids]
        if not ids:
            return []
        st = e._sp(stream if stream is not None else torch.cuda.current_stream(e.device))
        tot = (C.c_longlong * (3 * len(ids)))()
        e._chk(e.lib.vv_pause_totals(e._ctx, st, self.slot, len(ids), (C.c_int * len(ids))(*ids), tot), "vv_pause_totals")
        return [(int(tot[3 * i]), int(tot[3 * i + 1]), int(tot[3 * i + 2])) for i in range(len(ids))]

    def dropped(self, ids: Optional[Sequence[int]] = None, stream=None):
        """the samples streams `ids` (default: all) have dropped so far, a list of ints.  It synchronises: the totals live on the
        device, this call waits for `stream` (default: the device's current torch stream)."""
        return [t[2] for t in self.totals(ids, stream)]


class Loudness(_RowStage):
    """One streaming loudness configuration of an engine (Engine.loudness): n_streams chunk-continuous adaptive levellers at 24 kHz,
    each with the target, start gain and upper bound of its first push until its reset (which clears them with the rest).  What a stream
    delivers does not depend on how its input was cut into pushes (vibevoice_amd/loudness.py): the concatenation of its pushes equals
    Engine.apply_loudness() of the concatenated input, bit for bit, as many samples; nothing is held back (delay_samples = 0) and the
    flush emits nothing.  max_in: the input samples one row of a push may bring.  fp32 only: a level stage follows this one."""
    KIND, ROW, ROWS_FN, RESET_FN = "loudness", _lib.VVLoudRow, "vv_loud_rows", "vv_loud_reset"
    NO_ROWS = (0,)                                        # one launch, which vv_loud_rows refuses by name

    def __init__(self, engine: Engine, slot: int, n_streams: int):
        from . import loudness as _ld
        super().__init__(engine, slot, n_streams)
        self.rate, self.delay_samples, self.max_in = _ld.RATE, 0, _ld.push_width()
        h = np.ascontiguousarray(_ld.taps())
        engine._chk(engine.lib.vv_loud_set(engine._ctx, slot, C.c_void_p(h.ctypes.data), self.n_streams, engine._s), "vv_loud_set")

    def counts(self, stream_id: int, n_in: int, flush: bool = False) -> int:
        """samples a push of n_in samples to stream_id would emit now: as many as it brings"""
        from . import loudness as _ld
        return _ld.counts(self.total[stream_id], n_in, flush)[1]

    def max_out(self, n_in: int) -> int:
        """what a push of up to n_in samples emits at most: n_in (at least one column: a flush that brings nothing still names rows)"""
        return max(int(n_in), 1)

    def take(self, ids, remaining, flush=False):
        return min(self.max_in, max(remaining))

    def push(self, audio: Optional[torch.Tensor], stream_ids: Sequence[int], targets_lufs, start_db=0.0, max_boost_db=12.0, flush=False,
             out: Optional[torch.Tensor] = None, n_in=None, stream=None, pcm16: bool = False):
        """Row i of audio [n, samples] (contiguous fp32 on the engine's device; None where no row brings samples) goes to stream
        stream_ids[i] (distinct) with targets_lufs[i], start_db[i] and max_boost_db[i] (or one value for all rows; a stream keeps the
        parameters of its first push); n_in: samples of each row that count (default: all), flush: bool or one per row -- a stream's
        last push, after which it takes no more until reset().  -> (out, counts): out[i, :counts[i]] is what row i emitted, fp32,
        counts[i] = n_in[i].  out: a contiguous fp32 [>= n, capacity] tensor to write into (default: a new one).  Two kernel launches per
        16 rows on `stream` (default: the device's current torch stream); nothing waits for the device.  A row of more than max_in
        samples is refused: push it in pieces of take().  pcm16 is refused by name: the stage is never the last one."""
        from . import loudness as _ld
        ids, samples, nin, fl, tg, sd, mb = self._args(audio, stream_ids, flush, n_in, targets_lufs=targets_lufs, start_db=start_db,
                                                       max_boost_db=max_boost_db)
        par = [(float(_ld.target_of(a)), float(_ld.start_of(b)), float(_ld.boost_of(c))) for a, b, c in zip(tg, sd, mb)]
        n, out = len(ids), self._out(out, len(ids), nin, pcm16)
        rows = (self.ROW * max(n, 1))()
        for i in range(n):
            rows[i].stream, rows[i].n_in, rows[i].flush = ids[i], nin[i], int(fl[i])
            rows[i].t, rows[i].g0, rows[i].wmax = par[i]
        return out, self._launch(audio, samples, ids, nin, rows, out, pcm16, stream)
