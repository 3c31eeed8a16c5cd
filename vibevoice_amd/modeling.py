"""Host-side mirror of the reference's inference class for the hot path.

`VibeVoiceForConditionalGenerationInference` here keeps the reference's public
surface for this path (vibevoice/modular/modeling_vibevoice_inference.py):

    from_pretrained(path, torch_dtype=..., device_map=..., attn_implementation=...)   demo/inference_from_file.py:297-317
    .model.{language_model, prediction_head, acoustic_connector, semantic_connector, ...}   :87-117, lora_loading.py:88-169
    eval(), set_ddpm_inference_steps(num_steps)                                         :146-147
    generate(**processor_outputs, max_new_tokens, cfg_scale, tokenizer, generation_config,
             verbose, is_prefill, audio_streamer, stop_check_fn, refresh_negative, ...)  :326-348
      -> VibeVoiceGenerationOutput(sequences, speech_outputs, reach_max_step_sample)     :38-51,691-695

but every tensor op of the loop body (:432-675) and of sample_speech_tokens
(:697-710) executes in libvvhip.so.  The Python below only does what the
reference also does on the host: token bookkeeping, stop checks, streamer calls.

Differences from the reference that do not change results:
  * per-utterance compact KV caches instead of a left-padded batch + masks
    (pads carry no information; position = cumsum(mask)-1 = compact index);
  * the CFG-negative LM row is evaluated speculatively in the same weight pass
    as the positive row (it consumes the same embedding, :579-581); if the sampled
    token turns out not to be <speech_diffusion> the appended cache entry is
    dropped by not advancing the negative length -- exactly what the reference's
    mask fix-ups (:594-624) achieve;
  * finished rows are not forwarded (the reference forwards them and discards);
  * lm_head is evaluated only on the <=5 ids the constraint processor allows
    (:53-66, :405-419): identical argmax / identical softmax over the allowed set.

Beyond the reference: `generate_continuous()` keeps up to n_slots
utterances in flight on one GPU and admits the next queued utterance into a slot the
moment its occupant finishes, without draining the batch; every utterance comes out
exactly as generate() would have produced it alone (the reference's batched loop has
no cross-sample arithmetic, :393-394,549,573,594).
"""
import json
import contextlib
import os
import threading
import time
import warnings
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional, Sequence

import numpy as np
import torch

from . import noise as _noise
from . import schedule as _schedule
from .engine import Engine, EngineConfig, map_param_name

_WARNED_QUEUED_RNG = False


@contextlib.contextmanager
def _end_streamer_on_error(streamer):
    """an exception out of the generate loops (an engine error, a failed request) must not leave an AudioStreamer consumer blocked in
    get() forever: every stream is ended before the exception travels on"""
    try:
        yield
    except BaseException:
        if streamer is not None:
            try:
                streamer.end()
            except Exception:
                pass
        raise


MAX_BATCH = 8          # rows of one diffusion-head pass (2 per utterance, 16-row MFMA tile); vv_diffusion_sample's limit


@dataclass
class BenchHooks:
    """What a measurement harness (bench.py) may hang on generate() / generate_continuous() through `_bench_hooks=`: nothing
    in here changes what is computed for the positions generate() itself fills.
      step_callback(step)      called at the top of every loop iteration (timed-region marks, profiler windows, host-delay probe)
      kv_start, kv_fill_fn     long-context decode measurement: after the real prompt prefill the positive cache is declared
                               kv_start positions long and kv_fill_fn(engine, cache, p0, p1) writes the positions in between"""
    step_callback: Optional[Callable[[int], None]] = None
    kv_start: int = 0
    kv_fill_fn: Optional[Callable] = None


@dataclass
class VibeVoiceGenerationOutput:
    """modeling_vibevoice_inference.py:38-51"""
    sequences: torch.LongTensor = None
    speech_outputs: Optional[List[Optional[torch.Tensor]]] = None
    reach_max_step_sample: Optional[torch.BoolTensor] = None


def engine_config_from_reference(cfg: dict, **runtime) -> EngineConfig:
    """cfg: the dict form of VibeVoiceConfig (vibevoice/configs/qwen2.5_*.json)."""
    d = cfg["decoder_config"]
    h = cfg["diffusion_head_config"]
    a = cfg["acoustic_tokenizer_config"]
    s = cfg.get("semantic_tokenizer_config")
    depths = a["encoder_depths"]
    depths = [int(x) for x in depths.split("-")] if isinstance(depths, str) else list(depths)
    if a.get("decoder_depths") not in (None, "", []):
        dd = a["decoder_depths"]
        dd = [int(x) for x in dd.split("-")] if isinstance(dd, str) else list(dd)
        if dd != list(reversed(depths)):
            raise ValueError("decoder_depths other than reversed(encoder_depths) are not supported")
    if s is not None:
        sd = s["encoder_depths"]
        sd = [int(x) for x in sd.split("-")] if isinstance(sd, str) else list(sd)
        if sd != depths or list(s["encoder_ratios"]) != list(a["encoder_ratios"]) or s["encoder_n_filters"] != a["encoder_n_filters"]:
            raise ValueError("semantic and acoustic encoders must share depths/ratios/filters")
    if a.get("decoder_ratios") not in (None, []) and list(a["decoder_ratios"]) != list(a["encoder_ratios"]):
        raise ValueError("decoder_ratios != encoder_ratios is not supported")
    for k, v in (("mixer_layer", "depthwise_conv"), ("layernorm", "RMSNorm"), ("pad_mode", "constant"), ("conv_norm", "none")):
        if a.get(k, v) != v:
            raise ValueError(f"acoustic_tokenizer_config.{k}={a.get(k)!r} is not supported by the HIP codec")
    kw = dict(
        lm_hidden=d["hidden_size"], lm_layers=d["num_hidden_layers"], lm_heads=d["num_attention_heads"],
        lm_kv_heads=d["num_key_value_heads"], lm_inter=d["intermediate_size"], lm_vocab=d["vocab_size"],
        lm_eps=d.get("rms_norm_eps", 1e-6), rope_theta=d.get("rope_theta", 1e6),
        head_layers=h.get("head_layers", 4), head_ffn_ratio=h.get("head_ffn_ratio", 3.0),
        latent_dim=h.get("latent_size", 64), head_eps=h.get("rms_norm_eps", 1e-5),
        n_filters=a.get("decoder_n_filters", 32), ratios=tuple(a["encoder_ratios"]), enc_depths=tuple(depths),
        sem_dim=(s["vae_dim"] if s is not None else 0), codec_eps=a.get("layernorm_eps", 1e-5),
        max_ctx=d.get("max_position_embeddings", 32768),
    )
    kw.update(runtime)
    return EngineConfig(**kw)


# ---------------------------------------------------------------------- the attribute surface callers read
class _Ns(dict):
    """dict with attribute access (config objects: `model.config.decoder_config.hidden_size`)."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k)
        return _Ns(v) if isinstance(v, dict) and not isinstance(v, _Ns) else v

    def __setattr__(self, k, v):
        self[k] = v

    def to_dict(self):
        return dict(self)


class WeightHandle:
    """What `model.model.<component>` is on the HIP path: the reference keeps an nn.Module there; here the weights live
    repacked inside the engine, and this handle is the write side of that snapshot.  It supports what the reference's
    callers do with the attribute (lora_loading.py:71-84,112-131,163-169; demo/inference_from_file.py:367-368):
    `load_state_dict(sd, strict=False)` (uploads -> the engine re-packs), `.to(device)`, `.eval()`, `.config`,
    `.device`, `parameters()` (one placeholder tensor, enough for `next(model.parameters()).device`)."""

    def __init__(self, owner, ref_prefix: str, config: Optional[dict] = None, to_engine=None, to_reference=None):
        self._owner = owner
        self._ref_prefix = ref_prefix
        self.config = _Ns(config or {})
        # reference state_dict key <-> engine parameter name (the streaming model splits its layers differently)
        self._to_engine = to_engine or map_param_name
        self._to_reference = to_reference or _engine_name_to_reference

    @property
    def device(self):
        return self._owner.device

    @property
    def dtype(self):
        return self._owner.dtype

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def parameters(self):
        yield self._owner._param_placeholder

    def expected_keys(self):
        """state_dict keys (relative to this component) the engine holds"""
        out = []
        for name in self._owner.engine.expected_weights():
            key = self._to_reference(name)
            if key is not None and key.startswith(self._ref_prefix):
                out.append(key[len(self._ref_prefix):])
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        """Upload a (partial) state dict of this component; returns (missing, unexpected) like nn.Module."""
        eng = self._owner.engine
        exp = eng.expected_weights()
        seen, unexpected = set(), []
        for k, v in state_dict.items():
            name = self._to_engine(self._ref_prefix + k)
            if name is None or name not in exp:
                unexpected.append(k)
                continue
            eng.upload(name, v)
            seen.add(k)
        if seen and hasattr(self._owner, "_bump_weights_epoch"):
            self._owner._bump_weights_epoch()        # prompt prefixes computed under the old weights are stale
        missing = [k for k in self.expected_keys() if k not in seen]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict({self._ref_prefix}): missing {missing[:4]}, unexpected {unexpected[:4]}")
        import collections
        return collections.namedtuple("IncompatibleKeys", "missing_keys unexpected_keys")(missing, unexpected)


_PREFIX_BACK = tuple((a, b) for a, b in (
    ("model.language_model.", "lm."), ("model.prediction_head.", "head."),
    ("model.acoustic_tokenizer.decoder.", "dec."), ("model.acoustic_tokenizer.encoder.", "aenc."),
    ("model.semantic_tokenizer.encoder.", "senc."), ("model.acoustic_connector.", "ac_conn."),
    ("model.semantic_connector.", "sem_conn.")))


class _SchedulerView:
    """`noise_scheduler` as callers use it (modeling_vibevoice_inference.py:91-93; demo/gradio_demo.py:142-146): `.config` (the
    DPMSolverMultistepScheduler init arguments the model class passes, modeling_vibevoice.py:138-142, plus that class's
    defaults), `.num_inference_steps`, `.timesteps`, and `.from_config(config, **overrides)` -> a new view, which the gradio
    demo assigns back to `model.model.noise_scheduler` to switch the solver to 'sde-dpmsolver++'.  The arithmetic itself
    lives in the engine's coefficient table (vibevoice_amd/schedule.py)."""

    DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="cosine", trained_betas=None,
                    solver_order=2, prediction_type="v_prediction", thresholding=False, dynamic_thresholding_ratio=0.995,
                    sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                    euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero",
                    lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
                    rescale_betas_zero_snr=False)

    def __init__(self, config: dict, num_inference_steps: Optional[int] = None):
        self.config = _Ns(dict(self.DEFAULTS, **{k: v for k, v in dict(config).items() if k in self.DEFAULTS}))
        self.num_inference_steps = num_inference_steps

    def from_config(self, config, **kwargs):
        return _SchedulerView(dict(dict(config), **kwargs), self.num_inference_steps)

    @property
    def timesteps(self):
        from . import schedule as _schedule
        n = self.num_inference_steps or 20
        if _schedule.is_shipped(self.config):
            tv, _ = _schedule.make_table(n, False)
        else:                       # the configuration's own spacing, offset and lambda cut, as the reference's set_timesteps(n) lists them
            tv, _ = _schedule.general_timesteps_and_sigmas(self.config, n)
        return torch.from_numpy(np.asarray(tv)).long()

    TRAINING = "a property of how the checkpoint was trained, not of how it is sampled"
    REFERENCE_FAILS = "the reference itself fails on this model's [2n, 64] latents"

    def check_supported(self):
        """The configurations the HIP sampler implements: every combination of the reference's sampling-time settings
        (schedule.SAMPLING_KEYS) -- the two shipped configurations on the shipped sampler, the rest through the general table.
        Anything else fails loudly, naming the key and why it stays refused, rather than running a different solver."""
        from . import schedule as _schedule
        c = self.config
        bad = {}
        for k, v in dict(num_train_timesteps=1000, trained_betas=None, prediction_type="v_prediction", rescale_betas_zero_snr=False,
                         variance_type=None).items():
            if c[k] != v:
                bad[k] = (c[k], self.TRAINING)
        if c["beta_schedule"] not in ("cosine", "squaredcos_cap_v2"):          # the same Glide cosine betas (dpm_solver.py:240-242)
            bad["beta_schedule"] = (c["beta_schedule"], self.TRAINING)
        for k, exc in (("use_karras_sigmas", "KeyError: 'sigma_min'"), ("thresholding", "TypeError in reshape"),
                       ("use_lu_lambdas", "IndexError at 20 steps")):
            if c[k]:
                bad[k] = (c[k], f"{self.REFERENCE_FAILS} ({exc})")
        bad.update(_schedule.check_solver(c))
        if bad:
            raise NotImplementedError("noise scheduler configuration not implemented by the HIP sampler: "
                                      + "; ".join(f"{k}={v!r}: {why}" for k, (v, why) in bad.items()))
        if not _schedule.is_shipped(c) and self.num_inference_steps:
            _schedule.general_timesteps_and_sigmas(c, self.num_inference_steps)      # a steps_offset that leaves [0, 1000): ValueError


def _engine_name_to_reference(name: str):
    for a, b in _PREFIX_BACK:
        if name.startswith(b):
            return a + name[len(b):]
    return None


class _ModelNamespace:
    """`model.model` (VibeVoiceModel, modeling_vibevoice.py:108-146) as far as callers read it."""

    def __init__(self, owner, config: dict, attn_implementation: str):
        d = dict(config.get("decoder_config", {}))
        d["_attn_implementation"] = attn_implementation
        self.language_model = WeightHandle(owner, "model.language_model.", d)
        self.prediction_head = WeightHandle(owner, "model.prediction_head.", config.get("diffusion_head_config"))
        self.acoustic_tokenizer = WeightHandle(owner, "model.acoustic_tokenizer.", config.get("acoustic_tokenizer_config"))
        self.acoustic_connector = WeightHandle(owner, "model.acoustic_connector.")
        if config.get("semantic_tokenizer_config") is not None:
            self.semantic_tokenizer = WeightHandle(owner, "model.semantic_tokenizer.", config.get("semantic_tokenizer_config"))
            self.semantic_connector = WeightHandle(owner, "model.semantic_connector.")
        self._owner = owner

    @property
    def speech_scaling_factor(self):
        return torch.tensor(self._owner._scaling)

    @property
    def speech_bias_factor(self):
        return torch.tensor(self._owner._bias)

    @property
    def noise_scheduler(self):
        return self._owner.noise_scheduler

    @noise_scheduler.setter
    def noise_scheduler(self, view):
        # demo/gradio_demo.py:142-146: model.model.noise_scheduler = model.model.noise_scheduler.from_config(config, algorithm_type=...)
        if not isinstance(view, _SchedulerView):
            raise TypeError("model.model.noise_scheduler takes the object noise_scheduler.from_config(...) returns")
        view.check_supported()
        self._owner._sched_cfg = dict(view.config)


class _LaneStreamer:
    """one lane's view of the caller's AudioStreamer in generate_interleaved: the lane's request j is the caller's sample idx[j]; the
    lane's closing end() ends only the lane's own samples (the caller's streamer is closed once, after every lane has finished)"""

    def __init__(self, inner, idx):
        self.inner, self.idx = inner, [int(i) for i in idx]
        self._ended = set()

    @property
    def finished_flags(self):
        ff = getattr(self.inner, "finished_flags", None)
        return [bool(ff[i]) for i in self.idx] if ff is not None else [False] * len(self.idx)

    def put(self, chunks, sample_indices):
        self.inner.put(chunks, torch.tensor([self.idx[int(i)] for i in sample_indices.tolist()]))

    def end(self, sample_indices=None):
        ids = self.idx if sample_indices is None else [self.idx[int(i)] for i in sample_indices.tolist()]
        ids = [i for i in ids if i not in self._ended]          # one end per sample, as one generate() call gives
        self._ended.update(ids)
        if ids:
            self.inner.end(torch.tensor(ids))


class PromptPrefix:
    """The K/V of a prompt head that many requests share -- system prompt, ` Voice input:`, the speakers' voice blocks -- computed
    once (model.build_prompt_prefix) and copied in front of every request that starts with it (generate(prompt_prefix=...)): the
    voice samples are not encoded again and the LM runs over the rest of the prompt only.  Holds the engine's snapshot of positions
    [0, n_pos) of the positive cache (device resident, independent of max_ctx: a fork()ed lane restores it), the n_pos token ids
    and the speech positions it was computed from (a request is checked against both), the model geometry and the weights epoch
    of the model that built it (a prefix is refused after the weights changed).  The voice latents' noise is ONE draw, fixed when
    the prefix was built -- the reference draws it per call (_process_speech_inputs); the Streaming presets fix it the same way."""
    FORMAT = "vibevoice_amd.prompt_prefix.v1"

    def __init__(self, k, v, n_pos, ids, speech_pos, geometry, epoch, weights_token=None, model=None):
        self.k, self.v = k, v
        self.n_pos = int(n_pos)
        self.ids = [int(i) for i in ids]
        self.speech_pos = sorted(int(p) for p in speech_pos)
        self.geometry = tuple(int(g) for g in geometry)       # (layers, kv heads, head dim)
        self.epoch = int(epoch)
        self._weights_token = weights_token                   # identity of the weight copy (shared by a model and its forks)
        self._model = model
        if len(self.ids) != self.n_pos:
            raise ValueError(f"a prefix of {self.n_pos} positions holds {len(self.ids)} token ids")

    def __repr__(self):
        return f"PromptPrefix(n_pos={self.n_pos}, speech_positions={len(self.speech_pos)}, geometry={self.geometry}, epoch={self.epoch})"

    def save(self, path):
        """One torch.save file: per-layer bf16 K/V in HF layout [kv_heads, n_pos, head_dim] (keys rotated, as cached) plus the
        metadata -- independent of the tile layout of the build that wrote it.  Goes through KV cache 0 of the model that built the
        prefix as scratch (restore, then export layer by layer): not while that model generates."""
        m = self._model
        if m is None:
            raise RuntimeError("PromptPrefix.save: the prefix is not attached to a model (build_prompt_prefix / load attach it)")
        m._check_prefix(self)
        e = m.engine
        with torch.cuda.stream(e.stream):
            e.kv_restore(0, self.n_pos, self.k, self.v)
            layers = [e.kv_export(0, l, 0, self.n_pos, dtype=torch.bfloat16) for l in range(self.geometry[0])]
        e.sync()
        torch.save({"format": self.FORMAT, "n_pos": self.n_pos, "ids": list(self.ids), "speech_pos": list(self.speech_pos),
                    "geometry": list(self.geometry), "k": [k.cpu() for k, _ in layers], "v": [v.cpu() for _, v in layers]}, path)

    @classmethod
    def load(cls, path, model):
        """Read a saved prefix into `model`: kv_import_at into KV cache 0 (scratch; not while the model generates), then a snapshot.
        The file does not say which weights it was computed with: loading one under other weights is the caller's mistake, as with
        the Streaming presets."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") != cls.FORMAT:
            raise ValueError(f"{path} is not a saved PromptPrefix")
        geo = tuple(int(g) for g in d["geometry"])
        if geo != model._kv_geometry():
            raise ValueError(f"the prefix was saved for (layers, kv heads, head dim) = {geo}; this model has {model._kv_geometry()}")
        n = int(d["n_pos"])
        e = model.engine
        with torch.cuda.stream(e.stream):
            for l in range(geo[0]):
                e.kv_import_at(0, l, 0, d["k"][l].to(e.device), d["v"][l].to(e.device))
            k, v = e.kv_snapshot(0, n)
        e.sync()
        return cls(k, v, n, d["ids"], d["speech_pos"], geo, model.weights_epoch, model._epoch_box, model)


def _speakers_of_rows(need, have):
    """Voice sample i contributes have[i] speech rows; the batch rows consume them in order, need[b] each (_process_speech_inputs +
    the masked scatter, :149-163,470-474).  -> the sample indices of every row, or None when a sample spans two rows."""
    out, i = [], 0
    for nb in need:
        got, mine = 0, []
        while got < nb:
            if i >= len(have):
                return None
            mine.append(i)
            got += have[i]
            i += 1
        if got != nb:
            return None
        out.append(mine)
    return out


def _speech_positions(speech_input_mask_row, attention_mask_row):
    """positions of a row's speech tokens within its unpadded prompt: an int64 index tensor on the host (the masks are the
    processor's host data: no device count)"""
    return speech_input_mask_row.cpu()[attention_mask_row.bool().cpu()].to(torch.bool).nonzero().squeeze(1)


def _cfg_scale_values(cfg_scale, n, what):
    """cfg_scale of one call -> n finite Python floats, one per utterance.  A real number stands for every row; a sequence or 1-D
    tensor / array carries one value per row.  ValueError on a wrong length, a non-finite value or anything that is not a real
    number -- on the host, before anything is enqueued."""
    import math
    import numbers
    if isinstance(cfg_scale, (torch.Tensor, np.ndarray)):
        if cfg_scale.ndim > 1:
            raise ValueError(f"{what}: cfg_scale has {cfg_scale.ndim} dimensions; a number or one value per utterance ({n}) is expected")
        vals = cfg_scale.tolist()
        seq = cfg_scale.ndim == 1
        vals = vals if seq else [vals]
    elif isinstance(cfg_scale, (list, tuple)):
        vals, seq = list(cfg_scale), True
    else:
        vals, seq = [cfg_scale], False
    out = []
    for v in vals:
        if isinstance(v, torch.Tensor) and v.ndim == 0:
            v = v.item()
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"{what}: cfg_scale {v!r} is not a real number")
        v = float(v)
        if not math.isfinite(v):
            raise ValueError(f"{what}: cfg_scale {v!r} is not finite")
        out.append(v)
    if not seq:
        return out * n
    if len(out) != n:
        raise ValueError(f"{what}: cfg_scale holds {len(out)} values for {n} utterances")
    return out


def _request_cfg_scales(requests, cfg_scale, what):
    """the guidance scale of every request of a queue: its own "cfg_scale" key, else the call's argument"""
    default = _cfg_scale_values(cfg_scale, 1, what)[0]
    return [_cfg_scale_values(r["cfg_scale"], 1, f"{what}, request {i}")[0] if r.get("cfg_scale") is not None else default
            for i, r in enumerate(requests)]


def _seed_values(seed, n, what):
    """seed of one generate() call -> n entries, each an int in [0, 2**64) or None (a row without a seed of its own).  One int stands
    for a one-row call only: a row's draws must not depend on its batch index, so several rows take one seed each."""
    if seed is None:
        return [None] * n
    if isinstance(seed, (list, tuple)):
        if len(seed) != n:
            raise ValueError(f"{what}: seed holds {len(seed)} entries for {n} rows (one int or None per row)")
        return [None if v is None else _noise.check_seed(v, f"{what}: seed[{i}]") for i, v in enumerate(seed)]
    seed = _noise.check_seed(seed, f"{what}: seed")
    if n != 1:
        raise ValueError(f"{what}: one seed for {n} rows -- pass one seed per row (a list with an int or None for every row): a row's "
                         "result must not depend on its batch index")
    return [seed]


def _resolve_seeds(seeds, cpu_gen=None):
    """The seeds of a call's requests (ints or None) -> None when no request carries one (the call takes the torch generators' path,
    draw for draw), else one seed per request: the requests without one get theirs from ONE torch.randint on the session's CPU
    generator, in request order."""
    if all(v is None for v in seeds):
        return None
    out = list(seeds)
    miss = [i for i, v in enumerate(out) if v is None]
    if miss:
        drawn = torch.randint(0, 2 ** 63 - 1, (len(miss),), dtype=torch.int64, generator=cpu_gen).tolist()
        for i, v in zip(miss, drawn):
            out[i] = int(v)
    return out


def _request_seeds(requests, what):
    return [None if r.get("seed") is None else _noise.check_seed(r["seed"], f"{what}, request {i}: seed") for i, r in enumerate(requests)]


_NO_VALID_TOKEN_LEFT = ("the full-vocabulary logits processors (top_k / top_p / min_p) removed every valid speech token "
                        "of a row: nothing is left to sample from (the reference fails in torch.multinomial here: "
                        "'probability tensor contains either `inf`, `nan` or element < 0')")


@dataclass(slots=True)
class _Session:
    """What one generate() / generate_continuous() call holds beside its utterances (_session builds it; every field has a default, so
    a caller of one stage -- a test, a tool -- names only what that stage reads)."""
    sde: bool = False                              # the stochastic solver ('sde-dpmsolver++')
    solver_steps: int = 0                          # general solver table: the steps the reference's set_timesteps yields (0: ddpm_inference_steps)
    sde_noise_fn: Optional[Callable] = None        # test hook: the recorded variance draws
    nv: int = 0                                    # number of valid ids
    valid_t: Optional[torch.Tensor] = None         # the valid ids in the engine's order (host, int64)
    start_id: Optional[int] = None
    end_id: Optional[int] = None
    diff_id: Optional[int] = None
    eos_id: Optional[int] = None
    pad_id: Optional[int] = None
    cfg_scale: float = 1.0                         # the call's guidance scale
    cfg_rows: bool = False                         # the utterances carry different scales (_cfg_arg)
    do_sample: bool = False
    temperature: float = 1.0
    warp: Optional[dict] = None                    # the full-vocabulary processors' settings (_generation_options); None: none asked for
    trace: Any = None
    audio_streamer: Any = None
    verbose: bool = False
    forced: Any = None                             # test / bench hooks: token plan per row, noise_fn(step, rows), teacher(step, rows)
    noise_fn: Optional[Callable] = None
    teacher: Optional[Callable] = None
    n_rows: int = 0
    refresh_negative: bool = True
    lockstep: bool = True                          # the rows are one batch of the reference's loop (False: independent requests)
    sample_rows: Optional[Callable] = None         # order -> the row ids of the torch.multinomial call (_choose_tokens)
    seeds: Optional[List[int]] = None              # one seed per request when the call runs the counter path (noise.py)
    cpu_gen: Optional[torch.Generator] = None      # the session's own generators (generate_interleaved gives every lane a pair); None: the
    dev_gen: Optional[torch.Generator] = None      # process-global CPU / device generators, i.e. the reference's RNG streams
    frame_rows: int = 0                            # rows of the frame store written so far
    n_frames: int = 0
    step: int = 0                                  # the caller's loop iteration
    _seen: dict = field(default_factory=dict)      # repetition penalty, torch path: {idx: [seen mask [V], tokens folded in]}
    _seen_dev: dict = field(default_factory=dict)  # ... device path: {idx: tokens folded in} (the masks are rows of the model's _seen_buf)

    @property
    def seeded(self) -> bool:
        """the call is on the counter path: no draw touches a torch generator"""
        return self.seeds is not None


class _Utt:
    """One utterance in flight: its engine slot (KV caches 2*slot / 2*slot+1, codec states), lengths and outputs."""
    __slots__ = ("idx", "slot", "ids", "seq_len0", "init_len", "max_length", "max_steps", "max_step_sample", "step", "pos_len",
                 "neg_len", "have_embeds", "finished", "reach_max", "tokens", "chunks", "last", "forced", "noise_fn", "req",
                 "t_admit", "t_done", "neg_book", "cfg_scale", "seed", "n_lat")

    def __init__(self, idx, slot, ids, seq_len0, max_length, max_length_times, start_id):
        self.idx, self.slot, self.ids = idx, slot, ids
        self.seq_len0 = seq_len0                      # width of the (padded) prompt batch this utterance arrived in
        self.init_len = len(ids)
        self.max_length = max_length
        self.max_steps = min(max_length - seq_len0, int(max_length_times * seq_len0))               # :421 (loop length)
        self.max_step_sample = min(max_length - self.init_len, int(max_length_times * self.init_len))    # :422
        self.step = 0
        self.pos_len = self.neg_len = 0
        self.have_embeds = False
        self.finished = self.reach_max = False
        self.tokens, self.chunks = [], []
        self.last = ids[-1] if ids else start_id
        self.forced = self.noise_fn = self.req = None
        self.t_admit = self.t_done = None
        self.cfg_scale = None                         # this utterance's guidance scale (a session with mixed scales; else the session's)
        self.seed = None                              # the request's seed (a call on the counter path, noise.py); else None
        self.n_lat = 0                                # latents accepted so far: counter word t of the seeded solver noise
        # the reference's bookkeeping of this row's negative cache, without the tensors: [attention mask incl. the next token's slot,
        # entries ever appended, corrections so far (correct_cnt)] -- to recognise the one correction that keeps THIS step's entry (vv_kv_move)
        self.neg_book = [[1], 0, 0]


class _AudioRates:
    """What both model classes offer around the 24 kHz the tokenizers work at (self.engine: the class's Engine)."""

    def resample_audio(self, audio: torch.Tensor, dst_rate: int, src_rate: int = 24000) -> torch.Tensor:
        """audio [samples] or [n, samples] at src_rate -> fp32 on the engine's device at dst_rate, ceil(samples * dst / src) samples
        (Engine.resample).  For speech_outputs after the fact -- resample_audio(out.speech_outputs[0], 48000) -- and for a voice
        sample before the processor, which wants 24 kHz: resample_audio(wav, 24000, src_rate=44100).  generate() itself stays at 24 kHz."""
        return self.engine.resample(audio, int(src_rate), int(dst_rate))

    def time_stretch(self, audio: torch.Tensor, speed: float) -> torch.Tensor:
        """audio [samples] or [n, samples] at 24 kHz -> fp32 on the engine's device at `speed` times the speaking rate (0.5 .. 2.0), the
        pitch kept, ceil(samples / speed) samples (Engine.time_stretch).  For speech_outputs after the fact --
        time_stretch(out.speech_outputs[0], 1.2); in front of resample_audio where both are wanted.  generate() itself has no rate input."""
        return self.engine.time_stretch(audio, speed)

    def pitch_shift(self, audio: torch.Tensor, semitones: float, speed: float = 1.0, formant=None) -> torch.Tensor:
        """audio [samples] or [n, samples] at 24 kHz -> fp32 on the engine's device, the pitch moved by `semitones` (-12 .. +12) and the
        speaking rate by `speed` (Engine.pitch_shift): a tempo change by speed * Q / P, then resampling by P / Q, samples / speed samples
        to within one and the tempo stage's rounding.  formant=None: a resampling shifter, the formants move with the pitch, so a few
        semitones read as the same voice and more changes its character.  formant=0.0 keeps the voice's formants (a spectral-envelope
        warp by Q / P in front of the resampler), formant=F leaves them F semitones from where they were.  For speech_outputs after the
        fact -- pitch_shift(out.speech_outputs[0], -4, formant=0.0); in place of time_stretch where both are wanted.  generate() itself
        has no pitch input."""
        return self.engine.pitch_shift(audio, semitones, speed, formant=formant)

    def formant_shift(self, audio: torch.Tensor, semitones) -> torch.Tensor:
        """audio [samples] or [n, samples] at 24 kHz -> fp32 on the engine's device, as many samples, the formants moved by `semitones`
        (-12 .. +12; one value, or one per row) and the pitch kept (Engine.formant_warp): timbre, or voice size.  For speech_outputs
        after the fact -- formant_shift(out.speech_outputs[0], -2).  generate() itself has no formant input."""
        return self.engine.formant_warp(audio, semitones)

    def apply_level(self, audio: torch.Tensor, volume_db: float = 0.0, ceiling_db: float = -1.0, rate: int = 24000) -> torch.Tensor:
        """audio [samples] or [n, samples] at `rate` Hz -> fp32 on the engine's device, as many samples: volume_db of gain (-40 .. +24),
        then a look-ahead peak limiter that keeps every sample within ceiling_db (-20 .. 0) of full scale (Engine.apply_level).  For
        speech_outputs after the fact -- apply_level(out.speech_outputs[0], 6.0); behind time_stretch and resample_audio where those
        are wanted, at the rate they deliver.  generate() itself has no level input."""
        return self.engine.apply_level(audio, volume_db, ceiling_db, int(rate))

    def shorten_pauses(self, audio: torch.Tensor, max_pause_ms=None, max_lead_ms=None, threshold_db: float = -50.0, rate: int = 24000):
        """audio [samples] or [n, samples] at `rate` Hz -> (a list of 1-D fp32 tensors on the engine's device, one per signal; the samples
        each dropped): silences (10 ms segments below threshold_db, -80 .. -20) longer than max_pause_ms (100 .. 5000) keep their
        beginning and their end around a 10 ms cross-fade, the lead-in in front of the first loud segment is capped at max_lead_ms
        (0 .. 5000; None: max_pause_ms applies) (Engine.shorten_pauses).  For speech_outputs after the fact --
        shorten_pauses(out.speech_outputs[0], 400, 50); the last step, behind apply_level, at the rate that delivers.  It waits for the
        device: the lengths depend on the data.  generate() itself has no pause input."""
        return self.engine.shorten_pauses(audio, max_pause_ms, max_lead_ms, threshold_db, int(rate))

    def measure_loudness(self, audio: torch.Tensor) -> torch.Tensor:
        """The ITU-R BS.1770-4 loudness in LUFS of audio [samples] or [n, samples] at 24 kHz -> a float64 CPU tensor, one value per row;
        -inf for silence and for less than 400 ms (Engine.measure_loudness).  For speech_outputs, and for a voice sample: its reading
        tells AudioStreamer(loudness_start_db=target - reading) where to start."""
        return self.engine.measure_loudness(audio)

    def normalize_loudness(self, audio: torch.Tensor, target_lufs: float = -16.0, ceiling_db: float = -1.0) -> torch.Tensor:
        """audio [samples] at 24 kHz -> fp32 on the engine's device at target_lufs (-16 for podcasts, -23 for broadcast): one fixed gain
        of target_lufs - measure_loudness(audio) dB, then the peak limiter of apply_level under ceiling_db.  Where the limiter engages
        the result reads below the target.  [n, samples]: each row by its own measurement.  Refused by name: a signal that reads -inf
        (silence, or shorter than 400 ms) and a gain outside apply_level's -40 .. +24 dB."""
        from . import level as _lv
        from . import loudness as _ld
        target = _ld._range("target_lufs", target_lufs, _ld.MIN_TARGET, _ld.MAX_TARGET, "LUFS")
        measured = self.measure_loudness(audio).reshape(-1).tolist()
        vols = []
        for i, m in enumerate(measured):
            if m == float("-inf"):
                raise ValueError(f"normalize_loudness: signal {i} reads -inf LUFS (silence, or shorter than 400 ms): there is no gain that "
                                 "brings it to a target")
            vol = target - m
            if not (_lv.MIN_VOLUME_DB <= vol <= _lv.MAX_VOLUME_DB):
                raise ValueError(f"normalize_loudness: signal {i} reads {m:.2f} LUFS; target_lufs = {target} asks for volume_db = {vol:.2f}, "
                                 f"outside apply_level's [{_lv.MIN_VOLUME_DB}, {_lv.MAX_VOLUME_DB}] dB")
            vols.append(vol)
        if audio.dim() == 1:
            return self.apply_level(audio, vols[0], ceiling_db)
        rows = audio.reshape(-1, audio.shape[-1])
        return torch.stack([self.apply_level(rows[i], vols[i], ceiling_db) for i in range(len(vols))]).reshape(audio.shape)

    def apply_loudness(self, audio: torch.Tensor, target_lufs: float = -16.0, start_db: float = 0.0, max_boost_db: float = 12.0,
                       return_gain: bool = False):
        """audio [samples] or [n, samples] at 24 kHz -> fp32 on the engine's device, as many samples, through the adaptive leveller
        AudioStreamer(loudness_lufs=...) runs while the audio is produced (Engine.apply_loudness): the gain follows the speaker.  No
        limiter: run apply_level behind it.  generate() itself has no loudness input."""
        return self.engine.apply_loudness(audio, target_lufs, start_db, max_boost_db, return_gain=return_gain)


class VibeVoiceForConditionalGenerationInference(_AudioRates):
    """Drop-in for the reference class on the generate() path, backed by libvvhip.so."""

    def __init__(self, config: dict, engine: Engine, model_dtype=torch.bfloat16, attn_implementation: Optional[str] = None):
        self.config_dict = config
        self.config = _Ns(config)
        self.engine = engine
        self.dtype = model_dtype
        self.device = engine.device
        self.ddpm_inference_steps = config["diffusion_head_config"].get("ddpm_num_inference_steps", 20)
        self.max_position_embeddings = config["decoder_config"].get("max_position_embeddings", 32768)
        self.acoustic_vae_dim = config.get("acoustic_vae_dim", 64)
        self.fix_std = config["acoustic_tokenizer_config"].get("fix_std", 0.5)
        self.std_dist_type = config["acoustic_tokenizer_config"].get("std_dist_type", "gaussian")
        self._scaling = float("nan")
        self._bias = float("nan")
        self._valid_key = None
        # what the attention really is on this path; the value the caller asked for is kept beside it
        self.requested_attn_implementation = attn_implementation
        self._param_placeholder = torch.empty(0, dtype=model_dtype, device=self.device)
        hcfg = config["diffusion_head_config"]
        # the scheduler the model class builds (modeling_vibevoice.py:138-142)
        self._sched_cfg = dict(_SchedulerView({"num_train_timesteps": hcfg.get("ddpm_num_steps", 1000),
                                               "beta_schedule": hcfg.get("ddpm_beta_schedule", "cosine"),
                                               "prediction_type": hcfg.get("prediction_type", "v_prediction")}).config)
        self._sde_flat = None                    # per-step variance noise of the stochastic solver, [64 * MAX_BATCH * latent]
        self.model = _ModelNamespace(self, config, "vvhip_mfma_flash_decoding_gfx950")
        H = engine.cfg.lm_hidden
        e = engine
        NB = MAX_BATCH
        self._x_in = e.new(2 * NB, H)
        self._hidden = e.new(2 * NB, H)
        self._hid_fresh = e.new(max(1, engine.cfg.n_slots), H)       # last prompt row of a freshly prefilled utterance, per slot
        self._logits = e.new(2 * NB * 16)                            # dense [n][n_valid] blocks, as vv_lm_logits writes them
        self._cond = e.new(2 * NB, H)
        self._noise = e.new(NB, engine.cfg.latent_dim)
        self._latent = e.new(NB, engine.cfg.latent_dim)
        self._audio = e.new(NB, engine.cfg.hop)
        self._sem = e.new(NB, max(1, engine.cfg.sem_dim))
        self._emb_out = e.new(NB, H)
        self._start_emb = e.new(1, H)
        self._neg_hidden = e.new(NB, H)
        self._nxt_x = e.new(NB, H)
        self._tmp_emb = e.new(NB, H)
        # pinned host staging: the logits come back without a blocking copy, noise goes out without one
        self._logits_pin = torch.empty(2 * NB * 16, dtype=torch.float32).pin_memory()
        self._noise_pin = [torch.empty(NB, engine.cfg.latent_dim, dtype=torch.float32).pin_memory() for _ in range(4)]
        self._noise_i = 0
        # per-row guidance scales of a sampler call: ONE device buffer (its address is in the sampler's graph key), written from a
        # ring of pinned rows; _cfg_staged = what the device buffer holds once the stream gets there
        self._cfg_dev = e.new(NB)
        self._cfg_pin = torch.empty(4, NB, dtype=torch.float32).pin_memory()
        self._cfg_i = 0
        self._cfg_staged = []
        self._lg_event = torch.cuda.Event()
        self._fork_ev = torch.cuda.Event()
        self._join_ev = torch.cuda.Event()
        self._side_streams = [torch.cuda.Stream(device=self.device) for _ in range(min(NB, engine.cfg.n_slots))] if engine.cfg.n_slots > 1 else []
        self._audio_blocks = []                                       # output frames, FRAME_BLOCK steps per block (no per-step allocation)
        self.frame_block = 64
        self._frame_w = min(NB, max(1, engine.cfg.n_slots))           # utterances per row of the frame store (the call's batch / slots)
        self._first_row = None                                        # generate_continuous: {id(utterance): its first frame-store row}
        # allocated on first use: the one-pass prompt buffers, the processors' [16, V] logits, the warp kernel's outputs, its seen rows
        self._pf_buf = self._full_logits = self._warp_out = self._warp_surv = self._seen_buf = None
        self._t_lm_pass = self._t_kv_fill = 0.0                       # VVHIP_TIME_PREFILL: seconds inside the LM launches / the bench's cache fill
        self._lanes = []                                              # generate_interleaved: the fork()ed models, kept until close_lanes()
        # plain attributes (tests flip them): per-utterance tokenizer chains on forked streams; several utterances' chains of a step
        # as ONE engine call (vv_codec_chain_batch); the sampler enqueued speculatively behind the LM pass
        self.concurrent_codecs = True
        self.batched_codecs = hasattr(engine, "codec_chain_batch")
        self.speculate_sampling = True
        # the full-vocabulary logits processors (repetition penalty, top-k / top-p / min-p) as ONE kernel over lm_logits_full's output
        # (vv_lm_warp_valid) instead of the chain of torch ops in _full_vocab_scores; engines without the entry take the torch path
        self.warp_on_device = True
        self.last_stats = {}
        # weights epoch: [count of parameter updates since construction]; one box per weight copy (forks share their parent's).  A
        # PromptPrefix remembers the value it was computed under
        self._epoch_box = [0]
        # device-resident LoRA adapters: {name: (merge_dtype, {engine parameter: (A, B, scale)})} with A / B on the engine device
        self._adapters = {}
        self._active_adapter = None

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_state_dict(cls, config: dict, state_dict, model_dtype=torch.bfloat16, device=None, attn_implementation=None, **runtime):
        """state_dict: mapping (or iterable of (key, tensor)) keyed like the reference checkpoint."""
        runtime.setdefault("max_rows", 512)          # prompt rows per LM weight pass (MFMA tile GEMM above ~48 workgroups)
        ecfg = engine_config_from_reference(config, **runtime)
        eng = Engine(ecfg, device)
        items = state_dict.items() if hasattr(state_dict, "items") else state_dict
        exp = eng.expected_weights()
        scaling = bias = None
        for k, v in items:
            if k == "model.speech_scaling_factor":
                scaling = float(v)
                continue
            if k == "model.speech_bias_factor":
                bias = float(v)
                continue
            name = map_param_name(k)
            if name is not None and name in exp:
                eng.upload(name, v)
        miss = eng.missing_weights()
        if miss:
            raise RuntimeError(f"checkpoint is missing {len(miss)} parameters, e.g. {miss[:4]}")
        m = cls(config, eng, model_dtype, attn_implementation=attn_implementation)
        if scaling is not None and bias is not None:
            m.set_speech_factors(scaling, bias)
        return m

    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.bfloat16, device_map=None, attn_implementation=None, **runtime):
        """Reads config.json + *.safetensors written by the reference's converter
        (scripts/convert_nnscaler_checkpoint_to_transformers.py:119-123)."""
        from safetensors import safe_open
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        files = sorted(fn for fn in os.listdir(path) if fn.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no .safetensors shards under {path}")

        def it():
            for fn in files:
                with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as sf:
                    for k in sf.keys():
                        yield k, sf.get_tensor(k)
        device = None
        if isinstance(device_map, (str, torch.device)) and str(device_map) not in ("auto", "cpu"):
            device = torch.device(device_map)
        # the drop-in entry point: any batch generate() can take (MAX_BATCH utterances) works without an extra argument; the KV
        # caches of 8 slots at the model's full context are 30 GB for the 7B model -- a tenth of the HBM
        runtime.setdefault("n_slots", MAX_BATCH)
        do_warm = runtime.pop("warmup", True)
        m = cls.from_state_dict(config, it(), torch_dtype or torch.bfloat16, device, attn_implementation=attn_implementation, **runtime)
        m.source_path = path
        if do_warm and hasattr(m.engine, "acoustic_encode") and getattr(m.engine, "lib", None) is not None:
            try:
                m.warmup()
            except Exception as ex:         # a failed warm-up costs the first request its latency, never the model load --
                try:                        # unless the device itself is gone: then the load fails here, with the cause
                    torch.cuda.synchronize(m.device)
                    m.engine.sync()
                except Exception as dead:
                    raise RuntimeError(f"vibevoice_amd: warm-up failed ({ex!r}) and the device does not answer any more") from dead
                warnings.warn(f"vibevoice_amd: warm-up failed ({ex!r}); the first generate() will pay the cold-start costs")

        def base_tensor(key):          # lazy access to the checkpoint's own tensors (LoRA merge: vibevoice_amd/lora.py)
            for fn in files:
                with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as sf:
                    if key in sf.keys():
                        return sf.get_tensor(key)
            raise KeyError(key)
        m.base_tensor = base_tensor
        return m

    @classmethod
    def from_reference(cls, live_model, device=None, **runtime):
        """Snapshot a live reference `VibeVoiceForConditionalGenerationInference` (an nn.Module, e.g. one that already carries
        merged adapters) into a HIP-path model: its config.to_dict() + state_dict() + scalar speech factors."""
        cfg = live_model.config.to_dict() if hasattr(live_model.config, "to_dict") else dict(live_model.config)
        sd = live_model.state_dict()
        dt = next(iter(live_model.parameters())).dtype
        runtime.setdefault("n_slots", MAX_BATCH)
        m = cls.from_state_dict(cfg, sd, dt, device, **runtime)
        m.base_tensor = lambda key: sd[key].detach().cpu()
        steps = getattr(live_model, "ddpm_inference_steps", None)
        if steps:
            m.set_ddpm_inference_steps(steps)
        return m

    # ---- reference properties (:87-117) ----
    @property
    def speech_scaling_factor(self):
        return self._scaling

    @property
    def speech_bias_factor(self):
        return self._bias

    @property
    def noise_scheduler(self):
        return _SchedulerView(self._sched_cfg, self.ddpm_inference_steps)

    prediction_head = property(lambda self: self.model.prediction_head)
    acoustic_tokenizer = property(lambda self: self.model.acoustic_tokenizer)
    semantic_tokenizer = property(lambda self: getattr(self.model, "semantic_tokenizer", None))
    acoustic_connector = property(lambda self: self.model.acoustic_connector)
    semantic_connector = property(lambda self: getattr(self.model, "semantic_connector", None))

    def parameters(self):
        yield self._param_placeholder

    def to(self, *a, **k):
        return self

    def tie_weights(self):
        """the engine reads lm_head rows from embed_tokens when no lm_head.weight was uploaded (vv_set_valid_tokens)"""
        self._valid_key = None

    def set_speech_factors(self, scaling, bias):
        self._scaling = float(scaling)
        self._bias = float(bias)
        self.engine.set_speech_factors(scaling, bias)

    def eval(self):
        return self

    def set_ddpm_inference_steps(self, num_steps=None):
        self.ddpm_inference_steps = num_steps or self.config_dict["diffusion_head_config"].get("ddpm_num_inference_steps", 20)

    # ------------------------------------------------------------------ parameter updates on a live model
    @property
    def weights_epoch(self) -> int:
        return self._epoch_box[0]

    def _bump_weights_epoch(self):
        self._epoch_box[0] += 1

    def upload(self, name: str, tensor):
        """One parameter by its ENGINE name ("lm.layers.0.self_attn.q_proj.weight", include/vvhip.h); K/V computed before it is stale."""
        self.engine.upload(name, tensor)
        self._bump_weights_epoch()

    # ------------------------------------------------------------------ device-resident LoRA adapters
    def load_adapter(self, name: str, checkpoint_dir: str, merge_dtype: str = "float32"):
        """Reads the LoRA adapter(s) under checkpoint_dir (lora.read_adapter: language model and diffusion head) and keeps their A / B
        factors on the device under `name`; nothing is merged until set_adapter(name).  merge_dtype: where the delta is rounded, as
        lora.merge_lora.  Memory: the factors, plus -- from the first set_adapter on -- one bf16 base snapshot of every matrix an
        adapter has touched (engine.stat(7) bytes).  Needs no checkpoint on disk for the base model."""
        from . import lora as _lora
        if not isinstance(name, str) or not name:
            raise ValueError("load_adapter: name is a non-empty string")
        if merge_dtype not in _lora.MERGE_DTYPES:
            raise ValueError(f"merge_dtype must be one of {_lora.MERGE_DTYPES}, got {merge_dtype!r}")
        if name == self._active_adapter:
            raise ValueError(f"adapter {name!r} is active: set_adapter(None) or switch before loading another one under its name")
        expected = self.engine.expected_weights() if hasattr(self.engine, "expected_weights") else None
        pairs = _lora.read_adapter(checkpoint_dir, expected)
        shape_of = getattr(self.engine, "_mat_shape", None)
        for k, (a, b, _) in pairs.items():                 # the exact [out, in] of the packed matrix, not only its element count
            nk = shape_of(k) if shape_of is not None else None
            if nk is not None and (int(b.shape[0]), int(a.shape[1])) != nk:
                raise ValueError(f"{checkpoint_dir}: LoRA pair of {k}: B @ A is [{b.shape[0]}, {a.shape[1]}], the parameter is {list(nk)}; "
                                 "use load_lora_assets")
        self._register_adapter(name, pairs, merge_dtype)
        return sorted(pairs)

    def _register_adapter(self, name, pairs, merge_dtype):
        """pairs: {engine parameter name: (A fp32 [r, in], B fp32 [out, r], scale)}, as lora.read_adapter returns them"""
        dev = self.engine.device
        self._adapters[name] = (merge_dtype, {k: (a.to(dev, torch.float32).contiguous(), b.to(dev, torch.float32).contiguous(), float(sc))
                                              for k, (a, b, sc) in pairs.items()})

    def set_adapter(self, name: Optional[str]):
        """Switches the merged adapter in place on the device; None restores the base model.  Calls close_lanes() first (shared
        engine contexts hold snapshots derived from the parameters; lanes are forked again on the next generate_interleaved).
        Parameters the outgoing adapter touched and the incoming one does not are reset to their base; the incoming pairs are merged
        from the base snapshots (never cumulative).  All launches go on the engine stream, with one sync at the end.  The packed
        weights do not move, so captured hipGraphs stay valid; the weights epoch is bumped, so a PromptPrefix built under other
        weights is refused.  Setting the adapter that is already active does nothing.  One batch has one adapter: call between
        generate() calls."""
        if name is not None and name not in self._adapters:
            raise KeyError(name)
        if name == self._active_adapter:
            return
        self.close_lanes()
        eng = self.engine
        old = self._adapters[self._active_adapter][1] if self._active_adapter is not None else {}
        merge_dtype, new = self._adapters[name] if name is not None else ("float32", {})
        for k in old:
            if k not in new:
                eng.lora_reset(k)
        for k, (a, b, sc) in new.items():
            eng.lora_merge(k, a, b, sc, merge_dtype)
        eng.sync()
        self._active_adapter = name
        self._bump_weights_epoch()

    def unload_adapter(self, name: str):
        """Drops a resident adapter's factors (the active one must be switched away from first).  Base snapshots stay."""
        if name not in self._adapters:
            raise KeyError(name)
        if name == self._active_adapter:
            raise ValueError(f"adapter {name!r} is active: set_adapter(None) or switch first")
        del self._adapters[name]

    @property
    def active_adapter(self) -> Optional[str]:
        return self._active_adapter

    def load_state_dict(self, state_dict, strict: bool = True):
        """A (partial) state dict keyed like the reference checkpoint, uploaded into the live engine (which re-packs); returns
        (missing_keys, unexpected_keys) like nn.Module.  Prompt prefixes built before it are refused afterwards."""
        eng = self.engine
        exp = eng.expected_weights()
        seen, unexpected = set(), []
        scaling = bias = None
        for k, v in state_dict.items():
            if k == "model.speech_scaling_factor":
                scaling = float(v)
                continue
            if k == "model.speech_bias_factor":
                bias = float(v)
                continue
            name = map_param_name(k)
            if name is None or name not in exp:
                unexpected.append(k)
                continue
            eng.upload(name, v)
            seen.add(name)
        self._bump_weights_epoch()
        if scaling is not None and bias is not None:
            self.set_speech_factors(scaling, bias)
        missing = [_engine_name_to_reference(n) or n for n in exp if n not in seen and n != "lm.rope.inv_freq"]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:4]}, unexpected {unexpected[:4]}")
        import collections
        return collections.namedtuple("IncompatibleKeys", "missing_keys unexpected_keys")(missing, unexpected)

    # ------------------------------------------------------------------ prompt prefixes (voice presets for this class)
    def _kv_geometry(self):
        c = self.engine.cfg
        return (int(c.lm_layers), int(c.lm_kv_heads), int(c.lm_head_dim))

    def _check_prefix(self, prefix):
        if not isinstance(prefix, PromptPrefix):
            raise TypeError(f"prompt_prefix takes a PromptPrefix (model.build_prompt_prefix / PromptPrefix.load), not {type(prefix).__name__}")
        if prefix.geometry != self._kv_geometry():
            raise ValueError(f"the prompt prefix was built for (layers, kv heads, head dim) = {prefix.geometry}; this model has {self._kv_geometry()}")
        if prefix._weights_token is not self._epoch_box:
            raise RuntimeError("the prompt prefix was built by another model (not this one or a fork() of it): its K/V belongs to other weights")
        if prefix.epoch != self.weights_epoch:
            raise RuntimeError(f"the prompt prefix is stale: it was built at weights epoch {prefix.epoch} and the model's parameters have been "
                               f"updated since (epoch {self.weights_epoch}: load_state_dict / upload / load_lora_assets); build it again")

    def _prefix_plan(self, prefix, ids: List[int], speech_pos: Optional[List[int]]) -> int:
        """How many leading positions of the prompt `ids` come from `prefix`: r = min(prefix.n_pos, len(ids) - 1) -- at least one row goes
        through the LM, its hidden state starts the loop -- after checking that the prompt really starts with the prefix (token ids and
        speech positions below r; a mismatch raises: a silent fallback would hide a wrong voice).  0 = prefill the row in full: no
        prefix, or a speech position of the row at or beyond r (its voice rows are not in the prefix).  speech_pos None: the call
        carries no speech mask, the prefix's own positions are taken."""
        if prefix is None:
            return 0
        self._check_prefix(prefix)
        r = min(prefix.n_pos, len(ids) - 1)
        if r < 1:
            return 0
        if ids[:r] != prefix.ids[:r]:
            p = next(i for i in range(r) if ids[i] != prefix.ids[i])
            raise ValueError(f"prompt_prefix does not match the prompt: token {ids[p]} at position {p}, the prefix holds {prefix.ids[p]}")
        if speech_pos is None:
            if any(p >= r for p in prefix.speech_pos):
                raise ValueError(f"the prompt ends at position {len(ids) - 1}, inside the prefix's voice block, and the call carries no speech inputs")
            return r
        mine, theirs = set(p for p in speech_pos if p < r), set(p for p in prefix.speech_pos if p < r)
        if mine != theirs:
            raise ValueError(f"prompt_prefix does not match the prompt: position {min(mine ^ theirs)} is a speech position in one of them only")
        if any(p >= r for p in speech_pos):
            return 0
        return r

    @staticmethod
    def _prefix_list(prompt_prefix, n_rows):
        if prompt_prefix is None or isinstance(prompt_prefix, PromptPrefix):
            return [prompt_prefix] * n_rows
        if not isinstance(prompt_prefix, (list, tuple)):
            raise TypeError(f"prompt_prefix takes a PromptPrefix or a list of them (None for a row without one), not {type(prompt_prefix).__name__}")
        lst = list(prompt_prefix)
        if len(lst) != n_rows:
            raise ValueError(f"prompt_prefix: {len(lst)} entries for {n_rows} rows (one PromptPrefix for all rows, or one entry or None per row)")
        return lst

    @torch.no_grad()
    def build_prompt_prefix(self, input_ids, speech_tensors=None, speech_masks=None, speech_input_mask=None, attention_mask=None,
                            n_prefix: Optional[int] = None, **kw) -> PromptPrefix:
        """Compute the K/V of the first n_prefix positions of ONE row of processor output and keep it as a PromptPrefix: the voice
        samples go through the acoustic encoder and the connector, the LM runs over the head (engine slot 0), the positive cache is
        snapshotted.  n_prefix defaults to one past the last True of speech_input_mask (the whole voice block); without a speech
        mask it is required.  _prefill_noise=(r1, r2) fixes the voice latents' noise as in generate(); without it the draw comes from
        the device generator -- either way the prefix holds ONE draw for every request that uses it, where the reference draws per
        call (_process_speech_inputs), exactly as the Streaming presets do.  Not while the model generates."""
        e = self.engine
        prefill_noise = kw.pop("_prefill_noise", None)
        seed = kw.pop("seed", None)                # the voice draws of the prefix as a function of this seed (noise.py); None: the device generator
        if seed is not None:
            seed = _noise.check_seed(seed, "build_prompt_prefix(): seed")
        input_ids = input_ids.cpu()
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
        if input_ids.shape[0] != 1:
            raise ValueError("build_prompt_prefix takes one row of processor output")
        am = torch.ones_like(input_ids) if attention_mask is None else attention_mask.cpu().reshape(1, -1)
        keep = am[0].bool()
        ids = input_ids[0][keep].tolist()
        sp_all = []
        if speech_input_mask is not None:
            sp_all = _speech_positions(speech_input_mask.reshape(1, -1)[0], keep).tolist()
        if n_prefix is None:
            if not sp_all:
                raise ValueError("build_prompt_prefix: n_prefix is required when the row has no speech positions")
            n_prefix = sp_all[-1] + 1
        n_prefix = int(n_prefix)
        if not 1 <= n_prefix <= len(ids):
            raise ValueError(f"n_prefix = {n_prefix} outside [1, {len(ids)}] (the row's unpadded prompt)")
        if n_prefix > e.max_ctx:
            raise ValueError(f"n_prefix = {n_prefix} exceeds the engine's max_ctx {e.max_ctx}")
        sp = [p for p in sp_all if p < n_prefix]
        with torch.cuda.stream(e.stream):
            rows = pos = None
            if sp:
                if speech_tensors is None or speech_masks is None:
                    raise ValueError("build_prompt_prefix: the row has speech positions; speech_tensors and speech_masks are required")
                pos = torch.tensor(sp, dtype=torch.long).to(self.device)
                _, emb = self._process_speech_inputs(speech_tensors, speech_masks, prefill_noise,
                                                     seeds=None if seed is None else [(seed, i) for i in range(speech_tensors.shape[0])])
                if emb.shape[0] < len(sp):
                    raise ValueError("speech_masks hold fewer frames than speech_input_mask marks")
                rows = emb[:len(sp)]
            u = _Utt(0, 0, ids[:n_prefix], n_prefix, n_prefix, 2, 0)
            self._prefill_checked([(u, u.ids, rows, pos, 0, None)])
            k, v = e.kv_snapshot(0, n_prefix)
        e.sync()               # complete before any other stream (a lane's) reads it
        return PromptPrefix(k, v, n_prefix, ids[:n_prefix], sp, self._kv_geometry(), self.weights_epoch, self._epoch_box, self)

    def warmup(self, prompt_rows: Optional[Sequence[int]] = None, voice_frames: int = 75):
        """Touch everything the first request needs, so that its time to first audio is a warm process's: the first launch of
        a kernel pays for its code object and launch attributes, and the first use of a torch op on the device (the Gaussian
        draw of the voice-prompt latents, the masked scatter of the speech rows, ...) loads its module -- measured on the 7B
        north-star request: voice-prompt encode 0.098 s cold against 0.03-0.04 s warm.  Runs (a) one LM prompt pass per entry
        of `prompt_rows` (default: a full max_rows pass and a ragged remainder) and (b) a REAL generate() on a synthetic
        one-speaker request (`voice_frames`-frame silent voice prompt, short prompt, three forced frames, explicit noise), i.e.
        the request path itself: encoder, connectors, prompt scatter, decode steps under the graph keys generate() uses,
        sampler, both tokenizers, the streamer hand-off.  Draws nothing from any RNG (noise is passed in; the device
        generator's state is saved and restored around it) and leaves no state behind: caches are overwritten by the next
        prefill, codec states are zeroed at the start of every generate()."""
        import types
        e = self.engine
        H, hop, L = e.cfg.lm_hidden, e.cfg.hop, e.cfg.latent_dim
        R = e.cfg.max_rows
        cap = max(1, min(R, e.max_ctx - 16))                    # never more rows than one LM launch takes (max_rows may be 2..7)
        if prompt_rows is None:
            prompt_rows = sorted({cap, max(1, min(cap, cap // 3 + 5))}, reverse=True)
        rng = torch.cuda.get_rng_state(self.device)
        saved_valid, saved_stats = getattr(e, "_valid_ids", None), dict(self.last_stats)
        try:
            with torch.cuda.stream(e.stream):
                for n in prompt_rows:
                    n = int(max(1, min(n, cap)))
                    x = torch.zeros(n, H, dtype=torch.float32, device=self.device)
                    hid = torch.empty_like(x)
                    if hasattr(e, "lm_forward_span"):
                        e.lm_forward_span(0, 0, n, x, hid)
                    else:
                        e.lm_forward([(0, j) for j in range(n)], x, hid)
                    del x, hid
            e.sync()
            has_voice = bool(getattr(e.cfg, "has_acoustic_encoder", False)) and voice_frames > 0
            vf = voice_frames if has_voice else 0
            n_prompt = int(min(cap, e.max_ctx - 16, vf + 24))
            vf = max(0, min(vf, n_prompt - 8))
            tok = types.SimpleNamespace(speech_start_id=0, speech_end_id=1, speech_diffusion_id=2, eos_token_id=3, bos_token_id=None)
            ids = torch.full((1, n_prompt), 4 % e.cfg.lm_vocab, dtype=torch.long)
            sim = torch.zeros(1, n_prompt, dtype=torch.bool)
            kw = {}
            if vf > 0:
                ids[0, 4:4 + vf] = tok.speech_diffusion_id
                sim[0, 4:4 + vf] = True
                kw = dict(speech_tensors=torch.zeros(1, vf * hop), speech_masks=torch.ones(1, vf, dtype=torch.bool), speech_input_mask=sim,
                          _prefill_noise=(torch.zeros(1), torch.zeros(1, vf, L)))
            ids[0, -1] = tok.speech_start_id
            D = tok.speech_diffusion_id
            scaled = not (self._scaling != self._scaling)              # speech factors may not be set yet (NaN): use neutral ones here
            if not scaled:
                self.engine.set_speech_factors(1.0, 0.0)
                self._scaling, self._bias = 1.0, 0.0
            # through an AudioStreamer, as a serving request goes: its copy stream exists and its pinned ring buffers sit in the
            # streamer module's pool afterwards, so the first real request's first chunk does not wait for pinned allocations
            from .streamer import AudioStreamer
            st = AudioStreamer(batch_size=1)
            try:
                self.generate(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=tok, cfg_scale=1.3,
                              generation_config={"do_sample": False}, max_new_tokens=4, show_progress_bar=False, audio_streamer=st,
                              _forced_tokens=[[D, D, D, tok.eos_token_id]], _noise_fn=lambda step, n2: torch.zeros(n2, L), **kw)
            finally:
                st.close()
            if not scaled:
                self._scaling = self._bias = float("nan")
            self._valid_key = None
        finally:
            torch.cuda.set_rng_state(rng, self.device)
            if saved_valid:                                       # the synthetic request's control-token ids must not outlive it
                e.set_valid_tokens(saved_valid)
            elif hasattr(e, "_valid_ids"):
                e._valid_ids = None
            self.last_stats = saved_stats
        e.sync()

    # ------------------------------------------------------------------ helpers
    def _embed_ids(self, ids: List[int], out: torch.Tensor):
        ch = getattr(self.engine, "embed_chunk", 64)         # one call per prompt chunk, not per 64 ids
        for i0 in range(0, len(ids), ch):
            self.engine.embed(ids[i0:i0 + ch], out[i0:])

    def _stage_noise(self, nz, n):
        """noise rows -> device without blocking the host (pageable H2D copies are synchronous with the stream)"""
        if nz.is_cuda:
            self._noise[:n].copy_(nz[:n].to(torch.float32))
            return
        pin = self._noise_pin[self._noise_i]
        self._noise_i = (self._noise_i + 1) % len(self._noise_pin)
        pin[:n].copy_(nz[:n])
        self._noise[:n].copy_(pin[:n], non_blocking=True)

    def _cfg_arg(self, S, utts):
        """cfg_scale of one sampler call over `utts` (in the order of its condition rows): the session's float when every request of
        the session has the same scale -- the scalar kernels and graphs -- else a view of the one staging buffer holding each row's own
        scale.  The values travel host -> pinned -> device on the engine stream without a sync; nothing is copied while the rows and
        their scales are what the buffer already holds."""
        if not S.cfg_rows:
            return S.cfg_scale
        vals = [u.cfg_scale for u in utts]
        n = len(vals)
        if self._cfg_staged[:n] != vals:
            pin = self._cfg_pin[self._cfg_i]
            self._cfg_i = (self._cfg_i + 1) % self._cfg_pin.shape[0]
            pin[:n] = torch.tensor(vals, dtype=torch.float32)
            self._cfg_dev[:n].copy_(pin[:n], non_blocking=True)
            self._cfg_staged[:n] = vals
        return self._cfg_dev[:n]

    def _voice_normals(self, seeds, frames):
        """(r1 [n_spk], r2 [n_spk, frames, latent]) of seeded voice samples on the device: seeds[i] = (the request's seed, the sample's
        speaker index within its request).  r2 = stream 0x80000001 (rows = speakers, t = frame, aux = speaker) through vv_noise_rows;
        r1 = normal 0 of quad 0 of stream 0x80000002 (aux = speaker), on the host: n_spk numbers per request."""
        e = self.engine
        L, n_spk = e.cfg.latent_dim, len(seeds)
        r1 = torch.stack([_noise.normals(sd, 0, 1, _noise.STREAM_VOICE_SCALE, 1, spk, 4)[0, 0, 0] for sd, spk in seeds])
        if hasattr(e, "noise_rows") and L % 4 == 0:
            r2 = torch.empty(n_spk, frames, L, dtype=torch.float32, device=self.device)
            for i0 in range(0, n_spk, 16):
                e.noise_rows([(sd, 0, spk) for sd, spk in seeds[i0:i0 + 16]], _noise.STREAM_VOICE, 1, frames, L, r2[i0:])
        else:
            r2 = torch.cat([_noise.normals(sd, 0, frames, _noise.STREAM_VOICE, 1, spk, L) for sd, spk in seeds])
        return r1.to(self.device, torch.float32), r2.to(self.device, torch.float32)

    def _process_speech_inputs(self, speech_tensors, speech_masks, prefill_noise=None, dev_gen=None, seeds=None):
        """_process_speech_inputs (:149-163): encode voice prompts, sample, scale, connect.
        dev_gen: a lane's own device generator (generate_interleaved); None = the device's global generator, as the reference.
        seeds: one (seed, speaker index within its request) per voice sample of a call on the counter path (noise.py) -- no generator
        is touched then; an explicit prefill_noise keeps precedence.
        Every host -> device copy of the call (waveform, frame selection, explicit noise) goes out BEFORE the encoder is enqueued:
        a pageable copy blocks the host until the stream has drained, and a boolean-mask gather synchronises to count its rows --
        behind the encoder either one keeps the prompt pass from being enqueued while the encoder runs."""
        e = self.engine
        hop = e.cfg.hop
        n_spk, S = speech_tensors.shape
        frames = S // hop
        valid = None
        if frames * hop != S:
            # the batch tensor does not end on a frame: the engine takes whole frames of zero-padded waveform plus the signal length --
            # the reference right-pads per strided conv LAYER (zeros, not the activations of a zero waveform), which only the last,
            # partial frame's latent can tell (vv_acoustic_encode_ragged)
            pad = (frames + 1) * hop - S
            speech_tensors = torch.nn.functional.pad(speech_tensors, (0, pad))
            frames += 1
            valid = S
        if tuple(speech_masks.shape) != (n_spk, frames):
            # the reference's feats[speech_masks] raises on a mask that does not have the encoder output's shape; a flattened gather
            # would silently pick other rows
            raise ValueError(f"speech_masks has shape {tuple(speech_masks.shape)}; {n_spk} voice samples of {S} samples give "
                             f"({n_spk}, {frames}) frames (ceil(S / {hop}))")
        wav = speech_tensors.to(self.device, torch.float32).contiguous()
        # rows of the [n_spk * frames] encoder output that are real frames (speech_masks is the processor's host data)
        sel_idx = speech_masks.reshape(-1).to(torch.bool).cpu().nonzero().squeeze(1).to(self.device)
        if prefill_noise is not None:
            prefill_noise = tuple(t.to(self.device, torch.float32) for t in prefill_noise)
        elif seeds is not None and self.std_dist_type in ("gaussian", "fix"):
            if len(seeds) != n_spk:
                raise ValueError(f"{len(seeds)} seeds for {n_spk} voice samples")
            prefill_noise = self._voice_normals(list(seeds), frames)
        mean = e.new(n_spk, frames, e.cfg.latent_dim)
        for i in range(n_spk):
            e.acoustic_encode(frames, wav[i], mean[i], valid_samples=valid)
        if self.std_dist_type == "gaussian":
            if prefill_noise is None:
                # VibeVoiceTokenizerEncoderOutput.sample('gaussian'), modular_vibevoice_tokenizer.py:980-989:
                # two draws from the device generator.  The reference's `mean` is latents.permute(0, 2, 1) (:1085) and its noise is
                # randn_like(mean): the same call on a tensor with the same strides is what stays on the reference's RNG stream
                # (a contiguous draw takes a different generator path).  Pinned by tests/golden/generate_sampled_b1.npz.
                if dev_gen is not None:
                    r1 = torch.randn(n_spk, device=self.device, dtype=torch.float32, generator=dev_gen)
                    r2 = torch.randn(tuple(mean.shape), device=self.device, dtype=torch.float32, generator=dev_gen)
                else:
                    r1 = torch.randn(n_spk, device=self.device, dtype=torch.float32)
                    r2 = torch.randn_like(torch.empty(n_spk, mean.shape[2], mean.shape[1], device=self.device, dtype=torch.float32).permute(0, 2, 1))
            else:
                r1, r2 = prefill_noise
            lat = mean + (r1 * (self.fix_std / 0.8))[:, None, None] * r2
        elif self.std_dist_type == "fix":
            if prefill_noise is not None:
                r2 = prefill_noise[1]
            elif dev_gen is not None:
                r2 = torch.randn(tuple(mean.shape), device=self.device, dtype=torch.float32, generator=dev_gen)
            else:
                r2 = torch.randn_like(torch.empty(n_spk, mean.shape[2], mean.shape[1], device=self.device).permute(0, 2, 1))
            lat = mean + self.fix_std * r2
        else:
            lat = mean
        feats = ((lat + self._bias) * self._scaling).contiguous()
        sel = feats.reshape(n_spk * frames, -1).index_select(0, sel_idx)   # [n_valid, 64]: feats[speech_masks] without the count sync
        out = e.new(sel.shape[0], e.cfg.lm_hidden)
        e.connect(sel.shape[0], sel, None, out)
        return feats, out

    @staticmethod
    def _generation_options(generation_config):
        """generation_config: None, a dict (what every reference caller passes: the reference does
        GenerationConfig(**generation_config), :261-266) or an object with to_dict() (an HF GenerationConfig)."""
        if generation_config is None:
            gc = {}
        elif isinstance(generation_config, dict):
            gc = dict(generation_config)
        elif hasattr(generation_config, "to_dict"):
            gc = {k: v for k, v in generation_config.to_dict().items() if v is not None}
            # an HF GenerationConfig object carries its class defaults (top_k=50, ...): only what differs from them is a request
            for k, dflt in (("top_k", 50), ("top_p", 1.0), ("repetition_penalty", 1.0), ("temperature", 1.0)):
                if gc.get(k) == dflt:
                    gc.pop(k)
        else:
            raise TypeError(f"generation_config must be a dict, None or have to_dict(); got {type(generation_config).__name__}")
        do_sample = bool(gc.get("do_sample", False))
        temperature = float(gc.get("temperature", 1.0) or 1.0)
        # processors this path does not implement: refuse them instead of silently decoding from something else
        for k in ("typical_p", "epsilon_cutoff", "eta_cutoff", "top_h", "no_repeat_ngram_size", "encoder_no_repeat_ngram_size",
                  "bad_words_ids", "num_beams", "num_beam_groups", "penalty_alpha", "diversity_penalty", "sequence_bias",
                  "suppress_tokens", "begin_suppress_tokens", "forced_bos_token_id", "forced_eos_token_id", "min_length",
                  "min_new_tokens", "exponential_decay_length_penalty", "guidance_scale", "encoder_repetition_penalty",
                  "renormalize_logits", "watermarking_config"):
            v = gc.get(k)
            if v not in (None, 0, 0.0, 1, 1.0, [], ()):
                raise NotImplementedError(f"generation_config[{k!r}]={v!r} is not implemented on the HIP path")
        # The processors that act on the FULL vocabulary in front of the valid-token constraint (HF's list, :310-319, then the
        # constraint appended at :416-419): repetition penalty (also without sampling), and with do_sample the warpers
        # temperature -> top-k -> top-p -> min-p.  transformers==4.51.3 (the reference's pin) defaults top_k to 50 whenever
        # do_sample is set: an absent top_k means 50 here too; top_k=0 / None switches it off.  Any of them routes the token
        # choice through vv_lm_logits_full (one pass over the whole lm_head per step) instead of the <= 16 valid rows.
        rep = float(gc.get("repetition_penalty") or 1.0)
        warp = None
        if do_sample:
            top_k = int((gc["top_k"] if "top_k" in gc else 50) or 0)
            top_p = float(gc["top_p"]) if gc.get("top_p") is not None else 1.0
            min_p = float(gc.get("min_p") or 0.0)
            if top_k < 0 or not (0.0 <= top_p <= 1.0) or not (0.0 <= min_p <= 1.0):
                raise ValueError(f"top_k={top_k}, top_p={top_p}, min_p={min_p}: out of range")
            if top_k > 0 or top_p < 1.0 or min_p > 0.0 or rep != 1.0:
                warp = dict(top_k=top_k, top_p=top_p, min_p=min_p, repetition_penalty=rep)
        elif rep != 1.0:
            warp = dict(top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=rep)
        if rep <= 0.0:
            raise ValueError(f"repetition_penalty={rep} must be > 0")
        return do_sample, temperature, warp

    def _full_vocab_scores(self, hidden: torch.Tensor, order, S) -> torch.Tensor:
        """[n, lm_vocab] scores of the given positive rows after the reference's full-vocabulary logits processors, in HF's order
        (generation/utils.py `_get_logits_processor`): repetition penalty over the row's input_ids (left padding, prompt and
        generated tokens), then -- with do_sample -- temperature, top-k, top-p, min-p (min_tokens_to_keep = 1).  The valid-token
        constraint comes after them (the caller)."""
        e, w = self.engine, S.warp
        n, V = hidden.shape[0], e.cfg.lm_vocab
        if self._full_logits is None or self._full_logits.numel() < 16 * V:
            self._full_logits = torch.empty(16 * V, dtype=torch.float32, device=self.device)
        hidden = hidden.to(torch.float32).contiguous()
        parts = []
        for i0 in range(0, n, 16):
            k = min(16, n - i0)
            e.lm_logits_full(k, hidden[i0:i0 + k], self._full_logits)
            parts.append(self._full_logits[:k * V].view(k, V).clone())
        scores = torch.cat(parts)                    # (the step loop runs under torch.cuda.stream(engine.stream): one ordered stream)
        if w["repetition_penalty"] != 1.0:
            # RepetitionPenaltyLogitsProcessor: every id present in the row's input_ids (left padding, prompt, generated tokens) is
            # penalised once.  The row's "seen" set is a [V] mask kept on the device for the session and extended by the tokens
            # generated since the last step: O(1) per step, not O(history) (a 90-minute utterance has ~40 K of them).
            pen = w["repetition_penalty"]
            seen = S._seen
            for i, u in enumerate(order):
                ent = seen.get(u.idx)
                if ent is None:
                    base = list(u.ids) + ([S.pad_id] if (u.seq_len0 > u.init_len and S.pad_id is not None) else [])
                    mask = torch.zeros(V, dtype=torch.bool, device=scores.device)
                    mask[torch.tensor([int(t) for t in base if 0 <= int(t) < V], dtype=torch.long, device=scores.device)] = True
                    ent = seen[u.idx] = [mask, 0]
                fresh_tok = [int(t) for t in u.tokens[ent[1]:] if 0 <= int(t) < V]
                if fresh_tok:
                    ent[0][torch.tensor(fresh_tok, dtype=torch.long, device=scores.device)] = True
                ent[1] = len(u.tokens)
                sc = scores[i]
                scores[i] = torch.where(ent[0], torch.where(sc < 0, sc * pen, sc / pen), sc)
        if S.do_sample:
            if S.temperature != 1.0:
                scores = scores / S.temperature
            if w["top_k"] > 0:
                kth = torch.topk(scores, min(w["top_k"], V))[0][..., -1, None]
                scores = scores.masked_fill(scores < kth, float("-inf"))
            if w["top_p"] < 1.0:
                srt, idx = torch.sort(scores, descending=False)
                remove = srt.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - w["top_p"])
                remove[..., -1:] = False
                scores = scores.masked_fill(remove.scatter(1, idx, remove), float("-inf"))
            if w["min_p"] > 0.0:
                probs = torch.softmax(scores, dim=-1)
                remove = probs < w["min_p"] * probs.amax(dim=-1, keepdim=True)
                idx = torch.argsort(scores, descending=True, dim=-1)
                srt_remove = torch.gather(remove, dim=-1, index=idx)
                srt_remove[..., :1] = False
                scores = scores.masked_fill(srt_remove.scatter(1, idx, srt_remove), float("-inf"))
        return scores

    def _warp_valid_scores(self, hidden: torch.Tensor, order, S) -> torch.Tensor:
        """[n, n_valid] scores of the valid ids of the given positive rows after the same processors as _full_vocab_scores and the
        valid-token constraint (-inf where a filter removed an id), from vv_lm_warp_valid: no [n, V] clone and no torch op over the
        vocabulary.  _warp_surv[:n] holds how many valid ids every row keeps (_valid_scores refuses a row without one)."""
        e, w = self.engine, S.warp
        n, V, nv = hidden.shape[0], e.cfg.lm_vocab, S.nv
        if self._full_logits is None or self._full_logits.numel() < 16 * V:
            self._full_logits = torch.empty(16 * V, dtype=torch.float32, device=self.device)
        if self._warp_out is None or self._warp_out.numel() < n * 16:
            self._warp_out = torch.empty(max(16, n) * 16, dtype=torch.float32, device=self.device)
            self._warp_surv = torch.empty(max(16, n), dtype=torch.int32, device=self.device)
        hidden = hidden.to(torch.float32).contiguous()
        pen = w["repetition_penalty"]
        if pen != 1.0:
            # the rows' "seen" sets (RepetitionPenaltyLogitsProcessor: left padding, prompt, generated tokens) are rows of one
            # [slots][V] byte buffer on the device, one per engine slot, extended by the tokens generated since the last step --
            # the same ids in the same order as the dict of bool masks of _full_vocab_scores
            n_rows = max(int(getattr(e.cfg, "n_slots", 1)), max(u.slot for u in order) + 1)
            if self._seen_buf is None or self._seen_buf.shape[0] < n_rows or self._seen_buf.shape[1] != V:
                self._seen_buf = torch.zeros(n_rows, V, dtype=torch.uint8, device=self.device)
                S._seen_dev = {}
            done = S._seen_dev
            flat = []                                 # every row's new ids as positions of the flat buffer: one upload, one scatter per step
            for u in order:
                if u.idx not in done:
                    self._seen_buf[u.slot].zero_()    # once per utterance: the slot's previous owner
                    fresh_tok = list(u.ids) + ([S.pad_id] if (u.seq_len0 > u.init_len and S.pad_id is not None) else [])
                    done[u.idx] = 0
                else:
                    fresh_tok = []
                flat += [u.slot * V + int(t) for t in fresh_tok + list(u.tokens[done[u.idx]:]) if 0 <= int(t) < V]
                done[u.idx] = len(u.tokens)
            if flat:
                self._seen_buf.view(-1)[torch.tensor(flat, dtype=torch.long, device=self.device)] = 1
        for i0 in range(0, n, 16):
            k = min(16, n - i0)
            e.lm_logits_full(k, hidden[i0:i0 + k], self._full_logits)
            # the kernel takes dense rows: one launch per run of consecutive slots (one launch unless an earlier row has finished)
            j0 = 0
            while j0 < k:
                j1 = k if pen == 1.0 else j0 + 1
                while j1 < k and order[i0 + j1].slot == order[i0 + j1 - 1].slot + 1:
                    j1 += 1
                e.lm_warp_valid(j1 - j0, self._full_logits[j0 * V:], self._seen_buf[order[i0 + j0].slot:].reshape(-1) if pen != 1.0 else None,
                                self._warp_out[(i0 + j0) * nv:], self._warp_surv[i0 + j0:], repetition_penalty=pen,
                                temperature=S.temperature, do_sample=S.do_sample, top_k=w["top_k"], top_p=w["top_p"], min_p=w["min_p"])
                j0 = j1
        return self._warp_out[:n * nv].view(n, nv)

    # ------------------------------------------------------------------ prompt prefill of one utterance
    def _prefill(self, u: _Utt, ids: List[int], speech_rows: Optional[torch.Tensor], speech_pos: Optional[torch.Tensor],
                 kv_start: int = 0, kv_fill_fn=None, prefix: Optional[PromptPrefix] = None, pos0: int = 0):
        """LM prefill of one utterance's prompt into KV cache 2*slot; the last row's hidden state -> _hid_fresh[slot].
        prefix / pos0 (_prefix_plan): the first pos0 positions are restored from the prefix's snapshot and the LM runs over ids[pos0:]
        only, appended behind them (speech rows all lie below pos0 then)."""
        e = self.engine
        H = e.cfg.lm_hidden
        if prefix is not None:
            e.kv_restore(2 * u.slot, prefix.n_pos, prefix.k, prefix.v)
            ids = ids[pos0:]
            speech_rows = speech_pos = None
        n = len(ids)
        CH = e.cfg.max_rows          # prompt rows per weight pass
        if n <= CH:
            # one-pass prompts (the common case) reuse two persistent [max_rows, H] buffers: a fresh 2 x 150 MB allocation per
            # request is milliseconds of hipMalloc; every row is overwritten by the embedding lookup, no zero fill needed
            if self._pf_buf is None or self._pf_buf.shape[1] < n:
                with torch.cuda.stream(e.stream):
                    self._pf_buf = torch.empty(2, CH, H, dtype=torch.float32, device=self.device)
            emb = self._pf_buf[0, :n]
            hid = self._pf_buf[1, :n]
        else:
            emb = e.new(n, H)
            hid = e.new(CH, H)
        self._embed_ids(ids, emb)
        if speech_rows is not None and speech_pos is not None and speech_rows.shape[0]:
            if speech_pos.dtype == torch.bool:
                emb[speech_pos] = speech_rows                   # boolean mask: counts its rows on the host (a sync)
            else:
                emb.index_copy_(0, speech_pos, speech_rows)     # int64 positions, uploaded by the caller ahead of the encoder
        timed = os.environ.get("VVHIP_TIME_PREFILL") is not None
        if timed:                    # split the reported prefill time: embedding + voice-row scatter | LM passes
            e.sync(); torch.cuda.current_stream(self.device).synchronize(); t_emb = time.perf_counter()
        for i0 in range(0, n, CH):
            k = min(CH, n - i0)
            if hasattr(e, "lm_forward_span"):
                e.lm_forward_span(2 * u.slot, pos0 + i0, k, emb[i0:i0 + k], hid)
            else:
                e.lm_forward([(2 * u.slot, pos0 + i0 + j) for j in range(k)], emb[i0:i0 + k], hid)
        self._hid_fresh[u.slot].copy_(hid[(n - 1) % CH])
        if timed:
            e.sync(); torch.cuda.current_stream(self.device).synchronize()
            self._t_lm_pass += time.perf_counter() - t_emb
        n = u.pos_len = pos0 + n
        if kv_start > n:             # bench hook: decode measured at a long context (kv_fill_fn supplies the cache contents)
            if kv_fill_fn is not None:
                timed = os.environ.get("VVHIP_TIME_PREFILL") is not None
                if timed:            # keep the bench-only cache fill out of the reported prompt-prefill time
                    e.sync(); t0 = time.perf_counter()
                kv_fill_fn(e, 2 * u.slot, n, kv_start)
                if timed:
                    e.sync(); torch.cuda.current_stream(self.device).synchronize()
                    self._t_kv_fill += time.perf_counter() - t0
            u.pos_len = kv_start

    def _prefill_checked(self, jobs):
        """_prefill for every (utterance, ids, speech rows, speech positions, kv_start, kv_fill_fn) of `jobs`; prompts long enough for the
        prefill GEMM's K-split round (>= 1024 rows) are waited for and checked before the first frame is enqueued: a lost hand-off
        (vv_check: the engine re-arms itself and says the pass in flight is invalid) is answered by ONE repeat of the prompt passes --
        they only overwrite the same cache positions.  The wait costs nothing measurable: the first frame's launches would have
        queued behind the prompt pass anyway."""
        e = self.engine
        for attempt in (0, 1):
            for j in jobs:
                self._prefill(*j)
            if max(len(j[1]) for j in jobs) < 1024:
                return
            try:
                e.sync()
                return
            except RuntimeError as ex:
                if attempt or "K-split" not in str(ex):
                    raise
                warnings.warn(f"vibevoice_amd: {ex}; repeating the prompt pass once", RuntimeWarning)

    def _block_rows(self, i: int):
        """row i of the frame store: [utterances in flight, hop] fp32, frame_block rows per block"""
        b, r = divmod(i, self.frame_block)
        w = self._frame_w
        if any(t is not None and t.shape[1] != w for t in self._audio_blocks):
            self._audio_blocks = []
        while len(self._audio_blocks) <= b:
            self._audio_blocks.append(None)
        if self._audio_blocks[b] is None:
            self._audio_blocks[b] = self.engine.new(self.frame_block, w, self.engine.cfg.hop)
        return self._audio_blocks[b][r]

    def _release_frames(self):
        """the frame store holds one row per diffusion iteration of the call that just ended; its outputs have been copied out
        (torch.cat), so only the first block stays allocated for the next call"""
        self._audio_blocks = [t for t in self._audio_blocks if t is not None][:1]
        self._first_row = None

    # ------------------------------------------------------------------ one iteration of the hot loop over the active utterances
    def _iterate(self, S, act: List[_Utt]):
        """modeling_vibevoice_inference.py:466-672 for the utterances in `act`; returns the utterances still live."""
        run = [u for u in act if u.have_embeds]
        fresh = [u for u in act if not u.have_embeds]
        order = run + fresh
        nR = len(run)
        self._lm_pass(S, run, fresh)

        def hidden_of(i):                       # hidden state of order[i]'s positive row, [1, H]
            return self._hidden[i:i + 1] if i < nR else self._hid_fresh[order[i].slot:order[i].slot + 1]
        # ---- speculative sampling: a row that has just emitted <speech_diffusion>/<speech_start> almost always
        # emits <speech_diffusion> next.  The sampler (stateless: cond + noise -> latent) is enqueued behind the LM
        # pass BEFORE the host waits for the logits, so the token decision below overlaps GPU work instead of
        # leaving the GPU idle; if the guess is wrong the latent is discarded and the RNG state restored.
        # (the counter path: a discarded guess spends nothing, there is no state to restore)
        speculated = bool(run and not fresh and self.speculate_sampling
                          and (S.seeded or (not S.sde      # a discarded guess would spend device-RNG draws
                                            and not (S.do_sample and S.noise_fn is None and S.forced is None)))   # keep the reference's RNG draw order
                          and all(u.last in (S.diff_id, S.start_id) for u in run))
        # all active rows diffusing, in order: cond rows == [hidden[:nR]; hidden[nR:2nR]]
        rng_state = self._sample(S, run, self._hidden, undoable=True) if speculated else None
        logits = self._await_logits(S, order, hidden_of)
        self._choose_tokens(S, order, logits, hidden_of)
        self._retire(S, order)
        # ---------------- next input embeddings (:569) ----------------
        live = [u for u in order if not u.finished]
        diff = [u for u in live if u.last == S.diff_id]
        plain = [u for u in live if u.last != S.diff_id]
        if plain:
            self._embed_ids([u.last for u in plain], self._tmp_emb)
            for i, u in enumerate(plain):
                self._nxt_x[live.index(u)].copy_(self._tmp_emb[i])      # rows re-packed to the next step's active order
        if speculated and diff != order:
            speculated = False                                   # wrong guess: drop the latent, undo the draw
            if rng_state is not None:
                (S.cpu_gen.set_state if S.cpu_gen is not None else torch.set_rng_state)(rng_state)
        if S.lockstep and len(order) > 1:
            self._negative_bookkeeping(S, order, live, diff)
        if not S.refresh_negative and not diff:
            # the entry the negative pass appended at this step stays for a live row that does not diffuse, unless some row of the
            # batch does: then the reference's correction of :590-624 shifts it back out (pinned by generate_norefresh_b2.npz)
            for u in plain:
                u.neg_len += 1
        if diff and speculated:
            for u in diff:
                u.neg_len += 1
        elif diff:
            self._negative_conditions(S, order, diff, nR, hidden_of)
            self._sample(S, diff, self._cond)
        direct = False
        if diff:
            self._tokenizer_chain(S, diff)
            direct = self._emit_frames(S, live, diff, self._hidden if speculated else self._cond)
        if live:
            self._next_inputs(S, live, direct)
        for u in order:
            u.step += 1
        for u in live:
            u.have_embeds = True
        return live

    def _lm_pass(self, S, run, fresh):
        """The positive (+ speculative negative) LM pass over `run`, the valid-id logits of every row (`fresh` rows from their prompt's
        last hidden state), their copy to the host with its event, and -- refresh_negative=False -- the step-0 negative rows."""
        e, nv, nR = self.engine, S.nv, len(run)
        if run:
            rows = [(2 * u.slot, u.pos_len) for u in run] + [(2 * u.slot + 1, u.neg_len) for u in run]
            self._x_in[nR:2 * nR].copy_(self._x_in[:nR])
            e.lm_forward(rows, self._x_in, self._hidden)
            for u in run:
                u.pos_len += 1
            e.lm_logits(nR, self._hidden, self._logits)
        if fresh:
            if not run and [u.slot for u in fresh] == list(range(len(fresh))):
                e.lm_logits(len(fresh), self._hid_fresh, self._logits)
            else:
                for i, u in enumerate(fresh):
                    e.lm_logits(1, self._hid_fresh[u.slot:u.slot + 1], self._logits[(nR + i) * nv:])
        self._logits_pin.copy_(self._logits, non_blocking=True)      # whole (contiguous) buffer: a true async D2H
        self._lg_event.record(e.stream)
        if not S.refresh_negative:
            # refresh_negative=False (:503-516): the negative pass runs at EVERY step for every row on the input the positive pass
            # consumed -- the speculative rows above for `run`; at step 0 (inputs_embeds still None, :395) the lone <speech_start>
            # prompt token
            for i, u in enumerate(fresh):
                e.lm_forward([(2 * u.slot + 1, u.neg_len)], self._start_emb, self._neg_hidden[i:i + 1])

    def _sample(self, S, utts, cond, *, undoable=False):
        """Diffusion sampling (:697-710) of `utts` from the condition rows cond[:2n] into self._latent[:n]: the start noise (a hook's,
        the counter path's, or torch.randn on the CPU generator, as the reference, :701), the guidance scales, the solver.
        undoable: returns the state of the generator the draw came from, taken before the draw (None when nothing was drawn from one)
        -- on the session's OWN generator when it has one (a lane of generate_interleaved): rewinding the process-global generator from
        one lane would hand another lane draws it has already consumed."""
        e, n = self.engine, len(utts)
        nz = rng_state = None
        if any(u.noise_fn is not None for u in utts):         # explicit noise (test / bench hooks), per utterance or per call
            rows = [u.noise_fn(u.step, 2)[:1].to(torch.float32) for u in utts]
            nz = torch.cat(rows + rows)
        elif S.noise_fn is not None:
            nz = S.noise_fn(S.step, 2 * n)
        if nz is None and S.seeded:
            self._seeded_noise(utts)
        else:
            if nz is None:
                if undoable:
                    rng_state = S.cpu_gen.get_state() if S.cpu_gen is not None else torch.get_rng_state()
                nz = torch.randn(2 * n, e.cfg.latent_dim, generator=S.cpu_gen)
            self._stage_noise(nz, n)
        cfg_scale = self._cfg_arg(S, utts)
        sde = {"step_noise": self._sde_draws(S, n, utts)} if S.sde else {}
        e.diffusion_sample(n, cond, self._noise, cfg_scale, self._latent, **sde)
        return rng_state

    def _await_logits(self, S, order, hidden_of):
        """wait for the step's logits on the host -> [rows, n_valid] (a copy); the trace's positive hidden states and scores"""
        nA, nv = len(order), S.nv
        self._lg_event.synchronize()
        logits = self._logits_pin[:nA * nv].view(nA, nv).clone()
        if S.trace is not None:
            S.trace.pos_hidden.append(torch.cat([hidden_of(i) for i in range(nA)]).cpu())
            if hasattr(S.trace, "logits"):
                S.trace.logits.append(logits.clone())             # [rows, n_valid]: the scores the token decision is taken from
        return logits

    def _valid_scores(self, S, order, hidden_of, plain):
        """[n, n_valid] scores of the rows' valid ids the token is drawn from: `plain` (the LM's own, on the host or the device, as the
        caller holds them) over the temperature, or -- full-vocabulary processors -- what survives of the valid ids after them and the
        constraint (-inf where a filter removed one), from the kernel or from the torch ops.  A row that loses ALL its valid ids has
        NaN probabilities in the reference too -- torch.multinomial raises there; here the one place that says why."""
        if S.warp is None:
            return plain / S.temperature
        hidden = torch.cat([hidden_of(i) for i in range(len(order))])
        if self.warp_on_device and hasattr(self.engine, "lm_warp_valid"):
            lg = self._warp_valid_scores(hidden, order, S)
            alive = int(self._warp_surv[:len(order)].min()) >= 1
        else:
            lg = self._full_vocab_scores(hidden, order, S)[:, S.valid_t.to(self.device)]
            alive = bool(torch.isfinite(lg).any(dim=-1).all())
        if not alive:
            raise RuntimeError(_NO_VALID_TOKEN_LEFT)
        return lg

    def _choose_tokens(self, S, order, logits, hidden_of):
        """token selection (:488-501): u.last and u.tokens of every row of `order`; logits: the host copy of their valid-id scores"""
        e, valid_t = self.engine, S.valid_t
        nA, nv = len(order), S.nv
        if S.forced is not None or any(u.forced is not None for u in order):
            for u in order:
                f = u.forced if u.forced is not None else S.forced[u.idx]
                u.last = int(f[u.step]) if u.step < len(f) else S.eos_id
        elif S.seeded and S.do_sample:
            # the counter path: one uniform per (request, token index) and the inverse CDF of the float64 softmax over the row's
            # valid-id scores, per row on the host -- no [rows, lm_vocab] tensor, no generator; finished rows draw nothing
            lg = self._valid_scores(S, order, hidden_of, logits).cpu().numpy()
            for i, u in enumerate(order):
                u.last = int(valid_t[_noise.choose(lg[i], _noise.uniform(u.seed, len(u.tokens)))])
        elif S.do_sample or S.warp is not None:
            # the reference samples torch.multinomial(softmax(scores)) over the FULL vocabulary rows of the WHOLE batch (-inf
            # outside the valid ids, :490-496; finished rows included, their draw is overwritten by eos, :499) on the model's
            # device.  One-sample multinomial spends one exponential variate per (row, category), so the same call on the
            # same-shaped tensor keeps a seeded run on the reference's RNG stream (pinned on CPU by generate_sampled_b1.npz)
            rows_of = S.sample_rows(order)               # batch mode: every batch row; continuous mode: one row per utterance
            full = torch.full((len(rows_of), e.cfg.lm_vocab), float("-inf"), device=self.device, dtype=torch.float32)
            vt = valid_t.to(self.device)
            full[:, vt] = 0.0                              # finished rows: any proper distribution, the draw is discarded
            lg = self._valid_scores(S, order, hidden_of, self._logits[:nA * nv].view(nA, nv).float())
            for i, u in enumerate(order):
                full[rows_of.index(u.idx), vt] = lg[i]
            if S.do_sample:
                pick_ids = torch.multinomial(torch.softmax(full, dim=-1), num_samples=1, generator=S.dev_gen).squeeze(1).cpu()
            else:
                pick_ids = torch.argmax(full, dim=-1).cpu()
            for u in order:
                u.last = int(pick_ids[rows_of.index(u.idx)])
        else:
            pick = torch.argmax(logits, dim=-1)
            for i, u in enumerate(order):
                u.last = int(valid_t[pick[i]])
        for u in order:
            u.tokens.append(u.last)
        if S.trace is not None:
            nxt = torch.full((S.n_rows,), S.eos_id, dtype=torch.long)
            for u in order:
                nxt[u.idx] = u.last
            S.trace.tokens.append(nxt)

    def _retire(self, S, order):
        """bookkeeping (:518-539): rows ended by <eos> or by their cap, and what a control token does to a row's engine state"""
        e, audio_streamer = self.engine, S.audio_streamer
        def end(rows, what, reach_max):
            for u in rows:
                u.finished, u.reach_max = True, reach_max
            if rows and S.verbose:
                print(f"Samples {sorted(u.idx for u in rows)} reached {what} at step {rows[0].step + 1}.", flush=True)
            if rows and audio_streamer is not None:
                audio_streamer.end(torch.tensor(sorted(u.idx for u in rows)))
        end([u for u in order if u.last == S.eos_id], "EOS token", False)
        end([u for u in order if not u.finished and u.step >= u.max_step_sample], "max generation length", True)
        for u in order:
            if u.finished:                            # the repetition-penalty mask of a finished utterance ([V] bools on the device)
                S._seen.pop(u.idx, None)
                S._seen_dev.pop(u.idx, None)
        for u in order:
            if u.last == S.end_id:
                e.codec_reset(u.slot)
            if S.refresh_negative and not u.finished and u.last == S.start_id:
                # :549-565 -- the reference masks the whole negative cache and un-masks only the slot of the NEXT token, so the
                # negative context restarts empty and the next negative pass re-feeds <speech_start> at position 0
                # (pinned against the reference's generate(): tests/golden/generate_forced_*.npz)
                u.neg_len = 0

    def _negative_conditions(self, S, order, diff, nR, hidden_of):
        """condition rows of the sampler call over `diff` -> self._cond: [positive hidden states; negative hidden states]"""
        e, n = self.engine, len(diff)
        for j, u in enumerate(diff):
            oi = order.index(u)
            self._cond[j].copy_(hidden_of(oi)[0])
            if u.have_embeds:
                self._cond[n + j].copy_(self._hidden[nR + oi])
            elif not S.refresh_negative:
                self._cond[n + j].copy_(self._neg_hidden[oi - nR])
            else:
                # first negative step of a fresh utterance: the lone <speech_start> prompt token (:379-386)
                e.lm_forward([(2 * u.slot + 1, u.neg_len)], self._start_emb, self._neg_hidden[j:j + 1])
                self._cond[n + j].copy_(self._neg_hidden[j])
            u.neg_len += 1

    def _tokenizer_chain(self, S, diff):
        """codec decode and semantic re-encode (:636-672) of self._latent[:n] -> self._audio[:n], self._sem[:n]"""
        e, n = self.engine, len(diff)
        started = [u for u in diff if u.chunks]
        if S.lockstep and started and len(started) < n:
            # The reference's VibeVoiceTokenizerStreamingCache.get (modular_vibevoice_tokenizer.py:198-207) answers "no history" for
            # EVERY row of a decode / encode call as soon as ONE of its rows has no entry yet: in a lock-step batch, a row that
            # diffuses for the first time costs the rows decoded with it their conv history for that frame (both tokenizers).  It
            # cannot fire on processor-built prompts (every row takes its first frame at step 0); pinned by
            # tests/golden/generate_late_start_b2*.npz.  A queue of independent requests (generate_continuous) keeps every row's own
            # history instead -- each request ends as generate() on it alone would.
            for u in started:
                e.codec_reset(u.slot)
        if self.batched_codecs:
            # the reference decodes / re-encodes the step's diffusion rows as one batch (:636-672): one engine call, the
            # weight-heavy tokenizer stages read their weights once for all rows; one utterance's chain too (one captured
            # sequence instead of two: a graph-to-graph transition costs ~7 us against ~1.5 us between two kernels of one graph)
            e.codec_chain_batch([u.slot for u in diff], self._latent[:n], self._audio[:n],
                                self._sem[:n] if e.cfg.sem_dim > 0 else None)
        elif len(diff) > 1 and self.concurrent_codecs and self._side_streams:
            # each utterance's tokenizer chain (decode -> semantic re-encode) is an independent, launch-latency
            # bound graph: fork them onto side streams so they overlap, join before the connectors
            self._fork_ev.record(e.stream)
            for j, u in enumerate(diff):
                ss = self._side_streams[j % len(self._side_streams)]
                ss.wait_event(self._fork_ev)
                e.codec_decode(u.slot, self._latent[j:j + 1], self._audio[j], stream=ss)
                if e.cfg.sem_dim > 0:
                    e.semantic_encode(u.slot, self._audio[j], self._sem[j], stream=ss)
            for ss in self._side_streams[:min(len(diff), len(self._side_streams))]:
                self._join_ev.record(ss)
                e.stream.wait_event(self._join_ev)
        else:
            for j, u in enumerate(diff):
                e.codec_decode(u.slot, self._latent[j:j + 1], self._audio[j])
                if e.cfg.sem_dim > 0:
                    e.semantic_encode(u.slot, self._audio[j], self._sem[j])

    def _emit_frames(self, S, live, diff, cond_used):
        """connectors (:636-672), the frame store, the streamer and the trace for the step's frames; -> True when the connectors wrote
        the next step's LM input rows in place"""
        e, n = self.engine, len(diff)
        # every live row diffuses, in order (the steady state of a speech segment): the connectors write the next step's LM input
        # rows in place -- no staging through _emb_out / _nxt_x, two device copies fewer on the step's dependency line
        direct = diff == live and S.teacher is None
        e.connect(n, self._latent, self._sem if e.cfg.sem_dim > 0 else None, self._x_in if direct else self._emb_out)
        chunk = self._block_rows(S.frame_rows)
        S.frame_rows += 1
        chunk[:n].copy_(self._audio[:n])
        for j, u in enumerate(diff):
            if self._first_row is not None and not u.chunks:
                self._first_row[id(u)] = S.frame_rows - 1
            u.chunks.append(chunk[j])
            if not direct:
                self._nxt_x[live.index(u)].copy_(self._emb_out[j])
        if S.audio_streamer is not None:
            S.audio_streamer.put(chunk[:n, None, :].to(self.dtype), torch.tensor([u.idx for u in diff]))
        S.n_frames += n
        trace = S.trace
        if trace is not None and hasattr(trace, "noise"):
            nz_host = self._noise[:n].cpu()                   # (request, t, start noise) of every ACCEPTED latent
            for j, u in enumerate(diff):
                trace.noise.append((u.idx, u.n_lat, nz_host[j].clone()))
        for u in diff:
            u.n_lat += 1
        if trace is not None:
            trace.neg_hidden.append(cond_used[n:2 * n].cpu())
            trace.latents.append(self._latent[:n].cpu())
            trace.semantic.append(self._sem[:n].cpu())
        return direct

    def _next_inputs(self, S, live, direct):
        """self._x_in[:len(live)] = the next step's LM input rows (already there when the connectors wrote them in place)"""
        if S.teacher is not None:
            # test hook (SURVEY 8d "teacher-forced per step"): the next step consumes the embeddings the oracle fed its LM at
            # this step, so a bf16-mode run is compared step by step without the autoregressive feedback compounding
            te = S.teacher(S.step, [u.idx for u in live])
            if te is not None:
                self._nxt_x[:len(live)].copy_(te.to(self.device, torch.float32))
        if not direct:
            self._x_in[:len(live)].copy_(self._nxt_x[:len(live)])
        if S.trace is not None:
            S.trace.next_embeds.append(self._x_in[:len(live)].cpu())

    def _negative_bookkeeping(self, S, order, live, diff):
        """The reference's array bookkeeping of the negative branch (oracle.generate.NegativeRow restates it with the tensors), masks
        and counters only.  Its correction of a non-diffusing row (:594-624) guards the mask shift and the K/V shift differently
        (:603 vs :613): for a row holding exactly one valid entry the mask moves and the K/V does not, so the reference KEEPS the entry
        appended at this step and masks the older one out.  Everywhere else the net effect is "this step's entry is dropped".  Needs a one-frame speech segment (or a non-diffusion token
        at step 1 with refresh_negative=False) in one row of a batch while another row diffuses; found by
        tools/fuzz_generate_vs_reference.py.  Followed with vv_kv_move: the entry of this step is moved onto the older one."""
        def fwd():
            for u in order:
                b = u.neg_book
                b[1] += 1
                b[0].append(1)
        refresh = S.refresh_negative
        if not refresh:
            fwd()
        else:
            for u in live:
                if u.last == S.start_id:
                    u.neg_book[0] = [0] * (len(u.neg_book[0]) - 1) + [1]
        if not diff:
            return
        if refresh:
            fwd()
        for u in live:
            if u in diff:
                continue
            mask, c, cnt = u.neg_book
            if c - cnt == 2 and mask[cnt] == 1:
                # the row's one valid entry sits at compact position 0, this step's entry (written by the speculative negative row of
                # the LM pass above) at position 1: the reference keeps the NEW one.  Position 1 -> 0 with its rotation, length stays 1
                assert u.neg_len == 1, (u.idx, u.neg_len)
                self.engine.kv_move(2 * u.slot + 1, 1, 0)
            if cnt + 1 < len(mask) - 1:
                mask[cnt + 1:] = mask[cnt:-1]
            mask[cnt] = 0
            u.neg_book[2] = cnt + 1

    def _seeded_noise(self, utts):
        """start noise of one sampler call over seeded utterances -> self._noise[:n]: row j is stream 0 of utts[j]'s seed at t = the
        latents it has accepted (noise.py).  One vv_noise_rows launch: no host draw, no staging copy."""
        e = self.engine
        L = e.cfg.latent_dim
        if hasattr(e, "noise_rows") and L % 4 == 0:
            e.noise_rows([(u.seed, u.n_lat, 0) for u in utts], _noise.STREAM_START, 1, 1, L, self._noise)
        else:
            for j, u in enumerate(utts):
                self._noise[j].copy_(_noise.normals(u.seed, u.n_lat, 1, _noise.STREAM_START, 1, 0, L)[0, 0])

    def _sde_draws(self, S, n, utts=None):
        """The variance noise of one frame's solver steps, [N, n, latent] fp32 on the device.  scheduler.step() draws
        randn(model_output.shape = [2n, latent], device=model_output.device, float32) once per solver step on the device's
        global generator (dpm_solver.py:994-997; generate() passes no generator); only the first n rows survive the next step's
        `speech[:n]` (modeling_vibevoice_inference.py:703-704).  Same calls, same order -> same stream for a seeded run."""
        e = self.engine
        N, L = S.solver_steps or self.ddpm_inference_steps, e.cfg.latent_dim
        if self._sde_flat is None:
            self._sde_flat = e.new(64 * MAX_BATCH * L)
        buf = self._sde_flat[:N * n * L].view(N, n, L)
        if S.sde_noise_fn is not None:                        # test hook: the recorded draws, [N, 2n, latent]
            buf.copy_(S.sde_noise_fn(S.step, N, 2 * n)[:, :n].to(buf.device, torch.float32))
            return buf
        if S.seeded:                                          # the counter path: streams 1 .. N of every row's seed, at its own t
            if hasattr(e, "noise_rows") and L % 4 == 0:
                e.noise_rows([(u.seed, u.n_lat, 0) for u in utts], _noise.STREAM_START + 1, N, 1, L, buf)
            else:
                for j, u in enumerate(utts):
                    buf[:, j].copy_(_noise.normals(u.seed, u.n_lat, 1, _noise.STREAM_START + 1, N, 0, L)[:, 0])
            return buf
        for i in range(N):
            buf[i].copy_(torch.randn(2 * n, L, device=self.device, dtype=torch.float32, generator=S.dev_gen)[:n])
        return buf

    def _session(self, tokenizer, generation_config, cfg_scales, kwargs, audio_streamer, n_rows, *, seeds, sample_rows, lockstep=True):
        """cfg_scales: the validated guidance scale of every utterance of the call (_cfg_scale_values); seeds: the requests' seeds as
        given (ints or None, _resolve_seeds settles them on the session's CPU generator)"""
        e = self.engine
        if tokenizer is None:
            raise ValueError("generate() needs tokenizer= (speech_start_id / speech_end_id / speech_diffusion_id / eos_token_id)")
        do_sample, temperature, warp = self._generation_options(generation_config)
        start_id, end_id, diff_id = tokenizer.speech_start_id, tokenizer.speech_end_id, tokenizer.speech_diffusion_id
        eos_id = tokenizer.eos_token_id
        bos_id = getattr(tokenizer, "bos_token_id", None)
        valid = [start_id, end_id, diff_id, eos_id] + ([bos_id] if bos_id is not None else [])
        if self._valid_key != tuple(valid):
            e.set_valid_tokens(valid)
            self._valid_key = tuple(valid)
        algo = self._sched_cfg["algorithm_type"]
        # a shipped configuration is installed as before (engines and stand-ins that predate the general table take no solver=);
        # any other one passes its non-default sampling-time settings, and the engine routes diffusion_sample by the installed table
        general = not _schedule.is_shipped(self._sched_cfg)
        solver = {k: self._sched_cfg[k] for k, v in _schedule.SHIPPED.items() if self._sched_cfg[k] != v} if general else None
        e.set_num_steps(self.ddpm_inference_steps, t_cast_bf16=(self.dtype == torch.bfloat16 and kwargs.get("_t_cast", True)),
                        **({} if algo == "dpmsolver++" else {"algorithm_type": algo}), **({"solver": solver} if general else {}))
        solver_steps = len(_schedule.general_timesteps_and_sigmas(self._sched_cfg, self.ddpm_inference_steps)[0]) if general else 0
        cpu_gen, dev_gen = kwargs.pop("_generators", None) or (None, None)
        return _Session(sde=(algo == "sde-dpmsolver++"), solver_steps=solver_steps, sde_noise_fn=kwargs.pop("_sde_noise_fn", None), nv=len(valid),
                        valid_t=torch.tensor(valid, dtype=torch.long), start_id=start_id, end_id=end_id, diff_id=diff_id, eos_id=eos_id,
                        pad_id=getattr(tokenizer, "pad_token_id", None), cfg_scale=cfg_scales[0] if cfg_scales else 1.0,
                        cfg_rows=len(set(cfg_scales)) > 1, do_sample=do_sample, temperature=temperature, warp=warp,
                        trace=kwargs.pop("_trace", None), audio_streamer=audio_streamer, verbose=kwargs.get("verbose", False),
                        forced=kwargs.pop("_forced_tokens", None), noise_fn=kwargs.pop("_noise_fn", None),
                        teacher=kwargs.pop("_teacher_embeds", None), n_rows=n_rows, refresh_negative=bool(kwargs.get("refresh_negative", True)),
                        lockstep=lockstep, sample_rows=sample_rows, seeds=_resolve_seeds(seeds, cpu_gen), cpu_gen=cpu_gen, dev_gen=dev_gen)

    # ------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, inputs=None, generation_config=None, logits_processor=None, stopping_criteria=None,
                 prefix_allowed_tokens_fn=None, synced_gpus=None, assistant_model=None, audio_streamer=None,
                 negative_prompt_ids=None, negative_prompt_attention_mask=None, speech_tensors=None,
                 speech_masks=None, speech_input_mask=None, is_prefill=True, return_speech=True,
                 cfg_scale=1.0, stop_check_fn: Optional[Callable[[], bool]] = None, tqdm_class=None, **kwargs):
        """logits_processor / stopping_criteria are accepted and unused, as in the reference (its generate() overwrites the
        arguments with the lists it builds itself, :375-377).
        seed (keyword): an int for a one-row call, or a list with one int or None per row.  With at least one seed the call runs the
        counter path (vibevoice_amd/noise.py): every draw of a row -- solver noise, token choice, voice latents -- is a function of
        the row's seed and its own counters, whatever it shares the batch or the queue with; rows without a seed get one from ONE
        torch.randint on the CPU generator.  No seed: the torch generators, as the reference, draw for draw."""
        e = self.engine
        tokenizer = kwargs.pop("tokenizer", None)
        seeds_in = _seed_values(kwargs.pop("seed", None), (kwargs["input_ids"] if inputs is None else inputs).shape[0], "generate()")
        kwargs.pop("parsed_scripts", None)
        kwargs.pop("all_speakers_list", None)
        max_length_times = kwargs.pop("max_length_times", 2)
        prefill_noise = kwargs.pop("_prefill_noise", None)
        prompt_prefix = kwargs.pop("prompt_prefix", None)      # PromptPrefix (every row) or a list with one entry / None per row
        hooks = kwargs.pop("_bench_hooks", None) or BenchHooks()  # measurement harness only (bench.py): see BenchHooks
        step_cb, kv_start, kv_fill_fn = hooks.step_callback, hooks.kv_start, hooks.kv_fill_fn
        input_ids = kwargs["input_ids"] if inputs is None else inputs
        attention_mask = kwargs.get("attention_mask")
        input_ids = input_ids.cpu()
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        attention_mask = attention_mask.cpu()
        B, L0 = input_ids.shape
        cfg_scales = _cfg_scale_values(cfg_scale, B, "generate()")      # a float, or one guidance scale per row
        if B > MAX_BATCH or B > e.cfg.n_slots or 2 * B > e.cfg.max_rows:
            # the reference's batch is unbounded (:393-394); one engine pass carries MAX_BATCH utterances (and this engine was created with
            # n_slots / max_rows), so a larger batch is decoded through the continuous-admission queue and handed back in the batch's own
            # output form
            return self._generate_queued(input_ids, attention_mask, tokenizer, generation_config, cfg_scales, audio_streamer,
                                         speech_tensors, speech_masks, speech_input_mask, is_prefill, return_speech, stop_check_fn,
                                         max_length_times, prefill_noise, step_cb, kwargs, prompt_prefix=prompt_prefix, seeds=seeds_in)
        prefixes = self._prefix_list(prompt_prefix, B)
        pf_stats = {"prefix_rows_reused": 0, "prompt_rows_computed": 0}
        S = self._session(tokenizer, generation_config, cfg_scales, kwargs, audio_streamer, B, seeds=seeds_in,
                          sample_rows=lambda order: list(range(B)))
        self._frame_w = B                                 # frame-store rows are as wide as this call's batch
        max_new_tokens = kwargs["max_new_tokens"] if kwargs.get("max_new_tokens") is not None else self.max_position_embeddings - L0
        max_length = min(L0 + max_new_tokens, e.max_ctx)
        utts = []
        for b in range(B):
            m = attention_mask[b].bool()
            utts.append(_Utt(b, b, input_ids[b][m].tolist(), L0, max_length, max_length_times, S.start_id))
            utts[-1].cfg_scale = cfg_scales[b]
            if S.seeded:
                utts[-1].seed = S.seeds[b]
        max_steps = min(max_length - L0, int(max_length_times * L0))
        if tqdm_class is not None and kwargs.get("show_progress_bar", True):
            progress = tqdm_class(range(max_steps), desc="Generating", leave=False)
        else:
            progress = range(max_steps)
        n_steps = 0
        with torch.cuda.stream(e.stream), _end_streamer_on_error(audio_streamer):
            for b in range(B):
                e.codec_reset(b)
            e.embed([S.start_id], self._start_emb)
            active = list(utts)
            for step in progress:
                S.step = step
                if step_cb is not None:
                    step_cb(step)
                if stop_check_fn is not None and stop_check_fn():
                    if audio_streamer is not None:
                        audio_streamer.end()
                    break
                if audio_streamer is not None and hasattr(audio_streamer, "finished_flags") and any(audio_streamer.finished_flags):
                    break
                if not active:
                    break
                if L0 + step >= max_length:
                    for u in active:
                        u.reach_max = True
                    break
                if step == 0:
                    pf_stats = self._prefill_batch(S, utts, prefixes, attention_mask, speech_input_mask,
                                                   (speech_tensors, speech_masks) if is_prefill else (None, None), prefill_noise,
                                                   kv_start, kv_fill_fn)
                active = self._iterate(S, active)
                n_steps += 1
            if audio_streamer is not None:
                audio_streamer.end()
            out = self._output(utts, input_ids, n_steps, S.eos_id, return_speech)
        e.sync()
        self._release_frames()
        self.last_stats = {"frames": S.n_frames, "steps": n_steps, **pf_stats}
        return out

    def _prefill_batch(self, S, utts, prefixes, attention_mask, speech_input_mask, voice, prefill_noise, kv_start, kv_fill_fn):
        """prompt prefill (:467-474, _process_speech_inputs) of a generate() batch: the voice samples `voice` = (speech_tensors,
        speech_masks) encoded and scattered into the rows' speech positions, the rows that start with a prompt prefix restored from it;
        -> the call's prefix_rows_reused / prompt_rows_computed"""
        e = self.engine
        speech_tensors, speech_masks = voice
        time_prefill = os.environ.get("VVHIP_TIME_PREFILL") is not None     # debug: sync + time the two prefill phases
        sp_embeds = None
        t_pf = [time.perf_counter()] if time_prefill else None
        self._t_kv_fill = self._t_lm_pass = 0.0
        with_voice = speech_tensors is not None and speech_masks is not None
        # masks are host data (the processor's output): positions and counts on the host (a device-side .sum() costs a
        # lazy kernel-module load (~20 ms) on its first use and a sync on every use), uploaded while the stream is
        # still idle -- behind the encoder a pageable copy would hold the host until the encoder has finished
        sp_pos, sp_host = {}, {}
        if speech_input_mask is not None and (with_voice or any(p is not None for p in prefixes)):
            for u in utts:
                idx = _speech_positions(speech_input_mask[u.idx], attention_mask[u.idx])
                sp_host[u.idx] = idx.tolist()
                if with_voice and idx.numel():
                    sp_pos[u.idx] = (int(idx.numel()), idx.to(self.device))
        # rows that start with a prompt prefix: r leading positions come from its snapshot (0: today's full prefill)
        reuse = {u.idx: self._prefix_plan(prefixes[u.idx], u.ids, sp_host.get(u.idx)) for u in utts}
        seeded_voice = with_voice and S.seeded and prefill_noise is None
        spk = spk_seeds = None
        if seeded_voice or (with_voice and any(reuse.values())):
            # the voice samples every row consumes (None: a sample spans two rows)
            spk = _speakers_of_rows([sp_pos[u.idx][0] if u.idx in sp_pos else 0 for u in utts],
                                    [int(speech_masks[i].sum()) for i in range(speech_masks.shape[0])])
        if seeded_voice:
            # every voice sample draws from the seed of the row it belongs to, under its index within that row
            if spk is None:
                raise ValueError("generate(seed=...): a voice sample spans two batch rows; with seeds the rows' speech "
                                 "positions must consume whole voice samples")
            spk_seeds = [None] * speech_masks.shape[0]
            for u in utts:
                for k, i in enumerate(spk[u.idx]):
                    spk_seeds[i] = (u.seed, k)
            for i in range(len(spk_seeds)):          # samples no row consumes: their latents are never read
                if spk_seeds[i] is None:
                    spk_seeds[i] = (utts[-1].seed, i)
        if with_voice and any(reuse.values()) and spk is not None:
            # the voice samples of a prefixed row are in the prefix: only the other rows' samples are encoded (none: no
            # encoder call at all).  A sample that spans two rows cannot be told apart: then every sample is encoded.
            keep_spk = [i for u in utts if not reuse[u.idx] for i in spk[u.idx]]
            for u in utts:
                if reuse[u.idx]:
                    sp_pos.pop(u.idx, None)
            if keep_spk:
                sel = torch.tensor(keep_spk, dtype=torch.long)
                speech_tensors, speech_masks = speech_tensors.cpu()[sel], speech_masks.cpu()[sel]
                if prefill_noise is not None:
                    prefill_noise = tuple(t.cpu()[sel] for t in prefill_noise)
                if spk_seeds is not None:
                    spk_seeds = [spk_seeds[i] for i in keep_spk]
            else:
                with_voice = False
        if with_voice:
            _, sp_embeds = self._process_speech_inputs(speech_tensors, speech_masks, prefill_noise, seeds=spk_seeds)
        if time_prefill:
            e.sync(); torch.cuda.current_stream(self.device).synchronize(); t_pf.append(time.perf_counter())
        sp_off = 0
        jobs = []
        for u in utts:
            rows = pos = None
            if sp_embeds is not None and u.idx in sp_pos:
                cnt, pos = sp_pos[u.idx]
                rows = sp_embeds[sp_off:sp_off + cnt]
                sp_off += cnt
            jobs.append((u, u.ids, rows, pos, kv_start, kv_fill_fn, prefixes[u.idx] if reuse[u.idx] else None, reuse[u.idx]))
        self._prefill_checked(jobs)
        if time_prefill:
            e.sync(); t_pf.append(time.perf_counter())
            self.last_prefill = {"voice_encode_s": round(t_pf[1] - t_pf[0], 5),
                                 "lm_prefill_s": round(t_pf[2] - t_pf[1] - self._t_kv_fill, 5),
                                 "lm_passes_s": round(self._t_lm_pass, 5),      # the LM launches alone (the rest of
                                 "bench_kv_fill_s": round(self._t_kv_fill, 5)}  # lm_prefill_s: embedding + row scatter)
        return {"prefix_rows_reused": sum(reuse.values()), "prompt_rows_computed": sum(len(u.ids) - reuse[u.idx] for u in utts)}

    def _output(self, utts, input_ids, n_new, eos_id, return_speech):
        """utterances -> VibeVoiceGenerationOutput (:691-695): row b = input_ids[b] + utts[b]'s tokens, padded with eos to n_new new
        columns (:499); one waveform (or None) per row"""
        B, L0 = input_ids.shape
        seq = torch.full((B, L0 + n_new), eos_id, dtype=torch.long)
        seq[:, :L0] = input_ids
        for b, u in enumerate(utts):
            if u.tokens:
                seq[b, L0:L0 + len(u.tokens)] = torch.tensor(u.tokens, dtype=torch.long)
        outs = [torch.cat(u.chunks, dim=-1)[None].to(self.dtype) if u.chunks else None for u in utts]
        return VibeVoiceGenerationOutput(
            sequences=seq.to(self.device), speech_outputs=outs if return_speech else None,
            reach_max_step_sample=torch.tensor([u.reach_max for u in utts], dtype=torch.bool).to(self.device))

    def _generate_queued(self, input_ids, attention_mask, tokenizer, generation_config, cfg_scales, audio_streamer, speech_tensors,
                         speech_masks, speech_input_mask, is_prefill, return_speech, stop_check_fn, max_length_times, prefill_noise,
                         step_cb, kwargs, prompt_prefix=None, seeds=None):
        """generate() for a batch of more than MAX_BATCH rows (the reference's batch is unbounded, :393-394): every row becomes a
        one-utterance request of generate_continuous() -- up to n_slots of them in flight, a finished row's slot refilled at once --
        and the results are assembled into ONE VibeVoiceGenerationOutput as the batched loop returns it (sequences [B, L0 + steps]
        padded with eos after a row's end, :499; speech_outputs one entry per row; reach_max_step_sample [B]).  Rows are
        independent in the reference's loop (no cross-sample arithmetic, :393-394,549,573,594) with ONE exception this path does not
        reproduce: a row whose first frame comes later than another's costs the rows decoded with it their tokenizer conv history
        for that frame (the cache quirk described in _tokenizer_chain; impossible on processor-built prompts, where every row takes its first
        frame at step 0) -- and one consequence of the queue itself: the batch-level early exit with an audio_streamer (the loop ends when
        ANY stream has finished, :443-447) can fire while rows are still waiting for a slot; those rows return as their prompt without
        audio (the lock-step batch would have advanced them to that step) and a RuntimeWarning says so.
        So under greedy / forced decoding each row is exactly what the batched call gives it; RNG-dependent draws (diffusion noise, do_sample) are consumed in queue
        order instead of the batch's lock-step order.  Loop lengths follow the batch: every row's cap uses the batch's padded
        width L0 (:421-422)."""
        B, L0 = input_ids.shape
        prefixes = self._prefix_list(prompt_prefix, B)
        if prefill_noise is not None:
            raise NotImplementedError("_prefill_noise (test hook) is per call; not supported for batches above MAX_BATCH")
        forced = kwargs.pop("_forced_tokens", None)
        noise_fn = kwargs.pop("_noise_fn", None)
        global _WARNED_QUEUED_RNG
        all_seeded = seeds is not None and all(v is not None for v in seeds)      # every draw is the row's own: nothing follows the queue
        if not _WARNED_QUEUED_RNG and not all_seeded and (noise_fn is None or self._generation_options(generation_config)[0]):
            _WARNED_QUEUED_RNG = True
            warnings.warn(f"generate(): a batch of {B} rows exceeds one engine pass ({min(MAX_BATCH, self.engine.cfg.n_slots, self.engine.cfg.max_rows // 2)} "
                          "utterances) and is decoded through the continuous-admission queue: every row is what generate() gives it alone, but "
                          "random draws (diffusion noise, do_sample) are consumed in queue order, not in the lock-step batch's order -- a seeded "
                          "run does not reproduce the reference's batch bit for bit", UserWarning, stacklevel=3)
        # voice-prompt rows: speaker i of speech_tensors contributes speech_masks[i].sum() frames; the rows' speech positions
        # consume those frames in row-major order (_process_speech_inputs + the masked scatter, :149-163,470-474)
        spk_of_row = [[] for _ in range(B)]
        if is_prefill and speech_tensors is not None and speech_masks is not None and speech_input_mask is not None:
            need = [int((speech_input_mask[b].cpu() & attention_mask[b].bool()).sum()) for b in range(B)]
            have = [int(speech_masks[i].sum()) for i in range(speech_masks.shape[0])]
            if sum(have) < sum(need):
                raise ValueError("speech_masks hold fewer frames than speech_input_mask marks")
            spk_of_row = _speakers_of_rows(need, have)
            if spk_of_row is None:
                raise ValueError("a voice prompt spans two batch rows: the rows' speech positions must consume whole speakers")
        reqs = []
        for b in range(B):
            r = {"input_ids": input_ids[b:b + 1], "attention_mask": attention_mask[b:b + 1]}
            if spk_of_row[b]:
                idx = torch.tensor(spk_of_row[b], dtype=torch.long)
                r["speech_tensors"] = speech_tensors[idx]
                r["speech_masks"] = speech_masks[idx]
                r["speech_input_mask"] = speech_input_mask[b:b + 1]
            elif prefixes[b] is not None and speech_input_mask is not None:
                r["speech_input_mask"] = speech_input_mask[b:b + 1]
            if prefixes[b] is not None:
                r["prompt_prefix"] = prefixes[b]
            if forced is not None:
                r["_forced_tokens"] = forced[b]
            if noise_fn is not None:
                r["_noise_fn"] = noise_fn                # per utterance here: noise_fn(its own step, 2) -> [2, latent]
            r["cfg_scale"] = cfg_scales[b]               # the row's own guidance scale (all equal when generate() got a float)
            if seeds is not None and seeds[b] is not None:
                r["seed"] = seeds[b]
            reqs.append(r)
        kw = {k: v for k, v in kwargs.items() if k in ("verbose", "refresh_negative", "_trace", "_teacher_embeds", "_t_cast", "_sde_noise_fn")}
        outs = self.generate_continuous(reqs, tokenizer=tokenizer, generation_config=generation_config, cfg_scale=cfg_scales[0],
                                        audio_streamer=audio_streamer, is_prefill=is_prefill, return_speech=return_speech,
                                        max_new_tokens=kwargs.get("max_new_tokens"), max_length_times=max_length_times,
                                        stop_check_fn=stop_check_fn, _bench_hooks=BenchHooks(step_callback=step_cb), _batch_exit=True, **kw)
        eos = tokenizer.eos_token_id
        width = max(int(o.sequences.shape[1]) for o in outs)
        seq = torch.full((B, width), eos, dtype=torch.long, device=self.device)
        for b, o in enumerate(outs):
            seq[b, :o.sequences.shape[1]] = o.sequences[0]
        speech = [o.speech_outputs[0] if o.speech_outputs else None for o in outs] if return_speech else None
        return VibeVoiceGenerationOutput(sequences=seq, speech_outputs=speech,
                                         reach_max_step_sample=torch.cat([o.reach_max_step_sample.reshape(1) for o in outs]).to(self.device))

    # ------------------------------------------------------------------ two decode chains over one weight copy
    def fork(self, **runtime):
        """A second model object over THIS model's weights (Engine.fork -> vv_create_shared: one copy in HBM) with its own engine
        context -- KV caches, tokenizer state, graphs, stream -- and its own host-side buffers.  runtime: n_slots / max_ctx / max_rows
        overrides.  generate() on the fork and on the original may run at the same time from two host threads."""
        m = type(self)(self.config_dict, self.engine.fork(**runtime), self.dtype, self.requested_attn_implementation)
        m._epoch_box = self._epoch_box          # one weight copy, one epoch: a prefix built on either model serves both
        m.set_speech_factors(self._scaling, self._bias)
        m.set_ddpm_inference_steps(self.ddpm_inference_steps)
        m._sched_cfg = dict(self._sched_cfg)
        m.concurrent_codecs, m.batched_codecs, m.speculate_sampling = self.concurrent_codecs, self.batched_codecs, self.speculate_sampling
        m.warp_on_device = self.warp_on_device
        return m

    def generate_interleaved(self, requests: List[dict], lanes: int = 2, audio_streamer=None, **kwargs) -> List[VibeVoiceGenerationOutput]:
        """generate_continuous() over `lanes` engine contexts that share this model's weights, one host thread and one stream per lane.
        A decode step is a chain of ~300-450 DEPENDENT launches, each paying a fixed boundary cost the chip idles through; a second,
        independent chain fills those boundaries (measured with two processes on one GPU in round 4: 1.63 x the aggregate at 1.5B).
        The queue is split longest-prompt-first over the lanes (parallel.shard_utterances); with greedy / forced decoding and explicit
        noise every request ends exactly as generate() on it alone (the lanes share nothing but read-only weights).  Random draws:
        every lane owns a CPU and a device torch.Generator seeded from the process-global CPU generator when the call starts, so a
        seeded call is reproducible and no lane consumes (or, undoing a speculative draw, rewinds) another lane's stream -- but the
        noise a request sees is its lane's, not what the same request would draw on the global generators through generate().  Requests
        with a "seed" key (generate_continuous) draw from their own counters instead: the lane generators are not used for them and the
        lane a request lands in does not matter.  Returns the outputs in request order.  The lanes are
        created on first use (each owns KV caches for its n_slots) and kept: `model.close_lanes()` releases them."""
        from .parallel import shard_utterances
        _request_cfg_scales(requests, kwargs.get("cfg_scale", 1.0), "generate_interleaved()")      # refused here, before any lane starts
        seeds = _request_seeds(requests, "generate_interleaved()")
        lanes = max(1, min(int(lanes), len(requests)))
        if lanes == 1:
            return self.generate_continuous(requests, audio_streamer=audio_streamer, **kwargs)
        # seeds are settled here, on the caller's thread (a request without one in a call that has some: one randint on the
        # process-global CPU generator, in request order), so which lane a request lands in does not matter
        seeds = _resolve_seeds(seeds)
        if seeds is not None:
            requests = [dict(r, seed=sd) for r, sd in zip(requests, seeds)]
        while len(self._lanes) < lanes - 1:
            self._lanes.append(self.fork())
        models = [self] + self._lanes[:lanes - 1]
        shards = shard_utterances([int(r["input_ids"].shape[-1]) for r in requests], lanes)
        outs: List[Optional[VibeVoiceGenerationOutput]] = [None] * len(requests)
        errs: List[Optional[BaseException]] = [None] * lanes
        # every lane draws from its OWN generators (diffusion noise and the speculative draw's rewind on the CPU one; voice-prompt
        # sampling, multinomial and the sde variance noise on the device one), seeded here, on the caller's thread, from the
        # process-global CPU generator: a seeded call (torch.manual_seed) is reproducible, no lane can rewind or consume another
        # lane's draws, and the global device generator is not touched from the lane threads
        lane_seeds = torch.randint(0, 2 ** 62, (lanes, 2), dtype=torch.int64).tolist()
        gens = []
        for k in range(lanes):
            cg = torch.Generator()
            cg.manual_seed(lane_seeds[k][0])
            dg = torch.Generator(device=self.device)
            dg.manual_seed(lane_seeds[k][1])
            gens.append((cg, dg))

        def run(k):
            try:
                torch.cuda.set_device(self.device)
                st = _LaneStreamer(audio_streamer, shards[k]) if audio_streamer is not None else None
                res = models[k].generate_continuous([requests[i] for i in shards[k]], audio_streamer=st, _generators=gens[k], **kwargs)
                for i, o in zip(shards[k], res):
                    outs[i] = o
            except BaseException as ex:                 # noqa: BLE001 -- handed to the caller's thread below
                errs[k] = ex
        threads = [threading.Thread(target=run, args=(k,), name=f"vv-lane-{k}") for k in range(1, lanes)]
        for t in threads:
            t.start()
        run(0)
        for t in threads:
            t.join()
        for ex in errs:
            if ex is not None:
                if audio_streamer is not None:
                    audio_streamer.end()
                raise ex
        if audio_streamer is not None:
            audio_streamer.end()
        self.last_stats = {"lanes": lanes, "frames": sum(m.last_stats.get("frames", 0) for m in models),
                           "capture_fallbacks": [m.engine.stat(4) if hasattr(m.engine, "stat") else 0 for m in models],
                           "prefix_rows_reused": sum(m.last_stats.get("prefix_rows_reused", 0) for m in models),
                           "prompt_rows_computed": sum(m.last_stats.get("prompt_rows_computed", 0) for m in models),
                           "per_lane": [dict(m.last_stats) for m in models], "shards": shards}
        return outs

    def close_lanes(self):
        for m in self._lanes:
            m.engine.close()
        self._lanes = []

    # ------------------------------------------------------------------ continuous batching
    @torch.no_grad()
    def generate_continuous(self, requests: List[dict], tokenizer=None, generation_config=None, cfg_scale=1.0,
                            audio_streamer=None, is_prefill=True, return_speech=True, max_new_tokens=None,
                            max_length_times=2, stop_check_fn: Optional[Callable[[], bool]] = None,
                            max_concurrent: Optional[int] = None, **kwargs) -> List[VibeVoiceGenerationOutput]:
        """Decode a queue of single-utterance requests (each a dict of processor outputs with batch dimension 1) with up to
        `max_concurrent` (default: the engine's n_slots, at most 8) in flight.  A slot freed by EOS / length cap is refilled by
        the next queued request on the following iteration -- the running utterances never wait for a batch to drain; all rows
        in flight share every LM / diffusion-head weight pass.  Each request ends exactly as generate() on it alone would
        (greedy / forced decoding; with do_sample the draws interleave on the global generator).  Returns one
        VibeVoiceGenerationOutput per request, in request order; `audio_streamer` (batch_size = len(requests)) sees
        sample index = request index.
        A request's "seed" key (an int in [0, 2**64)) makes every draw of that request a function of the seed and the request's own
        counters (vibevoice_amd/noise.py): the same take in any slot, behind any queue.  One seeded request puts the whole call on that
        path -- the others get a seed from ONE torch.randint on the session's CPU generator, in request order."""
        e = self.engine
        n_req = len(requests)
        cfg_scales = _request_cfg_scales(requests, cfg_scale, "generate_continuous()")      # a request's own "cfg_scale" key, else the call's
        cap = min(max_concurrent or e.cfg.n_slots, e.cfg.n_slots, MAX_BATCH, e.cfg.max_rows // 2)
        if cap < 1:
            raise ValueError("no engine slot available")
        kwargs = dict(kwargs)
        step_cb = (kwargs.pop("_bench_hooks", None) or BenchHooks()).step_callback
        batch_exit = bool(kwargs.pop("_batch_exit", False))      # _generate_queued: the reference's batch-level early exit applies
        if not kwargs.get("refresh_negative", True):
            # with refresh_negative=False a row's negative cache depends on whether ANOTHER row of the same batch diffuses at that
            # step (the correction of :590-624): defined for the lock-step batch of generate(), not for a queue of requests
            raise NotImplementedError("refresh_negative=False is a rule over the rows of one lock-step batch: use generate() with at "
                                      f"most {MAX_BATCH} rows (continuous admission / larger batches refuse it)")
        # lockstep=False: independent requests, no cross-row tokenizer-cache coupling (_tokenizer_chain)
        S = self._session(tokenizer, generation_config, cfg_scales or _cfg_scale_values(cfg_scale, 1, "generate_continuous()"), kwargs,
                          audio_streamer, n_req, seeds=_request_seeds(requests, "generate_continuous()"),
                          sample_rows=lambda order: [u.idx for u in order], lockstep=False)
        self._frame_w = cap
        self._first_row = {}
        queue = list(range(n_req))
        done = [None] * n_req
        active: List[_Utt] = []
        it = 0
        stats = {"iterations": 0, "admissions": [], "max_in_flight": 0, "prefix_rows_reused": 0, "prompt_rows_computed": 0}
        with torch.cuda.stream(e.stream), _end_streamer_on_error(audio_streamer):
            e.embed([S.start_id], self._start_emb)
            while queue or active:
                S.step = it
                if step_cb is not None:
                    step_cb(it)
                if stop_check_fn is not None and stop_check_fn():
                    if audio_streamer is not None:
                        audio_streamer.end()
                    break
                if batch_exit and audio_streamer is not None and hasattr(audio_streamer, "finished_flags") and any(audio_streamer.finished_flags):
                    # standing in for ONE batched generate(): its loop ends with the first finished stream (:443-447).  The reference's
                    # lock-step batch has advanced EVERY row to this step by then; a queue has not -- rows still waiting for a slot come
                    # back as their prompt with no audio.  Said once, loudly: a caller that streams a batch this large wants to know.
                    if queue:
                        warnings.warn(f"generate(): the batch-level early exit (a finished audio stream, modeling_vibevoice_inference.py:443-447) fired "
                                      f"while {len(queue)} of {n_req} rows were still queued for an engine slot: the reference's lock-step batch would "
                                      "have decoded them up to this step, here they return as their prompt without audio.  Use batches of at most "
                                      f"{cap} rows with an audio_streamer, or generate_continuous() (no batch-level exit).", RuntimeWarning, stacklevel=3)
                    break
                active = self._retire_at_loop_end(active, audio_streamer)
                # ---- refill free slots ----
                in_flight = {u.slot for u in active}
                free = [s for s in range(cap) if s not in in_flight]
                while queue and free:
                    ri, slot = queue.pop(0), free.pop(0)
                    mnt = requests[ri].get("max_new_tokens", max_new_tokens)
                    u, reuse = self._admit(S, ri, slot, requests[ri], cfg_scales[ri], mnt, max_length_times, is_prefill)
                    stats["prefix_rows_reused"] += reuse
                    stats["prompt_rows_computed"] += len(u.ids) - reuse
                    done[ri] = u
                    stats["admissions"].append((it, ri, slot))
                    if u.max_steps > 0 and u.seq_len0 < u.max_length:
                        active.append(u)
                    else:
                        u.finished = True
                        u.reach_max = u.seq_len0 >= u.max_length
                if not active:
                    continue
                stats["max_in_flight"] = max(stats["max_in_flight"], len(active))
                before = active
                active = self._iterate(S, active)
                it += 1
                self._trim_frame_store(S, [u for u in before if u.finished], active)
            if audio_streamer is not None:
                audio_streamer.end()
            outs = []
            for ri in range(n_req):
                u = done[ri]
                if u is None:                       # stopped before admission
                    outs.append(VibeVoiceGenerationOutput(sequences=requests[ri]["input_ids"].to(self.device), speech_outputs=[None],
                                                          reach_max_step_sample=torch.tensor([False], device=self.device)))
                else:
                    outs.append(self._output([u], requests[ri]["input_ids"].cpu(), len(u.tokens), S.eos_id, return_speech))
        e.sync()
        self._release_frames()
        stats["iterations"] = it
        self.last_stats = {"frames": S.n_frames, "steps": it, **stats}
        return outs

    def _retire_at_loop_end(self, active, audio_streamer):
        """retire by the loop-level conditions of a batch-1 generate(): range(max_steps) exhausted / max_length; -> the survivors"""
        keep, keep_rows = [], []
        for i, u in enumerate(active):
            if u.step >= u.max_steps:
                u.finished = True
            elif u.seq_len0 + u.step >= u.max_length:
                u.finished = u.reach_max = True
            if not u.finished:
                keep.append(u)
                keep_rows.append(i)
            elif audio_streamer is not None:
                audio_streamer.end(torch.tensor([u.idx]))
        if keep and len(keep) != len(active):
            # _iterate packed the next-step embeddings in the order of the utterances it returned (`active`) and reads
            # them back by position: the rows of the survivors move up to the survivors' new positions
            sel = torch.tensor(keep_rows, dtype=torch.long, device=self._x_in.device)
            self._x_in[:len(keep)] = self._x_in.index_select(0, sel)
        return keep

    def _admit(self, S, ri, slot, r, cfg_scale, max_new_tokens, max_length_times, is_prefill):
        """request `r` (index ri of the queue) into engine slot `slot`: its _Utt, tokenizer state reset, voice samples encoded (or its
        prompt prefix restored) and prompt prefilled; -> (the utterance, the prompt positions taken from a prefix)"""
        e = self.engine
        ids_t = r["input_ids"].cpu()
        am = r.get("attention_mask")
        am = torch.ones_like(ids_t) if am is None else am.cpu()
        if ids_t.shape[0] != 1:
            raise ValueError("generate_continuous: every request carries exactly one utterance")
        L0 = ids_t.shape[1]
        mnt = self.max_position_embeddings - L0 if max_new_tokens is None else max_new_tokens
        u = _Utt(ri, slot, ids_t[0][am[0].bool()].tolist(), L0, min(L0 + mnt, e.max_ctx), max_length_times, S.start_id)
        u.forced, u.noise_fn, u.req = r.get("_forced_tokens"), r.get("_noise_fn"), r
        u.cfg_scale = cfg_scale
        if S.seeded:
            u.seed = S.seeds[ri]
        u.t_admit = S.step
        e.codec_reset(slot)
        sim = r.get("speech_input_mask")
        sp_idx = None if sim is None else _speech_positions(sim[0], am[0])
        rows = pos = None
        reuse = 0
        if r.get("prompt_prefix") is not None:      # the request starts with a prompt prefix: its voice rows are in the snapshot
            reuse = self._prefix_plan(r["prompt_prefix"], u.ids, None if sp_idx is None else sp_idx.tolist())
        if not reuse and is_prefill and r.get("speech_tensors") is not None and r.get("speech_masks") is not None:
            _, sp = self._process_speech_inputs(r["speech_tensors"], r["speech_masks"], r.get("_prefill_noise"), dev_gen=S.dev_gen,
                                                seeds=None if u.seed is None else [(u.seed, k) for k in range(r["speech_tensors"].shape[0])])
            if sp_idx is not None and sp_idx.numel():
                pos = sp_idx.to(self.device)
                rows = sp[:int(sp_idx.numel())]
        self._prefill_checked([(u, u.ids, rows, pos, 0, None, r["prompt_prefix"] if reuse else None, reuse)])
        return u, reuse

    def _trim_frame_store(self, S, ended, active):
        """a finished utterance's frames leave the shared frame store at once (its own contiguous tensor); blocks no live utterance
        points into are dropped, so the store follows the audio IN FLIGHT, not the queue's total"""
        for u in ended:
            if u.chunks:
                u.chunks = [torch.cat(u.chunks, dim=-1)]
        if ended:
            rows0 = [self._first_row[id(u)] for u in active if id(u) in self._first_row]
            lo = min(rows0 + [S.frame_rows]) // self.frame_block
            for b in range(min(lo, len(self._audio_blocks))):
                self._audio_blocks[b] = None
            for u in ended:
                self._first_row.pop(id(u), None)
