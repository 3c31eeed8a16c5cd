"""ctypes binding of libvvhip.so (include/vvhip.h).  There is NO fallback: if the
shared library is missing or a symbol is absent, importing the engine raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VVHIP_LIB", os.path.join(HERE, "libvvhip.so"))   # override only for A/B benchmarking of builds


class VVConfig(C.Structure):
    _fields_ = [
        ("lm_hidden", C.c_int), ("lm_layers", C.c_int), ("lm_heads", C.c_int), ("lm_kv_heads", C.c_int),
        ("lm_head_dim", C.c_int), ("lm_inter", C.c_int), ("lm_vocab", C.c_int), ("lm_eps", C.c_float),
        ("head_layers", C.c_int), ("head_ffn", C.c_int), ("latent_dim", C.c_int), ("head_eps", C.c_float),
        ("n_filters", C.c_int), ("n_ratios", C.c_int), ("ratios", C.c_int * 8),
        ("n_stages", C.c_int), ("enc_depths", C.c_int * 8), ("sem_dim", C.c_int),
        ("has_acoustic_encoder", C.c_int), ("codec_eps", C.c_float),
        ("n_slots", C.c_int), ("max_ctx", C.c_int), ("max_rows", C.c_int), ("xsplit", C.c_int),
        ("attn_splits", C.c_int), ("enc_frames", C.c_int), ("use_graph", C.c_int), ("tts_layers", C.c_int),
    ]


class VVRow(C.Structure):
    _fields_ = [("cache", C.c_int), ("pos", C.c_int)]


_P = C.c_void_p


class VVGemvCase(C.Structure):
    """vv_gemv_case_args (include/vvhip.h): every operand of one decode-GEMV launch"""
    _fields_ = [
        ("W", _P), ("W2", _P), ("X", _P), ("Y", _P),
        ("T", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ldx", C.c_int), ("ldy", C.c_int),
        ("pro", C.c_int), ("epi", C.c_int),
        ("nw", _P), ("eps", C.c_float), ("bias", _P), ("nscale", _P),
        ("mod_scale", _P), ("mod_shift", _P), ("ld_mod", C.c_int),
        ("addvec", _P), ("x_row_mod", C.c_int), ("add_rows_per_vec", C.c_int),
        ("gate", _P), ("ld_gate", C.c_int),
        ("z", _P), ("x0p", _P), ("coef", _P), ("cfg", C.c_float), ("n_cfg", C.c_int), ("sde_noise", _P),
        ("kgrid", C.c_int), ("yparts", _P), ("xa", _P), ("n_xa", C.c_int), ("ya", _P), ("n_ya", C.c_int), ("part_stride", C.c_int),
        ("sl_n", C.c_int), ("sl_T", C.c_int), ("sl_x", C.c_int), ("sl_y", C.c_int), ("sl_id", C.c_int * 8),
        ("dw_hist", _P), ("dw_w", _P), ("dw_b", _P), ("dw_gamma", _P), ("dw_nw", _P), ("dw_xout", _P), ("dw_hnew", _P),
        ("cfg_rows", _P),
    ]


class VVGemv16pCase(C.Structure):
    """vv_gemv16p_case_args (include/vvhip.h): every operand of one launch of the batch-decode packed GEMV"""
    _fields_ = [
        ("W", _P), ("W2", _P), ("Xp", _P), ("Y", _P), ("Yp", _P), ("bias", _P), ("gate", _P),
        ("T", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ldy", C.c_int), ("ld_gate", C.c_int),
        ("ssq_in", _P), ("ssq_tiles", C.c_int), ("eps", C.c_float),
        ("Xs", _P),
        ("pk_nw", _P), ("pk_sc", _P), ("ld_pk", C.c_int), ("ssq_out", _P),
        ("z", _P), ("x0p", _P), ("coef", _P), ("cfg", C.c_float), ("n_cfg", C.c_int), ("sde_noise", _P),
        ("cfg_rows", _P),
    ]


class VVNoiseKey(C.Structure):
    """vv_noise_key (include/vvhip.h): the seed's two halves, the first counter word t and aux of one row of vv_noise_rows"""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("t0", C.c_uint32), ("aux", C.c_uint32)]


class VVResampleRow(C.Structure):
    """vv_resample_row (include/vvhip.h): the stream, the input samples and the flush mark of one row of vv_resample_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int)]


class VVTempoRow(C.Structure):
    """vv_tempo_row (include/vvhip.h): the stream, the input samples, the flush mark and the speed P / Q of one row of vv_tempo_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("P", C.c_int), ("Q", C.c_int)]


class VVFormantRow(C.Structure):
    """vv_formant_row (include/vvhip.h): the stream, the input samples, the flush mark and the warp A / B of one row of vv_formant_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("A", C.c_int), ("B", C.c_int)]


class VVPitchRow(C.Structure):
    """vv_pitch_row (include/vvhip.h): the stream, the input samples, the flush mark and the ratio P / Q of one row of vv_pitch_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("P", C.c_int), ("Q", C.c_int)]


class VVLevelRow(C.Structure):
    """vv_level_row (include/vvhip.h): the stream, the input samples, the flush mark and the gain of one row of vv_level_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("gain", C.c_float)]


class VVLoudRow(C.Structure):
    """vv_loud_row (include/vvhip.h): the stream, the input samples, the flush mark and t, g0, wmax of one row of vv_loud_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("t", C.c_float), ("g0", C.c_float), ("wmax", C.c_float)]


class VVPauseRow(C.Structure):
    """vv_pause_row (include/vvhip.h): the stream, the input samples, the flush mark, seg, the caps C, C0 and theta of one row of vv_pause_rows"""
    _fields_ = [("stream", C.c_int), ("n_in", C.c_int), ("flush", C.c_int), ("seg", C.c_int), ("C", C.c_int), ("C0", C.c_int),
                ("theta", C.c_longlong)]


GEMV_REFUSED = 1     # VV_GEMV_REFUSED
TEMPO_OVER_CAPACITY = 3     # VV_TEMPO_OVER_CAPACITY
_SIGS = {
    "vv_create": (C.c_int, [C.POINTER(VVConfig), C.POINTER(_P)]),
    "vv_create_shared": (C.c_int, [C.POINTER(VVConfig), _P, C.POINTER(_P)]),
    "vv_destroy": (None, [_P]),
    "vv_last_error": (C.c_char_p, [_P]),
    "vv_num_weights": (C.c_int, [_P]),
    "vv_weight_info": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "vv_upload": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int64]),
    "vv_set_speech_factors": (C.c_int, [_P, C.c_float, C.c_float]),
    "vv_set_valid_tokens": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    "vv_set_schedule": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "vv_set_schedule_sde": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "vv_set_schedule_general": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, _P]),
    "vv_lm_forward": (C.c_int, [_P, _P, C.c_int, C.POINTER(VVRow), _P, _P]),
    "vv_lm_forward_range": (C.c_int, [_P, _P, C.c_int, C.POINTER(VVRow), _P, _P, C.c_int, C.c_int, C.c_int]),
    "vv_kv_import": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vv_kv_import_at": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vv_add_type_embedding": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P]),
    "vv_eos_logit": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "vv_embed": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P]),
    "vv_lm_logits": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "vv_lm_logits_full": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "vv_lm_warp_valid": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P]),
    "vv_noise_rows": (C.c_int, [_P, _P, C.c_int, C.POINTER(VVNoiseKey), C.c_uint32, C.c_int, C.c_int, C.c_int, _P]),
    "vv_diffusion_sample": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_float, _P]),
    "vv_diffusion_sample_sde": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_float, _P]),
    "vv_diffusion_sample_rows": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "vv_diffusion_sample_general": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_float, _P, _P]),
    "vv_head_forward": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_float), _P, _P]),
    "vv_codec_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vv_semantic_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "vv_codec_chain_batch": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "vv_acoustic_encode": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "vv_acoustic_encode_ragged": (C.c_int, [_P, _P, C.c_int, C.c_longlong, _P, _P]),
    "vv_kv_move": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "vv_kv_export": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "vv_kv_snapshot_bytes": (C.c_int64, [_P, C.c_int]),
    "vv_kv_snapshot": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "vv_kv_restore": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "vv_set_enc_pass_frames": (C.c_int, [_P, C.c_int]),
    "vv_audio_to_pcm16": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "vv_resampler_set": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "vv_resampler_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_resample_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVResampleRow), _P, C.c_int, _P, C.c_int, C.c_int,
                                   C.POINTER(C.c_int)]),
    "vv_resample_once": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_tempo_set": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "vv_tempo_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_tempo_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVTempoRow), _P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_int), _P,
                                C.c_int]),
    "vv_tempo_once": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_pitch_set": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "vv_pitch_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_pitch_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVPitchRow), _P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_pitch_once": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_formant_set": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "vv_formant_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_formant_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVFormantRow), _P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_formant_once": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_longlong]),
    "vv_level_set": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "vv_level_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_level_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVLevelRow), _P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_level_once": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_loud_set": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "vv_loud_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_loud_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVLoudRow), _P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_loud_energy": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_loud_once": (C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "vv_pause_set": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "vv_pause_reset": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_pause_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(VVPauseRow), _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "vv_pause_totals": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "vv_pause_once": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_longlong,
                                _P]),
    "vv_codec_reset": (C.c_int, [_P, _P, C.c_int]),
    "vv_connect": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "vv_packed_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "vv_pack_matrix": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vv_unpack_matrix": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vv_lora_merge_raw": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_float, C.c_int]),
    "vv_weight_read": (C.c_int, [_P, _P, C.c_char_p, _P]),
    "vv_weight_shape": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vv_lora_merge": (C.c_int, [_P, _P, C.c_char_p, _P, _P, C.c_int, C.c_float, C.c_int]),
    "vv_lora_reset": (C.c_int, [_P, _P, C.c_char_p]),
    "vv_gemm_raw": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              _P, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int]),
    "vv_gemv_case": (C.c_int, [_P, C.POINTER(VVGemvCase), C.c_int, C.POINTER(C.c_int)]),
    "vv_w13_twin_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "vv_w13_pack_matrix": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vv_w13_unpack_matrix": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "vv_w13_gemv_case": (C.c_int, [_P, C.POINTER(VVGemvCase), _P, _P, C.c_int, C.c_int]),
    "vv_gemv16p_case": (C.c_int, [_P, C.POINTER(VVGemv16pCase), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "vv_pack16_case": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_float, _P, _P, C.c_int, _P, C.c_int, C.c_int]),
    "vv_pack16_tiles_case": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "vv_gemm3_raw": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    "vv_profile_begin": (C.c_int, [_P]),
    "vv_profile_end": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vv_profile_replay": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vv_profile_replay_family": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vv_stat": (C.c_int64, [_P, C.c_int]),
    "vv_build_id": (C.c_char_p, []),
    "vv_check": (C.c_int, [_P, _P]),
}

EXPORTS = tuple(_SIGS)
_lib = None


def load():
    """dlopen libvvhip.so and bind every symbol of include/vvhip.h; raises if impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine has not been built "
            "(run `python -m vibevoice_amd.build`); there is no CPU/PyTorch fallback")
    from . import build as _build
    if _build.have_sources() and _build.binary_id(LIB_PATH) != _build.source_id():
        # a binary from other sources must never run silently: rebuild where a compiler exists, refuse otherwise
        import sys
        print(f"[vibevoice_amd] {LIB_PATH} was built from other sources (binary id {_build.binary_id(LIB_PATH)}, sources "
              f"{_build.source_id()}): rebuilding with hipcc (about two minutes)", file=sys.stderr, flush=True)
        try:
            _build.build_locked()          # one process compiles; the other ranks of a torchrun job wait for its binary
        except Exception as ex:
            raise RuntimeError(
                f"{LIB_PATH} was built from different sources (binary id {_build.binary_id(LIB_PATH)}, sources "
                f"{_build.source_id()}) and could not be rebuilt ({ex}); run `python -m vibevoice_amd.build`") from ex
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
