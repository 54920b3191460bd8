"""ctypes binding of libnc_mi355x.so (the C ABI declared in include/nc_mi355x.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there is
no Python/torch fallback for any operator.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnc_mi355x.so")

NC_OK, NC_EINVAL, NC_ENOTFOUND, NC_ESTATE, NC_EDEVICE, NC_ENOMEM, NC_EUNSUPPORTED = range(7)
NC_KC_NAMES = ("conv_k7", "conv_k1", "conv_down", "conv_up", "conv_misc", "rvq", "elem", "dwconv", "norm", "attn", "lstm", "stem", "head")


class NcError(RuntimeError):
    """Base of engine errors (the reference's NeuralCodecException, Core/Exceptions/NeuralCodecException.cs:10-73)."""


class NcDeviceError(NcError):
    pass


class NcDacConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("encoder_dim", C.c_int32), ("n_encoder_rates", C.c_int32),
                ("encoder_rates", C.c_int32 * 8), ("decoder_dim", C.c_int32), ("n_decoder_rates", C.c_int32),
                ("decoder_rates", C.c_int32 * 8), ("latent_dim", C.c_int32), ("n_codebooks", C.c_int32),
                ("codebook_size", C.c_int32), ("codebook_dim", C.c_int32)]


class NcSnacConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("encoder_dim", C.c_int32), ("n_encoder_rates", C.c_int32),
                ("encoder_rates", C.c_int32 * 8), ("decoder_dim", C.c_int32), ("n_decoder_rates", C.c_int32),
                ("decoder_rates", C.c_int32 * 8), ("latent_dim", C.c_int32), ("attn_window_size", C.c_int32),
                ("codebook_size", C.c_int32), ("codebook_dim", C.c_int32), ("n_vq_strides", C.c_int32),
                ("vq_strides", C.c_int32 * 8), ("noise", C.c_int32), ("depthwise", C.c_int32)]


class NcEncodecConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("dimension", C.c_int32), ("n_filters", C.c_int32),
                ("n_ratios", C.c_int32), ("ratios", C.c_int32 * 8), ("lstm_layers", C.c_int32), ("compress", C.c_int32),
                ("kernel_size", C.c_int32), ("last_kernel_size", C.c_int32), ("residual_kernel_size", C.c_int32),
                ("time_group_norm", C.c_int32), ("causal", C.c_int32), ("normalize", C.c_int32), ("segment_length", C.c_int32),
                ("segment_stride", C.c_int32), ("codebook_size", C.c_int32), ("n_codebooks", C.c_int32), ("frame_rate", C.c_int32),
                ("bandwidth", C.c_float)]


class NcProfileEntry(C.Structure):
    _fields_ = [("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class NcConvDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("K", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("dil", C.c_int32), ("out_pad", C.c_int32), ("Tin", C.c_int64),
                ("transposed", C.c_int32), ("tanh_out", C.c_int32)]


class NcHalo(C.Structure):
    _fields_ = [("enc_left", C.c_int64), ("enc_right", C.c_int64), ("dec_left", C.c_int64), ("dec_right", C.c_int64), ("align", C.c_int64)]


class NcChunkPlan(C.Structure):
    _fields_ = [("n_chunks", C.c_int64), ("chunk_frames", C.c_int64), ("halo_left", C.c_int64), ("halo_right", C.c_int64),
                ("arena_bytes", C.c_int64)]


class NcRaggedPlan(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("window_frames", "kept_frames", "halo_left", "halo_right", "n_windows", "n_window_batches",
                                         "n_exact_groups", "n_rows", "n_batches", "arena_bytes", "total_frames", "total_codes",
                                         "total_samples")]


class NcRaggedWindow(C.Structure):
    _fields_ = [("clip", C.c_int32), ("batch", C.c_int32), ("start", C.c_int64), ("width", C.c_int64), ("keep_start", C.c_int64),
                ("keep_frames", C.c_int64)]


class NcEncodecRaggedPlan(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_rows", "n_keys", "n_batches", "max_rows", "total_code_frames", "total_codes", "total_scales",
                                         "total_samples")]


class NcEncodecRaggedRow(C.Structure):
    _fields_ = [("clip", C.c_int32), ("segment", C.c_int32), ("batch", C.c_int32), ("row", C.c_int32), ("offset", C.c_int64),
                ("length", C.c_int64), ("frames", C.c_int64)]


class NcEncodecCausalInfo(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("hop", "halo_e", "halo_d", "min_frames_e", "min_frames_d", "carry_e", "carry_d", "taint_e", "taint_d")]


class NcEncodecCausalRow(C.Structure):
    _fields_ = [("entry", C.c_int32), ("batch", C.c_int32), ("row", C.c_int32), ("one_clip", C.c_int32), ("start", C.c_int64),
                ("width", C.c_int64), ("new_frames", C.c_int64)]


class NcSessionStep(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("w0", "w1", "k0", "k1", "resident")]


class NcDiaSampleParams(C.Structure):
    _fields_ = [("cfg_scale", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("eos", C.c_int32),
                ("pad", C.c_int32)]


class NcQualityCfg(C.Structure):
    _fields_ = [("n_scales", C.c_int32), ("W", C.c_int32 * 8), ("H", C.c_int32 * 8), ("n_mels", C.c_int32 * 8), ("fmin", C.c_float * 8),
                ("fmax", C.c_float * 8), ("clamp_eps", C.c_float), ("log_weight", C.c_float), ("mag_weight", C.c_float)]


class NcQualityRow(C.Structure):
    _fields_ = [("l1", C.c_float), ("si_sdr_db", C.c_float), ("mel_distance", C.c_float), ("mel_log", C.c_float * 8), ("mel_mag", C.c_float * 8),
                ("n_bad", C.c_int32)]


class NcLoudnessCfg(C.Structure):
    _fields_ = [("filter", C.c_int32), ("target_db", C.c_float)]


class NcLoudnessRow(C.Structure):
    _fields_ = [("lufs", C.c_float), ("gain", C.c_float), ("n_blocks", C.c_int32), ("n_pass_abs", C.c_int32), ("n_pass_rel", C.c_int32),
                ("n_bad", C.c_int32)]


class NcResampleCfg(C.Structure):
    _fields_ = [("zeros", C.c_int32), ("rolloff", C.c_float)]


NC_CHUNK_AUTO, NC_CHUNK_OFF = 0, -1
NC_KWEIGHT_REFERENCE, NC_KWEIGHT_DESIGNED = 0, 1
NC_WINDOW_HANN, NC_WINDOW_ONES = 0, 1

_lib = None

# every symbol include/nc_mi355x.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("nc_last_error", C.c_char_p, []),
    ("nc_version", C.c_char_p, []),
    ("nc_device_count", C.c_int, []),
    ("nc_debug_switches", C.c_char_p, []),
    ("nc_dac_create", C.c_int, [C.POINTER(NcDacConfig), C.c_int, C.POINTER(_P)]),
    ("nc_codec_destroy", C.c_int, [_P]),
    ("nc_codec_load_weights", C.c_int, [_P, C.c_char_p]),
    ("nc_codec_load_weights_mem", C.c_int, [_P, _P, C.c_size_t]),
    ("nc_blob_check", C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int32)]),
    ("nc_codec_set_stream", C.c_int, [_P, _P]),
    ("nc_codec_reset_stream", C.c_int, [_P]),
    ("nc_codec_synchronize", C.c_int, [_P]),
    ("nc_codec_check_errors", C.c_int, [_P]),
    ("nc_encodec_lstm_stats", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("nc_dac_query", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("nc_dac_encode", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_dac_encode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_dac_decode", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_dac_decode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_dac_from_codes", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, _P]),
    ("nc_dac_from_codes_dev", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, _P]),
    ("nc_dac_from_latents", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_dac_from_latents_dev", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_dac_decode_code_matrix", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_dac_decode_code_matrix_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_dac_encode_code_matrix", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_dac_encode_code_matrix_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_snac_create", C.c_int, [C.POINTER(NcSnacConfig), C.c_int, C.POINTER(_P)]),
    ("nc_snac_query", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("nc_snac_noise_len", C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_snac_process_audio_len", C.c_int, [_P, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    ("nc_snac_process_audio", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_uint64, _P]),
    ("nc_snac_encode", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_snac_encode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_snac_query_tensor", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("nc_snac_encode_tensor", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_snac_encode_tensor_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_snac_from_codes", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_snac_from_codes_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_snac_decode", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, C.c_uint64, _P]),
    ("nc_snac_decode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, C.c_uint64, _P]),
    ("nc_dac_halo", C.c_int, [C.POINTER(NcDacConfig), C.POINTER(NcHalo)]),
    ("nc_snac_halo", C.c_int, [C.POINTER(NcSnacConfig), C.POINTER(NcHalo)]),
    ("nc_codec_set_chunk_frames", C.c_int, [_P, C.c_int64]),
    ("nc_codec_chunk_plan", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.POINTER(NcChunkPlan)]),
    ("nc_dac_ragged_windows", C.c_int, [C.POINTER(NcDacConfig), C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, C.POINTER(NcRaggedPlan), _P,
                                        C.c_int64]),
    ("nc_snac_ragged_windows", C.c_int, [C.POINTER(NcSnacConfig), C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, C.POINTER(NcRaggedPlan), _P,
                                         C.c_int64]),
    ("nc_codec_set_ragged_window", C.c_int, [_P, C.c_int64, C.c_int32]),
    ("nc_codec_ragged_plan", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(NcRaggedPlan)]),
    ("nc_dac_ragged_query", C.c_int, [_P, C.c_int32, _P, _P, _P]),
    ("nc_dac_encode_ragged", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    ("nc_dac_encode_ragged_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    ("nc_dac_decode_codes_ragged", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("nc_dac_decode_codes_ragged_dev", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("nc_snac_ragged_query", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("nc_snac_encode_ragged", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("nc_snac_encode_ragged_dev", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("nc_snac_decode_ragged", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_uint64, _P]),
    ("nc_snac_decode_ragged_dev", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_uint64, _P]),
    ("nc_session_schedule", C.c_int, [C.POINTER(NcHalo), C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("nc_session_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("nc_session_destroy", C.c_int, [_P]),
    ("nc_session_reset", C.c_int, [_P]),
    ("nc_session_set_seed", C.c_int, [_P, C.c_uint64]),
    ("nc_session_query", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_session_pending", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("nc_session_push", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_session_push_dev", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_session_flush", C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_session_flush_dev", C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_session_pool_plan", C.c_int, [C.POINTER(NcHalo), C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    ("nc_session_pool_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("nc_session_pool_destroy", C.c_int, [_P]),
    ("nc_session_pool_reset_slot", C.c_int, [_P, C.c_int32]),
    ("nc_session_pool_set_seed", C.c_int, [_P, C.c_int32, C.c_uint64]),
    ("nc_session_pool_pending", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    ("nc_session_pool_query", C.c_int, [_P, C.c_int32, _P, _P, _P]),
    ("nc_session_pool_step", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("nc_session_pool_step_dev", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("nc_encodec_create", C.c_int,[C.POINTER(NcEncodecConfig), C.c_int, C.POINTER(_P)]),
    ("nc_encodec_set_bandwidth", C.c_int, [_P, C.c_float]),
    ("nc_encodec_query", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int32,
                                   C.POINTER(C.c_int64)]),
    ("nc_encodec_clip_length", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("nc_encodec_encode", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_encodec_encode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_encodec_decode", C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_encodec_decode_dev", C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_encodec_ragged_rows", C.c_int, [C.POINTER(NcEncodecConfig), C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(NcEncodecRaggedPlan), _P,
                                         C.c_int64]),
    ("nc_encodec_set_ragged_rows", C.c_int, [_P, C.c_int32]),
    ("nc_encodec_ragged_rows_of", C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(NcEncodecRaggedPlan), _P, C.c_int64]),
    ("nc_encodec_ragged_query", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("nc_encodec_encode_ragged", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    ("nc_encodec_encode_ragged_dev", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    ("nc_encodec_decode_ragged", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("nc_encodec_decode_ragged_dev", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("nc_encodec_stream_plan", C.c_int, [C.POINTER(NcEncodecConfig), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32,
                                         C.POINTER(NcEncodecRaggedPlan), _P, C.c_int64, _P, _P, _P]),
    ("nc_encodec_stream_pool_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("nc_encodec_stream_pool_destroy", C.c_int, [_P]),
    ("nc_encodec_stream_pool_reset_slot", C.c_int, [_P, C.c_int32]),
    ("nc_encodec_stream_pool_pending", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    ("nc_encodec_stream_pool_query", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    ("nc_encodec_stream_pool_plan", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.POINTER(NcEncodecRaggedPlan), _P, C.c_int64]),
    ("nc_encodec_stream_pool_step", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P]),
    ("nc_encodec_stream_pool_step_dev", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P]),
    ("nc_encodec_causal_plan", C.c_int, [C.POINTER(NcEncodecConfig), C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32,
                                         C.POINTER(NcEncodecCausalInfo), _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    ("nc_encodec_causal_pool_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("nc_encodec_causal_pool_destroy", C.c_int, [_P]),
    ("nc_encodec_causal_pool_reset_slot", C.c_int, [_P, C.c_int32]),
    ("nc_encodec_causal_pool_pending", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    ("nc_encodec_causal_pool_query", C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    ("nc_encodec_causal_pool_plan", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("nc_encodec_causal_pool_step", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("nc_encodec_causal_pool_step_dev", C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("nc_packed_bytes", C.c_int64, [C.c_int64, C.c_int32]),
    ("nc_pack_codes_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P]),
    ("nc_unpack_codes_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P]),
    ("nc_pack_codes", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_unpack_codes", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P]),
    ("nc_audio_resample_len", C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ("nc_audio_pcm16_to_float_dev", C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    ("nc_audio_float_to_pcm16_dev", C.c_int, [C.c_int, _P, C.c_int64, _P, _P]),
    ("nc_audio_mix_to_mono_dev", C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P]),
    ("nc_audio_interleave_dev", C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P]),
    ("nc_audio_deinterleave_dev", C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P]),
    ("nc_audio_resample_linear_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    ("nc_dia_output_query", C.c_int, [_P, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("nc_dia_decode_output", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_decode_output_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_apply_delay_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_revert_delay_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_revert_pack_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_adjust_speed_len", C.c_int64, [C.c_int64, C.c_float]),
    ("nc_dia_adjust_speed_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, _P, _P]),
    ("nc_dia_prompt_query", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    ("nc_dia_encode_prompts", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_encode_prompts_dev", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_dia_prefill_pack_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P]),
    ("nc_audio_mix_to_mono_ragged_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, _P, _P]),
    ("nc_dia_sample_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(NcDiaSampleParams), _P, _P, _P, _P]),
    ("nc_dia_sample_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(NcDiaSampleParams), _P, _P, _P]),
    ("nc_dia_generate_state_init_dev", C.c_int, [C.c_int, C.c_int32, _P, _P]),
    ("nc_dia_generate_step_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(NcDiaSampleParams), _P, _P, C.c_int64, C.c_int64,
                                           C.c_int32, _P, _P, C.c_int64, _P, _P, _P]),
    ("nc_dia_generate_lengths", C.c_int, [C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, C.POINTER(C.c_int64)]),
    ("nc_dia_generate_collect_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    ("nc_audio_stft_frames", C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ("nc_audio_dft_basis", C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    ("nc_audio_mel_filterbank", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P]),
    ("nc_audio_stft_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_audio_stft_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("nc_audio_mel_spectrogram_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P,
                                               _P, _P]),
    ("nc_audio_mel_spectrogram_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P]),
    ("nc_quality_metrics_dev", C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcQualityCfg), _P, _P]),
    ("nc_quality_metrics", C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcQualityCfg), _P]),
    ("nc_quality_metrics_host", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcQualityCfg), _P]),
    ("nc_audio_kweight_coeffs", C.c_int, [C.c_int32, C.c_int32, _P, _P]),
    ("nc_audio_kweight_tables", C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("nc_audio_kweight_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_audio_kweight", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("nc_audio_kweight_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("nc_loudness_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P, _P]),
    ("nc_loudness", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P]),
    ("nc_loudness_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P]),
    ("nc_loudness_normalize_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P, _P, _P, _P]),
    ("nc_loudness_normalize", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P, _P, _P]),
    ("nc_loudness_normalize_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.POINTER(NcLoudnessCfg), _P, _P, _P]),
    ("nc_audio_apply_gain_db_dev", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("nc_audio_apply_gain_db", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("nc_audio_apply_gain_db_host", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("nc_audio_resample_sinc_len", C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ("nc_audio_resample_sinc_geom", C.c_int, [C.c_int32, C.c_int32, C.POINTER(NcResampleCfg), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("nc_audio_resample_sinc_table", C.c_int, [C.c_int32, C.c_int32, C.POINTER(NcResampleCfg), _P]),
    ("nc_audio_resample_sinc_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcResampleCfg), _P, _P, _P]),
    ("nc_audio_resample_sinc", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcResampleCfg), _P, _P]),
    ("nc_audio_resample_sinc_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(NcResampleCfg), _P, _P]),
    ("nc_audio_istft_len", C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    ("nc_audio_idft_basis", C.c_int, [C.c_int32, C.c_int32, _P]),
    ("nc_audio_istft_workspace", C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    ("nc_audio_istft_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("nc_audio_istft", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_audio_istft_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_audio_mask_freq_bins", C.c_int, [C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("nc_audio_mask_time_frames", C.c_int, [C.c_float, C.c_int64, C.c_float, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("nc_audio_spec_fill_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_float, _P]),
    ("nc_audio_spec_fill_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_float]),
    ("nc_audio_dct_matrix", C.c_int, [C.c_int32, C.c_int32, _P]),
    ("nc_audio_mfcc_dev", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                    C.c_float, _P, _P, _P]),
    ("nc_audio_mfcc_host", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float, _P,
                                     _P]),
    ("nc_group_unique_id", C.c_int, [_P]),
    ("nc_group_create_rank", C.c_int, [C.c_int32, C.c_int32, _P, _P, C.POINTER(_P)]),
    ("nc_group_create_local", C.c_int, [C.c_int32, C.POINTER(_P), C.POINTER(_P)]),
    ("nc_group_create_local_ex", C.c_int, [C.c_int32, C.POINTER(_P), C.c_uint32, C.POINTER(_P)]),
    ("nc_group_destroy", C.c_int, [_P]),
    ("nc_group_info", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("nc_group_set_code_bits", C.c_int, [_P, C.c_int32]),
    ("nc_group_dac_encode_allgather_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    ("nc_group_snac_encode_allgather_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_group_wait", C.c_int, [_P]),
    ("nc_group_dac_encode_allgather", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    ("nc_group_snac_encode_allgather", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    ("nc_group_dac_encode_allgather_local_dev", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.c_int32, C.POINTER(_P),
                                                          C.POINTER(_P), C.POINTER(_P)]),
    ("nc_group_snac_encode_allgather_local_dev", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.c_int64, C.POINTER(_P)]),
    ("nc_group_encodec_encode_allgather_dev", C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P]),
    ("nc_group_encodec_encode_allgather_local_dev", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.c_int64, C.POINTER(_P), C.POINTER(_P)]),
    ("nc_codec_profile_enable", C.c_int, [_P, C.c_int32]),
    ("nc_codec_profile_reset", C.c_int, [_P]),
    ("nc_codec_profile_read", C.c_int, [_P, C.POINTER(NcProfileEntry)]),
    ("nc_op_conv1d", C.c_int, [C.c_int, C.POINTER(NcConvDesc), _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    ("nc_op_conv1d_bench", C.c_int, [C.c_int, C.POINTER(NcConvDesc), C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    ("nc_op_res_unit", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                 C.c_int32, C.POINTER(C.c_double)]),
    ("nc_op_vq_argmin", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, _P, C.c_int32, _P, _P]),
    ("nc_op_euclid_rvq", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("nc_op_dac_rvq", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32,
                                _P, _P, _P]),
    ("nc_op_rvq_update", C.c_int, [C.c_int, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    ("nc_op_vq_gather", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int64, _P, C.c_int64]),
    ("nc_op_encodec_lstm_carried", C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int64, _P, _P, _P]),
    ("nc_op_encodec_trace", C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("nc_op_concat_copy", C.c_int, [C.c_int, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64]),
    ("nc_op_log10f", C.c_int, [_P, C.c_int64, _P]),
    ("nc_op_logf", C.c_int, [_P, C.c_int64, _P]),
    ("nc_op_fold_weight_norm", C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    ("nc_op_dwconv1d", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("nc_op_layer_norm", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, _P]),
    ("nc_op_local_attn", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]),
    ("nc_op_avg_pool", C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, _P, _P]),
    ("nc_op_snac_unit", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
]


def lib():
    """Load the engine.  Importing torch first (when present) makes the loader bind the already
    loaded libamdhip64.so.7 of the torch wheel, so both share one HIP runtime in this process."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("NC_MI355X_LIB") or LIB_PATH          # (diagnostic: A/B of library builds, tools/probe/ab_libs*.sh)
    if not os.path.exists(path):
        raise NcError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(make -C neuralcodecs_amd/csrc). There is no fallback implementation.")
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401  (shares its HIP runtime with the engine)
        except Exception:
            pass
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        try:
            fn = getattr(L, name)
        except AttributeError:
            # A/B against an OLDER build of the library (NC_MI355X_LIB=<path>): only the exports named in NC_ALLOW_MISSING_EXPORTS (comma
            # separated) may be absent -- a symbol dropped by accident from any build must fail here, not as an AttributeError later
            if os.environ.get("NC_MI355X_LIB") and name in [x.strip() for x in os.environ.get("NC_ALLOW_MISSING_EXPORTS", "").split(",")]:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def lib_path() -> str:
    return os.environ.get("NC_MI355X_LIB") or LIB_PATH


def lib_sha256() -> str:
    """SHA-256 of the engine library file this process loads: profiles/traffic.json records the one its counters were measured on."""
    import hashlib
    h = hashlib.sha256()
    with open(lib_path(), "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def check(status: int) -> None:
    if status == NC_OK:
        return
    msg = lib().nc_last_error().decode(errors="replace")
    if status == NC_EINVAL:
        raise ValueError(msg)              # ArgumentException / ArgumentNullException
    if status == NC_ENOTFOUND:
        raise FileNotFoundError(msg)       # FileNotFoundException
    if status == NC_ESTATE:
        raise RuntimeError(msg)            # InvalidOperationException
    if status == NC_ENOMEM:
        raise MemoryError(msg)
    if status == NC_EDEVICE:
        raise NcDeviceError(msg)
    raise NcError(f"status {status}: {msg}")


def i64_array(values):
    """A host int64 array for the lengths[] / frames[] arguments of the ragged calls."""
    v = [int(x) for x in values]
    return (C.c_int64 * len(v))(*v)


def ragged_windows(fn, c_cfg, frames, decode: bool = False, kept_frames: int = 0, max_windows: int = 0):
    """nc_{dac,snac}_ragged_windows: (plan dict, list of window dicts in launch order) from a config alone -- no device."""
    f = i64_array(frames)
    p = NcRaggedPlan()
    check(fn(C.byref(c_cfg), 1 if decode else 0, len(f), f, int(kept_frames), int(max_windows), C.byref(p), None, 0))
    rows = (NcRaggedWindow * max(1, int(p.n_rows)))()
    check(fn(C.byref(c_cfg), 1 if decode else 0, len(f), f, int(kept_frames), int(max_windows), C.byref(p), rows, int(p.n_rows)))
    plan = {k: int(getattr(p, k)) for k, _ in NcRaggedPlan._fields_}
    return plan, [{k: int(getattr(rows[i], k)) for k, _ in NcRaggedWindow._fields_} for i in range(int(p.n_rows))]


def split_packed(flat, sizes):
    """Views of a packed 1-D array or tensor, one per clip."""
    out, o = [], 0
    for n in sizes:
        out.append(flat[o:o + n])
        o += n
    return out


class ProfileMixin:
    """HIP-event kernel-class profile of a codec handle (nc_codec_profile_*): the numbers bench.py's `roofline` objects come from."""

    def check_errors(self) -> None:
        """nc_codec_check_errors: device-side failures of an earlier device-pointer call (raises NcDeviceError); call it once the
        caller's own synchronisation (torch.cuda.synchronize) has made the stream idle."""
        check(lib().nc_codec_check_errors(self._h))

    def set_chunk_frames(self, n: int) -> None:
        """nc_codec_set_chunk_frames: NC_CHUNK_AUTO (0, default), NC_CHUNK_OFF (-1) or a chunk size in latent frames (long clips)."""
        check(lib().nc_codec_set_chunk_frames(self._h, int(n)))

    def chunk_plan(self, frames: int, decode: bool = False, B: int = 1) -> dict:
        """nc_codec_chunk_plan: what a call on `frames` latent frames would do under the handle's chunk setting."""
        p = NcChunkPlan()
        check(lib().nc_codec_chunk_plan(self._h, 1 if decode else 0, int(B), int(frames), C.byref(p)))
        return {k: int(getattr(p, k)) for k, _ in NcChunkPlan._fields_}

    def set_ragged_window(self, kept_frames: int = 0, max_windows: int = 0) -> None:
        """nc_codec_set_ragged_window: kept frames per window and rows per launch batch of the ragged calls (0 = default)."""
        check(lib().nc_codec_set_ragged_window(self._h, int(kept_frames), int(max_windows)))

    def ragged_plan(self, frames, decode: bool = False) -> dict:
        """nc_codec_ragged_plan: what a ragged call on clips of these frame counts would do under the handle's setting."""
        f = i64_array(frames)
        p = NcRaggedPlan()
        check(lib().nc_codec_ragged_plan(self._h, 1 if decode else 0, len(f), f, C.byref(p)))
        return {k: int(getattr(p, k)) for k, _ in NcRaggedPlan._fields_}

    def profile_enable(self, on: bool = True):
        check(lib().nc_codec_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        check(lib().nc_codec_profile_reset(self._h))

    def profile_read(self):
        arr = (NcProfileEntry * len(NC_KC_NAMES))()
        check(lib().nc_codec_profile_read(self._h, arr))
        return {n: {"launches": arr[i].launches, "ms": arr[i].ms, "flops": arr[i].flops, "bytes": arr[i].bytes}
                for i, n in enumerate(NC_KC_NAMES)}
