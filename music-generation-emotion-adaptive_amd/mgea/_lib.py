"""ctypes binding of the C ABI in include/mgea.h (libmgea_hip.so, built by csrc/Makefile).

There is NO CPU fallback: if the shared library is missing, or no HIP device is visible when an
engine is created, this raises -- the product path never routes through oracle/ or PyTorch math.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MGEA_LIB_PATH: tools/ only -- an instrumented build of the same library, e.g. tools/libmgea_hip_stamps.so)
LIB_PATH = os.environ.get("MGEA_LIB_PATH") or os.path.join(_HERE, "libmgea_hip.so")

OK, EINVAL, ENOMEM, EHIP, ECAPACITY, ENODEVICE = 0, -1, -2, -3, -4, -5
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
BLOCK_PRELN_GELU, BLOCK_POSTLN_RELU = 0, 1
POS_REFERENCE, POS_ABSOLUTE, POS_CAUSAL = 0, 1, 2
KV_PAGE_TOKENS = 64


class MgeaError(RuntimeError):
    """A HIP / allocation failure inside the native library."""


class DecoderConfig(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("seq_len", C.c_int32), ("d_model", C.c_int32), ("n_head", C.c_int32),
                ("n_layer", C.c_int32), ("d_ff", C.c_int32), ("max_batch", C.c_int32), ("max_ctx", C.c_int32),
                ("dtype", C.c_int32), ("block_mode", C.c_int32), ("pos_mode", C.c_int32), ("ln_eps", C.c_float)]


class SamplerConfig(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("eos_id", C.c_int32),
                ("seed", C.c_uint64)]


class RowSampler(C.Structure):
    """mgea_row_sampler: one batch row's sampler settings (mgea_decoder_generate_rows, mgea_op_sample_rows)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("eos_id", C.c_int32), ("max_new_tokens", C.c_int32), ("seed", C.c_uint64), ("stream", C.c_uint32),
                ("reserved", C.c_uint32)]


class RowLogits(C.Structure):
    """mgea_row_logits: one batch row's logit bias and minimum length (mgea_decoder_generate_rows_biased, mgea_op_sample_rows_biased)."""
    _fields_ = [("bias_dev", C.c_void_p), ("min_new_tokens", C.c_int32), ("reserved", C.c_int32)]


class RowGuidance(C.Structure):
    """mgea_row_guidance: one batch row's classifier-free-guidance pair (mgea_decoder_generate_rows_guided)."""
    _fields_ = [("shadow_row", C.c_int32), ("scale", C.c_float)]


class RowSchedule(C.Structure):
    """mgea_row_schedule: one batch row's prompt schedule (mgea_decoder_generate_rows_scheduled)."""
    _fields_ = [("n_segments", C.c_int32), ("key", C.c_int32), ("threshold", C.c_int32 * 7), ("reserved", C.c_int32)]


class RowTruncation(C.Structure):
    """mgea_row_truncation: one batch row's min-p / typical-p / epsilon / eta settings (mgea_decoder_generate_rows_truncated)."""
    _fields_ = [("min_p", C.c_float), ("typical_p", C.c_float), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float)]


class RowBlend(C.Structure):
    """mgea_row_blend: one batch row's blend group and weight (mgea_decoder_generate_rows_blended)."""
    _fields_ = [("leader", C.c_int32), ("weight", C.c_float)]


BLEND_MAX_ROWS = 8


class RowClassPenalty(C.Structure):
    """mgea_row_class_penalty: one batch row's windowed penalty over token classes (mgea_decoder_generate_rows_class_penalized)."""
    _fields_ = [("frequency", C.c_float), ("presence", C.c_float), ("window", C.c_int32), ("reserved", C.c_int32)]


CLASS_PENALTY_MAX_WINDOW = 4096


class BertConfig(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("max_pos", C.c_int32), ("dim", C.c_int32), ("n_heads", C.c_int32),
                ("n_layers", C.c_int32), ("hidden", C.c_int32), ("num_labels", C.c_int32),
                ("max_tokens", C.c_int32), ("dtype", C.c_int32), ("ln_eps", C.c_float)]


_P = C.c_void_p
_I32, _I64, _F = C.c_int32, C.c_int64, C.c_float


class DecodeGemmArgs(C.Structure):
    """mgea_decode_gemm_args: one decode-step GEMM on caller buffers (mgea_op_decode_gemm, test only)."""
    _fields_ = [("epi", _I32), ("rowmajor", _I32), ("w_f16", _I32), ("M", _I32), ("N", _I32), ("K", _I32), ("act", _I32), ("eps", _F),
                ("a_dev", _P), ("w_dev", _P), ("bias_dev", _P), ("ln_c1_dev", _P), ("ln_g_dev", _P), ("ln_b_dev", _P),
                ("stats_in_dev", _P), ("n_part", _I32), ("part_cnt", _I32), ("out_dev", _P), ("stats_out_dev", _P),
                ("pages_dev", _P), ("page_table_dev", _P), ("ctx_len_dev", _P), ("lens_dev", _P),
                ("n_pages", _I32), ("page_dtype", _I32), ("n_head", _I32), ("head_dim", _I32), ("layer", _I32), ("max_pages", _I32),
                ("T", _I32), ("arith_batch", _I32), ("partials_dev", _P)]


class StepTailArgs(C.Structure):
    """mgea_step_tail_args: one end-of-step launch on caller buffers (mgea_op_step_tail, test only)."""
    _fields_ = [("kind", _I32), ("B", _I32), ("n_steps", _I32), ("eos_id", _I32),
                ("cur_ids_dev", _P), ("ctx_len_dev", _P), ("done_dev", _P), ("row_step_dev", _P), ("n_done_dev", _P), ("ids_out_dev", _P),
                ("rows", C.POINTER(RowSampler)), ("ctx_cap", C.POINTER(_I32)), ("logits_rows", C.POINTER(RowLogits)),
                ("pval_dev", _P), ("pidx_dev", _P), ("n_tiles", _I32), ("reserved", _I32), ("sampled_dev", _P),
                ("tok_emb_dev", _P), ("pos_emb_dev", _P), ("x_dev", _P), ("stats_dev", _P),
                ("C", _I32), ("vocab", _I32), ("pos_rows", _I32), ("absolute_pos", _I32),
                ("qkv0_dev", _P), ("qkv_dev", _P), ("pages_dev", _P), ("page_table_dev", _P),
                ("n_pages", _I32), ("page_dtype", _I32), ("n_head", _I32), ("head_dim", _I32), ("arith_batch", _I32), ("max_pages", _I32),
                ("presence_dev", _P), ("V", _I32), ("hist_stride", _I32),
                ("logprob_step_dev", _P), ("choice_step_dev", _P), ("logprob_hist_dev", _P), ("choice_hist_dev", _P), ("err_flag_dev", _P),
                ("logits_dev", _P), ("forced_dev", _P), ("forced_stride", _I32), ("n_state", _I32), ("n_class", _I32), ("reserved2", _I32),
                ("class_of_dev", _P), ("next_dev", _P), ("states_dev", _P)]


TAIL_ARGMAX, TAIL_ARGMAX_EMBED, TAIL_ADVANCE, TAIL_EMBED_QKV0, TAIL_SAMPLE = 0, 1, 2, 3, 4
DECODE_GEMM_PLAN_INTS = 11
EPI_QKV, EPI_RES, EPI_ACT, EPI_LOGITS = 0, 1, 2, 3
DG_SKINNY, DG_HEAD, DG_GEMV = 0, 1, 2

# name -> (restype, argtypes); every symbol include/mgea.h declares
PROTOTYPES = {
    "mgea_last_error": (C.c_char_p, []),
    "mgea_version": (C.c_int, []),
    "mgea_device_count": (C.c_int, []),
    "mgea_tune_set": (C.c_int, [C.c_char_p, _I32]),
    "mgea_tune_get": (C.c_int, [C.c_char_p, C.POINTER(_I32)]),
    "mgea_decoder_arena_layout": (C.c_int, [C.POINTER(DecoderConfig), C.POINTER(_I64), C.POINTER(_I32), C.POINTER(_I64)]),
    "mgea_decoder_create": (C.c_int, [C.POINTER(DecoderConfig), _P, C.POINTER(_P)]),
    "mgea_decoder_destroy": (C.c_int, [_P]),
    "mgea_decoder_refresh_weights": (C.c_int, [_P, _P]),
    "mgea_decoder_reset": (C.c_int, [_P, _I32, _I32, _P]),
    "mgea_decoder_forward": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P]),
    "mgea_decoder_step": (C.c_int, [_P, _P, C.POINTER(SamplerConfig), _P, _P, _P]),
    "mgea_decoder_generate": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(SamplerConfig), _P, _P]),
    "mgea_decoder_generate_penalized": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(SamplerConfig), _F, _P, _P]),
    "mgea_decoder_generate_rows": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), _P, _P]),
    "mgea_decoder_generate_rows_biased": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P, _P]),
    "mgea_decoder_generate_rows_scored": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P, _P, _P,
                                                   _P, _P]),
    "mgea_decoder_set_grammar": (C.c_int, [_P, _P, _P, _I32, _I32, _P]),
    "mgea_decoder_generate_rows_grammar": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P, _P, _P,
                                                    _P, _P, _P]),
    "mgea_decoder_generate_rows_guided": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P,
                                                   C.POINTER(RowGuidance), _P, _P, _P, _P, _P]),
    "mgea_decoder_guidance_info": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_generate_rows_scheduled": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P,
                                                      C.POINTER(RowGuidance), C.POINTER(RowSchedule), _I32, _P, _P, _P, _P, _P]),
    "mgea_decoder_generate_rows_truncated": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P,
                                                      C.POINTER(RowGuidance), C.POINTER(RowSchedule), _I32, _P, _P, _P, _P,
                                                      C.POINTER(RowTruncation), _P]),
    "mgea_decoder_truncation_info": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_generate_rows_blended": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P,
                                                    C.POINTER(RowGuidance), C.POINTER(RowSchedule), _I32, _P, _P, _P, _P,
                                                    C.POINTER(RowTruncation), C.POINTER(RowBlend), _P]),
    "mgea_decoder_blend_info": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_set_penalty_classes": (C.c_int, [_P, _P, _I32, _P]),
    "mgea_decoder_generate_rows_class_penalized": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, C.POINTER(RowSampler), C.POINTER(RowLogits), _P,
                                                            C.POINTER(RowGuidance), C.POINTER(RowSchedule), _I32, _P, _P, _P, _P,
                                                            C.POINTER(RowTruncation), C.POINTER(RowBlend), C.POINTER(RowClassPenalty), _P]),
    "mgea_decoder_class_penalty_info": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_schedule_info": (C.c_int, [_P, C.POINTER(_I64), _P]),
    "mgea_decoder_segments": (C.c_int, [_P, _P, _P]),
    "mgea_decoder_set_window": (C.c_int, [_P, _I32, _I32, _I32, _P]),
    "mgea_decoder_window_info": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32), _P]),
    "mgea_decoder_grammar_states": (C.c_int, [_P, _P, _P]),
    "mgea_decoder_grammar_info": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_presence": (C.c_int, [_P, _P, _P]),
    "mgea_decoder_context_lengths": (C.c_int, [_P, _P, _P]),
    "mgea_decoder_kv_pages": (C.c_int, [_P, _I32, _P, _I64, _P, C.POINTER(_I64), _P]),
    "mgea_decoder_stats": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_qkv0_table_bytes": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_decoder_error_flags": (C.c_int, [_P, C.POINTER(_I32), _P]),
    "mgea_bert_error_flags": (C.c_int, [_P, C.POINTER(_I32), _P]),
    "mgea_decoder_profile": (C.c_int, [_P, _I32]),
    "mgea_decoder_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(_I64), _I32]),
    "mgea_bert_arena_layout": (C.c_int, [C.POINTER(BertConfig), C.POINTER(_I64), C.POINTER(_I32), C.POINTER(_I64)]),
    "mgea_bert_create": (C.c_int, [C.POINTER(BertConfig), _P, C.POINTER(_P)]),
    "mgea_bert_destroy": (C.c_int, [_P]),
    "mgea_bert_forward": (C.c_int, [_P, _P, _P, _I32, _I32, _P, _P, _P]),
    "mgea_bert_forward_packed": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mgea_bert_stats": (C.c_int, [_P, C.POINTER(_I64)]),
    "mgea_lora_merge": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _F, _P]),
    "mgea_op_gemm_workspace_floats": (_I64, [_I32, _I32, _I32]),
    "mgea_op_gemm_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "mgea_op_layernorm": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _F, _P]),
    "mgea_op_attention_f32": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_attention_f32_ex": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_attention_f32_causal": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_logprob_gather": (C.c_int, [_P, _I64, _P, _P, _I32, _I32, _P]),
    "mgea_op_f32_to_bf16": (C.c_int, [_P, _P, _I64, _P]),
    "mgea_op_gemm_bf16": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_gemm_bf16_ln": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, C.POINTER(_I32), _P]),
    "mgea_op_ln_rowstat": (C.c_int, [_P, _P, _I32, _I32, _I32, _F, _P]),
    "mgea_op_fold_ln_bf16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "mgea_op_attention_bf16": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_layernorm_bf16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _F, _P]),
    "mgea_op_gemm_f16_ln": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, C.POINTER(_I32), _P]),
    "mgea_op_gemm16": (C.c_int, [_P, _I32, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, C.POINTER(_I32), _P]),
    "mgea_op_f32_to_16": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "mgea_op_fold_ln_16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "mgea_op_attention16": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _I32, _P]),
    "mgea_op_kv_scatter_f16": (C.c_int, [_P, _P, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_dec_embed_f16": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "mgea_op_attention_paged": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, C.POINTER(_I32), _P]),
    "mgea_op_attn_split_count": (C.c_int, [_I32, _I32, _I32, _I32]),
    "mgea_op_attn_split_scratch": (C.c_int, [_I32, C.POINTER(_I64), C.POINTER(_I64)]),
    "mgea_op_attention_paged_ex": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32,
                                             _P, _I64, _P, _I64, C.POINTER(_I32), _P]),
    "mgea_op_attention_paged_causal": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32,
                                                 _P, _I64, _P, _I64, C.POINTER(_I32), _P]),
    "mgea_op_tiled_weight_floats": (C.c_int64, [_I32, _I32]),
    "mgea_op_tile_weights": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "mgea_op_tile_rows": (C.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "mgea_op_fold_ln": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P]),
    "mgea_op_skinny": (C.c_int, [_I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_skinny_logits_partials": (C.c_int, [_I32, _I32, _I32]),
    "mgea_op_decode_gemm": (C.c_int, [C.POINTER(DecodeGemmArgs), C.POINTER(_I32), _P]),
    "mgea_op_tile_weights_f16": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "mgea_op_ln_vectors": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    "mgea_op_sample": (C.c_int, [_P, _I32, _I32, C.POINTER(SamplerConfig), _I64, _P, _P, _P]),
    "mgea_op_sample_penalized": (C.c_int, [_P, _I32, _I32, C.POINTER(SamplerConfig), _F, _P, _I64, _P, _P, _P]),
    "mgea_op_sample_rows": (C.c_int, [_P, _I32, _I32, C.POINTER(RowSampler), _P, _I64, _P, _P, _P]),
    "mgea_op_sample_rows_biased": (C.c_int, [_P, _I32, _I32, C.POINTER(RowSampler), _P, C.POINTER(RowLogits), _I64, _P, _P, _P]),
    "mgea_op_sample_rows_scored": (C.c_int, [_P, _I32, _I32, C.POINTER(RowSampler), _P, C.POINTER(RowLogits), _I64, _P, _P, _P, _P, _P, _P]),
    "mgea_op_window_evict": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _P, _I32, _P]),
    "mgea_op_guidance_mix": (C.c_int, [_P, _I32, _I32, _P, _P, _P]),
    "mgea_op_blend_mix": (C.c_int, [_P, _I32, _I32, _P, _P, _P]),
    "mgea_op_class_penalty": (C.c_int, [_P, _I32, _I32, _P, _I32, _P, _I32, _P, _P, C.POINTER(RowClassPenalty), _P]),
    "mgea_op_recondition": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P,
                                      _P, _P, _P]),
    "mgea_op_sample_rows_grammar": (C.c_int, [_P, _I32, _I32, C.POINTER(RowSampler), _P, C.POINTER(RowLogits), _P, _P, _I32, _I32, _P, _I64, _P,
                                              _P, _P, _P]),
    "mgea_op_sample_rows_truncated": (C.c_int, [_P, _I32, _I32, C.POINTER(RowSampler), _P, C.POINTER(RowLogits), C.POINTER(RowTruncation), _I64,
                                                _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P]),
    "mgea_op_attention_cls": (C.c_int, [_P, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_bert_embed": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "mgea_op_gather_cls": (C.c_int, [_P, _I32, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P]),
    "mgea_op_gemm_f32_direct": (C.c_int, [_P, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_slab_bias_act": (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_slab_bias_res_ln": (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _P, _P, _F, _I32, _I32, _I32, _P]),
    "mgea_op_slab_logits_argmax": (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32, _I32, _P, _P]),
    "mgea_op_slab_qkv_scatter": (C.c_int, [_P, _I32, _I64, _I32, _P, _P, _P, _I32, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "mgea_op_step_tail": (C.c_int, [C.POINTER(StepTailArgs), _P]),
    "mgea_op_dec_embed": (C.c_int, [_I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "mgea_op_take_last": (C.c_int, [_P, _P, _P, _I32, _I32, _P]),
    "mgea_op_add_lens": (C.c_int, [_P, _P, _I32, _I32, _P]),
    "mgea_op_presence_seed": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "mgea_op_unpark_rows": (C.c_int, [_P, _P, _I32, _P]),
    "mgea_op_grammar_allow": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "mgea_op_row_budgets": (C.c_int, [C.POINTER(SamplerConfig), C.POINTER(RowSampler), _I32, _P, _I32, _I32, C.POINTER(RowSampler),
                                      C.POINTER(_I32), _P]),
}

_lib = None


def load():
    """Load libmgea_hip.so (after torch, so both share torch's libamdhip64.so.7 by SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C music-generation-emotion-adaptive_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads the HIP runtime the extension must share)
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def tune_get(name: str) -> int:
    v = _I32(0)
    check(load().mgea_tune_get(name.encode(), C.byref(v)))
    return int(v.value)


def tune_set(name: str, value: int) -> int:
    """Set an A/B switch of the native library (tools/README.md); returns the previous value."""
    old = tune_get(name)
    check(load().mgea_tune_set(name.encode(), int(value)))
    return old


def last_error() -> str:
    return (load().mgea_last_error() or b"").decode("utf-8", "replace")


def check(rc: int) -> int:
    """Map status codes to the exception classes the reference would raise."""
    if rc >= 0:
        return rc
    msg = last_error()
    if rc == EINVAL:
        # the reference's shape failures are torch RuntimeErrors (api_cache.py:99)
        raise RuntimeError(msg)
    if rc == ECAPACITY:
        raise ValueError(msg)
    if rc == ENOMEM:
        raise MemoryError(msg)
    raise MgeaError(f"[{rc}] {msg}")


def ptr(t) -> C.c_void_p:
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def stream_ptr(stream=None) -> C.c_void_p:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)
