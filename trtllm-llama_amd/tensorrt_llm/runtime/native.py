"""ctypes binding of include/tllm_runtime_api.h (the C++ host decode loop).

The reference's GenerationSession drives a TensorRT execution context from Python
(T/tensorrt_llm/runtime/generation.py:43-100); here the same object drives `tllm_session_*`.
torch tensors are handed over as raw device pointers (tensor handoff only)."""
import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from ..plugin import capi

_NP2C = {np.dtype(np.float32): capi.FLOAT, np.dtype(np.float16): capi.HALF, np.dtype(np.int8): capi.INT8,
         np.dtype(np.int32): capi.INT32, np.dtype(np.uint8): capi.INT8}

_bound = False


def _lib():
    global _bound
    lib = capi.load_library()
    if _bound:
        return lib
    c = ctypes
    lib.tllm_session_create.argtypes = [c.c_char_p]
    lib.tllm_session_create.restype = c.c_void_p
    lib.tllm_session_set_tensor.argtypes = [c.c_void_p, c.c_char_p, c.c_int32, c.POINTER(c.c_int64), c.c_int32,
                                            c.c_void_p, c.c_int32]
    lib.tllm_session_set_tensor.restype = c.c_int32
    lib.tllm_session_finalize.argtypes = [c.c_void_p]
    lib.tllm_session_finalize.restype = c.c_int32
    lib.tllm_session_load_engine.argtypes = [c.c_void_p, c.c_size_t]
    lib.tllm_session_load_engine.restype = c.c_void_p
    lib.tllm_session_load_engine_keys.argtypes = [c.c_void_p, c.c_size_t, c.c_char_p]
    lib.tllm_session_load_engine_keys.restype = c.c_void_p
    lib.tllm_session_setup.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_int32]
    lib.tllm_session_setup.restype = c.c_int32
    lib.tllm_session_setup_beam.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_int32]
    lib.tllm_session_setup_beam.restype = c.c_int32
    lib.tllm_session_get_beam_output.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_beam_output.restype = c.c_int32
    lib.tllm_session_get_beam_state.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_beam_state.restype = c.c_int32
    lib.tllm_session_logit_rows.argtypes = [c.c_void_p]
    lib.tllm_session_logit_rows.restype = c.c_int32
    lib.tllm_session_vocab_size.argtypes = [c.c_void_p]
    lib.tllm_session_vocab_size.restype = c.c_int32
    lib.tllm_session_generate.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int32, c.c_int32, c.c_int32,
                                          c.c_void_p, c.c_void_p]
    lib.tllm_session_generate.restype = c.c_int32
    lib.tllm_session_context.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_context.restype = c.c_int32
    lib.tllm_session_step.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_void_p]
    lib.tllm_session_step.restype = c.c_int32
    lib.tllm_session_fake_context.argtypes = [c.c_void_p, c.c_int32, c.c_uint32, c.c_void_p]
    lib.tllm_session_fake_context.restype = c.c_int32
    lib.tllm_session_get_logits.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_logits.restype = c.c_int32
    lib.tllm_session_get_output_ids.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_output_ids.restype = c.c_int32
    lib.tllm_session_kv_cache_ptr.argtypes = [c.c_void_p, c.c_int32]
    lib.tllm_session_kv_cache_ptr.restype = c.c_void_p
    lib.tllm_session_get_step_state.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_step_state.restype = c.c_int32
    lib.tllm_session_get_step_epoch.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_get_step_epoch.restype = c.c_int32
    lib.tllm_session_get_tap.argtypes = [c.c_void_p, c.c_int32, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.tllm_session_get_tap.restype = c.c_int32
    lib.tllm_session_get_tap_ex.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.tllm_session_get_tap_ex.restype = c.c_int32
    lib.tllm_session_force_tokens.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_force_tokens.restype = c.c_int32
    lib.tllm_session_step_bytes.argtypes = [c.c_void_p, c.c_int32]
    lib.tllm_session_step_bytes.restype = c.c_int64
    lib.tllm_session_profile.argtypes = [c.c_void_p, c.c_int32, c.POINTER(c.c_float), c.POINTER(c.c_int64), c.c_void_p]
    lib.tllm_session_profile.restype = c.c_int32
    lib.tllm_session_time_kernel.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.POINTER(c.c_float), c.POINTER(c.c_int64),
                                             c.c_void_p]
    lib.tllm_session_time_kernel.restype = c.c_int32
    lib.tllm_session_fused_retries.argtypes = [c.c_void_p]
    lib.tllm_session_fused_retries.restype = c.c_int32
    lib.tllm_session_decode_form.argtypes = [c.c_void_p]
    lib.tllm_session_decode_form.restype = c.c_int32
    lib.tllm_session_greedy_partials_used.argtypes = [c.c_void_p]
    lib.tllm_session_greedy_partials_used.restype = c.c_int64
    lib.tllm_session_destroy.argtypes = [c.c_void_p]
    lib.tllm_session_destroy.restype = None
    lib.tllm_session_set_sampling.argtypes = [c.c_void_p, c.POINTER(SamplingConfigC)]
    lib.tllm_session_set_sampling.restype = c.c_int32
    lib.tllm_sample_tokens.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_int32, c.POINTER(SamplingConfigC),
                                       c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p,
                                       c.c_void_p, c.c_void_p]
    lib.tllm_sample_tokens.restype = c.c_int32
    lib.tllm_session_score.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_score.restype = c.c_int32
    lib.tllm_token_logprobs.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p,
                                        c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_token_logprobs.restype = c.c_int32
    lib.tllm_session_append.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_session_append.restype = c.c_int32
    lib.tllm_session_append_generate.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_int32, c.c_void_p,
                                                 c.c_void_p]
    lib.tllm_session_append_generate.restype = c.c_int32
    lib.tllm_session_append_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_session_append_ragged.restype = c.c_int32
    lib.tllm_session_append_ragged_generate.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int32, c.c_int32, c.c_int32,
                                                        c.c_int32, c.c_void_p, c.c_void_p]
    lib.tllm_session_append_ragged_generate.restype = c.c_int32
    lib.tllm_attention_append_ragged.argtypes = [c.POINTER(AttentionAppendParamsC), c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_attention_append_ragged.restype = c.c_int32
    lib.tllm_session_append_launches.argtypes = [c.c_void_p, c.POINTER(c.c_int64), c.POINTER(c.c_int64)]
    lib.tllm_session_append_launches.restype = c.c_int32
    lib.tllm_attention_append.argtypes = [c.POINTER(AttentionAppendParamsC), c.c_void_p]
    lib.tllm_attention_append.restype = c.c_int32
    lib.tllm_attention_append_paged.argtypes = [c.POINTER(AttentionAppendParamsC), c.c_void_p, c.c_int32, c.c_int32, c.c_void_p,
                                                c.c_int32, c.c_void_p]
    lib.tllm_attention_append_paged.restype = c.c_int32
    lib.tllm_attention_append_layout.argtypes = [c.POINTER(AttentionAppendParamsC), c.POINTER(c.c_int32)]
    lib.tllm_attention_append_layout.restype = c.c_int32
    lib.tllm_session_verify.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_session_verify.restype = c.c_int32
    lib.tllm_session_verify_top1.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_session_verify_top1.restype = c.c_int32
    lib.tllm_session_generate_lookup.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int32, c.c_int32, c.c_int32,
                                                 c.POINTER(LookupConfigC), c.c_void_p, c.POINTER(LookupStatsC), c.c_void_p]
    lib.tllm_session_generate_lookup.restype = c.c_int32
    lib.tllm_spec_accept.argtypes = [c.POINTER(SpecAcceptParamsC), c.c_void_p]
    lib.tllm_spec_accept.restype = c.c_int32
    lib.tllm_prompt_lookup.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p,
                                       c.c_int32, c.c_int32, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_prompt_lookup.restype = c.c_int32
    lib.tllm_session_verify_sampled.argtypes = lib.tllm_session_verify.argtypes
    lib.tllm_session_verify_sampled.restype = c.c_int32
    lib.tllm_session_verify_draws.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_session_verify_draws.restype = c.c_int32
    lib.tllm_session_verify_logits.argtypes = [c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p]
    lib.tllm_session_verify_logits.restype = c.c_int32
    lib.tllm_session_generate_lookup_sampled.argtypes = lib.tllm_session_generate_lookup.argtypes
    lib.tllm_session_generate_lookup_sampled.restype = c.c_int32
    lib.tllm_spec_sample_rows.argtypes = [c.c_void_p, c.c_int32, c.c_int32, c.c_int32, c.c_int32, c.c_int32,
                                          c.POINTER(SamplingConfigC), c.c_int32, c.c_void_p, c.c_void_p, c.c_int32, c.c_void_p,
                                          c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    lib.tllm_spec_sample_rows.restype = c.c_int32
    lib.tllm_session_lora_set_tensor.argtypes = [c.c_void_p, c.c_int32, c.c_char_p, c.c_int32, c.POINTER(c.c_int64), c.c_int32,
                                                 c.c_void_p, c.c_int32]
    lib.tllm_session_lora_set_tensor.restype = c.c_int32
    lib.tllm_session_lora_commit.argtypes = [c.c_void_p, c.c_int32, c.c_float, c.c_int32]
    lib.tllm_session_lora_commit.restype = c.c_int32
    lib.tllm_session_lora_clear.argtypes = [c.c_void_p, c.c_int32]
    lib.tllm_session_lora_clear.restype = c.c_int32
    lib.tllm_session_lora_select.argtypes = [c.c_void_p, c.c_void_p]
    lib.tllm_session_lora_select.restype = c.c_int32
    lib.tllm_session_graph_captures.argtypes = [c.c_void_p]
    lib.tllm_session_graph_captures.restype = c.c_int64
    _bound = True
    return lib


VERIFY_MAX_TOKENS = 32  # TLLM_VERIFY_MAX_TOKENS


class LookupConfigC(ctypes.Structure):
    """tllm_lookup_config_t"""
    _fields_ = [('num_draft_tokens', ctypes.c_int32), ('max_ngram', ctypes.c_int32)]


class LookupStatsC(ctypes.Structure):
    """tllm_lookup_stats_t"""
    _fields_ = [(k, ctypes.c_int64) for k in ('rounds', 'verify_rounds', 'step_rounds', 'drafted', 'accepted')]


class GreedyParamsC(ctypes.Structure):
    """tllm_greedy_params_t"""
    _fields_ = [('logits', ctypes.c_void_p), ('batch', ctypes.c_int32), ('vocab_part', ctypes.c_int32), ('nparts', ctypes.c_int32),
                ('vocab', ctypes.c_int32), ('cur_ids', ctypes.c_void_p), ('out_ids', ctypes.c_void_p), ('out_stride', ctypes.c_int32),
                ('seq_len', ctypes.c_void_p), ('finished', ctypes.c_void_p), ('end_id', ctypes.c_int32), ('advance', ctypes.c_int32),
                ('rope_row_out', ctypes.c_void_p), ('rope_pos_out', ctypes.c_void_p), ('rope_table', ctypes.c_void_p),
                ('rope_half', ctypes.c_int32), ('rope_table_len', ctypes.c_int32), ('input_lengths', ctypes.c_void_p),
                ('max_input_len', ctypes.c_int32), ('emb_table', ctypes.c_void_p), ('x_out', ctypes.c_void_p),
                ('hidden', ctypes.c_int32), ('step_epoch', ctypes.c_void_p), ('argmax_part', ctypes.c_void_p)]


class SpecAcceptParamsC(ctypes.Structure):
    """tllm_spec_accept_params_t"""
    _fields_ = [('g', GreedyParamsC), ('n', ctypes.c_int32), ('ids', ctypes.c_void_p), ('top1', ctypes.c_void_p),
                ('limit', ctypes.c_void_p), ('accepted', ctypes.c_void_p), ('logits_out', ctypes.c_void_p)]


def spec_accept(ids, top1, *, logits, seq_len, finished, cur_ids, out_ids, end_id=-1, limit=None, accepted=None, logits_out=None,
                rope_row_out=None, rope_pos_out=None, rope_table=None, input_lengths=None, max_input_len=0, emb_table=None,
                x_out=None, step_epoch=None, vocab=None, stream: int = 0):
    """tllm_spec_accept on torch cuda tensors (the rule: csrc/kernels/kernels.h SpecAcceptParams, spec_ref.accept): ids, top1 int32
    [B, n]; logits f32 [B * n, vocab_part]; seq_len / finished / cur_ids / limit / accepted / input_lengths / rope_pos_out int32 [B];
    out_ids int32 [B, Smax]; logits_out f32 [B, vocab_part]; rope_table f32 [len, half, 2], rope_row_out f32 [B, half, 2]; emb_table
    fp16 [vocab, hidden], x_out fp16 [B, hidden]; step_epoch int32 / uint32 [>= 1].  The state tensors are updated in place."""
    B, n = ids.shape
    for t in (ids, top1, logits, seq_len, finished, cur_ids, out_ids, limit, accepted, logits_out, rope_row_out, rope_pos_out,
              rope_table, input_lengths, emb_table, x_out, step_epoch):
        assert t is None or (t.is_cuda and t.is_contiguous())
    ptr = lambda t: t.data_ptr() if t is not None else None
    g = GreedyParamsC(logits=ptr(logits), batch=B, vocab_part=logits.shape[-1], nparts=1, vocab=vocab or logits.shape[-1],
                      cur_ids=ptr(cur_ids), out_ids=ptr(out_ids), out_stride=out_ids.shape[1], seq_len=ptr(seq_len),
                      finished=ptr(finished), end_id=end_id, advance=0, rope_row_out=ptr(rope_row_out),
                      rope_pos_out=ptr(rope_pos_out), rope_table=ptr(rope_table),
                      rope_half=rope_table.shape[1] if rope_table is not None else 0,
                      rope_table_len=rope_table.shape[0] if rope_table is not None else 0, input_lengths=ptr(input_lengths),
                      max_input_len=max_input_len, emb_table=ptr(emb_table), x_out=ptr(x_out),
                      hidden=emb_table.shape[1] if emb_table is not None else 0, step_epoch=ptr(step_epoch), argmax_part=None)
    p = SpecAcceptParamsC(g=g, n=n, ids=ptr(ids), top1=ptr(top1), limit=ptr(limit), accepted=ptr(accepted),
                          logits_out=ptr(logits_out))
    _check(_lib().tllm_spec_accept(ctypes.byref(p), stream), 'spec_accept')


def prompt_lookup(out_ids, seq_len, n: int, max_ngram: int, *, max_input_len: int, vocab: int, input_lengths=None, finished=None,
                  limit=None, stream: int = 0):
    """tllm_prompt_lookup on torch cuda tensors (the rule: kernels.h PromptLookupParams, spec_ref.prompt_lookup): out_ids int32
    [B, Smax], seq_len / input_lengths / finished / limit int32 [B] -> (ids int32 [B, n], draft_len int32 [B])."""
    import torch
    B, smax = out_ids.shape
    for t in (out_ids, seq_len, input_lengths, finished, limit):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32)
    ptr = lambda t: t.data_ptr() if t is not None else None
    ids = torch.empty((B, n), dtype=torch.int32, device=out_ids.device)
    dl = torch.empty(B, dtype=torch.int32, device=out_ids.device)
    _check(_lib().tllm_prompt_lookup(out_ids.data_ptr(), B, smax, seq_len.data_ptr(), ptr(input_lengths), max_input_len,
                                     ptr(finished), ptr(limit), vocab, n, max_ngram, ids.data_ptr(), dl.data_ptr(), stream),
           'prompt_lookup')
    return ids, dl


class SamplingConfigC(ctypes.Structure):
    """tllm_sampling_config_t"""
    _fields_ = [('top_k', ctypes.c_int32), ('top_p', ctypes.c_float), ('temperature', ctypes.c_float),
                ('repetition_penalty', ctypes.c_float), ('presence_penalty', ctypes.c_float), ('min_length', ctypes.c_int32),
                ('random_seed', ctypes.c_uint64)]


class AttentionAppendParamsC(ctypes.Structure):
    """tllm_attention_append_params_t"""
    _fields_ = [('batch', ctypes.c_int32), ('n', ctypes.c_int32), ('num_heads', ctypes.c_int32), ('num_kv_heads', ctypes.c_int32),
                ('head_size', ctypes.c_int32), ('rotary_dim', ctypes.c_int32), ('neox', ctypes.c_int32), ('q_scaling', ctypes.c_float),
                ('kv_cache_type', ctypes.c_int32), ('max_seq_len', ctypes.c_int32), ('max_input_len', ctypes.c_int32),
                ('max_past', ctypes.c_int32), ('append_kernel', ctypes.c_int32), ('qkv', ctypes.c_void_p),
                ('kv_cache', ctypes.c_void_p), ('sequence_length', ctypes.c_void_p), ('input_lengths', ctypes.c_void_p),
                ('masked_tokens', ctypes.c_void_p), ('kv_scale_orig_quant', ctypes.c_void_p),
                ('kv_scale_quant_orig', ctypes.c_void_p), ('out', ctypes.c_void_p)]


APPEND_ATTN_WAVE, APPEND_ATTN_MFMA = 1, 2


def attention_append_kernel(n: int, head_size: int, append_kernel: int = 0) -> int:
    """the attention kernel tllm_attention_append would run (APPEND_ATTN_WAVE / APPEND_ATTN_MFMA); raises where a forced kind
    cannot run.  Needs no GPU."""
    p = AttentionAppendParamsC(n=int(n), head_size=int(head_size), append_kernel=int(append_kernel))
    kind = ctypes.c_int32()
    _check(_lib().tllm_attention_append_layout(ctypes.byref(p), ctypes.byref(kind)), 'attention_append_layout')
    return int(kind.value)


def attention_append(qkv, kv_cache, out, sequence_length, input_lengths, *, num_heads, num_kv_heads=0, head_size, max_input_len,
                     max_past=None, masked_tokens=None, kv_cache_type=0, kv_scale_orig_quant=None, kv_scale_quant_orig=None,
                     rotary_dim=None, neox=1, q_scaling=1.0, append_kernel=0, n_per_seq=None, max_end=None, stream: int = 0):
    """tllm_attention_append on torch cuda tensors: qkv fp16 [B, n, (H + 2 Hkv) * Dh] (q and k rewritten in place), kv_cache
    [B, 2, Hkv, Smax, Dh] fp16 / int8 / uint8, out fp16 [B, n, H * Dh], sequence_length / input_lengths int32 [B], masked_tokens
    int32 [B, Smax] or None, the two scales f32 [1] (one-byte caches; kv_cache_type capi.INT8 / capi.FP8).  Asynchronous.
    n_per_seq (int32 [B] on the device) with max_end >= every sequence_length[b] + n_per_seq[b]: tllm_attention_append_ragged -
    sequence b appends n_per_seq[b] of its n rows, max_past is ignored."""
    B, n = qkv.shape[0], qkv.shape[1]
    if (n_per_seq is None) != (max_end is None):
        raise ValueError('n_per_seq and max_end go together')
    if n_per_seq is None and max_past is None:
        raise ValueError('max_past must be given (or n_per_seq with max_end)')
    for t in (qkv, kv_cache, out, sequence_length, input_lengths, masked_tokens, kv_scale_orig_quant, kv_scale_quant_orig,
              n_per_seq):
        assert t is None or (t.is_cuda and t.is_contiguous())
    ptr = lambda t: t.data_ptr() if t is not None else None
    p = AttentionAppendParamsC(batch=B, n=n, num_heads=num_heads, num_kv_heads=num_kv_heads, head_size=head_size,
                               rotary_dim=head_size if rotary_dim is None else rotary_dim, neox=neox, q_scaling=q_scaling,
                               kv_cache_type=kv_cache_type, max_seq_len=kv_cache.shape[3], max_input_len=max_input_len,
                               max_past=max_past or 0, append_kernel=append_kernel, qkv=ptr(qkv), kv_cache=ptr(kv_cache),
                               sequence_length=ptr(sequence_length), input_lengths=ptr(input_lengths),
                               masked_tokens=ptr(masked_tokens), kv_scale_orig_quant=ptr(kv_scale_orig_quant),
                               kv_scale_quant_orig=ptr(kv_scale_quant_orig), out=ptr(out))
    if n_per_seq is None:
        _check(_lib().tllm_attention_append(ctypes.byref(p), stream), 'attention_append')
    else:
        assert str(n_per_seq.dtype) == 'torch.int32' and tuple(n_per_seq.shape) == (B, ), 'n_per_seq must be int32 [B]'
        _check(_lib().tllm_attention_append_ragged(ctypes.byref(p), n_per_seq.data_ptr(), int(max_end), stream),
               'attention_append_ragged')


def attention_append_paged(qkv, pool, block_pointers, out, sequence_length, input_lengths, *, tokens_per_block, max_seq_len,
                           num_heads, num_kv_heads=0, head_size, max_input_len, max_past=None, masked_tokens=None, kv_cache_type=0,
                           kv_scale_orig_quant=None, kv_scale_quant_orig=None, rotary_dim=None, neox=1, q_scaling=1.0,
                           append_kernel=0, n_per_seq=None, max_end=None, stream: int = 0):
    """tllm_attention_append_paged: attention_append on a paged cache.  pool is the memory the blocks [Hkv, tokens_per_block, Dh]
    live in (any shape), block_pointers int64 [B, 2, max_blocks_per_seq] on the device (K row, V row per sequence; 0 = a block that
    is not mapped), max_seq_len the capacity Smax the linear cache would have (masked_tokens is [B, Smax]).  Everything else, the
    ragged form (n_per_seq with max_end) included, as attention_append takes it."""
    B, n = qkv.shape[0], qkv.shape[1]
    if (n_per_seq is None) != (max_end is None):
        raise ValueError('n_per_seq and max_end go together')
    if n_per_seq is None and max_past is None:
        raise ValueError('max_past must be given (or n_per_seq with max_end)')
    for t in (qkv, pool, block_pointers, out, sequence_length, input_lengths, masked_tokens, kv_scale_orig_quant,
              kv_scale_quant_orig, n_per_seq):
        assert t is None or (t.is_cuda and t.is_contiguous())
    assert str(block_pointers.dtype) == 'torch.int64' and block_pointers.dim() == 3 and tuple(block_pointers.shape[:2]) == (B, 2), \
        'block_pointers must be int64 [B, 2, max_blocks_per_seq]'
    ptr = lambda t: t.data_ptr() if t is not None else None
    p = AttentionAppendParamsC(batch=B, n=n, num_heads=num_heads, num_kv_heads=num_kv_heads, head_size=head_size,
                               rotary_dim=head_size if rotary_dim is None else rotary_dim, neox=neox, q_scaling=q_scaling,
                               kv_cache_type=kv_cache_type, max_seq_len=int(max_seq_len), max_input_len=max_input_len,
                               max_past=max_past or 0, append_kernel=append_kernel, qkv=ptr(qkv), kv_cache=ptr(pool),
                               sequence_length=ptr(sequence_length), input_lengths=ptr(input_lengths),
                               masked_tokens=ptr(masked_tokens), kv_scale_orig_quant=ptr(kv_scale_orig_quant),
                               kv_scale_quant_orig=ptr(kv_scale_quant_orig), out=ptr(out))
    if n_per_seq is not None:
        assert str(n_per_seq.dtype) == 'torch.int32' and tuple(n_per_seq.shape) == (B, ), 'n_per_seq must be int32 [B]'
    _check(_lib().tllm_attention_append_paged(ctypes.byref(p), block_pointers.data_ptr(), int(tokens_per_block),
                                              int(block_pointers.shape[2]), ptr(n_per_seq), int(max_end or 0), stream),
           'attention_append_paged')


def _sampling_config(top_k=1, top_p=0.0, temperature=1.0, repetition_penalty=1.0, presence_penalty=0.0, min_length=1,
                     random_seed=0) -> SamplingConfigC:
    return SamplingConfigC(int(top_k), float(top_p), float(temperature), float(repetition_penalty), float(presence_penalty),
                           int(min_length), int(random_seed or 0) & 0xFFFFFFFFFFFFFFFF)


def sample_tokens(logits, g, out_ids, *, vocab=None, end_id=-1, history=None, input_lengths=None, max_input_len=0, u_out=None,
                  stream: int = 0, **config):
    """tllm_sample_tokens on torch cuda tensors: logits f32 [rows, vocab] or [nparts, rows, vocab_part] (then `vocab` = the
    real vocabulary size), g int32 [rows] (1-based number of the token drawn), out_ids int32 [rows]; history int32
    [rows, stride] and input_lengths int32 [rows] as the header describes; u_out optional f32 [rows].  **config: the fields of
    tllm_sampling_config_t.  Asynchronous on `stream`."""
    import torch
    if logits.dim() == 2:
        logits = logits.unsqueeze(0)
    nparts, rows, vpart = logits.shape
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32
    for t, n in ((g, rows), (out_ids, rows), (input_lengths, rows), (u_out, rows)):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() == n)
    for t in (g, out_ids, input_lengths, history):
        assert t is None or t.dtype == torch.int32
    assert u_out is None or u_out.dtype == torch.float32
    stride = 0
    if history is not None:
        assert history.is_cuda and history.is_contiguous() and history.dim() == 2 and history.shape[0] == rows
        stride = history.shape[1]
    ptr = lambda t: t.data_ptr() if t is not None else None
    cfg = _sampling_config(**config)
    _check(_lib().tllm_sample_tokens(logits.data_ptr(), nparts, rows, vpart, vocab or nparts * vpart, ctypes.byref(cfg), end_id,
                                     ptr(history), stride, ptr(input_lengths), max_input_len, g.data_ptr(), out_ids.data_ptr(),
                                     ptr(u_out), stream), 'sample_tokens')


def spec_sample_rows(logits, ids, seq_len, draws, *, max_input_len: int, vocab=None, end_id=-1, out_ids=None, input_lengths=None,
                     finished=None, limit=None, u_out=None, nparts: int = 1, stream: int = 0, **config):
    """tllm_spec_sample_rows on torch cuda tensors (the rule: csrc/kernels/kernels.h SpecSampleParams, spec_ref.sample_rows): the
    sampler on all n rows per sequence of a verify pass.  logits f32 [batch * n, vocab_part] (never written), ids int32
    [batch, n], seq_len / input_lengths / finished / limit int32 [batch], out_ids int32 [batch, Smax] the token record (needed
    with a penalty), draws int32 [batch, n], u_out optional f32 [batch, n].  **config: the fields of tllm_sampling_config_t.
    Asynchronous on `stream`."""
    import torch
    B, n = ids.shape
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32 and logits.dim() == 2
    assert logits.shape[0] == B * n
    for t, k in ((ids, B * n), (draws, B * n), (seq_len, B), (input_lengths, B), (finished, B), (limit, B)):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= k)
    assert u_out is None or (u_out.is_cuda and u_out.is_contiguous() and u_out.dtype == torch.float32 and u_out.numel() >= B * n)
    stride = 0
    if out_ids is not None:
        assert out_ids.is_cuda and out_ids.is_contiguous() and out_ids.dtype == torch.int32 and out_ids.shape[0] == B
        stride = out_ids.shape[1]
    ptr = lambda t: t.data_ptr() if t is not None else None
    cfg = _sampling_config(**config)
    vpart = logits.shape[1]
    _check(_lib().tllm_spec_sample_rows(logits.data_ptr(), nparts, B, n, vpart, vocab or vpart, ctypes.byref(cfg), end_id,
                                        ids.data_ptr(), ptr(out_ids), stride, seq_len.data_ptr(), ptr(input_lengths), max_input_len,
                                        ptr(finished), ptr(limit), draws.data_ptr(), ptr(u_out), stream), 'spec_sample_rows')


def token_logprobs(logits, targets, *, vocab=None, partials=None, stream: int = 0):
    """tllm_token_logprobs on torch cuda tensors: logits f32 [rows, vocab] or [nparts, rows, vocab_part] (then `vocab` = the real
    vocabulary size), targets int32 [rows] (-1 = no target) -> (log_probs f32 [rows], lse f32 [rows], top1_ids int32 [rows]).
    partials: optional f32 [nparts, rows, 8] that receives the per-part records.  Asynchronous on `stream`."""
    import torch
    if logits.dim() == 2:
        logits = logits.unsqueeze(0)
    nparts, rows, vpart = logits.shape
    assert logits.is_cuda and logits.is_contiguous() and logits.dtype == torch.float32
    assert targets.is_cuda and targets.is_contiguous() and targets.dtype == torch.int32 and targets.numel() == rows
    if partials is None:
        partials = torch.empty((nparts, rows, 8), dtype=torch.float32, device=logits.device)
    assert partials.is_cuda and partials.is_contiguous() and partials.dtype == torch.float32 and partials.numel() == nparts * rows * 8
    lp = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    top = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _check(_lib().tllm_token_logprobs(logits.data_ptr(), nparts, rows, vpart, vocab or nparts * vpart, targets.data_ptr(),
                                      partials.data_ptr(), lp.data_ptr(), lse.data_ptr(), top.data_ptr(), stream), 'token_logprobs')
    return lp, lse, top


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f'{what} failed: {capi.last_error()}')


class NativeSession:
    """Thin owner of a tllm_session_t."""

    def __init__(self, config: Optional[Dict] = None, engine: Optional[bytes] = None, runtime_keys: Optional[Dict] = None):
        """config: the session keys; or engine: a serialized engine, whose header holds them - then runtime_keys adds the keys
        that belong to the runtime and not to the engine (paged_append; tllm_session_load_engine_keys refuses every other)."""
        lib = _lib()
        self._keep = []  # torch tensors whose device memory the session references
        if engine is not None:
            buf = (ctypes.c_char * len(engine)).from_buffer_copy(engine)
            if runtime_keys:
                text = '\n'.join(f'{k}={v}' for k, v in runtime_keys.items())
                self._h = lib.tllm_session_load_engine_keys(buf, len(engine), text.encode())
            else:
                self._h = lib.tllm_session_load_engine(buf, len(engine))
        else:
            text = '\n'.join(f'{k}={v}' for k, v in config.items())
            self._h = lib.tllm_session_create(text.encode())
        if not self._h:
            raise RuntimeError(f'tllm_session create failed: {capi.last_error()}')
        self.batch = self.max_in = self.max_new = 0
        self.vocab = int(config['vocab_size']) if config else (int(lib.tllm_session_vocab_size(self._h)) or None)

    def set_tensor(self, name: str, t):
        lib = _lib()
        if isinstance(t, np.ndarray):
            a = np.ascontiguousarray(t)
            dims = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _check(lib.tllm_session_set_tensor(self._h, name.encode(), _NP2C[a.dtype], dims, a.ndim, a.ctypes.data, 0),
                   f'set_tensor({name})')
        else:  # torch cuda tensor: hand the device pointer over, keep the tensor alive
            import torch
            assert t.is_cuda and t.is_contiguous()
            code = {torch.float32: capi.FLOAT, torch.float16: capi.HALF, torch.int8: capi.INT8, torch.uint8: capi.INT8,
                    torch.int32: capi.INT32}[t.dtype]
            dims = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            _check(lib.tllm_session_set_tensor(self._h, name.encode(), code, dims, t.dim(), t.data_ptr(), 1),
                   f'set_tensor({name})')
            self._keep.append(t)

    def finalize(self):
        _check(_lib().tllm_session_finalize(self._h), 'finalize')

    def setup(self, batch: int, max_input_len: int, max_new_tokens: int, beam_width: int = 1):
        """batch prompts x beam_width hypotheses (beam search when > 1, beam_width <= 8; beyond 8 sequences the generation GEMVs run in slabs of 8 rows)."""
        _check(_lib().tllm_session_setup_beam(self._h, batch, beam_width, max_input_len, max_new_tokens), 'setup')
        self.batch, self.max_in, self.max_new, self.beam = batch, max_input_len, max_new_tokens, beam_width

    def lora_load(self, slot: int, tensors: Dict, alpha: float, use_rslora: bool = False):
        """One LoRA adapter into slot `slot` (session keys lora_max_rank / lora_max_adapters / lora_target_modules): tensors maps
        'layers.{i}.{attention.q|attention.k|attention.v|attention.dense|mlp.fc|mlp.gate|mlp.proj}.lora_a' to fp16 [r, K] and
        '.lora_b' to fp16 [N, r].  scale = alpha / r, alpha / sqrt(r) with use_rslora.  A refused adapter leaves the slot as it
        was."""
        lib = _lib()
        arrays = {name: np.ascontiguousarray(np.asarray(t), dtype=np.float16) for name, t in tensors.items()}
        for name, a in arrays.items():  # before anything is staged
            if a.ndim != 2 or a.size == 0:
                raise ValueError(f'lora_load: {name} is not a matrix (shape {a.shape})')
        for name, a in arrays.items():
            dims = (ctypes.c_int64 * 2)(*a.shape)
            _check(lib.tllm_session_lora_set_tensor(self._h, slot, name.encode(), capi.HALF, dims, 2, a.ctypes.data, 0),
                   f'lora_set_tensor({name})')
        _check(lib.tllm_session_lora_commit(self._h, slot, float(alpha), 1 if use_rslora else 0), 'lora_commit')

    def graph_captures(self) -> int:
        """step graphs captured since the session was created (one per capture, none per replay)"""
        return int(_lib().tllm_session_graph_captures(self._h))

    def lora_clear(self, slot: int):
        _check(_lib().tllm_session_lora_clear(self._h, slot), 'lora_clear')

    def lora_select(self, slots):
        """slots: one adapter slot per sequence, -1 = none; after setup(), holds until changed (all -1 after every setup).  Like
        lora_load() and lora_clear() it waits for the device to be idle first: work in flight on any stream finishes under the old
        selection."""
        sl = self._i32(slots)
        assert sl.shape == (self.batch, )
        _check(_lib().tllm_session_lora_select(self._h, sl.ctypes.data), 'lora_select')

    def set_sampling(self, config: Optional[Dict] = None, **fields):
        """Top-k / top-p sampling for the requests that follow (after setup(), before context() / generate(); beam_width 1):
        fields of tllm_sampling_config_t - top_k, top_p, temperature, repetition_penalty, presence_penalty, min_length,
        random_seed - as a dict or keywords.  set_sampling(None) with no fields returns to greedy."""
        fields = dict(config or {}, **fields)
        if config is None and not fields:
            _check(_lib().tllm_session_set_sampling(self._h, None), 'set_sampling')
            return
        cfg = _sampling_config(**fields)
        _check(_lib().tllm_session_set_sampling(self._h, ctypes.byref(cfg)), 'set_sampling')

    sample_tokens = staticmethod(sample_tokens)
    token_logprobs = staticmethod(token_logprobs)

    @staticmethod
    def _i32(a) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(a), dtype=np.int32)

    def context(self, input_ids, input_lengths, stream: int = 0):
        ids, lens = self._i32(input_ids), self._i32(input_lengths)
        assert ids.shape == (self.batch, self.max_in) and lens.shape == (self.batch, )
        _check(_lib().tllm_session_context(self._h, ids.ctypes.data, lens.ctypes.data, stream), 'context')

    def score(self, input_ids, input_lengths, stream: int = 0):
        """context() + the log-probability of every prompt token given the tokens before it (tllm_session_score):
        (log_probs f32 [batch, max_in], top1_ids int32 [batch, max_in]); 0 / -1 at t = 0 and behind a sequence's end.  The session
        is left as context() leaves it.  beam_width 1 only."""
        ids, lens = self._i32(input_ids), self._i32(input_lengths)
        assert ids.shape == (self.batch, self.max_in) and lens.shape == (self.batch, )
        lp = np.empty((self.batch, self.max_in), np.float32)
        top = np.empty((self.batch, self.max_in), np.int32)
        _check(_lib().tllm_session_score(self._h, ids.ctypes.data, lens.ctypes.data, lp.ctypes.data, top.ctypes.data, stream), 'score')
        return lp, top

    def step(self, n_steps: int = 1, use_graph: bool = False, stream: int = 0):
        _check(_lib().tllm_session_step(self._h, n_steps, 1 if use_graph else 0, stream), 'step')

    def fake_context(self, length: int, seed: int = 0, stream: int = 0):
        _check(_lib().tllm_session_fake_context(self._h, length, seed, stream), 'fake_context')

    def logits(self, vocab: Optional[int] = None, stream: int = 0) -> np.ndarray:
        v = vocab or self.vocab
        rows = _lib().tllm_session_logit_rows(self._h)  # batch after the prompt, batch * beam after a step
        out = np.empty((rows, v), np.float32)
        _check(_lib().tllm_session_get_logits(self._h, out.ctypes.data, stream), 'get_logits')
        return out

    def output_ids(self, stream: int = 0) -> np.ndarray:
        """Per-sequence token record [batch * beam, max_seq_len] (with beam search: the un-back-tracked step ids)."""
        out = np.empty((self.batch * self.beam, self.max_in + self.max_new), np.int32)
        _check(_lib().tllm_session_get_output_ids(self._h, out.ctypes.data, stream), 'get_output_ids')
        return out

    def beam_output(self, stream: int = 0):
        """(ids [batch, beam, max_seq_len] back-tracked and best first, cum_log_probs [batch, beam])."""
        out = np.empty((self.batch, self.beam, self.max_in + self.max_new), np.int32)
        cum = np.empty((self.batch, self.beam), np.float32)
        _check(_lib().tllm_session_get_beam_output(self._h, out.ctypes.data, cum.ctypes.data if self.beam > 1 else None, stream),
               'get_beam_output')
        return out, (cum if self.beam > 1 else None)

    def beam_state(self, stream: int = 0):
        """dict(parent_ids, cache_indirection [batch * beam, max_seq_len], finished, sequence_lengths [batch * beam])."""
        n, smax = self.batch * self.beam, self.max_in + self.max_new
        d = dict(parent_ids=np.empty((n, smax), np.int32), cache_indirection=np.empty((n, smax), np.int32),
                 finished=np.empty(n, np.int32), sequence_lengths=np.empty(n, np.int32))
        _check(_lib().tllm_session_get_beam_state(self._h, d['parent_ids'].ctypes.data, d['cache_indirection'].ctypes.data,
                                                  d['finished'].ctypes.data, d['sequence_lengths'].ctypes.data, stream),
               'get_beam_state')
        return d

    def generate(self, input_ids, input_lengths, max_new_tokens: int, end_id: int = -1, pad_id: int = 0,
                 stream: int = 0) -> np.ndarray:
        ids, lens = self._i32(input_ids), self._i32(input_lengths)
        shape = (self.batch, self.max_in + self.max_new) if self.beam == 1 else (self.batch, self.beam, self.max_in + self.max_new)
        out = np.empty(shape, np.int32)
        _check(_lib().tllm_session_generate(self._h, ids.ctypes.data, lens.ctypes.data, max_new_tokens, end_id, pad_id,
                                            out.ctypes.data, stream), 'generate')
        return out

    PROFILE_CLASSES = ('gemv_layer', 'gemv_head', 'attention', 'other', 'comm')

    def profile(self, n_steps: int, stream: int = 0):
        """{class: (total ms, launches)} over n_steps instrumented (eager) generation steps."""
        ms = (ctypes.c_float * 5)()
        cnt = (ctypes.c_int64 * 5)()
        _check(_lib().tllm_session_profile(self._h, n_steps, ms, cnt, stream), 'profile')
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(self.PROFILE_CLASSES)}

    LAYER_KERNELS = {'qkv': 1, 'attention': 2, 'o_proj': 4, 'gate_up': 5, 'down': 6, 'front': 7, 'mlp': 8}

    def fused_retries(self) -> int:
        """requests generate() repeated behind an expired in-launch wait of the one-launch projection + attention"""
        return int(_lib().tllm_session_fused_retries(self._h))

    def decode_form(self) -> int:
        """bit 0: QKV projection + attention in one launch, bit 1: + the O-projection stage, bit 2: the gated MLP in one launch"""
        return int(_lib().tllm_session_decode_form(self._h))

    def greedy_partials_used(self) -> int:
        """greedy-step launches enqueued with the lm_head launch's arg-max pairs since setup (a captured step counts once)"""
        return int(_lib().tllm_session_greedy_partials_used(self._h))

    def time_kernel(self, which: str, sweeps: int = 4, stream: int = 0):
        """(average microseconds per launch, launches) of one per-layer kernel launched back to back over all layers."""
        us = ctypes.c_float()
        n = ctypes.c_int64()
        _check(_lib().tllm_session_time_kernel(self._h, self.LAYER_KERNELS[which], sweeps, ctypes.byref(us),
                                               ctypes.byref(n), stream), 'time_kernel')
        return float(us.value), int(n.value)

    def kv_cache_ptr(self, layer: int) -> int:
        return _lib().tllm_session_kv_cache_ptr(self._h, layer)

    def step_state(self, stream: int = 0):
        """dict(sequence_length, next_position, input_lengths [batch * beam], masked_tokens [batch * beam, max_seq_len]): the
        device-resident counterparts of the per-step host tensors of the reference's decode loop."""
        n, smax = self.batch * self.beam, self.max_in + self.max_new
        d = dict(sequence_length=np.empty(n, np.int32), next_position=np.empty(n, np.int32),
                 masked_tokens=np.empty((n, smax), np.int32), input_lengths=np.empty(n, np.int32))
        _check(_lib().tllm_session_get_step_state(self._h, d['sequence_length'].ctypes.data, d['next_position'].ctypes.data,
                                                  d['masked_tokens'].ctypes.data, d['input_lengths'].ctypes.data, stream),
               'get_step_state')
        return d

    def step_epoch(self, stream: int = 0) -> int:
        """the device word the sampler advances once per generation step"""
        v = ctypes.c_uint32()
        _check(_lib().tllm_session_get_step_epoch(self._h, ctypes.byref(v), stream), 'get_step_epoch')
        return int(v.value)

    def force_tokens(self, ids, stream: int = 0):
        """teacher forcing: overwrite the token the last step chose (parity tests compare on identical prefixes)"""
        ids = self._i32(ids)
        assert ids.shape == (self.batch, )
        _check(_lib().tllm_session_force_tokens(self._h, ids.ctypes.data, stream), 'force_tokens')

    def _lengths(self, ids, lengths):
        lengths = self._i32(lengths)
        assert lengths.shape == (ids.shape[0], ), 'lengths must be [batch]'
        return lengths

    def append(self, ids, lengths=None, stream: int = 0):
        """Append ids [batch, n] to the live cache in one prefill pass (tllm_session_append): the parallel form of n times
        force_tokens(ids[:, i]); step(1).  Token 0 replaces the pending token (pass it as ids[:, 0] to keep it).  Afterwards
        logits() holds the last appended token's logits and a new pending token is chosen.  beam_width 1, tp 1; a paged cache with
        the session key paged_append = 1.
        lengths [batch] (tllm_session_append_ragged): sequence b appends ids[b, :lengths[b]] alone, 1 <= lengths[b] <= n; what
        stands behind them in the row is never read."""
        ids = self._i32(ids)
        assert ids.ndim == 2 and (not self.batch or ids.shape[0] == self.batch), 'ids must be [batch, n]'
        if lengths is None:
            _check(_lib().tllm_session_append(self._h, ids.ctypes.data, ids.shape[1], stream), 'append')
        else:
            lengths = self._lengths(ids, lengths)
            _check(_lib().tllm_session_append_ragged(self._h, ids.ctypes.data, lengths.ctypes.data, ids.shape[1], stream),
                   'append_ragged')

    def append_generate(self, ids, max_new_tokens: int, end_id: int = -1, pad_id: int = 0, stream: int = 0,
                        lengths=None) -> np.ndarray:
        """append(ids), then up to max_new_tokens generated tokens (tllm_session_append_generate): the token record
        [batch, max_seq_len], its unused tail filled as generate() fills it.  lengths as append()
        (tllm_session_append_ragged_generate): every sequence gets the same number of generation steps."""
        ids = self._i32(ids)
        assert ids.ndim == 2 and (not self.batch or ids.shape[0] == self.batch), 'ids must be [batch, n]'
        out = np.empty((self.batch, self.max_in + self.max_new), np.int32)
        if lengths is None:
            _check(_lib().tllm_session_append_generate(self._h, ids.ctypes.data, ids.shape[1], max_new_tokens, end_id, pad_id,
                                                       out.ctypes.data, stream), 'append_generate')
        else:
            lengths = self._lengths(ids, lengths)
            _check(_lib().tllm_session_append_ragged_generate(self._h, ids.ctypes.data, lengths.ctypes.data, ids.shape[1],
                                                              max_new_tokens, end_id, pad_id, out.ctypes.data, stream),
                   'append_ragged_generate')
        return out

    def append_launches(self):
        """(wave, mfma): attention launches append() has enqueued since setup, by kernel (one per layer and call)"""
        w, m = ctypes.c_int64(), ctypes.c_int64()
        _check(_lib().tllm_session_append_launches(self._h, ctypes.byref(w), ctypes.byref(m)), 'append_launches')
        return int(w.value), int(m.value)

    attention_append = staticmethod(attention_append)
    attention_append_paged = staticmethod(attention_append_paged)
    spec_accept = staticmethod(spec_accept)
    prompt_lookup = staticmethod(prompt_lookup)
    spec_sample_rows = staticmethod(spec_sample_rows)

    def verify(self, ids, sampled: bool = False, stream: int = 0):
        """Verify ids [batch, n] in one append pass (tllm_session_verify): ids[:, 0] takes the pending token's place, ids[:, 1:] are
        drafts; the longest prefix greedy decoding would have produced is kept.  Returns (accepted int32 [batch]: drafts kept, -1 for
        a finished sequence; log_probs f32 [batch, n]: log p(ids[b][i] | everything before it), 0 at i = 0).  logits() then holds
        the row behind the last kept token and the arg-max of that row is the new pending token.
        sampled=True (tllm_session_verify_sampled): under the configuration of set_sampling() a draft is kept only where it equals
        the token the sampler draws there, the draw behind the last kept draft is the new pending token; log_probs stay the raw
        model's.  With a greedy configuration the two are the same call."""
        ids = self._i32(ids)
        assert ids.ndim == 2 and (not self.batch or ids.shape[0] == self.batch), 'ids must be [batch, n]'
        acc = np.empty(ids.shape[0], np.int32)
        lp = np.empty(ids.shape, np.float32)
        fn = _lib().tllm_session_verify_sampled if sampled else _lib().tllm_session_verify
        _check(fn(self._h, ids.ctypes.data, ids.shape[1], acc.ctypes.data, lp.ctypes.data, stream),
               'verify_sampled' if sampled else 'verify')
        return acc, lp

    def verify_draws(self, n: int, stream: int = 0) -> np.ndarray:
        """the ids [batch, n] the last verify() of n ids compared the drafts with: the sampler's draws after a sampled pass, the
        arg-maxes after a greedy one (tests)"""
        d = np.empty((self.batch, n), np.int32)
        _check(_lib().tllm_session_verify_draws(self._h, d.ctypes.data, n, stream), 'verify_draws')
        return d

    def verify_logits(self, n: int, vocab: Optional[int] = None, stream: int = 0) -> np.ndarray:
        """the fp32 logits rows [batch, n, vocab] of the last verify() of n ids (tests)"""
        v = _lib().tllm_session_vocab_size(self._h)
        assert vocab is None or vocab == v
        out = np.empty((self.batch, n, v), np.float32)
        _check(_lib().tllm_session_verify_logits(self._h, out.ctypes.data, n, stream), 'verify_logits')
        return out

    def verify_top1(self, n: int, stream: int = 0) -> np.ndarray:
        """the arg-max ids [batch, n] of the logits rows of the last verify() of n ids (tests)"""
        top = np.empty((self.batch, n), np.int32)
        _check(_lib().tllm_session_verify_top1(self._h, top.ctypes.data, n, stream), 'verify_top1')
        return top

    def generate_lookup(self, input_ids, input_lengths, max_new_tokens: int, end_id: int = -1, pad_id: int = 0,
                        num_draft_tokens: int = 8, max_ngram: int = 3, sampled: bool = False, stream: int = 0):
        """generate() with prompt-lookup drafts verified num_draft_tokens ids at a time (tllm_session_generate_lookup): the same
        tokens.  max_new_tokens + num_draft_tokens <= setup's max_new_tokens.  Returns (output_ids [batch, max_seq_len], stats:
        dict(rounds, verify_rounds, step_rounds, drafted, accepted)).  sampled=True (tllm_session_generate_lookup_sampled): under
        the configuration of set_sampling(), the tokens generate() yields for that configuration and seed."""
        ids, lens = self._i32(input_ids), self._i32(input_lengths)
        out = np.empty((self.batch, self.max_in + self.max_new), np.int32)
        cfg, st = LookupConfigC(int(num_draft_tokens), int(max_ngram)), LookupStatsC()
        fn = _lib().tllm_session_generate_lookup_sampled if sampled else _lib().tllm_session_generate_lookup
        _check(fn(self._h, ids.ctypes.data, lens.ctypes.data, max_new_tokens, end_id, pad_id, ctypes.byref(cfg), out.ctypes.data,
                  ctypes.byref(st), stream), 'generate_lookup_sampled' if sampled else 'generate_lookup')
        return out, {k: int(getattr(st, k)) for k, _ in LookupStatsC._fields_}

    def attention_tap(self, layer: int, heads_x_dh: int, quantised: bool, stream: int = 0) -> np.ndarray:
        """O-projection input of the last generation step (debug_taps=1): [batch * beam, H/tp * Dh] fp16, int8 for SmoothQuant."""
        out = np.empty((self.batch * self.beam, heads_x_dh), np.int8 if quantised else np.float16)
        _check(_lib().tllm_session_get_tap(self._h, layer, out.ctypes.data, out.nbytes, stream), 'get_tap')
        return out

    TAPS = {'qkv_in': 0, 'o_in': 1, 'mlp_in': 2, 'proj_in': 3, 'x_in': 4}

    def tap(self, layer: int, which: str, width: int, quantised: bool, stream: int = 0) -> np.ndarray:
        """Input of one of the layer's four GEMMs in the last generation step, behind its prologue (debug_taps=1):
        [batch * beam, width] fp16, int8 for SmoothQuant (the output of that GEMM's activation quantiser)."""
        out = np.empty((self.batch * self.beam, width), np.int8 if (quantised and which != 'x_in') else np.float16)
        _check(_lib().tllm_session_get_tap_ex(self._h, layer, self.TAPS[which], out.ctypes.data, out.nbytes, stream), 'get_tap_ex')
        return out

    def step_bytes(self, context_len: int) -> int:
        return _lib().tllm_session_step_bytes(self._h, context_len)

    def close(self):
        if getattr(self, '_h', None):
            _lib().tllm_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
