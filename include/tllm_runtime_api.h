/*
 * tllm_runtime_api.h — host decode loop of the MI355X LLaMA path behind a C ABI.
 *
 * Takes the place of the TensorRT engine + execution context that the reference's runtime drives
 * (T/tensorrt_llm/runtime/generation.py:43-100 `_Runtime`, :413-488 `setup`, :782-997 `decode`) and of the
 * C++ GptSession host loop (T/cpp/tensorrt_llm/runtime/gptSession.cpp:252,700).  The Python front-end
 * (tensorrt_llm.runtime.GenerationSession) keeps its reference signature and calls these entry points;
 * PyTorch is only used to own device buffers that are handed in as raw pointers.
 *
 * An "engine" here is: a text configuration (key=value lines, the builder_config / plugin_config of
 * config.json, T/tensorrt_llm/builder.py:259-267) plus named weight tensors (module paths of the reference's
 * LLaMAForCausalLM, T/examples/llama_quant/llama_model.py:122-251).  Execution = the plugin kernels of
 * tllm_plugin_api.h enqueued layer by layer on one HIP stream; the generation step is fused
 * (RMSNorm / quantisation / SwiGLU / residual folded into the GEMV launches) and replayed as a hipGraph.
 */
#ifndef TLLM_RUNTIME_API_H
#define TLLM_RUNTIME_API_H

#include "tllm_plugin_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tllm_session* tllm_session_t;

/* Create a session from a configuration text.  Recognised keys (defaults in parentheses):
 *   num_layers, num_heads, hidden_size, inter_size, vocab_size, max_position_embeddings (2048),
 *   num_kv_heads (num_heads; grouped-query attention: Hkv K/V heads, query head h reads K/V head h / (num_heads / Hkv); the
 *   attention.qkv weight is [(H + 2 Hkv) Dh / tp, hidden] in the block order q | k | v, the cache [B, 2, Hkv / tp, Smax, Dh]; refused
 *   with an error naming the key when it does not divide num_heads, when tp_size does not divide it, or with SmoothQuant
 *   weights; a session with Hkv != num_heads runs the separate-launch generation step),
 *   rms_norm_eps (1e-6), tp_size (1), tp_rank (0), quant_mode (0: QuantMode bits,
 *   T/tensorrt_llm/quantization/mode.py:6-21; bit 32 = int8 KV cache, bit 64 = fp8 (OCP E4M3) KV cache: one-byte cache
 *   elements and the two attention.kv_*_scale tensors per layer either way, the two bits are exclusive and an fp8 session runs
 *   the separate-launch generation step), weight_only_precision (int8|int4),
 *   use_gpt_attention_plugin/use_gemm_plugin (informational), neox_rotary_style (1),
 *   force_comm (0; tests: issue the tensor-parallel collectives on a 1-rank communicator as well),
 *   remove_input_padding (0; 1: the context phase runs on the packed real tokens only),
 *   paged_kv_cache (0; 1: every layer's cache is a pool of [Hr, tokens_per_block, Dh] blocks reached through a per-sequence
 *   table of block pointers - K/kvCacheUtils.h:34-112, PY/runtime/kv_cache_manager.py; the table is filled at setup),
 *   tokens_per_block (64; a power of two),
 *   paged_append (0; 1, with paged_kv_cache = 1 only - refused by name otherwise: tllm_session_append, _append_ragged, their
 *   _generate forms, tllm_session_verify, _verify_sampled and both tllm_session_generate_lookup loops, LoRA included, serve the
 *   paged cache through its table, bit for bit what the linear session computes; without the key a paged session refuses them
 *   as before.  A key of the runtime, not of the engine header: tllm_session_load_engine_keys adds it to a loaded engine),
 *   debug_taps (0; 1: keep per-layer intermediates of the generation step for tllm_session_get_tap),
 *   gemm_tactics (optional; the table tllm_gemm_tactics_export wrote, as the builder stores it in the engine).
 * Returns NULL on error (tllm_last_error()). */
tllm_session_t tllm_session_create(const char* config_text);

/* Register one weight tensor by module path, e.g. "layers.3.attention.qkv.weight", "vocab_embedding.weight",
 * "ln_f.weight", "lm_head.weight" (reference attribute names, T/examples/llama_quant/weight_quant.py:172-446).
 *   location 0: `data` is a HOST pointer, the bytes are copied to device memory owned by the session;
 *   location 1: `data` is a DEVICE pointer that outlives the session (tensor handoff from torch). */
int32_t tllm_session_set_tensor(tllm_session_t s, const char* name, int32_t dtype, const int64_t* dims, int32_t nbDims,
    const void* data, int32_t location);

/* Resolve the weights against the configuration; fails listing the first missing / mis-shaped tensor. */
int32_t tllm_session_finalize(tllm_session_t s);

/* Parse a serialized engine (format written by tensorrt_llm.Builder.build_engine: "TLLMENG1" header, config
 * text, tensor table, data) = tllm_engine_verify + create + set_tensor(location 0) + finalize. */
tllm_session_t tllm_session_load_engine(const void* engine, size_t nbytes);
/* The same with session keys of the runtime behind the header's: runtime_keys is "key=value" lines (NULL or empty: none).  Only
 * the keys that are not the engine's to decide are taken - paged_append - and any other line is refused by name, so nothing the
 * engine was built and verified with can be overridden here. */
tllm_session_t tllm_session_load_engine_keys(const void* engine, size_t nbytes, const char* runtime_keys);

/* The check tllm_session_load_engine applies before it accepts an engine, on its own (host only, no GPU needed): the traced
 * network the engine carries (`network_json`: plugin nodes in order, their inputs, fields and the weights feeding them, the
 * I/O tensor names of T/tensorrt_llm/runtime/generation.py:188-208) must be exactly the LLaMA schedule the session executes
 * for the engine's configuration - "the engine is what was defined" (T/tensorrt_llm/builder.py:259-267).  A model
 * definition that was edited (another plugin, another field value, another weight on a port, a node more or less) is
 * refused with an error naming the first node that differs.  0 = accepted. */
int32_t tllm_engine_verify(const void* engine, size_t nbytes);

/* GenerationSession.setup (generation.py:413-488): allocates the per-layer KV cache
 * [B, 2, H/tp, max_input_len + max_new_tokens, Dh] (fp16 or int8), activations and the RoPE table. */
int32_t tllm_session_setup(tllm_session_t s, int32_t batch_size, int32_t max_input_len, int32_t max_new_tokens);

/* The same with beam search (SamplingConfig.num_beams > 1, generation.py:365-411, 823-866): batch_size prompts, beam_width
 * hypotheses each (1 <= beam_width <= 8; batch_size * beam_width is not limited: the generation GEMVs take 8 rows per launch and
 * run more sequences in slabs of 8, each slab streaming the weights again).  The KV cache holds
 * batch_size * beam_width sequences; the prompt's K/V is stored once per batch entry (in hypothesis 0's rows) and reached by
 * the others through the cache indirection [batch_size * beam_width, max_seq_len] (value = sibling hypothesis whose rows
 * hold that time step), which the device-side beam step re-parents every step - the reference's src/tgt
 * cache_indirection pair (gptAttention plugin input, decoderMaskedMultiheadAttentionTemplate.h:1137-1146) in one buffer.
 * Selection rule of the reference's dynamic decoder without beam_hyps (onlineSoftmaxBeamsearchKernels.cu): the
 * beam_width best cum_log_prob + log_softmax(logits) over (hypothesis, token); a finished hypothesis continues with
 * end_id at unchanged score.  tllm_session_generate then returns [batch_size, beam_width, max_seq_len]. */
int32_t tllm_session_setup_beam(tllm_session_t s, int32_t batch_size, int32_t beam_width, int32_t max_input_len,
    int32_t max_new_tokens);

/* gather_tree (decodingKernels.cu:30-171; generation.py:990-994): ids HOST int32 [batch_size, beam_width, max_seq_len], the
 * back-tracked hypotheses, best first; cum_log_probs HOST float [batch_size, beam_width] or NULL.  After the first end_id
 * and beyond the current length the row is filled with end_id.  With beam_width 1 it is tllm_session_get_output_ids. */
int32_t tllm_session_get_beam_output(tllm_session_t s, int32_t* ids, float* cum_log_probs, tllm_stream_t stream);

/* The device-side beam bookkeeping, for tests and debugging (any pointer may be NULL): parent_ids and cache_indirection
 * HOST int32 [batch_size * beam_width, max_seq_len] (generation.py:387-391, 823-837), finished and sequence_lengths
 * HOST int32 [batch_size * beam_width]. */
int32_t tllm_session_get_beam_state(tllm_session_t s, int32_t* parent_ids, int32_t* cache_indirection, int32_t* finished,
    int32_t* sequence_lengths, tllm_stream_t stream);

/* Rows the last logits hold (tllm_session_get_logits): batch_size after the prompt, batch_size * beam_width after a step. */
int32_t tllm_session_logit_rows(tllm_session_t s);

/* Vocabulary size of the model the session holds (the width of a logits row; the reference reads it from the engine's `logits`
 * binding, runtime/session.py:116-145 infer_shapes). */
int32_t tllm_session_vocab_size(tllm_session_t s);

/* GenerationSession.decode (generation.py:782-997), greedy (top-k = 1): context step on the padded prompts,
 * then up to max_new_tokens generation steps with the sampler on device and no per-step host sync
 * (the reference syncs every step, generation.py:963).
 *   input_ids     HOST int32 [B, max_input_len] (padded with pad_id), input_lengths HOST int32 [B];
 *   output_ids    HOST int32 [B, max_input_len + max_new_tokens]: the prompt followed by the generated ids;
 *   end_id < 0 disables early stopping (benchmarks).  Blocks until the ids are on the host. */
int32_t tllm_session_generate(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream);

/* Step-wise interface (parity tests, benchmarks):
 *   context: runs the prompt, leaves the fp32 logits of the last real token of every sequence in the session;
 *   step:    runs `n_steps` generation steps (greedy feedback on device); timing is the caller's business.
 *   use_graph != 0 replays the captured generation step. */
int32_t tllm_session_context(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    tllm_stream_t stream);
int32_t tllm_session_step(tllm_session_t s, int32_t n_steps, int32_t use_graph, tllm_stream_t stream);
/* tllm_session_context + the log-probability of every prompt token given the tokens before it.
 *   log_probs HOST float [B, max_input_len]: log_probs[b][t] = log softmax(logits after ids[b][0..t-1])[ids[b][t]] for
 *             1 <= t < input_lengths[b]; 0 at t = 0 and at t >= input_lengths[b];
 *   top1_ids  HOST int32 [B, max_input_len] or NULL: the arg-max of that same distribution (ties -> lowest id); -1 where log_probs is 0 by definition.
 * Leaves the session in exactly the state tllm_session_context leaves it in (cache, last-token logits, first sampled token, step state):
 * generation can continue from it.  beam_width 1 only.  Synchronises the stream.
 * The final hidden rows that have a next token go through ln_f and lm_head in chunks of rows (fp32 logits of one chunk at a
 * time: as many rows as fit 64 MiB, a multiple of 32; session key score_chunk_rows overrides) and a streaming kernel reduces
 * every row to (log-sum-exp, target logit, arg-max): the [tokens, vocab] logits never reach the host.  Tensor parallel: every
 * rank reduces its own vocabulary shard, the 32-byte records are all-gathered and merged; every rank returns the same values.
 * A token id outside [0, vocab_size) scores 0.  The buffers are allocated by the first call after a setup. */
int32_t tllm_session_score(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths, float* log_probs,
    int32_t* top1_ids, tllm_stream_t stream);
/* Fill the KV cache for `length` positions with pseudo-random content (as a prompt of that length would)
 * without running a prefill; for decode-rate benchmarks at a given context length. */
int32_t tllm_session_fake_context(tllm_session_t s, int32_t length, uint32_t seed, tllm_stream_t stream);
/* Copy state to HOST buffers (synchronises the stream). */
int32_t tllm_session_get_logits(tllm_session_t s, float* logits /* [B, vocab] */, tllm_stream_t stream);
int32_t tllm_session_get_output_ids(tllm_session_t s, int32_t* ids /* [B, max_in + max_new] */, tllm_stream_t stream);
/* Device pointer of a layer's KV cache (layout [B,2,H/tp,Smax,Dh]) for inspection. */
void* tllm_session_kv_cache_ptr(tllm_session_t s, int32_t layer);
/* Diagnostic: with the session key fused_timeline = 1, the device buffer [heads * 8 workgroups][16] of 100 MHz clock ticks the
 * last fused QKV-projection + attention launch stamped at its stages (kernels/qkv_attn_fused.hip; tools/fused_timeline.py);
 * NULL when the session does not run that launch. */
void* tllm_session_fused_timeline_ptr(tllm_session_t s);
/* ... and of the last one-launch MLP ([256 workgroups][16]; kernels/mlp_fused.hip). */
void* tllm_session_mlp_timeline_ptr(tllm_session_t s);
/* The step-dependent tensors the reference's Python loop builds on the host every step (PY/runtime/generation.py:556-579,
 * :686-689, :735-750, :812-821) live in device memory here and are advanced by the sampler kernel; this copies them out so
 * that tests can pin them to the reference's values (any pointer may be NULL):
 *   sequence_length [B]        cache slots in use = the reference's `sequence_length` / `past_key_value_length[0]` input of
 *                              the NEXT generation step (max_input_len + step);
 *   next_position   [B]        rotary position of the token the next step consumes = the reference's `position_ids` of that
 *                              step (input_lengths + step);
 *   masked_tokens   [B, Smax]  1 on the padding slots [input_lengths[b], max_input_len);
 *   input_lengths   [B]. */
int32_t tllm_session_get_step_state(tllm_session_t s, int32_t* sequence_length, int32_t* next_position, int32_t* masked_tokens,
    int32_t* input_lengths, tllm_stream_t stream);

/* The device word the sampler advances once per generation step (the tags of the in-launch hand-offs derive from it): zero after
 * tllm_session_setup's allocation, + 1 per step whichever sampler runs it.  For tests. */
int32_t tllm_session_get_step_epoch(tllm_session_t s, uint32_t* epoch, tllm_stream_t stream);

/* Teacher forcing for parity tests (greedy sessions): replace the token the last context / generation step chose by ids[b]
 * (host, [B]) - in the output buffer, as the next step's input id and as its input embedding row - so that two
 * implementations can be compared step by step on the SAME prefix (the reference's tests feed HF's tokens the same way,
 * T/tests/model/test_llama.py:300-354).  Does not touch the KV cache or the step counters. */
int32_t tllm_session_force_tokens(tllm_session_t s, const int32_t* ids, tllm_stream_t stream);

/* Append n tokens per sequence to the live cache in ONE prefill pass (multi-turn chat, chunked prefill, verification of n known
 * tokens): the parallel form of  for i < n: tllm_session_force_tokens(ids[:, i]); tllm_session_step(1).
 *   ids  HOST int32 [B, n].
 * With p_b = sequence_length[b]: appended token i replaces (i = 0) or extends from the pending token the last sampler chose - it
 * occupies output slot and cache slot p_b + i at rotary position p_b + i - (max_input_len - input_lengths[b]) and sees every
 * unmasked slot < p_b plus the appended tokens 0 .. i (kernels/append_attn.hip; DESIGN.md section 7c states the numeric rule).
 * A caller who wants the model's own pending token kept passes it as ids[:, 0].  Afterwards: sequence_length += n, finished = 0,
 * the fp32 logits of the last appended token are in the session (tllm_session_get_logits), and the sampler (greedy or the
 * configured one) has chosen a new pending token and prepared the next step's RoPE row and input row exactly as after
 * tllm_session_context; masked_tokens and input_lengths are unchanged; a captured step graph stays valid (it reads device state
 * only).  The pass is the prefill schedule on B * n rows with the append attention in place of the context attention.
 * Reads sequence_length back, so it synchronises the stream.  Refused, with nothing enqueued: before setup; before any context
 * (every sequence_length must be >= max_input_len); n < 1, n > max_input_len (the activation buffers are sized for that) or
 * sequence_length[b] + n > max_seq_len; beam_width > 1, tensor parallel > 1, the paged cache without the session key paged_append;
 * a token id outside [0, vocab_size).
 * Packed-input sessions are accepted (the appended rows are dense either way), and paged sessions with paged_append = 1 (the
 * attention reaches the cache through the block table; every result is the linear session's).  A different n per sequence: tllm_session_append_ragged.  The
 * scoring of the appended tokens is tllm_session_verify's. */
int32_t tllm_session_append(tllm_session_t s, const int32_t* ids, int32_t n, tllm_stream_t stream);
/* tllm_session_append, then up to max_new_tokens generated tokens as tllm_session_generate produces them (the first by the
 * append's sampler launch, the rest by generation steps from the graph, the finished flags polled every 32 steps).
 *   output_ids  HOST int32 [B, max_seq_len]: the session's token record; from slot sequence_length[b] + n + (tokens produced) on,
 *               and behind a sequence's first end_id among the new tokens, the row is filled with end_id (pad_id when end_id < 0).
 * max_new_tokens >= 1 and sequence_length[b] + n + max_new_tokens <= max_seq_len.  When a bounded wait of the one-launch step
 * expires, the call fails and the error says that the session's results are invalid: unlike tllm_session_generate it cannot
 * repeat the request, because the append has consumed the state it started from. */
int32_t tllm_session_append_generate(tllm_session_t s, const int32_t* ids, int32_t n, int32_t max_new_tokens, int32_t end_id,
    int32_t pad_id, int32_t* output_ids, tllm_stream_t stream);
/* tllm_session_append with a different number of tokens per sequence, in the padded layout
 *   ids      HOST int32 [B, W];   lengths  HOST int32 [B], 1 <= lengths[b] <= W <= max_input_len.
 * For sequence b the call is tllm_session_append with n = n_b = lengths[b]: placement, RoPE position, visibility, numerics and the
 * store rule are that entry's with n_b in place of n.  Only ids[b][0 .. n_b) are read - what stands behind them in a row is never
 * looked at, range-checked or copied into the token record.  The cache is written in slots [p_b, p_b + n_b) alone, the token
 * record in [p_b, p_b + n_b] (its last slot by the sampler), sequence_length[b] += n_b, finished[b] = 0, and the session's logits
 * row b belongs to appended token n_b - 1.  The pass runs on B * N rows, N = max_b n_b (not W), and N chooses the attention kernel;
 * rows i >= n_b are padding that nothing outliving the call depends on.  With every n_b = W the call is tllm_session_append bit
 * for bit.  Refused, with nothing enqueued: everything tllm_session_append refuses, with the capacity check per sequence
 * (sequence_length[b] + n_b > max_seq_len); lengths NULL; an n_b < 1 or > W; an id outside [0, vocab_size) among the first n_b of a
 * row.  Not built: a sequence that sits the call out (n_b = 0); a packed row layout (sum of n_b rows). */
int32_t tllm_session_append_ragged(tllm_session_t s, const int32_t* ids, const int32_t* lengths, int32_t W, tllm_stream_t stream);
/* tllm_session_append_ragged, then tllm_session_append_generate from there: every sequence gets the same number of generation
 * steps, sequence_length[b] + n_b + max_new_tokens <= max_seq_len per sequence, and the tail fill of output_ids starts behind
 * sequence_length[b] + n_b + (tokens produced).  The failure contract for an expired in-launch wait is
 * tllm_session_append_generate's. */
int32_t tllm_session_append_ragged_generate(tllm_session_t s, const int32_t* ids, const int32_t* lengths, int32_t W,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream);
/* Attention launches tllm_session_append and tllm_session_append_ragged have enqueued since setup, by kernel (one per layer and
 * call): *wave, *mfma (either may be NULL).  For tests: which kernel served a chunk. */
int32_t tllm_session_append_launches(tllm_session_t s, int64_t* wave, int64_t* mfma);

/* Speculative greedy decoding (the rules are stated in csrc/kernels/kernels.h, SpecAcceptParams and
 * PromptLookupParams, and restated in numpy in tensorrt_llm/runtime/spec_ref.py).  Opt-in: tllm_session_generate, the step graph
 * and the append are what they were.
 *
 * Verify n ids per sequence in ONE append pass and keep the longest prefix plain greedy decoding would have produced.
 *   ids        HOST int32 [B, n]: ids[b][0] takes the pending token's place (pass the pending token itself to keep it), ids[b][1..]
 *              are drafts of the tokens behind it;
 *   accepted   HOST int32 [B]: m_b, the number of drafts kept; -1 for a frozen sequence (finished: nothing of it changes);
 *   log_probs  HOST float [B, n] or NULL: log_probs[b][i] = log softmax(logits row i - 1)[ids[b][i]] for 1 <= i < n, 0 at i = 0 - the
 *              scoring of the appended tokens, whether they were kept or not.
 * The pass is tllm_session_append's with the head on all B * n rows (fp32, on the device); row i of a sequence is the distribution
 * behind ids[b][0..i], a_i its arg-max (ties: lowest id).  With p = sequence_length[b]:
 *   m = 0; while (m + 1 < n && a[m] != end_id && ids[b][m + 1] == a[m]) ++m;
 *   output slots p .. p + m = ids[b][0..m], slot p + m + 1 = a[m] (the new pending token), sequence_length[b] = p + m + 1,
 *   finished[b] |= a[m] == end_id; the next step's RoPE row and input row as every sampler launch leaves them.
 * Afterwards tllm_session_get_logits returns row m_b of every sequence and generation continues by step, append or another verify.
 * The cache rows of the rejected drafts stay behind the sequence length, where no launch reads them, and are overwritten by the
 * next tokens.  end_id is the session's (the last tllm_session_generate* call's; -1 after setup).  Synchronises the stream.
 * Refused, with nothing enqueued: everything tllm_session_append refuses; n > TLLM_VERIFY_MAX_TOKENS;
 * sequence_length[b] + n + 1 > max_seq_len; a sampling configuration that is not plain arg-max (speculative sampling is not built
 * into this entry: tllm_session_verify_sampled below takes it).
 * Not built: a draft model with a soft distribution q and the rejection rule's residual distribution (speculative sampling is
 * by exact match with the draw, below), a different n per sequence, beam / tensor-parallel sessions (a paged session: key paged_append), a verify pass in
 * the one-launch form of the generation step. */
#define TLLM_VERIFY_MAX_TOKENS 32
int32_t tllm_session_verify(tllm_session_t s, const int32_t* ids, int32_t n, int32_t* accepted, float* log_probs,
    tllm_stream_t stream);
/* For tests: the arg-max ids a[b][i] of the n logits rows per sequence of the last verify pass, HOST int32 [B, n] (n as that
 * pass's; refused before any verify pass).  Synchronises the stream. */
int32_t tllm_session_verify_top1(tllm_session_t s, int32_t* top1, int32_t n, tllm_stream_t stream);

/* Speculative SAMPLING by exact match (the rule of the draws: csrc/kernels/kernels.h SpecSampleParams,
 * restated in numpy in spec_ref.sample_rows).  tllm_session_verify under the session's sampling configuration
 * (tllm_session_set_sampling): same arguments, same append pass, same head on all B * n rows, same log_probs (the raw model's
 * log p, whatever the configuration), and the accept rule with the sampler's draws in the arg-maxes' place:
 *   d[i] = the id the sampler selects from row i for generated-token number g = sequence_length[b] + i + 2 - max_input_len, with
 *          the step's own uniform variate Philox(random_seed; b, g) and, for the penalties, the history prompt + record +
 *          ids[b][0..i] - the token a plain sampled step would put behind ids[b][0..i];
 *   m = 0; while (m + 1 < n && d[m] != end_id && ids[b][m + 1] == d[m]) ++m;   the new pending token is d[m].
 * Draft i + 1 survives only where it EQUALS the draw of row i; the draw behind the last kept draft is the new pending token.  For
 * one-hot drafts the acceptance probability is p(draft), the rejection rule's min(1, p / q) at q = 1 - and beyond equality in
 * distribution the tokens are the very tokens tllm_session_generate yields for that configuration and seed, whatever the drafts
 * and whatever n (up to the arithmetic of the logits: a verify row comes from the append's GEMMs, a step's from the GEMVs).
 * With a configuration that is plain arg-max, or none, no sampler launch is made: the call is tllm_session_verify bit for bit.
 * Refused: everything tllm_session_verify refuses except the sampling configuration.
 * Not built: a draft model with a soft q and the residual-distribution rule. */
int32_t tllm_session_verify_sampled(tllm_session_t s, const int32_t* ids, int32_t n, int32_t* accepted, float* log_probs,
    tllm_stream_t stream);
/* For tests: the ids the last verify pass compared the drafts with, HOST int32 [B, n]: the draws d[b][i] after a sampled pass, the
 * arg-maxes after a greedy one (rows of frozen sequences of a sampled pass hold end_id).  n as that pass's; refused before any
 * verify pass.  Synchronises the stream. */
int32_t tllm_session_verify_draws(tllm_session_t s, int32_t* draws, int32_t n, tllm_stream_t stream);
/* For tests: the B * n logits rows of the last verify pass, HOST f32 [B, n, vocab].  n as that pass's; refused before any verify
 * pass.  Synchronises the stream. */
int32_t tllm_session_verify_logits(tllm_session_t s, float* logits, int32_t n, tllm_stream_t stream);

/* tllm_session_generate with prompt-lookup drafts: the same tokens (greedy), fewer passes where the text repeats itself.
 * After tllm_session_context every round enqueues (1) the prompt lookup - per sequence the up to num_draft_tokens - 1 tokens that
 * followed the most recent earlier occurrence of its last max_ngram .. 1 tokens, in its own record (prompt without the padding +
 * generated tokens) - straight into the pass's input ids, (2) ONE readback of {sequence_length, finished, draft length} per
 * sequence, the round's only host synchronisation, (3) one pass: a generation step (from the graph) when no sequence has a draft
 * and none is frozen - a step advances every sequence, so it is taken only while all are live - else a verify pass of
 * num_draft_tokens ids.  A sequence is frozen once it is finished or holds max_new_tokens tokens; the loop ends when all are.
 *   cfg    num_draft_tokens in [2, TLLM_VERIFY_MAX_TOKENS] (ids per verify pass, the pending token included), max_ngram in [1, 8];
 *   stats  (may be NULL) rounds = passes, verify_rounds + step_rounds = rounds, drafted = draft tokens offered, accepted = drafts kept;
 *   output_ids as tllm_session_generate fills it.
 * Refused: what tllm_session_verify refuses; max_new_tokens < 1 or max_new_tokens + num_draft_tokens > setup's max_new_tokens (the
 * last verify pass still writes num_draft_tokens cache rows from the current length).  When a bounded wait of the one-launch
 * generation step expires the call fails as tllm_session_append_generate does: the session's results are invalid. */
typedef struct
{
    int32_t num_draft_tokens;
    int32_t max_ngram;
} tllm_lookup_config_t;
typedef struct
{
    int64_t rounds, verify_rounds, step_rounds, drafted, accepted;
} tllm_lookup_stats_t;
int32_t tllm_session_generate_lookup(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, const tllm_lookup_config_t* cfg, int32_t* output_ids,
    tllm_lookup_stats_t* stats, tllm_stream_t stream);
/* tllm_session_generate_lookup under the session's sampling configuration: same signature, rounds and statistics.  A plain round
 * is the graph's sampler step, a verify round is tllm_session_verify_sampled's pass.  The tokens are tllm_session_generate's for
 * the same configuration and seed (see there for the one reservation, the arithmetic of the logits).  Refused: what
 * tllm_session_generate_lookup refuses except the sampling configuration. */
int32_t tllm_session_generate_lookup_sampled(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, const tllm_lookup_config_t* cfg, int32_t* output_ids,
    tllm_lookup_stats_t* stats, tllm_stream_t stream);

/* Top-k / top-p sampling with temperature, repetition / presence penalty and minimum length, on the device inside the
 * generation step (the reference's dynamic decoder with beam_width 1: PY/runtime/generation.py:299-345, 949-961 ->
 * layers/baseSamplingLayer.cpp:171-248, layers/topKSamplingLayer.cu, K/samplingTopKKernels.cu, samplingTopPKernels.cu,
 * samplingPenaltyKernels.cu).  The rule is stated in trtllm-llama_amd/csrc/kernels/kernels.h (SamplingParams) and restated in
 * numpy in tensorrt_llm/runtime/sampling_ref.py.  The uniform variate of row b's generated token g is a function of
 * (random_seed, b, g) alone (Philox4x32-10; the reference's cuRAND sequence is not reproduced) and the weights are summed as
 * integers, so the tokens are a function of the prompt, the configuration and the seed: the same in every launch, process and
 * tensor-parallel rank.  Defaults (the greedy configuration): top_k 1, top_p 0, temperature 1, repetition_penalty 1,
 * presence_penalty 0, min_length 1, random_seed 0. */
typedef struct
{
    int32_t top_k;            /* 0 = no top-k limit (top-p only); clipped to 1024 */
    float top_p;              /* clipped to [0, 1]; 0 with top_k > 0 means 1, 0 with top_k == 0 means arg-max */
    float temperature;        /* > 0 */
    float repetition_penalty; /* > 0; 1 = off.  Mutually exclusive with presence_penalty */
    float presence_penalty;   /* 0 = off */
    int32_t min_length;       /* end_id cannot be drawn before this many tokens were generated */
    uint64_t random_seed;
} tllm_sampling_config_t;
/* Valid after tllm_session_setup (which returns the session to greedy), beam_width 1 only (the reference's beam search ignores
 * these fields too).  Call it between requests: it applies from the next sampler launch on, so the next tllm_session_context /
 * tllm_session_generate runs under it as a whole.  The session does not track where a request driven through
 * tllm_session_step ends and therefore does not refuse a call between a context and its steps; the remaining steps of that
 * request then follow the new rule.  cfg == NULL returns to greedy.  A configuration that is plain arg-max (top_k 1,
 * temperature 1, no penalty, min_length <= 1) keeps launching the greedy step.  Drops the captured step graph. */
int32_t tllm_session_set_sampling(tllm_session_t s, const tllm_sampling_config_t* cfg);
/* Kernel-level entry (parity tests, micro-benchmarks): one draw per row through the launcher the session uses.
 *   logits         DEVICE f32 [nparts, rows, vocab_part] (vocabulary shards as the all-gather leaves them; id = part * vocab_part + i,
 *                  ids >= vocab are padding);
 *   history        DEVICE int32 [rows, history_stride] or NULL when cfg sets no penalty: slots [0, max_input_len) the padded
 *                  prompt, of which [0, input_lengths[r]) are real (input_lengths DEVICE int32 [rows], NULL = all), behind them
 *                  the g[r] - 1 tokens generated so far;
 *   g              DEVICE int32 [rows]: number of the generated token drawn, 1-based;
 *   out_ids        DEVICE int32 [rows];  u_out  optional DEVICE f32 [rows]: the uniform variate of each draw. */
int32_t tllm_sample_tokens(const float* logits, int32_t nparts, int32_t rows, int32_t vocab_part, int32_t vocab,
    const tllm_sampling_config_t* cfg, int32_t end_id, const int32_t* history, int32_t history_stride, const int32_t* input_lengths,
    int32_t max_input_len, const int32_t* g, int32_t* out_ids, float* u_out, tllm_stream_t stream);
/* Kernel-level entry (parity tests): per-row log-probability of a target id, log-sum-exp and arg-max through the launchers
 * tllm_session_score uses (rule and special values: TokenLogprobParams in csrc/kernels/kernels.h - target outside [0, vocab):
 * log_prob 0; target logit -inf: log_prob -inf; NaN / +inf logits: undefined; the logits are not written).
 * logits DEVICE f32 [nparts, rows, vocab_part] (id = part * vocab_part + i; ids >= vocab are padding); targets DEVICE int32 [rows];
 * partials DEVICE f32 [nparts, rows, 8] scratch (left readable); log_probs DEVICE f32 [rows]; lse (f32) and top1_ids (int32) DEVICE [rows] or NULL. */
int32_t tllm_token_logprobs(const float* logits, int32_t nparts, int32_t rows, int32_t vocab_part, int32_t vocab,
    const int32_t* targets, float* partials, float* log_probs, float* lse, int32_t* top1_ids, tllm_stream_t stream);

/* Parity-test tap (sessions created with debug_taps=1 only): the input of layer `layer`'s O-projection GEMM as the last
 * generation step computed it - the attention context after the split-KV merge, [B, H/tp * Dh] fp16, or int8 when the
 * O-projection's prologue quantises it (SmoothQuant: sat(rni(ctx * attention.quantization_scaling_factor)), or the
 * per-token flavour).  This is the tensor the reference's attention tests compare at atol 2e-3
 * (T/tests/attention/test_gpt_attention.py:828-831).  HOST buffer of exactly that many bytes. */
int32_t tllm_session_get_tap(tllm_session_t s, int32_t layer, void* host, size_t nbytes, tllm_stream_t stream);
/* The same for every GEMM input of the layer, i.e. all four quantisers of the SmoothQuant block
 * (PY/quantization/layer.py:223-265 norm + quant, :385-439 MLP, :596-852 attention; K/quantization.cu:31-118):
 *   which 0  QKV input        [B, hidden]     behind input_layernorm (+ its quantiser)
 *         1  O-projection in  [B, H/tp * Dh]  (= tllm_session_get_tap)
 *         2  fc | gate input  [B, hidden]     behind post_layernorm (+ its quantiser)
 *         3  proj input       [B, inter/tp]   SwiGLU output (+ its quantiser)
 *         4  the layer's input row of the residual stream [B, hidden], always fp16
 * 0..3: fp16, or int8 with SmoothQuant - parity tests compare these against the oracle in LSBs, and check every stage of the layer
 * as a function of the engine's OWN previous tap (no compounding across stages).  HOST buffer of exactly that size. */
int32_t tllm_session_get_tap_ex(tllm_session_t s, int32_t layer, int32_t which, void* host, size_t nbytes, tllm_stream_t stream);
/* Bytes a generation step must move from HBM at context length L (weights + KV read + KV write): the
 * algorithmic-bytes model of SURVEY.md §8(d), evaluated for this session's configuration. */
int64_t tllm_session_step_bytes(tllm_session_t s, int32_t context_len);

/* Live per-kernel timing for bench.py's roofline: launches ONLY kernel K<which> of every layer (1 = RMSNorm+QKV GEMV - or, when
 * the session runs the one-launch projection + attention, that launch WITHOUT its later stages; 2 = decode attention,
 * 4 = O-projection GEMV, 5 = RMSNorm+gate|up GEMV+SwiGLU, 6 = down GEMV, 7 = the one-launch projection + attention exactly
 * as the generation step runs it, with every stage tllm_session_decode_form reports, 8 = the one-launch MLP - RMSNorm + gate|up +
 * SwiGLU + down + residual, kernels/mlp_fused.hip - where the session runs it; 5 / 6 then time the two GEMVs it replaces) back to back,
 * `sweeps` passes over the layers (each layer has its own weights, so every launch streams cold HBM exactly as in a
 * real step), bracketed by one HIP event pair on the session's stream.  avg_us = elapsed / launches (inter-launch
 * gaps included).  Activations are whatever the buffers hold: timing only, call tllm_session_fake_context or
 * tllm_session_context again before generating. */
int32_t tllm_session_time_kernel(tllm_session_t s, int32_t which, int32_t sweeps, float* avg_us, int64_t* launches,
    tllm_stream_t stream);

/* Requests tllm_session_generate ran a SECOND time because a bounded in-launch wait of the one-launch projection + attention
 * expired (the session falls back to separate launches and repeats the request: generation is a function of the prompt and,
 * with sampling on, of the seed - the sampler's random numbers are counter-based and its sums are integer, so the repeat draws
 * the same tokens). */
int32_t tllm_session_fused_retries(tllm_session_t s);

/* Which launches a generation step of this session is made of (decided at setup; a time-out of the one-launch form clears it):
 * bit 0 = QKV projection + RoPE + cache append + attention in one launch (kernels/qkv_attn_fused.hip), bit 1 = the O-projection +
 * residual as a stage of that launch, bit 2 = the gated MLP (gate|up GEMV + down GEMV) in one launch (kernels/mlp_fused.hip, r06;
 * opt-in with the session key fuse_mlp = 1: bit-identical, measured slower than the two GEMVs).  -1 before setup. */
int32_t tllm_session_decode_form(tllm_session_t s);
/* Step graphs this session has captured since it was created (tllm_session_step with use_graph: one per capture, none per
 * replay).  A test sees with it that select / commit / clear of LoRA adapters did not cost a capture.  -1: null session. */
int64_t tllm_session_graph_captures(tllm_session_t s);
/* Greedy-step launches this session has enqueued WITH the lm_head launch's arg-max pairs since its last setup (session key
 * greedy_partials; batch 1, tp 1, greedy).  A step captured into the graph counts once, when it is captured, not per replay.
 * 0 after generation steps = every greedy step scanned the logits.  -1: null session. */
int64_t tllm_session_greedy_partials_used(tllm_session_t s);

/* Instrumented generation steps (eager, a hipEvent pair around every launch) for the roofline report:
 * elapsed milliseconds and launch counts per class over `n_steps` steps.
 * Classes: 0 layer GEMVs (QKV, O, gate|up, down), 1 lm_head GEMV, 2 attention (split-KV + combine),
 *          3 embedding + sampler, 4 tensor-parallel collectives.  Arrays of TLLM_PROFILE_CLASSES entries. */
#define TLLM_PROFILE_CLASSES 5
int32_t tllm_session_profile(tllm_session_t s, int32_t n_steps, float* ms_per_class, int64_t* launches_per_class,
    tllm_stream_t stream);

void tllm_session_destroy(tllm_session_t s);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entry for the fused skinny GEMM that the generation step is built from (kernels/gemv.hip);
 * exposed so that parity tests and the micro-benchmark can drive every prologue / epilogue directly.
 * Field meanings: trtllm-llama_amd/csrc/kernels/kernels.h (GemvParams).
 * ---------------------------------------------------------------------------------------------- */
typedef struct
{
    int32_t wtype, pro, epi, out_dtype;
    int32_t M, N, K;
    const void* x;
    int64_t ldx;
    const void* w;
    int64_t ldw;
    const void* scale_col;
    const float* scale_row;
    int32_t per_channel, per_token;
    const void* gamma;
    float eps;
    const float* act_scale;
    float* dyn_scale_out;
    void* x_pro_out;
    const void* residual;
    const float* epi_scale;
    void* y;
    int64_t ldy;
} tllm_gemv_params_t;

int32_t tllm_gemv(const tllm_gemv_params_t* p, tllm_stream_t stream);
/* The same launch with the two options of the lm_head launch (kernels.h GemvParams::resident_rows / argmax_part; fp16 weights,
 * M = 1, no epilogue - anything else is refused): rows [0, resident_rows) of W load with the allocating cache policy, the rest
 * non-temporally (results do not depend on it); argmax_part, if not NULL, receives TLLM_ARGMAX_PAIRS pairs {float value, int32
 * index}: per wave of the launch the arg-max of the outputs it finished (ties: lowest index), {-inf, INT32_MAX} elsewhere. */
#define TLLM_ARGMAX_PAIRS 2048
int32_t tllm_gemv_head(const tllm_gemv_params_t* p, int32_t resident_rows, void* argmax_part, tllm_stream_t stream);

/* Kernel-level entries of the two LoRA launches (kernels/lora.hip; the rule: kernels.h LoraShrinkParams / LoraExpandParams), so
 * that tests reach them without a model.  table: device array of num_adapters records {const void* a; const void* b; float
 * scale; int32 reserved} (24 bytes each): A fp16 [nseg * r, K], B fp16 [sum seg_n, r].  row_adapter: device int32 [M], a value
 * outside [0, num_adapters) = no adapter for that row.
 *   shrink  t[m][j] = sum_k A[j][k] xh[m][k] (fp32), xh = x (pro 0) or RMSNorm(x) gamma (pro 1), R = nseg * r rows of A;
 *   expand  y[m][n] = f16(f32(y[m][n]) + scale * sum_j B[n][j] t[m][seg(n) r + j]) in place; segment g has seg_n[g] columns that
 *           start at seg_y[g] with row stride seg_ldy[g] (elements). */
#define TLLM_LORA_MAX_ADAPTERS 8
#define TLLM_LORA_MAX_SEGMENTS 3
typedef struct
{
    int32_t M, K, R, pro;
    const void* x;
    int64_t ldx;
    const void* gamma;
    float eps;
    const int32_t* row_adapter;
    const void* table;
    int32_t num_adapters;
    float* t;
} tllm_lora_shrink_params_t;
int32_t tllm_lora_shrink(const tllm_lora_shrink_params_t* p, tllm_stream_t stream);
typedef struct
{
    int32_t M, r, nseg;
    int32_t seg_n[TLLM_LORA_MAX_SEGMENTS];
    void* seg_y[TLLM_LORA_MAX_SEGMENTS];
    int64_t seg_ldy[TLLM_LORA_MAX_SEGMENTS];
    const float* t;
    const int32_t* row_adapter;
    const void* table;
    int32_t num_adapters;
} tllm_lora_expand_params_t;
int32_t tllm_lora_expand(const tllm_lora_expand_params_t* p, tllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LoRA adapters per sequence.  Session keys: lora_max_rank (0 = off; 8, 16, 32 or 64),
 * lora_max_adapters (1 .. 8, default 1), lora_target_modules (comma list out of q,k,v,o,gate,up,down; default q,k,v,o).
 * Refused with the key's name: SmoothQuant weights, tp_size > 1 (create), beam_width > 1 (setup).
 *   lora_set_tensor  stages one tensor of adapter slot `slot`: "layers.{i}.{attention.q|attention.k|attention.v|attention.dense|
 *                    mlp.fc|mlp.gate|mlp.proj}.lora_a" fp16 [r, K] or ".lora_b" fp16 [N_module, r], r <= lora_max_rank.
 *                    location as tllm_session_set_tensor (0 host, 1 device); the data is copied before the call returns.
 *   lora_commit      checks the staged tensors against the configuration (a module outside lora_target_modules is refused by
 *                    name, one of the list that the adapter lacks is zeros, the ranks of a and b of a module must agree), packs
 *                    them into the sites' layout zero-padded to lora_max_rank, sets scale = alpha / r (flags & 1, rsLoRA:
 *                    alpha / sqrt(r)), r the adapter's own rank, and drops the staged tensors.  A refused commit leaves the slot
 *                    as it was and drops the staged tensors.
 *   lora_clear       the slot is uncommitted again (sequences that selected it go back to none).
 *   lora_select      slots: HOST int32 [batch], -1 = none; after setup, holds until changed, all -1 after every setup.  An
 *                    uncommitted or out-of-range slot is refused with nothing written.
 * The adapters live at fixed device addresses and the selection is a device array: a captured step graph stays valid across
 * select, commit and clear.
 * Ordering: these entry points take no stream.  commit, clear and select wait for the device to be idle (hipDeviceSynchronize)
 * before they write, so work that an earlier tllm_session_step / _context / _append left in flight on ANY stream - the caller's
 * non-blocking one included - finishes under the old adapters and selection, and whatever is enqueued afterwards sees the new.
 * ---------------------------------------------------------------------------------------------- */
int32_t tllm_session_lora_set_tensor(tllm_session_t s, int32_t slot, const char* name, int32_t dtype, const int64_t* dims,
    int32_t nbDims, const void* data, int32_t location);
int32_t tllm_session_lora_commit(tllm_session_t s, int32_t slot, float alpha, int32_t flags);
int32_t tllm_session_lora_clear(tllm_session_t s, int32_t slot);
int32_t tllm_session_lora_select(tllm_session_t s, const int32_t* slots);

/* Kernel-level entry for the greedy step that ends a generation step (kernels/decode_step.hip; kernels.h GreedyParams), for parity
 * tests: the arg-max of logits f32 [nparts, batch, vocab_part] (ids >= vocab are padding), then the bookkeeping on the caller's
 * device buffers - seq_len[b] += advance, finished rows emit end_id, out_ids[b, seq_len[b]] = id, cur_ids[b] = id,
 * finished[b] |= id == end_id, the RoPE row of position seq_len[b] - (max_input_len - input_lengths[b]) and the embedding row
 * of id.  argmax_part (batch 1, nparts 1): the pairs tllm_gemv_head left for these logits - reduced instead of the logits. */
typedef struct
{
    const float* logits;
    int32_t batch, vocab_part, nparts, vocab;
    int32_t* cur_ids;
    int32_t* out_ids;
    int32_t out_stride;
    int32_t* seq_len;
    int32_t* finished;
    int32_t end_id, advance;
    float* rope_row_out;
    int32_t* rope_pos_out;
    const float* rope_table;
    int32_t rope_half, rope_table_len;
    const int32_t* input_lengths;
    int32_t max_input_len;
    const void* emb_table;
    void* x_out;
    int32_t hidden;
    uint32_t* step_epoch;
    const void* argmax_part;
} tllm_greedy_params_t;
int32_t tllm_greedy_step(const tllm_greedy_params_t* p, tllm_stream_t stream);
/* Kernel-level entries of speculative greedy decoding (kernels/spec_decode.hip; kernels.h SpecAcceptParams / PromptLookupParams),
 * for parity tests.  All pointers DEVICE.
 * tllm_spec_accept: the accept step on the caller's buffers.  g as tllm_greedy_step takes it, except g.logits = the verify rows f32
 *   [batch * n, vocab_part] (nparts 1), g.advance / g.argmax_part ignored.  ids, top1 int32 [batch, n]; limit int32 [batch] or
 *   NULL; accepted int32 [batch] or NULL; logits_out f32 [batch, vocab_part] or NULL (receives row accepted[b] of sequence b).
 * tllm_prompt_lookup: ids int32 [batch, n] = [pending, draft..., pending...], draft_len int32 [batch] from out_ids int32
 *   [batch, out_stride] / seq_len / input_lengths (NULL = max_input_len) / finished (or NULL) / limit (or NULL), all int32 [batch]. */
typedef struct
{
    tllm_greedy_params_t g;
    int32_t n;
    const int32_t* ids;
    const int32_t* top1;
    const int32_t* limit;
    int32_t* accepted;
    float* logits_out;
} tllm_spec_accept_params_t;
int32_t tllm_spec_accept(const tllm_spec_accept_params_t* p, tllm_stream_t stream);
int32_t tllm_prompt_lookup(const int32_t* out_ids, int32_t batch, int32_t out_stride, const int32_t* seq_len,
    const int32_t* input_lengths, int32_t max_input_len, const int32_t* finished, const int32_t* limit, int32_t vocab, int32_t n,
    int32_t max_ngram, int32_t* ids, int32_t* draft_len, tllm_stream_t stream);
/* tllm_spec_sample_rows: the sampler on all n rows per sequence of a verify pass, on the caller's buffers (kernels.h
 *   SpecSampleParams; the launcher tllm_session_verify_sampled uses).  All pointers DEVICE.  logits f32 [batch * n, vocab_part]
 *   (nparts must be 1, vocab <= vocab_part; never written); ids int32 [batch, n]; out_ids int32 [batch, out_stride] the token
 *   record (prompt slots [0, max_input_len), committed tokens behind; NULL when cfg sets no penalty); seq_len int32 [batch];
 *   input_lengths / finished / limit int32 [batch] or NULL; draws int32 [batch, n]: the id drawn for generated-token number
 *   seq_len[b] + i + 2 - max_input_len, end_id in the rows of a frozen sequence (finished, or seq_len >= limit); u_out optional
 *   f32 [batch, n].  Refused: n outside [1, TLLM_VERIFY_MAX_TOKENS], nparts != 1, what tllm_sample_tokens refuses of cfg. */
int32_t tllm_spec_sample_rows(const float* logits, int32_t nparts, int32_t batch, int32_t n, int32_t vocab_part, int32_t vocab,
    const tllm_sampling_config_t* cfg, int32_t end_id, const int32_t* ids, const int32_t* out_ids, int32_t out_stride,
    const int32_t* seq_len, const int32_t* input_lengths, int32_t max_input_len, const int32_t* finished, const int32_t* limit,
    int32_t* draws, float* u_out, tllm_stream_t stream);
/* Test/bench knob: persistent workgroups per CU (0 = occupancy query). */
void tllm_gemv_set_blocks_per_cu(int32_t n);
/* Test/bench knob: number of rows (sequences) from which the SmoothQuant decode GEMM runs on the matrix pipe
 * (kernels/gemv_mfma_sq.hip, static activation scales) instead of the skinny vector-ALU kernel: 0 = never, -1 = the default
 * (5).  Both kernels give bit-identical results. */
void tllm_gemv_set_mfma_rows(int32_t n);
/* Test/bench knob: kernel id of the prefill GEMM (0 = tactic table, else the static rule).  1..12: lock-step tile shapes of
 * kernels/gemm_glds.hip (8 = 128x128, 6 = 256x192, 2 = 256x256, 4 = 128x256 are the production ones); 15..63: the phased
 * SmoothQuant pipeline of kernels/gemm_sqp.hip (20 = 256x192, 42 = 256x128, one tile per workgroup; 63 / 62 their persistent
 * forms, r05; 64 / 65 = 256x128 / 128x128 as two workgroups per tile splitting K, r06; 21..33 are ablations with wrong results on purpose);
 * 50..58: the same pipeline on fp16 operands (50 = 256x192, 54 = 256x128, 55 / 56 persistent, 57 / 58 split-K); 101..106: the weight-only kernel of kernels/gemm_woq.hip (101 = 256x192, 102 = 128x128,
 * 106 = 256x128); -2: the fused SwiGLU GEMM in its one-tile form.  The ids are what tllm_gemm_profile reports. */
void tllm_gemm_set_tile_cfg(int32_t cfg);

/* Kernel-level entry for the prefill GEMMs (kernels/gemm_mfma.hip; M <= 8 goes to the skinny GEMM):
 * C[m,n] = epi(sum_k A[m,k] W[n,k]); wtype / layouts / scales as tllm_gemv_params_t.  Used by the MFMA-utilisation
 * report (SmoothQuant GEMM at M = 1024) and by parity tests. */
typedef struct
{
    int32_t wtype, out_dtype;
    int32_t M, N, K;
    const void* a;
    int64_t lda;
    const void* w;
    int64_t ldw;
    const void* scale_col;
    const float* scale_row;
    int32_t per_channel, per_token;
    void* c;
    int64_t ldc;
} tllm_gemm_params_t;

int32_t tllm_gemm(const tllm_gemm_params_t* p, tllm_stream_t stream);
/* The same with the decoder layer's residual add in the epilogue: c = fp16(fp16(epi(A W^T)) + residual), residual fp16 [M, ldc]
 * (the `hidden_states = residual + attention_output` / `+ mlp_output` of Q/llama_model.py:78-86, which the prefill runs inside its
 * O- and down-projection GEMMs).  fp16 output only; parity tests of the multi-tile (persistent) kernels' residual path. */
int32_t tllm_gemm_residual(const tllm_gemm_params_t* p, const void* residual, tllm_stream_t stream);
/* tllm_gemm with either optional epilogue operand (both fp16 [M, ldc], fp16 output, not together): residual as above; silu_gate:
 * c = fp16(fp16(silu(gate)) * fp16(epi(A W^T))), the gate half of SwiGLU that the fp16 / weight-only prefill runs inside its
 * up-projection GEMM.  Whatever kernel the dispatch picks, including the passes behind the kernels that fuse neither. */
int32_t tllm_gemm_epi(const tllm_gemm_params_t* p, const void* residual, const void* silu_gate, tllm_stream_t stream);
/* EXACTLY this kernel or nothing (parity tests: a forced id that refuses the problem must not fall back silently).  Returns 0
 * when the kernel was launched, 1 when it does not serve the problem (reason in the last-error string, c not written), a
 * negative value on a launch error.  kernel_id: 1..65 as tllm_gemm_set_tile_cfg takes them (the ablations 21..27 / 31..33 are
 * refused), 101..106 the weight-only kernel of kernels/gemm_woq.hip with that tile shape, TLLM_GEMM_KERNEL_REGISTER_STAGED the
 * 128 x 128 register-staged kernel of kernels/gemm_mfma.hip (every weight type; fuses neither residual nor gate: refused). */
#define TLLM_GEMM_KERNEL_REGISTER_STAGED 200
int32_t tllm_gemm_kernel(const tllm_gemm_params_t* p, const void* residual, const void* silu_gate, int32_t kernel_id,
    tllm_stream_t stream);
/* The kernel id the static rule picks for the problem on this device when the tactic table has no entry (0: none of the
 * LDS-DMA kernels serves it). */
int32_t tllm_gemm_static_cfg(const tllm_gemm_params_t* p);
/* The SmoothQuant MLP's fc and gate projections in one launch (static activation scales): c = int8 [M, ldc] =
 * sat(rni(fp16(silu16(fp16(A W^T s)) * fp16(A W_up^T s_up)) * quant_scale[0])) - the rounding points of GEMM + GEMM + SwiGLU +
 * quantiser run separately (PY/layers/mlp.py:68-73 with K/quantization.cu's static quantiser), which it replaces in the
 * prefill.  p->w / p->scale_col: the matrix that goes through SiLU; p->c: int8 output. */
int32_t tllm_gemm_swiglu_quant(const tllm_gemm_params_t* p, const void* w_up, const void* scale_col_up, const float* quant_scale,
    tllm_stream_t stream);
/* On-device tactic selection for the prefill GEMMs (M >= 32; SmoothQuant int8 = wtype 3, fp16 = wtype 0 - also what the weight-only
 * prefill runs on its expanded weights).  Takes the place of the profile the reference's SmoothQuant GEMM plugin runs when an
 * engine is built - every CUTLASS tile configuration timed on the device per M bucket
 * (K/cutlass_kernels/int8_gemm/int8_gemm_template.h:372-457), the winners kept in the plugin's serialisation
 * (P/smoothQuantGemmPlugin/smoothQuantGemmPlugin.cpp:253-282):
 *   profile : times every candidate kernel (tile shape x lock-step / phased pipeline) for C[M, N] = A[M, K] W[N, K]^T on random
 *             operands of its own and records the fastest in the process-wide table; best_cfg = its id (as tllm_gemm_set_tile_cfg
 *             takes them), 0 when no MFMA kernel serves the shape.  A session does this for its own four GEMM shapes at
 *             tllm_session_setup (unless the engine brought the table, or TLLM_GEMM_TACTICS=off);
 *   export  : the table as text "wtype:M:N:K:cfg:us;..." - returns the bytes needed including the terminator; the builder stores
 *             it in the engine file (header line `gemm_tactics=`), tllm_session_load_engine / tllm_session_create import it;
 *   lookup  : the kernel id tllm_gemm will use for the shape (exact M, else the nearest profiled M of the same power-of-two
 *             bucket), 0 = the static "fewest workgroup rounds" rule. */
int32_t tllm_gemm_profile(int32_t wtype, int32_t M, int32_t N, int32_t K, int32_t* best_cfg, float* best_us, tllm_stream_t stream);
int64_t tllm_gemm_tactics_export(char* buf, int64_t capacity);
int32_t tllm_gemm_tactics_import(const char* text);
void tllm_gemm_tactics_clear(void);
int32_t tllm_gemm_tactic_lookup(int32_t wtype, int32_t M, int32_t N, int32_t K);
/* Microbenchmark hook: while set (non-NULL), every workgroup of the phased SmoothQuant GEMM writes {shader cycles, ticks of
 * the constant 100 MHz counter} over its lifetime to device_buffer[2 * workgroup] (uint64) - the clock the chip held. */
void tllm_gemm_set_clock_probe(void* device_buffer);

/* Kernel-level entry for the two attention launchers (kernels/mmha_decode.hip, kernels/context_attn.hip) with grouped-query
 * attention: num_kv_heads = Hkv K/V heads, 1 <= Hkv <= H, H % Hkv == 0, query head h reads K/V head h / (H / Hkv); 0 or H is
 * multi-head attention, bit for bit what the GPTAttention plugin runs; Hkv = 1 is multi-query attention.  Layouts:
 *   qkv     fp16, one row per token [ q: H*Dh | k: Hkv*Dh | v: Hkv*Dh ]; decode [B, row], context [B, S, row] or, packed
 *           (cu_seqlens set), [sum(len), row]; the context launch rewrites q and k in place with RoPE applied;
 *   cache   [B, 2, Hkv, Smax, Dh] fp16 / int8 / fp8 E4M3 (kv_cache_type TLLM_HALF / TLLM_INT8 / TLLM_FP8); paged (block_pointers
 *           int64 [B, 2, max_blocks_per_seq] set): blocks [Hkv, tokens_per_block, Dh], kv_cache = the pool the blocks lie in (the
 *           decode launch reads the rows of a block the table does not map yet - entry 0 - from there, and masks them);
 *   out     fp16 [B, H*Dh] (decode), [B, S, H*Dh] or packed (context).
 * Numerics are those documented at the head of the two kernel files, per query head on the K/V head it maps to; RoPE on the new
 * k, the cache quantisation and the cache write happen once per K/V head.  The RoPE table is the process-wide one the plugin uses.
 * Every field not needed is 0 / NULL (memset the struct). */
typedef struct
{
    int32_t batch;         /* sequences (decode: batch x beam) */
    int32_t seq;           /* context: the padded / longest prompt length; decode: ignored */
    int32_t num_heads, num_kv_heads, head_size;
    int32_t rotary_dim, neox;
    float q_scaling;       /* scores * 1 / (sqrt(Dh) * q_scaling); 0 = 1 */
    int32_t kv_cache_type; /* TLLM_HALF (or 0), TLLM_INT8, TLLM_FP8 */
    int32_t max_seq_len;   /* cache capacity Smax */
    int32_t max_input_len; /* decode: padded prompt length (RoPE position = timestep - (max_input_len - input_lengths[b])) */
    int32_t timestep;      /* decode: past length from the host; -1 = sequence_length[b] */
    void* qkv;
    void* kv_cache;
    const int32_t* sequence_length; /* decode: device int32 [B], slots in use; the new token goes to that slot */
    const int32_t* input_lengths;   /* device int32 [B] */
    const int32_t* masked_tokens;   /* decode: device int32 [B, Smax] or NULL */
    const float* kv_scale_orig_quant; /* device f32 [1] (int8 / fp8 cache) */
    const float* kv_scale_quant_orig; /* device f32 [1] (decode, int8 / fp8 cache) */
    const int32_t* cache_indirection; /* decode, beam_width > 1: device int32 [B, Smax] */
    int32_t beam_width;               /* 0 = 1 */
    int32_t cache_seq_stride;         /* context: prompt b fills the cache rows of sequence b * cache_seq_stride; 0 = 1 */
    const int64_t* block_pointers;
    int32_t tokens_per_block, max_blocks_per_seq;
    const int32_t* cu_seqlens; /* context, packed inputs: device int32 [B + 1] */
    /* decode launch shape.  rows_per_group: cache rows per lane group and split (4, 12, 16); 0 = the plugin's rule.
     * q_heads_per_workgroup: query heads of one K/V head served from one load of the cache rows (1, 2, 4, 8); 0 = the launcher's
     * rule.  A forced value runs exactly that instance or the call returns non-zero with tllm_last_error() set and nothing
     * launched - never a substitute.  combine_launch: 1 = merge the splits in a second launch even where the in-launch merge
     * (at most 16 splits) would serve. */
    int32_t rows_per_group, q_heads_per_workgroup, combine_launch;
    /* context launch shape.  context_kernel: the attention kernel, TLLM_CTX_ATTN_WAVE (one wave per query), _MFMA_NARROW (64
     * queries per workgroup), _MFMA_WIDE (128) or _MFMA_PAIRED (two 64-query blocks per workgroup, three operand stages); 0 = the
     * launcher's rule.  A forced value runs exactly that instance or the call returns non-zero with tllm_last_error() set and
     * nothing launched - never a substitute: the MFMA kinds need head size 64 / 128, the workspace, seq >= 64 and a positive score
     * scale. */
    int32_t context_kernel;
    const float* tail_quant_scale; /* decode, in-launch merge: static int8 image of the context row to tail_out_q8 */
    void* tail_out_q8;
    int8_t* out_q8; /* context: static int8 image instead of (MFMA kernel) or next to `out` */
    const float* out_q_scale;
    void* out;
    void* workspace; /* tllm_attention_workspace_size() bytes; context: NULL runs the wave-per-query kernel */
} tllm_attention_params_t;
/* bytes of workspace for the decode (is_context 0: merge tickets + split partials) or the context launch (the V^T image) */
size_t tllm_attention_workspace_size(const tllm_attention_params_t* p, int32_t is_context);
int32_t tllm_attention_decode(const tllm_attention_params_t* p, tllm_stream_t stream);
int32_t tllm_attention_context(const tllm_attention_params_t* p, tllm_stream_t stream);
/* split geometry of the decode launch tllm_attention_decode would run for p: time steps per split, splits for max_seq_len, the
 * query tile, and whether the splits are merged inside the launch (1) or by the combine launch (0).  Non-zero: p is refused. */
int32_t tllm_attention_decode_layout(const tllm_attention_params_t* p, int32_t* tchunk, int32_t* nsplit, int32_t* q_tile,
    int32_t* in_launch_merge);
/* the attention kernel tllm_attention_context would run for p (batch, seq, num_heads, head_size, q_scaling, context_kernel and
 * whether workspace is NULL are read; no pointer is followed) on a device of `cus` compute units: its kind (TLLM_CTX_ATTN_*), the
 * queries per workgroup, the operand stages in LDS (0 for the wave-per-query kernel) and the workgroups of the launch.  cus 0 = the
 * current device; a non-zero cus needs no GPU.  Non-zero: p is refused (a forced context_kernel the launch cannot run). */
#define TLLM_CTX_ATTN_WAVE 1
#define TLLM_CTX_ATTN_MFMA_NARROW 2
#define TLLM_CTX_ATTN_MFMA_WIDE 3
#define TLLM_CTX_ATTN_MFMA_PAIRED 4
int32_t tllm_attention_context_layout(const tllm_attention_params_t* p, int32_t cus, int32_t* kind, int32_t* query_block,
    int32_t* stages, int32_t* workgroups);

/* Kernel-level entry of the append attention (kernels/append_attn.hip; the rule is DESIGN.md section 7c, restated in numpy float64
 * in tensorrt_llm/runtime/append_ref.py): n new tokens per sequence onto a live cache, the parallel form of n decode steps.
 * With p_b = sequence_length[b]: appended token i of sequence b gets RoPE at position p_b + i - (max_input_len -
 * input_lengths[b]), its k and v go to cache slot p_b + i by the store rule of the cache type, and its query sees every slot
 * t < p_b with masked_tokens[b][t] == 0 - read as the decode launch reads them - plus the appended tokens 0 .. i, whose k and v
 * enter un-quantised.  sequence_length is NOT advanced (the session's advance launch does that).  Two launches: RoPE + cache
 * write, then the attention.
 *   qkv    fp16 [B, n, (H + 2 Hkv) * Dh], rows [ q | k | v ]; q and k are rewritten in place with RoPE applied;
 *   cache  [B, 2, Hkv, Smax, Dh] fp16 / int8 / fp8 E4M3 (the paged cache: tllm_attention_append_paged);   out  fp16 [B, n, H * Dh].
 * max_past is the caller's promise max_past >= every sequence_length[b]: max_past + n > max_seq_len is refused with nothing
 * launched; on the device every cache store is guarded by slot < max_seq_len and every load index is clamped all the same.
 * append_kernel: TLLM_APPEND_ATTN_WAVE (one wave per query: every n, head sizes 32 / 64 / 128 / 256) or TLLM_APPEND_ATTN_MFMA (64
 * queries per workgroup, head sizes 64 / 128, n >= 16); 0 = the launcher's rule (MFMA where it serves).  A forced value runs exactly
 * that kernel or the call returns non-zero with tllm_last_error() set and nothing launched - never a substitute.
 * A struct of its own (tllm_attention_params_t keeps its layout); every field not needed is 0 / NULL (memset the struct). */
#define TLLM_APPEND_ATTN_WAVE 1
#define TLLM_APPEND_ATTN_MFMA 2
typedef struct
{
    int32_t batch;
    int32_t n;             /* tokens appended per sequence, the same for all */
    int32_t num_heads, num_kv_heads, head_size; /* num_kv_heads 0 = num_heads */
    int32_t rotary_dim, neox;
    float q_scaling;       /* scores * 1 / (sqrt(Dh) * q_scaling); 0 = 1 */
    int32_t kv_cache_type; /* TLLM_HALF (or 0), TLLM_INT8, TLLM_FP8 */
    int32_t max_seq_len;   /* cache capacity Smax */
    int32_t max_input_len; /* padded prompt length */
    int32_t max_past;
    int32_t append_kernel;
    void* qkv;
    void* kv_cache;
    const int32_t* sequence_length; /* device int32 [B]: the past lengths p_b, may differ per sequence */
    const int32_t* input_lengths;   /* device int32 [B] */
    const int32_t* masked_tokens;   /* device int32 [B, Smax] or NULL */
    const float* kv_scale_orig_quant; /* device f32 [1] (int8 / fp8 cache) */
    const float* kv_scale_quant_orig; /* device f32 [1] (int8 / fp8 cache) */
    void* out;
} tllm_attention_append_params_t;
int32_t tllm_attention_append(const tllm_attention_append_params_t* p, tllm_stream_t stream);
/* tllm_attention_append with a different number of tokens per sequence: sequence b appends n_b = n_per_seq[b] tokens (DEVICE int32
 * [batch]; clamped into [0, p->n] on the device), and everything above holds with n_b in place of n.  p->n stays the row stride
 * of qkv and out, the upper bound of every n_b and what chooses the kernel; p->max_past is ignored - max_end is the caller's
 * promise max_end >= every sequence_length[b] + n_b, and max_end > max_seq_len (or < 1) is refused with nothing launched.  Rows
 * i >= n_b of a sequence are padding: their qkv bits stay as they are (no RoPE), nothing of them is stored to the cache or read
 * as a query, key or value - NaN there reaches nothing - and their rows of out are written as zeros. */
int32_t tllm_attention_append_ragged(const tllm_attention_append_params_t* p, const int32_t* n_per_seq, int32_t max_end,
    tllm_stream_t stream);
/* tllm_attention_append (n_per_seq NULL; max_end ignored) or tllm_attention_append_ragged (n_per_seq set) on the paged cache:
 * p->kv_cache is the pool, block_pointers a DEVICE table int64 [batch, 2, max_blocks_per_seq] - row [b][0] the K blocks of sequence
 * b, row [b][1] its V blocks - of pointers to blocks laid out [Hkv, tokens_per_block, Dh]; slot t of a sequence is row
 * t % tokens_per_block of its block t / tokens_per_block, and p->max_seq_len stays the capacity Smax (masked_tokens is [B, Smax]).
 * Everything else is the linear entry's, and so is every result: out, the rewritten qkv and the rows the pool holds behind the
 * table are bit for bit what the linear launch leaves on the same logical cache.
 * A table entry of 0 is a block that is not mapped (a table grown on demand, KVCacheManager.extend): the store of a slot in it is
 * skipped, never aimed at 0 + offset - mapping the blocks of the slots [p_b, p_b + n_b) before the call is the caller's part - and
 * no load address is formed from it (such a load is pointed at the pool; slots >= p_b never enter a product).  Blocks may be
 * shared between sequences for slots below both their p_b.
 * Refused, with nothing launched: what the linear entries refuse; block_pointers NULL; a table without a pool; tokens_per_block
 * that is not a power of two; max_blocks_per_seq * tokens_per_block < max_seq_len.  The kernel choice does not depend on the
 * layout (tllm_attention_append_layout). */
int32_t tllm_attention_append_paged(const tllm_attention_append_params_t* p, const int64_t* block_pointers, int32_t tokens_per_block,
    int32_t max_blocks_per_seq, const int32_t* n_per_seq /* NULL = uniform */, int32_t max_end, tllm_stream_t stream);
/* the attention kernel tllm_attention_append would run for p (n, head_size and append_kernel are read; no pointer is followed; no
 * GPU needed): TLLM_APPEND_ATTN_WAVE or _MFMA in *kind.  Non-zero: a forced append_kernel the launch cannot run. */
int32_t tllm_attention_append_layout(const tllm_attention_append_params_t* p, int32_t* kind);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entries of the row-wise and element-wise kernels (kernels/pointwise.hip), so that tests reach every kernel without
 * a plugin or a session.  tllm_rmsnorm_params_t restates kernels.h RmsnormParams field for field (every field not needed is
 * 0 / NULL):
 *   y = f16(f16(x' * rsqrt(mean(x'^2) + eps)) * gamma), x' = x or f16(x + residual) (then written to sum_out, which is required);
 *   layernorm != 0: y = f16((x' - mean) * rstd * gamma + beta), variance as E[x^2] - mean^2 (use_diff_of_squares) or E[(x - mean)^2];
 *   q, if set: sat(rni(y * static_scale[0])), or with dyn_scale_out sat(rni(y * (127 / amax))) and dyn_scale_out[m] = amax / 127,
 *   amax = max(|y[m, :]|, f16(1e-6)).  y may be NULL when only q is wanted.
 * kernel: 0 = the launcher's choice, 1 = the scalar LDS kernel (any N, any fp16 alignment), 2 = the 16-byte LDS kernel (N % 8 == 0,
 * 16-byte aligned fp16 pointers, 8-byte aligned q), 3 = the register kernel (what 2 needs, RMSNorm only, 8 <= N <= 8192).  Both LDS
 * kernels hold the row in 128 + 2 N <= 64 KiB.  A forced kernel whose precondition does not hold returns -1 with
 * tllm_last_error() set and nothing launched - never a substitute.  0 on success (an empty problem included). */
typedef struct
{
    int32_t M, N;
    const void* x;
    const void* residual;
    void* sum_out;
    const void* gamma;
    float eps;
    void* y;
    int8_t* q;
    const float* static_scale;
    float* dyn_scale_out;
    int32_t layernorm, use_diff_of_squares;
    const void* beta;
} tllm_rmsnorm_params_t;
int32_t tllm_rmsnorm(const tllm_rmsnorm_params_t* p, int32_t kernel, tllm_stream_t stream);
/* the kernel tllm_rmsnorm(p, 0, ..) would run (the launcher's own rule; no pointer is followed, no GPU needed): 1, 2, or
 * 3 + 8 * NV for the register kernel with NV = 1 (N <= 2048), 2 (<= 4096) or 4 (<= 8192) vectors per thread; 0 for an empty problem
 * (M <= 0 or N <= 0: nothing is launched); -1 with tllm_last_error() set where the launch is refused. */
int32_t tllm_rmsnorm_kernel(const tllm_rmsnorm_params_t* p);
/* The launchers of kernels.h as they are (fp16 operands; non-zero with tllm_last_error() set on failure):
 *   swiglu y = f16(f16(silu(a)) * b); swiglu_quant q = sat(rni(swiglu * scale[0])); add y = f16(a + b) (y may be a);
 *   quantize_tensor / quantize_per_token: src_dtype TLLM_HALF or TLLM_FLOAT;
 *   embedding out[t] = table[ids[t]], an id outside [0, vocab) gives a zero row;
 *   gather_last_token out[b] = hidden[b, clamp(last_token_ids[b] - 1, 0, seq - 1)]; gather_rows out[b] = hidden[rows[b]];
 *   exclusive_scan_i32 cu[0] = 0, cu[i + 1] = cu[i] + lens[i] (cu holds n + 1);
 *   fill_random: dtype TLLM_HALF / TLLM_FLOAT (U(-scale, scale)), TLLM_INT8 ([-127, 127]), TLLM_FP8 (finite E4M3 codes, |x| < 2). */
int32_t tllm_swiglu(void* y, const void* a, const void* b, int64_t n, tllm_stream_t stream);
int32_t tllm_swiglu_quant(int8_t* q, const void* a, const void* b, int64_t n, const float* scale, tllm_stream_t stream);
int32_t tllm_add(void* y, const void* a, const void* b, int64_t n, tllm_stream_t stream);
int32_t tllm_quantize_tensor(int8_t* dst, const void* src, int32_t src_dtype, int64_t size, const float* scale, tllm_stream_t stream);
int32_t tllm_quantize_per_token(int8_t* dst, const void* src, int32_t src_dtype, int64_t rows, int64_t cols, float* scale_out,
    tllm_stream_t stream);
int32_t tllm_embedding(void* out, const int32_t* ids, const void* table, int64_t tokens, int32_t hidden, int32_t vocab,
    tllm_stream_t stream);
int32_t tllm_gather_last_token(void* out, const void* hidden, const int32_t* last_token_ids, int32_t batch, int32_t seq,
    int32_t hidden_size, tllm_stream_t stream);
int32_t tllm_gather_rows(void* out, const void* hidden, const int32_t* rows, int32_t batch, int32_t hidden_size, tllm_stream_t stream);
int32_t tllm_exclusive_scan_i32(int32_t* cu, const int32_t* lens, int32_t n, tllm_stream_t stream);
int32_t tllm_fill_i32(int32_t* dst, int32_t value, int64_t n, tllm_stream_t stream);
int32_t tllm_fill_random(void* dst, int32_t dtype, int64_t n, uint32_t seed, float scale, tllm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TLLM_RUNTIME_API_H */
