// The prefill schedule: the whole prompt batch through every layer as GEMMs on M = tokens rows, then the head on every
// sequence's last token.  Layer graph = Q/llama_model.py:78-119 (LLaMADecoderLayer.forward); head = :253-287.
//   RMSNorm (+ quantiser) -> QKV GEMM -> context attention (RoPE, cache fill) -> (quantiser) -> O GEMM + residual
//   RMSNorm (+ quantiser) -> fc / gate GEMMs + SwiGLU (+ quantiser), in as few launches as the mode allows -> down GEMM + residual
// SmoothQuant block template: SURVEY Appendix A.4 (the reference's SmoothQuant-LLaMA never ran; designed by analogy to
// PY/quantization/layer.py:385-439,596-852).
#include "session.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

int tllm_session::gemm(const Linear& L, int M, const void* a, void* c, int out_dtype, hipStream_t st, const void* residual,
    const void* silu_gate)
{
    const bool dyn = sq && per_token; // the activation's quantiser left one scale per row in qscale
    GemmParams g;
    g.residual = residual;
    g.silu_gate = silu_gate;
    g.wtype = L.wtype;
    g.out_dtype = out_dtype;
    g.M = M;
    g.N = L.N;
    g.K = L.K;
    g.a = a;
    g.lda = L.K;
    g.w = L.w;
    g.ldw = L.ldw;
    g.scale_col = L.scale_col;
    g.scale_row = dyn ? qscale : L.act_scale;
    g.per_channel = L.per_channel;
    g.per_token = dyn;
    g.c = c;
    g.ldc = L.N;
    return launch_gemm(g, st) ? 1 : 0;
}

// On-device tactic selection (kernels/gemm_tactics.hip; reference: int8_gemm_template.h:372-457, stored per M bucket in the
// plugin, smoothQuantGemmPlugin.cpp:253-282): the MFMA kernel of each prefill GEMM shape of this model at M rows is the one
// that measured fastest on THIS device - timed once per process and shape unless the engine file brought the choice along.
// TLLM_GEMM_TACTICS=off keeps the static rule.
int tllm_session::profile_prefill_gemms(int M)
{
    static const bool off = [] {
        const char* e = getenv("TLLM_GEMM_TACTICS");
        return e && (!strcmp(e, "off") || !strcmp(e, "0"));
    }();
    if (off || layers.empty() || packed) // packed inputs: M varies with the prompt batch, the nearest bucket entry serves
        return 0;
    const Layer& L = layers[0];
    // weight-only prefill runs gemm_woq.hip (one kernel per shape class, no tactic table)
    if (L.qkv.wtype == W_INT8_WOQ || L.qkv.wtype == W_INT4_WOQ)
        return 0;
    for (const Linear* l : {&L.qkv, &L.dense, &L.fc, &L.proj})
    {
        const int wt = l->wtype == W_INT8_SQ ? W_INT8_SQ : W_FP16;
        // an entry of the same power-of-two M bucket (what the engine file brought along, Builder._profile_gemm_tactics)
        // serves: the launcher would use it for this M anyway
        if (gemm_tactic_lookup(wt, M, l->N, l->K) > 0)
            continue;
        int cfg = 0;
        float us = 0.f;
        // best effort: a profile that cannot run (no memory left for its operands next to a large session) leaves the shape
        // to the static rule - it must not fail the set-up, nor leave its message behind for a later, unrelated failure
        if (gemm_profile(wt, M, l->N, l->K, &cfg, &us, nullptr))
        {
            set_error("%s", "");
            break;
        }
    }
    return 0;
}

// x -> RMSNorm(x) * gamma as the next GEMM's operand: fp16 in tmp, or (SmoothQuant) int8 in q8 with the static scale or one
// scale per row in qscale
int tllm_session::context_norm(int M, const void* gamma, const float* static_scale, hipStream_t st)
{
    RmsnormParams r;
    r.M = M;
    r.N = hidden;
    r.x = x;
    r.gamma = gamma;
    r.eps = eps;
    if (sq)
    {
        r.q = q8;
        if (per_token)
            r.dyn_scale_out = qscale;
        else
            r.static_scale = static_scale;
    }
    else
        r.y = tmp;
    return launch_rmsnorm(r, st);
}

int tllm_session::context_attention(const Layer& L, bool q_in_attn, hipStream_t st)
{
    ContextAttnParams c;
    c.batch = Bc;
    c.seq = max_in;
    c.num_heads = Hr;
    c.num_kv_heads = Hkvr;
    c.head_size = Dh;
    c.rotary_dim = Dh;
    c.neox = neox;
    c.inv_sqrt_dh = 1.f / sqrtf((float) Dh);
    c.kv_dtype = kv_dtype;
    c.max_seq_len = Smax;
    c.qkv = qkv;
    c.kv_cache = L.kv;
    c.input_lengths = in_len_ctx;
    c.cache_seq_stride = beam;
    c.block_pointers = L.kv_table;
    c.tokens_per_block = tokens_per_block;
    c.max_blocks_per_seq = max_blocks;
    c.kv_scale_orig_quant = L.kv_oq;
    c.rope_table = rope;
    c.rope_table_len = rope_len;
    c.out = ctx;
    c.workspace = ctx_ws;
    c.cu_seqlens = packed ? cu_dev : nullptr;
    if (q_in_attn)
    {
        c.out_q8 = q8;
        c.out_q_scale = L.attn_qscale;
    }
    return launch_context_attention(c, st);
}

// fc and gate on a_in, SwiGLU, and the down-projection's quantiser where the mode has one.  *p_in: where the result is
int tllm_session::context_gate_up(int li, int M, const void* a_in, const void** p_in, hipStream_t st)
{
    const Layer& L = layers[li];
    *p_in = inter_buf;
    if (sq && !per_token && M >= 32 && dual_mlp_cfg != 0)
    {
        // fc and gate in one kernel with SwiGLU + the static quantiser in its epilogue (gemm_sqp.hip, DUAL): the two fp16
        // [M, Ir] intermediates and the pointwise pass between the GEMMs disappear.  The int8 result goes to inter_buf
        // (q8 is this kernel's INPUT)
        GemmParams d;
        d.wtype = L.fc.wtype;
        d.out_dtype = DT_INT8;
        d.M = M;
        d.N = L.fc.N;
        d.K = L.fc.K;
        d.a = a_in;
        d.lda = L.fc.K;
        d.w = L.fc.w;
        d.ldw = L.fc.ldw;
        d.scale_col = L.fc.scale_col;
        d.scale_row = L.fc.act_scale;
        d.per_channel = L.fc.per_channel;
        d.per_token = 0;
        d.c = inter_buf;
        d.ldc = L.fc.N;
        d.w2 = L.gate.w;
        d.scale_col2 = L.gate.scale_col;
        d.scale_row2 = L.gate.act_scale;
        d.swiglu_qscale = L.mlp_qscale;
        if (L.gate.ldw == L.fc.ldw && L.gate.per_channel == L.fc.per_channel && L.gate.N == L.fc.N && L.gate.K == L.fc.K)
        {
            const int rc = launch_gemm_swiglu(d, st);
            if (rc < 0)
                return 1;
            if (rc == 0)
                return 0;
        }
    }
    RUN(gemm(L.fc, M, a_in, g, DT_HALF, st));
    if (lora_site_on(LS_GATE_UP))
    {
        // gate or up among the adapters' modules (never SmoothQuant): both projections in memory, the adapters on both, then SwiGLU
        RUN(gemm(L.gate, M, a_in, u, DT_HALF, st));
        RUN(lora_apply(li, LS_GATE_UP, M, a_in, PRO_NONE, nullptr, lora_rows, st));
        return launch_swiglu(inter_buf, g, u, (int64_t) M * Ir, st);
    }
    if (!sq)
    {
        // fp16 / weight-only: SwiGLU folded into the second projection's epilogue (g is read there instead of in a pass of
        // its own; same rounding points) - one launch and a [M, Ir] write + read fewer per layer
        return gemm(L.gate, M, a_in, inter_buf, DT_HALF, st, nullptr, g);
    }
    RUN(gemm(L.gate, M, a_in, u, DT_HALF, st));
    *p_in = q8;
    if (!per_token)
        return launch_swiglu_quant(q8, g, u, (int64_t) M * Ir, L.mlp_qscale, st); // SwiGLU and its quantiser in one pass
    RUN(launch_swiglu(inter_buf, g, u, (int64_t) M * Ir, st));
    return launch_quantize_per_token(q8, inter_buf, DT_HALF, M, Ir, qscale, st);
}

// x <- x + L(in): the residual rides in the GEMM's epilogue (same rounding: fp16(gemm) then fp16(sum)), or - tensor parallel,
// or a shape the epilogue does not serve - the partial sums go to tmp, through the all-reduce, and are added by a pass of its own
int tllm_session::context_proj_residual(const Linear& L, int M, const void* in, bool fuse_res, hipStream_t st)
{
    if (fuse_res)
        return gemm(L, M, in, x, DT_HALF, st, x);
    RUN(gemm(L, M, in, tmp, DT_HALF, st));
    RUN(allreduce(tmp, (int64_t) M * hidden, st));
    return launch_add(x, x, tmp, (int64_t) M * hidden, st);
}

// ------------------------------------------------------------------------------------------ one layer
// One decoder layer of the prefill schedule on the M rows of x.  append_n == 0: the prompt's layer (context attention);
// append_n > 0: the layer of an append pass on B * append_n rows (append attention onto the live cache, max_past as
// AppendAttnParams) - everything but the attention launch is the same code.
int tllm_session::context_layer(int li, int M, int append_n, int max_past, hipStream_t st)
{
    Layer& L = layers[li];
    const int D = hidden;
    const void* a_in = sq ? (const void*) q8 : tmp; // what context_norm leaves
    // (weight-only: gemm_woq.hip adds the residual in its epilogue too - same two roundings; its own serve conditions)
    const bool woq_w = L.dense.wtype == W_INT8_WOQ || L.dense.wtype == W_INT4_WOQ;
    const bool fuse_res = tp == 1 && !force_comm && M >= 32 && D % 8 == 0
        && (woq_w ? (L.dense.K % 64 == 0 && L.proj.K % 64 == 0)
                  : ((L.dense.wtype == W_INT8_SQ || L.dense.wtype == W_FP16)
                      && (L.dense.K * (L.dense.wtype == W_FP16 ? 2 : 1)) % 128 == 0
                      && (L.proj.K * (L.proj.wtype == W_FP16 ? 2 : 1)) % 128 == 0));
    // --- attention block
    RUN(context_norm(M, L.ln1, L.ln1_scale, st));
    RUN(gemm(L.qkv, M, a_in, qkv, DT_HALF, st));
    // LoRA: behind every base projection, on the rows' own adapters (lora_rows, derived per pass from the
    // selection).  tmp holds the normalised fp16 row the GEMM consumed; the expands update qkv, g / u and x in place.  append,
    // score and verify run this body and inherit the hooks
    RUN(lora_apply(li, LS_QKV, M, a_in, PRO_NONE, nullptr, lora_rows, st));
    // SmoothQuant static: the O-projection's input quantiser rides in the context attention's epilogue (padded inputs; with
    // packed inputs M counts real tokens only and the pass below covers exactly those).  The append attention has no such
    // epilogue: the quantiser pass follows it
    const bool q_in_attn = sq && !per_token && !packed && append_n == 0;
    if (append_n > 0)
        RUN(append_attention(L, append_n, max_past, st));
    else
        RUN(context_attention(L, q_in_attn, st));
    if (sq && per_token)
        RUN(launch_quantize_per_token(q8, ctx, DT_HALF, M, Dr, qscale, st));
    else if (sq && !q_in_attn)
        RUN(launch_quantize_tensor(q8, ctx, DT_HALF, (int64_t) M * Dr, L.attn_qscale, st));
    RUN(context_proj_residual(L.dense, M, sq ? (const void*) q8 : ctx, fuse_res, st));
    RUN(lora_apply(li, LS_DENSE, M, ctx, PRO_NONE, nullptr, lora_rows, st));
    // --- MLP block
    RUN(context_norm(M, L.ln2, L.ln2_scale, st));
    const void* p_in = nullptr; // inter_buf or q8, as the path through gate|up leaves it
    RUN(context_gate_up(li, M, a_in, &p_in, st));
    RUN(context_proj_residual(L.proj, M, p_in, fuse_res, st));
    RUN(lora_apply(li, LS_PROJ, M, p_in, PRO_NONE, nullptr, lora_rows, st));
    return 0;
}

// ------------------------------------------------------------------------------------------ context step
int tllm_session::run_context(hipStream_t st)
{
    const int S = max_in, M = packed ? ctx_tokens : Bc * S, D = hidden;
    RUN(launch_embedding(x, ids_in, emb, M, D, vocab, st));
    RUN(lora_map_rows(M, packed ? 0 : S, st));
    for (int li = 0; li < num_layers; ++li)
        RUN(context_layer(li, M, 0, 0, st));
    // head: last real token of every sequence -> ln_f -> lm_head -> fp32 logits  (Q/llama_model.py:272-279)
    if (packed)
        RUN(launch_gather_rows(last_hidden, x, last_rows, Bc, D, st));
    else
        RUN(launch_gather_last_token(last_hidden, x, last_tok, Bc, S, D, st));
    RUN(run_head(last_hidden, Bc, st));
    return 0;
}

// ------------------------------------------------------------------------------------------ append
int tllm_session::append_attention(const Layer& L, int n, int max_past, hipStream_t st)
{
    AppendAttnParams a;
    a.batch = B;
    a.n = n;
    a.num_heads = Hr;
    a.num_kv_heads = Hkvr;
    a.head_size = Dh;
    a.rotary_dim = Dh;
    a.neox = neox;
    a.inv_sqrt_dh = 1.f / sqrtf((float) Dh);
    a.kv_dtype = kv_dtype;
    a.max_seq_len = Smax;
    a.max_input_len = max_in;
    a.max_past = max_past;
    if (append_max_end > 0) // a ragged pass: the lengths are in append_last
    {
        a.n_per_seq = append_last;
        a.max_end = append_max_end;
    }
    a.qkv = qkv;
    a.kv_cache = L.kv;
    a.block_pointers = L.kv_table; // paged session (key paged_append): the pool and its table, as the prefill and the step take them
    a.tokens_per_block = tokens_per_block;
    a.max_blocks_per_seq = max_blocks;
    a.sequence_length = seq_len;
    a.input_lengths = in_len;
    a.masked_tokens = masked;
    a.kv_scale_orig_quant = L.kv_oq;
    a.kv_scale_quant_orig = L.kv_qo;
    a.rope_table = rope;
    a.rope_table_len = rope_len;
    a.out = ctx;
    const int kind = append_attention_kernel(Dh, n, APPEND_ATTN_RULE);
    RUN(launch_append_attention(a, st) ? 1 : 0);
    ++(kind == APPEND_ATTN_MFMA ? append_mfma_launches : append_wave_launches);
    return 0;
}

// n appended tokens per sequence (their ids in ids_in, [B, n]) through every layer on M = B * n rows: the body of an append pass
// and of a verify pass.  sequence_length is read by every layer's attention and not written.
int tllm_session::append_layers(int n, int max_past, hipStream_t st)
{
    const int M = B * n;
    RUN(launch_embedding(x, ids_in, emb, M, hidden, vocab, st));
    RUN(lora_map_rows(M, n, st));
    for (int li = 0; li < num_layers; ++li)
        RUN(context_layer(li, M, n, max_past, st));
    return 0;
}

// ... and the head on row n - 1 of every sequence.  The caller advances sequence_length afterwards.
int tllm_session::run_append(int n, int max_past, hipStream_t st)
{
    RUN(append_layers(n, max_past, st));
    // row n - 1 of every sequence (append_last holds n for every sequence: the padded-layout gather takes row last - 1)
    RUN(launch_fill_i32(append_last, n, B, st));
    RUN(launch_gather_last_token(last_hidden, x, append_last, B, n, hidden, st));
    RUN(run_head(last_hidden, B, st));
    return 0;
}

// The pass on B * n rows, n = max_b n_b, with the lengths n_b in append_last (uploaded by the caller): the attention takes them as
// n_per_seq, the head runs on row n_b - 1 of every sequence.
int tllm_session::run_append_ragged(int n, int max_end, hipStream_t st)
{
    append_max_end = max_end;
    const int rc = append_layers(n, 0, st);
    append_max_end = 0;
    RUN(rc);
    RUN(launch_gather_last_token(last_hidden, x, append_last, B, n, hidden, st));
    RUN(run_head(last_hidden, B, st));
    return 0;
}

// ------------------------------------------------------------------------------------------ verify
// The buffers of a verify pass, sized for kVerifyMaxTokens ids per sequence; allocated by the first one after a setup.
int tllm_session::verify_buffers()
{
    if (verify.logits)
        return 0;
    VerifyBuffers vb;
    const size_t rows = (size_t) B * kVerifyMaxTokens;
    RUN(dalloc(&vb.logits, rows * Vr * 4));
    RUN(dalloc(&vb.targets, rows * 4));
    RUN(dalloc(&vb.rec, rows * 8 * 4));
    RUN(dalloc(&vb.log_probs, rows * 4));
    RUN(dalloc(&vb.top1, rows * 4));
    RUN(dalloc(&vb.draws, rows * 4));
    RUN(dalloc(&vb.accepted, (size_t) B * 4));
    RUN(dalloc(&vb.limit, (size_t) B * 4));
    RUN(dalloc(&vb.state, (size_t) B * 4 * 4));
    verify = vb;
    return 0;
}

// run_append's layers, then every one of the B * n final hidden rows through the head: row (b, i) is the distribution behind
// ids[b][0..i].  The rows are scored against the next id of their sequence (top1 = the arg-max the accept rule compares the
// drafts with, log_probs for the caller) and the accept step commits the longest right prefix in the sampler's place
// (kernels.h SpecAcceptParams).  sequence_length is read by every layer's attention and written by the accept step alone.
// A sampled pass (kernels.h SpecSampleParams) puts one launch between the scoring and the accept step: the
// sampler on all R rows, each with the history and the token number plain sampled decoding would have had there, and the accept
// step compares the drafts with those draws.  log_probs stay the raw model's.  Under a configuration that is plain arg-max (or
// none) that launch is not made: the pass is the greedy one.
int tllm_session::run_verify(int n, int max_past, const int32_t* limit, bool sampled, hipStream_t st)
{
    const int R = B * n;
    RUN(verify_buffers());
    verify_n = n;
    RUN(append_layers(n, max_past, st));
    RUN(head_norm(x, R, st));
    RUN(head_gemm_f32(tmp, R, verify.logits, st));
    RUN(launch_spec_targets(verify.targets, ids_in, B, n, st) ? 1 : 0);
    TokenLogprobParams p;
    p.logits = verify.logits;
    p.ld = Vr;
    p.rows = R;
    p.vocab_part = Vr;
    p.vocab = vocab;
    p.targets = verify.targets;
    p.partials = verify.rec;
    RUN(launch_token_logprob_partial(p, st) ? 1 : 0);
    RUN(launch_token_logprob_merge(verify.rec, 1, R, vocab, verify.targets, verify.log_probs, nullptr, verify.top1, st) ? 1 : 0);
    head_partials_live = false; // the session's logits are a copied row from here on, no head launch's partials belong to them
    logit_rows = B;
    verify_cmp = verify.top1;
    if (sampled && sampling_on && !sampling_is_greedy(sampling))
    {
        SpecSampleParams sp;
        sp.s = sampling;
        sp.s.g = greedy_params();
        sp.s.g.logits = verify.logits;
        sp.s.history = out_ids;
        sp.s.history_stride = Smax;
        sp.s.g_base = max_in;
        sp.n = n;
        sp.ids = ids_in;
        sp.limit = limit;
        sp.draws = verify.draws;
        RUN(launch_spec_sample_rows(sp, st) ? 1 : 0);
        verify_cmp = verify.draws;
    }
    SpecAcceptParams a;
    a.g = greedy_params();
    a.g.logits = verify.logits;
    a.n = n;
    a.ids = ids_in;
    a.top1 = verify_cmp;
    a.limit = limit;
    a.accepted = verify.accepted;
    a.logits_out = logits_local;
    return launch_spec_accept(a, st) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ the head on many rows
int tllm_session::head_norm(const void* h, int R, hipStream_t st)
{
    RmsnormParams r;
    r.M = R;
    r.N = hidden;
    r.x = h;
    r.gamma = lnf;
    r.eps = eps;
    r.y = tmp; // [Bc * S, D] fp16, free between the last layer and the next call
    return launch_rmsnorm(r, st);
}

int tllm_session::head_gemm_f32(const void* a, int rows, float* out, hipStream_t st)
{
    GemmParams g;
    g.wtype = head.wtype;
    g.out_dtype = DT_FLOAT;
    g.M = rows;
    g.N = head.N;
    g.K = head.K;
    g.a = a;
    g.lda = hidden;
    g.w = head.w;
    g.ldw = head.ldw;
    g.scale_col = head.scale_col;
    g.per_channel = head.per_channel;
    g.c = out;
    g.ldc = Vr;
    return launch_gemm(g, st) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------ scoring
// The log-probability of every prompt token that has a predecessor.  Row (b, t) of x, t < len_b - 1, is the final hidden state
// after ids[b][0..t]; it predicts ids[b][t + 1].  Only those rows go through the head: gathered -> ln_f (fp16 in tmp, the kernel
// itself: context_norm would quantise in a SmoothQuant session) -> lm_head as a prefill GEMM with fp32 output, one chunk of rows
// at a time -> kernels/token_logprob.hip on the chunk.  The [rows, Vr] logits exist one chunk at a time and stay on the device.
int tllm_session::score_enqueue(const int32_t* input_ids, const int32_t* input_lengths, hipStream_t st)
{
    const int S = max_in, D = hidden;
    std::vector<int32_t> src, tgt;
    score_pos.clear();
    int packed_base = 0;
    for (int b = 0; b < Bc; ++b)
    {
        const int len = input_lengths[b]; // upload_prompt has checked the range
        const int base = packed ? packed_base : b * S;
        for (int t = 0; t + 1 < len; ++t)
        {
            src.push_back(base + t);
            tgt.push_back(input_ids[(size_t) b * S + t + 1]);
            score_pos.push_back(b * S + t + 1);
        }
        packed_base += len;
    }
    const int R = (int) src.size();
    score_lp_host.assign(R, 0.f);
    score_top_host.assign(R, -1);
    if (R == 0)
        return 0;
    const bool gather = (tp > 1 || force_comm) && !no_comm;
    if (!score.logits)
    {
        ScoreBuffers sb;
        sb.max_rows = Bc * (S - 1);
        int chunk = score_chunk_cfg > 0 ? score_chunk_cfg : std::max(32, (int) (((size_t) 64 << 20) / ((size_t) Vr * 4) / 32 * 32));
        sb.chunk = std::min(chunk, sb.max_rows);
        RUN(dalloc(&sb.hidden, (size_t) sb.max_rows * D * 2));
        RUN(dalloc(&sb.logits, (size_t) sb.chunk * Vr * 4));
        RUN(dalloc(&sb.src_rows, (size_t) sb.max_rows * 4));
        RUN(dalloc(&sb.targets, (size_t) sb.max_rows * 4));
        RUN(dalloc(&sb.rec_local, (size_t) sb.max_rows * 8 * 4));
        if (gather)
            RUN(dalloc(&sb.rec_all, (size_t) tp * sb.max_rows * 8 * 4));
        RUN(dalloc(&sb.log_probs, (size_t) sb.max_rows * 4));
        RUN(dalloc(&sb.top1, (size_t) sb.max_rows * 4));
        score = sb;
    }
    HIP_OK(hipMemcpyAsync(score.src_rows, src.data(), (size_t) R * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(score.targets, tgt.data(), (size_t) R * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); // src / tgt go out of scope
    RUN(launch_gather_rows(score.hidden, x, score.src_rows, R, D, st));
    RUN(head_norm(score.hidden, R, st));
    for (int r0 = 0; r0 < R; r0 += score.chunk)
    {
        const int rows = std::min(score.chunk, R - r0);
        RUN(head_gemm_f32(static_cast<const char*>(tmp) + (size_t) r0 * D * 2, rows, score.logits, st));
        TokenLogprobParams p;
        p.logits = score.logits;
        p.ld = Vr;
        p.rows = rows;
        p.first_part = rank; // this rank's vocabulary shard: ids [rank * Vr, min(vocab, (rank + 1) * Vr))
        p.vocab_part = Vr;
        p.vocab = vocab;
        p.targets = score.targets + r0;
        p.partials = score.rec_local + (size_t) r0 * 8;
        if (launch_token_logprob_partial(p, st))
            return 1;
    }
    const float* rec = score.rec_local;
    if (gather)
    {
        // 32 bytes per row and rank instead of the rank's logits: the choice of transport is run_head's
        const int64_t bytes = (int64_t) R * 8 * 4;
        if (comm::p2p::usable(tp, bytes))
        {
            if (comm::p2p::all_gather(score.rec_local, score.rec_all, bytes, st))
                return 1;
        }
        else if (comm::all_gather(group, score.rec_local, score.rec_all, (int64_t) R * 8, TLLM_FLOAT, st))
            return 1;
        rec = score.rec_all;
    }
    // (no_comm: a timing-only session merges its own shard alone)
    if (launch_token_logprob_merge(rec, gather ? tp : 1, R, vocab, score.targets, score.log_probs, nullptr, score.top1, st))
        return 1;
    HIP_OK(hipMemcpyAsync(score_lp_host.data(), score.log_probs, (size_t) R * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(score_top_host.data(), score.top1, (size_t) R * 4, hipMemcpyDeviceToHost, st));
    return 0;
}

void tllm_session::score_collect(float* log_probs, int32_t* top1_ids)
{
    const size_t n = (size_t) Bc * max_in;
    std::fill(log_probs, log_probs + n, 0.f);
    if (top1_ids)
        std::fill(top1_ids, top1_ids + n, -1);
    for (size_t k = 0; k < score_pos.size(); ++k)
    {
        log_probs[score_pos[k]] = score_lp_host[k];
        if (top1_ids)
            top1_ids[score_pos[k]] = score_top_host[k];
    }
}
