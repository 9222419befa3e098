// The generation-step schedule of the LLaMA path (include/tllm_runtime_api.h).
//
// What the reference does with a TensorRT engine + two execution contexts + a Python loop that syncs with the device
// every step (PY/runtime/generation.py:852-983), this does with the plugin kernels enqueued layer by layer on one HIP
// stream and a step whose step-dependent scalars (sequence length, current token, finished flags, RoPE row) live in
// device memory - so one captured hipGraph is replayed for every step and the host never waits inside the loop.
//
// Layer graph = Q/llama_model.py:78-119 (LLaMADecoderLayer.forward).  What TensorRT/Myelin fuses out of pointwise layers is
// fused here by construction; one layer of a step is, in the form a batch-1 greedy session on one GPU runs by default,
// THREE launches:
//   front    RMSNorm (+ quant) -> QKV projection -> RoPE + KV append -> split-KV attention + merge
//            -> (quant) O-projection + residual                                        stage_front   (qkv_attn_fused.hip)
//   gate|up  RMSNorm (+ quant) -> fc, gate GEMV -> silu * mul (+ quant)                stage_gate_up (gemv prologue / epilogue)
//   down     (quant) -> proj GEMV -> + residual                                        stage_down    (gemv prologue / epilogue)
// and every other shape (batch, beam, paged cache, tensor parallel) or session key that switches a fusion off runs the same
// computation through more launch sites, chosen once at setup (tllm_session::decide_decode_form):
//   !o_fused         front without its third stage, then stage_o_proj  (quant) -> O GEMV -> + residual
//   !qkv_attn_fused  stage_qkv (RMSNorm (+ quant) -> QKV GEMV), stage_attention (mmha_decode.hip), stage_o_proj
//   mlp_fused_dec    gate|up + down as one launch, stage_mlp_one (mlp_fused.hip)
// Tensor parallel: stage_seam after each row-parallel projection - an all-reduce of x, or over the peer-to-peer transport
// all-reduce + residual + the next RMSNorm (+ quant) in one launch (p2p_allreduce.hip), which the next GEMV then consumes as is.
// Behind the layers: run_head (ln_f -> lm_head -> logits all-gather) and run_sampler (greedy / sampling / beam step, which also
// leaves the next step's input row and RoPE row).
#include "session.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

// ------------------------------------------------------------------------------------------ launch wrappers
int tllm_session::gemv(const Linear& L, int M, int pro, int epi, const void* xin, int64_t ldx, const void* gamma,
    const float* in_qscale, const void* residual, const float* epi_scale, void* y, int64_t ldy, int out_dtype, const Linear* up,
    hipStream_t st, const float* row_scales, void* tap)
{
    GemvParams p;
    p.wtype = L.wtype;
    p.pro = pro;
    p.epi = epi;
    p.out_dtype = out_dtype;
    p.M = M;
    p.N = L.N;
    p.K = L.K;
    p.x = xin;
    p.ldx = ldx;
    p.w = L.w;
    p.ldw = L.ldw;
    p.scale_col = L.scale_col;
    p.scale_row = L.act_scale;
    p.per_channel = L.per_channel;
    p.per_token = 0;
    if (row_scales) // activations quantised per token upstream (the fused all-reduce tail): one dequantisation scale per row
    {
        p.scale_row = row_scales;
        p.per_token = 1;
    }
    p.gamma = gamma;
    p.eps = eps;
    p.act_scale = in_qscale;
    p.residual = residual;
    p.epi_scale = epi_scale;
    p.y = y;
    p.ldy = ldy;
    p.x_pro_out = tap;
    p.resident_rows = gemv_resident_rows;
    p.argmax_part = gemv_argmax_part;
    if (up)
    {
        p.w_up = up->w;
        p.scale_col_up = up->scale_col;
        p.scale_row_up = up->act_scale;
    }
    if (M <= 8)
        return timed(gemv_cls, st, [&] { return launch_gemv(p, st) ? 1 : 0; });
    // more than 8 sequences (batch x beam width): the skinny kernel takes 8 rows per launch, so the rows go through it in
    // slabs of 8 - every operand that is indexed by the row moves along.  Each slab streams the weights again: beyond 8
    // sequences a step costs ceil(B / 8) weight passes (the throughput per sequence of B = 8), but nothing is refused -
    // build.py's default --max_batch_size 8 with any beam width > 1 asks for exactly this (Q/build.py:73-76).
    const int xes = (L.wtype == W_INT8_SQ && pro == PRO_NONE) ? 1 : 2; // raw s8 activations, else fp16
    const int yes = out_dtype == DT_INT8 ? 1 : (out_dtype == DT_HALF ? 2 : 4);
    const int tap_es = L.wtype == W_INT8_SQ ? 1 : 2;
    return timed(gemv_cls, st, [&] {
        for (int m0 = 0; m0 < M; m0 += 8)
        {
            GemvParams q = p;
            q.M = M - m0 < 8 ? M - m0 : 8;
            q.x = static_cast<const char*>(xin) + (int64_t) m0 * ldx * xes;
            q.y = static_cast<char*>(y) + (int64_t) m0 * ldy * yes;
            if (residual)
                q.residual = static_cast<const char*>(residual) + (int64_t) m0 * ldy * 2;
            if (p.per_token && p.scale_row)
                q.scale_row = p.scale_row + m0;
            if (p.x_pro_out)
                q.x_pro_out = static_cast<char*>(p.x_pro_out) + (int64_t) m0 * L.K * tap_es;
            if (launch_gemv(q, st))
                return 1;
        }
        return 0;
    });
}

int tllm_session::allreduce(void* buf, int64_t n, hipStream_t st)
{
    if ((tp == 1 && !force_comm) || no_comm)
        return 0;
    if (comm::p2p::usable(tp, n * 2))
        return timed(PC_COMM, st, [&] { return comm::p2p::all_reduce_f16(buf, n, st) ? 1 : 0; });
    // a vector longer than one inbox slot (the prefill's [tokens, D] partial sums) goes through the peer-to-peer path in
    // slot-sized pieces - the same kernel, one epoch per piece - instead of silently needing a second transport
    // (only when no RCCL communicator exists for the group: the one-workgroup exchange kernel is built for the decode
    // step's 8 KB vectors, a ring is the better transport for the prefill's megabytes)
    const int64_t cap = comm::p2p::slot_capacity(tp) / 2 / 8 * 8; // fp16 elements per exchange, whole 16-byte vectors
    if (cap > 0 && n % 8 == 0 && !comm::has_comm(group))
    {
        static bool warned = false;
        if (!warned && n > 8 * cap)
        {
            warned = true;
            fprintf(stderr, "[tllm] warning: a %lld-element all-reduce goes through the peer-to-peer inbox in %lld pieces of %lld "
                            "(no RCCL communicator is registered for this group): register one (tllm_comm_init_rank) or size the inbox "
                            "(tllm_comm_p2p_create max_bytes) for the prefill\n",
                (long long) n, (long long) ((n + cap - 1) / cap), (long long) cap);
        }
        return timed(PC_COMM, st, [&] {
            for (int64_t off = 0; off < n; off += cap)
                if (comm::p2p::all_reduce_f16(static_cast<char*>(buf) + off * 2, n - off < cap ? n - off : cap, st))
                    return 1;
            return 0;
        });
    }
    return timed(PC_COMM, st, [&] { return comm::all_reduce_sum(group, buf, buf, n, TLLM_HALF, st) ? 1 : 0; });
}

// ln_f -> lm_head -> fp32 logits of this rank's vocabulary shard (-> all-gather)
int tllm_session::run_head(const void* h, int rows, hipStream_t st, bool normalised)
{
    logit_rows = rows;
    gemv_cls = PC_GEMV_HEAD;
    // one row: the launch of a batch-1 step (and of a single prompt) - the instance that takes the two lm_head options
    const bool one_row = rows == 1 && head.wtype == W_FP16;
    const bool greedy = beam == 1 && !(sampling_on && !sampling_is_greedy(sampling));
    head_partials_live = one_row && greedy && B == 1 && tp == 1 && !force_comm && greedy_partials_cfg != 0 && argmax_part;
    gemv_resident_rows = one_row ? head_resident_rows : 0;
    gemv_argmax_part = head_partials_live ? argmax_part : nullptr;
    const int head_rc = gemv(head, rows, normalised ? PRO_NONE : PRO_RMSNORM, EPI_NONE, h, hidden, lnf, nullptr, nullptr, nullptr,
        logits_local, Vr, DT_FLOAT, nullptr, st);
    gemv_resident_rows = 0;
    gemv_argmax_part = nullptr;
    gemv_cls = PC_GEMV_LAYER;
    if (head_rc)
        head_partials_live = false;
    RUN(head_rc);
    if ((tp > 1 || force_comm) && !no_comm)
    {
        const int64_t bytes = (int64_t) rows * Vr * 4;
        if (comm::p2p::usable(tp, bytes))
        {
            if (comm::p2p::all_gather(logits_local, logits, bytes, st))
                return 1;
        }
        else if (comm::all_gather(group, logits_local, logits, (int64_t) rows * Vr, TLLM_FLOAT, st))
            return 1;
    }
    return 0;
}

// the session's logits, step words and next-step buffers as a sampler launch takes them (greedy, top-k / top-p or accept step)
GreedyParams tllm_session::greedy_params()
{
    GreedyParams gp;
    gp.logits = (tp > 1 || force_comm) ? logits : logits_local;
    gp.batch = B;
    gp.vocab_part = Vr;
    gp.nparts = tp;
    gp.vocab = vocab;
    gp.cur_ids = cur_ids;
    gp.out_ids = out_ids;
    gp.out_stride = Smax;
    gp.seq_len = seq_len;
    gp.finished = finished;
    gp.end_id = end_id;
    gp.rope_row_out = rope_row;
    gp.rope_pos_out = rope_pos;
    gp.step_epoch = step_epoch;
    gp.rope_table = rope;
    gp.rope_half = Dh / 2;
    gp.rope_table_len = rope_len;
    gp.input_lengths = in_len;
    gp.max_input_len = max_in;
    if (hidden % 8 == 0)
    {
        gp.emb_table = emb; // the sampler leaves the next step's input row in x (run_decode_step skips its embedding launch)
        gp.x_out = x;
        gp.hidden = hidden;
    }
    return gp;
}

int tllm_session::run_sampler(int advance, hipStream_t st)
{
    // the partials belong to the logits of the head launch just before this sampler, and to no later one
    const bool partials = head_partials_live;
    head_partials_live = false;
    if (beam > 1)
    {
        BeamParams bp;
        bp.logits = (tp > 1 || force_comm) ? logits : logits_local;
        bp.logits_per_batch = advance ? 0 : 1;
        bp.batch = Bc;
        bp.beam = beam;
        bp.vocab_part = Vr;
        bp.nparts = tp;
        bp.vocab = vocab;
        bp.cum_log_probs = cum_log_probs;
        bp.cur_ids = cur_ids;
        bp.out_ids = out_ids;
        bp.parent_ids = parent_ids;
        bp.out_stride = Smax;
        bp.seq_len = seq_len;
        bp.finished = finished;
        bp.end_id = end_id;
        bp.advance = advance;
        bp.cache_indirection = cache_ind;
        bp.rope_row_out = rope_row;
        bp.rope_pos_out = rope_pos;
        bp.rope_table = rope;
        bp.rope_half = Dh / 2;
        bp.rope_table_len = rope_len;
        bp.input_lengths = in_len;
        bp.max_input_len = max_in;
        return timed(PC_OTHER, st, [&] { return launch_beam_step(bp, st) ? 1 : 0; });
    }
    GreedyParams gp = greedy_params();
    gp.advance = advance;
    if (sampling_on && !sampling_is_greedy(sampling))
    {
        // same logits (gathered shards included), same bookkeeping; every tensor-parallel rank draws the same token
        SamplingParams sp = sampling;
        sp.g = gp;
        sp.history = out_ids;
        sp.history_stride = Smax;
        sp.g_base = max_in;
        return timed(PC_OTHER, st, [&] { return launch_sampling_step(sp, st) ? 1 : 0; });
    }
    if (partials && B == 1 && tp == 1 && !force_comm) // every other shape scans the logits
    {
        gp.argmax_part = argmax_part;
        ++greedy_partials_used;
    }
    return timed(PC_OTHER, st, [&] { return launch_greedy_step(gp, st) ? 1 : 0; });
}

// ------------------------------------------------------------------------------------------ generation step
// What is fixed for one call of run_decode_step: the tensor-parallel seam, the operand types, and which launch sites the call
// issues.  All of tllm_session_time_kernel's ids are interpreted here and nowhere else.
struct tllm_session::DecodeStep
{
    hipStream_t st;
    // only_kernel < 0: a whole step (embedding, every stage, seams, head, sampler).  Otherwise just the launch site of that id
    // in every layer, eagerly, outside a step:
    //   1 QKV GEMV - or the fused front in its two-stage form     2 attention     4 O-projection GEMV     5 gate|up GEMV
    //   6 down GEMV     7 the fused front exactly as the step runs it     8 the one-launch MLP
    // (id 1 runs the front's third stage too - front_o - while the stage clock is on, fused_timing: see plan_decode_step)
    bool whole;
    bool taps; // debug_taps, whole steps only
    // Tensor parallel over the peer-to-peer transport: the layer seam  all-reduce -> residual add -> next RMSNorm (-> quantiser)
    // is ONE launch (kernels/p2p_allreduce.hip fused tail; reference seam: PY/quantization/layer.py:215,377 allreduce,
    // Q/llama_model.py:107-118 adds, PY/layers/normalization.py:33-54).  The row-parallel GEMVs then write their bare partial
    // sums, every rank adds the residual itself (no rank is special), and the consuming GEMV starts from its operand type.
    // RCCL (or TLLM_NO_FUSED_ALLREDUCE=1) keeps the three-stage path: rank 0 carries the residual, the consumers normalise.
    bool fused_ar;
    int ar_quant;          // the seam's quantiser: 0 none, 1 static, 2 per token
    const float* ar_rows;  // per-token scales behind the fused quantiser
    int epi_res;           // epilogue of a row-parallel GEMV outside the fused seam: the residual rides on one rank only
    int pro_norm, pro_q;   // GEMV prologues: RMSNorm (+ quantiser) | quantiser alone, in this session's quantisation mode
    bool q_inter;          // the SwiGLU epilogue quantises: the down-projection reads int8 from q8, else fp16 from inter_buf
    bool tail_q8;          // the attention's in-launch merge leaves the O-projection's int8 operand in ctx_q8
    // launch sites of this call
    bool front, front_o, qkv, attn, o_proj, mlp_one, gate_up, down;
};

tllm_session::DecodeStep tllm_session::plan_decode_step(hipStream_t st)
{
    DecodeStep ds;
    ds.st = st;
    const int ok = only_kernel;
    ds.whole = ok < 0;
    auto on = [&](int id) { return ds.whole || ok == id; };
    ds.taps = debug_taps && ds.whole;
    // decided ONCE per step (layers and head must take the same branch) from the transport's own state: the verdict of the
    // caller's validation lives in comm::p2p (tllm_comm_p2p_enable_fused), not in a process-wide cached getenv;
    // TLLM_NO_FUSED_ALLREDUCE=1 stays as the user's A/B switch and is read per step
    ds.fused_ar = tp > 1 && !getenv("TLLM_NO_FUSED_ALLREDUCE") && hidden % 8 == 0
        && comm::p2p::usable_fused(tp, (int64_t) B * hidden * 2);
    ds.ar_quant = !sq ? 0 : (per_token ? 2 : 1);
    ds.ar_rows = (sq && per_token) ? ar_scale : nullptr;
    ds.epi_res = (tp == 1 || rank == 0) ? EPI_RESIDUAL : EPI_NONE;
    ds.pro_norm = !sq ? PRO_RMSNORM : (per_token ? PRO_RMSNORM_QDYN : PRO_RMSNORM_QSTATIC);
    ds.pro_q = !sq ? PRO_NONE : (per_token ? PRO_QDYN : PRO_QSTATIC);
    ds.q_inter = sq && !per_token;
    ds.tail_q8 = attn_plan.in_launch_merge && sq && !per_token;
    // (kernel-timing id 1 measures the front's two-stage form, id 7 the launch exactly as the step runs it; with the stage clock
    //  on, the three-stage form is what id 1 looks at too - x is overwritten by every timed launch: the timer restores it)
    ds.front = qkv_attn_fused && (on(1) || ok == 7);
    ds.front_o = ds.front && o_fused && (ds.whole || ok == 7 || fused_timing);
    ds.qkv = !qkv_attn_fused && on(1);
    ds.attn = !qkv_attn_fused && on(2);
    ds.o_proj = on(4) && !(ds.whole && qkv_attn_fused && o_fused); // (a whole step: the front's third stage did it)
    ds.mlp_one = mlp_fused_dec && !ds.fused_ar && on(8);
    ds.gate_up = !ds.mlp_one && on(5);
    ds.down = !ds.mlp_one && on(6);
    return ds;
}

// a tap whose GEMV does not transform its input: the input itself, copied
int tllm_session::tap_copy(const DecodeStep& ds, int which, int li, const void* src, int elem_bytes)
{
    HIP_OK(hipMemcpyAsync(tap_ptr(which, li), src, (size_t) B * tap_width(which) * elem_bytes, hipMemcpyDeviceToDevice, ds.st));
    return 0;
}

// K1 + K2 + K3 in one launch (kernels/qkv_attn_fused.hip), with the O-projection + residual as its third stage (front_o)
int tllm_session::stage_front(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    hipStream_t st = ds.st;
    FusedQkvAttnParams f;
    f.K = hidden;
    f.num_heads = Hr;
    f.head_size = Dh;
    f.x = x;
    f.gamma = L.ln1;
    f.eps = eps;
    f.w = L.qkv.w;
    f.ldw = L.qkv.ldw;
    f.scale_col = L.qkv.scale_col;
    f.per_channel = L.qkv.per_channel;
    f.wtype = L.qkv.wtype;
    f.act_quant_scale = (per_token || !sq) ? nullptr : L.ln1_scale;
    f.act_dequant_scale = (per_token || !sq) ? nullptr : L.qkv.act_scale;
    f.kv_dtype = kv_dtype;
    f.max_seq_len = Smax;
    f.inv_sqrt_dh = 1.f / sqrtf((float) Dh);
    f.kv_cache = L.kv;
    f.sequence_length = seq_len;
    f.masked_tokens = masked;
    f.kv_scale_orig_quant = L.kv_oq;
    f.kv_scale_quant_orig = L.kv_qo;
    f.rope_row = rope_row;
    f.xchg = fused_xchg;
    f.epoch = step_epoch;
    f.tag_mul = (uint32_t) num_layers + 1;
    f.tag_add = (uint32_t) li + 1;
    if (!ds.whole) // eager launches outside a step: the epoch does not advance between them
        f.tag_host = 1u + (++timing_tag & 0x3fffffffu); // (the kernel sets the top bit: host tags never meet step tags)
    f.error = fused_err;
    if (fused_max_spins >= 0)
        f.max_spins = fused_max_spins;
    f.qkv_out = qkv;
    f.out = ctx;
    if (sq && !per_token)
    {
        f.out_q8 = ctx_q8;
        f.out_quant_scale = L.attn_qscale;
    }
    f.x_pro_out = ds.taps ? tap_ptr(0, li) : nullptr;
    f.timing = fused_timing;
    if (ds.front_o)
    {
        f.o_w = L.dense.w;
        f.o_ldw = L.dense.ldw;
        f.o_n = L.dense.N;
        f.o_per_channel = L.dense.per_channel;
        f.o_scale_col = L.dense.scale_col;
        f.o_scale_row = L.dense.act_scale;
        f.x_out = x;
    }
    RUN(timed(PC_ATTENTION, st, [&] { return launch_qkv_attn_fused(f, st) ? 1 : 0; }));
    if (ds.taps && ds.front_o) // x already holds x + O(ctx); the third stage read the context row as the launch left it
        RUN(tap_copy(ds, 1, li, sq ? (const void*) ctx_q8 : ctx, sq ? 1 : 2));
    return 0;
}

// K1: RMSNorm (+ quant) -> QKV GEMV
int tllm_session::stage_qkv(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    if (ds.fused_ar && li > 0)
    {
        // the previous layer's seam left input_layernorm's output (quantised for SmoothQuant) in ar_norm
        if (ds.taps)
            RUN(tap_copy(ds, 0, li, ar_norm, sq ? 1 : 2));
        return gemv(L.qkv, B, PRO_NONE, EPI_NONE, ar_norm, hidden, nullptr, nullptr, nullptr, nullptr, qkv, QKVr, DT_HALF, nullptr,
            ds.st, ds.ar_rows);
    }
    RUN(gemv(L.qkv, B, ds.pro_norm, EPI_NONE, x, hidden, L.ln1, L.ln1_scale, nullptr, nullptr, qkv, QKVr, DT_HALF, nullptr,
        ds.st, nullptr, ds.taps ? tap_ptr(0, li) : nullptr));
    // LoRA (tp 1, no SmoothQuant): the GEMV normalised x inside its prologue and left no fp16 row, so the shrink normalises again
    // with the same rounding points; the expand updates qkv in place, ahead of RoPE and the cache write
    return lora_apply(li, LS_QKV, B, x, PRO_RMSNORM, L.ln1, lora_sel, ds.st);
}

// K2 / K3: RoPE + KV append + split-KV attention, merged in the launch (attn_plan.in_launch_merge) or by its combine launch
int tllm_session::stage_attention(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    hipStream_t st = ds.st;
    MmhaParams m;
    m.batch = B;
    m.num_heads = Hr;
    m.num_kv_heads = Hkvr;
    m.head_size = Dh;
    m.rotary_dim = Dh;
    m.neox = neox;
    m.inv_sqrt_dh = 1.f / sqrtf((float) Dh);
    m.kv_dtype = kv_dtype;
    m.max_seq_len = Smax;
    m.max_input_len = max_in;
    m.qkv = qkv;
    m.kv_cache = L.kv;
    m.sequence_length = seq_len;
    m.input_lengths = in_len;
    m.masked_tokens = masked;
    m.timestep_host = -1; // device-resident step state: one graph serves every step
    m.kv_scale_orig_quant = L.kv_oq;
    m.kv_scale_quant_orig = L.kv_qo;
    m.rope_table = rope;
    m.rope_table_len = rope_len;
    m.rope_row = rope_row;
    m.cache_indirection = beam > 1 ? cache_ind : nullptr;
    m.beam_width = beam;
    m.block_pointers = L.kv_table;
    m.tokens_per_block = tokens_per_block;
    m.max_blocks_per_seq = max_blocks;
    if (ds.tail_q8)
    {
        m.tail_out_q8 = ctx_q8;
        m.tail_quant_scale = L.attn_qscale;
    }
    m.out = ctx;
    RUN(mmha_bind_workspace(m, attn_plan, mmha_ws, false, st)); // (the tickets: zero since setup / the prompt, re-armed by every launch)
    return timed(PC_ATTENTION, st, [&] { return launch_mmha(m, st); });
}

// K4: x <- x + O(ctx)     (TP: rank 0 carries the residual into the all-reduce, or the fused seam adds it)
int tllm_session::stage_o_proj(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    // (tail merge + static SmoothQuant: the attention launch left the int8 operand itself - no prologue at all)
    const void* o_in = ds.tail_q8 ? ctx_q8 : ctx;
    const int pro = ds.tail_q8 ? (int) PRO_NONE : ds.pro_q;
    void* tap = nullptr;
    if (ds.taps && pro == PRO_NONE) // nothing is transformed in the prologue: the input itself is the tap
        RUN(tap_copy(ds, 1, li, o_in, ds.tail_q8 ? 1 : 2));
    else if (ds.taps)
        tap = tap_ptr(1, li);
    if (ds.fused_ar)
        return gemv(L.dense, B, pro, EPI_NONE, o_in, Dr, nullptr, L.attn_qscale, nullptr, nullptr, ar_partial, hidden, DT_HALF,
            nullptr, ds.st, nullptr, tap);
    RUN(gemv(L.dense, B, pro, ds.epi_res, o_in, Dr, nullptr, L.attn_qscale, x, nullptr, x, hidden, DT_HALF, nullptr, ds.st,
        nullptr, tap));
    return lora_apply(li, LS_DENSE, B, ctx, PRO_NONE, nullptr, lora_sel, ds.st); // on x, behind the residual add
}

// Behind a row-parallel projection: x <- sum over ranks.  The fused seam also adds the residual and leaves
// RMSNorm(x) * gamma (-> int8) in ar_norm for the GEMV that follows.
int tllm_session::stage_seam(const DecodeStep& ds, const void* gamma, const float* quant_scale, int quant)
{
    hipStream_t st = ds.st;
    if (!ds.fused_ar)
        return allreduce(x, (int64_t) B * hidden, st);
    comm::p2p::FusedTail t;
    t.x = x;
    t.gamma = gamma;
    t.eps = eps;
    t.norm_out = ar_norm;
    t.quant = quant;
    t.quant_scale = quant_scale;
    t.dyn_scale_out = ar_scale;
    return timed(PC_COMM, st, [&] { return comm::p2p::all_reduce_residual_norm(ar_partial, B, hidden, t, st) ? 1 : 0; });
}

// K5 + K6 in one launch (kernels/mlp_fused.hip)
int tllm_session::stage_mlp_one(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    hipStream_t st = ds.st;
    FusedMlpParams f;
    f.K = hidden;
    f.I = Ir;
    f.N = L.proj.N;
    f.x = x;
    f.x_out = x;
    f.gamma = L.ln2;
    f.eps = eps;
    f.act_quant = L.ln2_scale;
    f.w_fc = L.fc.w;
    f.w_gate = L.gate.w;
    f.ldw = L.fc.ldw;
    f.scale_fc = L.fc.scale_col;
    f.scale_gate = L.gate.scale_col;
    f.per_channel = L.fc.per_channel;
    f.row_fc = L.fc.act_scale;
    f.row_gate = L.gate.act_scale ? L.gate.act_scale : L.fc.act_scale;
    f.out_quant = L.mlp_qscale;
    f.inter = ds.taps ? q8 : nullptr; // (the compact row: only a tap reads it)
    f.w_proj = L.proj.w;
    f.ldw_proj = L.proj.ldw;
    f.scale_proj = L.proj.scale_col;
    f.per_channel_proj = L.proj.per_channel;
    f.row_proj = L.proj.act_scale;
    f.flags = mlp_flags;
    f.error = fused_err;
    if (fused_max_spins >= 0)
        f.max_spins = fused_max_spins;
    f.x_pro_out = ds.taps ? tap_ptr(2, li) : nullptr;
    f.timing = mlp_timing;
    RUN(timed(PC_GEMV_LAYER, st, [&] { return launch_mlp_fused(f, st) ? 1 : 0; }));
    if (ds.taps)
        RUN(tap_copy(ds, 3, li, q8, 1));
    return 0;
}

// K5: RMSNorm (+ quant) -> gate|up GEMV -> silu * mul (+ quant)
int tllm_session::stage_gate_up(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    const int epi = ds.q_inter ? EPI_SWIGLU_QSTATIC : EPI_SWIGLU;
    void* out = ds.q_inter ? (void*) q8 : inter_buf;
    const int out_dtype = ds.q_inter ? DT_INT8 : DT_HALF;
    if (ds.fused_ar)
    {
        // the attention seam left post_layernorm's output (quantised for SmoothQuant) in ar_norm
        if (ds.taps)
            RUN(tap_copy(ds, 2, li, ar_norm, sq ? 1 : 2));
        return gemv(L.fc, B, PRO_NONE, epi, ar_norm, hidden, nullptr, nullptr, nullptr, L.mlp_qscale, out, Ir, out_dtype, &L.gate,
            ds.st, ds.ar_rows);
    }
    if (lora_site_on(LS_GATE_UP))
    {
        // gate or up among the adapters' modules: the SwiGLU epilogue would consume the two projections before the adapter has
        // reached them, so they go to g / u as two GEMVs, the LoRA launches update both, and the SwiGLU pass follows - the
        // unfused sequence of the prefill (context_gate_up), same rounding points
        RUN(gemv(L.fc, B, ds.pro_norm, EPI_NONE, x, hidden, L.ln2, nullptr, nullptr, nullptr, g, Ir, DT_HALF, nullptr, ds.st, nullptr,
            ds.taps ? tap_ptr(2, li) : nullptr));
        RUN(gemv(L.gate, B, ds.pro_norm, EPI_NONE, x, hidden, L.ln2, nullptr, nullptr, nullptr, u, Ir, DT_HALF, nullptr, ds.st));
        RUN(lora_apply(li, LS_GATE_UP, B, x, PRO_RMSNORM, L.ln2, lora_sel, ds.st));
        return timed(PC_OTHER, ds.st, [&] { return launch_swiglu(inter_buf, g, u, (int64_t) B * Ir, ds.st) ? 1 : 0; });
    }
    return gemv(L.fc, B, ds.pro_norm, epi, x, hidden, L.ln2, L.ln2_scale, nullptr, L.mlp_qscale, out, Ir, out_dtype, &L.gate, ds.st,
        nullptr, ds.taps ? tap_ptr(2, li) : nullptr);
}

// K6: (quant) -> down GEMV -> + residual
int tllm_session::stage_down(const DecodeStep& ds, int li)
{
    const Layer& L = layers[li];
    const void* in = ds.q_inter ? (const void*) q8 : inter_buf;
    const int pro = ds.q_inter ? (int) PRO_NONE : ds.pro_q;
    void* tap = nullptr;
    if (ds.taps && pro == PRO_NONE) // the SwiGLU epilogue left the operand (s8 behind the static quantiser, fp16 otherwise)
        RUN(tap_copy(ds, 3, li, in, ds.q_inter ? 1 : 2));
    else if (ds.taps)
        tap = tap_ptr(3, li);
    if (ds.fused_ar)
        return gemv(L.proj, B, pro, EPI_NONE, in, Ir, nullptr, L.mlp_qscale, nullptr, nullptr, ar_partial, hidden, DT_HALF, nullptr,
            ds.st, nullptr, tap);
    RUN(gemv(L.proj, B, pro, ds.epi_res, in, Ir, nullptr, L.mlp_qscale, x, nullptr, x, hidden, DT_HALF, nullptr, ds.st, nullptr,
        tap));
    return lora_apply(li, LS_PROJ, B, inter_buf, PRO_NONE, nullptr, lora_sel, ds.st); // on x, behind the residual add
}

int tllm_session::run_decode_step(hipStream_t st)
{
    const DecodeStep ds = plan_decode_step(st);
    if (ds.whole && (beam > 1 || hidden % 8 != 0)) // greedy: the sampler gathered the row already
        RUN(timed(PC_OTHER, st, [&] { return launch_embedding(x, cur_ids, emb, B, hidden, vocab, st); }));
    for (int li = 0; li < num_layers; ++li)
    {
        const Layer& L = layers[li];
        if (ds.taps)
            RUN(tap_copy(ds, 4, li, x, 2));
        if (ds.front)
            RUN(stage_front(ds, li));
        if (ds.qkv)
            RUN(stage_qkv(ds, li));
        if (ds.attn)
            RUN(stage_attention(ds, li));
        if (ds.o_proj)
            RUN(stage_o_proj(ds, li));
        if (ds.whole) // x <- x + sum_r O_r(ctx_r);  ar_norm <- post_layernorm(x) [-> int8]
            RUN(stage_seam(ds, L.ln2, L.ln2_scale, ds.ar_quant));
        if (ds.mlp_one)
            RUN(stage_mlp_one(ds, li));
        if (ds.gate_up)
            RUN(stage_gate_up(ds, li));
        if (ds.down)
            RUN(stage_down(ds, li));
        if (ds.whole)
        {
            // x <- x + sum_r proj_r(...);  ar_norm <- the NEXT layer's input_layernorm(x) [-> int8], or ln_f(x) for the head
            const bool last = li + 1 == num_layers;
            RUN(stage_seam(ds, last ? lnf : layers[li + 1].ln1, last ? nullptr : layers[li + 1].ln1_scale, last ? 0 : ds.ar_quant));
        }
    }
    if (!ds.whole)
        return 0;
    RUN(run_head(ds.fused_ar ? ar_norm : x, B, st, ds.fused_ar));
    RUN(run_sampler(1, st));
    return 0;
}
