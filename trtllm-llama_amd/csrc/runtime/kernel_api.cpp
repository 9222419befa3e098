// The entry points of include/tllm_runtime_api.h that need no session: single GEMV / GEMM / row-wise launches, the prefill GEMM tactic
// table, the kernels' tuning hooks and the stand-alone sampler (tests, microbenchmarks, the Python builder's profile).
#include "../../../include/tllm_runtime_api.h"
#include "../kernels/kernels.h"
#include "../plugins/plugin_base.h"
#include "sampling_config.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

namespace tllm
{
namespace kernels
{
extern int gemv_tune_blocks_per_cu;
extern int gemv_mfma_min_rows;
extern int gemm_tune_cfg;
extern int gemm_woq_tune_cfg;
extern bool gemm_swiglu_one_tile; // gemm_sqp.hip: A/B hook
extern void* gemm_clock_probe;
int launch_gemm_cfg(const GemmParams& p, int cfg, hipStream_t stream);     // gemm_glds.hip: exactly this kernel id, 1 = not served
int gemm_static_cfg(const GemmParams& p);                                    // gemm_glds.hip
int launch_gemm_woq_cfg(const GemmParams& p, int cfg, hipStream_t stream); // gemm_woq.hip: exactly this tile shape, 1 = not served
int launch_gemm_mfma(const GemmParams& p, hipStream_t stream);             // gemm_mfma.hip
}
} // namespace tllm

static GemmParams gemm_params(const tllm_gemm_params_t* q)
{
    GemmParams g;
    g.wtype = q->wtype;
    g.out_dtype = q->out_dtype;
    g.M = q->M;
    g.N = q->N;
    g.K = q->K;
    g.a = q->a;
    g.lda = q->lda;
    g.w = q->w;
    g.ldw = q->ldw;
    g.scale_col = q->scale_col;
    g.scale_row = q->scale_row;
    g.per_channel = q->per_channel;
    g.per_token = q->per_token;
    g.c = q->c;
    g.ldc = q->ldc;
    return g;
}

// tllm_attention_params_t -> the decode launcher's struct and the split-KV plan of the launch (mmha_plan: the GPTAttention plugin's
// where the caller left rows_per_group open)
static int attention_decode_params(const tllm_attention_params_t* q, MmhaParams& p, MmhaPlan& plan)
{
    static_assert((int) TLLM_HALF == DT_HALF && (int) TLLM_INT8 == DT_INT8 && (int) TLLM_FP8 == DT_FP8, "kv_cache_type is a DType");
    if (!q || q->batch < 1 || q->num_heads < 1 || q->head_size < 1 || q->max_seq_len < 1)
    {
        set_error("tllm_attention_decode: bad arguments (batch, num_heads, head_size, max_seq_len)");
        return 1;
    }
    p.num_heads = q->num_heads;
    p.num_kv_heads = q->num_kv_heads;
    p.q_heads_per_workgroup = q->q_heads_per_workgroup;
    if (mmha_resolve_grouping(p)) // the launcher's own check: one statement of the rule
        return 1;
    if (q->rows_per_group != 0 && q->rows_per_group != 4 && q->rows_per_group != 12 && q->rows_per_group != 16)
    {
        set_error("tllm_attention_decode: rows_per_group %d is not 4, 12 or 16", q->rows_per_group);
        return 1;
    }
    if (q->kv_cache_type != 0 && q->kv_cache_type != TLLM_HALF && q->kv_cache_type != TLLM_INT8 && q->kv_cache_type != TLLM_FP8)
    {
        set_error("tllm_attention_decode: kv_cache_type %d is not TLLM_HALF, TLLM_INT8 or TLLM_FP8", q->kv_cache_type);
        return 1;
    }
    plan = mmha_plan(q->head_size, q->max_seq_len, q->batch, q->num_heads, q->rows_per_group, q->combine_launch != 0);
    if (plan.rows_per_group == 0)
    {
        set_error("tllm_attention_decode: head_size %d not supported", q->head_size);
        return 1;
    }
    p.batch = q->batch;
    p.head_size = q->head_size;
    p.rotary_dim = q->rotary_dim;
    p.neox = q->neox;
    p.inv_sqrt_dh = 1.f / (sqrtf((float) q->head_size) * (q->q_scaling != 0.f ? q->q_scaling : 1.f));
    p.kv_dtype = q->kv_cache_type ? q->kv_cache_type : DT_HALF; // (TLLM_* and DT_* share their values)
    p.max_seq_len = q->max_seq_len;
    p.max_input_len = q->max_input_len;
    p.qkv = q->qkv;
    p.kv_cache = q->kv_cache;
    p.sequence_length = q->sequence_length;
    p.input_lengths = q->input_lengths;
    p.masked_tokens = q->masked_tokens;
    p.timestep_host = q->timestep;
    p.kv_scale_orig_quant = q->kv_scale_orig_quant;
    p.kv_scale_quant_orig = q->kv_scale_quant_orig;
    if (q->beam_width > 1)
    {
        p.cache_indirection = q->cache_indirection;
        p.beam_width = q->beam_width;
    }
    p.block_pointers = q->block_pointers;
    p.tokens_per_block = q->tokens_per_block;
    p.max_blocks_per_seq = q->max_blocks_per_seq;
    p.tail_quant_scale = q->tail_quant_scale;
    p.tail_out_q8 = q->tail_out_q8;
    p.out = q->out;
    return 0;
}

extern "C" {

size_t tllm_attention_workspace_size(const tllm_attention_params_t* q, int32_t is_context)
{
    if (!q)
        return 0;
    if (is_context)
        return context_attention_workspace_size(q->batch, q->num_heads, q->head_size, q->seq) + 256;
    return mmha_plan(q->head_size, q->max_seq_len, q->batch, q->num_heads).workspace_bytes + 256;
}

int32_t tllm_attention_decode_layout(const tllm_attention_params_t* q, int32_t* tchunk, int32_t* nsplit, int32_t* q_tile,
    int32_t* in_launch_merge)
{
    MmhaParams p;
    MmhaPlan plan;
    if (attention_decode_params(q, p, plan))
        return 1;
    if (tchunk)
        *tchunk = plan.tchunk;
    if (nsplit)
        *nsplit = plan.nsplit;
    if (q_tile)
        *q_tile = p.q_heads_per_workgroup;
    if (in_launch_merge)
        *in_launch_merge = plan.in_launch_merge ? 1 : 0;
    return 0;
}

int32_t tllm_attention_decode(const tllm_attention_params_t* q, tllm_stream_t stream)
{
    MmhaParams p;
    MmhaPlan plan;
    if (attention_decode_params(q, p, plan))
        return 1;
    // paged: kv_cache is the pool itself - the rows of a block the table does not map yet are still loaded (and masked), from there
    if (!q->qkv || !q->out || !q->workspace || !q->sequence_length || !q->input_lengths || !q->kv_cache)
    {
        set_error("tllm_attention_decode: qkv, out, workspace, sequence_length, input_lengths and kv_cache (paged: the pool) must be set");
        return 1;
    }
    if (q->beam_width > 1 && !q->cache_indirection)
    {
        set_error("tllm_attention_decode: beam width %d without a cache indirection", q->beam_width);
        return 1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p.rotary_dim > 0)
    {
        p.rope_table = tllm::plugins::rope_table(p.rotary_dim, p.max_seq_len, &p.rope_table_len);
        if (!p.rope_table)
            return 1;
    }
    // the merge tickets are zeroed per call, as the plugin does
    if (mmha_bind_workspace(p, plan, q->workspace, true, st))
        return 1;
    return launch_mmha(p, st) ? 1 : 0;
}

int32_t tllm_attention_context(const tllm_attention_params_t* q, tllm_stream_t stream)
{
    if (!q || q->batch < 1 || q->seq < 1 || q->num_heads < 1 || !q->qkv || !q->out || !q->input_lengths
        || (!q->kv_cache && !q->block_pointers))
    {
        set_error("tllm_attention_context: bad arguments (batch, seq, num_heads, qkv, out, input_lengths and the cache must be set)");
        return 1;
    }
    if (q->kv_cache_type != 0 && q->kv_cache_type != TLLM_HALF && q->kv_cache_type != TLLM_INT8 && q->kv_cache_type != TLLM_FP8)
    {
        set_error("tllm_attention_context: kv_cache_type %d is not TLLM_HALF, TLLM_INT8 or TLLM_FP8", q->kv_cache_type);
        return 1;
    }
    ContextAttnParams p;
    p.batch = q->batch;
    p.seq = q->seq;
    p.num_heads = q->num_heads;
    p.num_kv_heads = q->num_kv_heads;
    p.head_size = q->head_size;
    p.rotary_dim = q->rotary_dim;
    p.neox = q->neox;
    p.inv_sqrt_dh = 1.f / (sqrtf((float) q->head_size) * (q->q_scaling != 0.f ? q->q_scaling : 1.f));
    p.kv_dtype = q->kv_cache_type ? q->kv_cache_type : DT_HALF; // (TLLM_* and DT_* share their values)
    p.max_seq_len = q->max_seq_len;
    p.qkv = q->qkv;
    p.kv_cache = q->kv_cache;
    p.input_lengths = q->input_lengths;
    p.kv_scale_orig_quant = q->kv_scale_orig_quant;
    if (p.rotary_dim > 0)
    {
        p.rope_table = tllm::plugins::rope_table(p.rotary_dim, p.max_seq_len, &p.rope_table_len);
        if (!p.rope_table)
            return 1;
    }
    p.out = q->out;
    p.out_q8 = q->out_q8;
    p.out_q_scale = q->out_q_scale;
    p.workspace = q->workspace;
    p.cu_seqlens = q->cu_seqlens;
    p.cache_seq_stride = q->cache_seq_stride > 0 ? q->cache_seq_stride : 1;
    p.block_pointers = q->block_pointers;
    p.tokens_per_block = q->tokens_per_block;
    p.max_blocks_per_seq = q->max_blocks_per_seq;
    p.kernel = q->context_kernel;
    return launch_context_attention(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_attention_context_layout(const tllm_attention_params_t* q, int32_t cus, int32_t* kind, int32_t* query_block,
    int32_t* stages, int32_t* workgroups)
{
    static_assert(TLLM_CTX_ATTN_WAVE == CTX_ATTN_WAVE && TLLM_CTX_ATTN_MFMA_NARROW == CTX_ATTN_MFMA_NARROW
            && TLLM_CTX_ATTN_MFMA_WIDE == CTX_ATTN_MFMA_WIDE && TLLM_CTX_ATTN_MFMA_PAIRED == CTX_ATTN_MFMA_PAIRED,
        "the header's kinds are the launcher's");
    if (!q || cus < 0)
    {
        set_error("tllm_attention_context_layout: bad arguments");
        return 1;
    }
    // the score scale as tllm_attention_context computes it: the launcher's own plan, one statement of the rule
    const float inv_sqrt_dh = 1.f / (sqrtf((float) q->head_size) * (q->q_scaling != 0.f ? q->q_scaling : 1.f));
    const ContextAttnPlan plan = context_attention_plan(q->head_size, q->seq, q->batch, q->num_heads, q->workspace != nullptr,
        inv_sqrt_dh > 0.f, cus, q->context_kernel);
    if (plan.kernel == 0)
    {
        set_error("tllm_attention_context_layout: kernel %d refused: %s", q->context_kernel, plan.refused ? plan.refused : "no plan");
        return 1;
    }
    if (kind)
        *kind = plan.kernel;
    if (query_block)
        *query_block = plan.query_block;
    if (stages)
        *stages = plan.stages;
    if (workgroups)
        *workgroups = (int32_t) (plan.grid[0] * plan.grid[1] * plan.grid[2]);
    return 0;
}

int32_t tllm_attention_append_layout(const tllm_attention_append_params_t* q, int32_t* kind)
{
    static_assert(TLLM_APPEND_ATTN_WAVE == APPEND_ATTN_WAVE && TLLM_APPEND_ATTN_MFMA == APPEND_ATTN_MFMA, "the header's kinds are the launcher's");
    if (!q)
    {
        set_error("tllm_attention_append_layout: bad arguments");
        return 1;
    }
    const char* why = nullptr;
    const int k = append_attention_kernel(q->head_size, q->n, q->append_kernel, &why);
    if (k == 0)
    {
        set_error("tllm_attention_append_layout: kernel %d refused: %s", q->append_kernel, why ? why : "no plan");
        return 1;
    }
    if (kind)
        *kind = k;
    return 0;
}

// n_per_seq null: tllm_attention_append (q->max_past holds); else tllm_attention_append_ragged (max_end in its place).
// block_pointers set: tllm_attention_append_paged (q->kv_cache is the pool)
static int32_t attention_append(const char* who, const tllm_attention_append_params_t* q, const int32_t* n_per_seq, int32_t max_end,
    tllm_stream_t stream, const int64_t* block_pointers = nullptr, int32_t tokens_per_block = 0, int32_t max_blocks_per_seq = 0)
{
    if (!q || q->batch < 1 || q->n < 1 || q->num_heads < 1 || q->head_size < 1 || q->max_seq_len < 1)
    {
        set_error("%s: bad arguments (batch, n, num_heads, head_size, max_seq_len)", who);
        return 1;
    }
    if (q->kv_cache_type != 0 && q->kv_cache_type != TLLM_HALF && q->kv_cache_type != TLLM_INT8 && q->kv_cache_type != TLLM_FP8)
    {
        set_error("%s: kv_cache_type %d is not TLLM_HALF, TLLM_INT8 or TLLM_FP8", who, q->kv_cache_type);
        return 1;
    }
    AppendAttnParams p;
    p.batch = q->batch;
    p.n = q->n;
    p.n_per_seq = n_per_seq;
    p.max_end = max_end;
    p.num_heads = q->num_heads;
    p.num_kv_heads = q->num_kv_heads;
    p.head_size = q->head_size;
    p.rotary_dim = q->rotary_dim;
    p.neox = q->neox;
    p.inv_sqrt_dh = 1.f / (sqrtf((float) q->head_size) * (q->q_scaling != 0.f ? q->q_scaling : 1.f));
    p.kv_dtype = q->kv_cache_type ? q->kv_cache_type : DT_HALF; // (TLLM_* and DT_* share their values)
    p.max_seq_len = q->max_seq_len;
    p.max_input_len = q->max_input_len;
    p.max_past = q->max_past;
    p.kernel = q->append_kernel;
    p.qkv = q->qkv;
    p.kv_cache = q->kv_cache;
    p.sequence_length = q->sequence_length;
    p.input_lengths = q->input_lengths;
    p.masked_tokens = q->masked_tokens;
    p.kv_scale_orig_quant = q->kv_scale_orig_quant;
    p.kv_scale_quant_orig = q->kv_scale_quant_orig;
    p.out = q->out;
    p.block_pointers = block_pointers;
    p.tokens_per_block = tokens_per_block;
    p.max_blocks_per_seq = max_blocks_per_seq;
    if (p.rotary_dim > 0)
    {
        p.rope_table = tllm::plugins::rope_table(p.rotary_dim, p.max_seq_len, &p.rope_table_len);
        if (!p.rope_table)
            return 1;
    }
    return launch_append_attention(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_attention_append(const tllm_attention_append_params_t* q, tllm_stream_t stream)
{
    return attention_append("tllm_attention_append", q, nullptr, 0, stream);
}

int32_t tllm_attention_append_ragged(const tllm_attention_append_params_t* q, const int32_t* n_per_seq, int32_t max_end,
    tllm_stream_t stream)
{
    if (!n_per_seq)
    {
        set_error("tllm_attention_append_ragged: n_per_seq is null");
        return 1;
    }
    return attention_append("tllm_attention_append_ragged", q, n_per_seq, max_end, stream);
}

int32_t tllm_attention_append_paged(const tllm_attention_append_params_t* q, const int64_t* block_pointers, int32_t tokens_per_block,
    int32_t max_blocks_per_seq, const int32_t* n_per_seq, int32_t max_end, tllm_stream_t stream)
{
    if (!block_pointers)
    {
        set_error("tllm_attention_append_paged: block_pointers is null");
        return 1;
    }
    return attention_append("tllm_attention_append_paged", q, n_per_seq, max_end, stream, block_pointers, tokens_per_block,
        max_blocks_per_seq);
}

static GemvParams gemv_params(const tllm_gemv_params_t* q)
{
    GemvParams p;
    p.wtype = q->wtype;
    p.pro = q->pro;
    p.epi = q->epi;
    p.out_dtype = q->out_dtype;
    p.M = q->M;
    p.N = q->N;
    p.K = q->K;
    p.x = q->x;
    p.ldx = q->ldx;
    p.w = q->w;
    p.ldw = q->ldw;
    p.scale_col = q->scale_col;
    p.scale_row = q->scale_row;
    p.per_channel = q->per_channel;
    p.per_token = q->per_token;
    p.gamma = q->gamma;
    p.eps = q->eps;
    p.act_scale = q->act_scale;
    p.dyn_scale_out = q->dyn_scale_out;
    p.x_pro_out = q->x_pro_out;
    p.residual = q->residual;
    p.epi_scale = q->epi_scale;
    p.y = q->y;
    p.ldy = q->ldy;
    return p;
}

int32_t tllm_gemv(const tllm_gemv_params_t* q, tllm_stream_t stream)
{
    if (!q)
        return 1;
    return launch_gemv(gemv_params(q), reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gemv_head(const tllm_gemv_params_t* q, int32_t resident_rows, void* argmax_part, tllm_stream_t stream)
{
    static_assert(TLLM_ARGMAX_PAIRS == kArgmaxPairs, "the header's constant is the kernels'");
    if (!q || resident_rows < 0)
    {
        set_error("tllm_gemv_head: bad arguments");
        return 1;
    }
    GemvParams p = gemv_params(q);
    p.resident_rows = resident_rows;
    p.argmax_part = argmax_part;
    return launch_gemv(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_lora_shrink(const tllm_lora_shrink_params_t* q, tllm_stream_t stream)
{
    static_assert(TLLM_LORA_MAX_ADAPTERS == kLoraMaxAdapters && TLLM_LORA_MAX_SEGMENTS == kLoraMaxSegments,
        "the header's constants are the kernels'");
    if (!q)
        return 1;
    LoraShrinkParams p;
    p.M = q->M;
    p.K = q->K;
    p.R = q->R;
    p.pro = q->pro;
    p.x = q->x;
    p.ldx = q->ldx;
    p.gamma = q->gamma;
    p.eps = q->eps;
    p.row_adapter = q->row_adapter;
    p.table = static_cast<const LoraAdapterRec*>(q->table);
    p.num_adapters = q->num_adapters;
    p.t = q->t;
    return launch_lora_shrink(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_lora_expand(const tllm_lora_expand_params_t* q, tllm_stream_t stream)
{
    if (!q)
        return 1;
    LoraExpandParams p;
    p.M = q->M;
    p.r = q->r;
    p.nseg = q->nseg;
    for (int g = 0; g < kLoraMaxSegments; ++g)
    {
        p.seg_n[g] = q->seg_n[g];
        p.seg_y[g] = q->seg_y[g];
        p.seg_ldy[g] = q->seg_ldy[g];
    }
    p.t = q->t;
    p.row_adapter = q->row_adapter;
    p.table = static_cast<const LoraAdapterRec*>(q->table);
    p.num_adapters = q->num_adapters;
    return launch_lora_expand(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

static bool greedy_args_ok(const tllm_greedy_params_t* q)
{
    return q && q->logits && q->cur_ids && q->out_ids && q->seq_len && q->batch >= 1 && q->nparts >= 1 && q->vocab_part >= 1
        && q->vocab >= 1 && (int64_t) q->nparts * q->vocab_part >= q->vocab
        && !(q->rope_row_out && (q->rope_half < 1 || q->rope_half > 960 || q->rope_table_len < 1)); // (the launchers check the rest)
}

static GreedyParams greedy_params(const tllm_greedy_params_t* q)
{
    GreedyParams g;
    g.logits = q->logits;
    g.batch = q->batch;
    g.vocab_part = q->vocab_part;
    g.nparts = q->nparts;
    g.vocab = q->vocab;
    g.cur_ids = q->cur_ids;
    g.out_ids = q->out_ids;
    g.out_stride = q->out_stride;
    g.seq_len = q->seq_len;
    g.finished = q->finished;
    g.end_id = q->end_id;
    g.advance = q->advance;
    g.rope_row_out = q->rope_row_out;
    g.rope_pos_out = q->rope_pos_out;
    g.rope_table = q->rope_table;
    g.rope_half = q->rope_half;
    g.rope_table_len = q->rope_table_len;
    g.input_lengths = q->input_lengths;
    g.max_input_len = q->max_input_len;
    g.emb_table = q->emb_table;
    g.x_out = q->x_out;
    g.hidden = q->hidden;
    g.step_epoch = q->step_epoch;
    g.argmax_part = q->argmax_part;
    return g;
}

int32_t tllm_greedy_step(const tllm_greedy_params_t* q, tllm_stream_t stream)
{
    if (!greedy_args_ok(q))
    {
        set_error("tllm_greedy_step: bad arguments");
        return 1;
    }
    return launch_greedy_step(greedy_params(q), reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_spec_accept(const tllm_spec_accept_params_t* q, tllm_stream_t stream)
{
    static_assert(TLLM_VERIFY_MAX_TOKENS == kVerifyMaxTokens, "the header's constant is the kernels'");
    if (!q || !greedy_args_ok(&q->g) || q->g.nparts != 1 || q->g.out_stride < 1)
    {
        set_error("tllm_spec_accept: bad arguments (the greedy step's, with one vocabulary part)");
        return 1;
    }
    SpecAcceptParams p;
    p.g = greedy_params(&q->g);
    p.g.argmax_part = nullptr;
    p.n = q->n;
    p.ids = q->ids;
    p.top1 = q->top1;
    p.limit = q->limit;
    p.accepted = q->accepted;
    p.logits_out = q->logits_out;
    return launch_spec_accept(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_prompt_lookup(const int32_t* out_ids, int32_t batch, int32_t out_stride, const int32_t* seq_len,
    const int32_t* input_lengths, int32_t max_input_len, const int32_t* finished, const int32_t* limit, int32_t vocab, int32_t n,
    int32_t max_ngram, int32_t* ids, int32_t* draft_len, tllm_stream_t stream)
{
    if (batch < 1)
    {
        set_error("tllm_prompt_lookup: bad arguments");
        return 1;
    }
    PromptLookupParams p;
    p.batch = batch;
    p.n = n;
    p.max_ngram = max_ngram;
    p.out_ids = out_ids;
    p.out_stride = out_stride;
    p.seq_len = seq_len;
    p.input_lengths = input_lengths;
    p.max_input_len = max_input_len;
    p.finished = finished;
    p.limit = limit;
    p.vocab = vocab;
    p.ids = ids;
    p.draft_len = draft_len;
    return launch_prompt_lookup(p, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gemm(const tllm_gemm_params_t* q, tllm_stream_t stream)
{
    if (!q)
        return 1;
    return launch_gemm(gemm_params(q), reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gemm_residual(const tllm_gemm_params_t* q, const void* residual, tllm_stream_t stream)
{
    if (!q || !residual || q->out_dtype != DT_HALF)
    {
        set_error("tllm_gemm_residual: needs a residual and fp16 output");
        return 1;
    }
    GemmParams g = gemm_params(q);
    g.residual = residual;
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gemm_epi(const tllm_gemm_params_t* q, const void* residual, const void* silu_gate, tllm_stream_t stream)
{
    if (!q)
        return 1;
    GemmParams g = gemm_params(q);
    g.residual = residual;
    g.silu_gate = silu_gate;
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gemm_kernel(const tllm_gemm_params_t* q, const void* residual, const void* silu_gate, int32_t kernel_id,
    tllm_stream_t stream)
{
    if (!q)
    {
        set_error("tllm_gemm_kernel: null argument");
        return 1;
    }
    GemmParams g = gemm_params(q);
    g.residual = residual;
    g.silu_gate = silu_gate;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = 1;
    const char* why = "this kernel does not take the problem (weight type, alignment, K, M, output type or epilogue)";
    if (g.M <= 0 || g.N <= 0 || g.K <= 0)
        why = "empty problem";
    else if (residual && silu_gate)
        why = "the residual and the SwiGLU gate exclude each other";
    else if ((kernel_id >= 21 && kernel_id <= 27) || (kernel_id >= 31 && kernel_id <= 33))
        why = "an ablation of the phased pipeline (wrong results on purpose): microbench only";
    else if (kernel_id >= 1 && kernel_id <= 65)
        rc = launch_gemm_cfg(g, kernel_id, s);
    else if (kernel_id >= 101 && kernel_id <= 106)
        rc = launch_gemm_woq_cfg(g, kernel_id - 100, s);
    else if (kernel_id == TLLM_GEMM_KERNEL_REGISTER_STAGED)
    {
        if (residual || silu_gate)
            why = "the register-staged kernel fuses neither the residual nor the SwiGLU gate";
        else if ((g.wtype == W_INT8_WOQ || g.wtype == W_INT4_WOQ) && !g.scale_col)
            why = "weight-only weights need their scales";
        else
            rc = launch_gemm_mfma(g, s);
    }
    else
        why = "no such kernel id";
    if (rc > 0)
        set_error("tllm_gemm_kernel: kernel id %d refuses %d x %d x %d (wtype %d): %s", kernel_id, g.M, g.N, g.K, g.wtype, why);
    return rc;
}

int32_t tllm_gemm_static_cfg(const tllm_gemm_params_t* q)
{
    return q ? gemm_static_cfg(gemm_params(q)) : 0;
}

int32_t tllm_gemm_profile(int32_t wtype, int32_t M, int32_t N, int32_t K, int32_t* best_cfg, float* best_us, tllm_stream_t stream)
{
    int cfg = 0;
    float us = 0.f;
    if (gemm_profile(wtype, M, N, K, &cfg, &us, reinterpret_cast<hipStream_t>(stream)))
        return 1;
    if (best_cfg)
        *best_cfg = cfg;
    if (best_us)
        *best_us = us;
    return 0;
}

int64_t tllm_gemm_tactics_export(char* buf, int64_t capacity)
{
    const std::string t = gemm_tactics_export();
    if (buf && capacity > 0)
    {
        const size_t n = std::min((size_t) capacity - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int64_t) t.size() + 1;
}

int32_t tllm_gemm_tactics_import(const char* text)
{
    return gemm_tactics_import(text) < 0 ? 1 : 0;
}

void tllm_gemm_tactics_clear(void)
{
    gemm_tactics_clear();
}

int32_t tllm_gemm_tactic_lookup(int32_t wtype, int32_t M, int32_t N, int32_t K)
{
    return gemm_tactic_lookup(wtype, M, N, K);
}

void tllm_gemv_set_blocks_per_cu(int32_t n)
{
    tllm::kernels::gemv_tune_blocks_per_cu = n;
}

void tllm_gemv_set_mfma_rows(int32_t n)
{
    tllm::kernels::gemv_mfma_min_rows = n;
}

int32_t tllm_gemm_swiglu_quant(const tllm_gemm_params_t* q, const void* w_up, const void* scale_col_up, const float* quant_scale,
    tllm_stream_t stream)
{
    if (!q || !w_up || !scale_col_up || !quant_scale)
    {
        set_error("tllm_gemm_swiglu_quant: null argument");
        return 1;
    }
    GemmParams g = gemm_params(q);
    g.out_dtype = DT_INT8;
    g.w2 = w_up;
    g.scale_col2 = scale_col_up;
    g.swiglu_qscale = quant_scale;
    const int rc = tllm::kernels::launch_gemm_swiglu(g, reinterpret_cast<hipStream_t>(stream));
    if (rc == 1)
        set_error("tllm_gemm_swiglu_quant: problem not served by the fused kernel (SmoothQuant static, K %% 128 == 0, M >= 32, 16-byte aligned operands)");
    return rc ? 1 : 0;
}

void tllm_gemm_set_clock_probe(void* device_buffer)
{
    tllm::kernels::gemm_clock_probe = device_buffer;
}

void tllm_gemm_set_tile_cfg(int32_t cfg)
{
    // 0 resets both tables; 101.. select the tile shape of the weight-only main-loop-dequantising GEMM (gemm_woq.hip: 101 = 256 x 192,
    // 102 = 128 x 128, 103 = 256 x 192 two stages ahead, 104 = 256 x 192 on 4 waves)
    // -2: the fused SwiGLU SmoothQuant GEMM in its one-tile-per-workgroup form (A/B against the persistent one; 0 resets)
    if (cfg == 0 || cfg == -2)
        tllm::kernels::gemm_swiglu_one_tile = cfg == -2;
    if (cfg == -2)
        return;
    if (cfg == 0 || cfg > 100)
        tllm::kernels::gemm_woq_tune_cfg = cfg > 100 ? cfg - 100 : 0;
    if (cfg > 100)
        return;
    tllm::kernels::gemm_tune_cfg = cfg;
}


int32_t tllm_sample_tokens(const float* logits, int32_t nparts, int32_t rows, int32_t vocab_part, int32_t vocab,
    const tllm_sampling_config_t* cfg, int32_t end_id, const int32_t* history, int32_t history_stride, const int32_t* input_lengths,
    int32_t max_input_len, const int32_t* g, int32_t* out_ids, float* u_out, tllm_stream_t stream)
{
    if (!logits || !cfg || !g || !out_ids || rows < 1 || max_input_len < 0)
    {
        set_error("tllm_sample_tokens: bad arguments");
        return 1;
    }
    if (const int rc = check_sampling_config("tllm_sample_tokens", *cfg))
        return rc;
    SamplingParams sp;
    sampling_from_config(sp, *cfg);
    sp.g.logits = logits;
    sp.g.batch = rows;
    sp.g.vocab_part = vocab_part;
    sp.g.nparts = nparts;
    sp.g.vocab = vocab;
    sp.g.cur_ids = out_ids;
    sp.g.seq_len = const_cast<int32_t*>(g); // advance = 0: read only; with g_base = 1 the token number is g[r] itself
    sp.g.end_id = end_id;
    sp.g.input_lengths = input_lengths;
    sp.g.max_input_len = max_input_len;
    sp.g_base = 1;
    sp.history = history;
    sp.history_stride = history_stride;
    sp.u_out = u_out;
    return launch_sampling_step(sp, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_spec_sample_rows(const float* logits, int32_t nparts, int32_t batch, int32_t n, int32_t vocab_part, int32_t vocab,
    const tllm_sampling_config_t* cfg, int32_t end_id, const int32_t* ids, const int32_t* out_ids, int32_t out_stride,
    const int32_t* seq_len, const int32_t* input_lengths, int32_t max_input_len, const int32_t* finished, const int32_t* limit,
    int32_t* draws, float* u_out, tllm_stream_t stream)
{
    if (!logits || !cfg || !ids || !seq_len || !draws || batch < 1 || max_input_len < 0 || (out_ids && out_stride < 1))
    {
        set_error("tllm_spec_sample_rows: bad arguments");
        return 1;
    }
    if (const int rc = check_sampling_config("tllm_spec_sample_rows", *cfg))
        return rc;
    SpecSampleParams sp;
    sampling_from_config(sp.s, *cfg);
    sp.s.g.logits = logits;
    sp.s.g.batch = batch;
    sp.s.g.vocab_part = vocab_part;
    sp.s.g.nparts = nparts;
    sp.s.g.vocab = vocab;
    sp.s.g.seq_len = const_cast<int32_t*>(seq_len); // read only
    sp.s.g.finished = const_cast<int32_t*>(finished);
    sp.s.g.end_id = end_id;
    sp.s.g.input_lengths = input_lengths;
    sp.s.g.max_input_len = max_input_len;
    sp.s.g_base = max_input_len;
    sp.s.history = out_ids;
    sp.s.history_stride = out_ids ? out_stride : 0;
    sp.s.u_out = u_out;
    sp.n = n;
    sp.ids = ids;
    sp.limit = limit;
    sp.draws = draws;
    return launch_spec_sample_rows(sp, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_token_logprobs(const float* logits, int32_t nparts, int32_t rows, int32_t vocab_part, int32_t vocab,
    const int32_t* targets, float* partials, float* log_probs, float* lse, int32_t* top1_ids, tllm_stream_t stream)
{
    if (!logits || !targets || !partials || !log_probs || nparts < 1 || rows < 1 || vocab_part < 1 || vocab < 1
        || (int64_t) nparts * vocab_part < vocab)
    {
        set_error("tllm_token_logprobs: bad arguments (the parts must cover the vocabulary)");
        return 1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TokenLogprobParams p;
    p.logits = logits;
    p.part_stride = (int64_t) rows * vocab_part;
    p.ld = vocab_part;
    p.rows = rows;
    p.nparts = nparts;
    p.vocab_part = vocab_part;
    p.vocab = vocab;
    p.targets = targets;
    p.partials = partials;
    if (launch_token_logprob_partial(p, st))
        return 1;
    return launch_token_logprob_merge(partials, nparts, rows, vocab, targets, log_probs, lse, top1_ids, st) ? 1 : 0;
}

static RmsnormParams rmsnorm_params(const tllm_rmsnorm_params_t* q)
{
    RmsnormParams p;
    p.M = q->M;
    p.N = q->N;
    p.x = q->x;
    p.residual = q->residual;
    p.sum_out = q->sum_out;
    p.gamma = q->gamma;
    p.eps = q->eps;
    p.y = q->y;
    p.q = q->q;
    p.static_scale = q->static_scale;
    p.dyn_scale_out = q->dyn_scale_out;
    p.layernorm = q->layernorm;
    p.use_diff_of_squares = q->use_diff_of_squares;
    p.beta = q->beta;
    return p;
}

int32_t tllm_rmsnorm(const tllm_rmsnorm_params_t* q, int32_t kernel, tllm_stream_t stream)
{
    if (!q || !q->x || !q->gamma || (!q->y && !q->q))
    {
        set_error("tllm_rmsnorm: bad arguments (x, gamma and one of y, q must be set)");
        return -1;
    }
    return launch_rmsnorm_kernel(rmsnorm_params(q), kernel, reinterpret_cast<hipStream_t>(stream)) ? -1 : 0;
}

int32_t tllm_rmsnorm_kernel(const tllm_rmsnorm_params_t* q)
{
    if (!q)
    {
        set_error("tllm_rmsnorm_kernel: null argument");
        return -1;
    }
    return rmsnorm_kernel_for(rmsnorm_params(q));
}

int32_t tllm_swiglu(void* y, const void* a, const void* b, int64_t n, tllm_stream_t stream)
{
    return launch_swiglu(y, a, b, n, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_swiglu_quant(int8_t* q, const void* a, const void* b, int64_t n, const float* scale, tllm_stream_t stream)
{
    return launch_swiglu_quant(q, a, b, n, scale, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_add(void* y, const void* a, const void* b, int64_t n, tllm_stream_t stream)
{
    return launch_add(y, a, b, n, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_quantize_tensor(int8_t* dst, const void* src, int32_t src_dtype, int64_t size, const float* scale, tllm_stream_t stream)
{
    return launch_quantize_tensor(dst, src, src_dtype, size, scale, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_quantize_per_token(int8_t* dst, const void* src, int32_t src_dtype, int64_t rows, int64_t cols, float* scale_out,
    tllm_stream_t stream)
{
    return launch_quantize_per_token(dst, src, src_dtype, rows, cols, scale_out, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_embedding(void* out, const int32_t* ids, const void* table, int64_t tokens, int32_t hidden, int32_t vocab,
    tllm_stream_t stream)
{
    return launch_embedding(out, ids, table, tokens, hidden, vocab, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gather_last_token(void* out, const void* hidden, const int32_t* last_token_ids, int32_t batch, int32_t seq,
    int32_t hidden_size, tllm_stream_t stream)
{
    return launch_gather_last_token(out, hidden, last_token_ids, batch, seq, hidden_size, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_gather_rows(void* out, const void* hidden, const int32_t* rows, int32_t batch, int32_t hidden_size, tllm_stream_t stream)
{
    return launch_gather_rows(out, hidden, rows, batch, hidden_size, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_exclusive_scan_i32(int32_t* cu, const int32_t* lens, int32_t n, tllm_stream_t stream)
{
    return launch_exclusive_scan_i32(cu, lens, n, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_fill_i32(int32_t* dst, int32_t value, int64_t n, tllm_stream_t stream)
{
    return launch_fill_i32(dst, value, n, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

int32_t tllm_fill_random(void* dst, int32_t dtype, int64_t n, uint32_t seed, float scale, tllm_stream_t stream)
{
    return launch_fill_random(dst, dtype, n, seed, scale, reinterpret_cast<hipStream_t>(stream)) ? 1 : 0;
}

} // extern "C"
