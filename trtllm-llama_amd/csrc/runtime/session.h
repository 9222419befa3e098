// The decode session behind include/tllm_runtime_api.h: its state and the declarations of what runs on it.  Internal to
// csrc/runtime (not installed).  The definitions live by concern:
//   session_weights.cpp  configuration text -> fields, named tensors -> Linear / Layer, the engine-file parser
//   session_setup.cpp    buffer allocation, the decision which decode form runs, check_comm (which withdraws that decision)
//   session_context.cpp  the prefill schedule
//   session_decode.cpp   the generation-step schedule, head, sampler, all-reduce
//   session_lora.cpp     LoRA adapters per sequence: their buffers, load / commit / clear / select, the two launches behind a projection
//   session.cpp          the rest of the C API: prompt upload, graph capture, the generate loop, getters, instrumentation
#pragma once
#include "../../../include/tllm_runtime_api.h"
#include "../kernels/kernels.h"
#include "../kernels/weight_layout.h"
#include "../plugins/comm.h"
#include "../plugins/plugin_base.h"
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace tllm
{
namespace runtime
{

enum QuantBits
{
    QM_INT4_WEIGHTS = 1,
    QM_INT8_WEIGHTS = 2,
    QM_ACTIVATIONS = 4,
    QM_PER_CHANNEL = 8,
    QM_PER_TOKEN = 16,
    QM_INT8_KV = 32,
    QM_FP8_KV = 64
};

struct TensorRec
{
    int32_t dtype = 0;
    std::vector<int64_t> dims;
    void* dev = nullptr;
    bool owned = false;
    size_t bytes = 0;
    int64_t numel() const
    {
        int64_t n = 1;
        for (auto d : dims)
            n *= d;
        return n;
    }
};

struct Linear
{
    int wtype = kernels::W_FP16;
    const void* w = nullptr;
    int64_t ldw = 0;
    int N = 0, K = 0;
    const void* scale_col = nullptr; // fp16 [N] (weight-only) | f32 [N] or [1] (SmoothQuant)
    int per_channel = 0;
    const float* act_scale = nullptr; // SmoothQuant static: dequant scale of the GEMM [1,1]
};

struct Layer
{
    const void* ln1 = nullptr;
    const void* ln2 = nullptr;
    const float* ln1_scale = nullptr;  // input_layernorm.scale_to_int (SQ static)
    const float* ln2_scale = nullptr;  // post_layernorm.scale_to_int
    const float* attn_qscale = nullptr; // attention.quantization_scaling_factor (ctx -> int8, SQ static)
    const float* mlp_qscale = nullptr;  // mlp.quantization_scaling_factor (silu*mul -> int8, SQ static)
    const float* kv_oq = nullptr;
    const float* kv_qo = nullptr;
    Linear qkv, dense, fc, gate, proj;
    void* kv = nullptr;                // linear cache [B, 2, Hr, Smax, Dh], or the block pool [2, blocks, Hr, tokens_per_block, Dh]
    const int64_t* kv_table = nullptr; // paged: device table int64 [B, 2, max_blocks] of block pointers into `kv`
};

// A bounded in-launch wait of a fused decode launch expired (tllm_session::check_comm).  Distinct from 1:
// tllm_session_generate re-runs the request on the launches the session has fallen back to.
constexpr int kFusedTimedOut = 2;

} // namespace runtime
} // namespace tllm

#define HIP_OK(expr)                                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess)                                                                                          \
        {                                                                                                              \
            set_error("%s failed: %s", #expr, hipGetErrorString(_e));                                                  \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

#define RUN(expr)                                                                                                      \
    do                                                                                                                 \
    {                                                                                                                  \
        const int _rc = (expr); /* (the callee's code travels up: kFusedTimedOut is told apart from a plain failure) */   \
        if (_rc != 0)                                                                                                  \
            return _rc;                                                                                                \
    } while (0)

struct tllm_session
{
    using TensorRec = tllm::runtime::TensorRec;
    using Linear = tllm::runtime::Linear;
    using Layer = tllm::runtime::Layer;

    // ---- configuration
    int num_layers = 0, num_heads = 0, hidden = 0, inter = 0, vocab = 0, max_pos = 2048;
    int tp = 1, rank = 0;
    int quant_mode = 0;
    int neox = 1;
    float eps = 1e-6f;
    std::string wo_precision = "int8";
    std::string network_json; // the traced network an engine file carries (Builder.build_engine), verified by load_engine
    // derived
    int Hr = 0, Dh = 0, Dr = 0, Ir = 0, Vr = 0;
    // grouped-query attention (config key num_kv_heads, default num_heads): K/V heads of the model and of this rank (Hkv / tp), and
    // the extent of a fused QKV row of this rank, (Hr + 2 * Hkvr) * Dh
    int num_kv_heads = 0, Hkvr = 0, QKVr = 0;
    bool sq = false, woq = false, per_token = false, per_channel = false;
    int kv_dtype = tllm::kernels::DT_HALF; // cache element: DT_INT8 (quant_mode bit 32) or DT_FP8 (OCP E4M3, bit 64), never both
    size_t kv_esz() const { return kv_dtype == tllm::kernels::DT_HALF ? 2 : 1; }
    int wtype = tllm::kernels::W_FP16; // of every layer's five projections (lm_head stays fp16)

    std::map<std::string, TensorRec> tensors;
    std::vector<Layer> layers;
    const void* emb = nullptr;
    const void* lnf = nullptr;
    Linear head;
    bool finalized = false;
    std::vector<int32_t> group;
    bool packed = false;       // remove_input_padding: the context phase runs on the real tokens only
    int ctx_tokens = 0;        // ... their number in the current prompt batch
    int32_t* cu_dev = nullptr;    // [B + 1] exclusive prefix sum of the input lengths
    int32_t* last_rows = nullptr; // [B] packed row of every sequence's last prompt token
    // paged KV cache (plugin field paged_kv_cache; K/kvCacheUtils.h KVBlockArray, PY/runtime/kv_cache_manager.py): the session
    // owns the pool and hands every sequence its blocks at setup - the whole table is known then, so the generation graph
    // needs no host-side block allocation between steps
    bool paged_kv = false;
    int tokens_per_block = 64, max_blocks = 0;
    // session key paged_append (a key of the runtime, not of the engine header): the append passes - append, verify, the lookup
    // loops - serve the paged cache through the table (the paged instances of kernels/append_attn.hip).  Without it a paged
    // session refuses them as it always did
    bool paged_append = false;
    size_t kv_elems = 0; // elements of one layer's cache / pool
    bool force_comm = false; // tests: run the TP collectives on a 1-rank communicator too (RCCL inside the captured graph)
    // session key no_comm = 1: a rank's launches WITHOUT its collectives (all-reduces and the logits all-gather are skipped, nothing
    // else changes) - the per-rank step time of a tensor-parallel shard on one GPU, bench.py's prediction for the first multi-GPU
    // run.  TIMING ONLY: hidden states are one rank's partial sums.
    bool no_comm = false;
    bool debug_taps = false; // tests: keep every layer's GEMV inputs of the last generation step (tllm_session_get_tap[_ex])
    // tap w of layer li: the activation exactly as GEMV w consumes it, behind its prologue (RMSNorm / split merge / quantiser):
    //   0 QKV input [B, D]   1 O-projection input [B, Dr]   2 gate|up input [B, D]   3 down-projection input [B, Ir]
    // fp16, or s8 where the path quantises (SmoothQuant) - the four quantisers of the SmoothQuant layer;
    //   4 the layer's input row of the residual stream [B, D], always fp16 (tap 4 of layer num_layers - 1 + 1 does not exist:
    //     the last layer's output is what the head consumes)
    static constexpr int kTaps = 5;
    char* tap_buf[kTaps] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // each [num_layers][B][width] x 2 bytes
    int tap_width(int which) const { return which == 1 ? Dr : (which == 3 ? Ir : hidden); }
    char* tap_ptr(int which, int li) const { return tap_buf[which] + (size_t) li * B * tap_width(which) * 2; }

    // ---- runtime state (setup)
    int B = 0, max_in = 0, max_new = 0, Smax = 0;
    // beam search: Bc prompts, `beam` hypotheses each; B = Bc * beam sequences in the generation phase (B == Bc otherwise)
    int Bc = 0, beam = 1;
    int logit_rows = 0; // rows of the last head launch (Bc after the prompt, B after a generation step)
    float* cum_log_probs = nullptr; // [B]
    int32_t *parent_ids = nullptr, *cache_ind = nullptr, *in_len_ctx = nullptr; // [B, Smax], [B, Smax], [Bc]
    std::vector<void*> allocs;
    void *x = nullptr, *qkv = nullptr, *ctx = nullptr, *g = nullptr, *u = nullptr, *inter_buf = nullptr, *tmp = nullptr;
    int8_t* q8 = nullptr;   // quantised activations (context path) [B*S, max(D, I)]
    float* qscale = nullptr; // per-token scales [B*S]
    float* logits = nullptr; // [B, V] (or gathered [tp, B, Vr])
    float* logits_local = nullptr;
    void* last_hidden = nullptr;
    // tensor-parallel decode with the fused peer-to-peer seam (kernels/p2p_allreduce.hip): this rank's partial projection
    // output, the normalised (+ quantised) row the next GEMV consumes, its per-token scales
    void* ar_partial = nullptr; // [B, D] fp16
    void* ar_norm = nullptr;    // [B, D] fp16 | s8
    float* ar_scale = nullptr;  // [B]
    void* mmha_ws = nullptr;
    void* ctx_ws = nullptr; // V^T scratch of the MFMA context attention
    int32_t *ids_in = nullptr, *cur_ids = nullptr, *out_ids = nullptr, *seq_len = nullptr, *in_len = nullptr,
            *masked = nullptr, *finished = nullptr, *last_tok = nullptr;
    bool has_context = false;       // a prompt has been uploaded since setup (tllm_session_append needs a live cache)
    int32_t* append_last = nullptr; // [B]: tokens appended per sequence (the gather of the appended rows' last one): n for every
                                    // sequence, or the lengths of a ragged append - then the attention's n_per_seq too
    int append_max_end = 0;         // > 0 during a ragged append pass: max_b (past[b] + n_b), and append_last holds the lengths
    int64_t append_wave_launches = 0, append_mfma_launches = 0; // attention launches of tllm_session_append since setup, by kernel
    const float* rope = nullptr;
    int rope_len = 0;
    float* rope_row = nullptr; // [B, Dh/2, 2]: cos/sin row of the next generation step (written by the sampler)
    int32_t* rope_pos = nullptr; // [B]: the position that row belongs to (tllm_session_get_step_state)
    // the split-KV plan of the attention (kernels.h): in_launch_merge - the last split of a head to arrive merges inside the launch
    // (mmha_decode.hip step 6), its tickets at the head of mmha_ws - or the finest split with its own combine launch
    tllm::kernels::MmhaPlan attn_plan;
    // r05: batch-1 greedy decode of a SmoothQuant engine runs the QKV projection, RoPE, the cache append and the attention of a head
    // in ONE launch (kernels/qkv_attn_fused.hip); session key fuse_qkv_attention = 0 keeps the two launches (A/B, parity tests)
    int fuse_qkv_cfg = -1;          // -1 auto, 0 off
    bool qkv_attn_fused = false;    // decided at setup
    // ... and the O-projection + residual of the layer as a third stage of that launch (static SmoothQuant: the context row
    // travels as its int8 image); session key fuse_o_projection = 0 keeps the GEMV launch
    int fuse_o_cfg = -1;
    int fused_retries = 0;          // requests tllm_session_generate ran a second time behind an expired in-launch wait
    int dual_mlp_cfg = -1;          // session key dual_mlp_gemm = 0: prefill fc / gate as two GEMMs + the SwiGLU-quantiser pass (A/B)
    int fused_max_spins = -1;       // session key fused_max_spins: bound of the in-launch waits (tests: 0 = the first miss times out)
    bool o_fused = false;
    uint64_t* fused_xchg = nullptr; // granule exchange, shared by all layers
    uint32_t* step_epoch = nullptr; // advanced by the sampler once per generation step (the granule tags derive from it)
    uint32_t* fused_err = nullptr;  // raised by a bounded wait that expired
    uint32_t timing_tag = 0;        // explicit tags of eager launches outside a step (tllm_session_time_kernel)
    // r06: the gated MLP of a decode step (gate|up GEMV + down GEMV) in ONE launch (kernels/mlp_fused.hip): batch 1, tp 1, static
    // SmoothQuant, the 7B extents.  Bit-identical to the two GEMV launches but measured 1 us per layer SLOWER (26.4 against
    // 16.4 + 9.0 us, profiles/r06_mlp_one_launch.txt), so it runs only when asked for: session key fuse_mlp = 1
    int fuse_mlp_cfg = 0;
    bool mlp_fused_dec = false;  // decided at setup
    uint8_t* mlp_flags = nullptr; // one byte per workgroup (shared by all layers), zero before the first launch and after a failed one
    uint64_t* mlp_timing = nullptr;
    uint64_t* fused_timing = nullptr; // session key fused_timeline = 1: stage clock of the fused launch, [Hr * 8][16] ticks
    bool fused_timeline = false;
    void* ctx_q8 = nullptr;
    // The tail of a generation step ("The tail of the step").
    // Rows [0, head_resident_rows) of this rank's lm_head shard load with the allocating cache policy in the one-row head launch,
    // the rest streams `nt` (GemvParams::resident_rows): measured 2 us shorter at 7B, cause open - not shown to be Infinity Cache
    // hits.  Session key head_resident_pct: -1 = the rule of decide_head_residency (setup), 0 .. 100 = that share of the rows.
    int head_resident_cfg = -1;
    int head_resident_rows = 0; // decided at setup
    // Greedy, batch 1, one vocabulary part: the head launch leaves per-wave arg-max pairs and the greedy step reduces those
    // instead of reading the logits again.  Session key greedy_partials = 0: the scan.
    int greedy_partials_cfg = 1;
    void* argmax_part = nullptr;     // kArgmaxPairs pairs
    bool head_partials_live = false; // the last head launch wrote them and no sampler has run since
    int64_t greedy_partials_used = 0; // greedy-step launches ENQUEUED with the pairs since setup (a captured step counts once per
                                      // capture, not per replay): tllm_session_greedy_partials_used, so that a test sees a quiet fall-back
    int gemv_resident_rows = 0;      // the two lm_head options of the next gemv() call (run_head sets and clears them)
    void* gemv_argmax_part = nullptr;
    int end_id = -1;
    bool sampling_on = false;       // tllm_session_set_sampling: run_sampler launches kernels/sampling.hip with `sampling`
    tllm::kernels::SamplingParams sampling; // configuration fields only; pointers and shapes are filled per launch
    // tllm_session_score (session_context.cpp): session key score_chunk_rows = rows of fp32 logits per head GEMM (0: as many as fit
    // 64 MiB).  The buffers below exist from the first score call on and go with the others in free_runtime
    int score_chunk_cfg = 0;
    struct ScoreBuffers
    {
        int chunk = 0;               // rows of `logits`
        int max_rows = 0;            // Bc * (max_in - 1): rows that can have a next token
        void* hidden = nullptr;      // fp16 [max_rows, D]: the gathered final hidden rows (ln_f leaves its result in tmp)
        float* logits = nullptr;     // f32 [chunk, Vr]
        int32_t* src_rows = nullptr; // [max_rows] row of x
        int32_t* targets = nullptr;  // [max_rows] the next token's id
        float* rec_local = nullptr;  // [max_rows, 8] this rank's records
        float* rec_all = nullptr;    // [tp, max_rows, 8] (tensor parallel: the all-gather's result)
        float* log_probs = nullptr;  // [max_rows]
        int32_t* top1 = nullptr;     // [max_rows]
    } score;
    // tllm_session_verify / tllm_session_generate_lookup (run_verify): the buffers exist from the first verify pass after a setup on
    struct VerifyBuffers
    {
        float* logits = nullptr;    // f32 [B * kVerifyMaxTokens, Vr]: the logits rows of one pass
        int32_t* targets = nullptr; // [B * kVerifyMaxTokens] ids[b][i + 1], -1 on a sequence's last row
        float* rec = nullptr;       // [B * kVerifyMaxTokens, 8] token_logprob records
        float* log_probs = nullptr; // [B * kVerifyMaxTokens]
        int32_t* top1 = nullptr;    // [B * kVerifyMaxTokens]
        int32_t* draws = nullptr;   // [B * kVerifyMaxTokens] the sampler's draw of every row (a sampled pass: launch_spec_sample_rows)
        int32_t* accepted = nullptr; // [B]
        int32_t* limit = nullptr;    // [B] largest sequence length the lookup loop may leave
        int32_t* state = nullptr;    // [B, 4] the prompt lookup's {seq_len, finished, draft_len, frozen}
    } verify;
    int verify_n = 0; // ids per sequence of the last verify pass (0: none since setup)
    const int32_t* verify_cmp = nullptr; // what that pass's accept step compared the drafts with: verify.top1 or verify.draws
    std::vector<int32_t> score_pos;  // host: output slot b * max_in + t + 1 of every scored row of the current call
    std::vector<float> score_lp_host;
    std::vector<int32_t> score_top_host;
    // ---- LoRA adapters per sequence (session_lora.cpp; the rule: kernels.h LoraShrinkParams).  Session keys
    // lora_max_rank (0 = off), lora_max_adapters, lora_target_modules.  The adapters' device buffers are allocated by the first
    // lora call and live until the session is destroyed, at fixed addresses; what a setup allocates is the selection, the row map
    // of the prefill passes and the shrink's result.
    enum LoraModule { LM_Q = 0, LM_K, LM_V, LM_O, LM_GATE, LM_UP, LM_DOWN, LM_COUNT };
    enum LoraSite { LS_QKV = 0, LS_DENSE, LS_GATE_UP, LS_PROJ, LS_COUNT };
    int lora_rank = 0, lora_adapters = 1;
    bool lora_mod[LM_COUNT] = {false, false, false, false, false, false, false}; // lora_target_modules
    bool lora_site_on(int site) const
    {
        if (lora_rank <= 0)
            return false;
        switch (site)
        {
        case LS_QKV: return lora_mod[LM_Q] || lora_mod[LM_K] || lora_mod[LM_V];
        case LS_DENSE: return lora_mod[LM_O];
        case LS_GATE_UP: return lora_mod[LM_GATE] || lora_mod[LM_UP];
        default: return lora_mod[LM_DOWN];
        }
    }
    struct LoraSiteBuf
    {
        void* a[tllm::kernels::kLoraMaxAdapters]; // fp16 [nseg * lora_rank, K] per slot
        void* b[tllm::kernels::kLoraMaxAdapters]; // fp16 [N, lora_rank] per slot
        tllm::kernels::LoraAdapterRec* table;     // device [lora_adapters]
    };
    std::vector<LoraSiteBuf> lora_sites; // [num_layers][LS_COUNT]; empty until the first lora call
    std::vector<void*> lora_allocs;
    bool lora_committed[tllm::kernels::kLoraMaxAdapters] = {false, false, false, false, false, false, false, false};
    struct LoraStaged
    {
        std::vector<int64_t> dims;
        std::vector<uint16_t> data;
    };
    std::map<std::string, LoraStaged> lora_staged[tllm::kernels::kLoraMaxAdapters]; // host copies between set_tensor and commit
    std::vector<int32_t> lora_sel_host; // [B], -1 = none
    int32_t* lora_sel = nullptr;        // device [B]: the row -> adapter map of a generation step
    int32_t* lora_rows = nullptr;       // device [prompt rows]: ... of a prefill / append pass (lora_map_rows)
    float* lora_t = nullptr;            // f32 [rows, 3 * lora_rank]
    int lora_alloc();                   // the adapters' buffers and tables, once
    void lora_site_shape(int site, int* K, int* nseg, int* seg_n) const;
    int lora_map_rows(int M, int rows_per_seq, hipStream_t st); // lora_rows <- lora_sel (rows_per_seq 0: the packed prompt layout)
    // shrink + expand of one site of layer li on M rows: xin (fp16 [M, K of the site]) through prologue pro (PRO_NONE |
    // PRO_RMSNORM with gamma) is the row the base projection consumed; the site's output buffers are updated in place
    int lora_apply(int li, int site, int M, const void* xin, int pro, const void* gamma, const int32_t* rows, hipStream_t st);

    hipGraphExec_t graph = nullptr;
    int64_t graph_captures = 0; // step graphs captured since the session was created (tllm_session_graph_captures)
    hipStream_t graph_stream = nullptr;
    uint64_t graph_comm_gen = 0;   // comm::p2p::generation() the step graph was captured under
    uint64_t comm_err_seen = 0;    // comm::p2p::error_generation() at this session's last check_comm
    hipStream_t own_stream = nullptr; // used when the caller passes the NULL stream (it cannot be captured)

    // ---- optional per-launch instrumentation (tllm_session_profile): event pairs around every launch class
    enum ProfClass
    {
        PC_GEMV_LAYER = 0,
        PC_GEMV_HEAD = 1,
        PC_ATTENTION = 2,
        PC_OTHER = 3,
        PC_COMM = 4,
        PC_COUNT = 5
    };
    bool profiling = false;
    // tllm_session_time_kernel: launch just stage <only_kernel> of every layer (DecodeStep says which launch sites an id means)
    int only_kernel = -1;
    int gemv_cls = PC_GEMV_LAYER;
    struct ProfRec
    {
        hipEvent_t a, b;
        int cls;
    };
    std::vector<ProfRec> prof;

    hipStream_t pick(tllm_stream_t stream)
    {
        if (stream)
            return reinterpret_cast<hipStream_t>(stream);
        if (!own_stream)
            (void) hipStreamCreate(&own_stream);
        return own_stream;
    }

    ~tllm_session(); // session.cpp

    // ---- session_weights.cpp
    const TensorRec* find(const std::string& name, bool required = true);
    int want(const TensorRec* t, const std::string& name, int32_t dtype, int64_t numel);
    // resolve one linear layer "prefix" with logical shape [N, K] for this session's quantisation mode
    int resolve_linear(const std::string& prefix, int N, int K, Linear& L, bool force_fp16 = false);
    int scalar_f32(const std::string& name, const float** out);

    // ---- session_setup.cpp
    template <typename T>
    int dalloc(T** p, size_t bytes); // device memory the session owns until free_runtime (defined below the struct)
    void free_runtime();
    void drop_graph(); // the captured step no longer matches what an eager step would issue
    int alloc_buffers();
    int decide_decode_form();       // attention split layout, qkv_attn_fused / o_fused / mlp_fused_dec
    void decide_head_residency();   // head_resident_rows
    int alloc_decode_form_buffers(); // what the forms decide_decode_form chose need
    // After a stream synchronisation: did a fused decode launch or a peer-to-peer collective of this session time out?  Fails
    // the call then, and withdraws the decode form / the transport that timed out.
    int check_comm();

    // ---- session_context.cpp
    // context: plain GEMM on M rows (activation already in the operand type; per-token SmoothQuant: its scales are in qscale)
    int gemm(const Linear& L, int M, const void* a, void* c, int out_dtype, hipStream_t st, const void* residual = nullptr,
        const void* silu_gate = nullptr);
    int profile_prefill_gemms(int M);
    int context_norm(int M, const void* gamma, const float* static_scale, hipStream_t st);
    int context_attention(const Layer& L, bool q_in_attn, hipStream_t st);
    int context_gate_up(int li, int M, const void* a_in, const void** p_in, hipStream_t st);
    int context_proj_residual(const Linear& L, int M, const void* in, bool fuse_res, hipStream_t st);
    // one decoder layer of the prefill schedule on M rows; append_n > 0: with the append attention (n rows per sequence)
    int context_layer(int li, int M, int append_n, int max_past, hipStream_t st);
    int run_context(hipStream_t st);
    // tllm_session_append: the prefill schedule on B * n appended rows (ids in ids_in) onto the live cache, head on row n - 1
    int append_attention(const Layer& L, int n, int max_past, hipStream_t st);
    int run_append(int n, int max_past, hipStream_t st);
    // the ragged pass: lengths already in append_last, n = their maximum, max_end as AppendAttnParams
    int run_append_ragged(int n, int max_end, hipStream_t st);
    int append_layers(int n, int max_past, hipStream_t st); // embedding + every layer on the B * n rows (ids in ids_in)
    // tllm_session_verify: append_layers, then the head on ALL B * n rows (fp32, verify.logits), their scoring (verify.top1 /
    // .log_probs against the next id of the row) and the accept step in the sampler's place; limit: device int32 [B] or null.
    // sampled (tllm_session_verify_sampled) under a configuration that is not plain arg-max: the sampler draws on all B * n rows
    // (verify.draws) and the accept step compares the drafts with the draws; otherwise no launch is added and none differs.
    int run_verify(int n, int max_past, const int32_t* limit, bool sampled, hipStream_t st);
    int verify_buffers(); // allocates `verify` on first use after a setup
    // ln_f of R hidden rows into tmp (fp16), and lm_head as a prefill GEMM on `rows` of them with fp32 output [rows, Vr]: the
    // head of scoring and of a verify pass (run_head's fused GEMV leaves at most B rows, in the session's logits)
    int head_norm(const void* h, int R, hipStream_t st);
    int head_gemm_f32(const void* a, int rows, float* out, hipStream_t st);
    // score: enqueue ln_f -> lm_head in row chunks -> partial records (-> all-gather) -> merge on the rows of x that have a next
    // token (between run_context and the sampler, which reuses x); collect: after the stream is synchronised, scatter to the host
    int score_enqueue(const int32_t* input_ids, const int32_t* input_lengths, hipStream_t st);
    void score_collect(float* log_probs, int32_t* top1_ids);

    // ---- session_decode.cpp
    template <typename F>
    int timed(int cls, hipStream_t st, F&& f); // f(), between an event pair of class cls while profiling (defined below the struct)
    // decode: fused skinny GEMM.  `tap`: where the launch leaves its prologue's result (x_pro_out), or nullptr
    int gemv(const Linear& L, int M, int pro, int epi, const void* xin, int64_t ldx, const void* gamma, const float* in_qscale,
        const void* residual, const float* epi_scale, void* y, int64_t ldy, int out_dtype, const Linear* up, hipStream_t st,
        const float* row_scales = nullptr, void* tap = nullptr);
    int allreduce(void* buf, int64_t n, hipStream_t st);
    int run_head(const void* h, int rows, hipStream_t st, bool normalised = false);
    tllm::kernels::GreedyParams greedy_params();
    int run_sampler(int advance, hipStream_t st);
    struct DecodeStep; // what is fixed for one generation step (session_decode.cpp)
    DecodeStep plan_decode_step(hipStream_t st);
    int tap_copy(const DecodeStep& ds, int which, int li, const void* src, int elem_bytes);
    int stage_front(const DecodeStep& ds, int li);
    int stage_qkv(const DecodeStep& ds, int li);
    int stage_attention(const DecodeStep& ds, int li);
    int stage_o_proj(const DecodeStep& ds, int li);
    int stage_seam(const DecodeStep& ds, const void* gamma, const float* quant_scale, int quant);
    int stage_mlp_one(const DecodeStep& ds, int li);
    int stage_gate_up(const DecodeStep& ds, int li);
    int stage_down(const DecodeStep& ds, int li);
    int run_decode_step(hipStream_t st);
};

// The two member templates: every unit that uses one must see its body, so they are here and not in a .cpp file.
template <typename T>
int tllm_session::dalloc(T** p, size_t bytes)
{
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 16) != hipSuccess)
    {
        tllm::set_error("session: hipMalloc(%zu) failed", bytes);
        return 1;
    }
    allocs.push_back(d);
    *p = static_cast<T*>(d);
    return 0;
}

template <typename F>
int tllm_session::timed(int cls, hipStream_t st, F&& f)
{
    if (!profiling)
        return f();
    ProfRec r;
    r.cls = cls;
    (void) hipEventCreate(&r.a);
    (void) hipEventCreate(&r.b);
    (void) hipEventRecord(r.a, st);
    const int rc = f();
    (void) hipEventRecord(r.b, st);
    prof.push_back(r);
    return rc;
}
