// Host-side launch interface of the gfx950 kernels.  Every launcher enqueues on `stream`, never
// synchronises, returns 0 on success or a negative code (and sets tllm::set_error) on a shape it
// cannot run.  SURVEY.md §8a row ids (A2, A5, ...) are cited per kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <stddef.h>
#include <stdint.h>

namespace tllm
{

void set_error(const char* fmt, ...);
const char* last_error();

namespace kernels
{

enum DType : int32_t
{
    DT_FLOAT = 0,
    DT_HALF = 1,
    DT_INT8 = 2,
    DT_INT32 = 3,
    DT_FP8 = 6 // OCP E4M3 bytes (KV cache only; the value of TLLM_FP8)
};

// ---------------------------------------------------------------------------------------------
// Skinny GEMM (M <= 8 rows; decode).  y[m,n] = epi( scale * sum_k x'[m,k] * W[n,k] ),  x' = pro(x).
//   A7 (fp16 Gemm), A8 (weight-only int8/int4), A10 (SmoothQuant int8xint8->int32), with the
//   A5 RMSNorm / A11 activation quantisers as prologues and A6 SwiGLU / residual add as epilogues.
// HBM-bound: streams W once with 16-byte non-temporal loads, x' staged in LDS once per workgroup.
// ---------------------------------------------------------------------------------------------
enum WType : int32_t
{
    W_FP16 = 0,     // W fp16 [N, K] row-major
    W_INT8_WOQ = 1, // W u8 = q + 128, [N, ldw] (k contiguous), fp16 per-column scales; x fp16
    W_INT4_WOQ = 2, // W packed nibbles n = q + 8, see weight_layout.h; fp16 per-column scales; x fp16
    W_INT8_SQ = 3   // W s8 [N, ldw]; x s8; int32 accumulate; fp32 per-row x per-col scales
};

enum Prologue : int32_t
{
    PRO_NONE = 0,            // x already in the operand type (fp16, or s8 for W_INT8_SQ)
    PRO_RMSNORM = 1,         // x fp16 -> rmsnorm(x) * gamma (fp16)
    PRO_RMSNORM_QSTATIC = 2, // ... -> s8 with static scale act_scale[0]          (W_INT8_SQ)
    PRO_RMSNORM_QDYN = 3,    // ... -> s8 with per-token scale amax/127            (W_INT8_SQ)
    PRO_QSTATIC = 4,         // x fp16 -> s8 static                                (W_INT8_SQ)
    PRO_QDYN = 5             // x fp16 -> s8 per-token                             (W_INT8_SQ)
};

enum Epilogue : int32_t
{
    EPI_NONE = 0,
    EPI_RESIDUAL = 1,      // y = fp16(fp16(v) + residual)
    EPI_SWIGLU = 2,        // W rows [0,N) gate (mlp.fc), [N,2N) up (mlp.gate): y = fp16(silu(g) * u)
    EPI_SWIGLU_QSTATIC = 3 // ... then s8 with static scale epi_scale[0]
};

struct GemvParams
{
    int32_t wtype = W_FP16, pro = PRO_NONE, epi = EPI_NONE;
    int32_t out_dtype = DT_HALF; // DT_HALF | DT_FLOAT | DT_INT32 (SQ only) | DT_INT8 (EPI_SWIGLU_QSTATIC)
    int32_t M = 1, N = 0, K = 0; // N = output columns (for SWIGLU the weight has 2N rows)
    const void* x = nullptr;     // [M, ldx] fp16 or s8
    int64_t ldx = 0;             // elements
    const void* w = nullptr;
    int64_t ldw = 0;                  // bytes per weight row, multiple of 16
    const void* w_up = nullptr;       // SWIGLU: the "up" matrix (mlp.gate) [N, ldw]; null => rows [N, 2N) of w
    const void* scale_col = nullptr;  // WOQ: fp16 [N]; SQ: f32 [N] or [1]
    const void* scale_col_up = nullptr; // SWIGLU: scales of w_up; null => scale_col + N (per-channel) / scale_col
    const float* scale_row_up = nullptr; // SWIGLU + SQ static: act_scale of the up GEMM [1]; null => scale_row
    const float* scale_row = nullptr; // SQ: f32 [M] or [1] (ignored when the prologue quantises per token)
    int32_t per_channel = 0, per_token = 0;
    const void* gamma = nullptr; // fp16 [K]
    float eps = 1e-6f;
    const float* act_scale = nullptr; // PRO_*QSTATIC: f32 [1] (scale_to_int)
    float* dyn_scale_out = nullptr;   // optional f32 [M]: per-token scales computed by the prologue
    void* x_pro_out = nullptr;        // optional [M, K]: the prologue's result (fp16 or s8), written by workgroup 0
    const void* residual = nullptr;   // fp16 [M, ldy]
    const float* epi_scale = nullptr; // EPI_SWIGLU_QSTATIC: f32 [1]
    void* y = nullptr;
    int64_t ldy = 0; // elements
    // The two options of the lm_head launch (fp16 weights, M = 1, no epilogue; any other call that sets one is refused):
    //   resident_rows  rows [0, resident_rows) of W load with the allocating cache policy, the rows from it on stream non-temporally
    //                  like every layer weight.  Measured on the 7B head: 2 us shorter from 75 % of the rows up; built so that the
    //                  rows could stay in the Infinity Cache between steps, which the counters do NOT confirm - the cause is open
    //                  (profiles/lm_head_residency.txt).  Rounded up to the kernel's row pair; > N means N.  0: the whole matrix
    //                  streams.  Results do not depend on it.
    //   argmax_part    fp32 output only: kArgmaxPairs pairs {float value, int32 index} - per wave of the grid the arg-max of the
    //                  outputs it finished (greater value wins, ties go to the lowest index; {-inf, INT32_MAX} for none and for
    //                  the slots beyond the grid).  launch_greedy_step reduces them instead of reading the logits again.
    int32_t resident_rows = 0;
    void* argmax_part = nullptr;
};
constexpr int kArgmaxPairs = 2048; // 16 KB: one pair per wave of 512 workgroups (two per CU of a 256-CU device)

int launch_gemv(const GemvParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// RMSNorm (A5) with optional fused int8 quantisation (A11 pattern of layernormKernels.cu:162-183).
//   y = fp16( fp16(x * rsqrt(mean(x^2) + eps)) * gamma ); q = sat(rni(y * s)).
// ---------------------------------------------------------------------------------------------
struct RmsnormParams
{
    int32_t M = 0, N = 0;
    const void* x = nullptr;        // fp16 [M, N]
    // residual / sum_out: nothing in the product sets them (neither the plugins nor the session) - both kernels implement them and
    // tests/test_gpu_pointwise_instances.py (through tllm_rmsnorm) is what keeps them correct
    const void* residual = nullptr; // optional fp16 [M, N]: x <- x + residual first, sum written to sum_out
    void* sum_out = nullptr;        // fp16 [M, N] (required when residual != nullptr)
    const void* gamma = nullptr;    // fp16 [N]
    float eps = 1e-6f;
    void* y = nullptr;                // fp16 [M, N] (may be null when only q is wanted)
    int8_t* q = nullptr;              // optional s8 [M, N]
    const float* static_scale = nullptr; // f32 [1] -> static quant
    float* dyn_scale_out = nullptr;      // f32 [M] -> per-token dynamic quant (amax / 127)
    // LayerNorm flavour (LayernormQuantization plugin, K/layernormKernels.cu:61-205): y = fp16((x - mean) * rstd * gamma + beta)
    int32_t layernorm = 0, use_diff_of_squares = 1;
    const void* beta = nullptr; // fp16 [N]
};
int launch_rmsnorm(const RmsnormParams& p, hipStream_t stream);
// The one dispatch rule of launch_rmsnorm, host only (no pointer is followed): the kernel it runs for p as
// 1 = rmsnorm_kernel<1>, 2 = rmsnorm_kernel<8>, 3 + 8 * NV = rmsnorm_reg_kernel<NV> (NV = 1, 2, 4); 0 for an empty problem
// (M <= 0 or N <= 0: nothing to launch); -1 with set_error where it refuses.
// kernel: 0 = the launcher's choice; 1 / 2 = that rmsnorm_kernel; 3 = rmsnorm_reg_kernel (NV by N) - a forced kernel whose
// precondition does not hold is refused (-1), never replaced.
int rmsnorm_kernel_for(const RmsnormParams& p, int kernel = 0);
// launch_rmsnorm with the kernel forced as above (tests: both kernels on the same row)
int launch_rmsnorm_kernel(const RmsnormParams& p, int kernel, hipStream_t stream);

// A11: quantize_tensor (static per-tensor) and quantize_per_token.  K/quantization.cu:31-128.
int launch_quantize_tensor(int8_t* dst, const void* src, int32_t src_dtype, int64_t size, const float* scale,
    hipStream_t stream);
int launch_quantize_per_token(int8_t* dst, const void* src, int32_t src_dtype, int64_t rows, int64_t cols,
    float* scale_out, hipStream_t stream);

// A6 standalone SwiGLU: y = fp16(silu(a) * b), a,b fp16 [n].
int launch_swiglu(void* y, const void* a, const void* b, int64_t n, hipStream_t stream);
// the same, quantised on the way out: q = sat(rni(float(fp16(silu(a) * b)) * scale[0])) (static per-tensor SmoothQuant)
int launch_swiglu_quant(int8_t* q, const void* a, const void* b, int64_t n, const float* scale, hipStream_t stream);
// elementwise fp16 add: y = a + b
int launch_add(void* y, const void* a, const void* b, int64_t n, hipStream_t stream);
// A16 embedding gather: out[t, :] = table[ids[t], :] (fp16), ids int32; out-of-range id -> zeros.
int launch_embedding(void* out, const int32_t* ids, const void* table, int64_t tokens, int32_t hidden, int32_t vocab,
    hipStream_t stream);
// A16 gather_last_token_logits input: out[b,:] = hidden[b, last_token_ids[b]-1, :] (padded layout)
int launch_gather_last_token(void* out, const void* hidden, const int32_t* last_token_ids, int32_t batch, int32_t seq,
    int32_t hidden_size, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Decode attention (A2/A3): masked multi-head attention for one new token per sequence, with RoPE,
// KV-cache write (fp16, int8 or fp8 E4M3) and split-KV across workgroups.
// ---------------------------------------------------------------------------------------------
struct MmhaParams
{
    int32_t batch = 0, num_heads = 0, head_size = 0;
    int32_t rotary_dim = 0, neox = 1;
    float inv_sqrt_dh = 1.f;
    int32_t kv_dtype = DT_HALF; // cache element: DT_HALF, DT_INT8 or DT_FP8 (one byte per element, the two scales below)
    int32_t max_seq_len = 0;    // cache capacity Smax
    int32_t max_input_len = 0; // padded prompt length (RoPE position = timestep - (max_input_len - input_len[b]))
    const void* qkv = nullptr; // fp16 [B, 3*H*Dh] (q | k | v)
    void* kv_cache = nullptr;  // [B, 2, H, Smax, Dh] fp16, s8 or e4m3
    const int32_t* sequence_length = nullptr; // [B] device: tlength (slots already used)
    const int32_t* input_lengths = nullptr;   // [B] device
    const int32_t* masked_tokens = nullptr;   // [B, Smax] device or null
    int32_t timestep_host = -1;               // past_kv_len from the host scalar; -1 => use sequence_length[0]
    const float* kv_scale_orig_quant = nullptr; // f32 [1]
    const float* kv_scale_quant_orig = nullptr; // f32 [1]
    const float* rope_table = nullptr;          // f32 [max_pos, rotary_dim/2, 2] (cos, sin)
    int32_t rope_table_len = 0;
    const float* rope_row = nullptr; // optional f32 [B, rotary_dim/2, 2]: this step's cos/sin row, prepared on the
                                     // device by the sampler (removes the length -> position -> table dependency)
    int32_t rows_per_group = 0;      // cache rows per lane group and split: 4 (finest split), 12 or 16 - MmhaPlan::rows_per_group,
                                     // set by mmha_bind_workspace; the launcher refuses 0
    // beam search (MM/...Template.h:1137-1146, :1624-1631): `batch` counts batch x beam sequences; sequence bb = b * beam_width
    // + k reads the K/V of timestep t from the cache rows of sequence b * beam_width + cache_indirection[bb, t]
    const int32_t* cache_indirection = nullptr; // int32 [batch, max_seq_len]
    int32_t beam_width = 1;
    // paged KV cache (K/kvCacheUtils.h:34-112 KVBlockArray): instead of kv_cache, a table int64 [batch, 2, max_blocks_per_seq]
    // of device pointers to blocks laid out [H, tokens_per_block, Dh]; time step t is row t % tokens_per_block of block
    // t / tokens_per_block (tokens_per_block a power of two)
    const int64_t* block_pointers = nullptr;
    int32_t tokens_per_block = 0, max_blocks_per_seq = 0;
    // The split merge: when set (uint32 [B * H], zero before the first launch, self-resetting), the LAST split of a (sequence,
    // head) to arrive merges all partials (at most 16) inside this launch and writes the normalised context to `out` (and, with
    // tail_quant_scale, its static int8 image to tail_out_q8); null: a combine launch follows the partial launch.
    uint32_t* tail_tickets = nullptr;
    const float* tail_quant_scale = nullptr; // f32 [1]: SmoothQuant static activation scale of the O-projection's input
    void* tail_out_q8 = nullptr;             // s8 [B, H*Dh]
    void* out = nullptr;       // fp16 [B, H*Dh]
    void* workspace = nullptr; // the partials: MmhaPlan::ticket_bytes into the caller's workspace (mmha_bind_workspace)
    // grouped-query attention: Hkv K/V heads, 1 <= Hkv <= H, H % Hkv == 0, query head h reads K/V head h / (H / Hkv); 0 = num_heads.
    // With Hkv != H:  qkv is fp16 [B, (H + 2*Hkv)*Dh] (q: H*Dh | k: Hkv*Dh | v: Hkv*Dh), the cache [B, 2, Hkv, Smax, Dh], paged
    // blocks [Hkv, tokens_per_block, Dh]; tickets, workspace and `out` stay per QUERY head.
    int32_t num_kv_heads = 0;
    // query heads of one K/V head that a workgroup serves from ONE load of its cache rows: 1, 2, 4 or 8 (must divide H / Hkv; a
    // value the launcher cannot run is an error, never a substitute); 0 = the launcher's rule (mmha_default_q_tile)
    int32_t q_heads_per_workgroup = 0;
};
// the launcher's rule for q_heads_per_workgroup = 0
int mmha_default_q_tile(int32_t num_heads, int32_t num_kv_heads);
// num_kv_heads / q_heads_per_workgroup of p resolved (0 -> num_heads / the default tile) and checked; non-zero: refused, error set
int mmha_resolve_grouping(MmhaParams& p);
// The split-KV plan of a decode attention launch - the geometry, the launch rule and the workspace layout, stated once:
//   tchunk = (2048 / head_size) * rows_per_group cache slots per split (4 waves x 64 / (head_size / 8) lane groups x rows),
//   nsplit = ceil(max_seq_len / tchunk) splits per (sequence, head), at most kMmhaMaxSplits;
//   rows requested as 0: 16 while that needs <= kMmhaTailSlots splits - 12 while those need <= 8 (7 x 32 instead of 5 x 32
//   workgroups at the 1024-token bench context) - with the merge inside the launch (mmha_decode.hip step 6), else the finest
//   split, 4, with the combine launch;  4 / 12 / 16 requested: the in-launch merge iff nsplit <= kMmhaTailSlots;
//   force_combine: the combine launch whatever the split count.
// Workspace: the merge tickets uint32 [B, H] | {max, sum} float2 [B, H, nsplit] | out f32 [B, H, nsplit, Dh], the first two
// rounded up to 256 bytes; workspace_bytes covers the finest split, so one allocation serves every plan of the shape.
// A head size whose cache row is not a whole fraction of a wave (64 % (head_size / 8) != 0) or rows other than 0 / 4 / 12 / 16
// give the empty plan (rows_per_group 0, workspace_bytes 0).
constexpr int kMmhaTailSlots = 16;  // partials the in-launch merge takes
constexpr int kMmhaMaxSplits = 256; // partials the combine launch takes (one per thread)
struct MmhaPlan
{
    int32_t rows_per_group = 0, tchunk = 0, nsplit = 0;
    bool in_launch_merge = false;
    size_t ticket_bytes = 0;    // the tickets at the head of the workspace = the offset of {max, sum}
    size_t ml_bytes = 0;        // {max, sum} of this plan's split = the offset of `out` behind them
    size_t workspace_bytes = 0;
};
MmhaPlan mmha_plan(int32_t head_size, int32_t max_seq_len, int32_t batch, int32_t num_heads, int32_t rows_per_group = 0,
    bool force_combine = false);
// p.rows_per_group, p.tail_tickets and p.workspace from a plan (p.batch and p.num_heads set).  The tickets must be zero before
// the FIRST launch on a workspace (every launch re-arms them): reset_tickets enqueues that memset - the plugins per enqueue; the
// session zeroes its workspace at setup and with every prompt instead.
int mmha_bind_workspace(MmhaParams& p, const MmhaPlan& plan, void* workspace, bool reset_tickets, hipStream_t stream);
int launch_mmha(const MmhaParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Decode step, batch 1: the QKV projection (SmoothQuant int8, RMSNorm + quantiser prologue) of head h, RoPE, the cache append
// and the masked attention of head h in ONE launch (kernels/qkv_attn_fused.hip).  8 workgroups per head; the projection outputs
// and the split partials travel between them as 8-byte {tag, value} granules through `xchg`.
// ---------------------------------------------------------------------------------------------
struct FusedQkvAttnParams
{
    int32_t K = 0, num_heads = 0, head_size = 0;
    const void* x = nullptr;     // fp16 [K]: the layer's input row
    const void* gamma = nullptr; // fp16 [K]: input_layernorm
    float eps = 1e-6f;
    const void* w = nullptr; // s8 [3 * num_heads * head_size, ldw]: q | k | v rows
    int64_t ldw = 0;         // bytes
    const void* scale_col = nullptr; // SmoothQuant: f32 [3 * H * Dh] (per_channel) or [1]; weight-only: fp16 [3 * H * Dh]
    int32_t per_channel = 0;
    // W_INT8_SQ; W_INT8_WOQ: weight-only int8 rows (u8 = q + 128) against the normalised fp16 row, no quantiser; W_INT4_WOQ (r06):
    // int4 rows (ldw = K / 2 bytes, fp16 scales), two-stage form; W_FP16 (r06): fp16 rows (ldw = 2 K bytes, no scales), no quantiser,
    // no O-projection stage
    int32_t wtype = W_INT8_SQ;
    const float* act_quant_scale = nullptr;   // f32 [1]: static quantiser of the normalised row; null -> per-token (amax / 127)
    const float* act_dequant_scale = nullptr; // f32 [1]: the static activation scale of the dequantisation
    int32_t kv_dtype = DT_HALF, max_seq_len = 0; // DT_HALF or DT_INT8 (no E4M3 instance)
    float inv_sqrt_dh = 1.f;
    void* kv_cache = nullptr;                 // [2, H, Smax, Dh] fp16 or s8 (batch 1)
    const int32_t* sequence_length = nullptr; // [1] device: slots in use
    const int32_t* masked_tokens = nullptr;   // [Smax] device or null
    const float* kv_scale_orig_quant = nullptr;
    const float* kv_scale_quant_orig = nullptr;
    const float* rope_row = nullptr; // f32 [Dh / 2, 2]: this step's (cos, sin) row (NeoX pairs), prepared by the sampler
    uint64_t* xchg = nullptr;        // qkv_attn_fused_xchg_bytes(), zero before the first launch
    const uint32_t* epoch = nullptr; // device word advanced once per generation step
    uint32_t tag_mul = 1, tag_add = 1; // tag of this launch = epoch * tag_mul + tag_add (never 0, unique per launch)
    uint32_t tag_host = 0;             // non-zero: the tag itself (eager launches outside a step, e.g. kernel timing)
    uint32_t* error = nullptr;         // device word: non-zero after a bounded wait expired (a launch that finds it set returns at once)
    // polls (s_sleep + one L2 round trip, ~1 us each) a wait may take: ~50 ms against hand-offs of 1 - 5 us.  Generous enough for a
    // grid that is delayed by another queue's kernels, short enough that ONE expired wait - later launches return at entry - costs a
    // request less than a second
    int32_t max_spins = 50000;
    void* qkv_out = nullptr; // optional fp16 [3 * H * Dh]: the projection's output (before RoPE)
    void* out = nullptr;     // fp16 [H * Dh]: the attention context
    void* out_q8 = nullptr;  // optional s8 [H * Dh] = sat(rni(float(out) * out_quant_scale[0])) (the O-projection's static quantiser)
    const float* out_quant_scale = nullptr;
    void* x_pro_out = nullptr; // optional s8 [K]: the quantised operand (tap)
    uint64_t* timing = nullptr; // optional [workgroups][16] stage clock (100 MHz ticks): tools/fused_timeline.py
    // optional third stage (r05): the O-projection + residual of the same layer in the same launch,  x_out[n] = x[n] + O(ctx)[n]
    // (needs out_q8: the context row reaches the row workers as its static int8 image).  o_w null: the launch ends with the context.
    const void* o_w = nullptr;             // s8 [o_n, o_ldw]: rows of the dense projection, K = num_heads * head_size
    int64_t o_ldw = 0;                     // bytes
    int32_t o_n = 0, o_per_channel = 0;
    const void* o_scale_col = nullptr;     // SmoothQuant: f32 [o_n] (per_channel) or [1]; weight-only: fp16 [o_n]
    const float* o_scale_row = nullptr;    // f32 [1]: the static activation scale of the dequantisation
    void* x_out = nullptr;                 // fp16 [o_n]: may be x itself (every workgroup has consumed x long before)
};
size_t qkv_attn_fused_xchg_bytes(int32_t num_heads);
bool qkv_attn_fused_serves_o(int32_t num_heads, int32_t head_size, int32_t o_n, int32_t o_k, int64_t o_ldw, int32_t wtype = W_INT8_SQ,
    int32_t num_kv_heads = 0);
// (wtype / o_stage decide the instance and its dynamic LDS: the residency check - occupancy query x CUs of the current device >= grid
// - is made for exactly the launch that will run)
// kv_dtype DT_FP8, num_kv_heads != num_heads (and != 0): not served
bool qkv_attn_fused_serves(int32_t K, int32_t num_heads, int32_t head_size, int32_t max_seq_len, int32_t kv_dtype,
    int32_t wtype = W_INT8_SQ, int32_t o_stage = 0, int32_t num_kv_heads = 0);
int launch_qkv_attn_fused(const FusedQkvAttnParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Decode step, batch 1, SmoothQuant static: RMSNorm + gate|up + SwiGLU + quantiser + down-projection + residual in ONE launch
// (kernels/mlp_fused.hip, r06): 256 workgroups, the intermediate row handed over inside the launch (write-through bytes, a flag
// byte per workgroup polled through the scalar path), the down-projection's rows requested ahead of it.
// ---------------------------------------------------------------------------------------------
struct FusedMlpParams
{
    int32_t K = 0, I = 0, N = 0; // hidden size (gate|up K), intermediate size (gate|up rows, down K), down rows (= K for LLaMA)
    const void* x = nullptr;     // fp16 [K]: the layer's residual stream behind the attention block (also the residual of the output)
    void* x_out = nullptr;       // fp16 [N]: may be x itself (every workgroup has consumed x before any workgroup writes)
    const void* gamma = nullptr; // fp16 [K]: post_layernorm
    float eps = 1e-6f;
    const float* act_quant = nullptr; // f32 [1]: static quantiser of the normalised row
    const void* w_fc = nullptr;       // s8 [I, ldw]
    const void* w_gate = nullptr;     // s8 [I, ldw]
    int64_t ldw = 0;
    const void* scale_fc = nullptr;   // f32 [I] (per_channel) or [1]
    const void* scale_gate = nullptr;
    int32_t per_channel = 0;
    const float* row_fc = nullptr;    // f32 [1]: activation scale of the dequantisation (fc); row_gate null -> the same
    const float* row_gate = nullptr;
    const float* out_quant = nullptr; // f32 [1]: static quantiser of silu(fc) * gate
    void* inter = nullptr;            // optional s8 [I]: the intermediate row as the two-launch form leaves it (taps)
    const void* w_proj = nullptr;     // s8 [N, ldw_proj]
    int64_t ldw_proj = 0;
    const void* scale_proj = nullptr; // f32 [N] (per_channel_proj) or [1]
    int32_t per_channel_proj = 0;
    const float* row_proj = nullptr;  // f32 [1]
    uint8_t* flags = nullptr;         // the exchange area (a 64-byte line per workgroup: its int8 outputs + the tag; a line per group
                                      // of 16): mlp_fused_flag_bytes(), zero before the first launch
    uint32_t* error = nullptr;        // device word: bit 16 after a bounded wait expired (a launch that finds it set returns at once)
    int32_t max_spins = 50000;
    void* x_pro_out = nullptr;  // optional s8 [K]: the quantised operand (tap)
    uint64_t* timing = nullptr; // optional [256][16] stage clock
};
size_t mlp_fused_flag_bytes();
bool mlp_fused_serves(int32_t K, int32_t I, int32_t N);
int launch_mlp_fused(const FusedMlpParams& p, hipStream_t stream);

// RoPE table builder (host -> device buffer owned by caller): cos/sin(pos / 10000^(2j/rot)) in fp32,
// formula of K/decoderMaskedMultiheadAttentionUtils.h:1511-1515.
void fill_rope_table_host(float* table, int32_t max_pos, int32_t rotary_dim);

// ---------------------------------------------------------------------------------------------
// Context attention (A4): RoPE + KV-cache write + causal/padding-masked softmax(QK^T)V for the prompt.
// ---------------------------------------------------------------------------------------------
struct ContextAttnParams
{
    int32_t batch = 0, seq = 0, num_heads = 0, head_size = 0;
    int32_t rotary_dim = 0, neox = 1;
    float inv_sqrt_dh = 1.f;
    int32_t kv_dtype = DT_HALF, max_seq_len = 0; // DT_HALF, DT_INT8 or DT_FP8 (the one-byte types with kv_scale_orig_quant)
    void* qkv = nullptr;      // fp16 [B, S, 3*H*Dh]; q,k rewritten in place with RoPE applied (reference :1401-1403)
    void* kv_cache = nullptr; // [B, 2, H, Smax, Dh]
    const int32_t* input_lengths = nullptr; // [B]
    const float* kv_scale_orig_quant = nullptr;
    const float* rope_table = nullptr;
    int32_t rope_table_len = 0;
    void* out = nullptr; // fp16 [B, S, H*Dh]; rows >= input_len[b] are zero
    // optional static quantiser behind the attention (SmoothQuant's O-projection input, K/quantization.cu): when set the result
    // goes to out_q8 = sat(rni(float(fp16(ctx)) * out_q_scale[0])), int8 [B, S, H*Dh], and the MFMA kernel does not write `out`
    // at all (the other kernels write `out` and a quantiser pass follows - same values either way)
    int8_t* out_q8 = nullptr;
    const float* out_q_scale = nullptr;
    void* workspace = nullptr; // context_attention_workspace_size() bytes; NULL -> the (slow) wave-per-query kernel
    // packed inputs (remove_input_padding, P/gptAttentionPlugin/gptAttentionPlugin.cpp:344-356): qkv / out hold only the real
    // tokens, [sum(len), ...]; token s of sequence b is row cu_seqlens[b] + s.  `seq` stays the longest sequence (grid bound).
    const int32_t* cu_seqlens = nullptr; // device int32 [B + 1], exclusive prefix sum of input_lengths
    // beam search: prompt b fills the cache rows of sequence b * cache_seq_stride (hypothesis 0 of its beam group; the
    // siblings reach those rows through the cache indirection, so the prompt's K/V is stored once)
    int32_t cache_seq_stride = 1;
    // paged KV cache: see MmhaParams (kv_cache unused when set)
    const int64_t* block_pointers = nullptr;
    int32_t tokens_per_block = 0, max_blocks_per_seq = 0;
    // grouped-query attention, as MmhaParams::num_kv_heads (0 = num_heads): qkv rows are [q: H*Dh | k: Hkv*Dh | v: Hkv*Dh], RoPE
    // on k, the cache quantisation and the cache write run once per K/V head; `out` stays [B, S, H*Dh]
    int32_t num_kv_heads = 0;
    // the attention kernel of the launch, a ContextAttnKernel: 0 = the launcher's rule (context_attention_plan); a forced kind runs
    // exactly that instance, and one the launcher cannot run is an error with nothing enqueued, never a substitute
    int32_t kernel = 0;
};
size_t context_attention_workspace_size(int batch, int num_heads, int head_size, int seq);
// The launch plan of the context attention - which of the four attention kernels runs, and its geometry - stated once:
//   wg128 = ceil(seq / 128) * num_heads * batch, the workgroups a launch of 128-query workgroups would have;
//   the MFMA kernels serve head sizes 64 / 128 with a workspace (the V^T image), seq >= 64 and a positive score scale; everything
//   else is the wave-per-query kernel (4 queries per workgroup, no dynamic LDS);
//   among the MFMA kernels: PAIRED (two 64-query blocks per workgroup, three operand stages) while wg128 <= cus <= 4 * wg128,
//   else NARROW (64 queries) while wg128 < 256, else WIDE (128 queries); both of the latter with two stages.
// forced_kernel != 0: that kind or the empty plan (kernel 0, `refused` says why) - an MFMA kind outside what the MFMA kernels
// serve, or an unknown value.  cus 0 = the CU count of the current device (asked only where the rule needs it).
enum ContextAttnKernel
{
    CTX_ATTN_RULE = 0,
    CTX_ATTN_WAVE = 1,
    CTX_ATTN_MFMA_NARROW = 2,
    CTX_ATTN_MFMA_WIDE = 3,
    CTX_ATTN_MFMA_PAIRED = 4
};
struct ContextAttnPlan
{
    int32_t kernel = 0;                 // the kind that runs; 0 = refused
    int32_t query_block = 0;            // queries per workgroup: 4, 64 or 128 (PAIRED: two blocks of 64)
    int32_t stages = 0;                 // operand stages in LDS: 2 or 3 (WAVE: 0)
    uint32_t grid[3] = {0, 0, 0};       // workgroups
    int32_t threads = 0;
    size_t lds_bytes = 0;               // dynamic LDS
    const char* refused = nullptr;
};
ContextAttnPlan context_attention_plan(int32_t head_size, int32_t seq, int32_t batch, int32_t num_heads, bool has_workspace,
    bool score_scale_positive, int32_t cus = 0, int32_t forced_kernel = 0);
// cu[0] = 0, cu[b + 1] = cu[b] + lens[b]  (device, one tiny launch; packed-input bookkeeping)
int launch_exclusive_scan_i32(int32_t* cu, const int32_t* lens, int32_t n, hipStream_t stream);
// out[b, :] = hidden[rows[b], :]  (fp16 rows; the packed-input flavour of gather_last_token)
int launch_gather_rows(void* out, const void* hidden, const int32_t* rows, int32_t batch, int32_t hidden_size, hipStream_t stream);
int launch_context_attention(const ContextAttnParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Append attention (kernels/append_attn.hip): n new tokens per sequence onto a live cache - RoPE + cache
// write of the n rows, then their attention over the unmasked slots < sequence_length[b] (read as the decode kernel reads them)
// and, causally, over the appended rows themselves (un-quantised, from the QKV buffer).  The parallel form of n decode steps.
// ---------------------------------------------------------------------------------------------
enum AppendAttnKernel
{
    APPEND_ATTN_RULE = 0, // the MFMA kernel where it serves (head size 64 / 128, n >= 16), else one wave per query
    APPEND_ATTN_WAVE = 1, // one wave per query: every n, head sizes 32 / 64 / 128 / 256
    APPEND_ATTN_MFMA = 2  // 64 queries per workgroup, online soft-max over 64-key blocks
};
struct AppendAttnParams
{
    // n: tokens appended per sequence; with n_per_seq their upper bound - and the row stride of qkv and out either way
    int32_t batch = 0, n = 0;
    // [B] device or null (= n for every sequence): sequence b appends n_per_seq[b] tokens, clamped into [0, n] on the device; rows
    // behind them are padding - no RoPE, no cache store, never read, `out` rows zero
    const int32_t* n_per_seq = nullptr;
    // with n_per_seq, in place of max_past: >= every sequence_length[b] + n_per_seq[b], promised by the caller; max_end >
    // max_seq_len is refused with nothing enqueued (max_past + n would refuse a long past with a short turn beside a long turn)
    int32_t max_end = 0;
    int32_t num_heads = 0, num_kv_heads = 0, head_size = 0; // num_kv_heads as MmhaParams (0 = num_heads)
    int32_t rotary_dim = 0, neox = 1;
    float inv_sqrt_dh = 1.f;
    int32_t kv_dtype = DT_HALF; // DT_HALF, DT_INT8 or DT_FP8 (the one-byte types with both scales)
    int32_t max_seq_len = 0;    // cache capacity Smax
    int32_t max_input_len = 0;  // padded prompt length: rotary position of slot t = t - (max_input_len - input_lengths[b])
    // >= every sequence_length[b], promised by the caller: max_past + n > max_seq_len is refused with nothing enqueued.  On the
    // device every cache store is still guarded by slot < Smax and every load index clamped
    int32_t max_past = 0;
    void* qkv = nullptr;      // fp16 [B, n, (H + 2 Hkv) * Dh]; q and k rewritten in place with RoPE applied
    void* kv_cache = nullptr; // [B, 2, Hkv, Smax, Dh]
    const int32_t* sequence_length = nullptr; // [B] device: the past lengths p_b (may differ per sequence); not written
    const int32_t* input_lengths = nullptr;   // [B] device
    const int32_t* masked_tokens = nullptr;   // [B, Smax] device or null
    const float* kv_scale_orig_quant = nullptr;
    const float* kv_scale_quant_orig = nullptr;
    const float* rope_table = nullptr; // f32 [rope_table_len, rotary_dim / 2, 2]
    int32_t rope_table_len = 0;
    void* out = nullptr; // fp16 [B, n, H * Dh]
    int32_t kernel = 0;  // an AppendAttnKernel; a forced kind runs exactly that kernel or the launch is refused, never a substitute
    // paged KV cache, as MmhaParams (the fields stand last: the linear instances read what they read before, where it was): a table
    // int64 [batch, 2, max_blocks_per_seq] of pointers to blocks [Hkv, tokens_per_block, Dh], slot t = row t % tokens_per_block of
    // block t / tokens_per_block, tokens_per_block a power of two; kv_cache is then the pool the blocks live in (where the load of
    // a slot whose entry is 0 is pointed; such a slot is never stored to and never enters a product).  Same kernels as compile-time
    // paged instances, same arithmetic in the same order: every result is the linear launch's on the same logical cache, bit for bit
    const int64_t* block_pointers = nullptr;
    int32_t tokens_per_block = 0, max_blocks_per_seq = 0;
};
// the attention kernel a launch runs (APPEND_ATTN_WAVE / _MFMA), 0 = refused (*refused says why)
int append_attention_kernel(int32_t head_size, int32_t n, int32_t forced_kernel, const char** refused = nullptr);
int launch_append_attention(const AppendAttnParams& p, hipStream_t stream);
// sequence_length[b] += n; finished[b] = 0 (finished may be null): one workgroup, a launch of its own
int launch_append_advance(int32_t* sequence_length, int32_t* finished, int32_t batch, int32_t n, hipStream_t stream);
// sequence_length[b] += n_per_seq[b] clamped into [0, n] (n_per_seq [B] device)
int launch_append_advance_ragged(int32_t* sequence_length, int32_t* finished, const int32_t* n_per_seq, int32_t batch, int32_t n,
    hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// MFMA GEMMs for M > 8 (prefill): C[m,n] = sum_k A[m,k] * B[n,k].
// ---------------------------------------------------------------------------------------------
struct GemmParams
{
    int32_t wtype = W_FP16; // same weight layouts as GemvParams
    int32_t out_dtype = DT_HALF;
    int32_t M = 0, N = 0, K = 0;
    const void* a = nullptr; // fp16 [M, lda] or s8 [M, lda]
    int64_t lda = 0;
    const void* w = nullptr;
    int64_t ldw = 0; // bytes
    const void* scale_col = nullptr;
    const float* scale_row = nullptr;
    int32_t per_channel = 0, per_token = 0;
    void* c = nullptr;
    int64_t ldc = 0;
    const void* residual = nullptr; // optional fp16 [M, ldc]: C = fp16(fp16(gemm) + residual) (may alias c); fp16 output only
    // optional fp16 [M, ldc] (fp16 / weight-only weights, fp16 output, not together with residual): C = fp16(fp16(silu(gate)) * fp16(gemm)) -
    // the SwiGLU pass of the prefill MLP folded into the second projection (may alias c)
    const void* silu_gate = nullptr;
    // SmoothQuant dual GEMM (prefill MLP, static activation scales): w2 / scale_col2 = the second weight matrix [N, ldw] and
    // its per-channel scales; c = int8 [M, ldc] = sat(rni(fp16(silu16(A W^T) * fp16(A W2^T)) * swiglu_qscale[0])) with the
    // fp16 rounding points of the un-fused path (two fp16 GEMM outputs, SwiGLU in fp16, static quantiser); launch_gemm_swiglu
    const void* w2 = nullptr;
    const void* scale_col2 = nullptr;
    const float* scale_row2 = nullptr; // static dequantisation scale of the second GEMM [1] (null: scale_row)
    const float* swiglu_qscale = nullptr;
    // microbench hook (tllm_gemm_set_clock_probe), set by the launchers only: 2 x uint64 per workgroup {shader cycles, 100 MHz ticks}
    void* clock_probe = nullptr;
    // split-K-2 forms of gemm_sqp.hip (r06), set by the launcher only: per tile two slabs of AH x BN accumulators + two flag words
    void* ksplit_ws = nullptr;
};
int launch_gemm(const GemmParams& p, hipStream_t stream);
// fc and gate projections of the SmoothQuant MLP in one kernel with SwiGLU + static int8 quantisation in its epilogue
// (gemm_sqp.hip); returns 1 when the problem is not served (caller runs the two GEMMs + launch_swiglu_quant instead)
int launch_gemm_swiglu(const GemmParams& p, hipStream_t stream);
// On-device tactic selection for the prefill GEMMs (gemm_tactics.hip; reference: int8_gemm_template.h:372-457 profileGemm +
// smoothQuantGemmPlugin.cpp:253-282 mMNKProfileMap).  lookup: kernel id for the shape, 0 = nothing profiled (static rule).
int gemm_tactic_lookup(int wtype, int M, int N, int K);
bool gemm_tactic_known(int wtype, int M, int N, int K);
int gemm_profile(int wtype, int M, int N, int K, int* best_cfg, float* best_us, hipStream_t stream);
void gemm_tactics_clear();
int gemm_tactics_import(const char* text); // entries taken, -1 on a parse error
std::string gemm_tactics_export();       // "wtype:M:N:K:cfg:us;..."

// One-shot peer-to-peer sum all-reduce of an fp16 vector, in place (kernels/p2p_allreduce.hip; plugins/p2p.cpp owns the
// inboxes).  peer[r]: base of rank r's region as mapped in THIS process: [2 gens][world][slot_bytes] data, then flags.
struct P2PParams
{
    void* peer[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t world = 0, rank = 0;
    size_t slot_bytes = 0, flag_offset = 0;
    void* x = nullptr; // fp16, n16 * 8 elements, 16-byte aligned (sum: in place; gather: this rank's contribution)
    void* gather_out = nullptr; // non-null: all-gather instead of sum, out = [world][n16 * 16 bytes]
    int32_t n16 = 0;
    uint32_t* epoch = nullptr; // device counter, advanced by the kernel
    uint32_t* error = nullptr; // device flag: non-zero after a spin timed out (bit 31: a PEER reported the time-out)
    int32_t max_spins = 4000000;
    // optional fused tail of the sum (never with gather_out):
    //   residual != null           : the sum starts from residual[v]                       (hidden = residual + all_reduce(...))
    //   x_out    != null           : the fp16 result goes there instead of back into x     (may alias residual)
    //   norm_out != null           : + RMSNorm over rows of `cols` elements: norm_out = fp16(fp16(x_out * inv) * gamma), or its
    //                                int8 quantisation (quant 1: static scale quant_scale[0]; 2: per token, scales to dyn_scale_out)
    const void* residual = nullptr;
    void* x_out = nullptr;
    void* norm_out = nullptr;
    const void* gamma = nullptr;
    float eps = 1e-6f;
    int32_t rows = 0, cols = 0, quant = 0;
    const float* quant_scale = nullptr;
    float* dyn_scale_out = nullptr;
};
constexpr size_t P2P_POISON_OFFSET = 2048; // byte offset behind flag_offset of the "a peer gave up" word in every region
int launch_p2p_allreduce(const P2PParams& p, hipStream_t stream);

// Greedy sampler: argmax over fp32 logits [B, V] -> ids; ties -> lowest index.
int launch_argmax(int32_t* out_ids, const float* logits, int32_t batch, int32_t vocab, hipStream_t stream);

// One greedy sampling step with the bookkeeping of GenerationSession.decode kept on the device
// (PY/runtime/generation.py:943-983: DynamicDecodeOp top-k=1 + sequence-length update + stop criteria):
//   id = argmax_v logits[b, v]   (logits may be the all-gather of `nparts` vocabulary shards [nparts, B, vocab_part])
//   if advance: seq_len[b] += 1 ;  finished sequences keep emitting end_id ;  out_ids[b, seq_len[b]] = id ;
//   cur_ids[b] = id ;  finished[b] |= (id == end_id)
struct GreedyParams
{
    const float* logits = nullptr;
    int32_t batch = 0, vocab_part = 0, nparts = 1, vocab = 0;
    int32_t* cur_ids = nullptr;
    int32_t* out_ids = nullptr;
    int32_t out_stride = 0;
    int32_t* seq_len = nullptr;
    int32_t* finished = nullptr;
    int32_t end_id = -1, advance = 0;
    // optional: prepare the RoPE cos/sin row of the NEXT generation step, position = seq_len[b] - (max_input_len -
    // input_lengths[b])  (MM/...Template.h:1425-1426), so that the attention kernel does not chase
    // length -> position -> table
    float* rope_row_out = nullptr;     // f32 [B, rope_half, 2]
    int32_t* rope_pos_out = nullptr;   // optional int32 [B]: the position that row was taken at (parity tests read it back)
    const float* rope_table = nullptr; // f32 [rope_table_len, rope_half, 2]
    int32_t rope_half = 0, rope_table_len = 0;
    const int32_t* input_lengths = nullptr;
    int32_t max_input_len = 0;
    // optional: gather the chosen token's embedding row into the next step's input (fp16 [B, hidden]) - one launch and one
    // dependent round trip less per generation step than a separate embedding kernel
    const void* emb_table = nullptr; // fp16 [vocab, hidden]
    void* x_out = nullptr;
    int32_t hidden = 0;
    uint32_t* step_epoch = nullptr; // optional device word, += 1 per call (tags of the in-launch hand-offs of the next step)
    // optional (batch 1, nparts 1 only - anything else is refused): the kArgmaxPairs pairs the lm_head launch that produced
    // `logits` left (GemvParams::argmax_part).  The kernel reduces them and does not read the logits; the token is the same.
    const void* argmax_part = nullptr;
};
int launch_greedy_step(const GreedyParams& p, hipStream_t stream);

// One top-k / top-p sampling step with temperature, penalties and minimum length (kernels/sampling.hip), the counterpart of
// the reference's dynamic decoder with beam_width 1 (layers/baseSamplingLayer.cpp:171-248, layers/topKSamplingLayer.cu,
// K/samplingTopKKernels.cu, K/samplingTopPKernels.cu, K/samplingPenaltyKernels.cu).  The rule, for row b producing generated
// token number g (1-based; g = 1 is the token the prompt pass yields) from the raw fp32 logits x[v], v < vocab:
//   1. temperature: y = x * (1 / (temperature + 1e-6f)) in fp32; skipped when temperature == 1.
//   2. penalty, applied ONCE to every distinct id that occurs in the row's real prompt tokens [0, input_lengths[b]) or in its
//      g - 1 generated tokens so far (padding slots [input_lengths[b], max_input_len) are skipped): repetition
//      (y < 0 ? y * r : y / r, when repetition_penalty != 1) or else presence (y - r, when presence_penalty != 0).
//   3. minimum length: y[end_id] = -FLT_MAX while g < min_length.  (NaN logits count as -inf, -0 as +0.)
//   4. candidates: the ids ordered by (y descending, id ascending).  k' = top_k clipped to [1, 1024], or vocab when top_k == 0;
//      p' = top_p clipped to [0, 1]; top_k == 0 && top_p == 0 -> k' = 1; top_k > 0 && top_p == 0 -> p' = 1.
//   5. draw: w_i = exp(y_i - y_max) (0 for y_i = -inf, 1 for y_i = y_max) over the first k' ids of that order, S = sum w_i,
//      target = u * p' * S; the token is the first i whose inclusive prefix sum reaches target, else the last of the k'.
//      A row whose y are all -inf yields the first id of the order.
//   6. the bookkeeping of launch_greedy_step (finished rows keep emitting end_id, finished |= id == end_id, out_ids, cur_ids,
//      seq_len, next RoPE row and position, step_epoch, the next step's embedding row).
// u in (0, 1] is a function of (random_seed, b, g) and nothing else: Philox4x32-10 (Salmon et al., SC'11) with key = (low, high
// half of random_seed), counter = (b, g, 0, 0), u = ((word0 >> 8) + 1) * 2^-24.  No state is advanced by the host or by an
// earlier launch, so a replayed graph needs no new arguments; the reference's cuRAND sequence is NOT reproduced.
// The weights are accumulated as integers (w * 2^40, truncated): integer sums do not depend on the order of the LDS atomics,
// so the same logits, history and (seed, b, g) give the same id in every launch, process and tensor-parallel rank.  What is
// rounded away are ids of probability below 1e-12.  The logits are not modified in memory.
struct SamplingParams
{
    GreedyParams g;             // logits, shapes and bookkeeping, exactly as the greedy step; g.out_ids may be NULL (no record)
    const int32_t* history = nullptr; // int32 [batch, history_stride]: prompt slots [0, max_input_len), generated tokens behind;
    int32_t history_stride = 0;       // the session passes out_ids.  May be NULL when no penalty is set.
    int32_t g_base = 0;         // g = seq_len[b] + advance - g_base + 1 (the session: max_input_len)
    int32_t top_k = 1;
    float top_p = 0.f, temperature = 1.f, repetition_penalty = 1.f, presence_penalty = 0.f;
    int32_t min_length = 1;
    uint64_t random_seed = 0;
    float* u_out = nullptr;     // optional f32 [batch]: the uniform variate of each row (tests)
};
int launch_sampling_step(const SamplingParams& p, hipStream_t stream);
// true when the configuration is the plain arg-max the greedy step computes (top_k == 1, no penalty, min_length <= 1)
bool sampling_is_greedy(const SamplingParams& p);

// Per-token log-probabilities from fp32 logits rows without the rows leaving the device (kernels/token_logprob.hip; the
// numpy float64 restatement is tensorrt_llm/runtime/scoring_ref.py).  Row r with target t = targets[r], over the ids v < vocab:
//   lse = log sum_v exp(x[v]),  log_prob = x[t] - lse,  top1 = arg-max_v x[v] (ties -> lowest id, as launch_argmax).
// The vocabulary may come in parts (tensor-parallel shards): the partial launch leaves one record of 8 words per (part, row),
//   m = max of the part's valid ids (-inf if it has none),  s = sum exp(x - m) in fp32 (0 if m = -inf),
//   xt = x[t] if t lies in the part else -inf,  top_val, top_id (global id; INT_MAX if the part has no valid id),  3 words of 0,
// and the merge launch folds a row's records in part order: M = max m_p, S = sum s_p exp(m_p - M), lse = M + log S.  With one
// part the merge is the identity on (m, s, xt, top).  Columns whose global id is >= vocab are padding and are never read.
// Special values:
//   * t outside [0, vocab) (-1 marks "no target"): log_prob = 0, nothing is read for it;
//   * x[t] = -inf: log_prob = -inf; this includes the row of only -inf, whose lse is -inf and whose top1 is 0;
//   * NaN or +inf among the valid ids: undefined.
// The logits are never written.  Any ld and any 4-byte row alignment is served.  For a given launch geometry the result is
// bit-reproducible: no atomics, a fixed reduction order.
struct TokenLogprobParams
{
    const float* logits = nullptr; // part q (of this launch), row r, column i: logits[q * part_stride + r * ld + i]
    int64_t part_stride = 0, ld = 0; // elements
    int32_t rows = 0;
    int32_t nparts = 1;     // parts in this launch
    int32_t first_part = 0; // column i of launch part q has the global id (first_part + q) * vocab_part + i
    int32_t vocab_part = 0, vocab = 0;
    const int32_t* targets = nullptr; // int32 [rows]
    float* partials = nullptr;        // f32 [nparts, rows, 8]
};
int launch_token_logprob_partial(const TokenLogprobParams& p, hipStream_t stream);
// partials f32 [nparts, rows, 8] -> log_probs f32 [rows]; lse f32 [rows] and top1_ids int32 [rows] optional
int launch_token_logprob_merge(const float* partials, int32_t nparts, int32_t rows, int32_t vocab, const int32_t* targets,
    float* log_probs, float* lse, int32_t* top1_ids, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Speculative greedy decoding (kernels/spec_decode.hip; the numpy restatement is
// tensorrt_llm/runtime/spec_ref.py).  A verify pass runs n ids per sequence - t[0] the pending token, t[1..] drafts - onto the
// live cache in one append pass and scores all n rows; a[i] is the arg-max id of row i, the distribution behind t[0..i].
//
// The accept step takes the sampler's place behind that pass.  One workgroup per sequence b; p = seq_len[b],
// lim = limit ? limit[b] : INT32_MAX (the largest sequence length the call may leave):
//   frozen (finished[b] != 0 or p >= lim): accepted[b] = -1 and no state of the sequence is written (its input row in x_out, which
//     the pass has used as an activation buffer, is put back from cur_ids[b]);
//   otherwise  m = 0; while (m + 1 < n && p + m + 1 < lim && a[m] != end_id && t[m + 1] == a[m]) ++m;  bonus = a[m];
//     out_ids[b][p + i] = t[i] for i <= m, out_ids[b][p + m + 1] = bonus (slots above are not written), seq_len[b] = p + m + 1,
//     cur_ids[b] = bonus, finished[b] |= bonus == end_id, accepted[b] = m; the RoPE row (and rope_pos_out) of position
//     p + m + 1 - (max_input_len - input_lengths[b]), clamped into the table; the embedding row of bonus into x_out; row m of the
//     sequence's logits rows into row b of logits_out;
//   once per launch: step_epoch += 1, as every sampler launch does.
// The tokens are those plain greedy decoding defines whatever the drafts were: a draft is kept only where it is the arg-max.
// Fields of g as launch_greedy_step reads them, except: g.logits = the verify rows f32 [batch * n, vocab_part] (one part, read
// only for the row copy), g.advance and g.argmax_part are ignored.  Guards: cache slot < out_stride, id < vocab (else a zero row).
// ---------------------------------------------------------------------------------------------
constexpr int kVerifyMaxTokens = 32; // ids per sequence of one verify pass (TLLM_VERIFY_MAX_TOKENS)
constexpr int kLookupMaxNgram = 8;   // longest suffix the prompt lookup matches
struct SpecAcceptParams
{
    GreedyParams g;
    int32_t n = 0;                 // ids per sequence, 1 .. kVerifyMaxTokens
    const int32_t* ids = nullptr;  // int32 [batch, n]: t
    const int32_t* top1 = nullptr; // int32 [batch, n]: a - the arg-maxes, or the draws of launch_spec_sample_rows (a sampled pass)
    const int32_t* limit = nullptr; // int32 [batch] or null
    int32_t* accepted = nullptr;   // int32 [batch] or null
    float* logits_out = nullptr;   // f32 [batch, vocab_part] or null
};
int launch_spec_accept(const SpecAcceptParams& p, hipStream_t stream);

// Prompt lookup: drafts from the sequence's own token record.  One workgroup per sequence b.  The logical sequence is
// out_ids[b][0 .. input_lengths[b]) followed by out_ids[b][max_input_len .. seq_len[b]] - the padding slots between are not part
// of it - and its last element is the pending token.  With k = n - 1 draft slots: for g = max_ngram down to 1 the last g tokens
// are the suffix; among the starts s with s + g < len whose g tokens equal it the most recent wins, at the first g that has one.
// The draft is the up to k tokens behind the match that exist inside the logical sequence; draft_len[b] is their number, 0
// without a match and for a frozen sequence (finished, or seq_len >= limit).  ids[b] = [pending, draft..., pending...]: any valid
// id serves behind the draft, the accept rule rejects or rightly accepts whatever it is given.  state_out (optional, int32
// [batch, 4]) = {seq_len, finished, draft_len, frozen}: what the host loop reads back in one copy.
struct PromptLookupParams
{
    int32_t batch = 0, n = 0, max_ngram = 0; // n 1 .. kVerifyMaxTokens, max_ngram 1 .. kLookupMaxNgram
    const int32_t* out_ids = nullptr;        // int32 [batch, out_stride]
    int32_t out_stride = 0;
    const int32_t* seq_len = nullptr;        // int32 [batch]
    const int32_t* input_lengths = nullptr;  // int32 [batch] or null (= max_input_len)
    int32_t max_input_len = 0;
    const int32_t* finished = nullptr;       // int32 [batch] or null
    const int32_t* limit = nullptr;          // int32 [batch] or null
    int32_t vocab = 0;                       // an id outside [0, vocab) in the record is passed on as 0
    int32_t* ids = nullptr;                  // int32 [batch, n]
    int32_t* draft_len = nullptr;            // int32 [batch] or null
    int32_t* state_out = nullptr;            // int32 [batch, 4] or null
};
int launch_prompt_lookup(const PromptLookupParams& p, hipStream_t stream);
// targets[b][i] = ids[b][i + 1], -1 at i = n - 1: the next-token targets of a verify pass's n rows (token_logprob)
int launch_spec_targets(int32_t* targets, const int32_t* ids, int32_t batch, int32_t n, hipStream_t stream);

// Speculative sampling by exact match (kernels/sampling.hip, beside the step kernel whose row draw it shares; DESIGN.md section
// 7e; the numpy restatement is spec_ref.sample_rows): the sampler on ALL n rows of a verify pass, so that the accept step above
// can compare the drafts with the DRAWS plain sampled decoding would have made instead of with the arg-maxes.  One workgroup per
// (sequence b, row i < n); p = seq_len[b], t = ids[b], S = g_base = max_input_len.  Row (b, i) is row b * n + i of the logits:
//   draws[b][i] = the id steps 1 - 5 of SamplingParams select from that row for generated-token number g = p + i + 2 - S - the
//     token that would land in slot p + i + 1 - with u = Philox(random_seed; b, g), the step's own variate for that token;
//   the row's history for the penalty: the real prompt tokens record[b][0 .. input_lengths[b]), the record [S .. p), then
//     t[0..i] in the places of slots p .. p + i - from ids, not from the record: t[0] stands in the pending token's place and the
//     drafts are not in the record yet.  Padding slots [input_lengths[b], S) are skipped, an id outside [0, vocab) is skipped;
//   min_length masks end_id per row by the row's own g (it may hold for the first rows of a pass and not for the later ones);
//   frozen (finished[b] != 0, p >= limit[b], or p < 0): the rows are not drawn, draws[b][i] = end_id (the accept step does not
//     read them); u_out is written all the same.
// A draw is a pure function of (logits row, history, seed, b, g): the same integer weight sums as the step, so draws[b][i] is
// bit-identical to what launch_sampling_step selects for the same row, history and g, whatever n and whatever the other rows
// hold.  The logits are never written.  Both forms of the step kernel are kept: y staged in LDS beside the history bitmap when
// it fits, recomputed otherwise.
// Fields read of s: the configuration (top_k .. random_seed), g_base, history = the token record int32 [batch, history_stride]
// (NULL without a penalty), u_out (optional f32 [batch, n]); of s.g: logits f32 [batch * n, vocab_part] (nparts 1: anything else
// is refused), batch, vocab_part, vocab, seq_len, finished (or NULL), end_id, input_lengths (or NULL = max_input_len),
// max_input_len.  Nothing else of s.g is read and none of the step words is written.
struct SpecSampleParams
{
    SamplingParams s;
    int32_t n = 0;                  // rows per sequence, 1 .. kVerifyMaxTokens
    const int32_t* ids = nullptr;   // int32 [batch, n]: t
    const int32_t* limit = nullptr; // int32 [batch] or null
    int32_t* draws = nullptr;       // int32 [batch, n]
};
int launch_spec_sample_rows(const SpecSampleParams& p, hipStream_t stream);

// teacher forcing for parity tests: overwrite the sampler's last choice (output slot seq_len[b], step input id, next input row)
int launch_force_token(const int32_t* ids_dev, int32_t* cur_ids, int32_t* out_ids, int32_t out_stride, const int32_t* seq_len,
    const void* emb, void* x, int32_t batch, int32_t hidden, int32_t vocab, hipStream_t stream);

// One beam-search step on the device (K/onlineSoftmaxBeamsearchKernels.cu, layers/onlineBeamSearchLayer.cu; called at
// PY/runtime/generation.py:949-961 with beam_width > 1).  Per batch entry, over its `beam` hypotheses:
//   score(k, v) = cum_log_probs[k] + log_softmax(logits[k])[v]      (a finished hypothesis only continues with end_id, score kept)
//   the `beam` best (k, v) in score order (ties: lowest k * vocab + v) become the new hypotheses j: token v, parent k;
//   cache_indirection[j, s] <- cache_indirection[parent, s] for every used slot s, and the slot the consumed token's K/V
//   went to <- parent;  out_ids / parent_ids[j, slot] record the step for the final back-track (gather_tree).
// Bookkeeping (sequence length, current ids, next RoPE row) as launch_greedy_step.
struct BeamParams
{
    const float* logits = nullptr; // [nparts, batch * beam, vocab_part]  ([nparts, batch, vocab_part] if logits_per_batch)
    int32_t logits_per_batch = 0;  // first step after the prompt: one logits row per batch entry, shared by its hypotheses
    int32_t batch = 0, beam = 1, vocab_part = 0, nparts = 1, vocab = 0;
    float* cum_log_probs = nullptr; // [batch * beam]
    int32_t* cur_ids = nullptr;
    int32_t* out_ids = nullptr;    // [batch * beam, out_stride]
    int32_t* parent_ids = nullptr; // [batch * beam, out_stride]
    int32_t out_stride = 0;
    int32_t* seq_len = nullptr;
    int32_t* finished = nullptr;
    int32_t end_id = -1, advance = 0;
    int32_t* cache_indirection = nullptr; // [batch * beam, out_stride]
    float* rope_row_out = nullptr;
    int32_t* rope_pos_out = nullptr; // as GreedyParams
    const float* rope_table = nullptr;
    int32_t rope_half = 0, rope_table_len = 0;
    const int32_t* input_lengths = nullptr;
    int32_t max_input_len = 0;
};
int launch_beam_step(const BeamParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// LoRA adapters per row (kernels/lora.hip; the numpy float64 restatement is
// tensorrt_llm/runtime/lora_ref.py).  A projection site is the fused QKV, attention.dense, fc|gate or mlp.proj.  For row m with
// adapter a = row_adapter[m] in [0, num_adapters), rank r and scale s_a (alpha / r, or alpha / sqrt(r) under rsLoRA):
//   shrink  t[m][g r + j] = sum_k f32(A_a[g r + j][k]) f32(xh[m][k]), accumulated and kept in fp32.  xh is the fp16 row the base
//           projection consumes - x itself (PRO_NONE) or RMSNorm(x) gamma with the rounding points of the GEMV's PRO_RMSNORM
//           (gemv_impl.h: inv = 1 / sqrt(ss / K + eps) in fp32, n = f16(x inv), xh = f16(n gamma)); g is the segment of the site
//           (q | k | v of the fused QKV, fc | gate of the MLP's first projections, one segment otherwise);
//   expand  y[m][n] <- f16(f32(y[m][n]) + s_a sum_j f32(B_a[n][j]) t[m][seg(n) r + j]), in place on the fp16 buffer the base
//           projection left its result in: qkv, g, u (before SwiGLU), x (behind the residual add of O and of down).  Segments may
//           be unequal (grouped heads) and may live in different buffers (g and u).
// A row whose adapter is outside [0, num_adapters) (-1 = none) is not read by shrink, its t row is neither written nor read, and
// expand leaves its y bits alone.  Adapters of lower rank are zero-padded to r by the caller, so one r serves every launch.
// No floating-point atomics, a fixed reduction order: the result is a function of the inputs, launch after launch, eager or
// replayed from a graph.  Nothing step-dependent is a launch argument: the adapters' A / B base pointers and scales come from a
// device table, the row -> adapter map from a device array.
// Operands: K % 8 == 0; r one of 8, 16, 32, 64; x, A, B rows 16-byte aligned (ldx % 8 == 0); every index is predicated.
// Geometry: shrink - one workgroup per (A row, adapter, tile of 8 rows of x), the 256 threads split K, each A row is read once
// per workgroup and serves the tile's rows of that adapter (four A rows per workgroup beyond 8 rows); expand - r / 8 lanes per B
// row with 16-byte loads, 2048 / r output columns per workgroup, a tile of 8 (32 beyond 8 rows) rows of t staged in LDS.  A
// workgroup whose adapter no row of its tile uses returns before its first load.
// ---------------------------------------------------------------------------------------------
struct LoraAdapterRec // one adapter slot of one site, 24 bytes in device memory
{
    const void* a = nullptr; // fp16 [nseg * r, K]
    const void* b = nullptr; // fp16 [sum of the segments' N, r]
    float scale = 0.f;
    int32_t reserved = 0;
};
constexpr int kLoraMaxAdapters = 8;
constexpr int kLoraMaxSegments = 3;
struct LoraShrinkParams
{
    int32_t M = 0, K = 0;
    int32_t R = 0;                 // rows of A = nseg * r
    int32_t pro = PRO_NONE;        // PRO_NONE | PRO_RMSNORM
    const void* x = nullptr;       // fp16 [M, ldx]
    int64_t ldx = 0;               // elements
    const void* gamma = nullptr;   // fp16 [K] (PRO_RMSNORM)
    float eps = 1e-6f;
    const int32_t* row_adapter = nullptr; // device int32 [M]
    const LoraAdapterRec* table = nullptr; // device [num_adapters]
    int32_t num_adapters = 0;      // 1 .. kLoraMaxAdapters
    float* t = nullptr;            // f32 [M, R]
};
int launch_lora_shrink(const LoraShrinkParams& p, hipStream_t stream);
struct LoraExpandParams
{
    int32_t M = 0, r = 0, nseg = 1; // nseg 1 .. kLoraMaxSegments
    int32_t seg_n[kLoraMaxSegments] = {0, 0, 0};   // output columns of every segment; B row of column n of segment g: sum(seg_n[< g]) + n
    void* seg_y[kLoraMaxSegments] = {nullptr, nullptr, nullptr}; // fp16: column 0 of the segment in row 0
    int64_t seg_ldy[kLoraMaxSegments] = {0, 0, 0}; // elements
    const float* t = nullptr;      // f32 [M, nseg * r]
    const int32_t* row_adapter = nullptr;
    const LoraAdapterRec* table = nullptr;
    int32_t num_adapters = 0;
};
int launch_lora_expand(const LoraExpandParams& p, hipStream_t stream);
// rows[m] = sel[sequence of row m]: rows_per_seq > 0 - sequence m / rows_per_seq (padded prompt rows, appended rows); else the
// packed layout, sequence b owns rows [cu_seqlens[b], cu_seqlens[b + 1]).  A row no sequence owns gets -1.
int launch_lora_row_adapter(int32_t* rows, const int32_t* sel, int32_t batch, int32_t M, int32_t rows_per_seq,
    const int32_t* cu_seqlens, hipStream_t stream);

// deterministic pseudo-random fill (fp16 ~U(-scale, scale) or int8 ~U[-127,127]) for synthetic KV caches
int launch_fill_random(void* dst, int32_t dtype, int64_t n, uint32_t seed, float scale, hipStream_t stream);
// int32 fill
int launch_fill_i32(int32_t* dst, int32_t value, int64_t n, hipStream_t stream);

} // namespace kernels
} // namespace tllm
