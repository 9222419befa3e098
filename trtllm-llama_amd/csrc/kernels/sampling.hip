// Top-k / top-p sampling step with temperature, repetition / presence penalty and minimum length (SamplingParams in
// kernels.h states the rule).  One workgroup of 1024 threads per row, plain launch, no waits on other workgroups.
// Two kernels share the row draw (draw_row): sampling_step_kernel, one row per sequence with the step's bookkeeping, and
// spec_sample_rows_kernel, all n rows per sequence of a verify pass and nothing else (SpecSampleParams in kernels.h).
//
// How the row is processed:
//   * the row's history (real prompt tokens + generated tokens) becomes a membership bitmap in LDS (vocab / 8 bytes), the
//     penalties are applied on the fly from it; the logits in memory are never written;
//   * the transformed row y is staged in LDS when it fits next to the bitmap (vocab 32000: 128 000 B + 4 000 B of the 160 KiB
//     one workgroup may declare), otherwise every pass recomputes it from memory (same arithmetic, same bits);
//   * every id gets the 64-bit sort key  (order-preserving integer image of y) << 32 | ~id : descending key order is exactly
//     (y descending, id ascending) and all keys are distinct;
//   * a radix descent on that key, 8 bits per level, with per-bucket COUNTS finds the key of the k'-th candidate (skipped for
//     top_k == 0); the same descent with per-bucket WEIGHT sums finds the crossing point of the prefix sum directly.  No sort,
//     no nucleus is materialised.  A level stops as soon as its bucket is resolved (holds exactly what is still needed / one id);
//   * weights are integers, trunc(exp(y - y_max) * 2^40), summed with 64-bit LDS integer atomics: the sums do not depend on the
//     order the atomics retire in, so the result is bit-reproducible across launches, processes and tensor-parallel ranks.
//     Each thread folds runs of equal bucket into one atomic, which removes most of the same-address serialisation of the
//     top levels (sign + exponent bits are nearly constant over a row of logits).
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"
#include <cfloat>

namespace tllm
{
namespace kernels
{
namespace
{

constexpr int kThreads = 1024;
constexpr int kBuckets = 256;
// static LDS of the kernel is below 6 KiB; the rest of the 160 KiB a workgroup may declare is the dynamic part
constexpr size_t kDynLdsBudget = 160 * 1024 - 6 * 1024;
constexpr float kFixedOne = 1099511627776.0f; // 2^40

struct SampleArgs
{
    SamplingParams p;
    // derived on the host (launch_sampling_step)
    int32_t kprime = 1;    // candidates kept, 1 .. vocab
    float pprime = 1.f;    // share of their mass the draw may reach
    float inv_temp = 1.f;  // 1 / (temperature + 1e-6f)
    int32_t use_temp = 0;
    int32_t pen_mode = 0;  // 0 none, 1 repetition, 2 presence
    float pen = 0.f;
    int32_t bm_words = 0;  // dynamic LDS: history bitmap words, then (staged) vocab floats
    int32_t staged = 0;
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11); word 0 of the output block
__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r)
    {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int delta)
{
    const uint32_t lo = __shfl_up((uint32_t) v, delta, 64), hi = __shfl_up((uint32_t) (v >> 32), delta, 64);
    return ((uint64_t) hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    const uint32_t lo = __shfl((uint32_t) v, src, 64), hi = __shfl((uint32_t) (v >> 32), src, 64);
    return ((uint64_t) hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m)
{
    const uint32_t lo = __shfl_xor((uint32_t) v, m, 64), hi = __shfl_xor((uint32_t) (v >> 32), m, 64);
    return ((uint64_t) hi << 32) | lo;
}

// (y descending, id ascending) as one descending 64-bit key
__device__ __forceinline__ uint64_t sort_key(float y, int id)
{
    const uint32_t bits = __float_as_uint(y);
    const uint32_t k = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ((uint64_t) k << 32) | (uint32_t) ~(uint32_t) id;
}
__device__ __forceinline__ float key_value(uint64_t key)
{
    const uint32_t k = (uint32_t) (key >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Wave 0, all 64 lanes: the buckets are walked from 255 down; `hist` is read as uint64.  Returns in every lane the grand total;
// the one lane that holds the crossing  before < need <= before + hist[d]  (1 <= need <= total) stores d and `before`.
template <typename T, typename NeedFn>
__device__ __forceinline__ void scan_pick(const T* hist, NeedFn need_of_total, int* s_d, uint64_t* s_before, uint64_t* s_need)
{
    const int lane = threadIdx.x & 63;
    uint64_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        v[j] = (uint64_t) hist[kBuckets - 1 - 4 * lane - j];
        s += v[j];
    }
    uint64_t incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        const uint64_t t = shfl_up_u64(incl, off);
        if (lane >= off)
            incl += t;
    }
    const uint64_t total = shfl_u64(incl, 63);
    const uint64_t need = need_of_total(total);
    uint64_t before = incl - s;
    if (before < need && need <= incl)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            if (before + v[j] >= need)
            {
                *s_d = kBuckets - 1 - 4 * lane - j;
                *s_before = before;
                *s_need = need;
                break;
            }
            before += v[j];
        }
    }
}

// Steps 1 - 5 of the rule (SamplingParams in kernels.h) for ONE row, by the whole workgroup of kThreads threads: the body the step
// kernel and the verify-rows kernel share, so that the two select the same id bit for bit.  The row is given by what the rule
// reads: raw_logit(v) the fp32 logit of id v < V, for_history(mark) calls mark(id) for every id of the row's history (the
// workgroup's threads share them out; called only with a penalty), gnum the generated-token number (min_length), u the variate.
// dyn is the kernel's dynamic LDS (a.bm_words bitmap words, then V floats when a.staged).  Every thread returns the chosen id.
template <typename LogitFn, typename HistoryFn>
__device__ __forceinline__ int draw_row(const SampleArgs& a, const int V, const int end_id, const int gnum, const float u,
    uint32_t* dyn, LogitFn raw_logit, HistoryFn for_history)
{
    __shared__ uint64_t s_w[kBuckets];
    __shared__ uint32_t s_cnt[kBuckets];
    __shared__ uint32_t s_min[kBuckets];
    __shared__ uint64_t s_red[kThreads / 64];
    __shared__ uint64_t s_before, s_need;
    __shared__ int s_d;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t* bm = dyn;
    float* sy = reinterpret_cast<float*>(dyn + a.bm_words);
    int chosen;

    // ---- history bitmap
    if (a.pen_mode)
    {
        for (int i = tid; i < a.bm_words; i += kThreads)
            bm[i] = 0;
        __syncthreads();
        for_history([&](int id) {
            if (id >= 0 && id < V)
                atomicOr(&bm[id >> 5], 1u << (id & 31));
        });
        __syncthreads();
    }
    const bool mask_end = gnum < a.p.min_length && end_id >= 0 && end_id < V;
    auto compute_y = [&](int v) -> float {
        float y = raw_logit(v);
        // separately rounded operations (no fused multiply-add across them): every pass and the host restatement get the same y
        if (a.use_temp)
            y = __fmul_rn(y, a.inv_temp);
        if (a.pen_mode && ((bm[v >> 5] >> (v & 31)) & 1u))
            y = a.pen_mode == 1 ? (y < 0.f ? __fmul_rn(y, a.pen) : __fdiv_rn(y, a.pen)) : __fsub_rn(y, a.pen);
        if (mask_end && v == end_id)
            y = -FLT_MAX;
        if (!(y == y))
            y = -INFINITY;
        if (y == 0.f)
            y = 0.f; // -0 -> +0: one key per value
        return y;
    };
    auto get_y = [&](int v) -> float { return a.staged ? sy[v] : compute_y(v); };

    // ---- pass 1: stage y, largest key of the row (= y_max and the arg-max with ties to the lowest id)
    uint64_t best = 0;
    constexpr int kBatch = 8; // loads of a thread in flight together (latency-bound otherwise, as the greedy step)
    for (int v0 = tid; v0 < V; v0 += kThreads * kBatch)
    {
        float yy[kBatch];
#pragma unroll
        for (int e = 0; e < kBatch; ++e)
        {
            const int v = v0 + e * kThreads;
            yy[e] = v < V ? compute_y(v) : -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < kBatch; ++e)
        {
            const int v = v0 + e * kThreads;
            if (v < V)
            {
                if (a.staged)
                    sy[v] = yy[e];
                const uint64_t key = sort_key(yy[e], v);
                best = key > best ? key : best;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
    {
        const uint64_t o = shfl_xor_u64(best, m);
        best = o > best ? o : best;
    }
    if (lane == 0)
        s_red[wid] = best;
    __syncthreads();
    for (int w = 0; w < kThreads / 64; ++w)
        best = s_red[w] > best ? s_red[w] : best;
    const float ymax = key_value(best);
    chosen = (int) ~(uint32_t) best;

    if (a.kprime > 1 && ymax != -INFINITY)
    {
        // levels: the 4 bytes of the value image, then the bytes of ~id that can differ (the higher ones are 0xff for all)
        int nid = 1;
        while (nid < 4 && ((uint32_t) (V - 1) >> (8 * nid)))
            ++nid;
        const uint64_t fixed = nid == 4 ? 0ull : (uint64_t) (0xffffffffu << (8 * nid));
        const int nlev = 4 + nid;
        auto shift_of = [&](int l) { return l < 4 ? 56 - 8 * l : 8 * (nid - 1 - (l - 4)); };

        // ---- the key of the k'-th candidate: everything >= kth is a candidate
        uint64_t kth = 0;
        if (a.kprime < V)
        {
            uint64_t prefix = fixed, mask = fixed, need = (uint64_t) a.kprime;
            for (int l = 0; l < nlev; ++l)
            {
                const int sh = shift_of(l);
                if (tid < kBuckets)
                    s_cnt[tid] = 0;
                __syncthreads();
                int cur = -1;
                uint32_t run = 0;
                for (int v = tid; v < V; v += kThreads)
                {
                    const uint64_t key = sort_key(get_y(v), v);
                    if ((key & mask) != prefix)
                        continue;
                    const int d = (int) (key >> sh) & 255;
                    if (d != cur)
                    {
                        if (run)
                            atomicAdd(&s_cnt[cur], run);
                        cur = d;
                        run = 0;
                    }
                    ++run;
                }
                if (run)
                    atomicAdd(&s_cnt[cur], run);
                __syncthreads();
                if (wid == 0)
                    scan_pick(s_cnt, [&](uint64_t) { return need; }, &s_d, &s_before, &s_need);
                __syncthreads();
                const int d = s_d & (kBuckets - 1);
                need -= s_before;
                prefix |= (uint64_t) d << sh;
                mask |= 255ull << sh;
                if ((uint64_t) s_cnt[d] == need) // the whole bucket belongs to the candidates
                    break;
                __syncthreads(); // s_cnt is cleared next
            }
            kth = prefix;
            __syncthreads();
        }

        // ---- the crossing point of the prefix sum of the candidates' weights
        auto weight = [&](float y) -> uint64_t {
            if (y == ymax)
                return (uint64_t) kFixedOne;
            if (y == -INFINITY)
                return 0ull;
            return (uint64_t) (expf(y - ymax) * kFixedOne);
        };
        uint64_t prefix = fixed, mask = fixed, target = 0;
        for (int l = 0; l < nlev; ++l)
        {
            const int sh = shift_of(l);
            if (tid < kBuckets)
            {
                s_cnt[tid] = 0;
                s_w[tid] = 0;
                s_min[tid] = 0xffffffffu;
            }
            __syncthreads();
            int cur = -1;
            uint32_t run = 0, run_min = 0xffffffffu;
            uint64_t run_w = 0;
            auto flush = [&]() {
                if (run)
                {
                    atomicAdd(&s_cnt[cur], run);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&s_w[cur]), (unsigned long long) run_w);
                    atomicMin(&s_min[cur], run_min);
                }
            };
            for (int v = tid; v < V; v += kThreads)
            {
                const float y = get_y(v);
                const uint64_t key = sort_key(y, v);
                if (key < kth || (key & mask) != prefix)
                    continue;
                const int d = (int) (key >> sh) & 255;
                if (d != cur)
                {
                    flush();
                    cur = d;
                    run = 0;
                    run_w = 0;
                    run_min = 0xffffffffu;
                }
                ++run;
                run_w += weight(y);
                run_min = min(run_min, (uint32_t) v);
            }
            flush();
            __syncthreads();
            if (wid == 0)
            {
                if (l == 0)
                    scan_pick(
                        s_w,
                        [&](uint64_t total) {
                            // target = u * p' * S, as the smallest integer the integer prefix sums can reach
                            const double t = ceil((double) u * (double) a.pprime * (double) total);
                            uint64_t T = t >= 18446744073709551615.0 ? total : (uint64_t) t;
                            T = T > total ? total : T;
                            return T < 1 ? (uint64_t) 1 : T;
                        },
                        &s_d, &s_before, &s_need);
                else
                    scan_pick(s_w, [&](uint64_t) { return target; }, &s_d, &s_before, &s_need);
            }
            __syncthreads();
            const int d = s_d & (kBuckets - 1);
            target = s_need - s_before;
            prefix |= (uint64_t) d << sh;
            mask |= 255ull << sh;
            if (s_cnt[d] == 1u)
            {
                chosen = (int) s_min[d];
                break;
            }
            __syncthreads(); // the histograms are cleared next
        }
    }
    return chosen;
}

// u in (0, 1] of row b's generated token number gnum: a function of (seed, b, gnum) and nothing else
__device__ __forceinline__ float draw_uniform(uint64_t seed, int b, int gnum)
{
    const uint32_t r0 = philox4x32_10_word0((uint32_t) b, (uint32_t) gnum, 0u, 0u, (uint32_t) seed, (uint32_t) (seed >> 32));
    return (float) ((r0 >> 8) + 1u) * 5.9604644775390625e-8f; // 2^-24
}

__global__ __launch_bounds__(kThreads) void sampling_step_kernel(const SampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    __shared__ int s_id;

    const GreedyParams& g = a.p.g;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = g.vocab;

    // read before thread 0 advances them (several barriers further down)
    const int slot = g.seq_len[b] + (g.advance ? 1 : 0); // where this token goes = slots of the row in use before it
    const int gnum = slot - a.p.g_base + 1;              // generated token number, 1-based
    const int was_finished = g.finished ? g.finished[b] : 0;

    if (g.rope_row_out && tid >= 64 && tid < 64 + g.rope_half)
    {
        // next step's position: (seq_len after this step's advance) - padding of this sequence
        const int j = tid - 64;
        int pos = slot - (g.max_input_len - g.input_lengths[b]);
        pos = pos < 0 ? 0 : (pos >= g.rope_table_len ? g.rope_table_len - 1 : pos);
        reinterpret_cast<float2*>(g.rope_row_out)[(int64_t) b * g.rope_half + j]
            = reinterpret_cast<const float2*>(g.rope_table)[(int64_t) pos * g.rope_half + j];
        if (j == 0 && g.rope_pos_out)
            g.rope_pos_out[b] = pos;
    }

    const float u = draw_uniform(a.p.random_seed, b, gnum);
    if (a.p.u_out && tid == 0)
        a.p.u_out[b] = u;

    int chosen = g.end_id;
    if (!was_finished) // uniform over the workgroup
        chosen = draw_row(
            a, V, g.end_id, gnum, u, dyn,
            [&](int v) -> float {
                const int part = v / g.vocab_part, vi = v - part * g.vocab_part;
                return g.logits[((int64_t) part * g.batch + b) * g.vocab_part + vi];
            },
            [&](auto mark) {
                const int32_t* h = a.p.history + (int64_t) b * a.p.history_stride;
                const int n_prompt = g.input_lengths ? min(g.input_lengths[b], g.max_input_len) : g.max_input_len;
                // generated tokens behind the prompt slots; clamped BEFORE the sum (g is the caller's through tllm_sample_tokens)
                const int room = max(a.p.history_stride - g.max_input_len, 0);
                const int hist_end = min(g.max_input_len, a.p.history_stride) + min(max(gnum - 1, 0), room);
                for (int t = tid; t < hist_end; t += kThreads)
                {
                    if (t >= n_prompt && t < g.max_input_len) // padding slots
                        continue;
                    mark(h[t]);
                }
            });

    // ---- bookkeeping: a second copy of greedy_step_kernel's (decode_step.hip), not shared code - the RoPE row above, the commit,
    // step_epoch and the next input row below must be edited in both kernels together
    __syncthreads();
    if (tid == 0)
    {
        int id = chosen;
        if (g.advance)
            g.seq_len[b] = slot;
        if (g.finished)
        {
            if (was_finished)
                id = g.end_id;
            else if (g.end_id >= 0 && id == g.end_id)
                g.finished[b] = 1;
        }
        if (g.out_ids && slot < g.out_stride)
            g.out_ids[(int64_t) b * g.out_stride + slot] = id;
        g.cur_ids[b] = id;
        s_id = id;
        if (b == 0 && g.step_epoch)
            *g.step_epoch += 1;
    }
    if (g.emb_table) // uniform: the next step's input row, as the greedy step leaves it
    {
        __syncthreads();
        const int id = s_id;
        const bool ok = id >= 0 && id < V;
        const uint16_t* src = reinterpret_cast<const uint16_t*>(g.emb_table) + (int64_t) (ok ? id : 0) * g.hidden;
        uint16_t* dst = reinterpret_cast<uint16_t*>(g.x_out) + (int64_t) b * g.hidden;
        for (int k = tid * 8; k < g.hidden; k += kThreads * 8) // hidden % 8 == 0 (checked by the launcher)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(src + k);
            *reinterpret_cast<uint4*>(dst + k) = ok ? v : make_uint4(0, 0, 0, 0);
        }
    }
}

// The draw on all n rows of a verify pass (SpecSampleParams in kernels.h): workgroup (b, i) draws, from logits row b * n + i, the
// token plain sampled decoding would put behind t[0..i].  Nothing of the step's bookkeeping: the accept step commits.
struct SpecSampleArgs
{
    SampleArgs a;
    int32_t n = 0;
    const int32_t* ids = nullptr;
    const int32_t* limit = nullptr;
    int32_t* draws = nullptr;
};

__global__ __launch_bounds__(kThreads) void spec_sample_rows_kernel(const SpecSampleArgs q)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    const SampleArgs& a = q.a;
    const GreedyParams& g = a.p.g;
    const int n = q.n, b = blockIdx.x / n, i = blockIdx.x - b * n, tid = threadIdx.x;
    const int V = g.vocab, S = g.max_input_len;
    const int p = g.seq_len[b];
    const int lim = q.limit ? q.limit[b] : 0x7fffffff;
    const bool frozen = (g.finished && g.finished[b] != 0) || p >= lim || p < 0;
    const int gnum = (int) ((int64_t) p + i + 2 - a.p.g_base); // the token of slot p + i + 1
    const int64_t row = (int64_t) b * n + i;

    const float u = draw_uniform(a.p.random_seed, b, gnum);
    if (a.p.u_out && tid == 0)
        a.p.u_out[row] = u;

    int chosen = g.end_id;
    if (!frozen) // uniform over the workgroup
        chosen = draw_row(
            a, V, g.end_id, gnum, u, dyn, [&](int v) -> float { return g.logits[row * g.vocab_part + v]; },
            [&](auto mark) {
                const int32_t* h = a.p.history + (int64_t) b * a.p.history_stride;
                const int32_t* t = q.ids + (int64_t) b * n;
                const int n_prompt = g.input_lengths ? min(g.input_lengths[b], S) : S;
                const int rec_end = min(p, a.p.history_stride); // the record: the prompt and the tokens committed before the pass
                for (int s = tid; s < rec_end; s += kThreads)
                {
                    if (s >= n_prompt && s < S) // padding slots
                        continue;
                    mark(h[s]);
                }
                for (int j = tid; j <= i; j += kThreads) // t[0..i] in the places of slots p .. p + i
                {
                    const int64_t s = (int64_t) p + j;
                    if (s >= n_prompt && s < S)
                        continue;
                    mark(t[j]);
                }
            });
    if (tid == 0)
        q.draws[row] = chosen;
}

} // namespace

bool sampling_is_greedy(const SamplingParams& p)
{
    return p.top_k == 1 && p.temperature == 1.f && p.repetition_penalty == 1.f && p.presence_penalty == 0.f && p.min_length <= 1;
}

// What both launchers derive from the configuration: the checks of its fields, k' and p', the penalty mode, and the dynamic LDS
// (history bitmap, then the staged row when it fits beside it).  *dyn_out = bytes of dynamic LDS.
static int derive_args(SampleArgs& a, size_t& dyn_out, const SamplingParams& p, const char* who)
{
    const GreedyParams& g = p.g;
    if (!(p.temperature > 0.f) || p.top_k < 0 || !(p.top_p >= 0.f) || !(p.repetition_penalty > 0.f))
    {
        set_error("%s: needs temperature > 0, top_k >= 0, top_p >= 0, repetition_penalty > 0", who);
        return -1;
    }
    if (p.repetition_penalty != 1.f && p.presence_penalty != 0.f)
    {
        set_error("%s: repetition_penalty and presence_penalty are mutually exclusive", who);
        return -1;
    }
    a.p = p;
    // layers/topKSamplingLayer.cu:42-60
    int k = p.top_k;
    float pp = p.top_p > 1.f ? 1.f : p.top_p;
    if (k == 0 && pp == 0.f)
        k = 1;
    else if (k > 0 && pp == 0.f)
        pp = 1.f;
    k = k == 0 ? g.vocab : (k > 1024 ? 1024 : k);
    a.kprime = k > g.vocab ? g.vocab : k;
    a.pprime = pp;
    a.use_temp = p.temperature != 1.f;
    a.inv_temp = 1.f / (p.temperature + 1e-6f);
    a.pen_mode = p.repetition_penalty != 1.f ? 1 : (p.presence_penalty != 0.f ? 2 : 0);
    a.pen = a.pen_mode == 1 ? p.repetition_penalty : p.presence_penalty;
    if (a.pen_mode && (!p.history || p.history_stride <= 0))
    {
        set_error("%s: a penalty needs the row's token history", who);
        return -1;
    }
    a.bm_words = a.pen_mode ? (g.vocab + 31) / 32 : 0;
    const size_t bm_bytes = (size_t) a.bm_words * 4, row_bytes = (size_t) g.vocab * 4;
    if (bm_bytes > kDynLdsBudget)
    {
        set_error("%s: the history bitmap of a vocabulary of %d does not fit the LDS", who, g.vocab);
        return -1;
    }
    a.staged = bm_bytes + row_bytes <= kDynLdsBudget;
    dyn_out = bm_bytes + (a.staged ? row_bytes : 0);
    return 0;
}

int launch_spec_sample_rows(const SpecSampleParams& p, hipStream_t stream)
{
    const GreedyParams& g = p.s.g;
    if (g.batch <= 0)
        return 0;
    if (p.n < 1 || p.n > kVerifyMaxTokens)
    {
        set_error("spec sample rows: n %d outside [1, %d]", p.n, kVerifyMaxTokens);
        return -1;
    }
    if (g.nparts != 1)
    {
        set_error("spec sample rows: the verify rows come in one vocabulary part (got %d parts)", g.nparts);
        return -1;
    }
    if (!g.logits || !g.seq_len || !p.ids || !p.draws || g.vocab <= 0 || g.vocab_part < g.vocab || g.max_input_len < 0)
    {
        set_error("spec sample rows: bad arguments (the logits rows, seq_len, the ids and the draws are needed, vocab %d <= vocab_part %d)",
            g.vocab, g.vocab_part);
        return -1;
    }
    SpecSampleArgs q;
    size_t dyn = 0;
    if (derive_args(q.a, dyn, p.s, "spec sample rows"))
        return -1;
    q.n = p.n;
    q.ids = p.ids;
    q.limit = p.limit;
    q.draws = p.draws;
    const void* kfn = reinterpret_cast<const void*>(spec_sample_rows_kernel);
    if (dyn > 64 * 1024)
        launch_util::ensure_dynamic_lds(kfn, kDynLdsBudget);
    hipLaunchKernelGGL(spec_sample_rows_kernel, dim3(g.batch * p.n), dim3(kThreads), dyn, stream, q);
    return launch_util::check_launch("spec_sample_rows");
}

int launch_sampling_step(const SamplingParams& p, hipStream_t stream)
{
    const GreedyParams& g = p.g;
    if (g.batch <= 0)
        return 0;
    if (!g.logits || !g.cur_ids || !g.seq_len || g.vocab <= 0 || g.vocab_part <= 0 || g.nparts <= 0
        || (int64_t) g.nparts * g.vocab_part < g.vocab)
    {
        set_error("sampling step: bad logits / shape arguments");
        return -1;
    }
    if (g.emb_table && (!g.x_out || g.hidden % 8 != 0))
    {
        set_error("sampling step: fused embedding gather needs x_out and hidden %% 8 == 0 (got %d)", g.hidden);
        return -1;
    }
    if (g.rope_row_out && (!g.rope_table || !g.input_lengths || g.rope_half > kThreads - 64))
    {
        set_error("sampling step: the RoPE row needs its table, input_lengths and rope_half <= %d", kThreads - 64);
        return -1;
    }
    SampleArgs a;
    size_t dyn = 0;
    if (derive_args(a, dyn, p, "sampling step"))
        return -1;
    const void* kfn = reinterpret_cast<const void*>(sampling_step_kernel);
    if (dyn > 64 * 1024)
        launch_util::ensure_dynamic_lds(kfn, kDynLdsBudget);
    hipLaunchKernelGGL(sampling_step_kernel, dim3(g.batch), dim3(kThreads), dyn, stream, a);
    return launch_util::check_launch("sampling_step");
}

} // namespace kernels
} // namespace tllm
