// Per-token log-probabilities from fp32 logits rows (TokenLogprobParams in kernels.h states the rule and the special values).
//   token_logprob_partial_kernel  one workgroup of 256 threads per (row, vocabulary part): ONE pass over the part with an online
//                                 max + sum (the flash-softmax recurrence), the arg-max and the target's logit on the way; leaves
//                                 an 8-word record {m, s, xt, top_val, top_id, 0, 0, 0} per (part, row);
//   token_logprob_merge_kernel    one thread per row: the records of its parts, in part order, become log_prob / lse / top1.
// The row is read with 16-byte loads: rows of an odd leading dimension (vocab 32003) start at any 4-byte boundary, so up to three
// head elements are peeled to reach a 16-byte address and up to three tail elements follow the last whole vector.
// No atomics, no waits on other workgroups: every thread folds a fixed subset of the ids in a fixed order, the 64 lanes of a wave
// are joined by a shuffle tree, the 4 waves in wave order - the record is a function of (row contents, alignment of the row,
// launch geometry) alone.  The logits are only read.
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"
#include <climits>
#include <cmath>

namespace tllm
{
namespace kernels
{
namespace
{

using launch_util::check_launch;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRec = 8; // words per record

// running state of the one-pass reduction: s = sum exp(x - m) over the ids folded so far, (tv, ti) their arg-max
struct Run
{
    float m, s, tv;
    int32_t ti;
};

__device__ __forceinline__ Run run_empty()
{
    return Run{-INFINITY, 0.f, -INFINITY, INT_MAX};
}

__device__ __forceinline__ void take_top(Run& r, float x, int32_t id)
{
    if (x > r.tv || (x == r.tv && id < r.ti))
    {
        r.tv = x;
        r.ti = id;
    }
}

// new running maximum: the sum so far is rescaled once (m = -inf: s is 0 and stays 0)
__device__ __forceinline__ void raise(Run& r, float cm)
{
    if (cm > r.m)
    {
        r.s *= expf(r.m - cm);
        r.m = cm;
    }
}

__device__ __forceinline__ void add_term(Run& r, float x)
{
    if (x > -INFINITY) // then r.m >= x is finite; an -inf entry adds nothing
        r.s += expf(x - r.m);
}

__device__ __forceinline__ void fold1(Run& r, float x, int32_t id)
{
    raise(r, x);
    add_term(r, x);
    take_top(r, x, id);
}

// four consecutive ids: one rescale for the group, then its four terms
__device__ __forceinline__ void fold4(Run& r, const float4& v, int32_t id)
{
    raise(r, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    if (r.m > -INFINITY) // exp(-inf - m) = 0: an -inf entry adds nothing.  The group is summed as a tree before it joins the
                         // thread's chain: 32 + 2 additions deep per thread at vocab 32000 instead of 125
        r.s += (expf(v.x - r.m) + expf(v.y - r.m)) + (expf(v.z - r.m) + expf(v.w - r.m));
    take_top(r, v.x, id);
    take_top(r, v.y, id + 1);
    take_top(r, v.z, id + 2);
    take_top(r, v.w, id + 3);
}

// a (+) b, a's ids before b's
__device__ __forceinline__ Run join(const Run& a, const Run& b)
{
    Run o;
    o.m = fmaxf(a.m, b.m);
    o.s = 0.f;
    if (a.m > -INFINITY)
        o.s = a.s * expf(a.m - o.m);
    if (b.m > -INFINITY)
        o.s += b.s * expf(b.m - o.m);
    o.tv = a.tv;
    o.ti = a.ti;
    take_top(o, b.tv, b.ti);
    return o;
}

__device__ __forceinline__ Run shfl_down_run(const Run& r, int delta)
{
    Run o;
    o.m = __shfl_down(r.m, delta, 64);
    o.s = __shfl_down(r.s, delta, 64);
    o.tv = __shfl_down(r.tv, delta, 64);
    o.ti = __shfl_down(r.ti, delta, 64);
    return o;
}

__global__ __launch_bounds__(kThreads) void token_logprob_partial_kernel(const TokenLogprobParams p)
{
    const int row = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    // the part's real columns: ids [first, first + n)
    const int64_t first = (int64_t) (p.first_part + part) * p.vocab_part;
    const int64_t left = (int64_t) p.vocab - first;
    const int n = left <= 0 ? 0 : (left < p.vocab_part ? (int) left : p.vocab_part);
    const float* x = p.logits + (int64_t) part * p.part_stride + (int64_t) row * p.ld;

    // [0, head) scalars up to the first 16-byte address, nvec whole vectors, `tail` scalars behind them
    int head = (int) (((16u - (uint32_t) (reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    const int nvec = (n - head) >> 2;
    const int tail = n - head - 4 * nvec;
    const int32_t id0 = (int32_t) first;

    Run r = run_empty();
    if (tid < head)
        fold1(r, x[tid], id0 + tid);
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    int v = tid;
    for (; v + kThreads < nvec; v += 2 * kThreads)
    {
        // both loads in flight before the first dependent exp
        const float4 a = xv[v], b = xv[v + kThreads];
        fold4(r, a, id0 + head + 4 * v);
        fold4(r, b, id0 + head + 4 * (v + kThreads));
    }
    if (v < nvec)
        fold4(r, xv[v], id0 + head + 4 * v);
    if (tid < tail)
        fold1(r, x[head + 4 * nvec + tid], id0 + head + 4 * nvec + tid);

    // lanes: shuffle tree, the lower lane's ids first; waves: in wave order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        const Run o = shfl_down_run(r, d);
        r = join(r, o);
    }
    __shared__ Run wave_run[kWaves];
    if ((tid & 63) == 0)
        wave_run[tid >> 6] = r;
    __syncthreads();
    if (tid == 0)
    {
        Run t = wave_run[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            t = join(t, wave_run[w]);
        const int64_t tg = p.targets[row];
        float xt = -INFINITY;
        if (tg >= first && tg < first + n)
            xt = x[tg - first];
        float4* rec = reinterpret_cast<float4*>(p.partials + ((int64_t) part * p.rows + row) * kRec);
        rec[0] = make_float4(t.m, t.s, xt, t.tv);
        rec[1] = make_float4(__int_as_float(t.ti), 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(kThreads) void token_logprob_merge_kernel(const float* partials, int32_t nparts, int32_t rows,
    int32_t vocab, const int32_t* targets, float* log_probs, float* lse_out, int32_t* top1_ids)
{
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows)
        return;
    float M = -INFINITY;
    for (int q = 0; q < nparts; ++q)
        M = fmaxf(M, partials[((int64_t) q * rows + row) * kRec]);
    float S = 0.f, xt = -INFINITY, tv = -INFINITY;
    int32_t ti = INT_MAX;
    for (int q = 0; q < nparts; ++q)
    {
        const float4 a = *reinterpret_cast<const float4*>(partials + ((int64_t) q * rows + row) * kRec);
        const int32_t id = __float_as_int(partials[((int64_t) q * rows + row) * kRec + 4]);
        if (a.x > -INFINITY)
            S += a.y * expf(a.x - M); // one part: exp(0) = 1 and S = s, bit for bit
        xt = fmaxf(xt, a.z);          // at most one part holds the target
        if (a.w > tv || (a.w == tv && id < ti))
        {
            tv = a.w;
            ti = id;
        }
    }
    const float lse = M > -INFINITY ? M + logf(S) : -INFINITY;
    const int32_t tg = targets[row];
    float lp = 0.f;
    if (tg >= 0 && tg < vocab)
        lp = xt > -INFINITY ? xt - lse : -INFINITY;
    log_probs[row] = lp;
    if (lse_out)
        lse_out[row] = lse;
    if (top1_ids)
        top1_ids[row] = ti == INT_MAX ? 0 : ti;
}

} // namespace

int launch_token_logprob_partial(const TokenLogprobParams& p, hipStream_t stream)
{
    if (p.rows <= 0 || p.nparts <= 0)
        return 0;
    if (!p.logits || !p.targets || !p.partials || p.vocab_part < 1 || p.vocab < 1 || p.first_part < 0 || p.ld < p.vocab_part
        || (p.nparts > 1 && p.part_stride < (int64_t) (p.rows - 1) * p.ld + p.vocab_part) || p.nparts > 65535
        || (int64_t) (p.first_part + p.nparts) * p.vocab_part > (int64_t) INT_MAX)
    {
        set_error("token_logprob: bad arguments (rows %d, parts %d from %d, vocab %d in parts of %d, ld %lld, part stride %lld)", p.rows,
            p.nparts, p.first_part, p.vocab, p.vocab_part, (long long) p.ld, (long long) p.part_stride);
        return -1;
    }
    hipLaunchKernelGGL(token_logprob_partial_kernel, dim3(p.rows, p.nparts), dim3(kThreads), 0, stream, p);
    return check_launch("token_logprob_partial");
}

int launch_token_logprob_merge(const float* partials, int32_t nparts, int32_t rows, int32_t vocab, const int32_t* targets,
    float* log_probs, float* lse, int32_t* top1_ids, hipStream_t stream)
{
    if (rows <= 0)
        return 0;
    if (!partials || !targets || !log_probs || nparts < 1 || vocab < 1)
    {
        set_error("token_logprob_merge: bad arguments (rows %d, parts %d, vocab %d)", rows, nparts, vocab);
        return -1;
    }
    hipLaunchKernelGGL(token_logprob_merge_kernel, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, partials, nparts,
        rows, vocab, targets, log_probs, lse, top1_ids);
    return check_launch("token_logprob_merge");
}

} // namespace kernels
} // namespace tllm
