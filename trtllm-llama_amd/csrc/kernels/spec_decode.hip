// Speculative greedy decoding (the numpy restatement is tensorrt_llm/runtime/spec_ref.py): the two
// bookkeeping kernels around a verify pass, and the targets of its scoring.  One workgroup per sequence, nothing crosses a
// workgroup: the kernel boundary orders them against the pass.
//   (a) spec_accept_kernel    takes the sampler's place behind a verify pass over n ids per sequence: the longest prefix of the
//                             drafts that IS the arg-max of the row before it is kept, the arg-max behind it is the new pending
//                             token, and the step words (SpecAcceptParams in kernels.h states the rule) are committed as
//                             greedy_step_kernel (decode_step.hip) commits them for one token;
//   (b) prompt_lookup_kernel  drafts from the sequence's own token record: the followers of the most recent earlier occurrence
//                             of its last max_ngram .. 1 tokens (PromptLookupParams);
//   (c) spec_targets_kernel   targets[b][i] = ids[b][i + 1], -1 on the last row: what the scoring of a verify pass is asked for.
// Every index is guarded: an output slot by < out_stride, a RoPE position is clamped into the table, an id outside [0, vocab)
// gathers a zero row (accept) or is passed on as 0 (lookup); a wrong word on the device can give wrong ids, never an access
// outside the buffers.
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"

namespace tllm
{
namespace kernels
{
using launch_util::check_launch;

namespace
{

constexpr int kSpecThreads = 256;

__global__ __launch_bounds__(kSpecThreads) void spec_accept_kernel(const SpecAcceptParams p)
{
    __shared__ int s_m, s_id, s_pos;
    const GreedyParams& g = p.g;
    const int b = blockIdx.x, n = p.n, tid = threadIdx.x;
    if (tid == 0)
    {
        const int sl = g.seq_len[b];
        const int lim = p.limit ? p.limit[b] : 0x7fffffff;
        const int fin = g.finished ? g.finished[b] : 0;
        int m = -1, id = g.cur_ids[b]; // frozen: nothing of the sequence changes (its input row is put back below)
        if (!fin && sl < lim && sl >= 0) // (a negative length is no live sequence: its slots do not exist)
        {
            const int32_t* t = p.ids + (int64_t) b * n;
            const int32_t* a = p.top1 + (int64_t) b * n;
            m = 0;
            // (sl + m + 1 < lim in 64 bits: sl near INT32_MAX must not wrap)
            while (m + 1 < n && (int64_t) sl + m + 1 < lim && !(g.end_id >= 0 && a[m] == g.end_id) && t[m + 1] == a[m])
                ++m;
            id = a[m];
            int32_t* o = g.out_ids + (int64_t) b * g.out_stride;
            for (int i = 0; i <= m; ++i)
                if ((int64_t) sl + i < g.out_stride)
                    o[sl + i] = t[i];
            const int64_t nsl = (int64_t) sl + m + 1;
            if (nsl < g.out_stride)
                o[nsl] = id;
            g.seq_len[b] = (int32_t) nsl;
            g.cur_ids[b] = id;
            if (g.finished && g.end_id >= 0 && id == g.end_id)
                g.finished[b] = 1;
            int64_t pos = nsl - (g.max_input_len - (g.input_lengths ? g.input_lengths[b] : g.max_input_len));
            pos = pos < 0 ? 0 : (pos >= g.rope_table_len ? g.rope_table_len - 1 : pos);
            s_pos = (int) pos;
            if (g.rope_row_out && g.rope_pos_out)
                g.rope_pos_out[b] = (int32_t) pos;
        }
        if (p.accepted)
            p.accepted[b] = m;
        s_m = m;
        s_id = id;
        if (b == 0 && g.step_epoch)
            *g.step_epoch += 1; // only this thread of this launch touches the word
    }
    __syncthreads();
    const int m = s_m, id = s_id;
    if (g.emb_table) // the pass used x as its activation buffer: the next step's input row, of the frozen sequences too
    {
        const bool ok = id >= 0 && id < g.vocab;
        const uint16_t* src = reinterpret_cast<const uint16_t*>(g.emb_table) + (int64_t) (ok ? id : 0) * g.hidden;
        uint16_t* dst = reinterpret_cast<uint16_t*>(g.x_out) + (int64_t) b * g.hidden;
        for (int k = tid * 8; k < g.hidden; k += kSpecThreads * 8) // hidden % 8 == 0 (checked by the launcher)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(src + k);
            *reinterpret_cast<uint4*>(dst + k) = ok ? v : make_uint4(0, 0, 0, 0);
        }
    }
    if (m < 0) // uniform
        return;
    if (g.rope_row_out)
    {
        const int pos = s_pos;
        for (int j = tid; j < g.rope_half; j += kSpecThreads)
            reinterpret_cast<float2*>(g.rope_row_out)[(int64_t) b * g.rope_half + j]
                = reinterpret_cast<const float2*>(g.rope_table)[(int64_t) pos * g.rope_half + j];
    }
    if (p.logits_out)
    {
        // row m of the sequence's n logits rows -> row b of the session's [B, vocab_part] logits
        const float* src = g.logits + ((int64_t) b * n + m) * g.vocab_part;
        float* dst = p.logits_out + (int64_t) b * g.vocab_part;
        if ((g.vocab_part & 3) == 0 && ((reinterpret_cast<uintptr_t>(g.logits) | reinterpret_cast<uintptr_t>(p.logits_out)) & 15) == 0)
            for (int k = tid; k < (g.vocab_part >> 2); k += kSpecThreads)
                reinterpret_cast<float4*>(dst)[k] = reinterpret_cast<const float4*>(src)[k];
        else
            for (int k = tid; k < g.vocab_part; k += kSpecThreads)
                dst[k] = src[k];
    }
}

// slot of element j of the logical sequence: the prompt's real tokens, then the generated ones (the padding slots are skipped)
__device__ __forceinline__ int lookup_slot(int j, int in_len, int max_in)
{
    return j < in_len ? j : max_in + (j - in_len);
}

__global__ __launch_bounds__(kSpecThreads) void prompt_lookup_kernel(const PromptLookupParams p)
{
    __shared__ int s_red[kSpecThreads / 64];
    __shared__ int s_best;
    const int b = blockIdx.x, tid = threadIdx.x, n = p.n, k = p.n - 1;
    const int32_t* row = p.out_ids + (int64_t) b * p.out_stride;
    int sl = p.seq_len[b];
    const int fin = p.finished ? p.finished[b] : 0;
    const int lim = p.limit ? p.limit[b] : 0x7fffffff;
    // a length outside [max_input_len, out_stride) cannot be a live sequence: no draft, and the pending token is read in range
    const bool sane = sl >= p.max_input_len && sl < p.out_stride;
    const bool frozen = fin != 0 || sl >= lim || !sane;
    sl = sl < 0 ? 0 : (sl >= p.out_stride ? p.out_stride - 1 : sl);
    int in_len = p.input_lengths ? p.input_lengths[b] : p.max_input_len;
    in_len = in_len < 0 ? 0 : (in_len > p.max_input_len ? p.max_input_len : in_len);
    auto valid = [&](int id) { return id >= 0 && id < p.vocab ? id : 0; };
    const int pending = valid(row[sl]);
    const int len = sane ? in_len + (sl - p.max_input_len + 1) : 0; // elements of the logical sequence
    int best = -1, best_g = 0;
    if (!frozen && k > 0) // uniform
    {
        for (int g = p.max_ngram; g >= 1; --g)
        {
            if (len < g + 1) // no start with a follower
                continue;
            int32_t suf[kLookupMaxNgram];
#pragma unroll
            for (int e = 0; e < kLookupMaxNgram; ++e)
                suf[e] = e < g ? row[lookup_slot(len - g + e, in_len, p.max_input_len)] : 0;
            int mine = -1;
            for (int s = tid; s + g < len; s += kSpecThreads) // ascending: the last match a thread sees is its most recent
            {
                bool eq = true;
#pragma unroll
                for (int e = 0; e < kLookupMaxNgram; ++e)
                    if (e < g)
                        eq = eq && row[lookup_slot(s + e, in_len, p.max_input_len)] == suf[e];
                if (eq)
                    mine = s;
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1)
            {
                const int o = __shfl_xor(mine, sh, 64);
                mine = o > mine ? o : mine;
            }
            __syncthreads(); // the words below may still be read from the g before
            if ((tid & 63) == 0)
                s_red[tid >> 6] = mine;
            __syncthreads();
            if (tid == 0)
            {
                int v = s_red[0];
                for (int w = 1; w < kSpecThreads / 64; ++w)
                    v = s_red[w] > v ? s_red[w] : v;
                s_best = v;
            }
            __syncthreads();
            if (s_best >= 0)
            {
                best = s_best;
                best_g = g;
                break; // uniform: every thread read the same word
            }
        }
    }
    int dl = 0;
    if (best >= 0)
    {
        dl = len - (best + best_g);
        dl = dl > k ? k : dl;
    }
    for (int i = tid; i < n; i += kSpecThreads)
    {
        int id = pending;
        if (i >= 1 && i <= dl)
            id = valid(row[lookup_slot(best + best_g + i - 1, in_len, p.max_input_len)]);
        p.ids[(int64_t) b * n + i] = id;
    }
    if (tid == 0)
    {
        if (p.draft_len)
            p.draft_len[b] = dl;
        if (p.state_out)
        {
            int32_t* st = p.state_out + (int64_t) b * 4;
            st[0] = p.seq_len[b];
            st[1] = fin;
            st[2] = dl;
            st[3] = frozen ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kSpecThreads) void spec_targets_kernel(int32_t* targets, const int32_t* ids, int32_t batch, int32_t n)
{
    const int64_t total = (int64_t) batch * n;
    for (int64_t r = (int64_t) blockIdx.x * kSpecThreads + threadIdx.x; r < total; r += (int64_t) gridDim.x * kSpecThreads)
        targets[r] = (r % n) + 1 < n ? ids[r + 1] : -1;
}

} // namespace

int launch_spec_accept(const SpecAcceptParams& p, hipStream_t stream)
{
    const GreedyParams& g = p.g;
    if (g.batch <= 0)
        return 0;
    if (!g.seq_len || !g.cur_ids || !g.out_ids || !p.ids || !p.top1 || p.n < 1 || p.n > kVerifyMaxTokens || g.out_stride < 1
        || g.vocab < 1)
    {
        set_error("spec accept: bad arguments (n %d in [1, %d], the ids, their arg-max ids and the step words are needed)", p.n,
            kVerifyMaxTokens);
        return -1;
    }
    if (g.emb_table && (!g.x_out || g.hidden <= 0 || (g.hidden & 7)))
    {
        set_error("spec accept: the embedding gather needs x_out and hidden %% 8 == 0 (got %d)", g.hidden);
        return -1;
    }
    if (g.rope_row_out && (!g.input_lengths || !g.rope_table || g.rope_half < 1 || g.rope_table_len < 1))
    {
        set_error("spec accept: the next RoPE row needs input_lengths and the RoPE table");
        return -1;
    }
    if (p.logits_out && (!g.logits || g.nparts != 1 || g.vocab_part < 1))
    {
        set_error("spec accept: the logits row copy needs the n rows per sequence in one vocabulary part (got %d parts)", g.nparts);
        return -1;
    }
    hipLaunchKernelGGL(spec_accept_kernel, dim3(g.batch), dim3(kSpecThreads), 0, stream, p);
    return check_launch("spec_accept");
}

int launch_prompt_lookup(const PromptLookupParams& p, hipStream_t stream)
{
    if (p.batch <= 0)
        return 0;
    if (!p.out_ids || !p.seq_len || !p.ids || p.n < 1 || p.n > kVerifyMaxTokens || p.max_ngram < 1 || p.max_ngram > kLookupMaxNgram
        || p.out_stride < 1 || p.max_input_len < 0 || p.max_input_len > p.out_stride || p.vocab < 1)
    {
        set_error("prompt lookup: bad arguments (n %d in [1, %d], max_ngram %d in [1, %d], max_input_len %d <= out_stride %d)", p.n,
            kVerifyMaxTokens, p.max_ngram, kLookupMaxNgram, p.max_input_len, p.out_stride);
        return -1;
    }
    hipLaunchKernelGGL(prompt_lookup_kernel, dim3(p.batch), dim3(kSpecThreads), 0, stream, p);
    return check_launch("prompt_lookup");
}

int launch_spec_targets(int32_t* targets, const int32_t* ids, int32_t batch, int32_t n, hipStream_t stream)
{
    if (!targets || !ids || batch < 1 || n < 1)
    {
        set_error("spec targets: bad arguments");
        return -1;
    }
    const int64_t total = (int64_t) batch * n;
    const int blocks = (int) ((total + kSpecThreads - 1) / kSpecThreads);
    hipLaunchKernelGGL(spec_targets_kernel, dim3(blocks > 64 ? 64 : blocks), dim3(kSpecThreads), 0, stream, targets, ids, batch, n);
    return check_launch("spec_targets");
}

} // namespace kernels
} // namespace tllm
