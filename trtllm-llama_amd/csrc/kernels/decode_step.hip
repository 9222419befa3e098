// The kernels that end a decode step: arg-max, the greedy step, the beam-search step and token forcing (teacher forcing for
// parity tests).  One workgroup per row.  sampling_step_kernel (sampling.hip) carries its own copy of greedy_step_kernel's
// bookkeeping (next RoPE row, token commit, step_epoch, next input row): a change to what is committed in one is a change to
// both.  (How the greedy kernel gets there - the lm_head launch's arg-max partials, the step words loaded at entry - is its own.)
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"

namespace tllm
{
namespace kernels
{
using namespace dev;
using launch_util::check_launch;

namespace
{

// greedy argmax; ties -> lowest index (torch.argmax / top-k=1 of the reference sampler)
__global__ __launch_bounds__(1024) void argmax_kernel(int32_t* out_ids, const float* logits, int32_t vocab)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    const float* l = logits + (int64_t) blockIdx.x * vocab;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < vocab; i += blockDim.x)
    {
        const float v = l[i];
        if (v > best || (v == best && i < bi))
        {
            best = v;
            bi = i;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
    {
        const float ov = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ov > best || (ov == best && oi < bi))
        {
            best = ov;
            bi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0)
    {
        sv[wid] = best;
        si[wid] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 1; w < nw; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bi))
            {
                best = sv[w];
                bi = si[w];
            }
        out_ids[blockIdx.x] = bi == 0x7fffffff ? 0 : bi;
    }
}

// Entry contract (gemv_impl.h): what the first loads are built from leads the parameter list and is preloaded into SGPRs - the
// logits (or the lm_head launch's arg-max partials) and the three step words of the row; the struct trails it for the
// bookkeeping and is first read behind those requests.  launch_greedy_step fills both from the one GreedyParams.
//
// hot_part (batch 1, one vocabulary part): the kArgmaxPairs {value, index} pairs the lm_head launch left, one per wave of its
// grid (GemvParams::argmax_part).  The head had every logit in a register when it wrote it; reducing its 16 KB of pairs - two
// loads per thread - replaces pulling all 128 KB of logits through this one CU's queue.  The rule is the scan's (greater wins,
// ties to the lowest index) and is associative, so the token is the same.  The kernel boundary orders the two launches: no flag,
// no wait.  hot_part null: the scan.
//
// seq_len[b], finished[b] and input_lengths[b] are requested here as well, as raw values (no conversion or compare next to the
// load), and the epoch word right behind the first requests, so that thread 0's commit below contains no load: it used to chase
// seq_len -> finished, two dependent round trips behind the reduction, and then read-modify-write the epoch.  hot_finished /
// hot_input_lengths are never null: the launcher points an absent one at seq_len (loaded, ignored; a RoPE row without
// input_lengths is refused).
__global__ __launch_bounds__(1024) void greedy_step_kernel(const float* const hot_logits, const uint2* const hot_part,
    const int32_t* const hot_seq_len, const int32_t* const hot_finished, const int32_t* const hot_input_lengths, const int hot_batch,
    const int hot_vocab_part, const int hot_nparts, const int hot_vocab, const GreedyParams p)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    const int b = blockIdx.x;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    // raw step words, consumed behind the reduction
    const int sl0 = hot_seq_len[b], fin0 = hot_finished[b], inlen0 = hot_input_lengths[b];
    uint32_t epoch0 = 0; // requested behind the first logits / pairs loads: its pointer is the struct's
    if (hot_part) // uniform, a preloaded scalar
    {
        const uint2 pr[2] = {hot_part[threadIdx.x], hot_part[threadIdx.x + kArgmaxPairs / 2]};
        // unconditional (no branch around a load): an absent epoch word reads a valid word, ignored
        epoch0 = *(p.step_epoch ? p.step_epoch : reinterpret_cast<const uint32_t*>(hot_seq_len));
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            const float v = __uint_as_float(pr[u].x);
            const int id = (int) pr[u].y;
            if (id < hot_vocab && (v > best || (v == best && id < bi)))
            {
                best = v;
                bi = id;
            }
        }
    }
    else
    {
        for (int part = 0; part < hot_nparts; ++part)
        {
            const float* l = hot_logits + ((int64_t) part * hot_batch + b) * hot_vocab_part;
            const int base_id = part * hot_vocab_part;
            if ((hot_vocab_part & 3) == 0 && (reinterpret_cast<uintptr_t>(l) & 15) == 0)
            {
                // 16-byte loads, all of a thread's requests in flight before the compares (latency-bound otherwise)
                constexpr int UNR = 8;
                const int nvec = hot_vocab_part >> 2;
                for (int v0 = threadIdx.x; v0 < nvec; v0 += blockDim.x * UNR)
                {
                    float4 vals[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
                    {
                        const int vi = v0 + u * blockDim.x;
                        vals[u] = vi < nvec ? reinterpret_cast<const float4*>(l)[vi]
                                            : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
                    {
                        const int id0 = base_id + (v0 + u * blockDim.x) * 4;
                        const float f[4] = {vals[u].x, vals[u].y, vals[u].z, vals[u].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                        {
                            const int id = id0 + e;
                            if (id < hot_vocab && (f[e] > best || (f[e] == best && id < bi)))
                            {
                                best = f[e];
                                bi = id;
                            }
                        }
                    }
                }
                continue;
            }
            for (int i = threadIdx.x; i < hot_vocab_part; i += blockDim.x)
            {
                const int id = base_id + i;
                if (id >= hot_vocab)
                    break;
                const float v = l[i];
                if (v > best || (v == best && id < bi))
                {
                    best = v;
                    bi = id;
                }
            }
        }
        epoch0 = *(p.step_epoch ? p.step_epoch : reinterpret_cast<const uint32_t*>(hot_seq_len));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
    {
        const float ov = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ov > best || (ov == best && oi < bi))
        {
            best = ov;
            bi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0)
    {
        sv[wid] = best;
        si[wid] = bi;
    }
    if (p.rope_row_out && threadIdx.x >= 64 && threadIdx.x < 64 + p.rope_half)
    {
        // next step's position: (seq_len after this step's advance) - padding of this sequence
        const int j = threadIdx.x - 64;
        int pos = sl0 + (p.advance ? 1 : 0) - (p.max_input_len - inlen0);
        pos = pos < 0 ? 0 : (pos >= p.rope_table_len ? p.rope_table_len - 1 : pos);
        reinterpret_cast<float2*>(p.rope_row_out)[(int64_t) b * p.rope_half + j]
            = reinterpret_cast<const float2*>(p.rope_table)[(int64_t) pos * p.rope_half + j];
        if (j == 0 && p.rope_pos_out)
            p.rope_pos_out[b] = pos;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 1; w < nw; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bi))
            {
                best = sv[w];
                bi = si[w];
            }
        int id = bi == 0x7fffffff ? 0 : bi;
        int sl = sl0;
        if (p.advance)
        {
            sl += 1;
            p.seq_len[b] = sl;
        }
        if (p.finished)
        {
            if (fin0)
                id = p.end_id;
            else if (p.end_id >= 0 && id == p.end_id)
                p.finished[b] = 1;
        }
        if (sl < p.out_stride)
            p.out_ids[(int64_t) b * p.out_stride + sl] = id;
        p.cur_ids[b] = id;
        si[0] = id;
        if (b == 0 && p.step_epoch)
            *p.step_epoch = epoch0 + 1; // (only this thread of this launch writes the word: the value read at entry is current)
    }
    if (p.emb_table) // uniform: the next step's input row, gathered here instead of by an embedding launch of its own
    {
        __syncthreads();
        const int id = si[0];
        const bool ok = id >= 0 && id < hot_vocab;
        const uint16_t* src = reinterpret_cast<const uint16_t*>(p.emb_table) + (int64_t) (ok ? id : 0) * p.hidden;
        uint16_t* dst = reinterpret_cast<uint16_t*>(p.x_out) + (int64_t) b * p.hidden;
        for (int k = threadIdx.x * 8; k < p.hidden; k += blockDim.x * 8) // hidden % 8 == 0 (checked by the launcher)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(src + k);
            *reinterpret_cast<uint4*>(dst + k) = ok ? v : make_uint4(0, 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Beam search step (see BeamParams in kernels.h).  One workgroup of 1024 threads per batch entry.
// Dynamic LDS: the cache-indirection rows being re-parented, [beam][used slots] int32.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void beam_step_kernel(const BeamParams p)
{
    constexpr int MAXW = 8;
    extern __shared__ int32_t ci_stage[];
    __shared__ float red[32];
    __shared__ int redi[32];
    __shared__ float s_lse[MAXW], s_cum[MAXW], s_score[MAXW];
    __shared__ int s_fin[MAXW], s_idx[MAXW];
    const int b = blockIdx.x, W = p.beam, V = p.vocab, tid = threadIdx.x, bb0 = b * W;
    const int nrows = p.logits_per_batch ? p.batch : p.batch * W;
    auto logit = [&](int k, int v) -> float {
        const int part = v / p.vocab_part, vi = v % p.vocab_part;
        return p.logits[((int64_t) part * nrows + (p.logits_per_batch ? b : bb0 + k)) * p.vocab_part + vi];
    };
    if (tid < W)
    {
        s_cum[tid] = p.cum_log_probs[bb0 + tid];
        s_fin[tid] = p.finished ? p.finished[bb0 + tid] : 0;
    }
    __syncthreads();
    // ---- 1. log-sum-exp of every live hypothesis
    for (int k = 0; k < W; ++k)
    {
        if (s_fin[k]) // uniform
            continue;
        float mx = -INFINITY;
        for (int v = tid; v < V; v += blockDim.x)
            mx = fmaxf(mx, logit(k, v));
        mx = block_max(mx, red);
        float sm = 0.f;
        for (int v = tid; v < V; v += blockDim.x)
            sm += __expf(logit(k, v) - mx);
        sm = block_sum(sm, red);
        if (tid == 0)
            s_lse[k] = mx + __logf(sm);
        __syncthreads();
    }
    // ---- 2. the W best (hypothesis, token) pairs, best first; ties -> lowest k * V + v
    for (int j = 0; j < W; ++j)
    {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        auto consider = [&](float sc, int idx) {
            if (sc > best || (sc == best && idx < bi))
            {
                bool taken = false;
                for (int q = 0; q < j; ++q)
                    taken = taken || s_idx[q] == idx;
                if (!taken)
                {
                    best = sc;
                    bi = idx;
                }
            }
        };
        for (int k = 0; k < W; ++k)
        {
            if (s_fin[k])
            {
                // a finished hypothesis stays as it is: one candidate, end_id, at its score
                if (tid == 0 && p.end_id >= 0)
                    consider(s_cum[k], k * V + p.end_id);
                continue;
            }
            const float base = s_cum[k] - s_lse[k];
            for (int v = tid; v < V; v += blockDim.x)
                consider(logit(k, v) + base, k * V + v);
        }
        // block arg-max
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
        {
            const float ov = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (ov > best || (ov == best && oi < bi))
            {
                best = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if ((tid & 63) == 0)
        {
            red[tid >> 6] = best;
            redi[tid >> 6] = bi;
        }
        __syncthreads();
        if (tid == 0)
        {
            for (int w = 1; w < (int) (blockDim.x >> 6); ++w)
                if (red[w] > best || (red[w] == best && redi[w] < bi))
                {
                    best = red[w];
                    bi = redi[w];
                }
            if (bi == 0x7fffffff) // every remaining candidate is -inf (fewer live candidates than beams): repeat the best
            {
                bi = j > 0 ? s_idx[0] : 0;
                best = j > 0 ? s_score[0] : -INFINITY;
            }
            s_idx[j] = bi;
            s_score[j] = best;
        }
        __syncthreads();
    }
    // ---- 3. re-parent the cache indirection: stage the parents' rows, then write them to the children
    const int sl_old = p.seq_len[bb0];
    const int sl_new = sl_old + (p.advance ? 1 : 0);
    const int used = p.advance ? sl_old : sl_new; // slots whose K/V exist before this step's token: [0, used)
    int32_t* ci = p.cache_indirection;
    if (ci)
    {
        for (int i = tid; i < W * used; i += blockDim.x)
        {
            const int j = i / used, sidx = i % used;
            ci_stage[i] = ci[(int64_t) (bb0 + s_idx[j] / V) * p.out_stride + sidx];
        }
        __syncthreads();
        for (int i = tid; i < W * used; i += blockDim.x)
        {
            const int j = i / used, sidx = i % used;
            ci[(int64_t) (bb0 + j) * p.out_stride + sidx] = ci_stage[i];
        }
        // the token consumed by this step put its K/V into the parent's rows at slot sl_old
        if (p.advance && tid < W && sl_old < p.out_stride)
            ci[(int64_t) (bb0 + tid) * p.out_stride + sl_old] = s_idx[tid] / V;
    }
    // ---- 4. bookkeeping of the new hypotheses
    if (tid < W)
    {
        const int j = tid, parent = s_idx[j] / V, tok = s_idx[j] % V;
        const int fin = s_fin[parent] || (p.end_id >= 0 && tok == p.end_id);
        p.cum_log_probs[bb0 + j] = s_score[j];
        if (p.finished)
            p.finished[bb0 + j] = fin;
        p.seq_len[bb0 + j] = sl_new;
        p.cur_ids[bb0 + j] = tok;
        if (sl_new < p.out_stride)
        {
            p.out_ids[(int64_t) (bb0 + j) * p.out_stride + sl_new] = tok;
            p.parent_ids[(int64_t) (bb0 + j) * p.out_stride + sl_new] = parent;
        }
    }
    if (p.rope_row_out)
    {
        // next step's RoPE row, the same position for every hypothesis of this batch entry
        int pos = sl_new - (p.max_input_len - p.input_lengths[bb0]);
        pos = pos < 0 ? 0 : (pos >= p.rope_table_len ? p.rope_table_len - 1 : pos);
        for (int i = tid; i < W * p.rope_half; i += blockDim.x)
            reinterpret_cast<float2*>(p.rope_row_out)[(int64_t) bb0 * p.rope_half + i]
                = reinterpret_cast<const float2*>(p.rope_table)[(int64_t) pos * p.rope_half + i % p.rope_half];
        if (p.rope_pos_out && tid < W)
            p.rope_pos_out[bb0 + tid] = pos;
    }
}

} // namespace

int launch_greedy_step(const GreedyParams& p, hipStream_t stream)
{
    if (p.batch <= 0)
        return 0;
    if (p.emb_table && (!p.x_out || p.hidden <= 0 || (p.hidden & 7)))
    {
        set_error("greedy step: fused embedding gather needs x_out and hidden %% 8 == 0 (got %d)", p.hidden);
        return -1;
    }
    if (p.rope_row_out && (!p.input_lengths || !p.rope_table))
    {
        set_error("greedy step: the next RoPE row needs input_lengths and the RoPE table");
        return -1;
    }
    if (p.argmax_part && (p.batch != 1 || p.nparts != 1 || (reinterpret_cast<uintptr_t>(p.argmax_part) & 7)))
    {
        set_error("greedy step: arg-max partials serve batch 1 and one vocabulary part (got batch %d, %d parts)", p.batch, p.nparts);
        return -1;
    }
    hipLaunchKernelGGL(greedy_step_kernel, dim3(p.batch), dim3(1024), 0, stream, p.logits, static_cast<const uint2*>(p.argmax_part),
        p.seq_len, p.finished ? p.finished : p.seq_len, p.input_lengths ? p.input_lengths : p.seq_len, p.batch, p.vocab_part, p.nparts,
        p.vocab, p);
    return check_launch("greedy_step");
}

// Teacher forcing (parity tests): replace the token the sampler just chose by ids[b] - the output slot it wrote, the
// step's input id and the embedding row the next step consumes.  One workgroup per sequence.
__global__ __launch_bounds__(256) void force_token_kernel(const int32_t* ids, int32_t* cur_ids, int32_t* out_ids, int32_t out_stride,
    const int32_t* seq_len, const void* emb, void* x, int32_t hidden, int32_t vocab)
{
    const int b = blockIdx.x, id = ids[b];
    if (threadIdx.x == 0)
    {
        const int sl = seq_len[b];
        if (sl < out_stride)
            out_ids[(int64_t) b * out_stride + sl] = id;
        cur_ids[b] = id;
    }
    if (emb && x)
    {
        const bool ok = id >= 0 && id < vocab;
        const uint16_t* src = reinterpret_cast<const uint16_t*>(emb) + (int64_t) (ok ? id : 0) * hidden;
        uint16_t* dst = reinterpret_cast<uint16_t*>(x) + (int64_t) b * hidden;
        for (int k = threadIdx.x; k < hidden; k += blockDim.x)
            dst[k] = ok ? src[k] : (uint16_t) 0;
    }
}

int launch_force_token(const int32_t* ids_dev, int32_t* cur_ids, int32_t* out_ids, int32_t out_stride, const int32_t* seq_len,
    const void* emb, void* x, int32_t batch, int32_t hidden, int32_t vocab, hipStream_t stream)
{
    if (batch <= 0)
        return 0;
    hipLaunchKernelGGL(force_token_kernel, dim3(batch), dim3(256), 0, stream, ids_dev, cur_ids, out_ids, out_stride, seq_len, emb, x,
        hidden, vocab);
    return check_launch("force_token");
}

int launch_beam_step(const BeamParams& p, hipStream_t stream)
{
    if (p.batch <= 0)
        return 0;
    if (p.beam < 1 || p.beam > 8 || !p.cum_log_probs || !p.parent_ids || !p.cache_indirection)
    {
        set_error("beam step: beam width %d out of [1, 8] or missing state buffers", p.beam);
        return -1;
    }
    const size_t smem = (size_t) p.beam * p.out_stride * sizeof(int32_t);
    if (smem > 96 * 1024)
    {
        set_error("beam step: beam %d x %d slots does not fit the staging buffer", p.beam, p.out_stride);
        return -1;
    }
    launch_util::ensure_dynamic_lds(reinterpret_cast<const void*>(beam_step_kernel), 96 * 1024);
    hipLaunchKernelGGL(beam_step_kernel, dim3(p.batch), dim3(1024), smem, stream, p);
    return check_launch("beam_step");
}

int launch_argmax(int32_t* out_ids, const float* logits, int32_t batch, int32_t vocab, hipStream_t stream)
{
    if (batch <= 0)
        return 0;
    hipLaunchKernelGGL(argmax_kernel, dim3(batch), dim3(1024), 0, stream, out_ids, logits, vocab);
    return check_launch("argmax");
}

} // namespace kernels
} // namespace tllm
