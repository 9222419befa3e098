// What the decode attention kernels share (mmha_decode.hip: one lane group per cache row, v_dot2; mmha_gqa_mfma.hip: the query heads
// of a K/V head as MFMA columns): the RoPE of one row of the new token and the in-launch merge of the split partials.
#pragma once
#include "dev_utils.h"
#include "kernels.h"

namespace tllm
{
namespace kernels
{
namespace mmha
{
using namespace dev;

// RoPE coefficients (cos, sin) of the 8 elements d0 .. d0 + 7 of a row of sequence b: one row of the table (or the row the sampler
// prepared for this step), as 16-byte loads.  NeoX pairs (d, d + rot/2) share coefficient d mod rot/2; GPT-J pairs (2i, 2i+1)
// share coefficient i.  tl: the slots the sequence has used (its position when the host passed no time step).
__device__ __forceinline__ void rope_coeffs(const MmhaParams& p, int b, int tl, int d0, float4 (&c4)[4])
{
    c4[0] = c4[1] = c4[2] = c4[3] = make_float4(1.f, 0.f, 1.f, 0.f);
    if (p.rotary_dim > 0) // uniform
    {
        const int half = p.rotary_dim >> 1;
        const float2* row;
        if (p.rope_row) // uniform: prepared by the sampler for this step
            row = reinterpret_cast<const float2*>(p.rope_row) + (int64_t) b * half;
        else
        {
            const int ts = p.timestep_host >= 0 ? p.timestep_host : tl;
            int pos = ts - (p.max_input_len - p.input_lengths[b]);
            pos = pos < 0 ? 0 : (pos >= p.rope_table_len ? p.rope_table_len - 1 : pos);
            row = reinterpret_cast<const float2*>(p.rope_table) + (int64_t) pos * half;
        }
        int idx0 = p.neox ? (d0 >= half ? d0 - half : d0) : (d0 >> 1);
        const int span = p.neox ? 8 : 4;
        idx0 = idx0 + span <= half ? idx0 : (half >= span ? half - span : 0);
        const float4* r4 = reinterpret_cast<const float4*>(row + idx0);
        c4[0] = r4[0];
        c4[1] = r4[1];
        if (p.neox)
        {
            c4[2] = r4[2];
            c4[3] = r4[3];
        }
    }
}

// RoPE of 8 elements of one row (q of a head, or the new k), fp32 -> fp16.  LPR = head_size / 8 consecutive lanes hold the row, lane
// li of them elements 8 li .. 8 li + 7; cs = the lane's coefficients (rope_coeffs).  Every lane of the row calls it together.
template <int LPR>
__device__ __forceinline__ uint4 rope_row8(const uint4& raw, const float (&cs)[16], int rotary_dim, int neox, int li)
{
    float xf[8];
    h8_to_f(raw, xf);
    if (rotary_dim > 0)
    {
        if (neox)
        {
            // pair (j, j + rot/2); rot == DH: the partner sits in lane li ^ (LPR/2)
            const bool second = li >= LPR / 2;
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                const float xp = __shfl_xor(xf[j], LPR / 2, 64);
                // first half:  x' = x cos - y sin ; second half: y' = y cos + x sin
                // fp16 rounding of the rotated value (...Utils.h:1517-1531)
                const float c = cs[2 * j], sn = second ? cs[2 * j + 1] : -cs[2 * j + 1];
                xf[j] = h2f(f2h(c * xf[j] + sn * xp));
            }
        }
        else
        {
            // GPT-J style: pair (2i, 2i+1), both in this lane
#pragma unroll
            for (int j = 0; j < 8; j += 2)
            {
                const float c = (li * 8 + j < rotary_dim) ? cs[j] : 1.f;
                const float sn = (li * 8 + j < rotary_dim) ? cs[j + 1] : 0.f;
                const float x0 = xf[j], x1 = xf[j + 1];
                xf[j] = h2f(f2h(c * x0 - sn * x1));
                xf[j + 1] = h2f(f2h(c * x1 + sn * x0));
            }
        }
    }
    return f_to_h8(xf);
}

// The in-launch merge of the split partials (MmhaParams::tail_tickets), called by every thread of a 256-thread workgroup behind its
// write-through partials: the stores are drained by every storing wave (vmcnt(0) in asm: the compiler may drop its own wait), a
// workgroup barrier, one relaxed agent-scope ticket on `ticket`; the LAST of the nact workgroups that share the word re-arms it for
// the next launch (ordered by the kernel boundary) and merges heads h0 .. h0 + nheads - 1 of sequence b: the partials are read with
// agent-scope (L1-bypassing) loads behind the ticket, merged in slot order in fp32 (the arithmetic of the O-projection's merge
// prologue, gemv_impl.h PK_ATTN: bit-identical results), and `out` (and, with tail_out_q8, its static int8 image) is written.
// Up to kMmhaTailSlots partials.  No waits: a workgroup that is not the last returns.
template <int DH>
__device__ __forceinline__ void tail_merge(const MmhaParams& p, const float2* ws_ml, const float* ws_o, int nsplit_max, uint32_t* ticket,
    int b, int h0, int nheads, int nact)
{
    constexpr int kTailSlots = kMmhaTailSlots;
    const int tid = threadIdx.x, H = p.num_heads;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ uint32_t sm_ticket;
    if (tid == 0)
        sm_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if ((int) sm_ticket != nact - 1)
        return;
    if (tid == 0) // re-arm for the next launch (ordered by the kernel boundary)
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int e = tid; e < nheads * DH; e += 256)
    {
        const int h = h0 + e / DH, d = e % DH;
        const int64_t base = ((int64_t) b * H + h) * nsplit_max;
        float ms[kTailSlots], ls[kTailSlots], os[kTailSlots];
#pragma unroll
        for (int i = 0; i < kTailSlots; ++i)
        {
            const int ic = i < nact ? i : 0;
            const uint64_t mlb = __hip_atomic_load(reinterpret_cast<const uint64_t*>(ws_ml + base + ic), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ms[i] = __uint_as_float((uint32_t) mlb);
            ls[i] = __uint_as_float((uint32_t) (mlb >> 32));
            os[i] = __hip_atomic_load(ws_o + (base + ic) * DH + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        float Mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kTailSlots; ++i)
            Mx = i < nact ? fmaxf(Mx, ms[i]) : Mx;
        float Lt = 0.f, Ot = 0.f;
#pragma unroll
        for (int i = 0; i < kTailSlots; ++i)
        {
            const bool act = i < nact && ms[i] != -INFINITY;
            const float e = act ? __expf(ms[i] - Mx) : 0.f;
            Lt += act ? ls[i] * e : 0.f;
            Ot += act ? os[i] * e : 0.f;
        }
        const uint16_t h16 = f2h(Ot * (1.f / (Lt + 1.e-6f)));
        const int64_t o = ((int64_t) b * H + h) * DH + d;
        reinterpret_cast<uint16_t*>(p.out)[o] = h16;
        if (p.tail_out_q8)
            reinterpret_cast<int8_t*>(p.tail_out_q8)[o] = f2i8_rni_sat(h2f(h16) * p.tail_quant_scale[0]);
    }
}

} // namespace mmha
} // namespace kernels
} // namespace tllm
