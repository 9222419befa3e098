// Decode attention for grouped K/V heads on the matrix pipe ("Grouped K/V heads"): one new token per sequence,
// G = H / Hkv >= 2 query heads per K/V head, head sizes 64 / 128, fp16 / int8 / fp8 cache elements, the linear cache.  The rule is
// mmha_decode.hip's, unchanged - RoPE position timestep - (max_input_len - input_lengths[b]), RoPE on q and the new k from rope_row
// or the table, the new k / v un-quantised in the soft-max, masked_tokens and slots >= the live length at -inf, cache elements as
// the exact fp16 value of their byte with kv_scale_quant_orig once on the score and once on the sum of p.v, fp32 soft-max,
// probabilities rounded to fp16, the append quantised by quant8 / quant8_fp8 - only the summation order differs.  Where
// mmha_partial_kernel runs one workgroup per QUERY head, so that the G heads of a K/V head each request the same cache rows, here
// the G heads are the COLUMNS of an MFMA tile and every cache row is requested once per K/V head (G <= 16) or once per 16 heads.
//
// mmha_gqa_mfma_kernel, grid (splits, Hkv * column tiles, B), 256 threads.  A workgroup serves ONE (split c, K/V head, column tile,
// sequence b): the past slots [c * tchunk, min((c + 1) * tchunk, tl)) of MmhaPlan's split (every tchunk is a multiple of 64, so a
// 64-key block never straddles a split) against columns = query heads kvh * G + 16 * tile + 0 .. 15; G <= 16 is one tile padded
// to 16 columns (a padding column computes on the last real head and is not stored), G > 16 is G / 16 full tiles.
// Instruction: v_mfma_f32_16x16x32_f16, roles as append_attn_split.hip:
//   S^T[key, c]  = K[key, :] . Q^T[:, c]       A = K rows (LDS [64][DH], rows padded by 16 bytes), B = q of head c after RoPE
//                                              (registers, read once from the LDS rows the prologue wrote)
//       -> lane (c = lane & 15, kb = lane >> 4) holds 8 scores of ITS head: tile s, register j = key 32 u + 16 s + 4 kb + j;
//   O^T[d, c]   += V^T[d, keys] . P^T[keys, c] A = V^T rows (LDS [DH][64], rows padded by 16 bytes), B = the 8 score registers
//                                              rounded to fp16 in place (the loader permutes the keys of V^T to match).
// There is one column tile, so the four waves split a 64-key block AND the rows of O^T: wave 2 u + dq scores keys 32 u .. 32 u + 31
// (the two waves of a key half compute the same scores, bit for bit: 2 DH / 32 MFMAs that buy a soft-max with no exchange between
// waves) and accumulates rows d of O^T in tiles dq * DH / 32 .. of 16, with a running (m, l) of its own.  After the last block the
// two key halves merge once through LDS (the operand images are dead), together with the new token.
// Loader (append_attn_split.hip's, linear): K rows and V rows (transposed on the way in) become fp16 in LDS; rows of masked slots
// and of slots >= the live length are written as zeros and score -inf, by clamp-and-select with no branch around a load (every
// load index is clamped below min(split end, tl) <= Smax).  The raw bytes of the NEXT 64-key block (and its mask words) are
// requested into registers right after the current block has been written to LDS: one LDS stage, one register stage.
// The new token: the prologue - under the first block's loads - rotates q of the tile's heads and the new k (LPR lanes per row,
// mmha::rope_row8) into LDS and keeps v; the workgroup whose split owns slot tl (and column tile 0) appends k / v to the cache,
// exactly once per (K/V head, sequence).  In the owning split slot tl itself is >= the live length (a zero row, -inf); the new
// token enters as a partial of its own, m = q . k_new / sqrt(Dh), l = 1, O = v_new, merged with the two key halves.
// Output: the split partial of every real head - {max, sum} and the un-normalised fp32 O[DH] - in MmhaPlan's workspace, per QUERY
// head, so mmha_combine_kernel and the in-launch merge (mmha::tail_merge: one self-resetting ticket per (sequence, column tile) at
// the tile's first head, at most 16 splits, the tail_quant_scale / tail_out_q8 image) serve unchanged.  No spin waits; no memset:
// the launch is captured in the step's hipGraph as it is.
// Refused by name, nothing launched: G = 1, G > 16 with G % 16 != 0, head sizes other than 64 / 128, beam_width > 1, the paged cache.
#include "append_attn_common.h"
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"
#include "mmha_common.h"
#include <type_traits>

namespace tllm
{
namespace kernels
{
using namespace dev;
using namespace append_attn;

namespace
{
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

constexpr int kCols = 16; // query heads of a column tile

template <int DH, int KV>
__global__ __launch_bounds__(256) void mmha_gqa_mfma_kernel(const MmhaParams p, float2* ws_ml, float* ws_o, const int nsplit_max,
    const int tchunk, const int group, const int ntiles)
{
    constexpr int ESZ = KV == 0 ? 2 : 1;
    constexpr int KP = DH * 2 + 16; // bytes per row of the K image (and of a q row)
    constexpr int VP = 64 * 2 + 16; // bytes per row of the V^T image
    constexpr int KT = DH / 32;     // k-steps of a score tile
    constexpr int DT = DH / 32;     // 16-row tiles of O^T a wave owns (half of DH / 16)
    constexpr int LPR = DH / 8, KPP = 256 / LPR, KPASS = 64 / KPP, VPASS = LPR / 4;
    constexpr int QPASS = (kCols + 2 + KPP - 1) / KPP; // prologue passes: 16 q rows, k, v at KPP rows per pass
    constexpr int MREC = DT * 4 + 2;                   // floats a lane hands over in the merge of the key halves: O^T registers, m, l
    static_assert(2 * 64 * MREC * 4 <= 64 * KP + DH * VP, "the merge records fit the operand images");
    typedef typename kv_raw8<KV>::type raw_t;
    __shared__ __attribute__((aligned(16))) char smem[64 * KP + DH * VP];
    __shared__ __attribute__((aligned(16))) char sQ[(kCols + 1) * KP]; // q of the tile's heads after RoPE, row 16: the new k
    __shared__ __attribute__((aligned(16))) uint16_t sVn[DH];         // the new v
    __shared__ int sOk[64];
    char* const sK = smem;
    char* const sV = smem + 64 * KP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, kb = lane >> 4;
    const int dq = wv & 1; // rows of O^T: tiles dq * DT .. dq * DT + DT - 1
    const int u = wv >> 1; // key half: keys 32 u .. 32 u + 31 of every 64-key block
    const int H = p.num_heads, Hkv = p.num_kv_heads, Smax = p.max_seq_len;
    const int c = blockIdx.x, kvh = blockIdx.y / ntiles, tile = blockIdx.y % ntiles, b = blockIdx.z;
    const int ncols = min(group, kCols), h0 = kvh * group + tile * kCols;
    const int tl = p.sequence_length[b]; // slots already used; the new token goes to slot tl
    // splits that hold a used slot or slot tl, as mmha_partial_kernel counts them: a split beyond takes no ticket
    const int nact = min(tl / tchunk + 1, nsplit_max);
    if (c >= nact)
        return; // uniform
    const int kbeg = c * tchunk;
    const int kend = min(kbeg + tchunk, min(tl, Smax));
    const bool own = tl / tchunk == c && tl >= 0 && tl < Smax; // uniform: this split holds slot tl
    char* const kc = reinterpret_cast<char*>(p.kv_cache) + ((((int64_t) b * 2 + 0) * Hkv + kvh) * Smax) * DH * ESZ;
    char* const vc = reinterpret_cast<char*>(p.kv_cache) + ((((int64_t) b * 2 + 1) * Hkv + kvh) * Smax) * DH * ESZ;
    const int32_t* mask = p.masked_tokens ? p.masked_tokens + (int64_t) b * Smax : nullptr;
    float s_oq = 1.f, s_qo = 1.f;
    if constexpr (KV != 0)
    {
        s_oq = p.kv_scale_orig_quant[0];
        s_qo = p.kv_scale_quant_orig[0];
    }
    const float kscale = s_qo * p.inv_sqrt_dh;

    f16x8_t qf[KT];
    float s_new = -INFINITY; // the new token's score against this lane's head (the owning split)
    // ---- the prologue: q of the tile's heads and the new k through RoPE into LDS, the new v beside them, the cache append.  LPR
    //      lanes per row; row r < ncols: head h0 + r, row ncols: k, row ncols + 1: v; further rows repeat v and store nothing
    auto prologue = [&]() __attribute__((always_inline)) {
        const int li = tid % LPR;
        float4 c4[4];
        mmha::rope_coeffs(p, b, tl, li * 8, c4);
        const float cs[16] = {c4[0].x, c4[0].y, c4[0].z, c4[0].w, c4[1].x, c4[1].y, c4[1].z, c4[1].w,
            c4[2].x, c4[2].y, c4[2].z, c4[2].w, c4[3].x, c4[3].y, c4[3].z, c4[3].w};
        const uint16_t* qkv = reinterpret_cast<const uint16_t*>(p.qkv) + (int64_t) b * (H + 2 * Hkv) * DH; // q: H | k: Hkv | v: Hkv
#pragma unroll
        for (int ps = 0; ps < QPASS; ++ps)
        {
            const int r = min(ps * KPP + tid / LPR, ncols + 1);
            const bool live = ps * KPP + tid / LPR <= ncols + 1;
            const int src = r < ncols ? h0 + r : (r == ncols ? H + kvh : H + Hkv + kvh);
            const uint4 raw = *reinterpret_cast<const uint4*>(qkv + (int64_t) src * DH + li * 8);
            const uint4 rot = mmha::rope_row8<LPR>(raw, cs, p.rotary_dim, p.neox, li);
            if (live && r < ncols)
                *reinterpret_cast<uint4*>(sQ + r * KP + li * 16) = rot;
            if (live && r == ncols)
                *reinterpret_cast<uint4*>(sQ + kCols * KP + li * 16) = rot;
            if (live && r == ncols + 1)
                *reinterpret_cast<uint4*>(sVn + li * 8) = raw;
            // the append: the split that owns slot tl, the first column tile - once per (K/V head, sequence)
            if (live && r >= ncols && own && tile == 0)
            {
                const uint4 val = r == ncols ? rot : raw;
                char* const dst = (r == ncols ? kc : vc) + ((int64_t) tl * DH + li * 8) * ESZ;
                if constexpr (KV == 1)
                    *reinterpret_cast<uint2*>(dst) = quant8(val, s_oq);
                else if constexpr (KV == 2)
                    *reinterpret_cast<uint2*>(dst) = quant8_fp8(val, s_oq);
                else
                    *reinterpret_cast<uint4*>(dst) = val;
            }
        }
        __syncthreads();
        const int cq = min(c16, ncols - 1);
        float dn = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t)
        {
            const uint4 q4 = *reinterpret_cast<const uint4*>(sQ + cq * KP + (32 * t + 8 * kb) * 2);
            const uint4 k4 = *reinterpret_cast<const uint4*>(sQ + kCols * KP + (32 * t + 8 * kb) * 2);
            qf[t] = __builtin_bit_cast(f16x8_t, q4);
            dn = dot2(q4.x, k4.x, dn);
            dn = dot2(q4.y, k4.y, dn);
            dn = dot2(q4.z, k4.z, dn);
            dn = dot2(q4.w, k4.w, dn);
        }
        dn += __shfl_xor(dn, 16, 64);
        dn += __shfl_xor(dn, 32, 64);
        if (own)
            s_new = dn * p.inv_sqrt_dh;
    };

    f32x4_t oacc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
        oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // the loader's roles: LPR consecutive lanes fetch one K row; for V lane = key, so a wave writes 64 consecutive halfs of a V^T row
    const int kc8 = tid % LPR, krow = tid / LPR, kl = tid & 63;
    const int vpos = (kl & 0x23) | ((kl & 0x0c) << 1) | ((kl & 0x10) >> 2); // the key's column of V^T (append_attn_split.hip)
    auto keep8 = [](uint4 v, bool live) -> uint4 {
        const uint32_t k = live ? 0xffffffffu : 0u;
        return make_uint4(v.x & k, v.y & k, v.z & k, v.w & k);
    };
    auto store_v = [&](int cc, uint4 v) {
        uint16_t* const col = reinterpret_cast<uint16_t*>(sV + (cc * 8) * VP + vpos * 2);
        constexpr int VPH = VP / 2;
        col[0 * VPH] = (uint16_t) v.x, col[1 * VPH] = (uint16_t) (v.x >> 16);
        col[2 * VPH] = (uint16_t) v.y, col[3 * VPH] = (uint16_t) (v.y >> 16);
        col[4 * VPH] = (uint16_t) v.z, col[5 * VPH] = (uint16_t) (v.z >> 16);
        col[6 * VPH] = (uint16_t) v.w, col[7 * VPH] = (uint16_t) (v.w >> 16);
    };
    // one 64-key block out of LDS: scores of this wave's key half, online soft-max, its rows of O^T += V^T P^T
    auto compute = [&]() __attribute__((always_inline)) {
        f32x4_t sacc[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            sacc[s] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
            {
                const f16x8_t a = *reinterpret_cast<const f16x8_t*>(sK + (32 * u + 16 * s + c16) * KP + (32 * t + 8 * kb) * 2);
                sacc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[t], sacc[s], 0, 0, 0);
            }
        }
        float mt = -INFINITY;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                const bool ok = sOk[32 * u + 16 * s + 4 * kb + j] != 0;
                sacc[s][j] = ok ? sacc[s][j] * kscale : -INFINITY;
                mt = fmaxf(mt, sacc[s][j]);
            }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
        m = mn;
        float lsum = 0.f;
        f16x8_t pf;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                const float pr = (sacc[s][j] == -INFINITY) ? 0.f : __expf(sacc[s][j] - mn);
                lsum += pr;
                pf[4 * s + j] = (_Float16) pr;
            }
        l = l * alpha + lsum; // this lane's keys; the four key groups of a head are summed after the last block
#pragma unroll
        for (int i = 0; i < DT; ++i)
        {
            oacc[i] *= alpha;
            const f16x8_t a = *reinterpret_cast<const f16x8_t*>(sV + (16 * (dq * DT + i) + c16) * VP + (32 * u + 8 * kb) * 2);
            oacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf, oacc[i], 0, 0, 0);
        }
    };
    // the register stage: the raw rows of the block at slot k0, and the mask words of their slots as loaded.  No branch and no use of
    // a loaded value in fetch().  A slot >= kend reads slot kend - 1 instead (kbeg <= kend - 1 < Smax) and a masked slot reads its own
    // bytes; both become zeros on the way into LDS.  HM: the launch has a slot mask (a compile-time copy each, so that the prefetch
    // has no branch)
    raw_t kr[KPASS], vr[VPASS];
    int kmask[KPASS], vmask = 0;
    auto fetch = [&](auto has_mask, int k0) __attribute__((always_inline)) {
        constexpr bool HM = decltype(has_mask)::value;
#pragma unroll
        for (int ps = 0; ps < KPASS; ++ps)
        {
            const int slot = min(k0 + ps * KPP + krow, kend - 1);
            kr[ps] = *reinterpret_cast<const raw_t*>(kc + ((int64_t) slot * DH + kc8 * 8) * ESZ);
            kmask[ps] = 0;
            if constexpr (HM)
                kmask[ps] = mask[slot];
        }
        const int slot = min(k0 + kl, kend - 1);
        vmask = 0;
        if constexpr (HM)
            vmask = mask[slot];
#pragma unroll
        for (int ps = 0; ps < VPASS; ++ps)
            vr[ps] = *reinterpret_cast<const raw_t*>(vc + ((int64_t) slot * DH + ((tid >> 6) + 4 * ps) * 8) * ESZ);
    };
    // the loop over the split's past slots, the first block's rows requested
    auto past_range = [&](auto has_mask) __attribute__((always_inline)) {
        for (int k0 = kbeg; k0 < kend; k0 += 64)
        {
            __syncthreads(); // the previous block's fragment reads are done
#pragma unroll
            for (int ps = 0; ps < KPASS; ++ps)
                *reinterpret_cast<uint4*>(sK + (ps * KPP + krow) * KP + kc8 * 16) = keep8(kv8_to_h8<KV>(kr[ps]), k0 + ps * KPP + krow < kend && kmask[ps] == 0);
            const bool vlive = k0 + kl < kend && vmask == 0;
            if (tid < 64)
                sOk[kl] = vlive ? 1 : 0;
#pragma unroll
            for (int ps = 0; ps < VPASS; ++ps)
                store_v((tid >> 6) + 4 * ps, keep8(kv8_to_h8<KV>(vr[ps]), vlive));
            if (k0 + 64 < kend) // uniform: the next block's loads fly while this one computes
                fetch(has_mask, k0 + 64);
            __syncthreads();
            compute();
        }
    };
    const bool has_past = kbeg < kend; // uniform (false: the split holds slot tl alone)
    if (has_past && mask)
        fetch(std::true_type{}, kbeg);
    else if (has_past)
        fetch(std::false_type{}, kbeg);
    prologue(); // under the first block's loads
    if (has_past && mask)
        past_range(std::true_type{});
    else if (has_past)
        past_range(std::false_type{});

    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if constexpr (KV != 0) // every product of the cache rows carries the dequantisation scale of v, once
    {
#pragma unroll
        for (int i = 0; i < DT; ++i)
            oacc[i] *= s_qo;
    }
    // the two key halves merge through LDS (the operand images are dead): record of lane x of row half dq is float [MREC][64] at
    // dq, so a wave's accesses are contiguous
    __syncthreads();
    float* const rec = reinterpret_cast<float*>(smem) + (dq * MREC) * 64 + lane;
    if (u == 1)
    {
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                rec[(i * 4 + j) * 64] = oacc[i][j];
        rec[(DT * 4) * 64] = m;
        rec[(DT * 4 + 1) * 64] = l;
    }
    __syncthreads();
    const bool tail = p.tail_tickets != nullptr; // uniform
    if (u == 0 && c16 < ncols)
    {
        // key half 0, key half 1 and the new token (m = its score, l = 1, O = v_new) in that order
        const float m1 = rec[(DT * 4) * 64], l1 = rec[(DT * 4 + 1) * 64];
        const float mx = fmaxf(fmaxf(m, m1), s_new);
        const float a0 = (m == -INFINITY) ? 0.f : __expf(m - mx), a1 = (m1 == -INFINITY) ? 0.f : __expf(m1 - mx);
        const float an = (s_new == -INFINITY) ? 0.f : __expf(s_new - mx);
        l = l * a0 + l1 * a1 + an;
        const int64_t pi = ((int64_t) b * H + h0 + c16) * nsplit_max + c;
#pragma unroll
        for (int i = 0; i < DT; ++i)
        {
            const int d0 = 16 * (dq * DT + i) + 4 * kb; // register j of the tile is d = d0 + j
            const uint2 vn = *reinterpret_cast<const uint2*>(sVn + d0);
            const float vf[4] = {h2f((uint16_t) vn.x), h2f((uint16_t) (vn.x >> 16)), h2f((uint16_t) vn.y), h2f((uint16_t) (vn.y >> 16))};
            f32x4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = oacc[i][j] * a0 + rec[(i * 4 + j) * 64] * a1 + an * vf[j];
            float* const dst = ws_o + pi * DH + d0;
            // (in-launch merge: write-through stores, the merging workgroup may sit on another XCD - mmha_decode.hip step 5)
            if (tail)
                asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(o) : "memory");
            else
                *reinterpret_cast<f32x4_t*>(dst) = o;
        }
        if (dq == 0 && kb == 0)
        {
            if (tail) // (m, l) as ONE 8-byte write-through store
                __hip_atomic_store(reinterpret_cast<uint64_t*>(ws_ml + pi),
                    (uint64_t) __float_as_uint(mx) | ((uint64_t) __float_as_uint(l) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                ws_ml[pi] = make_float2(mx, l);
        }
    }
    if (!tail)
        return;
    mmha::tail_merge<DH>(p, ws_ml, ws_o, nsplit_max, p.tail_tickets + b * H + h0, b, h0, ncols, nact);
}

template <int DH>
int launch_gqa_dh(const MmhaParams& p, const MmhaPlan& plan, hipStream_t stream)
{
    const int group = p.num_heads / p.num_kv_heads, ntiles = (group + kCols - 1) / kCols;
    const dim3 grid(plan.nsplit, p.num_kv_heads * ntiles, p.batch);
    float2* ws_ml = reinterpret_cast<float2*>(p.workspace);
    float* ws_o = reinterpret_cast<float*>(reinterpret_cast<char*>(p.workspace) + plan.ml_bytes);
    const int kv = kv_kind(p.kv_dtype);
    if (kv == 0)
        hipLaunchKernelGGL((mmha_gqa_mfma_kernel<DH, 0>), grid, dim3(256), 0, stream, p, ws_ml, ws_o, plan.nsplit, plan.tchunk, group, ntiles);
    else if (kv == 1)
        hipLaunchKernelGGL((mmha_gqa_mfma_kernel<DH, 1>), grid, dim3(256), 0, stream, p, ws_ml, ws_o, plan.nsplit, plan.tchunk, group, ntiles);
    else
        hipLaunchKernelGGL((mmha_gqa_mfma_kernel<DH, 2>), grid, dim3(256), 0, stream, p, ws_ml, ws_o, plan.nsplit, plan.tchunk, group, ntiles);
    if (launch_util::check_launch("grouped decode attention (partials)"))
        return -1;
    return p.tail_tickets ? 0 : launch_mmha_combine(p, plan, stream);
}

} // namespace

const char* mmha_grouped_refusal(int32_t num_heads, int32_t num_kv_heads, int32_t head_size, int32_t beam_width, bool paged)
{
    if (num_kv_heads == 0)
        num_kv_heads = num_heads;
    if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads)
        return "num_kv_heads must divide num_heads";
    const int group = num_heads / num_kv_heads;
    if (group == 1)
        return "num_kv_heads equals num_heads: one query head per K/V head has no columns to share a cache row";
    if (group > kCols && group % kCols)
        return "num_heads / num_kv_heads above 16 must be a multiple of 16";
    if (head_size != 64 && head_size != 128)
        return "head_size must be 64 or 128";
    if (beam_width > 1)
        return "beam_width above 1 is not built";
    if (paged)
        return "block_pointers (the paged cache) is not built";
    return nullptr;
}

int launch_mmha_grouped(const MmhaParams& pin, hipStream_t stream)
{
    MmhaParams p = pin;
    if (mmha_resolve_grouping(p))
        return -1;
    if (const char* why = mmha_grouped_refusal(p.num_heads, p.num_kv_heads, p.head_size, p.beam_width, p.block_pointers != nullptr))
    {
        set_error("grouped decode attention (H %d, Hkv %d, Dh %d, beams %d) refused: %s", p.num_heads, p.num_kv_heads, p.head_size,
            p.beam_width, why);
        return -1;
    }
    if (mmha_check_launch(p))
        return -1;
    const MmhaPlan plan = mmha_plan(p.head_size, p.max_seq_len, p.batch, p.num_heads, p.rows_per_group);
    if (mmha_check_plan(p, plan))
        return -1;
    if (plan.tchunk % 64 || p.batch > 65535 || (int64_t) p.num_kv_heads * ((p.num_heads / p.num_kv_heads + kCols - 1) / kCols) > 65535)
    {
        set_error("grouped decode attention: batch %d or num_kv_heads %d exceeds the grid (or a split of %d slots is no multiple of 64)",
            p.batch, p.num_kv_heads, plan.tchunk);
        return -1;
    }
    return p.head_size == 64 ? launch_gqa_dh<64>(p, plan, stream) : launch_gqa_dh<128>(p, plan, stream);
}

} // namespace kernels
} // namespace tllm
