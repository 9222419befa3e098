// Split-KV append attention (APPEND_ATTN_SPLIT): the attention launch of an append of 1 <= n <= 32 tokens
// per sequence onto a long live cache, head sizes 64 / 128, the linear or the paged cache.  The rule is append_attn.hip's, unchanged - visibility,
// cache elements as the exact fp16 value of their byte, kv_scale_quant_orig once on the score and once on the sum of p.v, fp32
// soft-max, probabilities rounded to fp16, normaliser 1 / (l + 1e-6), one rounding of the result - only the summation order differs.
// Two launches behind launch (a), ordered by the kernel boundary alone (no tickets, flags or waits inside a launch):
//
// 1. append_attn_split_kernel, grid (ranges + 1, Hkv * tile groups, B), 256 threads.  A workgroup serves ONE (sequence b, K/V head,
//    key range): range r < ranges is the past slots [r * chunk, min((r + 1) * chunk, p_b)), scaled by kv_scale_quant_orig; range
//    `ranges` is the sequence's own n_b appended keys, un-quantised from the QKV buffer and causally masked - so the scale never
//    changes inside a workgroup.  Its MFMA columns are the query rows that read the K/V head: column c = g * n_b + i is appended
//    token i of query head kvh * G + g (G = H / Hkv), packed densely, 32 columns to a tile group (grid.y), so a tile may straddle
//    a head boundary and the last one may be partly filled.  Every cache byte of a range is read once per (b, K/V head, tile
//    group), not once per query row.
//    Instruction: v_mfma_f32_16x16x32_f16.  The columns are few (n * G <= 32 in a tile group, 2 .. 8 in a verify pass): a 16-column
//    tile wastes half of what a 32-column tile does at n <= 16, a 64-key block of 32 columns is four 32 x 16 tiles - one per wave -
//    where 32x32x16 would leave two of the four waves without a tile, and the accumulators of a wave are DH / 4 registers.
//    Wave 2 u + ct takes keys 32 u .. 32 u + 31 of every 64-key block against columns 16 ct .. 16 ct + 15 with a running (m, l, O)
//    of its own; the two key halves merge once, through LDS, after the last block.  Roles as append_attn_mfma_kernel:
//      S^T[key, c]  = K[key, :] . Q^T[:, c]      A = K rows (LDS [64][DH], rows padded by 16 bytes), B = Q (registers, loaded once)
//          -> lane (c = lane & 15, kb = lane >> 4) holds 8 scores of ITS column: tile s, register j = key 32 u + 16 s + 4 kb + j;
//             the row maximum and sum are in-register plus the exchanges with lanes ^ 16 and ^ 32;
//      O^T[d, c]   += V^T[d, keys] . P^T[keys, c] A = V^T rows (LDS [DH][64], rows padded by 16 bytes), B = the 8 score registers
//             rounded to fp16 in place: element e is key 16 (e >> 2) + 4 kb + (e & 3), so the loader writes key k of a 32-key
//             half to column 8 ((k >> 2) & 3) + 4 (k >> 4) + (k & 3) of V^T and the A fragment is one 16-byte LDS read.
//    Loader: K rows and V rows (transposed on the way in) become fp16 in LDS; the rows of masked slots and of slots >= p_b are
//    written as zeros and their scores are -inf.  The raw cache bytes of the NEXT 64-key block (and its mask words) are requested
//    into registers right after the current block has been written to LDS, so they are in flight while it computes: one LDS stage,
//    one register stage.  Every load index is clamped below min(range end, p_b) <= Smax.
//    Output per (b, query head, row i, range): m, l and the un-normalised O[DH], fp32, in the workspace.  A range that starts at or
//    behind p_b writes the empty partial (m = -inf, l = 0, O = 0), decided before the first barrier.  A workgroup whose every
//    column is padding (tile group at or behind n_b * G) writes NOTHING: the merge takes rows i >= n_b as zeros without reading
//    a partial, and every (row i < n_b, range) has exactly one workgroup that writes it - the merge never reads an unwritten word.
//    The paged cache (template parameter PG; block_pointers set): only where a past row comes from differs - slot t is row t & (T - 1)
//    of the page block_pointers[(b * 2 + {K 0, V 1}) * max_blocks_per_seq + (t >> lg T)], pages [Hkv, T, Dh] - so every result is the
//    linear instance's bit for bit.  A 64-key block starts at a multiple of 64: it lies inside one page (T >= 64) or spans 64 / T
//    pages, at most 64 K and 64 V entries.  Scheme: the table entries travel ONE STAGE AHEAD of the rows.  Entry threads (tid <
//    128: 64 K, 64 V, NE = max(64 / T, 1) of each live) request the entries of the block AFTER NEXT into a register right behind the
//    row requests of an iteration (the memory counter is in order, so the wait for the rows in front of the LDS writes never
//    includes a table load), so the request flies under compute(); an iteration later they publish the register into an LDS
//    ring of 2 slots x 128 x 8 bytes ahead of the top barrier, and the fetch() behind that barrier forms each row address from an
//    LDS read.  So no row load of block k0 + 64 waits on a table load issued in the same iteration, and the register stage of the
//    rows is exactly the linear instance's.  Only the prologue has a dependent pair (the first block's entries, then its rows); the
//    second block's entries are requested next to the first's.  Two slots, not one: a publication never touches the slot the
//    previous fetch() read, so its place in the iteration is free.  Every page index is clamped to the page of slot
//    min(range end, p_b) - 1, an entry of 0 is replaced by the pool's address before it is published (no address is formed from
//    0), the slots read in that way are >= kend and become zeros on the way into LDS as before, and the chunk range reads no entry.
// 2. append_split_merge_kernel, one wave per row of `out`: M = max_r m_r, l = sum_r l_r e^(m_r - M), O likewise, in range order
//    (deterministic), out = fp16(O / (l + 1e-6)); rows i >= n_b are zeros.
#include "append_attn_common.h"
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"
#include <algorithm>
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

constexpr int kSplitCols = 32; // columns of a tile group

// 8 cache elements at an address made from a block-table entry.  The address is cast to the global address space: through a
// generic pointer the row loads would be flat loads, which count as LDS traffic too - every wait for a fragment read in compute()
// would then wait for the prefetch
template <int KV>
__device__ __forceinline__ typename kv_raw8<KV>::type load_page_raw8(int64_t addr)
{
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
    if constexpr (KV == 0)
    {
        const u32x4_t g = *(const __attribute__((address_space(1))) u32x4_t*) (uintptr_t) addr;
        return make_uint4(g.x, g.y, g.z, g.w);
    }
    else
    {
        const u32x2_t g = *(const __attribute__((address_space(1))) u32x2_t*) (uintptr_t) addr;
        return make_uint2(g.x, g.y);
    }
}

// workspace: O [rows][R][DH] fp32, then (m, l) [rows][R][2]; rows = B * n * H in the order of `out`, R = ranges + 1
template <int DH, int KV, bool PG>
__global__ __launch_bounds__(256) void append_attn_split_kernel(const AppendAttnParams p, const int chunk, const int ranges)
{
    constexpr int ESZ = KV == 0 ? 2 : 1;
    constexpr int KP = DH * 2 + 16; // bytes per row of the K image
    constexpr int VP = 64 * 2 + 16; // bytes per row of the V^T image
    constexpr int KT = DH / 32;     // k-steps of a score tile
    constexpr int DT = DH / 16;     // 16-row tiles of O^T
    constexpr int LPR = DH / 8, KPP = 256 / LPR, KPASS = 64 / KPP, VPASS = LPR / 4;
    constexpr int MREC = DT * 4 + 2; // floats a lane hands over in the merge of the key halves: O^T registers, m, l
    static_assert(2 * 64 * MREC * 4 <= 64 * KP + DH * VP, "the merge records fit the operand images");
    typedef typename kv_raw8<KV>::type raw_t;
    __shared__ __attribute__((aligned(16))) char smem[64 * KP + DH * VP];
    __shared__ int sOk[64];
    int64_t* sEnt = nullptr; // paged: the ring of table entries, 2 slots x (64 K + 64 V)
    if constexpr (PG)
    {
        __shared__ int64_t ent_lds[2 * 128];
        sEnt = ent_lds;
    }
    char* const sK = smem;
    char* const sV = smem + 64 * KP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, kb = lane >> 4;
    const int ct = wv & 1; // column tile: columns 16 ct .. 16 ct + 15 of the tile group
    const int u = wv >> 1; // key half: keys 32 u .. 32 u + 31 of every 64-key block
    const int H = p.num_heads, Hkv = p.num_kv_heads, Smax = p.max_seq_len, n = p.n, G = H / Hkv, R = ranges + 1;
    const int tgs = gridDim.y / Hkv;
    const int r = blockIdx.x, kvh = blockIdx.y / tgs, tg = blockIdx.y % tgs, b = blockIdx.z;
    const int nb = p.n_per_seq ? clampi(p.n_per_seq[b], 0, n) : n;
    const int ncols = nb * G, cbase = tg * kSplitCols;
    if (cbase >= ncols) // padding columns alone (uniform over the workgroup): nothing is written, the merge reads none of it
        return;
    const int pb = clampi(p.sequence_length[b], 0, Smax);
    const bool past = r < ranges; // uniform
    const int64_t kbeg64 = (int64_t) r * chunk;
    const int kbeg = past ? (int) (kbeg64 < Smax ? kbeg64 : Smax) : 0;
    const int64_t rend64 = kbeg64 + chunk; // (64 bits: a forced chunk has no upper bound)
    const int kend = past ? (int) (rend64 < pb ? rend64 : pb) : nb;
    float* const wsO = reinterpret_cast<float*>(p.workspace);
    float* const wsML = wsO + (int64_t) p.batch * n * H * R * DH;
    // the partial of column c < ncols for this range: index of its (row, range) pair
    auto pair_of = [&](int c) -> int64_t {
        const int g = c / nb, i = c - g * nb;
        return (((int64_t) b * n + i) * H + kvh * G + g) * R + r;
    };
    if (past && kbeg >= pb) // an empty range (uniform, before the first barrier): the empty partial of every real column
    {
        for (int x = tid; x < kSplitCols * (DH / 4); x += 256)
        {
            const int c = cbase + x / (DH / 4), piece = x % (DH / 4);
            if (c < ncols)
            {
                const int64_t pr = pair_of(c);
                *reinterpret_cast<float4*>(wsO + pr * DH + piece * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                if (piece == 0)
                    *reinterpret_cast<float2*>(wsML + pr * 2) = make_float2(-INFINITY, 0.f);
            }
        }
        return;
    }
    const int64_t rs = (int64_t) (H + 2 * Hkv) * DH;
    const uint16_t* base = reinterpret_cast<const uint16_t*>(p.qkv) + (int64_t) b * n * rs;
    const uint16_t* kq = base + (int64_t) (H + kvh) * DH;
    const uint16_t* vq = base + (int64_t) (H + Hkv + kvh) * DH;
    const char* kc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 0) * Hkv + kvh) * Smax) * DH * ESZ;
    const char* vc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 1) * Hkv + kvh) * Smax) * DH * ESZ;
    const int32_t* mask = p.masked_tokens ? p.masked_tokens + (int64_t) b * Smax : nullptr;
    const float s_qo = (KV != 0 && past) ? p.kv_scale_quant_orig[0] : 1.f;
    const float kscale = s_qo * p.inv_sqrt_dh;
    // this lane's column; a padding column of a partly filled tile computes on column ncols - 1 and is not stored
    const int col = cbase + 16 * ct + c16;
    const bool active = cbase + 16 * ct < ncols; // uniform over the wave: a wave without a real column only loads
    const int cq = min(col, ncols - 1), qg = cq / nb, qi = cq - qg * nb;
    f16x8_t qf[KT];
    {
        const uint16_t* qrow = base + (int64_t) qi * rs + (int64_t) (kvh * G + qg) * DH + 8 * kb;
#pragma unroll
        for (int t = 0; t < KT; ++t)
            qf[t] = *reinterpret_cast<const f16x8_t*>(qrow + 32 * t);
    }
    f32x4_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        oacc[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // the loader's roles: LPR consecutive lanes fetch one K row; for V lane = key, so a wave writes 64 consecutive halfs of a V^T row
    const int kc8 = tid % LPR, krow = tid / LPR, kl = tid & 63;
    const int vpos = (kl & 0x23) | ((kl & 0x0c) << 1) | ((kl & 0x10) >> 2); // the key's column of V^T (see above)
    // everything below selects on VALUES (a mask on the four words, never a choice between two objects): the register stage
    // stays in registers
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
    // one 64-key block out of LDS: scores, online soft-max, O^T += V^T P^T
    auto compute = [&]() {
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
                const int key = 32 * u + 16 * s + 4 * kb + j;
                const bool ok = past ? sOk[key] != 0 : key <= qi; // (the chunk: qi < n_b, so a visible key is a real one)
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
        l = l * alpha + lsum; // this lane's keys; the four key groups of a column are summed after the last block
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
        {
            oacc[dt] *= alpha;
            const f16x8_t a = *reinterpret_cast<const f16x8_t*>(sV + (16 * dt + c16) * VP + (32 * u + 8 * kb) * 2);
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf, oacc[dt], 0, 0, 0);
        }
    };

    // paged: entry thread tid < 128 owns entry e = tid & 63 < NE = max(64 / T, 1) of the K (tid < 64) or V row of the table for
    // the 64-key block at slot k0 - the page of slot k0 + e * T, clamped to the page of slot kend - 1 (kend <= p_b <= Smax <=
    // max_blocks_per_seq * T: inside the sequence's row).  An entry of 0 becomes the pool's own address: a select, never 0 + offset
    const int pg_T = PG ? p.tokens_per_block : 1, pg_lg = PG ? 31 - __builtin_clz(pg_T) : 0;
    const bool is_ent = PG && tid < 128 && (tid & 63) < max(64 >> pg_lg, 1);
    auto pg_entry = [&](int k0) -> int64_t {
        const int j = min((k0 >> pg_lg) + (tid & 63), (kend - 1) >> pg_lg);
        return p.block_pointers[((int64_t) b * 2 + (tid >> 6)) * p.max_blocks_per_seq + j]; // (as loaded: the select waits for it)
    };
    // the loop over a past range; HM: the launch has a slot mask (a compile-time copy each, so that the prefetch has no branch)
    auto past_range = [&](auto has_mask) {
        constexpr bool HM = decltype(has_mask)::value;
        raw_t kr[KPASS], vr[VPASS];
        int kmask[KPASS], vmask = 0;
        // the raw rows of the block at slot k0 into registers, and the mask words of their slots as loaded.  No branch and no use of
        // a loaded value here - what a row means is decided when the block is written to LDS - so nothing waits for a load before
        // the block in LDS has been computed.  A slot >= kend reads slot kend - 1 instead (kend <= p_b <= Smax) and a masked slot
        // reads its own bytes (they are the cache's); both become zeros on the way into LDS
        // paged: `ents` is the ring slot that holds the block's table entries (K 0 .. 63, V 64 .. 127), entry e for the page of slot
        // k0 + e * T; a row's address is an LDS read away, never a table load away
        auto fetch = [&](int k0, const int64_t* ents) {
            const int pg0 = k0 >> pg_lg;
#pragma unroll
            for (int ps = 0; ps < KPASS; ++ps)
            {
                const int slot = min(k0 + ps * KPP + krow, kend - 1); // (a non-empty range: kend - 1 >= kbeg >= 0)
                if constexpr (PG)
                    kr[ps] = load_page_raw8<KV>(ents[(slot >> pg_lg) - pg0]
                        + (((int64_t) kvh * pg_T + (slot & (pg_T - 1))) * DH + kc8 * 8) * ESZ);
                else
                    kr[ps] = *reinterpret_cast<const raw_t*>(kc + ((int64_t) slot * DH + kc8 * 8) * ESZ);
                kmask[ps] = 0;
                if constexpr (HM)
                    kmask[ps] = mask[slot];
            }
            const int slot = min(k0 + kl, kend - 1);
            vmask = 0;
            if constexpr (HM)
                vmask = mask[slot];
            if constexpr (PG)
            {
                const int64_t vrow = ents[64 + (slot >> pg_lg) - pg0] + ((int64_t) kvh * pg_T + (slot & (pg_T - 1))) * DH * ESZ;
#pragma unroll
                for (int ps = 0; ps < VPASS; ++ps)
                    vr[ps] = load_page_raw8<KV>(vrow + (((tid >> 6) + 4 * ps) * 8) * ESZ);
            }
            else
            {
#pragma unroll
                for (int ps = 0; ps < VPASS; ++ps)
                    vr[ps] = *reinterpret_cast<const raw_t*>(vc + ((int64_t) slot * DH + ((tid >> 6) + 4 * ps) * 8) * ESZ);
            }
        };
        int64_t pg_next = 0;
        if constexpr (PG)
        {
            // the first block's entries directly, and the second block's behind them: the one dependent load of a workgroup
            if (is_ent)
            {
                const int64_t e0 = pg_entry(kbeg);
                if (kbeg + 64 < kend)
                    pg_next = pg_entry(kbeg + 64);
                sEnt[tid] = e0 ? e0 : reinterpret_cast<int64_t>(p.kv_cache);
            }
            __syncthreads();
        }
        fetch(kbeg, sEnt);
        for (int k0 = kbeg; k0 < kend; k0 += 64)
        {
            int64_t* const ents_next = PG ? sEnt + ((((k0 - kbeg) >> 6) + 1) & 1) * 128 : nullptr;
            if constexpr (PG)
            {
                // the entries of block k0 + 64, requested an iteration ago, ahead of the barrier that precedes their fetch; the slot
                // was last read by the fetch of block k0 - 64, two barriers back
                if (is_ent && k0 + 64 < kend)
                    ents_next[tid] = pg_next ? pg_next : reinterpret_cast<int64_t>(p.kv_cache);
            }
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
                fetch(k0 + 64, ents_next);
            if constexpr (PG)
            {
                // the entries of the block after next, BEHIND the row requests (the memory counter is in order: a wait for the
                // rows never includes this load) and unused until the publication above: in flight under compute()
                if (is_ent && k0 + 128 < kend)
                    pg_next = pg_entry(k0 + 128);
            }
            __syncthreads();
            if (active)
                compute();
        }
    };
    if (past)
    {
        if (mask)
            past_range(std::true_type{});
        else
            past_range(std::false_type{});
    }
    else
    {
        // the chunk's own keys 0 .. n_b - 1 (<= 32: one block), from the QKV buffer after launch (a); rows >= n_b are zeros
#pragma unroll
        for (int ps = 0; ps < KPASS; ++ps)
        {
            const int key = ps * KPP + krow;
            uint4 k4 = make_uint4(0, 0, 0, 0);
            if (key < nb)
                k4 = *reinterpret_cast<const uint4*>(kq + (int64_t) key * rs + kc8 * 8);
            *reinterpret_cast<uint4*>(sK + key * KP + kc8 * 16) = k4;
        }
#pragma unroll
        for (int ps = 0; ps < VPASS; ++ps)
        {
            const int cc = (tid >> 6) + 4 * ps;
            uint4 v4 = make_uint4(0, 0, 0, 0);
            if (kl < nb)
                v4 = *reinterpret_cast<const uint4*>(vq + (int64_t) kl * rs + cc * 8);
            store_v(cc, v4);
        }
        __syncthreads();
        if (active)
            compute();
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (KV != 0 && past) // every product of a past range carries the dequantisation scale of v, once
    {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            oacc[dt] *= s_qo;
    }
    // the two key halves of a column tile merge through LDS (the operand images are dead): record of lane x of tile ct is float
    // [MREC][64] at tile ct, so a wave's accesses are contiguous
    __syncthreads();
    float* const rec = reinterpret_cast<float*>(smem) + (ct * MREC) * 64 + lane;
    if (u == 1 && active)
    {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                rec[(dt * 4 + j) * 64] = oacc[dt][j];
        rec[(DT * 4) * 64] = m;
        rec[(DT * 4 + 1) * 64] = l;
    }
    __syncthreads();
    if (u == 1 || !active || col >= ncols)
        return;
    {
        const float m1 = rec[(DT * 4) * 64], l1 = rec[(DT * 4 + 1) * 64];
        const float mx = fmaxf(m, m1);
        const float a0 = (m == -INFINITY) ? 0.f : __expf(m - mx), a1 = (m1 == -INFINITY) ? 0.f : __expf(m1 - mx);
        l = l * a0 + l1 * a1;
        m = mx;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                oacc[dt][j] = oacc[dt][j] * a0 + rec[(dt * 4 + j) * 64] * a1;
    }
    const int64_t pr = pair_of(col);
    float* const orow = wsO + pr * DH + 4 * kb; // register j of tile dt is d = 16 dt + 4 kb + j
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<float4*>(orow + 16 * dt) = make_float4(oacc[dt][0], oacc[dt][1], oacc[dt][2], oacc[dt][3]);
    if (kb == 0)
        *reinterpret_cast<float2*>(wsML + pr * 2) = make_float2(m, l);
}

// grid ceil(B * n * H / 4), 256 threads: one wave per row of `out`, lane x owns elements DH / 64 * x ..
template <int DH>
__global__ __launch_bounds__(256) void append_split_merge_kernel(const AppendAttnParams p, const int ranges)
{
    constexpr int EPT = DH / 64;
    const int lane = threadIdx.x & 63, n = p.n, H = p.num_heads, R = ranges + 1;
    const int64_t rows = (int64_t) p.batch * n * H, row = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows)
        return;
    const int i = (int) ((row / H) % n), b = (int) (row / ((int64_t) H * n));
    const int nb = p.n_per_seq ? clampi(p.n_per_seq[b], 0, n) : n;
    uint16_t* const out = reinterpret_cast<uint16_t*>(p.out) + row * DH + lane * EPT;
    float o[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        o[e] = 0.f;
    float inv = 0.f;
    if (i < nb) // a padding row is zeros and reads no partial (none was written for it)
    {
        const float* const wsO = reinterpret_cast<const float*>(p.workspace);
        const float* const ml = wsO + rows * R * DH + row * R * 2;
        const float* const orow = wsO + row * R * DH + lane * EPT;
        float M = -INFINITY, l = 0.f;
        for (int r = 0; r < R; ++r)
            M = fmaxf(M, ml[2 * r]);
        for (int r = 0; r < R; ++r) // fixed order: two runs give the same bits
        {
            const float mr = ml[2 * r];
            const float w = (mr == -INFINITY) ? 0.f : __expf(mr - M);
            l += ml[2 * r + 1] * w;
#pragma unroll
            for (int e = 0; e < EPT; ++e)
                o[e] += orow[(int64_t) r * DH + e] * w;
        }
        inv = 1.f / (l + 1.e-6f);
    }
    if constexpr (EPT == 2)
        *reinterpret_cast<uint32_t*>(out) = pack_h2(o[0] * inv, o[1] * inv);
    else
        *out = f2h(o[0] * inv);
}

template <int DH, bool PG>
int launch_split_dh(const AppendAttnParams& p, const AppendSplitPlan& plan, hipStream_t stream)
{
    const dim3 grid(plan.ranges + 1, p.num_kv_heads * plan.tile_groups, p.batch);
    const int kv = kv_kind(p.kv_dtype);
    if (kv == 0)
        hipLaunchKernelGGL((append_attn_split_kernel<DH, 0, PG>), grid, dim3(256), 0, stream, p, plan.chunk, plan.ranges);
    else if (kv == 1)
        hipLaunchKernelGGL((append_attn_split_kernel<DH, 1, PG>), grid, dim3(256), 0, stream, p, plan.chunk, plan.ranges);
    else
        hipLaunchKernelGGL((append_attn_split_kernel<DH, 2, PG>), grid, dim3(256), 0, stream, p, plan.chunk, plan.ranges);
    if (launch_util::check_launch("append attention (split-KV partials)"))
        return -1;
    const int64_t rows = (int64_t) p.batch * p.n * p.num_heads;
    hipLaunchKernelGGL((append_split_merge_kernel<DH>), dim3((unsigned) ((rows + 3) / 4)), dim3(256), 0, stream, p, plan.ranges);
    return launch_util::check_launch("append attention (split-KV merge)");
}

} // namespace

AppendSplitPlan append_split_plan(int32_t head_size, int32_t n, int32_t batch, int32_t num_heads, int32_t num_kv_heads,
    int32_t max_keys, int32_t cus, int32_t forced_chunk)
{
    AppendSplitPlan plan;
    if (num_kv_heads == 0)
        num_kv_heads = num_heads;
    if (head_size != 64 && head_size != 128)
        plan.refused = "the split-KV kernel needs head size 64 or 128";
    else if (n < 1 || n > 32)
        plan.refused = "the split-KV kernel needs 1 <= n <= 32";
    else if (batch < 1 || batch > 65535 || num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0 || max_keys < 0)
        plan.refused = "bad shape (batch, num_heads, num_kv_heads, max_keys)";
    else if (forced_chunk < 0 || forced_chunk % 64 != 0)
        plan.refused = "split_chunk is not a positive multiple of 64 (or 0 for the plan's)";
    if (plan.refused)
        return plan;
    const int64_t cols = (int64_t) n * (num_heads / num_kv_heads);
    const int64_t tgs = (cols + kSplitCols - 1) / kSplitCols;
    if (num_kv_heads * tgs > 65535)
    {
        plan.refused = "num_kv_heads * tile groups exceeds the grid";
        return plan;
    }
    int64_t chunk = forced_chunk;
    if (chunk == 0)
    {
        if (cus <= 0)
            cus = 256;
        // ranges that fill the CUs once next to the other grid dimensions, at most 64
        const int64_t others = (int64_t) num_kv_heads * tgs * batch;
        const int64_t want = std::min<int64_t>(64, std::max<int64_t>(1, cus / others));
        chunk = std::max<int64_t>(128, ((max_keys + want - 1) / want + 63) / 64 * 64);
    }
    plan.chunk = (int32_t) chunk;
    plan.ranges = (int32_t) ((max_keys + chunk - 1) / chunk);
    plan.tile_groups = (int32_t) tgs;
    plan.workspace_bytes = (int64_t) batch * n * num_heads * (plan.ranges + 1) * (head_size + 2) * 4;
    return plan;
}

int64_t append_split_workspace_max(int32_t head_size, int32_t max_n, int32_t batch, int32_t num_heads, int32_t num_kv_heads,
    int32_t max_seq_len, int32_t cus)
{
    if (num_kv_heads == 0)
        num_kv_heads = num_heads;
    if (cus <= 0)
        cus = 256;
    // one tile group is the finest case: want = min(64, cus / (Hkv * B)), chunk >= max(128, max_keys / want), so ranges <= want
    // and ranges <= ceil(max_keys / 128)
    const int64_t want = std::min<int64_t>(64, std::max<int64_t>(1, cus / ((int64_t) num_kv_heads * batch)));
    const int64_t ranges = std::min<int64_t>(want, ((int64_t) max_seq_len + 127) / 128);
    return (int64_t) batch * max_n * num_heads * (ranges + 1) * (head_size + 2) * 4;
}

namespace append_attn
{
int launch_append_attn_split(const AppendAttnParams& p, const AppendSplitPlan& plan, hipStream_t stream)
{
    if (p.block_pointers) // the paged instances (the table has been checked by launch_append_attention)
        return p.head_size == 64 ? launch_split_dh<64, true>(p, plan, stream) : launch_split_dh<128, true>(p, plan, stream);
    return p.head_size == 64 ? launch_split_dh<64, false>(p, plan, stream) : launch_split_dh<128, false>(p, plan, stream);
}
} // namespace append_attn

} // namespace kernels
} // namespace tllm
