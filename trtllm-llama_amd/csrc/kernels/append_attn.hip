// Append attention: n new tokens per sequence onto a live KV cache - the parallel form of n decode steps.
//
// Sequence b has p_b = sequence_length[b] cache slots in use.  Appended token i goes to slot p_b + i, its rotary position is
// p_b + i - (max_input_len - input_lengths[b]), and its query sees every unmasked slot < p_b plus the appended tokens 0 .. i.
// Launches (ordered by the kernel boundary alone - no flags, tickets or waits inside a launch):
//   (a) append_rope_kv_kernel   RoPE on q and k of the n rows in place in the fused QKV buffer; k and v to the cache slots
//                               p_b + i by the store rule of the cache type (dev_utils.h quant8 / quant8_fp8), once per K/V head;
//   (b) append_attn_mfma_kernel flash-style, head sizes 64 / 128, n >= 16: 64 queries per workgroup, online soft-max over 64-key
//                               blocks - first the past blocks from the cache, then the chunk's blocks from the QKV buffer;
//   (c) append_attn_wave_kernel one wave per query: every n, head sizes 32 / 64 / 128 / 256;
//   (d) append_advance_kernel   sequence_length[b] += n, finished[b] = 0 (the session's bookkeeping, a launch of its own).
// A different number of tokens per sequence (n_per_seq, device [B]; null = n for all): sequence b appends n_b = n_per_seq[b]
// clamped into [0, n], n stays the row stride of the QKV buffer and of `out`, and the rule above holds with n_b in place of n.  Rows
// i >= n_b are padding: (a) leaves them alone (no RoPE, no cache store - their bits in the QKV buffer stay), (b) and (c) write
// their `out` rows as zeros and never load them - not as a query, not as a key, not as a value - and (d) adds n_b.
// The paged cache (block_pointers set; kernels.h): (a), (b) and (c) each have a paged instance - template parameter PG - that differs
// from the linear one in address formation alone: slot t is row t % T of the sequence's block t / T, blocks [Hkv, T, Dh].  Same
// arithmetic in the same order, so every result is the linear launch's bit for bit.  A table entry of 0 (a block not mapped): (a)
// skips the store, no load address is ever formed from it, and the slots it stands for (>= p_b) never enter a product.
// Numerics, both attention kernels: past slots are read as the decode kernel reads them - a one-byte element becomes the exact
// fp16 value of its byte, kv_scale_quant_orig is applied once to the score and once to the sum of p.v; the appended tokens' own
// k and v enter un-quantised from the QKV buffer (as the prefill does for the prompt and decode for the current token).  Scores,
// soft-max and accumulation in fp32, probabilities rounded to fp16, normaliser 1 / (l + 1e-6), one rounding of the result to fp16.
// Every load index is clamped or predicated and every cache store is guarded by slot < Smax: a wrong length on the device can give
// wrong numbers, never an access outside the cache, the QKV buffer or `out`.  Keys that are masked or beyond a length are never
// multiplied in (their V rows enter as zero), so what such slots hold - NaN included - does not reach the result.
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"

namespace tllm
{
namespace kernels
{
using namespace dev;

namespace
{

__device__ __forceinline__ int clampi(int v, int lo, int hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// cache element kinds of the instances: 0 fp16, 1 int8, 2 fp8 (E4M3)
constexpr int kv_kind(int32_t kv_dtype)
{
    return kv_dtype == DT_INT8 ? 1 : (kv_dtype == DT_FP8 ? 2 : 0);
}

// 8 cache elements -> 8 fp16: the value of the byte itself for the one-byte types (exact; the scale is applied by the caller)
template <int KV>
__device__ __forceinline__ uint4 load_kv8(const char* ptr)
{
    if constexpr (KV == 0)
        return *reinterpret_cast<const uint4*>(ptr);
    else
    {
        const uint2 q = *reinterpret_cast<const uint2*>(ptr);
        if constexpr (KV == 2)
            return dequant8_fp8(q);
        else
        {
            float f[8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                f[j] = (float) (int8_t) (q.x >> (8 * j));
                f[4 + j] = (float) (int8_t) (q.y >> (8 * j));
            }
            return f_to_h8(f);
        }
    }
}

// ---- (a) grid (n, ceil(H / HG), B), 256 threads: DH / 8 lanes own the 8-element pieces of one head of one appended token
template <int DH, bool PG>
__global__ __launch_bounds__(256) void append_rope_kv_kernel(const AppendAttnParams p)
{
    constexpr int LPR = DH / 8, HG = 256 / LPR;
    const int i = blockIdx.x, h = blockIdx.y * HG + threadIdx.x / LPR, b = blockIdx.z;
    if (h >= p.num_heads) // whole lane groups (the shuffles stay inside a group)
        return;
    if (p.n_per_seq && i >= clampi(p.n_per_seq[b], 0, p.n)) // a padding row (uniform over the workgroup)
        return;
    const int li = threadIdx.x % LPR;
    const int H = p.num_heads, Hkv = p.num_kv_heads, Smax = p.max_seq_len;
    const bool has_kv = h < Hkv; // the row of query head h < Hkv also carries K/V head h
    const int pb = clampi(p.sequence_length[b], 0, Smax);
    const int slot = pb + i;
    uint16_t* row = reinterpret_cast<uint16_t*>(p.qkv) + ((int64_t) b * p.n + i) * ((int64_t) (H + 2 * Hkv) * DH);
    uint16_t* qp = row + (int64_t) h * DH + li * 8;
    uint16_t* kp = row + (int64_t) (H + (has_kv ? h : 0)) * DH + li * 8;
    const uint16_t* vp = row + (int64_t) (H + Hkv + (has_kv ? h : 0)) * DH + li * 8;
    uint4 q4 = *reinterpret_cast<const uint4*>(qp);
    uint4 k4 = make_uint4(0, 0, 0, 0), v4 = make_uint4(0, 0, 0, 0);
    if (has_kv)
    {
        k4 = *reinterpret_cast<const uint4*>(kp);
        v4 = *reinterpret_cast<const uint4*>(vp);
    }
    if (p.rotary_dim > 0)
    {
        float qf[8], kf[8];
        h8_to_f(q4, qf);
        h8_to_f(k4, kf);
        const int half = p.rotary_dim >> 1;
        const int pos = clampi(slot - (p.max_input_len - p.input_lengths[b]), 0, p.rope_table_len - 1);
        const float2* tab = reinterpret_cast<const float2*>(p.rope_table) + (int64_t) pos * half;
        if (p.neox) // rotary_dim == DH (the launcher's check): pair (d, d + DH / 2), the partner sits in lane li ^ (LPR / 2)
        {
            float qo[8], ko[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                qo[j] = __shfl_xor(qf[j], LPR / 2, 64);
                ko[j] = __shfl_xor(kf[j], LPR / 2, 64);
            }
            const bool second = li >= LPR / 2;
#pragma unroll
            for (int j = 0; j < 8; ++j)
            {
                const int d = li * 8 + j;
                const float2 cs = tab[second ? d - half : d];
                const float sn = second ? cs.y : -cs.y;
                qf[j] = cs.x * qf[j] + sn * qo[j];
                kf[j] = cs.x * kf[j] + sn * ko[j];
            }
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 8; j += 2)
            {
                const int d = li * 8 + j;
                if (d < p.rotary_dim)
                {
                    const float2 cs = tab[d >> 1];
                    const float q0 = qf[j], q1 = qf[j + 1], k0 = kf[j], k1 = kf[j + 1];
                    qf[j] = cs.x * q0 - cs.y * q1;
                    qf[j + 1] = cs.x * q1 + cs.y * q0;
                    kf[j] = cs.x * k0 - cs.y * k1;
                    kf[j + 1] = cs.x * k1 + cs.y * k0;
                }
            }
        }
        q4 = f_to_h8(qf);
        k4 = f_to_h8(kf);
    }
    *reinterpret_cast<uint4*>(qp) = q4;
    if (!has_kv)
        return;
    *reinterpret_cast<uint4*>(kp) = k4;
    if (slot >= Smax)
        return;
    const int esz = p.kv_dtype == DT_HALF ? 2 : 1;
    char* kc = reinterpret_cast<char*>(p.kv_cache) + ((((int64_t) b * 2 + 0) * Hkv + h) * Smax + slot) * DH * esz + li * 8 * esz;
    char* vc = reinterpret_cast<char*>(p.kv_cache) + ((((int64_t) b * 2 + 1) * Hkv + h) * Smax + slot) * DH * esz + li * 8 * esz;
    if constexpr (PG)
    {
        // the sequence's OWN block of slot p_b + i (slot < Smax <= max_blocks_per_seq * T: the index stays inside its row of the
        // table).  An entry of 0 is a block the caller has not mapped: the store is skipped, never aimed at 0 + offset
        const int T = p.tokens_per_block, lg = 31 - __builtin_clz(T);
        const int64_t* row = p.block_pointers + (int64_t) b * 2 * p.max_blocks_per_seq + (slot >> lg);
        const int64_t kblk = row[0], vblk = row[p.max_blocks_per_seq];
        if (kblk == 0 || vblk == 0)
            return;
        const int64_t off = (((int64_t) h * T + (slot & (T - 1))) * DH + li * 8) * esz;
        kc = reinterpret_cast<char*>(kblk) + off;
        vc = reinterpret_cast<char*>(vblk) + off;
    }
    if (p.kv_dtype == DT_INT8)
    {
        const float sc = p.kv_scale_orig_quant[0];
        *reinterpret_cast<uint2*>(kc) = quant8(k4, sc);
        *reinterpret_cast<uint2*>(vc) = quant8(v4, sc);
    }
    else if (p.kv_dtype == DT_FP8)
    {
        const float sc = p.kv_scale_orig_quant[0];
        *reinterpret_cast<uint2*>(kc) = quant8_fp8(k4, sc);
        *reinterpret_cast<uint2*>(vc) = quant8_fp8(v4, sc);
    }
    else
    {
        *reinterpret_cast<uint4*>(kc) = k4;
        *reinterpret_cast<uint4*>(vc) = v4;
    }
}

// ---- (c) grid (ceil(n / 4), H, B); 4 waves, one query per wave; the lane groups of a wave take disjoint keys and share the
// running maximum, so the merge at the end is a plain sum (the scheme of context_attn_kernel).
template <int DH, int KV, bool PG>
__global__ __launch_bounds__(256) void append_attn_wave_kernel(const AppendAttnParams p)
{
    constexpr int LPR = DH / 8, RPW = 64 / LPR, NIT = 4, ESZ = KV == 0 ? 2 : 1;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + wid, h = blockIdx.y, b = blockIdx.z;
    if (qi >= p.n)
        return;
    const int li = lane % LPR, grp = lane / LPR;
    const int H = p.num_heads, Hkv = p.num_kv_heads, Smax = p.max_seq_len;
    if (p.n_per_seq && qi >= clampi(p.n_per_seq[b], 0, p.n)) // a padding row (uniform over the wave): zeros, no key is read
    {
        if (grp == 0)
            *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(p.out) + (((int64_t) b * p.n + qi) * H + h) * DH + li * 8) = make_uint4(0, 0, 0, 0);
        return;
    }
    const int kvh = h / (H / Hkv);
    const int pb = clampi(p.sequence_length[b], 0, Smax);
    const int64_t rs = (int64_t) (H + 2 * Hkv) * DH;
    const uint16_t* base = reinterpret_cast<const uint16_t*>(p.qkv) + (int64_t) b * p.n * rs;
    const uint4 q16 = *reinterpret_cast<const uint4*>(base + (int64_t) qi * rs + (int64_t) h * DH + li * 8);
    const uint16_t* kb = base + (int64_t) (H + kvh) * DH + li * 8;
    const uint16_t* vb = base + (int64_t) (H + Hkv + kvh) * DH + li * 8;
    const char* kc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 0) * Hkv + kvh) * Smax) * DH * ESZ + li * 8 * ESZ;
    const char* vc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 1) * Hkv + kvh) * Smax) * DH * ESZ + li * 8 * ESZ;
    const int32_t* mask = p.masked_tokens ? p.masked_tokens + (int64_t) b * Smax : nullptr;
    const float s_qo = KV != 0 ? p.kv_scale_quant_orig[0] : 1.f;
    const int pg_mask = PG ? p.tokens_per_block - 1 : 0, pg_lg = PG ? 31 - __builtin_clz(p.tokens_per_block) : 0;

    float m = -INFINITY, l = 0.f;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // RPW * NIT keys: kscale on the scores, vscale on the p.v contribution (the dequantisation scale for cache rows, else 1)
    auto block = [&](const uint4(&kk)[NIT], const uint4(&vv)[NIT], const bool(&ok)[NIT], float kscale, float vscale) {
        float s[NIT];
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < NIT; ++i)
        {
            float d = 0.f;
            d = dot2(q16.x, kk[i].x, d);
            d = dot2(q16.y, kk[i].y, d);
            d = dot2(q16.z, kk[i].z, d);
            d = dot2(q16.w, kk[i].w, d);
            d = group_sum<LPR>(d) * kscale;
            s[i] = ok[i] ? d : -INFINITY;
            mt = fmaxf(mt, s[i]);
        }
#pragma unroll
        for (int mk = 32; mk >= LPR; mk >>= 1)
            mt = fmaxf(mt, __shfl_xor(mt, mk, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
        l *= alpha;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] *= alpha;
        m = mn;
#pragma unroll
        for (int i = 0; i < NIT; ++i)
        {
            const float pr = (s[i] == -INFINITY) ? 0.f : __expf(s[i] - m);
            l += pr;
            const float pv = h2f(f2h(pr)) * vscale;
            float vf[8];
            h8_to_f(vv[i], vf);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                o[j] = fmaf(pv, vf[j], o[j]);
        }
    };
    // the past: cache slots [0, p_b) that are not masked
    for (int j0 = 0; j0 < pb; j0 += RPW * NIT)
    {
        uint4 kk[NIT], vv[NIT];
        bool ok[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i)
        {
            const int t = j0 + i * RPW + grp;
            ok[i] = t < pb && (!mask || mask[t] == 0);
            kk[i] = vv[i] = make_uint4(0, 0, 0, 0);
            if (ok[i])
            {
                if constexpr (PG)
                {
                    // one look at the table per key row (the LPR lanes of a row read the same two entries, and the rows of a block
                    // find them in the vector cache); t < p_b, so the block is one the sequence holds - and should its entry be 0
                    // all the same, the load goes to the pool, not to 0 + offset.  (Looking the NIT rows of the next pass up one
                    // pass ahead, unconditionally, was tried and was slower: profiles/append_paged.txt)
                    const int64_t* row = p.block_pointers + (int64_t) b * 2 * p.max_blocks_per_seq + (t >> pg_lg);
                    const int64_t kblk = row[0], vblk = row[p.max_blocks_per_seq];
                    const int64_t off = (((int64_t) kvh * p.tokens_per_block + (t & pg_mask)) * DH + li * 8) * ESZ;
                    kk[i] = load_kv8<KV>((kblk ? reinterpret_cast<const char*>(kblk) : reinterpret_cast<const char*>(p.kv_cache)) + off);
                    vv[i] = load_kv8<KV>((vblk ? reinterpret_cast<const char*>(vblk) : reinterpret_cast<const char*>(p.kv_cache)) + off);
                }
                else
                {
                    kk[i] = load_kv8<KV>(kc + (int64_t) t * DH * ESZ);
                    vv[i] = load_kv8<KV>(vc + (int64_t) t * DH * ESZ);
                }
            }
        }
        block(kk, vv, ok, s_qo * p.inv_sqrt_dh, s_qo);
    }
    // the chunk: appended tokens 0 .. qi from the QKV buffer (after launch (a): k with RoPE applied)
    const int nkeys = qi + 1;
    for (int j0 = 0; j0 < nkeys; j0 += RPW * NIT)
    {
        uint4 kk[NIT], vv[NIT];
        bool ok[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i)
        {
            const int j = j0 + i * RPW + grp;
            ok[i] = j < nkeys;
            kk[i] = vv[i] = make_uint4(0, 0, 0, 0);
            if (ok[i])
            {
                kk[i] = *reinterpret_cast<const uint4*>(kb + (int64_t) j * rs);
                vv[i] = *reinterpret_cast<const uint4*>(vb + (int64_t) j * rs);
            }
        }
        block(kk, vv, ok, p.inv_sqrt_dh, 1.f);
    }
#pragma unroll
    for (int mk = 32; mk >= LPR; mk >>= 1)
    {
        l += __shfl_xor(l, mk, 64);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] += __shfl_xor(o[j], mk, 64);
    }
    if (grp == 0)
    {
        const float inv = 1.f / (l + 1.e-6f);
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            r[j] = o[j] * inv;
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(p.out) + (((int64_t) b * p.n + qi) * H + h) * DH + li * 8) = f_to_h8(r);
    }
}

// ---- (b) MFMA, flash-style.  Workgroup = 4 waves = 64 consecutive queries of one (sequence, head); keys advance in blocks of 64,
// the past blocks (cache slots 64 k .., masked by slot < p_b and the slot mask) before the chunk's blocks (appended tokens
// 64 k .., masked causally on the block that crosses the diagonal).  Wave 2 u + w serves queries 32 w .. 32 w + 31 on keys
// 32 u .. 32 u + 31 of every block with a running (m, l, O) of its own; the two key halves of a query slice merge once, after
// the last block, through LDS (the key split of context_attn_mfma_ks_kernel).  Operand roles as in
// context_attn_mfma_ks_kernel, so that everything the soft-max needs is lane-local (v_mfma_f32_32x32x16_f16):
//   S^T[key, q]  = K[key, :] . Q^T[:, q]       A = K rows (LDS image [64][DH], rows padded by 16 bytes), B = Q (registers, loaded once)
//       -> lane (q = lane & 31, half = lane >> 5) holds 16 scores of ITS query, register i = key 32 u + (i & 3) + 8 (i >> 2) +
//          4 half; the row maximum and sum are in-register plus one exchange with lane ^ 32;
//   O^T[d, q]   += V^T[d, keys] . P^T[keys, q]  A = V^T rows (LDS image [DH][64], rows padded by 16 bytes), B = the score registers
//          8 s .. 8 s + 7 of a tile converted to fp16 in place.  Element j of that fragment is key 16 s + 8 (j >> 2) + 4 half +
//          (j & 3) of the tile, so the loader writes key k of a block to column (k with bits 2 and 3 swapped) of V^T and the A
//          fragment is one 16-byte LDS read.
// The loader is the only part that differs between the two sources: cache rows of a one-byte type become fp16 on the way into
// LDS (their dequantisation scale multiplies the scores of the block, and the accumulator once, on the step from the last past
// block to the first chunk block - every past product carries it, no chunk product does), V is transposed on the way in, and the
// V rows of keys that are masked or beyond a length are written as zero.  One operand stage: load, barrier, compute, barrier.
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// Paged instances (PG): the table is looked up once per 64-key block, not once per row - a block of keys spans NE = max(64 / T, 1)
// cache blocks (T = 128: half of one).  Threads 0 .. 127 hold the K (0 .. 63) and V (64 .. 127) entries of the NEXT past block in
// a register, requested while the current block computes, and publish them in sBlk ahead of the barrier that opens the block's
// loads; a row then takes its block's address from LDS.  An entry of 0 is published as the pool's own address (a select, never
// 0 + offset), and the K rows, which are loaded whether their key counts or not, take the slot min(key, p_b - 1): a slot below
// p_b, which the sequence holds (a past block exists only where p_b >= 1).  What such a row holds is masked as before.
template <int DH, int KV, bool PG>
__global__ __launch_bounds__(256) void append_attn_mfma_kernel(const AppendAttnParams p)
{
    constexpr int ESZ = KV == 0 ? 2 : 1;
    constexpr int KP = DH * 2 + 16; // bytes per row of the K image: 16 consecutive rows start 4 banks apart
    constexpr int VP = 64 * 2 + 16; // bytes per row of the V^T image
    constexpr int KT = DH / 16;     // k-steps of a score tile
    constexpr int DT = DH / 32;     // 32-row tiles of O^T
    constexpr int LPR = DH / 8, KPP = 256 / LPR, KPASS = 64 / KPP, VPASS = LPR / 4;
    constexpr int MREC = DT * 16 + 2; // floats a lane hands over in the merge: O^T registers, m, l
    static_assert(2 * 64 * MREC * 4 <= 64 * KP + DH * VP, "the merge records fit the operand images");
    __shared__ __attribute__((aligned(16))) char smem[64 * KP + DH * VP];
    __shared__ int sOk[64];
    char* const sK = smem;
    char* const sV = smem + 64 * KP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int w = wv & 1;  // query slice: queries 32 w .. 32 w + 31 of the block
    const int u = wv >> 1; // key half: keys 32 u .. 32 u + 31 of every 64-key block
    const int h = blockIdx.x, qb = blockIdx.y, b = blockIdx.z;
    const int H = p.num_heads, Hkv = p.num_kv_heads, Smax = p.max_seq_len, n = p.n;
    const int nb = p.n_per_seq ? clampi(p.n_per_seq[b], 0, n) : n; // this sequence's tokens; rows nb .. n - 1 are padding
    if (qb * 64 >= nb) // a query block of padding alone (uniform over the workgroup, before the first barrier): zeros
    {
        for (int x = tid; x < 64 * LPR; x += 256)
        {
            const int row = qb * 64 + x / LPR;
            if (row < n)
                *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(p.out) + (((int64_t) b * n + row) * H + h) * DH + (x % LPR) * 8) = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    const int kvh = h / (H / Hkv);
    const int pb = clampi(p.sequence_length[b], 0, Smax);
    const int64_t rs = (int64_t) (H + 2 * Hkv) * DH;
    const uint16_t* base = reinterpret_cast<const uint16_t*>(p.qkv) + (int64_t) b * n * rs;
    const uint16_t* kb = base + (int64_t) (H + kvh) * DH;
    const uint16_t* vb = base + (int64_t) (H + Hkv + kvh) * DH;
    const char* kc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 0) * Hkv + kvh) * Smax) * DH * ESZ;
    const char* vc = reinterpret_cast<const char*>(p.kv_cache) + ((((int64_t) b * 2 + 1) * Hkv + kvh) * Smax) * DH * ESZ;
    const int32_t* mask = p.masked_tokens ? p.masked_tokens + (int64_t) b * Smax : nullptr;
    const float s_qo = KV != 0 ? p.kv_scale_quant_orig[0] : 1.f;
    const int qi = qb * 64 + w * 32 + r; // this lane's query (index into the chunk); rows >= nb compute on row nb - 1: stored as zeros below n, not at all from n on
    f16x8_t qf[KT];
    {
        const uint16_t* qrow = base + (int64_t) min(qi, nb - 1) * rs + (int64_t) h * DH + 8 * hh;
#pragma unroll
        for (int t = 0; t < KT; ++t)
            qf[t] = *reinterpret_cast<const f16x8_t*>(qrow + 16 * t);
    }
    f32x16_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            oacc[dt][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int npast = (pb + 63) >> 6, nblk = npast + qb + 1;
    // paged: the entry thread tid < 128 fetches for the 64-key block at slot k0 - entry e = tid & 63 of the K (tid < 64) or V row,
    // clamped to the block of slot p_b - 1; entries e >= NE are never read
    int64_t* sBlk = nullptr;
    int64_t pg_next = 0;
    const int pg_T = PG ? p.tokens_per_block : 1, pg_lg = PG ? 31 - __builtin_clz(pg_T) : 0;
    auto pg_entry = [&](int k0) -> int64_t {
        const int j = min((k0 >> pg_lg) + (tid & 63), max(pb - 1, 0) >> pg_lg);
        const int64_t e = p.block_pointers[((int64_t) b * 2 + (tid >> 6)) * p.max_blocks_per_seq + j];
        return e ? e : reinterpret_cast<int64_t>(p.kv_cache);
    };
    if constexpr (PG)
    {
        __shared__ int64_t blk_lds[128];
        sBlk = blk_lds;
        if (tid < 128 && npast > 0)
            pg_next = pg_entry(0);
    }
    for (int blk = 0; blk < nblk; ++blk)
    {
        const bool past = blk < npast; // uniform
        const int k0 = (past ? blk : blk - npast) * 64;
        if (KV != 0 && blk == npast)
        {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                oacc[dt] *= s_qo;
        }
        if constexpr (PG)
        {
            if (past && tid < 128) // (the loads of the previous block, the last readers of sBlk, ended before its second barrier)
                sBlk[tid] = pg_next;
        }
        __syncthreads(); // the previous block's fragment reads are done
        if constexpr (PG)
        {
            if (tid < 128 && blk + 1 < npast)
                pg_next = pg_entry(k0 + 64);
        }
        {
            // K rows: LPR consecutive lanes fetch one row
            const int c = tid % LPR;
            uint4 kr[KPASS];
#pragma unroll
            for (int ps = 0; ps < KPASS; ++ps)
            {
                const int key = k0 + ps * KPP + tid / LPR;
                if (past)
                {
                    if constexpr (PG)
                    {
                        const int kq = min(key, pb - 1); // >= k0: a past block starts below p_b
                        const char* blkp = reinterpret_cast<const char*>(sBlk[(kq >> pg_lg) - (k0 >> pg_lg)]);
                        kr[ps] = load_kv8<KV>(blkp + (((int64_t) kvh * pg_T + (kq & (pg_T - 1))) * DH + c * 8) * ESZ);
                    }
                    else
                        kr[ps] = load_kv8<KV>(kc + ((int64_t) min(key, Smax - 1) * DH + c * 8) * ESZ);
                }
                else
                    kr[ps] = *reinterpret_cast<const uint4*>(kb + (int64_t) min(key, nb - 1) * rs + c * 8);
            }
#pragma unroll
            for (int ps = 0; ps < KPASS; ++ps)
                *reinterpret_cast<uint4*>(sK + (ps * KPP + tid / LPR) * KP + c * 16) = kr[ps];
            // V rows, transposed: lane = key, so a wave writes 64 consecutive halfs of a V^T row per element
            const int kl = tid & 63, key = k0 + kl;
            const bool ok = past ? (key < pb && (!mask || mask[key] == 0)) : key < nb;
            if (tid < 64)
                sOk[kl] = ok ? 1 : 0;
            const int col = (kl & ~12) | ((kl & 4) << 1) | ((kl & 8) >> 1);
            uint4 vr[VPASS];
#pragma unroll
            for (int ps = 0; ps < VPASS; ++ps)
            {
                const int cc = (tid >> 6) + 4 * ps;
                vr[ps] = make_uint4(0, 0, 0, 0);
                if constexpr (PG)
                {
                    if (ok && past) // key < p_b: its entry is among the NE published ones
                        vr[ps] = load_kv8<KV>(reinterpret_cast<const char*>(sBlk[64 + (key >> pg_lg) - (k0 >> pg_lg)])
                            + (((int64_t) kvh * pg_T + (key & (pg_T - 1))) * DH + cc * 8) * ESZ);
                    else if (ok)
                        vr[ps] = *reinterpret_cast<const uint4*>(vb + (int64_t) key * rs + cc * 8);
                }
                else if (ok)
                    vr[ps] = past ? load_kv8<KV>(vc + ((int64_t) key * DH + cc * 8) * ESZ)
                                  : *reinterpret_cast<const uint4*>(vb + (int64_t) key * rs + cc * 8);
            }
#pragma unroll
            for (int ps = 0; ps < VPASS; ++ps)
            {
                const int cc = (tid >> 6) + 4 * ps;
                const uint32_t wv[4] = {vr[ps].x, vr[ps].y, vr[ps].z, vr[ps].w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    *reinterpret_cast<uint16_t*>(sV + (cc * 8 + e) * VP + col * 2) = (uint16_t) (wv[e >> 1] >> (16 * (e & 1)));
            }
        }
        __syncthreads();
        // scores of this wave's 32 queries against its 32 keys of the block
        f32x16_t sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            sacc[i] = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t)
        {
            const f16x8_t a = *reinterpret_cast<const f16x8_t*>(sK + (32 * u + r) * KP + (16 * t + 8 * hh) * 2);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[t], sacc, 0, 0, 0);
        }
        const float kscale = past ? s_qo * p.inv_sqrt_dh : p.inv_sqrt_dh;
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            const int kl = 32 * u + (i & 3) + 8 * (i >> 2) + 4 * hh;
            const bool ok = past ? sOk[kl] != 0 : k0 + kl <= qi; // (chunk: qi < nb for every row stored as computed, so k0 + kl < nb too)
            sacc[i] = ok ? sacc[i] * kscale : -INFINITY;
            mt = fmaxf(mt, sacc[i]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
        m = mn;
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            const float pr = (sacc[i] == -INFINITY) ? 0.f : __expf(sacc[i] - mn);
            lsum += pr;
            sacc[i] = pr;
        }
        l = l * alpha + lsum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            oacc[dt] *= alpha;
#pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            f16x8_t pf;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                pf[j] = (_Float16) sacc[8 * s + j];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
            {
                const f16x8_t a = *reinterpret_cast<const f16x8_t*>(sV + (32 * dt + r) * VP + (32 * u + 16 * s + 8 * hh) * 2);
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf, oacc[dt], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    // the two key halves of a query slice merge once, through LDS (the operand images are dead): O = O0 a0 + O1 a1, l likewise,
    // a = exp(m_i - max(m0, m1)).  Record of lane x of slice w: float [MREC][64] at slice w, so a wave's accesses are contiguous
    __syncthreads();
    float* const rec = reinterpret_cast<float*>(smem) + (w * MREC) * 64 + lane;
    if (u == 1)
    {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                rec[(dt * 16 + i) * 64] = oacc[dt][i];
        rec[(DT * 16) * 64] = m;
        rec[(DT * 16 + 1) * 64] = l;
    }
    __syncthreads();
    if (u == 1)
        return;
    {
        const float m1 = rec[(DT * 16) * 64], l1 = rec[(DT * 16 + 1) * 64];
        const float mx = fmaxf(m, m1);
        const float a0 = (m == -INFINITY) ? 0.f : __expf(m - mx), a1 = (m1 == -INFINITY) ? 0.f : __expf(m1 - mx);
        l = l * a0 + l1 * a1;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                oacc[dt][i] = oacc[dt][i] * a0 + rec[(dt * 16 + i) * 64] * a1;
    }
    if (qi < n)
    {
        const float inv = qi < nb ? 1.f / (l + 1.e-6f) : 0.f;
        if (qi >= nb) // a padding row of a partly filled block: zeros, whatever the clamped loads gave
        {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    oacc[dt][i] = 0.f;
        }
        uint16_t* orow = reinterpret_cast<uint16_t*>(p.out) + (((int64_t) b * n + qi) * H + h) * DH + 4 * hh;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<uint2*>(orow + 32 * dt + 8 * g) = make_uint2(
                    pack_h2(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv), pack_h2(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv));
    }
}

// ---- (d) one workgroup
__global__ __launch_bounds__(256) void append_advance_kernel(int32_t* sequence_length, int32_t* finished, const int32_t* n_per_seq,
    int32_t batch, int32_t n)
{
    for (int b = threadIdx.x; b < batch; b += 256)
    {
        sequence_length[b] += n_per_seq ? clampi(n_per_seq[b], 0, n) : n;
        if (finished)
            finished[b] = 0;
    }
}

template <int DH, bool PG>
int launch_dh(const AppendAttnParams& p, int kind, hipStream_t stream)
{
    constexpr int HG = 256 / (DH / 8);
    hipLaunchKernelGGL((append_rope_kv_kernel<DH, PG>), dim3(p.n, (p.num_heads + HG - 1) / HG, p.batch), dim3(256), 0, stream, p);
    if (launch_util::check_launch("append attention (RoPE, cache write)"))
        return -1;
    const int kv = kv_kind(p.kv_dtype);
    if (kind == APPEND_ATTN_MFMA)
    {
        if constexpr (DH == 64 || DH == 128)
        {
            const dim3 grid(p.num_heads, (p.n + 63) / 64, p.batch);
            if (kv == 0)
                hipLaunchKernelGGL((append_attn_mfma_kernel<DH, 0, PG>), grid, dim3(256), 0, stream, p);
            else if (kv == 1)
                hipLaunchKernelGGL((append_attn_mfma_kernel<DH, 1, PG>), grid, dim3(256), 0, stream, p);
            else
                hipLaunchKernelGGL((append_attn_mfma_kernel<DH, 2, PG>), grid, dim3(256), 0, stream, p);
        }
    }
    else
    {
        const dim3 grid((p.n + 3) / 4, p.num_heads, p.batch);
        if (kv == 0)
            hipLaunchKernelGGL((append_attn_wave_kernel<DH, 0, PG>), grid, dim3(256), 0, stream, p);
        else if (kv == 1)
            hipLaunchKernelGGL((append_attn_wave_kernel<DH, 1, PG>), grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((append_attn_wave_kernel<DH, 2, PG>), grid, dim3(256), 0, stream, p);
    }
    return launch_util::check_launch("append attention");
}

} // namespace

int append_attention_kernel(int32_t head_size, int32_t n, int32_t forced_kernel, const char** refused)
{
    const char* why = nullptr;
    int kind = 0;
    const bool wave_ok = head_size == 32 || head_size == 64 || head_size == 128 || head_size == 256;
    const bool mfma_ok = (head_size == 64 || head_size == 128) && n >= 16;
    if (n < 1)
        why = "no tokens to append";
    else if (!wave_ok)
        why = "head size is not 32, 64, 128 or 256";
    else if (forced_kernel == APPEND_ATTN_RULE)
        kind = mfma_ok ? APPEND_ATTN_MFMA : APPEND_ATTN_WAVE;
    else if (forced_kernel == APPEND_ATTN_WAVE)
        kind = APPEND_ATTN_WAVE;
    else if (forced_kernel == APPEND_ATTN_MFMA)
    {
        if (mfma_ok)
            kind = APPEND_ATTN_MFMA;
        else
            why = "the MFMA kernel needs head size 64 or 128 and n >= 16";
    }
    else
        why = "unknown kernel kind";
    if (refused)
        *refused = why;
    return kind;
}

int launch_append_attention(const AppendAttnParams& pin, hipStream_t stream)
{
    AppendAttnParams p = pin;
    if (p.num_kv_heads == 0)
        p.num_kv_heads = p.num_heads;
    if (p.batch < 1 || p.batch > 65535 || p.n < 1 || p.num_heads < 1 || p.num_heads > 65535 || p.max_seq_len < 1)
    {
        set_error("append attention: bad shape (batch %d, n %d, num_heads %d, max_seq_len %d)", p.batch, p.n, p.num_heads, p.max_seq_len);
        return -1;
    }
    if (p.num_kv_heads < 1 || p.num_kv_heads > p.num_heads || p.num_heads % p.num_kv_heads != 0)
    {
        set_error("append attention: num_kv_heads %d must divide num_heads %d", p.num_kv_heads, p.num_heads);
        return -1;
    }
    const char* why = nullptr;
    const int kind = append_attention_kernel(p.head_size, p.n, p.kernel, &why);
    if (kind == 0)
    {
        set_error("append attention: kernel %d refused (head size %d, n %d): %s", p.kernel, p.head_size, p.n, why ? why : "no plan");
        return -1;
    }
    if (launch_util::check_kv_dtype("append attention", p.kv_dtype, p.kv_scale_orig_quant && p.kv_scale_quant_orig))
        return -1;
    if (p.block_pointers)
    {
        const int t = p.tokens_per_block;
        if (t < 1 || (t & (t - 1)) || (int64_t) p.max_blocks_per_seq * t < p.max_seq_len)
        {
            set_error("append attention: paged KV cache needs tokens_per_block a power of two and max_blocks_per_seq * "
                      "tokens_per_block >= max_seq_len (got %d x %d for %d)", p.max_blocks_per_seq, t, p.max_seq_len);
            return -1;
        }
        if (!p.kv_cache)
        {
            set_error("append attention: paged KV cache needs the pool in kv_cache (the block table alone is not enough)");
            return -1;
        }
    }
    if (!p.qkv || !p.kv_cache || !p.out || !p.sequence_length || !p.input_lengths)
    {
        set_error("append attention: qkv, kv_cache, out, sequence_length and input_lengths must be set");
        return -1;
    }
    if (((uintptr_t) p.qkv | (uintptr_t) p.kv_cache | (uintptr_t) p.out) & 15)
    {
        set_error("append attention: qkv, kv_cache and out must be 16-byte aligned");
        return -1;
    }
    if (p.n_per_seq)
    {
        if (p.max_end < 1 || p.max_end > p.max_seq_len)
        {
            set_error("append attention: max_end %d outside [1, the cache capacity %d]", p.max_end, p.max_seq_len);
            return -1;
        }
    }
    else if (p.max_past < 0 || (int64_t) p.max_past + p.n > p.max_seq_len)
    {
        set_error("append attention: max_past %d + n %d exceeds the cache capacity %d", p.max_past, p.n, p.max_seq_len);
        return -1;
    }
    if (p.rotary_dim < 0 || p.rotary_dim > p.head_size || (p.rotary_dim & 1) || (p.neox && p.rotary_dim != 0 && p.rotary_dim != p.head_size))
    {
        set_error("append attention: rotary_dim %d not served (even, <= head size; NeoX pairs: the head size itself)", p.rotary_dim);
        return -1;
    }
    if (p.rotary_dim > 0 && (!p.rope_table || p.rope_table_len < 1))
    {
        set_error("append attention: rotary_dim %d without a RoPE table", p.rotary_dim);
        return -1;
    }
    if (p.block_pointers) // the paged instances
    {
        switch (p.head_size)
        {
        case 32: return launch_dh<32, true>(p, kind, stream);
        case 64: return launch_dh<64, true>(p, kind, stream);
        case 128: return launch_dh<128, true>(p, kind, stream);
        default: return launch_dh<256, true>(p, kind, stream);
        }
    }
    switch (p.head_size)
    {
    case 32: return launch_dh<32, false>(p, kind, stream);
    case 64: return launch_dh<64, false>(p, kind, stream);
    case 128: return launch_dh<128, false>(p, kind, stream);
    default: return launch_dh<256, false>(p, kind, stream);
    }
}

int launch_append_advance(int32_t* sequence_length, int32_t* finished, int32_t batch, int32_t n, hipStream_t stream)
{
    if (!sequence_length || batch < 1 || n < 1)
    {
        set_error("append advance: bad arguments");
        return -1;
    }
    hipLaunchKernelGGL(append_advance_kernel, dim3(1), dim3(256), 0, stream, sequence_length, finished, (const int32_t*) nullptr, batch, n);
    return launch_util::check_launch("append advance");
}

int launch_append_advance_ragged(int32_t* sequence_length, int32_t* finished, const int32_t* n_per_seq, int32_t batch, int32_t n,
    hipStream_t stream)
{
    if (!sequence_length || !n_per_seq || batch < 1 || n < 1)
    {
        set_error("append advance: bad arguments");
        return -1;
    }
    hipLaunchKernelGGL(append_advance_kernel, dim3(1), dim3(256), 0, stream, sequence_length, finished, n_per_seq, batch, n);
    return launch_util::check_launch("append advance");
}

} // namespace kernels
} // namespace tllm
