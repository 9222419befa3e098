// fp16-weight GEMM for 9 <= M <= 64 activation rows as a WEIGHT STREAM whose ring feeds the matrix pipe directly.
//
//   v[m, n] = sum_k A16[m, k] * W16[n, k]          exact products, fp32 accumulation, no scale
//   C       = fp16(v) | fp32 v | fp16(fp16(v) + residual16) | silu_mul_fp16(gate16, v)
//
// Why: fp16 was the one weight type without a stream.  The append / verify / lookup passes of an fp16 engine run their
// projections at 9 .. 64 rows through launch_gemm's prefill tiles, and the lm_head - fp16 in EVERY engine, 262 MB at the 7B
// extents - goes through the same tiles (verify, scoring) or through 8-row GEMV slabs that stream it once per slab.  At these row
// counts the weights are the traffic and should cross the memory bus once.  This is gemm_stream_woq.hip's geometry with the
// dequantisation taken out: what the DMA leaves in the ring IS the MFMA operand.
//
// Geometry: a wave owns 16 weight rows, a workgroup of 4 waves a quad of row groups.  v_mfma_f32_16x16x32_f16 takes the weight
// fragment as its first operand (row = lane & 15, 8 k-elements per lane, quarter g4 = lane >> 4 of the 32-element k-step) against
// T = ceil(M / 16) activation tiles in the same geometry and leaves lane (m = lane & 15) four consecutive outputs n = 4 g4 + e of
// every tile: no cross-lane reduction, and a weight fragment is used T times.  T (1 .. 4) is the template parameter.
//
// Weights: a private LDS ring of 16 KB per wave, filled by LDS-DMA (`nt`: every byte is read once per call).  fp16 doubles the
// bytes per k-element, so a slot is one block of 128 k-elements of the wave's 16 rows = 16 x 256 bytes = 4 KB, four slots, filled by
// 4 instructions of 4 rows x 256 bytes - whole 128-byte lines, 12 KB in flight per wave as in the siblings: the int8 sibling's
// addressing with a row block of 256 bytes.  The 16-byte pieces of a row are rotated by the row so that the fragment read of 16 rows
// at one piece falls on 16 different bank groups.  A piece is 8 k-elements = one lane's MFMA operand: k-step c (0 .. 3) of a block
// reads piece c * 4 + g4 with one ds_read_b128 and hands it to the matrix instruction as it is - nothing between the LDS and the
// MFMA, which is the point of this variant.
//
// Activations: 64 x 4096 fp16 = 512 KB do not fit, so K is split: a workgroup keeps A[bucket, K-slice] resident in the 96 KB
// behind the rings (3072 / 1536 / 1024 / 768 k-elements for the four buckets), ZERO where row >= M or k >= the slice's end, and
// walks its quads of row groups against it - quad q = blockIdx.x + i * gridDim.x, one group per wave; blockIdx.y is the slice.
// 16-byte piece P of row r lives at P ^ (r & 15), so the fragment read of 16 rows at one piece covers 16 bank groups.  The fp32
// partial sums of (slice, group, tile) go to the caller's workspace as the wave holds them (1 KB, coalesced) and a second small
// launch adds the slices IN SLICE ORDER, applies the epilogue and stores C.  No atomics, no counter, no workgroup waits on another:
// two runs give the same bits.  No barrier in the main loop (the ring is private, the panel read-only behind the one barrier that
// publishes it).
//
// gemm_stream_f16_plan() states the split (pure host code): slices are multiples of 128 elements (K itself below 128), as few as
// the panel allows, more while quads x slices leave CUs idle and a slice keeps >= 512 elements (1 KB of a row, the siblings'
// bound in bytes), then the count with the least traffic on the longest-running workgroup - 2 bytes per weight element PLUS the
// partial sums a slice adds (bucket x 4 bytes per weight row, written and read back).  The lm_head shows why the second term is
// there: 32000 x 4096 at 64 rows cannot have fewer than 6 slices (the panel holds 768 elements), which is 49 MB of partial sums
// written and read back beside 262 MB of weights; 7 or 8 slices would only add to that, and the plan stays at 6.  At 16 rows the
// same head takes 2 slices and 4 MB.  The largest workspace the 7B head needs (M = 64): 6 x 2000 x 4 x 1024 = 49,152,000 bytes.
//
// Bounds: a weight row index is clamped to N - 1 and a piece behind the slice's end to the block's first piece of the same row
// (the loads happen, from real weights: their products face zero activations or land in outputs that are never stored); panel
// loads come from clamped addresses and are zeroed where row >= M or k >= the slice's end; every store is predicated by m < M,
// n < N.  Nothing behind K in a row, behind row N - 1 of W or behind row M - 1 of A is read.
#include "dev_utils.h"
#include "kernels.h"
#include "launch_util.h"
#include "lds_dma.h"
#include <algorithm>

namespace tllm
{
namespace kernels
{
using namespace dev;

namespace
{
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int kBlockK = 128;        // k-elements of a ring slot
constexpr int kRowBytes = 256;      // bytes of a row's block
constexpr int kSlotBytes = 4096;    // 16 rows x 256 bytes
constexpr int kSlots = 4;           // slots of a wave's ring
constexpr int kRingBytes = kSlots * kSlotBytes;
constexpr int kPanelBytes = 98304;  // the most the activation panel takes
constexpr int kLdsLimit = 160 * 1024;
constexpr int kMinSlice = 512;      // k-elements below which a slice is not split further to fill CUs

// T: activation tiles of 16 rows (bucket = 16 T).  kpad = the slice length ks rounded up to 128; part = the workspace.  ldw in bytes.
template <int T>
__global__ __launch_bounds__(256) void gemm_stream_f16_kernel(const uint16_t* __restrict__ a, const int64_t lda,
    const char* __restrict__ w, const int64_t ldw, const int M, const int N, const int K, const int ks, const int kpad,
    const int ngroups, f32x4* __restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = kSlots;
    constexpr int NI = 4;                // DMA instructions per slot: 4 rows x 16 pieces each
    char* panel = smem + 4 * kRingBytes; // [16 T][2 kpad bytes] fp16, piece P of row r at P ^ (r & 15)
    const int pitch = 2 * kpad;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: M0 and DMA bases
    const int r16 = lane & 15, g4 = lane >> 4;
    const int kbeg = (int) blockIdx.y * ks;
    const int klen = K - kbeg < ks ? K - kbeg : ks; // > 0 and a multiple of 64 (the plan has no empty slice)
    const int klenb = klen * 2;                     // in weight bytes: a multiple of 128, whole pieces
    const int nblk = (klen + kBlockK - 1) / kBlockK;

    // ---- this wave's weight stream: group 4 * quad + wid of the quads blockIdx.x, blockIdx.x + gridDim.x, ..
    const int nquads = (ngroups + 3) / 4;
    int nq_mine = (int) blockIdx.x < nquads ? (nquads - (int) blockIdx.x + (int) gridDim.x - 1) / (int) gridDim.x : 0;
    if (nq_mine > 0 && 4 * ((int) blockIdx.x + (nq_mine - 1) * (int) gridDim.x) + wid >= ngroups)
        --nq_mine; // the last quad may hold fewer than four groups
    const int total = nq_mine * nblk;
    const int ring_off = wid * kRingBytes;
    const uint32_t ring = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) void*) (smem + ring_off); // its LDS byte address (M0)
    const int drow = lane >> 4, dpos = lane & 15; // this lane's row and position inside a DMA instruction
    auto issue = [&](int q) {
        const int gi = q / nblk, j = q - gi * nblk;
        const int g = 4 * ((int) blockIdx.x + gi * (int) gridDim.x) + wid;
        const char* base = w + (int64_t) g * 16 * ldw + (int64_t) kbeg * 2 + j * kRowBytes;
        const uint32_t slot = ring + (uint32_t) (q % D) * kSlotBytes;
        const int last_row = N - 1 - g * 16; // >= 0: rows behind it are clamped onto it
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int row = 4 * i + drow;
            const int piece = (dpos + row) & 15; // rotated by the row (see the fragment read)
            const uint32_t off = (uint32_t) (row < last_row ? row : last_row) * (uint32_t) ldw
                + (j * kRowBytes + piece * 16 < klenb ? (uint32_t) piece * 16u : 0u);
            glds16s_nt(base, off, slot + i * 1024);
        }
    };
    for (int q = 0; q < D - 1 && q < total; ++q)
        issue(q); // before the panel: the first weights do not depend on it

    // ---- the activation panel: 16 lanes take 256 contiguous bytes of one row, a wave four rows per instruction
    {
        // (every load happens, from a clamped address, and is zeroed afterwards: a predicated load costs a round trip of its own)
        const int prow = tid >> 4;
#pragma unroll 2
        for (int P = tid & 15; P < kpad / 8; P += 16)
        {
            const int kc = P * 8 < klen ? P * 8 : 0;
            uint4 v[T];
#pragma unroll
            for (int t = 0; t < T; ++t)
            {
                const int r = prow + 16 * t;
                v[t] = *reinterpret_cast<const uint4*>(a + (int64_t) (r < M ? r : 0) * lda + kbeg + kc);
            }
#pragma unroll
            for (int t = 0; t < T; ++t)
            {
                const int r = prow + 16 * t;
                const bool ok = r < M && P * 8 < klen;
                *reinterpret_cast<uint4*>(panel + (size_t) r * pitch + (size_t) (P ^ prow) * 16)
                    = make_uint4(ok ? v[t].x : 0u, ok ? v[t].y : 0u, ok ? v[t].z : 0u, ok ? v[t].w : 0u);
            }
        }
    }
    __syncthreads();

    // ---- main loop
    // k-step c of a block: piece c * 4 + g4 - in the panel at that index ^ r16 of the row's block, in the ring at that index - r16
    const char* xrow = panel + (size_t) r16 * pitch;
    const char* wfrag = smem + ring_off + r16 * kRowBytes;
    int xoff[4], woff[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
        xoff[c] = ((c * 4 + g4) ^ r16) * 16;
        woff[c] = ((c * 4 + g4 - r16) & 15) * 16;
    }
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int q = 0;
    for (int gi = 0; gi < nq_mine; ++gi)
    {
        for (int j = 0; j < nblk; ++j, ++q)
        {
            // keep D - 1 blocks in flight; then block q has landed when at most the younger ones are outstanding (in-order counter;
            // the partial stores of the group before only make the wait longer)
            if (q + D - 1 < total)
            {
                issue(q + D - 1);
                wait_vmcnt<(D - 1) * NI>();
            }
            else
                wait_vmcnt<0>();
            const char* slot = wfrag + (q % D) * kSlotBytes;
            const char* xk = xrow + (size_t) j * (kBlockK * 2);
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                const uint4 wr = *reinterpret_cast<const uint4*>(slot + woff[c]);
                f16x8 w8;
                __builtin_memcpy(&w8, &wr, 16);
#pragma unroll
                for (int t = 0; t < T; ++t)
                {
                    const uint4 xr = *reinterpret_cast<const uint4*>(xk + (size_t) t * 16 * pitch + xoff[c]);
                    f16x8 x8;
                    __builtin_memcpy(&x8, &xr, 16);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w8, x8, acc[t], 0, 0, 0);
                }
            }
            // the slot is free for the DMA of the next iteration only once its fragments are in registers
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        // the accumulators through a VGPR operand HERE, in the MFMAs' own block (gemm_stream_sq.hip: hipcc otherwise reads them at
        // the head of the next block, ahead of the wait states the last MFMA is owed)
#pragma unroll
        for (int t = 0; t < T; ++t)
            asm volatile("; accumulator out of the matrix pipe" : "+v"(acc[t]));
        const int g = 4 * ((int) blockIdx.x + gi * (int) gridDim.x) + wid;
        f32x4* dst = part + (((size_t) blockIdx.y * ngroups + g) * T) * 64 + lane;
#pragma unroll
        for (int t = 0; t < T; ++t)
        {
            dst[(size_t) t * 64] = acc[t];
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

struct FinishArgs
{
    const f32x4* part;
    int32_t slices, ngroups, tiles;
    int32_t M, N, out_dtype;
    const uint16_t* residual;
    const uint16_t* silu_gate;
    void* c;
    int64_t ldc;
};

// one wave per (group, tile) fragment: the slices' partial sums in slice order, the epilogue, the store
__global__ __launch_bounds__(256) void gemm_stream_f16_finish_kernel(const FinishArgs f)
{
    const int lane = threadIdx.x & 63;
    const int frag = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (frag >= f.ngroups * f.tiles)
        return;
    const int g = frag / f.tiles, t = frag - g * f.tiles;
    const int m = t * 16 + (lane & 15), n0 = g * 16 + (lane >> 4) * 4;
    if (m >= f.M || n0 >= f.N)
        return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < f.slices; ++s)
        v += f.part[(((size_t) s * f.ngroups + g) * f.tiles + t) * 64 + lane];
    const int64_t o = (int64_t) m * f.ldc + n0;
    const int nv = f.N - n0 < 4 ? f.N - n0 : 4; // outputs of this lane that exist
    uint16_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int64_t oe = o + (e < nv ? e : 0);
        if (f.silu_gate)
            h[e] = f2h(silu_mul_fp16(h2f(f.silu_gate[oe]), v[e]));
        else if (f.residual)
            h[e] = f2h(h2f(f2h(v[e])) + h2f(f.residual[oe]));
        else
            h[e] = f2h(v[e]);
    }
    if (f.out_dtype == DT_HALF)
    {
        uint16_t* y = reinterpret_cast<uint16_t*>(f.c) + o;
        if (nv == 4)
            *reinterpret_cast<uint2*>(y) = make_uint2((uint32_t) h[0] | ((uint32_t) h[1] << 16), (uint32_t) h[2] | ((uint32_t) h[3] << 16));
        else
            for (int e = 0; e < nv; ++e)
                y[e] = h[e];
    }
    else
    {
        float* y = reinterpret_cast<float*>(f.c) + o;
        if (nv == 4)
            *reinterpret_cast<float4*>(y) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int e = 0; e < nv; ++e)
                y[e] = v[e];
    }
}

template <int T>
int launch_bucket(const GemmParams& p, const GemmStreamPlan& plan, void* workspace, hipStream_t stream)
{
    auto kfn = gemm_stream_f16_kernel<T>;
    launch_util::ensure_dynamic_lds(reinterpret_cast<const void*>(kfn), kLdsLimit); // the most any plan asks for: set once
    const int kpad = (plan.k_slice + kBlockK - 1) / kBlockK * kBlockK;
    hipLaunchKernelGGL(kfn, dim3((unsigned) plan.grid_x, (unsigned) plan.k_slices), dim3(256), (size_t) plan.lds_bytes, stream,
        reinterpret_cast<const uint16_t*>(p.a), p.lda, reinterpret_cast<const char*>(p.w), p.ldw, p.M, p.N, p.K, plan.k_slice, kpad,
        plan.row_groups, reinterpret_cast<f32x4*>(workspace));
    return launch_util::check_launch("gemm_stream_f16");
}

} // namespace

GemmStreamPlan gemm_stream_f16_plan(int32_t M, int32_t N, int32_t K, int32_t cus)
{
    GemmStreamPlan plan;
    if (M < 9 || M > 64)
    {
        plan.refused = "M outside 9 .. 64 rows";
        return plan;
    }
    if (N < 1 || K < 64 || (K & 63))
    {
        plan.refused = "N < 1, or K not a positive multiple of 64";
        return plan;
    }
    if (cus <= 0)
        cus = 256;
    plan.bucket = (M + 15) / 16 * 16;
    const int ks_max = (kPanelBytes / (2 * plan.bucket)) & ~(kBlockK - 1); // 3072 / 1536 / 1024 / 768
    plan.row_groups = (N + 15) / 16;
    const int nquads = (plan.row_groups + 3) / 4;
    // gemm_stream_woq_plan's rule: the fewest slices the panel allows, more while quads x slices leave CUs idle; from there up to
    // `most` the count that leaves the longest-running workgroup the least traffic, ties to the fewer.  A quad's traffic per weight
    // row: the slice's 2 bytes per element and the partial sums of its bucket, 4 bytes each, written here and read back by the finish
    const int fill = (cus + nquads - 1) / nquads, most = K / kMinSlice > 1 ? K / kMinSlice : 1;
    const int lo = std::max((K + ks_max - 1) / ks_max, std::min(fill, most));
    int64_t best = -1;
    for (int s = lo; s <= std::max(lo, std::min(most, 4 * lo)); ++s)
    {
        int ks = (K + s - 1) / s;
        ks = K < kBlockK ? K : std::min((ks + kBlockK - 1) / kBlockK * kBlockK, ks_max);
        const int slices = (K + ks - 1) / ks;
        const int gx = std::min(nquads, std::max(1, cus / slices));
        const int64_t cost = (int64_t) ((gx * slices + cus - 1) / cus) * ((nquads + gx - 1) / gx) * (ks * 2 + 8 * plan.bucket);
        if (best < 0 || cost < best)
        {
            best = cost;
            plan.k_slice = ks;
            plan.k_slices = slices;
            plan.grid_x = gx;
        }
    }
    plan.groups_per_workgroup = (nquads + plan.grid_x - 1) / plan.grid_x * 4;
    plan.lds_bytes = 4 * kRingBytes + plan.bucket * 2 * ((plan.k_slice + kBlockK - 1) / kBlockK * kBlockK);
    plan.workspace_bytes = (int64_t) plan.k_slices * plan.row_groups * (plan.bucket / 16) * 1024;
    return plan;
}

// 0 launched, -1 launch error, 1 refused (the reason is the error string; nothing is enqueued)
int launch_gemm_stream_f16(const GemmParams& p, void* workspace, int64_t workspace_bytes, hipStream_t stream)
{
    auto refuse = [&](const char* why) {
        set_error("gemm_stream_f16: %d x %d x %d refused: %s", p.M, p.N, p.K, why);
        return 1;
    };
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (p.wtype != W_FP16)
        return refuse("the weight type is not fp16 (tllm_gemm_stream serves SmoothQuant and weight-only int8 / int4)");
    const GemmStreamPlan plan = gemm_stream_f16_plan(p.M, p.N, p.K, gemm_stream_cus());
    if (plan.refused)
        return refuse(plan.refused);
    if (p.w2)
        return refuse("a dual GEMM is not served");
    if (p.out_dtype != DT_HALF && p.out_dtype != DT_FLOAT)
        return refuse("the output type is neither fp16 nor fp32");
    if ((p.residual || p.silu_gate) && p.out_dtype != DT_HALF)
        return refuse("a residual or a SwiGLU gate needs fp16 output");
    if (p.residual && p.silu_gate)
        return refuse("a residual and a SwiGLU gate together are not served");
    if (!p.a || !p.w || !p.c)
        return refuse("a null operand");
    if (misaligned(p.a, 16) || (p.lda & 7) || p.lda < p.K)
        return refuse("A is not 16-byte aligned, or lda is below K or not a multiple of 8");
    if (misaligned(p.w, 16) || (p.ldw & 15) || p.ldw < (int64_t) 2 * p.K || (int64_t) 16 * p.ldw + 256 >= (1ll << 32))
        return refuse("W is not 16-byte aligned, or ldw is below the row's 2 K bytes, not a multiple of 16 bytes (8 elements) or beyond 32-bit offsets in a row group");
    if (misaligned(p.c, p.out_dtype == DT_HALF ? 8 : 16) || (p.ldc & 3) || p.ldc < p.N)
        return refuse("C is not aligned to four outputs, or ldc is below N or not a multiple of 4");
    if (misaligned(p.residual, 2) || misaligned(p.silu_gate, 2))
        return refuse("the residual or the gate is not aligned");
    if (!workspace || misaligned(workspace, 16) || workspace_bytes < plan.workspace_bytes)
        return refuse("the workspace is null, not 16-byte aligned or smaller than gemm_stream_f16_plan's workspace_bytes");
    if (plan.lds_bytes > kLdsLimit)
        return refuse("the plan does not fit the LDS");
    int rc;
    switch (plan.bucket / 16)
    {
    case 1: rc = launch_bucket<1>(p, plan, workspace, stream); break;
    case 2: rc = launch_bucket<2>(p, plan, workspace, stream); break;
    case 3: rc = launch_bucket<3>(p, plan, workspace, stream); break;
    default: rc = launch_bucket<4>(p, plan, workspace, stream); break;
    }
    if (rc)
        return rc;
    FinishArgs f;
    f.part = reinterpret_cast<const f32x4*>(workspace);
    f.slices = plan.k_slices;
    f.ngroups = plan.row_groups;
    f.tiles = plan.bucket / 16;
    f.M = p.M;
    f.N = p.N;
    f.out_dtype = p.out_dtype;
    f.residual = reinterpret_cast<const uint16_t*>(p.residual);
    f.silu_gate = reinterpret_cast<const uint16_t*>(p.silu_gate);
    f.c = p.c;
    f.ldc = p.ldc;
    const int frags = f.ngroups * f.tiles;
    hipLaunchKernelGGL(gemm_stream_f16_finish_kernel, dim3((unsigned) ((frags + 3) / 4)), dim3(256), 0, stream, f);
    return launch_util::check_launch("gemm_stream_f16_finish");
}

} // namespace kernels
} // namespace tllm
