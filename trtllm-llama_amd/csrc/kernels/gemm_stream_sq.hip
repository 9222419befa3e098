// SmoothQuant GEMM for 9 <= M <= 64 activation rows as a WEIGHT STREAM with the arithmetic on the matrix pipe.
//
//   C[m, n] = epi( float(sum_k A8[m, k] * W8[n, k]) * (s_col[n or 0] * s_row[m or 0]) )      epi: none (fp16 / fp32) or + residual (fp16)
//
// Why: between the skinny kernels (M <= 8, every weight byte once) and the LDS-DMA prefill GEMMs (tiles of 128 rows, built to be
// MFMA-bound at M = 1024) the append / verify passes run B * n = 9 .. 64 rows on kernels that either stream the weights once per
// 8-row slab or fill a quarter of a tile.  At these row counts the GEMM is HBM-bound: the weights are the traffic, and they should
// cross the memory bus once.
//
// Geometry (that of gemv_mfma_sq.hip, which proved it): a wave owns 16 weight rows; v_mfma_i32_16x16x64_i8 takes 16 B per lane of W
// (row = lane & 15, k-bytes (lane >> 4) * 16 of a 64-byte k-step) against T = ceil(M / 16) activation tiles in the same geometry and
// leaves lane (m = lane & 15) four consecutive outputs n = 4 (lane >> 4) + e of every tile: no cross-lane reduction, and a weight
// fragment, once in a register, is used T times.  Rows >= M of the last tile face zeros and are never stored.  T is the template
// parameter (row buckets 16 / 32 / 48 / 64).
//
// Weights: a private LDS ring per wave, filled by LDS-DMA instructions of 4 rows x 256 contiguous bytes (whole 128-byte lines), the
// 16-byte pieces of a row rotated by the row index so that the fragment read of 16 rows at one k position falls on 16 bank groups -
// gemv_mfma_sq.hip's ring, statement for statement.  `nt`: every byte is read once per call.
//
// Activations: they do not fit in LDS (64 x 4096 B = 256 KB against 160 KB), and reading all of A from L2 for every 16-row weight
// group would cost M / 16 times the weight traffic.  So K is split: a workgroup keeps the panel A[bucket, K-slice] resident in LDS
// (64 KB at most: 4096 / 2048 / 1280 / 1024 k-bytes for the four buckets) and walks its row groups against it - four at a time, one
// per wave, quad q = blockIdx.x + i * gridDim.x - so the panel is loaded once per workgroup and the L2 traffic for A is
// bucket / (16 * groups per wave) of the weight traffic.  blockIdx.y is the K-slice.  The int32 partial sums of the slices are exact
// and order-free; every (slice, group, tile) fragment goes to the caller's workspace as the wave holds it (1 KB, fully coalesced),
// and a second small launch adds the slices in slice order, scales, applies the epilogue and stores C.  No atomics, no counter, no
// workgroup waits on another: two runs give the same bits.  No barrier in the main loop either (the ring is private, the panel is
// read-only behind the one barrier that publishes it).
//
// gemm_stream_plan() states the split (pure host code): slices are multiples of 256 bytes (of 64 where K < 256), as few as the panel
// allows, more while quads x slices leave CUs idle and a slice keeps >= 1024 bytes, then the count that balances the quads over the
// workgroups; the grid is (min(quads, CUs / slices), slices).
//
// Bounds: a weight row index is clamped to N - 1 and a 16-byte piece behind the slice's end to the block's first piece (the loads
// happen, their products face zero activations or land in outputs that are never stored); panel loads are predicated by row < M
// and k < slice length; every store by m < M and n < N.
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
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kRing = 4;           // slots of a wave's weight ring (gemv_mfma_sq.hip: deeper rings measured no faster)
constexpr int kSlot = 4096;        // a slot: one 256-byte K block of the wave's 16 rows
constexpr int kPanelBytes = 65536; // the most the activation panel takes (its row pitch of 16 bytes on top)
constexpr int kLdsLimit = 160 * 1024;
constexpr int kMinSlice = 1024;    // K bytes below which a slice is not split further to fill CUs

int stream_cus_override = 0; // tllm_gemm_stream_set_cus: tests and sweeps (0 = the device's CU count)

// T: activation tiles of 16 rows (bucket = 16 T).  kpad = the slice length ks rounded up to 256; part = the workspace.
template <int T>
__global__ __launch_bounds__(256) void gemm_stream_sq_kernel(const int8_t* __restrict__ a, const int64_t lda, const char* __restrict__ w,
    const int64_t ldw, const int M, const int N, const int K, const int ks, const int kpad, const int ngroups, i32x4* __restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = kRing, SLOT = kSlot;
    char* panel = smem + 4 * D * SLOT; // [16 T][pitch] s8, zero where row >= M or k >= klen
    const int pitch = kpad + 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: M0 and DMA bases
    const int r16 = lane & 15, g4 = lane >> 4;
    const int kbeg = (int) blockIdx.y * ks;
    const int klen = K - kbeg < ks ? K - kbeg : ks; // > 0 and a multiple of 64 (the plan has no empty slice)
    const int nblk = (klen + 255) / 256;

    // ---- this wave's weight stream: group 4 * quad + wid of the quads blockIdx.x, blockIdx.x + gridDim.x, ..
    const int nquads = (ngroups + 3) / 4;
    int nq_mine = (int) blockIdx.x < nquads ? (nquads - (int) blockIdx.x + (int) gridDim.x - 1) / (int) gridDim.x : 0;
    if (nq_mine > 0 && 4 * ((int) blockIdx.x + (nq_mine - 1) * (int) gridDim.x) + wid >= ngroups)
        --nq_mine; // the last quad may hold fewer than four groups
    const int total = nq_mine * nblk;
    const int ring_off = wid * D * SLOT;
    const uint32_t ring = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) void*) (smem + ring_off); // its LDS byte address (M0)
    auto issue = [&](int q) {
        const int gi = q / nblk, j = q - gi * nblk;
        const int g = 4 * ((int) blockIdx.x + gi * (int) gridDim.x) + wid;
        const char* base = w + (int64_t) g * 16 * ldw + kbeg + j * 256;
        const uint32_t slot = ring + (uint32_t) (q % D) * SLOT;
        const int last_row = N - 1 - g * 16; // >= 0: rows behind it are clamped onto it
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int row = 4 * i + g4;
            const int piece = (r16 + row) & 15; // rotated by the row (see the fragment read)
            const uint32_t off = (uint32_t) (row < last_row ? row : last_row) * (uint32_t) ldw
                + (j * 256 + piece * 16 < klen ? (uint32_t) piece * 16u : 0u);
            glds16s_nt(base, off, slot + i * 1024);
        }
    };
    for (int q = 0; q < D - 1 && q < total; ++q)
        issue(q); // before the panel: the first weights do not depend on it

    // ---- the activation panel: 16 lanes take the 256 contiguous bytes of one row's block, a wave four rows per instruction
    {
        // (every load happens, from a clamped address, and is zeroed afterwards: a predicated load costs a round trip of its own)
        const int prow = tid >> 4, pcol = (tid & 15) * 16;
#pragma unroll 2
        for (int k = pcol; k < kpad; k += 256)
        {
            const int kc = k < klen ? k : 0;
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
                const bool ok = r < M && k < klen;
                *reinterpret_cast<uint4*>(panel + (size_t) r * pitch + k)
                    = make_uint4(ok ? v[t].x : 0u, ok ? v[t].y : 0u, ok ? v[t].z : 0u, ok ? v[t].w : 0u);
            }
        }
    }
    __syncthreads();

    // ---- main loop
    const char* xlane = panel + (size_t) r16 * pitch + g4 * 16;
    // fragment read of this lane inside a slot: row r16 lives in instruction r16 >> 2 at row-in-instruction r16 & 3; piece c at
    // position (c - r16) & 15
    const char* wfrag = smem + ring_off + (r16 >> 2) * 1024 + (r16 & 3) * 256;
    i32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
        acc[t] = i32x4{0, 0, 0, 0};
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
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * 4) : "memory");
            }
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const char* slot = wfrag + (q % D) * SLOT;
            const char* xk = xlane + (size_t) j * 256;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4)
            {
                const int c = c4 * 4 + g4; // 16-byte piece of the 256-byte block = this lane's share of k-step c4
                const uint4 wr = *reinterpret_cast<const uint4*>(slot + ((c - r16) & 15) * 16);
                const i32x4 wf = {(int) wr.x, (int) wr.y, (int) wr.z, (int) wr.w};
#pragma unroll
                for (int t = 0; t < T; ++t)
                {
                    const uint4 xr = *reinterpret_cast<const uint4*>(xk + (size_t) t * 16 * pitch + c4 * 64);
                    const i32x4 xa = {(int) xr.x, (int) xr.y, (int) xr.z, (int) xr.w};
                    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, xa, acc[t], 0, 0, 0);
                }
            }
            // the slot is free for the DMA of the next iteration only once its fragments are in registers
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        // the accumulators through a VGPR operand HERE, in the MFMAs' own block (gemv_mfma_sq.hip finish_group: hipcc otherwise
        // reads them at the head of the next block, ahead of the wait states the last MFMA is owed)
#pragma unroll
        for (int t = 0; t < T; ++t)
            asm volatile("; accumulator out of the matrix pipe" : "+v"(acc[t]));
        const int g = 4 * ((int) blockIdx.x + gi * (int) gridDim.x) + wid;
        i32x4* dst = part + (((size_t) blockIdx.y * ngroups + g) * T) * 64 + lane;
#pragma unroll
        for (int t = 0; t < T; ++t)
        {
            dst[(size_t) t * 64] = acc[t];
            acc[t] = i32x4{0, 0, 0, 0};
        }
    }
}

struct FinishArgs
{
    const i32x4* part;
    int32_t slices, ngroups, tiles;
    int32_t M, N, out_dtype, per_channel, per_token;
    const float* scale_col;
    const float* scale_row;
    const uint16_t* residual;
    void* c;
    int64_t ldc;
};

// one wave per (group, tile) fragment: the slices' partial sums in slice order, the scales, the epilogue, the store
__global__ __launch_bounds__(256) void gemm_stream_sq_finish_kernel(const FinishArgs f)
{
    const int lane = threadIdx.x & 63;
    const int frag = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (frag >= f.ngroups * f.tiles)
        return;
    const int g = frag / f.tiles, t = frag - g * f.tiles;
    const int m = t * 16 + (lane & 15), n0 = g * 16 + (lane >> 4) * 4;
    if (m >= f.M || n0 >= f.N)
        return;
    i32x4 v = {0, 0, 0, 0};
    for (int s = 0; s < f.slices; ++s)
        v += f.part[(((size_t) s * f.ngroups + g) * f.tiles + t) * 64 + lane];
    const float rs = f.scale_row ? f.scale_row[f.per_token ? m : 0] : 1.f;
    const int64_t o = (int64_t) m * f.ldc + n0;
    const int nv = f.N - n0 < 4 ? f.N - n0 : 4; // outputs of this lane that exist
    float r0[4];
    uint16_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
    {
        const int n = e < nv ? n0 + e : n0;
        r0[e] = (float) v[e] * (f.scale_col[f.per_channel ? n : 0] * rs);
        h[e] = f2h(r0[e]);
    }
    if (f.residual)
    {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            h[e] = f2h(h2f(h[e]) + h2f(f.residual[o + (e < nv ? e : 0)]));
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
            *reinterpret_cast<float4*>(y) = make_float4(r0[0], r0[1], r0[2], r0[3]);
        else
            for (int e = 0; e < nv; ++e)
                y[e] = r0[e];
    }
}

template <int T>
int launch_bucket(const GemmParams& p, const GemmStreamPlan& plan, void* workspace, hipStream_t stream)
{
    auto kfn = gemm_stream_sq_kernel<T>;
    launch_util::ensure_dynamic_lds(reinterpret_cast<const void*>(kfn), kLdsLimit); // the most any plan asks for: set once
    const int kpad = (plan.k_slice + 255) / 256 * 256;
    hipLaunchKernelGGL(kfn, dim3((unsigned) plan.grid_x, (unsigned) plan.k_slices), dim3(256), (size_t) plan.lds_bytes, stream,
        reinterpret_cast<const int8_t*>(p.a), p.lda, reinterpret_cast<const char*>(p.w), p.ldw, p.M, p.N, p.K, plan.k_slice, kpad,
        plan.row_groups, reinterpret_cast<i32x4*>(workspace));
    return launch_util::check_launch("gemm_stream_sq");
}

} // namespace

void gemm_stream_set_cus(int cus)
{
    stream_cus_override = cus > 0 ? cus : 0;
}

int gemm_stream_cus()
{
    return stream_cus_override ? stream_cus_override : launch_util::device_cus();
}

GemmStreamPlan gemm_stream_plan(int32_t M, int32_t N, int32_t K, int32_t cus)
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
    const int ks_max = (kPanelBytes / plan.bucket) & ~255; // 4096 / 2048 / 1280 / 1024
    plan.row_groups = (N + 15) / 16;
    const int nquads = (plan.row_groups + 3) / 4;
    // the fewest slices the panel allows, more while quads x slices leave CUs idle; from there up to `most` the count that leaves
    // the longest-running workgroup the fewest weight bytes (rounds of the grid x quads per workgroup x slice length: 192 quads in
    // 2 slices on 256 CUs are 2 quads for half of the workgroups and 1 for the rest, in 4 slices 3 for every one), ties to the fewer
    const int fill = (cus + nquads - 1) / nquads, most = K / kMinSlice > 1 ? K / kMinSlice : 1;
    const int lo = std::max((K + ks_max - 1) / ks_max, std::min(fill, most));
    int64_t best = -1;
    for (int s = lo; s <= std::max(lo, std::min(most, 4 * lo)); ++s)
    {
        int ks = (K + s - 1) / s;
        ks = K < 256 ? K : std::min((ks + 255) / 256 * 256, ks_max);
        const int slices = (K + ks - 1) / ks;
        const int gx = std::min(nquads, std::max(1, cus / slices));
        const int64_t cost = (int64_t) ((gx * slices + cus - 1) / cus) * ((nquads + gx - 1) / gx) * ks;
        if (best < 0 || cost < best)
        {
            best = cost;
            plan.k_slice = ks;
            plan.k_slices = slices;
            plan.grid_x = gx;
        }
    }
    const int ks = plan.k_slice;
    plan.groups_per_workgroup = (nquads + plan.grid_x - 1) / plan.grid_x * 4;
    plan.lds_bytes = 4 * kRing * kSlot + plan.bucket * ((ks + 255) / 256 * 256 + 16);
    plan.workspace_bytes = (int64_t) plan.k_slices * plan.row_groups * (plan.bucket / 16) * 1024;
    return plan;
}

// 0 launched, -1 launch error, 1 refused (the reason is the error string; nothing is enqueued)
int launch_gemm_stream(const GemmParams& p, void* workspace, int64_t workspace_bytes, hipStream_t stream)
{
    auto refuse = [&](const char* why) {
        set_error("gemm_stream: %d x %d x %d refused: %s", p.M, p.N, p.K, why);
        return 1;
    };
    auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (p.wtype != W_INT8_SQ)
        return refuse("the weight type is not SmoothQuant int8 (W_INT8_SQ)");
    const int cus = gemm_stream_cus();
    const GemmStreamPlan plan = gemm_stream_plan(p.M, p.N, p.K, cus);
    if (plan.refused)
        return refuse(plan.refused);
    if (p.silu_gate || p.w2)
        return refuse("a SwiGLU epilogue is not served");
    if (p.out_dtype != DT_HALF && p.out_dtype != DT_FLOAT)
        return refuse("the output type is neither fp16 nor fp32");
    if (p.residual && p.out_dtype != DT_HALF)
        return refuse("a residual needs fp16 output");
    if (!p.a || !p.w || !p.c || !p.scale_col)
        return refuse("a null operand");
    if (misaligned(p.a, 16) || (p.lda & 15) || p.lda < p.K)
        return refuse("A is not 16-byte aligned, or lda is below K or not a multiple of 16");
    if (misaligned(p.w, 16) || (p.ldw & 15) || p.ldw < p.K || (int64_t) 16 * p.ldw + 256 >= (1ll << 32))
        return refuse("W is not 16-byte aligned, or ldw is below K, not a multiple of 16 or beyond 32-bit offsets in a row group");
    if (misaligned(p.c, p.out_dtype == DT_HALF ? 8 : 16) || (p.ldc & 3) || p.ldc < p.N)
        return refuse("C is not aligned to four outputs, or ldc is below N or not a multiple of 4");
    if (p.residual && misaligned(p.residual, 2))
        return refuse("the residual is not aligned");
    if (!workspace || misaligned(workspace, 16) || workspace_bytes < plan.workspace_bytes)
        return refuse("the workspace is null, not 16-byte aligned or smaller than gemm_stream_plan's workspace_bytes");
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
    f.part = reinterpret_cast<const i32x4*>(workspace);
    f.slices = plan.k_slices;
    f.ngroups = plan.row_groups;
    f.tiles = plan.bucket / 16;
    f.M = p.M;
    f.N = p.N;
    f.out_dtype = p.out_dtype;
    f.per_channel = p.per_channel;
    f.per_token = p.per_token;
    f.scale_col = reinterpret_cast<const float*>(p.scale_col);
    f.scale_row = p.scale_row;
    f.residual = reinterpret_cast<const uint16_t*>(p.residual);
    f.c = p.c;
    f.ldc = p.ldc;
    const int frags = f.ngroups * f.tiles;
    hipLaunchKernelGGL(gemm_stream_sq_finish_kernel, dim3((unsigned) ((frags + 3) / 4)), dim3(256), 0, stream, f);
    return launch_util::check_launch("gemm_stream_sq_finish");
}

} // namespace kernels
} // namespace tllm
