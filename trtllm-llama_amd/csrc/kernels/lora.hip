// LoRA adapters per row: the two skinny products behind a base projection (kernels.h LoraShrinkParams / LoraExpandParams state
// the rule).  Both are latency- and L2-bound: an adapter's A and B of one site are a few hundred KB, read
// with 16-byte loads, reduced on the wave64 DPP network, no atomics.  Which adapter a row takes is read from device memory, so a
// captured launch serves every selection.
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

constexpr int kShrinkRows = 8; // rows of x per shrink workgroup

__device__ __forceinline__ float dot8(const uint4& a, const uint4& b, float acc)
{
    acc = dot2(a.x, b.x, acc);
    acc = dot2(a.y, b.y, acc);
    acc = dot2(a.z, b.z, acc);
    return dot2(a.w, b.w, acc);
}

// RMSNorm of 8 elements with the rounding points of the GEMV's prologue (gemv_impl.h): n = f16(x * inv), xh = f16(n * gamma)
__device__ __forceinline__ uint4 norm8(const uint4& x, const uint4& g, float inv)
{
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, gs[4] = {g.x, g.y, g.z, g.w};
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        h2_t h = u32_as_h2(xs[q]);
        const h2_t gg = u32_as_h2(gs[q]);
        const float n0 = h2f(f2h((float) h.x * inv)), n1 = h2f(f2h((float) h.y * inv));
        h.x = (_Float16) (n0 * (float) gg.x);
        h.y = (_Float16) (n1 * (float) gg.y);
        o[q] = h2_as_u32(h);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// One workgroup: JR rows of A of adapter blockIdx.y against the rows of x tile blockIdx.z that take that adapter.  The 256 threads
// split K in 16-byte pieces; a piece of A is loaded once and meets the piece of every row of the tile that takes the adapter.
// A row of the tile that does not take it costs nothing: `mask` is uniform, so every loop over the tile's rows skips it with a
// scalar branch, and no row of another adapter or of none is ever read.  ALL: every row of the tile takes the adapter (the
// prefill's usual tile) - the same loops without the branches, so that the tile's eight loads of a piece are issued together.
template <bool NORM, int JR, bool ALL>
__device__ __forceinline__ void lora_shrink_tile(const LoraShrinkParams& p, const LoraAdapterRec& rec, uint32_t mask, int m0, int j0,
    float* red)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int K8 = p.K >> 3;
    auto on = [&](int i) { return ALL || ((mask >> i) & 1); };
    const uint4* xr[kShrinkRows];
#pragma unroll
    for (int i = 0; i < kShrinkRows; ++i)
        xr[i] = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(p.x) + (int64_t) (m0 + i) * p.ldx); // read only if on(i)
    float inv[kShrinkRows];
#pragma unroll
    for (int i = 0; i < kShrinkRows; ++i)
        inv[i] = 1.f;
    if constexpr (NORM)
    {
        float ss[kShrinkRows];
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
            ss[i] = 0.f;
        for (int c = tid; c < K8; c += 256)
        {
#pragma unroll
            for (int i = 0; i < kShrinkRows; ++i)
            {
                if (!on(i))
                    continue;
                float f[8];
                h8_to_f(xr[i][c], f);
#pragma unroll
                for (int e = 0; e < 8; e += 2)
                    ss[i] += f[e] * f[e] + f[e + 1] * f[e + 1];
            }
        }
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
        {
            if (!on(i))
                continue;
            const float v = wave_sum(ss[i]);
            if (lane == 0)
                red[i * 4 + wid] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
            if (on(i))
                inv[i] = 1.0f / sqrtf((red[i * 4] + red[i * 4 + 1] + red[i * 4 + 2] + red[i * 4 + 3]) / (float) p.K + p.eps);
        __syncthreads(); // red is written again below
    }
    const uint4* ar[JR];
#pragma unroll
    for (int jr = 0; jr < JR; ++jr)
    {
        const int j = j0 + jr < p.R ? j0 + jr : p.R - 1; // clamped; the row beyond R is not written
        ar[jr] = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(rec.a) + (int64_t) j * p.K);
    }
    const uint4* gam = reinterpret_cast<const uint4*>(p.gamma);
    float acc[JR][kShrinkRows];
#pragma unroll
    for (int jr = 0; jr < JR; ++jr)
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
            acc[jr][i] = 0.f;
    for (int c = tid; c < K8; c += 256)
    {
        uint4 av[JR];
#pragma unroll
        for (int jr = 0; jr < JR; ++jr)
            av[jr] = ar[jr][c];
        uint4 gv = make_uint4(0, 0, 0, 0);
        if constexpr (NORM)
            gv = gam[c];
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
        {
            if (!on(i))
                continue;
            uint4 xv = xr[i][c];
            if constexpr (NORM)
                xv = norm8(xv, gv, inv[i]);
#pragma unroll
            for (int jr = 0; jr < JR; ++jr)
                acc[jr][i] = dot8(av[jr], xv, acc[jr][i]);
        }
    }
#pragma unroll
    for (int jr = 0; jr < JR; ++jr)
#pragma unroll
        for (int i = 0; i < kShrinkRows; ++i)
        {
            if (!on(i))
                continue;
            const float v = wave_sum(acc[jr][i]);
            if (lane == 0)
                red[(jr * kShrinkRows + i) * 4 + wid] = v;
        }
    __syncthreads();
    if (tid < JR * kShrinkRows)
    {
        const int jr = tid / kShrinkRows, i = tid % kShrinkRows;
        if (((mask >> i) & 1) && j0 + jr < p.R)
            p.t[(int64_t) (m0 + i) * p.R + j0 + jr] = red[tid * 4] + red[tid * 4 + 1] + red[tid * 4 + 2] + red[tid * 4 + 3];
    }
}

template <bool NORM, int JR>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const LoraShrinkParams p)
{
    __shared__ float red[JR * kShrinkRows * 4];
    const int a = blockIdx.y, m0 = blockIdx.z * kShrinkRows, j0 = blockIdx.x * JR;
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < kShrinkRows; ++i)
        if (m0 + i < p.M && p.row_adapter[m0 + i] == a)
            mask |= 1u << i;
    if (!mask) // uniform: the adapter of this workgroup serves no row of the tile
        return;
    const LoraAdapterRec rec = p.table[a];
    if (mask == (1u << kShrinkRows) - 1)
        lora_shrink_tile<NORM, JR, true>(p, rec, mask, m0, j0, red);
    else
        lora_shrink_tile<NORM, JR, false>(p, rec, mask, m0, j0, red);
}

// One workgroup: 256 / LPR output columns (LPR = r / 8 lanes per B row, one 16-byte load each) for a tile of MT rows, whose t rows
// and adapters are staged in LDS.  Per adapter that the tile uses the B row is loaded once and serves the tile's rows of it.
template <int LPR, int MT>
__global__ __launch_bounds__(256) void lora_expand_kernel(const LoraExpandParams p)
{
    constexpr int r = 8 * LPR;
    __shared__ __attribute__((aligned(16))) float ts[MT * kLoraMaxSegments * r];
    __shared__ int ra[MT];
    const int tid = threadIdx.x, m0 = blockIdx.y * MT, R = p.nseg * r;
    if (tid < MT)
    {
        const int m = m0 + tid;
        int v = m < p.M ? p.row_adapter[m] : -1;
        if (v < 0 || v >= p.num_adapters)
            v = -1;
        ra[tid] = v;
    }
    __syncthreads();
    uint32_t used = 0; // adapters of the tile (uniform)
#pragma unroll 8
    for (int i = 0; i < MT; ++i)
        used |= ra[i] >= 0 ? 1u << ra[i] : 0u;
    if (!used)
        return;
    for (int idx = tid; idx < MT * R; idx += 256)
    {
        const int i = idx / R;
        if (ra[i] >= 0)
            ts[idx] = p.t[(int64_t) (m0 + i) * R + (idx - i * R)];
    }
    __syncthreads();
    const int n1 = p.seg_n[0], n2 = n1 + p.seg_n[1], ntot = n2 + p.seg_n[2];
    const int n = blockIdx.x * (256 / LPR) + tid / LPR, sub = tid % LPR;
    const bool valid = n < ntot;
    const int nc = valid ? n : ntot - 1; // clamped for the loads; nothing is stored for it
    const int g = (nc >= n1 ? 1 : 0) + (nc >= n2 ? 1 : 0);
    const int nl = nc - (g == 0 ? 0 : (g == 1 ? n1 : n2));
    uint16_t* yb = reinterpret_cast<uint16_t*>(g == 0 ? p.seg_y[0] : (g == 1 ? p.seg_y[1] : p.seg_y[2])) + nl;
    const int64_t ldy = g == 0 ? p.seg_ldy[0] : (g == 1 ? p.seg_ldy[1] : p.seg_ldy[2]);
    for (int a = 0; a < p.num_adapters; ++a)
    {
        if (!((used >> a) & 1))
            continue;
        const LoraAdapterRec rec = p.table[a];
        float bf[8];
        h8_to_f(*reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(rec.b) + (int64_t) nc * r + sub * 8), bf);
        for (int i = 0; i < MT; ++i)
        {
            if (ra[i] != a) // uniform
                continue;
            const float* tp = ts + i * R + g * r + sub * 8;
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                d = fmaf(bf[e], tp[e], d);
            d = group_sum<LPR>(d);
            if (valid && sub == 0)
            {
                uint16_t* y = yb + (int64_t) (m0 + i) * ldy;
                *y = f2h(h2f(*y) + rec.scale * d);
            }
        }
    }
}

__global__ __launch_bounds__(256) void lora_row_adapter_kernel(int32_t* rows, const int32_t* sel, int32_t batch, int32_t M,
    int32_t rows_per_seq, const int32_t* cu)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M)
        return;
    int b = -1;
    if (rows_per_seq > 0)
        b = m / rows_per_seq;
    else
        for (int i = 0; i < batch; ++i)
            if (m >= cu[i] && m < cu[i + 1])
                b = i;
    rows[m] = (b >= 0 && b < batch) ? sel[b] : -1;
}

int check_common(const char* who, int32_t M, const int32_t* row_adapter, const LoraAdapterRec* table, int32_t num_adapters)
{
    if (M < 1 || M > 65535 * kShrinkRows || !row_adapter || !table || num_adapters < 1 || num_adapters > kLoraMaxAdapters)
    {
        set_error("%s: bad arguments (M %d, num_adapters %d in [1, %d], row_adapter / table %s)", who, M, num_adapters,
            kLoraMaxAdapters, row_adapter && table ? "set" : "null");
        return -1;
    }
    return 0;
}

} // namespace

int launch_lora_shrink(const LoraShrinkParams& p, hipStream_t stream)
{
    if (check_common("launch_lora_shrink", p.M, p.row_adapter, p.table, p.num_adapters))
        return -1;
    if (p.K < 8 || p.K % 8 || p.R < 1 || !p.x || !p.t || p.ldx < p.K || p.ldx % 8 || (reinterpret_cast<uintptr_t>(p.x) & 15))
    {
        set_error("launch_lora_shrink: K %d (%% 8 == 0), R %d, ldx %lld (>= K, %% 8 == 0) and a 16-byte aligned x are required", p.K,
            p.R, (long long) p.ldx);
        return -1;
    }
    if (p.pro != PRO_NONE && p.pro != PRO_RMSNORM)
    {
        set_error("launch_lora_shrink: prologue %d is neither PRO_NONE nor PRO_RMSNORM", p.pro);
        return -1;
    }
    const bool norm = p.pro == PRO_RMSNORM;
    if (norm && (!p.gamma || (reinterpret_cast<uintptr_t>(p.gamma) & 15)))
    {
        set_error("launch_lora_shrink: PRO_RMSNORM needs a 16-byte aligned gamma");
        return -1;
    }
    const int tiles = (p.M + kShrinkRows - 1) / kShrinkRows;
    const int jr = p.M <= kShrinkRows ? 1 : 4; // decode: a workgroup per A row, so that the site's A bytes stream from many CUs
    const dim3 grid((p.R + jr - 1) / jr, p.num_adapters, tiles);
    if (jr == 1)
    {
        if (norm)
            hipLaunchKernelGGL((lora_shrink_kernel<true, 1>), grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((lora_shrink_kernel<false, 1>), grid, dim3(256), 0, stream, p);
    }
    else
    {
        if (norm)
            hipLaunchKernelGGL((lora_shrink_kernel<true, 4>), grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((lora_shrink_kernel<false, 4>), grid, dim3(256), 0, stream, p);
    }
    return check_launch("lora_shrink");
}

namespace
{
template <int MT>
void expand_dispatch(const LoraExpandParams& p, int ntot, hipStream_t stream)
{
    const int lpr = p.r / 8;
    const dim3 grid((ntot + 256 / lpr - 1) / (256 / lpr), (p.M + MT - 1) / MT);
    switch (lpr)
    {
    case 1: hipLaunchKernelGGL((lora_expand_kernel<1, MT>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((lora_expand_kernel<2, MT>), grid, dim3(256), 0, stream, p); break;
    case 4: hipLaunchKernelGGL((lora_expand_kernel<4, MT>), grid, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((lora_expand_kernel<8, MT>), grid, dim3(256), 0, stream, p); break;
    }
}
} // namespace

int launch_lora_expand(const LoraExpandParams& p, hipStream_t stream)
{
    if (check_common("launch_lora_expand", p.M, p.row_adapter, p.table, p.num_adapters))
        return -1;
    if ((p.r != 8 && p.r != 16 && p.r != 32 && p.r != 64) || p.nseg < 1 || p.nseg > kLoraMaxSegments || !p.t)
    {
        set_error("launch_lora_expand: r %d must be 8, 16, 32 or 64, nseg %d in [1, %d], t set", p.r, p.nseg, kLoraMaxSegments);
        return -1;
    }
    LoraExpandParams q = p;
    int64_t ntot = 0;
    for (int g = 0; g < kLoraMaxSegments; ++g)
    {
        if (g >= p.nseg) // the kernel finds a column's segment by the running sums: an unused segment is empty
        {
            q.seg_n[g] = 0;
            q.seg_y[g] = nullptr;
            q.seg_ldy[g] = 0;
            continue;
        }
        if (p.seg_n[g] < 1 || !p.seg_y[g] || p.seg_ldy[g] < p.seg_n[g])
        {
            set_error("launch_lora_expand: segment %d has N %d, ldy %lld, y %s", g, p.seg_n[g], (long long) p.seg_ldy[g],
                p.seg_y[g] ? "set" : "null");
            return -1;
        }
        ntot += p.seg_n[g];
    }
    if (ntot > (int64_t) 1 << 30)
    {
        set_error("launch_lora_expand: %lld output columns", (long long) ntot);
        return -1;
    }
    if (p.M <= 8)
        expand_dispatch<8>(q, (int) ntot, stream);
    else
        expand_dispatch<32>(q, (int) ntot, stream);
    return check_launch("lora_expand");
}

int launch_lora_row_adapter(int32_t* rows, const int32_t* sel, int32_t batch, int32_t M, int32_t rows_per_seq,
    const int32_t* cu_seqlens, hipStream_t stream)
{
    if (!rows || !sel || batch < 1 || M < 1 || (rows_per_seq <= 0 && !cu_seqlens))
    {
        set_error("launch_lora_row_adapter: bad arguments");
        return -1;
    }
    hipLaunchKernelGGL(lora_row_adapter_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, rows, sel, batch, M, rows_per_seq,
        cu_seqlens);
    return check_launch("lora_row_adapter");
}

} // namespace kernels
} // namespace tllm
