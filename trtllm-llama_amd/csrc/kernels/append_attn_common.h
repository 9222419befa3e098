// What the units of the append attention share (append_attn.hip: launches (a) - (d) and the launcher; append_attn_split.hip: the
// split-KV kernel and its merge): the cache element kinds and the one way a cache element becomes fp16.
#pragma once
#include "dev_utils.h"
#include "kernels.h"

namespace tllm
{
namespace kernels
{
namespace append_attn
{
using namespace dev;

__device__ __forceinline__ int clampi(int v, int lo, int hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// cache element kinds of the instances: 0 fp16, 1 int8, 2 fp8 (E4M3)
constexpr int kv_kind(int32_t kv_dtype)
{
    return kv_dtype == DT_INT8 ? 1 : (kv_dtype == DT_FP8 ? 2 : 0);
}

// 8 cache elements as they lie in memory: 16 bytes of fp16, 8 bytes of a one-byte type
template <int KV>
struct kv_raw8
{
    typedef uint2 type;
};
template <>
struct kv_raw8<0>
{
    typedef uint4 type;
};

// 8 cache elements -> 8 fp16: the value of the byte itself for the one-byte types (exact; the scale is applied by the caller)
template <int KV>
__device__ __forceinline__ uint4 kv8_to_h8(const typename kv_raw8<KV>::type q)
{
    if constexpr (KV == 0)
        return q;
    else if constexpr (KV == 2)
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

template <int KV>
__device__ __forceinline__ uint4 load_kv8(const char* ptr)
{
    return kv8_to_h8<KV>(*reinterpret_cast<const typename kv_raw8<KV>::type*>(ptr));
}

// append_attn_split.hip: the partial and the merge launch of APPEND_ATTN_SPLIT on a checked AppendAttnParams (launch (a) has been
// enqueued, the workspace holds plan.workspace_bytes); 0 or -1 with the error set
int launch_append_attn_split(const AppendAttnParams& p, const AppendSplitPlan& plan, hipStream_t stream);

} // namespace append_attn
} // namespace kernels
} // namespace tllm
