// tllm_sampling_config_t (include/tllm_runtime_api.h) -> kernels::SamplingParams: the one validation and the one copy that
// the session's sampler (tllm_session_set_sampling) and the stand-alone one (tllm_sample_tokens) share.
#pragma once
#include "../../../include/tllm_runtime_api.h"
#include "../kernels/kernels.h"
#include "../plugins/plugin_base.h"

namespace tllm
{
namespace runtime
{

inline void sampling_from_config(kernels::SamplingParams& sp, const tllm_sampling_config_t& c)
{
    sp.top_k = c.top_k;
    sp.top_p = c.top_p;
    sp.temperature = c.temperature;
    sp.repetition_penalty = c.repetition_penalty;
    sp.presence_penalty = c.presence_penalty;
    sp.min_length = c.min_length;
    sp.random_seed = c.random_seed;
}

inline int check_sampling_config(const char* who, const tllm_sampling_config_t& c)
{
    if (!(c.temperature > 0.f) || c.top_k < 0 || !(c.top_p >= 0.f) || !(c.repetition_penalty > 0.f))
    {
        set_error("%s: needs temperature > 0, top_k >= 0, top_p >= 0, repetition_penalty > 0", who);
        return 1;
    }
    if (c.repetition_penalty != 1.f && c.presence_penalty != 0.f)
    {
        // layers/baseSamplingLayer.cpp:149-167
        set_error("%s: repetition_penalty and presence_penalty are mutually exclusive", who);
        return 1;
    }
    return 0;
}

} // namespace runtime
} // namespace tllm
