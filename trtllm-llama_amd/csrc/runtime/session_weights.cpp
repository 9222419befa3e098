// Session creation and weights: configuration text -> fields, named tensors -> the Linear / Layer records the schedules
// run on, and the engine file ("TLLMENG1", tensorrt_llm/builder.py) that carries both.
#include "engine_check.h"
#include "session.h"
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

namespace
{
size_t dtype_bytes(int32_t t)
{
    switch (t)
    {
    case TLLM_FLOAT:
    case TLLM_INT32: return 4;
    case TLLM_HALF: return 2;
    default: return 1;
    }
}
} // namespace

const TensorRec* tllm_session::find(const std::string& name, bool required)
{
    auto it = tensors.find(name);
    if (it == tensors.end())
    {
        if (required)
            set_error("session: missing tensor '%s'", name.c_str());
        return nullptr;
    }
    return &it->second;
}

int tllm_session::want(const TensorRec* t, const std::string& name, int32_t dtype, int64_t numel)
{
    if (!t)
        return 1;
    if (t->dtype != dtype || t->numel() != numel)
    {
        set_error("session: tensor '%s' has dtype %d / %lld elements, expected dtype %d / %lld", name.c_str(),
            t->dtype, (long long) t->numel(), dtype, (long long) numel);
        return 1;
    }
    return 0;
}

int tllm_session::resolve_linear(const std::string& prefix, int N, int K, Linear& L, bool force_fp16)
{
    L.N = N;
    L.K = K;
    const std::string wn = prefix + ".weight";
    const TensorRec* w = find(wn);
    if (!w)
        return 1;
    if (force_fp16 || (!sq && !woq))
    {
        RUN(want(w, wn, TLLM_HALF, (int64_t) N * K));
        L.wtype = W_FP16;
        L.w = w->dev;
        L.ldw = (int64_t) K * 2;
        return 0;
    }
    if (woq)
    {
        // processed bytes, declared fp32 [K, N/4 | N/8] (reference view) or int8 [N, ldw]
        L.wtype = wtype;
        L.ldw = layout::row_bytes(wtype, K);
        if ((int64_t) w->bytes != (int64_t) N * L.ldw)
        {
            set_error("session: tensor '%s' has %zu bytes, expected %lld (processed weight-only layout)",
                wn.c_str(), w->bytes, (long long) N * L.ldw);
            return 1;
        }
        L.w = w->dev;
        const TensorRec* s = find(prefix + ".per_channel_scale");
        RUN(want(s, prefix + ".per_channel_scale", TLLM_HALF, N));
        L.scale_col = s->dev;
        return 0;
    }
    // SmoothQuant: int8 [N, K] (or fp32 view [N, K/4])
    L.wtype = W_INT8_SQ;
    L.ldw = K;
    if ((int64_t) w->bytes != (int64_t) N * K || (K % 16))
    {
        set_error("session: tensor '%s' must hold N*K = %lld int8 values with K %% 16 == 0", wn.c_str(),
            (long long) N * K);
        return 1;
    }
    L.w = w->dev;
    const TensorRec* s = find(prefix + ".per_channel_scale");
    if (!s)
        return 1;
    L.per_channel = s->numel() == N ? 1 : 0;
    if (s->dtype != TLLM_FLOAT || (s->numel() != N && s->numel() != 1))
    {
        set_error("session: '%s.per_channel_scale' must be f32 [1,%d] or [1,1]", prefix.c_str(), N);
        return 1;
    }
    L.scale_col = s->dev;
    if (!per_token)
    {
        const TensorRec* a = find(prefix + ".act_scale");
        RUN(want(a, prefix + ".act_scale", TLLM_FLOAT, 1));
        L.act_scale = static_cast<const float*>(a->dev);
    }
    return 0;
}

int tllm_session::scalar_f32(const std::string& name, const float** out)
{
    const TensorRec* t = find(name);
    RUN(want(t, name, TLLM_FLOAT, 1));
    *out = static_cast<const float*>(t->dev);
    return 0;
}

extern "C" {

tllm_session_t tllm_session_create(const char* config_text)
{
    if (!config_text)
    {
        set_error("tllm_session_create: null config");
        return nullptr;
    }
    auto s = std::make_unique<tllm_session>();
    std::istringstream in(config_text);
    std::string line;
    std::map<std::string, std::string> kv;
    while (std::getline(in, line))
    {
        const size_t eq = line.find('=');
        if (eq == std::string::npos)
            continue;
        auto trim = [](std::string v) {
            const size_t a = v.find_first_not_of(" \t\r");
            const size_t b = v.find_last_not_of(" \t\r");
            return a == std::string::npos ? std::string() : v.substr(a, b - a + 1);
        };
        kv[trim(line.substr(0, eq))] = trim(line.substr(eq + 1));
    }
    auto geti = [&](const char* k, int def) { return kv.count(k) ? atoi(kv[k].c_str()) : def; };
    s->num_layers = geti("num_layers", 0);
    s->num_heads = geti("num_heads", 0);
    s->num_kv_heads = geti("num_kv_heads", s->num_heads);
    s->hidden = geti("hidden_size", 0);
    s->inter = geti("inter_size", 0);
    s->vocab = geti("vocab_size", 0);
    s->max_pos = geti("max_position_embeddings", 2048);
    s->tp = geti("tp_size", 1);
    s->rank = geti("tp_rank", 0);
    s->quant_mode = geti("quant_mode", 0);
    s->neox = geti("neox_rotary_style", 1);
    s->force_comm = geti("force_comm", 0) != 0;
    s->no_comm = geti("no_comm", 0) != 0;
    s->debug_taps = geti("debug_taps", 0) != 0;
    s->fuse_qkv_cfg = geti("fuse_qkv_attention", -1);
    s->fuse_o_cfg = geti("fuse_o_projection", -1);
    s->fuse_mlp_cfg = geti("fuse_mlp", 0);
    s->fused_max_spins = geti("fused_max_spins", -1);
    s->head_resident_cfg = geti("head_resident_pct", -1);
    s->greedy_partials_cfg = geti("greedy_partials", 1);
    s->dual_mlp_cfg = geti("dual_mlp_gemm", -1);
    s->score_chunk_cfg = geti("score_chunk_rows", 0);
    s->fused_timeline = geti("fused_timeline", 0) != 0;
    if (kv.count("gemm_tactics") && !kv["gemm_tactics"].empty())
    {
        // the prefill GEMM kernels the builder's on-device profile chose (engine header; Builder.build_engine)
        if (gemm_tactics_import(kv["gemm_tactics"].c_str()) < 0)
            return nullptr;
    }
    s->packed = geti("remove_input_padding", 0) != 0;
    s->paged_kv = geti("paged_kv_cache", 0) != 0;
    s->tokens_per_block = geti("tokens_per_block", 64);
    if (s->paged_kv && (s->tokens_per_block < 1 || (s->tokens_per_block & (s->tokens_per_block - 1))))
    {
        set_error("tllm_session_create: tokens_per_block must be a power of two (got %d)", s->tokens_per_block);
        return nullptr;
    }
    s->paged_append = geti("paged_append", 0) != 0;
    if (s->paged_append && !s->paged_kv)
    {
        set_error("tllm_session_create: paged_append = 1 needs paged_kv_cache = 1 (the append passes of a linear cache need no key)");
        return nullptr;
    }
    if (kv.count("rms_norm_eps"))
        s->eps = (float) atof(kv["rms_norm_eps"].c_str());
    if (kv.count("weight_only_precision"))
        s->wo_precision = kv["weight_only_precision"];
    if (kv.count("network_json"))
        s->network_json = kv["network_json"];
    if (s->num_layers <= 0 || s->num_heads <= 0 || s->hidden <= 0 || s->inter <= 0 || s->vocab <= 0 || s->tp < 1
        || s->rank < 0 || s->rank >= s->tp)
    {
        set_error("tllm_session_create: num_layers/num_heads/hidden_size/inter_size/vocab_size/tp_size/tp_rank invalid");
        return nullptr;
    }
    if (s->hidden % s->num_heads || s->num_heads % s->tp || s->inter % s->tp)
    {
        set_error("tllm_session_create: heads must divide hidden, tp must divide heads and inter_size");
        return nullptr;
    }
    s->Dh = s->hidden / s->num_heads;
    s->Hr = s->num_heads / s->tp;
    s->Dr = s->Hr * s->Dh;
    if (s->num_kv_heads < 1 || s->num_kv_heads > s->num_heads || s->num_heads % s->num_kv_heads)
    {
        set_error("tllm_session_create: num_kv_heads %d must divide num_heads %d", s->num_kv_heads, s->num_heads);
        return nullptr;
    }
    if (s->num_kv_heads % s->tp)
    {
        set_error("tllm_session_create: tp_size %d must divide num_kv_heads %d (K/V head replication is not built)", s->tp, s->num_kv_heads);
        return nullptr;
    }
    s->Hkvr = s->num_kv_heads / s->tp;
    s->QKVr = (s->Hr + 2 * s->Hkvr) * s->Dh;
    s->Ir = s->inter / s->tp;
    // vocab padded to a multiple of tp (PY/_utils.py:194-195, Q/llama_model.py:244)
    s->Vr = (s->vocab + s->tp - 1) / s->tp;
    const int qm = s->quant_mode;
    s->sq = (qm & QM_ACTIVATIONS) && (qm & QM_INT8_WEIGHTS);
    s->woq = !s->sq && (qm & (QM_INT8_WEIGHTS | QM_INT4_WEIGHTS));
    s->kv_dtype = (qm & QM_INT8_KV) ? DT_INT8 : ((qm & QM_FP8_KV) ? DT_FP8 : DT_HALF);
    if ((qm & QM_INT8_KV) && (qm & QM_FP8_KV))
    {
        set_error("tllm_session_create: quant_mode %d sets both INT8_KV_CACHE (32) and FP8_KV_CACHE (64); a cache has one element type", qm);
        return nullptr;
    }
    if (s->sq && s->num_kv_heads != s->num_heads)
    {
        set_error("tllm_session_create: num_kv_heads %d != num_heads %d with SmoothQuant weights is not built (the o_proj smoother folds "
                  "into v_proj rows that several query heads share)", s->num_kv_heads, s->num_heads);
        return nullptr;
    }
    s->per_token = qm & QM_PER_TOKEN;
    s->per_channel = qm & QM_PER_CHANNEL;
    if (s->woq)
        s->wtype = (qm & QM_INT4_WEIGHTS) ? W_INT4_WOQ : W_INT8_WOQ;
    else if (s->sq)
        s->wtype = W_INT8_SQ;
    for (int i = 0; i < s->tp; ++i)
        s->group.push_back(i);
    // LoRA adapters per sequence
    s->lora_rank = geti("lora_max_rank", 0);
    if (s->lora_rank != 0)
    {
        const int r = s->lora_rank;
        if (r != 8 && r != 16 && r != 32 && r != 64)
        {
            set_error("tllm_session_create: lora_max_rank %d is not 0 (off), 8, 16, 32 or 64", r);
            return nullptr;
        }
        s->lora_adapters = geti("lora_max_adapters", 1);
        if (s->lora_adapters < 1 || s->lora_adapters > kLoraMaxAdapters)
        {
            set_error("tllm_session_create: lora_max_adapters %d outside [1, %d]", s->lora_adapters, kLoraMaxAdapters);
            return nullptr;
        }
        if (s->sq)
        {
            set_error("tllm_session_create: lora_max_rank with SmoothQuant weights is not built (the smoother is folded into the norm "
                      "weights and would have to be folded into the columns of every lora_a)");
            return nullptr;
        }
        if (s->tp > 1)
        {
            set_error("tllm_session_create: lora_max_rank with tp_size %d is not built (tp_size 1 only)", s->tp);
            return nullptr;
        }
        if (s->hidden % 8 || s->Dr % 8 || s->Ir % 8)
        {
            set_error("tllm_session_create: lora_max_rank needs hidden_size and inter_size to be multiples of 8");
            return nullptr;
        }
        static const char* keys[tllm_session::LM_COUNT] = {"q", "k", "v", "o", "gate", "up", "down"};
        std::istringstream mods(kv.count("lora_target_modules") ? kv["lora_target_modules"] : std::string("q,k,v,o"));
        std::string m;
        int found = 0;
        while (std::getline(mods, m, ','))
        {
            const size_t a = m.find_first_not_of(" \t"), b = m.find_last_not_of(" \t");
            m = a == std::string::npos ? std::string() : m.substr(a, b - a + 1);
            int which = -1;
            for (int i = 0; i < tllm_session::LM_COUNT; ++i)
                if (m == keys[i])
                    which = i;
            if (which < 0)
            {
                set_error("tllm_session_create: lora_target_modules names '%s'; the modules are q,k,v,o,gate,up,down", m.c_str());
                return nullptr;
            }
            s->lora_mod[which] = true;
            ++found;
        }
        if (!found)
        {
            set_error("tllm_session_create: lora_target_modules is empty");
            return nullptr;
        }
    }
    return s.release();
}

int32_t tllm_session_set_tensor(tllm_session_t s, const char* name, int32_t dtype, const int64_t* dims, int32_t nbDims,
    const void* data, int32_t location)
{
    if (!s || !name || !dims || !data || nbDims < 0 || nbDims > 8)
    {
        set_error("tllm_session_set_tensor: bad arguments");
        return 1;
    }
    TensorRec t;
    t.dtype = dtype;
    t.dims.assign(dims, dims + nbDims);
    t.bytes = (size_t) t.numel() * dtype_bytes(dtype);
    if (location == 0)
    {
        HIP_OK(hipMalloc(&t.dev, t.bytes ? t.bytes : 16));
        t.owned = true;
        HIP_OK(hipMemcpy(t.dev, data, t.bytes, hipMemcpyHostToDevice));
    }
    else
        t.dev = const_cast<void*>(data);
    auto it = s->tensors.find(name);
    if (it != s->tensors.end() && it->second.owned && it->second.dev)
        (void) hipFree(it->second.dev);
    s->tensors[name] = t;
    s->finalized = false;
    return 0;
}

int32_t tllm_session_finalize(tllm_session_t s)
{
    if (!s)
        return 1;
    const int D = s->hidden;
    {
        const TensorRec* t = s->find("vocab_embedding.weight");
        RUN(s->want(t, "vocab_embedding.weight", TLLM_HALF, (int64_t) s->vocab * D));
        s->emb = t->dev;
        t = s->find("ln_f.weight");
        RUN(s->want(t, "ln_f.weight", TLLM_HALF, D));
        s->lnf = t->dev;
        // lm_head stays fp16 in every quantisation mode (Q/quant.py:58)
        RUN(s->resolve_linear("lm_head", s->Vr, D, s->head, true));
    }
    s->layers.assign(s->num_layers, Layer());
    for (int i = 0; i < s->num_layers; ++i)
    {
        Layer& L = s->layers[i];
        const std::string p = "layers." + std::to_string(i) + ".";
        const TensorRec* t = s->find(p + "input_layernorm.weight");
        RUN(s->want(t, p + "input_layernorm.weight", TLLM_HALF, D));
        L.ln1 = t->dev;
        t = s->find(p + "post_layernorm.weight");
        RUN(s->want(t, p + "post_layernorm.weight", TLLM_HALF, D));
        L.ln2 = t->dev;
        RUN(s->resolve_linear(p + "attention.qkv", s->QKVr, D, L.qkv));
        RUN(s->resolve_linear(p + "attention.dense", D, s->Dr, L.dense));
        RUN(s->resolve_linear(p + "mlp.fc", s->Ir, D, L.fc));
        RUN(s->resolve_linear(p + "mlp.gate", s->Ir, D, L.gate));
        RUN(s->resolve_linear(p + "mlp.proj", D, s->Ir, L.proj));
        if (s->sq && !s->per_token)
        {
            RUN(s->scalar_f32(p + "input_layernorm.scale_to_int", &L.ln1_scale));
            RUN(s->scalar_f32(p + "post_layernorm.scale_to_int", &L.ln2_scale));
            RUN(s->scalar_f32(p + "attention.quantization_scaling_factor", &L.attn_qscale));
            RUN(s->scalar_f32(p + "mlp.quantization_scaling_factor", &L.mlp_qscale));
        }
        if (s->kv_dtype != DT_HALF)
        {
            RUN(s->scalar_f32(p + "attention.kv_orig_quant_scale", &L.kv_oq));
            RUN(s->scalar_f32(p + "attention.kv_quant_orig_scale", &L.kv_qo));
        }
    }
    if (s->tp > 1 && !s->no_comm && !comm::has_comm(s->group) && !comm::p2p::attached())
    {
        set_error("session: tp_size=%d but no communicator registered (tllm_comm_init_rank / tllm_comm_p2p_attach)", s->tp);
        return 1;
    }
    s->finalized = true;
    return 0;
}

namespace
{
struct EngineEntry
{
    std::string name;
    int32_t dtype, nd;
    int64_t dims[8];
    uint64_t nbytes, offset;
};

// "TLLMENG1" | u64 header length | header text | u64 tensor count | table | 64-byte aligned data (tensorrt_llm/builder.py)
int parse_engine(const void* engine, size_t nbytes, std::string& cfg, std::vector<EngineEntry>& ents, size_t& data0)
{
    const char* p = static_cast<const char*>(engine);
    auto fail = [](const char* why) {
        set_error("engine: %s", why);
        return 1;
    };
    if (!p || nbytes < 24 || std::memcmp(p, "TLLMENG1", 8) != 0)
        return fail("not a TLLMENG1 engine");
    size_t off = 8;
    auto rd64 = [&](uint64_t* v) {
        if (off + 8 > nbytes)
            return false;
        std::memcpy(v, p + off, 8);
        off += 8;
        return true;
    };
    uint64_t hlen = 0, nt = 0;
    if (!rd64(&hlen) || hlen > nbytes || off + hlen > nbytes)
        return fail("truncated header");
    cfg.assign(p + off, p + off + hlen);
    off += hlen;
    if (!rd64(&nt) || nt > nbytes / 24)
        return fail("truncated tensor table");
    ents.assign(nt, EngineEntry());
    for (auto& e : ents)
    {
        uint32_t nl = 0;
        if (off + 4 > nbytes)
            return fail("truncated tensor table");
        std::memcpy(&nl, p + off, 4);
        off += 4;
        if (nl > nbytes || off + nl + 8 > nbytes)
            return fail("truncated tensor table");
        e.name.assign(p + off, p + off + nl);
        off += nl;
        std::memcpy(&e.dtype, p + off, 4);
        std::memcpy(&e.nd, p + off + 4, 4);
        off += 8;
        if (e.nd < 0 || e.nd > 8 || off + 8 * (size_t) e.nd + 16 > nbytes)
            return fail("bad tensor entry");
        std::memcpy(e.dims, p + off, 8 * (size_t) e.nd);
        off += 8 * (size_t) e.nd;
        std::memcpy(&e.nbytes, p + off, 8);
        std::memcpy(&e.offset, p + off + 8, 8);
        off += 16;
    }
    data0 = (off + 63) / 64 * 64;
    for (auto& e : ents)
        if (e.offset > nbytes || e.nbytes > nbytes || data0 + e.offset + e.nbytes > nbytes)
            return fail("tensor data out of range");
    return 0;
}

// The engine's traced network against the schedule a session of this configuration executes (runtime/engine_check.h).
int verify_engine_network(tllm_session_t s, const std::vector<EngineEntry>& ents)
{
    if (s->network_json.empty())
    {
        set_error("engine: no network_json in the header - not an engine built by tensorrt_llm.Builder.build_engine");
        return 1;
    }
    runtime::ScheduleDesc d;
    d.num_layers = s->num_layers;
    d.heads_per_rank = s->Hr;
    d.head_size = s->Dh;
    d.tp = s->tp;
    d.eps = s->eps;
    d.sq = s->sq;
    d.per_token = s->per_token;
    d.woq = s->woq;
    d.int4 = s->wtype == W_INT4_WOQ;
    d.int8_kv = s->kv_dtype == DT_INT8;
    d.fp8_kv = s->kv_dtype == DT_FP8;
    d.paged = s->paged_kv;
    d.packed = s->packed;
    d.neox = s->neox != 0;
    // has_per_channel_scaling of every SmoothQuant GEMM = what the scale tensor the engine carries implies (a "per tensor"
    // QKV scale is stored as one factor per channel: examples/llama_quant/weight.py)
    for (const char* n : {"attention.qkv", "attention.dense", "mlp.fc", "mlp.gate", "mlp.proj"})
    {
        int pc = s->per_channel ? 1 : 0;
        const std::string want = std::string("layers.0.") + n + ".per_channel_scale";
        for (auto& e : ents)
            if (e.name == want)
            {
                int64_t numel = 1;
                for (int i = 0; i < e.nd; ++i)
                    numel *= e.dims[i];
                pc = numel > 1 ? 1 : 0;
            }
        d.per_channel.push_back(pc);
    }
    // the fused QKV weight has the extent the configuration's num_kv_heads implies: (Hr + 2 Hkvr) Dh output channels (fp16: the
    // rows of [N, K]; weight-only / SmoothQuant: one scale per output channel)
    for (auto& e : ents)
    {
        const bool w = e.name.size() > 21 && e.name.compare(e.name.size() - 21, 21, ".attention.qkv.weight") == 0;
        const bool sc = e.name.size() > 32 && e.name.compare(e.name.size() - 32, 32, ".attention.qkv.per_channel_scale") == 0;
        int64_t numel = 1;
        for (int i = 0; i < e.nd; ++i)
            numel *= e.dims[i];
        int64_t got = -1;
        if (w && !s->sq && !s->woq && e.nd == 2)
            got = e.dims[0];
        else if (sc && numel > 1)
            got = numel;
        if (got >= 0 && got != s->QKVr)
        {
            set_error("engine: %s has %lld output channels, num_kv_heads = %d (num_heads %d, head size %d, tp %d) implies %d", e.name.c_str(),
                (long long) got, s->num_kv_heads, s->num_heads, s->Dh, s->tp, s->QKVr);
            return 1;
        }
    }
    std::string why;
    if (runtime::verify_network(s->network_json, d, why))
    {
        set_error("engine: %s", why.c_str());
        return 1;
    }
    return 0;
}
} // namespace

int32_t tllm_engine_verify(const void* engine, size_t nbytes)
{
    std::string cfg;
    std::vector<EngineEntry> ents;
    size_t data0 = 0;
    RUN(parse_engine(engine, nbytes, cfg, ents, data0));
    tllm_session_t s = tllm_session_create(cfg.c_str());
    if (!s)
        return 1;
    const int rc = verify_engine_network(s, ents);
    tllm_session_destroy(s);
    return rc;
}

tllm_session_t tllm_session_load_engine(const void* engine, size_t nbytes)
{
    return tllm_session_load_engine_keys(engine, nbytes, nullptr);
}

tllm_session_t tllm_session_load_engine_keys(const void* engine, size_t nbytes, const char* runtime_keys)
{
    std::string cfg;
    std::vector<EngineEntry> ents;
    size_t data0 = 0;
    if (parse_engine(engine, nbytes, cfg, ents, data0))
        return nullptr;
    if (runtime_keys)
    {
        // key=value lines behind the header's: only the keys that are the runtime's to set
        std::istringstream in(runtime_keys);
        std::string line;
        while (std::getline(in, line))
        {
            const size_t a = line.find_first_not_of(" \t\r"), eq = line.find('=');
            if (a == std::string::npos)
                continue;
            const size_t e = eq == std::string::npos ? std::string::npos : line.find_last_not_of(" \t\r", eq - 1);
            const std::string key = eq == std::string::npos || eq == a ? std::string() : line.substr(a, e - a + 1);
            if (key != "paged_append")
            {
                set_error("tllm_session_load_engine_keys: '%s' is not a runtime key (paged_append); the engine header holds the rest",
                    line.c_str());
                return nullptr;
            }
            cfg += "\n" + line;
        }
        cfg += "\n";
    }
    tllm_session_t s = tllm_session_create(cfg.c_str());
    if (!s)
        return nullptr;
    // the engine is what was defined: refuse a traced network that is not the schedule this session would run
    if (verify_engine_network(s, ents))
    {
        tllm_session_destroy(s);
        return nullptr;
    }
    const char* p = static_cast<const char*>(engine);
    for (auto& e : ents)
    {
        if (tllm_session_set_tensor(s, e.name.c_str(), e.dtype, e.dims, e.nd, p + data0 + e.offset, 0))
        {
            tllm_session_destroy(s);
            return nullptr;
        }
    }
    if (tllm_session_finalize(s))
    {
        tllm_session_destroy(s);
        return nullptr;
    }
    return s;
}

} // extern "C"
