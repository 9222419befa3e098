// LoRA adapters per sequence: the adapters' device buffers, the load / commit / clear / select entry points
// and the two launches (kernels/lora.hip) the schedules put behind a base projection.  The rule is stated once, in kernels.h.
//
// A site is what one base projection launch produces: the fused QKV (segments q | k | v), attention.dense, fc | gate (two
// segments, two buffers) and mlp.proj.  Per layer, site and slot the session holds A [nseg * lora_max_rank, K] and
// B [N, lora_max_rank] in fp16, zero where the adapter has no module or a lower rank, and per layer and site a table of
// {A, B, scale} records that the kernels index with the row's slot.  Everything is allocated by the first lora call or by setup,
// whichever comes first, and stays where it is until the session is destroyed: commit and clear rewrite contents, select
// rewrites the device array of slots, and a captured step graph reads all of it through pointers that never change.
#include "session.h"
#include <cmath>
#include <cstring>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

namespace
{
// module names of the tensors, in tllm_session::LoraModule order, with their site and segment
struct ModuleInfo
{
    const char* name;
    int site, seg;
};
const ModuleInfo kModules[tllm_session::LM_COUNT] = {{"attention.q", tllm_session::LS_QKV, 0}, {"attention.k", tllm_session::LS_QKV, 1},
    {"attention.v", tllm_session::LS_QKV, 2}, {"attention.dense", tllm_session::LS_DENSE, 0}, {"mlp.fc", tllm_session::LS_GATE_UP, 0},
    {"mlp.gate", tllm_session::LS_GATE_UP, 1}, {"mlp.proj", tllm_session::LS_PROJ, 0}};
const char* kModuleKeys[tllm_session::LM_COUNT] = {"q", "k", "v", "o", "gate", "up", "down"};

bool lora_ready(tllm_session_t s, const char* who, int32_t slot)
{
    if (!s)
    {
        set_error("%s: null session", who);
        return false;
    }
    if (s->lora_rank <= 0)
    {
        set_error("%s: the session was created without lora_max_rank", who);
        return false;
    }
    if (slot < 0 || slot >= s->lora_adapters)
    {
        set_error("%s: slot %d outside [0, lora_max_adapters = %d)", who, slot, s->lora_adapters);
        return false;
    }
    return true;
}
} // namespace

void tllm_session::lora_site_shape(int site, int* K, int* nseg, int* seg_n) const
{
    seg_n[0] = seg_n[1] = seg_n[2] = 0;
    switch (site)
    {
    case LS_QKV:
        *K = hidden;
        *nseg = 3;
        seg_n[0] = Hr * Dh;
        seg_n[1] = seg_n[2] = Hkvr * Dh;
        break;
    case LS_DENSE:
        *K = Dr;
        *nseg = 1;
        seg_n[0] = hidden;
        break;
    case LS_GATE_UP:
        *K = hidden;
        *nseg = 2;
        seg_n[0] = seg_n[1] = Ir;
        break;
    default:
        *K = Ir;
        *nseg = 1;
        seg_n[0] = hidden;
        break;
    }
}

int tllm_session::lora_alloc()
{
    if (!lora_sites.empty() || lora_rank <= 0)
        return 0;
    std::vector<LoraSiteBuf> sites((size_t) num_layers * LS_COUNT);
    auto take = [&](void** p, size_t bytes) {
        HIP_OK(hipMalloc(p, bytes));
        lora_allocs.push_back(*p);
        HIP_OK(hipMemset(*p, 0, bytes));
        return 0;
    };
    for (int li = 0; li < num_layers; ++li)
        for (int site = 0; site < LS_COUNT; ++site)
        {
            LoraSiteBuf& sb = sites[(size_t) li * LS_COUNT + site];
            memset(&sb, 0, sizeof(sb));
            if (!lora_site_on(site))
                continue;
            int K = 0, nseg = 0, seg_n[3];
            lora_site_shape(site, &K, &nseg, seg_n);
            const size_t ntot = (size_t) seg_n[0] + seg_n[1] + seg_n[2];
            std::vector<LoraAdapterRec> recs(lora_adapters);
            for (int slot = 0; slot < lora_adapters; ++slot)
            {
                RUN(take(&sb.a[slot], (size_t) nseg * lora_rank * K * 2));
                RUN(take(&sb.b[slot], ntot * lora_rank * 2));
                recs[slot].a = sb.a[slot];
                recs[slot].b = sb.b[slot];
            }
            void* t = nullptr;
            RUN(take(&t, recs.size() * sizeof(LoraAdapterRec)));
            sb.table = static_cast<LoraAdapterRec*>(t);
            HIP_OK(hipMemcpy(t, recs.data(), recs.size() * sizeof(LoraAdapterRec), hipMemcpyHostToDevice));
        }
    lora_sites.swap(sites);
    return 0;
}

int tllm_session::lora_map_rows(int M, int rows_per_seq, hipStream_t st)
{
    if (lora_rank <= 0)
        return 0;
    return launch_lora_row_adapter(lora_rows, lora_sel, B, M, rows_per_seq, rows_per_seq > 0 ? nullptr : cu_dev, st) ? 1 : 0;
}

int tllm_session::lora_apply(int li, int site, int M, const void* xin, int pro, const void* gamma, const int32_t* rows,
    hipStream_t st)
{
    if (!lora_site_on(site))
        return 0;
    if (lora_sites.empty() || !lora_t || !rows)
    {
        set_error("session: LoRA buffers are not allocated (setup after the lora keys)");
        return 1;
    }
    const LoraSiteBuf& sb = lora_sites[(size_t) li * LS_COUNT + site];
    int K = 0, nseg = 0, seg_n[3];
    lora_site_shape(site, &K, &nseg, seg_n);
    LoraShrinkParams sp;
    sp.M = M;
    sp.K = K;
    sp.R = nseg * lora_rank;
    sp.pro = pro;
    sp.x = xin;
    sp.ldx = K;
    sp.gamma = gamma;
    sp.eps = eps;
    sp.row_adapter = rows;
    sp.table = sb.table;
    sp.num_adapters = lora_adapters;
    sp.t = lora_t;
    LoraExpandParams ep;
    ep.M = M;
    ep.r = lora_rank;
    ep.nseg = nseg;
    for (int g = 0; g < nseg; ++g)
        ep.seg_n[g] = seg_n[g];
    uint16_t* q16 = static_cast<uint16_t*>(qkv);
    switch (site)
    {
    case LS_QKV:
        ep.seg_y[0] = q16;
        ep.seg_y[1] = q16 + seg_n[0];
        ep.seg_y[2] = q16 + seg_n[0] + seg_n[1];
        ep.seg_ldy[0] = ep.seg_ldy[1] = ep.seg_ldy[2] = QKVr;
        break;
    case LS_GATE_UP:
        ep.seg_y[0] = g;
        ep.seg_y[1] = u;
        ep.seg_ldy[0] = ep.seg_ldy[1] = Ir;
        break;
    default: // attention.dense, mlp.proj: the residual stream, behind the projection's residual add
        ep.seg_y[0] = x;
        ep.seg_ldy[0] = hidden;
        break;
    }
    ep.t = lora_t;
    ep.row_adapter = rows;
    ep.table = sb.table;
    ep.num_adapters = lora_adapters;
    RUN(timed(PC_OTHER, st, [&] { return launch_lora_shrink(sp, st) ? 1 : 0; }));
    return timed(PC_OTHER, st, [&] { return launch_lora_expand(ep, st) ? 1 : 0; });
}

extern "C" {

int32_t tllm_session_lora_set_tensor(tllm_session_t s, int32_t slot, const char* name, int32_t dtype, const int64_t* dims,
    int32_t nbDims, const void* data, int32_t location)
{
    if (!lora_ready(s, "tllm_session_lora_set_tensor", slot))
        return 1;
    if (!name || !dims || !data || nbDims != 2 || dtype != TLLM_HALF || dims[0] < 1 || dims[1] < 1)
    {
        set_error("tllm_session_lora_set_tensor: '%s' must be an fp16 matrix", name ? name : "(null)");
        return 1;
    }
    tllm_session::LoraStaged t;
    t.dims.assign(dims, dims + 2);
    t.data.resize((size_t) dims[0] * dims[1]);
    if (location == 0)
        memcpy(t.data.data(), data, t.data.size() * 2);
    else
        HIP_OK(hipMemcpy(t.data.data(), data, t.data.size() * 2, hipMemcpyDeviceToHost));
    s->lora_staged[slot][name] = std::move(t);
    return 0;
}

int32_t tllm_session_lora_commit(tllm_session_t s, int32_t slot, float alpha, int32_t flags)
{
    if (!lora_ready(s, "tllm_session_lora_commit", slot))
        return 1;
    // whatever happens, the staged tensors do not outlive this call
    std::map<std::string, tllm_session::LoraStaged> staged;
    staged.swap(s->lora_staged[slot]);
    const int Rk = s->lora_rank;
    // every staged name is a module of a layer, of the key's list, with both halves of one rank r <= lora_max_rank
    int r = 0;
    size_t used = 0;
    for (int li = 0; li < s->num_layers; ++li)
        for (int m = 0; m < tllm_session::LM_COUNT; ++m)
        {
            const std::string base = "layers." + std::to_string(li) + "." + kModules[m].name;
            auto ia = staged.find(base + ".lora_a"), ib = staged.find(base + ".lora_b");
            if (ia == staged.end() && ib == staged.end())
                continue;
            if (!s->lora_mod[m])
            {
                set_error("tllm_session_lora_commit: module '%s' (%s) is not in lora_target_modules", base.c_str(), kModuleKeys[m]);
                return 1;
            }
            if (ia == staged.end() || ib == staged.end())
            {
                set_error("tllm_session_lora_commit: '%s' has only one of lora_a / lora_b", base.c_str());
                return 1;
            }
            int K = 0, nseg = 0, seg_n[3];
            s->lora_site_shape(kModules[m].site, &K, &nseg, seg_n);
            const int64_t ra = ia->second.dims[0], N = seg_n[kModules[m].seg];
            if (ra > Rk)
            {
                set_error("tllm_session_lora_commit: '%s.lora_a' has rank %lld above lora_max_rank %d", base.c_str(), (long long) ra, Rk);
                return 1;
            }
            if (ia->second.dims[1] != K || ib->second.dims[0] != N || ib->second.dims[1] != ra)
            {
                set_error("tllm_session_lora_commit: '%s' has lora_a [%lld, %lld] / lora_b [%lld, %lld], expected [r, %d] / [%lld, r]",
                    base.c_str(), (long long) ia->second.dims[0], (long long) ia->second.dims[1], (long long) ib->second.dims[0],
                    (long long) ib->second.dims[1], K, (long long) N);
                return 1;
            }
            if (r && ra != r)
            {
                set_error("tllm_session_lora_commit: '%s' has rank %lld, other modules of the adapter rank %d", base.c_str(),
                    (long long) ra, r);
                return 1;
            }
            r = (int) ra;
            used += 2;
        }
    if (used != staged.size())
    {
        for (auto& kv : staged)
        {
            bool known = false;
            for (int li = 0; li < s->num_layers && !known; ++li)
                for (int m = 0; m < tllm_session::LM_COUNT && !known; ++m)
                {
                    const std::string base = "layers." + std::to_string(li) + "." + kModules[m].name;
                    known = kv.first == base + ".lora_a" || kv.first == base + ".lora_b";
                }
            if (!known)
            {
                set_error("tllm_session_lora_commit: '%s' names no LoRA module of this model", kv.first.c_str());
                return 1;
            }
        }
    }
    if (r == 0)
    {
        set_error("tllm_session_lora_commit: slot %d has no tensors", slot);
        return 1;
    }
    RUN(s->lora_alloc());
    HIP_OK(hipDeviceSynchronize()); // a step or prefill in flight on any stream finishes under the slot's old contents
    const float scale = (flags & 1) ? alpha / sqrtf((float) r) : alpha / (float) r;
    std::vector<uint16_t> ha, hb;
    for (int li = 0; li < s->num_layers; ++li)
        for (int site = 0; site < tllm_session::LS_COUNT; ++site)
        {
            if (!s->lora_site_on(site))
                continue;
            const tllm_session::LoraSiteBuf& sb = s->lora_sites[(size_t) li * tllm_session::LS_COUNT + site];
            int K = 0, nseg = 0, seg_n[3];
            s->lora_site_shape(site, &K, &nseg, seg_n);
            const size_t ntot = (size_t) seg_n[0] + seg_n[1] + seg_n[2];
            ha.assign((size_t) nseg * Rk * K, 0);
            hb.assign(ntot * Rk, 0);
            for (int m = 0; m < tllm_session::LM_COUNT; ++m)
            {
                if (kModules[m].site != site)
                    continue;
                const std::string base = "layers." + std::to_string(li) + "." + kModules[m].name;
                auto ia = staged.find(base + ".lora_a");
                if (ia == staged.end())
                    continue;
                const tllm_session::LoraStaged& ta = ia->second;
                const tllm_session::LoraStaged& tb = staged.find(base + ".lora_b")->second;
                const int g = kModules[m].seg;
                size_t n_off = 0;
                for (int i = 0; i < g; ++i)
                    n_off += seg_n[i];
                for (int j = 0; j < r; ++j)
                    memcpy(&ha[((size_t) g * Rk + j) * K], &ta.data[(size_t) j * K], (size_t) K * 2);
                for (int n = 0; n < seg_n[g]; ++n)
                    memcpy(&hb[(n_off + n) * Rk], &tb.data[(size_t) n * r], (size_t) r * 2);
            }
            HIP_OK(hipMemcpy(sb.a[slot], ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(sb.b[slot], hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
            LoraAdapterRec rec;
            rec.a = sb.a[slot];
            rec.b = sb.b[slot];
            rec.scale = scale;
            HIP_OK(hipMemcpy(sb.table + slot, &rec, sizeof(rec), hipMemcpyHostToDevice));
        }
    s->lora_committed[slot] = true;
    return 0;
}

int32_t tllm_session_lora_clear(tllm_session_t s, int32_t slot)
{
    if (!lora_ready(s, "tllm_session_lora_clear", slot))
        return 1;
    s->lora_staged[slot].clear();
    s->lora_committed[slot] = false;
    bool changed = false;
    for (auto& v : s->lora_sel_host)
        if (v == slot)
        {
            v = -1;
            changed = true;
        }
    if (changed && s->lora_sel)
    {
        HIP_OK(hipDeviceSynchronize()); // as tllm_session_lora_select
        HIP_OK(hipMemcpy(s->lora_sel, s->lora_sel_host.data(), s->lora_sel_host.size() * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

int32_t tllm_session_lora_select(tllm_session_t s, const int32_t* slots)
{
    if (!s || s->lora_rank <= 0)
    {
        set_error("tllm_session_lora_select: the session was created without lora_max_rank");
        return 1;
    }
    if (!s->B || !s->lora_sel || !slots)
    {
        set_error("tllm_session_lora_select: call tllm_session_setup first (and pass one slot per sequence)");
        return 1;
    }
    for (int b = 0; b < s->B; ++b)
    {
        if (slots[b] == -1)
            continue;
        if (slots[b] < 0 || slots[b] >= s->lora_adapters || !s->lora_committed[slots[b]])
        {
            set_error("tllm_session_lora_select: slots[%d] = %d is not a committed slot of [0, lora_max_adapters = %d)", b, slots[b],
                s->lora_adapters);
            return 1;
        }
    }
    s->lora_sel_host.assign(slots, slots + s->B);
    // no stream argument: the copy below is ordered by the null stream only against blocking streams, and a caller's stream need
    // not be one - wait for everything in flight, so that no step runs half under the old selection and half under the new
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(s->lora_sel, s->lora_sel_host.data(), (size_t) s->B * 4, hipMemcpyHostToDevice));
    return 0;
}

} // extern "C"
