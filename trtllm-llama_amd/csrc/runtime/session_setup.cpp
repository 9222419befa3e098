// tllm_session_setup[_beam]: the buffers of a (batch, beam, lengths) shape, and the decision which form of the decode
// layer runs on them.  check_comm, the only code that withdraws that decision again, sits next to it.
#include "session.h"
#include <algorithm>
#include <string>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

void tllm_session::drop_graph()
{
    if (graph)
    {
        (void) hipGraphExecDestroy(graph);
        graph = nullptr;
    }
}

void tllm_session::free_runtime()
{
    drop_graph();
    for (auto p : allocs)
        (void) hipFree(p);
    allocs.clear();
    score = ScoreBuffers();
    verify = VerifyBuffers();
    verify_n = 0;
    verify_cmp = nullptr;
}

// ------------------------------------------------------------------------------------------ buffers
int tllm_session::alloc_buffers()
{
    const int S = max_in, D = hidden;
    const size_t M = std::max((size_t) Bc * S, (size_t) B); // prompt rows; the generation phase needs B
    const size_t kv_esz = this->kv_esz();
    size_t kv_bytes = (size_t) B * 2 * Hkvr * Smax * Dh * kv_esz;
    const int T = tokens_per_block;
    max_blocks = paged_kv ? (Smax + T - 1) / T : 0;
    const size_t nblocks = (size_t) B * max_blocks, blk_bytes = (size_t) Hkvr * T * Dh * kv_esz;
    if (paged_kv)
        kv_bytes = 2 * nblocks * blk_bytes;
    kv_elems = kv_bytes / kv_esz;
    for (auto& L : layers)
    {
        RUN(dalloc(&L.kv, kv_bytes));
        HIP_OK(hipMemset(L.kv, 0, kv_bytes));
        L.kv_table = nullptr;
        if (paged_kv)
        {
            // pool [2, blocks, Hr, T, Dh] (K half then V half, like the reference's BlocksManager:
            // kv_cache_manager.py:84-96); logical block j of sequence bb is pool block j * B + bb, so consecutive time
            // blocks of one sequence are NOT contiguous
            std::vector<int64_t> table((size_t) B * 2 * max_blocks);
            const int64_t base = reinterpret_cast<int64_t>(L.kv);
            for (int bb = 0; bb < B; ++bb)
                for (int j = 0; j < max_blocks; ++j)
                {
                    const int64_t blk = (int64_t) j * B + bb;
                    table[((size_t) bb * 2 + 0) * max_blocks + j] = base + blk * (int64_t) blk_bytes;
                    table[((size_t) bb * 2 + 1) * max_blocks + j] = base + ((int64_t) nblocks + blk) * (int64_t) blk_bytes;
                }
            int64_t* dev = nullptr;
            RUN(dalloc(&dev, table.size() * 8));
            HIP_OK(hipMemcpy(dev, table.data(), table.size() * 8, hipMemcpyHostToDevice));
            L.kv_table = dev;
        }
    }
    RUN(dalloc(&x, M * D * 2));
    RUN(dalloc(&tmp, M * D * 2));
    RUN(dalloc(&qkv, M * QKVr * 2));
    RUN(dalloc(&ctx, M * Dr * 2));
    RUN(dalloc(&g, M * Ir * 2));
    RUN(dalloc(&u, M * Ir * 2));
    RUN(dalloc(&inter_buf, M * Ir * 2));
    RUN(dalloc(&q8, M * (size_t) std::max(D, Ir)));
    RUN(dalloc(&qscale, M * 4));
    RUN(dalloc(&logits_local, (size_t) B * Vr * 4));
    RUN(dalloc(&logits, (size_t) B * Vr * tp * 4));
    RUN(dalloc(&last_hidden, (size_t) B * D * 2));
    RUN(dalloc(&ctx_ws, context_attention_workspace_size(Bc, Hr, Dh, S) + 256));
    if ((size_t) Bc * S >= 32)
        RUN(profile_prefill_gemms(Bc * S));
    RUN(dalloc(&ar_partial, (size_t) B * D * 2));
    RUN(dalloc(&ar_norm, (size_t) B * D * 2));
    RUN(dalloc(&ar_scale, (size_t) B * 4));
    for (int w = 0; w < tllm_session::kTaps; ++w)
    {
        tap_buf[w] = nullptr;
        if (debug_taps)
        {
            const size_t nb = (size_t) num_layers * B * tap_width(w) * 2;
            RUN(dalloc(&tap_buf[w], nb));
            HIP_OK(hipMemset(tap_buf[w], 0, nb));
        }
    }
    RUN(dalloc(&cu_dev, (size_t) (Bc + 1) * 4));
    RUN(dalloc(&last_rows, (size_t) Bc * 4));
    const size_t mmha_bytes = mmha_plan(Dh, Smax, B, Hr).workspace_bytes + 256;
    RUN(dalloc(&mmha_ws, mmha_bytes));
    HIP_OK(hipMemset(mmha_ws, 0, mmha_bytes)); // (the merge tickets at its head among them)
    RUN(dalloc(&ids_in, M * 4));
    RUN(dalloc(&cur_ids, (size_t) B * 4));
    RUN(dalloc(&out_ids, (size_t) B * Smax * 4));
    RUN(dalloc(&seq_len, (size_t) B * 4));
    RUN(dalloc(&in_len, (size_t) B * 4));
    RUN(dalloc(&last_tok, (size_t) Bc * 4));
    RUN(dalloc(&in_len_ctx, (size_t) Bc * 4));
    RUN(dalloc(&append_last, (size_t) B * 4));
    append_wave_launches = append_mfma_launches = 0;
    has_context = false;
    cum_log_probs = nullptr;
    parent_ids = cache_ind = nullptr;
    if (beam > 1)
    {
        RUN(dalloc(&cum_log_probs, (size_t) B * 4));
        RUN(dalloc(&parent_ids, (size_t) B * Smax * 4));
        RUN(dalloc(&cache_ind, (size_t) B * Smax * 4));
    }
    RUN(dalloc(&finished, (size_t) B * 4));
    RUN(dalloc(&masked, (size_t) B * Smax * 4));
    rope = plugins::rope_table(Dh, Smax > max_pos ? Smax : max_pos, &rope_len);
    if (!rope)
        return 1;
    RUN(dalloc(&rope_row, (size_t) B * Dh * sizeof(float)));
    HIP_OK(hipMemset(rope_row, 0, (size_t) B * Dh * sizeof(float)));
    RUN(dalloc(&rope_pos, (size_t) B * 4));
    HIP_OK(hipMemset(rope_pos, 0, (size_t) B * 4));
    RUN(dalloc(&step_epoch, 64));
    HIP_OK(hipMemset(step_epoch, 0, 64));
    fused_err = step_epoch + 8;
    lora_sel = lora_rows = nullptr;
    lora_t = nullptr;
    lora_sel_host.assign(B, -1);
    if (lora_rank > 0)
    {
        // the selection (all -1 after a setup), the row map of a prefill pass, the shrink's result; the adapters themselves are
        // not the setup's: they keep their addresses and contents across setups
        RUN(lora_alloc());
        RUN(dalloc(&lora_sel, (size_t) B * 4));
        HIP_OK(hipMemcpy(lora_sel, lora_sel_host.data(), (size_t) B * 4, hipMemcpyHostToDevice));
        RUN(dalloc(&lora_rows, M * 4));
        HIP_OK(hipMemset(lora_rows, 0xff, M * 4));
        RUN(dalloc(&lora_t, M * kLoraMaxSegments * lora_rank * 4));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ decode form
// Which launches a generation step of this session consists of.  Decides, allocates nothing:
//   attn_plan        the split-KV plan of the attention (kernels.h, mmha_plan)
//   qkv_attn_fused   QKV projection + RoPE + cache append + attention in one launch (kernels/qkv_attn_fused.hip)
//   o_fused          ... with the O-projection + residual as its third stage
//   mlp_fused_dec    gate|up + down in one launch (kernels/mlp_fused.hip)
int tllm_session::decide_decode_form()
{
    const int D = hidden;
    attn_plan = mmha_plan(Dh, Smax, B, Hr);
    if (attn_plan.rows_per_group == 0)
    {
        set_error("session: unsupported head size %d", Dh);
        return 1;
    }

    qkv_attn_fused = false;
    o_fused = false;
    mlp_fused_dec = false;
    if (layers.empty())
        return 0;
    // LoRA: the adapters' launches sit behind the QKV, O and down GEMVs (stage_qkv, stage_o_proj, stage_down), so the step runs
    // the separate launches - neither the one-launch front nor the one-launch MLP
    if (lora_rank > 0)
        return 0;
    // the one-launch MLP: batch 1, tp 1, static SmoothQuant, only when asked for
    if (fuse_mlp_cfg > 0 && B == 1 && beam == 1 && tp == 1 && sq && !per_token && mlp_fused_serves(D, Ir, D))
    {
        bool ok = true;
        for (auto& L : layers)
            ok = ok && L.fc.wtype == W_INT8_SQ && L.gate.wtype == W_INT8_SQ && L.proj.wtype == W_INT8_SQ && L.fc.K == D && L.gate.K == D
                && L.fc.N == Ir && L.gate.N == Ir && L.fc.ldw == L.gate.ldw && L.fc.per_channel == L.gate.per_channel
                && L.proj.N == D && L.proj.K == Ir && L.fc.scale_col && L.gate.scale_col && L.proj.scale_col && L.fc.act_scale
                && L.proj.act_scale && L.ln2 && L.ln2_scale && L.mlp_qscale && L.fc.ldw % 16 == 0 && L.proj.ldw % 16 == 0;
        mlp_fused_dec = ok;
    }
    // the one-launch QKV projection + attention: batch 1, greedy, linear cache, the geometry the kernel is built for (K = 4096,
    // head size 128, heads x 8 workgroups = one per CU), NeoX rotary over the whole head.  Weights: SmoothQuant, or - r05 -
    // weight-only int8 (the same 4 KB weight rows against the normalised fp16 row), or - r06 - fp16 (rows of 8 KB, two tiles
    // per row pair; BASELINE.json configs[1]), or weight-only int4.  Every projection of a session has the session's weight type
    // (resolve_linear), so that type is the kind of all layers.
    const bool w16 = wtype == W_FP16, woq4 = wtype == W_INT4_WOQ;
    // An fp8 cache (the one-launch form has no E4M3 instance yet, DESIGN.md section 4: qkv_attn_fused_serves refuses it) and grouped
    // K/V heads (Hkvr != Hr: the front is built for one K/V head per query head) run the separate launches - QKV GEMV, attention
    // with its in-launch merge, O GEMV
    if (fuse_qkv_cfg == 0 || Hkvr != Hr || !attn_plan.in_launch_merge || B != 1 || beam != 1 || paged_kv || tp != 1 || !neox
        || !qkv_attn_fused_serves(D, Hr, Dh, Smax, kv_dtype, wtype, 0, Hkvr))
        return 0;
    for (auto& L : layers)
        if (!(L.qkv.wtype == wtype && L.qkv.K == D && L.qkv.ldw == (w16 ? 2 * D : (woq4 ? D / 2 : D)) && L.qkv.N == 3 * Dr
                && (L.qkv.scale_col || w16)))
            return 0;
    qkv_attn_fused = true;
    // (tp == 1 here: no all-reduce behind the projection.  Weight-only int8: the context row travels as fp16)
    // (int4: the stage is built and bit-identical but measures at par with the GEMV launch it replaces - 724 vs 721 - 735 tokens/s -
    //  so it is on only when asked for: fuse_o_projection = 1)
    o_fused = fuse_o_cfg != 0 && !w16 && (woq4 ? fuse_o_cfg > 0 : true) && (sq ? !per_token : true);
    for (auto& L : layers)
        o_fused = o_fused && L.dense.N == D && L.dense.scale_col && L.dense.wtype == wtype
            && (sq ? (L.dense.act_scale && L.attn_qscale) : true)
            && qkv_attn_fused_serves_o(Hr, Dh, L.dense.N, L.dense.K, L.dense.ldw, wtype, Hkvr);
    // ... and the instance that will run must be resident as a whole (occupancy query x CUs of this device >= its grid)
    if (!qkv_attn_fused_serves(D, Hr, Dh, Smax, kv_dtype, wtype, o_fused ? 1 : 0, Hkvr))
    {
        o_fused = false;
        qkv_attn_fused = qkv_attn_fused_serves(D, Hr, Dh, Smax, kv_dtype, wtype, 0, Hkvr);
    }
    return 0;
}

// HIP reports no last-level cache size (l2CacheSize is one XCD's L2, or 0), so the Infinity Cache is taken from the architecture:
// 256 MiB on gfx942 / gfx950, none known otherwise - and then nothing is made resident.
static int64_t infinity_cache_bytes()
{
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return 0;
    const std::string arch = prop.gcnArchName;
    return (arch.rfind("gfx950", 0) == 0 || arch.rfind("gfx942", 0) == 0) ? (int64_t) 256 << 20 : 0;
}

// How many rows of the lm_head shard the one-row head launch loads with the allocating policy ("The tail
// of the step").  What is measured (profiles/lm_head_residency.txt, one run per setting): the 7B head launch takes 38.4 - 38.9 us
// from 75 % of the rows up against 40.5 - 41.0 us at 0 %, and its FETCH_SIZE is the whole table at every setting - so the gain
// is kept on its own A/B and NOT explained: Infinity Cache hits are not shown.  The rule below is the one the mechanism would
// want, and for 7B it lands in the measured range (31744 of 32000 rows): the cache of the architecture less 8 MiB for what else
// allocates in a step (audited in DESIGN.md), whole shard if it fits, else as many rows as do; under 64 MiB of such rows the launch
// stays exactly the streaming one.  Both figures are assumptions of that unconfirmed mechanism, not tuned values.
void tllm_session::decide_head_residency()
{
    constexpr int64_t kStepAllocBytes = (int64_t) 8 << 20, kMinResidentBytes = (int64_t) 64 << 20;
    head_resident_rows = 0;
    if (head.wtype != W_FP16 || !head.w || head.ldw <= 0)
        return;
    if (head_resident_cfg >= 0)
    {
        head_resident_rows = (int) ((int64_t) head.N * std::min(head_resident_cfg, 100) / 100);
        return;
    }
    const int64_t budget = infinity_cache_bytes() - kStepAllocBytes;
    const int64_t rows = budget <= 0 ? 0 : std::min<int64_t>(head.N, budget / head.ldw);
    if (rows * head.ldw >= kMinResidentBytes)
        head_resident_rows = (int) rows;
}

int tllm_session::alloc_decode_form_buffers()
{
    argmax_part = nullptr;
    head_partials_live = false;
    greedy_partials_used = 0;
    if (B == 1 && beam == 1 && tp == 1 && greedy_partials_cfg != 0)
    {
        RUN(dalloc(&argmax_part, (size_t) kArgmaxPairs * 8));
        HIP_OK(hipMemset(argmax_part, 0, (size_t) kArgmaxPairs * 8));
    }
    ctx_q8 = nullptr;
    fused_xchg = nullptr;
    fused_timing = nullptr;
    mlp_flags = nullptr;
    mlp_timing = nullptr;
    if (attn_plan.in_launch_merge)
        RUN(dalloc(&ctx_q8, (size_t) B * Dr));
    if (mlp_fused_dec)
    {
        RUN(dalloc(&mlp_flags, mlp_fused_flag_bytes()));
        HIP_OK(hipMemset(mlp_flags, 0, mlp_fused_flag_bytes()));
        if (fused_timeline)
        {
            RUN(dalloc(&mlp_timing, (size_t) 256 * 16 * 8));
            HIP_OK(hipMemset(mlp_timing, 0, (size_t) 256 * 16 * 8));
        }
    }
    if (qkv_attn_fused)
    {
        const size_t xb = qkv_attn_fused_xchg_bytes(Hr);
        RUN(dalloc(&fused_xchg, xb));
        HIP_OK(hipMemset(fused_xchg, 0, xb));
        if (fused_timeline)
        {
            RUN(dalloc(&fused_timing, (size_t) Hr * 8 * 16 * 8));
            HIP_OK(hipMemset(fused_timing, 0, (size_t) Hr * 8 * 16 * 8));
        }
    }
    return 0;
}

// After a stream synchronisation: did a fused decode launch, or a peer-to-peer collective of this tensor-parallel session,
// time out?  (The kernels never hang: a bounded wait that expires raises a device flag and every later launch backs off, p2p_allreduce.hip.)  Then
// the hidden states / logits behind this point are not sums over all ranks: fail the call and take the transport out of
// service, so that later sessions of this process fall back to RCCL.
int tllm_session::check_comm()
{
    if ((qkv_attn_fused || mlp_fused_dec) && fused_err)
    {
        // the fused projection + attention launch waits (bounded) for sibling workgroups of the same launch; an expired wait means
        // the grid was not resident at once - the rows behind it are not attention outputs
        uint32_t e = 0;
        if (hipMemcpy(&e, fused_err, 4, hipMemcpyDeviceToHost) != hipSuccess)
        {
            set_error("session: cannot read the fused-attention error word");
            return 1;
        }
        if (e)
        {
            (void) hipMemset(fused_err, 0, 4);
            qkv_attn_fused = false; // later steps take the two-launch path
            o_fused = false;
            mlp_fused_dec = false;  // ... and the two GEMV launches of the MLP
            drop_graph();
            set_error("session: a fused decode launch (QKV + attention: codes 1 - 8, MLP: 16) timed out waiting for a sibling workgroup "
                      "(code %u); the results of this call are invalid, later steps run the unfused launches", e);
            return kFusedTimedOut;
        }
    }
    // only while the transport is IN SERVICE: once a time-out has taken it out (below), later calls run over RCCL and the
    // words that recorded the failure must not fail them (disable_after_error clears them as well)
    if (tp == 1 && !force_comm)
        return 0;
    // A time-out detected through ANOTHER live session of this process took the transport out of service (and cleared the
    // words) since this session last looked: the launches this call replayed from its captured graph ran against the broken
    // group - they spun to their time-out and left x / ar_norm untouched.  Fail this call too and drop the graph.
    const uint64_t eg = comm::p2p::error_generation();
    if (eg != comm_err_seen)
    {
        comm_err_seen = eg;
        if (graph && graph_comm_gen != comm::p2p::generation())
        {
            drop_graph();
            set_error("session: the peer-to-peer transport timed out (seen by another session of this process) while this "
                      "session's captured step still used it; the results of this call are invalid, later calls use RCCL");
            return 1;
        }
    }
    if (!comm::p2p::enabled())
        return 0;
    uint32_t e = 0;
    if (comm::p2p::error_flag(&e) != 0)
    {
        set_error("session: cannot read the peer-to-peer error flag");
        return 1;
    }
    if (e)
    {
        comm::p2p::disable_after_error();
        comm_err_seen = comm::p2p::error_generation();
        drop_graph(); // the captured step holds the peer-to-peer launches
        set_error("session: a peer-to-peer all-reduce timed out waiting for a rank (%s, epoch %u); the results of this call are "
                  "invalid and the peer-to-peer transport is out of service on every rank of the group (later calls use RCCL)",
            (e & 0x80000000u) ? "reported by a peer" : "on this rank", e & 0x7fffffffu);
        return 1;
    }
    return 0;
}

extern "C" {

int32_t tllm_session_setup(tllm_session_t s, int32_t batch_size, int32_t max_input_len, int32_t max_new_tokens)
{
    return tllm_session_setup_beam(s, batch_size, 1, max_input_len, max_new_tokens);
}

int32_t tllm_session_setup_beam(tllm_session_t s, int32_t batch_size, int32_t beam_width, int32_t max_input_len,
    int32_t max_new_tokens)
{
    if (!s || !s->finalized)
    {
        set_error("tllm_session_setup: session not finalized");
        return 1;
    }
    if (batch_size < 1 || max_input_len < 1 || max_new_tokens < 0 || beam_width < 1 || beam_width > 8)
    {
        set_error("tllm_session_setup: bad sizes (batch %d, beam width %d in [1, 8], input %d, new %d)", batch_size, beam_width,
            max_input_len, max_new_tokens);
        return 1;
    }
    if (beam_width > 1 && (size_t) beam_width * (max_input_len + max_new_tokens) * sizeof(int32_t) > 96 * 1024)
    {
        // the device-side beam step stages the cache-indirection rows it re-parents in LDS (decode_step.hip beam_step_kernel)
        set_error("tllm_session_setup: beam_width %d x max_seq_len %d exceeds the beam step's LDS staging (24576 int32)", beam_width,
            max_input_len + max_new_tokens);
        return 1;
    }
    if (beam_width > 1 && s->lora_rank > 0)
    {
        set_error("tllm_session_setup: lora_max_rank with beam_width %d is not built (beam_width 1 only)", beam_width);
        return 1;
    }
    s->free_runtime();
    s->sampling_on = false; // a sampling configuration is set per setup (tllm_session_set_sampling)
    s->Bc = batch_size;
    s->beam = beam_width;
    s->B = batch_size * beam_width;
    s->max_in = max_input_len;
    s->max_new = max_new_tokens;
    s->Smax = max_input_len + max_new_tokens; // generation.py:450-461
    RUN(s->alloc_buffers());
    RUN(s->decide_decode_form());
    s->decide_head_residency();
    return s->alloc_decode_form_buffers();
}

} // extern "C"
