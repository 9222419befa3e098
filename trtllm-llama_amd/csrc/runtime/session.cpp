// The C API of a set-up session (include/tllm_runtime_api.h): prompt upload and the context call, the generation step and
// its captured graph, the generate loop, sampling configuration, the getters, and the instrumentation (taps, kernel timing,
// launch-class profile).  Creation and weights: session_weights.cpp; setup: session_setup.cpp; what a context call and a
// step enqueue: session_context.cpp, session_decode.cpp; the entry points that need no session: kernel_api.cpp.
#include "sampling_config.h"
#include "session.h"
#include <algorithm>

using namespace tllm;
using namespace tllm::kernels;
using namespace tllm::runtime;

tllm_session::~tllm_session()
{
    if (own_stream)
        (void) hipStreamDestroy(own_stream);
    free_runtime();
    for (auto p : lora_allocs)
        (void) hipFree(p);
    for (auto& kv : tensors)
        if (kv.second.owned && kv.second.dev)
            (void) hipFree(kv.second.dev);
}

// ================================================================================================
// C API
// ================================================================================================
extern "C" {

static int upload_prompt(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths, hipStream_t st)
{
    // input_ids / input_lengths describe the Bc prompts; the per-sequence generation state is tiled over the beam
    // (generation.py:898-915 _tile_beam_width) - the prompt itself runs once per batch entry
    const int B = s->B, Bc = s->Bc, W = s->beam, S = s->max_in, Smax = s->Smax;
    std::vector<int32_t> lens_c(input_lengths, input_lengths + Bc), lens(B), seq(B, S), zeros(B, 0);
    std::vector<int32_t> mask((size_t) B * Smax, 0), out((size_t) B * Smax, 0);
    for (int bb = 0; bb < B; ++bb)
    {
        const int b = bb / W;
        lens[bb] = lens_c[b];
        if (lens[bb] < 1 || lens[bb] > S)
        {
            set_error("session: input_lengths[%d]=%d out of range [1, %d]", b, lens[bb], S);
            return 1;
        }
        // masked_tokens[b, len_b:max_in] = 1 (generation.py:812-821)
        for (int t = lens[bb]; t < S; ++t)
            mask[(size_t) bb * Smax + t] = 1;
        for (int t = 0; t < S; ++t)
            out[(size_t) bb * Smax + t] = input_ids[(size_t) b * S + t];
    }
    std::vector<int32_t> packed_ids, cu(Bc + 1, 0), last(Bc, 0);
    if (s->packed)
    {
        // the real tokens back to back; generation keeps the padded cache layout (slots [len, max_in) masked), so only
        // the context phase changes shape (generation.py:556-568 with remove_input_padding)
        for (int b = 0; b < Bc; ++b)
        {
            cu[b + 1] = cu[b] + lens_c[b];
            last[b] = cu[b + 1] - 1;
            packed_ids.insert(packed_ids.end(), input_ids + (size_t) b * S, input_ids + (size_t) b * S + lens_c[b]);
        }
        s->ctx_tokens = cu[Bc];
        HIP_OK(hipMemcpyAsync(s->ids_in, packed_ids.data(), packed_ids.size() * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s->cu_dev, cu.data(), cu.size() * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s->last_rows, last.data(), last.size() * 4, hipMemcpyHostToDevice, st));
    }
    else
        HIP_OK(hipMemcpyAsync(s->ids_in, input_ids, (size_t) Bc * S * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->in_len, lens.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->in_len_ctx, lens_c.data(), Bc * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->last_tok, lens_c.data(), Bc * 4, hipMemcpyHostToDevice, st));
    std::vector<float> cum;
    if (W > 1)
    {
        // only hypothesis 0 of every beam group is live before the first step (generation.py:392-397)
        cum.assign(B, -1e20f);
        for (int b = 0; b < Bc; ++b)
            cum[(size_t) b * W] = 0.f;
        HIP_OK(hipMemcpyAsync(s->cum_log_probs, cum.data(), B * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(s->parent_ids, 0, (size_t) B * Smax * 4, st));
        HIP_OK(hipMemsetAsync(s->cache_ind, 0, (size_t) B * Smax * 4, st)); // every slot -> hypothesis 0's rows
    }
    HIP_OK(hipMemcpyAsync(s->seq_len, seq.data(), B * 4, hipMemcpyHostToDevice, st));
    if (s->attn_plan.in_launch_merge) // re-arm the in-launch merge (it re-arms itself per launch; this covers a step that never finished)
        HIP_OK(hipMemsetAsync(s->mmha_ws, 0, (size_t) B * s->Hr * 4, st));
    HIP_OK(hipMemcpyAsync(s->finished, zeros.data(), B * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->masked, mask.data(), mask.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->out_ids, out.data(), out.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); // the host vectors above go out of scope
    s->has_context = true;
    return 0;
}

int32_t tllm_session_context(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    tllm_stream_t stream)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_context: call tllm_session_setup first");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    RUN(upload_prompt(s, input_ids, input_lengths, st));
    RUN(s->run_context(st));
    RUN(s->run_sampler(0, st));
    return 0;
}

int32_t tllm_session_score(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths, float* log_probs,
    int32_t* top1_ids, tllm_stream_t stream)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_score: call tllm_session_setup first");
        return 1;
    }
    if (s->beam > 1)
    {
        set_error("tllm_session_score: beam_width 1 only (set up with beam_width %d)", s->beam);
        return 1;
    }
    if (!input_ids || !input_lengths || !log_probs)
    {
        set_error("tllm_session_score: null argument");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    // exactly tllm_session_context's launches, with the scoring between the head and the sampler (which leaves the next step's
    // input row in x): the scoring writes buffers of its own and tmp, which every later launch fills before it reads it
    RUN(upload_prompt(s, input_ids, input_lengths, st));
    RUN(s->run_context(st));
    RUN(s->score_enqueue(input_ids, input_lengths, st));
    RUN(s->run_sampler(0, st));
    HIP_OK(hipStreamSynchronize(st));
    RUN(s->check_comm());
    s->score_collect(log_probs, top1_ids);
    return 0;
}

int32_t tllm_session_step(tllm_session_t s, int32_t n_steps, int32_t use_graph, tllm_stream_t stream)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_step: call tllm_session_setup first");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    // a graph captured while the transport was in another state (enabled / fused seam / a re-created region) holds launches
    // that no longer match what an eager step would issue: capture again
    if (use_graph && (!s->graph || s->graph_stream != st || (s->tp > 1 && s->graph_comm_gen != comm::p2p::generation())))
    {
        s->drop_graph();
        hipGraph_t g = nullptr;
        HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = s->run_decode_step(st);
        const hipError_t ce = hipStreamEndCapture(st, &g);
        if (rc || ce != hipSuccess || !g)
        {
            if (!rc)
                set_error("session: hipStreamEndCapture failed: %s", hipGetErrorString(ce));
            return 1;
        }
        const hipError_t ie = hipGraphInstantiate(&s->graph, g, nullptr, nullptr, 0);
        (void) hipGraphDestroy(g);
        if (ie != hipSuccess)
        {
            set_error("session: hipGraphInstantiate failed: %s", hipGetErrorString(ie));
            s->graph = nullptr;
            return 1;
        }
        s->graph_stream = st;
        s->graph_comm_gen = comm::p2p::generation();
        ++s->graph_captures;
    }
    for (int i = 0; i < n_steps; ++i)
    {
        if (use_graph)
            HIP_OK(hipGraphLaunch(s->graph, st));
        else
            RUN(s->run_decode_step(st));
    }
    return 0;
}

int32_t tllm_session_fake_context(tllm_session_t s, int32_t length, uint32_t seed, tllm_stream_t stream)
{
    if (!s || !s->B || length < 1 || length > s->max_in)
    {
        set_error("tllm_session_fake_context: bad length");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    const int B = s->B, S = s->max_in;
    std::vector<int32_t> ids((size_t) s->Bc * S, 3), lens(s->Bc, length);
    // a padded prompt of `length` real tokens: slots [length, max_in) are masked
    RUN(upload_prompt(s, ids.data(), lens.data(), st));
    for (int i = 0; i < s->num_layers; ++i)
        RUN(launch_fill_random(s->layers[i].kv, s->kv_dtype, s->kv_elems, seed + 7919u * i, 1.0f, st));
    RUN(s->run_sampler(0, st)); // prepares the RoPE row of the first generation step (the ids are overwritten next)
    RUN(launch_fill_i32(s->cur_ids, 3, B, st));
    RUN(launch_embedding(s->x, s->cur_ids, s->emb, B, s->hidden, s->vocab, st)); // what the sampler would have left in x
    return 0;
}

static int32_t generate_once(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths, int32_t max_new_tokens,
    int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream);
static int32_t generate_steps(tllm_session_t s, int32_t max_new_tokens, int32_t end_id, int* produced_out, tllm_stream_t stream);
static void fill_output_tail(tllm_session_t s, int32_t* output_ids, const std::vector<int>& first, int produced, int32_t end_id,
    int32_t pad_id);

int32_t tllm_session_generate(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream)
{
    // A bounded wait of the one-launch projection + attention expired (its grid was not resident at once - another queue's kernels
    // held CUs): the session has fallen back to the two-launch path, the tokens behind the expired wait are invalid.  Generation
    // is a function of the prompt and the seed alone - greedy trivially; the sampler draws u from a counter-based generator keyed
    // by (seed, row, token number) and sums its weights as integers (kernels/sampling.hip), so it repeats bit for bit - and
    // every cache slot is rewritten before it is read: run the request again.
    const int32_t rc = generate_once(s, input_ids, input_lengths, max_new_tokens, end_id, pad_id, output_ids, stream);
    if (rc != kFusedTimedOut)
        return rc;
    s->fused_retries += 1;
    return generate_once(s, input_ids, input_lengths, max_new_tokens, end_id, pad_id, output_ids, stream) ? 1 : 0;
}

int32_t tllm_session_set_sampling(tllm_session_t s, const tllm_sampling_config_t* cfg)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_set_sampling: call tllm_session_setup first");
        return 1;
    }
    if (cfg)
    {
        if (s->beam > 1)
        {
            set_error("tllm_session_set_sampling: beam_width 1 only (beam search does not sample)");
            return 1;
        }
        RUN(check_sampling_config("tllm_session_set_sampling", *cfg));
        sampling_from_config(s->sampling, *cfg);
    }
    s->sampling_on = cfg != nullptr;
    s->drop_graph(); // the configuration is baked into the captured sampler node, as end_id is
    return 0;
}

int32_t tllm_session_fused_retries(tllm_session_t s)
{
    return s ? s->fused_retries : 0;
}

static int32_t generate_once(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths, int32_t max_new_tokens,
    int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream)
{
    if (!s || !s->B || !input_ids || !input_lengths || !output_ids)
    {
        set_error("tllm_session_generate: bad arguments / setup not called");
        return 1;
    }
    if (max_new_tokens > s->max_new)
    {
        set_error("tllm_session_generate: max_new_tokens %d exceeds setup's %d", max_new_tokens, s->max_new);
        return 1;
    }
    s->end_id = end_id;
    s->drop_graph(); // end_id is baked into the captured sampler node
    RUN(tllm_session_context(s, input_ids, input_lengths, stream));
    int produced = 0;
    RUN(generate_steps(s, max_new_tokens, end_id, &produced, stream));
    if (s->beam > 1)
        return tllm_session_get_beam_output(s, output_ids, nullptr, stream);
    RUN(tllm_session_get_output_ids(s, output_ids, stream));
    fill_output_tail(s, output_ids, std::vector<int>(s->B, s->max_in), produced, end_id, pad_id);
    return 0;
}

// The generation steps behind a sampler launch that has produced the first of max_new_tokens tokens (the prompt pass, or an
// append): *produced = tokens generated per sequence, that first one included.
static int32_t generate_steps(tllm_session_t s, int32_t max_new_tokens, int32_t end_id, int* produced_out, tllm_stream_t stream)
{
    hipStream_t st = s->pick(stream);
    int produced = max_new_tokens > 0 ? 1 : 0; // tokens generated per sequence (the pass before yields the first)
    if (max_new_tokens > 1)
    {
        // first generation step eagerly (also warms lazily-initialised state), the rest from the graph
        RUN(tllm_session_step(s, 1, 0, stream));
        produced = 2;
        if (max_new_tokens > 2)
        {
            const int chunk = 32; // poll the finished flags every `chunk` steps instead of every step
            int done = 2;
            std::vector<int32_t> fin(s->B);
            while (done < max_new_tokens)
            {
                const int n = std::min(chunk, max_new_tokens - done);
                RUN(tllm_session_step(s, n, 1, stream));
                done += n;
                produced = done;
                if (end_id >= 0 && done < max_new_tokens)
                {
                    HIP_OK(hipMemcpyAsync(fin.data(), s->finished, s->B * 4, hipMemcpyDeviceToHost, st));
                    HIP_OK(hipStreamSynchronize(st));
                    RUN(s->check_comm());
                    bool all = true;
                    for (auto f : fin)
                        all = all && f;
                    if (all)
                        break;
                }
            }
        }
    }
    *produced_out = produced;
    return 0;
}

// The reference runs gather_tree for beam_width 1 too (generation.py:990-994; K/decodingKernels.cu:130-156): everything
// after a sequence's first end token, and the tail no step wrote because every sequence had finished, is end_id - not the
// 0 (<unk>) the buffer was initialised with.  Without an end token (benchmarks) the unused tail is pad_id.
// first[b]: the slot of sequence b's first generated token of this request (max_input_len behind a prompt).
static void fill_output_tail(tllm_session_t s, int32_t* output_ids, const std::vector<int>& first, int produced, int32_t end_id,
    int32_t pad_id)
{
    const int32_t fill = end_id >= 0 ? end_id : pad_id;
    for (int b = 0; b < s->B; ++b)
    {
        int32_t* o = output_ids + (size_t) b * s->Smax;
        bool done = false;
        for (int t = first[b]; t < s->Smax; ++t)
        {
            if (done || t >= first[b] + produced)
                o[t] = fill;
            else if (end_id >= 0 && o[t] == end_id)
                done = true;
        }
    }
}

// ------------------------------------------------------------------------------------------ append
// What a session must be for an append pass (tllm_session_append, _verify, _generate_lookup)
static int32_t append_session_ok(tllm_session_t s, const char* who)
{
    if (!s || !s->B)
    {
        set_error("%s: call tllm_session_setup first", who);
        return 1;
    }
    if (s->beam > 1 || (s->paged_kv && !s->paged_append) || s->tp > 1) // (a paged session serves with the key paged_append)
    {
        set_error("%s: not built for beam search, the paged cache or tensor parallelism (beam_width %d, paged %d, tp %d)", who, s->beam,
            s->paged_kv ? 1 : 0, s->tp);
        return 1;
    }
    return 0;
}

// The checks of tllm_session_append; they enqueue nothing but the read of sequence_length.  past[b] = sequence_length[b] before
// the call, *max_past_out their maximum.  lengths (host [B], or null = n for every sequence): sequence b appends lengths[b] of the
// n ids of its row - what stands behind them is not looked at; *max_end_out (may be null) = max_b (past[b] + its tokens).
static int32_t append_checks(tllm_session_t s, const char* who, const int32_t* ids, int32_t n, const int32_t* lengths,
    int32_t reserve_new, std::vector<int32_t>& past, int* max_past_out, int* max_end_out, tllm_stream_t stream)
{
    RUN(append_session_ok(s, who));
    if (!ids)
    {
        set_error("%s: null argument", who);
        return 1;
    }
    if (n < 1 || n > s->max_in)
    {
        set_error("%s: n %d out of range [1, max_input_len %d] (the activation buffers are sized for the prompt)", who, n, s->max_in);
        return 1;
    }
    if (!s->has_context)
    {
        set_error("%s: no context yet - the cache is not live (call tllm_session_context first)", who);
        return 1;
    }
    const int B = s->B, Smax = s->Smax;
    if (lengths)
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 1 || lengths[b] > n)
            {
                set_error("%s: lengths[%d] = %d out of range [1, %d] (a sequence that sits the call out is not built)", who, b,
                    lengths[b], n);
                return 1;
            }
    for (int b = 0; b < B; ++b)
        for (int i = 0, nb = lengths ? lengths[b] : n; i < nb; ++i)
        {
            const int32_t id = ids[(size_t) b * n + i];
            if (id < 0 || id >= s->vocab)
            {
                set_error("%s: token id %d (sequence %d, token %d) outside [0, %d)", who, id, b, i, s->vocab);
                return 1;
            }
        }
    hipStream_t st = s->pick(stream);
    past.assign(B, 0);
    HIP_OK(hipMemcpyAsync(past.data(), s->seq_len, (size_t) B * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    RUN(s->check_comm());
    int max_past = 0, max_end = 0;
    for (int b = 0; b < B; ++b)
    {
        const int nb = lengths ? lengths[b] : n;
        if (past[b] < s->max_in)
        {
            set_error("%s: sequence_length[%d] = %d is below max_input_len %d - no context has run", who, b, past[b], s->max_in);
            return 1;
        }
        if ((int64_t) past[b] + nb + reserve_new > Smax)
        {
            set_error("%s: sequence %d: %d slots in use + %d appended + %d new exceed the cache capacity %d", who, b, past[b], nb,
                reserve_new, Smax);
            return 1;
        }
        max_past = std::max(max_past, past[b]);
        max_end = std::max(max_end, past[b] + nb);
    }
    *max_past_out = max_past;
    if (max_end_out)
        *max_end_out = max_end;
    return 0;
}

// append_checks (nothing is enqueued before every one has passed), then: the ids to the device and into the token record, the
// append pass, the advance launch, the sampler.  With lengths (host [B]; ids [B, n] padded) the pass runs on B * N rows, N their
// maximum: the ids are compacted to [B, N] on the host, the padded positions filled with the row's own last id (a valid row for the
// embedding; nothing that outlives the call depends on those rows), and the lengths go to append_last once - the attention's
// n_per_seq, the head's gather and the advance launch all read them there.
static int32_t append_enqueue(tllm_session_t s, const char* who, const int32_t* ids, int32_t n, const int32_t* lengths,
    int32_t reserve_new, std::vector<int32_t>& past, tllm_stream_t stream)
{
    int max_past = 0, max_end = 0;
    RUN(append_checks(s, who, ids, n, lengths, reserve_new, past, &max_past, &max_end, stream));
    hipStream_t st = s->pick(stream);
    const int B = s->B, Smax = s->Smax;
    if (lengths)
    {
        const int N = *std::max_element(lengths, lengths + B);
        std::vector<int32_t> dense((size_t) B * N);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < N; ++i)
                dense[(size_t) b * N + i] = ids[(size_t) b * n + std::min(i, lengths[b] - 1)];
        HIP_OK(hipMemcpyAsync(s->ids_in, dense.data(), dense.size() * 4, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s->append_last, lengths, (size_t) B * 4, hipMemcpyHostToDevice, st));
        for (int b = 0; b < B; ++b)
            HIP_OK(hipMemcpyAsync(s->out_ids + (size_t) b * Smax + past[b], ids + (size_t) b * n, (size_t) lengths[b] * 4,
                hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st)); // the caller's buffers (and dense) may go out of scope
        RUN(s->run_append_ragged(N, max_end, st));
        RUN(launch_append_advance_ragged(s->seq_len, s->finished, s->append_last, B, N, st) ? 1 : 0);
        RUN(s->run_sampler(0, st));
        return 0;
    }
    HIP_OK(hipMemcpyAsync(s->ids_in, ids, (size_t) B * n * 4, hipMemcpyHostToDevice, st));
    for (int b = 0; b < B; ++b)
        HIP_OK(hipMemcpyAsync(s->out_ids + (size_t) b * Smax + past[b], ids + (size_t) b * n, (size_t) n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); // the caller's buffer may go out of scope
    RUN(s->run_append(n, max_past, st));
    RUN(launch_append_advance(s->seq_len, s->finished, B, n, st) ? 1 : 0);
    RUN(s->run_sampler(0, st));
    return 0;
}

int32_t tllm_session_append(tllm_session_t s, const int32_t* ids, int32_t n, tllm_stream_t stream)
{
    std::vector<int32_t> past;
    return append_enqueue(s, "tllm_session_append", ids, n, nullptr, 0, past, stream) ? 1 : 0;
}

int32_t tllm_session_append_ragged(tllm_session_t s, const int32_t* ids, const int32_t* lengths, int32_t W, tllm_stream_t stream)
{
    const char* who = "tllm_session_append_ragged";
    RUN(append_session_ok(s, who) ? 1 : 0);
    if (!lengths)
    {
        set_error("%s: null argument", who);
        return 1;
    }
    std::vector<int32_t> past;
    return append_enqueue(s, who, ids, W, lengths, 0, past, stream) ? 1 : 0;
}

// tllm_session_append_generate (lengths null) and tllm_session_append_ragged_generate
static int32_t append_generate_entry(tllm_session_t s, const char* who, const int32_t* ids, int32_t n, const int32_t* lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream)
{
    if (!s || !s->B || !output_ids || max_new_tokens < 1)
    {
        set_error("%s: bad arguments (max_new_tokens >= 1, output_ids set) / setup not called", who);
        return 1;
    }
    if (end_id != s->end_id)
    {
        s->end_id = end_id;
        s->drop_graph(); // end_id is baked into the captured sampler node
    }
    std::vector<int32_t> past;
    // the last of the max_new_tokens tokens is chosen by a sampler that writes slot past + n + max_new_tokens - 1
    int rc = append_enqueue(s, who, ids, n, lengths, max_new_tokens, past, stream);
    int produced = 0;
    if (!rc)
        rc = generate_steps(s, max_new_tokens, end_id, &produced, stream);
    if (!rc)
        rc = tllm_session_get_output_ids(s, output_ids, stream);
    if (rc == kFusedTimedOut)
        set_error("%s: a bounded in-launch wait of the generation step expired: the session's tokens and cache behind it are invalid, "
                  "and the append has consumed the state the call started from - run the conversation again from tllm_session_context",
            who);
    if (rc)
        return 1;
    std::vector<int> first(s->B);
    for (int b = 0; b < s->B; ++b)
        first[b] = past[b] + (lengths ? lengths[b] : n);
    fill_output_tail(s, output_ids, first, produced, end_id, pad_id);
    return 0;
}

int32_t tllm_session_append_generate(tllm_session_t s, const int32_t* ids, int32_t n, int32_t max_new_tokens, int32_t end_id,
    int32_t pad_id, int32_t* output_ids, tllm_stream_t stream)
{
    return append_generate_entry(s, "tllm_session_append_generate", ids, n, nullptr, max_new_tokens, end_id, pad_id, output_ids, stream);
}

int32_t tllm_session_append_ragged_generate(tllm_session_t s, const int32_t* ids, const int32_t* lengths, int32_t W,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, int32_t* output_ids, tllm_stream_t stream)
{
    const char* who = "tllm_session_append_ragged_generate";
    if (s && s->B && !lengths)
    {
        set_error("%s: null argument", who);
        return 1;
    }
    return append_generate_entry(s, who, ids, W, lengths, max_new_tokens, end_id, pad_id, output_ids, stream);
}

int32_t tllm_session_append_launches(tllm_session_t s, int64_t* wave, int64_t* mfma)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_append_launches: setup not called");
        return 1;
    }
    if (wave)
        *wave = s->append_wave_launches;
    if (mfma)
        *mfma = s->append_mfma_launches;
    return 0;
}

// ------------------------------------------------------------------------------------------ speculative decoding
// What a session must be for a verify pass.  The greedy entries refuse a sampling configuration that is not plain arg-max (their
// accept rule compares with the arg-max); the *_sampled entries take it.
static int32_t verify_session_ok(tllm_session_t s, const char* who, bool sampled)
{
    RUN(append_session_ok(s, who));
    if (!sampled && s->sampling_on && !sampling_is_greedy(s->sampling))
    {
        set_error("%s: the session samples (top-k / top-p / penalties): the accept rule is greedy - speculative sampling is not built "
                  "into this entry: use %s_sampled", who, who);
        return 1;
    }
    return 0;
}

static int32_t verify_entry(tllm_session_t s, const char* who, bool sampled, const int32_t* ids, int32_t n, int32_t* accepted,
    float* log_probs, tllm_stream_t stream)
{
    RUN(verify_session_ok(s, who, sampled) ? 1 : 0);
    if (!accepted)
    {
        set_error("%s: null argument", who);
        return 1;
    }
    if (n > TLLM_VERIFY_MAX_TOKENS)
    {
        set_error("%s: n %d exceeds TLLM_VERIFY_MAX_TOKENS %d", who, n, TLLM_VERIFY_MAX_TOKENS);
        return 1;
    }
    std::vector<int32_t> past;
    int max_past = 0;
    // (one slot behind the n rows: the accept step writes the new pending token to slot p + m + 1 <= p + n)
    RUN(append_checks(s, who, ids, n, nullptr, 1, past, &max_past, nullptr, stream) ? 1 : 0);
    hipStream_t st = s->pick(stream);
    const int B = s->B;
    HIP_OK(hipMemcpyAsync(s->ids_in, ids, (size_t) B * n * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); // the caller's buffer may go out of scope
    RUN(s->run_verify(n, max_past, nullptr, sampled, st) ? 1 : 0);
    HIP_OK(hipMemcpyAsync(accepted, s->verify.accepted, (size_t) B * 4, hipMemcpyDeviceToHost, st));
    if (log_probs) // row (b, i - 1) scored ids[b][i]; its last row had no target and scored 0
    {
        for (int b = 0; b < B; ++b)
            log_probs[(size_t) b * n] = 0.f;
        if (n > 1)
            HIP_OK(hipMemcpy2DAsync(log_probs + 1, (size_t) n * 4, s->verify.log_probs, (size_t) n * 4, (size_t) (n - 1) * 4, B,
                hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    return s->check_comm() ? 1 : 0;
}

int32_t tllm_session_verify(tllm_session_t s, const int32_t* ids, int32_t n, int32_t* accepted, float* log_probs,
    tllm_stream_t stream)
{
    return verify_entry(s, "tllm_session_verify", false, ids, n, accepted, log_probs, stream);
}

int32_t tllm_session_verify_sampled(tllm_session_t s, const int32_t* ids, int32_t n, int32_t* accepted, float* log_probs,
    tllm_stream_t stream)
{
    return verify_entry(s, "tllm_session_verify_sampled", true, ids, n, accepted, log_probs, stream);
}

int32_t tllm_session_verify_top1(tllm_session_t s, int32_t* top1, int32_t n, tllm_stream_t stream)
{
    if (!s || !s->B || !top1 || !s->verify.top1 || n != s->verify_n)
    {
        set_error("tllm_session_verify_top1: bad arguments, or no verify pass of n = %d ids has run since setup", n);
        return 1;
    }
    hipStream_t st = s->pick(stream);
    HIP_OK(hipMemcpyAsync(top1, s->verify.top1, (size_t) s->B * n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_verify_draws(tllm_session_t s, int32_t* draws, int32_t n, tllm_stream_t stream)
{
    if (!s || !s->B || !draws || !s->verify_cmp || n != s->verify_n)
    {
        set_error("tllm_session_verify_draws: bad arguments, or no verify pass of n = %d ids has run since setup", n);
        return 1;
    }
    hipStream_t st = s->pick(stream);
    HIP_OK(hipMemcpyAsync(draws, s->verify_cmp, (size_t) s->B * n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_verify_logits(tllm_session_t s, float* logits, int32_t n, tllm_stream_t stream)
{
    if (!s || !s->B || !logits || !s->verify.logits || n != s->verify_n)
    {
        set_error("tllm_session_verify_logits: bad arguments, or no verify pass of n = %d ids has run since setup", n);
        return 1;
    }
    hipStream_t st = s->pick(stream);
    // the rows are Vr floats apart on the device, vocab of them are ids
    HIP_OK(hipMemcpy2DAsync(logits, (size_t) s->vocab * 4, s->verify.logits, (size_t) s->Vr * 4, (size_t) s->vocab * 4,
        (size_t) s->B * n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

static int32_t generate_lookup_entry(tllm_session_t s, const char* who, bool sampled, const int32_t* input_ids,
    const int32_t* input_lengths, int32_t max_new_tokens, int32_t end_id, int32_t pad_id, const tllm_lookup_config_t* cfg,
    int32_t* output_ids, tllm_lookup_stats_t* stats, tllm_stream_t stream)
{
    RUN(verify_session_ok(s, who, sampled) ? 1 : 0);
    if (!input_ids || !input_lengths || !output_ids || !cfg)
    {
        set_error("%s: null argument", who);
        return 1;
    }
    const int n = cfg->num_draft_tokens;
    if (n < 2 || n > TLLM_VERIFY_MAX_TOKENS || cfg->max_ngram < 1 || cfg->max_ngram > kLookupMaxNgram)
    {
        set_error("%s: num_draft_tokens %d outside [2, %d] or max_ngram %d outside [1, %d]", who, n, TLLM_VERIFY_MAX_TOKENS,
            cfg->max_ngram, kLookupMaxNgram);
        return 1;
    }
    if (n > s->max_in)
    {
        set_error("%s: num_draft_tokens %d exceeds max_input_len %d (the activation buffers are sized for the prompt)", who, n, s->max_in);
        return 1;
    }
    if (max_new_tokens < 1 || (int64_t) max_new_tokens + n > s->max_new)
    {
        set_error("%s: max_new_tokens %d + num_draft_tokens %d exceed setup's max_new_tokens %d (the last verify pass still writes "
                  "num_draft_tokens cache rows from the current length)", who, max_new_tokens, n, s->max_new);
        return 1;
    }
    hipStream_t st = s->pick(stream);
    const int B = s->B, S = s->max_in;
    if (end_id != s->end_id)
    {
        s->end_id = end_id;
        s->drop_graph(); // end_id is baked into the captured sampler node
    }
    RUN(tllm_session_context(s, input_ids, input_lengths, stream) ? 1 : 0);
    const int lim = S + max_new_tokens - 1; // sequence length with max_new_tokens tokens in the record
    tllm_lookup_stats_t acc = {0, 0, 0, 0, 0};
    std::vector<int32_t> state((size_t) B * 4), before(B, 0);
    bool verify_pending = false, stepped = false;
    RUN(s->verify_buffers() ? 1 : 0); // the lookup's state record and the limits are among them
    RUN(launch_fill_i32(s->verify.limit, lim, B, st) ? 1 : 0);
    for (;;)
    {
        PromptLookupParams lp;
        lp.batch = B;
        lp.n = n;
        lp.max_ngram = cfg->max_ngram;
        lp.out_ids = s->out_ids;
        lp.out_stride = s->Smax;
        lp.seq_len = s->seq_len;
        lp.input_lengths = s->in_len;
        lp.max_input_len = S;
        lp.finished = s->finished;
        lp.limit = s->verify.limit;
        lp.vocab = s->vocab;
        lp.ids = s->ids_in;
        lp.state_out = s->verify.state;
        RUN(launch_prompt_lookup(lp, st) ? 1 : 0);
        HIP_OK(hipMemcpyAsync(state.data(), s->verify.state, state.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st)); // the round's only host synchronisation
        const int crc = s->check_comm();
        if (crc == kFusedTimedOut)
            set_error("%s: a bounded in-launch wait of the generation step expired: the session's tokens and cache behind it are invalid "
                      "- run the request again from tllm_session_context", who);
        if (crc)
            return 1;
        bool all_frozen = true, any_frozen = false, any_draft = false;
        int max_past = 0;
        for (int b = 0; b < B; ++b)
        {
            const int32_t* r = &state[(size_t) b * 4];
            if (verify_pending && before[b] >= 0) // drafts the last verify pass kept: what the length moved by, less the bonus token
                acc.accepted += r[0] - before[b] - 1;
            const bool frozen = r[3] != 0;
            all_frozen = all_frozen && frozen;
            any_frozen = any_frozen || frozen;
            any_draft = any_draft || r[2] > 0;
            before[b] = frozen ? -1 : r[0];
            max_past = std::max(max_past, r[0]);
        }
        if (all_frozen)
            break;
        if (!any_draft && !any_frozen)
        {
            // a plain step: the first of a call eagerly (it also warms lazily-initialised state), the others from the graph
            RUN(tllm_session_step(s, 1, stepped ? 1 : 0, stream) ? 1 : 0);
            stepped = true;
            verify_pending = false;
            acc.step_rounds += 1;
        }
        else
        {
            if (max_past + n + 1 > s->Smax) // (cannot happen behind the room check above: the lengths come from the device)
            {
                set_error("%s: sequence length %d + %d ids do not fit the cache capacity %d", who, max_past, n, s->Smax);
                return 1;
            }
            for (int b = 0; b < B; ++b)
                acc.drafted += state[(size_t) b * 4 + 2];
            RUN(s->run_verify(n, max_past, s->verify.limit, sampled, st) ? 1 : 0);
            verify_pending = true;
            acc.verify_rounds += 1;
        }
        acc.rounds += 1;
    }
    RUN(tllm_session_get_output_ids(s, output_ids, stream) ? 1 : 0);
    // every sequence is finished (the row is end_id behind its first end_id) or holds max_new_tokens tokens
    fill_output_tail(s, output_ids, std::vector<int>(B, S), max_new_tokens, end_id, pad_id);
    if (stats)
        *stats = acc;
    return 0;
}

int32_t tllm_session_generate_lookup(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, const tllm_lookup_config_t* cfg, int32_t* output_ids,
    tllm_lookup_stats_t* stats, tllm_stream_t stream)
{
    return generate_lookup_entry(s, "tllm_session_generate_lookup", false, input_ids, input_lengths, max_new_tokens, end_id, pad_id,
        cfg, output_ids, stats, stream);
}

int32_t tllm_session_generate_lookup_sampled(tllm_session_t s, const int32_t* input_ids, const int32_t* input_lengths,
    int32_t max_new_tokens, int32_t end_id, int32_t pad_id, const tllm_lookup_config_t* cfg, int32_t* output_ids,
    tllm_lookup_stats_t* stats, tllm_stream_t stream)
{
    return generate_lookup_entry(s, "tllm_session_generate_lookup_sampled", true, input_ids, input_lengths, max_new_tokens, end_id,
        pad_id, cfg, output_ids, stats, stream);
}

int32_t tllm_session_get_logits(tllm_session_t s, float* logits, tllm_stream_t stream)
{
    if (!s || !s->B || !logits)
        return 1;
    hipStream_t st = s->pick(stream);
    const int rows = s->logit_rows;
    if (s->tp == 1)
    {
        HIP_OK(hipMemcpyAsync(logits, s->logits_local, (size_t) rows * s->vocab * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return s->check_comm();
    }
    std::vector<float> g((size_t) s->tp * rows * s->Vr);
    HIP_OK(hipMemcpyAsync(g.data(), s->logits, g.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    RUN(s->check_comm());
    for (int b = 0; b < rows; ++b)
        for (int v = 0; v < s->vocab; ++v)
            logits[(size_t) b * s->vocab + v] = g[((size_t) (v / s->Vr) * rows + b) * s->Vr + v % s->Vr];
    return 0;
}

int32_t tllm_session_get_output_ids(tllm_session_t s, int32_t* ids, tllm_stream_t stream)
{
    if (!s || !s->B || !ids)
        return 1;
    hipStream_t st = s->pick(stream);
    HIP_OK(hipMemcpyAsync(ids, s->out_ids, (size_t) s->B * s->Smax * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return s->check_comm();
}

int32_t tllm_session_logit_rows(tllm_session_t s)
{
    return s ? s->logit_rows : 0;
}

int32_t tllm_session_vocab_size(tllm_session_t s)
{
    return s ? s->vocab : 0;
}

// Back-track the beams (K/decodingKernels.cu:30-171 gatherTree, called at PY/runtime/generation.py:990-994): hypothesis j of
// batch entry b ends with the token recorded for it at the last slot; its earlier tokens are those of its ancestors.
int32_t tllm_session_get_beam_output(tllm_session_t s, int32_t* ids, float* cum_log_probs, tllm_stream_t stream)
{
    if (!s || !s->B || !ids)
    {
        set_error("tllm_session_get_beam_output: bad arguments / setup not called");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    const int B = s->B, W = s->beam, Smax = s->Smax, S = s->max_in;
    if (W == 1)
    {
        if (cum_log_probs)
        {
            set_error("tllm_session_get_beam_output: cum_log_probs are only kept with beam_width > 1");
            return 1;
        }
        return tllm_session_get_output_ids(s, ids, stream);
    }
    std::vector<int32_t> step_ids((size_t) B * Smax), parents((size_t) B * Smax), len(B);
    HIP_OK(hipMemcpyAsync(step_ids.data(), s->out_ids, step_ids.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(parents.data(), s->parent_ids, parents.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(len.data(), s->seq_len, B * 4, hipMemcpyDeviceToHost, st));
    if (cum_log_probs)
        HIP_OK(hipMemcpyAsync(cum_log_probs, s->cum_log_probs, B * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    RUN(s->check_comm());
    const int32_t fill = s->end_id >= 0 ? s->end_id : 0;
    for (int bb = 0; bb < B; ++bb)
    {
        const int b0 = bb / W * W;
        int32_t* o = ids + (size_t) bb * Smax;
        const int last = std::min(len[bb], Smax - 1); // slot of the newest token
        for (int t = 0; t < S; ++t)
            o[t] = step_ids[(size_t) bb * Smax + t]; // the (padded) prompt, shared by the beam group
        int j = bb - b0;
        for (int t = last; t >= S; --t)
        {
            o[t] = step_ids[(size_t) (b0 + j) * Smax + t];
            j = parents[(size_t) (b0 + j) * Smax + t];
            if (j < 0 || j >= W)
                j = 0;
        }
        // everything after the first end token, and the unused tail, is the end token (:130-156)
        bool done = false;
        for (int t = S; t < Smax; ++t)
        {
            if (t > last || done)
                o[t] = fill;
            else if (s->end_id >= 0 && o[t] == s->end_id)
                done = true;
        }
    }
    return 0;
}

int32_t tllm_session_get_beam_state(tllm_session_t s, int32_t* parent_ids, int32_t* cache_indirection, int32_t* finished,
    int32_t* sequence_lengths, tllm_stream_t stream)
{
    if (!s || !s->B || s->beam < 2)
    {
        set_error("tllm_session_get_beam_state: no beam search set up");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    const size_t n = (size_t) s->B * s->Smax * 4;
    if (parent_ids)
        HIP_OK(hipMemcpyAsync(parent_ids, s->parent_ids, n, hipMemcpyDeviceToHost, st));
    if (cache_indirection)
        HIP_OK(hipMemcpyAsync(cache_indirection, s->cache_ind, n, hipMemcpyDeviceToHost, st));
    if (finished)
        HIP_OK(hipMemcpyAsync(finished, s->finished, (size_t) s->B * 4, hipMemcpyDeviceToHost, st));
    if (sequence_lengths)
        HIP_OK(hipMemcpyAsync(sequence_lengths, s->seq_len, (size_t) s->B * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_get_step_state(tllm_session_t s, int32_t* sequence_length, int32_t* next_position, int32_t* masked_tokens,
    int32_t* input_lengths, tllm_stream_t stream)
{
    if (!s || !s->B)
    {
        set_error("tllm_session_get_step_state: setup not called");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    if (sequence_length)
        HIP_OK(hipMemcpyAsync(sequence_length, s->seq_len, (size_t) s->B * 4, hipMemcpyDeviceToHost, st));
    if (next_position)
        HIP_OK(hipMemcpyAsync(next_position, s->rope_pos, (size_t) s->B * 4, hipMemcpyDeviceToHost, st));
    if (masked_tokens)
        HIP_OK(hipMemcpyAsync(masked_tokens, s->masked, (size_t) s->B * s->Smax * 4, hipMemcpyDeviceToHost, st));
    if (input_lengths)
        HIP_OK(hipMemcpyAsync(input_lengths, s->in_len, (size_t) s->B * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_get_step_epoch(tllm_session_t s, uint32_t* epoch, tllm_stream_t stream)
{
    if (!s || !s->B || !epoch)
    {
        set_error("tllm_session_get_step_epoch: bad arguments / setup not called");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    HIP_OK(hipMemcpyAsync(epoch, s->step_epoch, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_force_tokens(tllm_session_t s, const int32_t* ids, tllm_stream_t stream)
{
    if (!s || !s->B || !ids)
    {
        set_error("tllm_session_force_tokens: bad arguments / setup not called");
        return 1;
    }
    if (s->beam > 1)
    {
        set_error("tllm_session_force_tokens: greedy sessions only");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    // staged through the (idle between steps) prompt-id buffer; the greedy sampler leaves the next input row in x only when
    // hidden % 8 == 0, otherwise the step gathers it from cur_ids itself
    HIP_OK(hipMemcpyAsync(s->ids_in, ids, (size_t) s->B * 4, hipMemcpyHostToDevice, st));
    const bool gather = s->hidden % 8 == 0;
    if (tllm::kernels::launch_force_token(s->ids_in, s->cur_ids, s->out_ids, s->Smax, s->seq_len, gather ? s->emb : nullptr,
            gather ? s->x : nullptr, s->B, s->hidden, s->vocab, st))
        return 1;
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_get_tap_ex(tllm_session_t s, int32_t layer, int32_t which, void* host, size_t nbytes, tllm_stream_t stream)
{
    if (!s || !s->B || !host || layer < 0 || layer >= s->num_layers || which < 0 || which >= tllm_session::kTaps)
    {
        set_error("tllm_session_get_tap: bad arguments / setup not called");
        return 1;
    }
    if (!s->tap_buf[which])
    {
        set_error("tllm_session_get_tap: the session was not created with debug_taps=1");
        return 1;
    }
    const size_t row = (size_t) s->B * s->tap_width(which) * ((s->sq && which != 4) ? 1 : 2);
    if (nbytes != row)
    {
        set_error("tllm_session_get_tap: buffer of %zu bytes, the tap holds %zu", nbytes, row);
        return 1;
    }
    hipStream_t st = s->pick(stream);
    HIP_OK(hipMemcpyAsync(host, s->tap_ptr(which, layer), row, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int32_t tllm_session_get_tap(tllm_session_t s, int32_t layer, void* host, size_t nbytes, tllm_stream_t stream)
{
    return tllm_session_get_tap_ex(s, layer, 1, host, nbytes, stream);
}

void* tllm_session_fused_timeline_ptr(tllm_session_t s)
{
    return s ? s->fused_timing : nullptr;
}

void* tllm_session_mlp_timeline_ptr(tllm_session_t s)
{
    return s ? s->mlp_timing : nullptr;
}

void* tllm_session_kv_cache_ptr(tllm_session_t s, int32_t layer)
{
    if (!s || layer < 0 || layer >= (int) s->layers.size())
        return nullptr;
    return s->layers[layer].kv;
}

int64_t tllm_session_step_bytes(tllm_session_t s, int32_t context_len)
{
    if (!s)
        return 0;
    // weights once + KV read of `context_len` positions + KV write of one position, per rank
    auto lin = [&](const Linear& L) {
        int64_t b = (int64_t) L.N * L.ldw;
        if (L.wtype == W_INT8_WOQ || L.wtype == W_INT4_WOQ)
            b += (int64_t) L.N * 2;
        else if (L.wtype == W_INT8_SQ && L.per_channel)
            b += (int64_t) L.N * 4;
        return b;
    };
    int64_t bytes = lin(s->head);
    const int64_t kv_row = (int64_t) 2 * s->Hkvr * s->Dh * (int64_t) s->kv_esz();
    for (auto& L : s->layers)
        bytes += lin(L.qkv) + lin(L.dense) + lin(L.fc) + lin(L.gate) + lin(L.proj) + kv_row * s->B * (context_len + 1);
    return bytes;
}

int32_t tllm_session_time_kernel(tllm_session_t s, int32_t which, int32_t sweeps, float* avg_us, int64_t* launches,
    tllm_stream_t stream)
{
    if (!s || !s->B || sweeps < 1 || !avg_us || !launches
        || !(which == 1 || which == 2 || which == 4 || which == 5 || which == 6 || which == 7 || which == 8))
    {
        set_error("tllm_session_time_kernel: bad arguments (which in {1,2,4,5,6,7,8}) / setup not called");
        return 1;
    }
    if (which == 8 && !s->mlp_fused_dec)
    {
        set_error("tllm_session_time_kernel: kernel 8 is the one-launch MLP, which this session does not run");
        return 1;
    }
    if (which == 7 && !s->qkv_attn_fused)
    {
        set_error("tllm_session_time_kernel: kernel 7 is the one-launch projection + attention, which this session does not run");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    hipEvent_t a, b;
    (void) hipEventCreate(&a);
    (void) hipEventCreate(&b);
    // (id 7 with the O-projection stage adds O(ctx) to x on every launch: the residual row is put back afterwards)
    std::vector<char> x_keep;
    if (which == 7 || which == 8)
    {
        x_keep.resize((size_t) s->B * s->hidden * 2);
        HIP_OK(hipMemcpyAsync(x_keep.data(), s->x, x_keep.size(), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    s->only_kernel = which;
    int rc = s->run_decode_step(st); // untimed sweep
    (void) hipEventRecord(a, st);
    for (int i = 0; i < sweeps && !rc; ++i)
        rc = s->run_decode_step(st);
    (void) hipEventRecord(b, st);
    s->only_kernel = -1;
    (void) hipStreamSynchronize(st);
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, a, b) != hipSuccess)
    {
        set_error("tllm_session_time_kernel: event timing failed");
        rc = 1;
    }
    (void) hipEventDestroy(a);
    (void) hipEventDestroy(b);
    if (!x_keep.empty())
    {
        HIP_OK(hipMemcpyAsync(s->x, x_keep.data(), x_keep.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    *launches = (int64_t) sweeps * s->num_layers;
    *avg_us = ms * 1000.f / (float) *launches;
    return rc;
}

int64_t tllm_session_greedy_partials_used(tllm_session_t s)
{
    return s ? s->greedy_partials_used : -1;
}

int64_t tllm_session_graph_captures(tllm_session_t s)
{
    return s ? s->graph_captures : -1;
}

int32_t tllm_session_decode_form(tllm_session_t s)
{
    if (!s || !s->B)
        return -1;
    return (s->qkv_attn_fused ? 1 : 0) | (s->qkv_attn_fused && s->o_fused ? 2 : 0) | (s->mlp_fused_dec ? 4 : 0);
}

int32_t tllm_session_profile(tllm_session_t s, int32_t n_steps, float* ms_per_class, int64_t* launches_per_class,
    tllm_stream_t stream)
{
    if (!s || !s->B || n_steps < 1 || !ms_per_class || !launches_per_class)
    {
        set_error("tllm_session_profile: bad arguments / setup not called");
        return 1;
    }
    hipStream_t st = s->pick(stream);
    s->profiling = true;
    s->prof.clear();
    int rc = 0;
    for (int i = 0; i < n_steps && !rc; ++i)
        rc = s->run_decode_step(st);
    s->profiling = false;
    (void) hipStreamSynchronize(st);
    for (int c = 0; c < tllm_session::PC_COUNT; ++c)
    {
        ms_per_class[c] = 0.f;
        launches_per_class[c] = 0;
    }
    for (auto& r : s->prof)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess)
        {
            ms_per_class[r.cls] += ms;
            launches_per_class[r.cls] += 1;
        }
        (void) hipEventDestroy(r.a);
        (void) hipEventDestroy(r.b);
    }
    s->prof.clear();
    return rc;
}

void tllm_session_destroy(tllm_session_t s)
{
    delete s;
}

} // extern "C"
