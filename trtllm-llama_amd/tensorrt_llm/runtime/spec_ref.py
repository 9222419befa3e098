"""Host restatement, in numpy, of the two rules of speculative greedy decoding the device implements (csrc/kernels/kernels.h,
SpecAcceptParams / PromptLookupParams; csrc/kernels/spec_decode.hip; tllm_session_verify, tllm_session_generate_lookup; DESIGN.md
section 7d), the counterpart of sampling_ref.py and scoring_ref.py.

accept: behind a verify pass over the n ids t[0..n-1] of a sequence (t[0] the pending token, t[1..] the drafts), whose logits
rows have the arg-max ids a[0..n-1] (row i = the distribution behind t[0..i]), with p = seq_len and lim = limit or INT32_MAX:
    frozen (finished, or p >= lim): accepted = -1, nothing of the sequence changes;
    else  m = 0; while m + 1 < n and p + m + 1 < lim and a[m] != end_id and t[m + 1] == a[m]: m += 1
          bonus = a[m]; out_ids[p + i] = t[i] (i <= m); out_ids[p + m + 1] = bonus; seq_len = p + m + 1; cur_ids = bonus;
          finished |= bonus == end_id; accepted = m; the next RoPE position is p + m + 1 - (max_input_len - input_lengths).
The tokens are those of plain greedy decoding whatever the drafts were: a draft only survives where it IS the arg-max.

prompt_lookup: drafts from the sequence's own record.  The logical sequence is out_ids[0 .. input_lengths) followed by
out_ids[max_input_len .. seq_len]; its last element is the pending token.  For g = max_ngram down to 1 the last g tokens are the
suffix; the most recent start s with s + g < len whose g tokens equal it wins, at the first (largest) g that has one.  The draft is
the up to n - 1 tokens behind the match that exist; the row is [pending, draft..., pending...].

sample_rows (speculative sampling by exact match; kernels.h SpecSampleParams): the sampler on all n rows of
a verify pass.  Row i of sequence b is drawn as sampling_ref.draw draws generated token number g = p + i + 2 - max_input_len (the
token of slot p + i + 1), with the history prompt + record[max_input_len .. p) + t[0..i].  accept() fed with these draws in the
arg-maxes' place is the accept rule of a sampled pass: a draft survives only where it equals the draw."""
import numpy as np

from . import sampling_ref

INT32_MAX = 0x7FFFFFFF


def accept(seq_len, finished, ids, top1, end_id=-1, limit=None, out_ids=None, cur_ids=None, input_lengths=None, max_input_len=0,
           rope_table_len=None):
    """seq_len, finished int [B]; ids, top1 int [B, n]; limit int [B] or None; out_ids int [B, Smax] / cur_ids int [B] optional
    (copies are updated); input_lengths / max_input_len / rope_table_len for the next RoPE position (clamped to the table as the
    device clamps it).  Returns a dict of new arrays: accepted, seq_len, finished, bonus (-1 where frozen), and where their inputs
    were given out_ids, cur_ids, rope_pos (-1 where frozen: not written)."""
    seq_len, finished = np.array(seq_len, np.int64), np.array(finished, np.int64)
    ids, top1 = np.asarray(ids, np.int64), np.asarray(top1, np.int64)
    B, n = ids.shape
    r = dict(accepted=np.full(B, -1, np.int32), bonus=np.full(B, -1, np.int32))
    out = None if out_ids is None else np.array(out_ids)
    cur = None if cur_ids is None else np.array(cur_ids)
    pos = None if input_lengths is None else np.full(B, -1, np.int32)
    for b in range(B):
        p = int(seq_len[b])
        lim = INT32_MAX if limit is None else int(limit[b])
        if finished[b] != 0 or p >= lim:
            continue
        t, a = ids[b], top1[b]
        m = 0
        while m + 1 < n and p + m + 1 < lim and a[m] != end_id and t[m + 1] == a[m]:
            m += 1
        bonus = int(a[m])
        if out is not None:
            for i in range(m + 1):
                if p + i < out.shape[1]:
                    out[b, p + i] = t[i]
            if p + m + 1 < out.shape[1]:
                out[b, p + m + 1] = bonus
        if cur is not None:
            cur[b] = bonus
        seq_len[b] = p + m + 1
        if end_id >= 0 and bonus == end_id:
            finished[b] = 1
        r['accepted'][b], r['bonus'][b] = m, bonus
        if pos is not None:
            q = p + m + 1 - (int(max_input_len) - int(input_lengths[b]))
            pos[b] = max(0, q if rope_table_len is None else min(q, rope_table_len - 1))
    r.update(seq_len=seq_len.astype(np.int32), finished=finished.astype(np.int32))
    if out is not None:
        r['out_ids'] = out
    if cur is not None:
        r['cur_ids'] = cur
    if pos is not None:
        r['rope_pos'] = pos
    return r


def sample_rows(logits_rows, cfg, b, p, ids_row, record_row, input_length, max_input_len, end_id=-1, finished=0, limit=None):
    """logits_rows f32 [n, vocab]: the verify rows of sequence b; cfg a sampling_ref.Config; p = seq_len[b]; ids_row int [n] = t;
    record_row int [Smax] the sequence's token record (prompt slots [0, max_input_len), committed tokens behind).  Returns the
    sampling_ref.Draw of every row, a list of n; None for every row of a frozen sequence (finished, or p >= limit), where the
    device writes end_id without drawing."""
    logits_rows = np.asarray(logits_rows)
    n = logits_rows.shape[0]
    if finished or (limit is not None and p >= limit):
        return [None] * n
    t = np.asarray(ids_row, np.int64)
    rec = np.array(record_row, np.int64)
    out = []
    for i in range(n):
        g = p + i + 2 - max_input_len
        # t[0..i] in the places of slots p .. p + i: from the ids, not from the record (t[0] stands in the pending token's place)
        hist = np.concatenate([rec[:p], t[:i + 1]])
        out.append(sampling_ref.draw(logits_rows[i], cfg, b, g, end_id, sampling_ref.history_ids(hist, input_length, max_input_len, g)))
    return out


def logical_sequence(row, input_length, max_input_len, seq_len):
    """the tokens of one sequence without the padding slots: the prompt, then the generated tokens up to the pending one"""
    row = np.asarray(row)
    return np.concatenate([row[:input_length], row[max_input_len:seq_len + 1]])


def prompt_lookup(out_ids, input_lengths, max_input_len, seq_len, n, max_ngram, finished=None, limit=None):
    """out_ids int [B, Smax]; input_lengths, seq_len int [B]; n = ids per row (k = n - 1 draft slots).  Returns (ids int32 [B, n],
    draft_len int32 [B])."""
    out_ids = np.asarray(out_ids)
    B, k = out_ids.shape[0], n - 1
    ids, draft_len = np.zeros((B, n), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        p = int(seq_len[b])
        seq = logical_sequence(out_ids[b], int(input_lengths[b]), max_input_len, p)
        ids[b, :] = seq[-1]
        frozen = (finished is not None and finished[b] != 0) or (limit is not None and p >= limit[b])
        if frozen:
            continue
        L = len(seq)
        for g in range(max_ngram, 0, -1):
            best = -1
            for s in range(L - g - 1, -1, -1):  # s + g < L: a start that has a follower, so never the suffix itself
                if np.array_equal(seq[s:s + g], seq[L - g:]):
                    best = s
                    break
            if best >= 0:
                d = seq[best + g:best + g + k]
                draft_len[b] = len(d)
                ids[b, 1:1 + len(d)] = d
                break
    return ids, draft_len


def simulate_lookup_rounds(prompt, continuation, n, max_ngram, max_new, end_id=-1):
    """The loop of tllm_session_generate_lookup on a model whose greedy continuation of `prompt` is known: `prompt` one token list
    (or a list of them: a batch, padded to the longest as the session pads), `continuation` its greedy tokens (>= max_new of them
    per sequence).  A round is one pass: a plain step while every sequence is live and none has a draft, else a verify pass of n
    ids.  Returns dict(rounds, verify_rounds, step_rounds, drafted, accepted, tokens [B, max_new])."""
    batch = len(prompt) > 0 and np.ndim(prompt[0]) > 0
    prompts = [np.asarray(q, np.int64) for q in (prompt if batch else [prompt])]
    conts = [np.asarray(c, np.int64) for c in (continuation if batch else [continuation])]
    B = len(prompts)
    lens = np.array([len(q) for q in prompts], np.int32)
    S = int(lens.max())
    assert max_new >= 1 and all(len(c) >= max_new for c in conts)
    Smax = S + max_new + n
    out = np.zeros((B, Smax), np.int64)
    for b in range(B):
        out[b, :lens[b]] = prompts[b]
        out[b, S] = conts[b][0]  # the prompt pass's token
    seq_len = np.full(B, S, np.int32)
    finished = np.array([1 if end_id >= 0 and c[0] == end_id else 0 for c in conts], np.int32)
    limit = np.full(B, S + max_new - 1, np.int32)
    st = dict(rounds=0, verify_rounds=0, step_rounds=0, drafted=0, accepted=0)

    def model_top1(b, rows):
        # row i is the arg-max behind t[0..i]; it is the known continuation while t[1..i] are right - the only rows accept reads
        g = int(seq_len[b]) - S + 1
        c = conts[b]
        return [c[min(g + i, len(c) - 1)] for i in range(rows)]

    while True:
        frozen = (finished != 0) | (seq_len >= limit)
        if frozen.all():
            break
        ids, dl = prompt_lookup(out, lens, S, seq_len, n, max_ngram, finished, limit)
        if not frozen.any() and not dl.any():
            rows = 1
            ids = ids[:, :1]
            st['step_rounds'] += 1
        else:
            rows = n
            st['verify_rounds'] += 1
            st['drafted'] += int(dl.sum())
        top1 = np.array([model_top1(b, rows) for b in range(B)], np.int64)
        r = accept(seq_len, finished, ids, top1, end_id, limit, out_ids=out)
        if rows > 1:
            st['accepted'] += int(r['accepted'][r['accepted'] > 0].sum())
        seq_len, finished, out = r['seq_len'], r['finished'], r['out_ids']
        st['rounds'] += 1
    st['tokens'] = out[:, S:S + max_new].astype(np.int32)
    return st
