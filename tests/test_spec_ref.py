"""tensorrt_llm/runtime/spec_ref.py, the numpy restatement of the two rules of speculative greedy decoding (accept step, prompt
lookup), held on the CPU on hand-made cases, and the loop built from them pinned on the trained fixture: the GPU tests
(test_gpu_spec_kernels.py, test_gpu_generate_lookup.py) compare the device against these functions."""
import os

import numpy as np

from tensorrt_llm.runtime import spec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 9


def one(seq_len, finished, t, a, end_id=END, limit=None, smax=24):
    out = np.full((1, smax), -7, np.int32)
    r = R.accept([seq_len], [finished], [t], [a], end_id, None if limit is None else [limit], out_ids=out, cur_ids=[-3],
                 input_lengths=[4], max_input_len=6, rope_table_len=64)
    return r, out


def accept_cases():
    """(name, seq_len, finished, t, a, limit) -> (accepted, new seq_len, finished, bonus); shared with the GPU kernel test"""
    return [
        ('all drafts right', 10, 0, [5, 6, 7, 8, 3], [6, 7, 8, 3, 4], None, (4, 15, 0, 4)),
        ('first draft wrong', 10, 0, [5, 6, 7, 8, 3], [1, 7, 8, 3, 4], None, (0, 11, 0, 1)),
        ('mismatch in the middle', 10, 0, [5, 6, 7, 8, 3], [6, 7, 2, 3, 4], None, (2, 13, 0, 2)),
        ('end_id mid-way stops and finishes', 10, 0, [5, 6, END, 8, 3], [6, END, 8, 3, 4], None, (1, 12, 1, END)),
        ('bonus is end_id', 10, 0, [5, 6, 7, 8, 3], [6, 7, END, 3, 4], None, (2, 13, 1, END)),
        ('finished at entry', 10, 1, [5, 6, 7, 8, 3], [6, 7, 8, 3, 4], None, (-1, 10, 1, -1)),
        ('clipped by the limit', 10, 0, [5, 6, 7, 8, 3], [6, 7, 8, 3, 4], 12, (1, 12, 0, 7)),
        ('at the limit', 12, 0, [5, 6, 7, 8, 3], [6, 7, 8, 3, 4], 12, (-1, 12, 0, -1)),
    ]


def test_accept_cases():
    for name, p, fin, t, a, lim, (m, sl, f, bonus) in accept_cases():
        r, before = one(p, fin, t, a, limit=lim)
        assert (r['accepted'][0], r['seq_len'][0], r['finished'][0], r['bonus'][0]) == (m, sl, f, bonus), name
        want = before.copy()
        if m >= 0:
            want[0, p:p + m + 1] = t[:m + 1]
            want[0, p + m + 1] = bonus
            assert r['cur_ids'][0] == bonus and r['rope_pos'][0] == sl - (6 - 4), name
        else:
            assert r['cur_ids'][0] == -3 and r['rope_pos'][0] == -1, name  # nothing of a frozen sequence is written
        np.testing.assert_array_equal(r['out_ids'], want, err_msg=name)  # the slots above the bonus stay untouched


def test_accept_with_one_id_is_a_greedy_step():
    r, _ = one(10, 0, [5], [6])
    assert (r['accepted'][0], r['seq_len'][0], r['bonus'][0], r['out_ids'][0, 10], r['out_ids'][0, 11]) == (0, 11, 6, 5, 6)
    r, _ = one(10, 0, [5], [END])
    assert r['finished'][0] == 1
    # without an end id nothing finishes, whatever the ids
    r, _ = one(10, 0, [5, 6], [6, 7], end_id=-1)
    assert (r['accepted'][0], r['finished'][0]) == (1, 0)


def test_accept_keeps_an_accidentally_right_filler_and_clamps_the_rope_position():
    # the lookup pads a row with the pending token: where the model repeats it, the filler IS the greedy token
    r, _ = one(10, 0, [5, 5, 5], [5, 5, 8])
    assert (r['accepted'][0], r['bonus'][0]) == (2, 8)
    r = R.accept([70], [0], [[5, 6]], [[6, 7]], -1, input_lengths=[6], max_input_len=6, rope_table_len=64)
    assert r['rope_pos'][0] == 63


# ------------------------------------------------------------------------------------------------ prompt lookup
def record(prompt, generated, max_in, smax=40, pad=None):
    """a token record row: the prompt, padding slots (holding `pad` ids), the generated tokens (the last one pending)"""
    row = np.zeros(smax, np.int32)
    row[:len(prompt)] = prompt
    if pad is not None:
        row[len(prompt):max_in] = pad[:max_in - len(prompt)]
    row[max_in:max_in + len(generated)] = generated
    return row, len(prompt), max_in + len(generated) - 1


def lookup_cases():
    """(name, row, input_length, seq_len, {(n, g_max): (draft_len, draft)}); max_input_len 12, Smax 40; shared with the GPU test"""
    c = []
    # the padding holds the decoy: "3 4" followed by 99 - only a search over the physical slots would find it
    row, il, sl = record([1, 2, 5, 6, 7, 8, 9], [3, 4], 12, pad=[3, 4, 99, 99, 99])
    c.append(('decoy in the padding must not match', row, il, sl, {(5, 3): (0, []), (5, 1): (0, [])}))
    # suffix "7 8 9": the 3-gram at 0 (followed by 50) must win over the later 1-gram "9" at 6 (followed by 60)
    row, il, sl = record([7, 8, 9, 50, 51, 52, 9, 60, 61], [20, 7, 8, 9], 12)
    c.append(('the longest g wins', row, il, sl, {(5, 3): (4, [50, 51, 52, 9]), (5, 1): (4, [60, 61, 20, 7]), (2, 3): (1, [50]),
                                                     (8, 3): (7, [50, 51, 52, 9, 60, 61, 20])}))
    # "4 5" occurs twice: followed by 30, and later by 31
    row, il, sl = record([4, 5, 30, 1, 4, 5, 31, 2], [6, 4, 5], 12)
    c.append(('the most recent match wins', row, il, sl, {(5, 3): (4, [31, 2, 6, 4]), (2, 3): (1, [31])}))
    # the match sits two tokens before the end: the followers run out (they include the suffix's own tokens)
    row, il, sl = record([1, 2, 3], [8, 9, 8], 12)
    c.append(('followers run out', row, il, sl, {(5, 3): (2, [9, 8]), (8, 1): (2, [9, 8])}))
    row, il, sl = record([1, 2, 3, 4], [5, 6], 12)
    c.append(('no match', row, il, sl, {(5, 3): (0, []), (8, 1): (0, [])}))
    row, il, sl = record([1], [2], 12)
    c.append(('shorter than the n-gram', row, il, sl, {(5, 3): (0, [])}))
    # the only occurrence of the suffix is the suffix: a start needs a follower (s + g < len)
    row, il, sl = record([1, 2, 3], [4, 5, 6], 12)
    c.append(('a suffix that only matches itself', row, il, sl, {(5, 3): (0, []), (5, 1): (0, [])}))
    # a match that crosses from the prompt into the generated tokens over the padding
    row, il, sl = record([1, 2, 3, 4], [5, 6, 7, 3, 4, 5], 12, pad=[77] * 8)
    c.append(('a match across the padding', row, il, sl, {(5, 3): (4, [6, 7, 3, 4])}))
    return c


def test_prompt_lookup_cases():
    for name, row, il, sl, want in lookup_cases():
        for (n, g), (dl, draft) in want.items():
            ids, got = R.prompt_lookup(row[None], [il], 12, [sl], n, g)
            assert got[0] == dl, (name, n, g, got)
            pending = row[sl]
            np.testing.assert_array_equal(ids[0], [pending] + list(draft) + [pending] * (n - 1 - dl), err_msg=f'{name} {n} {g}')


def test_prompt_lookup_frozen_sequences_get_no_draft():
    _, row, il, sl, _ = lookup_cases()[1]
    for kw in (dict(finished=[1]), dict(limit=[sl]), dict(finished=[0], limit=[sl - 1])):
        ids, dl = R.prompt_lookup(row[None], [il], 12, [sl], 5, 3, **kw)
        assert dl[0] == 0 and (ids[0] == row[sl]).all()
    assert R.prompt_lookup(row[None], [il], 12, [sl], 5, 3, finished=[0], limit=[sl + 1])[1][0] == 4


def test_results_never_depend_on_the_drafts():
    r = np.random.default_rng(4)
    cont = r.integers(0, 4, 64)
    prompt = r.integers(0, 4, 9)
    for n, g in ((2, 1), (5, 3), (8, 8)):
        st = R.simulate_lookup_rounds(prompt, cont, n, g, 40)
        np.testing.assert_array_equal(st['tokens'][0], cont[:40])
        assert st['rounds'] == st['verify_rounds'] + st['step_rounds'] and st['accepted'] <= st['drafted'] + st['verify_rounds'] * n
    st = R.simulate_lookup_rounds(prompt, cont, 5, 3, 40, end_id=int(cont[17]))
    first = int(np.nonzero(cont == cont[17])[0][0])
    np.testing.assert_array_equal(st['tokens'][0, :first + 1], cont[:first + 1])  # it stops at the first end id


# ------------------------------------------------------------------------------------------------ the trained fixture
def fixture(rows):
    e = np.load(os.path.join(ROOT, 'tests', 'golden', 'trained_llama', 'eval.npz'))
    return [e['prompts'][b, :e['lengths'][b]] for b in rows], [e['hf_tokens'][b] for b in rows]


LOOKUP_NEW, LOOKUP_N, LOOKUP_G = 48, 8, 3
# prompts 0 and 1 freeze at different rounds and never step together (prompt 0 has a draft in every one of its rounds, and a plain
# step is taken only while all are live); prompts 1 and 6 do both: step rounds while neither has a draft, verify rounds otherwise
LOOKUP_BATCHES = ((0, 1), (1, 6))


def test_lookup_rounds_on_the_trained_fixture():
    p, c = fixture((0, 1))
    assert [len(q) for q in p] == [110, 64]
    a = R.simulate_lookup_rounds(p[0], c[0], LOOKUP_N, LOOKUP_G, LOOKUP_NEW)
    b = R.simulate_lookup_rounds(p[1], c[1], LOOKUP_N, LOOKUP_G, LOOKUP_NEW)
    np.testing.assert_array_equal(a['tokens'][0], c[0][:LOOKUP_NEW])
    np.testing.assert_array_equal(b['tokens'][0], c[1][:LOOKUP_NEW])
    # prompt 0 repeats itself: far fewer rounds than tokens (the GPU test's rounds * 3 <= 48); prompt 1 rarely does
    assert (a['rounds'], a['verify_rounds'], a['step_rounds'], a['drafted'], a['accepted']) == (6, 6, 0, 42, 41)
    assert (b['rounds'], b['verify_rounds'], b['step_rounds'], b['drafted'], b['accepted']) == (42, 16, 26, 111, 5)
    assert a['rounds'] * 3 <= LOOKUP_NEW and b['step_rounds'] * 2 > b['rounds'] > 30
    # the batch: prompt 0 is frozen from round 6 on, so every later round is a verify pass - no plain step in this batch
    ab = R.simulate_lookup_rounds(p, c, LOOKUP_N, LOOKUP_G, LOOKUP_NEW)
    np.testing.assert_array_equal(ab['tokens'], np.stack(c)[:, :LOOKUP_NEW])
    assert (ab['rounds'], ab['verify_rounds'], ab['step_rounds']) == (42, 42, 0)


def test_the_second_batch_of_the_gpu_test_runs_both_kinds_of_round():
    p, c = fixture(LOOKUP_BATCHES[1])
    st = R.simulate_lookup_rounds(p, c, LOOKUP_N, LOOKUP_G, LOOKUP_NEW)
    np.testing.assert_array_equal(st['tokens'], np.stack(c)[:, :LOOKUP_NEW])
    assert st['step_rounds'] > 0 and st['verify_rounds'] > 0 and st['rounds'] < LOOKUP_NEW
