"""tllm_session_append_ragged / tllm_session_append_ragged_generate: a different number of tokens per sequence onto the live cache in
one prefill pass.  For sequence b the call is tllm_session_append with n = n_b, so every sequence is held to the oracles'
teacher-forced logits on ITS OWN token chain (oracle rows are independent), and the call as a whole to what defines it: with every
n_b = W it is the uniform entry bit for bit, and what stands behind the lengths in a row is never read."""
import numpy as np
import pytest

from oracle import llama_oracle as O
from oracle import quant_oracle as QO
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime.native import NativeSession, _lib
from test_gpu_score import TINY_BOUND, kv_bytes, load_tiny, quant_session, synth_bounds, tiny_session
from test_gpu_session_append import (FP8_KV, ONE_BYTE_INPUTS, SYNTH_N, SYNTH_STEPS, close, forced_steps, synth_inputs,
                                     tp_rank_session)

pytestmark = pytest.mark.gpu
LENGTHS = np.array([20, 9], np.int32)  # of W = 20, head size 64: the MFMA kernel with one sequence below its threshold of 16


def everything(s, nbytes, layers=2):
    """logits, token record, the four step-state arrays, the KV bytes"""
    st = s.step_state()
    return [s.logits(), s.output_ids()] + [st[k] for k in sorted(st)] + kv_bytes(s, layers, nbytes)


def same_everything(a, b, what=''):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f'{what}: item {i} differs'


# ------------------------------------------------------------------------------------------------ (a) tiny fp16 model
def test_tiny_model_ragged_appends_against_the_oracle_on_every_sequences_own_chain():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    assert B == 2 and S == 8 and len(set(lens.tolist())) == 2
    NEW, H, Dh = 8, 2, 32
    smax = S + NEW
    r = np.random.default_rng(22)
    a1, n1 = r.integers(3, 128, (B, 3)).astype(np.int32), np.array([3, 1], np.int32)
    forced = r.integers(3, 128, (B, 2)).astype(np.int32)
    a2, n2 = r.integers(3, 128, (B, 5)).astype(np.int32), np.array([2, 5], np.int32)
    chains = [np.concatenate([a1[b, :n1[b]], forced[b], a2[b, :n2[b]]]) for b in range(B)]
    assert [len(c) for c in chains] == [7, 8]  # sequence 1 ends in the cache's last slot
    a1[1, 1:], a2[0, 2:] = -1, 128 + 5         # behind the lengths: never read
    # one oracle chain, a row per sequence (rows are independent): ref[i][b] = the logits behind token i of sequence b's chain
    fed = np.stack([np.concatenate([chains[0], [3]]), chains[1]]).astype(np.int32)
    ow = {k: w[k].astype(np.float32) for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    ow['layers'] = [{k[len(f'layers.{i}.'):]: w[k].astype(np.float32) for k in w if k.startswith(f'layers.{i}.')} for i in range(2)]
    caches = [np.zeros((B, 2, H, smax, Dh), np.float16) for _ in range(2)]
    O.llama_logits_context(ids, ow, caches, lens, H)
    masked = np.zeros((B, smax), np.int32)
    for b in range(B):
        masked[b, lens[b]:S] = 1
    ref = [O.llama_logits_decode(fed[:, i], ow, caches, [S + i] * B, lens, S, S + i, H, masked) for i in range(fed.shape[1])]

    s = tiny_session(w)
    s.setup(B, S, NEW)
    s.context(ids, lens)
    done = np.zeros(B, np.int64)

    def stage(tag, logits, record_before=None):
        st = s.step_state()
        rec = s.output_ids()
        for b in range(B):
            close(logits[b:b + 1], ref[done[b] - 1][b:b + 1], TINY_BOUND, tag=f'tiny {tag} b={b}')
            assert st['sequence_length'][b] == S + done[b], (tag, b)
            assert st['next_position'][b] == S + done[b] - (S - lens[b]), (tag, b)
            np.testing.assert_array_equal(rec[b, S:S + done[b]], chains[b][:done[b]], err_msg=f'{tag} b={b}')
            if record_before is not None:  # nothing behind the pending token's slot p_b + n_b
                np.testing.assert_array_equal(rec[b, S + done[b] + 1:], record_before[b, S + done[b] + 1:], err_msg=f'{tag} b={b}')

    before = s.output_ids()
    s.append(a1, lengths=n1)
    done += n1
    stage('append (3, 1)', s.logits(), before)
    for j in range(2):
        s.force_tokens(forced[:, j])
        s.step(1, use_graph=False)
        done += 1
        stage(f'forced step {j}', s.logits())
    before = s.output_ids()
    s.append(a2, lengths=n2)
    done += n2
    stage('append (2, 5)', s.logits(), before)
    assert s.step_state()['sequence_length'].tolist() == [smax - 1, smax]
    assert s.append_launches() == (2 * 2, 0)  # head size 32: the wave kernel, one launch per layer and call
    s.close()


# ------------------------------------------------------------------------------------------------ (b) modes x cache types
def ragged_feed(feed, extra):
    """[2, 20 + steps]: row b = the LENGTHS[b] appended ids of sequence b, the forced ids of the steps, filler"""
    out = np.full((2, SYNTH_N + extra.shape[1]), 3, np.int32)
    for b in range(2):
        nb = LENGTHS[b]
        out[b, :nb] = feed[b, :nb]
        out[b, nb:nb + extra.shape[1]] = extra[b]
    return out


def run_ragged(s, ids, lens, feed):
    """context, the ragged append of feed[:, :20] with LENGTHS, SYNTH_STEPS forced steps; the logits after each"""
    s.setup(2, ids.shape[1], SYNTH_N + SYNTH_STEPS + 1)
    s.context(ids, lens)
    padded = feed[:, :SYNTH_N].copy()
    padded[1, LENGTHS[1]:] = -1
    s.append(padded, lengths=LENGTHS)
    return [s.logits()] + forced_steps(s, feed[:, SYNTH_N:])


def hold_to_own_chain(got, ref, mode, tag):
    for j, g in enumerate(got):
        for b in range(2):
            z = np.asarray(ref[LENGTHS[b] + j])
            bmax, bmean = synth_bounds(mode, z)  # (as tests/test_append_ragged_ref.py's headroom check takes them)
            close(g[b:b + 1], z[b:b + 1], bmax, bmean, tag=f'{tag} b={b} {"append" if j == 0 else f"step {j}"}')


@pytest.mark.parametrize('mode,cache,keys', [
    ('fp16', 'fp16', {}), ('woq8', 'int8', {}), ('sq_dyn_pc', 'int8', {}), ('sq_static_pc', 'fp16', {}),
    ('fp16', 'fp16', dict(remove_input_padding=1))],
    ids=['fp16-fp16', 'woq8-int8', 'sq_dyn_pc-int8', 'sq_static_pc-fp16', 'fp16-fp16-packed'])
def test_quantised_modes_against_the_teacher_forced_oracle_per_sequence(mode, cache, keys):
    """context, ragged append (20, 9) of W = 20 (N = 20, head size 64: the MFMA kernel, sequence 1 below its threshold), 3 forced
    steps; sequence b against quant_oracle.run_model fed ITS chain, at index n_b + j.  The int8-cache modes on ONE_BYTE_INPUTS
    (tests/test_append_ragged_ref.py holds the rule itself to half the bounds there)."""
    cfg, w, ids, lens, feed = synth_inputs(**(ONE_BYTE_INPUTS if cache == 'int8' else {}))
    S = ids.shape[1]
    qmodel = QO.quantise_model(cfg, w, mode, 1 if cache == 'int8' else 0, calib_ids=ids, calib_lens=lens)
    chain = ragged_feed(feed, feed[:, SYNTH_N:])
    ref, _ = QO.run_model(qmodel, ids, lens, 1 + chain.shape[1], feed_ids=chain)
    s = quant_session(cfg, qmodel, **keys)
    got = run_ragged(s, ids, lens, feed)
    assert s.append_launches() == (0, cfg['num_layers'])
    rec, st = s.output_ids(), s.step_state()
    s.close()
    for b in range(2):
        nb = LENGTHS[b] + SYNTH_STEPS
        np.testing.assert_array_equal(rec[b, S:S + nb], chain[b, :nb])
        assert st['sequence_length'][b] == S + nb
    hold_to_own_chain(got, ref, mode, f'{mode} {cache}')


def test_the_kernel_is_chosen_by_the_longest_length_not_by_the_row_width():
    cfg, w, ids, lens, feed = synth_inputs()
    qmodel = QO.quantise_model(cfg, w, 'fp16', 0, calib_ids=ids, calib_lens=lens)
    s = quant_session(cfg, qmodel)
    s.setup(2, ids.shape[1], SYNTH_N + 1)
    s.context(ids, lens)
    s.append(feed[:, :SYNTH_N], lengths=[3, 2])
    assert s.append_launches() == (cfg['num_layers'], 0)
    assert s.step_state()['sequence_length'].tolist() == [ids.shape[1] + 3, ids.shape[1] + 2]
    s.append(feed[:, :SYNTH_N], lengths=[3, 16])
    assert s.append_launches() == (cfg['num_layers'], cfg['num_layers'])
    s.close()


def test_fp8_cache_against_the_engines_own_forced_steps_per_sequence():
    """as tests/test_gpu_session_append.py's fp8 test and for its reason: the ragged append (20, 9) against the same engine's
    forced steps - run once, 20 of them, sequence 1 read at step 9 - at twice synth_bounds' max bound"""
    mode = 'fp16'
    cfg, w, ids, lens, feed = synth_inputs(**ONE_BYTE_INPUTS)
    qmodel = QO.quantise_model(cfg, w, mode, 0, calib_ids=ids, calib_lens=lens)
    tensors = dict(qmodel['engine_tensors'])
    for i in range(cfg['num_layers']):
        tensors[f'layers.{i}.attention.kv_orig_quant_scale'] = np.array([8.0], np.float32)
        tensors[f'layers.{i}.attention.kv_quant_orig_scale'] = np.array([0.125], np.float32)
    got = {}
    for route in 'AB':
        s = NativeSession(dict(cfg, quant_mode=qmodel['quant_mode'] | FP8_KV))
        for k, v in tensors.items():
            s.set_tensor(k, v)
        s.finalize()
        s.setup(2, ids.shape[1], SYNTH_N + 1)
        s.context(ids, lens)
        if route == 'A':
            s.append(feed[:, :SYNTH_N], lengths=LENGTHS)
            got[route] = s.logits()
            assert s.append_launches() == (0, cfg['num_layers'])
        else:
            steps = forced_steps(s, feed[:, :SYNTH_N])
            got[route] = np.stack([steps[LENGTHS[b] - 1][b] for b in range(2)])
        s.close()
    for b in range(2):
        gb = got['B'][b:b + 1]
        close(got['A'][b:b + 1], gb.astype(np.float64), 2 * synth_bounds(mode, gb)[0], tag=f'fp8 ragged b={b}')


def test_grouped_heads_against_the_replicated_multi_head_oracle_per_sequence():
    cfg, w, ids, lens, feed = synth_inputs()
    H, Hkv, Dh = 4, 2, 64
    wg, wm = dict(w), dict(w)
    for i in range(cfg['num_layers']):
        k = f'layers.{i}.attention.qkv.weight'
        wg[k] = np.ascontiguousarray(G.fold_qkv(w[k].T, H, Hkv, Dh).T)
        wm[k] = np.ascontiguousarray(G.expand_qkv_weight(wg[k], H, Hkv, Dh))
    chain = ragged_feed(feed, feed[:, SYNTH_N:])
    ref, _ = QO.run_fp16_model(cfg, wm, ids, lens, 1 + chain.shape[1], feed_ids=chain)
    s = NativeSession(dict(cfg, quant_mode=0, num_kv_heads=Hkv))
    for k, v in wg.items():
        s.set_tensor(k, v)
    s.finalize()
    got = run_ragged(s, ids, lens, feed)
    s.close()
    hold_to_own_chain(got, ref, 'fp16', 'gqa ragged')


# ------------------------------------------------------------------------------------------------ (c) what defines the call
def tiny_pair(new=8):
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    pair = []
    for _ in range(2):
        s = tiny_session(w)
        s.setup(B, S, new)
        s.context(ids, lens)
        s.step(1)
        pair.append(s)
    return pair, B, B * 2 * 2 * (S + new) * 32 * 2


def test_lengths_all_equal_to_the_width_are_the_uniform_append_bit_for_bit():
    (a, b), B, nbytes = tiny_pair()
    tok = np.random.default_rng(5).integers(3, 128, (B, 4)).astype(np.int32)
    a.append(tok, lengths=[4, 4])
    b.append(tok)
    same_everything(everything(a, nbytes), everything(b, nbytes), 'lengths (4, 4) against append')
    a.step(2)
    b.step(2)
    same_everything(everything(a, nbytes), everything(b, nbytes), 'two steps later')
    a.close()
    b.close()


def test_what_stands_behind_the_lengths_is_never_read():
    (a, b), B, nbytes = tiny_pair()
    tok = np.random.default_rng(6).integers(3, 128, (B, 4)).astype(np.int32)
    ta, tb = tok.copy(), tok.copy()
    ta[0, 3], ta[1, 1:] = -1, 128 + 5
    tb[0, 3], tb[1, 1:] = 5, 5
    a.append(ta, lengths=[3, 1])
    b.append(tb, lengths=[3, 1])
    same_everything(everything(a, nbytes), everything(b, nbytes), 'padding -1 / vocab + 5 against 5')
    rec = a.output_ids()
    assert (rec != -1).all() and (rec != 128 + 5).all(), 'a padded id reached the token record'
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (d) append_generate
def ragged_turns(w, ids, lens, user, lengths, sampling=None, new=6, generate=True):
    B, S = ids.shape
    s = tiny_session(w)
    s.setup(B, S, 24)
    if sampling:
        s.set_sampling(**sampling)
    s.generate(ids, lens, new, end_id=-1)
    if generate:
        rec = s.append_generate(user, new, end_id=-1, lengths=lengths)
    else:
        s.append(user, lengths=lengths)
        s.step(new - 1, use_graph=True)
        rec = s.output_ids()
    state = s.step_state()
    s.close()
    return rec, state


def test_append_generate_with_lengths_is_the_ragged_append_and_steps():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    user = np.random.default_rng(3).integers(3, 128, (B, 4)).astype(np.int32)
    lengths = np.array([4, 2], np.int32)
    user[1, 2:] = -1
    got, state = ragged_turns(w, ids, lens, user, lengths)
    want, wstate = ragged_turns(w, ids, lens, user, lengths, generate=False)
    p = S + 5  # five steps behind the prompt pass; the sixth token is pending and the first user token takes its place
    for b in range(B):
        end = p + lengths[b] + 6
        np.testing.assert_array_equal(got[b, :end], want[b, :end])
        np.testing.assert_array_equal(got[b, p:p + lengths[b]], user[b, :lengths[b]])
        assert (got[b, end:] == 0).all(), 'end_id < 0: the tail behind past + n_b + max_new_tokens is pad_id'
        assert state['sequence_length'][b] == wstate['sequence_length'][b] == p + lengths[b] + 5


def test_append_generate_with_lengths_draws_the_same_tokens_in_two_sessions():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    user = np.random.default_rng(3).integers(3, 128, (2, 4)).astype(np.int32)
    cfg = dict(top_k=8, temperature=0.8, random_seed=7)
    a = ragged_turns(w, ids, lens, user, [4, 2], sampling=cfg)
    b = ragged_turns(w, ids, lens, user, [4, 2], sampling=cfg)
    np.testing.assert_array_equal(a[0], b[0])
    greedy = ragged_turns(w, ids, lens, user, [4, 2])
    assert not np.array_equal(a[0], greedy[0])


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_refusals_leave_the_session_untouched():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    NEW = 6
    tok = np.full((B, 2), 5, np.int32)
    s = tiny_session(w)
    with pytest.raises(RuntimeError, match='setup'):
        s.append(tok, lengths=[2, 1])
    s.setup(B, S, NEW)
    with pytest.raises(RuntimeError, match='context'):
        s.append(tok, lengths=[2, 1])
    s.context(ids, lens)
    s.step(1)
    nbytes = B * 2 * 2 * (S + NEW) * 32 * 2

    def snapshot():
        return s.logits(), s.output_ids(), s.step_state(), kv_bytes(s, 1, nbytes)[0]

    def untouched(what):
        after = snapshot()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3]), what
        for k in before[2]:
            assert np.array_equal(before[2][k], after[2][k]), (what, k)

    before = snapshot()
    room = S + NEW - (S + 1)  # slots left behind the prompt and one step
    assert room + 1 <= S, 'the capacity case must not be refused for its width'
    for what, bad, lengths, why in (
            ('a length 0', tok, [2, 0], 'out of range'),
            ('a length W + 1', tok, [3, 1], 'out of range'),
            ('W = 0', np.zeros((B, 0), np.int32), [0, 0], 'out of range'),
            ('W > max_input_len', np.full((B, S + 1), 5, np.int32), [1, 1], 'out of range'),
            ('p + n_b > Smax by one for one sequence only', np.full((B, room + 1), 5, np.int32), [1, room + 1], 'capacity'),
            ('id >= vocab in front of a length', np.array([[5, 128], [5, 5]], np.int32), [2, 1], 'outside'),
            ('id < 0 in front of a length', np.array([[5, 5], [-1, 5]], np.int32), [1, 1], 'outside')):
        with pytest.raises(RuntimeError, match=why):
            s.append(bad, lengths=lengths)
        untouched(what)
        with pytest.raises(RuntimeError, match=why):
            s.append_generate(bad, 1, lengths=lengths)
        untouched(what + ' (generate)')
    # lengths NULL at the C entry
    assert _lib().tllm_session_append_ragged(s._h, tok.ctypes.data, None, 2, 0) != 0
    out = np.empty((B, S + NEW), np.int32)
    assert _lib().tllm_session_append_ragged_generate(s._h, tok.ctypes.data, None, 2, 1, -1, 0, out.ctypes.data, 0) != 0
    untouched('lengths NULL')
    # the generate loop's tokens count against the capacity per sequence
    with pytest.raises(RuntimeError, match='capacity'):
        s.append_generate(np.full((B, room), 5, np.int32), 2, lengths=[1, room - 1])
    untouched('p + n_b + max_new_tokens > Smax by one for one sequence only')
    # accepted: an id >= vocab (and one < 0) behind a length
    s.append(np.array([[5, 128], [5, 5]], np.int32), lengths=[1, 2])
    assert s.step_state()['sequence_length'].tolist() == [S + 2, S + 3]
    s.append(np.array([[5, 5, 5, 5], [5, -1, -1, -1]], np.int32), lengths=[4, 1])  # sequence 0 ends exactly at the capacity
    assert s.step_state()['sequence_length'].tolist() == [S + NEW, S + 4]
    s.close()
    for keys, beam in ((dict(paged_kv_cache=1, tokens_per_block=16), 1), ({}, 2)):
        s = tiny_session(w, **keys)
        s.setup(B, S, NEW, beam)
        s.context(ids, lens)
        with pytest.raises(RuntimeError, match='not built'):
            s.append(np.full((B * beam, 2), 5, np.int32)[:B], lengths=[2, 1])
        s.close()
    s = tp_rank_session()
    s.setup(1, 8, 4)
    s.fake_context(8, seed=3)
    with pytest.raises(RuntimeError, match='not built'):
        s.append(np.full((1, 2), 5, np.int32), lengths=[1])
    s.close()


# ------------------------------------------------------------------------------------------------ (f) front-end
def test_generation_session_takes_input_lengths_and_gives_the_native_sessions_result():
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_frontend import build_tiny_engine
    engine, _, t = build_tiny_engine(QuantMode(0))
    _, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    r = np.random.default_rng(3)
    user, more = r.integers(3, 128, (B, 4)).astype(np.int32), r.integers(3, 128, (B, 3)).astype(np.int32)
    ul, ml = np.array([4, 2], np.int32), np.array([1, 3], np.int32)
    user[1, 2:], more[0, 1:] = -1, 128
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    dec.setup(B, S, 24)
    scfg = SamplingConfig(end_id=-1, pad_id=0)
    dec.decode(ids, lens, scfg, max_new_tokens=6)
    t2 = dec.decode_append(user, scfg, max_new_tokens=6, input_lengths=ul)
    logits = dec.append(more, input_lengths=ml)
    assert t2.shape == (B, 1, S + 24) and logits.shape == (B, 128)
    nat = tiny_session(w)
    nat.setup(B, S, 24)
    nat.generate(ids, lens, 6, end_id=-1)
    n2 = nat.append_generate(user, 6, end_id=-1, lengths=ul)
    nat.append(more, lengths=ml)
    np.testing.assert_array_equal(t2[:, 0], n2)
    close(logits, nat.logits().astype(np.float64), TINY_BOUND, tag='front-end ragged append')
    np.testing.assert_array_equal(dec.runtime.step_state()['sequence_length'], nat.step_state()['sequence_length'])
    # with max_new_tokens left open, decode_append fills the room of the sequence that has the least left
    used = nat.step_state()['sequence_length'] + ml
    nat.close()
    dec.decode_append(more, scfg, input_lengths=ml)
    after = dec.runtime.step_state()['sequence_length']
    assert int(after.max()) == S + 24 - 1 and (after - used == after[0] - used[0]).all()
    for bad, err in ((ul[:1], ValueError), (ul.astype(np.float32), TypeError), (np.array([0, 2]), ValueError),
                     (np.array([5, 2]), ValueError), (np.array([4, 3]), ValueError), (np.array([[4, 2]]), ValueError)):
        with pytest.raises(err):
            dec.append(user, input_lengths=bad)
        with pytest.raises(err):
            dec.decode_append(user, scfg, input_lengths=bad)
