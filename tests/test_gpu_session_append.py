"""tllm_session_append / tllm_session_append_generate: n tokens onto the live cache in one prefill pass, held to what defines it -
the sequence  force_tokens(ids[:, i]); step(1)  of the same session code (route B) - and to the oracles' teacher-forced logits."""
import numpy as np
import pytest

from oracle import llama_oracle as O
from oracle import quant_oracle as QO
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import TINY_BOUND, kv_bytes, load_tiny, quant_session, synth_bounds, synth_model, tiny_session

pytestmark = pytest.mark.gpu
FP8_KV = 64


def same_state(a, b, upto):
    """token record on the slots written, all four step-state arrays (next_position = where the next RoPE row was taken)"""
    np.testing.assert_array_equal(a.output_ids()[:, :upto], b.output_ids()[:, :upto])
    sa, sb = a.step_state(), b.step_state()
    for k in ('sequence_length', 'next_position', 'masked_tokens', 'input_lengths'):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)


def forced_steps(s, ids):
    """route B: ids [B, n] one generation step at a time; the logits after every step"""
    out = []
    for i in range(ids.shape[1]):
        s.force_tokens(ids[:, i])
        s.step(1, use_graph=i >= 2)
        out.append(s.logits())
    return out


def close(got, ref, bmax, bmean=None, tag=''):
    d = np.abs(got.astype(np.float64) - ref)
    print(f'[{tag}] max |d| {d.max():.3e} (bound {bmax:.3e}), mean {d.mean():.3e}' + (f' (bound {bmean:.3e})' if bmean else ''))
    assert d.max() <= bmax, f'{tag}: {d.max():.3e} > {bmax:.3e}'
    assert bmean is None or d.mean() <= bmean, f'{tag}: mean {d.mean():.3e} > {bmean:.3e}'


# ------------------------------------------------------------------------------------------------ (a) tiny fp16 model
def test_tiny_model_append_equals_forced_steps_and_the_oracle():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    assert B == 2 and S == 8 and len(set(lens.tolist())) == 2  # ragged
    NEW, H, Dh = 12, 2, 32
    smax = S + NEW
    r = np.random.default_rng(21)
    feed = r.integers(3, 128, (B, 3 + 4 + 5)).astype(np.int32)  # append 3, 4 forced steps, append 5
    # the oracle's teacher-forced chain
    ow = {k: w[k].astype(np.float32) for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    ow['layers'] = [{k[len(f'layers.{i}.'):]: w[k].astype(np.float32) for k in w if k.startswith(f'layers.{i}.')} for i in range(2)]
    caches = [np.zeros((B, 2, H, smax, Dh), np.float16) for _ in range(2)]
    O.llama_logits_context(ids, ow, caches, lens, H)
    masked = np.zeros((B, smax), np.int32)
    for b in range(B):
        masked[b, lens[b]:S] = 1
    ref = [O.llama_logits_decode(feed[:, i], ow, caches, [S + i] * B, lens, S, S + i, H, masked) for i in range(feed.shape[1])]

    a, b = tiny_session(w), tiny_session(w)
    a.setup(B, S, NEW)
    b.setup(B, S, NEW)
    a.context(ids, lens)
    b.context(ids, lens)
    a.append(feed[:, :3])
    lb = forced_steps(b, feed[:, :3])
    same_state(a, b, S + 3 + 1)  # the three appended ids and the new pending token
    np.testing.assert_array_equal(a.output_ids()[:, S:S + 3], feed[:, :3])
    assert (a.step_state()['sequence_length'] == S + 3).all()
    close(a.logits(), ref[2], TINY_BOUND, tag='tiny append 3')
    close(lb[-1], ref[2], TINY_BOUND, tag='tiny forced 3')
    # four more teacher-forced steps on both routes: they read the appended K/V
    la, lb = forced_steps(a, feed[:, 3:7]), forced_steps(b, feed[:, 3:7])
    for i in range(4):
        close(la[i], ref[3 + i], TINY_BOUND, tag=f'tiny A step {i}')
        close(lb[i], ref[3 + i], TINY_BOUND, tag=f'tiny B step {i}')
    same_state(a, b, S + 7)
    # a second append on route A, up to the cache's last slot
    a.append(feed[:, 7:12])
    close(a.logits(), ref[11], TINY_BOUND, tag='tiny append 5')
    assert (a.step_state()['sequence_length'] == smax).all()
    np.testing.assert_array_equal(a.output_ids()[:, S:], feed)
    assert a.append_launches() == (2 * 2, 0)  # head size 32: the wave kernel, one launch per layer and call
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (b) modes x cache types
# (the prompts are padded to 20, not 16: an append of n = 20 needs max_input_len >= 20 - the activation buffers are the prompt's)
SYNTH_S, SYNTH_N, SYNTH_STEPS = 20, 20, 3
# The cases with a one-byte cache run on longer prompts (120 / 97 of 128).  A teacher-forced step reads EVERY earlier token from the
# quantised cache, the append reads its own 20 tokens un-quantised (the rule): behind 12 / 7 prompt tokens those 20 are most of
# what a query sees, and the rule alone is 1.5e-1 (int8) and 3.6e-1 - 5.1e-1 (fp8) from the teacher-forced logits (measured on the
# MI355X with woq8 / fp16 / woq4 weights) - above the weight-only bound of 1.1e-1.  Behind 120 / 97 tokens it is 0.3 - 0.4 of the
# bounds (tests/test_append_ref.py::test_headroom_of_the_one_byte_cache_session_cases, which holds these inputs to half of them).
ONE_BYTE_INPUTS = dict(seed=5, S=128, prompt=(120, 97))
INT8_CACHE_MODES = ('woq8', 'sq_dyn_pc')  # the modes of the parametrisation below that run with the int8 cache


def synth_inputs(seed=5, S=SYNTH_S, prompt=(12, 7)):
    cfg, w = synth_model(11)
    cfg = dict(cfg, max_position_embeddings=256)
    r = np.random.default_rng(seed)
    ids = r.integers(3, cfg['vocab_size'], (2, S)).astype(np.int32)
    lens = np.array(prompt, np.int32)
    for b in range(2):
        ids[b, lens[b]:] = 2
    feed = r.integers(3, cfg['vocab_size'], (2, SYNTH_N + SYNTH_STEPS)).astype(np.int32)
    return cfg, w, ids, lens, feed


def run_route_a(s, ids, lens, feed):
    s.setup(2, ids.shape[1], SYNTH_N + SYNTH_STEPS + 1)
    s.context(ids, lens)
    s.append(feed[:, :SYNTH_N])
    return [s.logits()] + forced_steps(s, feed[:, SYNTH_N:])


@pytest.mark.parametrize('mode,cache,keys', [
    ('fp16', 'fp16', {}), ('woq8', 'int8', {}), ('woq4', 'fp16', {}), ('sq_static_pc', 'fp16', {}), ('sq_dyn_pc', 'fp16', {}),
    ('sq_dyn_pc', 'int8', {}), ('fp16', 'fp16', dict(remove_input_padding=1))],
    ids=['fp16-fp16', 'woq8-int8', 'woq4-fp16', 'sq_static_pc-fp16', 'sq_dyn_pc-fp16', 'sq_dyn_pc-int8', 'fp16-fp16-packed'])
def test_quantised_modes_against_the_teacher_forced_oracle(mode, cache, keys):
    """context (12 / 7 of 20; int8 cache: 120 / 97 of 128), append 20 (the MFMA kernel: head size 64), 3 forced steps, against
    quant_oracle.run_model fed the same ids one step at a time"""
    assert cache != 'int8' or mode in INT8_CACHE_MODES  # (the headroom check runs exactly these)
    cfg, w, ids, lens, feed = synth_inputs(**(ONE_BYTE_INPUTS if cache == 'int8' else {}))
    S = ids.shape[1]
    qmodel = QO.quantise_model(cfg, w, mode, 1 if cache == 'int8' else 0, calib_ids=ids, calib_lens=lens)
    ref, _ = QO.run_model(qmodel, ids, lens, 1 + feed.shape[1], feed_ids=feed)
    s = quant_session(cfg, qmodel, **keys)
    got = run_route_a(s, ids, lens, feed)
    assert s.append_launches() == (0, cfg['num_layers'])
    np.testing.assert_array_equal(s.output_ids()[:, S:S + feed.shape[1]], feed)
    s.close()
    for i, g in enumerate(got):
        z = ref[SYNTH_N + i]
        bmax, bmean = synth_bounds(mode, z)
        close(g, z, bmax, bmean, tag=f'{mode} {cache} {"append" if i == 0 else f"step {i}"}')


@pytest.mark.parametrize('mode', ['fp16', 'woq4'])
def test_fp8_cache_against_the_engines_own_forced_steps(mode):
    """the quantisation oracle does not model the fp8 cache: route A (append) against route B (forced steps) of the same engine,
    at twice synth_bounds' max bound - each route is within one bound of the same function.  On the longer prompts of the
    one-byte cases (ONE_BYTE_INPUTS: route B reads the 20 tokens from the E4M3 cache, 3 mantissa bits, route A un-quantised)."""
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
        if route == 'A':
            got[route] = run_route_a(s, ids, lens, feed)
        else:
            s.setup(2, ids.shape[1], SYNTH_N + SYNTH_STEPS + 1)
            s.context(ids, lens)
            got[route] = forced_steps(s, feed)[SYNTH_N - 1:]
        s.close()
    for i, (ga, gb) in enumerate(zip(got['A'], got['B'])):
        close(ga, gb.astype(np.float64), 2 * synth_bounds(mode, gb)[0], tag=f'fp8 {mode} {"append" if i == 0 else f"step {i}"}')


def test_grouped_heads_against_the_replicated_multi_head_oracle():
    """Hkv = 2 of H = 4: the engine runs the folded QKV weight, the oracle the multi-head model with every K/V head repeated"""
    cfg, w, ids, lens, feed = synth_inputs()
    H, Hkv, Dh = 4, 2, 64
    wg, wm = dict(w), dict(w)
    for i in range(cfg['num_layers']):
        k = f'layers.{i}.attention.qkv.weight'
        wg[k] = np.ascontiguousarray(G.fold_qkv(w[k].T, H, Hkv, Dh).T)
        wm[k] = np.ascontiguousarray(G.expand_qkv_weight(wg[k], H, Hkv, Dh))
    ref, _ = QO.run_fp16_model(cfg, wm, ids, lens, 1 + feed.shape[1], feed_ids=feed)
    s = NativeSession(dict(cfg, quant_mode=0, num_kv_heads=Hkv))
    for k, v in wg.items():
        s.set_tensor(k, v)
    s.finalize()
    got = run_route_a(s, ids, lens, feed)
    s.close()
    for i, g in enumerate(got):
        bmax, bmean = synth_bounds('fp16', ref[SYNTH_N + i])
        close(g, ref[SYNTH_N + i], bmax, bmean, tag=f'gqa {"append" if i == 0 else f"step {i}"}')


# ------------------------------------------------------------------------------------------------ (c) chunked = one-shot
def test_chunked_prefill_equals_the_one_shot_prefill():
    cfg, w = synth_model(11)
    cfg = dict(cfg, max_position_embeddings=256)
    total, first = 165, 64
    r = np.random.default_rng(8)
    ids = r.integers(3, cfg['vocab_size'], (1, total)).astype(np.int32)
    qmodel = QO.quantise_model(cfg, w, 'fp16', 0, calib_ids=ids[:, :32], calib_lens=np.array([32], np.int32))
    z = np.asarray(QO.run_model(qmodel, ids, np.array([total], np.int32), 1)[0][0], np.float64)
    bmax, bmean = synth_bounds('fp16', z)
    a = quant_session(cfg, qmodel)
    a.setup(1, first, total - first + 4)
    a.context(ids[:, :first], np.array([first], np.int32))
    a.append(ids[:, first:2 * first])
    assert a.append_launches() == (0, cfg['num_layers']), 'the 64-token chunk must run the MFMA kernel'
    a.append(ids[:, 2 * first:])
    assert a.append_launches() == (0, 2 * cfg['num_layers'])
    b = quant_session(cfg, qmodel)
    b.setup(1, total, 4)
    b.context(ids, np.array([total], np.int32))
    close(a.logits(), z, bmax, bmean, tag='chunked 64 + 64 + 37')
    close(b.logits(), z, bmax, bmean, tag='one-shot 165')
    assert (a.step_state()['sequence_length'] == total).all() and (a.step_state()['next_position'] == total).all()
    np.testing.assert_array_equal(a.output_ids()[:, :total], ids)
    top2 = np.sort(z[0])[-2:]
    if top2[1] - top2[0] >= bmax:
        assert a.output_ids()[0, total] == b.output_ids()[0, total] == int(z[0].argmax())
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (d) append_generate
def tiny_turns(w, ids, lens, user, end_id=-1, sampling=None, new=6):
    B, S = ids.shape
    s = tiny_session(w)
    s.setup(B, S, 24)
    if sampling:
        s.set_sampling(**sampling)
    t1 = s.generate(ids, lens, new, end_id=end_id)
    t2 = s.append_generate(user, new, end_id=end_id)
    state = s.step_state()
    s.close()
    return t1, t2, state


def test_append_generate_equals_teacher_forced_generation():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    user = np.random.default_rng(3).integers(3, 128, (B, 4)).astype(np.int32)
    t1, t2, state = tiny_turns(w, ids, lens, user)
    p = S + 5  # five steps behind the prompt pass: the sixth token is pending and the first user token takes its place
    np.testing.assert_array_equal(t2[:, :p], t1[:, :p])
    np.testing.assert_array_equal(t2[:, p:p + 4], user)
    assert (state['sequence_length'] == p + 4 + 5).all()
    assert (t2[:, p + 4 + 6:] == 0).all()  # end_id < 0: the unused tail is pad_id
    # route B: the same record teacher-forced one step at a time, then five free steps
    s = tiny_session(w)
    s.setup(B, S, 24)
    s.generate(ids, lens, 6, end_id=-1)
    forced_steps(s, user)
    s.step(5, use_graph=True)
    np.testing.assert_array_equal(t2[:, :p + 4 + 6], s.output_ids()[:, :p + 4 + 6])
    s.close()


def test_append_generate_draws_the_same_tokens_in_two_sessions():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    user = np.random.default_rng(3).integers(3, 128, (2, 4)).astype(np.int32)
    cfg = dict(top_k=8, temperature=0.8, random_seed=7)
    a = tiny_turns(w, ids, lens, user, sampling=cfg)
    b = tiny_turns(w, ids, lens, user, sampling=cfg)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    greedy = tiny_turns(w, ids, lens, user)
    assert not np.array_equal(a[1], greedy[1])


def test_generation_continues_after_an_end_id_hit_in_the_first_turn():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    user = np.random.default_rng(3).integers(3, 128, (B, 4)).astype(np.int32)
    free, _, _ = tiny_turns(w, ids, lens, user)
    end_id = int(free[0, S + 2])  # sequence 0 stops at its third token
    t1, t2, _ = tiny_turns(w, ids, lens, user, end_id=end_id)
    assert (t1[0, S + 2:] == end_id).all()  # finished: the row emits end_id from there on
    p = S + 5
    np.testing.assert_array_equal(t2[:, :p], t1[:, :p])
    # reference: the turn-1 record and the user tokens teacher-forced in a session that never finished, then free greedy steps
    s = tiny_session(w)
    s.setup(B, S, 24)
    s.context(ids, lens)
    np.testing.assert_array_equal(s.output_ids()[:, S], t1[:, S])  # the prompt pass's own token
    s.step(1)
    forced_steps(s, np.concatenate([t1[:, S + 1:p], user], axis=1))
    s.step(5, use_graph=False)
    want = s.output_ids()[:, :p + 4 + 6].copy()
    s.close()
    assert want[0, p + 4] != end_id, 'choose another case: the continuation itself starts with end_id'
    for b in range(B):  # the tail rule of generate: behind the first end_id among the new tokens the row is end_id
        hit = np.nonzero(want[b, p + 4:] == end_id)[0]
        if len(hit):
            want[b, p + 4 + hit[0]:] = end_id
    np.testing.assert_array_equal(t2[:, :p + 4 + 6], want)


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_refusals_leave_the_session_untouched():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    NEW = 6
    tok = np.full((B, 2), 5, np.int32)
    s = tiny_session(w)
    with pytest.raises(RuntimeError, match='setup'):
        s.append(tok)
    s.setup(B, S, NEW)
    with pytest.raises(RuntimeError, match='context'):
        s.append(tok)
    s.context(ids, lens)
    s.step(1)
    nbytes = B * 2 * 2 * (S + NEW) * 32 * 2

    def snapshot():
        return s.logits(), s.output_ids(), s.step_state(), kv_bytes(s, 1, nbytes)[0]

    before = snapshot()
    room = S + NEW - (S + 1)  # slots left behind the prompt and one step
    assert room + 1 <= S, 'the capacity case must not be refused for its length'
    for what, bad, why in (('n = 0', np.zeros((B, 0), np.int32), 'out of range'),
                           ('n > max_input_len', np.full((B, S + 1), 5, np.int32), 'out of range'),
                           ('p + n > Smax by one', np.full((B, room + 1), 5, np.int32), 'capacity'),
                           ('id >= vocab', np.array([[5, 128], [5, 5]], np.int32), 'outside'),
                           ('id < 0', np.array([[5, 5], [-1, 5]], np.int32), 'outside')):
        with pytest.raises(RuntimeError, match=why):
            s.append(bad)
        after = snapshot()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3]), what
        for k in before[2]:
            assert np.array_equal(before[2][k], after[2][k]), (what, k)
    s.append(np.full((B, room), 5, np.int32))  # exactly up to the capacity is served
    s.close()
    for keys, beam in ((dict(paged_kv_cache=1, tokens_per_block=16), 1), ({}, 2)):
        s = tiny_session(w, **keys)
        s.setup(B, S, NEW, beam)
        s.context(ids, lens)
        with pytest.raises(RuntimeError, match='not built'):
            s.append(np.full((B * beam, 2), 5, np.int32)[:B])
        s.close()
    # a tensor-parallel rank (its collectives switched off: one GPU) is refused like any tp > 1 session
    s = tp_rank_session()
    s.setup(1, 8, 4)
    s.fake_context(8, seed=3)
    with pytest.raises(RuntimeError, match='not built'):
        s.append(np.full((1, 2), 5, np.int32))
    s.close()


# ------------------------------------------------------------------------------------------------ (f) front-end
def test_generation_session_append_and_decode_append_give_the_native_sessions_result():
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
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    dec.setup(B, S, 24)
    scfg = SamplingConfig(end_id=-1, pad_id=0)
    t1 = dec.decode(ids, lens, scfg, max_new_tokens=6)
    t2 = dec.decode_append(user, scfg, max_new_tokens=6)
    logits = dec.append(more)
    assert t1.shape == t2.shape == (B, 1, S + 24) and logits.shape == (B, 128)
    nat = tiny_session(w)
    nat.setup(B, S, 24)
    n1 = nat.generate(ids, lens, 6, end_id=-1)
    n2 = nat.append_generate(user, 6, end_id=-1)
    nat.append(more)
    np.testing.assert_array_equal(t1[:, 0], n1)
    np.testing.assert_array_equal(t2[:, 0], n2)
    close(logits, nat.logits().astype(np.float64), TINY_BOUND, tag='front-end append')  # (the engine may pick other GEMM kernels)
    # with max_new_tokens left open, decode_append fills the room the cache has left
    used = int(nat.step_state()['sequence_length'].max())
    rest = dec.decode_append(more, scfg)
    assert (rest[:, 0, used + 3:] != 0).any() and int(dec.runtime.step_state()['sequence_length'].max()) == S + 24 - 1
    nat.close()
    for bad, err in ((user[:1], ValueError), (user.astype(np.float32), TypeError), (np.full((B, S + 1), 5, np.int32), ValueError),
                     (np.full((B, 2), 128, np.int32), ValueError), (user[0], ValueError)):
        with pytest.raises(err):
            dec.append(bad)


def tp_rank_session():
    """rank 0 of a tp = 2 engine with its collectives switched off (session key no_comm), the recipe of
    tests/test_gpu_session.py::test_a_tensor_parallel_rank_without_its_collectives_runs_alone"""
    cfg, w = synth_model(5, L=2, H=4, D=256, I=512, V=512)
    tp = 2
    H, D, I, V = cfg['num_heads'], cfg['hidden_size'], cfg['inter_size'], cfg['vocab_size']
    Dh = D // H
    s = NativeSession(dict(cfg, quant_mode=0, tp_size=tp, tp_rank=0, no_comm=1))
    for k, v in w.items():
        if k.endswith('attention.qkv.weight'):
            v = v.reshape(3, H, Dh, D)[:, :H // tp].reshape(3 * D // tp, D)
        elif k.endswith('attention.dense.weight'):
            v = v[:, :D // tp]
        elif k.endswith('mlp.fc.weight') or k.endswith('mlp.gate.weight'):
            v = v[:I // tp]
        elif k.endswith('mlp.proj.weight'):
            v = v[:, :I // tp]
        elif k == 'lm_head.weight':
            v = v[:V // tp]
        s.set_tensor(k, np.ascontiguousarray(v))
    s.finalize()
    return s
