"""The append passes of a session on the paged KV cache (session keys paged_kv_cache = 1, paged_append = 1): append, the ragged
append, append_generate, verify, verify(sampled), both generate_lookup loops and LoRA on them - a linear and a paged session side by
side on the same inputs.  Paging only changes where a K/V row lives, so everything the getters of test_gpu_session_append*.py and
test_gpu_session_verify*.py return is compared with assert_array_equal, never a tolerance (the linear session is held to the
oracles there).

Block sizes T = 8 and 64 on the synthetic model's padded prompt of 20: with T = 8 the prompt ends mid-block (slot 19 is row 3 of
block 2), an append of 20 covers the slots 20 - 39 and crosses the boundaries at 24 and 32, and a verify of 6 ids at p = 20 writes
into block 3 and is rolled back into block 2."""
import numpy as np
import pytest

from oracle import llama_oracle as O
from oracle import quant_oracle as QO
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime import lora_ref as LR
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import TINY_BOUND, load_tiny, quant_session, tiny_session
from test_gpu_session_append import close, forced_steps, same_state, synth_inputs

pytestmark = pytest.mark.gpu
FP8_KV = 64
NEW = 40  # setup's max_new_tokens: the cache holds 60 slots
MODES = ['fp16-fp16', 'sq_static-int8', 'woq4-fp8', 'gqa-fp16']


def engine(mode):
    """(cfg, tensors, keys, ids, lens, feed) of one mode on the inputs of test_gpu_session_append.synth_inputs"""
    cfg, w, ids, lens, feed = synth_inputs()
    keys = {}
    if mode == 'gqa-fp16':
        H, Hkv, Dh = 4, 2, 64
        tensors = dict(w)
        for i in range(cfg['num_layers']):
            k = f'layers.{i}.attention.qkv.weight'
            tensors[k] = np.ascontiguousarray(G.fold_qkv(w[k].T, H, Hkv, Dh).T)
        keys = dict(quant_mode=0, num_kv_heads=Hkv)
    else:
        qmode, int8_kv = {'fp16-fp16': ('fp16', 0), 'sq_static-int8': ('sq_static_pc', 1), 'woq4-fp8': ('woq4', 0)}[mode]
        qmodel = QO.quantise_model(cfg, w, qmode, int8_kv, calib_ids=ids, calib_lens=lens)
        tensors = dict(qmodel['engine_tensors'])
        keys = dict(quant_mode=qmodel['quant_mode'])
        if mode == 'woq4-fp8':
            keys['quant_mode'] |= FP8_KV
            for i in range(cfg['num_layers']):
                tensors[f'layers.{i}.attention.kv_orig_quant_scale'] = np.array([8.0], np.float32)
                tensors[f'layers.{i}.attention.kv_quant_orig_scale'] = np.array([0.125], np.float32)
    return cfg, tensors, keys, ids, lens, feed


def session(cfg, tensors, keys, paged, T, **more):
    k = dict(cfg, **keys, **more)
    if paged:
        k.update(paged_kv_cache=1, tokens_per_block=T, paged_append=1)
    s = NativeSession(k)
    for name, v in tensors.items():
        s.set_tensor(name, v)
    s.finalize()
    return s


def state(s):
    st = s.step_state()
    return [s.output_ids()] + [st[k] for k in ('sequence_length', 'next_position', 'masked_tokens', 'input_lengths')]


def side_by_side(script, cfg, tensors, keys, T, **more):
    """script(session) -> list of arrays: the linear session's against the paged session's, element for element"""
    res = []
    for paged in (False, True):
        s = session(cfg, tensors, keys, paged, T, **more)
        res.append([np.asarray(x) for x in script(s)])
        s.close()
    assert len(res[0]) == len(res[1]) and len(res[0]) > 0
    for i, (a, b) in enumerate(zip(*res)):
        np.testing.assert_array_equal(a, b, err_msg=f'result {i} of the script')
    return res[0]


# ------------------------------------------------------------------------------------------------ appends
def append_script(ids, lens, feed):
    r = np.random.default_rng(17)
    more = r.integers(3, 500, (2, 9)).astype(np.int32)

    def run(s):
        out = []
        s.setup(2, ids.shape[1], NEW)
        s.context(ids, lens)
        out.append(s.logits())
        s.append(feed[:, :3])  # n = 3: the wave kernel; slots 20 - 22
        out += [s.logits()] + state(s)
        s.step(1)
        out.append(s.logits())
        s.append(feed[:, 3:23])  # n = 20: the MFMA kernel (head size 64); slots 24 - 43
        out += [s.logits()] + state(s)
        s.step(1, use_graph=True)
        out.append(s.logits())
        s.append(more[:, :5], [5, 2])  # ragged
        out += [s.logits()] + state(s)
        out.append(s.append_generate(more[:, 5:9], 3))
        out += [s.logits()] + state(s)
        wave, mfma = s.append_launches()
        assert wave > 0 and mfma > 0
        out.append(np.array([wave, mfma]))
        return out
    return run


@pytest.mark.parametrize('T', [8, 64])
@pytest.mark.parametrize('mode', MODES)
def test_append_ragged_append_and_append_generate_equal_the_linear_session(mode, T):
    cfg, tensors, keys, ids, lens, feed = engine(mode)
    res = side_by_side(append_script(ids, lens, feed), cfg, tensors, keys, T)
    assert res[-5].tolist() == [56, 53]  # sequence_length: 20 + 3 + 1 + 20 + 1 + (5, 2) + 4 + the 3 generated less the pending one


def test_packed_inputs():
    cfg, tensors, keys, ids, lens, feed = engine('fp16-fp16')
    side_by_side(append_script(ids, lens, feed), cfg, tensors, keys, 8, remove_input_padding=1)


# ------------------------------------------------------------------------------------------------ speculative
def greedy_tokens(cfg, tensors, keys, ids, lens, n):
    s = session(cfg, tensors, keys, False, 0)
    s.setup(2, ids.shape[1], NEW)
    out = s.generate(ids, lens, n)
    s.close()
    return out[:, ids.shape[1]:ids.shape[1] + n]


def verify_script(ids, lens, tok, vocab, sampled, exact):
    S, n = ids.shape[1], 6

    def drafts(pending, right, kept):
        f = np.zeros((2, n), np.int32)
        for b in range(2):
            f[b, 0] = pending[b]
            for i in range(1, n):
                f[b, i] = right[b, i] if i <= kept[b] else (right[b, i] + 1) % vocab
        return f

    def run(s):
        out = []
        s.setup(2, S, NEW)
        if sampled:
            s.set_sampling(top_k=8, temperature=0.8, random_seed=7)
        s.context(ids, lens)
        # round 1: the drafts of sequence b are the greedy tokens up to kept[b]; 6 ids at p = 20 write the slots 20 - 25
        f = drafts(s.output_ids()[:, S], tok, (3, 1))
        acc, lp = s.verify(f, sampled=sampled)
        out += [acc, lp, s.logits(), s.verify_draws(n) if sampled else s.verify_top1(n)] + state(s)
        if exact:  # (fp16, greedy: the margins of the synthetic model are far above the arithmetic of a pass)
            assert acc.tolist() == [3, 1]
            # sequence 1: slot 25 (block 3 of T = 8) was written, sequence_length is back at 22 (block 2)
            assert s.step_state()['sequence_length'].tolist() == [24, 22]
        s.step(1)
        out += [s.logits()] + state(s)
        # round 2: every draft wrong - all of it rolled back but the first id
        p = s.step_state()['sequence_length'].copy()
        pend = np.array([s.output_ids()[b, p[b]] for b in range(2)], np.int32)
        acc, lp = s.verify(drafts(pend, np.full((2, n), 3, np.int32), (0, 0)), sampled=sampled)
        out += [acc, lp, s.logits()] + state(s)
        s.step(2, use_graph=True)
        out += [s.logits()] + state(s)
        return out
    return run


@pytest.mark.parametrize('T', [8, 64])
@pytest.mark.parametrize('mode', ['fp16-fp16', 'sq_static-int8'])
@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'sampled'])
def test_verify_with_a_roll_back_across_a_block_boundary_then_step(sampled, mode, T):
    cfg, tensors, keys, ids, lens, _ = engine(mode)
    tok = greedy_tokens(cfg, tensors, keys, ids, lens, 8)
    side_by_side(verify_script(ids, lens, tok, cfg['vocab_size'], sampled, mode == 'fp16-fp16' and not sampled), cfg, tensors, keys, T)


@pytest.mark.parametrize('T', [8, 64])
@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'sampled'])
def test_generate_lookup_gives_the_linear_sessions_tokens_and_pass_counts(sampled, T):
    cfg, tensors, keys, ids, lens, _ = engine('fp16-fp16')
    ids = ids.copy()
    for b in range(2):  # a prompt that repeats itself: there is always an earlier occurrence to draft from
        ids[b, :lens[b]] = np.resize(ids[b, :4], lens[b])

    def run(s):
        s.setup(2, ids.shape[1], NEW)
        if sampled:
            s.set_sampling(top_k=4, temperature=0.7, random_seed=11)
        out, stats = s.generate_lookup(ids, lens, 24, num_draft_tokens=5, max_ngram=3, sampled=sampled)
        assert stats['verify_rounds'] > 0 and stats['drafted'] > 0
        return [out, np.array([stats[k] for k in sorted(stats)])] + state(s)
    side_by_side(run, cfg, tensors, keys, T)


# ------------------------------------------------------------------------------------------------ LoRA
def test_a_qkvo_adapter_on_one_of_the_two_sequences():
    cfg, tensors, keys, ids, lens, feed = engine('fp16-fp16')
    ad = LR.random_adapter(cfg, 77, 8, modules=('q', 'k', 'v', 'o'))

    def run(s):
        s.lora_load(0, ad, 16.0)
        s.setup(2, ids.shape[1], NEW)
        s.lora_select([0, -1])
        s.context(ids, lens)
        out = [s.logits()]
        s.append(feed[:, :20])
        out += [s.logits()] + state(s)
        s.step(1)
        out.append(s.logits())
        p = s.step_state()['sequence_length']
        f = np.stack([np.concatenate([[s.output_ids()[b, p[b]]], feed[b, 20:23]]) for b in range(2)]).astype(np.int32)
        acc, lp = s.verify(f)
        return out + [acc, lp, s.logits()] + state(s)
    res = side_by_side(run, cfg, tensors, keys, 8, lora_max_rank=8, lora_max_adapters=1, lora_target_modules='q,k,v,o')
    base = side_by_side(lambda s: (s.setup(2, ids.shape[1], NEW), s.context(ids, lens), [s.logits()])[2], cfg, tensors, keys, 8)
    assert not np.array_equal(res[0][0], base[0][0]), 'the adapter acts'


# ------------------------------------------------------------------------------------------------ forced steps
def test_the_paged_append_equals_forced_steps_of_the_paged_session_and_the_oracle():
    """test_gpu_session_append.py::test_tiny_model_append_equals_forced_steps_and_the_oracle on paged sessions (T = 4: the prompt
    of 8 ends on a boundary, the second append crosses the one at 16) - same_state between the two routes, TINY_BOUND to the oracle"""
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    NEW_T, H, Dh = 12, 2, 32
    smax = S + NEW_T
    feed = np.random.default_rng(21).integers(3, 128, (B, 3 + 4 + 5)).astype(np.int32)
    ow = {k: w[k].astype(np.float32) for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    ow['layers'] = [{k[len(f'layers.{i}.'):]: w[k].astype(np.float32) for k in w if k.startswith(f'layers.{i}.')} for i in range(2)]
    caches = [np.zeros((B, 2, H, smax, Dh), np.float16) for _ in range(2)]
    O.llama_logits_context(ids, ow, caches, lens, H)
    masked = np.zeros((B, smax), np.int32)
    for b in range(B):
        masked[b, lens[b]:S] = 1
    ref = [O.llama_logits_decode(feed[:, i], ow, caches, [S + i] * B, lens, S, S + i, H, masked) for i in range(feed.shape[1])]
    paged = dict(paged_kv_cache=1, tokens_per_block=4, paged_append=1)
    a, b = tiny_session(w, **paged), tiny_session(w, **paged)
    for s in (a, b):
        s.setup(B, S, NEW_T)
        s.context(ids, lens)
    a.append(feed[:, :3])
    lb = forced_steps(b, feed[:, :3])
    same_state(a, b, S + 3 + 1)
    close(a.logits(), ref[2], TINY_BOUND, tag='paged append 3')
    close(lb[-1], ref[2], TINY_BOUND, tag='paged forced 3')
    la, lb = forced_steps(a, feed[:, 3:7]), forced_steps(b, feed[:, 3:7])
    for i in range(4):
        close(la[i], ref[3 + i], TINY_BOUND, tag=f'paged A step {i}')
        close(lb[i], ref[3 + i], TINY_BOUND, tag=f'paged B step {i}')
    same_state(a, b, S + 7)
    a.append(feed[:, 7:12])
    close(a.logits(), ref[11], TINY_BOUND, tag='paged append 5')
    assert (a.step_state()['sequence_length'] == smax).all()
    np.testing.assert_array_equal(a.output_ids()[:, S:], feed)
    assert a.append_launches() == (2 * 2, 0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the key
def test_the_key_is_refused_on_a_linear_session_and_a_paged_session_without_it_still_refuses():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    with pytest.raises(RuntimeError, match='paged_append'):
        tiny_session(w, paged_append=1)
    s = tiny_session(w, paged_kv_cache=1, tokens_per_block=4)
    s.setup(B, S, 6)
    s.context(ids, lens)
    tok = np.full((B, 2), 5, np.int32)
    with pytest.raises(RuntimeError, match='not built'):
        s.append(tok)
    with pytest.raises(RuntimeError, match='not built'):
        s.verify(tok)
    s.close()
    # beam search stays refused with the key
    s = tiny_session(w, paged_kv_cache=1, tokens_per_block=8, paged_append=1)
    s.setup(B, S, 6, 2)
    s.context(ids, lens)
    with pytest.raises(RuntimeError, match='not built'):
        s.append(tok)
    s.close()


# ------------------------------------------------------------------------------------------------ front-end
def build_tiny_paged_engine(T):
    """tests/test_frontend.py::build_tiny_engine with the paged cache switched on, blocks of T tokens"""
    import os
    import tensorrt_llm
    from tensorrt_llm.models import LLaMAForCausalLM
    from tensorrt_llm.network import net_guard
    from test_frontend import GOLD, hf_state_dict
    from weight import load_from_hf_llama
    t = dict(np.load(os.path.join(GOLD, 'hf_tiny_llama.npz')))
    model = LLaMAForCausalLM(num_layers=2, num_heads=2, hidden_size=64, vocab_size=128, hidden_act='silu',
                             max_position_embeddings=64, dtype='float16', mlp_hidden_size=24, tensor_parallel=1,
                             tensor_parallel_group=[0])
    load_from_hf_llama(model, hf_state_dict(t), 0, 1, 'float16')
    builder = tensorrt_llm.Builder()
    net = builder.create_network()
    net.plugin_config.set_gpt_attention_plugin('float16')
    net.plugin_config.set_gemm_plugin('float16')
    net.plugin_config.enable_paged_kv_cache()
    net.plugin_config.tokens_per_block = T
    with net_guard(net):
        net.set_named_parameters(model.named_parameters())
        model(*model.prepare_inputs(2, 16, 8, True, 1))
    cfg = builder.create_builder_config(name='llama', precision='float16', tensor_parallel=1, num_layers=2, num_heads=2,
                                        hidden_size=64, vocab_size=128, hidden_act='silu', max_position_embeddings=64,
                                        inter_size=24, quant_mode=0, tp_rank=0)
    engine = builder.build_engine(net, cfg)
    assert engine is not None and b'paged_kv_cache=1' in bytes(engine)[:4096] and b'paged_append' not in bytes(engine)[:4096]
    return engine, t


def test_generation_session_on_a_paged_engine_gives_the_linear_engines_results():
    """append, decode_append, verify, decode_lookup and score followed by append through GenerationSession: an engine built with
    the paged cache (blocks of 4 tokens) beside the linear engine of tests/test_frontend.py, everything equal"""
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_frontend import build_tiny_engine
    paged_engine, t = build_tiny_paged_engine(4)
    linear_engine, _, _ = build_tiny_engine(QuantMode(0))
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    r = np.random.default_rng(3)
    user, more = r.integers(3, 128, (B, 4)).astype(np.int32), r.integers(3, 128, (B, 3)).astype(np.int32)
    rep = ids.copy()
    for b in range(B):
        rep[b, :lens[b]] = np.resize(ids[b, :3], lens[b])
    scfg = SamplingConfig(end_id=-1, pad_id=0)
    mc = dict(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64)
    res = []
    for engine, paged in ((linear_engine, False), (paged_engine, True)):
        dec = GenerationSession(ModelConfig(paged_kv_cache=paged, tokens_per_block=4, **mc), engine, Mapping(1, 0))
        dec.setup(B, S, 24)
        out = [dec.decode(ids, lens, scfg, max_new_tokens=6), dec.decode_append(user, scfg, max_new_tokens=4), dec.append(more)]
        p = dec.runtime.step_state()['sequence_length']
        f = np.stack([np.concatenate([[dec.runtime.output_ids()[b, p[b]]], more[b]]) for b in range(B)]).astype(np.int32)
        v = dec.verify(f)
        out += [v['accepted'], v['log_probs'], v['logits'], dec.append(more, np.array([3, 1]))]
        sc = dec.score(ids, lens)
        out += [sc['log_probs'], sc['top1_ids'], dec.append(user)]
        out.append(dec.decode_lookup(rep, lens, scfg, num_draft_tokens=4, max_ngram=2, max_new_tokens=12))
        out.append(np.array([dec.lookup_stats[k] for k in sorted(dec.lookup_stats)]))
        res.append([np.asarray(x) for x in out])
    for i, (a, b) in enumerate(zip(*res)):
        np.testing.assert_array_equal(a, b, err_msg=f'result {i}')
    # the key is the front-end's to add: the same engine through the plain loader refuses an append
    s = NativeSession(engine=bytes(paged_engine))
    s.setup(B, S, 6)
    s.context(ids, lens)
    with pytest.raises(RuntimeError, match='not built'):
        s.append(user)
    s.close()
    with pytest.raises(RuntimeError, match='runtime key'):
        NativeSession(engine=bytes(paged_engine), runtime_keys=dict(tokens_per_block=8))
    with pytest.raises(RuntimeError, match='paged_append'):
        NativeSession(engine=bytes(linear_engine), runtime_keys=dict(paged_append=1))
