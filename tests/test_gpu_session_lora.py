"""LoRA adapters per sequence in the session: prefill, generation step (eager and from the graph), append,
ragged append and score under adapters, against quant_oracle with lora_ref.wrap_oracle_linear in its linears.

The inputs are those whose headroom tests/test_lora_ref.py::test_headroom_of_the_gpu_session_cases asserts: synth_model(11), prompts
12 / 7 of 20 (seed 5), adapter seed 77, r = 8, alpha = 16, all seven modules - the adapter moves the logits by more than 10 x
synth_bounds' max bound, so a session that ignores, swaps or mis-routes a selection cannot stay within one bound."""
import numpy as np
import pytest

from oracle import quant_oracle as QO
from tensorrt_llm.runtime import gqa_ref as G
from tensorrt_llm.runtime import lora_ref as LR
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_score import check_scores, position_logits, quant_session, synth_bounds
from test_gpu_session_append import ONE_BYTE_INPUTS, close, synth_inputs

pytestmark = pytest.mark.gpu
RANK, ALPHA, SEED = 8, 16.0, 77
ALL = 'q,k,v,o,gate,up,down'
STEPS = 3
KEYS = dict(lora_max_rank=RANK, lora_max_adapters=2, lora_target_modules=ALL)


def adapter(cfg, seed=SEED, r=RANK, **kw):
    return LR.random_adapter(cfg, seed, r, **kw)


def oracle_run(model, ids, lens, feed, n):
    """context logits + the logits after n teacher-forced steps"""
    return QO._forward(model, ids, lens, 1 + n, feed_ids=feed)[0]


def forced(s, feed, n, use_graph=True):
    out = []
    for i in range(n):
        s.force_tokens(feed[:, i])
        s.step(1, use_graph=use_graph)
        out.append(s.logits())
    return out


def within(got, ref, mode, tag):
    for i, (g, z) in enumerate(zip(got, ref)):
        bmax, bmean = synth_bounds(mode, z)
        close(g, z, bmax, bmean, tag=f'{tag} {"context" if i == 0 else f"step {i}"}')


# ------------------------------------------------------------------------------------------------ oracle cases
@pytest.mark.parametrize('mode,cache', [('fp16', 'fp16'), ('woq8', 'int8'), ('woq4', 'fp16')], ids=['fp16', 'woq8-int8', 'woq4'])
def test_all_seven_modules_against_the_wrapped_oracle(mode, cache):
    cfg, w, ids, lens, feed = synth_inputs(**(ONE_BYTE_INPUTS if cache == 'int8' else {}))
    qmodel = QO.quantise_model(cfg, w, mode, 1 if cache == 'int8' else 0, calib_ids=ids, calib_lens=lens)
    ad, s_a = adapter(cfg), LR.scale(ALPHA, RANK)
    ref = oracle_run(LR.adapt_oracle(qmodel['oracle'], cfg, [(ad, s_a)], RANK), ids, lens, feed, STEPS)
    s = quant_session(cfg, qmodel, **KEYS)
    s.lora_load(0, ad, ALPHA)
    s.setup(2, ids.shape[1], STEPS + 1)
    s.lora_select([0, 0])
    s.context(ids, lens)
    got = [s.logits()] + forced(s, feed, STEPS)
    assert s.decode_form() == 0  # the separate-launch step: neither one-launch form
    s.close()
    within(got, ref, mode, f'{mode} {cache}')


# ------------------------------------------------------------------------------------------------ selection cases
@pytest.fixture(scope='module')
def fp16_case():
    cfg, w, ids, lens, feed = synth_inputs()
    qmodel = QO.quantise_model(cfg, w, 'fp16', 0, calib_ids=ids, calib_lens=lens)
    a0, a1 = adapter(cfg), adapter(cfg, seed=78, r=RANK)
    s0, s1 = LR.scale(ALPHA, RANK), LR.scale(ALPHA, RANK, use_rslora=True)
    base = qmodel['oracle']
    run = lambda per: oracle_run(LR.adapt_oracle(base, cfg, per, RANK), ids, lens, feed, STEPS)
    refs = dict(base=oracle_run(base, ids, lens, feed, STEPS), a0=run([(a0, s0)]), a1=run([(a1, s1)]),
                a0_none=run([(a0, s0), None]), a0_a1=run([(a0, s0), (a1, s1)]))
    return dict(cfg=cfg, qmodel=qmodel, ids=ids, lens=lens, feed=feed, a0=a0, a1=a1, refs=refs)


def loaded_session(c, **keys):
    s = quant_session(c['cfg'], c['qmodel'], **dict(KEYS, **keys))
    s.lora_load(0, c['a0'], ALPHA)
    s.lora_load(1, c['a1'], ALPHA, use_rslora=True)
    return s


def run_selected(c, slots, **keys):
    s = loaded_session(c, **keys)
    s.setup(2, c['ids'].shape[1], STEPS + 1)
    s.lora_select(slots)
    s.context(c['ids'], c['lens'])
    got = [s.logits()] + forced(s, c['feed'], STEPS)
    s.close()
    return got


def test_one_sequence_on_an_adapter_and_one_on_none(fp16_case):
    c = fp16_case
    got = run_selected(c, [0, -1])
    within(got, c['refs']['a0_none'], 'fp16', 'slots 0 / -1')
    # per sequence: sequence 1 is the base model's, sequence 0 the adapted one's - and the two oracles are 10 bounds apart
    for i, g in enumerate(got):
        bmax, _ = synth_bounds('fp16', c['refs']['base'][i])
        close(g[1:], c['refs']['base'][i][1:], bmax, tag=f'sequence 1 against the base oracle, stage {i}')
        close(g[:1], c['refs']['a0'][i][:1], bmax, tag=f'sequence 0 against the adapted oracle, stage {i}')
        assert np.abs(c['refs']['a0'][i].astype(np.float64) - c['refs']['base'][i]).max(axis=1).min() >= 10 * bmax


def test_two_different_adapters_on_the_two_sequences(fp16_case):
    c = fp16_case
    within(run_selected(c, [0, 1]), c['refs']['a0_a1'], 'fp16', 'slots 0 / 1')
    # (rsLoRA scale on slot 1: alpha / sqrt(r) is what the oracle of a1 used)
    bmax, _ = synth_bounds('fp16', c['refs']['a0_a1'][0])
    assert np.abs(c['refs']['a0_a1'][0].astype(np.float64) - c['refs']['a0'][0])[1].max() >= 10 * bmax


def test_all_minus_one_is_the_base_model(fp16_case):
    c = fp16_case
    within(run_selected(c, [-1, -1]), c['refs']['base'], 'fp16', 'slots -1 / -1')


def test_select_between_two_replays_of_one_graph_switches_the_function(fp16_case):
    """the same captured step, replayed from the same state under three selections: each time the logits of that selection's
    oracle.  The state is rebuilt by context() (which captures nothing); the graph is captured once, by the first step - the
    session's capture counter (tllm_session_graph_captures) says so after every select, commit and clear."""
    c = fp16_case
    s = loaded_session(c)
    s.setup(2, c['ids'].shape[1], STEPS + 1)
    got = {}
    for name, slots in (('a0', [0, 0]), ('base', [-1, -1]), ('a0_a1', [0, 1])):
        s.lora_select([-1, -1])
        s.context(c['ids'], c['lens'])  # the same cache every time: the prompt under no adapter
        s.lora_select(slots)
        s.force_tokens(c['feed'][:, 0])
        s.step(1, use_graph=True)
        got[name] = s.logits()
        assert s.graph_captures() == 1
    # eager under the last selection: the replay's bits
    s.lora_select([-1, -1])
    s.context(c['ids'], c['lens'])
    s.lora_select([0, 1])
    s.force_tokens(c['feed'][:, 0])
    s.step(1, use_graph=False)
    np.testing.assert_array_equal(s.logits().view(np.uint32), got['a0_a1'].view(np.uint32))
    # commit and clear under the live graph: slot 1 becomes a0 - the function follows, no re-capture
    s.lora_load(1, c['a0'], ALPHA)
    s.lora_select([-1, -1])
    s.context(c['ids'], c['lens'])
    s.lora_select([1, 1])
    s.force_tokens(c['feed'][:, 0])
    s.step(1, use_graph=True)
    np.testing.assert_array_equal(s.logits().view(np.uint32), got['a0'].view(np.uint32))
    s.lora_clear(0)  # sequences on slot 0 would fall back to none; nobody is on it
    s.step(1, use_graph=True)
    assert s.graph_captures() == 1  # three selects, a commit and a clear later: still the first capture
    s.close()
    # the step alone under an adapter, on a prompt cache of the base model: the oracle of exactly that
    cfg, ids, lens, feed = c['cfg'], c['ids'], c['lens'], c['feed']
    base = c['qmodel']['oracle']
    for name, per in (('a0', [(c['a0'], LR.scale(ALPHA, RANK))]), ('base', None),
                      ('a0_a1', [(c['a0'], LR.scale(ALPHA, RANK)), (c['a1'], LR.scale(ALPHA, RANK, use_rslora=True))])):
        taps = {}
        QO._forward(base, ids, lens, 1, taps=taps)
        model = base if per is None else LR.adapt_oracle(base, cfg, per, RANK)
        S = ids.shape[1]
        caches = [np.concatenate([k, np.zeros(k.shape[:3] + (1, k.shape[4]), k.dtype)], axis=3) for k in taps['caches_after_context']]
        z = QO._forward(model, ids, lens, 2, feed_ids=feed, start_caches=caches)[0][1]
        bmax, bmean = synth_bounds('fp16', z)
        close(got[name], z, bmax, bmean, tag=f'graph replay under {name}')


# ------------------------------------------------------------------------------------------------ append, score
def teacher_forced(c, n):
    return oracle_run(LR.adapt_oracle(c['qmodel']['oracle'], c['cfg'], [(c['a0'], LR.scale(ALPHA, RANK))], RANK), c['ids'], c['lens'],
                      c['feed'], n)


def test_append_of_20_tokens_under_an_adapter(fp16_case):
    c = fp16_case
    n = 20
    ref = teacher_forced(c, n + 1)
    s = loaded_session(c)
    s.setup(2, c['ids'].shape[1], n + 2)
    s.lora_select([0, 0])
    s.context(c['ids'], c['lens'])
    s.append(c['feed'][:, :n])
    got = s.logits()
    assert s.append_launches() == (0, c['cfg']['num_layers'])  # the MFMA attention kernel, prefill-regime LoRA rows
    nxt = forced(s, c['feed'][:, n:], 1)[0]
    s.close()
    within([got, nxt], [ref[n], ref[n + 1]], 'fp16', 'append 20 | next')


def test_ragged_append_under_an_adapter(fp16_case):
    c = fp16_case
    lengths = np.array([5, 11], np.int32)
    ref = teacher_forced(c, 11)
    s = loaded_session(c)
    s.setup(2, c['ids'].shape[1], 16)
    s.lora_select([0, 0])
    s.context(c['ids'], c['lens'])
    s.append(c['feed'][:, :11], lengths)
    got = s.logits()
    s.close()
    for b in range(2):
        z = ref[lengths[b]][b:b + 1]
        bmax, bmean = synth_bounds('fp16', z)
        close(got[b:b + 1], z, bmax, bmean, tag=f'ragged append, sequence {b} ({lengths[b]} tokens)')


def test_score_under_an_adapter_against_scoring_ref(fp16_case):
    c = fp16_case
    cfg, ids, lens = c['cfg'], c['ids'], c['lens']
    model = LR.adapt_oracle(c['qmodel']['oracle'], cfg, [(c['a0'], LR.scale(ALPHA, RANK))], RANK)
    z = position_logits(lambda i, l: np.asarray(QO._forward(model, i, l, 1)[0][0], np.float64), ids, lens, cfg['vocab_size'])
    s = loaded_session(c)
    s.setup(2, ids.shape[1], 2)
    s.lora_select([0, 0])
    lp, top = s.score(ids, lens)
    s.close()
    bmax, bmean = synth_bounds('fp16', z)
    check_scores(lp, top, z, ids, lens, bmax, bmean, tag='score under an adapter')


# ------------------------------------------------------------------------------------------------ layout cases
def greedy(c, ids, lens, slots, n=4, **keys):
    s = loaded_session(c, **keys)
    s.setup(ids.shape[0], ids.shape[1], n + 1)
    s.lora_select(slots)
    s.context(ids, lens)
    l0 = s.logits()
    s.step(n, use_graph=True)
    out, l1 = s.output_ids(), s.logits()
    s.close()
    return out, l0, l1


def test_packed_inputs_and_the_paged_cache_equal_the_padded_linear_session(fp16_case):
    """the prompts of tests/test_gpu_session.py::test_packed_context_equals_padded - 40 / 7 / 23 / 33 of 40, 103 packed rows: both
    layouts run the prefill GEMMs of 32 rows and more, whose rows do not depend on how many there are - under two adapters and
    none: logits after the prompt, logits after 4 steps and the token record, bit for bit.  The LoRA launches sum every row in the
    same order whatever the row count and whatever else shares its tile."""
    c = fp16_case
    r = np.random.default_rng(19)
    lens = np.array([40, 7, 23, 33], np.int32)
    ids = np.full((4, 40), 2, np.int32)
    for b in range(4):
        ids[b, :lens[b]] = r.integers(3, c['cfg']['vocab_size'], lens[b])
    slots = [0, 1, -1, 0]
    want = greedy(c, ids, lens, slots)
    base = greedy(c, ids, lens, [-1] * 4)
    assert not np.array_equal(want[1][0], base[1][0]) and np.array_equal(want[1][2], base[1][2])  # the adapters act, row 2 has none
    for name, keys in (('paged', dict(paged_kv_cache=1, tokens_per_block=16)), ('packed', dict(remove_input_padding=1))):
        got = greedy(c, ids, lens, slots, **keys)
        np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=f'{name}: logits after the prompt')
        np.testing.assert_array_equal(got[2].view(np.uint32), want[2].view(np.uint32), err_msg=f'{name}: logits after 4 steps')
        np.testing.assert_array_equal(got[0], want[0], err_msg=f'{name}: token record')


def test_grouped_heads_within_the_replicated_sessions_error():
    """num_kv_heads 2 of 4: the grouped session (folded QKV weight, k / v adapters of Hkv * Dh rows) against the multi-head oracle
    whose weights AND adapter rows are the replicated ones, within 1.25 x the error of the replicated multi-head session under the
    replicated adapter (the form of tests/test_gpu_gqa_session.py) and within the bound"""
    cfg, w, ids, lens, feed = synth_inputs()
    H, Hkv, Dh = 4, 2, 64
    wg, wm = dict(w), dict(w)
    ag = adapter(cfg, num_kv_heads=Hkv)
    am = dict(ag)
    for i in range(cfg['num_layers']):
        k = f'layers.{i}.attention.qkv.weight'
        wg[k] = np.ascontiguousarray(G.fold_qkv(w[k].T, H, Hkv, Dh).T)
        wm[k] = np.ascontiguousarray(G.expand_qkv_weight(wg[k], H, Hkv, Dh))
        for m in ('k', 'v'):  # rows of B repeated like the weight's rows; A is shared
            n = f'layers.{i}.attention.{m}.lora_b'
            am[n] = np.ascontiguousarray(np.repeat(ag[n].reshape(Hkv, Dh, RANK), H // Hkv, axis=0).reshape(H * Dh, RANK))
    s_a = LR.scale(ALPHA, RANK)
    ref = oracle_run(LR.adapt_oracle(QO._fp16_model(cfg, wm), cfg, [(am, s_a)], RANK), ids, lens, feed, STEPS)
    err = {}
    for kind, ww, ad, extra in (('gqa', wg, ag, dict(num_kv_heads=Hkv)), ('mha', wm, am, {})):
        s = NativeSession(dict(cfg, quant_mode=0, **dict(KEYS, **extra)))
        for k, v in ww.items():
            s.set_tensor(k, v)
        s.finalize()
        s.lora_load(0, ad, ALPHA)
        s.setup(2, ids.shape[1], STEPS + 1)
        s.lora_select([0, 0])
        s.context(ids, lens)
        got = [s.logits()] + forced(s, feed, STEPS)
        s.close()
        if kind == 'gqa':
            within(got, ref, 'fp16', 'grouped heads')
        err[kind] = [np.abs(g.astype(np.float64) - z).max() for g, z in zip(got, ref)]
    print(f'max |logits - oracle|: grouped {err["gqa"]}, replicated {err["mha"]}')
    assert err['gqa'][0] <= 1.25 * err['mha'][0] and max(err['gqa'][1:]) <= 1.25 * max(err['mha'][1:])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_key_and_leave_the_session_usable(fp16_case):
    c = fp16_case
    cfg, ids, lens = c['cfg'], c['ids'], c['lens']
    with pytest.raises(RuntimeError, match='SmoothQuant'):
        NativeSession(dict(cfg, quant_mode=QO.QM['INT8_WEIGHTS'] | QO.QM['ACTIVATIONS'] | QO.QM['PER_CHANNEL'], lora_max_rank=8))
    with pytest.raises(RuntimeError, match='tp_size'):
        NativeSession(dict(cfg, quant_mode=0, tp_size=2, tp_rank=0, lora_max_rank=8))
    s = quant_session(cfg, c['qmodel'], lora_max_rank=RANK, lora_max_adapters=2, lora_target_modules='q,v')
    with pytest.raises(RuntimeError, match='beam_width'):
        s.setup(2, ids.shape[1], 4, beam_width=2)
    s.setup(2, ids.shape[1], 4)
    with pytest.raises(RuntimeError, match='lora_max_rank'):
        s.lora_load(0, adapter(cfg, r=16, modules=('q', 'v')), ALPHA)
    with pytest.raises(RuntimeError, match='lora_target_modules'):
        s.lora_load(0, adapter(cfg, modules=('q', 'v', 'down')), ALPHA)
    with pytest.raises(RuntimeError, match='committed'):
        s.lora_select([0, -1])  # nothing was committed: both loads were refused
    with pytest.raises(RuntimeError, match='slot'):
        s.lora_load(2, adapter(cfg, modules=('q', 'v')), ALPHA)
    # still usable: the base model under the refused selection's default, then a good adapter
    s.context(ids, lens)
    z = c['refs']['base'][0]
    close(s.logits(), z, *synth_bounds('fp16', z), tag='after the refusals: base')
    aqv = adapter(cfg, modules=('q', 'v'))
    s.lora_load(0, aqv, ALPHA)
    s.lora_select([0, 0])
    s.context(ids, lens)
    zq = oracle_run(LR.adapt_oracle(c['qmodel']['oracle'], cfg, [(aqv, LR.scale(ALPHA, RANK))], RANK), ids, lens, c['feed'], 0)[0]
    close(s.logits(), zq, *synth_bounds('fp16', zq), tag='after the refusals: q, v adapter')
    s.lora_clear(0)
    with pytest.raises(RuntimeError, match='committed'):
        s.lora_select([0, 0])
    s.context(ids, lens)  # clear put both sequences back on none
    close(s.logits(), z, *synth_bounds('fp16', z), tag='after clear: base')
    s.close()
