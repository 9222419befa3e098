"""GPU tests of tllm_session_score: the log-probability of every prompt token from one prefill.

THE ORACLE FOR EVERY POSITION is one call of the existing oracle on a tiled batch of prefixes: ids = tile(seq, (T, 1)),
lens = 1 ... T, one new token; row t of its context logits is the distribution after seq[:t + 1] (checked on the CPU for fp16,
sq_dyn_pc, sq_static_pc and woq4 with int8 KV against single-prefix runs: agreement to 2e-6).  Log-probabilities come from
those logits in float64 (tensorrt_llm/runtime/scoring_ref.py).

THE BOUND.  |d log-softmax| <= 2 max |d logit|, so the bound is twice the logit bound the project already applies between
engine and oracle for that model and mode: 2 x 2e-2 on the tiny HF model (tests/test_gpu_session.py); on the synthetic and
trained models 2 x (5e-2 if SmoothQuant else 1e-2) x scale on the largest error and 2 x (1e-2 / 2.5e-3) x scale on the mean
(test_quantised_paths_vs_oracle), scale = the largest |logit| of the oracle (at least 1).  top1_ids: the oracle's logit at the
engine's id is within the same bound of the oracle's maximum.  No position is left out."""
import ctypes
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import llama_oracle as O
from oracle import quant_oracle as QO
from tensorrt_llm.runtime import scoring_ref as R
from tensorrt_llm.runtime.native import NativeSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
EX = os.path.join(ROOT, 'trtllm-llama_amd', 'examples', 'llama_quant')
pytestmark = pytest.mark.gpu

TINY_CFG = dict(num_layers=2, num_heads=2, hidden_size=64, inter_size=24, vocab_size=128, max_position_embeddings=64,
                rms_norm_eps=1e-6)
TINY_BOUND = 2 * 2e-2


def load_tiny():
    t = dict(np.load(os.path.join(GOLD, 'hf_tiny_llama.npz')))
    w = {k: t[k] for k in t if k.startswith('layers.') or k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    return t, w


def tiny_session(w, **cfg):
    s = NativeSession(dict(TINY_CFG, quant_mode=0, **cfg))
    for k, v in w.items():
        s.set_tensor(k, v)
    s.finalize()
    return s


@functools.lru_cache(maxsize=4)
def synth_model(seed, L=2, H=4, D=256, I=512, V=512):
    """the generator of tests/test_gpu_session.py (cached; callers do not modify it)"""
    r = np.random.default_rng(seed)
    xav = lambda n, k: r.uniform(-1, 1, (n, k)) * np.sqrt(6.0 / (n + k)) * 2
    w = {'vocab_embedding.weight': r.standard_normal((V, D)) * 0.5, 'ln_f.weight': 1 + 0.1 * r.uniform(-1, 1, D),
         'lm_head.weight': xav(V, D)}
    for i in range(L):
        p = f'layers.{i}.'
        w[p + 'input_layernorm.weight'] = 1 + 0.1 * r.uniform(-1, 1, D)
        w[p + 'post_layernorm.weight'] = 1 + 0.1 * r.uniform(-1, 1, D)
        w[p + 'attention.qkv.weight'] = xav(3 * D, D)
        w[p + 'attention.dense.weight'] = xav(D, D)
        w[p + 'mlp.fc.weight'] = xav(I, D)
        w[p + 'mlp.gate.weight'] = xav(I, D)
        w[p + 'mlp.proj.weight'] = xav(D, I)
    w = {k: v.astype(np.float16) for k, v in w.items()}
    cfg = dict(num_layers=L, num_heads=H, hidden_size=D, inter_size=I, vocab_size=V, max_position_embeddings=128,
               rms_norm_eps=1e-6)
    return cfg, w


def position_logits(context_logits, ids, lens, vocab):
    """[B, S, V] float64: row (b, t), t < lens[b] - 1, from ONE oracle call per sequence on the tiled prefixes of that sequence.
    context_logits(ids [T, n], lens [T]) -> [T, V]."""
    B, S = ids.shape
    z = np.zeros((B, S, vocab))
    for b in range(B):
        n = int(lens[b])
        if n > 1:
            tiled = np.ascontiguousarray(np.tile(ids[b, :n], (n - 1, 1))).astype(np.int32)
            z[b, :n - 1] = context_logits(tiled, np.arange(1, n, dtype=np.int32))
    return z


def tiny_oracle(w):
    ow = {k: w[k].astype(np.float32) for k in ('vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight')}
    ow['layers'] = [{k[len(f'layers.{i}.'):]: w[k].astype(np.float32) for k in w if k.startswith(f'layers.{i}.')} for i in range(2)]

    def run(ids, lens):
        T, n = ids.shape
        caches = [np.zeros((T, 2, 2, n + 1, 32), np.float16) for _ in range(2)]
        return O.llama_logits_context(ids, ow, caches, lens, 2)
    return run


def quant_oracle(qmodel):
    return lambda ids, lens: np.asarray(QO.run_model(qmodel, ids, lens, 1)[0][0], np.float64)


def check_scores(lp, top, z, ids, lens, bound_max, bound_mean=None, tag=''):
    """engine scores against the oracle's position logits z [B, S, V]: values, the places that are 0 / -1 by definition, top1"""
    B, S = ids.shape
    lp0, top0 = R.sequence_scores(z, ids, lens)
    scored = np.zeros((B, S), bool)
    for b in range(B):
        scored[b, 1:int(lens[b])] = True
    assert lp.shape == (B, S) and top.shape == (B, S) and lp.dtype == np.float32 and top.dtype == np.int32
    assert (lp[~scored] == 0).all() and (top[~scored] == -1).all(), f'{tag}: 0 / -1 exactly where there is nothing to score'
    assert np.isfinite(lp).all() and (lp[scored] < 0).all() and (top[scored] >= 0).all() and (top[scored] < z.shape[2]).all()
    d = np.abs(lp.astype(np.float64) - lp0)[scored]
    print(f'[score {tag}] {int(scored.sum())} positions: max |d log_prob| {d.max():.3e} (bound {bound_max:.3e}), mean {d.mean():.3e}'
          + (f' (bound {bound_mean:.3e})' if bound_mean else ''))
    assert d.max() <= bound_max, f'{tag}: log_probs off by {d.max():.3e} > {bound_max:.3e}'
    if bound_mean is not None:
        assert d.mean() <= bound_mean, f'{tag}: mean |d log_prob| {d.mean():.3e} > {bound_mean:.3e}'
    # the distribution of token t is row t - 1
    for b in range(B):
        for t in range(1, int(lens[b])):
            row = z[b, t - 1]
            assert row.max() - row[top[b, t]] <= bound_max, f'{tag}: top1[{b}][{t}] = {top[b, t]} is {row.max() - row[top[b, t]]:.3e} below the oracle\'s maximum'
    return lp0, top0


def synth_case(mode, int8_kv, B, S, lens, seed=5):
    cfg, w = synth_model(11)
    r = np.random.default_rng(seed)
    ids = r.integers(3, cfg['vocab_size'], (B, S)).astype(np.int32)
    lens = np.array(lens, np.int32)
    for b in range(B):
        ids[b, lens[b]:] = 2
    qmodel = QO.quantise_model(cfg, w, mode, int8_kv, calib_ids=ids, calib_lens=lens)
    return cfg, qmodel, ids, lens


def quant_session(cfg, qmodel, **keys):
    s = NativeSession(dict(cfg, quant_mode=qmodel['quant_mode'], **keys))
    for k, v in qmodel['engine_tensors'].items():
        s.set_tensor(k, v)
    s.finalize()
    return s


def synth_bounds(mode, z):
    scale = max(np.abs(z).max(), 1.0)
    sq = mode.startswith('sq')
    return 2 * (5e-2 if sq else 1e-2) * scale, 2 * (1e-2 if sq else 2.5e-3) * scale


def kv_bytes(s, layers, nbytes):
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = []
    for li in range(layers):
        host = np.empty(nbytes, np.uint8)
        assert hip.hipMemcpy(host.ctypes.data, s.kv_cache_ptr(li), nbytes, 2) == 0
        out.append(host)
    return out


# ------------------------------------------------------------------------------------------------ (a) tiny HF model
def test_tiny_model_scores_and_leaves_the_session_as_context_does():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    assert B == 2 and S == 8 and len(set(lens.tolist())) == 2  # ragged
    NEW = 4
    a, b = tiny_session(w), tiny_session(w)
    a.setup(B, S, NEW)
    b.setup(B, S, NEW)
    lp, top = a.score(ids, lens)
    b.context(ids, lens)
    z = position_logits(tiny_oracle(w), ids, lens, 128)
    check_scores(lp, top, z, ids, lens, TINY_BOUND, tag='tiny fp16')
    # a second call on the same session: same bits (buffers reused)
    lp2, top2 = a.score(ids, lens)
    assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(top, top2)

    def same_state():
        assert np.array_equal(a.logits().view(np.uint32), b.logits().view(np.uint32))
        assert np.array_equal(a.output_ids(), b.output_ids())
        sa, sb = a.step_state(), b.step_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
        n = B * 2 * 2 * (S + NEW) * 32 * 2
        for x, y in zip(kv_bytes(a, 2, n), kv_bytes(b, 2, n)):
            assert np.array_equal(x, y)
    same_state()
    a.step(2)
    b.step(2)
    same_state()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ (b) quantisation modes
@pytest.mark.parametrize('mode', ['woq8', 'woq4', 'sq_static_pc', 'sq_dyn_pc'])
@pytest.mark.parametrize('int8_kv', [0, 1])
def test_quantised_modes_vs_oracle(mode, int8_kv):
    cfg, qmodel, ids, lens = synth_case(mode, int8_kv, 2, 12, (12, 7))
    s = quant_session(cfg, qmodel)
    s.setup(2, 12, 2)
    lp, top = s.score(ids, lens)
    s.close()
    z = position_logits(quant_oracle(qmodel), ids, lens, cfg['vocab_size'])
    bmax, bmean = synth_bounds(mode, z)
    check_scores(lp, top, z, ids, lens, bmax, bmean, tag=f'{mode} kv8={int8_kv}')


# ------------------------------------------------------------------------------------------------ (c) head GEMM regimes, chunk seams
@pytest.mark.parametrize('mode', ['fp16', 'sq_static_pc'])
def test_head_gemm_regimes_and_chunk_seams(mode):
    """39 rows through the MFMA GEMM, 5 rows through the skinny one, and 39 rows in chunks of 16 (16 + 16 + 7: a ragged tail that
    takes the skinny path): the chunked run scores every row once, in its place."""
    got = {}
    for name, S, keys in (('mfma', 40, {}), ('skinny', 6, {}), ('chunks', 40, dict(score_chunk_rows=16))):
        cfg, qmodel, ids, lens = synth_case(mode, 0, 1, S, (S, ), seed=9)
        s = quant_session(cfg, qmodel, **keys)
        s.setup(1, S, 2)
        lp, top = s.score(ids, lens)
        s.close()
        z = position_logits(quant_oracle(qmodel), ids, lens, cfg['vocab_size'])
        bmax, bmean = synth_bounds(mode, z)
        check_scores(lp, top, z, ids, lens, bmax, bmean, tag=f'{mode} {name}')
        got[name] = (lp, top)
    # same prompt, same model: the seams move rows between GEMM kernels, not between positions
    bmax, _ = synth_bounds(mode, z)
    assert np.abs(got['mfma'][0] - got['chunks'][0]).max() <= bmax


# ------------------------------------------------------------------------------------------------ (d) packed inputs, paged cache
@pytest.mark.parametrize('mode', ['fp16', 'sq_static_pc'])
def test_packed_inputs_and_paged_cache(mode):
    cfg, qmodel, ids, lens = synth_case(mode, 0, 2, 12, (12, 7))
    z = position_logits(quant_oracle(qmodel), ids, lens, cfg['vocab_size'])
    bmax, bmean = synth_bounds(mode, z)
    for keys in (dict(remove_input_padding=1), dict(paged_kv_cache=1, tokens_per_block=16),
                 dict(remove_input_padding=1, paged_kv_cache=1, tokens_per_block=16)):
        s = quant_session(cfg, qmodel, **keys)
        s.setup(2, 12, 2)
        lp, top = s.score(ids, lens)
        s.step(1)  # generation continues from it
        s.close()
        check_scores(lp, top, z, ids, lens, bmax, bmean, tag=f'{mode} {keys}')


# ------------------------------------------------------------------------------------------------ (e) records through the 1-rank all-gather
def test_force_comm_is_bit_identical():
    from tensorrt_llm.plugin import capi
    lib = capi.load_library()
    uid = (ctypes.c_char * 128)()
    assert lib.tllm_comm_get_unique_id(uid) == 0, capi.last_error()
    assert lib.tllm_comm_init_rank((ctypes.c_int32 * 1)(0), 1, 0, uid) == 0, capi.last_error()
    try:
        t, w = load_tiny()
        ids, lens = t['ids'], t['input_lengths']
        B, S = ids.shape
        got = []
        for cfg in ({}, dict(force_comm=1)):
            s = tiny_session(w, **cfg)
            s.setup(B, S, 2)
            got.append(s.score(ids, lens))
            s.close()
        assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
        assert np.array_equal(got[0][1], got[1][1])
    finally:
        assert lib.tllm_comm_destroy_all() == 0


# ------------------------------------------------------------------------------------------------ (f) two ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, 'trtllm-llama_amd'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from tensorrt_llm.plugin import capi
    import test_tp_session_p2p as T
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        lib = capi.load_library()
        lib.tllm_comm_p2p_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]
        lib.tllm_comm_p2p_attach.argtypes = [ctypes.c_void_p]
        lib.tllm_comm_p2p_enable.argtypes = [ctypes.c_int32]
        lib.tllm_comm_p2p_enable.restype = None
        T._p2p_up(lib, capi, torch, dist, ctypes, world, rank)
        CFG, t, ids, lens = T.model()
        B, S = ids.shape
        s = NativeSession(dict(CFG, quant_mode=0, tp_size=world, tp_rank=rank))
        for k, v in T.shard(t, world, rank).items():
            s.set_tensor(k, v)
        s.finalize()
        s.setup(B, S, 2)
        lp, top = s.score(ids, lens)
        s.step(1)
        s.close()
        q.put((rank, lp, top, int(lib.tllm_comm_p2p_error())))
        dist.barrier()
        lib.tllm_comm_destroy_all()
    except BaseException as e:  # the parent must not wait for a result that will never come
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_identical_scores_within_the_bound_of_the_unsharded_oracle():
    import torch.multiprocessing as mp
    import test_tp_session_p2p as T
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    assert all(len(r) == 4 for r in res), [r for r in res if len(r) != 4]
    res = sorted(res, key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][3] == 0 and res[1][3] == 0, 'a peer-to-peer wait timed out'
    assert np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32)) and np.array_equal(res[0][2], res[1][2])
    cfg, w, ids, lens = T.model()
    qmodel = QO.quantise_model(cfg, w, 'fp16', 0, calib_ids=ids, calib_lens=lens)
    z = position_logits(quant_oracle(qmodel), ids, lens, cfg['vocab_size'])
    bmax, bmean = synth_bounds('fp16', z)
    check_scores(res[0][1], res[0][2], z, ids, lens, bmax, bmean, tag='tp2 fp16')


# ------------------------------------------------------------------------------------------------ (g) errors
def test_errors_and_the_sequence_of_one_token():
    t, w = load_tiny()
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    s = tiny_session(w)
    s.batch, s.max_in, s.max_new, s.beam = B, S, 2, 1  # the Python side's shape checks pass; the library has seen no setup
    with pytest.raises(RuntimeError, match='tllm_session_setup first'):
        s.score(ids, lens)
    s.setup(B, S, 2, beam_width=2)
    with pytest.raises(RuntimeError, match='beam_width 1'):
        s.score(ids, lens)
    s.setup(B, S, 2)
    with pytest.raises(RuntimeError, match='out of range'):
        s.score(ids, np.array([0, 5], np.int32))
    with pytest.raises(RuntimeError, match='out of range'):
        s.score(ids, np.array([S + 1, 5], np.int32))
    lp, top = s.score(ids, np.array([1, 5], np.int32))  # a length of 1: nothing to score, not an error
    assert (lp[0] == 0).all() and (top[0] == -1).all() and (lp[1, 1:5] < 0).all() and (lp[1, 5:] == 0).all()
    lp, top = s.score(ids, np.array([1, 1], np.int32))
    assert (lp == 0).all() and (top == -1).all()
    s.close()


# ------------------------------------------------------------------------------------------------ (h) trained stochastic parent
@functools.lru_cache(maxsize=1)
def _trained_prompts():
    import trained_parents as TP
    e = TP.load_eval('stochastic')
    rows = []
    for b in range(2):
        n = int(e['lengths'][b])
        rows.append(np.concatenate([e['prompts'][b, :n], e['reference'][b]])[-64:].astype(np.int32))
    return np.stack(rows), np.array([64, 64], np.int32)


_ppl = {}


@pytest.mark.parametrize('mode', ['fp16', 'sq_static_int8kv', 'woq4_int8kv'])
def test_trained_stochastic_parent(mode):
    import trained_parents as TP
    ids, lens = _trained_prompts()
    cfg, qmodel = TP.quantised('stochastic', mode)
    s = quant_session(cfg, qmodel)
    s.setup(2, 64, 2)
    lp, top = s.score(ids, lens)
    s.close()
    z = position_logits(quant_oracle(qmodel), ids, lens, cfg['vocab_size'])
    bmax, bmean = synth_bounds(mode, z)
    lp0, _ = check_scores(lp, top, z, ids, lens, bmax, bmean, tag=f'trained {mode}')
    _ppl[mode] = R.perplexity(lp, lens)
    print(f'[score trained {mode}] perplexity {_ppl[mode]:.4f} (oracle {R.perplexity(lp0, lens):.4f}'
          + (f', fp16 engine {_ppl["fp16"]:.4f})' if 'fp16' in _ppl else ')'))


# ------------------------------------------------------------------------------------------------ (i) front-end
def test_generation_session_score_equals_the_native_session():
    import torch
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig
    from test_frontend import build_tiny_engine
    engine, _, t = build_tiny_engine(QuantMode(0))
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    dec.setup(B, S, 4)
    out = dec.score(ids, lens)
    _, w = load_tiny()
    s = tiny_session(w)
    s.setup(B, S, 4)
    lp, top = s.score(ids, lens)
    s.close()
    assert np.array_equal(out['log_probs'].view(np.uint32), lp.view(np.uint32)) and np.array_equal(out['top1_ids'], top)
    want = [R.perplexity(lp[b], lens[b:b + 1]) for b in range(B)]
    assert out['perplexity'].shape == (B, ) and np.allclose(out['perplexity'], want, rtol=1e-6)
    tout = dec.score(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda())
    for k in ('log_probs', 'top1_ids', 'perplexity'):
        assert tout[k].is_cuda and np.array_equal(tout[k].cpu().numpy(), out[k])


def test_summarize_eval_ppl_engine_vs_hf(tmp_path):
    """hf_llama_convert -> build (fp16) -> summarize.py --eval_ppl --test_hf --test_trt_llm, as test_summarize_engine_vs_hf runs it:
    both perplexities reported, |mean NLL(engine) - mean NLL(HF)| <= 2e-1, twice the reference's fp16 logit tolerance of 1e-1."""
    import test_convert as T
    _, hf_dir = T.tiny_hf(tmp_path)
    ft = tmp_path / 'ft'
    subprocess.run([sys.executable, os.path.join(EX, 'hf_llama_convert.py'), '-i', hf_dir, '-o', str(ft), '-sq', '0.5',
                    '--calibrate-kv-cache', '--calib-samples', '8', '--calib-len', '64'], check=True, cwd=EX, timeout=600)
    eng = tmp_path / 'eng'
    subprocess.run([sys.executable, os.path.join(EX, 'build.py'), '--model_dir', str(ft / '1-gpu'), '--output_dir', str(eng),
                    '--max_batch_size', '2', '--max_input_len', '64', '--max_output_len', '16', '--log_level', 'error'],
                   check=True, cwd=EX, timeout=600)
    out = tmp_path / 'ppl.json'
    subprocess.run([sys.executable, os.path.join(EX, 'summarize.py'), '--hf_model_location', hf_dir, '--test_hf',
                    '--test_trt_llm', '--engine_dir', str(eng), '--synthetic', '--synthetic_len', '40', '--output_len', '12',
                    '--batch_size', '2', '--max_ite', '4', '--log_level', 'error', '--output_json', str(out), '--eval_ppl'],
                   check=True, cwd=EX, timeout=900)
    r = json.load(open(out))
    print(f"[summarize --eval_ppl] engine {r['tensorrt_llm_perplexity']:.4f}, HF {r['hf_perplexity']:.4f}, "
          f"mean NLL delta {r['mean_nll_delta']:.3e}")
    assert r['tensorrt_llm_perplexity'] > 1 and r['hf_perplexity'] > 1
    assert abs(r['mean_nll_delta']) <= 2e-1, r
    assert 'token_match_rate' in r  # the rest of the report is still there
