"""GPU tests of the device-side top-k / top-p sampler (csrc/kernels/sampling.hip) against the numpy restatement of its rule
(tensorrt_llm/runtime/sampling_ref.py): the generator bit for bit, every draw inside the restatement's prefix-sum interval,
the distribution of 20000 draws, and the sampler inside the session - eager, graph-replayed, generate(), paged, the one-launch
front, two tensor-parallel ranks - plus the front-end.

The per-draw assertion: the returned id i is among the first k' ids of the restatement's order and
    prefix[i-1] - TOL * S <= target <= prefix[i] + TOL * S
with the restatement's fp64 prefix sums; where the configuration leaves one possible id, that id exactly.

TOL.  Device and host differ in the weights only: y - y_max is rounded to fp32 on the device (2^-21 relative, i.e. 2^-20 = 9.5e-7
absolute on the exponent for every id within 16 of the maximum - ids further away weigh below 1.2e-7 of it), expf adds 1 - 2 ulp
(1.2e-7 - 2.4e-7), the fixed point truncates 2^-40 per id (3e-8 of S at vocab 32000).  A prefix sum and S are therefore each off by
at most about 1e-6 of S.  Measured on an MI355X over every draw of this file (855 kernel-level draws: 5 vocabulary layouts x
19 configurations x 9 rows, the 2 x 20 000 draws of the distribution row, the session steps; profiles/sampling_kernel.txt): the largest
excess is 0 - no target fell within the device's error of an interval end - so "4 x measured" gives no scale and the bar is 4 x the
1e-6 derived above instead: TOL = 4e-6, a factor 25 below the 1e-4 from which a neighbouring id of noticeable probability would
pass."""
import os
import socket
import sys

import numpy as np
import pytest

from tensorrt_llm.runtime import sampling_ref as R
from tensorrt_llm.runtime.native import NativeSession, sample_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MEASURED_EXCESS = 0.0  # largest excess seen on an MI355X (share of S); see the module docstring
TOL = 4e-6
assert TOL <= 1e-4

_worst = [0.0]


def check_draw(d: R.Draw, token: int, tag):
    """the assertion of the module docstring for one draw; returns the excess"""
    i, lo, hi = d.interval(token)
    assert i >= 0, f'{tag}: id {token} is not among the first {len(d.cand)} candidates'
    if d.unique():
        assert token == d.token, f'{tag}: the only possible id is {d.token}, got {token}'
    ex = d.excess(token)
    if ex > _worst[0]:
        _worst[0] = ex
        print(f'[sampling] largest excess so far {ex:.3e} of S ({tag})')
    assert ex <= TOL, f'{tag}: target {d.target!r} outside [{lo!r}, {hi!r}] by {ex:.3e} of S = {d.total!r} (id {token}, ' \
                      f'restatement {d.token})'
    return ex


def run_kernel(x, cfg: dict, g, end_id=-1, history=None, in_len=None, max_in=0, nparts=1, want_u=False):
    """x [rows, V] fp32 host -> ids [rows] (and u [rows]) from tllm_sample_tokens; nparts > 1: the rows are laid out as the
    all-gather of vocabulary shards leaves them, [nparts, rows, ceil(V / nparts)], the padding ids holding LARGE logits"""
    import torch
    rows, V = x.shape
    vp = -(-V // nparts)
    full = np.full((rows, nparts * vp), 1e30, np.float32)
    full[:, :V] = x
    dev = torch.from_numpy(np.ascontiguousarray(full.reshape(rows, nparts, vp).transpose(1, 0, 2))).cuda()
    t32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    out = torch.full((rows, ), -7, dtype=torch.int32, device='cuda')
    u = torch.zeros(rows, dtype=torch.float32, device='cuda') if want_u else None
    before = dev.clone()
    sample_tokens(dev, t32(g), out, vocab=V, end_id=end_id, history=t32(history), input_lengths=t32(in_len), max_input_len=max_in,
                  u_out=u, **cfg)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), dev.view(torch.int32)), 'the sampler must not modify the logits'
    return (out.cpu().numpy(), u.cpu().numpy()) if want_u else out.cpu().numpy()


def test_device_generator_equals_the_restatement_bit_for_bit():
    x = np.zeros((64, 16), np.float32)
    for seed in (0, 1, 0xdeadbeefcafef00d, 2**64 - 1):
        g = (np.arange(64, dtype=np.int64) * 37 % 1000 + 1).astype(np.int32)
        g[:4] = [1, 2, 2**20, 2**31 - 2]
        _, u = run_kernel(x, dict(top_k=4, random_seed=seed), g, want_u=True)
        want = np.array([R.uniform(seed, b, int(g[b])) for b in range(64)], np.float32)
        np.testing.assert_array_equal(u.view(np.uint32), want.view(np.uint32))
        assert (u > 0).all() and (u <= 1).all()


def logits_rows(r, rows, V, scale):
    return (r.standard_normal((rows, V)) * scale).astype(np.float32)


# top-k only, top-p only, both, temperatures, each penalty, min_length
CONFIGS = [dict(top_k=1, repetition_penalty=1.3), dict(top_k=1, min_length=5), dict(top_k=2), dict(top_k=50), dict(top_k=1024),
           dict(top_k=0, top_p=0.1), dict(top_k=0, top_p=0.9), dict(top_k=0, top_p=1.0), dict(top_k=40, top_p=0.9),
           dict(top_k=50, temperature=0.5), dict(top_k=0, top_p=0.9, temperature=0.8), dict(top_k=50, temperature=2.0),
           dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1), dict(top_k=50, presence_penalty=1.5),
           dict(top_k=0, top_p=0.95, repetition_penalty=0.7), dict(top_k=8, min_length=5), dict(top_k=0, top_p=0.0),
           dict(top_k=3, top_p=0.0), dict(top_k=5000, top_p=2.0)]
SHAPES = [(32000, 1), (32003, 1), (257, 1), (32003, 4), (1000, 4)]


@pytest.mark.parametrize('V,nparts', SHAPES, ids=[f'v{v}-x{n}' for v, n in SHAPES])
def test_kernel_draws_lie_in_the_restatements_interval(V, nparts):
    """Every config x rows whose soft-max has from a handful to thousands of ids above 1e-4, rows with exact ties and with
    -inf entries; history with repeated ids and padding slots; no case left out."""
    r = np.random.default_rng(V * 7 + nparts)
    scales = [0.5, 1.0, 2.0, 4.0, 8.0, 16.0]  # std of the logits: nearly flat ... a handful of ids carry the mass
    rows = len(scales) + 3
    max_in, stride = 12, 12 + 40
    end_id = 2
    for ci, cfg in enumerate(CONFIGS):
        x = np.concatenate([logits_rows(r, 1, V, s) for s in scales] + [np.zeros((3, V), np.float32)])
        # exact ties: few distinct values, the top one shared by several ids
        x[rows - 3] = r.integers(-3, 4, V).astype(np.float32)
        # -inf entries: most of the row, and the row of only -inf
        x[rows - 2] = np.where(r.uniform(size=V) < 0.9, -np.inf, logits_rows(r, 1, V, 2.0)[0])
        x[rows - 1] = -np.inf
        x[0, end_id] = 30.0  # end_id would win row 0: min_length has something to mask
        g = r.integers(1, 40, rows).astype(np.int32)
        g[0] = 3
        hist = r.integers(0, min(V, 300), (rows, stride)).astype(np.int32)  # small range: repeated ids
        hist[:, max_in:] = np.argsort(-np.nan_to_num(x, neginf=-1e30), axis=1)[:, :stride - max_in]  # likely ids get penalised
        in_len = r.integers(1, max_in + 1, rows).astype(np.int32)
        cfg = dict(cfg, random_seed=1000 + ci)
        ids = run_kernel(x, cfg, g, end_id, hist, in_len, max_in, nparts)
        rc = R.Config(**cfg)
        for b in range(rows):
            h = R.history_ids(hist[b], int(in_len[b]), max_in, int(g[b]))
            d = R.draw(x[b], rc, b, int(g[b]), end_id, h)
            assert 0 <= ids[b] < V
            check_draw(d, int(ids[b]), f'V={V} x{nparts} {cfg} row {b}')
        # same arguments again: bit-reproducible
        np.testing.assert_array_equal(ids, run_kernel(x, cfg, g, end_id, hist, in_len, max_in, nparts))
    print(f'[sampling] V={V} x{nparts}: largest excess {_worst[0]:.3e} of S')


def test_distribution_of_20000_draws_on_one_row():
    """8 ids carry almost all mass; g = 1 ... 20000 as the rows of one call.  Each id's frequency is within 5 binomial standard
    deviations of the restatement's probability (8 ids: a correct sampler trips this with probability below 1e-5)."""
    n, V = 20000, 64
    r = np.random.default_rng(99)
    row = (r.standard_normal(V) - 40.0).astype(np.float32)  # the other 56 ids: mass e^-40, below the generator's 2^-24 grid
    heavy = r.choice(V, 8, replace=False)
    row[heavy] = np.log(np.array([0.3, 0.2, 0.15, 0.12, 0.1, 0.06, 0.04, 0.03])).astype(np.float32)
    x = np.broadcast_to(row, (n, V)).copy()
    g = np.arange(1, n + 1, dtype=np.int32)
    for cfg in (dict(top_k=0, top_p=1.0, random_seed=5), dict(top_k=6, top_p=0.9, temperature=0.9, random_seed=6)):
        ids = run_kernel(x, cfg, g)
        rc = R.Config(**cfg)
        for b in range(n):
            check_draw(R.draw(row, rc, b, b + 1), int(ids[b]), f'distribution {cfg} draw {b}')
        p = R.probabilities(row, rc)
        freq = np.bincount(ids, minlength=V) / n
        sd = np.sqrt(p * (1 - p) / n)
        bad = np.nonzero(np.abs(freq - p) > 5 * sd + 1e-12)[0]
        assert len(bad) == 0, [(int(i), freq[i], p[i]) for i in bad]
        assert p[heavy].sum() > 0.999
    print(f'[sampling] distribution: largest excess {_worst[0]:.3e} of S')


# ------------------------------------------------------------------------------------------------ through the session
SAMPLING = dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1)


def build(mode, **keys):
    """(session, cfg, ids, lens): the synthetic 2-layer LLaMA of tests/test_gpu_session.py, fp16 or SmoothQuant; batch 3, ragged"""
    from oracle import quant_oracle as QO
    from test_gpu_session import synth_model
    cfg, w = synth_model(61)
    r = np.random.default_rng(23)
    B, S = 3, 10
    lens = np.array([10, 6, 8], np.int32)
    ids = np.full((B, S), 2, np.int32)
    for b in range(B):
        ids[b, :lens[b]] = r.integers(3, cfg['vocab_size'], lens[b])
    if mode == 'fp16':
        s = NativeSession(dict(cfg, quant_mode=0, **keys))
        tensors = w
    else:
        q = QO.quantise_model(cfg, w, mode, 0, calib_ids=ids, calib_lens=lens)
        s = NativeSession(dict(cfg, quant_mode=q['quant_mode'], **keys))
        tensors = q['engine_tensors']
    for k, v in tensors.items():
        s.set_tensor(k, v)
    s.finalize()
    return s, cfg, ids, lens


def check_session_step(s, rc, lens, S, g, end_id, tag):
    """the token the engine chose for generated token number g, against the restatement on the engine's OWN logits and history"""
    logits, out = s.logits(), s.output_ids()
    for b in range(out.shape[0]):
        tok = int(out[b, S + g - 1])
        if end_id >= 0 and end_id in out[b, S:S + g - 1]:
            assert tok == end_id, f'{tag}: a finished row keeps emitting end_id'
            continue
        h = R.history_ids(out[b], int(lens[b]), S, g)
        check_draw(R.draw(logits[b], rc, b, g, end_id, h), tok, f'{tag} row {b} token {g}')
    return out


@pytest.mark.parametrize('mode', ['fp16', 'sq_static'])
def test_session_steps_follow_the_rule_on_the_engines_own_logits(mode):
    """context + 12 single steps (eager, then from the graph) with sampling on, batch 3 with ragged prompts; end_id is a token a
    row draws early, so that row finishes and keeps emitting it; the step state equals what the greedy path holds."""
    s, cfg, ids, lens = build(mode)
    B, S = ids.shape
    NEW = 13
    scfg = dict(SAMPLING, random_seed=77)
    rc = R.Config(**scfg)
    s.setup(B, S, NEW)
    s.set_sampling(scfg)
    free = s.generate(ids, lens, NEW, end_id=-1)
    end_id = int(free[0, S + 3])  # row 0 draws it as its 4th token (possibly earlier, or another row does: all fine)
    s.setup(B, S, NEW)
    s.set_sampling(**scfg)
    # the step API takes end_id from the last generate(): run one with the stop token, then drive the steps by hand
    stopped = s.generate(ids, lens, NEW, end_id=end_id)
    s.context(ids, lens)
    states = []
    for g in range(1, NEW + 1):
        if g > 1:
            s.step(1, use_graph=g > 3)
        out = check_session_step(s, rc, lens, S, g, end_id, f'{mode} steps')
        states.append(s.step_state())
    assert (out[0, S + 3:] == end_id).all() or end_id in out[0, S:S + 3]
    # generate() = the hand-driven steps, up to the fill behind the end token
    for b in range(B):
        hit = np.nonzero(out[b, S:] == end_id)[0]
        upto = S + NEW if len(hit) == 0 else S + hit[0] + 1
        np.testing.assert_array_equal(stopped[b, :upto], out[b, :upto])
        assert (stopped[b, upto:] == end_id).all()
    # the device-resident step state: what the greedy path holds at the same lengths
    s.setup(B, S, NEW)
    s.generate(ids, lens, 1, end_id=end_id)  # greedy
    s.context(ids, lens)
    for g in range(1, NEW + 1):
        if g > 1:
            s.step(1, use_graph=g > 3)
        want = s.step_state()
        for k in ('sequence_length', 'next_position', 'masked_tokens', 'input_lengths'):
            np.testing.assert_array_equal(states[g - 1][k], want[k], err_msg=f'{k} at token {g}')
    s.close()
    print(f'[sampling] session {mode}: largest excess {_worst[0]:.3e} of S')


def test_eager_graph_generate_paged_and_seeds():
    """eager steps = graph-replayed steps = generate() for one seed, bit for bit; the same request twice is identical; another
    seed differs; paged KV = linear KV; back to greedy = the tokens and decode form of a session that never sampled."""
    NEW = 24
    outs = {}
    for paged in (0, 1):
        s, cfg, ids, lens = build('fp16', paged_kv_cache=paged, tokens_per_block=8)
        B, S = ids.shape
        s.setup(B, S, NEW)
        form = s.decode_form()
        greedy = s.generate(ids, lens, NEW, end_id=-1)
        scfg = dict(SAMPLING, random_seed=5)
        s.set_sampling(scfg)
        assert s.decode_form() == form
        a = s.generate(ids, lens, NEW, end_id=-1)
        np.testing.assert_array_equal(a, s.generate(ids, lens, NEW, end_id=-1))  # the same request twice
        s.context(ids, lens)
        s.step(NEW - 1, use_graph=False)
        np.testing.assert_array_equal(a, s.output_ids())
        s.context(ids, lens)
        s.step(NEW - 1, use_graph=True)
        np.testing.assert_array_equal(a, s.output_ids())
        assert not np.array_equal(a, greedy)
        s.set_sampling(dict(SAMPLING, random_seed=6))
        other = s.generate(ids, lens, NEW, end_id=-1)
        assert not np.array_equal(a, other)
        # a configuration that is plain arg-max, then no configuration: the greedy tokens again
        s.set_sampling(top_k=1, top_p=0.3, random_seed=9)
        np.testing.assert_array_equal(greedy, s.generate(ids, lens, NEW, end_id=-1))
        s.set_sampling(scfg)
        np.testing.assert_array_equal(a, s.generate(ids, lens, NEW, end_id=-1))
        s.set_sampling(None)
        np.testing.assert_array_equal(greedy, s.generate(ids, lens, NEW, end_id=-1))
        assert s.decode_form() == form
        # top_k = 1 with a penalty goes through the sampler: arg-max of the penalised logits
        s.set_sampling(top_k=1, repetition_penalty=1.5)
        s.context(ids, lens)
        rc = R.Config(top_k=1, repetition_penalty=1.5)
        for g in range(1, 6):
            if g > 1:
                s.step(1, use_graph=True)
            check_session_step(s, rc, lens, S, g, -1, 'top_k 1 + penalty')
        # forcing a token works with sampling on: the next draw sees it in its history
        s.set_sampling(scfg)
        s.context(ids, lens)
        forced = np.array([7, 8, 9], np.int32)
        s.force_tokens(forced)
        s.step(1, use_graph=False)
        out = check_session_step(s, R.Config(**scfg), lens, S, 2, -1, 'forced')
        np.testing.assert_array_equal(out[:, S], forced)
        # beam search does not sample
        s.setup(B, S, 4, beam_width=2)
        with pytest.raises(RuntimeError, match='beam'):
            s.set_sampling(scfg)
        s.close()
        outs[paged] = (greedy, a, other)
    for x, y in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(x, y)


def test_one_launch_front_consumes_the_samplers_hand_off():
    """Dh = 128, 32 heads, batch 1, SmoothQuant: the generation step's first launch reads step_epoch and the embedding row the
    sampler leaves; with sampling on it stays the one-launch form and every step follows the rule."""
    from test_gpu_fused_envelope import model
    cfg, q = model('sq_static_pc', 1)
    s = NativeSession(dict(cfg, quant_mode=q['quant_mode']))
    for k, v in q['engine_tensors'].items():
        s.set_tensor(k, v)
    s.finalize()
    r = np.random.default_rng(4)
    S, NEW = 49, 10
    lens = np.array([40], np.int32)
    ids = np.full((1, S), 2, np.int32)
    ids[0, :40] = r.integers(3, cfg['vocab_size'], 40)
    s.setup(1, S, NEW)
    assert s.decode_form() & 1
    greedy = s.generate(ids, lens, NEW, end_id=-1)
    scfg = dict(SAMPLING, random_seed=3)
    rc = R.Config(**scfg)
    s.set_sampling(scfg)
    s.context(ids, lens)
    for g in range(1, NEW + 1):
        if g > 1:
            s.step(1, use_graph=g > 2)
        out = check_session_step(s, rc, lens, S, g, -1, 'one-launch front')
    assert s.decode_form() & 1 and s.fused_retries() == 0
    np.testing.assert_array_equal(out, s.generate(ids, lens, NEW, end_id=-1))
    assert not np.array_equal(out, greedy)
    s.set_sampling(None)
    np.testing.assert_array_equal(greedy, s.generate(ids, lens, NEW, end_id=-1))
    s.close()


# ------------------------------------------------------------------------------------------------ tensor parallel 2
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_rank(rank, world, port, q):
    import ctypes
    import torch
    import torch.distributed as dist
    for p in (os.path.join(ROOT, 'trtllm-llama_amd'), ROOT, os.path.join(ROOT, 'tests')):
        sys.path.insert(0, p)
    from tensorrt_llm.plugin import capi
    from tensorrt_llm.runtime.native import NativeSession
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
        h = (ctypes.c_char * 64)()
        assert lib.tllm_comm_p2p_create(world, rank, 64 * 1024, h) == 0, capi.last_error()
        allh = [torch.zeros(64, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(allh, torch.frombuffer(bytearray(h.raw), dtype=torch.uint8))
        blob = b''.join(bytes(x.numpy().tobytes()) for x in allh)
        assert lib.tllm_comm_p2p_attach(ctypes.create_string_buffer(blob, len(blob))) == 0, capi.last_error()
        lib.tllm_comm_p2p_enable(1)
        CFG, t, ids, lens = T.model()
        B, S = ids.shape
        NEW = 16
        s = NativeSession(dict(CFG, quant_mode=0, tp_size=world, tp_rank=rank))
        for k, v in T.shard(t, world, rank).items():
            s.set_tensor(k, v)
        s.finalize()
        s.setup(B, S, NEW)
        greedy = s.generate(ids, lens, NEW, end_id=-1)
        s.set_sampling(dict(SAMPLING, random_seed=21))
        out = s.generate(ids, lens, NEW, end_id=-1)
        logits = s.logits()
        s.close()
        q.put((rank, out, logits, lib.tllm_comm_p2p_error(), greedy))
        dist.barrier()
        lib.tllm_comm_destroy_all()
    except BaseException as e:  # the parent must not wait for a result that will never come
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_tp2_ranks_draw_the_same_tokens():
    """Two ranks as processes sharing the GPU over the peer-to-peer transport: each runs the sampler on the all-gathered logits;
    counter-based u + integer sums -> identical ids for 16 sampled tokens without a broadcast.  The last token also follows the
    rule on the gathered logits."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    assert all(len(r) == 5 for r in res), [r for r in res if len(r) != 5]
    res = sorted(res, key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][3] == 0 and res[1][3] == 0
    np.testing.assert_array_equal(res[0][1], res[1][1])
    import test_tp_session_p2p as T
    _, _, ids, lens = T.model()
    S, NEW = ids.shape[1], 16
    out = res[0][1]
    np.testing.assert_array_equal(out[:, :S], ids)
    assert out.shape == (2, S + NEW) and (out[:, S:] >= 0).all() and (out[:, S:] < 512).all()
    np.testing.assert_array_equal(res[0][2], res[1][2])  # and the ranks hold the same gathered logits
    # the logits a session holds after generate() are the ones its last token was drawn from
    rc = R.Config(**dict(SAMPLING, random_seed=21))
    for b in range(2):
        h = R.history_ids(out[b], int(lens[b]), S, NEW)
        check_draw(R.draw(res[0][2][b], rc, b, NEW, -1, h), int(out[b, S + NEW - 1]), f'tp2 row {b} token {NEW}')
    # and sampling was not ignored: a greedy request on the same ranks gives other tokens
    np.testing.assert_array_equal(res[0][4], res[1][4])
    assert not np.array_equal(out, res[0][4])


# ------------------------------------------------------------------------------------------------ front-end
def test_front_end_decode_samples_reproducibly():
    """GenerationSession.decode with the configuration LLaMA is normally run with: [batch, 1, max_in + max_new], the same ids
    for the same random_seed, other ids for another; the default SamplingConfig still decodes greedily."""
    from tensorrt_llm import Mapping
    from tensorrt_llm.quantization import QuantMode
    from tensorrt_llm.runtime import GenerationSession, ModelConfig, SamplingConfig
    from test_frontend import build_tiny_engine
    engine, _, t = build_tiny_engine(QuantMode(0))
    dec = GenerationSession(ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64), engine, Mapping(1, 0))
    ids, lens = t['ids'], t['input_lengths']
    B, S = ids.shape
    NEW = 12
    dec.setup(B, S, NEW)
    greedy = dec.decode(ids, lens, SamplingConfig(end_id=-1, pad_id=2))
    scfg = SamplingConfig(end_id=-1, pad_id=2, top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1)
    scfg.random_seed = 42
    a = dec.decode(ids, lens, scfg)
    assert a.shape == (B, 1, S + NEW) and a.dtype == np.int32
    np.testing.assert_array_equal(a[:, 0, :S], ids)
    np.testing.assert_array_equal(a, dec.decode(ids, lens, scfg))
    scfg.random_seed = 43
    assert not np.array_equal(a, dec.decode(ids, lens, scfg))
    assert not np.array_equal(a, greedy)
    np.testing.assert_array_equal(greedy, dec.decode(ids, lens, SamplingConfig(end_id=-1, pad_id=2)))
    np.testing.assert_array_equal(greedy[:, 0, S], t['next_ids'])
