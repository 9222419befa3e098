"""The arg-max partials between the lm_head launch and the greedy step (kernels.h GemvParams::argmax_part, GreedyParams::argmax_part):
the head's fp32 epilogue leaves one {value, index} pair per wave, the greedy step reduces those pairs instead of reading the logits
again.  Same rule on both sides (greater value wins, ties go to the lowest index), so the step must commit exactly what the scan
commits.

Logits are stamped exactly: the head instance runs with the copy prologue on x = (1, 0, ..., 0) and K = 8, so logit n is the fp16
value W[n, 0].  Vocabularies 7, 64, 1000 and 32003 (one row group, fewer groups than waves, more groups than waves of one
workgroup, several groups per wave with a ragged last round).  Into random logits go: the maximum at the first row, at the last
row, and at the last row of a wave that owns fewer groups than its neighbours; an exact tie of the maximum between two waves of
one workgroup and between two workgroups.  The pairs are held against a numpy restatement of the epilogue's rule (which wave owns
which rows follows from the number of waves that wrote a pair), the greedy step with the pairs against the scanning step on
copies of the same state: token, sequence length, finished flag, output record, RoPE row and position, next input row, step epoch.
All-(-inf) logits (token 0 either way) are written directly, with the pairs the rule gives for them.  The fall-backs: batch 2 and
two vocabulary parts are refused with the pairs and scan without them; a session runs 6 greedy steps with the partials on and
off - tokens and logits equal - and the same with a forced token and at batch 2; the session's count of greedy steps enqueued with
the pairs says that the path ran (and did not, at batch 2), and a step on the pairs over poisoned logits that it reads the pairs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gemv_cases as GC
from helpers import GemvParams
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import NativeSession

pytestmark = pytest.mark.gpu

PAIRS = 2048  # TLLM_ARGMAX_PAIRS
NONE_ID = 0x7fffffff
VOCABS = [7, 64, 1000, 32003]
HID, ROPE_HALF, TABLE_LEN, STRIDE = 64, 16, 40, 24


class GreedyParamsC(ctypes.Structure):
    """tllm_greedy_params_t (include/tllm_runtime_api.h)"""
    _fields_ = [('logits', ctypes.c_void_p), ('batch', ctypes.c_int32), ('vocab_part', ctypes.c_int32), ('nparts', ctypes.c_int32),
                ('vocab', ctypes.c_int32), ('cur_ids', ctypes.c_void_p), ('out_ids', ctypes.c_void_p), ('out_stride', ctypes.c_int32),
                ('seq_len', ctypes.c_void_p), ('finished', ctypes.c_void_p), ('end_id', ctypes.c_int32), ('advance', ctypes.c_int32),
                ('rope_row_out', ctypes.c_void_p), ('rope_pos_out', ctypes.c_void_p), ('rope_table', ctypes.c_void_p),
                ('rope_half', ctypes.c_int32), ('rope_table_len', ctypes.c_int32), ('input_lengths', ctypes.c_void_p),
                ('max_input_len', ctypes.c_int32), ('emb_table', ctypes.c_void_p), ('x_out', ctypes.c_void_p), ('hidden', ctypes.c_int32),
                ('step_epoch', ctypes.c_void_p), ('argmax_part', ctypes.c_void_p)]


@pytest.fixture(scope='module')
def api(lib):
    lib.tllm_gemv_head.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.tllm_gemv_head.restype = ctypes.c_int32
    lib.tllm_greedy_step.argtypes = [ctypes.POINTER(GreedyParamsC), ctypes.c_void_p]
    lib.tllm_greedy_step.restype = ctypes.c_int32
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def head_launch(api, vals, resident_rows=0):
    """logits[n] = vals[n] (fp16) through the head instance -> (logits f32 [V] numpy, pairs uint32 [PAIRS, 2] numpy, device tensors)"""
    V = len(vals)
    w = np.zeros((V, 8), np.float16)
    w[:, 0] = vals
    wd = torch.from_numpy(w).cuda()
    x = torch.zeros(8, dtype=torch.float16, device='cuda')
    x[0] = 1.0
    y = torch.full((V, ), float('nan'), dtype=torch.float32, device='cuda')
    part = torch.full((PAIRS, 2), 0x55555555, dtype=torch.int64, device='cuda').to(torch.int32)
    q = GemvParams(GC.W_FP16, GC.PRO_NONE, GC.EPI_NONE, GC.DT_FLOAT, 1, V, 8, x.data_ptr(), 8, wd.data_ptr(), 16, None, None, 1, 0, None,
                   1e-6, None, None, None, None, None, y.data_ptr(), V)
    rc = api.tllm_gemv_head(ctypes.byref(q), resident_rows, part.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, capi.last_error()
    return y.cpu().numpy(), part.cpu().numpy().view(np.uint32), y, part


def rule_pairs(logits, nw):
    """the epilogue's rule restated: wave w of nw finishes row groups w, w + nw, ... (rows 2 g, 2 g + 1); greater wins, ties to
    the lowest index, starting from {-inf, INT32_MAX}; slots >= nw hold that neutral pair"""
    V = len(logits)
    ngroups = (V + 1) // 2
    out = np.zeros((PAIRS, 2), np.uint32)
    out[:, 0] = np.float32(-np.inf).view(np.uint32)
    out[:, 1] = NONE_ID
    for w in range(min(nw, ngroups)):
        rows = np.concatenate([np.arange(2 * g, min(2 * g + 2, V)) for g in range(w, ngroups, nw)])
        v = logits[rows]
        if np.isnan(v).all():
            continue
        best = np.nanmax(v)
        out[w, 0] = np.float32(best).view(np.uint32)
        out[w, 1] = rows[v == best].min()
    return out


def waves_of(pairs):
    return int((pairs[:, 1] != NONE_ID).sum())


def stamped(V, kind, nw):
    """random fp16 logits in (-4, 4) with the maximum 9.5 stamped by `kind`; returns (values, expected token)"""
    r = np.random.default_rng(V * 131 + len(kind))
    vals = r.uniform(-4, 4, V).astype(np.float16)
    ngroups = (V + 1) // 2
    if kind == 'first':
        at = [0]
    elif kind == 'last':
        at = [V - 1]
    elif kind == 'short_wave':
        # the last wave owns the fewest groups (the rounds are ragged whenever nw does not divide ngroups): its last row
        w = min(nw, ngroups) - 1
        g = max(range(w, ngroups, nw))
        at = [min(2 * g + 1, V - 1)]
    elif kind == 'tie_waves':
        # groups 1 and 2: waves 1 and 2 of workgroup 0 (one group, V = 7: rows 0 and 1 of the same wave stay a tie of two lanes)
        at = [min(3, V - 1), min(4, V - 1)] if ngroups > 2 else [0, 1]
    else:  # tie_workgroups: groups 0 and 4 belong to waves 0 and 4 = workgroups 0 and 1 (where the grid has a second workgroup)
        at = [1, min(8, V - 1)] if ngroups > 4 else [0, V - 1]
    vals[at] = 9.5
    return vals, min(at)


class StepState:
    """the device buffers of one greedy step, filled identically for the scanning run and the run on the pairs"""

    def __init__(self, V, finished=0, seq=7, in_len=5):
        r = np.random.default_rng(V)
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.cur = cu(np.full(1, -1, np.int32))
        self.out = cu(np.full((1, STRIDE), -1, np.int32))
        self.seq = cu(np.array([seq], np.int32))
        self.fin = cu(np.array([finished], np.int32))
        self.in_len = cu(np.array([in_len], np.int32))
        self.rope_row = cu(np.full((1, ROPE_HALF, 2), -7.0, np.float32))
        self.rope_pos = cu(np.full(1, -1, np.int32))
        self.table = cu(r.standard_normal((TABLE_LEN, ROPE_HALF, 2)).astype(np.float32))
        self.emb = cu(r.standard_normal((V, HID)).astype(np.float16))
        self.x = cu(np.full((1, HID), 3.0, np.float16))
        self.epoch = cu(np.array([11], np.uint32).view(np.int32))

    def run(self, api, logits_dev, V, part, end_id, batch=1, nparts=1, vocab_part=None):
        q = GreedyParamsC(logits_dev.data_ptr(), batch, vocab_part or V, nparts, V, self.cur.data_ptr(), self.out.data_ptr(), STRIDE,
                          self.seq.data_ptr(), self.fin.data_ptr(), end_id, 1, self.rope_row.data_ptr(), self.rope_pos.data_ptr(),
                          self.table.data_ptr(), ROPE_HALF, TABLE_LEN, self.in_len.data_ptr(), 6, self.emb.data_ptr(), self.x.data_ptr(),
                          HID, self.epoch.data_ptr(), part.data_ptr() if part is not None else None)
        rc = api.tllm_greedy_step(ctypes.byref(q), _stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ('cur', 'out', 'seq', 'fin', 'rope_row', 'rope_pos', 'x', 'epoch')}


def both_ways(api, logits_dev, part_dev, V, end_id=-1, finished=0):
    got = []
    for part in (None, part_dev):
        st = StepState(V, finished)
        assert st.run(api, logits_dev, V, part, end_id) == 0, capi.last_error()
        got.append(st.read())
    for k in got[0]:
        assert np.array_equal(got[0][k].view(np.uint8), got[1][k].view(np.uint8)), f'{k}: the step on the pairs differs from the scan'
    return got[1]


@pytest.mark.parametrize('V', VOCABS)
def test_the_pairs_and_the_step_on_them(V, api):
    # the grid of this vocabulary on this device, from a plain run: as many pairs as waves that own a row group
    base = np.random.default_rng(V).uniform(-4, 4, V).astype(np.float16)
    logits, pairs, _, _ = head_launch(api, base)
    assert np.array_equal(logits, base.astype(np.float32))
    nw = waves_of(pairs)
    ngroups = (V + 1) // 2
    assert 1 <= nw <= min(ngroups, PAIRS)
    print(f'[V {V}] {ngroups} row groups on {nw} waves ({-(-ngroups // nw)} rounds, the last of {ngroups - (ngroups - 1) // nw * nw} groups)')
    for kind in ('first', 'last', 'short_wave', 'tie_waves', 'tie_workgroups'):
        vals, want = stamped(V, kind, nw)
        for rr in (0, V):  # the row boundary of the cache policy changes neither logits nor pairs
            logits, pairs, ldev, pdev = head_launch(api, vals, rr)
            assert np.array_equal(logits.view(np.uint32), vals.astype(np.float32).view(np.uint32))
            assert np.array_equal(pairs, rule_pairs(logits, nw)), (kind, rr)
        assert int(np.argmax(logits)) == want
        for end_id, finished in ((-1, 0), (want, 0), (3, 1)):
            got = both_ways(api, ldev, pdev, V, end_id, finished)
            tok = 3 if finished else want
            assert got['cur'][0] == tok and got['seq'][0] == 8 and got['out'][0, 8] == tok and got['epoch'].view(np.uint32)[0] == 12
            assert got['fin'][0] == (1 if (finished or end_id == want) else 0)
            assert got['rope_pos'][0] == 7 and np.array_equal(got['out'][0, :8], np.full(8, -1))
        print(f'[V {V}] {kind}: token {want}, pairs and step identical')


def test_with_the_pairs_the_step_does_not_read_the_logits(api):
    """the logits behind the pairs overwritten with another arg-max (and NaN bits): the step on the pairs still commits the pairs'
    token, the scan the poisoned one - so a step that was handed the pairs and scanned anyway cannot pass for the partials path"""
    V = 1000
    vals, want = stamped(V, 'last', 500)
    _, _, ldev, pdev = head_launch(api, vals)
    ldev.fill_(float('nan'))
    ldev[17] = 50.0
    got = []
    for part in (None, pdev):
        st = StepState(V)
        assert st.run(api, ldev, V, part, -1) == 0, capi.last_error()
        got.append(int(st.read()['cur'][0]))
    assert got == [17, want], got


def test_a_rope_row_without_input_lengths_is_refused(api):
    V = 64
    st = StepState(V)
    ldev = torch.zeros(V, dtype=torch.float32, device='cuda')
    q = GreedyParamsC(ldev.data_ptr(), 1, V, 1, V, st.cur.data_ptr(), st.out.data_ptr(), STRIDE, st.seq.data_ptr(), None, -1, 1,
                      st.rope_row.data_ptr(), None, st.table.data_ptr(), ROPE_HALF, TABLE_LEN, None, 6, None, None, 0, None, None)
    before = st.read()
    assert api.tllm_greedy_step(ctypes.byref(q), _stream()) != 0 and 'input_lengths' in capi.last_error()
    torch.cuda.synchronize()
    after = st.read()
    assert all(np.array_equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize('V', [7, 32003])
def test_all_minus_inf_gives_token_zero(V, api):
    _, pairs, _, _ = head_launch(api, np.zeros(V, np.float16))
    nw = waves_of(pairs)
    logits = np.full(V, -np.inf, np.float32)
    want = rule_pairs(logits, nw)  # every wave: {-inf, its lowest row}
    assert want[0, 1] == 0 and (want[:nw, 0] == np.float32(-np.inf).view(np.uint32)).all()
    ldev = torch.from_numpy(logits).cuda()
    pdev = torch.from_numpy(want.view(np.int32)).cuda()
    got = both_ways(api, ldev, pdev, V)
    assert got['cur'][0] == 0 and got['out'][0, 8] == 0
    # ... and with every slot neutral (a head launch that finished no row): still token 0
    neutral = rule_pairs(logits, 0)
    got = both_ways(api, ldev, torch.from_numpy(neutral.view(np.int32)).cuda(), V)
    assert got['cur'][0] == 0


def test_batch_2_and_two_parts_scan(api):
    """the pairs serve one row and one vocabulary part: with them such a launch is refused and writes nothing, without them it is
    the scan it always was"""
    V = 1000
    r = np.random.default_rng(5)
    logits = r.uniform(-4, 4, (2, V)).astype(np.float32)
    logits[1, 517] = logits[1, 44] = 9.0
    ldev = torch.from_numpy(logits).cuda()
    part = torch.zeros((PAIRS, 2), dtype=torch.int32, device='cuda')
    # two vocabulary parts of 500 for one row: the same memory read as [2 parts][1 row][500]
    for kw, want in ((dict(batch=2), None), (dict(nparts=2, vocab_part=500), int(np.argmax(logits.reshape(-1)[:1000])))):
        st = StepState(V)
        if 'batch' in kw:
            for name in ('cur', 'seq', 'fin', 'in_len', 'rope_pos'):
                setattr(st, name, getattr(st, name).repeat(2))
            st.out, st.rope_row, st.x = st.out.repeat(2, 1), st.rope_row.repeat(2, 1, 1), st.x.repeat(2, 1)
        before = st.read()
        assert st.run(api, ldev, V, part, -1, **kw) != 0 and 'partials' in capi.last_error()
        after = st.read()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        assert st.run(api, ldev, V, None, -1, **kw) == 0, capi.last_error()
        toks = st.read()['cur']
        if 'batch' in kw:
            assert toks.tolist() == [int(np.argmax(logits[0])), 44]
        else:
            assert toks.tolist() == [want]


def _tiny_session(partials, B, resident_pct):
    t = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hf_tiny_llama.npz')))
    cfg = dict(num_layers=2, num_heads=2, hidden_size=64, inter_size=24, vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-6,
               quant_mode=0, greedy_partials=partials, head_resident_pct=resident_pct)
    s = NativeSession(cfg)
    for k in [k for k in t if k.startswith('layers.')] + ['vocab_embedding.weight', 'ln_f.weight', 'lm_head.weight']:
        s.set_tensor(k, t[k])
    s.finalize()
    return s, t['ids'][:B], t['input_lengths'][:B]


@pytest.mark.parametrize('B,force', [(1, False), (1, True), (2, False)])
def test_session_tokens_and_logits_with_the_partials_on_and_off(B, force):
    """the tiny golden model, 6 greedy steps (eager, then from the replayed graph): partials + resident head against the scan +
    streaming head.  force: token 5 forced behind step 2 - the next step consumes the forced row, the step after is on its own
    again.  B = 2: the session keeps scanning whatever the key says."""
    rec = {}
    for on in (0, 1):
        s, ids, lens = _tiny_session(on, B, 100 if on else 0)
        S = ids.shape[1]
        s.setup(B, S, 8)
        s.context(ids, lens)
        logits = [s.logits()]
        for i in range(6):
            s.step(1, use_graph=i >= 2)
            logits.append(s.logits())
            if force and i == 2:
                s.force_tokens(np.full(B, 5, np.int32))
        rec[on] = (s.output_ids(), logits, s.step_state()['sequence_length'])
        # the path under test really ran: the prompt's sampler, two eager steps and the one capture took the pairs (replays of the
        # graph enqueue nothing) - and nothing did where the session must scan.  A quiet fall-back to the scan fails here.
        used = s.greedy_partials_used()
        assert (used >= 4) if (on and B == 1) else (used == 0), used
        s.close()
    np.testing.assert_array_equal(rec[0][0], rec[1][0])
    np.testing.assert_array_equal(rec[0][2], rec[1][2])
    for a, b in zip(rec[0][1], rec[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    toks, logits = rec[1][0], rec[1][1]
    S = toks.shape[1] - 8
    for i in range(7):  # each recorded token is numpy's arg-max of the logits it was chosen from (the forced one aside)
        if not (force and i == 3):
            np.testing.assert_array_equal(toks[:, S + i], np.argmax(logits[i], axis=1))
