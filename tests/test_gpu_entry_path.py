"""The decode step's kernels take the values their first loads are built from as leading, preloaded parameters and the struct
behind them ("entry contract").  A leading parameter filled from the wrong field - a base pointer, a row
stride, an extent - is what these cases are for, at the smallest shapes where it shows:

  * the GEMVs through the C ABI (tllm_gemv) on INTERIOR views of 0xFF-filled allocations with ldw = row bytes + 48, ldx > K,
    ldy > N and a residual that is not y: a wrong base or stride reads 0xFF bytes (fp16 NaN, int8 -1) or writes a sentinel.  Held
    to oracle/gemv_oracle.py with the bounds of tests/test_gpu_gemv_instances.py for these families (SmoothQuant: bit-exact;
    SwiGLU + quantiser: 1 LSB, 98 % identical; fp16 weights, fp32 output: 0.5 fp16 ulp of the row's largest value);
  * the one-launch projection + attention through the session at one layer of the 7B dimensions, against the two launches it
    replaces, eager and from the replayed graph: the projection's operand and the KV cache identical, logits within the bound of
    tests/test_gpu_fused_qkv_attn.py;
  * the greedy step through the session at a vocabulary of 32003 (the session passes vocab_part = 32003, not a multiple of 4: the
    kernel's element-wise logits loop; the benchmark's 32000 takes the 16-byte one, which the rest of the suite runs): the token equals numpy's arg-max of the step's logits (first index on ties), sequence length and step epoch advance by one."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import bench
import gemv_cases as GC
import test_gpu_gemv_instances as TG
from helpers import GemvParams
from oracle import gemv_oracle as GO
from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import NativeSession
from test_gpu_fused_qkv_attn import make, read_cache, weights

pytestmark = pytest.mark.gpu

FRONT = 4096 + 64  # bytes of 0xFF in front of (and at least as many behind) every operand inside its allocation
_C = GC.Case
SQ, F16 = GC.W_INT8_SQ, GC.W_FP16

GEMV_CASES = [
    # general kernel, SmoothQuant, one row: less than one tile per row; the session's QKV form (RMSNorm + static quantiser, residual
    # epilogue) and its gate|up form (SwiGLU + static quantiser)
    _C('entry', SQ, GC.PRO_RMSNORM_QSTATIC, GC.EPI_RESIDUAL, 1, 5, 64),
    _C('entry', SQ, GC.PRO_RMSNORM_QSTATIC, GC.EPI_SWIGLU_QSTATIC, 1, 7, 96),
    # K-split: five chunks, the first K it serves; N odd against its two rows per workgroup
    _C('entry', SQ, GC.PRO_NONE, GC.EPI_RESIDUAL, 1, 3, 4112),
    # the head's form: fp16 weights, fp32 logits
    _C('entry', F16, GC.PRO_RMSNORM, GC.EPI_NONE, 1, 33, 72, out=GC.DT_FLOAT),
]
EXPECT = [('valu', SQ, GC.PK_NORM, GC.EK_PLAIN, 1, GC.NXV_SMALL, GC.U), ('valu', SQ, GC.PK_NORM, GC.EK_SWIGLU, 1, GC.NXV_SMALL, GC.U),
          ('ksplit', SQ, 2), ('valu', F16, GC.PK_NORM, GC.EK_PLAIN, 1, GC.NXV_SMALL, GC.U)]


@pytest.fixture(scope='module')
def gemv(lib):
    lib.tllm_gemv.argtypes = [ctypes.POINTER(GemvParams), ctypes.c_void_p]
    lib.tllm_gemv.restype = ctypes.c_int32
    return lib


class View:
    """`a` (numpy) inside a 0xFF-filled device allocation, FRONT bytes from its start"""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.full(FRONT + self.host.size + FRONT, 0xFF, np.uint8)
        buf[FRONT:FRONT + self.host.size] = self.host
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + FRONT
        assert self.ptr % 16 == 0

    def read(self):
        b = self.t.cpu().numpy()
        return b[:FRONT], b[FRONT:FRONT + self.host.size], b[FRONT + self.host.size:]


def _rows(a, ld):
    """[rows, n] -> [rows, ld] with 0xFF bytes in the columns >= n"""
    out = np.full((a.shape[0], ld * a.itemsize), 0xFF, np.uint8).view(a.dtype)
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize('c,want', list(zip(GEMV_CASES, EXPECT)), ids=[GC.case_id(c) for c in GEMV_CASES])
def test_gemv_on_interior_views(c, want, gemv):
    assert GC.instance(c) == want
    tag = f'[{GC.case_id(c)}]'
    sq = c.wt == SQ
    r = np.random.default_rng(zlib.crc32(GC.case_id(c).encode()))
    rows = 2 * c.N if GC.is_swiglu(c) else c.N
    rb = GC.row_bytes(c.wt, c.K)
    ldw, ldx, ldy = rb + 48, c.K + 16, c.N + 8
    raw_s8 = sq and c.pro == GC.PRO_NONE
    x = r.integers(-127, 128, (1, c.K)).astype(np.int8) if raw_s8 else (1.7 * r.standard_normal((1, c.K))).astype(np.float16)
    gamma = r.uniform(0.5, 1.5, c.K).astype(np.float16)
    d = dict(x=x, gamma=gamma)
    if sq:
        w = r.integers(-127, 128, (rows, c.K)).astype(np.int8)
        full = np.zeros((rows, rb), np.int8)  # the layout pads a row with zeros up to Kp
        full[:, :c.K] = w
        wbuf = _rows(full, ldw)
        d['scale_row'] = np.array([0.013], np.float32)
        d['scale_col'] = (r.uniform(0.5, 1.5, rows) / (np.sqrt(c.K) * 73 * 45 * 0.013)).astype(np.float32)
        d['act_scale'], d['epi_scale'] = np.float32(37.0), np.float32(21.0)
    else:
        w = (1.7 * r.uniform(-1, 1, (rows, c.K)) / np.sqrt(c.K)).astype(np.float16)
        wbuf = _rows(w.view(np.uint8), ldw)
    d['w'] = w
    res = r.standard_normal((1, c.N)).astype(np.float16)
    d['residual'] = res
    odt = GC.out_dtype(c)
    ynp = TG._NP_OF[odt]
    V = dict(x=View(_rows(x, ldx)), w=View(wbuf), gamma=View(gamma), res=View(_rows(res, ldy)),
             y=View(np.full((1, ldy), 0xFF, np.uint8).repeat(np.dtype(ynp).itemsize, axis=1)),
             xpro=View(np.full(c.K * (1 if sq else 2), 0xFF, np.uint8)))
    for k in ('scale_col', 'scale_row'):
        V[k] = View(d[k]) if k in d else None
    V['act'] = View(np.array([d['act_scale']], np.float32)) if sq else None
    V['epi'] = View(np.array([d['epi_scale']], np.float32)) if sq else None
    ptr = lambda v: v.ptr if v is not None else None
    side = c.pro != GC.PRO_NONE
    q = GemvParams(c.wt, c.pro, c.epi, odt, c.M, c.N, c.K, V['x'].ptr, ldx, V['w'].ptr, ldw, ptr(V['scale_col']), ptr(V['scale_row']),
                   1, 0, V['gamma'].ptr if GC.pro_kind(c.pro) == GC.PK_NORM else None, 1e-6,
                   ptr(V['act']) if c.pro == GC.PRO_RMSNORM_QSTATIC else None, None, V['xpro'].ptr if side else None,
                   V['res'].ptr if c.epi == GC.EPI_RESIDUAL else None, ptr(V['epi']) if c.epi == GC.EPI_SWIGLU_QSTATIC else None,
                   V['y'].ptr, ldy)
    rc = gemv.tllm_gemv(ctypes.byref(q), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, capi.last_error()
    # nothing outside the views was written, no operand was modified
    for k, v in V.items():
        if v is None:
            continue
        front, mid, back = v.read()
        assert (front == 0xFF).all() and (back == 0xFF).all(), f'{k}: bytes outside the view written'
        if k not in ('y', 'xpro'):
            assert np.array_equal(mid, v.host), f'{k} was modified'
    y = V['y'].read()[1].view(ynp).reshape(1, ldy)
    assert TG._untouched(y[:, c.N:]), 'y columns >= N written'
    if side:
        xpro = V['xpro'].read()[1].view(np.int8 if sq else np.float16).reshape(1, c.K)
        ref = GO.prologue(x, c.pro, gamma, 1e-6, d.get('act_scale'))
        diff = (np.abs(xpro.astype(np.int32) - ref['xp'].astype(np.int32)) if sq else np.abs(TG._ord16(xpro) - TG._ord16(ref['xp'])))
        print(f'{tag} A: x_pro_out worst {diff.max()} {"LSB" if sq else "fp16 ulp"}, {100 * float((diff == 0).mean()):.3f} % identical')
        assert diff.max() <= (1 if sq else 2) and float((diff == 0).mean()) >= 0.99
        xp = xpro
    else:
        assert TG._untouched(V['xpro'].read()[1])
        xp = x
    TG.stage_b(c, d, y, xp, d.get('scale_row'), tag)


# ------------------------------------------------------------------------------------------------ the front launch
@pytest.mark.parametrize('S', [3, 193])
def test_front_launch_equals_the_two_launches(S):
    """one layer of the 7B dimensions, contexts of 3 and 193 tokens, four eager steps and four from the replayed graph"""
    layers, NEW = 1, 9
    cfg, w, qm = weights(layers, 1)
    D, H = cfg['hidden_size'], cfg['num_heads']
    ids = np.random.default_rng(S).integers(3, cfg['vocab_size'], (1, S)).astype(np.int32)
    lens = np.array([S], np.int32)
    forced = np.random.default_rng(1000 + S).integers(3, cfg['vocab_size'], NEW).astype(np.int32)
    out = {}
    for fuse in (0, 1):
        s = make(cfg, w, qm, fuse)
        s.setup(1, S, NEW)
        assert (s.decode_form() & 1) == fuse
        s.context(ids, lens)
        rec = dict(qkv_in=[], logits=[s.logits()], epoch=[s.step_epoch()])
        for i in range(NEW - 1):
            s.step(1, use_graph=i >= 4)
            rec['qkv_in'].append(s.tap(0, 'qkv_in', D, quantised=True)[0])
            rec['logits'].append(s.logits())
            rec['epoch'].append(s.step_epoch())
            # teacher forcing: a near-tie of the random weights' logits must not put the two runs on different prefixes
            s.force_tokens(forced[i:i + 1])
        rec['tokens'] = s.output_ids()
        rec['cache'] = read_cache(s, 0, 2 * H * (S + NEW) * (D // H))
        out[fuse] = rec
        s.close()
    a, b = out[0], out[1]
    assert np.diff(b['epoch']).tolist() == [1] * (NEW - 1), b['epoch']
    np.testing.assert_array_equal(a['logits'][0], b['logits'][0])  # the prefill is the same code
    np.testing.assert_array_equal(a['tokens'], b['tokens'])  # (forced: both runs consume the same tokens at every step)
    for i in range(NEW - 1):
        np.testing.assert_array_equal(a['qkv_in'][i], b['qkv_in'][i])
        dl = np.abs(a['logits'][i + 1] - b['logits'][i + 1])
        scale = max(1.0, float(np.abs(a['logits'][i + 1]).max()))
        print(f'[S {S}] step {i} ({"graph" if i >= 4 else "eager"}): logits differ by at most {dl.max():.4g} (mean {dl.mean():.4g}), scale {scale:.3g}')
        assert dl.max() <= 5e-2 * scale and dl.mean() <= 1.2e-2 * scale, (i, dl.max(), dl.mean(), scale)
    # one layer: every projection input is an embedding row, so every slot of the cache holds the same integers
    np.testing.assert_array_equal(a['cache'], b['cache'])


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('B', [1, 3])
def test_greedy_step_at_an_odd_vocabulary(B):
    V, S, NEW = 32003, 5, 4
    cfg = dict(num_layers=1, num_heads=2, hidden_size=64, inter_size=24, vocab_size=V, max_position_embeddings=64, rms_norm_eps=1e-6,
               quant_mode=0)
    r = np.random.default_rng(B)
    s = NativeSession(cfg)
    D, I = cfg['hidden_size'], cfg['inter_size']
    f16 = lambda *shape, sc=1.0: (sc * r.standard_normal(shape)).astype(np.float16)
    t = {'vocab_embedding.weight': f16(V, D), 'ln_f.weight': np.ones(D, np.float16), 'lm_head.weight': f16(V, D, sc=0.2)}
    # ties: the upper half of the head repeats the lower half, so every logit below 16000 has an equal twin 16000 ids above it -
    # the largest one too, and the lower id must win
    t['lm_head.weight'][16000:32000] = t['lm_head.weight'][:16000]
    names = ['input_layernorm.weight', 'attention.qkv.weight', 'attention.dense.weight', 'post_layernorm.weight', 'mlp.fc.weight',
             'mlp.gate.weight', 'mlp.proj.weight']
    golden = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hf_tiny_llama.npz')))
    for n in names:
        t[f'layers.0.{n}'] = golden[f'layers.0.{n}']
    for k, v in t.items():
        s.set_tensor(k, v)
    s.finalize()
    ids = r.integers(3, V, (B, S)).astype(np.int32)
    lens = np.full(B, S, np.int32)
    s.setup(B, S, NEW)
    s.context(ids, lens)
    e0, l0 = s.step_epoch(), s.step_state()['sequence_length'].copy()
    for i in range(NEW - 1):
        logits = s.logits()  # of the step before: the sampler that ended it chose from these
        toks = s.output_ids()
        lg = logits.reshape(B, -1)
        assert lg.shape[1] == V  # rows of 32003 floats: no padding to a multiple of 4
        want = np.argmax(lg, axis=1)  # first index on ties
        assert all((lg[b] == lg[b, want[b]]).sum() >= (2 if want[b] < 16000 else 1) for b in range(B))
        np.testing.assert_array_equal(toks[:, S + i], want)
        s.step(1, use_graph=i >= 1)
        st = s.step_state()
        assert s.step_epoch() == e0 + i + 1
        np.testing.assert_array_equal(st['sequence_length'], l0 + i + 1)
    s.close()
