"""The append rule through a whole model, in numpy, for the headroom check of tests/test_append_ref.py: the logits
tllm_session_append must produce for a quantised model of oracle/quant_oracle.py - the n appended tokens as one prefill pass whose
attention is tensorrt_llm/runtime/append_ref.py (past slots from the cache the oracle's context pass left, the appended tokens'
own k and v un-quantised) - next to the oracle's teacher-forced steps, which read every earlier token from the quantised cache."""
import numpy as np

from oracle import llama_oracle as O
from oracle import quant_oracle as QO
from tensorrt_llm.runtime import append_ref as R


def append_logits(qmodel, ids, lens, feed):
    """(logits of the append rule after feed [B, n] onto the context of ids / lens, the oracle's teacher-forced logits there)"""
    m = qmodel['oracle']
    cfg = m['cfg']
    B, S = ids.shape
    n = feed.shape[1]
    H, D = cfg['num_heads'], cfg['hidden_size']
    Dh = D // H
    eps = cfg.get('rms_norm_eps', 1e-6)
    taps = {}
    ref, _ = QO.run_model(qmodel, ids, lens, 1 + n, feed_ids=feed, taps=taps)
    caches = taps['caches_after_context']
    kv = 'int8' if m['int8_kv'] else 'fp16'
    masked = np.zeros((B, S + 1 + n), np.int32)
    for b in range(B):
        masked[b, lens[b]:S] = 1
    pos = R.positions([S] * B, n, S, lens)

    def quant_in(x16, static_scale):
        if not m['sq']:
            return None
        return O.quantize_per_token(x16) if m['per_token'] else (O.quantize_tensor(x16, static_scale), None)

    x = O.f16(m['emb'][feed]).reshape(B * n, D)
    for li, lw in enumerate(m['layers']):
        h = O.rmsnorm(x, lw['ln1'], eps)
        qkv = lw['attention.qkv'](h, quant_in(h, lw.get('ln1_scale'))).reshape(B, n, 3, H, Dh)
        for b in range(B):
            for i in range(n):
                qkv[b, i, :2] = O.apply_rope(qkv[b, i, :2], int(pos[b, i]), Dh, True)
        q, k, v = (O.f16(qkv[:, :, j]).reshape(B, n, D) for j in range(3))
        out, _ = R.append_ref(q, k, v, caches[li], [S] * B, H, H, Dh, 1.0 / np.sqrt(Dh), kv, lw.get('kv_qo'), masked)
        ctx = O.f16(out.reshape(B * n, D))
        attn = lw['attention.dense'](ctx, quant_in(ctx, lw.get('attn_qscale')))
        x1 = O.f16(x + attn)
        h2 = O.rmsnorm(x1, lw['ln2'], eps)
        qi = quant_in(h2, lw.get('ln2_scale'))
        inter = O.swiglu(lw['mlp.fc'](h2, qi), lw['mlp.gate'](h2, qi))
        x = O.f16(x1 + lw['mlp.proj'](inter, quant_in(inter, lw.get('mlp_qscale'))))
    last = x.reshape(B, n, D)[:, -1]
    return (O.rmsnorm(last, m['lnf'], eps) @ m['head'].T).astype(np.float32), ref[n]
