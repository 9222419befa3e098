"""Cost of the device-side sampler next to the greedy step, in one process at the bench geometry (LLaMA-7B extents, vocab 32000,
batch 1, SmoothQuant + int8 KV, context 1024): per configuration
  * the sampler launch alone: class `other` of tllm_session_profile (a HIP event pair around every launch of eager steps;
    at hidden % 8 == 0 the sampler is the only launch of that class), microseconds per launch over `--profile-steps` steps;
  * the whole generation step: wall time of `--steps` graph-replayed steps after warm-up, as bench.py times them.
The first row is the greedy step (greedy_step_kernel), the others launch sampling_step_kernel.

    python tools/sampling_cost.py [--layers 32] [--steps 128] [--profile-steps 200]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'trtllm-llama_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = [('greedy (top_k=1)', None),
           ('top_k=1 + repetition_penalty=1.1', dict(top_k=1, repetition_penalty=1.1)),
           ('top_k=50', dict(top_k=50)),
           ('top_k=1024', dict(top_k=1024)),
           ('top_p=0.9 (top_k=0)', dict(top_k=0, top_p=0.9)),
           ('top_k=40 top_p=0.9 T=0.8 rep=1.1', dict(top_k=40, top_p=0.9, temperature=0.8, repetition_penalty=1.1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, default=32)
    ap.add_argument('--context', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--profile-steps', type=int, default=200)
    args = ap.parse_args()
    import torch
    import bench
    from tensorrt_llm.runtime.native import NativeSession
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = dict(bench.LLAMA_7B, num_layers=args.layers)
    sess = NativeSession(dict(cfg, quant_mode=bench.QM['sq'] | bench.INT8_KV))
    weights = bench.synth_weights(torch, cfg, 'sq', True, 1, 0, dev)
    for k, v in weights.items():
        sess.set_tensor(k, v)
    sess.finalize()
    stream = torch.cuda.current_stream().cuda_stream
    K, W, P = args.steps, args.warmup, args.profile_steps
    print(f'vocab {cfg["vocab_size"]}, batch 1, {args.layers} layers, context {args.context}; sampler us = event pair around the launch, '
          f'{P} launches; step ms = wall over {K} graph-replayed steps')
    print(f'{"configuration":<36} {"sampler us":>10} {"ms_per_step":>12}')
    for name, sc in CONFIGS:
        sess.setup(1, args.context, K + W + P + 8)
        if sc is not None:
            sess.set_sampling(dict(sc, random_seed=1))
        sess.fake_context(args.context, seed=1, stream=stream)
        sess.step(2, use_graph=False, stream=stream)
        sess.step(max(W, 1), use_graph=True, stream=stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.step(K, use_graph=True, stream=stream)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms, n = sess.profile(P, stream=stream)['other']
        assert n == P, f'class `other` holds {n} launches over {P} steps: not the sampler alone'
        print(f'{name:<36} {ms * 1e3 / n:>10.2f} {wall * 1e3 / K:>12.4f}', flush=True)
    sess.close()


if __name__ == '__main__':
    main()
