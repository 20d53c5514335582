#!/usr/bin/env python3
"""Time the two attention-sink kernels (csrc/rfa_sink.hip) at one shape — alone, with HIP events, or as the program of a
profiler run, whose per-kernel statistics then carry the figures:

    python tools/sink_kernels.py --seq 8192 --heads 64 --kv-heads 8 --dim 64 [--window 127 0] [--attention]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/sink_kernels.py ...

Prints one JSON line: microseconds per call (median of --iters) and the achieved bytes/s of each kernel, counting what the
kernel has to move: sink_apply reads and writes out (io dtype) and lse (fp32); sink_grad reads dO, out' and lse'.
--attention also runs `with_sinks(ring_flash_attn_func, sinks)` forward and backward once per iteration on a single-rank
group (causal, with the window), so that a profile shows the two kernels beside the attention kernels of the same step."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--heads", type=int, default=64)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--window", type=int, nargs=2, default=(-1, -1))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--attention", action="store_true")
    a = ap.parse_args()
    from ring_flash_attn.backend import get_backend

    dev = torch.device("cuda:0")
    be = get_backend()
    B, S, H, D = a.batch, a.seq, a.heads, a.dim
    g = torch.Generator().manual_seed(0)
    out = torch.randn(B, S, H, D, generator=g).bfloat16().to(dev)
    do = torch.randn(B, S, H, D, generator=g).bfloat16().to(dev)
    lse = (3 + torch.randn(B, H, S, generator=g)).to(dev)
    sinks = (3 + torch.randn(H, generator=g)).to(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return sorted(ts)[len(ts) // 2]

    o2, l2 = be.sink_apply(out, lse, sinks, varlen=False)
    t_apply = timed(lambda: be.sink_apply(out, lse, sinks, varlen=False, inplace=False))
    t_grad = timed(lambda: be.sink_grad(do, o2, l2, sinks, varlen=False))
    rows = B * S * H
    bytes_apply = rows * (2 * D * 2 + 2 * 4)
    bytes_grad = rows * (2 * D * 2 + 4)
    res = dict(shape=dict(B=B, S=S, H=H, Hk=a.kv_heads, D=D, window=list(a.window)),
               sink_apply_us=round(t_apply, 2), sink_apply_bytes=bytes_apply, sink_apply_TBps=round(bytes_apply / t_apply / 1e6, 3),
               sink_grad_us=round(t_grad, 2), sink_grad_bytes=bytes_grad, sink_grad_TBps=round(bytes_grad / t_grad / 1e6, 3),
               note="event timing of one backend call: launch overhead and the allocation of the outputs included")
    if a.attention:
        import torch.distributed as dist

        import ring_flash_attn as R

        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29541")
            dist.init_process_group("gloo", rank=0, world_size=1)
        q = torch.randn(B, S, H, D, generator=g).bfloat16().to(dev).requires_grad_(True)
        k, v = (torch.randn(B, S, a.kv_heads, D, generator=g).bfloat16().to(dev).requires_grad_(True) for _ in range(2))
        sk = sinks.clone().requires_grad_(True)

        def step(fn):
            fn(q, k, v, causal=True, window_size=tuple(a.window)).backward(do)

        res["step_with_sinks_us"] = round(timed(lambda: step(R.with_sinks(R.ring_flash_attn_func, sk))), 1)
        res["step_plain_us"] = round(timed(lambda: step(R.ring_flash_attn_func)), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
