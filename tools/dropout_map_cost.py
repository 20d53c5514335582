#!/usr/bin/env python3
"""Cost of the dropout position map (profiles/dropout_ring.md): forward and backward of ONE dropout call through the
backend, S = 8192, H = 32 / Hk = 8, D = 128, bf16, causal, p = 0.1, with

    identity   offsets alone: the word-per-four-keys path (the only form a tree without position maps has)
    Z          both sides two pieces split at S / 2 + 1 (inside a 4-key group), the zigzag layout of rank 1 of 4
    S3         stride 3 on both sides, the stripe layout of a 3-rank group

Device events around `--iters` calls after `--warmup`, the variants alternated `--rounds` times; one JSON line.
`--identity-only` runs on a tree whose backend does not take the maps (the parent of the change), for the A/B."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--identity-only", action="store_true")
    a = ap.parse_args()

    import torch
    from ring_flash_attn import _C
    from ring_flash_attn.backend import get_backend

    assert torch.cuda.is_available(), "needs a GPU: nothing is measured without one"
    dev = torch.device("cuda:0")
    be = get_backend()
    B, S, H, Hk, D, p, seed = 1, a.seq, 32, 8, 128, 0.1, 1234
    g = torch.Generator().manual_seed(0)
    q, do = (torch.randn(B, S, H, D, generator=g).bfloat16().to(dev) for _ in range(2))
    k, v = (torch.randn(B, S, Hk, D, generator=g).bfloat16().to(dev) for _ in range(2))
    out, dq = torch.empty_like(q), torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    c = S // 2 + 1
    variants = {"identity": (p, seed, c, c, 0)}      # (misaligned like Z: two mask words per group in both)
    if not a.identity_only:
        variants["Z"] = (p, seed, c, c, 0, (1, c, 6 * c), (1, c, 6 * c))
        variants["S3"] = (p, seed, 1, 2, 0, (3, 0, 0), (3, 0, 0))
    scale = D ** -0.5

    def fwd(drop):
        be.fwd(q, k, v, softmax_scale=scale, causal=True, out=out, lse=lse, dropout=drop)

    def bwd(drop):
        be.bwd_preprocess(do, out, delta)
        be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=True, dq=dq, dk=dk, dv=dv, dropout=drop)

    def timed(fn, drop):
        for _ in range(a.warmup):
            fn(drop)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(drop)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    res = {n: {"fwd_ms": [], "bwd_ms": []} for n in variants}
    for _ in range(a.rounds):
        for n, drop in variants.items():
            res[n]["fwd_ms"].append(round(timed(fwd, drop), 4))
            res[n]["bwd_ms"].append(round(timed(bwd, drop), 4))
    print(json.dumps({"shape": dict(B=B, S=S, H=H, Hk=Hk, D=D, p=p, causal=True), "iters": a.iters, "rounds": a.rounds,
                      "build_id": be.lib.rfa_build_id().decode(), "abi": be.lib.rfa_abi_version(),
                      "device": torch.cuda.get_device_name(0), "ms_per_call": res}))


if __name__ == "__main__":
    main()
