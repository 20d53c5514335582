#!/usr/bin/env python3
"""Timings behind profiles/vdim.md, on one MI355X: a value head dim of its own (csrc/rfa_vdim.hip) beside what callers did
before it — V, dout and out zero-padded to the QK head dim through the existing kernels (csrc/rfa_bigd.hip).

Shapes: D 192 / Dv 128, causal, bf16, H = Hk = 16; S = 8192, B = 1 and S = 2048, B = 4.  Timed: `be.fwd`, then
`be.bwd_preprocess` + `be.bwd` (the 5-GEMM form: the reusable dS scratch is made before the clock starts), the same two on the
padded tensors, and — separately — the pad / slice copies a caller of the padded form pays around them (pad V; pad dout;
slice out; slice dV).  The calls ALTERNATE batch by batch; device events around each batch; the median, and the spread
(min, max) over the batches — the padded call's spread is the margin the comparison is read against.

Usage: python tools/vdim_bench.py [--batches 15] [--per-batch 5] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ring-flash-attention_amd"))


def timed(fns, batches, per_batch):
    """(median, min, max) milliseconds per call of each fn: batches alternate between the fns"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(batches):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_batch):
                fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / per_batch)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def flops(B, S, H, D, Dv):
    """useful multiply-adds x 2 of the causal forward / 5-GEMM backward (half the square); the padded call is credited with
    the SAME useful work"""
    pairs = B * H * S * S / 2
    return 2 * pairs * (D + Dv), 2 * pairs * (3 * D + 2 * Dv)


def one_shape(be, dev, B, S, H, D, Dv, batches, per_batch):
    g = torch.Generator().manual_seed(0)
    mk = lambda d: torch.randn(B, S, H, d, generator=g).bfloat16().to(dev)
    q, k, v, do = mk(D), mk(D), mk(Dv), mk(Dv)
    pad = lambda t: torch.nn.functional.pad(t, (0, D - Dv))
    vp, dop = pad(v), pad(do)
    scale = D ** -0.5
    out, outp = torch.empty(B, S, H, Dv, dtype=q.dtype, device=dev), torch.empty_like(q)
    lse, lsep = (torch.empty(B, H, S, dtype=torch.float32, device=dev) for _ in range(2))
    delta, deltap = torch.empty_like(lse), torch.empty_like(lse)
    dq, dk, dv, dvp = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(vp)

    fwd = lambda: be.fwd(q, k, v, softmax_scale=scale, causal=True, out=out, lse=lse)
    fwdp = lambda: be.fwd(q, k, vp, softmax_scale=scale, causal=True, out=outp, lse=lsep)

    def bwd():
        be.bwd_preprocess(do, out, delta)
        be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=True, dq=dq, dk=dk, dv=dv)

    def bwdp():
        be.bwd_preprocess(dop, outp, deltap)
        be.bwd(dop, q, k, vp, lsep, deltap, softmax_scale=scale, causal=True, dq=dq, dk=dk, dv=dvp)

    def copies():
        pad(v), pad(do), outp[..., :Dv].contiguous(), dvp[..., :Dv].contiguous()

    fwd(), fwdp(), bwd(), bwdp()                                   # (the dS scratch exists from here on)
    torch.cuda.synchronize()
    assert torch.equal(lse, lsep) or (lse - lsep).abs().max().item() < 1e-4
    names = ("fwd", "fwd_padded", "bwd", "bwd_padded", "pad_slice_copies")
    res = dict(zip(names, timed([fwd, fwdp, bwd, bwdp, copies], batches, per_batch)))
    # the padded calls a second time, alone: the run-to-run spread of the yardstick inside this session
    again = dict(zip(("fwd_padded_again", "bwd_padded_again"), timed([fwdp, bwdp], batches, per_batch)))
    res.update(again)
    ff, fb = flops(B, S, H, D, Dv)
    row = dict(shape=dict(B=B, S=S, H=H, Hk=H, D=D, Dv=Dv, causal=True, dtype="bf16"),
               ms={n: dict(median=round(t[0], 4), min=round(t[1], 4), max=round(t[2], 4)) for n, t in res.items()},
               tflops=dict(fwd=round(ff / res["fwd"][0] * 1e-9, 1), fwd_padded=round(ff / res["fwd_padded"][0] * 1e-9, 1),
                           bwd=round(fb / res["bwd"][0] * 1e-9, 1), bwd_padded=round(fb / res["bwd_padded"][0] * 1e-9, 1)),
               ratio=dict(fwd=round(res["fwd"][0] / res["fwd_padded"][0], 4), bwd=round(res["bwd"][0] / res["bwd_padded"][0], 4)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--per-batch", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from ring_flash_attn.backend import get_backend

    be, dev = get_backend(), torch.device("cuda:0")
    rows = [one_shape(be, dev, B, S, 16, 192, 128, a.batches, a.per_batch) for B, S in ((1, 8192), (4, 2048))]
    for r in rows:
        s, ms = r["shape"], r["ms"]
        print(f"B {s['B']} S {s['S']} H {s['H']} D {s['D']} / Dv {s['Dv']} causal bf16")
        for n, t in ms.items():
            print(f"  {n:18s} median {t['median']:.4f} ms (min {t['min']:.4f}, max {t['max']:.4f})")
        print(f"  new / padded (medians): fwd {r['ratio']['fwd']:.4f}, bwd {r['ratio']['bwd']:.4f}; useful TFLOP/s {r['tflops']}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
