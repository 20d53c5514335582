#!/usr/bin/env python3
"""Timings behind profiles/lse_grad.md, on one MI355X:

  1. rfa_bwd_preprocess_lse beside rfa_bwd_preprocess at the headline shape (B 1, S 8192, H 32, D 128, bf16): the two calls
     alternate, device events around batches of launches, the median over the batches.
  2. merge_attn forward and backward beside the torch composite (logaddexp, exp, two scaled adds, a cast; autograd for the
     backward) at (1, 8192, 32, 128), as achieved bandwidth over the bytes the operation NEEDS (computed from the shapes here:
     every input read once, every output written once).

Usage: python tools/lse_grad_perf.py [--batches 40] [--per-batch 50]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ring-flash-attention_amd"))


def timed(fns, batches, per_batch):
    """median microseconds per call of each fn: batches alternate between the fns, events around `per_batch` launches"""
    for fn in fns:
        for _ in range(10):
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
            times[i].append(a.elapsed_time(b) * 1e3 / per_batch)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--per-batch", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from ring_flash_attn.backend import get_backend
    import ring_flash_attn as R

    be, dev = get_backend(), torch.device("cuda:0")
    B, S, H, D = 1, 8192, 32, 128
    g = torch.Generator().manual_seed(0)
    mk = lambda: torch.randn(B, S, H, D, generator=g).bfloat16().to(dev)
    do, o = mk(), mk()
    dlse = torch.randn(B, H, S, generator=g).to(dev)
    delta = torch.empty(B, H, S, device=dev)
    (plain, lse_) = timed([lambda: be.bwd_preprocess(do, o, delta), lambda: be.bwd_preprocess(do, o, delta, dlse=dlse)],
                          a.batches, a.per_batch)
    n = B * S * H
    for nm, t, nbytes in (("rfa_bwd_preprocess", plain, n * (2 * 2 * D + 4)), ("rfa_bwd_preprocess_lse", lse_, n * (2 * 2 * D + 8))):
        print(f"{nm}: median {t[0]:.2f} us (min {t[1]:.2f}, max {t[2]:.2f}), {nbytes / t[0] * 1e-3:.0f} GB/s over {nbytes} bytes")
    print(f"ratio lse / plain (medians): {lse_[0] / plain[0]:.4f}")

    oa, ob, dout = mk(), mk(), mk()
    la, lb = (3 + 2 * torch.randn(B, H, S, generator=g)).to(dev), (3 + 2 * torch.randn(B, H, S, generator=g)).to(dev)

    def composite(oa, la, ob, lb):
        lse = torch.logaddexp(la, lb)
        wa, wb = (torch.exp(l - lse).transpose(1, 2).unsqueeze(-1) for l in (la, lb))
        return (wa * oa.float() + wb * ob.float()).to(oa.dtype), lse

    leaves = [t.clone().requires_grad_(True) for t in (oa, la, ob, lb)]

    def fwd_bwd(fn):
        def run():
            for t in leaves:
                t.grad = None
            out, lse = fn(*leaves)
            torch.autograd.backward([out, lse], [dout, dlse])
        return run

    with torch.no_grad():
        f_k, f_t = timed([lambda: R.merge_attn(oa, la, ob, lb), lambda: composite(oa, la, ob, lb)], a.batches, a.per_batch)
    fb_k, fb_t = timed([fwd_bwd(R.merge_attn), fwd_bwd(composite)], a.batches, max(1, a.per_batch // 5))
    fwd_bytes = n * (3 * 2 * D + 3 * 4)
    bwd_bytes = n * (5 * 2 * D + 5 * 4)
    print(f"merge_attn forward: kernel {f_k[0]:.1f} us = {fwd_bytes / f_k[0] * 1e-3:.0f} GB/s; torch composite {f_t[0]:.1f} us = "
          f"{fwd_bytes / f_t[0] * 1e-3:.0f} GB/s over the {fwd_bytes} bytes the operation needs")
    for nm, fb, f in (("kernel", fb_k, f_k), ("torch composite", fb_t, f_t)):
        bw = fb[0] - f[0]
        print(f"merge_attn forward + backward ({nm}): {fb[0]:.1f} us; backward alone (difference, autograd overhead included) "
              f"{bw:.1f} us = {bwd_bytes / bw * 1e-3:.0f} GB/s over {bwd_bytes} bytes")
    out_k, lse_k = R.merge_attn(oa, la, ob, lb)
    out_t, lse_t = composite(oa, la, ob, lb)
    print(f"kernel vs composite: max|out diff| {(out_k.float() - out_t.float()).abs().max().item():.3e}, "
          f"max|lse diff| {(lse_k - lse_t).abs().max().item():.3e}")


if __name__ == "__main__":
    main()
