#!/usr/bin/env python3
"""Time the per-head max attention logit (csrc/rfa_maxlogit.hip, HipBackend.max_logit) beside what it is a subset of and
what it replaces, and print the table of profiles/max_logit.md:

    python tools/max_logit_bench.py [--iters 20] [--out FILE]

Shapes: B 1, S 8192, H 32 / Hk 8, D 128 causal and non-causal; D 64; D 256; B 4 x S 2048.  Per shape, in ONE process, warmed,
device events, the three arms alternating inside every iteration (so that clocks and temperature drift hit them alike):
    max_logit   one be.max_logit call — the attention kernel and the finish kernel
    fwd         be.fwd of the same arguments (plain outputs)
    composite   the torch code it replaces: per chunk of 4 query heads einsum(q, k) * scale, the causal mask, amax
Columns: median microseconds, TFLOP/s of max_logit over 2 * visible pairs * D, and the two ratios the design promises
(max_logit <= fwd; max_logit < composite) with a plain yes / NO."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [dict(B=1, S=8192, H=32, Hk=8, D=128, causal=True), dict(B=1, S=8192, H=32, Hk=8, D=128, causal=False),
          dict(B=1, S=8192, H=32, Hk=8, D=64, causal=True), dict(B=1, S=8192, H=32, Hk=8, D=256, causal=True),
          dict(B=4, S=2048, H=32, Hk=8, D=128, causal=True)]


def composite(q, k, scale, causal, chunk=4):
    """the max logit per head in plain torch, a chunk of query heads at a time (the full score tensor of 32 heads at S 8192
    would be 8 GiB in fp32)"""
    B, S, H, D = q.shape
    G = H // k.shape[2]
    out = torch.empty(H, dtype=torch.float32, device=q.device)
    mask = torch.ones(S, k.shape[1], dtype=torch.bool, device=q.device).tril_() if causal else None
    for h0 in range(0, H, chunk):
        kk = k[:, :, h0 // G:(h0 + chunk + G - 1) // G].repeat_interleave(G, dim=2)[:, :, :chunk]
        s = torch.einsum("bihd,bjhd->bhij", q[:, :, h0:h0 + chunk], kk).float() * scale
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        out[h0:h0 + chunk] = s.amax(dim=(0, 2, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ring_flash_attn.backend import get_backend

    dev = torch.device("cuda:0")
    be = get_backend()
    lines = ["| shape | max_logit us | TFLOP/s | fwd us | composite us | max_logit / fwd | <= fwd | composite / max_logit | < composite | agrees |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for sh in SHAPES:
        B, S, H, Hk, D, causal = (sh[n] for n in ("B", "S", "H", "Hk", "D", "causal"))
        g = torch.Generator().manual_seed(0)
        q = torch.randn(B, S, H, D, generator=g).bfloat16().to(dev)
        k = torch.randn(B, S, Hk, D, generator=g).bfloat16().to(dev)
        v = torch.randn(B, S, Hk, D, generator=g).bfloat16().to(dev)
        out, lse = torch.empty_like(q), torch.empty(B, H, S, dtype=torch.float32, device=dev)
        m = torch.empty(H, dtype=torch.float32, device=dev)
        scale = D ** -0.5
        arms = {"max_logit": lambda: be.max_logit(q, k, m, softmax_scale=scale, causal=causal, accumulate=False),
                "fwd": lambda: be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse),
                "composite": lambda: composite(q, k, scale, causal)}
        for fn in arms.values():                                     # warm-up: code objects, scratch, the allocator's pool
            fn()
            fn()
        torch.cuda.synchronize()
        ts = {n: [] for n in arms}
        for _ in range(a.iters):
            for n, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[n].append(e0.elapsed_time(e1) * 1e3)
        med = {n: sorted(x)[len(x) // 2] for n, x in ts.items()}
        # (the composite's einsum rounds its output to bf16 — a relative 2^-8 — before the scale: twice that is allowed)
        agrees = bool(torch.allclose(m, composite(q, k, scale, causal), rtol=2.0 ** -7, atol=0))
        pairs = B * H * (S * (S + 1) // 2 if causal else S * S)
        tflops = 2 * pairs * D / med["max_logit"] / 1e6
        r_f, r_c = med["max_logit"] / med["fwd"], med["composite"] / med["max_logit"]
        lines.append(f"| B {B} S {S} H {H}/{Hk} D {D} {'causal' if causal else 'full'} | {med['max_logit']:.1f} | {tflops:.0f} | "
                     f"{med['fwd']:.1f} | {med['composite']:.1f} | {r_f:.2f} | {'yes' if r_f <= 1.0 else 'NO'} | {r_c:.1f} | "
                     f"{'yes' if r_c > 1.0 else 'NO'} | {'yes' if agrees else 'NO'} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
