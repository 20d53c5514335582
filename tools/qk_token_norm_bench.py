"""Time of the fused token-wide QK RMSNorm + rotary (csrc/rfa_qktoken.hip, ring_flash_attn.apply_qk_token_norm_rotary) beside
(1) the composite a caller runs without it — torch.nn.functional.rms_norm over the flattened H * D width, then
ring_flash_attn.apply_rotary — and (2) the per-head fused call apply_qk_norm_rotary at the same shape (another function, the same
traffic); same device, same process, alternating windows; the source of the table in profiles/qk_token_norm.md.

    python tools/qk_token_norm_bench.py [--out FILE.json]     on a machine with the GPU and a built librfa_hip.so

Rows: q (1, 8192, 32, 128) + k (1, 8192, 8, 128); q (1, 4096, 40, 128) + k (1, 4096, 8, 128) (OLMo-2 32B: four waves a row).
bf16, R = D (halves), fp32 tables, bf16 weights, the zigzag map of rank 1 of 4.  Forward and backward are timed apart, each side
through its public call (the fused side's direct backend calls too: `kernel`): the forwards run under no_grad, the backwards are
torch.autograd.grad over a graph that is built once per buffer set and kept.  Per side: warm-up, then five windows of 20 calls,
the sides alternating; buffers rotate over four sets (4 x 84 MB of inputs and as much output do not sit in the 256 MB cache).  One
JSON line per row and direction: the median window in us per call, bytes / s over the bytes the algorithm needs (forward: x
read, o written; backward: dO and x read, dx written), the ratios composite / fused and fused / per-head, the spreads."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    sys.path.insert(0, p)
import ring_flash_attn as R  # noqa: E402
from ring_flash_attn._common import zigzag_map  # noqa: E402

dev = torch.device("cuda:0")
DT, EPS, W, RANK = torch.bfloat16, 1e-6, 4, 1
SHAPES = [(1, 8192, 32, 8, 128), (1, 4096, 40, 8, 128)]
NSETS, WINDOWS, CALLS = 4, 5, 20


def composite(q, k, wq, wk, wd, cos, sin, pos):
    nq, nk = F.rms_norm(q.flatten(-2), (wq.numel(),), wq, EPS).view_as(q), F.rms_norm(k.flatten(-2), (wk.numel(),), wk, EPS).view_as(k)
    return R.apply_rotary(nq, nk, cos, sin, positions=pos)


def fused(q, k, wq, wk, wd, cos, sin, pos):
    return R.apply_qk_token_norm_rotary(q, k, wq, wk, cos, sin, positions=pos, eps=EPS)


def per_head(q, k, wq, wk, wd, cos, sin, pos):
    return R.apply_qk_norm_rotary(q, k, wd[0], wd[1], cos, sin, positions=pos, eps=EPS)


def windows(sides):
    """sides: {name: fn(i)}; returns {name: [us per call of each window]}"""
    times = {n: [] for n in sides}
    for fn in sides.values():
        for i in range(6):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(CALLS):
                fn(i)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    return times


def main():
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    res = []
    for B, S, H, HK, D in SHAPES:
        gen = torch.Generator().manual_seed(5)
        ang = torch.arange(W * S, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
        cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
        pos = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev)
        pm = zigzag_map(RANK, W, S // 2)
        wq, wk = ((1.0 + 0.25 * torch.randn(h * D, generator=gen)).to(DT).to(dev).requires_grad_(True) for h in (H, HK))
        wd = [(1.0 + 0.25 * torch.randn(D, generator=gen)).to(DT).to(dev).requires_grad_(True) for _ in range(2)]
        sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev).requires_grad_(True) for h in (H, HK)] for _ in range(NSETS)]
        douts = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(NSETS)]
        numel = sum(t.numel() for t in sets[0])
        # once: the composite and the fused call agree up to the composite's extra rounding between norm and rotation
        with torch.no_grad():
            a, b = fused(*sets[0], wq, wk, wd, cos, sin, pos), composite(*sets[0], wq, wk, wd, cos, sin, pos)
        for x, y in zip(a, b):
            assert bool(((x.float() - y.float()).abs() <= 2.0 ** -6 * y.float().abs() + 2.0 ** -5).all()), "composite and fused disagree"
        sides = dict(fused=fused, composite=composite, per_head=per_head)

        def fwd(fn):
            def run(i):
                with torch.no_grad():
                    fn(*sets[i % NSETS], wq, wk, wd, cos, sin, pos)
            return run

        outs = [[torch.empty_like(t) for t in ts] for ts in sets]
        dws = [torch.empty(h * D, dtype=torch.float32, device=dev) for h in (H, HK)]

        def kernel_fwd(i):
            be.qk_token_norm_rotary_fwd([t.detach() for t in sets[i % NSETS]], outs[i % NSETS], [wq.detach(), wk.detach()], cos, sin,
                                        pos_map=pm, eps=EPS)

        def kernel_bwd(i):
            be.qk_token_norm_rotary_bwd([t.detach() for t in sets[i % NSETS]], douts[i % NSETS], outs[i % NSETS],
                                        [wq.detach(), wk.detach()], dws, cos, sin, pos_map=pm, eps=EPS)

        t_f = windows(dict({n: fwd(fn) for n, fn in sides.items()}, kernel=kernel_fwd))
        graphs = {n: [fn(*ts, wq, wk, wd, cos, sin, pos) for ts in sets] for n, fn in sides.items()}

        def bwd(name):
            def run(i):
                j = i % NSETS
                torch.autograd.grad(graphs[name][j], sets[j] + (wd if name == "per_head" else [wq, wk]), douts[j], retain_graph=True)
            return run

        t_b = windows(dict({n: bwd(n) for n in sides}, kernel=kernel_bwd))
        for direction, times, passes in (("forward", t_f, 2), ("backward", t_b, 3)):
            med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
            nbytes = passes * numel * 2
            row = dict(shape=[B, S, H, HK, D], direction=direction, MB=round(nbytes / 1e6, 1),
                       **{f"{n}_us": round(v, 1) for n, v in med.items()},
                       **{f"{n}_spread": [round(min(v), 1), round(max(v), 1)] for n, v in times.items()},
                       kernel_TBps=round(nbytes / med["kernel"] / 1e6, 2), fused_TBps=round(nbytes / med["fused"] / 1e6, 2),
                       composite_over_fused=round(med["composite"] / med["fused"], 2),
                       fused_over_per_head=round(med["fused"] / med["per_head"], 2))
            res.append(row)
            print(json.dumps(row), flush=True)
        del graphs, sets, douts, outs
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
