"""Time of the token-wide QK RMSNorm + rotary that forms its own angles (csrc/rfa_qktokenfreq.hip,
ring_flash_attn.apply_qk_token_norm_rotary_freqs) beside (1) the table call apply_qk_token_norm_rotary on fp32 tables, (2) the
two calls it replaces — the token norm alone, then apply_rotary_freqs — and (3) those two calls behind cos / sin built per call
from inv_freq and the positions, then apply_rotary; same device, same process, alternating windows; the source of the table in
profiles/qk_token_norm_freqs.md.

    python tools/qk_token_norm_freqs_bench.py [--out FILE.json]     on a machine with the GPU and a built librfa_hip.so

q (1, 8192, 32, 128) + k (1, 8192, 8, 128) bf16, R = D (halves), bf16 weights, the positions of rank 1 of 4 of the zigzag
layout as an int32 tensor.  Forward and backward are timed apart, each side through its public call (the fused side's direct
backend calls too: `kernel`; the backward's includes the fold launch): the forwards run under no_grad, the backwards are
torch.autograd.grad over a graph that is built once per buffer set and kept.  Per side: warm-up, then five windows of 20 calls,
the sides alternating; buffers rotate over four sets.  One JSON line per direction: the median window in us per call, the
(min, max) over the windows, and the ratios of medians."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    sys.path.insert(0, p)
import ring_flash_attn as R  # noqa: E402

dev = torch.device("cuda:0")
DT, EPS, W, RANK = torch.bfloat16, 1e-6, 4, 1
B, S, H, HK, D = 1, 8192, 32, 8, 128
NSETS, WINDOWS, CALLS = 4, 5, 20


def fused(q, k, wq, wk, inv, cos, sin, pos):
    return R.apply_qk_token_norm_rotary_freqs(q, k, wq, wk, inv, positions=pos, eps=EPS)


def tables(q, k, wq, wk, inv, cos, sin, pos):
    return R.apply_qk_token_norm_rotary(q, k, wq, wk, cos, sin, positions=pos, eps=EPS)


def two_calls(q, k, wq, wk, inv, cos, sin, pos):
    nq, nk = R.apply_qk_token_norm_rotary(q, k, wq, wk, eps=EPS)
    return R.apply_rotary_freqs(nq, nk, inv, positions=pos)


def two_calls_own_tables(q, k, wq, wk, inv, cos, sin, pos):
    nq, nk = R.apply_qk_token_norm_rotary(q, k, wq, wk, eps=EPS)
    ang = pos.float().unsqueeze(-1) * inv                          # (S, R/2): what a caller without tables builds per call
    return R.apply_rotary(nq, nk, ang.cos(), ang.sin())


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
    gen = torch.Generator().manual_seed(5)
    inv = (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2))).float().to(dev)
    ang = torch.arange(W * S, dtype=torch.float32, device=dev).view(-1, 1) * inv
    cos, sin = ang.cos(), ang.sin()
    pos = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev)
    wq, wk = ((1.0 + 0.25 * torch.randn(h * D, generator=gen)).to(DT).to(dev).requires_grad_(True) for h in (H, HK))
    sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev).requires_grad_(True) for h in (H, HK)] for _ in range(NSETS)]
    douts = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(NSETS)]
    with torch.no_grad():                                          # once: the sides agree up to the composites' extra rounding
        a = fused(*sets[0], wq, wk, inv, cos, sin, pos)
        for other in (tables, two_calls, two_calls_own_tables):
            for x, y in zip(a, other(*sets[0], wq, wk, inv, cos, sin, pos)):
                assert bool(((x.float() - y.float()).abs() <= 2.0 ** -6 * y.float().abs() + 2.0 ** -5).all()), other.__name__
    sides = dict(fused=fused, tables=tables, two_calls=two_calls, two_calls_own_tables=two_calls_own_tables)

    def fwd(fn):
        def run(i):
            with torch.no_grad():
                fn(*sets[i % NSETS], wq, wk, inv, cos, sin, pos)
        return run

    outs = [[torch.empty_like(t) for t in ts] for ts in sets]
    dws = [torch.empty(h * D, dtype=torch.float32, device=dev) for h in (H, HK)]

    def kernel_fwd(i):
        be.qk_token_norm_freqs_rotary_fwd([t.detach() for t in sets[i % NSETS]], outs[i % NSETS], [wq.detach(), wk.detach()], inv,
                                          positions=pos, eps=EPS)

    def kernel_bwd(i):
        be.qk_token_norm_freqs_rotary_bwd([t.detach() for t in sets[i % NSETS]], douts[i % NSETS], outs[i % NSETS],
                                          [wq.detach(), wk.detach()], dws, inv, positions=pos, eps=EPS)

    def table_kernel_fwd(i):
        be.qk_token_norm_rotary_fwd([t.detach() for t in sets[i % NSETS]], outs[i % NSETS], [wq.detach(), wk.detach()], cos, sin,
                                    positions=pos, eps=EPS)

    def table_kernel_bwd(i):
        be.qk_token_norm_rotary_bwd([t.detach() for t in sets[i % NSETS]], douts[i % NSETS], outs[i % NSETS],
                                    [wq.detach(), wk.detach()], dws, cos, sin, positions=pos, eps=EPS)

    res = []
    t_f = windows(dict({n: fwd(fn) for n, fn in sides.items()}, kernel=kernel_fwd, table_kernel=table_kernel_fwd))
    graphs = {n: [fn(*ts, wq, wk, inv, cos, sin, pos) for ts in sets] for n, fn in sides.items()}

    def bwd(name):
        def run(i):
            j = i % NSETS
            torch.autograd.grad(graphs[name][j], sets[j] + [wq, wk], douts[j], retain_graph=True)
        return run

    t_b = windows(dict({n: bwd(n) for n in sides}, kernel=kernel_bwd, table_kernel=table_kernel_bwd))
    for direction, times in (("forward", t_f), ("backward", t_b)):
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        row = dict(shape=[B, S, H, HK, D], direction=direction,
                   **{f"{n}_us": round(v, 1) for n, v in med.items()},
                   **{f"{n}_spread": [round(min(v), 1), round(max(v), 1)] for n, v in times.items()},
                   tables_over_fused=round(med["tables"] / med["fused"], 3),
                   two_calls_over_fused=round(med["two_calls"] / med["fused"], 3),
                   two_calls_own_tables_over_fused=round(med["two_calls_own_tables"] / med["fused"], 3),
                   table_kernel_over_kernel=round(med["table_kernel"] / med["kernel"], 3))
        res.append(row)
        print(json.dumps(row), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
