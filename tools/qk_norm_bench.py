"""Time of the fused per-head QK RMSNorm + rotary (csrc/rfa_qknorm.hip, ring_flash_attn.apply_qk_norm_rotary) beside (1) the
composite a caller runs without it — torch.nn.functional.rms_norm over each head, then ring_flash_attn.apply_rotary — and (2)
apply_rotary alone; same device, same process, alternating windows; the source of the table in profiles/qk_norm.md.

    python tools/qk_norm_bench.py [--out FILE.json]     on a machine with the GPU and a built librfa_hip.so
    python tools/qk_norm_bench.py --rehearse            tiny shapes on the CPU test backend, no timing

Rows: q (1, 8192, 32, 128) + k (1, 8192, 8, 128); the same with D = 256; B 4, S 2048 at D = 128.  bf16, R = D (halves), fp32
tables, bf16 weights, the zigzag map of rank 1 of 4.  Forward and backward are timed apart, each side through its public call
(the fused side's direct backend calls too: `kernel`): the forwards run under no_grad, the backwards are torch.autograd.grad
over a graph that is built once per buffer set and kept.  Per side: warm-up, then five windows of 20 calls, the sides
alternating; buffers rotate over four sets (4 x 84 MB of inputs and as much output do not sit in the 256 MB cache).  One JSON
line per row and direction: the median window in us per call, bytes / s over the bytes the algorithm needs (forward: x read, o
written; backward: dO and x read, dx written), the ratios composite / fused and fused / rotary, the spreads."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ring_flash_attn as R  # noqa: E402
from ring_flash_attn import _testing  # noqa: E402
from ring_flash_attn._common import zigzag_map  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
dev = torch.device("cpu" if REHEARSE else "cuda:0")
DT, EPS, W, RANK = torch.bfloat16, 1e-6, 4, 1
SHAPES = [(1, 8, 4, 2, 32)] if REHEARSE else [(1, 8192, 32, 8, 128), (1, 8192, 32, 8, 256), (4, 2048, 32, 8, 128)]
NSETS, WINDOWS, CALLS = (1, 1, 1) if REHEARSE else (4, 5, 20)


def composite(q, k, wq, wk, cos, sin, pos):
    D = q.shape[-1]
    return R.apply_rotary(F.rms_norm(q, (D,), wq, EPS), F.rms_norm(k, (D,), wk, EPS), cos, sin, positions=pos)


def fused(q, k, wq, wk, cos, sin, pos):
    return R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin, positions=pos, eps=EPS)


def rotary(q, k, wq, wk, cos, sin, pos):
    return R.apply_rotary(q, k, cos, sin, positions=pos)


def windows(sides):
    """sides: {name: fn(i)}; returns {name: [us per call of each window]}"""
    times = {n: [] for n in sides}
    if REHEARSE:
        for fn in sides.values():
            fn(0)
        return {n: [0.0] for n in sides}
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
    if REHEARSE:
        from _qknorm_backend import QkNormBackend

        _testing.set_backend(QkNormBackend(serves=("mask_shift",)))
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    res = []
    for B, S, H, HK, D in SHAPES:
        gen = torch.Generator().manual_seed(5)
        P = W * S
        ang = torch.arange(P, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
        cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
        pos = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev)
        pm = zigzag_map(RANK, W, S // 2)
        wq, wk = ((1.0 + 0.25 * torch.randn(D, generator=gen)).to(DT).to(dev).requires_grad_(True) for _ in range(2))
        sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev).requires_grad_(True) for h in (H, HK)] for _ in range(NSETS)]
        douts = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(NSETS)]
        numel = sum(t.numel() for t in sets[0])
        # once: the composite and the fused call agree up to the composite's extra rounding between norm and rotation
        with torch.no_grad():
            a, b = fused(*sets[0], wq, wk, cos, sin, pos), composite(*sets[0], wq, wk, cos, sin, pos)
        for x, y in zip(a, b):
            assert bool(((x.float() - y.float()).abs() <= 2.0 ** -6 * y.float().abs() + 2.0 ** -5).all()), "composite and fused disagree"
        sides = dict(fused=fused, composite=composite, rotary=rotary)

        def fwd(fn):
            def run(i):
                with torch.no_grad():
                    fn(*sets[i % NSETS], wq, wk, cos, sin, pos)
            return run

        outs = [[torch.empty_like(t) for t in ts] for ts in sets]
        dws = [torch.empty(D, dtype=torch.float32, device=dev) for _ in range(2)]

        def kernel_fwd(i):
            be.qk_norm_rotary_fwd([t.detach() for t in sets[i % NSETS]], outs[i % NSETS], [wq.detach(), wk.detach()], cos, sin,
                                  pos_map=pm, eps=EPS)

        def kernel_bwd(i):
            be.qk_norm_rotary_bwd([t.detach() for t in sets[i % NSETS]], douts[i % NSETS], outs[i % NSETS],
                                  [wq.detach(), wk.detach()], dws, cos, sin, pos_map=pm, eps=EPS)

        t_f = windows(dict({n: fwd(fn) for n, fn in sides.items()}, kernel=kernel_fwd))
        graphs = {n: [fn(*ts, wq, wk, cos, sin, pos) for ts in sets] for n, fn in sides.items()}

        def bwd(name):
            def run(i):
                j = i % NSETS
                leaves = sets[j] + ([wq, wk] if name != "rotary" else [])
                torch.autograd.grad(graphs[name][j], leaves, douts[j], retain_graph=True)
            return run

        t_b = windows(dict({n: bwd(n) for n in sides}, kernel=kernel_bwd))
        for direction, times, passes in (("forward", t_f, 2), ("backward", t_b, 3)):
            med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
            nbytes = passes * numel * 2
            rot_bytes = 2 * numel * 2                                         # (the rotation's backward reads dO and writes dx)
            row = dict(shape=[B, S, H, HK, D], direction=direction, MB=round(nbytes / 1e6, 1),
                       **{f"{n}_us": round(v, 1) for n, v in med.items()},
                       **{f"{n}_spread": [round(min(v), 1), round(max(v), 1)] for n, v in times.items()})
            if not REHEARSE:
                row.update(kernel_TBps=round(nbytes / med["kernel"] / 1e6, 2), fused_TBps=round(nbytes / med["fused"] / 1e6, 2),
                           rotary_TBps=round(rot_bytes / med["rotary"] / 1e6, 2),
                           composite_over_fused=round(med["composite"] / med["fused"], 2),
                           fused_over_rotary=round(med["fused"] / med["rotary"], 2))
            res.append(row)
            print(json.dumps(row), flush=True)
        del graphs, sets, douts, outs
    if REHEARSE:
        print("rehearsal ok")
        return
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
