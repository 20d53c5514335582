"""Time of the per-head QK RMSNorm + rotary that forms its own angles (csrc/rfa_qknormfreq.hip,
ring_flash_attn.apply_qk_norm_rotary_freqs) beside the two things a caller runs without it: (1) `two_calls` — the norm alone,
apply_qk_norm_rotary(cos=None, sin=None), then apply_rotary_freqs — and (2) `tables` — apply_qk_norm_rotary on fp32 tables of
the unsharded sequence (single axis only: no table describes three).  Same device, same process, alternating windows; the
source of the table in profiles/qk_norm_freqs.md.

    python tools/qk_norm_freqs_bench.py [--out FILE.json]     on a machine with the GPU and a built librfa_hip.so

q (1, 8192, 32, 128) + k (1, 8192, 8, 128) bf16, R = 128 halves, bf16 weights; single axis: the positions of rank 1 of a 4-rank
zigzag; three axes: Qwen3-VL's interleaved sections over random (t, h, w) below 2^20.  Forward and backward are timed apart, each
side through its public call (the fused side's direct backend calls too: `kernel`): the forwards under no_grad, the backwards
torch.autograd.grad over graphs built once per buffer set.  Per side: warm-up, then five windows of 20 calls, the sides
alternating; buffers rotate over four sets.  One JSON line per row and direction: the median window in us per call, every
side's (min, max) over its windows, and the ratios two_calls / fused and tables / fused."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    sys.path.insert(0, p)
import ring_flash_attn as R  # noqa: E402
from ring_flash_attn.backend import get_backend  # noqa: E402

dev = torch.device("cuda:0")
DT, EPS, W, RANK = torch.bfloat16, 1e-6, 4, 1
B, S, H, HK, D = 1, 8192, 32, 8, 128
NSETS, WINDOWS, CALLS = 4, 5, 20
QWEN3_VL = [0] * 64
QWEN3_VL[1:60:3] = [1] * 20
QWEN3_VL[2:60:3] = [2] * 20


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
    be = get_backend()
    gen = torch.Generator().manual_seed(5)
    inv = (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2))).float().to(dev)
    ang = torch.arange(W * S, dtype=torch.float64).view(-1, 1) * inv.double().cpu()
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    zz = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev)
    thw = torch.randint(0, 2 ** 20, (3, B, S), generator=gen).to(torch.int32).to(dev)
    wq, wk = ((1.0 + 0.25 * torch.randn(D, generator=gen)).to(DT).to(dev).requires_grad_(True) for _ in range(2))
    sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev).requires_grad_(True) for h in (H, HK)] for _ in range(NSETS)]
    douts = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(NSETS)]
    outs = [[torch.empty_like(t) for t in ts] for ts in sets]
    dws = [torch.empty(D, dtype=torch.float32, device=dev) for _ in range(2)]
    res = []
    for axes, pkw in (("one axis", dict(positions=zz)), ("three axes", dict(positions=thw, freq_axis=QWEN3_VL))):
        def fused(q, k):
            return R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv, eps=EPS, **pkw)

        def two_calls(q, k):
            return R.apply_rotary_freqs(*R.apply_qk_norm_rotary(q, k, wq, wk, eps=EPS), inv, **pkw)

        def tables(q, k):
            return R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin, positions=zz, eps=EPS)

        sides = dict(fused=fused, two_calls=two_calls)
        if "freq_axis" not in pkw:
            sides["tables"] = tables
        # once: the sides agree up to the two calls' extra rounding between norm and rotation
        with torch.no_grad():
            want = fused(*sets[0])
            for fn in sides.values():
                for x, y in zip(fn(*sets[0]), want):
                    assert bool(((x.float() - y.float()).abs() <= 2.0 ** -6 * y.float().abs() + 2.0 ** -5).all()), "the sides disagree"
        bkw = dict(eps=EPS, freq_axis=pkw.get("freq_axis"), positions=pkw["positions"])

        def fwd(fn):
            def run(i):
                with torch.no_grad():
                    fn(*sets[i % NSETS])
            return run

        def kernel_fwd(i):
            be.qk_norm_freqs_rotary_fwd([t.detach() for t in sets[i % NSETS]], outs[i % NSETS], [wq.detach(), wk.detach()], inv, **bkw)

        def kernel_bwd(i):
            be.qk_norm_freqs_rotary_bwd([t.detach() for t in sets[i % NSETS]], douts[i % NSETS], outs[i % NSETS],
                                        [wq.detach(), wk.detach()], dws, inv, **bkw)

        t_f = windows(dict({n: fwd(fn) for n, fn in sides.items()}, kernel=kernel_fwd))
        graphs = {n: [fn(*ts) for ts in sets] for n, fn in sides.items()}

        def bwd(name):
            def run(i):
                j = i % NSETS
                torch.autograd.grad(graphs[name][j], sets[j] + [wq, wk], douts[j], retain_graph=True)
            return run

        t_b = windows(dict({n: bwd(n) for n in sides}, kernel=kernel_bwd))
        for direction, times in (("forward", t_f), ("backward", t_b)):
            med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
            row = dict(shape=[B, S, H, HK, D], axes=axes, direction=direction,
                       **{f"{n}_us": round(v, 1) for n, v in med.items()},
                       **{f"{n}_spread": [round(min(v), 1), round(max(v), 1)] for n, v in times.items()},
                       two_calls_over_fused=round(med["two_calls"] / med["fused"], 2))
            if "tables" in med:
                row["tables_over_fused"] = round(med["tables"] / med["fused"], 2)
            res.append(row)
            print(json.dumps(row), flush=True)
        del graphs
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
