"""Kernel time of the rotary embedding (csrc/rfa_rotary.hip, backend.rotary) beside the torch composite it replaces — same
device, same process, alternating windows; the source of the table in profiles/rotary.md.

    python tools/rotary_bench.py [--out FILE.json]      on a machine with the GPU and a built librfa_hip.so
    python tools/rotary_bench.py --rehearse             tiny shapes on the CPU against tests/_rotary_backend.torch_rotary, no timing

q (1, 8192, 32, 128) + k (1, 8192, 8, 128), bf16, R = 128 (halves), fp32 tables of 4 x 8192 positions, the zigzag map of rank 1
of 4; in place and out of place, forward and conjugate, q and k in ONE launch.  The composite does the same job in torch:
cos / sin indexed by local_positions (built once, outside the timing), the rotate_half formulation, fp32 arithmetic, one
rounding to bf16, for q and for k.  Per configuration: the composite's result is checked against the kernel's (one bf16 step:
torch does not fuse the two products), both are warmed up, then five windows of 40 calls per side are timed with device events,
the two sides alternating; buffers rotate over six sets (6 x 84 MB of q and k do not sit in the 256 MB cache).  One JSON line per
configuration: the median window in us per call, the bytes the algorithm needs (q and k read once and written once) over it,
the ratio composite / kernel, and the spread (min, max) over the five windows."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import _rotary_backend as RB  # noqa: E402
from ring_flash_attn import local_positions, zigzag_ring_flash_attn_func  # noqa: E402
from ring_flash_attn._common import zigzag_map  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
dev = torch.device("cpu" if REHEARSE else "cuda:0")
B, S, H, HK, D, W, RANK = (1, 8, 4, 2, 32, 4, 1) if REHEARSE else (1, 8192, 32, 8, 128, 4, 1)
DT = torch.bfloat16


def rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat([-x2, x1], dim=-1)


def composite(tensors, cos_rows, sin_rows, conj):
    """cos_rows / sin_rows: (S, 1, D) fp32, the tables already gathered by position and repeated over the two halves"""
    s = -sin_rows if conj else sin_rows
    outs = []
    for x in tensors:
        xf = x.float()
        outs.append((xf * cos_rows + rotate_half(xf) * s).to(x.dtype))
    return outs


def main():
    if REHEARSE:
        fused = lambda srcs, dsts, cos, sin, **kw: RB.torch_rotary(srcs, dsts, cos, sin, **kw)
    else:
        from ring_flash_attn.backend import get_backend
        fused = get_backend().rotary
    gen = torch.Generator().manual_seed(5)
    P = W * S
    ang = torch.arange(P, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2)))
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    pm = zigzag_map(RANK, W, S // 2)
    pos = local_positions(zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev).long()
    cos_rows = torch.cat([cos[pos], cos[pos]], dim=-1).unsqueeze(1)             # (S, 1, D): what a model caches per step
    sin_rows = torch.cat([sin[pos], sin[pos]], dim=-1).unsqueeze(1)
    nsets = 1 if REHEARSE else 6                       # rotate buffers: 6 x 84 MB of inputs do not sit in the 256 MB cache
    sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(nsets)]
    outs = [[torch.empty_like(t) for t in ts] for ts in sets]
    nbytes = 2 * sum(t.numel() for t in sets[0]) * 2                            # read once + written once, 2 bytes each
    res = []
    for conj in (False, True):
        for inplace in (False, True):
            # once: the composite produces what the kernel produces, up to the step of one differently rounded product
            srcs = [t.clone() for t in sets[0]]
            dsts = srcs if inplace else [torch.empty_like(t) for t in srcs]
            fused(srcs, dsts, cos, sin, pos_map=pm, conj=conj)
            for got, want in zip(dsts, composite(sets[0], cos_rows, sin_rows, conj)):
                err = (got.float() - want.float()).abs()
                assert bool((err <= 2.0 ** -7 * want.float().abs() + 1e-6).all()), ("composite and kernel disagree", conj, inplace)
            if REHEARSE:
                continue
            times = {"fused": [], "torch": []}

            def run(which, i):
                ts = sets[i % nsets]
                if which == "torch":
                    composite(ts, cos_rows, sin_rows, conj)
                else:
                    fused(ts, ts if inplace else outs[i % nsets], cos, sin, pos_map=pm, conj=conj)

            for which in ("fused", "torch"):
                for i in range(8):
                    run(which, i)
            torch.cuda.synchronize()
            for rep in range(5):                                               # alternate the two, 40 calls per window
                for which in ("fused", "torch"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(40):
                        run(which, i)
                    e1.record()
                    e1.synchronize()
                    times[which].append(e0.elapsed_time(e1) / 40 * 1e3)         # us per call
            f, t = sorted(times["fused"])[2], sorted(times["torch"])[2]
            row = dict(direction="conjugate" if conj else "forward", inplace=inplace, MB=nbytes / 1e6, fused_us=round(f, 1),
                       torch_us=round(t, 1), fused_TBps=round(nbytes / f / 1e6, 2), torch_TBps=round(nbytes / t / 1e6, 2),
                       ratio=round(t / f, 2), fused_spread=[round(min(times["fused"]), 1), round(max(times["fused"]), 1)],
                       torch_spread=[round(min(times["torch"]), 1), round(max(times["torch"]), 1)])
            res.append(row)
            print(json.dumps(row), flush=True)
    if REHEARSE:
        print("rehearsal ok")
        return
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
