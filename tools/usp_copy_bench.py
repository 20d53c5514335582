"""Kernel time of the four sequence/head copy ops (csrc/rfa_seqhead.hip, backend.seq_head_copy) beside the torch composite they
replace — same device, same process, alternating windows; the source of the table in profiles/usp.md.

    python tools/usp_copy_bench.py [--out FILE.json]      on a machine with the GPU and a built librfa_hip.so
    python tools/usp_copy_bench.py --rehearse             tiny shapes on the CPU against tests/_usp_backend.torch_copy, no timing

B 1, S 8192 rows per rank, H 32 / Hk 8, D 128, bf16, q | k | v in ONE launch; U = 2, 4, 8; every layout and op.  Per
configuration: the composite's result is checked equal to the kernel's, both are warmed up, then five windows of 40 calls per
side are timed with device events, the two sides alternating; buffers rotate over four sets so that a call's 201 MB are not
cache-resident.  One JSON line per configuration: the median window in us per call, bytes moved (every element read once and
written once) over it, the ratio composite / kernel, and the spread (min, max) over the five windows."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import _usp_backend as UB  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
dev = torch.device("cpu" if REHEARSE else "cuda:0")
B, S, H, HK, D = (1, 8, 8, 8, 16) if REHEARSE else (1, 8192, 32, 8, 128)
DT = torch.bfloat16


def rows_to_merged(x, layout, U):
    """x (U, B, S, Hs, D) -> merged (B, U*S, Hs, D), contiguous copy"""
    _, b, s, hs, d = x.shape
    if layout == UB.CONTIGUOUS:
        return x.permute(1, 0, 2, 3, 4).reshape(b, U * s, hs, d)
    if layout == UB.STRIPE:
        return x.permute(1, 2, 0, 3, 4).reshape(b, s * U, hs, d)
    c = s // 2
    front = x[:, :, :c].permute(1, 0, 2, 3, 4).reshape(b, U * c, hs, d)
    back = x[:, :, c:].flip(0).permute(1, 0, 2, 3, 4).reshape(b, U * c, hs, d)
    return torch.cat([front, back], 1)


def merged_to_rows(m, layout, U):
    """inverse: merged (B, U*S, Hs, D) -> (U, B, S, Hs, D) contiguous"""
    b, us, hs, d = m.shape
    s = us // U
    if layout == UB.CONTIGUOUS:
        return m.view(b, U, s, hs, d).permute(1, 0, 2, 3, 4).contiguous()
    if layout == UB.STRIPE:
        return m.view(b, s, U, hs, d).permute(2, 0, 1, 3, 4).contiguous()
    c = s // 2
    front = m[:, :U * c].view(b, U, c, hs, d).permute(1, 0, 2, 3, 4)
    back = m[:, U * c:].view(b, U, c, hs, d).permute(1, 0, 2, 3, 4).flip(0)
    return torch.cat([front, back], 2)


def composite(op, layout, U, tensors, slots):
    """the torch ops the fused launch replaces; returns what it produced (slots for the two packing ops, else the tensors)"""
    if op in (UB.PACK, UB.MERGED_TO_SLOTS):
        parts = []
        for t in tensors:
            if op == UB.PACK:
                b, s, h, d = t.shape
                x = t.view(b, s, U, h // U, d).permute(2, 0, 1, 3, 4).contiguous()
            else:
                x = merged_to_rows(t, layout, U)
            parts.append(x.view(U, -1))
        return torch.cat(parts, 1).view(-1)
    outs, base = [], 0
    buf = slots.view(U, -1)
    for t in tensors:
        n = t.numel() // U
        if op == UB.UNPACK:
            b, us, hs, d = t.shape
            x = buf[:, base:base + n].view(U, b, us // U, hs, d)
            outs.append(rows_to_merged(x, layout, U).contiguous())
        else:
            b, s, h, d = t.shape
            x = buf[:, base:base + n].view(U, b, s, h // U, d)
            outs.append(x.permute(1, 2, 0, 3, 4).reshape(b, s, h, d))
        base += n
    return outs


def main():
    if REHEARSE:
        fused = UB.torch_copy
    else:
        from ring_flash_attn.backend import get_backend
        fused = get_backend().seq_head_copy
    gen = torch.Generator().manual_seed(5)
    res = []
    nsets = 1 if REHEARSE else 4                       # rotate buffers: 4 x 200 MB per op does not sit in the 256 MB cache
    for layout_name, layout in (("contiguous", UB.CONTIGUOUS), ("zigzag", UB.ZIGZAG), ("stripe", UB.STRIPE)):
        for U in (2, 4, 8):
            for op_name, op in (("pack", UB.PACK), ("unpack", UB.UNPACK), ("merged_to_slots", UB.MERGED_TO_SLOTS),
                                ("slots_to_heads", UB.SLOTS_TO_HEADS)):
                local = op in (UB.PACK, UB.SLOTS_TO_HEADS)
                shape = lambda h: (B, S, h, D) if local else (B, U * S, h // U, D)
                sets = []
                for _ in range(nsets):
                    ts = [torch.randn(shape(h), generator=gen).to(DT).to(dev) for h in (H, HK, HK)]
                    n = sum(t.numel() for t in ts)
                    sets.append((ts, torch.randn(n, generator=gen).to(DT).to(dev)))
                # once: the composite produces what the fused launch produces
                ts, slots = sets[0]
                if op in (UB.PACK, UB.MERGED_TO_SLOTS):
                    got = torch.empty_like(slots)
                    fused(op, layout, U, ts, got)
                    assert torch.equal(got, composite(op, layout, U, ts, slots)), (layout_name, U, op_name)
                else:
                    got = [torch.empty_like(t) for t in ts]
                    fused(op, layout, U, got, slots)
                    assert all(torch.equal(a, b) for a, b in zip(got, composite(op, layout, U, ts, slots))), (layout_name, U, op_name)
                if REHEARSE:
                    continue
                nbytes = 2 * n * 2                      # every element read once and written once, 2 bytes each
                times = {"fused": [], "torch": []}
                outs = [torch.empty_like(slots) if op in (UB.PACK, UB.MERGED_TO_SLOTS) else [torch.empty_like(t) for t in ts]
                        for _ in range(nsets)]

                def run(which, i):
                    ts, slots = sets[i % nsets]
                    if which == "torch":
                        composite(op, layout, U, ts, slots)
                    elif op in (UB.PACK, UB.MERGED_TO_SLOTS):
                        fused(op, layout, U, ts, outs[i % nsets])
                    else:
                        fused(op, layout, U, outs[i % nsets], slots)

                for which in ("fused", "torch"):
                    for i in range(8):
                        run(which, i)
                torch.cuda.synchronize()
                for rep in range(5):                    # alternate the two, 40 calls per window
                    for which in ("fused", "torch"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(40):
                            run(which, i)
                        e1.record()
                        e1.synchronize()
                        times[which].append(e0.elapsed_time(e1) / 40 * 1e3)     # us per call
                f, t = sorted(times["fused"])[2], sorted(times["torch"])[2]
                row = dict(layout=layout_name, U=U, op=op_name, MB=nbytes / 1e6, fused_us=round(f, 1), torch_us=round(t, 1),
                           fused_TBps=round(nbytes / f / 1e6, 2), torch_TBps=round(nbytes / t / 1e6, 2), ratio=round(t / f, 2),
                           fused_spread=[round(min(times["fused"]), 1), round(max(times["fused"]), 1)],
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
