"""Kernel time of the rotary embedding that forms its own angles (csrc/rfa_rotfreq.hip, backend.rotary_freqs) beside the table
kernel (csrc/rfa_rotary.hip, backend.rotary, fp32 tables) and, for M-RoPE, beside the torch composite it replaces — same device,
same process, alternating windows; the source of the table in profiles/rotary_freqs.md.

    python tools/rotary_freqs_bench.py [--out FILE.json]      on a machine with the GPU and a built librfa_hip.so
    python tools/rotary_freqs_bench.py --rehearse             tiny shapes on the CPU: the composite and the bookkeeping, no kernel

q (1, 8192, 32, 128) + k (1, 8192, 8, 128), bf16, R = 128 (halves), q and k in ONE launch.
  single axis   the zigzag map of rank 1 of 4, out of place and in place: rotary_freqs (inv_freq) against rotary (fp32 tables of
                4 x 8192 positions)
  M-RoPE        (3, 1, 8192) positions, Qwen2-VL's sections [16, 24, 24], out of place: rotary_freqs against the composite as
                Hugging Face writes it — inv_freq x positions per axis, cos / sin, the sections picked, rotate_half in fp32, one
                rounding — once with the cos / sin tensors built inside the timing (what a step does) and once with them cached
Both sides are warmed up, then five windows of 40 calls per side are timed with device events, the sides alternating; buffers
rotate over six sets (6 x 84 MB of q and k do not sit in the 256 MB cache).  One JSON line per configuration: the median window
in us per call, the bytes the algorithm needs (q and k read once and written once) over it, and the spread (min, max)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    sys.path.insert(0, p)
from ring_flash_attn._common import zigzag_map  # noqa: E402

REHEARSE = "--rehearse" in sys.argv
dev = torch.device("cpu" if REHEARSE else "cuda:0")
B, S, H, HK, D, W, RANK = (1, 8, 4, 2, 32, 4, 1) if REHEARSE else (1, 8192, 32, 8, 128, 4, 1)
SECTIONS = [4, 6, 6] if REHEARSE else [16, 24, 24]
DT = torch.bfloat16


def rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat([-x2, x1], dim=-1)


def mrope_cos_sin(inv_freq, pos):
    """(B, S, 1, D) fp32 cos / sin from (3, B, S) positions: every section of frequencies from its axis, repeated over the halves"""
    ang = pos.float().unsqueeze(-1) * inv_freq                                  # (3, B, S, D/2)
    ang = torch.cat([a[i % 3] for i, a in enumerate(ang.split(SECTIONS, dim=-1))], dim=-1)
    emb = torch.cat([ang, ang], dim=-1).unsqueeze(2)
    return emb.cos(), emb.sin()


def composite(tensors, cos, sin):
    return [(x.float() * cos + rotate_half(x.float()) * sin).to(x.dtype) for x in tensors]


def timed(sides):
    """sides: name -> callable(i); five alternating windows of 40 calls each; name -> (median, min, max) in us per call"""
    for fn in sides.values():
        for i in range(8):
            fn(i)
    torch.cuda.synchronize()
    times = {n: [] for n in sides}
    for rep in range(5):
        for n, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(40):
                fn(i)
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / 40 * 1e3)
    return {n: (sorted(t)[2], min(t), max(t)) for n, t in times.items()}


def main():
    gen = torch.Generator().manual_seed(5)
    inv_freq = (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2))).float().to(dev)
    ang = torch.arange(W * S, dtype=torch.float64).view(-1, 1) * inv_freq.double().cpu()
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    pm = zigzag_map(RANK, W, S // 2)
    axes = [i % 3 for i, n in enumerate(SECTIONS) for _ in range(n)]
    pos3 = torch.randint(0, W * S, (3, B, S), generator=gen).to(torch.int32).to(dev)
    nsets = 1 if REHEARSE else 6
    sets = [[torch.randn(B, S, h, D, generator=gen).to(DT).to(dev) for h in (H, HK)] for _ in range(nsets)]
    outs = [[torch.empty_like(t) for t in ts] for ts in sets]
    nbytes = 2 * sum(t.numel() for t in sets[0]) * 2
    c3, s3 = mrope_cos_sin(inv_freq, pos3)
    want = composite(sets[0], c3, s3)
    if REHEARSE:
        assert want[0].shape == sets[0][0].shape and len(axes) == D // 2 and c3.shape == (B, S, 1, D)
        print("rehearsal ok")
        return
    from ring_flash_attn.backend import get_backend
    be = get_backend()
    # once: the M-RoPE kernel produces what the composite produces, up to the step of one differently rounded product
    got = [torch.empty_like(t) for t in sets[0]]
    be.rotary_freqs(sets[0], got, inv_freq, freq_axis=axes, positions=pos3)
    for g, w in zip(got, want):
        assert bool(((g.float() - w.float()).abs() <= 2.0 ** -7 * w.float().abs() + 1e-5).all()), "composite and kernel disagree"
    res = []

    def report(name, t, base):
        row = dict(config=name, MB=nbytes / 1e6)
        for n, (med, lo, hi) in t.items():
            row[n + "_us"], row[n + "_TBps"], row[n + "_spread"] = round(med, 1), round(nbytes / med / 1e6, 2), [round(lo, 1), round(hi, 1)]
        row["ratio"] = round(t[base][0] / t["freqs"][0], 3)
        res.append(row)
        print(json.dumps(row), flush=True)

    for inplace in (False, True):
        dst = lambda i: sets[i % nsets] if inplace else outs[i % nsets]
        t = timed({"freqs": lambda i: be.rotary_freqs(sets[i % nsets], dst(i), inv_freq, pos_map=pm),
                   "tables": lambda i: be.rotary(sets[i % nsets], dst(i), cos, sin, pos_map=pm)})
        report("single axis, zigzag map, " + ("in place" if inplace else "out of place"), t, "tables")
    t = timed({"freqs": lambda i: be.rotary_freqs(sets[i % nsets], outs[i % nsets], inv_freq, freq_axis=axes, positions=pos3),
               "torch": lambda i: composite(sets[i % nsets], *mrope_cos_sin(inv_freq, pos3)),
               "torch_cached": lambda i: composite(sets[i % nsets], c3, s3)})
    report("M-RoPE [16, 24, 24], out of place", t, "torch")
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
