"""Time of MLA's k / v assembly fused with a rotary embedding whose angles the kernel forms (csrc/rfa_mlaropefreq.hip,
ring_flash_attn.apply_mla_rotary_freqs) beside the table kernels of apply_mla_rotary and beside the torch composite it replaces —
same device, same process, alternating windows; the source of the table in profiles/mla_rotary_freqs.md.

    python tools/mla_rotary_freqs_bench.py [--out FILE.json]      on a machine with the GPU and a built librfa_hip.so

tools/mla_rotary_bench.py's shapes: q (1, 8192, 128, 192), kv (1, 8192, 128, 256), k_pe a column slice of (1, 8192, 576), bf16,
Dn = 128, Dr = 64, Dv = 128, the positions of rank 1 of a 4-rank zigzag, attention_scaling = 0.1 ln 40 + 1; fp32 tables of
4 x 8192 positions for the table kernels.  Rows:
  fwd_kernel / bwd_kernel              HipBackend.mla_rotary_freqs_fwd / _bwd into preallocated outputs (the map's four numbers)
  fwd_table_kernel / bwd_table_kernel  HipBackend.mla_rotary_fwd / _bwd, the same
  fwd_call / fwd_bwd_call              apply_mla_rotary_freqs with its allocations, and with torch.autograd.grad of all three inputs
  fwd_torch / fwd_bwd_torch            the composite: apply_rotary_freqs on q's slice and on k_pe, expand, cat, contiguous — and
                                       autograd through it
Every side is warmed up, then five windows of 10 calls per row are timed with device events, the rows alternating inside a
repetition.  One call moves 2 GB, eight times the 256 MB cache: the buffers are not rotated.  One JSON line per row: the median
window in us per call, the bytes the algorithm needs (every input read once, every output written once) over it, and the spread
(min, max) over the five windows."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd")):
    sys.path.insert(0, p)
from ring_flash_attn import apply_mla_rotary_freqs, apply_rotary_freqs, local_positions, zigzag_ring_flash_attn_func  # noqa: E402
from ring_flash_attn._common import zigzag_map  # noqa: E402
from ring_flash_attn.backend import get_backend  # noqa: E402

dev = torch.device("cuda:0")
B, S, H, DN, DR, DV, W, RANK = 1, 8192, 128, 128, 64, 128, 4, 1
DT, SCALING = torch.bfloat16, 0.1 * math.log(40) + 1


def composite(q, kv, k_pe, inv_freq, pos):
    qo = apply_rotary_freqs(q, None, inv_freq, attention_scaling=SCALING, positions=pos, rot_offset=DN)
    pe = apply_rotary_freqs(k_pe.unsqueeze(2), None, inv_freq, attention_scaling=SCALING, positions=pos)
    return qo, torch.cat([kv[..., :DN], pe.expand(-1, -1, H, -1)], -1), kv[..., DN:].contiguous()


def main():
    be = get_backend()
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float32).to(DT).to(dev)
    freq = 10000.0 ** (-torch.arange(DR // 2, dtype=torch.float64) / (DR // 2))
    inv_freq = freq.float().to(dev)
    ang = torch.arange(W * S, dtype=torch.float64).view(-1, 1) * freq
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    pm = zigzag_map(RANK, W, S // 2)
    pos = local_positions(zigzag_ring_flash_attn_func, S, rank=RANK, world_size=W, device=dev)
    q, kv, k_pe = rand(B, S, H, DN + DR), rand(B, S, H, DN + DV), rand(B, S, 576)[..., 512:]
    outs = [torch.empty(B, S, H, DN + DR, dtype=DT, device=dev), torch.empty(B, S, H, DN + DR, dtype=DT, device=dev),
            torch.empty(B, S, H, DV, dtype=DT, device=dev)]
    grads = [rand(*t.shape) for t in outs]
    dins = [torch.empty_like(q), torch.empty_like(kv), torch.empty(B, S, DR, dtype=DT, device=dev)]
    leaves = [t.detach().requires_grad_(True) for t in (q, kv, k_pe)]
    call = lambda *t: apply_mla_rotary_freqs(*t, inv_freq, attention_scaling=SCALING, positions=pos)
    # once: the composite produces the fused call's bits, forward and backward
    want, got = composite(*leaves, inv_freq, pos), call(*leaves)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    gw, gg = torch.autograd.grad(want, leaves, grads), torch.autograd.grad(got, leaves, grads)
    assert torch.equal(gw[0], gg[0]) and torch.equal(gw[1], gg[1])
    print(json.dumps(dict(dk_pe_max_abs_diff_vs_torch=(gw[2].float() - gg[2].float()).abs().max().item())), flush=True)
    del want, got, gw, gg
    elems = lambda ts: 2 * sum(t.numel() for t in ts)
    fwd_bytes, bwd_bytes = elems([q, kv, k_pe] + outs), elems(grads + dins)
    fkw, tkw = dict(nope_dim=DN, scaling=SCALING, pos_map=pm), dict(nope_dim=DN, pos_map=pm)
    rows = {
        "fwd_kernel": (fwd_bytes, lambda: be.mla_rotary_freqs_fwd(q, outs[0], kv, k_pe, outs[1], outs[2], inv_freq, **fkw)),
        "fwd_table_kernel": (fwd_bytes, lambda: be.mla_rotary_fwd(q, outs[0], kv, k_pe, outs[1], outs[2], cos, sin, **tkw)),
        "bwd_kernel": (bwd_bytes, lambda: be.mla_rotary_freqs_bwd(grads[0], dins[0], grads[1], grads[2], dins[1], dins[2], inv_freq,
                                                                  v_dim=DV, heads=H, **fkw)),
        "bwd_table_kernel": (bwd_bytes, lambda: be.mla_rotary_bwd(grads[0], dins[0], grads[1], grads[2], dins[1], dins[2], cos, sin,
                                                                  v_dim=DV, heads=H, **tkw)),
        "fwd_call": (fwd_bytes, lambda: call(q, kv, k_pe)),
        "fwd_torch": (fwd_bytes, lambda: composite(q, kv, k_pe, inv_freq, pos)),
        "fwd_bwd_call": (fwd_bytes + bwd_bytes, lambda: torch.autograd.grad(call(*leaves), leaves, grads)),
        "fwd_bwd_torch": (fwd_bytes + bwd_bytes, lambda: torch.autograd.grad(composite(*leaves, inv_freq, pos), leaves, grads)),
    }
    times = {name: [] for name in rows}
    for _, fn in rows.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for rep in range(5):
        for name, (_, fn) in rows.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / 10 * 1e3)                  # us per call
    res = []
    for name, (nbytes, _) in rows.items():
        t = sorted(times[name])
        res.append(dict(row=name, MB=round(nbytes / 1e6, 1), us=round(t[2], 1), TBps=round(nbytes / t[2] / 1e6, 2),
                        spread=[round(t[0], 1), round(t[-1], 1)]))
        print(json.dumps(res[-1]), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
