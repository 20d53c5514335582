"""What a sliding window buys a packed (varlen) ring in COMPUTE: forward + backward time of ONE rank's whole
`ring_flash_attn_varlen` block sequence (virtual ring — the exchange looped back inside one process, so the block calls a
rank of W = 8 would issue are replayed locally with mask_shift_lens = 0 .. rank) at the varlen benchmark's shape: 8192
packed tokens per rank, 32 / 8 heads, head dim 128, bf16, the benchmark's 4 cu_seqlens patterns, for several window_left
values beside the unwindowed causal ring.  The exchange is a full rotation in every row (the traffic does not follow the
window for packed input); the times are compute + launch + local copies.  Prints a markdown table.

usage: window_varlen.py [--world 8] [--rank 7] [--iters 5] [--windows 1024,4096,-1]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ring-flash-attention_amd"))

# local cu_seqlens patterns of the varlen benchmark (bench.py: VARLEN_PATTERNS)
PATTERNS = [[0, 8192], [0, 256, 7648, 8192], [0, 4096, 8192], [0, 3104, 6304, 7904, 8064, 8192]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=-1, help="virtual rank (default: the last, which computes the most)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", default="1024,4096,-1")
    a = ap.parse_args()
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29581")
    dist.init_process_group("gloo", rank=0, world_size=1)
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from ring_flash_attn.backend import get_backend

    W, T, H, Hk, D = a.world, 8192, 32, 8, 128
    rank = a.rank if a.rank >= 0 else W - 1
    dev = torch.device("cuda:0")
    q = torch.randn(T, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    kv = torch.randn(T, 2, Hk, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn_like(q)
    _testing.set_loopback((rank, W))
    be = get_backend()
    shifts = []
    fwd0 = be.fwd

    def fwd(*x, **kw):
        shifts.append(kw.get("mask_shift_lens", 0))
        return fwd0(*x, **kw)

    be.fwd = fwd
    cus = [torch.tensor(p, dtype=torch.int32, device=dev) for p in PATTERNS]
    mxs = [max(y - x for x, y in zip(p[:-1], p[1:])) for p in PATTERNS]

    def step(window, n):
        q.grad = kv.grad = None
        R.ring_flash_attn_varlen_kvpacked_func(q, kv, cus[n], mxs[n], causal=True, window_size=window).backward(do)

    print(f"virtual varlen ring: W = {W}, rank {rank}, {T} packed rows per rank, H {H} / Hk {Hk}, D {D}, bf16, causal; "
          f"device {torch.cuda.get_device_name(0)}, library {get_backend().lib.rfa_build_id().decode()}")
    print("| window_left | local cu_seqlens | fwd+bwd ms (median) | min ms | mask_shift_lens of the forward's block calls |")
    print("|---|---|---|---|---|")
    for w in [int(x) for x in a.windows.split(",")]:
        window = (w, 0) if w >= 0 else (-1, -1)
        for n, p in enumerate(PATTERNS):
            for _ in range(2):
                step(window, n)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.iters):
                del shifts[:]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(window, n)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            times.sort()
            print(f"| {'unbounded' if w < 0 else w} | {p} | {times[len(times) // 2]:.3f} | {times[0]:.3f} | {shifts} |", flush=True)


if __name__ == "__main__":
    main()
