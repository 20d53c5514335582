"""What a sliding window buys a contiguous ring: forward + backward time of ONE rank's whole ring (virtual ring — the
exchange looped back inside one process, as tools/profile_virtual_step.py does) at the headline shape, S = 8192 rows
per rank, 32 / 8 heads, head dim 128, bf16, W = 8 virtual ranks, for several window_left values beside the unwindowed
causal ring; with the block calls, K/V hops and K/V bytes a rank exchanges.  Prints a markdown table.

usage: window_ring.py [--world 8] [--rank 7] [--seq 8192] [--iters 5] [--windows 1024,4096,8192,16384,-1]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ring-flash-attention_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=-1, help="virtual rank (default: the last, which computes the most)")
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", default="1024,4096,8192,16384,-1")
    a = ap.parse_args()
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29579")
    dist.init_process_group("gloo", rank=0, world_size=1)
    import ring_flash_attn as R
    from ring_flash_attn import _testing, utils
    from ring_flash_attn.backend import get_backend

    W, S, H, Hk, D = a.world, a.seq, 32, 8, 128
    rank = a.rank if a.rank >= 0 else W - 1
    dev = torch.device("cuda:0")
    q = torch.randn(1, S, H, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    kv = torch.randn(1, S, 2, Hk, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn_like(q)
    _testing.set_loopback((rank, W))
    be = get_backend()
    counts = {"fwd": 0, "bwd": 0, "hops": 0, "bytes": 0}
    fwd0, bwd0, commit0, sr0 = be.fwd, be.bwd, utils.RingComm.commit, utils.RingComm.send_recv

    def fwd(*x, **kw):
        counts["fwd"] += 1
        return fwd0(*x, **kw)

    def bwd(*x, **kw):
        if not (kw.get("phases", 0) & 2) or (kw.get("phases", 0) & 1):
            counts["bwd"] += 1
        return bwd0(*x, **kw)

    def commit(self):
        counts["hops"] += 1
        return commit0(self)

    def send_recv(self, t, *x, **kw):
        counts["bytes"] += t.numel() * t.element_size()
        return sr0(self, t, *x, **kw)

    be.fwd, be.bwd, utils.RingComm.commit, utils.RingComm.send_recv = fwd, bwd, commit, send_recv

    def step(window):
        q.grad = kv.grad = None
        R.ring_flash_attn_kvpacked_func(q, kv, causal=True, window_size=window).backward(do)

    print(f"virtual ring: W = {W}, rank {rank}, S = {S} rows per rank, H {H} / Hk {Hk}, D {D}, bf16, causal; "
          f"device {torch.cuda.get_device_name(0)}, library {get_backend().lib.rfa_build_id().decode()}")
    print("| window_left | fwd+bwd ms (median) | min ms | block calls fwd / bwd | exchanges fwd+bwd | bytes sent per rank (MB) |")
    print("|---|---|---|---|---|---|")
    for w in [int(x) for x in a.windows.split(",")]:
        window = (w, 0) if w >= 0 else (-1, -1)
        for _ in range(2):
            step(window)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            for k_ in counts:
                counts[k_] = 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(window)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        print(f"| {'unbounded' if w < 0 else w} | {times[len(times) // 2]:.3f} | {times[0]:.3f} | {counts['fwd']} / {counts['bwd']} | "
              f"{counts['hops']} | {counts['bytes'] / 1e6:.1f} |", flush=True)


if __name__ == "__main__":
    main()
