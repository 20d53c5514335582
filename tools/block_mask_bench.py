#!/usr/bin/env python3
"""Timings behind profiles/block_mask.md, on one MI355X: block-sparse masks (the kBlk kernel instances) beside the calls that
describe the same or a larger mask without them.

Shape: B 1, S 8192, H 32 / Hk 8, D 128, bf16; forward, and bwd_preprocess + backward.
  (a) the plain causal dense call, forced to the kernel forms a masked call runs (the 8 x 32 forward, the 7-GEMM dQ kernel, the
      128-key dK/dV kernel, no dS hand-off); measured again alone for its own spread;
  (b) the all-True mask, causal=True, beside (a): the price of the list walk where it skips nothing;
  (c) 8 documents of 1024 tokens as a block mask, causal=True, beside (a), beside the same mask through with_row_ranges'
      kernels, and beside the cu_seqlens call of the same documents (the library's own plan);
  (d) window + global + random blocks at about 1/8 density, causal=True, beside (a), with its lit-tile count.
The calls ALTERNATE batch by batch; device events around each batch; the median and the spread (min, max) over the batches.

Usage: python tools/block_mask_bench.py [--batches 15] [--per-batch 5] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ring-flash-attention_amd"))


def timed(fns, batches, per_batch):
    """(median, min, max) milliseconds per call of each fn: batches alternate between the fns"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(batches):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_batch):
                fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / per_batch)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def sparse_mask(N, seed=0):
    """window (the diagonal block and the one in front of it) + global (the first block) + random blocks, causal, at about 1/8
    of the N (N + 1) / 2 causal blocks"""
    g = torch.Generator().manual_seed(seed)
    r, c = torch.arange(N).view(-1, 1), torch.arange(N).view(1, -1)
    causal = c <= r
    m = ((r - c >= 0) & (r - c <= 1)) | (c == 0)
    want = causal.sum().item() // 8
    extra = max(0, want - int((m & causal).sum()))
    cand = (causal & ~m).flatten().nonzero().flatten()
    pick = cand[torch.randperm(len(cand), generator=g)[:extra]]
    m = m.flatten()
    m[pick] = True
    return (m.view(N, N) & causal).view(1, 1, N, N).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--per-batch", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from ring_flash_attn import config
    from ring_flash_attn.backend import get_backend

    be, dev = get_backend(), torch.device("cuda:0")
    B, S, H, Hk, D, ndoc = 1, 8192, 32, 8, 128, 8
    N = S // 128
    g = torch.Generator().manual_seed(0)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).bfloat16().to(dev)
    q, k, v, do = mk(H), mk(Hk), mk(Hk), mk(H)
    scale = D ** -0.5
    i = torch.arange(S, dtype=torch.int32)
    L = S // ndoc
    doc_rr = (i // L * L).view(1, S).contiguous().to(dev), ((i // L + 1) * L).view(1, S).contiguous().to(dev)
    blk = torch.arange(N) // (L // 128)
    m_doc = (blk.view(-1, 1) == blk.view(1, -1)).view(1, 1, N, N).contiguous().to(dev)
    m_all = torch.ones(1, 1, N, N, dtype=torch.bool, device=dev)
    m_sp_cpu = sparse_mask(N)
    m_sp = m_sp_cpu.to(dev)
    cu = torch.arange(0, S + 1, L, dtype=torch.int32, device=dev)
    tri = torch.tril(torch.ones(N, N, dtype=torch.bool))
    # 64-key tiles under causal: a diagonal block holds 3 of its 4 (forward / dQ: per 128 rows), a block below it all 4
    tiles = lambda m: int(4 * (m[0, 0] & tri).sum() - (m[0, 0].diagonal()).sum())

    def buffers():
        return (torch.empty_like(q), torch.empty(B, H, S, dtype=torch.float32, device=dev), torch.empty(B, H, S, dtype=torch.float32, device=dev),
                torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))

    def dense(kw, forced):
        out, lse, delta, dq, dk, dv = buffers()

        def fwd():
            with config.override(**forced):
                be.fwd(q, k, v, softmax_scale=scale, causal=True, out=out, lse=lse, **kw)

        def bwd():
            with config.override(**forced):
                be.bwd_preprocess(do, out, delta)
                be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=True, dq=dq, dk=dk, dv=dv, **kw)

        return fwd, bwd, (out, lse, dq, dk, dv)

    def packed():
        pq, pk, pv, pdo = q[0], k[0], v[0], do[0]
        out, lse, delta = torch.empty_like(pq), torch.empty(H, S, dtype=torch.float32, device=dev), torch.empty(H, S, dtype=torch.float32, device=dev)
        dq, dk, dv = torch.empty_like(pq), torch.empty_like(pk), torch.empty_like(pv)
        kw = dict(softmax_scale=scale, causal=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=L, max_seqlen_k=L)

        def fwd():
            be.fwd(pq, pk, pv, out=out, lse=lse, **kw)

        def bwd():
            be.bwd_preprocess(pdo, out, delta, cu_seqlens_q=cu, max_seqlen_q=L)
            be.bwd(pdo, pq, pk, pv, lse, delta, dq=dq, dk=dk, dv=dv, **kw)

        return fwd, bwd, (out, lse, dq, dk, dv)

    forced = dict(fwd_form="8x32", fwd_kv_nsplit=1, dkdv_wide=0, bwd_ds_spill=False)
    calls = {"causal_forced": dense({}, forced), "all_true": dense({"block_mask": (m_all, 0)}, {}),
             "doc_block_mask": dense({"block_mask": (m_doc, 0)}, {}), "doc_row_ranges": dense({"row_ranges": (*doc_rr, 0)}, {}),
             "doc_cu_seqlens": packed(), "sparse_block_mask": dense({"block_mask": (m_sp, 0)}, {})}
    for f, b, _ in calls.values():
        f()
        b()
    torch.cuda.synchronize()
    diff = lambda x, y: max((s.float() - t.float()).abs().max().item() for s, t in zip(x, y))
    agree = dict(all_true_vs_causal=diff(calls["all_true"][2], calls["causal_forced"][2]),
                 doc_vs_row_ranges=diff(calls["doc_block_mask"][2], calls["doc_row_ranges"][2]),
                 doc_vs_cu_seqlens=max((x[0].float() - y.float()).abs().max().item() for x, y in zip(calls["doc_block_mask"][2], calls["doc_cu_seqlens"][2])))
    names, fns = [], []
    for n, (f, b, _) in calls.items():
        names += ["fwd_" + n, "bwd_" + n]
        fns += [f, b]
    res = dict(zip(names, timed(fns, a.batches, a.per_batch)))
    res.update(zip(("fwd_causal_forced_again", "bwd_causal_forced_again"), timed(list(calls["causal_forced"][:2]), a.batches, a.per_batch)))
    med = {n: t[0] for n, t in res.items()}
    total = lambda tag: med["fwd_" + tag] + med["bwd_" + tag]
    ratio = lambda x, y: dict(sum=round(total(x) / total(y), 4), fwd=round(med["fwd_" + x] / med["fwd_" + y], 4),
                              bwd=round(med["bwd_" + x] / med["bwd_" + y], 4))
    ratios = dict(all_true_over_causal_forced=ratio("all_true", "causal_forced"),
                  doc_over_causal_forced=ratio("doc_block_mask", "causal_forced"),
                  doc_over_row_ranges=ratio("doc_block_mask", "doc_row_ranges"),
                  doc_over_cu_seqlens=ratio("doc_block_mask", "doc_cu_seqlens"),
                  sparse_over_causal_forced=ratio("sparse_block_mask", "causal_forced"))
    lit = dict(causal_tiles=tiles(torch.ones(1, 1, N, N, dtype=torch.bool)), doc_tiles=tiles(m_doc.cpu()), sparse_tiles=tiles(m_sp_cpu),
               sparse_blocks=int((m_sp_cpu[0, 0] & tri).sum()), causal_blocks=int(tri.sum()))
    print(f"B {B} S {S} H {H} / Hk {Hk} D {D} bf16, {ndoc} documents of {L}")
    for n, t in res.items():
        print(f"  {n:26s} median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})")
    print("  ratios (medians):", json.dumps(ratios))
    print("  lit 64-key tiles per query-block row set:", lit)
    print("  max |difference|:", agree)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, S=S, H=H, Hk=Hk, D=D, dtype="bf16", documents=ndoc),
                           ms={n: dict(median=round(t[0], 4), min=round(t[1], 4), max=round(t[2], 4)) for n, t in res.items()},
                           ratios=ratios, lit=lit, agree=agree), f, indent=1)
    assert ratios["doc_over_causal_forced"]["sum"] < 1.0, "the document mask must be faster than the causal call it is one eighth of"


if __name__ == "__main__":
    main()
