#!/usr/bin/env python3
"""Timings behind profiles/row_ranges.md, on one MI355X: per-row key ranges (the kRng kernel instances) beside the calls that
describe the same or a larger mask without them.

Shape: B 1, S 8192, H 32 / Hk 8, D 128, bf16; forward, and bwd_preprocess + backward.
  documents   the ranged call describes 8 documents of 1024 tokens, causal=True, beside
                (a) the plain causal dense call of that shape, forced to the same kernel forms (the 8 x 32 forward, the 7-GEMM dQ
                    kernel, the 128-key dK/dV kernel, no dS hand-off) — eight times the score work;
                (b) the cu_seqlens call of the same documents, with the library's own plan;
  causal      ranges that spell plain causal (start = 0, end = i + 1, causal=False) beside (a): the price of the per-lane
              predicates and of the tile-bounds pre-kernel.
The calls ALTERNATE batch by batch; device events around each batch; the median and the spread (min, max) over the batches.

Usage: python tools/row_ranges_bench.py [--batches 15] [--per-batch 5] [--json FILE]"""
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
    g = torch.Generator().manual_seed(0)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).bfloat16().to(dev)
    q, k, v, do = mk(H), mk(Hk), mk(Hk), mk(H)
    scale = D ** -0.5
    i = torch.arange(S, dtype=torch.int32)
    L = S // ndoc
    doc = (i // L * L).view(1, S).contiguous().to(dev), ((i // L + 1) * L).view(1, S).contiguous().to(dev)
    tri = torch.zeros(1, S, dtype=torch.int32, device=dev), (i + 1).view(1, S).contiguous().to(dev)
    cu = torch.arange(0, S + 1, L, dtype=torch.int32, device=dev)

    def buffers():
        return (torch.empty_like(q), torch.empty(B, H, S, dtype=torch.float32, device=dev), torch.empty(B, H, S, dtype=torch.float32, device=dev),
                torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))

    def dense(causal, rr, forced):
        out, lse, delta, dq, dk, dv = buffers()
        kw = {} if rr is None else {"row_ranges": (rr[0], rr[1], 0)}

        def fwd():
            with config.override(**forced):
                be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **kw)

        def bwd():
            with config.override(**forced):
                be.bwd_preprocess(do, out, delta)
                be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, **kw)

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

    # (a): the forms a ranged call runs — the 8 x 32 forward without shares, the 128-key dK/dV kernel, the 7-GEMM dQ kernel
    forced = dict(fwd_form="8x32", fwd_kv_nsplit=1, dkdv_wide=0, bwd_ds_spill=False)
    f_doc, b_doc, r_doc = dense(True, doc, {})
    f_tri, b_tri, r_tri = dense(False, tri, {})
    f_a, b_a, r_a = dense(True, None, forced)
    f_b, b_b, r_b = packed()
    for fn in (f_doc, b_doc, f_tri, b_tri, f_a, b_a, f_b, b_b):
        fn()
    torch.cuda.synchronize()
    # the ranged calls compute what the calls beside them compute
    agree = dict(doc_vs_cu_seqlens=max((x[0].float() - y.float()).abs().max().item() for x, y in zip(r_doc, r_b)),
                 causal_by_ranges_vs_causal=max((x.float() - y.float()).abs().max().item() for x, y in zip(r_tri, r_a)))
    names = ("fwd_doc_ranges", "bwd_doc_ranges", "fwd_causal_forced", "bwd_causal_forced", "fwd_doc_cu_seqlens", "bwd_doc_cu_seqlens",
             "fwd_causal_by_ranges", "bwd_causal_by_ranges")
    res = dict(zip(names, timed([f_doc, b_doc, f_a, b_a, f_b, b_b, f_tri, b_tri], a.batches, a.per_batch)))
    res.update(zip(("fwd_causal_forced_again", "bwd_causal_forced_again"), timed([f_a, b_a], a.batches, a.per_batch)))
    med = {n: t[0] for n, t in res.items()}
    total = lambda tag: med["fwd_" + tag] + med["bwd_" + tag]
    ratios = dict(doc_ranges_over_causal_forced=round(total("doc_ranges") / total("causal_forced"), 4),
                  doc_ranges_over_cu_seqlens=round(total("doc_ranges") / total("doc_cu_seqlens"), 4),
                  causal_by_ranges_over_causal_forced=round(total("causal_by_ranges") / total("causal_forced"), 4),
                  fwd_causal_by_ranges_over_causal_forced=round(med["fwd_causal_by_ranges"] / med["fwd_causal_forced"], 4),
                  bwd_causal_by_ranges_over_causal_forced=round(med["bwd_causal_by_ranges"] / med["bwd_causal_forced"], 4))
    print(f"B {B} S {S} H {H} / Hk {Hk} D {D} bf16, {ndoc} documents of {L}")
    for n, t in res.items():
        print(f"  {n:26s} median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})")
    print("  ratios (forward + backward, medians):", ratios)
    print("  max |difference|:", agree)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, S=S, H=H, Hk=Hk, D=D, dtype="bf16", documents=ndoc),
                           ms={n: dict(median=round(t[0], 4), min=round(t[1], 4), max=round(t[2], 4)) for n, t in res.items()},
                           ratios=ratios, agree=agree), f, indent=1)
    assert ratios["doc_ranges_over_causal_forced"] < 1.0, "the ranged document call must be faster than the causal call it is one eighth of"


if __name__ == "__main__":
    main()
