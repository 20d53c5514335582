"""Per-row key ranges (include/rfa.h: rfa_fwd_rr / rfa_bwd_rr; ring_flash_attn.with_row_ranges) in the kernels against fp64
with the explicit boolean mask (tests/_rowrange_backend.py) through tests/_tol.py, unchanged: the kRng instances of the 8 x 32
forward, the 7-GEMM dQ kernel and the 128-key dK/dV kernel for head dims 128 and 64 (full) and 72 and 40 (the zero-padded
layouts), bf16 and fp16 — interval edges on and around the 64-, 128- and 256-key tile boundaries, one-key rows, empty rows,
whole empty workgroups, a k_pos0 that puts the ranges partly and wholly outside the block, Sq != Sk, each with and without
`causal`; ranges that spell plain causal against the causal call; ranges that spell five documents against the cu_seqlens
call; accumulate-mode outputs and the two-phase backward; the six public functions over W = 2 and 4 ranks sharing the GPU; and
two runs of one ranged backward, bit for bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _rowrange_backend as RB                   # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
B, H, HK, S = 2, 4, 2, 320
KINDS5 = ("out", "lse", "grad", "grad", "grad")
NAMES5 = ("out", "lse", "dq", "dk", "dv")
EDGES = (63, 64, 65, 127, 128, 129, 255, 256, 257)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _pattern(name, sq, sk):
    """(start, end, k_pos0): int32 (B, sq) global key positions and where key row 0 of the block sits"""
    i = torch.arange(sq)
    e = torch.tensor(EDGES)
    k0 = 0
    if name == "edges":            # batch 0: [0, edge), batch 1: [edge, end) — every edge, in every residue of the row index
        start = torch.stack([torch.zeros(sq, dtype=torch.long), e[i % 9]])
        end = torch.stack([e[(i + i // 9) % 9], torch.full((sq,), sk)])
    elif name == "edge_pairs":     # both bounds on the edges: [edge a, edge b), empty where a >= b
        start = torch.stack([e[i % 9], e[(i // 3) % 9]])
        end = torch.stack([e[(i // 9) % 9], e[(i + 4) % 9]])
    elif name == "one_key":        # batch 0: the diagonal, batch 1: the anti-diagonal
        start = torch.stack([i % sk, (sk - 1 - i) % sk])
        end = start + 1
    elif name == "empty_rows":     # random intervals, two rows in three are empty
        g = torch.Generator().manual_seed(11)
        start = torch.randint(0, sk, (B, sq), generator=g)
        end = start + torch.randint(1, sk, (B, sq), generator=g)
        end[:, 1::3] = start[:, 1::3]
        end[:, 2::3] = start[:, 2::3] - 5
    elif name == "empty_workgroups":   # batch 0: the first 256 rows see nothing, batch 1: the rows from 256 on
        start = torch.zeros(B, sq, dtype=torch.long)
        end = torch.full((B, sq), sk)
        end[0, :256] = 0
        start[1, 256:] = sk + 7
    elif name == "partly_outside":     # ranges of a longer sequence: the block holds the keys 100 .. 100 + sk - 1 of it
        k0 = 100
        start = torch.stack([(i - 30).clamp(min=0), torch.full((sq,), 50)])
        end = torch.stack([i + 130, torch.full((sq,), 100 + sk + 500)])
    elif name == "wholly_outside":     # ... and a block none of whose keys any row asks for
        k0 = 1000
        start = torch.stack([i, torch.full((sq,), 2000)])
        end = torch.stack([i + 500, torch.full((sq,), 2 ** 31 - 1)])
    else:
        raise ValueError(name)
    return start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous(), k0


PATTERNS = ("edges", "edge_pairs", "one_key", "empty_rows", "empty_workgroups", "partly_outside", "wholly_outside")


def _inputs(sq, sk, D, dt, seed=0):
    gen = torch.Generator().manual_seed(5100 + sq + 3 * sk + 7 * D + seed)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dt)
    return mk(B, sq, H, D), mk(B, sk, HK, D), mk(B, sk, HK, D), mk(B, sq, H, D)


def _run(be, q, k, v, do, causal, rr, **kw):
    """forward and backward into plain outputs: (out, lse, dq, dk, dv)"""
    scale = q.shape[-1] ** -0.5
    out = torch.empty_like(q)
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    extra = {} if rr is None else {"row_ranges": rr}
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **extra, **kw)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, **extra, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _failures(got, ref, tag, kinds=KINDS5):
    bad = []
    for name, g_, r_, kind in zip(NAMES5, got, ref, kinds):
        m = _tol.metrics(g_, r_)
        print(f"{tag}{name}: max_err {m['max_err']:.3e} max_ref {m['max_ref']:.3e} fro {m['fro']:.3e} mean_err {m['mean_err']:.3e}")
        bad += _tol.failures(tag + name, g_, r_, kind)
    return bad


def _block(D, dt, sq, sk, patterns):
    be, dev = _be(), _dev()
    q, k, v, do = _inputs(sq, sk, D, dt)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    bad = []
    for name in patterns:
        start, end, k0 = _pattern(name, sq, sk)
        rr = (start.to(dev), end.to(dev), k0)
        for causal in (False, True):
            ref = RB.single_device(q, k, v, do, RB.block_mask(start, end, k0, sk, causal))
            got = _run(be, qd, kd, vd, dod, causal, rr)
            bad += _failures(got, ref, f"{name}-{'causal' if causal else 'full'}.")
            if name == "wholly_outside":
                assert not torch.isfinite(got[1]).any() and all(float(t.abs().max()) == 0.0 for t in (got[0],) + got[2:])
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("dt", [BF, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [128, 64, 72, 40])
def test_block_interval_edges(D, dt):
    """B 2, Sq = Sk = 320, H 4 / Hk 2: every pattern with and without causal, forward and backward, against fp64"""
    _block(D, dt, S, S, PATTERNS)


@pytest.mark.parametrize("sq,sk", [(130, 320), (320, 130)])
@pytest.mark.parametrize("D,dt", [(128, BF), (64, FP16), (72, BF)])
def test_block_with_unequal_lengths(D, dt, sq, sk):
    """Sq != Sk: the causal diagonal is bottom-right aligned, the ranges are absolute"""
    _block(D, dt, sq, sk, ("edges", "empty_rows", "partly_outside"))


@pytest.mark.parametrize("D", [128, 64])
def test_ranges_under_a_window_and_a_shifted_band(D):
    """the ranges intersect a causal window of 100 keys, once with the block one block in front (mask_shift = Sk)"""
    be, dev = _be(), _dev()
    q, k, v, do = _inputs(S, S, D, BF, seed=3)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    start, end, k0 = _pattern("edges", S, S)
    bad = []
    for shift in (0, 200):
        ref = RB.single_device(q, k, v, do, RB.block_mask(start, end, k0, S, True, (100, -1), shift))
        got = _run(be, qd, kd, vd, dod, True, (start.to(dev), end.to(dev), k0), window=(100, -1), mask_shift=shift)
        bad += _failures(got, ref, f"window-shift{shift}.")
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("D,dt", [(128, BF), (64, FP16), (40, BF)])
def test_ranges_that_spell_causal_against_the_causal_call(D, dt):
    """start = 0, end = i + 1 on a non-causal call is the causal mask: within tolerance of the plain causal call (and of fp64)"""
    be, dev = _be(), _dev()
    q, k, v, do = _inputs(S, S, D, dt, seed=5)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    i = torch.arange(S, dtype=torch.int32)
    start, end = torch.zeros(B, S, dtype=torch.int32), (i + 1).expand(B, S).contiguous()
    got = _run(be, qd, kd, vd, dod, False, (start.to(dev), end.to(dev), 0))
    plain = _run(be, qd, kd, vd, dod, True, None)
    ref = RB.single_device(q, k, v, do, RB.block_mask(start, end, 0, S, True))
    bad = _failures(got, ref, "vs fp64.") + _failures(got, plain, "vs the causal call.")
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [128, 64])
def test_ranges_that_spell_five_documents_against_the_cu_seqlens_call(D, causal):
    """one dense row of 320 tokens = five packed documents: the ranged dense call against the existing cu_seqlens call"""
    be, dev = _be(), _dev()
    lens = [50, 70, 64, 100, 36]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    gen = torch.Generator().manual_seed(77 + D)
    mk = lambda h: torch.randn(1, S, h, D, generator=gen).to(BF).to(dev)
    q, k, v, do = mk(H), mk(HK), mk(HK), mk(H)
    doc = torch.bucketize(torch.arange(S), torch.tensor(cu[1:-1]), right=True)
    start = torch.tensor(cu)[doc].to(torch.int32).view(1, S).contiguous().to(dev)
    end = torch.tensor(cu)[doc + 1].to(torch.int32).view(1, S).contiguous().to(dev)
    got = _run(be, q, k, v, do, causal, (start, end, 0))
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    scale = D ** -0.5
    pq, pk, pv, pdo = (t[0] for t in (q, k, v, do))
    out, lse = torch.empty_like(pq), torch.empty((H, S), dtype=torch.float32, device=dev)
    kw = dict(softmax_scale=scale, causal=causal, cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=max(lens), max_seqlen_k=max(lens))
    be.fwd(pq, pk, pv, out=out, lse=lse, **kw)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(pdo, out, delta, cu_seqlens_q=cu_t, max_seqlen_q=max(lens))
    dq, dk, dv = torch.empty_like(pq), torch.empty_like(pk), torch.empty_like(pv)
    be.bwd(pdo, pq, pk, pv, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
    torch.cuda.synchronize()
    packed = (out.unsqueeze(0), lse.unsqueeze(0), dq.unsqueeze(0), dk.unsqueeze(0), dv.unsqueeze(0))
    bad = _failures(got, packed, "vs cu_seqlens.")
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("D,dt", [(128, BF), (72, FP16)])
def test_accumulate_mode_and_the_two_phase_backward(D, dt):
    """keys [0, 130) and [130, 320) as two ranged block calls (k_pos0 = 0 and 130) merged through out_acc / lse_acc — the
    second one dark for the rows whose range ends in front of it —, then RFA_BWD_COMPUTE / RFA_BWD_REDUCE per block `+=` into
    fp32 accumulators that hold a known value: against the one fp64 attention over all keys"""
    from ring_flash_attn import _C

    be, dev = _be(), _dev()
    h = 130
    q, k, v, do = _inputs(S, S, D, dt, seed=9)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    start, end, _ = _pattern("edges", S, S)
    ref = RB.single_device(q, k, v, do, RB.block_mask(start, end, 0, S, True))
    sd, ed = start.to(dev), end.to(dev)
    scale = D ** -0.5
    out_acc = torch.empty(q.shape, dtype=torch.float32, device=dev)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    blocks = ((slice(0, h), S - h, 0), (slice(h, S), 0, h))
    for n, (ks, shift, k0) in enumerate(blocks):
        be.fwd(qd, kd[:, ks], vd[:, ks], softmax_scale=scale, causal=True, out_acc=out_acc, lse_acc=lse_acc, acc_init=n == 0,
               row_ranges=(sd, ed, k0), **({"mask_shift": shift} if shift else {}))
    out = out_acc.to(dt)
    lse = lse_acc.clone()
    delta = torch.empty_like(lse)
    be.bwd_preprocess(dod, out, delta)
    acc = [torch.full(t.shape, 0.5, dtype=torch.float32, device=dev) for t in (q, k, v)]
    for ks, shift, k0 in blocks:
        kw = dict(softmax_scale=scale, causal=True, dq_acc=acc[0], dk_acc=acc[1][:, ks], dv_acc=acc[2][:, ks],
                  row_ranges=(sd, ed, k0), **({"mask_shift": shift} if shift else {}))
        part = be.bwd(dod, qd, kd[:, ks], vd[:, ks], lse, delta, phases=_C.BWD_COMPUTE, **kw)
        be.bwd(dod, qd, kd[:, ks], vd[:, ks], lse, delta, phases=_C.BWD_REDUCE, partials=part, **kw)
    torch.cuda.synchronize()
    lse_got = torch.where(torch.isinf(lse_acc), torch.full_like(lse_acc, float("inf")), lse_acc)     # (-inf: a row without a key)
    bad = _failures((out_acc, lse_got, acc[0] - 0.5, acc[1] - 0.5, acc[2] - 0.5), ref, "two blocks.",
                    ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring"))
    assert not bad, "; ".join(bad[:12])


def test_two_runs_of_one_ranged_backward_give_the_same_bits():
    be, dev = _be(), _dev()
    q, k, v, do = (t.to(dev) for t in _inputs(S, S, 128, BF, seed=13))
    start, end, k0 = _pattern("empty_rows", S, S)
    rr = (start.to(dev), end.to(dev), k0)
    a = _run(be, q, k, v, do, True, rr)
    b = _run(be, q, k, v, do, True, rr)
    for name, x, y in zip(NAMES5, a, b):
        assert torch.equal(x, y), name


def _multi_cases(W):
    pats = [dict(pattern="doc", causal=True), dict(pattern="prefix", causal=False), dict(pattern="random", causal=False)]
    cases = []
    for kind, forms in (("ring", (None,)), ("zigzag", ("ring", "gather"))):
        for pack in (None, "kv", "qkv"):
            for n, p in enumerate(pats):
                form = forms[n % len(forms)]
                cases.append(dict(kind=kind, W=W, S=128, D=128 if n != 1 else 64, pack=pack, **({"form": form} if form else {}), **p))
    return cases


@pytest.mark.parametrize("W", [2, 4])
def test_the_six_functions_over_ranks_sharing_the_gpu(W):
    """ring_ and zigzag_ring_flash_attn_{,kvpacked_,qkvpacked_}func with the ranks sharing cuda:0 (host staging), S = 128 rows per
    rank: documents under causal, a non-causal prefix-LM mask, random intervals with empty rows — each against ONE single-device
    fp64 attention with the explicit mask"""
    import _rowrange_worker as RW

    errs, notes = RW.run_world(W, _multi_cases(W), True, free_port(), limit_s=240)
    print("\n".join(notes))
    assert not errs, "\n".join(errs[:20])
