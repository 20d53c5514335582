"""`mask_shift` of the C ABI (include/rfa.h, ABI 7) on the GPU: one dense sequence computed once unsharded with a
sliding window and once as a grid of blocks that are told where they sit, merged through the fp32 accumulators — both
against an fp64 attention with an explicit mask (tests/_blockref.py), computed on the device.  Plus the band normalisation of the
dispatch layer (a block wholly inside the band IS the unwindowed call; an empty block touches nothing) and a block call
under HIP graph capture."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _bandref import band_ref                  # noqa: E402

BF = torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _inputs(B, Sq, Sk, H, Hk, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    dev = _dev()
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(dev)
    return mk(B, Sq, H, D), mk(B, Sk, Hk, D), mk(B, Sk, Hk, D), mk(B, Sq, H, D)


def _unsharded(be, q, k, v, do, causal, window):
    B, Sq, H, D = q.shape
    out = torch.empty_like(q)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=D ** -0.5, causal=causal, out=out, lse=lse, window=window)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=D ** -0.5, causal=causal, dq=dq, dk=dk, dv=dv, window=window)
    return out, lse, dq, dk, dv


def _blocked(be, q, k, v, do, causal, window, bq, bk):
    """the same attention as a grid of (bq x bk) blocks with mask_shift, accumulated in fp32"""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    scale = D ** -0.5
    out_acc = torch.empty(B, Sq, H, D, dtype=torch.float32, device=q.device)
    lse_acc = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    qb = [(a, min(bq, Sq - a)) for a in range(0, Sq, bq)]
    kb = [(a, min(bk, Sk - a)) for a in range(0, Sk, bk)]

    def shift(q0, lq, k0, lk):
        # (global position of q row 0 + len_q) - (global position of k row 0 + len_k); q row 0 of the whole call sits at Sk - Sq
        return (q0 + Sk - Sq + lq) - (k0 + lk)

    for q0, lq in qb:
        for n, (k0, lk) in enumerate(kb):
            be.fwd(q[:, q0:q0 + lq], k[:, k0:k0 + lk], v[:, k0:k0 + lk], softmax_scale=scale, causal=causal, window=window,
                   out_acc=out_acc[:, q0:q0 + lq], lse_acc=lse_acc[:, :, q0:q0 + lq], acc_init=(n == 0),
                   mask_shift=shift(q0, lq, k0, lk))
    out = be.cast(out_acc, q.dtype)
    lse = torch.where(torch.isinf(lse_acc), torch.full_like(lse_acc, float("inf")), lse_acc)   # (-inf: no key in any block)
    delta = torch.empty_like(lse_acc)
    be.bwd_preprocess(do, out, delta)
    dq = torch.zeros(B, Sq, H, D, dtype=torch.float32, device=q.device)
    dk = torch.zeros(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.zeros(v.shape, dtype=torch.float32, device=q.device)
    for q0, lq in qb:
        lse_b = lse[:, :, q0:q0 + lq].contiguous()
        delta_b = delta[:, :, q0:q0 + lq].contiguous()
        for k0, lk in kb:
            be.bwd(do[:, q0:q0 + lq], q[:, q0:q0 + lq], k[:, k0:k0 + lk], v[:, k0:k0 + lk], lse_b, delta_b,
                   softmax_scale=scale, causal=causal, window=window, dq_acc=dq[:, q0:q0 + lq],
                   dk_acc=dk[:, k0:k0 + lk], dv_acc=dv[:, k0:k0 + lk], mask_shift=shift(q0, lq, k0, lk))
    return out, lse, be.cast(dq, q.dtype), be.cast(dk, q.dtype), be.cast(dv, q.dtype)


def _compare_all(tag, got, ref, kinds):
    import _tol

    bad = []
    for name, g, r, kind in zip(("out", "lse", "dq", "dk", "dv"), got, ref, kinds):
        bad += _tol.failures(f"{tag}.{name}", g, r.float(), kind)
    assert not bad, "; ".join(bad)


CASES = [
    # D, dtype, Sq, Sk, bq, bk, causal, window
    pytest.param(128, BF, 1536, 1536, 512, 512, True, (700, 0), id="d128-causal-700"),
    pytest.param(128, BF, 1536, 1536, 512, 512, False, (600, 250), id="d128-two-sided"),
    pytest.param(128, BF, 1536, 1536, 512, 512, True, (-1, -1), id="d128-causal-only"),
    pytest.param(128, BF, 1536, 1536, 512, 512, True, (100, 0), id="d128-narrow", marks=pytest.mark.extended),
    pytest.param(128, BF, 1536, 1536, 512, 512, False, (-1, 300), id="d128-right-only", marks=pytest.mark.extended),
    pytest.param(128, BF, 1024, 1536, 512, 768, True, (500, 0), id="d128-sq-lt-sk", marks=pytest.mark.extended),
    pytest.param(128, BF, 1536, 1000, 512, 500, False, (400, 100), id="d128-sq-gt-sk", marks=pytest.mark.extended),
    pytest.param(128, torch.float16, 1536, 1536, 512, 512, True, (700, 0), id="d128-fp16", marks=pytest.mark.extended),
    pytest.param(64, BF, 1536, 1536, 512, 512, True, (700, 0), id="d64", marks=pytest.mark.extended),
    pytest.param(96, BF, 1024, 1024, 512, 512, True, (600, 0), id="d96", marks=pytest.mark.extended),
    pytest.param(192, BF, 1024, 1024, 512, 512, True, (600, 0), id="d192", marks=pytest.mark.extended),
    pytest.param(256, BF, 1024, 1024, 512, 512, True, (600, 0), id="d256", marks=pytest.mark.extended),
    pytest.param(256, BF, 1024, 1024, 512, 512, False, (300, 200), id="d256-two-sided", marks=pytest.mark.extended),
]


@pytest.mark.parametrize("D,dtype,Sq,Sk,bq,bk,causal,window", CASES)
def test_blocks_with_mask_shift_match_the_unsharded_window(D, dtype, Sq, Sk, bq, bk, causal, window):
    """one windowed attention, unsharded and as a grid of shifted blocks, against the explicit-mask fp64 reference"""
    be = _be()
    q, k, v, do = _inputs(1, Sq, Sk, 8, 2, D, dtype, 1234 + D)
    ref = band_ref(q, k, v, do, causal, window)
    _compare_all("unsharded", _unsharded(be, q, k, v, do, causal, window), ref, ("out", "lse", "grad", "grad", "grad"))
    _compare_all("blocks", _blocked(be, q, k, v, do, causal, window, bq, bk), ref,
                 ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring"))


def _bwd_args(C_, B, Sq, Sk, H, Hk, D, causal, window, shift, acc=False):
    a = C_.BwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.total_k = B, Sq, Sk, H, Hk, D, 0, B * Sk
    a.causal = 1 if causal else 0
    if window[0] >= 0 or window[1] >= 0:
        a.window, a.window_left, a.window_right = 1, window[0], window[1]
    a.mask_shift = shift
    a.ds_scratch = 256            # (non-NULL: the plan functions are pure functions of the arguments and never read it)
    if acc:
        a.dq_acc = a.dk_acc = a.dv_acc = 256
    return a


def test_block_inside_the_band_is_the_unwindowed_call():
    """normalisation: a block every element of which is visible runs the instance, plan and dS-spill form of the
    unwindowed non-causal call — identical bits, identical rfa_bwd_plan"""
    from ring_flash_attn import _C

    be = _be()
    B, S, H, Hk, D = 1, 1024, 8, 2, 128
    q, k, v, do = _inputs(B, S, S, H, Hk, D, BF, 5)
    scale = D ** -0.5

    def run(**band):
        out = torch.empty_like(q)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
        be.fwd(q, k, v, softmax_scale=scale, out=out, lse=lse, **band)
        delta = torch.empty_like(lse)
        be.bwd_preprocess(do, out, delta)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, dq=dq, dk=dk, dv=dv, **band)
        return out, lse, dq, dk, dv

    plain = run(causal=False)
    # the keys lie 2 S rows in front of the queries; the window reaches 3 S - 1 rows back: everything is visible
    for band in (dict(causal=True, window=(3 * S - 1, 0), mask_shift=2 * S), dict(causal=True, mask_shift=S),
                 dict(causal=False, window=(5 * S, 5 * S), mask_shift=-3 * S), dict(causal=True, mask_shift=1 << 40)):
        got = run(**band)
        for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, plain):
            assert torch.equal(a, b), f"{band}: {name} differs from the unwindowed non-causal call"
    for shape in ((1, 1024, 1024, 8, 2, 128), (1, 8192, 8192, 32, 8, 128), (4, 2048, 2048, 32, 8, 128), (1, 2048, 2048, 8, 2, 64)):
        want = be.bwd_plan(_bwd_args(_C, *shape, False, (-1, -1), 0))
        assert be.bwd_plan(_bwd_args(_C, *shape, True, (3 * shape[1], 0), 2 * shape[1])) == want
        assert be.bwd_plan(_bwd_args(_C, *shape, True, (-1, -1), shape[1])) == want
        a0, a1 = _bwd_args(_C, *shape, False, (-1, -1), 0), _bwd_args(_C, *shape, True, (3 * shape[1], 0), 2 * shape[1])
        assert be.lib.rfa_bwd_ds_scratch_bytes(a0) == be.lib.rfa_bwd_ds_scratch_bytes(a1)
        assert be.lib.rfa_bwd_workspace_bytes(a0) == be.lib.rfa_bwd_workspace_bytes(a1)
    # forms keyed on the block's own diagonal decline a shifted causal band: the headline block shifted by half a block
    form, _, _ = be.bwd_plan(_bwd_args(_C, 1, 8192, 8192, 32, 8, 128, True, (-1, -1), 0))
    assert form == _C.DKDV_BAL
    form, _, _ = be.bwd_plan(_bwd_args(_C, 1, 8192, 8192, 32, 8, 128, True, (-1, -1), 4096))
    assert form != _C.DKDV_BAL


def test_empty_block_touches_nothing():
    """a block with no visible element: accumulators (poisoned here) stay as they are, plain outputs read 0 / +inf"""
    be = _be()
    B, S, H, Hk, D = 1, 512, 8, 2, 128
    q, k, v, do = _inputs(B, S, S, H, Hk, D, BF, 6)
    scale = D ** -0.5
    dev = q.device
    lse_g = torch.randn(B, H, S, device=dev)
    delta = torch.randn(B, H, S, device=dev)
    # keys BEHIND the queries of a causal call; keys further in front than the window reaches; beyond the right side
    for band in (dict(causal=True, mask_shift=-S), dict(causal=True, window=(100, 0), mask_shift=2 * S),
                 dict(causal=False, window=(-1, 10), mask_shift=-2 * S), dict(causal=True, mask_shift=-(1 << 45))):
        out_acc = torch.full((B, S, H, D), 7.0, device=dev)
        lse_acc = torch.full((B, H, S), 3.0, device=dev)
        be.fwd(q, k, v, softmax_scale=scale, out_acc=out_acc, lse_acc=lse_acc, **band)
        assert bool((out_acc == 7.0).all()) and bool((lse_acc == 3.0).all()), band
        out = torch.full_like(q, 5.0)
        lse = torch.full((B, H, S), 5.0, device=dev)
        be.fwd(q, k, v, softmax_scale=scale, out=out, lse=lse, **band)
        assert bool((out == 0).all()) and bool((lse == float("inf")).all()), band
        # the first block of a ring may be empty too: the accumulators are overwritten with "nothing yet"
        be.fwd(q, k, v, softmax_scale=scale, out_acc=out_acc, lse_acc=lse_acc, acc_init=True, **band)
        assert bool((out_acc == 0).all()) and bool((lse_acc == float("-inf")).all()), band
        dq, dk, dv = (torch.full(t.shape, 9.0, device=dev) for t in (q, k, v))
        be.bwd(do, q, k, v, lse_g, delta, softmax_scale=scale, dq_acc=dq, dk_acc=dk, dv_acc=dv, **band)
        assert all(bool((t == 9.0).all()) for t in (dq, dk, dv)), band
        part = be.bwd(do, q, k, v, lse_g, delta, softmax_scale=scale, dq_acc=dq, dk_acc=dk, dv_acc=dv, phases=1, **band)
        be.bwd(do, q, k, v, lse_g, delta, softmax_scale=scale, dq_acc=dq, dk_acc=dk, dv_acc=dv, phases=2, partials=part, **band)
        assert all(bool((t == 9.0).all()) for t in (dq, dk, dv)), band
        pq, pk, pv = torch.full_like(q, 5.0), torch.full_like(k, 5.0), torch.full_like(v, 5.0)
        be.bwd(do, q, k, v, lse_g, delta, softmax_scale=scale, dq=pq, dk=pk, dv=pv, **band)
        assert all(bool((t == 0).all()) for t in (pq, pk, pv)), band


def test_shift_needs_dense_input():
    from ring_flash_attn import _C

    be = _be()
    q, k, v, _ = _inputs(1, 256, 256, 4, 2, 128, BF, 7)
    q, k, v = q[0], k[0], v[0]
    cu = torch.tensor([0, 256], dtype=torch.int32, device=q.device)
    out, lse = torch.empty_like(q), torch.empty(4, 256, dtype=torch.float32, device=q.device)
    with pytest.raises(RuntimeError, match="rfa status -8"):
        be.fwd(q, k, v, softmax_scale=0.1, causal=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=256, max_seqlen_k=256,
               out=out, lse=lse, mask_shift=256)
    assert _C.RFA_ABI_VERSION >= 7


def test_shifted_block_under_hip_graph_capture():
    """a windowed block call with mask_shift (a band that cuts the block: workgroups with no visible tile leave early),
    forward and backward into fp32 accumulators, captured into a HIP graph and replayed on new data: the eager bits"""
    be = _be()
    B, S, H, Hk, D = 1, 1024, 8, 2, 128
    dev = _dev()
    scale = D ** -0.5
    band = dict(causal=True, window=(600, 0), mask_shift=S)
    g = torch.Generator().manual_seed(99)
    mk = lambda: tuple(torch.randn(*s, generator=g).to(BF).to(dev) for s in ((B, S, H, D), (B, S, Hk, D), (B, S, Hk, D), (B, S, H, D)))

    def step(q, k, v, do, bufs):
        out_acc, lse_acc, delta, dq, dk, dv = bufs
        be.fwd(q, k, v, softmax_scale=scale, out_acc=out_acc, lse_acc=lse_acc, acc_init=True, **band)
        lse = torch.where(torch.isinf(lse_acc), torch.zeros_like(lse_acc), lse_acc)
        be.bwd_preprocess(do, be.cast(out_acc, BF), delta)
        be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, dq_acc=dq, dk_acc=dk, dv_acc=dv, acc_init=True, **band)

    def bufs():
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        return f(B, S, H, D), f(B, H, S), f(B, H, S), f(B, S, H, D), f(B, S, Hk, D), f(B, S, Hk, D)

    sq, sk, sv, sdo = mk()
    sb = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(sq, sk, sv, sdo, sb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(sq, sk, sv, sdo, sb)
    for trial in range(2):
        q1, k1, v1, do1 = mk()
        with torch.no_grad():
            sq.copy_(q1); sk.copy_(k1); sv.copy_(v1); sdo.copy_(do1)
        graph.replay()
        torch.cuda.synchronize()
        eb = bufs()
        step(q1, k1, v1, do1, eb)
        torch.cuda.synchronize()
        for name, a, b in zip(("out_acc", "lse_acc", "delta", "dq", "dk", "dv"), sb, eb):
            assert torch.equal(a, b), f"{name} differs on replay {trial}"
