"""Block-sparse masks (include/rfa.h: rfa_fwd_bm / rfa_bwd_bm; ring_flash_attn.with_block_mask) in the kernels against fp64 with
the explicit boolean mask (tests/_blockmask_backend.py) through tests/_tol.py, unchanged: the kBlk instances of the 8 x 32
forward, the 7-GEMM dQ kernel and the 128-key dK/dV kernel for head dims 128 and 64 (full) and 72 and 40 (the zero-padded
layouts), bf16 and fp16.  Sq 640 / Sk 1024 is three forward / dQ workgroups (the last holds ONE query block) against 8 key
blocks = 16 tiles; Sq 320 / Sk 333 has partial tail blocks both ways.  The patterns cover visited lists of length 1, 2, 3, odd
and even, gaps longer than the LDS ring, a dark sibling query block, a wholly dark workgroup, a wholly dark key block, masks per
batch entry and per head inside one K/V group, and a k_blk0 that puts columns partly and wholly outside the mask — each with
and without `causal`, and under a window with a mask_shift of both signs.  An all-True mask gives the bits of the call without
one; five aligned documents agree with the cu_seqlens call and with with_row_ranges; accumulate outputs, the two-phase
backward, two runs bit for bit, and the six public functions over W = 2 and 4 ranks sharing the GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _blockmask_backend as MB                  # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
B, H, HK = 2, 4, 2
KINDS5 = ("out", "lse", "grad", "grad", "grad")
NAMES5 = ("out", "lse", "dq", "dk", "dv")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _pattern(name, nq, nk, heads=H):
    """(mask, k_blk0): bool (Bm, Hm, nq, NK) and the mask column of key row 0 (NK = nk unless the pattern moves the block)"""
    r, c = torch.arange(nq).view(-1, 1), torch.arange(nk).view(1, -1)
    g = torch.Generator().manual_seed(31 + nq + 7 * nk)
    rnd = lambda *s: torch.rand(*s, generator=g) < 0.4
    k0 = 0
    if name == "alternate":          # every other block lit
        m = ((r + c) % 2 == 0).expand(1, 1, nq, nk)
    elif name == "last":             # only the last key block: one list entry far from the start
        m = (c == nk - 1).expand(1, 1, nq, nk)
    elif name == "first_last":       # a gap longer than the LDS ring
        m = ((c == 0) | (c == nk - 1)).expand(1, 1, nq, nk)
    elif name == "lists":            # per workgroup (two query blocks): 1, then 2, then 3 lit key blocks (2, 4, 6 tiles; causal cuts some to odd)
        m = torch.zeros(1, 1, nq, nk, dtype=torch.bool)
        m[..., 0:2, min(2, nk - 1)] = True
        if nq > 2:
            m[..., 2, min(1, nk - 1)] = True
        if nq > 3:
            m[..., 3, min(5, nk - 1)] = True
        if nq > 4:
            m[..., 4, [0, min(3, nk - 1), nk - 1]] = True
    elif name == "sibling_dark":     # one query block of a workgroup dark while its sibling is lit
        m = rnd(1, 1, nq, nk) | (c == 1)
        m[..., 0::4, :] = False
        m[..., 3::4, :] = False
    elif name == "dark_workgroup":   # rows 0 .. 255 see nothing
        m = rnd(1, 1, nq, nk) | (c == 0)
        m[..., 0:2, :] = False
    elif name == "dark_key_block":   # dK = dV = 0 there
        m = (rnd(1, 1, nq, nk) | (c == 0)) & (c != min(3, nk - 1))
    elif name == "per_batch":
        m = rnd(B, 1, nq, nk) | (c == 0)
    elif name == "per_head":         # masks that differ inside one K/V group
        m = rnd(1, heads, nq, nk)
        m[:, 0] |= (c == 0)
        m[:, 1::2, :, 1:] ^= True
    elif name == "partly_outside":   # the block's first two key blocks lie in front of the mask, its last ones behind
        m, k0 = rnd(1, 1, nq, max(nk - 3, 1)) | (c[:, :max(nk - 3, 1)] == 0), -2
    elif name == "wholly_outside":   # a block none of whose columns exists
        m, k0 = torch.ones(1, 1, nq, nk, dtype=torch.bool), nk + 5
    else:
        raise ValueError(name)
    return m.contiguous(), k0


PATTERNS = ("alternate", "last", "first_last", "lists", "sibling_dark", "dark_workgroup", "dark_key_block", "per_batch", "per_head",
            "partly_outside", "wholly_outside")


def _inputs(sq, sk, D, dt, seed=0, heads=(H, HK)):
    gen = torch.Generator().manual_seed(6100 + sq + 3 * sk + 7 * D + seed)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dt)
    return mk(B, sq, heads[0], D), mk(B, sk, heads[1], D), mk(B, sk, heads[1], D), mk(B, sq, heads[0], D)


def _run(be, q, k, v, do, causal, bm, **kw):
    """forward and backward into plain outputs: (out, lse, dq, dk, dv)"""
    scale = q.shape[-1] ** -0.5
    out = torch.empty_like(q)
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    extra = {} if bm is None else {"block_mask": bm}
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


def _block(D, dt, sq, sk, patterns, heads=(H, HK), bands=((False, {}), (True, {}))):
    be, dev = _be(), _dev()
    q, k, v, do = _inputs(sq, sk, D, dt, heads=heads)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    nq, nk = -(-sq // 128), -(-sk // 128)
    bad = []
    for name in patterns:
        m, k0 = _pattern(name, nq, nk, heads[0])
        for causal, band in bands:
            ref = MB.single_device(q, k, v, do, MB.expand(m, B, heads[0], sq, sk, causal, band.get("window", (-1, -1)), k0,
                                                          band.get("mask_shift", 0)))
            got = _run(be, qd, kd, vd, dod, causal, (m.to(dev), k0), **band)
            bad += _failures(got, ref, f"{name}-{'causal' if causal else 'full'}{band or ''}.")
            if name == "wholly_outside":
                assert not torch.isfinite(got[1]).any() and all(float(t.abs().max()) == 0.0 for t in (got[0],) + got[2:])
            if name == "dark_key_block":
                c = min(3, nk - 1)
                assert float(got[3][:, 128 * c:128 * c + 128].abs().max()) == 0.0 and float(got[4][:, 128 * c:128 * c + 128].abs().max()) == 0.0
    assert not bad, "; ".join(bad[:12])


_SWEEP = [pytest.param(128, BF, id="128-bf16"), pytest.param(64, FP16, id="64-fp16"),
          pytest.param(128, FP16, id="128-fp16", marks=pytest.mark.extended), pytest.param(64, BF, id="64-bf16", marks=pytest.mark.extended),
          pytest.param(72, BF, id="72-bf16"), pytest.param(72, FP16, id="72-fp16", marks=pytest.mark.extended),
          pytest.param(40, BF, id="40-bf16", marks=pytest.mark.extended), pytest.param(40, FP16, id="40-fp16")]


@pytest.mark.parametrize("D,dt", _SWEEP)
def test_block_patterns(D, dt):
    """B 2, Sq 640 / Sk 1024, H 4 / Hk 2: every pattern with and without causal, forward and backward, against fp64"""
    _block(D, dt, 640, 1024, PATTERNS)


@pytest.mark.parametrize("D,dt", [(128, BF), (64, FP16), pytest.param(72, BF, marks=pytest.mark.extended),
                                  pytest.param(40, FP16, marks=pytest.mark.extended)])
def test_partial_tail_blocks(D, dt):
    """Sq 320 / Sk 333: the last query block holds 64 rows, the last key block 77 keys"""
    _block(D, dt, 320, 333, ("alternate", "last", "first_last", "sibling_dark", "per_head", "partly_outside"))


@pytest.mark.parametrize("D,dt", [(128, BF), pytest.param(64, FP16, marks=pytest.mark.extended)])
def test_eight_heads_in_groups_of_four(D, dt):
    """H 8 / Hk 2: per-head masks inside a K/V group of four (the dK/dV item walk steps over (tile, head) pairs)"""
    _block(D, dt, 640, 1024, ("per_head", "alternate"), heads=(8, 2))


BANDS = tuple((True, dict(window=(200, -1), mask_shift=s)) for s in (0, 150, -150)) + \
    tuple((False, dict(window=(130, 70), mask_shift=s)) for s in (0, 200, -100))


@pytest.mark.parametrize("band", range(len(BANDS)), ids=[f"{'causal' if c_ else 'full'}-w{b_['window'][0]}_{b_['window'][1]}-shift{b_['mask_shift']}"
                                                          for c_, b_ in BANDS])
@pytest.mark.parametrize("D,dt", [pytest.param(128, BF, id="128-bf16"), pytest.param(64, FP16, id="64-fp16"),
                                  pytest.param(72, FP16, id="72-fp16", marks=pytest.mark.extended),
                                  pytest.param(40, BF, id="40-bf16", marks=pytest.mark.extended)])
def test_masks_under_a_window_and_a_shifted_band(D, dt, band):
    """EVERY pattern under a causal window of 200 keys and under a two-sided one, each with the band in place and moved both ways
    (a non-zero first key of the band, an odd first visited tile, workgroups whose band is empty) — one band per case"""
    _block(D, dt, 640, 1024, PATTERNS, bands=(BANDS[band],))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D,dt", [(128, BF), (64, FP16), pytest.param(72, BF, marks=pytest.mark.extended), pytest.param(40, FP16, marks=pytest.mark.extended)])
def test_an_all_true_mask_gives_the_bits_of_the_unmasked_call(D, dt, causal):
    """the list walk where it skips nothing: out, lse, dq, dk, dv equal, bit for bit, those of the same call without a mask forced
    to the same kernel forms (8 x 32 forward, 7-GEMM dQ, 128-key dK/dV, no dS scratch)"""
    from ring_flash_attn import config

    be, dev = _be(), _dev()
    q, k, v, do = (t.to(dev) for t in _inputs(640, 1024, D, dt, seed=5))
    got = _run(be, q, k, v, do, causal, (torch.ones(1, 1, 5, 8, dtype=torch.bool, device=dev), 0))
    with config.override(fwd_form="8x32", fwd_kv_nsplit=1, dkdv_wide=0, bwd_ds_spill=False):
        plain = _run(be, q, k, v, do, causal, None)
    for name, x, y in zip(NAMES5, got, plain):
        assert torch.equal(x, y), (name, float((x.float() - y.float()).abs().max()))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [128, pytest.param(64, marks=pytest.mark.extended)])
def test_five_aligned_documents_against_cu_seqlens_and_row_ranges(D, causal):
    """one dense row of 1152 tokens = five packed documents of 128-aligned lengths: the block-diagonal mask against the
    cu_seqlens call and against with_row_ranges spelling the same mask"""
    be, dev = _be(), _dev()
    lens = [128, 256, 128, 384, 256]
    S = sum(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    gen = torch.Generator().manual_seed(79 + D)
    mk = lambda h: torch.randn(1, S, h, D, generator=gen).to(BF).to(dev)
    q, k, v, do = mk(H), mk(HK), mk(HK), mk(H)
    doc = torch.bucketize(torch.arange(S), torch.tensor(cu[1:-1]), right=True)
    blk = doc[::128]
    m = (blk.view(-1, 1) == blk.view(1, -1)).view(1, 1, S // 128, S // 128).contiguous().to(dev)
    got = _run(be, q, k, v, do, causal, (m, 0))
    start = torch.tensor(cu)[doc].to(torch.int32).view(1, S).contiguous().to(dev)
    end = torch.tensor(cu)[doc + 1].to(torch.int32).view(1, S).contiguous().to(dev)
    scale = D ** -0.5
    out, lse = torch.empty_like(q), torch.empty((1, H, S), dtype=torch.float32, device=dev)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, row_ranges=(start, end, 0))
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, row_ranges=(start, end, 0))
    ranged = (out, lse, dq, dk, dv)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    pq, pk, pv, pdo = (t[0] for t in (q, k, v, do))
    out, lse = torch.empty_like(pq), torch.empty((H, S), dtype=torch.float32, device=dev)
    kw = dict(softmax_scale=scale, causal=causal, cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=max(lens), max_seqlen_k=max(lens))
    be.fwd(pq, pk, pv, out=out, lse=lse, **kw)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(pdo, out, delta, cu_seqlens_q=cu_t, max_seqlen_q=max(lens))
    dq, dk, dv = torch.empty_like(pq), torch.empty_like(pk), torch.empty_like(pv)
    be.bwd(pdo, pq, pk, pv, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
    torch.cuda.synchronize()
    packed = tuple(t.unsqueeze(0) for t in (out, lse, dq, dk, dv))
    bad = _failures(got, packed, "vs cu_seqlens.") + _failures(got, ranged, "vs row ranges.")
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("D,dt", [(128, BF), pytest.param(72, FP16, marks=pytest.mark.extended)])
def test_accumulate_mode_and_the_two_phase_backward(D, dt):
    """keys [0, 384) and [384, 1024) as two masked block calls (k_blk0 = 0 and 3) merged through out_acc / lse_acc, then
    RFA_BWD_COMPUTE / RFA_BWD_REDUCE per block `+=` into fp32 accumulators that hold a known value: against the one fp64
    attention over all keys.  A `dkdv_nsplit` asked for through the configuration is IGNORED by a masked call (it runs the
    RFA_DKDV_128 plan, which has no shares): the results with 1 and with 4 asked for are the same bits"""
    from ring_flash_attn import _C, config

    be, dev = _be(), _dev()
    sq, sk, h = 640, 1024, 384
    q, k, v, do = _inputs(sq, sk, D, dt, seed=9)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    m, _ = _pattern("per_head", 5, 8)
    ref = MB.single_device(q, k, v, do, MB.expand(m, B, H, sq, sk, True))
    md = m.to(dev)
    scale = D ** -0.5
    blocks = ((slice(0, h), sk - h, 0), (slice(h, sk), 0, 3))       # (keys, mask_shift, k_blk0): the causal diagonal is the whole call's
    bad, runs = [], []
    for nsplit in (1, 4):
        out_acc = torch.empty(q.shape, dtype=torch.float32, device=dev)
        lse_acc = torch.empty((B, H, sq), dtype=torch.float32, device=dev)
        for n, (ks, shift, k0) in enumerate(blocks):
            be.fwd(qd, kd[:, ks], vd[:, ks], softmax_scale=scale, causal=True, out_acc=out_acc, lse_acc=lse_acc, acc_init=n == 0,
                   block_mask=(md, k0), **({"mask_shift": shift} if shift else {}))
        out = out_acc.to(dt)
        lse = lse_acc.clone()
        delta = torch.empty_like(lse)
        be.bwd_preprocess(dod, out, delta)
        acc = [torch.full(t.shape, 0.5, dtype=torch.float32, device=dev) for t in (q, k, v)]
        with config.override(dkdv_nsplit=nsplit):
            for ks, shift, k0 in blocks:
                kw = dict(softmax_scale=scale, causal=True, dq_acc=acc[0], dk_acc=acc[1][:, ks], dv_acc=acc[2][:, ks],
                          block_mask=(md, k0), **({"mask_shift": shift} if shift else {}))
                part = be.bwd(dod, qd, kd[:, ks], vd[:, ks], lse, delta, phases=_C.BWD_COMPUTE, **kw)
                be.bwd(dod, qd, kd[:, ks], vd[:, ks], lse, delta, phases=_C.BWD_REDUCE, partials=part, **kw)
        torch.cuda.synchronize()
        lse_got = torch.where(torch.isinf(lse_acc), torch.full_like(lse_acc, float("inf")), lse_acc)     # (-inf: a row without a key)
        runs.append((out_acc, lse_got, acc[0], acc[1], acc[2]))
        if nsplit == 1:
            bad += _failures((out_acc, lse_got, acc[0] - 0.5, acc[1] - 0.5, acc[2] - 0.5), ref, "two blocks.",
                             ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring"))
    assert not bad, "; ".join(bad[:12])
    for name, x, y in zip(NAMES5, *runs):
        assert torch.equal(x, y), f"dkdv_nsplit changed {name} of a masked call"


def test_two_runs_of_one_masked_backward_give_the_same_bits():
    be, dev = _be(), _dev()
    q, k, v, do = (t.to(dev) for t in _inputs(640, 1024, 128, BF, seed=13))
    m, k0 = _pattern("per_head", 5, 8)
    a = _run(be, q, k, v, do, True, (m.to(dev), k0))
    b = _run(be, q, k, v, do, True, (m.to(dev), k0))
    for name, x, y in zip(NAMES5, a, b):
        assert torch.equal(x, y), name


def _multi_cases(W):
    pats = [dict(pattern="docs", causal=True), dict(pattern="bigbird", causal=False), dict(pattern="per_head", causal=True)]
    cases = []
    for kind, forms in (("ring", (None,)), ("zigzag", ("ring", "gather", "gather_ps"))):
        for pack in (None, "kv", "qkv"):
            for n, p in enumerate(pats):
                form = forms[(n + (0 if pack is None else 1 if pack == "kv" else 2)) % len(forms)]
                cases.append(dict(kind=kind, W=W, S=256, D=128 if n != 1 else 64, pack=pack, **({"form": form} if form else {}), **p))
    return cases


@pytest.mark.parametrize("W", [2, 4])
def test_the_six_functions_over_ranks_sharing_the_gpu(W):
    """ring_ and zigzag_ring_flash_attn_{,kvpacked_,qkvpacked_}func with the ranks sharing cuda:0 (host staging), S = 256 rows per
    rank: block-diagonal documents under causal, a non-causal window + global + random mask, per-head masks — each against ONE
    single-device fp64 attention with the expanded mask"""
    import _blockmask_worker as MW

    errs, notes = MW.run_world(W, _multi_cases(W), True, free_port(), limit_s=240)
    print("\n".join(notes))
    assert not errs, "\n".join(errs[:20])
