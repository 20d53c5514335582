"""The per-head max attention logit on the device: csrc/rfa_maxlogit.hip through HipBackend.max_logit and
ring_flash_attn.with_max_logit against the fp64 reference of tests/_maxlogit_backend.py (einsum of the 16-bit inputs in fp64,
masked with tests/_blockref.visible, amax), on planted inputs that make a mask error visible.

Tolerance (derived, tests/_maxlogit_backend.tolerance): |got - ref| <= (D + 2) 2^-23 softmax_scale max_visible sum_d |q_d||k_d|,
the fp32 accumulation bound of a D-term dot product for any summation order with a factor 2; -inf compares exactly.  Every
test prints the worst |err| / tol it saw (profiles/max_logit.md quotes them)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _bandref as BR                            # noqa: E402
import _maxlogit_backend as ML                   # noqa: E402
import _maxlogit_worker as MW                    # noqa: E402
from _blockref import visible                    # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
H, HK = 4, 2
NEG_INF = float("-inf")
LENS = (1, 31, 33, 64, 0, 130, 257, 300, 777)        # the packed batch of tests/test_gpu_band_varlen.py and an empty sequence


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _new(n=H, fill=NEG_INF):
    return torch.full((n,), fill, dtype=torch.float32, device=_dev())


def _check(tag, got, q, k, scale, **ref_kw):
    """got (H,) against the fp64 reference of the block (q, k on the device); prints and returns the worst |err| / tol"""
    ref = ML.head_max(ML.row_max(q, k, scale, **ref_kw))
    tol = ML.tolerance(q.shape[-1], scale, ML.head_max(ML.row_max(q, k, scale, absolute=True, **ref_kw)))
    ratio = ML.close(got, ref, tol)
    print(f"max_logit {tag}: ref {[round(x, 4) for x in ref.tolist()]} worst |err| / tol {ratio:.4f}")
    return ratio


def _geometry_inputs(g, D, dtype, seed=0):
    gen = torch.Generator().manual_seed(7700 + seed + D)
    q = torch.randn(g.B, g.lq, H, D, generator=gen)
    k = torch.randn(g.B, g.lk, HK, D, generator=gen)
    ML.plant_dense(q, k, visible(g.lq, g.lk, g.causal, g.window, g.shift))
    return q.to(dtype).to(_dev()), k.to(dtype).to(_dev())


def _run_geometry(g, D, dtype):
    be = _be()
    q, k = _geometry_inputs(g, D, dtype)
    scale = D ** -0.5
    m = _new(fill=123.0)
    be.max_logit(q, k, m, softmax_scale=scale, accumulate=False, **g.band)
    return _check(f"{g.name} D{D} {dtype}", m, q, k, scale, causal=g.causal, window=g.window, shift=g.shift)


# ---------------------------------------------------------------------------------------------- the kernel against fp64
_CORE_GEOS = ("two-sided+65",)


@pytest.mark.parametrize("name", [pytest.param(g.name, marks=() if g.name in _CORE_GEOS else _EXT) for g in BR.GEOMETRIES])
def test_every_band_geometry_head_dim_128(name):
    _run_geometry(BR.BY_NAME[name], 128, BF)


_SWEEP_GEOS = [g.name for g in BR.GEOMETRIES if g.cls.startswith("corner") or g.cls in ("hi-live", "lo-live")] + \
              ["causal+33", "wl130+401", "rows200-keys4096-100"]


@pytest.mark.parametrize("dtype", [BF, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [40, 64, 72, 96, 136, 192, 256])
@pytest.mark.parametrize("name", _SWEEP_GEOS)
@_EXT
def test_head_dims_and_dtypes_on_the_edge_geometries(name, D, dtype):
    _run_geometry(BR.BY_NAME[name], D, dtype)


@pytest.mark.parametrize("name,D,dtype", [("wl130+401", 192, FP16), ("hi-live", 40, BF), ("corner-lo", 256, BF), ("lo-live", 64, FP16)])
def test_head_dims_and_dtypes_core(name, D, dtype):
    _run_geometry(BR.BY_NAME[name], D, dtype)


def test_all_negative_logits_do_not_report_the_zero_padding():
    """q = |randn|, k = -|randn|, 100 rows against 77 keys (a partial last tile, a partial workgroup), D 72 (zeroed chunks):
    every true logit is negative; keys behind lk and columns behind D read as zero — a leak reports 0"""
    be, dev = _be(), _dev()
    gen = torch.Generator().manual_seed(5)
    for dtype in (BF, FP16):
        q = torch.randn(1, 100, H, 72, generator=gen).abs().to(dtype).to(dev)
        k = (-torch.randn(1, 77, HK, 72, generator=gen).abs()).to(dtype).to(dev)
        m = _new()
        be.max_logit(q, k, m, softmax_scale=72 ** -0.5, causal=False)
        assert bool((m < -1.0).all()), m
        _check(f"all-negative {dtype}", m, q, k, 72 ** -0.5)
        m = _new()
        be.max_logit(q, k, m, softmax_scale=72 ** -0.5, causal=True)
        _check(f"all-negative causal {dtype}", m, q, k, 72 ** -0.5, causal=True)


def test_empty_band_accumulate_and_head_offset():
    be = _be()
    g = BR.BY_NAME["corner-hi-1"]                                      # nothing visible
    q, k = _geometry_inputs(g, 128, BF)
    m = _new(fill=5.0)
    be.max_logit(q, k, m, softmax_scale=0.1, accumulate=True, **g.band)
    assert torch.equal(m, _new(fill=5.0))
    be.max_logit(q, k, m, softmax_scale=0.1, accumulate=False, **g.band)
    assert torch.equal(m, _new())
    # no rows / no keys
    m = _new(fill=1.0)
    be.max_logit(q[:, :0], k, m, softmax_scale=0.1, causal=False, accumulate=False)
    assert torch.equal(m, _new())
    m = _new(fill=1.0)
    be.max_logit(q, k[:, :0], m, softmax_scale=0.1, causal=False, accumulate=False)
    assert torch.equal(m, _new())
    # accumulate = max(dst, new); overwrite = new
    g = BR.BY_NAME["causal+33"]
    q, k = _geometry_inputs(g, 128, BF)
    new = _new()
    be.max_logit(q, k, new, softmax_scale=0.05, accumulate=False, **g.band)
    assert bool(torch.isfinite(new).all())
    pre = new.clone()
    pre[0] += 1.0
    pre[1] -= 1.0
    pre[2] = NEG_INF
    pre[3] = 1e9
    acc = pre.clone()
    be.max_logit(q, k, acc, softmax_scale=0.05, accumulate=True, **g.band)
    assert torch.equal(acc, torch.maximum(pre, new))
    # head0 writes only its slice
    wide = _new(n=11, fill=-7.0)
    be.max_logit(q, k, wide, softmax_scale=0.05, accumulate=False, head0=5, **g.band)
    assert torch.equal(wide[5:9], new) and bool((wide[:5] == -7.0).all()) and bool((wide[9:] == -7.0).all())
    with pytest.raises(ValueError):
        be.max_logit(q, k, _new(n=6), softmax_scale=0.05, head0=3, **g.band)


@pytest.mark.parametrize("halves", [0, 1, 2], ids=["whole", "front", "back"])
@pytest.mark.parametrize("n", [-1, 0, 1, 2])
def test_packed_batch_with_lit_cut_dark_and_empty_sequences(n, halves):
    """ONE packed launch: sequences wholly inside the window, cut by it, wholly dark (n = 2: all three kinds together) and an
    empty one; with the half selectors every sequence is the front / back half of one twice as long"""
    be, dev = _be(), _dev()
    D, causal, window = 128, True, (130, 0)
    mul = 2 if halves else 1
    cu = [0]
    for l in LENS:
        cu.append(cu[-1] + mul * l)
    gen = torch.Generator().manual_seed(9100 + n + 10 * halves)
    q = torch.randn(cu[-1], H, D, generator=gen)
    k = torch.randn(cu[-1], HK, D, generator=gen)
    if not halves:
        ML.plant_packed(q, k, cu, lambda b, L: visible(L, L, causal, window, n * L))
    else:
        # the other half holds junk far above every logit of the half that is looked at
        for b, l in enumerate(LENS):
            s = cu[b] + (l if halves == 1 else 0)
            q[s:s + l] = 30.0 / D ** 0.5
            k[s:s + l] = 30.0 / D ** 0.5
    q, k = q.to(BF).to(dev), k.to(BF).to(dev)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    vl = dict(cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=mul * max(LENS), max_seqlen_k=mul * max(LENS))
    m = _new()
    be.max_logit(q, k, m, softmax_scale=D ** -0.5, causal=causal, window=window, mask_shift_lens=n, q_half=halves, k_half=halves,
                 **vl)
    if n == -1:
        assert torch.equal(m, _new())                                 # every sequence is dark
    _check(f"packed n={n} halves={halves}", m, q, k, D ** -0.5, causal=causal, window=window, shift_lens=n, cu_seqlens=cu,
           q_half=halves, k_half=halves)


def test_a_block_cut_into_block_calls_accumulates_to_the_same_bits():
    """rows cut at 200, keys at 333 (both unaligned), mask_shift adjusted: the four block calls max-accumulate to the bits of
    the one call; two runs give the same bits"""
    be = _be()
    for name, D in (("causal+33", 128), ("two-sided+65", 128), ("wl130+401", 64), ("causal+257", 256)):
        g = BR.BY_NAME[name]
        q, k = _geometry_inputs(g, D, BF, seed=1)
        scale = D ** -0.5
        one, again, parts = _new(), _new(), _new()
        be.max_logit(q, k, one, softmax_scale=scale, **g.band)
        be.max_logit(q, k, again, softmax_scale=scale, **g.band)
        assert torch.equal(one, again), name
        for r0, r1 in ((0, 200), (200, g.lq)):
            for c0, c1 in ((0, 333), (333, g.lk)):
                shift = g.off - c0 + r0 - ((c1 - c0) - (r1 - r0))
                be.max_logit(q[:, r0:r1], k[:, c0:c1], parts, softmax_scale=scale, causal=g.causal, window=g.window,
                             mask_shift=shift)
        assert torch.equal(one, parts), (name, one, parts)
        _check(f"decomposition {name}", one, q, k, scale, causal=g.causal, window=g.window, shift=g.shift)


# ---------------------------------------------------------------------------------------------- with_max_logit, one device
def _pub_inputs(Sq, Sk, D, dtype=BF, Hk=HK, window=(-1, -1), causal=True, seed=0):
    gen = torch.Generator().manual_seed(300 + seed + D + Sq)
    q = torch.randn(2, Sq, H, D, generator=gen)
    k = torch.randn(2, Sk, Hk, D, generator=gen)
    v = torch.randn(2, Sk, Hk, D, generator=gen)
    ML.plant_dense(q, k, visible(Sq, Sk, causal, window))
    return tuple(t.to(dtype).to(_dev()) for t in (q, k, v))


def _grads(fn, tensors, *a, **kw):
    ts = [t.clone().requires_grad_(True) for t in tensors]
    out = fn(*ts, *a, **kw)
    gen = torch.Generator().manual_seed(1)
    out.backward(torch.randn(out.shape, generator=gen).to(out.dtype).to(out.device))
    return (out.detach(), *(t.grad for t in ts))


def _same(a, b, tag):
    for x, y in zip(a, b):
        assert torch.equal(x, y), tag


@pytest.mark.parametrize("D", [64, 128, 256])
def test_with_max_logit_dense_calls_leave_out_and_gradients_bit_identical(single_rank_group, D):
    import ring_flash_attn as R

    _be()
    scale = D ** -0.5
    for Sq, Sk, causal, window in ((100, 100, True, (-1, -1)), (70, 50, True, (-1, -1)), (50, 70, False, (-1, -1)),
                                   (100, 100, True, (30, 0)), (100, 100, False, (20, 9))):
        q, k, v = _pub_inputs(Sq, Sk, D, window=window, causal=causal)
        m = _new()
        kw = dict(causal=causal, window_size=window)
        fn = R.ring_flash_attn_func
        _same(_grads(R.with_max_logit(fn, m), (q, k, v), **kw), _grads(fn, (q, k, v), **kw), (D, Sq, Sk))
        _check(f"with_max_logit D{D} {Sq}x{Sk} causal={causal} w={window}", m, q, k, scale, causal=causal, window=window)


def test_with_max_logit_packed_entries_dropout_alibi_softcap_and_varlen(single_rank_group):
    import ring_flash_attn as R

    _be()
    D = 64
    scale = D ** -0.5
    q, k, v = _pub_inputs(100, 100, D)
    ref_kw = dict(causal=True)
    # kvpacked / qkvpacked
    m = _new()
    kv = torch.stack([k, v], dim=2)
    _same(_grads(R.with_max_logit(R.ring_flash_attn_kvpacked_func, m), (q, kv), causal=True),
          _grads(R.ring_flash_attn_kvpacked_func, (q, kv), causal=True), "kvpacked")
    _check("kvpacked", m, q, k, scale, **ref_kw)
    q4, k4, v4 = _pub_inputs(100, 100, D, Hk=H, seed=2)
    qkv = torch.stack([q4, k4, v4], dim=2)
    m = _new()
    _same(_grads(R.with_max_logit(R.zigzag_ring_flash_attn_qkvpacked_func, m), (qkv,), causal=True),
          _grads(R.zigzag_ring_flash_attn_qkvpacked_func, (qkv,), causal=True), "qkvpacked")
    _check("qkvpacked", m, q4, k4, scale, **ref_kw)
    # alibi_slopes and a with_softcap result: the raw logit, and the call's own results untouched
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625], device=_dev())
    m = _new()
    _same(_grads(R.with_max_logit(R.ring_flash_attn_func, m), (q, k, v), causal=True, alibi_slopes=slopes),
          _grads(R.ring_flash_attn_func, (q, k, v), causal=True, alibi_slopes=slopes), "alibi")
    _check("alibi", m, q, k, scale, **ref_kw)
    capped = R.with_softcap(R.ring_flash_attn_func, 20.0)
    m = _new()
    _same(_grads(R.with_max_logit(capped, m), (q, k, v), causal=True), _grads(capped, (q, k, v), causal=True), "softcap")
    _check("softcap", m, q, k, scale, **ref_kw)
    sunk = R.with_sinks(R.ring_flash_attn_func, torch.zeros(H, device=_dev()))
    m = _new()
    _same(_grads(R.with_max_logit(sunk, m), (q, k, v), causal=True), _grads(sunk, (q, k, v), causal=True), "sinks")
    _check("sinks", m, q, k, scale, **ref_kw)
    # dropout: the mask is drawn per call, so only the tensor is compared
    m = _new()
    R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, dropout_p=0.1, causal=True)
    _check("dropout", m, q, k, scale, **ref_kw)
    # packed input with an empty sequence, windowed
    lens = [40, 0, 33, 27]
    cu = [0, 40, 40, 73, 100]
    gen = torch.Generator().manual_seed(77)
    pq, pk, pv = (torch.randn(100, h, D, generator=gen) for h in (H, HK, HK))
    ML.plant_packed(pq, pk, cu, lambda b, L: visible(L, L, True, (20, 0)))
    pq, pk, pv = (t.to(BF).to(_dev()) for t in (pq, pk, pv))
    cu_t = torch.tensor(cu, dtype=torch.int32, device=_dev())
    m = _new()
    fn = R.ring_flash_attn_varlen_func
    kw = dict(causal=True, window_size=(20, 0))
    _same(_grads(R.with_max_logit(fn, m), (pq, pk, pv), cu_t, max(lens), **kw), _grads(fn, (pq, pk, pv), cu_t, max(lens), **kw), "varlen")
    _check("varlen", m, pq, pk, scale, causal=True, window=(20, 0), cu_seqlens=cu)


# ---------------------------------------------------------------------------------------------- the schedules, 2 and 4 ranks
def _worlds(W):
    S = 128
    lens = [32 * W, 96 * W, 128 * W]
    return [dict(kind="ring", W=W, S=S, causal=True), dict(kind="zigzag", W=W, S=S, causal=True, form="ring"),
            dict(kind="stripe", W=W, S=S, causal=True, window=(S + 37, 0)),
            dict(kind="ring_varlen", W=W, S=S, causal=False, lens=lens), dict(kind="zigzag_varlen", W=W, S=S, causal=True, lens=lens),
            dict(kind="llama3", W=W, S=S, causal=True, stride=1, groups=2), dict(kind="zigzag_llama3", W=W, S=S, causal=True)]


@pytest.mark.parametrize("W", [2, 4])
def test_one_function_per_family_over_ranks_sharing_the_gpu(W):
    """the MAX over the ranks is bit-identical to one be.max_logit call on the unsharded tensors; each rank's partial is within
    the tolerance of the fp64 reference on its rows (tests/_maxlogit_worker.py)"""
    errs, notes = MW.run_world(W, _worlds(W), True, free_port(), limit_s=300)
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
