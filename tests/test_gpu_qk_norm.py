"""The fused QK RMSNorm + rotary kernels on the device (`-m gpu`): csrc/rfa_qknorm.hip through
ring_flash_attn.apply_qk_norm_rotary and HipBackend.qk_norm_rotary_fwd / _bwd.

Shapes: B 2, S 38, H 3 / Hk 1, P 80 table rows plus a NaN row, the (D, R, rot_offset, pairing) rows of COMBOS, bf16 and fp16,
fp32 and io-dtype tables and weights in all four mixes, one packed case of T = 77.  Against the textbook formulas in fp64
(tests/_qknorm_backend.py: reference), elementwise, with DERIVED bounds; u = 2^-8 (bf16) / 2^-11 (fp16), `half` the io dtype's
half subnormal step:
    forward  |err| <= max(u |ref|, half) + 2^-19 Mf      Mf = |y1 c| + |y2 s| (pass-through: |y|)
    dx       |err| <= max(u |ref|, half) + 2^-18 Mb      Mb = rstd (|g|mag |a| + |xh| (1/D) sum_c |g|mag |a| |xh|)
    dw       |err| <= (n + 24) 2^-24 T  (fp32 out of the C ABI)       T = sum |g|mag |xh|
The implemented order (csrc/rfa_qknorm.hip, SUMMATION ORDERS) keeps ONE 16-byte chunk per lane — the partner chunk of the
halves pairing comes by a shuffle — so that the row sums do not depend on what is rotated: 8 in-lane squares and a butterfly of
depth <= 5 are 13 roundings, fewer than the 21 the forward bound was derived for (16 in-lane squares); the other steps (rstd,
three roundings to y, rot()) are the derivation's, so the constants 2^-19 and 2^-18 stand as stated and are not widened.
n = the longest sequential chain of a column's sum for the tensor's own item count (_qknorm_backend.kernel_chain): a lane's
walk, the workgroup's 256/G lane groups, a run of ceil(nparts/16) partials, the 16 runs.
Bit identities: map mode == explicit positions, q and k together == one at a time (the weight gradients too), a strided view of a
qkv tensor == its contiguous copy, tables of cos 1 / sin 0 == the norm-only call, two runs (dw included), autograd == the direct
calls.  Inputs scaled by 0.01 and 30; an all-zero row; eps = 0 with partly filled workgroups; NaN guards around inputs and sentinels around outputs; weight
gradients over several workgroups with a ragged last one and over a walk of two steps; a batch entry past 4 GiB; W = 2 / 4
processes sharing the GPU with the ring / zigzag / stripe schedule behind the call."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                               # noqa: E402
import _farview as FV                                        # noqa: E402
import _qknorm_worker as QW                                  # noqa: E402
from _qknorm_backend import kernel_chain, reference          # noqa: E402

pytestmark = pytest.mark.gpu

B, S, H, HK, P = 2, 38, 3, 1, 80
#         D    R   rot_offset  interleaved
COMBOS = [(128, 128, 0, False), (64, 64, 0, False), (256, 256, 0, False), (192, 64, 128, False), (72, 32, 0, False),
          (40, 16, 8, False), (40, 8, 8, True), (8, 8, 0, True), (128, 0, 0, False)]
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # half the spacing of the subnormal numbers
EPS = 1e-6


def _dev():
    return torch.device("cuda:0")


def _tables(Rw, dtype, rows=P):
    """cos / sin of `rows` positions plus ONE more row that no position uses, filled with NaN; Rw == 0: no tables"""
    if not Rw:
        return None, None
    ang = torch.arange(rows, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(Rw // 2, dtype=torch.float64) / (Rw // 2)))
    pad = torch.full((1, Rw // 2), float("nan"), dtype=torch.float64)
    return torch.cat([ang.cos(), pad]).to(dtype).to(_dev()), torch.cat([ang.sin(), pad]).to(dtype).to(_dev())


def _cut(t):
    return None if t is None else t[:P]


def _qk(D, dtype, seed=5, lead=(B, S), scale=1.0, heads=(H, HK)):
    g = torch.Generator().manual_seed(seed)
    return tuple((scale * torch.randn(*lead, h, D, generator=g)).to(dtype).to(_dev()) for h in heads)


def _w(D, dtype, seed=4):
    g = torch.Generator().manual_seed(seed)
    return tuple((1.0 + 0.25 * torch.randn(D, generator=g)).to(dtype).to(_dev()) for _ in range(2))


def _positions(seed=3, lead=(B, S)):
    """every position below P at least possible, the NaN row (index P) never"""
    return torch.randint(0, P, lead, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(_dev())


def _check(what, got, ref, mag, dtype, fac):
    """one rounding to the io dtype plus the fp32 share fac * mag; prints the largest err / bound (the result is rounded, so the
    fp32 share cannot be told apart from the rounding: an element counts with its whole error)"""
    err = (got.detach().double().cpu() - ref).abs()
    lim = (U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + fac * mag
    worst = (err - lim).max().item()
    print(f"{what}: max|err| {err.max().item():.3e}, worst err - bound {worst:.3e}, worst err / bound {(err / lim).max().item():.4f}")
    assert not torch.isnan(got).any(), f"{what}: NaN in the result"
    assert worst <= 0, f"{what}: |err| exceeds the bound by {worst:.3e}"


def _check_dw(what, got, ref, T, n):
    assert got.dtype == torch.float32
    err = (got.double().cpu() - ref).abs()
    lim = (n + 24) * 2.0 ** -24 * T
    print(f"{what}: max|err| {err.max().item():.3e}, chain {n}, worst err / (2^-24 T) {(err / (2.0 ** -24 * T)).max().item():.3f}, "
          f"of the bound {(err / lim).max().item():.4f}")
    assert not torch.isnan(got).any() and bool((err <= lim).all()), f"{what}: {(err - lim).max().item():.3e} over (n + 24) 2^-24 T"


def _direct(be, xs, ws, cos, sin, douts=None, want_dw=True, **kw):
    """the two backend calls on fresh outputs: ([y], [dx], [dw fp32])"""
    ys = [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in xs]
    be.qk_norm_rotary_fwd(list(xs), ys, list(ws), cos, sin, **kw)
    if douts is None:
        return ys, None, None
    dxs = [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in xs]
    dws = [torch.full((x.shape[-1],), float("nan"), dtype=torch.float32, device=x.device) if want_dw else None for x in xs]
    be.qk_norm_rotary_bwd(list(xs), list(douts), dxs, list(ws), dws, cos, sin, **kw)
    return ys, dxs, dws


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("aux", ["fp32", "io", "tables32-weights16", "tables16-weights32"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,Rw,ro,inter", COMBOS)
def test_forward_backward_and_bit_identities(single_rank_group, D, Rw, ro, inter, dtype, aux):
    import ring_flash_attn as R
    from ring_flash_attn._common import zigzag_map
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    assert be.name == "hip" and be.serves_qk_norm
    # tables and weights in fp32 or the io dtype, every mix of the two (fp32 tables with io-dtype weights: a bf16 model)
    tdt = torch.float32 if aux in ("fp32", "tables32-weights16") else dtype
    adt = torch.float32 if aux in ("fp32", "tables16-weights32") else dtype
    cos, sin = _tables(Rw, tdt)
    wq, wk = _w(D, adt)
    q, k = _qk(D, dtype)
    dqo, dko = _qk(D, dtype, seed=6)
    pos = _positions() if Rw else None
    kw = dict(interleaved=inter, rot_offset=ro, eps=EPS, weight_offset=0.0)
    (qo, ko), (dq, dk), (dwq, dwk) = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), positions=pos, **kw)
    for name, x, w, out, dout, dx, dw in (("q", q, wq, qo, dqo, dq, dwq), ("k", k, wk, ko, dko, dk, dwk)):
        r = reference(x, w, _cut(cos), _cut(sin), None if pos is None else pos.cpu(), inter, ro, EPS, 0.0, dout=dout)
        _check(f"{name} forward", out, r["y"], r["Mf"], dtype, 2.0 ** -19)
        _check(f"d{name}", dx, r["dx"], r["Mb"], dtype, 2.0 ** -18)
        _check_dw(f"dw_{name}", dw, r["dw"], r["T"], kernel_chain(x.shape[0] * x.shape[1] * x.shape[2], D))
    # autograd == the direct calls; the weight gradient is the fp32 sum rounded once to the weight's dtype
    leaves = [t.clone().requires_grad_(True) for t in (q, k, wq, wk)]
    aq, ak = R.apply_qk_norm_rotary(*leaves, cos, sin, positions=pos, **kw)
    torch.autograd.backward([aq, ak], [dqo, dko])
    assert _same((aq, ak, leaves[0].grad, leaves[1].grad), (qo, ko, dq, dk))
    assert leaves[2].grad.dtype == adt and _same((leaves[2].grad, leaves[3].grad), (dwq.to(adt), dwk.to(adt)))
    # two runs give the same bits, dw included
    again = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), positions=pos, **kw)
    assert _same(again[0], (qo, ko)) and _same(again[1], (dq, dk)) and _same(again[2], (dwq, dwk))
    # q and k together == one at a time — the weight gradients too
    for x, w, dout, want in ((q, wq, dqo, (qo, dq, dwq)), (k, wk, dko, (ko, dk, dwk))):
        y1, dx1, dw1 = _direct(be, (x,), (w,), cos, sin, (dout,), positions=pos, **kw)
        assert _same((y1[0], dx1[0], dw1[0]), want)
    # without a dweight the input gradients are the same bits
    assert _same(_direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), want_dw=False, positions=pos, **kw)[1], (dq, dk))
    # a strided view of a qkv tensor == its contiguous copy (MHA: three heads each), gradients in a strided buffer too
    g = torch.Generator().manual_seed(9)
    qkv, dqkv = (torch.randn(B, S, 3, H, D, generator=g).to(dtype).to(_dev()) for _ in range(2))
    sv = _direct(be, (qkv[:, :, 0], qkv[:, :, 1]), (wq, wk), cos, sin, (dqkv[:, :, 0], dqkv[:, :, 1]), positions=pos, **kw)
    cv = _direct(be, (qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous()), (wq, wk), cos, sin,
                 (dqkv[:, :, 0].contiguous(), dqkv[:, :, 1].contiguous()), positions=pos, **kw)
    assert all(_same(a, b) for a, b in zip(sv, cv))
    if not Rw:
        return
    # tables of cos 1 / sin 0 == the norm-only call, forward and backward
    ones, zeros = torch.ones_like(cos), torch.zeros_like(sin)
    unit = _direct(be, (q, k), (wq, wk), ones, zeros, (dqo, dko), positions=pos, **kw)
    bare = _direct(be, (q, k), (wq, wk), None, None, (dqo, dko), **dict(kw, rot_offset=0))
    assert all(_same(a, b) for a, b in zip(unit, bare))
    # map mode == explicit positions of the same values: rank 1 of a 2-rank zigzag (chunks 1 and 2 of 19 rows)
    pm = zigzag_map(1, 2, S // 2)
    zz = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=1, world_size=2, device=_dev())
    assert zz.tolist() == list(range(19, 57))
    by_map = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), pos_map=pm, **kw)
    by_pos = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), positions=zz, **kw)
    assert all(_same(a, b) for a, b in zip(by_map, by_pos))
    assert not torch.equal(by_map[0][0], qo)
    off5 = R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, offset=5, **kw)
    assert torch.equal(off5, R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, offset=5, **kw,
                                                    positions=torch.arange(S, dtype=torch.int32, device=_dev())))
    plain = R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, **kw)
    for f in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        assert torch.equal(R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, layout=f, **kw), plain)


@pytest.mark.parametrize("scale", [0.01, 30.0])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,Rw,ro,inter", [(128, 128, 0, False), (40, 8, 8, True)])
def test_scaled_inputs_and_a_weight_offset(single_rank_group, D, Rw, ro, inter, dtype, scale):
    """inputs scaled by 0.01 and by 30 with Gemma-3's weight_offset = 1 (weights around 0): the same bounds"""
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    cos, sin = _tables(Rw, torch.float32)
    wq, wk = (w - 1.0 for w in _w(D, torch.float32))
    q, k = _qk(D, dtype, scale=scale)
    dqo, dko = _qk(D, dtype, seed=6, scale=scale)
    pos = _positions()
    kw = dict(interleaved=inter, rot_offset=ro, eps=EPS, weight_offset=1.0)
    (qo, ko), (dq, dk), (dwq, dwk) = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), positions=pos, **kw)
    for name, x, w, out, dout, dx, dw in (("q", q, wq, qo, dqo, dq, dwq), ("k", k, wk, ko, dko, dk, dwk)):
        r = reference(x, w, _cut(cos), _cut(sin), pos.cpu(), inter, ro, EPS, 1.0, dout=dout)
        _check(f"{name} forward x{scale}", out, r["y"], r["Mf"], dtype, 2.0 ** -19)
        _check(f"d{name} x{scale}", dx, r["dx"], r["Mb"], dtype, 2.0 ** -18)
        _check_dw(f"dw_{name} x{scale}", dw, r["dw"], r["T"], kernel_chain(x.shape[0] * x.shape[1] * x.shape[2], D))


@pytest.mark.parametrize("D,Rw,ro,inter", [(128, 128, 0, False), (40, 8, 8, True), (72, 0, 0, False)])
def test_eps_zero_with_partly_filled_workgroups(single_rank_group, D, Rw, ro, inter):
    """eps = 0 is served.  228 (row, head)s of q and 76 of k fill no whole number of workgroups (16 or 32 items each): the lane
    groups past a tensor's end hold zeros, whose rsqrt(0) = inf must reach neither dx nor — through 0 * inf — the weight
    gradient their lanes accumulate.  Forward, dx and dw against the fp64 reference with eps = 0, the same bounds."""
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    dtype = torch.bfloat16
    cos, sin = _tables(Rw, torch.float32)
    wq, wk = _w(D, dtype)
    q, k = _qk(D, dtype)
    dqo, dko = _qk(D, dtype, seed=6)
    pos = _positions() if Rw else None
    kw = dict(interleaved=inter, rot_offset=ro, eps=0.0, weight_offset=0.0)
    (qo, ko), (dq, dk), (dwq, dwk) = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), positions=pos, **kw)
    for name, x, w, out, dout, dx, dw in (("q", q, wq, qo, dqo, dq, dwq), ("k", k, wk, ko, dko, dk, dwk)):
        items = x.shape[0] * x.shape[1] * x.shape[2]
        assert items % (256 // max(1, 1 << (D // 8 - 1).bit_length())) != 0                  # a partly filled last workgroup
        r = reference(x, w, _cut(cos), _cut(sin), None if pos is None else pos.cpu(), inter, ro, 0.0, 0.0, dout=dout)
        _check(f"{name} forward, eps 0", out, r["y"], r["Mf"], dtype, 2.0 ** -19)
        _check(f"d{name}, eps 0", dx, r["dx"], r["Mb"], dtype, 2.0 ** -18)
        _check_dw(f"dw_{name}, eps 0", dw, r["dw"], r["T"], kernel_chain(items, D))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_packed_input_and_an_all_zero_row(single_rank_group, dtype):
    import ring_flash_attn as R

    T, D, Rw = 77, 128, 64
    cos, sin = _tables(Rw, torch.float32)
    wq, wk = _w(D, torch.float32)
    q, k = _qk(D, dtype, lead=(T,))
    q[5, 1] = 0                                               # one (row, head) of zeros: eps > 0 gives zeros, never NaN
    pos = _positions(lead=(T,))
    dqo, dko = _qk(D, dtype, seed=6, lead=(T,))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, wq, wk)]
    qo, ko = R.apply_qk_norm_rotary(*leaves, cos, sin, positions=pos, eps=EPS)
    torch.autograd.backward([qo, ko], [dqo, dko])
    assert bool((qo[5, 1] == 0).all()) and not torch.isnan(qo).any() and not torch.isnan(leaves[0].grad).any()
    for name, x, w, out, dout, xl, wl in (("q", q, wq, qo, dqo, leaves[0], leaves[2]), ("k", k, wk, ko, dko, leaves[1], leaves[3])):
        r = reference(x, w, _cut(cos), _cut(sin), pos.cpu(), eps=EPS, dout=dout)
        _check(f"packed {name}", out, r["y"], r["Mf"], dtype, 2.0 ** -19)
        _check(f"packed d{name}", xl.grad, r["dx"], r["Mb"], dtype, 2.0 ** -18)
        _check_dw(f"packed dw_{name}", wl.grad, r["dw"], r["T"], kernel_chain(T * x.shape[1], D))
    # (T, H, D) is the (1, T, H, D) call
    q4, k4 = R.apply_qk_norm_rotary(q.unsqueeze(0), k.unsqueeze(0), wq, wk, cos, sin, positions=pos.view(1, T), eps=EPS)
    assert torch.equal(q4[0], qo.detach()) and torch.equal(k4[0], ko.detach())


@pytest.mark.parametrize("D,Rw,ro,inter", [(128, 128, 0, False), (192, 64, 128, False), (40, 8, 8, True), (72, 0, 0, False)])
def test_guards_around_inputs_and_sentinels_around_outputs(single_rank_group, D, Rw, ro, inter):
    """x and dout are views inside NaN-filled buffers (padding behind every head's D columns, heads beyond H, rows beyond S, a
    further batch entry), the weights sit between NaNs, the tables end in a NaN row; y, dx and dw are views inside buffers
    filled with a sentinel.  The results are the bits of the plain call, no NaN arrives, every sentinel is intact."""
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    dtype = torch.bfloat16
    cos, sin = _tables(Rw, torch.float32)
    q, k = _qk(D, dtype)
    dqo, dko = _qk(D, dtype, seed=6)
    wq, wk = _w(D, torch.float32)
    pos = _positions() if Rw else None
    kw = dict(interleaved=inter, rot_offset=ro, eps=EPS, weight_offset=0.0, positions=pos)
    want = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), **kw)

    def inside(x, fill):
        h = x.shape[2]
        buf = torch.full((B + 1, S + 3, h + 2, D + 8), fill, dtype=x.dtype, device=_dev())
        v = buf[:B, :S, :h, :D]
        if fill != fill:
            v.copy_(x)
        return buf, v

    def vec_inside(w, fill):
        buf = torch.full((D + 16,), fill, dtype=w.dtype, device=_dev())
        v = buf[8:8 + D]
        if fill != fill:
            v.copy_(w)
        return buf, v

    nan = float("nan")
    xs, gs = [inside(t, nan) for t in (q, k)], [inside(t, nan) for t in (dqo, dko)]
    ws = [vec_inside(w, nan) for w in (wq, wk)]
    ys, dxs = [inside(t, 5.0) for t in (q, k)], [inside(t, 5.0) for t in (q, k)]
    dws = [vec_inside(w, 5.0) for w in (wq, wk)]
    be.qk_norm_rotary_fwd([v for _, v in xs], [v for _, v in ys], [v for _, v in ws], cos, sin, **kw)
    be.qk_norm_rotary_bwd([v for _, v in xs], [v for _, v in gs], [v for _, v in dxs], [v for _, v in ws], [v for _, v in dws],
                          cos, sin, **kw)
    for got, ref in ((ys, want[0]), (dxs, want[1]), (dws, want[2])):
        for (buf, v), r in zip(got, ref):
            assert torch.equal(v, r) and not torch.isnan(v).any()
            mask = torch.ones_like(buf, dtype=torch.bool)
            if buf.dim() == 1:
                mask[8:8 + D] = False
            else:
                mask[:B, :S, :v.shape[2], :D] = False
            assert bool((buf[mask] == 5.0).all()), "a neighbour of an output was written"


@pytest.mark.parametrize("lead,heads,D", [((2, 700), (3, 1), 128), ((1, 2100), (4, 1), 256)],
                         ids=["132-workgroups-ragged-last", "1024-partials-walk-of-2"])
def test_weight_gradient_over_many_workgroups(single_rank_group, lead, heads, D):
    """B 2, S 700, H 3, D 128: 4200 items of q in 132 workgroups of 32, the last one with 8 (k: 1400 items in 44, the last with
    24).  B 1, S 2100, H 4, D 256: 8400 items of 8 per workgroup are more than the 1024 partials hold in one step: a walk of two,
    the second one 26 workgroups long (k: 263 workgroups, the last with 4 items)."""
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    dtype = torch.bfloat16
    rows = lead[0] * lead[1]
    cos, sin = _tables(D, torch.float32, rows=lead[1])
    q, k = _qk(D, dtype, lead=lead, heads=heads)
    dqo, dko = _qk(D, dtype, seed=6, lead=lead, heads=heads)
    wq, wk = _w(D, torch.float32)
    kw = dict(eps=EPS, weight_offset=0.0)
    _, (dq, dk), (dwq, dwk) = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), **kw)
    pos = torch.arange(lead[1])
    for name, x, w, dout, dx, dw in (("q", q, wq, dqo, dq, dwq), ("k", k, wk, dko, dk, dwk)):
        items = rows * x.shape[2]
        r = reference(x, w, cos[:-1], sin[:-1], pos, eps=EPS, dout=dout)
        _check(f"d{name}", dx, r["dx"], r["Mb"], dtype, 2.0 ** -18)
        _check_dw(f"dw_{name} over {items} items", dw, r["dw"], r["T"], kernel_chain(items, D))
        alone = _direct(be, (x,), (w,), cos, sin, (dout,), **kw)
        assert torch.equal(alone[2][0], dw) and torch.equal(alone[1][0], dx)
    again = _direct(be, (q, k), (wq, wk), cos, sin, (dqo, dko), **kw)
    assert _same(again[2], (dwq, dwk)) and _same(again[1], (dq, dk))


@pytest.mark.extended
def test_batch_entry_past_4_gib(single_rank_group):
    """x and dout in one arena, y and dx in another (tests/_farview.py, kind `batch`): batch entry 1 of every tensor lies more
    than 2^32 bytes behind its base pointer.  The results are the bits of the compact call; the regions a 32-bit offset would
    hit hold NaN (inputs) or sentinels (outputs), and the sentinels and the bands around the far pieces stay intact."""
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    dtype, D, Sf, Hf = torch.bfloat16, 64, 5, 2
    spec = lambda name: FV.Spec(name, (2, Sf, Hf, D), "bshd", "q")
    vin, nin = FV.layout("batch", [spec("x"), spec("dout")], 2)
    vout, nout = FV.layout("batch", [spec("y"), spec("dx")], 2)
    ain, aout = FV.Arena(vin, nin, dtype, _dev(), False), FV.Arena(vout, nout, dtype, _dev(), True)
    ain.poison(), aout.poison()
    g = torch.Generator().manual_seed(2)
    x, dout = (torch.randn(2, Sf, Hf, D, generator=g).to(dtype).to(_dev()) for _ in range(2))
    ain.view("x").copy_(x), ain.view("dout").copy_(dout)
    assert FV.reach_bytes(vin["x"]) >= 2 ** 32 and FV.reach_bytes(vout["dx"]) >= 2 ** 32
    w = _w(D, torch.float32)[0]
    cos, sin = _tables(D, torch.float32)
    pos = _positions(lead=(2, Sf))
    kw = dict(eps=EPS, weight_offset=0.0, positions=pos)
    want = _direct(be, (x,), (w,), cos, sin, (dout,), **kw)
    dw = torch.empty(D, dtype=torch.float32, device=_dev())
    be.qk_norm_rotary_fwd([ain.view("x")], [aout.view("y")], [w], cos, sin, **kw)
    be.qk_norm_rotary_bwd([ain.view("x")], [ain.view("dout")], [aout.view("dx")], [w], [dw], cos, sin, **kw)
    assert torch.equal(aout.view("y"), want[0][0]) and torch.equal(aout.view("dx"), want[1][0]) and torch.equal(dw, want[2][0])
    aout.check()
    r = reference(x, w, _cut(cos), _cut(sin), pos.cpu(), eps=EPS, dout=dout)
    _check("far y", aout.view("y"), r["y"], r["Mf"], dtype, 2.0 ** -19)
    del ain, aout
    torch.cuda.empty_cache()


@pytest.mark.parametrize("W", [2, 4])
def test_norm_rotary_then_the_schedule_on_shared_gpu(W):
    """W processes sharing the GPU: apply_qk_norm_rotary(layout=func) on the shards, then func, forward and backward, for ring,
    zigzag and stripe.  Un-sharded: the shards' results are bit-equal to the shards of the single-device result; dq, dk and the
    sum of the ranks' partial weight gradients lie within the derived bounds of one fp64 computation; out / dq / dk / dv behind
    the schedule within the *_ring kinds of tests/_tol.py of exact attention, carried back through the norm in fp64."""
    cases = [dict(kind=kind, W=W, S=S, B=B, H=H, Hk=HK, D=64, R=64, attn=True) for kind in ("ring", "zigzag", "stripe")]
    res, errs = QW.run_world(W, cases, True, free_port())
    assert not errs, "\n".join(errs)
    bad = [b for c in cases for b in QW.check_case(c, res[QW.case_name(c)], reference, lambda items: kernel_chain(items, 64))]
    assert not bad, "\n".join(bad)
