"""The rotary kernel on the device (`-m gpu`): csrc/rfa_rotary.hip through ring_flash_attn.apply_rotary and HipBackend.rotary.

Shapes: B 2, S 38 (a zigzag chunk of 19 rows: a multiple of nothing), H 3 / Hk 1, the (D, R, rot_offset, pairing) rows of COMBOS,
bf16 and fp16, fp32 and io-dtype tables, one packed case of T = 77.  Against the textbook formula in fp64
(tests/_rotary_backend.py: reference), elementwise, with the DERIVED tolerance
    |err| <= u |ref| + 2^-22 (|x1 c| + |x2 s|),    u = 2^-8 (bf16), 2^-11 (fp16)
— the one rounding to the io dtype, and the fp32 products' error (each of the two products and their sum is within 2^-24 of
its operands' magnitudes).  Where a result falls below the io dtype's smallest normal number the rounding is absolute, not
relative — half a subnormal step: 2^-25 for fp16 (2^-134 for bf16) — so the first term is max(u |ref|, that half step); a D = 256
fp16 case has a few such elements (|ref| < 2^-14), which u |ref| alone misses by up to 2.9e-9 with any correct rounding.
Bit identities: map mode == explicit positions, in place == out of place, q and k together == one at a time, a strided view of a qkv tensor == its contiguous copy, pass-through columns == the input, two runs.  Round trip
through the conjugate within twice the tolerance plus u (|o1 c| + |o2 s|) — the first step's rounding of the pair (o1, o2),
carried back by the inverse: twice the tolerance with the element's own |ref| alone holds for no implementation (x1 = 0 returns
as u |x2 sin 2a|; measured up to 7.2e-3 over it for bf16, 8e-8 under the bound asserted here); backward against fp64 autograd; poisoned neighbours; a row past 4 GiB; and
W = 2 / 4 processes sharing the GPU: rotary on the shards, then the ring / zigzag / stripe schedule, forward and backward."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _rotary_worker as RW                      # noqa: E402
from _rotary_backend import reference            # noqa: E402

pytestmark = pytest.mark.gpu

B, S, H, HK, P = 2, 38, 3, 1, 80
#         D    R   rot_offset  interleaved
COMBOS = [(64, 64, 0, False), (128, 64, 0, False), (192, 64, 128, False), (256, 256, 0, False), (40, 16, 8, False),
          (40, 8, 8, True)]
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # half the spacing of the subnormal numbers


def _dev():
    return torch.device("cuda:0")


def _tables(Rw, dtype, rows=P):
    """cos / sin of `rows` positions plus ONE more row that no position uses, filled with NaN"""
    ang = torch.arange(rows, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(Rw // 2, dtype=torch.float64) / (Rw // 2)))
    pad = torch.full((1, Rw // 2), float("nan"), dtype=torch.float64)
    return torch.cat([ang.cos(), pad]).to(dtype).to(_dev()), torch.cat([ang.sin(), pad]).to(dtype).to(_dev())


def _qk(D, dtype, seed=5, lead=(B, S)):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*lead, H, D, generator=g).to(dtype).to(_dev()), torch.randn(*lead, HK, D, generator=g).to(dtype).to(_dev()))


def _positions(seed=3, lead=(B, S)):
    """every position below P at least possible, the NaN row (index P) never"""
    return torch.randint(0, P, lead, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(_dev())


def _check(what, got, ref, mag, dtype, factor=1.0):
    err = (got.detach().double().cpu() - ref).abs()
    lim = factor * ((U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + 2.0 ** -22 * mag)
    worst = (err - lim).max().item()
    print(f"{what}: max|err| {err.max().item():.3e}, worst err - bound {worst:.3e}")
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    assert worst <= 0, f"{what}: |err| exceeds u |ref| + 2^-22 (|x1 c| + |x2 s|) by {worst:.3e}"


@pytest.mark.parametrize("tables", ["fp32", "io"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,Rw,ro,inter", COMBOS)
def test_forward_backward_and_bit_identities(single_rank_group, D, Rw, ro, inter, dtype, tables):
    import ring_flash_attn as R
    from ring_flash_attn._common import zigzag_map
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    assert be.name == "hip" and be.serves_rotary
    cos, sin = _tables(Rw, torch.float32 if tables == "fp32" else dtype)
    q, k = _qk(D, dtype)
    pos = _positions()
    kw = dict(interleaved=inter, rot_offset=ro)
    qa, ka = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    qo, ko = R.apply_rotary(qa, ka, cos, sin, positions=pos, **kw)
    dqo, dko = _qk(D, dtype, seed=6)
    torch.autograd.backward([qo, ko], [dqo, dko])
    for name, x, out, dout, grad in (("q", q, qo, dqo, qa.grad), ("k", k, ko, dko, ka.grad)):
        ref, mag = reference(x, cos[:P], sin[:P], pos.cpu(), inter, ro)
        _check(f"{name} forward", out, ref, mag, dtype)
        gref, gmag = reference(dout, cos[:P], sin[:P], pos.cpu(), inter, ro, conj=True)     # = fp64 autograd (tests/test_rotary_cpu.py)
        _check(f"d{name}", grad, gref, gmag, dtype)
        # out of place, the pass-through columns are the input's bits
        assert torch.equal(out[..., :ro], x[..., :ro]) and torch.equal(out[..., ro + Rw:], x[..., ro + Rw:])
        # round trip: the conjugate returns the input within twice the tolerance
        back = torch.empty_like(out)
        be.rotary([out.detach()], [back], cos, sin, positions=pos, conj=True, **kw)
        xr, xmag = reference(out.detach(), cos[:P], sin[:P], pos.cpu(), inter, ro, conj=True)
        err = (back.double().cpu() - x.double().cpu()).abs()
        # twice the tolerance of the step (u |x| + 2^-22 (|o1 c| + |o2 s|)), plus what NO implementation can avoid: `out` is
        # already rounded, each o by up to u |o|, and the inverse rotation carries that into the element as up to
        # u (|o1 c| + |o2 s|) however small the element itself is (x1 = 0 comes back as u |x2 sin 2a|); 1 % covers the
        # second-order terms
        tol2 = 2 * ((U_OF[dtype] * x.double().cpu().abs()).clamp(min=HALF_STEP[dtype]) + 2.0 ** -22 * xmag)
        lim = tol2 + 1.01 * U_OF[dtype] * xmag
        print(f"{name} round trip: max|err| {err.max().item():.3e}; over twice the step's tolerance alone by "
              f"{(err - tol2).max().item():.3e}; over the bound by {(err - lim).max().item():.3e}")
        assert bool((err <= lim).all()), f"{name} round trip: {(err - lim).max().item():.3e} over"
    qo, ko = qo.detach(), ko.detach()
    # two runs give the same bits; q and k together == one at a time
    q2, k2 = R.apply_rotary(q, k, cos, sin, positions=pos, **kw)
    assert torch.equal(q2, qo) and torch.equal(k2, ko)
    assert torch.equal(R.apply_rotary(q, None, cos, sin, positions=pos, **kw), qo)
    assert torch.equal(R.apply_rotary(k, None, cos, sin, positions=pos, **kw), ko)
    # in place == out of place (and the pass-through columns are not touched: they hold the input's bits either way)
    q3, k3 = q.clone(), k.clone()
    r3 = R.apply_rotary(q3, k3, cos, sin, positions=pos, inplace=True, **kw)
    assert r3[0] is q3 and torch.equal(q3, qo) and torch.equal(k3, ko)
    # a strided view of a qkv tensor == its contiguous copy (MHA: three heads each)
    qkv = torch.randn(B, S, 3, H, D, generator=torch.Generator().manual_seed(9)).to(dtype).to(_dev())
    a, b = R.apply_rotary(qkv[:, :, 0], qkv[:, :, 1], cos, sin, positions=pos, **kw)
    c, d = R.apply_rotary(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), cos, sin, positions=pos, **kw)
    assert torch.equal(a, c) and torch.equal(b, d)
    # map mode == explicit positions of the same values: rank 1 of a 2-rank zigzag (chunks 1 and 2 of 19 rows), an offset
    pm = zigzag_map(1, 2, S // 2)
    m_q, m_k = torch.empty_like(q), torch.empty_like(k)
    be.rotary([q, k], [m_q, m_k], cos, sin, pos_map=pm, **kw)
    zz = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=1, world_size=2, device=_dev())
    assert zz.tolist() == list(range(19, 57))
    e_q, e_k = R.apply_rotary(q, k, cos, sin, positions=zz, **kw)
    assert torch.equal(m_q, e_q) and torch.equal(m_k, e_k)
    assert torch.equal(R.apply_rotary(q, None, cos, sin, offset=5, **kw),
                       R.apply_rotary(q, None, cos, sin, positions=torch.arange(S, dtype=torch.int32, device=_dev()), offset=5, **kw))
    # all nine dense layouts on a one-rank group are positions 0 .. S-1
    plain = R.apply_rotary(q, None, cos, sin, **kw)
    for f in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        assert torch.equal(R.apply_rotary(q, None, cos, sin, layout=f, **kw), plain)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_packed_input(single_rank_group, dtype):
    import ring_flash_attn as R

    T, D, Rw = 77, 128, 64
    cos, sin = _tables(Rw, torch.float32)
    q, k = _qk(D, dtype, lead=(T,))
    pos = _positions(lead=(T,))
    qa = q.clone().requires_grad_(True)
    qo, ko = R.apply_rotary(qa, k, cos, sin, positions=pos)
    dqo, _ = _qk(D, dtype, seed=6, lead=(T,))
    qo.backward(dqo)
    for name, x, out in (("q", q, qo), ("k", k, ko)):
        ref, mag = reference(x, cos[:P], sin[:P], pos.cpu())
        _check(f"packed {name}", out, ref, mag, dtype)
    gref, gmag = reference(dqo, cos[:P], sin[:P], pos.cpu(), conj=True)
    _check("packed dq", qa.grad, gref, gmag, dtype)
    # (T, H, D) is the (1, T, H, D) call
    q4, k4 = R.apply_rotary(q.unsqueeze(0), k.unsqueeze(0), cos, sin, positions=pos.view(1, T))
    assert torch.equal(q4[0], qo.detach()) and torch.equal(k4[0], ko)


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("D,Rw,ro,inter", [(128, 64, 0, False), (192, 64, 128, False), (40, 8, 8, True)])
def test_poisoned_neighbours_stay_untouched(single_rank_group, D, Rw, ro, inter, inplace):
    """q and k are views inside a larger NaN-filled buffer: padding behind every head's D columns, heads beyond H, rows beyond
    S and a further batch entry are bit-unchanged afterwards; the cos / sin tables end in a NaN row no position uses, and no NaN
    appears in the output; explicit positions -1 and P give the rows 0 and P-1 of the tables"""
    import ring_flash_attn as R

    dtype = torch.bfloat16
    cos, sin = _tables(Rw, torch.float32)
    cos, sin = cos[:P + 1], sin[:P + 1]                       # P used rows + the NaN row: the kernel's P is P + 1
    q, k = _qk(D, dtype)
    pos = _positions()
    kw = dict(interleaved=inter, rot_offset=ro)
    want_q, want_k = R.apply_rotary(q, k, cos, sin, positions=pos, **kw)
    bufs, views = [], []
    for x in (q, k):
        h = x.shape[2]
        buf = torch.full((B + 1, S + 3, h + 2, D + 8), float("nan"), dtype=dtype, device=_dev())
        v = buf[:B, :S, :h, :D]
        v.copy_(x)
        bufs.append(buf)
        views.append(v)
    before = [b.clone() for b in bufs]
    outs = R.apply_rotary(views[0], views[1], cos, sin, positions=pos, inplace=inplace, **kw)
    assert torch.equal(outs[0], want_q) and torch.equal(outs[1], want_k) and not torch.isnan(outs[0]).any()
    for buf, was, v, want in zip(bufs, before, views, (want_q, want_k)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:B, :S, :v.shape[2], :D] = False
        same = buf.view(torch.int16)[mask] == was.view(torch.int16)[mask]
        assert bool(same.all()), "a neighbour of the view was written"
        assert torch.equal(v, want if inplace else was[:B, :S, :v.shape[2], :D])
    # the clamp: positions -1 and P + 1 (one past the last table row) read rows 0 and P of the tables
    lo = torch.full((B, S), -1, dtype=torch.int32, device=_dev())
    hi_tab = (cos[:P].contiguous(), sin[:P].contiguous())
    hi = torch.full((B, S), P, dtype=torch.int32, device=_dev())
    assert torch.equal(R.apply_rotary(q, None, *hi_tab, positions=lo, **kw), R.apply_rotary(q, None, *hi_tab, positions=lo * 0, **kw))
    assert torch.equal(R.apply_rotary(q, None, *hi_tab, positions=hi, **kw), R.apply_rotary(q, None, *hi_tab, positions=hi - 1, **kw))


@pytest.mark.extended
def test_second_row_past_4_gib_in_place(single_rank_group):
    """a (1, 2, 1, 64) view whose second row lies past 4 GiB of one allocation, rotated in place: both rows correct, the
    element in front of the second row untouched"""
    import ring_flash_attn as R

    dtype, D = torch.bfloat16, 64
    row = 2 ** 31 + 4096                                      # elements: 4 GiB + 8 KiB
    buf = torch.empty(row + 4096, dtype=dtype, device=_dev())
    v = torch.as_strided(buf, (1, 2, 1, D), (0, row, D, 1), 0)
    x = torch.randn(1, 2, 1, D, generator=torch.Generator().manual_seed(2)).to(dtype)
    v.copy_(x.to(_dev()))
    buf[row - 8:row] = 5.0
    buf[D:D + 8] = 5.0                                        # (where a second row truncated to 32 bits of bytes would NOT land, but behind row 0)
    cos, sin = _tables(D, torch.float32)
    pos = torch.tensor([7, 33], dtype=torch.int32, device=_dev())
    out = R.apply_rotary(v, None, cos, sin, positions=pos, inplace=True)
    assert out is v
    ref, mag = reference(x, cos[:P], sin[:P], pos.cpu())
    _check("far rows", v, ref, mag, dtype)
    assert bool((buf[row - 8:row] == 5.0).all()) and bool((buf[D:D + 8] == 5.0).all())
    del buf, v, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("W", [2, 4])
def test_rotary_then_the_schedule_on_shared_gpu(W):
    """W processes sharing the GPU: apply_rotary(layout=func) on the shards, then func, forward and backward, for ring, zigzag
    and stripe.  Un-sharded: the rotated shards are bit-equal to the shards of the rotated full tensor, and out / dq / dk / dv
    lie within the *_ring kinds of tests/_tol.py of exact attention over the rotated full tensors, the gradients carried back by
    the conjugate rotation in fp64."""
    cases = [dict(kind=kind, W=W, S=S, B=B, H=H, Hk=HK, D=64, R=64, attn=True) for kind in ("ring", "zigzag", "stripe")]
    res, errs = RW.run_world(W, cases, True, free_port())
    assert not errs, "\n".join(errs)
    bad = [b for c in cases for b in RW.check_case(c, res[RW.case_name(c)], reference)]
    assert not bad, "\n".join(bad)
