"""tests/_blockref.py and tests/_ref_backend.py — the yardstick of the CPU schedule tests and of the GPU kernel tests — pinned
by checks that do not depend on their own formulas: the band mask against matrices written out by hand, the block forward
/ backward against the frozen fp32 oracle (oracle/flash_attn_ref.py) and against torch.autograd through the forward, and
the backend's delivery (accumulate mode, phases, dark rows, refusals).  CPU only."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _blockref as R                           # noqa: E402
import _tol                                     # noqa: E402
from _ref_backend import FEATURES, RefBackend   # noqa: E402
from oracle import flash_attn_ref as O          # noqa: E402
from oracle.oracle_backend import BWD_COMPUTE, BWD_REDUCE, HALF_BACK, HALF_FRONT   # noqa: E402

H, HK, D = 4, 2, 32
SCALE = D ** -0.5
NOWIN = (-1, -1)
SLOPES = torch.tensor([0.5, 0.25, 0.125, 0.0625])


def _m(*rows):
    return torch.tensor([[c == "1" for c in r] for r in rows])


# (lq, lk, causal, window, shift) -> the mask, row by row: off - wl <= j - i <= off + wr, off = lk - lq + shift
MASKS = [
    ((3, 5, True, NOWIN, 0), _m("11100", "11110", "11111")),                      # causal, bottom-right aligned
    ((5, 3, True, NOWIN, 0), _m("000", "000", "100", "110", "111")),
    ((3, 5, False, (1, 1), 0), _m("01110", "00111", "00011")),                    # a two-sided window
    ((5, 3, False, (1, 1), 0), _m("000", "100", "110", "111", "011")),
    ((3, 5, True, (1, 0), -1), _m("11000", "01100", "00110")),                    # ... with causal and a shift
    ((3, 5, True, NOWIN, 1), _m("11110", "11111", "11111")),                      # a positive shift
    ((5, 3, True, NOWIN, 2), _m("100", "110", "111", "111", "111")),
    ((3, 5, True, NOWIN, -3), _m("00000", "10000", "11000")),                     # a negative shift
    ((3, 5, True, NOWIN, -5), _m("00000", "00000", "00000")),                     # a dark block
    ((5, 3, False, (2, 1), 7), _m("000", "000", "000", "000", "000")),
    ((3, 5, False, (10, 10), 0), _m("11111", "11111", "11111")),                  # both bounds out of reach
    ((5, 3, False, (1 << 40, 7), -3), _m("111", "111", "111", "111", "111")),
    ((3, 5, False, NOWIN, 99), _m("11111", "11111", "11111")),                    # no band: the shift is ignored
]


@pytest.mark.parametrize("args,want", MASKS, ids=[str(a) for a, _ in MASKS])
def test_visible_against_masks_written_out_by_hand(args, want):
    assert torch.equal(R.visible(*args), want)


def _inputs(lq, lk, seed, B=None):
    g = torch.Generator().manual_seed(seed)
    lead = () if B is None else (B,)
    return tuple(torch.randn(*lead, n, h, D, generator=g).bfloat16() for n, h in ((lq, H), (lk, HK), (lk, HK), (lq, H)))


# ---------------------------------------------------------------------------------------- against the frozen fp32 oracle
@pytest.mark.parametrize("lq,lk", [(40, 56), (56, 40), (33, 0)])
@pytest.mark.parametrize("causal,window,drop", [(False, NOWIN, None), (True, NOWIN, None), (False, (9, 4), None), (True, (12, 0), None),
                                                (True, NOWIN, (0.2, 77, 300, 100, 2))],
                         ids=["plain", "causal", "window", "causal-window", "dropout"])
def test_block_against_the_fp32_oracle(lq, lk, causal, window, drop):
    """test_oracle.py's bounds for oracle versus fp64: out and lse < 2e-5 absolute, gradients < 5e-5 max(1, max|ref|)"""
    q, k, v, do = _inputs(lq, lk, 11)
    od = None
    kw = dict(causal=causal, window=window)
    if drop is not None:
        p, seed, q0, k0, h0 = drop
        od = dict(p=p, seed=seed, batch=1, head0=h0, q_pos0=q0, k_pos0=k0)
        kw.update(keep=R.keep_mask(drop, 1, H, lq, lk), rescale=O.drop_rescale(p))
    oo, ol = O._fwd_one(q, k, v, SCALE, causal, window, drop=od)
    ro, rl = R.block_forward(q, k, v, SCALE, **kw)
    dark = torch.isinf(rl)
    assert torch.equal(dark, torch.isinf(ol)) and (rl[dark] > 0).all() and (ol[dark] > 0).all()
    assert torch.equal(dark, ~R.visible(lq, lk, causal, window).any(1).expand(H, lq))
    assert (ro.permute(1, 0, 2)[dark] == 0).all()
    assert (oo.double() - ro).abs().max() < 2e-5
    if (~dark).any():
        assert (ol.double() - rl)[~dark].abs().max() < 2e-5
    delta = (do.float() * oo).sum(-1).transpose(0, 1)
    got = O._bwd_one(do, q, k, v, None, ol, SCALE, causal, delta=delta, window=window, drop=od)
    ref = R.block_backward(do, q, k, v, ol, delta, SCALE, **kw)
    for nm, g_, r_ in zip(("dq", "dk", "dv"), got, ref):
        assert g_.shape == r_.shape, nm
        if r_.numel():
            assert (g_.double() - r_).abs().max() < 5e-5 * max(1.0, r_.abs().max().item()), nm
    if lk == 0:
        assert all((r_ == 0).all() for r_ in ref)


# ------------------------------------------------------------------------------- against autograd through block_forward
def _mapped_keep(B, lq, lk):
    drop = (0.3, 4321, 1000, 50, 1, (1, lq // 2, 5000), (3, 0, 0))
    return [R.keep_mask(drop, b, H, lq, lk) for b in range(B)]


FEATURE_CASES = {
    "plain": dict(),
    "causal": dict(causal=True),
    "window": dict(window=(9, 4)),
    "shift": dict(causal=True, shift=5),
    "cap": dict(softcap=5.0),
    "bias": dict(slopes=SLOPES, alibi_shift=3),
    "bias-per-batch": dict(slopes=torch.stack([SLOPES, 1.5 * SLOPES]), causal=True),
    "keep": dict(keep="mapped", rescale=O.drop_rescale(0.3)),
    # what no reference file could express before
    "cap+window+shift": dict(softcap=5.0, causal=True, window=(12, 0), shift=4),
    "bias+shift": dict(slopes=SLOPES, alibi_shift=-7, causal=True, shift=6),
    "bias+window": dict(slopes=SLOPES, window=(9, 4)),
    "cap+bias": dict(softcap=50.0, slopes=SLOPES, alibi_shift=2),
    "keep+causal": dict(keep="mapped", rescale=O.drop_rescale(0.3), causal=True),
}


@pytest.mark.parametrize("lq,lk", [(40, 56), (56, 40)])
@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_block_backward_is_the_gradient_of_block_forward(name, lq, lk):
    """block-local lse and delta = rowsum(dout * out); both sides fp64, only reassociation separates them: <= 1e-12 max|ref|
    (about 2^12 ulp; sums of up to 10^3 terms).  lq > lk: the first rows of a causal block see no key."""
    kw = dict(FEATURE_CASES[name])
    if kw.get("keep") is not None:
        kw["keep"] = _mapped_keep(2, lq, lk)
    q, k, v, do = _inputs(lq, lk, 23, B=2)
    ref = R.attention(q, k, v, dout=do, autograd=True, **kw)
    got = R.attention(q, k, v, dout=do, **kw)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    for nm, g_, r_ in zip(("dq", "dk", "dv"), got[2:], ref[2:]):
        assert torch.isfinite(r_).all() and r_.abs().max() > 1e-3, nm
        assert (g_ - r_).abs().max() <= 1e-12 * r_.abs().max(), (nm, ((g_ - r_).abs().max() / r_.abs().max()).item())


def test_packed_input_with_an_empty_sequence():
    """three packed sequences, the middle one without a query row: per sequence the dense call on its rows, and the gradient
    of the forward"""
    cq, ck = [0, 13, 13, 40], [0, 21, 26, 56]
    q, k, v, do = _inputs(40, 56, 31)
    kw = dict(causal=True, window=(6, 0), shift_lens=0, softcap=5.0, slopes=torch.stack([SLOPES, 2 * SLOPES, 3 * SLOPES]))
    got = R.attention(q, k, v, dout=do, cu_seqlens_q=cq, cu_seqlens_k=ck, **kw)
    ref = R.attention(q, k, v, dout=do, autograd=True, cu_seqlens_q=cq, cu_seqlens_k=ck, **kw)
    assert got[0].shape == (40, H, D) and got[1].shape == (H, 40) and got[3].shape == (56, HK, D)
    for g_, r_ in zip(got[2:], ref[2:]):
        assert (g_ - r_).abs().max() <= 1e-12 * r_.abs().max()
    assert (got[3][21:26] == 0).all() and (got[4][21:26] == 0).all()               # keys of the sequence without queries
    for b in (0, 2):
        one = R.attention(q[None, cq[b]:cq[b + 1]], k[None, ck[b]:ck[b + 1]], v[None, ck[b]:ck[b + 1]], dout=do[None, cq[b]:cq[b + 1]],
                          **dict(kw, slopes=kw["slopes"][b]))
        assert torch.equal(one[0][0], got[0][cq[b]:cq[b + 1]]) and torch.equal(one[1][0], got[1][:, cq[b]:cq[b + 1]])
        assert torch.equal(one[3][0], got[3][ck[b]:ck[b + 1]])


# --------------------------------------------------------------------------------------------------- RefBackend delivery
B, LQ, LK, CUT = 2, 40, 56, 24          # the keys are delivered as blocks [0, CUT) and [CUT, LK)
_S = 5                                  # whole call: causal, off = LK - LQ + _S; block 1 needs off too: shift + LK - CUT


def _delivery(feature):
    """(serves, keywords of the whole call, of key block 1, of key block 2, rows of block 2 without a key or None)"""
    causal = dict(softmax_scale=SCALE, causal=True)
    dark2 = ~R.visible(LQ, LK - CUT, True, NOWIN, _S).any(1)
    if feature == "mask_shift":
        return (feature,), dict(causal, mask_shift=_S), dict(causal, mask_shift=_S + LK - CUT), dict(causal, mask_shift=_S), dark2
    if feature == "mask_shift_lens":                 # block 1: -1 * CUT = -LK + (LK - CUT); block 2: -(LK - CUT) - CUT = -LK
        win = dict(softmax_scale=SCALE, causal=False, window=(45, 60))
        dark = ~R.visible(LQ, LK - CUT, False, (45, 60), -LK).any(1)
        return (("mask_shift", feature), dict(win, mask_shift_lens=-1), dict(win, mask_shift_lens=-1),
                dict(win, mask_shift_lens=-1, mask_shift=-CUT), dark)
    if feature == "alibi":
        return (("mask_shift", feature), dict(causal, mask_shift=_S, alibi=(SLOPES, 3)),
                dict(causal, mask_shift=_S + LK - CUT, alibi=(SLOPES, 3 + LK - CUT)), dict(causal, mask_shift=_S, alibi=(SLOPES, 3)), dark2)
    if feature == "softcap":
        return (("mask_shift", feature), dict(causal, mask_shift=_S, softcap=5.0), dict(causal, mask_shift=_S + LK - CUT, softcap=5.0),
                dict(causal, mask_shift=_S, softcap=5.0), dark2)
    assert feature == "dropout_positions"            # (no shift with dropout: non-causal; the key map's split is the cut)
    plain = dict(softmax_scale=SCALE, causal=False)
    head, qm = (0.25, 99, 700, 20, 1), (2, LQ // 2 + 1, 3000)
    return ((feature,), dict(plain, dropout=(*head, qm, (3, CUT, 9000))), dict(plain, dropout=(*head, qm, (3, 0, 0))),
            dict(plain, dropout=(0.25, 99, 700, 9000, 1, qm, (3, 0, 0))), None)


@pytest.mark.parametrize("feature", FEATURES)
def test_ref_backend_delivery(feature):
    serves, whole, kw1, kw2, dark2 = _delivery(feature)
    be = RefBackend(serves=serves)
    assert {a for a in dir(be) if a.startswith("serves_")} == {"serves_" + f for f in serves}
    q, k, v, do = _inputs(LQ, LK, 41, B=B)
    k1, v1, k2, v2 = k[:, :CUT], v[:, :CUT], k[:, CUT:], v[:, CUT:]
    out, lse = torch.empty_like(q), torch.empty(B, H, LQ)
    be.fwd(q, k, v, out=out, lse=lse, **whole)
    assert torch.isfinite(lse).all()

    # accumulate mode over the two key blocks (acc_init, then merge) is the plain call over all keys
    oa, la = torch.full((B, LQ, H, D), float("nan")), torch.full((B, H, LQ), float("nan"))
    be.fwd(q, k1, v1, out_acc=oa, lse_acc=la, acc_init=True, **kw1)
    o1, l1 = oa.clone(), la.clone()
    be.fwd(q, k2, v2, out_acc=oa, lse_acc=la, **kw2)
    _tol.compare(f"{feature} out", oa, out.double(), "out_ring")
    _tol.compare(f"{feature} lse", la, lse.double(), "lse_ring")
    if dark2 is not None:                            # rows without a key in block 2: untouched, to the bit
        assert dark2.any() and not dark2.all()
        assert torch.equal(oa[:, dark2], o1[:, dark2]) and torch.equal(la[:, :, dark2], l1[:, :, dark2])
        assert not torch.equal(oa[:, ~dark2], o1[:, ~dark2])

    # two phases with the returned partials are the one-phase call, to the bit; RFA_BWD_KV_OVERWRITE overwrites
    delta = torch.empty(B, H, LQ)
    be.bwd_preprocess(do, out, delta)
    args = (do, q, k2, v2, lse, delta)

    def accs(**kw):
        acc = [torch.full(t.shape, 1.5) for t in (q, k2, v2)]
        return acc, dict(kw2, dq_acc=acc[0], dk_acc=acc[1], dv_acc=acc[2], **kw)

    one, kw = accs()
    assert be.bwd(*args, **kw) is None
    two, kw = accs()
    token = be.bwd(*args, phases=BWD_COMPUTE, **kw)
    assert torch.equal(two[0], one[0]) and (two[1] == 1.5).all() and (two[2] == 1.5).all()
    assert be.bwd(*args, phases=BWD_REDUCE, partials=token, **kw) is None
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    init, kw = accs(acc_init=True)
    be.bwd(*args, **kw)
    over, kw = accs()
    token = be.bwd(*args, phases=BWD_COMPUTE, **kw)
    be.bwd(*args, phases=BWD_REDUCE | 16, partials=token, **kw)
    assert torch.equal(over[0], one[0]) and torch.equal(over[1], init[1]) and torch.equal(over[2], init[2])
    assert (init[1] != 0).any() and not torch.equal(one[1], init[1])
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k2), torch.empty_like(v2)
    be.bwd(*args, dq=dq, dk=dk, dv=dv, **kw2)
    assert all(torch.equal(a.float(), b) for a, b in zip((dq, dk, dv), init))

    # a backend that serves everything but this feature: TypeError, as for an unknown keyword
    other = RefBackend(serves=tuple(f for f in FEATURES if f != feature))
    with pytest.raises(TypeError):
        other.fwd(q, k, v, out=out, lse=lse, **whole)
    with pytest.raises(TypeError):
        other.bwd(do, q, k, v, lse, delta, dq=dq, dk=torch.empty_like(k), dv=torch.empty_like(v), **whole)
    with pytest.raises(TypeError):
        be.fwd(q, k, v, out=out, lse=lse, no_such_keyword=1, **whole)


def test_ref_backend_without_an_extension_is_the_oracle():
    from oracle.oracle_backend import OracleBackend

    q, k, v, _ = _inputs(LQ, LK, 43, B=B)
    res = []
    for be, kw in ((OracleBackend(), dict()), (RefBackend(serves=FEATURES), dict(mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0))):
        out, lse = torch.empty_like(q), torch.empty(B, H, LQ)
        be.fwd(q, k, v, softmax_scale=SCALE, causal=True, window=(7, 0), dropout=(0.1, 5, 0, 0, 0), out=out, lse=lse, **kw)
        res.append((out, lse))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_ref_backend_packed_halves_of_odd_length():
    """packed input, the BACK half of every q sequence against the FRONT half of its keys, odd lengths: per sequence the
    reference on those rows, with shift = mask_shift_lens * (the half's key length); rows outside the halves untouched"""
    be = RefBackend(serves=("mask_shift", "mask_shift_lens", "softcap"))
    lens, cu = [7, 0, 9], torch.tensor([0, 7, 7, 16], dtype=torch.int32)
    q, k, v, _ = _inputs(16, 16, 47)
    out, lse = torch.full_like(q, 7.0), torch.full((H, 16), 7.0)
    be.fwd(q, k, v, softmax_scale=SCALE, causal=True, window=(2, 0), cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=9, max_seqlen_k=9,
           q_half=HALF_BACK, k_half=HALF_FRONT, out=out, lse=lse, mask_shift_lens=1, softcap=5.0)
    s = 0
    for L in lens:
        h = L // 2                                                       # FRONT: L // 2 rows, BACK: the other L - L // 2
        if L:
            ro, rl = R.attention(q[None, s + h:s + L], k[None, s:s + h], v[None, s:s + h], scale=SCALE, causal=True, window=(2, 0),
                                 shift_lens=1, softcap=5.0)
            _tol.compare("out", out[s + h:s + L], ro[0], "out_ring")
            assert torch.equal(torch.isinf(lse[:, s + h:s + L]), torch.isinf(rl[0])) and torch.isinf(rl[0]).any() and not torch.isinf(rl[0]).all()
            fin = ~torch.isinf(rl[0])
            assert (lse[:, s + h:s + L][fin].double() - rl[0][fin]).abs().max() < 1e-5
            assert (out[s:s + h] == 7.0).all() and (lse[:, s:s + h] == 7.0).all()
        s += L
