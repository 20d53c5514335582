"""Attention sinks on the MI355X (csrc/rfa_sink.hip; ring_flash_attn.with_sinks).

1. The two kernels alone, through backend.sink_apply / sink_grad on random (out, lse, dO), against the fp64 formulas of
   tests/_sinkref.py: head dims 40 .. 256 (two passes of the 16 lanes above 128), row x head counts that are no multiple of
   16, two row chunks, bf16 and fp16, dense and packed, a strided dO, rows with lse = +inf, out_dst aliasing out_src or not;
   dsink bit-identical over two runs and within DSINK_TOL (4 x the error of a plain fp32 evaluation, measured on the CPU) of
   the fp64 formula on the same stored inputs.
2. `with_sinks` on one device against the INDEPENDENT fp64 reference (the sink column appended to the scores), kinds out, lse,
   grad of tests/_tol.py, dsink on kind grad.
3. W = 2 with the ranks sharing the GPU: five schedule families, kinds *_ring, dsink summed over the ranks."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _sinkref as SK                            # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
def _kernel_params():
    """core: every head dim at the middle shape and every shape at D = 64 and 136, bf16 dense / fp16 packed alternating;
    extended: the rest of the product"""
    out = []
    for D in SK.KERNEL_D:
        for bsh in SK.KERNEL_BSH:
            for dt in (BF, FP16):
                for packed in (False, True):
                    core = (dt is BF) != packed and (bsh == SK.KERNEL_BSH[1] or D in (64, 136))
                    out.append(pytest.param(D, bsh, dt, packed, marks=() if core else _EXT,
                                            id=f"D{D}-{'x'.join(map(str, bsh))}-{'bf16' if dt is BF else 'fp16'}-"
                                               f"{'packed' if packed else 'dense'}"))
    return out


@pytest.mark.parametrize("D,bsh,dt,packed", _kernel_params())
def test_sink_kernels_against_the_fp64_formulas(D, bsh, dt, packed):
    be, dev = _be(), _dev()
    do, o, l, s = SK.kernel_inputs(*bsh, D, dt, packed)
    ref_o, ref_l = SK.apply_formula(o, l, s)
    dod, od, ld, sd = (t.to(dev) for t in (do.contiguous(), o, l, s))
    wide = torch.zeros(*do.shape[:-1], D + 8, dtype=dt, device=dev)
    wide[..., :D] = dod
    dod = wide[..., :D]                                              # a strided dO: a slice of a wider tensor
    assert not dod.is_contiguous() or do.numel() == D
    o2, l2 = be.sink_apply(od, ld, sd, varlen=packed)
    assert o2.data_ptr() != od.data_ptr() and torch.equal(od.cpu(), o)            # not aliasing: the source is untouched
    oa, la = od.clone(), ld.clone()
    o3, l3 = be.sink_apply(oa, la, sd, varlen=packed, inplace=True)                # out_dst aliasing out_src
    assert o3.data_ptr() == oa.data_ptr() and l3.data_ptr() == la.data_ptr()
    assert torch.equal(o3, o2) and torch.equal(l3, l2)
    m = _tol.metrics(l2, ref_l)
    print(f"lse': max_err {m['max_err']:.3e}; ", end="")
    _tol.compare("sink_apply.lse", l2, ref_l, "lse")
    _tol.compare("sink_apply.out", o2, ref_o, "out")
    # rows without a visible key: lse' = the sink, out' = 0
    inf = torch.isinf(l.transpose(-1, -2))
    assert inf.any() or bsh[1] == 0
    assert torch.equal(l2.cpu().transpose(-1, -2)[inf], s.expand_as(inf)[inf])
    assert not o2.cpu()[inf].any()
    # dsink from the STORED out', lse': the same bits twice, and the fp64 formula on the same inputs within DSINK_TOL
    d1 = be.sink_grad(dod, o2, l2, sd, varlen=packed)
    d2 = be.sink_grad(dod, o2, l2, sd, varlen=packed)
    torch.cuda.synchronize()
    assert d1.dtype == torch.float32 and d1.shape == s.shape and torch.equal(d1, d2)
    ref_d, norm = SK.dsink_formula(do, o2.cpu(), l2.cpu(), s)
    err = ((d1.cpu().double() - ref_d).abs() / norm.clamp_min(1e-300)).max().item()
    print(f"dsink: error / sum|terms| {err:.3e} (bound {SK.DSINK_TOL:.3e})")
    assert err <= SK.DSINK_TOL, (err, SK.DSINK_TOL)


def test_a_low_sink_returns_the_input_bits_and_no_rows_give_zeros():
    be, dev = _be(), _dev()
    do, o, l, s = (t.to(dev) for t in SK.kernel_inputs(2, 17, 3, 64, BF, False))
    fin = torch.where(torch.isinf(l), torch.zeros_like(l), l)       # (rows without a key are covered above)
    low = torch.full_like(s, -1e4)
    o2, l2 = be.sink_apply(o, fin, low, varlen=False)
    assert torch.equal(o2, o) and torch.equal(l2, fin)
    assert torch.equal(be.sink_grad(do.contiguous(), o2, l2, low, varlen=False), torch.zeros_like(s))
    empty = be.sink_grad(do[:, :0], o[:, :0], l[:, :, :0], s, varlen=False)
    eo, el = be.sink_apply(o[:, :0], l[:, :, :0], s, varlen=False)
    torch.cuda.synchronize()
    assert torch.equal(empty, torch.zeros_like(s)) and eo.numel() == 0 and el.numel() == 0


# ---------------------------------------------------------------------------------------------- 2. one device, end to end
H, HK = 8, 2
KINDS6 = ("out", "lse", "grad", "grad", "grad", "grad")
NAMES6 = ("out", "lse", "dq", "dk", "dv", "dsink")


class _Case:
    """one seeded input set, its sinks (around the mean lse of the attention without them, +- 2) and its fp64 reference —
    computed once, shared by the tests that need it, never changed"""

    def __init__(self, sq, sk, D, window=(-1, -1), cu=None, keep=None, rescale=1.0, dt=BF):
        gen = torch.Generator().manual_seed(5100 + sq + 3 * sk + 7 * D)
        lead_q, lead_k = ((sq,), (sk,)) if cu is not None else ((2, sq), (2, sk))
        mk = lambda *s: torch.randn(*s, generator=gen).to(dt)
        self.q, self.k, self.v, self.do = mk(*lead_q, H, D), mk(*lead_k, HK, D), mk(*lead_k, HK, D), mk(*lead_q, H, D)
        self.kw = dict(causal=True, window=window, keep=keep, rescale=rescale)
        if cu is not None:
            self.kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu)
        self.plain = SK.attention(self.q, self.k, self.v, None, dout=self.do, **self.kw)
        lse = self.plain[1]
        self.sinks = (lse[torch.isfinite(lse)].mean() + 4 * torch.rand(H, generator=gen, dtype=torch.float64) - 2).float()
        self.ref = SK.attention(self.q, self.k, self.v, self.sinks, dout=self.do, **self.kw)

    def dev(self):
        d = _dev()
        return tuple(t.to(d) for t in (self.q, self.k, self.v, self.do)) + (self.sinks.to(d).requires_grad_(True),)


_CASES = {}


def _case(*key, **kw):
    full = key + tuple(sorted((k, str(v)) for k, v in kw.items() if k != "keep"))
    if full not in _CASES:
        while len(_CASES) >= 6:
            _CASES.pop(next(iter(_CASES)))
        _CASES[full] = _Case(*key, **kw)
    return _CASES[full]


def _check(got, ref, tag=""):
    bad = []
    for name, g_, r_, kind in zip(NAMES6, got, ref, KINDS6):
        m = _tol.metrics(g_, r_)
        print(f"{tag}{name}: max_err {m['max_err']:.3e} max_ref {m['max_ref']:.3e} fro {m['fro']:.3e} mean_err {m['mean_err']:.3e}")
        bad += _tol.failures(tag + name, g_, r_, kind)
    assert not bad, "; ".join(bad)


def _discriminates(c):
    """on the reference alone: out and dq with the sinks differ from those without by at least 10 x the rtol of their kind"""
    for i, kind in ((0, "out"), (2, "grad")):
        gap = ((c.ref[i] - c.plain[i]).abs().max() / c.ref[i].abs().max()).item()
        assert gap >= 10 * _tol.KINDS[kind][1], (i, gap)


@pytest.mark.parametrize("sq,sk,D,window", [(100, 100, 64, (-1, -1)), (100, 100, 128, (-1, -1)), (70, 50, 64, (-1, -1)),
                                            (100, 100, 64, (16, 0)), pytest.param(70, 50, 128, (-1, -1), marks=_EXT),
                                            pytest.param(100, 100, 128, (16, 0), marks=_EXT)])
def test_with_sinks_on_one_device(single_rank_group, sq, sk, D, window):
    """H 8 / Hk 2, causal.  Sq 70 against Sk 50: the first 20 rows see no key — out' = 0, lse' = the sink, nothing for dsink
    (the reference has all three by construction)"""
    import ring_flash_attn as R

    _be()
    c = _case(sq, sk, D, window=window)
    _discriminates(c)
    q, k, v, do, sinks = c.dev()
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    out, lse, _ = R.with_sinks(R.ring_flash_attn_func, sinks)(q, k, v, causal=True, window_size=window, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, q.grad, k.grad, v.grad, sinks.grad), c.ref)
    if sq > sk:
        assert not out[:, :sq - sk].any() and torch.equal(lse[:, :, :sq - sk], sinks.detach().view(1, H, 1).expand(2, H, sq - sk))


def test_with_sinks_on_packed_input_with_an_empty_sequence(single_rank_group):
    import ring_flash_attn as R

    _be()
    cu = [0, 5, 5, 100]
    c = _case(100, 100, 64, cu=cu)
    _discriminates(c)
    q, k, v, do, sinks = c.dev()
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    cud = torch.tensor(cu, dtype=torch.int32, device=_dev())
    out, lse, _ = R.with_sinks(R.ring_flash_attn_varlen_func, sinks)(q, k, v, cud, 95, causal=True, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, q.grad, k.grad, v.grad, sinks.grad), c.ref, "varlen.")
    # llama3 on the same packed batch (one rank: the whole key range)
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s2 = sinks.detach().clone().requires_grad_(True)
    out, lse, _ = R.with_sinks(R.llama3_flash_attn_varlen_func, s2)(q2, k2, v2, cud, cud, 95, 95, heads_k_stride=1,
                                                                    local_k_slice=slice(0, 100), causal=True, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, q2.grad, k2.grad, v2.grad, s2.grad), c.ref, "llama3.")


def test_with_sinks_kvpacked_and_qkvpacked(single_rank_group):
    import ring_flash_attn as R

    _be()
    c = _case(100, 100, 64)
    q, k, v, do, sinks = c.dev()
    qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)
    out, lse, _ = R.with_sinks(R.ring_flash_attn_kvpacked_func, sinks)(qq, kv, causal=True, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, qq.grad, kv.grad[:, :, 0], kv.grad[:, :, 1], sinks.grad), c.ref, "kvpacked.")
    G = H // HK
    qkv = torch.stack([c.q, c.k.repeat_interleave(G, dim=2), c.v.repeat_interleave(G, dim=2)], dim=2)
    ref = SK.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], c.sinks, dout=c.do, causal=True)
    qkv = qkv.to(_dev()).requires_grad_(True)
    s2 = sinks.detach().clone().requires_grad_(True)
    out, lse, _ = R.with_sinks(R.zigzag_ring_flash_attn_qkvpacked_func, s2)(qkv, causal=True, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, qkv.grad[:, :, 0], qkv.grad[:, :, 1], qkv.grad[:, :, 2], s2.grad), ref, "qkvpacked.")


def test_with_sinks_and_dropout(single_rank_group):
    """dropout 0.1: the keep mask multiplies P', delta' absorbs it — against the reference with the mask of tests/_blockref.py"""
    import ring_flash_attn as R
    from _blockref import keep_mask
    from oracle.flash_attn_ref import drop_rescale

    _be()
    p, S = 0.1, 100
    gen = torch.Generator().manual_seed(9)
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=gen))
    keep = [keep_mask((p, seed, 0, 0, 0), b, H, S, S) for b in range(2)]
    c = _case(S, S, 64, keep=keep, rescale=drop_rescale(p))
    _discriminates(c)
    q, k, v, do, sinks = c.dev()
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    gen.manual_seed(9)                                               # the forward draws the same seed
    R.set_dropout_generator(gen)
    try:
        out, lse, _ = R.with_sinks(R.ring_flash_attn_func, sinks)(q, k, v, dropout_p=p, causal=True, return_attn_probs=True)
    finally:
        R.set_dropout_generator(None)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, q.grad, k.grad, v.grad, sinks.grad), c.ref, "dropout.")


@pytest.mark.parametrize("window", [(-1, -1), (16, 0)])
def test_a_sink_of_minus_1e4_is_the_plain_call_bit_for_bit(single_rank_group, window):
    import ring_flash_attn as R

    _be()
    c = _case(100, 100, 64, window=window)
    got = []
    for sinks in (torch.full((H,), -1e4, device=_dev(), requires_grad=True), None):
        q, k, v, do, _ = c.dev()
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        out, lse, _ = R.with_sinks(R.ring_flash_attn_func, sinks)(q, k, v, causal=True, window_size=window, return_attn_probs=True)
        out.backward(do)
        torch.cuda.synchronize()
        got.append((out, lse, q.grad, k.grad, v.grad))
        if sinks is not None:
            assert torch.equal(sinks.grad, torch.zeros_like(sinks))
    for name, a_, b_ in zip(NAMES6, *got):
        assert torch.equal(a_, b_), name


# ---------------------------------------------------------------------------------------------- 3. W = 2 on one GPU
MULTI = [
    dict(kind="ring", W=2, S=128, D=64, causal=True),
    dict(kind="zigzag", W=2, S=128, D=64, causal=True, form="ring"),
    dict(kind="stripe", W=2, S=128, D=64, causal=True, window=(100, 0)),
    dict(kind="ring_varlen", W=2, S=128, D=64, causal=True, lens=[96, 160]),
    dict(kind="llama3", W=2, S=128, D=64, causal=True),
]


def test_five_schedules_over_two_ranks_sharing_the_gpu():
    """W = 2, the ranks share cuda:0 (host staging), S = 128 rows per rank, D = 64: the dense ring, zigzag, stripe with a
    window, ring varlen and llama3 — each against ONE single-device fp64 call, dsink summed over the ranks"""
    import _sinks_worker as KW

    errs, notes = KW.run_world(2, MULTI, True, free_port(), limit_s=240)
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
