"""ALiBi (alibi_slopes; include/rfa.h: rfa_ext_args) in the kernels against fp64 (tests/_blockref.py) through tests/_tol.py
(kinds out, lse, grad): the kBias instances of the forward, dQ and dK/dV kernels for head dims 128 and 64 (full) and 72 and
40 (the zero-padded 128- / 64-wide layouts), bf16 and fp16, square / few-rows / few-keys blocks that are no multiple of a
tile, causal and not, with the block's own distance (alibi_shift 0), a whole block in front (+Sk) or behind (-Sk) and a
shift that puts the kink of |i - j| inside a tile (37); (H,) and (B, H) slopes; a packed batch with unequal q / k lengths;
accumulate mode (two half-key blocks merged through out_acc / lse_acc equal the one call over all keys: an lse that
dropped the row term of the bias would not merge); the backward into plain outputs and, two-phase, into fp32
accumulators; zero slopes through the bias instances against the plain call; and one ring and one zigzag case at W = 2
with the ranks sharing the GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _blockref as AR                           # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
B, H, HK = 2, 4, 2
DIMS = (128, 64, 72, 40)
# (Sq, Sk, causal)
GEOS = ((333, 333, True), (130, 333, True), (130, 333, False), (333, 130, False))


def _blocks():
    """(Sq, Sk, causal, alibi_shift): every geometry on its own diagonal and one block in front; the non-causal ones also one
    block behind and 37 rows off (the kink of |.| inside a tile).  A causal block in front moves its diagonal by the same
    distance (mask_shift), as the ring does."""
    out = []
    for sq, sk, causal in GEOS:
        out += [(sq, sk, causal, 0), (sq, sk, causal, sk)]
        if not causal:
            out += [(sq, sk, causal, -sk), (sq, sk, causal, 37)]
    return out


def _params():
    ps = []
    for sq, sk, causal, shift in _blocks():
        for D in DIMS:
            for dt in (BF, FP16):
                kinds = ("H", "BH") if (D == 128 and dt is BF) else (("BH",) if D == 64 else ("H",))
                for sl in kinds:
                    core = dt is BF and (sq, sk, causal, shift, D, sl) in (
                        (333, 333, True, 0, 128, "H"), (130, 333, False, 37, 128, "BH"), (333, 130, False, -130, 64, "BH"),
                        (130, 333, True, 333, 72, "H"), (333, 333, True, 0, 40, "H"))
                    ps.append(pytest.param(sq, sk, causal, shift, D, dt, sl, marks=[] if core else [_EXT],
                                           id=f"q{sq}-k{sk}-{'causal' if causal else 'full'}-s{shift}-d{D}-"
                                              f"{'bf16' if dt is BF else 'fp16'}-{sl}"))
    return ps


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _slopes(kind, nb=B):
    s = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)
    return s if kind == "H" else torch.stack([s * (1 + 0.5 * b) for b in range(nb)])


class _Case:
    """one seeded input set and its fp64 reference (computed once, shared by the tests that need it, never changed)"""

    def __init__(self, sq, sk, causal, shift, D, dt, sl):
        gen = torch.Generator().manual_seed(9100 + sq + 3 * sk + 7 * D + shift)
        mk = lambda *s: torch.randn(*s, generator=gen).to(dt)
        self.q, self.k, self.v, self.do = mk(B, sq, H, D), mk(B, sk, HK, D), mk(B, sk, HK, D), mk(B, sq, H, D)
        self.slopes = _slopes(sl)
        self.ms = shift if causal else 0
        self.ref = AR.attention(self.q, self.k, self.v, slopes=self.slopes, causal=causal, alibi_shift=shift, shift=self.ms, dout=self.do,
                                autograd=True)
        self.scale = D ** -0.5

    def dev(self):
        d = _dev()
        return tuple(t.to(d) for t in (self.q, self.k, self.v, self.do, self.slopes))


_CASES = {}


def _case(*key):
    if key not in _CASES:
        while len(_CASES) >= 8:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = _Case(*key)
    return _CASES[key]


def _forward(be, q, k, v, scale, causal, **kw):
    out = torch.empty_like(q)
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **kw)
    return out, lse


@pytest.mark.parametrize("sq,sk,causal,shift,D,dt,sl", _params())
def test_block_forward_and_backward(sq, sk, causal, shift, D, dt, sl):
    c = _case(sq, sk, causal, shift, D, dt, sl)
    be = _be()
    q, k, v, do, slopes = c.dev()
    band = {"mask_shift": c.ms} if c.ms else {}
    out, lse = _forward(be, q, k, v, c.scale, causal, alibi=(slopes, shift), **band)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=c.scale, causal=causal, dq=dq, dk=dk, dv=dv, alibi=(slopes, shift), **band)
    torch.cuda.synchronize()
    ro, rl, rdq, rdk, rdv = c.ref
    bad = []
    for name, got, ref, kind in (("out", out, ro, "out"), ("lse", lse, rl, "lse"), ("dq", dq, rdq, "grad"), ("dk", dk, rdk, "grad"),
                                 ("dv", dv, rdv, "grad")):
        m = _tol.metrics(got, ref)
        print(f"{name}: max_err {m['max_err']:.3e} max_ref {m['max_ref']:.3e} fro {m['fro']:.3e} mean_err {m['mean_err']:.3e}")
        bad += _tol.failures(name, got, ref, kind)         # (fp16: the bf16 bounds hold, 3 more mantissa bits)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D,dt", [(128, BF), pytest.param(64, BF, marks=_EXT), pytest.param(72, FP16, marks=_EXT)])
def test_two_phase_backward_into_fp32_accumulators(D, dt):
    """RFA_BWD_COMPUTE then RFA_BWD_REDUCE with the partials, `+=` into fp32 accumulators that hold a known value"""
    from ring_flash_attn import _C

    c = _case(333, 333, True, 0, D, dt, "H")
    be = _be()
    q, k, v, do, slopes = c.dev()
    ro, rl, rdq, rdk, rdv = c.ref
    out, lse = _forward(be, q, k, v, c.scale, True, alibi=(slopes, 0))
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    acc = [torch.full(t.shape, 0.5, dtype=torch.float32, device=q.device) for t in (q, k, v)]
    kw = dict(softmax_scale=c.scale, causal=True, dq_acc=acc[0], dk_acc=acc[1], dv_acc=acc[2], alibi=(slopes, 0))
    part = be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_COMPUTE, **kw)
    be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_REDUCE, partials=part, **kw)
    torch.cuda.synchronize()
    bad = []
    for name, got, ref in zip(("dq", "dk", "dv"), acc, (rdq, rdk, rdv)):
        bad += _tol.failures(name, got - 0.5, ref, "grad")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [128, pytest.param(40, marks=_EXT)])
def test_two_half_key_blocks_merge_to_the_one_call(causal, D):
    """keys [0, 130) and [130, 333) as two block calls with their shifts (S - 130 and 0), merged through out_acc / lse_acc,
    against the one call over all keys and against fp64.  The first block's keys are ALL far from the late rows: if lse dropped
    the per-row part of the bias the merge weights would be wrong by exp(slope * distance)."""
    S, h = 333, 130
    c = _case(S, S, causal, 0, D, BF, "H")
    be = _be()
    q, k, v, do, slopes = c.dev()
    out_acc = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    first = True
    for ks, shift in ((slice(0, h), S - h), (slice(h, S), 0)):
        band = {"mask_shift": shift} if (causal and shift) else {}
        be.fwd(q, k[:, ks], v[:, ks], softmax_scale=c.scale, causal=causal, out_acc=out_acc, lse_acc=lse_acc, acc_init=first,
               alibi=(slopes, shift), **band)
        first = False
    one_out, one_lse = _forward(be, q, k, v, c.scale, causal, alibi=(slopes, 0))
    torch.cuda.synchronize()
    ro, rl = c.ref[:2]
    bad = _tol.failures("merged out vs fp64", out_acc, ro, "out") + _tol.failures("merged lse vs fp64", lse_acc, rl, "lse")
    bad += _tol.failures("merged out vs one call", out_acc, one_out, "out") + _tol.failures("merged lse vs one call", lse_acc, one_lse, "lse")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D,dt", [(128, BF), pytest.param(64, FP16, marks=_EXT), pytest.param(72, BF, marks=_EXT)])
def test_packed_batch_with_unequal_lengths(D, dt):
    """cu_seqlens_q = [0, 24, 64, 200] against longer key sequences, causal (bottom-right aligned) and not, (3, H) slopes"""
    cu_q, cu_k = [0, 24, 64, 200], [0, 30, 100, 333]
    gen = torch.Generator().manual_seed(77 + D)
    mk = lambda t, h: torch.randn(t, h, D, generator=gen).to(dt)
    q, k, v, do = mk(200, H), mk(333, HK), mk(333, HK), mk(200, H)
    slopes = _slopes("BH", 3)
    be, dev = _be(), _dev()
    qd, kd, vd, dod, sd = (t.to(dev) for t in (q, k, v, do, slopes))
    cq, ck = (torch.tensor(c_, dtype=torch.int32, device=dev) for c_ in (cu_q, cu_k))
    vl = dict(cu_seqlens_q=cq, cu_seqlens_k=ck, max_seqlen_q=136, max_seqlen_k=233)
    bad = []
    for causal in (True, False):
        ro, rl, rdq, rdk, rdv = AR.attention(q, k, v, slopes=slopes, causal=causal, dout=do, autograd=True, cu_seqlens_q=cu_q,
                                             cu_seqlens_k=cu_k)
        out, lse = torch.empty_like(qd), torch.empty((H, 200), dtype=torch.float32, device=dev)
        be.fwd(qd, kd, vd, softmax_scale=D ** -0.5, causal=causal, out=out, lse=lse, alibi=(sd, 0), **vl)
        delta = torch.empty_like(lse)
        be.bwd_preprocess(dod, out, delta, cu_seqlens_q=cq, max_seqlen_q=136)
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        be.bwd(dod, qd, kd, vd, lse, delta, softmax_scale=D ** -0.5, causal=causal, dq=dq, dk=dk, dv=dv, alibi=(sd, 0), **vl)
        torch.cuda.synchronize()
        for name, got, ref, kind in (("out", out, ro, "out"), ("lse", lse, rl, "lse"), ("dq", dq, rdq, "grad"),
                                     ("dk", dk, rdk, "grad"), ("dv", dv, rdv, "grad")):
            bad += _tol.failures(f"{'causal' if causal else 'full'} {name}", got, ref, kind)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D", [128, pytest.param(72, marks=_EXT)])
def test_zero_slopes_through_the_bias_instances_equal_the_plain_call(D):
    c = _case(333, 333, True, 0, D, BF, "H")
    be = _be()
    q, k, v, do, _ = c.dev()
    zero = torch.zeros(H, dtype=torch.float32, device=q.device)
    res = []
    for kw in (dict(alibi=(zero, 0)), dict()):
        out, lse = _forward(be, q, k, v, c.scale, True, **kw)
        delta = torch.empty_like(lse)
        be.bwd_preprocess(do, out, delta)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        be.bwd(do, q, k, v, lse, delta, softmax_scale=c.scale, causal=True, dq=dq, dk=dk, dv=dv, **kw)
        res.append((out, lse, dq, dk, dv))
    torch.cuda.synchronize()
    bad = []
    for name, a, b_, kind in zip(("out", "lse", "dq", "dk", "dv"), *res, ("out", "lse", "grad", "grad", "grad")):
        bad += _tol.failures(name, a, b_, kind)
    assert not bad, "; ".join(bad)


def test_public_api_single_rank_and_its_refusals(single_rank_group):
    import ring_flash_attn as R

    _be()
    dev = _dev()
    c = _case(333, 333, True, 0, 64, BF, "BH")
    q, k, v, do, slopes = c.dev()
    qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)
    out, lse, _ = R.zigzag_ring_flash_attn_kvpacked_func(qq, kv, causal=True, alibi_slopes=slopes, return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    ro, rl, rdq, rdk, rdv = c.ref
    bad = _tol.failures("out", out, ro, "out") + _tol.failures("lse", lse, rl, "lse") + _tol.failures("dq", qq.grad, rdq, "grad")
    bad += _tol.failures("dk", kv.grad[:, :, 0], rdk, "grad") + _tol.failures("dv", kv.grad[:, :, 1], rdv, "grad")
    assert not bad, "; ".join(bad)
    big = torch.randn(1, 64, 2, 192, device=dev).bfloat16()
    with pytest.raises(NotImplementedError):
        R.ring_flash_attn_func(big, big, big, causal=True, alibi_slopes=slopes[0, :2].contiguous())
    with pytest.raises(ValueError):
        R.ring_flash_attn_func(q, k, v, causal=True, alibi_slopes=slopes.cpu())


def test_ring_and_zigzag_over_two_ranks_sharing_the_gpu():
    """W = 2, the ranks share cuda:0 (host staging): ring S = 130 per rank, zigzag 2 x 101 rows per rank in the gather form"""
    import _alibi_worker as AW

    cases = [dict(kind="ring", W=2, S=130, causal=True), dict(kind="zigzag", form="gather", W=2, S=202, causal=True)]
    res, errs = AW.run_world(2, cases, True, free_port(), limit_s=240)
    assert not errs, "\n".join(errs)
    bad = []
    for c in cases:
        name = AW.case_name(c)
        (ro, rl, rdq, rdk, rdv), r0 = AW.reference(c)
        out, lse, dq, dk, dv = res[name]
        assert (ro - r0).abs().max() > 0.05, name
        bad += _tol.failures(f"{name} out", out, ro, "out_ring") + _tol.failures(f"{name} lse", lse, rl, "lse_ring")
        for nm, got, ref in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
            bad += _tol.failures(f"{name} {nm}", got, ref, "grad_ring")
    assert not bad, "; ".join(bad)
