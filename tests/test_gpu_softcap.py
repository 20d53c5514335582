"""Logit soft-capping (flash_attn's softcap; include/rfa.h: rfa_ext_args.softcap) in the kernels against fp64
(tests/_blockref.py) through tests/_tol.py (kinds out, lse, grad; *_ring over several ranks): the kCap instances of the
forward, dQ and dK/dV kernels for head dims 128 and 64 (full) and 72 and 40 (the zero-padded layouts), bf16 and fp16, blocks
that are no multiple of a tile, causal and not, in two regimes — softcap = 2.0, where tanh saturates (the reference itself
shows that a dropped cap or a dropped 1 - t^2 would be far outside the tolerance), and the realistic 50.0; with windows, a
band cut inside the block (mask_shift) and a packed batch (mask_shift_lens); accumulate mode; the two-phase backward; an
extension whose cap is 0 against the plain call, bit for bit; and four schedules at W = 2 with the ranks sharing the GPU.

Head dims 65 .. 127 with a cap AND a window are refused by the library (the zero-padded 128-wide windowed dK/dV instance with
a cap does not fit the register file and is not built — profiles/softcap.md): the D = 72 window cases check that refusal."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _blockref as SR                         # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
B, H, HK = 2, 4, 2
DIMS = (128, 64, 72, 40)
CAPS = (2.0, 50.0)
NOWIN = (-1, -1)
# (Sq, Sk, causal)
GEOS = ((333, 333, True), (130, 333, True), (130, 333, False), (333, 130, False))
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


class _Case:
    """one seeded input set and its fp64 reference (computed once, shared by the tests that need it, never changed)"""

    def __init__(self, sq, sk, causal, D, dt, cap, window=NOWIN, shift=0):
        gen = torch.Generator().manual_seed(4400 + sq + 3 * sk + 7 * D)
        mk = lambda *s: torch.randn(*s, generator=gen).to(dt)
        self.q, self.k, self.v, self.do = mk(B, sq, H, D), mk(B, sk, HK, D), mk(B, sk, HK, D), mk(B, sq, H, D)
        self.scale = D ** -0.5
        self.kw = dict(causal=causal, window=window, shift=shift)
        self.ref = SR.attention(self.q, self.k, self.v, softcap=cap, dout=self.do, **self.kw)

    def uncapped(self):
        return SR.attention(self.q, self.k, self.v, dout=self.do, **self.kw)

    def dev(self):
        d = _dev()
        return tuple(t.to(d) for t in (self.q, self.k, self.v, self.do))


_CASES = {}


def _case(*key):
    if key not in _CASES:
        while len(_CASES) >= 8:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = _Case(*key)
    return _CASES[key]


def _run(be, q, k, v, do, scale, causal, **kw):
    """forward and backward into plain outputs: (out, lse, dq, dk, dv)"""
    out = torch.empty_like(q)
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **kw)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _check(got, ref, tag=""):
    bad = []
    for name, g_, r_, kind in zip(NAMES5, got, ref, KINDS5):
        m = _tol.metrics(g_, r_)
        print(f"{tag}{name}: max_err {m['max_err']:.3e} max_ref {m['max_ref']:.3e} fro {m['fro']:.3e} mean_err {m['mean_err']:.3e}")
        bad += _tol.failures(tag + name, g_, r_, kind)             # (fp16: the bf16 bounds hold, 3 more mantissa bits)
    assert not bad, "; ".join(bad)


def _discriminates(c):
    """the suite must not pass on a kernel that ignores the cap: on the fp64 reference itself, capped and uncapped out and
    dq differ by at least 10 x the rtol of their kind (softcap = 2.0 cases)"""
    plain = c.uncapped()
    for i, kind in ((0, "out"), (2, "grad")):
        gap = ((c.ref[i] - plain[i]).abs().max() / c.ref[i].abs().max()).item()
        assert gap >= 10 * _tol.KINDS[kind][1], (NAMES5[i], gap)


def _block_params():
    core = {(333, 333, True, 128, BF, 2.0), (333, 333, True, 128, BF, 50.0), (130, 333, False, 64, BF, 2.0),
            (333, 130, False, 72, FP16, 2.0), (130, 333, True, 40, BF, 50.0)}
    ps = []
    for sq, sk, causal in GEOS:
        for D in DIMS:
            for dt in (BF, FP16):
                for cap in CAPS:
                    ps.append(pytest.param(sq, sk, causal, D, dt, cap, marks=[] if (sq, sk, causal, D, dt, cap) in core else [_EXT],
                                           id=f"q{sq}-k{sk}-{'causal' if causal else 'full'}-d{D}-"
                                              f"{'bf16' if dt is BF else 'fp16'}-cap{cap:g}"))
    return ps


@pytest.mark.parametrize("sq,sk,causal,D,dt,cap", _block_params())
def test_block_forward_and_backward(sq, sk, causal, D, dt, cap):
    c = _case(sq, sk, causal, D, dt, cap)
    if cap == 2.0:
        _discriminates(c)
    q, k, v, do = c.dev()
    _check(_run(_be(), q, k, v, do, c.scale, causal, softcap=cap), c.ref)


def _window_params():
    ps = []
    for causal, window in ((True, (100, -1)), (False, (64, 32))):
        for shift in (0, 333):
            for D in (128, 64, 72):
                core = (causal, shift, D) in ((True, 0, 128), (False, 333, 64), (True, 333, 72))
                ps.append(pytest.param(causal, window, shift, D, marks=[] if core else [_EXT],
                                       id=f"{'causal' if causal else 'full'}-w{window[0]}_{window[1]}-s{shift}-d{D}"))
    return ps


@pytest.mark.parametrize("causal,window,shift,D", _window_params())
def test_windowed_blocks(causal, window, shift, D):
    """causal with window_left = 100, non-causal with (64, 32); shift = Sk: the block sits one block in front, the band is
    cut inside it (rows past the band see nothing: lse = +inf, out = 0)"""
    S, cap = 333, 2.0
    be = _be()
    if D == 72:
        # not built (module docstring): refused by the forward and by the backward, nothing is launched
        dev = _dev()
        q = torch.zeros(B, S, H, D, dtype=BF, device=dev)
        k = torch.zeros(B, S, HK, D, dtype=BF, device=dev)
        lse = torch.zeros(B, H, S, dtype=torch.float32, device=dev)
        kw = dict(softmax_scale=D ** -0.5, causal=causal, window=window, mask_shift=shift, softcap=cap)
        with pytest.raises(RuntimeError, match="rfa_fwd_ex"):
            be.fwd(q, k, k, out=torch.empty_like(q), lse=lse, **kw)
        with pytest.raises(RuntimeError, match="rfa_bwd_ex"):
            be.bwd(q, q, k, k, lse, lse, dq=torch.empty_like(q), dk=torch.empty_like(k), dv=torch.empty_like(k), **kw)
        return
    c = _case(S, S, causal, D, BF, cap, window, shift)
    _discriminates(c)
    q, k, v, do = c.dev()
    _check(_run(be, q, k, v, do, c.scale, causal, softcap=cap, window=window, mask_shift=shift), c.ref)


@pytest.mark.parametrize("shift_lens", [0, 1])
@pytest.mark.parametrize("D,dt", [(128, BF), pytest.param(64, FP16, marks=_EXT)])
def test_packed_batch_with_unequal_lengths_and_a_window(D, dt, shift_lens):
    """cu_seqlens_q = [0, 24, 64, 200] against longer key sequences, causal with window_left = 100; mask_shift_lens = 1 puts
    every sequence's block one own key length in front (the packed ring's band)"""
    cu_q, cu_k = [0, 24, 64, 200], [0, 30, 100, 333]
    cap, window = 2.0, (100, -1)
    gen = torch.Generator().manual_seed(91 + D)
    mk = lambda t, h: torch.randn(t, h, D, generator=gen).to(dt)
    q, k, v, do = mk(200, H), mk(333, HK), mk(333, HK), mk(200, H)
    ref = SR.attention(q, k, v, softcap=cap, causal=True, window=window, shift_lens=shift_lens, dout=do, cu_seqlens_q=cu_q,
                       cu_seqlens_k=cu_k)
    be, dev = _be(), _dev()
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    cq, ck = (torch.tensor(c_, dtype=torch.int32, device=dev) for c_ in (cu_q, cu_k))
    kw = dict(softmax_scale=D ** -0.5, causal=True, window=window, softcap=cap, cu_seqlens_q=cq, cu_seqlens_k=ck,
              max_seqlen_q=136, max_seqlen_k=233)
    if shift_lens:
        kw["mask_shift_lens"] = shift_lens
    out, lse = torch.empty_like(qd), torch.empty((H, 200), dtype=torch.float32, device=dev)
    be.fwd(qd, kd, vd, out=out, lse=lse, **kw)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(dod, out, delta, cu_seqlens_q=cq, max_seqlen_q=136)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    be.bwd(dod, qd, kd, vd, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
    torch.cuda.synchronize()
    _check((out, lse, dq, dk, dv), ref)


@pytest.mark.parametrize("causal", [True, pytest.param(False, marks=_EXT)])
@pytest.mark.parametrize("D,cap", [(128, 2.0), pytest.param(40, 50.0, marks=_EXT)])
def test_two_half_key_blocks_merge_to_the_one_call(causal, D, cap):
    """keys [0, 130) and [130, 333) as two block calls merged through out_acc / lse_acc, against the one call over all keys
    and against fp64: lse must be the log-sum-exp of the CAPPED scores for the blocks to merge"""
    S, h = 333, 130
    c = _case(S, S, causal, D, BF, cap)
    be = _be()
    q, k, v, do = c.dev()
    out_acc = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    first = True
    for ks, shift in ((slice(0, h), S - h), (slice(h, S), 0)):
        band = {"mask_shift": shift} if (causal and shift) else {}
        be.fwd(q, k[:, ks], v[:, ks], softmax_scale=c.scale, causal=causal, out_acc=out_acc, lse_acc=lse_acc, acc_init=first,
               softcap=cap, **band)
        first = False
    one_out = torch.empty_like(q)
    one_lse = torch.empty_like(lse_acc)
    be.fwd(q, k, v, softmax_scale=c.scale, causal=causal, out=one_out, lse=one_lse, softcap=cap)
    torch.cuda.synchronize()
    ro, rl = c.ref[:2]
    bad = _tol.failures("merged out vs fp64", out_acc, ro, "out") + _tol.failures("merged lse vs fp64", lse_acc, rl, "lse")
    bad += _tol.failures("merged out vs one call", out_acc, one_out, "out") + _tol.failures("merged lse vs one call", lse_acc, one_lse, "lse")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D,dt,window", [(128, BF, NOWIN), pytest.param(64, BF, (100, -1), marks=_EXT),
                                         pytest.param(72, FP16, NOWIN, marks=_EXT)])
def test_two_phase_backward_into_fp32_accumulators(D, dt, window):
    """RFA_BWD_COMPUTE then RFA_BWD_REDUCE with the partials, `+=` into fp32 accumulators that hold a known value"""
    from ring_flash_attn import _C

    cap = 2.0
    c = _case(333, 333, True, D, dt, cap, window)
    be = _be()
    q, k, v, do = c.dev()
    ro, rl, rdq, rdk, rdv = c.ref
    out = torch.empty_like(q)
    lse = torch.empty((B, H, 333), dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=c.scale, causal=True, out=out, lse=lse, softcap=cap, window=window)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    acc = [torch.full(t.shape, 0.5, dtype=torch.float32, device=q.device) for t in (q, k, v)]
    kw = dict(softmax_scale=c.scale, causal=True, dq_acc=acc[0], dk_acc=acc[1], dv_acc=acc[2], softcap=cap, window=window)
    part = be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_COMPUTE, **kw)
    be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_REDUCE, partials=part, **kw)
    torch.cuda.synchronize()
    bad = []
    for name, got, ref in zip(("dq", "dk", "dv"), acc, (rdq, rdk, rdv)):
        bad += _tol.failures(name, got - 0.5, ref, "grad")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("D,window", [(128, NOWIN), pytest.param(64, (100, -1), marks=_EXT)])
def test_an_extension_with_softcap_zero_is_the_plain_call_bit_for_bit(D, window, monkeypatch):
    """the calls go through rfa_fwd_ex / rfa_bwd_ex with an extension whose features are all off; the plain backward is held
    to the forms the backend names for an extension (the 128-key dK/dV kernel, no dS hand-off) so that both run one plan"""
    from ring_flash_attn import _C, backend

    monkeypatch.setenv("RFA_FWD_KV_NSPLIT", "1")                    # (the *_ex path passes no split-KV workspace)
    monkeypatch.setenv("RFA_DKDV_WIDE", "0")
    monkeypatch.setenv("RFA_BWD_DS_SPILL", "0")
    c = _case(333, 333, True, D, BF, 2.0, window)
    be = _be()
    q, k, v, do = c.dev()
    plain = _run(be, q, k, v, do, c.scale, True, window=window)
    made = []

    def all_off(alibi, q_, softcap=0.0):
        e = _C.ExtArgs()
        assert e.softcap == 0.0 and e.alibi_slopes is None
        made.append(e)
        return e

    monkeypatch.setattr(backend, "_ext_args", all_off)
    through_ex = _run(be, q, k, v, do, c.scale, True, window=window)
    assert len(made) == 2                                           # forward and backward both took the *_ex entry
    for name, a_, b_ in zip(NAMES5, plain, through_ex):
        assert torch.equal(a_, b_), name


def test_public_api_single_rank(single_rank_group):
    """with_softcap on a single-rank group, Gemma-2's pair: softcap 50 and a sliding window"""
    import ring_flash_attn as R

    _be()
    c = _case(333, 333, True, 128, BF, 50.0, (100, -1))
    q, k, v, do = c.dev()
    qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)
    fn = R.with_softcap(R.ring_flash_attn_kvpacked_func, 50.0)
    out, lse, _ = fn(qq, kv, causal=True, window_size=(100, 0), return_attn_probs=True)
    out.backward(do)
    torch.cuda.synchronize()
    _check((out, lse, qq.grad, kv.grad[:, :, 0], kv.grad[:, :, 1]), c.ref)
    d72 = torch.zeros(1, 64, 2, 72, dtype=BF, device=_dev())
    with pytest.raises(NotImplementedError):
        R.with_softcap(R.ring_flash_attn_func, 50.0)(d72, d72, d72, causal=True, window_size=(16, 0))


MULTI = [
    dict(kind="ring", W=2, S=128, D=128, causal=True, softcap=2.0),
    dict(kind="zigzag_varlen", W=2, S=128, D=128, causal=True, softcap=2.0, lens=[96, 160]),
    dict(kind="stripe", W=2, S=128, D=128, causal=True, softcap=2.0, window=(100, 0)),
    dict(kind="ring_varlen", W=2, S=128, D=128, causal=True, softcap=2.0, lens=[96, 160], window=(100, 0)),
]


def test_four_schedules_over_two_ranks_sharing_the_gpu():
    """W = 2, the ranks share cuda:0 (host staging), S = 128 rows per rank, D = 128, softcap = 2.0: the dense ring, zigzag
    varlen (the halves), stripe with a window, ring varlen with a window — each against ONE single-device fp64 call"""
    import _softcap_worker as SW

    for c in MULTI:
        capped, plain = SW.reference(c), SW.reference(c, softcap=0.0)
        for i, kd in ((0, "out_ring"), (2, "grad_ring")):
            gap = ((capped[i] - plain[i]).abs().max() / capped[i].abs().max()).item()
            assert gap >= 10 * _tol.KINDS[kd][1], (SW.case_name(c), i, gap)
    errs, notes = SW.run_world(2, MULTI, True, free_port(), limit_s=240)
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
