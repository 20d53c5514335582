"""ALiBi (alibi_slopes), no device: the extension entry points of the C ABI (symbols, layout, the refusals that can be
tested with NULL tensors), the shift arithmetic of the ring and zigzag schedules against positions written out by hand,
the schedules under gloo through the public functions against ONE single-device biased call (tests/_blockref.py, fp64;
CPU oracle with `alibi=`, tests/_ref_backend.py), and what must be refused."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _blockref as AR                           # noqa: E402
import _alibi_worker as AW                       # noqa: E402
import _tol                                      # noqa: E402

ERR_NULL, ERR_ARGS = -1, -8
NEW = ("rfa_fwd_ex", "rfa_bwd_ex", "rfa_ext_args_bytes")


# ---------------------------------------------------------------------------------------------- C ABI
def test_extension_symbols_are_declared_exported_and_bound(built):
    from ring_flash_attn import _C

    hdr = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    lib = _C.load()
    for name in NEW:
        assert f" {name}(" in hdr, name
        assert f" {name}\n" in exported, name
        assert name in _C.SYMBOLS and hasattr(lib, name), name
    # no existing struct changed: version and revision stay
    assert _C.RFA_ABI_VERSION == 8 and lib.rfa_abi_version() == 8
    assert _C.RFA_ABI_REVISION == 1 and lib.rfa_abi_revision() == 1
    assert "#define RFA_ABI_VERSION 8" in hdr and "#define RFA_ABI_REVISION 1" in hdr
    assert lib.rfa_ext_args_bytes() == C.sizeof(_C.ExtArgs)


def test_ext_args_match_the_c_layout(built):
    from ring_flash_attn import _C

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rfa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rfa_ext_args), offsetof(rfa_ext_args, struct_bytes),
         offsetof(rfa_ext_args, reserved), offsetof(rfa_ext_args, alibi_slopes),
         offsetof(rfa_ext_args, alibi_batch_stride), offsetof(rfa_ext_args, alibi_shift));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    E = _C.ExtArgs
    assert got == [C.sizeof(E), E.struct_bytes.offset, E.reserved.offset, E.alibi_slopes.offset,
                   E.alibi_batch_stride.offset, E.alibi_shift.offset]
    assert E().struct_bytes == C.sizeof(E)                      # the binding fills it in


def test_ex_with_a_null_extension_returns_the_codes_of_the_plain_call(built):
    """the sequence of tests/test_abi.py::test_argument_errors_without_device through rfa_fwd_ex(args, NULL) / rfa_bwd_ex"""
    from ring_flash_attn import _C

    lib = _C.load()
    assert lib.rfa_fwd_ex(None, None, None) == -1
    a = _C.FwdArgs()
    a.B, a.H, a.Hk, a.D, a.Sq, a.Sk, a.dtype = 1, 4, 3, 64, 8, 8, 0
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == -4                # H % Hk
    a.Hk, a.D = 2, 264
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == -3                # head dim: above 256 ...
    a.D = 132
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == -3                # ... or not a multiple of 8
    a.D, a.dtype = 64, 7
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == -2                # dtype
    a.dtype = 0
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == -1                # q/k/v NULL
    e = _C.ExtArgs()                                                   # an extension with everything off: the same
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(e), None) == -1
    a.Sq = 0
    assert lib.rfa_fwd_ex(C.byref(a), None, None) == 0                 # empty problem is a no-op
    b = _C.BwdArgs()
    b.B, b.H, b.Hk, b.D, b.Sq, b.Sk, b.dtype = 1, 4, 2, 64, 8, 8, 0
    assert lib.rfa_bwd_ex(None, None, None) == -1
    assert lib.rfa_bwd_ex(C.byref(b), None, None) == -1
    assert lib.rfa_bwd_ex(C.byref(b), C.byref(e), None) == -1


def _fwd(**kw):
    from ring_flash_attn import _C

    a = _C.FwdArgs()
    a.B, a.H, a.Hk, a.D, a.Sq, a.Sk, a.dtype, a.softmax_scale = 1, 4, 2, 64, 128, 128, 0, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(**kw):
    from ring_flash_attn import _C

    b = _C.BwdArgs()
    b.B, b.H, b.Hk, b.D, b.Sq, b.Sk, b.dtype, b.softmax_scale = 1, 4, 2, 64, 128, 128, 0, 0.125
    b.total_k, b.dkdv_form = 128, _C.DKDV_128
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _ext(**kw):
    from ring_flash_attn import _C

    e = _C.ExtArgs()
    e.alibi_slopes = 256                                        # a non-NULL address that is never dereferenced
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_extension_struct_size_contract(built):
    from ring_flash_attn import _C

    lib = _C.load()
    a = _fwd()
    ok_code = ERR_NULL                                          # an accepted extension reaches the base struct's NULL tensors
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(_ext()), None) == ok_code
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(_ext(reserved=1)), None) == ERR_ARGS
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(_ext(struct_bytes=4)), None) == ERR_ARGS        # below the fixed head
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(_ext(struct_bytes=8)), None) == ok_code         # head only: everything reads 0
    # a shorter struct: the missing tail reads as zero — alibi_shift (a refusable value) is not seen
    short = _ext(alibi_shift=1 << 40, struct_bytes=_C.ExtArgs.alibi_shift.offset)
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(short), None) == ok_code
    assert lib.rfa_fwd_ex(C.byref(a), C.byref(_ext(alibi_shift=1 << 40)), None) == ERR_ARGS

    class Longer(C.Structure):
        _fields_ = [("e", _C.ExtArgs), ("tail", C.c_int64)]

    big = Longer()
    big.e = _ext(struct_bytes=C.sizeof(Longer))
    assert lib.rfa_fwd_ex(C.byref(a), C.cast(C.byref(big), C.POINTER(_C.ExtArgs)), None) == ok_code   # a zero tail
    big.tail = 1
    assert lib.rfa_fwd_ex(C.byref(a), C.cast(C.byref(big), C.POINTER(_C.ExtArgs)), None) == ERR_ARGS
    assert lib.rfa_bwd_ex(C.byref(_bwd()), C.cast(C.byref(big), C.POINTER(_C.ExtArgs)), None) == ERR_ARGS


def test_every_bias_refusal_returns_err_args_with_null_tensors(built):
    from ring_flash_attn import _C

    lib = _C.load()
    cu = 256                                                    # a non-NULL cu_seqlens address, never dereferenced either
    bad = {
        "a bounded window that survives normalisation": (dict(window=1, window_left=16, window_right=-1), {}),
        "a right window without causal": (dict(window=1, window_left=-1, window_right=16), {}),
        "dropout": (dict(dropout_p=0.1), {}),
        "head dim 136": (dict(D=136), {}),
        "a shift with cu_seqlens": (dict(cu_seqlens_q=cu, cu_seqlens_k=cu), dict(alibi_shift=128)),
        "|shift| + Sq + Sk = 2^31": (dict(), dict(alibi_shift=(1 << 31) - 256)),
        "a negative shift as large": (dict(), dict(alibi_shift=-((1 << 31) - 256))),
        "softmax_scale 0": (dict(softmax_scale=0.0), {}),
        "softmax_scale < 0": (dict(softmax_scale=-0.125), {}),
        "a negative batch stride": (dict(), dict(alibi_batch_stride=-4)),
    }
    for what, (akw, ekw) in bad.items():
        assert lib.rfa_fwd_ex(C.byref(_fwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_ARGS, f"fwd: {what}"
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_ARGS, f"bwd: {what}"
    fine = {
        "a window the band normalisation drops": (dict(window=1, window_left=500, window_right=-1), {}),
        "the largest shift": (dict(), dict(alibi_shift=(1 << 31) - 257)),
        "a shifted causal diagonal": (dict(causal=1, mask_shift=64), dict(alibi_shift=64)),
        "a batch stride": (dict(B=2), dict(alibi_batch_stride=4)),
        "packed input": (dict(cu_seqlens_q=cu, cu_seqlens_k=cu), {}),
        # forward forms that do not exist for a bias read as AUTO (the base struct's own range check stays)
    }
    for what, (akw, ekw) in fine.items():
        assert lib.rfa_fwd_ex(C.byref(_fwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_NULL, f"fwd: {what}"
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_NULL, f"bwd: {what}"
    for form in (_C.FWD_4x32, _C.FWD_P8x32):
        assert lib.rfa_fwd_ex(C.byref(_fwd(fwd_form=form, kv_nsplit=4)), C.byref(_ext()), None) == ERR_NULL
    # the backward must already PLAN to the bias forms: the 128-key dK/dV kernel, no dS scratch
    for akw in (dict(dkdv_form=_C.DKDV_AUTO), dict(dkdv_form=_C.DKDV_256), dict(dkdv_form=_C.DKDV_BAL), dict(ds_scratch=256)):
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext()), None) == ERR_ARGS, akw
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), None, None) == ERR_NULL, akw                  # (fine without a bias)
    form, ns, five = C.c_int32(), C.c_int32(), C.c_int32()
    b = _bwd(D=128, Sq=8192, Sk=8192, H=32, Hk=8, causal=1, total_k=8192)
    assert lib.rfa_bwd_plan(C.byref(b), C.byref(form), C.byref(ns), C.byref(five)) == 0
    assert (form.value, ns.value, five.value) == (_C.DKDV_128, 1, 0)      # what HipBackend.bwd sets for a bias call
    # a block with no visible element has nothing to bias: it is the call without the extension (here: reaches the NULLs)
    dark = dict(causal=1, mask_shift=-4096)
    assert lib.rfa_fwd_ex(C.byref(_fwd(**dark)), C.byref(_ext(alibi_shift=-4096)), None) == ERR_NULL
    assert lib.rfa_bwd_ex(C.byref(_bwd(dkdv_form=_C.DKDV_AUTO, **dark)), C.byref(_ext(alibi_shift=-4096)), None) == ERR_NULL


def test_load_refuses_a_library_without_the_extension(built, monkeypatch):
    from ring_flash_attn import _C

    real = C.CDLL(built.LIB)

    class Old:
        """the library as it was before the extension entry points: same version, same revision"""
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(C, "CDLL", lambda path: Old())
    with pytest.raises(RuntimeError, match="rebuild"):
        _C.load()


def test_backend_fills_the_extension_and_plans_the_bias_forms():
    from ring_flash_attn import _C
    from ring_flash_attn.backend import HipBackend, _ext_args

    assert HipBackend.serves_alibi is True
    q = torch.zeros(2, 4, 4, 8)
    assert _ext_args(None, q) is None and _ext_args((None, 3), q) is None
    s1, s2 = torch.ones(4), torch.ones(2, 4)
    e = _ext_args((s1, 260), q)
    assert (e.struct_bytes, e.reserved, e.alibi_slopes, e.alibi_batch_stride, e.alibi_shift) == \
        (C.sizeof(_C.ExtArgs), 0, s1.data_ptr(), 0, 260)
    e = _ext_args((s2[:, 2:], -130), q)                       # a head-group slice: a pointer offset, the batch stride stays
    assert (e.alibi_slopes, e.alibi_batch_stride, e.alibi_shift) == (s2.data_ptr() + 8, 4, -130)
    with pytest.raises(ValueError):
        _ext_args((s1.double(), 0), q)


# ---------------------------------------------------------------------------------------------- shift arithmetic
def test_ring_and_zigzag_shifts_against_positions_written_out_by_hand():
    """W = 2, chunks of 3 rows.  The bias of a block call is |i + (len_k - len_q) + alibi_shift - j| in LOCAL rows; it must
    equal |global position of the query - global position of the key| written out by hand."""
    from ring_flash_attn._common import alibi_kw
    from ring_flash_attn.ring_flash_attn import _band, ring_window_plan
    from ring_flash_attn.zigzag_ring_flash_attn import zigzag_window_pairs

    sl = torch.ones(2)
    assert alibi_kw(None, 5) == {} and alibi_kw(sl, 5)["alibi"][1] == 5
    assert alibi_kw(torch.ones(2, 4), 0, heads=slice(2, 4))["alibi"][0].shape == (2, 2)
    # ring, S = 3: rank 0 holds rows 0 1 2, rank 1 rows 3 4 5.  Step d: the K/V of rank (r - d) mod 2 are on hand.
    pos = {0: [0, 1, 2], 1: [3, 4, 5]}
    for causal in (True, False):
        for rank in (0, 1):
            n_steps, dists = ring_window_plan(rank, 2, 3, causal, (-1, -1))
            assert n_steps == 2
            for d, t in enumerate(dists):
                src = (rank - d) % 2
                if t is None:
                    assert causal and src > rank                 # keys behind the queries: nothing visible
                    continue
                kw = _band(causal, (-1, -1), t, 3, sl)
                shift = kw["alibi"][1]
                assert shift == {(0, 0): 0, (1, 1): 0, (1, 0): 3, (0, 1): -3}[(rank, src)]
                assert kw.get("mask_shift", 0) == shift          # the causal diagonal moves with the same distance
                want = torch.tensor([[abs(i - j) for j in pos[src]] for i in pos[rank]], dtype=torch.float64)
                assert torch.equal(AR.bias(3, 3, shift), want)
    # zigzag, C = 3: rank 0 holds chunks 0 and 3 (rows 0 1 2 | 9 10 11), rank 1 chunks 1 and 2 (rows 3 4 5 | 6 7 8)
    chunk = lambda c: [3 * c, 3 * c + 1, 3 * c + 2]
    chunks = {0: (0, 3), 1: (1, 2)}
    seen = set()
    for rank in (0, 1):
        for src in (0, 1):
            for hq, hk, shift in zigzag_window_pairs(rank, src, 2, 3, -1):
                cq, ck = chunks[rank][hq], chunks[src][hk]
                assert shift == (cq - ck) * 3 and cq >= ck
                want = torch.tensor([[abs(i - j) for j in chunk(ck)] for i in chunk(cq)], dtype=torch.float64)
                assert torch.equal(AR.bias(3, 3, shift), want)
                seen.add((cq, ck))
    assert seen == {(cq, ck) for cq in range(4) for ck in range(4) if ck <= cq}      # every causal chunk pair, once
    assert zigzag_window_pairs(0, 1, 2, 3, -1) == [(1, 0, 6), (1, 1, 3)]                 # chunk 3 against chunks 1 and 2


# ---------------------------------------------------------------------------------------------- schedules under gloo
def _cases(W):
    zz = lambda form, **kw: dict(kind="zigzag", form=form, W=W, S=202, causal=True, **kw)
    cases = [dict(kind="ring", W=W, S=130, causal=True), dict(kind="ring", W=W, S=130, causal=False),
             zz("ring"), zz("gather"), zz("gather_ps"), dict(kind="llama3", W=W, S=208 // W * 2, causal=True)]
    if W == 2:
        cases += [dict(kind="ring", W=W, S=130, causal=True, slopes="BH"), zz("gather", api="kvpacked"),
                  dict(kind="ring", W=W, S=130, causal=False, api="qkvpacked"),
                  dict(kind="llama3", W=W, S=208, causal=True, stride=2, api="kvpacked"), dict(refusals=True)]
    return cases


_REF = {}


def _reference(c):
    """one single-device fp64 call per (layout, unsharded shape, mask, slopes): shared by every schedule that un-shards to it"""
    key = (c["kind"] == "llama3", c["W"] * c["S"], c["causal"], c.get("api") == "qkvpacked", c.get("slopes", "H"))
    if key not in _REF:
        _REF[key] = AW.reference(c)
    return _REF[key]


def _check_world(W, cases):
    res, errs = AW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs)
    for c in cases:
        if c.get("refusals"):
            continue
        name = AW.case_name(c)
        (ro, rl, rdq, rdk, rdv), r0 = _reference(c)
        out, lse, dq, dk, dv = res[name]
        assert (ro - r0).abs().max() > 0.05, name                                      # the bias did something
        _tol.compare(f"{name} out", out, ro, "out_ring")
        _tol.compare(f"{name} lse", lse, rl, "lse_ring")
        for nm, got, ref in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
            _tol.compare(f"{name} {nm}", got, ref, "grad_ring")


@pytest.mark.parametrize("W", [2, 4])
def test_alibi_over_ranks_equals_the_single_device_call(W):
    """ring (causal and not, S = 130 per rank), zigzag in every exchange form (2 x 101 rows per rank) and causal llama3 (the
    reference's [0, 7, 14, 16] fixture scaled to 416 tokens) at W = 2 and 4, B = 2, H = 4, Hk = 2, D = 64, slopes
    2^(-8 (h + 1) / H); at W = 2 also (B, H) slopes, one kv-packed and one qkv-packed call, llama3 with two K/V heads per
    group, and what must be refused.  Fails on a tree without the feature with AssertionError."""
    _check_world(W, _cases(W))


def test_single_rank_group_serves_every_function(single_rank_group):
    """shift 0: dense, *_varlen, llama3 and zigzag_llama3 through the public functions on a single-rank group"""
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _ref_backend import RefBackend

    _testing.set_backend(RefBackend(serves=("mask_shift", "alibi")))
    g = torch.Generator().manual_seed(5)
    Bq, S, Hh, Hk, Dd = 2, 48, 4, 2, 32
    q, k, v, do = (torch.randn(Bq, S, h, Dd, generator=g).bfloat16() for h in (Hh, Hk, Hk, Hh))
    sl = torch.tensor([2.0 ** (-8.0 * (h + 1) / Hh) for h in range(Hh)], dtype=torch.float32)
    sl2 = torch.stack([sl, 1.5 * sl])

    def check(name, fn, args, ref_kw, slopes, tensors, dout):
        ins = [t.clone().requires_grad_(True) for t in tensors]
        out, lse, _ = fn(*ins, *args, alibi_slopes=slopes, return_attn_probs=True)
        out.backward(dout)
        ro, rl, rdq, rdk, rdv = AR.attention(*tensors, slopes=slopes, dout=dout, autograd=True, **ref_kw)
        _tol.compare(f"{name} out", out, ro, "out_ring")
        _tol.compare(f"{name} lse", lse, rl, "lse_ring")
        for nm, got, ref in zip(("dq", "dk", "dv"), (t.grad for t in ins), (rdq, rdk, rdv)):
            _tol.compare(f"{name} {nm}", got, ref, "grad_ring")

    for fn, causal in ((R.ring_flash_attn_func, False), (R.ring_flash_attn_func, True), (R.zigzag_ring_flash_attn_func, True),
                       (R.stripe_flash_attn_func, True)):
        for slopes in (sl, sl2):
            check(fn.__name__, lambda *a, **kw: fn(*a, causal=causal, **kw), (), dict(causal=causal), slopes, (q, k, v), do)
    cu = torch.tensor([0, 20, 48], dtype=torch.int32)
    pq, pk, pv, pdo = q[0], k[0], v[0], do[0]
    pref = dict(causal=True, cu_seqlens_q=cu.tolist(), cu_seqlens_k=cu.tolist())
    for fn in (R.ring_flash_attn_varlen_func, R.zigzag_ring_flash_attn_varlen_func):
        for slopes in (sl, sl2):
            check(fn.__name__, lambda *a, **kw: fn(*a, causal=True, **kw), (cu, 28), pref, slopes, (pq, pk, pv), pdo)
    cq, ck, mq, mk, ks = R.llama3_flash_attn_prepare_cu_seqlens(cu, True, 0, 1)
    for causal in (True, False):
        check("llama3", lambda *a, **kw: R.llama3_flash_attn_varlen_func(*a, heads_k_stride=1, local_k_slice=ks, causal=causal, **kw),
              (cq, ck, mq, mk), dict(pref, causal=causal), sl2, (pq, pk, pv), pdo)
    check("zigzag_llama3", lambda *a, **kw: R.zigzag_llama3_flash_attn_varlen_func(*a, causal=True, **kw), (cu,), pref, sl,
          (pq, pk, pv), pdo)
    with pytest.raises(NotImplementedError):
        R.zigzag_llama3_flash_attn_varlen_func(pq, pk, pv, cu, causal=False, alibi_slopes=sl)
    with pytest.raises(NotImplementedError):
        R.zigzag_llama3_flash_attn_varlen_func(pq, pk, pv, cu, causal=True, alibi_slopes=sl2)
    with pytest.raises(NotImplementedError):
        R.ring_flash_attn_func(q, k, v, causal=True, window_size=(8, 0), alibi_slopes=sl)
    with pytest.raises(ValueError):
        R.ring_flash_attn_func(q, k, v, causal=True, alibi_slopes=sl.bfloat16())


def test_require_alibi_and_the_check():
    from oracle.oracle_backend import OracleBackend
    from ring_flash_attn import _api
    from ring_flash_attn._common import check_alibi_slopes, require_alibi
    from _ref_backend import RefBackend

    with pytest.raises(NotImplementedError, match="alibi"):
        require_alibi(OracleBackend(), "ring_flash_attn")
    require_alibi(RefBackend(serves=("mask_shift", "alibi")), "ring_flash_attn")
    q = torch.zeros(2, 8, 4, 16)
    assert check_alibi_slopes(None, q, 2) is None
    assert check_alibi_slopes(torch.ones(4), q, 2).shape == (4,) and check_alibi_slopes(torch.ones(2, 4), q, 2).shape == (2, 4)
    for bad in (torch.ones(4).double(), torch.ones(3), torch.ones(3, 4), torch.ones(2, 4, 1), [0.5] * 4):
        with pytest.raises(ValueError):
            check_alibi_slopes(bad, q, 2)
    sl = torch.ones(4)
    _api._check_unsupported(0.0, (-1, -1), sl, windows_ok=True, alibi_ok=True)
    _api._check_unsupported(0.0, (-1, -1), None)                                   # the positional signature stays
    for kw in (dict(), dict(windows_ok=True), dict(windows_ok=True, alibi_ok=False)):
        with pytest.raises(NotImplementedError):
            _api._check_unsupported(0.0, (-1, -1), sl, **kw)
    with pytest.raises(NotImplementedError):
        _api._check_unsupported(0.1, (-1, -1), sl, windows_ok=True, alibi_ok=True)
    with pytest.raises(NotImplementedError):
        _api._check_unsupported(0.0, (8, 0), sl, windows_ok=True, alibi_ok=True)
