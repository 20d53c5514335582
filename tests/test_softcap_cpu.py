"""Logit soft-capping (flash_attn's softcap), no device: the grown rfa_ext_args of the C ABI (layout, the size contract, every
refusal that can be tested with NULL tensors), what HipBackend puts into the struct, `ring_flash_attn.with_softcap`, the
Hugging Face adapter, the value on every block call of every schedule family (a recording backend under gloo), and the
schedules' numerics against ONE single-device capped call (tests/_blockref.py, fp64; CPU oracle with `softcap=`,
tests/_ref_backend.py)."""
import ctypes as C
import inspect
import math
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
import _blockref as SR                         # noqa: E402
import _softcap_worker as SW                     # noqa: E402
import _tol                                      # noqa: E402

ERR_NULL, ERR_ARGS = -1, -8


# ---------------------------------------------------------------------------------------------- C ABI
def test_grown_ext_args_match_the_c_layout_and_the_version_stays(built):
    from ring_flash_attn import _C

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rfa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(rfa_ext_args), offsetof(rfa_ext_args, alibi_shift),
         offsetof(rfa_ext_args, softcap), offsetof(rfa_ext_args, softcap_pad), sizeof(((rfa_ext_args *)0)->softcap));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    E = _C.ExtArgs
    assert got == [C.sizeof(E), E.alibi_shift.offset, E.softcap.offset, E.softcap_pad.offset, 4]
    assert E.softcap.offset == E.alibi_shift.offset + 8 and C.sizeof(E) == E.softcap_pad.offset + 4   # grown at the END
    lib = _C.load()
    assert lib.rfa_ext_args_bytes() == C.sizeof(E) == 40
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    assert "softcap" not in exported                               # no new exported symbol


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
    e.softcap = 50.0
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_a_struct_cut_in_front_of_softcap_is_the_plain_call_and_the_pad_must_be_zero(built):
    from ring_flash_attn import _C

    lib = _C.load()
    cut = _C.ExtArgs.softcap.offset
    # a value that would be refused (negative) is not seen through a struct that ends in front of it; the dS scratch a
    # capped backward refuses is accepted: the call is the plain one (it reaches the base struct's NULL tensors)
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap=-1.0, struct_bytes=cut)), None) == ERR_NULL
    assert lib.rfa_bwd_ex(C.byref(_bwd(ds_scratch=256, dkdv_form=_C.DKDV_AUTO)), C.byref(_ext(struct_bytes=cut)), None) == ERR_NULL
    assert lib.rfa_bwd_ex(C.byref(_bwd(ds_scratch=256)), C.byref(_ext()), None) == ERR_ARGS             # (seen: refused)
    # ... a struct that ends behind softcap but in front of the pad reads the pad as 0
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap_pad=7, struct_bytes=cut + 4)), None) == ERR_NULL
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap_pad=7)), None) == ERR_ARGS
    assert lib.rfa_bwd_ex(C.byref(_bwd()), C.byref(_ext(softcap_pad=1)), None) == ERR_ARGS
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap=0.0, softcap_pad=1)), None) == ERR_ARGS  # with the cap off too
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext()), None) == ERR_NULL


def test_every_softcap_refusal_returns_err_args_with_null_tensors(built):
    from ring_flash_attn import _C

    lib = _C.load()
    cu = 256                                                    # a non-NULL address that is never dereferenced
    for bad in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), -float("inf")):
        assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap=bad)), None) == ERR_ARGS, bad
        assert lib.rfa_bwd_ex(C.byref(_bwd()), C.byref(_ext(softcap=bad)), None) == ERR_ARGS, bad
        assert lib.rfa_fwd_ex(None, C.byref(_ext(softcap=bad)), None) == ERR_NULL          # (a NULL base struct comes first)
    bad = {
        "dropout": (dict(dropout_p=0.1), {}),
        "alibi_slopes": (dict(), dict(alibi_slopes=256)),
        "head dim 136": (dict(D=136), {}),
        "head dim 256": (dict(D=256), {}),
        "softmax_scale 0": (dict(softmax_scale=0.0), {}),
        "softmax_scale < 0": (dict(softmax_scale=-0.125), {}),
        # the zero-padded 128-wide windowed dK/dV instance with a cap is not built: forward and backward alike
        "a window at head dim 72": (dict(D=72, causal=1, window=1, window_left=16, window_right=-1), {}),
        "a two-sided window at head dim 120": (dict(D=120, window=1, window_left=16, window_right=8), {}),
    }
    for what, (akw, ekw) in bad.items():
        assert lib.rfa_fwd_ex(C.byref(_fwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_ARGS, f"fwd: {what}"
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_ARGS, f"bwd: {what}"
    fine = {
        "a causal window": (dict(causal=1, window=1, window_left=16, window_right=-1), {}),
        "a two-sided window": (dict(window=1, window_left=64, window_right=32), {}),
        "a window at head dim 128": (dict(D=128, causal=1, window=1, window_left=16, window_right=-1), {}),
        "a window at head dim 40": (dict(D=40, causal=1, window=1, window_left=16, window_right=-1), {}),
        "head dim 72 without a window": (dict(D=72, causal=1), {}),
        "head dim 72 with a window the normalisation drops": (dict(D=72, causal=1, window=1, window_left=500, window_right=-1), {}),
        "mask_shift inside the block": (dict(causal=1, window=1, window_left=100, window_right=-1, mask_shift=128), {}),
        "packed input with mask_shift_lens": (dict(cu_seqlens_q=cu, cu_seqlens_k=cu, causal=1, window=1, window_left=100,
                                                   window_right=-1, mask_shift_lens=1), {}),
        "halves": (dict(cu_seqlens_q=cu, cu_seqlens_k=cu, causal=1, q_half=2, k_half=1), {}),
        "a tiny cap": (dict(), dict(softcap=1e-30)),
        "alibi fields without slopes": (dict(), dict(alibi_shift=1 << 40, alibi_batch_stride=-4)),
    }
    for what, (akw, ekw) in fine.items():
        assert lib.rfa_fwd_ex(C.byref(_fwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_NULL, f"fwd: {what}"
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext(**ekw)), None) == ERR_NULL, f"bwd: {what}"
    # ALiBi and the cap are parsed independently: a bias alone keeps its own rules, softcap 0 beside it is off
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap=0.0, alibi_slopes=256)), None) == ERR_NULL
    assert lib.rfa_fwd_ex(C.byref(_fwd()), C.byref(_ext(softcap=0.0, alibi_slopes=256, alibi_batch_stride=-4)), None) == ERR_ARGS
    # forward forms that do not exist for a cap read as AUTO / never split
    for form in (_C.FWD_4x32, _C.FWD_P8x32):
        assert lib.rfa_fwd_ex(C.byref(_fwd(fwd_form=form, kv_nsplit=4)), C.byref(_ext()), None) == ERR_NULL
    # accumulate mode, two-phase backwards and RFA_BWD_KV_OVERWRITE combine with a cap (NULL tensors: ERR_NULL, not ERR_ARGS)
    assert lib.rfa_fwd_ex(C.byref(_fwd(out_acc=256)), C.byref(_ext()), None) == ERR_NULL
    for phases in (_C.BWD_COMPUTE, _C.BWD_REDUCE, 16):
        assert lib.rfa_bwd_ex(C.byref(_bwd(phases=phases)), C.byref(_ext()), None) == ERR_NULL, phases
    # the backward must already PLAN to the capped forms: the 128-key dK/dV kernel, no dS scratch
    for akw in (dict(dkdv_form=_C.DKDV_AUTO), dict(dkdv_form=_C.DKDV_256), dict(dkdv_form=_C.DKDV_BAL), dict(ds_scratch=256)):
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext()), None) == ERR_ARGS, akw
        assert lib.rfa_bwd_ex(C.byref(_bwd(**akw)), C.byref(_ext(softcap=0.0)), None) == ERR_NULL, akw   # (fine with the cap off)
    # a block whose band is empty runs as the call without the extension
    dark = dict(causal=1, mask_shift=-4096)
    assert lib.rfa_fwd_ex(C.byref(_fwd(**dark)), C.byref(_ext()), None) == ERR_NULL
    assert lib.rfa_bwd_ex(C.byref(_bwd(dkdv_form=_C.DKDV_AUTO, **dark)), C.byref(_ext()), None) == ERR_NULL


# ---------------------------------------------------------------------------------------------- backend
def test_backend_builds_one_struct_for_bias_and_cap():
    from ring_flash_attn import _C
    from ring_flash_attn.backend import HipBackend, _ext_args

    assert HipBackend.serves_softcap is True
    for fn in (HipBackend.fwd, HipBackend.bwd):
        assert inspect.signature(fn).parameters["softcap"].default == 0.0
    q = torch.zeros(2, 4, 4, 8)
    assert _ext_args(None, q) is None and _ext_args(None, q, 0.0) is None and _ext_args(None, q, None) is None
    e = _ext_args(None, q, 50.0)
    assert (e.struct_bytes, e.reserved, e.alibi_slopes, e.alibi_batch_stride, e.alibi_shift, e.softcap, e.softcap_pad) == \
        (C.sizeof(_C.ExtArgs), 0, None, 0, 0, 50.0, 0)
    s1 = torch.ones(4)
    e = _ext_args((s1, 260), q, 2.0)                               # (the library refuses the pair; the struct carries both)
    assert (e.alibi_slopes, e.alibi_shift, e.softcap) == (s1.data_ptr(), 260, 2.0)
    assert _ext_args((s1, 260), q).softcap == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _ext_args(None, q, bad)


# ---------------------------------------------------------------------------------------------- with_softcap
@pytest.fixture
def cpu_backend(single_rank_group):
    from ring_flash_attn import _testing
    from _ref_backend import RefBackend

    _testing.set_backend(RefBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
    yield
    _testing.set_backend(None)


def _qkv(S=48, D=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda h: torch.randn(2, S, h, D, generator=g).bfloat16()
    return mk(4), mk(2), mk(2), mk(4)


def test_with_softcap_validates_its_arguments_and_keeps_the_signatures():
    import ring_flash_attn as R

    assert "with_softcap" in dir(R)
    funcs = [getattr(R, n) for n in dir(R) if n.endswith("_func")]
    assert len(funcs) == 21
    before = {f.__name__: str(inspect.signature(f)) for f in funcs}
    for f in funcs:
        g = R.with_softcap(f, 50.0)
        assert g is not f and inspect.signature(g) == inspect.signature(f) and g.__name__ == f.__name__
        assert R.with_softcap(f, None) is f and R.with_softcap(f, 0) is f and R.with_softcap(f, 0.0) is f
    assert {f.__name__: str(inspect.signature(f)) for f in funcs} == before
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            R.with_softcap(R.ring_flash_attn_func, bad)
    for notf in (len, lambda q, k, v: q, R.llama3_flash_attn_prepare_cu_seqlens, R.substitute_hf_flash_attn,
                 R.with_softcap(R.ring_flash_attn_func, 2.0)):
        with pytest.raises(TypeError):
            R.with_softcap(notf, 2.0)


def test_with_softcap_caps_forward_and_backward_and_checkpointing_recomputes_with_the_cap(cpu_backend):
    import ring_flash_attn as R
    from torch.utils.checkpoint import checkpoint

    q, k, v, do = _qkv()
    cap = 2.0
    ref = SR.attention(q, k, v, softcap=cap, causal=True, dout=do)
    plain = SR.attention(q, k, v, causal=True, dout=do)
    assert (ref[0] - plain[0]).abs().max() > 0.05                  # the cap does something at this size
    capped = R.with_softcap(R.ring_flash_attn_func, cap)

    def run(fn, ckpt):
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        if ckpt:
            out = checkpoint(lambda a, b, c: fn(a, b, c, causal=True), *ins, use_reentrant=False)
        else:
            out = fn(*ins, causal=True)
        out.backward(do)                                           # (outside every wrapper: the node holds the value)
        return [out.detach()] + [t.grad for t in ins]

    got = run(capped, False)
    for nm, g_, r_, kd in zip(("out", "dq", "dk", "dv"), got, (ref[0],) + tuple(ref[2:]), ("out", "grad", "grad", "grad")):
        _tol.compare(f"with_softcap.{nm}", g_, r_, kd)
    again = run(capped, True)
    for a_, b_ in zip(got, again):
        assert torch.equal(a_, b_)                                  # the recomputation ran with the cap
    # None / 0: the function itself; an uncapped call after capped ones sees no cap
    base = run(R.ring_flash_attn_func, False)
    for nm, g_, r_, kd in zip(("out", "dq", "dk", "dv"), base, (plain[0],) + tuple(plain[2:]), ("out", "grad", "grad", "grad")):
        _tol.compare(f"uncapped.{nm}", g_, r_, kd)
    # a backward of a capped node that runs inside ANOTHER wrapper's call keeps its own value
    ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = capped(*ins, causal=True)
    from ring_flash_attn.backend import softcap_scope

    with softcap_scope(7.0):
        out.backward(do)
    for a_, b_ in zip(got[1:], [t.grad for t in ins]):
        assert torch.equal(a_, b_)


def test_refusals_at_the_public_entry(cpu_backend):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _ref_backend import RefBackend

    q, k, v, _ = _qkv()
    NI = NotImplementedError
    for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        capped = R.with_softcap(fn, 30.0)
        with pytest.raises(NI, match="dropout"):
            capped(q, k, v, causal=True, dropout_p=0.1)
        with pytest.raises(NI, match="alibi"):
            capped(q, k, v, causal=True, alibi_slopes=torch.ones(4))
    big = torch.zeros(1, 16, 2, 136, dtype=torch.bfloat16)
    with pytest.raises(NI, match="head dims up to 128"):
        R.with_softcap(R.ring_flash_attn_func, 30.0)(big, big, big, causal=True)
    d72 = torch.zeros(1, 16, 2, 72, dtype=torch.bfloat16)
    with pytest.raises(NI, match="sliding window"):
        R.with_softcap(R.ring_flash_attn_func, 30.0)(d72, d72, d72, causal=True, window_size=(4, 0))
    cu = torch.tensor([0, 20, 48], dtype=torch.int32)
    with pytest.raises(NI, match="dropout"):
        R.with_softcap(R.llama3_flash_attn_varlen_func, 30.0)(q[0], k[0], v[0], cu, cu, 28, 28, heads_k_stride=1,
                                                              local_k_slice=slice(0, 48), causal=True, dropout_p=0.1)
    with pytest.raises(NI, match="dropout"):
        R.with_softcap(R.zigzag_llama3_flash_attn_varlen_func, 30.0)(q[0], k[0], v[0], cu, causal=True, dropout_p=0.1)
    _testing.set_backend(RefBackend(serves=("mask_shift",)))                            # serves mask_shift, not softcap
    with pytest.raises(NI, match="serves `softcap`"):
        R.with_softcap(R.ring_flash_attn_func, 30.0)(q, k, v, causal=True)
    R.ring_flash_attn_func(q, k, v, causal=True)                   # (the same backend serves the uncapped call)


def test_hf_adapter_forwards_the_cap(cpu_backend):
    from ring_flash_attn import _testing
    from ring_flash_attn.adapters import hf_adapter
    from _ref_backend import Recording, RefBackend

    rec = Recording(RefBackend(serves=("mask_shift",)))
    _testing.set_backend(rec)
    S = 48
    hf_adapter.update_ring_flash_attn_params(torch.tensor([0, 20, S], dtype=torch.int32), None)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(1, S, 4, 32, generator=g).bfloat16().requires_grad_(True)
    k, v = (torch.randn(1, S, 2, 32, generator=g).bfloat16() for _ in range(2))
    kw = dict(dropout=0.0, softmax_scale=None, causal=True, sliding_window=16)
    hf_adapter._ring_attention(q, k, v, softcap=50.0, **kw).sum().backward()
    assert rec.seen["fwd"] and set(rec.seen["fwd"]) == {50.0} and rec.seen["bwd"] and set(rec.seen["bwd"]) == {50.0}
    rec.seen = {"fwd": [], "bwd": []}
    hf_adapter._ring_attention(q, k, v, softcap=None, **kw).sum().backward()
    assert rec.seen["fwd"] and set(rec.seen["fwd"]) == {None} and set(rec.seen["bwd"]) == {None}


# ---------------------------------------------------------------------------------------------- schedules under gloo
RECORD = [dict(kind=kd, W=2, S=32, causal=True, softcap=30.0, record=True, **extra) for kd, extra in (
    ("ring", {}), ("zigzag", dict(form="ring")), ("zigzag", dict(form="gather")), ("zigzag", dict(form="gather_ps")),
    ("stripe", {}), ("ring_varlen", dict(lens=[24, 40])), ("zigzag_varlen", dict(lens=[24, 40])),
    ("llama3", {}), ("zigzag_llama3", {}))] + [
    dict(kind="ring", W=2, S=32, causal=False, softcap=30.0, record=True),
    dict(kind="ring", W=2, S=32, causal=True, window=(20, 0), softcap=30.0, record=True),
    dict(kind="zigzag", W=2, S=32, causal=True, window=(20, 0), softcap=30.0, record=True, form="ring"),
]


def test_every_block_call_of_every_schedule_family_carries_the_cap():
    errs, _ = SW.run_world(2, RECORD, False, free_port())
    assert not errs, "\n".join(errs)


NUMERIC = {
    2: [dict(kind="ring", W=2, S=64, causal=True, softcap=2.0), dict(kind="ring", W=2, S=64, causal=False, softcap=2.0),
        dict(kind="zigzag", W=2, S=64, causal=True, softcap=2.0, form="gather"),
        dict(kind="zigzag", W=2, S=64, causal=True, softcap=2.0, form="ring"),
        dict(kind="llama3", W=2, S=64, causal=True, softcap=2.0),
        dict(kind="ring", W=2, S=64, causal=True, window=(40, 0), softcap=2.0)],
    4: [dict(kind="ring", W=4, S=64, causal=True, softcap=2.0), dict(kind="ring", W=4, S=64, causal=False, softcap=2.0)],
}


@pytest.mark.parametrize("W", [2, 4])
def test_schedules_match_one_single_device_capped_call(W):
    """S = 64 rows per rank, H 4 / Hk 2, D 64, softcap = 2.0 (tanh saturates: a dropped cap or a dropped 1 - t^2 is far
    outside the tolerance — checked on the reference itself below)"""
    c0 = NUMERIC[W][0]
    capped, plain = SW.reference(c0), SW.reference(c0, softcap=0.0)
    for i, kd in ((0, "out_ring"), (2, "grad_ring")):
        gap = (capped[i] - plain[i]).abs().max() / capped[i].abs().max()
        assert gap > 10 * _tol.KINDS[kd][1], (i, float(gap))
    errs, notes = SW.run_world(W, NUMERIC[W], False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)


def test_cap_tanh_formula_in_fp32_is_within_the_stated_error():
    """the kernels' tanh, 1 - 2 / (1 + exp2(2 log2(e) x)), evaluated in fp32 on the CPU against fp64: a few 2^-23 absolute,
    finite and exact at both ends"""
    x = torch.linspace(-12, 12, 200001, dtype=torch.float32)
    y = x * (2.0 * 1.4426950408889634)
    t = 1.0 - 2.0 / (1.0 + torch.exp2(y))
    err = (t.double() - torch.tanh(x.double())).abs().max().item()
    assert err <= 4 * 2.0 ** -23, err
    big = torch.tensor([1e4, -1e4, float("inf"), -float("inf")], dtype=torch.float32) * (2.0 * 1.4426950408889634)
    assert (1.0 - 2.0 / (1.0 + torch.exp2(big))).tolist() == [1.0, -1.0, 1.0, -1.0]
    assert math.isfinite(err)
