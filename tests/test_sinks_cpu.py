"""Attention sinks (ring_flash_attn.with_sinks) without a GPU: the two new C-ABI entry points' structs and argument checks,
the public wrapper's refusals, and every schedule family under gloo on the CPU test backend (tests/_sink_backend.py) against
ONE single-device call of the fp64 reference that appends the sink column (tests/_sinkref.py)."""
import ctypes as C
import inspect
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import free_port                   # noqa: E402
import _sinkref as SK                            # noqa: E402
import _sinks_worker as KW                       # noqa: E402
import _tol                                      # noqa: E402


# ---------------------------------------------------------------------------------------------- C ABI
def test_sink_structs_match_the_c_layout_and_the_abi_numbers_stay(built):
    from ring_flash_attn import _C

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rfa.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(rfa_sink_apply_args), sizeof(rfa_sink_grad_args), sizeof(rfa_ext_args));
  printf("%zu %zu %zu %zu\n", offsetof(rfa_sink_apply_args, lse_dst), offsetof(rfa_sink_apply_args, dtype),
         offsetof(rfa_sink_grad_args, dsink), offsetof(rfa_sink_grad_args, workspace_bytes));
  printf("%d %d\n", RFA_ABI_VERSION, RFA_ABI_REVISION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [C.sizeof(_C.SinkApplyArgs), C.sizeof(_C.SinkGradArgs), 40]
    assert out[3:7] == [_C.SinkApplyArgs.lse_dst.offset, _C.SinkApplyArgs.dtype.offset, _C.SinkGradArgs.dsink.offset,
                        _C.SinkGradArgs.workspace_bytes.offset]
    assert out[7:] == [8, 1]
    lib = _C.load()
    assert lib.rfa_ext_args_bytes() == 40 == C.sizeof(_C.ExtArgs)
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1
    for name in ("rfa_sink_apply", "rfa_sink_grad", "rfa_sink_grad_workspace_bytes"):
        assert name in _C.SYMBOLS and hasattr(lib, name)


def _apply_args(**kw):
    from ring_flash_attn import _C

    a = _C.SinkApplyArgs()
    a.B, a.S, a.H, a.D, a.dtype = 2, 16, 4, 64, 0
    st = _C.Strides(16 * 4 * 64, 4 * 64, 64)
    a.out_src_st, a.out_dst_st = st, st
    a.lse_src_batch, a.lse_src_head, a.lse_dst_batch, a.lse_dst_head = 64, 16, 64, 16
    a.out_src = a.out_dst = a.lse_src = a.lse_dst = a.sinks = 4096            # never dereferenced: every case below is refused
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grad_args(**kw):
    from ring_flash_attn import _C

    a = _C.SinkGradArgs()
    a.B, a.S, a.H, a.D, a.dtype = 2, 16, 4, 64, 0
    st = _C.Strides(16 * 4 * 64, 4 * 64, 64)
    a.dout_st, a.out_st = st, st
    a.lse_batch, a.lse_head = 64, 16
    a.dout = a.out = a.lse = a.sinks = a.dsink = a.workspace = 4096
    a.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_sink_argument_errors_without_a_device(built):
    from ring_flash_attn import _C

    lib = _C.load()
    NULL, DTYPE, HEAD_DIM, HEADS, SHAPE, ALIGN, ARGS = -1, -2, -3, -4, -5, -6, -8
    odd = _C.Strides(16 * 4 * 64, 4 * 64 + 4, 64)
    for fn, mk, tensors, strided in (
            (lib.rfa_sink_apply, _apply_args, ("out_src", "out_dst", "lse_src", "lse_dst", "sinks"), ("out_src_st", "out_dst_st")),
            (lib.rfa_sink_grad, _grad_args, ("dout", "out", "lse", "sinks", "dsink", "workspace"), ("dout_st", "out_st"))):
        assert fn(None, None) == NULL
        for t in tensors:
            assert fn(C.byref(mk(**{t: None})), None) == NULL, t
        for D in (0, 4, 12, 264, -8):
            assert fn(C.byref(mk(D=D)), None) == HEAD_DIM, D
        assert fn(C.byref(mk(dtype=2)), None) == DTYPE and fn(C.byref(mk(dtype=-1)), None) == DTYPE
        assert fn(C.byref(mk(H=0)), None) == HEADS
        assert fn(C.byref(mk(S=-1)), None) == SHAPE and fn(C.byref(mk(B=-1)), None) == SHAPE
        assert fn(C.byref(mk(H=70000)), None) == SHAPE and fn(C.byref(mk(B=70000)), None) == SHAPE
        assert fn(C.byref(mk(reserved=1)), None) == ARGS
        for t in tensors:
            if t.startswith("lse") or t in ("sinks", "dsink"):
                continue
            assert fn(C.byref(mk(**{t: 4096 + 8})), None) == ALIGN, t
        for st in strided:
            assert fn(C.byref(mk(**{st: odd})), None) == ALIGN, st
        # the dtype and the head dim are looked at before the pointers, the pointers before their alignment
        assert fn(C.byref(mk(dtype=5, D=12, **{tensors[0]: None})), None) == DTYPE
        assert fn(C.byref(mk(D=12, **{tensors[0]: None})), None) == HEAD_DIM
        assert fn(C.byref(mk(**{tensors[0]: None, tensors[1]: 4096 + 8})), None) == NULL
    # zero rows: RFA_OK with nothing launched, whatever the tensors
    for kw in (dict(B=0), dict(S=0)):
        assert lib.rfa_sink_apply(C.byref(_apply_args(out_src=None, lse_dst=None, **kw)), None) == 0
        assert lib.rfa_sink_grad(C.byref(_grad_args(dsink=None, **kw)), None) == NULL      # (dsink is zeroed even then)
        assert lib.rfa_sink_grad_workspace_bytes(C.byref(_grad_args(**kw))) == 0
    # the workspace: one fp32 partial per (batch entry, chunk of 256 rows, head); too small a one is refused
    ws = lib.rfa_sink_grad_workspace_bytes
    assert ws(None) == 0 and ws(C.byref(_grad_args(D=12))) == 0
    assert ws(C.byref(_grad_args())) == 2 * 1 * 4 * 4
    assert ws(C.byref(_grad_args(B=1, S=257, H=5))) == 2 * 5 * 4 and ws(C.byref(_grad_args(B=1, S=256, H=5))) == 5 * 4
    assert ws(C.byref(_grad_args(B=1, S=8192, H=64))) == 32 * 64 * 4
    assert lib.rfa_sink_grad(C.byref(_grad_args(workspace_bytes=31)), None) == ARGS


# ---------------------------------------------------------------------------------------------- with_sinks
@pytest.fixture
def cpu_backend(single_rank_group):
    from ring_flash_attn import _testing
    from _sink_backend import SinkBackend

    _testing.set_backend(SinkBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
    yield
    _testing.set_backend(None)


B, S, H, HK, D = 2, 48, 4, 2, 32


def _qkv(seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).bfloat16()
    return mk(H), mk(HK), mk(HK), mk(H)


def _sinks_near(lse, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (lse[torch.isfinite(lse)].mean() + 4 * torch.rand(H, generator=g, dtype=torch.float64) - 2).float()


def test_with_sinks_validates_its_arguments_and_keeps_the_signatures(cpu_backend):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _ref_backend import RefBackend

    assert "with_sinks" in dir(R)
    funcs = [getattr(R, n) for n in dir(R) if n.endswith("_func")]
    assert len(funcs) == 21
    before = {f.__name__: str(inspect.signature(f)) for f in funcs}
    sinks = torch.zeros(H)
    for f in funcs:
        g = R.with_sinks(f, sinks)
        assert g is not f and inspect.signature(g) == inspect.signature(f) and g.__name__ == f.__name__
        assert R.with_sinks(f, None) is f
    assert {f.__name__: str(inspect.signature(f)) for f in funcs} == before
    for bad in (torch.zeros(H, dtype=torch.int32), torch.zeros(2, H), torch.zeros(()), 1.0, [0.0] * H):
        with pytest.raises(ValueError, match="sinks"):
            R.with_sinks(R.ring_flash_attn_func, bad)
    for notf in (len, lambda q, k, v: q, R.llama3_flash_attn_prepare_cu_seqlens, R.substitute_hf_flash_attn,
                 R.with_sinks(R.ring_flash_attn_func, sinks)):
        with pytest.raises(TypeError):
            R.with_sinks(notf, sinks)
    with pytest.raises(TypeError, match="with_softcap"):               # the composition is refused, with its reason
        R.with_sinks(R.with_softcap(R.ring_flash_attn_func, 30.0), sinks)
    with pytest.raises(TypeError):
        R.with_softcap(R.with_sinks(R.ring_flash_attn_func, sinks), 30.0)
    # at the call: the head count and the device are q's
    q, k, v, _ = _qkv()
    cu = torch.tensor([0, 20, S], dtype=torch.int32)
    for bad in (torch.zeros(H + 1), torch.zeros(HK), torch.zeros(H, device="meta")):
        with pytest.raises(ValueError, match="sinks"):
            R.with_sinks(R.ring_flash_attn_func, bad)(q, k, v, causal=True)
        with pytest.raises(ValueError, match="sinks"):
            R.with_sinks(R.ring_flash_attn_qkvpacked_func, bad)(torch.stack([q, q, q], dim=2), causal=True)
        with pytest.raises(ValueError, match="sinks"):
            R.with_sinks(R.llama3_flash_attn_varlen_func, bad)(q[0], k[0], v[0], cu, cu, 28, 28, heads_k_stride=1,
                                                               local_k_slice=slice(0, S), causal=True)
        with pytest.raises(ValueError, match="sinks"):
            R.with_sinks(R.zigzag_llama3_flash_attn_varlen_func, bad)(q[0], k[0], v[0], cu, causal=True)
    # a backend that does not serve sinks: refused at the public entry; the same backend serves the plain call
    _testing.set_backend(RefBackend(serves=("mask_shift",)))
    for fn, args in ((R.ring_flash_attn_func, (q, k, v)), (R.zigzag_llama3_flash_attn_varlen_func, (q[0], k[0], v[0], cu)),
                     (R.llama3_flash_attn_varlen_func, (q[0], k[0], v[0], cu, cu, 28, 28, 1, slice(0, S)))):
        with pytest.raises(NotImplementedError, match="sinks"):
            R.with_sinks(fn, sinks)(*args, causal=True)
    R.ring_flash_attn_func(q, k, v, causal=True)


def _run(fn, tensors, do, sinks=None, ckpt=False, **kw):
    from torch.utils.checkpoint import checkpoint

    ins = [t.clone().requires_grad_(True) for t in tensors]
    if sinks is not None:
        sinks.grad = None
    if ckpt:
        out = checkpoint(lambda *a: fn(*a, **kw), *ins, use_reentrant=False)
    else:
        out = fn(*ins, **kw)
    out.backward(do)                                                 # (outside every wrapper: the node holds the tensor)
    return [out.detach()] + [t.grad for t in ins] + ([] if sinks is None else [sinks.grad.clone()])


def test_with_sinks_forward_backward_checkpointing_and_packed_forms(cpu_backend):
    import ring_flash_attn as R

    q, k, v, do = _qkv()
    plain = SK.attention(q, k, v, None, causal=True, dout=do)
    sinks = _sinks_near(plain[1]).requires_grad_(True)
    ref = SK.attention(q, k, v, sinks, causal=True, dout=do)
    kinds = ("out", "grad", "grad", "grad", "grad")
    want = (ref[0],) + tuple(ref[2:])
    fn = R.with_sinks(R.ring_flash_attn_func, sinks)
    got = _run(fn, (q, k, v), do, sinks, causal=True)
    for nm, g_, r_, kd in zip(("out", "dq", "dk", "dv", "dsink"), got, want, kinds):
        _tol.compare(f"with_sinks.{nm}", g_, r_, kd)
    out, lse, none = fn(q, k, v, causal=True, return_attn_probs=True)
    assert none is None and torch.equal(out, got[0])
    _tol.compare("with_sinks.lse", lse, ref[1], "lse")               # return_attn_probs yields lse'
    # activation checkpointing re-runs the wrapped call and binds the tensor again: the same bits, sinks.grad included
    again = _run(fn, (q, k, v), do, sinks, ckpt=True, causal=True)
    for a_, b_ in zip(got, again):
        assert torch.equal(a_, b_)
    # a plain call after calls with sinks sees none
    base = _run(R.ring_flash_attn_func, (q, k, v), do, causal=True)
    for nm, g_, r_, kd in zip(("out", "dq", "dk", "dv"), base, (plain[0],) + tuple(plain[2:5]), kinds):
        _tol.compare(f"plain.{nm}", g_, r_, kd)
    # the packed forms: the gradients land in one packed buffer, the sinks' beside it
    kv, qkv = torch.stack([k, v], dim=2), torch.stack([q, k.repeat_interleave(2, dim=2), v.repeat_interleave(2, dim=2)], dim=2)
    g_kv = _run(R.with_sinks(R.ring_flash_attn_kvpacked_func, sinks), (q, kv), do, sinks, causal=True)
    assert torch.equal(g_kv[0], got[0]) and torch.equal(g_kv[1], got[1]) and torch.equal(g_kv[3], got[4])
    assert torch.equal(g_kv[2][:, :, 0], got[2]) and torch.equal(g_kv[2][:, :, 1], got[3])
    ref3 = SK.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], sinks, causal=True, dout=do)
    g_qkv = _run(R.with_sinks(R.ring_flash_attn_qkvpacked_func, sinks), (qkv,), do, sinks, causal=True)
    for i, nm in enumerate(("dq", "dk", "dv")):
        _tol.compare(f"qkvpacked.{nm}", g_qkv[1][:, :, i], ref3[2 + i], "grad")
    _tol.compare("qkvpacked.dsink", g_qkv[2], ref3[5], "grad")
    # the gradient comes in sinks' dtype; a sinks that needs none gets none
    half = sinks.detach().bfloat16().requires_grad_(True)
    g_h = _run(R.with_sinks(R.ring_flash_attn_func, half), (q, k, v), do, half, causal=True)
    assert g_h[4].dtype == torch.bfloat16
    frozen = sinks.detach()
    out = R.with_sinks(R.ring_flash_attn_func, frozen)(q.clone().requires_grad_(True), k, v, causal=True)
    out.backward(do)
    assert frozen.grad is None and torch.equal(out, got[0])


@pytest.mark.parametrize("family", ["ring", "varlen", "llama3", "zigzag_llama3"])
def test_a_sink_of_minus_1e4_is_the_plain_call_bit_for_bit(cpu_backend, family):
    import ring_flash_attn as R

    q, k, v, do = _qkv()
    cu = torch.tensor([0, 20, S], dtype=torch.int32)
    fn, tensors, do_, args = {
        "ring": (R.ring_flash_attn_func, (q, k, v), do, ()),
        "varlen": (R.ring_flash_attn_varlen_func, (q[0], k[0], v[0]), do[0], (cu, 28)),
        "llama3": (R.llama3_flash_attn_varlen_func, (q[0], k[0], v[0]), do[0], (cu, cu, 28, 28, 1, slice(0, S))),
        "zigzag_llama3": (R.zigzag_llama3_flash_attn_varlen_func, (q[0], k[0], v[0]), do[0], (cu,)),
    }[family]
    low = torch.full((H,), -1e4, requires_grad=True)
    a = _run(lambda *t, **kw: R.with_sinks(fn, low)(*t, *args, **kw), tensors, do_, low, causal=True, window_size=(16, 0))
    b = _run(lambda *t, **kw: fn(*t, *args, **kw), tensors, do_, causal=True, window_size=(16, 0))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[4], torch.zeros(H))                         # dsink is exactly 0


def test_hf_adapter_binds_s_aux(cpu_backend):
    import ring_flash_attn as R
    from ring_flash_attn.adapters import hf_adapter

    hf_adapter.update_ring_flash_attn_params(torch.tensor([0, 20, S], dtype=torch.int32), None)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(1, S, H, D, generator=g).bfloat16().requires_grad_(True)
    k, v = (torch.randn(1, S, HK, D, generator=g).bfloat16() for _ in range(2))
    kw = dict(dropout=0.0, softmax_scale=None, causal=True, sliding_window=16)
    cu = [0, 20, S]
    plain = SK.attention(q[0], k[0], v[0], None, causal=True, window=(16, 0), cu_seqlens_q=cu, cu_seqlens_k=cu)
    s_aux = _sinks_near(plain[1]).requires_grad_(True)
    do = torch.randn(1, S, H, D, generator=g).bfloat16()
    ref = SK.attention(q[0], k[0], v[0], s_aux, causal=True, window=(16, 0), cu_seqlens_q=cu, cu_seqlens_k=cu, dout=do[0])
    out = hf_adapter._ring_attention(q, k, v, s_aux=s_aux, **kw)
    out.backward(do)
    _tol.compare("hf.out", out[0], ref[0], "out")
    _tol.compare("hf.dq", q.grad[0], ref[2], "grad")
    _tol.compare("hf.dsink", s_aux.grad, ref[5], "grad")
    assert (ref[0] - plain[0]).abs().max() > 10 * _tol.KINDS["out"][1] * ref[0].abs().max()
    none = hf_adapter._ring_attention(q, k, v, s_aux=None, **kw)
    _tol.compare("hf.plain", none[0], plain[0], "out")
    assert "s_aux" in inspect.signature(hf_adapter.ring_flash_attention_forward).parameters


# ---------------------------------------------------------------------------------------------- schedules under gloo
def _cases(W):
    c = [dict(kind=kd, W=W, S=32, causal=True, **extra) for kd, extra in (
        ("ring", {}), ("zigzag", dict(form="ring")), ("zigzag", dict(form="gather")), ("stripe", {}),
        ("ring_varlen", dict(lens=[24, 40])), ("zigzag_varlen", dict(lens=[24, 40])),      # packed, different lengths
        ("llama3", {}), ("zigzag_llama3", {}))]
    c.append(dict(kind="ring", W=W, S=32, causal=True, window=(20, 0)))                  # a window below the per-rank length
    c.append(dict(kind="ring", W=W, S=32, causal=False))
    return c


def test_the_sinks_of_the_schedule_tests_discriminate():
    """on the reference alone: with the sinks the tests draw (around the mean lse, +- 2) the sink column holds a real share of
    the softmax, and out and dq differ from the attention without sinks by far more than the comparisons allow"""
    for c in (_cases(2)[0], _cases(4)[4], _cases(2)[8]):
        sinks = KW.draw_sinks(c)
        with_, without = KW.reference(c, sinks), KW.reference(c, None)
        for i, kd in ((0, "out_ring"), (2, "grad_ring")):
            gap = (with_[i] - without[i]).abs().max() / with_[i].abs().max()
            assert gap > 10 * _tol.KINDS[kd][1], (KW.case_name(c), i, float(gap))
        share = (1 - torch.exp(without[1] - with_[1])).mean()                             # mean probability of the sink column
        assert 0.2 <= share <= 0.8, (KW.case_name(c), float(share))
        assert with_[5].abs().min() > 0


@pytest.mark.parametrize("W", [1, 2, 4])
def test_schedules_match_one_single_device_call_with_the_sink_column(W):
    """S = 32 rows per rank, H 4 / Hk 2, D 64: every family's un-sharded out, lse, dq, dk, dv and the SUM of the ranks' dsink
    against one fp64 call over the full sequence"""
    errs, notes = KW.run_world(W, _cases(W), False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)


def test_dsink_tolerance_is_four_times_the_fp32_formula_error():
    """DSINK_TOL (tests/_sinkref.py) comes from the plain fp32 torch evaluation of the formula, never from a kernel: measure
    that evaluation against fp64 over the kernel-alone cases again"""
    worst = 0.0
    for Dh in SK.KERNEL_D:
        for bsh in SK.KERNEL_BSH:
            for dt in (torch.bfloat16, torch.float16):
                for packed in (False, True):
                    for seed in range(3):
                        do, o, l, s = SK.kernel_inputs(*bsh, Dh, dt, packed, seed)
                        o2, l2 = SK.apply_formula(o, l, s)
                        o2, l2 = o2.to(dt), l2.float()
                        r, n = SK.dsink_formula(do, o2, l2, s)
                        f, _ = SK.dsink_formula(do, o2, l2, s, torch.float32)
                        worst = max(worst, ((f.double() - r).abs() / n.clamp_min(1e-300)).max().item())
    print(f"fp32 formula against fp64, worst error / sum|terms|: {worst:.3e} (recorded {SK.DSINK_FP32_WORST:.3e})")
    assert SK.DSINK_TOL == 4 * SK.DSINK_FP32_WORST and 0 < worst <= SK.DSINK_TOL
