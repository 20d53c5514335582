"""`mask_shift_lens` (include/rfa.h ABI 8) on the host, no device: the launch plans of the packed cases that
tests/test_gpu_band_varlen.py runs — every (band, form) pair plans the form it names, never the balanced schedule, never
split-KV shares, COMPUTE and REDUCE phases alike — the argument checks of the pure size / plan functions, the dense fold
(`mask_shift_lens = n` plans what `mask_shift = n * len_k` plans), and the mix of lit / cut / dark sequences per band."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402
import test_gpu_band_varlen as T                 # noqa: E402  (the case lists and the host-side checks; nothing is launched)

ERR_ARGS = -8


def _lib():
    from ring_flash_attn import _C

    return _C, types.SimpleNamespace(lib=_C.load())


def _fake(causal, window, n, D, halves=False):
    """what the host-side checks read of a test context (pointers: any non-NULL value)"""
    mul = 2 if halves else 1
    x = types.SimpleNamespace(lens=T.LENS, D=D, band=dict(causal=causal, window=window, mask_shift_lens=n),
                              cu=torch.zeros(len(T.LENS) + 1, dtype=torch.int32), q=torch.zeros(mul * sum(T.LENS), 1),
                              vl=dict(max_seqlen_q=mul * max(T.LENS), max_seqlen_k=mul * max(T.LENS)))
    if halves:
        x.vl.update(q_half=2, k_half=2)
    return x


def test_abi_version_and_field():
    _C, be = _lib()
    assert _C.RFA_ABI_VERSION == 8 and be.lib.rfa_abi_version() == 8
    for st in (_C.FwdArgs, _C.BwdArgs):
        assert st._fields_[-1] == ("mask_shift_lens", C.c_int32)
    from ring_flash_attn.backend import HipBackend

    assert HipBackend.serves_mask_shift_lens is True


def test_mix_of_lit_cut_and_dark_sequences():
    for causal, window in T.WINDOWS.values():
        for n in T.SHIFTS:
            T.assert_mix(T.LENS, causal, window, n)
    assert T.seq_kinds(T.LENS, True, (130, 0), 2) == ["lit", "lit", "lit", "cut", "dark", "dark", "dark", "dark"]
    assert T.seq_kinds(T.LENS, True, (130, 0), 1) == ["lit"] * 4 + ["cut"] * 4
    for n in (1, -1):
        T.assert_mix(T.LENS, True, T.NOWIN, n)


def test_packed_shifted_calls_plan_the_form_they_name():
    _C, be = _lib()
    for causal, window in T.WINDOWS.values():
        for n in T.SHIFTS:
            for D in T.WIN_DIMS:
                for halves in (False, True):
                    x = _fake(causal, window, n, D, halves)
                    T.check_fwd_plan(be, x, T.BF)
                    for phases in (0, 1, 2):
                        T.check_bwd_plan(be, x, T.BF, "windowed", phases=phases)
    for n in (1, -1):
        for D in (128, 64):
            x = _fake(True, T.NOWIN, n, D)
            T.check_fwd_plan(be, x, T.BF)
            for form in T.CAUSAL_FORMS + ("7gemm",):
                if form == "5gemm" and D == 64:
                    continue
                plans = set()
                for phases in (0, 1, 2):
                    T.check_bwd_plan(be, x, T.BF, form, phases=phases)
                    a = T._packed_bwd_args(_C, x, 0, BR.BWD_FORMS[form][0], acc=True, phases=phases)
                    plans.add((BR.bwd_plan(be.lib, a)[:2], be.lib.rfa_bwd_workspace_bytes(C.byref(a))))
                assert len({p[0] for p in plans}) == 1, (form, n, D, plans)     # COMPUTE and REDUCE agree with each other


def test_causal_packed_shift_keeps_the_ds_hand_off_and_declines_nothing_else():
    """a causal packed call with a shift and no window: the packed-row dS scratch has the size of the unshifted call's (its
    layout is rectangular per row) and the call is 5-GEMM; a bounded window is not eligible, as before"""
    _C, be = _lib()
    sizes = []
    for n in (0, 1, -1):
        a = T._packed_bwd_args(_C, _fake(True, T.NOWIN, n, 128), 0)
        sizes.append(be.lib.rfa_bwd_ds_scratch_bytes(C.byref(a)))
        assert BR.bwd_plan(be.lib, a)[2] == 1
    assert sizes[0] > 0 and sizes[0] == sizes[1] == sizes[2]
    a = T._packed_bwd_args(_C, _fake(True, (130, 0), 1, 128), 0)
    assert be.lib.rfa_bwd_ds_scratch_bytes(C.byref(a)) == 0 and BR.bwd_plan(be.lib, a)[2] == 0


def test_argument_checks_of_the_pure_functions():
    _C, be = _lib()
    f, n_, five = C.c_int32(), C.c_int32(), C.c_int32()
    plan = lambda a: be.lib.rfa_bwd_plan(C.byref(a), C.byref(f), C.byref(n_), C.byref(five))
    x = _fake(True, T.NOWIN, 1, 128)
    ok = T._packed_bwd_args(_C, x, 0)
    assert plan(ok) == 0
    a = T._packed_bwd_args(_C, x, 0)
    a.dropout_p = 0.1                                                     # packed + mask_shift_lens + dropout
    assert plan(a) == ERR_ARGS and be.lib.rfa_bwd_workspace_bytes(C.byref(a)) == 0
    a = T._packed_bwd_args(_C, x, 0)
    a.mask_shift = 4                                                      # packed + the absolute shift: as before
    assert plan(a) == ERR_ARGS
    big = (1 << 30) // max(T.LENS)
    for lens, want in ((big, 0), (big + 1, ERR_ARGS), (-big, 0), (-big - 1, ERR_ARGS)):
        a = T._packed_bwd_args(_C, x, 0)
        a.mask_shift_lens = lens                                          # |mask_shift_lens| * Sk at or beyond 2^30
        assert plan(a) == want, lens
    # dense input: the same range rule
    g = BR.Geometry("d", "d", 256, 256, True, T.NOWIN, 0, 1, None)
    for lens, want in (((1 << 22) - 1, 0), (1 << 22, ERR_ARGS)):
        a = BR.bwd_args(_C, g, T.H, T.HK, 128)
        a.mask_shift_lens = lens
        assert plan(a) == want, lens


@pytest.mark.parametrize("name", ["causal+33", "causal-333", "wl130+65", "two-sided-333", "corner-hi", "hi-dropped"])
def test_dense_fold_plans_what_the_absolute_shift_plans(name):
    """mask_shift_lens * len_k is folded into mask_shift before norm_band: same plan, workspace and scratch sizes"""
    _C, be = _lib()
    g = BR.BY_NAME[name]
    for n in (1, -1, 2):
        for acc in (False, True):
            a, b = BR.bwd_args(_C, g, T.H, T.HK, 128, acc=acc), BR.bwd_args(_C, g, T.H, T.HK, 128, acc=acc)
            a.mask_shift, a.mask_shift_lens = g.shift, n
            b.mask_shift = g.shift + n * g.lk
            assert BR.bwd_plan(be.lib, a) == BR.bwd_plan(be.lib, b)
            assert be.lib.rfa_bwd_workspace_bytes(C.byref(a)) == be.lib.rfa_bwd_workspace_bytes(C.byref(b))
            assert be.lib.rfa_bwd_ds_scratch_bytes(C.byref(a)) == be.lib.rfa_bwd_ds_scratch_bytes(C.byref(b))
            fa, fb = BR.fwd_args(_C, g, T.H, T.HK, 128, acc=acc), BR.fwd_args(_C, g, T.H, T.HK, 128, acc=acc)
            fa.mask_shift, fa.mask_shift_lens = g.shift, n
            fb.mask_shift = g.shift + n * g.lk
            assert BR.fwd_shares(be.lib, fa) == BR.fwd_shares(be.lib, fb)
