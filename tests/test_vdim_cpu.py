"""A value head dim of its own (MLA: QK head dim 192, V head dim 128) without a GPU: the C ABI of rfa_fwd_vd / rfa_bwd_vd, the
backend's routing, the five ring-type schedules under gloo on a CPU backend with `serves_vdim` (tests/_vdim_backend.py)
against ONE single-device fp64 autograd attention, every refusal of the public entry, and the register audit of
csrc/rfa_vdim.hip."""
import ctypes as C
import os
import re
import shutil
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
import _vdim_worker as VW                        # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays(built):
    from ring_flash_attn import _C

    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert "int rfa_fwd_vd(const rfa_fwd_args *args, const rfa_vdim_args *vd, void *stream);" in header
    assert "int rfa_bwd_vd(const rfa_bwd_args *args, const rfa_vdim_args *vd, void *stream);" in header
    for sym in ("rfa_fwd_vd", "rfa_bwd_vd"):
        assert sym in names and sym in _C.SYMBOLS
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)


def test_struct_matches_the_c_layout(built):
    from ring_flash_attn import _C

    fields = [n for n, _ in _C.VdimArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu\\n", sizeof(rfa_vdim_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_vdim_args, {n}));\n' for n in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _C.VdimArgs
    assert got[0] == C.sizeof(A) == 16
    assert got[1:] == [getattr(A, n).offset for n in fields] == [0, 4, 8, 12]
    assert A().struct_bytes == 16


def _base(cls, **kw):
    a = cls()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.softmax_scale = 2, 300, 300, 4, 2, 192, 0, 0.07
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def _vd(**kw):
    from ring_flash_attn import _C

    v = _C.VdimArgs()
    v.head_dim_v = 128
    for n, x in kw.items():
        setattr(v, n, x)
    return v


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_every_argument_check_with_null_tensors_in_the_stated_order(built, which):
    """every tensor pointer is NULL: nothing is read, nothing is launched, no device is needed"""
    from ring_flash_attn import _C

    lib = _C.load()
    fn, cls = (lib.rfa_fwd_vd, _C.FwdArgs) if which == "fwd" else (lib.rfa_bwd_vd, _C.BwdArgs)
    run = lambda a, v: fn(C.byref(a), None if v is None else C.byref(v), None)
    assert fn(None, C.byref(_vd()), None) == ERR_NULL
    # the extension's own checks, each alone
    assert run(_base(cls), None) == ERR_ARGS
    for kw, want in [(dict(struct_bytes=8), ERR_ARGS), (dict(struct_bytes=15), ERR_ARGS), (dict(reserved=1), ERR_ARGS),
                     (dict(pad=1), ERR_ARGS),
                     (dict(head_dim_v=0), ERR_HEAD_DIM), (dict(head_dim_v=-8), ERR_HEAD_DIM), (dict(head_dim_v=4), ERR_HEAD_DIM),
                     (dict(head_dim_v=68), ERR_HEAD_DIM), (dict(head_dim_v=136), ERR_HEAD_DIM), (dict(head_dim_v=192), ERR_HEAD_DIM)]:
        assert run(_base(cls), _vd(**kw)) == want, kw
    assert run(_base(cls, dropout_p=0.1), _vd()) == ERR_ARGS
    for D in (0, 64, 128, 132, 140, 200, 256):
        assert run(_base(cls, D=D), _vd()) == ERR_HEAD_DIM, D
    # a longer struct whose unknown tail is zero is accepted, one with a non-zero tail is not
    class Longer(C.Structure):
        _fields_ = [("v", _C.VdimArgs), ("tail", C.c_int32 * 2)]

    lo = Longer()
    lo.v = _vd(struct_bytes=24)
    as_vd = lambda: C.cast(C.pointer(lo), C.POINTER(_C.VdimArgs))
    assert fn(C.byref(_base(cls)), as_vd(), None) == ERR_NULL          # through to the base call's NULL tensors
    lo.tail[1] = 1
    assert fn(C.byref(_base(cls)), as_vd(), None) == ERR_ARGS
    # the order inside the extension: struct, reserved / pad and dropout (ARGS) in front of the two head dims (HEAD_DIM),
    # all of them in front of every base check
    assert run(_base(cls, D=64, dtype=7), _vd(reserved=1, head_dim_v=4)) == ERR_ARGS
    assert run(_base(cls, D=64, dtype=7, dropout_p=0.5), _vd(head_dim_v=4)) == ERR_ARGS
    assert run(_base(cls, D=64, dtype=7), _vd(head_dim_v=4)) == ERR_HEAD_DIM
    assert run(_base(cls, D=64, dtype=7), _vd()) == ERR_HEAD_DIM
    # then the base call's checks in their existing order
    chain = [(dict(dtype=7), ERR_DTYPE), (dict(Hk=3), ERR_HEADS), (dict(B=-1), ERR_SHAPE), (dict(Sq=-1), ERR_SHAPE)]
    for i, (_, want) in enumerate(chain):
        kw = {}
        for later, _w in chain[i:]:
            kw.update(later)
        assert run(_base(cls, **kw), _vd()) == want, (i, kw)
    assert run(_base(cls, B=0), _vd()) == OK                           # nothing to do
    assert run(_base(cls), _vd()) == ERR_NULL                          # q, k, v ...
    for Dv in range(8, 129, 8):
        for D in range(136, 193, 8):
            assert run(_base(cls, D=D), _vd(head_dim_v=Dv)) == ERR_NULL, (D, Dv)
    # the base entry points answer as before
    base_fn = lib.rfa_fwd if which == "fwd" else lib.rfa_bwd
    assert base_fn(C.byref(_base(cls)), None) == ERR_NULL and base_fn(C.byref(_base(cls, D=260)), None) == ERR_HEAD_DIM
    if which == "bwd":
        # the base arguments' own plan and sizes describe the call: a 128-wide dV fits the 192-wide slots of the workspace
        a = _base(cls, phases=1, total_k=600)
        assert lib.rfa_bwd_workspace_bytes(C.byref(a)) >= 2 * 600 * 2 * 192 * 2


# ---------------------------------------------------------------------------------------------- routing
class _RecLib:
    """the loaded library with a note of every function called through it; nothing is launched (no device here)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if name in ("rfa_fwd", "rfa_fwd_ex", "rfa_fwd_vd", "rfa_bwd", "rfa_bwd_ex", "rfa_bwd_vd", "rfa_bwd_preprocess"):
            def noted(*a):
                self.calls.append((name, a))
                return 0
            return noted
        return real


@pytest.fixture
def rec_backend(built, monkeypatch):
    from ring_flash_attn import backend

    be = backend.HipBackend()
    be.lib = _RecLib(be.lib)
    monkeypatch.setattr(backend.HipBackend, "_check_dev", staticmethod(lambda *ts: None))
    monkeypatch.setattr(backend, "_stream", lambda t: None)
    monkeypatch.setattr(backend, "_spill_enabled", lambda: False)
    return be


def _tensors(D, Dv, S=64):
    mk = lambda h, d: torch.zeros(1, S, h, d, dtype=torch.bfloat16)
    return mk(4, D), mk(2, D), mk(2, Dv)


@pytest.mark.parametrize("D", [64, 128, 136, 192, 256])
def test_equal_widths_never_reach_the_new_functions(rec_backend, D):
    be = rec_backend
    assert be.serves_vdim is True
    q, k, v = _tensors(D, D)
    out, lse = torch.empty_like(q), torch.empty(1, 4, 64)
    be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=True, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v))
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd", "rfa_bwd"]
    # ... with the arguments such a call always had: D from q, v's own strides, no third argument
    for _, args in be.lib.calls:
        assert len(args) == 2 and args[0]._obj.D == D and (args[0]._obj.v_st.row, args[0]._obj.v_st.head) == (2 * D, D)


def test_differing_widths_reach_the_new_pair_with_the_value_head_dim(rec_backend):
    from ring_flash_attn import _C

    be = rec_backend
    q, k, v = _tensors(192, 128)
    out, lse = torch.empty(1, 64, 4, 128, dtype=torch.bfloat16), torch.empty(1, 4, 64)
    be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=True, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v))
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd_vd", "rfa_bwd_vd"]
    for _, (a, vd, _s) in be.lib.calls:
        assert a._obj.D == 192 and vd._obj.head_dim_v == 128 and vd._obj.struct_bytes == C.sizeof(_C.VdimArgs)
        assert (a._obj.v_st.row, a._obj.v_st.head) == (2 * 128, 128)
    fa, ba = be.lib.calls[0][1][0]._obj, be.lib.calls[1][1][0]._obj
    assert (fa.out_st.row, fa.out_st.head) == (4 * 128, 128) and (ba.dout_st.row, ba.dv_st.row, ba.dk_st.row) == (512, 256, 384)
    # what the kernels of such a call do not have is refused before the library is called
    n = len(be.lib.calls)
    slopes = torch.ones(4)
    for kw in (dict(alibi=(slopes, 0)), dict(softcap=30.0), dict(dropout=(0.1, 1, 0, 0, 0))):
        with pytest.raises(NotImplementedError):
            be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse, **kw)
        with pytest.raises(NotImplementedError):
            be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=True, dq=torch.empty_like(q),
                   dk=torch.empty_like(k), dv=torch.empty_like(v), **kw)
    assert len(be.lib.calls) == n


# ---------------------------------------------------------------------------------------------- schedules
PAIRS = ((192, 128), (136, 72))


def _schedule_cases(W):
    S = 16
    lens = [8 * W, 4 * W]
    cs = []
    for i, (D, Dv) in enumerate(PAIRS):
        base = dict(W=W, S=S, D=D, Dv=Dv)
        cs += [dict(base, kind="ring", causal=True), dict(base, kind="ring", causal=False),
               dict(base, kind="stripe", causal=True),
               dict(base, kind="ring_varlen", causal=True, lens=lens), dict(base, kind="ring_varlen", causal=False, lens=lens)]
        # one zigzag case per exchange form, spread over the two pairs
        for form in (("ring", "gather_ps") if i == 0 else ("gather",)):
            cs.append(dict(base, kind="zigzag", causal=True, form=form))
        cs.append(dict(base, kind="zigzag_varlen", causal=True, lens=lens, vform="ring" if i == 0 else "gather"))
    cs.append(dict(W=W, S=S, D=192, Dv=128, kind="ring", causal=True, window=(S + 3, -1)))
    cs.append(dict(W=W, S=S, D=136, Dv=72, kind="zigzag", causal=True, window=(S // 2 + 1, -1), form="ring"))
    return cs


@pytest.mark.parametrize("W", [1, 2, 4])
def test_the_five_functions_match_one_single_device_fp64_attention(W):
    """out (..., H, Dv), lse, dq / dk like q / k, dv like v on every rank — GQA (4 / 2 heads), causal and not, a window, every
    zigzag exchange form.  (The parent commit returns out as wide as q.)"""
    errs, notes = VW.run_world(W, _schedule_cases(W), False, free_port())
    assert not errs, "\n".join(errs[:20])
    assert len(notes) == 5 * W * len(_schedule_cases(W))


def test_the_binders_serve_a_result_with_differing_widths(single_rank_group):
    """with_lse_grad, with_sinks and with_max_logit see only out / lse or q / k: a bound ring call at D 192 / Dv 128 against the
    fp64 autograd statement of what each computes"""
    import _blockref as BR
    import ring_flash_attn as R
    from _lsegrad_backend import LseGradBackend
    from _maxlogit_backend import MaxLogitBackend
    from _sink_backend import SinkBackend
    import _vdim_backend as VB
    import _tol
    from ring_flash_attn import _testing

    class All(VB.VdimBackend, LseGradBackend, MaxLogitBackend, SinkBackend):
        pass

    g = torch.Generator().manual_seed(5)
    S, H, HK, D, Dv = 40, 4, 2, 192, 128
    mk = lambda h, d: torch.randn(1, S, h, d, generator=g).bfloat16()
    q, k, v, do = mk(H, D), mk(HK, D), mk(HK, Dv), mk(H, Dv)
    dl = torch.randn(1, H, S, generator=g)
    sinks = torch.randn(H, generator=g)
    scale = D ** -0.5

    def ref(sink=None, dlse=None):
        qd, kd, vd = (t[0].double().requires_grad_(True) for t in (q, k, v))
        sd = None if sink is None else sink.double().requires_grad_(True)
        o, l = BR.block_forward(qd, kd, vd, scale, causal=True)
        if sd is not None:
            l2 = torch.logaddexp(l, sd.view(-1, 1))
            o, l = o * torch.exp(l - l2).transpose(0, 1).unsqueeze(-1), l2
        loss = (o * do[0].double()).sum() + (0 if dlse is None else (l * dlse[0].double()).sum())
        loss.backward()
        return o.detach()[None], l.detach()[None], qd.grad[None], kd.grad[None], vd.grad[None], None if sd is None else sd.grad

    _testing.set_backend(All(serves=("mask_shift", "mask_shift_lens")))
    try:
        for name in ("lse_grad", "sinks", "max_logit"):
            qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
            sk = sinks.clone().requires_grad_(True)
            m = torch.full((H,), float("-inf"))
            fn = {"lse_grad": lambda: R.with_lse_grad(R.ring_flash_attn_func), "sinks": lambda: R.with_sinks(R.ring_flash_attn_func, sk),
                  "max_logit": lambda: R.with_max_logit(R.ring_flash_attn_func, m)}[name]()
            out, lse, _ = fn(qq, kk, vv, causal=True, return_attn_probs=True)
            assert out.shape == (1, S, H, Dv)
            if name == "lse_grad":
                torch.autograd.backward([out, lse], [do, dl])
            else:
                out.backward(do)
            want = ref(sinks if name == "sinks" else None, dl if name == "lse_grad" else None)
            for nm, got, w, kd_ in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, qq.grad, kk.grad, vv.grad), want,
                                       ("out", "lse", "grad", "grad", "grad")):
                _tol.compare(f"{name}.{nm}", got, w, kd_)
            if name == "sinks":
                assert torch.allclose(sk.grad.double(), want[5], rtol=2e-2, atol=2e-2)
            if name == "max_logit":
                s = torch.einsum("qhd,khd->hqk", q[0].double(), k[0].double().repeat_interleave(H // HK, dim=1)) * scale
                s = s.masked_fill(~BR.visible(S, S, True), float("-inf"))
                assert torch.allclose(m.double(), s.amax((1, 2)), rtol=1e-6)
    finally:
        _testing.set_backend(None)


# ---------------------------------------------------------------------------------------------- refusals
def _refusal_cases(W):
    S = 16
    lens = [8 * W, 4 * W]
    ok = dict(W=W, S=S, D=192, Dv=128, causal=True)
    cs = [
        dict(ok, kind="ring", refuse="ValueError", how="rows"),
        dict(ok, kind="ring_varlen", lens=lens, refuse="ValueError", how="rows"),
        dict(ok, kind="ring", Dv=68, refuse="ValueError"),
        dict(ok, kind="zigzag", D=128, Dv=64, refuse="NotImplementedError"),
        dict(ok, kind="ring", D=64, Dv=32, refuse="NotImplementedError"),
        dict(ok, kind="stripe", D=256, Dv=128, refuse="NotImplementedError"),
        dict(ok, kind="ring", D=200, Dv=128, refuse="NotImplementedError"),
        dict(ok, kind="ring", D=192, Dv=160, refuse="NotImplementedError"),
        dict(ok, kind="ring", D=136, Dv=192, refuse="NotImplementedError"),
        dict(ok, kind="llama3", refuse="NotImplementedError"),
        dict(ok, kind="zigzag_llama3", refuse="NotImplementedError"),
    ]
    for kind in ("ring", "zigzag", "stripe", "ring_varlen", "zigzag_varlen"):
        more = dict(lens=lens) if kind.endswith("varlen") else {}
        cs += [dict(ok, kind=kind, refuse="NotImplementedError", how=how, **more) for how in ("dropout", "alibi", "backend")]
    if W > 1:
        cs.append(dict(ok, kind="ring", refuse="NotImplementedError", how="ulysses"))
    return cs


@pytest.mark.parametrize("W", [1, 2])
def test_every_refusal_is_raised_on_every_rank_before_anything_is_exchanged(W):
    errs, _ = VW.run_world(W, _refusal_cases(W), False, free_port())
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------------------------------------- register audit
def test_the_kernels_fit_the_register_file(tmp_path):
    """csrc/rfa_vdim.hip runs one wave per SIMD with the whole 512-entry register file, as csrc/rfa_bigd.hip does; its kernels
    are held to what their counterparts there are allowed (tests/test_abi.py): forward and dK + dV at most 512 registers with
    0 and at most 4 spilled, the 7-GEMM dQ at most 32 spilled.  Register and spill counts only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "ring-flash-attention_amd", "csrc", "rfa_vdim.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", str(tmp_path / "x.o"),
                        "-Wno-inline-asm", "-save-temps=obj"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(tmp_path / [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")][0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {}
    for name, vgpr, spill in kernels:
        assert not any(k in name for k in ("fwd_big", "dq_big", "dkdv_big", "dkdv_fused_big")), name
        kind = next((k for k in ("vd_fwd_kernel", "vd_dq_kernel", "vd_dkdv_kernel") if k in name), None)
        assert kind, name
        seen.setdefault(kind, []).append((int(vgpr), int(spill)))
    assert all(len(seen.get(k, [])) == 2 for k in ("vd_fwd_kernel", "vd_dq_kernel", "vd_dkdv_kernel")), seen     # bf16, fp16
    assert all(v <= 512 and s == 0 for v, s in seen["vd_fwd_kernel"]), seen
    assert all(v <= 512 and s <= 4 for v, s in seen["vd_dkdv_kernel"]), seen
    assert all(v <= 512 and s <= 32 for v, s in seen["vd_dq_kernel"]), seen
