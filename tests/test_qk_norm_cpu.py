"""Fused per-head QK RMSNorm + rotary (ring_flash_attn.apply_qk_norm_rotary), no device: the index arithmetic of the kernels (a
stand-alone C++ program under ASan / UBSan), the C ABI of rfa_qk_norm_rotary_fwd / _bwd (layout against a compiled C snippet,
the export set, every argument check with pointers that are never dereferenced, what HipBackend writes into the structs), and
— on the CPU test backend with the two calls written in torch fp32 (tests/_qknorm_backend.py) — forward and all four gradients
against fp64 autograd of the textbook formula, the refusals, the bit properties on shards, and W gloo ranks with the attention
behind it.

Bounds (u = 2^-8 bf16 / 2^-11 fp16, `half` the io dtype's half subnormal step):
    forward  |err| <= max(u |ref|, half) + 2^-19 Mf      Mf = |y1 c| + |y2 s|, pass-through |y|
    dx       |err| <= max(u |ref|, half) + 2^-18 Mb      Mb = rstd (|g|mag |a| + |xh| (1/D) sum |g|mag |a| |xh|)
    dw       |err| <= (n + 24) 2^-24 T   (fp32)          T = sum |g|mag |xh|, n the longest accumulation chain
On this backend the sum over (batch, row, head) is torch's own: n is bounded by the number of terms, B S H.  A weight gradient
returned in the io dtype is rounded once more: + u |ref|."""
import ctypes as C
import os
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
import _qknorm_worker as QW                      # noqa: E402
from _droppos_worker import PREFIX, shard, unshard   # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


# ---------------------------------------------------------------------------------------------- the index arithmetic
def test_index_functions_host_check_under_asan_and_ubsan():
    """tests/native/qknorm_check.cpp on the very header the kernels include: lane-group size, every chunk's offsets, every
    column of every (row, head) owned once, roles / partners / table columns, the walk, the partial count, the fold's runs"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "qknorm_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "qknorm_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "1731 configurations ok" in res.stdout, res.stdout


# ---------------------------------------------------------------------------------------------- C ABI
HEAD = ["ntensors", "B", "S", "D", "dtype", "R", "rot_offset", "interleaved", "table_dtype", "weight_dtype", "eps", "weight_offset",
        "t", "weight", "cos", "sin", "P", "positions", "pos_batch", "pos_offset", "pos_stride", "pos_split", "pos_offset2"]
TAIL = ["g", "dweight", "workspace", "workspace_bytes"]
GRAD = ["dout", "dout_batch", "dout_row", "dout_head"]


def test_structs_match_the_c_layout_and_the_export_set(built):
    from ring_flash_attn import _C

    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu %zu %zu %d\\n", sizeof(rfa_qk_norm_rotary_args), sizeof(rfa_qk_norm_rotary_bwd_args), ' \
           'sizeof(rfa_qk_norm_grad), RFA_QK_NORM_WEIGHT_F32);\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_norm_rotary_args, {f}));\n' for f in HEAD) + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_norm_rotary_bwd_args, {f}));\n' for f in HEAD + TAIL) + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_norm_grad, {f}));\n' for f in GRAD) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    F, Bw, G = _C.QkNormRotaryArgs, _C.QkNormRotaryBwdArgs, _C.QkNormGrad
    assert got[:4] == [C.sizeof(F), C.sizeof(Bw), C.sizeof(G), _C.QK_NORM_WEIGHT_F32]
    assert got[4:] == [getattr(F, f).offset for f in HEAD] + [getattr(Bw, f).offset for f in HEAD + TAIL] + \
        [getattr(G, f).offset for f in GRAD]
    assert [f for f, _ in F._fields_] == ["struct_bytes", "reserved"] + HEAD
    assert [f for f, _ in Bw._fields_] == ["struct_bytes", "reserved"] + HEAD + TAIL and [f for f, _ in G._fields_] == GRAD
    assert F.struct_bytes.offset == 0 and F.reserved.offset == 4 and Bw.struct_bytes.offset == 0 and Bw.reserved.offset == 4
    assert F().struct_bytes == C.sizeof(F) and Bw().struct_bytes == C.sizeof(Bw)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40      # the ABI stays
    new = {"rfa_qk_norm_rotary_fwd", "rfa_qk_norm_rotary_bwd", "rfa_qk_norm_rotary_bwd_workspace_bytes"}
    assert new <= set(_C.SYMBOLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)


def _args(bwd=False, **kw):
    from ring_flash_attn import _C

    a = (_C.QkNormRotaryBwdArgs if bwd else _C.QkNormRotaryArgs)()
    a.ntensors, a.B, a.S, a.D, a.dtype, a.R, a.rot_offset = 1, 2, 6, 32, 0, 32, 0
    a.table_dtype, a.weight_dtype, a.eps = _C.ROTARY_TABLE_F32, _C.QK_NORM_WEIGHT_F32, 1e-6
    a.cos, a.sin, a.P = 4096, 8192, 16                         # (addresses that are never dereferenced)
    a.weight[0] = 1 << 16
    t = a.t[0]
    t.src, t.dst, t.H = 512, 1 << 20, 8
    t.src_batch, t.src_row, t.src_head = 6 * 8 * 32, 8 * 32, 32
    t.dst_batch, t.dst_row, t.dst_head = 6 * 8 * 32, 8 * 32, 32
    if bwd:
        g = a.g[0]
        g.dout, g.dout_batch, g.dout_row, g.dout_head = 1 << 22, 6 * 8 * 32, 8 * 32, 32
        a.dweight[0], a.workspace, a.workspace_bytes = 1 << 24, 1 << 26, 1 << 20
    for k, v in kw.items():
        if k.startswith("t_"):
            setattr(a.t[0], k[2:], v)
        elif k.startswith("g_"):
            setattr(a.g[0], k[2:], v)
        elif k in ("weight", "dweight"):
            getattr(a, k)[0] = v
        else:
            setattr(a, k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    """Past every host check a call would launch, so every case below stops at the check it names; none passes them all."""
    from ring_flash_attn import _C

    lib = _C.load()
    assert lib.rfa_qk_norm_rotary_fwd(None, None) == ERR_NULL and lib.rfa_qk_norm_rotary_bwd(None, None) == ERR_NULL
    assert lib.rfa_qk_norm_rotary_bwd_workspace_bytes(None) == 0
    inf, nan = float("inf"), float("nan")
    shared = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(ntensors=0), dict(ntensors=3), dict(interleaved=2),
                   dict(interleaved=-1), dict(t_pad=1), dict(eps=-1e-6), dict(eps=inf), dict(eps=nan), dict(weight_offset=inf),
                   dict(weight_offset=nan), dict(t_dst=512), dict(pos_batch=-1), dict(pos_stride=-1), dict(pos_split=6),
                   dict(pos_split=-1), dict(pos_offset=11), dict(pos_offset=-1), dict(P=5), dict(pos_stride=3, P=15),
                   dict(pos_split=3, pos_offset2=14), dict(pos_offset=1 << 62)],
        ERR_DTYPE: [dict(dtype=2), dict(dtype=-1), dict(table_dtype=1), dict(table_dtype=3), dict(weight_dtype=1),
                    dict(weight_dtype=3), dict(dtype=1, table_dtype=0), dict(dtype=1, weight_dtype=0)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(D=-8), dict(R=-16), dict(R=24), dict(R=48),
                       dict(interleaved=1, R=12), dict(rot_offset=4), dict(rot_offset=-8), dict(rot_offset=8), dict(R=16, rot_offset=24),
                       dict(R=0, rot_offset=40)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(P=0), dict(P=-3), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, t_H=2)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2)],
        ERR_NULL: [dict(cos=None), dict(sin=None), dict(t_src=None), dict(t_dst=None), dict(weight=None)],
        ERR_ALIGN: [dict(cos=4100), dict(sin=8200), dict(t_src=520), dict(t_dst=(1 << 20) + 8), dict(weight=(1 << 16) + 8),
                    dict(t_src_row=8 * 32 + 4), dict(t_src_batch=6 * 8 * 32 + 2), dict(t_src_head=36), dict(t_dst_row=8 * 32 + 4),
                    dict(t_dst_batch=3), dict(t_dst_head=36)],
    }
    only_bwd = {
        ERR_NULL: [dict(g_dout=None), dict(workspace=None)],
        ERR_ALIGN: [dict(g_dout=(1 << 22) + 8), dict(g_dout_row=8 * 32 + 4), dict(g_dout_head=36), dict(g_dout_batch=2),
                    dict(dweight=(1 << 24) + 2), dict(workspace=(1 << 26) + 8)],
        ERR_ARGS: [dict(t_dst=1 << 22), dict(workspace_bytes=0), dict(workspace_bytes=127)],
    }
    for bwd, fn in ((False, lib.rfa_qk_norm_rotary_fwd), (True, lib.rfa_qk_norm_rotary_bwd)):
        call = lambda **kw: fn(C.byref(_args(bwd, **kw)), None)
        for want, cases in shared.items():
            for kw in cases:
                assert call(**kw) == want, (bwd, want, kw)
        # the order: the struct's size first, flags and eps before a dtype, a dtype before a head dim, ...
        assert call(struct_bytes=8, dtype=2) == ERR_ARGS
        assert call(eps=-1.0, dtype=2) == ERR_ARGS
        assert call(dtype=2, D=12) == ERR_DTYPE
        assert call(weight_dtype=1, D=12) == ERR_DTYPE
        assert call(D=12, B=-1) == ERR_HEAD_DIM
        assert call(B=-1, t_H=0) == ERR_SHAPE
        assert call(t_H=0, cos=None) == ERR_HEADS
        assert call(cos=None, t_src=520) == ERR_NULL
        assert call(t_src=520, t_dst=512) == ERR_ALIGN
        assert call(weight=(1 << 16) + 8, pos_stride=-1) == ERR_ALIGN
        # no rows: nothing is launched and no pointer is needed; the map is not looked at either
        assert call(B=0, cos=None, sin=None, t_src=None, t_dst=None, weight=None) == OK
        assert call(S=0, cos=None, sin=None, t_src=None, t_dst=None, pos_split=3) == OK
        # R == 0 is the norm alone: tables, P and the map are not looked at — the call gets as far as the next check
        assert call(R=0, cos=None, sin=None, P=0, pos_stride=-1, pos_split=99, t_src=None) == ERR_NULL
        assert call(R=0, cos=None, sin=None, P=0, pos_stride=-1, t_dst=512) == ERR_ARGS
        # with `positions` the map's fields are not looked at
        assert call(positions=64, pos_stride=-1, pos_split=99, P=1, cos=None) == ERR_NULL
        # a second tensor is checked like the first, and EVERY tensor's heads before ANY tensor's item count
        a = _args(bwd, ntensors=2, cos=None)
        a.t[1].src, a.t[1].dst, a.t[1].H = 512, 1024, 0
        assert fn(C.byref(a), None) == ERR_HEADS
        a.t[1].H = 2
        assert fn(C.byref(a), None) == ERR_NULL                    # (cos — and the second tensor has no weight)
        a.t[0].H, a.t[1].H = 2 ** 30, 0
        assert fn(C.byref(a), None) == ERR_HEADS
        a.t[1].H = 2
        assert fn(C.byref(a), None) == ERR_SHAPE
    call = lambda **kw: lib.rfa_qk_norm_rotary_bwd(C.byref(_args(True, **kw)), None)
    for want, cases in only_bwd.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    assert call(g_dout=None, t_src=520) == ERR_NULL and call(g_dout=(1 << 22) + 8, t_dst=512) == ERR_ALIGN
    # without a dweight neither the workspace nor its size is looked at: the call gets as far as the last check
    assert call(dweight=None, workspace=None, workspace_bytes=0, pos_offset=11) == ERR_ARGS
    # the workspace size: a function of the shape alone — 2 x 6 x 8 items of 4 lanes: 64 per workgroup, 2 partials of 32 floats
    size = lambda **kw: lib.rfa_qk_norm_rotary_bwd_workspace_bytes(C.byref(_args(True, **kw)))
    assert size() == 2 * 32 * 4 == size(cos=None, t_src=None, dweight=None, workspace=None, pos_offset=99)
    assert size(B=1, S=64) == 8 * 32 * 4 and size(B=1, S=65) == 9 * 32 * 4
    assert size(B=1, S=2 ** 20) == 1024 * 32 * 4 == size(B=2 ** 4, S=2 ** 20)        # capped at 1024 partials
    assert size(D=12) == 0 and size(reserved=1) == 0 and size(B=0) == 0
    assert call(workspace_bytes=2 * 32 * 4 - 1) == ERR_ARGS


def test_what_the_backend_writes_into_the_structs(built, monkeypatch):
    """HipBackend.qk_norm_rotary_fwd / _bwd on CPU tensors with the library replaced by a recorder: every field of both structs"""
    from ring_flash_attn import _C, backend

    seen = {}

    class Lib:
        def rfa_qk_norm_rotary_fwd(self, a, s):
            seen["fwd"] = _C.QkNormRotaryArgs.from_buffer_copy(a._obj)
            return 0

        def rfa_qk_norm_rotary_bwd(self, a, s):
            seen["bwd"] = _C.QkNormRotaryBwdArgs.from_buffer_copy(a._obj)
            return 0

        def rfa_qk_norm_rotary_bwd_workspace_bytes(self, a):
            return 4096

    monkeypatch.setattr(backend, "_stream", lambda t: None)
    monkeypatch.setattr(backend.HipBackend, "_check_dev", staticmethod(lambda *ts: None))
    be = object.__new__(backend.HipBackend)
    be.lib = Lib()
    qkv = torch.zeros(2, 6, 3, 4, 64, dtype=torch.float16)
    q, k = qkv[:, :, 0], qkv[:, :, 1, :2]
    oq, ok = torch.empty(2, 6, 4, 64, dtype=torch.float16), torch.empty(2, 6, 2, 64, dtype=torch.float16)
    wq, wk = torch.ones(64), torch.ones(64)
    cos, sin = torch.ones(40, 16), torch.zeros(40, 16)
    pos = torch.zeros(2, 6, dtype=torch.int32)
    be.qk_norm_rotary_fwd([q, k], [oq, ok], [wq, wk], cos, sin, positions=pos, pos_map=(5, (1, 0, 0)), interleaved=True,
                          rot_offset=8, eps=1e-5, weight_offset=1.0)
    a = seen["fwd"]
    assert (a.struct_bytes, a.reserved, a.ntensors, a.B, a.S, a.D, a.dtype) == (C.sizeof(_C.QkNormRotaryArgs), 0, 2, 2, 6, 64, 1)
    assert (a.R, a.rot_offset, a.interleaved, a.table_dtype, a.weight_dtype) == (32, 8, 1, _C.ROTARY_TABLE_F32, _C.QK_NORM_WEIGHT_F32)
    assert abs(a.eps - 1e-5) < 1e-12 and a.weight_offset == 1.0
    t0, t1 = a.t[0], a.t[1]
    assert (t0.src, t0.dst, t0.H, t0.pad) == (q.data_ptr(), oq.data_ptr(), 4, 0) and (t1.src, t1.dst, t1.H) == (k.data_ptr(), ok.data_ptr(), 2)
    assert (t0.src_batch, t0.src_row, t0.src_head) == (6 * 768, 768, 64) == (t1.src_batch, t1.src_row, t1.src_head)
    assert (t0.dst_batch, t0.dst_row, t0.dst_head) == (6 * 256, 256, 64) and (t1.dst_batch, t1.dst_row, t1.dst_head) == (6 * 128, 128, 64)
    assert list(a.weight) == [wq.data_ptr(), wk.data_ptr()] and (a.cos, a.sin, a.P) == (cos.data_ptr(), sin.data_ptr(), 40)
    assert (a.positions, a.pos_batch, a.pos_offset, a.pos_stride, a.pos_split, a.pos_offset2) == (pos.data_ptr(), 6, 5, 0, 0, 0)
    # backward: packed input, io-dtype weights and tables, the map, one dweight only, norm-only
    x, g, dx = (torch.zeros(7, 3, 64, dtype=torch.float16) for _ in range(3))
    w16, dw = torch.ones(64, dtype=torch.float16), torch.empty(64)
    be.qk_norm_rotary_bwd([x, x], [g, g], [dx, dx], [w16, w16], [None, dw], cos.half(), sin.half(), pos_map=(3, (2, 4, 20)))
    b = seen["bwd"]
    assert (b.struct_bytes, b.ntensors, b.B, b.S, b.D, b.R, b.P) == (C.sizeof(_C.QkNormRotaryBwdArgs), 2, 1, 7, 64, 32, 40)
    assert (b.table_dtype, b.weight_dtype, b.positions) == (1, 1, None)
    assert (b.pos_offset, b.pos_stride, b.pos_split, b.pos_offset2) == (3, 2, 4, 20)
    assert (b.t[0].src, b.t[0].dst, b.t[0].src_batch, b.t[0].src_row, b.t[0].src_head) == (x.data_ptr(), dx.data_ptr(), 0, 192, 64)
    assert (b.g[1].dout, b.g[1].dout_batch, b.g[1].dout_row, b.g[1].dout_head) == (g.data_ptr(), 0, 192, 64)
    assert list(b.dweight) == [None, dw.data_ptr()] and b.workspace and b.workspace_bytes == 4096
    be.qk_norm_rotary_bwd([x], [g], [dx], [w16], [None], None, None)
    b = seen["bwd"]
    assert (b.R, b.cos, b.sin, b.P, b.table_dtype, b.workspace, b.workspace_bytes) == (0, None, None, 0, 1, None, 0)
    with pytest.raises(ValueError, match="dweight"):
        be.qk_norm_rotary_bwd([x], [g], [dx], [w16], [torch.empty(64, dtype=torch.float16)], None, None)
    with pytest.raises(ValueError, match="weights"):
        be.qk_norm_rotary_fwd([x], [dx], [torch.ones(32)], None, None)


# ---------------------------------------------------------------------------------------------- on the test backend
@pytest.fixture
def qk_backend():
    from ring_flash_attn import _testing
    from _qknorm_backend import QkNormBackend

    be = QkNormBackend(serves=("mask_shift",))
    _testing.set_backend(be)
    yield be
    _testing.set_backend(None)


def _tables(P, R, dtype=torch.float32):
    ang = torch.arange(P, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(R // 2, dtype=torch.float64) / (R // 2)))
    return ang.cos().to(dtype), ang.sin().to(dtype)


def _qk(B, S, H, Hk, D, dtype=torch.bfloat16, seed=5, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(B, S, H, D, generator=g)).to(dtype), (scale * torch.randn(B, S, Hk, D, generator=g)).to(dtype)


def _w(D, dtype=torch.float32, seed=4):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.25 * torch.randn(D, generator=g)).to(dtype), (1.0 + 0.25 * torch.randn(D, generator=g)).to(dtype)


def _textbook(x, w, cos, sin, pos, inter, ro, eps, woff):
    """differentiable, any dtype: the formulas as the papers print them"""
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (woff + w)
    if cos is None:
        return y
    Rw = 2 * cos.shape[1]
    c, s = cos[pos].unsqueeze(-2), sin[pos].unsqueeze(-2)
    r = y[..., ro:ro + Rw]
    if inter:
        x1, x2 = r[..., 0::2], r[..., 1::2]
        rot = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)
    else:
        x1, x2 = r[..., :Rw // 2], r[..., Rw // 2:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return torch.cat([y[..., :ro], rot, y[..., ro + Rw:]], dim=-1)


def _over(got, ref, mag, dtype, fac):
    lim = (U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + fac * mag
    return ((got.double() - ref).abs() - lim).max().item()


def _over_dw(got, ref, T, n, wdtype):
    lim = (n + 24) * 2.0 ** -24 * T
    if wdtype != torch.float32:
        lim = lim + (U_OF[wdtype] * ref.abs()).clamp(min=HALF_STEP[wdtype])
    return ((got.double() - ref).abs() - lim).max().item()


@pytest.mark.parametrize("inter,D,Rw,ro", [(False, 64, 64, 0), (True, 40, 8, 8), (False, 192, 64, 128), (False, 128, 0, 0)])
@pytest.mark.parametrize("dtype,tdtype,woff,scale", [(torch.bfloat16, torch.float32, 0.0, 1.0), (torch.float16, torch.float16, 1.0, 0.01),
                                                     (torch.bfloat16, torch.bfloat16, 1.0, 30.0)])
def test_forward_and_all_four_gradients_against_fp64_autograd(qk_backend, inter, D, Rw, ro, dtype, tdtype, woff, scale):
    """out, dq, dk, dw_q, dw_k within the derived bounds of fp64 autograd through the textbook formula — fp32 and io-dtype tables
    and weights, weight_offset 0 and 1 (Gemma-3), inputs scaled by 0.01 and 30, (B, S) positions, the norm-only call, packed"""
    import ring_flash_attn as R
    from _qknorm_backend import reference

    B, S, H, Hk, eps = 2, 11, 3, 1, 1e-6
    q, k = _qk(B, S, H, Hk, D, dtype, scale=scale)
    wq, wk = _w(D, tdtype)
    cos, sin = _tables(40, Rw, tdtype) if Rw else (None, None)
    pos = torch.randint(0, 40, (B, S), generator=torch.Generator().manual_seed(8)).to(torch.int32)
    dqo, dko = _qk(B, S, H, Hk, D, dtype, seed=6)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, wq, wk)]
    kw = dict(eps=eps, weight_offset=woff, interleaved=inter, rot_offset=ro)
    qo, ko = R.apply_qk_norm_rotary(*leaves, cos, sin, positions=pos if Rw else None, **kw)
    assert qo.dtype == dtype and qo.is_contiguous() and qo.shape == q.shape and ko.shape == k.shape
    torch.autograd.backward([qo, ko], [dqo, dko])
    for name, x, w, out, dout, xl, wl in (("q", q, wq, qo, dqo, leaves[0], leaves[2]), ("k", k, wk, ko, dko, leaves[1], leaves[3])):
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        ref = _textbook(x64, w64, None if cos is None else cos.double(), None if sin is None else sin.double(), pos.long(),
                        inter, ro, eps, woff)
        ref.backward(dout.double())
        r = reference(x, w, cos, sin, pos, inter, ro, eps, woff, dout=dout)
        # (the two statements of the formulas agree: values and both gradients)
        assert torch.allclose(r["y"], ref.detach(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(r["dx"], x64.grad, rtol=1e-9, atol=1e-12 * scale ** -1)
        assert torch.allclose(r["dw"], w64.grad, rtol=1e-9, atol=1e-11)
        assert _over(out, ref.detach(), r["Mf"], dtype, 2.0 ** -19) <= 0, name
        assert _over(xl.grad, x64.grad, r["Mb"], dtype, 2.0 ** -18) <= 0, name
        assert wl.grad.dtype == w.dtype and _over_dw(wl.grad, w64.grad, r["T"], B * S * x.shape[2], tdtype) <= 0, name
    # packed input: (T, H, D) with (T,) positions is the (1, T, H, D) call
    qp = q.reshape(B * S, H, D)
    out_p = R.apply_qk_norm_rotary(qp, None, wq, None, cos, sin, positions=pos.reshape(-1) if Rw else None, **kw)
    assert torch.equal(out_p, qo.detach().reshape(B * S, H, D))
    calls = qk_backend.qk_norm_calls
    assert [c["dir"] for c in calls[:2]] == ["fwd", "bwd"] and calls[0]["n"] == calls[1]["n"] == 2         # one call per direction
    assert calls[1]["dweights"] == [True, True] and calls[0]["tables"] == bool(Rw)


def test_eps_zero_is_served(qk_backend):
    """eps = 0: forward and all four gradients against the fp64 reference with eps = 0, the same bounds"""
    import ring_flash_attn as R
    from _qknorm_backend import reference

    B, S, H, Hk, D = 2, 11, 3, 1, 64
    q, k = _qk(B, S, H, Hk, D)
    wq, wk = _w(D)
    cos, sin = _tables(40, 32)
    dqo, dko = _qk(B, S, H, Hk, D, seed=6)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, wq, wk)]
    qo, ko = R.apply_qk_norm_rotary(*leaves, cos, sin, eps=0, rot_offset=16)
    torch.autograd.backward([qo, ko], [dqo, dko])
    assert qk_backend.qk_norm_calls[0]["eps"] == 0.0
    for x, w, out, dout, xl, wl in ((q, wq, qo, dqo, leaves[0], leaves[2]), (k, wk, ko, dko, leaves[1], leaves[3])):
        r = reference(x, w, cos, sin, torch.arange(S), False, 16, 0.0, 0.0, dout=dout)
        assert _over(out, r["y"], r["Mf"], torch.bfloat16, 2.0 ** -19) <= 0
        assert _over(xl.grad, r["dx"], r["Mb"], torch.bfloat16, 2.0 ** -18) <= 0
        assert _over_dw(wl.grad, r["dw"], r["T"], B * S * x.shape[2], torch.float32) <= 0


def test_saved_tensors_checkpointing_partial_gradients_and_one_tensor(qk_backend):
    import ring_flash_attn as R
    from torch.utils.checkpoint import checkpoint

    q, k = _qk(2, 12, 4, 2, 64)
    wq, wk = _w(64)
    cos, sin = _tables(64, 32)
    dqo, dko = _qk(2, 12, 4, 2, 64, seed=6)
    kw = dict(rot_offset=16, eps=1e-5)

    def grads(fn, wgrad=(True, True), douts=(dqo, dko)):
        ls = [q.clone().requires_grad_(True), k.clone().requires_grad_(True), wq.clone().requires_grad_(wgrad[0]),
              wk.clone().requires_grad_(wgrad[1])]
        outs = fn(*ls)
        torch.autograd.backward([o for o, d in zip(outs, douts) if d is not None], [d for d in douts if d is not None])
        return outs, [t.grad for t in ls]

    plain = lambda a, b, c, d: R.apply_qk_norm_rotary(a, b, c, d, cos, sin, **kw)
    (qo, ko), (dq, dk, dwq, dwk) = grads(plain)
    # what the Function keeps: the inputs, the weights and the tables — neither rstd nor the outputs
    ls = [q.clone().requires_grad_(True), k.clone().requires_grad_(True), wq.clone().requires_grad_(True), wk.clone().requires_grad_(True)]
    o = R.apply_qk_norm_rotary(*ls, cos, sin, **kw)
    saved = [t for t in o[0].grad_fn.saved_tensors if t is not None]
    assert {t.data_ptr() for t in saved} == {t.data_ptr() for t in ls + [cos, sin]}
    # checkpointing re-runs the call and gives the same bits
    n0 = len(qk_backend.qk_norm_calls)
    (qc, kc), gc = grads(lambda a, b, c, d: checkpoint(plain, a, b, c, d, use_reentrant=False))
    assert [c["dir"] for c in qk_backend.qk_norm_calls[n0:]] == ["fwd", "fwd", "bwd"]
    assert torch.equal(qc, qo) and torch.equal(kc, ko) and all(torch.equal(a, b) for a, b in zip(gc, (dq, dk, dwq, dwk)))
    # weights without grad: no dweight is asked for, the input gradients are the same bits
    _, g2 = grads(plain, wgrad=(False, True))
    assert qk_backend.qk_norm_calls[-1]["dweights"] == [False, True]
    assert g2[2] is None and torch.equal(g2[3], dwk) and torch.equal(g2[0], dq) and torch.equal(g2[1], dk)
    _, g3 = grads(plain, wgrad=(False, False))
    assert qk_backend.qk_norm_calls[-1]["dweights"] == [False, False] and g3[2] is None and g3[3] is None and torch.equal(g3[0], dq)
    # an incoming None gradient for one tensor skips that tensor
    _, g4 = grads(plain, douts=(None, dko))
    assert qk_backend.qk_norm_calls[-1]["n"] == 1 and g4[0] is None and g4[2] is None and torch.equal(g4[1], dk) and torch.equal(g4[3], dwk)
    # one tensor only == its half of the pair; strided qkv slices == their contiguous copies, in one launch
    one = R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, **kw)
    assert isinstance(one, torch.Tensor) and torch.equal(one, qo)
    qkv = torch.randn(2, 12, 3, 4, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    n0 = len(qk_backend.qk_norm_calls)
    a, b = R.apply_qk_norm_rotary(qkv[:, :, 0], qkv[:, :, 1], wq, wk, cos, sin, **kw)
    c, d = R.apply_qk_norm_rotary(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), wq, wk, cos, sin, **kw)
    assert torch.equal(a, c) and torch.equal(b, d) and len(qk_backend.qk_norm_calls) == n0 + 2
    # norm-only == tables of cos 1 / sin 0; weight_offset = 1 with w == a weight of 1 + w
    ones, zeros = torch.ones(64, 16), torch.zeros(64, 16)
    assert torch.equal(R.apply_qk_norm_rotary(q, None, wq, None), R.apply_qk_norm_rotary(q, None, wq, None, ones, zeros, rot_offset=16))
    assert torch.equal(R.apply_qk_norm_rotary(q, None, wq - 1.0, None, cos, sin, weight_offset=1.0),
                       R.apply_qk_norm_rotary(q, None, (wq - 1.0) + 1.0, None, cos, sin))
    # modes: offset, explicit positions, the clamp — as apply_rotary
    ar = torch.arange(12, dtype=torch.int32)
    off = R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, offset=7)
    assert torch.equal(off, R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, positions=ar + 7))
    assert torch.equal(off, R.apply_qk_norm_rotary(q, None, wq, None, cos, sin, positions=ar, offset=7)) and not torch.equal(off, one)
    # an all-zero row with eps > 0 gives zeros, no NaN
    z = q.clone()
    z[0, 3] = 0
    zo = R.apply_qk_norm_rotary(z, None, wq, None, cos, sin)
    assert not torch.isnan(zo).any() and bool((zo[0, 3] == 0).all())


def test_every_refusal_comes_before_a_launch(qk_backend, single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _rotary_backend import RotaryBackend

    q, k = _qk(2, 12, 4, 2, 64)
    wq, wk = _w(64)
    cos, sin = _tables(64, 32)
    ar = torch.arange(12, dtype=torch.int32)
    value = [
        (dict(q_weight=wq[:32]), "weights must be"), (dict(k_weight=wk.view(1, 64)), "weights must be"),
        (dict(q_weight=wq.double()), "weights must be"), (dict(q_weight=wq.half(), k_weight=wk.half()), "weights must be"),
        (dict(k_weight=wk.bfloat16()), "weights must be"), (dict(q_weight=torch.ones(128)[::2]), "weights must be"),
        (dict(q_weight=[1.0] * 64), "weights must be"), (dict(q_weight=wq.to("meta")), "weights must be"),
        (dict(sin=None), "cos and sin come together"), (dict(cos=None), "cos and sin come together"),
        (dict(k=None), "k and k_weight"), (dict(k_weight=None), "k and k_weight"),
        (dict(eps=-1e-6), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
        (dict(weight_offset=float("inf")), "weight_offset"), (dict(weight_offset=float("nan")), "weight_offset"),
        (dict(layout=R.ring_flash_attn_func, positions=ar), "at most one"),
        (dict(q=q.float()), "bf16"), (dict(q=q[..., :60]), "head dim"), (dict(q=q[0, 0]), r"\(B, S, H, D\)"),
        (dict(k=k[:, :6]), "k must share"), (dict(k=k.half()), "k must share"), (dict(k=k[..., :32]), "k must share"),
        (dict(cos=cos[:, :8]), "one shape"), (dict(cos=cos.double(), sin=sin.double()), "fp32 or"),
        (dict(cos=cos.half(), sin=sin.half()), "fp32 or"), (dict(cos=cos.t().contiguous().t(), sin=sin.t().contiguous().t()), "contiguous"),
        (dict(cos=cos[:, :12].contiguous(), sin=sin[:, :12].contiguous()), "multiple of 16"),
        (dict(cos=cos[:, :6].contiguous(), sin=sin[:, :6].contiguous(), interleaved=True), "multiple of 8"),
        (dict(rot_offset=4), "rot_offset"), (dict(rot_offset=40), "rot_offset"), (dict(rot_offset=-8), "rot_offset"),
        (dict(cos=None, sin=None, rot_offset=72), "rot_offset"),
        (dict(positions=ar.long()), "int32"), (dict(positions=ar[:5]), "int32"), (dict(positions=ar.view(1, 12)), "int32"),
        (dict(positions=list(range(12))), "int32"),
        (dict(offset=53), "positions 53 .. 64"), (dict(offset=-1), "positions -1 .. 10"),
        (dict(layout=R.zigzag_ring_flash_attn_func, q=q[:, :11], k=k[:, :11]), "odd"),
        (dict(layout=R.ring_flash_attn_func, q=q[0], k=k[0]), r"needs \(B, S, H, D\)"),
        (dict(cos=3.0, sin=4.0), "cos and sin must be tensors"),
    ]
    for kw, match in value:
        a = dict(dict(q=q, k=k, q_weight=wq, k_weight=wk, cos=cos, sin=sin), **kw)
        with pytest.raises(ValueError, match=match):
            R.apply_qk_norm_rotary(a.pop("q"), a.pop("k"), a.pop("q_weight"), a.pop("k_weight"), a.pop("cos"), a.pop("sin"), **a)
    for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.llama3_flash_attn_varlen_func,
                 R.ring_flash_attn_varlen_func, R.zigzag_llama3_flash_attn_varlen_kvpacked_func):
        with pytest.raises(TypeError):
            R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin, layout=notf)
    with pytest.raises(TypeError):                                                     # there is no in-place mode
        R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin, inplace=True)
    assert not qk_backend.qk_norm_calls                                                # nothing was launched
    # all nine dense functions are layouts (a group of one rank: positions 0 .. S-1)
    plain = R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin)
    for kind in PREFIX.values():
        for form in ("", "kvpacked_", "qkvpacked_"):
            got = R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin, layout=getattr(R, f"{kind}_{form}func"))
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
            assert qk_backend.qk_norm_calls[-1]["positions"] is False                  # the map's numbers: no tensor was built
    # a backend without the flag
    _testing.set_backend(RotaryBackend(serves=("mask_shift",)))
    with pytest.raises(NotImplementedError, match="serves `qk_norm`"):
        R.apply_qk_norm_rotary(q, k, wq, wk, cos, sin)
    assert "apply_qk_norm_rotary" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21


@pytest.mark.parametrize("kind", ["ring", "zigzag", "stripe"])
@pytest.mark.parametrize("W", [2, 4])
def test_every_ranks_shard_is_the_shard_of_the_single_device_result(qk_backend, kind, W):
    """positions = local_positions(rank=r): rank r's result is, bit for bit, rank r's shard of the single-device result — both
    pairings, a rot_offset, the norm alone, with and without k; the ranks' PARTIAL weight gradients sum to the single-device one
    within the bound (each rank's partial within the bound of its own chain and magnitudes; the sum taken in fp64)"""
    import ring_flash_attn as R
    from _qknorm_backend import reference

    func = getattr(R, PREFIX[kind] + "_func")
    n = 10
    for inter, D, Rw, ro in ((False, 64, 64, 0), (True, 40, 8, 8), (False, 192, 64, 128), (False, 72, 0, 0)):
        q, k = _qk(2, W * n, 3, 1, D)
        wq, wk = _w(D)
        dqo, dko = _qk(2, W * n, 3, 1, D, seed=6)
        cos, sin = _tables(W * n, Rw) if Rw else (None, None)
        kw = dict(interleaved=inter, rot_offset=ro, weight_offset=1.0)
        wl = [wq.clone().requires_grad_(True), wk.clone().requires_grad_(True)]
        qf, kf = R.apply_qk_norm_rotary(q, k, *wl, cos, sin, **kw)
        torch.autograd.backward([qf, kf], [dqo, dko])
        parts, dws = [], []
        for r in range(W):
            pos = R.local_positions(func, n, rank=r, world_size=W)
            ws = [wq.clone().requires_grad_(True), wk.clone().requires_grad_(True)]
            qs, ks = R.apply_qk_norm_rotary(shard(kind, q, r, W), shard(kind, k, r, W), *ws, cos, sin, positions=pos, **kw)
            assert torch.equal(R.apply_qk_norm_rotary(shard(kind, q, r, W), None, ws[0], None, cos, sin, positions=pos, **kw), qs)
            torch.autograd.backward([qs, ks], [shard(kind, dqo, r, W), shard(kind, dko, r, W)])
            parts.append((qs.detach(), ks.detach()))
            dws.append([w.grad for w in ws])
        assert torch.equal(unshard(kind, [p[0] for p in parts]), qf) and torch.equal(unshard(kind, [p[1] for p in parts]), kf)
        for i, (x, w, dout) in enumerate(((q, wq, dqo), (k, wk, dko))):
            ref = reference(x, w, cos, sin, torch.arange(W * n), inter, ro, 1e-6, 1.0, dout=dout)
            total = torch.stack([d[i].double() for d in dws]).sum(0)
            assert _over_dw(total, ref["dw"], ref["T"], 2 * n * x.shape[2], torch.float32) <= 0
            assert _over_dw(wl[i].grad, ref["dw"], ref["T"], 2 * W * n * x.shape[2], torch.float32) <= 0


def test_layout_on_real_groups_and_the_attention_behind_it():
    """2 gloo ranks: apply_qk_norm_rotary(layout=func) on every rank's shard equals the explicit positions in bits and un-shards
    to the single-device result bit for bit; dq, dk and the summed partial weight gradients lie within the derived bounds of one
    fp64 computation; `func` on the results lies within the *_ring kinds of exact attention, the gradients carried back through
    the norm in fp64"""
    from _qknorm_backend import reference

    W = 2
    base = dict(W=W, S=10, B=2, H=4, Hk=2, D=32, R=32)
    cases = [dict(base, kind=kind, attn=True) for kind in ("ring", "zigzag", "stripe")]
    cases.append(dict(base, kind="zigzag", D=40, R=8, rot_offset=8, interleaved=True, weight_offset=1.0))
    res, errs = QW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs)
    bad = [b for c in cases for b in QW.check_case(c, res[QW.case_name(c)], reference, lambda items: items)]
    assert not bad, "\n".join(bad)
