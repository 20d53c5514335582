"""Token-wide QK RMSNorm + rotary (ring_flash_attn.apply_qk_token_norm_rotary), no device: the index arithmetic of the kernels
(a stand-alone C++ program under ASan / UBSan), the C ABI of rfa_qk_token_norm_rotary_fwd / _bwd / _bwd_workspace_bytes (export
set, layout against a compiled C snippet, every argument check in its order with pointers that are never dereferenced) and the
public call's refusals, which all come before a launch."""
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

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
NAMES = ["rfa_qk_token_norm_rotary_fwd", "rfa_qk_token_norm_rotary_bwd", "rfa_qk_token_norm_rotary_bwd_workspace_bytes"]


def test_index_functions_host_check_under_asan_and_ubsan():
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "qktoken_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "ring-flash-attention_amd", "csrc"), os.path.join(ROOT, "tests", "native", "qktoken_check.cpp"),
                        "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "1143 configurations ok" in res.stdout, res.stdout + res.stderr


def test_symbols_and_struct_layout(built):
    from ring_flash_attn import _C

    lib = _C.load()
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in _C.SYMBOLS and hasattr(lib, n) and f" {n}(" in header and f" {n}\n" in exported
    F, Bw = _C.QkTokenNormRotaryArgs, _C.QkTokenNormRotaryBwdArgs
    fields = {"rfa_qk_token_norm_rotary_args": [f for f, _ in F._fields_], "rfa_qk_token_norm_rotary_bwd_args": [f for f, _ in Bw._fields_]}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' + \
           "".join(f'  printf("%zu\\n", sizeof({s}));\n' + "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for f in fs)
                   for s, fs in fields.items()) + '  printf("%d %d\\n", RFA_QK_TOKEN_NORM_MAX_WIDTH, RFA_QK_TOKEN_NORM_MAX_PARTS);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()]
    want = [v for T in (F, Bw) for v in [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]]
    assert got == want + [_C.QK_TOKEN_NORM_MAX_WIDTH, 512]
    assert F().struct_bytes == C.sizeof(F) and Bw().struct_bytes == C.sizeof(Bw) and F._fields_[0][0] == "struct_bytes"


def _args(bwd=False, **kw):
    from ring_flash_attn import _C      # one tensor (2, 6, 8, 32) with addresses that are never dereferenced
    a = (_C.QkTokenNormRotaryBwdArgs if bwd else _C.QkTokenNormRotaryArgs)()
    a.ntensors, a.B, a.S, a.D, a.dtype, a.R, a.rot_offset = 1, 2, 6, 32, 0, 32, 0
    a.table_dtype, a.weight_dtype, a.eps = _C.ROTARY_TABLE_F32, _C.QK_NORM_WEIGHT_F32, 1e-6
    a.cos, a.sin, a.P, a.weight[0] = 4096, 8192, 16, 1 << 16
    t = a.t[0]
    t.src, t.dst, t.H = 512, 1 << 20, 8
    t.src_batch, t.src_row, t.src_head = t.dst_batch, t.dst_row, t.dst_head = 6 * 8 * 32, 8 * 32, 32
    if bwd:
        g = a.g[0]
        g.dout, g.dout_batch, g.dout_row, g.dout_head = 1 << 22, 6 * 8 * 32, 8 * 32, 32
        a.dweight[0], a.workspace, a.workspace_bytes = 1 << 24, 1 << 26, 1 << 20
    for k, v in kw.items():
        if k[:2] in ("t_", "g_"):
            setattr(a.t[0] if k[0] == "t" else a.g[0], k[2:], v)
        elif k in ("weight", "dweight"):
            getattr(a, k)[0] = v
        else:
            setattr(a, k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    from ring_flash_attn import _C      # past every host check a call would launch: every case stops at the check it names
    lib = _C.load()
    assert lib.rfa_qk_token_norm_rotary_fwd(None, None) == ERR_NULL == lib.rfa_qk_token_norm_rotary_bwd(None, None)
    assert lib.rfa_qk_token_norm_rotary_bwd_workspace_bytes(None) == 0
    inf, nan = float("inf"), float("nan")
    shared = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(ntensors=0), dict(ntensors=3), dict(interleaved=2), dict(t_pad=1),
                   dict(eps=-1e-6), dict(eps=inf), dict(eps=nan), dict(weight_offset=inf), dict(weight_offset=nan), dict(t_dst=512),
                   dict(pos_batch=-1), dict(pos_stride=-1), dict(pos_split=6), dict(pos_offset=11), dict(P=5), dict(pos_offset=1 << 62)],
        ERR_DTYPE: [dict(dtype=2), dict(table_dtype=1), dict(table_dtype=3), dict(weight_dtype=1), dict(dtype=1, weight_dtype=0)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(R=-16), dict(R=24), dict(interleaved=1, R=12), dict(rot_offset=4),
                       dict(rot_offset=8), dict(R=0, rot_offset=40)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(P=0), dict(B=2 ** 16, S=2 ** 15)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2), dict(t_H=513), dict(t_H=2 ** 30), dict(D=256, R=0, t_H=65)],   # H D > 16384
        ERR_NULL: [dict(cos=None), dict(sin=None), dict(t_src=None), dict(t_dst=None), dict(weight=None)],
        ERR_ALIGN: [dict(cos=4100), dict(t_src=520), dict(t_dst=(1 << 20) + 8), dict(weight=(1 << 16) + 8), dict(t_src_row=8 * 32 + 4),
                    dict(t_src_head=36), dict(t_dst_batch=3)],
    }
    only_bwd = {ERR_NULL: [dict(g_dout=None), dict(workspace=None)],
                ERR_ALIGN: [dict(g_dout=(1 << 22) + 8), dict(g_dout_row=8 * 32 + 4), dict(dweight=(1 << 24) + 2), dict(workspace=(1 << 26) + 8)],
                ERR_ARGS: [dict(t_dst=1 << 22), dict(workspace_bytes=0), dict(workspace_bytes=3 * 256 * 4 - 1)]}
    for bwd, fn in ((False, lib.rfa_qk_token_norm_rotary_fwd), (True, lib.rfa_qk_token_norm_rotary_bwd)):
        call = lambda **kw: fn(C.byref(_args(bwd, **kw)), None)
        for want, cases in list(shared.items()) + (list(only_bwd.items()) if bwd else []):
            for kw in cases:
                assert call(**kw) == want, (bwd, want, kw)
        # the order: the struct's size first, a dtype before a head dim, a shape, the heads, a NULL, the alignment, the rest
        order = [dict(struct_bytes=8), dict(dtype=2), dict(D=12), dict(B=-1), dict(t_H=513), dict(cos=None),
                 dict(t_src=520), dict(t_dst=512)]
        for first, later in zip(order, order[1:]):
            assert call(**first, **later) == call(**first) != call(**later), (first, later)
        # no rows: nothing is launched and no pointer is needed; the norm alone looks at no table, position or map
        assert call(B=0, cos=None, t_src=None, weight=None) == OK == call(S=0, sin=None, t_dst=None, pos_split=3)
        assert call(R=0, cos=None, sin=None, P=0, pos_stride=-1, pos_split=99, t_src=None) == ERR_NULL
        a = _args(bwd, ntensors=2)                              # a second tensor is checked like the first
        a.t[1].src, a.t[1].dst, a.t[1].H = 512, 1024, 0
        assert fn(C.byref(a), None) == ERR_HEADS
    # the workspace: per tensor min(ceil(rows / slots), 512) partials of H D floats — 12 rows of 256 columns: 3 workgroups of 4
    size = lambda **kw: lib.rfa_qk_token_norm_rotary_bwd_workspace_bytes(C.byref(_args(True, **kw)))
    assert size() == 3 * 256 * 4 == size(cos=None, t_src=None, dweight=None, workspace=None, pos_offset=99)
    assert size(t_H=64) == 6 * 2048 * 4 and size(D=256, R=0, t_H=64) == 12 * 16384 * 4          # teams of 128 and 256 lanes
    assert size(B=1, S=2 ** 20) == 512 * 256 * 4 and size(D=12) == 0 == size(B=0)                # capped; refused; no rows


def test_the_public_refusals_come_before_a_launch():
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _qknorm_backend import QkNormBackend

    class Serves(QkNormBackend):                                 # (no token-norm methods: a launch would be an AttributeError)
        serves_qk_token_norm = True

    q, k = torch.zeros(2, 12, 4, 64, dtype=torch.bfloat16), torch.zeros(2, 12, 2, 64, dtype=torch.bfloat16)
    wq, wk, cos, sin = torch.ones(256), torch.ones(2, 64), torch.ones(64, 16), torch.zeros(64, 16)
    base = dict(q=q, k=k, q_weight=wq, k_weight=wk, cos=cos, sin=sin)
    call = lambda f, **kw: (lambda a: f(a.pop("q"), a.pop("k"), a.pop("q_weight"), a.pop("k_weight"), a.pop("cos"), a.pop("sin"), **a))(dict(base, **kw))
    try:
        _testing.set_backend(Serves(serves=("mask_shift",)))
        value = [dict(q_weight=torch.ones(64)), dict(q_weight=torch.ones(64, 4)), dict(k_weight=torch.ones(256)), dict(q_weight=wq.double()),
                 dict(q_weight=wq.bfloat16()), dict(q_weight=torch.ones(512)[::2]), dict(q_weight=[1.0] * 256), dict(k=None),
                 dict(k_weight=None), dict(cos=None), dict(sin=None), dict(layout=R.ring_flash_attn_func, q=q[0], k=k[0]),
                 dict(q=torch.zeros(1, 2, 65, 256, dtype=torch.bfloat16), k=None, k_weight=None, q_weight=torch.ones(65 * 256), cos=None, sin=None),
                 dict(eps=-1.0), dict(rot_offset=40), dict(positions=torch.arange(12))]
        for kw in value:
            with pytest.raises(ValueError):
                call(R.apply_qk_token_norm_rotary, **kw)
        for kw in (dict(layout=R.ring_flash_attn_varlen_func), dict(layout=R.llama3_flash_attn_varlen_func), dict(inplace=True)):
            with pytest.raises(TypeError):
                call(R.apply_qk_token_norm_rotary, **kw)
        with pytest.raises(ValueError, match="weights must be"):                          # the per-head call is unchanged
            call(R.apply_qk_norm_rotary)
        _testing.set_backend(QkNormBackend(serves=("mask_shift",)))
        with pytest.raises(NotImplementedError, match="serves `qk_token_norm`"):
            call(R.apply_qk_token_norm_rotary)
    finally:
        _testing.set_backend(None)
