"""Rotary embedding with the angles formed in the kernel (ring_flash_attn.apply_rotary_freqs), no device: the tile / unit
arithmetic of csrc/rfa_rotfreq_index.h (a stand-alone C++ program under ASan / UBSan), the C ABI of rfa_rotary_freqs (layout
against a compiled C probe, every argument check in the header's order with pointers that are never dereferenced), what
HipBackend.rotary_freqs writes into the struct, and the refusals of the public function."""
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
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")
FIELDS = ["ntensors", "B", "S", "D", "dtype", "R", "rot_offset", "interleaved", "conj", "naxes", "t", "inv_freq", "scaling", "pad",
          "freq_axis", "positions", "pos_batch", "pos_axis", "pos_offset", "pos_stride", "pos_split", "pos_offset2"]


def test_tile_and_unit_arithmetic_host_check_under_asan_and_ubsan():
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rotfreq_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "rotfreq_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "660 configurations ok" in res.stdout, res.stdout


def test_struct_matches_the_c_layout_and_the_abi_stays(built):
    from ring_flash_attn import _C

    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu\\n", sizeof(rfa_rotary_freqs_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_rotary_freqs_args, {f}));\n' for f in FIELDS) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _C.RotaryFreqsArgs
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in FIELDS]
    assert [f for f, _ in A._fields_] == ["struct_bytes", "reserved"] + FIELDS and A().struct_bytes == C.sizeof(A)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1
    assert "rfa_rotary_freqs" in _C.SYMBOLS


def _args(**kw):
    from ring_flash_attn import _C

    a = _C.RotaryFreqsArgs()
    a.ntensors, a.B, a.S, a.D, a.dtype, a.R, a.rot_offset, a.naxes, a.scaling = 1, 2, 6, 32, 0, 32, 0, 1, 1.0
    a.inv_freq = 4096                                          # (addresses that are never dereferenced)
    t = a.t[0]
    t.src, t.dst, t.H = 512, 1 << 20, 8
    t.src_batch, t.src_row, t.src_head = 6 * 8 * 32, 8 * 32, 32
    t.dst_batch, t.dst_row, t.dst_head = 6 * 8 * 32, 8 * 32, 32
    for k, v in kw.items():
        if k.startswith("t_"):
            setattr(a.t[0], k[2:], v)
        elif k.startswith("axis"):
            a.freq_axis[int(k[4:])] = v
        else:
            setattr(a, k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    """Past every host check a call would launch, so every case stops at the check it names; none passes them all."""
    from ring_flash_attn import _C

    lib = _C.load()
    call = lambda **kw: lib.rfa_rotary_freqs(C.byref(_args(**kw)), None)
    assert lib.rfa_rotary_freqs(None, None) == ERR_NULL
    size = C.sizeof(_C.RotaryFreqsArgs)
    inf, nan = float("inf"), float("nan")
    bad = {
        ERR_ARGS: [dict(struct_bytes=size - 8), dict(struct_bytes=C.sizeof(_C.RotaryArgs)), dict(reserved=1), dict(ntensors=0),
                   dict(ntensors=3), dict(interleaved=2), dict(conj=-1), dict(t_pad=1), dict(pad=1), dict(naxes=0), dict(naxes=5),
                   dict(scaling=0.0), dict(scaling=-1.0), dict(scaling=inf), dict(scaling=nan),
                   dict(axis0=1), dict(naxes=2, axis0=2), dict(naxes=3, positions=64, axis0=3 << 30), dict(axis0=1 << 32),
                   dict(naxes=4, positions=64, axis1=1), dict(axis3=1 << 63),
                   dict(t_dst=512, t_dst_row=8 * 32 + 8), dict(pos_batch=-1), dict(pos_axis=-1), dict(naxes=2),
                   dict(pos_offset=1 << 41), dict(positions=64, pos_offset=-(1 << 41)),
                   dict(pos_stride=-1), dict(pos_split=6), dict(pos_split=-1), dict(pos_offset=-1), dict(pos_offset=2 ** 31 - 5),
                   dict(pos_stride=2 ** 29), dict(pos_split=3, pos_offset2=2 ** 31 - 2), dict(pos_split=3, pos_offset2=-1)],
        ERR_DTYPE: [dict(dtype=2), dict(dtype=-1)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(R=0), dict(R=24), dict(R=48), dict(interleaved=1, R=12),
                       dict(rot_offset=4), dict(rot_offset=-8), dict(rot_offset=8), dict(R=16, rot_offset=24)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, t_H=2),
                    dict(B=2 ** 14, S=2 ** 13, t_H=4, D=64, R=16)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2)],
        ERR_NULL: [dict(inv_freq=None), dict(t_src=None), dict(t_dst=None)],
        ERR_ALIGN: [dict(inv_freq=4098), dict(t_src=520), dict(t_dst=(1 << 20) + 8), dict(t_src_row=8 * 32 + 4),
                    dict(t_src_batch=6 * 8 * 32 + 2), dict(t_src_head=36), dict(t_dst_row=8 * 32 + 4), dict(t_dst_head=36)],
    }
    for want, cases in bad.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # the order of the header: size, flags, naxes and scaling before a dtype, a dtype before a head dim, ... the axis codes
    # behind the unit count and in front of "no rows", a NULL before an alignment, an alignment before the positions
    assert call(struct_bytes=8, dtype=2) == ERR_ARGS
    assert call(naxes=5, dtype=2) == ERR_ARGS and call(scaling=nan, dtype=2) == ERR_ARGS
    assert call(dtype=2, D=12) == ERR_DTYPE
    assert call(D=12, B=-1) == ERR_HEAD_DIM
    assert call(B=-1, t_H=0) == ERR_SHAPE
    assert call(t_H=0, axis0=1) == ERR_HEADS
    assert call(B=2 ** 15, S=2 ** 15, t_H=2, axis0=1) == ERR_SHAPE
    assert call(axis0=1, B=0) == ERR_ARGS
    assert call(inv_freq=None, t_src=520) == ERR_NULL
    assert call(t_src=520, pos_stride=-1) == ERR_ALIGN and call(inv_freq=4098, naxes=2) == ERR_ALIGN
    # no rows: nothing is launched and no pointer is needed
    assert call(B=0, inv_freq=None, t_src=None, t_dst=None) == OK
    assert call(S=0, inv_freq=None, t_src=None, t_dst=None, pos_split=3, naxes=2) == OK
    # a 4-byte aligned inv_freq is enough; the last axis code that counts is entry R/2 - 1
    assert call(inv_freq=4100, t_src=None) == ERR_NULL
    assert call(naxes=4, positions=64, axis0=0xFFFFFFFF, t_src=None) == ERR_NULL
    assert call(R=16, naxes=4, positions=64, axis0=0xFFFF, t_src=None) == ERR_NULL
    assert call(R=16, naxes=4, positions=64, axis0=0x1FFFF) == ERR_ARGS
    # with `positions` the map's fields are not looked at and any int32 may come: nothing bounds them
    assert call(positions=64, pos_stride=-1, pos_split=99, t_src=None) == ERR_NULL


def test_what_the_backend_writes_into_the_struct(built, monkeypatch):
    """HipBackend.rotary_freqs on CPU tensors with the library replaced by a recorder"""
    from ring_flash_attn import _C, backend
    from ring_flash_attn._common import zigzag_map

    seen = []

    class Lib:
        def rfa_rotary_freqs(self, a, s):
            seen.append(_C.RotaryFreqsArgs.from_buffer_copy(a._obj))
            return 0

    monkeypatch.setattr(backend, "_stream", lambda t: None)
    monkeypatch.setattr(backend.HipBackend, "_check_dev", staticmethod(lambda *ts: None))
    be = object.__new__(backend.HipBackend)
    be.lib = Lib()
    qkv = torch.zeros(2, 6, 3, 4, 64, dtype=torch.float16)
    q, k = qkv[:, :, 0], qkv[:, :, 1, :2]
    oq, ok = torch.empty(2, 6, 4, 64, dtype=torch.float16), torch.empty(2, 6, 2, 64, dtype=torch.float16)
    inv = torch.ones(16)
    # (S,) positions, an offset, both tensors, interleaved
    pos = torch.zeros(6, dtype=torch.int32)
    be.rotary_freqs([q, k], [oq, ok], inv, scaling=1.25, positions=pos, pos_map=(5, (1, 0, 0)), interleaved=True, rot_offset=8, conj=True)
    a = seen[-1]
    assert (a.struct_bytes, a.reserved, a.ntensors, a.B, a.S, a.D, a.dtype) == (C.sizeof(_C.RotaryFreqsArgs), 0, 2, 2, 6, 64, 1)
    assert (a.R, a.rot_offset, a.interleaved, a.conj, a.naxes, a.pad) == (32, 8, 1, 1, 1, 0)
    assert (a.inv_freq, a.scaling, list(a.freq_axis)) == (inv.data_ptr(), 1.25, [0, 0, 0, 0])
    t0, t1 = a.t[0], a.t[1]
    assert (t0.src, t0.dst, t0.H, t0.pad) == (q.data_ptr(), oq.data_ptr(), 4, 0) and (t1.src, t1.dst, t1.H) == (k.data_ptr(), ok.data_ptr(), 2)
    assert (t0.src_batch, t0.src_row, t0.src_head) == (6 * 768, 768, 64) == (t1.src_batch, t1.src_row, t1.src_head)
    assert (t0.dst_batch, t0.dst_row, t0.dst_head) == (6 * 256, 256, 64) and (t1.dst_batch, t1.dst_row, t1.dst_head) == (6 * 128, 128, 64)
    assert (a.positions, a.pos_batch, a.pos_axis, a.pos_offset, a.pos_stride, a.pos_split, a.pos_offset2) == (pos.data_ptr(), 0, 0, 5, 0, 0, 0)
    # (B, S) positions
    pos2 = torch.zeros(2, 6, dtype=torch.int32)
    be.rotary_freqs([q], [oq], inv, positions=pos2)
    a = seen[-1]
    assert (a.ntensors, a.naxes, a.positions, a.pos_batch, a.pos_axis, a.pos_offset, a.scaling, a.conj) == (1, 1, pos2.data_ptr(), 6, 0, 0, 1.0, 0)
    # (A, B, S) positions with an axis list: frequency c in bits 2c, 2c + 1
    pos3 = torch.zeros(3, 2, 6, dtype=torch.int32)
    inv48 = torch.ones(48)
    q96, o96 = torch.zeros(2, 6, 1, 96, dtype=torch.bfloat16), torch.empty(2, 6, 1, 96, dtype=torch.bfloat16)
    axes = [c % 3 for c in range(48)]
    be.rotary_freqs([q96], [o96], inv48, freq_axis=axes, positions=pos3)
    a = seen[-1]
    assert (a.R, a.naxes, a.positions, a.pos_batch, a.pos_axis, a.dtype) == (96, 3, pos3.data_ptr(), 6, 12, 0)
    assert list(a.freq_axis) == [sum(axes[c] << (2 * c) for c in range(32)), sum(axes[32 + c] << (2 * c) for c in range(16)), 0, 0]
    # (A, T) positions, packed input
    x, dx = torch.zeros(7, 3, 64, dtype=torch.float16), torch.empty(7, 3, 64, dtype=torch.float16)
    pos4 = torch.zeros(2, 7, dtype=torch.int32)
    be.rotary_freqs([x], [dx], inv, freq_axis=[1] * 16, positions=pos4)
    a = seen[-1]
    assert (a.B, a.S, a.naxes, a.pos_batch, a.pos_axis, a.freq_axis[0]) == (1, 7, 2, 0, 7, 0x55555555)
    assert (a.t[0].src_batch, a.t[0].src_row, a.t[0].src_head) == (0, 192, 64)
    # a zigzag layout: the map's four numbers, no tensor
    be.rotary_freqs([q], [oq], inv, pos_map=zigzag_map(1, 4, 3))
    a = seen[-1]
    assert (a.positions, a.naxes, a.pos_offset, a.pos_stride, a.pos_split, a.pos_offset2) == (None, 1, 3, 1, 3, 18)


class _Recorder:
    name = "recorder"
    serves_rotary_freqs = True

    def __init__(self):
        self.calls = []

    def rotary_freqs(self, srcs, dsts, inv_freq, **kw):
        self.calls.append(kw)
        for s, d in zip(srcs, dsts):
            if d is not s:
                d.copy_(s)


@pytest.fixture
def recorder():
    from ring_flash_attn import _testing

    be = _Recorder()
    _testing.set_backend(be)
    yield be
    _testing.set_backend(None)


_Q = torch.zeros(2, 12, 4, 64, dtype=torch.bfloat16)
_K = torch.zeros(2, 12, 2, 64, dtype=torch.bfloat16)
_INV = torch.ones(16)
_AR = torch.arange(12, dtype=torch.int32)
_THW = torch.zeros(3, 2, 12, dtype=torch.int32)
_AX = [0, 1, 2, 0] * 4
REFUSALS = [
    (dict(q=_Q.float()), "bf16"), (dict(q=_Q[..., :60]), "head dim"), (dict(k=_K[:, :6]), "k must share"), (dict(q=None), "tensors"),
    (dict(inv_freq=None), "inv_freq"), (dict(inv_freq=_INV.double()), "inv_freq"), (dict(inv_freq=_INV.view(1, 16)), "inv_freq"),
    (dict(inv_freq=torch.ones(32)[::2]), "inv_freq"), (dict(inv_freq=torch.ones(12)), "multiple of 16"),
    (dict(inv_freq=torch.ones(6), interleaved=True), "multiple of 8"), (dict(inv_freq=torch.ones(0)), "positive multiple"),
    (dict(inv_freq=torch.ones(40)), r"rot_offset \+ R"),
    (dict(attention_scaling=0.0), "attention_scaling"), (dict(attention_scaling=-1.0), "attention_scaling"),
    (dict(attention_scaling=float("inf")), "attention_scaling"), (dict(attention_scaling=float("nan")), "attention_scaling"),
    (dict(attention_scaling="1"), "attention_scaling"),
    (dict(rot_offset=4), "rot_offset"), (dict(rot_offset=40), "rot_offset"), (dict(rot_offset=-8), "rot_offset"),
    (dict(positions=_AR, layout="ring"), "at most one"), (dict(positions=_AR.long()), "int32"), (dict(positions=_AR[:5]), "int32"),
    (dict(positions=_THW), "int32"), (dict(offset=-1), "positions -1 .. 10"), (dict(offset=2 ** 31 - 11), "outside 0 .. 2"),
    (dict(layout="zigzag", q=_Q[:, :11], k=_K[:, :11]), "odd"), (dict(layout="ring", q=_Q[0], k=_K[0]), r"needs \(B, S, H, D\)"),
    (dict(inplace=True, q=_Q[..., 1:57], k=None, inv_freq=torch.ones(8)), "inplace=True needs"),
    (dict(freq_axis=_AX), "with freq_axis, positions"), (dict(freq_axis=_AX, layout="ring"), "one position per row"),
    (dict(freq_axis=_AX, positions=_AR), "with freq_axis, positions"), (dict(freq_axis=_AX, positions=_THW.long()), "with freq_axis"),
    (dict(freq_axis=_AX, positions=_THW[:, :, :6]), "with freq_axis"), (dict(freq_axis=_AX, positions=_THW.transpose(0, 1)), "with freq_axis"),
    (dict(freq_axis=_AX, positions=torch.zeros(5, 2, 12, dtype=torch.int32)), "with freq_axis"),
    (dict(freq_axis=_AX[:15], positions=_THW), "R/2 = 16 ints"), (dict(freq_axis=[0.0] * 16, positions=_THW), "R/2 = 16 ints"),
    (dict(freq_axis=torch.zeros(16), positions=_THW), "CPU int tensor"), (dict(freq_axis=[0] * 15 + [3], positions=_THW), r"axes in \[0, 3\)"),
    (dict(freq_axis=[0] * 15 + [-1], positions=_THW), r"axes in \[0, 3\)"),
    (dict(positions=_AR, offset=2 ** 41), "offset"), (dict(freq_axis=_AX, positions=_THW, offset=-2 ** 41), "offset"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"case{i}" for i in range(len(REFUSALS))])
def test_every_refusal_comes_before_a_launch(recorder, single_rank_group, kw, match):
    import ring_flash_attn as R

    layouts = {"ring": R.ring_flash_attn_func, "zigzag": R.zigzag_ring_flash_attn_func}
    a = dict(dict(q=_Q, k=_K, inv_freq=_INV), **kw)
    if "layout" in a:
        a["layout"] = layouts[a["layout"]]
    with pytest.raises(ValueError, match=match):
        R.apply_rotary_freqs(a.pop("q"), a.pop("k"), a.pop("inv_freq"), **a)
    assert not recorder.calls


def test_type_errors_the_missing_flag_and_what_is_served(recorder, single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _usp_backend import UspBackend

    for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.llama3_flash_attn_varlen_func):
        with pytest.raises(TypeError):
            R.apply_rotary_freqs(_Q, _K, _INV, layout=notf)
        with pytest.raises(TypeError):
            R.apply_rotary_freqs(_Q, _K, _INV, layout=notf, freq_axis=_AX, positions=_THW)
    assert not recorder.calls
    # served: a layout as the map's numbers, an axis list as a tuple beside (A, B, S) positions, a CPU int tensor likewise;
    # the backward is the same launch with conj on the gradients, and inv_freq gets none
    q = _Q.clone().requires_grad_(True)
    inv = _INV.clone().requires_grad_(True)
    out = R.apply_rotary_freqs(q, None, inv, layout=R.zigzag_ring_flash_attn_func, offset=3, attention_scaling=2)
    out.sum().backward()
    assert [c["conj"] for c in recorder.calls] == [False, True] and inv.grad is None and q.grad is not None
    assert all(c["positions"] is None and c["pos_map"] == (3, (1, 6, 9)) and c["scaling"] == 2.0 for c in recorder.calls)
    R.apply_rotary_freqs(_Q, _K, _INV, freq_axis=torch.tensor(_AX), positions=_THW, offset=1)
    c = recorder.calls[-1]
    assert c["freq_axis"] == tuple(_AX) and c["positions"].data_ptr() == _THW.data_ptr() and c["pos_map"][0] == 1
    _testing.set_backend(UspBackend(serves=("mask_shift",)))
    with pytest.raises(NotImplementedError, match="serves `rotary_freqs`"):
        R.apply_rotary_freqs(_Q, _K, _INV)
    assert "apply_rotary_freqs" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21
