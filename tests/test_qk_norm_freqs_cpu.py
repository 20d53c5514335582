"""Per-head QK RMSNorm fused with a rotation whose angles the kernel forms (ring_flash_attn.apply_qk_norm_rotary_freqs), no
device: the tile / item / LDS arithmetic of csrc/rfa_qknormfreq_index.h (a stand-alone C++ program under ASan / UBSan), the C
ABI of rfa_qk_norm_rotary_freqs_fwd / _bwd (layout against a compiled C probe, the export set, every argument check in the
header's order with pointers that are never dereferenced, the workspace size) and the refusals of the public function."""
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
HEAD = ["ntensors", "B", "S", "D", "dtype", "R", "rot_offset", "interleaved", "naxes", "weight_dtype", "eps", "weight_offset", "t",
        "weight", "inv_freq", "scaling", "pad", "freq_axis", "positions", "pos_batch", "pos_axis", "pos_offset", "pos_stride",
        "pos_split", "pos_offset2"]
TAIL = ["g", "dweight", "workspace", "workspace_bytes"]
NAMES = {"rfa_qk_norm_rotary_freqs_fwd", "rfa_qk_norm_rotary_freqs_bwd", "rfa_qk_norm_rotary_freqs_bwd_workspace_bytes"}


def test_index_functions_host_check_under_asan_and_ubsan():
    """tests/native/qknormfreq_check.cpp on the very header the kernels include: every (row, head, chunk) of q and k visited
    once by the forward's tiles and by the backward's walk, every LDS read on the entry the angle phase wrote"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "qknormfreq_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "qknormfreq_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "305 configurations ok" in res.stdout, res.stdout


def test_structs_match_the_c_layout_and_the_three_name_sets_agree(built):
    from ring_flash_attn import _C

    F, Bw = _C.QkNormRotaryFreqsArgs, _C.QkNormRotaryFreqsBwdArgs
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu %zu %d\\n", sizeof(rfa_qk_norm_rotary_freqs_args), sizeof(rfa_qk_norm_rotary_freqs_bwd_args), ' \
           'RFA_QK_NORM_FREQS_TILE_ROWS);\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_norm_rotary_freqs_args, {f}));\n' for f in HEAD) + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_norm_rotary_freqs_bwd_args, {f}));\n' for f in HEAD + TAIL) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [C.sizeof(F), C.sizeof(Bw), _C.QK_NORM_FREQS_TILE_ROWS]
    assert got[3:] == [getattr(F, f).offset for f in HEAD] + [getattr(Bw, f).offset for f in HEAD + TAIL]
    assert [f for f, _ in F._fields_] == ["struct_bytes", "reserved"] + HEAD
    assert [f for f, _ in Bw._fields_] == ["struct_bytes", "reserved"] + HEAD + TAIL
    assert F().struct_bytes == C.sizeof(F) and Bw().struct_bytes == C.sizeof(Bw)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40      # the ABI stays
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert NAMES <= set(_C.SYMBOLS) and {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)
    assert all(f"{n}(" in header for n in NAMES)


def _args(bwd=False, **kw):
    from ring_flash_attn import _C

    a = (_C.QkNormRotaryFreqsBwdArgs if bwd else _C.QkNormRotaryFreqsArgs)()
    a.ntensors, a.B, a.S, a.D, a.dtype, a.R, a.rot_offset, a.naxes, a.scaling = 1, 2, 6, 32, 0, 32, 0, 1, 1.0
    a.weight_dtype, a.eps = _C.QK_NORM_WEIGHT_F32, 1e-6
    a.inv_freq = 4096                                          # (addresses that are never dereferenced)
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
        elif k.startswith("axis"):
            a.freq_axis[int(k[4:])] = v
        elif k in ("weight", "dweight"):
            getattr(a, k)[0] = v
        else:
            setattr(a, k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    """Past every host check a call would launch, so every case below stops at the check it names; none passes them all."""
    from ring_flash_attn import _C

    lib = _C.load()
    assert lib.rfa_qk_norm_rotary_freqs_fwd(None, None) == ERR_NULL and lib.rfa_qk_norm_rotary_freqs_bwd(None, None) == ERR_NULL
    assert lib.rfa_qk_norm_rotary_freqs_bwd_workspace_bytes(None) == 0
    inf, nan = float("inf"), float("nan")
    shared = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(ntensors=0), dict(ntensors=3), dict(interleaved=2), dict(t_pad=1),
                   dict(pad=1), dict(naxes=0), dict(naxes=5), dict(scaling=0.0), dict(scaling=-1.0), dict(scaling=inf),
                   dict(scaling=nan), dict(eps=-1e-6), dict(eps=inf), dict(eps=nan), dict(weight_offset=inf), dict(weight_offset=nan),
                   dict(axis0=1), dict(naxes=2, axis0=2), dict(axis0=1 << 32), dict(axis1=1), dict(naxes=4, axis3=3),
                   dict(t_dst=512), dict(pos_batch=-1), dict(pos_axis=-1), dict(pos_stride=-1), dict(pos_split=6), dict(pos_split=-1),
                   dict(pos_offset=-1), dict(pos_offset=2 ** 31 - 5), dict(pos_offset=1 << 41), dict(positions=64, pos_offset=-(1 << 41)),
                   dict(naxes=2), dict(pos_split=3, pos_offset2=2 ** 31 - 2)],
        ERR_DTYPE: [dict(dtype=2), dict(dtype=-1), dict(weight_dtype=1), dict(weight_dtype=3), dict(dtype=1, weight_dtype=0)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(R=0), dict(R=-16), dict(R=24), dict(R=48), dict(interleaved=1, R=12),
                       dict(rot_offset=4), dict(rot_offset=-8), dict(rot_offset=8), dict(R=16, rot_offset=24)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, t_H=2), dict(B=1, S=1, t_H=2 ** 30)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2)],
        ERR_NULL: [dict(inv_freq=None), dict(t_src=None), dict(t_dst=None), dict(weight=None)],
        ERR_ALIGN: [dict(inv_freq=4098), dict(t_src=520), dict(t_dst=(1 << 20) + 8), dict(weight=(1 << 16) + 8),
                    dict(t_src_row=8 * 32 + 4), dict(t_src_batch=6 * 8 * 32 + 2), dict(t_src_head=36), dict(t_dst_row=8 * 32 + 4),
                    dict(t_dst_batch=3), dict(t_dst_head=36)],
    }
    only_bwd = {
        ERR_NULL: [dict(g_dout=None), dict(workspace=None)],
        ERR_ALIGN: [dict(g_dout=(1 << 22) + 8), dict(g_dout_row=8 * 32 + 4), dict(g_dout_head=36), dict(g_dout_batch=2),
                    dict(dweight=(1 << 24) + 2), dict(workspace=(1 << 26) + 8)],
        ERR_ARGS: [dict(t_dst=1 << 22), dict(workspace_bytes=0), dict(workspace_bytes=4 * 32 * 4 - 1)],
    }
    for bwd, fn in ((False, lib.rfa_qk_norm_rotary_freqs_fwd), (True, lib.rfa_qk_norm_rotary_freqs_bwd)):
        call = lambda **kw: fn(C.byref(_args(bwd, **kw)), None)
        for want, cases in shared.items():
            for kw in cases:
                assert call(**kw) == want, (bwd, want, kw)
        # the order: the struct's size first, flags, scaling and eps before a dtype, a dtype before a head dim, ...
        assert call(struct_bytes=8, naxes=9) == ERR_ARGS and call(scaling=nan, dtype=2) == ERR_ARGS
        assert call(dtype=2, D=12) == ERR_DTYPE and call(weight_dtype=1, D=12) == ERR_DTYPE
        assert call(D=12, B=-1) == ERR_HEAD_DIM and call(B=-1, t_H=0) == ERR_SHAPE and call(t_H=0, axis0=1) == ERR_HEADS
        assert call(B=1, S=1, t_H=2 ** 30, axis0=1) == ERR_SHAPE and call(axis0=1, inv_freq=None) == ERR_ARGS
        assert call(inv_freq=None, t_src=520) == ERR_NULL and call(t_src=520, t_dst=512) == ERR_ALIGN
        assert call(inv_freq=4098, pos_stride=-1) == ERR_ALIGN
        # no rows: nothing is launched and no pointer is needed; the map is not looked at either — the axis codes are
        assert call(B=0, inv_freq=None, t_src=None, t_dst=None, weight=None) == OK
        assert call(S=0, inv_freq=None, t_src=None, t_dst=None, pos_split=3) == OK and call(S=0, axis0=1) == ERR_ARGS
        # with `positions` the map's fields are not looked at, and several axes are served
        assert call(positions=64, pos_stride=-1, pos_split=99, naxes=3, axis0=0b100100, inv_freq=None) == ERR_NULL
    call = lambda **kw: lib.rfa_qk_norm_rotary_freqs_bwd(C.byref(_args(True, **kw)), None)
    for want, cases in only_bwd.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # without a dweight neither the workspace nor its size is looked at: the call gets as far as the last check
    assert call(dweight=None, workspace=None, workspace_bytes=0, pos_offset=-1) == ERR_ARGS


def test_workspace_size_is_a_function_of_the_shapes_alone(built):
    """ntensors * min(B * ceil(S / 4), 1024) partials of D floats — whatever the heads, the pointers or the positions"""
    from ring_flash_attn import _C

    lib = _C.load()
    size = lambda **kw: lib.rfa_qk_norm_rotary_freqs_bwd_workspace_bytes(C.byref(_args(True, **kw)))
    assert size() == 2 * 2 * 32 * 4 == size(inv_freq=None, t_src=None, dweight=None, workspace=None, pos_offset=-99, t_H=77)
    assert size(B=1, S=8) == 2 * 32 * 4 and size(B=1, S=9) == 3 * 32 * 4 and size(B=3, S=9) == 9 * 32 * 4
    assert size(B=1, S=4096) == 1024 * 32 * 4 == size(B=2 ** 4, S=2 ** 20)              # capped at 1024 partials
    two = _args(True, ntensors=2)
    two.t[1].H = 3
    assert lib.rfa_qk_norm_rotary_freqs_bwd_workspace_bytes(C.byref(two)) == 2 * size()
    assert size(D=12) == 0 and size(reserved=1) == 0 and size(B=0) == 0 and size(naxes=5) == 0 and size(axis0=1) == 0


def test_every_refusal_comes_before_a_launch(single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _rotary_backend import RotaryBackend

    launched = []

    class Served(RotaryBackend):
        serves_qk_norm_freqs = True

        def qk_norm_freqs_rotary_fwd(self, xs, outs, *a, **kw):
            launched.append(kw)
            for o in outs:
                o.zero_()

    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(2, 12, 4, 64, generator=g).bfloat16(), torch.randn(2, 12, 2, 64, generator=g).bfloat16()
    wq, wk = torch.ones(64), torch.ones(64)
    inv = torch.rand(16, generator=g)
    ar = torch.arange(12, dtype=torch.int32)
    thw = torch.stack([ar, ar, ar])
    axes = [0] * 6 + [1] * 5 + [2] * 5
    value = [
        (dict(q_weight=wq[:32]), "weights must be"), (dict(q_weight=wq.double()), "weights must be"),
        (dict(k_weight=wk.bfloat16()), "weights must be"), (dict(q_weight=[1.0] * 64), "weights must be"),
        (dict(k=None), "k and k_weight"), (dict(k_weight=None), "k and k_weight"),
        (dict(eps=-1e-6), "eps"), (dict(eps=float("nan")), "eps"), (dict(weight_offset=float("inf")), "weight_offset"),
        (dict(q=q.float()), "bf16"), (dict(q=q[..., :60]), "head dim"), (dict(k=k[:, :6]), "k must share"),
        (dict(inv_freq=inv.double()), "inv_freq must be"), (dict(inv_freq=inv.view(1, 16)), "inv_freq must be"),
        (dict(inv_freq=None), "inv_freq must be"), (dict(inv_freq=torch.rand(32)[::2]), "inv_freq must be"),
        (dict(inv_freq=inv[:12]), "multiple of 16"), (dict(inv_freq=inv[:6], interleaved=True), "multiple of 8"),
        (dict(inv_freq=torch.rand(40)), "rot_offset"), (dict(rot_offset=4), "rot_offset"), (dict(rot_offset=40), "rot_offset"),
        (dict(attention_scaling=0.0), "attention_scaling"), (dict(attention_scaling=float("inf")), "attention_scaling"),
        (dict(attention_scaling=True), "attention_scaling"),
        (dict(layout=R.ring_flash_attn_func, positions=ar), "at most one"),
        (dict(positions=ar.long()), "int32"), (dict(positions=ar[:5]), "int32"),
        (dict(offset=-1), "positions -1 .. 10"), (dict(offset=2 ** 31 - 5), "outside 0 .. 2"),
        (dict(positions=ar, offset=2 ** 31), "offset"),
        (dict(layout=R.zigzag_ring_flash_attn_func, q=q[:, :11], k=k[:, :11]), "odd"),
        (dict(freq_axis=axes), "with freq_axis, positions"), (dict(freq_axis=axes, positions=ar), "with freq_axis, positions"),
        (dict(freq_axis=axes[:8], positions=thw), "freq_axis must hold"), (dict(freq_axis=[0.0] * 16, positions=thw), "freq_axis must hold"),
        (dict(freq_axis=[3] + axes[1:], positions=thw), "freq_axis must name axes"),
        (dict(freq_axis=axes, positions=torch.stack([ar] * 5)), "with freq_axis, positions"),
        (dict(freq_axis=axes, positions=thw, layout=R.ring_flash_attn_func), "one position per row"),
    ]
    _testing.set_backend(Served(serves=("mask_shift",)))
    try:
        for kw, match in value:
            a = dict(dict(q=q, k=k, q_weight=wq, k_weight=wk, inv_freq=inv), **kw)
            with pytest.raises(ValueError, match=match):
                R.apply_qk_norm_rotary_freqs(a.pop("q"), a.pop("k"), a.pop("q_weight"), a.pop("k_weight"), a.pop("inv_freq"), **a)
        for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.ring_flash_attn_varlen_func):
            with pytest.raises(TypeError):
                R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv, layout=notf)
        with pytest.raises(TypeError):                                                 # there is no in-place mode
            R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv, inplace=True)
        assert not launched                                                            # nothing was launched
        # what a served call hands to the backend: the map's numbers for a layout, the axes as given
        R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv, layout=R.zigzag_ring_flash_attn_func, attention_scaling=2, rot_offset=16)
        R.apply_qk_norm_rotary_freqs(q, None, wq, None, inv, positions=thw, freq_axis=axes, offset=3, weight_offset=1.0)
        assert launched[0] == dict(positions=None, scaling=2.0, freq_axis=None, pos_map=(0, (1, 6, 6)), interleaved=False,
                                   rot_offset=16, eps=1e-6, weight_offset=0.0)
        assert launched[1]["positions"] is thw and launched[1]["freq_axis"] == tuple(axes) and launched[1]["pos_map"][0] == 3
        # a backend without the flag
        _testing.set_backend(RotaryBackend(serves=("mask_shift",)))
        with pytest.raises(NotImplementedError, match="serves `qk_norm_freqs`"):
            R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv)
    finally:
        _testing.set_backend(None)
    assert "apply_qk_norm_rotary_freqs" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21
