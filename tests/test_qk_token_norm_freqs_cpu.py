"""ring_flash_attn.apply_qk_token_norm_rotary_freqs without a device: the C ABI of rfa_qk_token_norm_rotary_freqs_fwd / _bwd
(layout against a compiled C probe, the export set, every argument check in the header's order with pointers that are never
dereferenced, the workspace size) and the public refusals.  The kernels add no index arithmetic to csrc/rfa_qktoken_index.h."""
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

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
PROBED = ["struct_bytes", "naxes", "t", "weight", "inv_freq", "scaling", "freq_axis", "positions", "pos_axis", "pos_offset2"]
PROBED_BWD = PROBED + ["g", "dweight", "workspace_bytes"]
NAMES = {"rfa_qk_token_norm_rotary_freqs" + n for n in ("_fwd", "_bwd", "_bwd_workspace_bytes")}


def test_structs_match_the_c_layout_and_the_three_name_sets_agree(built):
    from ring_flash_attn import _C

    F, Bw = _C.QkTokenNormRotaryFreqsArgs, _C.QkTokenNormRotaryFreqsBwdArgs
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu %zu\\n", sizeof(rfa_qk_token_norm_rotary_freqs_args), sizeof(rfa_qk_token_norm_rotary_freqs_bwd_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_token_norm_rotary_freqs_args, {f}));\n' for f in PROBED) + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_qk_token_norm_rotary_freqs_bwd_args, {f}));\n' for f in PROBED_BWD) + \
           "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(F), C.sizeof(Bw)] + [getattr(F, f).offset for f in PROBED] + [getattr(Bw, f).offset for f in PROBED_BWD]
    assert F().struct_bytes == C.sizeof(F) and Bw().struct_bytes == C.sizeof(Bw)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40      # the ABI stays
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert NAMES <= set(_C.SYMBOLS) and {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)
    assert all(f"{n}(" in header for n in NAMES)


def _args(bwd=False, **kw):
    """B 2, S 6, H 8, D 32: N = 256, one wave a row, 4 rows a workgroup, 3 partials of 256 floats"""
    from ring_flash_attn import _C

    a = (_C.QkTokenNormRotaryFreqsBwdArgs if bwd else _C.QkTokenNormRotaryFreqsArgs)()
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
    for k, v in kw.items():                                    # t_* / g_*: of tensor 0; axisN: freq_axis[N]; else the struct's
        if k.startswith("axis"):
            a.freq_axis[int(k[4:])] = v
        elif k in ("weight", "dweight"):
            getattr(a, k)[0] = v
        else:
            setattr(*((a.t[0], k[2:]) if k.startswith("t_") else (a.g[0], k[2:]) if k.startswith("g_") else (a, k)), v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read_and_the_workspace_size(built):
    """Past every host check a call would launch, so every case stops at the check it names.  The token call's fault (a width
    above the limit) and the freqs call's (scaling, naxes, axis codes, pos_axis, the 2^31 - 1 map) return those calls' codes."""
    from ring_flash_attn import _C

    lib = _C.load()
    assert lib.rfa_qk_token_norm_rotary_freqs_fwd(None, None) == ERR_NULL == lib.rfa_qk_token_norm_rotary_freqs_bwd(None, None)
    assert lib.rfa_qk_token_norm_rotary_freqs_bwd_workspace_bytes(None) == 0
    inf, nan = float("inf"), float("nan")
    shared = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(ntensors=3), dict(interleaved=2), dict(t_pad=1), dict(pad=1),
                   dict(naxes=0), dict(naxes=5), dict(scaling=0.0), dict(scaling=nan), dict(eps=-1e-6), dict(weight_offset=inf),
                   dict(axis0=1), dict(naxes=2, axis0=2), dict(axis0=1 << 32), dict(axis1=1), dict(t_dst=512), dict(pos_batch=-1),
                   dict(pos_axis=-1), dict(pos_stride=-1), dict(pos_split=6), dict(pos_offset=-1), dict(pos_offset=2 ** 31 - 5),
                   dict(positions=64, pos_offset=-(1 << 41)), dict(naxes=2), dict(pos_split=3, pos_offset2=2 ** 31 - 2)],
        ERR_DTYPE: [dict(dtype=2), dict(weight_dtype=1), dict(weight_dtype=3), dict(dtype=1, weight_dtype=0)],
        ERR_HEAD_DIM: [dict(D=12), dict(D=264), dict(R=0), dict(R=24), dict(interleaved=1, R=12), dict(R=16, rot_offset=24)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(B=2 ** 16, S=2 ** 15)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2), dict(t_H=513), dict(D=256, R=16, t_H=65), dict(t_H=2 ** 30)],
        ERR_NULL: [dict(inv_freq=None), dict(t_src=None), dict(t_dst=None), dict(weight=None)],
        ERR_ALIGN: [dict(inv_freq=4098), dict(t_src=520), dict(weight=(1 << 16) + 8), dict(t_src_row=8 * 32 + 4), dict(t_dst_batch=3)],
    }
    only_bwd = {
        ERR_NULL: [dict(g_dout=None), dict(workspace=None)],
        ERR_ALIGN: [dict(g_dout=(1 << 22) + 8), dict(dweight=(1 << 24) + 2), dict(workspace=(1 << 26) + 8)],
        ERR_ARGS: [dict(t_dst=1 << 22), dict(workspace_bytes=0), dict(workspace_bytes=3 * 256 * 4 - 1)],
    }
    for bwd, fn in ((False, lib.rfa_qk_token_norm_rotary_freqs_fwd), (True, lib.rfa_qk_token_norm_rotary_freqs_bwd)):
        call = lambda **kw: fn(C.byref(_args(bwd, **kw)), None)
        for want, cases in shared.items():
            for kw in cases:
                assert call(**kw) == want, (bwd, want, kw)
        assert call(struct_bytes=8, naxes=9) == ERR_ARGS and call(scaling=nan, dtype=2) == ERR_ARGS
        assert call(dtype=2, D=12) == ERR_DTYPE and call(D=12, B=-1) == ERR_HEAD_DIM and call(B=-1, t_H=0) == ERR_SHAPE
        assert call(t_H=513, axis0=1) == ERR_HEADS and call(axis0=1, inv_freq=None) == ERR_ARGS
        assert call(inv_freq=None, t_src=520) == ERR_NULL and call(t_src=520, t_dst=512) == ERR_ALIGN == call(inv_freq=4098, pos_stride=-1)
        # no rows: nothing is launched and no pointer is needed; the map is not looked at either — the axis codes are
        assert call(B=0, inv_freq=None, t_src=None, t_dst=None, weight=None) == OK and call(S=0, axis0=1) == ERR_ARGS
        assert call(positions=64, pos_stride=-1, pos_split=99, naxes=3, axis0=0b100100, inv_freq=None) == ERR_NULL
    call = lambda **kw: lib.rfa_qk_token_norm_rotary_freqs_bwd(C.byref(_args(True, **kw)), None)
    for want, cases in only_bwd.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    assert call(dweight=None, workspace=None, workspace_bytes=0, pos_offset=-1) == ERR_ARGS
    # the workspace: per tensor min(ceil(B S / rows per workgroup), 512) partials of H D floats, whatever the pointers or positions
    size = lambda **kw: lib.rfa_qk_token_norm_rotary_freqs_bwd_workspace_bytes(C.byref(_args(True, **kw)))
    assert size() == 3 * 256 * 4 == size(inv_freq=None, t_src=None, dweight=None, workspace=None, pos_offset=-99)
    assert size(B=1, S=8) == 2 * 256 * 4 and size(B=1, S=9) == 3 * 256 * 4                 # N <= 1024: 4 rows a workgroup
    assert size(t_H=64) == 6 * 2048 * 4 and size(t_H=512) == 12 * 16384 * 4                # 2 rows, 1 row
    assert size(B=1, S=4096) == 512 * 256 * 4 == size(B=2 ** 4, S=2 ** 20)                 # capped at 512 partials
    two = _args(True, ntensors=2)
    two.t[1].H = 64
    assert lib.rfa_qk_token_norm_rotary_freqs_bwd_workspace_bytes(C.byref(two)) == size() + size(t_H=64)
    assert size(D=12) == 0 and size(reserved=1) == 0 and size(B=0) == 0 and size(naxes=5) == 0 and size(axis0=1) == 0 == size(t_H=513)


def test_every_refusal_comes_before_a_launch(single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _rotary_backend import RotaryBackend

    launched = []

    class Served(RotaryBackend):
        serves_qk_token_norm_freqs = True

        def qk_token_norm_freqs_rotary_fwd(self, xs, outs, *a, **kw):
            launched.append(kw)
            for o in outs:
                o.zero_()

    q, k, wide = torch.randn(2, 12, 4, 64).bfloat16(), torch.randn(2, 12, 2, 64).bfloat16(), torch.zeros(1, 2, 65, 256).bfloat16()
    wq, wk, inv, ar = torch.ones(256), torch.ones(2, 64), torch.rand(16), torch.arange(12, dtype=torch.int32)
    thw, axes = torch.stack([ar, ar, ar]), [0] * 6 + [1] * 5 + [2] * 5
    value = [
        (dict(q_weight=torch.ones(64)), "weights must be"), (dict(q_weight=wq.double()), "weights must be"),
        (dict(k_weight=wk.bfloat16()), "weights must be"), (dict(k_weight=torch.ones(64, 2)), "weights must be"),
        (dict(q=wide, k=None, q_weight=torch.ones(65 * 256), k_weight=None), "more than the 16384 columns"),
        (dict(k_weight=None), "k and k_weight"), (dict(eps=-1e-6), "eps"), (dict(weight_offset=float("inf")), "weight_offset"),
        (dict(q=q.float()), "bf16"), (dict(inv_freq=inv.double()), "inv_freq must be"), (dict(inv_freq=inv[:12]), "multiple of 16"),
        (dict(inv_freq=torch.rand(40)), "rot_offset"), (dict(rot_offset=4), "rot_offset"), (dict(attention_scaling=0.0), "attention_scaling"),
        (dict(layout=R.ring_flash_attn_func, positions=ar), "at most one"), (dict(positions=ar.long()), "int32"),
        (dict(offset=-1), "positions -1 .. 10"), (dict(offset=2 ** 31 - 5), "outside 0 .. 2"), (dict(positions=ar, offset=2 ** 31), "offset"),
        (dict(freq_axis=axes), "with freq_axis, positions"), (dict(freq_axis=[3] + axes[1:], positions=thw), "freq_axis must name axes"),
        (dict(freq_axis=axes, positions=torch.stack([ar] * 5)), "with freq_axis, positions"),
        (dict(freq_axis=axes, positions=thw, layout=R.ring_flash_attn_func), "one position per row"),
    ]
    _testing.set_backend(Served(serves=("mask_shift",)))
    try:
        for kw, match in value:
            a = dict(dict(q=q, k=k, q_weight=wq, k_weight=wk, inv_freq=inv), **kw)
            with pytest.raises(ValueError, match=match):
                R.apply_qk_token_norm_rotary_freqs(a.pop("q"), a.pop("k"), a.pop("q_weight"), a.pop("k_weight"), a.pop("inv_freq"), **a)
        for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.ring_flash_attn_varlen_func):
            with pytest.raises(TypeError):
                R.apply_qk_token_norm_rotary_freqs(q, k, wq, wk, inv, layout=notf)
        assert not launched                                                            # nothing was launched
        R.apply_qk_token_norm_rotary_freqs(q, k, wq, wk, inv, layout=R.zigzag_ring_flash_attn_func, attention_scaling=2, rot_offset=16)
        R.apply_qk_token_norm_rotary_freqs(q, None, wq, None, inv, positions=thw, freq_axis=axes, offset=3, weight_offset=1.0)
        assert launched[0] == dict(positions=None, scaling=2.0, freq_axis=None, pos_map=(0, (1, 6, 6)), interleaved=False, rot_offset=16, eps=1e-6, weight_offset=0.0)
        assert launched[1]["positions"] is thw and launched[1]["freq_axis"] == tuple(axes) and launched[1]["pos_map"][0] == 3
        _testing.set_backend(RotaryBackend(serves=("mask_shift",)))
        with pytest.raises(NotImplementedError, match="serves `qk_token_norm_freqs`"):
            R.apply_qk_token_norm_rotary_freqs(q, k, wq, wk, inv)
    finally:
        _testing.set_backend(None)
    assert "apply_qk_token_norm_rotary_freqs" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21
