"""ring_flash_attn.apply_mla_rotary without a device: csrc/rfa_mlarope_index.h under ASan / UBSan, the C ABI of rfa_mla_rotary_fwd /
_bwd (layout, every argument check in the header's order, pointers never dereferenced), the public refusals on a stub backend."""
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
HEAD = ["B", "S", "dtype", "Dn", "Dr", "Dv", "H", "Hq", "interleaved", "table_dtype"]
TAIL = ["cos", "sin", "P", "positions", "pos_batch", "pos_offset", "pos_stride", "pos_split", "pos_offset2"]
TENSORS = {"MlaRotaryArgs": ["q", "q_out", "kv", "k_pe", "k", "v"], "MlaRotaryBwdArgs": ["dq_out", "dq", "dk", "dv", "dkv", "dk_pe"]}
C_NAME = {"MlaRotaryArgs": "rfa_mla_rotary_args", "MlaRotaryBwdArgs": "rfa_mla_rotary_bwd_args"}


def test_tile_unit_and_head_sum_arithmetic_host_check_under_asan_and_ubsan():
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "mlarope_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "mlarope_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "224 configurations ok" in res.stdout, res.stdout


@pytest.mark.parametrize("cls", sorted(TENSORS))
def test_structs_match_the_c_layout_and_the_symbols_are_bound(built, cls):
    from ring_flash_attn import _C

    fields = HEAD + TENSORS[cls] + TAIL
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           f'  printf("%zu %zu\\n", sizeof({C_NAME[cls]}), sizeof(rfa_mla_rotary_tensor));\n' + \
           "".join(f'  printf("%zu\\n", offsetof({C_NAME[cls]}, {f}));\n' for f in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = getattr(_C, cls)
    assert got == [C.sizeof(A), C.sizeof(_C.MlaRotaryTensor)] + [getattr(A, f).offset for f in fields]
    assert [f for f, _ in A._fields_] == ["struct_bytes", "reserved"] + fields and A().struct_bytes == C.sizeof(A)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    for name in ("rfa_mla_rotary_fwd", "rfa_mla_rotary_bwd"):
        assert name in _C.SYMBOLS and f"int {name}(" in header and hasattr(lib, name)


def _args(cls, **kw):
    """a call that passes every check (addresses that are never dereferenced): B 2, S 6, H 4, Hq 3, Dn 16, Dr 32, Dv 24"""
    from ring_flash_attn import _C

    a = getattr(_C, cls)()
    a.B, a.S, a.dtype, a.Dn, a.Dr, a.Dv, a.H, a.Hq, a.P = 2, 6, 0, 16, 32, 24, 4, 3, 16
    a.cos, a.sin = 4096, 8192
    widths = dict(q=(3, 48), q_out=(3, 48), kv=(4, 40), k_pe=(1, 32), k=(4, 48), v=(4, 24))
    roles = dict(zip(TENSORS[cls], ("q", "q_out", "k", "v", "kv", "k_pe") if cls.endswith("BwdArgs") else TENSORS[cls]))
    for n, (name, role) in enumerate(roles.items()):
        t, (h, w) = getattr(a, name), widths[role]
        t.ptr, t.batch, t.row, t.head = (n + 1) << 20, 6 * h * w, h * w, 0 if role == "k_pe" else w
    for k, v in kw.items():
        if "__" in k:
            setattr(getattr(a, k.split("__")[0]), k.split("__")[1], v)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("cls,fn", [("MlaRotaryArgs", "rfa_mla_rotary_fwd"), ("MlaRotaryBwdArgs", "rfa_mla_rotary_bwd")])
def test_every_argument_check_returns_before_a_pointer_is_read(built, cls, fn):
    """Past every host check a call would launch, so every case stops at the check it names; none passes them all."""
    from ring_flash_attn import _C

    lib = _C.load()
    call = lambda **kw: getattr(lib, fn)(C.byref(_args(cls, **kw)), None)
    assert getattr(lib, fn)(None, None) == ERR_NULL
    fwd = cls == "MlaRotaryArgs"
    qs, qd, kk, vv, kvn, pe = ("q", "q_out", "k", "v", "kv", "k_pe") if fwd else ("dq_out", "dq", "dk", "dv", "dkv", "dk_pe")
    null = lambda *names: {f"{n}__ptr": None for n in names}
    bad = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(interleaved=2), dict(pos_batch=-1), dict(pos_stride=-1), dict(pos_split=6),
                   dict(pos_offset=-1), dict(pos_offset=11), dict(P=5), dict(pos_split=3, pos_offset2=14), dict(pos_offset=1 << 41)],
        ERR_DTYPE: [dict(dtype=2), dict(table_dtype=1), dict(table_dtype=3)],
        ERR_HEAD_DIM: [dict(Dn=-8), dict(Dn=12), dict(Dr=0), dict(Dr=24), dict(interleaved=1, Dr=12), dict(Dv=0), dict(Dv=12),
                       dict(Dv=264), dict(Dn=232), dict(Dn=0, Dr=272)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(P=0), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, H=2),
                    dict(B=2 ** 15, S=2 ** 14, H=1, Hq=4), dict(B=2 ** 14, S=2 ** 13, H=2, Hq=0)],
        ERR_HEADS: [dict(H=0), dict(Hq=-1)],
        ERR_NULL: [dict(cos=None), dict(sin=None), null(qs), null(qd)] +
                  ([null(kvn), null(pe), null(kk), null(vv)] if fwd else [null(kk, vv), null(kk), dict(Hq=0, **null(kvn, pe))]),
        ERR_ALIGN: [dict(cos=4104)] + [{f"{n}__{f}": v} for n in (qs, qd, kk, vv, kvn, pe) for f, v in (("ptr", 520), ("row", 196), ("batch", 1154))] +
                   [{f"{n}__head": 36} for n in (qs, qd, kk, vv, kvn)],
    }
    for want, cases in bad.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # the header's order: struct, dtype, dims, shape, heads, unit count, "no rows", NULL, alignment, positions
    assert call(reserved=1, dtype=2) == ERR_ARGS and call(dtype=2, Dn=12) == ERR_DTYPE and call(Dn=12, B=-1) == ERR_HEAD_DIM
    assert call(B=-1, H=0) == ERR_SHAPE and call(H=0, B=2 ** 15, S=2 ** 15) == ERR_HEADS
    assert call(B=2 ** 15, S=2 ** 15, H=2, cos=None) == ERR_SHAPE
    assert call(cos=None, sin=8200) == ERR_NULL and call(sin=8200, pos_stride=-1) == ERR_ALIGN
    # no rows: nothing is launched and no pointer is needed; without q its tensors are not looked at
    assert call(B=0, cos=None, **null(qs, qd, kk, vv, kvn, pe)) == OK and call(S=0, sin=None, pos_split=3) == OK
    assert call(Hq=0, pos_stride=-1, **{f"{qs}__ptr": None, f"{qd}__row": 3}) == ERR_ARGS
    if not fwd:                                               # a gradient that did not arrive: what is left still checks out
        assert call(pos_stride=-1, **null(vv)) == ERR_ARGS and call(pos_stride=-1, **null(kk, pe)) == ERR_ARGS
        assert call(pos_stride=-1, Hq=0, **null(qs, qd, vv, kvn)) == ERR_ARGS


class _Stub:
    name = "stub"
    serves_mla_rotary = True

    def __init__(self):
        self.calls = []

    def mla_rotary_fwd(self, *tensors, **kw):
        self.calls.append(("fwd", tensors, kw))

    def mla_rotary_bwd(self, *tensors, **kw):
        self.calls.append(("bwd", tensors, kw))


@pytest.fixture
def stub():
    from ring_flash_attn import _testing

    be = _Stub()
    _testing.set_backend(be)
    yield be
    _testing.set_backend(None)


_Q = torch.zeros(2, 12, 3, 48, dtype=torch.bfloat16)
_KV = torch.zeros(2, 12, 4, 40, dtype=torch.bfloat16)
_PE = torch.zeros(2, 12, 1, 32, dtype=torch.bfloat16)
_COS = torch.ones(16, 16)
_AR = torch.arange(12, dtype=torch.int32)
REFUSALS = [
    (dict(kv=None), "tensors"), (dict(cos=_COS[0]), "cos and sin"), (dict(kv=_KV.float()), "bf16"), (dict(kv=_KV[0, 0]), "kv must be"),
    (dict(q=_Q.half()), "q must share"), (dict(q=_Q[:, :6]), "q must share"), (dict(nope_dim=24), "disagrees"), (dict(q=None), "nope_dim"),
    (dict(q=None, nope_dim=12), "multiples of 8"), (dict(q=None, nope_dim=40), "multiples of 8"), (dict(q=_Q[..., :28]), "multiples of 8"),
    (dict(k_pe=_PE[:, :6]), "k_pe must be"), (dict(k_pe=_PE.half()), "k_pe must be"), (dict(k_pe=_PE.expand(2, 12, 4, 32)), "k_pe must be"),
    (dict(cos=_COS[:, :12].contiguous(), sin=_COS[:, :12].contiguous(), q=None, nope_dim=16, k_pe=_PE[..., :24]), "multiple of 16"),
    (dict(positions=_AR, layout="ring"), "at most one"), (dict(positions=_AR.long()), "int32"), (dict(offset=5), "positions 5 .. 16"),
    (dict(layout="zigzag", offset=9), "the tables have 16"), (dict(layout="ring", q=_Q[0], kv=_KV[0], k_pe=_PE[0]), r"needs \(B, S, H, D\)"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"case{i}" for i in range(len(REFUSALS))])
def test_every_refusal_comes_before_a_launch(stub, single_rank_group, kw, match):
    import ring_flash_attn as R

    a = dict(dict(q=_Q, kv=_KV, k_pe=_PE, cos=_COS, sin=_COS), **kw)
    if "layout" in a:
        a["layout"] = {"ring": R.ring_flash_attn_func, "zigzag": R.zigzag_ring_flash_attn_func}[a["layout"]]
    with pytest.raises(ValueError, match=match):
        R.apply_mla_rotary(a.pop("q"), a.pop("kv"), a.pop("k_pe"), a.pop("cos"), a.pop("sin"), **a)
    assert not stub.calls


def test_type_errors_the_missing_flag_and_what_reaches_the_backend(stub, single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing

    for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.llama3_flash_attn_varlen_func):
        with pytest.raises(TypeError):
            R.apply_mla_rotary(_Q, _KV, _PE, _COS, _COS, layout=notf)
    assert not stub.calls
    # served: a layout as the map's numbers; the backward gets exactly the gradients that arrived, for the inputs that want one
    q, kv, pe = _Q.clone().requires_grad_(True), _KV.clone().requires_grad_(True), _PE[:, :, 0].clone()
    qo, k, v = R.apply_mla_rotary(q, kv, pe, _COS, _COS, layout=R.zigzag_ring_flash_attn_func, offset=3, interleaved=True)
    kw = stub.calls[-1][2]
    assert kw["pos_map"] == (3, (1, 6, 9)) and kw["nope_dim"] == 16 and kw["interleaved"] and kw["positions"] is None
    assert (qo.shape, k.shape, v.shape) == (q.shape, (2, 12, 4, 48), (2, 12, 4, 24)) and all(t.is_contiguous() for t in (qo, k, v))
    (qo.sum() + v.sum()).backward()
    kind, (dq_out, dq, dk, dv, dkv, dk_pe, _, _), kw = stub.calls[-1]
    assert kind == "bwd" and dq_out is not None and dq is not None and dk is None and dv is not None and dk_pe is None
    assert dkv.shape == kv.shape and not dkv.any() and (kw["nope_dim"], kw["v_dim"], kw["heads"]) == (16, 24, 4) and pe.grad is None
    assert R.apply_mla_rotary(None, _KV, _PE, _COS, _COS, nope_dim=16, positions=_AR)[0] is None and stub.calls[-1][1][0] is None
    _testing.set_backend(type("Plain", (), {"name": "plain"})())
    with pytest.raises(NotImplementedError, match="serves `mla_rotary`"):
        R.apply_mla_rotary(_Q, _KV, _PE, _COS, _COS)
    assert "apply_mla_rotary" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21
