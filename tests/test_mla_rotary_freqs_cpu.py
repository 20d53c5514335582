"""ring_flash_attn.apply_mla_rotary_freqs without a device: the C ABI of rfa_mla_rotary_freqs_fwd / _bwd (layout, every argument
check in the header's order, pointers never dereferenced) and the public refusals and hand-over on a stub backend.  The kernel
needs no index arithmetic beyond rfa_mlarope_index.h and rfa_rotfreq_index.h, whose host checks other files run."""
import ctypes as C
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

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
HEAD = ["B", "S", "dtype", "Dn", "Dr", "Dv", "H", "Hq", "interleaved", "pad0"]
TAIL = ["inv_freq", "scaling", "pad", "positions", "pos_batch", "pos_offset", "pos_stride", "pos_split", "pos_offset2"]
TENSORS = {"MlaRotaryFreqsArgs": ["q", "q_out", "kv", "k_pe", "k", "v"], "MlaRotaryFreqsBwdArgs": ["dq_out", "dq", "dk", "dv", "dkv", "dk_pe"]}
C_NAME = {"MlaRotaryFreqsArgs": "rfa_mla_rotary_freqs_args", "MlaRotaryFreqsBwdArgs": "rfa_mla_rotary_freqs_bwd_args"}
FN = {"MlaRotaryFreqsArgs": "rfa_mla_rotary_freqs_fwd", "MlaRotaryFreqsBwdArgs": "rfa_mla_rotary_freqs_bwd"}


@pytest.mark.parametrize("cls", sorted(TENSORS))
def test_structs_match_the_c_layout_and_the_symbols_are_bound(built, cls):
    from ring_flash_attn import _C

    fields = HEAD + TENSORS[cls] + TAIL
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           f'  printf("%zu\\n", sizeof({C_NAME[cls]}));\n' + \
           "".join(f'  printf("%zu\\n", offsetof({C_NAME[cls]}, {f}));\n' for f in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = getattr(_C, cls)
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields]
    assert [f for f, _ in A._fields_] == ["struct_bytes", "reserved"] + fields and A().struct_bytes == C.sizeof(A)
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1
    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    assert FN[cls] in _C.SYMBOLS and f"int {FN[cls]}(" in header and hasattr(lib, FN[cls])


def _args(cls, **kw):
    """a call that passes every check (addresses that are never dereferenced): B 2, S 6, H 4, Hq 3, Dn 16, Dr 32, Dv 24"""
    from ring_flash_attn import _C

    a = getattr(_C, cls)()
    a.B, a.S, a.dtype, a.Dn, a.Dr, a.Dv, a.H, a.Hq, a.scaling, a.inv_freq = 2, 6, 0, 16, 32, 24, 4, 3, 1.25, 4096
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


@pytest.mark.parametrize("cls", sorted(TENSORS))
def test_every_argument_check_returns_before_a_pointer_is_read(built, cls):
    """Past every host check a call would launch, so every case stops at the check it names; none passes them all."""
    from ring_flash_attn import _C

    lib, fn = _C.load(), FN[cls]
    call = lambda **kw: getattr(lib, fn)(C.byref(_args(cls, **kw)), None)
    assert getattr(lib, fn)(None, None) == ERR_NULL
    fwd = cls == "MlaRotaryFreqsArgs"
    qs, qd, kk, vv, kvn, pe = ("q", "q_out", "k", "v", "kv", "k_pe") if fwd else ("dq_out", "dq", "dk", "dv", "dkv", "dk_pe")
    null = lambda *names: {f"{n}__ptr": None for n in names}
    big = 2 ** 31 - 1
    bad = {
        ERR_ARGS: [dict(struct_bytes=8), dict(reserved=1), dict(interleaved=2), dict(pad0=1), dict(pad=1), dict(scaling=0.0),
                   dict(scaling=-1.0), dict(scaling=math.inf), dict(scaling=math.nan), dict(pos_batch=-1), dict(pos_stride=-1),
                   dict(pos_split=6), dict(pos_offset=-1), dict(pos_offset=big - 4), dict(pos_split=3, pos_offset2=big - 1),
                   dict(pos_offset=1 << 41), dict(positions=64, pos_offset=-(1 << 41))],
        ERR_DTYPE: [dict(dtype=2), dict(dtype=-1)],
        ERR_HEAD_DIM: [dict(Dn=-8), dict(Dn=12), dict(Dr=0), dict(Dr=24), dict(interleaved=1, Dr=12), dict(Dv=0), dict(Dv=12),
                       dict(Dv=264), dict(Dn=232), dict(Dn=0, Dr=272)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, H=2),
                    dict(B=2 ** 15, S=2 ** 14, H=1, Hq=4), dict(B=2 ** 14, S=2 ** 13, H=2, Hq=0)],
        ERR_HEADS: [dict(H=0), dict(Hq=-1)],
        ERR_NULL: [dict(inv_freq=None), null(qs), null(qd)] +
                  ([null(kvn), null(pe), null(kk), null(vv)] if fwd else [null(kk, vv), null(kk), dict(Hq=0, **null(kvn, pe))]),
        ERR_ALIGN: [dict(inv_freq=4098)] + [{f"{n}__{f}": v} for n in (qs, qd, kk, vv, kvn, pe) for f, v in (("ptr", 520), ("row", 196), ("batch", 1154))] +
                   [{f"{n}__head": 36} for n in (qs, qd, kk, vv, kvn)],
    }
    for want, cases in bad.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # the header's order: struct, scaling, dtype, dims, shape, heads, unit count, "no rows", NULL, alignment, positions
    assert call(reserved=1, dtype=2) == ERR_ARGS and call(scaling=0.0, dtype=2) == ERR_ARGS and call(dtype=2, Dn=12) == ERR_DTYPE
    assert call(Dn=12, B=-1) == ERR_HEAD_DIM and call(B=-1, H=0) == ERR_SHAPE and call(H=0, B=2 ** 15, S=2 ** 15) == ERR_HEADS
    assert call(B=2 ** 15, S=2 ** 15, H=2, inv_freq=None) == ERR_SHAPE
    assert call(inv_freq=None, **{f"{kk}__row": 196}) == ERR_NULL and call(inv_freq=4098, pos_stride=-1) == ERR_ALIGN
    # no rows: nothing is launched and no pointer is needed; without q its tensors are not looked at
    assert call(B=0, inv_freq=None, **null(qs, qd, kk, vv, kvn, pe)) == OK and call(S=0, pos_split=3) == OK
    assert call(Hq=0, pos_stride=-1, **{f"{qs}__ptr": None, f"{qd}__row": 3}) == ERR_ARGS
    if not fwd:                                               # a gradient that did not arrive: what is left still checks out
        assert call(pos_stride=-1, **null(vv)) == ERR_ARGS and call(pos_stride=-1, **null(kk, pe)) == ERR_ARGS


class _Stub:
    name = "stub"
    serves_mla_rotary_freqs = True

    def __init__(self):
        self.calls = []

    def mla_rotary_freqs_fwd(self, *tensors, **kw):
        self.calls.append(("fwd", tensors, kw))

    def mla_rotary_freqs_bwd(self, *tensors, **kw):
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
_IF = torch.ones(16)
_AR = torch.arange(12, dtype=torch.int32)
REFUSALS = [
    (dict(kv=None), "tensors"), (dict(inv_freq=None), "inv_freq must be"), (dict(inv_freq=_IF.view(4, 4)), "inv_freq must be"),
    (dict(inv_freq=_IF.double()), "inv_freq must be"), (dict(kv=_KV.float()), "bf16"), (dict(kv=_KV[0, 0]), "kv must be"),
    (dict(q=_Q.half()), "q must share"), (dict(nope_dim=24), "disagrees"), (dict(q=None), "nope_dim"),
    (dict(q=None, nope_dim=12), "multiples of 8"), (dict(q=_Q[..., :28]), "multiples of 8"), (dict(k_pe=_PE[:, :6]), "k_pe must be"),
    (dict(inv_freq=_IF[:12].contiguous(), q=None, nope_dim=16, k_pe=_PE[..., :24]), "multiple of 16"),
    (dict(attention_scaling=0.0), "attention_scaling"), (dict(attention_scaling=math.nan), "attention_scaling"),
    (dict(attention_scaling=True), "attention_scaling"), (dict(positions=_AR, layout="ring"), "at most one"),
    (dict(positions=_AR.long()), "int32"), (dict(offset=-1), "outside 0 .. 2"), (dict(layout="zigzag", offset=2 ** 31 - 11), "outside 0 .. 2"),
    (dict(positions=_AR, offset=2 ** 31), "offset"), (dict(layout="ring", q=_Q[0], kv=_KV[0], k_pe=_PE[0]), r"needs \(B, S, H, D\)"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"case{i}" for i in range(len(REFUSALS))])
def test_every_refusal_comes_before_a_launch(stub, single_rank_group, kw, match):
    import ring_flash_attn as R

    a = dict(dict(q=_Q, kv=_KV, k_pe=_PE, inv_freq=_IF), **kw)
    if "layout" in a:
        a["layout"] = {"ring": R.ring_flash_attn_func, "zigzag": R.zigzag_ring_flash_attn_func}[a["layout"]]
    with pytest.raises(ValueError, match=match):
        R.apply_mla_rotary_freqs(a.pop("q"), a.pop("kv"), a.pop("k_pe"), a.pop("inv_freq"), **a)
    assert not stub.calls


def test_type_errors_the_missing_flag_and_what_reaches_the_backend(stub, single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing

    for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.llama3_flash_attn_varlen_func):
        with pytest.raises(TypeError):
            R.apply_mla_rotary_freqs(_Q, _KV, _PE, _IF, layout=notf)
    assert not stub.calls
    # served: a layout as the map's numbers; the backward gets exactly the gradients that arrived, for the inputs that want one
    q, kv, pe = _Q.clone().requires_grad_(True), _KV.clone().requires_grad_(True), _PE[:, :, 0].clone()
    qo, k, v = R.apply_mla_rotary_freqs(q, kv, pe, _IF, attention_scaling=1.5, layout=R.zigzag_ring_flash_attn_func, offset=3,
                                        interleaved=True)
    kind, tensors, kw = stub.calls[-1]
    assert kind == "fwd" and tensors[-1].data_ptr() == _IF.data_ptr() and len(tensors) == 7
    assert kw == dict(nope_dim=16, positions=None, scaling=1.5, pos_map=(3, (1, 6, 9)), interleaved=True)
    assert (qo.shape, k.shape, v.shape) == (q.shape, (2, 12, 4, 48), (2, 12, 4, 24)) and all(t.is_contiguous() for t in (qo, k, v))
    (qo.sum() + v.sum()).backward()
    kind, (dq_out, dq, dk, dv, dkv, dk_pe, inv_freq), kw = stub.calls[-1]
    assert kind == "bwd" and dq_out is not None and dq is not None and dk is None and dv is not None and dk_pe is None
    assert dkv.shape == kv.shape and not dkv.any() and inv_freq.data_ptr() == _IF.data_ptr() and pe.grad is None
    assert (kw["nope_dim"], kw["v_dim"], kw["heads"], kw["scaling"], kw["pos_map"]) == (16, 24, 4, 1.5, (3, (1, 6, 9)))
    assert R.apply_mla_rotary_freqs(None, _KV, _PE, _IF, nope_dim=16, positions=_AR)[0] is None and stub.calls[-1][1][0] is None
    assert stub.calls[-1][2]["positions"] is not None and stub.calls[-1][2]["scaling"] == 1.0
    _testing.set_backend(type("Plain", (), {"name": "plain", "serves_mla_rotary": True})())
    with pytest.raises(NotImplementedError, match="serves `mla_rotary_freqs`"):
        R.apply_mla_rotary_freqs(_Q, _KV, _PE, _IF)
    assert "apply_mla_rotary_freqs" in dir(R) and len([n for n in dir(R) if n.endswith("_func")]) == 21
