"""Dropout over several ranks in the dense ring, zigzag and stripe schedules, no device: the position-map arithmetic
against positions written out by hand, the schedules under gloo through the public functions against ONE single-device
dropout call with the same seed (CPU oracle with position maps, tests/_ref_backend.py), what must still be refused,
and the host side of the C ABI (revision, fields, argument checks, plans)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _droppos_worker as DW                     # noqa: E402

ERR_ARGS = -8


# ---------------------------------------------------------------------------------------------- map arithmetic
def test_position_maps_against_positions_written_out_by_hand():
    from ring_flash_attn._common import dropout_arg, map_positions, pos_map, stripe_map, zigzag_map
    from _blockref import positions

    # zigzag, W = 2, 4 rows per rank (chunks of 2): rank 0 holds chunks 0 and 3, rank 1 chunks 1 and 2
    assert map_positions(zigzag_map(0, 2, 2), 4) == [0, 1, 6, 7]
    assert map_positions(zigzag_map(1, 2, 2), 4) == [2, 3, 4, 5]
    assert map_positions(zigzag_map(1, 2, 2, "front"), 2) == [2, 3]          # `k[:, :half]` of rank 1
    assert map_positions(zigzag_map(0, 2, 2, "back"), 2) == [6, 7]           # `q[:, half:]` of rank 0
    # W = 4, chunks of 101 rows: rank 1 holds chunks 1 and 6
    assert zigzag_map(1, 4, 101) == (101, (1, 101, 606))
    # stripe, W = 3, 3 rows per rank: rank 1 holds tokens 1, 4, 7; the shifted views of a step whose keys are one token ahead
    assert map_positions(stripe_map(1, 3), 3) == [1, 4, 7]
    assert map_positions(stripe_map(1, 3, skip=1), 2) == [4, 7]              # `q[:, 1:]` of rank 1
    assert map_positions(stripe_map(2, 3), 2) == [2, 5]                      # `k[:, :-1]` of rank 2
    # ring: a contiguous block is the identity map behind an offset — the 5-tuple every backend serves
    assert map_positions(pos_map(3 * 130), 3) == [390, 391, 392]
    assert dropout_arg(0.2, 7, q_map=pos_map(260), k_map=pos_map(130)) == (0.2, 7, 260, 130, 0)
    assert dropout_arg(0.2, 7, q_map=zigzag_map(1, 4, 101), k_map=zigzag_map(2, 4, 101, "front")) == \
        (0.2, 7, 101, 202, 0, (1, 101, 606), (1, 0, 0))
    assert dropout_arg(0.2, 7, q_map=stripe_map(1, 3, skip=1), k_map=stripe_map(2, 3)) == (0.2, 7, 4, 2, 0, (3, 0, 0), (3, 0, 0))
    assert dropout_arg(0.0, None, q_map=stripe_map(1, 3)) is None
    # the test backend's restatement of the formula (stride 0 reads as 1)
    assert positions(101, (1, 101, 606), 202) == list(range(101, 202)) + list(range(606, 707))
    assert positions(5, (0, 0, 0), 3) == [5, 6, 7]


def test_backend_flag_and_the_require_helper():
    from oracle.oracle_backend import OracleBackend
    from ring_flash_attn._common import require_dropout_positions
    from ring_flash_attn.backend import HipBackend
    from _ref_backend import RefBackend

    assert HipBackend.serves_dropout_positions is True
    with pytest.raises(NotImplementedError, match="position maps"):
        require_dropout_positions(OracleBackend(), "ring_flash_attn")
    require_dropout_positions(RefBackend(serves=("dropout_positions",)), "ring_flash_attn")


def test_set_dropout_fills_the_map_fields():
    from ring_flash_attn import _C
    from ring_flash_attn.backend import _set_dropout

    for st in (_C.FwdArgs, _C.BwdArgs):
        a = st()
        _set_dropout(a, (0.2, 7, 101, 202, 3, (1, 101, 606), (4, 0, 0)))
        assert (a.q_pos_offset, a.q_pos_stride, a.q_pos_split, a.q_pos_offset2) == (101, 1, 101, 606)
        assert (a.k_pos_offset, a.k_pos_stride, a.k_pos_split, a.k_pos_offset2, a.head_offset) == (202, 4, 0, 0, 3)
        b = st()
        _set_dropout(b, (0.2, 7, 101, 202, 3))                    # the 5-tuple: the map stays zero-initialised
        assert (b.q_pos_stride, b.q_pos_split, b.q_pos_offset2, b.k_pos_stride, b.k_pos_split, b.k_pos_offset2) == (0,) * 6


# ---------------------------------------------------------------------------------------------- schedules under gloo
def _cases(W):
    zz = lambda form, **kw: dict(kind="zigzag", form=form, W=W, S=202, causal=True, **kw)
    cases = [dict(kind="ring", W=W, S=130, causal=True), dict(kind="ring", W=W, S=130, causal=False),
             zz("ring"), zz("gather"), zz("gather_ps"), dict(kind="stripe", W=W, S=130, causal=True)]
    if W == 2:
        cases += [zz("gather", api="kvpacked"), dict(kind="stripe", W=W, S=130, causal=True, api="qkvpacked"),
                  dict(refusals=True)]
    return cases


_REF = {}


def _reference(c):
    """one single-device oracle call per (unsharded shape, mask): shared by every schedule that un-shards to it"""
    key = (c["W"] * c["S"], c["causal"], c.get("api") == "qkvpacked")
    if key not in _REF:
        _REF[key] = DW.reference(c)
    return _REF[key]


def _check_world(W, cases):
    res, errs = DW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs)
    for c in cases:
        if c.get("refusals"):
            continue
        name = DW.case_name(c)
        (ro, rl, rdq, rdk, rdv), r0 = _reference(c)
        out, lse, dq, dk, dv = res[name]
        assert (ro.float() - r0.float()).abs().max() > 0.05, name                      # dropout did something
        # (the bounds of test_schedules_cpu.py::test_llama3_dropout_is_consistent_across_ranks)
        assert (out.float() - ro.float()).abs().max() <= 2e-2, name
        # lse is that of the UNDROPPED softmax: fp32 on both sides, merged in fp32
        assert torch.equal(torch.isfinite(lse), torch.isfinite(rl)) and (lse - rl).abs().max() <= 1e-4, name
        for nm, got, ref in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
            d = (got.float() - ref.float()).abs().max().item()
            assert d <= 3e-2 + 1e-2 * ref.float().abs().max().item(), f"{name} {nm}: {d:.3e}"


@pytest.mark.parametrize("W", [2, 4])
def test_dropout_over_ranks_equals_the_single_device_call(W):
    """ring (causal and not), zigzag in every exchange form and stripe at W = 2 and 4, B = 2, H = 4, Hk = 2, D = 64,
    p = 0.2; zigzag with 2 x 101 rows per rank (an odd half that is no multiple of 4), 130 rows otherwise; one kv-packed
    and one qkv-packed call; at W = 2 also what must still be refused.  Fails on a tree without the feature with
    NotImplementedError."""
    _check_world(W, _cases(W))


def test_stripe_dropout_over_three_ranks():
    _check_world(3, [dict(kind="stripe", W=3, S=130, causal=True)])


def test_single_rank_calls_keep_the_five_tuple(single_rank_group):
    """a single-rank group is the identity map: the schedules hand the backend the 5-tuple, so the frozen oracle backend
    keeps serving those calls"""
    import ring_flash_attn as R
    from oracle.oracle_backend import OracleBackend
    from ring_flash_attn import _testing

    seen = []

    class Spy(OracleBackend):
        def fwd(self, *a, **kw):
            seen.append(kw.get("dropout"))
            return super().fwd(*a, **kw)

    _testing.set_backend(Spy())
    try:
        q = torch.randn(1, 64, 2, 32, generator=torch.Generator().manual_seed(1)).bfloat16()
        for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
            fn(q, q, q, dropout_p=0.3, causal=True)
        assert len(seen) == 3 and all(d is not None and len(d) == 5 for d in seen), seen
    finally:
        _testing.set_backend(None)


def test_message_of_the_varlen_refusal_names_what_works():
    from ring_flash_attn import _api

    with pytest.raises(NotImplementedError, match="dense ring, zigzag and stripe"):
        _api._check_unsupported(0.1, (-1, -1), None, windows_ok=True, dropout_ok=False)
    with pytest.raises(NotImplementedError, match="dropout together"):
        _api._check_unsupported(0.1, (4, 0), None, windows_ok=True, dropout_ok=True)
    _api._check_unsupported(0.1, (-1, -1), None, windows_ok=True, dropout_ok=True)


# ---------------------------------------------------------------------------------------------- C ABI on the host
def _lib():
    from ring_flash_attn import _C

    return _C, _C.load()


def _fwd(_C, Sq=202, Sk=202, D=128, p=0.2):
    a = _C.FwdArgs()
    a.q = a.k = a.v = a.out = a.lse = 256                        # (any non-NULL value: the checks come before any launch)
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype = 2, Sq, Sk, 4, 2, D, 0
    a.softmax_scale, a.causal, a.dropout_p, a.dropout_seed = D ** -0.5, 1, p, 11
    return a


def _bwd(_C, Sq=202, Sk=202, D=128, p=0.2):
    a = _C.BwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.total_k = 2, Sq, Sk, 4, 2, D, 0, 2 * Sk
    a.softmax_scale, a.causal, a.dropout_p, a.dropout_seed = D ** -0.5, 1, p, 11
    a.dq_acc = a.dk_acc = a.dv_acc = 256
    return a


def _plan(lib, a):
    f, n, five = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.rfa_bwd_plan(C.byref(a), C.byref(f), C.byref(n), C.byref(five))
    return rc, (f.value, n.value, five.value)


def test_abi_revision_and_fields():
    _C, lib = _lib()
    assert _C.RFA_ABI_VERSION == 8 and lib.rfa_abi_version() == 8
    assert _C.RFA_ABI_REVISION == 1 and lib.rfa_abi_revision() == 1
    assert "rfa_abi_revision" in _C.SYMBOLS
    new = [("q_pos_stride", C.c_int32), ("k_pos_stride", C.c_int32), ("q_pos_split", C.c_int32), ("k_pos_split", C.c_int32),
           ("q_pos_offset2", C.c_int64), ("k_pos_offset2", C.c_int64)]
    for st in (_C.FwdArgs, _C.BwdArgs):
        names = [f[0] for f in st._fields_]
        i = names.index("k_pos_offset")
        assert st._fields_[i + 1:i + 7] == new and names[i + 7] == "head_offset"       # next to the offsets, in rfa.h's order
        assert st._fields_[-1] == ("mask_shift_lens", C.c_int32)
    # the header declares the same fields in the same order, in both structs, and the revision
    hdr = open(os.path.join(ROOT, "include", "rfa.h")).read()
    decl = ("int64_t q_pos_offset, k_pos_offset;", "int32_t q_pos_stride, k_pos_stride;", "int32_t q_pos_split, k_pos_split;",
            "int64_t q_pos_offset2, k_pos_offset2;", "int32_t head_offset;")
    for body in (hdr[hdr.index("typedef struct {\n  /* inputs */"):hdr.index("} rfa_fwd_args;")],
                 hdr[hdr.index("} rfa_fwd_args;"):hdr.index("} rfa_bwd_args;")]):
        at = [body.index(d) for d in decl]
        assert at == sorted(at)
    assert "#define RFA_ABI_REVISION 1" in hdr and "int rfa_abi_revision(void);" in hdr


def test_load_refuses_a_library_of_another_revision(monkeypatch):
    from ring_flash_attn import _C

    class Stale:                                             # a library from before the revision: the symbol is missing
        def __getattr__(self, name):
            if name == "rfa_abi_revision":
                raise AttributeError(name)
            return lambda *a: 8

    class Other(Stale):
        def __getattr__(self, name):
            return lambda *a: 2 if name == "rfa_abi_revision" else 8

    for fake in (Stale(), Other()):
        with monkeypatch.context() as m:
            m.setattr(_C, "_lib", None)
            m.setattr(_C.C, "CDLL", lambda path, fake=fake: fake)
            with pytest.raises(RuntimeError, match="rebuild"):
                _C.load()
    assert _C.load().rfa_abi_revision() == 1


def test_position_map_argument_checks():
    _C, lib = _lib()
    fwd = lambda a: lib.rfa_fwd(C.byref(a), None)

    def both(edit, want):
        a, b = _fwd(_C), _bwd(_C)
        edit(a)
        edit(b)
        assert (fwd(a) == ERR_ARGS) == (want == ERR_ARGS), "rfa_fwd"
        assert _plan(lib, b)[0] == want, "rfa_bwd_plan"
        if want == ERR_ARGS:
            assert lib.rfa_bwd_workspace_bytes(C.byref(b)) == 0 and lib.rfa_fwd_workspace_bytes(C.byref(a), None) == 0

    def st(**kw):
        def edit(a):
            for k_, v_ in kw.items():
                setattr(a, k_, v_)
        return edit

    cu = 256                                                                 # (a non-NULL cu_seqlens pointer: never read here)
    both(st(q_pos_stride=-1), ERR_ARGS)
    both(st(k_pos_stride=-3), ERR_ARGS)
    for side, S in (("q", 202), ("k", 202)):
        both(st(**{f"{side}_pos_split": S}), ERR_ARGS)                       # a split outside [1, S - 1]
        both(st(**{f"{side}_pos_split": -1}), ERR_ARGS)
        both(st(**{f"{side}_pos_split": 300}), ERR_ARGS)
    both(st(q_pos_split=101, cu_seqlens_q=cu, cu_seqlens_k=cu), ERR_ARGS)    # a non-default map with packed input
    both(st(k_pos_stride=3, cu_seqlens_q=cu, cu_seqlens_k=cu), ERR_ARGS)
    both(st(q_pos_split=50, q_half=1), ERR_ARGS)                             # ... with half sequences
    both(st(k_pos_stride=2, k_half=2), ERR_ARGS)
    # dropout with a window: as before — refused by the calls themselves (the pure plan function never looked at it)
    a, b = _fwd(_C), _bwd(_C)
    b.dout = b.q = b.k = b.v = b.lse = b.delta = 256
    for x in (a, b):
        st(q_pos_split=101, window=1, window_left=8, window_right=0)(x)
    assert fwd(a) == ERR_ARGS and lib.rfa_bwd(C.byref(b), None) == ERR_ARGS
    both(st(q_pos_split=101, mask_shift=4), ERR_ARGS)                        # ... with a shift: as before
    both(st(q_pos_split=101, mask_shift_lens=1), ERR_ARGS)
    # valid maps plan; the fields are not read without dropout
    for edit in (st(q_pos_split=1), st(q_pos_split=201, k_pos_split=101, q_pos_offset2=606), st(q_pos_stride=3, k_pos_stride=4),
                 st(q_pos_stride=1, k_pos_stride=1), st(dropout_p=0.0, q_pos_stride=-1, k_pos_split=5000)):
        b = _bwd(_C)
        edit(b)
        assert _plan(lib, b)[0] == 0
    b = _bwd(_C)
    b.cu_seqlens_q = b.cu_seqlens_k = cu
    b.q_pos_stride = b.k_pos_stride = 1                                      # the explicit identity is a default map: packed input takes it
    assert _plan(lib, b)[0] == 0


def test_zero_map_and_explicit_identity_plan_alike():
    _C, lib = _lib()
    for D in (64, 128, 192, 256):
        for S in (202, 4096):
            a, b, c = _bwd(_C, S, S, D), _bwd(_C, S, S, D), _bwd(_C, S, S, D)
            b.q_pos_stride = b.k_pos_stride = 1
            c.q_pos_split, c.q_pos_offset2, c.k_pos_stride = S // 2, 5 * S, 3          # a real map plans the same form too
            plans = [_plan(lib, x) for x in (a, b, c)]
            assert plans[0][0] == 0 and plans[0] == plans[1] == plans[2], (D, S, plans)
            assert len({lib.rfa_bwd_workspace_bytes(C.byref(x)) for x in (a, b, c)}) == 1
            assert len({lib.rfa_bwd_ds_scratch_bytes(C.byref(x)) for x in (a, b, c)}) == 1
            fa, fb = _fwd(_C, S, S, D), _fwd(_C, S, S, D)
            fb.q_pos_stride = fb.k_pos_stride = 1
            n1, n2 = C.c_int32(), C.c_int32()
            assert lib.rfa_fwd_workspace_bytes(C.byref(fa), C.byref(n1)) == lib.rfa_fwd_workspace_bytes(C.byref(fb), C.byref(n2))
            assert n1.value == n2.value
