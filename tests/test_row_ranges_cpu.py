"""Per-row key ranges (ring_flash_attn.with_row_ranges) without a GPU: the host check of the shared clamp / skip arithmetic,
the C ABI of rfa_fwd_rr / rfa_bwd_rr, the backend's routing, every refusal of the public entry on every rank, activation
checkpointing, and the dense ring and zigzag schedules (all three exchange forms) under gloo on a CPU backend with
`serves_row_ranges` (tests/_rowrange_backend.py) against ONE single-device fp64 autograd attention with the explicit mask."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _rowrange_backend as RB                   # noqa: E402
import _rowrange_worker as RW                    # noqa: E402
import _tol                                      # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8


# ---------------------------------------------------------------------------------------------- shared arithmetic
def test_clamp_and_skip_arithmetic_against_a_brute_force_mask_under_sanitizers():
    """tests/native/rowrange_check.cpp: rr_row / rr_rel / rr_tiles / rr_touches of csrc/rfa_rowrange.h — the header the three
    kernels and the tile-bounds pre-kernel share — over small geometries, under ASan / UBSan, as a program of its own"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rowrange_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "rowrange_check.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "configurations ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays(built):
    from ring_flash_attn import _C

    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert "int rfa_fwd_rr(const rfa_fwd_args *args, const rfa_rowrange_args *rr, void *stream);" in header
    assert "int rfa_bwd_rr(const rfa_bwd_args *args, const rfa_rowrange_args *rr, void *stream);" in header
    for sym in ("rfa_fwd_rr", "rfa_bwd_rr", "rfa_rowrange_workspace_bytes"):
        assert sym in names and sym in _C.SYMBOLS
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)


def test_struct_matches_the_c_layout(built):
    from ring_flash_attn import _C

    fields = [n for n, _ in _C.RowRangeArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu\\n", sizeof(rfa_rowrange_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_rowrange_args, {n}));\n' for n in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _C.RowRangeArgs
    assert got[0] == C.sizeof(A) == 48
    assert got[1:] == [getattr(A, n).offset for n in fields] == [0, 4, 8, 16, 24, 32, 40]
    assert A().struct_bytes == 48


def _base(cls, **kw):
    a = cls()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.softmax_scale = 2, 300, 300, 4, 2, 128, 0, 0.07
    if hasattr(a, "dkdv_form"):
        from ring_flash_attn import _C

        a.dkdv_form = _C.DKDV_128
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def _rr(**kw):
    from ring_flash_attn import _C

    r = _C.RowRangeArgs()
    for n, x in kw.items():
        setattr(r, n, x)
    return r


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_every_argument_check_with_null_tensors_in_the_stated_order(built, which):
    """every tensor pointer is NULL: nothing is read, nothing is launched, no device is needed"""
    from ring_flash_attn import _C

    lib = _C.load()
    fn, cls = (lib.rfa_fwd_rr, _C.FwdArgs) if which == "fwd" else (lib.rfa_bwd_rr, _C.BwdArgs)
    run = lambda a, r: fn(C.byref(a), None if r is None else C.byref(r), None)
    assert fn(None, C.byref(_rr()), None) == ERR_NULL
    # the struct's own checks, each alone
    assert run(_base(cls), None) == ERR_ARGS
    for kw in (dict(struct_bytes=8), dict(struct_bytes=47), dict(reserved=1)):
        assert run(_base(cls), _rr(**kw)) == ERR_ARGS, kw
    # what the ranged kernels do not have, in the base arguments: dropout, packed input, halves (and, backward, another plan)
    cu = (C.c_int32 * 3)(0, 100, 300)
    cu_p = C.cast(cu, C.c_void_p).value
    for kw in (dict(dropout_p=0.1), dict(cu_seqlens_q=cu_p, cu_seqlens_k=cu_p), dict(q_half=1), dict(k_half=2)):
        assert run(_base(cls, **kw), _rr()) == ERR_ARGS, kw
    if which == "bwd":
        for kw in (dict(dkdv_form=_C.DKDV_AUTO), dict(dkdv_form=_C.DKDV_256), dict(dkdv_form=_C.DKDV_BAL), dict(ds_scratch=4096)):
            assert run(_base(cls, **kw), _rr()) == ERR_ARGS, kw
    for D in (136, 192, 256):
        assert run(_base(cls, D=D), _rr()) == ERR_HEAD_DIM, D
    assert run(_base(cls), _rr(batch_stride=-1)) == ERR_ARGS
    # a longer struct whose unknown tail is zero is accepted, one with a non-zero tail is not
    class Longer(C.Structure):
        _fields_ = [("r", _C.RowRangeArgs), ("tail", C.c_int32 * 2)]

    lo = Longer()
    lo.r = _rr(struct_bytes=56)
    as_rr = lambda: C.cast(C.pointer(lo), C.POINTER(_C.RowRangeArgs))
    assert fn(C.byref(_base(cls)), as_rr(), None) == ERR_NULL          # through to the base call's NULL tensors
    lo.tail[1] = 1
    assert fn(C.byref(_base(cls)), as_rr(), None) == ERR_ARGS
    # the order: struct (ARGS) < base combination (ARGS) < head dim (HEAD_DIM) < batch_stride (ARGS) < every base check
    assert run(_base(cls, D=192, dtype=7, dropout_p=0.5), _rr(reserved=1, batch_stride=-1)) == ERR_ARGS
    assert run(_base(cls, D=192, dtype=7), _rr(batch_stride=-1)) == ERR_HEAD_DIM
    assert run(_base(cls, dtype=7), _rr(batch_stride=-1)) == ERR_ARGS
    chain = [(dict(dtype=7), ERR_DTYPE), (dict(Hk=3), ERR_HEADS), (dict(B=-1), ERR_SHAPE), (dict(Sq=-1), ERR_SHAPE)]
    for i, (_, want) in enumerate(chain):
        kw = {}
        for later, _w in chain[i:]:
            kw.update(later)
        assert run(_base(cls, **kw), _rr()) == want, (i, kw)
    assert run(_base(cls, B=0), _rr()) == OK                           # nothing to do
    assert run(_base(cls), _rr()) == ERR_NULL                          # q, k, v ...
    for D in range(8, 129, 8):
        assert run(_base(cls, D=D), _rr()) == ERR_NULL, D
    assert run(_base(cls, D=132), _rr()) == ERR_HEAD_DIM               # (the base check: not a multiple of 8)
    # the base entry points answer as before
    base_fn = lib.rfa_fwd if which == "fwd" else lib.rfa_bwd
    assert base_fn(C.byref(_base(cls)), None) == ERR_NULL and base_fn(C.byref(_base(cls, D=260)), None) == ERR_HEAD_DIM
    if which == "bwd":
        assert lib.rfa_rowrange_workspace_bytes(C.byref(_base(cls))) == 2 * 5 * 8          # B x ceil(300 / 64) pairs of int32
        assert lib.rfa_rowrange_workspace_bytes(C.byref(_base(cls, Sq=0))) == 0
        assert lib.rfa_rowrange_workspace_bytes(None) == 0


# ---------------------------------------------------------------------------------------------- routing
class _RecLib:
    """the loaded library with a note of every function called through it; nothing is launched (no device here)"""
    NOTED = ("rfa_fwd", "rfa_fwd_ex", "rfa_fwd_vd", "rfa_fwd_rr", "rfa_bwd", "rfa_bwd_ex", "rfa_bwd_vd", "rfa_bwd_rr")

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if name in self.NOTED:
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
    return be


def _tensors(D=64, S=128, Bt=2):
    mk = lambda h: torch.zeros(Bt, S, h, D, dtype=torch.bfloat16)
    return mk(4), mk(2), mk(2)


def test_calls_without_ranges_never_reach_the_new_functions(rec_backend, monkeypatch):
    from ring_flash_attn import backend

    monkeypatch.setattr(backend, "_spill_enabled", lambda: False)
    be = rec_backend
    assert be.serves_row_ranges is True
    q, k, v = _tensors()
    out, lse = torch.empty_like(q), torch.empty(2, 4, 128)
    be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=True, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v))
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd", "rfa_bwd"]


def test_what_the_backend_puts_into_the_struct(rec_backend):
    from ring_flash_attn import _C

    be = rec_backend
    q, k, v = _tensors()
    out, lse = torch.empty_like(q), torch.empty(2, 4, 128)
    start = torch.zeros(2, 256, dtype=torch.int32)
    end = torch.full((2, 256), 77, dtype=torch.int32)
    # a schedule hands over slices: row stride 1, the batch stride of the whole tensor
    rr = (start[:, 128:], end[:, 128:], 5_000_000_000)
    be.fwd(q, k, v, softmax_scale=0.1, causal=False, out=out, lse=lse, row_ranges=rr, window=(40, -1), mask_shift=64)
    # (the tile bounds come from torch's allocator on q's device: here the CPU, nothing is launched)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=False, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v), row_ranges=rr, window=(40, -1), mask_shift=64)
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd_rr", "rfa_bwd_rr"]
    for name, (a, r, _s) in be.lib.calls:
        a, r = a._obj, r._obj
        assert r.struct_bytes == C.sizeof(_C.RowRangeArgs) == 48 and r.reserved == 0
        assert r.start == start.data_ptr() + 4 * 128 and r.end == end.data_ptr() + 4 * 128
        assert r.batch_stride == 256 and r.k_pos0 == 5_000_000_000
        assert (a.window, a.window_left, a.window_right, a.mask_shift, a.causal) == (1, 40, -1, 64, 0)
        assert (r.tile_bounds is not None and r.tile_bounds % 16 == 0) if name == "rfa_bwd_rr" else not r.tile_bounds
    ba = be.lib.calls[1][1][0]._obj
    assert ba.dkdv_form == _C.DKDV_128 and not ba.ds_scratch and ba.dkdv_nsplit == 0       # what rfa_bwd_rr asks of the base arguments
    # one batch entry: the batch stride is never used, and says so
    be.lib.calls.clear()
    q1, k1, v1 = _tensors(Bt=1)
    be.fwd(q1, k1, v1, softmax_scale=0.1, causal=True, out=torch.empty_like(q1), lse=torch.empty(1, 4, 128),
           row_ranges=(start[:1, :128], end[:1, :128], 0))
    assert be.lib.calls[0][1][1]._obj.batch_stride == 0
    # what the kernels of such a call do not have, or tensors that do not fit q, are refused before the library is called
    be.lib.calls.clear()
    ok = (start[:, :128], end[:, :128], 0)
    kw = dict(softmax_scale=0.1, causal=True, out=out, lse=lse)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, row_ranges=ok, softcap=30.0, **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, row_ranges=ok, alibi=(torch.zeros(4), 0), **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, row_ranges=ok, dropout=(0.1, 1, 0, 0, 0), **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(*_tensors(D=192), row_ranges=ok, softmax_scale=0.1, causal=True, out=torch.empty(2, 128, 4, 192, dtype=torch.bfloat16), lse=lse)
    for bad in ((start[:, :127], end[:, :127], 0), (start[:, :128].long(), end[:, :128], 0), (start[:, ::2], end[:, :128], 0)):
        with pytest.raises(ValueError):
            be.fwd(q, k, v, row_ranges=bad, **kw)
    assert be.lib.calls == []


# ---------------------------------------------------------------------------------------------- binding
def test_bind_accepts_and_refuses_by_the_table(single_rank_group):
    import ring_flash_attn as R

    s = torch.zeros(2, 64, dtype=torch.int32)
    e = torch.full((2, 64), 64, dtype=torch.int32)
    for name in R._api.ROW_RANGE_FUNCS:
        fn = getattr(R, name)
        assert R.with_row_ranges(fn, None, None) is fn
        assert R.with_row_ranges(fn, s, e) is not fn
        lg = R.with_lse_grad(fn)
        assert R.with_row_ranges(lg, None, None) is lg and callable(R.with_row_ranges(lg, s, e))
    ranged = R.with_row_ranges(R.ring_flash_attn_func, s, e)
    assert ranged.__name__ == "ring_flash_attn_func"
    # the existing binders' checks are untouched and keep refusing a ranged function
    for binder in (lambda f: R.with_softcap(f, 30.0), lambda f: R.with_sinks(f, torch.zeros(4)), R.with_lse_grad,
                   lambda f: R.with_max_logit(f, torch.full((4,), float("-inf"))), lambda f: R.with_row_ranges(f, s, e)):
        with pytest.raises(TypeError):
            binder(ranged)
    others = [getattr(R, n) for n in dir(R) if n.endswith("_func") and n not in R._api.ROW_RANGE_FUNCS]
    assert len(others) == 15
    for fn in others + [R.with_softcap(R.ring_flash_attn_func, 30.0), R.with_sinks(R.ring_flash_attn_func, torch.zeros(4)),
                        R.with_max_logit(R.ring_flash_attn_func, torch.full((4,), float("-inf"))), len, None]:
        with pytest.raises(TypeError):
            R.with_row_ranges(fn, s, e)
    for bad in ((s, None), (None, e), (s.long(), e), (s, e.float()), (s[:, ::2], e[:, ::2]), (s, e[:, :32].contiguous()), (s[0], e[0])):
        with pytest.raises(ValueError):
            R.with_row_ranges(R.ring_flash_attn_func, *bad)


def _world(W, cases):
    errs, notes = RW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs[:20])
    return notes


REFUSALS = [("NotImplementedError", "dropout"), ("NotImplementedError", "alibi"), ("NotImplementedError", "head_dim"),
            ("NotImplementedError", "vdim"), ("NotImplementedError", "backend"),
            ("ValueError", "dtype"), ("ValueError", "shape"), ("ValueError", "contiguity"), ("ValueError", "one_of_two"),
            ("ValueError", "device")] + \
           [("TypeError", "func:" + f) for f in ("varlen", "zigzag_varlen", "stripe", "llama3", "zigzag_llama3", "softcap", "sinks",
                                                  "max_logit", "ulysses", "row_ranges", "lambda")]


@pytest.mark.parametrize("kind", ["ring", "zigzag"])
def test_every_row_of_the_refusal_table_on_every_rank(built, kind):
    """W = 2: each refusal comes before any block call and before anything is exchanged — a barrier finds both ranks"""
    cases = [dict(kind=kind, W=2, S=64, pattern="doc", causal=True, refuse=r, how=h) for r, h in REFUSALS]
    _world(2, cases)


def test_checkpointing_reruns_with_the_ranges(built, single_rank_group):
    """activation checkpointing re-runs the wrapped call: the re-run binds the ranges again, and the backward — which runs
    outside every binding — uses the node's own"""
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from torch.utils.checkpoint import checkpoint

    c = dict(kind="ring", W=1, S=64, pattern="doc", causal=True)
    q, k, v, do = RW.inputs(c)
    start, end = RW.ranges(c)
    rec = RB.Recording(RB.RowRangeBackend())
    _testing.set_backend(rec)
    try:
        attn = R.with_row_ranges(R.zigzag_ring_flash_attn_func, start, end)
        grads = []
        for ckpt in (False, True):
            ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
            rec.seen = {"fwd": [], "bwd": []}
            out = checkpoint(attn, *ins, use_reentrant=False, causal=True) if ckpt else attn(*ins, causal=True)
            assert R._api._row_ranges.get() is None and R._api._block_mask.get() is None    # nothing stays bound behind the call
            assert R._api._sinks.get() is None and R._api._lse_grad.get() is False
            out.backward(do)
            assert len(rec.seen["fwd"]) == (2 if ckpt else 1) and len(rec.seen["bwd"]) == 1
            assert all(n == (0, (2, 64), (2, 64)) for n in rec.seen["fwd"] + rec.seen["bwd"])
            grads.append([out.detach()] + [t.grad for t in ins])
        for a, b in zip(*grads):
            assert torch.equal(a, b)
        ref = RB.single_device(q, k, v, do, RB.mask_of(start, end, True))
        for nm, got, want, kd in zip(("out", "dq", "dk", "dv"), grads[1], (ref[0],) + tuple(ref[2:]), ("out", "grad", "grad", "grad")):
            _tol.compare(f"checkpointed.{nm}", got, want, kd)
    finally:
        _testing.set_backend(None)


# ---------------------------------------------------------------------------------------------- schedules
PATTERNS = [dict(pattern="doc", causal=True), dict(pattern="doc", causal=False), dict(pattern="prefix", causal=False),
            dict(pattern="random", causal=False), dict(pattern="random", causal=True),
            dict(pattern="doc", causal=True, window=(23, -1)), dict(pattern="prefix", causal=False, window=(30, 11))]


def _schedule_cases(W):
    cases = [dict(kind="ring", W=W, S=64, **p) for p in PATTERNS]
    for form in (("ring",) if W == 1 else ("ring", "gather", "gather_ps")):
        cases += [dict(kind="zigzag", form=form, W=W, S=64, **p) for p in PATTERNS]
    # the packed entry points and a with_lse_grad result underneath
    cases += [dict(kind="ring", W=W, S=64, pack="kv", **PATTERNS[0]), dict(kind="zigzag", W=W, S=64, pack="qkv", **PATTERNS[2]),
              dict(kind="zigzag", W=W, S=64, lse_grad=True, **PATTERNS[1])]
    return cases


@pytest.mark.parametrize("W", [1, 2, 4])
def test_ring_and_zigzag_against_one_fp64_attention_with_the_explicit_mask(built, W):
    """S = 64 rows per rank, H 4 / Hk 2, D 64; documents, prefix-LM (non-causal), random intervals with empty rows, ranges under
    causal and a window — out, lse, dq, dk, dv within the unchanged kinds of tests/_tol.py, and NOT within them of the same call
    without ranges"""
    notes = _world(W, _schedule_cases(W))
    assert len(notes) >= 5 * W * len(PATTERNS)


def test_union_of_intervals_by_two_ranged_calls_and_merge_attn(built):
    """the README's recipe: a causal window of 24 keys plus 8 global tokens = two disjoint intervals per row — two ranged calls
    under with_lse_grad, merge_attn — equals the fp64 attention with the union mask, forward and backward, at W = 2"""
    base = dict(W=2, S=64, pattern="window_part", causal=True, union=True, w=24, G=8)
    _world(2, [dict(kind="zigzag", **base), dict(kind="ring", **base)])
