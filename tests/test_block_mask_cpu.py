"""Block-sparse masks (ring_flash_attn.with_block_mask; include/rfa.h: rfa_fwd_bm / rfa_bwd_bm) without a device: the shared
bit / walk arithmetic under sanitizers, the C ABI (symbols, struct layout, every argument check with NULL tensors in the stated
order), what the HIP backend puts into the struct, the binder's table, every row of the refusal and ValueError tables on both
ranks of a W = 2 world, activation checkpointing, and the ring and zigzag schedules (all three exchange forms, W = 1, 2, 4,
S_local 256, D 32) on the CPU test backend (tests/_blockmask_backend.py) against ONE single-device fp64 attention with the
expanded mask, through tests/_tol.py unchanged — each case also NOT within tolerance of the un-masked attention."""
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
import _blockmask_backend as MB                  # noqa: E402
import _blockmask_worker as MW                   # noqa: E402
import _tol                                      # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8


# ---------------------------------------------------------------------------------------------- shared arithmetic
def test_bit_addressing_and_walks_against_a_brute_force_mask_under_sanitizers():
    """tests/native/blockmask_check.cpp: every function of csrc/rfa_blockmask.h — the header the three kernels share — over
    small geometries (k_blk0 negative, unaligned, partly and wholly outside the mask; lists of length 0 .. 3; G 1 .. 64 with
    per-head columns; nsplit 1 .. 4), under ASan / UBSan, as a program of its own"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "blockmask_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "blockmask_check.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "configurations ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays(built):
    import ring_flash_attn as R
    from ring_flash_attn import _C

    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert "int rfa_fwd_bm(const rfa_fwd_args *args, const rfa_blockmask_args *bm, void *stream);" in header
    assert "int rfa_bwd_bm(const rfa_bwd_args *args, const rfa_blockmask_args *bm, void *stream);" in header
    assert "#define RFA_BLOCK_MASK_SIZE 128" in header and R.BLOCK_MASK_SIZE == 128
    for sym in ("rfa_fwd_bm", "rfa_bwd_bm", "rfa_blockmask_workspace_bytes"):
        assert sym in names and sym in _C.SYMBOLS
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)


def test_struct_matches_the_c_layout(built):
    from ring_flash_attn import _C

    fields = [n for n, _ in _C.BlockMaskArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu\\n", sizeof(rfa_blockmask_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_blockmask_args, {n}));\n' for n in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _C.BlockMaskArgs
    assert fields == ["struct_bytes", "reserved", "mask", "batch_stride", "head_stride", "row_stride", "nk_blocks", "k_blk0", "workspace"]
    assert got[0] == C.sizeof(A) == 64
    assert got[1:] == [getattr(A, n).offset for n in fields] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert A().struct_bytes == 64


def _base(cls, **kw):
    a = cls()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.softmax_scale = 2, 300, 300, 4, 2, 128, 0, 0.07
    if hasattr(a, "dkdv_form"):
        from ring_flash_attn import _C

        a.dkdv_form = _C.DKDV_128
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def _bm(**kw):
    from ring_flash_attn import _C

    r = _C.BlockMaskArgs()
    r.nk_blocks = 3
    for n, x in kw.items():
        setattr(r, n, x)
    return r


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_every_argument_check_with_null_tensors_in_the_stated_order(built, which):
    """every tensor pointer is NULL: nothing is read, nothing is launched, no device is needed"""
    from ring_flash_attn import _C

    lib = _C.load()
    fn, cls = (lib.rfa_fwd_bm, _C.FwdArgs) if which == "fwd" else (lib.rfa_bwd_bm, _C.BwdArgs)
    run = lambda a, r: fn(C.byref(a), None if r is None else C.byref(r), None)
    assert fn(None, C.byref(_bm()), None) == ERR_NULL
    # the struct's own checks, each alone
    assert run(_base(cls), None) == ERR_ARGS
    for kw in (dict(struct_bytes=8), dict(struct_bytes=63), dict(reserved=1)):
        assert run(_base(cls), _bm(**kw)) == ERR_ARGS, kw
    # what the masked kernels do not have, in the base arguments: dropout, packed input, halves (and, backward, another plan)
    cu = (C.c_int32 * 3)(0, 100, 300)
    cu_p = C.cast(cu, C.c_void_p).value
    for kw in (dict(dropout_p=0.1), dict(cu_seqlens_q=cu_p, cu_seqlens_k=cu_p), dict(q_half=1), dict(k_half=2)):
        assert run(_base(cls, **kw), _bm()) == ERR_ARGS, kw
    if which == "bwd":
        for kw in (dict(dkdv_form=_C.DKDV_AUTO), dict(dkdv_form=_C.DKDV_256), dict(dkdv_form=_C.DKDV_BAL), dict(ds_scratch=4096)):
            assert run(_base(cls, **kw), _bm()) == ERR_ARGS, kw
    for D in (136, 192, 256):
        assert run(_base(cls, D=D), _bm()) == ERR_HEAD_DIM, D
    for kw in (dict(batch_stride=-1), dict(head_stride=-1), dict(row_stride=-1), dict(nk_blocks=-1), dict(nk_blocks=2 ** 31),
               dict(k_blk0=2 ** 30 + 1), dict(k_blk0=-2 ** 30 - 1)):
        assert run(_base(cls), _bm(**kw)) == ERR_ARGS, kw
    assert run(_base(cls, H=130, Hk=2), _bm()) == ERR_ARGS             # 65 query heads per K/V head
    assert run(_base(cls, H=128, Hk=2), _bm()) == ERR_NULL             # 64 are served
    # a longer struct whose unknown tail is zero is accepted, one with a non-zero tail is not
    class Longer(C.Structure):
        _fields_ = [("r", _C.BlockMaskArgs), ("tail", C.c_int32 * 2)]

    lo = Longer()
    lo.r = _bm(struct_bytes=72)
    as_bm = lambda: C.cast(C.pointer(lo), C.POINTER(_C.BlockMaskArgs))
    assert fn(C.byref(_base(cls)), as_bm(), None) == ERR_NULL          # through to the base call's NULL tensors
    lo.tail[1] = 1
    assert fn(C.byref(_base(cls)), as_bm(), None) == ERR_ARGS
    # the order: struct (ARGS) < base combination (ARGS) < head dim (HEAD_DIM) < the struct's numbers (ARGS) < every base check
    assert run(_base(cls, D=192, dtype=7, dropout_p=0.5), _bm(reserved=1, batch_stride=-1)) == ERR_ARGS
    assert run(_base(cls, D=192, dtype=7), _bm(batch_stride=-1)) == ERR_HEAD_DIM
    assert run(_base(cls, dtype=7), _bm(batch_stride=-1)) == ERR_ARGS
    chain = [(dict(dtype=7), ERR_DTYPE), (dict(Hk=3), ERR_HEADS), (dict(B=-1), ERR_SHAPE), (dict(Sq=-1), ERR_SHAPE)]
    for i, (_, want) in enumerate(chain):
        kw = {}
        for later, _w in chain[i:]:
            kw.update(later)
        assert run(_base(cls, **kw), _bm()) == want, (i, kw)
    assert run(_base(cls, B=0), _bm()) == OK                           # nothing to do
    assert run(_base(cls), _bm()) == ERR_NULL                          # q, k, v ... (and, behind them, the mask)
    for D in range(8, 129, 8):
        assert run(_base(cls, D=D), _bm()) == ERR_NULL, D
    assert run(_base(cls, D=132), _bm()) == ERR_HEAD_DIM               # (the base check: not a multiple of 8)
    # the base entry points answer as before
    base_fn = lib.rfa_fwd if which == "fwd" else lib.rfa_bwd
    assert base_fn(C.byref(_base(cls)), None) == ERR_NULL and base_fn(C.byref(_base(cls, D=260)), None) == ERR_HEAD_DIM
    if which == "bwd":
        assert lib.rfa_blockmask_workspace_bytes(C.byref(_base(cls))) == 0     # (the kernels read the bytes themselves)
        assert lib.rfa_blockmask_workspace_bytes(None) == 0


# ---------------------------------------------------------------------------------------------- routing
class _RecLib:
    """the loaded library with a note of every function called through it; nothing is launched (no device here)"""
    NOTED = ("rfa_fwd", "rfa_fwd_ex", "rfa_fwd_vd", "rfa_fwd_rr", "rfa_fwd_bm", "rfa_bwd", "rfa_bwd_ex", "rfa_bwd_vd", "rfa_bwd_rr",
             "rfa_bwd_bm")

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


def _tensors(D=64, S=256, Bt=2):
    mk = lambda h: torch.zeros(Bt, S, h, D, dtype=torch.bfloat16)
    return mk(4), mk(2), mk(2)


def test_calls_without_a_mask_never_reach_the_new_functions(rec_backend, monkeypatch):
    from ring_flash_attn import backend

    monkeypatch.setattr(backend, "_spill_enabled", lambda: False)
    be = rec_backend
    assert be.serves_block_mask is True
    q, k, v = _tensors()
    out, lse = torch.empty_like(q), torch.empty(2, 4, 256)
    be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=True, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v))
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd", "rfa_bwd"]


def test_what_the_backend_puts_into_the_struct(rec_backend):
    from ring_flash_attn import _C

    be = rec_backend
    q, k, v = _tensors()
    out, lse = torch.empty_like(q), torch.empty(2, 4, 256)
    mask = torch.ones(2, 4, 6, 9, dtype=torch.bool)
    # a schedule hands over a slice of the query-block axis: the strides of the whole tensor, the slice's first byte
    bm = (mask[:, :, 2:4], -7)
    be.fwd(q, k, v, softmax_scale=0.1, causal=False, out=out, lse=lse, block_mask=bm, window=(40, -1), mask_shift=64)
    be.bwd(out, q, k, v, lse, lse.clone(), softmax_scale=0.1, causal=False, dq=torch.empty_like(q), dk=torch.empty_like(k),
           dv=torch.empty_like(v), block_mask=bm, window=(40, -1), mask_shift=64)
    assert [n for n, _ in be.lib.calls] == ["rfa_fwd_bm", "rfa_bwd_bm"]
    for name, (a, r, _s) in be.lib.calls:
        a, r = a._obj, r._obj
        assert r.struct_bytes == C.sizeof(_C.BlockMaskArgs) == 64 and r.reserved == 0
        assert r.mask == mask.data_ptr() + 2 * 9
        assert (r.batch_stride, r.head_stride, r.row_stride, r.nk_blocks, r.k_blk0) == (4 * 6 * 9, 6 * 9, 9, 9, -7)
        assert not r.workspace
        assert (a.window, a.window_left, a.window_right, a.mask_shift, a.causal) == (1, 40, -1, 64, 0)
    ba = be.lib.calls[1][1][0]._obj
    assert ba.dkdv_form == _C.DKDV_128 and not ba.ds_scratch and ba.dkdv_nsplit == 0       # what rfa_bwd_bm asks of the base arguments
    # broadcast dims: their strides are 0; uint8 is taken as well
    be.lib.calls.clear()
    shared = torch.ones(1, 1, 2, 9, dtype=torch.uint8)
    be.fwd(q, k, v, softmax_scale=0.1, causal=True, out=out, lse=lse, block_mask=(shared, 0))
    r = be.lib.calls[0][1][1]._obj
    assert (r.batch_stride, r.head_stride, r.row_stride, r.nk_blocks) == (0, 0, 9, 9) and r.mask == shared.data_ptr()
    # what the kernels of such a call do not have, or a mask that does not fit q, is refused before the library is called
    be.lib.calls.clear()
    ok = (mask[:, :, :2], 0)
    kw = dict(softmax_scale=0.1, causal=True, out=out, lse=lse)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, block_mask=ok, softcap=30.0, **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, block_mask=ok, alibi=(torch.zeros(4), 0), **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, block_mask=ok, dropout=(0.1, 1, 0, 0, 0), **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(q, k, v, block_mask=ok, row_ranges=(torch.zeros(2, 256, dtype=torch.int32), torch.ones(2, 256, dtype=torch.int32), 0), **kw)
    with pytest.raises(NotImplementedError):
        be.fwd(*_tensors(D=192), block_mask=ok, softmax_scale=0.1, causal=True, out=torch.empty(2, 256, 4, 192, dtype=torch.bfloat16), lse=lse)
    for bad in ((mask[:, :, :3], 0), (mask[:, :, :2].float(), 0), (mask[:, :, :2, ::2], 0), (mask[:, :3, :2], 0), (mask[0, :, :2], 0)):
        with pytest.raises(ValueError):
            be.fwd(q, k, v, block_mask=bad, **kw)
    assert be.lib.calls == []


# ---------------------------------------------------------------------------------------------- binding
def test_bind_accepts_and_refuses_by_the_table(single_rank_group):
    import ring_flash_attn as R

    m = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    for name in R._api.ROW_RANGE_FUNCS:
        fn = getattr(R, name)
        assert R.with_block_mask(fn, None) is fn
        assert R.with_block_mask(fn, m) is not fn
        lg = R.with_lse_grad(fn)
        assert R.with_block_mask(lg, None) is lg and callable(R.with_block_mask(lg, m))
    masked = R.with_block_mask(R.ring_flash_attn_func, m)
    assert masked.__name__ == "ring_flash_attn_func" and not "with_block_mask".endswith("_func")
    # the existing binders' checks are untouched and refuse a masked function
    s, e = torch.zeros(2, 64, dtype=torch.int32), torch.full((2, 64), 64, dtype=torch.int32)
    for binder in (lambda f: R.with_softcap(f, 30.0), lambda f: R.with_sinks(f, torch.zeros(4)), R.with_lse_grad,
                   lambda f: R.with_max_logit(f, torch.full((4,), float("-inf"))), lambda f: R.with_row_ranges(f, s, e),
                   lambda f: R.with_ulysses(f, single_rank_group), lambda f: R.with_block_mask(f, m)):
        with pytest.raises(TypeError):
            binder(masked)
    others = [getattr(R, n) for n in dir(R) if n.endswith("_func") and n not in R._api.ROW_RANGE_FUNCS]
    assert len(others) == 15
    for fn in others + [R.with_softcap(R.ring_flash_attn_func, 30.0), R.with_sinks(R.ring_flash_attn_func, torch.zeros(4)),
                        R.with_max_logit(R.ring_flash_attn_func, torch.full((4,), float("-inf"))),
                        R.with_row_ranges(R.ring_flash_attn_func, s, e), len, None]:
        with pytest.raises(TypeError):
            R.with_block_mask(fn, m)
    for bad in (m.to(torch.uint8), m.float(), m[0], torch.ones(1, 1, 2, 4, dtype=torch.bool)[..., ::2], [[True]]):
        with pytest.raises(ValueError):
            R.with_block_mask(R.ring_flash_attn_func, bad)


def _world(W, cases):
    errs, notes = MW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs[:20])
    return notes


REFUSALS = [("NotImplementedError", "dropout"), ("NotImplementedError", "alibi"), ("NotImplementedError", "head_dim"),
            ("NotImplementedError", "vdim"), ("NotImplementedError", "backend"), ("NotImplementedError", "group"),
            ("ValueError", "dtype"), ("ValueError", "shape"), ("ValueError", "rows"), ("ValueError", "heads"), ("ValueError", "contiguity"),
            ("ValueError", "device"), ("ValueError", "alignment")] + \
           [("TypeError", "func:" + f) for f in ("varlen", "zigzag_varlen", "stripe", "llama3", "zigzag_llama3", "softcap", "sinks",
                                                  "max_logit", "ulysses", "row_ranges", "block_mask", "lambda")]


@pytest.mark.parametrize("kind", ["ring", "zigzag"])
def test_every_row_of_the_refusal_table_on_every_rank(built, kind):
    """W = 2: each refusal comes before any block call and before anything is exchanged — a barrier finds both ranks"""
    cases = [dict(kind=kind, W=2, S=256, pattern="docs", causal=True, refuse=r, how=h) for r, h in REFUSALS]
    _world(2, cases)


def test_one_rank_serves_any_lengths(built, single_rank_group):
    """W = 1: Sq 200 against Sk 333 (partial tail blocks, Sq != Sk), ring and zigzag entry points, causal or not"""
    import ring_flash_attn as R
    from ring_flash_attn import _testing

    g = torch.Generator().manual_seed(3)
    mk = lambda s, h: torch.randn(2, s, h, 32, generator=g).bfloat16()
    q, k, v, do = mk(200, 4), mk(333, 2), mk(333, 2), mk(200, 4)
    m = torch.tensor([[1, 0, 1], [0, 1, 1]], dtype=torch.bool).view(1, 1, 2, 3)
    _testing.set_backend(MB.BlockMaskBackend())
    try:
        for fn, causal in ((R.ring_flash_attn_func, False), (R.ring_flash_attn_func, True), (R.zigzag_ring_flash_attn_func, True)):
            ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
            out, lse, _ = R.with_block_mask(fn, m)(*ins, causal=causal, return_attn_probs=True)
            out.backward(do)
            ref = MB.single_device(q, k, v, do, MB.expand(m, 2, 4, 200, 333, causal))
            for nm, got, want, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse) + tuple(t.grad for t in ins), ref,
                                         ("out", "lse", "grad", "grad", "grad")):
                _tol.compare(f"{fn.__name__}.{nm}", got, want, kd)
    finally:
        _testing.set_backend(None)


def test_checkpointing_reruns_with_the_mask(built, single_rank_group):
    """activation checkpointing re-runs the wrapped call: the re-run binds the mask again, and the backward — which runs
    outside every binding — uses the node's own"""
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from torch.utils.checkpoint import checkpoint

    c = dict(kind="ring", W=1, S=256, pattern="per_head", causal=True)
    q, k, v, do = MW.inputs(c)
    mask = MW.global_mask(c)
    rec = MB.Recording(MB.BlockMaskBackend())
    _testing.set_backend(rec)
    try:
        attn = R.with_block_mask(R.zigzag_ring_flash_attn_func, mask)
        grads = []
        for ckpt in (False, True):
            ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
            rec.seen = {"fwd": [], "bwd": []}
            out = checkpoint(attn, *ins, use_reentrant=False, causal=True) if ckpt else attn(*ins, causal=True)
            assert R._api._row_ranges.get() is None and R._api._block_mask.get() is None    # nothing stays bound behind the call
            assert R._api._sinks.get() is None and R._api._lse_grad.get() is False
            out.backward(do)
            assert len(rec.seen["fwd"]) == (2 if ckpt else 1) and len(rec.seen["bwd"]) == 1
            assert all(n == (0, (2, 4, 2, 2), 0, (2, 256)) for n in rec.seen["fwd"] + rec.seen["bwd"])
            grads.append([out.detach()] + [t.grad for t in ins])
        for a, b in zip(*grads):
            assert torch.equal(a, b)
        ref = MB.single_device(q, k, v, do, MB.expand(mask, 2, 4, 256, 256, True))
        for nm, got, want, kd in zip(("out", "dq", "dk", "dv"), grads[1], (ref[0],) + tuple(ref[2:]), ("out", "grad", "grad", "grad")):
            _tol.compare(f"checkpointed.{nm}", got, want, kd)
    finally:
        _testing.set_backend(None)


# ---------------------------------------------------------------------------------------------- schedules
MASKS = ("docs", "bigbird", "per_head", "dark_rows")
BANDS = [dict(causal=True), dict(causal=True, window=(300, -1)), dict(causal=False, window=(200, 150))]
PATTERNS = [dict(pattern=m, **b) for m in MASKS for b in BANDS]


def _schedule_cases(W):
    cases = [dict(kind="ring", W=W, S=256, **p) for p in PATTERNS]
    for form in (("ring",) if W == 1 else ("ring", "gather", "gather_ps")):
        cases += [dict(kind="zigzag", form=form, W=W, S=256, check_mixed=True, **p) for p in PATTERNS]
    # a non-causal call without a window, the packed entry points and a with_lse_grad result underneath, with a loss on lse
    cases += [dict(kind="ring", W=W, S=256, pattern="bigbird", causal=False), dict(kind="zigzag", W=W, S=256, pattern="bigbird", causal=False),
              dict(kind="ring", W=W, S=256, pack="kv", **PATTERNS[0]), dict(kind="zigzag", W=W, S=256, pack="qkv", **PATTERNS[6]),
              dict(kind="zigzag", W=W, S=256, lse_grad=True, **PATTERNS[3]), dict(kind="ring", W=W, S=256, lse_grad=True, **PATTERNS[8])]
    return cases


@pytest.mark.parametrize("W", [1, 2, 4])
def test_ring_and_zigzag_against_one_fp64_attention_with_the_expanded_mask(built, W):
    """S = 256 rows per rank, H 4 / Hk 2, D 32; block-diagonal documents, window + global + random blocks, per-head masks with
    GQA, query blocks without a lit key block — each under causal, under a causal window and under a two-sided window: out, lse,
    dq, dk, dv within the unchanged kinds of tests/_tol.py, NOT within them of the same call without the mask, and every block
    call carried the k_blk0 and the mask rows of its query rows"""
    notes = _world(W, _schedule_cases(W))
    assert len(notes) >= 5 * W * len(PATTERNS)
