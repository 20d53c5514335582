"""Harmful neighbours: what a kernel must never read, and what it must never write.

Every case compares a clean run with a poisoned run BIT FOR BIT over every output, and checks that every byte outside the
addressed output region keeps its sentinel.

  guard bands    q, k, v, do, lse, delta (inputs) and out, lse, dq, dk, dv and the fp32 accumulators (outputs) are views into
                 larger allocations with extra rows behind every batch entry (behind the packed rows), extra heads, and 8 extra
                 elements behind every head's D; the inputs' padding is NaN — a tile that reads past a sequence's end and masks
                 it with p = 0 yields 0 * NaN = NaN, where finite neighbours hide it — the outputs' padding a sentinel.  All
                 strides are multiples of 8, so the backend passes the views through; a spy on the library call asserts that the
                 struct's pointers are the views' own (a silent copy would make the test vacuous).
  neighbours     one whole packed sequence, one whole batch entry, one whole K/V head group (the K/V head and all its query
                 heads) is NaN in q, k, v, do, lse and delta: every other sequence / entry / group has the clean run's bits.
  stale scratch  the pooled dS scratch of the 5-GEMM backward (be._ds_pool) is filled with 0xFF bytes between two runs, whole
                 and chunked: a call reads only what it wrote.  Only data buffers are touched — nothing a kernel waits on (the
                 balanced dK/dV schedule's flags live in the per-call workspace), and no test in this file runs the balanced
                 schedule.

Out of scope: NaN in a MASKED key of the same sequence — 0 * NaN there is what flash_attn does too."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402
import test_gpu_band_forms as GF                 # noqa: E402  (the device helpers; nothing in it touches a device at import)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_EXT = pytest.mark.extended
NAN = float("nan")
SENTINEL = 5.0
PAD_ROWS, PAD_HEADS, PAD_D = 3, 1, 8
H, Hk = 4, 2
DENSE = BR.Geometry("dense-300-520", "poison", 300, 520, True, BR.NOWIN, 220, 2, None)      # tails of 44 rows and 8 keys
CU_Q = [0, 100, 100, 101, 700, 1000]                                                        # (an empty and a one-row sequence)
CU_K = [0, 300, 300, 333, 1500, 1800]
FWD_ENV = dict(BR.FWD_FORMS, p8x32=(dict(RFA_FWD_FORM="p8x32", RFA_FWD_KV_NSPLIT="1"), 1))
# (forward form, backward form, D, Dv)
CASES = [("8x32", "7gemm", 128, 128), ("4x32", "5gemm", 128, 128), ("p8x32", "dkdv128", 128, 128), ("split3", "dkdv256-2", 128, 128),
         ("8x32", "dkdv128", 64, 64), ("4x32", "dkdv256-2", 64, 64), ("split3", "dkdv128", 64, 64),
         ("auto", "auto", 80, 80), ("auto", "7gemm", 192, 192), ("auto", "5gemm", 192, 192), ("auto", "auto", 192, 128)]
CORE = {("8x32", "7gemm", 128, 128), ("4x32", "5gemm", 128, 128), ("split3", "dkdv256-2", 128, 128), ("auto", "auto", 192, 128)}


def _bwd_env(form):
    return {} if form == "auto" else BR.BWD_FORMS[form][0]


def _check_forms(lib, fwd, bwd, D, Dv):
    """the dense case runs the forms it names (host side, as tests/test_gpu_band_forms.py does)"""
    from ring_flash_attn import _C

    if Dv != D or D in (80, 192):
        assert fwd == "auto"
        if bwd != "auto":
            five = BR.bwd_plan(lib, BR.bwd_args(_C, DENSE, H, Hk, D, _bwd_env(bwd)))[2]
            assert five == (1 if bwd == "5gemm" else 0)
        return
    if fwd == "p8x32":
        assert D == 128 and DENSE.shift == 0
    else:
        BR.check_fwd_form(_C, lib, DENSE, fwd, D, H, Hk)
    if not (bwd in ("5gemm", "7gemm") and D == 64):
        BR.check_bwd_form(_C, lib, DENSE, bwd, D, H, Hk)


# ---- guarded allocations ---------------------------------------------------------------------------------------------------
def _guarded(t, fill, rows_dim):
    """(view, whole): `view` holds t's values inside a larger allocation `whole` filled with `fill` — PAD_ROWS more rows along
    rows_dim, PAD_HEADS more heads, PAD_D more elements behind D; an lse-like tensor ((B, H, S) / (H, T)): rows and heads"""
    shape = list(t.shape)
    lse_like = t.dtype == torch.float32 and rows_dim == t.dim() - 1
    if lse_like:
        shape[-1] += PAD_ROWS + 5                      # (any row count: the row stride is 1)
        shape[-2] += PAD_HEADS
    else:
        shape[rows_dim] += PAD_ROWS
        shape[-2] += PAD_HEADS
        shape[-1] += PAD_D
    whole = torch.full(shape, fill, dtype=t.dtype, device=t.device)
    view = whole[tuple(slice(0, n) for n in t.shape)]
    view.copy_(t)
    assert view.data_ptr() == whole.data_ptr() and not view.is_contiguous()
    return view, whole


def _outside_untouched(name, view, whole, before):
    """every element of `whole` outside `view` still holds its sentinel, bit for bit"""
    a, b = whole.clone(), before.clone()
    a[tuple(slice(0, n) for n in view.shape)] = 0
    b[tuple(slice(0, n) for n in view.shape)] = 0
    assert torch.equal(a, b), f"{name}: written outside the addressed region"


class _Spy:
    """wraps the library's entry points of one call and records the argument struct's pointers"""
    NAMES = ("rfa_fwd", "rfa_bwd", "rfa_fwd_vd", "rfa_bwd_vd")
    FIELDS = ("q", "k", "v", "dout", "out", "lse", "delta", "dq", "dk", "dv", "out_acc", "lse_acc", "dq_acc", "dk_acc", "dv_acc")

    def __init__(self, monkeypatch, lib):
        self.seen = []
        for n in self.NAMES:
            monkeypatch.setattr(lib, n, self._wrap(n, getattr(lib, n)), raising=True)

    def _wrap(self, name, fn):
        def call(args, *rest):
            a = args._obj
            self.seen.append((name, {f: getattr(a, f) for f in self.FIELDS if hasattr(a, f)}))
            return fn(args, *rest)
        return call

    def last(self, prefix):
        return next(p for n, p in reversed(self.seen) if n.startswith(prefix))

    def assert_passed_through(self, prefix, **views):
        got = self.last(prefix)
        for f, t in views.items():
            assert (got[f] or 0) == t.data_ptr(), f"{prefix}: {f} is not the view's own storage — the backend copied it"


def _inputs(shape_q, shape_k, D, Dv, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda lead, h, d: torch.randn(*lead, h, d, generator=gen).to(BF).to(dev)
    return mk(shape_q, H, D), mk(shape_k, Hk, D), mk(shape_k, Hk, Dv), mk(shape_q, H, Dv)


def _run_all(be, q, k, v, do, kw, lse_shape, rows_dim, guard, spy=None, lse_in=None, delta_in=None):
    """forward (plain, overwritten accumulators) and backward (plain, += onto zeroed accumulators) of one call; with `guard`
    every tensor is a view into a NaN- (inputs) or sentinel-padded (outputs) allocation.  Returns ({name: output}, lse, delta)"""
    dev, Dv = q.device, v.shape[-1]
    wholes = {}

    def inp(name, t):
        if not guard:
            return t
        view, _ = _guarded(t, NAN, rows_dim if t.dim() > len(lse_shape) else t.dim() - 1)
        return view

    def outp(name, shape, dtype, init=SENTINEL):
        t = torch.full(shape, init, dtype=dtype, device=dev)
        if not guard:
            return t
        view, whole = _guarded(t, SENTINEL, rows_dim if len(shape) > len(lse_shape) else len(shape) - 1)
        wholes[name] = (view, whole, whole.clone())
        return view

    qs, ks, vs, dos = inp("q", q), inp("k", k), inp("v", v), inp("do", do)
    o_shape = (*q.shape[:-1], Dv)
    res = {}
    res["out"], res["lse"] = outp("out", o_shape, q.dtype), outp("lse", lse_shape, torch.float32)
    be.fwd(qs, ks, vs, out=res["out"], lse=res["lse"], **kw)
    if spy is not None and guard:
        spy.assert_passed_through("rfa_fwd", q=qs, k=ks, v=vs, out=res["out"], lse=res["lse"])
    res["out_acc"], res["lse_acc"] = outp("out_acc", o_shape, torch.float32), outp("lse_acc", lse_shape, torch.float32)
    be.fwd(qs, ks, vs, out_acc=res["out_acc"], lse_acc=res["lse_acc"], acc_init=True, **kw)
    if lse_in is None:                                   # (the clean run makes the backward's inputs for both runs)
        lse_in = res["lse"].contiguous().clone()
        delta_in = torch.empty_like(lse_in)
        pre = {n: kw[n] for n in ("cu_seqlens_q", "max_seqlen_q", "q_half") if n in kw}
        delta_in.zero_()
        be.bwd_preprocess(do, res["out"].contiguous(), delta_in, **pre)
    ls, ds = inp("lse_in", lse_in), inp("delta_in", delta_in)
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        res[n] = outp(n, t.shape, t.dtype)
        res[n + "_acc"] = outp(n + "_acc", t.shape, torch.float32, init=0.0)
    be.bwd(dos, qs, ks, vs, ls, ds, dq=res["dq"], dk=res["dk"], dv=res["dv"], **kw)
    if spy is not None and guard:
        spy.assert_passed_through("rfa_bwd", dout=dos, q=qs, k=ks, v=vs, lse=ls, delta=ds, dq=res["dq"], dk=res["dk"], dv=res["dv"])
    be.bwd(dos, qs, ks, vs, ls, ds, dq_acc=res["dq_acc"], dk_acc=res["dk_acc"], dv_acc=res["dv_acc"], **kw)
    torch.cuda.synchronize()
    for name, (view, whole, before) in wholes.items():
        _outside_untouched(name, view, whole, before)
    return res, lse_in, delta_in


def _assert_same_bits(tag, clean, got, select=None):
    for n in clean:
        a, b = clean[n], got[n]
        if select is not None:
            a, b = select(n, a), select(n, b)
        assert torch.equal(a, b), f"{tag}: {n} differs from the clean run ({int((a != b).sum())} elements)"


def _set_forms(monkeypatch, fwd, bwd):
    GF._setenv(monkeypatch, FWD_ENV[fwd][0])
    GF._setenv(monkeypatch, _bwd_env(bwd))


def _packed_kw(dev, **extra):
    cq, ck = (torch.tensor(c, dtype=torch.int32, device=dev) for c in (CU_Q, CU_K))
    mq, mk = (max(b - a for a, b in zip(c, c[1:])) for c in (CU_Q, CU_K))
    return dict(cu_seqlens_q=cq, cu_seqlens_k=ck, max_seqlen_q=mq, max_seqlen_k=mk, **extra)


def _params(cases=None):
    return [pytest.param(*c, id=f"{c[0]}-{c[1]}-d{c[2]}" + (f"v{c[3]}" if c[3] != c[2] else ""), marks=[] if c in CORE else [_EXT])
            for c in (CASES if cases is None else cases)]


# the packed batch: the persistent forward declines cu_seqlens input (it would silently run another form), every other case stays
PACKED_CASES = [c for c in CASES if c[0] != "p8x32"] + [("8x32", "dkdv128", 128, 128)]


def _packed_args(C_, make, D, env, **kw):
    """the argument struct of the packed batch (host side), its cu_seqlens pointers those of a real int32 tensor; returns
    (struct, the tensor that must outlive it)"""
    mq, mk = (max(b - a for a, b in zip(c, c[1:])) for c in (CU_Q, CU_K))
    g = BR.Geometry("packed", "poison", mq, mk, True, BR.NOWIN, mk - mq, len(CU_Q) - 1, None)
    keep = torch.tensor(CU_Q + CU_K, dtype=torch.int32)
    a = make(C_, g, H, Hk, D, env, **kw)
    a.mask_shift = 0
    a.cu_seqlens_q, a.cu_seqlens_k = keep.data_ptr(), keep.data_ptr() + 4 * len(CU_Q)
    a.total_q = CU_Q[-1]
    if hasattr(a, "total_k"):
        a.total_k = CU_K[-1]
    return a, keep


def _check_packed_forms(lib, fwd, bwd, D, Dv):
    """the packed case runs the forms it names (host side)"""
    from ring_flash_attn import _C

    if Dv == D and D in (128, 64):
        a, keep = _packed_args(_C, BR.fwd_args, D, FWD_ENV[fwd][0])
        nbytes, ns = BR.fwd_shares(lib, a)
        want = FWD_ENV[fwd][1]
        assert want is None or (ns == want and (nbytes > 0) == (want > 1)), (fwd, D, nbytes, ns)
    if bwd != "auto":
        a, keep = _packed_args(_C, BR.bwd_args, D, _bwd_env(bwd))
        f, ns, five = BR.bwd_plan(lib, a)
        wform, wns, wfive = BR.BWD_FORMS[bwd][1]
        if D > 128:
            wform = wns = None                                           # (head dims above 128: one dK/dV form; the name asks for the dQ form)
        assert (wform is None or f == wform) and (wns is None or ns == wns) and (wfive is None or five == wfive), (bwd, D, f, ns, five)


# ---- guard bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd,bwd,D,Dv", _params())
def test_guard_bands_around_a_dense_call(monkeypatch, fwd, bwd, D, Dv):
    be = GF._be()
    dev = GF._dev()
    _check_forms(be.lib, fwd, bwd, D, Dv)
    _set_forms(monkeypatch, fwd, bwd)
    g = DENSE
    q, k, v, do = _inputs((g.B, g.lq), (g.B, g.lk), D, Dv, 41 + D, dev)
    kw = dict(softmax_scale=D ** -0.5, causal=True)
    be.release_scratch()
    try:
        clean, lse_in, delta_in = _run_all(be, q, k, v, do, kw, (g.B, H, g.lq), 1, guard=False)
        assert all(bool(torch.isfinite(t).all()) for t in clean.values())
        spy = _Spy(monkeypatch, be.lib)
        got, _, _ = _run_all(be, q, k, v, do, kw, (g.B, H, g.lq), 1, guard=True, spy=spy, lse_in=lse_in, delta_in=delta_in)
        _assert_same_bits(f"dense.{fwd}.{bwd}.d{D}", clean, got)
    finally:
        be.release_scratch()


@pytest.mark.parametrize("fwd,bwd,D,Dv", _params(PACKED_CASES))
def test_guard_bands_around_a_packed_batch(monkeypatch, fwd, bwd, D, Dv):
    be = GF._be()
    dev = GF._dev()
    _check_packed_forms(be.lib, fwd, bwd, D, Dv)
    _set_forms(monkeypatch, fwd, bwd)
    q, k, v, do = _inputs((CU_Q[-1],), (CU_K[-1],), D, Dv, 43 + D, dev)
    kw = dict(softmax_scale=D ** -0.5, causal=True, **_packed_kw(dev))
    be.release_scratch()
    try:
        clean, lse_in, delta_in = _run_all(be, q, k, v, do, kw, (H, CU_Q[-1]), 0, guard=False)
        assert all(bool(torch.isfinite(t).all()) for t in clean.values())
        spy = _Spy(monkeypatch, be.lib)
        got, _, _ = _run_all(be, q, k, v, do, kw, (H, CU_Q[-1]), 0, guard=True, spy=spy, lse_in=lse_in, delta_in=delta_in)
        _assert_same_bits(f"packed.{fwd}.{bwd}.d{D}", clean, got)
    finally:
        be.release_scratch()


# ---- poisoned neighbours inside the tensor ---------------------------------------------------------------------------------
def _poison(t, index):
    t = t.clone()
    t[index] = NAN
    return t


@pytest.mark.parametrize("extra", [dict(), pytest.param(dict(q_half=2, k_half=0, causal=False), marks=_EXT, id="q-back-half"),
                                   pytest.param(dict(q_half=0, k_half=1, causal=False), marks=_EXT, id="k-front-half"),
                                   pytest.param(dict(window=(37, -1), mask_shift_lens=1), marks=_EXT, id="shift-lens")])
@pytest.mark.parametrize("D,Dv", [(128, 128), pytest.param(64, 64, marks=_EXT), pytest.param(192, 128, marks=_EXT)])
def test_a_poisoned_packed_sequence_leaves_the_others_alone(D, Dv, extra):
    """sequence 3 (600 query rows, 1167 keys: between two others) is NaN in q, k, v, do, lse and delta"""
    be = GF._be()
    dev = GF._dev()
    q, k, v, do = _inputs((CU_Q[-1],), (CU_K[-1],), D, Dv, 47 + D, dev)
    kw = dict(dict(softmax_scale=D ** -0.5, causal=True, **_packed_kw(dev)), **extra)
    sq, sk = slice(CU_Q[3], CU_Q[4]), slice(CU_K[3], CU_K[4])
    be.release_scratch()
    try:
        clean, lse_in, delta_in = _run_all(be, q, k, v, do, kw, (H, CU_Q[-1]), 0, guard=False)
        lse_p, delta_p = lse_in.clone(), delta_in.clone()
        lse_p[:, sq], delta_p[:, sq] = NAN, NAN
        got, _, _ = _run_all(be, _poison(q, sq), _poison(k, sk), _poison(v, sk), _poison(do, sq), kw, (H, CU_Q[-1]), 0, guard=False,
                             lse_in=lse_p, delta_in=delta_p)

        def others(name, t):
            rows = sk if name.startswith(("dk", "dv")) else sq
            keep = torch.ones(t.shape[-1] if name.startswith("lse") else t.shape[0], dtype=torch.bool, device=dev)
            keep[rows] = False
            return t[:, keep] if name.startswith("lse") else t[keep]

        _assert_same_bits(f"packed-seq.d{D}", clean, got, others)
    finally:
        be.release_scratch()


@pytest.mark.parametrize("what", ["batch-entry", "head-group"])
@pytest.mark.parametrize("fwd,bwd,D,Dv", _params())
def test_a_poisoned_batch_entry_or_head_group_leaves_the_others_alone(monkeypatch, fwd, bwd, D, Dv, what):
    be = GF._be()
    dev = GF._dev()
    _check_forms(be.lib, fwd, bwd, D, Dv)
    _set_forms(monkeypatch, fwd, bwd)
    g = DENSE
    q, k, v, do = _inputs((g.B, g.lq), (g.B, g.lk), D, Dv, 53 + D, dev)
    kw = dict(softmax_scale=D ** -0.5, causal=True)
    G = H // Hk
    if what == "batch-entry":
        iq = ik = il = (slice(1, 2),)
        keep_q = keep_k = keep_l = (slice(0, 1),)
    else:                                               # K/V head 0 and its query heads 0 .. G-1
        iq, ik, il = (slice(None), slice(None), slice(0, G)), (slice(None), slice(None), slice(0, 1)), (slice(None), slice(0, G))
        keep_q, keep_k, keep_l = (slice(None), slice(None), slice(G, H)), (slice(None), slice(None), slice(1, Hk)), (slice(None), slice(G, H))
    be.release_scratch()
    try:
        clean, lse_in, delta_in = _run_all(be, q, k, v, do, kw, (g.B, H, g.lq), 1, guard=False)
        got, _, _ = _run_all(be, _poison(q, iq), _poison(k, ik), _poison(v, ik), _poison(do, iq), kw, (g.B, H, g.lq), 1, guard=False,
                             lse_in=_poison(lse_in, il), delta_in=_poison(delta_in, il))
        pick = lambda n, t: t[keep_l if n.startswith("lse") else (keep_k if n.startswith(("dk", "dv")) else keep_q)]
        _assert_same_bits(f"{what}.{fwd}.{bwd}.d{D}", clean, got, pick)
    finally:
        be.release_scratch()


# ---- stale dS scratch ------------------------------------------------------------------------------------------------------
def _packed_scratch_limit(C_, lib, form, D):
    """the packed batch's own hand-off plan (host side): the scratch limit that makes it run `form`, None for the whole hand-off"""
    env, (_, _, wfive), limit = BR.BWD_FORMS[form]
    held = []

    def args(scratch_bytes):
        a, keep = _packed_args(C_, BR.bwd_args, D, env, scratch_bytes=scratch_bytes)
        held.append(keep)
        return a

    full, per = lib.rfa_bwd_ds_scratch_bytes(C.byref(args(0))), lib.rfa_bwd_ds_scratch_min_bytes(C.byref(args(0)))
    assert per > 0 and full == H * per, (full, per)
    sb = None if limit is None else limit(full, per, H // Hk)
    a = args(sb or 0)
    n, hc, gc, cb = BR.bwd_chunks(lib, a)
    assert BR.bwd_plan(lib, a)[2] == wfive, form
    if form == "5gemm":
        assert (n, hc, gc, cb) == (1, Hk, H // Hk, full)
    elif form == "5gemm-kv-chunks":
        assert n == Hk // hc > 1 and gc == H // Hk and cb <= sb
    else:
        assert hc == 1 and gc < H // Hk and n == Hk * (H // Hk // gc) and cb <= sb
    return sb


@pytest.mark.parametrize("form", ["5gemm", pytest.param("5gemm-kv-chunks", marks=_EXT), pytest.param("5gemm-q-fractions", marks=_EXT)])
@pytest.mark.parametrize("packed", [False, pytest.param(True, marks=_EXT)], ids=["dense", "packed"])
def test_backward_reads_only_the_ds_it_wrote(monkeypatch, form, packed):
    """run a 5-GEMM backward, fill the pooled dS scratch with 0xFF bytes (a NaN pattern in every io dtype), run it again: the
    first run's bits"""
    from ring_flash_attn import _C

    be = GF._be()
    dev = GF._dev()
    g, D = DENSE, 128
    if packed:
        limit = _packed_scratch_limit(_C, be.lib, form, D)
    else:
        limit = BR.check_bwd_form(_C, be.lib, g, form, D, H, Hk)
    GF._setenv(monkeypatch, BR.BWD_FORMS[form][0])
    if limit is not None:
        monkeypatch.setenv("RFA_DS_SPILL_MAX_BYTES", str(limit))
    if packed:
        q, k, v, do = _inputs((CU_Q[-1],), (CU_K[-1],), D, D, 59, dev)
        kw, lse_shape, rows_dim = dict(softmax_scale=D ** -0.5, causal=True, **_packed_kw(dev)), (H, CU_Q[-1]), 0
    else:
        q, k, v, do = _inputs((g.B, g.lq), (g.B, g.lk), D, D, 61, dev)
        kw, lse_shape, rows_dim = dict(softmax_scale=D ** -0.5, causal=True), (g.B, H, g.lq), 1
    be.release_scratch()
    try:
        first, lse_in, delta_in = _run_all(be, q, k, v, do, kw, lse_shape, rows_dim, guard=False)
        pool = [t for t in be._ds_pool.values() if torch.is_tensor(t)]
        assert pool, "the 5-GEMM backward took no scratch from the pool"
        for t in pool:
            t.view(torch.uint8).fill_(0xFF)
        again, _, _ = _run_all(be, q, k, v, do, kw, lse_shape, rows_dim, guard=False, lse_in=lse_in, delta_in=delta_in)
        assert [t.data_ptr() for t in be._ds_pool.values() if torch.is_tensor(t)] == [t.data_ptr() for t in pool]     # (reused, not re-made)
        _assert_same_bits(f"stale-ds.{form}", first, again)
    finally:
        be.release_scratch()
