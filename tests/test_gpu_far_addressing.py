"""Addressing past 4 GiB and sequences past 64K rows: every kernel form with operands more than 2^31 elements / 2^32 bytes away
from the pointer the library is given, long walks inside one sequence, and the dS hand-off at the top of its 32-bit range.

The kernels form bases with 64-bit products and address inside a tile with 32-bit offsets (include/rfa.h, "row strides"); a
rewrite that turned one 64-bit product into a 32-bit one would pass every test whose tensors are small.  Here they are not:

  far views      (tests/_farview.py) q, k, v, dout / out, dq, dk, dv / lse, delta and the fp32 accumulators are views into
                 arenas of 4 .. 13 GiB that are never filled: batch entry 1, the last K/V head group, or every packed sequence
                 sits past 2^31 elements.  The far run must equal the compact run of the same values BIT FOR BIT (same kernels,
                 same plan — asserted on the host —, deterministic), the compact run is compared with fp64 once per case, a spy
                 asserts that the struct's pointers are the views' own, and where a truncated offset would land (offset mod 2^32
                 bytes) the arena holds NaN (inputs) or a sentinel that must survive (outputs, plus 64 KiB on either side of
                 every far piece).  tests/test_far_cases_cpu.py proves without a device that every case crosses the lines.
  long walks     256 rows against 262144 keys whose rows are 8192 (and 8200) elements apart, so that the running tile pointers
                 and j * tile * row_stride walk to the 2^32-byte line (and across it); a packed batch of 64 x 4096 rows on
                 8192-wide rows whose last sequences start past 2^31 elements.  Against the full fp64 reference.
  dS hand-off    a dense causal sequence of 65504 rows: one head's dS scratch is 4 292 870 144 bytes, just under the 4 GiB the
                 dK/dV kernel's 32-bit block offset can reach; a second head whose share starts past 4 GiB from the pointer.
  row strides    the largest row stride the contract allows next to its compact twin, and a public call beyond it (copied).

No kernel with a deliberately wrong offset is ever run: it would touch memory outside its operands.  Every test computes what
it needs before it allocates and gives arenas and scratch back (release_scratch, empty_cache) when it ends."""
import ctypes as C
import gc
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402
import _blockref as BLK                          # noqa: E402
import _farview as FV                            # noqa: E402
import _tol                                      # noqa: E402
import test_gpu_band_forms as GF                 # noqa: E402  (device helpers; nothing in it touches a device at import)
import test_gpu_poison as GP                     # noqa: E402  (the shapes, CASES and the spy of the poison tests)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
_EXT = pytest.mark.extended
GiB = 1 << 30
H, Hk = GP.H, GP.Hk
R0 = FV.PACKED_ROW0
CU_Q, CU_K = [R0 + c for c in GP.CU_Q], [R0 + c for c in GP.CU_K]       # the poison file's packed batch, behind row R0
BAL = ("auto", "balanced", 128, 128)                                      # the balanced dK/dV schedule at its smallest shape
DENSE_CASES = GP.CASES + [BAL]
OUTPUTS = ("out", "lse", "out_acc", "lse_acc", "dq", "dk", "dv", "dq_acc", "dk_acc", "dv_acc")
ZERO_INIT = ("dq_acc", "dk_acc", "dv_acc")                                # (+= onto zeroed accumulators; the rest: overwritten)
SLACK = 2 * GiB


def _need(nbytes):
    """skip (with the reason) only when the device cannot hold what the test is about to allocate"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + SLACK:
        pytest.skip(f"needs {(nbytes + SLACK) / GiB:.1f} GiB of free device memory, {free / GiB:.1f} GiB are free")


def _give_back(be):
    be.release_scratch()
    gc.collect()
    torch.cuda.empty_cache()


class _Spy(GP._Spy):
    """the poison tests' spy over every attention entry point, which also keeps a copy of each argument struct"""
    NAMES = ("rfa_fwd", "rfa_bwd", "rfa_fwd_vd", "rfa_bwd_vd", "rfa_fwd_ex", "rfa_bwd_ex", "rfa_fwd_rr", "rfa_bwd_rr")

    def __init__(self, monkeypatch, lib):
        self.structs = []
        super().__init__(monkeypatch, lib)

    def _wrap(self, name, fn):
        inner = super()._wrap(name, fn)

        def call(args, *rest):
            a = args._obj
            self.structs.append((name, type(a).from_buffer_copy(a)))
            return inner(args, *rest)
        return call


def _plans(lib, structs):
    """what each recorded call runs, from its own argument struct (host side): forward (workspace bytes, shares), backward
    (dK/dV form, shares, five_gemm, dS chunks)"""
    out = []
    for name, a in structs:
        if name.startswith("rfa_fwd"):
            out.append((name,) + tuple(BR.fwd_shares(lib, a)))
        else:
            out.append((name,) + tuple(BR.bwd_plan(lib, a)) + tuple(BR.bwd_chunks(lib, a)))
    return out


def _passed_through(spy, first, T):
    """the four calls recorded from index `first` on took the tensors' own storage"""
    calls = spy.seen[first:]
    assert [n[:7] for n, _ in calls] == ["rfa_fwd", "rfa_fwd", "rfa_bwd", "rfa_bwd"], [n for n, _ in calls]
    want = [dict(q="q", k="k", v="v", out="out", lse="lse"), dict(q="q", k="k", v="v", out_acc="out_acc", lse_acc="lse_acc"),
            dict(dout="dout", q="q", k="k", v="v", lse="lse_in", delta="delta_in", dq="dq", dk="dk", dv="dv"),
            dict(dout="dout", q="q", k="k", v="v", lse="lse_in", delta="delta_in", dq_acc="dq_acc", dk_acc="dk_acc", dv_acc="dv_acc")]
    for (name, got), fields in zip(calls, want):
        for f, t in fields.items():
            assert (got[f] or 0) == T[t].data_ptr(), f"{name}: {f} is not the view's own storage — the backend copied it"


# ---- one call: forward (plain, overwritten accumulators) and backward (plain, += / overwritten accumulators) ------------------
def _alloc(specs, far, dev):
    """({name: tensor}, [arena]): the groups named in `far` as views into poisoned arenas, the others plain tensors"""
    T, arenas = {}, []
    for group, ss in specs.items():
        dt = BF if FV.GROUP_ESIZE[group] == 2 else F32
        if group in far:
            views, n = far[group]
            ar = FV.Arena(views, n, dt, dev, output=group.endswith("out"))
            ar.poison()
            arenas.append(ar)
            T.update({name: ar.view(name) for name in views})
        else:
            T.update({s.name: torch.empty(s.shape, dtype=dt, device=dev) for s in ss})
    return T, arenas


def _put(dst, src, packed):
    """src's values into dst; packed: the rows behind R0 only (the rows in front belong to nobody — in a far input view some of
    them hold the alias NaNs)"""
    if not packed:
        dst.copy_(src)
    elif dst.dim() == 2:
        dst[:, R0:] = src[:, R0:]
    else:
        dst[R0:] = src[R0:]


def _run(be, T, kw, pre, derive, acc_init=False):
    be.fwd(T["q"], T["k"], T["v"], out=T["out"], lse=T["lse"], **kw)
    be.fwd(T["q"], T["k"], T["v"], out_acc=T["out_acc"], lse_acc=T["lse_acc"], acc_init=True, **kw)
    if derive:                                            # (the compact run makes the backward's inputs for both runs)
        T["lse_in"].copy_(T["lse"])
        T["delta_in"].zero_()
        be.bwd_preprocess(T["dout"], T["out"], T["delta_in"], **pre)
    be.bwd(T["dout"], T["q"], T["k"], T["v"], T["lse_in"], T["delta_in"], dq=T["dq"], dk=T["dk"], dv=T["dv"], **kw)
    be.bwd(T["dout"], T["q"], T["k"], T["v"], T["lse_in"], T["delta_in"], dq_acc=T["dq_acc"], dk_acc=T["dk_acc"], dv_acc=T["dv_acc"],
           acc_init=acc_init, **kw)
    torch.cuda.synchronize()


def _live(t, packed):
    """the part of a tensor the call addresses: all of it; packed: the rows behind R0"""
    if not packed:
        return t
    return t[:, R0:] if t.dim() == 2 else t[R0:]


def _init_outputs(T, packed):
    for n in OUTPUTS:
        _live(T[n], packed).fill_(0.0 if n in ZERO_INIT else FV.SENTINEL)


class _Shape:
    """the geometry of one case: dense 300 x 520 (the poison file's), dense 512 x 512 (balanced) or the packed batch"""

    def __init__(self, case, packed):
        self.case, self.packed = case, packed
        self.fwd, self.bwd, self.D, self.Dv = case
        self.bal = case == BAL
        if packed:
            self.lead_q, self.lead_k = (CU_Q[-1],), (CU_K[-1],)
        elif self.bal:
            self.lead_q = self.lead_k = (2, 512)
        else:
            self.lead_q, self.lead_k = (GP.DENSE.B, GP.DENSE.lq), (GP.DENSE.B, GP.DENSE.lk)
        self.specs = FV.call_specs(self.lead_q, self.lead_k, H, Hk, self.D, self.Dv, packed)

    def kw(self, dev):
        kw = dict(softmax_scale=self.D ** -0.5, causal=True)
        if self.packed:
            cq, ck = (torch.tensor(c, dtype=torch.int32, device=dev) for c in (CU_Q, CU_K))
            mq, mk = (max(b - a for a, b in zip(c, c[1:])) for c in (CU_Q, CU_K))
            kw.update(cu_seqlens_q=cq, cu_seqlens_k=ck, max_seqlen_q=mq, max_seqlen_k=mk)
        return kw

    def set_forms(self, monkeypatch):
        if self.bal:
            monkeypatch.setenv("RFA_DKDV_WIDE", "2")
        else:
            GP._set_forms(monkeypatch, self.fwd, self.bwd)

    def inputs(self, dev):
        """{q, k, v, dout}: N(0, 1) in bf16; packed: rows R0 .. of tensors whose rows in front are never addressed"""
        gen = torch.Generator().manual_seed(8100 + self.D + 7 * self.Dv + (3 if self.packed else 0) + (5 if self.bal else 0))
        src = {}
        for s in self.specs["io-in"]:
            if self.packed:
                t = torch.zeros(s.shape, dtype=BF, device=dev)
                t[R0:] = torch.randn(s.shape[0] - R0, *s.shape[1:], generator=gen).to(BF).to(dev)
            else:
                t = torch.randn(*s.shape, generator=gen).to(BF).to(dev)
            src[s.name] = t
        return src

    def reference(self, src):
        """fp64 (out, lse, dq, dk, dv) of the live rows (a value head dim of its own: the gradients by autograd through the
        forward — tests/_blockref.py's backward formula is written for one head dim)"""
        auto = self.Dv != self.D
        if not self.packed:
            return BLK.attention(src["q"], src["k"], src["v"], dout=src["dout"], causal=True, autograd=auto)
        cq, ck = [c - R0 for c in CU_Q], [c - R0 for c in CU_K]
        return BLK.attention(src["q"][R0:], src["k"][R0:], src["v"][R0:], dout=src["dout"][R0:], cu_seqlens_q=cq, cu_seqlens_k=ck,
                             causal=True, autograd=auto)

    def live(self, name, t):
        return _live(t, self.packed)

    def check_forms(self, lib, plans):
        """the compact run ran the forms the case names (host side)"""
        if not self.packed and not self.bal:
            GP._check_forms(lib, self.fwd, self.bwd, self.D, self.Dv)
            return
        (_, nbytes, ns), _, (_, f, bns, five, *_), _ = plans
        if self.bal:
            assert f == BR.DKDV_BAL, plans
            return
        if self.Dv == self.D and self.D in (128, 64):
            want = GP.FWD_ENV[self.fwd][1]
            assert want is None or (ns == want and (nbytes > 0) == (want > 1)), (self.case, nbytes, ns)
        if self.bwd != "auto":
            wform, wns, wfive = BR.BWD_FORMS[self.bwd][1]
            if self.D > 128:
                wform = wns = None                                # (head dims above 128: one dK/dV form; the name asks for the dQ form)
            assert (wform is None or f == wform) and (wns is None or bns == wns) and (wfive is None or five == wfive), (self.case, f, bns, five)


_CLEAN = {}                                     # (case, packed, feature) -> the compact run: its inputs, outputs and plans; the last one only


def _clean_run(be, monkeypatch, shape, dev, kw_extra=None, key_extra=None, reference=None, derive_src=None):
    """the compact run of a case (cached), checked once against fp64 by the rows of tests/_tol.py"""
    key = (shape.case, shape.packed, key_extra)
    if key in _CLEAN:
        return _CLEAN[key]
    _CLEAN.clear()                              # (the kinds and sides of one case run back to back)
    _WALK.clear()
    src = shape.inputs(dev)
    if derive_src is not None:
        src.update(derive_src(src))
    T, _ = _alloc(shape.specs, {}, dev)
    for n in ("q", "k", "v", "dout"):
        T[n] = src[n]
    _init_outputs(T, shape.packed)
    spy = _Spy(monkeypatch, be.lib)
    kw = dict(shape.kw(dev), **(kw_extra(src) if kw_extra else {}))
    pre = {n: kw[n] for n in ("cu_seqlens_q", "max_seqlen_q") if n in kw}
    _run(be, T, kw, pre, derive=True, acc_init=shape.bal)
    plans = _plans(be.lib, spy.structs)
    assert all(bool(torch.isfinite(shape.live(n, T[n])).all()) for n in OUTPUTS), "the compact run is not finite"
    ref = (reference or shape.reference)(src)
    bad = []
    for names, r, kind in ((("out", "out_acc"), ref[0], "out"), (("lse", "lse_acc"), ref[1], "lse"), (("dq", "dq_acc"), ref[2], "grad"),
                           (("dk", "dk_acc"), ref[3], "grad"), (("dv", "dv_acc"), ref[4], "grad")):
        for n in names:
            bad += _tol.failures(f"far.compact.{'-'.join(map(str, shape.case))}.{key_extra or ('packed' if shape.packed else 'dense')}.{n}",
                                 shape.live(n, T[n]), r, kind)
    assert not bad, "; ".join(bad)
    src.update(lse_in=T["lse_in"], delta_in=T["delta_in"])
    _CLEAN[key] = (src, {n: T[n] for n in OUTPUTS}, plans)
    return _CLEAN[key]


def _far_run(be, monkeypatch, shape, kind, side, dev, src, clean, plans, kw_extra=None, extra=None, far_src=None):
    """the same call with one side's tensors far: the compact run's bits, its plan, the views' own pointers, sentinels intact"""
    far = FV.far_case(kind, side, shape.lead_q, shape.lead_k, H, Hk, shape.D, shape.Dv, extra)
    _need(FV.arena_bytes(far) + (6 * GiB if shape.packed else GiB))
    T, arenas = _alloc(shape.specs, far, dev)
    try:
        for n in ("q", "k", "v", "dout", "lse_in", "delta_in"):
            _put(T[n], src[n], shape.packed)
        _init_outputs(T, shape.packed)
        held = dict(src)
        if far_src is not None:                               # a feature's own operands inside a far arena
            held.update(far_src(arenas, src))
        spy = _Spy(monkeypatch, be.lib)
        first = len(spy.seen)
        kw = dict(shape.kw(dev), **(kw_extra(held) if kw_extra else {}))
        _run(be, T, kw, {}, derive=False, acc_init=shape.bal)
        _passed_through(spy, first, T)
        assert _plans(be.lib, spy.structs) == plans, "the far call got another plan than its compact twin"
        for n in OUTPUTS:
            a, b = shape.live(n, T[n]), shape.live(n, clean[n])
            assert torch.equal(a, b), f"{kind}.{side}: {n} differs from the compact run ({int((a != b).sum())} elements)"
        for ar in arenas:
            ar.check()
    finally:
        del T, arenas
        _give_back(be)


def _form_params():
    ps = []
    for case in DENSE_CASES:
        for kind in ("batch", "head"):
            for side in FV.SIDES:
                core = (case, kind, side) == (("4x32", "5gemm", 128, 128), "batch", "outputs")
                ps.append(pytest.param(case, kind, side, id=_case_id(case, kind, side), marks=[] if core else [_EXT]))
    for case in GP.PACKED_CASES:
        for side in FV.SIDES:
            ps.append(pytest.param(case, "packed", side, id=_case_id(case, "packed", side), marks=[_EXT]))
    return ps


def _case_id(case, kind, side):
    return f"{case[0]}-{case[1]}-d{case[2]}" + (f"v{case[3]}" if case[3] != case[2] else "") + f"-{kind}-{side}"


@pytest.mark.parametrize("case,kind,side", _form_params())
def test_far_views_in_every_kernel_form(monkeypatch, case, kind, side):
    """every entry of the poison tests' CASES (forward 8 x 32 / 4 x 32 / persistent / 3 split-KV shares, backward 7-GEMM / 5-GEMM /
    128-key / 256-key in 2 shares, head dims 128, 64, 80, 192, 192 / 128) and the balanced dK/dV schedule (512 x 512 causal, dense
    kinds: packed input does not run it), with batch entry 1 / the last K/V head group / every packed sequence past 2^31 elements,
    once on the input side (q, k, v, dout, lse, delta) and once on the output side (out, dq, dk, dv, lse, the fp32 accumulators)"""
    be, dev = GF._be(), GF._dev()
    shape = _Shape(case, kind == "packed")
    shape.set_forms(monkeypatch)
    be.release_scratch()
    try:
        src, clean, plans = _clean_run(be, monkeypatch, shape, dev)
        shape.check_forms(be.lib, plans)
        _far_run(be, monkeypatch, shape, kind, side, dev, src, clean, plans)
    finally:
        _give_back(be)


# ---- feature instances: the batch kind, inputs far and outputs far ------------------------------------------------------------
FEATURE_CASE = ("auto", "auto", 128, 128)
RR_K0 = 40


def _rr_pattern(dev):
    """int32 (B, Sq) global key positions: every row sees at least the keys [start, start + 150) it is allowed to by the band"""
    i = torch.arange(GP.DENSE.lq)
    start = torch.stack([(i * 3) % 200, (i * 7) % 170]) + RR_K0
    end = start + torch.tensor([[150], [233]])
    return start.to(torch.int32).to(dev).contiguous(), end.to(torch.int32).to(dev).contiguous()


def _feature(name):
    """(keywords of the call from the held tensors, extra far specs, the fp64 reference, how the extra tensors are made)"""
    from oracle.flash_attn_ref import drop_rescale

    g = GP.DENSE
    ref = lambda s, **kw: BLK.attention(s["q"], s["k"], s["v"], dout=s["dout"], causal=True, **kw)
    if name == "window":
        return (lambda s: dict(window=(37, -1))), None, (lambda s: ref(s, window=(37, -1))), None
    if name == "dropout":
        drop = (0.2, 1234567, 0, 0, 0)
        keep = lambda: [BLK.keep_mask(drop, b, H, g.lq, g.lk) for b in range(g.B)]
        return (lambda s: dict(dropout=drop)), None, (lambda s: ref(s, keep=keep(), rescale=drop_rescale(drop[0]))), None
    if name == "softcap":
        return (lambda s: dict(softcap=2.0)), None, (lambda s: ref(s, softcap=2.0)), None
    if name == "alibi":
        make = lambda s: dict(slopes=(torch.arange(1, g.B * H + 1, dtype=F32, device=s["q"].device) * 0.03).view(g.B, H))
        return ((lambda s: dict(alibi=(s["slopes"], 0))), {"f32-in": [FV.Spec("slopes", (g.B, H), "bh", "q")]},
                (lambda s: ref(s, slopes=s["slopes"])), make)
    if name == "row_ranges":
        import _rowrange_backend as RB

        def make(s):
            start, end = _rr_pattern(s["q"].device)
            return dict(rr_start=start, rr_end=end)

        def rr_ref(s):
            mask = RB.block_mask(s["rr_start"], s["rr_end"], RR_K0, g.lk, True)
            return RB.single_device(*(s[n].cpu() for n in ("q", "k", "v", "dout")), mask)
        extra = {"f32-in": [FV.Spec("rr_start", (g.B, g.lq), "bs", "q"), FV.Spec("rr_end", (g.B, g.lq), "bs", "q")]}
        return (lambda s: dict(row_ranges=(s["rr_start"], s["rr_end"], RR_K0))), extra, rr_ref, make
    raise ValueError(name)


@pytest.mark.extended
@pytest.mark.parametrize("name,side", [(n, s) for n in ("window", "dropout", "alibi", "softcap", "row_ranges") for s in FV.SIDES])
def test_far_batch_entry_with_a_feature(monkeypatch, name, side):
    """the kWin, kDrop (identity position map), kBias (slopes (B, H) with a far batch stride), kCap (softcap 2.0) and kRng
    (start / end with a far batch stride) instances on the dense 300 x 520 call: batch entry 1 past 2^31 elements"""
    be, dev = GF._be(), GF._dev()
    shape = _Shape(FEATURE_CASE, False)
    kw_extra, extra, reference, make = _feature(name)

    def far_src(arenas, src):
        """the feature's own tensors as views into the far fp32 input arena (int32 shares its element size)"""
        out = {}
        ar = next(a for a in arenas if "lse_in" in a.views)
        for n in (s.name for s in extra["f32-in"]):
            v = ar.view(n)
            v = v.view(src[n].dtype) if src[n].dtype != F32 else v
            v.copy_(src[n])
            out[n] = v
            assert v.stride(0) > 2 ** 31
        return out

    be.release_scratch()
    try:
        src, clean, plans = _clean_run(be, monkeypatch, shape, dev, kw_extra, name, reference, make)
        _far_run(be, monkeypatch, shape, "batch", side, dev, src, clean, plans, kw_extra,
                 extra if side == "inputs" else None, far_src if (side == "inputs" and extra) else None)
    finally:
        _give_back(be)


# ---- max_logit and the Δ preprocess ------------------------------------------------------------------------------------------
def _aux_arenas(case, dev):
    """{group: poisoned Arena} of one auxiliary case (tests/_farview.py: aux_layouts)"""
    lay = FV.aux_layouts()[case]
    _need(sum(n * es for _, n, es, _ in lay.values()) + GiB)
    arenas = {}
    for g, (views, n, es, out) in lay.items():
        arenas[g] = FV.Arena(views, n, BF if es == 2 else F32, dev, out)
        arenas[g].poison()
    return arenas


def _far_copy(arena, name, src):
    v = arena.view(name)
    assert tuple(v.shape) == tuple(src.shape), (name, v.shape, src.shape)
    v.copy_(src)
    return v


def _rand(gen, *shape, dtype=BF, dev=None):
    return torch.randn(*shape, generator=gen).to(dtype).to(dev)


@pytest.mark.extended
def test_max_logit_of_a_far_batch_entry():
    """q and k with batch entry 1 past 2^31 elements (the result is an (H,) vector behind a host-computed pointer: nothing of it
    can be far): the compact call's bits, and the fp64 maximum within the bound of tests/_maxlogit_backend.py"""
    import _maxlogit_backend as ML

    be, dev = GF._be(), GF._dev()
    gen = torch.Generator().manual_seed(8300)
    q, k = _rand(gen, 2, 300, 4, 128, dev=dev), _rand(gen, 2, 520, 2, 128, dev=dev)
    scale = 128 ** -0.5
    try:
        ar = _aux_arenas("max_logit", dev)
        qf, kf = _far_copy(ar["io"], "q", q), _far_copy(ar["io"], "k", k)
        m_c, m_f = (torch.full((4,), 123.0, dtype=F32, device=dev) for _ in range(2))
        be.max_logit(q, k, m_c, softmax_scale=scale, accumulate=False, causal=True)
        be.max_logit(qf, kf, m_f, softmax_scale=scale, accumulate=False, causal=True)
        torch.cuda.synchronize()
        assert torch.equal(m_f, m_c), (m_f, m_c)
        ref = ML.head_max(ML.row_max(q, k, scale, causal=True))
        ML.close(m_c, ref, ML.tolerance(128, scale, ML.head_max(ML.row_max(q, k, scale, causal=True, absolute=True))))
    finally:
        ar = qf = kf = None
        _give_back(be)


@pytest.mark.extended
def test_preprocess_with_far_operands_with_and_without_dlse():
    """delta = rowsum(dout * out) [- dlse] with dout, out, dlse and delta all far (batch entry 1): the compact call's bits, the
    sentinels around the far delta intact; the compact call: delta - dlse exactly (one correctly rounded fp32 subtraction) and
    |delta - fp64| <= (D + 2) 2^-23 sum |dout out| per row (a D-term fp32 sum of exact products, any order, factor 2)"""
    be, dev = GF._be(), GF._dev()
    gen = torch.Generator().manual_seed(8301)
    B, S, Hh, D = 2, 300, 3, 128
    do, o = _rand(gen, B, S, Hh, D, dev=dev), _rand(gen, B, S, Hh, D, dev=dev)
    dlse = _rand(gen, B, Hh, S, dtype=F32, dev=dev)
    try:
        ar = _aux_arenas("preprocess", dev)
        dof, of = _far_copy(ar["io"], "dout", do), _far_copy(ar["io"], "out", o)
        dlf = _far_copy(ar["f32"], "dlse", dlse)
        delta_f = ar["f32"].view("delta")
        plain = torch.full((B, Hh, S), 7.0, device=dev)
        got = torch.full((B, Hh, S), 7.0, device=dev)
        be.bwd_preprocess(do, o, plain)
        be.bwd_preprocess(do, o, got, dlse=dlse)
        assert torch.equal(got, plain - dlse)
        exact = (do.double() * o.double()).sum(-1).permute(0, 2, 1)
        bound = (D + 2) * 2.0 ** -23 * (do.double() * o.double()).abs().sum(-1).permute(0, 2, 1)
        assert bool(((plain.double() - exact).abs() <= bound).all()), float(((plain.double() - exact).abs() / bound).max())
        for want, extra in ((plain, {}), (got, dict(dlse=dlf))):
            delta_f.fill_(7.0)
            be.bwd_preprocess(dof, of, delta_f, **extra)
            torch.cuda.synchronize()
            assert torch.equal(delta_f, want), f"far delta differs from the compact run ({'with' if extra else 'without'} dlse)"
            ar["f32"].check()
    finally:
        ar = dof = of = dlf = delta_f = None
        _give_back(be)


# ---- auxiliary kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.extended
def test_sum_slots_slot_stride_past_2_31_into_a_far_slice():
    """rfa_sum_slots: two io-dtype slots 2^31 + elements apart, summed in fp32 into a destination whose batch entry 1 is far:
    bit-exact against the same fp32 sum rounded once (the formula of tests/test_gpu_kernels.py)"""
    be, dev = GF._be(), GF._dev()
    gen = torch.Generator().manual_seed(8302)
    slots = _rand(gen, 2, 2, 300, 3, 128, dev=dev)
    try:
        ar = _aux_arenas("sum_slots", dev)
        sf = _far_copy(ar["slots"], "slots", slots)
        dst = ar["dst"].view("dst")
        dst.fill_(7.0)
        assert sf.stride(0) > 2 ** 31 and dst.stride(0) > 2 ** 31
        be.sum_slots(sf, dst)
        torch.cuda.synchronize()
        assert torch.equal(dst, slots.float().sum(0).to(BF))
        ar["dst"].check()
    finally:
        ar = sf = dst = None
        _give_back(be)


@pytest.mark.extended
def test_merge_with_far_lse_strides():
    """rfa_merge (update_out_and_lse): out_acc, lse_acc and block_lse in one far fp32 arena, block_out in a far io arena — first
    block with acc_init, second merged in: the compact calls' bits, and the reference's sigmoid / logsigmoid formula within the
    1e-5 of tests/test_gpu_kernels.py"""
    import torch.nn.functional as Fn

    be, dev = GF._be(), GF._dev()
    gen = torch.Generator().manual_seed(8303)
    B, S, Hh, D = 2, 300, 3, 128
    blocks = [_rand(gen, B, S, Hh, D, dev=dev) for _ in range(2)]
    lses = [(_rand(gen, B, Hh, S, dtype=F32, dev=dev) * 4) for _ in range(2)]
    try:
        ar = _aux_arenas("merge", dev)
        oc, lc = torch.full((B, S, Hh, D), 7.0, device=dev), torch.full((B, Hh, S), 7.0, device=dev)
        of, lf, bl = (ar["f32"].view(n) for n in ("out_acc", "lse_acc", "block_lse"))
        bo = ar["io"].view("block_out")
        of.fill_(7.0)
        lf.fill_(7.0)
        for i, (b, l) in enumerate(zip(blocks, lses)):
            be.merge(oc, lc, b, l, acc_init=i == 0)
            bo.copy_(b)
            bl.copy_(l)
            be.merge(of, lf, bo, bl, acc_init=i == 0)
        torch.cuda.synchronize()
        assert torch.equal(of, oc) and torch.equal(lf, lc)
        ar["f32"].check()
        t = lambda l: l.transpose(-2, -1).unsqueeze(-1)
        ro, rl = blocks[0].float(), t(lses[0])
        ro, rl = ro - torch.sigmoid(t(lses[1]) - rl) * (ro - blocks[1].float()), rl - Fn.logsigmoid(rl - t(lses[1]))
        assert float((oc - ro).abs().max()) <= 1e-5 + 1e-5 * float(ro.abs().max())
        assert float((t(lc) - rl).abs().max()) <= 1e-5 + 1e-5 * float(rl.abs().max())
    finally:
        ar = of = lf = bl = bo = None
        _give_back(be)


@pytest.mark.extended
def test_merge_pair_forward_and_backward_with_far_inputs():
    """rfa_merge_pair / rfa_merge_pair_bwd (csrc/rfa_mergepair.hip) with out_a, out_b, dout and lse_a, lse_b, dlse far (the
    backend allocates the results itself): the compact calls' bits; the compact calls against fp64 autograd by the bounds of
    tests/test_gpu_lse_grad.py (empty-row cases included)"""
    import _lsegrad_worker as LW

    be, dev = GF._be(), GF._dev()
    ins = LW.merge_inputs(2, 300, 3, 128, BF, False)
    oa, la, ob, lb, do, dl = (t.to(dev) for t in ins)
    try:
        ar = _aux_arenas("merge_pair", dev)
        far = [_far_copy(ar["io" if t.dtype == BF else "f32"], n, t)
               for n, t in (("out_a", oa), ("lse_a", la), ("out_b", ob), ("lse_b", lb), ("dout", do), ("dlse", dl))]
        got_c = list(be.merge_pair(oa, la, ob, lb)) + list(be.merge_pair_bwd(do, dl, oa, la, ob, lb))
        got_f = list(be.merge_pair(*far[:4])) + list(be.merge_pair_bwd(far[4], far[5], *far[:4]))
        torch.cuda.synchronize()
        for nm, a, b in zip(("out", "lse", "dout_a", "dlse_a", "dout_b", "dlse_b"), got_f, got_c):
            assert torch.equal(a, b), f"merge_pair: {nm} differs from the compact run"
        errs, _ = LW.merge_failures("far.merge_pair", [t.cpu() for t in got_c], LW.merge_reference(*ins))
        errs += LW.empty_row_failures("far.merge_pair", [t.cpu() for t in got_c], ins, False, 2, 300)
        assert not errs, "\n".join(errs)
    finally:
        ar = far = None
        _give_back(be)


@pytest.mark.extended
def test_seq_head_copy_with_a_far_source():
    """rfa_seq_head_copy (PACK, two tensors): the second source's batch entry 1 past 2^31 elements; bit for bit the torch
    indexing of tests/_usp_backend.py"""
    import _usp_backend as UB

    be, dev = GF._be(), GF._dev()
    gen = torch.Generator().manual_seed(8304)
    near, local = _rand(gen, 2, 64, 4, 128, dev=dev), _rand(gen, 2, 64, 4, 128, dev=dev)
    try:
        ar = _aux_arenas("seq_head", dev)
        lf = _far_copy(ar["io"], "local", local)
        got, want = (torch.full((2 * local.numel() + 64,), 3.0, dtype=BF, device=dev) for _ in range(2))
        be.seq_head_copy(UB.PACK, UB.CONTIGUOUS, 2, [near, lf], got)
        UB.torch_copy(UB.PACK, UB.CONTIGUOUS, 2, [near, local], want)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    finally:
        ar = lf = None
        _give_back(be)


@pytest.mark.extended
def test_sink_kernels_with_a_far_lse():
    """rfa_sink_apply / rfa_sink_grad with out, dout and lse far: the compact calls' bits; the compact calls by the criteria of
    tests/test_gpu_sinks.py (out, lse kinds; dsink within DSINK_TOL of the fp64 formula on the stored out', lse')"""
    import _sinkref as SK

    be, dev = GF._be(), GF._dev()
    do, o, l, s = SK.kernel_inputs(2, 300, 3, 128, BF, False)
    dod, od, ld, sd = (t.to(dev) for t in (do.contiguous(), o, l, s))
    try:
        ar = _aux_arenas("sink", dev)
        of, dof, lf = _far_copy(ar["io"], "out", od), _far_copy(ar["io"], "dout", dod), _far_copy(ar["f32"], "lse", ld)
        o2, l2 = be.sink_apply(od, ld, sd, varlen=False)
        o2f, l2f = be.sink_apply(of, lf, sd, varlen=False)
        assert torch.equal(o2f, o2) and torch.equal(l2f, l2)
        ref_o, ref_l = SK.apply_formula(o, l, s)
        _tol.compare("far.sink_apply.lse", l2, ref_l, "lse")
        _tol.compare("far.sink_apply.out", o2, ref_o, "out")
        d1 = be.sink_grad(dod, o2, l2, sd, varlen=False)
        lf.copy_(l2)                                                   # (the far lse now holds lse')
        of.copy_(o2)
        d2 = be.sink_grad(dof, of, lf, sd, varlen=False)
        torch.cuda.synchronize()
        assert torch.equal(d1, d2)
        ref_d, norm = SK.dsink_formula(do, o2.cpu(), l2.cpu(), s)
        err = ((d1.cpu().double() - ref_d).abs() / norm.clamp_min(1e-300)).max().item()
        assert err <= SK.DSINK_TOL, (err, SK.DSINK_TOL)
    finally:
        ar = of = dof = lf = None
        _give_back(be)


@pytest.mark.extended
def test_cast_of_more_than_2_31_elements():
    """rfa_cast, n = 2^31 + 24: the first and the last MiB of the result and 64 random 4 KiB windows are the fp32 values
    rounded to bf16 (only those windows of the source are given values; the rest is whatever the allocation held)"""
    be, dev = GF._be(), GF._dev()
    n = FV.CAST_N
    _need(n * 6 + GiB)
    gen = torch.Generator().manual_seed(8305)
    try:
        src = torch.empty(n, dtype=F32, device=dev)
        mib, win = (1 << 20) // 2, 4096 // 2                           # elements of the bf16 result
        starts = [0, n - mib] + [int(x) // 8 * 8 for x in torch.randint(mib, n - mib - win, (64,), generator=gen)]
        spans = [(a, mib if i < 2 else win) for i, a in enumerate(starts)]
        for a, w in spans:
            src[a:a + w] = torch.randn(w, generator=gen).to(dev) * 3
        dst = be.cast(src, BF)
        torch.cuda.synchronize()
        assert dst.numel() == n and spans[1][0] + spans[1][1] == n > 2 ** 31          # (the last MiB ends behind element 2^31)
        for a, w in spans:
            assert torch.equal(dst[a:a + w], src[a:a + w].to(BF)), f"cast: window at {a}"
    finally:
        src = dst = None
        _give_back(be)


@pytest.mark.extended
def test_lse_flatten_and_unflatten_with_a_packed_head_stride_past_2_31():
    """rfa_lse_flatten into, and rfa_lse_unflatten out of, a packed (H, T) tensor whose head stride is 2^31 + elements: the
    re-layout is bit-identical (cu [0, 15, 156, 529], the reference's own fixture), the sentinels around head 1 intact"""
    from ring_flash_attn import _C
    from ring_flash_attn.backend import _stream

    be, dev = GF._be(), GF._dev()
    cu = [0, 15, 156, 529]
    cut = torch.tensor(cu, dtype=torch.int32, device=dev)
    maxlen = max(b - a for a, b in zip(cu[:-1], cu[1:]))
    lse = torch.randn(3, 2, maxlen, device=dev)
    try:
        ar = _aux_arenas("lse_relayout", dev)
        flat = ar["f32"].view("packed")
        flat.fill_(7.0)
        assert flat.stride(0) > 2 ** 31
        _C.check(be.lib.rfa_lse_flatten(flat.data_ptr(), lse.data_ptr(), cut.data_ptr(), 3, 2, maxlen, flat.stride(0), flat.stride(1),
                                        _stream(lse)), "rfa_lse_flatten")
        torch.cuda.synchronize()
        assert torch.equal(flat, torch.cat([lse[i, :, : cu[i + 1] - cu[i]] for i in range(3)], dim=1))
        ar["f32"].check()
        un = be.lse_unflatten(flat.transpose(0, 1), cut, maxlen)
        for i in range(3):
            n = cu[i + 1] - cu[i]
            assert torch.equal(un[i, :, :n], lse[i, :, :n])
    finally:
        ar = flat = None
        _give_back(be)


# ---- long walks inside one sequence ----------------------------------------------------------------------------------------------
WALK_TARGET = 12.0                                # the planted logit: weight ~ 0.25 against 262144 keys of logits ~ N(0, 1.1)
_WALK = {}


def _walk_case(D, Dv, causal, dev):
    """(q, k, v, do, targets, fp64 reference) of 256 rows against 262144 keys.  With N(0, 1) inputs every probability is ~ 4e-6 and
    every dK / dV row ~ 1e-4, far below the absolute terms of the tolerance rows: the comparison would see nothing.  So row i is
    aligned with ONE key t_i (q_i = c k_t with scale q_i . k_t = 12): out_i, dq_i and dk / dv of row t_i are O(0.1 .. 1) and a tile
    fetched from a wrong address changes them by that much.  The targets sit where addresses go wrong: the last 256 keys, the
    first 256 (where a wrapped offset lands), around key 131072 (the 2^31-byte line of 8192-wide rows), and spread over the rest."""
    key = (D, Dv, causal)
    if key in _WALK:
        return _WALK[key]
    _WALK.clear()
    _CLEAN.clear()
    Sq, Sk = FV.WALK_SQ, FV.WALK_SK
    gen = torch.Generator(device=dev).manual_seed(8400 + D + Dv)
    k = torch.randn(1, Sk, 1, D, generator=gen, device=dev).to(BF)
    v = torch.randn(1, Sk, 1, Dv, generator=gen, device=dev).to(BF)
    do = torch.randn(1, Sq, 1, Dv, generator=gen, device=dev).to(BF)
    i = torch.arange(Sq, device=dev)
    last_visible = i + (Sk - Sq)
    t = torch.where(i % 4 == 0, last_visible, torch.where(i % 4 == 1, i, torch.where(i % 4 == 2, Sk // 2 - Sq // 2 + i, (i * 1021) % (Sk - 1024) + 512)))
    kt = k[0, t, 0].float()
    q = (kt * (WALK_TARGET / (D ** -0.5 * (kt * kt).sum(-1, keepdim=True)))).to(BF).view(1, Sq, 1, D)
    ref = BLK.attention(q, k, v, dout=do, causal=causal, autograd=D != Dv)
    _WALK[key] = (q, k, v, do, t, ref)
    return _WALK[key]


def _walk_params():
    ps = []
    pairs = [("auto", "7gemm"), ("8x32", "5gemm"), ("auto", "dkdv128"), ("8x32", "dkdv256-1")]
    for causal in (True, False):
        for fwd, bwd in pairs:
            ps.append(pytest.param(FV.ROW_W, fwd, bwd, 128, 128, causal, marks=[_EXT]))
        for D, Dv in ((192, 192), (192, 128)):
            ps.append(pytest.param(FV.ROW_W, "auto", "auto", D, Dv, causal, marks=[_EXT]))
    # rows 8200 elements apart: the same walk ACROSS 2^31 elements / 2^32 bytes (8192-wide rows end 8065 elements short of it);
    # the first of them is the section's one case of the core tier — the only kind of walk that crosses the line
    ps += [pytest.param(FV.ROW_W + 8, "auto", "5gemm", 128, 128, True),
           pytest.param(FV.ROW_W + 8, "8x32", "dkdv256-1", 128, 128, False, marks=[_EXT]),
           pytest.param(FV.ROW_W + 8, "auto", "auto", 192, 128, True, marks=[_EXT])]
    return ps


@pytest.mark.parametrize("width,fwd,bwd,D,Dv,causal", _walk_params())
def test_few_rows_against_keys_up_to_the_2_32_byte_line(monkeypatch, width, fwd, bwd, D, Dv, causal):
    """Sq 256, Sk 262144, H = Hk = 1: k and v are the last columns of one arena of Sk rows of `width` elements, dk and dv of a
    second one — the running tile pointers and j * tile * row_stride walk to 2^32 bytes (width 8192) and across them (8200).
    Forward: the library's choice (asserted to be a split-KV plan) or the 8 x 32 form; backward: 7-GEMM, 5-GEMM, 128-key and
    256-key dK/dV; head dims 192 and 192 / 128 under the library's choice.  Against the full fp64 reference (256 x 262144
    scores) by the rows of tests/_tol.py: out, lse, dq, dk and dv whole, and dk / dv once more on the 256 target rows alone."""
    be, dev = GF._be(), GF._dev()
    Sq, Sk = FV.WALK_SQ, FV.WALK_SK
    _need(2 * Sk * width * 2 + 6 * GiB)
    GF._setenv(monkeypatch, GP.FWD_ENV[fwd][0])
    GF._setenv(monkeypatch, GP._bwd_env(bwd))
    be.release_scratch()
    try:
        q, k, v, do, targets, ref = _walk_case(D, Dv, causal, dev)
        ck, cv = (width - 2 * 192, width - 192) if D > 128 else (width - 256, width - 128)
        arenas = [torch.empty(Sk * width, dtype=BF, device=dev) for _ in range(2)]
        view = lambda ar, col, d: torch.as_strided(ar, (1, Sk, 1, d), (Sk * width, width, d, 1), col)
        kf, vf, dk, dv = view(arenas[0], ck, D), view(arenas[0], cv, Dv), view(arenas[1], ck, D), view(arenas[1], cv, Dv)
        assert FV.reach_bytes(FV.walk_view(width, ck, D)) == (Sk - 1) * width * 2 + 2 * D - 1
        kf.copy_(k)
        vf.copy_(v)
        dk.fill_(FV.SENTINEL)
        dv.fill_(FV.SENTINEL)
        out, dq = torch.full((1, Sq, 1, Dv), FV.SENTINEL, dtype=BF, device=dev), torch.full((1, Sq, 1, D), FV.SENTINEL, dtype=BF, device=dev)
        lse, delta = torch.full((1, 1, Sq), FV.SENTINEL, device=dev), torch.zeros((1, 1, Sq), device=dev)
        kw = dict(softmax_scale=D ** -0.5, causal=causal)
        spy = _Spy(monkeypatch, be.lib)
        be.fwd(q, kf, vf, out=out, lse=lse, **kw)
        be.bwd_preprocess(do, out, delta)
        be.bwd(do, q, kf, vf, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
        torch.cuda.synchronize()
        spy.assert_passed_through("rfa_fwd", k=kf, v=vf)
        spy.assert_passed_through("rfa_bwd", k=kf, v=vf, dk=dk, dv=dv)
        (fname, nbytes, ns), (bname, f, bns, five, *_) = _plans(be.lib, spy.structs)
        if D == 128:
            want_ns = GP.FWD_ENV[fwd][1]
            assert (ns > 1 and nbytes > 0) if want_ns is None else ns == want_ns, (fwd, ns, nbytes)
            wform, wns, wfive = BR.BWD_FORMS[bwd][1]
            assert (wform is None or f == wform) and (wns is None or bns == wns) and (wfive is None or five == wfive), (bwd, f, bns, five)
        bad = []
        tag = f"walk.w{width}.{fwd}.{bwd}.d{D}v{Dv}.{'causal' if causal else 'full'}"
        for nm, got, r, kind in (("out", out, ref[0], "out"), ("lse", lse, ref[1], "lse"), ("dq", dq, ref[2], "grad")):
            bad += _tol.failures(f"{tag}.{nm}", got, r, kind)
        for nm, got, r in (("dk", dk, ref[3]), ("dv", dv, ref[4])):
            bad += _tol.failures(f"{tag}.{nm}", got, r, "grad", on_device=True)          # (33 M elements: no copy to the host)
            # ... and the rows that carry a target — O(0.1 .. 1) values, where the whole tensor's criteria are dominated by the
            # 262 000 rows that hold next to nothing — by the same rows on their own
            bad += _tol.failures(f"{tag}.{nm}[targets]", got[:, targets], r[:, targets], "grad")
        assert not bad, "; ".join(bad)
    finally:
        arenas = kf = vf = dk = dv = None
        _give_back(be)


@pytest.mark.extended
def test_packed_rows_whose_last_sequences_start_past_2_31_elements(monkeypatch):
    """64 sequences of 4096 rows, then 300, 0 and 77 rows, all on 8192-wide rows: q, k, v, dout in one arena, out, dq, dk, dv in
    another; sequence 64 starts at element 2^31 exactly, through row0 * row_stride alone.  H 4 / Hk 2, D 128, causal, the
    library's own forms.  The first sequence and the last three against fp64 by the rows of tests/_tol.py."""
    be, dev = GF._be(), GF._dev()
    lens = FV.LONG_LENS
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    T, W, D = cu[-1], FV.ROW_W, 128
    _need(2 * T * W * 2 + 12 * GiB)
    be.release_scratch()
    try:
        gen = torch.Generator(device=dev).manual_seed(8401)
        cols = dict(q=(0, H), k=(512, Hk), v=(768, Hk), dout=(1024, H))
        arenas = [torch.empty(T * W, dtype=BF, device=dev) for _ in range(2)]
        view = lambda ar, col, h: torch.as_strided(ar, (T, h, D), (W, D, 1), col)
        ins = {n: view(arenas[0], c, h) for n, (c, h) in cols.items()}
        for t in ins.values():
            t.copy_(torch.randn(t.shape, generator=gen, device=dev).to(BF))
        outs = {n: view(arenas[1], c, h) for n, (c, h) in dict(out=(0, H), dk=(512, Hk), dv=(768, Hk), dq=(1024, H)).items()}
        for t in outs.values():
            t.fill_(FV.SENTINEL)
        assert FV.reach(FV.long_packed_view(0, H, D)) > 2 ** 31 and cu[64] * W == 2 ** 31
        lse, delta = torch.full((H, T), FV.SENTINEL, device=dev), torch.zeros((H, T), device=dev)
        cut = torch.tensor(cu, dtype=torch.int32, device=dev)
        kw = dict(softmax_scale=D ** -0.5, causal=True, cu_seqlens_q=cut, cu_seqlens_k=cut, max_seqlen_q=max(lens), max_seqlen_k=max(lens))
        spy = _Spy(monkeypatch, be.lib)
        be.fwd(ins["q"], ins["k"], ins["v"], out=outs["out"], lse=lse, **kw)
        be.bwd_preprocess(ins["dout"], outs["out"], delta, cu_seqlens_q=cut, max_seqlen_q=max(lens))
        be.bwd(ins["dout"], ins["q"], ins["k"], ins["v"], lse, delta, dq=outs["dq"], dk=outs["dk"], dv=outs["dv"], **kw)
        torch.cuda.synchronize()
        spy.assert_passed_through("rfa_fwd", q=ins["q"], k=ins["k"], v=ins["v"], out=outs["out"])
        spy.assert_passed_through("rfa_bwd", dout=ins["dout"], q=ins["q"], k=ins["k"], v=ins["v"], dq=outs["dq"], dk=outs["dk"], dv=outs["dv"])
        bad = []
        for tag, lo, hi, cus in (("first", 0, cu[1], [0, cu[1]]), ("last3", cu[64], T, [c - cu[64] for c in cu[64:]])):
            ref = BLK.attention(ins["q"][lo:hi], ins["k"][lo:hi], ins["v"][lo:hi], dout=ins["dout"][lo:hi], cu_seqlens_q=cus,
                                cu_seqlens_k=cus, causal=True)
            for nm, got, r, kind in (("out", outs["out"][lo:hi], ref[0], "out"), ("lse", lse[:, lo:hi], ref[1], "lse"),
                                     ("dq", outs["dq"][lo:hi], ref[2], "grad"), ("dk", outs["dk"][lo:hi], ref[3], "grad"),
                                     ("dv", outs["dv"][lo:hi], ref[4], "grad")):
                bad += _tol.failures(f"far.long-packed.{tag}.{nm}", got, r, kind)
        assert not bad, "; ".join(bad)
    finally:
        arenas = ins = outs = None
        _give_back(be)


# ---- the dS hand-off at the top of its 32-bit range ----------------------------------------------------------------------------
DS_S = FV.DS_ROWS                                      # 65504 = 2047 x 32


def _ds_geometry(S):
    return BR.Geometry(f"dense-{S}", "far", S, S, True, BR.NOWIN, 0, 1, None)


def _ds_inputs(Hh, dev):
    gen = torch.Generator(device=dev).manual_seed(8500 + Hh)
    mk = lambda h: torch.randn(1, DS_S, h, 128, generator=gen, device=dev).to(BF)
    return mk(Hh), mk(1), mk(1), mk(Hh)


DS_SAMPLE = [0, 31, 32, 32767, 32768] + [DS_S - 64 + r for r in (0, 9, 18, 27, 36, 45, 54, 63)]


def _ds_sampled_rows(tag, q, k, v, do, out, lse, dq, h):
    """rows of out / lse / dq of query head h against their exact fp64 values: the criterion of
    tests/test_gpu_headline.py::test_max_length_65536_single_gpu (row-relative, plus the element-wise bound).  The sample: rows 0,
    31, 32 (where a wrapped block offset would land), 32767, 32768, and eight rows of the last two 32-row groups (the largest
    offsets)"""
    from test_gpu_headline import _row

    scale = 128 ** -0.5
    for i in DS_SAMPLE:
        kk, vv = k[0, : i + 1, 0].double(), v[0, : i + 1, 0].double()
        s = (kk @ q[0, i, h].double()) * scale
        l = torch.logsumexp(s, 0)
        p = torch.exp(s - l)
        o = p @ vv
        assert abs(float(l) - float(lse[0, h, i])) < 1e-3, (tag, i, float(l), float(lse[0, h, i]))
        _row(f"{tag}.out", i, h, out[0, i, h].double().cpu(), o.cpu())
        dp = vv @ do[0, i, h].double()
        delta = (do[0, i, h].double() * o).sum()
        _row(f"{tag}.dq", i, h, dq[0, i, h].double().cpu(), ((p * (dp - delta) * scale) @ kk).cpu())


def _ds_run(be, q, k, v, do, monkeypatch, spill):
    monkeypatch.setenv("RFA_BWD_DS_SPILL", spill)
    dev = q.device
    Hh = q.shape[2]
    out, lse = torch.empty_like(q), torch.empty((1, Hh, DS_S), device=dev)
    be.fwd(q, k, v, softmax_scale=128 ** -0.5, causal=True, out=out, lse=lse)
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=128 ** -0.5, causal=True, dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def test_ds_handoff_of_65504_rows_just_under_4_gib(monkeypatch):
    """dense causal, B 1, H = Hk = 1, D 128, bf16, 65504 rows: the 5-GEMM form with one head's dS scratch of 2047 * 2048 / 2 blocks
    of 2048 B = 4 292 870 144 B — the dK/dV kernel's 32-bit block offset within 2 MiB of its range (65536 rows run the 7-GEMM
    form: asserted on the host, run by tests/test_gpu_headline.py).  dK and dV are bit-identical between the 5-GEMM and the 7-GEMM
    form (profiles/value_ranges.md); sampled rows of out, lse, dq of both forms, and dk / dv of the last 512 keys, against fp64."""
    import _fullref
    from ring_flash_attn import _C, config
    from test_gpu_headline import all_rows_relative

    be, dev = GF._be(), GF._dev()
    lib = be.lib
    a = BR.bwd_args(_C, _ds_geometry(DS_S), 1, 1, 128, dict(RFA_BWD_DS_SPILL="1"))
    full = lib.rfa_bwd_ds_scratch_bytes(C.byref(a))
    assert full == FV.DS_HEAD_BYTES == 4292870144 and 2 ** 32 - 2 ** 21 <= full < 2 ** 32 and full <= config.get().ds_spill_max_bytes
    assert BR.bwd_plan(lib, a)[2] == 1 and BR.bwd_chunks(lib, a) == (1, 1, 1, full)
    assert BR.bwd_plan(lib, BR.bwd_args(_C, _ds_geometry(65536), 1, 1, 128, dict(RFA_BWD_DS_SPILL="1")))[2] == 0
    _need(full + 4 * GiB)
    be.release_scratch()
    try:
        q, k, v, do = _ds_inputs(1, dev)
        spy = _Spy(monkeypatch, lib)
        out5, lse5, dq5, dk5, dv5 = _ds_run(be, q, k, v, do, monkeypatch, "1")
        assert _plans(lib, spy.structs)[-1][3:] == (1, 1, 1, 1, full), _plans(lib, spy.structs)
        pool = [t for t in be._ds_pool.values() if torch.is_tensor(t)]
        assert [t.numel() for t in pool] == [full]
        out7, lse7, dq7, dk7, dv7 = _ds_run(be, q, k, v, do, monkeypatch, "0")
        assert _plans(lib, spy.structs)[-1][3] == 0
        assert torch.equal(dk5, dk7) and torch.equal(dv5, dv7), "dK / dV differ between the 5-GEMM and the 7-GEMM form"
        assert torch.equal(out5, out7) and torch.equal(lse5, lse7)
        _ds_sampled_rows("s65504.5gemm", q, k, v, do, out5, lse5, dq5, 0)
        _ds_sampled_rows("s65504.7gemm", q, k, v, do, out7, lse7, dq7, 0)
        j = DS_S - 512
        _, fl, fdq, fdk, fdv = _fullref.attention_fwd_bwd_fp64(q[0, j:], k[0], v[0], do[0, j:])
        assert (lse5[0, :, j:].double() - fl).abs().max().item() < 2e-5 + 2e-6 * fl.abs().max().item()
        all_rows_relative("s65504.dq", dq5[0, j:], fdq, _fullref.attention_fwd_bwd_fp64.dq_delta_allowance)
        all_rows_relative("s65504.dk", dk5[0, j:], fdk[j:])
        all_rows_relative("s65504.dv", dv5[0, j:], fdv[j:])
    finally:
        pool = None
        _give_back(be)


@pytest.mark.extended
def test_ds_handoff_second_head_past_4_gib(monkeypatch):
    """the same sequence with H 2, Hk 1 and a scratch limit of 9 GiB: one chunk (asserted on the host), so head 1's share lies
    from 4 292 870 144 B to 8 585 740 288 B behind the scratch pointer — across 2^32.  The sampled rows of both heads against fp64,
    dK / dV bit-identical to the 7-GEMM form."""
    from ring_flash_attn import _C, config

    be, dev = GF._be(), GF._dev()
    lib = be.lib
    full = 2 * FV.DS_HEAD_BYTES
    with config.override(ds_spill_max_bytes=9 * GiB):
        a = BR.bwd_args(_C, _ds_geometry(DS_S), 2, 1, 128, dict(RFA_BWD_DS_SPILL="1"), scratch_bytes=9 * GiB)
        assert lib.rfa_bwd_ds_scratch_bytes(C.byref(a)) == full and BR.bwd_chunks(lib, a) == (1, 1, 2, full)
    _need(2 * full + 4 * GiB)                                      # (the scratch may take at most half of the free memory)
    be.release_scratch()
    try:
        q, k, v, do = _ds_inputs(2, dev)
        spy = _Spy(monkeypatch, lib)
        monkeypatch.setenv("RFA_DS_SPILL_MAX_BYTES", str(9 * GiB))
        out5, lse5, dq5, dk5, dv5 = _ds_run(be, q, k, v, do, monkeypatch, "1")
        assert _plans(lib, spy.structs)[-1][3:] == (1, 1, 1, 2, full), _plans(lib, spy.structs)
        assert [t.numel() for t in be._ds_pool.values() if torch.is_tensor(t)] == [full]
        be.release_scratch()
        torch.cuda.empty_cache()
        out7, lse7, dq7, dk7, dv7 = _ds_run(be, q, k, v, do, monkeypatch, "0")
        assert torch.equal(dk5, dk7) and torch.equal(dv5, dv7), "dK / dV differ between the 5-GEMM and the 7-GEMM form"
        for h in range(2):
            _ds_sampled_rows(f"s65504.h{h}of2", q, k, v, do, out5, lse5, dq5, h)
    finally:
        _give_back(be)


# ---- row strides at and beyond the contract's bound --------------------------------------------------------------------------------
ROW_TOP = 2 ** 21                                     # elements: 256 * 2^21 * 2 = 2^30 bytes, the power of two below the bound (2^22 - 8)


def _stride_inputs(dev):
    gen = torch.Generator().manual_seed(8600)
    return tuple(_rand(gen, 1, n, h, 128, dev=dev) for n, h in ((300, 4), (300, 2), (300, 2), (300, 4)))


def test_row_stride_of_2_21_elements_is_its_compact_twin(monkeypatch):
    """q, k, v, dout as the first 512 / 256 columns of 300 rows that lie 2^21 elements (4 MiB) apart — a 1.2 GiB arena, a row
    stride the contract allows (include/rfa.h: at most 2^22 - 8 for D = 128) and no test came near: forward and backward, bit for
    bit the compact call, the views' own pointers in the struct"""
    be, dev = GF._be(), GF._dev()
    _need(300 * ROW_TOP * 2 + GiB)
    be.release_scratch()
    try:
        src = _stride_inputs(dev)
        arena = torch.empty(300 * ROW_TOP, dtype=BF, device=dev)
        col, wide = 0, []
        for t in src:
            v = torch.as_strided(arena, t.shape, (300 * ROW_TOP, ROW_TOP, 128, 1), col)
            v.copy_(t)
            wide.append(v)
            col += t.shape[2] * 128
        kw = dict(softmax_scale=128 ** -0.5, causal=True)
        res = []
        spy = _Spy(monkeypatch, be.lib)
        for q, k, v, do in (src, wide):
            out, lse = torch.full_like(src[0], FV.SENTINEL), torch.full((1, 4, 300), FV.SENTINEL, device=dev)
            be.fwd(q, k, v, out=out, lse=lse, **kw)
            delta = torch.zeros_like(lse)
            be.bwd_preprocess(do, out, delta)
            dq, dk, dv = (torch.full_like(t, FV.SENTINEL) for t in src[:3])
            be.bwd(do, q, k, v, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
            res.append((out, lse, dq, dk, dv))
        torch.cuda.synchronize()
        spy.assert_passed_through("rfa_fwd", q=wide[0], k=wide[1], v=wide[2])
        spy.assert_passed_through("rfa_bwd", q=wide[0], k=wide[1], v=wide[2], dout=wide[3])
        for nm, a, b in zip(("out", "lse", "dq", "dk", "dv"), *res):
            assert torch.equal(a, b), f"row stride 2^21: {nm} differs from the compact call"
    finally:
        arena = wide = None
        _give_back(be)


@pytest.mark.extended
def test_public_call_beyond_the_row_stride_bound_is_served_through_a_copy(monkeypatch, single_rank_group):
    """k and v with rows 2^22 elements apart (beyond the bound: the library itself answers RFA_ERR_ARGS, tests/test_abi.py) through
    a public function: the backend hands the library a contiguous copy — the spy sees other pointers than the views' — and the
    result is the fp64 attention's by the rows of tests/_tol.py"""
    import ring_flash_attn as R

    be, dev = GF._be(), GF._dev()
    row = 2 ** 22
    _need(2 * 300 * row * 2 + GiB)
    try:
        q, k, v, do = _stride_inputs(dev)
        arena = torch.empty(300 * row, dtype=BF, device=dev)
        kw_, vw = (torch.as_strided(arena, k.shape, (300 * row, row, 128, 1), c) for c in (0, 256))
        kw_.copy_(k)
        vw.copy_(v)
        spy = _Spy(monkeypatch, be.lib)
        qq, kk, vv = q.clone().requires_grad_(True), kw_.detach().requires_grad_(True), vw.detach().requires_grad_(True)
        assert kk.stride(1) == row and kk.data_ptr() == kw_.data_ptr()
        out, lse, _ = R.ring_flash_attn_func(qq, kk, vv, causal=True, return_attn_probs=True)
        out.backward(do)
        torch.cuda.synchronize()
        for prefix in ("rfa_fwd", "rfa_bwd"):
            got = spy.last(prefix)
            assert got["k"] not in (0, None, kw_.data_ptr()) and got["v"] not in (0, None, vw.data_ptr()), "an over-bound view reached the library"
            assert got["q"] == qq.data_ptr()
        ref = BR.band_ref(q, k, v, do, True, BR.NOWIN, 0)
        bad = []
        for nm, got, r, kind in (("out", out, ref[0], "out"), ("lse", lse, ref[1], "lse"), ("dq", qq.grad, ref[2], "grad"),
                                 ("dk", kk.grad, ref[3], "grad"), ("dv", vv.grad, ref[4], "grad")):
            bad += _tol.failures(f"far.over-bound-stride.{nm}", got, r, kind)
        assert not bad, "; ".join(bad)
    finally:
        arena = kw_ = vw = kk = vv = None
        _give_back(be)
