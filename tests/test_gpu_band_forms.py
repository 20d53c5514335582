"""Shifted attention bands (`mask_shift`, include/rfa.h ABI 7) in every kernel form against fp64: the block geometries
of tests/_bandref.py — one visible element in a corner, one masked element, bounds dropped by one, diagonals on both
sides of every 32 / 64 boundary and of both signs, bands narrower than a workgroup, split-KV shares outside the band,
live bands next to numbers beyond 2^28 — through the forward forms (8 x 32, 4 x 32, windowed instances, split-KV), the
backward forms (7-GEMM, 5-GEMM with the triangular dS scratch, whole and in chunks, the 128-key and the shared-range
256-key dK/dV plans, windowed instances, two-phase and overwrite calls), plain and fp32 accumulate outputs, each
compared with the explicit-mask fp64 attention of tests/_bandref.py through tests/_tol.py (kinds out, lse, grad).
Every case first asserts on the host that the call runs the form it names (tests/test_band_cases_cpu.py checks the same
without a device).  Rows without a key: out == 0 exactly, lse +inf (plain) / -inf (accumulators); gradients of dark rows
and columns exactly 0."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
_DT = {BF: 0, FP16: 1}
G_ = BR.BY_NAME

CAUSAL_ONLY = [g for g in BR.GEOMETRIES if g.causal_only]
WINDOWED = [g for g in BR.GEOMETRIES if not g.causal_only]
WIN_DIMS = (128, 64, 96, 80, 192, 256)           # (80 runs the 96 layout)
HEADS = (4, 2)
# the (geometry, form) pairs of the core tier: one per row of the geometry table at head dim 128, every class and every
# form family once; everything else is the extended tier
CORE_FWD = {("corner-hi", "8x32"), ("hi-live", "4x32"), ("causal+64", "auto"), ("corner-lo", "auto"), ("wl130+401", "auto"),
            ("rows200-keys4096-100", "split3")}
CORE_BWD = {("corner-hi-1", "dkdv128"), ("causal+33", "5gemm"), ("causal-63", "dkdv256-2"), ("causal-333", "5gemm-kv-chunks"),
            ("causal+401", "5gemm-q-fractions"), ("corner-lo+1", "windowed"), ("lo-live", "windowed"), ("two-sided-333", "windowed")}


def fwd_cases():
    """(geometry, form, D, H, Hk, dtype) of every forward case"""
    out = []
    for g in CAUSAL_ONLY:
        out += [(g, form, D, *HEADS, BF) for form in ("auto", "8x32", "4x32") for D in (128, 64)]
    for g in WINDOWED:
        out += [(g, "auto", D, *HEADS, BF) for D in WIN_DIMS]
    out.append((G_["wl130+65"], "auto", 128, *HEADS, FP16))
    for g in [x for x in BR.GEOMETRIES if x.cls == "few-rows"] + [G_["causal-333"]]:
        out += [(g, form, D, *HEADS, BF) for form in ("split2", "split3", "split8") for D in (128, 64)]
    for H, Hk in ((4, 4), (8, 1)):
        out += [(G_["causal+33"], "auto", 128, H, Hk, BF), (G_["wl130+65"], "auto", 128, H, Hk, BF)]
    return out


def bwd_cases():
    """(geometry, form, D, H, Hk, dtype) of every backward case"""
    out = []
    for g in CAUSAL_ONLY:
        out += [(g, form, 128, *HEADS, BF) for form in ("7gemm", "5gemm")]
        out += [(g, form, D, *HEADS, BF) for form in ("dkdv128", "dkdv256-1", "dkdv256-2", "dkdv256-3", "dkdv256-4") for D in (128, 64)]
    for n in ("causal-333", "causal+33", "causal+401"):
        out += [(G_[n], form, 256, *HEADS, BF) for form in ("7gemm", "5gemm")]
        out += [(G_[n], form, 128, *HEADS, BF) for form in ("5gemm-kv-chunks", "5gemm-q-fractions")]
    for g in WINDOWED:
        out += [(g, "windowed", D, *HEADS, BF) for D in WIN_DIMS]
    out.append((G_["wl130+65"], "windowed", 128, *HEADS, FP16))
    for H, Hk in ((4, 4), (8, 1)):
        out += [(G_["causal+33"], "5gemm", 128, H, Hk, BF), (G_["wl130+65"], "windowed", 128, H, Hk, BF)]
    out.append((G_["causal+33"], "5gemm-q-fractions", 128, 8, 1, BF))
    return out


def _params(cases, core):
    ps = []
    for g, form, D, H, Hk, dt in cases:
        is_core = (g.name, form) in core and D == 128 and (H, Hk) == HEADS and dt is BF
        ps.append(pytest.param(g, form, D, H, Hk, dt, id=f"{g.name}-{form}-d{D}-h{H}x{Hk}-{'bf16' if dt is BF else 'fp16'}",
                               marks=[] if is_core else [_EXT]))
    return ps


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


class _Ctx:
    """one seeded input set of a geometry and its fp64 reference (computed once on the device, reused by every form)"""

    def __init__(self, g, H, Hk, D, dtype):
        dev = _dev()
        gen = torch.Generator().manual_seed(7000 + 13 * BR.GEOMETRIES.index(g) + D + H)
        mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(dev)
        self.g, self.D, self.scale = g, D, D ** -0.5
        self.q, self.k, self.v, self.do = mk(g.B, g.lq, H, D), mk(g.B, g.lk, Hk, D), mk(g.B, g.lk, Hk, D), mk(g.B, g.lq, H, D)
        out, lse, dq, dk, dv = BR.band_ref(self.q, self.k, self.v, self.do, g.causal, g.window, g.shift)
        self.delta = (self.do.double() * out).sum(-1).permute(0, 2, 1).float().contiguous()
        self.ref = tuple(t.float() for t in (out, lse, dq, dk, dv))
        self.lse = self.ref[1].contiguous()                              # (+inf for rows without a key)
        vis = BR.band_mask(g.lq, g.lk, g.causal, g.window, g.shift, device=dev)
        self.dark_rows, self.dark_cols = ~vis.any(1), ~vis.any(0)


_CTX = {}


def _ctx(g, H, Hk, D, dtype):
    key = (g.name, H, Hk, D, dtype)
    if key not in _CTX:
        while len(_CTX) >= 6:
            _CTX.pop(next(iter(_CTX)))
        _CTX[key] = _Ctx(g, H, Hk, D, dtype)
    return _CTX[key]


def _setenv(monkeypatch, env):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)


def _compare(bad, name, got, ref, kind):
    import _tol

    bad += _tol.failures(name, got, ref, kind)


def _exact(bad, name, t, value):
    if t.numel() and not bool((t == value).all()):
        bad.append(f"{name}: not exactly {value} (e.g. {t.flatten()[(t != value).flatten().nonzero()[0]].item()})")


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(be, x, band):
    """plain outputs; accumulators overwritten (acc_init); accumulators merged onto what an EMPTY first block left
    (out 0 / lse -inf, the state a ring rank whose first block lies outside the band really starts from)"""
    g, q, k, v = x.g, x.q, x.k, x.v
    B, Sq, H, D = q.shape
    dev = q.device
    kw = dict(softmax_scale=x.scale, **band)
    out, lse = torch.full_like(q, 5.0), torch.full((B, H, Sq), 5.0, device=dev)
    be.fwd(q, k, v, out=out, lse=lse, **kw)
    nan = float("nan")
    oa, la = torch.full((B, Sq, H, D), nan, device=dev), torch.full((B, H, Sq), nan, device=dev)
    be.fwd(q, k, v, out_acc=oa, lse_acc=la, acc_init=True, **kw)
    ob, lb = torch.full((B, Sq, H, D), nan, device=dev), torch.full((B, H, Sq), nan, device=dev)
    be.fwd(q, k, v, softmax_scale=x.scale, causal=True, mask_shift=-(g.lk + 5), out_acc=ob, lse_acc=lb, acc_init=True)
    assert bool((ob == 0).all()) and bool((lb == float("-inf")).all()), "an empty first block must leave out 0 / lse -inf"
    be.fwd(q, k, v, out_acc=ob, lse_acc=lb, **kw)
    return dict(plain=(out, lse), init=(oa, la), merged=(ob, lb))


def check_fwd(tag, res, x):
    bad = []
    for mode, (o, l) in res.items():
        _compare(bad, f"{tag}.{mode}.out", o, x.ref[0], "out")
        _compare(bad, f"{tag}.{mode}.lse", l, x.ref[1], "lse")
        _exact(bad, f"{tag}.{mode}.out of rows without a key", o[:, x.dark_rows], 0.0)
        _exact(bad, f"{tag}.{mode}.lse of rows without a key", l[:, :, x.dark_rows], float("inf") if mode == "plain" else float("-inf"))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("g,form,D,H,Hk,dtype", _params(fwd_cases(), CORE_FWD))
def test_fwd_form_matches_the_band_reference(monkeypatch, g, form, D, H, Hk, dtype):
    from ring_flash_attn import _C

    be = _be()
    BR.check_fwd_form(_C, be.lib, g, form, D, H, Hk, _DT[dtype])
    _setenv(monkeypatch, BR.FWD_FORMS[form][0])
    x = _ctx(g, H, Hk, D, dtype)
    check_fwd(f"{g.name}.{form}.d{D}", run_fwd(be, x, g.band), x)


# ------------------------------------------------------------------------------------------------ backward
def run_bwd(be, x, band, modes=("plain", "acc", "init")):
    from ring_flash_attn import _C

    q, k, v, do = x.q, x.k, x.v, x.do
    dev = q.device
    kw = dict(softmax_scale=x.scale, **band)
    f32 = lambda t, val: torch.full(t.shape, val, dtype=torch.float32, device=dev)
    res = {}
    if "plain" in modes:
        dq, dk, dv = torch.full_like(q, 5.0), torch.full_like(k, 5.0), torch.full_like(v, 5.0)
        be.bwd(do, q, k, v, x.lse, x.delta, dq=dq, dk=dk, dv=dv, **kw)
        res["plain"] = (dq, dk, dv)
    if "acc" in modes:                                                    # += onto fp32 accumulators
        dqa, dka, dva = f32(q, 2.0), f32(k, -1.0), f32(v, 0.5)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, **kw)
        res["acc"] = (dqa - 2.0, dka + 1.0, dva - 0.5)
    if "init" in modes:                                                   # accumulators overwritten, never read
        nan = float("nan")
        dqa, dka, dva = f32(q, nan), f32(k, nan), f32(v, nan)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, acc_init=True, **kw)
        res["init"] = (dqa, dka, dva)
    if "two_phase" in modes:
        dqa, dka, dva = f32(q, 2.0), f32(k, -1.0), f32(v, 0.5)
        part = be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_COMPUTE, **kw)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_REDUCE, partials=part, **kw)
        res["two_phase"] = (dqa - 2.0, dka + 1.0, dva - 0.5)
    if "overwrite" in modes:                                              # dq_acc +=, dk_acc / dv_acc overwritten
        nan = float("nan")
        dqa, dka, dva = f32(q, 2.0), f32(k, nan), f32(v, nan)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_KV_OVERWRITE, **kw)
        res["overwrite"] = (dqa - 2.0, dka, dva)
    return res


def check_bwd(tag, res, x):
    bad = []
    for mode, (dq, dk, dv) in res.items():
        for nm, got, ref in zip(("dq", "dk", "dv"), (dq, dk, dv), x.ref[2:]):
            _compare(bad, f"{tag}.{mode}.{nm}", got, ref, "grad")
        _exact(bad, f"{tag}.{mode}.dq of rows without a key", dq[:, x.dark_rows], 0.0)
        _exact(bad, f"{tag}.{mode}.dk of keys no row sees", dk[:, x.dark_cols], 0.0)
        _exact(bad, f"{tag}.{mode}.dv of keys no row sees", dv[:, x.dark_cols], 0.0)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("g,form,D,H,Hk,dtype", _params(bwd_cases(), CORE_BWD))
def test_bwd_form_matches_the_band_reference(monkeypatch, g, form, D, H, Hk, dtype):
    from ring_flash_attn import _C

    be = _be()
    env = BR.BWD_FORMS[form][0]
    limit = BR.check_bwd_form(_C, be.lib, g, form, D, H, Hk, _DT[dtype])
    _setenv(monkeypatch, env)
    if limit is not None:
        monkeypatch.setenv("RFA_DS_SPILL_MAX_BYTES", str(limit))
    be.release_scratch()
    x = _ctx(g, H, Hk, D, dtype)
    try:
        res = run_bwd(be, x, g.band)
        if limit is not None:                                             # the ONE scratch is never larger than the limit
            pool = [t for t in be._ds_pool.values() if torch.is_tensor(t)]
            assert pool and all(t.numel() <= limit for t in pool), [t.numel() for t in pool]
        check_bwd(f"{g.name}.{form}.d{D}", res, x)
        if form.startswith("5gemm"):
            # the spill only adds stores to the dK/dV kernel: dK / dV are the 7-GEMM form's bits (as for unshifted calls)
            monkeypatch.setenv("RFA_BWD_DS_SPILL", "0")
            ref7 = run_bwd(be, x, g.band, modes=("plain",))["plain"]
            if form == "5gemm":
                assert torch.equal(res["plain"][1], ref7[1]) and torch.equal(res["plain"][2], ref7[2]), "dK/dV differ from the 7-GEMM form"
            check_bwd(f"{g.name}.7gemm-beside-{form}.d{D}", dict(plain=ref7), x)
    finally:
        be.release_scratch()


@pytest.mark.parametrize("name", ["causal+65", pytest.param("causal-333", marks=_EXT), pytest.param("wl130+65", marks=_EXT),
                                  pytest.param("wl130-333", marks=_EXT)])
def test_two_phase_and_overwrite_calls_with_a_shift(monkeypatch, name):
    """COMPUTE then REDUCE, and KV_OVERWRITE, on a partially visible shifted block — the 5-GEMM and the 7-GEMM form"""
    from ring_flash_attn import _C

    be = _be()
    g = G_[name]
    x = _ctx(g, *HEADS, 128, BF)
    for spill in ("1", "0"):
        monkeypatch.setenv("RFA_BWD_DS_SPILL", spill)
        a = BR.bwd_args(_C, g, *HEADS, 128, dict(RFA_BWD_DS_SPILL=spill), acc=True, phases=_C.BWD_COMPUTE)
        assert BR.bwd_plan(be.lib, a)[2] == (1 if spill == "1" and g.causal_only else 0)
        check_bwd(f"{name}.spill{spill}", run_bwd(be, x, g.band, modes=("two_phase", "overwrite")), x)
    be.release_scratch()


# ------------------------------------------------------------------------------------------------ bit identity
def _everything(be, x, band):
    f = run_fwd(be, x, band)
    b = run_bwd(be, x, band, modes=("plain", "init"))
    return {**{f"fwd.{m}.{n}": t for m, pair in f.items() for n, t in zip(("out", "lse"), pair)},
            **{f"bwd.{m}.{n}": t for m, tr in b.items() for n, t in zip(("dq", "dk", "dv"), tr)}}, f, b


@pytest.mark.parametrize("name", ["hi-dropped", "lo-dropped"])
@pytest.mark.parametrize("D", [128, pytest.param(64, marks=_EXT), pytest.param(256, marks=_EXT)])
def test_bound_dropped_by_one_is_the_unwindowed_call(name, D):
    """the bound that no element can reach any more — by exactly one — is dropped: the bits of the unwindowed non-causal call"""
    be = _be()
    g = G_[name]
    x = _ctx(g, *HEADS, D, BF)
    got, f, b = _everything(be, x, g.band)
    plain, _, _ = _everything(be, x, dict(causal=False))
    for key, t in got.items():
        assert torch.equal(t, plain[key]), f"{name}: {key} differs from the unwindowed non-causal call"
    check_fwd(name, f, x)
    check_bwd(name, b, x)


@pytest.mark.parametrize("name", ["big-left-edge", "big-right-edge"])
@pytest.mark.parametrize("D", [128, pytest.param(64, marks=_EXT), pytest.param(256, marks=_EXT)])
def test_live_band_beside_large_numbers_is_its_small_twin(name, D):
    """off and one window side beyond 2^28 with the other edge live: norm_band re-expresses the live edge in small numbers.
    Binding: the fp64 reference of the band as given; and bit for bit the small twin with the same two edges"""
    be = _be()
    g = G_[name]
    x = _ctx(g, *HEADS, D, BF)
    got, f, b = _everything(be, x, g.band)
    check_fwd(name, f, x)
    check_bwd(name, b, x)
    twin, _, _ = _everything(be, x, g.twin_geometry().band)
    for key, t in got.items():
        assert torch.equal(t, twin[key]), f"{name}: {key} differs from the small twin {g.twin}"


def test_shift_together_with_dense_halves():
    """rfa_fwd / rfa_bwd take dense q_half / k_half together with a shift: the band sits on the HALF lengths.  The off = 65
    block as the back halves of twice-as-long tensors (front halves: NaN — never read, not even into a masked tile, where
    0 * NaN would show — and never written)"""
    from ring_flash_attn import _C

    be = _be()
    g = G_["causal+65"]
    x = _ctx(g, *HEADS, 128, BF)
    dev = x.q.device
    junk = lambda t: torch.cat([torch.full_like(t, float("nan")), t], dim=1).contiguous()
    q2, k2, v2, do2 = junk(x.q), junk(x.k), junk(x.v), junk(x.do)
    B, Sq, H, D = x.q.shape
    halves = dict(q_half=_C.HALF_BACK, k_half=_C.HALF_BACK)
    out2, lse2 = torch.full_like(q2, 5.0), torch.full((B, H, 2 * Sq), 5.0, device=dev)
    be.fwd(q2, k2, v2, softmax_scale=x.scale, out=out2, lse=lse2, **halves, **g.band)
    pad = lambda t, dim: torch.cat([torch.zeros_like(t), t], dim=dim).contiguous()
    lse_in, delta_in = pad(x.lse, 2), pad(x.delta, 2)
    dq2, dk2, dv2 = torch.full_like(q2, 5.0), torch.full_like(k2, 5.0), torch.full_like(v2, 5.0)
    be.bwd(do2, q2, k2, v2, lse_in, delta_in, softmax_scale=x.scale, dq=dq2, dk=dk2, dv=dv2, **halves, **g.band)
    for nm, t, n in (("out", out2, Sq), ("dq", dq2, Sq), ("dk", dk2, g.lk), ("dv", dv2, g.lk)):
        assert bool((t[:, :n] == 5.0).all()), f"{nm}: the front half was written"
    assert bool((lse2[:, :, :Sq] == 5.0).all())
    check_fwd("halves", dict(plain=(out2[:, Sq:], lse2[:, :, Sq:])), x)
    check_bwd("halves", dict(plain=(dq2[:, Sq:], dk2[:, g.lk:], dv2[:, g.lk:])), x)
    be.release_scratch()
