"""The per-sequence shift of packed input (`mask_shift_lens`, include/rfa.h ABI 8) in every kernel form against fp64.

ONE packed batch of sequences with the local lengths 1, 31, 33, 64, 130, 257, 300 and 777 (self-attention blocks: len_q =
len_k = l) is run with mask_shift_lens in {1, 2, -1} under the windows (130, 0) causal, (90, 40) and (300, -1), and causal
without a window at -1 (every sequence wholly dark) and +1 (every sequence wholly lit).  Sequence b's band is that of a
dense block with mask_shift = mask_shift_lens * l_b, so one launch mixes wholly lit, cut and wholly dark sequences — the
mix is asserted on the host from tests/_bandref.band_mask before anything is launched — and the reference is
tests/_bandref.band_ref on every sequence's own rows (fp64, explicit mask) through tests/_tol.py (kinds out, lse, grad).
Exact checks: out == 0 for rows without a key, lse +inf (plain) / -inf (accumulators) there, gradients of dark rows and dark
columns exactly 0, rows of other halves never written.  Every case first asserts through rfa_bwd_plan /
rfa_fwd_workspace_bytes that the call runs the form it names (never balanced, never split-KV; packed input is never
persistent)."""
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
LENS = (1, 31, 33, 64, 130, 257, 300, 777)
H, HK = 4, 2
NOWIN = (-1, -1)
WINDOWS = {"wl130": (True, (130, 0)), "two-sided": (False, (90, 40)), "left300": (False, (300, -1))}
WIN_DIMS = (128, 64, 96, 192, 256)
SHIFTS = (1, 2, -1)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def seq_kinds(lens, causal, window, n):
    """per sequence, from the boolean mask alone: 'dark' (no visible element), 'lit' (every element), 'cut'"""
    kinds = []
    for l in lens:
        vis = BR.band_mask(l, l, causal, window, n * l)
        kinds.append("dark" if not vis.any() else ("lit" if vis.all() else "cut"))
    return kinds


def assert_mix(lens, causal, window, n):
    kinds = seq_kinds(lens, causal, window, n)
    if window == NOWIN:
        assert set(kinds) == ({"dark"} if n < 0 else {"lit"}), kinds       # causal only: -1 wholly dark, +1 wholly lit
    elif (causal, window) == (True, (130, 0)) and n == 1:
        # a sequence always holds a visible key (l - 1 + 130 >= l); the short ones are wholly inside the window, the
        # long ones are cut on both sides
        assert "dark" not in kinds and kinds[0] == "lit" and all(k_ == "cut" for l, k_ in zip(lens, kinds) if l > 131), kinds
    elif (causal, window) == (True, (130, 0)) and n == 2:
        # dark iff l + 1 > 130: lit, cut and dark sequences in ONE launch
        assert [k_ == "dark" for k_ in kinds] == [l + 1 > 130 for l in lens] and {"lit", "cut", "dark"} <= set(kinds), kinds
    return kinds


class _Ctx:
    """the packed batch under one band: seeded inputs, the fp64 reference of every sequence, the rows / columns without a
    visible element.  halves: every sequence is the BACK half of a sequence twice as long whose front half holds junk."""

    def __init__(self, causal, window, n, D, dtype, halves=False, lens=LENS):
        dev = _dev()
        gen = torch.Generator().manual_seed(9100 + 7 * D + 3 * (n + 2) + (window[0] % 97))
        self.lens, self.D, self.scale, self.halves = lens, D, D ** -0.5, halves
        self.band = dict(causal=causal, window=window, mask_shift_lens=n)
        mul = 2 if halves else 1
        T = mul * sum(lens)
        mk = lambda h: torch.randn(T, h, D, generator=gen).to(dtype).to(dev)
        self.q, self.k, self.v, self.do = mk(H), mk(HK), mk(HK), mk(H)
        cu = [0]
        for l in lens:
            cu.append(cu[-1] + mul * l)
        self.cu = torch.tensor(cu, dtype=torch.int32, device=dev)
        self.vl = dict(cu_seqlens_q=self.cu, cu_seqlens_k=self.cu, max_seqlen_q=mul * max(lens), max_seqlen_k=mul * max(lens))
        if halves:
            from ring_flash_attn import _C

            self.vl.update(q_half=_C.HALF_BACK, k_half=_C.HALF_BACK)
        # rows of the packed tensors the call addresses
        self.rows = torch.zeros(T, dtype=torch.bool, device=dev)
        ref = [torch.zeros(T, H, D, device=dev), torch.zeros(H, T, device=dev), torch.zeros(T, H, D, device=dev),
               torch.zeros(T, HK, D, device=dev), torch.zeros(T, HK, D, device=dev)]
        self.dark_rows = torch.zeros(T, dtype=torch.bool, device=dev)
        self.dark_cols = torch.zeros(T, dtype=torch.bool, device=dev)
        self.delta = torch.zeros(H, T, device=dev)
        for b, l in enumerate(lens):
            s = cu[b] + (l if halves else 0)
            sl = slice(s, s + l)
            self.rows[sl] = True
            out, lse, dq, dk, dv = BR.band_ref(self.q[sl][None], self.k[sl][None], self.v[sl][None], self.do[sl][None],
                                               causal, window, n * l)
            for dst, src in zip(ref, (out[0], None, dq[0], dk[0], dv[0])):
                if src is not None:
                    dst[sl] = src.float()
            ref[1][:, sl] = lse[0].float()
            self.delta[:, sl] = (self.do[sl].double() * out[0]).sum(-1).t().float()
            vis = BR.band_mask(l, l, causal, window, n * l, device=dev)
            self.dark_rows[sl] = ~vis.any(1)
            self.dark_cols[sl] = ~vis.any(0)
        self.ref = tuple(ref)
        self.lse = ref[1].contiguous()                                     # (+inf for rows without a key)


_CTX = {}


def _ctx(*key):
    if key not in _CTX:
        while len(_CTX) >= 4:
            _CTX.pop(next(iter(_CTX)))
        _CTX[key] = _Ctx(*key)
    return _CTX[key]


def _compare(bad, name, got, ref, kind):
    import _tol

    bad += _tol.failures(name, got, ref, kind)


def _exact(bad, name, t, value):
    if t.numel() and not bool((t == value).all()):
        bad.append(f"{name}: not exactly {value} (e.g. {t.flatten()[(t != value).flatten().nonzero()[0]].item()})")


# ---- host side: the launch plan of the packed call (pure functions of the C ABI) -------------------------------------
def _packed_fwd_args(C_, x, dtype, env=None):
    env = env or {}
    a = C_.FwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype = len(x.lens), x.vl["max_seqlen_q"], x.vl["max_seqlen_k"], H, HK, x.D, dtype
    a.cu_seqlens_q = a.cu_seqlens_k = x.cu.data_ptr()
    a.total_q = x.q.shape[0]
    a.q_half, a.k_half = x.vl.get("q_half", 0), x.vl.get("k_half", 0)
    a.causal = 1 if x.band["causal"] else 0
    w = x.band["window"]
    if w[0] >= 0 or w[1] >= 0:
        a.window, a.window_left, a.window_right = 1, w[0], w[1]
    a.mask_shift_lens = x.band["mask_shift_lens"]
    return a


def _packed_bwd_args(C_, x, dtype, env=None, acc=False, phases=0):
    env = env or {}
    a = C_.BwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype = len(x.lens), x.vl["max_seqlen_q"], x.vl["max_seqlen_k"], H, HK, x.D, dtype
    a.cu_seqlens_q = a.cu_seqlens_k = x.cu.data_ptr()
    a.total_k = a.total_q = x.q.shape[0]
    a.q_half, a.k_half = x.vl.get("q_half", 0), x.vl.get("k_half", 0)
    a.causal = 1 if x.band["causal"] else 0
    w = x.band["window"]
    if w[0] >= 0 or w[1] >= 0:
        a.window, a.window_left, a.window_right = 1, w[0], w[1]
    a.mask_shift_lens = x.band["mask_shift_lens"]
    a.phases = phases
    wide, ns = env.get("RFA_DKDV_WIDE"), int(env.get("RFA_DKDV_NSPLIT", "0"))
    if wide == "0":
        a.dkdv_form = C_.DKDV_128
    elif ns > 0 or wide == "1":
        a.dkdv_form = C_.DKDV_256
    a.dkdv_nsplit = ns
    if env.get("RFA_BWD_DS_SPILL", "1") != "0":
        a.ds_scratch = 256
    if acc:
        a.dq_acc = a.dk_acc = a.dv_acc = 256
    return a


def check_fwd_plan(be, x, dtype):
    """windowed instances or the default ones, never with split-KV shares (packed input is never persistent)"""
    from ring_flash_attn import _C

    nbytes, ns = BR.fwd_shares(be.lib, _packed_fwd_args(_C, x, _DT[dtype]))
    assert (nbytes, ns) == (0, 1), (nbytes, ns)


def check_bwd_plan(be, x, dtype, form, phases=0):
    from ring_flash_attn import _C

    env, (wform, wns, wfive), _ = BR.BWD_FORMS[form]
    windowed = x.band["window"][0] >= 0 or (x.band["window"][1] >= 0 and not x.band["causal"])
    for acc in (False, True):
        f, ns, five = BR.bwd_plan(be.lib, _packed_bwd_args(_C, x, _DT[dtype], env, acc=acc, phases=phases))
        tag = (form, x.D, acc, f, ns, five)
        assert f != BR.DKDV_BAL, tag
        assert wform is None or f == wform, tag
        assert wns is None or ns == wns, tag
        assert wfive is None or five == wfive, tag
        if windowed:
            assert five == 0 and (x.D > 128 or (f, ns) == (BR.DKDV_128, 1)), tag      # the windowed instances: one form


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(be, x):
    """plain outputs; accumulators overwritten (acc_init); accumulators merged onto what an EMPTY first block left (every
    sequence wholly dark: out 0 / lse -inf)"""
    q, k, v = x.q, x.k, x.v
    T, _, D = q.shape
    dev = q.device
    kw = dict(softmax_scale=x.scale, **x.band, **x.vl)
    out, lse = torch.full_like(q, 5.0), torch.full((H, T), 5.0, device=dev)
    be.fwd(q, k, v, out=out, lse=lse, **kw)
    oa, la = torch.full((T, H, D), 7.0, device=dev), torch.full((H, T), 7.0, device=dev)
    be.fwd(q, k, v, out_acc=oa, lse_acc=la, acc_init=True, **kw)
    ob, lb = torch.full((T, H, D), 7.0, device=dev), torch.full((H, T), 7.0, device=dev)
    be.fwd(q, k, v, softmax_scale=x.scale, causal=True, mask_shift_lens=-2, out_acc=ob, lse_acc=lb, acc_init=True, **x.vl)
    assert bool((ob[x.rows] == 0).all()) and bool((lb[:, x.rows] == float("-inf")).all()), \
        "an empty first block must leave out 0 / lse -inf"
    be.fwd(q, k, v, out_acc=ob, lse_acc=lb, **kw)
    return dict(plain=(out, lse, 5.0), init=(oa, la, 7.0), merged=(ob, lb, 7.0))


def check_fwd(tag, res, x):
    bad = []
    r = x.rows
    for mode, (o, l, fill) in res.items():
        _compare(bad, f"{tag}.{mode}.out", o[r], x.ref[0][r], "out")
        _compare(bad, f"{tag}.{mode}.lse", l[:, r], x.ref[1][:, r], "lse")
        _exact(bad, f"{tag}.{mode}.out of rows without a key", o[x.dark_rows], 0.0)
        _exact(bad, f"{tag}.{mode}.lse of rows without a key", l[:, x.dark_rows], float("inf") if mode == "plain" else float("-inf"))
        _exact(bad, f"{tag}.{mode}.out of rows the call does not address", o[~r], fill)
        _exact(bad, f"{tag}.{mode}.lse of rows the call does not address", l[:, ~r], fill)
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ backward
def run_bwd(be, x, modes=("plain", "acc", "init", "two_phase", "overwrite")):
    from ring_flash_attn import _C

    q, k, v, do = x.q, x.k, x.v, x.do
    dev = q.device
    kw = dict(softmax_scale=x.scale, **x.band, **x.vl)
    f32 = lambda t, val: torch.full(t.shape, val, dtype=torch.float32, device=dev)
    res = {}
    if "plain" in modes:
        dq, dk, dv = torch.full_like(q, 5.0), torch.full_like(k, 5.0), torch.full_like(v, 5.0)
        be.bwd(do, q, k, v, x.lse, x.delta, dq=dq, dk=dk, dv=dv, **kw)
        res["plain"] = (dq, dk, dv, (5.0, 5.0, 5.0))
    if "acc" in modes:                                                    # += onto fp32 accumulators
        dqa, dka, dva = f32(q, 2.0), f32(k, -1.0), f32(v, 0.5)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, **kw)
        res["acc"] = (dqa - 2.0, dka + 1.0, dva - 0.5, (0.0, 0.0, 0.0))
    if "init" in modes:                                                   # accumulators overwritten
        dqa, dka, dva = f32(q, 7.0), f32(k, 7.0), f32(v, 7.0)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, acc_init=True, **kw)
        res["init"] = (dqa, dka, dva, (7.0, 7.0, 7.0))
    if "two_phase" in modes:
        dqa, dka, dva = f32(q, 2.0), f32(k, -1.0), f32(v, 0.5)
        part = be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_COMPUTE, **kw)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_REDUCE, partials=part, **kw)
        res["two_phase"] = (dqa - 2.0, dka + 1.0, dva - 0.5, (0.0, 0.0, 0.0))
    if "overwrite" in modes:                                              # dq_acc +=, dk_acc / dv_acc overwritten
        dqa, dka, dva = f32(q, 2.0), f32(k, 7.0), f32(v, 7.0)
        be.bwd(do, q, k, v, x.lse, x.delta, dq_acc=dqa, dk_acc=dka, dv_acc=dva, phases=_C.BWD_KV_OVERWRITE, **kw)
        res["overwrite"] = (dqa - 2.0, dka, dva, (0.0, 7.0, 7.0))
    return res


def check_bwd(tag, res, x):
    bad = []
    r = x.rows
    for mode, (dq, dk, dv, fills) in res.items():
        for nm, got, ref, fill in zip(("dq", "dk", "dv"), (dq, dk, dv), x.ref[2:], fills):
            _compare(bad, f"{tag}.{mode}.{nm}", got[r], ref[r], "grad")
            _exact(bad, f"{tag}.{mode}.{nm} of rows the call does not address", got[~r], fill)
        _exact(bad, f"{tag}.{mode}.dq of rows without a key", dq[x.dark_rows], 0.0)
        _exact(bad, f"{tag}.{mode}.dk of keys no row sees", dk[x.dark_cols], 0.0)
        _exact(bad, f"{tag}.{mode}.dv of keys no row sees", dv[x.dark_cols], 0.0)
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ cases
def _win_params():
    """(window name, mask_shift_lens, D, dtype): one core case per window family at head dim 128, the rest extended"""
    core = {("wl130", 2, 128), ("two-sided", 1, 128), ("left300", -1, 128)}
    ps = []
    for w in WINDOWS:
        for n in SHIFTS:
            for D in WIN_DIMS:
                if D != 128 and n != 2 and not (w == "wl130"):
                    continue                                               # (every head dim: all three shifts of one window, shift 2 of the others)
                ps.append(pytest.param(w, n, D, BF, id=f"{w}-n{n:+d}-d{D}-bf16", marks=[] if (w, n, D) in core else [_EXT]))
    ps.append(pytest.param("wl130", 2, 128, FP16, id="wl130-n+2-d128-fp16", marks=[_EXT]))
    return ps


@pytest.mark.parametrize("w,n,D,dtype", _win_params())
def test_windowed_packed_shift_matches_the_band_reference(w, n, D, dtype):
    causal, window = WINDOWS[w]
    assert_mix(LENS, causal, window, n)
    be = _be()
    x = _ctx(causal, window, n, D, dtype)
    check_fwd_plan(be, x, dtype)
    check_bwd_plan(be, x, dtype, "windowed")
    check_bwd_plan(be, x, dtype, "windowed", phases=1)
    tag = f"{w}.n{n:+d}.d{D}"
    try:
        check_fwd(tag, run_fwd(be, x), x)
        check_bwd(tag, run_bwd(be, x), x)
    finally:
        be.release_scratch()


CAUSAL_FORMS = ("5gemm", "dkdv128", "dkdv256-1", "dkdv256-2")


@pytest.mark.parametrize("n", [1, -1])
@pytest.mark.parametrize("D", [128, pytest.param(64, marks=_EXT)])
def test_causal_only_packed_shift_forward(n, D):
    """-1: every sequence wholly dark; +1: every sequence wholly lit — the default (not windowed) instances"""
    assert_mix(LENS, True, NOWIN, n)
    be = _be()
    x = _ctx(True, NOWIN, n, D, BF)
    check_fwd_plan(be, x, BF)
    check_fwd(f"causal.n{n:+d}.d{D}", run_fwd(be, x), x)


@pytest.mark.parametrize("form,n,D", [pytest.param(form, n, D, id=f"{form}-n{n:+d}-d{D}",
                                                   marks=[] if (form, n, D) in (("5gemm", 1, 128), ("dkdv256-2", -1, 128), ("dkdv128", 1, 128)) else [_EXT])
                                      for form in CAUSAL_FORMS for n in (1, -1) for D in (128, 64) if not (form == "5gemm" and D == 64)])
def test_causal_only_packed_shift_backward_forms(monkeypatch, form, n, D):
    """a causal packed call with a shift and no window keeps the default instances: the packed-row dS hand-off (5-GEMM, its
    dK/dV bit-equal to the 7-GEMM form's) and the 128-key / 256-key dK/dV forms with 1 and 2 shares"""
    assert_mix(LENS, True, NOWIN, n)
    be = _be()
    x = _ctx(True, NOWIN, n, D, BF)
    env = BR.BWD_FORMS[form][0]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    if form.startswith("dkdv"):
        monkeypatch.setenv("RFA_BWD_DS_SPILL", "0" if D == 64 else "1")
    check_bwd_plan(be, x, BF, form)
    check_bwd_plan(be, x, BF, form, phases=1)
    be.release_scratch()
    tag = f"causal.{form}.n{n:+d}.d{D}"
    try:
        res = run_bwd(be, x)
        check_bwd(tag, res, x)
        if form == "5gemm":
            monkeypatch.setenv("RFA_BWD_DS_SPILL", "0")
            check_bwd_plan(be, x, BF, "7gemm")
            res7 = run_bwd(be, x)
            check_bwd(tag + ".7gemm", res7, x)
            for mode in res:
                assert torch.equal(res[mode][1], res7[mode][1]) and torch.equal(res[mode][2], res7[mode][2]), \
                    f"{mode}: dK/dV of the 5-GEMM form differ from the 7-GEMM form's"
    finally:
        be.release_scratch()


@pytest.mark.parametrize("w,n", [("wl130", 1), pytest.param("two-sided", 2, marks=_EXT), pytest.param(None, 1, marks=_EXT)])
def test_packed_shift_with_back_halves(w, n):
    """q_half = k_half = BACK on sequences of even length: the band sits on the HALF lengths (shift = n * l / 2 of the
    doubled sequence); the junk front halves are never read into the result and never written"""
    causal, window = WINDOWS[w] if w else (True, NOWIN)
    be = _be()
    x = _ctx(causal, window, n, 128, BF, True)
    check_fwd_plan(be, x, BF)
    tag = f"halves.{w}.n{n:+d}"
    try:
        check_fwd(tag, run_fwd(be, x), x)
        check_bwd(tag, run_bwd(be, x), x)
    finally:
        be.release_scratch()


# ------------------------------------------------------------------------------------------------ dense identity
@pytest.mark.parametrize("n,causal,window", [(1, True, (130, 0)), pytest.param(-1, False, (90, 40), marks=_EXT),
                                             pytest.param(1, True, NOWIN, marks=_EXT), pytest.param(-1, True, NOWIN, marks=_EXT)])
def test_dense_mask_shift_lens_is_mask_shift_times_len_k(n, causal, window):
    """dense input folds the field into mask_shift on the host: the call with mask_shift = n * Sk, bit for bit"""
    be = _be()
    dev = _dev()
    gen = torch.Generator().manual_seed(42)
    B, Sq, Sk, D = 2, 300, 333, 128
    mk = lambda s, h: torch.randn(B, s, h, D, generator=gen).to(BF).to(dev)
    q, k, v, do = mk(Sq, H), mk(Sk, HK), mk(Sk, HK), mk(Sq, H)
    res = []
    for band in (dict(mask_shift_lens=n), dict(mask_shift=n * Sk)):
        kw = dict(softmax_scale=D ** -0.5, causal=causal, window=window, **band)
        out, lse = torch.full_like(q, 5.0), torch.full((B, H, Sq), 5.0, device=dev)
        be.fwd(q, k, v, out=out, lse=lse, **kw)
        delta = torch.empty((B, H, Sq), dtype=torch.float32, device=dev)
        be.bwd_preprocess(do, out, delta)
        dq, dk, dv = torch.full_like(q, 5.0), torch.full_like(k, 5.0), torch.full_like(v, 5.0)
        be.bwd(do, q, k, v, lse, delta, dq=dq, dk=dk, dv=dv, **kw)
        res.append((out, lse, dq, dk, dv))
    for nm, a_, b_ in zip(("out", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(a_, b_), f"{nm} differs"
    ro, rl, rdq, rdk, rdv = BR.band_ref(q, k, v, do, causal, window, n * Sk)
    import _tol

    bad = _tol.failures("out", res[0][0], ro.float(), "out") + _tol.failures("lse", res[0][1], rl.float(), "lse")
    assert not bad, "; ".join(bad)
    be.release_scratch()


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    """packed + mask_shift_lens + dropout: -8; |mask_shift_lens| * Sk >= 2^30: -8 (packed and dense); packed + the absolute
    mask_shift: still -8; and without causal and without a window the field is ignored"""
    be = _be()
    x = _ctx(True, (130, 0), 1, 128, BF)
    T = x.q.shape[0]
    out, lse = torch.empty_like(x.q), torch.empty((H, T), device=x.q.device)
    base = dict(softmax_scale=x.scale, out=out, lse=lse, **x.vl)
    with pytest.raises(RuntimeError, match="-8"):
        be.fwd(x.q, x.k, x.v, causal=True, mask_shift_lens=1, dropout=(0.1, 1, 0, 0, 0), **base)
    big = (1 << 30) // max(LENS) + 1
    with pytest.raises(RuntimeError, match="-8"):
        be.fwd(x.q, x.k, x.v, causal=True, mask_shift_lens=big, **base)
    with pytest.raises(RuntimeError, match="-8"):
        be.fwd(x.q, x.k, x.v, causal=True, mask_shift_lens=-big, **base)
    with pytest.raises(RuntimeError, match="-8"):
        be.fwd(x.q, x.k, x.v, causal=True, mask_shift=4, **base)
    qd = x.q[:256].view(1, 256, H, 128)
    kd, vd = x.k[:256].view(1, 256, HK, 128), x.v[:256].view(1, 256, HK, 128)
    od, ld = torch.empty_like(qd), torch.empty((1, H, 256), device=qd.device)
    with pytest.raises(RuntimeError, match="-8"):
        be.fwd(qd, kd, vd, softmax_scale=x.scale, causal=True, mask_shift_lens=1 << 22, out=od, lse=ld)
    dq, dk, dv = torch.empty_like(x.q), torch.empty_like(x.k), torch.empty_like(x.v)
    with pytest.raises(RuntimeError, match="-8"):
        be.bwd(x.do, x.q, x.k, x.v, x.lse, x.delta, softmax_scale=x.scale, causal=True, mask_shift_lens=big, dq=dq, dk=dk, dv=dv, **x.vl)
    with pytest.raises(RuntimeError, match="-8"):
        be.bwd(x.do, x.q, x.k, x.v, x.lse, x.delta, softmax_scale=x.scale, causal=True, mask_shift=4, dq=dq, dk=dk, dv=dv, **x.vl)
    # ignored without a band: the bits of the call without the field
    o0, l0 = torch.empty_like(x.q), torch.empty((H, T), device=x.q.device)
    be.fwd(x.q, x.k, x.v, softmax_scale=x.scale, causal=False, out=o0, lse=l0, **x.vl)
    be.fwd(x.q, x.k, x.v, causal=False, mask_shift_lens=3, **base)
    assert torch.equal(out, o0) and torch.equal(lse, l0)
    be.release_scratch()
