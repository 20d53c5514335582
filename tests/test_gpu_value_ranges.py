"""Every kernel form on inputs whose logits are NOT N(0,1) (tests/_valueref.py: stairs that make every key tile rescale
the online softmax with a different factor per row, a spike in the last visible tile, logit ranges around +-80, one-hot and
exactly uniform softmaxes) against the fp64 attention of tests/_blockref.py, by flash_attn's criterion: the error is at most
twice that of the kernels' rounding model (tests/_valueref.py: model_attention) plus the atol of tests/_tol.py, on the whole
tensor and again on the witness rows of the forward's deferred rescale alone; lse by tests/_tol.py kind `lse`.

Forward: the 8 x 32, 4 x 32, persistent and split-KV forms, a windowed instance, head dims 128, 64, 80, 40, 192, 256, 192 / 128,
bf16 and fp16; plain outputs, overwritten accumulators, accumulators merged onto an empty first block, and accumulators merged
onto a NON-empty first block whose lse lies 0, 5 and 100 nats above and below this block's, and a key range split over two
calls.  Backward (from the fp64 lse and delta rounded to fp32): 7-GEMM, 5-GEMM, the 128-key, shared-range 256-key and
balanced dK/dV plans, windowed instances, head dims 192 and 256, 192 / 128; plain, `+=` and overwritten accumulators.
Every case first asserts on the host that the call runs the form it names (tests/test_value_cases_cpu.py checks the same
without a device) and runs twice: the second run's bits are the first's.  `uniform` (q = 0): dK is exactly 0 — the dS^T Q
product of exact zeros; dQ and dV are held to the criterion."""
import collections
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402
import _blockref as R                            # noqa: E402
import _valueref as V                            # noqa: E402
import test_gpu_band_forms as GF                 # noqa: E402  (run_bwd, the device helpers; nothing in it touches a device at import)

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
_DT = {BF: 0, FP16: 1}
HEADS = (4, 2)
S_ = V.SHAPES

Case = collections.namedtuple("Case", "family shape form D Dv dtype")

# forward (form, shape) pairs at head dim 128; "window": the library's own choice on a windowed geometry
FWD_FORMS_128 = (("auto", "rect"), ("auto", "square"), ("8x32", "rect-causal"), ("8x32", "square"), ("4x32", "rect-causal"),
                 ("4x32", "square"), ("p8x32", "persistent"), ("split2", "split"), ("split3", "split"), ("split8", "split"),
                 ("window", "window"))
FWD_DIMS = ((64, 64, BF), (80, 80, BF), (40, 40, BF), (192, 192, BF), (256, 256, BF), (192, 128, BF), (128, 128, FP16),
            (192, 192, FP16))
CORE_FWD = {("8x32", "rect-causal"), ("4x32", "square"), ("p8x32", "persistent"), ("split3", "split"), ("window", "window")}
# backward (form, shape) pairs at head dim 128; "balanced": the balanced causal schedule by name (RFA_DKDV_WIDE=2)
BWD_FORMS_128 = (("7gemm", "rect-causal"), ("5gemm", "rect-causal"), ("5gemm", "square"), ("dkdv128", "rect-causal"),
                 ("dkdv256-1", "rect-causal"), ("dkdv256-2", "rect-causal"), ("dkdv256-3", "rect-causal"),
                 ("dkdv256-4", "rect-causal"), ("balanced", "square512"), ("windowed", "window"))
BWD_DIMS = (("7gemm", 192, 192, BF), ("5gemm", 192, 192, BF), ("7gemm", 256, 256, BF), ("5gemm", 256, 256, BF),
            ("7gemm", 192, 128, BF), ("5gemm", 192, 128, BF), ("dkdv128", 64, 64, BF), ("5gemm", 128, 128, FP16))
CORE_BWD = {("7gemm", "rect-causal"), ("5gemm", "rect-causal"), ("dkdv128", "rect-causal"), ("dkdv256-2", "rect-causal"),
            ("balanced", "square512"), ("windowed", "window")}
BALANCED_ENV = dict(RFA_DKDV_WIDE="2")
DROPOUT_FAMILIES = ("stairs-up", "late-spike")
MERGE_GAPS = (0.0, 5.0, -5.0, 100.0, -100.0)


def fwd_cases():
    out = []
    for fam in V.FAMILIES:
        out += [Case(fam, shape, form, 128, 128, BF) for form, shape in FWD_FORMS_128]
        out += [Case(fam, "rect-causal", "auto", D, Dv, dt) for D, Dv, dt in FWD_DIMS]
    return out


def bwd_cases():
    out = []
    for fam in V.FAMILIES:
        out += [Case(fam, shape, form, 128, 128, BF) for form, shape in BWD_FORMS_128]
        out += [Case(fam, "rect-causal", form, D, Dv, dt) for form, D, Dv, dt in BWD_DIMS]
    return out


def _params(cases, core):
    ps = []
    for c in cases:
        is_core = (c.form, c.shape) in core and c.D == c.Dv == 128 and c.dtype is BF
        dims = f"d{c.D}" if c.D == c.Dv else f"d{c.D}v{c.Dv}"
        ps.append(pytest.param(c, id=f"{c.family}-{c.form}-{c.shape}-{dims}-{'bf16' if c.dtype is BF else 'fp16'}",
                               marks=[] if is_core else [_EXT]))
    return ps


# ---- host side: the case runs the form it names (pure functions of the C ABI; tests/test_value_cases_cpu.py calls these too)
def fwd_env(c):
    if c.form == "p8x32":
        return dict(RFA_FWD_FORM="p8x32", RFA_FWD_KV_NSPLIT="1")
    return BR.FWD_FORMS["auto" if c.form == "window" else c.form][0]


def check_fwd_case(C_, lib, c):
    g = S_[c.shape]
    assert c.family in V.FAMILIES and (c.form == "window") == (not g.causal_only and g.causal), c
    if c.form == "p8x32":
        # the persistent form has no host-visible plan; its eligibility rule: head dim 128, an unshifted band, plain outputs
        assert c.D == c.Dv == 128 and g.causal_only and g.shift == 0, c
        assert BR.fwd_shares(lib, BR.fwd_args(C_, g, *HEADS, 128, fwd_env(c), _DT[c.dtype])) == (0, 1), c
        return
    if c.Dv != c.D:
        assert c.form == "auto" and c.D > 128, c                           # (csrc/rfa_vdim.hip: never split, one form)
        return
    BR.check_fwd_form(C_, lib, g, "auto" if c.form == "window" else c.form, c.D, *HEADS, _DT[c.dtype])
    if c.form.startswith("split"):
        assert g.lk >= 64 * 8 * 8, c                                       # (every share of split8 holds several key tiles)


def bwd_env(c):
    return BALANCED_ENV if c.form == "balanced" else BR.BWD_FORMS[c.form][0]


def check_bwd_case(C_, lib, c):
    g = S_[c.shape]
    assert c.family in V.FAMILIES, c
    if c.form == "balanced":
        # plain outputs and OVERWRITTEN accumulators run the balanced schedule; run_bwd's `+=` mode is not eligible and
        # exercises the plan's own choice under the same name (tests/test_gpu_kernels.py: test_dkdv_balanced_causal_schedule)
        assert c.D == 128 and g.lq == g.lk and g.shift == 0, c
        plain = BR.bwd_args(C_, g, *HEADS, c.D, BALANCED_ENV, _DT[c.dtype])
        init = BR.bwd_args(C_, g, *HEADS, c.D, BALANCED_ENV, _DT[c.dtype], acc=True)
        init.acc_init = 1
        add = BR.bwd_args(C_, g, *HEADS, c.D, BALANCED_ENV, _DT[c.dtype], acc=True)
        for a in (plain, init):
            f, ns, five = BR.bwd_plan(lib, a)
            assert f == C_.DKDV_BAL and five == 1, (c, f, ns, five)
        assert BR.bwd_plan(lib, add)[0] != C_.DKDV_BAL, c
        return
    if c.D in (128, 256, 64) and c.Dv == c.D:
        BR.check_bwd_form(C_, lib, g, c.form, c.D, *HEADS, _DT[c.dtype])
        return
    # head dim 192 and 192 / 128 (rfa_bwd_vd runs the base arguments' own plan): the dQ form the name asks for
    assert c.form in ("5gemm", "7gemm") and g.causal_only, c
    for acc in (False, True):
        f, ns, five = BR.bwd_plan(lib, BR.bwd_args(C_, g, *HEADS, c.D, bwd_env(c), _DT[c.dtype], acc=acc))
        assert five == (1 if c.form == "5gemm" else 0), (c, f, ns, five)


# ---- device side ------------------------------------------------------------------------------------------------------
class _Ctx:
    """one family's inputs at one shape, the fp64 reference, the rounding model and the witness rows — computed once on the
    device, shared by every form and left unchanged"""

    def __init__(self, family, shape, D, Dv, dtype):
        dev = GF._dev()
        g = S_[shape]
        seed = 9000 + 17 * V.FAMILIES.index(family) + 5 * list(S_).index(shape) + D + Dv
        self.g, self.D, self.scale, self.family = g, D, D ** -0.5, family
        self.q, self.k, self.v, self.do = (t.to(dev) for t in V.make_inputs(
            family, g.B, g.lq, g.lk, *HEADS, D, dtype, seed, Dv=Dv, causal=g.causal, window=g.window, shift=g.shift))
        band = dict(causal=g.causal, window=g.window, shift=g.shift)
        ex = R.attention(self.q, self.k, self.v, dout=self.do, autograd=Dv != D, **band)
        self.exact = tuple(t.detach() for t in ex)                          # fp64: out, lse, dq, dk, dv
        self.lse = ex[1].float().contiguous()                               # (+inf for rows without a key)
        self.delta = (self.do.double() * ex[0]).sum(-1).permute(0, 2, 1).float().contiguous()
        self.model = V.model_attention(self.q, self.k, self.v, self.do, lse=self.lse, delta=self.delta, **band)
        _, rows, _ = V.witness(V.scores(self.q, self.k, self.scale, g.causal, g.window, g.shift))
        self.rows = rows.permute(0, 2, 1).contiguous()                      # (B, lq, H): the leading dims of out / dq
        vis = BR.band_mask(g.lq, g.lk, g.causal, g.window, g.shift, device=dev)
        self.dark_rows = ~vis.any(1)


_CTX = {}


def _ctx(c):
    key = (c.family, c.shape, c.D, c.Dv, c.dtype)
    if key not in _CTX:
        while len(_CTX) >= 8:
            _CTX.pop(next(iter(_CTX)))
        _CTX[key] = _Ctx(*key)
    return _CTX[key]


def _merge64(o1, l1, o2, l2):
    """fp64 merge of two blocks: out (B, S, H, D), lse (B, H, S); -inf marks an empty block"""
    l = torch.logaddexp(l1, l2)
    w = lambda x: torch.exp(x - torch.where(torch.isinf(l), torch.zeros_like(l), l)).permute(0, 2, 1).unsqueeze(-1)
    return w(l1) * o1 + w(l2) * o2, l


def run_fwd(be, x, c):
    """{mode: (out, lse)}: plain; init (accumulators overwritten); merged (onto an EMPTY first block); gap<d> (onto a first block
    of other values whose lse is this block's + d); the persistent form takes plain outputs only"""
    g, q, k, v = x.g, x.q, x.k, x.v
    B, Sq, H, _ = q.shape
    Dv, dev = v.shape[-1], q.device
    kw = dict(softmax_scale=x.scale, **g.band)
    nan = float("nan")
    acc = lambda: (torch.full((B, Sq, H, Dv), nan, device=dev), torch.full((B, H, Sq), nan, device=dev))
    out, lse = torch.full((B, Sq, H, Dv), 5.0, dtype=q.dtype, device=dev), torch.full((B, H, Sq), 5.0, device=dev)
    be.fwd(q, k, v, out=out, lse=lse, **kw)
    res = dict(plain=(out, lse))
    if c.form == "p8x32":
        return res
    oa, la = acc()
    be.fwd(q, k, v, out_acc=oa, lse_acc=la, acc_init=True, **kw)
    res["init"] = (oa, la)
    ob, lb = acc()
    be.fwd(q, k, v, softmax_scale=x.scale, causal=True, mask_shift=-(g.lk + 5), out_acc=ob, lse_acc=lb, acc_init=True)
    assert bool((ob == 0).all()) and bool((lb == float("-inf")).all()), "an empty first block must leave out 0 / lse -inf"
    be.fwd(q, k, v, out_acc=ob, lse_acc=lb, **kw)
    res["merged"] = (ob, lb)
    for d in MERGE_GAPS:
        og, lg = x.first_out.clone(), torch.where(torch.isinf(x.lse), torch.full_like(x.lse, -1.0), x.lse + d)
        be.fwd(q, k, v, out_acc=og, lse_acc=lg, **kw)
        res[f"gap{d:+.0f}"] = (og, lg)
    return res


def _first_block(x):
    """the first block every gap mode merges onto: fixed values of order one"""
    if not hasattr(x, "first_out"):
        gen = torch.Generator().manual_seed(77)
        B, Sq, H, _ = x.q.shape
        x.first_out = torch.randn(B, Sq, H, x.v.shape[-1], generator=gen).to(x.q.device)


def check_fwd(tag, res, x):
    bad = []
    e_out, e_lse = x.exact[0], x.exact[1]
    m_out, m_lse = x.model[0], x.model[1]
    for mode, (o, l) in res.items():
        if mode.startswith("gap"):
            d = float(mode[3:])
            first = torch.where(torch.isinf(x.lse), torch.full_like(x.lse, -1.0), x.lse + d)
            dark = lambda t: torch.where(torch.isinf(t), torch.full_like(t, float("-inf")), t)       # (an empty block merges as -inf)
            eo, el = _merge64(x.first_out.double(), first.double(), e_out, dark(e_lse))
            mo, ml = _merge64(x.first_out.double(), first.double(), m_out.double(), dark(m_lse.double()))
            bad += V.failures(f"{tag}.{mode}.out", o, eo, mo, "out", x.rows)
            bad += V.lse_failures(f"{tag}.{mode}.lse", l, el)
            continue
        bad += V.failures(f"{tag}.{mode}.out", o, e_out, m_out, "out", x.rows)
        want = e_lse if mode == "plain" else torch.where(torch.isinf(e_lse), torch.full_like(e_lse, float("-inf")), e_lse)
        if mode == "plain":
            bad += V.lse_failures(f"{tag}.{mode}.lse", l, want)
        else:
            fin = torch.isfinite(want)
            bad += V.lse_failures(f"{tag}.{mode}.lse", l[fin], want[fin])
            GF._exact(bad, f"{tag}.{mode}.lse of rows without a key", l[~fin], float("-inf"))
        GF._exact(bad, f"{tag}.{mode}.out of rows without a key", o[:, x.dark_rows], 0.0)
    assert not bad, "; ".join(bad)


def _same_bits(tag, a, b):
    for mode in a:
        for n, (s, t) in enumerate(zip(a[mode], b[mode])):
            assert torch.equal(s, t), f"{tag}.{mode}[{n}]: the second run's bits differ from the first's"


@pytest.mark.parametrize("c", _params(fwd_cases(), CORE_FWD))
def test_fwd_form_on_the_value_family(monkeypatch, c):
    from ring_flash_attn import _C

    be = GF._be()
    check_fwd_case(_C, be.lib, c)
    x = _ctx(c)
    _first_block(x)
    GF._setenv(monkeypatch, fwd_env(c))
    res = run_fwd(be, x, c)
    tag = f"{c.family}.{c.form}.{c.shape}.d{c.D}"
    check_fwd(tag, res, x)
    _same_bits(tag, res, run_fwd(be, x, c))
    if c.form == "p8x32":
        # the persistent form claims the 8 x 32 form's bits: the same arithmetic in the same order per query row
        monkeypatch.setenv("RFA_FWD_FORM", "8x32")
        _same_bits(tag + " vs 8x32", res, dict(plain=run_fwd(be, x, c)["plain"]))


@pytest.mark.parametrize("family", ["stairs-up", pytest.param("one-hot", marks=_EXT), pytest.param("offset-80", marks=_EXT),
                                    pytest.param("late-spike", marks=_EXT)])
def test_fwd_key_range_split_over_two_calls(family):
    """the fused merge epilogue across different maxima: keys 0 .. 255 overwrite the accumulators, keys 256 .. 519 are merged
    onto them (stairs-up: the second block's lse lies tens of nats above the first's; stairs-down would be the reverse) —
    against the fp64 attention over all keys"""
    be = GF._be()
    c = Case(family, "rect", "auto", 128, 128, BF)
    x = _ctx(c)
    B, Sq, H, D = x.q.shape
    nan, cut = float("nan"), 256
    oa, la = torch.full((B, Sq, H, D), nan, device=x.q.device), torch.full((B, H, Sq), nan, device=x.q.device)
    kw = dict(softmax_scale=x.scale, causal=False, out_acc=oa, lse_acc=la)
    be.fwd(x.q, x.k[:, :cut], x.v[:, :cut], acc_init=True, **kw)
    be.fwd(x.q, x.k[:, cut:], x.v[:, cut:], **kw)
    bad = V.failures(f"{family}.two-calls.out", oa, x.exact[0], x.model[0], "out", x.rows)
    bad += V.lse_failures(f"{family}.two-calls.lse", la, x.exact[1])
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("family", [DROPOUT_FAMILIES[0], pytest.param(DROPOUT_FAMILIES[1], marks=_EXT)])
def test_fwd_dropout_on_the_value_family(family):
    """the dropout instance: out takes the kept P (scaled by 1 / (1 - p)), lsum — so lse — is the undropped softmax's"""
    from oracle import flash_attn_ref as O

    be = GF._be()
    c = Case(family, "rect-causal", "auto", 128, 128, BF)
    x = _ctx(c)
    g = x.g
    B, Sq, H, D = x.q.shape
    dropout = (0.2, 1234, 0, 0, 0)
    keep = [R.keep_mask(dropout, b, H, g.lq, g.lk).to(x.q.device) for b in range(B)]
    rescale = O.drop_rescale(dropout[0])
    e_out, e_lse = R.attention(x.q, x.k, x.v, causal=True, keep=keep, rescale=rescale)
    m_out, _ = V.model_attention(x.q, x.k, x.v, causal=True, keep=torch.stack(keep), rescale=rescale)
    out, lse = torch.full_like(x.q, 5.0), torch.full((B, H, Sq), 5.0, device=x.q.device)
    be.fwd(x.q, x.k, x.v, softmax_scale=x.scale, causal=True, out=out, lse=lse, dropout=dropout)
    assert torch.equal(e_lse, x.exact[1])                                     # (the reference's lse ignores the mask)
    bad = V.failures(f"{family}.dropout.out", out, e_out, m_out, "out", x.rows)
    bad += V.lse_failures(f"{family}.dropout.lse", lse, e_lse)
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ packed forward
PACKED_ENV = dict(RFA_FWD_FORM="8x32", RFA_FWD_KV_NSPLIT="1")


def packed_fwd_plan(C_, lib, D, env, dtype=0):
    """(workspace bytes, split-KV shares) the library reports for the forward of the packed batch of tests/_valueref.py under
    the switches `env` — host side; the cu_seqlens pointers are those of a real (host) int32 tensor"""
    cq, ck = V.cu_of(V.PACKED_LENS_Q), V.cu_of(V.PACKED_LENS_K)
    keep = torch.tensor(cq + ck, dtype=torch.int32)
    g = BR.Geometry("packed", "value", max(V.PACKED_LENS_Q), max(V.PACKED_LENS_K), True, BR.NOWIN, 0, len(cq) - 1, None)
    a = BR.fwd_args(C_, g, *HEADS, D, env, dtype)
    a.mask_shift = 0
    a.cu_seqlens_q, a.cu_seqlens_k = keep.data_ptr(), keep.data_ptr() + 4 * len(cq)
    a.total_q = cq[-1]
    return BR.fwd_shares(lib, a)


def check_packed_case(C_, lib, D=128):
    """the packed case runs the unsplit 8 x 32 form it names: one share, no workspace"""
    assert packed_fwd_plan(C_, lib, D, PACKED_ENV) == (0, 1)
    assert packed_fwd_plan(C_, lib, D, dict(RFA_FWD_KV_NSPLIT="3"))[1] == 3     # (... and the plan function does see the packed call)


@pytest.mark.parametrize("family", [pytest.param(f, marks=[] if f in ("stairs-up", "late-spike") else [_EXT]) for f in V.FAMILIES])
def test_fwd_packed_batch_on_the_value_family(monkeypatch, family):
    """one packed (cu_seqlens) causal batch — a long, an empty, a short and a square sequence, the family built per sequence so
    that every sequence holds trigger and sibling rows — against the per-sequence fp64 attention and the per-sequence model;
    plain outputs and overwritten accumulators; two runs, the same bits"""
    from ring_flash_attn import _C

    be = GF._be()
    dev = GF._dev()
    check_packed_case(_C, be.lib)
    GF._setenv(monkeypatch, PACKED_ENV)
    D = 128
    cq, ck = V.cu_of(V.PACKED_LENS_Q), V.cu_of(V.PACKED_LENS_K)
    q, k, v, _ = (t.to(dev) for t in V.make_packed_inputs(family, V.PACKED_LENS_Q, V.PACKED_LENS_K, *HEADS, D, BF,
                                                          9500 + V.FAMILIES.index(family)))
    e_out, e_lse = R.attention(q, k, v, causal=True, cu_seqlens_q=cq, cu_seqlens_k=ck)
    m_out, _ = V.packed_model_forward(q, k, v, cq, ck)
    _, rows = V.packed_witness(q, k, cq, ck)
    T, H = q.shape[0], q.shape[1]
    kw = dict(softmax_scale=D ** -0.5, causal=True, cu_seqlens_q=torch.tensor(cq, dtype=torch.int32, device=dev),
              cu_seqlens_k=torch.tensor(ck, dtype=torch.int32, device=dev), max_seqlen_q=max(V.PACKED_LENS_Q),
              max_seqlen_k=max(V.PACKED_LENS_K))

    def run():
        out, lse = torch.full_like(q, 5.0), torch.full((H, T), 5.0, device=dev)
        be.fwd(q, k, v, out=out, lse=lse, **kw)
        oa, la = torch.full((T, H, D), float("nan"), device=dev), torch.full((H, T), float("nan"), device=dev)
        be.fwd(q, k, v, out_acc=oa, lse_acc=la, acc_init=True, **kw)
        return dict(plain=(out, lse), init=(oa, la))

    res = run()
    bad = []
    for mode, (o, l) in res.items():
        bad += V.failures(f"{family}.packed.{mode}.out", o, e_out, m_out, "out", rows)
        bad += V.lse_failures(f"{family}.packed.{mode}.lse", l, e_lse)
    assert not bad, "; ".join(bad)
    _same_bits(f"{family}.packed", res, run())


# ------------------------------------------------------------------------------------------------ backward
def check_bwd(tag, res, x):
    bad = []
    for mode, grads in res.items():
        for n, (nm, got) in enumerate(zip(("dq", "dk", "dv"), grads)):
            bad += V.failures(f"{tag}.{mode}.{nm}", got, x.exact[2 + n], x.model[2 + n], "grad", x.rows if nm == "dq" else None)
        if x.family == "uniform":
            GF._exact(bad, f"{tag}.{mode}.dk of q = 0", grads[1], 0.0)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("c", _params(bwd_cases(), CORE_BWD))
def test_bwd_form_on_the_value_family(monkeypatch, c):
    from ring_flash_attn import _C

    be = GF._be()
    check_bwd_case(_C, be.lib, c)
    x = _ctx(c)
    GF._setenv(monkeypatch, bwd_env(c))
    be.release_scratch()
    tag = f"{c.family}.{c.form}.{c.shape}.d{c.D}"
    try:
        res = GF.run_bwd(be, x, x.g.band)
        check_bwd(tag, res, x)
        _same_bits(tag, res, GF.run_bwd(be, x, x.g.band))
        if c.form == "5gemm":
            # the hand-off only adds stores to the dK/dV kernel: dK / dV are the 7-GEMM form's bits
            monkeypatch.setenv("RFA_BWD_DS_SPILL", "0")
            ref7 = GF.run_bwd(be, x, x.g.band, modes=("plain",))["plain"]
            assert torch.equal(res["plain"][1], ref7[1]) and torch.equal(res["plain"][2], ref7[2]), "dK/dV differ from the 7-GEMM form"
    finally:
        be.release_scratch()
