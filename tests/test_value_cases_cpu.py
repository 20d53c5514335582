"""The input families of the value-range tests (tests/_valueref.py), checked on the CPU: every family shows, at every shape
tests/test_gpu_value_ranges.py runs it at, what it was written for — witness events of the forward's deferred rescale (rows
rescaled mid-loop from a stale max with alpha in [2^-6, 2^-0.5] while the earlier tiles still carry mass), or its own stated
property — and plain N(0,1) inputs show none: the reason these tests exist.  The rounding model stays finite, the tile
emulation of the forward passes the criterion against fp64 and every planted arithmetic fault fails it on the families that
claim to witness it; the CPU test backend passes it forward and backward; and every GPU case reports, through the host-side
plan functions of the C ABI (the library loads without a device), the form it names."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _blockref as R                            # noqa: E402
import _valueref as V                            # noqa: E402
import test_gpu_value_ranges as GV               # noqa: E402  (its case lists; nothing in it touches a device at import)

BF, FP16 = torch.bfloat16, torch.float16
H, Hk = GV.HEADS
WITNESSED = ("stairs-up", "late-spike")                       # families that must show witness events (the others: their own property)
MIN_EVENTS = 8                                               # (wave, tile) events with a witness row, per head


def _gpu_contexts():
    """(family, shape, D, Dv, dtype) of every reference the GPU file computes"""
    return sorted({(c.family, c.shape, c.D, c.Dv, c.dtype) for c in GV.fwd_cases() + GV.bwd_cases()},
                  key=lambda t: (t[0], t[1], t[2], t[3], str(t[4])))


_CACHE = {}


def _ctx(family, shape, D=128, Dv=128, dtype=BF):
    key = (family, shape, D, Dv, dtype)
    if key not in _CACHE:
        while len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE)))
        g = V.SHAPES[shape]
        band = dict(causal=g.causal, window=g.window, shift=g.shift)
        q, k, v, do = V.make_inputs(family, g.B, g.lq, g.lk, H, Hk, D, dtype, 11, Dv=Dv, **band)
        s = V.scores(q, k, D ** -0.5, **band)
        _CACHE[key] = dict(g=g, band=band, q=q, k=k, v=v, do=do, s=s, witness=V.witness(s))
    return _CACHE[key]


def _with_refs(x):
    if "exact" not in x:
        x["exact"] = R.attention(x["q"], x["k"], x["v"], dout=x["do"], autograd=x["v"].shape[-1] != x["q"].shape[-1], **x["band"])
        x["model"] = V.model_attention(x["q"], x["k"], x["v"], x["do"], **x["band"])
        x["rows"] = x["witness"][1].permute(0, 2, 1)
    return x


@pytest.mark.parametrize("key", _gpu_contexts(), ids=lambda k: f"{k[0]}-{k[1]}-d{k[2]}v{k[3]}-{'bf16' if k[4] is BF else 'fp16'}")
def test_family_shows_what_its_row_of_the_table_claims(key):
    family, shape, D, Dv, dtype = key
    x = _ctx(*key)
    g, s = x["g"], x["s"]
    events, rows, rescales = x["witness"]
    fin = torch.isfinite(s)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if family in WITNESSED:
        assert int(events.min()) >= MIN_EVENTS, (key, events.tolist())
        assert bool(rows.any(-1).all())                                   # ... in every (batch, head)
    elif family == "gauss":
        if g.window[0] < 0:                                               # (a sliding window drops old tiles: rescales are ordinary there)
            assert int(rescales.max()) == 0 and int(events.max()) == 0, (key, rescales.tolist())
    elif family == "stairs-down":
        # the max of every stepped row sits in the row's first visible tile; the last tile's mass runs from ordinary down to
        # below the smallest fp32 denormal
        steep = V.stair_a(g.lq) >= 4.0                                    # (8 nats per tile and more: beyond the noise)
        if g.window[0] < 0:
            assert bool((s.argmax(-1)[..., steep] < V.TILE).all())
        if not g.causal:
            tail = p[..., (g.lk - 1) // V.TILE * V.TILE:].sum(-1)
            assert float(tail.max()) > 2.0 ** -24 and float(tail.min()) < 2.0 ** -149, (key, float(tail.max()), float(tail.min()))
    elif family in ("offset+80", "offset-80"):
        sign = 1.0 if family == "offset+80" else -1.0
        assert bool(((sign * s[fin]) > V.OFFSET - 40).all())               # every logit on its side, far from 0
        assert float((sign * lse).min()) > V.OFFSET - 30 and float((sign * lse).max()) < V.OFFSET + 30, (key, float(lse.min()), float(lse.max()))
    elif family == "one-hot":
        pass                                                               # (its own property: below)
    elif family == "uniform":
        assert bool((x["q"] == 0).all()) and bool((s[fin] == 0).all())
        n = fin.sum(-1, keepdim=True).double()
        assert torch.allclose(p[fin], (1.0 / n).expand_as(p)[fin], rtol=1e-12, atol=0)
    if family == "one-hot":
        assert float((p.amax(-1) > 0.99).double().mean()) >= 0.9, key
    if family == "late-spike":
        pairs = V.spike_pairs(g.lq, g.lk, g.causal, g.window, g.shift)
        last = V.last_visible(g.lq, g.lk, g.causal, g.window, g.shift)
        assert len(pairs) == (g.lq + V.GROUP - 1) // V.GROUP
        for i, j in pairs:
            assert j // V.TILE == int(last[i]) // V.TILE or int(last[i]) - j <= 2      # in the last visible tile of its row
            assert float(s[:, 0, i, j].min()) > 50.0                                   # about + 60 nats on head 0 of every batch entry
        if g.causal:
            assert {int(last[i]) - j for i, j in pairs} == {0, 1, 2}                   # on the diagonal, and just below it


@pytest.mark.parametrize("family", V.FAMILIES)
def test_packed_batch_holds_witnesses_in_every_sequence(family):
    """the packed case of tests/test_gpu_value_ranges.py: the family is built per sequence, so EVERY non-empty sequence — the
    77-row one included — shows witness events of its own, at least 8 per head over the batch for the witnessed families and at
    least 2 per head in each sequence (its two full 32-row groups); the emulation and the model agree per sequence; each planted
    `alpha` fault fails the criterion on the witnessed families' packed batch too"""
    cq, ck = V.cu_of(V.PACKED_LENS_Q), V.cu_of(V.PACKED_LENS_K)
    q, k, v, _ = V.make_packed_inputs(family, V.PACKED_LENS_Q, V.PACKED_LENS_K, H, Hk, 128, BF, 21)
    assert q.shape[0] == cq[-1] and k.shape[0] == ck[-1]
    events, rows = V.packed_witness(q, k, cq, ck)
    live = [n for n, (lq, lk) in enumerate(zip(V.PACKED_LENS_Q, V.PACKED_LENS_K)) if lq and lk]
    assert len(live) == 3 and len(events) == 4 and int(events[1].sum()) == 0
    if family in WITNESSED:
        assert int(sum(events).min()) >= MIN_EVENTS, [e.tolist() for e in events]
        for n in live:
            assert int(events[n].min()) >= 2, (family, n, events[n].tolist())
            assert bool(rows[cq[n]:cq[n + 1]].any(0).all())
    elif family in ("gauss", "uniform"):
        assert int(sum(events).max()) == 0 and not bool(rows.any())
    e_out, e_lse = R.attention(q, k, v, causal=True, cu_seqlens_q=cq, cu_seqlens_k=ck)
    m_out, m_lse = V.packed_model_forward(q, k, v, cq, ck)
    assert bool(torch.isfinite(m_out).all()) and bool(torch.isfinite(m_lse).all())
    for fault in (None,) + ALPHA_FAULTS:
        outs, lses = [], []
        for sq, sk, sv, _ in V.per_sequence(q, k, v, q, cq, ck):
            if sq.shape[1] == 0:
                continue
            o, l = V.emulate_forward(sq, sk, sv, causal=True, fault=fault)
            outs.append(o[0])
            lses.append(l[0])
        bad = V.failures("packed.emu.out", torch.cat(outs), e_out, m_out, "out", rows) + V.lse_failures("packed.emu.lse", torch.cat(lses, 1), e_lse)
        if fault is None or family in ("gauss", "uniform"):
            assert not bad, (family, fault, bad)
        elif family in WITNESSED:
            assert bad, f"{fault} passes on the packed {family} batch"


@pytest.mark.parametrize("shape", ["split"])
def test_split_kv_shares_lie_far_apart_on_the_stairs(shape):
    """stairs-up / stairs-down at the split-KV shape: the lse of the two halves of the key range differ by more than 88 nats on
    rows of every 32-row group — one share's weight underflows in the combine (fp32: exp(-88) is the smallest normal)"""
    for family in ("stairs-up", "stairs-down"):
        x = _ctx(family, shape)
        s, g = x["s"], x["g"]
        half = g.lk // 2
        gap = (torch.logsumexp(s[..., :half], -1) - torch.logsumexp(s[..., half:], -1)).abs()
        far = (gap > 88.0) & torch.isfinite(gap)
        groups = far[..., : g.lq // V.GROUP * V.GROUP].view(*far.shape[:-1], -1, V.GROUP).any(-1)
        assert bool(groups.all()), family
        assert bool((gap[torch.isfinite(gap)] < 1.0).any()), family        # ... next to rows whose shares weigh the same


@pytest.mark.parametrize("dtype", [BF, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("family", V.FAMILIES)
def test_model_attention_stays_finite(family, dtype):
    for shape in ("rect-causal", "window"):
        x = _ctx(family, shape, dtype=dtype)
        out = V.model_attention(x["q"], x["k"], x["v"], x["do"], **x["band"])
        for n, t in zip(("out", "lse", "dq", "dk", "dv"), out):
            assert bool(torch.isfinite(t).all()), (family, shape, n)


# ---- the tile emulation: correct, and with each planted fault -----------------------------------------------------------
def _emu_failures(x, fault=None):
    x = _with_refs(x)
    out, lse = V.emulate_forward(x["q"], x["k"], x["v"], fault=fault, **x["band"])
    return V.failures("emu.out", out, x["exact"][0], x["model"][0], "out", x["rows"]) + V.lse_failures("emu.lse", lse, x["exact"][1])


EMU_SHAPES = ("rect", "rect-causal", "window", "split")


@pytest.mark.parametrize("shape", EMU_SHAPES)
@pytest.mark.parametrize("family", V.FAMILIES)
def test_emulated_forward_passes_the_criterion(family, shape):
    assert not _emu_failures(_ctx(family, shape))


# fault -> the (family, shape, dtype) that claim to witness it
ALPHA_FAULTS = ("alpha-skips-siblings", "alpha-of-trigger-row")
CLAIMS = {
    "alpha-skips-siblings": [(f, s, BF) for f in WITNESSED for s in ("rect", "rect-causal", "split")],
    "alpha-of-trigger-row": [(f, s, BF) for f in WITNESSED for s in ("rect", "rect-causal", "split")],
    "lsum-not-rescaled": [(f, s, BF) for f in WITNESSED for s in ("rect", "rect-causal", "split")],
    # a running max that starts at 0: P = exp(s) underflows where every logit of a row lies far below 0 — the windowed
    # stairs-down rows (about -8 nats per 32 keys down the diagonal) in any dtype, the -80 offset once P is rounded to fp16
    "neg-inf-max-as-zero": [("stairs-down", "window", BF), ("offset-80", "rect-causal", FP16), ("offset-80", "rect", FP16)],
}


@pytest.mark.parametrize("fault", list(CLAIMS))
def test_planted_fault_fails_the_criterion_where_a_family_claims_it(fault):
    assert len({f for f, _, _ in CLAIMS[fault]}) >= 2, "every fault is claimed by at least two families"
    for family, shape, dtype in CLAIMS[fault]:
        assert _emu_failures(_ctx(family, shape, dtype=dtype), fault), f"{fault} passes on {family} at {shape}"


@pytest.mark.parametrize("fault", ALPHA_FAULTS + ("lsum-not-rescaled",))
def test_gaussian_and_uniform_inputs_cannot_see_a_rescale_fault(fault):
    """the documented reason for the families: on N(0,1) logits the only rescale is a wave's first, alpha = 0 times O = 0"""
    for family in ("gauss", "uniform"):
        for shape in ("rect", "rect-causal", "split"):
            assert not _emu_failures(_ctx(family, shape), fault), (fault, family, shape)


def test_a_threshold_that_is_never_advanced_changes_no_value():
    """mthr left at -inf rescales at every tile: m, alpha and P stay consistent, so the arithmetic is the deferred form's up to
    rounding — the mutant is equivalent, no value test can reject it (it costs time, not correctness): it passes the criterion
    on every family, and it is the schedule of defer = 0"""
    for family in V.FAMILIES:
        x = _ctx(family, "rect-causal")
        assert not _emu_failures(x, "threshold-not-advanced"), family
        a = V.emulate_forward(x["q"], x["k"], x["v"], fault="threshold-not-advanced", **x["band"])
        b = V.emulate_forward(x["q"], x["k"], x["v"], defer=float("-inf"), **x["band"])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), family


# ---- the CPU test backend -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["rect-causal", "window"])
@pytest.mark.parametrize("family", V.FAMILIES)
def test_cpu_backend_passes_the_criterion(family, shape):
    from _ref_backend import RefBackend

    be = RefBackend(serves=("mask_shift",))
    x = _with_refs(_ctx(family, shape))
    q, k, v, do, g = x["q"], x["k"], x["v"], x["do"], x["g"]
    B, Sq, Hq, D = q.shape
    out, lse = torch.empty_like(q), torch.empty(B, Hq, Sq)
    be.fwd(q, k, v, softmax_scale=D ** -0.5, out=out, lse=lse, **g.band)
    ex, mo = x["exact"], x["model"]
    bad = V.failures("cpu.out", out, ex[0], mo[0], "out", x["rows"]) + V.lse_failures("cpu.lse", lse, ex[1])
    delta = (do.double() * ex[0]).sum(-1).permute(0, 2, 1).float().contiguous()
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, ex[1].float().contiguous(), delta, softmax_scale=D ** -0.5, dq=dq, dk=dk, dv=dv, **g.band)
    for n, (nm, got) in enumerate(zip(("dq", "dk", "dv"), (dq, dk, dv))):
        bad += V.failures(f"cpu.{nm}", got, ex[2 + n], mo[2 + n], "grad", x["rows"] if nm == "dq" else None)
    if family == "uniform":
        assert bool((dk == 0).all())
    assert not bad, "; ".join(bad)


# ---- every GPU case runs the form it names --------------------------------------------------------------------------------
def test_gpu_cases_report_the_form_they_name():
    from ring_flash_attn import _C

    lib = _C.load()
    fwd, bwd = GV.fwd_cases(), GV.bwd_cases()
    for c in fwd:
        GV.check_fwd_case(_C, lib, c)
    for c in bwd:
        GV.check_bwd_case(_C, lib, c)
    GV.check_packed_case(_C, lib)
    for fam in V.FAMILIES:
        assert {(c.form, c.shape) for c in fwd if c.family == fam and c.D == c.Dv == 128 and c.dtype is BF} == set(GV.FWD_FORMS_128)
        assert {(c.form, c.shape) for c in bwd if c.family == fam and c.D == c.Dv == 128 and c.dtype is BF} == set(GV.BWD_FORMS_128)
        assert {(c.D, c.Dv) for c in fwd if c.family == fam} >= {(128, 128), (64, 64), (80, 80), (40, 40), (192, 192), (256, 256), (192, 128)}
    assert GV.CORE_FWD <= set(GV.FWD_FORMS_128) and GV.CORE_BWD <= set(GV.BWD_FORMS_128)


def test_poison_cases_report_the_form_they_name():
    """tests/test_gpu_poison.py: the dense cases' forms, and the dS hand-off plans of the packed batch (whole, K/V-head chunks,
    query-head fractions), from the host-side plan functions"""
    import test_gpu_poison as GP
    from ring_flash_attn import _C

    lib = _C.load()
    for fwd, bwd, D, Dv in GP.CASES:
        GP._check_forms(lib, fwd, bwd, D, Dv)
    for fwd, bwd, D, Dv in GP.PACKED_CASES:
        GP._check_packed_forms(lib, fwd, bwd, D, Dv)
    assert all(c[0] != "p8x32" for c in GP.PACKED_CASES)                 # (the persistent forward declines packed input)
    assert set(GP.CORE) <= set(GP.CASES)
    assert {c[0] for c in GP.CASES} >= {"8x32", "4x32", "p8x32", "split3"}
    assert {c[1] for c in GP.CASES} >= {"7gemm", "5gemm", "dkdv128", "dkdv256-2"}
    assert {(c[2], c[3]) for c in GP.CASES} == {(128, 128), (64, 64), (80, 80), (192, 192), (192, 128)}
    limits = [GP._packed_scratch_limit(_C, lib, f, 128) for f in ("5gemm", "5gemm-kv-chunks", "5gemm-q-fractions")]
    assert limits[0] is None and limits[1] > limits[2] > 0
    # every padded stride is a multiple of 8 elements: the backend passes such views through (backend._rows16)
    assert GP.PAD_D % 8 == 0 and all((D + GP.PAD_D) % 8 == 0 for _, _, D, _ in GP.CASES)
