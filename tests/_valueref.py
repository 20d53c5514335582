"""TEST INFRASTRUCTURE: attention inputs whose logits are NOT N(0,1), the kernels' rounding model, and a tile emulation of
the forward's deferred online-softmax rescale.  No test in here (tests/test_value_cases_cpu.py checks this file,
tests/test_gpu_value_ranges.py runs the families through every kernel form).

Families.  Each starts from seeded N(0,1) q, k, v, do and adds a rank-one term q_i += a_i w, k_j += b_j w with w the constant
direction of length softmax_scale^-1/2 (softmax_scale |w|^2 = 1): the logits are a_i b_j plus noise of order one (the cross
terms a_i (w.k_j) and b_j (w.q_i) have standard deviation D^-1/4 per unit of a / b: they blur the steps, they do not remove
them).  The sum is rounded to the io dtype; every reference sees the rounded tensors.

  stairs-up    b_j = floor(j / 32); a_i cycles inside every 32-row group through STEPS nats per step; every third group is
               capped at 2 nats per step (4 nats = 5.8 log2 units per 64-key tile: below the forward's defer threshold of 8, so
               such a group skips a tile and rescales at the next), the others hold a row that triggers at every tile
  stairs-down  stairs-up with b negated: the max is in the first tile, later tiles underflow gradually
  late-spike   no rank-one term: per 32-row group one planted pair (i*, j*) with k_j* += t q_i*, softmax_scale t |q_i*|^2 = 60
               nats, j* in the last visible tile of row i* (with a right bound: on the diagonal, one and two below it in
               turn); the other rows of the group see that key at about 60 / sqrt(D) N(0,1) nats — the siblings
  offset+80    a_i b_j = +80 for every pair;   offset-80: -80
  one-hot      q scaled by ONE_HOT: logits of standard deviation 200, max P > 0.99 on 90 % of the rows
  uniform      q = 0 exactly: every logit 0, P = 1 / n, dK = 0
  gauss        the control: plain N(0,1)

The criterion (`failures` / `check`), flash_attn's: with `exact` the fp64 attention of tests/_blockref.py and `model` the
rounding model below,  max|got - exact| <= 2 max|model - exact| + atol  and  ||got - exact||_F <= 2 ||model - exact||_F +
FRO_FLOOR atol sqrt(n),  atol and FRO_FLOOR those of the matching row of tests/_tol.py — on the whole tensor and again on the
witness rows alone."""
import math
import os

import torch

import _bandref as BR
import _blockref as R
import _tol

FAMILIES = ("stairs-up", "stairs-down", "late-spike", "offset+80", "offset-80", "one-hot", "uniform", "gauss")
STEPS = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0)           # nats per 32-key step
# one-hot: the gap between the two largest of n Gaussian logits of standard deviation s is about exponential with mean
# s / sqrt(2 ln n); max P > 0.99 (a gap above 4.6 nats) on 90 % of the rows takes s of about 200 at n = 520 .. 4096 — at s = 30
# only 60 % of the rows are one-hot (tests/test_value_cases_cpu.py asserts the 90 %)
SPIKE, OFFSET, ONE_HOT = 60.0, 80.0, 200.0
TILE, GROUP, DEFER = 64, 32, 8.0                 # csrc/rfa_fwd.hip: kFwdKV, rows per wave, RFA_FWD_DEFER (log2 units)
LN2 = math.log(2.0)

# the shapes of the value-range cases: the smallest with several key tiles and an unaligned tail (44 query rows, 8 keys)
_G = lambda name, lq, lk, causal, window, off, B=2: BR.Geometry(name, "value", lq, lk, causal, window, off, B, None)
SHAPES = {g.name: g for g in (
    _G("rect", 300, 520, False, BR.NOWIN, 220),                  # every key visible
    _G("rect-causal", 300, 520, True, BR.NOWIN, 220),            # bottom-right aligned diagonal
    _G("square", 640, 640, True, BR.NOWIN, 0),
    _G("square512", 512, 512, True, BR.NOWIN, 0),                # the smallest the balanced dK/dV schedule takes
    _G("window", 300, 520, True, (130, 0), 285),                 # window (130, 0), mask_shift 65
    _G("persistent", 1000, 1000, True, BR.NOWIN, 0, B=1),        # the smallest tests/test_gpu_kernels.py runs the persistent form at
    _G("split", 200, 4096, True, BR.NOWIN, 3896),                # few rows against 64 key tiles: split-KV
)}


def stair_a(lq):
    """a_i of the stairs families, (lq,) fp64"""
    i = torch.arange(lq)
    g, r = i // GROUP, i % GROUP
    a = torch.tensor(STEPS, dtype=torch.float64)[(r + g) % len(STEPS)]
    return torch.where(g % 3 == 2, a.clamp(max=2.0), a)


def last_visible(lq, lk, causal, window=(-1, -1), shift=0):
    """(lq,) the last visible key of every row, -1 for a row that sees none"""
    vis = R.visible(lq, lk, causal, window, shift)
    j = torch.arange(lk).view(1, -1).expand(lq, lk)
    return torch.where(vis, j, torch.full_like(j, -1)).amax(1)


def spike_pairs(lq, lk, causal, window=(-1, -1), shift=0):
    """[(i*, j*)] of late-spike: one per 32-row group whose planted row sees a key"""
    if lq == 0 or lk == 0:
        return []
    last = last_visible(lq, lk, causal, window, shift)
    bounded = causal or (window is not None and window[1] >= 0)
    pairs = []
    for g in range((lq + GROUP - 1) // GROUP):
        i = min(g * GROUP + 3 + g % 5, lq - 1)
        jl = int(last[i])
        if jl < 0:
            continue
        if bounded:
            j = max(jl - g % 3, 0)                               # on the diagonal, one below, two below
        else:
            t0 = (jl // TILE) * TILE                              # anywhere in the last tile
            j = t0 + (7 * g) % (jl - t0 + 1)
        pairs.append((i, j))
    return pairs


def make_inputs(family, B, lq, lk, H, Hk, D, dtype, seed, *, Dv=None, causal=False, window=(-1, -1), shift=0):
    """q (B, lq, H, D), k (B, lk, Hk, D), v (B, lk, Hk, Dv), do (B, lq, H, Dv) of `family`, on the CPU, in `dtype`.  The mask
    only places late-spike's planted keys."""
    assert family in FAMILIES, family
    Dv = D if Dv is None else Dv
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    q, k, v, do = mk(B, lq, H, D), mk(B, lk, Hk, D), mk(B, lk, Hk, Dv), mk(B, lq, H, Dv)
    w = D ** -0.25                                               # every component of w: |w|^2 = sqrt(D) = 1 / softmax_scale
    a = b = None
    if family in ("stairs-up", "stairs-down"):
        a = stair_a(lq)
        b = (torch.arange(lk) // GROUP).double() * (1.0 if family == "stairs-up" else -1.0)
    elif family in ("offset+80", "offset-80"):
        a = torch.full((lq,), OFFSET ** 0.5, dtype=torch.float64)
        b = torch.full((lk,), OFFSET ** 0.5 * (1.0 if family == "offset+80" else -1.0), dtype=torch.float64)
    elif family == "one-hot":
        q = q * ONE_HOT
    elif family == "uniform":
        q = torch.zeros_like(q)
    elif family == "late-spike":
        G = H // Hk
        for i, j in spike_pairs(lq, lk, causal, window, shift):
            for hk in range(Hk):                                  # the K/V head follows its FIRST query head
                qi = q[:, i, hk * G]
                t = SPIKE * D ** 0.5 / (qi * qi).sum(-1, keepdim=True)
                k[:, j, hk] += t * qi
    if a is not None:
        q = q + a.view(1, -1, 1, 1) * w
        k = k + b.view(1, -1, 1, 1) * w
    return tuple(t.to(dtype) for t in (q, k, v, do))


# the packed batch of the value-range cases: a long, an empty, a short (two 32-row groups and a tail, four key tiles) and a
# square sequence; the family is built PER SEQUENCE — the stairs restart at every sequence's key 0 and every sequence plants
# its own spikes — so every 32-row group inside a sequence holds trigger and sibling rows
PACKED_LENS_Q = (300, 0, 77, 420)
PACKED_LENS_K = (520, 0, 200, 420)


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def make_packed_inputs(family, lens_q, lens_k, H, Hk, D, dtype, seed, *, Dv=None, causal=True):
    """packed q (T, H, D), k (Tk, Hk, D), v (Tk, Hk, Dv), do (T, H, Dv) of `family`, each sequence made by make_inputs on its own"""
    parts = [make_inputs(family, 1, lq, lk, H, Hk, D, dtype, seed + 101 * n, Dv=Dv, causal=causal)
             for n, (lq, lk) in enumerate(zip(lens_q, lens_k))]
    return tuple(torch.cat([p[i][0] for p in parts], dim=0) for i in range(4))


def per_sequence(q, k, v, do, cu_q, cu_k):
    """[(q, k, v, do)] of every sequence as dense tensors with batch 1"""
    return [tuple(t[a:b].unsqueeze(0) for t, (a, b) in ((q, (qa, qb)), (k, (ka, kb)), (v, (ka, kb)), (do, (qa, qb))))
            for qa, qb, ka, kb in zip(cu_q, cu_q[1:], cu_k, cu_k[1:])]


def packed_model_forward(q, k, v, cu_q, cu_k, causal=True):
    """model_attention per sequence: out (T, H, Dv), lse (H, T), fp32"""
    outs, lses = [], []
    for sq, sk, sv, _ in per_sequence(q, k, v, q, cu_q, cu_k):
        if sq.shape[1] == 0:
            continue
        assert sk.shape[1] > 0, "a sequence with queries and no keys"
        o, l = model_attention(sq, sk, sv, causal=causal)
        outs.append(o[0])
        lses.append(l[0])
    return torch.cat(outs, dim=0), torch.cat(lses, dim=1)


def packed_witness(q, k, cu_q, cu_k, causal=True):
    """(events per sequence and head: list of (H,) tensors, witness rows (T, H) bool) of the packed batch"""
    events, rows = [], []
    for sq, sk, _, _ in per_sequence(q, k, k, q, cu_q, cu_k):
        if sq.shape[1] == 0 or sk.shape[1] == 0:
            events.append(torch.zeros(q.shape[1], dtype=torch.long, device=q.device))
            rows.append(torch.zeros(sq.shape[1], q.shape[1], dtype=torch.bool, device=q.device))
            continue
        ev, r, _ = witness(scores(sq, sk, q.shape[-1] ** -0.5, causal))
        events.append(ev[0])
        rows.append(r[0].transpose(0, 1))
    return events, torch.cat(rows, dim=0)


# ---------------------------------------------------------------------------------------------------------------------
def scores(q, k, scale, causal=False, window=(-1, -1), shift=0, dtype=torch.float64):
    """masked scores (B, H, lq, lk) of dense q (B, lq, H, D), k (B, lk, Hk, D); -inf where the key is not visible"""
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(dtype), k.to(dtype).repeat_interleave(G, dim=2)) * scale
    return s.masked_fill(~R.visible(q.shape[1], k.shape[1], causal, window, shift, q.device), float("-inf"))


def witness(s, tile=TILE, group=GROUP, defer=DEFER):
    """The forward's rescale schedule on masked fp64 scores s (..., lq, lk): the wave-wide test any(mloc > m + defer log2
    units) per `group` rows and `tile` keys, a stale max in between.  A row is a WITNESS of a (wave, tile) rescale when its own
    alpha lies in [2^-6, 2^-0.5] there and the tiles before carry at least 2^-6 of its softmax mass: a wrong alpha on such a
    row changes its result by more than any rounding.  Returns (events (...,): the (wave, tile) pairs with a witness row,
    rows (..., lq) bool, rescales (...,): every (wave, tile) rescale that is not the wave's first)."""
    *lead, lq, lk = s.shape
    ng = (lq + group - 1) // group
    pad = ng * group - lq
    if pad:
        s = torch.cat([s, s.new_full((*lead, pad, lk), float("-inf"))], dim=-2)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse).unsqueeze(-1))
    m = s.new_full(s.shape[:-1], float("-inf"))
    thr = m.clone()
    rows = torch.zeros(s.shape[:-1], dtype=torch.bool, device=s.device)
    events = torch.zeros(lead, dtype=torch.long, device=s.device)
    rescales = events.clone()
    started = torch.zeros((*lead, ng), dtype=torch.bool, device=s.device)
    before = torch.zeros_like(m)
    for t0 in range(0, lk, tile):
        st = s[..., t0:t0 + tile]
        mloc = st.amax(-1)
        trig_g = (mloc > thr).view(*lead, ng, group).any(-1)
        trig = trig_g.repeat_interleave(group, dim=-1)
        mnew = torch.maximum(m, mloc)
        la = torch.where(torch.isinf(m), torch.full_like(m, float("-inf")), (m - mnew) / LN2)
        w = trig & (la >= -6.0) & (la <= -0.5) & (before >= 2.0 ** -6)
        rows |= w
        events += w.view(*lead, ng, group).any(-1).sum(-1)
        rescales += (trig_g & started).sum(-1)
        started |= trig_g
        m = torch.where(trig, mnew, m)
        thr = torch.where(trig, mnew + defer * LN2, thr)
        before = before + p[..., t0:t0 + tile].sum(-1)
    return events, rows[..., :lq], rescales


# ---------------------------------------------------------------------------------------------------------------------
def _rnd(x, dt):
    return x.to(dt).float()


def model_attention(q, k, v, do=None, *, scale=None, causal=False, window=(-1, -1), shift=0, lse=None, delta=None,
                    keep=None, rescale=1.0):
    """The kernels' documented rounding model, independent of them: fp32 on the upcast inputs; scores NOT rounded (they
    stay in the MFMA's fp32 accumulators); the probabilities that enter P V and P^T dO, and the dS that enters dS K and
    dS^T Q, rounded to the io dtype (MFMA operands); out and the plain gradients rounded once.  Dense q (B, lq, H, D), k
    (B, lk, Hk, D), v (B, lk, Hk, Dv).  keep: (B, H, lq, lk) bool — dropout: out takes the kept P times `rescale`, lse is
    the undropped softmax's.  lse / delta (B, H, lq) fp32: what the backward kernels are handed (default: the model's own).
    Returns (out, lse) or (out, lse, dq, dk, dv), fp32."""
    dt = q.dtype
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    Hk, G = k.shape[2], q.shape[2] // k.shape[2]
    ke, ve = k.float().repeat_interleave(G, dim=2), v.float().repeat_interleave(G, dim=2)
    s = scores(q, k, scale, causal, window, shift, dtype=torch.float32)
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m)
    pt = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))           # unnormalised, <= 1: what the kernel rounds
    l = pt.sum(-1, keepdim=True)
    pv = pt if keep is None else torch.where(keep, pt, torch.zeros_like(pt))
    o = torch.einsum("bhqk,bkhd->bqhd", _rnd(pv, dt), ve)
    inv = torch.where(empty, torch.zeros_like(l), rescale / l).permute(0, 2, 1, 3)
    out = _rnd(o * inv, dt)
    mlse = torch.where(empty, torch.full_like(m, float("inf")), m + torch.log(l)).squeeze(-1)
    if do is None:
        return out, mlse
    assert keep is None
    lse = mlse if lse is None else lse.float()
    delta = (do.float() * out).sum(-1).permute(0, 2, 1) if delta is None else delta.float()
    p = torch.exp(s - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse).unsqueeze(-1))
    p = torch.where(torch.isinf(s), torch.zeros_like(p), p)
    dp = torch.einsum("bqhd,bkhd->bhqk", do.float(), ve)
    ds = _rnd(p * (dp - delta.unsqueeze(-1)), dt)
    dq = _rnd(torch.einsum("bhqk,bkhd->bqhd", ds, ke) * scale, dt)
    B, lk = k.shape[0], k.shape[1]
    dk = torch.einsum("bhqk,bqhd->bkhd", ds, q.float()) * scale
    dv = torch.einsum("bhqk,bqhd->bkhd", _rnd(p, dt), do.float())
    fold = lambda t: _rnd(t.reshape(B, lk, Hk, G, t.shape[-1]).sum(3), dt)
    return out, mlse, dq, fold(dk), fold(dv)


FAULTS = ("alpha-skips-siblings", "alpha-of-trigger-row", "lsum-not-rescaled", "threshold-not-advanced", "neg-inf-max-as-zero")


def emulate_forward(q, k, v, *, scale=None, causal=False, window=(-1, -1), shift=0, fault=None, tile=TILE, group=GROUP,
                    defer=DEFER):
    """A blocked online softmax with the forward kernel's geometry (csrc/rfa_fwd.hip: 64-key tiles, the rescale decided per
    32-row wave by any(mloc > mthr), a stale max between rescales, P rounded to the io dtype for P V, lsum the fp32 sum of
    the unrounded P), fp32, CPU.  `fault` plants one arithmetic error:
      alpha-skips-siblings     rows of a rescaling wave that did not cross the threshold themselves keep alpha = 1
      alpha-of-trigger-row     the alpha of the wave's fastest-growing row is applied to all of its rows
      lsum-not-rescaled        O is rescaled, lsum is not
      threshold-not-advanced   mthr stays at -inf: every tile rescales — the SAME arithmetic (m, alpha and P stay
                               consistent), so no value test can see it; listed because its mutant of the kernel is equivalent
      neg-inf-max-as-zero      the running max starts at 0 instead of -inf
    Returns (out fp32 rounded to the io dtype, lse fp32)."""
    assert fault is None or fault in FAULTS, fault
    dt = q.dtype
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    G = q.shape[2] // k.shape[2]
    ve = v.float().repeat_interleave(G, dim=2).permute(0, 2, 1, 3)            # (B, H, lk, Dv)
    s = scores(q, k, scale, causal, window, shift, dtype=torch.float32)
    B, H, lq, lk = s.shape
    ng = (lq + group - 1) // group
    if ng * group - lq:
        s = torch.cat([s, s.new_full((B, H, ng * group - lq, lk), float("-inf"))], dim=2)
    ninf = float("-inf")
    m = s.new_full(s.shape[:-1], 0.0 if fault == "neg-inf-max-as-zero" else ninf)
    thr = s.new_full(s.shape[:-1], ninf)
    if fault == "neg-inf-max-as-zero":
        thr = m + defer * LN2
    l = torch.zeros_like(m)
    o = s.new_zeros((*s.shape[:-1], ve.shape[-1]))
    wave = lambda x: x.view(B, H, ng, group)
    for t0 in range(0, lk, tile):
        st = s[..., t0:t0 + tile]
        mloc = st.amax(-1)
        own = mloc > thr
        trig = wave(own).any(-1, keepdim=True).expand(B, H, ng, group).reshape(m.shape)
        mnew = torch.maximum(m, mloc)
        msafe = torch.where(torch.isinf(mnew), torch.zeros_like(mnew), mnew)
        alpha = torch.exp(m - msafe)                                          # (m = -inf: 0)
        if fault == "alpha-skips-siblings":
            alpha = torch.where(own, alpha, torch.ones_like(alpha))
        elif fault == "alpha-of-trigger-row":
            grow = torch.where(torch.isinf(m), torch.full_like(m, ninf), mnew - m)
            lead = wave(grow).argmax(-1, keepdim=True)
            alpha = wave(alpha).gather(-1, lead).expand(B, H, ng, group).reshape(m.shape)
            alpha = torch.where(torch.isinf(m), torch.zeros_like(alpha), alpha)      # (a first tile multiplies zeros anyway)
        alpha = torch.where(trig, alpha, torch.ones_like(alpha))
        if fault != "lsum-not-rescaled":
            l = l * alpha
        o = o * alpha.unsqueeze(-1)
        m = torch.where(trig, mnew, m)
        if fault != "threshold-not-advanced":
            thr = torch.where(trig, mnew + defer * LN2, thr)
        mc = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp(st - mc.unsqueeze(-1))
        l = l + p.sum(-1)
        o = o + torch.matmul(_rnd(p, dt), ve[:, :, t0:t0 + tile])
    has = l > 0
    out = torch.where(has.unsqueeze(-1), o / torch.where(has, l, torch.ones_like(l)).unsqueeze(-1), torch.zeros_like(o))
    lse = torch.where(has, mc_log(m, l), torch.full_like(l, float("inf")))
    return _rnd(out[:, :, :lq].permute(0, 2, 1, 3), dt), lse[:, :, :lq]


def mc_log(m, l):
    return torch.where(torch.isinf(m), torch.zeros_like(m), m) + torch.log(torch.where(l > 0, l, torch.ones_like(l)))


# ---------------------------------------------------------------------------------------------------------------------
def _log(line):
    path = os.environ.get("RFA_TOL_LOG")
    if path:
        try:
            with open(path, "a") as f:
                f.write(line + "\n")
        except OSError:
            pass


def failures(name, got, exact, model, kind="out", rows=None):
    """violated criteria (empty = pass) of `got` against the fp64 `exact`, with `model` the rounding model's result:
    max|got - exact| <= 2 max|model - exact| + atol;  ||got - exact||_F <= 2 ||model - exact||_F + FRO_FLOOR atol sqrt(n);
    the non-finite pattern that of `exact`.  rows: a bool mask over got's leading dims (got.shape[:rows.dim()]) — the
    criterion is evaluated a second time on those rows alone."""
    atol = _tol.KINDS[kind][0]
    got, exact, model = (t.detach().double() for t in (got, exact, model))          # (on got's own device)
    if got.shape != exact.shape:
        return [f"{name}: shape {tuple(got.shape)} vs {tuple(exact.shape)}"]
    bad = []
    fin = torch.isfinite(exact)
    if not torch.equal(torch.isfinite(got), fin):
        bad.append(f"{name}: non-finite pattern differs")
    eg = torch.where(fin, (got - exact).abs(), torch.zeros_like(exact)).nan_to_num(nan=float("inf"))
    em = torch.where(fin, (model - exact).abs(), torch.zeros_like(exact))
    parts = [("", eg, em)]
    if rows is not None and bool(rows.any()):
        r = rows.to(eg.device)
        parts.append((" [witness rows]", eg[r], em[r]))
    for tag, g, e in parts:
        n = g.numel()
        if not n:
            continue
        gm, mm, gf, mf = g.max().item(), e.max().item(), g.norm().item(), e.norm().item()
        _log(f"2x-model   {kind:5s} max_err {gm:.3e} vs model {mm:.3e} (ratio {gm / max(2 * mm + atol, 1e-300):.2f} of the bound) "
             f"fro {gf:.3e} vs model {mf:.3e} (ratio {gf / max(2 * mf + _tol.FRO_FLOOR * atol * n ** 0.5, 1e-300):.2f})  {name}{tag}")
        if not gm <= 2 * mm + atol:
            bad.append(f"{name}{tag}: max|err| {gm:.3e} > 2 x model {mm:.3e} + {atol:.0e}")
        lim = 2 * mf + _tol.FRO_FLOOR * atol * n ** 0.5
        if not gf <= lim:
            bad.append(f"{name}{tag}: ||err||_F {gf:.3e} > 2 x model {mf:.3e} + floor = {lim:.3e}")
    return bad


def check(name, got, exact, model, rows=None, kind="out"):
    bad = failures(name, got, exact, model, kind, rows)
    assert not bad, "; ".join(bad)


def lse_failures(name, got, exact):
    """lse by tests/_tol.py kind `lse`: absolute plus relative, meaningful at +-80 and beyond"""
    return _tol.failures(name, got, exact.float(), "lse")
