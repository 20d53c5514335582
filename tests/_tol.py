"""Stated tolerances of the parity tests — one place, several criteria per comparison.

A comparison `compare(name, got, ref, kind)` of a kernel result with the oracle (bf16 / fp16 io, fp32 accumulation,
N(0,1) inputs) must satisfy ALL of

  1. the non-finite pattern is identical (lse = +inf for rows without a visible key);
  2. max |err|        <= atol + rtol * max|ref|              (catches a single wrong element)
  3. ||err||_F <= fro * ||ref||_F + floor                    (catches a systematic error where |ref| is small
                                                              — late rows of a long causal sequence — which
                                                              criterion 2 cannot see: SURVEY section 8(c); the
                                                              floor, atol/4 per element, only matters when the
                                                              reference itself is numerically zero)
  4. mean |err|       <= mean_abs + mean_rel * mean|ref|     (1e-3 for out)

and `within_2x_naive(...)` states the criterion flash_attn's own tests use for their kernels and the reference's
README quotes: the error against an exact (fp32, unrounded) computation is at most twice the error a naive bf16
implementation of the same formula makes, plus epsilon.

The numbers below were set from the values observed on MI355X (profiles/history/r03_tolerances_observed.txt: every
comparison of the GPU suite logs its metrics when RFA_TOL_LOG names a file) with about 3x head-room.
"""
import os

import torch

#            atol    rtol     fro     mean_abs  mean_rel
# Observed on MI355X (profiles/history/r03_tolerances_observed.txt, 2118 comparisons of the GPU suite), worst case per kind ->
# bound: out max|err|/max|ref| 6.4e-3, fro 2.5e-3, mean/mean 2.0e-3; grad 7.8e-3, 3.0e-3, 2.3e-3; out_ring 6.9e-3,
# 3.2e-3, 2.3e-3; grad_ring 1.04e-2, 4.5e-3, 3.4e-3; lse 1.9e-6 absolute.
KINDS = {
    # oracle and kernel both round out to the io dtype: one ulp of the largest element + accumulated fp32 noise
    "out":  (4e-3,  1.2e-2,  6e-3,   2e-4,     5e-3),
    "lse":  (2e-5,  2e-6,    1e-6,   5e-6,     5e-7),
    # gradients: sums over up to S terms, rounded to the io dtype once (more often across ring steps: "grad_ring")
    "grad": (4e-3,  1.6e-2,  8e-3,   3e-4,     6e-3),
    # schedules over several ranks: block results are rounded to the io dtype at different points than in the
    # reference (fused fp32 merge vs bf16 block outputs): a few ulp of the largest element
    "out_ring":  (8e-3, 1.6e-2, 8e-3,   3e-4, 6e-3),
    "lse_ring":  (5e-5, 5e-6,   2e-6,   1e-5, 1e-6),
    "grad_ring": (8e-3, 2.4e-2, 1.2e-2, 5e-4, 8e-3),
}
# the Frobenius criterion is relative; a reference that is (numerically) zero — a query that sees a single key has
# dQ = 0 exactly — is covered by this absolute floor per element, as a fraction of the kind's atol
FRO_FLOOR = 0.25


def metrics(got, ref, on_device=False):
    """on_device: the same figures computed where the tensors live (tens of millions of elements: no copy to the host)"""
    got, ref = got.detach().float(), ref.detach().float()
    if not on_device:
        got, ref = got.cpu(), ref.cpu()
    fin = torch.isfinite(ref)
    same_pattern = bool(torch.equal(torch.isfinite(got), fin))
    if not fin.any():
        return dict(same_pattern=same_pattern, max_err=0.0, max_ref=0.0, fro=0.0, err_norm=0.0, ref_norm=0.0,
                    mean_err=0.0, mean_ref=0.0, n=0)
    g, r = got[fin].double(), ref[fin].double()
    e = (g - r).abs()
    nr = r.norm().item()
    return dict(same_pattern=same_pattern, max_err=e.max().item(), max_ref=r.abs().max().item(),
                fro=(e.norm().item() / nr) if nr > 0 else float("inf"), err_norm=e.norm().item(), ref_norm=nr,
                mean_err=e.mean().item(), mean_ref=r.abs().mean().item(), n=int(fin.sum()))


def _log(name, kind, m):
    path = os.environ.get("RFA_TOL_LOG")
    if path:
        try:
            with open(path, "a") as f:
                f.write(f"{kind:10s} max_err {m['max_err']:.3e} (/max_ref {m['max_err'] / max(m['max_ref'], 1e-30):.3e}) "
                        f"fro {m['fro']:.3e} mean_err {m['mean_err']:.3e} (/mean_ref "
                        f"{m['mean_err'] / max(m['mean_ref'], 1e-30):.3e}) max_ref {m['max_ref']:.3e}  {name}\n")
        except OSError:
            pass


def failures(name, got, ref, kind, scale=1.0, on_device=False):
    """list of violated criteria (empty = pass).  scale: multiplies every bound (fp16 / special inputs)."""
    if tuple(got.shape) != tuple(ref.shape):
        return [f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"]
    atol, rtol, fro, mabs, mrel = (x * scale for x in KINDS[kind])
    m = metrics(got, ref, on_device)
    _log(name, kind, m)
    bad = []
    if not m["same_pattern"]:
        bad.append(f"{name}: non-finite pattern differs")
    lim = atol + rtol * m["max_ref"]
    if not m["max_err"] <= lim:
        bad.append(f"{name}: max|err| {m['max_err']:.3e} > {lim:.3e}")
    lim = fro * m["ref_norm"] + FRO_FLOOR * atol * m["n"] ** 0.5
    if not m["err_norm"] <= lim:
        bad.append(f"{name}: ||err||_F {m['err_norm']:.3e} > {fro:.1e} ||ref||_F + floor = {lim:.3e} "
                   f"(relative Frobenius error {m['fro']:.3e})")
    lim = mabs + mrel * m["mean_ref"]
    if not m["mean_err"] <= lim:
        bad.append(f"{name}: mean|err| {m['mean_err']:.3e} > {lim:.3e}")
    return bad


def compare(name, got, ref, kind, scale=1.0):
    bad = failures(name, got, ref, kind, scale)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------
# the "<= 2x the error of a naive bf16 implementation" criterion
def exact_attention(q, k, v, do, causal, window=(-1, -1)):
    """fp32 attention on the upcast inputs with autograd, nothing rounded: (out, dq, dk, dv) in fp32.
    q (B,Sq,H,D), k/v (B,Sk,Hk,D); bottom-right aligned causal mask, flash_attn window semantics."""
    return _attention(q, k, v, do, causal, window, lambda x: x)


def naive_lowp_attention(q, k, v, do, causal, window=(-1, -1)):
    """the same formula as a naive implementation in the io dtype would run it: every matmul result and the
    probabilities are rounded to the io dtype (fp32 accumulation inside a matmul, as the hardware does);
    gradients by autograd through the roundings (straight-through)."""
    dt = q.dtype

    def rnd(x):
        return x + (x.to(dt).float() - x).detach()

    return _attention(q, k, v, do, causal, window, rnd)


def _attention(q, k, v, do, causal, window, rnd):
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    B, Sq, H, D = qf.shape
    Sk, Hk = kf.shape[1], kf.shape[2]
    g = H // Hk
    ke = kf.repeat_interleave(g, dim=2)
    ve = vf.repeat_interleave(g, dim=2)
    s = rnd(torch.einsum("bqhd,bkhd->bhqk", qf, ke) * (D ** -0.5))
    i = torch.arange(Sq).view(-1, 1) + (Sk - Sq)
    j = torch.arange(Sk).view(1, -1)
    mask = torch.zeros(Sq, Sk, dtype=torch.bool)
    wl, wr = window
    if causal:
        wr = 0
    if wr >= 0:
        mask |= j > i + wr
    if wl >= 0:
        mask |= j < i - wl
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)                    # rows without a visible key
    out = rnd(torch.einsum("bhqk,bkhd->bqhd", rnd(p), ve))
    out.backward(do.float())
    return out.detach(), rnd(qf.grad).detach(), rnd(kf.grad).detach(), rnd(vf.grad).detach()


def within_2x_naive(name, got, exact, naive, eps=1e-5):
    """max|got - exact| <= 2 max|naive - exact| + eps   (flash_attn's own test criterion)"""
    e_got = (got.detach().float().cpu() - exact).abs().max().item()
    e_naive = (naive - exact).abs().max().item()
    path = os.environ.get("RFA_TOL_LOG")
    if path:
        try:
            with open(path, "a") as f:
                f.write(f"2x-naive   err {e_got:.3e} vs naive {e_naive:.3e} (ratio {e_got / max(e_naive, 1e-30):.2f})  {name}\n")
        except OSError:
            pass
    assert e_got <= 2 * e_naive + eps, f"{name}: max|err| vs exact {e_got:.3e} > 2 x naive-lowp {e_naive:.3e}"
