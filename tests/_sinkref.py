"""TEST INFRASTRUCTURE: the fp64 reference of attention with sinks.  No test in here.

`attention` is the definition, written out: per sequence and head the scores softmax_scale * q.k are built explicitly and
masked, the sink logit of the head is APPENDED as one more column, the softmax runs over all columns, the sink's column is
dropped and the rest multiplies V.  Gradients — the sinks' included — come from torch.autograd in fp64.  It uses nothing the
kernels produce, and it does not use the identity the product is built on (lse' = logaddexp(lse, sink), out' = out
exp(lse - lse')): that identity is what the tests check against it.

`apply_formula` / `dsink_formula` evaluate the two formulas of include/rfa.h (rfa_sink_apply, rfa_sink_grad) on GIVEN tensors,
for the tests that run the two kernels alone on random inputs."""
import torch

import _blockref as R

# Tolerance of a computed dsink against dsink_formula(..., torch.float64) on the SAME stored inputs, as a fraction of the sum
# of |terms| the same call returns: 4 x the worst error of the plain fp32 torch evaluation dsink_formula(..., torch.float32)
# over the kernel-alone cases of tests/test_gpu_sinks.py (D 40 .. 256, the three (B, S, H), bf16 and fp16, dense and packed,
# rows with lse = +inf; kernel_inputs seeds 0, 1, 2), measured on the CPU: worst 9.16e-8 (tests/test_sinks_cpu.py measures it
# again, prints it and asserts that the fp32 evaluation itself is within DSINK_TOL).  Never taken from a kernel's output.
DSINK_FP32_WORST = 9.2e-8
DSINK_TOL = 4 * DSINK_FP32_WORST


def _one(q, k, v, sink, scale, causal, window, keep, rescale):
    """(out (lq, H, D), lse (H, lq)) of one sequence, fp64, differentiable.  sink: (H,) or None"""
    H, G = q.shape[1], q.shape[1] // k.shape[1]
    ke = k.permute(1, 0, 2).repeat_interleave(G, dim=0)
    ve = v.permute(1, 0, 2).repeat_interleave(G, dim=0)
    s = torch.matmul(q.permute(1, 0, 2), ke.transpose(1, 2)) * scale                     # (H, lq, lk)
    s = s.masked_fill(~R.visible(q.shape[0], k.shape[0], causal, window), float("-inf"))
    if sink is not None:
        s = torch.cat([s, sink.view(H, 1, 1).expand(H, q.shape[0], 1)], dim=-1)        # the sink column
    lse = torch.logsumexp(s, dim=-1) if s.shape[-1] else s.new_full(s.shape[:2], float("-inf"))
    empty = torch.isinf(lse)                                                           # (only without a sink)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(lse), lse).unsqueeze(-1))
    if sink is not None:
        p = p[..., :-1]                                                                # its value vector is zero
    if keep is not None:
        p = torch.where(keep, p * rescale, torch.zeros_like(p))
    out = torch.matmul(p, ve).permute(1, 0, 2)
    return out, torch.where(empty, torch.full_like(lse, float("inf")), lse)


def attention(q, k, v, sinks=None, *, scale=None, dout=None, causal=False, window=(-1, -1), cu_seqlens_q=None,
              cu_seqlens_k=None, keep=None, rescale=1.0):
    """(out, lse) or, with dout, (out, lse, dq, dk, dv, dsink) in fp64 (dsink None without sinks).  Dense q (B, Sq, H, D),
    k / v (B, Sk, Hk, D), lse (B, H, Sq); packed q (T, H, D) with cu_seqlens_*, lse (H, T).  keep: one bool (H, lq, lk) dropout
    mask per sequence (tests/_blockref.keep_mask) with its `rescale`; lse is that of the undropped scores."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    grad = dout is not None
    q, k, v = (t.detach().double().requires_grad_(grad) for t in (q, k, v))
    sk = None if sinks is None else sinks.detach().double().requires_grad_(grad)
    if cu_seqlens_q is None:
        idx = [(b, b) for b in range(q.shape[0])]
        join, join_lse = torch.stack, torch.stack
    else:
        cq, ck = [int(x) for x in cu_seqlens_q], [int(x) for x in cu_seqlens_k]
        idx = [(slice(cq[b], cq[b + 1]), slice(ck[b], ck[b + 1])) for b in range(len(cq) - 1)]
        join, join_lse = torch.cat, lambda ls: torch.cat(ls, dim=1)
    outs, lses = [], []
    for b, (iq, ik) in enumerate(idx):
        o, l = _one(q[iq], k[ik], v[ik], sk, scale, causal, window, None if keep is None else keep[b], rescale)
        outs.append(o)
        lses.append(l)
    out, lse = join(outs), join_lse(lses)
    if not grad:
        return out.detach(), lse.detach()
    out.backward(dout.double())
    return out.detach(), lse.detach(), q.grad, k.grad, v.grad, (None if sk is None else sk.grad)


def _rows_heads(lse):
    """lse (B, H, S) / (H, T) as (B, S, H) / (T, H): one value per (row, head), like out without its last dim"""
    return lse.transpose(-1, -2)


def apply_formula(out, lse, sinks, dtype=torch.float64):
    """(out', lse') of rfa_sink_apply on given tensors: lse' = logaddexp(lse, sink_h), out' = out * exp(lse - lse'); a row with
    an infinite lse (no visible key) gets lse' = sink_h and out' = 0"""
    o, l, s = out.to(dtype), _rows_heads(lse).to(dtype), sinks.to(dtype)
    s = s.expand_as(l)
    inf = torch.isinf(l)
    l0 = torch.where(inf, s, l)
    lnew = torch.where(inf, s, torch.logaddexp(l0, s))
    w = torch.where(inf, torch.zeros_like(l), torch.exp(l0 - lnew))
    return o * w.unsqueeze(-1), _rows_heads(lnew)


def dsink_formula(dout, out, lse, sinks, dtype=torch.float64):
    """(dsink (H,), sum of |terms| (H,)) of rfa_sink_grad on given tensors, evaluated in `dtype`:
    dsink_h = - sum over rows of exp(sink_h - lse') * rowsum(dout * out')"""
    l, s = _rows_heads(lse).to(dtype), sinks.to(dtype)
    dot = (dout.to(dtype) * out.to(dtype)).sum(-1)
    terms = torch.where(torch.isinf(l), torch.zeros_like(l), -torch.exp(s.expand_as(l) - l) * dot)
    terms = terms.reshape(-1, terms.shape[-1])
    return terms.sum(0), terms.abs().sum(0)


# ---- the inputs of the tests that run the two kernels alone (tests/test_gpu_sinks.py; the CPU measurement of DSINK_TOL) ----
KERNEL_D = (40, 64, 128, 136, 256)
KERNEL_BSH = ((1, 1, 1), (2, 17, 3), (1, 257, 5))              # rows x heads is no multiple of 16; 257 rows: two row chunks


def kernel_inputs(B, S, H, D, dtype, packed, seed=0):
    """(dout, out, lse, sinks) on the CPU: out ~ N(0, 1) in the io dtype, lse ~ N(3, 1) fp32, sinks 3 +- 2 fp32; every 7th row
    of head 0 has lse = +inf and an all-zero out (a row without a visible key); dout is a STRIDED view, the first D columns
    of a tensor 8 columns wider.  Dense: out (B, S, H, D), lse (B, H, S); packed: out (B S, H, D), lse (H, B S)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * D + S + H)
    lead = (B * S,) if packed else (B, S)
    out = torch.randn(*lead, H, D, generator=g).to(dtype)
    dout = torch.randn(*lead, H, D + 8, generator=g).to(dtype)[..., :D]
    lse = (3 + torch.randn(*lead, H, generator=g)).float()
    flat = lse.view(-1, H)
    flat[::7, 0] = float("inf")
    out.view(-1, H, D)[::7, 0] = 0
    sinks = (1 + 4 * torch.rand(H, generator=g)).float()
    return dout, out, lse.transpose(-1, -2).contiguous(), sinks
