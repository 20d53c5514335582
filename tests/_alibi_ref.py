"""TEST INFRASTRUCTURE: fp64 attention with an ALiBi bias, written from the definition in include/rfa.h.

For batch (or packed sequence) b, head h, query row i and key j of a block call

    score = softmax_scale * q.k  -  slope[b, h] * | i + (len_k - len_q) + alibi_shift - j |

added before masking and softmax; causal: j <= i + (len_k - len_q) + mask_shift.  Nothing is rounded: inputs are upcast
to fp64, `attention` returns out / lse (and, with `dout`, dq / dk / dv by autograd) in fp64.  lse is the log-sum-exp of
the biased scores, +inf for a row without a visible key (its out is 0).  Dense q (B, Sq, H, D), k / v (B, Sk, Hk, D), lse
(B, H, Sq); packed q (T, H, D) with cu_seqlens_q / cu_seqlens_k, lse (H, T).  slopes: (H,) or (B, H), any float dtype."""
import torch


def bias(lq, lk, shift):
    """| i + (lk - lq) + shift - j | as an (lq, lk) fp64 matrix"""
    i = torch.arange(lq, dtype=torch.float64).view(-1, 1) + (lk - lq) + shift
    j = torch.arange(lk, dtype=torch.float64).view(1, -1)
    return (i - j).abs()


def visible(lq, lk, causal, mask_shift=0):
    if not causal:
        return torch.ones(lq, lk, dtype=torch.bool)
    i = torch.arange(lq).view(-1, 1) + (lk - lq) + mask_shift
    j = torch.arange(lk).view(1, -1)
    return j <= i


def scores(q, k, slopes, scale, causal, shift=0, mask_shift=0):
    """masked, biased scores (H, lq, lk) fp64 of one sequence: q (lq, H, D), k (lk, Hk, D), slopes (H,)"""
    H, G = q.shape[1], q.shape[1] // k.shape[1]
    ke = k.permute(1, 0, 2).repeat_interleave(G, dim=0)
    s = torch.matmul(q.permute(1, 0, 2), ke.transpose(1, 2)) * scale
    s = s - slopes.double().view(H, 1, 1) * bias(q.shape[0], k.shape[0], shift)
    return s.masked_fill(~visible(q.shape[0], k.shape[0], causal, mask_shift), float("-inf"))


def _one(q, k, v, slopes, scale, causal, shift, mask_shift):
    G = q.shape[1] // k.shape[1]
    s = scores(q, k, slopes, scale, causal, shift, mask_shift)
    l = torch.logsumexp(s, dim=-1)                                       # (H, lq); -inf: no visible key
    empty = torch.isinf(l)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
    o = torch.matmul(p, v.permute(1, 0, 2).repeat_interleave(G, dim=0)).permute(1, 0, 2)
    return o, torch.where(empty, torch.full_like(l, float("inf")), l)


def _slopes_of(slopes, b):
    return slopes if slopes.dim() == 1 else slopes[b]


def attention(q, k, v, slopes, *, scale=None, causal=False, shift=0, mask_shift=0, dout=None, cu_seqlens_q=None,
              cu_seqlens_k=None):
    """(out, lse) or, with dout, (out, lse, dq, dk, dv) — fp64.  slopes = None: the unbiased attention."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    qd, kd, vd = (t.detach().double().requires_grad_(dout is not None) for t in (q, k, v))
    if slopes is None:
        slopes = torch.zeros(q.shape[-2], dtype=torch.float64)
    if cu_seqlens_q is None:
        res = [_one(qd[b], kd[b], vd[b], _slopes_of(slopes, b), scale, causal, shift, mask_shift) for b in range(q.shape[0])]
        out, lse = torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])
    else:
        cq, ck = [int(x) for x in cu_seqlens_q], [int(x) for x in cu_seqlens_k]
        res = [_one(qd[cq[b]:cq[b + 1]], kd[ck[b]:ck[b + 1]], vd[ck[b]:ck[b + 1]], _slopes_of(slopes, b), scale, causal,
                    shift, mask_shift) for b in range(len(cq) - 1)]
        out, lse = torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res], dim=1)
    if dout is None:
        return out.detach(), lse.detach()
    out.backward(dout.double())
    return out.detach(), lse.detach(), qd.grad, kd.grad, vd.grad


def block_backward(dout, q, k, v, lse, delta, slopes, scale, causal, shift=0, mask_shift=0):
    """(dq, dk, dv) fp64 of ONE sequence's block from the rows' GLOBAL lse and delta (the kernels' formula): P is
    recomputed from the biased scores, dS = P (dP - delta), the slopes get no gradient.  lse / delta: (H, lq)."""
    Hk, G = k.shape[1], q.shape[1] // k.shape[1]
    qd, dod = q.double().permute(1, 0, 2), dout.double().permute(1, 0, 2)
    ke = k.double().permute(1, 0, 2).repeat_interleave(G, dim=0)
    ve = v.double().permute(1, 0, 2).repeat_interleave(G, dim=0)
    s = scores(q.double(), k.double(), slopes, scale, causal, shift, mask_shift)
    l = lse.double()
    p = torch.exp(s - torch.where(torch.isinf(l), torch.zeros_like(l), l).unsqueeze(-1))      # masked: exp(-inf) = 0
    dp = torch.matmul(dod, ve.transpose(1, 2))
    ds = p * (dp - delta.double().unsqueeze(-1)) * scale
    lk, D = k.shape[0], k.shape[2]
    dq = torch.matmul(ds, ke).permute(1, 0, 2)
    dk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    dv = torch.matmul(p.transpose(1, 2), dod).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    return dq, dk, dv
