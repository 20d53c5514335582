"""TEST INFRASTRUCTURE: fp64 attention with logit soft-capping, a band and a shift, written from include/rfa.h.

For one sequence's block, query row i and key j:

    s' = softcap * tanh(softmax_scale * q.k / softcap)                 (softcap = 0: s' = softmax_scale * q.k)
    visible iff  off - wl <= j - i <= off + wr,  off = len_k - len_q + mask_shift      (each side only when set; causal: wr = 0)

the mask is applied to s', then softmax.  lse is the log-sum-exp of s' (+inf for a row without a visible key, whose out is
0).  Backward with t = tanh(...): P = exp(s' - lse), dS = P (dP - delta) (1 - t^2), dQ = scale dS K, dK = scale dS^T Q,
dV = P^T dO.  Nothing is rounded: inputs are upcast to fp64.  Dense q (B, Sq, H, D), k / v (B, Sk, Hk, D), lse (B, H, Sq);
packed q (T, H, D) with cu_seqlens_q / cu_seqlens_k, lse (H, T); mask_shift_lens: the shift in units of each sequence's own
key length."""
import torch


def visible(lq, lk, causal, window=(-1, -1), shift=0):
    wl, wr = window if window is not None else (-1, -1)
    if causal:
        wr = 0
    d = torch.arange(lk).view(1, -1) - torch.arange(lq).view(-1, 1)
    off = lk - lq + int(shift)
    vis = torch.ones(lq, lk, dtype=torch.bool)
    if wr >= 0:
        vis &= d <= off + wr
    if wl >= 0:
        vis &= d >= off - wl
    return vis


def _expand(x, G):
    return x.double().permute(1, 0, 2).repeat_interleave(G, dim=0)           # (H, L, D)


def capped_scores(q, k, scale, softcap):
    """(s', 1 - t^2) of one sequence, unmasked, (H, lq, lk) fp64: q (lq, H, D), k (lk, Hk, D)"""
    G = q.shape[1] // k.shape[1]
    s = torch.matmul(q.double().permute(1, 0, 2), _expand(k, G).transpose(1, 2)) * scale
    if not softcap:
        return s, torch.ones_like(s)
    t = torch.tanh(s / softcap)
    return softcap * t, 1.0 - t * t


def block_forward(q, k, v, scale, softcap, causal, window=(-1, -1), shift=0):
    """(out (lq, H, D), lse (H, lq)) fp64 of one sequence's block; lse = +inf, out = 0 for rows without a visible key"""
    G = q.shape[1] // k.shape[1]
    s, _ = capped_scores(q, k, scale, softcap)
    s = s.masked_fill(~visible(q.shape[0], k.shape[0], causal, window, shift), float("-inf"))
    l = torch.logsumexp(s, dim=-1)
    empty = torch.isinf(l)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
    o = torch.matmul(p, _expand(v, G)).permute(1, 0, 2)
    return o, torch.where(empty, torch.full_like(l, float("inf")), l)


def block_backward(dout, q, k, v, lse, delta, scale, softcap, causal, window=(-1, -1), shift=0):
    """(dq, dk, dv) fp64 of ONE sequence's block from the rows' GLOBAL lse and delta, both (H, lq): the kernels' formula"""
    Hk, G = k.shape[1], q.shape[1] // k.shape[1]
    lk, D = k.shape[0], k.shape[2]
    qd, dod = q.double().permute(1, 0, 2), dout.double().permute(1, 0, 2)
    ke, ve = _expand(k, G), _expand(v, G)
    s, dt = capped_scores(q, k, scale, softcap)
    vis = visible(q.shape[0], lk, causal, window, shift)
    l = lse.double()
    p = torch.exp(s - torch.where(torch.isinf(l), torch.zeros_like(l), l).unsqueeze(-1))
    p = torch.where(vis, p, torch.zeros_like(p))
    dp = torch.matmul(dod, ve.transpose(1, 2))
    ds = p * (dp - delta.double().unsqueeze(-1)) * dt * scale
    dq = torch.matmul(ds, ke).permute(1, 0, 2)
    dk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    dv = torch.matmul(p.transpose(1, 2), dod).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    return dq, dk, dv


def _seqs(q, k, cu_q, cu_k):
    if cu_q is None:
        return [((b, slice(None)), (b, slice(None))) for b in range(q.shape[0])]
    cq, ck = [int(x) for x in cu_q], [int(x) for x in cu_k]
    return [((slice(cq[b], cq[b + 1]),), (slice(ck[b], ck[b + 1]),)) for b in range(len(cq) - 1)]


def attention(q, k, v, softcap, *, scale=None, causal=False, window=(-1, -1), shift=0, shift_lens=0, dout=None,
              cu_seqlens_q=None, cu_seqlens_k=None):
    """(out, lse) or, with dout, (out, lse, dq, dk, dv) — fp64, the block taken as the WHOLE attention (block-local lse and
    delta: what a call with plain outputs computes)"""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    outs, lses, grads = [], [], []
    for iq, ik in _seqs(q, k, cu_seqlens_q, cu_seqlens_k):
        qs, ks, vs = q[iq], k[ik], v[ik]
        sh = shift + shift_lens * ks.shape[0]
        o, l = block_forward(qs, ks, vs, scale, softcap, causal, window, sh)
        outs.append(o)
        lses.append(l)
        if dout is not None:
            delta = (dout[iq].double() * o).sum(-1).transpose(0, 1)
            grads.append(block_backward(dout[iq], qs, ks, vs, l, delta, scale, softcap, causal, window, sh))
    if cu_seqlens_q is None:
        out, lse = torch.stack(outs), torch.stack(lses)
        gr = [torch.stack([g[i] for g in grads]) for i in range(3)] if grads else []
    else:
        out, lse = torch.cat(outs), torch.cat(lses, dim=1)
        gr = [torch.cat([g[i] for g in grads]) for i in range(3)] if grads else []
    return (out, lse, *gr)
