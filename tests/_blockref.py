"""TEST INFRASTRUCTURE: the ONE fp64 block attention of tests/, written from include/rfa.h.  No test in here.

For one sequence's block — q (lq, H, D), k / v (lk, Hk, D), query row i, key j —

    s   = softmax_scale * q.k
    s'  = softcap * tanh(s / softcap)                                     (softcap = 0: s' = s), t = tanh(...)
    s'' = s' - slope[h] * | i + (lk - lq) + alibi_shift - j |             (slopes = None: s'' = s')
    visible iff  off - wl <= j - i <= off + wr,  off = lk - lq + shift    (each side only when set; causal: wr = 0)

the mask is applied to s'', then softmax: P = exp(s'' - lse).  lse is that of the undropped scores, +inf for a row without
a visible key (its out is 0).  A keep mask (dropout) zeroes elements of the P that enters P V and of dP and scales the rest
by `rescale`.  Backward, the kernels' formula from the rows' GLOBAL lse and delta: dS = P (dP - delta) (1 - t^2),
dQ = scale dS K, dK = scale dS^T Q, dV = (kept P)^T dO; the slopes get no gradient.  Nothing is rounded: inputs are upcast to
fp64 on their own device."""
import torch

from oracle import flash_attn_ref as O


def visible(lq, lk, causal, window=(-1, -1), shift=0, device=None):
    """(lq, lk) bool: True where the key is visible"""
    wl, wr = window if window is not None else (-1, -1)
    if causal:
        wr = 0
    d = torch.arange(lk, device=device).view(1, -1) - torch.arange(lq, device=device).view(-1, 1)      # j - i, int64
    off = lk - lq + int(shift)
    vis = torch.ones(lq, lk, dtype=torch.bool, device=device)
    if wr >= 0:
        vis &= d <= off + wr
    if wl >= 0:
        vis &= d >= off - wl
    return vis


def bias(lq, lk, shift, device=None):
    """| i + (lk - lq) + shift - j | as an (lq, lk) fp64 matrix"""
    i = torch.arange(lq, dtype=torch.float64, device=device).view(-1, 1) + (lk - lq) + shift
    j = torch.arange(lk, dtype=torch.float64, device=device).view(1, -1)
    return (i - j).abs()


def positions(offset, m, n):
    """global positions of local rows 0 .. n-1 under the dropout position map m = (stride, split, offset2) behind `offset`"""
    stride, split, off2 = m
    stride = stride or 1
    return [offset + i * stride if (split == 0 or i < split) else off2 + (i - split) * stride for i in range(n)]


def keep_mask(dropout, b, H, lq, lk):
    """bool (H, lq, lk): the keep mask of batch entry b of a block call with the 5- or 7-tuple `dropout`; its rescale is
    oracle.flash_attn_ref.drop_rescale(dropout[0])"""
    p, seed, q0, k0, h0 = dropout[:5]
    qm, km = dropout[5:7] if len(dropout) > 5 else ((1, 0, 0), (1, 0, 0))
    return O.dropout_keep(seed, p, b, range(h0, h0 + H), positions(q0, qm, lq), positions(k0, km, lk))


def _expand(x, G):
    return x.double().permute(1, 0, 2).repeat_interleave(G, dim=0)           # (H, L, D)


def _scores(q, k, scale, slopes, alibi_shift, softcap):
    """(s'', 1 - t^2 or None) of one sequence, unmasked, (H, lq, lk) fp64"""
    s = torch.matmul(q.double().permute(1, 0, 2), _expand(k, q.shape[1] // k.shape[1]).transpose(1, 2)) * scale
    dt = None
    if softcap:
        t = torch.tanh(s / softcap)
        s, dt = softcap * t, 1.0 - t * t
    if slopes is not None:
        s = s - slopes.double().to(q.device).view(-1, 1, 1) * bias(q.shape[0], k.shape[0], alibi_shift, q.device)
    return s, dt


def block_forward(q, k, v, scale, *, causal=False, window=(-1, -1), shift=0, slopes=None, alibi_shift=0, softcap=0.0,
                  keep=None, rescale=1.0):
    """(out (lq, H, D), lse (H, lq)) fp64 of one sequence's block; lse = +inf, out = 0 for rows without a visible key"""
    s, _ = _scores(q, k, scale, slopes, alibi_shift, softcap)
    s = s.masked_fill(~visible(q.shape[0], k.shape[0], causal, window, shift, q.device), float("-inf"))
    l = torch.logsumexp(s, dim=-1) if k.shape[0] else s.new_full(s.shape[:2], float("-inf"))       # (H, lq)
    empty = torch.isinf(l)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
    if keep is not None:
        p = torch.where(keep.to(q.device), p * rescale, torch.zeros_like(p))
    o = torch.matmul(p, _expand(v, q.shape[1] // k.shape[1])).permute(1, 0, 2)
    return o, torch.where(empty, torch.full_like(l, float("inf")), l)


def block_backward(dout, q, k, v, lse, delta, scale, *, causal=False, window=(-1, -1), shift=0, slopes=None, alibi_shift=0,
                   softcap=0.0, keep=None, rescale=1.0):
    """(dq, dk, dv) fp64 of ONE sequence's block from the rows' GLOBAL lse and delta, both (H, lq): the kernels' formula"""
    Hk, G = k.shape[1], q.shape[1] // k.shape[1]
    lk, D = k.shape[0], k.shape[2]
    qd, dod = q.double().permute(1, 0, 2), dout.double().permute(1, 0, 2)
    ke, ve = _expand(k, G), _expand(v, G)
    s, dt = _scores(q, k, scale, slopes, alibi_shift, softcap)
    l = lse.double()
    p = torch.exp(s - torch.where(torch.isinf(l), torch.zeros_like(l), l).unsqueeze(-1))
    p = torch.where(visible(q.shape[0], lk, causal, window, shift, q.device), p, torch.zeros_like(p))
    dp = torch.matmul(dod, ve.transpose(1, 2))
    pd = p
    if keep is not None:
        keep = keep.to(q.device)
        dp = torch.where(keep, dp * rescale, torch.zeros_like(dp))
        pd = torch.where(keep, p * rescale, torch.zeros_like(p))
    ds = p * (dp - delta.double().unsqueeze(-1))
    if dt is not None:
        ds = ds * dt
    ds = ds * scale
    dq = torch.matmul(ds, ke).permute(1, 0, 2)
    dk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    dv = torch.matmul(pd.transpose(1, 2), dod).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
    return dq, dk, dv


def attention(q, k, v, *, scale=None, dout=None, autograd=False, cu_seqlens_q=None, cu_seqlens_k=None, shift=0, shift_lens=0,
              slopes=None, keep=None, **kw):
    """(out, lse) or, with dout, (out, lse, dq, dk, dv) — fp64, the block taken as the WHOLE attention (block-local lse and
    delta = rowsum(dout * out): what a call with plain outputs computes).  Dense q (B, Sq, H, D), k / v (B, Sk, Hk, D), lse
    (B, H, Sq); packed q (T, H, D) with cu_seqlens_q / cu_seqlens_k, lse (H, T).  shift_lens: a shift in units of each
    sequence's own key length; slopes: (H,) or (B, H); keep: one mask per sequence; **kw: block_forward's other keywords.
    autograd: the gradients come from torch.autograd through block_forward instead of from block_backward."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    if autograd:
        q, k, v = (t.detach().double().requires_grad_(dout is not None) for t in (q, k, v))
    if cu_seqlens_q is None:
        idx = [((b,), (b,)) for b in range(q.shape[0])]
        join, join_lse = torch.stack, torch.stack
    else:
        cq, ck = [int(x) for x in cu_seqlens_q], [int(x) for x in cu_seqlens_k]
        idx = [((slice(cq[b], cq[b + 1]),), (slice(ck[b], ck[b + 1]),)) for b in range(len(cq) - 1)]
        join, join_lse = torch.cat, lambda ls: torch.cat(ls, dim=1)
    outs, lses, grads = [], [], []
    for b, (iq, ik) in enumerate(idx):
        kw_b = dict(kw, shift=shift + shift_lens * k[ik].shape[0], keep=None if keep is None else keep[b],
                    slopes=slopes if slopes is None or slopes.dim() == 1 else slopes[b])
        o, l = block_forward(q[iq], k[ik], v[ik], scale, **kw_b)
        outs.append(o)
        lses.append(l)
        if dout is not None and not autograd:
            delta = (dout[iq].double() * o).sum(-1).transpose(0, 1)
            grads.append(block_backward(dout[iq], q[iq], k[ik], v[ik], l, delta, scale, **kw_b))
    out, lse = join(outs), join_lse(lses)
    if dout is None:
        return out.detach(), lse.detach()
    if autograd:
        out.backward(dout.double())
        return out.detach(), lse.detach(), q.grad, k.grad, v.grad
    return (out, lse, *(join([g[i] for g in grads]) for i in range(3)))
