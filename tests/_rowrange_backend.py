"""TEST INFRASTRUCTURE: the CPU test backend (tests/_lsegrad_backend.py: the gradient of lse and the pairwise merge on top of
tests/_ref_backend.py) with `serves_row_ranges` — fwd / bwd take `row_ranges=(start, end, k_pos0)` (include/rfa.h:
rfa_rowrange_args).  A block call without ranges is the parent class's, untouched.  One with ranges gets every sequence's block
in fp64 with the explicit boolean mask

    visible(i, j) = band(i, j)  and  start[b, i] <= k_pos0 + j < end[b, i]          (band: tests/_blockref.visible)

forward: softmax over the visible keys (lse = +inf, out = 0 for a row without one); backward: the kernels' formula from the
rows' GLOBAL lse and delta — P = exp(s - lse) where visible, dS = P (dP - delta), dQ = scale dS K, dK = scale dS^T Q,
dV = P^T dO — with the oracle's delivery and rounding points around it.

`Recording` notes the `row_ranges` every block call carried; `mask_of` builds the (B, T, T) boolean mask of a whole call from
GLOBAL (start, end); `single_device` is the ONE fp64 autograd attention with that mask the schedule tests compare with."""
import torch

import _blockref as R
from _lsegrad_backend import LseGradBackend


def _expand(x, G):
    return x.double().permute(1, 0, 2).repeat_interleave(G, dim=0)           # (H, L, D)


class RowRangeBackend(LseGradBackend):
    serves_row_ranges = True

    def __init__(self, serves=("mask_shift", "mask_shift_lens")):
        super().__init__(serves)
        self.name += "+row_ranges"

    def _vis(self, seq, q, k, causal, window, dropout, row_ranges, mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0):
        assert alibi is None and not softcap and (dropout is None or not dropout[0] > 0), \
            "a bias, a cap or dropout with row ranges: the public entry must refuse it before a block call"
        start, end, k_pos0 = row_ranges
        _, b, qs, _ks = seq
        assert b is not None, "row ranges with packed input"
        lq, lk = q.shape[0], k.shape[0]
        assert start.dtype == torch.int32 and end.dtype == torch.int32 and start.shape == end.shape and start.stride(-1) in (0, 1)
        s, e = start[b, qs:qs + lq].long().view(-1, 1), end[b, qs:qs + lq].long().view(-1, 1)
        assert s.shape[0] == lq, "the ranges must cover the call's query rows"
        pos = (int(k_pos0) + torch.arange(lk)).view(1, -1)
        return R.visible(lq, lk, causal, window, mask_shift + mask_shift_lens * lk) & (pos >= s) & (pos < e)

    def fwd(self, q, k, v, *, row_ranges=None, out_acc=None, lse_acc=None, acc_init=False, **kw):
        """a ranged call that merges into (out_acc, lse_acc) delivers here: with ranges a row may see nothing in the block
        that initialises the accumulators (lse_acc = -inf) and something in a later one, which the oracle's sigmoid form of the
        merge — written for rows that always see their diagonal block — turns into -inf - (-inf).  The kernels' form
        (csrc/rfa_fwd.hip: weights exp(x - logaddexp)) has no such case; out is rounded to the io dtype before it is merged, as
        the oracle does."""
        if row_ranges is None or out_acc is None:
            extra = {} if row_ranges is None else {"row_ranges": row_ranges}
            return super().fwd(q, k, v, out_acc=out_acc, lse_acc=lse_acc, acc_init=acc_init, **extra, **kw)
        assert kw.get("cu_seqlens_q") is None and not kw.get("q_half") and not kw.get("k_half"), "row ranges: dense input"
        self._check(kw)
        ext = {n: kw[n] for n in ("mask_shift", "mask_shift_lens", "alibi", "softcap") if n in kw}
        for b in range(q.shape[0]):
            o, l = self._fwd_block((b, b, 0, 0), q[b], k[b], v[b], kw["softmax_scale"], kw["causal"], kw.get("window", (-1, -1)),
                                   kw.get("dropout"), row_ranges=row_ranges, **ext)
            o = o.to(q.dtype).float()
            has = torch.isfinite(l)
            l = torch.where(has, l, torch.full_like(l, float("-inf")))
            if acc_init:
                out_acc[b].copy_(o)
                lse_acc[b].copy_(l)
                continue
            la = lse_acc[b]
            new_l = torch.logaddexp(la, l)
            safe = torch.where(torch.isfinite(new_l), new_l, torch.zeros_like(new_l))
            wo, wn = torch.exp(la - safe).transpose(0, 1).unsqueeze(-1), torch.exp(l - safe).transpose(0, 1).unsqueeze(-1)
            out_acc[b].copy_(torch.where(has.transpose(0, 1).unsqueeze(-1), wo * out_acc[b] + wn * o, out_acc[b]))
            lse_acc[b].copy_(torch.where(has, new_l, la))

    def _fwd_block(self, seq, q, k, v, scale, causal, window, dropout, row_ranges=None, **ext):
        if row_ranges is None:
            return super()._fwd_block(seq, q, k, v, scale, causal, window, dropout, **ext)
        vis = self._vis(seq, q, k, causal, window, dropout, row_ranges, **ext)
        G = q.shape[1] // k.shape[1]
        s = torch.matmul(q.double().permute(1, 0, 2), _expand(k, G).transpose(1, 2)) * scale
        s = s.masked_fill(~vis, float("-inf"))
        l = torch.logsumexp(s, dim=-1) if k.shape[0] else s.new_full(s.shape[:2], float("-inf"))
        empty = torch.isinf(l)
        p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
        o = torch.matmul(p, _expand(v, G)).permute(1, 0, 2)
        return o, torch.where(empty, torch.full_like(l, float("inf")), l).float()

    def _bwd_block(self, seq, dout, q, k, v, lse, delta, scale, causal, window, dropout, row_ranges=None, **ext):
        if row_ranges is None:
            return super()._bwd_block(seq, dout, q, k, v, lse, delta, scale, causal, window, dropout, **ext)
        vis = self._vis(seq, q, k, causal, window, dropout, row_ranges, **ext)
        Hk, G = k.shape[1], q.shape[1] // k.shape[1]
        lk, D = k.shape[0], k.shape[2]
        qd, dod = q.double().permute(1, 0, 2), dout.double().permute(1, 0, 2)
        ke, ve = _expand(k, G), _expand(v, G)
        s = torch.matmul(qd, ke.transpose(1, 2)) * scale
        l = lse.double()
        p = torch.exp(s - torch.where(torch.isinf(l), torch.zeros_like(l), l).unsqueeze(-1))
        p = torch.where(vis, p, torch.zeros_like(p))
        ds = p * (torch.matmul(dod, ve.transpose(1, 2)) - delta.double().unsqueeze(-1)) * scale
        dq = torch.matmul(ds, ke).permute(1, 0, 2)
        dk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
        dv = torch.matmul(p.transpose(1, 2), dod).view(Hk, G, lk, D).sum(1).permute(1, 0, 2)
        return dq, dk, dv


class Recording:
    """any backend, with a note per fwd / bwd block call: the k_pos0 and the ranges' shape it carried (None: no ranges)"""

    def __init__(self, inner):
        self.inner = inner
        self.seen = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    @staticmethod
    def _note(q, kw):
        rr = kw.get("row_ranges")
        return None if rr is None else (int(rr[2]), tuple(rr[0].shape), tuple(q.shape[:2]))

    def fwd(self, q, k, v, **kw):
        self.seen["fwd"].append(self._note(q, kw))
        return self.inner.fwd(q, k, v, **kw)

    def bwd(self, dout, q, k, v, *a, **kw):
        self.seen["bwd"].append(self._note(q, kw))
        return self.inner.bwd(dout, q, k, v, *a, **kw)


def mask_of(start, end, causal, window=(-1, -1)):
    """(B, T, T) bool of a whole call on the unsharded sequence: GLOBAL (start, end) — (B, T), or None for the call without
    ranges — intersected with the call's own mask"""
    T = start.shape[1] if start is not None else None
    band = R.visible(T, T, causal, tuple(window))
    j = torch.arange(T).view(1, 1, -1)
    return band.unsqueeze(0) & (j >= start.long().unsqueeze(-1)) & (j < end.long().unsqueeze(-1))


def block_mask(start, end, k_pos0, lk, causal, window=(-1, -1), shift=0):
    """(B, lq, lk) bool of ONE block call: (start, end) — (B, lq) — against the keys k_pos0 .. k_pos0 + lk - 1, intersected with
    the block's band (tests/_blockref.visible: bottom-right aligned, moved by `shift`)"""
    lq = start.shape[1]
    pos = (int(k_pos0) + torch.arange(lk)).view(1, 1, -1)
    return (R.visible(lq, lk, causal, tuple(window), shift).unsqueeze(0) & (pos >= start.long().cpu().unsqueeze(-1))
            & (pos < end.long().cpu().unsqueeze(-1)))


def single_device(q, k, v, do, mask, dlse=None):
    """(out, lse, dq, dk, dv) fp64 of ONE single-device attention with the explicit (B, T, T) boolean mask, gradients by
    autograd of <out, do> (+ <lse, dlse> over the rows that see a key); lse = +inf and out = 0 for a row that sees none"""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k.repeat_interleave(G, dim=2)) * q.shape[-1] ** -0.5
    s = s.masked_fill(~mask.unsqueeze(1), float("-inf"))
    l = torch.logsumexp(s, dim=-1)
    empty = torch.isinf(l)
    ls = torch.where(empty, torch.zeros_like(l), l)
    p = torch.exp(s - ls.unsqueeze(-1))
    out = torch.einsum("bhqk,bkhd->bqhd", p, v.repeat_interleave(G, dim=2))
    loss = (out * do.double()).sum()
    if dlse is not None:
        loss = loss + (ls * dlse.double()).sum()
    loss.backward()
    return out.detach(), torch.where(empty, torch.full_like(l, float("inf")), l).detach(), q.grad, k.grad, v.grad
