"""TEST INFRASTRUCTURE: the CPU test backend (tests/_rowrange_backend.py on tests/_lsegrad_backend.py on tests/_ref_backend.py)
with `serves_block_mask` — fwd / bwd take `block_mask=(mask_view, k_blk0)` (include/rfa.h: rfa_blockmask_args).  A block call
without a mask is the parent class's, untouched.  One with a mask gets every sequence's block in fp64 with the explicit boolean
mask

    visible(h, i, j) = band(i, j)  and  mask[b or 0, h or 0, i // 128, k_blk0 + j // 128]   (columns outside the mask: dark)

through the parent's ranged path (same forward, backward and accumulate delivery), whose `_vis` is the one thing replaced.

`Recording` notes the `block_mask` every block call carried; `expand` turns a (Bm, Hm, NQ, NK) block mask into the (B, H, T, T)
element mask; `single_device` is the ONE fp64 autograd attention with a (B, H, T, T) mask the schedule tests compare with."""
import torch

import _blockref as R
from _rowrange_backend import RowRangeBackend

BLOCK = 128


class _Masked:
    """a block mask travelling through the parent's `row_ranges=` plumbing"""

    def __init__(self, mask, k_blk0):
        self.mask, self.k_blk0 = mask, int(k_blk0)


class BlockMaskBackend(RowRangeBackend):
    serves_block_mask = True

    def __init__(self, serves=("mask_shift", "mask_shift_lens")):
        super().__init__(serves)
        self.name += "+block_mask"

    def _vis(self, seq, q, k, causal, window, dropout, row_ranges, mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0):
        if not isinstance(row_ranges, _Masked):
            return super()._vis(seq, q, k, causal, window, dropout, row_ranges, mask_shift, mask_shift_lens, alibi, softcap)
        assert alibi is None and not softcap and (dropout is None or not dropout[0] > 0), \
            "a bias, a cap or dropout with a block mask: the public entry must refuse it before a block call"
        _, b, qs, _ks = seq
        assert b is not None and qs == 0, "a block mask with packed input"
        lq, lk, H = q.shape[0], k.shape[0], q.shape[1]
        m = row_ranges.mask
        assert m.dtype in (torch.bool, torch.uint8) and m.dim() == 4 and m.shape[2] == -(-lq // BLOCK), \
            f"the mask view {tuple(m.shape)} must hold the call's {-(-lq // BLOCK)} query blocks"
        assert m.shape[1] in (1, H), "one mask for all query heads, or one per QUERY head"
        mb = m[b if m.shape[0] > 1 else 0].bool()                                 # (Hm, nq, NK)
        col = row_ranges.k_blk0 + torch.arange(lk) // BLOCK
        ok = (col >= 0) & (col < m.shape[3])
        rows = torch.arange(lq) // BLOCK
        vis = mb[:, rows][:, :, col.clamp(0, m.shape[3] - 1)] & ok.view(1, 1, -1)
        return vis & R.visible(lq, lk, causal, window, mask_shift + mask_shift_lens * lk).unsqueeze(0)

    @staticmethod
    def _kw(block_mask, row_ranges):
        if block_mask is None:
            return {} if row_ranges is None else {"row_ranges": row_ranges}
        assert row_ranges is None, "a block mask together with row ranges"
        return {"row_ranges": _Masked(*block_mask)}

    def fwd(self, q, k, v, *, block_mask=None, row_ranges=None, **kw):
        return super().fwd(q, k, v, **self._kw(block_mask, row_ranges), **kw)

    def bwd(self, dout, q, k, v, lse, delta, *, block_mask=None, row_ranges=None, **kw):
        return super().bwd(dout, q, k, v, lse, delta, **self._kw(block_mask, row_ranges), **kw)


class Recording:
    """any backend, with a note per fwd / bwd block call: the k_blk0, the mask view's shape and strides, its first row of bytes'
    data pointer offset from the bound mask, and the call's (B, Sq) (None: no mask)"""

    def __init__(self, inner):
        self.inner = inner
        self.seen = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    @staticmethod
    def _note(q, kw):
        bm = kw.get("block_mask")
        if bm is None:
            return None
        m = bm[0]
        return (int(bm[1]), tuple(m.shape), m.storage_offset(), tuple(q.shape[:2]))

    def fwd(self, q, k, v, **kw):
        self.seen["fwd"].append(self._note(q, kw))
        return self.inner.fwd(q, k, v, **kw)

    def bwd(self, dout, q, k, v, *a, **kw):
        self.seen["bwd"].append(self._note(q, kw))
        return self.inner.bwd(dout, q, k, v, *a, **kw)


def expand(block_mask, B, H, Tq, Tk, causal=False, window=(-1, -1), k_blk0=0, shift=0):
    """(B, H, Tq, Tk) bool of a call: block_mask (Bm, Hm, ceil(Tq / 128), NK), key 0 in column k_blk0, intersected with the call's
    own band (tests/_blockref.visible: bottom-right aligned, moved by `shift`)"""
    m = block_mask.bool().cpu()
    col = k_blk0 + torch.arange(Tk) // BLOCK
    ok = (col >= 0) & (col < m.shape[3])
    e = m[:, :, torch.arange(Tq) // BLOCK][:, :, :, col.clamp(0, m.shape[3] - 1)] & ok.view(1, 1, 1, -1)
    return e.expand(B, H, Tq, Tk) & R.visible(Tq, Tk, causal, tuple(window), shift).view(1, 1, Tq, Tk)


def single_device(q, k, v, do, mask, dlse=None):
    """(out, lse, dq, dk, dv) fp64 of ONE single-device attention with the explicit (B, H, T, T) boolean mask — H: query heads —,
    gradients by autograd of <out, do> (+ <lse, dlse> over the rows that see a key); lse = +inf and out = 0 for a row that sees
    none"""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k.repeat_interleave(G, dim=2)) * q.shape[-1] ** -0.5
    s = s.masked_fill(~mask, float("-inf"))
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
