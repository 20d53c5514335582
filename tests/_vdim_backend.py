"""TEST INFRASTRUCTURE: the CPU test backend (tests/_ref_backend.py) with `serves_vdim` — a `v` whose head dim differs from
q's.  A block call with equal widths is RefBackend's, untouched.  One with differing widths gets every sequence's block from
tests/_blockref.py under fp64 autograd (block_backward reshapes dV with K's width and is not used):

    forward    block_forward(q, k, v)
    backward   the kernels' formula from the rows' GLOBAL lse and delta, as the gradient of
                   < dout, P v > - < delta, rowsum(P) >,      P = exp(s'' - lse) where visible (lse a constant),
               whose derivative in s'' is P (dP - delta) and in v is P^T dout.

`Recording` notes which block calls carried differing widths; `single_device` is the ONE fp64 autograd attention on unsharded
tensors the schedule tests compare with."""
import torch

import _blockref as R
from _ref_backend import RefBackend


class VdimBackend(RefBackend):
    serves_vdim = True

    def __init__(self, serves=("mask_shift", "mask_shift_lens")):
        super().__init__(serves)
        self.name += "+vdim"

    def _vd_kw(self, k, causal, window, dropout, mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0):
        assert alibi is None and not softcap and (dropout is None or not dropout[0] > 0), \
            "a bias, a cap or dropout with a value head dim of its own: the schedules must refuse it before a block call"
        return dict(causal=causal, window=window, shift=mask_shift + mask_shift_lens * k.shape[0])

    def _fwd_block(self, seq, q, k, v, scale, causal, window, dropout, **ext):
        if v.shape[-1] == q.shape[-1]:
            return super()._fwd_block(seq, q, k, v, scale, causal, window, dropout, **ext)
        o, l = R.block_forward(q, k, v, scale, **self._vd_kw(k, causal, window, dropout, **ext))
        return o, l.float()

    def _bwd_block(self, seq, dout, q, k, v, lse, delta, scale, causal, window, dropout, **ext):
        if v.shape[-1] == q.shape[-1]:
            return super()._bwd_block(seq, dout, q, k, v, lse, delta, scale, causal, window, dropout, **ext)
        kw = self._vd_kw(k, causal, window, dropout, **ext)
        G = q.shape[1] // k.shape[1]
        with torch.enable_grad():
            qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
            s = torch.matmul(qd.permute(1, 0, 2), kd.permute(1, 0, 2).repeat_interleave(G, dim=0).transpose(1, 2)) * scale
            l = lse.double()
            p = torch.exp(s - torch.where(torch.isinf(l), torch.zeros_like(l), l).unsqueeze(-1))
            p = torch.where(R.visible(q.shape[0], k.shape[0], kw["causal"], kw["window"], kw["shift"]), p, torch.zeros_like(p))
            o = torch.matmul(p, vd.permute(1, 0, 2).repeat_interleave(G, dim=0)).permute(1, 0, 2)       # (lq, H, Dv)
            loss = (dout.double() * o).sum() - (delta.double() * p.sum(-1)).sum()
            return torch.autograd.grad(loss, (qd, kd, vd))


class Recording:
    """any backend, with a note per fwd / bwd block call: did v's head dim differ from q's"""

    def __init__(self, inner):
        self.inner = inner
        self.seen = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def fwd(self, q, k, v, **kw):
        self.seen["fwd"].append(v.shape[-1] != q.shape[-1])
        return self.inner.fwd(q, k, v, **kw)

    def bwd(self, dout, q, k, v, *a, **kw):
        self.seen["bwd"].append(v.shape[-1] != q.shape[-1])
        return self.inner.bwd(dout, q, k, v, *a, **kw)


def single_device(q, k, v, do, causal, window=(-1, -1), cu_seqlens=None):
    """(out, lse, dq, dk, dv) fp64: one single-device attention on the unsharded tensors, gradients by autograd"""
    kw = dict(causal=causal, window=tuple(window), dout=do, autograd=True)
    if cu_seqlens is not None:
        kw.update(cu_seqlens_q=list(cu_seqlens), cu_seqlens_k=list(cu_seqlens))
    return R.attention(q, k, v, **kw)
