"""TEST INFRASTRUCTURE: the CPU test backend (tests/_ref_backend.py) with the gradient of lse and the pairwise merge —
`serves_lse_grad` (bwd_preprocess takes `dlse=`), `serves_merge_pair`, `merge_pair` and `merge_pair_bwd` in torch, with the
product's rounding points (include/rfa.h: rfa_bwd_preprocess_lse, rfa_merge_pair, rfa_merge_pair_bwd): fp32 arithmetic, delta'
= delta - dlse as ONE fp32 subtraction behind the oracle's delta, out / dout_a / dout_b rounded to the io dtype once, lse and
dlse_a / dlse_b fp32.  The schedules under test run unchanged on top of it."""
import torch

from _ref_backend import RefBackend


def pair_weights(la, lb):
    """(w_a, w_b, lse, empty_a, empty_b) of rfa_merge_pair, in la's dtype: an infinite lse of either sign is an empty side"""
    ea, eb = torch.isinf(la), torch.isinf(lb)
    zero, one = torch.zeros_like(la), torch.ones_like(la)
    fa, fb = torch.where(ea, zero, la), torch.where(eb, zero, lb)          # (finite stand-ins: no inf - inf below)
    d = fa - fb
    t = torch.exp(-d.abs())
    big, small = 1.0 / (1.0 + t), t / (1.0 + t)
    wa = torch.where(ea, zero, torch.where(eb, one, torch.where(d >= 0, big, small)))
    wb = torch.where(eb, zero, torch.where(ea, one, torch.where(d >= 0, small, big)))
    l = torch.maximum(fa, fb) + torch.log1p(t)
    l = torch.where(ea, torch.where(eb, torch.full_like(la, float("-inf")), lb), torch.where(eb, la, l))
    return wa, wb, l, ea, eb


def _rh(l):
    """lse (B, H, S) / (H, T) as (B, S, H, 1) / (T, H, 1): one value per (row, head) against out"""
    return l.transpose(-1, -2).unsqueeze(-1)


class LseGradBackend(RefBackend):
    serves_lse_grad = True
    serves_merge_pair = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+lse_grad"

    def bwd_preprocess(self, dout, out, delta, *, dlse=None, **kw):
        super().bwd_preprocess(dout, out, delta, **kw)
        if dlse is not None:
            assert dlse.dtype == torch.float32 and dlse.shape == delta.shape and dlse.stride(-1) == 1
            delta.sub_(dlse)

    def merge_pair(self, out_a, lse_a, out_b, lse_b):
        assert lse_a.dtype == torch.float32 and lse_b.dtype == torch.float32
        wa, wb, l, ea, eb = pair_weights(lse_a, lse_b)
        a = torch.where(_rh(ea), torch.zeros((), dtype=torch.float32), out_a.float())    # (an empty side is never multiplied)
        b = torch.where(_rh(eb), torch.zeros((), dtype=torch.float32), out_b.float())
        return (_rh(wa) * a + _rh(wb) * b).to(out_a.dtype), l

    def merge_pair_bwd(self, dout, dlse, out_a, lse_a, out_b, lse_b):
        wa, wb, _, ea, eb = pair_weights(lse_a, lse_b)
        live = ~(ea | eb)
        g = torch.zeros_like(lse_a) if dlse is None else dlse.float()
        x = (dout.float() * (out_a.float() - out_b.float())).sum(-1).transpose(-1, -2)
        cross = torch.where(live, wa * wb * x, torch.zeros_like(x))
        zero = torch.zeros_like(g)
        return ((_rh(wa) * dout.float()).to(dout.dtype), torch.where(ea, zero, wa * g + cross),
                (_rh(wb) * dout.float()).to(dout.dtype), torch.where(eb, zero, wb * g - cross))
