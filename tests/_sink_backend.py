"""TEST INFRASTRUCTURE: the CPU test backend (tests/_ref_backend.py) with attention sinks — `serves_sinks`, `sink_apply` and
`sink_grad` in torch, with the product's rounding points (include/rfa.h: rfa_sink_apply, rfa_sink_grad): fp32 arithmetic,
out' rounded to the io dtype, lse' and dsink fp32.  The schedules under test run unchanged on top of it."""
import torch

from _ref_backend import RefBackend


class SinkBackend(RefBackend):
    serves_sinks = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+sinks"

    def sink_apply(self, out, lse, sinks, *, varlen, inplace=False):
        assert out.dim() == (3 if varlen else 4) and lse.dtype == torch.float32
        l = lse.transpose(-1, -2)                                   # (B, S, H) / (T, H)
        s = sinks.detach().float().expand_as(l)
        inf = torch.isinf(l)
        d = torch.where(inf, torch.zeros_like(l), s - l)
        w = torch.where(inf, torch.zeros_like(l), 1.0 / (1.0 + torch.exp(d)))
        lnew = torch.where(inf, s, torch.maximum(l, s) + torch.log1p(torch.exp(-d.abs())))
        out_new = (out.float() * w.unsqueeze(-1)).to(out.dtype)
        lse_new = lnew.transpose(-1, -2).contiguous()
        if inplace:
            out.copy_(out_new)
            lse.copy_(lse_new)
            return out, lse
        return out_new, lse_new

    def sink_grad(self, dout, out, lse, sinks, *, varlen):
        assert out.dim() == (3 if varlen else 4)
        l = lse.transpose(-1, -2)
        dot = (dout.float() * out.float()).sum(-1)
        terms = torch.where(torch.isinf(l), torch.zeros_like(l), -torch.exp(sinks.detach().float().expand_as(l) - l) * dot)
        return terms.reshape(-1, terms.shape[-1]).sum(0)
