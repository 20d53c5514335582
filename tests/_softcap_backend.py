"""TEST INFRASTRUCTURE: the CPU oracle backend with `mask_shift` (tests/_band_backend.py) extended with `softcap=`.

A block call with softcap > 0 is served by the fp64 reference of tests/_softcap_ref.py at the oracle's rounding points: the
block's out / dq / dk / dv are rounded to the io dtype before they are merged / added in fp32, rows that see no key leave
the accumulators untouched.  Dense and packed input, halves, plain and accumulate mode, one- and two-phase backwards, a
window and a shifted band (`mask_shift`, `mask_shift_lens`); no dropout, no bias — as in the library.  Calls without a cap
are the parent's, untouched.  `Recording` wraps any backend and notes the `softcap` every block call carried."""
import torch
import torch.nn.functional as F

import _softcap_ref as SR
from _band_backend import BandBackend
from oracle.oracle_backend import BWD_ALL, BWD_COMPUTE, BWD_REDUCE, _lse_rows, _rows, _seqs


def _check(kw):
    assert kw.get("dropout") is None and kw.get("alibi") is None


def _shift(kw, kl):
    return kw.get("mask_shift", 0) + kw.get("mask_shift_lens", 0) * kl


class SoftcapBackend(BandBackend):
    name = "oracle+band+softcap"
    serves_softcap = True
    serves_mask_shift_lens = True

    def fwd(self, q, k, v, *, softcap=0.0, **kw):
        if not softcap:
            return super().fwd(q, k, v, **kw)
        _check(kw)
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window") or (-1, -1)
        out, lse, out_acc, lse_acc = kw.get("out"), kw.get("lse"), kw.get("out_acc"), kw.get("lse_acc")
        cq, ck = kw.get("cu_seqlens_q"), kw.get("cu_seqlens_k")
        for (bq, qs, ql), (bk, ks, kl) in zip(_seqs(q, cq, kw.get("q_half", 0)), _seqs(k, ck, kw.get("k_half", 0))):
            o, l = SR.block_forward(_rows(q, bq, qs, ql), _rows(k, bk, ks, kl), _rows(v, bk, ks, kl), scale, softcap,
                                    causal, window, _shift(kw, kl))
            o, l = o.to(q.dtype), l.float()                                # rounded like flash_attn's out
            empty = torch.isinf(l)                                         # +inf: no visible key
            if out_acc is None:
                _rows(out, bq, qs, ql).copy_(o)
                _lse_rows(lse, bq, qs, ql).copy_(l)
                continue
            oa, la = _rows(out_acc, bq, qs, ql), _lse_rows(lse_acc, bq, qs, ql)
            if kw.get("acc_init"):
                oa.copy_(o.float())
                la.copy_(torch.where(empty, torch.full_like(l, float("-inf")), l))
                continue
            bl = l.transpose(0, 1).unsqueeze(-1)                           # (l, H, 1)
            cur = la.transpose(0, 1).unsqueeze(-1)
            new_o = oa - torch.sigmoid(bl - cur) * (oa - o.float())
            new_l = cur - F.logsigmoid(cur - bl)
            oa.copy_(torch.where(empty.transpose(0, 1).unsqueeze(-1), oa, new_o))
            la.copy_(torch.where(empty, la, new_l.squeeze(-1).transpose(0, 1)))

    def bwd(self, dout, q, k, v, lse, delta, *, softcap=0.0, **kw):
        if not softcap:
            return super().bwd(dout, q, k, v, lse, delta, **kw)
        _check(kw)
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window") or (-1, -1)
        phases = kw.get("phases", BWD_ALL)
        acc_init = kw.get("acc_init", False)
        kv_init = acc_init or bool(phases & 16)
        phases &= 3
        dq, dk, dv = kw.get("dq"), kw.get("dk"), kw.get("dv")
        dq_acc, dk_acc, dv_acc = kw.get("dq_acc"), kw.get("dk_acc"), kw.get("dv_acc")
        partials = kw.get("partials")
        cq, ck = kw.get("cu_seqlens_q"), kw.get("cu_seqlens_k")
        pairs = list(zip(_seqs(q, cq, kw.get("q_half", 0)), _seqs(k, ck, kw.get("k_half", 0))))
        if phases in (BWD_ALL, BWD_COMPUTE):
            pend = []
            for (bq, qs, ql), (bk, ks, kl) in pairs:
                gq, gk, gv = SR.block_backward(_rows(dout, bq, qs, ql), _rows(q, bq, qs, ql), _rows(k, bk, ks, kl),
                                               _rows(v, bk, ks, kl), _lse_rows(lse, bq, qs, ql),
                                               _lse_rows(delta, bq, qs, ql), scale, softcap, causal, window, _shift(kw, kl))
                gq, gk, gv = gq.to(q.dtype), gk.to(q.dtype), gv.to(q.dtype)   # flash_attn rounds here
                if dq_acc is not None:
                    t = _rows(dq_acc, bq, qs, ql)
                    t.copy_(gq.float() if acc_init else t + gq.float())
                else:
                    _rows(dq, bq, qs, ql).copy_(gq)
                pend.append((gk, gv))
            if phases == BWD_COMPUTE:
                return pend
            partials = pend
        if phases in (BWD_ALL, BWD_REDUCE):
            assert partials is not None
            for ((bq, qs, ql), (bk, ks, kl)), (gk, gv) in zip(pairs, partials):
                if dk_acc is not None:
                    tk, tv = _rows(dk_acc, bk, ks, kl), _rows(dv_acc, bk, ks, kl)
                    tk.copy_(gk.float() if kv_init else tk + gk.float())
                    tv.copy_(gv.float() if kv_init else tv + gv.float())
                else:
                    _rows(dk, bk, ks, kl).copy_(gk)
                    _rows(dv, bk, ks, kl).copy_(gv)
        return None


class Recording:
    """any backend, with a note of the `softcap` each fwd / bwd block call carried (None: the keyword was absent); the
    wrapped backend runs the call WITHOUT the cap, so one that predates the keyword serves as well"""
    serves_softcap = True

    def __init__(self, inner):
        self.inner = inner
        self.seen = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def fwd(self, *a, **kw):
        self.seen["fwd"].append(kw.pop("softcap", None))
        return self.inner.fwd(*a, **kw)

    def bwd(self, *a, **kw):
        self.seen["bwd"].append(kw.pop("softcap", None))
        return self.inner.bwd(*a, **kw)
