"""TEST INFRASTRUCTURE: the CPU oracle backend with `mask_shift` (tests/_band_backend.py) extended with `alibi=`.

A block call with `alibi=(slopes, shift)` is served by the fp64 reference of tests/_alibi_ref.py at the oracle's rounding
points: the block's out / dq / dk / dv are rounded to the io dtype before they are merged / added in fp32, rows that see
no key leave the accumulators untouched.  Dense and packed input, plain and accumulate mode, one- and two-phase
backwards, a shifted causal diagonal (`mask_shift`); no window, no dropout, no halves — as in the library.  Calls without
a bias are the parent's, untouched."""
import torch
import torch.nn.functional as F

import _alibi_ref as AR
from _band_backend import BandBackend
from oracle.oracle_backend import BWD_ALL, BWD_COMPUTE, BWD_REDUCE, _lse_rows, _rows, _seqs


def _plain(kw):
    win = kw.get("window") or (-1, -1)
    assert win[0] < 0 and win[1] < 0 and kw.get("dropout") is None and not kw.get("q_half") and not kw.get("k_half")
    assert not kw.get("mask_shift_lens")


class AlibiBackend(BandBackend):
    name = "oracle+band+alibi"
    serves_alibi = True

    def fwd(self, q, k, v, *, alibi=None, **kw):
        if alibi is None:
            return super().fwd(q, k, v, **kw)
        _plain(kw)
        slopes, shift = alibi
        scale, causal, ms = kw["softmax_scale"], kw["causal"], kw.get("mask_shift", 0)
        out, lse, out_acc, lse_acc = kw.get("out"), kw.get("lse"), kw.get("out_acc"), kw.get("lse_acc")
        cq, ck = kw.get("cu_seqlens_q"), kw.get("cu_seqlens_k")
        assert cq is None or shift == 0
        for n, ((bq, qs, ql), (bk, ks, kl)) in enumerate(zip(_seqs(q, cq, 0), _seqs(k, ck, 0))):
            sl = slopes if slopes.dim() == 1 else slopes[n]
            o, l = AR._one(_rows(q, bq, qs, ql).double(), _rows(k, bk, ks, kl).double(), _rows(v, bk, ks, kl).double(),
                           sl, scale, causal, shift, ms)
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

    def bwd(self, dout, q, k, v, lse, delta, *, alibi=None, **kw):
        if alibi is None:
            return super().bwd(dout, q, k, v, lse, delta, **kw)
        _plain(kw)
        slopes, shift = alibi
        scale, causal, ms = kw["softmax_scale"], kw["causal"], kw.get("mask_shift", 0)
        phases = kw.get("phases", BWD_ALL)
        acc_init = kw.get("acc_init", False)
        kv_init = acc_init or bool(phases & 16)
        phases &= 3
        dq, dk, dv = kw.get("dq"), kw.get("dk"), kw.get("dv")
        dq_acc, dk_acc, dv_acc = kw.get("dq_acc"), kw.get("dk_acc"), kw.get("dv_acc")
        partials = kw.get("partials")
        cq, ck = kw.get("cu_seqlens_q"), kw.get("cu_seqlens_k")
        pairs = list(zip(_seqs(q, cq, 0), _seqs(k, ck, 0)))
        if phases in (BWD_ALL, BWD_COMPUTE):
            pend = []
            for n, ((bq, qs, ql), (bk, ks, kl)) in enumerate(pairs):
                sl = slopes if slopes.dim() == 1 else slopes[n]
                gq, gk, gv = AR.block_backward(_rows(dout, bq, qs, ql), _rows(q, bq, qs, ql), _rows(k, bk, ks, kl),
                                               _rows(v, bk, ks, kl), _lse_rows(lse, bq, qs, ql),
                                               _lse_rows(delta, bq, qs, ql), sl, scale, causal, shift, ms)
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
