"""TEST INFRASTRUCTURE: the CPU band backend (tests/_band_backend.py) extended with `mask_shift_lens`.

A block call with a non-zero `mask_shift_lens` is served sequence by sequence — packed (cu_seqlens) or dense input, whole
sequences or the halves the q_half / k_half selectors name — by an fp64 attention whose mask is written out element by
element from the definition in include/rfa.h (ABI 8),

    i + off_b - window_left <= j <= i + off_b + window_right ,
    off_b = (len_k(b) - len_q(b)) + mask_shift + mask_shift_lens * len_k(b)

(each side only when it is set, causal: window_right = 0; len_*: the lengths after the half selectors), with the
oracle's rounding points: a sequence's out / dq / dk / dv are rounded to the io dtype before they are merged / added in
fp32, rows that see no key leave the accumulators untouched.  Calls without the field are the parent's, untouched."""
import torch
import torch.nn.functional as F

from oracle.oracle_backend import BWD_ALL, BWD_COMPUTE, BWD_REDUCE, _lse_rows, _rows, _seqs

from _band_backend import BandBackend, _expand, _visible


class BandVarlenBackend(BandBackend):
    name = "oracle+band+lens"
    serves_mask_shift_lens = True

    def fwd(self, q, k, v, *, mask_shift=0, mask_shift_lens=0, **kw):
        if not mask_shift_lens:
            return super().fwd(q, k, v, mask_shift=mask_shift, **kw)
        assert kw.get("dropout") is None
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window", (-1, -1))
        out, lse, out_acc, lse_acc = kw.get("out"), kw.get("lse"), kw.get("out_acc"), kw.get("lse_acc")
        G = q.shape[-2] // k.shape[-2]
        for (bq, qs, ql), (bk, ks, kl) in zip(_seqs(q, kw.get("cu_seqlens_q"), kw.get("q_half", 0)),
                                              _seqs(k, kw.get("cu_seqlens_k"), kw.get("k_half", 0))):
            if ql == 0:
                continue
            vis = _visible(ql, kl, causal, window, mask_shift + mask_shift_lens * kl)
            s = torch.matmul(_rows(q, bq, qs, ql).double().permute(1, 0, 2), _expand(_rows(k, bk, ks, kl), G).transpose(1, 2)) * scale
            s = s.masked_fill(~vis, float("-inf"))
            l = torch.logsumexp(s, dim=-1) if kl else torch.full(s.shape[:2], float("-inf"), dtype=s.dtype)     # (H, ql)
            empty = torch.isinf(l)
            p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
            o = torch.matmul(p, _expand(_rows(v, bk, ks, kl), G)).permute(1, 0, 2).to(q.dtype)     # rounded like flash_attn's out
            l = l.float()
            if out_acc is None:
                _rows(out, bq, qs, ql).copy_(o)
                _lse_rows(lse, bq, qs, ql).copy_(torch.where(empty, torch.full_like(l, float("inf")), l))
                continue
            oa, la = _rows(out_acc, bq, qs, ql), _lse_rows(lse_acc, bq, qs, ql)
            if kw.get("acc_init"):
                oa.copy_(o.float())
                la.copy_(l)                                                # (-inf: nothing yet)
                continue
            bl = l.transpose(0, 1).unsqueeze(-1)                           # (ql, H, 1)
            cur = la.transpose(0, 1).unsqueeze(-1)
            new_o = oa - torch.sigmoid(bl - cur) * (oa - o.float())
            new_l = cur - F.logsigmoid(cur - bl)
            oa.copy_(torch.where(empty.transpose(0, 1).unsqueeze(-1), oa, new_o))
            la.copy_(torch.where(empty, la, new_l.squeeze(-1).transpose(0, 1)))

    def bwd(self, dout, q, k, v, lse, delta, *, mask_shift=0, mask_shift_lens=0, **kw):
        if not mask_shift_lens:
            return super().bwd(dout, q, k, v, lse, delta, mask_shift=mask_shift, **kw)
        assert kw.get("dropout") is None
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window", (-1, -1))
        phases = kw.get("phases", BWD_ALL)
        acc_init = kw.get("acc_init", False)
        kv_init = acc_init or bool(phases & 16)
        phases &= 3
        dq, dk, dv = kw.get("dq"), kw.get("dk"), kw.get("dv")
        dq_acc, dk_acc, dv_acc = kw.get("dq_acc"), kw.get("dk_acc"), kw.get("dv_acc")
        partials = kw.get("partials")
        H, D = q.shape[-2], q.shape[-1]
        Hk = k.shape[-2]
        G = H // Hk
        pairs = list(zip(_seqs(q, kw.get("cu_seqlens_q"), kw.get("q_half", 0)), _seqs(k, kw.get("cu_seqlens_k"), kw.get("k_half", 0))))
        if phases in (BWD_ALL, BWD_COMPUTE):
            pend = []
            for (bq, qs, ql), (bk, ks, kl) in pairs:
                vis = _visible(ql, kl, causal, window, mask_shift + mask_shift_lens * kl)
                qd, dod = _rows(q, bq, qs, ql).double().permute(1, 0, 2), _rows(dout, bq, qs, ql).double().permute(1, 0, 2)
                ke, ve = _expand(_rows(k, bk, ks, kl), G), _expand(_rows(v, bk, ks, kl), G)
                s = torch.matmul(qd, ke.transpose(1, 2)) * scale
                p = torch.exp(s - _lse_rows(lse, bq, qs, ql).double().unsqueeze(-1))
                p = torch.where(vis, p, torch.zeros_like(p))
                dp = torch.matmul(dod, ve.transpose(1, 2))
                ds = p * (dp - _lse_rows(delta, bq, qs, ql).double().unsqueeze(-1)) * scale
                gq = torch.matmul(ds, ke).permute(1, 0, 2).to(q.dtype)
                gk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, kl, D).sum(1).permute(1, 0, 2).to(q.dtype)
                gv = torch.matmul(p.transpose(1, 2), dod).view(Hk, G, kl, D).sum(1).permute(1, 0, 2).to(q.dtype)
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
