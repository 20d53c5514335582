"""TEST INFRASTRUCTURE: the CPU oracle backend (oracle/oracle_backend.py, frozen) extended with `mask_shift`.

A block call with a non-zero shift is served by an fp64 attention whose mask is written out element by element from
the definition in include/rfa.h,

    i + (len_k - len_q) + mask_shift - window_left  <=  j  <=  i + (len_k - len_q) + mask_shift + window_right

(each side only when it is set, causal: window_right = 0), with the oracle's rounding points: the block's out / dq / dk /
dv are rounded to the io dtype before they are merged / added in fp32, rows that see no key leave the accumulators
untouched.  Calls without a shift are the parent's, untouched.  Dense input only, as in the library."""
import torch
import torch.nn.functional as F

from oracle.oracle_backend import BWD_ALL, BWD_COMPUTE, BWD_REDUCE, OracleBackend


def _visible(lq, lk, causal, window, shift):
    wl, wr = (window if window is not None else (-1, -1))
    if causal:
        wr = 0
    i = torch.arange(lq).view(-1, 1) + (lk - lq) + shift
    j = torch.arange(lk).view(1, -1)
    m = torch.ones(lq, lk, dtype=torch.bool)
    if wr >= 0:
        m &= j <= i + wr
    if wl >= 0:
        m &= j >= i - wl
    return m


def _expand(k, G):
    return k.double().permute(1, 0, 2).repeat_interleave(G, dim=0)       # (H, Lk, D)


class BandBackend(OracleBackend):
    name = "oracle+band"
    serves_mask_shift = True

    def fwd(self, q, k, v, *, mask_shift=0, **kw):
        if not mask_shift:
            return super().fwd(q, k, v, **kw)
        assert kw.get("cu_seqlens_q") is None and not kw.get("q_half") and not kw.get("k_half") and kw.get("dropout") is None
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window", (-1, -1))
        out, lse, out_acc, lse_acc = kw.get("out"), kw.get("lse"), kw.get("out_acc"), kw.get("lse_acc")
        B, Lq, H, D = q.shape
        Lk, G = k.shape[1], H // k.shape[2]
        vis = _visible(Lq, Lk, causal, window, mask_shift)
        for b in range(B):
            s = torch.matmul(q[b].double().permute(1, 0, 2), _expand(k[b], G).transpose(1, 2)) * scale
            s = s.masked_fill(~vis, float("-inf"))
            l = torch.logsumexp(s, dim=-1)                                 # (H, Lq), -inf: no key
            empty = torch.isinf(l)
            p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
            o = torch.matmul(p, _expand(v[b], G)).permute(1, 0, 2).to(q.dtype)          # rounded like flash_attn's out
            l = l.float()
            if out_acc is None:
                out[b].copy_(o)
                lse[b].copy_(torch.where(empty, torch.full_like(l, float("inf")), l))
                continue
            oa, la = out_acc[b], lse_acc[b]
            if kw.get("acc_init"):
                oa.copy_(o.float())
                la.copy_(l)                                                # (-inf: nothing yet)
                continue
            bl = l.transpose(0, 1).unsqueeze(-1)                           # (Lq, H, 1)
            cur = la.transpose(0, 1).unsqueeze(-1)
            new_o = oa - torch.sigmoid(bl - cur) * (oa - o.float())
            new_l = cur - F.logsigmoid(cur - bl)
            oa.copy_(torch.where(empty.transpose(0, 1).unsqueeze(-1), oa, new_o))
            la.copy_(torch.where(empty, la, new_l.squeeze(-1).transpose(0, 1)))

    def bwd(self, dout, q, k, v, lse, delta, *, mask_shift=0, **kw):
        if not mask_shift:
            return super().bwd(dout, q, k, v, lse, delta, **kw)
        assert kw.get("cu_seqlens_q") is None and not kw.get("q_half") and not kw.get("k_half") and kw.get("dropout") is None
        scale, causal, window = kw["softmax_scale"], kw["causal"], kw.get("window", (-1, -1))
        phases = kw.get("phases", BWD_ALL)
        acc_init = kw.get("acc_init", False)
        kv_init = acc_init or bool(phases & 16)
        phases &= 3
        dq, dk, dv = kw.get("dq"), kw.get("dk"), kw.get("dv")
        dq_acc, dk_acc, dv_acc = kw.get("dq_acc"), kw.get("dk_acc"), kw.get("dv_acc")
        partials = kw.get("partials")
        B, Lq, H, D = q.shape
        Lk, Hk = k.shape[1], k.shape[2]
        G = H // Hk
        if phases in (BWD_ALL, BWD_COMPUTE):
            vis = _visible(Lq, Lk, causal, window, mask_shift)
            pend = []
            for b in range(B):
                qd, dod = q[b].double().permute(1, 0, 2), dout[b].double().permute(1, 0, 2)
                ke, ve = _expand(k[b], G), _expand(v[b], G)
                s = torch.matmul(qd, ke.transpose(1, 2)) * scale
                p = torch.exp(s - lse[b].double().unsqueeze(-1))
                p = torch.where(vis, p, torch.zeros_like(p))
                dp = torch.matmul(dod, ve.transpose(1, 2))
                ds = p * (dp - delta[b].double().unsqueeze(-1)) * scale
                gq = torch.matmul(ds, ke).permute(1, 0, 2).to(q.dtype)
                gk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, Lk, D).sum(1).permute(1, 0, 2).to(q.dtype)
                gv = torch.matmul(p.transpose(1, 2), dod).view(Hk, G, Lk, D).sum(1).permute(1, 0, 2).to(q.dtype)
                if dq_acc is not None:
                    dq_acc[b].copy_(gq.float() if acc_init else dq_acc[b] + gq.float())
                else:
                    dq[b].copy_(gq)
                pend.append((gk, gv))
            if phases == BWD_COMPUTE:
                return pend
            partials = pend
        if phases in (BWD_ALL, BWD_REDUCE):
            assert partials is not None
            for b, (gk, gv) in enumerate(partials):
                if dk_acc is not None:
                    dk_acc[b].copy_(gk.float() if kv_init else dk_acc[b] + gk.float())
                    dv_acc[b].copy_(gv.float() if kv_init else dv_acc[b] + gv.float())
                else:
                    dk[b].copy_(gk)
                    dv[b].copy_(gv)
        return None
