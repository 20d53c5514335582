"""TEST INFRASTRUCTURE: the CPU oracle backend (oracle/oracle_backend.py, frozen) extended with dropout position maps.

A dense block call whose `dropout=` carries a position map — the 7-tuple (p, seed, q_pos_offset, k_pos_offset,
head_offset, q_map, k_map) of ring_flash_attn._common.dropout_arg, each map (stride, split, offset2) — is served by an
fp64 attention whose keep mask is

    oracle.flash_attn_ref.dropout_keep(seed, p, batch, heads, [pos_q(i)], [pos_k(j)])
    pos(i) = (split == 0 or i < split) ? offset + i * stride : offset2 + (i - split) * stride          (include/rfa.h)

with the oracle's rounding points (the block's out / dq / dk / dv are rounded to the io dtype before they are merged /
added in fp32; rows that see no key leave the accumulators untouched) and its `drop_rescale`.  lse is that of the undropped
softmax.  Every other call — no dropout, or the 5-tuple of an identity map — is the parent's, untouched.

`fwd64` / `bwd64` are the unrounded fp64 block results; the GPU tests compare the kernels with them directly."""
import torch
import torch.nn.functional as F

from oracle import flash_attn_ref as O
from oracle.oracle_backend import BWD_ALL, BWD_COMPUTE, BWD_REDUCE, OracleBackend


def positions(offset, m, n):
    """global positions of local rows 0 .. n-1 under the map m = (stride, split, offset2) behind `offset`"""
    stride, split, off2 = m
    stride = stride or 1
    return [offset + i * stride if (split == 0 or i < split) else off2 + (i - split) * stride for i in range(n)]


def keep_mask(dropout, b, H, Lq, Lk):
    """bool (H, Lq, Lk): the keep mask of batch entry b of a block call with the 5- or 7-tuple `dropout`"""
    p, seed, q0, k0, h0 = dropout[:5]
    qm, km = dropout[5:7] if len(dropout) > 5 else ((1, 0, 0), (1, 0, 0))
    return O.dropout_keep(seed, p, b, range(h0, h0 + H), positions(q0, qm, Lq), positions(k0, km, Lk))


def _visible(lq, lk, causal):
    if not causal:
        return torch.ones(lq, lk, dtype=torch.bool)
    return torch.arange(lk).view(1, -1) <= torch.arange(lq).view(-1, 1) + (lk - lq)


def _expand(k, G):
    return k.double().permute(1, 0, 2).repeat_interleave(G, dim=0)       # (H, Lk, D)


def fwd64(q, k, v, scale, causal, dropout):
    """per batch entry: (out fp64 (Lq, H, D), lse fp64 (H, Lq), -inf where a row sees no key)"""
    B, Lq, H, D = q.shape
    Lk, G = k.shape[1], H // k.shape[2]
    vis = _visible(Lq, Lk, causal)
    rp = O.drop_rescale(dropout[0])
    res = []
    for b in range(B):
        s = torch.matmul(q[b].double().permute(1, 0, 2), _expand(k[b], G).transpose(1, 2)) * scale
        s = s.masked_fill(~vis, float("-inf"))
        l = torch.logsumexp(s, dim=-1)
        empty = torch.isinf(l)
        p = torch.exp(s - torch.where(empty, torch.zeros_like(l), l).unsqueeze(-1))
        p = torch.where(keep_mask(dropout, b, H, Lq, Lk), p * rp, torch.zeros_like(p))
        res.append((torch.matmul(p, _expand(v[b], G)).permute(1, 0, 2), l))
    return res


def bwd64(dout, q, k, v, lse, delta, scale, causal, dropout):
    """per batch entry: fp64 (dq (Lq, H, D), dk (Lk, Hk, D), dv (Lk, Hk, D)); lse / delta (B, H, Lq)"""
    B, Lq, H, D = q.shape
    Lk, Hk = k.shape[1], k.shape[2]
    G = H // Hk
    vis = _visible(Lq, Lk, causal)
    rp = O.drop_rescale(dropout[0])
    res = []
    for b in range(B):
        qd, dod = q[b].double().permute(1, 0, 2), dout[b].double().permute(1, 0, 2)
        ke, ve = _expand(k[b], G), _expand(v[b], G)
        s = torch.matmul(qd, ke.transpose(1, 2)) * scale
        p = torch.exp(s - lse[b].double().unsqueeze(-1))
        p = torch.where(vis, p, torch.zeros_like(p))
        keep = keep_mask(dropout, b, H, Lq, Lk)
        dp = torch.matmul(dod, ve.transpose(1, 2))
        dp = torch.where(keep, dp * rp, torch.zeros_like(dp))
        pd = torch.where(keep, p * rp, torch.zeros_like(p))
        ds = p * (dp - delta[b].double().unsqueeze(-1)) * scale
        gq = torch.matmul(ds, ke).permute(1, 0, 2)
        gk = torch.matmul(ds.transpose(1, 2), qd).view(Hk, G, Lk, D).sum(1).permute(1, 0, 2)
        gv = torch.matmul(pd.transpose(1, 2), dod).view(Hk, G, Lk, D).sum(1).permute(1, 0, 2)
        res.append((gq, gk, gv))
    return res


def _mapped(dropout):
    return dropout is not None and dropout[0] > 0 and len(dropout) > 5


class DropPosBackend(OracleBackend):
    name = "oracle+droppos"
    serves_dropout_positions = True

    def fwd(self, q, k, v, **kw):
        dropout = kw.get("dropout")
        if not _mapped(dropout):
            return super().fwd(q, k, v, **kw)
        assert kw.get("cu_seqlens_q") is None and not kw.get("q_half") and not kw.get("k_half")
        assert kw.get("window", (-1, -1)) in (None, (-1, -1)) and not kw.get("mask_shift")
        out, lse, out_acc, lse_acc = kw.get("out"), kw.get("lse"), kw.get("out_acc"), kw.get("lse_acc")
        for b, (o, l) in enumerate(fwd64(q, k, v, kw["softmax_scale"], kw["causal"], dropout)):
            o = o.to(q.dtype)                                              # rounded like flash_attn's out
            empty = torch.isinf(l)
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

    def bwd(self, dout, q, k, v, lse, delta, **kw):
        dropout = kw.get("dropout")
        if not _mapped(dropout):
            return super().bwd(dout, q, k, v, lse, delta, **kw)
        assert kw.get("cu_seqlens_q") is None and not kw.get("q_half") and not kw.get("k_half")
        assert kw.get("window", (-1, -1)) in (None, (-1, -1)) and not kw.get("mask_shift")
        phases = kw.get("phases", BWD_ALL)
        acc_init = kw.get("acc_init", False)
        kv_init = acc_init or bool(phases & 16)
        phases &= 3
        dq, dk, dv = kw.get("dq"), kw.get("dk"), kw.get("dv")
        dq_acc, dk_acc, dv_acc = kw.get("dq_acc"), kw.get("dk_acc"), kw.get("dv_acc")
        partials = kw.get("partials")
        if phases in (BWD_ALL, BWD_COMPUTE):
            pend = []
            for b, (gq, gk, gv) in enumerate(bwd64(dout, q, k, v, lse, delta, kw["softmax_scale"], kw["causal"], dropout)):
                gq, gk, gv = gq.to(q.dtype), gk.to(q.dtype), gv.to(q.dtype)
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
