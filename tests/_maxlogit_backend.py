"""TEST INFRASTRUCTURE for ring_flash_attn.with_max_logit.  No test in here.

  * the fp64 reference: `row_max` — softmax_scale * q.k of the bf16 / fp16 inputs by einsum in fp64, masked with
    tests/_blockref.visible, max over the keys: one value per (query row, head); a head's max_logit over any set of rows (a
    rank's shard) is the amax of those rows.  `abs_bound` is the same with |q| |k|: what the device tolerance is made of.
  * `plant`: inputs that make a mask error visible — a pair of rows q_i = k_j = a ones / sqrt(D) gives the logit
    softmax_scale a^2 whatever D.  a = 16 at a VISIBLE band-edge element beats the random logits around it, a = 24 at a MASKED
    element right behind an edge (another row, another column) exceeds everything visible: a kernel or schedule that looks
    one element too far reports it.
  * `MaxLogitBackend`: the CPU test backend (tests/_ref_backend.py) with `max_logit` — the block's fp64 max from the same
    keywords a block call carries.
  * `tolerance`: |device - fp64| <= (D + 2) 2^-23 softmax_scale max_visible sum_d |q_d| |k_d| — the fp32 accumulation bound
    of a D-term dot product for any summation order, with a factor 2 (include/rfa.h: the products of 16-bit inputs are exact
    in fp32, the MFMA chain adds them in fp32, the scale is one more rounding)."""
import torch

from _blockref import visible
from _ref_backend import RefBackend
from oracle.oracle_backend import _rows, _seqs

NEG_INF = float("-inf")


def _seq_scores(q, k, scale, absolute=False):
    """(H, lq, lk) fp64 of one sequence: q (lq, H, D), k (lk, Hk, D)"""
    G = q.shape[1] // k.shape[1]
    qd, kd = q.double(), k.double().repeat_interleave(G, dim=1)
    if absolute:
        qd, kd = qd.abs(), kd.abs()
    return torch.einsum("ihd,jhd->hij", qd, kd) * scale


def _seq_row_max(q, k, scale, vis, absolute=False):
    """(lq, H) fp64: max over the visible keys of each row, -inf for a row that sees none"""
    lq, lk, H = q.shape[0], k.shape[0], q.shape[1]
    if lq == 0 or lk == 0:
        return torch.full((lq, H), NEG_INF, dtype=torch.float64, device=q.device)
    s = _seq_scores(q, k, scale, absolute).masked_fill(~vis.to(q.device), NEG_INF)
    return s.amax(dim=2).transpose(0, 1)


def row_max(q, k, scale, *, causal=False, window=(-1, -1), shift=0, shift_lens=0, cu_seqlens=None, q_half=0, k_half=0,
            cu_seqlens_k=None, absolute=False):
    """fp64, shaped like q without its last dimension — (B, Sq, H) or (T, H): every row's max visible logit, -inf for rows
    outside the selected half and rows that see nothing.  cu_seqlens: packed input (cu_seqlens_k: the keys' own, else the
    same); q_half / k_half: the kernels' half selectors"""
    cq = None if cu_seqlens is None else torch.as_tensor(cu_seqlens)
    ck = cq if cu_seqlens_k is None else torch.as_tensor(cu_seqlens_k)
    out = torch.full(q.shape[:-1], NEG_INF, dtype=torch.float64, device=q.device)
    for (bq, qs, ql), (bk, ks, kl) in zip(_seqs(q, cq, q_half), _seqs(k, ck, k_half)):
        vis = visible(ql, kl, causal, window, shift + shift_lens * kl)
        _rows(out, bq, qs, ql).copy_(_seq_row_max(_rows(q, bq, qs, ql), _rows(k, bk, ks, kl), scale, vis, absolute))
    return out


def head_max(rows):
    """(H,) from row_max's result (or a shard of it): amax over everything but the heads"""
    H = rows.shape[-1]
    flat = rows.reshape(-1, H)
    return flat.amax(dim=0) if flat.shape[0] else torch.full((H,), NEG_INF, dtype=torch.float64)


def tolerance(D, scale, abs_head_max):
    """per head: (D + 2) 2^-23 scale max sum |q||k| (abs_head_max comes from row_max(..., absolute=True), scale included)"""
    return (D + 2) * 2.0 ** -23 * abs_head_max.clamp_min(0.0)


def close(got, ref, tol):
    """-inf compares exactly, everything else within tol; returns the worst |got - ref| / tol (0 when nothing is finite)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), (got, ref)
    if inf.all():
        return 0.0
    err = (got[~inf] - ref[~inf]).abs()
    t = tol.double().cpu()[~inf]
    assert bool((err <= t).all()), (got, ref, err, t)
    return float((err / t.clamp_min(1e-300)).max())


# ---- plants ---------------------------------------------------------------------------------------------------------
VARIANTS = ("first", "last", "diag", "left")


def _pick(idx, where):
    return None if idx.shape[0] == 0 else tuple(int(x) for x in idx[{"first": 0, "last": -1}.get(where, idx.shape[0] // 2)])


def plant_pairs(vis, variant):
    """((i, j) visible or None, (i2, j2) masked or None) for one sequence's (lq, lk) visibility.  The visible element is the
    first / last visible one, one on the upper edge (its right neighbour is masked or does not exist: the diagonal, key
    lk - 1) or one on the window's left edge; the masked one lies right behind an edge — one element too far — in another
    row and another column."""
    lq, lk = vis.shape
    if lq == 0 or lk == 0 or not bool(vis.any()):
        return None, None
    right = torch.zeros_like(vis)
    right[:, :-1] = vis[:, 1:]
    left = torch.zeros_like(vis)
    left[:, 1:] = vis[:, :-1]
    allv = vis.nonzero()
    if variant == "diag":
        cand = (vis & ~right).nonzero()
    elif variant == "left":
        cand = (vis & ~left).nonzero()
    else:
        cand = allv
    v = _pick(cand if cand.shape[0] else allv, variant)
    behind = ((~vis) & (left | right)).nonzero()                   # masked, next to a visible element of its row
    behind = behind[(behind[:, 0] != v[0]) & (behind[:, 1] != v[1])]
    return v, _pick(behind, "last" if variant in ("last", "left") else "mid")


def plant_dense(q, k, vis, variants=VARIANTS):
    """dense q (B, Sq, H, D), k (B, Sk, Hk, D) with ONE visibility (Sq, Sk) for every batch entry; batch entry b, K/V head hk
    takes variants[(b + hk) % len].  Returns the list of (b, hk, visible, masked)."""
    D, G = q.shape[-1], q.shape[2] // k.shape[2]
    done = []
    for b in range(q.shape[0]):
        for hk in range(k.shape[2]):
            v, m = plant_pairs(vis, variants[(b + hk) % len(variants)])
            for pair, a in ((v, 16.0), (m, 24.0)):
                if pair is not None:
                    q[b, pair[0], hk * G:(hk + 1) * G] = a / D ** 0.5
                    k[b, pair[1], hk] = a / D ** 0.5
            done.append((b, hk, v, m))
    return done


def plant_packed(q, k, cu, vis_of, variants=VARIANTS):
    """packed q (T, H, D), k (T, Hk, D) with sequences cu; vis_of(n, L) -> (L, L) visibility of sequence n"""
    D, G = q.shape[-1], q.shape[1] // k.shape[1]
    done = []
    for n in range(len(cu) - 1):
        s, L = int(cu[n]), int(cu[n + 1] - cu[n])
        for hk in range(k.shape[1]):
            v, m = plant_pairs(vis_of(n, L), variants[(n + hk) % len(variants)])
            for pair, a in ((v, 16.0), (m, 24.0)):
                if pair is not None:
                    q[s + pair[0], hk * G:(hk + 1) * G] = a / D ** 0.5
                    k[s + pair[1], hk] = a / D ** 0.5
            done.append((n, hk, v, m))
    return done


# ---- the CPU test backend ----------------------------------------------------------------------------------------------
class MaxLogitBackend(RefBackend):
    """RefBackend + `max_logit`: the block's fp64 max from the keywords of the block call, stored to the fp32 tensor (the
    rounding of a max is the max of the roundings).  `calls` counts them."""
    serves_max_logit = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+max_logit"
        self.calls = []

    def max_logit(self, q, k, dst, *, softmax_scale, causal, cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None,
                  max_seqlen_k=None, q_half=0, k_half=0, window=(-1, -1), mask_shift=0, mask_shift_lens=0, accumulate=True,
                  head0=0):
        H = q.shape[-2]
        assert dst.dtype == torch.float32 and dst.dim() == 1 and 0 <= head0 and head0 + H <= dst.numel(), (dst.shape, head0, H)
        new = head_max(row_max(q.detach(), k.detach(), softmax_scale, causal=causal, window=window, shift=mask_shift,
                               shift_lens=mask_shift_lens, cu_seqlens=cu_seqlens_q, cu_seqlens_k=cu_seqlens_k,
                               q_half=q_half, k_half=k_half))
        self.calls.append((head0, H))
        sl = dst[head0:head0 + H]
        sl.copy_(torch.maximum(sl, new.float()) if accumulate else new.float())


class NoMaxLogit(RefBackend):
    """a backend that does not serve max_logit (and records that nobody called it)"""

    def __init__(self, serves=()):
        super().__init__(serves)
        self.called = 0

    def max_logit(self, *a, **kw):
        self.called += 1
        raise AssertionError("max_logit called on a backend that does not serve it")
