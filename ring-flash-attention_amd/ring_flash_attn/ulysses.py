"""Ulysses head exchange around the dense schedules: `with_ulysses(func, ulysses_group)` and `make_usp_groups`.

A group of W = U * R ranks is used as U-way head parallelism (DeepSpeed-Ulysses) in front of an R-rank ring ("USP"): inside
its Ulysses group every rank trades heads for rows with ONE all-to-all, runs the unchanged schedule `func` over the ring group
on H / U heads of U times the rows, and trades `out` back.  The caller's sharding does not change — each rank holds exactly
the shard `func` over all W ranks expects — because the exchange places the rows so that the longer tensor IS `func`'s own
layout at world size R.  Local row i of S on Ulysses index p becomes merged row m:

    family               merged row m                                   Ulysses group of ring rank rho     ring group
    ring (contiguous)    p S + i                                        global ranks rho U .. rho U + U-1   equal p (stride U)
    zigzag (C = S/2)     i < C ? p C + i : U C + (U-1-p) C + (i - C)    as ring                             as ring
    stripe               i U + p                                        ranks rho + R p (stride R)          R p .. R p + R-1

(ring: rank g = rho U + p holds rows g S ..; the merged tensor is rows rho U S .. of the sequence: chunk rho of R.  zigzag: g
holds chunks g and 2W-1-g of 2W; the merged front is chunks rho U .. rho U + U-1 = big chunk rho of 2R, and g's back chunk
2W-1-g = (2R-1-rho) U + (U-1-p) is piece U-1-p of big chunk 2R-1-rho.  stripe: g = rho + R p holds tokens i W + g =
(i U + p) R + rho: merged token m is global token m R + rho.)

The layout change on either side of the all-to-all is one launch of the backend's `seq_head_copy` (HIP: csrc/rfa_seqhead.hip)
for all tensors of the call; q, k and v travel in ONE buffer and one collective per direction.
"""
import inspect

import torch
import torch.distributed as dist

from . import _C
from ._api import _admit, _bind, checked_vdim
from .utils import all_to_all_async, audit_verify

_LAYOUT = {"ring_flash_attn": _C.SEQHEAD_CONTIGUOUS, "zigzag_ring_flash_attn": _C.SEQHEAD_ZIGZAG,
           "stripe_flash_attn": _C.SEQHEAD_STRIPE}
_FORMS = ("_qkvpacked_func", "_kvpacked_func", "_func")


def _resolve(func, who):
    """(layout, form) of one of the nine dense public functions, or of a with_softcap result of one; TypeError otherwise
    (_api._RULES: the row of with_ulysses)"""
    name = _admit("with_ulysses", func, who)
    form = next(f for f in _FORMS if name.endswith(f))
    return _LAYOUT[name[:-len(form)]], form


def make_usp_groups(func, ulysses_size, group=None):
    """(ulysses_group, ring_group) of this rank for `func`'s family (the table above), made with dist.new_group out of the
    W ranks of `group` (None: the default group), W = ulysses_size * R.  A COLLECTIVE over `group`, to be called once: every
    rank creates every group, as torch.distributed requires.  ValueError: ulysses_size does not divide W."""
    layout, _ = _resolve(func, "make_usp_groups")
    ranks = dist.get_process_group_ranks(dist.group.WORLD if group is None else group)
    W, U = len(ranks), int(ulysses_size)
    if U < 1 or W % U:
        raise ValueError(f"ring_flash_attn.make_usp_groups: ulysses_size {ulysses_size} does not divide the group's {W} ranks")
    R = W // U
    if layout == _C.SEQHEAD_STRIPE:
        ulysses = [[ranks[rho + R * p] for p in range(U)] for rho in range(R)]
        rings = [[ranks[R * p + rho] for rho in range(R)] for p in range(U)]
    else:
        ulysses = [[ranks[rho * U + p] for p in range(U)] for rho in range(R)]
        rings = [[ranks[rho * U + p] for rho in range(R)] for p in range(U)]
    me = dist.get_rank()
    mine = [None, None]
    for k, family in enumerate((ulysses, rings)):
        for members in family:
            g = dist.new_group(members)
            if me in members:
                mine[k] = g
    return tuple(mine)


# ---- the exchange -------------------------------------------------------------------------------------------------------
def _kernel_view(t):
    """`t` as the copies take it: last stride 1, every other stride of a dimension longer than 1 a multiple of 8 elements, a
    16-byte aligned start (a strided view such as kv[:, :, 0] passes as it is) — anything else is copied once"""
    ok = t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(st % 8 == 0 for n, st in zip(t.shape[:-1], t.stride()[:-1]) if n > 1)
    return t if ok else t.contiguous()


def _exchange(group, U, layout, srcs, to_merged):
    """the tensors `srcs` — local views (B,S,[P,]H,D) when to_merged, else merged views (B,U*S,[P,]H/U,D) — in the other
    view, as new contiguous tensors: layout copy into U slots, ONE all-to-all over `group`, layout copy out of the slots.
    The collective goes through utils.all_to_all_async (side stream under RCCL, host staging under gloo in tests, the
    exchange audit) and is waited for here: the attention that follows needs all of it.  Overlapping the exchange with
    attention by head sub-groups is a follow-up."""
    from .backend import get_backend

    be = get_backend()
    srcs = [_kernel_view(t) for t in srcs]
    B, D = srcs[0].shape[0], srcs[0].shape[-1]
    S = srcs[0].shape[1] if to_merged else srcs[0].shape[1] // U

    def other(t):
        mid = tuple(t.shape[2:-2])
        return ((B, U * S) + mid + (t.shape[-2] // U, D)) if to_merged else ((B, S) + mid + (t.shape[-2] * U, D))

    total = sum(t.numel() for t in srcs)
    # B = 1, contiguous rows, ONE tensor: slot j of the buffer IS rows j S .. j S + S-1 of the merged tensor, so the merged
    # side needs no copy — the received buffer is returned as the merged tensor, a contiguous merged tensor is sent as it
    # is.  With several tensors per call (q | k | v) the parts interleave per slot and the merged tensors are not contiguous
    # in the buffer; one fused collective with an unpack launch was kept over three collectives without one: fewer
    # collectives on the latency-bound side, and one code path for every batch size and layout.
    direct = layout == _C.SEQHEAD_CONTIGUOUS and B == 1 and len(srcs) == 1
    if direct and not to_merged and srcs[0].is_contiguous():
        send = srcs[0].view(-1)
    else:
        send = torch.empty(total, dtype=srcs[0].dtype, device=srcs[0].device)
        be.seq_head_copy(_C.SEQHEAD_PACK if to_merged else _C.SEQHEAD_MERGED_TO_SLOTS, layout, U, srcs, send)
    recv = torch.empty_like(send)
    all_to_all_async(recv.view(U, -1), send.view(U, -1), group).wait()
    audit_verify(group, "with_ulysses exchange")                # (config.exchange_check: a no-op otherwise)
    if direct and to_merged:
        return [recv.view(other(srcs[0]))]
    dsts = [torch.empty(other(t), dtype=t.dtype, device=t.device) for t in srcs]
    be.seq_head_copy(_C.SEQHEAD_UNPACK if to_merged else _C.SEQHEAD_SLOTS_TO_HEADS, layout, U, dsts, recv)
    return dsts


class _HeadsForRows(torch.autograd.Function):
    """the call's tensors jointly (q, k, v | q, kv | qkv), local -> merged; backward: the inverse exchange of their gradients
    in one transfer.  Everything the backward needs is on the node.
    The backward ALWAYS sends all of the call's gradients, a missing one as zeros: which inputs need a gradient is rank-local
    autograd state, and a transfer whose size depended on it would leave the group inside a collective of mismatched sizes
    if the ranks ever disagreed.  The shapes of a collective here are a function of the call's shapes alone."""

    @staticmethod
    def forward(ctx, group, U, layout, *tensors):
        ctx.meta = (group, U, layout)
        ctx.set_materialize_grads(False)
        merged = tuple(_exchange(group, U, layout, [t.detach() for t in tensors], True))
        ctx.like = [(tuple(m.shape), m.dtype, m.device) for m in merged]
        return merged

    @staticmethod
    def backward(ctx, *grads):
        group, U, layout = ctx.meta
        if all(g is None for g in grads):                       # (autograd does not call this node then; kept for direct calls)
            return (None,) * (3 + len(grads))
        full = [g if g is not None else torch.zeros(shape, dtype=dtype, device=device)
                for g, (shape, dtype, device) in zip(grads, ctx.like)]
        back = _exchange(group, U, layout, full, False)
        return (None, None, None) + tuple(b if ctx.needs_input_grad[3 + i] else None for i, b in enumerate(back))


class _RowsForHeads(torch.autograd.Function):
    """`out`, merged -> local; backward: the forward-direction exchange of dout"""

    @staticmethod
    def forward(ctx, group, U, layout, out):
        ctx.meta = (group, U, layout)
        return _exchange(group, U, layout, [out.detach()], False)[0]

    @staticmethod
    def backward(ctx, dout):
        group, U, layout = ctx.meta
        return None, None, None, _exchange(group, U, layout, [dout], True)[0]


def _merged_rows(layout, U, S, device):
    """(U, S) int64: merged row of local row i of Ulysses index j (the table)"""
    j = torch.arange(U, device=device).view(U, 1)
    i = torch.arange(S, device=device).view(1, S)
    if layout == _C.SEQHEAD_STRIPE:
        return i * U + j
    if layout == _C.SEQHEAD_ZIGZAG:
        C = S // 2
        return torch.where(i < C, j * C + i, U * C + (U - 1 - j) * C + (i - C))
    return j * S + i


def _lse_back(group, U, layout, lse):
    """lse (B, H/U, U*S) fp32 of the merged call -> (B, H, S) of this rank's rows, all heads.  Plain torch and an all-to-all of
    its own: not a hot path (return_attn_probs=True is a testing option, as in flash_attn)."""
    B, Hs, US = lse.shape
    S = US // U
    rows = _merged_rows(layout, U, S, lse.device).reshape(-1)
    send = lse.detach().index_select(2, rows).view(B, Hs, U, S).permute(2, 0, 1, 3).contiguous()
    recv = torch.empty_like(send)
    all_to_all_async(recv.view(U, -1), send.view(U, -1), group).wait()
    audit_verify(group, "with_ulysses lse exchange")
    return recv.permute(1, 0, 2, 3).reshape(B, U * Hs, S)


def with_ulysses(func, ulysses_group):
    """DeepSpeed-Ulysses head parallelism in front of one of the nine dense schedules ("USP"):

        ug, rg = make_usp_groups(zigzag_ring_flash_attn_func, ulysses_size=4)      # collective, once
        attn = with_ulysses(zigzag_ring_flash_attn_func, ug)
        out = attn(q, k, v, causal=True, group=rg)                                  # q: (B, S, H, D), this rank's shard

    returns a callable with `func`'s signature.  Per call it exchanges heads for rows inside `ulysses_group` (size U, this
    rank at index p) — q (B, U S, H/U, D), k / v (B, U S, Hk/U, D), rows placed as `func` at 1/U of the ranks wants them
    (module docstring) —, calls `func` on those with the caller's other arguments unchanged (`group=` is the ring group),
    and exchanges `out` back to (B, S, H, D).  The caller's input sharding is what `func` over all U * R ranks expects.
    Served: ring_, zigzag_ring_ and stripe_flash_attn_{,kvpacked_,qkvpacked_}func and a with_softcap result of one; any ring
    size R >= 1 (R = 1: pure Ulysses); everything `func` serves — causal or not, windows, GQA, head dims, bf16 / fp16,
    alibi_slopes (this rank's head slice is passed on), return_attn_probs=True (lse comes back as (B, H, S) fp32).
    `ulysses_group` None: `func` itself.  A group of size 1 at the call: the plain call.
    TypeError: any other `func` (varlen, llama3: follow-up), a with_sinks result (follow-up), a with_ulysses result.
    At the call, before anything is exchanged, on every rank alike — ValueError: H or Hk not divisible by U, odd S with a
    zigzag function, differing q / k / v row counts; NotImplementedError: dropout_p > 0 (the mask hashes the head index, which
    the exchange renumbers: reproducing the unsharded bits needs the kernels' head offset at the public call, follow-up) and
    a backend without `serves_seq_head_exchange`.
    Autograd: the exchanges are two small autograd Functions around the unchanged `func`; their backwards are the inverse
    exchanges (dq, dk, dv in one transfer) and read nothing ambient, so activation checkpointing simply re-runs the call.
    One all-to-all per direction in front of and one behind the wrapped call, in forward and in backward (one more in the
    forward for lse with return_attn_probs=True).  Under torch.compile the call runs eagerly behind a graph break."""
    layout, form = _resolve(func, "with_ulysses")
    if ulysses_group is None:
        return func
    sig = inspect.signature(func)
    names = {"_func": ("q", "k", "v"), "_kvpacked_func": ("q", "kv"), "_qkvpacked_func": ("qkv",)}[form]

    def exchanged(*args, **kwargs):
        U = dist.get_world_size(ulysses_group)
        if U == 1:
            return func(*args, **kwargs)
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        a = bound.arguments
        tensors = [a[n] for n in names]
        _check_call(func, tensors, names, layout, U, a)
        merged = _HeadsForRows.apply(ulysses_group, U, layout, *tensors)
        for n, t in zip(names, merged):
            a[n] = t
        if a.get("alibi_slopes") is not None:
            Hs = merged[0].shape[-2]
            p = dist.get_rank(ulysses_group)
            a["alibi_slopes"] = a["alibi_slopes"][..., p * Hs:(p + 1) * Hs].contiguous()
        res = func(*bound.args, **bound.kwargs)
        if a.get("return_attn_probs"):
            out, lse, rest = res
            return (_RowsForHeads.apply(ulysses_group, U, layout, out), _lse_back(ulysses_group, U, layout, lse), rest)
        return _RowsForHeads.apply(ulysses_group, U, layout, res)

    return _bind("with_ulysses", func, body=exchanged)


def _check_call(func, tensors, names, layout, U, a):
    from .backend import get_backend

    what = getattr(func, "__name__", "func")
    be = get_backend()
    if not getattr(be, "serves_seq_head_exchange", False):
        raise NotImplementedError(f"ring_flash_attn: with_ulysses({what}) needs a backend that serves `seq_head_copy`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not")
    if a.get("dropout_p") and a["dropout_p"] > 0:
        raise NotImplementedError(f"ring_flash_attn: with_ulysses({what}) with dropout is not served: the mask hashes the head "
                                  "index, which the exchange renumbers (follow-up: the kernels' head offset at the public call)")
    for n, t in zip(names, tensors):
        want = 4 if n in ("q", "k", "v") else 5
        if not isinstance(t, torch.Tensor) or t.dim() != want:
            raise ValueError(f"ring_flash_attn: with_ulysses({what}): {n} must be a {want}-dimensional tensor")
    if names == ("q", "k", "v"):                     # (q, k, v travel in one buffer of one width)
        checked_vdim(*tensors, a.get("dropout_p"), a.get("alibi_slopes"), f"with_ulysses({what})", served=False)
    S = tensors[0].shape[1]
    if any(t.shape[1] != S or t.shape[0] != tensors[0].shape[0] for t in tensors):
        raise ValueError(f"ring_flash_attn: with_ulysses({what}): q, k and v must have the same batch and row counts, got "
                         f"{[tuple(t.shape) for t in tensors]}")
    for n, t in zip(names, tensors):
        if t.shape[-2] % U:
            raise ValueError(f"ring_flash_attn: with_ulysses({what}): the {t.shape[-2]} heads of {n} are not divisible by "
                             f"the Ulysses group's {U} ranks")
    if layout == _C.SEQHEAD_ZIGZAG and S % 2:
        raise ValueError(f"ring_flash_attn: with_ulysses({what}): a zigzag shard is two chunks, its {S} rows are odd")
