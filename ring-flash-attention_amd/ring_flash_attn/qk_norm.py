"""Per-head QK RMSNorm fused with the rotary embedding at GLOBAL positions: `apply_qk_norm_rotary`.

Qwen3, Gemma-3 and OLMo-style models put an RMSNorm over each head of q and k directly in front of RoPE,
    q = rope(rmsnorm_D(q_proj(x)) * w_q),   k = rope(rmsnorm_D(k_proj(x)) * w_k).
As a torch composite in front of `apply_rotary` that is two more passes forward, four or five backward, a rounding to the io
dtype between norm and rotation, and a weight gradient out of an atomics-based reduction.  Here it is one launch per direction
(HIP: csrc/rfa_qknorm.hip), one rounding, a reproducible weight gradient, and — because positions are `apply_rotary`'s — shards
whose bits are the single-device result's.
"""
import math

import torch

from ._api import _opaque
from ._common import pos_map
from .rotary import _check_qk, _check_tables_positions, _conforms


class _QkNormRotary(torch.autograd.Function):
    """norm + rotation of one or two tensors in one launch.  Saved: the inputs, the weights, the tables and the positions (or
    the map's numbers) — neither rstd, which the backward recomputes with the forward's own code, nor the outputs."""

    @staticmethod
    def forward(ctx, q, k, wq, wk, cos, sin, positions, meta):
        from .backend import get_backend

        tensors = (q,) if k is None else (q, k)
        weights = (wq,) if k is None else (wq, wk)
        pm, interleaved, rot_offset, eps, weight_offset = meta
        srcs = [t if _conforms(t) else t.contiguous() for t in tensors]
        outs = [torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in tensors]
        get_backend().qk_norm_rotary_fwd(srcs, outs, list(weights), cos, sin, positions=positions, pos_map=pm,
                                         interleaved=interleaved, rot_offset=rot_offset, eps=eps, weight_offset=weight_offset)
        ctx.meta = meta
        ctx.n = len(tensors)
        ctx.save_for_backward(cos, sin, positions, *srcs, *weights)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from .backend import get_backend

        cos, sin, positions, *rest = ctx.saved_tensors
        n = ctx.n
        xs, ws = rest[:n], rest[n:]
        pm, interleaved, rot_offset, eps, weight_offset = ctx.meta
        need_w = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        dx, dw = [None, None], [None, None]
        live = [i for i in range(n) if grads[i] is not None]
        if live:
            douts = [grads[i] if _conforms(grads[i]) else grads[i].contiguous() for i in live]
            dxs = [torch.empty(xs[i].shape, dtype=xs[i].dtype, device=xs[i].device) for i in live]
            dws = [torch.empty(ws[i].shape, dtype=torch.float32, device=ws[i].device) if need_w[i] else None for i in live]
            get_backend().qk_norm_rotary_bwd([xs[i] for i in live], douts, dxs, [ws[i] for i in live], dws, cos, sin,
                                             positions=positions, pos_map=pm, interleaved=interleaved, rot_offset=rot_offset,
                                             eps=eps, weight_offset=weight_offset)
            for j, i in enumerate(live):
                dx[i] = dxs[j]
                dw[i] = dws[j].to(ws[i].dtype) if dws[j] is not None else None          # rounded once from the fp32 sum
        return (dx[0], dx[1], dw[0], dw[1], None, None, None, None)


def apply_qk_norm_rotary(q, k, q_weight, k_weight, cos=None, sin=None, *, eps=1e-6, weight_offset=0.0, layout=None, group=None,
                         positions=None, offset=0, interleaved=False, rot_offset=0):
    """Per-head RMSNorm of this rank's q (and k) and the rotary embedding at their GLOBAL positions, fused; returns the new q,
    or (q, k).

        q, k = apply_qk_norm_rotary(q, k, w_q, w_k, cos, sin, layout=zigzag_ring_flash_attn_func, group=group)    # Qwen3
        out = zigzag_ring_flash_attn_func(q, k, v, causal=True, group=group)

    q (B, S, H, D) and k (B, S, Hk, D), or packed (T, H, D) and (T, Hk, D); dtype, D (a multiple of 8 in 8 .. 256), the stride
    contract and the copy rule are `apply_rotary`'s.  k=None with k_weight=None serves one tensor.
    q_weight, k_weight: (D,), contiguous, on q's device, fp32 or the io dtype (both the same); they may require grad.
    cos, sin, layout, group, positions, offset, interleaved, rot_offset: exactly `apply_rotary`'s.  cos=None, sin=None is the
    normalisation alone, no column is rotated (NoPE layers).
    Per (row, head), in fp32 with ONE rounding to the io dtype at the end:
        rstd = rsqrt(sum_c x_c^2 / D + eps),  a_c = weight_offset + w_c,  y_c = (x_c rstd) a_c
    (Gemma-3: weight_offset=1.0), then the columns [rot_offset, rot_offset + R) of y rotated by `apply_rotary`'s expression; the
    norm always runs over all D columns.  An element's bits depend on the row's values, the weight and the position alone.
    Autograd: one backward launch (plus a small fold) gives dq, dk and both weight gradients; rstd is recomputed, not saved; the
    weight gradient is summed in fp32 in a fixed order (two runs: the same bits) and rounded once to the weight's dtype; cos /
    sin get no gradient; a weight that does not require grad, or a tensor whose incoming gradient is None, skips that work.
    Over several ranks the weight gradient is THIS RANK'S PARTIAL over its own rows — like `sinks.grad`: the package posts no
    collective, the caller's data-parallel reduction covers it.  There is no in-place mode: the backward needs x.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_qk_norm`; TypeError for a `layout`
    that is not one of the nine dense attention functions; ValueError for everything else."""
    from .backend import get_backend

    who = "ring_flash_attn.apply_qk_norm_rotary"
    be = get_backend()
    if not getattr(be, "serves_qk_norm", False):
        raise NotImplementedError(f"{who} needs a backend that serves `qk_norm`; {getattr(be, 'name', type(be).__name__)!r} "
                                  "does not")
    if not isinstance(q, torch.Tensor) or (k is not None and not isinstance(k, torch.Tensor)):
        raise ValueError(f"{who}: q and k must be tensors")
    if (k is None) != (k_weight is None):
        raise ValueError(f"{who}: k and k_weight come together (both None: one tensor)")
    if (cos is None) != (sin is None):
        raise ValueError(f"{who}: cos and sin come together (both None: the norm alone)")
    if cos is not None and (not isinstance(cos, torch.Tensor) or not isinstance(sin, torch.Tensor)):
        raise ValueError(f"{who}: cos and sin must be tensors of shape (P, R/2)")
    packed, D = _check_qk(who, q, k)
    weights = [q_weight] if k is None else [q_weight, k_weight]
    for w in weights:
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != (D,) or not w.is_contiguous() or w.device != q.device or \
                w.dtype not in (torch.float32, q.dtype) or w.dtype != weights[0].dtype:
            raise ValueError(f"{who}: the weights must be contiguous (D,) = ({D},) tensors on q's device, both fp32 or both {q.dtype}")
    eps, weight_offset = float(eps), float(weight_offset)
    if not math.isfinite(eps) or eps < 0:
        raise ValueError(f"{who}: eps must be finite and not negative, got {eps}")
    if not math.isfinite(weight_offset):
        raise ValueError(f"{who}: weight_offset must be finite, got {weight_offset}")
    positions, pm, interleaved, rot_offset = _check_tables_positions(who, q, packed, D, cos, sin, layout, group, positions, offset,
                                                                      interleaved, rot_offset)
    if cos is None:                                    # (the norm alone has no angle: nothing of the positions is used)
        positions, pm = None, pos_map(0)
    meta = (pm, interleaved, rot_offset, eps, weight_offset)
    outs = _QkNormRotary.apply(q, k, q_weight, k_weight, cos, sin, positions, meta)
    return outs[0] if k is None else outs


apply_qk_norm_rotary = _opaque(apply_qk_norm_rotary)
