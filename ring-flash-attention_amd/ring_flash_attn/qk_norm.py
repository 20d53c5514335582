"""QK RMSNorm fused with the rotary embedding at GLOBAL positions: per head with tables (`apply_qk_norm_rotary`), per head with the
angles formed in the kernel (`apply_qk_norm_rotary_freqs`) and over all heads of a token, with tables
(`apply_qk_token_norm_rotary`) or with the angles formed in the kernel (`apply_qk_token_norm_rotary_freqs`, both at the end of
this file).

Qwen3, Gemma-3 and OLMo-style models put an RMSNorm over each head of q and k directly in front of RoPE,
    q = rope(rmsnorm_D(q_proj(x)) * w_q),   k = rope(rmsnorm_D(k_proj(x)) * w_k).
As a torch composite in front of `apply_rotary` that is two more passes forward, four or five backward, a rounding to the io
dtype between norm and rotation, and a weight gradient out of an atomics-based reduction.  Here it is one launch per direction
(HIP: csrc/rfa_qknorm.hip), one rounding, a reproducible weight gradient, and — because positions are `apply_rotary`'s — shards
whose bits are the single-device result's.
"""
import math

import torch

from . import _C
from ._api import _opaque
from ._common import pos_map
from .rotary import _check_freqs, _check_qk, _check_tables_positions, _conforms


class _NormRotary(torch.autograd.Function):
    """norm (per head or over the token: meta["fwd"] / meta["bwd"] name the backend's methods) + rotation of one or two tensors
    in one launch.  Saved: the inputs, the weights, the tables — or, where the kernel forms its angles, inv_freq in the place of
    cos, sin None — and the positions (or the map's numbers): neither rstd, which the backward recomputes with the forward's own
    code, nor the outputs."""

    @staticmethod
    def forward(ctx, q, k, wq, wk, cos, sin, positions, meta):
        from .backend import get_backend

        tensors = (q,) if k is None else (q, k)
        weights = (wq,) if k is None else (wq, wk)
        srcs = [t if _conforms(t) else t.contiguous() for t in tensors]
        outs = [torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in tensors]
        getattr(get_backend(), meta["fwd"])(srcs, outs, list(weights), cos, sin, positions=positions, **meta["launch"])
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
        need_w = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        dx, dw = [None, None], [None, None]
        live = [i for i in range(n) if grads[i] is not None]
        if live:
            douts = [grads[i] if _conforms(grads[i]) else grads[i].contiguous() for i in live]
            dxs = [torch.empty(xs[i].shape, dtype=xs[i].dtype, device=xs[i].device) for i in live]
            dws = [torch.empty(ws[i].shape, dtype=torch.float32, device=ws[i].device) if need_w[i] else None for i in live]
            getattr(get_backend(), ctx.meta["bwd"])([xs[i] for i in live], douts, dxs, [ws[i] for i in live], dws, cos, sin,
                                                    positions=positions, **ctx.meta["launch"])
            for j, i in enumerate(live):
                dx[i] = dxs[j]
                dw[i] = dws[j].to(ws[i].dtype) if dws[j] is not None else None          # rounded once from the fp32 sum
        return (dx[0], dx[1], dw[0], dw[1], None, None, None, None)


def _norm_rotary(who, feature, check_weight, q, k, q_weight, k_weight, cos, sin, eps, weight_offset, layout, group, positions,
                 offset, interleaved, rot_offset, freqs=None):
    """what the four norm + rotary calls share: every check in front of the launch, in one order, and the node.  feature:
    `qk_norm` / `qk_norm_freqs` / `qk_token_norm` / `qk_token_norm_freqs` (the backend's serves_* flag and the stem of its two methods);
    check_weight(x, w, D): ValueError unless w is a weight of tensor x; freqs = (inv_freq, attention_scaling, freq_axis): the
    kernel forms the angles, there are no tables (cos = sin = None) and the angle's checks are apply_rotary_freqs's."""
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, f"serves_{feature}", False):
        raise NotImplementedError(f"{who} needs a backend that serves `{feature}`; {getattr(be, 'name', type(be).__name__)!r} "
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
    for x, w in [(q, q_weight)] if k is None else [(q, q_weight), (k, k_weight)]:
        check_weight(x, w, D)
    eps, weight_offset = float(eps), float(weight_offset)
    if not math.isfinite(eps) or eps < 0:
        raise ValueError(f"{who}: eps must be finite and not negative, got {eps}")
    if not math.isfinite(weight_offset):
        raise ValueError(f"{who}: weight_offset must be finite, got {weight_offset}")
    if freqs is not None:
        positions, launch = _check_freqs(who, q, packed, D, *freqs, layout, group, positions, offset, interleaved, rot_offset)
        cos = freqs[0]
    else:
        positions, pm, interleaved, rot_offset = _check_tables_positions(who, q, packed, D, cos, sin, layout, group, positions,
                                                                          offset, interleaved, rot_offset)
        if cos is None:                                # (the norm alone has no angle: nothing of the positions is used)
            positions, pm = None, pos_map(0)
        launch = dict(pos_map=pm, interleaved=interleaved, rot_offset=rot_offset)
    meta = dict(fwd=f"{feature}_rotary_fwd", bwd=f"{feature}_rotary_bwd", launch=dict(launch, eps=eps, weight_offset=weight_offset))
    outs = _NormRotary.apply(q, k, q_weight, k_weight, cos, sin, positions, meta)
    return outs[0] if k is None else outs


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
    who = "ring_flash_attn.apply_qk_norm_rotary"

    def check_weight(x, w, D):
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != (D,) or not w.is_contiguous() or w.device != q.device or \
                w.dtype not in (torch.float32, q.dtype) or w.dtype != q_weight.dtype:
            raise ValueError(f"{who}: the weights must be contiguous (D,) = ({D},) tensors on q's device, both fp32 or both {q.dtype}")

    return _norm_rotary(who, "qk_norm", check_weight, q, k, q_weight, k_weight, cos, sin, eps, weight_offset, layout, group,
                        positions, offset, interleaved, rot_offset)


apply_qk_norm_rotary = _opaque(apply_qk_norm_rotary)


def apply_qk_norm_rotary_freqs(q, k, q_weight, k_weight, inv_freq, *, eps=1e-6, weight_offset=0.0, attention_scaling=1.0,
                               freq_axis=None, layout=None, group=None, positions=None, offset=0, interleaved=False,
                               rot_offset=0):
    """`apply_qk_norm_rotary` without tables: the per-head RMSNorm and a rotation whose angles the kernel forms from `inv_freq`
    and the positions, fused (HIP: csrc/rfa_qknormfreq.hip); returns the new q, or (q, k).  Nothing of the size of the unsharded
    sequence is held, and a row may have up to four positions (M-RoPE).

        q, k = apply_qk_norm_rotary_freqs(q, k, w_q, w_k, inv_freq, layout=zigzag_ring_flash_attn_func, group=group)   # Qwen3
        q, k = apply_qk_norm_rotary_freqs(q, k, w_q, w_k, inv_freq, positions=pos_thw, freq_axis=axes)                 # Qwen3-VL

    q, k, q_weight, k_weight, eps, weight_offset, rot_offset and k=None with k_weight=None are `apply_qk_norm_rotary`'s, with
    its checks; inv_freq, attention_scaling, freq_axis, layout, group, positions, offset and interleaved are
    `apply_rotary_freqs`'s, with its checks (at most four axes; `layout` with freq_axis is a ValueError, and so is a map that
    leaves [0, 2^31 - 1]).  R = 2 len(inv_freq); the columns [rot_offset, rot_offset + R) are rotated, the norm always runs over
    all D columns.
    Per (row, head), in fp32 with ONE rounding to the io dtype at the end: `apply_qk_norm_rotary`'s norm, the angle
    ang = float(pos[axis(c)]) * inv_freq[c] as one rounded multiply, the precise sincosf, both times attention_scaling, then
    `apply_rotary`'s expression.  An element's bits depend on the row's values, the weight, the position(s), inv_freq and the
    scaling alone: every rank's shard is the shard of the single-device result, bit for bit, which the two calls this one
    replaces (the norm alone, then `apply_rotary_freqs`) do not give — they round to the io dtype in between.
    Autograd: one backward launch (plus a small fold) gives dq, dk and both weight gradients; kept are q, k, the weights,
    inv_freq and the positions or the map — neither rstd nor the outputs; the weight gradient is summed in fp32 in a fixed order
    without atomics (two runs: the same bits) and rounded once to the weight's dtype; inv_freq gets no gradient; a weight that
    does not require grad, or a tensor whose incoming gradient is None, skips that work.  Over several ranks the weight gradient
    is THIS RANK'S PARTIAL, like `sinks.grad`.  There is no in-place mode.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_qk_norm_freqs`; TypeError for a
    `layout` that is not one of the nine dense attention functions; ValueError for everything else."""
    who = "ring_flash_attn.apply_qk_norm_rotary_freqs"

    def check_weight(x, w, D):
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != (D,) or not w.is_contiguous() or w.device != q.device or \
                w.dtype not in (torch.float32, q.dtype) or w.dtype != q_weight.dtype:
            raise ValueError(f"{who}: the weights must be contiguous (D,) = ({D},) tensors on q's device, both fp32 or both {q.dtype}")

    return _norm_rotary(who, "qk_norm_freqs", check_weight, q, k, q_weight, k_weight, None, None, eps, weight_offset, layout, group,
                        positions, offset, interleaved, rot_offset, freqs=(inv_freq, attention_scaling, freq_axis))


apply_qk_norm_rotary_freqs = _opaque(apply_qk_norm_rotary_freqs)


def _token_weight_check(who, q, q_weight):
    """check_weight of the token-wide norms: w is (H * D,) or (H, D) for tensor x, and H * D is a width that is served"""
    width = _C.QK_TOKEN_NORM_MAX_WIDTH                 # H * D (and Hk * D) that is served: include/rfa.h

    def check_weight(x, w, D):
        H = x.shape[-2]
        if H * D > width:
            raise ValueError(f"{who}: H * D = {H * D} is more than the {width} columns a token row may have")
        if not isinstance(w, torch.Tensor) or tuple(w.shape) not in ((H * D,), (H, D)) or not w.is_contiguous() or \
                w.device != q.device or w.dtype not in (torch.float32, q.dtype) or w.dtype != q_weight.dtype:
            raise ValueError(f"{who}: the weights must be contiguous (H * D,) = ({H * D},) or (H, D) = ({H}, {D}) tensors on q's "
                             f"device, both fp32 or both {q.dtype}")

    return check_weight


def apply_qk_token_norm_rotary(q, k, q_weight, k_weight, cos=None, sin=None, *, eps=1e-6, weight_offset=0.0, layout=None,
                               group=None, positions=None, offset=0, interleaved=False, rot_offset=0):
    """RMSNorm of this rank's q (and k) over ALL heads of a token — OLMo-2 / OLMo-3 normalise q_proj(x) and k_proj(x) over the
    whole projection width before the heads are split — and the rotary embedding at their GLOBAL positions, fused; returns the
    new q, or (q, k).

        q, k = apply_qk_token_norm_rotary(q, k, w_q, w_k, cos, sin, layout=zigzag_ring_flash_attn_func, group=group)
        out = zigzag_ring_flash_attn_func(q, k, v, causal=True, group=group)

    Tensors, dtypes, D, strides, tables, every position argument and every refusal are `apply_qk_norm_rotary`'s, except:
    q_weight: (H * D,) or (H, D); k_weight: (Hk * D,) or (Hk, D) — contiguous, on q's device, fp32 or the io dtype (both the
    same); column h * D + d belongs to head h, column d.  H * D and Hk * D are at most 16384.
    Per token row, in fp32 with ONE rounding to the io dtype at the end:
        rstd = rsqrt(sum over all heads and columns of x^2 / (H D) + eps),  a = weight_offset + w,  y = (x rstd) a
    then the columns [rot_offset, rot_offset + R) of every head of y rotated by `apply_rotary`'s expression.  An element's bits
    depend on its token row's values, the weight and the position alone — not on the strides, on where the row sits in the
    launch, on whether k rode along or on how the position was delivered: every rank's shard is the shard of the single-device
    result, bit for bit.
    Autograd: one backward launch (plus a small fold) gives dq, dk and both weight gradients; rstd is recomputed, not saved; the
    weight gradient is summed in fp32 in a fixed order without atomics (two runs: the same bits) and rounded once to the
    weight's dtype; a weight that does not require grad, or a tensor whose incoming gradient is None, skips that work.
    Over several ranks the weight gradient is THIS RANK'S PARTIAL over its own rows, like `sinks.grad`; the statistic is
    token-local, so nothing crosses ranks under sequence parallelism.  Head-parallel callers (a `with_ulysses` region among
    them) split the token row across ranks and are not served.  There is no in-place mode.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_qk_token_norm`; TypeError for a
    `layout` that is not one of the nine dense attention functions; ValueError for everything else."""
    who = "ring_flash_attn.apply_qk_token_norm_rotary"
    return _norm_rotary(who, "qk_token_norm", _token_weight_check(who, q, q_weight), q, k, q_weight, k_weight, cos, sin, eps, weight_offset, layout, group,
                        positions, offset, interleaved, rot_offset)


apply_qk_token_norm_rotary = _opaque(apply_qk_token_norm_rotary)


def apply_qk_token_norm_rotary_freqs(q, k, q_weight, k_weight, inv_freq, *, eps=1e-6, weight_offset=0.0, attention_scaling=1.0,
                                     freq_axis=None, layout=None, group=None, positions=None, offset=0, interleaved=False,
                                     rot_offset=0):
    """`apply_qk_token_norm_rotary` without tables: the RMSNorm over ALL heads of a token and a rotation whose angles the kernel
    forms from `inv_freq` and the positions, fused (HIP: csrc/rfa_qktokenfreq.hip); returns the new q, or (q, k).  Nothing of
    the size of the unsharded sequence is held, and a row may have up to four positions (M-RoPE).

        q, k = apply_qk_token_norm_rotary_freqs(q, k, w_q, w_k, inv_freq, layout=zigzag_ring_flash_attn_func, group=group)  # OLMo-2
        q, k = apply_qk_token_norm_rotary_freqs(q, k, w_q, w_k, inv_freq, positions=pos_thw, freq_axis=axes)

    q, k, q_weight ((H * D,) or (H, D)), k_weight, eps, weight_offset, rot_offset and k=None with k_weight=None are
    `apply_qk_token_norm_rotary`'s, with its checks (H * D and Hk * D at most 16384); inv_freq, attention_scaling, freq_axis,
    layout, group, positions, offset and interleaved are `apply_rotary_freqs`'s, with its checks (at most four axes; `layout`
    with freq_axis is a ValueError, and so is a map that leaves [0, 2^31 - 1]).  R = 2 len(inv_freq); the columns [rot_offset,
    rot_offset + R) of every head are rotated, the norm always runs over all H * D columns.
    Per token row, in fp32 with ONE rounding to the io dtype at the end: `apply_qk_token_norm_rotary`'s norm (the same device
    functions: rstd has that kernel's bits), the angle ang = float(pos[axis(c)]) * inv_freq[c] as one rounded multiply, the
    precise sincosf, both times attention_scaling, then `apply_rotary`'s expression.  An element's bits depend on its token
    row's values, the weight, the position(s), inv_freq and the scaling alone: every rank's shard is the shard of the
    single-device result, bit for bit, which the two calls this one replaces (the token norm alone, then `apply_rotary_freqs`)
    do not give — they round to the io dtype in between.
    Autograd: one backward launch (plus a small fold) gives dq, dk and both weight gradients; kept are q, k, the weights,
    inv_freq and the positions or the map — neither rstd nor the outputs; the weight gradient is summed in fp32 in a fixed order
    without atomics (two runs: the same bits) and rounded once to the weight's dtype; inv_freq gets no gradient; a weight that
    does not require grad, or a tensor whose incoming gradient is None, skips that work.  Over several ranks the weight gradient
    is THIS RANK'S PARTIAL, like `sinks.grad`.  Head-parallel callers (a `with_ulysses` region among them) split the token row
    across ranks and are not served.  There is no in-place mode.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_qk_token_norm_freqs`; TypeError for a
    `layout` that is not one of the nine dense attention functions; ValueError for everything else."""
    who = "ring_flash_attn.apply_qk_token_norm_rotary_freqs"
    return _norm_rotary(who, "qk_token_norm_freqs", _token_weight_check(who, q, q_weight), q, k, q_weight, k_weight, None, None,
                        eps, weight_offset, layout, group, positions, offset, interleaved, rot_offset,
                        freqs=(inv_freq, attention_scaling, freq_axis))


apply_qk_token_norm_rotary_freqs = _opaque(apply_qk_token_norm_rotary_freqs)
