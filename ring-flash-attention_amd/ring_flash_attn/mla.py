"""Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi K2) between its projections and the attention call:
`apply_mla_rotary` and `apply_mla_rotary_freqs`.

The projections of an MLA layer leave q (.., Hq, Dn + Dr) whose last Dr columns are the rope part, kv (.., H, Dn + Dv) — the
`kv_b_proj` output per head, [k_nope | v] — and k_pe (.., 1, Dr), ONE rope key per token for all heads, a strided slice of the
`kv_a_proj` output.  Attention at a QK head dim of Dn + Dr = 192 and a value head dim of Dv = 128 (csrc/rfa_vdim.hip) wants q with
its rope columns rotated, k = [k_nope | rope(k_pe) for every head] and v, all contiguous — as torch ops a split, two rotations, an
expand, a cat and two copies, and backward a sum over heads.  `apply_mla_rotary` is one launch per direction
(HIP: csrc/rfa_mlarope.hip) at the GLOBAL positions of this rank's rows, which are `apply_rotary`'s to the letter.
`apply_mla_rotary_freqs` is the same call without tables: `inv_freq`, YaRN's `attention_scaling` and the positions, as
`apply_rotary_freqs` takes them; the kernel forms the angles (HIP: csrc/rfa_mlaropefreq.hip).
"""
import torch

from ._api import _opaque
from .rotary import _check_freqs, _check_tables_positions, _conforms


def _taken(t):
    """a tensor as the kernel takes it: itself, or a contiguous copy of one off the stride contract; None stays None"""
    return t if t is None or _conforms(t) else t.contiguous()


class _MlaRotary(torch.autograd.Function):
    """forward and backward are one launch each of the backend methods meta["method"] + "_fwd" / "_bwd" — `mla_rotary` with
    tables = (cos, sin), `mla_rotary_freqs` with tables = (inv_freq,).  Saved: the tables, the positions (or the map's numbers)
    and the dims — no activation: every gradient is a function of the incoming gradients alone."""

    @staticmethod
    def forward(ctx, q, kv, k_pe, positions, meta, *tables):
        from .backend import get_backend

        ctx.meta, ctx.k_pe_shape = meta, k_pe.shape
        ctx.save_for_backward(*tables, positions)
        ctx.set_materialize_grads(False)
        Dn, Dr, Dv = meta["dims"]
        lead, H = kv.shape[:-2], kv.shape[-2]
        new = lambda *shape: torch.empty(shape, dtype=kv.dtype, device=kv.device)
        q_out = None if q is None else new(*q.shape)
        k, v = new(*lead, H, Dn + Dr), new(*lead, H, Dv)
        getattr(get_backend(), meta["method"] + "_fwd")(_taken(q), q_out, _taken(kv), _taken(k_pe), k, v, *tables, nope_dim=Dn,
                                                        positions=positions, **meta["launch"])
        return q_out, k, v

    @staticmethod
    def backward(ctx, dq_out, dk, dv):
        from .backend import get_backend

        *tables, positions = ctx.saved_tensors
        Dn, Dr, Dv = ctx.meta["dims"]
        want_q, want_kv, want_pe = ctx.needs_input_grad[:3]
        g = dk if dk is not None else dv
        dq = dkv = dk_pe = None
        if want_q and dq_out is not None:
            dq = torch.empty(dq_out.shape, dtype=dq_out.dtype, device=dq_out.device)
        if want_kv and g is not None:
            # (a part whose gradient did not arrive is zero, and is not the kernel's work)
            make = torch.empty if dk is not None and dv is not None else torch.zeros
            dkv = make(*g.shape[:-1], Dn + Dv, dtype=g.dtype, device=g.device)
        if want_pe and dk is not None:
            dk_pe = torch.empty(ctx.k_pe_shape, dtype=dk.dtype, device=dk.device)
        if dq is not None or dkv is not None or dk_pe is not None:
            rest = dkv is not None or dk_pe is not None
            getattr(get_backend(), ctx.meta["method"] + "_bwd")(
                _taken(dq_out) if dq is not None else None, dq, _taken(dk) if rest else None, _taken(dv) if dkv is not None else None,
                dkv, dk_pe, *tables, nope_dim=Dn, v_dim=Dv, heads=ctx.meta["heads"], positions=positions, **ctx.meta["launch"])
        return (dq, dkv, dk_pe, None, None) + (None,) * len(tables)


def _check_mla(who, q, kv, k_pe, Dr, nope_dim):
    """the checks of q, kv and k_pe (tensors by now) that apply_mla_rotary and apply_mla_rotary_freqs share, once Dr is known;
    returns (Dn, Dv, H)"""
    if kv.dim() not in (3, 4):
        raise ValueError(f"{who}: kv must be (B, S, H, Dn + Dv) or packed (T, H, Dn + Dv), got {tuple(kv.shape)}")
    if kv.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: bf16 / fp16 only, got {kv.dtype}")
    lead, H = kv.shape[:-2], kv.shape[-2]
    if q is not None:
        if q.dim() != kv.dim() or q.shape[:-2] != lead or q.dtype != kv.dtype or q.device != kv.device or q.shape[-2] < 1:
            raise ValueError(f"{who}: q must share kv's batch, rows, dtype and device: {tuple(q.shape)} vs {tuple(kv.shape)}")
        Dn = q.shape[-1] - Dr
        if nope_dim is not None and int(nope_dim) != Dn:
            raise ValueError(f"{who}: nope_dim {nope_dim} disagrees with q: {q.shape[-1]} columns less Dr = {Dr} are {Dn}")
    elif nope_dim is None:
        raise ValueError(f"{who}: without q, nope_dim (the k_nope columns of kv) must be given")
    else:
        Dn = int(nope_dim)
    Dv = kv.shape[-1] - Dn
    if Dn < 0 or Dn % 8 or Dn + Dr > 256 or Dv < 8 or Dv % 8 or Dv > 256 or H < 1:
        raise ValueError(f"{who}: Dn = {Dn}, Dr = {Dr}, Dv = {Dv} must be multiples of 8 with Dn >= 0, Dn + Dr <= 256 and "
                         f"8 <= Dv <= 256, with at least one head")
    if tuple(k_pe.shape) not in (tuple(lead) + (1, Dr), tuple(lead) + (Dr,)) or k_pe.dtype != kv.dtype or k_pe.device != kv.device:
        raise ValueError(f"{who}: k_pe must be {tuple(lead) + (1, Dr)} or {tuple(lead) + (Dr,)} of kv's dtype on its device, got "
                         f"{tuple(k_pe.shape)} {k_pe.dtype}")
    return Dn, Dv, H


def apply_mla_rotary(q, kv, k_pe, cos, sin, *, nope_dim=None, layout=None, group=None, positions=None, offset=0, interleaved=False):
    """MLA's q, k and v for an attention call from the layer's projections, rotated at this rank's GLOBAL positions; returns
    (q_out, k, v), all contiguous and freshly allocated.

        q, k, v = apply_mla_rotary(q, kv, k_pe, cos, sin, layout=zigzag_ring_flash_attn_func, group=group)
        out = zigzag_ring_flash_attn_func(q, k, v, causal=True, group=group)          # QK head dim 192, value head dim 128

    q (B, S, Hq, Dn + Dr) or packed (T, Hq, Dn + Dr), or None: only k and v are made (q_out is None) and `nope_dim` = Dn must be
    given; with a q, Dn = q.shape[-1] - Dr and a `nope_dim` that disagrees is refused.  kv (.., H, Dn + Dv) = [k_nope | v] per
    head.  k_pe (.., 1, Dr) or (.., Dr): one rope key per token.  Hq and H are independent.  bf16 / fp16, one dtype; any strides
    with last stride 1 and 16-byte aligned rows are served without a copy (k_pe as a column slice of the kv_a_proj output, kv as
    a view of (B, S, H * (Dn + Dv))).  Dn, Dr, Dv multiples of 8 (Dr of 16 for the halves pairing), Dn + Dr <= 256, 8 <= Dv <= 256,
    Dn >= 0.
    cos, sin (P, Dr/2) and `layout`, `group`, `positions`, `offset`, `interleaved` are apply_rotary's, with its meaning and checks.
    Returns  q_out = [q[..., :Dn] | rope(q[..., Dn:])],  k[..., h, :] = [kv[..., h, :Dn] | rope(k_pe)] — the same rope bits for
    every head — and  v = kv[..., Dn:].  Copied columns keep their bits; rotated ones are apply_rotary's (fp32, o1 = x1 c - x2 s,
    o2 = x2 c + x1 s, one rounding): q_out is bit for bit apply_rotary(q, rot_offset=Dn), k's rope columns apply_rotary(k_pe).
    Autograd: one launch; dq is the conjugate rotation of dq_out, dkv = [dk[..., :Dn] | dv], and
    dk_pe = the conjugate rotation of sum_h dk[..., h, Dn:] — summed in fp32 in a fixed order that depends on H and Dr alone,
    rotated after the sum, rounded once, no atomics: two runs give the same bits.  An output whose gradient is None costs
    nothing; an input that does not require grad gets None; cos / sin get none.  Every rank's result is bit for bit the shard
    of the single-device result.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_mla_rotary`; TypeError for a `layout`
    as apply_rotary raises it; ValueError for everything else."""
    from .backend import get_backend

    who = "ring_flash_attn.apply_mla_rotary"
    be = get_backend()
    if not getattr(be, "serves_mla_rotary", False):
        raise NotImplementedError(f"{who} needs a backend that serves `mla_rotary`; {getattr(be, 'name', type(be).__name__)!r} "
                                  "does not")
    if not all(isinstance(t, torch.Tensor) for t in (kv, k_pe)) or (q is not None and not isinstance(q, torch.Tensor)):
        raise ValueError(f"{who}: q (or None), kv and k_pe must be tensors")
    if not isinstance(cos, torch.Tensor) or not isinstance(sin, torch.Tensor) or cos.dim() != 2:
        raise ValueError(f"{who}: cos and sin must be tensors of shape (P, Dr/2)")
    Dr = 2 * cos.shape[1]
    Dn, Dv, H = _check_mla(who, q, kv, k_pe, Dr, nope_dim)
    positions, pm, interleaved, _ = _check_tables_positions(who, kv, kv.dim() == 3, Dn + Dr, cos, sin, layout, group, positions,
                                                            offset, interleaved, Dn)
    meta = dict(method="mla_rotary", dims=(Dn, Dr, Dv), heads=H, launch=dict(pos_map=pm, interleaved=interleaved))
    return _MlaRotary.apply(q, kv, k_pe, positions, meta, cos, sin)


apply_mla_rotary = _opaque(apply_mla_rotary)


def apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, *, attention_scaling=1.0, nope_dim=None, layout=None, group=None, positions=None,
                           offset=0, interleaved=False):
    """`apply_mla_rotary` without tables: the kernel forms the angles from `inv_freq` and the positions; returns (q_out, k, v).
    No rank holds (P, Dr/2) tables of the unsharded sequence, and YaRN's `attention_scaling` — which DeepSeek-V2 / V3 / R1 and
    Kimi K2 all run with — is an argument.

        q, k, v = apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, attention_scaling=0.1 * math.log(40) + 1,
                                         layout=zigzag_ring_flash_attn_func, group=group)

    q, kv, k_pe, `nope_dim`, the returned tensors, the stride contract and the ranges of Dn, Dr, Dv are apply_mla_rotary's, with
    its checks; Dr = 2 len(inv_freq).  inv_freq (fp32 (Dr/2,), contiguous, on kv's device), attention_scaling (a finite float
    > 0 that multiplies cos and sin), `layout`, `group`, `positions` (any int32, not read on the host), `offset` and
    `interleaved` are apply_rotary_freqs's, with its checks; there is one position per row (no freq_axis).
    Per rotated pair, in fp32: ang = float(pos) * inv_freq[c] (one rounded multiply), the precise sincosf, both times
    attention_scaling, then apply_rotary's expression, each result rounded once: q_out is bit for bit
    apply_rotary_freqs(q, None, inv_freq, rot_offset=Dn, ...), k's rope columns apply_rotary_freqs(k_pe, ...) for every head;
    copied columns keep their bits.
    Autograd: one launch, no workspace, no atomics; dq is the conjugate rotation of dq_out, dkv = [dk[..., :Dn] | dv], and
    dk_pe = the conjugate rotation of sum_h dk[..., h, Dn:] — apply_mla_rotary's fp32 sum in its fixed order, rotated after the
    sum, rounded once: two runs give the same bits.  An output whose gradient is None costs nothing; an input that does not
    require grad gets None; inv_freq gets none.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_mla_rotary_freqs`; TypeError for a
    `layout` as apply_rotary raises it; ValueError for everything else."""
    from .backend import get_backend

    who = "ring_flash_attn.apply_mla_rotary_freqs"
    be = get_backend()
    if not getattr(be, "serves_mla_rotary_freqs", False):
        raise NotImplementedError(f"{who} needs a backend that serves `mla_rotary_freqs`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not")
    if not all(isinstance(t, torch.Tensor) for t in (kv, k_pe)) or (q is not None and not isinstance(q, torch.Tensor)):
        raise ValueError(f"{who}: q (or None), kv and k_pe must be tensors")
    if not isinstance(inv_freq, torch.Tensor) or inv_freq.dim() != 1:
        raise ValueError(f"{who}: inv_freq must be a contiguous fp32 (Dr/2,) tensor on kv's device")
    Dr = 2 * inv_freq.shape[0]
    Dn, Dv, H = _check_mla(who, q, kv, k_pe, Dr, nope_dim)
    positions, launch = _check_freqs(who, kv, kv.dim() == 3, Dn + Dr, inv_freq, attention_scaling, None, layout, group, positions,
                                     offset, interleaved, Dn)
    meta = dict(method="mla_rotary_freqs", dims=(Dn, Dr, Dv), heads=H,
                launch=dict(scaling=launch["scaling"], pos_map=launch["pos_map"], interleaved=launch["interleaved"]))
    return _MlaRotary.apply(q, kv, k_pe, positions, meta, inv_freq)


apply_mla_rotary_freqs = _opaque(apply_mla_rotary_freqs)
