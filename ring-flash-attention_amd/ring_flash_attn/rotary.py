"""Rotary position embedding at GLOBAL positions for sharded q / k: `apply_rotary`, `apply_rotary_freqs` and `local_positions`.

Under context parallelism the rotation angle of local row i is its position in the unsharded sequence, and that depends on
the schedule: a ring rank holds one contiguous run, a zigzag rank two distant chunks, a stripe rank every W-th token, the
packed families count inside each document.  The package already does this arithmetic for the dropout hash, `with_row_ranges`,
`with_block_mask` and ALiBi (_common.pos_map / zigzag_map / stripe_map); `local_positions(func, n_local)` hands it out as an
int32 tensor for the sharding `func` expects, and `apply_rotary(q, k, cos, sin, layout=func)` rotates this rank's shards in
one launch of one streaming kernel (HIP: csrc/rfa_rotary.hip) — the positions of the dense families travel as the four numbers
of a position map, so no tensor is built.  `apply_rotary_freqs` takes `inv_freq` in place of the tables and forms the angles in
the kernel (HIP: csrc/rfa_rotfreq.hip): no table of the unsharded sequence on every rank, and rows with several positions
(multi-axis M-RoPE), which no table describes.
"""
import math

import torch
import torch.distributed as dist

from ._api import _opaque
from ._common import pos_map, stripe_map, zigzag_map

_FORMS = ("_qkvpacked_func", "_kvpacked_func", "_func")
_DENSE = ("ring_flash_attn", "zigzag_ring_flash_attn", "stripe_flash_attn")
_PACKED = ("ring_flash_attn_varlen", "zigzag_ring_flash_attn_varlen", "llama3_flash_attn_varlen", "zigzag_llama3_flash_attn_varlen")


def _family(func, who):
    """the family name (one of _DENSE + _PACKED) of one of the 21 public attention functions; TypeError otherwise"""
    import ring_flash_attn as pkg

    public = {id(getattr(pkg, n)): n for n in dir(pkg) if n.endswith("_func")}
    name = public.get(id(func)) if callable(func) else None
    if name is not None:
        for form in _FORMS:
            if name.endswith(form) and name[:-len(form)] in _DENSE + _PACKED:
                return name[:-len(form)]
    raise TypeError(f"ring_flash_attn.{who}: expected one of the public attention functions (ring_flash_attn.*_func; the result "
                    f"of a binder such as with_softcap is not unwrapped: pass the function it wraps), got {func!r}")


def _rank_world(group, rank, world_size):
    if rank is None:
        rank = dist.get_rank(group)
    if world_size is None:
        world_size = dist.get_world_size(group)
    rank, world_size = int(rank), int(world_size)
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"ring_flash_attn: rank {rank} is outside a group of {world_size} ranks")
    return rank, world_size


def _dense_map(family, n_local, rank, world):
    """the pos_map of a dense family's shard of n_local rows (the maps the schedules themselves use)"""
    if family == "zigzag_ring_flash_attn":
        if n_local % 2:
            raise ValueError(f"ring_flash_attn: a zigzag shard is two chunks, its {n_local} rows are odd")
        return zigzag_map(rank, world, n_local // 2)
    if family == "stripe_flash_attn":
        return stripe_map(rank, world)
    return pos_map(rank * n_local)


def _map_bounds(pm, n):
    """(smallest, largest) position of rows 0 .. n-1 under pos_map `pm` (its pieces are monotone: their ends bound them)"""
    off, (stride, split, off2) = pm
    stride = stride or 1
    ends = [off, off + ((split if split else n) - 1) * stride]
    if split:
        ends += [off2, off2 + (n - split - 1) * stride]
    return min(ends), max(ends)


def _map_tensor(pm, n, device):
    off, (stride, split, off2) = pm
    i = torch.arange(n, dtype=torch.int64, device=device)
    pos = off + i * (stride or 1)
    if split:
        pos = torch.where(i < split, pos, off2 + (i - split) * (stride or 1))
    return pos.to(torch.int32)


def _in_pieces(cu, first, idx):
    """for packed rows idx (int64) cut at the boundaries cu (int64, (n+1,)): (piece of each row, its index inside the piece);
    `first`: what the piece's first row counts as"""
    d = torch.searchsorted(cu[1:].contiguous(), idx, right=True).clamp_(max=cu.numel() - 2)
    return d, idx - cu[d] + (first[d] if first is not None else 0)


def local_positions(func, n_local, *, group=None, rank=None, world_size=None, cu_seqlens=None, device=None):
    """int32 tensor with the global position of every local row, in the order of q's rows, for the sharding `func` expects.

    func: one of the 21 public attention functions (TypeError otherwise; binder results are not unwrapped).  n_local: the rows
    of this rank's q — S of (B, S, H, D), T of packed (T, H, D).  rank / world_size override the group's (tests; the caller of
    a with_ulysses result shards like `func` over ALL ranks: pass the whole group).
      ring_*               rank * S + i
      zigzag_ring_*        chunks rank and 2W-1-rank of 2W (odd n_local: ValueError)
      stripe_*             i * W + rank
      *_varlen (ring, zigzag)   cu_seqlens = the LOCAL cu_seqlens the function is called with; every document is sharded like
                           the dense family, in units of its own local length; positions count inside each document
      llama3_*             cu_seqlens = the GLOBAL cu_seqlens; this rank's contiguous run of the token stream
      zigzag_llama3_*      cu_seqlens = the GLOBAL cu_seqlens; slices rank and 2W-1-rank of 2W, read off
                           zigzag_llama3_flash_attn_prepare_cu_seqlens
    Plain torch ops, no kernel; llama3_* and zigzag_llama3_* read cu_seqlens on the host once.  The result depends on the
    arguments alone: cache it."""
    family = _family(func, "local_positions")
    n_local = int(n_local)
    if n_local < 0:
        raise ValueError("ring_flash_attn.local_positions: n_local must not be negative")
    rank, W = _rank_world(group, rank, world_size)
    if family in _DENSE:
        if cu_seqlens is not None:
            raise ValueError(f"ring_flash_attn.local_positions: {family} is a dense family and takes no cu_seqlens")
        return _map_tensor(_dense_map(family, n_local, rank, W), n_local, device)
    if cu_seqlens is None:
        raise ValueError(f"ring_flash_attn.local_positions: {family} is a packed family and needs cu_seqlens")
    cu = torch.as_tensor(cu_seqlens)
    if device is None:
        device = cu.device
    idx = torch.arange(n_local, dtype=torch.int64, device=device)
    if family in ("ring_flash_attn_varlen", "zigzag_ring_flash_attn_varlen"):
        cu = cu.to(device=device, dtype=torch.int64)
        d, i = _in_pieces(cu, None, idx)
        L = (cu[1:] - cu[:-1])[d]                                  # the document's LOCAL length
        if family == "ring_flash_attn_varlen":
            return (rank * L + i).to(torch.int32)
        c = L // 2
        return torch.where(i < c, rank * c + i, (2 * W - 1 - rank) * c + (i - c)).to(torch.int32)
    # the llama3 families: a slice of the stream cut into n equal slices, as *_prepare_cu_seqlens describes it with `causal` —
    # the keys of a piece end with its last local query, so a piece's first query sits at (its keys) - (its queries)
    from .llama3_flash_attn_varlen import llama3_flash_attn_prepare_cu_seqlens
    from .zigzag_llama3_flash_attn_varlen import zigzag_llama3_flash_attn_prepare_cu_seqlens

    cu = cu.to(device="cpu", dtype=torch.int64)
    slices = 1 if family == "llama3_flash_attn_varlen" else 2
    total = int(cu[-1])
    if n_local % slices or n_local * W != total:
        raise ValueError(f"ring_flash_attn.local_positions: {family} over {W} ranks shards the {total} tokens of cu_seqlens "
                         f"into {total // W if total % W == 0 else total / W} rows per rank, not {n_local}")
    if slices == 1:
        params = (llama3_flash_attn_prepare_cu_seqlens(cu, True, rank, W),)
    else:
        params = zigzag_llama3_flash_attn_prepare_cu_seqlens(cu, True, rank, W)
    out = []
    for cu_q, cu_k, *_ in params:
        cu_q, cu_k = cu_q.to(device), cu_k.to(device)
        first = (cu_k[1:] - cu_k[:-1]) - (cu_q[1:] - cu_q[:-1])
        out.append(_in_pieces(cu_q, first, idx[:n_local // slices])[1])
    return torch.cat(out).to(torch.int32)


# ---- apply_rotary -------------------------------------------------------------------------------------------------------
def _conforms(t):
    """last stride 1, a 16-byte aligned start, every other stride of a dimension longer than 1 a multiple of 8 elements: what
    the kernel takes as it is (the slices of a qkv / kv packed tensor do)"""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(st % 8 == 0 for n, st in zip(t.shape[:-1], t.stride()[:-1]) if n > 1)


def _check_qk(who, q, k):
    """the shape / dtype checks of q and k that apply_rotary and apply_qk_norm_rotary share; returns (packed, D)"""
    if q.dim() not in (3, 4):
        raise ValueError(f"{who}: q must be (B, S, H, D) or packed (T, H, D), got {tuple(q.shape)}")
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: bf16 / fp16 only, got {q.dtype}")
    D = q.shape[-1]
    if D % 8 or not 8 <= D <= 256:
        raise ValueError(f"{who}: head dim {D} is not a multiple of 8 in 8 .. 256")
    if k is not None and (k.dim() != q.dim() or k.shape[:-2] != q.shape[:-2] or k.shape[-1] != D or k.dtype != q.dtype or
                          k.device != q.device):
        raise ValueError(f"{who}: k must share q's batch, rows, head dim, dtype and device: {tuple(q.shape)} vs {tuple(k.shape)}")
    return q.dim() == 3, D


def _check_tables_positions(who, q, packed, D, cos, sin, layout, group, positions, offset, interleaved, rot_offset):
    """the checks of the tables, the rotated columns and the positions that apply_rotary and apply_qk_norm_rotary share, in
    apply_rotary's order; cos = sin = None (apply_qk_norm_rotary's norm alone) is R = 0: no table, no bound on the positions.
    Returns (positions, pos_map, interleaved, rot_offset) as the backend takes them."""
    P = R = 0
    interleaved = bool(interleaved)
    if cos is not None:
        if cos.dim() != 2 or cos.shape != sin.shape or cos.dtype != sin.dtype or not cos.is_contiguous() or not sin.is_contiguous():
            raise ValueError(f"{who}: cos and sin must be contiguous (P, R/2) tensors of one shape and dtype")
        if cos.dtype not in (torch.float32, q.dtype) or cos.device != q.device or sin.device != q.device:
            raise ValueError(f"{who}: cos / sin must be fp32 or {q.dtype} on q's device")
        P, R = cos.shape[0], 2 * cos.shape[1]
        if P < 1 or R < 1 or R % (8 if interleaved else 16):
            raise ValueError(f"{who}: the rotary width R = {R} must be a positive multiple of {8 if interleaved else 16} "
                             f"({'interleaved' if interleaved else 'halves'}), with at least one table row")
    rot_offset, offset = int(rot_offset), int(offset)
    if rot_offset < 0 or rot_offset % 8 or rot_offset + R > D:
        raise ValueError(f"{who}: rot_offset {rot_offset} must be a multiple of 8 with rot_offset + R = {rot_offset + R} <= D = {D}")
    if layout is not None and positions is not None:
        raise ValueError(f"{who}: at most one of `layout` and `positions`")
    S = q.shape[0] if packed else q.shape[1]
    if positions is not None:
        want = ((S,),) if packed else ((S,), (q.shape[0], S))
        if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or tuple(positions.shape) not in want or \
                positions.device != q.device:
            raise ValueError(f"{who}: positions must be an int32 tensor of shape {' or '.join(map(str, want))} on q's device")
        return positions.contiguous(), pos_map(offset), interleaved, rot_offset
    if layout is not None:
        family = _family(layout, who.rsplit(".", 1)[-1])
        if family not in _DENSE:
            raise TypeError(f"{who}: `layout` serves the nine dense functions; for {family} pass "
                            "positions=local_positions(func, T, cu_seqlens=...)")
        if packed:
            raise ValueError(f"{who}: `layout` needs (B, S, H, D) input")
        off, rest = _dense_map(family, S, *_rank_world(group, None, None))
        pm = (off + offset, (rest[0], rest[1], rest[2] + offset if rest[1] else 0))
    else:
        pm = pos_map(offset)
    if S and cos is not None:
        lo, hi = _map_bounds(pm, S)
        if lo < 0 or hi > P - 1:
            raise ValueError(f"{who}: the rows sit at positions {lo} .. {hi}, the tables have {P} rows")
    return None, pm, interleaved, rot_offset


class _Rotary(torch.autograd.Function):
    """the rotation of one or two tensors in one launch of the backend method meta["method"] — `rotary` with tables = (cos, sin),
    `rotary_freqs` with tables = (inv_freq,); backward: the same kernel with the conjugate flag on the incoming gradients.
    Saved: the tables, the positions (or the map's numbers) and the flags — neither inputs nor outputs."""

    @staticmethod
    def forward(ctx, q, k, positions, meta, *tables):
        from .backend import get_backend

        # (q comes first: where autograd rewrites the history of a VIEW modified in place it takes the view for input 0)
        tensors = (q,) if k is None else (q, k)
        ctx.meta = meta
        ctx.save_for_backward(*tables, positions)
        ctx.set_materialize_grads(False)
        if meta["inplace"]:
            ctx.mark_dirty(*tensors)
            outs = list(tensors)
        else:
            outs = [torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in tensors]
        srcs = [t if _conforms(t) else t.contiguous() for t in tensors]        # (inplace: checked to conform before)
        getattr(get_backend(), meta["method"])(srcs, outs, *tables, positions=positions, conj=False, **meta["launch"])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from .backend import get_backend

        *tables, positions = ctx.saved_tensors
        live = [g for g in grads if g is not None]
        if live:
            srcs = [g if _conforms(g) else g.contiguous() for g in live]
            outs = [torch.empty(g.shape, dtype=g.dtype, device=g.device) for g in live]
            getattr(get_backend(), ctx.meta["method"])(srcs, outs, *tables, positions=positions, conj=True, **ctx.meta["launch"])
            it = iter(outs)
            grads = tuple(next(it) if g is not None else None for g in grads)
        return (grads[0], grads[1] if len(grads) > 1 else None, None, None) + (None,) * len(tables)


def _rotate(who, method, q, k, tables, positions, inplace, launch):
    """the end of apply_rotary and apply_rotary_freqs: the check of `inplace`, then the node on q and k"""
    tensors = [q] if k is None else [q, k]
    inplace = bool(inplace)
    if inplace and not all(_conforms(t) for t in tensors):
        raise ValueError(f"{who}: inplace=True needs last stride 1, a 16-byte aligned start and strides that are multiples of 8")
    meta = dict(method=method, inplace=inplace, launch=launch)
    if inplace and k is not None and torch.is_grad_enabled() and any(t._is_view() for t in tensors):
        # (autograd lets a Function that modifies a VIEW in place return one tensor only: q and k one after the other — the
        #  bits do not depend on it)
        return tuple(_Rotary.apply(t, None, positions, meta, *tables)[0] for t in tensors)
    outs = _Rotary.apply(q, k, positions, meta, *tables)
    return outs[0] if k is None else outs


def apply_rotary(q, k=None, cos=None, sin=None, *, layout=None, group=None, positions=None, offset=0, interleaved=False,
                 rot_offset=0, inplace=False):
    """Rotary position embedding of this rank's q (and k) at their GLOBAL positions; returns the rotated q, or (q, k).

        q, k = apply_rotary(q, k, cos, sin, layout=zigzag_ring_flash_attn_func, group=group)
        out = zigzag_ring_flash_attn_func(q, k, v, causal=True, group=group)

    q (B, S, H, D) and k (B, S, Hk, D), or packed (T, H, D) and (T, Hk, D); bf16 / fp16; D a multiple of 8 in 8 .. 256; any
    strides with last stride 1 and 16-byte aligned rows are served without a copy (the slices of a qkv / kv packed tensor).
    q and k share rows and positions and go through one launch.
    cos, sin: (P, R/2), contiguous, fp32 or the io dtype.  The columns [rot_offset, rot_offset + R) of every head are rotated,
    the rest pass through (MLA's rope part: rot_offset=128, R=64 of 192).  interleaved=False pairs column c with c + R/2
    (GPT-NeoX; R a multiple of 16), interleaved=True columns 2c and 2c+1 (GPT-J; R a multiple of 8).
    Positions, at most one of:
      layout=func      one of the nine dense functions: the positions local_positions(func, S, group=group) of its shards,
                       handed to the kernel as the four numbers of a position map — no tensor is built
      positions=       int32 (S,) or (B, S) — packed input: (T,) — on q's device: the packed families' local_positions,
                       Hugging Face's position_ids.  They are not read on the host (no sync): the CALLER OWNS THEIR RANGE; the
                       kernel clamps them to [0, P-1], so it never reads outside the tables, and a position outside is
                       silently the nearest row's angle
      neither          row i is position i
    `offset` is added in every mode.  With a map the largest position is known on the host: a P it does not fit is a
    ValueError before any launch.
    Arithmetic: fp32, o1 = x1 c - x2 s, o2 = x2 c + x1 s, each rounded once; an element's bits depend on its values and its
    position alone — not on how the position was delivered, the strides, `inplace`, or whether k rode along.
    Autograd: the backward is the same kernel with s -> -s on the incoming gradients; cos / sin get no gradient.
    inplace=True rotates q and k where they are (they must conform to the stride contract), marks them dirty and returns them.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_rotary`; TypeError for a `layout`
    that is not one of the public attention functions or is one of the packed families; ValueError for everything else."""
    from .backend import get_backend

    who = "ring_flash_attn.apply_rotary"
    be = get_backend()
    if not getattr(be, "serves_rotary", False):
        raise NotImplementedError(f"{who} needs a backend that serves `rotary`; {getattr(be, 'name', type(be).__name__)!r} "
                                  "does not")
    if not isinstance(q, torch.Tensor) or (k is not None and not isinstance(k, torch.Tensor)):
        raise ValueError(f"{who}: q and k must be tensors")
    if not isinstance(cos, torch.Tensor) or not isinstance(sin, torch.Tensor):
        raise ValueError(f"{who}: cos and sin must be tensors of shape (P, R/2)")
    packed, D = _check_qk(who, q, k)
    positions, pm, interleaved, rot_offset = _check_tables_positions(who, q, packed, D, cos, sin, layout, group, positions, offset,
                                                                      interleaved, rot_offset)
    return _rotate(who, "rotary", q, k, (cos, sin), positions, inplace,
                   dict(pos_map=pm, interleaved=interleaved, rot_offset=rot_offset))


apply_rotary = _opaque(apply_rotary)


# ---- apply_rotary_freqs -------------------------------------------------------------------------------------------------
_POS_MAX = 2 ** 31 - 1


def _check_freqs(who, q, packed, D, inv_freq, attention_scaling, freq_axis, layout, group, positions, offset, interleaved,
                 rot_offset):
    """the checks of inv_freq, the scaling, freq_axis and the positions that apply_rotary_freqs and apply_qk_norm_rotary_freqs
    share, in apply_rotary_freqs's order.  Returns (positions, launch): the positions as the backend takes them and its
    keywords scaling, freq_axis, pos_map, interleaved, rot_offset."""
    if not isinstance(inv_freq, torch.Tensor) or inv_freq.dtype != torch.float32 or inv_freq.dim() != 1 or \
            not inv_freq.is_contiguous() or inv_freq.device != q.device:
        raise ValueError(f"{who}: inv_freq must be a contiguous fp32 (R/2,) tensor on q's device")
    interleaved = bool(interleaved)
    half = inv_freq.shape[0]
    R = 2 * half
    if R < 1 or R % (8 if interleaved else 16):
        raise ValueError(f"{who}: the rotary width R = {R} must be a positive multiple of {8 if interleaved else 16} "
                         f"({'interleaved' if interleaved else 'halves'})")
    if isinstance(attention_scaling, bool) or not isinstance(attention_scaling, (int, float)) or \
            not math.isfinite(attention_scaling) or not attention_scaling > 0:
        raise ValueError(f"{who}: attention_scaling must be a finite number > 0, got {attention_scaling!r}")
    S = q.shape[0] if packed else q.shape[1]
    if freq_axis is None:
        # (apply_rotary's checks of rot_offset, layout and positions; no table: nothing bounds the positions there)
        positions, pm, _, rot_offset = _check_tables_positions(who, q, packed, D, None, None, layout, group, positions, offset,
                                                               interleaved, rot_offset)
        if positions is None and S:
            lo, hi = _map_bounds(pm, S)
            if lo < 0 or hi > _POS_MAX:
                raise ValueError(f"{who}: the rows sit at positions {lo} .. {hi}, outside 0 .. 2^31 - 1")
    else:
        if isinstance(freq_axis, torch.Tensor):
            if freq_axis.is_floating_point() or freq_axis.device.type != "cpu" or freq_axis.dim() != 1:
                raise ValueError(f"{who}: freq_axis must be a sequence or a 1-d CPU int tensor")
            freq_axis = freq_axis.tolist()
        freq_axis = tuple(freq_axis)
        if len(freq_axis) != half or not all(isinstance(a, int) and not isinstance(a, bool) for a in freq_axis):
            raise ValueError(f"{who}: freq_axis must hold R/2 = {half} ints, one axis number per frequency")
        if layout is not None:
            if _family(layout, who.rsplit(".", 1)[-1]) not in _DENSE:
                raise TypeError(f"{who}: `layout` serves the nine dense functions")
            raise ValueError(f"{who}: `layout` yields one position per row and cannot serve freq_axis; pass positions= of shape (A, ...)")
        _, pm, _, rot_offset = _check_tables_positions(who, q, packed, D, None, None, None, group, None, offset, interleaved,
                                                       rot_offset)
        lead = ((S,),) if packed else ((S,), (q.shape[0], S))
        if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or positions.device != q.device or \
                not positions.is_contiguous() or not 1 <= positions.shape[0] <= 4 or tuple(positions.shape[1:]) not in lead:
            raise ValueError(f"{who}: with freq_axis, positions must be a contiguous int32 tensor of shape "
                             f"{' or '.join(str(('A',) + w) for w in lead)}, 1 <= A <= 4, on q's device")
        A = positions.shape[0]
        if not all(0 <= a < A for a in freq_axis):
            raise ValueError(f"{who}: freq_axis must name axes in [0, {A}), the first dimension of positions")
    # (rot_offset is apply_rotary's by now: an int, a multiple of 8 inside D; the offset of tensor positions is bounded like a
    # map's, where rfa_rotary_freqs would refuse it)
    if rot_offset + R > D:
        raise ValueError(f"{who}: rot_offset {rot_offset} must be a multiple of 8 with rot_offset + R = {rot_offset + R} <= D = {D}")
    if positions is not None and abs(pm[0]) > _POS_MAX:
        raise ValueError(f"{who}: offset {pm[0]} is outside -(2^31 - 1) .. 2^31 - 1")
    return positions, dict(scaling=float(attention_scaling), freq_axis=freq_axis, pos_map=pm, interleaved=interleaved,
                           rot_offset=rot_offset)


def apply_rotary_freqs(q, k=None, inv_freq=None, *, attention_scaling=1.0, freq_axis=None, layout=None, group=None,
                       positions=None, offset=0, interleaved=False, rot_offset=0, inplace=False):
    """`apply_rotary` without tables: the kernel forms the angles from `inv_freq` and the positions; returns the rotated q, or
    (q, k).  Nothing of the size of the unsharded sequence is held, and a row may have up to four positions (M-RoPE).

        q, k = apply_rotary_freqs(q, k, inv_freq, layout=zigzag_ring_flash_attn_func, group=group)
        q, k = apply_rotary_freqs(q, k, inv_freq, positions=position_ids_thw, freq_axis=axes)      # Qwen2-VL / Qwen3-VL

    q, k, `layout`, `group`, `positions`, `offset`, `interleaved`, `rot_offset` and `inplace` are apply_rotary's, with its checks.
    inv_freq: fp32 (R/2,), contiguous, on q's device — with whatever Llama-3 / YaRN / NTK / linear scaling the model applies
    already in it; R = 2 len(inv_freq) obeys apply_rotary's rules.  attention_scaling: a finite float > 0 that multiplies cos and
    sin (Hugging Face's convention for YaRN / longrope).
    freq_axis=None: one position per row — `positions` int32 (S,) / (B, S) / (T,), or `layout`, or neither (row i is position i).
    freq_axis = a sequence or CPU int tensor of R/2 axis numbers in [0, A), 1 <= A <= 4: `positions` must be given, int32,
    contiguous, (A, S), (A, B, S) or (A, T), and frequency c reads axis freq_axis[c]; `layout` is refused (a map yields one number
    per row).  For R/2 = 64 and (t, h, w) position_ids:
      Qwen2-VL, mrope_section [16, 24, 24]:   freq_axis = [0] * 16 + [1] * 24 + [2] * 24
      Qwen3-VL, interleaved [24, 20, 20]:     freq_axis = [0] * 64; freq_axis[1:60:3] = [1] * 20; freq_axis[2:60:3] = [2] * 20
    Per rotated pair, in fp32: ang = float(pos) * inv_freq[c] (one rounded multiply — what inv_freq.float() @
    position_ids.float() gives), (s, c) = sincosf(ang) with full range reduction, both times attention_scaling, then
    apply_rotary's expression, each result rounded once.  An element's bits depend on its values, its position(s), inv_freq and
    the scaling alone.  Tensor positions may be any int32 and are not read on the host; a map (`layout` / `offset`) whose
    positions leave [0, 2^31 - 1] is a ValueError.
    Autograd: the backward is the same kernel with s -> -s on the incoming gradients; inv_freq gets no gradient.
    Under torch.compile the call runs eagerly behind a graph break.
    Raises, before anything is launched: NotImplementedError for a backend without `serves_rotary_freqs`; TypeError for a
    `layout` as apply_rotary raises it; ValueError for everything else."""
    from .backend import get_backend

    who = "ring_flash_attn.apply_rotary_freqs"
    be = get_backend()
    if not getattr(be, "serves_rotary_freqs", False):
        raise NotImplementedError(f"{who} needs a backend that serves `rotary_freqs`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not")
    if not isinstance(q, torch.Tensor) or (k is not None and not isinstance(k, torch.Tensor)):
        raise ValueError(f"{who}: q and k must be tensors")
    packed, D = _check_qk(who, q, k)
    positions, launch = _check_freqs(who, q, packed, D, inv_freq, attention_scaling, freq_axis, layout, group, positions, offset,
                                     interleaved, rot_offset)
    return _rotate(who, "rotary_freqs", q, k, (inv_freq,), positions, inplace, launch)


apply_rotary_freqs = _opaque(apply_rotary_freqs)
