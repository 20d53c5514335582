"""Rotary position embedding at GLOBAL positions for sharded q / k: `apply_rotary` and `local_positions`.

Under context parallelism the rotation angle of local row i is its position in the unsharded sequence, and that depends on
the schedule: a ring rank holds one contiguous run, a zigzag rank two distant chunks, a stripe rank every W-th token, the
packed families count inside each document.  The package already does this arithmetic for the dropout hash, `with_row_ranges`,
`with_block_mask` and ALiBi (_common.pos_map / zigzag_map / stripe_map); `local_positions(func, n_local)` hands it out as an
int32 tensor for the sharding `func` expects, and `apply_rotary(q, k, cos, sin, layout=func)` rotates this rank's shards in
one launch of one streaming kernel (HIP: csrc/rfa_rotary.hip) — the positions of the dense families travel as the four numbers
of a position map, so no tensor is built.
"""
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
    """the rotation of one or two tensors in one launch; backward: the same kernel with the conjugate flag on the incoming
    gradients.  Saved: cos, sin, the positions (or the map's numbers) and the flags — neither inputs nor outputs."""

    @staticmethod
    def forward(ctx, q, k, cos, sin, positions, meta):
        from .backend import get_backend

        # (q comes first: where autograd rewrites the history of a VIEW modified in place it takes the view for input 0)
        tensors = (q,) if k is None else (q, k)
        pm, interleaved, rot_offset, inplace = meta
        ctx.meta = meta
        ctx.save_for_backward(cos, sin, positions)
        ctx.set_materialize_grads(False)
        if inplace:
            ctx.mark_dirty(*tensors)
            outs = list(tensors)
        else:
            outs = [torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in tensors]
        srcs = [t if _conforms(t) else t.contiguous() for t in tensors]        # (inplace: checked to conform before)
        get_backend().rotary(srcs, outs, cos, sin, positions=positions, pos_map=pm, interleaved=interleaved,
                             rot_offset=rot_offset, conj=False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        from .backend import get_backend

        cos, sin, positions = ctx.saved_tensors
        pm, interleaved, rot_offset, _ = ctx.meta
        live = [g for g in grads if g is not None]
        if live:
            srcs = [g if _conforms(g) else g.contiguous() for g in live]
            outs = [torch.empty(g.shape, dtype=g.dtype, device=g.device) for g in live]
            get_backend().rotary(srcs, outs, cos, sin, positions=positions, pos_map=pm, interleaved=interleaved,
                                 rot_offset=rot_offset, conj=True)
            it = iter(outs)
            grads = tuple(next(it) if g is not None else None for g in grads)
        return (grads[0], grads[1] if len(grads) > 1 else None, None, None, None, None)


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
    tensors = [q] if k is None else [q, k]
    packed, D = _check_qk(who, q, k)
    positions, pm, interleaved, rot_offset = _check_tables_positions(who, q, packed, D, cos, sin, layout, group, positions, offset,
                                                                      interleaved, rot_offset)
    inplace = bool(inplace)
    if inplace and not all(_conforms(t) for t in tensors):
        raise ValueError(f"{who}: inplace=True needs last stride 1, a 16-byte aligned start and strides that are multiples of 8")
    meta = (pm, interleaved, rot_offset, inplace)
    if inplace and k is not None and torch.is_grad_enabled() and any(t._is_view() for t in tensors):
        # (autograd lets a Function that modifies a VIEW in place return one tensor only: q and k one after the other — the
        #  bits do not depend on it)
        return tuple(_Rotary.apply(t, None, cos, sin, positions, meta)[0] for t in tensors)
    outs = _Rotary.apply(q, k, cos, sin, positions, meta)
    return outs[0] if k is None else outs


apply_rotary = _opaque(apply_rotary)
