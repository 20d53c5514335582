"""Small helpers shared by the schedule modules."""

def packed_pair(k, v):
    """the contiguous (..., 2, Hk, D) tensor whose slices [..., 0, :, :] / [..., 1, :, :] k and v are (the `kv`
    argument of the kvpacked entry points and its gradient), or None"""
    import torch
    if (k.dim() < 3 or k.shape != v.shape or k.stride() != v.stride() or k.dtype != v.dtype or k.device != v.device
            or k.untyped_storage().data_ptr() != v.untyped_storage().data_ptr()):
        return None
    hk, d = k.shape[-2], k.shape[-1]
    lead = tuple(k.shape[:-2])
    want = [d, 1]
    run = 2 * hk * d
    for n in reversed(lead):
        want.insert(0, run)
        run *= n
    if tuple(k.stride()) != tuple(want) or v.storage_offset() - k.storage_offset() != hk * d:
        return None
    strides = tuple(want[:-2]) + (hk * d, d, 1)
    return torch.as_strided(k, lead + (2, hk, d), strides, k.storage_offset())


def out_shape(q, v):
    """the shape of attention's output: q's rows and heads, v's head dim (they differ for MLA: 192 / 128)"""
    return tuple(q.shape[:-1]) + (v.shape[-1],)


def _prep_qkv(q, k, v, group, packed_travel=False):
    """Kernels take strided views (last stride 1, 16-byte aligned rows).  K/V only have to be
    contiguous when they travel (world_size > 1: they are RCCL send buffers), so the packed
    `kv[:, :, 0]` views of the benchmark are not copied on a single GPU — nor on several when the schedule moves
    the packed tensor as ONE buffer (packed_travel: the zigzag gather form)."""
    from .utils import group_rank_world, single_rank
    travels = not single_rank(group_rank_world(group)[1])
    if travels and packed_travel and packed_pair(k, v) is not None:
        travels = False
    if q.stride(-1) != 1:
        q = q.contiguous()
    if travels or k.stride(-1) != 1:
        k = k.contiguous()
    if travels or v.stride(-1) != 1:
        v = v.contiguous()
    return q, k, v


def global_window(window_size, causal, total):
    """The sides of `window_size` that cut something in a sequence of `total` rows, as (left, right) with -1 for a side
    that does not, or None when neither does: a window that covers the whole sequence is dropped on the host, so that
    such a call takes the unwindowed code path bit for bit.  `causal` bounds the right side itself (flash_attn: it
    forces window_right = 0), so the right side of the window is then never needed."""
    if window_size is None:
        return None
    wl, wr = int(window_size[0]), int(window_size[1])
    if wl < 0 or wl >= total - 1:
        wl = -1
    if causal or wr < 0 or wr >= total - 1:
        wr = -1
    return None if wl < 0 and wr < 0 else (wl, wr)


def require_mask_shift(be, what):
    """A windowed call over several ranks needs a backend that can be told where a block sits in the full sequence
    (`mask_shift`, include/rfa.h: HipBackend.serves_mask_shift).  One that cannot would band every block on its own, which
    is wrong: refuse before anything is exchanged, on every rank alike."""
    if not getattr(be, "serves_mask_shift", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with a sliding window on a multi-rank group needs a backend "
                                  f"that serves `mask_shift`; {getattr(be, 'name', type(be).__name__)!r} does not (it would "
                                  "apply the window per block)")


def require_mask_shift_lens(be, what):
    """The packed (varlen) counterpart of require_mask_shift: the lengths of packed sequences differ, so a block's place
    in the full sequences is a multiple of every sequence's own length (`mask_shift_lens`, include/rfa.h:
    HipBackend.serves_mask_shift_lens).  Refused before anything is exchanged, on every rank alike."""
    if not getattr(be, "serves_mask_shift_lens", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with a sliding window on a multi-rank group needs a backend "
                                  f"that serves `mask_shift_lens`; {getattr(be, 'name', type(be).__name__)!r} does not (it "
                                  "would apply the window per block)")


def require_alibi(be, what):
    """A call with alibi_slopes needs a backend that adds the bias inside its kernels (`alibi=` of fwd / bwd, include/rfa.h:
    rfa_ext_args; HipBackend.serves_alibi).  One that cannot would drop the bias silently: refuse before anything is
    exchanged, on every rank alike."""
    if not getattr(be, "serves_alibi", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with alibi_slopes needs a backend that serves `alibi`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not (it would ignore the bias)")


def check_alibi_slopes(alibi_slopes, q, batch):
    """alibi_slopes as the kernels take them — fp32, on q's device, (H,) or (batch, H) with H = q's heads, innermost stride
    1 — or None; ValueError otherwise.  Validated once per public call (flash_attn's contract: alibi_slopes is fp32)."""
    if alibi_slopes is None:
        return None
    import torch
    H = q.shape[-2]
    if (not torch.is_tensor(alibi_slopes) or alibi_slopes.dtype != torch.float32 or alibi_slopes.device != q.device
            or tuple(alibi_slopes.shape) not in ((H,), (batch, H))):
        raise ValueError(f"ring_flash_attn: alibi_slopes must be a float32 tensor of shape ({H},) or ({batch}, {H}) on "
                         f"{q.device}; got {getattr(alibi_slopes, 'dtype', type(alibi_slopes))} "
                         f"{tuple(getattr(alibi_slopes, 'shape', ()))} on {getattr(alibi_slopes, 'device', None)}")
    return alibi_slopes.detach().contiguous()


def alibi_kw(alibi_slopes, shift=0, heads=None):
    """the `alibi=` keyword of a block call whose q row 0 sits `shift` rows behind its k row 0 in the full sequence
    (include/rfa.h: alibi_shift), for the query heads `heads` (a slice: a head group's slopes are a view); nothing without
    slopes, so that backends that predate the keyword keep serving unbiased calls"""
    if alibi_slopes is None:
        return {}
    if heads is not None:
        alibi_slopes = alibi_slopes[..., heads]
    return {"alibi": (alibi_slopes, int(shift))}


def row_ranges_kw(row_ranges, k_pos0, rows=None):
    """the `row_ranges=` keyword of a block call whose key row 0 sits at global position `k_pos0`, for the query rows `rows`
    (a slice of this rank's rows: the ranges are views) — ring_flash_attn.with_row_ranges; nothing without ranges, so that
    backends that predate the keyword keep serving plain calls"""
    if row_ranges is None:
        return {}
    start, end = row_ranges[:2]
    if rows is not None:
        start, end = start[:, rows], end[:, rows]
    return {"row_ranges": (start, end, int(k_pos0))}


def block_mask_kw(block_mask, k_blk0, qblocks=None):
    """the `block_mask=` keyword of a block call whose key row 0 sits in mask column `k_blk0` (global key position / 128), for
    the query blocks `qblocks` (a slice of this rank's rows of the mask: a view, its strides go to the library) —
    ring_flash_attn.with_block_mask; nothing without a mask, so that backends that predate the keyword keep serving plain calls"""
    if block_mask is None:
        return {}
    mask = block_mask[0] if isinstance(block_mask, tuple) else block_mask
    if qblocks is not None:
        mask = mask[:, :, qblocks]
    return {"block_mask": (mask, int(k_blk0))}


def dlse_kw(dlse):
    """the `dlse=` keyword of a backward's bwd_preprocess (the gradient of lse, ring_flash_attn.with_lse_grad); nothing
    without one, so that backends that predate the keyword keep serving plain calls"""
    return {} if dlse is None else {"dlse": dlse}


def _as_cu(cu_seqlens, device):
    """cu_seqlens as an int32 tensor on the compute device (the kernels read it on device)."""
    import torch
    if not torch.is_tensor(cu_seqlens):
        cu_seqlens = torch.tensor(cu_seqlens, dtype=torch.int32)
    if cu_seqlens.dtype != torch.int32:
        cu_seqlens = cu_seqlens.to(torch.int32)
    if cu_seqlens.device != device:
        cu_seqlens = cu_seqlens.to(device)
    return cu_seqlens.contiguous()


def require_dropout_positions(be, what):
    """Dropout over several ranks needs a backend that can be told where the rows of a block sit in the full sequence
    even when they are not one contiguous run (the position maps of `dropout=`, include/rfa.h: q_pos_stride ...;
    HipBackend.serves_dropout_positions).  One that cannot would draw another mask than the unsharded call — and, in the
    backward of a block whose keys came from another rank, another mask than that rank's forward: refuse before anything
    is exchanged, on every rank alike.  The contiguous ring asks for it too, although offsets alone would serve it, so
    that one flag tells whether a backend serves dropout over a multi-rank group."""
    if not getattr(be, "serves_dropout_positions", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with dropout on a multi-rank group needs a backend that serves "
                                  f"dropout position maps; {getattr(be, 'name', type(be).__name__)!r} does not (it would "
                                  "draw the mask per block)")


IDENTITY_MAP = (1, 0, 0)


def pos_map(offset=0, stride=1, split=0, offset2=0):
    """(offset, (stride, split, offset2)) of a tensor whose local row i is global position
    `offset + i * stride` for i < split (or split == 0), `offset2 + (i - split) * stride` from row `split` on"""
    return int(offset), (int(stride), int(split), int(offset2))


def map_positions(pm, n):
    """the global positions of local rows 0 .. n-1 under pos_map `pm` (tests, documentation: the kernels' arithmetic)"""
    off, (stride, split, off2) = pm
    stride = stride or 1
    return [off + i * stride if (split == 0 or i < split) else off2 + (i - split) * stride for i in range(n)]


def zigzag_map(x, W, c, part="all"):
    """pos_map of rank x's zigzag tensor with chunk length c: chunks x and 2W-1-x of the sequence (part "all"), its
    front chunk alone ("front": `k[:, :c]`) or its back chunk alone ("back": `q[:, c:]`)"""
    if part == "front":
        return pos_map(x * c)
    if part == "back":
        return pos_map((2 * W - 1 - x) * c)
    return pos_map(x * c, 1, c, (2 * W - 1 - x) * c)


def stripe_map(x, W, skip=0):
    """pos_map of rank x's stripe tensor (local row i is global token i W + x), `skip` leading rows sliced off"""
    return pos_map(x + skip * W, W)


def dropout_arg(dropout_p, dropout_seed, q_pos_offset=0, k_pos_offset=0, head_offset=0, q_map=None, k_map=None):
    """backend `dropout=` argument (p, seed, q_pos_offset, k_pos_offset, head_offset), or None when dropout is off.
    The seed comes from the autograd Function (one draw per forward, reused by its backward).
    q_map / k_map: a pos_map() each, for tensors whose rows are not one contiguous run of the global sequence; they
    replace the offsets.  When both are the identity (stride 1, one piece) the result is the 5-tuple every backend
    serves; otherwise the 7-tuple (..., (stride, split, offset2) of q, of k) that needs `serves_dropout_positions`."""
    if not dropout_p or not dropout_p > 0:
        return None
    if dropout_seed is None:
        raise ValueError("ring_flash_attn: dropout_p > 0 needs a dropout_seed (the public functions draw one)")
    qm = km = IDENTITY_MAP
    if q_map is not None:
        q_pos_offset, qm = q_map
    if k_map is not None:
        k_pos_offset, km = k_map
    qm, km = ((m[0] or 1, m[1], m[2] if m[1] else 0) for m in (qm, km))
    base = (float(dropout_p), int(dropout_seed), int(q_pos_offset), int(k_pos_offset), int(head_offset))
    if qm == IDENTITY_MAP and km == IDENTITY_MAP:
        return base
    return base + (qm, km)


_DROPOUT_SOURCE = {"generator": None, "group": None, "sync": False}


def set_dropout_generator(generator=None, sync_group=None, sync=False):
    """Where the per-forward dropout seeds come from.  Default (generator=None): torch's default CPU generator, like
    any torch random op — reproducible under torch.manual_seed, but it advances the stream data loaders and
    initialisers share, and the documented "sharded mask == unsharded mask" property then needs every rank of a context-
    parallel group to have seeded alike.  With a dedicated `torch.Generator` the global stream is left alone; with
    `sync=True` every draw is additionally broadcast from rank 0 of `sync_group` (one 8-byte broadcast per forward), so
    the ranks agree whatever their seeds (frameworks that seed per rank).  INTEGRATION.md, "Dropout"."""
    _DROPOUT_SOURCE.update(generator=generator, group=sync_group, sync=bool(sync))


def draw_dropout_seed() -> int:
    """one 62-bit seed per forward: from torch's default CPU generator (reproducible under torch.manual_seed; ranks
    that seeded alike draw alike, which makes the mask of a sharded call equal to the unsharded one — include/rfa.h), or
    from the source installed with set_dropout_generator()"""
    import torch
    src = _DROPOUT_SOURCE
    seed = torch.randint(0, 2 ** 62, (1,), generator=src["generator"])
    if src["sync"]:
        import torch.distributed as dist

        if dist.get_backend(src["group"]) != "gloo":           # RCCL broadcasts device memory
            seed = seed.cuda()
        dist.broadcast(seed, dist.get_global_rank(src["group"], 0) if src["group"] is not None else 0, group=src["group"])
    return int(seed.item())
