"""Public-API factory: one autograd Function + the (func, kvpacked_func, qkvpacked_func)
trio per algorithm, generated from its `*_forward` / `*_backward` schedule.

The generated callables keep the exact keyword surface of the reference package
(/root/reference/ring_flash_attn/__init__.py:1-35 and SURVEY.md Appendix A):
    dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), alibi_slopes=None,
    deterministic=False, return_attn_probs=False, group=None
with the reference's semantics: softmax_scale None -> head_dim ** -0.5; alibi_slopes (flash_attn's: fp32, (H,) or
(B, H)) works on single-rank groups with every function and over several ranks with the dense ring and zigzag schedules and
with causal llama3 (not together with a window or dropout, head dims <= 128); dropout_p works on single-rank groups, on the llama3 path and over several ranks with the dense ring, zigzag and
stripe schedules (the reference declares dropout over a ring unsupported, README.md:158-159; the `*_varlen` ring families
still raise here); window_size works with every schedule; the two together raise;
return_attn_probs=True -> (out, softmax_lse, None); `group=None` is the default process group;
inputs are the caller's LOCAL shard.
"""
import torch

from ._common import _prep_qkv, _as_cu, check_alibi_slopes, draw_dropout_seed, require_alibi
from .backend import softcap_scope
from .utils import audit_verify


def _opaque(fn):
    """The schedules are ctypes calls into librfa_hip.so interleaved with torch.distributed traffic, which dynamo
    cannot trace: behind `torch.compiler.disable` a compiled caller graph-breaks around them and runs them
    eagerly, with identical results (multi-rank groups; llama3)."""
    try:
        import functools

        wrapped = torch.compiler.disable(fn)
        functools.update_wrapper(wrapped, fn)
        return wrapped
    except Exception:        # very old torch without torch.compiler
        return fn


def _single_rank(group) -> bool:
    import torch.distributed as dist

    return dist.get_world_size(group) == 1


def _compilable(fn, lower, multi=None):
    """Public callable = `fn` (eager: the autograd Functions above, opaque to dynamo) except while dynamo is
    TRACING it on a single-rank group: then `lower(...)` expresses the call with the registered custom
    operators (_ops.py: rfa::attn_fwd / rfa::attn_bwd, fake kernels + autograd formula), so `torch.compile`
    captures the operator in its graph instead of breaking it (the reference runs its tests a second time under
    torch.compile: test/test.sh:23-25).  `multi(...)`, where the schedule has one: the same for a multi-rank group —
    the whole schedule as one operator per direction (_ops.py: rfa::sched_fwd / rfa::sched_bwd)."""
    import functools

    eager = _opaque(fn)

    import inspect

    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def public(*args, **kwargs):
        if torch.compiler.is_compiling():
            # `group` may be passed positionally: resolve it the way the call itself would
            bound = sig.bind(*args, **kwargs).arguments
            # (a value head dim of its own runs eagerly too: the registered operators' fake kernels assume out like q)
            if "v" in bound and "q" in bound and bound["v"].shape[-1] != bound["q"].shape[-1]:
                return eager(*args, **kwargs)
            # (dropout draws a host-side seed per call: such calls run eagerly behind a graph break)
            # (a bias runs the eager autograd path too: the registered operators have no biased form)
            if not bound.get("dropout_p", 0.0) and bound.get("alibi_slopes", None) is None:
                if _single_rank(bound.get("group", None)):
                    return lower(*args, **kwargs)
                # several ranks: the whole schedule as one registered operator (_ops.py: rfa::sched_fwd / sched_bwd),
                # where the schedule has one — windowed calls and llama3 keep the eager path behind a graph break
                if multi is not None and not has_window(bound.get("window_size", (-1, -1))):
                    return multi(*args, **kwargs)
        return eager(*args, **kwargs)

    return public


def _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=False, dropout_ok=None, alibi_ok=False):
    """Sliding windows and dropout are implemented in the kernels (flash_attn semantics; dropout: the counter-based
    mask of include/rfa.h).  Dropout is usable wherever ONE kernel call sees all the keys a query may attend to: every
    function on a single-rank group, and llama3_flash_attn_varlen_func on any group (it gathers K/V) — the coverage the
    reference gets from forwarding dropout_p to flash_attn (llama3_flash_attn_varlen.py:131-147); it declares dropout
    over a ring unsupported (README.md:158-159).  Here the dense ring, zigzag (every exchange form) and stripe schedules
    serve it on any group as well: the mask is a function of global positions, and those schedules tell every block
    call where its rows sit (the position maps of `dropout=`, _common.dropout_arg), so the un-sharded result is the
    single-device dropout call's with the same seed; they pass dropout_ok=True.  The two `*_varlen` ring families
    (position maps for packed input do not exist) and the `torch.compile` whole-schedule operator still raise.
    Windows are usable there too, and on any
    group with every ring schedule, each of which tells every block call where it sits in the full sequence: the dense
    ring and zigzag schedules in rows (`mask_shift`, include/rfa.h), the two `*_varlen` ring families in units of every
    packed sequence's own length (`mask_shift_lens`), the stripe schedule — token i of rank r is global token i W + r —
    as a dense shifted band in local rows.  These schedules pass windows_ok=True for such calls; windows_ok=False (the
    `torch.compile` whole-schedule operator, which has no windowed form) still raises.
    Dropout together with a window is not available anywhere.
    ALiBi (alibi_slopes) is implemented in the kernels as well (include/rfa.h: rfa_ext_args).  The bias is a function of
    the GLOBAL distance i - j, so it is usable wherever ONE call sees whole sequences (every function on a single-rank group)
    and wherever the schedule tells every block call where it sits (`alibi_shift`): the dense ring (the block at signed rank
    distance t: t S), the zigzag schedule (per chunk pair, (cq - ck) C) and causal llama3 (bottom-right alignment against
    the truncated cu_seqlens_k IS the global distance); those pass alibi_ok=True.  Everything else — stripe, the *_varlen
    ring families and zigzag_llama3 over several ranks, non-causal llama3 over several ranks, the torch.compile operators
    — raises, as does a bias together with a window or dropout."""
    if dropout_ok is None:
        dropout_ok = windows_ok
    drop = bool(dropout_p) and dropout_p > 0
    if drop and not 0 < dropout_p < 1:
        raise ValueError("dropout_p must be in [0, 1)")
    if drop and not dropout_ok:
        raise NotImplementedError("ring_flash_attn: dropout over a multi-rank group is served by the dense ring, zigzag "
                                  "and stripe functions and by llama3_flash_attn_varlen_func, not by the *_varlen ring "
                                  "functions (position maps for packed input are not implemented) nor under "
                                  "torch.compile's whole-schedule operator; use one of those or a single-rank group")
    if not windows_ok and has_window(window_size):
        raise NotImplementedError("ring_flash_attn: sliding window over a multi-rank group is served by the eager ring, "
                                  "zigzag, stripe and *_varlen ring functions and by llama3_flash_attn_varlen_func, not "
                                  "by this entry (the whole-schedule operator has no windowed form)")
    if drop and has_window(window_size):
        raise NotImplementedError("ring_flash_attn: dropout together with a sliding window is not supported")
    if alibi_slopes is not None:
        if not alibi_ok:
            raise NotImplementedError("ring_flash_attn: alibi_slopes over a multi-rank group is served by the eager dense "
                                      "ring and zigzag functions and by causal llama3_flash_attn_varlen_func, not by this "
                                      "entry (stripe, the *_varlen ring functions, zigzag_llama3, non-causal llama3 and "
                                      "torch.compile's operators have no biased form); use one of those or a single-rank group")
        if drop or has_window(window_size):
            raise NotImplementedError("ring_flash_attn: alibi_slopes together with dropout or a sliding window is not supported")


def checked_alibi(alibi_slopes, q, batch, what):
    """alibi_slopes validated once per public call (ValueError: _common.check_alibi_slopes) and the refusals that need the
    tensors: head dims above 128 and a backend that does not serve a bias — NotImplementedError, before anything is
    exchanged, on every rank alike.  None stays None."""
    if alibi_slopes is None:
        return None
    slopes = check_alibi_slopes(alibi_slopes, q, batch)
    if q.shape[-1] > 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with alibi_slopes serves head dims up to 128, not {q.shape[-1]}")
    from .backend import get_backend

    require_alibi(get_backend(), what)
    return slopes


def checked_softcap(dropout_p, alibi_slopes, q, what, window_size=None, causal=False):
    """the soft cap bound to this public call by `with_softcap` (0.0: none) and its refusals — together with dropout or
    alibi_slopes, head dims above 128, a window at head dims 65 .. 127 (include/rfa.h: that dK/dV instance is not built; a
    window_size (-1, 0) with `causal` bounds nothing), a backend that does not serve a cap: NotImplementedError before anything is
    exchanged, on every rank alike.  Read ONCE, in the autograd Function's forward, and kept on the node: the backward runs
    under `softcap_scope(ctx.softcap)` and reads nothing ambient."""
    from .backend import get_backend, pending_softcap, softcap_scope

    cap = pending_softcap()
    if not cap:
        return 0.0
    if dropout_p and dropout_p > 0:
        raise NotImplementedError(f"ring_flash_attn: {what} with softcap together with dropout is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError(f"ring_flash_attn: {what} with softcap together with alibi_slopes is not supported")
    if q.shape[-1] > 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with softcap serves head dims up to 128, not {q.shape[-1]}")
    bounded = has_window(window_size) and (window_size[0] >= 0 or not causal)
    if bounded and 64 < q.shape[-1] < 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with softcap and a sliding window serves head dims up to 64 "
                                  f"and 128, not {q.shape[-1]}")
    with softcap_scope(cap):
        get_backend()                                # (refuses a backend without `serves_softcap`)
    return cap


VDIM_QK = (136, 192)      # QK head dims served next to a value head dim of its own (csrc/rfa_vdim.hip) ...
VDIM_V = (8, 128)         # ... and the value head dims


def checked_vdim(q, k, v, dropout_p, alibi_slopes, what, served=True):
    """A `v` whose head dim differs from q's (multi-head latent attention: 192 / 128), decided once per public call, on every
    rank alike, before anything is exchanged.  Equal widths: nothing to check.  ValueError: v's leading dims differ from k's,
    a value head dim that is no multiple of 8.  NotImplementedError: a (D, Dv) pair outside QK head dims 136 .. 192 and value
    head dims 8 .. 128, dropout, alibi_slopes, a function that does not serve it (`served` False: the llama3 families and
    with_ulysses move K and V in one buffer of one width), a backend without `serves_vdim`."""
    D, Dv = q.shape[-1], v.shape[-1]
    if Dv == D:
        return False
    if tuple(v.shape[:-1]) != tuple(k.shape[:-1]):
        raise ValueError(f"ring_flash_attn: {what}: v {tuple(v.shape)} must have k's leading dims {tuple(k.shape[:-1])}")
    if Dv % 8:
        raise ValueError(f"ring_flash_attn: {what}: the value head dim must be a multiple of 8, got {Dv}")
    if not served:
        raise NotImplementedError(f"ring_flash_attn: {what} does not serve a value head dim ({Dv}) that differs from q's ({D}): "
                                  "K and V travel in one buffer of one width there; the ring, zigzag and stripe functions "
                                  "and their *_varlen forms do")
    if not (VDIM_QK[0] <= D <= VDIM_QK[1] and VDIM_V[0] <= Dv <= VDIM_V[1]):
        raise NotImplementedError(f"ring_flash_attn: {what} serves a value head dim of its own for QK head dims {VDIM_QK[0]} .. "
                                  f"{VDIM_QK[1]} and value head dims {VDIM_V[0]} .. {VDIM_V[1]}, not ({D}, {Dv})")
    if dropout_p and dropout_p > 0:
        raise NotImplementedError(f"ring_flash_attn: {what} with dropout and a value head dim that differs from q's is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError(f"ring_flash_attn: {what} with alibi_slopes and a value head dim that differs from q's is not supported")
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_vdim", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with a value head dim that differs from q's needs a backend that "
                                  f"serves it (serves_vdim); {getattr(be, 'name', type(be).__name__)!r} does not")
    return True


def with_softcap(func, softcap):
    """flash_attn's logit soft-capping for one of this package's public attention functions:

        capped = with_softcap(ring_flash_attn_func, 50.0)
        out = capped(q, k, v, causal=True, window_size=(4095, 0))

    returns a callable with `func`'s signature that runs `func` with scores = softcap * tanh(softmax_scale * q.k / softcap)
    in front of the mask and the softmax (include/rfa.h: rfa_ext_args.softcap), on any group and with any window the
    function serves.  `softcap` None or 0: `func` itself.  ValueError: a negative or non-finite value; TypeError: `func` is
    not one of the public attention functions.  NotImplementedError at the call: together with dropout or alibi_slopes,
    head dims above 128, and (windowed calls) head dims 65 .. 127.
    The value is bound to the call and kept on the autograd node — activation checkpointing re-runs the wrapped call and
    gets the same cap; there is no user-managed context.  Under torch.compile the capped call runs eagerly behind a graph
    break (the registered operators have no capped form)."""
    import functools

    import ring_flash_attn as pkg
    from .backend import check_softcap, softcap_scope

    public = {id(getattr(pkg, n)): n for n in dir(pkg) if n.endswith("_func")}
    if id(func) not in public:
        raise TypeError("ring_flash_attn.with_softcap: `func` must be one of the package's public attention functions "
                        f"(ring_flash_attn.*_func), got {func!r}")
    cap = check_softcap(softcap)
    if not cap:
        return func

    # (updated=(): `func`'s own attributes are not copied — a function that is already opaque to dynamo carries the marker
    #  that makes torch.compiler.disable unwrap to ITS original, which would drop this wrapper)
    @functools.wraps(func, updated=())
    def capped(*args, **kwargs):
        with softcap_scope(cap):
            return func(*args, **kwargs)

    capped._rfa_softcap = cap                        # (with_sinks refuses to wrap a capped function)
    return _opaque(capped)


# ---- a gradient for the returned lse (ring_flash_attn.with_lse_grad) ------------------------------------------------------
# lse_i = log sum_j exp(s_ij), so d lse_i / d s_ij = P_ij: a gradient g_i on lse_i adds g_i P_ij to dS = P (dP - delta).  Every
# backward kernel is therefore served, unchanged, by delta' = delta - g (include/rfa.h: rfa_bwd_preprocess_lse): the ONE place a
# schedule's backward computes delta takes `dlse=`.  The binding is read once, at the public entry of the forward, and kept on
# the node (ctx.lse_grad); a backward reads ctx and the gradients autograd hands it, nothing ambient.  An unbound node is the
# node it always was: it never looks at the gradient of lse.
import contextvars

_lse_grad = contextvars.ContextVar("ring_flash_attn_lse_grad", default=False)


def checked_lse_grad(ctx, what):
    """True inside a call bound by `with_lse_grad` — the node then takes undefined output gradients as None (an unused lse costs
    nothing and leaves the plain backward, bit for bit).  NotImplementedError: a backend whose bwd_preprocess does not take
    `dlse=` — before anything is exchanged, on every rank alike."""
    if not _lse_grad.get():
        return False
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_lse_grad", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with a gradient for lse needs a backend that serves `lse_grad` "
                                  f"(bwd_preprocess(dlse=)); {getattr(be, 'name', type(be).__name__)!r} does not")
    ctx.set_materialize_grads(False)
    return True


def lse_grad_kw(ctx, dout, args, out, lse):
    """(dout, the `dlse=` keyword of the schedule's backward) from what autograd handed a node's backward: an unbound node
    passes dout through and no keyword; a bound one replaces an undefined dout (a loss that uses lse alone) by zeros in out's
    dtype and passes the gradient of lse — fp32, in lse's layout, contiguous — when there is one"""
    if not getattr(ctx, "lse_grad", False):
        return dout, {}
    if dout is None:
        dout = torch.zeros_like(out)
    dlse = args[0] if args else None
    if dlse is None:
        return dout, {}
    if tuple(dlse.shape) != tuple(lse.shape):
        raise ValueError(f"ring_flash_attn: the gradient of lse has shape {tuple(dlse.shape)}, lse has {tuple(lse.shape)}")
    return dout, {"dlse": dlse.to(torch.float32).contiguous()}


def with_lse_grad(func):
    """A differentiable `lse` for one of this package's public attention functions:

        attn = with_lse_grad(zigzag_ring_flash_attn_func)
        out, lse, _ = attn(q, k, v, causal=True, return_attn_probs=True)
        loss = f(out) + 1e-4 * lse.square().mean()               # e.g. a z-loss on the attention normaliser

    returns a callable with `func`'s signature whose returned lse carries its gradient into dq and dk (dv does not depend on
    lse) — exactly: the backward kernels get delta' = rowsum(dout * out) - dlse in place of delta, at the cost of 4 more bytes
    read per row and head.  That makes (out, lse) the handle by which attention over two key sets composes, backward included:
    `merge_attn` of two such calls is attention over the union of their keys.  A plain call's lse also leaves the autograd node,
    but its gradient is dropped.
    Served: the 21 `*_func` of the package and `with_softcap` results of them, on any group and with everything `func` serves
    there — windows, packed input, GQA, alibi_slopes, dropout (lse is the undropped softmax's).  `dlse` belongs to the rank
    that owns the query rows; no collective is added.  TypeError: any other callable — `with_sinks` results (the sinks'
    gradient needs the same term: follow-up), `with_max_logit`, `with_ulysses` and `with_lse_grad` results (bind with_lse_grad
    first: the other binders refuse its result as well).  NotImplementedError at the call, before anything is exchanged: a
    backend that does not serve it.  An lse that the loss does not use costs nothing: the backward is the plain one, bit for
    bit; a loss that uses lse alone is served too.  Double backward is not.  Under torch.compile the call runs eagerly behind a
    graph break."""
    import functools

    import ring_flash_attn as pkg

    for marker, what in (("_rfa_lse_grad", "with_lse_grad"), ("_rfa_sinks", "with_sinks"), ("_rfa_max_logit", "with_max_logit"),
                         ("_rfa_ulysses", "with_ulysses")):
        if getattr(func, marker, False):
            raise TypeError(f"ring_flash_attn.with_lse_grad: `func` is a {what} result; not served")
    public = {id(getattr(pkg, n)): n for n in dir(pkg) if n.endswith("_func")}
    f = func
    while id(f) not in public and getattr(f, "_rfa_softcap", None) and hasattr(f, "__wrapped__"):
        f = f.__wrapped__                            # (a with_softcap result leads to the public function it wraps)
    if id(f) not in public:
        raise TypeError("ring_flash_attn.with_lse_grad: `func` must be one of the package's public attention functions "
                        f"(ring_flash_attn.*_func) or a with_softcap result of one, got {func!r}")

    @functools.wraps(func, updated=())              # (updated=(): as in with_softcap; the cap's marker is NOT carried over)
    def bound(*args, **kwargs):
        token = _lse_grad.set(True)
        try:
            return func(*args, **kwargs)
        finally:
            _lse_grad.reset(token)

    bound._rfa_lse_grad = True
    return _opaque(bound)


# ---- per-row key ranges (ring_flash_attn.with_row_ranges) -----------------------------------------------------------------
# Row i sees key j iff start[i] <= pos(j) < end[i] and the call's own mask allows the pair: one interval of GLOBAL key positions
# per query row (FlashMask's O(S) description of document, prefix-LM, shared-prefix masks ...).  The two tensors are bound to
# the call like the gradient of lse above: read ONCE, in the autograd Function's forward, kept on the node (ctx.row_ranges) and
# handed to the schedule's forward and backward as `row_ranges=` — a backward reads nothing ambient.  The schedules give every
# block call the slice that belongs to its query rows and the global position of its key row 0 (include/rfa.h: rfa_rowrange_args).
_row_ranges = contextvars.ContextVar("ring_flash_attn_row_ranges", default=None)

ROW_RANGE_FUNCS = tuple(f"{p}_{s}" for p in ("ring_flash_attn", "zigzag_ring_flash_attn") for s in ("func", "kvpacked_func", "qkvpacked_func"))


def _check_row_range_tensors(start, end, q=None):
    """ValueError unless start and end are contiguous int32 2-d tensors of one shape on one device — and, given the call's q,
    (B, S_local) on q's device"""
    for nm, t in (("start", start), ("end", end)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous():
            got = f"{tuple(t.shape)} {t.dtype}, contiguous={t.is_contiguous()}" if isinstance(t, torch.Tensor) else repr(t)
            raise ValueError(f"ring_flash_attn.with_row_ranges: {nm} must be a contiguous int32 tensor of shape (B, S_local); got {got}")
    if start.shape != end.shape or start.device != end.device:
        raise ValueError(f"ring_flash_attn.with_row_ranges: start {tuple(start.shape)} on {start.device} and end "
                         f"{tuple(end.shape)} on {end.device} must have one shape and device")
    if q is not None and (tuple(start.shape) != tuple(q.shape[:2]) or start.device != q.device):
        raise ValueError(f"ring_flash_attn.with_row_ranges: start / end must be {tuple(q.shape[:2])} on {q.device} — one entry "
                         f"per local query row; got {tuple(start.shape)} on {start.device}")


def checked_row_ranges(q, k, v, dropout_p, alibi_slopes, what):
    """(start, end) bound to this public call by `with_row_ranges`, or None.  ValueError: tensors that do not fit q.
    NotImplementedError — before anything is exchanged, on every rank alike: dropout, alibi_slopes, head dims above 128, a value
    head dim of its own, a backend without `serves_row_ranges`."""
    rr = _row_ranges.get()
    if rr is None:
        return None
    _check_row_range_tensors(rr[0], rr[1], q)
    if dropout_p and dropout_p > 0:
        raise NotImplementedError(f"ring_flash_attn: {what} with row ranges together with dropout is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError(f"ring_flash_attn: {what} with row ranges together with alibi_slopes is not supported")
    if q.shape[-1] > 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with row ranges serves head dims up to 128, not {q.shape[-1]}")
    if v.shape[-1] != q.shape[-1]:
        raise NotImplementedError(f"ring_flash_attn: {what} with row ranges does not serve a value head dim ({v.shape[-1]}) "
                                  f"that differs from q's ({q.shape[-1]})")
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_row_ranges", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with row ranges needs a backend that serves `row_ranges` "
                                  f"(serves_row_ranges); {getattr(be, 'name', type(be).__name__)!r} does not")
    return rr


def row_ranges_extra(ctx):
    """the `row_ranges=` keyword of the schedule's forward / backward of a bound node; nothing for an unbound one"""
    rr = getattr(ctx, "row_ranges", None)
    return {} if rr is None else {"row_ranges": rr}


def with_row_ranges(func, start, end):
    """One interval of keys per query row — document masks on dense (zigzag-balanced) input, prefix-LM and image-bidirectional
    masks, shared prefixes — for the dense ring and zigzag functions:

        attn = with_row_ranges(zigzag_ring_flash_attn_func, start, end)     # int32 (B, S_local), contiguous, on q's device
        out = attn(q, k, v, causal=False)

    returns a callable with `func`'s signature and return value in which query row i sees key j iff
    start[b, i] <= pos(j) < end[b, i] AND the call's own mask (`causal`, `window_size`) allows the pair.  start / end hold THIS
    rank's query rows in the order of q's rows; their values are GLOBAL key positions in the natural order of the unsharded
    sequence (0 .. W * S_local), not layout indices.  Values outside [0, total] are clamped; start >= end is an empty row
    (out = 0, lse = +inf, zero gradients); all query heads share the ranges; the ranges get no gradient, dq, dk, dv are exact.
    The kernels skip every key tile (forward, dQ) and every query tile (dK/dV) that no row's range reaches.  A zigzag call may
    be non-causal.  Unions of disjoint intervals compose through `with_lse_grad` and `merge_attn` (README).
    `start=None, end=None`: `func` itself.  Served: ring_flash_attn_{,kvpacked_,qkvpacked_}func and
    zigzag_ring_flash_attn_{,kvpacked_,qkvpacked_}func or a `with_lse_grad` result of one (with_row_ranges goes on the outside),
    on any group, with windows, GQA, return_attn_probs, bf16 / fp16.  TypeError: any other callable — the *_varlen, stripe_,
    llama3_ and zigzag_llama3_ families and with_softcap / with_sinks / with_max_logit / with_ulysses / with_row_ranges results.
    ValueError: only one of start / end; tensors that are not contiguous int32 (B, S_local) on q's device.  NotImplementedError at
    the call, before anything is exchanged: dropout_p > 0, alibi_slopes, head dims above 128, a value head dim of its own, a
    backend that does not serve it.  The tensors are bound to the call and kept on the autograd node — activation
    checkpointing re-runs the wrapped call and binds them again.  Under torch.compile the call runs eagerly behind a graph break."""
    import functools

    import ring_flash_attn as pkg

    for marker, what in (("_rfa_row_ranges", "with_row_ranges"), ("_rfa_softcap", "with_softcap"), ("_rfa_sinks", "with_sinks"),
                         ("_rfa_max_logit", "with_max_logit"), ("_rfa_ulysses", "with_ulysses")):
        if getattr(func, marker, False):
            raise TypeError(f"ring_flash_attn.with_row_ranges: `func` is a {what} result; not served")
    served = {id(getattr(pkg, n)) for n in ROW_RANGE_FUNCS}
    f = func
    # (a with_lse_grad result carries the marker on both of its layers and leads to the public function it wraps)
    while id(f) not in served and getattr(f, "_rfa_lse_grad", False) and hasattr(f, "__wrapped__"):
        f = f.__wrapped__
    if id(f) not in served:
        raise TypeError("ring_flash_attn.with_row_ranges: `func` must be one of ring_flash_attn_{,kvpacked_,qkvpacked_}func and "
                        f"zigzag_ring_flash_attn_{{,kvpacked_,qkvpacked_}}func or a with_lse_grad result of one, got {func!r}")
    if (start is None) != (end is None):
        raise ValueError("ring_flash_attn.with_row_ranges: start and end come together (both tensors, or both None)")
    if start is None:
        return func
    _check_row_range_tensors(start, end)

    @functools.wraps(func, updated=())              # (updated=(): as in with_softcap)
    def ranged(*args, **kwargs):
        token = _row_ranges.set((start, end))
        try:
            return func(*args, **kwargs)
        finally:
            _row_ranges.reset(token)

    ranged._rfa_row_ranges = True                    # (the other binders refuse a ranged function)
    return _opaque(ranged)


# ---- block-sparse masks (ring_flash_attn.with_block_mask) -----------------------------------------------------------------
# Local query block i sees key block j of the unsharded sequence iff block_mask[b or 0, h or 0, i, j] and the call's own mask
# allows the pair; blocks of BLOCK_MASK_SIZE = 128 positions.  Bound like the ranges above: read ONCE, in the autograd
# Function's forward, kept on the node (ctx.block_mask) and handed to the schedule's forward and backward as `block_mask=` — a
# backward reads nothing ambient.  The schedules give every block call the rows of the mask that belong to its query rows and
# the mask column of its key row 0 (include/rfa.h: rfa_blockmask_args).
from . import _C as _C_abi

BLOCK_MASK_SIZE = _C_abi.BLOCK_MASK_SIZE
BLOCK_MASK_MAX_GROUP = 64         # query heads per K/V head the dK/dV item walk holds in one window (csrc/rfa_kernels.hpp: kBmMaxGroup)
_block_mask = contextvars.ContextVar("ring_flash_attn_block_mask", default=None)


def _check_block_mask_tensor(mask):
    """ValueError unless the mask is a contiguous 4-d bool tensor"""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 4 or not mask.is_contiguous():
        got = f"{tuple(mask.shape)} {mask.dtype}, contiguous={mask.is_contiguous()}" if isinstance(mask, torch.Tensor) else repr(mask)
        raise ValueError(f"ring_flash_attn.with_block_mask: block_mask must be a contiguous bool tensor of shape (Bm, Hm, NQ, NK); got {got}")


def checked_block_mask(q, k, v, dropout_p, alibi_slopes, what, group):
    """the mask bound to this public call by `with_block_mask`, or None.  ValueError: a mask that does not fit the call, local
    lengths that are no multiple of the block on a multi-rank group.  NotImplementedError: dropout, alibi_slopes, head dims
    above 128, more than 64 query heads per K/V head, a value head dim of its own, a backend without `serves_block_mask` — all before anything is exchanged, from
    numbers every rank has alike."""
    mask = _block_mask.get()
    if mask is None:
        return None
    from .utils import group_rank_world

    _check_block_mask_tensor(mask)
    world = group_rank_world(group)[1]
    B, Sq, H = q.shape[0], q.shape[1], q.shape[2]
    Sk = k.shape[1]
    if world > 1:
        zigzag = what.lower().startswith("zigzag")      # (only the dense ring and zigzag functions bind a mask)
        unit, per = (Sq // 2, "half of the local length") if zigzag else (Sq, "the local length")
        if Sq != Sk or (zigzag and Sq % 2) or unit % BLOCK_MASK_SIZE:
            raise ValueError(f"ring_flash_attn: {what} with a block mask on {world} ranks needs {per} to be a multiple of "
                             f"{BLOCK_MASK_SIZE}; got a local length of {Sq} (keys: {Sk})")
    nq, nk = -(-Sq // BLOCK_MASK_SIZE), -(-(world * Sk) // BLOCK_MASK_SIZE)
    if (mask.shape[0] not in (1, B) or mask.shape[1] not in (1, H) or tuple(mask.shape[2:]) != (nq, nk) or mask.device != q.device):
        raise ValueError(f"ring_flash_attn: {what}: block_mask must be ({{1, {B}}}, {{1, {H}}}, {nq}, {nk}) on {q.device} — this "
                         f"rank's query blocks against the key blocks of the whole sequence; got {tuple(mask.shape)} on {mask.device}")
    if dropout_p and dropout_p > 0:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask together with dropout is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask together with alibi_slopes is not supported")
    if q.shape[-1] > 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask serves head dims up to 128, not {q.shape[-1]}")
    if k.shape[2] > 0 and H // k.shape[2] > BLOCK_MASK_MAX_GROUP:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask serves at most {BLOCK_MASK_MAX_GROUP} query heads per "
                                  f"K/V head, not {H} / {k.shape[2]}")
    if v.shape[-1] != q.shape[-1]:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask does not serve a value head dim ({v.shape[-1]}) "
                                  f"that differs from q's ({q.shape[-1]})")
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_block_mask", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask needs a backend that serves `block_mask` "
                                  f"(serves_block_mask); {getattr(be, 'name', type(be).__name__)!r} does not")
    return mask


def block_mask_extra(ctx):
    """the `block_mask=` keyword of the schedule's forward / backward of a bound node; nothing for an unbound one"""
    mask = getattr(ctx, "block_mask", None)
    return {} if mask is None else {"block_mask": mask}


def with_block_mask(func, block_mask):
    """A block-sparse mask — window + global + random blocks (BigBird, Longformer), block-selected attention, document masks
    with shared tokens, the blocks of a FlexAttention BlockMask — for the dense ring and zigzag functions:

        attn = with_block_mask(zigzag_ring_flash_attn_func, block_mask)     # bool (Bm, Hm, NQ, NK), contiguous, on q's device
        out = attn(q, k, v, causal=True)

    returns a callable with `func`'s signature and return value in which local query row i sees key j iff
    block_mask[b or 0, h or 0, i // 128, pos(j) // 128] AND the call's own mask (`causal`, `window_size`) allows the pair — the
    diagonal blocks of a causal block mask are just True with causal=True.  Bm in {1, B} and Hm in {1, H} (H: QUERY heads; 1
    broadcasts).  NQ = ceil(S_local / 128): THIS rank's query blocks in the order of q's rows (zigzag: the first chunk's blocks,
    then the second chunk's); NK = ceil(W S_local / 128): the key blocks of the unsharded sequence in natural order (pos(j): the
    global position, as for with_row_ranges).  A row without a visible key: out = 0, lse as for every such row, zero gradients.
    The mask gets no gradient; dq, dk, dv are exact.  The kernels skip every key tile (forward, dQ) and every (query tile,
    head) item (dK/dV) in a dark block.  A zigzag call may be non-causal.
    `block_mask=None`: `func` itself.  Served: ring_flash_attn_{,kvpacked_,qkvpacked_}func and
    zigzag_ring_flash_attn_{,kvpacked_,qkvpacked_}func or a `with_lse_grad` result of one (with_block_mask goes on the outside),
    on any group, with windows, GQA (at most 64 query heads per K/V head), return_attn_probs, bf16 / fp16, head dims 8 .. 128.
    TypeError: any other callable — the *_varlen, stripe_, llama3_ and zigzag_llama3_ families and with_softcap / with_sinks /
    with_max_logit / with_ulysses / with_row_ranges / with_block_mask results.  ValueError: a mask that is not a contiguous bool
    4-d tensor; at the call, a shape or device that does not fit q, and on a multi-rank group a local length (zigzag: half of
    it) that is no multiple of 128 (at one rank any lengths are served, tail blocks are partial, Sq != Sk is fine).
    NotImplementedError at the call, before anything is exchanged: dropout_p > 0, alibi_slopes, head dims above 128, more than
    64 query heads per K/V head, a value head dim of its own, a backend that does not serve it.  The mask is bound to the call and kept on the autograd node —
    activation checkpointing re-runs the wrapped call and binds it again.  Under torch.compile the call runs eagerly behind a
    graph break."""
    import functools

    import ring_flash_attn as pkg

    for marker, what in (("_rfa_block_mask", "with_block_mask"), ("_rfa_row_ranges", "with_row_ranges"), ("_rfa_softcap", "with_softcap"),
                         ("_rfa_sinks", "with_sinks"), ("_rfa_max_logit", "with_max_logit"), ("_rfa_ulysses", "with_ulysses")):
        if getattr(func, marker, False):
            raise TypeError(f"ring_flash_attn.with_block_mask: `func` is a {what} result; not served")
    served = {id(getattr(pkg, n)) for n in ROW_RANGE_FUNCS}
    f = func
    # (a with_lse_grad result carries the marker on both of its layers and leads to the public function it wraps)
    while id(f) not in served and getattr(f, "_rfa_lse_grad", False) and hasattr(f, "__wrapped__"):
        f = f.__wrapped__
    if id(f) not in served:
        raise TypeError("ring_flash_attn.with_block_mask: `func` must be one of ring_flash_attn_{,kvpacked_,qkvpacked_}func and "
                        f"zigzag_ring_flash_attn_{{,kvpacked_,qkvpacked_}}func or a with_lse_grad result of one, got {func!r}")
    if block_mask is None:
        return func
    _check_block_mask_tensor(block_mask)

    @functools.wraps(func, updated=())              # (updated=(): as in with_softcap)
    def masked(*args, **kwargs):
        token = _block_mask.set(block_mask)
        try:
            return func(*args, **kwargs)
        finally:
            _block_mask.reset(token)

    masked._rfa_block_mask = True                    # (the other binders refuse a masked function)
    return _opaque(masked)


# ---- attention over the union of two key sets (ring_flash_attn.merge_attn) ------------------------------------------------
def _check_merge_args(out_a, lse_a, out_b, lse_b):
    ts = (out_a, lse_a, out_b, lse_b)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError("ring_flash_attn.merge_attn: out_a, lse_a, out_b, lse_b must be tensors")
    if out_a.dim() not in (3, 4) or out_a.shape != out_b.shape or out_a.dtype != out_b.dtype:
        raise ValueError(f"ring_flash_attn.merge_attn: out_a {tuple(out_a.shape)} {out_a.dtype} and out_b {tuple(out_b.shape)} "
                         f"{out_b.dtype} must be (B, S, H, D) or (T, H, D) tensors of one shape and dtype")
    want = (out_a.shape[1], out_a.shape[0]) if out_a.dim() == 3 else (out_a.shape[0], out_a.shape[2], out_a.shape[1])
    for nm, l in (("lse_a", lse_a), ("lse_b", lse_b)):
        if l.dtype != torch.float32 or tuple(l.shape) != want:
            raise ValueError(f"ring_flash_attn.merge_attn: {nm} must be float32 of shape {want} — (B, H, S) for a (B, S, H, D) "
                             f"out, (H, T) for a (T, H, D) out; got {l.dtype} {tuple(l.shape)}")
    if any(t.device != out_a.device for t in ts):
        raise ValueError("ring_flash_attn.merge_attn: out_a, lse_a, out_b, lse_b must be on one device; got "
                         + ", ".join(str(t.device) for t in ts))


class _MergeAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_a, lse_a, out_b, lse_b):
        from .backend import get_backend

        out, lse = get_backend().merge_pair(out_a, lse_a, out_b, lse_b)
        ctx.save_for_backward(out_a, lse_a, out_b, lse_b)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, dlse):
        from .backend import get_backend

        out_a, lse_a, out_b, lse_b = ctx.saved_tensors
        if dout is None:
            dout = torch.zeros_like(out_a)
        if dlse is not None:
            dlse = dlse.to(torch.float32)
        da, dla, db, dlb = get_backend().merge_pair_bwd(dout, dlse, out_a, lse_a, out_b, lse_b)
        need = ctx.needs_input_grad
        return (da if need[0] else None, dla if need[1] else None, db if need[2] else None, dlb if need[3] else None)


def merge_attn(out_a, lse_a, out_b, lse_b):
    """(out, lse) of attention over the UNION of two key sets, from the finished results of attention over each:

        attn = with_lse_grad(zigzag_ring_flash_attn_func)
        out_s, lse_s, _ = attn(q, k, v, causal=True, return_attn_probs=True)                # the sharded sequence
        out_p, lse_p, _ = with_lse_grad(ring_flash_attn_func)(q, kp, vp, return_attn_probs=True, group=self_group)   # replicated prefix keys
        out, lse = merge_attn(out_p, lse_p, out_s, lse_s)

    lse = logaddexp(lse_a, lse_b), out = exp(lse_a - lse) out_a + exp(lse_b - lse) out_b — one fused kernel each way, fp32
    arithmetic, out rounded once; differentiable in all four inputs (once).  The forward is exact; the backward is exact only
    if the gradients of lse_a / lse_b reach the scores, which is what `with_lse_grad` is for.  out_x: (B, S, H, D) with lse_x
    (B, H, S) float32, or packed (T, H, D) with (H, T) — the layouts the attention functions return; bf16 / fp16.
    Empty rows: an infinite lse_x of either sign (+inf: a row without a visible key) marks side x as empty — weight 0, zero
    gradients; both empty: out = 0, lse = -inf.  No NaN comes out of such rows.  The result merges again (an N-way merge is a
    chain of these).
    ValueError: mismatched shapes or dtypes, an lse that is not float32 in the layout belonging to out, tensors on different
    devices.  NotImplementedError: a backend that does not serve it."""
    _check_merge_args(out_a, lse_a, out_b, lse_b)
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_merge_pair", False):
        raise NotImplementedError("ring_flash_attn.merge_attn needs a backend that serves `merge_pair` / `merge_pair_bwd`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not")
    return _MergeAttn.apply(out_a, lse_a, out_b, lse_b)


merge_attn = _opaque(merge_attn)


# ---- attention sinks (ring_flash_attn.with_sinks) ------------------------------------------------------------------------
# The sink is applied once, to the merged (out, lse) a schedule's forward returned (include/rfa.h: rfa_sink_apply), so no
# schedule and no attention kernel computes anything for it.  The tensor has to be a real INPUT of the autograd node for
# `sinks.grad` to be filled by ordinary autograd: with_sinks binds it to the call, the public function that runs inside hands
# it to its autograd Function as ONE extra trailing argument of `apply` (sink_args: nothing for a call without sinks — such a
# call builds the node it always built), and the node saves it.  The binding is read there, at the public entry of the
# forward, and nowhere else: a backward reads its saved tensors only.
import contextvars

_sinks = contextvars.ContextVar("ring_flash_attn_sinks", default=None)


def sink_args():
    """() for a plain call, (sinks,) inside a call bound by `with_sinks`: the tail of the autograd Functions' `apply`"""
    t = _sinks.get()
    return () if t is None else (t,)


def split_sinks(rest, n):
    """(the n regular arguments, sinks or None) of an autograd Function's `*rest`"""
    return rest[:n], (rest[n] if len(rest) > n else None)


def checked_sinks(sinks, q, what):
    """the refusals of a call with sinks that need the tensors — ValueError: not a floating (H,) tensor on q's device;
    NotImplementedError: a backend that does not serve sinks — before anything is exchanged, on every rank alike"""
    if sinks is None:
        return None
    H = q.shape[-2]
    if (not isinstance(sinks, torch.Tensor) or not sinks.is_floating_point() or sinks.dim() != 1 or sinks.shape[0] != H
            or sinks.device != q.device):
        got = f"{tuple(sinks.shape)} {sinks.dtype} on {sinks.device}" if isinstance(sinks, torch.Tensor) else repr(sinks)
        raise ValueError(f"ring_flash_attn: {what} with sinks needs a floating tensor of shape ({H},) on {q.device}, one "
                         f"logit per query head; got {got}")
    from .backend import get_backend

    be = get_backend()
    if not getattr(be, "serves_sinks", False):
        raise NotImplementedError(f"ring_flash_attn: {what} with sinks needs a backend that serves `sink_apply` / `sink_grad`; "
                                  f"{getattr(be, 'name', type(be).__name__)!r} does not")
    return sinks


def apply_sinks(sinks, out, lse):
    """(out', lse') of the call with sinks from the schedule's merged (out, lse); the pair itself without sinks"""
    if sinks is None:
        return out, lse
    from .backend import get_backend

    return get_backend().sink_apply(out, lse, sinks, varlen=out.dim() == 3)


def sinks_grad(ctx, sinks, dout, out, lse):
    """the tail of a backward's gradients for the trailing `sinks` input: () without one, else (dsink,) — this rank's sum over
    its own query rows, in sinks' dtype (None when sinks needs no gradient)"""
    if sinks is None:
        return ()
    if not ctx.needs_input_grad[-1]:
        return (None,)
    from .backend import get_backend

    return (get_backend().sink_grad(dout, out, lse, sinks, varlen=out.dim() == 3).to(sinks.dtype),)


def with_sinks(func, sinks):
    """Attention sinks (GPT-OSS, the streaming-LLM family; flash_attn's and Hugging Face's `s_aux`) for one of this package's
    public attention functions:

        attn = with_sinks(ring_flash_attn_func, sinks)       # sinks: (H,) floating tensor on q's device, may require grad
        out = attn(q, k, v, causal=True, window_size=(127, 0))

    returns a callable with `func`'s signature that runs `func` with one extra softmax column per query head whose logit is
    sinks[h] and whose value vector is zero: p_ij = exp(s_ij - lse'_i), lse'_i = log(sum_j exp(s_ij) + exp(sinks[h])),
    out'_i = sum_j p_ij v_j.  The call returns out' (and lse' with return_attn_probs=True); dq, dk, dv are exact, and
    `sinks.grad` is filled by autograd, in sinks' dtype.  Served on any group and with everything `func` serves there —
    windows, packed input, GQA, dropout.  `sinks` None: `func` itself.
    Several ranks: the sink is applied on the rank that owns the query rows, after its blocks are merged; the gradient a
    rank gets is its PARTIAL, the sum over its own query rows — as for every replicated parameter under sequence
    parallelism, the framework's gradient all-reduce over the group completes it.  This package posts no collective for it.
    The schedules return `out` rounded to the io dtype, so out' is rounded twice (profiles/sinks.md).
    ValueError: sinks is not a floating tensor of shape (H,) (at the call: H is q's head count, on q's device).  TypeError:
    `func` is not one of the public attention functions; a `with_softcap` result is refused too — the cap and the sinks
    together are not served yet.  NotImplementedError at the call: a backend that does not serve sinks.
    The tensor is bound to the call and saved on the autograd node — activation checkpointing re-runs the wrapped call and
    binds it again; the backward reads nothing ambient.  Under torch.compile the call runs eagerly behind a graph break."""
    import functools

    import ring_flash_attn as pkg

    if getattr(func, "_rfa_softcap", None):
        raise TypeError("ring_flash_attn.with_sinks: `func` is a with_softcap result; soft-capping together with sinks is not "
                        "served yet (the cap and the sinks would have to be bound to one call)")
    public = {id(getattr(pkg, n)): n for n in dir(pkg) if n.endswith("_func")}
    if id(func) not in public:
        raise TypeError("ring_flash_attn.with_sinks: `func` must be one of the package's public attention functions "
                        f"(ring_flash_attn.*_func), got {func!r}")
    if sinks is None:
        return func
    if not isinstance(sinks, torch.Tensor) or not sinks.is_floating_point() or sinks.dim() != 1:
        raise ValueError("ring_flash_attn.with_sinks: sinks must be a floating tensor of shape (H,), one logit per query "
                         f"head; got {tuple(sinks.shape) if isinstance(sinks, torch.Tensor) else sinks!r}")

    @functools.wraps(func, updated=())              # (updated=(): as in with_softcap)
    def sunk(*args, **kwargs):
        token = _sinks.set(sinks)
        try:
            return func(*args, **kwargs)
        finally:
            _sinks.reset(token)

    sunk._rfa_sinks = True                           # (with_ulysses refuses to wrap a function with sinks)
    return _opaque(sunk)


# ---- per-head max attention logit (ring_flash_attn.with_max_logit) ---------------------------------------------------------
def _check_max_logit_tensor(t, q=None):
    """ValueError unless t is a contiguous float32 1-d tensor that does not require grad — and, given the call's first tensor
    argument (q, or a packed qkv: heads are its second-to-last dimension), has one entry per query head on its device"""
    ok = (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous()
          and not t.requires_grad)
    if ok and q is not None:
        ok = t.shape[0] == q.shape[-2] and t.device == q.device
    if not ok:
        want = f"({q.shape[-2]},) on {q.device}" if q is not None else "(H,)"
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}, requires_grad={t.requires_grad}" if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f"ring_flash_attn.with_max_logit: max_logit must be a contiguous float32 tensor of shape {want}, one "
                         f"entry per query head, that does not require grad; got {got}")


def with_max_logit(func, max_logit):
    """The per-head max attention logit (QK-Clip / MuonClip; Transformer Engine's and Megatron's `max_logit`) of one of this
    package's public attention functions:

        m = torch.full((H,), float("-inf"), device=q.device)        # fp32; -inf starts a new measurement
        attn = with_max_logit(ring_flash_attn_func, m)
        out = attn(q, k, v, causal=True)
        dist.all_reduce(m, op=dist.ReduceOp.MAX, group=group)       # several ranks: the caller completes it

    returns a callable with `func`'s signature and return value; every forward it runs max-accumulates, for every query head h,

        max over batch b, this rank's query rows i and ALL keys j of the full sequence that row i sees
        of softmax_scale * q[b,i,h,:] . k[b,j,h // G,:]

    into max_logit[h] — "sees" is exactly the visibility of the attention that ran (causal, window_size, packed sequences, the
    schedule's own layout); the value is the raw scaled dot product, whatever softcap, alibi_slopes, dropout or sinks the call
    carries; a head without a visible pair contributes -inf; NaN logits are ignored.  There is no gradient and the backward
    never touches the tensor; a re-run under activation checkpointing accumulates the same values again.
    Several ranks: a rank gets its PARTIAL — its own query rows against all keys, the convention of `sinks.grad`; this package
    posts no collective for it.
    `max_logit` None: `func` itself.  Served: the 21 `*_func` of the package and `with_softcap` / `with_sinks` results of them, on
    any group, head dims 8 .. 256.  TypeError: any other callable — a `with_ulysses` result (heads are renumbered) and a
    `with_max_logit` result included.  ValueError, here or at the call: a tensor that is not float32, (H,), contiguous, on q's
    device, or that requires grad; at the call: softmax_scale <= 0.  NotImplementedError at the call, before anything is
    exchanged: a backend that does not serve `max_logit`.  Under torch.compile the call runs eagerly behind a graph break.
    The separate pass over q and k costs about a forward's S GEMM (profiles/max_logit.md)."""
    import functools
    import inspect

    import ring_flash_attn as pkg
    from .backend import max_logit_scope, require_max_logit

    if getattr(func, "_rfa_ulysses", False):
        raise TypeError("ring_flash_attn.with_max_logit: `func` is a with_ulysses result; the exchange renumbers the heads a "
                        "rank computes — not served yet (bind with_max_logit to the function and read the head slices)")
    if getattr(func, "_rfa_max_logit", False):
        raise TypeError("ring_flash_attn.with_max_logit: `func` is a with_max_logit result already")
    public = {id(getattr(pkg, n)): n for n in dir(pkg) if n.endswith("_func")}
    if id(func) not in public and not getattr(func, "_rfa_softcap", None) and not getattr(func, "_rfa_sinks", False):
        raise TypeError("ring_flash_attn.with_max_logit: `func` must be one of the package's public attention functions "
                        f"(ring_flash_attn.*_func) or a with_softcap / with_sinks result of one, got {func!r}")
    if max_logit is None:
        return func
    _check_max_logit_tensor(max_logit)
    sig = inspect.signature(func)

    @functools.wraps(func, updated=())               # (updated=(): as in with_softcap)
    def measured(*args, **kwargs):
        bound = sig.bind(*args, **kwargs).arguments
        _check_max_logit_tensor(max_logit, next(iter(bound.values())))
        scale = bound.get("softmax_scale", None)
        if scale is not None and not scale > 0:
            raise ValueError(f"ring_flash_attn.with_max_logit: softmax_scale must be positive, got {scale!r}")
        require_max_logit(public.get(id(func), getattr(func, "__name__", "the call")) + " with max_logit")
        with max_logit_scope(max_logit):
            return func(*args, **kwargs)

    measured._rfa_max_logit = True
    return _opaque(measured)


def has_window(window_size) -> bool:
    return window_size is not None and (window_size[0] >= 0 or window_size[1] >= 0)


def window_ok_for(group) -> bool:
    from .utils import group_rank_world

    return group_rank_world(group)[1] == 1


def _keep_list(ctx, forward_impl):
    """Schedules that can hand buffers from their forward to their backward (`forward_impl.keeps_for_backward`: the
    zigzag gather form keeps the K/V it gathered) get a list to append tensors to — only when an input needs a
    gradient.  The tensors are stored with ctx.save_for_backward, i.e. they are owned by the autograd graph: freed with
    it, never kept for torch.no_grad() calls (no graph), discarded and re-made under activation checkpointing, visible
    to saved-tensor hooks (offloading) — there is no process-global hand-off."""
    if getattr(forward_impl, "keeps_for_backward", False) and any(ctx.needs_input_grad[:3]):
        keep = _KeepList()
        return keep, {"keep": keep}
    return None, {}


class _KeepList(list):
    """the tensors a forward hands to its backward, the reservation they hold in the process-wide budget of kept bytes
    (config.kept_budget) and the group's agreement that EVERY rank kept (utils.Agreement; None: nothing was asked)"""
    token = None
    agreed = None


def _hold_kept(ctx, keep):
    ctx.kept_token = keep.token if keep is not None else None
    ctx.kept_agreed = keep.agreed if keep is not None else None


def _release_kept(ctx):
    """The reservation returns when the kept buffers are gone: with the backward when the graph is not retained, else
    with the graph (Token.__del__).  Whether this backward retains the graph is not visible from inside it, so the test
    runs as an engine callback at the END of the backward pass: by then a non-retained node has dropped its saved tensors
    (reading them raises), a retained one still has them and keeps its reservation."""
    tok = getattr(ctx, "kept_token", None)
    if tok is None:
        return

    def after_backward():
        try:
            ctx.saved_tensors
        except RuntimeError:
            tok.release()

    try:
        torch.autograd.Variable._execution_engine.queue_callback(after_backward)
    except Exception:                # (not inside an engine run: a direct call of the backward in a test)
        tok.release()


def _split_kept(ctx, more):
    n = getattr(ctx, "n_lead_t", len(more))
    tensors_lead, kept = more[:n], more[n:]
    agreed = getattr(ctx, "kept_agreed", None)
    if agreed is not None and not agreed.resolve():
        # some rank could not keep its gathered K/V: EVERY rank gathers again (a rank deciding alone would leave the
        # others in a collective it does not join); this rank's buffers are simply not used
        kept = ()
    return tensors_lead, ({"kept": tuple(kept)} if kept else {})


def make_autograd_function(name, forward_impl, backward_impl, n_lead, window_ring=False, dropout_ring=False,
                           alibi_ring=False, vdim=False):
    """n_lead: number of non-tensor positional arguments between (q,k,v) and the common tail
    (0 for the batch API, 2 = (cu_seqlens, max_seqlen) for varlen).  window_ring: the schedule serves a sliding window
    on a multi-rank group (every ring family does: dense and varlen ring and zigzag, stripe).  dropout_ring: it serves
    dropout there (the dense ring, zigzag and stripe schedules: every block call is told the global positions of its
    rows, _common.dropout_arg).  alibi_ring: it serves alibi_slopes there (the dense ring and zigzag schedules).
    vdim: it serves a `v` whose head dim differs from q's (the five ring-type families, on any group: checked_vdim)."""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v, *rest):
            rest, sinks = split_sinks(rest, n_lead + 8)
            lead = rest[:n_lead]
            (dropout_p, softmax_scale, causal, window_size, alibi_slopes, deterministic,
             return_softmax, group) = rest[n_lead:]
            if softmax_scale is None:
                softmax_scale = q.shape[-1] ** (-0.5)
            checked_vdim(q, k, v, dropout_p, alibi_slopes, name, served=vdim)
            single = window_ok_for(group)
            _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=single or window_ring, dropout_ok=single or dropout_ring,
                               alibi_ok=single or alibi_ring)
            alibi_slopes = checked_alibi(alibi_slopes, q, (len(lead[0]) - 1) if n_lead else q.shape[0], name)
            ctx.softcap = checked_softcap(dropout_p, alibi_slopes, q, name, window_size, causal)
            ctx.lse_grad = checked_lse_grad(ctx, name)
            ctx.row_ranges = checked_row_ranges(q, k, v, dropout_p, alibi_slopes, name)
            ctx.block_mask = checked_block_mask(q, k, v, dropout_p, alibi_slopes, name, group)
            sinks = checked_sinks(sinks, q, name)
            q, k, v = _prep_qkv(q, k, v, group)
            tensors_lead = ()
            if n_lead:
                cu = _as_cu(lead[0], q.device)
                lead = (cu,) + tuple(lead[1:])
                tensors_lead = (cu,)
            keep, extra = _keep_list(ctx, forward_impl)
            extra.update(row_ranges_extra(ctx))
            extra.update(block_mask_extra(ctx))
            ctx.dropout = (dropout_p, draw_dropout_seed()) if dropout_p and dropout_p > 0 else (0.0, None)
            if ctx.dropout[1] is not None:
                extra["dropout_seed"] = ctx.dropout[1]
            with softcap_scope(ctx.softcap):
                out, softmax_lse = forward_impl(
                    group, q, k, v, *lead, softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                    window_size=window_size, alibi_slopes=alibi_slopes, deterministic=False, **extra,
                )
            audit_verify(group, f"{name} forward")          # (config.exchange_check: a no-op otherwise)
            # (with sinks: out', lse' are what the backward is handed and what the call returns)
            out, softmax_lse = apply_sinks(sinks, out, softmax_lse)
            ctx.save_for_backward(q, k, v, out, softmax_lse, *tensors_lead, *(keep or ()), *(() if sinks is None else (sinks,)))
            ctx.has_sinks = sinks is not None
            _hold_kept(ctx, keep)
            ctx.n_lead_t, ctx.n_keep = len(tensors_lead), len(keep or ())
            ctx.lead_rest = tuple(lead[1:]) if n_lead else ()
            ctx.softmax_scale = softmax_scale
            ctx.causal = causal
            ctx.deterministic = deterministic
            ctx.group = group
            ctx.window_size = tuple(window_size)
            ctx.alibi_slopes = alibi_slopes             # (no gradient, as in flash_attn: held, not saved for backward)
            return out if not return_softmax else (out, softmax_lse, None)

        @staticmethod
        def backward(ctx, dout, *args):
            q, k, v, out, softmax_lse, *more = ctx.saved_tensors
            sinks = more.pop() if ctx.has_sinks else None
            tensors_lead, extra = _split_kept(ctx, more)
            dout, lse_kw = lse_grad_kw(ctx, dout, args, out, softmax_lse)
            extra.update(lse_kw)
            extra.update(row_ranges_extra(ctx))
            extra.update(block_mask_extra(ctx))
            if ctx.dropout[1] is not None:
                extra["dropout_seed"] = ctx.dropout[1]
            with softcap_scope(ctx.softcap):
                dq, dk, dv = backward_impl(
                    ctx.group, dout, q, k, v, out, softmax_lse, *tensors_lead, *ctx.lead_rest,
                    softmax_scale=ctx.softmax_scale, dropout_p=ctx.dropout[0], causal=ctx.causal,
                    window_size=ctx.window_size, alibi_slopes=ctx.alibi_slopes, deterministic=ctx.deterministic, **extra,
                )
            _release_kept(ctx)
            audit_verify(ctx.group, f"{name} backward")
            return (dq, dk, dv) + (None,) * (n_lead + 8) + sinks_grad(ctx, sinks, dout, out, softmax_lse)

    _Fn.__name__ = _Fn.__qualname__ = name
    return _Fn


def make_packed_function(name, base_fn, forward_impl, backward_impl, n_lead, pack_dim, n_packed, packed_travel=False,
                         window_ring=False, dropout_ring=False, alibi_ring=False):
    """autograd Function for the packed entry points (`kv` = 2 tensors, `qkv` = 3 tensors stacked on
    `pack_dim`).  Same math as `base_fn`; the only difference is where the gradients land: ONE packed
    buffer whose slices are handed to the schedule as output views (`out_grads`), instead of letting
    autograd build the packed gradient from three slice-gradients (zero-fill + copy + add kernels
    per step).  Falls back to the generic path when the schedule returns fresh tensors (W > 1)."""

    class _PFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *args):
            n_t = 1 if n_packed == 3 else 2                 # (qkv,) or (q, kv)
            tensors, rest = args[:n_t], args[n_t:]
            packed = tensors[-1]
            parts = [packed.select(pack_dim, i) for i in range(n_packed)]
            q, k, v = (parts if n_packed == 3 else [tensors[0]] + parts)
            rest, sinks = split_sinks(rest, n_lead + 8)
            lead = rest[:n_lead]
            (dropout_p, softmax_scale, causal, window_size, alibi_slopes, deterministic,
             return_softmax, group) = rest[n_lead:]
            if softmax_scale is None:
                softmax_scale = q.shape[-1] ** (-0.5)
            single = window_ok_for(group)
            _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=single or window_ring, dropout_ok=single or dropout_ring,
                               alibi_ok=single or alibi_ring)
            alibi_slopes = checked_alibi(alibi_slopes, q, (len(lead[0]) - 1) if n_lead else q.shape[0], name)
            ctx.softcap = checked_softcap(dropout_p, alibi_slopes, q, name, window_size, causal)
            ctx.lse_grad = checked_lse_grad(ctx, name)
            ctx.row_ranges = checked_row_ranges(q, k, v, dropout_p, alibi_slopes, name)
            ctx.block_mask = checked_block_mask(q, k, v, dropout_p, alibi_slopes, name, group)
            sinks = checked_sinks(sinks, q, name)
            q, k, v = _prep_qkv(q, k, v, group, packed_travel=packed_travel and n_packed == 2)
            tensors_lead = ()
            if n_lead:
                cu = _as_cu(lead[0], q.device)
                lead = (cu,) + tuple(lead[1:])
                tensors_lead = (cu,)
            keep, extra = _keep_list(ctx, forward_impl)
            extra.update(row_ranges_extra(ctx))
            extra.update(block_mask_extra(ctx))
            ctx.dropout = (dropout_p, draw_dropout_seed()) if dropout_p and dropout_p > 0 else (0.0, None)
            if ctx.dropout[1] is not None:
                extra["dropout_seed"] = ctx.dropout[1]
            with softcap_scope(ctx.softcap):
                out, softmax_lse = forward_impl(
                    group, q, k, v, *lead, softmax_scale=softmax_scale, dropout_p=dropout_p, causal=causal,
                    window_size=window_size, alibi_slopes=alibi_slopes, deterministic=False, **extra,
                )
            audit_verify(group, f"{name} forward")          # (config.exchange_check: a no-op otherwise)
            # (with sinks: out', lse' are what the backward is handed and what the call returns)
            out, softmax_lse = apply_sinks(sinks, out, softmax_lse)
            ctx.save_for_backward(q, k, v, out, softmax_lse, *tensors_lead, *(keep or ()), *(() if sinks is None else (sinks,)))
            ctx.has_sinks = sinks is not None
            _hold_kept(ctx, keep)
            ctx.n_lead_t, ctx.n_keep = len(tensors_lead), len(keep or ())
            ctx.lead_rest = tuple(lead[1:]) if n_lead else ()
            ctx.softmax_scale = softmax_scale
            ctx.causal = causal
            ctx.deterministic = deterministic
            ctx.group = group
            ctx.window_size = tuple(window_size)
            ctx.alibi_slopes = alibi_slopes             # (no gradient, as in flash_attn: held, not saved for backward)
            ctx.packed_meta = (packed.shape, packed.dtype, packed.device)
            return out if not return_softmax else (out, softmax_lse, None)

        @staticmethod
        def backward(ctx, dout, *args):
            q, k, v, out, softmax_lse, *more = ctx.saved_tensors
            sinks = more.pop() if ctx.has_sinks else None
            tensors_lead, extra = _split_kept(ctx, more)
            dout, lse_kw = lse_grad_kw(ctx, dout, args, out, softmax_lse)
            extra.update(lse_kw)
            extra.update(row_ranges_extra(ctx))
            extra.update(block_mask_extra(ctx))
            shape, dtype, device = ctx.packed_meta
            dpacked = torch.empty(shape, dtype=dtype, device=device)
            views = [dpacked.select(pack_dim, i) for i in range(n_packed)]
            if n_packed == 3:
                out_grads = tuple(views)
            else:
                out_grads = (None, views[0], views[1])
            if ctx.dropout[1] is not None:
                extra["dropout_seed"] = ctx.dropout[1]
            with softcap_scope(ctx.softcap):
                dq, dk, dv = backward_impl(
                    ctx.group, dout, q, k, v, out, softmax_lse, *tensors_lead, *ctx.lead_rest,
                    softmax_scale=ctx.softmax_scale, dropout_p=ctx.dropout[0], causal=ctx.causal,
                    window_size=ctx.window_size, alibi_slopes=ctx.alibi_slopes, deterministic=ctx.deterministic,
                    out_grads=out_grads, **extra,
                )
            got = (dq, dk, dv)[3 - n_packed:]
            for view, g in zip(views, got):
                if g.data_ptr() != view.data_ptr():       # schedule returned its own tensor
                    view.copy_(g)
            grads = (dpacked,) if n_packed == 3 else (dq, dpacked)
            _release_kept(ctx)
            audit_verify(ctx.group, f"{name} backward")
            return grads + (None,) * (n_lead + 8) + sinks_grad(ctx, sinks, dout, out, softmax_lse)

    _PFn.__name__ = _PFn.__qualname__ = name
    return _PFn


def _grad_buffers(out_grads, q, k, v):
    """(dq, dk, dv) output tensors for the single-GPU path: caller-provided views or fresh."""
    og = out_grads or (None, None, None)
    return (og[0] if og[0] is not None else (torch.empty_like(q) if q is not None else None),
            og[1] if og[1] is not None else torch.empty_like(k),
            og[2] if og[2] is not None else torch.empty_like(v))


def make_dense_api(fn, prefix, forward_impl=None, backward_impl=None, packed_travel=False, window_ring=False,
                   dropout_ring=False, alibi_ring=False):
    """(B,S,H,D) API: returns (func, kvpacked_func, qkvpacked_func).  packed_travel: the schedule exchanges a
    packed `kv` as one buffer and writes dK/dV straight into the packed gradient (`out_grads`) at any world size.
    window_ring, dropout_ring, alibi_ring: as in make_autograd_function (pass the same values to both)."""
    kv_fn = qkv_fn = None
    if forward_impl is not None:
        kv_fn = make_packed_function(fn.__name__ + "KVPacked", fn, forward_impl, backward_impl, 0, 2, 2,
                                     packed_travel=packed_travel, window_ring=window_ring, dropout_ring=dropout_ring,
                                     alibi_ring=alibi_ring)
        qkv_fn = make_packed_function(fn.__name__ + "QKVPacked", fn, forward_impl, backward_impl, 0, 2, 3,
                                      window_ring=window_ring, dropout_ring=dropout_ring, alibi_ring=alibi_ring)

    def func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
             alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
        return fn.apply(q, k, v, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                        deterministic, return_attn_probs, group, *sink_args())

    def kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                      alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
        if kv_fn is not None:
            return kv_fn.apply(q, kv, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                               deterministic, return_attn_probs, group, *sink_args())
        return fn.apply(q, kv[:, :, 0], kv[:, :, 1], dropout_p, softmax_scale, causal, window_size,
                        alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    def qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                       alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
        if qkv_fn is not None:
            return qkv_fn.apply(qkv, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                                deterministic, return_attn_probs, group, *sink_args())
        return fn.apply(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], dropout_p, softmax_scale, causal,
                        window_size, alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    must_be_causal = prefix in ("zigzag_ring_flash_attn", "stripe_flash_attn")

    def lower(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), alibi_slopes=None,
              deterministic=False, return_attn_probs=False, group=None):
        from ._ops import single_device_attention

        _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=True)
        assert causal or not must_be_causal, f"{prefix} is meaningless for causal=False"
        return single_device_attention(q, k, v, None, 0, softmax_scale, causal, return_attn_probs, window_size)

    def lower_kv(q, kv, *a, **kw):
        return lower(q, kv[:, :, 0], kv[:, :, 1], *a, **kw)

    def lower_qkv(qkv, *a, **kw):
        return lower(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], *a, **kw)

    multi = multi_kv = multi_qkv = None
    if forward_impl is not None:
        from . import _ops

        _ops.register_schedule(prefix, forward_impl, backward_impl)

        def multi(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), alibi_slopes=None,
                  deterministic=False, return_attn_probs=False, group=None):
            _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=False)
            assert causal or not must_be_causal, f"{prefix} is meaningless for causal=False"
            return _ops.multi_rank_attention(prefix, q, k, v, None, 0, softmax_scale, causal, return_attn_probs, group)

        def multi_kv(q, kv, *a, **kw):
            return multi(q, kv[:, :, 0], kv[:, :, 1], *a, **kw)

        def multi_qkv(qkv, *a, **kw):
            return multi(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], *a, **kw)

    for f, suffix in ((func, "func"), (kvpacked_func, "kvpacked_func"), (qkvpacked_func, "qkvpacked_func")):
        f.__name__ = f.__qualname__ = f"{prefix}_{suffix}"
    return (_compilable(func, lower, multi), _compilable(kvpacked_func, lower_kv, multi_kv),
            _compilable(qkvpacked_func, lower_qkv, multi_qkv))


def make_varlen_api(fn, prefix, forward_impl=None, backward_impl=None, window_ring=False):
    """(T,H,D) + (cu_seqlens, max_seqlen) API.  With the schedule's forward / backward the packed entry points get
    their own autograd Function (gradients land in ONE packed buffer, see make_packed_function).
    window_ring: as in make_autograd_function (pass the same value to both)."""
    kv_fn = qkv_fn = None
    if forward_impl is not None:
        kv_fn = make_packed_function(fn.__name__ + "KVPacked", fn, forward_impl, backward_impl, 2, 1, 2,
                                     window_ring=window_ring)
        qkv_fn = make_packed_function(fn.__name__ + "QKVPacked", fn, forward_impl, backward_impl, 2, 1, 3,
                                      window_ring=window_ring)

    def func(q, k, v, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
             window_size=(-1, -1), alibi_slopes=None, deterministic=False, return_attn_probs=False,
             group=None):
        return fn.apply(q, k, v, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                        alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    def kvpacked_func(q, kv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                      window_size=(-1, -1), alibi_slopes=None, deterministic=False,
                      return_attn_probs=False, group=None):
        if kv_fn is not None:
            return kv_fn.apply(q, kv, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                               alibi_slopes, deterministic, return_attn_probs, group, *sink_args())
        return fn.apply(q, kv[:, 0], kv[:, 1], cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal,
                        window_size, alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    def qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                       window_size=(-1, -1), alibi_slopes=None, deterministic=False,
                       return_attn_probs=False, group=None):
        if qkv_fn is not None:
            return qkv_fn.apply(qkv, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                                alibi_slopes, deterministic, return_attn_probs, group, *sink_args())
        return fn.apply(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu_seqlens, max_seqlen, dropout_p, softmax_scale,
                        causal, window_size, alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    must_be_causal = prefix.startswith("zigzag")

    def lower(q, k, v, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
              window_size=(-1, -1), alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
        from ._ops import single_device_attention

        _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=True)
        assert causal or not must_be_causal, f"{prefix} is meaningless for causal=False"
        return single_device_attention(q, k, v, cu_seqlens, max_seqlen, softmax_scale, causal, return_attn_probs,
                                       window_size)

    def lower_kv(q, kv, *a, **kw):
        return lower(q, kv[:, 0], kv[:, 1], *a, **kw)

    def lower_qkv(qkv, *a, **kw):
        return lower(qkv[:, 0], qkv[:, 1], qkv[:, 2], *a, **kw)

    multi = multi_kv = multi_qkv = None
    if forward_impl is not None:
        from . import _ops

        _ops.register_schedule(prefix, forward_impl, backward_impl)

        def multi(q, k, v, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                  window_size=(-1, -1), alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
            _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=False)
            assert causal or not must_be_causal, f"{prefix} is meaningless for causal=False"
            return _ops.multi_rank_attention(prefix, q, k, v, cu_seqlens, max_seqlen, softmax_scale, causal,
                                             return_attn_probs, group)

        def multi_kv(q, kv, *a, **kw):
            return multi(q, kv[:, 0], kv[:, 1], *a, **kw)

        def multi_qkv(qkv, *a, **kw):
            return multi(qkv[:, 0], qkv[:, 1], qkv[:, 2], *a, **kw)

    for f, suffix in ((func, "func"), (kvpacked_func, "kvpacked_func"), (qkvpacked_func, "qkvpacked_func")):
        f.__name__ = f.__qualname__ = f"{prefix}_{suffix}"
    return (_compilable(func, lower, multi), _compilable(kvpacked_func, lower_kv, multi_kv),
            _compilable(qkvpacked_func, lower_qkv, multi_qkv))
