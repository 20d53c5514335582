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

The layer is four things, each written once:
    ScheduleSpec    what a schedule family serves and how its public functions are shaped; built once per family and handed to
                    the node factory (make_autograd_function) and to the API factory (make_api) alike.
    the node body   _node_forward / _node_backward: the plain, kv-packed and qkv-packed autograd Functions are adapters that
                    select views and say where the gradients land.  call_preamble is the per-call list of refusals, in ONE
                    order, for these nodes and for the two llama3 families.
    the binders     with_softcap, with_sinks, with_max_logit, with_lse_grad, with_row_ranges, with_block_mask (and
                    ulysses.with_ulysses) are _admit + _bind: `_RULES` is the one table that says which functions a binder
                    serves, which other binders' results it takes and what it answers otherwise; _bind makes the callable.
    _refuse         the clauses every call-level feature repeats (dropout, alibi_slopes, head dims above 128, a value head dim
                    of its own, a backend that does not serve it), parameterised by the feature's name.
A new call-level feature is a row of `_RULES`, a `checked_*` in call_preamble and its keyword to the schedules.
"""
import contextvars
import functools
import inspect
from typing import NamedTuple, Optional

import torch

from ._common import _prep_qkv, _as_cu, check_alibi_slopes, draw_dropout_seed, require_alibi
from .backend import get_backend, softcap_scope
from .utils import audit_verify


def _opaque(fn):
    """The schedules are ctypes calls into librfa_hip.so interleaved with torch.distributed traffic, which dynamo
    cannot trace: behind `torch.compiler.disable` a compiled caller graph-breaks around them and runs them
    eagerly, with identical results (multi-rank groups; llama3)."""
    try:
        wrapped = torch.compiler.disable(fn)
        functools.update_wrapper(wrapped, fn)
        return wrapped
    except Exception:        # very old torch without torch.compiler
        return fn


def _single_rank(group) -> bool:
    import torch.distributed as dist

    return dist.get_world_size(group) == 1


def _compilable(fn, lower, multi):
    """Public callable = `fn` (eager: the autograd Functions below, opaque to dynamo) except while dynamo is
    TRACING it on a single-rank group: then `lower(bound)` — bound: the call's arguments by name — expresses the call
    with the registered custom
    operators (_ops.py: rfa::attn_fwd / rfa::attn_bwd, fake kernels + autograd formula), so `torch.compile`
    captures the operator in its graph instead of breaking it (the reference runs its tests a second time under
    torch.compile: test/test.sh:23-25).  `multi(bound)`: the same for a multi-rank group —
    the whole schedule as one operator per direction (_ops.py: rfa::sched_fwd / rfa::sched_bwd)."""
    eager = _opaque(fn)
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
                    return lower(bound)
                # several ranks: the whole schedule as one registered operator (_ops.py: rfa::sched_fwd / sched_bwd)
                # — windowed calls keep the eager path behind a graph break
                if not has_window(bound.get("window_size", (-1, -1))):
                    return multi(bound)
        return eager(*args, **kwargs)

    return public


# ---- the refusals every call-level feature shares ---------------------------------------------------------------------------
def _refuse(what, feature, q=None, v=None, dropout_p=None, alibi_slopes=None, backend=None):
    """NotImplementedError for `what` (the function the message names) with `feature` ("softcap", "row ranges", "a block
    mask" ...) in a call it is not served in — the clauses, in their one order, each only for what is handed in: dropout_p > 0,
    alibi_slopes, q's head dim above 128, v's head dim differing from q's, and `backend` = (serves_* attribute, how the message
    spells what is missing): a backend without it.  Before anything is exchanged, from numbers every rank has alike."""
    if dropout_p and dropout_p > 0:
        raise NotImplementedError(f"ring_flash_attn: {what} with {feature} together with dropout is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError(f"ring_flash_attn: {what} with {feature} together with alibi_slopes is not supported")
    if q is not None and q.shape[-1] > 128:
        raise NotImplementedError(f"ring_flash_attn: {what} with {feature} serves head dims up to 128, not {q.shape[-1]}")
    if v is not None and v.shape[-1] != q.shape[-1]:
        raise NotImplementedError(f"ring_flash_attn: {what} with {feature} does not serve a value head dim ({v.shape[-1]}) "
                                  f"that differs from q's ({q.shape[-1]})")
    if backend is not None:
        be = get_backend()
        if not getattr(be, backend[0], False):
            raise NotImplementedError(f"ring_flash_attn: {what} with {feature} needs a backend that serves {backend[1]}; "
                                      f"{getattr(be, 'name', type(be).__name__)!r} does not")


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
    _refuse(what, "alibi_slopes", q)
    require_alibi(get_backend(), what)
    return slopes


def checked_softcap(dropout_p, alibi_slopes, q, what, window_size=None, causal=False):
    """the soft cap bound to this public call by `with_softcap` (0.0: none) and its refusals — together with dropout or
    alibi_slopes, head dims above 128, a window at head dims 65 .. 127 (include/rfa.h: that dK/dV instance is not built; a
    window_size (-1, 0) with `causal` bounds nothing), a backend that does not serve a cap: NotImplementedError before anything is
    exchanged, on every rank alike.  Read ONCE, in the autograd Function's forward, and kept on the node: the backward runs
    under `softcap_scope(ctx.softcap)` and reads nothing ambient."""
    from .backend import pending_softcap

    cap = pending_softcap()
    if not cap:
        return 0.0
    _refuse(what, "softcap", q, dropout_p=dropout_p, alibi_slopes=alibi_slopes)
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
    _refuse(what, "a value head dim that differs from q's", backend=("serves_vdim", "it (serves_vdim)"))
    return True


# ---- the binders: one table, one resolver, one wrapper ---------------------------------------------------------------------
# A binder (with_softcap, with_sinks ...) takes one of the package's public attention functions — or another binder's result,
# where the table says so — and returns a callable with the same signature that runs it with a value bound to the call.  Which
# binder takes what is a rule of the package, and `_RULES` is the one place it is written down: a row names the attribute the
# binder's results carry, the public functions it serves, the binders whose results (of a served function) it takes as well,
# what it answers to everything else, and the answers of its own to particular binders' results.
ROW_RANGE_FUNCS = tuple(f"{p}_{s}" for p in ("ring_flash_attn", "zigzag_ring_flash_attn") for s in ("func", "kvpacked_func", "qkvpacked_func"))
DENSE_FUNCS = ROW_RANGE_FUNCS + tuple(f"stripe_flash_attn_{s}" for s in ("func", "kvpacked_func", "qkvpacked_func"))


class _Rule(NamedTuple):
    marker: str                       # the attribute its results carry
    serves: Optional[tuple]           # the public functions it binds (None: all 21)
    over: tuple                       # the binders whose results, of a served function, it binds as well
    expects: str                      # TypeError for anything else, up to the repr of `func`
    refuses: dict                     # binder -> TypeError of its own for that binder's results


def _not_served(*binders):
    return {b: f"`func` is a {b} result; not served" for b in binders}


_ANY_FUNC = "`func` must be one of the package's public attention functions (ring_flash_attn.*_func)"
_RANGED_FUNC = ("`func` must be one of ring_flash_attn_{,kvpacked_,qkvpacked_}func and zigzag_ring_flash_attn_{,kvpacked_,qkvpacked_}func "
                "or a with_lse_grad result of one, got ")
_RULES = {
    "with_softcap": _Rule("_rfa_softcap", None, (), _ANY_FUNC + ", got ", {}),
    "with_sinks": _Rule("_rfa_sinks", None, (), _ANY_FUNC + ", got ", {
        "with_softcap": "`func` is a with_softcap result; soft-capping together with sinks is not served yet (the cap and the "
                        "sinks would have to be bound to one call)"}),
    "with_max_logit": _Rule("_rfa_max_logit", None, ("with_softcap", "with_sinks"),
                            _ANY_FUNC + " or a with_softcap / with_sinks result of one, got ", {
        "with_ulysses": "`func` is a with_ulysses result; the exchange renumbers the heads a rank computes — not served yet "
                        "(bind with_max_logit to the function and read the head slices)",
        "with_max_logit": "`func` is a with_max_logit result already"}),
    "with_lse_grad": _Rule("_rfa_lse_grad", None, ("with_softcap",), _ANY_FUNC + " or a with_softcap result of one, got ",
                           _not_served("with_lse_grad", "with_sinks", "with_max_logit", "with_ulysses")),
    "with_row_ranges": _Rule("_rfa_row_ranges", ROW_RANGE_FUNCS, ("with_lse_grad",), _RANGED_FUNC,
                             _not_served("with_row_ranges", "with_softcap", "with_sinks", "with_max_logit", "with_ulysses")),
    "with_block_mask": _Rule("_rfa_block_mask", ROW_RANGE_FUNCS, ("with_lse_grad",), _RANGED_FUNC,
                             _not_served("with_block_mask", "with_row_ranges", "with_softcap", "with_sinks", "with_max_logit",
                                         "with_ulysses")),
    "with_ulysses": _Rule("_rfa_ulysses", DENSE_FUNCS, ("with_softcap",),
                          "`func` must be one of the nine dense functions (ring_, zigzag_ring_ and "
                          "stripe_flash_attn_{,kvpacked_,qkvpacked_}func) or a with_softcap result of one; the *_varlen families, "
                          "llama3_* and zigzag_llama3_* are a follow-up; got ", {
        "with_sinks": "`func` is a with_sinks result; sinks are per head and would need slicing and a scattered gradient under "
                      "the head exchange: follow-up",
        "with_ulysses": "`func` is already a with_ulysses result"}),
}
_public = {}                          # id -> name of the package's 21 public attention functions (made at the first bind)


def _resolve(func):
    """(the public name `func` leads to or None, the binders passed on the way — outermost first).  A binder's result
    carries its marker on both of its layers (the callable and its dynamo-opaque wrapper) and leads, by `__wrapped__`, to what
    it wraps."""
    if not _public:
        import ring_flash_attn as pkg

        _public.update((id(getattr(pkg, n)), n) for n in dir(pkg) if n.endswith("_func"))
    passed, f = [], func
    while id(f) not in _public:
        binder = next((b for b, rule in _RULES.items() if getattr(f, rule.marker, False)), None)
        if binder is None:
            return None, tuple(passed)
        if not passed or passed[-1] != binder:
            passed.append(binder)
        if not hasattr(f, "__wrapped__"):
            return None, tuple(passed)
        f = f.__wrapped__
    return _public[id(f)], tuple(passed)


def _admit(binder, func, who=None):
    """the public name behind `func` if the table lets `binder` bind it; TypeError — in the name of `who`, the binder itself
    by default — otherwise"""
    rule = _RULES[binder]
    name, passed = _resolve(func)
    if passed and passed[0] in rule.refuses:
        raise TypeError(f"ring_flash_attn.{who or binder}: {rule.refuses[passed[0]]}")
    if (name is None or (rule.serves is not None and name not in rule.serves)
            or not (passed == () or (len(passed) == 1 and passed[0] in rule.over))):
        raise TypeError(f"ring_flash_attn.{who or binder}: {rule.expects}{func!r}")
    return name


class _binding:
    """`with _binding(var, value):` — the context variable holds `value` inside"""
    __slots__ = ("var", "value", "token")

    def __init__(self, var, value):
        self.var, self.value = var, value

    def __enter__(self):
        self.token = self.var.set(self.value)

    def __exit__(self, *exc):
        self.var.reset(self.token)
        return False


def _bind(binder, func, scope=None, before=None, body=None):
    """`binder`'s result for `func`: a callable with func's signature and name that runs every call inside a fresh `scope()`
    (a context manager: the value is bound for the duration of the call and nothing stays behind it, raised or returned),
    after `before(args, kwargs)` where the binder checks something per call — or runs `body(*args, **kwargs)`, for a binder
    that does more around `func` than bind a value; marked as the table says; opaque to dynamo."""
    if body is None:
        def body(*args, **kwargs):
            if before is not None:
                before(args, kwargs)
            with scope():
                return func(*args, **kwargs)

    # (updated=(): `func`'s own attributes are not copied — a function that is already opaque to dynamo carries the marker
    #  that makes torch.compiler.disable unwrap to ITS original, which would drop this wrapper; another binder's marker is
    #  not carried over either)
    bound = functools.wraps(func, updated=())(body)
    setattr(bound, _RULES[binder].marker, True)
    return _opaque(bound)


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
    from .backend import check_softcap

    _admit("with_softcap", func)
    cap = check_softcap(softcap)
    if not cap:
        return func
    return _bind("with_softcap", func, lambda: softcap_scope(cap))


# ---- a gradient for the returned lse (ring_flash_attn.with_lse_grad) ------------------------------------------------------
# lse_i = log sum_j exp(s_ij), so d lse_i / d s_ij = P_ij: a gradient g_i on lse_i adds g_i P_ij to dS = P (dP - delta).  Every
# backward kernel is therefore served, unchanged, by delta' = delta - g (include/rfa.h: rfa_bwd_preprocess_lse): the ONE place a
# schedule's backward computes delta takes `dlse=`.  The binding is read once, at the public entry of the forward, and kept on
# the node (ctx.lse_grad); a backward reads ctx and the gradients autograd hands it, nothing ambient.  An unbound node is the
# node it always was: it never looks at the gradient of lse.
_lse_grad = contextvars.ContextVar("ring_flash_attn_lse_grad", default=False)


def checked_lse_grad(ctx, what):
    """True inside a call bound by `with_lse_grad` — the node then takes undefined output gradients as None (an unused lse costs
    nothing and leaves the plain backward, bit for bit).  NotImplementedError: a backend whose bwd_preprocess does not take
    `dlse=` — before anything is exchanged, on every rank alike."""
    if not _lse_grad.get():
        return False
    _refuse(what, "a gradient for lse", backend=("serves_lse_grad", "`lse_grad` (bwd_preprocess(dlse=))"))
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
    _admit("with_lse_grad", func)
    return _bind("with_lse_grad", func, lambda: _binding(_lse_grad, True))


# ---- per-row key ranges (ring_flash_attn.with_row_ranges) -----------------------------------------------------------------
# Row i sees key j iff start[i] <= pos(j) < end[i] and the call's own mask allows the pair: one interval of GLOBAL key positions
# per query row (FlashMask's O(S) description of document, prefix-LM, shared-prefix masks ...).  The two tensors are bound to
# the call like the gradient of lse above: read ONCE, in the autograd Function's forward, kept on the node (ctx.row_ranges) and
# handed to the schedule's forward and backward as `row_ranges=` — a backward reads nothing ambient.  The schedules give every
# block call the slice that belongs to its query rows and the global position of its key row 0 (include/rfa.h: rfa_rowrange_args).
_row_ranges = contextvars.ContextVar("ring_flash_attn_row_ranges", default=None)


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
    _refuse(what, "row ranges", q, v, dropout_p, alibi_slopes, backend=("serves_row_ranges", "`row_ranges` (serves_row_ranges)"))
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
    _admit("with_row_ranges", func)
    if (start is None) != (end is None):
        raise ValueError("ring_flash_attn.with_row_ranges: start and end come together (both tensors, or both None)")
    if start is None:
        return func
    _check_row_range_tensors(start, end)
    return _bind("with_row_ranges", func, lambda: _binding(_row_ranges, (start, end)))


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


def checked_block_mask(q, k, v, dropout_p, alibi_slopes, what, group, zigzag=False):
    """the mask bound to this public call by `with_block_mask`, or None.  ValueError: a mask that does not fit the call, local
    lengths that are no multiple of the block on a multi-rank group.  NotImplementedError: dropout, alibi_slopes, head dims
    above 128, more than 64 query heads per K/V head, a value head dim of its own, a backend without `serves_block_mask` — all before anything is exchanged, from
    numbers every rank has alike.  zigzag: the schedule's local rows are two chunks (ScheduleSpec.zigzag)."""
    mask = _block_mask.get()
    if mask is None:
        return None
    from .utils import group_rank_world

    _check_block_mask_tensor(mask)
    world = group_rank_world(group)[1]
    B, Sq, H = q.shape[0], q.shape[1], q.shape[2]
    Sk = k.shape[1]
    if world > 1:
        unit, per = (Sq // 2, "half of the local length") if zigzag else (Sq, "the local length")
        if Sq != Sk or (zigzag and Sq % 2) or unit % BLOCK_MASK_SIZE:
            raise ValueError(f"ring_flash_attn: {what} with a block mask on {world} ranks needs {per} to be a multiple of "
                             f"{BLOCK_MASK_SIZE}; got a local length of {Sq} (keys: {Sk})")
    nq, nk = -(-Sq // BLOCK_MASK_SIZE), -(-(world * Sk) // BLOCK_MASK_SIZE)
    if (mask.shape[0] not in (1, B) or mask.shape[1] not in (1, H) or tuple(mask.shape[2:]) != (nq, nk) or mask.device != q.device):
        raise ValueError(f"ring_flash_attn: {what}: block_mask must be ({{1, {B}}}, {{1, {H}}}, {nq}, {nk}) on {q.device} — this "
                         f"rank's query blocks against the key blocks of the whole sequence; got {tuple(mask.shape)} on {mask.device}")
    _refuse(what, "a block mask", q, dropout_p=dropout_p, alibi_slopes=alibi_slopes)
    if k.shape[2] > 0 and H // k.shape[2] > BLOCK_MASK_MAX_GROUP:
        raise NotImplementedError(f"ring_flash_attn: {what} with a block mask serves at most {BLOCK_MASK_MAX_GROUP} query heads per "
                                  f"K/V head, not {H} / {k.shape[2]}")
    _refuse(what, "a block mask", q, v, backend=("serves_block_mask", "`block_mask` (serves_block_mask)"))
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
    _admit("with_block_mask", func)
    if block_mask is None:
        return func
    _check_block_mask_tensor(block_mask)
    return _bind("with_block_mask", func, lambda: _binding(_block_mask, block_mask))


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
        out, lse = get_backend().merge_pair(out_a, lse_a, out_b, lse_b)
        ctx.save_for_backward(out_a, lse_a, out_b, lse_b)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, dlse):
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
    _refuse(what, "sinks", backend=("serves_sinks", "`sink_apply` / `sink_grad`"))
    return sinks


def apply_sinks(sinks, out, lse):
    """(out', lse') of the call with sinks from the schedule's merged (out, lse); the pair itself without sinks"""
    if sinks is None:
        return out, lse
    return get_backend().sink_apply(out, lse, sinks, varlen=out.dim() == 3)


def sinks_grad(ctx, sinks, dout, out, lse):
    """the tail of a backward's gradients for the trailing `sinks` input: () without one, else (dsink,) — this rank's sum over
    its own query rows, in sinks' dtype (None when sinks needs no gradient)"""
    if sinks is None:
        return ()
    if not ctx.needs_input_grad[-1]:
        return (None,)
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
    _admit("with_sinks", func)
    if sinks is None:
        return func
    if not isinstance(sinks, torch.Tensor) or not sinks.is_floating_point() or sinks.dim() != 1:
        raise ValueError("ring_flash_attn.with_sinks: sinks must be a floating tensor of shape (H,), one logit per query "
                         f"head; got {tuple(sinks.shape) if isinstance(sinks, torch.Tensor) else sinks!r}")
    return _bind("with_sinks", func, lambda: _binding(_sinks, sinks))


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
    from .backend import max_logit_scope, require_max_logit

    name = _admit("with_max_logit", func)
    if max_logit is None:
        return func
    _check_max_logit_tensor(max_logit)
    sig = inspect.signature(func)

    def check_call(args, kwargs):
        bound = sig.bind(*args, **kwargs).arguments
        _check_max_logit_tensor(max_logit, next(iter(bound.values())))
        scale = bound.get("softmax_scale", None)
        if scale is not None and not scale > 0:
            raise ValueError(f"ring_flash_attn.with_max_logit: softmax_scale must be positive, got {scale!r}")
        require_max_logit(name + " with max_logit")

    return _bind("with_max_logit", func, lambda: max_logit_scope(max_logit), before=check_call)


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


class ScheduleSpec(NamedTuple):
    """What one schedule family is, said once (at the end of its module) and read by the node factory and the API factory:
    name            of its autograd Function, which is what a refusal's message names ("RingFlashAttnFunc")
    prefix          of its three public functions ("ring_flash_attn" -> ring_flash_attn_{,kvpacked_,qkvpacked_}func)
    n_lead          non-tensor positional arguments between (q, k, v) and the common tail: 0 for the batch API, 2 =
                    (cu_seqlens, max_seqlen) for varlen
    pack_dim        the dimension `kv` / `qkv` stack their tensors on
    window_ring     it serves a sliding window on a multi-rank group (every ring family does)
    dropout_ring    it serves dropout there (the dense ring, zigzag and stripe schedules: every block call is told the global
                    positions of its rows, _common.dropout_arg)
    alibi_ring      it serves alibi_slopes there (the dense ring and zigzag schedules)
    vdim            it serves a `v` whose head dim differs from q's (the five ring-type families, on any group: checked_vdim)
    zigzag          a rank's rows are two chunks of the sequence
    must_be_causal  the layout only means something for causal attention
    packed_travel   the schedule exchanges a packed `kv` as one buffer and writes dK/dV straight into the packed gradient
                    (`out_grads`) at any world size"""
    name: str
    prefix: Optional[str] = None
    n_lead: int = 0
    pack_dim: int = 2
    window_ring: bool = False
    dropout_ring: bool = False
    alibi_ring: bool = False
    vdim: bool = False
    zigzag: bool = False
    must_be_causal: bool = False
    packed_travel: bool = False


def call_preamble(ctx, what, q, k, v, sinks, dropout_p, window_size, alibi_slopes, causal, group, batch, *, vdim,
                  window_ring, dropout_ring, alibi_ring, alibi_single=True, masks=None, before_alibi=None):
    """Every refusal of one public call, in the ONE order in which they have always been asked — which error wins when two
    apply is observable — before anything is exchanged, on every rank alike; called first thing by the forward of every autograd
    node of the package.  Puts what the call bound on the node (ctx.softcap, ctx.lse_grad, ctx.row_ranges, ctx.block_mask: a
    backward reads these, nothing ambient) and returns (alibi_slopes, sinks) as validated.
    what: the name the messages carry.  batch: sequences in the call, for a (batch, H) bias.  vdim: the function serves a value
    head dim of its own.  window_ring / dropout_ring / alibi_ring: it serves these on a multi-rank group (on a single-rank one
    every function does; alibi_single False: not even there).  masks: the ScheduleSpec of a family that row ranges and block
    masks can be bound to; None — the llama3 families, which the binders never let such a binding reach — reads neither.
    before_alibi(alibi_slopes): a refusal of the function's own that belongs in front of the bias' validation."""
    checked_vdim(q, k, v, dropout_p, alibi_slopes, what, served=vdim)
    single = window_ok_for(group)
    _check_unsupported(dropout_p, window_size, alibi_slopes, windows_ok=single or window_ring, dropout_ok=single or dropout_ring,
                       alibi_ok=(single and alibi_single) or alibi_ring)
    if before_alibi is not None:
        before_alibi(alibi_slopes)
    alibi_slopes = checked_alibi(alibi_slopes, q, batch, what)
    ctx.softcap = checked_softcap(dropout_p, alibi_slopes, q, what, window_size, causal)
    ctx.lse_grad = checked_lse_grad(ctx, what)
    ctx.row_ranges = ctx.block_mask = None
    if masks is not None:
        ctx.row_ranges = checked_row_ranges(q, k, v, dropout_p, alibi_slopes, what)
        ctx.block_mask = checked_block_mask(q, k, v, dropout_p, alibi_slopes, what, group, zigzag=masks.zigzag)
    return alibi_slopes, checked_sinks(sinks, q, what)


def _node_forward(ctx, spec, what, forward_impl, q, k, v, rest, packed_travel=False):
    """the forward of every generic autograd Function: (q, k, v) as the adapter selected them, `rest` = the lead arguments,
    the eight of the common tail and, inside a with_sinks call, the sinks"""
    n_lead = spec.n_lead
    rest, sinks = split_sinks(rest, n_lead + 8)
    lead = rest[:n_lead]
    (dropout_p, softmax_scale, causal, window_size, alibi_slopes, deterministic,
     return_softmax, group) = rest[n_lead:]
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    alibi_slopes, sinks = call_preamble(
        ctx, what, q, k, v, sinks, dropout_p, window_size, alibi_slopes, causal, group, (len(lead[0]) - 1) if n_lead else q.shape[0],
        vdim=spec.vdim, window_ring=spec.window_ring, dropout_ring=spec.dropout_ring, alibi_ring=spec.alibi_ring, masks=spec)
    q, k, v = _prep_qkv(q, k, v, group, packed_travel=packed_travel)
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
    audit_verify(group, f"{what} forward")          # (config.exchange_check: a no-op otherwise)
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


def _node_backward(ctx, spec, what, backward_impl, dout, args, out_grads=None):
    """the backward of every generic autograd Function -> ((dq, dk, dv), the gradients of everything behind the tensors: None
    for the plain arguments, the sinks' gradient inside a with_sinks call).  out_grads: (dq, dk, dv) views the schedule is to
    write into, None where it allocates (the packed adapters); it may still return tensors of its own (W > 1)."""
    q, k, v, out, softmax_lse, *more = ctx.saved_tensors
    sinks = more.pop() if ctx.has_sinks else None
    tensors_lead, extra = _split_kept(ctx, more)
    dout, lse_kw = lse_grad_kw(ctx, dout, args, out, softmax_lse)
    extra.update(lse_kw)
    extra.update(row_ranges_extra(ctx))
    extra.update(block_mask_extra(ctx))
    if ctx.dropout[1] is not None:
        extra["dropout_seed"] = ctx.dropout[1]
    if out_grads is not None:
        extra["out_grads"] = out_grads
    with softcap_scope(ctx.softcap):
        grads = backward_impl(
            ctx.group, dout, q, k, v, out, softmax_lse, *tensors_lead, *ctx.lead_rest,
            softmax_scale=ctx.softmax_scale, dropout_p=ctx.dropout[0], causal=ctx.causal,
            window_size=ctx.window_size, alibi_slopes=ctx.alibi_slopes, deterministic=ctx.deterministic, **extra,
        )
    _release_kept(ctx)
    audit_verify(ctx.group, f"{what} backward")
    return tuple(grads), (None,) * (spec.n_lead + 8) + sinks_grad(ctx, sinks, dout, out, softmax_lse)


def make_autograd_function(spec, forward_impl, backward_impl, n_lead=0, **serves):
    """the autograd Function of a family's (q, k, v) entry from its schedule's `*_forward` / `*_backward`.  spec: the
    family's ScheduleSpec — or the Function's name, with n_lead and the spec's `window_ring`, `dropout_ring`, `alibi_ring`,
    `vdim` as keywords."""
    if not isinstance(spec, ScheduleSpec):
        spec = ScheduleSpec(name=spec, n_lead=n_lead, **serves)

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v, *rest):
            return _node_forward(ctx, spec, spec.name, forward_impl, q, k, v, rest)

        @staticmethod
        def backward(ctx, dout, *args):
            grads, tail = _node_backward(ctx, spec, spec.name, backward_impl, dout, args)
            return grads + tail

    _Fn.__name__ = _Fn.__qualname__ = spec.name
    return _Fn


def _packed_function(spec, forward_impl, backward_impl, n_packed):
    """autograd Function for the packed entry points (`kv` = 2 tensors, `qkv` = 3 tensors stacked on spec.pack_dim).  Same
    math as the family's plain Function; the only difference is where the gradients land: ONE packed
    buffer whose slices are handed to the schedule as output views (`out_grads`), instead of letting
    autograd build the packed gradient from three slice-gradients (zero-fill + copy + add kernels
    per step); a gradient the schedule returned in a tensor of its own (W > 1) is copied into its slice."""
    what = spec.name + ("KVPacked" if n_packed == 2 else "QKVPacked")
    n_own = 3 - n_packed                                # tensors in front of the packed one: q of (q, kv), none of (qkv,)

    class _PFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *args):
            packed = args[n_own]
            ctx.packed_meta = (packed.shape, packed.dtype, packed.device)
            # (one packed tensor has one width, so the preamble's checked_vdim has nothing to refuse here)
            return _node_forward(ctx, spec, what, forward_impl, *args[:n_own], *(packed.select(spec.pack_dim, i) for i in range(n_packed)),
                                 args[n_own + 1:], packed_travel=spec.packed_travel and n_packed == 2)

        @staticmethod
        def backward(ctx, dout, *args):
            shape, dtype, device = ctx.packed_meta
            dpacked = torch.empty(shape, dtype=dtype, device=device)
            views = tuple(dpacked.select(spec.pack_dim, i) for i in range(n_packed))
            grads, tail = _node_backward(ctx, spec, what, backward_impl, dout, args, out_grads=(None,) * n_own + views)
            for view, g in zip(views, grads[n_own:]):
                if g.data_ptr() != view.data_ptr():       # schedule returned its own tensor
                    view.copy_(g)
            return grads[:n_own] + (dpacked,) + tail

    _PFn.__name__ = _PFn.__qualname__ = what
    return _PFn


def _grad_buffers(out_grads, q, k, v):
    """(dq, dk, dv) output tensors for the single-GPU path: caller-provided views or fresh."""
    og = out_grads or (None, None, None)
    return (og[0] if og[0] is not None else (torch.empty_like(q) if q is not None else None),
            og[1] if og[1] is not None else torch.empty_like(k),
            og[2] if og[2] is not None else torch.empty_like(v))


def make_api(spec, fn, forward_impl, backward_impl):
    """(func, kvpacked_func, qkvpacked_func) of a family: the (B,S,H,D) API, or with spec.n_lead == 2 the (T,H,D) +
    (cu_seqlens, max_seqlen) one.  fn: the family's autograd Function (make_autograd_function with the same spec); the packed
    entry points get Functions of their own (gradients land in ONE packed buffer, see _packed_function)."""
    from . import _ops

    kv_fn, qkv_fn = (_packed_function(spec, forward_impl, backward_impl, n) for n in (2, 3))
    if spec.n_lead == 0:
        def func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                 alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
            return fn.apply(q, k, v, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                            deterministic, return_attn_probs, group, *sink_args())

        def kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                          alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
            return kv_fn.apply(q, kv, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                               deterministic, return_attn_probs, group, *sink_args())

        def qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                           alibi_slopes=None, deterministic=False, return_attn_probs=False, group=None):
            return qkv_fn.apply(qkv, dropout_p, softmax_scale, causal, window_size, alibi_slopes,
                                deterministic, return_attn_probs, group, *sink_args())
    else:
        def func(q, k, v, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                 window_size=(-1, -1), alibi_slopes=None, deterministic=False, return_attn_probs=False,
                 group=None):
            return fn.apply(q, k, v, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                            alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

        def kvpacked_func(q, kv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                          window_size=(-1, -1), alibi_slopes=None, deterministic=False,
                          return_attn_probs=False, group=None):
            return kv_fn.apply(q, kv, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                               alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

        def qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), alibi_slopes=None, deterministic=False,
                           return_attn_probs=False, group=None):
            return qkv_fn.apply(qkv, cu_seqlens, max_seqlen, dropout_p, softmax_scale, causal, window_size,
                                alibi_slopes, deterministic, return_attn_probs, group, *sink_args())

    # what dynamo traces instead (_compilable): the call as registered operators, from its arguments by name — one text for
    # the three forms and for both APIs (a dense call has no cu_seqlens: None, 0)
    def traced(a, windows_ok):
        if "qkv" in a:
            q, k, v = [a["qkv"].select(spec.pack_dim, i) for i in range(3)]
        elif "kv" in a:
            q, (k, v) = a["q"], [a["kv"].select(spec.pack_dim, i) for i in range(2)]
        else:
            q, k, v = a["q"], a["k"], a["v"]
        causal, window_size = a.get("causal", False), a.get("window_size", (-1, -1))
        _check_unsupported(a.get("dropout_p", 0.0), window_size, a.get("alibi_slopes", None), windows_ok=windows_ok)
        assert causal or not spec.must_be_causal, f"{spec.prefix} is meaningless for causal=False"
        return (q, k, v, a.get("cu_seqlens", None), a.get("max_seqlen", 0), a.get("softmax_scale", None), causal,
                a.get("return_attn_probs", False)), window_size

    def lower(a):
        args, window_size = traced(a, True)
        return _ops.single_device_attention(*args, window_size)

    _ops.register_schedule(spec.prefix, forward_impl, backward_impl)

    def multi(a):
        args, _ = traced(a, False)
        return _ops.multi_rank_attention(spec.prefix, *args, a.get("group", None))

    for f, suffix in ((func, "func"), (kvpacked_func, "kvpacked_func"), (qkvpacked_func, "qkvpacked_func")):
        f.__name__ = f.__qualname__ = f"{spec.prefix}_{suffix}"
    return tuple(_compilable(f, lower, multi) for f in (func, kvpacked_func, qkvpacked_func))
