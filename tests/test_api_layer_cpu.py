"""The public API layer (ring_flash_attn/_api.py, ulysses.py) without a GPU: which binder accepts which callable, which refusal
wins when a call trips two, and that nothing ambient stays bound behind a call.

The expected outcomes (tests/golden/api_layer.json) were recorded ONCE, by running `bind_outcomes()` and `call_outcomes()` of
this file on the commit before the API layer was refactored; they are data and are not regenerated: a change of the composition
rules or of a refusal's text shows up here as a difference from that record.

    binds   "<func>|<binder>[|<binder>]" -> [outcome, outcome with a None value]: each of the 21 `*_func`, each of the seven
            binders applied to it, and each binder applied to every result that was accepted.  An outcome is "accepted", or
            "<exception type>: <message>" with the repr of `func` replaced by <FUNC>; for a None value it is "func itself" where
            the binder handed `func` back ("-": with_lse_grad binds no value).
    calls   "<case>" -> "<exception type>: <message>" of calls on the CPU test backend that trip more than one refusal."""
import inspect
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_layer.json")
BINDERS = ("softcap", "sinks", "max_logit", "lse_grad", "row_ranges", "block_mask", "ulysses")


def _ambient_is_default():
    """nothing stays bound behind a bind or a call: the four bindings of _api read their defaults"""
    from ring_flash_attn import _api

    assert _api._row_ranges.get() is None and _api._block_mask.get() is None
    assert _api._sinks.get() is None and _api._lse_grad.get() is False


def _binders():
    """name -> (bind(func), bind_none(func) or None)"""
    import ring_flash_attn as R

    s, e = torch.zeros(2, 64, dtype=torch.int32), torch.full((2, 64), 64, dtype=torch.int32)
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    ug, _ = R.make_usp_groups(R.ring_flash_attn_func, 1)
    return {
        "softcap": (lambda f: R.with_softcap(f, 30.0), lambda f: R.with_softcap(f, None)),
        "sinks": (lambda f: R.with_sinks(f, torch.zeros(4)), lambda f: R.with_sinks(f, None)),
        "max_logit": (lambda f: R.with_max_logit(f, torch.full((4,), float("-inf"))), lambda f: R.with_max_logit(f, None)),
        "lse_grad": (R.with_lse_grad, None),
        "row_ranges": (lambda f: R.with_row_ranges(f, s, e), lambda f: R.with_row_ranges(f, None, None)),
        "block_mask": (lambda f: R.with_block_mask(f, mask), lambda f: R.with_block_mask(f, None)),
        "ulysses": (lambda f: R.with_ulysses(f, ug), lambda f: R.with_ulysses(f, None)),
    }


def _outcome(bind, func):
    """(outcome, result or None)"""
    try:
        res = bind(func)
    except Exception as exc:        # noqa: BLE001 (the type is part of the record)
        return f"{type(exc).__name__}: {str(exc).replace(repr(func), '<FUNC>')}", None
    finally:
        _ambient_is_default()
    return ("func itself", None) if res is func else ("accepted", res)


def bind_outcomes():
    """the table of the module docstring, and (key, func, result) of every accepted bind"""
    import ring_flash_attn as R

    binders = _binders()
    names = sorted(n for n in dir(R) if n.endswith("_func"))
    assert len(names) == 21
    table, accepted = {}, []
    level = [(n, getattr(R, n)) for n in names]
    for _depth in range(2):
        nxt = []
        for key, func in level:
            for b in BINDERS:
                bind, bind_none = binders[b]
                out, res = _outcome(bind, func)
                table[f"{key}|{b}"] = [out, _outcome(bind_none, func)[0] if bind_none else "-"]
                if res is not None:
                    accepted.append((f"{key}|{b}", func, res))
                    nxt.append((f"{key}|{b}", res))
        level = nxt
    return table, accepted


@pytest.fixture(scope="module")
def golden_api():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def binds(single_rank_group):
    return bind_outcomes()


def test_every_binder_on_every_function_and_on_every_accepted_result(binds, golden_api):
    table, _ = binds
    want = golden_api["binds"]
    assert sorted(table) == sorted(want)
    wrong = [f"{k}: {table[k]} != {want[k]}" for k in sorted(want) if table[k] != want[k]]
    assert not wrong, f"{len(wrong)} of {len(want)} differ\n" + "\n".join(wrong[:10])


def test_the_recorded_pattern_is_the_documented_one(golden_api):
    """the shape of the record itself: what each binder takes besides the plain functions it serves; everything else TypeError"""
    import ring_flash_attn as R

    want = golden_api["binds"]
    names = sorted(n for n in dir(R) if n.endswith("_func"))
    dense = [n for n in names if "varlen" not in n]
    ranged = list(R._api.ROW_RANGE_FUNCS)
    assert len(dense) == 9 and len(ranged) == 6
    serves = {"softcap": names, "sinks": names, "max_logit": names, "lse_grad": names, "row_ranges": ranged, "block_mask": ranged,
              "ulysses": dense}
    takes = {"max_logit": ("softcap", "sinks"), "lse_grad": ("softcap",), "row_ranges": ("lse_grad",), "block_mask": ("lse_grad",),
             "ulysses": ("softcap",), "softcap": (), "sinks": ()}
    for key, (out, none) in want.items():
        name, *chain = key.split("|")
        ok = name in serves[chain[-1]] and (len(chain) == 1 or (chain[0] in takes[chain[-1]] and name in serves[chain[0]]))
        assert (out == "accepted") == ok, key
        assert out == "accepted" or out.startswith("TypeError: "), key
        assert none == ("-" if chain[-1] == "lse_grad" else "func itself" if ok else out), key
    assert sum(out == "accepted" for out, _ in want.values()) == 21 * 4 + 6 * 2 + 9 + 21 * 3 + 6 * 2 + 9


def test_accepted_results_keep_the_signature_and_the_name(binds):
    _, accepted = binds
    assert accepted
    for key, func, res in accepted:
        assert inspect.signature(res) == inspect.signature(func), key
        assert res.__name__ == func.__name__ == key.split("|")[0], key


# ---------------------------------------------------------------------------------------------- refusal order at the call
def _qkv(D=64, Dv=None, S=128, H=4, Hk=2, B=2):
    g = torch.Generator().manual_seed(7)
    return (torch.randn(B, S, H, D, generator=g).bfloat16(), torch.randn(B, S, Hk, D, generator=g).bfloat16(),
            torch.randn(B, S, Hk, Dv or D, generator=g).bfloat16())


def _call_cases():
    """name -> a call that trips more than one refusal"""
    import ring_flash_attn as R

    slopes = torch.full((4,), 0.5)
    s, e = torch.zeros(2, 128, dtype=torch.int32), torch.full((2, 128), 128, dtype=torch.int32)
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    cu = torch.tensor([0, 100, 256], dtype=torch.int32)

    def packed(q, k, v):
        return q.reshape(-1, *q.shape[2:]), k.reshape(-1, *k.shape[2:]), v.reshape(-1, *v.shape[2:])

    def kv(k, v, dim):
        return torch.stack((k, v), dim)

    q160 = _qkv(D=160)
    q, k, v = _qkv()
    cases = {
        "softcap+dropout+D160": lambda: R.with_softcap(R.ring_flash_attn_func, 30.0)(*q160, dropout_p=0.1),
        "softcap+dropout+D160 kvpacked": lambda: R.with_softcap(R.zigzag_ring_flash_attn_kvpacked_func, 30.0)(
            q160[0], kv(q160[1], q160[2], 2), dropout_p=0.1, causal=True),
        "softcap+alibi+D160 varlen": lambda: R.with_softcap(R.ring_flash_attn_varlen_func, 30.0)(
            *packed(*q160), cu, 156, alibi_slopes=slopes),
        "softcap+dropout+D160 llama3": lambda: R.with_softcap(R.llama3_flash_attn_varlen_func, 30.0)(
            *packed(*q160), cu, cu, 156, 156, 1, slice(0, 256), dropout_p=0.1),
        "softcap+dropout+window": lambda: R.with_softcap(R.stripe_flash_attn_func, 30.0)(q, k, v, dropout_p=0.1, window_size=(8, 0),
                                                                                          causal=True),
        "row_ranges+alibi+vdim 192/128": lambda: R.with_row_ranges(R.ring_flash_attn_func, s, e)(*_qkv(D=192, Dv=128), alibi_slopes=slopes),
        "row_ranges+alibi+vdim 64/32": lambda: R.with_row_ranges(R.zigzag_ring_flash_attn_func, s, e)(*_qkv(D=64, Dv=32), alibi_slopes=slopes,
                                                                                                       causal=True),
        "row_ranges+alibi+dropout": lambda: R.with_row_ranges(R.ring_flash_attn_func, s, e)(q, k, v, alibi_slopes=slopes, dropout_p=0.1),
        "row_ranges+alibi+D160": lambda: R.with_row_ranges(R.ring_flash_attn_func, s, e)(*q160, alibi_slopes=slopes),
        "row_ranges+dropout qkvpacked": lambda: R.with_row_ranges(R.ring_flash_attn_qkvpacked_func, s, e)(
            torch.stack((q, q, q), 2), dropout_p=0.1),
        "block_mask on varlen": lambda: R.with_block_mask(R.ring_flash_attn_varlen_func, mask)(*packed(q, k, v), cu, 156, dropout_p=0.1),
        "block_mask+dropout+alibi": lambda: R.with_block_mask(R.ring_flash_attn_func, mask)(q, k, v, dropout_p=0.1, alibi_slopes=slopes),
        "block_mask+dropout+D160": lambda: R.with_block_mask(R.zigzag_ring_flash_attn_func, mask)(*q160, dropout_p=0.1, causal=True),
        "block_mask+dropout kvpacked": lambda: R.with_block_mask(R.ring_flash_attn_kvpacked_func, mask)(q, kv(k, v, 2), dropout_p=0.1),
        "block_mask of a wrong shape+dropout": lambda: R.with_block_mask(R.ring_flash_attn_func, torch.ones(1, 1, 2, 2, dtype=torch.bool))(
            q, k, v, dropout_p=0.1),
        "lse_grad+softcap+dropout": lambda: R.with_lse_grad(R.with_softcap(R.ring_flash_attn_func, 30.0))(q, k, v, dropout_p=0.1),
        "sinks of a wrong length+dropout out of range": lambda: R.with_sinks(R.ring_flash_attn_func, torch.zeros(3))(q, k, v, dropout_p=1.5),
        "sinks without a backend for them+alibi (B, H) zigzag_llama3": lambda: R.with_sinks(R.zigzag_llama3_flash_attn_varlen_func, torch.zeros(4))(
            *packed(q, k, v), cu, alibi_slopes=torch.full((2, 4), 0.5), causal=True),
        "dropout zigzag_llama3+softcap": lambda: R.with_softcap(R.zigzag_llama3_flash_attn_varlen_func, 30.0)(
            *packed(q, k, v), cu, dropout_p=0.1, causal=True),
        "vdim llama3+dropout": lambda: R.llama3_flash_attn_varlen_func(*packed(*_qkv(D=192, Dv=128)), cu, cu, 156, 156, 1, slice(0, 256),
                                                                       dropout_p=0.1),
        "max_logit+softcap+dropout": lambda: R.with_max_logit(R.with_softcap(R.ring_flash_attn_func, 30.0), torch.full((4,), float("-inf")))(
            q, k, v, dropout_p=0.1),
    }
    return cases


def call_outcomes():
    from ring_flash_attn import _testing
    from _blockmask_backend import BlockMaskBackend

    # (serves everything the cases bind but sinks and a value head dim of its own; max_logit is asked of it at the call)
    _testing.set_backend(BlockMaskBackend(serves=("mask_shift", "mask_shift_lens", "softcap", "alibi", "dropout_positions")))
    got = {}
    try:
        for name, call in _call_cases().items():
            try:
                call()
                got[name] = "accepted"
            except Exception as exc:        # noqa: BLE001
                got[name] = f"{type(exc).__name__}: " + re.sub(r"<function \w+ at 0x[0-9a-f]+>", "<FUNC>", str(exc))
            _ambient_is_default()
    finally:
        _testing.set_backend(None)
    return got


def test_the_refusal_that_wins_when_a_call_trips_two(single_rank_group, golden_api):
    got, want = call_outcomes(), golden_api["calls"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert all(w != "accepted" and "<function" not in w for w in want.values())


def test_served_calls_leave_nothing_bound(single_rank_group):
    """a forward and a backward through every binding of _api on the CPU test backend: the four bindings read their defaults
    behind the call, behind the backward, and the bound values reached the node"""
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _blockmask_backend import BlockMaskBackend
    from _sink_backend import SinkBackend

    q, k, v = _qkv(S=128)
    s, e = torch.zeros(2, 128, dtype=torch.int32), torch.full((2, 128), 128, dtype=torch.int32)
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    sinks = torch.zeros(4, requires_grad=True)
    full = BlockMaskBackend(serves=("mask_shift", "mask_shift_lens", "softcap"))
    runs = [(full, R.with_softcap(R.ring_flash_attn_func, 30.0), (q, k, v)),
            (full, R.with_row_ranges(R.with_lse_grad(R.zigzag_ring_flash_attn_func), s, e), (q, k, v)),
            (full, R.with_block_mask(R.ring_flash_attn_kvpacked_func, mask), (q, torch.stack((k, v), 2))),
            (full, R.with_lse_grad(R.ring_flash_attn_qkvpacked_func), (torch.stack((q, q, q), 2),)),
            (SinkBackend(), R.with_sinks(R.stripe_flash_attn_func, sinks), (q, k, v))]
    try:
        for be, attn, tensors in runs:
            _testing.set_backend(be)
            ins = [t.clone().requires_grad_(True) for t in tensors]
            out, lse, _ = attn(*ins, causal=True, return_attn_probs=True)
            _ambient_is_default()
            (out.float().sum() + (lse.sum() if lse.requires_grad else 0.0)).backward()
            _ambient_is_default()
            assert all(t.grad is not None and torch.isfinite(t.grad.float()).all() for t in ins)
        assert sinks.grad is not None
    finally:
        _testing.set_backend(None)
