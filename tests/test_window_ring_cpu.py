"""Sliding windows over multi-rank ring and zigzag schedules, on the CPU: gloo worlds of 2, 3, 4 and 8 ranks run the
public functions through the oracle backend extended with `mask_shift` (tests/_ref_backend.py) and are compared with
ONE windowed attention over the unsharded tensors (oracle.flash_attn_ref.full_attention_fp64).  Tolerance: TOL_ORACLE of
tests/_ring_worker.py.  Also: the number of block calls and exchanges a windowed ring makes (conditions from the step
rule, not measurements), and that a window covering the whole sequence — and every unwindowed call — takes the
unwindowed path."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _window_worker as WW                      # noqa: E402
from conftest import free_port                   # noqa: E402

FORMS = ("func", "kvpacked", "qkvpacked")
S = 16                                           # rows per rank (zigzag: chunks of 8)


def _windows(W):
    """smaller than a chunk, equal to S, spanning several ranks, 0, larger than the sequence"""
    return [5, S, 2 * S + 4, 0, W * S + 7]


def _cases(kind, W):
    cases = []
    for n, wl in enumerate(_windows(W)):
        cases.append(dict(name=f"{kind}_w{W}_wl{wl}", kind=kind, W=W, S=S, H=4, Hk=2, D=32, seed=100 + 10 * W + n, causal=True,
                          window=(wl, -1 if n % 2 else 0), forms=FORMS if n < 2 else ("func",), check=("counts",)))
    return cases


# shards that are not powers of two (appended to the W = 4 worlds below): 328 rows per rank is no multiple of 32, so every
# mask_shift of the ring (328, 656, 984) is unaligned; zigzag chunks of 168 rows likewise; batch 2
RAGGED_RING_CAUSAL = dict(name="ring_w4_s328_413", kind="ring", W=4, S=328, B=2, H=4, Hk=2, D=64, seed=911, causal=True,
                          window=(413, 0), forms=("func",), check=("counts",))
RAGGED_RING_TWO_SIDED = dict(name="ring_nc_w4_s328_150_411", kind="ring", W=4, S=328, B=2, H=4, Hk=2, D=32, seed=912,
                             causal=False, window=(150, 411), dtype=torch.float16, forms=("func",), check=("counts",))
RAGGED_ZIGZAG = dict(name="zigzag_w4_s336_413", kind="zigzag", W=4, S=336, B=2, H=4, Hk=2, D=32, seed=913, causal=True,
                     window=(413, 0), forms=("func",), check=("counts",))


@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_ring_causal_window(W):
    cases = _cases("ring", W) + ([RAGGED_RING_CAUSAL] if W == 4 else [])
    errs, _ = WW.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_zigzag_window(W, monkeypatch):
    monkeypatch.setenv("RFA_ZIGZAG_EXCHANGE", "ring")
    cases = _cases("zigzag", W) + ([RAGGED_ZIGZAG] if W == 4 else [])
    errs, _ = WW.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("form", ["gather", "gather_ps"])
@pytest.mark.parametrize("W", [2, 4])
def test_zigzag_window_gather_forms(W, form, monkeypatch):
    monkeypatch.setenv("RFA_ZIGZAG_EXCHANGE", form)
    cases = _cases("zigzag", W) + ([RAGGED_ZIGZAG] if (W, form) == (4, "gather") else [])
    errs, _ = WW.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_ring_two_sided_window(W):
    """non-causal (left, right) windows: results are required, the early stop is not (the rotation stays complete)"""
    cases = [dict(name=f"ring_nc_w{W}_{wl}_{wr}", kind="ring", W=W, S=S, H=4, Hk=2, D=32, seed=300 + 7 * W + n, causal=False,
                  window=(wl, wr), forms=("func", "kvpacked") if n == 0 else ("func",), check=("counts",))
             for n, (wl, wr) in enumerate([(5, 3), (S, 2 * S + 1), (-1, 4), (0, 0), (2 * S, -1), (W * S, W * S)])]
    if W == 4:
        cases.append(RAGGED_RING_TWO_SIDED)
    errs, _ = WW.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


def test_ring_step_counts_of_the_rule():
    """the rule itself, against the counts written down for W = 8, S = 16: block calls summed over the ranks"""
    total = lambda wl: sum(WW.ring_rule(8, 16, r, True, (wl, 0))[0] for r in range(8))
    assert [total(w) for w in (5, 8, 20, 0)] == [15, 15, 21, 8] and total(-1) == 36 and total(8 * 16) == 36
    from ring_flash_attn.ring_flash_attn import ring_window_plan

    for W in (2, 3, 4, 8):
        for wl in (0, 1, 5, 16, 17, 33, 100):
            for r in range(W):
                n_steps, dists = ring_window_plan(r, W, 16, True, (wl, -1))
                assert (sum(d is not None for d in dists), n_steps - 1) == WW.ring_rule(W, 16, r, True, (wl, 0)), (W, wl, r)


@pytest.mark.parametrize("kind", ["ring", "zigzag"])
def test_covering_window_and_unwindowed_calls_take_the_unwindowed_path(kind, monkeypatch):
    """bit-identical results and the same backend calls, in the same order; and the unwindowed calls are the parent
    commit's: no window, no shift, the step pattern of the schedule (ring: rank + 1 causal blocks, one masked)"""
    monkeypatch.setenv("RFA_ZIGZAG_EXCHANGE", "ring")
    W = 4
    cases = [dict(name=f"{kind}_cover", kind=kind, W=W, S=S, H=4, Hk=2, D=32, seed=77, causal=True, window=(W * S - 1, 0),
                  forms=FORMS, check=("same_as_unwindowed",))]
    if kind == "ring":
        cases.append(dict(name="ring_cover_nc", kind=kind, W=W, S=S, H=4, Hk=2, D=32, seed=78, causal=False,
                          window=(W * S, W * S - 1), forms=("func",), check=("same_as_unwindowed",)))
    errs, logs = WW.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)
    for r in range(W):
        log = logs[f"log:{kind}_cover:func:{r}"]
        fwd = [e for e in log if e[0] == "fwd"]
        if kind == "ring":
            assert len(fwd) == r + 1 and [dict(e[2])["causal"] for e in fwd] == [True] + [False] * r
        else:
            assert len(fwd) == W and [dict(e[2])["causal"] for e in fwd] == [True] + [False] * (W - 1)


def test_still_unsupported_combinations_raise():
    """dropout over a ring, dropout with a window, and a window on the schedules that cannot place a block (stripe, the
    varlen rings: windows_ok stays False for them) still raise, with a message that names what does work"""
    from ring_flash_attn import _api

    with pytest.raises(NotImplementedError, match="dropout"):
        _api._check_unsupported(0.1, (-1, -1), None, windows_ok=True, dropout_ok=False)
    with pytest.raises(NotImplementedError, match="dropout together"):
        _api._check_unsupported(0.1, (4, 0), None, windows_ok=True, dropout_ok=True)
    with pytest.raises(NotImplementedError, match="stripe"):
        _api._check_unsupported(0.0, (4, 0), None, windows_ok=False)
    _api._check_unsupported(0.0, (4, 0), None, windows_ok=True, dropout_ok=False)
    # a backend that cannot be told where a block sits would band every block on its own: the schedules refuse it
    from oracle.oracle_backend import OracleBackend
    from ring_flash_attn._common import require_mask_shift
    from _ref_backend import RefBackend

    with pytest.raises(NotImplementedError, match="mask_shift"):
        require_mask_shift(OracleBackend(), "ring_flash_attn")
    require_mask_shift(RefBackend(serves=("mask_shift",)), "ring_flash_attn")
