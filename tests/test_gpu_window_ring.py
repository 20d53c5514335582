"""Sliding windows over multi-rank ring and zigzag schedules on the HIP kernels: W = 2, 4, 8 gloo ranks share the GPU
(the tests/_ring_worker.py pattern), head dim 128, shards of several kernel tiles, every explicit zigzag exchange
form, against ONE windowed fp64 attention over the unsharded tensors (computed on the device by rank 0).  Tolerance:
the `*_ring` kinds of tests/_tol.py.  The ring cases also check the number of block calls and exchanges against the
step rule (tests/_window_worker.py: ring_rule)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _window_worker as WW                      # noqa: E402
from conftest import free_port                   # noqa: E402

S = 512                                          # rows per rank: two 256-row forward blocks, zigzag chunks of 256


def _case(kind, W, wl, n, causal=True, wr=0, forms=("kvpacked",)):
    return dict(name=f"{kind}_w{W}_{wl}_{wr}", kind=kind, W=W, S=S, H=8, Hk=2, D=128, seed=500 + 13 * W + n, causal=causal,
                window=(wl, wr), forms=forms, check=("counts",))


def _ragged(kind, rows, window, causal, n, D=128, dtype=torch.bfloat16):
    return dict(name=f"{kind}_w4_s{rows}_{window[0]}_{window[1]}", kind=kind, W=4, S=rows, B=2, H=8, Hk=2, D=D, dtype=dtype,
                seed=900 + n, causal=causal, window=window, forms=("func",), check=("counts",))


@pytest.mark.parametrize("W", [2, 4, 8])
def test_ring_window_on_the_hip_kernels(W):
    """windows below a tile, cutting a shard, spanning shards; the last also two-sided without `causal`"""
    cases = [_case("ring", W, 100, 0, forms=("func", "kvpacked")), _case("ring", W, S + 200, 1), _case("ring", W, 2 * S, 2),
             _case("ring", W, 300, 3, causal=False, wr=S + 50, forms=("func",))]
    if W == 4:
        # shards that are no multiple of 32 rows (every mask_shift unaligned: 328, 656, 984), batch 2; head dim 64 and fp16 once
        cases += [_ragged("ring", 328, (413, 0), True, 4, D=64), _ragged("ring", 328, (150, 411), False, 5, dtype=torch.float16)]
    errs, _ = WW.run_world(W, cases, use_hip=True, port=free_port())
    assert not errs, "\n".join(errs)


_EXT = pytest.mark.extended


@pytest.mark.parametrize("W,form", [
    (2, "ring"), (4, "ring"), (4, "gather"), (4, "gather_ps"), (8, "gather"),
    pytest.param(2, "gather", marks=_EXT), pytest.param(2, "gather_ps", marks=_EXT), pytest.param(8, "ring", marks=_EXT),
    pytest.param(8, "gather_ps", marks=_EXT)])
def test_zigzag_window_on_the_hip_kernels(W, form, monkeypatch):
    """every explicit exchange form at W = 4, each world size in at least one form (the rest: extended tier)"""
    monkeypatch.setenv("RFA_ZIGZAG_EXCHANGE", form)
    cases = [_case("zigzag", W, 100, 0), _case("zigzag", W, S + 200, 1, forms=("func",))]
    if form == "ring":
        cases.append(_case("zigzag", W, 256, 2, forms=("qkvpacked",)))
    if W == 4 and form in ("ring", "gather"):
        cases.append(_ragged("zigzag", 336, (413, 0), True, 6))          # chunks of 168 rows
    errs, _ = WW.run_world(W, cases, use_hip=True, port=free_port())
    assert not errs, "\n".join(errs)
