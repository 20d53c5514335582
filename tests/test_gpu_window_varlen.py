"""Sliding windows over multi-rank varlen ring, varlen zigzag and stripe schedules on the HIP kernels: the worker of
tests/test_window_varlen_cpu.py with `use_hip=True` — W = 2 and 4 ranks sharing cuda:0 through gloo host staging, every
world under its own time limit, a failing world ends the test without retries.  Reference: per sequence, ONE windowed
fp64 attention over the unsharded sequence; tolerances TOL_HIP of tests/_ring_worker.py (tests/_tol.py kinds).  The packed
batch has local lengths on both sides of 32 / 64 / 256 rows (full lengths W * {24, 72, 520}) under a window of 100: the
short sequence lies wholly inside the window on every hop, the long one is cut, and distant hops are wholly dark for it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _window_varlen_worker as WV               # noqa: E402
from conftest import free_port                   # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = ("func", "kvpacked", "qkvpacked")


def _cases(W):
    lens = [W * 24, W * 72, W * 520]
    base = dict(W=W, H=4, Hk=2, D=128, causal=True)
    return [
        dict(base, name=f"ring_varlen_w{W}_100", kind="ring_varlen", lens=lens, seed=1200 + W, window=(100, 0), forms=FORMS),
        dict(base, name=f"ring_varlen_nc_w{W}_100_40", kind="ring_varlen", lens=lens, seed=1210 + W, causal=False, window=(100, 40)),
        dict(base, name=f"zigzag_varlen_w{W}_100_ring", kind="zigzag_varlen", lens=lens, seed=1220 + W, window=(100, -1),
             exchange="ring", forms=FORMS),
        dict(base, name=f"zigzag_varlen_w{W}_100_gather", kind="zigzag_varlen", lens=lens, seed=1230 + W, window=(100, 0),
             exchange="gather", forms=("func", "kvpacked")),
        dict(base, name=f"ring_varlen_w{W}_100_d64", kind="ring_varlen", lens=lens, seed=1240 + W, window=(100, 0), D=64),
        dict(base, name=f"stripe_w{W}_wl{W}", kind="stripe", S=300, seed=1250 + W, window=(W, 0), forms=FORMS, check=("skips",)),
        dict(base, name=f"stripe_w{W}_wl130", kind="stripe", S=300, seed=1260 + W, window=(130, -1), check=("skips",)),
    ]


@pytest.mark.parametrize("W", [2, pytest.param(4, marks=pytest.mark.extended)])
def test_window_varlen_and_stripe_schedules_on_the_hip_kernels(W):
    errs = WV.run_world(W, _cases(W), use_hip=True, port=free_port(), limit_s=300)
    assert not errs, "\n".join(errs)
