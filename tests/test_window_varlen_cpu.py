"""Sliding windows over multi-rank `ring_flash_attn_varlen`, `zigzag_ring_flash_attn_varlen` and `stripe_flash_attn`
schedules, on the CPU: gloo worlds of 2, 3 and 4 ranks run the public functions through the oracle backend extended with
`mask_shift` and `mask_shift_lens` (tests/_ref_backend.py) and are compared, sequence by sequence, with ONE
windowed attention over the unsharded sequence (oracle.flash_attn_ref.full_attention_fp64).  Tolerance: TOL_ORACLE of
tests/_ring_worker.py with _window_worker._cmp's absolute floor.  Also: the stripe blocks that are skipped (the rule, not
a measurement), that a window covering the longest sequence takes the unwindowed path bit for bit, and that a backend
which cannot serve `mask_shift_lens` is refused before anything is exchanged."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _window_varlen_worker as WV               # noqa: E402
from conftest import free_port                   # noqa: E402

FORMS = ("func", "kvpacked", "qkvpacked")
WORLDS = [2, 3, 4]


def _lens(W):
    """full lengths, multiples of 2 W; the smallest is exactly 2 W: 1-row zigzag chunks, 2-row ring shards"""
    return [2 * W, 6 * W, 16 * W]


def _windows(W):
    """0; shorter than the shortest local shard (2 rows); between that shard and its sequence (2 W rows); longer than the
    shortest sequence and shorter than the longest (16 W >= 32 rows)"""
    return [0, 1, W + 1, 19]


def _varlen_cases(kind, W, causal=True, rights=None, **more):
    cases = []
    for n, wl in enumerate(_windows(W)):
        wr = rights[n] if rights is not None else (-1 if n % 2 else 0)
        cases.append(dict(name=f"{kind}_w{W}_{wl}_{wr}", kind=kind, W=W, lens=_lens(W), H=4, Hk=2, D=32, seed=500 + 10 * W + n,
                          causal=causal, window=(wl, wr), forms=FORMS if n < 2 else ("func",), **more))
    return cases


@pytest.mark.parametrize("W", WORLDS)
def test_ring_varlen_causal_window(W):
    errs = WV.run_world(W, _varlen_cases("ring_varlen", W), use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("W", WORLDS)
def test_ring_varlen_two_sided_window(W):
    """non-causal (left, right) windows, a one-sided one among them"""
    cases = _varlen_cases("ring_varlen", W, causal=False, rights=[0, 2, 3, 7])
    cases.append(dict(name=f"ring_varlen_nc_w{W}_right_only", kind="ring_varlen", W=W, lens=_lens(W), H=4, Hk=2, D=32,
                      seed=577 + W, causal=False, window=(-1, 5)))
    errs = WV.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("exchange", ["ring", "gather"])
@pytest.mark.parametrize("W", WORLDS)
def test_zigzag_varlen_window(W, exchange):
    errs = WV.run_world(W, _varlen_cases("zigzag_varlen", W, exchange=exchange), use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("W", WORLDS)
def test_stripe_window(W):
    """S per rank 5 and 64; every window class of the rule: one token, a neighbour on the next rank, W - 1 (the last
    window that never reaches the same rank's previous row), W, and several local rows"""
    cases = []
    for S in (5, 64):
        for n, wl in enumerate((0, 1, W - 1, W, 3 * W + 1)):
            cases.append(dict(name=f"stripe_w{W}_s{S}_wl{wl}", kind="stripe", W=W, S=S, B=2 if S == 5 else 1, H=4, Hk=2, D=32,
                              seed=700 + 10 * W + n + S, causal=True, window=(wl, 0 if n % 2 else -1),
                              forms=FORMS if (S == 5 and n in (0, 3)) else ("func",), check=("skips",)))
    errs = WV.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


def test_stripe_skip_rule():
    """the rule itself, against the blocks written down by hand for W = 4: a = rq - rk in -3 .. 3"""
    from ring_flash_attn.stripe_flash_attn import stripe_window_band

    vis = lambda wl: [a for a in range(-3, 4) if not WV.stripe_skipped(a, wl, 4)]
    # wl = 0: only the token itself (a = 0).  wl = 1: also the key one rank in front (a = 1) and, through the previous local
    # row, the key three ranks behind (a = -3: global distance W - 3 = 1).  wl = 3: every rank in front, and behind down
    # to a = -1 (distance 3).  wl = 4: the same rank's previous row comes into reach, every block holds a visible element
    assert vis(0) == [0] and vis(1) == [-3, 0, 1] and vis(3) == [-3, -2, -1, 0, 1, 2, 3] and vis(2) == [-3, -2, 0, 1, 2]
    for W in (2, 3, 4, 8):
        for wl in (0, 1, W - 1, W, 3 * W + 1, 100):
            for rq in range(W):
                for rk in range(W):
                    band = stripe_window_band(rq, rk, W, wl)
                    assert (band is None) == WV.stripe_skipped(rq - rk, wl, W), (W, wl, rq, rk)
                    if band is not None:
                        # element by element: local (i, j) is visible iff 0 <= (i W + rq) - (j W + rk) <= wl
                        for i in range(8):
                            for j in range(8):
                                d = (i * W + rq) - (j * W + rk)
                                assert (0 <= d <= wl) == (i + band[0] - band[1] <= j <= i + band[0]), (W, wl, rq, rk, i, j)


@pytest.mark.parametrize("kind", ["ring_varlen", "zigzag_varlen", "stripe"])
def test_covering_window_takes_the_unwindowed_path(kind):
    """a window that covers the whole of the longest sequence: the unwindowed call sequence, bit-identical results"""
    W = 3
    if kind == "stripe":
        cases = [dict(name="stripe_cover", kind=kind, W=W, S=5, H=4, Hk=2, D=32, seed=81, causal=True, window=(W * 5 - 1, 0),
                      forms=FORMS, check=("same_as_unwindowed",))]
    else:
        top = max(_lens(W))
        cases = [dict(name=f"{kind}_cover", kind=kind, W=W, lens=_lens(W), H=4, Hk=2, D=32, seed=82, causal=True,
                      window=(top - 1, 0), forms=FORMS, check=("same_as_unwindowed",))]
        if kind == "ring_varlen":
            cases.append(dict(name="ring_varlen_cover_nc", kind=kind, W=W, lens=_lens(W), H=4, Hk=2, D=32, seed=83, causal=False,
                              window=(top, top - 1), check=("same_as_unwindowed",)))
    errs = WV.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


def test_backend_without_mask_shift_lens_is_refused():
    """before any exchange, on every rank alike; and the helper itself"""
    from _ref_backend import RefBackend
    from ring_flash_attn._common import require_mask_shift_lens

    with pytest.raises(NotImplementedError, match="mask_shift_lens"):
        require_mask_shift_lens(RefBackend(serves=("mask_shift",)), "ring_flash_attn_varlen")
    require_mask_shift_lens(RefBackend(serves=("mask_shift", "mask_shift_lens")), "ring_flash_attn_varlen")
    W = 2
    cases = [dict(name=f"refuse_{kind}", kind="refuse", refuse=kind, W=W, lens=_lens(W), H=4, Hk=2, D=32, seed=90, causal=True,
                  window=(3, 0)) for kind in ("ring_varlen", "zigzag_varlen")]
    errs = WV.run_world(W, cases, use_hip=False, port=free_port())
    assert not errs, "\n".join(errs)


def test_band_varlen_backend_serves_the_definition():
    """the test backend against tests/_bandref.band_ref, per sequence, with shift = mask_shift_lens * len_k: packed input
    with halves, and dense input (where the field folds into mask_shift)"""
    import torch

    from _ref_backend import RefBackend
    from _bandref import band_ref

    be = RefBackend(serves=("mask_shift", "mask_shift_lens"))
    g = torch.Generator().manual_seed(5)
    lens = [4, 10, 16]
    cu = torch.tensor([0, 4, 14, 30], dtype=torch.int32)
    q, do = (torch.randn(30, 4, 16, generator=g).bfloat16() for _ in range(2))
    k, v = (torch.randn(30, 2, 16, generator=g).bfloat16() for _ in range(2))
    for n, window, causal in ((1, (3, -1), True), (-1, (2, 3), False), (2, (-1, -1), True)):
        out, lse = torch.full_like(q, 7.0), torch.full((4, 30), 7.0)
        be.fwd(q, k, v, softmax_scale=0.25, causal=causal, window=window, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=16,
               max_seqlen_k=16, q_half=2, k_half=1, out=out, lse=lse, mask_shift_lens=n)
        s = 0
        for L in lens:
            h = L // 2
            ro, rl, *_ = band_ref(q[s + h:s + L][None], k[s:s + h][None], v[s:s + h][None], do[s + h:s + L][None], causal, window, n * h)
            assert torch.allclose(out[s + h:s + L].double(), ro[0], atol=2e-2) and (out[s:s + h] == 7.0).all()
            assert torch.equal(torch.isinf(lse[:, s + h:s + L]), torch.isinf(rl[0].float()))
            fin = ~torch.isinf(rl[0])
            assert torch.allclose(lse[:, s + h:s + L][fin].double(), rl[0][fin], atol=1e-5)
            s += L
