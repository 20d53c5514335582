"""The block geometries of the shifted-band tests (tests/_bandref.py: GEOMETRIES), checked on the CPU: every geometry
shows, from its boolean mask alone, what it was put on the list for (the counts below were taken from the masks when the
list was written — a later edit that turns a sharp case into a bland one fails here), every class is populated, and every
(geometry, kernel form) pair that tests/test_gpu_band_forms.py runs reports, through the host-side plan functions of the
C ABI (the library loads without a device), the form the pair names — no GPU case silently runs another form."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _bandref as BR                            # noqa: E402
import test_gpu_band_forms as GF                 # noqa: E402  (its case lists; nothing in it touches a device at import)

# name -> (visible, empty rows, empty cols, (query workgroups none, all), (256-key workgroups none, all))
EXPECTED = {
    "corner-hi": (1, 776, 999, (3, 0), (3, 0)),
    "corner-hi-1": (0, 777, 1000, (4, 0), (4, 0)),
    "corner-lo": (1, 776, 999, (3, 0), (3, 0)),
    "corner-lo+1": (0, 777, 1000, (4, 0), (4, 0)),
    "hi-live": (776999, 0, 0, (0, 3), (0, 3)),
    "hi-dropped": (777000, 0, 0, (0, 4), (0, 4)),
    "lo-live": (776999, 0, 0, (0, 3), (0, 3)),
    "lo-dropped": (777000, 0, 0, (0, 4), (0, 4)),
    "causal-333": (98790, 333, 556, (1, 0), (2, 0)),
    "causal-32": (277885, 32, 255, (0, 0), (1, 0)),
    "causal-31": (278631, 31, 254, (0, 0), (1, 0)),
    "causal+1": (303030, 0, 222, (0, 0), (0, 0)),
    "causal+31": (326340, 0, 192, (0, 0), (0, 0)),
    "causal+33": (327894, 0, 190, (0, 0), (0, 0)),
    "causal+63": (351204, 0, 160, (0, 0), (0, 0)),
    "causal+64": (351981, 0, 159, (0, 0), (0, 0)),
    "causal+65": (352758, 0, 158, (0, 0), (0, 0)),
    "causal+257": (501347, 0, 0, (0, 1), (0, 1)),
    "causal+401": (597899, 0, 0, (0, 1), (0, 1)),
    "causal+600": (697200, 0, 0, (0, 2), (0, 2)),
    "causal-63": (255255, 63, 286, (0, 0), (1, 0)),
    "rows1000-keys300-300": (165150, 300, 0, (1, 1), (0, 0)),
    "wl130-333": (49649, 333, 556, (1, 0), (2, 0)),
    "wl130+65": (99642, 0, 158, (0, 0), (0, 0)),
    "wl130+401": (86984, 48, 271, (1, 0), (1, 0)),
    "two-sided-333": (54889, 293, 516, (1, 0), (2, 0)),
    "two-sided+65": (101462, 0, 118, (0, 0), (0, 0)),
    "two-sided+401": (81744, 88, 311, (1, 0), (1, 0)),
    "rows256-keys4096+1500": (416896, 0, 2340, (0, 0), (9, 5)),
    "rows200-keys4096-100": (5050, 100, 3996, (0, 0), (15, 0)),
    "rows384-keys4096+3000": (1225920, 0, 712, (0, 0), (2, 11)),
}


def _lib():
    from ring_flash_attn import _C

    return _C, _C.load()


_plan, _chunks, _fwd_ws = BR.bwd_plan, BR.bwd_chunks, BR.fwd_shares


@pytest.mark.parametrize("g", BR.GEOMETRIES, ids=lambda g: g.name)
def test_geometry_shows_what_its_row_of_the_table_claims(g):
    c = BR.classify(g.lq, g.lk, g.causal, g.window, g.shift)
    assert c["off"] == g.off and g.shift == g.off - (g.lk - g.lq)
    if g.twin is not None:
        # a live band next to numbers beyond 2^28: the mask of the small twin, element for element; the far bound is out of reach
        t = g.twin_geometry()
        assert torch.equal(BR.band_mask(g.lq, g.lk, g.causal, g.window, g.shift), BR.band_mask(t.lq, t.lk, t.causal, t.window, t.shift))
        assert abs(g.off) > 1 << 28 and max(g.window) > 1 << 28 and max(g.window) < 1 << 31
        assert 0 < c["visible"] < c["total"]
        edge = g.off - g.window[0] if g.cls == "big-left" else g.off + g.window[1]
        assert edge == {"big-left": -25, "big-right": 105}[g.cls]
        return
    vis, er, ec, qwg, kwg = EXPECTED[g.name]
    assert (c["visible"], c["empty_rows"], c["empty_cols"]) == (vis, er, ec)
    assert (c["q_none"], c["q_all"]) == qwg and (c["k_none"], c["k_all"]) == kwg
    assert c["total"] == g.lq * g.lk and c["empty"] == (vis == 0) and c["all_visible"] == (vis == g.lq * g.lk)


def test_corner_and_threshold_geometries_name_their_element():
    m = lambda n: BR.band_mask(*(lambda g: (g.lq, g.lk, g.causal, g.window, g.shift))(BR.BY_NAME[n]))
    assert m("corner-hi").nonzero().tolist() == [[776, 0]]
    assert m("corner-lo").nonzero().tolist() == [[0, 999]]
    assert (~m("hi-live")).nonzero().tolist() == [[0, 999]]
    assert (~m("lo-live")).nonzero().tolist() == [[776, 0]]
    g = BR.BY_NAME["lo-live"]
    assert g.lq - 1 + g.off - g.window[0] == 1
    g = BR.BY_NAME["lo-dropped"]
    assert g.lq - 1 + g.off - g.window[0] == 0


def test_every_class_is_populated_and_the_list_keeps_its_edges():
    by_cls = {}
    for g in BR.GEOMETRIES:
        by_cls.setdefault(g.cls, []).append(g)
    assert set(by_cls) == set(BR.CLASSES) and len(BR.BY_NAME) == len(BR.GEOMETRIES)
    assert len(by_cls["unaligned-causal"]) == 14 and len(by_cls["unaligned-windowed"]) == 6 and len(by_cls["few-rows"]) == 3
    offs = [g.off for g in BR.GEOMETRIES if g.cls in ("unaligned-causal", "unaligned-windowed", "few-rows")]
    assert any(o > 0 and o % 32 for o in offs) and any(o < 0 and o % 32 for o in offs)
    assert any(o % 64 == 0 and o - 1 in offs and o + 1 in offs for o in offs)
    assert {-32, -31, 31, 33, 63, 64, 65} <= set(offs)
    # a wholly dark and a wholly lit query workgroup in the same call
    assert any(c["q_none"] > 0 and c["q_all"] > 0
               for c in (BR.classify(g.lq, g.lk, g.causal, g.window, g.shift) for g in BR.GEOMETRIES))
    # split-KV shares: with 2 .. 8 shares of the 64 key tiles, whole shares of the few-rows geometries lie outside the band
    for g in by_cls["few-rows"]:
        c = BR.classify(g.lq, g.lk, g.causal, g.window, g.shift)
        assert c["k_none"] >= 2 and g.lk == 4096


def test_fwd_cases_report_the_form_they_name():
    _C, lib = _lib()
    cases = GF.fwd_cases()
    for g, form, D, H, Hk, dtype in cases:
        BR.check_fwd_form(_C, lib, g, form, D, H, Hk, GF._DT[dtype])
        # the persistent forward declines a shifted band: asked for by name it plans like the library's own choice
        if D == 128 and g.causal_only and g.shift != 0:
            p8, au = (BR.fwd_args(_C, g, H, Hk, D, dict(RFA_FWD_FORM=f)) for f in ("p8x32", "auto"))
            assert BR.fwd_shares(lib, p8) == BR.fwd_shares(lib, au), g.name
    ran = {(g.name, form) for g, form, *_ in cases}
    assert GF.CORE_FWD <= ran and {g.name for g in BR.GEOMETRIES} == {n for n, _ in ran}
    # whole split-KV shares outside the band: the shares are contiguous runs of the 64-key tiles below the causal edge
    assert {f for n, f in ran if n == "rows200-keys4096-100"} >= {"split2", "split3", "split8"}


def test_bwd_cases_report_the_form_they_name():
    _C, lib = _lib()
    cases = GF.bwd_cases()
    limits = {}
    for g, form, D, H, Hk, dtype in cases:
        limits[(g.name, form, H, Hk)] = BR.check_bwd_form(_C, lib, g, form, D, H, Hk, GF._DT[dtype])
        # the balanced dK/dV schedule declines a shifted band
        if g.causal_only and g.shift != 0 and D in (128, 64):
            assert BR.bwd_plan(lib, BR.bwd_args(_C, g, H, Hk, D, dict(RFA_DKDV_WIDE="2")))[0] != _C.DKDV_BAL, g.name
    ran = {(g.name, form) for g, form, *_ in cases}
    assert GF.CORE_BWD <= ran and {g.name for g in BR.GEOMETRIES} == {n for n, _ in ran}
    assert sum(v is not None for v in limits.values()) == 7                 # 3 geometries x 2 chunkings + one at H 8 / Hk 1


def test_balanced_and_persistent_forms_decline_a_shift_where_they_would_run_unshifted():
    """Sq == Sk == 1024 causal: the balanced schedule by name runs at shift 0 and is declined at shift 33 (a partially
    visible band); the persistent forward has no host-visible plan, its eligibility rule is the same `mask_shift != 0`"""
    _C, lib = _lib()
    g0 = BR.Geometry("sq", "x", 1024, 1024, True, BR.NOWIN, 0, 2, None)
    assert _plan(lib, BR.bwd_args(_C, g0, 4, 2, 128, dict(RFA_DKDV_WIDE="2")))[0] == _C.DKDV_BAL
    g1 = g0._replace(off=33)
    assert _plan(lib, BR.bwd_args(_C, g1, 4, 2, 128, dict(RFA_DKDV_WIDE="2")))[0] != _C.DKDV_BAL


@pytest.mark.parametrize("D", [128, 64, 256])
def test_dropped_bounds_and_large_number_twins_plan_like_their_equals(D):
    """hi / lo 'dropped': plan, workspace bytes and dS-scratch bytes of the unwindowed non-causal call; a large-number
    geometry: those of its small twin — for plain and accumulate outputs, every forcing switch left alone"""
    _C, lib = _lib()
    pairs = []
    for n in ("hi-dropped", "lo-dropped"):
        g = BR.BY_NAME[n]
        pairs.append((g, g._replace(causal=False, window=BR.NOWIN, off=g.lk - g.lq)))
    for n in ("big-left-edge", "big-right-edge"):
        pairs.append((BR.BY_NAME[n], BR.BY_NAME[n].twin_geometry()))
    for g, same in pairs:
        for acc in (False, True):
            a, b = (BR.bwd_args(_C, x, 4, 2, D, acc=acc) for x in (g, same))
            assert _plan(lib, a) == _plan(lib, b), g.name
            assert _chunks(lib, a) == _chunks(lib, b), g.name
            for fn in (lib.rfa_bwd_ds_scratch_bytes, lib.rfa_bwd_ds_scratch_min_bytes, lib.rfa_bwd_workspace_bytes):
                assert fn(C.byref(a)) == fn(C.byref(b)), g.name
            fa, fb = (BR.fwd_args(_C, x, 4, 2, D, acc=acc) for x in (g, same))
            assert _fwd_ws(lib, fa) == _fwd_ws(lib, fb), g.name
    # ... and the 'live by one' neighbours are NOT the unwindowed call: their bound stays (seen where a size depends on it)
    g = BR.BY_NAME["lo-live"]
    if D >= 128:
        assert lib.rfa_bwd_ds_scratch_bytes(C.byref(BR.bwd_args(_C, g, 4, 2, D))) == 0
        assert lib.rfa_bwd_ds_scratch_bytes(C.byref(BR.bwd_args(_C, BR.BY_NAME["lo-dropped"], 4, 2, D))) > 0


def test_triangular_scratch_follows_a_negative_offset():
    """ds_row_off / ds_row_len (csrc/rfa_kernels.hpp) for c <= 0 — leading rows of zero length — are reachable on the host
    only through rfa_bwd_ds_scratch_bytes: B H 2048 sum_qt clamp(qt + c, 0, nKb), c = ((31 + off) >> 5) + 1"""
    _C, lib = _lib()
    checked = 0
    for g in BR.GEOMETRIES:
        if not g.causal_only:
            continue
        c = BR.classify(g.lq, g.lk, g.causal, g.window, g.shift)
        if c["empty"]:
            continue
        for H, Hk in ((4, 2), (8, 1)):
            got = lib.rfa_bwd_ds_scratch_bytes(C.byref(BR.bwd_args(_C, g, H, Hk, 128)))
            assert got == BR.tri_scratch_bytes(g, H), (g.name, got)
        checked += g.off < 0
    assert checked >= 5                                       # corner-hi, -333, -32, -31, the 200-row block at -100
    # both sides of a 32 boundary differ by one block column per row where the diagonal is inside the block
    b = lambda n: lib.rfa_bwd_ds_scratch_bytes(C.byref(BR.bwd_args(_C, BR.BY_NAME[n], 4, 2, 128)))
    assert b("causal-32") < b("causal-31") <= b("causal+1") == b("causal+31") < b("causal+33") == b("causal+64") < b("causal+65")


def test_halves_with_a_shift_plan_on_the_half_lengths():
    """dense q_half / k_half together with a shift: the band is normalised on the HALF lengths (norm_band takes the
    halves) — the plan of the back halves of twice-as-long tensors is the plan of the block itself"""
    _C, lib = _lib()
    g = BR.BY_NAME["causal+65"]
    a = BR.bwd_args(_C, g, 4, 2, 128)
    b = BR.bwd_args(_C, g, 4, 2, 128)
    b.Sq, b.Sk, b.q_half, b.k_half, b.total_k = 2 * g.lq, 2 * g.lk, _C.HALF_BACK, _C.HALF_BACK, g.B * 2 * g.lk
    assert _plan(lib, a) == _plan(lib, b)
    assert lib.rfa_bwd_ds_scratch_bytes(C.byref(a)) == lib.rfa_bwd_ds_scratch_bytes(C.byref(b))
