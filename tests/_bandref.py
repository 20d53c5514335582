"""Shifted attention bands: the fp64 reference (from tests/_blockref.py), what a band looks like from its mask alone, and
the named list of block geometries the band tests run (tests/test_band_cases_cpu.py checks the list, tests/test_gpu_band_forms.py runs it through
every kernel form).  No test in here.

A block's band (include/rfa.h, `mask_shift`): query row i sees key j iff

    off - wl <= j - i <= off + wr ,      off = len_k - len_q + mask_shift ,

each side only when set (>= 0); `causal` means wr = 0.  The geometries are stated through `off` — the position of the
diagonal inside the block — because that is what decides which clamp, tile range and in-tile mask a kernel takes."""
import collections

from _blockref import attention, visible as band_mask

BIG = 1 << 30


def band_ref(q, k, v, do, causal, window, shift=0):
    """_blockref.attention with the block taken as the WHOLE attention: out, lse, dq, dk, dv in fp64 — lse = +inf and out = 0
    for rows without a key, block-local lse and delta: what a call with plain outputs computes.  q, do (B, Sq, H, D); k, v
    (B, Sk, Hk, D)."""
    return attention(q, k, v, dout=do, causal=causal, window=window, shift=shift)


def classify(lq, lk, causal, window, shift):
    """what the boolean mask alone shows (CPU, no kernel).  Workgroups: 256 query rows (forward, dQ), 256 / 128 keys
    (dK/dV); `none` = sees nothing, `all` = every element of it visible."""
    vis = band_mask(lq, lk, causal, window, shift)
    off = lk - lq + int(shift)

    def groups(m, size):                     # m: (n, other) rows = the axis that is cut into workgroups
        none = full = 0
        for a in range(0, m.shape[0], size):
            blk = m[a:a + size]
            none += int(not blk.any())
            full += int(blk.all())
        return none, full, (m.shape[0] + size - 1) // size

    q_none, q_all, nq = groups(vis, 256)
    k_none, k_all, nk = groups(vis.t(), 256)
    k128_none, k128_all, nk128 = groups(vis.t(), 128)
    visible = int(vis.sum())
    return dict(off=off, off32=off % 32, off64=off % 64, visible=visible, total=lq * lk,
                empty_rows=int((~vis.any(1)).sum()), empty_cols=int((~vis.any(0)).sum()),
                q_none=q_none, q_all=q_all, nq=nq, k_none=k_none, k_all=k_all, nk=nk,
                k128_none=k128_none, k128_all=k128_all, nk128=nk128,
                all_visible=visible == lq * lk, empty=visible == 0)


class Geometry(collections.namedtuple("Geometry", "name cls lq lk causal window off B twin")):
    """one block geometry.  cls: the class of the table it belongs to; twin: (window, off) of the small-number geometry
    with the same two edges (large-number classes), or None"""
    __slots__ = ()

    @property
    def shift(self):
        return self.off - (self.lk - self.lq)

    @property
    def band(self):
        """the keywords of be.fwd / be.bwd"""
        return dict(causal=self.causal, window=self.window, mask_shift=self.shift)

    @property
    def causal_only(self):
        return self.causal and self.window[0] < 0

    def twin_geometry(self):
        w, off = self.twin
        return self._replace(name=self.name + "-twin", window=w, off=off, twin=None)


def _g(name, cls, causal, window, off, lq=777, lk=1000, B=2, twin=None):
    return Geometry(name, cls, lq, lk, causal, window, off, B, twin)


NOWIN = (-1, -1)
UNALIGNED_OFFS = (-333, -32, -31, 1, 31, 33, 63, 64, 65, 257, 401, 600)

GEOMETRIES = [
    # exactly one visible element in a corner, and the empty block next to it
    _g("corner-hi", "corner-hi", True, NOWIN, -776),
    _g("corner-hi-1", "corner-hi-1", True, NOWIN, -777),
    _g("corner-lo", "corner-lo", True, (100, 0), 1099),
    _g("corner-lo+1", "corner-lo+1", True, (100, 0), 1100),
    # exactly one masked element, and the bound that is dropped next to it
    _g("hi-live", "hi-live", True, NOWIN, 998),
    _g("hi-dropped", "hi-dropped", True, NOWIN, 999),
    _g("lo-live", "lo-live", False, (300, -1), -475),
    _g("lo-dropped", "lo-dropped", False, (300, -1), -476),
] + [_g(f"causal{off:+d}", "unaligned-causal", True, NOWIN, off) for off in UNALIGNED_OFFS] + [
    # row 63 sees key 0 and nothing else: the first query row of key block 0 is the LAST row of a 64-row Q/dO tile, and
    # the one element that tile holds carries a whole probability (the dK/dV tile range's lower clamp, to the row)
    _g("causal-63", "unaligned-causal", True, NOWIN, -63),
    # more queries than keys: a wholly dark (rows 0 .. 255) and a wholly lit (rows 768 .. 999) query workgroup in one call
    _g("rows1000-keys300-300", "unaligned-causal", True, NOWIN, -300, lq=1000, lk=300),
] + [
    _g(f"wl130{off:+d}", "unaligned-windowed", True, (130, 0), off) for off in (-333, 65, 401)] + [
    _g(f"two-sided{off:+d}", "unaligned-windowed", False, (90, 40), off) for off in (-333, 65, 401)] + [
    # few rows against many keys: with 2 .. 8 split-KV shares whole shares lie outside the band
    _g("rows256-keys4096+1500", "few-rows", True, NOWIN, 1500, lq=256, lk=4096),
    _g("rows200-keys4096-100", "few-rows", True, NOWIN, -100, lq=200, lk=4096),
    _g("rows384-keys4096+3000", "few-rows", True, NOWIN, 3000, lq=384, lk=4096),
    # a live band next to numbers beyond 2^28: the one bound in reach is re-expressed, the other is dropped
    _g("big-left-edge", "big-left", False, (BIG + 90, 40), BIG + 65, twin=((90, -1), 65)),
    _g("big-right-edge", "big-right", False, (90, BIG + 40), -BIG + 65, twin=((-1, 40), 65)),
]
BY_NAME = {g.name: g for g in GEOMETRIES}
CLASSES = ("corner-hi", "corner-hi-1", "corner-lo", "corner-lo+1", "hi-live", "hi-dropped", "lo-live", "lo-dropped",
           "unaligned-causal", "unaligned-windowed", "few-rows", "big-left", "big-right")


# ---- kernel forms: the switches that force one (ring_flash_attn.config) and the launch plan each must report ---------
# forward: env, and the split-KV share count rfa_fwd_workspace_bytes must report (None: the library's choice)
FWD_FORMS = {
    "auto": (dict(), None),
    "8x32": (dict(RFA_FWD_FORM="8x32", RFA_FWD_KV_NSPLIT="1"), 1),
    "4x32": (dict(RFA_FWD_FORM="4x32", RFA_FWD_KV_NSPLIT="1"), 1),
    "split2": (dict(RFA_FWD_KV_NSPLIT="2"), 2),
    "split3": (dict(RFA_FWD_KV_NSPLIT="3"), 3),
    "split8": (dict(RFA_FWD_KV_NSPLIT="8"), 8),
}
# backward: env, (dkdv form, shares, five_gemm) rfa_bwd_plan must report (None: not fixed by the form's name), and the
# dS scratch limit as a function of (whole hand-off, one query head's share, query heads per K/V head) or None
DKDV_128, DKDV_256, DKDV_BAL = 1, 2, 3
BWD_FORMS = {
    "7gemm": (dict(RFA_BWD_DS_SPILL="0"), (None, None, 0), None),
    "5gemm": (dict(RFA_BWD_DS_SPILL="1"), (None, None, 1), None),
    "5gemm-kv-chunks": (dict(RFA_BWD_DS_SPILL="1"), (None, None, 1), lambda full, per, G: full - 1),
    "5gemm-q-fractions": (dict(RFA_BWD_DS_SPILL="1"), (None, None, 1), lambda full, per, G: per * G - 1),
    "dkdv128": (dict(RFA_DKDV_WIDE="0"), (DKDV_128, 1, None), None),
    "dkdv256-1": (dict(RFA_DKDV_WIDE="1", RFA_DKDV_NSPLIT="1"), (DKDV_256, 1, None), None),
    "dkdv256-2": (dict(RFA_DKDV_WIDE="1", RFA_DKDV_NSPLIT="2"), (DKDV_256, 2, None), None),
    "dkdv256-3": (dict(RFA_DKDV_WIDE="1", RFA_DKDV_NSPLIT="3"), (DKDV_256, 3, None), None),
    "dkdv256-4": (dict(RFA_DKDV_WIDE="1", RFA_DKDV_NSPLIT="4"), (DKDV_256, 4, None), None),
    "windowed": (dict(), (DKDV_128, None, None), None),
}


def fwd_args(C_, g, H, Hk, D, env=None, dtype=0, acc=False):
    """rfa_fwd_args of geometry g as HipBackend.fwd fills them under the switches `env` (pointers: any non-NULL value —
    the size / plan functions are pure functions of the arguments)"""
    env = env or {}
    a = C_.FwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype = g.B, g.lq, g.lk, H, Hk, D, dtype
    a.causal = 1 if g.causal else 0
    if g.window[0] >= 0 or g.window[1] >= 0:
        a.window, a.window_left, a.window_right = 1, g.window[0], g.window[1]
    a.mask_shift = g.shift
    a.fwd_form = {"auto": C_.FWD_AUTO, "8x32": C_.FWD_8x32, "4x32": C_.FWD_4x32, "p8x32": C_.FWD_P8x32}[env.get("RFA_FWD_FORM", "auto")]
    a.kv_nsplit = int(env.get("RFA_FWD_KV_NSPLIT", "0"))
    if acc:
        a.out_acc = a.lse_acc = 256
    return a


def bwd_args(C_, g, H, Hk, D, env=None, dtype=0, acc=False, scratch=True, scratch_bytes=0, phases=0):
    """rfa_bwd_args of geometry g as HipBackend.bwd fills them under the switches `env`"""
    env = env or {}
    a = C_.BwdArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.total_k = g.B, g.lq, g.lk, H, Hk, D, dtype, g.B * g.lk
    a.causal = 1 if g.causal else 0
    if g.window[0] >= 0 or g.window[1] >= 0:
        a.window, a.window_left, a.window_right = 1, g.window[0], g.window[1]
    a.mask_shift = g.shift
    a.phases = phases
    wide, ns = env.get("RFA_DKDV_WIDE"), int(env.get("RFA_DKDV_NSPLIT", "0"))
    if wide == "0":
        a.dkdv_form = C_.DKDV_128
    elif wide == "2" and ns <= 0:
        a.dkdv_form = C_.DKDV_BAL
    elif ns > 0 or wide == "1":
        a.dkdv_form = C_.DKDV_256
    a.dkdv_nsplit = ns
    if scratch and env.get("RFA_BWD_DS_SPILL", "1") != "0":
        a.ds_scratch = 256
        a.ds_scratch_bytes = scratch_bytes
    if acc:
        a.dq_acc = a.dk_acc = a.dv_acc = 256
    return a


def tri_scratch_bytes(g, H):
    """rfa_bwd_ds_scratch_bytes of a dense causal-only call from the header's own formula (csrc/rfa_kernels.hpp): row qt
    of 32 query rows holds clamp(qt + c, 0, nKb) blocks of 2 KiB, c = ((31 + off) >> 5) + 1 capped at nKb"""
    nqt, nkb = (g.lq + 31) // 32, (g.lk + 31) // 32
    c = min(((31 + g.off) >> 5) + 1, nkb)
    return g.B * H * 2048 * sum(min(max(qt + c, 0), nkb) for qt in range(nqt))


# ---- host-side checks: the (geometry, form) pair runs the form it names (pure functions of the C ABI, no device) ------
def _ctypes():
    import ctypes

    return ctypes


def bwd_plan(lib, a):
    C = _ctypes()
    f, n, five = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.rfa_bwd_plan(C.byref(a), C.byref(f), C.byref(n), C.byref(five)) == 0
    return f.value, n.value, five.value


def bwd_chunks(lib, a):
    C = _ctypes()
    n, hc, gc, cb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert lib.rfa_bwd_ds_chunks(C.byref(a), C.byref(n), C.byref(hc), C.byref(gc), C.byref(cb)) == 0
    return n.value, hc.value, gc.value, cb.value


def fwd_shares(lib, a):
    C = _ctypes()
    n = C.c_int32()
    return lib.rfa_fwd_workspace_bytes(C.byref(a), C.byref(n)), n.value


def check_fwd_form(C_, lib, g, form, D, H, Hk, dtype=0):
    """the forward of geometry g under form `form` runs what the form names"""
    env, want_ns = FWD_FORMS[form]
    c = classify(g.lq, g.lk, g.causal, g.window, g.shift)
    if form != "auto":
        assert g.causal_only and D in (128, 64), (g.name, form, D)      # (4x32 and the split-KV shares exist without a window only)
    for acc in (False, True):
        nbytes, ns = fwd_shares(lib, fwd_args(C_, g, H, Hk, D, env, dtype, acc))
        tag = (g.name, form, D, acc, nbytes, ns)
        if want_ns is not None:
            assert ns == want_ns, tag
            assert nbytes == (0 if want_ns == 1 else want_ns * g.B * g.lq * H * (D + 1) * 4), tag
        if not g.causal_only and not c["all_visible"]:
            assert (nbytes, ns) == (0, 1), tag                           # windowed instances: one form, no shares


def check_bwd_form(C_, lib, g, form, D, H, Hk, dtype=0, phases=0):
    """the backward of geometry g under form `form` runs what the form names; returns the dS scratch limit to run it with
    (None: the default)"""
    C = _ctypes()
    env, (wform, wns, wfive), limit = BWD_FORMS[form]
    c = classify(g.lq, g.lk, g.causal, g.window, g.shift)
    G = H // Hk
    a0 = bwd_args(C_, g, H, Hk, D, env, dtype, phases=phases)
    full, per = lib.rfa_bwd_ds_scratch_bytes(C.byref(a0)), lib.rfa_bwd_ds_scratch_min_bytes(C.byref(a0))
    sb = None
    if limit is not None:
        assert D == 128 and per > 0 and full == H * per, (g.name, form, full, per)
        sb = limit(full, per, G)
    if form.startswith("dkdv"):
        assert g.causal_only and D in (128, 64), (g.name, form, D)      # (RFA_DKDV_256 is ignored with a window)
    if form == "windowed":
        assert not g.causal_only, (g.name, form)
    if form.startswith("5gemm") or form == "7gemm":
        assert g.causal_only and D in (128, 256), (g.name, form, D)
    if c["empty"]:
        return sb                                                        # (nothing is launched or only zeros are stored)
    for acc in (False, True):
        a = bwd_args(C_, g, H, Hk, D, env, dtype, acc=acc, scratch_bytes=sb or 0, phases=phases)
        f, ns, five = bwd_plan(lib, a)
        n, hc, gc, cb = bwd_chunks(lib, a)
        tag = (g.name, form, D, acc, (f, ns, five), (n, hc, gc, cb), full, per)
        assert wform is None or f == wform, tag
        assert wns is None or ns == wns, tag
        assert wfive is None or five == wfive, tag
        if form == "windowed" and D <= 128:
            assert ns == 1, tag
        if form == "5gemm":
            assert full == tri_scratch_bytes(g, H), tag          # (the triangle follows the shifted diagonal, to the block)
            assert (n, hc, gc, cb) == (1, Hk, G, full), tag
        elif form == "5gemm-kv-chunks":
            assert n == Hk // hc > 1 and gc == G and cb <= sb, tag
        elif form == "5gemm-q-fractions":
            assert hc == 1 and gc < G and n == Hk * (G // gc) and cb <= sb, tag
        elif form == "7gemm":
            assert n == 0, tag
    return sb
