"""TEST INFRASTRUCTURE: far views — operands that lie more than 2^31 elements / 2^32 bytes from the pointer the library is
given.  No test in here; the layout arithmetic is plain Python (tests/test_far_cases_cpu.py checks it without a device),
only `Arena` touches memory.

An ARENA is one `torch.empty` allocation (never filled) that holds all tensors of one role group side by side:

    io-in    q, k, v, dout                              (io dtype)
    io-out   out, dq, dk, dv                            (io dtype)
    f32-in   lse, delta as the backward reads them      (fp32)
    f32-out  lse and the fp32 accumulators out_acc, lse_acc, dq_acc, dk_acc, dv_acc

and is made of slabs: slab 0 at offset 0, slab 1 from SLAB1 = 2^31 + 4096 elements of the arena's dtype on (past 2^32 bytes
for bf16 / fp16, past 2^33 for fp32).  Three far KINDS put part of every tensor of a group into slab 1:

    batch    B = 2 and batch entry 1 in slab 1: the batch stride is SLAB1 + A
    head     the last K/V head group — K/V head Hk - 1, query heads H - G .. H - 1 — in slab 1, through the head stride:
             (SLAB1 + A) / (index of the first far head), so that head lands on SLAB1 + A exactly
    packed   cu_seqlens input over rows of ROW_W = 8192 elements, the tensors side by side in the columns: every sequence
             starts behind row PACKED_ROW0 = 2^31 / 8192 + 64, i.e. past 2^31 elements through row0 * row_stride alone (the row
             stride stays in contract: include/rfa.h, "row strides"); the lse-like (H, T) tensors, whose row stride is 1, are
             far through their head stride

A (a few MiB, more than all live data of slab 0 together) moves every ALIAS out of the live data: an offset truncated to 32
bits lands `offset mod 2^31` elements, or `offset * size mod 2^32` bytes, from the base pointer, and with A in the stride that
is unused arena.  `Arena.poison` fills those alias regions — NaN for an input group, SENTINEL for an output group, which
also gets a band of 64 KiB on either side of every far piece — and `Arena.check` asserts the sentinels are untouched.  (The
rows of a packed view in front of PACKED_ROW0 belong to no sequence: the caller leaves them alone, so the alias rows keep
their fill.)  All strides are multiples of 8 and all bases 16-byte aligned: the backend passes the views through.

A view is described by `View`: shape, strides, offset (elements from the arena's start) and its LIVE pieces (start, extent)
relative to the view's own base — the contiguous runs (up to interleaving with its neighbours' columns, packed kind) the
kernels may touch.  `reach(view)` is the largest element offset from the base pointer any live piece holds."""
import collections
import itertools

SLAB1 = 2 ** 31 + 4096
ROW_W = 8192
PACKED_ROW0 = 2 ** 31 // ROW_W + 64
BAND_BYTES = 64 * 1024
SENTINEL = 5.0
KINDS = ("batch", "head", "packed")
SIDES = ("inputs", "outputs")

# name, layout, far-head rule: "q" = query heads (first far head H - G), "k" = K/V heads (Hk - 1)
Spec = collections.namedtuple("Spec", "name shape layout heads")
View = collections.namedtuple("View", "name shape strides offset esize live interleaved layout")


def _up(x, m):
    return (x + m - 1) // m * m


def reach(v):
    """largest element offset from the view's base pointer inside a live piece"""
    return max(s + n - 1 for s, n in v.live)


def reach_bytes(v):
    return reach(v) * v.esize + v.esize - 1


def far_pieces(v):
    """the live pieces whose END lies past 2^31 elements or 2^32 bytes from the base pointer"""
    return [(s, n) for s, n in v.live if s + n - 1 >= 2 ** 31 or (s + n) * v.esize - 1 >= 2 ** 32]


def aliases(v):
    """(start, extent) relative to the view's base: where the far pieces would land under a 32-bit truncation of the element
    offset (mod 2^31) or of the byte offset (mod 2^32)"""
    out = set()
    for s, n in far_pieces(v):
        for a in (s % 2 ** 31, (s * v.esize % 2 ** 32) // v.esize):
            if a != s:
                out.add((a, n))
    return sorted(out)


def bands(v):
    """(start, extent) relative to the view's base: 64 KiB in front of and behind every far piece (a packed view's rows are
    interleaved with its neighbours' and some of those are longer: in front only — tail_band() is the one behind them all)"""
    w = BAND_BYTES // v.esize
    if v.interleaved:                              # (whole rows: from the start of the piece's first row backwards)
        return sorted({(s - v.offset % ROW_W - w, w) for s, n in far_pieces(v)})
    return sorted({r for s, n in far_pieces(v) for r in ((s - w, w), (s + n, w))})


def tail_band(views):
    """[(start, extent)] in ARENA elements: 64 KiB behind the last row of the packed views of an arena"""
    ends = [v.offset + s + n for v in views.values() if v.interleaved for s, n in v.live]
    return [(_up(max(ends), ROW_W), BAND_BYTES // next(iter(views.values())).esize)] if ends else []


def _first_far_head(spec, G):
    H = spec.shape[-2] if spec.layout in ("bshd", "thd") else spec.shape[-2 if spec.layout == "bhs" else 0]
    f = H - G if spec.heads == "q" else H - 1
    assert f >= 1, (spec, "a far head group needs a near one in front of it")
    return H, f


def layout(kind, specs, esize, G=2):
    """({name: View}, arena elements) of the tensors `specs` (one role group) under far kind `kind`.  Layouts: bshd (B, S, H,
    D), bhs (B, H, S) for dense input; thd (T, H, D), ht (H, T) for packed input (T counts from row 0: the sequences start at
    PACKED_ROW0).  G: query heads per K/V head."""
    band = BAND_BYTES // esize
    views = {}
    if kind == "batch":
        foot = [_prod(s.shape[1:]) for s in specs]
        offs, o = [], band
        for f in foot:
            offs.append(o)
            o = _up(o + f + 2 * band, 4096)
        A = _up(4 * o, 4096)
        far = SLAB1 + A
        for s, f, o_ in zip(specs, foot, offs):
            assert s.shape[0] == 2, s                       # (any layout: entry 1 is contiguous like entry 0)
            inner = _contig(s.shape[1:])
            views[s.name] = View(s.name, tuple(s.shape), (far,) + inner, o_, esize, ((0, f), (far, f)), False, s.layout)
    elif kind == "head":
        foot = [_prod(s.shape) // _first_far_head(s, G)[0] for s in specs]          # one head's (B, S, D) / (B, S)
        offs, o = [], band
        for f in foot:
            offs.append(o)
            o = _up(o + f + 2 * band, 4096)
        A = _up(4 * o, 4096)
        for s, f, o_ in zip(specs, foot, offs):
            H, first = _first_far_head(s, G)
            hs = _up(-(-(SLAB1 + A) // first), 8)
            if s.layout == "bshd":
                B, S, _, D = s.shape
                strides = (S * D, D, hs, 1)
            else:
                assert s.layout == "bhs", s
                B, _, S = s.shape
                strides = (S, hs, 1)
            views[s.name] = View(s.name, tuple(s.shape), strides, o_, esize, tuple((h * hs, f) for h in range(H)), False, s.layout)
    elif kind == "packed":
        col = 0
        flat = [s for s in specs if s.layout == "ht"]
        for s in specs:
            if s.layout != "thd":
                continue
            T, H, D = s.shape
            assert T > PACKED_ROW0, s
            views[s.name] = View(s.name, tuple(s.shape), (ROW_W, D, 1), col, esize,
                                 ((PACKED_ROW0 * ROW_W, (T - PACKED_ROW0 - 1) * ROW_W + H * D),), True, s.layout)
            col += _up(H * D, 8)
        assert col <= ROW_W, col
        # (H, T): head h at h * hs + o; heads 1 .. H - 2 fall into unused rows in front of PACKED_ROW0, the last one behind every row
        o = 8192 * ROW_W
        for s in flat:
            H, T = s.shape
            hs = _up(-(-(SLAB1 + 16 * 4096) // (H - 1)), 8)
            views[s.name] = View(s.name, tuple(s.shape), (hs, 1), o, esize,
                                 tuple((h * hs + PACKED_ROW0, T - PACKED_ROW0) for h in range(H)), False, s.layout)
            o = _up(o + T + 2 * band, 4096)
    else:
        raise ValueError(kind)
    size = max(v.offset + max(max(s + n for s, n in v.live), max((s + n for s, n in bands(v)), default=0)) for v in views.values())
    size = max([size] + [s + n for s, n in tail_band(views)])
    check_layout(views, size)
    return views, _up(size + band, 4096)


def _prod(shape):
    n = 1
    for x in shape:
        n *= x
    return n


def _contig(shape):
    st, run = [], 1
    for n in reversed(shape):
        st.insert(0, run)
        run *= n
    return tuple(st)


def _overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def check_layout(views, size=None):
    """the live pieces of an arena's views are pairwise disjoint (packed thd views interleave by columns instead), and no alias
    region or band touches a live piece; strides and offsets keep the library's 16-byte contract"""
    live = [(v.name, v.interleaved, (v.offset + s, n)) for v in views.values() for s, n in v.live]
    for (na, ia, a), (nb, ib, b) in itertools.combinations(live, 2):
        if ia and ib:
            continue
        assert not _overlap(a, b), ("live pieces overlap", na, a, nb, b)
    for r in tail_band(views):
        for nm, _, piece in live:
            assert not _overlap(r, piece), ("tail band", r, nm, piece)
    for v in views.values():
        assert v.offset % 8 == 0 and v.strides[-1] == 1, v
        if v.layout in ("bshd", "thd"):
            assert all(st % 8 == 0 for st in v.strides[:-1]), v
        for what, regs in (("alias", aliases(v)), ("band", bands(v))):
            for s, n in regs:
                r = (v.offset + s, n)
                assert r[0] >= 0 and (size is None or what == "band" or r[0] + n <= size), (what, v.name, r)
                for nm, inter, piece in live:
                    assert not _overlap(r, piece), (what, v.name, r, nm, piece)


# ---- the role groups of one attention call ---------------------------------------------------------------------------------
def call_specs(lead_q, lead_k, H, Hk, D, Dv, packed):
    """{group: [Spec]} of a forward + backward with plain and accumulated outputs.  lead_q / lead_k: (B, S) or (T,)"""
    t4 = lambda name, lead, h, d, heads: Spec(name, (*lead, h, d), "thd" if packed else "bshd", heads)
    l3 = lambda name: Spec(name, (H, lead_q[0]) if packed else (lead_q[0], H, lead_q[1]), "ht" if packed else "bhs", "q")
    return {
        "io-in": [t4("q", lead_q, H, D, "q"), t4("k", lead_k, Hk, D, "k"), t4("v", lead_k, Hk, Dv, "k"), t4("dout", lead_q, H, Dv, "q")],
        "io-out": [t4("out", lead_q, H, Dv, "q"), t4("dq", lead_q, H, D, "q"), t4("dk", lead_k, Hk, D, "k"), t4("dv", lead_k, Hk, Dv, "k")],
        "f32-in": [l3("lse_in"), l3("delta_in")],
        "f32-out": [l3("lse"), l3("lse_acc"), t4("out_acc", lead_q, H, Dv, "q"), t4("dq_acc", lead_q, H, D, "q"),
                    t4("dk_acc", lead_k, Hk, D, "k"), t4("dv_acc", lead_k, Hk, Dv, "k")],
    }


SIDE_GROUPS = {"inputs": ("io-in", "f32-in"), "outputs": ("io-out", "f32-out")}
GROUP_ESIZE = {"io-in": 2, "io-out": 2, "f32-in": 4, "f32-out": 4}


def far_case(kind, side, lead_q, lead_k, H, Hk, D, Dv, extra=None):
    """{group: ({name: View}, arena elements)} of the groups that are far in case (kind, side); extra: {group: [Spec]} of
    further tensors that live in a group's arena (a feature's own operands)"""
    specs = call_specs(lead_q, lead_k, H, Hk, D, Dv, kind == "packed")
    return {g: layout(kind, specs[g] + list((extra or {}).get(g, ())), GROUP_ESIZE[g], H // Hk) for g in SIDE_GROUPS[side]}


def compact_reach(spec, esize):
    """(elements, bytes) the contiguous twin of a tensor reaches from its base pointer"""
    n = _prod(spec.shape)
    return n - 1, n * esize - 1


def arena_bytes(case):
    return sum(n * GROUP_ESIZE[g] for g, (_, n) in case.items())


# ---- memory: the only part that needs torch -------------------------------------------------------------------------------
class Arena:
    """one torch.empty allocation and the views of one role group in it"""

    def __init__(self, views, nelems, dtype, device, output):
        import torch

        self.torch, self.views, self.output = torch, views, output
        self.buf = torch.empty(nelems, dtype=dtype, device=device)
        assert self.buf.element_size() == next(iter(views.values())).esize
        self.regions = sorted({(v.offset + s, n) for v in views.values() for s, n in aliases(v) + (bands(v) if output else [])}
                              | set(tail_band(views) if output else []))
        self.regions = [(max(s, 0), min(s + n, nelems) - max(s, 0)) for s, n in self.regions]

    def view(self, name):
        v = self.views[name]
        t = self.torch.as_strided(self.buf, v.shape, v.strides, v.offset)
        assert t.data_ptr() % 16 == 0
        return t

    def poison(self):
        """fill the alias regions (and, for an output group, the bands): call BEFORE the views are given their values"""
        for s, n in self.regions:
            self.buf[s:s + n] = SENTINEL if self.output else float("nan")

    def check(self):
        """an output group's sentinels are untouched"""
        if not self.output:
            return
        for s, n in self.regions:
            assert bool((self.buf[s:s + n] == SENTINEL).all()), f"written outside the addressed region: arena elements [{s}, {s + n})"


# ---- the case tables (tests/test_far_cases_cpu.py checks them; tests/test_gpu_far_addressing.py runs them) ----------------------
HEADS = (4, 2)                                                   # H, Hk of every attention case
DIMS = ((128, 128), (64, 64), (80, 80), (192, 192), (192, 128))  # (D, Dv) of the poison tests' CASES
DENSE_LEADS = ((2, 300), (2, 520))                               # (B, Sq), (B, Sk): the poison tests' dense call
BALANCED_LEADS = ((2, 512), (2, 512))                            # the balanced dK/dV schedule's smallest shape
PACKED_LEADS = ((PACKED_ROW0 + 1000,), (PACKED_ROW0 + 1800,))    # rows of the poison tests' packed batch behind PACKED_ROW0


def form_cases():
    """[(id, kind, side, lead_q, lead_k, D, Dv)] of section "far views in every kernel form" (one per distinct layout: the
    kernel forms of one head dim share it)"""
    out = []
    for kind in KINDS:
        for side in SIDES:
            leads = [("packed", PACKED_LEADS)] if kind == "packed" else [("dense", DENSE_LEADS), ("balanced", BALANCED_LEADS)]
            for tag, (lq, lk) in leads:
                for D, Dv in (DIMS if tag != "balanced" else DIMS[:1]):
                    out.append((f"{tag}-d{D}v{Dv}-{kind}-{side}", kind, side, lq, lk, D, Dv))
    return out


def aux_layouts():
    """{case: {group: (views, arena elements, element size, output)}} of the auxiliary kernels' far operands: all of the batch
    kind (the leading extent is 2 and its stride SLAB1 + A), except the flat cast"""
    B, S, Hh, D = 2, 300, 3, 128
    L = lambda specs, esize, out=False: layout("batch", specs, esize) + (esize, out)
    t4 = lambda name, shape=(B, S, Hh, D): Spec(name, shape, "bshd", "q")
    l3 = lambda name, shape=(B, Hh, S): Spec(name, shape, "bhs", "q")
    return {
        "sum_slots": {"slots": L([Spec("slots", (2, B, S, Hh, D), "wbshd", "q")], 2), "dst": L([t4("dst")], 2, True)},
        "merge": {"io": L([t4("block_out")], 2), "f32": L([t4("out_acc"), l3("lse_acc"), l3("block_lse")], 4, True)},
        "merge_pair": {"io": L([t4("out_a"), t4("out_b"), t4("dout")], 2), "f32": L([l3("lse_a"), l3("lse_b"), l3("dlse")], 4)},
        "seq_head": {"io": L([t4("local", (B, 64, 4, D))], 2)},
        "sink": {"io": L([t4("out"), t4("dout")], 2), "f32": L([l3("lse")], 4)},
        "preprocess": {"io": L([t4("dout"), t4("out")], 2), "f32": L([l3("dlse"), l3("delta")], 4, True)},
        "max_logit": {"io": L([Spec("q", (B, 300, 4, D), "bshd", "q"), Spec("k", (B, 520, 2, D), "bshd", "k")], 2)},
        # (H, T) and (T, H) with the head stride past 2^31: two "entries" of T contiguous floats
        "lse_relayout": {"f32": L([Spec("packed", (2, 529), "ht", "q")], 4, True)},
    }


CAST_N = 2 ** 31 + 24                                            # elements of the flat cast: src fp32, dst io dtype

# long walks inside one sequence: rows of ROW_W (and ROW_W + 8) elements, k and v in the last columns of one arena
WALK_SQ, WALK_SK = 256, 262144
WALK_WIDTHS = (ROW_W, ROW_W + 8)


def walk_view(width, col, D, Sk=WALK_SK):
    """the (1, Sk, 1, D) view of columns [col, col + D) of an arena of Sk rows of `width` elements"""
    return View("kv", (1, Sk, 1, D), (Sk * width, width, D, 1), col, 2, ((0, (Sk - 1) * width + D),), False, "bshd")


# the packed long input: 64 sequences of 4096 rows, then 300, 0 and 77 rows, on ROW_W-wide rows
LONG_LENS = [4096] * 64 + [300, 0, 77]


def long_packed_view(col, H, D):
    T = sum(LONG_LENS)
    first_far = sum(LONG_LENS[:64])
    return View("thd", (T, H, D), (ROW_W, D, 1), col, 2, ((0, first_far * ROW_W), (first_far * ROW_W, (T - first_far - 1) * ROW_W + H * D)), True, "thd")


# the dS hand-off at the top of its 32-bit range: one head's share of the scratch of a dense causal sequence of 65504 rows
DS_ROWS = 65504
DS_BLOCK_BYTES = 2048
DS_HEAD_BYTES = (DS_ROWS // 32) * (DS_ROWS // 32 + 1) // 2 * DS_BLOCK_BYTES
