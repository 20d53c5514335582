"""The far-view case tables of tests/_farview.py, checked without a device: every case of tests/test_gpu_far_addressing.py puts
every tensor of the role group it names more than 2^31 elements AND more than 2^32 bytes behind the pointer the library is
given, its compact twin crosses neither line, the arenas' live pieces do not overlap, and wherever a 32-bit truncation of a far
offset would land — offset mod 2^31 elements, offset * size mod 2^32 bytes — the arena is unused (so NaN / a sentinel can sit
there).  This is what keeps the GPU tests from being vacuous: they never run a kernel with a wrong offset."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _farview as FV                            # noqa: E402

E31, B32 = 2 ** 31, 2 ** 32
GiB = 1 << 30


def _crosses(v):
    return FV.reach(v) > E31 and FV.reach_bytes(v) > B32


@pytest.mark.parametrize("case", FV.form_cases(), ids=lambda c: c[0])
def test_every_form_case_crosses_both_lines_and_its_compact_twin_neither(case):
    _, kind, side, lq, lk, D, Dv = case
    H, Hk = FV.HEADS
    far = FV.far_case(kind, side, lq, lk, H, Hk, D, Dv)
    specs = FV.call_specs(lq, lk, H, Hk, D, Dv, kind == "packed")
    assert set(far) == set(FV.SIDE_GROUPS[side])
    for group, (views, nelems) in far.items():
        es = FV.GROUP_ESIZE[group]
        assert {s.name for s in specs[group]} == set(views)
        FV.check_layout(views, nelems)
        for s in specs[group]:
            v = views[s.name]
            assert v.shape == tuple(s.shape) and v.esize == es
            assert _crosses(v), (group, s.name, FV.reach(v), FV.reach_bytes(v))
            assert FV.far_pieces(v) and FV.aliases(v), (group, s.name)
            assert v.offset + FV.reach(v) < nelems
            # the far pieces are where the kind says: batch entry 1 / the last K/V head group / every packed sequence
            n_far = {"batch": 1, "head": None, "packed": None}[kind]
            if n_far is not None:
                assert len([p for p in v.live if p[0] >= E31]) == n_far
            if kind == "head":
                Hn, first = FV._first_far_head(s, H // Hk)
                assert [p[0] >= E31 for p in v.live] == [h >= first for h in range(Hn)]
            if kind == "packed" and s.layout == "thd":
                assert v.strides[0] == FV.ROW_W and all(p[0] >= E31 for p in v.live) and 256 * v.strides[0] * es + 256 * es < E31
            el, by = FV.compact_reach(s, es)
            assert el < E31 and by < B32, (group, s.name, el, by)
    assert FV.arena_bytes(far) <= 20 * GiB, FV.arena_bytes(far) / GiB
    # the groups of the other side stay compact
    assert not set(far) & set(FV.SIDE_GROUPS["outputs" if side == "inputs" else "inputs"])


def test_the_form_cases_are_the_poison_tests_shapes():
    import test_gpu_far_addressing as T
    import test_gpu_poison as GP

    assert FV.HEADS == (GP.H, GP.Hk)
    assert {(c[2], c[3]) for c in GP.CASES + GP.PACKED_CASES} == set(FV.DIMS)
    assert FV.DENSE_LEADS == ((GP.DENSE.B, GP.DENSE.lq), (GP.DENSE.B, GP.DENSE.lk))
    assert FV.PACKED_LEADS == ((T.CU_Q[-1],), (T.CU_K[-1],)) and T.CU_Q[0] == FV.PACKED_ROW0
    assert FV.PACKED_ROW0 * FV.ROW_W > E31
    ids = [p.id for p in T._form_params()]
    assert len(ids) == len(set(ids)) == (len(GP.CASES) + 1) * 4 + len(GP.PACKED_CASES) * 2
    for p in T._form_params():                                   # every GPU case has its layout in the table above
        case, kind, side = p.values
        shape = T._Shape(case, kind == "packed")
        assert any((k, s, lq, lk, D, Dv) == (kind, side, shape.lead_q, shape.lead_k, shape.D, shape.Dv)
                   for _, k, s, lq, lk, D, Dv in FV.form_cases()), p.id
    assert sum(1 for p in T._form_params() if not p.marks) == 1


@pytest.mark.parametrize("name", sorted(FV.aux_layouts()))
def test_every_auxiliary_case_crosses_both_lines(name):
    total = 0
    for group, (views, nelems, es, out) in FV.aux_layouts()[name].items():
        FV.check_layout(views, nelems)
        total += nelems * es
        for v in views.values():
            assert _crosses(v) and v.strides[0] > E31, (name, group, v.name)
            n = 1
            for x in v.shape:
                n *= x
            assert n < E31 and n * es < B32
    assert total <= 20 * GiB


def test_the_long_walks_the_cast_and_the_ds_handoff():
    # 8192-wide rows: the last key row ends 8065 elements short of 2^31 — the walk crosses the 2^31-BYTE line and stops 16 KiB
    # short of 2^32 bytes; 8200-wide rows cross both lines
    narrow, wide = (FV.walk_view(w, w - 256, 128) for w in FV.WALK_WIDTHS)
    assert E31 - 8192 < FV.reach(narrow) < E31 and E31 < FV.reach_bytes(narrow) < B32
    assert _crosses(wide)
    for w in FV.WALK_WIDTHS:
        assert w % 8 == 0 and 256 * w * 2 + 256 * 2 < E31                       # (row strides inside the contract)
        assert FV.WALK_SK * w * 2 * 2 <= 20 * GiB
    # tile j of 64 keys starts j * 64 * row_stride elements in: as a 32-bit product it would wrap inside the walk of the wide rows
    assert (FV.WALK_SK // 64 - 1) * 64 * FV.WALK_WIDTHS[1] > E31 > (FV.WALK_SK // 64 - 1) * 64 * FV.WALK_WIDTHS[0]
    v = FV.long_packed_view(0, 4, 128)
    assert sum(FV.LONG_LENS[:64]) * FV.ROW_W == E31 and FV.LONG_LENS[64:] == [300, 0, 77]
    assert FV.far_pieces(v) == [v.live[1]] and v.live[1][0] == E31 and FV.reach(v) > E31
    assert FV.CAST_N > E31 and FV.CAST_N % 8 == 0
    # one head's dS of a dense causal sequence of 65504 rows: 2047 * 2048 / 2 blocks of 2048 B, 2 MiB under 2^32
    assert FV.DS_ROWS == 2047 * 32 and FV.DS_HEAD_BYTES == 2047 * 2048 // 2 * 2048 == 4292870144 == B32 - 2 ** 21
    assert (65536 // 32) * (65536 // 32 + 1) // 2 >= 2 ** 21 > FV.DS_HEAD_BYTES // FV.DS_BLOCK_BYTES        # (65536 rows: the 7-GEMM form)
    assert 2 * FV.DS_HEAD_BYTES > B32
