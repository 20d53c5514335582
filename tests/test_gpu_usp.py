"""The Ulysses head exchange on the MI355X (csrc/rfa_seqhead.hip; ring_flash_attn.with_ulysses).

1. The copy kernel alone, through backend.seq_head_copy, bit for bit against the torch indexing of tests/_usp_backend.py
   (written from the text of include/rfa.h, not from the kernel's index function).  The destination — with its padding and a
   spare tail — is poisoned first and compared WHOLE, so a write outside the map shows.  All four ops x three layouts; per
   pair the full product of D in {8, 72, 128, 256}, U in {2, 3, 8} and S in {2, 5, 64, 257} (odd S on ring and stripe only);
   H/U in {1, 4}, B in {1, 2} and P in {1, 2, 3} are drawn per shape from a seeded generator, independently of D, U and S and
   of each other — not their full product, which the host check (tests/native/seqhead_check.cpp) covers for the index map;
   the test asserts that every listed value of each was drawn.  The strided side is a slice of a wider tensor.  Once each:
   bf16 and fp16, the strided kv[:, :, 0] / kv[:, :, 1] views with q in ONE launch, round trips.
2. `with_ulysses` over W = U x R gloo ranks sharing the GPU (tests/_usp_worker.py) against ONE fp64 attention over the
   unsharded tensors computed on the device by rank 0 (kinds *_ring of tests/_tol.py), and bit for bit against the plain
   R-rank call."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _usp_backend as UB                        # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16
_EXT = pytest.mark.extended
POISON = 0x7A5C
OPS = {"pack": UB.PACK, "unpack": UB.UNPACK, "merged_to_slots": UB.MERGED_TO_SLOTS, "slots_to_heads": UB.SLOTS_TO_HEADS}
LAYOUTS = {"contiguous": UB.CONTIGUOUS, "zigzag": UB.ZIGZAG, "stripe": UB.STRIPE}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


def _bits(shape, gen, dt, dev):
    """random 16-bit patterns (NaNs and all: the copies move bytes) as a tensor of dtype dt"""
    return torch.randint(-32768, 32767, shape, generator=gen, dtype=torch.int16).to(dev).view(dt)


def _strided(op, U, B, S, P, Hs, D, dt, gen, dev, fill):
    """(base, view): the strided side of shape (B, rows, [P,] heads, D) as a slice of a wider, longer base tensor"""
    local = op in (UB.PACK, UB.SLOTS_TO_HEADS)
    rows, heads = (S, U * Hs) if local else (U * S, Hs)
    shape = (B, rows + 1) + ((P,) if P > 1 else ()) + (heads + 1, D + 8)
    base = _bits(shape, gen, dt, dev) if fill else torch.full(shape, POISON, dtype=torch.int16, device=dev).view(dt)
    return base, base[:, :rows, ..., :heads, :D]


def _one(be, op, layout, U, B, S, Hs, D, Ps, dt, gen, dev):
    """one launch over len(Ps) tensors against the torch copy; everything either side could have touched is compared"""
    from_slots = op in (UB.UNPACK, UB.SLOTS_TO_HEADS)
    pairs = [[_strided(op, U, B, S, P, Hs, D, dt, gen, dev, fill=not from_slots) for P in Ps] for _ in range(2)]
    if from_slots:
        n = sum(v.numel() for _, v in pairs[0])
        slots = [_bits((n + 64,), gen, dt, dev)] * 2
    else:
        for (b0, _), (b1, _) in zip(*pairs):
            b1.copy_(b0)
        n = sum(v.numel() for _, v in pairs[0])
        slots = [torch.full((n + 64,), POISON, dtype=torch.int16, device=dev).view(dt) for _ in range(2)]
    be.seq_head_copy(op, layout, U, [v for _, v in pairs[0]], slots[0])
    UB.torch_copy(op, layout, U, [v for _, v in pairs[1]], slots[1])
    what = f"U{U} B{B} S{S} Hs{Hs} D{D} P{Ps}"
    assert torch.equal(slots[0].view(torch.int16), slots[1].view(torch.int16)), f"slot side differs: {what}"
    for (b0, _), (b1, _) in zip(*pairs):
        assert torch.equal(b0.view(torch.int16), b1.view(torch.int16)), f"strided side differs: {what}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("op", list(OPS))
def test_copy_kernel_bit_for_bit_against_torch_indexing(op, layout):
    be, dev = _be(), _dev()
    gen = torch.Generator().manual_seed(77)
    draw = torch.Generator().manual_seed(1000 + 10 * OPS[op] + LAYOUTS[layout])
    seen = set()
    for D, U, S in itertools.product((8, 72, 128, 256), (2, 3, 8), (2, 5, 64, 257)):
        if layout == "zigzag" and S % 2:
            continue
        Hs, B, P = (vals[int(torch.randint(len(vals), (1,), generator=draw))] for vals in ((1, 4), (1, 2), (1, 2, 3)))
        seen |= {("Hs", Hs), ("B", B), ("P", P)}
        _one(be, OPS[op], LAYOUTS[layout], U, B, S, Hs, D, (P,), BF, gen, dev)
    assert len(seen) == 7, seen
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", [BF, FP16], ids=["bf16", "fp16"])
def test_q_and_the_two_strided_views_of_a_packed_kv_in_one_launch_and_round_trips(dt):
    """q (H 8) with kv[:, :, 0] and kv[:, :, 1] (Hk 4) of ONE packed kv as three tensors of one launch — the benchmark's input
    —, against torch; then UNPACK, MERGED_TO_SLOTS and SLOTS_TO_HEADS bring the very tensors back, for every layout"""
    be, dev = _be(), _dev()
    gen = torch.Generator().manual_seed(78)
    U, B, S, D = 2, 2, 66, 128
    q = _bits((B, S, 8, D), gen, dt, dev)
    kv = _bits((B, S, 2, 4, D), gen, dt, dev)
    srcs = [q, kv[:, :, 0], kv[:, :, 1]]
    assert not srcs[1].is_contiguous()
    n = sum(t.numel() for t in srcs)
    for layout in LAYOUTS.values():
        sent, want = (torch.full((n,), POISON, dtype=torch.int16, device=dev).view(dt) for _ in range(2))
        be.seq_head_copy(UB.PACK, layout, U, srcs, sent)
        UB.torch_copy(UB.PACK, layout, U, srcs, want)
        assert torch.equal(sent.view(torch.int16), want.view(torch.int16))
        merged = [torch.full((B, U * S, t.shape[2] // U, D), POISON, dtype=torch.int16, device=dev).view(dt) for t in srcs]
        be.seq_head_copy(UB.UNPACK, layout, U, merged, sent)
        check = [torch.empty_like(t) for t in merged]
        UB.torch_copy(UB.UNPACK, layout, U, check, want)
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(merged, check))
        back = torch.full((n,), POISON, dtype=torch.int16, device=dev).view(dt)
        be.seq_head_copy(UB.MERGED_TO_SLOTS, layout, U, merged, back)
        assert torch.equal(back.view(torch.int16), sent.view(torch.int16))                 # round trip 1
        q2, kv2 = torch.empty_like(q), torch.empty_like(kv)
        be.seq_head_copy(UB.SLOTS_TO_HEADS, layout, U, [q2, kv2[:, :, 0], kv2[:, :, 1]], back)
        assert torch.equal(q2.view(torch.int16), q.view(torch.int16))                      # round trip 2
        assert torch.equal(kv2.view(torch.int16), kv.view(torch.int16))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. the schedules
def _core(U, R):
    c = dict(U=U, R=R, S=256, H=8, D=128, causal=True, checks=("fp64",))
    return [
        dict(c, kind="ring", B=1, Hk=2, checks=("fp64", "plain")),          # (also bit-identical to the plain R-rank call)
        dict(c, kind="ring", B=2, Hk=4, window=(300, 0)),
        dict(c, kind="zigzag", zz="ring", B=2, Hk=2),
        dict(c, kind="zigzag", zz="gather", B=1, Hk=4),
        dict(c, kind="stripe", B=1, Hk=2),
        dict(c, kind="stripe", B=2, Hk=4, form="kvpacked"),
    ]


def _world(W, cases):
    import _usp_worker as UW

    errs, notes, _ = UW.run_world(W, cases, True, free_port(), limit_s=240)
    print("\n".join(notes))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("U,R", [(2, 1), (2, 2)], ids=["W2-U2", "W4-U2xR2"])
def test_with_ulysses_over_ranks_sharing_the_gpu(U, R):
    """S = 256 rows per rank, H 8 / Hk 2 or 4, D = 128, B = 1 and 2, causal and one window that cuts a shard: ring, zigzag
    (ring and gather exchange forms), stripe"""
    _world(U * R, _core(U, R))


@_EXT
@pytest.mark.parametrize("cases", [
    [dict(kind="ring", U=4, R=2, B=1, S=256, H=8, Hk=4, D=64, causal=True, dtype="fp16", checks=("fp64",)),
     dict(kind="zigzag", zz="ring", U=4, R=2, B=2, S=256, H=8, Hk=4, D=64, causal=True, checks=("fp64", "plain"))],
    [dict(kind="zigzag", zz="ring", form="qkvpacked", U=8, R=1, B=1, S=256, H=8, Hk=8, D=256, causal=True, checks=("fp64",)),
     dict(kind="stripe", U=8, R=1, B=1, S=256, H=8, Hk=8, D=256, causal=True, checks=("fp64",))],
], ids=["U4xR2-D64-fp16", "U8xR1-D256-qkvpacked"])
def test_with_ulysses_over_eight_ranks(cases):
    _world(8, cases)
