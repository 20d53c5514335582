"""The Ulysses head exchange (ring_flash_attn.with_ulysses, make_usp_groups), no device: the index arithmetic of the copy kernel
(a stand-alone C++ program under ASan / UBSan), the C ABI of rfa_seq_head_copy (layout against a compiled C snippet, every
argument check with pointers that are never dereferenced), the binder's contract, and — under gloo on the CPU test backend
with the copies written in torch indexing (tests/_usp_backend.py) — the exchange as pure data movement: bit for bit against the
plain call at world size R, within the *_ring kinds of tests/_tol.py of ONE fp64 attention over the unsharded tensors, the
count of collectives, activation checkpointing."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conftest import free_port                   # noqa: E402
import _usp_worker as UW                         # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")


# ---------------------------------------------------------------------------------------------- the index arithmetic
def test_index_function_host_check_under_asan_and_ubsan():
    """tests/native/seqhead_check.cpp: every chunk of every op x layout over the stated grid — offsets in bounds, a bijection,
    undone by the inverse op, merged rows as in the table — on the very header the kernel includes"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "seqhead_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "seqhead_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "3840 configurations ok" in res.stdout, res.stdout


# ---------------------------------------------------------------------------------------------- C ABI
def test_struct_matches_the_c_layout_and_the_abi_stays(built):
    from ring_flash_attn import _C

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rfa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rfa_seq_head_args), sizeof(rfa_seq_head_tensor),
         offsetof(rfa_seq_head_args, op), offsetof(rfa_seq_head_args, U), offsetof(rfa_seq_head_args, elem_bytes),
         offsetof(rfa_seq_head_args, t), offsetof(rfa_seq_head_args, slots), offsetof(rfa_seq_head_args, slots_elems),
         offsetof(rfa_seq_head_tensor, batch), offsetof(rfa_seq_head_tensor, part), offsetof(rfa_seq_head_tensor, P),
         offsetof(rfa_seq_head_tensor, H));
  printf("%d %d %d %d %d %d %d\n", RFA_SEQHEAD_PACK, RFA_SEQHEAD_UNPACK, RFA_SEQHEAD_MERGED_TO_SLOTS, RFA_SEQHEAD_SLOTS_TO_HEADS,
         RFA_SEQHEAD_CONTIGUOUS, RFA_SEQHEAD_ZIGZAG, RFA_SEQHEAD_STRIPE);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A, T = _C.SeqHeadArgs, _C.SeqHeadTensor
    assert got[:12] == [C.sizeof(A), C.sizeof(T), A.op.offset, A.U.offset, A.elem_bytes.offset, A.t.offset, A.slots.offset,
                        A.slots_elems.offset, T.batch.offset, T.part.offset, T.P.offset, T.H.offset]
    assert A.struct_bytes.offset == 0 and A.reserved.offset == 4                     # leads with struct_bytes / reserved
    assert got[12:] == [_C.SEQHEAD_PACK, _C.SEQHEAD_UNPACK, _C.SEQHEAD_MERGED_TO_SLOTS, _C.SEQHEAD_SLOTS_TO_HEADS,
                        _C.SEQHEAD_CONTIGUOUS, _C.SEQHEAD_ZIGZAG, _C.SEQHEAD_STRIPE]
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert "rfa_seq_head_copy" in _C.SYMBOLS
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)            # ONE new entry point, all bound


def _args(**kw):
    from ring_flash_attn import _C

    a = _C.SeqHeadArgs()
    a.op, a.layout, a.U, a.B, a.S, a.D, a.elem_bytes, a.ntensors = 0, 0, 2, 2, 6, 32, 2, 1
    a.slots, a.slots_elems = 256, 2 * 6 * 8 * 32              # (addresses that are never dereferenced)
    t = a.t[0]
    t.ptr, t.batch, t.row, t.part, t.head, t.P, t.H = 512, 6 * 8 * 32, 8 * 32, 0, 32, 1, 8
    tk = {}
    for k, v in kw.items():
        if k.startswith("t_"):
            tk[k[2:]] = v
        else:
            setattr(a, k, v)
    for k, v in tk.items():
        setattr(a.t[0], k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    from ring_flash_attn import _C

    lib = _C.load()
    call = lambda **kw: lib.rfa_seq_head_copy(C.byref(_args(**kw)), None)
    assert lib.rfa_seq_head_copy(None, None) == ERR_NULL
    bad = {
        ERR_ARGS: [dict(struct_bytes=C.sizeof(_C.SeqHeadArgs) - 8), dict(struct_bytes=C.sizeof(_C.SeqHeadArgs) + 8), dict(reserved=1),
                   dict(op=4), dict(op=-1), dict(layout=3), dict(layout=-1), dict(ntensors=0), dict(ntensors=4), dict(t_P=0),
                   dict(t_P=4), dict(slots_elems=2 * 6 * 8 * 32 - 1)],
        ERR_DTYPE: [dict(elem_bytes=4), dict(elem_bytes=1)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(D=-8)],
        ERR_SHAPE: [dict(U=0), dict(U=-2), dict(B=-1), dict(S=-1), dict(layout=1, S=5), dict(U=2, S=2 ** 30, t_H=2),
                    dict(B=2 ** 20, S=2 ** 10, slots_elems=2 ** 62)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=7), dict(U=3), dict(t_H=-2)],
        ERR_NULL: [dict(slots=None), dict(t_ptr=None)],
        ERR_ALIGN: [dict(slots=264), dict(t_ptr=520), dict(t_row=8 * 32 + 4), dict(t_batch=6 * 8 * 32 + 2), dict(t_head=36),
                    dict(t_P=2, t_part=4, t_H=4, t_head=32)],
    }
    for want, cases in bad.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # the order: a struct of the wrong size is refused before anything else is looked at, a dtype before a head dim, ...
    assert call(struct_bytes=8, elem_bytes=4, D=12) == ERR_ARGS
    assert call(elem_bytes=4, D=12) == ERR_DTYPE
    assert call(D=12, U=0) == ERR_HEAD_DIM
    assert call(U=0, t_H=7) == ERR_SHAPE
    assert call(t_H=7, slots=None) == ERR_HEADS
    assert call(slots=None, t_ptr=520) == ERR_NULL
    # no rows: nothing is launched and no pointer is needed
    assert call(B=0, slots=None, t_ptr=None) == OK and call(S=0, slots=None, t_ptr=None) == OK
    # `part` is not looked at for P == 1; a second tensor is checked like the first
    assert call(t_part=3, slots=None) == ERR_NULL
    a = _args(ntensors=2, slots=None)
    a.t[1].ptr, a.t[1].batch, a.t[1].row, a.t[1].head, a.t[1].P, a.t[1].H = 512, 6 * 4 * 32, 4 * 32, 32, 1, 3
    assert lib.rfa_seq_head_copy(C.byref(a), None) == ERR_HEADS
    a.t[1].H = 4
    assert lib.rfa_seq_head_copy(C.byref(a), None) == ERR_NULL
    # ... and EVERY tensor's heads are checked before ANY tensor's chunk count (which needs its H): a first tensor too large
    # does not hide a second one's bad H
    a.t[0].H, a.t[1].H = 2 ** 28, 3
    assert lib.rfa_seq_head_copy(C.byref(a), None) == ERR_HEADS
    a.t[1].H = 4
    assert lib.rfa_seq_head_copy(C.byref(a), None) == ERR_SHAPE


# ---------------------------------------------------------------------------------------------- the binder
DENSE = [f"{pre}_{form}func" for pre in ("ring_flash_attn", "zigzag_ring_flash_attn", "stripe_flash_attn")
         for form in ("", "kvpacked_", "qkvpacked_")]


def test_with_ulysses_keeps_the_signatures_and_refuses_what_it_does_not_serve(single_rank_group):
    import torch.distributed as dist

    import ring_flash_attn as R

    assert "with_ulysses" in dir(R) and "make_usp_groups" in dir(R)
    funcs = {n: getattr(R, n) for n in dir(R) if n.endswith("_func")}
    assert len(funcs) == 21                                              # the two new names do not end in _func
    ug, rg = R.make_usp_groups(R.ring_flash_attn_func, 1)                 # (a world of one rank: groups of size 1)
    assert dist.get_world_size(ug) == 1 and dist.get_world_size(rg) == 1
    before = {n: str(inspect.signature(f)) for n, f in funcs.items()}
    for n, f in funcs.items():
        if n in DENSE:
            g = R.with_ulysses(f, ug)
            assert g is not f and inspect.signature(g) == inspect.signature(f) and g.__name__ == f.__name__
            assert R.with_ulysses(f, None) is f
            with pytest.raises(TypeError, match="already a with_ulysses result"):
                R.with_ulysses(g, ug)
            capped = R.with_softcap(f, 30.0)
            assert inspect.signature(R.with_ulysses(capped, ug)) == inspect.signature(f)
            with pytest.raises(TypeError, match="with_sinks result.*follow-up"):
                R.with_ulysses(R.with_sinks(f, torch.zeros(4)), ug)
        else:
            with pytest.raises(TypeError, match="follow-up"):
                R.with_ulysses(f, ug)
            with pytest.raises(TypeError, match="follow-up"):
                R.with_ulysses(f, None)
            with pytest.raises(TypeError):
                R.make_usp_groups(f, 1)
    assert {n: str(inspect.signature(f)) for n, f in funcs.items()} == before
    for notf in (None, len, lambda q, k, v: q):
        with pytest.raises(TypeError):
            R.with_ulysses(notf, ug)
    with pytest.raises(ValueError, match="does not divide"):
        R.make_usp_groups(R.ring_flash_attn_func, 2)


def test_a_ulysses_group_of_one_rank_is_the_plain_call_bit_for_bit(single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _usp_backend import UspBackend

    _testing.set_backend(UspBackend(serves=("mask_shift",)))
    try:
        ug, _ = R.make_usp_groups(R.zigzag_ring_flash_attn_func, 1)
        g = torch.Generator().manual_seed(2)
        q, k, v, do = (torch.randn(2, 12, h, 32, generator=g).bfloat16() for h in (4, 2, 2, 4))
        got = []
        for fn in (R.with_ulysses(R.zigzag_ring_flash_attn_func, ug), R.zigzag_ring_flash_attn_func):
            ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
            out, lse, _ = fn(*ins, causal=True, return_attn_probs=True)
            out.backward(do)
            got.append((out, lse) + tuple(t.grad for t in ins))
        assert all(torch.equal(a, b) for a, b in zip(*got))
    finally:
        _testing.set_backend(None)


# ---------------------------------------------------------------------------------------------- the exchange under gloo
def _cases(U, R):
    H, Hk = (12, 6) if U == 3 else (8, 4)
    c = dict(U=U, R=R, B=2, S=12, H=H, Hk=Hk, D=32, causal=True)
    out = [dict(c, kind=kind, form=form, checks=("plain", "fp64", "count", "ckpt", "only_q") if form == "func" else ("plain", "fp64"))
           for kind in ("ring", "zigzag", "stripe") for form in ("func", "kvpacked", "qkvpacked")]
    out += [dict(c, kind=kind, causal=False) for kind in ("ring",)]          # (zigzag and stripe are causal schedules)
    out += [dict(c, kind=kind, window=(17, 0)) for kind in ("ring", "zigzag", "stripe")]    # 17 keys back: cuts a 12-row shard
    out += [dict(c, kind="ring", alibi=True), dict(c, kind="zigzag", alibi=True)]
    out += [dict(c, kind="stripe", softcap=30.0), dict(c, kind="ring", form="kvpacked", softcap=30.0)]
    return out


@pytest.mark.parametrize("U,R", [(2, 1), (2, 2), (4, 1), (2, 3), (3, 2)])
def test_exchange_is_pure_data_movement_and_matches_fp64(U, R):
    """W = U x R gloo ranks.  Every case: out, lse, dq, dk, dv of with_ulysses(f, ug) at W ranks equal, bit for bit, the plain
    run of f at world size R on the merged tensors with this rank's head slice, and lie within the *_ring kinds of ONE fp64
    attention over the unsharded tensors.  The `func` form of every family also counts the collectives — exactly one
    all-to-all on the Ulysses group in front of and one behind the wrapped call, forward and backward, alike on every rank —
    and re-runs under activation checkpointing."""
    cases = _cases(U, R)
    errs, notes, counts = UW.run_world(U * R, cases, False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
    counted = [UW.case_name(c) for c in cases if "count" in c.get("checks", ())]
    assert len(counted) == 3
    for r in range(U * R):
        assert counts[r] == {n: ("AFA", "ABA") for n in counted}, (r, counts[r])


def test_every_refusal_at_the_call_comes_before_anything_is_exchanged():
    errs, _, _ = UW.run_world(2, [dict(refusals=True, U=2, checks=())], False, free_port())
    assert not errs, "\n".join(errs)
