"""Rotary embedding at global positions (ring_flash_attn.apply_rotary, local_positions), no device: the index arithmetic of the
kernel (a stand-alone C++ program under ASan / UBSan), the C ABI of rfa_rotary (layout against a compiled C snippet, every
argument check with pointers that are never dereferenced), `local_positions` of all 21 functions against each family's own
sharding of arange, and — on the CPU test backend with the rotation written in torch fp32 (tests/_rotary_backend.py) — the bit
properties of `apply_rotary` on shards, its gradients against fp64 autograd of the textbook formula, and its argument handling."""
import ctypes as C
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
import _rotary_worker as RW                      # noqa: E402
from _droppos_worker import PREFIX, shard, unshard   # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")


# ---------------------------------------------------------------------------------------------- the index arithmetic
def test_index_functions_host_check_under_asan_and_ubsan():
    """tests/native/rotary_check.cpp: every unit of every configuration of the stated grid — offsets in bounds, every rotated
    and every pass-through element written exactly once and nothing else, partners / roles / table columns, map positions, far
    strides — on the very header the kernel includes"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rotary_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "rotary_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "3504 configurations ok" in res.stdout, res.stdout


# ---------------------------------------------------------------------------------------------- C ABI
def test_struct_matches_the_c_layout_and_the_abi_stays(built):
    from ring_flash_attn import _C

    fields_a = ["ntensors", "B", "S", "D", "dtype", "R", "rot_offset", "interleaved", "conj", "table_dtype", "t", "cos", "sin", "P",
                "positions", "pos_batch", "pos_offset", "pos_stride", "pos_split", "pos_offset2"]
    fields_t = ["src", "dst", "src_batch", "src_row", "src_head", "dst_batch", "dst_row", "dst_head", "H", "pad"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu %zu %d\\n", sizeof(rfa_rotary_args), sizeof(rfa_rotary_tensor), RFA_ROTARY_TABLE_F32);\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_rotary_args, {f}));\n' for f in fields_a) + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_rotary_tensor, {f}));\n' for f in fields_t) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A, T = _C.RotaryArgs, _C.RotaryTensor
    assert got[:3] == [C.sizeof(A), C.sizeof(T), _C.ROTARY_TABLE_F32]
    assert got[3:] == [getattr(A, f).offset for f in fields_a] + [getattr(T, f).offset for f in fields_t]
    assert [f for f, _ in A._fields_] == ["struct_bytes", "reserved"] + fields_a and [f for f, _ in T._fields_] == fields_t
    assert A.struct_bytes.offset == 0 and A.reserved.offset == 4                     # leads with struct_bytes / reserved
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert "rfa_rotary" in _C.SYMBOLS
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)            # ONE new entry point, all bound


def _args(**kw):
    from ring_flash_attn import _C

    a = _C.RotaryArgs()
    a.ntensors, a.B, a.S, a.D, a.dtype, a.R, a.rot_offset, a.table_dtype = 1, 2, 6, 32, 0, 32, 0, _C.ROTARY_TABLE_F32
    a.cos, a.sin, a.P = 4096, 8192, 16                         # (addresses that are never dereferenced)
    t = a.t[0]
    t.src, t.dst, t.H = 512, 1 << 20, 8
    t.src_batch, t.src_row, t.src_head = 6 * 8 * 32, 8 * 32, 32
    t.dst_batch, t.dst_row, t.dst_head = 6 * 8 * 32, 8 * 32, 32
    for k, v in kw.items():
        if k.startswith("t_"):
            setattr(a.t[0], k[2:], v)
        else:
            setattr(a, k, v)
    return a


def test_every_argument_check_returns_before_a_pointer_is_read(built):
    from ring_flash_attn import _C

    lib = _C.load()
    call = lambda **kw: lib.rfa_rotary(C.byref(_args(**kw)), None)
    assert lib.rfa_rotary(None, None) == ERR_NULL
    size = C.sizeof(_C.RotaryArgs)
    # past every host check the call would launch: the cases below each stop at the check they name (a case that passed them
    # all would dereference the made-up addresses, so there is none)
    bad = {
        ERR_ARGS: [dict(struct_bytes=size - 8), dict(struct_bytes=size + 8), dict(reserved=1), dict(ntensors=0), dict(ntensors=3),
                   dict(interleaved=2), dict(interleaved=-1), dict(conj=2), dict(conj=-1), dict(t_pad=1),
                   dict(t_dst=512, t_dst_row=8 * 32 + 8), dict(pos_batch=-1), dict(pos_stride=-1), dict(pos_split=6),
                   dict(pos_split=-1), dict(pos_offset=11), dict(pos_offset=-1), dict(P=5), dict(pos_stride=3, P=15),
                   dict(pos_split=3, pos_offset2=14), dict(pos_split=3, pos_offset2=-1), dict(pos_offset=1 << 62)],
        ERR_DTYPE: [dict(dtype=2), dict(dtype=-1), dict(table_dtype=1), dict(table_dtype=3), dict(dtype=1, table_dtype=0)],
        ERR_HEAD_DIM: [dict(D=0), dict(D=12), dict(D=264), dict(D=-8), dict(R=0), dict(R=-16), dict(R=24), dict(R=48),
                       dict(interleaved=1, R=12), dict(rot_offset=4), dict(rot_offset=-8), dict(rot_offset=8), dict(R=16, rot_offset=24)],
        ERR_SHAPE: [dict(B=-1), dict(S=-1), dict(P=0), dict(P=-3), dict(B=2 ** 16, S=2 ** 15), dict(B=2 ** 15, S=2 ** 15, t_H=2),
                    dict(B=2 ** 14, S=2 ** 13, t_H=8), dict(B=2 ** 14, S=2 ** 13, t_H=4, D=64, R=16)],
        ERR_HEADS: [dict(t_H=0), dict(t_H=-2)],
        ERR_NULL: [dict(cos=None), dict(sin=None), dict(t_src=None), dict(t_dst=None)],
        ERR_ALIGN: [dict(cos=4100), dict(sin=8200), dict(t_src=520), dict(t_dst=(1 << 20) + 8), dict(t_src_row=8 * 32 + 4),
                    dict(t_src_batch=6 * 8 * 32 + 2), dict(t_src_head=36), dict(t_dst_row=8 * 32 + 4), dict(t_dst_batch=3),
                    dict(t_dst_head=36)],
    }
    for want, cases in bad.items():
        for kw in cases:
            assert call(**kw) == want, (want, kw)
    # (2^14 * 2^13 * 4 heads * 1 unit is 2^29 in place ... the out-of-place call has 1 + 6 units per head: 7 * 2^29 > 2^31 - 1)
    assert call(B=2 ** 14, S=2 ** 13, t_H=4, D=64, R=16, t_dst=512, cos=None) == ERR_NULL
    # the order: a struct of the wrong size is refused before anything else is looked at, a dtype before a head dim, ...
    assert call(struct_bytes=8, dtype=2, D=12) == ERR_ARGS
    assert call(dtype=2, D=12) == ERR_DTYPE
    assert call(D=12, B=-1) == ERR_HEAD_DIM
    assert call(R=24, B=-1) == ERR_HEAD_DIM
    assert call(B=-1, t_H=0) == ERR_SHAPE
    assert call(t_H=0, cos=None) == ERR_HEADS
    assert call(cos=None, t_src=520) == ERR_NULL
    assert call(t_src=520, pos_stride=-1) == ERR_ALIGN
    # no rows: nothing is launched and no pointer is needed; the map is not looked at either
    assert call(B=0, cos=None, sin=None, t_src=None, t_dst=None) == OK
    assert call(S=0, cos=None, sin=None, t_src=None, t_dst=None, pos_split=3) == OK
    # a second tensor is checked like the first, and EVERY tensor's heads before ANY tensor's unit count
    a = _args(ntensors=2, cos=None)
    a.t[1].src, a.t[1].dst, a.t[1].H = 512, 512, 0
    assert lib.rfa_rotary(C.byref(a), None) == ERR_HEADS
    a.t[1].H = 2
    assert lib.rfa_rotary(C.byref(a), None) == ERR_NULL
    a.t[0].H, a.t[1].H = 2 ** 30, 0
    assert lib.rfa_rotary(C.byref(a), None) == ERR_HEADS
    a.t[1].H = 2
    assert lib.rfa_rotary(C.byref(a), None) == ERR_SHAPE
    # with `positions` the map's fields are not looked at (the kernel clamps what it reads)
    assert call(positions=64, pos_stride=-1, pos_split=99, P=1, cos=None) == ERR_NULL
    # the largest position the map reaches: row 5 of 6 at offset 10 needs 16 table rows
    assert call(pos_offset=10, cos=None) == ERR_NULL and call(pos_offset=10, P=15) == ERR_ARGS


# ---------------------------------------------------------------------------------------------- local_positions
def _funcs(R, family):
    return [getattr(R, f"{family}_{form}func") for form in ("", "kvpacked_", "qkvpacked_")]


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_local_positions_of_all_21_functions_are_the_shards_of_arange(W):
    """Each family's own sharding applied to the positions of the unsharded input, compared exactly.  Dense: the shard helper
    of the multi-rank workers on arange(W * n).  Packed: documents of lengths [96, 160] and an uneven third one of 56 — for the
    llama3 families these are the GLOBAL lengths (312 tokens: divisible by every 2W here); the ring / zigzag varlen families
    shard every document by itself, so there they are the LOCAL lengths of documents W times as long."""
    import ring_flash_attn as R
    from ring_flash_attn import local_positions

    seen = set()
    for kind, family in PREFIX.items():
        for n in (38, 6):
            full = torch.arange(W * n, dtype=torch.int32)
            for r in range(W):
                for f in _funcs(R, family):
                    got = local_positions(f, n, rank=r, world_size=W)
                    assert got.dtype == torch.int32 and torch.equal(got, shard(kind, full, r, W, dim=0)), (family, W, r)
                    seen.add(f)
    lens = [96, 160, 56]
    for zig, family in ((False, "ring_flash_attn_varlen"), (True, "zigzag_ring_flash_attn_varlen")):
        cu_local = torch.tensor([0, 96, 256, 312], dtype=torch.int32)
        for r in range(W):
            parts = []
            for L in lens:
                doc = torch.arange(L * W, dtype=torch.int32)
                parts.append(shard("zigzag" if zig else "ring", doc, r, W, dim=0))
            for f in _funcs(R, family):
                got = local_positions(f, 312, rank=r, world_size=W, cu_seqlens=cu_local)
                assert got.dtype == torch.int32 and torch.equal(got, torch.cat(parts)), (family, W, r)
                seen.add(f)
    cu = torch.tensor([0, 96, 256, 312], dtype=torch.int32)
    stream = torch.cat([torch.arange(L, dtype=torch.int32) for L in lens])            # the position of every token of the stream
    for r in range(W):
        for f in _funcs(R, "llama3_flash_attn_varlen"):
            got = local_positions(f, 312 // W, rank=r, world_size=W, cu_seqlens=cu)
            assert got.dtype == torch.int32 and torch.equal(got, shard("ring", stream, r, W, dim=0)), ("llama3", W, r)
            seen.add(f)
        cu_q, cu_k, *_ = R.llama3_flash_attn_prepare_cu_seqlens(cu, True, r, W)
        _against_prepare(got, [(cu_q, cu_k)])
        for f in _funcs(R, "zigzag_llama3_flash_attn_varlen"):
            got = local_positions(f, 312 // W, rank=r, world_size=W, cu_seqlens=cu)
            assert got.dtype == torch.int32 and torch.equal(got, shard("zigzag", stream, r, W, dim=0)), ("zigzag_llama3", W, r)
            seen.add(f)
        _against_prepare(got, [(p[0], p[1]) for p in R.zigzag_llama3_flash_attn_prepare_cu_seqlens(cu, True, r, W)])
    assert len(seen) == 21 == len([n for n in dir(R) if n.endswith("_func")])


def _against_prepare(got, params):
    """the split as *_prepare_cu_seqlens itself states it (causal: a piece's keys end with its last query): inside every piece
    of every slice the positions count up by one, and the piece's last query sits at (its keys) - 1"""
    got = got.tolist()
    base = 0
    for cu_q, cu_k in params:
        cu_q, cu_k = cu_q.tolist(), cu_k.tolist()
        for j in range(len(cu_q) - 1):
            a, b = base + cu_q[j], base + cu_q[j + 1]
            assert got[a:b] == list(range(got[a], got[a] + b - a))
            assert got[b - 1] == cu_k[j + 1] - cu_k[j] - 1
        base += cu_q[-1]
    assert base == len(got)


def test_local_positions_refusals(single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import local_positions

    assert local_positions(R.ring_flash_attn_func, 4).tolist() == [0, 1, 2, 3]          # the group's rank and size: one rank
    for notf in (None, len, lambda q, k, v: q, R.with_softcap(R.ring_flash_attn_func, 30.0), R.apply_rotary,
                 R.llama3_flash_attn_prepare_cu_seqlens):
        with pytest.raises(TypeError):
            local_positions(notf, 4, rank=0, world_size=1)
    with pytest.raises(ValueError, match="odd"):
        local_positions(R.zigzag_ring_flash_attn_func, 5, rank=0, world_size=2)
    with pytest.raises(ValueError, match="outside"):
        local_positions(R.ring_flash_attn_func, 4, rank=2, world_size=2)
    with pytest.raises(ValueError, match="needs cu_seqlens"):
        local_positions(R.llama3_flash_attn_varlen_func, 4, rank=0, world_size=2)
    with pytest.raises(ValueError, match="takes no cu_seqlens"):
        local_positions(R.ring_flash_attn_func, 4, rank=0, world_size=2, cu_seqlens=[0, 4])
    with pytest.raises(ValueError, match="rows per rank"):
        local_positions(R.llama3_flash_attn_varlen_func, 5, rank=0, world_size=2, cu_seqlens=[0, 8])


# ---------------------------------------------------------------------------------------------- apply_rotary on the test backend
@pytest.fixture
def rotary_backend():
    from ring_flash_attn import _testing
    from _rotary_backend import RotaryBackend

    be = RotaryBackend(serves=("mask_shift",))
    _testing.set_backend(be)
    yield be
    _testing.set_backend(None)


def _tables(P, R, dtype=torch.float32):
    ang = torch.arange(P, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(R // 2, dtype=torch.float64) / (R // 2)))
    return ang.cos().to(dtype), ang.sin().to(dtype)


def _qk(B, S, H, Hk, D, dtype=torch.bfloat16, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, H, D, generator=g).to(dtype), torch.randn(B, S, Hk, D, generator=g).to(dtype)


@pytest.mark.parametrize("kind", ["ring", "zigzag", "stripe"])
@pytest.mark.parametrize("W", [2, 4])
def test_every_ranks_shard_is_the_shard_of_the_single_device_result(rotary_backend, kind, W):
    """positions = local_positions(rank=r): rotating rank r's shard gives, bit for bit, rank r's shard of the rotated full
    tensor — for both pairings, a rot_offset, with and without k.  (`layout=` on real groups: the worlds below.)"""
    import ring_flash_attn as R

    func = getattr(R, PREFIX[kind] + "_func")
    for inter, D, Rw, ro in ((False, 64, 64, 0), (True, 40, 8, 8), (False, 192, 64, 128)):
        q, k = _qk(2, W * 10, 3, 1, D)
        cos, sin = _tables(W * 10, Rw)
        kw = dict(interleaved=inter, rot_offset=ro)
        qf, kf = R.apply_rotary(q, k, cos, sin, **kw)
        assert not torch.equal(qf, q)
        parts = []
        for r in range(W):
            pos = R.local_positions(func, 10, rank=r, world_size=W)
            qs, ks = R.apply_rotary(shard(kind, q, r, W), shard(kind, k, r, W), cos, sin, positions=pos, **kw)
            assert torch.equal(R.apply_rotary(shard(kind, q, r, W), None, cos, sin, positions=pos, **kw), qs)
            parts.append((qs, ks))
        assert torch.equal(unshard(kind, [p[0] for p in parts]), qf) and torch.equal(unshard(kind, [p[1] for p in parts]), kf)


def _world_cases(W):
    base = dict(W=W, S=10, B=2, H=4, Hk=2, D=32, R=32)
    cases = [dict(base, kind=kind, attn=True) for kind in ("ring", "zigzag", "stripe")]
    cases.append(dict(base, kind="zigzag", D=40, R=8, rot_offset=8, interleaved=True))
    if W == 4:
        cases += [dict(base, kind=kind, attn=True, U=2) for kind in ("ring", "zigzag", "stripe")]    # with_ulysses' sharding
    return cases


@pytest.mark.parametrize("W", [2, 4])
def test_layout_on_real_groups_and_the_attention_behind_it(W):
    """W gloo ranks: apply_rotary(layout=func) on every rank's shard — the map's four numbers from the group's rank — equals the
    explicit positions in bits and un-shards to the single-device rotation bit for bit; `func` (W = 4: also
    with_ulysses(func, ug) over 2 x 2 ranks, whose caller shards like func over all four) on the rotated shards lies within the
    *_ring kinds of exact attention over the rotated full tensors, the gradients those of the conjugate rotation."""
    from _rotary_backend import reference

    cases = _world_cases(W)
    res, errs = RW.run_world(W, cases, False, free_port())
    assert not errs, "\n".join(errs)
    bad = [b for c in cases for b in RW.check_case(c, res[RW.case_name(c)], reference)]
    assert not bad, "\n".join(bad)


def _textbook(x, cos, sin, pos, inter, ro):
    """differentiable, any dtype: the formula as papers print it"""
    Rw = 2 * cos.shape[1]
    c, s = cos[pos].unsqueeze(-2), sin[pos].unsqueeze(-2)
    r = x[..., ro:ro + Rw]
    if inter:
        x1, x2 = r[..., 0::2], r[..., 1::2]
        rot = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)
    else:
        x1, x2 = r[..., :Rw // 2], r[..., Rw // 2:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return torch.cat([x[..., :ro], rot, x[..., ro + Rw:]], dim=-1)


U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # below the smallest normal number the rounding is absolute


def _within(got, ref, mag, dtype, factor=1.0):
    lim = factor * ((U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + 2.0 ** -22 * mag)
    return bool(((got.double() - ref).abs() <= lim).all())


@pytest.mark.parametrize("inter,D,Rw,ro", [(False, 64, 64, 0), (True, 64, 32, 16), (False, 192, 64, 128)])
@pytest.mark.parametrize("dtype,tdtype", [(torch.bfloat16, torch.float32), (torch.float16, torch.float16)])
def test_forward_and_gradients_against_fp64_autograd_of_the_textbook_formula(rotary_backend, inter, D, Rw, ro, dtype, tdtype):
    """out, dq and dk within one rounding to the io dtype plus the fp32 products' error (u |ref| + 2^-22 (|x1 c| + |x2 s|)) of
    fp64 autograd through the textbook formula, with fp32 and io-dtype tables, (B, S) positions, and packed input"""
    import ring_flash_attn as R
    from _rotary_backend import reference

    B, S = 2, 11
    q, k = _qk(B, S, 3, 1, D, dtype)
    cos, sin = _tables(40, Rw, tdtype)
    g = torch.Generator().manual_seed(8)
    pos = torch.randint(0, 40, (B, S), generator=g).to(torch.int32)
    dq_out, dk_out = _qk(B, S, 3, 1, D, dtype, seed=6)
    qa, ka = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    qo, ko = R.apply_rotary(qa, ka, cos, sin, positions=pos, interleaved=inter, rot_offset=ro)
    assert qo.dtype == dtype and qo.is_contiguous() and not cos.requires_grad
    torch.autograd.backward([qo, ko], [dq_out, dk_out])
    for x, out, dout, grad in ((q, qo, dq_out, qa.grad), (k, ko, dk_out, ka.grad)):
        x64 = x.double().requires_grad_(True)
        ref = _textbook(x64, cos.double(), sin.double(), pos.long(), inter, ro)
        ref.backward(dout.double())
        ref2, mag = reference(x, cos, sin, pos, inter, ro)
        assert torch.equal(ref2, ref.detach())                                       # (the two statements of the formula agree)
        assert _within(out, ref.detach(), mag, dtype)
        gref, gmag = reference(dout, cos, sin, pos, inter, ro, conj=True)
        assert torch.allclose(gref, x64.grad, rtol=0, atol=1e-12)
        assert _within(grad, x64.grad, gmag, dtype)
    # packed input: (T, H, D) with (T,) positions is the (1, T, H, D) call
    qp = q.reshape(B * S, 3, D)
    out_p = R.apply_rotary(qp, None, cos, sin, positions=pos.reshape(-1), interleaved=inter, rot_offset=ro)
    assert torch.equal(out_p, qo.detach().reshape(B * S, 3, D))
    # the backward saved the tables and the positions, neither inputs nor outputs, and ran the conjugate on the gradients
    calls = rotary_backend.rotary_calls
    assert [c["conj"] for c in calls[:2]] == [False, True] and calls[0]["n"] == calls[1]["n"] == 2


def test_modes_flags_and_inplace(rotary_backend):
    import ring_flash_attn as R

    q, k = _qk(2, 12, 4, 2, 64)
    cos, sin = _tables(64, 32)
    ref_q, ref_k = R.apply_rotary(q, k, cos, sin, rot_offset=16)
    # neither layout nor positions: row i at offset + i; offset is added in every mode
    ar = torch.arange(12, dtype=torch.int32)
    off_q = R.apply_rotary(q, None, cos, sin, rot_offset=16, offset=7)
    assert torch.equal(off_q, R.apply_rotary(q, None, cos, sin, rot_offset=16, positions=ar + 7))
    assert torch.equal(off_q, R.apply_rotary(q, None, cos, sin, rot_offset=16, positions=ar, offset=7))
    assert torch.equal(ref_q, R.apply_rotary(q, None, cos, sin, rot_offset=16, positions=ar))
    assert not torch.equal(off_q, ref_q)
    # pass-through columns are the input's bits; the rotated ones are not
    assert torch.equal(ref_q[..., :16], q[..., :16]) and torch.equal(ref_q[..., 48:], q[..., 48:])
    assert not torch.equal(ref_q[..., 16:48], q[..., 16:48])
    # io-dtype tables are accepted; explicit positions outside the tables clamp to their ends
    R.apply_rotary(q, k, cos.bfloat16(), sin.bfloat16())
    far = torch.tensor([-1, 64] + [3] * 10, dtype=torch.int32)
    near = torch.tensor([0, 63] + [3] * 10, dtype=torch.int32)
    assert torch.equal(R.apply_rotary(q, None, cos, sin, positions=far), R.apply_rotary(q, None, cos, sin, positions=near))
    # strided views (the slices of a qkv tensor) are served as they are and give the bits of their contiguous copies
    qkv = torch.randn(2, 12, 3, 4, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    n0 = len(rotary_backend.rotary_calls)
    a, b = R.apply_rotary(qkv[:, :, 0], qkv[:, :, 1], cos, sin)
    c, d = R.apply_rotary(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), cos, sin)
    assert torch.equal(a, c) and torch.equal(b, d) and len(rotary_backend.rotary_calls) == n0 + 2      # one launch for q and k
    # inplace: the inputs are marked dirty and returned; the result is the out-of-place one; q and k ride in one launch
    q2, k2 = q.clone(), k.clone()
    v0 = q2._version
    rq, rk = R.apply_rotary(q2, k2, cos, sin, rot_offset=16, inplace=True)
    assert rq is q2 and rk is k2 and q2._version > v0 and torch.equal(q2, ref_q) and torch.equal(k2, ref_k)
    assert rotary_backend.rotary_calls[-1]["inplace"] == [True, True]
    # ... with autograd: a non-leaf is rotated in place and the gradient flows through the conjugate
    leaf = q.clone().float().requires_grad_(True)
    mid = leaf.bfloat16()
    out = R.apply_rotary(mid, None, cos, sin, rot_offset=16, inplace=True)
    assert out is mid
    out.backward(torch.ones_like(out))
    plain = q.clone().requires_grad_(True)
    R.apply_rotary(plain, None, cos, sin, rot_offset=16).backward(torch.ones_like(q))
    assert torch.equal(leaf.grad.bfloat16(), plain.grad)
    with pytest.raises(RuntimeError):                                                  # (a leaf that requires grad: autograd's rule)
        R.apply_rotary(q.clone().requires_grad_(True), None, cos, sin, inplace=True)
    # ... on the views of a qkv tensor under autograd (one Function per tensor: autograd's rule for views)
    base = qkv.clone().float().requires_grad_(True)
    w = base.bfloat16()
    e, f = R.apply_rotary(w[:, :, 0], w[:, :, 1], cos, sin, inplace=True)
    assert torch.equal(w[:, :, 0], a) and torch.equal(w[:, :, 1], b) and torch.equal(w[:, :, 2], qkv[:, :, 2])
    w.sum().backward()
    assert base.grad is not None and torch.equal(base.grad[:, :, 2], torch.ones_like(base.grad[:, :, 2]))


def test_every_refusal_comes_before_a_launch(rotary_backend, single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _usp_backend import UspBackend

    q, k = _qk(2, 12, 4, 2, 64)
    cos, sin = _tables(64, 32)
    ar = torch.arange(12, dtype=torch.int32)
    value = [
        (dict(layout=R.ring_flash_attn_func, positions=ar), "at most one"),
        (dict(q=q.float()), "bf16"), (dict(q=q[..., :60]), "head dim"), (dict(q=q[0, 0]), r"\(B, S, H, D\)"),
        (dict(k=k[:, :6]), "k must share"), (dict(k=k.half()), "k must share"), (dict(k=k[..., :32]), "k must share"),
        (dict(cos=cos[:, :8]), "one shape"), (dict(cos=cos.double(), sin=sin.double()), "fp32 or"),
        (dict(cos=cos.half(), sin=sin.half()), "fp32 or"), (dict(cos=cos.t().contiguous().t(), sin=sin.t().contiguous().t()), "contiguous"),
        (dict(cos=cos[:, :12].contiguous(), sin=sin[:, :12].contiguous()), "multiple of 16"),
        (dict(cos=cos[:, :6].contiguous(), sin=sin[:, :6].contiguous(), interleaved=True), "multiple of 8"),
        (dict(rot_offset=4), "rot_offset"), (dict(rot_offset=40), "rot_offset"), (dict(rot_offset=-8), "rot_offset"),
        (dict(positions=ar.long()), "int32"), (dict(positions=ar[:5]), "int32"), (dict(positions=ar.view(1, 12)), "int32"),
        (dict(positions=list(range(12))), "int32"),
        (dict(offset=53), "positions 53 .. 64"), (dict(offset=-1), "positions -1 .. 10"),
        (dict(layout=R.zigzag_ring_flash_attn_func, q=q[:, :11], k=k[:, :11]), "odd"),
        (dict(layout=R.ring_flash_attn_func, q=q[0], k=k[0]), r"needs \(B, S, H, D\)"),
        (dict(inplace=True, q=q[..., 1:57], k=None, cos=cos[:, :8].contiguous(), sin=sin[:, :8].contiguous()), "inplace=True needs"),
        (dict(cos=None), "cos and sin"),
    ]
    n0 = len(rotary_backend.rotary_calls)
    for kw, match in value:
        a = dict(dict(q=q, k=k, cos=cos, sin=sin), **kw)
        with pytest.raises(ValueError, match=match):
            R.apply_rotary(a.pop("q"), a.pop("k"), a.pop("cos"), a.pop("sin"), **a)
    for notf in (len, "ring", R.with_softcap(R.ring_flash_attn_func, 30.0), R.llama3_flash_attn_varlen_func,
                 R.ring_flash_attn_varlen_func, R.zigzag_llama3_flash_attn_varlen_kvpacked_func):
        with pytest.raises(TypeError):
            R.apply_rotary(q, k, cos, sin, layout=notf)
    assert len(rotary_backend.rotary_calls) == n0                                      # nothing was launched
    # all nine dense functions are layouts (a group of one rank: positions 0 .. S-1)
    plain = R.apply_rotary(q, k, cos, sin)
    for kind in PREFIX.values():
        for f in _funcs(R, kind):
            got = R.apply_rotary(q, k, cos, sin, layout=f)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
            assert rotary_backend.rotary_calls[-1]["positions"] is False                # the map's numbers: no tensor was built
    # a backend without the flag
    _testing.set_backend(UspBackend(serves=("mask_shift",)))
    with pytest.raises(NotImplementedError, match="serves `rotary`"):
        R.apply_rotary(q, k, cos, sin)
    assert "apply_rotary" in dir(R) and "local_positions" in dir(R)
    assert len([n for n in dir(R) if n.endswith("_func")]) == 21                       # the two new names do not end in _func
