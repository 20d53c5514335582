"""A differentiable lse (ring_flash_attn.with_lse_grad) and the pairwise merge (ring_flash_attn.merge_attn) without a GPU: the
three new C-ABI entry points' structs and argument checks, the binders' refusals, every schedule family under gloo on the CPU
test backend (tests/_lsegrad_backend.py) against ONE single-device fp64 autograd computation (tests/_lsegrad_worker.py), the
merge against fp64 autograd of the torch expression with empty rows of both spellings, and the composition of a replicated
prefix with a zigzag-sharded sequence."""
import ctypes as C
import inspect
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import free_port                   # noqa: E402
import _lsegrad_worker as LW                     # noqa: E402
import _tol                                      # noqa: E402


# ---------------------------------------------------------------------------------------------- C ABI
def test_structs_match_the_c_layout_and_the_abi_numbers_stay(built):
    from ring_flash_attn import _C

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rfa.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(rfa_bwd_preprocess_lse_args), sizeof(rfa_merge_pair_args),
         sizeof(rfa_merge_pair_bwd_args), sizeof(rfa_bwd_preprocess_args), sizeof(rfa_ext_args));
  printf("%zu %zu %zu\n", offsetof(rfa_bwd_preprocess_lse_args, dlse), offsetof(rfa_bwd_preprocess_lse_args, cu_seqlens_q),
         offsetof(rfa_bwd_preprocess_lse_args, reserved));
  printf("%zu %zu %zu\n", offsetof(rfa_merge_pair_args, lse_b_head), offsetof(rfa_merge_pair_args, lse),
         offsetof(rfa_merge_pair_args, reserved));
  printf("%zu %zu %zu %zu\n", offsetof(rfa_merge_pair_bwd_args, dlse), offsetof(rfa_merge_pair_bwd_args, lse_a),
         offsetof(rfa_merge_pair_bwd_args, dlse_b_head), offsetof(rfa_merge_pair_bwd_args, reserved));
  printf("%d %d\n", RFA_ABI_VERSION, RFA_ABI_REVISION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    L, P, PB = _C.BwdPreLseArgs, _C.MergePairArgs, _C.MergePairBwdArgs
    assert out[:5] == [C.sizeof(L), C.sizeof(P), C.sizeof(PB), C.sizeof(_C.BwdPreArgs), 40]
    assert out[5:8] == [L.dlse.offset, L.cu_seqlens_q.offset, L.reserved.offset]
    assert out[8:11] == [P.lse_b_head.offset, P.lse.offset, P.reserved.offset]
    assert out[11:15] == [PB.dlse.offset, PB.lse_a.offset, PB.dlse_b_head.offset, PB.reserved.offset]
    assert out[15:] == [8, 1]
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    for name in ("rfa_bwd_preprocess_lse", "rfa_merge_pair", "rfa_merge_pair_bwd"):
        assert name in _C.SYMBOLS and hasattr(lib, name)


_ST = (16 * 4 * 64, 4 * 64, 64)
_PTR = 4096            # never dereferenced: every case below is refused or launches nothing


def _pre_args(**kw):
    from ring_flash_attn import _C

    a = _C.BwdPreLseArgs()
    a.B, a.Sq, a.H, a.D, a.dtype = 2, 16, 4, 64, 0
    a.dout_st, a.out_st = _C.Strides(*_ST), _C.Strides(*_ST)
    a.delta_batch, a.delta_head, a.dlse_batch, a.dlse_head = 64, 16, 64, 16
    a.dout = a.out = a.delta = a.dlse = _PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pair_args(**kw):
    from ring_flash_attn import _C

    a = _C.MergePairArgs()
    a.B, a.S, a.H, a.D, a.dtype = 2, 16, 4, 64, 0
    a.out_a_st, a.out_b_st, a.out_st = (_C.Strides(*_ST) for _ in range(3))
    for n in ("lse_a", "lse_b", "lse"):
        setattr(a, n + "_batch", 64)
        setattr(a, n + "_head", 16)
    a.out_a = a.out_b = a.lse_a = a.lse_b = a.out = a.lse = _PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pair_bwd_args(**kw):
    from ring_flash_attn import _C

    a = _C.MergePairBwdArgs()
    a.B, a.S, a.H, a.D, a.dtype = 2, 16, 4, 64, 0
    for n in ("dout", "out_a", "out_b", "dout_a", "dout_b"):
        setattr(a, n + "_st", _C.Strides(*_ST))
        setattr(a, n, _PTR)
    for n in ("dlse", "lse_a", "lse_b", "dlse_a", "dlse_b"):
        setattr(a, n + "_batch", 64)
        setattr(a, n + "_head", 16)
        setattr(a, n, _PTR)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_without_a_device(built):
    from ring_flash_attn import _C

    lib = _C.load()
    NULL, DTYPE, HEAD_DIM, HEADS, SHAPE, ALIGN, ARGS = -1, -2, -3, -4, -5, -6, -8
    odd = _C.Strides(16 * 4 * 64, 4 * 64 + 4, 64)
    for fn, mk, rows, tensors, optional, io, strided in (
            (lib.rfa_bwd_preprocess_lse, _pre_args, "Sq", ("dout", "out", "delta"), "dlse", ("dout", "out"), ("dout_st", "out_st")),
            (lib.rfa_merge_pair, _pair_args, "S", ("out_a", "out_b", "lse_a", "lse_b", "out", "lse"), None,
             ("out_a", "out_b", "out"), ("out_a_st", "out_b_st", "out_st")),
            (lib.rfa_merge_pair_bwd, _pair_bwd_args, "S",
             ("dout", "out_a", "out_b", "lse_a", "lse_b", "dout_a", "dout_b", "dlse_a", "dlse_b"), "dlse",
             ("dout", "out_a", "out_b", "dout_a", "dout_b"), ("dout_st", "out_a_st", "out_b_st", "dout_a_st", "dout_b_st"))):
        assert fn(None, None) == NULL
        for t in tensors:
            assert fn(C.byref(mk(**{t: None})), None) == NULL, t
        for D in (0, 4, 12, 264, -8):
            assert fn(C.byref(mk(D=D)), None) == HEAD_DIM, D
        assert fn(C.byref(mk(dtype=2)), None) == DTYPE and fn(C.byref(mk(dtype=-1)), None) == DTYPE
        assert fn(C.byref(mk(H=0)), None) == HEADS
        assert fn(C.byref(mk(**{rows: -1})), None) == SHAPE and fn(C.byref(mk(B=-1)), None) == SHAPE
        assert fn(C.byref(mk(reserved=1)), None) == ARGS
        for t in io:
            assert fn(C.byref(mk(**{t: _PTR + 8})), None) == ALIGN, t
        for st in strided:
            assert fn(C.byref(mk(**{st: odd})), None) == ALIGN, st
        # the order: dtype, head dim, heads, shape, reserved, then the pointers, then their alignment
        assert fn(C.byref(mk(dtype=5, D=12, **{tensors[0]: None})), None) == DTYPE
        assert fn(C.byref(mk(D=12, H=0, **{tensors[0]: None})), None) == HEAD_DIM
        assert fn(C.byref(mk(H=0, B=-1)), None) == HEADS
        assert fn(C.byref(mk(**{rows: -1, "reserved": 1})), None) == SHAPE
        assert fn(C.byref(mk(reserved=1, **{tensors[0]: None})), None) == ARGS
        assert fn(C.byref(mk(**{tensors[0]: None, io[1]: _PTR + 8})), None) == NULL
        # zero rows: RFA_OK with nothing launched, whatever the tensors
        for kw in ({"B": 0}, {rows: 0}):
            assert fn(C.byref(mk(**{tensors[0]: None}, **kw)), None) == 0
        if optional is not None:                                        # (a NULL dlse is no error: refused for the OTHER pointer)
            assert fn(C.byref(mk(**{optional: None, tensors[0]: None})), None) == NULL
    # the merge entries also bound B and H (grid dimensions); the preprocess variant also refuses a half selector it does not know
    for fn, mk in ((lib.rfa_merge_pair, _pair_args), (lib.rfa_merge_pair_bwd, _pair_bwd_args)):
        assert fn(C.byref(mk(H=70000)), None) == SHAPE and fn(C.byref(mk(B=70000)), None) == SHAPE
    assert lib.rfa_bwd_preprocess_lse(C.byref(_pre_args(q_half=3)), None) == ARGS
    assert lib.rfa_bwd_preprocess_lse(C.byref(_pre_args(q_half=-1)), None) == ARGS


# ---------------------------------------------------------------------------------------------- the binders
@pytest.fixture
def cpu_backend(single_rank_group):
    from ring_flash_attn import _testing
    from _lsegrad_backend import LseGradBackend

    _testing.set_backend(LseGradBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
    yield
    _testing.set_backend(None)


B, S, H, HK, D = 2, 48, 4, 2, 32


def _qkv(seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).bfloat16()
    return mk(H), mk(HK), mk(HK), mk(H)


def test_with_lse_grad_validates_its_argument_and_keeps_the_signatures(cpu_backend):
    import ring_flash_attn as R
    from ring_flash_attn import _testing
    from _ref_backend import RefBackend
    from _sink_backend import SinkBackend

    assert "with_lse_grad" in dir(R) and "merge_attn" in dir(R) and not R.merge_attn.__name__.endswith("_func")
    funcs = [getattr(R, n) for n in dir(R) if n.endswith("_func")]
    assert len(funcs) == 21
    before = {f.__name__: str(inspect.signature(f)) for f in funcs}
    for f in funcs:
        g = R.with_lse_grad(f)
        assert g is not f and inspect.signature(g) == inspect.signature(f) and g.__name__ == f.__name__
        R.with_lse_grad(R.with_softcap(f, 30.0))                          # a with_softcap result is served
    assert {f.__name__: str(inspect.signature(f)) for f in funcs} == before
    bound = R.with_lse_grad(R.ring_flash_attn_func)
    m = torch.full((H,), float("-inf"))
    for notf in (len, lambda q, k, v: q, R.llama3_flash_attn_prepare_cu_seqlens, R.merge_attn, bound,
                 R.with_sinks(R.ring_flash_attn_func, torch.zeros(H)), R.with_max_logit(R.ring_flash_attn_func, m),
                 R.with_ulysses(R.ring_flash_attn_func, torch.distributed.group.WORLD)):
        with pytest.raises(TypeError):
            R.with_lse_grad(notf)
    # the other binders refuse a with_lse_grad result, through the checks they always had
    for binder in (lambda f: R.with_softcap(f, 30.0), lambda f: R.with_sinks(f, torch.zeros(H)),
                   lambda f: R.with_max_logit(f, m), lambda f: R.with_ulysses(f, torch.distributed.group.WORLD)):
        with pytest.raises(TypeError):
            binder(bound)
        with pytest.raises(TypeError):
            binder(R.with_lse_grad(R.with_softcap(R.ring_flash_attn_func, 30.0)))
    # a backend that does not serve it: refused at the public entry of every family; the same backend serves the plain call
    q, k, v, _ = _qkv()
    cu = torch.tensor([0, 20, S], dtype=torch.int32)
    _testing.set_backend(SinkBackend(serves=("mask_shift",)))
    for fn, args in ((R.ring_flash_attn_func, (q, k, v)), (R.ring_flash_attn_qkvpacked_func, (torch.stack([q, q, q], dim=2),)),
                     (R.zigzag_llama3_flash_attn_varlen_func, (q[0], k[0], v[0], cu)),
                     (R.llama3_flash_attn_varlen_func, (q[0], k[0], v[0], cu, cu, 28, 28, 1, slice(0, S)))):
        with pytest.raises(NotImplementedError, match="lse"):
            R.with_lse_grad(fn)(*args, causal=True)
    R.ring_flash_attn_func(q, k, v, causal=True)
    out, lse, _ = R.ring_flash_attn_func(q, k, v, causal=True, return_attn_probs=True)
    with pytest.raises(NotImplementedError, match="merge_pair"):
        R.merge_attn(out, lse, out, lse)
    _testing.set_backend(RefBackend(serves=("mask_shift",)))
    with pytest.raises(NotImplementedError, match="lse"):
        R.with_lse_grad(R.ring_flash_attn_func)(q, k, v, causal=True)


def test_merge_attn_validates_its_arguments(cpu_backend):
    import ring_flash_attn as R

    o = torch.zeros(B, S, H, D, dtype=torch.bfloat16)
    l = torch.zeros(B, H, S)
    R.merge_attn(o, l, o, l)
    R.merge_attn(o[0], l[0], o[0], l[0])                                  # packed: (T, H, D) with (H, T)
    for bad in ((o, l, o[:, :-1], l), (o, l, o.half(), l), (o, l.double(), o, l), (o, l, o, l.transpose(1, 2)),
                (o, l[0], o, l), (o[0], l, o[0], l), (o, l, o, l[:, :, :-1]), (o, l, o, l.to("meta")), (o.to("meta"), l, o, l),
                (o[0, 0], l[0, 0], o[0, 0], l[0, 0]), (o, None, o, l)):
        with pytest.raises(ValueError, match="merge_attn"):
            R.merge_attn(*bad)


def _bound_run(fn, tensors, grads, **kw):
    """[out, lse, the inputs' gradients] of one call with the output gradients `grads` = (dout or None, dlse or None)"""
    ins = [t.clone().requires_grad_(True) for t in tensors]
    out, lse, _ = fn(*ins, return_attn_probs=True, **kw)
    pairs = [(o, g) for o, g in zip((out, lse), grads) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return [out.detach(), lse.detach()] + [t.grad for t in ins]


def test_none_gradients_packed_forms_and_checkpointing(cpu_backend):
    """an unused lse leaves the plain call bit for bit; a loss on lse alone delivers an undefined dout; the packed forms land
    the same gradients in one buffer; a checkpointed re-run binds again"""
    import ring_flash_attn as R
    from torch.utils.checkpoint import checkpoint

    q, k, v, do = _qkv()
    g = torch.Generator().manual_seed(11)
    dl = torch.randn(B, H, S, generator=g)
    plain, bound = R.ring_flash_attn_func, R.with_lse_grad(R.ring_flash_attn_func)
    a, b = _bound_run(bound, (q, k, v), (do, None), causal=True), _bound_run(plain, (q, k, v), (do, None), causal=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the plain call drops a gradient of lse, silently (the behaviour this feature leaves alone)
    c = _bound_run(plain, (q, k, v), (do, dl), causal=True)
    for x, y in zip(b, c):
        assert torch.equal(x, y)
    full = _bound_run(bound, (q, k, v), (do, dl), causal=True)
    assert not torch.equal(full[2], b[2]) and not torch.equal(full[3], b[3]) and torch.equal(full[4], b[4])   # dv: no lse in it
    only = _bound_run(bound, (q, k, v), (None, dl), causal=True)
    assert torch.equal(only[4], torch.zeros_like(only[4]))
    # linear in the output gradients, up to the roundings of the io dtype
    for i in (2, 3):
        _tol.compare(f"lse-only + out-only [{i}]", only[i].float() + b[i].float(), full[i].double(), "grad")
    # a non-contiguous, non-fp32 gradient of lse is taken as fp32 in lse's layout
    odd = _bound_run(bound, (q, k, v), (do, dl.double().transpose(1, 2).contiguous().transpose(1, 2)), causal=True)
    for x, y in zip(full, odd):
        assert torch.equal(x, y)
    kv, qkv = torch.stack([k, v], dim=2), torch.stack([q, k.repeat_interleave(2, dim=2), v.repeat_interleave(2, dim=2)], dim=2)
    g_kv = _bound_run(R.with_lse_grad(R.ring_flash_attn_kvpacked_func), (q, kv), (do, dl), causal=True)
    assert torch.equal(g_kv[2], full[2]) and torch.equal(g_kv[3][:, :, 0], full[3]) and torch.equal(g_kv[3][:, :, 1], full[4])
    g3 = _bound_run(bound, (qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]), (do, dl), causal=True)
    g_qkv = _bound_run(R.with_lse_grad(R.ring_flash_attn_qkvpacked_func), (qkv,), (do, dl), causal=True)
    for i in range(3):
        assert torch.equal(g_qkv[2][:, :, i], g3[2 + i])
    ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out, lse, _ = checkpoint(lambda *t: bound(*t, causal=True, return_attn_probs=True), *ins, use_reentrant=False)
    torch.autograd.backward([out, lse], [do, dl])
    for x, y in zip(full[2:], (t.grad for t in ins)):
        assert torch.equal(x, y)
    # without return_attn_probs the bound call is the plain call
    o1 = bound(q.clone().requires_grad_(True), k, v, causal=True)
    o1.backward(do)
    assert torch.equal(o1, b[0])


def test_under_torch_compile_the_bound_call_and_the_merge_run_eagerly(cpu_backend):
    """a compiled caller graph-breaks around the bound call and around merge_attn: the eager results and gradients, bit for
    bit — the gradient of lse included (the registered operators, which the plain call lowers to, would drop it)"""
    import ring_flash_attn as R

    q, k, v, do = _qkv()
    dl = torch.randn(B, H, S, generator=torch.Generator().manual_seed(11))
    bound = R.with_lse_grad(R.ring_flash_attn_func)

    def step(a, b, c):
        out, lse, _ = bound(a, b, c, causal=True, return_attn_probs=True)
        return R.merge_attn(out, lse, out, lse * 0.5)

    res = []
    for fn in (step, torch.compile(step, backend="eager")):
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, lse = fn(*ins)
        torch.autograd.backward([out, lse], [do, dl])
        res.append([out.detach(), lse.detach()] + [t.grad for t in ins])
    for x, y in zip(*res):
        assert torch.equal(x, y)
    plain = _bound_run(R.ring_flash_attn_func, (q, k, v), (do, None), causal=True)
    assert not torch.equal(res[0][2], plain[2])                        # (lse's gradient reached dq)


# ---------------------------------------------------------------------------------------------- schedules under gloo
def _cases(W):
    lens = [16 * W, 12 * W, 4 * W]                     # 32 packed rows per rank; local lengths 16, 12, 4
    base = dict(W=W, S=32, D=16, causal=True)
    c = [dict(base, kind=kd, **extra) for kd, extra in (
        ("ring", {}), ("zigzag", {}), ("stripe", {}),
        # packed and windowed: at W = 4 a block call of a later ring step holds a wholly lit sequence (local length 4, one
        # step back), cut ones, and a wholly dark one (local length 16, two steps back: every distance is above 10)
        ("ring_varlen", dict(lens=lens, window=(10, 0))), ("zigzag_varlen", dict(lens=lens)),
        ("llama3", {}), ("zigzag_llama3", {}))]
    c.append(dict(base, kind="ring", window=(20, 0)))                          # a window below the per-rank length
    c.append(dict(base, kind="zigzag", softcap=20.0))                          # with_lse_grad of a with_softcap result
    c.append(dict(base, kind="ring", lse_only=True))                           # the loss touches lse alone
    c += [dict(base, kind=kd, unused=True, **extra) for kd, extra in (
        ("zigzag", {}), ("ring_varlen", dict(lens=lens)), ("llama3", {}), ("zigzag_llama3", {}))]
    return c


@pytest.mark.parametrize("W", [1, 2, 4])
def test_schedules_carry_the_gradient_of_lse(W):
    """S = 32 rows per rank, H 4 / Hk 2, D 16, causal, loss <out, dO> + <lse, dL>, dL ~ N(0, 1): every family's dq, dk, dv
    against one fp64 autograd computation over the unsharded tensors — and off the dL = 0 gradients by more than the tolerance;
    with dL unused the bound call is the plain call bit for bit.  Fails on a backward that drops the gradient of lse."""
    errs, notes = LW.run_world(W, _cases(W), False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)


def test_composition_of_a_replicated_prefix_with_a_sharded_sequence():
    """M = 5 replicated prefix keys (all visible) through a bound call on a one-rank group, the zigzag-sharded sequence through
    a bound call at W = 2, merged with merge_attn: out, lse, dq, the sequence's dk / dv and the prefix's dk / dv summed over
    the ranks against ONE fp64 softmax over [prefix; sequence].  Fails on a backward that drops the gradient of lse."""
    errs, notes = LW.run_world(2, [dict(kind="zigzag", W=2, S=32, D=16, causal=True, compose=True)], False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------- merge_attn
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_merge_attn_against_fp64_autograd_with_empty_rows(cpu_backend, dtype, packed):
    """forward and backward against fp64 autograd of the torch expression; rows with one side empty (+inf and -inf) and with
    both; no NaN although the empty sides' out holds NaN; exact zeros to empty sides; undefined gradients; two runs, same bits"""
    import ring_flash_attn as R

    ins = LW.merge_inputs(2, 9, 3, 24, dtype, packed)
    got, ref = LW.merge_run(R.merge_attn, ins), LW.merge_reference(*ins)
    errs, worst = LW.merge_failures("merge", got, ref)
    print(worst)
    assert not errs, "\n".join(errs)
    errs = LW.empty_row_failures("merge", got, ins, packed, 2, 9)
    assert not errs, "\n".join(errs)
    # undefined gradients: a loss on out alone, and on lse alone
    leaves = [t.clone().requires_grad_(True) for t in ins[:4]]
    R.merge_attn(*leaves)[0].backward(ins[4])
    ref_o = LW.merge_reference(*ins[:5], torch.zeros_like(ins[5]))
    for i, nm in enumerate(("dout_a", "dlse_a", "dout_b", "dlse_b")):
        check = LW.lse_relative_failures if nm.startswith("dlse") else (lambda *a: _tol.failures(*a, "grad"))
        assert not check(f"out-only.{nm}", leaves[i].grad, ref_o[2 + i])
    leaves = [t.clone().requires_grad_(True) for t in ins[:4]]
    R.merge_attn(*leaves)[1].backward(ins[5])
    ref_l = LW.merge_reference(*ins[:4], torch.zeros_like(ins[4]), ins[5])
    assert torch.equal(leaves[0].grad, torch.zeros_like(leaves[0].grad)) and torch.equal(leaves[2].grad, torch.zeros_like(leaves[2].grad))
    assert not LW.lse_relative_failures("lse-only.dlse_a", leaves[1].grad, ref_l[3])
    assert not LW.lse_relative_failures("lse-only.dlse_b", leaves[3].grad, ref_l[5])
    # a frozen input gets no gradient
    frozen = [ins[0].clone().requires_grad_(True), ins[1], ins[2], ins[3]]
    out, lse = R.merge_attn(*frozen)
    torch.autograd.backward([out, lse], [ins[4], ins[5]])
    assert torch.equal(frozen[0].grad, got[2]) and frozen[1].grad is None
    for x, y in zip(got, LW.merge_run(R.merge_attn, ins)):
        assert torch.equal(x, y)
