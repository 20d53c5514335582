"""The per-head max attention logit (ring_flash_attn.with_max_logit), no device: the C ABI of rfa_max_logit (symbols, struct
layout, every argument check with NULL tensors and their order, the workspace size), the kernel's tile arithmetic against the
brute-force mask (tests/native/maxlogit_check.cpp under ASan + UBSan), the binder's refusals, and the schedules — one function
of each of the seven families at 1, 2 and 4 ranks under gloo on the CPU test backend with `max_logit`
(tests/_maxlogit_backend.py) — against ONE single-device fp64 computation on the unsharded, planted tensors."""
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
import _bandref as BR                            # noqa: E402
import _maxlogit_backend as ML                   # noqa: E402
import _maxlogit_worker as MW                    # noqa: E402
from _blockref import visible                    # noqa: E402

OK, ERR_NULL, ERR_DTYPE, ERR_HEAD_DIM, ERR_HEADS, ERR_SHAPE, ERR_ALIGN, ERR_ARGS = 0, -1, -2, -3, -4, -5, -6, -8
CSRC = os.path.join(ROOT, "ring-flash-attention_amd", "csrc")
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------- the tile arithmetic
def test_tile_arithmetic_host_check_under_asan_and_ubsan():
    """tests/native/maxlogit_check.cpp: tile range, tile classes and row limits of every geometry of its grid against the
    brute-force mask — on the very header the kernel includes"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "maxlogit_check")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "maxlogit_check.cpp"), "-o", exe], check=True)
        res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "max-logit tile arithmetic ok" in res.stdout and "297863 geometries" in res.stdout, res.stdout


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays(built):
    from ring_flash_attn import _C

    header = open(os.path.join(ROOT, "include", "rfa.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", built.LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for sym in ("rfa_max_logit", "rfa_max_logit_workspace_bytes"):
        assert f"{sym}(const rfa_max_logit_args" in header and sym in names and sym in _C.SYMBOLS
    lib = _C.load()
    assert lib.rfa_abi_version() == 8 and lib.rfa_abi_revision() == 1 and lib.rfa_ext_args_bytes() == 40
    assert {n for n in names if n.startswith("rfa_")} == set(_C.SYMBOLS)


def test_struct_matches_the_c_layout(built):
    from ring_flash_attn import _C

    fields = [n for n, _ in _C.MaxLogitArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rfa.h"\nint main(void) {\n' \
           '  printf("%zu\\n", sizeof(rfa_max_logit_args));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(rfa_max_logit_args, {n}));\n' for n in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A = _C.MaxLogitArgs
    assert got[0] == C.sizeof(A)
    assert got[1:] == [getattr(A, n).offset for n in fields]
    assert A.struct_bytes.offset == 0 and A.reserved.offset == 4 and A().struct_bytes == C.sizeof(A)


def _args(**kw):
    from ring_flash_attn import _C

    a = _C.MaxLogitArgs()
    a.B, a.Sq, a.Sk, a.H, a.Hk, a.D, a.dtype, a.softmax_scale = 2, 300, 500, 4, 2, 64, 0, 0.125
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def test_every_argument_check_with_null_tensors_in_the_stated_order(built):
    from ring_flash_attn import _C

    lib = _C.load()
    run = lambda a: lib.rfa_max_logit(C.byref(a), None)
    assert lib.rfa_max_logit(None, None) == ERR_NULL and lib.rfa_max_logit_workspace_bytes(None) == 0
    need = 4 * 2 * 2 * 4                                             # H x B x ceil(300 / 256) floats
    assert lib.rfa_max_logit_workspace_bytes(C.byref(_args())) == need
    good = dict(workspace_bytes=need)
    # each refusal alone (every tensor pointer is NULL: nothing is read)
    alone = [
        (dict(struct_bytes=184), ERR_ARGS), (dict(struct_bytes=200), ERR_ARGS), (dict(reserved=1), ERR_ARGS),
        (dict(q_half=3), ERR_ARGS), (dict(k_half=-1), ERR_ARGS),
        (dict(dtype=2), ERR_DTYPE),
        (dict(D=0), ERR_HEAD_DIM), (dict(D=60), ERR_HEAD_DIM), (dict(D=264), ERR_HEAD_DIM),
        (dict(B=-1), ERR_SHAPE), (dict(Sq=-1), ERR_SHAPE), (dict(Sk=-1), ERR_SHAPE), (dict(total_q=-1), ERR_SHAPE),
        (dict(B=1 << 20, Sq=1 << 20, H=64), ERR_SHAPE),
        (dict(H=0), ERR_HEADS), (dict(Hk=0), ERR_HEADS), (dict(H=4, Hk=3), ERR_HEADS),
        (dict(softmax_scale=0.0), ERR_ARGS), (dict(softmax_scale=-1.0), ERR_ARGS), (dict(softmax_scale=float("inf")), ERR_ARGS),
        (dict(softmax_scale=float("nan")), ERR_ARGS),
        (dict(cu_seqlens_q=256), ERR_ARGS),                           # only one of the two
        (dict(cu_seqlens_q=256, cu_seqlens_k=256, mask_shift=1, causal=1), ERR_ARGS),
        (dict(mask_shift_lens=1 << 22, Sk=256, causal=1), ERR_ARGS), (dict(mask_shift_lens=-(1 << 22), Sk=256), ERR_ARGS),
        (dict(workspace_bytes=need - 1), ERR_ARGS),
    ]
    for kw, want in alone:
        a = _args(**dict(good, **kw))
        assert run(a) == want, (kw, run(a), want)
        if want != ERR_ARGS or "workspace_bytes" not in kw:
            assert lib.rfa_max_logit_workspace_bytes(C.byref(a)) == 0, kw          # refused arguments need no workspace
    # the order: the earlier check wins whatever comes later
    chain = [(dict(reserved=1), ERR_ARGS), (dict(dtype=5), ERR_DTYPE), (dict(D=12), ERR_HEAD_DIM), (dict(Sk=-2), ERR_SHAPE),
             (dict(Hk=3), ERR_HEADS), (dict(softmax_scale=0.0), ERR_ARGS)]
    for i, (_, want) in enumerate(chain):
        kw = dict(good)
        for later, _w in chain[i:]:
            kw.update(later)
        assert run(_args(**kw)) == want, (i, kw)
    # heads in front of the scale, the scale in front of the workspace, the workspace in front of the NULL tensors
    assert run(_args(Hk=3, softmax_scale=0.0)) == ERR_HEADS
    assert run(_args(softmax_scale=0.0, workspace_bytes=0)) == ERR_ARGS
    assert run(_args(workspace_bytes=0)) == ERR_ARGS
    assert run(_args(**good)) == ERR_NULL                            # max_logit, q, k, workspace
    assert run(_args(max_logit=256, **good)) == ERR_NULL             # q, k, workspace
    assert run(_args(max_logit=256, q=256, k=256, **good)) == ERR_NULL
    assert run(_args(max_logit=256, q=264, k=256, workspace=256, **good)) == ERR_ALIGN
    a = _args(max_logit=256, q=256, k=256, workspace=256, **good)
    a.q_st.row = 4
    assert run(a) == ERR_ALIGN


def test_workspace_size_is_a_pure_function(built):
    from ring_flash_attn import _C

    lib = _C.load()
    size = lambda **kw: lib.rfa_max_logit_workspace_bytes(C.byref(_args(**kw)))
    assert size() == size() == 4 * 2 * 2 * 4
    assert size(Sq=256) == 4 * 2 * 1 * 4 and size(Sq=257) == 4 * 2 * 2 * 4 and size(Sq=513, q_half=1) == 4 * 2 * 2 * 4
    assert size(B=0) == 0 and size(Sq=0) == 0 and size(Sk=0) == 0
    # what the band, the pointers, the scale's value or `accumulate` are does not enter
    assert size(causal=1, window=1, window_left=7, window_right=0, mask_shift=-12345, accumulate=1, q=256, workspace=256,
                softmax_scale=3.0, D=256, dtype=1) == size()


# ---------------------------------------------------------------------------------------------- the binder
@pytest.fixture()
def cpu_backend(single_rank_group):
    from ring_flash_attn import _testing
    from _sink_backend import SinkBackend

    class CpuBackend(ML.MaxLogitBackend, SinkBackend):
        pass

    be = CpuBackend(serves=("mask_shift", "mask_shift_lens", "softcap", "alibi"))
    _testing.set_backend(be)
    yield be
    _testing.set_backend(None)


def _qkv(S=48, D=32, B=2, Hq=4, Hk=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    mk = lambda s, h: torch.randn(B, s, h, D, generator=g).bfloat16()
    return mk(S, Hq), mk(S, Hk), mk(S, Hk)


def test_binder_validates_its_arguments_and_keeps_the_signatures(cpu_backend):
    import ring_flash_attn as R

    m = torch.full((4,), NEG_INF)
    names = sorted(n for n in dir(R) if n.endswith("_func"))
    assert len(names) == 21
    for n in names:
        f = getattr(R, n)
        assert R.with_max_logit(f, None) is f
        w = R.with_max_logit(f, m)
        assert w is not f and inspect.signature(w) == inspect.signature(f) and w.__name__ == f.__name__
    f = R.ring_flash_attn_func
    for bad in (lambda *a, **k: None, torch.nn.functional.scaled_dot_product_attention, R.with_max_logit(f, m)):
        with pytest.raises(TypeError):
            R.with_max_logit(bad, m)
    with pytest.raises(TypeError):
        R.with_max_logit(lambda q, k, v: q, None)                     # (None does not excuse another callable)
    # a with_ulysses result (made without a group: the marker is what the binder reads)
    marked = lambda *a, **k: None
    marked._rfa_ulysses = True
    with pytest.raises(TypeError, match="with_ulysses"):
        R.with_max_logit(marked, m)
    import torch.distributed as dist

    real = R.with_ulysses(f, dist.new_group([0]))                     # a real one, over a group of one rank
    assert getattr(real, "_rfa_ulysses", False)
    with pytest.raises(TypeError, match="with_ulysses"):
        R.with_max_logit(real, m)
    # with_softcap / with_sinks results are served
    R.with_max_logit(R.with_softcap(f, 30.0), m)
    R.with_max_logit(R.with_sinks(f, torch.zeros(4)), m)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bfloat16), torch.zeros(2, 4), torch.zeros(8)[::2],
                torch.zeros(4, requires_grad=True), [0.0] * 4, 1.0):
        with pytest.raises(ValueError):
            R.with_max_logit(f, bad)
    q, k, v = _qkv()
    with pytest.raises(ValueError, match=r"\(4,\)"):
        R.with_max_logit(f, torch.zeros(3))(q, k, v)                  # H is known at the call
    with pytest.raises(ValueError, match="softmax_scale"):
        R.with_max_logit(f, m)(q, k, v, softmax_scale=0.0)
    with pytest.raises(ValueError, match="softmax_scale"):
        R.with_max_logit(f, m)(q, k, v, 0.0, -1.0)
    assert torch.equal(m, torch.full((4,), NEG_INF)) and cpu_backend.calls == []


def test_a_backend_without_max_logit_is_refused_at_the_public_entry_and_plain_calls_never_call_it(single_rank_group):
    import ring_flash_attn as R
    from ring_flash_attn import _testing

    be = ML.NoMaxLogit(serves=("mask_shift",))
    _testing.set_backend(be)
    try:
        q, k, v = _qkv()
        m = torch.full((4,), NEG_INF)
        with pytest.raises(NotImplementedError, match="max_logit"):
            R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, causal=True)
        assert be.called == 0
        rec = ML.MaxLogitBackend(serves=("mask_shift",))
        _testing.set_backend(rec)
        R.ring_flash_attn_func(q, k, v, causal=True)                  # a call without the binder
        R.with_softcap(R.ring_flash_attn_func, 0)(q, k, v, causal=True)
        assert rec.calls == []
        R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, causal=True)
        assert rec.calls == [(0, 4)] and bool(torch.isfinite(m).all())
    finally:
        _testing.set_backend(None)


def _ref(q, k, scale=None, **kw):
    return ML.head_max(ML.row_max(q, k, q.shape[-1] ** -0.5 if scale is None else scale, **kw))


def test_single_rank_calls_composition_backward_and_checkpointing(cpu_backend):
    import ring_flash_attn as R
    from torch.utils.checkpoint import checkpoint

    q, k, v = _qkv(S=80)
    ML.plant_dense(q, k, visible(80, 80, True, (30, 0)))
    ref = _ref(q, k, causal=True, window=(30, 0)).float()
    kw = dict(causal=True, window_size=(30, 0))
    for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        m = torch.full((4,), NEG_INF)
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = R.with_max_logit(fn, m)(qq, kk, vv, **kw)
        plain = fn(q, k, v, **kw)
        assert torch.equal(out, plain) and torch.equal(m, ref), (fn.__name__, m, ref)
        keep = m.clone()
        out.sum().backward()
        assert torch.equal(m, keep)                                   # the backward never touches it
        # composition: the raw logit, whatever the call carries
        for wrapped in (R.with_softcap(fn, 5.0), R.with_sinks(fn, torch.full((4,), 0.3))):
            m2 = torch.full((4,), NEG_INF)
            R.with_max_logit(wrapped, m2)(q, k, v, **kw)
            assert torch.equal(m2, ref), (fn.__name__, m2, ref)
    # packed entry points and another scale
    m = torch.full((4,), NEG_INF)
    kv = torch.stack([k, v], dim=2)
    R.with_max_logit(R.ring_flash_attn_kvpacked_func, m)(q, kv, softmax_scale=0.5, **kw)
    assert torch.equal(m, _ref(q, k, 0.5, causal=True, window=(30, 0)).float())
    q4, k4, v4 = _qkv(S=40, Hk=4)
    m = torch.full((4,), NEG_INF)
    R.with_max_logit(R.ring_flash_attn_qkvpacked_func, m)(torch.stack([q4, k4, v4], dim=2), causal=False)
    assert torch.equal(m, _ref(q4, k4).float())
    # alibi_slopes and dropout do not enter either
    m = torch.full((4,), NEG_INF)
    R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, causal=True, alibi_slopes=torch.tensor([0.5, 0.25, 0.1, 0.05]))
    assert torch.equal(m, _ref(q, k, causal=True).float())
    m = torch.full((4,), NEG_INF)
    R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, dropout_p=0.2, causal=True)
    assert torch.equal(m, _ref(q, k, causal=True).float())
    # accumulation over calls, a tensor above every logit, and activation checkpointing (the forward runs twice)
    m = torch.full((4,), 1e3)
    R.with_max_logit(R.ring_flash_attn_func, m)(q, k, v, **kw)
    assert torch.equal(m, torch.full((4,), 1e3))
    m = torch.full((4,), NEG_INF)
    fn = R.with_max_logit(R.ring_flash_attn_func, m)
    qq = q.clone().requires_grad_(True)
    n0 = len(cpu_backend.calls)
    out = checkpoint(lambda a: fn(a, k, v, **kw), qq, use_reentrant=False)
    keep = m.clone()
    out.sum().backward()
    assert len(cpu_backend.calls) == n0 + 2 and torch.equal(m, keep) and torch.equal(m, ref)
    # an attention without rows (B = 0) sees nothing: -inf stays
    m = torch.full((4,), NEG_INF)
    R.with_max_logit(R.ring_flash_attn_func, m)(q[:0], k[:0], v[:0], causal=True)
    assert torch.equal(m, torch.full((4,), NEG_INF))


def test_under_torch_compile_the_call_runs_eagerly(cpu_backend):
    import ring_flash_attn as R

    q, k, v = _qkv()
    m = torch.full((4,), NEG_INF)
    fn = R.with_max_logit(R.ring_flash_attn_func, m)
    out = torch.compile(lambda a, b, c: fn(a, b, c, causal=True) * 2, backend="eager")(q, k, v)
    assert torch.equal(out, R.ring_flash_attn_func(q, k, v, causal=True) * 2)
    assert torch.equal(m, _ref(q, k, causal=True).float())


# ---------------------------------------------------------------------------------------------- the reference's own inputs
@pytest.mark.parametrize("D", [40, 64, 128, 256])
def test_plants_make_a_mask_error_visible_on_every_band_geometry(D):
    """reference alone: on every geometry of tests/_bandref.py the visible plant beats every other visible logit of its head
    by >= 10 where it decides the head's max, and the masked plant exceeds the true maximum by > 10 — looking one element
    too far (the band widened by one on either side) changes the result"""
    g = torch.Generator().manual_seed(D)
    seen = 0
    for geo in BR.GEOMETRIES:
        lq, lk = (geo.lq, geo.lk) if geo.lk <= 1000 else (geo.lq, 1024)
        shift = geo.off - (lk - lq)
        vis = visible(lq, lk, geo.causal, geo.window, shift)
        q = torch.randn(1, lq, 2, D, generator=g)
        k = torch.randn(1, lk, 1, D, generator=g)
        done = ML.plant_dense(q, k, vis, variants=(ML.VARIANTS[seen % 4],))
        q, k = q.bfloat16(), k.bfloat16()
        scale = D ** -0.5
        ref = ML.head_max(ML.row_max(q, k, scale, causal=geo.causal, window=geo.window, shift=shift))
        (_, _, v, m), = done
        if v is None:
            assert bool(torch.isinf(ref).all())
            continue
        seen += 1
        s = ML._seq_scores(q[0], k[0], scale)
        planted = s[:, v[0], v[1]]
        assert bool((planted > 256 * scale * 0.98).all())
        if m is not None:
            leak = s[:, m[0], m[1]]
            assert not bool(vis[m[0], m[1]]) and bool((leak > ref + 10).all()), (geo.name, leak, ref)
            # one element too far on the side the masked plant sits on
            wl, wr = geo.window
            wr = 0 if geo.causal else wr
            wide = visible(lq, lk, False, (wl + 1 if wl >= 0 else -1, wr + 1 if wr >= 0 else -1), shift)
            assert bool(wide[m[0], m[1]]), geo.name
    assert seen >= len(BR.GEOMETRIES) - 4


def test_all_negative_case_reference():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, 100, 2, 72, generator=g).abs().bfloat16()
    k = (-torch.randn(1, 77, 1, 72, generator=g).abs()).bfloat16()
    ref = _ref(q, k)
    assert bool((ref < -1.0).all()) and bool((ref > -6.0).all()), ref


# ---------------------------------------------------------------------------------------------- the schedules
def _cases(W):
    S = 32
    lens = [8 * W, 16 * W, 24 * W][:3]
    out = []
    for kind, extra in (("ring", {}), ("zigzag", dict(form="ring")), ("zigzag", dict(form="gather")), ("stripe", {}),
                        ("ring_varlen", dict(lens=lens)), ("zigzag_varlen", dict(lens=lens)), ("llama3", dict(stride=1)),
                        ("zigzag_llama3", {})):
        out.append(dict(kind=kind, W=W, S=S, causal=True, **extra))
        if kind in ("ring", "ring_varlen", "llama3"):
            out.append(dict(kind=kind, W=W, S=S, causal=False, **extra))
        if kind != "zigzag_llama3" and extra.get("form") != "gather":
            out.append(dict(kind=kind, W=W, S=S, causal=True, window=(S + 5, 0), **extra))
    # llama3 in several head groups: a wrong head offset lands in the wrong slot
    out.append(dict(kind="llama3", W=W, S=S, causal=True, stride=1, groups=2))
    out.append(dict(kind="llama3", W=W, S=S, causal=True, stride=1, groups=2, window=(20, 0)))
    out.append(dict(kind="ring", W=W, S=S, causal=True, wrap="softcap"))
    out.append(dict(kind="zigzag", W=W, S=S, causal=True, wrap="sinks", form="ring"))
    out.append(dict(kind="llama3", W=W, S=S, causal=True, wrap="sinks", stride=1))
    return out


@pytest.mark.parametrize("W", [1, 2, 4])
def test_every_family_matches_one_single_device_computation(W):
    cases = _cases(W)
    # composition gives the numbers of the unwrapped case: same inputs, same reference
    errs, notes = MW.run_world(W, cases, False, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
