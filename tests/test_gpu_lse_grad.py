"""A differentiable lse (ring_flash_attn.with_lse_grad) and the pairwise merge (ring_flash_attn.merge_attn) on the HIP kernels:
the delta-preprocess variant bit for bit against `plain delta - dlse`; the bound public call on one rank through every consumer
of delta (the 128-key dK/dV kernel with the 7-GEMM dQ, the dS hand-off, the 256-key and the balanced dK/dV forms, head dims 160
and 256, a window, a soft cap, dropout) against fp64 autograd of <out, dO> + <lse, dL> (tests/_lsegrad_worker.reference); the two
merge kernels against fp64 autograd of the torch expression, with empty rows of both spellings; and the composition of a
replicated prefix with a zigzag-sharded sequence at W = 2 and 4, the ranks sharing the GPU."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from conftest import free_port                   # noqa: E402
import _bandref as BR                            # noqa: E402
import _lsegrad_worker as LW                     # noqa: E402
import _tol                                      # noqa: E402

pytestmark = pytest.mark.gpu

BF, FP16 = torch.bfloat16, torch.float16


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn._testing import set_backend
    from ring_flash_attn.backend import get_backend

    set_backend(None)
    return get_backend()


# ---------------------------------------------------------------------------------------------- the preprocess variant
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("D", [8, 64, 128, 136, 256])
def test_preprocess_with_dlse_is_the_plain_delta_minus_dlse_bit_for_bit(D, packed):
    """H = 3 and 33 rows: a workgroup's 16 (row, head) items straddle rows and the last block is partial; above 128 columns
    the kernel loop takes a second pass.  The accumulator is the plain instance's and one fp32 subtraction is correctly
    rounded, so the result IS torch's fp32 `plain_delta - dlse`.  dlse has strides of its own (a view of a wider tensor).
    Packed: an empty sequence in the batch, and both q_half selectors (rows outside the selected half are not written)."""
    from ring_flash_attn import _C

    be, dev = _be(), _dev()
    H, gen = 3, torch.Generator().manual_seed(300 + D)
    for dtype in (BF, FP16):
        if not packed:
            B, S = 2, 33
            do, o = (torch.randn(B, S, H, D, generator=gen).to(dtype).to(dev) for _ in range(2))
            dlse = torch.randn(B, H + 1, S + 7, generator=gen).to(dev)[:, :H, :S]
            plain, got = torch.full((B, H, S), 7.0, device=dev), torch.full((B, H, S), 7.0, device=dev)
            be.bwd_preprocess(do, o, plain)
            be.bwd_preprocess(do, o, got, dlse=dlse)
            assert bool((plain != 7.0).all())
            assert torch.equal(got, plain - dlse), f"D={D} {dtype}: max diff {(got - (plain - dlse)).abs().max().item():.3e}"
            continue
        lens = [33, 0, 20]
        T, cu = sum(lens), torch.tensor([0, 33, 33, 53], dtype=torch.int32, device=dev)
        do, o = (torch.randn(T, H, D, generator=gen).to(dtype).to(dev) for _ in range(2))
        dlse = torch.randn(H + 1, T + 7, generator=gen).to(dev)[:H, :T]
        for half, rows in ((_C.HALF_FULL, 53), (_C.HALF_FRONT, 16 + 10), (_C.HALF_BACK, 17 + 10)):
            plain, got = torch.full((H, T), 7.0, device=dev), torch.full((H, T), 7.0, device=dev)
            be.bwd_preprocess(do, o, plain, cu_seqlens_q=cu, max_seqlen_q=33, q_half=half)
            be.bwd_preprocess(do, o, got, cu_seqlens_q=cu, max_seqlen_q=33, q_half=half, dlse=dlse)
            written = plain != 7.0
            assert int(written.sum()) == H * rows, (half, int(written.sum()))
            assert torch.equal(got, torch.where(written, plain - dlse, plain)), f"D={D} {dtype} q_half={half}"


# ---------------------------------------------------------------------------------------------- end to end on one rank
S_E2E = 160                                      # unaligned: no multiple of a 32- / 64- / 128-row tile
# name -> (D, S, causal, window, softcap, dropout_p, env, the (dK/dV form, five_gemm) rfa_bwd_plan must report or None)
FORMS = {
    "dkdv128-7gemm": (128, S_E2E, True, (-1, -1), 0.0, 0.0, dict(RFA_DKDV_WIDE="0", RFA_BWD_DS_SPILL="0"), (BR.DKDV_128, 0)),
    "dkdv128-7gemm-full": (128, S_E2E, False, (-1, -1), 0.0, 0.0, dict(RFA_DKDV_WIDE="0", RFA_BWD_DS_SPILL="0"), (BR.DKDV_128, 0)),
    "5gemm": (128, S_E2E, True, (-1, -1), 0.0, 0.0, dict(RFA_BWD_DS_SPILL="1"), (None, 1)),
    "5gemm-full": (128, S_E2E, False, (-1, -1), 0.0, 0.0, dict(RFA_BWD_DS_SPILL="1"), (None, 1)),
    "dkdv256": (128, S_E2E, True, (-1, -1), 0.0, 0.0, dict(RFA_DKDV_WIDE="1", RFA_DKDV_NSPLIT="2", RFA_BWD_DS_SPILL="0"), (BR.DKDV_256, 0)),
    # (the balanced schedule exists for dense causal blocks of a multiple of 512 rows only: its smallest shape)
    "balanced": (128, 512, True, (-1, -1), 0.0, 0.0, dict(RFA_DKDV_WIDE="2"), (BR.DKDV_BAL, None)),
    "d160": (160, S_E2E, True, (-1, -1), 0.0, 0.0, dict(), None),            # the fused big kernel + dq_big
    "d256": (256, S_E2E, True, (-1, -1), 0.0, 0.0, dict(RFA_BWD_DS_SPILL="1"), (None, 1)),   # two launches + rfa_dqs
    "window": (128, S_E2E, True, (50, 0), 0.0, 0.0, dict(), (BR.DKDV_128, 0)),
    "softcap": (128, S_E2E, True, (-1, -1), 20.0, 0.0, dict(), None),
    "dropout": (128, S_E2E, True, (-1, -1), 0.0, 0.2, dict(), None),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_bound_call_on_one_rank_through_every_consumer_of_delta(monkeypatch, single_rank_group, form):
    """S = 160, B 2, H 4 / Hk 2, loss <out, dO> + <lse, dL>: out, lse, dq, dk, dv against fp64 autograd (kinds out, lse, grad).
    The form is forced by the switches of tests/test_gpu_band_forms.py and asserted on the host (rfa_bwd_plan) first.  Dropout:
    the reference applies the kernels' keep mask (tests/_blockref.keep_mask, the seed drawn as the call draws it) to P V and dP
    and leaves lse the undropped softmax's."""
    import ring_flash_attn as R
    from ring_flash_attn import _C

    D, S, causal, window, cap, p, env, plan = FORMS[form]
    be, dev = _be(), _dev()
    if plan is not None:
        g = types.SimpleNamespace(B=LW.B, lq=S, lk=S, causal=causal, window=window, shift=0)
        f, _, five = BR.bwd_plan(be.lib, BR.bwd_args(_C, g, LW.H, LW.HK, D, env))
        assert (plan[0] is None or f == plan[0]) and (plan[1] is None or five == plan[1]), (form, f, five)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    c = dict(kind="ring", W=1, S=S, D=D, causal=causal, window=window, softcap=cap)
    if p:
        torch.manual_seed(4242)
        c["dropout"] = (p, int(torch.randint(0, 2 ** 62, (1,)).item()))
        torch.manual_seed(4242)                                           # (the call draws the same seed)
    dL = LW.draw_dl(c)
    ref = LW.reference(c, dL)
    q, k, v, do = (t.to(dev) for t in LW.SW.inputs(c))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    try:
        out, lse, _ = LW.bind(R, c)(q, k, v, causal=causal, window_size=window, dropout_p=p, return_attn_probs=True)
        torch.autograd.backward([out, lse], [do, dL.float().to(dev)])
        bad = []
        for nm, got, want, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), ref,
                                     ("out", "lse", "grad", "grad", "grad")):
            m = _tol.metrics(got, want)
            print(f"{form}.{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
            bad += _tol.failures(f"{form}.{nm}", got, want, kd)
        assert not bad, "; ".join(bad)
    finally:
        be.release_scratch()


# ---------------------------------------------------------------------------------------------- the merge kernels
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("dtype", [BF, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [8, 128, 136, 256])
def test_merge_kernels_against_fp64_autograd(single_rank_group, D, dtype, packed):
    """B 2, 33 rows, H 3: out by the `out` kind, lse by `lse`, dout_a / dout_b by `grad`, dlse_a / dlse_b by the lse kind's
    relative bounds; the empty-row cases of the CPU file (an empty side's out holds NaN); two runs give the same bits"""
    import ring_flash_attn as R

    _be()
    dev = _dev()
    ins = LW.merge_inputs(2, 33, 3, D, dtype, packed)
    on_dev = tuple(t.to(dev) for t in ins)
    got = [t.cpu() for t in LW.merge_run(R.merge_attn, on_dev)]
    errs, worst = LW.merge_failures(f"merge.D{D}", got, LW.merge_reference(*ins))
    print(f"merge.D{D}.{dtype}.{'packed' if packed else 'dense'}: " + ", ".join(f"{k_} {v_:.3e}" for k_, v_ in worst.items()))
    errs += LW.empty_row_failures(f"merge.D{D}", got, ins, packed, 2, 33)
    assert not errs, "\n".join(errs)
    for x, y in zip(got, LW.merge_run(R.merge_attn, on_dev)):
        assert torch.equal(x, y.cpu())
    # strided inputs (the halves of a wider tensor) are taken as they are
    wide = torch.cat([on_dev[0], on_dev[2]], dim=-1)
    out2, lse2 = R.merge_attn(wide[..., :D], on_dev[1], wide[..., D:], on_dev[3])
    assert torch.equal(out2.cpu(), got[0]) and torch.equal(lse2.cpu(), got[1])


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("W", [2, 4])
def test_composition_of_a_replicated_prefix_with_a_sharded_sequence(W):
    """the composition test of tests/test_lse_grad_cpu.py on the kernels: S = 128 rows per rank, D = 128, the ranks sharing
    the GPU"""
    errs, notes = LW.run_world(W, [dict(kind="zigzag", W=W, S=128, D=128, causal=True, compose=True)], True, free_port())
    print("\n".join(notes))
    assert not errs, "\n".join(errs)
