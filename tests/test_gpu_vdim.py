"""A value head dim of its own (csrc/rfa_vdim.hip: QK head dims 136 … 192, V head dims 8 … 128) on the GPU (`-m gpu`).

Every case goes through HipBackend (rfa_fwd_vd / rfa_bwd_vd) and is compared with the fp64 block reference (tests/_blockref.py,
gradients by autograd) under the `out` / `lse` / `grad` kinds of tests/_tol.py, fp16 like bf16 as the head-dim-256 tests do.
Shapes are the smallest at which these kernels can go wrong: ragged tails, more than one 128-key block, more 32-row Q tiles
than LDS stages, the group sum in registers, padded quarters, rows without a key.  Only the first test is in the core tier."""
import pytest
import torch

from test_gpu_kernels import BF, _check, _dev, _grads_ok

FP = torch.float16
extended = pytest.mark.extended
pytestmark = [pytest.mark.gpu]


def _be():
    from ring_flash_attn.backend import get_backend
    from ring_flash_attn._testing import set_backend

    set_backend(None)
    return get_backend(), _dev()


def _inputs(D, Dv, B, Sq, Sk, H, Hk, dtype, seed, dev):
    g = torch.Generator().manual_seed(seed)
    mk = lambda s, h, d: torch.randn(B, s, h, d, generator=g).to(dtype).to(dev)
    return mk(Sq, H, D), mk(Sk, Hk, D), mk(Sk, Hk, Dv), mk(Sq, H, Dv)


def _ref(q, k, v, do, causal, window=(-1, -1), **kw):
    """(out, lse, dq, dk, dv) fp64, on the tensors' device"""
    import _blockref as R

    return R.attention(q, k, v, dout=do, autograd=True, causal=causal, window=tuple(window), **kw)


def _run(be, q, k, v, do, causal, fwd_kw=None, **kw):
    """(out, lse, delta, dq, dk, dv) of one forward and one backward with plain outputs"""
    B, Sq, H, D = q.shape
    scale = D ** -0.5
    out = torch.empty(B, Sq, H, v.shape[-1], dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **(kw if fwd_kw is None else fwd_kw))
    delta = torch.empty_like(lse)
    be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, **kw)
    return out, lse, delta, dq, dk, dv


def _same(name, got, ref):
    out, lse, _, dq, dk, dv = got
    _check(f"{name}.out", out, ref[0], 0, kind="out")
    _check(f"{name}.lse", lse, ref[1], 0, kind="lse")
    _grads_ok(name, (dq, dk, dv), ref[2:])


def _accumulate(be, name, q, k, v, do, lse, delta, causal, ref):
    """accumulate outputs: the forward's `acc_init`, then a second merge (the same block again: the same out, lse + log 2); the
    backward's dq_acc / dk_acc / dv_acc twice"""
    B, Sq, H, D = q.shape
    Dv, scale, dev = v.shape[-1], D ** -0.5, q.device
    oa = torch.empty(B, Sq, H, Dv, dtype=torch.float32, device=dev)
    la = torch.empty(B, H, Sq, dtype=torch.float32, device=dev)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out_acc=oa, lse_acc=la, acc_init=True)
    _check(f"{name}.out_acc", oa, ref[0], 0, kind="out")
    fin = torch.isfinite(ref[1])
    assert torch.allclose(la[fin].double(), ref[1][fin], atol=1e-4) and bool((la[~fin] == float("-inf")).all())
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out_acc=oa, lse_acc=la)
    _check(f"{name}.out_acc2", oa, ref[0], 0, kind="out")
    assert torch.allclose(la[fin].double(), ref[1][fin] + 0.6931471805599453, atol=1e-4)
    dqa = torch.empty(q.shape, dtype=torch.float32, device=dev)
    dka, dva = torch.empty(k.shape, dtype=torch.float32, device=dev), torch.empty(v.shape, dtype=torch.float32, device=dev)
    common = dict(softmax_scale=scale, causal=causal, dq_acc=dqa, dk_acc=dka, dv_acc=dva)
    be.bwd(do, q, k, v, lse, delta, acc_init=True, **common)
    _grads_ok(f"{name}.acc", (dqa, dka, dva), ref[2:])
    be.bwd(do, q, k, v, lse, delta, acc_init=False, **common)
    _grads_ok(f"{name}.acc2", (dqa / 2, dka / 2, dva / 2), ref[2:])


def test_mla_192_128_gqa_ragged_causal():
    """(192, 128) bf16, B 2, H 4 / Hk 2, Sq = Sk = 333, causal: ragged tails, three 128-key blocks, eleven 32-row Q tiles (more
    than the LDS stages), the group sum in registers; plain and accumulate outputs"""
    be, dev = _be()
    q, k, v, do = _inputs(192, 128, 2, 333, 333, 4, 2, BF, 1, dev)
    ref = _ref(q, k, v, do, True)
    got = _run(be, q, k, v, do, True)
    assert got[0].shape == (2, 333, 4, 128) and got[5].shape == v.shape
    _same("mla", got, ref)
    _accumulate(be, "mla", q, k, v, do, got[1], got[2], True, ref)


@extended
@pytest.mark.parametrize("D,Dv,dtype,B,Sq,Sk,H,Hk,causal", [
    (192, 128, FP, 1, 130, 333, 4, 2, True),         # bottom-right aligned, more keys than queries
    (192, 128, FP, 1, 130, 333, 4, 2, False),
    (192, 128, FP, 1, 260, 130, 2, 1, True),         # rows without a key: lse = +inf, out = 0
    (136, 72, BF, 2, 333, 333, 4, 2, True),          # padded widths: 8 columns of the third QK quarter, 8 of the second V quarter
    (160, 64, BF, 1, 333, 200, 2, 2, True),          # the second V quarter all padding
    (144, 128, BF, 1, 200, 333, 2, 1, False),
    (192, 8, BF, 1, 333, 333, 4, 2, True),           # one 16-byte chunk of V
    (192, 128, BF, 1, 2500, 2500, 2, 1, True),       # both LDS stages, every wave role
])
def test_shapes_against_fp64(D, Dv, dtype, B, Sq, Sk, H, Hk, causal):
    be, dev = _be()
    q, k, v, do = _inputs(D, Dv, B, Sq, Sk, H, Hk, dtype, D + Dv + Sq, dev)
    ref = _ref(q, k, v, do, causal)
    got = _run(be, q, k, v, do, causal)
    _same(f"d{D}_{Dv}", got, ref)
    if Sq == 260:
        dark = torch.isinf(ref[1])
        assert dark.any() and bool((got[1][dark] == float("inf")).all()) and bool((got[0].transpose(1, 2)[dark] == 0).all())
    if Sq < 2000:
        _accumulate(be, f"d{D}_{Dv}", q, k, v, do, got[1], got[2], causal, ref)


@extended
@pytest.mark.parametrize("window,shift", [((100, -1), 0), ((100, -1), 50), ((100, -1), -60), ((37, 21), 0), ((37, 21), 45),
                                          ((37, 21), -45)])
@pytest.mark.parametrize("D,Dv", [(192, 128), (136, 72)])
def test_bounded_windows_and_mask_shift_run_the_7_gemm_dq(D, Dv, window, shift):
    be, dev = _be()
    causal = window[1] < 0
    q, k, v, do = _inputs(D, Dv, 1, 333, 333, 4, 2, BF, 7 + shift, dev)
    ref = _ref(q, k, v, do, causal, window, shift=shift)
    kw = dict(window=window, **({"mask_shift": shift} if shift else {}))
    _same(f"win{window}{shift:+d}", _run(be, q, k, v, do, causal, **kw), ref)


def _packed(lens, D, Dv, H, Hk, dev, seed):
    g = torch.Generator().manual_seed(seed)
    T = sum(lens)
    mk = lambda h, d: torch.randn(T, h, d, generator=g).to(BF).to(dev)
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    return mk(H, D), mk(Hk, D), mk(Hk, Dv), mk(H, Dv), cu


def _half_rows(cu, half):
    """indices of the packed rows a half selects (oracle/oracle_backend.py: _span) and the cu_seqlens of the selection"""
    idx, out = [], [0]
    for a, b in zip(cu, cu[1:]):
        L = b - a
        s, n = (a, L) if half == 0 else ((a, L // 2) if half == 1 else (a + L // 2, L - L // 2))
        idx += list(range(s, s + n))
        out.append(out[-1] + n)
    return idx, out


@extended
@pytest.mark.parametrize("q_half,k_half,causal,window,shift_lens", [
    (0, 0, True, (-1, -1), 0),          # every sequence whole
    (2, 0, False, (-1, -1), 0),         # the zigzag steps' halves
    (0, 1, False, (-1, -1), 0),
    (0, 0, True, (37, -1), 1),          # a band moved by every sequence's own length: short ones lit, long ones cut and dark rows
    (0, 0, True, (37, -1), -1),         # ... wholly dark
])
def test_packed_batch_with_halves_and_per_sequence_shift(q_half, k_half, causal, window, shift_lens):
    """one packed batch mixing lit, cut, dark and empty sequences"""
    be, dev = _be()
    lens = [0, 6, 40, 333, 0, 130]
    D, Dv, H, Hk = 192, 128, 4, 2
    q, k, v, do, cu = _packed(lens, D, Dv, H, Hk, dev, 17)
    iq, cq = _half_rows(cu, q_half)
    ik, ck = _half_rows(cu, k_half)
    ref = _ref(q[iq], k[ik], v[ik], do[iq], causal, window, cu_seqlens_q=cq, cu_seqlens_k=ck, shift_lens=shift_lens)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    T, scale = q.shape[0], D ** -0.5
    vl = dict(cu_seqlens_q=cu_t, cu_seqlens_k=cu_t, max_seqlen_q=max(lens), max_seqlen_k=max(lens), q_half=q_half, k_half=k_half,
              window=window, **({"mask_shift_lens": shift_lens} if shift_lens else {}))
    out = torch.full((T, H, Dv), 7.0, dtype=BF, device=dev)
    lse = torch.full((H, T), 7.0, dtype=torch.float32, device=dev)
    be.fwd(q, k, v, softmax_scale=scale, causal=causal, out=out, lse=lse, **vl)
    _check("packed.out", out[iq], ref[0], 0, kind="out")
    _check("packed.lse", lse[:, iq], ref[1], 0, kind="lse")
    rest = sorted(set(range(T)) - set(iq))
    assert bool((out[rest] == 7.0).all()) and bool((lse[:, rest] == 7.0).all())        # rows of the other half stay untouched
    delta = torch.zeros_like(lse)
    be.bwd_preprocess(do, out, delta, cu_seqlens_q=cu_t, max_seqlen_q=max(lens), q_half=q_half)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=scale, causal=causal, dq=dq, dk=dk, dv=dv, **vl)
    _grads_ok("packed", (dq[iq], dk[ik], dv[ik]), ref[2:])


@extended
@pytest.mark.parametrize("nsplit", [0, 1, 2, 3, 4])
def test_two_phase_backward_and_forced_shares(nsplit):
    """BWD_COMPUTE / BWD_REDUCE into fp32 accumulators that already hold something; dkdv_nsplit forced to 1 … 4 (fp32 partials,
    one reduce launch per tensor: dK 192 wide, dV 128 wide); nsplit 0: the plan's own choice, single phase"""
    from ring_flash_attn import _C, config

    be, dev = _be()
    q, k, v, do = _inputs(192, 128, 2, 600, 600, 4, 2, BF, 23, dev)
    ref = _ref(q, k, v, do, True)
    scale = 192 ** -0.5
    with config.override(dkdv_nsplit=nsplit):
        out, lse, delta, dq, dk, dv = _run(be, q, k, v, do, True)
        _same(f"ns{nsplit}", (out, lse, delta, dq, dk, dv), ref)
        dqa = torch.full(q.shape, 2.0, dtype=torch.float32, device=dev)
        dka = torch.full(k.shape, -1.0, dtype=torch.float32, device=dev)
        dva = torch.full(v.shape, 0.5, dtype=torch.float32, device=dev)
        common = dict(softmax_scale=scale, causal=True, dq_acc=dqa, dk_acc=dka, dv_acc=dva)
        part = be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_COMPUTE, **common)
        assert bool((dka == -1.0).all()) and bool((dva == 0.5).all())                  # nothing reduced yet
        be.bwd(do, q, k, v, lse, delta, phases=_C.BWD_REDUCE, partials=part, **common)
    _grads_ok(f"ns{nsplit}.two_phase", (dqa - 2.0, dka + 1.0, dva - 0.5), ref[2:])


@extended
@pytest.mark.parametrize("D,Dv,Sq,Sk,causal", [(192, 128, 333, 333, True), (136, 72, 300, 500, True), (160, 64, 400, 260, False)])
def test_hand_off_on_off_and_a_scratch_too_small_for_it(D, Dv, Sq, Sk, causal):
    """the 5-GEMM backward (dS hand-off to csrc/rfa_dqs.hip) and the 7-GEMM one each against fp64; dK / dV bit-identical (the same
    kernel with and without the dS stores); a scratch below the hand-off's size runs the base arguments' own plan for it"""
    from ring_flash_attn import config

    be, dev = _be()
    q, k, v, do = _inputs(D, Dv, 2, Sq, Sk, 4, 2, BF, 29, dev)
    ref = _ref(q, k, v, do, causal)
    res = {}
    for spill in (True, False):
        with config.override(bwd_ds_spill=spill):
            res[spill] = _run(be, q, k, v, do, causal)
        _same(f"spill={spill}", res[spill], ref)
    assert torch.equal(res[True][4], res[False][4]) and torch.equal(res[True][5], res[False][5])
    small = torch.empty(64 << 10, dtype=torch.uint8, device=dev)
    _same("small scratch", _run(be, q, k, v, do, causal, fwd_kw={}, ds_scratch=small), ref)


@extended
@pytest.mark.parametrize("D,Dv,causal,window", [(192, 128, True, (-1, -1)), (136, 72, False, (-1, -1)), (192, 128, True, (100, -1))])
def test_agrees_with_the_zero_padded_call_through_the_existing_kernels(D, Dv, causal, window):
    be, dev = _be()
    q, k, v, do = _inputs(D, Dv, 2, 333, 333, 4, 2, BF, 31, dev)
    pad = lambda t: torch.nn.functional.pad(t, (0, D - Dv))
    got = _run(be, q, k, v, do, causal, window=window)
    want = _run(be, q, k, pad(v), pad(do), causal, window=window)
    _check("pad.out", got[0], want[0][..., :Dv].float(), 0, kind="out")
    assert bool((want[0][..., Dv:] == 0).all())
    _check("pad.lse", got[1], want[1], 0, kind="lse")
    _grads_ok("pad", got[3:], (want[3].float(), want[4].float(), want[5][..., :Dv].float()))


@extended
@pytest.mark.parametrize("W", [2, 4])
def test_the_five_functions_over_ranks_sharing_the_gpu(W):
    """S = 128 rows per rank, D 192 / Dv 128, host staging, against the single-device fp64 call"""
    import _vdim_worker as VW
    from conftest import free_port

    S = 128
    lens = [2 * W * 40, 2 * W * 24]
    base = dict(W=W, S=S, D=192, Dv=128, causal=True)
    cases = [dict(base, kind="ring"), dict(base, kind="ring", causal=False), dict(base, kind="zigzag", form="ring"),
             dict(base, kind="zigzag", form="gather"), dict(base, kind="stripe"), dict(base, kind="ring_varlen", lens=lens),
             dict(base, kind="zigzag_varlen", lens=lens), dict(base, kind="ring", window=(S + 30, -1))]
    errs, notes = VW.run_world(W, cases, True, free_port())
    assert not errs, "\n".join(errs[:20])
    assert len(notes) == 5 * W * len(cases)
