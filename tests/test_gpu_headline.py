"""Full-size checks at the BASELINE.json headline shape (B=1, S=8192, H=32, Hk=8, D=128, bf16, causal) — the exact
launch bench.py times (256-key dK/dV form, query-range split 2, triangular dS spill):
  * ONE WHOLE K/V-HEAD GROUP (4 query heads + their kv head, all 8192 query rows and key rows) against the CPU oracle
    with every criterion of tests/_tol.py, and against an fp64 computation of the same group ROW BY ROW (relative to
    each row's own norm) — references that consume nothing the kernels produced (own lse, own out, own delta)
  * sampled query rows of the other heads recomputed exactly on the host (fp64) — out, lse, dq
  * V = const  =>  out = const  (softmax rows sum to one over 8192 keys)
  * splitting the key range in two and merging with the fused accumulate epilogue == one pass
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

S, H, HK, D = 8192, 32, 8, 128


def _row(name, i, h, got, ref):
    """one sampled row (128 values) against its exact fp64 value: RELATIVE to the row itself — late rows of a long
    causal sequence have |out| ~ 0.02, where an absolute bound would hide a systematic error — plus the
    element-wise bound; the io dtype's rounding alone is 2^-9 ~ 2e-3 relative"""
    import os

    err = (got - ref)
    rel = (err.norm() / ref.norm().clamp_min(1e-30)).item()
    mx = err.abs().max().item()
    path = os.environ.get("RFA_TOL_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"row        rel-norm {rel:.3e} max_err {mx:.3e} max_ref {ref.abs().max().item():.3e}  headline.{name}[{i},{h}]\n")
    # (observed on MI355X: <= 3.3e-3; a row whose exact value is zero — dq of a query that sees one key — is held to
    #  the absolute floor instead: ROW_FLOOR per element, i.e. 1.1e-3 on the norm of a 128-wide row, 0.6 % of the norm
    #  of a late causal row (||out|| ~ 0.2))
    assert err.norm().item() <= ROW_REL * ref.norm().item() + ROW_FLOOR * ref.numel() ** 0.5, \
        f"{name}[{i},{h}]: relative error of the row {rel:.3e} > {ROW_REL}"
    assert mx <= 2e-3 + 1.6e-2 * ref.abs().max().item(), f"{name}[{i},{h}]: max|err| {mx:.3e}"


ROW_REL, ROW_FLOOR = 1e-2, 1e-4


def all_rows_relative(name, got, ref, allowance=None):
    """EVERY row (last dim) of got against the exact fp64 ref, relative to the row's own norm — the criterion of _row,
    vectorised: ||err_row|| <= ROW_REL ||ref_row|| + ROW_FLOOR sqrt(D) (+ allowance per row: dQ only, the effect of
    delta being computed from the ROUNDED saved output — tests/_fullref.py: dq_delta_allowance; it is O(1) relative
    for the first few rows of a sequence and vanishes for the others)"""
    import os

    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    en, rn = (got - ref).norm(dim=-1), ref.norm(dim=-1)
    lim = ROW_REL * rn + ROW_FLOOR * ref.shape[-1] ** 0.5
    if allowance is not None:
        lim = lim + allowance.double().cpu()
    worst = (en / lim).max().item()
    path = os.environ.get("RFA_TOL_LOG")
    if path:
        rel = (en / rn.clamp_min(1e-30))[rn > 10 * ROW_FLOOR * ref.shape[-1] ** 0.5]
        with open(path, "a") as f:
            f.write(f"all-rows   worst err/limit {worst:.3f}, worst rel-norm {rel.max().item() if rel.numel() else 0.0:.3e} "
                    f"over {en.numel()} rows  {name}\n")
    bad = (en > lim).nonzero()
    assert bad.numel() == 0, (f"{name}: {bad.shape[0]} of {en.numel()} rows exceed the row-relative bound, first at "
                              f"{bad[0].tolist()}: ||err|| {en[tuple(bad[0])].item():.3e} vs ||ref|| {rn[tuple(bad[0])].item():.3e}")


def _inputs(dev):
    g = torch.Generator().manual_seed(42)
    q = torch.randn(1, S, H, D, generator=g).to(torch.bfloat16)
    kv = torch.randn(1, S, 2, HK, D, generator=g).to(torch.bfloat16)
    do = torch.randn(1, S, H, D, generator=g).to(torch.bfloat16)
    return q, kv, do


def test_headline_sampled_rows(single_rank_group):
    import ring_flash_attn as R

    dev = torch.device("cuda:0")
    q, kv, do = _inputs(dev)
    qd, kvd = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    out, lse, _ = R.zigzag_ring_flash_attn_kvpacked_func(qd, kvd, causal=True, return_attn_probs=True)
    out.backward(do.to(dev))
    out, lse = out.cpu().double(), lse.cpu().double()
    dq, dkv = qd.grad.cpu().double(), kvd.grad.cpu().double()
    qf, kf, vf, dof = q.double(), kv[:, :, 0].double(), kv[:, :, 1].double(), do.double()
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(1)
    rows = [0, 1, 255, 256, 4095, 4096, S - 1] + torch.randint(0, S, (9,), generator=g).tolist()
    for i in rows:
        h = int(torch.randint(0, H, (1,), generator=g))
        hk = h // (H // HK)
        s = (kf[0, : i + 1, hk] @ qf[0, i, h]) * scale
        l = torch.logsumexp(s, 0)
        p = torch.exp(s - l)
        o = p @ vf[0, : i + 1, hk]
        assert abs(l - lse[0, h, i]) < 1e-3
        _row("out", i, h, out[0, i, h], o)
        dp = vf[0, : i + 1, hk] @ dof[0, i, h]
        delta = (dof[0, i, h] * o).sum()              # (the exact out, not the kernel's)
        ds = p * (dp - delta) * scale
        ref_dq = ds @ kf[0, : i + 1, hk]
        _row("dq", i, h, dq[0, i, h], ref_dq)


@pytest.mark.parametrize("hk", [5])
def test_headline_full_tensor_one_kv_group(single_rank_group, hk):
    """The launch bench.py times, checked on a WHOLE K/V-head group: the 4 query heads of kv head `hk` and that kv head,
    all 8192 query rows (out, lse, dq) and all 8192 key rows (dk, dv: sums over the 4 heads and every later query).
    (i) the CPU oracle on exactly that group with every criterion of tests/_tol.py; (ii) an fp64 computation of the
    group (tests/_fullref.py on the device: rocBLAS + torch, nothing of this library) row by row, relative to each
    row.  Neither reference reads the kernels' lse / out."""
    import _fullref
    import _tol
    import ring_flash_attn as R
    from oracle import flash_attn_ref as O

    dev = torch.device("cuda:0")
    q, kv, do = _inputs(dev)
    qd, kvd = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    out, lse, _ = R.zigzag_ring_flash_attn_kvpacked_func(qd, kvd, causal=True, return_attn_probs=True)
    out.backward(do.to(dev))
    G = H // HK
    hs = slice(hk * G, (hk + 1) * G)
    got = dict(out=out[0, :, hs].detach(), lse=lse[0, hs].detach(), dq=qd.grad[0, :, hs],
               dk=kvd.grad[0, :, 0, hk], dv=kvd.grad[0, :, 1, hk])
    got = {n: t.float().cpu() for n, t in got.items()}
    # (i) the oracle, one group
    qs, ks, vs, dos = q[:, :, hs], kv[:, :, 0, hk:hk + 1], kv[:, :, 1, hk:hk + 1], do[:, :, hs]
    ro, rl, _, _ = O._flash_attn_forward(qs, ks, vs, 0.0, D ** -0.5, True)
    rdq, rdk, rdv = torch.empty_like(qs), torch.empty_like(ks), torch.empty_like(vs)
    O._flash_attn_backward(dos, qs, ks, vs, ro, rl, rdq, rdk, rdv, 0.0, D ** -0.5, True)
    _tol.compare(f"headline.group{hk}.out", got["out"], ro[0], "out")
    _tol.compare(f"headline.group{hk}.lse", got["lse"], rl[0], "lse")
    _tol.compare(f"headline.group{hk}.dq", got["dq"], rdq[0], "grad")
    _tol.compare(f"headline.group{hk}.dk", got["dk"], rdk[0, :, 0], "grad")
    _tol.compare(f"headline.group{hk}.dv", got["dv"], rdv[0, :, 0], "grad")
    # (ii) fp64, every row relative to itself
    fo, fl, fdq, fdk, fdv = _fullref.attention_fwd_bwd_fp64(qs[0].to(dev), ks[0].to(dev), vs[0].to(dev), dos[0].to(dev))
    assert (got["lse"].double() - fl.cpu()).abs().max().item() < 2e-5 + 2e-6 * fl.abs().max().item()
    all_rows_relative(f"headline.group{hk}.out", got["out"], fo)
    all_rows_relative(f"headline.group{hk}.dq", got["dq"], fdq, _fullref.attention_fwd_bwd_fp64.dq_delta_allowance)
    all_rows_relative(f"headline.group{hk}.dk", got["dk"], fdk[:, 0])
    all_rows_relative(f"headline.group{hk}.dv", got["dv"], fdv[:, 0])


def test_headline_constant_v_and_split_merge(single_rank_group):
    from ring_flash_attn.backend import get_backend
    from ring_flash_attn._testing import set_backend

    set_backend(None)
    be = get_backend()
    dev = torch.device("cuda:0")
    q, kv, _ = _inputs(dev)
    q, k = q.to(dev), kv[:, :, 0].to(dev).contiguous()
    v = torch.full((1, S, HK, D), 0.75, dtype=torch.bfloat16, device=dev)
    scale = D ** -0.5
    out = torch.empty_like(q)
    lse = torch.empty((1, H, S), dtype=torch.float32, device=dev)
    be.fwd(q, k, v, softmax_scale=scale, causal=True, out=out, lse=lse)
    assert (out.float() - 0.75).abs().max().item() < 4e-3          # rows of P sum to 1

    # non-causal over [0,S) in one pass vs two half passes merged by the fused epilogue
    v = kv[:, :, 1].to(dev).contiguous()
    one = torch.empty((1, S, H, D), dtype=torch.float32, device=dev)
    l_one = torch.empty((1, H, S), dtype=torch.float32, device=dev)
    be.fwd(q, k, v, softmax_scale=scale, causal=False, out_acc=one, lse_acc=l_one, acc_init=True)
    two = torch.empty_like(one)
    l_two = torch.empty_like(l_one)
    be.fwd(q, k[:, : S // 2], v[:, : S // 2], softmax_scale=scale, causal=False, out_acc=two, lse_acc=l_two, acc_init=True)
    be.fwd(q, k[:, S // 2:], v[:, S // 2:], softmax_scale=scale, causal=False, out_acc=two, lse_acc=l_two)
    assert (l_one - l_two).abs().max().item() < 1e-4
    assert (one - two).abs().max().item() < 2e-3


def test_max_length_65536_single_gpu(single_rank_group):
    """The headline's TOTAL sequence (8192 x 8 = 65536) on one GPU: 256 query blocks per head, 1024 KV tiles, the 7-GEMM
    backward (one head's dS would pass the hand-off's 32-bit block offset).  Its largest tensor holds 67 M elements (128 MiB):
    it walks long sequences, it does not come near 2^31 elements or 2^32 bytes from a pointer — tests/test_gpu_far_addressing.py
    does.  Checks: sampled rows of out/lse/dq in fp64 on the host, and the last 5536 key rows of
    dk/dv (+ the same query rows of dq, lse) of one kv head against a full fp64 computation of that sub-problem."""
    import ring_flash_attn as R

    dev = torch.device("cuda:0")
    SL, HH, HKK = 65536, 4, 2
    g = torch.Generator().manual_seed(65)
    q = torch.randn(1, SL, HH, D, generator=g).to(torch.bfloat16)
    kv = torch.randn(1, SL, 2, HKK, D, generator=g).to(torch.bfloat16)
    do = torch.randn(1, SL, HH, D, generator=g).to(torch.bfloat16)
    qd, kvd = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    out, lse, _ = R.zigzag_ring_flash_attn_kvpacked_func(qd, kvd, causal=True, return_attn_probs=True)
    out.backward(do.to(dev))
    out, lse = out.cpu().double(), lse.cpu().double()
    dq, dkv = qd.grad.cpu().double(), kvd.grad.cpu().double()
    qf, kf, vf, dof = q.double(), kv[:, :, 0].double(), kv[:, :, 1].double(), do.double()
    scale = 1.0 / math.sqrt(D)
    for i, h in [(0, 0), (255, 1), (256, 2), (32767, 3), (32768, 0), (65535, 1), (50001, 2)]:
        hk = h // (HH // HKK)
        s = (kf[0, : i + 1, hk] @ qf[0, i, h]) * scale
        l = torch.logsumexp(s, 0)
        p = torch.exp(s - l)
        o = p @ vf[0, : i + 1, hk]
        assert abs(l - lse[0, h, i]) < 1e-3
        _row("out", i, h, out[0, i, h], o)
        dp = vf[0, : i + 1, hk] @ dof[0, i, h]
        delta = (dof[0, i, h] * o).sum()              # (the exact out, not the kernel's)
        ref_dq = (p * (dp - delta) * scale) @ kf[0, : i + 1, hk]
        _row("dq", i, h, dq[0, i, h], ref_dq)
    # dk / dv: the key rows 60000 .. 65535 of kv head 1 receive gradient from the queries 60000 .. 65535 of its two query
    # heads only, so an fp64 computation of THAT sub-problem (5536 bottom-right aligned queries against all keys; own lse,
    # out and delta — tests/_fullref.py on the device) is their exact reference, row by row
    import _fullref

    j, hk = 60000, 1
    hs = slice(hk * (HH // HKK), (hk + 1) * (HH // HKK))
    _, fl, fdq, fdk, fdv = _fullref.attention_fwd_bwd_fp64(q[0, j:, hs].to(dev), kv[0, :, 0, hk:hk + 1].to(dev),
                                                          kv[0, :, 1, hk:hk + 1].to(dev), do[0, j:, hs].to(dev))
    assert (lse[0, hs, j:] - fl.cpu()).abs().max().item() < 2e-5 + 2e-6 * fl.abs().max().item()
    all_rows_relative("s65536.dq", dq[0, j:, hs], fdq, _fullref.attention_fwd_bwd_fp64.dq_delta_allowance)
    all_rows_relative("s65536.dk", dkv[0, j:, 0, hk], fdk[j:, 0])
    all_rows_relative("s65536.dv", dkv[0, j:, 1, hk], fdv[j:, 0])
