"""Dropout position maps on the HIP kernels (`-m gpu`): include/rfa.h q_pos_stride / q_pos_split / q_pos_offset2 and
their k counterparts, which tell a block call where its rows sit in the full sequence when they are not one contiguous
run — what dropout over the dense ring, zigzag and stripe schedules is built on.

  1. mask read-out, EXACT: with q = 0 every visible probability of a row is the same, so one-hot values / keys / output
     gradients make every kernel print the keep mask it applied; the boolean read-outs must EQUAL
     oracle.flash_attn_ref.dropout_keep at the mapped positions;
  2. numeric: random inputs with GQA against the fp64 attention of tests/_blockref.py, tests/_tol.py kinds
     out / lse / grad unscaled, in every output mode the schedules use;
  3. identities, bit for bit: an explicit identity map is the default call, a two-piece map that describes a contiguous
     range is the one-piece call;
  4. the schedules themselves on the HIP kernels, gloo ranks sharing the GPU, against the single-device oracle call.

Geometries — the smallest at which each kernel can go wrong (a map is (offset, (stride, split, offset2))):
  Z    202 x 202, both sides two pieces split at 101 (odd: inside a 4-key group, a 32-row block, a wave's rows and a tile),
       offsets 101 / 606: misaligned by 1 in front of the split and by (606 - 101) & 3 = 1 behind it
  Zt   256 x 256, split 128 — on the tile boundaries —, offsets 128 / 768
  Zh   two-piece q (202) against one-piece k (101 rows at 303), and one-piece q (101 rows at 606) against two-piece k (202)
  S3   130 x 130, stride 3, q offset 1, k offset 2; S3s: its shifted views, 129 rows, q offset 4
  S4   130 x 130, stride 4, q offset 3, k offset 1
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

BF = torch.bfloat16
SEED = 0x5EED1234ABCD
ZMAP = (101, (1, 101, 606))

#            name   Sq   Sk   q map                  k map
GEO = {
    "Z":   (202, 202, ZMAP, ZMAP),
    "Zt":  (256, 256, (128, (1, 128, 768)), (128, (1, 128, 768))),
    "Zhq": (202, 101, ZMAP, (303, (1, 0, 0))),
    "Zhk": (101, 202, (606, (1, 0, 0)), ZMAP),
    "S3":  (130, 130, (1, (3, 0, 0)), (2, (3, 0, 0))),
    "S3s": (129, 129, (4, (3, 0, 0)), (2, (3, 0, 0))),
    "S4":  (130, 130, (3, (4, 0, 0)), (1, (4, 0, 0))),
}


def _dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda:0")


def _be():
    from ring_flash_attn import _testing
    from ring_flash_attn.backend import get_backend

    _testing.set_backend(None)
    return get_backend()


def _drop(geo, p, head0=0):
    Sq, Sk, (q0, qm), (k0, km) = GEO[geo]
    return (p, SEED, q0, k0, head0, qm, km)


_KEEP = {}


def _keep(geo, p, B, H, causal):
    """the reference: bool (B, H, Sq, Sk), keep mask at the mapped positions AND visible; computed once per case"""
    from _blockref import keep_mask, visible

    key = (geo, p, B, H, causal)
    if key not in _KEEP:
        Sq, Sk = GEO[geo][:2]
        d = _drop(geo, p)
        _KEEP[key] = torch.stack([keep_mask(d, b, H, Sq, Sk) for b in range(B)]) & visible(Sq, Sk, causal)
    return _KEEP[key]


def _fwd(be, q, k, v, causal, drop):
    B, Sq, H, D = q.shape
    out = torch.empty_like(q)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    be.fwd(q, k, v, softmax_scale=D ** -0.5, causal=causal, out=out, lse=lse, dropout=drop)
    return out, lse


def _bwd(be, do, q, k, v, out, lse, causal, drop, delta=None):
    B, Sq, H, D = q.shape
    if delta is None:
        delta = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
        be.bwd_preprocess(do, out, delta)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    be.bwd(do, q, k, v, lse, delta, softmax_scale=D ** -0.5, causal=causal, dq=dq, dk=dk, dv=dv, dropout=drop)
    return dq, dk, dv


def _one_hot_rows(B, S, H, D, base, dtype, dev, value=1.0):
    """(B, S, H, D): row j is value * e_(j - base) for base <= j < base + D, zero elsewhere"""
    t = torch.zeros(B, S, H, D, dtype=dtype, device=dev)
    n = min(D, S - base)
    idx = torch.arange(n, device=dev)
    t[:, base + idx, :, idx] = value
    return t


def _readout(geo, D, causal, dtype=BF):
    """the three read-outs of one geometry; B = 2 (the batch index enters the hash), H = Hk = 2"""
    be, dev = _be(), _dev()
    B, H = 2, 2
    Sq, Sk = GEO[geo][:2]
    q = torch.zeros(B, Sq, H, D, dtype=dtype, device=dev)
    zk = torch.zeros(B, Sk, H, D, dtype=dtype, device=dev)

    # ---- forward: v_j = e_(j - base)  ->  out[i, c] > 0  <=>  keep(i, base + c)
    p = 0.2
    want = _keep(geo, p, B, H, causal)
    got = torch.zeros_like(want)
    lse = None
    for base in range(0, Sk, D):
        n = min(D, Sk - base)
        out, lse = _fwd(be, q, zk, _one_hot_rows(B, Sk, H, D, base, dtype, dev), causal, _drop(geo, p))
        got[:, :, :, base:base + n] = (out[..., :n] > 0).permute(0, 2, 1, 3).cpu()
    assert torch.equal(got, want), f"forward mask of {geo} D={D}: {(got != want).sum().item()} of {want.numel()} elements differ"

    # ---- dK/dV kernel: dO_i = e_(i - base)  ->  dV[j, c] > 0  <=>  keep(base + c, j)      (v = 0: out = 0, delta = 0)
    got = torch.zeros_like(want)
    delta0 = torch.zeros((B, H, Sq), dtype=torch.float32, device=dev)
    for base in range(0, Sq, D):
        n = min(D, Sq - base)
        do = _one_hot_rows(B, Sq, H, D, base, dtype, dev)
        _, _, dv = _bwd(be, do, q, zk, zk, None, lse, causal, _drop(geo, p), delta=delta0)
        got[:, :, base:base + n, :] = (dv[..., :n] > 0).permute(0, 2, 3, 1).cpu()
    assert torch.equal(got, want), f"dK/dV mask of {geo} D={D}: {(got != want).sum().item()} of {want.numel()} elements differ"

    # ---- dQ kernel: k_j = e_(j - base), v = 0.125, dO = 8 / D  ->  dP = 1 on every element, dS_ij = P (keep_ij r - delta_i)
    # with delta_i = r x (kept fraction of row i): dQ[i, c] > 0  <=>  keep(i, base + c), unless EVERY visible key of the row
    # is kept (then dS is exactly 0 for the whole row).  p = 0.5 makes that a matter of the first rows of a causal call
    # only; the reference says which rows they are, nothing is excluded from the comparison.
    p = 0.5
    keep = _keep(geo, p, B, H, causal)
    from _blockref import visible

    nvis = visible(Sq, Sk, causal).sum(-1)                                   # (Sq,)
    whole = keep.sum(-1) == nvis                                              # (B, H, Sq): every visible key kept
    want = keep & ~whole.unsqueeze(-1)
    got = torch.zeros_like(want)
    v = torch.full((B, Sk, H, D), 0.125, dtype=dtype, device=dev)
    do = torch.full((B, Sq, H, D), 8.0 / D, dtype=dtype, device=dev)
    for base in range(0, Sk, D):
        n = min(D, Sk - base)
        k = _one_hot_rows(B, Sk, H, D, base, dtype, dev)
        out, lse2 = _fwd(be, q, k, v, causal, _drop(geo, p))
        dq, _, _ = _bwd(be, do, q, k, v, out, lse2, causal, _drop(geo, p))
        got[:, :, :, base:base + n] = (dq[..., :n] > 0).permute(0, 2, 1, 3).cpu()
    assert torch.equal(got, want), f"dQ mask of {geo} D={D}: {(got != want).sum().item()} of {want.numel()} elements differ"


# ---------------------------------------------------------------------------------------------- 1. mask read-out
@pytest.mark.parametrize("geo,causal", [("Z", True), ("Z", False), ("S3", True)])
def test_mask_readout_core(geo, causal):
    """core tier: the zigzag and the stripe geometry at head dim 128 (the tuned kernels' kDrop / kMap instances)"""
    _readout(geo, 128, causal)


@pytest.mark.extended
@pytest.mark.parametrize("geo,causal", [("Zt", True), ("Zt", False), ("Zhq", False), ("Zhk", False), ("S3", False), ("S3s", True),
                                        ("S4", True), ("S4", False)])
def test_mask_readout_all_geometries(geo, causal):
    _readout(geo, 128, causal)


@pytest.mark.extended
@pytest.mark.parametrize("D", [64, 80, 192, 256])
@pytest.mark.parametrize("geo,causal", [("Z", True), ("Z", False), ("S3", True)])
def test_mask_readout_head_dims(geo, causal, D):
    """64: the two-rows-per-LDS-row instances; 80: zero-padded 128-wide; 192: the wide kernels with the one-launch dK + dV
    form; 256: the wide kernels with one launch per tensor"""
    _readout(geo, D, causal)


@pytest.mark.extended
def test_mask_readout_fp16():
    _readout("Z", 128, True, torch.float16)


# ---------------------------------------------------------------------------------------------- 2. numeric
def _rand(B, Sq, Sk, H, Hk, D, dtype=BF):
    g = torch.Generator().manual_seed(77)
    return (torch.randn(B, Sq, H, D, generator=g).to(dtype), torch.randn(B, Sk, Hk, D, generator=g).to(dtype),
            torch.randn(B, Sk, Hk, D, generator=g).to(dtype), torch.randn(B, Sq, H, D, generator=g).to(dtype))


@pytest.mark.extended
@pytest.mark.parametrize("H,Hk", [(4, 2), (8, 1)])
@pytest.mark.parametrize("D", [128, 64, 256])
@pytest.mark.parametrize("geo", ["Z", "S3"])
def test_numeric_against_fp64(geo, D, H, Hk):
    """random N(0,1) inputs with GQA; forward in plain and accumulate mode, backward in plain, two-phase fp32-accumulate
    and RFA_BWD_KV_OVERWRITE mode, against the fp64 block attention with the mapped keep mask"""
    import _blockref as DP
    import _tol
    from oracle.flash_attn_ref import drop_rescale
    from ring_flash_attn import _C

    be, dev = _be(), _dev()
    B, causal, p = 2, True, 0.2
    Sq, Sk = GEO[geo][:2]
    q, k, v, do = _rand(B, Sq, Sk, H, Hk, D)
    drop = _drop(geo, p)
    scale = D ** -0.5
    ro, rl, rdq, rdk, rdv = DP.attention(q, k, v, dout=do, causal=causal, rescale=drop_rescale(p),
                                         keep=[DP.keep_mask(drop, b, H, Sq, Sk) for b in range(B)])
    tag = f"droppos.{geo}.D{D}.H{H}x{Hk}"

    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    out, lse = _fwd(be, qd, kd, vd, causal, drop)
    _tol.compare(f"{tag}.out", out, ro, "out")
    _tol.compare(f"{tag}.lse", lse, rl, "lse")
    out_acc = torch.full((B, Sq, H, D), float("nan"), dtype=torch.float32, device=dev)
    lse_acc = torch.full((B, H, Sq), float("nan"), dtype=torch.float32, device=dev)
    be.fwd(qd, kd, vd, softmax_scale=scale, causal=causal, out_acc=out_acc, lse_acc=lse_acc, acc_init=True, dropout=drop)
    _tol.compare(f"{tag}.out_acc", out_acc, ro, "out")
    _tol.compare(f"{tag}.lse_acc", lse_acc, rl, "lse")

    dq, dk, dv = _bwd(be, dod, qd, kd, vd, out, lse, causal, drop)
    for nm, got, r_ in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        _tol.compare(f"{tag}.plain.{nm}", got, r_, "grad")
    dlt = torch.empty((B, H, Sq), dtype=torch.float32, device=dev)
    be.bwd_preprocess(dod, out, dlt)
    # two phases into fp32 accumulators that already hold something (zeros), as a ring step does
    acc = [torch.zeros(t.shape, dtype=torch.float32, device=dev) for t in (q, k, v)]
    kw = dict(softmax_scale=scale, causal=causal, dq_acc=acc[0], dk_acc=acc[1], dv_acc=acc[2], dropout=drop)
    part = be.bwd(dod, qd, kd, vd, lse, dlt, phases=_C.BWD_COMPUTE, **kw)
    be.bwd(dod, qd, kd, vd, lse, dlt, phases=_C.BWD_REDUCE, partials=part, **kw)
    for nm, got, r_ in (("dq", acc[0], rdq), ("dk", acc[1], rdk), ("dv", acc[2], rdv)):
        _tol.compare(f"{tag}.two_phase.{nm}", got, r_, "grad")
    # dK/dV overwritten in place (the gather forms' contribution slots), dQ initialised by the call
    acc = [torch.full(t.shape, float("nan"), dtype=torch.float32, device=dev) for t in (q, k, v)]
    be.bwd(dod, qd, kd, vd, lse, dlt, softmax_scale=scale, causal=causal, dq_acc=acc[0], dk_acc=acc[1], dv_acc=acc[2],
           acc_init=True, phases=_C.BWD_KV_OVERWRITE, dropout=drop)
    for nm, got, r_ in (("dq", acc[0], rdq), ("dk", acc[1], rdk), ("dv", acc[2], rdv)):
        _tol.compare(f"{tag}.overwrite.{nm}", got, r_, "grad")


# ---------------------------------------------------------------------------------------------- 3. identities
def _all_five(be, q, k, v, do, causal, drop):
    out, lse = _fwd(be, q, k, v, causal, drop)
    return (out, lse) + _bwd(be, do, q, k, v, out, lse, causal, drop)


@pytest.mark.extended
@pytest.mark.parametrize("D", [128, 64, 192, 256])
def test_identity_maps_are_the_default_call_bit_for_bit(D):
    """reference-free: (a) a call with the explicit identity map (stride 1, no split) is the call with offsets alone;
    (b) a two-piece map whose second piece continues the first (offset2 = offset + split) is the one-piece call, for
    splits on and off every boundary — the mapped kernels' bits against the word-per-four-keys path's"""
    be, dev = _be(), _dev()
    B, S, H, Hk, p = 2, 202, 4, 2, 0.2
    q, k, v, do = (t.to(dev) for t in _rand(B, S, S, H, Hk, D))
    q0, k0 = 101, 606                                                        # misaligned by 1 and by 2
    base = _all_five(be, q, k, v, do, True, (p, SEED, q0, k0, 0))
    names = ("out", "lse", "dq", "dk", "dv")
    same = _all_five(be, q, k, v, do, True, (p, SEED, q0, k0, 0, (1, 0, 0), (1, 0, 0)))
    for nm, a, b in zip(names, base, same):
        assert torch.equal(a, b), f"explicit identity map, D={D}: {nm} differs"
    for sq, sk in ((101, 101), (4, 128), (1, 201), (128, 3), (33, 64)):
        two = _all_five(be, q, k, v, do, True, (p, SEED, q0, k0, 0, (1, sq, q0 + sq), (1, sk, k0 + sk)))
        for nm, a, b in zip(names, base, two):
            assert torch.equal(a, b), f"contiguous two-piece map split q {sq} / k {sk}, D={D}: {nm} differs"


# ---------------------------------------------------------------------------------------------- 4. schedules
def _world_cases(W):
    zz = lambda form, **kw: dict(kind="zigzag", form=form, W=W, S=202, causal=True, **kw)
    cases = [dict(kind="ring", W=W, S=130, causal=True), dict(kind="ring", W=W, S=130, causal=False),
             zz("ring"), zz("gather"), zz("gather_ps"), dict(kind="stripe", W=W, S=130, causal=True)]
    if W == 2:
        cases += [zz("gather", api="kvpacked"), dict(kind="stripe", W=W, S=130, causal=True, api="qkvpacked")]
    else:
        cases += [dict(kind="zigzag", form="gather", W=W, S=512, D=128, causal=True)]    # calls of several workgroups
    return cases


@pytest.mark.extended
@pytest.mark.parametrize("W", [2, 4])
def test_schedules_on_the_hip_kernels(W):
    """the CPU schedule matrix (tests/test_dropout_ring_cpu.py) on the HIP kernels, W gloo ranks sharing the GPU, against
    the single-device oracle call with the same seed; at W = 4 also zigzag at head dim 128 with 512 rows per rank"""
    import _droppos_worker as DW
    import _tol
    from conftest import free_port

    cases = _world_cases(W)
    res, errs = DW.run_world(W, cases, True, free_port())
    assert not errs, "\n".join(errs)
    refs = {}
    for c in cases:
        name = DW.case_name(c)
        key = (c["W"] * c["S"], c.get("D", 64), c["causal"], c.get("api") == "qkvpacked")
        if key not in refs:
            refs[key] = DW.reference(c)
        (ro, rl, rdq, rdk, rdv), r0 = refs[key]
        out, lse, dq, dk, dv = res[name]
        assert (ro.float() - r0.float()).abs().max() > 0.05, name              # dropout did something
        _tol.compare(f"{name}.out", out, ro, "out_ring")
        _tol.compare(f"{name}.lse", lse, rl, "lse_ring")
        for nm, got, ref in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
            _tol.compare(f"{name}.{nm}", got, ref, "grad_ring")
