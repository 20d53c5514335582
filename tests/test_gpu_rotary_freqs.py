"""The rotary kernel that forms its own angles, on the device (`-m gpu`): csrc/rfa_rotfreq.hip through
ring_flash_attn.apply_rotary_freqs.

Reference (`reference` below): ang32 = pos.float() * inv_freq in torch fp32 — the one rounded multiply of the definition — then
cos / sin of ang32 in fp64, times the fp32 value of the scaling, and the textbook rotation in fp64.  Tolerance, derived:
    |out - ref| <= ulp_io(ref) + (|x1| + |x2|) * scaling * (2 k + 3) * 2^-24
ulp_io(ref): the one rounding to the io dtype (half an ulp) and its boundary case (the fp32 value on the other side of a
power of two or of a rounding boundary: up to another half).  Second term: sincosf is within k ulp on values of magnitude <= 1
(k 2^-24 for each of c and s: 2 k), the scaling multiply rounds once, rot() rounds twice (3).  k = 4: OpenCL's bound for sincos,
taken because the HIP math API text installed with ROCm states none for sincosf (profiles/rotary_freqs.md).
Shapes: B 2; S 1, 3 and 5 — one row short of a tile of 2 rows, one over, a prime above two tiles; (H, Hk) (1, 1), (5, 2), q
alone with 17 heads (a tile of more units than a workgroup has threads); the (D, R, rot_offset) rows of GEOM; both pairings;
bf16 and fp16."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

K_ULP = 4
B = 2
CASES = [(1, 1, 1), (3, 5, 2), (5, 17, None)]                    # S, H, Hk (None: q alone)
GEOM = [(128, 128, 0), (192, 64, 128), (40, 16, 8), (256, 256, 0)]  # D, R, rot_offset
SCALINGS = [1.0, 0.0707 * math.log(40) + 1]
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _dev():
    return torch.device("cuda:0")


def _inv_freq(R):
    return (10000.0 ** (-torch.arange(R // 2, dtype=torch.float64) / (R // 2))).float().to(_dev())


def _randn(*shape, dtype, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(_dev())


def _positions(kind, shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    if kind == "arange":
        pos = torch.arange(n) % shape[-1]
    elif kind == "big":                                            # the fp32 conversion rounds; the range reduction works
        pos = torch.tensor([2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31 - 1])[torch.arange(n) % 3]
    else:
        pos = torch.randint(0, 2 ** 20, (n,), generator=g)
        pos = -pos if kind == "negative" else pos
    return pos.to(torch.int32).view(shape).to(_dev())


def reference(x, inv_freq, pos, axes, scaling, inter, ro, conj=False):
    """x (B, S, H, D), pos (A, B, S) int32, axes: the axis of each of the R/2 frequencies -> on the CPU in fp64: the rotated
    tensor and |x1| + |x2| of every element's pair (0 for the pass-through columns)"""
    x, half = x.detach().double().cpu(), inv_freq.numel()
    ang32 = pos.cpu()[torch.tensor(axes)].permute(1, 2, 0).float() * inv_freq.cpu()        # (B, S, R/2), torch fp32
    s32 = torch.tensor(scaling, dtype=torch.float32).double()
    c, s = (ang32.double().cos() * s32).unsqueeze(2), (ang32.double().sin() * s32).unsqueeze(2)
    s = -s if conj else s
    out, mag = x.clone(), torch.zeros_like(x)
    cut = (lambda t: (t[..., ro:ro + 2 * half:2], t[..., ro + 1:ro + 2 * half:2])) if inter else \
        (lambda t: (t[..., ro:ro + half], t[..., ro + half:ro + 2 * half]))
    (x1, x2), (o1, o2), (m1, m2) = cut(x), cut(out), cut(mag)
    o1.copy_(x1 * c - x2 * s)
    o2.copy_(x2 * c + x1 * s)
    m1.copy_(x1.abs() + x2.abs())
    m2.copy_(x1.abs() + x2.abs())
    return out, mag


def _bound(ref, mag, scaling, dtype):
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(ref.abs().clamp(min=2.0 ** emin))[1] - 1       # floor(log2 |ref|), the subnormal range counted as emin
    return torch.ldexp(torch.ones_like(ref), e - mant) + mag * scaling * (2 * K_ULP + 3) * 2.0 ** -24


def _check(what, got, ref, bound):
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    frac = ((got.detach().double().cpu() - ref).abs() / bound).max().item()
    print(f"{what}: worst |err| / bound {frac:.3f}")
    assert frac <= 1.0, f"{what}: |err| is {frac:.3f} of ulp_io(ref) + (|x1| + |x2|) scaling (2 k + 3) 2^-24"


def _off(got, ref, bound):
    """`got` is NOT the result `ref` describes: somewhere it is off by more than the tolerance"""
    return bool(((got.detach().double().cpu() - ref).abs() > bound).any())


@DTYPES
@pytest.mark.parametrize("inter", [False, True], ids=["halves", "interleaved"])
@pytest.mark.parametrize("D,Rw,ro", GEOM)
def test_forward_backward_and_bit_identities(single_rank_group, D, Rw, ro, inter, dtype):
    import ring_flash_attn as R
    from ring_flash_attn.backend import get_backend

    be = get_backend()
    assert be.name == "hip" and be.serves_rotary_freqs
    inv = _inv_freq(Rw)
    axes = [0] * (Rw // 2)
    kw = dict(interleaved=inter, rot_offset=ro)
    for S, H, Hk in CASES:
        q = _randn(B, S, H, D, dtype=dtype, seed=5)
        k = _randn(B, S, Hk, D, dtype=dtype, seed=6) if Hk else None
        for kind in ("arange", "random", "big", "negative"):
            pos = _positions(kind, (B, S))
            for scaling in SCALINGS:
                outs = R.apply_rotary_freqs(q, k, inv, positions=pos, attention_scaling=scaling, **kw)
                for name, x, out in zip("qk", (q, k), outs if Hk else (outs,)):
                    ref, mag = reference(x, inv, pos[None], axes, scaling, inter, ro)
                    _check(f"S {S} {kind} x{scaling:.2f} {name}", out, ref, _bound(ref, mag, scaling, dtype))
                    assert torch.equal(out[..., :ro], x[..., :ro]) and torch.equal(out[..., ro + Rw:], x[..., ro + Rw:])
                    if scaling != 1.0:                             # a kernel that ignores the argument fails here
                        ref1, mag1 = reference(x, inv, pos[None], axes, 1.0, inter, ro)
                        assert _off(out, ref1, _bound(ref1, mag1, 1.0, dtype))
        # backward = the inverse rotation of the incoming gradient; forward and then conj restores the input
        pos = _positions("random", (B, S))
        qa = q.clone().requires_grad_(True)
        g = _randn(B, S, H, D, dtype=dtype, seed=7)
        out = R.apply_rotary_freqs(qa, None, inv, positions=pos, attention_scaling=SCALINGS[1], **kw)
        out.backward(g)
        gref, gmag = reference(g, inv, pos[None], axes, SCALINGS[1], inter, ro, conj=True)
        _check(f"S {S} dq", qa.grad, gref, _bound(gref, gmag, SCALINGS[1], dtype))
        fwd = R.apply_rotary_freqs(q, None, inv, positions=pos, **kw)
        back = torch.empty_like(q)
        be.rotary_freqs([fwd], [back], inv, positions=pos, conj=True, **kw)
        # the second step's own tolerance at its input (o1, o2), plus the first step's error of o1 and o2 — each within ITS
        # tolerance — carried back by a rotation: |c| e1 + |s| e2 <= e1 + e2
        o64, x64 = fwd.double().cpu(), q.double().cpu()
        _, omag = reference(fwd, inv, pos[None], axes, 1.0, inter, ro)
        _, xmag = reference(q, inv, pos[None], axes, 1.0, inter, ro)
        first = _bound(o64, xmag, 1.0, dtype)
        _, carried = reference(first, inv, pos[None], axes, 1.0, inter, ro)       # (e1 + e2 of every pair)
        _check(f"S {S} round trip", back, x64, _bound(x64, omag, 1.0, dtype) + carried)
        # bit identities: two runs, k riding along or alone, in place, a strided qkv slice, the (1, T) and the packed form
        one = R.apply_rotary_freqs(q, k, inv, positions=pos, **kw)
        two = R.apply_rotary_freqs(q, k, inv, positions=pos, **kw)
        q1, k1 = one if Hk else (one, None)
        assert torch.equal(q1, two[0] if Hk else two) and torch.equal(q1, fwd)
        qkv = _randn(B, S, 3, H, D, dtype=dtype, seed=9)
        a, b = R.apply_rotary_freqs(qkv[:, :, 0], qkv[:, :, 1], inv, positions=pos, **kw)
        c, d = R.apply_rotary_freqs(qkv[:, :, 0].contiguous(), qkv[:, :, 1].contiguous(), inv, positions=pos, **kw)
        assert torch.equal(a, c) and torch.equal(b, d)
        w = qkv.clone()
        r3 = R.apply_rotary_freqs(w[:, :, 0], w[:, :, 1], inv, positions=pos, inplace=True, **kw)
        assert r3[0].data_ptr() == w[:, :, 0].data_ptr() and torch.equal(w[:, :, 0], a) and torch.equal(w[:, :, 1], b) and torch.equal(w[:, :, 2], qkv[:, :, 2])
        if Hk:
            assert torch.equal(R.apply_rotary_freqs(k, None, inv, positions=pos, **kw), k1)
        packed = R.apply_rotary_freqs(q[0], None, inv, positions=pos[0], **kw)
        assert torch.equal(packed, q1[0])
        ar = R.apply_rotary_freqs(q, None, inv, offset=11, **kw)
        assert torch.equal(ar, R.apply_rotary_freqs(q, None, inv, positions=_positions("arange", (S,)), offset=11, **kw))


QWEN2_VL = [0] * 16 + [1] * 24 + [2] * 24                         # mrope_section [16, 24, 24]
QWEN3_VL = [0] * 64                                               # interleaved [24, 20, 20]: t h w t h w ... t t t t
QWEN3_VL[1:60:3] = [1] * 20
QWEN3_VL[2:60:3] = [2] * 20
FOUR = [c % 4 for c in range(64)]


@DTYPES
@pytest.mark.parametrize("axes", [QWEN2_VL, QWEN3_VL, FOUR], ids=["qwen2vl", "qwen3vl", "four_axes"])
def test_mrope(single_rank_group, axes, dtype):
    import ring_flash_attn as R

    S, H, Hk, D = 5, 5, 2, 128
    A = max(axes) + 1
    inv = _inv_freq(D)
    q, k = _randn(B, S, H, D, dtype=dtype, seed=5), _randn(B, S, Hk, D, dtype=dtype, seed=6)
    pos = torch.stack([_positions("random", (B, S), seed=20 + a) for a in range(A)])
    scaling = SCALINGS[1]
    qa = q.clone().requires_grad_(True)
    qo, ko = R.apply_rotary_freqs(qa, k, inv, positions=pos, freq_axis=axes, attention_scaling=scaling)
    g = _randn(B, S, H, D, dtype=dtype, seed=7)
    qo.backward(g)
    for name, x, out, conj in (("q", q, qo, False), ("k", k, ko, False), ("dq", g, qa.grad, True)):
        ref, mag = reference(x, inv, pos, axes, scaling, False, 0, conj)
        _check(f"mrope {name}", out, ref, _bound(ref, mag, scaling, dtype))
        ref0, mag0 = reference(x, inv, pos, [0] * 64, scaling, False, 0, conj)       # a kernel that reads axis 0 alone fails
        assert _off(out, ref0, _bound(ref0, mag0, scaling, dtype))
    # every axis carrying the same positions is the single-axis call, bit for bit; (A, T) positions of the packed form
    same = pos[:1].expand(A, B, S).contiguous()
    q1, k1 = R.apply_rotary_freqs(q, k, inv, positions=same, freq_axis=axes, attention_scaling=scaling)
    q2, k2 = R.apply_rotary_freqs(q, k, inv, positions=pos[0], attention_scaling=scaling)
    assert torch.equal(q1, q2) and torch.equal(k1, k2)
    packed = R.apply_rotary_freqs(q[1], None, inv, positions=pos[:, 1].contiguous(), freq_axis=axes, attention_scaling=scaling)
    assert torch.equal(packed, qo.detach()[1])


@pytest.mark.parametrize("inter", [False, True], ids=["halves", "interleaved"])
@pytest.mark.parametrize("kind", ["ring", "zigzag_ring", "stripe"])
def test_layout_of_a_shard_is_its_positions_and_the_rows_of_the_whole(single_rank_group, kind, inter):
    """rank r of W = 4, its map handed to the backend as the public call hands it: the map equals
    positions=local_positions(..., rank=r, world_size=W) on the same shard and the shard's rows of the single-device result,
    bit for bit"""
    import ring_flash_attn as R
    from ring_flash_attn._common import pos_map, stripe_map, zigzag_map
    from ring_flash_attn.backend import get_backend

    W, n, H, Hk, D, Rw, ro = 4, 10, 3, 1, 64, 32, 16
    func = getattr(R, f"{kind}_flash_attn_func")
    inv = _inv_freq(Rw)
    kw = dict(interleaved=inter, rot_offset=ro)
    q, k = _randn(B, W * n, H, D, dtype=torch.bfloat16, seed=5), _randn(B, W * n, Hk, D, dtype=torch.bfloat16, seed=6)
    qf, kf = R.apply_rotary_freqs(q, k, inv, attention_scaling=SCALINGS[1], **kw)
    assert torch.equal(R.apply_rotary_freqs(q, None, inv, layout=func, attention_scaling=SCALINGS[1], **kw), qf)   # rank 0 of 1
    for r in range(W):
        pos = R.local_positions(func, n, rank=r, world_size=W, device=_dev())
        pm = {"ring": pos_map(r * n), "zigzag_ring": zigzag_map(r, W, n // 2), "stripe": stripe_map(r, W)}[kind]
        qs, ks = q.index_select(1, pos.long()), k.index_select(1, pos.long())
        ql, kl = torch.empty_like(qs), torch.empty_like(ks)
        get_backend().rotary_freqs([qs, ks], [ql, kl], inv, pos_map=pm, scaling=SCALINGS[1], **kw)
        qp, kp = R.apply_rotary_freqs(qs, ks, inv, positions=pos, attention_scaling=SCALINGS[1], **kw)
        assert torch.equal(ql, qp) and torch.equal(kl, kp)
        assert torch.equal(ql, qf.index_select(1, pos.long())) and torch.equal(kl, kf.index_select(1, pos.long()))
