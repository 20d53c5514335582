"""The per-head QK RMSNorm + rotary kernels that form their own angles, on the device (`-m gpu`): csrc/rfa_qknormfreq.hip through
ring_flash_attn.apply_qk_norm_rotary_freqs.

Reference: the textbook formula under fp64 autograd, the angle formed as the kernel forms it — ang32 = float32(pos) * inv_freq in
torch fp32, then cos / sin of ang32 in fp64, times the fp32 value of the scaling — so positions near 10^6 test the range
reduction and not the angle's own rounding.  Bounds: the sum of the two derived bounds the siblings state, each for its part
(u = 2^-8 bf16 / 2^-11 fp16, `half` the io dtype's half subnormal step, k = 4 ulp for sincosf as in tests/test_gpu_rotary_freqs.py):
    forward  |err| <= max(u |ref|, half) + 2^-19 Mf + (2 k + 1) 2^-24 Af      (tests/test_gpu_qk_norm.py: norm, scale, rot())
    dx       |err| <= max(u |ref|, half) + 2^-18 Mb + (2 k + 1) 2^-24 Ab
    dw       |err| <= (n + 24) 2^-24 T + (2 k + 1) 2^-24 At     (fp32 sum; a weight gradient in the io dtype: + u |ref|)
Mf, Mb, T are that file's magnitudes with |c'| and |s'| in them.  The angle's share — sincosf within k ulp for each of c and s,
one rounding by the scaling — enters where a table would be exact: Af, Ab, At are the SAME magnitudes with |c'| = |s'| =
scaling, i.e. (|y1| + |y2|) scaling in the place of |y1 c'| + |y2 s'| (computed by the same function on tables of that
constant).  n = the longest chain of a column's sum from the header of csrc/rfa_qknormfreq.hip:
ceil(tiles / nparts) * passes + 256/G + ceil(nparts/16) + 16 with tiles = B ceil(S / 4), nparts = min(tiles, 1024),
passes = ceil(4 H / (256/G)).
Shapes: B 2, S 6 (tiles of 4 and 2 rows), H 5 / Hk 1 (20 and 4 items of a tile: no whole number of passes), the rows of CASES."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _qknorm_backend import reference as magnitudes          # noqa: E402

pytestmark = pytest.mark.gpu

K_ULP = 4
ROWS = 4
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
QWEN3_VL = [0] * 64                                               # interleaved sections [24, 20, 20]: t h w t h w ... t t t t
QWEN3_VL[1:60:3] = [1] * 20
QWEN3_VL[2:60:3] = [2] * 20
BF, FP = torch.bfloat16, torch.float16
#   id                 lead      H  Hk    D    R   ro  inter dtype wdtype woff scaling eps   positions
CASES = {
    "d128-map-1e6":   ((2, 6), 5, 1, 128, 128, 0, False, BF, torch.float32, 0.0, 1.0, 1e-6, "map"),
    "d64-interleaved": ((2, 6), 5, 1, 64, 64, 0, True, FP, FP, 1.0, 1.25, 1e-6, "tensor"),
    "d72-idle-eps0":  ((2, 6), 5, 1, 72, 32, 8, False, BF, BF, 0.0, 1.0, 0.0, "tensor"),
    "d256":           ((2, 6), 5, 1, 256, 256, 0, False, FP, torch.float32, 0.0, 0.75, 1e-6, "batch"),
    "d192-q-alone-qkv": ((2, 6), 5, None, 192, 64, 128, False, BF, torch.float32, 0.0, 1.0, 1e-6, "batch"),
    "packed-three-axes": ((7,), 5, 1, 128, 128, 0, False, BF, torch.float32, 0.0, 1.0, 1e-6, "thw"),
    "walk-over-the-cap": ((1, ROWS * 1024 + 5), 1, 1, 16, 16, 0, False, BF, torch.float32, 0.0, 1.0, 1e-6, "map"),
}


def _dev():
    return torch.device("cuda:0")


def _randn(*shape, seed, dtype):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _inputs(name):
    """everything of a case on the CPU: tensors, the call's keywords, the (A, B, S) positions and the axis of every frequency"""
    lead, H, Hk, D, Rw, ro, inter, dtype, wdt, woff, scaling, eps, mode = CASES[name]
    heads = (H,) if Hk is None else (H, Hk)
    if name.endswith("qkv"):                                       # strided slices of one (.., 3, H, D) tensor, gradients too
        xs = [_randn(*lead, 3, H, D, seed=5, dtype=dtype)[..., 0, :, :]]
        gs = [_randn(*lead, 3, H, D, seed=6, dtype=dtype)[..., 1, :, :]]
    else:
        xs = [_randn(*lead, h, D, seed=5 + i, dtype=dtype) for i, h in enumerate(heads)]
        gs = [_randn(*lead, h, D, seed=8 + i, dtype=dtype) for i, h in enumerate(heads)]
    ws = [(1.0 - woff + 0.25 * _randn(D, seed=3 + i, dtype=torch.float32)).to(wdt) for i in range(len(heads))]
    inv = (10000.0 ** (-torch.arange(Rw // 2, dtype=torch.float64) / (Rw // 2))).float()
    kw = dict(eps=eps, weight_offset=woff, attention_scaling=scaling, interleaved=inter, rot_offset=ro)
    S = lead[-1]
    rows = (1, S) if len(lead) == 1 else lead
    g = torch.Generator().manual_seed(11)
    axes = [0] * (Rw // 2)
    if mode == "map":                                              # row i at 10^6 - 3 + i: no tensor
        kw["offset"] = 10 ** 6 - 3
        pos = (kw["offset"] + torch.arange(S)).expand(rows).unsqueeze(0)
    elif mode == "thw":                                            # three axes up to about 10^6 (packed: (A, T))
        pos = torch.randint(0, 10 ** 6, (3, *rows), generator=g)
        kw["positions"], kw["freq_axis"], axes = pos.view(3, *lead).to(torch.int32), QWEN3_VL, QWEN3_VL
    else:                                                          # (S,) shared by the batch entries, or (B, S)
        pos = torch.randint(0, 10 ** 6, (1, S) if mode == "tensor" else rows, generator=g)
        kw["positions"] = (pos[0] if mode == "tensor" else pos).to(torch.int32)
        pos = pos.expand(rows).unsqueeze(0)
    return xs, gs, ws, inv, kw, pos, axes, (lead, D, Rw, ro, inter, dtype, wdt, woff, scaling, eps)


def _textbook(x, w, c, s, inter, ro, eps, woff):
    """differentiable fp64: the formulas as the papers print them; c, s (B, S, 1, R/2)"""
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (woff + w)
    Rw = 2 * c.shape[-1]
    r = y[..., ro:ro + Rw]
    if inter:
        x1, x2 = r[..., 0::2], r[..., 1::2]
        rot = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).flatten(-2)
    else:
        x1, x2 = r[..., :Rw // 2], r[..., Rw // 2:]
        rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return torch.cat([y[..., :ro], rot, y[..., ro + Rw:]], dim=-1)


def _chain(B, S, H, D):
    G = max(1, 1 << (D // 8 - 1).bit_length())
    per, tiles = 256 // G, B * -(-S // ROWS)
    nparts = min(tiles, 1024)
    return -(-tiles // nparts) * -(-ROWS * H // per) + per + -(-nparts // 16) + 16


def _bounds(name):
    """per tensor of the case: (ref y, bound), (ref dx, bound), (ref dw, bound) — fp64 on the CPU, computed once per case"""
    if name in _bounds.cache:
        return _bounds.cache[name]
    xs, gs, ws, inv, kw, pos, axes, (lead, D, Rw, ro, inter, dtype, wdt, woff, scaling, eps) = _inputs(name)
    ang32 = pos[torch.tensor(axes)].permute(1, 2, 0).float() * inv                           # (B, S, R/2), torch fp32
    s32 = torch.tensor(scaling, dtype=torch.float32).double()
    c, s = ang32.double().cos() * s32, ang32.double().sin() * s32
    Bn, Sn = ang32.shape[:2]
    rowid = torch.arange(Bn * Sn).view(Bn, Sn)
    flat, const = (c.reshape(Bn * Sn, -1), s.reshape(Bn * Sn, -1)), torch.full((1, Rw // 2), float(s32), dtype=torch.float64)
    u, hs, ka = U_OF[dtype], HALF_STEP[dtype], (2 * K_ULP + 1) * 2.0 ** -24
    res = []
    for x, g, w in zip(xs, gs, ws):
        x4, g4 = (t.reshape(Bn, Sn, *t.shape[-2:]) for t in (x, g))
        x64, w64 = x4.double().requires_grad_(True), w.double().requires_grad_(True)
        y = _textbook(x64, w64, c.unsqueeze(2), s.unsqueeze(2), inter, ro, eps, woff)
        y.backward(g4.double())
        m = magnitudes(x4, w, *flat, rowid, inter, ro, eps, woff, dout=g4)                   # Mf, Mb, T with |c'|, |s'|
        rot = torch.zeros(D, dtype=torch.bool)
        rot[ro:ro + Rw] = True                                     # (the angle's share: rotated columns only)
        a = magnitudes(x4, w, const, const, torch.zeros_like(rowid), inter, ro, eps, woff, dout=g4 * rot)
        Af, Ab, At = a["Mf"] * rot, a["Mb"], a["T"]
        lim = lambda ref, tail: (u * ref.abs()).clamp(min=hs) + tail
        dw_lim = (_chain(Bn, Sn, x.shape[-2], D) + 24) * 2.0 ** -24 * m["T"] + ka * At
        if wdt != torch.float32:
            dw_lim = dw_lim + (U_OF[wdt] * w64.grad.abs()).clamp(min=HALF_STEP[wdt])
        res.append(((y.detach().reshape(x.shape), lim(y.detach(), 2.0 ** -19 * m["Mf"] + ka * Af).reshape(x.shape)),
                    (x64.grad.reshape(x.shape), lim(x64.grad, 2.0 ** -18 * m["Mb"] + ka * Ab).reshape(x.shape)),
                    (w64.grad, dw_lim)))
    _bounds.cache[name] = res
    return res


_bounds.cache = {}


def _to_dev(t):
    """to the device with the strides it has (a slice of a qkv tensor stays one)"""
    if t._base is None:
        return t.to(_dev())
    return t._base.to(_dev()).as_strided(t.shape, t.stride(), t.storage_offset())


def _run(name, **over):
    """the public call under autograd on the device: ([out], [dx], [dw])"""
    import ring_flash_attn as R

    xs, gs, ws, inv, kw, *_ = _inputs(name)
    kw = {k: (v.to(_dev()) if isinstance(v, torch.Tensor) else v) for k, v in dict(kw, **over).items()}
    leaves = [_to_dev(t).requires_grad_(True) for t in xs + ws]
    n = len(xs)
    outs = R.apply_qk_norm_rotary_freqs(leaves[0], leaves[1] if n == 2 else None, leaves[n], leaves[n + 1] if n == 2 else None,
                                        inv.to(_dev()), **kw)
    outs = (outs,) if n == 1 else outs
    torch.autograd.backward(list(outs), [_to_dev(g) for g in gs])
    return [o.detach() for o in outs], [t.grad for t in leaves[:n]], [t.grad for t in leaves[n:]]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_every_gradient_against_fp64_autograd(single_rank_group, name):
    from ring_flash_attn.backend import get_backend

    assert get_backend().name == "hip" and get_backend().serves_qk_norm_freqs
    outs, dxs, dws = _run(name)
    for i, (got3, ref3) in enumerate(zip(zip(outs, dxs, dws), _bounds(name))):
        for what, got, (ref, lim) in zip(("out", "dx", "dw"), got3, ref3):
            err = (got.double().cpu() - ref).abs()
            print(f"{name} tensor {i} {what}: max|err| {err.max().item():.3e}, worst err / bound {(err / lim).max().item():.4f}")
            assert not torch.isnan(got).any() and got.shape == ref.shape and bool((err <= lim).all()), (name, i, what)
    assert dws[0].dtype == CASES[name][8] and outs[0].is_contiguous()
    again = _run(name)                                             # two runs give the same bits, dw included
    assert all(torch.equal(a, b) for p, q in zip(again, (outs, dxs, dws)) for a, b in zip(p, q))


@pytest.mark.parametrize("name", ["d128-map-1e6", "d64-interleaved", "d72-idle-eps0"])
def test_bit_identities(single_rank_group, name):
    import ring_flash_attn as R

    xs, gs, ws, inv, kw, pos, *_ = _inputs(name)
    outs, dxs, dws = _run(name)
    q, k, wq, wk, gq = (t.to(_dev()) for t in (*xs, *ws, gs[0]))
    kw = {k_: (v.to(_dev()) if isinstance(v, torch.Tensor) else v) for k_, v in kw.items()}
    # q's bits with and without k, and its weight gradient's
    ql, wl = q.clone().requires_grad_(True), wq.clone().requires_grad_(True)
    alone = R.apply_qk_norm_rotary_freqs(ql, None, wl, None, inv.to(_dev()), **kw)
    alone.backward(gq)
    assert torch.equal(alone, outs[0]) and torch.equal(ql.grad, dxs[0]) and torch.equal(wl.grad, dws[0])
    # inv_freq = 0 with scaling 1: the bits of the table kernel's norm alone, outputs and dq / dk — the row statistic's order
    norm = dict(eps=kw["eps"], weight_offset=kw["weight_offset"])
    leaves = [t.clone().requires_grad_(True) for t in (q, k)]
    a = R.apply_qk_norm_rotary_freqs(*leaves, wq, wk, torch.zeros_like(inv).to(_dev()), **dict(kw, attention_scaling=1.0))
    torch.autograd.backward(list(a), [g.to(_dev()) for g in gs])
    leaves2 = [t.clone().requires_grad_(True) for t in (q, k)]
    b = R.apply_qk_norm_rotary(*leaves2, wq, wk, **norm)
    torch.autograd.backward(list(b), [g.to(_dev()) for g in gs])
    assert all(torch.equal(x, y) for x, y in zip((*a, leaves[0].grad, leaves[1].grad), (*b, leaves2[0].grad, leaves2[1].grad)))
    # layout=func == positions=local_positions(func, ...) of the same rank (a group of one rank: 0 .. S-1)
    S = q.shape[1]
    plain = {k_: v for k_, v in kw.items() if k_ not in ("positions", "offset")}
    for f in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        by_map = R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv.to(_dev()), layout=f, offset=7, **plain)
        by_pos = R.apply_qk_norm_rotary_freqs(q, k, wq, wk, inv.to(_dev()), positions=R.local_positions(f, S, device=_dev()),
                                              offset=7, **plain)
        assert torch.equal(by_map[0], by_pos[0]) and torch.equal(by_map[1], by_pos[1])


@pytest.mark.parametrize("kind", ["ring", "zigzag_ring", "stripe"])
@pytest.mark.parametrize("W", [2, 4])
def test_every_ranks_shard_is_the_shard_of_the_single_device_result(single_rank_group, kind, W):
    """rank r of W with its map, as the public call hands it to the backend, and with positions=local_positions(rank=r): both
    are, bit for bit, the shard's rows of the single-device result — forward and dq / dk; three-axis positions too"""
    import ring_flash_attn as R
    from ring_flash_attn._common import pos_map, stripe_map, zigzag_map
    from ring_flash_attn.backend import get_backend

    be, n, B, H, Hk, D = get_backend(), 6, 2, 5, 1, 128
    func = getattr(R, f"{kind}_flash_attn_func")
    dev, bf = _dev(), torch.bfloat16
    q, k, gq, gk = (_randn(B, W * n, h, D, seed=s, dtype=bf).to(dev) for s, h in ((5, H), (6, Hk), (7, H), (8, Hk)))
    wq, wk = (1.0 + 0.25 * _randn(D, seed=s, dtype=torch.float32).to(dev) for s in (3, 4))
    inv = (10000.0 ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2))).float().to(dev)
    thw = torch.randint(0, 10 ** 6, (3, B, W * n), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    kw = dict(interleaved=False, rot_offset=0, eps=1e-6, weight_offset=0.0, scaling=1.25)

    def direct(xs, gs, **pk):
        ys, dxs = ([torch.empty_like(x) for x in xs] for _ in range(2))
        be.qk_norm_freqs_rotary_fwd(xs, ys, [wq, wk], inv, **kw, **pk)
        be.qk_norm_freqs_rotary_bwd(xs, gs, dxs, [wq, wk], [None, None], inv, **kw, **pk)
        return ys + dxs

    whole, whole3 = direct([q, k], [gq, gk]), direct([q, k], [gq, gk], positions=thw, freq_axis=QWEN3_VL)
    for r in range(W):
        pos = R.local_positions(func, n, rank=r, world_size=W, device=dev)
        pm = {"ring": pos_map(r * n), "zigzag_ring": zigzag_map(r, W, n // 2), "stripe": stripe_map(r, W)}[kind]
        sh = lambda t: t.index_select(1, pos.long())
        want = [sh(t) for t in whole]
        assert all(torch.equal(a, b) for a, b in zip(direct([sh(q), sh(k)], [sh(gq), sh(gk)], pos_map=pm), want))
        assert all(torch.equal(a, b) for a, b in zip(direct([sh(q), sh(k)], [sh(gq), sh(gk)], positions=pos), want))
        got3 = direct([sh(q), sh(k)], [sh(gq), sh(gk)], positions=thw.index_select(2, pos.long()).contiguous(), freq_axis=QWEN3_VL)
        assert all(torch.equal(a, b) for a, b in zip(got3, [sh(t) for t in whole3]))
