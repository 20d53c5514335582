"""The token-wide QK RMSNorm + rotary kernels that form their own angles, on the device (`-m gpu`): csrc/rfa_qktokenfreq.hip
through ring_flash_attn.apply_qk_token_norm_rotary_freqs, against fp64 autograd of the textbook formula.

Reference angle, as tests/test_gpu_qk_norm_freqs.py forms it: float32(pos) * inv_freq in torch fp32, then cos / sin in fp64,
times the fp32 scaling.  Bounds: the sum of the two derived bounds the project states (e = 2^-24; u = 2^-8 bf16 / 2^-11 fp16; `half`
the io dtype's half subnormal step; k = 4 ulp for sincosf, ka = (2 k + 1) e: c', s' within k ulp and one rounding by the scaling):
    forward  |err| <= max(u |ref|, half) + ((n_ss/2 + 10) e + ka) Mf,        Mf = 2 max_row |ref|
    dx       |err| <= max(u |ref|, half) + ((2.5 n_ss + 20) e + ka) Mb,      Mb = rstd G A (1 + max_row |xh|)
    dw       |err| <= ((n_dw + n_ss/2 + 8) e + ka) T (+ u |ref| for an io-dtype weight),   T_c = sum_rows G |xh_c|
the first summand of each tests/test_gpu_qk_token_norm.py's (norm, scale, rot(), dw; its derivation stands there), the second
the angle's share on the SAME magnitudes with |c'| = |s'| = scaling: a pair rotated by (c', s') of length `scaling` has
|y1 c'| + |y2 s'| <= scaling (|y1| + |y2|) <= 2 max_row |ref|, and G = 2 max(1, scaling) max_row |dout| >= |g|.
n_ss = 8 K + 6 + (team/64 - 1) and n_dw = walk + slots + ceil(nparts/8) + 8 from SUMMATION ORDERS in csrc/rfa_qktokenfreq.hip.
Measured worst err / bound: profiles/qk_token_norm_freqs.md.
(H, Hk, D): (1,1,8) one chunk; (3,1,40) a partly filled wave; (4,2,128) q fills one wave exactly, k half of it; (40,8,128) q on 4
waves and k on 1 in one launch; (64,8,256) the 16384 limit, 8 chunks a lane; (3,1,40) x 2100 rows: 512 partials, a walk of 2, a
ragged last step; (2,1,256) with R = 256: one wave forms 128 angles, two per lane."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
U_OF = {BF: 2.0 ** -8, HF: 2.0 ** -11}
HALF_STEP = {BF: 2.0 ** -134, HF: 2.0 ** -25}
E, KA = 2.0 ** -24, (2 * 4 + 1) * 2.0 ** -24
_axes = lambda half: [c % 3 for c in range(half)]                # t h w t h w ..: an interleaved three-axis map


#   id            H  Hk  D   dtype R   ro inter aux woff eps  scaling positions lead
CASES = {
    "one-chunk": (1, 1, 8, BF, 8, 0, True, F32, 0.0, 1e-6, 1.0, "row", (2, 37)),
    "part-wave": (3, 1, 40, HF, 16, 8, False, HF, 1.0, 0.0, 1.25, "batch", (2, 37)),
    "one-wave-map-1e6": (4, 2, 128, BF, 128, 0, False, F32, 0.0, 1e-6, 1.0, "map", (2, 37)),
    "four-waves-thw": (40, 8, 128, BF, 64, 32, False, BF, 0.0, 0.0, 1.0, "thw", (2, 37)),
    "limit-interleaved": (64, 8, 256, HF, 256, 0, True, F32, 1.0, 1e-6, 0.75, "batch", (2, 37)),
    "walk-of-two": (3, 1, 40, BF, 32, 0, False, F32, 0.0, 1e-6, 1.0, "map", (1, 2100)),
    "two-angles-a-lane-packed-q-alone": (2, None, 256, BF, 256, 0, False, F32, 0.0, 1e-6, 1.0, "thw", (74,)),
}


def _rand(shape, dtype, seed, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(dtype).to(DEV)


def _inputs(name):
    """(q, k, wq, wk, dq, dk) on the device (q alone: k, wk, dk None), inv_freq, the call's keywords, the reference's (B, S, R/2) positions"""
    H, Hk, D, dt, Rw, ro, inter, aux, woff, eps, scaling, mode, lead = CASES[name]
    aux = dt if aux in (BF, HF) else F32
    q, dq = _rand((*lead, H, D), dt, 5), _rand((*lead, H, D), dt, 7)
    k, dk = (None, None) if Hk is None else (_rand((*lead, Hk, D), dt, 6), _rand((*lead, Hk, D), dt, 8))
    wq = _rand((H * D,), aux, 4, 0.25, 1.0 - woff)
    wk = None if Hk is None else _rand((Hk, D), aux, 9, 0.25, 1.0 - woff)
    half = Rw // 2
    inv = (10000.0 ** (-torch.arange(half, dtype=torch.float64) / half)).float()
    kw = dict(eps=eps, weight_offset=woff, attention_scaling=scaling, interleaved=inter, rot_offset=ro)
    rows, g = ((1, *lead) if len(lead) == 1 else lead), torch.Generator().manual_seed(11)
    if mode == "map":                                              # row i at 10^6 - 3 + i: no tensor
        kw["offset"] = 10 ** 6 - 3
        pos = (kw["offset"] + torch.arange(rows[1])).expand(rows).unsqueeze(-1).expand(*rows, half)
    elif mode == "thw":                                            # (3, B, S) / packed (3, T), frequency c reads axis c % 3
        p3 = torch.randint(0, 10 ** 6, (3, *rows), generator=g)
        kw["positions"], kw["freq_axis"] = p3.view(3, *lead).to(torch.int32).to(DEV), _axes(half)
        pos = p3[torch.tensor(_axes(half))].permute(1, 2, 0)
    else:                                                          # (S,) shared by the batch entries, or (B, S)
        p = torch.randint(0, 10 ** 6, (rows[1],) if mode == "row" else rows, generator=g)
        kw["positions"] = p.to(torch.int32).to(DEV)
        pos = p.expand(rows).unsqueeze(-1).expand(*rows, half)
    return (q, k, wq, wk, dq, dk), inv, kw, pos


def _textbook(x, w, c, s, inter, ro, eps, woff):                    # x (B, S, H, D), w (H, D), c / s (B, S, 1, R/2); fp64
    y = x * torch.rsqrt(x.pow(2).mean((-2, -1), keepdim=True) + eps) * (woff + w)
    R = 2 * c.shape[-1]
    r = y[..., ro:ro + R]
    x1, x2 = (r[..., 0::2], r[..., 1::2]) if inter else (r[..., :R // 2], r[..., R // 2:])
    o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
    rot = torch.stack([o1, o2], -1).flatten(-2) if inter else torch.cat([o1, o2], -1)
    return torch.cat([y[..., :ro], rot, y[..., ro + R:]], -1)


def _chains(N, rows):
    team = 64 if N <= 1024 else (128 if N <= 4096 else 256)
    slots = 256 // team
    nparts = min(-(-rows // slots), 512)
    return 8 * -(-N // (8 * team)) + 6 + team // 64 - 1, -(-rows // (nparts * slots)) + slots + -(-nparts // 8) + 8


def _check(what, x, w, dout, got, gdx, gdw, inv, pos, inter, ro, eps, woff, scaling):
    dt, (H, D), (B, S) = x.dtype, x.shape[-2:], pos.shape[:2]
    n_ss, n_dw = _chains(H * D, B * S)
    ang32 = pos.float() * inv                                      # torch fp32, one rounded multiply
    s32 = torch.tensor(scaling, dtype=F32).double()
    c, s = (ang32.double().cos() * s32).unsqueeze(2), (ang32.double().sin() * s32).unsqueeze(2)
    x64, d64 = x.double().cpu().view(B, S, H, D).requires_grad_(True), dout.double().cpu().view(B, S, H, D)
    w64 = w.double().cpu().view(H, D).requires_grad_(True)
    ref = _textbook(x64, w64, c, s, inter, ro, eps, woff)
    ref.backward(d64)
    ref = ref.detach()
    rowmax = lambda t: t.abs().amax((-2, -1), keepdim=True)
    rstd = torch.rsqrt(x64.detach().pow(2).mean((-2, -1), keepdim=True) + eps)
    xh, G = x64.detach().abs() * rstd, 2 * max(1.0, float(s32)) * rowmax(d64)
    io = lambda r, t: (U_OF[t] * r.abs()).clamp(min=HALF_STEP[t])
    lims = [("fwd", got, ref, io(ref, dt) + ((n_ss / 2 + 10) * E + KA) * 2 * rowmax(ref)),
            ("dx", gdx, x64.grad, io(x64.grad, dt) + ((2.5 * n_ss + 20) * E + KA) * rstd * G * (woff + w64.detach()).abs().max() * (1 + rowmax(xh))),
            ("dw", gdw, w64.grad, ((n_dw + n_ss / 2 + 8) * E + KA) * (G * xh).reshape(-1, H, D).sum(0) +
             (io(w64.grad, w.dtype) if w.dtype != F32 else 0))]
    for name, g, r, lim in lims:
        err = (g.detach().double().cpu().view(r.shape) - r).abs()
        print(f"{what} {name}: max|err| {err.max().item():.3e}, worst err / bound {(err / lim).max().item():.4f}")
        assert not torch.isnan(g).any() and bool((err <= lim).all()), f"{what} {name}: {(err - lim).max().item():.3e} over the bound"


def _run(q, k, wq, wk, dq, dk, inv, **kw):
    import ring_flash_attn as R                # the public call (inv None: the table call's norm alone): ([outs], [dx], [dw])
    ls = [t.clone().requires_grad_(True) for t in (q, k, wq, wk) if t is not None]
    n = len(ls) // 2
    qkw = (ls[0], ls[1] if n == 2 else None, ls[n], ls[n + 1] if n == 2 else None)
    outs = R.apply_qk_token_norm_rotary(*qkw, **kw) if inv is None else R.apply_qk_token_norm_rotary_freqs(*qkw, inv.to(DEV), **kw)
    outs = outs if n == 2 else (outs,)
    torch.autograd.backward(list(outs), [dq, dk][:n])
    return [o.detach() for o in outs], [t.grad for t in ls[:n]], [t.grad for t in ls[n:]]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(sum(a, []), sum(b, [])))


@pytest.mark.parametrize("name", list(CASES))
def test_forward_dx_dw_against_fp64_and_the_bit_identities(name):
    from ring_flash_attn.backend import get_backend

    assert get_backend().name == "hip" and get_backend().serves_qk_token_norm_freqs
    H, Hk, D, dt, Rw, ro, inter, aux, woff, eps, scaling, mode, lead = CASES[name]
    ts, inv, kw, pos = _inputs(name)
    q, k, wq, wk, dq, dk = ts
    res = _run(*ts, inv, **kw)
    for i, (t, x, w, d) in enumerate((("q", q, wq, dq), ("k", k, wk, dk))[:1 if k is None else 2]):
        assert res[2][i].dtype == w.dtype and res[2][i].shape == w.shape and res[0][i].is_contiguous()
        _check(f"{name} {t}", x, w, d, res[0][i], res[1][i], res[2][i], inv, pos, inter, ro, eps, woff, scaling)
    assert _same(_run(*ts, inv, **kw), res)                                              # two runs, dw included
    if k is not None:                                                                    # q does not see whether k rode along
        assert _same(_run(q, None, wq, None, dq, None, inv, **kw), [r[:1] for r in res])
    # inv_freq = 0 with scaling 1: every angle 0, the bits of the table kernel's norm alone — out, dx and dw
    assert _same(_run(*ts, torch.zeros_like(inv), **dict(kw, attention_scaling=1.0)), _run(*ts, None, eps=eps, weight_offset=woff))
    if mode == "map":                                              # the map's positions as an (S,) tensor: the same bits
        as_tensor = (kw["offset"] + torch.arange(lead[-1])).to(torch.int32).to(DEV)
        assert _same(_run(*ts, inv, **dict(kw, offset=0, positions=as_tensor)), res)


@pytest.mark.parametrize("kind", ["ring", "zigzag_ring", "stripe"])
def test_every_ranks_shard_is_the_shard_of_the_single_device_result(kind):
    """W = 2, H D = 1280 (two waves a row) and 256: rank r with its map — what `layout=` hands to the backend — and with
    positions=local_positions(rank=r) through the public call both give rank r's rows of the single call, bit for bit"""
    import ring_flash_attn as R
    from ring_flash_attn._common import pos_map, stripe_map, zigzag_map
    from ring_flash_attn.backend import get_backend

    be, W, n, func = get_backend(), 2, 8, getattr(R, f"{kind}_flash_attn_func")
    q, k, dq, dk = (_rand((2, W * n, h, 64), BF, s) for s, h in ((5, 20), (6, 4), (7, 20), (8, 4)))
    wq, wk = _rand((20, 64), F32, 4, 0.25, 1.0), _rand((256,), F32, 9, 0.25, 1.0)
    inv = (10000.0 ** (-torch.arange(16, dtype=torch.float64) / 16)).float().to(DEV)
    kw = dict(rot_offset=16, attention_scaling=1.25)
    full = _run(q, k, wq, wk, dq, dk, inv, **kw)

    def direct(xs, gs, pm):
        ys, dxs = ([torch.empty_like(x) for x in xs] for _ in range(2))
        lk = dict(pos_map=pm, rot_offset=16, scaling=1.25, eps=1e-6, weight_offset=0.0)
        be.qk_token_norm_freqs_rotary_fwd(xs, ys, [wq, wk], inv, **lk)
        be.qk_token_norm_freqs_rotary_bwd(xs, gs, dxs, [wq, wk], [None, None], inv, **lk)
        return [ys, dxs]

    for r in range(W):
        pos = R.local_positions(func, n, rank=r, world_size=W, device=DEV)
        pm = {"ring": pos_map(r * n), "zigzag_ring": zigzag_map(r, W, n // 2), "stripe": stripe_map(r, W)}[kind]
        sh = lambda t: t.index_select(1, pos.long())
        want = [[sh(t) for t in part] for part in full[:2]]
        assert _same(_run(sh(q), sh(k), wq, wk, sh(dq), sh(dk), inv, positions=pos, **kw)[:2], want)
        assert _same(direct([sh(q), sh(k)], [sh(dq), sh(dk)], pm), want)
