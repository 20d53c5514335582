"""The token-wide QK RMSNorm + rotary kernels on the device (`-m gpu`): csrc/rfa_qktoken.hip through
ring_flash_attn.apply_qk_token_norm_rotary, against fp64 autograd of the textbook formula (`_textbook`).

Bounds, derived from SUMMATION ORDERS in csrc/rfa_qktoken.hip (e = 2^-24; u = 2^-8 bf16 / 2^-11 fp16; `half` the io dtype's half
subnormal step).  A row of N = H D columns is summed in n_ss = 8 K + 6 + (team/64 - 1) roundings (K chunks per lane, the wave's
butterfly, the team's waves), all terms positive, so rstd = rsqrt(ss/N + eps) carries at most r = n_ss/2 + 3 relative e.
    forward  a (1), y = (x rstd) a (2), rot (3):  |err| <= max(u |ref|, half) + (n_ss/2 + 10) e Mf,
             Mf = |y1 c| + |y2 s| <= |y1| + |y2| <= 2 max_row |ref|   (a rotation keeps a pair's length)
    dx = rstd (g a - xh m): g a carries 5 e, xh r + 1, m = sum(g a xh)/N n_ss + r + 8, the fma and rstd r + 2:
             |err| <= max(u |ref|, half) + (2.5 n_ss + 20) e Mb,  Mb = rstd G A (1 + max_row |xh|),
             G = 2 max_row |dout| >= |g|mag, A = max |a|  (and mean_row |xh| <= 1)
    dw       |err| <= (n_dw + n_ss/2 + 8) e T (+ u |ref| for an io-dtype weight),  T_c = sum_rows G |xh_c|,
             n_dw = walk + slots + ceil(nparts/8) + 8, the longest chain of the partials' sum
Measured worst err / bound: profiles/qk_token_norm.md.
(H, Hk, D): (1,1,8) one chunk; (3,1,40) 15 chunks, a partly filled wave; (4,2,128) q fills one wave's 64 lanes exactly, k half of
them; (5,5,64); (40,8,128) q on 4 waves, k on 1, in one launch; (64,8,256) the 16384 limit, 8 chunks a lane."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _droppos_worker import PREFIX, shard                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
U_OF = {BF: 2.0 ** -8, HF: 2.0 ** -11}
HALF_STEP = {BF: 2.0 ** -134, HF: 2.0 ** -25}
E = 2.0 ** -24
P = 80


def _textbook(x, w, cos, sin, pos, inter, ro, eps, woff):            # x (.., H, D), w (H, D); differentiable, any dtype
    y = x * torch.rsqrt(x.pow(2).mean((-2, -1), keepdim=True) + eps) * (woff + w)
    if cos is None:
        return y
    R = 2 * cos.shape[1]
    c, s, r = cos[pos].unsqueeze(-2), sin[pos].unsqueeze(-2), y[..., ro:ro + R]
    x1, x2 = (r[..., 0::2], r[..., 1::2]) if inter else (r[..., :R // 2], r[..., R // 2:])
    o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
    rot = torch.stack([o1, o2], -1).flatten(-2) if inter else torch.cat([o1, o2], -1)
    return torch.cat([y[..., :ro], rot, y[..., ro + R:]], -1)


def _chains(N, rows):
    team = 64 if N <= 1024 else (128 if N <= 4096 else 256)
    slots = 256 // team
    nparts = min(-(-rows // slots), 512)
    return 8 * -(-N // (8 * team)) + 6 + team // 64 - 1, -(-rows // (nparts * slots)) + slots + -(-nparts // 8) + 8


def _tables(R, dtype, rows=P):
    ang = torch.arange(rows, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(R // 2, dtype=torch.float64) / (R // 2)))
    return ang.cos().to(dtype).to(DEV), ang.sin().to(dtype).to(DEV)


def _rand(shape, dtype, seed, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(dtype).to(DEV)


def _check(what, x, w, dout, got, gdx, gdw, cos, sin, pos, inter, ro, eps, woff):
    # forward, dx and dw of one tensor against fp64 autograd within the module's bounds; prints worst err / bound
    dt, (H, D), rows = x.dtype, x.shape[-2:], x.numel() // (x.shape[-2] * x.shape[-1])
    n_ss, n_dw = _chains(H * D, rows)
    x64, w64 = x.double().cpu().requires_grad_(True), w.double().cpu().view(H, D).requires_grad_(True)
    c64, s64 = (None, None) if cos is None else (cos.double().cpu(), sin.double().cpu())
    ref = _textbook(x64, w64, c64, s64, None if pos is None else pos.cpu().long(), inter, ro, eps, woff)
    ref.backward(dout.double().cpu())
    ref = ref.detach()
    rowmax = lambda t: t.abs().amax((-2, -1), keepdim=True)
    rstd = torch.rsqrt(x64.detach().pow(2).mean((-2, -1), keepdim=True) + eps)
    xh, G = x64.detach().abs() * rstd, 2 * rowmax(dout.double().cpu())
    io = lambda r, t: (U_OF[t] * r.abs()).clamp(min=HALF_STEP[t])
    lims = [("fwd", got, ref, io(ref, dt) + (n_ss / 2 + 10) * E * 2 * rowmax(ref)),
            ("dx", gdx, x64.grad, io(x64.grad, dt) + (2.5 * n_ss + 20) * E * rstd * G * (woff + w64.detach()).abs().max() * (1 + rowmax(xh))),
            ("dw", gdw.view(H, D), w64.grad, (n_dw + n_ss / 2 + 8) * E * (G * xh).reshape(-1, H, D).sum(0) +
             (io(w64.grad, w.dtype) if w.dtype != F32 else 0))]
    for name, g, r, lim in lims:
        err = (g.detach().double().cpu() - r).abs()
        print(f"{what} {name}: max|err| {err.max().item():.3e}, worst err / bound {(err / lim).max().item():.4f}")
        assert not torch.isnan(g).any() and bool((err <= lim).all()), f"{what} {name}: {(err - lim).max().item():.3e} over the bound"


def _run(q, k, wq, wk, cos, sin, dq, dk, **kw):
    import ring_flash_attn as R                                  # the public call, forward and backward: ([outs], [dx], [dw])
    ls = [t.clone().requires_grad_(True) for t in (q, k, wq, wk) if t is not None]
    n = len(ls) // 2
    outs = R.apply_qk_token_norm_rotary(ls[0], ls[1] if n == 2 else None, ls[n], ls[n + 1] if n == 2 else None, cos, sin, **kw)
    outs = outs if n == 2 else (outs,)
    torch.autograd.backward(list(outs), [dq, dk][:n])
    return [o.detach() for o in outs], [t.grad for t in ls[:n]], [t.grad for t in ls[n:]]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(sum(a, []), sum(b, [])))


#        H  Hk  D    dtype R   ro inter aux  woff eps   lead
CASES = [(1, 1, 8, BF, 8, 0, True, F32, 0.0, 1e-6, (2, 37)), (3, 1, 40, HF, 16, 8, False, HF, 1.0, 0.0, (2, 37)),
         (4, 2, 128, BF, 128, 0, False, F32, 0.0, 1e-6, (2, 37)), (5, 5, 64, HF, 0, 0, False, F32, 1.0, 1e-6, (2, 37)),
         (40, 8, 128, BF, 64, 32, False, BF, 0.0, 0.0, (2, 37)), (40, 8, 128, HF, 128, 0, True, F32, 1.0, 1e-6, (2, 37)),
         (64, 8, 256, BF, 256, 0, False, F32, 0.0, 1e-6, (2, 37)),
         (3, 1, 40, BF, 32, 0, False, F32, 0.0, 1e-6, (1, 2100))]       # q: 512 partials, a walk of 2, the last step ragged


@pytest.mark.parametrize("H,Hk,D,dt,Rw,ro,inter,aux,woff,eps,lead", CASES)
def test_forward_dx_dw_against_fp64_and_the_bit_identities(H, Hk, D, dt, Rw, ro, inter, aux, woff, eps, lead):
    aux = dt if aux in (BF, HF) else F32
    cos, sin = _tables(Rw, aux, max(P, lead[1])) if Rw else (None, None)
    pos = torch.randint(0, P, lead, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV) if Rw else None
    q, k, dq, dk = (_rand((*lead, h, D), dt, s) for s, h in ((5, H), (6, Hk), (7, H), (8, Hk)))
    wq, wk = _rand((H * D,), aux, 4, 0.25, 1.0 - woff), _rand((Hk, D), aux, 9, 0.25, 1.0 - woff)
    q[1 % lead[0], 3] = 0                                        # an all-zero token row: eps > 0 gives zeros, never NaN
    kw = dict(positions=pos, interleaved=inter, rot_offset=ro, eps=eps, weight_offset=woff)
    if eps == 0:
        q[1 % lead[0], 3, 0, 0] = 1.0
    res = _run(q, k, wq, wk, cos, sin, dq, dk, **kw)
    assert eps == 0 or bool((res[0][0][1 % lead[0], 3] == 0).all())
    for i, (name, x, w, d) in enumerate((("q", q, wq, dq), ("k", k, wk, dk))):
        assert res[2][i].dtype == w.dtype and res[2][i].shape == w.shape
        _check(f"{name} {H}x{Hk}x{D}", x, w, d, res[0][i], res[1][i], res[2][i], cos, sin, pos, inter, ro, eps, woff)
    assert _same(_run(q, k, wq, wk, cos, sin, dq, dk, **kw), res)                       # two runs, dw included
    alone = _run(q, None, wq, None, cos, sin, dq, None, **kw)                           # k=None == q with k riding along
    assert _same(alone, [r[:1] for r in res])
    # the same rows through other strides: slices of one qkv tensor (and of its gradient), taken as they are
    from ring_flash_attn.rotary import _conforms
    qkv, dqkv = (torch.empty(*lead, H + 2 * Hk, D, dtype=dt, device=DEV) for _ in range(2))
    qkv[..., :H, :], qkv[..., H:H + Hk, :], dqkv[..., :H, :], dqkv[..., H:H + Hk, :] = q, k, dq, dk
    assert _conforms(qkv[..., H:H + Hk, :]) and not qkv[..., :H, :].is_contiguous()
    assert _same(_run(qkv[..., :H, :], qkv[..., H:H + Hk, :], wq, wk, cos, sin, dqkv[..., :H, :], dqkv[..., H:H + Hk, :], **kw), res)
    if Rw:                                                       # tables of cos 1 / sin 0 == the norm-only call
        unit = _run(q, k, wq, wk, torch.ones_like(cos), torch.zeros_like(sin), dq, dk, **kw)
        assert _same(unit, _run(q, k, wq, wk, None, None, dq, dk, eps=eps, weight_offset=woff))
        # packed (T, H, D) with (T,) positions is the same call
        flat = lambda t: t.reshape(-1, *t.shape[2:])
        packed = _run(flat(q), flat(k), wq, wk, cos, sin, flat(dq), flat(dk), **dict(kw, positions=pos.reshape(-1)))
        assert _same([[flat(t) for t in r] for r in res[:2]] + [res[2]], packed)


def test_a_weight_without_grad_and_a_none_gradient():
    import ring_flash_attn as R

    q, k, dk = (_rand((2, 37, h, 64), BF, s) for s, h in ((5, 20), (6, 4), (8, 4)))
    wq, wk = _rand((1280,), F32, 4, 0.25, 1.0), _rand((256,), F32, 9, 0.25, 1.0).requires_grad_(True)
    cos, sin = _tables(64, F32)
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    qo, ko = R.apply_qk_token_norm_rotary(ql, kl, wq, wk, cos, sin)
    ko.backward(dk)                                              # q's incoming gradient is None, w_q needs none
    want = _run(k, None, wk.detach(), None, cos, sin, dk, None)
    assert ql.grad is None and wq.grad is None and torch.equal(kl.grad, want[1][0]) and torch.equal(wk.grad, want[2][0])
    assert torch.equal(ko, want[0][0])


@pytest.mark.parametrize("kind", ["ring", "zigzag", "stripe"])
@pytest.mark.parametrize("W", [2, 4])
def test_every_ranks_shard_is_the_shard_of_the_single_device_result(kind, W):
    """H D = 1280 (two waves a row): the call on rank r's rows with positions=local_positions(..) equals, bit for bit, rank r's
    rows of the call on the full tensor with natural positions"""
    import ring_flash_attn as R

    func, n = getattr(R, PREFIX[kind] + "_func"), 8
    q, k, dq, dk = (_rand((2, W * n, h, 64), BF, s) for s, h in ((5, 20), (6, 4), (7, 20), (8, 4)))
    wq, wk = _rand((20, 64), F32, 4, 0.25, 1.0), _rand((256,), F32, 9, 0.25, 1.0)
    cos, sin = _tables(32, F32, W * n)
    full = _run(q, k, wq, wk, cos, sin, dq, dk, rot_offset=16)
    for r in range(W):
        pos = R.local_positions(func, n, rank=r, world_size=W, device=DEV)
        sh = lambda t: shard(kind, t.cpu(), r, W).to(DEV)
        mine = _run(sh(q), sh(k), wq, wk, cos, sin, sh(dq), sh(dk), positions=pos, rot_offset=16)
        assert _same(mine[:2], [[sh(t) for t in part] for part in full[:2]])
