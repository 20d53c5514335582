"""The MLA rotary kernels on the device (`-m gpu`): csrc/rfa_mlarope.hip through ring_flash_attn.apply_mla_rotary.

B 2, S 38 (a zigzag chunk of 19 rows; 19 tiles of two rows), Hq 3, COMBOS, bf16 / fp16, fp32 / io-dtype tables with a NaN row no
position uses, one packed case of T = 77 (a ragged last tile).  H in 1, 3 and 131.  131: a token's head sum runs on 128 lanes —
two waves — cut into 128 / (Dr / 8) slices (16, 64, 128, 32 for COMBOS' Dr); with 131 heads every Dr has slices that own two or
more heads next to slices that own fewer, the fold walks every slice and both waves' partials meet in LDS: every level of the
reduction is crossed.  Copied columns and whatever apply_rotary also computes are compared BIT FOR BIT; rope columns against fp64:
    |err| <= max(u |ref|, half a subnormal step) + 2^-22 (|x1 c| + |x2 s|),    u = 2^-8 (bf16), 2^-11 (fp16)    (test_gpu_rotary.py)
    dk_pe: 1.01 (max(u |ref|, half step) + (2^-22 + (H - 1) 2^-24) (A1 |c| + A2 |s|)),   A = sum_h |dk[..., h, Dn:]|
— (H - 1) fp32 additions of exactly representable terms on top of the rotation's two products and their sum, one rounding."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

B, S, HQ, P = 2, 38, 3, 80
#          Dn   Dr  Dv   interleaved
COMBOS = [(128, 64, 128, False), (192, 64, 128, False), (8, 16, 8, False), (24, 8, 40, True), (0, 32, 16, True)]
U_OF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HALF_STEP = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}      # half the spacing of the subnormal numbers
DEV = torch.device("cuda:0")


def _tables(Dr, dtype):
    """cos / sin of P positions plus ONE more row that no position uses, filled with NaN"""
    ang = torch.arange(P, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(Dr // 2, dtype=torch.float64) / (Dr // 2)))
    pad = torch.full((1, Dr // 2), float("nan"), dtype=torch.float64)
    return torch.cat([ang.cos(), pad]).to(dtype).to(DEV), torch.cat([ang.sin(), pad]).to(dtype).to(DEV)


def _rand(seed, *shape, dtype):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def _inputs(Dn, Dr, Dv, H, dtype, lead=(B, S), seed=5):
    pos = torch.randint(0, P, lead, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    return (_rand(seed, *lead, HQ, Dn + Dr, dtype=dtype), _rand(seed + 1, *lead, H, Dn + Dv, dtype=dtype),
            _rand(seed + 2, *lead, 1, Dr, dtype=dtype), pos)


def _rope64(x, c, s, inter):
    """the textbook rotation in fp64 of the columns x (.., Dr) by the angles c, s (.., Dr/2), and |x1 c| + |x2 s| per element"""
    x1, x2 = (x[..., 0::2], x[..., 1::2]) if inter else x.chunk(2, -1)
    join = (lambda a, b: torch.stack([a, b], -1).flatten(-2)) if inter else (lambda a, b: torch.cat([a, b], -1))
    return join(x1 * c - x2 * s, x2 * c + x1 * s), join((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs())


def _check(what, got, ref, mag, dtype, products=2.0 ** -22, factor=1.0):
    err = (got.detach().double().cpu() - ref).abs()
    lim = factor * ((U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + products * mag)
    worst = (err - lim).max().item()
    print(f"{what}: max|err| {err.max().item():.3e}, worst err - bound {worst:.3e}")
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    assert worst <= 0, f"{what}: |err| exceeds the bound by {worst:.3e}"


@pytest.mark.parametrize("tables", ["fp32", "io"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H", [1, 3, 131])
@pytest.mark.parametrize("Dn,Dr,Dv,inter", COMBOS)
def test_forward_backward_and_bit_identities(single_rank_group, Dn, Dr, Dv, inter, H, dtype, tables):
    import ring_flash_attn as R
    from ring_flash_attn.backend import get_backend

    assert get_backend().name == "hip" and get_backend().serves_mla_rotary
    cos, sin = _tables(Dr, torch.float32 if tables == "fp32" else dtype)
    q, kv, k_pe, pos = _inputs(Dn, Dr, Dv, H, dtype)
    qa, kva, pea = (t.clone().requires_grad_(True) for t in (q, kv, k_pe))
    qo, k, v = R.apply_mla_rotary(qa, kva, pea, cos, sin, positions=pos, interleaved=inter)
    assert all(t.is_contiguous() for t in (qo, k, v))
    # 1. forward bit identities
    rot = dict(positions=pos, interleaved=inter)
    assert torch.equal(qo, R.apply_rotary(q, None, cos, sin, rot_offset=Dn, **rot))
    assert torch.equal(k[..., :Dn], kv[..., :Dn]) and torch.equal(v, kv[..., Dn:])
    assert torch.equal(k[..., Dn:], R.apply_rotary(k_pe, None, cos, sin, **rot).expand(B, S, H, Dr))
    # 2. the rope columns against fp64
    c, s = (t.double().cpu()[pos.cpu().long()].unsqueeze(2) for t in (cos, sin))        # (B, S, 1, Dr/2), as the kernel reads them
    _check("k rope", k[..., :1, Dn:], *_rope64(k_pe.double().cpu(), c, s, inter), dtype)
    _check("q rope", qo[..., Dn:], *_rope64(q[..., Dn:].double().cpu(), c, s, inter), dtype)
    # 3. backward
    dqo, dk, dv = _rand(11, B, S, HQ, Dn + Dr, dtype=dtype), _rand(12, B, S, H, Dn + Dr, dtype=dtype), _rand(13, B, S, H, Dv, dtype=dtype)
    dq, dkv, dpe = torch.autograd.grad([qo, k, v], [qa, kva, pea], [dqo, dk, dv], retain_graph=True)
    ql = q.clone().requires_grad_(True)
    R.apply_rotary(ql, None, cos, sin, rot_offset=Dn, **rot).backward(dqo)
    assert torch.equal(dq, ql.grad) and torch.equal(dkv, torch.cat([dk[..., :Dn], dv], -1))
    rope = dk[..., Dn:].double().cpu()
    ref, _ = _rope64(rope.sum(2, keepdim=True), c, -s, inter)
    _, mag = _rope64(rope.abs().sum(2, keepdim=True), c.abs(), s.abs(), inter)
    _check("dk_pe", dpe, ref, mag, dtype, products=2.0 ** -22 + (H - 1) * 2.0 ** -24, factor=1.01)
    again = torch.autograd.grad([qo, k, v], [qa, kva, pea], [dqo, dk, dv])
    assert all(torch.equal(a, b) for a, b in zip(again, (dq, dkv, dpe)))


def test_strided_views_inside_poisoned_buffers(single_rank_group):
    """k_pe a column slice of the kv_a_proj output, kv a view with a padded row stride, q a slice of a qkv-like tensor, everything
    around them NaN: the results are those of contiguous copies, bit for bit, and hold no NaN"""
    import ring_flash_attn as R

    Dn, Dr, Dv, H, dtype = 128, 64, 128, 3, torch.bfloat16
    cos, sin = _tables(Dr, torch.float32)
    q, kv, k_pe, pos = _inputs(Dn, Dr, Dv, H, dtype)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    wide, padded, qkv = nan(B, S, 576), nan(B, S, H * (Dn + Dv) + 64), nan(B, S, 2, HQ, Dn + Dr)
    pe_v, kv_v, q_v = wide[..., 512:576], padded[..., :H * (Dn + Dv)].view(B, S, H, Dn + Dv), qkv[:, :, 1]
    for view, x in ((pe_v, k_pe[:, :, 0]), (kv_v, kv), (q_v, q)):
        view.copy_(x)
    want = R.apply_mla_rotary(q, kv, k_pe, cos, sin, positions=pos)
    for pe in (pe_v, pe_v.unsqueeze(2)):
        got = R.apply_mla_rotary(q_v, kv_v, pe, cos, sin, positions=pos)
        assert all(torch.equal(g, w) and not torch.isnan(g).any() for g, w in zip(got, want))


@pytest.mark.parametrize("Dn,Dr,Dv,inter", [COMBOS[1], COMBOS[3]])
def test_map_mode_no_q_and_packed_input(single_rank_group, Dn, Dr, Dv, inter):
    import ring_flash_attn as R
    from ring_flash_attn._common import zigzag_map
    from ring_flash_attn.backend import get_backend

    H, dtype = 3, torch.float16
    cos, sin = _tables(Dr, torch.float32)
    q, kv, k_pe, pos = _inputs(Dn, Dr, Dv, H, dtype)
    # a two-piece map == explicit positions of the same values: rank 1 of a 2-rank zigzag (chunks 1 and 2 of 19 rows)
    zz = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=1, world_size=2, device=DEV)
    want = R.apply_mla_rotary(q, kv, k_pe, cos, sin, positions=zz, interleaved=inter)
    got = [torch.empty_like(t) for t in want]
    get_backend().mla_rotary_fwd(q, got[0], kv, k_pe, got[1], got[2], cos, sin, nope_dim=Dn, pos_map=zigzag_map(1, 2, S // 2),
                                 interleaved=inter)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # the public `layout` on a one-rank group with an offset == the positions it stands for
    ar = torch.arange(S, dtype=torch.int32, device=DEV)
    for f in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
        a = R.apply_mla_rotary(q, kv, k_pe, cos, sin, layout=f, offset=5, interleaved=inter)
        assert all(torch.equal(x, y) for x, y in zip(a, R.apply_mla_rotary(q, kv, k_pe, cos, sin, positions=ar, offset=5, interleaved=inter)))
    # without q: the same k and v
    none, k, v = R.apply_mla_rotary(None, kv, k_pe, cos, sin, nope_dim=Dn, positions=zz, interleaved=inter)
    assert none is None and torch.equal(k, want[1]) and torch.equal(v, want[2])
    # packed (T, H, D) is the (1, T, H, D) call, and its last tile is ragged
    T = 77
    qp, kvp, pep, posp = _inputs(Dn, Dr, Dv, H, dtype, lead=(T,))
    leaves = [t.clone().requires_grad_(True) for t in (qp, kvp, pep[:, 0])]
    outs = R.apply_mla_rotary(*leaves, cos, sin, positions=posp, interleaved=inter)
    assert torch.equal(outs[0], R.apply_rotary(qp, None, cos, sin, positions=posp, rot_offset=Dn, interleaved=inter))
    l4 = [t.detach().unsqueeze(0).requires_grad_(True) for t in leaves]
    outs4 = R.apply_mla_rotary(*l4, cos, sin, positions=posp.view(1, T), interleaved=inter)
    assert all(torch.equal(a, b[0]) for a, b in zip(outs, outs4))
    gs = [_rand(31 + n, *t.shape, dtype=dtype) for n, t in enumerate(outs)]
    g3, g4 = torch.autograd.grad(outs, leaves, gs), torch.autograd.grad(outs4, l4, [g.unsqueeze(0) for g in gs])
    assert all(torch.equal(a, b[0]) for a, b in zip(g3, g4)) and g3[2].shape == (T, Dr)
