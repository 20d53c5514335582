"""The MLA rotary kernels that form their own angles, on the device (`-m gpu`): csrc/rfa_mlaropefreq.hip through
ring_flash_attn.apply_mla_rotary_freqs.

test_gpu_mla_rotary.py's shapes (B 2, S 38, Hq 3, COMBOS, H in 1, 3 and 131 — every level of the head sum is crossed; bf16 / fp16)
with int32 positions in [0, 2^20), one of them 0 and one 2^31 - 1 (the range reduction is crossed), and two scalings.  Whatever
apply_rotary_freqs also computes, and every copied column, is compared BIT FOR BIT.  dk_pe against fp64: the fp64 head sum rotated
by the fp64 cos / sin of the kernel's own fp32 angle fl32(float(pos) * inv_freq[c]), times the fp32 scaling;
    |err| <= 1.01 (max(u |ref|, half step) + (2^-22 + (H - 1) 2^-24) (A1 |c'| + A2 |s'|)        test_gpu_mla_rotary.py's bound
                   + (A1 + A2) scaling (2 k + 1) 2^-24),     A = sum_h |dk[..., h, Dn:]|
— the last term is what c' and s' themselves are off by: sincosf within k = 4 ulp of values <= 1 for each of them (2 k; K_ULP of
test_gpu_rotary_freqs.py) and the one rounding of the scaling multiply (1); the two roundings of rot(), which that file counts in
its 2 k + 3, are in the 2^-22 here."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_mla_rotary import B, COMBOS, DEV, HALF_STEP, HQ, S, U_OF, _rand, _rope64  # noqa: E402
from test_gpu_rotary_freqs import K_ULP, _inv_freq  # noqa: E402

pytestmark = pytest.mark.gpu

SCALINGS = [1.0, 0.1 * math.log(40) + 1]


def _inputs(Dn, Dr, Dv, H, dtype, lead=(B, S), seed=5):
    pos = torch.randint(0, 2 ** 20, lead, generator=torch.Generator().manual_seed(3))
    pos.view(-1)[1], pos.view(-1)[-2] = 0, 2 ** 31 - 1
    return (_rand(seed, *lead, HQ, Dn + Dr, dtype=dtype), _rand(seed + 1, *lead, H, Dn + Dv, dtype=dtype),
            _rand(seed + 2, *lead, 1, Dr, dtype=dtype), pos.to(torch.int32).to(DEV))


@pytest.mark.parametrize("scaling", SCALINGS, ids=["x1", "yarn"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H", [1, 3, 131])
@pytest.mark.parametrize("Dn,Dr,Dv,inter", COMBOS)
def test_forward_backward_and_bit_identities(single_rank_group, Dn, Dr, Dv, inter, H, dtype, scaling):
    import ring_flash_attn as R
    from ring_flash_attn.backend import get_backend

    assert get_backend().name == "hip" and get_backend().serves_mla_rotary_freqs
    inv_freq = _inv_freq(Dr)
    q, kv, k_pe, pos = _inputs(Dn, Dr, Dv, H, dtype)
    qa, kva, pea = (t.clone().requires_grad_(True) for t in (q, kv, k_pe))
    rot = dict(attention_scaling=scaling, positions=pos, interleaved=inter)
    qo, k, v = R.apply_mla_rotary_freqs(qa, kva, pea, inv_freq, **rot)
    assert all(t.is_contiguous() for t in (qo, k, v))
    # 1. forward bit identities
    assert torch.equal(qo, R.apply_rotary_freqs(q, None, inv_freq, rot_offset=Dn, **rot))
    assert torch.equal(k[..., :Dn], kv[..., :Dn]) and torch.equal(v, kv[..., Dn:])
    assert torch.equal(k[..., Dn:], R.apply_rotary_freqs(k_pe, None, inv_freq, **rot).expand(B, S, H, Dr))
    # 2. backward: dq and dkv bit for bit, dk_pe against fp64, a second run bit for bit
    dqo, dk, dv = _rand(11, B, S, HQ, Dn + Dr, dtype=dtype), _rand(12, B, S, H, Dn + Dr, dtype=dtype), _rand(13, B, S, H, Dv, dtype=dtype)
    dq, dkv, dpe = torch.autograd.grad([qo, k, v], [qa, kva, pea], [dqo, dk, dv], retain_graph=True)
    ql = q.clone().requires_grad_(True)
    R.apply_rotary_freqs(ql, None, inv_freq, rot_offset=Dn, **rot).backward(dqo)
    assert torch.equal(dq, ql.grad) and torch.equal(dkv, torch.cat([dk[..., :Dn], dv], -1))
    ang32 = (pos.cpu().float().unsqueeze(-1) * inv_freq.cpu()).double().unsqueeze(2)         # (B, S, 1, Dr/2), the kernel's angle
    s32 = torch.tensor(scaling, dtype=torch.float32).double()
    c, s = ang32.cos() * s32, ang32.sin() * s32
    rope = dk[..., Dn:].double().cpu()
    ref, _ = _rope64(rope.sum(2, keepdim=True), c, -s, inter)
    A = rope.abs().sum(2, keepdim=True)
    _, mag = _rope64(A, c.abs(), s.abs(), inter)
    _, pair = _rope64(A, torch.ones_like(c), torch.ones_like(s), inter)                      # A1 + A2 of every element's pair
    bound = 1.01 * ((U_OF[dtype] * ref.abs()).clamp(min=HALF_STEP[dtype]) + (2.0 ** -22 + (H - 1) * 2.0 ** -24) * mag +
                    pair * float(s32) * (2 * K_ULP + 1) * 2.0 ** -24)
    frac = ((dpe.double().cpu() - ref).abs() / bound).max().item()
    print(f"dk_pe: worst |err| / bound {frac:.3f}")
    assert not torch.isnan(dpe).any() and frac <= 1.0, f"dk_pe: |err| is {frac:.3f} of the bound"
    again = torch.autograd.grad([qo, k, v], [qa, kva, pea], [dqo, dk, dv])
    assert all(torch.equal(a, b) for a, b in zip(again, (dq, dkv, dpe)))


@pytest.mark.parametrize("Dn,Dr,Dv,inter", [COMBOS[1], COMBOS[3]])
def test_strided_views_map_mode_no_q_and_packed_input(single_rank_group, Dn, Dr, Dv, inter):
    import ring_flash_attn as R
    from ring_flash_attn._common import zigzag_map
    from ring_flash_attn.backend import get_backend

    H, dtype, inv_freq = 3, torch.bfloat16, _inv_freq(Dr)
    kw = dict(attention_scaling=SCALINGS[1], interleaved=inter)
    q, kv, k_pe, pos = _inputs(Dn, Dr, Dv, H, dtype)
    # strided views inside NaN-filled buffers: k_pe a column slice of a 576-wide row, kv with a padded row stride, q a slice of
    # a qkv-like tensor — the contiguous call's bits, and no NaN
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    wide, padded, qkv = nan(B, S, 576), nan(B, S, H * (Dn + Dv) + 64), nan(B, S, 2, HQ, Dn + Dr)
    pe_v, kv_v, q_v = wide[..., 576 - Dr:], padded[..., :H * (Dn + Dv)].view(B, S, H, Dn + Dv), qkv[:, :, 1]
    for view, x in ((pe_v, k_pe[:, :, 0]), (kv_v, kv), (q_v, q)):
        view.copy_(x)
    want = R.apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, positions=pos, **kw)
    for pe in (pe_v, pe_v.unsqueeze(2)):
        got = R.apply_mla_rotary_freqs(q_v, kv_v, pe, inv_freq, positions=pos, **kw)
        assert all(torch.equal(g, w) and not torch.isnan(g).any() for g, w in zip(got, want))
    # map mode: rank 1 of a 2-rank zigzag through the backend's pos_map, and `layout=` with an offset, against explicit positions
    zz = R.local_positions(R.zigzag_ring_flash_attn_func, S, rank=1, world_size=2, device=DEV)
    want = R.apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, positions=zz, **kw)
    got = [torch.empty_like(t) for t in want]
    get_backend().mla_rotary_freqs_fwd(q, got[0], kv, k_pe, got[1], got[2], inv_freq, nope_dim=Dn, scaling=SCALINGS[1],
                                       pos_map=zigzag_map(1, 2, S // 2), interleaved=inter)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    ar = torch.arange(S, dtype=torch.int32, device=DEV)
    a = R.apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, layout=R.zigzag_ring_flash_attn_func, offset=5, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, R.apply_mla_rotary_freqs(q, kv, k_pe, inv_freq, positions=ar, offset=5, **kw)))
    # without q: the same k and v
    none, k, v = R.apply_mla_rotary_freqs(None, kv, k_pe, inv_freq, nope_dim=Dn, positions=zz, **kw)
    assert none is None and torch.equal(k, want[1]) and torch.equal(v, want[2])
    # packed (T, H, D) is the (1, T, H, D) call, forward and backward, and its last tile is ragged
    T = 77
    qp, kvp, pep, posp = _inputs(Dn, Dr, Dv, H, dtype, lead=(T,))
    leaves = [t.clone().requires_grad_(True) for t in (qp, kvp, pep[:, 0])]
    outs = R.apply_mla_rotary_freqs(*leaves, inv_freq, positions=posp, **kw)
    l4 = [t.detach().unsqueeze(0).requires_grad_(True) for t in leaves]
    outs4 = R.apply_mla_rotary_freqs(*l4, inv_freq, positions=posp.view(1, T), **kw)
    assert all(torch.equal(a, b[0]) for a, b in zip(outs, outs4))
    gs = [_rand(31 + n, *t.shape, dtype=dtype) for n, t in enumerate(outs)]
    g3, g4 = torch.autograd.grad(outs, leaves, gs), torch.autograd.grad(outs4, l4, [g.unsqueeze(0) for g in gs])
    assert all(torch.equal(a, b[0]) for a, b in zip(g3, g4)) and g3[2].shape == (T, Dr)
