"""TEST INFRASTRUCTURE: the CPU test backend (tests/_usp_backend.py) with the rotary embedding — `serves_rotary` and
`rotary` written in torch fp32 from the text of include/rfa.h (rfa_rotary), independently of the index functions the kernel
uses — and the textbook formula in fp64 (`reference`), which the CPU and the GPU tests compare with."""
import torch

from ring_flash_attn._common import map_positions
from _usp_backend import UspBackend


def row_positions(shape, P, positions, pos_map):
    """(B, S) int64 positions of a (B,S,H,D) / (T,H,D) tensor as rfa_rotary reads the tables: offset added, clamped to [0, P-1]"""
    packed = len(shape) == 3
    B, S = (1, shape[0]) if packed else (shape[0], shape[1])
    off, rest = pos_map if pos_map is not None else (0, (1, 0, 0))
    if positions is not None:
        pos = positions.to(torch.int64).reshape(-1, S).expand(B, S) + off
    else:
        pos = torch.tensor(map_positions((off, rest), S), dtype=torch.int64).view(1, S).expand(B, S)
    return pos.clamp(0, P - 1)


def _pairs(x, R, rot_offset, interleaved):
    """(x1, x2) views of the rotated columns of x (..., D)"""
    r = x[..., rot_offset:rot_offset + R]
    return (r[..., 0::2], r[..., 1::2]) if interleaved else (r[..., :R // 2], r[..., R // 2:])


def rotate(x, cos, sin, pos, interleaved, rot_offset, conj, dtype):
    """x (B,S,H,D) any float dtype, pos (B,S) int64 -> (rotated x in `dtype` arithmetic, |x1 c| + |x2 s| per element)"""
    R = 2 * cos.shape[1]
    c = cos.to(dtype)[pos.to(cos.device)].unsqueeze(2)            # (B, S, 1, R/2)
    s = sin.to(dtype)[pos.to(sin.device)].unsqueeze(2)
    if conj:
        s = -s
    out = x.to(dtype).clone()
    mag = torch.zeros_like(out)
    x1, x2 = _pairs(x.to(dtype), R, rot_offset, interleaved)
    o1, o2 = _pairs(out, R, rot_offset, interleaved)
    m1, m2 = _pairs(mag, R, rot_offset, interleaved)
    o1.copy_(x1 * c - x2 * s)
    o2.copy_(x2 * c + x1 * s)
    m1.copy_((x1 * c).abs() + (x2 * s).abs())
    m2.copy_((x2 * c).abs() + (x1 * s).abs())
    return out, mag


def reference(x, cos, sin, pos, interleaved=False, rot_offset=0, conj=False):
    """fp64: (the rotated tensor, the magnitude |x1 c| + |x2 s| that scales the fp32 products' error); x (B,S,H,D) or (T,H,D),
    pos (S,) / (B,S) / (T,) positions inside the tables"""
    x4 = x.unsqueeze(0) if x.dim() == 3 else x
    pos = torch.as_tensor(pos, dtype=torch.int64).reshape(-1, x4.shape[1]).expand(x4.shape[0], x4.shape[1])
    out, mag = rotate(x4.double().cpu(), cos.double().cpu(), sin.double().cpu(), pos.cpu(), interleaved, rot_offset, conj, torch.float64)
    return (out[0], mag[0]) if x.dim() == 3 else (out, mag)


def torch_rotary(srcs, dsts, cos, sin, positions=None, pos_map=None, interleaved=False, rot_offset=0, conj=False):
    """include/rfa.h: rfa_rotary in torch fp32, each result rounded once to the io dtype; in place (dst is src) the pass-through
    columns are not written"""
    R = 2 * cos.shape[1]
    for s, d in zip(srcs, dsts):
        pos = row_positions(tuple(s.shape), cos.shape[0], positions, pos_map)
        s4, d4 = (t.unsqueeze(0) if t.dim() == 3 else t for t in (s, d))
        out, _ = rotate(s4, cos, sin, pos, interleaved, rot_offset, conj, torch.float32)
        if d is s:
            d4[..., rot_offset:rot_offset + R] = out[..., rot_offset:rot_offset + R].to(d.dtype)
        else:
            d4.copy_(out.to(d.dtype))


class RotaryBackend(UspBackend):
    serves_rotary = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+rotary"
        self.rotary_calls = []

    def rotary(self, srcs, dsts, cos, sin, *, positions=None, pos_map=None, interleaved=False, rot_offset=0, conj=False):
        self.rotary_calls.append(dict(n=len(srcs), positions=positions is not None, pos_map=pos_map, conj=conj,
                                      inplace=[d is s for s, d in zip(srcs, dsts)]))
        torch_rotary(srcs, dsts, cos, sin, positions, pos_map, interleaved, rot_offset, conj)
