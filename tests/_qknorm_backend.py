"""TEST INFRASTRUCTURE: the CPU test backend with the rotary embedding (tests/_rotary_backend.py) plus the fused per-head QK
RMSNorm — `serves_qk_norm` and `qk_norm_rotary_fwd` / `qk_norm_rotary_bwd` written in torch fp32 from the text of include/rfa.h
(rfa_qk_norm_rotary_fwd / _bwd), independently of the index functions the kernels use — and the textbook formulas in fp64
(`reference`) with the magnitudes that scale the derived tolerances, which the CPU and the GPU tests compare with."""
import torch

from _rotary_backend import RotaryBackend, rotate, row_positions


def _rot(v, cos, sin, pos, interleaved, rot_offset, conj, dtype):
    """(rotated v, magnitude): rotated columns |v1 c| + |v2 s|, pass-through columns |v|; cos None: nothing is rotated"""
    v = v.to(dtype)
    if cos is None:
        return v.clone(), v.abs()
    out, mag = rotate(v, cos, sin, pos, interleaved, rot_offset, conj, dtype)
    R = 2 * cos.shape[1]
    mag[..., :rot_offset] = v[..., :rot_offset].abs()
    mag[..., rot_offset + R:] = v[..., rot_offset + R:].abs()
    return out, mag


def norm_rotary(x, w, cos, sin, pos, interleaved, rot_offset, eps, weight_offset, dtype, dout=None):
    """x (B,S,H,D), pos (B,S) int64, arithmetic in `dtype`: dict with y and Mf; with dout also dx, Mb, dw, T and rstd"""
    D = x.shape[-1]
    x = x.to(dtype)
    a = weight_offset + w.to(dtype)
    rstd = torch.rsqrt(x.pow(2).sum(-1, keepdim=True) / D + eps)
    xh = x * rstd
    y, mf = _rot(xh * a, cos, sin, pos, interleaved, rot_offset, False, dtype)
    res = dict(y=y, Mf=mf)
    if dout is not None:
        g, gm = _rot(dout, cos, sin, pos, interleaved, rot_offset, True, dtype)
        ga = g * a
        m = (ga * xh).sum(-1, keepdim=True) / D
        res["dx"] = rstd * (ga - xh * m)
        res["Mb"] = rstd * (gm * a.abs() + xh.abs() * ((gm * a.abs() * xh.abs()).sum(-1, keepdim=True) / D))
        res["dw"] = (g * xh).sum(dim=(0, 1, 2))
        res["T"] = (gm * xh.abs()).sum(dim=(0, 1, 2))
    return res


def reference(x, w, cos, sin, pos, interleaved=False, rot_offset=0, eps=1e-6, weight_offset=0.0, dout=None):
    """fp64 on the CPU: x (B,S,H,D) or (T,H,D), pos (S,) / (B,S) / (T,) positions inside the tables (ignored without tables)"""
    x4 = (x.unsqueeze(0) if x.dim() == 3 else x).double().cpu()
    d4 = None if dout is None else (dout.unsqueeze(0) if dout.dim() == 3 else dout).double().cpu()
    if cos is not None:
        pos = torch.as_tensor(pos, dtype=torch.int64).cpu().reshape(-1, x4.shape[1]).expand(x4.shape[0], x4.shape[1])
        cos, sin = cos.double().cpu(), sin.double().cpu()
    res = norm_rotary(x4, w.double().cpu(), cos, sin, pos, interleaved, rot_offset, eps, weight_offset, torch.float64, d4)
    if x.dim() == 3:
        res = {n: (t[0] if n in ("y", "Mf", "dx", "Mb") else t) for n, t in res.items()}
    return res


class QkNormBackend(RotaryBackend):
    serves_qk_norm = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+qknorm"
        self.qk_norm_calls = []

    @staticmethod
    def _pos(x, cos, positions, pos_map):
        return None if cos is None else row_positions(tuple(x.shape), cos.shape[0], positions, pos_map)

    def qk_norm_rotary_fwd(self, xs, outs, weights, cos, sin, *, positions=None, pos_map=None, interleaved=False, rot_offset=0,
                           eps=1e-6, weight_offset=0.0):
        self.qk_norm_calls.append(dict(dir="fwd", n=len(xs), positions=positions is not None, pos_map=pos_map, eps=eps,
                                       weight_offset=weight_offset, tables=cos is not None))
        for x, o, w in zip(xs, outs, weights):
            x4, o4 = (t.unsqueeze(0) if t.dim() == 3 else t for t in (x, o))
            r = norm_rotary(x4, w, cos, sin, self._pos(x, cos, positions, pos_map), interleaved, rot_offset, eps, weight_offset,
                            torch.float32)
            o4.copy_(r["y"].to(o.dtype))

    def qk_norm_rotary_bwd(self, xs, douts, dxs, weights, dweights, cos, sin, *, positions=None, pos_map=None, interleaved=False,
                           rot_offset=0, eps=1e-6, weight_offset=0.0):
        self.qk_norm_calls.append(dict(dir="bwd", n=len(xs), dweights=[d is not None for d in dweights]))
        for x, g, dx, w, dw in zip(xs, douts, dxs, weights, dweights):
            x4, g4, dx4 = (t.unsqueeze(0) if t.dim() == 3 else t for t in (x, g, dx))
            r = norm_rotary(x4, w, cos, sin, self._pos(x, cos, positions, pos_map), interleaved, rot_offset, eps, weight_offset,
                            torch.float32, g4)
            dx4.copy_(r["dx"].to(dx.dtype))
            if dw is not None:
                dw.copy_(r["dw"])


def kernel_chain(items, D):
    """the longest sequential accumulation chain of the HIP weight gradient (csrc/rfa_qknorm.hip, SUMMATION ORDERS), from the
    shape alone: a lane's walk, the workgroup's 256/G lane groups, a run of partials, the 16 runs.  items: B S H of the tensor
    (its partial count does not depend on the tensor that rides along)."""
    G = 1
    while G * 8 < D:
        G *= 2
    per = 256 // G
    nparts = min(-(-items // per), 1024)
    walk = -(-items // (nparts * per))
    return walk + per + -(-nparts // 16) + 16
