"""Multi-process worker of the sliding-window ring / zigzag tests: one rank of a gloo world runs the public functions
on its shard of a seeded sequence and compares with ONE windowed attention over the unsharded tensors.  Backend: the
CPU oracle with `mask_shift` (tests/_ref_backend.py) or the HIP kernels with every rank sharing cuda:0."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def ring_rule(W, S, rank, causal, window):
    """the counts the issue's rule gives for a ring rank: (block calls, K/V hops)"""
    wl, wr = window
    total = W * S
    if wl >= total - 1:
        wl = -1
    if causal or wr >= total - 1:
        wr = -1
    if wl < 0 and wr < 0:
        return ((rank + 1) if causal else W), W - 1
    if causal:
        ok = lambda d: d == 0 or wl < 0 or wl >= (d - 1) * S + 1
        d_max = max(d for d in range(W) if ok(d))
        return sum(1 for d in range(W) if d <= rank and ok(d)), d_max
    n = 0
    for src in range(W):
        t = rank - src
        if t == 0 or (t > 0 and (wl < 0 or wl >= (t - 1) * S + 1)) or (t < 0 and (wr < 0 or wr >= (-t - 1) * S + 1)):
            n += 1
    return n, W - 1


class Counting:
    """wraps a backend: counts fwd / bwd block calls (a two-phase backward counts once) and logs their keywords"""

    def __init__(self, inner):
        self.inner, self.n_fwd, self.n_bwd, self.log = inner, 0, 0, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    @staticmethod
    def _sig(name, a, kw):
        keys = ("causal", "window", "mask_shift", "acc_init", "phases", "q_half", "k_half")
        return (name, tuple(tuple(t.shape) for t in a[:3]), tuple((k_, kw[k_]) for k_ in keys if k_ in kw),
                tuple(sorted(k_ for k_ in kw if k_.startswith(("out", "lse", "dq", "dk", "dv")) and kw[k_] is not None)))

    def fwd(self, *a, **kw):
        self.n_fwd += 1
        self.log.append(self._sig("fwd", a, kw))
        return self.inner.fwd(*a, **kw)

    def bwd(self, *a, **kw):
        if not (kw.get("phases", 0) & 2) or (kw.get("phases", 0) & 1):
            self.n_bwd += 1
        self.log.append(self._sig("bwd", a[1:], kw))
        return self.inner.bwd(*a, **kw)


def _cmp(name, got, ref, tol, errs):
    """_ring_worker._cmp with its bounds unchanged — |err| <= atol + rtol max|ref| (TOL_ORACLE) and a relative Frobenius
    error of 1e-2, or a tests/_tol.py kind for the HIP kernels — except that the Frobenius criterion carries the absolute
    floor tests/_tol.py uses (atol / 4 per element): with window_left = 0 every query sees exactly one key, dQ and dK
    are EXACTLY zero in the reference, and a relative criterion against a zero norm cannot be met by any rounded result."""
    from _ring_worker import _cmp as base

    if isinstance(tol, str):
        return base(name, got, ref, tol, errs)
    got, ref = got.float(), ref.float()
    if got.shape != ref.shape:
        errs.append(f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}")
        return
    atol, rtol = tol
    diff = (got - ref).abs().max().item()
    lim = atol + rtol * ref.abs().max().item()
    if not (diff <= lim):
        errs.append(f"{name}: max|diff| {diff:.3e} > {lim:.3e}")
    err_n, ref_n = (got - ref).double().norm().item(), ref.double().norm().item()
    lim = 1e-2 * ref_n + 0.25 * atol * ref.numel() ** 0.5
    if not (err_n <= lim):
        errs.append(f"{name}: ||err||_F {err_n:.3e} > 1e-2 ||ref||_F + floor = {lim:.3e}")


def _inputs(c):
    g = torch.Generator().manual_seed(c["seed"])
    W, B, S, H, Hk, D = c["W"], c.get("B", 1), c["S"], c["H"], c["Hk"], c["D"]
    dt = c.get("dtype", torch.bfloat16)
    mk = lambda h: torch.randn(B, W * S, h, D, generator=g).to(dt)
    return mk(H), mk(Hk), mk(Hk), mk(H)


def _reference(c, q, k, v, do, dev):
    """ONE windowed attention over the unsharded tensors in fp64 with autograd"""
    from oracle import flash_attn_ref as O

    qd, kd, vd = (t.to(dev).double().requires_grad_(True) for t in (q, k, v))
    out, lse = O.full_attention_fp64(qd, kd, vd, c["causal"], window=c["window"])
    out.backward(do.to(dev).double())
    return [t.detach().cpu() for t in (out, lse, qd.grad, kd.grad, vd.grad)]


def _shard(c, t, rank, dim=1):
    import make_golden as MG

    if c["kind"] == "zigzag":
        return MG.zigzag_extract(t, rank, c["W"], dim).contiguous()
    return t.chunk(c["W"], dim=dim)[rank].contiguous()


def _call(R, c, form, q, k, v, window):
    kw = dict(causal=c["causal"], window_size=window, return_attn_probs=True)
    pre = "zigzag_ring_flash_attn" if c["kind"] == "zigzag" else "ring_flash_attn"
    if form == "func":
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, lse, _ = getattr(R, pre + "_func")(*ins, **kw)
        grads = lambda: (ins[0].grad, ins[1].grad, ins[2].grad)
    elif form == "kvpacked":
        qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_kvpacked_func")(qq, kv, **kw)
        grads = lambda: (qq.grad, kv.grad[:, :, 0], kv.grad[:, :, 1])
    else:
        qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_qkvpacked_func")(qkv, **kw)
        grads = lambda: (qkv.grad[:, :, 0], qkv.grad[:, :, 1], qkv.grad[:, :, 2])
    return out, lse, grads


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, utils
        from _ring_worker import TOL_HIP, TOL_ORACLE

        if use_hip:
            from ring_flash_attn.backend import get_backend

            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.set_backend(None)
            _testing.allow_host_staging(True)
            inner, tol = get_backend(), TOL_HIP
        else:
            from _ref_backend import RefBackend

            dev = torch.device("cpu")
            inner, tol = RefBackend(serves=("mask_shift",)), TOL_ORACLE
        errs = []
        hops = [0]
        orig_commit = utils.RingComm.commit

        def counting_commit(self):
            hops[0] += 1
            return orig_commit(self)

        utils.RingComm.commit = counting_commit
        for c0 in cases:
            name = c0["name"]
            for form in c0.get("forms", ("func",)):
                # (the qkv-packed entry points need as many K/V heads as query heads: that form runs the case as MHA)
                c = dict(c0, Hk=c0["H"]) if form == "qkvpacked" else c0
                q, k, v, do = _inputs(c)
                ref = None
                if rank == 0 or not use_hip:
                    ref = _reference(c, q, k, v, do, dev if use_hip else torch.device("cpu"))
                if use_hip:
                    # (one fp64 reference per world, computed by rank 0 on the device, handed round as CPU tensors)
                    box = [ref]
                    dist.broadcast_object_list(box, src=0)
                    ref = box[0]
                ql, kl, vl, dol = (_shard(c, t, rank).to(dev) for t in (q, k, v, do))
                be = Counting(inner)
                _testing.set_backend(be)
                hops[0] = 0
                out, lse, grads = _call(R, c, form, ql, kl, vl, c["window"])
                f_calls, f_hops = be.n_fwd, hops[0]
                hops[0] = 0
                out.backward(dol)
                dq, dk, dv = grads()
                tag = f"{name}[{form}][r{rank}]"
                if c["kind"] == "ring" and "counts" in c.get("check", ()):
                    n_calls, n_hops = ring_rule(W, c["S"], rank, c["causal"], c["window"])
                    if f_calls != n_calls or be.n_bwd != n_calls:
                        errs.append(f"{tag}: {f_calls} fwd / {be.n_bwd} bwd block calls, the rule gives {n_calls}")
                    if f_hops != n_hops:
                        errs.append(f"{tag}: {f_hops} K/V hops in the forward, the rule gives {n_hops}")
                    # backward: the K/V hops again, the dK/dV accumulators one hop behind them, and ONE transfer home
                    want_b = 2 * n_hops + (1 if n_hops % W else 0)
                    if hops[0] != want_b:
                        errs.append(f"{tag}: {hops[0]} exchanges in the backward, the rule gives {want_b}")
                for nm, got, r_, kind in (("out", out, ref[0], "out"), ("lse", lse, ref[1], "lse"), ("dq", dq, ref[2], "grad"),
                                          ("dk", dk, ref[3], "grad"), ("dv", dv, ref[4], "grad")):
                    want = _shard(c, r_, rank, dim=2 if nm == "lse" else 1)
                    _cmp(f"{tag}.{nm}", got.detach().cpu().float(), want.float(), tol[kind], errs)
                if "same_as_unwindowed" in c.get("check", ()):
                    # a window that covers the whole sequence is dropped on the host: the unwindowed call's bits and calls
                    be2 = Counting(inner)
                    _testing.set_backend(be2)
                    out2, lse2, grads2 = _call(R, c, form, ql, kl, vl, (-1, -1))
                    out2.backward(dol)
                    for nm, a_, b_ in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, dq, dk, dv), (out2, lse2) + tuple(grads2())):
                        if not torch.equal(a_.detach(), b_.detach()):
                            errs.append(f"{tag}.{nm}: differs from the unwindowed call")
                    if be.log != be2.log:
                        errs.append(f"{tag}: backend calls differ from the unwindowed call's")
                    if any("mask_shift" in dict(e[2]) or dict(e[2]).get("window", (-1, -1)) != (-1, -1) for e in be2.log):
                        errs.append(f"{tag}: an unwindowed call passed a window or a shift to the backend")
                    ret[f"log:{name}:{form}:{rank}"] = be2.log
        utils.RingComm.commit = orig_commit
        ret[rank] = errs
    except Exception:
        ret[rank] = [f"rank {rank} crashed:\n{traceback.format_exc()}"]
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=420):
    """one world under its own time limit: ranks that have not finished after limit_s seconds are killed and the
    world reports that instead of results"""
    import time

    import torch.multiprocessing as mp

    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, cases, use_hip, ret), nprocs=W, join=False)
    deadline = time.time() + limit_s
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            return [f"world of {W} ranks did not finish within {limit_s} s"], {}
    errs = []
    for r in range(W):
        errs += list(ret.get(r, [f"rank {r} returned nothing"]))
    return errs, {k_: v_ for k_, v_ in ret.items() if isinstance(k_, str)}
