"""Worker of the multi-rank QK norm + rotary tests: one gloo rank of a world of W applies `apply_qk_norm_rotary(layout=func)` to
its shards of a seeded sequence — the shards `func` over all W ranks expects — twice: once with seeded gradients straight behind
it (dq, dk and this rank's PARTIAL weight gradients), once followed by `func` forward and backward.  Rank 0 also runs the
unsharded tensors on its own; the parent un-shards by the schedule's layout and compares with one fp64 computation.  Backend:
the CPU test backend (tests/_qknorm_backend.py) or the HIP kernels with every rank sharing cuda:0."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _droppos_worker import PREFIX, shard, unshard          # noqa: E402  (the dense families' own sharding)
from _rotary_worker import case_name, inputs, rot_kw         # noqa: E402  (the rotary cases' seeded inputs)

EPS = 1e-6


def weights(c):
    """(w_q, w_k) fp32 around 1 and the seeded gradient of the normed k (q's is the attention's `do`)"""
    g = torch.Generator().manual_seed(23)
    D, n = c["D"], c["W"] * c["S"]
    wq, wk = 1.0 + 0.25 * torch.randn(D, generator=g), 1.0 + 0.25 * torch.randn(D, generator=g)
    dk = torch.randn(c.get("B", 2), n, c.get("Hk", 1), D, generator=g).bfloat16()
    return wq, wk, dk


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
            _testing.set_backend(None)
        else:
            from _qknorm_backend import QkNormBackend

            dev = torch.device("cpu")
            _testing.set_backend(QkNormBackend(serves=("mask_shift",)))
        for c in cases:
            name, kind = case_name(c), c["kind"]
            func = getattr(R, PREFIX[kind] + "_func")
            q, k, v, do, cos, sin = inputs(c)
            wq, wk, dkn = weights(c)
            cos, sin = cos.to(dev), sin.to(dev)
            kw = dict(eps=EPS, weight_offset=c.get("weight_offset", 0.0), **rot_kw(c))
            qs, ks, vs, dos, dks = (shard(kind, t, rank, W).to(dev) for t in (q, k, v, do, dkn))
            wqd, wkd = wq.to(dev).requires_grad_(True), wk.to(dev).requires_grad_(True)
            qs.requires_grad_(True), ks.requires_grad_(True), vs.requires_grad_(True)
            # seeded gradients straight behind the call
            qr, kr = R.apply_qk_norm_rotary(qs, ks, wqd, wkd, cos, sin, layout=func, group=None, **kw)
            torch.autograd.backward([qr, kr], [dos, dks])
            got = {"qr": qr, "kr": kr, "dq0": qs.grad, "dk0": ks.grad, "dwq": wqd.grad, "dwk": wkd.grad}
            pos = R.local_positions(func, c["S"], device=dev)
            q2, k2 = R.apply_qk_norm_rotary(qs.detach(), ks.detach(), wqd.detach(), wkd.detach(), cos, sin, positions=pos, **kw)
            got["same"] = torch.tensor(torch.equal(q2, qr) and torch.equal(k2, kr))
            if c.get("attn"):
                qs.grad = ks.grad = None
                qr, kr = R.apply_qk_norm_rotary(qs, ks, wqd.detach(), wkd.detach(), cos, sin, layout=func, group=None, **kw)
                out = func(qr, kr, vs, causal=True)
                out.backward(dos)
                got.update(out=out, dq=qs.grad, dk=ks.grad, dv=vs.grad)
            if rank == 0:                                         # the single-device result of the unsharded tensors
                qf, kf = R.apply_qk_norm_rotary(q.to(dev), k.to(dev), wqd.detach(), wkd.detach(), cos, sin, **kw)
                got.update(qfull=qf, kfull=kf)
            ret[(name, rank)] = {n: t.detach().cpu() for n, t in got.items()}
        ret[rank] = "ok"
    except Exception:
        ret[rank] = f"rank {rank} crashed:\n{traceback.format_exc()}"
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=240):
    """one world under its own time limit; returns ({case name: {tensor name: un-sharded tensor}}, complaints); the weight
    gradients come back as the list of the ranks' partials"""
    import time

    import torch.multiprocessing as mp

    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, cases, use_hip, ret), nprocs=W, join=False)
    deadline = time.time() + limit_s
    while not ctx.join(timeout=1):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            return {}, [f"world of {W} ranks did not finish within {limit_s} s"]
    got = dict(ret)
    errs = [got.get(r, f"rank {r} returned nothing") for r in range(W) if got.get(r) != "ok"]
    res = {}
    if not errs:
        for c in cases:
            name = case_name(c)
            per = [got[(name, r)] for r in range(W)]
            res[name] = {n: unshard(c["kind"], [p[n] for p in per], dim=1)
                         for n in per[0] if n not in ("same", "qfull", "kfull", "dwq", "dwk")}
            res[name]["same"] = all(bool(p["same"]) for p in per)
            res[name]["qfull"], res[name]["kfull"] = per[0]["qfull"], per[0]["kfull"]
            res[name]["dwq"], res[name]["dwk"] = [p["dwq"] for p in per], [p["dwk"] for p in per]
    return res, errs


def check_case(c, r, reference, chain):
    """the parent's comparisons for one case's un-sharded results `r`: list of complaints.  reference: tests/_qknorm_backend.py;
    chain(items): the longest accumulation chain of a weight gradient over `items` (row, head)s on the backend that ran"""
    from _tol import exact_attention, failures

    name, bad = case_name(c), []
    q, k, v, do, cos, sin = inputs(c)
    wq, wk, dkn = weights(c)
    n, u, half = c["W"] * c["S"], 2.0 ** -8, 2.0 ** -134
    kw = dict(eps=EPS, weight_offset=c.get("weight_offset", 0.0), **rot_kw(c))
    if not r["same"]:
        bad.append(f"{name}: map mode and explicit positions differ in bits")
    if not (torch.equal(r["qr"], r["qfull"]) and torch.equal(r["kr"], r["kfull"])):
        bad.append(f"{name}: the shards' results are not the shards of the single-device result, bit for bit")
    for what, x, w, dout, y, dx, dws in (("q", q, wq, do, r["qr"], r["dq0"], r["dwq"]), ("k", k, wk, dkn, r["kr"], r["dk0"], r["dwk"])):
        ref = reference(x, w, cos, sin, torch.arange(n), dout=dout, **kw)
        for label, got, want, mag, fac in ((what, y, ref["y"], ref["Mf"], 2.0 ** -19), ("d" + what, dx, ref["dx"], ref["Mb"], 2.0 ** -18)):
            over = ((got.double() - want).abs() - ((u * want.abs()).clamp(min=half) + fac * mag)).max().item()
            if over > 0:
                bad.append(f"{name} {label}: {over:.3e} over the bound")
        # every rank's partial within the bound of ITS chain and ITS magnitudes: the sum over ranks within the sum of them
        items = x.shape[0] * c["S"] * x.shape[2]
        total = torch.stack([d.double() for d in dws]).sum(0)
        over = ((total - ref["dw"]).abs() - (chain(items) + 24) * 2.0 ** -24 * ref["T"]).max().item()
        if over > 0:
            bad.append(f"{name} dw_{what}: the ranks' partials sum to {over:.3e} over the bound")
    if c.get("attn"):
        out, dqr, dkr, dv = exact_attention(r["qfull"], r["kfull"], v, do, True)
        dq = reference(q, wq, cos, sin, torch.arange(n), dout=dqr, **kw)["dx"].float()
        dk = reference(k, wk, cos, sin, torch.arange(n), dout=dkr, **kw)["dx"].float()
        for what, got, ref, kind in (("out", r["out"], out, "out_ring"), ("dq", r["dq"], dq, "grad_ring"),
                                     ("dk", r["dk"], dk, "grad_ring"), ("dv", r["dv"], dv, "grad_ring")):
            bad += failures(f"{name} {what}", got, ref, kind)
    return bad
