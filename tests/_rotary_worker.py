"""Worker of the multi-rank rotary tests: one gloo rank of a world of W applies `apply_rotary(layout=func)` to its shards of a
seeded sequence — the shards `func` over all W ranks expects — then, where the case asks, runs `func` (or
`with_ulysses(func, ug)` over its ring group) forward and backward on them.  Rank 0 also rotates the unsharded tensors on its
own; the parent un-shards by the schedule's layout and compares.  Backend: the CPU test backend (tests/_rotary_backend.py)
or the HIP kernels with every rank sharing cuda:0."""
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


def case_name(c):
    return f"{c['kind']}-W{c['W']}-S{c['S']}-D{c['D']}-R{c['R']}+{c.get('rot_offset', 0)}" \
           f"{'-gptj' if c.get('interleaved') else ''}{'-U%d' % c['U'] if c.get('U') else ''}"


def inputs(c):
    """the unsharded (q, k, v, dout, cos, sin) of a case: W * S rows, one table row per position"""
    B, H, Hk, D, n = c.get("B", 2), c.get("H", 3), c.get("Hk", 1), c["D"], c["W"] * c["S"]
    g = torch.Generator().manual_seed(17)
    mk = lambda h: torch.randn(B, n, h, D, generator=g).bfloat16()
    q, k, v, do = mk(H), mk(Hk), mk(Hk), mk(H)
    ang = torch.arange(n, dtype=torch.float64).view(-1, 1) * (10000.0 ** (-torch.arange(c["R"] // 2, dtype=torch.float64) / (c["R"] // 2)))
    return q, k, v, do, ang.cos().float(), ang.sin().float()


def rot_kw(c):
    return dict(interleaved=bool(c.get("interleaved")), rot_offset=c.get("rot_offset", 0))


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
            from _rotary_backend import RotaryBackend

            dev = torch.device("cpu")
            _testing.set_backend(RotaryBackend(serves=("mask_shift",)))
        groups = {}
        for c in cases:
            name, kind = case_name(c), c["kind"]
            func = getattr(R, PREFIX[kind] + "_func")
            q, k, v, do, cos, sin = inputs(c)
            cos, sin = cos.to(dev), sin.to(dev)
            qs, ks, vs, dos = (shard(kind, t, rank, W).to(dev) for t in (q, k, v, do))
            qs.requires_grad_(True), ks.requires_grad_(True), vs.requires_grad_(True)
            qr, kr = R.apply_rotary(qs, ks, cos, sin, layout=func, group=None, **rot_kw(c))
            got = {"qr": qr, "kr": kr}
            # the same positions as a tensor: the same bits
            pos = R.local_positions(func, c["S"], device=dev)
            q2, k2 = R.apply_rotary(qs.detach(), ks.detach(), cos, sin, positions=pos, **rot_kw(c))
            got["same"] = torch.tensor(torch.equal(q2, qr) and torch.equal(k2, kr))
            got["pos"] = pos
            if c.get("attn"):
                attn = func
                kw = dict(causal=True)
                if c.get("U"):
                    key = (kind == "stripe", c["U"])
                    if key not in groups:
                        groups[key] = R.make_usp_groups(func, c["U"])
                    ug, rg = groups[key]
                    attn, kw = R.with_ulysses(func, ug), dict(causal=True, group=rg)
                out = attn(qr, kr, vs, **kw)
                out.backward(dos)
                got.update(out=out, dq=qs.grad, dk=ks.grad, dv=vs.grad)
            if rank == 0:                                         # the single-device rotation of the unsharded tensors
                qf, kf = R.apply_rotary(q.to(dev), k.to(dev), cos, sin, **rot_kw(c))
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
    """one world under its own time limit; returns ({case name: {tensor name: un-sharded tensor}}, complaints)"""
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
            res[name] = {n: unshard(c["kind"], [p[n] for p in per], dim=0 if n == "pos" else 1)
                         for n in per[0] if n not in ("same", "qfull", "kfull")}
            res[name]["same"] = all(bool(p["same"]) for p in per)
            res[name]["qfull"], res[name]["kfull"] = per[0]["qfull"], per[0]["kfull"]
    return res, errs


def check_case(c, r, conj_reference):
    """the parent's comparisons for one case's un-sharded results `r`: list of complaints"""
    from _tol import exact_attention, failures

    name, bad = case_name(c), []
    q, k, v, do, cos, sin = inputs(c)
    n = c["W"] * c["S"]
    if r["pos"].tolist() != list(range(n)):
        bad.append(f"{name}: the un-sharded local_positions are not 0 .. {n - 1}")
    if not r["same"]:
        bad.append(f"{name}: map mode and explicit positions differ in bits")
    if not (torch.equal(r["qr"], r["qfull"]) and torch.equal(r["kr"], r["kfull"])):
        bad.append(f"{name}: the rotated shards are not the shards of the rotated full tensor, bit for bit")
    if c.get("attn"):
        out, dqr, dkr, dv = exact_attention(r["qfull"], r["kfull"], v, do, True)
        # the rotation's backward is the conjugate rotation of the gradients (fp64)
        dq = conj_reference(dqr, cos, sin, torch.arange(n), conj=True, **rot_kw(c))[0].float()
        dk = conj_reference(dkr, cos, sin, torch.arange(n), conj=True, **rot_kw(c))[0].float()
        for what, got, ref, kind in (("out", r["out"], out, "out_ring"), ("dq", r["dq"], dq, "grad_ring"),
                                     ("dk", r["dk"], dk, "grad_ring"), ("dv", r["dv"], dv, "grad_ring")):
            bad += failures(f"{name} {what}", got, ref, kind)
    return bad
