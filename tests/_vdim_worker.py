"""Worker of the multi-rank tests of a value head dim of its own: one gloo rank runs a public function on its shard of a
seeded sequence whose `v` is Dv wide next to a D-wide q / k, and compares out, lse, dq, dk, dv with its shard of ONE
single-device fp64 autograd attention on the unsharded tensors (tests/_vdim_backend.py: single_device) that the parent made
once.  Backend: the CPU test backend with `serves_vdim` or the HIP kernels with every rank sharing cuda:0 (host staging).
Kinds and sharding are those of tests/_softcap_worker.py.  A case with `refuse` names the exception the call must raise on
EVERY rank before anything is exchanged: no block call is made, and a barrier afterwards finds every rank in step."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _softcap_worker as SW                                  # noqa: E402
import _tol                                                   # noqa: E402
import _vdim_backend as VB                                    # noqa: E402

B, H, HK = 2, 4, 2
DENSE = SW.DENSE


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-D{c['D']}_{c['Dv']}-" \
           f"{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}{'-' + c['refuse'] if c.get('refuse') else ''}" \
           f"{'-' + c['how'] if c.get('how') else ''}"


def _cu(lens):
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    return cu


def inputs(c):
    """(q, k, v, do) unsharded, seeded; v and do are Dv wide"""
    g = torch.Generator().manual_seed(31)
    lens = SW.lens_of(c)
    lead = (B, c["W"] * c["S"]) if lens is None else (sum(lens),)
    mk = lambda h, d: torch.randn(*lead, h, d, generator=g).to(c.get("dtype", torch.bfloat16))
    return mk(H, c["D"]), mk(HK, c["D"]), mk(HK, c["Dv"]), mk(H, c["Dv"])


def reference(c):
    q, k, v, do = inputs(c)
    lens = SW.lens_of(c)
    return VB.single_device(q, k, v, do, c["causal"], c.get("window", (-1, -1)), None if lens is None else _cu(lens))


def call(R, c, q, k, v, rank, dev, **more):
    fn = getattr(R, SW.FUNCS[c["kind"]])
    how = c.get("how")
    if how == "ulysses":
        fn = R.with_ulysses(fn, more.pop("ulysses_group"))
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True, **more)
    kind = c["kind"]
    if kind in DENSE:
        return fn(q, k, v, **kw)
    if kind in ("ring_varlen", "zigzag_varlen"):
        local = [L // c["W"] for L in c["lens"]]
        cu = torch.tensor(_cu(local), dtype=torch.int32, device=dev)
        return fn(q, k, v, cu, max(local), **kw)
    cu_all = torch.tensor(_cu(SW.lens_of(c)), dtype=torch.int32)
    if kind == "zigzag_llama3":
        return fn(q, k, v, cu_all, **kw)
    cq, ck, mq, mk, sl = R.llama3_flash_attn_prepare_cu_seqlens(cu_all, c["causal"], rank, c["W"])
    return fn(q, k, v, cq.to(dev), ck.to(dev), mq, mk, heads_k_stride=1, local_k_slice=sl, **kw)


def _refusal(R, c, q, k, v, rank, dev, be_cpu, _testing):
    """the complaint of a `refuse` case, or None"""
    how, more = c.get("how"), {}
    rec = VB.Recording(be_cpu)
    if how == "backend":                                        # a backend without serves_vdim
        from _ref_backend import RefBackend

        rec = VB.Recording(RefBackend(serves=("mask_shift", "mask_shift_lens")))
    _testing.set_backend(rec)
    if how == "dropout":
        more["dropout_p"] = 0.1
    elif how == "alibi":
        more["alibi_slopes"] = torch.full((H,), 0.1, dtype=torch.float32, device=dev)
    elif how == "ulysses":
        more["ulysses_group"] = dist.new_group(list(range(c["W"])))
    elif how == "rows":
        v = v[..., :-1, :, :].contiguous() if c["kind"] in DENSE else v[:-1].contiguous()
    want = {"ValueError": ValueError, "NotImplementedError": NotImplementedError}[c["refuse"]]
    try:
        call(R, c, q, k, v, rank, dev, **more)
    except want:
        pass
    except Exception as e:
        return f"raised {type(e).__name__}: {e}, want {c['refuse']}"
    else:
        return f"did not raise {c['refuse']}"
    if rec.seen["fwd"] or rec.seen["bwd"]:
        return "a block call was made before the refusal"
    dist.barrier()                                              # every rank refused: nobody waits in a collective
    return None


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config

        be_cpu = VB.VdimBackend()
        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        errs, notes = [], []
        for c in cases:
            name = f"{case_name(c)}[r{rank}]"
            dense = c["kind"] in DENSE
            rd = 1 if dense else 0
            q, k, v, do = (SW.shard(c, t, rank, rd).to(dev) for t in inputs(c))
            q, k, v = (t.requires_grad_(True) for t in (q, k, v))
            if c.get("refuse"):
                bad = _refusal(R, c, q, k, v, rank, dev, be_cpu, _testing)
                if bad:
                    errs.append(f"{name}: {bad}")
                continue
            _testing.set_backend(None if use_hip else be_cpu)
            with config.override(zigzag_exchange=c.get("form") or "ring", zigzag_varlen_exchange=c.get("vform") or "ring"):
                out, lse, _ = call(R, c, q, k, v, rank, dev)
                if tuple(out.shape) != tuple(q.shape[:-1]) + (c["Dv"],):
                    errs.append(f"{name}: out is {tuple(out.shape)}, want (..., {c['Dv']})")
                    continue
                out.backward(do)
            for t, g in ((q, q.grad), (k, k.grad), (v, v.grad)):
                if g is None or g.shape != t.shape:
                    errs.append(f"{name}: a gradient of shape {None if g is None else tuple(g.shape)} for {tuple(t.shape)}")
            kinds = ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
            for nm, got, ref, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), c["ref"], kinds):
                want = SW.shard(c, ref, rank, (2 if dense else 1) if nm == "lse" else rd)
                m = _tol.metrics(got, want)
                notes.append(f"{name}.{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}.{nm}", got, want, kd, c.get("tol_scale", 1.0))
        ret[("notes", rank)] = notes
        ret[rank] = errs
    except Exception:
        ret[rank] = [f"rank {rank} crashed:\n{traceback.format_exc()}"]
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=240):
    """one world under its own time limit; returns (complaints, measured figures)"""
    import time

    import torch.multiprocessing as mp

    cases = [c if c.get("refuse") else dict(c, ref=reference(c)) for c in cases]
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, cases, use_hip, ret), nprocs=W, join=False)
    deadline = time.time() + limit_s
    while not ctx.join(timeout=1):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            return [f"world of {W} ranks did not finish within {limit_s} s"], []
    errs, notes = [], []
    for r in range(W):
        errs += list(ret.get(r, [f"rank {r} returned nothing"]))
        notes += list(ret.get(("notes", r), []))
    return errs, notes
