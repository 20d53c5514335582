"""Worker of the multi-rank attention-sink tests: one gloo rank runs `with_sinks(<public function>, sinks)` on its shard of a
seeded sequence and compares out, lse, dq, dk, dv with its shard of ONE single-device call of the fp64 reference
(tests/_sinkref.py) that the parent computed once; its dsink — the partial over its own query rows — goes back to the parent,
which compares the SUM over the ranks with the reference's.  Backend: the CPU test backend with sinks
(tests/_sink_backend.py) or the HIP kernels with every rank sharing cuda:0.  Kinds, inputs and sharding are those of
tests/_softcap_worker.py."""
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

H, DENSE, FUNCS = SW.H, SW.DENSE, SW.FUNCS


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-D{c.get('D', 64)}-" \
           f"{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}-sinks"


def _ref_kw(c):
    kw = dict(causal=c["causal"], window=tuple(c.get("window", (-1, -1))))
    lens = SW.lens_of(c)
    if lens is not None:
        cu = [0]
        for L in lens:
            cu.append(cu[-1] + L)
        kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu)
    return kw


def draw_sinks(c):
    """(H,) fp32 around the mean lse of the case's attention WITHOUT sinks, +- 2: the sink column then takes a share of the
    softmax that is neither negligible nor everything"""
    import _sinkref as SK

    q, k, v, _ = SW.inputs(c)
    lse = SK.attention(q, k, v, None, **_ref_kw(c))[1]
    g = torch.Generator().manual_seed(41)
    return (lse[torch.isfinite(lse)].mean() + 4 * torch.rand(H, generator=g, dtype=torch.float64) - 2).float()


def reference(c, sinks):
    """(out, lse, dq, dk, dv, dsink) fp64 of the ONE single-device call over the unsharded tensors; sinks None: without"""
    import _sinkref as SK

    q, k, v, do = SW.inputs(c)
    return SK.attention(q, k, v, sinks, dout=do, **_ref_kw(c))


def call(R, c, sinks, q, k, v, rank, dev):
    fn = R.with_sinks(getattr(R, FUNCS[c["kind"]]), sinks)
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True)
    kind = c["kind"]
    if kind in DENSE:
        return fn(q, k, v, **kw)
    if kind in ("ring_varlen", "zigzag_varlen"):
        local = [L // c["W"] for L in c["lens"]]
        cu = torch.tensor([0] + torch.tensor(local).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        return fn(q, k, v, cu, max(local), **kw)
    lens = SW.lens_of(c)
    cu_all = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    if kind == "zigzag_llama3":
        return fn(q, k, v, cu_all, **kw)
    cq, ck, mq, mk, sl = R.llama3_flash_attn_prepare_cu_seqlens(cu_all, c["causal"], rank, c["W"])
    return fn(q, k, v, cq.to(dev), ck.to(dev), mq, mk, heads_k_stride=c.get("stride", 1), local_k_slice=sl, **kw)


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config
        from _sink_backend import SinkBackend

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        _testing.set_backend(None if use_hip else SinkBackend(serves=("mask_shift", "mask_shift_lens")))
        errs, notes, dsinks = [], [], []
        for c in cases:
            name = case_name(c)
            dense = c["kind"] in DENSE
            rd = 1 if dense else 0
            q, k, v, do = (SW.shard(c, t, rank, rd).to(dev) for t in SW.inputs(c))
            q, k, v = (t.requires_grad_(True) for t in (q, k, v))
            sinks = c["sinks"].to(dev).requires_grad_(True)
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                out, lse, _ = call(R, c, sinks, q, k, v, rank, dev)
                out.backward(do)
            kinds = ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
            for nm, got, ref, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), c["ref"], kinds):
                want = SW.shard(c, ref, rank, (2 if dense else 1) if nm == "lse" else rd)
                m = _tol.metrics(got, want)
                notes.append(f"{name}[r{rank}].{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}[r{rank}].{nm}", got, want, kd)
            if sinks.grad is None or sinks.grad.dtype != sinks.dtype or sinks.grad.shape != sinks.shape:
                errs.append(f"{name}[r{rank}]: sinks.grad is {sinks.grad!r}")
                dsinks.append(None)
            else:
                dsinks.append(sinks.grad.detach().double().cpu())
        ret[("notes", rank)] = notes
        ret[("dsink", rank)] = dsinks
        ret[rank] = errs
    except Exception:
        ret[rank] = [f"rank {rank} crashed:\n{traceback.format_exc()}"]
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=240):
    """one world under its own time limit; returns (complaints, measured figures).  Every case gets its sinks (unless it
    brings them) and the ONE fp64 reference here, before the ranks start; the ranks' dsink partials are summed here."""
    import time

    import torch.multiprocessing as mp

    full = []
    for c in cases:
        sinks = c["sinks"] if "sinks" in c else draw_sinks(c)
        full.append(dict(c, sinks=sinks, ref=reference(c, sinks)))
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, full, use_hip, ret), nprocs=W, join=False)
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
    if not errs:
        for i, c in enumerate(full):
            parts = [ret[("dsink", r)][i] for r in range(W)]
            total = torch.stack(parts).sum(0)
            m = _tol.metrics(total, c["ref"][5])
            notes.append(f"{case_name(c)}.dsink (sum of {W} ranks): max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}")
            errs += _tol.failures(f"{case_name(c)}.dsink", total, c["ref"][5], "grad_ring")
    return errs, notes
