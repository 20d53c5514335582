"""Worker of the multi-rank soft-capping tests: one gloo rank runs `with_softcap(<public function>, cap)` on its shard of a
seeded sequence and compares with its shard of ONE single-device capped call (tests/_blockref.py, fp64) that the parent
computed once; or, `record`, runs under a recording backend and reports the `softcap` every block call carried.  Backend:
the CPU oracle with `softcap=` (tests/_ref_backend.py) or the HIP kernels with every rank sharing cuda:0.  Kinds:
    ring / zigzag / stripe            dense (B, W S, H, D)
    ring_varlen / zigzag_varlen       packed, `lens` = the FULL lengths of the sequences (multiples of 2 W)
    llama3 / zigzag_llama3            packed stream of W S tokens, sequences L3_CU scaled"""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _tol                                                   # noqa: E402

B, H, HK = 2, 4, 2
L3_CU = [0, 7, 14, 16]
FUNCS = {"ring": "ring_flash_attn_func", "zigzag": "zigzag_ring_flash_attn_func", "stripe": "stripe_flash_attn_func",
         "ring_varlen": "ring_flash_attn_varlen_func", "zigzag_varlen": "zigzag_ring_flash_attn_varlen_func",
         "llama3": "llama3_flash_attn_varlen_func", "zigzag_llama3": "zigzag_llama3_flash_attn_varlen_func"}
DENSE = ("ring", "zigzag", "stripe")


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-D{c.get('D', 64)}-" \
           f"{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}-cap{c['softcap']}"


def lens_of(c):
    """full lengths of the packed sequences (None: dense)"""
    if c["kind"] in DENSE:
        return None
    if c["kind"] in ("llama3", "zigzag_llama3"):
        m = c["W"] * c["S"] // L3_CU[-1]
        return [(b - a) * m for a, b in zip(L3_CU, L3_CU[1:])]
    return list(c["lens"])


def inputs(c):
    D = c.get("D", 64)
    g = torch.Generator().manual_seed(23)
    lens = lens_of(c)
    lead = (B, c["W"] * c["S"]) if lens is None else (sum(lens),)
    mk = lambda h: torch.randn(*lead, h, D, generator=g).bfloat16()
    return mk(H), mk(HK), mk(HK), mk(H)


def reference(c, softcap=None):
    """(out, lse, dq, dk, dv) fp64 of the ONE single-device call over the unsharded tensors"""
    import _blockref as SR

    q, k, v, do = inputs(c)
    kw = dict(causal=c["causal"], window=c.get("window", (-1, -1)), dout=do)
    lens = lens_of(c)
    if lens is not None:
        cu = [0]
        for L in lens:
            cu.append(cu[-1] + L)
        kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu)
    return SR.attention(q, k, v, softcap=c["softcap"] if softcap is None else softcap, **kw)


def shard(c, t, rank, dim):
    W, kind = c["W"], c["kind"]
    if kind in ("ring", "llama3"):
        return t.chunk(W, dim=dim)[rank].contiguous()
    if kind in ("zigzag", "zigzag_llama3"):
        ch = t.chunk(2 * W, dim=dim)
        return torch.cat([ch[rank], ch[2 * W - 1 - rank]], dim=dim).contiguous()
    if kind == "stripe":
        return t.index_select(dim, torch.arange(rank, t.shape[dim], W)).contiguous()
    out, s = [], 0
    for L in c["lens"]:
        seq = t.narrow(dim, s, L)
        if kind == "ring_varlen":
            out.append(seq.chunk(W, dim=dim)[rank])
        else:
            ch = seq.chunk(2 * W, dim=dim)
            out += [ch[rank], ch[2 * W - 1 - rank]]
        s += L
    return torch.cat(out, dim=dim).contiguous()


def call(R, c, q, k, v, rank, dev):
    fn = R.with_softcap(getattr(R, FUNCS[c["kind"]]), c["softcap"])
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True)
    kind = c["kind"]
    if kind in DENSE:
        return fn(q, k, v, **kw)
    if kind in ("ring_varlen", "zigzag_varlen"):
        local = [L // c["W"] for L in c["lens"]]
        cu = torch.tensor([0] + torch.tensor(local).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        return fn(q, k, v, cu, max(local), **kw)
    lens = lens_of(c)
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
        from _ref_backend import Recording, RefBackend

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        errs, notes = [], []
        for c in cases:
            name = case_name(c)
            dense = c["kind"] in DENSE
            rd = 1 if dense else 0
            q, k, v, do = (shard(c, t, rank, rd).to(dev) for t in inputs(c))
            q, k, v = (t.requires_grad_(True) for t in (q, k, v))
            rec = None
            if c.get("record"):
                rec = Recording(RefBackend(serves=("mask_shift",)))
                _testing.set_backend(rec)
            else:
                _testing.set_backend(None if use_hip else RefBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                out, lse, _ = call(R, c, q, k, v, rank, dev)
                out.backward(do)
            if rec is not None:
                for which in ("fwd", "bwd"):
                    seen = rec.seen[which]
                    if not seen or any(x != c["softcap"] for x in seen):
                        errs.append(f"{name}[r{rank}]: {which} block calls carried softcap {seen}, want {c['softcap']} on each")
                continue
            kinds = ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
            for nm, got, ref, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), c["ref"], kinds):
                want = shard(c, ref, rank, (2 if dense else 1) if nm == "lse" else rd)
                m = _tol.metrics(got, want)
                notes.append(f"{name}[r{rank}].{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}[r{rank}].{nm}", got, want, kd)
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
    """one world under its own time limit; returns (complaints, measured figures).  Cases without `record` get the ONE
    fp64 reference here, before the ranks start."""
    import time

    import torch.multiprocessing as mp

    cases = [c if c.get("record") else dict(c, ref=reference(c)) for c in cases]
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
