"""Worker of the multi-rank ALiBi tests (dense ring, zigzag, llama3): one gloo rank runs the public functions with
alibi_slopes on its shard of a seeded sequence and hands out / lse / dq / dk / dv back; the parent un-shards them by the
schedule's own layout and compares with ONE single-device biased call (tests/_blockref.py, fp64).  Backend: the CPU
oracle with `alibi=` (tests/_ref_backend.py) or the HIP kernels with every rank sharing cuda:0."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _droppos_worker import PREFIX, shard, unshard           # noqa: E402  (the schedules' layouts)

B, H, HK, D = 2, 4, 2, 64
L3_CU = [0, 7, 14, 16]                                       # the reference's llama3 fixture, scaled by c["S"] // 16 per rank


def case_name(c):
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-" \
           f"{'causal' if c['causal'] else 'full'}-{c.get('api', 'func')}-{c.get('slopes', 'H')}"


def slopes_of(c):
    """2^(-8 (h + 1) / H) per head; the (B, H) case scales batch entry b by 1 + b / 2"""
    s = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)
    if c.get("slopes") == "BH":
        s = torch.stack([s * (1 + 0.5 * b) for b in range(B)])
    return s


def l3_cu(c):
    m = c["W"] * c["S"] // L3_CU[-1]
    return torch.tensor([x * m for x in L3_CU], dtype=torch.int32)


def inputs(c):
    """the unsharded (q, k, v, dout) of a case; a qkv-packed case runs as MHA; llama3: packed (T, H, D)"""
    hk = H if c.get("api") == "qkvpacked" else HK
    g = torch.Generator().manual_seed(11)
    lead = (c["W"] * c["S"],) if c["kind"] == "llama3" else (B, c["W"] * c["S"])
    mk = lambda h: torch.randn(*lead, h, D, generator=g).bfloat16()
    return mk(H), mk(hk), mk(hk), mk(H)


def call(R, c, q, k, v, slopes, rank, dev):
    kw = dict(causal=c["causal"], return_attn_probs=True, alibi_slopes=slopes)
    api = c.get("api", "func")
    if c["kind"] == "llama3":
        cq, ck, mq, mk, sl = R.llama3_flash_attn_prepare_cu_seqlens(l3_cu(c), c["causal"], rank, c["W"])
        args = (cq.to(dev), ck.to(dev), mq, mk)
        kw.update(heads_k_stride=c.get("stride", 1), local_k_slice=sl)
        pre, pack = "llama3_flash_attn_varlen", 1
    else:
        args, pre, pack = (), PREFIX[c["kind"]], 2
    if api == "func":
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, lse, _ = getattr(R, pre + "_func")(*ins, *args, **kw)
        return out, lse, lambda: (ins[0].grad, ins[1].grad, ins[2].grad)
    if api == "kvpacked":
        qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=pack).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_kvpacked_func")(qq, kv, *args, **kw)
        return out, lse, lambda: (qq.grad, kv.grad.select(pack, 0), kv.grad.select(pack, 1))
    qkv = torch.stack([q, k, v], dim=pack).requires_grad_(True)
    out, lse, _ = getattr(R, pre + "_qkvpacked_func")(qkv, *args, **kw)
    return out, lse, lambda: tuple(qkv.grad.select(pack, i) for i in range(3))


def _refusals(R, rank, W, dev):
    """what must raise on a multi-rank group — NotImplementedError before anything is exchanged, ValueError for slopes
    that are not fp32 (H,) / (B, H) on the device: list of complaints"""
    from _ref_backend import RefBackend
    from ring_flash_attn import _api, _testing, utils

    bad = []
    posted = [0]
    orig = utils.RingComm.commit, utils.AllGatherComm.all_gather, utils.SourceArrivals.post

    def counted(fn):
        def wrapper(*a, **kw):
            posted[0] += 1
            return fn(*a, **kw)
        return wrapper

    utils.RingComm.commit, utils.AllGatherComm.all_gather, utils.SourceArrivals.post = (counted(f) for f in orig)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(1, 64, 2, 32, generator=g).bfloat16().to(dev)
    sl = torch.tensor([0.25, 0.0625], dtype=torch.float32, device=dev)

    def raises(exc, what, fn, *a, **kw):
        try:
            fn(*a, **kw)
            bad.append(f"r{rank}: {what} did not raise")
        except exc:
            pass
        except Exception as e:                                   # noqa: BLE001 — reported to the parent
            bad.append(f"r{rank}: {what} raised {type(e).__name__}: {e}")

    try:
        NI = NotImplementedError
        raises(NI, "stripe", R.stripe_flash_attn_func, q, q, q, causal=True, alibi_slopes=sl)
        cu = torch.tensor([0, 24, 64], dtype=torch.int32)
        qv = q[0]
        for fn in (R.ring_flash_attn_varlen_func, R.zigzag_ring_flash_attn_varlen_func):
            raises(NI, fn.__name__, fn, qv, qv, qv, cu, 40, causal=True, alibi_slopes=sl)
        cu_all = torch.tensor([0, 24 * W, 64 * W], dtype=torch.int32)
        raises(NI, "zigzag_llama3", R.zigzag_llama3_flash_attn_varlen_func, qv, qv, qv, cu_all, causal=True, alibi_slopes=sl)
        cq, ck, mq, mk, ks = R.llama3_flash_attn_prepare_cu_seqlens(cu_all, False, rank, W)
        raises(NI, "non-causal llama3", R.llama3_flash_attn_varlen_func, qv, qv, qv, cq, ck, mq, mk, heads_k_stride=1,
               local_k_slice=ks, causal=False, alibi_slopes=sl)
        for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func):
            raises(NI, fn.__name__ + " with a window", fn, q, q, q, causal=True, window_size=(8, 0), alibi_slopes=sl)
            raises(NI, fn.__name__ + " with dropout", fn, q, q, q, causal=True, dropout_p=0.1, alibi_slopes=sl)
            raises(ValueError, fn.__name__ + " with fp64 slopes", fn, q, q, q, causal=True, alibi_slopes=sl.double())
            raises(ValueError, fn.__name__ + " with (3,) slopes", fn, q, q, q, causal=True, alibi_slopes=torch.ones(3, device=dev))
        big = torch.randn(1, 64, 2, 136, generator=g).bfloat16().to(dev)
        raises(NI, "head dim 136", R.ring_flash_attn_func, big, big, big, causal=True, alibi_slopes=sl)
        # the torch.compile whole-schedule operators call the check without alibi_ok
        raises(NI, "the whole-schedule operator's check", _api._check_unsupported, 0.0, (-1, -1), sl, windows_ok=False)
        if dev.type == "cpu":
            _testing.set_backend(RefBackend(serves=("mask_shift",)))                  # serves mask_shift, not alibi
            for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func):
                raises(NI, fn.__name__ + " on a backend without alibi", fn, q, q, q, causal=True, alibi_slopes=sl)
        if posted[0]:
            bad.append(f"r{rank}: {posted[0]} exchanges were posted by calls that must be refused before any")
    finally:
        utils.RingComm.commit, utils.AllGatherComm.all_gather, utils.SourceArrivals.post = orig
    return bad


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
            backend = None                                       # the product's: HipBackend
        else:
            from _ref_backend import RefBackend

            dev = torch.device("cpu")
            backend = RefBackend(serves=("mask_shift", "alibi"))
        for c in cases:
            _testing.set_backend(backend)
            if c.get("refusals"):
                ret[("refusals", rank)] = _refusals(R, rank, W, dev)
                continue
            kind = "ring" if c["kind"] == "llama3" else c["kind"]
            dim = 0 if c["kind"] == "llama3" else 1
            q, k, v, do = (shard(kind, t, rank, W, dim=dim).to(dev) for t in inputs(c))
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                out, lse, grads = call(R, c, q, k, v, slopes_of(c).to(dev), rank, dev)
                out.backward(do)
            ret[(case_name(c), rank)] = tuple(t.detach().cpu() for t in (out, lse) + tuple(grads()))
        ret[rank] = "ok"
    except Exception:
        ret[rank] = f"rank {rank} crashed:\n{traceback.format_exc()}"
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=300):
    """one world under its own time limit; returns {case name: (out, lse, dq, dk, dv) un-sharded} and the complaints"""
    import time

    import torch.multiprocessing as mp

    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, cases, use_hip, ret), nprocs=W, join=False)
    deadline = time.time() + limit_s
    while not ctx.join(timeout=2):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            return {}, [f"world of {W} ranks did not finish within {limit_s} s"]
    got = dict(ret)
    errs = [got.get(r, f"rank {r} returned nothing") for r in range(W) if got.get(r) != "ok"]
    for r in range(W):
        errs += list(got.get(("refusals", r), []))
    res = {}
    if not errs:
        for c in cases:
            if c.get("refusals"):
                continue
            n = case_name(c)
            parts = [got[(n, r)] for r in range(W)]
            if c["kind"] == "llama3":                            # packed: rows along dim 0, lse (H, T)
                res[n] = tuple(torch.cat([p_[i] for p_ in parts], dim=1 if i == 1 else 0) for i in range(5))
            else:
                res[n] = tuple(unshard(c["kind"], [p_[i] for p_ in parts], dim=2 if i == 1 else 1) for i in range(5))
    return res, errs


def reference(c):
    """the ONE single-device biased call on the unsharded tensors, fp64 (tests/_blockref.py): (out, lse, dq, dk, dv), and
    the unbiased out (to see that the bias did something)"""
    import _blockref as AR

    q, k, v, do = inputs(c)
    kw = dict(causal=c["causal"], dout=do, autograd=True)
    if c["kind"] == "llama3":
        cu = l3_cu(c).tolist()
        kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu)
    ref = AR.attention(q, k, v, slopes=slopes_of(c), **kw)
    kw.pop("dout")
    return ref, AR.attention(q, k, v, **kw)[0]
