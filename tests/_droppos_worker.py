"""Worker of the multi-rank dropout tests (dense ring, zigzag, stripe): one gloo rank runs the public functions with
dropout on its shard of a seeded sequence and hands out / lse / dq / dk / dv back; the parent un-shards them by the
schedule's own layout and compares with ONE single-device dropout call with the same seed.  Every rank seeds torch alike
before each call, so all ranks — and the parent — draw the same dropout seed.  Backend: the CPU oracle with dropout
position maps (tests/_ref_backend.py) or the HIP kernels with every rank sharing cuda:0."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, P_DROP = 4242, 0.2
PREFIX = {"ring": "ring_flash_attn", "zigzag": "zigzag_ring_flash_attn", "stripe": "stripe_flash_attn"}


def case_name(c):
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-D{c.get('D', 64)}-" \
           f"{'causal' if c['causal'] else 'full'}-{c.get('api', 'func')}"


def inputs(c):
    """the unsharded (q, k, v, dout) of a case; a qkv-packed case runs as MHA"""
    B, H, D = c.get("B", 2), c.get("H", 4), c.get("D", 64)
    Hk = H if c.get("api") == "qkvpacked" else c.get("Hk", 2)
    g = torch.Generator().manual_seed(9)
    mk = lambda h: torch.randn(B, c["W"] * c["S"], h, D, generator=g).bfloat16()
    return mk(H), mk(Hk), mk(Hk), mk(H)


def shard(kind, t, r, W, dim=1):
    if kind == "ring":
        return t.chunk(W, dim=dim)[r].contiguous()
    if kind == "zigzag":
        ch = t.chunk(2 * W, dim=dim)
        return torch.cat([ch[r], ch[2 * W - 1 - r]], dim=dim).contiguous()
    return t.index_select(dim, torch.arange(r, t.shape[dim], W)).contiguous()


def unshard(kind, parts, dim=1):
    """the inverse of shard(): parts[r] is rank r's tensor"""
    W = len(parts)
    if kind == "ring":
        return torch.cat(list(parts), dim=dim)
    if kind == "zigzag":
        ch = [None] * (2 * W)
        for r, t in enumerate(parts):
            ch[r], ch[2 * W - 1 - r] = t.chunk(2, dim=dim)
        return torch.cat(ch, dim=dim)
    shape = list(parts[0].shape)
    shape[dim] *= W
    full = parts[0].new_empty(shape)
    for r, t in enumerate(parts):
        full.index_copy_(dim, torch.arange(r, shape[dim], W), t)
    return full


def call(R, c, q, k, v, dropout_p=P_DROP, **extra):
    kw = dict(dropout_p=dropout_p, causal=c["causal"], return_attn_probs=True, **extra)
    pre, api = PREFIX[c["kind"]], c.get("api", "func")
    if api == "func":
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, lse, _ = getattr(R, pre + "_func")(*ins, **kw)
        return out, lse, lambda: (ins[0].grad, ins[1].grad, ins[2].grad)
    if api == "kvpacked":
        qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_kvpacked_func")(qq, kv, **kw)
        return out, lse, lambda: (qq.grad, kv.grad[:, :, 0], kv.grad[:, :, 1])
    qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
    out, lse, _ = getattr(R, pre + "_qkvpacked_func")(qkv, **kw)
    return out, lse, lambda: (qkv.grad[:, :, 0], qkv.grad[:, :, 1], qkv.grad[:, :, 2])


def _refusals(R, rank, W, dev):
    """what must still raise on a multi-rank group, and that a backend without position maps is refused before anything
    is exchanged: list of complaints"""
    from oracle.oracle_backend import OracleBackend
    from ring_flash_attn import _testing, utils

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

    def raises(exc, what, fn, *a, **kw):
        try:
            fn(*a, **kw)
            bad.append(f"r{rank}: {what} did not raise")
        except exc:
            pass
        except Exception as e:                                   # noqa: BLE001 — reported to the parent
            bad.append(f"r{rank}: {what} raised {type(e).__name__}: {e}")

    try:
        cu = torch.tensor([0, 24, 64], dtype=torch.int32)
        qv = q[0]
        for fn in (R.ring_flash_attn_varlen_func, R.zigzag_ring_flash_attn_varlen_func):
            raises(NotImplementedError, fn.__name__, fn, qv, qv, qv, cu, 40, dropout_p=0.1, causal=True)
        for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
            raises(NotImplementedError, fn.__name__ + " with a window", fn, q, q, q, dropout_p=0.1, causal=True,
                   window_size=(8, 0))
            raises(ValueError, fn.__name__ + " with p = 1", fn, q, q, q, dropout_p=1.0, causal=True)
        if dev.type == "cpu":
            _testing.set_backend(OracleBackend())                # the frozen oracle: no position maps
            for fn in (R.ring_flash_attn_func, R.zigzag_ring_flash_attn_func, R.stripe_flash_attn_func):
                raises(NotImplementedError, fn.__name__ + " on a backend without position maps", fn, q, q, q,
                       dropout_p=0.1, causal=True)
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
            backend = RefBackend(serves=("dropout_positions",))
        for c in cases:
            if c.get("refusals"):
                _testing.set_backend(backend)
                ret[("refusals", rank)] = _refusals(R, rank, W, dev)
                continue
            _testing.set_backend(backend)
            q, k, v, do = (shard(c["kind"], t, rank, W).to(dev) for t in inputs(c))
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                torch.manual_seed(SEED)
                out, lse, grads = call(R, c, q, k, v)
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
            res[n] = tuple(unshard(c["kind"], [p_[i] for p_ in parts], dim=2 if i == 1 else 1) for i in range(5))
    return res, errs


def reference(c):
    """the single-device dropout call on the unsharded tensors with the seed every rank drew: (out, lse, dq, dk, dv) of
    oracle.flash_attn_ref, and the undropped out (to see that dropout did something)"""
    from oracle import flash_attn_ref as O
    from ring_flash_attn._common import draw_dropout_seed

    q, k, v, do = inputs(c)
    torch.manual_seed(SEED)
    rng = torch.tensor([draw_dropout_seed(), 0])
    scale = q.shape[-1] ** -0.5
    ro, rl, _, _ = O._flash_attn_forward(q, k, v, P_DROP, scale, c["causal"], rng_state=rng)
    r0 = O._flash_attn_forward(q, k, v, 0.0, scale, c["causal"])[0]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    O._flash_attn_backward(do, q, k, v, ro, rl, dq, dk, dv, P_DROP, scale, c["causal"], rng_state=rng)
    return (ro, rl, dq, dk, dv), r0
