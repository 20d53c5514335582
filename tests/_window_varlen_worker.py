"""Multi-process worker of the sliding-window tests of the packed (varlen) ring and zigzag schedules and of the stripe
schedule: one rank of a gloo world runs the public functions on its shard of seeded sequences and compares, sequence by
sequence, with ONE windowed attention over the unsharded sequence (oracle.flash_attn_ref.full_attention_fp64).  Backend:
the CPU oracle with `mask_shift` and `mask_shift_lens` (tests/_ref_backend.py) or the HIP kernels with every rank
sharing cuda:0.  Case kinds:
    ring_varlen / zigzag_varlen   lens = the FULL lengths of the packed sequences, multiples of 2 W
    stripe                        dense, S rows per rank, token i of rank r = global token i W + r
    refuse                        a backend without `serves_mask_shift_lens` must be refused before any exchange"""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _window_worker import Counting as _Counting, _cmp        # noqa: E402


class Counting(_Counting):
    @staticmethod
    def _sig(name, a, kw):
        keys = ("causal", "window", "mask_shift", "mask_shift_lens", "acc_init", "phases", "q_half", "k_half")
        return (name, tuple(tuple(t.shape) for t in a[:3]), tuple((k_, kw[k_]) for k_ in keys if k_ in kw),
                tuple(sorted(k_ for k_ in kw if k_.startswith(("out", "lse", "dq", "dk", "dv")) and kw[k_] is not None)))


def stripe_skipped(a, wl, W):
    """the issue's rule: the block of queries of rank rq against keys of rank rk (a = rq - rk) holds no visible element
    iff floor(a / W) - ceil((a - wl) / W) < 0"""
    import math

    return math.floor(a / W) - math.ceil((a - wl) / W) < 0


def _varlen(c):
    return c["kind"] in ("ring_varlen", "zigzag_varlen")


def _inputs(c):
    g = torch.Generator().manual_seed(c["seed"])
    W, H, Hk, D = c["W"], c["H"], c["Hk"], c["D"]
    dt = c.get("dtype", torch.bfloat16)
    if _varlen(c):
        T = sum(c["lens"])
        mk = lambda h: torch.randn(T, h, D, generator=g).to(dt)
    else:
        mk = lambda h: torch.randn(c.get("B", 1), W * c["S"], h, D, generator=g).to(dt)
    return mk(H), mk(Hk), mk(Hk), mk(H)


def _reference(c, q, k, v, do, dev):
    """per sequence, ONE windowed attention over the unsharded sequence in fp64 with autograd; returns out, lse, dq, dk, dv
    with out / grads laid out like the inputs and lse as (H, T) (packed) or (B, H, S) (dense)"""
    from oracle import flash_attn_ref as O

    if not _varlen(c):
        qd, kd, vd = (t.to(dev).double().requires_grad_(True) for t in (q, k, v))
        out, lse = O.full_attention_fp64(qd, kd, vd, c["causal"], window=c["window"])
        out.backward(do.to(dev).double())
        return [t.detach().cpu() for t in (out, lse, qd.grad, kd.grad, vd.grad)]
    parts = [[] for _ in range(5)]
    s = 0
    for L in c["lens"]:
        qd, kd, vd = (t[s:s + L].unsqueeze(0).to(dev).double().requires_grad_(True) for t in (q, k, v))
        out, lse = O.full_attention_fp64(qd, kd, vd, c["causal"], window=c["window"])
        out.backward(do[s:s + L].unsqueeze(0).to(dev).double())
        for lst, t in zip(parts, (out[0], lse[0], qd.grad[0], kd.grad[0], vd.grad[0])):
            lst.append(t.detach().cpu())
        s += L
    return [torch.cat(lst, dim=1 if n == 1 else 0) for n, lst in enumerate(parts)]


def _shard(c, t, rank, dim):
    """this rank's rows of `t` along `dim`"""
    W = c["W"]
    if c["kind"] == "stripe":
        return t.narrow(dim, rank, t.shape[dim] - rank).index_select(dim, torch.arange(0, t.shape[dim] - rank, W)).contiguous()
    out, s = [], 0
    for L in c["lens"]:
        seq = t.narrow(dim, s, L)
        if c["kind"] == "ring_varlen":
            out.append(seq.chunk(W, dim=dim)[rank])
        else:
            ch = seq.chunk(2 * W, dim=dim)
            out += [ch[rank], ch[2 * W - 1 - rank]]
        s += L
    return torch.cat(out, dim=dim).contiguous()


def _call(R, c, form, q, k, v, window, dev):
    kw = dict(causal=c["causal"], window_size=window, return_attn_probs=True)
    pre = {"ring_varlen": "ring_flash_attn_varlen", "zigzag_varlen": "zigzag_ring_flash_attn_varlen",
           "stripe": "stripe_flash_attn"}[c["kind"]]
    lead, pd = (), 2
    if _varlen(c):
        local = [L // c["W"] for L in c["lens"]]
        cu = torch.tensor([0] + list(torch.tensor(local).cumsum(0).tolist()), dtype=torch.int32, device=dev)
        lead, pd = (cu, max(local)), 1
    if form == "func":
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out, lse, _ = getattr(R, pre + "_func")(*ins, *lead, **kw)
        grads = lambda: (ins[0].grad, ins[1].grad, ins[2].grad)
    elif form == "kvpacked":
        qq, kv = q.clone().requires_grad_(True), torch.stack([k, v], dim=pd).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_kvpacked_func")(qq, kv, *lead, **kw)
        grads = lambda: (qq.grad, kv.grad.select(pd, 0), kv.grad.select(pd, 1))
    else:
        qkv = torch.stack([q, k, v], dim=pd).requires_grad_(True)
        out, lse, _ = getattr(R, pre + "_qkvpacked_func")(qkv, *lead, **kw)
        grads = lambda: (qkv.grad.select(pd, 0), qkv.grad.select(pd, 1), qkv.grad.select(pd, 2))
    return out, lse, grads


def _check_stripe_log(tag, log, rank, W, wl, errs):
    """the forward issues, in step order, exactly the blocks the rule does not skip, each with the rule's band"""
    import math

    want = []
    for step in range(W):
        a = rank - (rank - step) % W
        if stripe_skipped(a, wl, W):
            continue
        hi = math.floor(a / W)
        want.append((hi, (hi - math.ceil((a - wl) / W), -1)))
    got = [(dict(e[2]).get("mask_shift", 0), tuple(dict(e[2])["window"])) for e in log if e[0] == "fwd"]
    if got != want:
        errs.append(f"{tag}: forward blocks (mask_shift, window) {got}, the rule gives {want}")
    n_bwd = len([e for e in log if e[0] == "bwd" and not (dict(e[2]).get("phases", 0) & 2)])
    if n_bwd != len(want):
        errs.append(f"{tag}: {n_bwd} backward blocks, the rule gives {len(want)}")


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config, utils
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
            inner, tol = RefBackend(serves=("mask_shift", "mask_shift_lens")), TOL_ORACLE
        errs = []
        hops = [0]
        orig_commit = utils.RingComm.commit

        def counting_commit(self):
            hops[0] += 1
            return orig_commit(self)

        utils.RingComm.commit = counting_commit
        for c0 in cases:
            name = c0["name"]
            if c0.get("exchange"):
                os.environ["RFA_ZIGZAG_VARLEN_EXCHANGE"] = c0["exchange"]
                config.reload()
            for form in c0.get("forms", ("func",)):
                # (the qkv-packed entry points need as many K/V heads as query heads: that form runs the case as MHA)
                c = dict(c0, Hk=c0["H"]) if form == "qkvpacked" else c0
                if c.get("refuse"):
                    c = dict(c, kind=c["refuse"])
                q, k, v, do = _inputs(c)
                tag = f"{name}[{form}][r{rank}]"
                if c.get("refuse"):
                    from _ref_backend import RefBackend

                    ql, kl, vl = (_shard(c, t, rank, 0).to(dev) for t in (q, k, v))
                    _testing.set_backend(Counting(RefBackend(serves=("mask_shift",))))
                    hops[0] = 0
                    try:
                        _call(R, c, form, ql, kl, vl, c["window"], dev)
                        errs.append(f"{tag}: a backend without serves_mask_shift_lens was not refused")
                    except NotImplementedError as e:
                        if "mask_shift_lens" not in str(e):
                            errs.append(f"{tag}: refused with {e!r}")
                    if hops[0]:
                        errs.append(f"{tag}: {hops[0]} exchanges before the refusal")
                    continue
                ref = None
                if rank == 0 or not use_hip:
                    ref = _reference(c, q, k, v, do, dev if use_hip else torch.device("cpu"))
                if use_hip:
                    # (one fp64 reference per world, computed by rank 0 on the device, handed round as CPU tensors)
                    box = [ref]
                    dist.broadcast_object_list(box, src=0)
                    ref = box[0]
                rd = 0 if _varlen(c) else 1
                ql, kl, vl, dol = (_shard(c, t, rank, rd).to(dev) for t in (q, k, v, do))
                be = Counting(inner)
                _testing.set_backend(be)
                out, lse, grads = _call(R, c, form, ql, kl, vl, c["window"], dev)
                out.backward(dol)
                dq, dk, dv = grads()
                for nm, got, r_, kind in (("out", out, ref[0], "out"), ("lse", lse, ref[1], "lse"), ("dq", dq, ref[2], "grad"),
                                          ("dk", dk, ref[3], "grad"), ("dv", dv, ref[4], "grad")):
                    want = _shard(c, r_, rank, (1 if _varlen(c) else 2) if nm == "lse" else rd)
                    _cmp(f"{tag}.{nm}", got.detach().cpu().float(), want.float(), tol[kind], errs)
                if c["kind"] == "stripe" and "skips" in c.get("check", ()):
                    _check_stripe_log(tag, be.log, rank, W, c["window"][0], errs)
                if "same_as_unwindowed" in c.get("check", ()):
                    # a window that covers the whole of the longest sequence is dropped on the host: the unwindowed
                    # call's bits and calls
                    be2 = Counting(inner)
                    _testing.set_backend(be2)
                    out2, lse2, grads2 = _call(R, c, form, ql, kl, vl, (-1, -1), dev)
                    out2.backward(dol)
                    for nm, a_, b_ in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, dq, dk, dv), (out2, lse2) + tuple(grads2())):
                        if not torch.equal(a_.detach(), b_.detach()):
                            errs.append(f"{tag}.{nm}: differs from the unwindowed call")
                    if be.log != be2.log:
                        errs.append(f"{tag}: backend calls differ from the unwindowed call's")
                    if any("mask_shift" in dict(e[2]) or "mask_shift_lens" in dict(e[2])
                           or tuple(dict(e[2]).get("window", (-1, -1))) != (-1, -1) for e in be2.log):
                        errs.append(f"{tag}: an unwindowed call passed a window or a shift to the backend")
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
            return [f"world of {W} ranks did not finish within {limit_s} s"]
    errs = []
    for r in range(W):
        errs += list(ret.get(r, [f"rank {r} returned nothing"]))
    return errs
