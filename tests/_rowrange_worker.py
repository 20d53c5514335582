"""Worker of the multi-rank tests of per-row key ranges (ring_flash_attn.with_row_ranges): one gloo rank runs a public function
on its shard of a seeded sequence with its shard of the GLOBAL (start, end) and compares out, lse, dq, dk, dv with its shard
of ONE single-device fp64 autograd attention with the explicit boolean mask (tests/_rowrange_backend.py: single_device) that
the parent made once — and checks that the result is NOT within tolerance of the same attention without the ranges.
Backend: the CPU test backend with `serves_row_ranges` or the HIP kernels with every rank sharing cuda:0 (host staging).
A case with `refuse` names the exception the call (or the bind) must raise on EVERY rank before anything is exchanged: no block
call is made, and a barrier afterwards finds every rank in step.  A case with `union` runs the recipe for a union of
intervals: a window plus G global tokens as two ranged calls under with_lse_grad, joined by merge_attn."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _rowrange_backend as RB                                # noqa: E402
import _tol                                                   # noqa: E402

B, H, HK = 2, 4, 2
FUNCS = {"ring": "ring_flash_attn", "zigzag": "zigzag_ring_flash_attn"}


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}{'-' + c['pack'] if c.get('pack') else ''}-W{c['W']}-S{c['S']}-" \
           f"D{c.get('D', 64)}-{c['pattern']}-{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}" \
           f"{'-' + c['refuse'] + '-' + c['how'] if c.get('refuse') else ''}{'-union' if c.get('union') else ''}"


def ranges(c):
    """GLOBAL (start, end), int32 (B, T), of the case's pattern over T = W S rows"""
    T = c["W"] * c["S"]
    i = torch.arange(T)
    g = torch.Generator().manual_seed(7 + T)
    if c["pattern"] == "doc":                                   # documents of uneven lengths, off every chunk boundary
        cuts = [0] + sorted({max(1, int(T * f)) for f in (0.11, 0.37, 0.52, 0.9)}) + [T]
        doc = torch.bucketize(i, torch.tensor(cuts[1:-1]), right=True)
        lo, hi = torch.tensor(cuts)[doc], torch.tensor(cuts)[doc + 1]
        start, end = torch.stack([lo, lo]), torch.stack([hi, hi])
        end[1] = torch.minimum(end[1], start[1] + 40)           # (batch entry 1: the first 40 keys of the row's document)
    elif c["pattern"] == "prefix":                              # prefix-LM: the prefix sees itself, the rest is causal
        P = T // 3 + 5
        start = torch.zeros(B, T, dtype=torch.long)
        end = torch.maximum(i + 1, torch.tensor(P)).expand(B, T).clone()
        end[1] = torch.maximum(i + 1, torch.tensor(T // 2 + 1))
    elif c["pattern"] == "random":                              # random intervals, out-of-range values, some empty rows
        start = torch.randint(-20, T, (B, T), generator=g)
        end = start + torch.randint(-10, T, (B, T), generator=g)
        end[:, ::7] = start[:, ::7]                             # every 7th row is empty
        end[0, 5] = 2 ** 31 - 1
        start[1, 9] = -2 ** 31
    elif c["pattern"] == "window_part":                         # the union recipe's first part: the causal window of w keys
        w = c["w"]
        start, end = (i - w + 1).clamp(min=c["G"]).expand(B, T).clone(), (i + 1).expand(B, T).clone()
    elif c["pattern"] == "global_part":                         # ... and its second: the G global tokens (causal)
        start, end = torch.zeros(B, T, dtype=torch.long), torch.minimum(i + 1, torch.tensor(c["G"])).expand(B, T).clone()
    else:
        raise ValueError(c["pattern"])
    return start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous()


def inputs(c):
    g = torch.Generator().manual_seed(41)
    mk = lambda h: torch.randn(B, c["W"] * c["S"], h, c.get("D", 64), generator=g).to(c.get("dtype", torch.bfloat16))
    hq = HK if c.get("pack") == "qkv" else H                   # (a packed qkv has one head count)
    return mk(hq), mk(HK), mk(HK), mk(hq)


def reference(c):
    """(ranged reference, the same call without ranges): each (out, lse, dq, dk, dv) fp64"""
    q, k, v, do = inputs(c)
    T = q.shape[1]
    win = tuple(c.get("window", (-1, -1)))
    if c.get("union"):
        i = torch.arange(T)
        mask = ((i.view(-1, 1) - i.view(1, -1) < c["w"]) | (i.view(1, -1) < c["G"])) & (i.view(1, -1) <= i.view(-1, 1))
        mask = mask.expand(B, T, T)
    else:
        mask = RB.mask_of(*ranges(c), c["causal"], win)
    full = RB.mask_of(torch.zeros(B, T, dtype=torch.int32), torch.full((B, T), T, dtype=torch.int32), c["causal"], win)
    return RB.single_device(q, k, v, do, mask), RB.single_device(q, k, v, do, full)


def shard(c, t, rank, dim):
    W = c["W"]
    if c["kind"] == "ring":
        return t.chunk(W, dim=dim)[rank].contiguous()
    ch = t.chunk(2 * W, dim=dim)
    return torch.cat([ch[rank], ch[2 * W - 1 - rank]], dim=dim).contiguous()


def call(R, c, fn_name, start, end, q, k, v, **more):
    """the case's public function (plain or a packed form), bound to (start, end); returns (out, lse)"""
    pack = c.get("pack")
    fn = getattr(R, f"{FUNCS[c['kind']]}_{pack + 'packed_' if pack else ''}func") if fn_name is None else fn_name
    if c.get("lse_grad"):
        fn = R.with_lse_grad(fn)
    attn = R.with_row_ranges(fn, start, end)
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True, **more)
    if pack == "kv":
        out, lse, _ = attn(q, torch.stack([k, v], dim=2), **kw)
    elif pack == "qkv":
        out, lse, _ = attn(torch.stack([q, k, v], dim=2), **kw)
    else:
        out, lse, _ = attn(q, k, v, **kw)
    return out, lse


def _refusal(R, c, start, end, q, k, v, dev, be_cpu, _testing):
    how, more = c["how"], {}
    rec = RB.Recording(be_cpu)
    if how == "backend":                                        # a backend without serves_row_ranges
        from _ref_backend import RefBackend

        rec = RB.Recording(RefBackend(serves=("mask_shift", "mask_shift_lens")))
    _testing.set_backend(rec)
    fn = None
    if how == "dropout":
        more["dropout_p"] = 0.1
    elif how == "alibi":
        more["alibi_slopes"] = torch.full((H,), 0.1, dtype=torch.float32, device=dev)
    elif how == "head_dim":
        q, k, v = (torch.cat([t, t, t], dim=-1) for t in (q, k, v))             # 192
    elif how == "vdim":
        q, k = (torch.cat([t, t, t], dim=-1) for t in (q, k))                   # 192 / 64
    elif how == "dtype":
        start = start.long()
    elif how == "shape":
        start, end = start[:, :-1].contiguous(), end[:, :-1].contiguous()
    elif how == "contiguity":
        start = start.t().contiguous().t()
    elif how == "one_of_two":
        end = None
    elif how == "device":
        start, end = start.to("meta"), end.to("meta")
    elif how.startswith("func:"):
        fn = {"varlen": R.ring_flash_attn_varlen_func, "zigzag_varlen": R.zigzag_ring_flash_attn_varlen_func,
              "stripe": R.stripe_flash_attn_func, "llama3": R.llama3_flash_attn_varlen_func,
              "zigzag_llama3": R.zigzag_llama3_flash_attn_varlen_func,
              "softcap": R.with_softcap(R.ring_flash_attn_func, 30.0),
              "sinks": R.with_sinks(R.ring_flash_attn_func, torch.zeros(H)),
              "max_logit": R.with_max_logit(R.ring_flash_attn_func, torch.full((H,), float("-inf"))),
              "ulysses": R.with_ulysses(R.ring_flash_attn_func, dist.new_group(list(range(c["W"])))),
              "row_ranges": R.with_row_ranges(R.ring_flash_attn_func, start, end),
              "lambda": (lambda *a, **k_: None)}[how[5:]]
    want = {"ValueError": ValueError, "NotImplementedError": NotImplementedError, "TypeError": TypeError}[c["refuse"]]
    try:
        call(R, c, fn, start, end, q, k, v, **more)
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


def _union(R, c, rank, dev, q, k, v):
    """window of w keys plus G global tokens = two disjoint intervals per row: two ranged calls, merged"""
    fn = R.with_lse_grad(getattr(R, FUNCS[c["kind"]] + "_func"))
    parts = []
    for pattern in ("window_part", "global_part"):
        s, e = (shard(c, t, rank, 1).to(dev) for t in ranges(dict(c, pattern=pattern)))
        o, l, _ = R.with_row_ranges(fn, s, e)(q, k, v, causal=True, return_attn_probs=True)
        parts += [o, l]
    return R.merge_attn(*parts)


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config

        be_cpu = RB.RowRangeBackend()
        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        errs, notes = [], []
        for c in cases:
            name = f"{case_name(c)}[r{rank}]"
            q, k, v, do = (shard(c, t, rank, 1).to(dev) for t in inputs(c))
            q, k, v = (t.requires_grad_(True) for t in (q, k, v))
            start, end = (shard(c, t, rank, 1).to(dev) for t in ranges(c))
            if c.get("refuse"):
                bad = _refusal(R, c, start, end, q, k, v, dev, be_cpu, _testing)
                if bad:
                    errs.append(f"{name}: {bad}")
                continue
            rec = RB.Recording(be_cpu)
            _testing.set_backend(None if use_hip else rec)
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                if c.get("union"):
                    out, lse = _union(R, c, rank, dev, q, k, v)
                else:
                    out, lse = call(R, c, None, start, end, q, k, v)
                out.backward(do)
            if not use_hip and not all(n is not None and n[1] == n[2] for n in rec.seen["fwd"] + rec.seen["bwd"]):
                errs.append(f"{name}: a block call without ranges, or with ranges that are not its query rows': {rec.seen}")
            kinds = ("out", "lse", "grad", "grad", "grad") if W == 1 else ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
            far = False
            for j, (nm, got, kd) in enumerate(zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), kinds)):
                want = shard(c, c["ref"][j], rank, 2 if nm == "lse" else 1)
                m = _tol.metrics(got, want)
                notes.append(f"{name}.{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}.{nm}", got, want, kd, c.get("tol_scale", 1.0))
                # ... and a call that ignored the ranges would land on the un-ranged attention
                far = far or bool(_tol.failures("", got, shard(c, c["ref0"][j], rank, 2 if nm == "lse" else 1), kd))
            if not far:
                errs.append(f"{name}: within tolerance of the attention WITHOUT the ranges — the test cannot see them")
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

    done = []
    for c in cases:
        if not c.get("refuse"):
            ref, ref0 = reference(c)
            c = dict(c, ref=ref, ref0=ref0)
        done.append(c)
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, done, use_hip, ret), nprocs=W, join=False)
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
