"""Worker of the multi-rank tests of block-sparse masks (ring_flash_attn.with_block_mask): one gloo rank runs a public function
on its shard of a seeded sequence with ITS query blocks of the GLOBAL block mask (all key blocks) and compares out, lse, dq, dk,
dv with its shard of ONE single-device fp64 autograd attention with the expanded mask (tests/_blockmask_backend.py:
single_device) that the parent made once — and checks that the result is NOT within tolerance of the same attention without the
mask.  Backend: the CPU test backend with `serves_block_mask` or the HIP kernels with every rank sharing cuda:0 (host staging).
A case with `refuse` names the exception the call (or the bind) must raise on EVERY rank before anything is exchanged: no block
call is made, and a barrier afterwards finds every rank in step."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _blockmask_backend as MB                               # noqa: E402
import _tol                                                   # noqa: E402

B, H, HK = 2, 4, 2
BLOCK = 128
FUNCS = {"ring": "ring_flash_attn", "zigzag": "zigzag_ring_flash_attn"}


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}{'-' + c['pack'] if c.get('pack') else ''}-W{c['W']}-S{c['S']}-" \
           f"D{c.get('D', 32)}-{c['pattern']}-{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}" \
           f"{'-lse_grad' if c.get('lse_grad') else ''}{'-' + c['refuse'] + '-' + c['how'] if c.get('refuse') else ''}"


def heads_q(c):
    return HK if c.get("pack") == "qkv" else H                  # (a packed qkv has one head count)


def global_mask(c):
    """the GLOBAL block mask, bool (Bm, Hm, N, N) over the N = W S / 128 blocks of the unsharded sequence"""
    N = c["W"] * c["S"] // BLOCK
    r, col = torch.arange(N).view(-1, 1), torch.arange(N).view(1, -1)
    g = torch.Generator().manual_seed(17 + N)
    if c["pattern"] == "docs":                                  # block-diagonal documents of uneven lengths
        cuts = sorted({0, N} | {max(1, int(N * f)) for f in (0.3, 0.55)})
        doc = torch.bucketize(torch.arange(N), torch.tensor(cuts[1:-1]), right=True)
        m = (doc.view(-1, 1) == doc.view(1, -1)).view(1, 1, N, N)
        if N >= 4:                                              # (N = 2: one document per block, so that the mask removes something under causal)
            return m.contiguous()
        return (r == col).view(1, 1, N, N).contiguous()
    if c["pattern"] == "bigbird":                               # window + global + random blocks (fixed seed); block 1 is never global
        m = ((r - col).abs() <= (1 if N > 4 else 0)) | ((col == 0) & (N > 2)) | (torch.rand(N, N, generator=g) < 0.15)
        m[-1, 1:-1] = False                                     # (the last query block: its own and the global block only)
        if N <= 2:                                              # (two blocks: the window alone, or a causal call would see everything)
            m = r == col
        return m.view(1, 1, N, N).contiguous()
    if c["pattern"] == "per_head":                              # masks per query head (GQA: they differ inside a K/V group), per batch entry
        hq = heads_q(c)
        m = torch.rand(B, hq, N, N, generator=g) < 0.5
        m |= (r == col)                                         # (every row sees its diagonal block ...)
        m[:, 1::2] &= ~((r - col) == 1)                         # (... odd heads never the block in front of it, even heads always)
        m[:, 0::2] |= ((r - col) == 1)
        return m.contiguous()
    if c["pattern"] == "dark_rows":                             # query blocks with no lit key block at all
        m = ((r - col).abs() <= 1) | (col == 0)
        m = m.view(1, 1, N, N).repeat(B, 1, 1, 1)
        m[0, :, 1::2] = False
        m[1, :, 0] = False
        return m.contiguous()
    raise ValueError(c["pattern"])


def inputs(c):
    g = torch.Generator().manual_seed(43)
    mk = lambda h: torch.randn(B, c["W"] * c["S"], h, c.get("D", 32), generator=g).to(c.get("dtype", torch.bfloat16))
    hq = heads_q(c)
    return mk(hq), mk(HK), mk(HK), mk(hq)


def dlse_of(c):
    g = torch.Generator().manual_seed(47)
    return torch.randn(B, heads_q(c), c["W"] * c["S"], generator=g)


def reference(c):
    """(masked reference, the same call without the mask): each (out, lse, dq, dk, dv) fp64"""
    q, k, v, do = inputs(c)
    T = q.shape[1]
    win = tuple(c.get("window", (-1, -1)))
    dlse = dlse_of(c) if c.get("lse_grad") else None
    mask = MB.expand(global_mask(c), B, q.shape[2], T, T, c["causal"], win)
    full = MB.expand(torch.ones(1, 1, T // BLOCK, T // BLOCK, dtype=torch.bool), B, q.shape[2], T, T, c["causal"], win)
    return MB.single_device(q, k, v, do, mask, dlse), MB.single_device(q, k, v, do, full, dlse)


def shard(c, t, rank, dim):
    W = c["W"]
    if c["kind"] == "ring":
        return t.chunk(W, dim=dim)[rank].contiguous()
    ch = t.chunk(2 * W, dim=dim)
    return torch.cat([ch[rank], ch[2 * W - 1 - rank]], dim=dim).contiguous()


def call(R, c, fn_name, mask, q, k, v, **more):
    """the case's public function (plain or a packed form), bound to the mask; returns (out, lse)"""
    pack = c.get("pack")
    fn = getattr(R, f"{FUNCS[c['kind']]}_{pack + 'packed_' if pack else ''}func") if fn_name is None else fn_name
    if c.get("lse_grad"):
        fn = R.with_lse_grad(fn)
    attn = R.with_block_mask(fn, mask)
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True, **more)
    if pack == "kv":
        out, lse, _ = attn(q, torch.stack([k, v], dim=2), **kw)
    elif pack == "qkv":
        out, lse, _ = attn(torch.stack([q, k, v], dim=2), **kw)
    else:
        out, lse, _ = attn(q, k, v, **kw)
    return out, lse


def _refusal(R, c, mask, q, k, v, dev, be_cpu, _testing):
    how, more = c["how"], {}
    rec = MB.Recording(be_cpu)
    if how == "backend":                                        # a backend without serves_block_mask
        from _rowrange_backend import RowRangeBackend

        rec = MB.Recording(RowRangeBackend())
    _testing.set_backend(rec)
    fn = None
    if how == "dropout":
        more["dropout_p"] = 0.1
    elif how == "alibi":
        more["alibi_slopes"] = torch.full((H,), 0.1, dtype=torch.float32, device=dev)
    elif how == "head_dim":
        q, k, v = (torch.cat([t] * 5, dim=-1) for t in (q, k, v))                # 160
    elif how == "vdim":
        q, k = (torch.cat([t] * 5, dim=-1) for t in (q, k))                      # 160 / 32
    elif how == "group":                                        # 65 query heads on one K/V head
        q = q.repeat(1, 1, 17, 1)[:, :, :65].contiguous()
        k, v = k[:, :, :1].contiguous(), v[:, :, :1].contiguous()
    elif how == "dtype":
        mask = mask.to(torch.uint8)
    elif how == "shape":
        mask = mask[..., :-1].contiguous()
    elif how == "rows":
        mask = torch.cat([mask, mask[:, :, :1]], dim=2).contiguous()
    elif how == "heads":
        mask = mask.expand(mask.shape[0], 3, *mask.shape[2:]).contiguous() if mask.shape[1] == 1 else mask[:, :3].contiguous()
    elif how == "contiguity":
        mask = mask.transpose(2, 3).contiguous().transpose(2, 3)
    elif how == "device":
        mask = mask.to("meta")
    elif how == "alignment":                                    # a local length that is no multiple of the block (zigzag: of two blocks)
        cut = 64 if c["kind"] == "ring" else 128
        q, k, v = (t[:, :-cut].contiguous() for t in (q, k, v))
    elif how.startswith("func:"):
        ones = torch.ones(B, q.shape[1], dtype=torch.int32)
        fn = {"varlen": R.ring_flash_attn_varlen_func, "zigzag_varlen": R.zigzag_ring_flash_attn_varlen_func,
              "stripe": R.stripe_flash_attn_func, "llama3": R.llama3_flash_attn_varlen_func,
              "zigzag_llama3": R.zigzag_llama3_flash_attn_varlen_func,
              "softcap": R.with_softcap(R.ring_flash_attn_func, 30.0),
              "sinks": R.with_sinks(R.ring_flash_attn_func, torch.zeros(H)),
              "max_logit": R.with_max_logit(R.ring_flash_attn_func, torch.full((H,), float("-inf"))),
              "ulysses": R.with_ulysses(R.ring_flash_attn_func, dist.new_group(list(range(c["W"])))),
              "row_ranges": R.with_row_ranges(R.ring_flash_attn_func, 0 * ones, 5 * ones),
              "block_mask": R.with_block_mask(R.ring_flash_attn_func, mask),
              "lambda": (lambda *a, **k_: None)}[how[5:]]
    want = {"ValueError": ValueError, "NotImplementedError": NotImplementedError, "TypeError": TypeError}[c["refuse"]]
    try:
        call(R, c, fn, mask, q, k, v, **more)
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


def _needed(c, q0, k0, L):
    """does the call's own band let a row of [q0, q0 + L) see a key of [k0, k0 + L)? (global positions)"""
    wl, wr = c.get("window", (-1, -1))
    dlo = 0 if c["causal"] else (-wr if wr >= 0 else -10 ** 9)          # allowed i - j
    dhi = wl if wl >= 0 else 10 ** 9
    return q0 - (k0 + L - 1) <= dhi and q0 + L - 1 - k0 >= dlo


def expected_calls(c, rank):
    """(needed, allowed): sets of (mask storage offset of the call's first query block, k_blk0) — the block calls the band needs
    (ring: rank distance t, k_blk0 = ((rank - t) mod W) S / 128 with all rows; zigzag: one per (query chunk, key chunk) pair,
    k_blk0 = ck C / 128 with the chunk's rows) and the ones the schedule may issue at all (causal: no key chunk behind the
    query chunk)"""
    W, S = c["W"], c["S"]
    N = W * S // BLOCK
    if c["kind"] == "ring" or W == 1:
        qs, ks, L = [(0, rank * S)], [s_ * S for s_ in range(W)], S
    else:
        L = S // 2
        qs, ks = [(0, rank * L), ((L // BLOCK) * N, (2 * W - 1 - rank) * L)], [ck * L for ck in range(2 * W)]
    needed, allowed = set(), set()
    for off, q0 in qs:
        for k0 in ks:
            if not c["causal"] or k0 <= q0:
                allowed.add((off, k0 // BLOCK))
                if _needed(c, q0, k0, L):
                    needed.add((off, k0 // BLOCK))
    return needed, allowed


def expected_notes(c, rank, notes):
    """complaints about the recorded (k_blk0, mask view shape, storage offset, (B, Sq)) of ONE direction's block calls: every
    call carries the mask rows of its query rows; the (rows, k_blk0) pairs are exactly the ones the band needs (under a window:
    at least those, and none the schedule could not issue)"""
    W, S = c["W"], c["S"]
    N = W * S // BLOCK
    L = S if c["kind"] == "ring" or W == 1 else S // 2
    bad, seen = [], set()
    for n in notes:
        if n is None:
            bad.append("a block call without a mask")
            continue
        k0, shape, off, (b_, sq) = n
        if shape[3] != N or shape[2] != sq // BLOCK or sq != L:
            bad.append(f"mask view {shape} for {sq} query rows (want {L}), {N} key blocks")
        seen.add((off, k0))
    needed, allowed = expected_calls(c, rank)
    windowed = tuple(c.get("window", (-1, -1))) != (-1, -1)
    if not (needed <= seen <= allowed) or (not windowed and seen != needed):
        bad.append(f"(mask offset, k_blk0) of the block calls {sorted(seen)}: the band needs {sorted(needed)}, the schedule may issue {sorted(allowed)}")
    return bad


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config

        be_cpu = MB.BlockMaskBackend()
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
            mask = shard(c, global_mask(c), rank, 2).clone().to(dev)     # (a tensor of its own: the recorded offsets are from its first byte)
            if c.get("refuse"):
                bad = _refusal(R, c, mask, q, k, v, dev, be_cpu, _testing)
                if bad:
                    errs.append(f"{name}: {bad}")
                continue
            rec = MB.Recording(be_cpu)
            _testing.set_backend(None if use_hip else rec)
            with config.override(zigzag_exchange=c.get("form") or "ring"):
                out, lse = call(R, c, None, mask, q, k, v)
                if c.get("lse_grad"):
                    dl = shard(c, dlse_of(c), rank, 2).to(dev)
                    torch.autograd.backward([out, lse], [do, torch.where(torch.isfinite(lse), dl.to(lse.dtype), torch.zeros_like(lse))])
                else:
                    out.backward(do)
            if not use_hip:
                for direction in ("fwd", "bwd"):
                    errs += [f"{name}: {direction}: {b_}" for b_ in expected_notes(c, rank, rec.seen[direction])]
                if c.get("check_mixed") and W > 1 and c["kind"] == "zigzag" and len({n[2] for n in rec.seen["fwd"] if n}) != 2:
                    errs.append(f"{name}: the pair calls never used the second chunk's rows of the mask")
            kinds = ("out", "lse", "grad", "grad", "grad") if W == 1 else ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
            far = False
            for j, (nm, got, kd) in enumerate(zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), kinds)):
                want = shard(c, c["ref"][j], rank, 2 if nm == "lse" else 1)
                m = _tol.metrics(got, want)
                notes.append(f"{name}.{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}.{nm}", got, want, kd, c.get("tol_scale", 1.0))
                # ... and a call that ignored the mask would land on the un-masked attention
                far = far or bool(_tol.failures("", got, shard(c, c["ref0"][j], rank, 2 if nm == "lse" else 1), kd))
            if not far:
                errs.append(f"{name}: within tolerance of the attention WITHOUT the mask — the test cannot see it")
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
