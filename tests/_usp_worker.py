"""Worker of the multi-rank `with_ulysses` tests: one gloo rank of a world of W = U * R runs
`with_ulysses(<dense public function>, ulysses_group)` over its ring group on its shard of a seeded sequence — the shard the
function over all W ranks expects — and checks, as the case asks:
    plain   bit for bit against a PLAIN run of the function at world size R on the merged tensors with this rank's head
            slice, which the test builds directly from the unsharded tensors (the exchange is pure data movement);
    fp64    against its shard of ONE single-device fp64 attention over the unsharded tensors (tests/_blockref.py), within
            the *_ring kinds of tests/_tol.py — computed once by the parent (CPU) or by rank 0 on the device (HIP);
    count   exactly one all-to-all on the Ulysses group in front of and one behind the wrapped call, forward and backward;
    ckpt    activation checkpointing around the wrapped call reproduces the gradients bit for bit;
    only_q  with k and v needing no gradient, dq is the full run's.
Backend: the CPU test backend with the exchange copies (tests/_usp_backend.py) or the HIP kernels with every rank sharing
cuda:0.  Sharding helpers are those of tests/_softcap_worker.py."""
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

PRE = {"ring": "ring_flash_attn", "zigzag": "zigzag_ring_flash_attn", "stripe": "stripe_flash_attn"}


def case_name(c):
    w = c.get("window", (-1, -1))
    return (f"{c['kind']}{'-' + c['zz'] if c.get('zz') else ''}-{c.get('form', 'func')}-U{c['U']}xR{c['R']}-B{c['B']}-S{c['S']}-"
            f"H{c['H']}_{c['Hk']}-D{c['D']}-{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}"
            f"{'-alibi' if c.get('alibi') else ''}{'-cap' if c.get('softcap') else ''}"
            f"{'-fp16' if c.get('dtype') == 'fp16' else ''}")


def inputs(c):
    g = torch.Generator().manual_seed(c.get("seed", 31))
    W = c["U"] * c["R"]
    dt = torch.float16 if c.get("dtype") == "fp16" else torch.bfloat16
    hk = c["H"] if c.get("form") == "qkvpacked" else c["Hk"]
    mk = lambda h: torch.randn(c["B"], W * c["S"], h, c["D"], generator=g).to(dt)
    return mk(c["H"]), mk(hk), mk(hk), mk(c["H"])


def slopes_of(c):
    return (2.0 ** -(1 + torch.arange(c["H"], dtype=torch.float32) * 8.0 / c["H"])) if c.get("alibi") else None


def reference(c, dev=None):
    """(out, lse, dq, dk, dv) fp64 of the ONE single-device attention over the unsharded tensors"""
    import _blockref as SR

    q, k, v, do = (t if dev is None else t.to(dev) for t in inputs(c))
    s = slopes_of(c)
    res = SR.attention(q, k, v, causal=c["causal"], window=tuple(c.get("window", (-1, -1))), dout=do,
                       softcap=c.get("softcap") or 0.0, slopes=None if s is None else s.to(q.device).double())
    return [t.detach().cpu() for t in res]


def place(c, rank):
    """(rho, p): ring rank and Ulysses index of a global rank (the table of ring_flash_attn/ulysses.py)"""
    U, R = c["U"], c["R"]
    return (rank % R, rank // R) if c["kind"] == "stripe" else (rank // U, rank % U)


def global_rank(c, rho, p):
    return rho + c["R"] * p if c["kind"] == "stripe" else rho * c["U"] + p


def shard(c, t, world, rank, dim=1):
    return SW.shard(dict(kind=c["kind"], W=world), t, rank, dim)


def merged_rows(c, p):
    """merged row of every local row of Ulysses index p, written from the table"""
    U, S = c["U"], c["S"]
    i = torch.arange(S)
    if c["kind"] == "stripe":
        return i * U + p
    if c["kind"] == "zigzag":
        C = S // 2
        return torch.where(i < C, p * C + i, U * C + (U - 1 - p) * C + (i - C))
    return p * S + i


def _run(fn, c, q, k, v, do, group, slopes, probs=True, checkpoint=False, after_forward=None):
    """(out, lse, dq, dk, dv) of one call in the case's form"""
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=probs, group=group,
              alibi_slopes=slopes)
    form = c.get("form", "func")
    if form == "func":
        ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
        grads = lambda: (ins[0].grad, ins[1].grad, ins[2].grad)
    elif form == "kvpacked":
        ins = [q.clone().requires_grad_(True), torch.stack([k, v], dim=2).requires_grad_(True)]
        grads = lambda: (ins[0].grad, ins[1].grad[:, :, 0], ins[1].grad[:, :, 1])
    else:
        ins = [torch.stack([q, k, v], dim=2).requires_grad_(True)]
        grads = lambda: (ins[0].grad[:, :, 0], ins[0].grad[:, :, 1], ins[0].grad[:, :, 2])
    if checkpoint:
        from torch.utils.checkpoint import checkpoint as ckpt

        res = ckpt(lambda *a: fn(*a, **kw), *ins, use_reentrant=False)
    else:
        res = fn(*ins, **kw)
    out, lse = (res[0], res[1]) if probs else (res, None)
    if after_forward is not None:
        after_forward()
    out.backward(do)
    return (out.detach(), None if lse is None else lse.detach()) + tuple(g.detach().clone() for g in grads())


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config
        from _usp_backend import UspBackend

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        _testing.set_backend(None if use_hip else UspBackend(serves=("mask_shift", "alibi", "softcap")))
        groups = {}
        errs, notes, counts = [], [], {}
        for c in cases:
            if c.get("refusals"):
                errs += refusals(R, c["U"], rank, dev, use_hip)
                continue
            name = case_name(c)
            U = c["U"]
            assert U * c["R"] == W
            form = c.get("form", "func")
            base = getattr(R, f"{PRE[c['kind']]}_{'' if form == 'func' else form + '_'}func")
            key = (c["kind"] == "stripe", U)
            if key not in groups:
                groups[key] = R.make_usp_groups(base, U)
            ug, rg = groups[key]
            func = R.with_softcap(base, c["softcap"]) if c.get("softcap") else base
            attn = R.with_ulysses(func, ug)
            rho, p = place(c, rank)
            if dist.get_rank(ug) != p or dist.get_rank(rg) != rho:
                errs.append(f"{name}[r{rank}]: group ranks ({dist.get_rank(rg)}, {dist.get_rank(ug)}) != (rho, p) = ({rho}, {p})")
                continue
            full = inputs(c)
            ql, kl, vl, dol = (shard(c, t, W, rank).to(dev) for t in full)
            sl = slopes_of(c)
            sl = None if sl is None else sl.to(dev)
            checks = c.get("checks", ("plain", "fp64"))
            with config.override(zigzag_exchange=c.get("zz") or "ring"):
                got = _run(attn, c, ql, kl, vl, dol, rg, sl)
                if "fp64" in checks:
                    ref = c.get("ref")
                    if use_hip:                                  # one fp64 reference per case, by rank 0 on the device
                        box = [reference(c, dev) if rank == 0 else None]
                        dist.broadcast_object_list(box, src=0)
                        ref = box[0]
                    kinds = ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
                    for nm, g_, r_, kd in zip(("out", "lse", "dq", "dk", "dv"), got, ref, kinds):
                        want = shard(c, r_, W, rank, 2 if nm == "lse" else 1)
                        m = _tol.metrics(g_, want)
                        notes.append(f"{name}[r{rank}].{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                        errs += _tol.failures(f"{name}[r{rank}].{nm}", g_, want, kd)
                if "plain" in checks:
                    # the plain call at world size R: the ring rank's shard of the unsharded tensors, this rank's head slice
                    def mine(t):
                        hs = t.shape[2] // U
                        return shard(c, t, c["R"], rho)[:, :, p * hs:(p + 1) * hs].contiguous().to(dev)

                    hs = c["H"] // U
                    plain = _run(func, c, *(mine(t) for t in full), rg, None if sl is None else sl[p * hs:(p + 1) * hs].contiguous())
                    box = [None] * W
                    dist.all_gather_object(box, [t.cpu() for t in plain])
                    rows = merged_rows(c, p)
                    for x, nm in enumerate(("out", "lse", "dq", "dk", "dv")):
                        # this rank's rows of every head slice j, from the rank that ran slice j of the same ring rank
                        parts = [box[global_rank(c, rho, j)][x] for j in range(U)]
                        want = torch.cat([t.index_select(2, rows) for t in parts], 1) if nm == "lse" else \
                            torch.cat([t.index_select(1, rows) for t in parts], 2)
                        if not torch.equal(got[x].cpu(), want):
                            errs.append(f"{name}[r{rank}].{nm}: differs from the plain call at world size {c['R']}")
                if "count" in checks:
                    # events of one call: "A" an all-to-all on the Ulysses group, "F" / "B" a block call of the wrapped schedule
                    from ring_flash_attn.backend import get_backend

                    events = []
                    orig = dist.all_to_all_single

                    def counting(output, input, *a, **kw):
                        if kw.get("group", a[2] if len(a) > 2 else None) is ug:
                            events.append("A")
                        return orig(output, input, *a, **kw)

                    inner = get_backend()
                    dist.all_to_all_single = counting
                    _testing.set_backend(_Events(inner, events))
                    try:
                        n0 = []
                        _run(attn, c, ql, kl, vl, dol, rg, sl, probs=False, after_forward=lambda: n0.append(len(events)))
                        n0 = n0[0]
                    finally:
                        dist.all_to_all_single = orig
                        _testing.set_backend(None if use_hip else inner)
                    squash = lambda ev: "".join(e for i, e in enumerate(ev) if i == 0 or e != ev[i - 1] or e == "A")
                    counts[name] = (squash(events[:n0]), squash(events[n0:]))
                    if counts[name] != ("AFA", "ABA"):
                        errs.append(f"{name}[r{rank}]: forward / backward events {counts[name]}, expected ('AFA', 'ABA'): one "
                                    "all-to-all on the Ulysses group in front of and one behind the wrapped call")
                if "only_q" in checks:
                    # k and v need no gradient: the backward still moves all three (a transfer's size never depends on
                    # rank-local autograd state), dq is the full run's, k and v get none
                    qq = ql.clone().requires_grad_(True)
                    attn(qq, kl, vl, causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), group=rg).backward(dol)
                    if not torch.equal(qq.grad, got[2]):
                        errs.append(f"{name}[r{rank}].dq: differs when only q needs a gradient")
                if "ckpt" in checks:
                    again = _run(attn, c, ql, kl, vl, dol, rg, sl, checkpoint=True)
                    for nm, a_, b_ in zip(("out", "lse", "dq", "dk", "dv"), got, again):
                        if not torch.equal(a_, b_):
                            errs.append(f"{name}[r{rank}].{nm}: differs under activation checkpointing")
        ret[("notes", rank)] = notes
        ret[("counts", rank)] = counts
        ret[rank] = errs
    except Exception:
        ret[rank] = [f"rank {rank} crashed:\n{traceback.format_exc()}"]
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def refusals(R, U, rank, dev, use_hip):
    """every refusal of a with_ulysses CALL on a Ulysses group of U > 1 ranks — raised before anything is exchanged"""
    from ring_flash_attn import _testing
    from ring_flash_attn.backend import get_backend
    from _ref_backend import RefBackend

    ug, rg = R.make_usp_groups(R.ring_flash_attn_func, U)
    errs, posted = [], []
    orig = dist.all_to_all_single

    def counting(*a, **kw):
        posted.append(1)
        return orig(*a, **kw)

    def expect(exc, what, fn, *a, **kw):
        try:
            fn(*a, group=rg, **kw)
            errs.append(f"[r{rank}] {what}: nothing raised, expected {exc.__name__}")
        except exc:
            pass
        except Exception as e:                               # noqa: BLE001
            errs.append(f"[r{rank}] {what}: {type(e).__name__}: {e}, expected {exc.__name__}")

    g = torch.Generator().manual_seed(3)
    mk = lambda s, h: torch.randn(2, s, h, 32, generator=g).bfloat16().to(dev)
    ring = R.with_ulysses(R.ring_flash_attn_func, ug)
    zig = R.with_ulysses(R.zigzag_ring_flash_attn_func, ug)
    kvp = R.with_ulysses(R.stripe_flash_attn_kvpacked_func, ug)
    H = 4 * U
    dist.all_to_all_single = counting
    try:
        expect(ValueError, "H not divisible by U", ring, mk(12, H + 1), mk(12, H + 1), mk(12, H + 1))
        expect(ValueError, "Hk not divisible by U", ring, mk(12, H), mk(12, 1), mk(12, 1))
        expect(ValueError, "Hk of a packed kv not divisible by U", kvp, mk(12, H), torch.stack([mk(12, 1), mk(12, 1)], 2), causal=True)
        expect(ValueError, "odd S with a zigzag function", zig, mk(11, H), mk(11, U), mk(11, U), causal=True)
        expect(ValueError, "q / k row counts differ", ring, mk(12, H), mk(10, U), mk(10, U))
        expect(ValueError, "k / v row counts differ", ring, mk(12, H), mk(12, U), mk(10, U))
        expect(NotImplementedError, "dropout", ring, mk(12, H), mk(12, U), mk(12, U), dropout_p=0.1)
        if not use_hip:
            inner = get_backend()
            _testing.set_backend(RefBackend(serves=("mask_shift",)))
            try:
                expect(NotImplementedError, "a backend without serves_seq_head_exchange", ring, mk(12, H), mk(12, U), mk(12, U))
            finally:
                _testing.set_backend(inner)
    finally:
        dist.all_to_all_single = orig
    if posted:
        errs.append(f"[r{rank}] {len(posted)} all-to-alls were posted by refused calls")
    return errs


class _Events:
    """wraps a backend: notes every fwd / bwd block call in `events`"""

    def __init__(self, inner, events):
        self.inner, self.events = inner, events

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def fwd(self, *a, **kw):
        self.events.append("F")
        return self.inner.fwd(*a, **kw)

    def bwd(self, *a, **kw):
        self.events.append("B")
        return self.inner.bwd(*a, **kw)


def run_world(W, cases, use_hip, port, limit_s=240):
    """one world under its own time limit; returns (complaints, measured figures, {rank: counts}).  On the CPU every case
    gets its ONE fp64 reference here, before the ranks start."""
    import time

    import torch.multiprocessing as mp

    full = [dict(c, ref=reference(c)) if not use_hip and "fp64" in c.get("checks", ("plain", "fp64")) else c for c in cases]
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(run_rank, args=(W, port, full, use_hip, ret), nprocs=W, join=False)
    deadline = time.time() + limit_s
    while not ctx.join(timeout=1):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            return [f"world of {W} ranks did not finish within {limit_s} s"], [], {}
    errs, notes, counts = [], [], {}
    for r in range(W):
        errs += list(ret.get(r, [f"rank {r} returned nothing"]))
        notes += list(ret.get(("notes", r), []))
        counts[r] = dict(ret.get(("counts", r), {}))
    return errs, notes, counts
