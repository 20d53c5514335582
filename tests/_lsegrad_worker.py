"""Worker of the multi-rank lse-gradient tests: one gloo rank runs `with_lse_grad(<public function>)` on its shard of a seeded
sequence with the loss <out, dO> + <lse, dL> and compares out, lse, dq, dk, dv with its shard of ONE single-device fp64
computation over the unsharded tensors that the parent made once (autograd through tests/_blockref.block_forward — it does not
use the delta' = delta - dlse identity the product is built on) — and asserts that dq and dk DIFFER from the dL = 0 gradients by
more than the tolerance, so that a backward that drops dL cannot pass.  Flags of a case: `unused` (the loss does not touch lse:
the bound call must equal the plain call bit for bit), `lse_only` (the loss touches lse alone: dout arrives undefined),
`softcap` (with_lse_grad of a with_softcap result), `compose` (replicated prefix keys on a one-rank group + the zigzag-sharded
sequence, merged with merge_attn, against one fp64 softmax over [prefix; sequence]).  Backend: the CPU test backend with the
lse gradient (tests/_lsegrad_backend.py) or the HIP kernels with every rank sharing cuda:0.  Kinds, inputs and sharding are
those of tests/_softcap_worker.py."""
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

B, H, HK, DENSE, FUNCS = SW.B, SW.H, SW.HK, SW.DENSE, SW.FUNCS
M_PREFIX = 5


def case_name(c):
    w = c.get("window", (-1, -1))
    flags = "".join(f"-{f}" for f in ("unused", "lse_only", "compose") if c.get(f)) + (f"-cap{c['softcap']}" if c.get("softcap") else "")
    return f"{c['kind']}-W{c['W']}-S{c['S']}-D{c.get('D', 64)}-{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}-dlse{flags}"


def _cu(lens):
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    return cu


def draw_dl(c):
    """dL ~ N(0, 1), fp64, in the layout of the unsharded lse: (B, H, W S) dense, (H, T) packed"""
    g = torch.Generator().manual_seed(97)
    lens = SW.lens_of(c)
    shape = (B, H, c["W"] * c["S"]) if lens is None else (H, sum(lens))
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def reference(c, dL):
    """(out, lse, dq, dk, dv) fp64 of ONE single-device attention over the unsharded tensors, the gradients by autograd of
    <out, dO> + <lse, dL> (dL None: of <out, dO> alone; `lse_only`: of <lse, dL> alone)"""
    import _blockref as R
    from oracle import flash_attn_ref as O

    q, k, v, do = SW.inputs(c)
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    kw = dict(causal=c["causal"], window=tuple(c.get("window", (-1, -1))), softcap=c.get("softcap", 0.0))
    scale = q.shape[-1] ** -0.5
    lens = SW.lens_of(c)
    if lens is None:
        drop = c.get("dropout")                              # (p, seed) of a dense single-device call: the kernels' keep mask
        kws = [kw if drop is None else dict(kw, keep=R.keep_mask((drop[0], drop[1], 0, 0, 0), b, H, q.shape[1], k.shape[1]),
                                            rescale=O.drop_rescale(drop[0])) for b in range(q.shape[0])]
        pairs = [R.block_forward(q[b], k[b], v[b], scale, **kws[b]) for b in range(q.shape[0])]
        out, lse = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    else:
        cu = _cu(lens)
        pairs = [R.block_forward(q[a:b], k[a:b], v[a:b], scale, **kw) for a, b in zip(cu, cu[1:])]
        out, lse = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs], dim=1)
    assert torch.isfinite(lse).all()                         # (every row of these cases sees a key: autograd stays finite)
    loss = 0.0 if c.get("lse_only") else (out * do.double()).sum()
    if dL is not None:
        loss = loss + (lse * dL).sum()
    loss.backward()
    return (out.detach(), lse.detach(), q.grad, k.grad,
            v.grad if v.grad is not None else torch.zeros_like(v))   # (v does not enter lse)


def bind(R, c, bound=True):
    fn = getattr(R, FUNCS[c["kind"]])
    if c.get("softcap"):
        fn = R.with_softcap(fn, c["softcap"])
    return R.with_lse_grad(fn) if bound else fn


def call(R, c, fn, q, k, v, rank, dev):
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))), return_attn_probs=True)
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
    return fn(q, k, v, cq.to(dev), ck.to(dev), mq, mk, heads_k_stride=c.get("stride", 1), local_k_slice=sl, **kw)


# ---- the composition: replicated prefix keys + the zigzag-sharded sequence --------------------------------------------------
def compose_inputs(c):
    """q (B, W S, H, D), k / v (B, W S, Hk, D), the prefix kp / vp (B, M, Hk, D), dO like q — bf16 — and dL (B, H, W S) fp64"""
    D, T = c.get("D", 64), c["W"] * c["S"]
    g = torch.Generator().manual_seed(61)
    mk = lambda rows, h: torch.randn(B, rows, h, D, generator=g).bfloat16()
    return mk(T, H), mk(T, HK), mk(T, HK), mk(M_PREFIX, HK), mk(M_PREFIX, HK), mk(T, H), torch.randn(B, H, T, generator=g, dtype=torch.float64)


def compose_reference(c):
    """(out, lse, dq, dk, dv, dkp, dvp) fp64: ONE softmax over [prefix; sequence] — every prefix key visible, the sequence
    causal — and autograd of <out, dO> + <lse, dL>"""
    q, k, v, kp, vp, do, dL = compose_inputs(c)
    q, k, v, kp, vp = (t.double().requires_grad_(True) for t in (q, k, v, kp, vp))
    T, G = q.shape[1], H // HK
    ke = torch.cat([kp, k], dim=1).repeat_interleave(G, dim=2)
    ve = torch.cat([vp, v], dim=1).repeat_interleave(G, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, ke) * q.shape[-1] ** -0.5
    vis = torch.cat([torch.ones(T, M_PREFIX, dtype=torch.bool), torch.ones(T, T, dtype=torch.bool).tril()], dim=1)
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.exp(s - lse.unsqueeze(-1)), ve)
    ((out * do.double()).sum() + (lse * dL).sum()).backward()
    return out.detach(), lse.detach(), q.grad, k.grad, v.grad, kp.grad, vp.grad


def compose_rank(R, c, rank, dev, self_group):
    """this rank's complaints and figures, and its partial (dkp, dvp) — the sum over its own query rows"""
    name = case_name(c)
    full = compose_inputs(c)
    q, k, v, do = (SW.shard(c, t, rank, 1).to(dev) for t in (full[0], full[1], full[2], full[5]))
    dl = SW.shard(c, full[6], rank, 2).float().to(dev)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    kp, vp = (t.to(dev).requires_grad_(True) for t in full[3:5])
    out_p, lse_p, _ = R.with_lse_grad(R.ring_flash_attn_func)(q, kp, vp, causal=False, return_attn_probs=True, group=self_group)
    out_s, lse_s, _ = R.with_lse_grad(R.zigzag_ring_flash_attn_func)(q, k, v, causal=True, return_attn_probs=True)
    out, lse = R.merge_attn(out_p, lse_p, out_s, lse_s)
    torch.autograd.backward([out, lse], [do, dl])
    errs, notes = [], []
    kinds = ("out_ring", "lse_ring", "grad_ring", "grad_ring", "grad_ring")
    for nm, got, ref, kd in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, q.grad, k.grad, v.grad), c["ref"], kinds):
        want = SW.shard(c, ref, rank, 2 if nm == "lse" else 1)
        m = _tol.metrics(got, want)
        notes.append(f"{name}[r{rank}].{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
        errs += _tol.failures(f"{name}[r{rank}].{nm}", got, want, kd)
    return errs, notes, (kp.grad.detach().double().cpu(), vp.grad.detach().double().cpu())


# ---- merge_attn alone: inputs, the fp64 reference, the comparisons --------------------------------------------------------
def merge_inputs(Bm, Sm, Hm, Dm, dtype, packed, seed=0):
    """(out_a, lse_a, out_b, lse_b, dout, dlse) on the CPU: outs ~ N(0, 1) in the io dtype, lse ~ N(3, 2) fp32, dlse ~ N(0, 1).
    Rows 0 .. 4 of head 0 (of every batch entry) are the empty-row cases — a = +inf; b = -inf; a = -inf; both (+inf, -inf); both
    (+inf, +inf) — and an empty side's out holds NaN there, which must never be multiplied.  Dense: out (B, S, H, D), lse
    (B, H, S); packed: out (B S, H, D), lse (H, B S)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Dm + Sm + Hm)
    lead = (Bm * Sm,) if packed else (Bm, Sm)
    outs = [torch.randn(*lead, Hm, Dm, generator=g).to(dtype) for _ in range(3)]
    lses = [(3 + 2 * torch.randn(*lead, Hm, generator=g)).float() for _ in range(2)] + [torch.randn(*lead, Hm, generator=g)]
    inf = float("inf")
    for r, (ia, ib) in enumerate(((inf, None), (None, -inf), (-inf, None), (inf, -inf), (inf, inf))):
        for l, o, val in ((lses[0], outs[0], ia), (lses[1], outs[1], ib)):
            if val is not None:
                l.view(Bm, Sm, Hm)[:, r, 0] = val
                o.view(Bm, Sm, Hm, Dm)[:, r, 0] = float("nan")
    t = lambda l: l.transpose(-1, -2).contiguous()
    return outs[0], t(lses[0]), outs[1], t(lses[1]), outs[2], t(lses[2])


def _rh(x):
    return x.transpose(-1, -2).unsqueeze(-1)


def merge_reference(out_a, lse_a, out_b, lse_b, dout, dlse):
    """(out, lse, dout_a, dlse_a, dout_b, dlse_b) fp64: torch.autograd through the torch expression lse = logaddexp(lse_a,
    lse_b), out = exp(lse_a - lse) out_a + exp(lse_b - lse) out_b.  An empty side (infinite lse, either sign) is taken out
    BEFORE the expression — its lse reads -1e300 (exp underflows to an exact 0; no inf - inf), its out 0 — and its gradients
    are 0 by definition; a both-empty row is out = 0, lse = -inf and passes no gradient."""
    ea, eb = torch.isinf(lse_a), torch.isinf(lse_b)
    zero = torch.zeros((), dtype=torch.float64)
    oa, ob = (torch.where(_rh(e), zero, o.double()).requires_grad_(True) for o, e in ((out_a, ea), (out_b, eb)))
    la, lb = (torch.where(e, torch.full((), -1e300, dtype=torch.float64), l.double()).requires_grad_(True)
              for l, e in ((lse_a, ea), (lse_b, eb)))
    lse = torch.logaddexp(la, lb)
    out = _rh(torch.exp(la - lse)) * oa + _rh(torch.exp(lb - lse)) * ob
    both = ea & eb
    torch.autograd.backward([out, lse], [torch.where(_rh(both), zero, dout.double()), torch.where(both, zero, dlse.double())])
    z = lambda g, e: torch.where(e, torch.zeros_like(g), g)
    return (torch.where(_rh(both), zero, out).detach(), torch.where(both, torch.full_like(lse, float("-inf")), lse).detach(),
            z(oa.grad, _rh(ea)), z(la.grad, ea), z(ob.grad, _rh(eb)), z(lb.grad, eb))


def merge_run(merge_attn, ins):
    """[out, lse, dout_a, dlse_a, dout_b, dlse_b] of merge_attn on ins = (out_a, lse_a, out_b, lse_b, dout, dlse)"""
    leaves = [t.clone().requires_grad_(True) for t in ins[:4]]
    out, lse = merge_attn(*leaves)
    torch.autograd.backward([out, lse], [ins[4], ins[5]])
    return [out.detach(), lse.detach()] + [t.grad for t in leaves]


def lse_relative_failures(name, got, ref):
    """the RELATIVE bounds of the `lse` kind of tests/_tol.py (max, Frobenius, mean) with its absolute terms dropped: what a
    gradient of lse is held to — a value of the size of dout . out rather than of the size of lse"""
    _, rtol, fro, _, mrel = _tol.KINDS["lse"]
    m = _tol.metrics(got, ref)
    bad = [] if m["same_pattern"] else [f"{name}: non-finite pattern differs"]
    if not m["max_err"] <= rtol * m["max_ref"]:
        bad.append(f"{name}: max|err| {m['max_err']:.3e} > {rtol:.1e} max|ref| = {rtol * m['max_ref']:.3e}")
    if not m["err_norm"] <= fro * m["ref_norm"]:
        bad.append(f"{name}: relative Frobenius error {m['fro']:.3e} > {fro:.1e}")
    if not m["mean_err"] <= mrel * m["mean_ref"]:
        bad.append(f"{name}: mean|err| {m['mean_err']:.3e} > {mrel:.1e} mean|ref| = {mrel * m['mean_ref']:.3e}")
    return bad


def merge_failures(tag, got, ref):
    """(complaints, the worst figure of each comparison): out by the `out` kind, lse by `lse`, dout_a / dout_b by `grad`,
    dlse_a / dlse_b by the lse kind's relative bounds; no NaN anywhere"""
    errs, worst = [], {}
    for i, (nm, kd) in enumerate((("out", "out"), ("lse", "lse"), ("dout_a", "grad"), ("dlse_a", None), ("dout_b", "grad"),
                                  ("dlse_b", None))):
        if torch.isnan(got[i]).any():
            errs.append(f"{tag}.{nm}: NaN")
        errs += lse_relative_failures(f"{tag}.{nm}", got[i], ref[i]) if kd is None else _tol.failures(f"{tag}.{nm}", got[i], ref[i], kd)
        m = _tol.metrics(got[i], ref[i])
        worst[nm] = m["max_err"] if nm == "lse" else m["max_err"] / max(m["max_ref"], 1e-30)
    return errs, worst


def empty_row_failures(tag, got, ins, packed, Bm, Sm):
    """the exact statements about rows 0 .. 4 of head 0 (merge_inputs): one side empty — the other side's out and lse pass
    through unchanged, the empty side's gradients are exactly 0; both empty — out = 0, lse = -inf, every gradient 0"""
    def dense(t, lse_like):
        if not packed:
            return t
        return t.view(t.shape[0], Bm, Sm).transpose(0, 1) if lse_like else t.view(Bm, Sm, *t.shape[1:])

    out, lse, da, dla, db, dlb = (dense(t, i % 2 == 1) for i, t in enumerate(got))
    oa, la, ob, lb = (dense(t, i % 2 == 1) for i, t in enumerate(ins[:4]))
    errs = []

    def zero(t, what):
        if not torch.equal(t, torch.zeros_like(t)):
            errs.append(f"{tag}: {what} is not exactly zero")

    for r, (d_e, l_e, o_live, l_live) in ((0, (da, dla, ob, lb)), (2, (da, dla, ob, lb)), (1, (db, dlb, oa, la))):
        if not torch.equal(out[:, r, 0], o_live[:, r, 0]) or not torch.equal(lse[:, 0, r], l_live[:, 0, r]):
            errs.append(f"{tag}: row {r}: the live side does not pass through")
        zero(d_e[:, r, 0], f"row {r}: dout of the empty side")
        zero(l_e[:, 0, r], f"row {r}: dlse of the empty side")
    for r in (3, 4):
        zero(out[:, r, 0], f"row {r} (both empty): out")
        if not torch.equal(lse[:, 0, r], torch.full_like(lse[:, 0, r], float("-inf"))):
            errs.append(f"{tag}: row {r} (both empty): lse is not -inf")
        for t, nm in ((da, "dout_a"), (db, "dout_b")):
            zero(t[:, r, 0], f"row {r} (both empty): {nm}")
        for t, nm in ((dla, "dlse_a"), (dlb, "dlse_b")):
            zero(t[:, 0, r], f"row {r} (both empty): {nm}")
    return errs


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing
        from _lsegrad_backend import LseGradBackend

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
        else:
            dev = torch.device("cpu")
        _testing.set_backend(None if use_hip else LseGradBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
        self_group = None
        if any(c.get("compose") for c in cases):
            for r in range(W):                                   # (every rank makes every group)
                g = dist.new_group([r])
                self_group = g if r == rank else self_group
        errs, notes, prefix = [], [], {}
        for i, c in enumerate(cases):
            name = case_name(c)
            if c.get("compose"):
                e, n, prefix[i] = compose_rank(R, c, rank, dev, self_group)
                errs += e
                notes += n
                continue
            dense = c["kind"] in DENSE
            rd, ld = (1, 2) if dense else (0, 1)
            q, k, v, do = (SW.shard(c, t, rank, rd).to(dev) for t in SW.inputs(c))
            dl = SW.shard(c, c["dL"], rank, ld).float().to(dev)

            def run(bound, with_dl):
                ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
                out, lse, _ = call(R, c, bind(R, c, bound), *ins, rank, dev)
                if c.get("lse_only"):
                    lse.backward(dl)
                elif with_dl:
                    torch.autograd.backward([out, lse], [do, dl])
                else:
                    out.backward(do)
                return [out.detach(), lse.detach()] + [t.grad for t in ins]

            if c.get("unused"):
                a, b = run(True, False), run(False, False)
                for nm, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, b):
                    if not torch.equal(x, y):
                        errs.append(f"{name}[r{rank}].{nm}: the bound call with an unused lse differs from the plain call")
                continue
            got = run(True, True)
            kd = "grad" if W == 1 else "grad_ring"
            kinds = ("out" if W == 1 else "out_ring", "lse" if W == 1 else "lse_ring", kd, kd, kd)
            for j, (nm, kind) in enumerate(zip(("out", "lse", "dq", "dk", "dv"), kinds)):
                want = SW.shard(c, c["ref"][j], rank, ld if nm == "lse" else rd)
                m = _tol.metrics(got[j], want)
                notes.append(f"{name}[r{rank}].{nm}: max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}, fro {m['fro']:.3e}")
                errs += _tol.failures(f"{name}[r{rank}].{nm}", got[j], want, kind)
                # ... and a backward that ignored dL would land on the dL = 0 gradients: dq and dk must be off those by more
                # than the same tolerance (dv does not depend on lse)
                if nm in ("dq", "dk"):
                    if not _tol.failures(f"{name}[r{rank}].{nm} vs dL = 0", got[j], SW.shard(c, c["ref0"][j], rank, rd), kind):
                        errs.append(f"{name}[r{rank}].{nm}: within tolerance of the dL = 0 gradient — the test cannot see dL")
        ret[("notes", rank)] = notes
        ret[("prefix", rank)] = prefix
        ret[rank] = errs
    except Exception:
        ret[rank] = [f"rank {rank} crashed:\n{traceback.format_exc()}"]
    finally:
        try:
            dist.destroy_process_group()
        except Exception:
            pass


def run_world(W, cases, use_hip, port, limit_s=240):
    """one world under its own time limit; returns (complaints, measured figures).  Every case gets its dL and the ONE fp64
    reference (and the dL = 0 reference) here, before the ranks start; the ranks' prefix-gradient partials are summed here."""
    import time

    import torch.multiprocessing as mp

    full = []
    for c in cases:
        if c.get("compose"):
            full.append(dict(c, ref=compose_reference(c)))
        elif c.get("unused"):
            full.append(dict(c, dL=draw_dl(c)))
        else:
            dL = draw_dl(c)
            ref = reference(c, dL)
            # (the dL = 0 gradients: those of <out, dO> alone — zero for a loss that touches lse alone)
            ref0 = tuple(torch.zeros_like(t) for t in ref) if c.get("lse_only") else reference(c, None)
            full.append(dict(c, dL=dL, ref=ref, ref0=ref0))
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
            if not c.get("compose"):
                continue
            for j, nm in ((0, "dk_prefix"), (1, "dv_prefix")):
                total = torch.stack([ret[("prefix", r)][i][j] for r in range(W)]).sum(0)
                m = _tol.metrics(total, c["ref"][5 + j])
                notes.append(f"{case_name(c)}.{nm} (sum of {W} ranks): max|err| {m['max_err']:.3e} / max|ref| {m['max_ref']:.3e}")
                errs += _tol.failures(f"{case_name(c)}.{nm}", total, c["ref"][5 + j], "grad_ring")
    return errs, notes
