"""Worker of the multi-rank max-logit tests: one gloo rank runs `with_max_logit(<public function>, m)` on its shard of a seeded,
planted sequence (tests/_maxlogit_backend.py) and compares its partial with ONE single-device fp64 computation on the unsharded
tensors, restricted to its query rows, that the parent made once; the parent compares the MAX over the ranks with the global
one.  Backend: the CPU test backend with `max_logit` (partials equal the reference to the fp32 rounding of the stored value) or
the HIP kernels with every rank sharing cuda:0 (partials within the derived tolerance; the MAX over the ranks bit-identical
to one `be.max_logit` call on the unsharded tensors, which rank 0 makes).  Kinds, sharding and calls are those of
tests/_softcap_worker.py.  A case may carry wrap="softcap" / "sinks": the numbers must not change."""
import os
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ring-flash-attention_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _maxlogit_backend as ML                                # noqa: E402
import _softcap_worker as SW                                  # noqa: E402
from _blockref import visible                                 # noqa: E402

B, H, HK = SW.B, SW.H, SW.HK
DENSE = SW.DENSE
NEG_INF = float("-inf")


def case_name(c):
    w = c.get("window", (-1, -1))
    return f"{c['kind']}{'-' + c['form'] if c.get('form') else ''}-W{c['W']}-S{c['S']}-D{c.get('D', 64)}-" \
           f"{'causal' if c['causal'] else 'full'}-w{w[0]}_{w[1]}{'-' + c['wrap'] if c.get('wrap') else ''}" \
           f"{'-groups' + str(c['groups']) if c.get('groups') else ''}"


def _cu(lens):
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + L)
    return cu


def inputs(c):
    """(q, k, v, do) unsharded, bf16, seeded, with the plants"""
    D = c.get("D", 64)
    g = torch.Generator().manual_seed(29)
    lens = SW.lens_of(c)
    lead = (B, c["W"] * c["S"]) if lens is None else (sum(lens),)
    mk = lambda h: torch.randn(*lead, h, D, generator=g)
    q, k, v, do = mk(H), mk(HK), mk(HK), mk(H)
    w = tuple(c.get("window", (-1, -1)))
    if lens is None:
        ML.plant_dense(q, k, visible(lead[1], lead[1], c["causal"], w))
    else:
        ML.plant_packed(q, k, _cu(lens), lambda n, L: visible(L, L, c["causal"], w))
    return tuple(t.to(c.get("dtype", torch.bfloat16)) for t in (q, k, v, do))


def reference(c, absolute=False):
    """row_max over the unsharded tensors: (B, S, H) / (T, H) fp64"""
    q, k, _, _ = inputs(c)
    lens = SW.lens_of(c)
    return ML.row_max(q, k, q.shape[-1] ** -0.5, causal=c["causal"], window=tuple(c.get("window", (-1, -1))),
                      cu_seqlens=None if lens is None else _cu(lens), absolute=absolute)


def call(R, c, m, q, k, v, rank, dev, sinks=None):
    fn = getattr(R, SW.FUNCS[c["kind"]])
    if c.get("wrap") == "softcap":
        fn = R.with_softcap(fn, 30.0)
    elif c.get("wrap") == "sinks":
        fn = R.with_sinks(fn, sinks)
    fn = R.with_max_logit(fn, m)
    kw = dict(causal=c["causal"], window_size=tuple(c.get("window", (-1, -1))))
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


def run_rank(rank, W, port, cases, use_hip, ret):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=W)
        import ring_flash_attn as R
        from ring_flash_attn import _testing, config
        from ring_flash_attn.backend import get_backend
        from _sink_backend import SinkBackend

        class CpuBackend(ML.MaxLogitBackend, SinkBackend):
            pass

        if use_hip:
            dev = torch.device("cuda:0")
            torch.cuda.set_device(dev)
            _testing.allow_host_staging(True)                    # several gloo ranks share this one GPU
            _testing.set_backend(None)
        else:
            dev = torch.device("cpu")
            _testing.set_backend(CpuBackend(serves=("mask_shift", "mask_shift_lens", "softcap")))
        errs, notes, parts, whole = [], [], [], []
        for c in cases:
            name = f"{case_name(c)}[r{rank}]"
            dense = c["kind"] in DENSE
            rd = 1 if dense else 0
            full = inputs(c)
            q, k, v, do = (SW.shard(c, t, rank, rd).to(dev) for t in full)
            q, k, v = (t.requires_grad_(True) for t in (q, k, v))
            sinks = torch.zeros(H, device=dev, requires_grad=True) if c.get("wrap") == "sinks" else None
            m = torch.full((H,), NEG_INF, dtype=torch.float32, device=dev)
            # (groups: llama3 gathers K/V in that many head groups — one block call per group of query heads)
            with config.override(zigzag_exchange=c.get("form") or "ring", llama3_min_groups=c.get("groups", 1)):
                out = call(R, c, m, q, k, v, rank, dev, sinks)
                first = m.clone()
                out.backward(do)
                if not torch.equal(m, first):
                    errs.append(f"{name}: the backward changed max_logit: {first} -> {m}")
                call(R, c, m, q, k, v, rank, dev, sinks)
                if not torch.equal(m, first):
                    errs.append(f"{name}: a second identical forward changed max_logit: {first} -> {m}")
                above = torch.full_like(m, 1e4)
                call(R, c, above, q, k, v, rank, dev, sinks)
                if not torch.equal(above, torch.full_like(m, 1e4)):
                    errs.append(f"{name}: a tensor pre-filled above every logit came back changed: {above}")
            want = ML.head_max(SW.shard(c, c["ref"], rank, rd))
            got = first.double().cpu()
            if use_hip:
                tol = ML.tolerance(q.shape[-1], 1.0, ML.head_max(SW.shard(c, c["ref_abs"], rank, rd)))
            else:
                tol = 2.0 ** -24 * want.abs().masked_fill(torch.isinf(want), 0.0) + 1e-12       # the fp32 store
            try:
                ratio = ML.close(got, want, tol)
                notes.append(f"{name}: max_logit {[round(x, 4) for x in got.tolist()]}, worst |err| / tol {ratio:.3e}")
            except AssertionError:
                errs.append(f"{name}: max_logit {got.tolist()}, fp64 reference on this rank's rows {want.tolist()}, tol {tol.tolist()}")
            parts.append(first.cpu())
            if use_hip and rank == 0:
                # ONE block call on the unsharded tensors (what the MAX over the ranks must equal, bit for bit)
                uq, uk = full[0].to(dev), full[1].to(dev)
                one = torch.full((H,), NEG_INF, dtype=torch.float32, device=dev)
                w = tuple(c.get("window", (-1, -1)))
                lens = SW.lens_of(c)
                if lens is None:
                    get_backend().max_logit(uq, uk, one, softmax_scale=uq.shape[-1] ** -0.5, causal=c["causal"], window=w)
                else:
                    cu = torch.tensor(_cu(lens), dtype=torch.int32, device=dev)
                    get_backend().max_logit(uq, uk, one, softmax_scale=uq.shape[-1] ** -0.5, causal=c["causal"], window=w,
                                            cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(lens), max_seqlen_k=max(lens))
                whole.append(one.cpu())
        ret[("notes", rank)] = notes
        ret[("parts", rank)] = parts
        ret[("whole", rank)] = whole
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

    cases = [dict(c, ref=reference(c), ref_abs=reference(c, absolute=True) if use_hip else None) for c in cases]
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
    if errs:
        return errs, notes
    for i, c in enumerate(cases):
        total = torch.stack([ret[("parts", r)][i] for r in range(W)]).amax(0)
        want = ML.head_max(c["ref"])
        if use_hip:
            one = ret[("whole", 0)][i]
            if not torch.equal(total, one):
                errs.append(f"{case_name(c)}: MAX over {W} ranks {total.tolist()} is not the bits of one call on the unsharded "
                            f"tensors {one.tolist()}")
            tol = ML.tolerance(c.get("D", 64), 1.0, ML.head_max(c["ref_abs"]))
        else:
            tol = 2.0 ** -24 * want.abs().masked_fill(torch.isinf(want), 0.0) + 1e-12
        try:
            ML.close(total, want, tol)
        except AssertionError:
            errs.append(f"{case_name(c)}: MAX over {W} ranks {total.tolist()}, global fp64 reference {want.tolist()}")
    return errs, notes
