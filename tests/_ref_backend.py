"""TEST INFRASTRUCTURE: the ONE CPU test backend — the oracle backend (oracle/oracle_backend.py) extended with the block
keywords that arrived after it: `mask_shift`, `mask_shift_lens`, `alibi=(slopes, shift)`, `softcap=` and the 7-tuple
`dropout=` that carries position maps (ring_flash_attn._common.dropout_arg).

`RefBackend(serves=(...))` declares exactly the `serves_*` attributes it is given; tests pick the subset a schedule is to
find.  A call that uses none of the extensions is the oracle's, untouched (fp32, the golden-fixture path).  A call that
uses a served one gets each sequence's block from tests/_blockref.py (fp64) and the oracle's delivery, so with the oracle's
rounding points: out / dq / dk / dv are rounded to the io dtype before they are merged / added in fp32, rows that see no
key leave the accumulators untouched.  A call that uses one that is not served raises TypeError, as an unknown keyword
does.  `Recording` wraps any backend and notes the `softcap` every block call carried."""
import _blockref as R
from oracle import flash_attn_ref as O
from oracle.oracle_backend import OracleBackend

FEATURES = ("mask_shift", "mask_shift_lens", "alibi", "softcap", "dropout_positions")


def _mapped(dropout):
    return dropout is not None and dropout[0] > 0 and len(dropout) > 5


def _used(kw):
    """the extensions a block call uses, by the name of their `serves_*` attribute"""
    use = [f for f in ("mask_shift", "mask_shift_lens", "softcap") if kw.get(f)]
    if kw.get("alibi") is not None:
        use.append("alibi")
    if _mapped(kw.get("dropout")):
        use.append("dropout_positions")
    return use


def check_combination(kw):
    """what the library answers with RFA_ERR_ARGS (include/rfa.h): a schedule must never issue it"""
    packed = kw.get("cu_seqlens_q") is not None
    halves = bool(kw.get("q_half") or kw.get("k_half"))
    wl, wr = kw.get("window") or (-1, -1)
    shifted = bool(kw.get("mask_shift") or kw.get("mask_shift_lens"))
    alibi, cap, dropout = kw.get("alibi"), bool(kw.get("softcap")), kw.get("dropout")
    # rfa_fwd_args.dropout_p, mask_shift, mask_shift_lens, rfa_ext_args: dropout with a window, a shift, a bias or a cap
    if dropout is not None and dropout[0] > 0:
        assert wl < 0 and wr < 0 and not shifted and alibi is None and not cap, "dropout with a window, a shift, a bias or a cap"
    # rfa_fwd_args.q_pos_stride: "a non-default map with cu_seqlens input or with q_half / k_half"
    if _mapped(dropout):
        assert not packed and not halves, "a dropout position map with packed input or halves"
    # rfa_fwd_args.mask_shift: "dense input only"; the halves belong to the zigzag schedules, which shift by mask_shift_lens
    if kw.get("mask_shift"):
        assert not packed and not halves, "an absolute mask_shift with packed input or halves"
    # rfa_ext_args, ALiBi: "a bounded window", "a non-zero alibi_shift with cu_seqlens"; no schedule biases halves or a
    # per-sequence shift
    if alibi is not None:
        assert wl < 0 and wr < 0 and not halves and not kw.get("mask_shift_lens"), "a bias with a window, halves or mask_shift_lens"
        assert not packed or alibi[1] == 0, "a non-zero alibi_shift with packed input"
    # rfa_ext_args, soft-capping: "softcap > 0 together with ... a non-NULL alibi_slopes"
    assert not cap or alibi is None, "a cap with a bias"


class RefBackend(OracleBackend):
    def __init__(self, serves=()):
        assert set(serves) <= set(FEATURES), serves
        self.name = "+".join(("oracle", *serves))
        for f in serves:
            setattr(self, "serves_" + f, True)

    def _check(self, kw):
        use = _used(kw)
        for f in use:
            if not getattr(self, "serves_" + f, False):
                raise TypeError(f"{self.name}: this backend does not serve {f}")
        if use:
            check_combination(kw)

    def fwd(self, q, k, v, **kw):
        self._check(kw)
        return super().fwd(q, k, v, **kw)

    def bwd(self, dout, q, k, v, lse, delta, **kw):
        self._check(kw)
        return super().bwd(dout, q, k, v, lse, delta, **kw)

    def _block_kw(self, seq, q, k, causal, window, dropout, mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0):
        """block_forward's keywords for one sequence of a call that uses an extension, None for one that uses none"""
        if not _used(dict(mask_shift=mask_shift, mask_shift_lens=mask_shift_lens, alibi=alibi, softcap=softcap, dropout=dropout)):
            return None
        n, b = seq[:2]
        slopes, alibi_shift = alibi or (None, 0)
        kw = dict(causal=causal, window=window, shift=mask_shift + mask_shift_lens * k.shape[0], softcap=softcap,
                  slopes=slopes if slopes is None or slopes.dim() == 1 else slopes[n], alibi_shift=alibi_shift)
        if dropout is not None and dropout[0] > 0:
            kw.update(keep=R.keep_mask(dropout, b, q.shape[1], q.shape[0], k.shape[0]), rescale=O.drop_rescale(dropout[0]))
        return kw

    def _fwd_block(self, seq, q, k, v, scale, causal, window, dropout, **ext):
        kw = self._block_kw(seq, q, k, causal, window, dropout, **ext)
        if kw is None:
            return super()._fwd_block(seq, q, k, v, scale, causal, window, dropout)
        o, l = R.block_forward(q, k, v, scale, **kw)
        return o, l.float()

    def _bwd_block(self, seq, dout, q, k, v, lse, delta, scale, causal, window, dropout, **ext):
        kw = self._block_kw(seq, q, k, causal, window, dropout, **ext)
        if kw is None:
            return super()._bwd_block(seq, dout, q, k, v, lse, delta, scale, causal, window, dropout)
        return R.block_backward(dout, q, k, v, lse, delta, scale, **kw)


class Recording:
    """any backend, with a note of the `softcap` each fwd / bwd block call carried (None: the keyword was absent); the
    wrapped backend runs the call WITHOUT the cap, so one that predates the keyword serves as well"""
    serves_softcap = True

    def __init__(self, inner):
        self.inner = inner
        self.seen = {"fwd": [], "bwd": []}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def fwd(self, *a, **kw):
        self.seen["fwd"].append(kw.pop("softcap", None))
        return self.inner.fwd(*a, **kw)

    def bwd(self, *a, **kw):
        self.seen["bwd"].append(kw.pop("softcap", None))
        return self.inner.bwd(*a, **kw)
