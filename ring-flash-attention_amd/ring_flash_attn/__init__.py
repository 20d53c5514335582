"""MI355X-native ring flash-attention.

Drop-in for the public API of zhuzilin/ring-flash-attention
(/root/reference/ring_flash_attn/__init__.py:1-35): same 21 names, same signatures, same
sharding contracts — the arithmetic runs in hand-written gfx950 HIP kernels reached through
the C ABI of librfa_hip.so (include/rfa.h); communication is RCCL via torch.distributed.
"""
from .llama3_flash_attn_varlen import (
    llama3_flash_attn_prepare_cu_seqlens,
    llama3_flash_attn_varlen_func,
    llama3_flash_attn_varlen_kvpacked_func,
    llama3_flash_attn_varlen_qkvpacked_func,
)
from .ring_flash_attn import (
    ring_flash_attn_func,
    ring_flash_attn_kvpacked_func,
    ring_flash_attn_qkvpacked_func,
)
from .ring_flash_attn_varlen import (
    ring_flash_attn_varlen_func,
    ring_flash_attn_varlen_kvpacked_func,
    ring_flash_attn_varlen_qkvpacked_func,
)
from .zigzag_ring_flash_attn import (
    zigzag_ring_flash_attn_func,
    zigzag_ring_flash_attn_kvpacked_func,
    zigzag_ring_flash_attn_qkvpacked_func,
)
from .zigzag_ring_flash_attn_varlen import (
    zigzag_ring_flash_attn_varlen_func,
    zigzag_ring_flash_attn_varlen_kvpacked_func,
    zigzag_ring_flash_attn_varlen_qkvpacked_func,
)
from .stripe_flash_attn import (
    stripe_flash_attn_func,
    stripe_flash_attn_kvpacked_func,
    stripe_flash_attn_qkvpacked_func,
)
# beyond the reference (its README.md:131 lists this entry as a TODO): llama3-style context parallelism over a
# zigzag-balanced split of the packed token stream
from .zigzag_llama3_flash_attn_varlen import (
    zigzag_llama3_flash_attn_prepare_cu_seqlens,
    zigzag_llama3_flash_attn_varlen_func,
    zigzag_llama3_flash_attn_varlen_kvpacked_func,
    zigzag_llama3_flash_attn_varlen_qkvpacked_func,
)
from .adapters import (
    substitute_hf_flash_attn,
    update_ring_flash_attn_params,
)

__version__ = "0.1.0"

# this library's own knobs (not part of the reference surface): the configuration object (config.py: every RFA_* switch,
# resolved once) and the source of the per-forward dropout seeds
from . import config
from ._common import set_dropout_generator
# flash_attn's softcap (logit soft-capping) for any of the attention functions above: with_softcap(func, softcap) — the
# positional signatures above are the reference's and stay as they are
from ._api import with_softcap
# attention sinks (GPT-OSS, streaming-LLM; Hugging Face's `s_aux`): with_sinks(func, sinks) — one learnable logit per query
# head as an extra softmax column with a zero value vector, with its gradient, on any group
from ._api import with_sinks
# QK-Clip / MuonClip (Transformer Engine's and Megatron's `max_logit`): with_max_logit(func, max_logit) max-accumulates the
# largest pre-softmax logit softmax_scale * q.k of every query head, over the pairs the attention looks at, into an fp32 (H,)
# tensor — this rank's partial; the caller's all_reduce(MAX) over the group completes it
from ._api import with_max_logit
# a differentiable lse: with_lse_grad(func) returns func with an lse whose gradient reaches dq / dk — what makes (out, lse) the
# handle by which attention over two key sets composes, backward included; merge_attn(out_a, lse_a, out_b, lse_b) is that
# composition as one fused, differentiable kernel each way (replicated prefix / global tokens next to a sharded sequence)
from ._api import merge_attn, with_lse_grad
# per-row key ranges (interval masks: documents on dense input, prefix-LM, shared prefixes): with_row_ranges(func, start, end)
# lets query row i see the keys start[i] <= j < end[i] (global positions) in the dense ring and zigzag functions
from ._api import with_row_ranges
# block-sparse masks (window + global + random blocks, block-selected attention, document masks with shared tokens):
# with_block_mask(func, block_mask) lets local query block i see key block j of the unsharded sequence iff block_mask[.., i, j],
# in blocks of BLOCK_MASK_SIZE = 128 positions, in the dense ring and zigzag functions
from ._api import BLOCK_MASK_SIZE, with_block_mask
# DeepSpeed-Ulysses head parallelism in front of the dense schedules ("USP"): with_ulysses(func, ulysses_group) exchanges heads
# for rows around `func`; make_usp_groups(func, ulysses_size) makes the (Ulysses, ring) groups of func's family
from .ulysses import make_usp_groups, with_ulysses
# rotary position embedding at GLOBAL positions for sharded q / k: apply_rotary(q, k, cos, sin, layout=func, group=group)
# rotates this rank's shards in one streaming kernel; local_positions(func, n_local, group=group) is the global position of
# every local row for the sharding `func` expects (dense and packed families)
from .rotary import apply_rotary, local_positions
# per-head QK RMSNorm (Qwen3, Gemma-3, OLMo) fused with that rotation: apply_qk_norm_rotary(q, k, w_q, w_k, cos, sin,
# layout=func, group=group) is one launch per direction, one rounding, and a reproducible weight gradient
from .qk_norm import apply_qk_norm_rotary
