"""ctypes binding of librfa_hip.so — field-for-field mirror of include/rfa.h.

The library is the ONLY compute path of this package: if it cannot be loaded, every operator
raises (there is no CPU or PyTorch fallback on purpose — see DESIGN.md "fail loudly").
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RFA_LIB_PATH: A/B tooling only (tools/ab_variants.py builds tuning variants of the same library)
LIB_PATH = os.environ.get("RFA_LIB_PATH") or os.path.join(_HERE, "librfa_hip.so")

RFA_ABI_VERSION = 8
RFA_ABI_REVISION = 1      # struct revision inside ABI 8 (include/rfa.h: rfa_abi_revision): the dropout position map
RFA_BF16, RFA_F16 = 0, 1
HALF_FULL, HALF_FRONT, HALF_BACK = 0, 1, 2
BWD_ALL, BWD_COMPUTE, BWD_REDUCE = 0, 1, 2
BWD_SKIP_DKDV, BWD_SKIP_DQ = 4, 8
BWD_KV_OVERWRITE = 16     # dk_acc / dv_acc are overwritten (dq_acc still follows acc_init)
DKDV_AUTO, DKDV_128, DKDV_256, DKDV_BAL = 0, 1, 2, 3
FWD_AUTO, FWD_8x32, FWD_4x32, FWD_P8x32 = 0, 1, 3, 4        # (2: a retired experiment, RFA_ERR_ARGS)


class Strides(C.Structure):
    _fields_ = [("batch", C.c_int64), ("row", C.c_int64), ("head", C.c_int64)]


class FwdArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p),
        ("q_st", Strides), ("k_st", Strides), ("v_st", Strides),
        ("out", C.c_void_p), ("out_st", Strides),
        ("lse", C.c_void_p), ("lse_batch", C.c_int64), ("lse_head", C.c_int64),
        ("out_acc", C.c_void_p), ("out_acc_st", Strides),
        ("lse_acc", C.c_void_p), ("lse_acc_batch", C.c_int64), ("lse_acc_head", C.c_int64),
        ("acc_init", C.c_int32),
        ("cu_seqlens_q", C.c_void_p), ("cu_seqlens_k", C.c_void_p),
        ("q_half", C.c_int32), ("k_half", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("Hk", C.c_int32), ("D", C.c_int32),
        ("Sq", C.c_int32), ("Sk", C.c_int32),
        ("softmax_scale", C.c_float),
        ("causal", C.c_int32),
        ("dtype", C.c_int32),
        ("window", C.c_int32), ("window_left", C.c_int32), ("window_right", C.c_int32),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
        ("q_pos_offset", C.c_int64), ("k_pos_offset", C.c_int64),
        ("q_pos_stride", C.c_int32), ("k_pos_stride", C.c_int32),          # dropout position map (ABI 8, revision 1)
        ("q_pos_split", C.c_int32), ("k_pos_split", C.c_int32),
        ("q_pos_offset2", C.c_int64), ("k_pos_offset2", C.c_int64),
        ("head_offset", C.c_int32),
        ("fwd_form", C.c_int32),
        ("workspace", C.c_void_p), ("kv_nsplit", C.c_int32), ("total_q", C.c_int64),
        ("mask_shift", C.c_int64),
        ("mask_shift_lens", C.c_int32),
    ]


class BwdPreArgs(C.Structure):
    _fields_ = [
        ("dout", C.c_void_p), ("out", C.c_void_p),
        ("dout_st", Strides), ("out_st", Strides),
        ("delta", C.c_void_p), ("delta_batch", C.c_int64), ("delta_head", C.c_int64),
        ("cu_seqlens_q", C.c_void_p),
        ("q_half", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("Sq", C.c_int32),
        ("dtype", C.c_int32),
    ]


class BwdArgs(C.Structure):
    _fields_ = [
        ("dout", C.c_void_p), ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p),
        ("dout_st", Strides), ("q_st", Strides), ("k_st", Strides), ("v_st", Strides),
        ("lse", C.c_void_p), ("lse_batch", C.c_int64), ("lse_head", C.c_int64),
        ("delta", C.c_void_p), ("delta_batch", C.c_int64), ("delta_head", C.c_int64),
        ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
        ("dq_st", Strides), ("dk_st", Strides), ("dv_st", Strides),
        ("dq_acc", C.c_void_p), ("dk_acc", C.c_void_p), ("dv_acc", C.c_void_p),
        ("dq_acc_st", Strides), ("dk_acc_st", Strides), ("dv_acc_st", Strides),
        ("acc_init", C.c_int32),
        ("workspace", C.c_void_p),
        ("cu_seqlens_q", C.c_void_p), ("cu_seqlens_k", C.c_void_p),
        ("q_half", C.c_int32), ("k_half", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("Hk", C.c_int32), ("D", C.c_int32),
        ("Sq", C.c_int32), ("Sk", C.c_int32),
        ("total_k", C.c_int64),
        ("softmax_scale", C.c_float),
        ("causal", C.c_int32),
        ("deterministic", C.c_int32),
        ("dtype", C.c_int32),
        ("phases", C.c_int32),
        ("ds_scratch", C.c_void_p),
        ("window", C.c_int32), ("window_left", C.c_int32), ("window_right", C.c_int32),
        ("dkdv_form", C.c_int32), ("dkdv_nsplit", C.c_int32),
        ("prof_events", C.POINTER(C.c_void_p)),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
        ("q_pos_offset", C.c_int64), ("k_pos_offset", C.c_int64),
        ("q_pos_stride", C.c_int32), ("k_pos_stride", C.c_int32),          # dropout position map (ABI 8, revision 1)
        ("q_pos_split", C.c_int32), ("k_pos_split", C.c_int32),
        ("q_pos_offset2", C.c_int64), ("k_pos_offset2", C.c_int64),
        ("head_offset", C.c_int32),
        ("ds_scratch_bytes", C.c_int64),
        ("total_q", C.c_int64),
        ("mask_shift", C.c_int64),
        ("mask_shift_lens", C.c_int32),
    ]


class ExtArgs(C.Structure):
    """rfa_ext_args: per-call features added after the ABI 8 structs were frozen (ALiBi, the soft cap); struct_bytes is
    filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("alibi_slopes", C.c_void_p), ("alibi_batch_stride", C.c_int64), ("alibi_shift", C.c_int64),
        ("softcap", C.c_float), ("softcap_pad", C.c_uint32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(ExtArgs)


class MergeArgs(C.Structure):
    _fields_ = [
        ("out_acc", C.c_void_p), ("out_acc_st", Strides),
        ("lse_acc", C.c_void_p), ("lse_acc_batch", C.c_int64), ("lse_acc_head", C.c_int64),
        ("block_out", C.c_void_p), ("block_out_st", Strides),
        ("block_lse", C.c_void_p), ("block_lse_batch", C.c_int64), ("block_lse_head", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("S", C.c_int32),
        ("acc_init", C.c_int32),
        ("dtype", C.c_int32),
        ("lse_acc_row", C.c_int64), ("block_lse_row", C.c_int64),
    ]


class SumSlotsArgs(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("slot_stride", C.c_int64), ("nslots", C.c_int32),
        ("dst", C.c_void_p),
        ("src_st", Strides), ("dst_st", Strides),
        ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32),
    ]


class SinkApplyArgs(C.Structure):
    """rfa_sink_apply_args: the attention sink applied to a merged (out, lse) pair"""
    _fields_ = [
        ("out_src", C.c_void_p), ("out_src_st", Strides),
        ("out_dst", C.c_void_p), ("out_dst_st", Strides),
        ("lse_src", C.c_void_p), ("lse_src_batch", C.c_int64), ("lse_src_head", C.c_int64),
        ("lse_dst", C.c_void_p), ("lse_dst_batch", C.c_int64), ("lse_dst_head", C.c_int64),
        ("sinks", C.c_void_p),
        ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class SinkGradArgs(C.Structure):
    """rfa_sink_grad_args: the sinks' gradient from (dout, out', lse')"""
    _fields_ = [
        ("dout", C.c_void_p), ("dout_st", Strides),
        ("out", C.c_void_p), ("out_st", Strides),
        ("lse", C.c_void_p), ("lse_batch", C.c_int64), ("lse_head", C.c_int64),
        ("sinks", C.c_void_p), ("dsink", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


SEQHEAD_PACK, SEQHEAD_UNPACK, SEQHEAD_MERGED_TO_SLOTS, SEQHEAD_SLOTS_TO_HEADS = 0, 1, 2, 3
SEQHEAD_CONTIGUOUS, SEQHEAD_ZIGZAG, SEQHEAD_STRIPE = 0, 1, 2


class SeqHeadTensor(C.Structure):
    """rfa_seq_head_tensor: one tensor of a sequence/head exchange copy — its local or merged view"""
    _fields_ = [
        ("ptr", C.c_void_p),
        ("batch", C.c_int64), ("row", C.c_int64), ("part", C.c_int64), ("head", C.c_int64),
        ("P", C.c_int32), ("H", C.c_int32),
    ]


class SeqHeadArgs(C.Structure):
    """rfa_seq_head_args: the layout change on either side of the Ulysses all-to-all; struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("op", C.c_int32), ("layout", C.c_int32),
        ("U", C.c_int32), ("B", C.c_int32), ("S", C.c_int32), ("D", C.c_int32),
        ("elem_bytes", C.c_int32), ("ntensors", C.c_int32),
        ("t", SeqHeadTensor * 3),
        ("slots", C.c_void_p), ("slots_elems", C.c_int64),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(SeqHeadArgs)


ROTARY_TABLE_F32 = 2              # RFA_ROTARY_TABLE_F32: fp32 cos / sin tables (otherwise the io dtype's code)


class RotaryTensor(C.Structure):
    """rfa_rotary_tensor: one tensor of a rotary call — read at the src strides, written at the dst strides"""
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p),
        ("src_batch", C.c_int64), ("src_row", C.c_int64), ("src_head", C.c_int64),
        ("dst_batch", C.c_int64), ("dst_row", C.c_int64), ("dst_head", C.c_int64),
        ("H", C.c_int32), ("pad", C.c_int32),
    ]


class RotaryArgs(C.Structure):
    """rfa_rotary_args: rotary position embedding of up to two tensors at global positions; struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("ntensors", C.c_int32),
        ("B", C.c_int32), ("S", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32),
        ("R", C.c_int32), ("rot_offset", C.c_int32),
        ("interleaved", C.c_int32), ("conj", C.c_int32),
        ("table_dtype", C.c_int32),
        ("t", RotaryTensor * 2),
        ("cos", C.c_void_p), ("sin", C.c_void_p),
        ("P", C.c_int64),
        ("positions", C.c_void_p), ("pos_batch", C.c_int64),
        ("pos_offset", C.c_int64),
        ("pos_stride", C.c_int32), ("pos_split", C.c_int32),
        ("pos_offset2", C.c_int64),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(RotaryArgs)


QK_NORM_WEIGHT_F32 = 2            # RFA_QK_NORM_WEIGHT_F32: fp32 norm weights (otherwise the io dtype's code)

_QK_NORM_HEAD = [
    ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
    ("ntensors", C.c_int32),
    ("B", C.c_int32), ("S", C.c_int32), ("D", C.c_int32),
    ("dtype", C.c_int32),
    ("R", C.c_int32), ("rot_offset", C.c_int32),
    ("interleaved", C.c_int32),
    ("table_dtype", C.c_int32), ("weight_dtype", C.c_int32),
    ("eps", C.c_float), ("weight_offset", C.c_float),
    ("t", RotaryTensor * 2),
    ("weight", C.c_void_p * 2),
    ("cos", C.c_void_p), ("sin", C.c_void_p),
    ("P", C.c_int64),
    ("positions", C.c_void_p), ("pos_batch", C.c_int64),
    ("pos_offset", C.c_int64),
    ("pos_stride", C.c_int32), ("pos_split", C.c_int32),
    ("pos_offset2", C.c_int64),
]


class QkNormRotaryArgs(C.Structure):
    """rfa_qk_norm_rotary_args: per-head RMSNorm + rotary of up to two tensors, forward; struct_bytes is filled in here"""
    _fields_ = list(_QK_NORM_HEAD)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(QkNormRotaryArgs)


class QkNormGrad(C.Structure):
    """rfa_qk_norm_grad: the incoming gradient of one tensor and its element strides"""
    _fields_ = [("dout", C.c_void_p), ("dout_batch", C.c_int64), ("dout_row", C.c_int64), ("dout_head", C.c_int64)]


class QkNormRotaryBwdArgs(C.Structure):
    """rfa_qk_norm_rotary_bwd_args: the forward's fields, then the gradients, dweight and the workspace"""
    _fields_ = list(_QK_NORM_HEAD) + [
        ("g", QkNormGrad * 2),
        ("dweight", C.c_void_p * 2),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(QkNormRotaryBwdArgs)


class MaxLogitArgs(C.Structure):
    """rfa_max_logit_args: the per-head max attention logit of one block call; struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("q", C.c_void_p), ("k", C.c_void_p),
        ("q_st", Strides), ("k_st", Strides),
        ("cu_seqlens_q", C.c_void_p), ("cu_seqlens_k", C.c_void_p),
        ("B", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32), ("H", C.c_int32), ("Hk", C.c_int32), ("D", C.c_int32),
        ("total_q", C.c_int64),
        ("q_half", C.c_int32), ("k_half", C.c_int32),
        ("softmax_scale", C.c_float),
        ("causal", C.c_int32),
        ("window", C.c_int32), ("window_left", C.c_int32), ("window_right", C.c_int32),
        ("mask_shift_lens", C.c_int32),
        ("mask_shift", C.c_int64),
        ("dtype", C.c_int32),
        ("accumulate", C.c_int32),
        ("max_logit", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(MaxLogitArgs)


class BwdPreLseArgs(C.Structure):
    """rfa_bwd_preprocess_lse_args: rfa_bwd_preprocess with the gradient of lse (delta' = delta - dlse)"""
    _fields_ = [
        ("dout", C.c_void_p), ("out", C.c_void_p),
        ("dout_st", Strides), ("out_st", Strides),
        ("delta", C.c_void_p), ("delta_batch", C.c_int64), ("delta_head", C.c_int64),
        ("dlse", C.c_void_p), ("dlse_batch", C.c_int64), ("dlse_head", C.c_int64),
        ("cu_seqlens_q", C.c_void_p),
        ("q_half", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("Sq", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class MergePairArgs(C.Structure):
    """rfa_merge_pair_args: the merge of two finished (out, lse) pairs"""
    _fields_ = [
        ("out_a", C.c_void_p), ("out_b", C.c_void_p),
        ("out_a_st", Strides), ("out_b_st", Strides),
        ("lse_a", C.c_void_p), ("lse_b", C.c_void_p),
        ("lse_a_batch", C.c_int64), ("lse_a_head", C.c_int64), ("lse_b_batch", C.c_int64), ("lse_b_head", C.c_int64),
        ("out", C.c_void_p), ("out_st", Strides),
        ("lse", C.c_void_p), ("lse_batch", C.c_int64), ("lse_head", C.c_int64),
        ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class MergePairBwdArgs(C.Structure):
    """rfa_merge_pair_bwd_args: its backward, from the forward's four inputs"""
    _fields_ = [
        ("dout", C.c_void_p), ("dout_st", Strides),
        ("dlse", C.c_void_p), ("dlse_batch", C.c_int64), ("dlse_head", C.c_int64),
        ("out_a", C.c_void_p), ("out_b", C.c_void_p),
        ("out_a_st", Strides), ("out_b_st", Strides),
        ("lse_a", C.c_void_p), ("lse_b", C.c_void_p),
        ("lse_a_batch", C.c_int64), ("lse_a_head", C.c_int64), ("lse_b_batch", C.c_int64), ("lse_b_head", C.c_int64),
        ("dout_a", C.c_void_p), ("dout_b", C.c_void_p),
        ("dout_a_st", Strides), ("dout_b_st", Strides),
        ("dlse_a", C.c_void_p), ("dlse_b", C.c_void_p),
        ("dlse_a_batch", C.c_int64), ("dlse_a_head", C.c_int64), ("dlse_b_batch", C.c_int64), ("dlse_b_head", C.c_int64),
        ("B", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class VdimArgs(C.Structure):
    """rfa_vdim_args: the V head dim of a call whose QK head dim (the base struct's D) differs; struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("head_dim_v", C.c_int32), ("pad", C.c_int32),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(VdimArgs)


class RowRangeArgs(C.Structure):
    """rfa_rowrange_args: per-row key ranges of a block call (start / end: int32 (B, Sq) global key positions, k_pos0: the
    global position of the block's key row 0, tile_bounds: the backward's workspace); struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("start", C.c_void_p), ("end", C.c_void_p),
        ("batch_stride", C.c_int64), ("k_pos0", C.c_int64),
        ("tile_bounds", C.c_void_p),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(RowRangeArgs)


BLOCK_MASK_SIZE = 128             # RFA_BLOCK_MASK_SIZE: query rows / keys per byte of a block mask


class BlockMaskArgs(C.Structure):
    """rfa_blockmask_args: the block-sparse mask of a block call (mask: uint8 (Bm, Hm, nq, nk_blocks), one byte per pair of
    128 query rows and 128 keys; the strides in bytes, 0 = broadcast; k_blk0: the column of the block's key row 0);
    struct_bytes is filled in here"""
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("reserved", C.c_uint32),
        ("mask", C.c_void_p),
        ("batch_stride", C.c_int64), ("head_stride", C.c_int64), ("row_stride", C.c_int64),
        ("nk_blocks", C.c_int64), ("k_blk0", C.c_int64),
        ("workspace", C.c_void_p),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.struct_bytes:
            self.struct_bytes = C.sizeof(BlockMaskArgs)


# every symbol include/rfa.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "rfa_abi_version": (C.c_int, []),
    "rfa_abi_revision": (C.c_int, []),
    "rfa_build_id": (C.c_char_p, []),
    "rfa_strerror": (C.c_char_p, [C.c_int]),
    "rfa_fwd": (C.c_int, [C.POINTER(FwdArgs), C.c_void_p]),
    "rfa_fwd_ex": (C.c_int, [C.POINTER(FwdArgs), C.POINTER(ExtArgs), C.c_void_p]),
    "rfa_ext_args_bytes": (C.c_int64, []),
    "rfa_fwd_workspace_bytes": (C.c_int64, [C.POINTER(FwdArgs), C.POINTER(C.c_int32)]),
    "rfa_bwd_preprocess": (C.c_int, [C.POINTER(BwdPreArgs), C.c_void_p]),
    "rfa_bwd_workspace_bytes": (C.c_int64, [C.POINTER(BwdArgs)]),
    "rfa_bwd_ds_scratch_bytes": (C.c_int64, [C.POINTER(BwdArgs)]),
    "rfa_bwd_ds_scratch_min_bytes": (C.c_int64, [C.POINTER(BwdArgs)]),
    "rfa_bwd_ds_chunks": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int64)]),
    "rfa_bwd_plan": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rfa_bwd": (C.c_int, [C.POINTER(BwdArgs), C.c_void_p]),
    "rfa_bwd_ex": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(ExtArgs), C.c_void_p]),
    "rfa_merge": (C.c_int, [C.POINTER(MergeArgs), C.c_void_p]),
    "rfa_sum_slots": (C.c_int, [C.POINTER(SumSlotsArgs), C.c_void_p]),
    "rfa_cast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "rfa_lse_flatten": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int64, C.c_int64, C.c_void_p]),
    "rfa_lse_unflatten": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int64, C.c_int64, C.c_void_p]),
    "rfa_sink_apply": (C.c_int, [C.POINTER(SinkApplyArgs), C.c_void_p]),
    "rfa_sink_grad": (C.c_int, [C.POINTER(SinkGradArgs), C.c_void_p]),
    "rfa_sink_grad_workspace_bytes": (C.c_int64, [C.POINTER(SinkGradArgs)]),
    "rfa_seq_head_copy": (C.c_int, [C.POINTER(SeqHeadArgs), C.c_void_p]),
    "rfa_rotary": (C.c_int, [C.POINTER(RotaryArgs), C.c_void_p]),
    "rfa_qk_norm_rotary_fwd": (C.c_int, [C.POINTER(QkNormRotaryArgs), C.c_void_p]),
    "rfa_qk_norm_rotary_bwd": (C.c_int, [C.POINTER(QkNormRotaryBwdArgs), C.c_void_p]),
    "rfa_qk_norm_rotary_bwd_workspace_bytes": (C.c_int64, [C.POINTER(QkNormRotaryBwdArgs)]),
    "rfa_max_logit": (C.c_int, [C.POINTER(MaxLogitArgs), C.c_void_p]),
    "rfa_max_logit_workspace_bytes": (C.c_int64, [C.POINTER(MaxLogitArgs)]),
    "rfa_bwd_preprocess_lse": (C.c_int, [C.POINTER(BwdPreLseArgs), C.c_void_p]),
    "rfa_merge_pair": (C.c_int, [C.POINTER(MergePairArgs), C.c_void_p]),
    "rfa_merge_pair_bwd": (C.c_int, [C.POINTER(MergePairBwdArgs), C.c_void_p]),
    "rfa_fwd_vd": (C.c_int, [C.POINTER(FwdArgs), C.POINTER(VdimArgs), C.c_void_p]),
    "rfa_bwd_vd": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(VdimArgs), C.c_void_p]),
    "rfa_fwd_rr": (C.c_int, [C.POINTER(FwdArgs), C.POINTER(RowRangeArgs), C.c_void_p]),
    "rfa_bwd_rr": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(RowRangeArgs), C.c_void_p]),
    "rfa_rowrange_workspace_bytes": (C.c_int64, [C.POINTER(BwdArgs)]),
    "rfa_fwd_bm": (C.c_int, [C.POINTER(FwdArgs), C.POINTER(BlockMaskArgs), C.c_void_p]),
    "rfa_bwd_bm": (C.c_int, [C.POINTER(BwdArgs), C.POINTER(BlockMaskArgs), C.c_void_p]),
    "rfa_blockmask_workspace_bytes": (C.c_int64, [C.POINTER(BwdArgs)]),
}

_lib = None


def load():
    """Load librfa_hip.so once; raise RuntimeError (never fall back) when it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"ring_flash_attn: HIP extension not built ({LIB_PATH} missing). "
            "Run `python ring-flash-attention_amd/build.py lib` (needs hipcc, ROCm >= 7). "
            "There is no CPU fallback."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing libamdhip64 etc.
        raise RuntimeError(f"ring_flash_attn: cannot load {LIB_PATH}: {e}") from e
    # the revision first: fields were added in the MIDDLE of the ABI 8 structs, so a library from before them reports the
    # same version number and would read every later field from the wrong place
    if not hasattr(lib, "rfa_abi_revision"):
        raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no rfa_abi_revision (binding revision {RFA_ABI_REVISION}); rebuild")
    # the extension entry points arrived without a version or revision bump (no existing struct changed): a library from
    # before them reports 8 / 1 as well
    for name in ("rfa_fwd_ex", "rfa_bwd_ex", "rfa_ext_args_bytes"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the extension entry points); rebuild")
    # ... and so did the attention-sink entry points (structs of their own)
    for name in ("rfa_sink_apply", "rfa_sink_grad", "rfa_sink_grad_workspace_bytes"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the attention-sink entry points); rebuild")
    # ... and the sequence/head exchange copy (a struct of its own)
    if not hasattr(lib, "rfa_seq_head_copy"):
        raise RuntimeError("ring_flash_attn: librfa_hip.so has no rfa_seq_head_copy (the sequence/head exchange copies); rebuild")
    # ... and the per-head max attention logit (a struct of its own)
    for name in ("rfa_max_logit", "rfa_max_logit_workspace_bytes"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the max-logit entry points); rebuild")
    # ... and the gradient of lse and the pairwise merge (structs of their own)
    for name in ("rfa_bwd_preprocess_lse", "rfa_merge_pair", "rfa_merge_pair_bwd"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the lse-gradient / merge entry points); rebuild")
    # ... and the pair with a value head dim of its own (a struct of its own)
    for name in ("rfa_fwd_vd", "rfa_bwd_vd"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the value-head-dim entry points); rebuild")
    # ... and the pair with per-row key ranges (a struct of its own)
    for name in ("rfa_fwd_rr", "rfa_bwd_rr", "rfa_rowrange_workspace_bytes"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the row-range entry points); rebuild")
    # ... and the pair with a block-sparse mask
    for name in ("rfa_fwd_bm", "rfa_bwd_bm", "rfa_blockmask_workspace_bytes"):
        if not hasattr(lib, name):
            raise RuntimeError(f"ring_flash_attn: librfa_hip.so has no {name} (the block-mask entry points); rebuild")
    # ... and the rotary embedding (a struct of its own)
    if not hasattr(lib, "rfa_rotary"):
        raise RuntimeError("ring_flash_attn: librfa_hip.so has no rfa_rotary (the rotary embedding entry point); rebuild")
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    ver = lib.rfa_abi_version()
    if ver != RFA_ABI_VERSION:
        raise RuntimeError(f"ring_flash_attn: librfa_hip.so ABI {ver} != binding {RFA_ABI_VERSION}; rebuild")
    rev = lib.rfa_abi_revision()
    if rev != RFA_ABI_REVISION:
        raise RuntimeError(f"ring_flash_attn: librfa_hip.so ABI {ver} revision {rev} != binding revision {RFA_ABI_REVISION}; rebuild")
    ext = lib.rfa_ext_args_bytes()
    if ext != C.sizeof(ExtArgs):
        raise RuntimeError(f"ring_flash_attn: librfa_hip.so rfa_ext_args is {ext} bytes, the binding's {C.sizeof(ExtArgs)}; rebuild")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().rfa_strerror(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} (rfa status {rc})")
