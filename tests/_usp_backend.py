"""TEST INFRASTRUCTURE: the CPU test backend (tests/_ref_backend.py) with the sequence/head exchange copies —
`serves_seq_head_exchange` and `seq_head_copy` written in torch indexing from the text of include/rfa.h
(rfa_seq_head_copy), independently of the index function the kernel uses.  The schedules and `with_ulysses` run unchanged
on top of it.  `torch_copy` is also what tests/test_gpu_usp.py compares the HIP kernel with, bit for bit."""
import torch

from _ref_backend import RefBackend

PACK, UNPACK, MERGED_TO_SLOTS, SLOTS_TO_HEADS = 0, 1, 2, 3
CONTIGUOUS, ZIGZAG, STRIPE = 0, 1, 2


def merged_rows(layout, U, S):
    """(U, S) long: the merged row of slot j's row i"""
    j = torch.arange(U).view(U, 1)
    i = torch.arange(S).view(1, S)
    if layout == STRIPE:
        return (i * U + j).expand(U, S)
    if layout == ZIGZAG:
        C = S // 2
        return torch.where(i < C, j * C + i, U * C + (U - 1 - j) * C + (i - C))
    return (j * S + i).expand(U, S)


def torch_copy(op, layout, U, tensors, slots):
    """include/rfa.h: rfa_seq_head_copy — the slot buffer is U x [tensor 0 | tensor 1 | ...], each part [B][S][P][Hs][D]"""
    local = op in (PACK, SLOTS_TO_HEADS)
    B, D = tensors[0].shape[0], tensors[0].shape[-1]
    S = tensors[0].shape[1] if local else tensors[0].shape[1] // U
    assert slots.is_contiguous() and slots.numel() >= sum(t.numel() for t in tensors)
    buf = slots.view(-1)[:sum(t.numel() for t in tensors)].view(U, -1)
    base = 0
    for t in tensors:
        t5 = t if t.dim() == 5 else t.unsqueeze(2)                           # (B, rows, P, heads, D), a view
        P = t5.shape[2]
        Hs = t5.shape[3] // U if local else t5.shape[3]
        n = B * S * P * Hs * D
        part = buf[:, base:base + n].view(U, B, S, P, Hs, D)
        base += n
        if local:
            view = t5.view(B, S, P, U, Hs, D).permute(3, 0, 1, 2, 4, 5) if t5.is_contiguous() else \
                torch.stack([t5[:, :, :, j * Hs:(j + 1) * Hs] for j in range(U)])
            if op == PACK:
                part.copy_(view)
            else:
                for j in range(U):
                    t5[:, :, :, j * Hs:(j + 1) * Hs] = part[j]
        else:
            rows = merged_rows(layout, U, S).to(t.device)
            for j in range(U):
                if op == MERGED_TO_SLOTS:
                    part[j] = t5.index_select(1, rows[j])
                else:
                    t5[:, rows[j]] = part[j]


class UspBackend(RefBackend):
    serves_seq_head_exchange = True

    def __init__(self, serves=()):
        super().__init__(serves)
        self.name += "+seqhead"

    def seq_head_copy(self, op, layout, U, tensors, slots):
        torch_copy(op, layout, U, tensors, slots)
