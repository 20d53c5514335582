// rfa_seqhead.hip — the copies of the Ulysses head/sequence exchange (gfx950; include/rfa.h: rfa_seq_head_copy;
// ring_flash_attn.with_ulysses).  Around the one all-to-all of a direction the data has to change layout twice: heads are cut
// into U slices on the way in (one slot of the send buffer per destination), and the U received slots become ONE tensor of
// U times the rows in the wrapped schedule's own row order (contiguous, zigzag or stripe).  In torch that is a permute-copy per
// tensor, a concatenation, and for zigzag a chunk reorder; here it is one launch per side for ALL tensors of the call.
//
// Pure streaming, in the style of the copies of rfa_aux.hip: one thread per 16-byte chunk, one 16-byte load and one 16-byte
// store, no LDS, nothing kept.  A chunk index walks the SLOT side in memory order (rfa_seqhead_index.h), so that side is a
// dense run of 4 KiB per workgroup; on the strided side a run of Hs * D elements (the head slice of one row) is contiguous,
// i.e. at least 16 lanes of a wave at D = 128 touch one run.  The kernel holds a handful of registers, so occupancy is set by
// the 256-thread workgroups alone (8 waves per SIMD) — what a memory-bound copy wants.
// grid: x = ceil(max over tensors of nchunks / 256), y = tensor of the call.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"

namespace rfa {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void seq_head_copy_kernel(const SeqHeadParams p) {
  const SeqHeadTensor t = p.t[blockIdx.y];
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= t.nchunks) return;
  int64_t so, to;
  seqhead_chunk(p.g, t, c, &so, &to);
  // (2-byte elements: the offsets count them)
  uint16_t* slot = (uint16_t*)p.slots + so;
  uint16_t* strided = (uint16_t*)p.strided[blockIdx.y] + to;
  if (seqhead_from_slots(p.g.op)) *(u32x4*)strided = *(const u32x4*)slot;
  else *(u32x4*)slot = *(const u32x4*)strided;
}

int launch_seq_head_copy(const SeqHeadParams& p, hipStream_t stream) {
  uint32_t most = 0;
  for (int i = 0; i < p.ntensors; ++i) most = p.t[i].nchunks > most ? p.t[i].nchunks : most;
  if (most == 0) return 0;
  dim3 grid((most + 255u) / 256u, (unsigned)p.ntensors);
  hipLaunchKernelGGL(seq_head_copy_kernel, grid, dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rfa
