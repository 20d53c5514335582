// rfa_vdim.hip — attention forward and backward with a value head dim of its own on gfx950 (MI355X): QK head dims
// 136 … 192, V head dims 8 … 128 (multi-head latent attention as DeepSeek-V2/V3 and Kimi K2 train it: 192 / 128).
//
// The three kernels follow the kQ = 3 instances of rfa_bigd.hip — one wave per SIMD, an LDS row of 256 columns as two swizzled
// [rows][128] chunk tiles, LDS-DMA fills, transpose reads, read-ahead GEMMs — with a second quarter count for the V side:
//   * a Q / K / dQ / dK row has kQ = 3 quarters of 64 columns (12 k-steps, 6 accumulator blocks),
//     a V / dO / O / dV row has kQv = 2 (8 k-steps, 4 accumulator blocks) and lives in ONE chunk tile;
//   * every loop over the V side runs over two quarters only: the V / dO tiles (half the DMA pieces, half the LDS), the O and
//     dV accumulators, the k-steps of dP = dO V^T;
//   * D < 192 and Dv < 128 are zero padded by pointing the DMA lanes of the missing 16-byte chunks past the descriptor
//     range; V and dO tiles are bounded by Dv, everything else by D.
// No dropout instance is built (rfa_api.cpp refuses dropout with differing widths).  The helpers below repeat those of
// rfa_bigd.hip on purpose: that source, and with it every kernel instance it produces, stays as it is.
#include <type_traits>

#include "rfa_common.hpp"
#include "rfa_kernels.hpp"

namespace rfa {

constexpr int kVdWaves = 4;
constexpr int kVdThreads = kVdWaves * 64;
constexpr int kVdRows = kVdWaves * 32;        // query rows (forward, dQ) / keys (dK + dV) per workgroup
static_assert(kVdRows <= kDescMaxRows, "a buffer descriptor spans at most kDescMaxRows rows (rfa_kernels.hpp)");
constexpr int kVdQ = 3, kVdQv = 2;            // 64-column quarters that hold data: QK side / V side
constexpr int kVdNK = 4 * kVdQ, kVdNB = 2 * kVdQ;       // 16-wide k-steps of a contraction over D, 32-wide blocks of a D-wide accumulator row
constexpr int kVdNKv = 4 * kVdQv, kVdNBv = 2 * kVdQv;   // the same over Dv
constexpr int kVdOob = 0x7ffffff0;            // byte offset past every descriptor range: the lane reads / DMAs zeros

// Per-lane global byte offsets of the LDS-DMA pieces one wave issues for a tile of R rows and kC chunk tiles (kC = 2: a QK-side
// row, kC = 1: a V-side row).  Piece P (1 KiB = 4 rows of a chunk tile) belongs to chunk c = P / (R / 4); waves take the
// pieces wave, wave + 4, ...
template <int R, int kC>
__device__ __forceinline__ void vd_dma_offsets(int wave, int lane, int row_stride, int D, int (&voff)[kC * R / 16]) {
#pragma unroll
  for (int i = 0; i < kC * R / 16; ++i) {
    const int P = wave + kVdWaves * i;
    const int c = P / (R / 4), pc = P % (R / 4);
    int row, ch;
    dma_lane_src<128>(pc, lane, row, ch);
    const int col = 128 * c + 8 * ch;
    voff[i] = col < D ? (row * row_stride + col) * 2 : kVdOob;
  }
}
template <int R, int kC>
__device__ __forceinline__ void vd_dma_piece(dma_rsrc_t r, int lds_base, int wave, const int (&voff)[kC * R / 16], int i) {
  const int P = wave + kVdWaves * i;
  const int c = P / (R / 4), pc = P % (R / 4);
  dma_load128(r, lds_base + c * R * 256 + pc * 1024, voff[i]);
}
template <int R, int kC>
__device__ __forceinline__ void vd_dma_tile(dma_rsrc_t r, int lds_base, int wave, const int (&voff)[kC * R / 16]) {
#pragma unroll
  for (int i = 0; i < kC * R / 16; ++i) vd_dma_piece<R, kC>(r, lds_base, wave, voff, i);
}

// kN MFMAs whose A operands come from LDS: operand i is fetched by fa(i) — kReads LDS instructions — kAhead MFMAs before
// mm(i, a) consumes it (rfa_bigd.hip: big_gemm); side(i) is issued behind MFMA i (the next tile's DMA pieces)
constexpr int kVdAhead = 4;
struct vd_no_side {
  __device__ __forceinline__ void operator()(int) const {}
};
template <typename T, int kN, int kReads, typename FA, typename MM, typename SD = vd_no_side>
__device__ __forceinline__ void vd_gemm(FA fa, MM mm, SD side = SD()) {
  constexpr int kAhead = kVdAhead < kN ? kVdAhead : kN;
  vec8<T> a[kN];
#pragma unroll
  for (int i = 0; i < kAhead; ++i) a[i] = fa(i);
#pragma unroll
  for (int i = 0; i < kN; ++i) {
    if (i + kAhead < kN) a[i + kAhead] = fa(i + kAhead);
    mm(i, a[i]);
    side(i);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, kReads * kAhead, 0);
#pragma unroll
  for (int i = 0; i < kN - kAhead; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, kAhead, 0);
}

// fp32 rows of a C-layout accumulator: columns 32 dblk + 8 jj + 4 g .. + 3 of lane (row, g), bounded by `width`
template <int kNBx, typename F>
__device__ __forceinline__ void vd_rows_f32(float* row_ptr, int g, int width, F f) {
#pragma unroll
  for (int dblk = 0; dblk < kNBx; ++dblk)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int d0 = 32 * dblk + 8 * jj + 4 * g;
      if (d0 < width) f((f32x4*)(row_ptr + d0), dblk, 4 * jj);
    }
}

// =====================================================================================
// forward: S = Q K^T over D, O = P V over Dv
// =====================================================================================
constexpr int kVdKV = 64;                          // keys per K/V tile (forward, dQ)
constexpr int kVdChunkTile = kVdKV * 256;          // [64][128] chunk tile: 16 KiB
constexpr int kVdKTile = 2 * kVdChunkTile;         // K: [64][256]
constexpr int kVdOffV = 2 * kVdKTile;              // V stages ([64][128] each) behind the two K stages
constexpr int kVdFwdSmem = kVdOffV + 2 * kVdChunkTile;   // K[2] V[2]: 96 KiB

template <typename T>
__global__ __launch_bounds__(kVdThreads) void vd_fwd_kernel(const FwdParamsVd pv) {
  const FwdParams& p = pv.base;
  const int Dv = pv.Dv;
  constexpr int kNK = kVdNK, kNBv = kVdNBv;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_t* smem = (lds_t*)smem_raw;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5;
  const int l31 = lane & 31;

  int idx = blockIdx.x;
  const int G = p.H / p.Hk;
  const int hk = idx % p.Hk;
  idx /= p.Hk;
  const int gq = idx % G;
  idx /= G;
  int qblk_i, b;
  split_block_batch<RFA_BATCH_FAST_Q>(idx, p.nqblk, p.B, qblk_i, b);
  const int qblk = p.nqblk - 1 - qblk_i;
  const int h = hk * G + gq;

  const SeqSpan qs = resolve_span(p.cu_q, b, p.Sq, p.q_half);
  const SeqSpan ks = resolve_span(p.cu_k, b, p.Sk, p.k_half);
  const int lq = qs.len, lk = ks.len;
  const int qwg0 = qblk * kVdRows;
  if (qwg0 >= lq) return;
  const int off = lk - lq + p.shift + p.shift_lens * lk;   // bottom-right alignment, moved by the block's place in the full sequence (rfa.h: mask_shift, mask_shift_lens)
  const int qw0 = qwg0 + wave * 32;
  const int qrow = qw0 + l31;
  const int qrow_c = qrow < lq ? qrow : lq - 1;
  const int64_t qbatch = p.cu_q ? 0 : (int64_t)b;
  const int64_t kbatch = p.cu_k ? 0 : (int64_t)b;

  const T* qbase = (const T*)p.q + qbatch * p.q_st.batch + (qs.row0 + qrow_c) * p.q_st.row + (int64_t)h * p.q_st.head;
  const T* kbase = (const T*)p.k + kbatch * p.k_st.batch + ks.row0 * p.k_st.row + (int64_t)hk * p.k_st.head;
  const T* vbase = (const T*)p.v + kbatch * p.v_st.batch + ks.row0 * p.v_st.row + (int64_t)hk * p.v_st.head;

  vec8<T> qf[kNK];
#pragma unroll
  for (int kk = 0; kk < kNK; ++kk) {
    const int d0 = 16 * kk + 8 * g;
    qf[kk] = d0 < p.D ? *(const vec8<T>*)(qbase + d0) : zero8<T>();
  }

  const int qend = (qwg0 + kVdRows < lq) ? qwg0 + kVdRows : lq;
  const bool win = p.wl >= 0 || (p.wr >= 0 && !p.causal);       // (rfa_kernels.hpp: windowed)
  const bool hi = win ? p.wr >= 0 : p.causal != 0;
  const bool lo = win && p.wl >= 0;
  const int wr = win ? p.wr : 0, wl = win ? p.wl : 0;
  int kmax = lk;
  if (hi && qend + off + wr < kmax) kmax = qend + off + wr;
  const int ntiles = kmax > 0 ? (kmax + kVdKV - 1) / kVdKV : 0;
  int kmin = lo ? qwg0 + off - wl : 0;
  kmin = kmin > 0 ? (kmin < lk ? kmin : lk) : 0;          // (a shifted band may start behind the last key)
  const int jt0 = kmin / kVdKV;
  if (jt0 >= ntiles && p.out_acc != nullptr && !p.acc_init) return;  // rows wholly outside the band: nothing to merge

  constexpr int kPk = kVdKV / 8, kPv = kVdKV / 16;        // DMA pieces per wave: K tile (two chunk tiles), V tile (one)
  int voff_k[kPk], voff_v[kPv];
  vd_dma_offsets<kVdKV, 2>(wave, lane, (int)p.k_st.row, p.D, voff_k);
  vd_dma_offsets<kVdKV, 1>(wave, lane, (int)p.v_st.row, Dv, voff_v);
  struct TileLoad {
    dma_rsrc_t rk, rv;
    int kb, vb;
  };
  auto prep_tile = [&](int j, int stage) {               // descriptors and LDS targets of a K/V tile (scalar work)
    int rows = lk - j * kVdKV;
    rows = rows < kVdKV ? rows : kVdKV;
    const int nk = rows > 0 ? ((rows - 1) * (int)p.k_st.row + p.D) * 2 : 0;
    const int nv = rows > 0 ? ((rows - 1) * (int)p.v_st.row + Dv) * 2 : 0;
    TileLoad t;
    t.rk = make_dma_rsrc(kbase + (int64_t)j * kVdKV * p.k_st.row, nk);
    t.rv = make_dma_rsrc(vbase + (int64_t)j * kVdKV * p.v_st.row, nv);
    t.kb = lds_addr(smem) + stage * kVdKTile;
    t.vb = lds_addr(smem) + kVdOffV + stage * kVdChunkTile;
    return t;
  };
  constexpr int kPieces = kPk + kPv;                     // DMA pieces per wave and tile (K, then V)
  auto issue_piece = [&](const TileLoad& t, int i) {
    if (i < kPk) vd_dma_piece<kVdKV, 2>(t.rk, t.kb, wave, voff_k, i);
    else vd_dma_piece<kVdKV, 1>(t.rv, t.vb, wave, voff_v, i - kPk);
  };
  auto load_tile = [&](int j, int stage) {
    const TileLoad t = prep_tile(j, stage);
#pragma unroll
    for (int i = 0; i < kPieces; ++i) issue_piece(t, i);
  };

  // fragment addresses inside a chunk tile: K rows (A operand of S^T = K Q^T), V^T by transpose reads
  int koff[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) koff[kk] = lds_addr(smem) + tile_off(l31, 2 * kk + g);
  int voff[4][2];
#pragma unroll
  for (int dblk = 0; dblk < 4; ++dblk)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) voff[dblk][hh] = lds_addr(smem) + tr_off_d<128>(lane, dblk, 8 * hh + 4 * g);

  const float c = p.scale * kLog2e;
  float m = -INFINITY;
  float lsum = 0.f;
  f32x16 o[kNBv];
#pragma unroll
  for (int i = 0; i < kNBv; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;

  load_tile(jt0, 0);                     // unconditional (rows past the end read as zero)
  wait_all_vmem();
  __syncthreads();

  for (int j = jt0; j < ntiles; ++j) {
    const int stage = (j - jt0) & 1;
    const bool more = j + 1 < ntiles;
    const TileLoad nxt = prep_tile(more ? j + 1 : j, stage ^ 1);
    const int kbo = stage * kVdKTile, vbo = kVdOffV + stage * kVdChunkTile;
    const int kt0 = j * kVdKV;
    const bool active = (qw0 < lq) && !(hi && kt0 > qw0 + 31 + off + wr) && !(lo && kt0 + kVdKV - 1 < qw0 + off - wl);
    if (!active && more) {
#pragma unroll
      for (int i = 0; i < kPieces; ++i) issue_piece(nxt, i);
    }
    if (active) {
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      vd_gemm<T, 2 * kNK, 1>(
          [&](int i) {                                  // i = t * kNK + kk
            const int t = i / kNK, kk = i % kNK;
            return lds_read128<T>(lds_ptr(koff[kk & 7]) + kbo + (kk >> 3) * kVdChunkTile + t * 32 * 256);
          },
          [&](int i, vec8<T> a) { s[i / kNK] = mfma(a, qf[i % kNK], s[i / kNK]); },
          [&](int i) {                                  // the next tile's DMA pieces in the shadows of the first MFMAs
            if (i < kPieces && more) issue_piece(nxt, i);
          });
      const bool need_mask = (kt0 + kVdKV > lk) || (hi && kt0 + kVdKV - 1 > qw0 + off + wr) || (lo && kt0 < qw0 + 31 + off - wl);
      if (need_mask) {
        const int lim = hi ? ((qrow + off + wr < lk - 1) ? qrow + off + wr : lk - 1) : lk - 1;
        const int lim_lo = lo ? qrow + off - wl : -0x40000000;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kt0 + 32 * t + crow(r, g);
            if (key > lim || key < lim_lo) s[t][r] = -INFINITY;
          }
      }
      float mloc = s[0][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s[0][r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[1][r]);
      mloc = max_xor32(mloc);
      const float mnew = fmaxf(m, mloc);
      // deferred rescale as in rfa_fwd.hip: while no row of the wave grew its max by more than 8 log2 units the stale
      // max stays (P <= 2^8, exact in fp32) and the rescale of O is skipped
      if (!__all((mnew - m) * c <= 8.f)) {
        const float msafe = (mnew == -INFINITY) ? 0.f : mnew;
        const float alpha = fast_exp2(m * c - msafe * c);
        m = mnew;
        lsum *= alpha;
#pragma unroll
        for (int i = 0; i < kNBv; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      }
      const float mc = ((m == -INFINITY) ? 0.f : m) * c;
      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pe = fast_exp2(__builtin_fmaf(s[t][r], c, -mc));
          s[t][r] = pe;
          psum += pe;
        }
      lsum += psum;
      {
        vec8<T> pb[4];                                  // [t][ks2]
#pragma unroll
        for (int x = 0; x < 4; ++x) pb[x] = pack8<T>(s[x >> 1], 8 * (x & 1));
        vd_gemm<T, 4 * kNBv, 2>(
            [&](int i) {                                // i = (t, ks2) * kNBv + dblk: rows 32 t + 16 ks2 of the V tile
              const int dblk = i % kNBv, cimm = vbo + (i / kNBv) * 16 * 256;
              return concat<T>(lds_read_tr<T>(lds_ptr(voff[dblk][0]) + cimm), lds_read_tr<T>(lds_ptr(voff[dblk][1]) + cimm));
            },
            [&](int i, vec8<T> a) { o[i % kNBv] = mfma(a, pb[i / kNBv], o[i % kNBv]); });
      }
    }
    wait_all_vmem();           // tile j+1 has landed
    __syncthreads();
  }

  if (qrow >= lq) return;
  const float l = sum_xor32(lsum);
  const bool has = l > 0.f;
  const float inv = has ? 1.f / l : 0.f;
  const float blse = has ? m * p.scale + __logf(l) : INFINITY;
  const int64_t orow = qs.row0 + qrow;
  if (p.out_acc == nullptr) {
    T* ob = (T*)p.out + qbatch * p.out_st.batch + orow * p.out_st.row + (int64_t)h * p.out_st.head;
    store_rows16<T, false, kNBv>(ob, o, inv, g, Dv, true);
    if (g == 0) p.lse[qbatch * p.lse_batch + (int64_t)h * p.lse_head + orow] = blse;
  } else {
    // fused online merge into the caller's fp32 accumulators: the epilogue of rfa_fwd.hip
    float* ab = p.out_acc + qbatch * p.out_acc_st.batch + orow * p.out_acc_st.row + (int64_t)h * p.out_acc_st.head;
    float* lp = p.lse_acc + qbatch * p.lse_acc_batch + (int64_t)h * p.lse_acc_head + orow;
    if (p.acc_init) {
      vd_rows_f32<kNBv>(ab, g, Dv, [&](f32x4* dst, int dblk, int r0) {
        f32x4 x;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = o[dblk][r0 + e] * inv;
        *dst = x;
      });
      if (g == 0) *lp = has ? blse : -INFINITY;
    } else if (has) {
      const float lold = *lp;
      const float mx = fmaxf(lold, blse);
      const float eo = __expf(lold - mx);
      const float eb = __expf(blse - mx);
      const float den = eo + eb;
      const float wo = eo / den;
      const float wb = eb / den * inv;
      const float lnew = mx + __logf(den);
      vd_rows_f32<kNBv>(ab, g, Dv, [&](f32x4* dst, int dblk, int r0) {
        f32x4 x = *dst;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] * wo + o[dblk][r0 + e] * wb;
        *dst = x;
      });
      if (g == 0) *lp = lnew;
    }
  }
}

// =====================================================================================
// dQ (7-GEMM form: S over D and dP over Dv recomputed, dQ over D)
// =====================================================================================
template <typename T>
__global__ __launch_bounds__(kVdThreads) void vd_dq_kernel(const BwdParamsVd pv) {
  const BwdParams& p = pv.base;
  const int Dv = pv.Dv;
  constexpr int kNK = kVdNK, kNB = kVdNB, kNKv = kVdNKv;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_t* smem = (lds_t*)smem_raw;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5;
  const int l31 = lane & 31;

  int idx = blockIdx.x;
  const int G = p.H / p.Hk;
  const int hk = idx % p.Hk;
  idx /= p.Hk;
  const int gq = idx % G;
  idx /= G;
  int qblk_i, b;
  split_block_batch<RFA_BATCH_FAST_Q>(idx, p.nqblk, p.B, qblk_i, b);
  const int qblk = p.nqblk - 1 - qblk_i;
  const int h = hk * G + gq;

  const SeqSpan qs = resolve_span(p.cu_q, b, p.Sq, p.q_half);
  const SeqSpan ks = resolve_span(p.cu_k, b, p.Sk, p.k_half);
  const int lq = qs.len, lk = ks.len;
  const int qwg0 = qblk * kVdRows;
  if (qwg0 >= lq) return;
  const int off = lk - lq + p.shift + p.shift_lens * lk;   // bottom-right alignment, moved by the block's place in the full sequence (rfa.h: mask_shift, mask_shift_lens)
  const int qw0 = qwg0 + wave * 32;
  const int qrow = qw0 + l31;
  const int qrow_c = qrow < lq ? qrow : lq - 1;
  const int64_t qbatch = p.cu_q ? 0 : (int64_t)b;
  const int64_t kbatch = p.cu_k ? 0 : (int64_t)b;
  const int64_t arow = qs.row0 + qrow_c;

  const T* qbase = (const T*)p.q + qbatch * p.q_st.batch + arow * p.q_st.row + (int64_t)h * p.q_st.head;
  const T* dobase = (const T*)p.dout + qbatch * p.dout_st.batch + arow * p.dout_st.row + (int64_t)h * p.dout_st.head;
  const T* kbase = (const T*)p.k + kbatch * p.k_st.batch + ks.row0 * p.k_st.row + (int64_t)hk * p.k_st.head;
  const T* vbase = (const T*)p.v + kbatch * p.v_st.batch + ks.row0 * p.v_st.row + (int64_t)hk * p.v_st.head;

  vec8<T> qf[kNK], dof[kNKv];
#pragma unroll
  for (int kk = 0; kk < kNK; ++kk) {
    const int d0 = 16 * kk + 8 * g;
    qf[kk] = d0 < p.D ? *(const vec8<T>*)(qbase + d0) : zero8<T>();
  }
#pragma unroll
  for (int kk = 0; kk < kNKv; ++kk) {
    const int d0 = 16 * kk + 8 * g;
    dof[kk] = d0 < Dv ? *(const vec8<T>*)(dobase + d0) : zero8<T>();
  }
  const float L2 = p.lse[qbatch * p.lse_batch + (int64_t)h * p.lse_head + arow] * kLog2e;
  const float dlt = p.delta[qbatch * p.delta_batch + (int64_t)h * p.delta_head + arow];

  const int qend = (qwg0 + kVdRows < lq) ? qwg0 + kVdRows : lq;
  const bool win = p.wl >= 0 || (p.wr >= 0 && !p.causal);       // (rfa_kernels.hpp: windowed)
  const bool hi = win ? p.wr >= 0 : p.causal != 0;
  const bool lo = win && p.wl >= 0;
  const int wr = win ? p.wr : 0, wl = win ? p.wl : 0;
  int kmax = lk;
  if (hi && qend + off + wr < kmax) kmax = qend + off + wr;
  const int ntiles = kmax > 0 ? (kmax + kVdKV - 1) / kVdKV : 0;
  int kmin = lo ? qwg0 + off - wl : 0;
  kmin = kmin > 0 ? (kmin < lk ? kmin : lk) : 0;          // (a shifted band may start behind the last key)
  const int jt0 = kmin / kVdKV;
  if (jt0 >= ntiles && p.dq_acc != nullptr && !p.acc_init) return;   // rows wholly outside the band add nothing to dq_acc

  int voff_k[kVdKV / 8], voff_v[kVdKV / 16];
  vd_dma_offsets<kVdKV, 2>(wave, lane, (int)p.k_st.row, p.D, voff_k);
  vd_dma_offsets<kVdKV, 1>(wave, lane, (int)p.v_st.row, Dv, voff_v);
  auto load_tile = [&](int j, int stage) {
    int rows = lk - j * kVdKV;
    rows = rows < kVdKV ? rows : kVdKV;
    const int nk = rows > 0 ? ((rows - 1) * (int)p.k_st.row + p.D) * 2 : 0;
    const int nv = rows > 0 ? ((rows - 1) * (int)p.v_st.row + Dv) * 2 : 0;
    const dma_rsrc_t rk = make_dma_rsrc(kbase + (int64_t)j * kVdKV * p.k_st.row, nk);
    const dma_rsrc_t rv = make_dma_rsrc(vbase + (int64_t)j * kVdKV * p.v_st.row, nv);
    vd_dma_tile<kVdKV, 2>(rk, lds_addr(smem) + stage * kVdKTile, wave, voff_k);
    vd_dma_tile<kVdKV, 1>(rv, lds_addr(smem) + kVdOffV + stage * kVdChunkTile, wave, voff_v);
  };
  int koff[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) koff[kk] = lds_addr(smem) + tile_off(l31, 2 * kk + g);
  int toff[4][2];
#pragma unroll
  for (int dblk = 0; dblk < 4; ++dblk)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) toff[dblk][hh] = lds_addr(smem) + tr_off_d<128>(lane, dblk, 8 * hh + 4 * g);

  const float c = p.scale * kLog2e;
  f32x16 dq[kNB];
#pragma unroll
  for (int i = 0; i < kNB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;

  load_tile(jt0, 0);
  wait_all_vmem();
  __syncthreads();

  for (int j = jt0; j < ntiles; ++j) {
    const int stage = (j - jt0) & 1;
    if (j + 1 < ntiles) load_tile(j + 1, stage ^ 1);     // (issued in front of this tile: rfa_bigd.hip, dq_big_kernel)
    const int kbo = stage * kVdKTile, vbo = kVdOffV + stage * kVdChunkTile;
    const int kt0 = j * kVdKV;
    const bool active = (qw0 < lq) && !(hi && kt0 > qw0 + 31 + off + wr) && !(lo && kt0 + kVdKV - 1 < qw0 + off - wl);
    if (active) {
      const bool need_mask = (kt0 + kVdKV > lk) || (hi && kt0 + kVdKV - 1 > qw0 + off + wr) || (lo && kt0 < qw0 + 31 + off - wl);
      const int lim = hi ? ((qrow + off + wr < lk - 1) ? qrow + off + wr : lk - 1) : lk - 1;
      const int lim_lo = lo ? qrow + off - wl : -0x40000000;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        vd_gemm<T, kNK + kNKv, 1>(
            [&](int i) {                                // i < kNK: K tile rows for S; else V tile rows for dP
              const int kk = i < kNK ? i : i - kNK;
              const int base = i < kNK ? kbo + (kk >> 3) * kVdChunkTile : vbo;
              return lds_read128<T>(lds_ptr(koff[kk & 7]) + base + t * 32 * 256);
            },
            [&](int i, vec8<T> a) {
              if (i < kNK) s = mfma(a, qf[i < kNK ? i : 0], s);
              else dp = mfma(a, dof[i < kNK ? 0 : i - kNK], dp);
            });
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = fast_exp2(__builtin_fmaf(s[r], c, -L2));
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kt0 + 32 * t + crow(r, g);
            s[r] = (key > lim || key < lim_lo) ? 0.f : s[r];
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = s[r] * (dp[r] - dlt);
        {
          const vec8<T> dsb[2] = {pack8<T>(s, 0), pack8<T>(s, 8)};
          vd_gemm<T, 2 * kNB, 2>(
              [&](int i) {                              // i = ks2 * kNB + dblk
                const int dblk = i % kNB, cimm = kbo + (32 * t + 16 * (i / kNB)) * 256 + (dblk >> 2) * kVdChunkTile;
                return concat<T>(lds_read_tr<T>(lds_ptr(toff[dblk & 3][0]) + cimm), lds_read_tr<T>(lds_ptr(toff[dblk & 3][1]) + cimm));
              },
              [&](int i, vec8<T> a) { dq[i % kNB] = mfma(a, dsb[i / kNB], dq[i % kNB]); });
        }
      }
    }
    wait_all_vmem();
    __syncthreads();
  }

  if (qrow >= lq) return;
  const int64_t orow = qs.row0 + qrow;
  if (p.dq_acc == nullptr) {
    T* ob = (T*)p.dq + qbatch * p.dq_st.batch + orow * p.dq_st.row + (int64_t)h * p.dq_st.head;
    store_rows16<T, false, kNB>(ob, dq, p.scale, g, p.D, true);
  } else {
    float* ab = p.dq_acc + qbatch * p.dq_acc_st.batch + orow * p.dq_acc_st.row + (int64_t)h * p.dq_acc_st.head;
    vd_rows_f32<kNB>(ab, g, p.D, [&](f32x4* dst, int dblk, int r0) {
      f32x4 x;
      if (p.acc_init) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = 0.f;
      } else {
        x = *dst;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] += dq[dblk][r0 + e] * p.scale;
      *dst = x;
    });
  }
}

// =====================================================================================
// dK + dV in ONE launch (from rfa_bigd.hip: dkdv_fused_big_kernel, plain instance)
// =====================================================================================
// K_w (this wave's 32 keys, D wide) is a register B operand; the workgroup's 128 V rows sit in LDS once, Dv wide: ONE chunk
// tile (32 KiB).  dK^T (6 blocks) and dV^T (4 blocks) of the K/V group are summed in registers: 96 + 64 accumulator registers.
constexpr int kVdQr = 32;                            // query rows per Q/dO tile
constexpr int kVdQChunk = kVdQr * 256;               // [32][128] chunk tile: 8 KiB
constexpr int kVdQTile = 2 * kVdQChunk;              // Q: [32][256]
constexpr int kVdStages = 2;
constexpr int kVdOffDo = kVdStages * kVdQTile;       // 32 KiB: dO stages ([32][128] each) behind the Q stages
constexpr int kVdOffVw = kVdOffDo + kVdStages * kVdQChunk;   // 48 KiB: V rows [128][128]
constexpr int kVdVChunk = kVdRows * 256;             // 32 KiB
constexpr int kVdOffStat = kVdOffVw + kVdVChunk;     // 80 KiB: per stage lse[64 slots, 32 used], delta[64 slots]
constexpr int kVdStatBytes = 2 * 256;
constexpr int kVdKvSmem = kVdOffStat + kVdStages * kVdStatBytes;

// 4-byte LDS-DMA (buffer_load_dword ... lds): lane L's dword lands at lds_wave_base + 4 L, out-of-range lanes write zeros
__device__ __forceinline__ void vd_dma_load32(dma_rsrc_t r, int lds_wave_base, int voffset) {
  asm volatile("s_mov_b32 m0, %2\n\tbuffer_load_dword %0, %1, 0 offen lds"
               :
               : "v"(voffset), "s"(r.w), "s"(__builtin_amdgcn_readfirstlane(lds_wave_base))
               : "m0");
}

template <typename T>
__global__ __launch_bounds__(kVdThreads) void vd_dkdv_kernel(const BwdParamsVd pv) {
  const BwdParams& p = pv.base;
  const int Dv = pv.Dv;
  constexpr int kNK = kVdNK, kNB = kVdNB, kNKv = kVdNKv, kNBv = kVdNBv;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_t* smem = (lds_t*)smem_raw;
  if (lds_addr(smem) & 0xffff) __builtin_trap();     // the stage / fragment XORs below need a 64 KiB-aligned block
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5;
  const int l31 = lane & 31;

  int idx = blockIdx.x;
  const int G = p.H / p.Hk;
  const int hk = idx % p.Hk;
  idx /= p.Hk;
  const int nsplit = p.nsplit;
  const int qsplit = idx % nsplit;
  idx /= nsplit;
  int kblk, b;
  split_block_batch<RFA_BATCH_FAST_KV>(idx, p.nkblk, p.B, kblk, b);
  const int h0 = hk * G;

  const SeqSpan qs = resolve_span(p.cu_q, b, p.Sq, p.q_half);
  const SeqSpan ks = resolve_span(p.cu_k, b, p.Sk, p.k_half);
  const int lq = qs.len, lk = ks.len;
  const int kwg0 = kblk * kVdRows;
  if (kwg0 >= lk) return;
  const int off = lk - lq + p.shift + p.shift_lens * lk;   // bottom-right alignment, moved by the block's place in the full sequence (rfa.h: mask_shift, mask_shift_lens)
  const int kw0 = kwg0 + wave * 32;
  const int krow = kw0 + l31;
  const int64_t qbatch = p.cu_q ? 0 : (int64_t)b;
  const int64_t kbatch = p.cu_k ? 0 : (int64_t)b;

  const T* kbase = (const T*)p.k + kbatch * p.k_st.batch + ks.row0 * p.k_st.row + (int64_t)hk * p.k_st.head;
  const T* vbase = (const T*)p.v + kbatch * p.v_st.batch + ks.row0 * p.v_st.row + (int64_t)hk * p.v_st.head;
  const T* qbase0 = (const T*)p.q + qbatch * p.q_st.batch + qs.row0 * p.q_st.row + (int64_t)h0 * p.q_st.head;
  const T* dobase0 = (const T*)p.dout + qbatch * p.dout_st.batch + qs.row0 * p.dout_st.row + (int64_t)h0 * p.dout_st.head;
  const float* lsebase0 = p.lse + qbatch * p.lse_batch + (int64_t)h0 * p.lse_head + qs.row0;
  const float* dltbase0 = p.delta + qbatch * p.delta_batch + (int64_t)h0 * p.delta_head + qs.row0;

  const bool win = p.wl >= 0 || (p.wr >= 0 && !p.causal);
  const bool hi = win ? p.wr >= 0 : p.causal != 0;
  const bool lo = win && p.wl >= 0;
  const int wr = win ? p.wr : 0, wl = win ? p.wl : 0;
  int qfirst = 0;
  if (hi) {
    qfirst = kwg0 - off - wr;
    qfirst = qfirst < 0 ? 0 : (qfirst < lq ? qfirst : lq);   // (a shifted band may start behind the last query row ...)
  }
  int qlast = lq;
  if (lo && kwg0 + kVdRows - off + wl < qlast) qlast = kwg0 + kVdRows - off + wl;
  if (qlast < 0) qlast = 0;                    // (... or end in front of the first)
  const int jt0 = qfirst / kVdQr;
  int jt1 = (qlast + kVdQr - 1) / kVdQr;
  if (jt1 <= jt0) jt1 = jt0;
  // this workgroup's tiles: every nsplit-th one counted from the top; the shares' fp32 partials are summed by reduce_kernel
  const int jtop = jt1 - 1 - qsplit;
  const int ntile_q = jtop >= jt0 ? (jtop - jt0) / nsplit + 1 : 0;

  // the workgroup's 128 V rows -> LDS (one DMA burst; rows past the end of the sequence read as zeros), this wave's K rows
  // -> registers (B operand of S = Q K_w^T)
  {
    int voff_v[kVdRows / 16];
    vd_dma_offsets<kVdRows, 1>(wave, lane, (int)p.v_st.row, Dv, voff_v);
    int rows = lk - kwg0;
    rows = rows < kVdRows ? rows : kVdRows;
    const dma_rsrc_t rv = make_dma_rsrc(vbase + (int64_t)kwg0 * p.v_st.row, ((rows - 1) * (int)p.v_st.row + Dv) * 2);
    vd_dma_tile<kVdRows, 1>(rv, lds_addr(smem) + kVdOffVw, wave, voff_v);
  }
  vec8<T> kwr[kNK];
  {
    const int kr = krow < lk ? krow : lk - 1;
    const T* kp = kbase + (int64_t)kr * p.k_st.row;
#pragma unroll
    for (int kk = 0; kk < kNK; ++kk) {
      const int d0 = 16 * kk + 8 * g;
      kwr[kk] = d0 < p.D ? *(const vec8<T>*)(kp + d0) : zero8<T>();
    }
  }

  constexpr int kPq = kVdQr / 8, kPdo = kVdQr / 16;      // DMA pieces per wave: Q tile (two chunk tiles), dO tile (one)
  int voff_q[kPq], voff_do[kPdo];
  vd_dma_offsets<kVdQr, 2>(wave, lane, (int)p.q_st.row, p.D, voff_q);
  vd_dma_offsets<kVdQr, 1>(wave, lane, (int)p.dout_st.row, Dv, voff_do);
  const int ntile = ntile_q * G;
  // Tiles are walked from the top one down, and for every tile the G heads of the group; loads past the last tile are issued
  // with an empty range (they write zeros).
  int ld_n = 0, ld_g = 0, ld_j = jtop > 0 ? jtop : 0;
  struct TileLoad {
    dma_rsrc_t rq, rdo, rs;
    int qb, dob, sbase;
  };
  auto prep_tile = [&]() {
    const bool valid = ld_n < ntile;
    const int j = valid ? ld_j : 0;
    const int stage = ld_n & (kVdStages - 1);
    const T* qbase = qbase0 + (int64_t)ld_g * p.q_st.head;
    const T* dobase = dobase0 + (int64_t)ld_g * p.dout_st.head;
    const float* statbase = (wave ? dltbase0 + (int64_t)ld_g * p.delta_head : lsebase0 + (int64_t)ld_g * p.lse_head) + j * kVdQr;
    ++ld_n;
    if (++ld_g >= G) {
      ld_g = 0;
      ld_j -= nsplit;
    }
    int rows = lq - j * kVdQr;
    rows = rows < kVdQr ? rows : kVdQr;
    rows = valid && rows > 0 ? rows : 0;
    const int nq = rows > 0 ? ((rows - 1) * (int)p.q_st.row + p.D) * 2 : 0;
    const int ndo = rows > 0 ? ((rows - 1) * (int)p.dout_st.row + Dv) * 2 : 0;
    TileLoad t;
    t.rq = make_dma_rsrc(qbase + (int64_t)j * kVdQr * p.q_st.row, nq);
    t.rdo = make_dma_rsrc(dobase + (int64_t)j * kVdQr * p.dout_st.row, ndo);
    t.rs = make_dma_rsrc(statbase, rows * 4);
    t.qb = lds_addr(smem) + stage * kVdQTile;
    t.dob = lds_addr(smem) + kVdOffDo + stage * kVdQChunk;
    t.sbase = lds_addr(smem) + kVdOffStat + stage * kVdStatBytes + wave * 256;
    return t;
  };
  constexpr int kPieces = kPq + kPdo + 1;                // per wave and tile: Q pieces, dO pieces, one statistics row
  auto issue_piece = [&](const TileLoad& t, int i) {     // i = 0 .. kPieces-1 (compile-time at every call site)
    if (i < kPq) vd_dma_piece<kVdQr, 2>(t.rq, t.qb, wave, voff_q, i);
    else if (i < kPq + kPdo) vd_dma_piece<kVdQr, 1>(t.rdo, t.dob, wave, voff_do, i - kPq);
    else if (wave < 2) vd_dma_load32(t.rs, t.sbase, lane * 4);
  };

  const int aq0 = lds_addr(smem) + tile_off(l31, g);                                  // Q rows (A operand of S), stage 0
  const int ado0 = lds_addr(smem) + kVdOffDo + tile_off(l31, g);                      // dO rows (A operand of dP), stage 0
  const int av = lds_addr(smem) + kVdOffVw + 32 * wave * 256 + tile_off(l31, g);      // this wave's V rows (B operand of dP)
  int tq0[2], tdo0[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    tq0[hh] = lds_addr(smem) + tr_off_d<128>(lane, 0, 8 * hh + 4 * g);
    tdo0[hh] = tq0[hh] + kVdOffDo;
  }
  const int sa0 = lds_addr(smem) + kVdOffStat + 4 * g * 4;

  const float c = p.scale * kLog2e;
  f32x16 acck[kNB], accv[kNBv];
#pragma unroll
  for (int i = 0; i < kNB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acck[i][r] = 0.f;
#pragma unroll
  for (int i = 0; i < kNBv; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) accv[i][r] = 0.f;

  // dS hand-off (rfa_dqs.hip reads the blocks back): block (b, h, qt = tile, kb = key / 32) of the scratch, slot order and row
  // layout of rfa_bwd.hip's kSpill instances
  const bool spill = p.ds != nullptr;
  const int ds_lane = 16 * (16 * (l31 >> 2) + 4 * g + (l31 & 3));
  const int ds_nkb = ds_blocks(p.Sk, p.k_half);
  const int64_t ds_head_bytes = spill ? p.ds_head_blocks * kDsBlockBytes : 0;
  const char* ds_b = spill ? (const char*)p.ds + ds_base_blocks(p, b) * kDsBlockBytes : nullptr;
  const int ds_kb = __builtin_amdgcn_readfirstlane(kblk * (kVdRows / 32) + wave);

  {
    const TileLoad t0 = prep_tile();
#pragma unroll
    for (int i = 0; i < kPieces; ++i) issue_piece(t0, i);
  }
  wait_all_vmem();                                     // V rows, K_w, tile 0
  __syncthreads();

  int j = jtop, cg = 0;
  for (int f = 0; f < ntile; ++f) {
    const TileLoad nxt = prep_tile();                  // tile f + 1 goes into the other stage
    const int sq = (f & (kVdStages - 1)) * kVdQTile, sd = (f & (kVdStages - 1)) * kVdQChunk;
    const int aq = aq0 + sq, ado = ado0 + sd;
    const int tq[2] = {tq0[0] + sq, tq0[1] + sq}, tdo[2] = {tdo0[0] + sd, tdo0[1] + sd};
    const int sa = sa0 + (f & (kVdStages - 1)) * kVdStatBytes;
    const int qs0 = j * kVdQr;
    const bool active = (kw0 < lk) && (qs0 < lq) && !(hi && qs0 + 31 + off + wr < kw0) && !(lo && qs0 + off - wl > kw0 + 31);
    if (active) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {                 // dp starts at -delta[q]
        const f32x4 dl = *(__attribute__((address_space(3))) f32x4*)(lds_ptr(sa) + 256 + 8 * jj * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) dp[4 * jj + e] = -dl[e];
      }
      // S = Q K_w^T over D: the next tile's DMA pieces in the shadows of its first MFMAs
      vd_gemm<T, kNK, 1>(
          [&](int kk) { return lds_read128<T>(lds_ptr(aq ^ ((kk & 7) << 5)) + (kk >> 3) * kVdQChunk); },
          [&](int kk, vec8<T> a) { s = mfma(a, kwr[kk], s); },
          [&](int i) {
            if (i < kPieces) issue_piece(nxt, i);
          });
      // dP - delta = dO V_w^T over Dv: both operands from LDS, read kAhead MFMAs ahead
      {
        constexpr int kAhead = kVdAhead < kNKv ? kVdAhead : kNKv;
        vec8<T> a[kNKv], w[kNKv];
        auto fa = [&](int kk) { return lds_read128<T>(lds_ptr(ado ^ (kk << 5))); };
        auto fw = [&](int kk) { return lds_read128<T>(lds_ptr(av ^ (kk << 5))); };
#pragma unroll
        for (int i = 0; i < kAhead; ++i) { a[i] = fa(i); w[i] = fw(i); }
#pragma unroll
        for (int i = 0; i < kNKv; ++i) {
          if (i + kAhead < kNKv) { a[i + kAhead] = fa(i + kAhead); w[i + kAhead] = fw(i + kAhead); }
          dp = mfma(a[i], w[i], dp);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * kAhead, 0);
#pragma unroll
        for (int i = 0; i < kNKv - kAhead; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, kAhead, 0);
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const f32x4 ls = *(__attribute__((address_space(3))) f32x4*)(lds_ptr(sa) + 8 * jj * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[4 * jj + e] = fast_exp2(__builtin_fmaf(s[4 * jj + e], c, -kLog2e * ls[e]));
      }
      const bool need_mask = (qs0 + 32 > lq) || (hi && qs0 + off + wr < kw0 + 31) || (lo && qs0 + 31 + off - wl > kw0);
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // (bitwise, not short-circuit: with && / || hipcc builds a branch per element)
          const int q = qs0 + crow(r, g);
          const bool ok = (q < lq) & (!hi | (krow <= q + off + wr)) & (!lo | (krow >= q + off - wl));
          s[r] = ok ? s[r] : 0.f;
        }
      }
      // pbv = P for the dV GEMM; s becomes dS = P (dP - delta) for the dK GEMM
      const vec8<T> pbv[2] = {pack8<T>(s, 0), pack8<T>(s, 8)};
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] *= dp[r];
      const vec8<T> pbk[2] = {pack8<T>(s, 0), pack8<T>(s, 8)};
      if (spill) {
        const char* blk = ds_b + (int64_t)(h0 + cg) * ds_head_bytes + (ds_rowpart(p, j, (qs.row0 >> 5) + b, ds_nkb) + ds_kb) * kDsBlockBytes;
        const buf_rsrc_t rb = make_rsrc(blk, kDsBlockBytes);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pbk[0]), rb, ds_lane, 0, 2);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pbk[1]), rb, ds_lane + 128, 0, 2);
      }
      // dV^T += dO^T P over Dv, dK^T += Q^T dS over D: A operands by transpose reads of the dO / Q tile
      vd_gemm<T, 2 * kNBv, 2>(
          [&](int i) {
            const int dblk = i % kNBv, imm = 16 * (i / kNBv) * 256;
            return concat<T>(lds_read_tr<T>(lds_ptr(tdo[0] ^ (dblk << 6)) + imm), lds_read_tr<T>(lds_ptr(tdo[1] ^ (dblk << 6)) + imm));
          },
          [&](int i, vec8<T> a) { accv[i % kNBv] = mfma(a, pbv[i / kNBv], accv[i % kNBv]); });
      vd_gemm<T, 2 * kNB, 2>(
          [&](int i) {
            const int dblk = i % kNB, imm = 16 * (i / kNB) * 256 + (dblk >> 2) * kVdQChunk;
            return concat<T>(lds_read_tr<T>(lds_ptr(tq[0] ^ ((dblk & 3) << 6)) + imm), lds_read_tr<T>(lds_ptr(tq[1] ^ ((dblk & 3) << 6)) + imm));
          },
          [&](int i, vec8<T> a) { acck[i % kNB] = mfma(a, pbk[i / kNB], acck[i % kNB]); });
    } else {
#pragma unroll
      for (int i = 0; i < kPieces; ++i) issue_piece(nxt, i);
    }
    // tile f + 1 must have landed; this tile's two dS stores (the youngest operations) may stay in flight
    if (spill && active) wait_vmem<2>();
    else wait_all_vmem();
    if (++cg >= G) {
      cg = 0;
      j -= nsplit;
    }
    __syncthreads();
  }
  wait_all_vmem();

  if (krow >= lk) return;
  const int64_t orow = ks.row0 + krow;
  {                                                    // dK: D wide, scaled
    const int64_t eoff = kbatch * p.dk_st.batch + orow * p.dk_st.row + (int64_t)hk * p.dk_st.head + (int64_t)qsplit * p.kv_split_stride;
    if (p.kv_f32) {
      vd_rows_f32<kNB>((float*)p.dk + eoff, g, p.D, [&](f32x4* dst, int dblk, int r0) {
        f32x4 x;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = acck[dblk][r0 + e] * p.scale;
        *dst = x;
      });
    } else {
      store_rows16<T, false, kNB>((T*)p.dk + eoff, acck, p.scale, g, p.D, true);
    }
  }
  {                                                    // dV: Dv wide
    const int64_t eoff = kbatch * p.dv_st.batch + orow * p.dv_st.row + (int64_t)hk * p.dv_st.head + (int64_t)qsplit * p.kv_split_stride;
    if (p.kv_f32) {
      vd_rows_f32<kNBv>((float*)p.dv + eoff, g, Dv, [&](f32x4* dst, int dblk, int r0) {
        f32x4 x;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = accv[dblk][r0 + e];
        *dst = x;
      });
    } else {
      store_rows16<T, false, kNBv>((T*)p.dv + eoff, accv, 1.f, g, Dv, true);
    }
  }
}

// ------------------------------------------------------------------------------------
static inline int vd_len(int S, int half) { return half ? (S + 1) / 2 : S; }

template <typename K, typename P>
static int launch_vd(K kernel, const P& p, int64_t nblocks, int smem, std::atomic<unsigned long long>& done, hipStream_t stream) {
  if (int rc = opt_in_dynamic_lds((const void*)kernel, smem, done)) return rc;
  if (nblocks <= 0) return kLaunchOk;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(kVdThreads), smem, stream, p);
  return hipGetLastError() == hipSuccess ? kLaunchOk : kLaunchFailed;
}

int launch_fwd_vd(const FwdParams& p0, int Dv, int dtype, hipStream_t stream) {
  static std::atomic<unsigned long long> done[2];
  FwdParamsVd p{p0, Dv};
  p.base.nqblk = (vd_len(p0.Sq, p0.q_half) + kVdRows - 1) / kVdRows;
  const int64_t n = (int64_t)p.base.nqblk * p0.H * p0.B;
  return dtype == 0 ? launch_vd(vd_fwd_kernel<bf16_t>, p, n, kVdFwdSmem, done[0], stream)
                    : launch_vd(vd_fwd_kernel<f16_t>, p, n, kVdFwdSmem, done[1], stream);
}

int launch_bwd_dq_vd(const BwdParams& p0, int Dv, int dtype, hipStream_t stream) {
  static std::atomic<unsigned long long> done[2];
  BwdParamsVd p{p0, Dv};
  p.base.nqblk = (vd_len(p0.Sq, p0.q_half) + kVdRows - 1) / kVdRows;
  const int64_t n = (int64_t)p.base.nqblk * p0.H * p0.B;
  return dtype == 0 ? launch_vd(vd_dq_kernel<bf16_t>, p, n, kVdFwdSmem, done[0], stream)
                    : launch_vd(vd_dq_kernel<f16_t>, p, n, kVdFwdSmem, done[1], stream);
}

int launch_bwd_dkdv_vd(const BwdParams& p0, int Dv, int dtype, hipStream_t stream) {
  static std::atomic<unsigned long long> done[2];
  BwdParamsVd p{p0, Dv};
  p.base.nkblk = (vd_len(p0.Sk, p0.k_half) + kVdRows - 1) / kVdRows;
  if (p.base.nsplit < 1) p.base.nsplit = 1;
  const int64_t n = (int64_t)p.base.nkblk * p0.Hk * p0.B * p.base.nsplit;
  return dtype == 0 ? launch_vd(vd_dkdv_kernel<bf16_t>, p, n, kVdKvSmem, done[0], stream)
                    : launch_vd(vd_dkdv_kernel<f16_t>, p, n, kVdKvSmem, done[1], stream);
}

}  // namespace rfa
