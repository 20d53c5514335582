// rfa_api.cpp — the C ABI of librfa_hip.so (see include/rfa.h for the contract and for the
// reference call sites each entry point replaces).  Pure argument checking + parameter
// translation; no allocation, no synchronisation, launches only on the caller's stream.
#include "../../include/rfa.h"
#include "rfa_kernels.hpp"

#include <algorithm>
#include <cfloat>
#include <atomic>
#include <vector>

using namespace rfa;

namespace {

inline Strides cv(const rfa_strides& s) { return Strides{s.batch, s.row, s.head}; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// element strides must keep every row start 16-byte aligned
inline bool stride_ok(const rfa_strides& s, int elt_bytes) {
  const int64_t q = 16 / elt_bytes;
  return (s.row % q) == 0 && (s.head % q) == 0 && (s.batch % q) == 0;
}

// ... and a row stride must leave the kernels' 32-bit descriptor arithmetic room (rfa_kernels.hpp: kDescMaxRows; rfa.h)
inline bool row_ok(const rfa_strides& s, int D, int elt_bytes) { return desc_row_stride_ok(s.row, D, elt_bytes); }
// B / H where a launcher makes them grid.y / grid.z, and a 1-D grid's block count (rfa_kernels.hpp)
inline bool grid_yz_ok(int64_t n) { return n <= kGridYZMax; }
inline bool grid_x_ok(int64_t nblocks) { return nblocks <= kGridXMax; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t mul_sat(int64_t a, int64_t b) {                     // a, b >= 0: the product, INT64_MAX where it does not fit
  return (a <= 0 || b <= 0) ? 0 : (a > INT64_MAX / b ? INT64_MAX : a * b);
}
inline int64_t mul_sat(int64_t a, int64_t b, int64_t c, int64_t d = 1) { return mul_sat(mul_sat(a, b), mul_sat(c, d)); }

// the side kernels' grids: B is grid.y, 16 (row, head) pairs per workgroup along grid.x
inline bool aux_extents_ok(int B, int S, int H) {
  return grid_yz_ok(B) && grid_x_ok(ceil_div(mul_sat(S, H), 16));
}

inline int check_common(int dtype, int H, int Hk, int D, int B) {
  if (dtype != RFA_BF16 && dtype != RFA_F16) return RFA_ERR_DTYPE;
  if (D <= 0 || D > kMaxHeadDim || (D % 8) != 0) return RFA_ERR_HEAD_DIM;
  if (H <= 0 || Hk <= 0 || (H % Hk) != 0) return RFA_ERR_HEADS;
  if (B < 0) return RFA_ERR_SHAPE;
  return RFA_OK;
}

inline int launch_status(int rc) {
  return rc == kLaunchOk ? RFA_OK : (rc == kLaunchAttrFailed ? RFA_ERR_ATTR : RFA_ERR_LAUNCH);
}

inline int eff_len(int S, int half) { return half == RFA_HALF_FULL ? S : (S + 1) / 2; }

// dropout_p -> keep threshold in 1/256 (256 = nothing dropped) — csrc/rfa_common.hpp: drop_keep
inline unsigned drop_threshold(float p) {
  if (!(p > 0.f)) return 256u;
  const int k = (int)((1.f - p) * 256.f + 0.5f);
  return (unsigned)(k < 0 ? 0 : (k > 255 ? 255 : k));      // p > 0 always drops something
}
// kept probabilities are rescaled by the reciprocal of the probability the mask REALLY keeps with (keep / 256, the
// quantised threshold above), not by 1 / (1 - p): E[dropout(P)] = P for every p (oracle/flash_attn_ref.py: drop_rescale)
inline float drop_rescale(float p) {
  const unsigned k = drop_threshold(p);
  return k >= 256u ? 1.f : (k == 0u ? 0.f : 256.f / (float)k);
}
// ---- band normalisation (dense input) ------------------------------------------------------------------------------
// A call's band is  i + off - wl <= j <= i + off + wr  with off = len_k - len_q + mask_shift (rfa.h).  Before anything is
// planned or launched it is brought to a canonical form, so that blocks of a sharded sequence that differ only in how far
// they lie from the diagonal run what an equivalent unsharded call would:
//   * a left bound no row can reach (row len_q - 1 already starts at key <= 0) and a right bound row 0 already clears
//     (off + wr >= len_k - 1) are dropped — a block wholly inside the window IS the unwindowed non-causal call: same
//     instance, same plan, same dS-spill form, bit for bit;
//   * a block no element of which is visible is flagged `empty` and given ONE canonical band (nothing visible, small
//     numbers) for the callers that still have to write zeros;
//   * what is left is re-expressed with small numbers where the caller's are large (the kernels keep off, off - wl and
//     off + wr in 32 bits): only the two edges off - wl and off + wr matter, and for a non-empty block with live bounds both
//     lie inside (-len_q, len_k).
// Packed (cu_seqlens) input is not normalised — the lengths live on the device — and takes no absolute shift (RFA_ERR_ARGS);
// its shift is mask_shift_lens, in units of each sequence's own key length, applied by the kernels.  Dense input folds
// mask_shift_lens * len_k into mask_shift first (fold_lens), so a dense call with mask_shift_lens = n IS the call with
// mask_shift = n * len_k.
struct Band { int causal, window, wl, wr; int64_t shift; bool empty; };
inline int dense_len(int S, int half) { return half == RFA_HALF_FULL ? S : (half == RFA_HALF_FRONT ? S / 2 : S - S / 2); }
inline Band norm_band(int Sq, int q_half, int Sk, int k_half, int causal, int window, int wl_in, int wr_in, int64_t shift) {
  Band b{causal ? 1 : 0, window ? 1 : 0, wl_in, wr_in, 0, false};
  int64_t wl = (window && wl_in >= 0) ? wl_in : -1;
  int64_t wr = causal ? 0 : ((window && wr_in >= 0) ? wr_in : -1);
  if (wl < 0 && wr < 0) return Band{0, 0, -1, -1, 0, false};          // no band: the shift is ignored
  const int64_t lq = dense_len(Sq, q_half), lk = dense_len(Sk, k_half);
  if (lq <= 0 || lk <= 0) { b.shift = 0; return b; }                  // (nothing to compute: the callers' own early returns)
  const int64_t off = lk - lq + shift;
  bool changed = false;
  if (wl >= 0 && lq - 1 + off - wl <= 0) { wl = -1; changed = true; }
  if (wr >= 0 && off + wr >= lk - 1) { wr = -1; changed = true; }
  if ((wr >= 0 && lq - 1 + off + wr < 0) || (wl >= 0 && off - wl > lk - 1))
    return Band{0, 1, -1, 0, -lk, true};                              // off' = -len_q, wr = 0: row i would see keys <= i - len_q
  if (wl < 0 && wr < 0) return Band{0, 0, -1, -1, 0, false};
  const int64_t big = (int64_t)1 << 28;
  int64_t s = shift;
  if (off > big || off < -big || wl > big || wr > big) {
    // same two edges, small numbers: anchored at the live right edge (wr = 0, so a causal call stays one), else at the left
    const int64_t lo_e = off - wl, hi_e = off + wr;
    if (wr >= 0) { s = hi_e - (lk - lq); if (wl >= 0) wl = hi_e - lo_e; wr = 0; }
    else { s = lo_e - (lk - lq); wl = 0; }
    changed = true;
  }
  if (!changed) { b.shift = shift; return b; }                        // (the caller's own fields, untouched)
  const int c = (causal && wr >= 0) ? 1 : 0;                          // (causal: wr was 0 and the bound is still live)
  return Band{c, (wl >= 0 || (wr >= 0 && !c)) ? 1 : 0, (int)wl, (int)wr, s, false};
}
template <typename A>
inline bool has_band(const A& a) {
  return a.causal || (a.window && (a.window_left >= 0 || a.window_right >= 0));
}
// mask_shift_lens made canonical: dense input folds it into mask_shift; a call without a band ignores it (as mask_shift)
template <typename A>
inline A fold_lens(const A& a) {
  A n = a;
  if (a.mask_shift_lens == 0) return n;
  if (a.cu_seqlens_q == nullptr && a.cu_seqlens_k == nullptr) {
    n.mask_shift = a.mask_shift + (int64_t)a.mask_shift_lens * dense_len(a.Sk, a.k_half);
    n.mask_shift_lens = 0;
  } else if (!has_band(a)) {
    n.mask_shift_lens = 0;
  }
  return n;
}
// the call with its band normalised (what every plan / size / launch below looks at)
template <typename A>
inline A norm_args(const A& a0) {
  const A a = fold_lens(a0);
  A n = a;
  if (a.cu_seqlens_q != nullptr || a.cu_seqlens_k != nullptr || a.dropout_p > 0.f) return n;   // (dropout: no window, no shift)
  const Band b = norm_band(a.Sq, a.q_half, a.Sk, a.k_half, a.causal, a.window, a.window_left, a.window_right, a.mask_shift);
  n.causal = b.causal; n.window = b.window; n.window_left = b.wl; n.window_right = b.wr; n.mask_shift = b.shift;
  return n;
}
template <typename A>
inline bool band_empty(const A& a0) {
  if (a0.cu_seqlens_q != nullptr || a0.cu_seqlens_k != nullptr || a0.dropout_p > 0.f) return false;
  const A a = fold_lens(a0);
  return norm_band(a.Sq, a.q_half, a.Sk, a.k_half, a.causal, a.window, a.window_left, a.window_right, a.mask_shift).empty;
}
// an absolute shift needs dense input, either shift no dropout (the keep mask has position offsets of its own); the
// per-sequence shift must leave the kernels' 32-bit off, off - wl, off + wr room: |mask_shift_lens| * Sk < 2^30
template <typename A>
inline bool shift_args_ok(const A& a) {
  if (a.mask_shift_lens != 0) {
    if (a.dropout_p > 0.f) return false;
    const int64_t n = a.mask_shift_lens < 0 ? -(int64_t)a.mask_shift_lens : (int64_t)a.mask_shift_lens;
    if (n * (int64_t)(a.Sk > 0 ? a.Sk : 0) >= ((int64_t)1 << 30)) return false;
  }
  if (a.mask_shift == 0) return true;
  return a.cu_seqlens_q == nullptr && a.cu_seqlens_k == nullptr && !(a.dropout_p > 0.f);
}
// the shift the plans reason with: the normalised mask_shift of dense input; packed input — whose lengths live on the
// device — stands in mask_shift_lens * Sk (the longest sequence's shift)
template <typename A>
inline int64_t plan_shift(const A* a) { return a->mask_shift + (int64_t)a->mask_shift_lens * a->Sk; }

inline bool drop_args_ok(float p, int window, int wl, int wr, int causal) {
  if (!(p >= 0.f) || p >= 1.f) return false;
  const bool win = window && (wl >= 0 || (wr >= 0 && !causal));
  return !(p > 0.f && win);
}

// dropout position map (rfa.h: q_pos_stride ...): a non-default map needs dense, unhalved input and a split inside the tensor
inline bool pos_map_default(int stride, int split) { return (stride == 0 || stride == 1) && split == 0; }
template <typename A>
inline bool pos_map_ok(const A& a) {
  if (!(a.dropout_p > 0.f)) return true;                       // the fields are read with dropout only
  if (a.q_pos_stride < 0 || a.k_pos_stride < 0) return false;
  const bool qd = pos_map_default(a.q_pos_stride, a.q_pos_split), kd = pos_map_default(a.k_pos_stride, a.k_pos_split);
  if (qd && kd) return true;
  if (a.cu_seqlens_q != nullptr || a.cu_seqlens_k != nullptr) return false;
  if (a.q_half != RFA_HALF_FULL || a.k_half != RFA_HALF_FULL) return false;
  if (a.q_pos_split != 0 && (a.q_pos_split < 1 || a.q_pos_split > a.Sq - 1)) return false;
  if (a.k_pos_split != 0 && (a.k_pos_split < 1 || a.k_pos_split > a.Sk - 1)) return false;
  return true;
}
// kernel parameters of the map: strides normalised to >= 1, drop_mapped = "not the identity" (the kernels' run-time branch)
template <typename P, typename A>
inline void set_pos_map(P& p, const A& a) {
  p.q_pos0 = (unsigned)a.q_pos_offset; p.k_pos0 = (unsigned)a.k_pos_offset; p.head0 = (unsigned)a.head_offset;
  p.q_pstride = 1u; p.k_pstride = 1u;
  if (!(a.dropout_p > 0.f)) return;
  p.q_pstride = a.q_pos_stride > 0 ? (unsigned)a.q_pos_stride : 1u;
  p.k_pstride = a.k_pos_stride > 0 ? (unsigned)a.k_pos_stride : 1u;
  p.q_psplit = a.q_pos_split; p.k_psplit = a.k_pos_split;
  p.q_pos2 = (unsigned)a.q_pos_offset2; p.k_pos2 = (unsigned)a.k_pos_offset2;
  p.drop_mapped = (p.q_pstride != 1u || p.k_pstride != 1u || p.q_psplit != 0 || p.k_psplit != 0) ? 1 : 0;
}


// ---- extension arguments (rfa.h: rfa_ext_args) -----------------------------------------------------------------------------
// The caller's struct may be shorter (an older caller: the missing tail reads as zero) or longer (a newer one: accepted while
// the tail this library does not know is zero) than ours.  Parsed before any pointer of the base struct is looked at.
struct Ext { const float* slopes; int64_t bstride, shift; float cap; };   // ALiBi (slopes = nullptr: off) and the soft cap (0: off), independent
constexpr uint32_t kExtHead = 2 * sizeof(uint32_t);              // struct_bytes + reserved
inline int parse_ext(const rfa_ext_args* e, Ext* out) {
  *out = Ext{nullptr, 0, 0, 0.f};
  if (e == nullptr) return RFA_OK;
  const uint32_t n = e->struct_bytes;
  if (n < kExtHead || e->reserved != 0) return RFA_ERR_ARGS;
  rfa_ext_args x{};
  const unsigned char* src = reinterpret_cast<const unsigned char*>(e);
  unsigned char* dst = reinterpret_cast<unsigned char*>(&x);
  for (uint32_t i = 0; i < n && i < sizeof(x); ++i) dst[i] = src[i];
  for (uint32_t i = sizeof(x); i < n; ++i)
    if (src[i] != 0) return RFA_ERR_ARGS;
  if (!(x.softcap >= 0.f) || !(x.softcap <= FLT_MAX) || x.softcap_pad != 0) return RFA_ERR_ARGS;   // negative, NaN, infinite
  out->cap = x.softcap;
  if (x.alibi_slopes == nullptr) return RFA_OK;                  // bias off: the shift and the stride are not read
  if (x.alibi_batch_stride < 0) return RFA_ERR_ARGS;
  out->slopes = x.alibi_slopes; out->bstride = x.alibi_batch_stride; out->shift = x.alibi_shift;
  return RFA_OK;
}
// what a call with a bias must look like (rfa.h), checked on the call as given and on its normalised band `n`
template <typename A>
inline bool bias_args_ok(const A& a, const A& n, const Ext& e) {
  if (a.dropout_p > 0.f || a.D > kHeadDim || !(a.softmax_scale > 0.f)) return false;
  if (n.window && (n.window_left >= 0 || (n.window_right >= 0 && !n.causal))) return false;   // a bound that survived
  if (e.shift != 0 && (a.cu_seqlens_q != nullptr || a.cu_seqlens_k != nullptr)) return false;
  if (e.shift <= -((int64_t)1 << 31) || e.shift >= ((int64_t)1 << 31)) return false;
  return (e.shift < 0 ? -e.shift : e.shift) + a.Sq + a.Sk < ((int64_t)1 << 31);
}
// what a call with a soft cap must look like (rfa.h); `n`: its normalised band.  A bounded window at head dims 65 .. 127
// would need the zero-padded 128-wide windowed dK/dV instance with a cap, which is not built (rfa_bwd.hip: launch_dkdv_cap)
// — refused in the forward too, so that no forward runs whose backward cannot
template <typename A>
inline bool cap_args_ok(const A& a, const A& n, const Ext& e) {
  if (a.dropout_p > 0.f || e.slopes != nullptr || a.D > kHeadDim || !(a.softmax_scale > 0.f)) return false;
  const bool win = n.window && (n.window_left >= 0 || (n.window_right >= 0 && !n.causal));
  return kCapPaddedWin || !(win && a.D > 64 && a.D < kHeadDim);
}
// the kernels' two constants, made once here (rfa_kernels.hpp)
template <typename P>
inline void set_cap(P& p, const Ext& e, float scale) {
  p.cap = e.cap; p.cap_in = 2.f * kLog2e * scale / e.cap; p.cap_c = e.cap * kLog2e;
}
template <typename P>
inline void set_bias(P& p, const Ext& e, float scale) {
  p.alibi = e.slopes; p.alibi_bstride = e.bstride; p.alibi_shift = (int)e.shift; p.alibi_rscale = 1.f / scale;
}

}  // namespace

// the library is built with -fvisibility=hidden: the C ABI below (include/rfa.h) is everything a loader can bind —
// no rfa::launch_* internals, no kernel stubs (tests/test_abi.py::test_library_exports_only_the_c_abi)
#pragma GCC visibility push(default)
extern "C" {

int rfa_abi_version(void) { return RFA_ABI_VERSION; }
int rfa_abi_revision(void) { return RFA_ABI_REVISION; }

#ifndef RFA_BUILD_ID
#define RFA_BUILD_ID "unstamped"
#endif
const char* rfa_build_id(void) { return RFA_BUILD_ID; }

const char* rfa_strerror(int status) {
  switch (status) {
    case RFA_OK: return "ok";
    case RFA_ERR_NULL: return "a required pointer is NULL";
    case RFA_ERR_DTYPE: return "unsupported dtype (only bf16 / fp16)";
    case RFA_ERR_HEAD_DIM: return "head_dim must be a multiple of 8 and <= 256";
    case RFA_ERR_HEADS: return "nheads must be a positive multiple of nheads_k";
    case RFA_ERR_SHAPE: return "negative or inconsistent extent";
    case RFA_ERR_ALIGN: return "pointer/stride violates the 16-byte alignment contract";
    case RFA_ERR_LAUNCH: return "HIP kernel launch failed";
    case RFA_ERR_ARGS: return "inconsistent flag / pointer combination (or dropout together with a window, dropout_p outside [0, 1))";
    case RFA_ERR_ATTR: return "could not opt the kernel into its dynamic LDS size on this device";
    default: return "unknown rfa status";
  }
}

// ---- launch plans (round 6: a cost estimate instead of shape thresholds) ------------------------------------------------
// Rounds 2-5 chose the forward form and the dK/dV plan with constants found on a handful of shapes (`wgs8 >= 112 &&
// wgs8 <= 192 && tiles >= 128`, `wgs128 * (ns + 1) <= 640`, `sq / (ns + 1) >= 2048`, ...).  tools/plan_sweep.py, which times
// the chosen form against every form that can be forced on BOTH sides of those boundaries, found the cliffs the round-5
// review predicted: forward launches of 96 / 160 / 192 / 224 workgroups against long key chains 8 - 26 % behind the best
// form, and backward launches with 1 - 4 K/V heads (a llama3 head group, any GQA model with few K/V heads) up to 1.9 x
// behind (profiles/r06_plan_sweep_before.md).  Both plans now come from ONE estimate of a launch's makespan:
//     workgroups are jobs of `tiles + kPlanWgOverhead` tile-times (prologue, epilogue, fill / drain), dealt heaviest
//     first (the kernels' blockIdx order) to the chip's 256 workgroup slots (one 8-wave workgroup per CU);
//     makespan x (1 + 0.4 busy^2): the tile time grows with the fraction of the chip that is busy (the board clocks to
//     its power cap: 1.33 us per forward tile with 96 CUs busy, 1.85 with 256 — profiles/r06_power_limiters.md);
//     + kPlanSecondPass tile-times when the shares' partials need a second kernel (combine / reduce).
// The plan is the candidate with the smallest estimate (ties: fewer shares).  A pure function of the call's shapes; the
// result is memoised per shape (a 256-entry table of atomics: no lock, no allocation).
// Fitted on / checked against tools/plan_sweep.py --dump (63 shapes x every forced form): worst chosen / best 1.06 where
// the old rules reached 1.26 (forward) and 1.90 (backward); tests/test_gpu_plan_rules.py keeps it that way.
namespace {

constexpr int kPlanSlots = 256;            // CUs: one 8-wave workgroup each (LDS and registers allow no second one)
constexpr double kPlanBusyGain = 0.4;

// makespan of `n` jobs (sizes[i] tile-times each + ovh), heaviest first, on kPlanSlots equal machines; *work = sum of all
double plan_makespan(std::vector<int>& sizes, double ovh, double* work) {
  std::sort(sizes.begin(), sizes.end(), [](int x, int y) { return x > y; });
  double total = 0;
  for (int v : sizes) total += v + ovh;
  *work = total;
  if (sizes.empty()) return 0;
  if ((int)sizes.size() <= kPlanSlots) return sizes[0] + ovh;
  // min-heap of machine loads
  std::vector<double> load(kPlanSlots, 0.0);
  auto cmp = [](double x, double y) { return x > y; };
  for (int v : sizes) {
    std::pop_heap(load.begin(), load.end(), cmp);
    load.back() += v + ovh;
    std::push_heap(load.begin(), load.end(), cmp);
  }
  double mk = 0;
  for (double l : load) mk = l > mk ? l : mk;
  return mk;
}
double plan_cost(std::vector<int>& sizes, double ovh, double second_pass) {
  double work = 0;
  const double mk = plan_makespan(sizes, ovh, &work);
  if (mk <= 0) return 0;
  double busy = work / (mk * kPlanSlots);
  busy = busy > 1 ? 1 : busy;
  return mk * (1 + kPlanBusyGain * busy * busy) + second_pass;
}

// memo: (56-bit hash of the shape key) << 8 | plan code; 0 = empty
std::atomic<uint64_t> g_plan_memo[256];
inline uint64_t plan_hash(const int64_t* k, int n) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < n; ++i) {
    h ^= (uint64_t)k[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
  }
  h &= 0x00FFFFFFFFFFFFFFull;
  return h ? h : 1;
}
inline bool plan_lookup(uint64_t h, int* code) {
  const uint64_t w = g_plan_memo[h & 255].load(std::memory_order_relaxed);
  if ((w >> 8) != h) return false;
  *code = (int)(w & 255);
  return true;
}
inline void plan_store(uint64_t h, int code) { g_plan_memo[h & 255].store((h << 8) | (uint64_t)(code & 255), std::memory_order_relaxed); }

}  // namespace

// Forward plan: query rows per workgroup (256 = 8 waves, 128 = 4 waves, two workgroups per CU) and split-KV shares.
//   * many workgroups (>= 384 of 256 rows: 1.5 rounds of the chip and more): no shares; 128-row workgroups for sequences
//     <= 1024 (+6 % at 1024, +13 % at 512, -2 % from 2048 on: round 4)
//   * sequences <= 1024 otherwise: the 128-row form, shares by the round-4 rule (fill 512 slots + 25 %, >= 32 tiles each)
//   * very few workgroups (<= 48 of 256 rows: one or two llama3 head groups) against >= 64 key tiles: the 128-row form,
//     shares until 256 workgroups exist (>= 16 tiles each) — a lone 4-wave workgroup walks its tiles 1.4 x faster than an
//     8-wave one does twice the rows (0.96 vs 1.33 us per tile), and there are CUs to spare
//   * fewer than 64 key tiles, or 257 .. 383 workgroups of 256 rows: the 128-row form, no shares (round 4's rules, confirmed
//     by the round-6 sweep)
//   * everything between: the 256-row form with the share count of the smallest estimated makespan
struct FwdPlan { int rows, ns, persist; };
// compute units of the current device (the persistent forward's grid; 256 when no device can be asked: plan queries on a host)
static int device_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return kPlanSlots;
  }
  int v = cached[dev & 63].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = kPlanSlots;
  }
  cached[dev & 63].store(n, std::memory_order_relaxed);
  return n;
}
// the persistent 256-row forward (rfa_fwd.hip: fwd_persist_kernel): what a call must look like
static bool fwd_persist_eligible(const rfa_fwd_args* a) {
  if (a->D != kHeadDim || a->cu_seqlens_q != nullptr || a->out_acc != nullptr || a->dropout_p > 0.f) return false;
  if (a->window && (a->window_left >= 0 || (a->window_right >= 0 && !a->causal))) return false;
  if (a->B <= 0 || a->Sq <= 0 || a->Sk <= 0) return false;
  if (plan_shift(a) != 0) return false;                      // (its item deal and 'off >= 0' assume the block's own diagonal)
  return eff_len(a->Sk, a->k_half) >= eff_len(a->Sq, a->q_half);
}
static FwdPlan fwd_plan_base(const rfa_fwd_args* a);
// Measured (profiles/r06_persistent_forward.md; bit-identical to the 8 x 32 form everywhere): at the headline the seam
// overlap buys nothing (0.4926 against 0.4905 ms: the dispatcher's own overlap of a finishing and a starting workgroup is as
// good), from 16384 rows on the static deal loses 1 %; sequences of 1024 .. 2048 rows in launches of >= 2 items per CU gain
// 1 - 4 % over the best other form (B 8 x S 1024: 0.0861 against 0.0898 for the 128-row form and 0.0941 for the 256-row one).
static FwdPlan fwd_plan(const rfa_fwd_args* a) {
  FwdPlan pl = fwd_plan_base(a);
  pl.persist = 0;
  if (!fwd_persist_eligible(a) || a->kv_nsplit > 1) return pl;
  const int sq = eff_len(a->Sq, a->q_half);
  const int64_t items = (int64_t)a->B * a->H * ((sq + 255) / 256);
  const bool by_name = a->fwd_form == RFA_FWD_P8x32;
  bool by_rule = a->fwd_form == RFA_FWD_AUTO && pl.ns == 1 && items >= 2 * (int64_t)kPlanSlots && sq >= 1024 && sq <= 2048;
  if (by_rule) {
    // the static deal must balance: the tiles every workgroup gets from its passes (every other pass reversed, as
    // fwd_persist_kernel deals them) within 4 % of the mean — whole pairs of passes over a causal launch do exactly; a
    // partial last pass does not (S 1280 x B 6: 3.75 passes, measured 27 % behind the 256-row form)
    const int sk = eff_len(a->Sk, a->k_half), off = sk - sq, nq = (sq + 255) / 256, grid = device_cus();
    std::vector<int64_t> load((size_t)grid, 0);
    int64_t total = 0;
    for (int64_t idx = 0; idx < items; ++idx) {
      const int64_t pass = idx / grid, r = idx % grid;
      const int64_t w = (pass & 1) ? grid - 1 - r : r;
      const int64_t blk = idx / ((int64_t)a->H);               // (kv head, query head in group) are the fastest digits
      const int qblk = nq - 1 - (int)(blk % nq);                // (batch slowest: RFA_BATCH_FAST_Q = 0)
      const int qend = (qblk + 1) * 256 < sq ? (qblk + 1) * 256 : sq;
      int kmax = sk;
      if (a->causal && qend + off < kmax) kmax = qend + off;
      const int nt = (kmax + 63) / 64 + 8;                     // + the estimate's per-item overhead
      load[(size_t)w] += nt;
      total += nt;
    }
    int64_t mx = 0;
    for (int64_t l : load) mx = l > mx ? l : mx;
    by_rule = mx * grid <= total + total / 25;
  }
  if (by_name || by_rule) {
    pl.rows = 256;
    pl.ns = 1;
    pl.persist = 1;
  }
  return pl;
}
static FwdPlan fwd_plan_base(const rfa_fwd_args* a) {
  FwdPlan pl{fwd_qrows_per_block(), 1, 0};
  const bool win = a->window && (a->window_left >= 0 || (a->window_right >= 0 && !a->causal));
  if ((a->D != kHeadDim && a->D != kHeadDim / 2) || win || a->dropout_p > 0.f) return pl;   // one form, no shares
  if (a->B <= 0 || a->Sq <= 0 || a->Sk <= 0) return pl;
  const int sq = eff_len(a->Sq, a->q_half), sk = eff_len(a->Sk, a->k_half);
  const int64_t w8 = (int64_t)a->B * a->H * ((sq + 255) / 256), w128 = (int64_t)a->B * a->H * ((sq + 127) / 128);
  const int tiles = (sk + 63) / 64;
  const bool can_split = a->kv_nsplit != 1;
  // a form / share count asked for by name (tuning, tests) is taken as given
  if (a->fwd_form == RFA_FWD_8x32 || a->fwd_form == RFA_FWD_4x32 || a->kv_nsplit > 1) {
    pl.rows = a->fwd_form == RFA_FWD_4x32 ? 128 : 256;
    pl.ns = a->kv_nsplit > 1 ? (a->kv_nsplit > 8 ? 8 : a->kv_nsplit) : 1;
    if (a->fwd_form == RFA_FWD_AUTO) {                      // shares forced, form free: the form the rules below would take
      rfa_fwd_args b = *a;
      b.kv_nsplit = 0;
      pl.rows = fwd_plan_base(&b).rows;
    }
    return pl;
  }
  if (w8 >= 384) {
    pl.rows = sq <= 1024 ? 128 : 256;
    return pl;
  }
  if (sq <= 1024) {
    pl.rows = 128;
    if (can_split && w128 < 384 && tiles >= 64) {
      int ns = 1;
      while (ns < 8 && w128 * (ns + 1) <= 640 && tiles / (ns + 1) >= 32) ++ns;
      pl.ns = ns;
    }
    return pl;
  }
  if (w8 <= 48 && tiles >= 64) {
    pl.rows = 128;
    if (can_split) {
      int ns = (int)(256 / w128);
      ns = ns < 1 ? 1 : (ns > 8 ? 8 : ns);
      while (ns > 1 && tiles / ns < 16) --ns;
      pl.ns = ns;
    }
    return pl;
  }
  if (tiles < 64) {
    // short key chains on an under-filled chip (S 2048, 16 heads: 128 workgroups of <= 32 tiles): nothing to share — shares of
    // < 32 tiles do not pay for the combine pass — and the 128-row form's two workgroups per CU balance the causal triangle
    // (round 4's rule; round 6 re-measured: 0.0385 ms against 0.0455 with two shares of 256-row workgroups, 0.0493 with one)
    pl.rows = 128;
    return pl;
  }
  if (w8 > 256) {
    // 257 .. 383 workgroups of 256 rows: one round of the chip plus a short second one.  The 128-row form (two workgroups
    // per CU, a light one's partner speeds up when it leaves) balances that better than any share count of the 256-row
    // form: S 6144, 12 heads, causal 0.130 vs 0.144 ms (round 4's rule for this range, kept: profiles/r06_plan_sweep_after.md)
    pl.rows = 128;
    return pl;
  }
  pl.rows = 256;
  if (!can_split) return pl;
  const int64_t key[8] = {1, a->B, a->H, sq, sk, a->causal ? 1 : 0, a->causal ? plan_shift(a) : 0, 0};
  const uint64_t h = plan_hash(key, 8);
  int code;
  if (plan_lookup(h, &code)) {
    pl.ns = code;
    return pl;
  }
  // workgroups of the 256-row form: block i of every (batch, head) sees the key tiles below its causal edge
  const int off = sk - sq + (int)plan_shift(a), nq = (sq + 255) / 256;
  const int64_t mult = (int64_t)a->B * a->H;
  double best = -1;
  static const int cand[] = {1, 2, 3, 4, 6, 8};
  for (int ns : cand) {
    if (ns > 1 && tiles / ns < 16) continue;
    std::vector<int> sizes;
    sizes.reserve((size_t)(nq * ns * mult));
    for (int i = 0; i < nq; ++i) {
      const int qend = (i + 1) * 256 < sq ? (i + 1) * 256 : sq;
      int kmax = sk;
      if (a->causal && qend + off < kmax) kmax = qend + off;
      const int nt = kmax > 0 ? (kmax + 63) / 64 : 0;
      int chunk = (nt + ns - 1) / ns;
      chunk = (chunk + 1) / 2 * 2;                           // (shares are a multiple of the LDS ring depth long: fwd_kernel)
      for (int sidx = 0; sidx < ns; ++sidx) {
        const int lo = sidx * chunk, hi = lo + chunk < nt ? lo + chunk : nt;
        const int n = hi > lo ? hi - lo : 0;
        for (int64_t m = 0; m < mult; ++m) sizes.push_back(n);
      }
    }
    const double c = plan_cost(sizes, 8.0, ns > 1 ? 8.0 : 0.0);
    if (best < 0 || c < 0.98 * best) {
      best = c;
      pl.ns = ns;
    }
  }
  plan_store(h, pl.ns);
  return pl;
}
static int fwd_kv_nsplit(const rfa_fwd_args* a) { return fwd_plan(a).ns; }
static int64_t fwd_rows_total(const rfa_fwd_args* a) {
  if (a->cu_seqlens_q != nullptr) return a->total_q > 0 ? a->total_q : 0;
  return (int64_t)a->B * a->Sq;
}

int64_t rfa_fwd_workspace_bytes(const rfa_fwd_args* a, int32_t* nsplit) {
  if (nsplit) *nsplit = 1;
  if (!a || check_common(a->dtype, a->H, a->Hk, a->D, a->B) || !shift_args_ok(*a) || !pos_map_ok(*a)) return 0;
  const rfa_fwd_args na = norm_args(*a);
  a = &na;
  const int ns = fwd_kv_nsplit(a);
  const int64_t rows = fwd_rows_total(a);
  if (ns <= 1 || rows <= 0) return 0;
  if (nsplit) *nsplit = ns;
  return (int64_t)ns * rows * a->H * ((int64_t)a->D + 1) * 4;      // fp32 partial outs + partial lse
}

int64_t rfa_ext_args_bytes(void) { return (int64_t)sizeof(rfa_ext_args); }

int rfa_fwd(const rfa_fwd_args* a, void* stream) { return rfa_fwd_ex(a, nullptr, stream); }

// ---- a value head dim of its own (rfa.h: rfa_vdim_args; csrc/rfa_vdim.hip) ---------------------------------------------------
// Parsed before any pointer of the base struct is looked at; a longer struct is accepted while its unknown tail is zero.
inline int parse_vdim(const rfa_vdim_args* v, float dropout_p, int D, int* Dv) {
  if (v == nullptr || v->struct_bytes < sizeof(rfa_vdim_args) || v->reserved != 0 || v->pad != 0) return RFA_ERR_ARGS;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(v);
  for (uint32_t i = sizeof(rfa_vdim_args); i < v->struct_bytes; ++i)
    if (src[i] != 0) return RFA_ERR_ARGS;
  if (dropout_p > 0.f) return RFA_ERR_ARGS;
  if (v->head_dim_v < 8 || v->head_dim_v > kVdMaxHeadDimV || (v->head_dim_v & 7)) return RFA_ERR_HEAD_DIM;
  if (D < kVdMinHeadDim || D > kVdMaxHeadDim || (D & 7)) return RFA_ERR_HEAD_DIM;
  *Dv = v->head_dim_v;
  return RFA_OK;
}

// ---- per-row key ranges (rfa.h: rfa_rowrange_args; the kRng kernel instances) ----------------------------------------------
// Parsed, and the base arguments' combination checked, before any tensor pointer of the base struct is looked at; a longer
// struct is accepted while its unknown tail is zero.
inline int parse_rr(const rfa_rowrange_args* r, RowRangeParams* out) {
  if (r == nullptr || r->struct_bytes < sizeof(rfa_rowrange_args) || r->reserved != 0) return RFA_ERR_ARGS;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(r);
  for (uint32_t i = sizeof(rfa_rowrange_args); i < r->struct_bytes; ++i)
    if (src[i] != 0) return RFA_ERR_ARGS;
  *out = RowRangeParams{};
  out->start = r->start;
  out->end = r->end;
  out->bstride = r->batch_stride;
  out->k_pos0 = r->k_pos0;
  out->tile_bounds = (int2*)r->tile_bounds;
  return RFA_OK;
}
inline int rr_base_check(float dropout_p, const void* cu_q, const void* cu_k, int q_half, int k_half) {
  if (dropout_p > 0.f || cu_q != nullptr || cu_k != nullptr || q_half != 0 || k_half != 0) return RFA_ERR_ARGS;
  return RFA_OK;
}
inline int rr_dim_check(int D, const RowRangeParams& r) {
  if (D > kHeadDim || (!kRngPadded128 && D > 64 && D < kHeadDim)) return RFA_ERR_HEAD_DIM;
  if (r.bstride < 0) return RFA_ERR_ARGS;
  return RFA_OK;
}

// ---- block-sparse masks (rfa.h: rfa_blockmask_args; the kBlk kernel instances) ------------------------------------------------
// Parsed like the ranges: before any tensor pointer of the base struct is looked at; a longer struct while its tail is zero.
inline int parse_bm(const rfa_blockmask_args* m, BlockMaskParams* out) {
  if (m == nullptr || m->struct_bytes < sizeof(rfa_blockmask_args) || m->reserved != 0) return RFA_ERR_ARGS;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(m);
  for (uint32_t i = sizeof(rfa_blockmask_args); i < m->struct_bytes; ++i)
    if (src[i] != 0) return RFA_ERR_ARGS;
  *out = BlockMaskParams{};
  out->mask = m->mask;
  out->bstride = m->batch_stride;
  out->hstride = m->head_stride;
  out->rstride = m->row_stride;
  out->nk_blocks = (int)m->nk_blocks;
  out->k_blk0 = (int)m->k_blk0;
  return RFA_OK;
}
inline int bm_dim_check(int D, int H, int Hk, const rfa_blockmask_args* m) {
  if (D > kHeadDim) return RFA_ERR_HEAD_DIM;
  if (m->batch_stride < 0 || m->head_stride < 0 || m->row_stride < 0 || m->nk_blocks < 0 || m->nk_blocks > 0x7fffffff ||
      m->k_blk0 < -0x40000000ll || m->k_blk0 > 0x40000000ll)
    return RFA_ERR_ARGS;
  if (Hk > 0 && H > 0 && H / Hk > kBmMaxGroup) return RFA_ERR_ARGS;     // (the dK/dV item walk: rfa_blockmask.h)
  return RFA_OK;
}

// Dv = 0: one head dim (rfa_fwd, rfa_fwd_ex); else the V head dim of rfa_fwd_vd; rr: the row ranges of rfa_fwd_rr; bm: the
// block mask of rfa_fwd_bm
static int fwd_impl(const rfa_fwd_args* a, const rfa_ext_args* ext, int Dv, void* stream, const RowRangeParams* rr = nullptr,
                    const BlockMaskParams* bm = nullptr);
int rfa_fwd_ex(const rfa_fwd_args* a, const rfa_ext_args* ext, void* stream) { return fwd_impl(a, ext, 0, stream); }
int rfa_fwd_vd(const rfa_fwd_args* a, const rfa_vdim_args* vd, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int Dv = 0;
  if (int rc = parse_vdim(vd, a->dropout_p, a->D, &Dv)) return rc;
  return fwd_impl(a, nullptr, Dv, stream);
}
int rfa_fwd_rr(const rfa_fwd_args* a, const rfa_rowrange_args* rr, void* stream) {
  if (!a) return RFA_ERR_NULL;
  RowRangeParams r;
  if (int rc = parse_rr(rr, &r)) return rc;
  if (int rc = rr_base_check(a->dropout_p, a->cu_seqlens_q, a->cu_seqlens_k, a->q_half, a->k_half)) return rc;
  if (int rc = rr_dim_check(a->D, r)) return rc;
  return fwd_impl(a, nullptr, 0, stream, &r);
}

int rfa_fwd_bm(const rfa_fwd_args* a, const rfa_blockmask_args* bm, void* stream) {
  if (!a) return RFA_ERR_NULL;
  BlockMaskParams m;
  if (int rc = parse_bm(bm, &m)) return rc;
  if (int rc = rr_base_check(a->dropout_p, a->cu_seqlens_q, a->cu_seqlens_k, a->q_half, a->k_half)) return rc;
  if (int rc = bm_dim_check(a->D, a->H, a->Hk, bm)) return rc;
  return fwd_impl(a, nullptr, 0, stream, nullptr, &m);
}

static int fwd_impl(const rfa_fwd_args* a, const rfa_ext_args* ext, int Dv, void* stream, const RowRangeParams* rr,
                    const BlockMaskParams* bm) {
  if (!a) return RFA_ERR_NULL;
  Ext e;
  if (int rce = parse_ext(ext, &e)) return rce;
  int rc = check_common(a->dtype, a->H, a->Hk, a->D, a->B);
  if (rc) return rc;
  if (a->Sq < 0 || a->Sk < 0) return RFA_ERR_SHAPE;
  if (e.cap > 0.f) {
    if (!cap_args_ok(*a, norm_args(*a), e)) return RFA_ERR_ARGS;     // (with a bias too: refused whatever the band)
    if (shift_args_ok(*a) && band_empty(*a)) e.cap = 0.f;           // nothing visible: the call without the extension
  }
  if (e.slopes != nullptr) {
    if (!shift_args_ok(*a)) return RFA_ERR_ARGS;
    if (band_empty(*a)) e.slopes = nullptr;        // nothing visible: the bias has nothing to act on — the call without it
    else if (!bias_args_ok(*a, norm_args(*a), e)) return RFA_ERR_ARGS;
  }
  if (a->B == 0 || a->Sq == 0) return RFA_OK;
  // what the launchers and the tile loaders' 32-bit descriptor arithmetic cannot express (rfa.h: "row strides", "extents"):
  // refused from the numbers alone, before a pointer is looked at.  The 1-D grids hold at most one workgroup per 128 query
  // rows, head, batch entry and split-KV share (the plan shares only under-filled grids by itself: a count that matters
  // here was asked for by name); the combine pass of such shares has B as grid.y.
  {
    const int Dw = Dv > a->D ? Dv : a->D;
    if (!row_ok(a->q_st, a->D, 2) || !row_ok(a->k_st, a->D, 2) || !row_ok(a->v_st, Dw, 2) ||
        !(a->out_acc ? row_ok(a->out_acc_st, Dw, 4) : row_ok(a->out_st, Dw, 2)))
      return RFA_ERR_ARGS;
    const int64_t shares = a->kv_nsplit > 1 ? (a->kv_nsplit > 8 ? 8 : a->kv_nsplit) : 1;
    if (!grid_x_ok(mul_sat(ceil_div(eff_len(a->Sq, a->q_half), 128), a->H, a->B, shares))) return RFA_ERR_SHAPE;
    if (shares > 1 && !grid_yz_ok(a->B)) return RFA_ERR_SHAPE;
  }
  if (!a->q || !a->k || !a->v) return RFA_ERR_NULL;
  if (a->out_acc) {
    if (!a->lse_acc) return RFA_ERR_NULL;
  } else if (!a->out || !a->lse) {
    return RFA_ERR_NULL;
  }
  if ((a->cu_seqlens_q == nullptr) != (a->cu_seqlens_k == nullptr)) return RFA_ERR_ARGS;
  if (!drop_args_ok(a->dropout_p, a->window, a->window_left, a->window_right, a->causal)) return RFA_ERR_ARGS;
  if (!pos_map_ok(*a)) return RFA_ERR_ARGS;
  if (!shift_args_ok(*a)) return RFA_ERR_ARGS;
  // a block with no visible element: accumulate mode has nothing to merge; plain mode (and the first block of a ring)
  // runs the canonical empty band, whose workgroups load no tile and write out = 0, lse = +inf (-inf into lse_acc)
  if (a->out_acc && !a->acc_init && a->Sk > 0 && band_empty(*a)) return RFA_OK;
  const rfa_fwd_args na = norm_args(*a);
  a = &na;
  if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v)) return RFA_ERR_ALIGN;
  if (!stride_ok(a->q_st, 2) || !stride_ok(a->k_st, 2) || !stride_ok(a->v_st, 2)) return RFA_ERR_ALIGN;
  if (a->out_acc) {
    if (!aligned16(a->out_acc) || !stride_ok(a->out_acc_st, 4)) return RFA_ERR_ALIGN;
  } else {
    if (!aligned16(a->out) || !stride_ok(a->out_st, 2)) return RFA_ERR_ALIGN;
  }
  FwdParams p{};
  p.q = a->q; p.k = a->k; p.v = a->v;
  p.out = a->out; p.lse = a->lse;
  p.out_acc = a->out_acc; p.lse_acc = a->lse_acc;
  p.cu_q = a->cu_seqlens_q; p.cu_k = a->cu_seqlens_k;
  p.q_st = cv(a->q_st); p.k_st = cv(a->k_st); p.v_st = cv(a->v_st);
  p.out_st = cv(a->out_st); p.out_acc_st = cv(a->out_acc_st);
  p.lse_batch = a->lse_batch; p.lse_head = a->lse_head;
  p.lse_acc_batch = a->lse_acc_batch; p.lse_acc_head = a->lse_acc_head;
  p.B = a->B; p.H = a->H; p.Hk = a->Hk; p.D = a->D; p.Sq = a->Sq; p.Sk = a->Sk;
  p.q_half = a->q_half; p.k_half = a->k_half;
  p.causal = a->causal ? 1 : 0; p.acc_init = a->acc_init ? 1 : 0;
  p.wl = (a->window && a->window_left >= 0) ? a->window_left : -1;
  p.wr = a->causal ? 0 : ((a->window && a->window_right >= 0) ? a->window_right : -1);
  p.shift = (p.causal || p.wl >= 0 || p.wr >= 0) ? (int)a->mask_shift : 0;
  p.shift_lens = (p.causal || p.wl >= 0 || p.wr >= 0) ? a->mask_shift_lens : 0;
  p.scale = a->softmax_scale;
  p.drop_keep = drop_threshold(a->dropout_p);
  p.drop_scale = drop_rescale(a->dropout_p);
  p.drop_seed = a->dropout_seed;
  set_pos_map(p, *a);
  // 256 query rows per workgroup (8 waves) or 128 (4 waves, two workgroups per CU), and the split-KV shares: fwd_plan()
  // a bias runs the 256-row form: the persistent form, the 4-wave form and split-KV shares do not exist for it and read as
  // RFA_FWD_AUTO / "never split" (`workspace` is ignored), as they do for dropout
  // (a soft cap likewise: the 256-row instances with or without a window)
  // (row ranges likewise: the windowed 256-row instances with kRng, never split)
  // (a block mask likewise: the windowed 256-row instances with kBlk)
  const bool bias = e.slopes != nullptr || e.cap > 0.f || rr != nullptr || bm != nullptr;
  if (rr != nullptr && (!rr->start || !rr->end)) return RFA_ERR_NULL;
  if (bm != nullptr && !bm->mask) return RFA_ERR_NULL;
  if (e.slopes != nullptr) set_bias(p, e, a->softmax_scale);
  if (e.cap > 0.f) set_cap(p, e, a->softmax_scale);
  const FwdPlan plan = bias ? FwdPlan{fwd_qrows_per_block(), 1, 0} : fwd_plan(a);
  int rows = plan.rows;
  // split-KV (needs the caller's workspace): the 128-row form with the key tiles of a workgroup shared by kv_nsplit
  const int ns = (a->workspace != nullptr && fwd_rows_total(a) > 0 && !bias) ? plan.ns : 1;
  if (a->kv_nsplit < 0) return RFA_ERR_ARGS;
  if (ns <= 1 && plan.ns > 1) {                              // planned with shares but called without a workspace: the unsplit plan
    rfa_fwd_args b = *a;
    b.kv_nsplit = 1;
    rows = fwd_plan(&b).rows;
  }
  CombineParams cb{};
  if (ns > 1) {
    if (!aligned16(a->workspace)) return RFA_ERR_ALIGN;
    const int64_t rt = fwd_rows_total(a);
    // partial layout: out (ns, rows_total, H, D) fp32, lse (ns, [B,] H, rows) fp32 behind it — addressed by the kernel
    // through the accumulate-mode fields (the call's own accumulators, if any, are the combine kernel's business)
    p.kv_nsplit = ns;
    p.part_out = (float*)a->workspace;
    p.part_lse = p.part_out + (int64_t)ns * rt * a->H * a->D;
    p.part_out_split = rt * a->H * a->D;
    p.part_lse_split = rt * a->H;
    p.out_acc_st = Strides{a->cu_seqlens_q ? 0 : (int64_t)a->Sq * a->H * a->D, (int64_t)a->H * a->D, (int64_t)a->D};
    p.lse_acc_batch = a->cu_seqlens_q ? 0 : (int64_t)a->H * a->Sq;
    p.lse_acc_head = a->cu_seqlens_q ? rt : (int64_t)a->Sq;
    cb.part_out = p.part_out; cb.part_lse = p.part_lse; cb.part_st = p.out_acc_st;
    cb.part_lse_batch = p.lse_acc_batch; cb.part_lse_head = p.lse_acc_head;
    cb.part_out_split = p.part_out_split; cb.part_lse_split = p.part_lse_split;
    cb.nsplit = ns;
    cb.out = a->out; cb.lse = a->lse; cb.out_acc = a->out_acc; cb.lse_acc = a->lse_acc;
    cb.out_st = cv(a->out_st); cb.out_acc_st = cv(a->out_acc_st);
    cb.lse_batch = a->lse_batch; cb.lse_head = a->lse_head;
    cb.lse_acc_batch = a->lse_acc_batch; cb.lse_acc_head = a->lse_acc_head;
    cb.cu_q = a->cu_seqlens_q;
    cb.B = a->B; cb.H = a->H; cb.D = a->D; cb.Sq = a->Sq; cb.q_half = a->q_half; cb.acc_init = a->acc_init ? 1 : 0;
  }
  p.qrows = rows;
  p.nqblk = (eff_len(a->Sq, a->q_half) + rows - 1) / rows;
  p.persist_grid = (plan.persist && rows == 256 && ns <= 1 && plan.ns <= 1) ? device_cus() : 0;
  if (a->fwd_form < RFA_FWD_AUTO || a->fwd_form > RFA_FWD_P8x32 || a->fwd_form == RFA_FWD_RETIRED_2) return RFA_ERR_ARGS;
  if (Dv) return launch_status(launch_fwd_vd(p, Dv, a->dtype, (hipStream_t)stream));
  if (rr != nullptr) return launch_status(launch_fwd_rr(p, *rr, a->dtype, (hipStream_t)stream));
  if (bm != nullptr) return launch_status(launch_fwd_bm(p, *bm, a->dtype, (hipStream_t)stream));
  if (a->D > kHeadDim) return launch_status(launch_fwd_big(p, a->dtype, (hipStream_t)stream));
  if (int rc2 = launch_fwd(p, a->dtype, (hipStream_t)stream)) return launch_status(rc2);
  if (ns > 1 && launch_combine(cb, a->dtype, (hipStream_t)stream)) return RFA_ERR_LAUNCH;
  return RFA_OK;
}

int rfa_bwd_preprocess(const rfa_bwd_preprocess_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = check_common(a->dtype, a->H, a->H, a->D, a->B);
  if (rc) return rc;
  if (a->Sq < 0 || !aux_extents_ok(a->B, a->Sq, a->H)) return RFA_ERR_SHAPE;
  if (a->B == 0 || a->Sq == 0) return RFA_OK;
  if (!row_ok(a->dout_st, a->D, 2) || !row_ok(a->out_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->dout || !a->out || !a->delta) return RFA_ERR_NULL;
  if (!aligned16(a->dout) || !aligned16(a->out) || !stride_ok(a->dout_st, 2) || !stride_ok(a->out_st, 2))
    return RFA_ERR_ALIGN;
  PreParams p{};
  p.dout = a->dout; p.out = a->out; p.delta = a->delta; p.cu_q = a->cu_seqlens_q;
  p.dout_st = cv(a->dout_st); p.out_st = cv(a->out_st);
  p.delta_batch = a->delta_batch; p.delta_head = a->delta_head;
  p.B = a->B; p.H = a->H; p.D = a->D; p.Sq = a->Sq; p.q_half = a->q_half;
  return launch_preprocess(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// delta' = rowsum(dout * out) - dlse (rfa.h): the gradient of lse rides on delta into every backward kernel.  A NULL dlse
// launches the plain instance — the call is rfa_bwd_preprocess.
int rfa_bwd_preprocess_lse(const rfa_bwd_preprocess_lse_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = check_common(a->dtype, a->H, a->H, a->D, a->B);
  if (rc) return rc;
  if (a->Sq < 0 || !aux_extents_ok(a->B, a->Sq, a->H)) return RFA_ERR_SHAPE;
  if (a->reserved != 0 || a->q_half < RFA_HALF_FULL || a->q_half > RFA_HALF_BACK) return RFA_ERR_ARGS;
  if (a->B == 0 || a->Sq == 0) return RFA_OK;
  if (!row_ok(a->dout_st, a->D, 2) || !row_ok(a->out_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->dout || !a->out || !a->delta) return RFA_ERR_NULL;
  if (!aligned16(a->dout) || !aligned16(a->out) || !stride_ok(a->dout_st, 2) || !stride_ok(a->out_st, 2))
    return RFA_ERR_ALIGN;
  PreParams p{};
  p.dout = a->dout; p.out = a->out; p.delta = a->delta; p.cu_q = a->cu_seqlens_q;
  p.dout_st = cv(a->dout_st); p.out_st = cv(a->out_st);
  p.delta_batch = a->delta_batch; p.delta_head = a->delta_head;
  p.B = a->B; p.H = a->H; p.D = a->D; p.Sq = a->Sq; p.q_half = a->q_half;
  p.dlse = a->dlse; p.dlse_batch = a->dlse_batch; p.dlse_head = a->dlse_head;
  return launch_preprocess(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// The dK/dV kernel sums the query heads of a K/V group itself, so GQA needs no scratch.  A workspace
// (bf16/fp16 partials, (rows, Hk, D) x 2) is only used when the result is ADDED to fp32 accumulators or
// when compute and reduction are issued as two phases (ring steps: compute overlaps the arrival of the
// accumulators).
static bool bwd_single_phase(const rfa_bwd_args* a) {
  return (a->phases & (RFA_BWD_COMPUTE | RFA_BWD_REDUCE)) == 0;
}
// single-phase call whose dK/dV accumulators are overwritten: the kernel stores fp32 directly
static bool bwd_kv_direct(const rfa_bwd_args* a) {
  return a->dk_acc != nullptr && bwd_single_phase(a) && (a->acc_init || (a->phases & RFA_BWD_KV_OVERWRITE));
}

// Which dK/dV kernel form a call runs — a pure function of the call's arguments (shapes + the dkdv_form /
// dkdv_nsplit fields), so that rfa_bwd_workspace_bytes, a BWD_COMPUTE and its BWD_REDUCE call agree: the 256-key
// workgroup form needs head dim 128 or 64 (exactly) and no window; its workgroups are B * Hk * ceil(Sk / 256), so the Q/dO tile
// range of a key block is shared by up to 4 workgroups until the launch has about two workgroups per CU (a causal
// launch needs that many for its heavy-first order to balance), each with at least 8 tiles.  Launches that stay
// small even so run the 128-key form (twice the workgroups).
struct DkdvPlan { int wide, nsplit, bal; };     // bal: the balanced causal schedule of the 256-key form (dkdv_kernel kBal)
struct DsChunks { int nchunks, hc, gc; int64_t chunk_bytes; };     // hc K/V heads x gc query heads per K/V head per chunk
static DsChunks bwd_ds_chunking(const rfa_bwd_args* a);
// The dK/dV plan by estimated makespan (see "launch plans" above).  Jobs: one workgroup per (batch, K/V head, key block
// [, share of its query tiles]); a key block that starts at key k0 walks the 64-row Q/dO tiles from its causal start
// max(0, k0 - off) to the end of the sequence for each of the G query heads of its K/V head; `ns` workgroups take every
// ns-th of those tiles.  The 128-key form has twice the workgroups, each tile-step with half the MFMAs but the same
// LDS-DMA staging and barrier: 0.7 of the 256-key form's tile time (fitted).  Shares need the fp32 partials + reduce_kernel
// pass: 12 tile-times.  Returns wide (0 / 1) and the share count; only_wide: the best share count of the 256-key form.
// Packed (cu_seqlens) input: the sequences' lengths live on the device — the estimate takes B sequences of the mean
// length total / B (bounded by max_seqlen), which is what the old rule's "about total_k / 256 key blocks" did.
static int bwd_dkdv_cost_plan(const rfa_bwd_args* a, int hk_launch, bool only_wide, int* ns_out, int* bal_out = nullptr) {
  int sk = eff_len(a->Sk, a->k_half), sq = eff_len(a->Sq, a->q_half);
  if (a->cu_seqlens_k != nullptr && a->total_k > 0 && a->B > 0) {
    const int64_t mean_k = (a->total_k + a->B - 1) / a->B;
    const int64_t mean_q = a->total_q > 0 ? (a->total_q + a->B - 1) / a->B : mean_k;
    sk = (int)(mean_k < sk ? mean_k : sk);
    sq = (int)(mean_q < sq ? mean_q : sq);
    if (a->k_half != RFA_HALF_FULL) sk = (sk + 1) / 2;
    if (a->q_half != RFA_HALF_FULL) sq = (sq + 1) / 2;
  }
  const bool big = a->D > kHeadDim;          // rfa_bigd.hip: 128-key workgroups (one wave per SIMD), 32-row Q/dO tiles; ONE form
  const int G = a->H / a->Hk;
  const int64_t key[8] = {2 + 16 * (a->causal ? plan_shift(a) : 0), a->B, hk_launch, G, sq, sk, a->causal ? 1 : 0, (big ? 4 : 0) | (a->D == 64 ? 2 : 0) | (only_wide ? 1 : 0)};
  const uint64_t h = plan_hash(key, 8);
  int code;
  if (plan_lookup(h, &code)) {
    *ns_out = code & 15;
    if (bal_out) *bal_out = (code >> 5) & 1;
    return (code >> 4) & 1;
  }
  if (bal_out) *bal_out = 0;
  const int off = sk - sq + (int)plan_shift(a);
  const int64_t mult = (int64_t)a->B * hk_launch;
  const int trows = big ? 32 : 64;
  const int ntq = (sq + trows - 1) / trows;
  auto estimate = [&](int keys, int ns) {
    const int nkb = (sk + keys - 1) / keys;
    std::vector<int> sizes;
    sizes.reserve((size_t)(nkb * ns * mult));
    for (int kb = 0; kb < nkb; ++kb) {
      int qfirst = a->causal ? kb * keys - off : 0;
      qfirst = qfirst < 0 ? 0 : qfirst;
      const int nt = ntq - qfirst / trows > 0 ? ntq - qfirst / trows : 0;
      for (int sidx = 0; sidx < ns; ++sidx) {
        const int n = nt > sidx ? (nt - 1 - sidx) / ns + 1 : 0;        // tiles nt-1-sidx, nt-1-sidx-ns, ... (dkdv_kernel)
        for (int64_t m = 0; m < mult; ++m) sizes.push_back(n * G);
      }
    }
    // constants: the wide head dims keep round 6's first fit; the 128-wide kernels were re-fitted on the 80 shapes of
    // profiles/r06_plan_sweep_final.md after the batch index became the fastest digit of the dK/dV work decode (which made
    // the heaviest-first assumption of this estimate TRUE for multi-batch launches and the 128-key form — twice the
    // workgroups — the best plan of several of them): worst chosen / best 1.03, mean 1.001
    const double ovh = big ? 12.0 : (keys == 128 ? 6.0 : 8.0);
    double work = 0;
    const double mk = plan_makespan(sizes, ovh, &work);
    if (mk <= 0) return 0.0;
    double busy = work / (mk * kPlanSlots);
    busy = busy > 1 ? 1 : busy;
    return mk * (keys == 128 && !big ? 0.65 : 1.0) * (1 + (big ? kPlanBusyGain : 0.3) * busy * busy) + (ns > 1 ? (big ? 12.0 : 8.0) : 0.0);
  };
  double best = -1;
  int wide = 0, best_ns = 1;
  if (big) {
    for (int ns = 1; ns <= 8; ++ns) {
      if (ns == 5 || ns == 7 || (ns > 1 && ntq / ns < 8)) continue;     // (shares of at least 8 tiles of 32 rows, as rounds 3-5)
      const double c = estimate(128, ns);
      if (best < 0 || c < 0.98 * best) {
        best = c;
        best_ns = ns;
      }
    }
    plan_store(h, best_ns);
    *ns_out = best_ns;
    return 0;
  }
  if (!only_wide) best = estimate(128, 1);
  for (int ns = 1; ns <= 8; ++ns) {
    if (ns == 5 || ns == 7) continue;
    if (ns > 1 && (sq < 1024 ? ns > 2 : ntq / ns < 2)) continue;       // (shares of at least 2 tiles; short sequences: two at most)
    const double c = estimate(256, ns);
    if (best < 0 || c < 0.98 * best) {
      best = c;
      wide = 1;
      best_ns = ns;
    }
  }
  // the balanced causal schedule, where the SHAPE allows it (the caller adds the call-level conditions: bwd_bal_eligible):
  // B * Hk * nkb equal workgroups of (T/2 + 2) G tile-times; half of them cross one key-block seam (a second prologue /
  // epilogue) and every pair exchanges one partial: 14 tile-times of overhead on average instead of 8, no second pass
  int bal = 0;
  if (!only_wide && !big && a->causal && plan_shift(a) == 0 && sq == sk && sk >= 512 && sk % 512 == 0) {
    const int nkb = sk / 256;
    std::vector<int> sizes((size_t)(mult * nkb), (2 * nkb + 2) * G);
    double work = 0;
    const double mk = plan_makespan(sizes, 14.0, &work);
    double busy = work / (mk * kPlanSlots);
    busy = busy > 1 ? 1 : busy;
    bal = mk * (1 + 0.3 * busy * busy) < 0.98 * best ? 1 : 0;
  }
  plan_store(h, (bal << 5) | (wide << 4) | best_ns);
  *ns_out = best_ns;
  if (bal_out) *bal_out = bal;
  return wide;
}

// The balanced causal schedule (rfa_bwd.hip: dkdv_kernel kBal): every workgroup of a dense causal self-attention block
// does the same T/2 + 2 tiles' worth of work, only the lower half of the key blocks is shared (by exactly two workgroups
// that add their partials between themselves): no nsplit fp32 partials per key, no reduce_kernel pass.  Needs the whole
// call in one launch that writes the final dK/dV (single phase, plain outputs or overwritten accumulators, all heads
// at once) and a sequence of whole PAIRS of 256-key blocks.
static bool bwd_bal_eligible(const rfa_bwd_args* a, bool whole_call) {
  if ((a->D != kHeadDim && a->D != 64) || !a->causal || a->cu_seqlens_q != nullptr || a->dropout_p > 0.f) return false;
  if (a->window && (a->window_left >= 0 || a->window_right >= 0)) return false;
  if (plan_shift(a) != 0) return false;        // (the tile deal assumes the block's own diagonal)
  const int lq = eff_len(a->Sq, a->q_half), lk = eff_len(a->Sk, a->k_half);
  if (lq != lk || lk < 512 || (lk % 512) != 0) return false;
  if (!bwd_single_phase(a) || (a->phases & (RFA_BWD_SKIP_DKDV | RFA_BWD_SKIP_DQ))) return false;
  if (a->dk_acc != nullptr && !bwd_kv_direct(a)) return false;
  return whole_call;                           // (not a head-group chunk of a chunked dS hand-off)
}
// hk_launch: K/V heads of ONE dK/dV launch (= Hk, or the K/V heads of a chunk of a chunked dS hand-off)
static DkdvPlan bwd_dkdv_plan_for(const rfa_bwd_args* a, int hk_launch, bool whole_call) {
  DkdvPlan pl{0, 1, 0};
  if (a->D > kHeadDim) {
    // rfa_bigd.hip: 128-key workgroups that occupy a CU each (one wave per SIMD); the tile range of a key block is shared by
    // the number of workgroups with the smallest estimated makespan (fp32 partials, summed by reduce_kernel; round 6: the
    // same estimate as the 128-wide kernels' plan instead of "until about two workgroups per CU")
    int ns = 1;
    (void)bwd_dkdv_cost_plan(a, hk_launch, false, &ns);
    if (a->dkdv_nsplit > 0) ns = a->dkdv_nsplit > 8 ? 8 : a->dkdv_nsplit;
    pl.nsplit = ns;
    return pl;
  }
  const bool win = a->window && (a->window_left >= 0 || (a->window_right >= 0 && !a->causal));
  if (a->dkdv_form == RFA_DKDV_128 || (a->D != kHeadDim && a->D != 64) || win || a->dropout_p > 0.f) return pl;
  // a plan asked for by name (tuning, tests; the REDUCE half of a two-phase call repeats its COMPUTE half's plan)
  if (a->dkdv_form == RFA_DKDV_BAL && bwd_bal_eligible(a, whole_call)) {
    pl.wide = pl.bal = 1;
    return pl;
  }
  if (a->dkdv_form == RFA_DKDV_256 || a->dkdv_nsplit > 0) {
    pl.wide = 1;
    if (a->dkdv_nsplit > 0) {
      pl.nsplit = a->dkdv_nsplit > 8 ? 8 : a->dkdv_nsplit;
    } else {
      rfa_bwd_args b = *a;                                   // form forced, shares free: the count the estimate gives the 256-key form
      b.dkdv_form = RFA_DKDV_AUTO;
      int best_ns = 1;
      (void)bwd_dkdv_cost_plan(&b, hk_launch, true, &best_ns);
      pl.nsplit = best_ns;
    }
    return pl;
  }
  int ns = 1, bal = 0;
  pl.wide = bwd_dkdv_cost_plan(a, hk_launch, false, &ns, &bal);
  pl.nsplit = pl.wide ? ns : 1;
  if (bal && bwd_bal_eligible(a, whole_call)) {
    pl.wide = pl.bal = 1;
    pl.nsplit = 1;
  }
  return pl;
}
static DkdvPlan bwd_dkdv_plan(const rfa_bwd_args* a) {
  const DsChunks ch = bwd_ds_chunking(a);
  return bwd_dkdv_plan_for(a, ch.nchunks > 1 ? ch.hc : a->Hk, ch.nchunks <= 1);
}
static bool bwd_needs_ws(const rfa_bwd_args* a) {
  if (!bwd_single_phase(a)) return true;
  if (bwd_dkdv_plan(a).bal) return true;
  if (bwd_dkdv_plan(a).nsplit > 1) return true;
  if (bwd_ds_chunking(a).gc < a->H / a->Hk) return true;      // query-head fractions of a K/V head accumulate in fp32 partials
  return a->dk_acc != nullptr && !bwd_kv_direct(a);
}

static int64_t bwd_ds_head_blocks(const rfa_bwd_args* a);
static bool bwd_spill_eligible(const rfa_bwd_args* a) {
  if (!((a->cu_seqlens_q == nullptr) == (a->cu_seqlens_k == nullptr) && a->D >= kHeadDim && a->D <= 2 * kHeadDim &&
        a->B > 0 && a->Sq > 0 && a->Sk > 0 && !(a->dropout_p > 0.f) &&
        !(a->window && (a->window_left >= 0 || (a->window_right >= 0 && !a->causal)))))
    return false;
  // one head's share of the scratch stays below 4 GiB: the dK/dV kernel addresses a dS block by a 32-bit scalar offset from
  // its head's base (a single dense causal sequence of 65536 rows — 4.3 GB per head — runs the 7-GEMM form)
  return bwd_ds_head_blocks(a) < ((int64_t)1 << 21);
}

// dS scratch rows: packed triangular for dense causal calls (block (qt, kb) is visited iff kb < qt + c), else
// rectangular, expressed as c >= nKb (rfa_kernels.hpp: ds_row_off)
static int bwd_ds_c(const rfa_bwd_args* a) {
  const int nkb = ds_blocks(a->Sk, a->k_half);
  if (!a->causal || a->cu_seqlens_q != nullptr) return nkb;
  const int off = eff_len(a->Sk, a->k_half) - eff_len(a->Sq, a->q_half) + (int)a->mask_shift;   // (the triangle follows the shifted band)
  const int c = ((31 + off) >> 5) + 1;                   // (arithmetic shift: off may be negative)
  return c > nkb ? nkb : c;
}

// blocks of the dS scratch per head: dense = one (batch, head) — rows rectangular or packed triangular —, packed
// (cu_seqlens) = ALL sequences of a head: total_q / 32 + B rows of ceil(max_seqlen_k / 32) blocks (rfa_kernels.hpp:
// ds_rowpart — bounded by the packed row count instead of B x the longest sequence)
static int64_t bwd_ds_head_blocks(const rfa_bwd_args* a) {
  const int nkb = ds_blocks(a->Sk, a->k_half);
  if (a->cu_seqlens_q != nullptr) {
    const int64_t tq = a->total_q > 0 ? a->total_q : a->total_k;
    return ((tq >> 5) + a->B) * (int64_t)nkb;
  }
  return ds_row_off(ds_blocks(a->Sq, a->q_half), nkb, bwd_ds_c(a), 1);
}
// dS bytes of ONE query head (all batches / packed sequences)
static int64_t bwd_ds_head_bytes(const rfa_bwd_args* a) {
  return (a->cu_seqlens_q != nullptr ? 1 : (int64_t)a->B) * bwd_ds_head_blocks(a) * kDsBlockBytes;
}

static int64_t bwd_ds_scratch_bytes(const rfa_bwd_args* a) {
  if (!bwd_spill_eligible(a)) return 0;
  return (int64_t)a->H * bwd_ds_head_bytes(a);
}

int64_t rfa_bwd_ds_scratch_bytes(const rfa_bwd_args* a) {
  if (!a || !shift_args_ok(*a) || !pos_map_ok(*a)) return 0;
  const rfa_bwd_args na = norm_args(*a);
  return bwd_ds_scratch_bytes(&na);
}

int64_t rfa_bwd_ds_scratch_min_bytes(const rfa_bwd_args* a) {
  if (!a || !shift_args_ok(*a) || !pos_map_ok(*a)) return 0;
  const rfa_bwd_args na = norm_args(*a);
  a = &na;
  if (!bwd_spill_eligible(a)) return 0;
  // head dim 256 (rfa_bigd.hip) has no chunked form; two-phase calls (COMPUTE / REDUCE) chunk by whole K/V heads only
  if (a->D != kHeadDim) return bwd_ds_scratch_bytes(a);
  const int G = a->H / a->Hk;
  return (bwd_single_phase(a) ? 1 : G) * bwd_ds_head_bytes(a);
}

// How the dS hand-off of a call is cut to fit the scratch it was given: all heads at once when they fit; else chunks
// of hc whole K/V heads (hc the largest divisor of Hk whose query heads fit); else — not even one K/V head's G query
// heads fit — chunks of gc query heads of ONE K/V head (gc the largest divisor of G that fits), whose dK/dV shares are
// accumulated in the fp32 partials of the workspace (kv_accum).  nchunks = 0: the 7-GEMM form.
static DsChunks bwd_ds_chunking(const rfa_bwd_args* a) {
  DsChunks none{0, a->Hk, a->H / a->Hk, 0};
  if (a->ds_scratch == nullptr || !bwd_spill_eligible(a)) return none;
  const int G = a->H / a->Hk;
  const int64_t per = bwd_ds_head_bytes(a);
  const int64_t full = per * a->H;
  const int64_t avail = a->ds_scratch_bytes > 0 ? a->ds_scratch_bytes : full;
  if (per <= 0) return none;
  if (avail >= full) return DsChunks{1, a->Hk, G, full};
  if (a->D != kHeadDim) return none;
  const int64_t fit = avail / per;                       // query heads whose dS fit
  if (fit >= G) {
    int hc = 1;
    for (int d = 1; d <= a->Hk; ++d)
      if (a->Hk % d == 0 && (int64_t)d * G <= fit) hc = d;
    return DsChunks{a->Hk / hc, hc, G, per * hc * G};
  }
  if (fit < 1 || !bwd_single_phase(a)) return none;
  int gc = 1;
  for (int d = 1; d <= G; ++d)
    if (G % d == 0 && d <= fit) gc = d;
  return DsChunks{a->Hk * (G / gc), 1, gc, per * gc};
}

int rfa_bwd_ds_chunks(const rfa_bwd_args* a, int32_t* nchunks, int32_t* kv_heads, int32_t* q_heads, int64_t* chunk_bytes) {
  if (!a) return RFA_ERR_NULL;
  if (int rc = check_common(a->dtype, a->H, a->Hk, a->D, a->B)) return rc;
  if (!shift_args_ok(*a) || !pos_map_ok(*a)) return RFA_ERR_ARGS;
  const rfa_bwd_args na = norm_args(*a);
  a = &na;
  const DsChunks ch = bwd_ds_chunking(a);
  if (nchunks) *nchunks = ch.nchunks;
  if (kv_heads) *kv_heads = ch.hc;
  if (q_heads) *q_heads = ch.gc;
  if (chunk_bytes) *chunk_bytes = ch.chunk_bytes;
  return RFA_OK;
}

int rfa_bwd_plan(const rfa_bwd_args* a, int32_t* form, int32_t* nsplit, int32_t* five_gemm) {
  if (!a) return RFA_ERR_NULL;
  if (!shift_args_ok(*a) || !pos_map_ok(*a)) return RFA_ERR_ARGS;
  const rfa_bwd_args na = norm_args(*a);
  a = &na;
  const DkdvPlan pl = bwd_dkdv_plan(a);
  if (form) *form = pl.bal ? RFA_DKDV_BAL : pl.wide ? RFA_DKDV_256 : RFA_DKDV_128;
  if (nsplit) *nsplit = pl.nsplit;
  if (five_gemm) *five_gemm = bwd_ds_chunking(a).nchunks > 0 ? 1 : 0;
  return RFA_OK;
}

static int64_t bal_flag_bytes(int64_t pairs) { return (pairs * 4 + 255) / 256 * 256; }

int64_t rfa_bwd_workspace_bytes(const rfa_bwd_args* a) {
  if (!a || !shift_args_ok(*a) || !pos_map_ok(*a)) return 0;
  const rfa_bwd_args na = norm_args(*a);
  a = &na;
  if (!bwd_needs_ws(a)) return 0;
  // balanced schedule: one fp32 pair slot (dK + dV accumulators of 256 keys) per key block of the lower half of every
  // (batch, K/V head) + one flag word per pair (rounded up to 256 bytes, in front of the slots)
  if (bwd_dkdv_plan(a).bal) {
    const int64_t pairs = (int64_t)a->B * a->Hk * (eff_len(a->Sk, a->k_half) / 512);
    return bal_flag_bytes(pairs) + pairs * 2 * 256 * (int64_t)a->D * 4;
  }
  // unsplit: one io-dtype partial per element; split launches: nsplit fp32 partials
  const int ns = bwd_dkdv_plan(a).nsplit;
  const bool f32 = ns > 1 || bwd_ds_chunking(a).gc < a->H / a->Hk;
  return 2 * a->total_k * (int64_t)a->Hk * a->D * (f32 ? 4 * ns : 2);
}

int rfa_bwd(const rfa_bwd_args* a, void* stream) { return rfa_bwd_ex(a, nullptr, stream); }

// Dv = 0: one head dim (rfa_bwd, rfa_bwd_ex); else the V head dim of rfa_bwd_vd — the same plan, workspace layout (dV in D-wide
// slots, Dv of them used) and dS hand-off, with the dK + dV and 7-GEMM dQ kernels of rfa_vdim.hip
static int bwd_impl(const rfa_bwd_args* a, const rfa_ext_args* ext, int Dv, void* stream, const RowRangeParams* rr = nullptr,
                    const BlockMaskParams* bm = nullptr);
// (the kernels read the mask's bytes through windows of bits in scalar registers: no packed form, no workspace)
int64_t rfa_blockmask_workspace_bytes(const rfa_bwd_args* a) {
  (void)a;
  return 0;
}
int rfa_bwd_bm(const rfa_bwd_args* a, const rfa_blockmask_args* bm, void* stream) {
  if (!a) return RFA_ERR_NULL;
  BlockMaskParams m;
  if (int rc = parse_bm(bm, &m)) return rc;
  if (int rc = rr_base_check(a->dropout_p, a->cu_seqlens_q, a->cu_seqlens_k, a->q_half, a->k_half)) return rc;
  // the masked kernels are the 128-key dK/dV and the 7-GEMM dQ, and the base arguments must say so (as for rfa_bwd_rr)
  if (a->ds_scratch != nullptr || a->dkdv_form != RFA_DKDV_128) return RFA_ERR_ARGS;
  if (int rc = bm_dim_check(a->D, a->H, a->Hk, bm)) return rc;
  return bwd_impl(a, nullptr, 0, stream, nullptr, &m);
}
int64_t rfa_rowrange_workspace_bytes(const rfa_bwd_args* a) {
  if (!a || a->B <= 0 || a->Sq <= 0) return 0;
  return (int64_t)a->B * ((a->Sq + kRrTileRows - 1) / kRrTileRows) * (int64_t)sizeof(int2);
}
int rfa_bwd_rr(const rfa_bwd_args* a, const rfa_rowrange_args* rr, void* stream) {
  if (!a) return RFA_ERR_NULL;
  RowRangeParams r;
  if (int rc = parse_rr(rr, &r)) return rc;
  if (int rc = rr_base_check(a->dropout_p, a->cu_seqlens_q, a->cu_seqlens_k, a->q_half, a->k_half)) return rc;
  // the ranged kernels are the 128-key dK/dV and the 7-GEMM dQ, and the base arguments must say so (as for rfa_bwd_ex)
  if (a->ds_scratch != nullptr || a->dkdv_form != RFA_DKDV_128) return RFA_ERR_ARGS;
  if (int rc = rr_dim_check(a->D, r)) return rc;
  r.ntile_q = a->Sq > 0 ? (a->Sq + kRrTileRows - 1) / kRrTileRows : 0;
  return bwd_impl(a, nullptr, 0, stream, &r);
}
int rfa_bwd_ex(const rfa_bwd_args* a, const rfa_ext_args* ext, void* stream) { return bwd_impl(a, ext, 0, stream); }
int rfa_bwd_vd(const rfa_bwd_args* a, const rfa_vdim_args* vd, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int Dv = 0;
  if (int rc = parse_vdim(vd, a->dropout_p, a->D, &Dv)) return rc;
  return bwd_impl(a, nullptr, Dv, stream);
}

static int bwd_impl(const rfa_bwd_args* a, const rfa_ext_args* ext, int Dv, void* stream, const RowRangeParams* rr,
                    const BlockMaskParams* bm) {
  if (!a) return RFA_ERR_NULL;
  Ext e;
  if (int rce = parse_ext(ext, &e)) return rce;
  int rc = check_common(a->dtype, a->H, a->Hk, a->D, a->B);
  if (rc) return rc;
  if (a->Sq < 0 || a->Sk < 0) return RFA_ERR_SHAPE;
  if (e.cap > 0.f) {
    if (!cap_args_ok(*a, norm_args(*a), e)) return RFA_ERR_ARGS;
    if (shift_args_ok(*a) && band_empty(*a)) e.cap = 0.f;           // nothing visible: zero gradients with or without a cap
    // as for the bias below: the capped kernels are the 128-key dK/dV and the 7-GEMM dQ, and the base arguments must say so
    else if (a->dkdv_form != RFA_DKDV_128 || a->ds_scratch != nullptr) return RFA_ERR_ARGS;
  }
  if (e.slopes != nullptr) {
    if (!shift_args_ok(*a)) return RFA_ERR_ARGS;
    if (band_empty(*a)) e.slopes = nullptr;        // nothing visible: zero gradients with or without a bias
    else if (!bias_args_ok(*a, norm_args(*a), e)) return RFA_ERR_ARGS;
    // a bias runs the plain 128-key dK/dV kernel and the 7-GEMM dQ kernel.  rfa_bwd_plan / rfa_bwd_workspace_bytes do not see
    // the extension, so the BASE arguments must already plan to that: the two can then never disagree with this call
    else if (a->dkdv_form != RFA_DKDV_128 || a->ds_scratch != nullptr) return RFA_ERR_ARGS;
  }
  if (a->B == 0 || a->Sq == 0 || a->Sk == 0) return RFA_OK;
  // as in the forward: row strides and 1-D grids the kernels and launchers cannot express are refused from the numbers alone
  // (dQ: one workgroup per 128 rows, head and batch entry at most; dK/dV: per 128 keys, K/V head, batch entry and share —
  // the plan shares only under-filled grids by itself)
  {
    const int Dw = Dv > a->D ? Dv : a->D;
    if (!row_ok(a->dout_st, Dw, 2) || !row_ok(a->q_st, a->D, 2) || !row_ok(a->k_st, a->D, 2) || !row_ok(a->v_st, Dw, 2) ||
        !(a->dq_acc ? row_ok(a->dq_acc_st, a->D, 4) : row_ok(a->dq_st, a->D, 2)) ||
        !(a->dk_acc ? row_ok(a->dk_acc_st, a->D, 4) && row_ok(a->dv_acc_st, Dw, 4)
                    : row_ok(a->dk_st, a->D, 2) && row_ok(a->dv_st, Dw, 2)))
      return RFA_ERR_ARGS;
    const int64_t shares = a->dkdv_nsplit > 1 ? a->dkdv_nsplit : 1;
    if (!grid_x_ok(mul_sat(ceil_div(eff_len(a->Sq, a->q_half), 128), a->H, a->B)) ||
        !grid_x_ok(mul_sat(ceil_div(eff_len(a->Sk, a->k_half), 128), a->Hk, a->B, shares)))
      return RFA_ERR_SHAPE;
  }
  if (!a->dout || !a->q || !a->k || !a->v || !a->lse || !a->delta) return RFA_ERR_NULL;
  if (!a->dq && !a->dq_acc) return RFA_ERR_NULL;
  if ((a->dk_acc == nullptr) != (a->dv_acc == nullptr)) return RFA_ERR_ARGS;
  if (!a->dk_acc && (!a->dk || !a->dv)) return RFA_ERR_NULL;
  if ((a->cu_seqlens_q == nullptr) != (a->cu_seqlens_k == nullptr)) return RFA_ERR_ARGS;
  if (a->dkdv_form < RFA_DKDV_AUTO || a->dkdv_form > RFA_DKDV_BAL || a->dkdv_nsplit < 0) return RFA_ERR_ARGS;
  if (!drop_args_ok(a->dropout_p, a->window, a->window_left, a->window_right, a->causal)) return RFA_ERR_ARGS;
  if (!pos_map_ok(*a)) return RFA_ERR_ARGS;
  if (!shift_args_ok(*a)) return RFA_ERR_ARGS;
  // a block with no visible element adds nothing to accumulators (either phase of a two-phase call); where something has
  // to be written — plain outputs, overwritten accumulators — the kernels run the canonical empty band and store zeros
  if (a->dq_acc && a->dk_acc && !a->acc_init && !(a->phases & RFA_BWD_KV_OVERWRITE) && band_empty(*a)) {
    if (a->prof_events)
      for (int i = 0; i < 4; ++i)
        if (a->prof_events[i]) (void)hipEventRecord((hipEvent_t)a->prof_events[i], (hipStream_t)stream);
    return RFA_OK;
  }
  const rfa_bwd_args na = norm_args(*a);
  a = &na;
  const bool ws = bwd_needs_ws(a);
  // B is grid.y of the pass that sums the workspace's partials (reduce_kernel: 16 (key, K/V head) pairs per workgroup along
  // grid.x) and of the row ranges' tile-bounds kernel
  if ((ws || rr != nullptr) && !grid_yz_ok(a->B)) return RFA_ERR_SHAPE;
  if (ws && !grid_x_ok(ceil_div(mul_sat(a->Sk, a->Hk), 16))) return RFA_ERR_SHAPE;
  if (ws && !a->workspace) return RFA_ERR_NULL;
  if (!aligned16(a->dout) || !aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v))
    return RFA_ERR_ALIGN;
  if (!stride_ok(a->dout_st, 2) || !stride_ok(a->q_st, 2) || !stride_ok(a->k_st, 2) || !stride_ok(a->v_st, 2))
    return RFA_ERR_ALIGN;
  if (a->dq_acc && (!aligned16(a->dq_acc) || !stride_ok(a->dq_acc_st, 4))) return RFA_ERR_ALIGN;
  if (!a->dq_acc && (!aligned16(a->dq) || !stride_ok(a->dq_st, 2))) return RFA_ERR_ALIGN;
  if (a->dk_acc && (!aligned16(a->dk_acc) || !aligned16(a->dv_acc) || !stride_ok(a->dk_acc_st, 4) ||
                    !stride_ok(a->dv_acc_st, 4)))
    return RFA_ERR_ALIGN;
  if (!a->dk_acc && (!aligned16(a->dk) || !aligned16(a->dv) || !stride_ok(a->dk_st, 2) || !stride_ok(a->dv_st, 2)))
    return RFA_ERR_ALIGN;

  if (rr != nullptr) {
    if (!rr->start || !rr->end || !rr->tile_bounds) return RFA_ERR_NULL;
    if (!aligned16(rr->tile_bounds)) return RFA_ERR_ALIGN;
  }
  if (bm != nullptr && !bm->mask) return RFA_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  BwdParams p{};
  p.dout = a->dout; p.q = a->q; p.k = a->k; p.v = a->v; p.lse = a->lse; p.delta = a->delta;
  p.dq = a->dq; p.dq_acc = a->dq_acc;
  p.cu_q = a->cu_seqlens_q; p.cu_k = a->cu_seqlens_k;
  p.dout_st = cv(a->dout_st); p.q_st = cv(a->q_st); p.k_st = cv(a->k_st); p.v_st = cv(a->v_st);
  p.dq_st = cv(a->dq_st); p.dq_acc_st = cv(a->dq_acc_st);
  p.lse_batch = a->lse_batch; p.lse_head = a->lse_head;
  p.delta_batch = a->delta_batch; p.delta_head = a->delta_head;
  p.B = a->B; p.H = a->H; p.Hk = a->Hk; p.D = a->D; p.Sq = a->Sq; p.Sk = a->Sk;
  p.q_half = a->q_half; p.k_half = a->k_half;
  p.causal = a->causal ? 1 : 0; p.acc_init = a->acc_init ? 1 : 0;
  p.wl = (a->window && a->window_left >= 0) ? a->window_left : -1;
  p.wr = a->causal ? 0 : ((a->window && a->window_right >= 0) ? a->window_right : -1);
  p.shift = (p.causal || p.wl >= 0 || p.wr >= 0) ? (int)a->mask_shift : 0;
  p.shift_lens = (p.causal || p.wl >= 0 || p.wr >= 0) ? a->mask_shift_lens : 0;
  p.scale = a->softmax_scale;
  p.drop_keep = drop_threshold(a->dropout_p);
  p.drop_scale = drop_rescale(a->dropout_p);
  p.drop_seed = a->dropout_seed;
  set_pos_map(p, *a);
  if (e.slopes != nullptr) set_bias(p, e, a->softmax_scale);
  if (e.cap > 0.f) set_cap(p, e, a->softmax_scale);
  p.nqblk = (eff_len(a->Sq, a->q_half) + bwd_dq_rows_per_block() - 1) / bwd_dq_rows_per_block();
  const DsChunks chunks = bwd_ds_chunking(a);
  const int Gfull = a->H / a->Hk;
  const bool frac = chunks.nchunks > 0 && chunks.gc < Gfull;       // query-head fractions of a K/V head per launch
  const DkdvPlan plan = bwd_dkdv_plan(a);
  p.wide = plan.wide; p.nsplit = plan.nsplit;
  p.nkblk = (eff_len(a->Sk, a->k_half) + bwd_dkdv_keys_per_block(plan.wide) - 1) / bwd_dkdv_keys_per_block(plan.wide);

  Strides ws_st{};
  const bool part_f32 = plan.nsplit > 1 || frac;
  if (plan.bal) {
    // balanced schedule: the kernel writes the FINAL dK / dV itself (io dtype, or the overwritten fp32 accumulators);
    // the workspace holds the pair flags and the pair slots
    const int64_t pairs = (int64_t)a->B * a->Hk * (p.nkblk / 2);
    p.bal = 1;
    p.pair_flags = (unsigned*)a->workspace;
    p.pair_ws = (char*)a->workspace + bal_flag_bytes(pairs);
    if (a->dk_acc) {
      p.dk = a->dk_acc; p.dv = a->dv_acc;
      p.dk_st = cv(a->dk_acc_st); p.dv_st = cv(a->dv_acc_st);
      p.kv_f32 = 1;
    } else {
      p.dk = a->dk; p.dv = a->dv;
      p.dk_st = cv(a->dk_st); p.dv_st = cv(a->dv_st);
    }
  } else if (bwd_kv_direct(a) && !part_f32) {
    p.dk = a->dk_acc; p.dv = a->dv_acc;
    p.dk_st = cv(a->dk_acc_st); p.dv_st = cv(a->dv_acc_st);
    p.kv_f32 = 1;
  } else if (ws) {
    // partials: (rows, Hk, nsplit, D) contiguous; dense rows = b*Sk + row (own batch stride).  The kernel addresses
    // K/V head hk of split s at element (hk * nsplit + s) * D of a row, reduce_kernel reads the nsplit entries of
    // a K/V head as its "group" (G = nsplit, head stride D).  Split launches — and launches that cover a fraction of
    // a K/V head's query heads (chunked dS hand-off: the later fractions ADD to the partial) — keep fp32 partials
    // (summed, then rounded once: the rounding an unsplit launch does); the others the io dtype.
    const int64_t ns = plan.nsplit;
    const int64_t esz = part_f32 ? 4 : 2;
    ws_st.head = a->D;
    ws_st.row = (int64_t)a->Hk * ns * a->D;
    ws_st.batch = a->cu_seqlens_k ? 0 : (int64_t)a->Sk * a->Hk * ns * a->D;
    p.dk = a->workspace;
    p.dv = (char*)a->workspace + a->total_k * (int64_t)a->Hk * ns * a->D * esz;
    p.dk_st = ws_st; p.dv_st = ws_st;
    p.dk_st.head = p.dv_st.head = ns * a->D;
    p.kv_split_stride = a->D;
    p.kv_f32 = p.kv_part_f32 = part_f32 ? 1 : 0;
  } else {
    p.dk = a->dk; p.dv = a->dv;
    p.dk_st = cv(a->dk_st); p.dv_st = cv(a->dv_st);
  }
  auto mark = [&](int i) {
    if (a->prof_events && a->prof_events[i]) (void)hipEventRecord((hipEvent_t)a->prof_events[i], st);
  };
  mark(0);
  const bool do_compute = bwd_single_phase(a) || (a->phases & RFA_BWD_COMPUTE);
  const bool do_reduce = bwd_single_phase(a) || (a->phases & RFA_BWD_REDUCE);
  const int kv_init = (a->acc_init || (a->phases & RFA_BWD_KV_OVERWRITE)) ? 1 : 0;
  if (do_compute) {
    if (chunks.nchunks > 0) {
      // 5-GEMM form: dK/dV kernel first (it stores dS), then dQ streams dS back — once over all heads, or (a scratch
      // smaller than the whole hand-off) chunk by chunk over head groups that reuse the one scratch in stream order
      if (!aligned16(a->ds_scratch)) return RFA_ERR_ALIGN;
      if (chunks.nchunks > 1 && (a->phases & (RFA_BWD_SKIP_DKDV | RFA_BWD_SKIP_DQ))) return RFA_ERR_ARGS;
      p.ds = a->ds_scratch;
      p.ds_c = bwd_ds_c(a);
      p.ds_tri = p.ds_c < ds_blocks(a->Sk, a->k_half) ? 1 : 0;
      p.ds_packed = a->cu_seqlens_q != nullptr ? 1 : 0;
      p.ds_head_blocks = bwd_ds_head_blocks(a);
      const int nfrac = Gfull / chunks.gc;
      const int64_t kv_esz = p.kv_f32 ? 4 : 2;
      for (int c = 0; c < chunks.nchunks; ++c) {
        BwdParams pc = p;
        if (chunks.nchunks > 1) {
          const int hk0 = frac ? c / nfrac : c * chunks.hc;      // first K/V head of the chunk
          const int f = frac ? c % nfrac : 0;                    // which fraction of that K/V head's query heads
          const int64_t qh0 = (int64_t)hk0 * Gfull + (int64_t)f * chunks.gc;   // first query head
          pc.Hk = chunks.hc;
          pc.H = chunks.hc * chunks.gc;
          pc.q = (const char*)p.q + qh0 * p.q_st.head * 2;
          pc.dout = (const char*)p.dout + qh0 * p.dout_st.head * 2;
          pc.lse = p.lse + qh0 * p.lse_head;
          pc.delta = p.delta + qh0 * p.delta_head;
          if (p.dq_acc) pc.dq_acc = p.dq_acc + qh0 * p.dq_acc_st.head;
          else pc.dq = (char*)p.dq + qh0 * p.dq_st.head * 2;
          pc.k = (const char*)p.k + (int64_t)hk0 * p.k_st.head * 2;
          pc.v = (const char*)p.v + (int64_t)hk0 * p.v_st.head * 2;
          pc.dk = (char*)p.dk + (int64_t)hk0 * p.dk_st.head * kv_esz;
          pc.dv = (char*)p.dv + (int64_t)hk0 * p.dv_st.head * kv_esz;
          pc.kv_accum = f > 0 ? 1 : 0;
        }
        if (!(a->phases & RFA_BWD_SKIP_DKDV))
          if (int rc2 = Dv ? launch_bwd_dkdv_vd(pc, Dv, a->dtype, st) : launch_bwd_dkdv(pc, a->dtype, st)) return launch_status(rc2);
        if (c == 0) mark(1);
        if (!(a->phases & RFA_BWD_SKIP_DQ))
          if (int rc2 = launch_bwd_dq_from_ds(pc, a->dtype, st)) return launch_status(rc2);
      }
      mark(2);
    } else {
      if (!(a->phases & RFA_BWD_SKIP_DQ))
        if (int rc2 = Dv ? launch_bwd_dq_vd(p, Dv, a->dtype, st) : rr ? launch_bwd_dq_rr(p, *rr, a->dtype, st) : bm ? launch_bwd_dq_bm(p, *bm, a->dtype, st) : launch_bwd_dq(p, a->dtype, st)) return launch_status(rc2);
      mark(1);
      if (!(a->phases & RFA_BWD_SKIP_DKDV))
        if (int rc2 = Dv ? launch_bwd_dkdv_vd(p, Dv, a->dtype, st) : rr ? launch_bwd_dkdv_rr(p, *rr, a->dtype, st) : bm ? launch_bwd_dkdv_bm(p, *bm, a->dtype, st) : launch_bwd_dkdv(p, a->dtype, st)) return launch_status(rc2);
      mark(2);
    }
  } else {
    mark(1);
    mark(2);
  }
  if (ws && do_reduce && !plan.bal) {
    // dK and dV in one launch (grid z)
    ReduceParams r{};
    r.src = p.dk; r.src2 = p.dv;
    r.src_st = ws_st;
    r.src_f32 = part_f32 ? 1 : 0;
    r.cu_k = a->cu_seqlens_k;
    r.B = a->B; r.Hk = a->Hk; r.G = plan.nsplit; r.D = a->D; r.Sk = a->Sk;   // query-head groups are already summed
    r.k_half = a->k_half; r.acc_init = kv_init;
    if (a->dk_acc) {
      r.dst_acc = a->dk_acc; r.dst_acc2 = a->dv_acc;
      r.dst_acc_st = cv(a->dk_acc_st); r.dst_acc2_st = cv(a->dv_acc_st);
    } else {
      r.dst = a->dk; r.dst2 = a->dv;
      r.dst_st = cv(a->dk_st); r.dst2_st = cv(a->dv_st);
    }
    if (Dv) {
      // dK (D wide) and dV (Dv wide) differ in width: the same kernel once per tensor
      ReduceParams rv = r;
      rv.src = r.src2; rv.dst = r.dst2; rv.dst_acc = r.dst_acc2; rv.dst_st = r.dst2_st; rv.dst_acc_st = r.dst_acc2_st;
      rv.src2 = nullptr; rv.dst2 = nullptr; rv.dst_acc2 = nullptr;
      rv.D = Dv;
      r.src2 = nullptr; r.dst2 = nullptr; r.dst_acc2 = nullptr;
      if (launch_reduce(rv, a->dtype, st)) return RFA_ERR_LAUNCH;
    }
    if (launch_reduce(r, a->dtype, st)) return RFA_ERR_LAUNCH;
  }
  mark(3);
  return RFA_OK;
}

int rfa_merge(const rfa_merge_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = check_common(a->dtype, a->H, a->H, a->D, a->B);
  if (rc) return rc;
  if (a->S < 0 || !aux_extents_ok(a->B, a->S, a->H)) return RFA_ERR_SHAPE;
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!row_ok(a->out_acc_st, a->D, 4) || !row_ok(a->block_out_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->out_acc || !a->lse_acc || !a->block_out || !a->block_lse) return RFA_ERR_NULL;
  if (!aligned16(a->out_acc) || !aligned16(a->block_out) || !stride_ok(a->out_acc_st, 4) ||
      !stride_ok(a->block_out_st, 2))
    return RFA_ERR_ALIGN;
  MergeParams p{};
  p.out_acc = a->out_acc; p.lse_acc = a->lse_acc; p.block_out = a->block_out; p.block_lse = a->block_lse;
  p.out_acc_st = cv(a->out_acc_st); p.block_out_st = cv(a->block_out_st);
  p.lse_acc_batch = a->lse_acc_batch; p.lse_acc_head = a->lse_acc_head;
  p.block_lse_batch = a->block_lse_batch; p.block_lse_head = a->block_lse_head;
  p.lse_acc_row = a->lse_acc_row ? a->lse_acc_row : 1;
  p.block_lse_row = a->block_lse_row ? a->block_lse_row : 1;
  p.B = a->B; p.H = a->H; p.D = a->D; p.S = a->S; p.acc_init = a->acc_init ? 1 : 0;
  return launch_merge(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int rfa_sum_slots(const rfa_sum_slots_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = check_common(a->dtype, a->H, a->H, a->D, a->B);
  if (rc) return rc;
  if (a->S < 0 || a->nslots < 1 || !aux_extents_ok(a->B, a->S, a->H)) return RFA_ERR_SHAPE;
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!row_ok(a->src_st, a->D, 2) || !row_ok(a->dst_st, a->D, 2)) return RFA_ERR_ARGS;   // (the slot stride is free: 64 bits)
  if (!a->src || !a->dst) return RFA_ERR_NULL;
  if (!aligned16(a->src) || !aligned16(a->dst) || !stride_ok(a->src_st, 2) || !stride_ok(a->dst_st, 2) ||
      (a->slot_stride % 8) != 0)
    return RFA_ERR_ALIGN;
  ReduceParams r{};
  r.src = a->src; r.src_st = cv(a->src_st);
  r.dst = a->dst; r.dst_st = cv(a->dst_st);
  r.B = a->B; r.Hk = a->H; r.G = a->nslots; r.D = a->D; r.Sk = a->S;
  r.k_half = RFA_HALF_FULL; r.acc_init = 1;
  r.g_stride = a->slot_stride;
  if (launch_reduce(r, a->dtype, (hipStream_t)stream)) return RFA_ERR_LAUNCH;
  return RFA_OK;
}

int rfa_cast(void* dst, const float* src, int64_t n, int32_t dtype, void* stream) {
  if (dtype != RFA_BF16 && dtype != RFA_F16) return RFA_ERR_DTYPE;
  if (n < 0) return RFA_ERR_SHAPE;
  if (n == 0) return RFA_OK;
  if (!dst || !src) return RFA_ERR_NULL;
  if (!aligned16(dst) || !aligned16(src)) return RFA_ERR_ALIGN;
  return launch_cast(dst, src, n, dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int rfa_lse_flatten(float* dst, const float* src, const int32_t* cu_seqlens, int32_t B, int32_t H,
                    int32_t max_seqlen, int64_t dst_head_stride, int64_t dst_row_stride, void* stream) {
  if (B < 0 || H < 0 || max_seqlen < 0 || !grid_yz_ok(B) || !grid_yz_ok(H)) return RFA_ERR_SHAPE;   // (H, B: grid.y, grid.z)
  if (B == 0 || H == 0 || max_seqlen == 0) return RFA_OK;
  if (!dst || !src || !cu_seqlens) return RFA_ERR_NULL;
  return launch_lse_relayout(dst, src, cu_seqlens, B, H, max_seqlen, dst_head_stride, dst_row_stride,
                             true, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int rfa_lse_unflatten(float* dst, const float* src, const int32_t* cu_seqlens, int32_t B, int32_t H,
                      int32_t max_seqlen, int64_t src_head_stride, int64_t src_row_stride, void* stream) {
  if (B < 0 || H < 0 || max_seqlen < 0 || !grid_yz_ok(B) || !grid_yz_ok(H)) return RFA_ERR_SHAPE;   // (H, B: grid.y, grid.z)
  if (B == 0 || H == 0 || max_seqlen == 0) return RFA_OK;
  if (!dst || !src || !cu_seqlens) return RFA_ERR_NULL;
  return launch_lse_relayout(dst, src, cu_seqlens, B, H, max_seqlen, src_head_stride, src_row_stride,
                             false, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- attention sinks (rfa.h; csrc/rfa_sink.hip) ----------------------------------------------------------------------------
static int sink_shape_check(int dtype, int B, int S, int H, int D, int reserved) {
  int rc = check_common(dtype, H, H, D, B);
  if (rc) return rc;
  if (S < 0 || B > 65535 || H > 65535) return RFA_ERR_SHAPE;       // (B and H are grid dimensions)
  if ((int64_t)S * H > (int64_t)16 * INT32_MAX) return RFA_ERR_SHAPE;   // (16 row-heads per workgroup of sink_apply)
  if (reserved != 0) return RFA_ERR_ARGS;
  return RFA_OK;
}

int rfa_sink_apply(const rfa_sink_apply_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = sink_shape_check(a->dtype, a->B, a->S, a->H, a->D, a->reserved);
  if (rc) return rc;
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!row_ok(a->out_src_st, a->D, 2) || !row_ok(a->out_dst_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->out_src || !a->out_dst || !a->lse_src || !a->lse_dst || !a->sinks) return RFA_ERR_NULL;
  if (!aligned16(a->out_src) || !aligned16(a->out_dst) || !stride_ok(a->out_src_st, 2) || !stride_ok(a->out_dst_st, 2))
    return RFA_ERR_ALIGN;
  SinkApplyParams p{};
  p.out_src = a->out_src; p.out_dst = a->out_dst; p.lse_src = a->lse_src; p.lse_dst = a->lse_dst; p.sinks = a->sinks;
  p.out_src_st = cv(a->out_src_st); p.out_dst_st = cv(a->out_dst_st);
  p.lse_src_batch = a->lse_src_batch; p.lse_src_head = a->lse_src_head;
  p.lse_dst_batch = a->lse_dst_batch; p.lse_dst_head = a->lse_dst_head;
  p.B = a->B; p.H = a->H; p.D = a->D; p.S = a->S;
  return launch_sink_apply(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int64_t rfa_sink_grad_workspace_bytes(const rfa_sink_grad_args* a) {
  if (!a || sink_shape_check(a->dtype, a->B, a->S, a->H, a->D, a->reserved)) return 0;
  return sink_grad_parts(a->B, a->S) * a->H * (int64_t)sizeof(float);
}

int rfa_sink_grad(const rfa_sink_grad_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = sink_shape_check(a->dtype, a->B, a->S, a->H, a->D, a->reserved);
  if (rc) return rc;
  if (a->B == 0 || a->S == 0) {                               // no rows: the sum is empty
    if (!a->dsink) return RFA_ERR_NULL;
    return hipMemsetAsync(a->dsink, 0, (size_t)a->H * sizeof(float), (hipStream_t)stream) == hipSuccess ? RFA_OK
                                                                                                         : RFA_ERR_LAUNCH;
  }
  if (!row_ok(a->dout_st, a->D, 2) || !row_ok(a->out_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->dout || !a->out || !a->lse || !a->sinks || !a->dsink || !a->workspace) return RFA_ERR_NULL;
  if (!aligned16(a->dout) || !aligned16(a->out) || !aligned16(a->workspace) || !stride_ok(a->dout_st, 2) ||
      !stride_ok(a->out_st, 2))
    return RFA_ERR_ALIGN;
  if (a->workspace_bytes < rfa_sink_grad_workspace_bytes(a)) return RFA_ERR_ARGS;
  SinkGradParams p{};
  p.dout = a->dout; p.out = a->out; p.lse = a->lse; p.sinks = a->sinks; p.dsink = a->dsink;
  p.partial = (float*)a->workspace;
  p.dout_st = cv(a->dout_st); p.out_st = cv(a->out_st);
  p.lse_batch = a->lse_batch; p.lse_head = a->lse_head;
  p.B = a->B; p.H = a->H; p.D = a->D; p.S = a->S;
  return launch_sink_grad(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- pairwise merge of two finished (out, lse) pairs and its backward (rfa.h; csrc/rfa_mergepair.hip) ---------------------
int rfa_merge_pair(const rfa_merge_pair_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = sink_shape_check(a->dtype, a->B, a->S, a->H, a->D, a->reserved);
  if (rc) return rc;
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!row_ok(a->out_a_st, a->D, 2) || !row_ok(a->out_b_st, a->D, 2) || !row_ok(a->out_st, a->D, 2)) return RFA_ERR_ARGS;
  if (!a->out_a || !a->out_b || !a->lse_a || !a->lse_b || !a->out || !a->lse) return RFA_ERR_NULL;
  if (!aligned16(a->out_a) || !aligned16(a->out_b) || !aligned16(a->out) || !stride_ok(a->out_a_st, 2) ||
      !stride_ok(a->out_b_st, 2) || !stride_ok(a->out_st, 2))
    return RFA_ERR_ALIGN;
  MergePairParams p{};
  p.out_a = a->out_a; p.out_b = a->out_b; p.out = a->out; p.lse_a = a->lse_a; p.lse_b = a->lse_b; p.lse = a->lse;
  p.out_a_st = cv(a->out_a_st); p.out_b_st = cv(a->out_b_st); p.out_st = cv(a->out_st);
  p.lse_a_st = LseSt{a->lse_a_batch, a->lse_a_head}; p.lse_b_st = LseSt{a->lse_b_batch, a->lse_b_head};
  p.lse_st = LseSt{a->lse_batch, a->lse_head};
  p.B = a->B; p.H = a->H; p.D = a->D; p.S = a->S;
  return launch_merge_pair(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int rfa_merge_pair_bwd(const rfa_merge_pair_bwd_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  int rc = sink_shape_check(a->dtype, a->B, a->S, a->H, a->D, a->reserved);
  if (rc) return rc;
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!row_ok(a->dout_st, a->D, 2) || !row_ok(a->out_a_st, a->D, 2) || !row_ok(a->out_b_st, a->D, 2) ||
      !row_ok(a->dout_a_st, a->D, 2) || !row_ok(a->dout_b_st, a->D, 2))
    return RFA_ERR_ARGS;
  if (!a->dout || !a->out_a || !a->out_b || !a->lse_a || !a->lse_b || !a->dout_a || !a->dout_b || !a->dlse_a || !a->dlse_b)
    return RFA_ERR_NULL;
  if (!aligned16(a->dout) || !aligned16(a->out_a) || !aligned16(a->out_b) || !aligned16(a->dout_a) || !aligned16(a->dout_b) ||
      !stride_ok(a->dout_st, 2) || !stride_ok(a->out_a_st, 2) || !stride_ok(a->out_b_st, 2) || !stride_ok(a->dout_a_st, 2) ||
      !stride_ok(a->dout_b_st, 2))
    return RFA_ERR_ALIGN;
  MergePairBwdParams p{};
  p.dout = a->dout; p.out_a = a->out_a; p.out_b = a->out_b; p.dlse = a->dlse; p.lse_a = a->lse_a; p.lse_b = a->lse_b;
  p.dout_a = a->dout_a; p.dout_b = a->dout_b; p.dlse_a = a->dlse_a; p.dlse_b = a->dlse_b;
  p.dout_st = cv(a->dout_st); p.out_a_st = cv(a->out_a_st); p.out_b_st = cv(a->out_b_st);
  p.dout_a_st = cv(a->dout_a_st); p.dout_b_st = cv(a->dout_b_st);
  p.dlse_st = LseSt{a->dlse_batch, a->dlse_head};
  p.lse_a_st = LseSt{a->lse_a_batch, a->lse_a_head}; p.lse_b_st = LseSt{a->lse_b_batch, a->lse_b_head};
  p.dlse_a_st = LseSt{a->dlse_a_batch, a->dlse_a_head}; p.dlse_b_st = LseSt{a->dlse_b_batch, a->dlse_b_head};
  p.B = a->B; p.H = a->H; p.D = a->D; p.S = a->S;
  return launch_merge_pair_bwd(p, a->dtype, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- sequence/head exchange copies (rfa.h; csrc/rfa_seqhead.hip) -----------------------------------------------------------
int rfa_seq_head_copy(const rfa_seq_head_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  if (a->struct_bytes != sizeof(rfa_seq_head_args) || a->reserved != 0) return RFA_ERR_ARGS;
  if (a->op < RFA_SEQHEAD_PACK || a->op > RFA_SEQHEAD_SLOTS_TO_HEADS) return RFA_ERR_ARGS;
  if (a->layout < RFA_SEQHEAD_CONTIGUOUS || a->layout > RFA_SEQHEAD_STRIPE) return RFA_ERR_ARGS;
  if (a->ntensors < 1 || a->ntensors > 3) return RFA_ERR_ARGS;
  for (int k = 0; k < a->ntensors; ++k)
    if (a->t[k].P < 1 || a->t[k].P > 3) return RFA_ERR_ARGS;
  if (a->elem_bytes != 2) return RFA_ERR_DTYPE;
  if (a->D <= 0 || a->D > kMaxHeadDim || (a->D % 8) != 0) return RFA_ERR_HEAD_DIM;
  if (a->U <= 0 || a->B < 0 || a->S < 0) return RFA_ERR_SHAPE;
  if (a->layout == RFA_SEQHEAD_ZIGZAG && (a->S & 1)) return RFA_ERR_SHAPE;
  if ((int64_t)a->U * a->S > INT32_MAX) return RFA_ERR_SHAPE;
  const int64_t rows = (int64_t)a->U * a->S * a->B;            // (U * S fits 31 bits: the product fits 62)
  if (rows > INT32_MAX) return RFA_ERR_SHAPE;
  for (int k = 0; k < a->ntensors; ++k)                        // every tensor's heads before any tensor's chunk count
    if (a->t[k].H <= 0 || (a->t[k].H % a->U) != 0) return RFA_ERR_HEADS;
  SeqHeadParams p{};
  p.g.op = a->op; p.g.layout = a->layout;
  p.g.U = (uint32_t)a->U; p.g.B = (uint32_t)a->B; p.g.S = (uint32_t)a->S; p.g.D8 = (uint32_t)a->D / 8;
  int64_t slot = 0;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_seq_head_tensor& s = a->t[k];
    const int64_t rowchunks = (int64_t)s.P * (s.H / a->U) * (a->D / 8);
    // (both factors are checked to fit 31 bits before they are multiplied: the product fits 62)
    if (rowchunks > INT32_MAX || rows * rowchunks > INT32_MAX) return RFA_ERR_SHAPE;
    const int64_t nchunks = rows * rowchunks;
    SeqHeadTensor& t = p.t[k];
    t.batch = s.batch; t.row = s.row; t.part = s.P > 1 ? s.part : 0; t.head = s.head;
    t.slot_base = slot;
    t.P = (uint32_t)s.P; t.Hs = (uint32_t)(s.H / a->U); t.rowchunks = (uint32_t)rowchunks; t.nchunks = (uint32_t)nchunks;
    slot += (int64_t)a->B * a->S * rowchunks * 8;
    p.strided[k] = s.ptr;
  }
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!a->slots) return RFA_ERR_NULL;
  for (int k = 0; k < a->ntensors; ++k)
    if (!a->t[k].ptr) return RFA_ERR_NULL;
  if (!aligned16(a->slots)) return RFA_ERR_ALIGN;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_seq_head_tensor& s = a->t[k];
    if (!aligned16(s.ptr) || (s.batch % 8) || (s.row % 8) || (s.head % 8) || (s.P > 1 && (s.part % 8))) return RFA_ERR_ALIGN;
  }
  if (a->slots_elems < (int64_t)a->U * slot) return RFA_ERR_ARGS;
  p.g.slot_stride = slot;
  p.slots = a->slots;
  p.ntensors = a->ntensors;
  return launch_seq_head_copy(p, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- rotary position embedding (rfa.h; csrc/rfa_rotary.hip) ------------------------------------------------------------------
int rfa_rotary(const rfa_rotary_args* a, void* stream) {
  if (!a) return RFA_ERR_NULL;
  if (a->struct_bytes != sizeof(rfa_rotary_args) || a->reserved != 0) return RFA_ERR_ARGS;
  if (a->ntensors < 1 || a->ntensors > 2) return RFA_ERR_ARGS;
  if (a->interleaved < 0 || a->interleaved > 1 || a->conj < 0 || a->conj > 1) return RFA_ERR_ARGS;
  for (int k = 0; k < a->ntensors; ++k)
    if (a->t[k].pad != 0) return RFA_ERR_ARGS;
  if (a->dtype != RFA_BF16 && a->dtype != RFA_F16) return RFA_ERR_DTYPE;
  if (a->table_dtype != a->dtype && a->table_dtype != RFA_ROTARY_TABLE_F32) return RFA_ERR_DTYPE;
  if (a->D <= 0 || a->D > kMaxHeadDim || (a->D % 8) != 0) return RFA_ERR_HEAD_DIM;
  if (a->R <= 0 || (a->R % (a->interleaved ? 8 : 16)) != 0) return RFA_ERR_HEAD_DIM;
  if (a->rot_offset < 0 || (a->rot_offset % 8) != 0 || a->rot_offset > a->D - a->R) return RFA_ERR_HEAD_DIM;
  if (a->B < 0 || a->S < 0 || a->P < 1) return RFA_ERR_SHAPE;
  const int64_t rows = (int64_t)a->B * a->S;
  if (rows > INT32_MAX) return RFA_ERR_SHAPE;
  for (int k = 0; k < a->ntensors; ++k)                        // every tensor's heads before any tensor's unit count
    if (a->t[k].H <= 0) return RFA_ERR_HEADS;
  RotaryParams p{};
  p.g.B = (uint32_t)a->B; p.g.S = (uint32_t)a->S; p.g.R = (uint32_t)a->R; p.g.rot_off = (uint32_t)a->rot_offset;
  p.g.rot_units = (uint32_t)(a->interleaved ? a->R / 8 : a->R / 16);
  p.g.interleaved = a->interleaved;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_rotary_tensor& s = a->t[k];
    const int64_t uph = rotary_units_per_head((uint32_t)a->D, (uint32_t)a->R, a->interleaved, s.dst == s.src);
    // (rows and H fit 31 bits each, uph <= 32: the products fit 62 and 36 bits)
    if (rows * s.H > INT32_MAX || rows * s.H * uph > INT32_MAX) return RFA_ERR_SHAPE;
    RotaryTensor& t = p.t[k];
    t.sb = s.src_batch; t.sr = s.src_row; t.sh = s.src_head;
    t.db = s.dst_batch; t.dr = s.dst_row; t.dh = s.dst_head;
    t.H = (uint32_t)s.H; t.uph = (uint32_t)uph; t.nunits = (uint32_t)(rows * s.H * uph);
    p.src[k] = s.src; p.dst[k] = s.dst;
  }
  if (a->B == 0 || a->S == 0) return RFA_OK;
  if (!a->cos || !a->sin) return RFA_ERR_NULL;
  for (int k = 0; k < a->ntensors; ++k)
    if (!a->t[k].src || !a->t[k].dst) return RFA_ERR_NULL;
  if (!aligned16(a->cos) || !aligned16(a->sin)) return RFA_ERR_ALIGN;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_rotary_tensor& s = a->t[k];
    if (!aligned16(s.src) || !aligned16(s.dst) || (s.src_batch % 8) || (s.src_row % 8) || (s.src_head % 8) ||
        (s.dst_batch % 8) || (s.dst_row % 8) || (s.dst_head % 8))
      return RFA_ERR_ALIGN;
  }
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_rotary_tensor& s = a->t[k];
    if (s.dst == s.src && (s.src_batch != s.dst_batch || s.src_row != s.dst_row || s.src_head != s.dst_head)) return RFA_ERR_ARGS;
  }
  if (a->pos_batch < 0) return RFA_ERR_ARGS;
  const uint32_t stride = a->pos_stride > 0 ? (uint32_t)a->pos_stride : 1u;
  if (!a->positions) {
    if (a->pos_stride < 0 || a->pos_split < 0 || a->pos_split > a->S - 1) return RFA_ERR_ARGS;
    // the map's pieces are monotone: their ends bound every position
    const uint32_t ends[4] = {0u, (uint32_t)(a->pos_split ? a->pos_split - 1 : a->S - 1), (uint32_t)a->pos_split, (uint32_t)(a->S - 1)};
    // (an offset beyond 2^40 names no table row; refused here so that the sums below cannot overflow)
    if (a->pos_offset < -(1ll << 40) || a->pos_offset > (1ll << 40) || a->pos_offset2 < -(1ll << 40) || a->pos_offset2 > (1ll << 40))
      return RFA_ERR_ARGS;
    for (int e = 0; e < 4; ++e) {
      const int64_t pos = rotary_map_pos(a->pos_offset, stride, a->pos_split, a->pos_offset2, ends[e]);
      if (pos < 0 || pos > a->P - 1) return RFA_ERR_ARGS;
    }
  }
  p.cos = a->cos; p.sin = a->sin; p.P = a->P;
  p.positions = a->positions; p.pos_batch = a->pos_batch;
  p.pos_off = a->pos_offset; p.pos_off2 = a->pos_offset2; p.pos_stride = stride; p.pos_split = a->pos_split;
  p.conj = a->conj;
  p.ntensors = a->ntensors;
  return launch_rotary(p, a->dtype, a->table_dtype == RFA_ROTARY_TABLE_F32, (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- per-head QK RMSNorm + rotary (rfa.h; csrc/rfa_qknorm.hip) ---------------------------------------------------------------
extern "C++" {
// the checks the forward and the backward struct share, in the header's order: `upto` 0 stops in front of "no rows" (everything
// that needs no pointer: what the workspace size depends on), 1 runs them all.  RFA_OK with *launch == false: nothing to do.
template <typename A>
static int qk_norm_check(const A* a, int upto, QkNormParams* p, bool* launch) {
  *launch = false;
  if (!a) return RFA_ERR_NULL;
  if (a->struct_bytes != sizeof(A) || a->reserved != 0) return RFA_ERR_ARGS;
  if (a->ntensors < 1 || a->ntensors > 2) return RFA_ERR_ARGS;
  if (a->interleaved < 0 || a->interleaved > 1) return RFA_ERR_ARGS;
  for (int k = 0; k < a->ntensors; ++k)
    if (a->t[k].pad != 0) return RFA_ERR_ARGS;
  if (!(a->eps >= 0.f) || !(a->eps <= FLT_MAX) || !(a->weight_offset >= -FLT_MAX && a->weight_offset <= FLT_MAX)) return RFA_ERR_ARGS;
  if (a->dtype != RFA_BF16 && a->dtype != RFA_F16) return RFA_ERR_DTYPE;
  if (a->table_dtype != a->dtype && a->table_dtype != RFA_ROTARY_TABLE_F32) return RFA_ERR_DTYPE;
  if (a->weight_dtype != a->dtype && a->weight_dtype != RFA_QK_NORM_WEIGHT_F32) return RFA_ERR_DTYPE;
  if (a->D <= 0 || a->D > kMaxHeadDim || (a->D % 8) != 0) return RFA_ERR_HEAD_DIM;
  if (a->R < 0 || (a->R % (a->interleaved ? 8 : 16)) != 0) return RFA_ERR_HEAD_DIM;
  if (a->rot_offset < 0 || (a->rot_offset % 8) != 0 || a->rot_offset > a->D - a->R) return RFA_ERR_HEAD_DIM;
  if (a->B < 0 || a->S < 0 || (a->R > 0 && a->P < 1)) return RFA_ERR_SHAPE;
  const int64_t rows = (int64_t)a->B * a->S;
  if (rows > INT32_MAX) return RFA_ERR_SHAPE;
  for (int k = 0; k < a->ntensors; ++k)
    if (a->t[k].H <= 0) return RFA_ERR_HEADS;
  for (int k = 0; k < a->ntensors; ++k) {
    if (rows * a->t[k].H > INT32_MAX) return RFA_ERR_SHAPE;
    const rfa_rotary_tensor& s = a->t[k];
    QkNormTensor& t = p->t[k];
    t.xb = s.src_batch; t.xr = s.src_row; t.xh = s.src_head;
    t.ob = s.dst_batch; t.orow = s.dst_row; t.oh = s.dst_head;
    t.H = (uint32_t)s.H; t.nitems = (uint32_t)(rows * s.H);
    p->x[k] = s.src; p->out[k] = s.dst; p->weight[k] = a->weight[k];
  }
  QkNormGeom& g = p->g;
  g.B = (uint32_t)a->B; g.S = (uint32_t)a->S; g.D = (uint32_t)a->D; g.R = (uint32_t)a->R; g.rot_off = (uint32_t)a->rot_offset;
  g.interleaved = a->interleaved; g.chunks = g.D / 8; g.group = qknorm_group(g.D);
  p->ntensors = a->ntensors;
  for (int k = 0; k < a->ntensors; ++k) {
    p->nparts[k] = qknorm_parts(p->t[k].nitems, g.group);
    p->walk[k] = qknorm_walk(p->t[k].nitems, p->nparts[k], g.group);
  }
  p->eps = a->eps; p->weight_offset = a->weight_offset;
  if (a->B == 0 || a->S == 0 || upto == 0) return RFA_OK;
  *launch = true;
  for (int k = 0; k < a->ntensors; ++k)
    if (!a->t[k].src || !a->t[k].dst || !a->weight[k]) return RFA_ERR_NULL;
  if (a->R > 0 && (!a->cos || !a->sin)) return RFA_ERR_NULL;
  return RFA_OK;
}

// the checks behind the NULL checks: alignment, then the rest
template <typename A>
static int qk_norm_check_rest(const A* a) {
  if (a->R > 0 && (!aligned16(a->cos) || !aligned16(a->sin))) return RFA_ERR_ALIGN;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_rotary_tensor& s = a->t[k];
    if (!aligned16(s.src) || !aligned16(s.dst) || !aligned16(a->weight[k]) || (s.src_batch % 8) || (s.src_row % 8) ||
        (s.src_head % 8) || (s.dst_batch % 8) || (s.dst_row % 8) || (s.dst_head % 8))
      return RFA_ERR_ALIGN;
  }
  return RFA_OK;
}

template <typename A>
static int qk_norm_check_map(const A* a, QkNormParams* p) {
  for (int k = 0; k < a->ntensors; ++k)
    if (a->t[k].dst == a->t[k].src) return RFA_ERR_ARGS;
  if (a->pos_batch < 0) return RFA_ERR_ARGS;
  const uint32_t stride = a->pos_stride > 0 ? (uint32_t)a->pos_stride : 1u;
  if (a->R > 0 && !a->positions) {
    if (a->pos_stride < 0 || a->pos_split < 0 || a->pos_split > a->S - 1) return RFA_ERR_ARGS;
    const uint32_t ends[4] = {0u, (uint32_t)(a->pos_split ? a->pos_split - 1 : a->S - 1), (uint32_t)a->pos_split, (uint32_t)(a->S - 1)};
    if (a->pos_offset < -(1ll << 40) || a->pos_offset > (1ll << 40) || a->pos_offset2 < -(1ll << 40) || a->pos_offset2 > (1ll << 40))
      return RFA_ERR_ARGS;
    for (int e = 0; e < 4; ++e) {
      const int64_t pos = rotary_map_pos(a->pos_offset, stride, a->pos_split, a->pos_offset2, ends[e]);
      if (pos < 0 || pos > a->P - 1) return RFA_ERR_ARGS;
    }
  }
  if (a->R > 0) {
    p->cos = a->cos; p->sin = a->sin; p->P = a->P;
    p->positions = a->positions; p->pos_batch = a->pos_batch;
    p->pos_off = a->pos_offset; p->pos_off2 = a->pos_offset2; p->pos_stride = stride; p->pos_split = a->pos_split;
  }
  return RFA_OK;
}
}  // extern "C++"

int rfa_qk_norm_rotary_fwd(const rfa_qk_norm_rotary_args* a, void* stream) {
  QkNormParams p{};
  bool launch = false;
  int rc = qk_norm_check(a, 1, &p, &launch);
  if (rc != RFA_OK || !launch) return rc;
  if ((rc = qk_norm_check_rest(a)) != RFA_OK) return rc;
  if ((rc = qk_norm_check_map(a, &p)) != RFA_OK) return rc;
  return launch_qknorm_fwd(p, a->dtype, a->table_dtype == RFA_ROTARY_TABLE_F32, a->weight_dtype == RFA_QK_NORM_WEIGHT_F32,
                           (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

int64_t rfa_qk_norm_rotary_bwd_workspace_bytes(const rfa_qk_norm_rotary_bwd_args* a) {
  QkNormParams p{};
  bool launch = false;
  if (qk_norm_check(a, 0, &p, &launch) != RFA_OK) return 0;
  return qknorm_workspace_bytes(1, p.nparts[0] + p.nparts[1], p.g.D);
}

int rfa_qk_norm_rotary_bwd(const rfa_qk_norm_rotary_bwd_args* a, void* stream) {
  QkNormParams p{};
  bool launch = false;
  int rc = qk_norm_check(a, 1, &p, &launch);
  if (rc != RFA_OK || !launch) return rc;
  bool any = false;
  for (int k = 0; k < a->ntensors; ++k) {
    if (!a->g[k].dout) return RFA_ERR_NULL;
    any = any || a->dweight[k] != nullptr;
  }
  if (any && !a->workspace) return RFA_ERR_NULL;
  if ((rc = qk_norm_check_rest(a)) != RFA_OK) return rc;
  for (int k = 0; k < a->ntensors; ++k) {
    const rfa_qk_norm_grad& g = a->g[k];
    if (!aligned16(g.dout) || (g.dout_batch % 8) || (g.dout_row % 8) || (g.dout_head % 8)) return RFA_ERR_ALIGN;
    if (a->dweight[k] && ((uintptr_t)a->dweight[k] % 4) != 0) return RFA_ERR_ALIGN;
  }
  if (any && !aligned16(a->workspace)) return RFA_ERR_ALIGN;
  if ((rc = qk_norm_check_map(a, &p)) != RFA_OK) return rc;
  for (int k = 0; k < a->ntensors; ++k) {
    if (a->t[k].dst == a->g[k].dout) return RFA_ERR_ARGS;
    p.dout[k] = a->g[k].dout;
    p.t[k].gb = a->g[k].dout_batch; p.t[k].gr = a->g[k].dout_row; p.t[k].gh = a->g[k].dout_head;
    p.dweight[k] = a->dweight[k];
  }
  if (any && a->workspace_bytes < qknorm_workspace_bytes(1, p.nparts[0] + p.nparts[1], p.g.D)) return RFA_ERR_ARGS;
  p.workspace = (float*)a->workspace;
  return launch_qknorm_bwd(p, a->dtype, a->table_dtype == RFA_ROTARY_TABLE_F32, a->weight_dtype == RFA_QK_NORM_WEIGHT_F32,
                           (hipStream_t)stream) ? RFA_ERR_LAUNCH : RFA_OK;
}

// ---- per-head max attention logit (rfa.h; csrc/rfa_maxlogit.hip) ------------------------------------------------------------
// everything that needs no tensor pointer, in the header's order; *nqblk = blocks of 256 query rows per batch entry
static int max_logit_check(const rfa_max_logit_args* a, int* nqblk) {
  if (!a) return RFA_ERR_NULL;
  if (a->struct_bytes != sizeof(rfa_max_logit_args) || a->reserved != 0) return RFA_ERR_ARGS;
  if (a->q_half < RFA_HALF_FULL || a->q_half > RFA_HALF_BACK || a->k_half < RFA_HALF_FULL || a->k_half > RFA_HALF_BACK)
    return RFA_ERR_ARGS;
  if (a->dtype != RFA_BF16 && a->dtype != RFA_F16) return RFA_ERR_DTYPE;
  if (a->D <= 0 || a->D > kMaxHeadDim || (a->D % 8) != 0) return RFA_ERR_HEAD_DIM;
  if (a->B < 0 || a->Sq < 0 || a->Sk < 0 || a->total_q < 0) return RFA_ERR_SHAPE;
  *nqblk = (eff_len(a->Sq, a->q_half) + kMlQRows - 1) / kMlQRows;
  if ((int64_t)(a->H > 0 ? a->H : 0) * a->B * *nqblk > INT32_MAX) return RFA_ERR_SHAPE;
  if (a->H <= 0 || a->Hk <= 0 || (a->H % a->Hk) != 0) return RFA_ERR_HEADS;
  if (!(a->softmax_scale > 0.f) || !(a->softmax_scale <= FLT_MAX)) return RFA_ERR_ARGS;       // NaN, infinite, zero, negative
  if ((a->cu_seqlens_q == nullptr) != (a->cu_seqlens_k == nullptr)) return RFA_ERR_ARGS;
  if (a->mask_shift != 0 && a->cu_seqlens_q != nullptr) return RFA_ERR_ARGS;
  const int64_t n = a->mask_shift_lens < 0 ? -(int64_t)a->mask_shift_lens : (int64_t)a->mask_shift_lens;
  if (n * (int64_t)a->Sk >= ((int64_t)1 << 30)) return RFA_ERR_ARGS;
  return RFA_OK;
}

int64_t rfa_max_logit_workspace_bytes(const rfa_max_logit_args* a) {
  int nqblk = 0;
  if (max_logit_check(a, &nqblk) || a->Sk == 0) return 0;
  return (int64_t)a->H * a->B * nqblk * (int64_t)sizeof(float);
}

int rfa_max_logit(const rfa_max_logit_args* a0, void* stream) {
  int nqblk = 0;
  if (int rc = max_logit_check(a0, &nqblk)) return rc;
  const int64_t need = rfa_max_logit_workspace_bytes(a0);
  if (a0->workspace_bytes < need) return RFA_ERR_ARGS;
  if (!a0->max_logit) return RFA_ERR_NULL;
  const rfa_max_logit_args a = fold_lens(*a0);
  MaxLogitParams p{};
  p.dst = a.max_logit; p.H = a.H; p.scale = a.softmax_scale; p.accumulate = a.accumulate ? 1 : 0;
  // nothing to look at — no rows, no keys, or a dense band no element of the block lies in: -inf, no attention launch
  bool attention = need > 0;
  Band band{a.causal ? 1 : 0, a.window ? 1 : 0, a.window_left, a.window_right, 0, false};
  if (attention && a.cu_seqlens_q == nullptr) {
    band = norm_band(a.Sq, a.q_half, a.Sk, a.k_half, a.causal, a.window, a.window_left, a.window_right, a.mask_shift);
    if (band.empty || dense_len(a.Sq, a.q_half) <= 0 || dense_len(a.Sk, a.k_half) <= 0) attention = false;
  }
  if (attention && (!row_ok(a.q_st, a.D, 2) || !row_ok(a.k_st, a.D, 2))) return RFA_ERR_ARGS;   // (before any launch)
  if (!attention) return launch_status(launch_max_logit(p, a.dtype, false, (hipStream_t)stream));
  if (!a.q || !a.k || !a.workspace) return RFA_ERR_NULL;
  if (!aligned16(a.q) || !aligned16(a.k) || !aligned16(a.workspace) || !stride_ok(a.q_st, 2) || !stride_ok(a.k_st, 2))
    return RFA_ERR_ALIGN;
  p.q = a.q; p.k = a.k; p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k;
  p.q_st = cv(a.q_st); p.k_st = cv(a.k_st);
  p.B = a.B; p.Hk = a.Hk; p.D = a.D; p.Sq = a.Sq; p.Sk = a.Sk;
  p.q_half = a.q_half; p.k_half = a.k_half;
  p.wl = (band.window && band.wl >= 0) ? band.wl : -1;
  p.wr = band.causal ? 0 : ((band.window && band.wr >= 0) ? band.wr : -1);
  const bool banded = p.wl >= 0 || p.wr >= 0;
  p.shift = banded ? band.shift : 0;                             // (packed input: 0 — an absolute shift is refused above)
  p.shift_lens = banded ? a.mask_shift_lens : 0;                 // (dense input: folded into the shift)
  p.nqblk = nqblk;
  p.partial = (float*)a.workspace;
  return launch_status(launch_max_logit(p, a.dtype, true, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
