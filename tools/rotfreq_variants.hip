// rotfreq_variants.hip — what each phase of the rotary kernel that forms its own angles (csrc/rfa_rotfreq.hip) costs: the kernel
// template is instantiated here WITHOUT one phase at a time (its VAR switches) and with other tile heights (ROWS), and every
// instance is timed beside the shipped one and beside the table kernel (csrc/rfa_rotary.hip, fp32 tables) in one process.  The
// shipped instances of librfa_hip.so are not touched; the source of the variant table in profiles/rotary_freqs.md.
//
//   cd ring-flash-attention_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -I. -I../../include \
//       ../../tools/rotfreq_variants.hip rfa_rotary.hip -o ../../tools/rotfreq_variants
//   tools/rotfreq_variants          (on the GPU)
//
// q (1, 8192, 32, 128) + k (1, 8192, 8, 128) bf16, R = 128 halves, out of place, the zigzag map of rank 1 of 4; six rotating
// buffer sets; five alternating windows of 40 launches per instance, median (min .. max) in us per launch.  The results of a
// variant are wrong on purpose; its addresses are the kernel's own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "rfa_rotfreq.hip"

using namespace rfa;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

enum { B = 1, S = 8192, H = 32, HK = 8, D = 128, W = 4, RANK = 1, NSETS = 6, WINDOWS = 5, CALLS = 40 };

typedef void (*Kernel)(const RotFreqParams);
struct Side { const char* name; Kernel kernel; uint32_t rows; };

template <int ROWS, int VAR>
static Side side(const char* name) { return Side{name, rotfreq_kernel<bf16_t, 0, ROWS, VAR>, ROWS}; }

int main() {
  const Side sides[] = {
      {"table kernel (rfa_rotary.hip), fp32 tables", nullptr, 0},
      side<kRotFreqRows, 0>("shipped tile height"),
      side<8, 0>("8 rows"),
      side<8, kRotFreqNoSincos>("8 rows, no sincosf"),
      side<8, kRotFreqNoBarrier>("8 rows, no barrier"),
      side<8, kRotFreqNoLdsRead>("8 rows, no LDS reads"),
      side<8, kRotFreqNoSincos | kRotFreqNoBarrier | kRotFreqNoLdsRead>("8 rows, none of the three (stream phase alone)"),
      side<16, 0>("16 rows"),
      side<4, 0>("4 rows"),
      side<2, 0>("2 rows"),
      side<2, kRotFreqNoSincos | kRotFreqNoBarrier | kRotFreqNoLdsRead>("2 rows, none of the three (stream phase alone)"),
      side<1, 0>("1 row"),
  };
  const int nsides = sizeof(sides) / sizeof(sides[0]);
  const size_t nq = (size_t)B * S * H * D, nk = (size_t)B * S * HK * D, P = (size_t)W * S;
  void *src[NSETS][2], *dst[NSETS][2];
  std::vector<uint16_t> host(nq, 0x3f80);                      // bf16 1.0
  for (int s = 0; s < NSETS; ++s)
    for (int k = 0; k < 2; ++k) {
      const size_t bytes = (k ? nk : nq) * 2;
      CK(hipMalloc(&src[s][k], bytes));
      CK(hipMalloc(&dst[s][k], bytes));
      CK(hipMemcpy(src[s][k], host.data(), bytes, hipMemcpyHostToDevice));
    }
  std::vector<float> inv(D / 2), ct(P * (D / 2)), st(P * (D / 2));
  for (int c = 0; c < D / 2; ++c) inv[c] = (float)std::pow(10000.0, -(double)c / (D / 2));
  for (size_t i = 0; i < P; ++i)
    for (int c = 0; c < D / 2; ++c) {
      ct[i * (D / 2) + c] = (float)std::cos((double)i * inv[c]);
      st[i * (D / 2) + c] = (float)std::sin((double)i * inv[c]);
    }
  float *d_inv, *d_cos, *d_sin;
  CK(hipMalloc(&d_inv, inv.size() * 4));
  CK(hipMalloc(&d_cos, ct.size() * 4));
  CK(hipMalloc(&d_sin, st.size() * 4));
  CK(hipMemcpy(d_inv, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_cos, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_sin, st.data(), st.size() * 4, hipMemcpyHostToDevice));

  RotFreqParams f{};
  RotaryParams r{};
  f.g.B = B; f.g.S = S; f.g.R = D; f.g.rot_off = 0; f.g.rot_units = D / 16; f.g.interleaved = 0;
  for (int k = 0; k < 2; ++k) {
    RotaryTensor& t = f.t[k];
    t.H = k ? HK : H;
    t.sh = t.dh = D; t.sr = t.dr = (int64_t)t.H * D; t.sb = t.db = (int64_t)S * t.H * D;
    t.uph = rotary_units_per_head(D, D, 0, false);
    t.nunits = B * S * t.H * t.uph;
    r.t[k] = t;
  }
  r.g = f.g;
  f.inv_freq = d_inv; f.scaling = 1.f;
  r.cos = d_cos; r.sin = d_sin; r.P = (int64_t)P;
  f.pos_stride = r.pos_stride = 1;
  f.pos_split = r.pos_split = S / 2;                           // zigzag: blocks RANK and 2 W - 1 - RANK of S / 2 rows
  f.pos_off = r.pos_off = (int64_t)RANK * (S / 2);
  f.pos_off2 = r.pos_off2 = (int64_t)(2 * W - 1 - RANK) * (S / 2);
  f.ntensors = r.ntensors = 2;

  auto launch = [&](const Side& sd, int i) {
    for (int k = 0; k < 2; ++k) {
      f.src[k] = r.src[k] = src[i % NSETS][k];
      f.dst[k] = r.dst[k] = dst[i % NSETS][k];
    }
    if (!sd.kernel) launch_rotary(r, 0, true, 0);
    else hipLaunchKernelGGL(sd.kernel, dim3(B * rotfreq_tiles_per_batch(S, sd.rows)), dim3(kRotFreqThreads), 0, 0, f);
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (const Side& sd : sides)
    for (int i = 0; i < 8; ++i) launch(sd, i);
  CK(hipDeviceSynchronize());
  std::vector<std::vector<float>> us(nsides);
  for (int w = 0; w < WINDOWS; ++w)
    for (int s = 0; s < nsides; ++s) {
      CK(hipEventRecord(e0, 0));
      for (int i = 0; i < CALLS; ++i) launch(sides[s], i);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      us[s].push_back(ms * 1e3f / CALLS);
    }
  CK(hipGetLastError());
  for (int s = 0; s < nsides; ++s) {
    std::sort(us[s].begin(), us[s].end());
    printf("%-52s %6.1f (%.1f .. %.1f) us\n", sides[s].name, us[s][WINDOWS / 2], us[s].front(), us[s].back());
  }
  return 0;
}
