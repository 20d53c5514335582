// qknormfreq_variants.hip — the tile height of the QK RMSNorm + rotary kernels that form their own angles
// (csrc/rfa_qknormfreq.hip): the kernel templates are instantiated here with other ROWS than the shipped kQkNfRows and every
// instance is timed beside the shipped one in one process.  The shipped instances of librfa_hip.so are not touched; the source
// of the tile-height table in profiles/qk_norm_freqs.md.
//
//   cd ring-flash-attention_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -I. -I../../include \
//       ../../tools/qknormfreq_variants.hip -o ../../tools/qknormfreq_variants
//   tools/qknormfreq_variants          (on the GPU)
//
// q (1, 8192, 32, 128) + k (1, 8192, 8, 128) bf16, bf16 weights, R = 128 halves, the zigzag map of rank 1 of 4; four rotating
// buffer sets; five alternating windows of 40 launches per instance, median (min .. max) in us per launch.  The backward is
// timed with both weight gradients (its partials; the fold launch, a few microseconds whatever the height, is left out).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "rfa_qknormfreq.hip"

using namespace rfa;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

enum { B = 1, S = 8192, H = 32, HK = 8, D = 128, W = 4, RANK = 1, NSETS = 4, WINDOWS = 5, CALLS = 40 };

typedef void (*Kernel)(const QkNormFreqParams);
struct Side { const char* name; Kernel kernel; uint32_t rows; bool bwd; };

template <int ROWS>
static Side fwd(const char* name) { return Side{name, qknormfreq_fwd_kernel<bf16_t, bf16_t, 0, ROWS>, ROWS, false}; }
template <int ROWS>
static Side bwd(const char* name) { return Side{name, qknormfreq_bwd_kernel<bf16_t, bf16_t, 0, ROWS>, ROWS, true}; }

int main() {
  const Side sides[] = {fwd<kQkNfRows>("forward, shipped height"), fwd<1>("forward, 1 row"), fwd<2>("forward, 2 rows"),
                        fwd<4>("forward, 4 rows"), fwd<8>("forward, 8 rows"), fwd<16>("forward, 16 rows"),
                        bwd<kQkNfRows>("backward, shipped height"), bwd<1>("backward, 1 row"), bwd<2>("backward, 2 rows"),
                        bwd<4>("backward, 4 rows"), bwd<8>("backward, 8 rows"), bwd<16>("backward, 16 rows")};
  const int nsides = sizeof(sides) / sizeof(sides[0]);
  const size_t n[2] = {(size_t)B * S * H * D, (size_t)B * S * HK * D};
  void *x[NSETS][2], *g[NSETS][2], *o[NSETS][2], *w[2];
  std::vector<uint16_t> host(n[0], 0x3f80);                    // bf16 1.0
  for (int k = 0; k < 2; ++k) {
    CK(hipMalloc(&w[k], D * 2));
    CK(hipMemcpy(w[k], host.data(), D * 2, hipMemcpyHostToDevice));
    for (int s = 0; s < NSETS; ++s) {
      CK(hipMalloc(&x[s][k], n[k] * 2));
      CK(hipMalloc(&g[s][k], n[k] * 2));
      CK(hipMalloc(&o[s][k], n[k] * 2));
      CK(hipMemcpy(x[s][k], host.data(), n[k] * 2, hipMemcpyHostToDevice));
      CK(hipMemcpy(g[s][k], host.data(), n[k] * 2, hipMemcpyHostToDevice));
    }
  }
  std::vector<float> inv(D / 2);
  for (int c = 0; c < D / 2; ++c) inv[c] = (float)std::pow(10000.0, -(double)c / (D / 2));
  float *d_inv, *d_ws, *d_dw;
  CK(hipMalloc(&d_inv, inv.size() * 4));
  CK(hipMemcpy(d_inv, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&d_ws, (size_t)2 * kQkNfMaxParts * D * 4));
  CK(hipMalloc(&d_dw, 2 * D * 4));

  QkNormFreqParams p{};
  p.g.B = B; p.g.S = S; p.g.D = D; p.g.R = D; p.g.rot_off = 0; p.g.interleaved = 0; p.g.chunks = D / 8; p.g.group = qknorm_group(D);
  for (int k = 0; k < 2; ++k) {
    QkNormTensor& t = p.t[k];
    t.H = k ? HK : H;
    t.xh = t.oh = t.gh = D;
    t.xr = t.orow = t.gr = (int64_t)t.H * D;
    t.xb = t.ob = t.gb = (int64_t)S * t.H * D;
    t.nitems = B * S * t.H;
    p.weight[k] = w[k];
    p.dweight[k] = d_dw + k * D;
  }
  p.workspace = d_ws;
  p.eps = 1e-6f; p.weight_offset = 0.f;
  p.inv_freq = d_inv; p.scaling = 1.f;
  p.pos_stride = 1;
  p.pos_split = S / 2;                                         // zigzag: blocks RANK and 2 W - 1 - RANK of S / 2 rows
  p.pos_off = (int64_t)RANK * (S / 2);
  p.pos_off2 = (int64_t)(2 * W - 1 - RANK) * (S / 2);
  p.ntensors = 2;

  auto launch = [&](const Side& sd, int i) {
    for (int k = 0; k < 2; ++k) {
      p.x[k] = x[i % NSETS][k];
      p.dout[k] = g[i % NSETS][k];
      p.out[k] = o[i % NSETS][k];
    }
    const uint32_t tiles = qknf_tiles(B, S, sd.rows);
    p.nparts = qknf_parts(tiles);
    p.walk = qknf_walk(tiles, p.nparts);
    hipLaunchKernelGGL(sd.kernel, sd.bwd ? dim3(p.nparts, 2) : dim3(tiles), dim3(kQkNfThreads), 0, 0, p);
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (const Side& sd : sides)
    for (int i = 0; i < 8; ++i) launch(sd, i);
  CK(hipDeviceSynchronize());
  std::vector<std::vector<float>> us(nsides);
  for (int win = 0; win < WINDOWS; ++win)
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
    printf("%-28s %6.1f (%.1f .. %.1f) us\n", sides[s].name, us[s][WINDOWS / 2], us[s].front(), us[s].back());
  }
  return 0;
}
