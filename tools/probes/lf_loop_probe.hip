// Where the time of hmc_kernel's leapfrog loop goes at one chain per wave
// (64 lanes x 1, f32 Rosenbrock): the kernel's own 9-VALU body (hmc_device.h
// lf(): gfma kick, gfma drift, RosenbrockLane<float,1>::eval64<false>, gfma
// kick) under different loop forms, at 2, 4 and 7 waves per SIMD. A launch
// runs TR "transitions" of L = 50 leapfrogs each, as the kernel does: L - 1 in
// the loop form under test and one more after it (the place of the kernel's
// last leapfrog). Prints cycles per wave-leapfrog (clock64() around the whole
// run, mean over waves), the clock (against wall_clock64()) and ns per
// wave-leapfrog slot (events), with a checksum of the end state: every
// variant but the no-DPP ones computes the same numbers. With the argument
// "spread" every launch requests as much unused LDS per block as lets a CU
// take exactly w blocks.
//
//   x1 x2 x4      the kernel's loop forms (for (; l + U < L; l += U))
//   cd5 .. cd49   count-down trip loop of U straight-line leapfrogs after
//                 (L - 1) % U single ones
//   sl49          49 leapfrogs straight-line, no branch inside a transition
//   nd1 nd2 nd4   x1 x2 x4 with the two DPP-fed subtracts reading in-lane
//                 values (wrong numbers: bounds the cost of the lane shifts)
//   The same forms on a hand-placed body (inline assembly; VALU, DPP and
//   s_nop only), which fixes the instruction order and the encodings:
//   h2-*   the compiler's encodings (v_fmac_f32, VOP2, for the kicks, the
//          drift and the gradient's last fma; 52 bytes per leapfrog), with
//          x^2, ONE wait state, then the two DPP-fed subtracts: the least the
//          DPP read-after-write hazard allows (the body is one dependency
//          chain: nothing of the same leapfrog is free to fill the state, and
//          the second half-kick cannot sink below the drift, which reads it)
//   h2n-*  h2 with two wait states (s_nop 1), what the compiler emits in
//          straight-line code (it counts the subtract's plain operand too)
//   h3-*   h2 with v_fma_f32 (VOP3, 8 bytes) for every fma: 68 bytes per
//          leapfrog, the code-size question asked in the other direction
//
// hipcc --offload-arch=gfx950 -O3 -std=c++20 -ffp-contract=off -fno-slp-vectorize \
//   tools/probes/lf_loop_probe.hip -o lf_loop_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../general-mcmc_amd/csrc/gm_device.h"

using namespace gm;

enum Body { CXX = 0, NODPP = 1, H3 = 2, H2 = 3, H2N = 4 };
enum Form { UP = 0, DOWN = 1, STRAIGHT = 2 };

#define LF_DPP_T "v_sub_f32_dpp %[t], %[q], %[xx] wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n"
#define LF_DPP_TP "v_subrev_f32_dpp %[tp], %[xx], %[q] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n"
#define LF_OPERANDS                                                                                    \
  : [p] "+v"(p), [q] "+v"(q), [g] "+v"(g), [xx] "=&v"(xx), [t] "=&v"(t), [tp] "=&v"(tp)                \
  : [half] "v"(half), [eps] "v"(eps), [b4m] "v"(tl.b4m[0]), [nc2m] "v"(tl.nc2m[0]), [nb2m] "v"(tl.nb2m[0]), \
    [cam] "v"(tl.cam[0])

template <int B>
__device__ __forceinline__ void leapfrog(const RosenbrockLane<float, 1>& tl, float& p, float& q, float& g, float half,
                                         float eps) {
  if constexpr (B == CXX) {
    // hmc_device.h lf(), E = 1
    float q1[1] = {q}, g1[1] = {g};
    p = gfma(g1[0], half, p);
    q1[0] = gfma(p, eps, q1[0]);
    tl.template eval64<false>(q1, g1);
    p = gfma(g1[0], half, p);
    q = q1[0];
    g = g1[0];
  } else if constexpr (B == NODPP) {
    // eval64_core with nx and pxx taken from this lane (no lane shift)
    p = gfma(g, half, p);
    q = gfma(p, eps, q);
    const float xx = q * q;
    const float t = p - xx, tp = q - xx;
    g = gfma(q, gfma(tl.b4m[0], t, tl.nc2m[0]), gfma(tl.nb2m[0], tp, tl.cam[0]));
    p = gfma(g, half, p);
  } else if constexpr (B == H3) {
    float xx, t, tp;
    asm volatile(
        "v_fma_f32 %[p], %[g], %[half], %[p]\n"
        "v_fma_f32 %[q], %[p], %[eps], %[q]\n"
        "v_mul_f32 %[xx], %[q], %[q]\n"
        "s_nop 0\n" LF_DPP_T LF_DPP_TP
        "v_fma_f32 %[t], %[b4m], %[t], %[nc2m]\n"
        "v_fma_f32 %[tp], %[nb2m], %[tp], %[cam]\n"
        "v_fma_f32 %[g], %[q], %[t], %[tp]\n"
        "v_fma_f32 %[p], %[g], %[half], %[p]\n" LF_OPERANDS);
  } else {
    float xx, t, tp;
    if constexpr (B == H2)
      asm volatile(
          "v_fmac_f32 %[p], %[half], %[g]\n"
          "v_fmac_f32 %[q], %[eps], %[p]\n"
          "v_mul_f32 %[xx], %[q], %[q]\n"
          "s_nop 0\n" LF_DPP_T LF_DPP_TP
          "v_fma_f32 %[t], %[b4m], %[t], %[nc2m]\n"
          "v_fma_f32 %[g], %[nb2m], %[tp], %[cam]\n"
          "v_fmac_f32 %[g], %[q], %[t]\n"
          "v_fmac_f32 %[p], %[half], %[g]\n" LF_OPERANDS);
    else
      asm volatile(
          "v_fmac_f32 %[p], %[half], %[g]\n"
          "v_fmac_f32 %[q], %[eps], %[p]\n"
          "v_mul_f32 %[xx], %[q], %[q]\n"
          "s_nop 1\n" LF_DPP_TP LF_DPP_T
          "v_fma_f32 %[t], %[b4m], %[t], %[nc2m]\n"
          "v_fma_f32 %[g], %[nb2m], %[tp], %[cam]\n"
          "v_fmac_f32 %[g], %[q], %[t]\n"
          "v_fmac_f32 %[p], %[half], %[g]\n" LF_OPERANDS);
  }
}

template <int B, int N>
__device__ __forceinline__ void leapfrogs(const RosenbrockLane<float, 1>& tl, float& p, float& q, float& g, float half,
                                          float eps) {
  if constexpr (N > 0) {
    leapfrog<B>(tl, p, q, g, half, eps);
    leapfrogs<B, N - 1>(tl, p, q, g, half, eps);
  }
}

template <int B, int F, int U>
__global__ __launch_bounds__(256) void probe(float* out, long long* cyc, int TR, int L, double eps_) {
  const int lane = threadIdx.x & 63;
  RosenbrockT<float> tg;
  tg.a = 1.f; tg.b = 100.f; tg.b2 = 200.f; tg.b4 = 400.f; tg.D = 64;
  const auto tl = tg.template bind<64, 1>(lane);
  // eps and eps / 2 as in the kernel (HmcLaunch::eps is a double: both end up in vector registers)
  const float eps = (float)eps_;
  const float half = 0.5f * eps;
  float q = 0.9f + 0.001f * (float)lane + 1e-6f * (float)blockIdx.x, p = 0.01f * (float)((lane * 7) % 13 - 6), g = 0.f;
  {
    float q1[1] = {q}, g1[1];
    tl.template eval64<false>(q1, g1);
    g = g1[0];
  }
  const long long r0 = wall_clock64();
  const long long t0 = clock64();
  for (int tr = 0; tr < TR; ++tr) {
    int l = 0;
    if constexpr (F == UP) {
      if constexpr (U > 1)
        for (; l + U < L; l += U) leapfrogs<B, U>(tl, p, q, g, half, eps);
      for (; l + 1 < L; ++l) leapfrog<B>(tl, p, q, g, half, eps);
    } else if constexpr (F == DOWN) {
      // single steps bring L - 1 to a multiple of U, then trips of U with one
      // scalar decrement, compare and branch each
      const int n1 = L - 1;
      int trips = n1 / U;
      for (int r = n1 - trips * U; r > 0; --r) leapfrog<B>(tl, p, q, g, half, eps);
      for (; trips > 0; --trips) leapfrogs<B, U>(tl, p, q, g, half, eps);
    } else {
      leapfrogs<B, U>(tl, p, q, g, half, eps);  // U = L - 1
    }
    leapfrog<B>(tl, p, q, g, half, eps);  // the place of the last leapfrog
    // a "rejected" proposal now and then keeps the state in range
    if ((tr & 3) == 3) { q = 0.9f + 0.001f * (float)lane; p = -p; float q1[1] = {q}, g1[1]; tl.template eval64<false>(q1, g1); g = g1[0]; }
  }
  const long long t1 = clock64();
  const long long r1 = wall_clock64();
  const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  out[gt] = q + p;
  if (lane == 0) {
    cyc[2 * (gt >> 6)] = t1 - t0;
    cyc[2 * (gt >> 6) + 1] = r1 - r0;
  }
}

struct Variant {
  const char* name;
  void (*k)(float*, long long*, int, int, double);
};

#define CHECK(x)                                                                 \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

int main(int argc, char** argv) {
  // "spread": each launch asks for so much (unused) LDS per block that a CU takes exactly w blocks
  const bool spread = argc > 1 && !strcmp(argv[1], "spread");
  const int L = 50, TR = 400;  // 20,000 leapfrogs per launch
  const Variant vs[] = {
      {"x1", probe<CXX, UP, 1>},        {"x2", probe<CXX, UP, 2>},        {"x4", probe<CXX, UP, 4>},
      {"cd5", probe<CXX, DOWN, 5>},     {"cd7", probe<CXX, DOWN, 7>},     {"cd10", probe<CXX, DOWN, 10>},
      {"cd14", probe<CXX, DOWN, 14>},   {"cd49", probe<CXX, DOWN, 49>},   {"sl49", probe<CXX, STRAIGHT, 49>},
      {"nd1", probe<NODPP, UP, 1>},     {"nd2", probe<NODPP, UP, 2>},     {"nd4", probe<NODPP, UP, 4>},
      {"h2-x1", probe<H2, UP, 1>},      {"h2-x2", probe<H2, UP, 2>},      {"h2-x4", probe<H2, UP, 4>},
      {"h2-cd5", probe<H2, DOWN, 5>},   {"h2-cd7", probe<H2, DOWN, 7>},   {"h2-cd10", probe<H2, DOWN, 10>},
      {"h2-sl49", probe<H2, STRAIGHT, 49>},
      {"h2n-x2", probe<H2N, UP, 2>},    {"h2n-cd7", probe<H2N, DOWN, 7>}, {"h2n-sl49", probe<H2N, STRAIGHT, 49>},
      {"h3-x1", probe<H3, UP, 1>},      {"h3-x2", probe<H3, UP, 2>},      {"h3-x4", probe<H3, UP, 4>},
      {"h3-cd5", probe<H3, DOWN, 5>},   {"h3-cd7", probe<H3, DOWN, 7>},   {"h3-cd10", probe<H3, DOWN, 10>},
      {"h3-sl49", probe<H3, STRAIGHT, 49>},
  };
  constexpr int NV = sizeof(vs) / sizeof(vs[0]), NW = 3, ROUNDS = 7;
  const int ws[NW] = {2, 4, 7};
  int dev = 0, cus = 256;
  CHECK(hipGetDevice(&dev));
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t nthr = (size_t)cus * ws[NW - 1] * 256;
  float* out;
  long long* cyc;
  CHECK(hipMalloc(&out, nthr * sizeof(float)));
  CHECK(hipMalloc(&cyc, nthr / 64 * 2 * sizeof(long long)));
  std::vector<float> ho(nthr);
  std::vector<long long> hc(nthr / 64 * 2);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  // the rounds run every variant in turn, so that a clock that moves during
  // the run moves under all of them; a second of launches comes first
  for (int i = 0; i < 300; ++i)
    hipLaunchKernelGGL(vs[1].k, dim3(cus * 4), dim3(256), 0, 0, out, cyc, TR, L, 1e-3);
  CHECK(hipDeviceSynchronize());
  static float ms_all[NV][NW][ROUNDS];
  static double cyc_all[NV][NW][ROUNDS], ghz_all[NV][NW][ROUNDS];
  static unsigned long long sum[NV][NW];
  for (int r = 0; r < ROUNDS; ++r)
    for (int vi = 0; vi < NV; ++vi)
      for (int wi = 0; wi < NW; ++wi) {
        const int blocks = cus * ws[wi];  // 4 waves per block, one per SIMD
        const size_t n = (size_t)blocks * 256;
        const size_t lds = spread ? std::min<size_t>(64 * 1024, 160 * 1024 / ws[wi] - 2048) : 0;
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(vs[vi].k, dim3(blocks), dim3(256), lds, 0, out, cyc, TR, L, 1e-3);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms_all[vi][wi][r], e0, e1));
        CHECK(hipMemcpy(hc.data(), cyc, n / 64 * 2 * sizeof(long long), hipMemcpyDeviceToHost));
        double sc = 0, sr = 0;
        for (size_t i = 0; i < n / 64; ++i) {
          sc += (double)hc[2 * i];
          sr += (double)hc[2 * i + 1];
        }
        cyc_all[vi][wi][r] = sc / (double)(n / 64);
        ghz_all[vi][wi][r] = sr > 0 ? sc / sr * 0.1 : 0;  // the real-time counter runs at 100 MHz
        if (r == 0) {
          CHECK(hipMemcpy(ho.data(), out, 256 * sizeof(float), hipMemcpyDeviceToHost));
          unsigned long long h = 1469598103934665603ull;  // the first block's end state, as bits
          for (int i = 0; i < 256; ++i) {
            unsigned u;
            memcpy(&u, &ho[i], 4);
            h = (h ^ u) * 1099511628211ull;
          }
          sum[vi][wi] = h;
        }
      }
  printf("%d CUs, L = %d, %d transitions per launch, %d rounds over all variants; w = waves per SIMD%s\n"
         "cyc/lf: clock64() ticks a wave spends per leapfrog (mean over waves), cyc/lf/w: that over w = SIMD cycles\n"
         "per wave-leapfrog, GHz: clock64() over wall_clock64() inside the waves; ns/lf/w: event time / leapfrogs / w.\n"
         "Median over the rounds (ns: min and max too).\n",
         cus, L, TR, ROUNDS, spread ? "; LDS request that lets a CU take exactly w blocks" : "");
  printf("%-9s %2s %8s %9s %6s %9s %8s %8s  %s\n", "variant", "w", "cyc/lf", "cyc/lf/w", "GHz", "ns/lf/w", "min",
         "max", "checksum");
  const double nlf = (double)TR * L;
  for (int vi = 0; vi < NV; ++vi)
    for (int wi = 0; wi < NW; ++wi) {
      const int w = ws[wi];
      std::sort(ms_all[vi][wi], ms_all[vi][wi] + ROUNDS);
      std::sort(cyc_all[vi][wi], cyc_all[vi][wi] + ROUNDS);
      std::sort(ghz_all[vi][wi], ghz_all[vi][wi] + ROUNDS);
      const double cpl = cyc_all[vi][wi][ROUNDS / 2] / nlf, k = 1e6 / nlf / w;
      printf("%-9s %2d %8.2f %9.2f %6.2f %9.3f %8.3f %8.3f  %016llx\n", vs[vi].name, w, cpl, cpl / w,
             ghz_all[vi][wi][ROUNDS / 2], ms_all[vi][wi][ROUNDS / 2] * k, ms_all[vi][wi][0] * k,
             ms_all[vi][wi][ROUNDS - 1] * k, sum[vi][wi]);
    }
  CHECK(hipFree(out));
  CHECK(hipFree(cyc));
  return 0;
}
