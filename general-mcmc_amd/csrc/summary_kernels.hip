// summary_kernels.hip — device stages of the posterior summary (gm_summary.h):
// rank-normalised split-R-hat, bulk / tail ESS (Vehtari et al. 2021),
// quantiles and pooled moments. Not in the reference.
//
// Per chunk of at most SM_PC_MAX parameters (parameter q's M pooled values at
// offset q * M of every buffer; blockIdx.y = q):
//   extract_kernel    strided sample -> order-preserving unsigned keys + the
//                     element's index into Y; reads coalesced along the
//                     parameter axis, transposed through LDS
//   sort              M <= SM_LDS_MAX: lds_sort_kernel, one workgroup, bitonic
//                     on (key, idx) in LDS.  Otherwise an LSD radix sort,
//                     SM_RADIX_BITS bits per pass, three kernels per pass:
//                       hist_kernel     digit counts per block of SM_TILE
//                       rowscan_kernel, digitscan_kernel
//                                       exclusive scan, digit-major
//                       scatter_kernel  stable scatter; a wave ranks its 64
//                                       keys per round by ballot (match on
//                                       the 8 digit bits), waves and rounds
//                                       are ordered through LDS counters
//   tie_kernel        run of equal keys around every sorted position by
//                     galloping + binary search (runs may be of any length),
//                     average rank, Phi^-1, scatter to [chain][draw][q]
//   order_kernel      median, y_(k05), y_(k95), quantiles (f64 interpolation)
//   indicator_kernel  I(Y <= y_(k))      fold_kernel  keys of |Y - median|
//   moment_*          pooled mean / sd in f64, fixed summation order
#include <hip/hip_runtime.h>

#include "gm_summary.h"

namespace gm {
namespace {

// ---- keys -------------------------------------------------------------------
// value -> unsigned key with the same order; -0 is +0; bad: NaN or infinity
__device__ __forceinline__ uint32_t key_of(float v, bool& bad) {
  uint32_t u = __float_as_uint(v);
  bad = (u & 0x7f800000u) == 0x7f800000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t key_of(double v, bool& bad) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  bad = (u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
  if (u == 0x8000000000000000ull) u = 0ull;
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double val_of(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
  return (double)__uint_as_float(u);
}
__device__ __forceinline__ double val_of(uint64_t k) {
  const uint64_t u = (k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k;
  return __longlong_as_double((long long)u);
}

// element e of Y -> its [chain][draw] slot
__device__ __forceinline__ void slot_of(const SmShape& s, long long e, long long& chain, long long& draw) {
  const long long k = e / s.h, t = e - k * s.h;
  chain = k < s.C ? k : k - s.C;
  draw = k < s.C ? t : s.N - s.h + t;
}

// ---- Phi^-1 -----------------------------------------------------------------
// Acklam's rational approximation (relative error 1.15e-9) refined by two
// Halley steps on Phi(x) - p with erfc, all in f64; p > 1/2 goes through
// 1 - p, which is exact there.
__device__ double ndtri_lower(double p) {  // 0 < p <= 1/2
  const double a0 = -3.969683028665376e+01, a1 = 2.209460984245205e+02, a2 = -2.759285104469687e+02,
               a3 = 1.383577518672690e+02, a4 = -3.066479806614716e+01, a5 = 2.506628277459239e+00;
  const double b0 = -5.447609879822406e+01, b1 = 1.615858368580409e+02, b2 = -1.556989798598866e+02,
               b3 = 6.680131188771972e+01, b4 = -1.328068155288572e+01;
  const double c0 = -7.784894002430293e-03, c1 = -3.223964580411365e-01, c2 = -2.400758277161838e+00,
               c3 = -2.549732539343734e+00, c4 = 4.374664141464968e+00, c5 = 2.938163982698783e+00;
  const double d0 = 7.784695709041462e-03, d1 = 3.224671290700398e-01, d2 = 2.445134137142996e+00,
               d3 = 3.754408661907416e+00;
  double x;
  if (p < 0.02425) {
    const double q = sqrt(-2.0 * log(p));
    x = (((((c0 * q + c1) * q + c2) * q + c3) * q + c4) * q + c5) / ((((d0 * q + d1) * q + d2) * q + d3) * q + 1.0);
  } else {
    const double q = p - 0.5, r = q * q;
    x = (((((a0 * r + a1) * r + a2) * r + a3) * r + a4) * r + a5) * q /
        (((((b0 * r + b1) * r + b2) * r + b3) * r + b4) * r + 1.0);
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = 0.5 * erfc(-x * 0.70710678118654752440) - p;
    const double u = e * 2.50662827463100050242 * exp(0.5 * x * x);
    x = x - u / (1.0 + 0.5 * x * u);
  }
  return x;
}
__device__ __forceinline__ double ndtri_dev(double p) { return p <= 0.5 ? ndtri_lower(p) : -ndtri_lower(1.0 - p); }

// ---- key extraction -----------------------------------------------------------
constexpr int EX_T = 256;  // threads = elements of Y per block
template <class T, class K>
__global__ __launch_bounds__(EX_T) void extract_kernel(const T* __restrict__ x, SmShape s, long long sc,
                                                       long long sd, long long sp, long long p0, int pc,
                                                       K* __restrict__ keys, uint32_t* __restrict__ idx,
                                                       int* __restrict__ flags) {
  __shared__ T tile[SM_PC_MAX][EX_T + 1];
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * EX_T;
  // consecutive threads read consecutive parameters of one draw
  for (int i = tid; i < EX_T * pc; i += EX_T) {
    const int el = i / pc, q = i - el * pc;
    const long long e = e0 + el;
    T v = (T)0;
    if (e < s.M) {
      long long chain, draw;
      slot_of(s, e, chain, draw);
      v = x[chain * sc + draw * sd + (p0 + q) * sp];
    }
    tile[q][el] = v;
  }
  __syncthreads();
  const long long e = e0 + tid;
  if (e >= s.M) return;
  for (int q = 0; q < pc; ++q) {
    bool bad;
    const K key = key_of(tile[q][tid], bad);
    keys[(long long)q * s.M + e] = key;
    idx[(long long)q * s.M + e] = (uint32_t)e;
    if (bad) atomicOr(&flags[q], 1);
  }
}

// ---- one-workgroup sort ---------------------------------------------------------
constexpr int LS_T = 1024;
template <class K>
__global__ __launch_bounds__(LS_T) void lds_sort_kernel(const K* kin, const uint32_t* iin, K* kout, uint32_t* iout,
                                                        int M) {
  __shared__ K sk[SM_LDS_MAX];
  __shared__ uint32_t si[SM_LDS_MAX];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.y * M;
  int n2 = 64;
  while (n2 < M) n2 <<= 1;  // <= SM_LDS_MAX, a power of two
  // padding sorts last: the largest key with the largest index
  for (int i = tid; i < n2; i += LS_T) {
    sk[i] = i < M ? kin[base + i] : (K) ~(K)0;
    si[i] = i < M ? iin[base + i] : 0xffffffffu;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += LS_T) {
        const int o = i ^ j;
        if (o > i) {
          const K a = sk[i], b = sk[o];
          const uint32_t ia = si[i], ib = si[o];
          const bool gt = a > b || (a == b && ia > ib);
          if (gt == ((i & k) == 0)) {
            sk[i] = b;
            sk[o] = a;
            si[i] = ib;
            si[o] = ia;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < M; i += LS_T) {
    kout[base + i] = sk[i];
    iout[base + i] = si[i];
  }
}

// ---- global radix sort ------------------------------------------------------------
constexpr int RX_T = 256;                  // threads per block (4 waves)
constexpr int RX_W = RX_T / 64;            // waves
constexpr int RX_R = SM_TILE / RX_T;       // rounds of 64 keys per wave
constexpr int RX_D = 1 << SM_RADIX_BITS;   // digits
static_assert(RX_D == RX_T, "one thread per digit");

// hist[(q * RX_D + digit) * nb + block]
template <class K>
__global__ __launch_bounds__(RX_T) void hist_kernel(const K* __restrict__ keys, long long M, int shift,
                                                    uint32_t* __restrict__ hist, long long nb) {
  __shared__ uint32_t bins[RX_D];
  const int tid = threadIdx.x, q = blockIdx.y;
  bins[tid] = 0u;
  __syncthreads();
  const K* k = keys + (long long)q * M;
  const long long t0 = (long long)blockIdx.x * SM_TILE;
  for (int i = tid; i < SM_TILE; i += RX_T) {
    const long long e = t0 + i;
    if (e < M) atomicAdd(&bins[(unsigned)(k[e] >> shift) & (RX_D - 1)], 1u);
  }
  __syncthreads();
  hist[((long long)q * RX_D + tid) * nb + blockIdx.x] = bins[tid];
}

// The exclusive scan of a parameter's digit-major counts in two steps:
// rowscan_kernel scans each digit's row of nb block counts in place (one
// workgroup per (digit, parameter), coalesced tiles of 4 * SC_T with a carry)
// and leaves the row's total; digitscan_kernel scans the RX_D totals. A
// block's first slot for a digit is then row value + scanned total.
constexpr int SC_T = 256;
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* sums) {
  const int tid = threadIdx.x;
  sums[tid] = v;
  __syncthreads();
  for (int off = 1; off < SC_T; off <<= 1) {
    const uint32_t o = tid >= off ? sums[tid - off] : 0u;
    __syncthreads();
    sums[tid] += o;
    __syncthreads();
  }
  return sums[tid];
}
__global__ __launch_bounds__(SC_T) void rowscan_kernel(uint32_t* __restrict__ hist, long long nb,
                                                       uint32_t* __restrict__ totals) {
  __shared__ uint32_t sums[SC_T];
  const int tid = threadIdx.x;
  const long long row = (long long)blockIdx.y * RX_D + blockIdx.x;
  uint32_t* a = hist + row * nb;
  uint32_t carry = 0u;
  for (long long t0 = 0; t0 < nb; t0 += 4 * SC_T) {
    const long long i0 = t0 + 4 * tid;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + j < nb ? a[i0 + j] : 0u;
    const uint32_t s = v[0] + v[1] + v[2] + v[3];
    const uint32_t incl = block_scan_incl(s, sums);
    const uint32_t total = sums[SC_T - 1];
    uint32_t run = carry + incl - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < nb) a[i0 + j] = run;
      run += v[j];
    }
    carry += total;
    __syncthreads();  // sums is rewritten by the next tile
  }
  if (tid == 0) totals[row] = carry;
}
__global__ __launch_bounds__(SC_T) void digitscan_kernel(uint32_t* __restrict__ totals) {
  __shared__ uint32_t sums[SC_T];
  static_assert(SC_T == RX_D, "one thread per digit");
  uint32_t* t = totals + (long long)blockIdx.x * RX_D;
  const uint32_t v = t[threadIdx.x];
  t[threadIdx.x] = block_scan_incl(v, sums) - v;
}

// Wave w of a block owns the tile's keys [w * RX_R * 64, (w + 1) * RX_R * 64)
// and walks them in RX_R rounds of 64, so (wave, round, lane) is the input
// order and the scatter is stable.
template <class K>
__global__ __launch_bounds__(RX_T) void scatter_kernel(const K* __restrict__ kin, const uint32_t* __restrict__ iin,
                                                       K* __restrict__ kout, uint32_t* __restrict__ iout, long long M,
                                                       int shift, const uint32_t* __restrict__ hist,
                                                       const uint32_t* __restrict__ totals, long long nb) {
  __shared__ uint32_t wh[RX_W][RX_D];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = blockIdx.y;
  const long long pb = (long long)q * M;
  const long long w0 = (long long)blockIdx.x * SM_TILE + (long long)w * (RX_R * 64);
  for (int i = tid; i < RX_W * RX_D; i += RX_T) (&wh[0][0])[i] = 0u;
  __syncthreads();
  K key[RX_R];
#pragma unroll
  for (int r = 0; r < RX_R; ++r) {
    const long long e = w0 + r * 64 + lane;
    key[r] = e < M ? kin[pb + e] : (K)0;
    if (e < M) atomicAdd(&wh[w][(unsigned)(key[r] >> shift) & (RX_D - 1)], 1u);
  }
  __syncthreads();
  {  // a digit's first output slot for each wave of this block
    uint32_t base = hist[((long long)q * RX_D + tid) * nb + blockIdx.x] + totals[q * RX_D + tid];
#pragma unroll
    for (int v = 0; v < RX_W; ++v) {
      const uint32_t c = wh[v][tid];
      wh[v][tid] = base;
      base += c;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < RX_R; ++r) {
    const long long e = w0 + r * 64 + lane;
    const bool valid = e < M;
    const unsigned d = (unsigned)(key[r] >> shift) & (RX_D - 1);
    unsigned long long peers = __ballot(valid);  // lanes of this round with the same digit
#pragma unroll
    for (int bit = 0; bit < SM_RADIX_BITS; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below), cnt = (uint32_t)__popcll(peers);
    const uint32_t off = valid ? wh[w][d] : 0u;
    // every lane has read the counter before the run's first lane advances it
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0u) wh[w][d] = off + cnt;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const long long dst = (long long)off + rank;
    if (valid && dst < M) {
      kout[pb + dst] = key[r];
      iout[pb + dst] = iin[pb + e];
    }
  }
}

// ---- tie pass -----------------------------------------------------------------------
constexpr int EL_T = 256;
template <class K>
__global__ __launch_bounds__(EL_T) void tie_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                   SmShape s, float* __restrict__ series, double* __restrict__ ranks,
                                                   double* __restrict__ z, long long osc, long long osd) {
  const int q = blockIdx.y;
  const long long i = (long long)blockIdx.x * EL_T + threadIdx.x;
  if (i >= s.M) return;
  const K* k = keys + (long long)q * s.M;
  const K v = k[i];
  // first and last position of the run of keys equal to v: gallop away from
  // i, then bisect between the last equal and the first unequal position
  long long lo = i, hi = i;
  if (i > 0 && k[i - 1] == v) {
    long long eq = i - 1, ne = -1, step = 1;
    for (;;) {
      const long long c = eq - step;
      if (c < 0) break;
      if (k[c] == v) {
        eq = c;
        step <<= 1;
      } else {
        ne = c;
        break;
      }
    }
    while (eq - ne > 1) {
      const long long mid = ne + (eq - ne) / 2;
      if (k[mid] == v) eq = mid;
      else ne = mid;
    }
    lo = eq;
  }
  if (i + 1 < s.M && k[i + 1] == v) {
    long long eq = i + 1, ne = s.M, step = 1;
    for (;;) {
      const long long c = eq + step;
      if (c >= s.M) break;
      if (k[c] == v) {
        eq = c;
        step <<= 1;
      } else {
        ne = c;
        break;
      }
    }
    while (ne - eq > 1) {
      const long long mid = eq + (ne - eq) / 2;
      if (k[mid] == v) eq = mid;
      else ne = mid;
    }
    hi = eq;
  }
  const double r = 0.5 * (double)(lo + hi + 2);  // mean of the 1-based positions lo+1 .. hi+1
  const double zz = ndtri_dev((r - 0.375) / ((double)s.M + 0.25));
  const long long e = (long long)idx[(long long)q * s.M + i];
  if (e >= s.M) return;  // never an index outside Y, whatever the sort left
  long long chain, draw;
  slot_of(s, e, chain, draw);
  const long long o = chain * osc + draw * osd + q;
  if (series) series[o] = (float)zz;
  if (ranks) ranks[o] = r;
  if (z) z[o] = zz;
}

// ---- order statistics -----------------------------------------------------------------
template <class K>
__global__ void order_kernel(const K* __restrict__ keys, long long M, long long k05, long long k95, int n_probs,
                             const double* __restrict__ probs, double* __restrict__ ostat,
                             double* __restrict__ quant, long long qstride, int* __restrict__ flags) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const K* k = keys + (long long)q * M;
  if (tid < n_probs) {
    const double pos = (double)(M - 1) * probs[tid];
    long long lo = (long long)floor(pos);
    if (lo > M - 1) lo = M - 1;
    const long long hi = lo + 1 < M ? lo + 1 : M - 1;
    const double g = pos - (double)lo;
    const double a = val_of(k[lo]), b = val_of(k[hi]), d = b - a;
    quant[(long long)tid * qstride + q] = g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
  }
  if (tid == 32) {
    ostat[q * 3 + 0] = (M & 1) ? val_of(k[M / 2]) : (val_of(k[M / 2 - 1]) + val_of(k[M / 2])) / 2.0;
    ostat[q * 3 + 1] = val_of(k[k05]);
    ostat[q * 3 + 2] = val_of(k[k95]);
    if (k[0] == k[M - 1]) atomicOr(&flags[q], 2);
  }
}

template <class K>
__global__ __launch_bounds__(EL_T) void indicator_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                         SmShape s, long long kq, float* __restrict__ series,
                                                         long long osc, long long osd) {
  const int q = blockIdx.y;
  const long long i = (long long)blockIdx.x * EL_T + threadIdx.x;
  if (i >= s.M) return;
  const K* k = keys + (long long)q * s.M;
  const long long e = (long long)idx[(long long)q * s.M + i];
  if (e >= s.M) return;
  long long chain, draw;
  slot_of(s, e, chain, draw);
  series[chain * osc + draw * osd + q] = k[i] <= k[kq] ? 1.0f : 0.0f;
}

template <class K>
__global__ __launch_bounds__(EL_T) void fold_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                    long long M, const double* __restrict__ ostat,
                                                    uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  const int q = blockIdx.y;
  const long long i = (long long)blockIdx.x * EL_T + threadIdx.x;
  if (i >= M) return;
  const long long o = (long long)q * M + i;
  bool bad;
  keys_out[o] = key_of(fabs(val_of(keys[o]) - ostat[q * 3]), bad);
  idx_out[o] = idx[o];
}

// ---- pooled moments ---------------------------------------------------------------------
// Draws are numbered r = draw * C + chain; block b sums rows [b, b + 1) *
// SM_MOM_ROWS, thread (q = tid % 16, tid / 16) every 16th of them, then a
// fixed tree: the order depends on (C, N) only. mean == null: sums of x;
// otherwise sums of (x - mean[q])^2.
constexpr int MO_T = 256;
template <class T>
__global__ __launch_bounds__(MO_T) void moment_partial_kernel(const T* __restrict__ x, long long C, long long N,
                                                              long long sc, long long sd, long long sp, long long p0,
                                                              int pc, const double* __restrict__ mean,
                                                              double* __restrict__ part) {
  __shared__ double red[MO_T];
  const int tid = threadIdx.x, q = tid & 15, rr = tid >> 4;
  const long long r0 = (long long)blockIdx.x * SM_MOM_ROWS;
  const long long r1 = r0 + SM_MOM_ROWS < C * N ? r0 + SM_MOM_ROWS : C * N;
  double s = 0.0;
  if (q < pc) {
    const double m = mean ? mean[q] : 0.0;
    for (long long r = r0 + rr; r < r1; r += 16) {
      const long long t = r / C, c = r - t * C;
      const double v = (double)x[c * sc + t * sd + (p0 + q) * sp];
      if (mean) s += (v - m) * (v - m);
      else s += v;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int w = MO_T / 2; w >= 16; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid < 16) part[(long long)blockIdx.x * 16 + tid] = red[tid];
}
__global__ __launch_bounds__(MO_T) void moment_final_kernel(const double* __restrict__ part, long long nblk,
                                                            double n, int sdev, double* __restrict__ out) {
  __shared__ double red[MO_T];
  const int tid = threadIdx.x, q = blockIdx.x;
  double s = 0.0;
  for (long long b = tid; b < nblk; b += MO_T) s += part[b * 16 + q];
  red[tid] = s;
  __syncthreads();
  for (int w = MO_T / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[q] = sdev ? sqrt(red[0] / (n - 1.0)) : red[0] / n;
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return GM_OK;
  set_error(std::string("posterior summary: ") + what + " kernel failed: " + hipGetErrorString(e));
  return GM_EHIP;
}
inline dim3 el_grid(long long M, int pc) { return dim3((unsigned)((M + EL_T - 1) / EL_T), (unsigned)pc); }

template <class K>
int sort_t(K* ka, K* kb, uint32_t* ia, uint32_t* ib, uint32_t* hist, long long M, int pc, hipStream_t st) {
  if (M <= SM_LDS_MAX) {
    hipLaunchKernelGGL(lds_sort_kernel<K>, dim3(1, (unsigned)pc), dim3(LS_T), 0, st, (const K*)ka,
                       (const uint32_t*)ia, ka, ia, (int)M);
    return launched("one-workgroup sort");
  }
  const long long nb = (M + SM_TILE - 1) / SM_TILE;
  const dim3 grid((unsigned)nb, (unsigned)pc);
  uint32_t* totals = hist + (size_t)pc * RX_D * nb;  // [pc][RX_D], behind the pc parameters' counts
  for (int shift = 0; shift < (int)sizeof(K) * 8; shift += SM_RADIX_BITS) {
    hipLaunchKernelGGL(hist_kernel<K>, grid, dim3(RX_T), 0, st, (const K*)ka, M, shift, hist, nb);
    hipLaunchKernelGGL(rowscan_kernel, dim3(RX_D, (unsigned)pc), dim3(SC_T), 0, st, hist, nb, totals);
    hipLaunchKernelGGL(digitscan_kernel, dim3((unsigned)pc), dim3(SC_T), 0, st, totals);
    hipLaunchKernelGGL(scatter_kernel<K>, grid, dim3(RX_T), 0, st, (const K*)ka, (const uint32_t*)ia, kb, ib, M,
                       shift, (const uint32_t*)hist, (const uint32_t*)totals, nb);
    int rc = launched("radix sort");
    if (rc) return rc;
    K* tk = ka;
    ka = kb;
    kb = tk;
    uint32_t* ti = ia;
    ia = ib;
    ib = ti;
  }
  // sizeof(K) passes: an even number, so the result is back in the caller's (ka, ia)
  static_assert((sizeof(K) * 8 / SM_RADIX_BITS) % 2 == 0, "an even number of passes");
  return GM_OK;
}

}  // namespace

int sm_extract(gm_dtype dt, const void* x, SmShape s, long long sc, long long sd, long long sp, long long p0, int pc,
               void* keys, uint32_t* idx, int* flags, hipStream_t st) {
  const dim3 grid((unsigned)((s.M + EX_T - 1) / EX_T));
  if (dt == GM_F32)
    hipLaunchKernelGGL((extract_kernel<float, uint32_t>), grid, dim3(EX_T), 0, st, (const float*)x, s, sc, sd, sp, p0,
                       pc, (uint32_t*)keys, idx, flags);
  else
    hipLaunchKernelGGL((extract_kernel<double, uint64_t>), grid, dim3(EX_T), 0, st, (const double*)x, s, sc, sd, sp,
                       p0, pc, (uint64_t*)keys, idx, flags);
  return launched("key extraction");
}

size_t sm_hist_words(long long M) {
  return M <= SM_LDS_MAX ? 0 : (size_t)RX_D * (size_t)((M + SM_TILE - 1) / SM_TILE + 1);
}

int sm_sort(int kb, void* ka, void* kb_, uint32_t* ia, uint32_t* ib, uint32_t* hist, long long M, int pc,
            hipStream_t st) {
  return kb == 4 ? sort_t((uint32_t*)ka, (uint32_t*)kb_, ia, ib, hist, M, pc, st)
                 : sort_t((uint64_t*)ka, (uint64_t*)kb_, ia, ib, hist, M, pc, st);
}

int sm_tie(int kb, const void* keys, const uint32_t* idx, SmShape s, int pc, float* series, double* ranks, double* z,
           long long osc, long long osd, hipStream_t st) {
  if (kb == 4)
    hipLaunchKernelGGL(tie_kernel<uint32_t>, el_grid(s.M, pc), dim3(EL_T), 0, st, (const uint32_t*)keys, idx, s,
                       series, ranks, z, osc, osd);
  else
    hipLaunchKernelGGL(tie_kernel<uint64_t>, el_grid(s.M, pc), dim3(EL_T), 0, st, (const uint64_t*)keys, idx, s,
                       series, ranks, z, osc, osd);
  return launched("tie pass");
}

int sm_order(int kb, const void* keys, long long M, int pc, long long k05, long long k95, int n_probs,
             const double* probs, double* ostat, double* quant, long long qstride, int* flags, hipStream_t st) {
  if (kb == 4)
    hipLaunchKernelGGL(order_kernel<uint32_t>, dim3((unsigned)pc), dim3(64), 0, st, (const uint32_t*)keys, M, k05,
                       k95, n_probs, probs, ostat, quant, qstride, flags);
  else
    hipLaunchKernelGGL(order_kernel<uint64_t>, dim3((unsigned)pc), dim3(64), 0, st, (const uint64_t*)keys, M, k05,
                       k95, n_probs, probs, ostat, quant, qstride, flags);
  return launched("order statistics");
}

int sm_indicator(int kb, const void* keys, const uint32_t* idx, SmShape s, int pc, long long k, float* series,
                 hipStream_t st) {
  const long long osc = s.N * pc, osd = pc;
  if (kb == 4)
    hipLaunchKernelGGL(indicator_kernel<uint32_t>, el_grid(s.M, pc), dim3(EL_T), 0, st, (const uint32_t*)keys, idx, s,
                       k, series, osc, osd);
  else
    hipLaunchKernelGGL(indicator_kernel<uint64_t>, el_grid(s.M, pc), dim3(EL_T), 0, st, (const uint64_t*)keys, idx, s,
                       k, series, osc, osd);
  return launched("indicator");
}

int sm_fold(int kb, const void* keys, const uint32_t* idx, long long M, int pc, const double* ostat, void* keys_out,
            uint32_t* idx_out, hipStream_t st) {
  if (kb == 4)
    hipLaunchKernelGGL(fold_kernel<uint32_t>, el_grid(M, pc), dim3(EL_T), 0, st, (const uint32_t*)keys, idx, M, ostat,
                       (uint64_t*)keys_out, idx_out);
  else
    hipLaunchKernelGGL(fold_kernel<uint64_t>, el_grid(M, pc), dim3(EL_T), 0, st, (const uint64_t*)keys, idx, M, ostat,
                       (uint64_t*)keys_out, idx_out);
  return launched("fold");
}

size_t sm_moment_words(long long C, long long N) { return (size_t)((C * N + SM_MOM_ROWS - 1) / SM_MOM_ROWS) * 16; }

int sm_moments(gm_dtype dt, const void* x, long long C, long long N, long long sc, long long sd, long long sp,
               long long p0, int pc, double* part, double* mean, double* sdev, hipStream_t st) {
  const long long nblk = (C * N + SM_MOM_ROWS - 1) / SM_MOM_ROWS;
  for (int pass = 0; pass < 2; ++pass) {
    const double* m = pass ? mean : nullptr;
    if (dt == GM_F32)
      hipLaunchKernelGGL(moment_partial_kernel<float>, dim3((unsigned)nblk), dim3(MO_T), 0, st, (const float*)x, C, N,
                         sc, sd, sp, p0, pc, m, part);
    else
      hipLaunchKernelGGL(moment_partial_kernel<double>, dim3((unsigned)nblk), dim3(MO_T), 0, st, (const double*)x, C,
                         N, sc, sd, sp, p0, pc, m, part);
    hipLaunchKernelGGL(moment_final_kernel, dim3((unsigned)pc), dim3(MO_T), 0, st, (const double*)part, nblk,
                       (double)(C * N), pass, pass ? sdev : mean);
    int rc = launched("moments");
    if (rc) return rc;
  }
  return GM_OK;
}

}  // namespace gm
