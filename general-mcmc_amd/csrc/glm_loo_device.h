// glm_loo_device.h — PSIS-LOO of a GLM over stored draws (gm_glm_loo*,
// include/gmcmc.h). Not in the reference.
//
// Per data row, from the S pointwise log-likelihoods ll_s of glm_predict_main
// (same operations, same bits): lw_s = -ll_s - max(-ll), the M largest lw (the
// tail) sorted, a generalised Pareto fit to the tail (Zhang & Stephens 2009),
// the smoothed tail, and elpd_loo = logsumexp(lw + ll) - logsumexp(lw).
//
// Two kernels per group of R data rows, R a multiple of 64 that the workspace
// holds (gmcmc_loo.cpp):
//
// glm_loo_product: glm_predict_main without its moments. Four waves own 64
// rows, Theta goes through LDS 32 draws at a time, two accumulator tiles a
// wave; each ll is stored to ll[row][s] (row stride ld, a multiple of 4: in
// f32 a lane's 4 consecutive draws are one 16-byte store) and a row with a
// non-finite ll sets bad[row] (every writer stores the same 1).
//
// glm_loo_row: one workgroup of 1024 threads per row, which reads nothing but
// its own row, so nothing is shared between workgroups: no global atomics and
// no merge kernel.
//   1. MSD radix select on order-preserving unsigned keys of ll (11 bits a
//      pass in f32: 3 passes; 13 bits in f64: 5 passes): the key of ascending
//      rank M (0-based) and the count of its ties; LDS histogram, lanes of a
//      wave that hold the same digit add once. The first pass also takes the
//      minimum key (integer atomic minimum in LDS).
//   2. One more pass: keys below the threshold go to sort[0 .. M] as float64
//      lw in order of arrival (an LDS counter; the segment is sorted next and
//      equal values are interchangeable), the missing ties are filled in as
//      the threshold's lw, and every key above the threshold adds exp(lw) to
//      its thread's float64 body sum: thread t takes the elements
//      V t + 1024 V i + e in ascending order (V = 4 | 2 per 16-byte load).
//   3. Bitonic sort of the P = 2^ceil(log2(M + 1)) slots (+inf padded) in
//      global memory, one path for every M. sort[0] is the largest lw outside
//      the tail, sort[1 .. M] the tail ascending.
//   4. The fit: wave w takes the grid points w, w + 16, ...; kappa(theta) is a
//      lane-strided sum (lane l: i = l + 1, l + 65, ...) closed by the xor
//      butterfly 32, 16, ..., 1. The weights, theta-hat (thread 0, ascending
//      j), k = kappa(theta-hat) and the tail sums are thread-strided sums
//      (thread t: j = t + 1, t + 1025, ...) closed by the butterfly and then
//      the 16 wave sums in ascending order.
//   5. elpd = (llmin + A) + log((n_body exp(-A) + sum_j exp(a_j - A))
//                                / (body + sum_j exp(lw~_j))),   a_j = lw~_j - lw_j,
//      A = max(0, max_j a_j): each body term of sum exp(lw + ll) is
//      exp(llmin) up to rounding, so the body is not read again. One logarithm
//      of the quotient, not the difference of two log-sums of the size of log S.
// Every floating-point sum has a fixed order that depends on (S, M) only.
#pragma once
#include "glm_predict_device.h"

namespace gm {

constexpr int GL_THREADS = 1024;            // threads of glm_loo_row
constexpr int GL_GRID_MAX = 2048;           // theta grid points (30 + floor sqrt M) at most
constexpr long long GL_MAX_DRAWS = 1LL << 24;  // 30 + sqrt(0.2 * 2^24) = 1861 grid points
constexpr double GL_LOG_TINY = -0x1.6232bdd7abcd2p+9;  // log(DBL_MIN)

template <class T> struct GlmLooProdArgs {
  const T* x;      // [M][4 KS] zero-padded
  const T* off;    // [M]
  const T* y;      // [M]
  const T* c;      // [M]
  const T* draws;  // [S] rows of stride elements
  long long S, stride, M;
  int D, family;
  long long row0, rows;  // this group's rows
  T* ll;                 // [rows][ld]
  long long ld;
  int* bad;              // [rows], zeroed
};

template <class T, int KS> __global__ __launch_bounds__(256) void glm_loo_product(const GlmLooProdArgs<T> a) {
  using Acc = GpAcc<T>;
  T* sth = (T*)gm_dyn_lds;  // [2 tiles][KS][64], the layout of glm_predict_main
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, r = lane & 15;
  constexpr int DP = 4 * KS;
  const long long s_begin = (long long)blockIdx.x * GP_SLAB;
  const long long s_end = a.S - s_begin < GP_SLAB ? a.S : s_begin + GP_SLAB;
  const long long lrow = (long long)blockIdx.y * GP_ROWS + wave * 16 + r;
  const long long m = a.row0 + lrow;
  const bool rowok = lrow < a.rows && m < a.M;

  T xb[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xb[ks] = rowok ? a.x[m * DP + 4 * ks + q] : (T)0;
  const T off = rowok ? a.off[m] : (T)0;
  const T ym = rowok ? a.y[m] : (T)0;
  const T cm = rowok ? a.c[m] : (T)0;
  T* out = a.ll + (rowok ? lrow : 0) * a.ld;
  bool bad = false;

  for (long long s0 = s_begin; s0 < s_end; s0 += GP_STAGE) {
    __syncthreads();  // the previous stage's fragment reads are done
    for (int idx = tid; idx < GP_STAGE * DP; idx += 256) {
      const int dr = idx / DP, col = idx - dr * DP;
      const long long s = s0 + dr;
      const T v = (s < s_end && col < a.D) ? a.draws[s * a.stride + col] : (T)0;
      sth[((dr >> 4) * KS + (col >> 2)) * 64 + (col & 3) * 16 + (dr & 15)] = v;
    }
    __syncthreads();
    typename Acc::type acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[t][g] = off;
    const bool two = s0 + GP_TILE < s_end;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      acc[0] = Acc::mma(sth[ks * 64 + lane], xb[ks], acc[0]);
      if (two) acc[1] = Acc::mma(sth[(KS + ks) * 64 + lane], xb[ks], acc[1]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t == 1 && !two) break;
      T ll[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const T eta = acc[t][g];
        T mu, A;
        gp_link<T>(a.family, eta, mu, A);
        ll[g] = (ym * eta - A) + cm;
      }
      if (!rowok) continue;
      const long long sv = s0 + t * GP_TILE + 4 * q;  // f32: the lane's 4 draws are sv .. sv + 3
      if (sizeof(T) == 4 && sv + 3 < s_end) {
        *(typename Acc::type*)(out + sv) = typename Acc::type{ll[0], ll[1], ll[2], ll[3]};
#pragma unroll
        for (int g = 0; g < 4; ++g) bad |= !(ll[g] - ll[g] == (T)0);
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const long long s = s0 + t * GP_TILE + Acc::draw(q, g);
          if (s >= s_end) continue;
          out[s] = ll[g];
          bad |= !(ll[g] - ll[g] == (T)0);
        }
      }
    }
  }
  if (rowok && bad) a.bad[lrow] = 1;
}

// order-preserving unsigned keys: ll ascending = key ascending
template <class T> struct GlKey;
template <> struct GlKey<float> {
  typedef unsigned U;
  typedef gp_f32x4 Vec;
  static constexpr int KB = 32, BITS = 11, V = 4;
  static __device__ __forceinline__ U key(float v) {
    const U u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
  }
  static __device__ __forceinline__ float val(U k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct GlKey<double> {
  typedef unsigned long long U;
  typedef double Vec __attribute__((ext_vector_type(2)));
  static constexpr int KB = 64, BITS = 13, V = 2;
  static __device__ __forceinline__ U key(double v) {
    const U u = (U)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double val(U k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
  }
};

// h[d] += 1 for every active lane; up to three groups of lanes with equal d
// add once each (a row's ll crowd into a few bins of the leading digits).
// Called by whole waves.
__device__ __forceinline__ void gl_hist_add(unsigned* h, unsigned d, bool active) {
  const int lane = (int)threadIdx.x & 63;
  unsigned long long rest = __ballot(active);
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    if (rest == 0) break;
    const int leader = __ffsll((long long)rest) - 1;
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, leader);  // (leader is wave-uniform)
    const unsigned long long same = __ballot(active && d == d0) & rest;
    if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
    rest &= ~same;
  }
  if ((rest >> lane) & 1) atomicAdd(&h[d], 1u);
}

__device__ __forceinline__ double gl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
// the butterfly, then the wave sums in ascending order; called by every thread
__device__ __forceinline__ double gl_block_sum(double v, double* red) {
  v = gl_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < GL_THREADS / 64; ++w) s = s + red[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double gl_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < GL_THREADS / 64; ++w) s = red[w] > s ? red[w] : s;
  __syncthreads();
  return s;
}

template <class T> struct GlmLooRowArgs {
  const T* ll;  // [rows][ld]
  long long ld, S;
  long long M;  // tail length, M + 1 <= S
  long long P;  // slots per row of sortb and eb, a power of two >= M + 1
  const int* bad;
  double* sortb;  // [rows][P]
  double* eb;     // [rows][P]
  double* out;    // [2][rows]: elpd_loo, pareto_k
  long long rows;
};

template <class T> __global__ __launch_bounds__(GL_THREADS) void glm_loo_row(const GlmLooRowArgs<T> a) {
  using K = GlKey<T>;
  using U = typename K::U;
  static_assert((1 << K::BITS) <= 8192 && K::KB % K::BITS >= 10, "histogram sizes");
  __shared__ double sm[3 * GL_GRID_MAX];  // the histogram, then the theta grid
  __shared__ double red[GL_THREADS / 64];
  __shared__ unsigned long long sh_min;
  __shared__ long long sh_sel[3];
  __shared__ unsigned sh_cnt;
  __shared__ double sh_theta;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long rw = blockIdx.x;
  const long long S = a.S, M = a.M, P = a.P;
  const T* row = a.ll + rw * a.ld;
  double* b = a.sortb + rw * P;
  double* eb = a.eb + rw * P;
  const double qnan = __builtin_nan("");

  if (a.bad[rw]) {  // a non-finite ll in some draw
    for (long long i = tid; i <= M; i += GL_THREADS) b[i] = qnan;
    if (tid == 0) {
      a.out[rw] = qnan;
      a.out[a.rows + rw] = qnan;
    }
    return;
  }

  // 1. the key of ascending rank M and the minimum
  unsigned* hist = (unsigned*)sm;             // [<= 8192]
  unsigned* gsum = (unsigned*)(sm + 4096);    // [1024]
  U prefix = 0, pmask = 0, kmin = ~(U)0;
  long long rank = M, ceq = 0;
  if (tid == 0) {
    sh_min = ~0ull;
    sh_cnt = 0;
  }
  for (int rem = K::KB; rem > 0;) {
    const int w = rem < K::BITS ? rem : K::BITS, shift = rem - w, nb = 1 << w;
    const bool first = rem == K::KB;
    for (int i = tid; i < nb; i += GL_THREADS) hist[i] = 0;
    __syncthreads();
    for (long long base = 0; base < S; base += (long long)GL_THREADS * K::V) {
      const long long i = base + (long long)tid * K::V;
      typename K::Vec v = (T)0;
      // ld is a multiple of 4, so the load is in bounds; the last one of a row may take in the
      // padding [S, ld), which no kernel writes: those elements are masked by `in` below
      if (i < S) v = *(const typename K::Vec*)(row + i);
#pragma unroll
      for (int e = 0; e < K::V; ++e) {
        const bool in = i + e < S;
        const U k = in ? K::key(v[e]) : ~(U)0;
        if (first) kmin = k < kmin ? k : kmin;
        gl_hist_add(hist, (unsigned)((k >> shift) & (U)(nb - 1)), in && (k & pmask) == prefix);
      }
    }
    if (first) atomicMin(&sh_min, (unsigned long long)kmin);
    __syncthreads();
    const int per = nb >> 10;
    unsigned s = 0;
    for (int j = 0; j < per; ++j) s += hist[tid * per + j];
    gsum[tid] = s;
    __syncthreads();
    if (tid == 0) {
      long long acc = 0;
      int g = 0;
      for (; g < GL_THREADS - 1; ++g) {
        if (acc + gsum[g] > rank) break;
        acc += gsum[g];
      }
      int d = g * per;
      for (; d < g * per + per - 1; ++d) {
        if (acc + hist[d] > rank) break;
        acc += hist[d];
      }
      sh_sel[0] = d;
      sh_sel[1] = acc;
      sh_sel[2] = hist[d];
    }
    __syncthreads();
    prefix |= (U)sh_sel[0] << shift;
    pmask |= (U)(nb - 1) << shift;
    rank -= sh_sel[1];
    ceq = sh_sel[2];
    rem = shift;
    __syncthreads();  // before the histogram is cleared again
  }
  // `rank` ties of the threshold lie in the tail, one more is sort[0]
  const U thr = prefix;
  const double negmax = -(double)K::val((U)sh_min);  // max(-ll)
  const double llmin = (double)K::val((U)sh_min);
  const double lw_thr = (-(double)K::val(thr)) - negmax;
  const long long c_less = M - rank;

  // 2. the tail's values and the body sum
  double acc = 0.0;
  for (long long base = 0; base < S; base += (long long)GL_THREADS * K::V) {
    const long long i = base + (long long)tid * K::V;
    if (i >= S) break;
    const typename K::Vec v = *(const typename K::Vec*)(row + i);
#pragma unroll
    for (int e = 0; e < K::V; ++e) {
      if (i + e >= S) break;
      const U k = K::key(v[e]);
      const double lw = (-(double)v[e]) - negmax;
      if (k < thr) {
        const long long slot = atomicAdd(&sh_cnt, 1u);
        if (slot <= M) b[slot] = lw;
      } else if (k > thr) {
        acc = acc + ::exp(lw);
      }
    }
  }
  double body = gl_block_sum(acc, red);
  body = body + (double)(ceq - rank) * ::exp(lw_thr);
  for (long long i = c_less + tid; i < P; i += GL_THREADS) b[i] = i <= M ? lw_thr : __builtin_inf();
  __syncthreads();

  // 3. ascending bitonic sort of b[0 .. P)
  for (long long k = 2; k <= P; k <<= 1)
    for (long long j = k >> 1; j > 0; j >>= 1) {
      for (long long idx = tid; idx < (P >> 1); idx += GL_THREADS) {
        const long long lo = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), hi = lo | j;
        const double x = b[lo], y = b[hi];
        const bool up = (lo & k) == 0;
        if ((x > y) == up) {
          b[lo] = y;
          b[hi] = x;
        }
      }
      __syncthreads();
    }

  // 4. the fit
  const double cutoff = b[0] > GL_LOG_TINY ? b[0] : GL_LOG_TINY;
  const double ec = ::exp(cutoff);
  for (long long j = 1 + tid; j <= M; j += GL_THREADS) eb[j] = ::exp(b[j]);
  __syncthreads();
  const double dM = (double)M;
  double kk = __builtin_inf(), sigma = 0.0;
  bool fit = false;
  double xM = 0.0, xs = 0.0;
  if (M >= 5) {
    xM = eb[M] - ec;
    xs = eb[(long long)::floor(dM / 4.0 + 0.5)] - ec;
    fit = xM > 0.0 && xs > 0.0;
  }
  __syncthreads();  // every thread has xM and xs in registers before step 5 overwrites eb
  if (fit) {  // (the same for every thread)
    double *th = sm, *tw = sm + GL_GRID_MAX, *l = sm + 2 * GL_GRID_MAX;
    int mg = 30 + (int)::floor(::sqrt(dM));
    mg = mg > GL_GRID_MAX ? GL_GRID_MAX : mg;  // (not reached for S <= GL_MAX_DRAWS)
    for (int j = wave; j < mg; j += GL_THREADS / 64) {
      const double theta = 1.0 / xM + (1.0 - ::sqrt((double)mg / ((double)(j + 1) - 0.5))) / (3.0 * xs);
      double s = 0.0;
      for (long long i = 1 + lane; i <= M; i += 64) s = s + ::log1p(-theta * (eb[i] - ec));
      const double kap = gl_wave_sum(s) / dM;
      if (lane == 0) {
        th[j] = theta;
        l[j] = dM * ((::log(-theta / kap) - kap) - 1.0);
      }
    }
    __syncthreads();
    for (int j = tid; j < mg; j += GL_THREADS) {
      double s = 0.0;
      const double lj = l[j];
      for (int jp = 0; jp < mg; ++jp) s = s + ::exp(l[jp] - lj);
      tw[j] = th[j] * (1.0 / s);
    }
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int j = 0; j < mg; ++j) t = t + tw[j];
      sh_theta = t;
    }
    __syncthreads();
    const double that = sh_theta;
    double s = 0.0;
    for (long long i = 1 + tid; i <= M; i += GL_THREADS) s = s + ::log1p(-that * (eb[i] - ec));
    kk = gl_block_sum(s, red) / dM;
    sigma = -kk / that;
    kk = (kk * dM + 5.0) / (dM + 10.0);
  }

  // 5. the smoothed tail and the two sums
  const bool smooth = fit && kk - kk == 0.0;
  double amax = 0.0;
  for (long long j = 1 + tid; j <= M; j += GL_THREADS) {
    const double raw = b[j];
    double lwt = raw;
    if (smooth) {
      const double lp = ::log1p(-(((double)j - 0.5) / dM));
      const double qj = kk == 0.0 ? -sigma * lp : sigma * ::expm1(-kk * lp) / kk;
      const double v = ::log(qj + ec);
      lwt = v > 0.0 ? 0.0 : v;  // (a NaN stays)
    }
    eb[j] = lwt;
    const double d = lwt - raw;
    amax = d > amax ? d : amax;
  }
  const double A = gl_block_max(amax, red);
  double num = 0.0, den = 0.0;
  for (long long j = 1 + tid; j <= M; j += GL_THREADS) {
    const double lwt = eb[j];
    num = num + ::exp((lwt - b[j]) - A);
    den = den + ::exp(lwt);
  }
  num = gl_block_sum(num, red);
  den = gl_block_sum(den, red);
  if (tid == 0) {
    // one logarithm of the quotient: the two log-sums are of the size of log S, and their
    // difference would carry a rounding step of that size into an elpd_loo of any size
    a.out[rw] = (llmin + A) + ::log(((double)(S - M) * ::exp(-A) + num) / (body + den));
    a.out[a.rows + rw] = kk;
  }
}

}  // namespace gm
