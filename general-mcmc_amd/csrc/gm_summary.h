// gm_summary.h — stages of the device posterior summary (summary_kernels.hip):
// key extraction, the segmented (key, index) sort, the tie pass with the
// normal scores, order statistics, fold / indicator series and the pooled
// moments. gmcmc_summary.cpp chains them per chunk of parameters.
#pragma once
#include "gm_internal.h"

namespace gm {

// The sort's sizes (gm_summary_sort_plan reads them back for the tests).
constexpr int SM_LDS_MAX = 4096;   // largest M sorted by one workgroup in LDS
constexpr int SM_TILE = 4096;      // elements per block of the global radix path
constexpr int SM_RADIX_BITS = 8;   // bits per radix pass
constexpr int SM_PC_MAX = 16;      // parameters per chunk, at most
constexpr int SM_MOM_ROWS = 4096;  // draws per block of the moment partial sums

// The split of a [C][N] series into Y[2C][h] and the pooled count.
struct SmShape {
  long long C, N, M;
  int h;
};

// All buffers below hold a chunk of pc parameters, parameter q at offset q * M
// (keys, indices). Keys are order-preserving unsigned images of the values:
// kb = 4 (f32 sample) or 8 (f64 sample, folded values) bytes each.

// Y of parameters [p0, p0 + pc) of the strided sample -> keys, idx = the
// element's index into Y (k * h + t); flags[q] |= 1 on a non-finite value.
int sm_extract(gm_dtype dt, const void* x, SmShape s, long long sc, long long sd, long long sp,
               long long p0, int pc, void* keys, uint32_t* idx, int* flags, hipStream_t st);
// Sorts every parameter's (key, idx) pairs by key; the result is in (ka, ia),
// (kb_, ib) and hist are scratch. hist: sm_hist_words(M) u32 per parameter.
size_t sm_hist_words(long long M);
int sm_sort(int kb, void* ka, void* kb_, uint32_t* ia, uint32_t* ib, uint32_t* hist, long long M, int pc,
            hipStream_t st);
// Average rank of every run of equal keys and its normal score, scattered to
// the element's [chain][draw] slot: out[chain * osc + draw * osd + q]. series
// (f32 z, for diag_series) and ranks / z (f64) may each be null.
int sm_tie(int kb, const void* keys, const uint32_t* idx, SmShape s, int pc, float* series, double* ranks,
           double* z, long long osc, long long osd, hipStream_t st);
// Order statistics of the sorted keys: ostat[q] = {median, y_(k05), y_(k95)}
// as f64, flags[q] |= 2 when all pooled values are equal, and
// quant[j * qstride + q] = the probs[j] quantile (probs on the device).
int sm_order(int kb, const void* keys, long long M, int pc, long long k05, long long k95, int n_probs,
             const double* probs, double* ostat, double* quant, long long qstride, int* flags,
             hipStream_t st);
// series[slot of element] = (key <= key of order statistic k) ? 1 : 0
int sm_indicator(int kb, const void* keys, const uint32_t* idx, SmShape s, int pc, long long k, float* series,
                 hipStream_t st);
// (8-byte key of |value - median|, idx) from the sorted (keys, idx)
int sm_fold(int kb, const void* keys, const uint32_t* idx, long long M, int pc, const double* ostat,
            void* keys_out, uint32_t* idx_out, hipStream_t st);
// Pooled mean and ddof = 1 standard deviation over all C * N draws, in f64,
// summed in a fixed order that depends on (C, N) only. part: scratch of
// sm_moment_words(C, N) doubles.
size_t sm_moment_words(long long C, long long N);
int sm_moments(gm_dtype dt, const void* x, long long C, long long N, long long sc, long long sd, long long sp,
               long long p0, int pc, double* part, double* mean, double* sdev, hipStream_t st);

}  // namespace gm
