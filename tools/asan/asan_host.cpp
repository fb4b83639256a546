// asan_host.cpp — AddressSanitizer driver for libgmcmc's host code (SURVEY.md
// section 5: ASan/UBSan builds of the C++ host). Runs without a GPU: every
// call below either validates its arguments or parses host memory before it
// would touch the device, and must do so without an out-of-bounds access,
// returning GM_EINVAL (or GM_EHIP where a GPU would be needed).
//
// Built by tools/asan/Makefile against libgmcmc_asan.so (the host sources
// compiled with -Xarch_host -fsanitize=address,undefined and GM_HOST_TEST).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/gmcmc.h"

extern "C" {
gm_sampler* gm_test_sampler(int kind, int dtype, long long C, int D, int mass_mode);
void gm_test_sampler_free(gm_sampler* s);
uint64_t gm_test_state_header(gm_sampler* s, void* out);
}

static int fails = 0;
#define EXPECT(cond, what)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAIL %s (line %d)\n", what, __LINE__);    \
      ++fails;                                               \
    }                                                        \
  } while (0)

static void state_blobs() {
  std::mt19937_64 rng(7);
  // kinds: 1 HMC, 2 MH, 3 NUTS (mass 0, 1, 2)
  const int cases[][3] = {{1, 0, 0}, {2, 1, 0}, {3, 1, 0}, {3, 0, 1}, {3, 1, 2}};
  for (auto& k : cases) {
    gm_sampler* s = gm_test_sampler(k[0], k[1], 7, 5, k[2]);
    uint64_t need = 0;
    EXPECT(gm_state_size(s, &need) == GM_OK && need > 64, "state size");
    std::vector<unsigned char> blob(need);
    const uint64_t hb = gm_test_state_header(s, blob.data());
    for (uint64_t i = hb; i < need; ++i) blob[i] = (unsigned char)rng();
    // every truncation is rejected before any state is touched
    for (uint64_t len = 0; len < need; len += 1 + len / 7) {
      std::vector<unsigned char> t(blob.begin(), blob.begin() + (long)len);  // exact-size heap copy
      EXPECT(gm_state_load(s, t.empty() ? (const void*)"" : t.data(), len) == GM_EINVAL, "truncated blob");
    }
    // corrupt headers: random bit flips anywhere in the header
    for (int r = 0; r < 2000; ++r) {
      std::vector<unsigned char> t(blob);
      const int nflip = 1 + (int)(rng() % 4);
      for (int f = 0; f < nflip; ++f) t[rng() % hb] ^= (unsigned char)(1u << (rng() % 8));
      const int rc = gm_state_load(s, t.data(), t.size());
      EXPECT(rc == GM_EINVAL || rc == GM_EHIP || rc == GM_OK, "corrupt header status");
    }
    // random garbage of every small length
    for (int len = 0; len < 512; ++len) {
      std::vector<unsigned char> t((size_t)len + 1);
      for (auto& c : t) c = (unsigned char)rng();
      EXPECT(gm_state_load(s, t.data(), (uint64_t)len) == GM_EINVAL, "garbage blob");
    }
    gm_test_sampler_free(s);
  }
}

static void gauss_from_cov() {
  std::mt19937_64 rng(3);
  std::normal_distribution<double> nd;
  for (int dim = 1; dim <= 9; ++dim) {
    std::vector<double> a((size_t)dim * dim), cov((size_t)dim * dim), prec((size_t)dim * dim);
    for (auto& v : a) v = nd(rng);
    for (int i = 0; i < dim; ++i)
      for (int j = 0; j < dim; ++j) {
        double s = i == j ? 1.0 : 0.0;
        for (int k = 0; k < dim; ++k) s += a[(size_t)i * dim + k] * a[(size_t)j * dim + k];
        cov[(size_t)i * dim + j] = s;
      }
    double nc = 0;
    EXPECT(gm_gauss_from_cov(dim, cov.data(), prec.data(), &nc) == GM_OK, "spd covariance");
    cov[0] = -1.0;  // not positive definite
    EXPECT(gm_gauss_from_cov(dim, cov.data(), prec.data(), &nc) == GM_EINVAL, "non-pd covariance");
    cov[0] = 0.0 / 0.0;
    EXPECT(gm_gauss_from_cov(dim, cov.data(), prec.data(), &nc) == GM_EINVAL, "nan covariance");
  }
  double nc;
  EXPECT(gm_gauss_from_cov(0, nullptr, nullptr, &nc) == GM_EINVAL, "dim 0");
  EXPECT(gm_gauss_from_cov(3, nullptr, nullptr, &nc) == GM_EINVAL, "null cov");
}

static void argument_checks() {
  gm_target t;
  std::memset(&t, 0, sizeof(t));
  t.kind = GM_TARGET_ROSENBROCK;
  t.dim = 4;
  t.a = 1;
  t.b = 100;
  std::vector<float> x(16, 0.5f);
  gm_sampler* s = nullptr;
  EXPECT(gm_hmc_create(&t, GM_F32, 0, 4, x.data(), 0.01, 5, 0, &s) == GM_EINVAL, "zero chains");
  EXPECT(gm_hmc_create(&t, GM_F32, 4, 4, nullptr, 0.01, 5, 0, &s) == GM_EINVAL, "null init");
  EXPECT(gm_hmc_create(&t, (gm_dtype)9, 4, 4, x.data(), 0.01, 5, 0, &s) == GM_EINVAL, "bad dtype");
  EXPECT(gm_hmc_create(&t, GM_F32, 4, 5, x.data(), 0.01, 5, 0, &s) == GM_EINVAL, "dim mismatch");
  EXPECT(gm_hmc_create(&t, GM_F32, 4, 4, x.data(), 0.01, -1, 0, &s) == GM_EINVAL, "negative L");
  EXPECT(gm_nuts_create(&t, GM_F32, 4, 4, x.data(), 0.8, 99, 0, &s) == GM_EINVAL, "max_depth");
  EXPECT(gm_mh_create(&t, GM_F32, 4, 4, x.data(), -1.0, 0, &s) == GM_EINVAL, "proposal std");
  EXPECT(gm_hmc_create(&t, GM_F32, 4, 4, x.data(), 0.01, 5, (1LL << 32), &s) == GM_EINVAL, "chain offset");
  float r[4], e[4];
  EXPECT(gm_split_rhat_ess(x.data(), GM_F32, 4, 1, 4, r, e) == GM_EINVAL, "one draw");
  EXPECT(gm_split_rhat_ess(nullptr, GM_F32, 4, 4, 1, r, e) == GM_EINVAL, "null sample");
  EXPECT(gm_copy_samples(nullptr, 0, nullptr) == GM_EINVAL, "null sampler");
  EXPECT(gm_step(nullptr) == GM_EINVAL, "null step");
  EXPECT(gm_bv_add_scaled_assign(GM_F32, -1, nullptr, nullptr, 1.0) == GM_EINVAL, "bv negative n");
  EXPECT(gm_bv_dot(GM_F32, 3, nullptr, nullptr, nullptr) == GM_EINVAL, "bv dot null");
  // host-only: initial positions into an exactly sized buffer
  for (int n = 0; n < 5; ++n)
    for (int d = 0; d < 7; ++d) {
      std::vector<double> out((size_t)n * d + 0);
      EXPECT(gm_init_positions(42, n, d, GM_F64, out.empty() ? nullptr : out.data()) == GM_OK, "init");
    }
}

// The HMC warm-up entry points (gm_hmc_set_adaptation, ...): the sampler kind
// and every argument are checked before the device is touched, and a state
// blob that claims per-chain HMC state is sized before it is read.
static void hmc_adapt_checks() {
  std::vector<double> eps(7, 0.1), out(7);
  std::vector<float> m(7 * 5, 1.0f), o(7 * 5);
  for (int kind : {2, 3}) {  // MH, NUTS: not valid in this sampler's state
    gm_sampler* s = gm_test_sampler(kind, 0, 7, 5, 0);
    EXPECT(gm_hmc_set_adaptation(s, 1, 0.8, 75, 50, 25, 0.05, 1e-6) == GM_ESTATE, "adaptation on non-HMC");
    EXPECT(gm_hmc_set_step_sizes(s, eps.data()) == GM_ESTATE, "step sizes on non-HMC");
    EXPECT(gm_hmc_get_step_sizes(s, out.data(), nullptr) == GM_ESTATE, "get step sizes on non-HMC");
    EXPECT(gm_hmc_set_metric(s, m.data()) == GM_ESTATE, "metric on non-HMC");
    EXPECT(gm_hmc_get_metric(s, o.data(), nullptr) == GM_ESTATE, "get metric on non-HMC");
    gm_test_sampler_free(s);
  }
  gm_sampler* s = gm_test_sampler(1, 0, 7, 5, 0);
  EXPECT(gm_hmc_set_adaptation(nullptr, 1, 0.8, 75, 50, 25, 0.05, 1e-6) == GM_EINVAL, "null sampler");
  for (double bad : {0.0, 1.0, 0.0 / 0.0, -1.0, 2.0})
    EXPECT(gm_hmc_set_adaptation(s, 1, bad, 75, 50, 25, 0.05, 1e-6) == GM_EINVAL, "target_accept");
  EXPECT(gm_hmc_set_adaptation(s, 5, 0.8, 75, 50, 25, 0.05, 1e-6) == GM_EINVAL, "mode");
  EXPECT(gm_hmc_set_adaptation(s, 2, 0.8, -1, 50, 25, 0.05, 1e-6) == GM_EINVAL, "start_buffer");
  EXPECT(gm_hmc_set_adaptation(s, 2, 0.8, 75, 50, 25, -0.1, 1e-6) == GM_EINVAL, "regularize");
  EXPECT(gm_hmc_set_step_sizes(s, nullptr) == GM_EINVAL, "null eps");
  eps[6] = -0.1;
  EXPECT(gm_hmc_set_step_sizes(s, eps.data()) == GM_EINVAL, "negative eps");
  EXPECT(gm_hmc_set_metric(s, nullptr) == GM_EINVAL, "null metric");
  for (float bad : {0.0f, -1.0f, 0.0f / 0.0f, 1.0f / 0.0f}) {
    m[7 * 5 - 1] = bad;  // the last entry: the whole array is read, none past it
    EXPECT(gm_hmc_set_metric(s, m.data()) == GM_EINVAL, "bad metric entry");
  }
  // before any of the set calls: the creation step size and ones, no device needed
  EXPECT(gm_hmc_get_step_sizes(s, out.data(), nullptr) == GM_OK && out[6] == (double)0.01f, "default step sizes");
  EXPECT(gm_hmc_get_metric(s, o.data(), nullptr) == GM_OK && o[7 * 5 - 1] == 1.0f, "default metric");
  // a plain-sized blob whose header claims per-chain state is too short
  uint64_t need = 0;
  gm_state_size(s, &need);
  std::vector<unsigned char> blob(need, 0);
  gm_test_state_header(s, blob.data());
  const int32_t one = 1;
  std::memcpy(blob.data() + 8 + 4 + 4 + 8 + 8 + 8 + 8 + 8 + 4, &one, 4);  // StateHeader::mass_mode
  EXPECT(gm_state_load(s, blob.data(), need) == GM_EINVAL, "per-chain state flag on a plain-sized blob");
  gm_test_sampler_free(s);
}

// gm_glm_predict*: every refusal comes before the first device call; the data
// scans read exactly sized arrays to their last element (the offender is last).
static void glm_predict_checks() {
  const int64_t rows = 37, dim = 5;
  std::vector<double> x((size_t)(rows * dim), 0.25), y((size_t)rows, 1.0), off((size_t)rows, 0.5), o((size_t)rows);
  std::vector<float> th((size_t)(3 * dim), 0.1f);
  gm_glm_desc g{};
  g.family = GM_GLM_BERNOULLI_LOGIT;
  g.n_rows = rows;
  g.x = x.data();
  g.y = y.data();
  g.offset = off.data();
  gm_glm_predict_out out{};
  out.eta_mean = o.data();
  out.lppd = o.data();
  off.back() = std::numeric_limits<double>::infinity();
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 3, &out) == GM_EINVAL, "predict: offset of the last row");
  off.back() = 0.5;
  y.back() = 2.0;
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 3, &out) == GM_EINVAL, "predict: y of the last row");
  y.back() = 1.0;
  x.back() = std::numeric_limits<double>::quiet_NaN();
  EXPECT(gm_glm_predict_device(&g, dim, GM_F64, th.data(), 3, dim, &out) == GM_EINVAL, "predict: last x");
  g.y = nullptr;
  g.offset = nullptr;
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 3, &out) == GM_EINVAL, "predict: lppd without y");
  out.lppd = nullptr;
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 3, &out) == GM_EINVAL, "predict: last x, no y, no offset");
  x.back() = 0.25;
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 0, &out) == GM_EINVAL, "predict: no draws");
  EXPECT(gm_glm_predict_device(&g, dim, GM_F32, th.data(), 3, dim - 1, &out) == GM_EINVAL, "predict: stride");
  EXPECT(gm_glm_predict(&g, dim, GM_F32, th.data(), 3, nullptr) == GM_EINVAL, "predict: null out");
  EXPECT(gm_glm_predict(nullptr, dim, GM_F32, th.data(), 3, &out) == GM_EINVAL, "predict: null model");
  int32_t plan[3] = {0, 0, 0};
  EXPECT(gm_glm_predict_plan(plan, 3) == GM_OK && plan[0] > 0 && plan[2] == 16, "predict plan");
  EXPECT(gm_glm_predict_plan(plan, -1) == GM_EINVAL, "predict plan cap");
}

int main() {
  state_blobs();
  gauss_from_cov();
  argument_checks();
  hmc_adapt_checks();
  glm_predict_checks();
  std::printf("%s\n", fails ? "ASAN HOST CHECKS FAILED" : "asan host checks ok");
  return fails ? 1 : 0;
}
