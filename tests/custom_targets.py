"""HIP sources of user targets for the CustomTarget tests: the built-in
targets restated as user code in the oracle's one-chain-per-lane arithmetic
(lanes 1, elems = dim: plain left-to-right sums), so that samples from the
runtime-compiled kernels can be compared bit for bit with the oracle."""
import numpy as np

# RosenbrockND in the select form of oracle/gm_oracle_t.inc (params: a, b)
ROSENBROCK = r"""
template <class T>
__device__ T gm_logp_grad(const T* x, T* g, const T* p) {
  const T a = p[0], b = p[1], b2 = (T)2 * b, b4 = (T)4 * b;
  T part = (T)0;
#pragma unroll
  for (int i = 0; i < GM_DIM; ++i) {
    const bool hs = i <= GM_DIM - 2, hp = i >= 1;
    const T am = a - x[i];
    const T ti = hs ? x[hs ? i + 1 : i] - x[i] * x[i] : (T)0;
    const T A = hs ? (b4 * x[i]) * ti + (T)2 * am : (T)0;
    const T B = hp ? b2 * (x[i] - x[hp ? i - 1 : i] * x[hp ? i - 1 : i]) : (T)0;
    g[i] = A - B;
    const T s = hs ? b * (ti * ti) + am * am : (T)0;
    part = (i == 0) ? s : part + s;
  }
  return -part;
}
"""

# IsotropicGaussian as a target (params: var = std*std in the sampler dtype)
ISO_GAUSS = r"""
template <class T>
__device__ T gm_logp_grad(const T* x, T* g, const T* p) {
  const T var = p[0];
  T part = (T)0;
#pragma unroll
  for (int i = 0; i < GM_DIM; ++i) {
    g[i] = (-x[i]) / var;
    const T s = x[i] * x[i];
    part = (i == 0) ? s : part + s;
  }
  return ((T)-0.5 * part) / var;
}
"""

BROKEN = r"""
template <class T>
__device__ T gm_logp_grad(const T* x, T* g, const T* p) { return undefined_symbol(x); }
"""

# The GLM target (gm.GLM) as user code, one chain per lane, every lane walking every row.
# params: [N, family (1 bernoulli_logit, 2 poisson_log), iv[D] = 1 / prior_sd^2, offset[N], y[N],
# X[N][D] row-major]. GLM walks the rows in ascending order, GLM_ROWS_DESCENDING in descending
# order: the same model and the same operations per row, another summation order, so the two
# differ by the rounding of the evaluation only (tests/test_gpu_glm.py, tools/glm_timing.py).
_GLM = r"""
__device__ inline float glm_l1p(float v) { return log1pf(v); }
__device__ inline double glm_l1p(double v) { return log1p(v); }
template <class T>
__device__ T gm_logp_grad(const T* x, T* g, const T* p) {
  const int N = (int)p[0];
  const int fam = (int)p[1];
  const T* iv = p + 2;
  const T* off = iv + GM_DIM;
  const T* y = off + N;
  const T* X = y + N;
  T lp = (T)0;
#pragma unroll
  for (int j = 0; j < GM_DIM; ++j) g[j] = (T)0;
  for (int n = 0; n < N; ++n) {
    const T* xr = X + (long long)n * GM_DIM;
    T eta = off[n];
#pragma unroll
    for (int j = 0; j < GM_DIM; ++j) eta = gm::gfma(xr[j], x[j], eta);
    T mu, A;
    if (fam == 2) {
      mu = gm::gexp(eta);
      A = mu;
    } else {
      const T ae = eta < (T)0 ? -eta : eta;
      const T em = gm::gexp(-ae);
      mu = (eta >= (T)0 ? (T)1 : em) / ((T)1 + em);
      A = (eta > (T)0 ? eta : (T)0) + glm_l1p(em);
    }
    lp = lp + (y[n] * eta - A);
    const T r = y[n] - mu;
#pragma unroll
    for (int j = 0; j < GM_DIM; ++j) g[j] = gm::gfma(xr[j], r, g[j]);
  }
#pragma unroll
  for (int j = 0; j < GM_DIM; ++j) {
    const T pv = x[j] * iv[j];
    lp = lp - ((T)0.5 * x[j]) * pv;
    g[j] = g[j] - pv;
  }
  return lp;
}
"""
_ROWS_ASC = "for (int n = 0; n < N; ++n) {"
assert _GLM.count(_ROWS_ASC) == 1
GLM = _GLM
GLM_ROWS_DESCENDING = _GLM.replace(_ROWS_ASC, "for (int n = N - 1; n >= 0; --n) {")


def glm_params(X, y, family, prior_sd, offset):
    """The params vector of GLM / GLM_ROWS_DESCENDING."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    fam = {"bernoulli_logit": 1.0, "poisson_log": 2.0}[family]
    sd = np.broadcast_to(np.asarray(prior_sd, dtype=np.float64), (D,))
    off = np.zeros(N) if offset is None else np.asarray(offset, dtype=np.float64)
    return np.concatenate([[N, fam], 1.0 / sd ** 2, off, np.asarray(y, dtype=np.float64), X.ravel()])
