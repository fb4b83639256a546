"""Helpers of tests/test_gpu_nuts_whitening.py: a dtype-faithful transcription
of the window end's Cholesky factorisation (cholesky_spd in nuts_kernels.hip),
the backward-error constant gamma_m, and the tie of a sampler's frozen
sampling phase to the CPU oracle with the metric read back from the GPU."""
import numpy as np

from tests._oracle import Target


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2.0


def gamma(m, dtype):
    """gamma_m = m u / (1 - m u) (Higham, Accuracy and Stability, Lemma 3.1)."""
    u = unit_roundoff(dtype)
    return m * u / (1.0 - m * u)


def cholesky_spd(a, dtype):
    """cholesky_spd of nuts_kernels.hip, operation by operation in `dtype`:
    row by row, sum = a_ij - l_ik l_jk with k ascending, every product and
    difference rounded on its own (no contraction). None when a pivot is
    non-positive or non-finite."""
    T = np.dtype(dtype).type
    a = np.asarray(a, dtype=dtype)
    dim = a.shape[0]
    l = np.zeros((dim, dim), dtype=dtype)
    for i in range(dim):
        for j in range(i + 1):
            s = T(a[i, j])
            for k in range(j):
                s = T(s - T(l[i, k] * l[j, k]))
            if i == j:
                if not (s > 0) or not np.isfinite(s):
                    return None
                l[i, j] = np.sqrt(s)
            else:
                d = l[j, j]
                if not (d > 0) or not np.isfinite(d):
                    return None
                l[i, j] = T(s / d)
    return l


def oracle_tie(oracle, s, target, dim, mode, n_collect, seed, init_step, chain_offset=0, max_depth=10,
               otarget=None):
    """GPU run(n_collect, 0) of sampler s against the oracle's frozen run from
    the state read back from s: positions, step sizes and every chain's metric
    as the arrays mass_matrix() returns. Samples and step sizes bit for bit.
    otarget: the oracle's Target where `target` is user code."""
    dtype = s.dtype
    n_chains = s.n_chains
    m = s.mass_matrix()
    eps, bar = s.step_sizes()
    q = s.positions()
    st = oracle.nuts_state(n_chains, dtype)
    st["eps"][:] = eps.astype(dtype)
    st["eps_bar"][:] = bar.astype(dtype)
    om = oracle.nuts_mass(mode, n_chains, dim, dtype)
    om.kind[:] = m.kind
    om.dinv[:] = m.diag_inv
    om.dsqrt[:] = m.diag_sqrt
    if mode == 2:
        om.minv[:] = m.dense_inv
        om.mchol[:] = m.dense_chol
    lanes, elems = s.layout()
    out = s.run(n_collect, 0)
    _, smp, _, _ = oracle.nuts_mass_run(otarget or Target.from_product(target, dim), q, st, om, 0.8, max_depth, seed, init_step,
                                        n_collect, 0, False, lanes, elems, chain_offset=chain_offset)
    np.testing.assert_array_equal(out, smp.transpose(1, 0, 2))
    e2, b2 = s.step_sizes()
    np.testing.assert_array_equal(e2.astype(dtype), st["eps"])
    np.testing.assert_array_equal(b2.astype(dtype), st["eps_bar"])
    return out
