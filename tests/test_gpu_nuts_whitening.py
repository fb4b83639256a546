"""NUTS whitening metric warm-up (M^-1 = Sigma_hat), per chain or pooled over
all chains (gm_nuts_set_metric_convention). The tree kernels are the
reference convention's: a whitening metric is other data in the same slots,
so the sampling phase is tied to the CPU oracle bit for bit with the metric
read back from the GPU, and the window ends are checked against the reference
convention's (same statistics) and against float64 evaluations."""
import numpy as np
import pytest

import bench
from tests import _hmc_dense_ref as href
from tests import _nuts_whiten_ref as ref
from tests.test_gpu_hmc_adapt import _same_run

gpu = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
COV3 = np.array([[2.0, 0.9, 0.0], [0.9, 1.0, 0.3], [0.0, 0.3, 0.5]])  # test_dense_warmup_bitexact's


def _cfg(gm, adaptation, sb, eb, iw, convention="whitening", pooled=False):
    return gm.NUTSMassMatrixConfig(adaptation, sb, eb, iw, 0.05, 1e-6, 75, convention, pooled)


def _rand_gauss(gm, D, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((D, D))
    cov = a @ a.T / D + 0.5 * np.eye(D)
    return gm.DenseGaussian(rng.standard_normal(D), cov)


# ---- 1. sampling under a whitening metric is the oracle's --------------------------
SHAPES = [(32, 36, (16, 2), True), (20, 10, (16, 2), True), (32, 36, (16, 2), False), (3, 16, None, True)]


@gpu
@pytest.mark.parametrize("D,chains,layout,mpass", SHAPES)
@pytest.mark.parametrize("kind", ["diag", "dense", "pooled"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_whitened_sampling_is_the_oracles(gm, oracle, dtype, kind, D, chains, layout, mpass):
    """run(1, 60) with windows 4/4/10 adapts the metric; run(25, 0) then equals
    the oracle's frozen run from the positions, step sizes and metric arrays
    read back: the kernels apply a whitening metric as they apply any."""
    if D == 3:
        t = gm.DenseGaussian(np.array([0.5, -1.0, 0.0]), COV3)
        x0 = gm.init_with_seed(chains, D, 4, dtype)
    else:
        t = _rand_gauss(gm, D, 31)
        x0 = gm.init_with_seed(chains, D, 7, np.float64).astype(dtype)
    mode = 1 if kind == "diag" else 2
    cfg = _cfg(gm, "diagonal" if kind == "diag" else "dense", 4, 4, 10, pooled=kind == "pooled")
    s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, cfg, dtype=dtype).set_seed(11)
    if layout:
        s.set_layout(*layout)
    if not mpass:
        s.set_momentum_pass(False)
    s.run(1, 60)
    m = s.mass_matrix()
    assert np.all(m.kind == mode)
    if kind == "pooled":
        assert s.metric_updates() == (4, 0)
        assert all(np.array_equal(m.dense_inv[c], m.dense_inv[0]) for c in range(chains))
    elif kind == "dense":  # M^-1 = the covariance estimate: exactly symmetric, its factor lower triangular
        np.testing.assert_array_equal(m.dense_inv, m.dense_inv.transpose(0, 2, 1))
        assert np.all(np.triu(m.dense_chol, 1) == 0)
        assert not np.array_equal(m.dense_inv[0], m.dense_inv[1])
    ref.oracle_tie(oracle, s, t, D, mode, 25, 11, 61)
    if mode == 2 and layout == (16, 2) and mpass:
        assert s.launch_plan()["frozen"] == 1
    s.close()


# ---- 2. the first window end against the reference convention ----------------------
def _first_update(gm, dtype, adaptation):
    t = gm.DenseGaussian(np.array([0.5, -1.0, 0.0]), COV3)
    x0 = gm.init_with_seed(16, 3, 4, dtype)
    out = []
    for conv in ("reference", "whitening"):
        s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, _cfg(gm, adaptation, 5, 5, 10, conv), dtype=dtype).set_seed(11)
        s.run(1, 22)  # one update, at m = 15 (the window ending at m = 16 holds one row)
        out.append(s.mass_matrix())
        s.close()
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_dense_update_against_reference_convention(gm, dtype):
    """Until the update both samplers run the identity metric on the same
    draws, so the window statistics and the jittered covariance tr are the
    same bits. Reference: mchol = chol(tr), minv = tr^-1. Whitening: minv = tr,
    mchol = chol(tr^-1), the same cholesky_spd on the same tr^-1."""
    r, w = _first_update(gm, dtype, "dense")
    assert np.all(r.kind == 2) and np.all(w.kind == 2)
    D = 3
    g = ref.gamma(2 * D + 2, dtype)
    worst = 0.0
    for c in range(16):
        want = ref.cholesky_spd(r.dense_inv[c], dtype)
        assert want is not None
        np.testing.assert_array_equal(w.dense_chol[c], want)
        L = r.dense_chol[c].astype(np.float64)
        err = np.abs(L @ L.T - w.dense_inv[c].astype(np.float64))
        bound = g * (np.abs(L) @ np.abs(L).T)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, err / bound)
    print(f"largest |L L^T - minv_w| / bound over the chains: {worst:.3e}")
    np.testing.assert_array_equal(w.dense_inv, w.dense_inv.transpose(0, 2, 1))
    assert np.all(np.triu(w.dense_chol, 1) == 0)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_diagonal_update_against_reference_convention(gm, dtype):
    r, w = _first_update(gm, dtype, "diagonal")
    assert np.all(r.kind == 1) and np.all(w.kind == 1)
    T = np.dtype(dtype).type
    np.testing.assert_array_equal(w.diag_sqrt, (T(1) / r.diag_sqrt).astype(dtype))
    u = ref.unit_roundoff(dtype)
    sq = r.diag_sqrt.astype(np.float64) ** 2
    assert np.all(np.abs(w.diag_inv.astype(np.float64) - sq) <= 2 * u * w.diag_inv.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cholesky_transcription(dtype):
    """The transcription against numpy's factorisation on the matrices of the
    3-D case: the regularised covariance and its inverse (float64 inputs
    rounded to dtype); a failed pivot is reported as None."""
    c = 0.95 * COV3 + 0.05 * np.eye(3)
    for a in (c, np.linalg.inv(c), COV3, np.linalg.inv(COV3)):
        a = (0.5 * (a + a.T)).astype(dtype)
        got = ref.cholesky_spd(a, dtype)
        want = np.linalg.cholesky(a.astype(np.float64))
        assert got.dtype == np.dtype(dtype) and np.all(np.triu(got, 1) == 0)
        # Cholesky backward error: |L L^T - A| <= gamma_{D+1} |L||L|^T
        L = got.astype(np.float64)
        assert np.all(np.abs(L @ L.T - a) <= ref.gamma(4, dtype) * (np.abs(L) @ np.abs(L).T))
        np.testing.assert_allclose(got, want, rtol=0, atol=64 * ref.unit_roundoff(dtype) * np.abs(want).max()
                                   * np.linalg.cond(a.astype(np.float64)))
    assert ref.cholesky_spd(np.array([[1.0, 2.0], [2.0, 1.0]]), dtype) is None
    assert ref.cholesky_spd(np.array([[np.nan, 0.0], [0.0, 1.0]]), dtype) is None


# ---- 2b. where the reference convention works, whitening does -------------------------
@gpu
def test_wide_layout_and_dense_max_dim(gm, oracle):
    """The diagonal whitening metric on a wide layout (one chain per
    workgroup, D = 300), and a dense request above dense_max_dim falling back
    to it: kind 1, inv = v and sqrt = 1/sqrt(v), sampling as the oracle's.
    inv * sqrt^2 = 1 within 9u: the square root within one ulp (2u) and the
    reciprocal (u) give sqrt 3u, its square 7u, the product 8u to first order."""
    dim, chains = 300, 6
    t = gm.IsotropicGaussian(1.1)
    x0 = gm.init_with_seed(chains, dim, 8, np.float64)
    cfg = gm.NUTSMassMatrixConfig("diagonal", start_buffer=4, end_buffer=4, initial_window=10, convention="whitening")
    s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, cfg, dtype=np.float64, max_depth=6).set_seed(3)
    assert s.layout()[0] > 64
    s.run(1, 40)
    m = s.mass_matrix()
    assert np.all(m.kind == 1)
    np.testing.assert_allclose(m.diag_inv * m.diag_sqrt ** 2, 1.0, rtol=0, atol=9 * ref.unit_roundoff(np.float64))
    ref.oracle_tie(oracle, s, t, dim, 1, 5, 3, 41, max_depth=6)
    s.close()
    t = _rand_gauss(gm, 6, 2)
    x0 = gm.init_with_seed(9, 6, 3, np.float32)
    cfg = gm.NUTSMassMatrixConfig("dense", 4, 4, 10, dense_max_dim=5, convention="whitening")
    s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, cfg, dtype=np.float32).set_seed(3)
    s.run(1, 40)
    m = s.mass_matrix()
    assert m.dense_inv is None and np.all(m.kind == 1)
    assert np.all(np.abs(m.diag_inv * m.diag_sqrt ** 2 - 1) <= 9 * ref.unit_roundoff(np.float32))
    ref.oracle_tie(oracle, s, t, 6, 1, 8, 3, 41)
    s.close()


@gpu
@pytest.mark.parametrize("kind", ["dense", "pooled"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_user_target(gm, oracle, dtype, kind):
    """The isotropic Gaussian as user code (runtime-compiled tree kernel,
    layout (1, dim)) under a per-chain and a pooled dense whitening metric:
    sampling as the oracle's with the built-in target's arithmetic."""
    from tests import custom_targets as ct
    from tests._oracle import Target
    dim, chains = 4, 20
    x0 = (gm.init_with_seed(chains, dim, 6, np.float64) * 0.5).astype(dtype)
    t = gm.CustomTarget(ct.ISO_GAUSS, dim, [float(dtype(1.1) * dtype(1.1))])
    cfg = _cfg(gm, "dense", 4, 4, 10, pooled=kind == "pooled")
    s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, cfg, dtype=dtype, max_depth=6).set_seed(13)
    assert s.layout() == (1, dim)
    s.run(1, 40)
    assert np.all(s.mass_matrix().kind == 2)
    if kind == "pooled":
        assert s.metric_updates() == (3, 0)  # window ends at m = 14, 24, 35
    ref.oracle_tie(oracle, s, t, dim, 2, 8, 13, 41, max_depth=6, otarget=Target(2, dim, std=1.1))
    s.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_pooled_diagonal(gm, oracle, dtype):
    """The pooled diagonal metric: until the first window end (m = 15 of
    run(1, 22)) a pooled dense sampler runs the same identity-metric
    transitions, so v is the diagonal of its Sigma_hat, bit for bit; every
    chain's copy is v and 1/sqrt(v) rounded once; sampling as the oracle's."""
    n_chains, dim = 70, 17
    t = _rand_gauss(gm, dim, 5)
    x0 = gm.init_with_seed(n_chains, dim, 22, np.float64).astype(dtype)
    res = {}
    for adaptation in ("diagonal", "dense"):
        s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, _cfg(gm, adaptation, 5, 5, 10, pooled=True), dtype=dtype)
        s.set_seed(4).run(1, 22)
        assert s.metric_updates() == (1, 0)
        res[adaptation] = s
    sigma, lp = res["diagonal"].pooled_metric()
    v = np.diag(sigma)
    np.testing.assert_array_equal(sigma, np.diag(v))
    np.testing.assert_array_equal(v, np.diag(res["dense"].pooled_metric()[0]))
    np.testing.assert_array_equal(lp, np.diag(np.diag(lp)))
    np.testing.assert_allclose(np.diag(lp), 1.0 / np.sqrt(v), rtol=4 * ref.unit_roundoff(np.float64), atol=0)
    m = res["diagonal"].mass_matrix()
    assert np.all(m.kind == 1) and m.dense_inv is None
    for c in range(n_chains):
        np.testing.assert_array_equal(m.diag_inv[c], v.astype(dtype))
        np.testing.assert_array_equal(m.diag_sqrt[c], np.diag(lp).astype(dtype))
    ref.oracle_tie(oracle, res["diagonal"], t, dim, 1, 8, 4, 23)
    for s in res.values():
        s.close()


# ---- 3. the pooled statistics ---------------------------------------------------------
POOLED = [(dt, c, d, 0.0) for dt in DTYPES for c in (1, 70, 1025) for d in (2, 17, 64)] + [
    (np.float32, 70, 17, 1e4)]


@gpu
@pytest.mark.parametrize("dtype,n_chains,dim,mean", POOLED)
def test_pooled_statistics(gm, dtype, n_chains, dim, mean):
    """One window (transitions 6..15 of a 26-transition warm-up). The
    positions of those transitions come from samplers that run the same
    warm-up without a window (start_buffer 1000) and stop after m transitions:
    the same kernel on the same draws under the identity metric, so the same
    bits. Both Sigmas are float64 sums of the same numbers; with y = x - c0 a
    sum of n products carries at most n 2^-52 sum |y_i||y_j|."""
    target = gm.DenseGaussian(np.full(dim, mean), np.eye(dim))
    x0 = (mean + gm.init_with_seed(n_chains, dim, 21, np.float64)).astype(dtype)
    reg, jitter = 0.05, 1e-6

    def make(start_buffer):
        cfg = gm.NUTSMassMatrixConfig("dense", start_buffer, 10, 10, reg, jitter, 75, "whitening", True)
        return gm.NUTS.new_with_mass_matrix(target, x0, 0.8, cfg, dtype=dtype).set_seed(17)

    a = make(5)
    a.run(1, 26)
    assert a.metric_updates() == (1, 0)
    st = href.Pooled(dim)
    rows = []
    for m in range(6, 16):
        b = make(1000)
        b.run(1, m)
        assert b.metric_updates() == (0, 0)
        rows.append(b.positions().astype(np.float64))
        st.add(rows[-1])
        b.close()
    assert len({r.tobytes() for r in rows}) >= len(rows) // 2  # the chains moved
    want = st.sigma(reg, jitter)
    y = np.abs(np.concatenate(rows) - st.c0)
    n = y.shape[0]
    bound = n * 2.0 ** -52 * (y.T @ y) / (n - 1)
    got, lp = a.pooled_metric()
    err = np.abs(got - want)
    print(f"Sigma: largest error / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound)
    np.testing.assert_array_equal(got, got.T)
    assert np.all(np.triu(lp, 1) == 0)
    np.testing.assert_allclose(lp @ lp.T @ got, np.eye(dim), rtol=0, atol=1e-9)
    mm = a.mass_matrix()
    assert np.all(mm.kind == 2)
    for c in range(n_chains):
        np.testing.assert_array_equal(mm.dense_inv[c], got.astype(dtype))
        np.testing.assert_array_equal(mm.dense_chol[c], lp.astype(dtype))
    a.close()


# ---- 4. launch splitting does not matter --------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_launch_splitting_does_not_matter(gm, dtype):
    n_chains, dim = 70, 17
    t = _rand_gauss(gm, dim, 5)
    x0 = gm.init_with_seed(n_chains, dim, 22, np.float64).astype(dtype)
    res = []
    for spl in (3, 7, 1000):
        s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, _cfg(gm, "dense", 5, 5, 10, pooled=True), dtype=dtype)
        s.set_seed(4).set_steps_per_launch(spl)
        out = s.run(10, 60)
        m = s.mass_matrix()
        res.append((out, s.positions()) + s.step_sizes() + (m.kind, m.dense_inv, m.dense_chol) + s.pooled_metric()
                   + (np.array(s.metric_updates()),))
        s.close()
    assert tuple(res[0][-1]) == (4, 0)  # window ends at m = 15, 25, 45, 54
    for other in res[1:]:
        for x, y in zip(res[0], other):
            np.testing.assert_array_equal(x, y)


# ---- 5. checkpoint ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint(gm, dtype):
    n_chains, dim = 40, 5
    t = _rand_gauss(gm, dim, 8)
    x0 = gm.init_with_seed(n_chains, dim, 15, np.float64).astype(dtype)

    def make(conv, pooled):
        return gm.NUTS.new_with_mass_matrix(t, x0, 0.8, _cfg(gm, "dense", 5, 5, 10, conv, pooled),
                                            dtype=dtype).set_seed(6)

    # a sampler that never used the feature, and one that went back to the
    # reference convention, write the reference convention's blob: header and
    # the per-chain parts only
    never = make("reference", False)
    back = make("whitening", True)
    back.set_mass_adaptation(_cfg(gm, "dense", 5, 5, 10, "reference", False))
    plain = never.save_state()
    assert back.save_state() == plain
    esz = np.dtype(dtype).itemsize
    parts = (n_chains * dim * esz + n_chains * 8 + 4 * n_chains * esz + n_chains * 8 + n_chains * 4
             + 2 * n_chains * dim * esz + 2 * n_chains * dim * dim * esz)
    header = len(gm.NUTS(t, x0, 0.8, dtype=dtype).save_state()) - (n_chains * dim * esz + 2 * n_chains * 8
                                                                  + 4 * n_chains * esz)
    assert len(plain) == header + parts
    a = make("whitening", True)
    a.run(1, 30)  # a first warm-up run: windows end at m = 15 and 24
    assert a.metric_updates() == (2, 0)
    mid = a.save_state()
    assert len(mid) == len(plain) + 8 * (4 * dim * dim + 2 * dim) + 32
    b = make("reference", False).load_state(mid)
    assert b.save_state() == mid
    _same_run(a, b, 5, 40)  # the warm-up goes on: the window schedule persists
    assert a.metric_updates() == b.metric_updates() and a.metric_updates()[0] > 2
    for x, y in zip(a.pooled_metric() + a.step_sizes(), b.pooled_metric() + b.step_sizes()):
        np.testing.assert_array_equal(x, y)
    after = a.save_state()
    assert b.save_state() == after
    c = make("whitening", True).load_state(after)
    _same_run(a, c, 6, 0)
    assert c.save_state() == a.save_state()
    # a reference-convention blob returns a whitening sampler to that path
    c.load_state(plain)
    assert c.save_state() == plain
    with pytest.raises(gm.GMError):
        c.pooled_metric()
    _same_run(c, never, 4, 25)


# ---- 6. statistics on changes nothing ------------------------------------------------
@gpu
def test_statistics_change_nothing(gm):
    t = _rand_gauss(gm, 6, 3)
    x0 = gm.init_with_seed(33, 6, 2, np.float64)
    pair = []
    for stats in (False, True):
        s = gm.NUTS.new_with_mass_matrix(t, x0, 0.8, _cfg(gm, "dense", 5, 5, 10, pooled=True)).set_seed(9)
        s.set_steps_per_launch(11)
        if stats:
            s.collect_stats("all")
        pair.append(s)
    _same_run(pair[0], pair[1], 12, 50)
    for x, y in zip(pair[0].pooled_metric() + pair[0].step_sizes(), pair[1].pooled_metric() + pair[1].step_sizes()):
        np.testing.assert_array_equal(x, y)
    assert pair[0].metric_updates() == pair[1].metric_updates() == (3, 0)
    assert pair[1].last_stats().n_transitions == 61


# ---- 7. it does what it is for --------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_warmup_on_the_rotated_gaussian(gm, oracle, dtype):
    mean, cov = bench.dense_gauss_32()
    n_chains, dim = 256, 32
    target = gm.DenseGaussian(mean, cov)
    x0 = gm.init_with_seed(n_chains, dim, 23, np.float64).astype(dtype)

    def arm(cfg):
        s = gm.NUTS(target, x0, 0.8, dtype=dtype) if cfg is None else gm.NUTS.new_with_mass_matrix(
            target, x0, 0.8, cfg, dtype=dtype)
        s.set_seed(31).collect_stats(True)
        out = s.run(200, 400)
        return s, out.astype(np.float64), float(s.last_stats().n_leapfrog.mean())

    s, out, lf_pooled = arm(gm.NUTSMassMatrixConfig("dense", convention="whitening", pooled=True))
    sigma, lp = s.pooled_metric()
    ev = np.linalg.eigvals(np.linalg.solve(cov, sigma)).real
    lam, vec = np.linalg.eigh(cov)
    var = ((out.reshape(-1, dim) - mean) @ vec).var(axis=0) / lam
    si, _, lf_ident = arm(None)
    sr, _, lf_ref = arm(gm.NUTSMassMatrixConfig("dense"))
    print(f"eigenvalues of Sigma^-1 Sigma_hat in [{ev.min():.3f}, {ev.max():.3f}]; variance along the "
          f"eigenvectors / eigenvalue in [{var.min():.3f}, {var.max():.3f}]; updates {s.metric_updates()}; "
          f"leapfrogs per collected transition: pooled whitening {lf_pooled:.2f}, identity {lf_ident:.2f}, "
          f"reference dense {lf_ref:.2f}")
    assert 0.7 <= ev.min() and ev.max() <= 1.7
    assert s.metric_updates()[1] == 0 and s.metric_updates()[0] > 0
    assert np.all((0.9 <= var) & (var <= 1.1))
    assert lf_pooled < lf_ident
    # the adapted Sigma_hat in a fresh sampler with another chain count: test 1's tie
    x1 = gm.init_with_seed(40, dim, 29, np.float64).astype(dtype)
    f = gm.NUTS.new_with_mass_matrix(target, x1, 0.8, gm.NUTSMassMatrixConfig("dense", convention="whitening"),
                                     dtype=dtype).set_seed(13)
    f.set_pooled_metric(sigma)
    m = f.mass_matrix()
    assert np.all(m.kind == 2)
    np.testing.assert_array_equal(m.dense_inv[39], sigma.astype(dtype))
    np.testing.assert_array_equal(m.dense_chol[0], lp.astype(dtype))
    ref.oracle_tie(oracle, f, target, dim, 2, 10, 13, 0)
    for x in (s, si, sr, f):
        x.close()


# ---- 8. error paths ---------------------------------------------------------------------
def _twin_check(make, s):
    """s is unchanged: its next run equals an untouched twin's."""
    t = make()
    _same_run(s, t, 3, 12)
    assert s.save_state() == t.save_state()


@gpu
def test_error_paths(gm):
    L = gm._lib
    lib = L.load()
    iso = gm.IsotropicGaussian(1.0)
    x0 = gm.init_det(4, 3)
    sig = np.eye(3)

    buf = np.zeros((3, 3))

    def calls(s):
        return [lib.gm_nuts_set_metric_convention(s._h, 1, 1), lib.gm_nuts_set_pooled_metric(s._h, L.ptr(sig)),
                lib.gm_nuts_get_pooled_metric(s._h, L.ptr(buf), None, None, None)]

    # HMC and MH samplers
    for make in (lambda: gm.HMC(iso, x0, 0.1, 3).set_seed(1),
                 lambda: gm.MetropolisHastings(iso, gm.IsotropicGaussian(0.5), x0).set_seed(1)):
        s = make()
        assert calls(s) == [L.GM_EINVAL] * 3
        t = make()
        np.testing.assert_array_equal(s.run(3, 2), t.run(3, 2))
        assert s.save_state() == t.save_state()

    small = dict(start_buffer=3, end_buffer=3, initial_window=10)

    def make():
        return gm.NUTS.new_with_mass_matrix(iso, x0, 0.8, gm.NUTSMassMatrixConfig("dense", **small)).set_seed(1)

    # pooled with the reference convention; bad codes; no pooled metric kept; no dense whitening configured
    s = make()
    assert lib.gm_nuts_set_metric_convention(s._h, 0, 1) == L.GM_EINVAL
    assert lib.gm_nuts_set_metric_convention(s._h, 2, 0) == L.GM_EINVAL
    assert lib.gm_nuts_set_metric_convention(s._h, 1, 2) == L.GM_EINVAL
    assert lib.gm_nuts_get_pooled_metric(s._h, None, None, None, None) == L.GM_ESTATE
    assert lib.gm_nuts_set_pooled_metric(s._h, L.ptr(sig)) == L.GM_ESTATE
    with pytest.raises(gm.GMError):
        s.set_mass_adaptation(gm.NUTSMassMatrixConfig("dense", pooled=True, **small))
    _twin_check(make, s)

    # whitening, but the diagonal or no metric: nothing to set
    for adaptation in ("diagonal", "none"):
        def make_d():
            return gm.NUTS.new_with_mass_matrix(
                iso, x0, 0.8, gm.NUTSMassMatrixConfig(adaptation, convention="whitening", **small)).set_seed(1)
        s = make_d()
        assert lib.gm_nuts_set_pooled_metric(s._h, L.ptr(sig)) == L.GM_ESTATE
        _twin_check(make_d, s)

    # pooled at dim 1 and 65 (per-chain whitening is allowed there)
    for dim in (1, 65):
        def make_n():
            return gm.NUTS.new_with_mass_matrix(
                iso, gm.init_det(4, dim), 0.8,
                gm.NUTSMassMatrixConfig("dense", convention="whitening", **small)).set_seed(1)
        s = make_n()
        assert lib.gm_nuts_set_metric_convention(s._h, 1, 1) == L.GM_EINVAL
        with pytest.raises(gm.GMError):
            s.set_mass_adaptation(gm.NUTSMassMatrixConfig("dense", convention="whitening", pooled=True, **small))
        bad = np.eye(dim)
        assert lib.gm_nuts_set_pooled_metric(s._h, L.ptr(bad)) == L.GM_ESTATE
        _twin_check(make_n, s)

    # a non-symmetric, indefinite or non-finite sigma
    def make_w():
        return gm.NUTS.new_with_mass_matrix(
            iso, x0, 0.8, gm.NUTSMassMatrixConfig("dense", convention="whitening", pooled=True, **small)).set_seed(1)

    asym = np.eye(3)
    asym[0, 1] = 0.1
    indef = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = np.eye(3)
    nan[2, 2] = float("nan")
    s = make_w()
    for bad in (asym, indef, nan):
        assert lib.gm_nuts_set_pooled_metric(s._h, L.ptr(bad)) == L.GM_EINVAL
    assert lib.gm_nuts_set_pooled_metric(s._h, None) == L.GM_EINVAL
    _twin_check(make_w, s)
    # a rejected matrix leaves a set one in place
    good = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, 0.25], [0.0, 0.25, 4.0]])
    s = make_w().set_pooled_metric(good)
    for bad in (asym, indef, nan):
        assert lib.gm_nuts_set_pooled_metric(s._h, L.ptr(bad)) == L.GM_EINVAL
    np.testing.assert_array_equal(s.pooled_metric()[0], good)
    _twin_check(lambda: make_w().set_pooled_metric(good), s)
