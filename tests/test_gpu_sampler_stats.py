"""Per-transition sampler statistics on the GPU (gm_sampler_set_stats,
Sampler.collect_stats, SamplerStats; gm_launch.h StatsRec).

1. HMC records against the numpy float64 transcription (tests/_hmc_stats_ref.py)
   driven by the engine's own draws;
2. exact identities of the records with the sampler's counters and samples,
   HMC and NUTS, every kernel family (lane-group, E = 2, wide);
3. NUTS per-transition leapfrogs against the oracle;
4. NUTS step sizes against a replay of the dual averaging from the recorded
   acceptance statistics;
5. NUTS energies: the kinetic energy they imply is chi^2_D / 2;
6. divergences, both outcomes exact, HMC and NUTS (a run-time-compiled target);
7. the device reduction against numpy, and a synthetic case through the C ABI;
8. the dense-metric HMC kernel and the frozen-dense NUTS kernel;
9. the error paths that need a sampler.

Tolerances: the GPU's largest deviation from the float64 numpy value,
measured on an MI355X and written beside each case; the assertion allows 64
times that (the convention of tests/test_gpu_hmc_adapt.py).
"""
import ctypes as C

import numpy as np
import pytest

from tests import _hmc_stats_ref as sref
from tests._oracle import Target

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
FIELDS = ("energy", "accept_stat", "step_size", "n_leapfrog", "tree_depth", "divergent", "accepted")


def _fields(st):
    return {k: getattr(st, k) for k in FIELDS}


# ---- 1. HMC against the transcription -----------------------------------------
# measured deviation (step_size relative; energy relative to max(1, |E|);
# accept_stat absolute), 80 transitions x 6 chains
MEASURED_HMC = {"step_size": 4.4e-9, "energy": 1.1e-8, "accept_stat": 1.9e-8}  # decision margin 3.6e-3
_SIGMA = np.array([0.5, 1.0, 3.0])


def _engine_draws(gm, n_chains, dim, seed, n):
    from general_mcmc_amd import batch_vector as bv
    z = bv.DeviceMatrix((n_chains, dim), np.float64)
    zs, us = [], []
    for t in range(n):
        bv.fill_random_normal(z, seed, t)
        zs.append(z.to_host())
        us.append(bv.sample_uniform(n_chains, np.float64, seed, t).to_host())
    return lambda t: (zs[t], us[t])


def _prec_gauss(gm, mean, prec):
    """A Gaussian target given by its precision matrix as it stands (the
    entries reach the device exactly), norm_const 0."""
    from general_mcmc_amd import _lib

    class PrecGauss(gm.distributions._TargetBase):
        def __init__(self):
            self.mean = np.ascontiguousarray(mean, dtype=np.float64)
            self.prec = np.ascontiguousarray(prec, dtype=np.float64)
            self.dim = self.mean.shape[0]

        def _fill(self, t, dim):
            t.kind = _lib.GM_TARGET_GAUSS
            t.mean = self.mean.ctypes.data_as(C.POINTER(C.c_double))
            t.prec = self.prec.ctypes.data_as(C.POINTER(C.c_double))
            t.norm_const = 0.0
            return [self.mean, self.prec]

    return PrecGauss()


def _hmc_adapting(gm, mode):
    n_chains, dim, seed = 6, 3, 29
    x0 = gm.init_with_seed(n_chains, dim, 14, np.float64)
    s = gm.HMC(_prec_gauss(gm, np.zeros(dim), np.diag(1.0 / _SIGMA ** 2)), x0, 0.5, 4, dtype=np.float64)
    s.set_seed(seed).set_adaptation(gm.HMCAdaptConfig("step_size", 0.8, 5, 10, 10, 0.05, 1e-6))
    return s.collect_stats(mode), x0, seed


def test_hmc_records_follow_the_transcription(gm):
    s, x0, seed = _hmc_adapting(gm, "all")
    out = s.run(20, 60)
    st = s.last_stats()
    assert (st.n_transitions, st.n_warmup, st.first_row, st.record_bytes) == (80, 60, 0, 32)
    prec = 1.0 / _SIGMA ** 2
    r = sref.run(lambda q: (-0.5 * np.sum(q * q * prec, axis=1), -q * prec), x0, 0.5, 4, 20, 60, 1,
                 _engine_draws(gm, 6, 3, seed, 80))
    assert r["margin"] >= 1e-9, r["margin"]
    np.testing.assert_array_equal(st.accepted, r["accepted"].T)
    assert 0 < st.accepted.sum() < st.accepted.size  # both outcomes
    np.testing.assert_array_equal(st.divergent, r["divergent"].T)
    np.testing.assert_array_equal(st.n_leapfrog, np.full((6, 80), 4))
    np.testing.assert_array_equal(st.tree_depth, np.zeros((6, 80)))
    dev = {"step_size": np.max(np.abs(st.step_size - r["step_size"].T) / r["step_size"].T),
           "energy": np.max(np.abs(st.energy - r["energy"].T) / np.maximum(1.0, np.abs(r["energy"].T))),
           "accept_stat": np.max(np.abs(st.accept_stat - r["accept_stat"].T))}
    print(f"HMC records, deviation from the transcription: {dev}, decision margin {r['margin']:.3e}")
    for k, v in dev.items():
        assert v <= 64 * MEASURED_HMC[k], dev
    # the collected mode is the tail of it
    full = _fields(st)
    c, _, _ = _hmc_adapting(gm, "collected")
    np.testing.assert_array_equal(c.run(20, 60), out)
    cs = c.last_stats()
    assert (cs.n_transitions, cs.n_warmup, cs.first_row) == (20, 0, 0)
    for k, v in _fields(cs).items():
        np.testing.assert_array_equal(v, full[k][:, 60:], err_msg=k)
    s.close()
    c.close()


# ---- 2. exact identities ------------------------------------------------------
def _check_identities(kind, make, run, n_total, row_of_first_transition):
    """make(mode) -> a fresh sampler; run(s) -> its samples [C, rows, D].
    The run has n_total transitions; its first collected transition ends in
    sample row row_of_first_transition."""
    plain = make(False)
    a0, l0 = plain.accept_counts(), plain.leapfrog_counts()
    ref = run(plain)
    s = make("all")
    out = run(s)
    st = s.last_stats()
    # samples and counters are those of the run without statistics
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(s.accept_counts(), plain.accept_counts())
    np.testing.assert_array_equal(s.leapfrog_counts(), plain.leapfrog_counts())
    np.testing.assert_array_equal(s.positions(), plain.positions())
    np.testing.assert_array_equal(np.asarray(s.step_sizes()), np.asarray(plain.step_sizes()))
    assert st.n_transitions == n_total and st.first_row == row_of_first_transition
    d_acc, d_lf = s.accept_counts() - a0, s.leapfrog_counts() - l0
    np.testing.assert_array_equal(st.n_leapfrog.sum(axis=1), d_lf)
    moved = st.accepted.sum(axis=1)
    if kind == "hmc":
        np.testing.assert_array_equal(moved, d_acc)
        np.testing.assert_array_equal(st.tree_depth, 0)
    else:
        # a NUTS accept count is the number of doublings that moved the chain
        # (several per transition); `accepted` is one bit per transition
        assert np.all(moved <= d_acc) and np.all(d_acc <= st.tree_depth.sum(axis=1))
        np.testing.assert_array_equal(moved == 0, d_acc == 0)
        np.testing.assert_array_equal(st.tree_depth, np.ceil(np.log2(st.n_leapfrog + 1.0)).astype(np.int32))
        assert st.tree_depth.min() >= 1
    # sample row r >= 1 is the state after the transition of record n_warmup + r - first_row
    rows = out.shape[1]
    differs = np.any(out[:, 1:] != out[:, :-1], axis=2)
    rec = st.n_warmup + np.arange(1, rows) - st.first_row
    np.testing.assert_array_equal(st.accepted[:, rec], differs)
    assert np.all(np.isfinite(st.energy)) and np.all((st.accept_stat >= 0) & (st.accept_stat <= 1))
    assert np.all(st.step_size > 0)
    full = _fields(st)
    # the collected mode holds the tail
    c = make("collected")
    np.testing.assert_array_equal(run(c), ref)
    cs = c.last_stats()
    assert cs.n_warmup == 0 and cs.first_row == st.first_row
    assert cs.n_transitions == st.n_transitions - st.n_warmup
    for k, v in _fields(cs).items():
        np.testing.assert_array_equal(v, full[k][:, st.n_warmup:], err_msg=k)
    # stale after the next run
    run(s)
    with pytest.raises(RuntimeError, match="stale"):
        st.energy
    with pytest.raises(RuntimeError, match="stale"):
        st.summary()
    fresh = s.last_stats()
    assert fresh.n_transitions == n_total
    for x in (plain, s, c):
        x.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [3, 65])
def test_hmc_identities(gm, dtype, dim):
    x0 = (gm.init_with_seed(70, dim, 11, np.float64) * 0.5).astype(dtype)

    def make(mode):
        s = gm.HMC(gm.IsotropicGaussian(1.3), x0, 0.9, 5, dtype=dtype, chain_offset=5).set_seed(3)
        return s.set_steps_per_launch(3).collect_stats(mode)
    _check_identities("hmc", make, lambda s: s.run(6, 5), 11, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,chains", [(3, 70), (33, 70), (300, 5)])
@pytest.mark.parametrize("progress", [False, True])
def test_nuts_identities(gm, dtype, dim, chains, progress):
    x0 = (gm.init_with_seed(chains, dim, 12, np.float64) * 0.5).astype(dtype)

    def make(mode):
        s = gm.NUTS(gm.IsotropicGaussian(1.3), x0, 0.8, dtype=dtype, max_depth=5).set_seed(9)
        return s.set_steps_per_launch(3).collect_stats(mode)
    if dim == 300:
        probe = make(False)
        assert probe.layout()[0] > 64  # the wide kernel
        probe.close()
    if progress:
        _check_identities("nuts", make, lambda s: s.run_progress(6, 5)[0], 11, 0)
    else:
        _check_identities("nuts", make, lambda s: s.run(6, 6), 11, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nuts_run_without_burn_in_has_no_transition_for_row_zero(gm, dtype):
    x0 = (gm.init_with_seed(70, 3, 12, np.float64) * 0.5).astype(dtype)

    def make(mode):
        s = gm.NUTS(gm.IsotropicGaussian(1.3), x0, 0.8, dtype=dtype, max_depth=5).set_seed(9)
        return s.set_steps_per_launch(3).collect_stats(mode)
    _check_identities("nuts", make, lambda s: s.run(12, 0), 11, 1)


def test_step_records_nothing_and_device_samples_carry_the_statistics(gm):
    x0 = gm.init_with_seed(9, 3, 1, np.float64)
    s = gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.3, 3, dtype=np.float64).set_seed(2).collect_stats(True)
    ds = s.run_positions(4, 2)
    st = ds.stats
    e = st.energy.copy()
    assert st.ptr != 0 and e.shape == (9, 4)
    s.step()  # not a run: records nothing, the last run's records stay
    np.testing.assert_array_equal(s.last_stats().energy, e)
    # a run that collects no row: its summary of the collected transitions is empty, not an error
    s.collect_stats("all").run(0, 3)
    st = s.last_stats()
    assert (st.n_transitions, st.n_warmup) == (3, 3)
    sm = st.summary()
    assert sm.n_transitions == 0 and np.all(sm.n_divergent == 0) and np.all(np.isnan(sm.ebfmi))
    assert "0 transitions" in str(sm)
    assert st.summary(warmup=True).n_transitions == 3
    s.collect_stats(False).run(2, 0)
    with pytest.raises(gm.GMError, match="recorded no statistics"):
        s.last_stats()
    s.close()


# ---- 3. NUTS per-transition leapfrogs against the oracle -----------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nuts_leapfrogs_per_transition_match_the_oracle(gm, oracle, dtype):
    n_chains, dim, n_collect, n_discard, depth, seed = 20, 5, 4, 8, 6, 9
    x0 = (gm.init_with_seed(n_chains, dim, 4, np.float64) * 0.5).astype(dtype)
    t = gm.RosenbrockND()
    s = gm.NUTS(t, x0, 0.8, dtype=dtype, max_depth=depth).set_seed(seed).collect_stats("all")
    s.set_steps_per_launch(5)
    s.run_progress(n_collect, n_discard)
    st = s.last_stats()
    assert (st.n_transitions, st.n_warmup, st.first_row) == (12, 8, 0)
    lay = s.layout()
    ot = Target.from_product(t, dim)
    state = oracle.nuts_state(n_chains, dtype)
    # init_chain_state alone, then one transition at a time
    q, _, _, _ = oracle.nuts_run(ot, x0, state, 0.8, depth, seed, 0, 0, 0, True, *lay)
    per = []
    for m in range(12):
        q, _, nlf = oracle.nuts_step(ot, q, state, 0.8, depth, seed, m, 1, m, n_discard, *lay)
        per.append(nlf)
    np.testing.assert_array_equal(st.n_leapfrog, np.array(per).T)
    np.testing.assert_array_equal(s.positions(), q)
    np.testing.assert_array_equal(st.n_leapfrog.sum(axis=1), s.leapfrog_counts())
    s.close()


# ---- 4. NUTS step size and acceptance tie --------------------------------------
MEASURED_NUTS_EPS = 1.4e-15  # largest relative deviation of step_size[m] from the float64 replay


def test_nuts_step_sizes_replay_from_the_recorded_acceptance(gm):
    n_chains, n_discard, n_collect = 20, 40, 5
    x0 = gm.init_with_seed(n_chains, 5, 4, np.float64) * 0.5
    s = gm.NUTS(gm.RosenbrockND(), x0, 0.8, dtype=np.float64, max_depth=6).set_seed(9).collect_stats("all")
    s.run_progress(n_collect, n_discard)
    st = s.last_stats()
    eps, a = st.step_size, st.accept_stat
    # generic_nuts.rs:882-893 from the state init_chain_state leaves
    gamma, t0, kappa, delta = 0.05, 10.0, 0.75, 0.8
    mu, h_bar, eps_bar = np.log(10.0 * eps[:, 0]), np.zeros(n_chains), np.ones(n_chains)
    dev = 0.0
    for m in range(1, n_discard + 1):
        eta = 1.0 / (m + t0)
        h_bar = (1.0 - eta) * h_bar + eta * (delta - a[:, m - 1])
        e = np.exp(mu - np.sqrt(m) / gamma * h_bar)
        eta = m ** (-kappa)
        eps_bar = np.exp((1.0 - eta) * np.log(eps_bar) + eta * np.log(e))
        dev = max(dev, float(np.max(np.abs(eps[:, m] - e) / e)))
    now, bar = s.step_sizes()
    dev = max(dev, float(np.max(np.abs(bar - eps_bar) / eps_bar)))
    print(f"NUTS step sizes, deviation from the replay: {dev:.3e}")
    assert dev <= 64 * MEASURED_NUTS_EPS
    assert np.ptp(eps[:, :n_discard + 1], axis=1).min() > 0  # the warm-up moved every chain's step size
    # transition n_discard still integrates with the warm-up's last step size;
    # from the next one on it is eps_bar, exactly
    np.testing.assert_array_equal(eps[:, n_discard + 1:], np.broadcast_to(bar[:, None], (n_chains, n_collect - 1)))
    np.testing.assert_array_equal(now, bar)
    s.close()


# ---- 5. NUTS energy -----------------------------------------------------------
def test_nuts_energy_is_the_hamiltonian_after_the_momentum_draw(gm):
    n_chains, dim, n = 256, 8, 50
    x0 = gm.init_with_seed(n_chains, dim, 6, np.float64)
    t = gm.IsotropicGaussian(1.0)
    s = gm.NUTS(t, x0, 0.8, dtype=np.float64).set_seed(5).collect_stats(True)
    ds = s.run_positions(n, 50)
    st = ds.stats
    assert (st.n_transitions, st.n_warmup, st.first_row) == (n, 0, 0)
    lp = ds.logp()
    host = ds.to_host()
    assert lp.shape == (n_chains, n)
    np.testing.assert_array_equal(lp, t.unnorm_logp_batch(host.reshape(-1, dim)).reshape(n_chains, n))
    # (8 squares and 7 additions in float64: far inside 1e-12)
    np.testing.assert_allclose(lp, -0.5 * np.sum(host * host, axis=2), rtol=1e-12, atol=1e-12)
    # record k starts from row k - 1: K0 = E + logp(previous row) = chi^2_D / 2
    k0 = st.energy[:, 1:] + lp[:, :-1]
    assert k0.min() >= 0
    cnt = k0.size
    # chi^2_8 / 2 is Gamma(4, 1): mean 4, variance 4, fourth central moment 72
    assert abs(k0.mean() - dim / 2) <= 5 * np.sqrt((dim / 2) / cnt)
    assert abs(k0.var(ddof=1) - dim / 2) <= 5 * np.sqrt((72.0 - 16.0) / cnt)
    s.close()


# ---- 6. divergences -----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_hmc_divergences(gm, dtype):
    n_chains = 32
    x0 = gm.init_with_seed(n_chains, 4, 8, np.float64).astype(dtype)
    eps = np.where(np.arange(n_chains) % 2 == 0, 0.1, 2.1)
    s = gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.1, 50, dtype=dtype).set_seed(3).set_step_sizes(eps)
    s.collect_stats("all").run(10, 2)
    st = s.last_stats()
    assert not st.divergent[0::2].any() and st.accepted[0::2].any()
    assert st.divergent[1::2].all() and not st.accepted[1::2].any()
    np.testing.assert_array_equal(st.accept_stat[1::2], 0)
    np.testing.assert_array_equal(st.step_size, np.broadcast_to(eps.astype(dtype)[:, None], (n_chains, 12)))
    np.testing.assert_array_equal(s.last_stats().summary(warmup=True).n_divergent, np.where(eps > 1, 12, 0))
    s.close()


# a unit Gaussian inside the radius sqrt(p[0]), a wall outside: -1e30, no gradient
WALL = r"""
template <class T>
__device__ T gm_logp_grad(const T* x, T* g, const T* p) {
  T part = (T)0;
#pragma unroll
  for (int i = 0; i < GM_DIM; ++i) part = (i == 0) ? x[i] * x[i] : part + x[i] * x[i];
  const bool in = part <= p[0];
#pragma unroll
  for (int i = 0; i < GM_DIM; ++i) g[i] = in ? -x[i] : (T)0;
  return in ? (T)-0.5 * part : (T)-1e30;
}
"""
WALL_RADIUS = 1.5  # on an MI355X: 36.5 % (f32) and 37.2 % (f64) of the 1920 leaves cross it


@pytest.mark.parametrize("dtype", DTYPES)
def test_nuts_divergences_with_a_run_time_compiled_target(gm, dtype):
    n_chains, n = 64, 30
    x0 = (gm.init_with_seed(n_chains, 2, 8, np.float64) * 0.5).astype(dtype)
    assert np.all(np.sum(x0.astype(np.float64) ** 2, axis=1) < WALL_RADIUS ** 2)
    t = gm.CustomTarget(WALL, 2, [WALL_RADIUS ** 2])
    s = gm.NUTS(t, x0, 0.8, dtype=dtype, max_depth=1).set_seed(7).collect_stats("all")
    out = s.run(n + 1, 0)
    st = s.last_stats()
    assert (st.n_transitions, st.first_row) == (n, 1)
    np.testing.assert_array_equal(st.n_leapfrog, 1)
    np.testing.assert_array_equal(st.tree_depth, 1)
    np.testing.assert_array_equal(st.divergent, st.accept_stat == 0)
    frac = st.divergent.mean()
    print(f"wall radius {WALL_RADIUS}: {frac:.3f} of the leaves diverge")
    assert 0.1 <= frac <= 0.9
    assert not (st.divergent & st.accepted).any()  # a divergent leaf never moves the chain
    assert np.all(np.sum(out.astype(np.float64) ** 2, axis=2) <= WALL_RADIUS ** 2 * (1 + 1e-6))
    sm = st.summary(warmup=True)
    np.testing.assert_array_equal(sm.n_divergent, st.divergent.sum(axis=1))
    np.testing.assert_array_equal(sm.n_max_depth, n)
    s.close()


# ---- 7. the reduction ----------------------------------------------------------
# measured relative deviation of the device reduction from numpy float64: the
# real run (f32 1.8e-15 / 1.4e-16, f64 1.5e-15 / 4.2e-16: E-BFMI / means) and
# the synthetic records (f32 8.8e-16 / 4.5e-16, f64 3.1e-15 / 2.7e-15). Summed
# without the shift, energies near 1e4 would leave E-BFMI some 1e-8 away.
MEASURED_REDUCE = {"ebfmi": 1.8e-15, "mean": 4.2e-16, "synthetic_ebfmi": 3.1e-15, "synthetic_mean": 2.7e-15}


def _numpy_summary(f, max_depth):
    with np.errstate(invalid="ignore", divide="ignore"):  # 0 / 0 where a range holds no finite energy
        return _numpy_summary_impl(f, max_depth)


def _numpy_summary_impl(f, max_depth):
    e = f["energy"].astype(np.float64)
    ok = np.isfinite(e)
    num = np.zeros(len(e))
    den = np.zeros(len(e))
    for c in range(len(e)):
        d = e[c, 1:] - e[c, :-1]
        num[c] = np.sum(d[ok[c, 1:] & ok[c, :-1]] ** 2)
        v = e[c][ok[c]]
        den[c] = np.sum((v - v.mean()) ** 2) if v.size else 0.0
    n = e.shape[1]
    per = dict(ebfmi=num / den, n_divergent=f["divergent"].sum(axis=1),
               mean_accept_stat=f["accept_stat"].astype(np.float64).sum(axis=1) / n,
               mean_n_leapfrog=f["n_leapfrog"].sum(axis=1) / n, mean_tree_depth=f["tree_depth"].sum(axis=1) / n,
               n_max_depth=(f["tree_depth"] >= max_depth).sum(axis=1) if max_depth else np.zeros(len(e)),
               n_energy=ok.sum(axis=1), n_skipped=(~ok).sum(axis=1))
    cn = e.size
    tot = dict(ebfmi=num.sum() / den.sum(), n_divergent=per["n_divergent"].sum(),
               mean_accept_stat=f["accept_stat"].astype(np.float64).sum() / cn,
               mean_n_leapfrog=f["n_leapfrog"].sum() / cn, mean_tree_depth=f["tree_depth"].sum() / cn,
               n_max_depth=per["n_max_depth"].sum(), n_energy=ok.sum(), n_skipped=(~ok).sum())
    return per, tot


def _compare_summary(sm, per, tot, ebfmi_tol, mean_tol):
    dev = {"ebfmi": 0.0, "mean": 0.0}
    for k in ("n_divergent", "n_max_depth", "n_energy", "n_skipped"):
        np.testing.assert_array_equal(getattr(sm, k), per[k], err_msg=k)
        assert sm.total[k] == tot[k], k
    for k in ("ebfmi", "mean_accept_stat", "mean_n_leapfrog", "mean_tree_depth"):
        g = np.append(getattr(sm, k), sm.total[k])
        r = np.append(per[k], tot[k])
        d = float(np.max(np.abs(g - r) / np.abs(r)))
        kk = "ebfmi" if k == "ebfmi" else "mean"
        dev[kk] = max(dev[kk], d)
    print(f"reduction, relative deviation from numpy: {dev}")
    assert dev["ebfmi"] <= 64 * ebfmi_tol and dev["mean"] <= 64 * mean_tol, dev
    return dev


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduction_of_a_real_run(gm, dtype):
    x0 = (gm.init_with_seed(70, 3, 12, np.float64) * 0.5).astype(dtype)
    s = gm.NUTS(gm.IsotropicGaussian(1.3), x0, 0.8, dtype=dtype, max_depth=3).set_seed(9).collect_stats("all")
    s.run_positions(100, 101)
    st = s.last_stats()
    assert (st.n_transitions, st.n_warmup) == (200, 100)
    f = _fields(st)
    for rows in ((0, 200), (100, 100), (17, 101), (3, 2)):
        sm = st.summary(rows=rows)
        per, tot = _numpy_summary({k: v[:, rows[0]:rows[0] + rows[1]] for k, v in f.items()}, 3)
        assert sm.n_transitions == rows[1]
        _compare_summary(sm, per, tot, MEASURED_REDUCE["ebfmi"], MEASURED_REDUCE["mean"])
    assert 0 < st.summary(warmup=True).total["n_max_depth"] < 200 * 70  # both sides of the depth count
    np.testing.assert_array_equal(st.summary().ebfmi, st.summary(rows=(100, 100)).ebfmi)
    text = str(st.summary())
    assert "E-BFMI" in text and "divergent" in text and len(text.splitlines()) == 8
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduction_keeps_the_digits_of_large_energies(gm, dtype):
    """Records written from the host, through gm_stats_reduce_device:
    energies 1e4 + N(0, 1), 300 chains (two blocks) x 1000 rows (several row
    splits), one NaN energy, a row range."""
    from general_mcmc_amd import _lib
    from general_mcmc_amd.batch_vector import DeviceMatrix
    lib = _lib.require_gpu()
    n_chains, n_rows, depth = 300, 1000, 4
    rng = np.random.default_rng(5)
    word = np.uint32 if dtype == np.float32 else np.uint64
    rec = np.zeros((n_rows, n_chains), dtype=[("energy", dtype), ("accept_stat", dtype), ("step_size", dtype),
                                              ("word", word)])
    assert rec.dtype.itemsize == 4 * np.dtype(dtype).itemsize
    rec["energy"] = 1e4 + rng.standard_normal((n_rows, n_chains))
    rec["energy"][500, 3] = np.nan
    rec["energy"][0, 7] = np.inf  # the first row of a chain: its shift comes from the second
    rec["accept_stat"] = rng.random((n_rows, n_chains))
    rec["step_size"] = 0.1
    td = rng.integers(1, depth + 1, (n_rows, n_chains))
    nlf = rng.integers(1, 1 << 20, (n_rows, n_chains))
    div = rng.random((n_rows, n_chains)) < 0.1
    acc = rng.random((n_rows, n_chains)) < 0.7
    rec["word"] = (nlf | (td << 24) | (div.astype(np.int64) << 30) | (acc.astype(np.int64) << 31)).astype(word)
    dev = DeviceMatrix.from_host(rec.view(np.uint8).reshape(n_rows, -1))
    f = dict(energy=rec["energy"].T, accept_stat=rec["accept_stat"].T, n_leapfrog=nlf.T, tree_depth=td.T,
             divergent=div.T, accepted=acc.T)
    from general_mcmc_amd.stats import _SUMMARY_NAMES, StatsSummary
    for r0, n in ((0, n_rows), (10, 900), (500, 1)):
        pc = np.empty((len(_SUMMARY_NAMES), n_chains))
        tot = np.empty(len(_SUMMARY_NAMES))
        _lib.check(lib.gm_stats_reduce_device(C.c_void_p(dev.ptr), _lib.dtype_code(dtype), n_chains, r0, n, depth,
                                              _lib.ptr(pc), _lib.ptr(tot)))
        sm = StatsSummary(n, *[pc[i] for i in range(len(_SUMMARY_NAMES))],
                          {k: float(tot[i]) for i, k in enumerate(_SUMMARY_NAMES)})
        per, tt = _numpy_summary({k: v[:, r0:r0 + n] for k, v in f.items()}, depth)
        if n == 1:  # one row: no difference, no spread: 0 / 0 on both sides
            assert np.all(np.isnan(sm.ebfmi)) and np.all(np.isnan(per["ebfmi"]))
            sm.ebfmi[:], per["ebfmi"][:] = 1.0, 1.0
            sm.total["ebfmi"], tt["ebfmi"] = 1.0, 1.0
        _compare_summary(sm, per, tt, MEASURED_REDUCE["synthetic_ebfmi"], MEASURED_REDUCE["synthetic_mean"])
        if n == n_rows:
            assert sm.n_skipped[3] == 1 and sm.n_skipped[7] == 1 and sm.total["n_skipped"] == 2
            assert np.all(np.abs(sm.ebfmi - 2.0) < 0.5)  # independent energies: E-BFMI near 2
    dev.close()


# ---- 8. the dense-metric kernels ----------------------------------------------
def _dense_cov(dim):
    rng = np.random.default_rng(31)
    a = rng.standard_normal((dim, dim))
    return a @ a.T / dim + 0.5 * np.eye(dim)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hmc_dense_metric_identities(gm, dtype):
    dim, cov = 5, _dense_cov(5)
    x0 = gm.init_with_seed(36, dim, 7, np.float64).astype(dtype)

    def make(mode):
        s = gm.HMC(gm.DenseGaussian(np.zeros(dim), cov), x0, 0.9, 4, dtype=dtype).set_seed(4)
        return s.set_dense_metric(cov).set_steps_per_launch(3).collect_stats(mode)
    _check_identities("hmc", make, lambda s: s.run(6, 5), 11, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nuts_frozen_dense_identities(gm, dtype):
    # (the frozen-dense kernel exists at layout 16 x 2 alone, which takes 17 <= dim <= 32)
    dim, cov = 17, _dense_cov(17)
    x0 = gm.init_with_seed(36, dim, 7, np.float64).astype(dtype)
    mc = gm.NUTSMassMatrixConfig("dense", start_buffer=4, end_buffer=4, initial_window=10, regularize=0.05,
                                 jitter=1e-6, dense_max_dim=75)
    made = []

    def make(mode):
        s = gm.NUTS.new_with_mass_matrix(gm.DenseGaussian(np.zeros(dim), cov), x0, 0.8, mc, dtype=dtype)
        s.set_seed(11).set_layout(16, 2).set_steps_per_launch(3).collect_stats(mode)
        s.run(1, 60)  # the warm-up: every chain's metric becomes dense
        assert np.all(s.mass_matrix().kind == 2)
        made.append(s)
        return s

    def run(s):
        out = s.run(12, 0)
        assert s.launch_plan()["frozen"] == 1
        return out
    _check_identities("nuts", make, run, 11, 1)


# ---- 9. errors ----------------------------------------------------------------
def test_error_paths_and_checkpoints(gm):
    E = gm._lib
    x0 = gm.init_with_seed(7, 5, 1, np.float64)
    m = gm.MetropolisHastings(gm.IsotropicGaussian(1.0), gm.IsotropicGaussian(0.5), x0)
    with pytest.raises(gm.GMError, match="HMC and NUTS") as e:
        m.collect_stats(True)
    assert e.value.code == E.GM_ESTATE
    wide = gm.HMC(gm.IsotropicGaussian(1.0), gm.init_with_seed(2, 1500, 1, np.float32), 0.01, 2)
    with pytest.raises(gm.GMError, match="wide") as e:
        wide.collect_stats("all")
    assert e.value.code == E.GM_EINVAL
    for s in (gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.3, 3).set_seed(5),
              gm.NUTS(gm.IsotropicGaussian(1.0), x0, 0.8).set_seed(5)):
        with pytest.raises(ValueError):
            s.collect_stats("everything")
        assert E.load().gm_sampler_set_stats(s._h, 3) == E.GM_EINVAL
        blob = s.save_state()
        s.collect_stats("all")
        with pytest.raises(gm.GMError, match="recorded no statistics") as e:
            s.last_stats()  # nothing has run
        assert e.value.code == E.GM_ESTATE
        assert s.save_state() == blob  # a run option, not sampler state
        s.run(3, 2)
        after = s.save_state()
        t = type(s)(gm.IsotropicGaussian(1.0), x0, *((0.3, 3) if isinstance(s, gm.HMC) else (0.8,))).set_seed(5)
        t.run(3, 2)
        assert t.save_state() == after
        with pytest.raises(gm.GMError, match="out of range"):
            s.last_stats().summary(rows=(3, 9))
        s.close()
        t.close()
    m.close()
    wide.close()
