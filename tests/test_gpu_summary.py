"""gm_summary / gm_rank_normalize on the GPU against the NumPy / SciPy
transcription of their definitions (tests/_rank_diag_ref.py).

Tolerances: ranks are exact. rhat atol 1e-3 and ESS rtol 1e-3 are the
project's own (test_split_rhat_ess_matches_oracle); mean, sd and quantiles
are f64 sums / one f64 interpolation, rtol 1e-12 of the parameter's largest
|x|. Normal scores: the device evaluates Phi^-1 in f64 by Halley steps on
erfc, so its error is the conditioning of Phi^-1 (|dz| = |dp| / phi(z) <=
|dp/p| / |z| in the tails, <= 1.26 |dp| at the centre) times the few ulp of
erfc and of the final step: below 50 * 2^-53 ~ 6e-15 absolute and relative;
1e-13 leaves a margin for SciPy's own few ulp."""
import functools

import numpy as np
import pytest

from tests import _rank_diag_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(4, 10, 2), (7, 41, 2), (33, 129, 17), (3, 1000, 1), (2, 10400, 1), (64, 1030, 3), (1024, 1026, 2)]
DTYPES = [np.float32, np.float64]
# a case whose Geyer margin is below 1e-5 under the shape-sum seed gets one other seed
SEED_SHIFT = {}


def _plan():
    import general_mcmc_amd as g
    return g.stats.sort_plan()


def _plan_shapes():
    """Pooled counts M = 2 C h around the one-workgroup limit and around one,
    two and three tiles of the global path (M is even: nearest below / at /
    above = -2 / 0 / +2, one element pair), as one chain of N = M or M + 1."""
    p = _plan()
    ms = {p["lds_max"] + d for d in (-2, 0, 2)}
    ms |= {k * p["tile"] + d for k in (1, 2, 3) for d in (-2, 0, 2)}
    return [(1, m + (i % 2), 1) for i, m in enumerate(sorted(ms))]


PLAN_SHAPES = _plan_shapes()


def pooled(shape):
    return 2 * shape[0] * (shape[1] // 2)


@functools.lru_cache(maxsize=None)
def sample(kind, shape, dtype):
    x = ref.generate(kind, shape, dtype, SEED_SHIFT.get((kind, shape, np.dtype(dtype).name), 0))
    x.setflags(write=False)
    return x


def rank_cases():
    for shape in SHAPES + PLAN_SHAPES:
        for dt in DTYPES:
            if shape == (1024, 1026, 2) and dt is np.float64:
                continue
            yield shape, dt


def test_both_sort_paths_are_covered():
    p = _plan()
    ms = [pooled(s) for s in SHAPES + PLAN_SHAPES]
    assert any(m <= p["lds_max"] for m in ms) and any(m > p["lds_max"] for m in ms)
    assert p["lds_max"] in ms and p["lds_max"] + 2 in ms
    assert any(m > 3 * p["tile"] for m in ms) and any(m > 1 << 20 for m in ms)
    assert p["radix_bits"] == 8 and 300 > p["chunk_params"]


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("shape,dtype", list(rank_cases()))
def test_ranks_are_exact(gm, shape, dtype, folded, kind):
    x = sample(kind, shape, dtype)
    r, z = gm.rank_normalize(x, folded=folded)
    rr, zr = ref.rank_normalize(x, folded=folded)
    np.testing.assert_array_equal(r, rr)
    ok = np.isfinite(zr)
    assert (np.isnan(z) == ~ok).all()
    err = np.abs(z[ok] - zr[ok]) / np.maximum(1.0, np.abs(zr[ok]))
    print(f"ranks {kind} {shape} {np.dtype(dtype).name} folded={folded}: max z error {err.max():.3e}")
    assert err.max() <= 1e-13


def _tie_inputs(shape, dtype):
    c, n, _ = shape
    rng = np.random.default_rng(5)
    fi = np.finfo(dtype)
    out = {
        "three_values": rng.integers(0, 3, size=shape).astype(dtype),
        "all_equal": np.full(shape, 1.25, dtype=dtype),
        "ascending": np.arange(c * n, dtype=dtype).reshape(shape),
        "descending": -np.arange(c * n, dtype=dtype).reshape(shape),
        "zeros_and_extremes": rng.choice(np.array(
            [-0.0, 0.0, -1.0, -2.5, 1.0, fi.smallest_subnormal, -fi.smallest_subnormal, 3 * fi.smallest_subnormal,
             fi.tiny, -fi.tiny, fi.max, -fi.max], dtype=dtype), size=shape),
    }
    if dtype is np.float64:
        out["below_f32_precision"] = 1.0 + rng.integers(0, 4096, size=shape) * 2.0 ** -40
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 1030, 1), (7, 41, 1)])
def test_ties_and_key_order(gm, shape, dtype):
    m = pooled(shape)
    for name, x in _tie_inputs(shape, dtype).items():
        for folded in (False, True):
            r, _ = gm.rank_normalize(x, folded=folded)
            rr, _ = ref.rank_normalize(x, folded=folded)
            np.testing.assert_array_equal(r, rr, err_msg=f"{name} folded={folded}")
        if name == "all_equal":
            assert (r[np.isfinite(r)] == (m + 1) / 2).all()
            s = gm.summary(x)
            assert s.mean[0] == 1.25 and (s.quantiles[:, 0] == 1.25).all() and s.sd[0] == 0.0
            assert np.isnan([s.rhat[0], s.ess_bulk[0], s.ess_tail[0]]).all()
        if name == "below_f32_precision":
            r, _ = gm.rank_normalize(x)
            assert len(np.unique(r[np.isfinite(r)])) > (4000 if m > 60000 else 200)  # rounded to f32: one run


@functools.lru_cache(maxsize=None)
def reference_summary(kind, shape, dtype):
    return ref.summary(sample(kind, shape, dtype))


def _check_summary(s, want, x, tag=""):
    scale = np.abs(x.astype(np.float64)).max(axis=(0, 1))
    dev = {
        "rhat": np.abs(s.rhat - want["rhat"]).max(),
        "ess_bulk": (np.abs(s.ess_bulk - want["ess_bulk"]) / want["ess_bulk"]).max(),
        "ess_tail": (np.abs(s.ess_tail - want["ess_tail"]) / want["ess_tail"]).max(),
        "mean": (np.abs(s.mean - want["mean"]) / scale).max(),
        "sd": (np.abs(s.sd - want["sd"]) / scale).max(),
        "quantiles": (np.abs(s.quantiles - want["quantiles"]) / scale).max(),
    }
    print(f"summary {tag}: " + " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    assert dev["rhat"] <= 1e-3 and dev["ess_bulk"] <= 1e-3 and dev["ess_tail"] <= 1e-3, dev
    assert dev["mean"] <= 1e-12 and dev["sd"] <= 1e-12 and dev["quantiles"] <= 1e-12, dev


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_summary_matches_transcription(gm, shape, dtype, kind):
    x = sample(kind, shape, dtype)
    want = reference_summary(kind, shape, dtype)
    # the Geyer truncation is a discontinuity: the case must not sit on it
    print(f"margin {kind} {shape} {np.dtype(dtype).name}: {want['margin'].min():.3e}")
    assert want["margin"].min() >= 1e-5
    s = gm.summary(x)
    assert s.probs == (0.05, 0.5, 0.95) and s.quantiles.shape == (3, shape[2])
    _check_summary(s, want, x, f"{kind} {shape} {np.dtype(dtype).name}")
    assert len(str(s).splitlines()) == 1 + shape[2]


def test_other_probs(gm):
    x = sample("cauchy", (7, 41, 2), np.float64)
    probs = (0.0, 0.013, 0.25, 0.5, 0.999, 1.0)
    s = gm.summary(x, probs=probs)
    want = ref.summary(x, probs)
    scale = np.abs(x).max(axis=(0, 1))
    assert (np.abs(s.quantiles - want["quantiles"]) / scale).max() <= 1e-12
    y = ref.split(x)
    np.testing.assert_array_equal(s.quantiles[0], y.min(axis=(0, 1)))
    np.testing.assert_array_equal(s.quantiles[-1], y.max(axis=(0, 1)))
    assert gm.summary(x, probs=()).quantiles.shape == (0, 2)


def _fields(s):
    return {k: getattr(s, k) for k in ("mean", "sd", "quantiles", "rhat", "ess_bulk", "ess_tail")}


def test_device_and_host_paths_agree(gm):
    x0 = gm.init_det(256, 8, np.float32)
    s = gm.HMC(gm.IsotropicGaussian(1.0), x0, 0.25, 8).set_seed(7)
    ds = s.run_positions(200, 50)
    on_dev = ds.summary()
    on_host = gm.summary(ds.to_host())
    for k, v in _fields(on_dev).items():
        np.testing.assert_array_equal(v, _fields(on_host)[k], err_msg=k)
    assert (on_dev.rhat < 1.05).all() and (on_dev.rhat >= 0.999).all()
    assert (on_dev.ess_bulk > 100).all() and (on_dev.ess_tail > 100).all()
    s.run_positions(4, 0)
    with pytest.raises(RuntimeError):
        ds.summary()
    with pytest.raises(RuntimeError):
        ds.split_rhat_ess()
    s.close()


@pytest.mark.parametrize("shape", [(4, 20, 5), (8, 600, 5)])
def test_nan_touches_one_parameter_only(gm, shape):
    x = np.array(sample("ar", shape, np.float64))
    clean = _fields(gm.summary(x))
    x[1, 3, 2] = np.nan
    dirty = _fields(gm.summary(x))
    keep = [0, 1, 3, 4]
    for k in clean:
        assert np.isnan(dirty[k][..., 2]).all(), k
        np.testing.assert_array_equal(dirty[k][..., keep], clean[k][..., keep], err_msg=k)
        assert np.isfinite(clean[k]).all(), k
    x[1, 3, 2] = np.inf
    assert np.isnan(gm.summary(x).mean[2]) and np.isnan(gm.summary(x).ess_tail[2])


def test_chunks_equal_single_parameters(gm):
    shape = (4, 20, 300)
    assert shape[2] > _plan()["chunk_params"]
    x = sample("ar", shape, np.float32)
    whole = _fields(gm.summary(x))
    for p in range(shape[2]):
        one = _fields(gm.summary(np.ascontiguousarray(x[:, :, p:p + 1])))
        for k in whole:
            np.testing.assert_array_equal(one[k][..., 0], whole[k][..., p], err_msg=f"{k} of parameter {p}")
    _check_summary(gm.summary(x), reference_summary("ar", shape, np.float32), x, "ar (4, 20, 300) float32")


def test_split_rhat_unchanged_by_summary(gm):
    for shape in [(64, 1030, 3), (33, 129, 17)]:
        x = sample("ties", shape, np.float32)
        r0, e0 = gm.split_rhat_mean_ess(x)
        gm.summary(x)
        gm.rank_normalize(x)
        r1, e1 = gm.split_rhat_mean_ess(x)
        np.testing.assert_array_equal(r0, r1)
        np.testing.assert_array_equal(e0, e1)
