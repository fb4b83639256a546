"""Convergence diagnostics (stats.rs), computed on the GPU.

split_rhat_mean_ess  stats.rs:439-450 (R-hat = sqrt(W/V), the reference's
                     orientation, stats.rs:452-454; ESS via Geyer's initial
                     monotone sequence, stats.rs:523-573)
basic_stats          stats.rs:342-368
RunStats             stats.rs:371-394
MultiChainTracker    stats.rs:199-339 (device); ChainTracker stats.rs:24-131 runs
                     fused in the MH / NUTS kernels during run_progress
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib


def split_rhat_mean_ess(sample) -> tuple[np.ndarray, np.ndarray]:
    """sample: [chains, draws, params] (host array). Returns (rhat, ess), f32."""
    x = np.asarray(sample)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    x = np.ascontiguousarray(x)
    if x.ndim != 3:
        raise ValueError("sample must be [chains, draws, params]")
    c, n, p = x.shape
    rhat = np.empty(p, dtype=np.float32)
    ess = np.empty(p, dtype=np.float32)
    lib = _lib.require_gpu()
    _lib.check(lib.gm_split_rhat_ess(_lib.ptr(x), _lib.dtype_code(x.dtype), c, n, p,
                                     _lib.ptr(rhat), _lib.ptr(ess)))
    return rhat, ess


def split_rhat_mean_ess_device(dev_ptr: int, dtype, n_chains: int, n_draws: int, n_params: int,
                               strides: tuple[int, int, int]):
    """Same, on device memory (element strides: chain, draw, param)."""
    rhat = np.empty(n_params, dtype=np.float32)
    ess = np.empty(n_params, dtype=np.float32)
    lib = _lib.require_gpu()
    _lib.check(lib.gm_split_rhat_ess_device(C.c_void_p(dev_ptr), _lib.dtype_code(dtype), n_chains,
                                            n_draws, n_params, strides[0], strides[1], strides[2],
                                            _lib.ptr(rhat), _lib.ptr(ess)))
    return rhat, ess


@dataclass
class Summary:
    """Per-parameter posterior summary (stats.summary, DeviceSamples.summary);
    every array is f64 of length n_params, quantiles [len(probs), n_params]."""
    mean: np.ndarray
    sd: np.ndarray
    quantiles: np.ndarray
    rhat: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    probs: tuple

    def __str__(self) -> str:
        qh = "".join(f" {f'q{100 * p:g}':>10}" for p in self.probs)
        rows = [f"{'param':>6} {'mean':>10} {'sd':>10}{qh} {'rhat':>7} {'ess_bulk':>9} {'ess_tail':>9}"]
        for p in range(len(self.mean)):
            q = "".join(f" {v:10.4g}" for v in self.quantiles[:, p])
            rows.append(f"{p:>6} {self.mean[p]:10.4g} {self.sd[p]:10.4g}{q} {self.rhat[p]:7.4f} "
                        f"{self.ess_bulk[p]:9.1f} {self.ess_tail[p]:9.1f}")
        return "\n".join(rows)


def _summary_call(call, n_params: int, probs) -> Summary:
    probs = tuple(float(p) for p in probs)
    pr = np.asarray(probs, dtype=np.float64)
    f = {n: np.empty(n_params) for n in ("mean", "sd", "rhat", "ess_bulk", "ess_tail")}
    f["quantiles"] = np.empty((len(probs), n_params))
    out = _lib.gm_summary_out(**{n: a.ctypes.data for n, a in f.items()})
    _lib.check(call(len(probs), _lib.ptr(pr), C.byref(out)))
    return Summary(probs=probs, **f)


def _sample_array(sample) -> np.ndarray:
    x = np.asarray(sample)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    x = np.ascontiguousarray(x)
    if x.ndim != 3:
        raise ValueError("sample must be [chains, draws, params]")
    return x


def summary(sample, probs=(0.05, 0.5, 0.95)) -> Summary:
    """Posterior summary of a host [chains, draws, params] sample (draws >= 4),
    computed on the GPU in the sample's own dtype (f32 or f64): mean, sd
    (ddof = 1) and quantiles (numpy's linear interpolation) of the draws, and
    the rank-normalised diagnostics of Vehtari et al. 2021: rhat = the larger of
    the bulk and the folded split-R-hat, ess_bulk, ess_tail (5 % / 95 %).

    Differences from Stan / ArviZ: the ESS is this project's Appendix-B
    estimator (Geyer's initial monotone sequence as in split_rhat_mean_ess)
    without the M log10(M) cap, and the tail indicators use the order
    statistic floor((M - 1) q) rather than an interpolated quantile. rhat has
    the usual orientation sqrt(V/W) >= 1; split_rhat_mean_ess keeps the
    reference's sqrt(W/V). A parameter with a non-finite draw is NaN
    throughout; a constant one has NaN rhat / ESS."""
    x = _sample_array(sample)
    c, n, p = x.shape
    lib = _lib.require_gpu()
    return _summary_call(lambda k, pr, out: lib.gm_summary(_lib.ptr(x), _lib.dtype_code(x.dtype), c, n, p, k, pr,
                                                           out), p, probs)


def summary_device(dev_ptr: int, dtype, n_chains: int, n_draws: int, n_params: int,
                   strides: tuple[int, int, int], probs=(0.05, 0.5, 0.95)) -> Summary:
    """Same, on device memory (element strides: chain, draw, param)."""
    lib = _lib.require_gpu()
    return _summary_call(lambda k, pr, out: lib.gm_summary_device(
        C.c_void_p(dev_ptr), _lib.dtype_code(dtype), n_chains, n_draws, n_params, strides[0], strides[1],
        strides[2], k, pr, out), n_params, probs)


def rank_normalize(sample, folded: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(ranks, z) of a host [chains, draws, params] sample, both f64 of the
    sample's shape: the 1-based tie-averaged ranks of the pooled split draws
    (first and last draws // 2 of every chain; an odd count's middle draw is
    NaN) and their normal scores Phi^-1((r - 3/8) / (M + 1/4)); folded: those
    of |x - pooled median|."""
    x = _sample_array(sample)
    c, n, p = x.shape
    r = np.empty(x.shape)
    z = np.empty(x.shape)
    lib = _lib.require_gpu()
    _lib.check(lib.gm_rank_normalize(_lib.ptr(x), _lib.dtype_code(x.dtype), c, n, p, int(bool(folded)),
                                     _lib.ptr(r), _lib.ptr(z)))
    return r, z


def sort_plan() -> dict:
    """The summary sort's internal sizes (gm_summary_sort_plan)."""
    v = (C.c_int32 * 4)()
    _lib.check(_lib.load().gm_summary_sort_plan(v, 4))
    return {"lds_max": v[0], "tile": v[1], "radix_bits": v[2], "chunk_params": v[3]}


@dataclass
class WAIC:
    """GLMPrediction.waic(): elpd_i = lppd_i - ll_var_i per data row."""
    elpd_waic: float
    p_waic: float
    se: float
    waic: float
    pointwise: np.ndarray
    n_high_variance: int

    def __str__(self) -> str:
        rows = [f"{'elpd_waic':>10} {'se':>10} {'p_waic':>10} {'waic':>10}",
                f"{self.elpd_waic:10.4g} {self.se:10.4g} {self.p_waic:10.4g} {self.waic:10.4g}"]
        if self.n_high_variance:
            rows.append(f"{self.n_high_variance} of {len(self.pointwise)} rows have a pointwise variance above "
                        f"{GLMPrediction.HIGH_VARIANCE}")
        return "\n".join(rows)


@dataclass
class GLMPrediction:
    """GLM.predict: per data row, over all draws, in f64: mean and sd of the
    linear predictor eta and of the mean response mu and, when y is known, the
    log pointwise predictive density lppd and the mean and variance of the
    pointwise log-likelihood (None without y). pointwise: the matrix
    ll [n_draws, n_rows] in the draws' dtype, when asked for."""
    eta_mean: np.ndarray
    eta_sd: np.ndarray
    mu_mean: np.ndarray
    mu_sd: np.ndarray
    lppd: np.ndarray | None
    ll_mean: np.ndarray | None
    ll_var: np.ndarray | None
    pointwise: np.ndarray | None
    n_draws: int

    HIGH_VARIANCE = 0.4  # Vehtari, Gelman & Gabry 2017: WAIC is unreliable for rows above it

    @property
    def lppd_total(self) -> float:
        self._need_y()
        return float(np.sum(self.lppd))

    def _need_y(self):
        if self.lppd is None:
            raise ValueError("GLM predict: lppd and WAIC need y")

    def waic(self) -> WAIC:
        self._need_y()
        elpd = self.lppd - self.ll_var
        m = len(elpd)
        se = float(np.sqrt(m * np.var(elpd, ddof=1))) if m > 1 else float("nan")
        total = float(np.sum(elpd))
        return WAIC(total, float(np.sum(self.ll_var)), se, -2.0 * total, elpd,
                    int(np.sum(self.ll_var > self.HIGH_VARIANCE)))

    def __str__(self) -> str:
        ll = self.lppd is not None
        head = f"{'row':>6} {'eta_mean':>10} {'eta_sd':>10} {'mu_mean':>10} {'mu_sd':>10}"
        if ll:
            head += f" {'lppd':>10} {'ll_mean':>10} {'ll_var':>10}"
        rows = [head]
        for m in range(len(self.eta_mean)):
            r = f"{m:>6} {self.eta_mean[m]:10.4g} {self.eta_sd[m]:10.4g} {self.mu_mean[m]:10.4g} {self.mu_sd[m]:10.4g}"
            if ll:
                r += f" {self.lppd[m]:10.4g} {self.ll_mean[m]:10.4g} {self.ll_var[m]:10.4g}"
            rows.append(r)
        if ll:
            rows.append(f"lppd {self.lppd_total:.6g} over {self.n_draws} draws")
        return "\n".join(rows)


def predict_plan() -> dict:
    """The GLM prediction's internal sizes (gm_glm_predict_plan)."""
    v = (C.c_int32 * 3)()
    _lib.check(_lib.load().gm_glm_predict_plan(v, 3))
    return {"slab_draws": v[0], "tile_rows": v[1], "mfma_draws": v[2]}


@dataclass
class GLMLoo:
    """GLM.loo: PSIS-LOO per data row, f64. elpd_loo and pareto_k are NaN for a
    row with a non-finite pointwise log-likelihood (n_nonfinite of them);
    pareto_k is +inf where nothing could be fitted. lppd is GLM.predict's;
    tail [n_rows, tail_len] is the sorted raw tail, when asked for."""
    elpd_loo: np.ndarray
    pareto_k: np.ndarray
    lppd: np.ndarray
    tail: np.ndarray | None
    tail_len: int
    n_nonfinite: int
    n_draws: int

    @property
    def elpd_loo_sum(self) -> float:
        return float(np.sum(self.elpd_loo))

    @property
    def p_loo(self) -> float:
        return float(np.sum(self.lppd - self.elpd_loo))

    @property
    def se(self) -> float:
        m = len(self.elpd_loo)
        return float(np.sqrt(m * np.var(self.elpd_loo, ddof=1))) if m > 1 else float("nan")

    @property
    def looic(self) -> float:
        return -2.0 * self.elpd_loo_sum

    @property
    def k_threshold(self) -> float:
        """min(1 - 1 / log10(S), 0.7), Vehtari et al. 2024"""
        with np.errstate(divide="ignore"):
            return float(min(1.0 - 1.0 / np.log10(float(self.n_draws)), 0.7))

    @property
    def bad_rows(self) -> np.ndarray:
        """Rows with pareto_k above k_threshold (+inf counts, NaN does not)."""
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(self.pareto_k > self.k_threshold)

    @property
    def n_bad_k(self) -> int:
        return int(len(self.bad_rows))

    def __str__(self) -> str:
        rows = [f"{'elpd_loo':>10} {'se':>10} {'p_loo':>10} {'looic':>10}",
                f"{self.elpd_loo_sum:10.4g} {self.se:10.4g} {self.p_loo:10.4g} {self.looic:10.4g}"]
        if self.n_bad_k:
            rows.append(f"{self.n_bad_k} of {len(self.elpd_loo)} rows have a Pareto k above {self.k_threshold:.3g}")
        if self.n_nonfinite:
            rows.append(f"{self.n_nonfinite} rows have a non-finite pointwise log-likelihood")
        return "\n".join(rows)


def loo_plan(dtype=np.float32, n_draws: int = 1, n_rows: int = 1, reff: float = 1.0, workspace_bytes: int = 0) -> dict:
    """The split of a GLM.loo call (gm_glm_loo_plan), without a device."""
    v = (C.c_int64 * 7)()
    _lib.check(_lib.load().gm_glm_loo_plan(_lib.dtype_code(dtype), n_draws, n_rows, float(reff), int(workspace_bytes),
                                           v, 7))
    return {"tail_len": v[0], "group_rows": v[1], "workspace_bytes": v[2], "row_bytes": v[3],
            "default_workspace_bytes": v[4], "max_draws": v[5], "sort_slots": v[6]}


@dataclass
class BasicStats:
    name: str
    min: float
    median: float
    max: float
    mean: float
    std: float

    def __str__(self) -> str:
        return (f"{self.name} in [{self.min:.2f}, {self.max:.2f}], median: {self.median:.2f}, "
                f"mean: {self.mean:.2f} ± {self.std:.2f}")


def basic_stats(name: str, data) -> BasicStats:
    """stats.rs:342-368: sort descending; min = last, max = first, median =
    element len/2 of the descending order; std with ddof = 1."""
    d = np.sort(np.asarray(data, dtype=np.float32))[::-1]
    std = float(np.std(d, ddof=1)) if len(d) > 1 else float("nan")
    return BasicStats(name, float(d[-1]), float(d[len(d) // 2]), float(d[0]),
                      float(np.mean(d, dtype=np.float32)), std)


@dataclass
class RunStats:
    ess: BasicStats
    rhat: BasicStats

    @classmethod
    def from_sample(cls, sample) -> "RunStats":
        rhat, ess = split_rhat_mean_ess(sample)
        return cls.from_arrays(rhat, ess)

    @classmethod
    def from_arrays(cls, rhat, ess) -> "RunStats":
        return cls(basic_stats("ESS", ess), basic_stats("Split R-hat", rhat))

    def __str__(self) -> str:
        return f"{self.ess}\n{self.rhat}"


# ---- live run_progress statistics (stats.rs:24-339) ----------------------

class Progress(NamedTuple):
    """One progress report of run_progress: transitions done of total, the
    tracker acceptance estimate and max R-hat (NaN skipped)."""
    done: int
    total: int
    p_accept: float
    max_rhat: float


@dataclass
class ChainStats:
    """ChainTracker::stats (stats.rs:35-46, 122-131) for every chain."""
    n: int
    p_accept: np.ndarray  # [C]
    mean: np.ndarray      # [C, dim]
    sm2: np.ndarray       # [C, dim]


def _print_progress(prefix: str):
    """A one-line progress bar on stderr in the reference's format
    ("{prefix:8} {bar:40} {pos}/{len} | p(accept)≈.. max(rhat)≈..")."""
    import sys

    def show(p: Progress):
        frac = p.done / p.total if p.total else 1.0
        fill = int(round(40 * frac))
        bar = "=" * max(fill - 1, 0) + (">" if 0 < fill < 40 else "=" if fill else "") + "-" * (40 - fill)
        msg = f"p(accept)≈{p.p_accept:.2f} max(rhat)≈{p.max_rhat:.2f}"
        end = "\n" if p.done >= p.total else "\r"
        sys.stderr.write(f"{prefix:8} {bar} {p.done}/{p.total} | {msg}{end}")
        sys.stderr.flush()
    return show


class MultiChainTracker:
    """MultiChainTracker (stats.rs:199-339) on the device: step() with the
    [n_chains, n_params] positions (host array, or a device pointer with
    its dtype), then p_accept / rhat() / max_rhat()."""

    def __init__(self, n_chains: int, n_params: int):
        self.lib = _lib.require_gpu()
        self.n_chains, self.n_params = int(n_chains), int(n_params)
        h = C.c_void_p()
        _lib.check(self.lib.gm_mct_create(self.n_chains, self.n_params, C.byref(h)))
        self.h = h
        self._dev = None

    def step(self, x=None, *, dev_ptr: int | None = None, dtype=np.float32) -> None:
        if dev_ptr is None:
            a = np.ascontiguousarray(x)
            if a.shape != (self.n_chains, self.n_params):
                raise ValueError("positions must be [n_chains, n_params]")
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            if self._dev is None or self._dev.dtype != a.dtype:
                from .batch_vector import DeviceMatrix
                self._dev = DeviceMatrix(a.shape, a.dtype)
            _lib.check(self.lib.gm_memcpy_htod(C.c_void_p(self._dev.ptr), _lib.ptr(a), a.nbytes))
            dev_ptr, dtype = self._dev.ptr, a.dtype
        _lib.check(self.lib.gm_mct_step(self.h, C.c_void_p(dev_ptr), _lib.dtype_code(dtype)))

    @property
    def p_accept(self) -> float:
        p = C.c_float()
        _lib.check(self.lib.gm_mct_stats(self.h, C.byref(p), None, None))
        return p.value

    def rhat(self) -> np.ndarray:
        r = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self.lib.gm_mct_stats(self.h, None, _lib.ptr(r), None))
        return r

    def max_rhat(self) -> float:
        m = C.c_float()
        _lib.check(self.lib.gm_mct_stats(self.h, None, None, C.byref(m)))
        return m.value

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.gm_mct_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- per-transition sampler statistics (gm_sampler_set_stats) ----------------
_STAT_FIELDS = {"energy": (0, None), "accept_stat": (1, None), "step_size": (2, None),
                "n_leapfrog": (3, np.int32), "tree_depth": (4, np.int32),
                "divergent": (5, np.bool_), "accepted": (6, np.bool_)}


@dataclass
class StatsSummary:
    """The device reduction of a range of a run's sampler statistics
    (SamplerStats.summary): per-chain arrays [n_chains] in f64 and the totals
    over chains. E-BFMI = sum (E_n - E_{n-1})^2 / sum (E_n - mean E)^2."""
    n_transitions: int
    ebfmi: np.ndarray
    n_divergent: np.ndarray
    mean_accept_stat: np.ndarray
    mean_n_leapfrog: np.ndarray
    mean_tree_depth: np.ndarray
    n_max_depth: np.ndarray
    n_energy: np.ndarray
    n_skipped: np.ndarray
    total: dict

    def __str__(self) -> str:
        t = self.total
        c, n = len(self.ebfmi), self.n_transitions
        rows = [f"{n} transitions x {c} chains",
                f"divergent transitions  {int(t['n_divergent'])} ({int((self.n_divergent > 0).sum())} chains)",
                f"E-BFMI                 {t['ebfmi']:.4g} (lowest chain "
                f"{np.nanmin(self.ebfmi) if np.isfinite(self.ebfmi).any() else float('nan'):.4g})",
                f"mean accept_stat       {t['mean_accept_stat']:.4g}",
                f"mean n_leapfrog        {t['mean_n_leapfrog']:.4g}",
                f"mean tree_depth        {t['mean_tree_depth']:.4g}",
                f"reached max_depth      {int(t['n_max_depth'])}",
                f"non-finite energies    {int(t['n_skipped'])}"]
        return "\n".join(rows)


_SUMMARY_NAMES = ("ebfmi", "n_divergent", "mean_accept_stat", "mean_n_leapfrog", "mean_tree_depth",
                  "n_max_depth", "n_energy", "n_skipped")


class SamplerStats:
    """The per-transition statistics of a sampler's last run (after
    Sampler.collect_stats): arrays [n_chains, n_transitions], copied from the
    device when first read. Stale, like DeviceSamples, once the sampler runs
    again.

    Transition n_warmup + k produced sample row first_row + k of the run;
    first_row is 0, except after NUTS.run(n, 0), whose row 0 is the start
    state and has no transition (first_row 1). In "collected" mode n_warmup is
    0; in "all" mode the first n_warmup transitions are the discarded ones."""

    def __init__(self, owner):
        self.owner = owner
        self.generation = owner._gen
        n, fc, fr, rb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(owner._lib.gm_sampler_stats_info(owner._h, C.byref(n), C.byref(fc), C.byref(fr), C.byref(rb)))
        self.n_transitions, self.n_warmup, self.first_row, self.record_bytes = n.value, fc.value, fr.value, rb.value
        self.n_chains = owner.n_chains
        self._cache = {}

    def _check_live(self):
        if self.owner._h is None or self.generation != self.owner._gen:
            raise RuntimeError("SamplerStats are stale: the sampler has run again (or was closed) "
                               "since they were produced")

    @property
    def ptr(self) -> int:
        """The records on the device, [n_transitions][n_chains] (gmcmc.h)."""
        self._check_live()
        p = C.c_void_p()
        _lib.check(self.owner._lib.gm_sampler_stats_device(self.owner._h, C.byref(p)))
        return p.value or 0

    def _field(self, name: str) -> np.ndarray:
        self._check_live()
        if name not in self._cache:
            code, dt = _STAT_FIELDS[name]
            out = np.empty((self.n_chains, self.n_transitions), dtype=dt or self.owner.dtype)
            _lib.check(self.owner._lib.gm_sampler_stats_field(self.owner._h, code, _lib.ptr(out)))
            self._cache[name] = out
        return self._cache[name]

    energy = property(lambda self: self._field("energy"))
    accept_stat = property(lambda self: self._field("accept_stat"))
    step_size = property(lambda self: self._field("step_size"))
    n_leapfrog = property(lambda self: self._field("n_leapfrog"))
    tree_depth = property(lambda self: self._field("tree_depth"))
    divergent = property(lambda self: self._field("divergent"))
    accepted = property(lambda self: self._field("accepted"))

    def summary(self, warmup: bool = False, rows: tuple[int, int] | None = None) -> StatsSummary:
        """The reduction on the device of the collected transitions (with
        warmup: of every recorded one; rows = (first, count): of that range)."""
        self._check_live()
        r0, n = rows if rows is not None else ((0, self.n_transitions) if warmup else
                                               (self.n_warmup, self.n_transitions - self.n_warmup))
        if n == 0 and 0 <= r0 <= self.n_transitions:
            # nothing to reduce (e.g. a run that collected no row): zero counts, undefined ratios
            z = {k: (0.0 if k.startswith("n_") else float("nan")) for k in _SUMMARY_NAMES}
            return StatsSummary(0, *[np.full(self.n_chains, z[k]) for k in _SUMMARY_NAMES], z)
        pc = np.empty((len(_SUMMARY_NAMES), self.n_chains), dtype=np.float64)
        tot = np.empty(len(_SUMMARY_NAMES), dtype=np.float64)
        _lib.check(self.owner._lib.gm_sampler_stats_reduce(self.owner._h, r0, n, _lib.ptr(pc), _lib.ptr(tot)))
        return StatsSummary(int(n), *[pc[i] for i in range(len(_SUMMARY_NAMES))],
                            {k: float(tot[i]) for i, k in enumerate(_SUMMARY_NAMES)})
