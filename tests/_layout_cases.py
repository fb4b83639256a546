"""The layout matrix: every (lanes per chain, elements per lane) layout the
sampling kernels are compiled for (GM_LAYOUT_LIST, csrc/gm_layouts.h), the
dims each one is run at, and the CPU oracle's runs that the GPU samplers are
compared with (tests/test_gpu_layout_matrix.py). A plain helper module: the
oracle runs are computed once per (sampler, target, layout, dim, dtype),
shared by the GPU tests and the CPU test that checks their conditions
(tests/test_layout_matrix_cases.py), and read-only.

Per layout two dims: D_full = lanes * elems and D_pad = lanes * elems - 3,
which pads three whole lanes at E = 1, one and a half lanes at E = 2 and the
inside of the last lane at E >= 4. 1 x 1 and 2 x 1 have their full dim only
(a smaller one belongs to a narrower layout) and 4 x 1 has 4 and 3.

Every run has 5 chains at global chain ids 3..7: at 64 lanes per chain that
is two workgroups, the second with one live wave; narrower lane groups leave
a partly filled wave.

HMC_EPS was chosen on the CPU with the oracle alone (L = 3, these starts, the
12 transitions of HMC_RUNS, both dtypes, every layout of the dim): a step
size from a grid whose accept fraction over the 5 x 12 proposals stays near
the middle (0.33-0.73) for all of the dim's layouts and both dtypes. The
fractions are in the table's comments; test_layout_matrix_cases.py asserts at
least 10 % accepted and at least 10 % rejected for every case.
"""
from __future__ import annotations

import functools

import numpy as np

from tests._oracle import Target

LAYOUTS = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (16, 2), (32, 2), (64, 2),
           (8, 4), (16, 4), (32, 4), (64, 4), (16, 8), (32, 8), (64, 8), (64, 16)]
DTYPES = [np.float32, np.float64]
TARGETS = ("rosenbrock", "iso", "gauss")
N_CHAINS, CHAIN_OFFSET, START_SEED, START_SCALE = 5, 3, 3, 0.5


def dims(lay):
    """[D_full, D_pad] of a layout (see the module docstring)."""
    full = lay[0] * lay[1]
    if full <= 2:
        return [full]
    return [full, 3 if full == 4 else full - 3]


CASES = [(lay, d) for lay in LAYOUTS for d in dims(lay)]
CASE_IDS = [f"{lay[0]}x{lay[1]}-D{d}" for lay, d in CASES]


@functools.lru_cache(maxsize=None)
def _targets(g, dim):
    rng = np.random.default_rng(dim)
    a = rng.standard_normal((dim, dim))
    cov = a @ a.T / dim + np.eye(dim)
    mean = rng.standard_normal(dim)
    return {"rosenbrock": g.RosenbrockND(), "iso": g.IsotropicGaussian(1.7),
            "gauss": g.DenseGaussian(mean, cov)}


def target(g, name, dim):
    """The built-in targets of test_gpu_parity.targets."""
    return _targets(g, dim)[name]


def start(g, dim, dtype, n=N_CHAINS):
    x = (g.init_with_seed(n, dim, START_SEED, np.float64) * START_SCALE).astype(dtype)
    x.setflags(write=False)
    return x


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- HMC ---------------------------------------------------------------------
HMC_L, HMC_SEED = 3, 11
HMC_RUNS = [(3, 2), (4, 3)]  # (n_collect, n_discard): the second launch starts at step 5
HMC_TRANSITIONS = sum(nc + nd for nc, nd in HMC_RUNS)

# (target, D) -> step size; comment: accept fraction of the 60 proposals,
# lowest - highest over the dim's layouts and both dtypes
HMC_EPS = {
    # RosenbrockND at D = 1 has no term: its log-density is 0 everywhere, the
    # gradient is 0 and every proposal is accepted at any step size (FLAT)
    ("rosenbrock", 1): 0.08,     # 1.00
    ("rosenbrock", 2): 0.08,     # 0.47
    ("rosenbrock", 3): 0.08,     # 0.35-0.48
    ("rosenbrock", 4): 0.068,    # 0.50-0.53
    ("rosenbrock", 5): 0.06,     # 0.70-0.73
    ("rosenbrock", 8): 0.06,     # 0.48-0.57
    ("rosenbrock", 13): 0.06,    # 0.33-0.38
    ("rosenbrock", 16): 0.06,    # 0.33-0.38
    ("rosenbrock", 29): 0.045,   # 0.52-0.60
    ("rosenbrock", 32): 0.045,   # 0.48-0.57
    ("rosenbrock", 61): 0.04,    # 0.43-0.50
    ("rosenbrock", 64): 0.04,    # 0.43-0.50
    ("rosenbrock", 125): 0.04,   # 0.47-0.58
    ("rosenbrock", 128): 0.04,   # 0.47-0.57
    ("rosenbrock", 253): 0.04,   # 0.47-0.60
    ("rosenbrock", 256): 0.04,   # 0.47-0.60
    ("rosenbrock", 509): 0.035,  # 0.45-0.48
    ("rosenbrock", 512): 0.035,  # 0.45-0.48
    ("rosenbrock", 1021): 0.035,  # 0.60-0.68
    ("rosenbrock", 1024): 0.035,  # 0.60-0.68
    ("iso", 1): 3.2,      # 0.38-0.52
    ("iso", 2): 2.6,      # 0.60-0.63
    ("iso", 3): 2.6,      # 0.53-0.57
    ("iso", 4): 2.3,      # 0.55-0.57
    ("iso", 5): 2.3,      # 0.42-0.52
    ("iso", 8): 2.0,      # 0.68
    ("iso", 13): 2.0,     # 0.53-0.60
    ("iso", 16): 2.0,     # 0.43-0.50
    ("iso", 29): 1.3,     # 0.57-0.63
    ("iso", 32): 1.15,    # 0.55-0.63
    ("iso", 61): 0.9,     # 0.45-0.58
    ("iso", 64): 0.9,     # 0.45-0.47
    ("iso", 125): 0.7,    # 0.40-0.50
    ("iso", 128): 0.7,    # 0.40-0.48
    ("iso", 253): 0.5,    # 0.45-0.62
    ("iso", 256): 0.5,    # 0.45-0.62
    ("iso", 509): 0.4,    # 0.50-0.62
    ("iso", 512): 0.4,    # 0.50-0.62
    ("iso", 1021): 0.3,   # 0.67-0.68
    ("iso", 1024): 0.3,   # 0.67-0.68
    ("gauss", 1): 2.0,    # 0.37-0.52
    ("gauss", 2): 1.9,    # 0.48-0.50
    ("gauss", 3): 1.85,   # 0.45-0.47
    ("gauss", 4): 1.8,    # 0.60-0.62
    ("gauss", 5): 1.5,    # 0.60
    ("gauss", 8): 1.7,    # 0.60-0.67
    ("gauss", 13): 1.5,   # 0.50-0.52
    ("gauss", 16): 1.3,   # 0.43-0.60
    ("gauss", 29): 1.3,   # 0.53-0.62
    ("gauss", 32): 1.3,   # 0.45-0.55
    ("gauss", 61): 0.8,   # 0.63-0.65
    ("gauss", 64): 1.15,  # 0.62-0.67
    ("gauss", 125): 0.8,  # 0.48-0.53
    ("gauss", 128): 0.7,  # 0.50-0.58
    ("gauss", 253): 0.6,  # 0.58
    ("gauss", 256): 0.7,  # 0.53-0.57
    ("gauss", 509): 0.5,  # 0.55-0.62
    ("gauss", 512): 0.5,  # 0.58-0.63
    ("gauss", 1021): 0.45,  # 0.50-0.63
    ("gauss", 1024): 0.35,  # 0.63
}
# (target, D) whose log-density is constant: every HMC and MH proposal is
# accepted, every NUTS tree runs to max_depth. The cases still run; the
# both-branches conditions are asserted for the other two targets of the case.
FLAT = {("rosenbrock", 1)}


def hmc_reference(g, oracle, name, lay, dim, dtype, eps=None):
    """Per run of HMC_RUNS: (samples [C, n_collect, D], positions after the
    run, accept counts since the start), the oracle continued from its own
    state."""
    return _hmc_reference(g, oracle.lib, name, lay, dim, np.dtype(dtype).name,
                          HMC_EPS[name, dim] if eps is None else eps)


@functools.lru_cache(maxsize=None)
def _hmc_reference(g, oracle_lib, name, lay, dim, dtype, eps):
    from tests._oracle import Oracle
    oracle = Oracle(oracle_lib)
    ot = Target.from_product(target(g, name, dim), dim)
    q, step0 = start(g, dim, dtype), 0
    total = np.zeros(N_CHAINS, dtype=np.int64)
    out = []
    for nc, nd in HMC_RUNS:
        q, samples, acc = oracle.hmc_run(ot, q, eps, HMC_L, HMC_SEED, step0, nc + nd, nd, *lay,
                                         chain_offset=CHAIN_OFFSET)
        total = total + acc
        out.append(_frozen(np.ascontiguousarray(samples.transpose(1, 0, 2)), q, total))
        step0 += nc + nd
    return out


# ---- MH ----------------------------------------------------------------------
MH_SEED = 3
# start steps 0, 66 and 71 (residues 0, 2 and 7 modulo 64); the accept-window
# boundaries at steps 64 and 128 each fall inside a launch
MH_RUNS = [(60, 6), (5, 0), (70, 0)]
MH_TRANSITIONS = sum(nc + nd for nc, nd in MH_RUNS)


def mh_prop_std(dim):
    return 2.38 / np.sqrt(dim)


def mh_reference(g, oracle, name, lay, dim, dtype):
    """Per run of MH_RUNS: (samples [C, n_collect, D] as float64, accept
    counts since the start), one oracle run continued across the three."""
    return _mh_reference(g, oracle.lib, name, lay, dim, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _mh_reference(g, oracle_lib, name, lay, dim, dtype):
    from tests._oracle import Oracle
    oracle = Oracle(oracle_lib)
    ot = Target.from_product(target(g, name, dim), dim)
    q, step0 = start(g, dim, dtype), 0
    total = np.zeros(N_CHAINS, dtype=np.int64)
    out = []
    for nc, nd in MH_RUNS:
        q, samples, acc = oracle.mh_run(ot, q, mh_prop_std(dim), MH_SEED, step0, nc + nd, nd, *lay,
                                        chain_offset=CHAIN_OFFSET)
        total = total + acc
        out.append(_frozen(samples.transpose(1, 0, 2).astype(np.float64), total))
        step0 += nc + nd
    return out


# ---- NUTS (identity metric) ----------------------------------------------------
NUTS_SEED, NUTS_TARGET_ACCEPT, NUTS_MAX_DEPTH, NUTS_STEPS_PER_LAUNCH = 9, 0.8, 5, 3
NUTS_RUNS = [(5, 4), (2, 0)]
# a run(n_collect, n_discard) returns the start and n_collect + n_discard - 1
# transitions (ChainRunner::run semantics)
NUTS_TRANSITIONS = sum(nc + nd - 1 for nc, nd in NUTS_RUNS)


def nuts_reference(g, oracle, name, lay, dim, dtype):
    """Per run of NUTS_RUNS: (samples [C, n_collect, D], accept counts and
    leapfrog counts since the start, eps, eps_bar)."""
    return _nuts_reference(g, oracle.lib, name, lay, dim, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _nuts_reference(g, oracle_lib, name, lay, dim, dtype):
    from tests._oracle import Oracle
    oracle = Oracle(oracle_lib)
    ot = Target.from_product(target(g, name, dim), dim)
    q, step0 = start(g, dim, dtype), 0
    st = oracle.nuts_state(N_CHAINS, np.dtype(dtype))
    acc_t = np.zeros(N_CHAINS, dtype=np.int64)
    nlf_t = np.zeros(N_CHAINS, dtype=np.int64)
    out = []
    for nc, nd in NUTS_RUNS:
        q, samples, acc, nlf = oracle.nuts_run(ot, q, st, NUTS_TARGET_ACCEPT, NUTS_MAX_DEPTH, NUTS_SEED,
                                               step0, nc, nd, False, *lay, chain_offset=CHAIN_OFFSET)
        acc_t, nlf_t = acc_t + acc, nlf_t + nlf
        out.append(_frozen(np.ascontiguousarray(samples.transpose(1, 0, 2)), acc_t, nlf_t,
                           st["eps"].copy(), st["eps_bar"].copy()))
        step0 += nc + nd
    return out
