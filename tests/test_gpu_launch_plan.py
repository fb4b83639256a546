"""The run drivers launch what the planner plans: last_run_stats()[1] of a
warm-up run equals the length of the plan recorded in
tests/golden/launch_plans.json (tests/test_launch_plan.py checks the planner
against those plans on the CPU), and the run's results do not depend on the
cut: steps_per_launch 7 and 1000 give the same bits."""
import json
import os

import numpy as np
import pytest

from tests.test_gpu_hmc_adapt import _target
from tests.test_gpu_nuts_whitening import _cfg, _rand_gauss

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
N_CHAINS, DIM = 64, 4
SB, EB, IW = 5, 10, 10
N_COLLECT, N_DISCARD = 20, 60


def _planned_launches(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")) as f:
        case = {c["name"]: c for c in json.load(f)["cases"]}[name]
    if case["sampler"] == "nuts":
        (run,) = case["runs"]
        # NUTS::run(20, 60) makes 79 transitions
        assert (run["total"], run["n_discard"]) == (N_COLLECT + N_DISCARD - 1, N_DISCARD)
        return len(run["launches"])
    assert (case["total"], case["warm"], case["sb"], case["eb"], case["iw"]) == (N_COLLECT + N_DISCARD, N_DISCARD, SB,
                                                                                 EB, IW)
    return len(case["launches"])


def _hmc(gm, dtype, adaptation):
    target, eps = _target(gm, "gauss", DIM)
    x0 = gm.init_with_seed(N_CHAINS, DIM, 22, np.float64).astype(dtype)
    cfg = gm.HMCAdaptConfig(adaptation, 0.8, SB, EB, IW, 0.05, 1e-6)
    return gm.HMC(target, x0, eps, 3, dtype=dtype).set_seed(4).set_adaptation(cfg)


def _nuts(gm, dtype):
    x0 = gm.init_with_seed(N_CHAINS, DIM, 22, np.float64).astype(dtype)
    return gm.NUTS.new_with_mass_matrix(_rand_gauss(gm, DIM, 5), x0, 0.8, _cfg(gm, "dense", SB, EB, IW, pooled=True),
                                        dtype=dtype).set_seed(4)


# sampler, its plans at steps_per_launch 7 and 1000 (None: not recorded).
# (64 chains x 4 dims: the slab holds more rows than a launch has, as with slab_rows 10^6)
CASES = {
    "hmc-diagonal": (lambda gm, dt: _hmc(gm, dt, "diagonal"), "adapt2-w60-c20-k7", "adapt2-w60-c20-k1000"),
    "hmc-dense": (lambda gm, dt: _hmc(gm, dt, "dense"), "dense-s1000000-w60-c20-k7", "dense-s1000000-w60-c20-k1000"),
    "nuts-pooled": (_nuts, "nuts-pooled-s1000000", None),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_launches_are_the_plan(gm, dtype, case):
    make, plan7, plan1000 = CASES[case]
    res = []
    for spl, plan in ((7, plan7), (1000, plan1000)):
        s = make(gm, dtype).set_steps_per_launch(spl)
        out = s.run(N_COLLECT, N_DISCARD)
        launches = s.last_run_stats()[1]
        print(f"{case} steps_per_launch {spl}: {launches} launches")
        if plan is not None:
            assert launches == _planned_launches(plan)
        res.append((out, s.positions(), s.accept_counts()) + tuple(s.step_sizes()))
        s.close()
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)
