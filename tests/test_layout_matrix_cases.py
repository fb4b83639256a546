"""The layout matrix's cases, checked on the CPU: the list is the compiled
one, and on the oracle alone every case takes both branches of each sampler's
decision, so the bitwise GPU tests (tests/test_gpu_layout_matrix.py) cannot
pass trivially.

Conditions, per target of a case (layout x dim x dtype):
* HMC: at least 10 % of the 5 x 12 proposals accepted and at least 10 %
  rejected.
* MH, 5 x 141 proposals at the proposal sd 2.38 / sqrt(D): the same for the
  isotropic and the dense Gaussian (0.31-0.62 accepted). RosenbrockND accepts
  0.011-0.038 of them at that sd at every D >= 2 (1-8 per chain, some chains
  none), so for it the test asks for accepted and rejected proposals in every
  case, and the 10 % / 10 % rule holds for the case's three targets together.
* NUTS: the per-chain leapfrog counts over the 9 transitions are not all
  equal and their mean exceeds 3 per transition. At D = 1 the bound is 2: a
  one-dimensional trajectory turns back within half a period, which at the
  step size dual averaging settles on is 2-4 leapfrogs, so the trees are one
  or two doublings (1 or 3 leapfrogs) and seldom three; a mean above 2 still
  needs transitions with merged subtrees (oracle: 2.02-2.69; the other dims
  3.1-27).
* RosenbrockND at D = 1 (layout 1 x 1 only) is flat: its log-density is 0, so
  HMC and MH accept every proposal and every NUTS transition is the same
  tree. The test asserts exactly that; the 1 x 1 case takes both branches
  with its two Gaussian targets.
"""
import os
import re

import numpy as np
import pytest

from tests import _layout_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matrix_is_the_compiled_list():
    with open(os.path.join(ROOT, "general-mcmc_amd", "csrc", "gm_layouts.h")) as f:
        text = f.read()
    m = re.search(r"#define\s+GM_LAYOUT_LIST\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", text)
    assert m, "GM_LAYOUT_LIST not found"
    compiled = [(int(a), int(b)) for a, b in re.findall(r"\bX\(\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]
    assert len(compiled) == len(set(compiled))
    assert compiled == lc.LAYOUTS
    # every layout has its full dim and, from 4 x 1 on, a padded one
    assert {lay for lay, _ in lc.CASES} == set(lc.LAYOUTS)
    for lay, d in lc.CASES:
        full = lay[0] * lay[1]
        assert full // 2 < d <= full or full == 1
    assert all((name, d) in lc.HMC_EPS for name in lc.TARGETS for _, d in lc.CASES)


@pytest.fixture(scope="module")
def g():
    import general_mcmc_amd
    return general_mcmc_amd  # host side only: starts and target parameters


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("lay,dim", lc.CASES, ids=lc.CASE_IDS)
def test_cases_take_both_branches(g, oracle, lay, dim, dtype):
    n = lc.N_CHAINS
    pooled = {"hmc": 0, "mh": 0}
    for name in lc.TARGETS:
        flat = (name, dim) in lc.FLAT
        hmc = int(lc.hmc_reference(g, oracle, name, lay, dim, dtype)[-1][2].sum())
        mh = int(lc.mh_reference(g, oracle, name, lay, dim, dtype)[-1][1].sum())
        nlf = lc.nuts_reference(g, oracle, name, lay, dim, dtype)[-1][2]
        pooled["hmc"] += hmc
        pooled["mh"] += mh
        n_hmc, n_mh = n * lc.HMC_TRANSITIONS, n * lc.MH_TRANSITIONS
        per_transition = nlf.mean() / lc.NUTS_TRANSITIONS
        print(f"{name}: HMC {hmc}/{n_hmc}, MH {mh}/{n_mh}, NUTS leapfrogs {nlf.tolist()} "
              f"({per_transition:.2f} per transition)")
        if flat:
            assert hmc == n_hmc and mh == n_mh and len(set(nlf.tolist())) == 1
            continue
        assert 0.1 * n_hmc <= hmc <= 0.9 * n_hmc, name
        if name == "rosenbrock":
            assert 0 < mh < n_mh, name
        else:
            assert 0.1 * n_mh <= mh <= 0.9 * n_mh, name
        assert len(set(nlf.tolist())) > 1, name
        assert per_transition > (2 if dim == 1 else 3), name
    for key, per_target in (("hmc", n * lc.HMC_TRANSITIONS), ("mh", n * lc.MH_TRANSITIONS)):
        total = len(lc.TARGETS) * per_target
        assert 0.1 * total <= pooled[key] <= 0.9 * total, key
