"""hmc_kernel's leapfrog loop forms at one chain per wave: 1, 2 or 4 leapfrogs
per loop trip and the long count-down form (U = 7 straight-line leapfrogs per
trip after (L - 1) % U single ones), each forced with gm_sampler_set_unroll.
Only the scalar bookkeeping differs between them, so every form gives the CPU
oracle's bits, and the log-densities of the other forms, at every leapfrog
count where a form takes another path: L = 0 and 1 run no loop step, 2 runs
one; U - 1 and U are the long form's single steps alone; U + 1 is one trip and
nothing else; 2U has a trip after U - 1 single steps, 2U + 1 two trips; the
bench's L = 50 is seven trips.

The shapes are those of the layout matrix (tests/_layout_cases.py): 5 chains at
chain offset 3 (two workgroups at 64 lanes per chain, the second with one live
wave), the layouts that compile the loop form in (64 x 1 and 64 x 2) at their
full and padded dims, both dtypes, RosenbrockND and the dense Gaussian, with
the matrix's step sizes. Those were chosen at L = 3. With the oracle alone, on
the CPU, they give both outcomes at every other leapfrog count of this file
but two: RosenbrockND accepts everything at L = 1 and rejects everything at
L = 50 (the integrator leaves its stable range), so these two take 1.5 and
0.75 times the matrix's step (EPS_SCALE). test_reference_accepts_and_rejects
asserts both outcomes for every case from L = 1 on; L = 0 proposes the
current position and always accepts.

The launch sequences of the last test start and end inside a draw block,
begin collecting inside one, and hold whole blocks inside the launch and the
collected range, under the automatic form and the long one; one oracle run
over all 157 transitions is the reference."""
import functools

import numpy as np
import pytest

from tests import _layout_cases as lc
from tests._oracle import Target

U = 7  # the long form's trip length (GM_LF_LONG, csrc/gm_launch.h) and its set_unroll number
FORMS = [1, 2, 4, U]
LS = [0, 1, 2, U - 1, U, U + 1, 2 * U, 2 * U + 1, 50]
CASES = [((64, 1), 64), ((64, 1), 61), ((64, 2), 128), ((64, 2), 125)]
CASE_IDS = [f"{lay[0]}x{lay[1]}-D{d}" for lay, d in CASES]
TARGETS = ["rosenbrock", "gauss"]
SEED, N_COLLECT, N_DISCARD = 11, 4, 2  # 6 transitions: a whole f32 draw block and half of the next
EPS_SCALE = {("rosenbrock", 1): 1.5, ("rosenbrock", 50): 0.75}  # (see above; 1 elsewhere)


def _eps(name, dim, L):
    return lc.HMC_EPS[name, dim] * EPS_SCALE.get((name, L), 1.0)


@functools.lru_cache(maxsize=None)
def _reference(g, oracle_lib, name, lay, dim, dtype, L):
    from tests._oracle import Oracle
    ot = Target.from_product(lc.target(g, name, dim), dim)
    q, samples, acc = Oracle(oracle_lib).hmc_run(ot, lc.start(g, dim, dtype), _eps(name, dim, L), L, SEED, 0,
                                                 N_COLLECT + N_DISCARD, N_DISCARD, *lay,
                                                 chain_offset=lc.CHAIN_OFFSET)
    out = (np.ascontiguousarray(samples.transpose(1, 0, 2)), q, acc)
    for a in out:
        a.setflags(write=False)
    return out


def _products():
    import general_mcmc_amd as g
    return g


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", TARGETS)
@pytest.mark.parametrize("lay,dim", CASES, ids=CASE_IDS)
def test_reference_accepts_and_rejects(oracle, lay, dim, name, dtype):
    """CPU: the oracle's accept counts of every case of test_every_form_bitwise
    (5 chains x 6 transitions): all accepted at L = 0, at least one proposal
    accepted and at least one rejected from L = 1 on."""
    g = _products()
    n = (N_COLLECT + N_DISCARD) * lc.N_CHAINS
    for L in LS:
        acc = int(_reference(g, oracle.lib, name, lay, dim, np.dtype(dtype).name, L)[2].sum())
        print(f"{name} {lay} D={dim} {np.dtype(dtype).name} L={L}: {acc}/{n} accepted")
        if L == 0:
            assert acc == n
        else:
            assert 0 < acc < n, f"L={L}: {acc} of {n} accepted"


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", TARGETS)
@pytest.mark.parametrize("lay,dim", CASES, ids=CASE_IDS)
def test_every_form_bitwise(gm, oracle, lay, dim, name, dtype, L):
    samples, q, acc = _reference(gm, oracle.lib, name, lay, dim, np.dtype(dtype).name, L)
    x0, t = lc.start(gm, dim, dtype), lc.target(gm, name, dim)
    logps = []
    for form in FORMS:
        s = gm.HMC(t, x0, _eps(name, dim, L), L, dtype=dtype, chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
        s.set_layout(*lay)
        s.set_unroll(form)
        out = s.run(N_COLLECT, N_DISCARD)
        msg = f"form {form}"
        np.testing.assert_array_equal(out, samples, err_msg=msg)
        np.testing.assert_array_equal(s.positions(), q, err_msg=msg)
        np.testing.assert_array_equal(s.accept_counts(), acc, err_msg=msg)
        logps.append(s.logp())
        s.close()
    assert np.isfinite(logps[0]).all()
    for form, lp in zip(FORMS[1:], logps[1:]):
        np.testing.assert_array_equal(lp, logps[0], err_msg=f"logp of form {form} against form 1")


# (n_collect, n_discard) of consecutive run_positions calls on one sampler:
# steps 0, 1..5, 6..16, 17..25 and 26..156. In f32 (4 transitions per draw
# block) the launches start at positions 0, 1, 2, 1, 2 of a block and end at
# 1, 2, 1, 2, 1; (3, 2) and (5, 6) begin collecting inside a block; (9, 0) and
# (130, 1) hold whole blocks that are collected throughout, and (130, 1)
# crosses the accept windows at steps 64 and 128.
SEQUENCE = [(1, 0), (3, 2), (5, 6), (9, 0), (130, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, U], ids=["auto", "long"])
@pytest.mark.parametrize("lay,dim,dtype", [((64, 1), 64, np.float32), ((64, 1), 61, np.float32),
                                           ((64, 2), 125, np.float32), ((64, 1), 64, np.float64)],
                         ids=["64x1-D64-f32", "64x1-D61-f32", "64x2-D125-f32", "64x1-D64-f64"])
def test_launch_sequence_against_one_oracle_run(gm, oracle, lay, dim, dtype, form):
    L, name = 2 * U + 1, "rosenbrock"
    eps = lc.HMC_EPS[name, dim]
    x0, t = lc.start(gm, dim, dtype), lc.target(gm, name, dim)
    total = sum(nc + nd for nc, nd in SEQUENCE)
    # collect_from = 0: every transition of the one oracle run, rows by step
    q, rows, acc = oracle.hmc_run(Target.from_product(t, dim), x0, eps, L, SEED, 0, total, 0, *lay,
                                  chain_offset=lc.CHAIN_OFFSET)
    assert 0 < acc.sum() < total * lc.N_CHAINS  # both outcomes
    s = gm.HMC(t, x0, eps, L, dtype=dtype, chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
    s.set_layout(*lay)
    s.set_unroll(form)
    step = 0
    for nc, nd in SEQUENCE:
        got = s.run_positions(nc, nd).to_host()  # [C, nc, D]
        np.testing.assert_array_equal(got, rows[step + nd:step + nd + nc].transpose(1, 0, 2),
                                      err_msg=f"run_positions({nc}, {nd})")
        step += nc + nd
    np.testing.assert_array_equal(s.positions(), q)
    np.testing.assert_array_equal(s.accept_counts(), acc)
    s.close()
