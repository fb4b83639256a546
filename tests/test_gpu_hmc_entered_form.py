"""hmc_kernel's block leapfrog loop form (GM_LF_BLOCK = 49, csrc/gm_launch.h:
(L - 1) % U leapfrogs as a binary ladder of straight-line pieces of 1, 2, 4,
8, 16 and 32, then (L - 1) / U count-down passes of U = 49 straight-line
leapfrogs), compiled for one chain per wave at one element per lane and
RosenbrockND, forced with gm_sampler_set_unroll(49) and chosen automatically
from 1025 to 4096 chains where the long form (7) was. Only scalar control
differs from the other forms, so every L gives the CPU oracle's bits and form
1's log-densities.

The leapfrog counts are those at which the form takes another path: 0 and 1
run no loop step; 2 is one leapfrog from the ladder (the piece of 1), 3 the
piece of 2, 13 the pieces of 4 and 8, 48 all but the piece of 16, U = 49 the
pieces of 16 and 32; U + 1 = 50 (the bench's L) is one pass and no ladder,
U + 2 a piece of 1 and a pass, 2U + 1 two passes, 2U + 2 a piece and two
passes.

The shapes are those of the layout matrix (tests/_layout_cases.py): 5 chains
at chain offset 3, layout 64 x 1 at its full and padded dim, both dtypes. The
automatic choice is by the launch's waves per SIMD, so its case runs 1029
chains (more than one wave per SIMD of the MI355X's 256 CUs) and asserts the
form the launch took (gm_sampler_last_unroll).

RosenbrockND at the matrix's step size rejects everything at long L, so each
L takes a scale of it (EPS_SCALE) at which the oracle alone, on the CPU, both
accepts and rejects in every case of this file:
test_reference_accepts_and_rejects asserts that.

The launch sequence of the last test starts and ends launches inside a draw
block, begins collecting inside one, has whole blocks collected throughout
and whole blocks discarded, launches whose last block is whole, and one
launch across the accept windows at steps 64 and 128, in f32 (4 transitions
per draw block) and f64 (2); one oracle run over all 180 transitions is the
reference."""
import functools

import numpy as np
import pytest

from tests import _layout_cases as lc
from tests._oracle import Target

U = 49  # the block's length (GM_LF_BLOCK) and the form's set_unroll number
NEW, LONG = U, 7
LS = [0, 1, 2, 3, 13, U - 1, U, U + 1, U + 2, 2 * U + 1, 2 * U + 2]
assert 50 in LS
CASES = [((64, 1), 64), ((64, 1), 61)]
CASE_IDS = [f"{lay[0]}x{lay[1]}-D{d}" for lay, d in CASES]
NAME = "rosenbrock"
SEED, N_COLLECT, N_DISCARD = 11, 4, 2  # 6 transitions, as test_gpu_hmc_loop_forms.py
# the step size as a multiple of the matrix's (chosen at L = 3), per L
EPS_SCALE = {1: 1.5, **{L: 0.8 for L in LS if L >= U - 1}}
# the automatic choice: chains (one wave each), L
AUTO_CHAINS, AUTO_L = 1029, 50

# (n_collect, n_discard) of consecutive run_positions calls on one sampler:
# launches of steps 0, 1..5, 6..16, 17..25, 26..156, 157..165, 166..173 and
# 174..179. f32 (4 transitions per draw block): they start at positions 0, 1,
# 2, 1, 2, 1, 2, 2 of a block and end inside one but for the last, whose last
# block (176..179) is whole; (3, 2) begins collecting inside a block; (9, 0),
# (130, 1), (8, 0) and (6, 0) hold whole blocks collected throughout, (5, 6)
# and (0, 9) whole blocks discarded; (130, 1) crosses the accept windows at
# steps 64 and 128. f64 (2 per block): the launches from steps 1, 17 and 157
# start and end inside a block, (3, 2) begins collecting inside block 2..3,
# (5, 6), (9, 0)... as above, and the launches that end at steps 6, 26, 166,
# 174 and 180 end with a whole block.
SEQUENCE = [(1, 0), (3, 2), (5, 6), (9, 0), (130, 1), (0, 9), (8, 0), (6, 0)]
SEQ_L = U + 2  # a ladder piece and a pass
SEQ_CASES = [((64, 1), 64, np.float32, NEW), ((64, 1), 64, np.float32, LONG),
             ((64, 1), 61, np.float32, NEW), ((64, 1), 61, np.float32, LONG),
             ((64, 1), 64, np.float64, NEW), ((64, 1), 64, np.float64, LONG),
             ((64, 1), 61, np.float64, NEW), ((64, 1), 61, np.float64, LONG),
             ((64, 2), 125, np.float32, LONG)]
SEQ_IDS = [f"{lay[0]}x{lay[1]}-D{d}-{np.dtype(dt).name}-form{f}" for lay, d, dt, f in SEQ_CASES]


def _eps(dim, L):
    return lc.HMC_EPS[NAME, dim] * EPS_SCALE.get(L, 1.0)


def _products():
    import general_mcmc_amd as g
    return g


@functools.lru_cache(maxsize=None)
def _reference(g, oracle_lib, lay, dim, dtype, L, chains=lc.N_CHAINS):
    """(samples [C, 4, D], positions, accept counts) of the 6 transitions."""
    from tests._oracle import Oracle
    ot = Target.from_product(lc.target(g, NAME, dim), dim)
    q, samples, acc = Oracle(oracle_lib).hmc_run(ot, lc.start(g, dim, dtype, chains), _eps(dim, L), L, SEED, 0,
                                                 N_COLLECT + N_DISCARD, N_DISCARD, *lay,
                                                 chain_offset=lc.CHAIN_OFFSET)
    out = (np.ascontiguousarray(samples.transpose(1, 0, 2)), q, acc)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sequence_reference(g, oracle_lib, lay, dim, dtype):
    """(positions, every transition's state [180, C, D], accept counts) of one run."""
    from tests._oracle import Oracle
    total = sum(nc + nd for nc, nd in SEQUENCE)
    ot = Target.from_product(lc.target(g, NAME, dim), dim)
    out = Oracle(oracle_lib).hmc_run(ot, lc.start(g, dim, dtype), _eps(dim, SEQ_L), SEQ_L, SEED, 0, total, 0, *lay,
                                     chain_offset=lc.CHAIN_OFFSET)
    for a in out:
        a.setflags(write=False)
    return out


def test_reference_accepts_and_rejects(oracle):
    """CPU: in every case of this file with L >= 1 the oracle alone accepts at
    least one proposal and rejects at least one (all accepted at L = 0)."""
    g = _products()
    for lay, dim in CASES:
        for dtype in lc.DTYPES:
            n = (N_COLLECT + N_DISCARD) * lc.N_CHAINS
            for L in LS:
                acc = int(_reference(g, oracle.lib, lay, dim, np.dtype(dtype).name, L)[2].sum())
                print(f"{lay} D={dim} {np.dtype(dtype).name} L={L}: {acc}/{n} accepted")
                if L == 0:
                    assert acc == n
                else:
                    assert 0 < acc < n, f"{lay} D={dim} {np.dtype(dtype).name} L={L}: {acc} of {n} accepted"
    for dtype in lc.DTYPES:
        acc = int(_reference(g, oracle.lib, (64, 1), 64, np.dtype(dtype).name, AUTO_L, AUTO_CHAINS)[2].sum())
        assert 0 < acc < (N_COLLECT + N_DISCARD) * AUTO_CHAINS
    total = sum(nc + nd for nc, nd in SEQUENCE)
    for lay, dim, dtype in sorted({(c[0], c[1], np.dtype(c[2]).name) for c in SEQ_CASES}):
        acc = int(_sequence_reference(g, oracle.lib, lay, dim, dtype)[2].sum())
        print(f"sequence {lay} D={dim} {dtype} L={SEQ_L}: {acc}/{total * lc.N_CHAINS} accepted")
        assert 0 < acc < total * lc.N_CHAINS


def _run(gm, lay, dim, dtype, L, form, chains=lc.N_CHAINS):
    s = gm.HMC(lc.target(gm, NAME, dim), lc.start(gm, dim, dtype, chains), _eps(dim, L), L, dtype=dtype,
               chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
    s.set_layout(*lay)
    s.set_unroll(form)
    out = s.run(N_COLLECT, N_DISCARD)
    res = (out, s.positions(), s.accept_counts(), s.logp(), s.last_unroll())
    s.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("lay,dim", CASES, ids=CASE_IDS)
def test_block_form_bitwise(gm, oracle, lay, dim, dtype, L):
    samples, q, acc = _reference(gm, oracle.lib, lay, dim, np.dtype(dtype).name, L)
    out1, q1, acc1, lp1, form1 = _run(gm, lay, dim, dtype, L, 1)
    out, qn, accn, lp, form = _run(gm, lay, dim, dtype, L, NEW)
    assert (form1, form) == (1, NEW)
    np.testing.assert_array_equal(out, samples)
    np.testing.assert_array_equal(qn, q)
    np.testing.assert_array_equal(accn, acc)
    assert np.isfinite(lp1).all()
    np.testing.assert_array_equal(lp, lp1, err_msg="logp against form 1")
    np.testing.assert_array_equal(out1, samples, err_msg="form 1")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
def test_automatic_choice_takes_the_block_form(gm, oracle, dtype):
    lay, dim = (64, 1), 64
    samples, q, acc = _reference(gm, oracle.lib, lay, dim, np.dtype(dtype).name, AUTO_L, AUTO_CHAINS)
    _, _, _, lp1, _ = _run(gm, lay, dim, dtype, AUTO_L, 1, AUTO_CHAINS)
    out, qn, accn, lp, form = _run(gm, lay, dim, dtype, AUTO_L, 0, AUTO_CHAINS)
    assert form == NEW, f"the automatic choice took form {form}"
    np.testing.assert_array_equal(out, samples)
    np.testing.assert_array_equal(qn, q)
    np.testing.assert_array_equal(accn, acc)
    np.testing.assert_array_equal(lp, lp1, err_msg="logp against form 1")
    # below the first L of the block form, and at two elements per lane, the choice is as before
    assert _run(gm, lay, dim, dtype, 2 * LONG, 0, AUTO_CHAINS)[4] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("lay,dim,dtype,form", SEQ_CASES, ids=SEQ_IDS)
def test_launch_sequence_against_one_oracle_run(gm, oracle, lay, dim, dtype, form):
    q, rows, acc = _sequence_reference(gm, oracle.lib, lay, dim, np.dtype(dtype).name)
    s = gm.HMC(lc.target(gm, NAME, dim), lc.start(gm, dim, dtype), _eps(dim, SEQ_L), SEQ_L, dtype=dtype,
               chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
    s.set_layout(*lay)
    s.set_unroll(form)
    step = 0
    for nc, nd in SEQUENCE:
        got = s.run_positions(nc, nd).to_host()  # [C, nc, D]
        np.testing.assert_array_equal(got, rows[step + nd:step + nd + nc].transpose(1, 0, 2),
                                      err_msg=f"run_positions({nc}, {nd})")
        step += nc + nd
    assert s.last_unroll() == form
    np.testing.assert_array_equal(s.positions(), q)
    np.testing.assert_array_equal(s.accept_counts(), acc)
    s.close()


@pytest.mark.gpu
def test_form_numbers(gm):
    s = gm.HMC(lc.target(gm, NAME, 64), lc.start(gm, 64, np.float32), 0.01, 3)
    for n in (0, 1, 2, 4, LONG, NEW):
        s.set_unroll(n)
    for n in (3, 5, 8, -1, 48, 50):
        with pytest.raises(gm.GMError):
            s.set_unroll(n)
    s.close()
