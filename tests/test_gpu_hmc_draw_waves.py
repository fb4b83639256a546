"""The draw-wave form of the block-form HMC kernel (hmc_dw_kernel,
csrc/hmc_dw_device.h): a workgroup of 4 chain waves and NDW = 1 draw wave,
the momenta, kinetic energies and accept windows of a draw block made by the
draw wave and handed over through double-buffered LDS, one barrier per draw
block. Forced with gm_sampler_set_draw_waves(1) and chosen automatically in
f32 where it measured faster: above two and a half and up to four chain waves
per SIMD (2561 to 4096 chains on the MI355X's 256 CUs) at L <= 50, where the
block form runs. At 1029 chains, the count the form was first planned for, it
measured 2.4 % slower than the block form alone (1.724 against 1.685 us per
transition) and the automatic choice leaves it off; the automatic case runs
3001 chains. The draws are the
same numbers made by other waves, so every case gives the CPU oracle's bits
and the bits of the same sampler with the form off.

Shapes (tests/_layout_cases.py): layout 64 x 1 at its full and padded dim,
both dtypes, chain offset 3, and 1, 4 and 5 chains: a workgroup with one live
chain wave, a full one, and a second workgroup with three empty chain waves.
L: 0 and 1 run no loop step, 2 one leapfrog from the block form's ladder, 50
(the bench's L) one pass and no ladder, 51 a piece and a pass. Every run is 10
transitions with the first 3 discarded: three draw blocks in f32 (the last one
cut short, collecting begins inside the first) and five in f64.

Each case takes a scale of the matrix's step size (EPS_SCALE) at which the
oracle alone, on the CPU, both accepts and rejects:
test_reference_accepts_and_rejects asserts that for every case of this file.

The launch sequence is that of test_gpu_hmc_entered_form.py: launches that
start and end inside a draw block, collecting that begins inside a block,
whole blocks discarded, and the accept windows crossed at steps 64 and 128;
one oracle run over all 180 transitions is the reference."""
import functools

import numpy as np
import pytest

from tests import _layout_cases as lc
from tests._oracle import Target

NDW = 1        # the compiled draw waves per workgroup (GM_DW_WAVES)
BLOCK = 49     # the block leapfrog form's set_unroll number
LS = [0, 1, 2, 50, 51]
CHAINS = [1, 4, 5]
CASES = [((64, 1), 64), ((64, 1), 61)]
CASE_IDS = [f"{lay[0]}x{lay[1]}-D{d}" for lay, d in CASES]
NAME = "rosenbrock"
SEED, N_COLLECT, N_DISCARD = 11, 7, 3
# the step size as a multiple of the matrix's (chosen at L = 3 for 5 chains), per L;
# the single chain's 10 proposals at long L both accept and reject in every
# dim and dtype only at 0.79 of a grid of 0.01 from 0.70 to 0.85 (accepted
# 9, 4, 6, 1 and 9, 4, 9, 1 of 10), hence its own scale there
EPS_SCALE = {1: 1.1, 50: 0.8, 51: 0.8, (1, 50): 0.79, (1, 51): 0.79}
AUTO_CHAINS, AUTO_L = 3001, 50

SEQUENCE = [(1, 0), (3, 2), (5, 6), (9, 0), (130, 1), (0, 9), (8, 0), (6, 0)]
SEQ_L = 51
SEQ_CASES = [(64, np.float32), (61, np.float32), (64, np.float64), (61, np.float64)]
SEQ_IDS = [f"D{d}-{np.dtype(dt).name}" for d, dt in SEQ_CASES]


def _eps(dim, L, chains=lc.N_CHAINS):
    return lc.HMC_EPS[NAME, dim] * EPS_SCALE.get((chains, L), EPS_SCALE.get(L, 1.0))


def _products():
    import general_mcmc_amd as g
    return g


@functools.lru_cache(maxsize=None)
def _reference(g, oracle_lib, lay, dim, dtype, L, chains):
    """(samples [C, N_COLLECT, D], positions, accept counts) of the 10 transitions."""
    from tests._oracle import Oracle
    ot = Target.from_product(lc.target(g, NAME, dim), dim)
    q, samples, acc = Oracle(oracle_lib).hmc_run(ot, lc.start(g, dim, dtype, chains), _eps(dim, L, chains), L, SEED, 0,
                                                 N_COLLECT + N_DISCARD, N_DISCARD, *lay,
                                                 chain_offset=lc.CHAIN_OFFSET)
    out = (np.ascontiguousarray(samples.transpose(1, 0, 2)), q, acc)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sequence_reference(g, oracle_lib, dim, dtype):
    """(positions, every transition's state [180, C, D], accept counts) of one run."""
    from tests._oracle import Oracle
    total = sum(nc + nd for nc, nd in SEQUENCE)
    ot = Target.from_product(lc.target(g, NAME, dim), dim)
    out = Oracle(oracle_lib).hmc_run(ot, lc.start(g, dim, dtype), _eps(dim, SEQ_L), SEQ_L, SEED, 0, total, 0, 64, 1,
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
            for chains in CHAINS:
                n = (N_COLLECT + N_DISCARD) * chains
                for L in LS:
                    acc = int(_reference(g, oracle.lib, lay, dim, np.dtype(dtype).name, L, chains)[2].sum())
                    print(f"{lay} D={dim} {np.dtype(dtype).name} C={chains} L={L}: {acc}/{n} accepted")
                    if L == 0:
                        assert acc == n
                    else:
                        assert 0 < acc < n, f"{lay} D={dim} {np.dtype(dtype).name} C={chains} L={L}: {acc} of {n}"
    acc = int(_reference(g, oracle.lib, (64, 1), 64, "float32", AUTO_L, AUTO_CHAINS)[2].sum())
    assert 0 < acc < (N_COLLECT + N_DISCARD) * AUTO_CHAINS
    total = sum(nc + nd for nc, nd in SEQUENCE)
    for dim, dtype in SEQ_CASES:
        acc = int(_sequence_reference(g, oracle.lib, dim, np.dtype(dtype).name)[2].sum())
        assert 0 < acc < total * lc.N_CHAINS


def test_prototypes_exist():
    """CPU: the ctypes prototypes of the two entry points."""
    g = _products()
    for name in ("gm_sampler_set_draw_waves", "gm_sampler_last_draw_waves"):
        assert name in g._lib.SIGNATURES
    assert callable(g.HMC.set_draw_waves) and callable(g.HMC.last_draw_waves)


def _run(gm, lay, dim, dtype, L, chains, draw_waves, unroll=BLOCK):
    s = gm.HMC(lc.target(gm, NAME, dim), lc.start(gm, dim, dtype, chains), _eps(dim, L, chains), L, dtype=dtype,
               chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
    s.set_layout(*lay)
    s.set_unroll(unroll)
    s.set_draw_waves(draw_waves)
    out = s.run(N_COLLECT, N_DISCARD)
    res = (out, s.positions(), s.accept_counts(), s.logp(), s.last_draw_waves())
    s.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("chains", CHAINS)
@pytest.mark.parametrize("dtype", lc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("lay,dim", CASES, ids=CASE_IDS)
def test_draw_wave_form_bitwise(gm, oracle, lay, dim, dtype, chains, L):
    samples, q, acc = _reference(gm, oracle.lib, lay, dim, np.dtype(dtype).name, L, chains)
    out0, q0, acc0, lp0, n0 = _run(gm, lay, dim, dtype, L, chains, 0)
    out, qn, accn, lp, n = _run(gm, lay, dim, dtype, L, chains, NDW)
    assert (n0, n) == (0, NDW)
    np.testing.assert_array_equal(out, samples)
    np.testing.assert_array_equal(qn, q)
    np.testing.assert_array_equal(accn, acc)
    assert np.isfinite(lp0).all()
    np.testing.assert_array_equal(lp, lp0, err_msg="logp against the form off")
    np.testing.assert_array_equal(out0, samples, err_msg="the form off")
    np.testing.assert_array_equal(q0, q, err_msg="the form off")
    np.testing.assert_array_equal(acc0, acc, err_msg="the form off")


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype", SEQ_CASES, ids=SEQ_IDS)
def test_launch_sequence_against_one_oracle_run(gm, oracle, dim, dtype):
    q, rows, acc = _sequence_reference(gm, oracle.lib, dim, np.dtype(dtype).name)
    s = gm.HMC(lc.target(gm, NAME, dim), lc.start(gm, dim, dtype), _eps(dim, SEQ_L), SEQ_L, dtype=dtype,
               chain_offset=lc.CHAIN_OFFSET).set_seed(SEED)
    s.set_layout(64, 1)
    s.set_draw_waves(NDW)
    step = 0
    for nc, nd in SEQUENCE:
        got = s.run_positions(nc, nd).to_host()  # [C, nc, D]
        assert s.last_draw_waves() == NDW and s.last_unroll() == BLOCK
        np.testing.assert_array_equal(got, rows[step + nd:step + nd + nc].transpose(1, 0, 2),
                                      err_msg=f"run_positions({nc}, {nd})")
        step += nc + nd
    np.testing.assert_array_equal(s.positions(), q)
    np.testing.assert_array_equal(s.accept_counts(), acc)
    s.close()


@pytest.mark.gpu
def test_automatic_choice(gm, oracle):
    """3001 chains (more than two and a half waves per SIMD of the MI355X's 256
    CUs) at L = 50 take the form in f32; 1029 chains, 5 chains, L = 99, f64
    and layout 64 x 2 do not."""
    lay, dim = (64, 1), 64
    samples, q, acc = _reference(gm, oracle.lib, lay, dim, "float32", AUTO_L, AUTO_CHAINS)
    out, qn, accn, _, n = _run(gm, lay, dim, np.float32, AUTO_L, AUTO_CHAINS, -1, unroll=0)
    assert n == NDW, f"the automatic choice took {n} draw waves"
    np.testing.assert_array_equal(out, samples)
    np.testing.assert_array_equal(qn, q)
    np.testing.assert_array_equal(accn, acc)
    assert _run(gm, lay, dim, np.float32, AUTO_L, 1029, -1, unroll=0)[4] == 0
    assert _run(gm, lay, dim, np.float32, AUTO_L, 5, -1, unroll=0)[4] == 0
    assert _run(gm, lay, dim, np.float32, 99, AUTO_CHAINS, -1, unroll=0)[4] == 0
    assert _run(gm, lay, dim, np.float64, AUTO_L, AUTO_CHAINS, -1, unroll=0)[4] == 0
    assert _run(gm, (64, 2), 128, np.float32, AUTO_L, AUTO_CHAINS, -1, unroll=0)[4] == 0


@pytest.mark.gpu
def test_error_paths(gm, oracle):
    lay, dim, dtype, L, chains = (64, 1), 64, np.float32, 2, 5
    s = gm.HMC(lc.target(gm, NAME, dim), lc.start(gm, dim, dtype), 0.01, 3)
    for n in (-1, 0, 1, 2, 4):
        s.set_draw_waves(n)
    for n in (-2, 3, 5, 8, 64):
        with pytest.raises(gm.GMError):
            s.set_draw_waves(n)
    s.set_draw_waves(-1)
    s.collect_stats(True)
    with pytest.raises(gm.GMError):
        s.set_draw_waves(NDW)
    s.close()
    # a count that is not compiled, and the compiled count at a layout without
    # the form, run as off and report 0
    samples, q, acc = _reference(gm, oracle.lib, lay, dim, np.dtype(dtype).name, L, chains)
    for n in (2, 4):
        out, qn, accn, _, got = _run(gm, lay, dim, dtype, L, chains, n)
        assert got == 0
        np.testing.assert_array_equal(out, samples)
        np.testing.assert_array_equal(accn, acc)
    assert _run(gm, (64, 2), 128, dtype, L, chains, NDW, unroll=0)[4] == 0
