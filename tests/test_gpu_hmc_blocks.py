"""hmc_kernel's transition loop runs draw block by draw block with the S
positions of a block unrolled (S = 4 in f32, 2 in f64), a launch starting and
ending at any position; one chain per wave (64 lanes) keeps its sums in row 3
of the wave and takes the accept decision from one bit of a vector compare.
Every case follows one sampler through successive run() calls and compares
samples, positions() and accept_counts() bit for bit with the CPU oracle
continued from the same state, at the smallest shapes where that control flow
can go wrong: 5 chains are two workgroups at 64 lanes per chain (the second
with one live wave and three that leave after the barrier)."""
import numpy as np
import pytest

from tests._oracle import Target

pytestmark = pytest.mark.gpu

# (n_collect, n_discard): 1, 2, 3, 4, 5, 7, 9, 1 and 5 transitions, so the
# launches start at step0 % 4 = 0, 1, 3, 2, 2, 3, 2, 3, 0 and end at 1, 3, 2,
# 2, 3, 2, 3, 0, 1; the short ones end before the block a wave would prefetch,
# the long ones cross one or two block boundaries; (3, 2), (1, 6) and (5, 4)
# put collect_from inside a block
RESIDUE_RUNS = [(1, 0), (1, 1), (3, 0), (2, 2), (3, 2), (1, 6), (5, 4), (1, 0), (5, 0)]
SHORT_RUNS = [(2, 1), (3, 3)]  # starts at residues 0 and 3, ends at 3 and 1


def _start(gm, n, d, dtype, scale=0.5):
    return (gm.init_with_seed(n, d, 3, np.float64) * scale).astype(dtype)


def _follow(gm, oracle, t, x0, eps, L, seed, lay, runs, offset=0, unroll=None):
    """one sampler through `runs`, each run against the oracle continued from
    the oracle's own state; returns the final positions and accept counts"""
    dim = x0.shape[1]
    s = gm.HMC(t, x0, eps, L, dtype=x0.dtype, chain_offset=offset).set_seed(seed)
    s.set_layout(*lay)
    if unroll is not None:
        s.set_unroll(unroll)
    ot = Target.from_product(t, dim)
    q, step0 = x0, 0
    total = np.zeros(x0.shape[0], dtype=np.int64)
    for nc, nd in runs:
        out = s.run(nc, nd)  # [C, nc, D]
        q, samples, acc = oracle.hmc_run(ot, q, eps, L, seed, step0, nc + nd, nd, *lay, chain_offset=offset)
        total += acc
        msg = f"run({nc}, {nd}) from step {step0}"
        np.testing.assert_array_equal(out, samples.transpose(1, 0, 2), err_msg=msg)
        np.testing.assert_array_equal(s.positions(), q, err_msg=msg)
        np.testing.assert_array_equal(s.accept_counts(), total, err_msg=msg)
        step0 += nc + nd
    s.close()
    return q, total


@pytest.mark.parametrize("dim", [64, 33])
def test_every_head_and_tail_residue_f32(gm, oracle, dim):
    x0 = _start(gm, 5, dim, np.float32, 0.8)
    _, total = _follow(gm, oracle, gm.RosenbrockND(), x0, 0.02, 3, 21, (64, 1), RESIDUE_RUNS, offset=3)
    assert total.sum() > 0  # some proposals are accepted: both branches ran


def test_every_head_and_tail_residue_f64_two_per_block(gm, oracle):
    x0 = _start(gm, 5, 40, np.float64, 0.8)
    _, total = _follow(gm, oracle, gm.RosenbrockND(), x0, 0.02, 3, 21, (64, 1), RESIDUE_RUNS, offset=3)
    assert total.sum() > 0


@pytest.mark.parametrize("unroll", [1, 2, 4])
@pytest.mark.parametrize("L", [0, 1, 2, 7])
def test_loop_forms(gm, oracle, unroll, L):
    x0 = _start(gm, 5, 64, np.float32)
    _follow(gm, oracle, gm.RosenbrockND(), x0, 0.01, L, 5, (64, 1), [(3, 2)], unroll=unroll)


@pytest.mark.parametrize("dim,lay", [(100, (64, 2)), (64, (32, 2)), (64, (16, 4))])
def test_other_group_widths(gm, oracle, dim, lay):
    x0 = _start(gm, 5, dim, np.float32)
    _follow(gm, oracle, gm.RosenbrockND(), x0, 0.01, 3, 11, lay, SHORT_RUNS, offset=3)


@pytest.mark.parametrize("target", ["iso", "gauss"])
def test_other_targets_one_chain_per_wave(gm, oracle, target):
    dim = 64
    if target == "iso":
        t = gm.IsotropicGaussian(1.7)
    else:
        rng = np.random.default_rng(dim)
        a = rng.standard_normal((dim, dim))
        t = gm.DenseGaussian(rng.standard_normal(dim), a @ a.T / dim + np.eye(dim))
    x0 = _start(gm, 5, dim, np.float32)
    _follow(gm, oracle, t, x0, 0.05, 3, 11, (64, 1), SHORT_RUNS, offset=3)


def test_nan_log_alpha_rejects_in_its_own_chain_only(gm, oracle):
    """Chain 2 of six starts at 1e20 in one coordinate: its energies are not
    finite, log_alpha is NaN at every transition and every proposal is
    rejected (the compare is false for NaN), while the other five chains match
    the oracle as if it were not there."""
    x0 = _start(gm, 6, 64, np.float32, 0.8)
    x0[2, 17] = np.float32(1e20)
    q, total = _follow(gm, oracle, gm.RosenbrockND(), x0, 0.02, 3, 21, (64, 1), [(3, 2), (1, 6)])
    assert total[2] == 0
    np.testing.assert_array_equal(q[2], x0[2])
    ok = np.arange(6) != 2
    assert total[ok].sum() > 0
    # the five healthy chains alone, at their own global chain ids
    for lo, hi in ((0, 2), (3, 6)):
        ql, tl = _follow(gm, oracle, gm.RosenbrockND(), x0[lo:hi], 0.02, 3, 21, (64, 1), [(3, 2), (1, 6)], offset=lo)
        np.testing.assert_array_equal(ql, q[lo:hi])
        np.testing.assert_array_equal(tl, total[lo:hi])
