"""One chain per wave, hmc_kernel keeps the accept log-uniforms of 64
consecutive transitions (a window, transitions 64 w .. 64 w + 63) in the 64
lanes of one register: one pass per window, computed by the first fill of a
launch or by the prefetch of the window's first draw block, and transition st
reads lane st % 64. Every case follows one sampler through consecutive
run_positions calls whose start steps mod 64 are 0, 2, 1, 1, 15, 16, 17 and
63 and whose lengths put zero, one and two window boundaries inside a launch,
and compares the concatenated samples, the final positions and the accept
counts bit for bit with ONE oracle run of the total. 5 chains are two
workgroups (the second with one live wave), so waves of prefetch phase 0..3
all run, and the launch that starts at residue 63 hands the next window over
both ways (prefetched by the phase-3 wave, filled directly by the others).

eps = 0.038 was chosen on the CPU with the oracle alone: over the 385
transitions its accept fraction is 0.76 (f32, D = 64), 0.72 (f32, D = 100)
and 0.77 (f64, D = 64), every chain between 0.70 and 0.79, so accepted and
rejected proposals both occur in every window; each case asserts that on the
oracle's counts.

The layouts with more than two elements per lane (the kernel's LF = 0 form)
run the same calls at a padded dim each. At eps = 0.038 the oracle's accept
fraction is 0.58 (f32, D = 253, 64 x 4; chains 0.51-0.61) and 0.43 (f32,
D = 509, 64 x 8; chains 0.27-0.48). At f64, D = 1021, 64 x 16 it is 0.23,
inside the band, but one chain accepts 1 of its 385 proposals (0.003), so its
windows would hold no accepted proposal; that case runs at eps = 0.03: 0.56,
every chain between 0.53 and 0.58 (oracle scan: 0.034 gives 0.35 with the
same chain stuck, 0.028 gives 0.62, 0.024 gives 0.75)."""
import numpy as np
import pytest

from tests._oracle import Target

# (n_collect, n_discard) per call; start step, start % 64, length, window
# boundaries strictly inside the launch:
#     0   0  130  2   (64, 128)
#   130   2   63  1   (192)
#   193   1   64  1   (256)
#   257   1   14  0
#   271  15    1  0
#   272  16   65  1   (320)
#   337  17   46  0
#   383  63    2  1   (384, after the launch's first transition)
RUNS = [(100, 30), (63, 0), (64, 0), (14, 0), (1, 0), (60, 5), (46, 0), (2, 0)]
TOTAL = sum(nc + nd for nc, nd in RUNS)
EPS, L, SEED, OFFSET = 0.038, 2, 21, 3


def test_runs_cover_the_residues_and_lengths():
    starts = np.cumsum([0] + [nc + nd for nc, nd in RUNS])[:-1]
    assert {0, 1, 15, 16, 63} <= {int(s) % 64 for s in starts}
    assert {1, 63, 64, 65, 130} <= {nc + nd for nc, nd in RUNS}
    inside = {int((s + n - 1) // 64 - s // 64) for s, n in zip(starts, (nc + nd for nc, nd in RUNS))}
    assert {0, 1, 2} <= inside


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim,lay,eps", [(np.float32, 64, (64, 1), EPS), (np.float32, 100, (64, 2), EPS),
                                               (np.float64, 64, (64, 1), EPS), (np.float32, 253, (64, 4), EPS),
                                               (np.float32, 509, (64, 8), EPS), (np.float64, 1021, (64, 16), 0.03)],
                         ids=["f32-64x1", "f32-64x2-padded", "f64-64x1", "f32-64x4-padded", "f32-64x8-padded",
                              "f64-64x16-padded"])
def test_consecutive_launches_equal_one_oracle_run(gm, oracle, dtype, dim, lay, eps):
    t = gm.RosenbrockND()
    x0 = (gm.init_with_seed(5, dim, 3, np.float64) * 0.5).astype(dtype)
    q, ref, acc = oracle.hmc_run(Target.from_product(t, dim), x0, eps, L, SEED, 0, TOTAL, 0, *lay,
                                 chain_offset=OFFSET)  # ref: [TOTAL, C, D]
    frac = acc.sum() / (x0.shape[0] * TOTAL)
    print(f"oracle accept fraction {frac:.4f}, per chain {acc / TOTAL}")
    assert 0.2 <= frac <= 0.8

    s = gm.HMC(t, x0, eps, L, dtype=dtype, chain_offset=OFFSET).set_seed(SEED)
    s.set_layout(*lay)
    assert s.layout() == lay
    step0 = 0
    for nc, nd in RUNS:
        got = s.run_positions(nc, nd).to_host()  # [C, nc, D]
        lo = step0 + nd
        np.testing.assert_array_equal(got, ref[lo:lo + nc].transpose(1, 0, 2),
                                      err_msg=f"run_positions({nc}, {nd}) from step {step0}")
        step0 += nc + nd
    np.testing.assert_array_equal(s.positions(), q)
    np.testing.assert_array_equal(s.accept_counts(), acc)
    s.close()
