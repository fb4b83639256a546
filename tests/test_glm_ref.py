"""The GLM target without a GPU: the numpy reference (tests/_glm_ref.py) against
finite differences and its asymptotes, the facade's validation, and the C
header's new struct against its ctypes mirror."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _glm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("offset", [False, True])
def test_gradient_is_the_finite_difference_of_logp(family, offset):
    N, D = 23, 4
    X, y, off = R.synth(N, D, family, 3, offset=offset)
    ref = R.GlmRef(X, y, family, prior_sd=np.array([0.5, 1.0, 2.0, 4.0]), offset=off)
    rng = np.random.default_rng(4)
    theta = rng.standard_normal((5, D))
    lp, g = ref.logp_grad(theta)
    h = 1e-5
    for j in range(D):
        e = np.zeros(D)
        e[j] = h
        fd = (ref.logp_grad(theta + e)[0] - ref.logp_grad(theta - e)[0]) / (2 * h)
        # central differences: h^2 f'''/6 + rounding u |logp| / h
        np.testing.assert_allclose(fd, g[:, j], rtol=0, atol=1e-7 * (1 + np.abs(lp).max()))


def test_bernoulli_is_finite_at_eta_800():
    X = np.array([[800.0], [-800.0], [800.0], [-800.0]])
    y = np.array([1.0, 1.0, 0.0, 0.0])
    ref = R.GlmRef(X, y, "bernoulli_logit", prior_sd=1e6)
    lp, g = ref.logp_grad(np.array([[1.0]]))
    eta = X[:, 0]
    asym = np.sum(-np.maximum(eta, 0) + y * eta) - 0.5 * 1.0 / 1e12
    assert np.isfinite(lp[0]) and np.all(np.isfinite(g))
    assert abs(lp[0] - asym) <= 4 * np.finfo(np.float64).eps * 1600
    # gradient: rows 1 (y=1, eta=-800) and 2 (y=0, eta=800) pull with |x| each
    np.testing.assert_allclose(g[0, 0], (1 - 0) * -800.0 + (0 - 1) * 800.0 - 1e-12, rtol=1e-15)


def test_poisson_overflow_is_not_a_finite_value():
    ref = R.GlmRef(np.array([[1.0], [1.0]]), np.array([3.0, 0.0]), "poisson_log")
    lp, g = ref.logp_grad(np.array([[800.0]]))
    assert not np.isfinite(lp[0])
    assert lp[0] == -np.inf or np.isnan(lp[0])


def test_facade_validation_without_a_device():
    import general_mcmc_amd as gm
    X = np.ones((4, 2))
    y = np.array([0.0, 1.0, 1.0, 0.0])
    gm.GLM(X, y)  # valid
    gm.GLM(X, y * 3, family="poisson_log", prior_sd=[1.0, 2.0], offset=np.zeros(4))

    def bad(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            gm.GLM(*a, **k)

    bad("family", X, y, family="probit")
    bad(r"X must be \[n_rows, dim\]", np.ones(4), y)
    bad("n_rows must be >= 1", np.ones((0, 2)), np.ones(0))
    bad(r"dim must be in \[1, 128\]", np.ones((4, 129)), y)
    bad(r"y must be \[n_rows\]", X, np.ones(3))
    bad("prior_sd must be a scalar or", X, y, prior_sd=[1.0, 2.0, 3.0])
    bad(r"offset must be \[n_rows\]", X, y, offset=np.zeros(5))
    bad("prior_sd must be > 0 at column 1", X, y, prior_sd=[1.0, 0.0])
    bad("prior_sd is not finite at column 0", X, y, prior_sd=[np.inf, 1.0])
    Xb = X.copy()
    Xb[2, 1] = np.nan
    bad("x is not finite at row 2, column 1", Xb, y)
    bad("bernoulli_logit needs 0 <= y <= 1 at row 3", X, np.array([0.0, 1.0, 0.5, 1.5]))
    bad("poisson_log needs y >= 0 at row 1", X, np.array([0.0, -1.0, 2.0, -3.0]), family="poisson_log")
    bad("y is not finite at row 0", X, np.array([np.nan, 1.0, 1.0, 7.0]))
    bad("offset is not finite at row 2", X, y, offset=np.array([0.0, 0.0, np.inf, 0.0]))
    # the first offending row wins, whatever its kind
    bad("y is not finite at row 1", Xb, np.array([0.0, np.inf, 1.0, 0.0]))


def _cc():
    for c in (os.environ.get("CC"), "cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_header_struct_is_the_ctypes_struct(tmp_path):
    from general_mcmc_amd import _lib
    cc = _cc()
    assert cc is not None, "no C compiler found"
    structs = {"gm_glm_desc": _lib.gm_glm_desc, "gm_target": _lib.gm_target}
    prints = "".join(
        f'printf("{s} %zu\\n", sizeof({s}));' + "".join(
            f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _ in t._fields_) for s, t in structs.items())
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gmcmc.h"\n'
                   f"int main(void) {{ {prints} return 0; }}\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    want = {}
    for s, t in structs.items():
        want[s] = str(C.sizeof(t))
        for f, _ in t._fields_:
            want[f"{s}.{f}"] = str(getattr(t, f).offset)
    assert got == want
    # the appended field is the struct's last, and the kind's value is the header's
    assert _lib.gm_target._fields_[-1][0] == "glm"
    hdr = open(os.path.join(ROOT, "include", "gmcmc.h")).read()
    assert "GM_TARGET_GLM = 5" in hdr and _lib.GM_TARGET_GLM == 5
    assert "#define GM_GLM_BERNOULLI_LOGIT 1" in hdr and "#define GM_GLM_POISSON_LOG 2" in hdr
