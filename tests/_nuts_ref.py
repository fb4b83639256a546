"""A float64 Python transcription of identity-metric NUTS that takes any
log-density: GenericNUTSChain::run / step / build_tree_with_mass /
stop_criterion / leapfrog_with_mass / find_reasonable_epsilon
(generic_nuts.rs:700-1418) under MassMatrix::identity, with the engine's
documented depth cap (the reference has none). Draws: the engine's RNG spec
through the oracle library's CPU restatement (momenta TAG_NUTS_MOM, the
transition's key block for Exp1 and the hashed uniforms).

tests/test_oracle_ref_forms.py ties it bit for bit to the oracle's form 1 on a
built-in target; tests/test_nuts_ref.py ties the oracle's form 0 (the kernels'
arithmetic) to it within rounding; the GPU tests of the GLM target
(tests/test_gpu_glm.py) drive it with tests/_glm_ref.py's log-density. It is
the NUTS counterpart of tests/_hmc_adapt_ref.py: `margin` is the smallest
distance of any of its decisions from the decision's threshold, so a run whose
margin is far above rounding has one decision sequence, which a correct
implementation in any summation order must reproduce.
"""
import ctypes
import math

import numpy as np

_libm = ctypes.CDLL("libm.so.6")
for _f in ("exp", "log"):
    getattr(_libm, _f).restype = ctypes.c_double
    getattr(_libm, _f).argtypes = [ctypes.c_double]
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]

TAG_NUTS_MOM, TAG_NUTS_INIT = 6, 11


def run(oracle, logp_grad, x0, eps0, n_collect, n_discard, seed, max_depth=10, target_accept=0.8):
    """logp_grad: [1, D] float64 -> (lp [1], g [1, D]). Returns per chain a dict:
    samples, q (final position), eps, eps_bar, h_bar, mu, acc and nlf (accept and
    leapfrog totals of the transitions), depth, n_leapfrog and fwd (per transition:
    doublings, leapfrogs, and how many of the doublings went forward in time),
    margin: the smallest distance of a decision from its threshold over
      the slice test logu < joint and the divergence test logu - 1000 < joint
        (|difference| of the two sides; a non-finite joint has none),
      both U-turn dot products, |dot| / (|diff| |p|),
      the subtree draw u < n' / (n + n') and the transition accept
        u < min(1, n' / n) (|u - threshold|),
      the comparisons of find_reasonable_epsilon (|difference| of the two sides)."""
    lib = oracle.lib
    C_, D = x0.shape
    mg = [math.inf]

    def near(d):
        if d == d and d < mg[0]:
            mg[0] = d

    def logp_and_grad(q):
        lp, g = logp_grad(np.asarray(q, dtype=np.float64)[None, :])
        return float(lp[0]), [float(v) for v in g[0]]

    def kinetic(p):                          # :230-235
        q = 0.0
        for v in p:
            q = q + v * v
        return 0.5 * q

    def dot(a, b):
        s = 0.0
        for x, y in zip(a, b):
            s = s + x * y
        return s

    def stop_criterion(qm, qp, pm, pp):      # :1357-1378, identity
        diff = [b - a for a, b in zip(qm, qp)]
        nd = math.sqrt(dot(diff, diff))
        d1 = dot(diff, pm)
        near(abs(d1) / (nd * math.sqrt(dot(pm, pm)) or math.inf))
        if not d1 >= 0.0:
            return False
        d2 = dot(diff, pp)
        near(abs(d2) / (nd * math.sqrt(dot(pp, pp)) or math.inf))
        return d2 >= 0.0

    counts = {"nlf": 0}

    def leapfrog(q, p, g, eps):              # :1396-1418
        half = 0.5
        p = [pi + gi * (eps * half) for pi, gi in zip(p, g)]
        q = [qi + vi * eps for qi, vi in zip(q, p)]
        lp, g = logp_and_grad(q)
        p = [pi + gi * (eps * half) for pi, gi in zip(p, g)]
        counts["nlf"] += 1
        return q, p, g, lp

    def find_reasonable_epsilon(q0, p0):     # :1025-1102
        eps, half = 1.0, 0.5
        ulogp, g0 = logp_and_grad(q0)
        q, p, g, ulogp1 = leapfrog(q0, p0, g0, eps)
        k = 1.0
        while not (math.isfinite(ulogp1) and all(math.isfinite(v) for v in g)):
            k = k * half
            q, p, g, ulogp1 = leapfrog(q0, p0, g0, eps * k)
        eps = half * k * eps
        la = ulogp1 - ulogp - (kinetic(p) - kinetic(p0))
        near(abs(la - _libm.log(half)))
        a = 1.0 if la > _libm.log(half) else -1.0
        near(abs(a * la + a * _libm.log(2.0)))
        while a * la > -a * _libm.log(2.0):
            eps = eps * _libm.pow(2.0, a)
            q, p, g, ulogp1 = leapfrog(q0, p0, g0, eps)
            la = ulogp1 - ulogp - (kinetic(p) - kinetic(p0))
            near(abs(a * la + a * _libm.log(2.0)))
        return eps

    def build_tree(q, p, g, logu, v, j, eps, joint0, key, ctr):   # :1153-1341
        if j == 0:
            q1, p1, g1, lp1 = leapfrog(q, p, g, float(v) * eps)
            joint = lp1 - kinetic(p1)
            if math.isfinite(joint):
                near(abs(joint - logu))
                near(abs(joint - (logu - 1000.0)))
            return dict(qm=q1, pm=p1, gm=g1, qp=q1, pp=p1, gp=g1, qprime=q1, gprime=g1, logp_prime=lp1,
                        n=int(logu < joint), s=(logu - 1000.0) < joint,
                        alpha=min(1.0, _libm.exp(joint - joint0)) if joint - joint0 == joint - joint0 else 1.0,
                        n_alpha=1)
        tr = build_tree(q, p, g, logu, v, j - 1, eps, joint0, key, ctr)
        if tr["s"]:
            if v == -1:
                t2 = build_tree(tr["qm"], tr["pm"], tr["gm"], logu, v, j - 1, eps, joint0, key, ctr)
                tr["qm"], tr["pm"], tr["gm"] = t2["qm"], t2["pm"], t2["gm"]
            else:
                t2 = build_tree(tr["qp"], tr["pp"], tr["gp"], logu, v, j - 1, eps, joint0, key, ctr)
                tr["qp"], tr["pp"], tr["gp"] = t2["qp"], t2["pp"], t2["gp"]
            u = lib.or_nuts_u_d(key, 64 + ctr[0])
            ctr[0] += 1
            near(abs(u - t2["n"] / max(tr["n"] + t2["n"], 1)))
            if u < t2["n"] / max(tr["n"] + t2["n"], 1):
                tr["qprime"], tr["gprime"], tr["logp_prime"] = t2["qprime"], t2["gprime"], t2["logp_prime"]
            tr["n"] += t2["n"]
            tr["s"] = tr["s"] and t2["s"] and stop_criterion(tr["qm"], tr["qp"], tr["pm"], tr["pp"])
            tr["alpha"] = tr["alpha"] + t2["alpha"]
            tr["n_alpha"] += t2["n_alpha"]
        return tr

    gamma, kappa, t0, delta = 0.05, 0.75, 10, target_accept
    total = n_discard + n_collect - 1
    out = []
    for c in range(C_):
        mg[0] = math.inf
        q = [float(v) for v in x0[c]]
        eps, eps_bar, h_bar = float(eps0), 1.0, 0.0
        # init_chain_state (:731-753)
        p_init = [lib.or_normal_d(seed, c, 0, TAG_NUTS_INIT, i) for i in range(D)]
        if abs(eps + 1.0) <= 2.220446049250313e-16:
            eps = find_reasonable_epsilon(q, p_init)
        mu = _libm.log(10.0 * eps)
        counts["nlf"] = 0  # the leapfrog count is the transitions' (the step-size search's are not counted)
        samples = [list(q)] if n_discard == 0 else []
        acc = 0
        depths, nlfs, fwds = [], [], []
        for s in range(total):
            m = s + 1
            nlf0 = counts["nlf"]
            key, w = oracle.nuts_key(seed, c, s)
            p0 = [lib.or_normal_d(seed, c, s, TAG_NUTS_MOM, i) for i in range(D)]
            logp, g0 = logp_and_grad(q)
            joint = logp - kinetic(p0)
            k = ((w[2] >> 5) << 26) | (w[3] >> 6)
            exp1 = -lib.or_log_d((k + 1) * 1.1102230246251565e-16)
            logu = joint - exp1
            qm, qp, pm, pp, gm, gp = q, q, p0, p0, g0, g0
            j, n, go, alpha, n_alpha = 0, 1, True, 0.0, 0
            ctr = [0]
            fwd = 0
            while go and j < max_depth:
                v = 1 if lib.or_nuts_u_d(key, 2 * j) < 0.5 else -1
                fwd += v == 1
                if v == -1:
                    tr = build_tree(qm, pm, gm, logu, v, j, eps, joint, key, ctr)
                    qm, pm, gm = tr["qm"], tr["pm"], tr["gm"]
                else:
                    tr = build_tree(qp, pp, gp, logu, v, j, eps, joint, key, ctr)
                    qp, pp, gp = tr["qp"], tr["pp"], tr["gp"]
                alpha, n_alpha = tr["alpha"], tr["n_alpha"]
                tmp = min(1.0, tr["n"] / n)
                if tr["s"]:
                    near(abs(lib.or_nuts_u_d(key, 2 * j + 1) - tmp))
                if tr["s"] and lib.or_nuts_u_d(key, 2 * j + 1) < tmp:
                    q = tr["qprime"]
                    acc += 1
                n += tr["n"]
                go = tr["s"] and stop_criterion(qm, qp, pm, pp)
                j += 1
            depths.append(j)
            fwds.append(fwd)
            nlfs.append(counts["nlf"] - nlf0)
            eta = 1.0 / (m + t0)
            h_bar = (1.0 - eta) * h_bar + eta * (delta - alpha / n_alpha)
            if m <= n_discard:
                eps = _libm.exp(mu - math.sqrt(m) / gamma * h_bar)
                eta = _libm.pow(float(m), -kappa)
                eps_bar = _libm.exp((1.0 - eta) * _libm.log(eps_bar) + eta * _libm.log(eps))
            else:
                eps = eps_bar
            if 0 <= (s + 1) - n_discard < n_collect:
                samples.append(list(q))
        out.append(dict(samples=np.array(samples), q=np.array(q), eps=eps, eps_bar=eps_bar, h_bar=h_bar, mu=mu,
                        acc=acc, nlf=counts["nlf"], depth=np.array(depths, dtype=np.int64),
                        n_leapfrog=np.array(nlfs, dtype=np.int64), fwd=np.array(fwds, dtype=np.int64),
                        margin=mg[0]))
    return out


def deviation(a, b):
    """The largest difference of two results of the same run: samples and final
    positions absolute (the callers' posteriors have sds of order 0.1 .. 1),
    eps and eps_bar relative. a, b: dicts of arrays with a leading chain axis
    (stack())."""
    return max(float(np.max(np.abs(a["samples"] - b["samples"]))), float(np.max(np.abs(a["q"] - b["q"]))),
               float(np.max(np.abs(a["eps"] - b["eps"]) / np.abs(b["eps"]))),
               float(np.max(np.abs(a["eps_bar"] - b["eps_bar"]) / np.abs(b["eps_bar"]))))


def stack(chains):
    """run()'s list of per-chain dicts as one dict of arrays with a leading chain axis."""
    keys = ("samples", "q", "eps", "eps_bar", "acc", "nlf", "depth", "n_leapfrog", "fwd", "margin")
    return {k: np.array([c[k] for c in chains]) for k in keys}


def same_decisions(a, b):
    """Two stacked results whose every transition built the same tree and moved alike."""
    return (np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["n_leapfrog"], b["n_leapfrog"])
            and np.array_equal(a["acc"], b["acc"]))
