/* gm_oracle_t.inc — CPU ORACLE, instantiated for T = double and T = float
 * from gm_oracle.c (test infrastructure only). */

#define F(name) CAT(name, SFX)
/* the elementary functions of a form: 0 the engine's (msun restatements,
 * the kernels' bits), 1 the C library's (the reference's f64::exp / ln) */
#define MEXP(form, x) ((form) == 1 ? REXP(x) : EXP(x))
#define MLOG(form, x) ((form) == 1 ? RLOG(x) : LOG(x))

/* the engine's declared summation order: per lane left-to-right over elems,
 * then pairwise stages combining lane l with partner l^1, l^2, l^7, l^15,
 * l^16, l^32 (as many as log2(lanes)) */
static T F(red)(const T* v, int lanes, int elems) {
  static const int partner_xor[6] = {1, 2, 7, 15, 16, 32};
  T part[64], tmp[64];
  if (lanes > 64) {
    /* a chain spread over lanes/64 waves (one workgroup, hmc_wide_kernel):
     * each wave's 64-lane total, then the wave totals left to right */
    T s = F(red)(v, 64, elems);
    for (int w = 1; w < lanes / 64; ++w) s = s + F(red)(v + (int64_t)w * 64 * elems, 64, elems);
    return s;
  }
  for (int l = 0; l < lanes; ++l) {
    T a = v[l * elems];
    for (int e = 1; e < elems; ++e) a = a + v[l * elems + e];
    part[l] = a;
  }
  for (int k = 0; (1 << (k + 1)) <= lanes; ++k) {
    const int m = partner_xor[k];
    for (int l = 0; l < lanes; ++l) tmp[l] = part[l] + part[l ^ m];
    for (int l = 0; l < lanes; ++l) part[l] = tmp[l];
  }
  return part[0];
}

/* dot product of two D-vectors in the declared order (padding = 0) */
static T F(dot)(const T* a, const T* b, int D, int lanes, int elems) {
  const int W = lanes * elems;
  if (W < 1) return (T)0;
  T buf[W];
  for (int i = 0; i < W; ++i) buf[i] = (i < D) ? a[i] * b[i] : (T)0;
  return F(red)(buf, lanes, elems);
}

/* log-density and gradient of the built-in targets
 *  Rosenbrock  distributions.rs:535-555 / 495-530 (analytic autodiff result)
 *  IsoGauss    distributions.rs:398-406
 *  Gauss       distributions.rs:257-320 (DiffableGaussian2D, generalised)  */
static T F(logp_grad_impl)(const or_target* t, int lanes, int elems, const T* x, T* g) {
  const int D = t->dim, W = lanes * elems;
  T buf[W];
  if (t->kind == 1 && lanes >= 64) {
    /* 64-lane (and wider) groups: g = x (4b t_i - 2) + (2a - 2b t_{i-1}) as
     * three fused multiply-adds whose [.] factors are per-lane constants that
     * are 0 where the term is absent (gm_device.h RosenbrockLane); the
     * neighbour values beyond the chain are 0. The same gradient as the
     * select form below up to rounding (fewer roundings here). */
    const T a = (T)t->a, b = (T)t->b, b2 = (T)2 * (T)t->b, b4 = (T)4 * (T)t->b;
    for (int i = 0; i < W; ++i) {
      if (i >= D) { buf[i] = (T)0; continue; }
      const T am = a - x[i];
      const int hs = i <= D - 2, hp = (i >= 1) && (i <= D - 1);
      const T xn = (i + 1 < D) ? x[i + 1] : (T)0;
      const T xp = (i >= 1) ? x[i - 1] : (T)0;
      const T ti = xn - x[i] * x[i];
      const T tp = x[i] - xp * xp;
      /* g = x (4b t - 2) + (2a - 2b t_prev) as three fused multiply-adds
       * (round 4: the t_prev term is an fma of its own, so the kernels' t
       * chain is two fmas deep) */
      g[i] = FMA(x[i], FMA(hs ? b4 : (T)0, ti, hs ? (T)-2 : (T)0), FMA(hp ? -b2 : (T)0, tp, hs ? (T)2 * a : (T)0));
      buf[i] = hs ? b * (ti * ti) + am * am : (T)0;
    }
    return -F(red)(buf, lanes, elems);
  }
  if (t->kind == 1) {
    const T a = (T)t->a, b = (T)t->b, b2 = (T)2 * (T)t->b, b4 = (T)4 * (T)t->b;
    for (int i = 0; i < W; ++i) {
      if (i >= D) { buf[i] = (T)0; continue; }
      /* g_i = A_i - B_i (the engine's branch-free form; [.] selects +0) */
      const T am = a - x[i];
      const int hs = i <= D - 2, hp = (i >= 1) && (i <= D - 1);
      const T ti = hs ? x[i + 1] - x[i] * x[i] : (T)0;
      const T A = hs ? (b4 * x[i]) * ti + (T)2 * am : (T)0;
      const T B = hp ? b2 * (x[i] - x[i - 1] * x[i - 1]) : (T)0;
      g[i] = A - B;
      buf[i] = hs ? b * (ti * ti) + am * am : (T)0;
    }
    return -F(red)(buf, lanes, elems);
  }
  if (t->kind == 2) {
    const T var = (T)t->std * (T)t->std;
    for (int i = 0; i < W; ++i) {
      if (i < D) {
        g[i] = (-x[i]) / var;
        buf[i] = x[i] * x[i];
      } else {
        buf[i] = (T)0;
      }
    }
    return ((T)-0.5 * F(red)(buf, lanes, elems)) / var;
  }
  /* dense Gaussian: d = x - mu, w = P d (fma chain, j ascending), logp = nc - 0.5 sum w d */
  T d[D];
  for (int i = 0; i < D; ++i) d[i] = x[i] - (T)t->mean[i];
  for (int i = 0; i < W; ++i) {
    if (i >= D) { buf[i] = (T)0; continue; }
    T w = (T)0;
    for (int j = 0; j < D; ++j) {
      const T pij = (T)t->prec[(int64_t)i * D + j];
      w = FMA(pij, d[j], w);  /* fma chain, j ascending, from w = 0 */
    }
    g[i] = -w;
    buf[i] = w * d[i];
  }
  return (T)t->norm_const - F(red)(buf, lanes, elems) * (T)0.5;
}

T F(or_logp_grad)(const or_target* t, int lanes, int elems, const T* x, T* g) {
  return F(logp_grad_impl)(t, lanes, elems, x, g);
}

/* ------------------------------------------------------------------ HMC */
typedef struct {
  const or_target* t;
  int lanes, elems;
  int64_t C;
  int D;
  T* q;
  double eps;
  int L;
  uint64_t seed, step0;
  uint32_t chain_offset;
  int64_t n_steps, collect_from;
  T* samples;
  int64_t* accepts;
  int form;
} F(hmc_ctx);

/* BatchedGenericHMC::step + leapfrog (batched_hmc.rs:129-190), one chain.
 * form 0 is the engine's leapfrog (hmc_device.h): the kicks p + g*(eps/2)
 * and the drift q + p*eps are fused multiply-adds (one rounding each);
 * form 1 is the reference's op structure (batched_hmc.rs:166-190 through
 * add_scaled_assign, euclidean.rs:392-394: the product and the sum rounded
 * separately), which the composed tier-2 ops reproduce. */
static void F(hmc_chains)(void* vctx, int64_t c0, int64_t c1) {
  F(hmc_ctx)* cx = (F(hmc_ctx)*)vctx;
  const int D = cx->D, lanes = cx->lanes, elems = cx->elems;
  const T eps = (T)cx->eps;
  const T half = (T)0.5 * eps;
  const size_t nb = sizeof(T) * (size_t)(lanes * elems > D ? lanes * elems : D);
  T *q = malloc(nb), *g = malloc(nb), *p = malloc(nb);
  T *q1 = malloc(nb), *p1 = malloc(nb), *g1 = malloc(nb);
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t cid = cx->chain_offset + (uint32_t)c;
    memcpy(q, &cx->q[c * D], sizeof(T) * D);
    T lp = F(logp_grad_impl)(cx->t, lanes, elems, q, g);
    int64_t acc = 0;
    for (int64_t s = 0; s < cx->n_steps; ++s) {
      const uint64_t st = cx->step0 + (uint64_t)s;
      for (int i = 0; i < D; ++i) p[i] = MOM_NORMAL(cx->seed, cid, st, TAG_MOM, (uint32_t)i);
      const T ke0 = F(dot)(p, p, D, lanes, elems) * (T)0.5;
      memcpy(q1, q, sizeof(T) * D);
      memcpy(p1, p, sizeof(T) * D);
      memcpy(g1, g, sizeof(T) * D);
      T lp1 = lp;
      for (int l = 0; l < cx->L; ++l) {
        if (cx->form == 0) {
          for (int i = 0; i < D; ++i) p1[i] = FMA(g1[i], half, p1[i]);
          for (int i = 0; i < D; ++i) q1[i] = FMA(p1[i], eps, q1[i]);
          lp1 = F(logp_grad_impl)(cx->t, lanes, elems, q1, g1);
          for (int i = 0; i < D; ++i) p1[i] = FMA(g1[i], half, p1[i]);
        } else {
          for (int i = 0; i < D; ++i) p1[i] = p1[i] + g1[i] * half;
          for (int i = 0; i < D; ++i) q1[i] = q1[i] + p1[i] * eps;
          lp1 = F(logp_grad_impl)(cx->t, lanes, elems, q1, g1);
          for (int i = 0; i < D; ++i) p1[i] = p1[i] + g1[i] * half;
        }
      }
      const T ke1 = F(dot)(p1, p1, D, lanes, elems) * (T)0.5;
      const T la = (lp1 - lp) + (ke0 - ke1);
      const T lnu = LOG(UNIF_CO(cx->seed, cid, st, TAG_ACC, 0u));
      if (la >= lnu) {
        memcpy(q, q1, sizeof(T) * D);
        memcpy(g, g1, sizeof(T) * D);
        lp = lp1;
        ++acc;
      }
      if (s >= cx->collect_from && cx->samples)
        memcpy(&cx->samples[((s - cx->collect_from) * cx->C + c) * D], q, sizeof(T) * D);
    }
    memcpy(&cx->q[c * D], q, sizeof(T) * D);
    if (cx->accepts) cx->accepts[c] += acc;
  }
  free(q); free(g); free(p); free(q1); free(p1); free(g1);
}

int F(or_hmc_run)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, double eps,
                  int L, uint64_t seed, uint64_t step0, uint32_t chain_offset, int64_t n_steps,
                  int64_t collect_from, T* samples, int64_t* accepts, int threads, int form) {
  if (D < 1 || D > GM_MAX_DIM || lanes * elems < D || lanes > 1024 || (lanes > 64 && lanes % 64) ||
      (form != 0 && form != 1))
    return 1;
  F(hmc_ctx) cx = {t, lanes, elems, C, D, q, eps, L, seed, step0, chain_offset, n_steps,
                   collect_from, samples, accepts, form};
  parallel_chains(C, threads, F(hmc_chains), &cx);
  return 0;
}

/* ------------------------------------------------------------------- MH */
typedef struct {
  const or_target* t;
  int lanes, elems;
  int64_t C;
  int D;
  T* q;
  double prop_std;
  uint64_t seed, step0;
  uint32_t chain_offset;
  int64_t n_steps, collect_from;
  T* samples;
  int64_t* accepts;
  int form;
} F(mh_ctx);

/* Target::unnorm_logp in the reference's op structure (form 1 of MH): the
 * IsotropicGaussian's `sum = sum + x * x` left to right, then
 * -0.5 * sum / (std * std) (distributions.rs:398-406). The other built-in
 * targets' sums are burn tensor reductions in the reference (order not
 * pinned); they keep the canonical order. */
static T F(logp_ref)(const or_target* t, int lanes, int elems, const T* x, T* g) {
  if (t->kind != 2) return F(logp_grad_impl)(t, lanes, elems, x, g);
  T sum = (T)0;
  for (int i = 0; i < t->dim; ++i) sum = sum + x[i] * x[i];
  return ((T)-0.5 * sum) / ((T)t->std * (T)t->std);
}

/* IsotropicGaussian::logp(from, to) as written (distributions.rs:378-390):
 * lp += -(diff * diff) / (two * var) left to right, then
 * lp += -d * 0.5 * ln(var * pi * std * std) */
static T F(prop_logp_ref)(const T* from, const T* to, int D, T sd) {
  const T two = (T)2, var = sd * sd, pi = (T)3.14159265358979323846;
  T lp = (T)0;
  for (int i = 0; i < D; ++i) {
    const T diff = to[i] - from[i];
    lp += -(diff * diff) / (two * var);
  }
  lp += -(T)D * (T)0.5 * RLOG(var * pi * sd * sd);
  return lp;
}

/* One MH proposal of a chain at counter step st and its log acceptance
 * ratio. Form 0 (the kernels' arithmetic): the proposal density's terms and
 * the target's in the canonical order, the forward and backward densities
 * one value (they are bitwise equal: (-d)^2 = d^2); form 1 (the reference's
 * op structure, metropolis_hastings.rs:306-318): every sum left to right,
 * log q forward and backward computed separately, the current state's
 * log-density recomputed from x. lp (form 0) is the carried log-density. */
static T F(mh_propose)(const or_target* t, int lanes, int elems, int D, const T* x, T lp, T* y, T* g, T* buf,
                       T sd, uint64_t seed, uint32_t cid, uint64_t st, int form, T* lp1_out) {
  const int W = lanes * elems;
  const T var = sd * sd, two_var = (T)2 * var;
  const T pi = (T)3.14159265358979323846;
  for (int i = 0; i < D; ++i) y[i] = x[i] + MH_NORMAL(seed, cid, st, TAG_MH_PROP, (uint32_t)i) * sd;
  if (form == 1) {
    const T current_lp = F(logp_ref)(t, lanes, elems, x, g);
    const T proposed_lp = F(logp_ref)(t, lanes, elems, y, g);
    const T log_q_forward = F(prop_logp_ref)(x, y, D, sd);
    const T log_q_backward = F(prop_logp_ref)(y, x, D, sd);
    *lp1_out = proposed_lp;
    return (proposed_lp + log_q_backward) - (current_lp + log_q_forward);
  }
  const T qconst = (-(T)D * (T)0.5) * LOG(((var * pi) * sd) * sd);
  /* the symmetric proposal's log q terms cancel whenever they are finite
   * (2 var normal, the constant finite): log alpha = lp1 - lp, the kernels'
   * form (mh_device.h `cancel`); otherwise the full form */
  if (isnormal(two_var) && isfinite(qconst)) {
    const T lp1 = F(logp_grad_impl)(t, lanes, elems, y, g);
    *lp1_out = lp1;
    return lp1 - lp;
  }
  for (int i = 0; i < W; ++i) {
    if (i < D) {
      const T d = y[i] - x[i];
      buf[i] = (-(d * d)) / two_var;
    } else {
      buf[i] = (T)0;
    }
  }
  const T logq = F(red)(buf, lanes, elems) + qconst;
  const T lp1 = F(logp_grad_impl)(t, lanes, elems, y, g);
  *lp1_out = lp1;
  return (lp1 + logq) - (lp + logq);
}

/* MHMarkovChain::step (metropolis_hastings.rs:306-318) with the
 * IsotropicGaussian proposal (distributions.rs:368-390) */
static void F(mh_chains)(void* vctx, int64_t c0, int64_t c1) {
  F(mh_ctx)* cx = (F(mh_ctx)*)vctx;
  const int D = cx->D, lanes = cx->lanes, elems = cx->elems;
  const T sd = (T)cx->prop_std;
  T *x = malloc(sizeof(T) * 1024), *y = malloc(sizeof(T) * 1024), *g = malloc(sizeof(T) * 1024);
  T* buf = malloc(sizeof(T) * 1024);
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t cid = cx->chain_offset + (uint32_t)c;
    memcpy(x, &cx->q[c * D], sizeof(T) * D);
    T lp = F(logp_grad_impl)(cx->t, lanes, elems, x, g);
    int64_t acc = 0;
    for (int64_t s = 0; s < cx->n_steps; ++s) {
      const uint64_t st = cx->step0 + (uint64_t)s;
      T lp1;
      const T la = F(mh_propose)(cx->t, lanes, elems, D, x, lp, y, g, buf, sd, cx->seed, cid, st, cx->form, &lp1);
      const T lnu = MLOG(cx->form, UNIF_CO(cx->seed, cid, st, TAG_MH_ACC, 0u));
      if (la > lnu) {
        memcpy(x, y, sizeof(T) * D);
        lp = lp1;
        ++acc;
      }
      if (s >= cx->collect_from && cx->samples)
        memcpy(&cx->samples[((s - cx->collect_from) * cx->C + c) * D], x, sizeof(T) * D);
    }
    memcpy(&cx->q[c * D], x, sizeof(T) * D);
    if (cx->accepts) cx->accepts[c] += acc;
  }
  free(x); free(y); free(g); free(buf);
}

int F(or_mh_run)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, double prop_std,
                 uint64_t seed, uint64_t step0, uint32_t chain_offset, int64_t n_steps,
                 int64_t collect_from, T* samples, int64_t* accepts, int threads, int form) {
  if (D < 1 || D > 1024 || lanes * elems < D || lanes > 64 || (form != 0 && form != 1)) return 1;
  F(mh_ctx) cx = {t, lanes, elems, C, D, q, prop_std, seed, step0, chain_offset, n_steps,
                  collect_from, samples, accepts, form};
  parallel_chains(C, threads, F(mh_chains), &cx);
  return 0;
}

/* one MH step's terms for every chain from the states x [C][D] at counter
 * step st, in the given form: la [C] the log acceptance ratio, lp1 [C] the
 * proposal's log-density, lnu [C] the accept log-uniform. Nothing moves. */
typedef struct {
  const or_target* t;
  int lanes, elems, D, form;
  const T* x;
  double prop_std;
  uint64_t seed, st;
  uint32_t chain_offset;
  T *la, *lp1, *lnu;
} F(mh_terms_ctx);
static void F(mh_terms_chains)(void* vctx, int64_t c0, int64_t c1) {
  F(mh_terms_ctx)* cx = (F(mh_terms_ctx)*)vctx;
  T *y = malloc(sizeof(T) * 1024), *g = malloc(sizeof(T) * 1024), *buf = malloc(sizeof(T) * 1024);
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t cid = cx->chain_offset + (uint32_t)c;
    const T* x = cx->x + c * cx->D;
    const T lp = F(logp_grad_impl)(cx->t, cx->lanes, cx->elems, x, g);
    cx->la[c] = F(mh_propose)(cx->t, cx->lanes, cx->elems, cx->D, x, lp, y, g, buf, (T)cx->prop_std, cx->seed,
                              cid, cx->st, cx->form, &cx->lp1[c]);
    cx->lnu[c] = MLOG(cx->form, UNIF_CO(cx->seed, cid, cx->st, TAG_MH_ACC, 0u));
  }
  free(y); free(g); free(buf);
}
int F(or_mh_terms)(const or_target* t, int lanes, int elems, int64_t C, int D, const T* x, double prop_std,
                   uint64_t seed, uint64_t st, uint32_t chain_offset, int form, T* la, T* lp1, T* lnu,
                   int threads) {
  if (D < 1 || D > 1024 || lanes * elems < D || lanes > 64 || (form != 0 && form != 1)) return 1;
  F(mh_terms_ctx) cx = {t, lanes, elems, D, form, x, prop_std, seed, st, chain_offset, la, lp1, lnu};
  parallel_chains(C, threads, F(mh_terms_chains), &cx);
  return 0;
}

/* ----------------------------------------------------------------- NUTS */
typedef struct {
  T *qm, *pm, *gm, *qp, *pp, *gp, *qprime, *gprime;
  T *vm, *wm, *vp, *wp; /* dense metric: M^-1 p and M^-1 g at the ends (carried) */
  T logp_prime;
  int64_t n;
  int s;
  T alpha;
  int64_t n_alpha;
} F(tree);

/* MassMatrix (generic_nuts.rs:175-304) of one chain: kind 0 identity,
 * 1 diagonal (inv, sq = sqrt of the variance), 2 dense (inv, chol; D x D) */
typedef struct {
  int kind;
  T *inv, *sq, *chol;
} F(mass);

typedef struct {
  const or_target* t;
  int lanes, elems, D;
  uint64_t seed, step;
  uint32_t cid;
  uint32_t merge_ctr;
  uint64_t key;   /* the transition's stream key (or_nuts_key) */
  F(tree) ws[32]; /* per-level workspace for the second subtree */
  T* tmpv;
  T* tmpv2;
  int64_t nlf;
  F(mass) M;
  int form; /* 0: the engine's arithmetic (the kernels); 1: the reference's op structure */
} F(nctx);

/* canonical-order sum of a D-vector */
static T F(csum)(const T* v, int D, int lanes, int elems) {
  T buf[1024];
  const int W = lanes * elems;
  for (int i = 0; i < W; ++i) buf[i] = (i < D) ? v[i] : (T)0;
  return F(red)(buf, lanes, elems);
}

/* MassMatrix::inv_mul (:258-276): out = M^-1 p. Dense: form 0 is the
 * engine's fma chain (j ascending from +0, the dense Gaussian product's form);
 * form 1 the reference's `acc = acc + inv[i*dim+j] * input[j]` (:266-273),
 * product and sum rounded separately. */
static void F(inv_mul)(const F(mass)* M, const T* p, T* out, int D, int form) {
  if (M->kind == 1) {
    for (int i = 0; i < D; ++i) out[i] = M->inv[i] * p[i];
  } else if (M->kind == 2) {
    for (int i = 0; i < D; ++i) {
      T acc = (T)0;
      if (form == 1)
        for (int j = 0; j < D; ++j) acc = acc + M->inv[i * D + j] * p[j];
      else
        for (int j = 0; j < D; ++j) acc = FMA(M->inv[i * D + j], p[j], acc);
      out[i] = acc;
    }
  } else {
    for (int i = 0; i < D; ++i) out[i] = p[i];
  }
}

/* MassMatrix::sample_momentum (:275-303) applied to standard normals z */
static void F(momentum_from)(const F(mass)* M, const T* z, T* out, int D) {
  if (M->kind == 1) {
    for (int i = 0; i < D; ++i) out[i] = z[i] * M->sq[i];
  } else if (M->kind == 2) {
    for (int i = 0; i < D; ++i) {
      T acc = (T)0;
      for (int j = 0; j <= i; ++j) acc = acc + M->chol[i * D + j] * z[j];
      out[i] = acc;
    }
  } else {
    for (int i = 0; i < D; ++i) out[i] = z[i];
  }
}

static void F(tree_alloc)(F(tree)* tr, int D) {
  T* b = (T*)malloc(sizeof(T) * 12 * (D > 0 ? D : 1));
  tr->qm = b; tr->pm = b + D; tr->gm = b + 2 * D; tr->qp = b + 3 * D;
  tr->pp = b + 4 * D; tr->gp = b + 5 * D; tr->qprime = b + 6 * D; tr->gprime = b + 7 * D;
  tr->vm = b + 8 * D; tr->wm = b + 9 * D; tr->vp = b + 10 * D; tr->wp = b + 11 * D;
}

/* MassMatrix::kinetic (:227-256). Form 0: the sum over coordinates in the
 * engine's canonical order (identity: p*p, diagonal: p*p*inv, dense:
 * p_i * (M^-1 p)_i); form 1: the reference's loops as written, left to right,
 * the dense form's row products `row_dot + inv[i*dim+j]*p[j]` (:244-253). */
static T F(kinetic)(F(nctx)* cx, const T* p) {
  const int D = cx->D;
  if (cx->form == 1) {
    T q = (T)0;
    if (cx->M.kind == 2) {
      for (int i = 0; i < D; ++i) {
        T row_dot = (T)0;
        for (int j = 0; j < D; ++j) row_dot = row_dot + cx->M.inv[i * D + j] * p[j];
        q = q + p[i] * row_dot;
      }
    } else if (cx->M.kind == 1) {
      for (int i = 0; i < D; ++i) q = q + p[i] * p[i] * cx->M.inv[i];
    } else {
      for (int i = 0; i < D; ++i) q = q + p[i] * p[i];
    }
    return (T)0.5 * q;
  }
  if (cx->M.kind == 1) {
    for (int i = 0; i < D; ++i) cx->tmpv2[i] = p[i] * p[i] * cx->M.inv[i];
    return (T)0.5 * F(csum)(cx->tmpv2, D, cx->lanes, cx->elems);
  }
  if (cx->M.kind == 2) {
    F(inv_mul)(&cx->M, p, cx->tmpv2, D, 0);
    for (int i = 0; i < D; ++i) cx->tmpv2[i] = p[i] * cx->tmpv2[i];
    return (T)0.5 * F(csum)(cx->tmpv2, D, cx->lanes, cx->elems);
  }
  return (T)0.5 * F(dot)(p, p, D, cx->lanes, cx->elems);
}

/* leapfrog_with_mass (generic_nuts.rs:1396-1418): drift by M^-1 p. With
 * vw_v (form 0, dense) the engine's carried velocity; otherwise the
 * reference's structure: M^-1 of the kicked momentum every leapfrog. */
static T F(leapfrog)(F(nctx)* cx, T* q, T* p, T* g, T* vw_v, T* vw_w, T epsv) {
  const int D = cx->D;
  const T h = epsv * (T)0.5;
  if (cx->M.kind == 2 && vw_v) {
    /* dense metric, the engine's carried velocity (nuts_device.h): v = M^-1 p
     * and w = M^-1 g of the starting point are carried by linearity,
     * M^-1 (p + g h) = v + w h: one product per leapfrog (w at the new
     * point) instead of M^-1 of the kicked momentum and of the final one */
    for (int i = 0; i < D; ++i) p[i] = p[i] + g[i] * h;
    for (int i = 0; i < D; ++i) vw_v[i] = vw_v[i] + vw_w[i] * h;
    for (int i = 0; i < D; ++i) q[i] = q[i] + vw_v[i] * epsv;
    const T lp = F(logp_grad_impl)(cx->t, cx->lanes, cx->elems, q, g);
    F(inv_mul)(&cx->M, g, vw_w, D, 0);
    for (int i = 0; i < D; ++i) p[i] = p[i] + g[i] * h;
    for (int i = 0; i < D; ++i) vw_v[i] = vw_v[i] + vw_w[i] * h;
    cx->nlf++;
    return lp;
  }
  for (int i = 0; i < D; ++i) p[i] = p[i] + g[i] * h;
  F(inv_mul)(&cx->M, p, cx->tmpv2, D, cx->form);
  for (int i = 0; i < D; ++i) q[i] = q[i] + cx->tmpv2[i] * epsv;
  const T lp = F(logp_grad_impl)(cx->t, cx->lanes, cx->elems, q, g);
  for (int i = 0; i < D; ++i) p[i] = p[i] + g[i] * h;
  cx->nlf++;
  return lp;
}

/* MassMatrix::kinetic with the carried v = M^-1 p (dense): 0.5 sum p_i v_i */
static T F(kinetic_v)(F(nctx)* cx, const T* p, const T* v) {
  for (int i = 0; i < cx->D; ++i) cx->tmpv2[i] = p[i] * v[i];
  return (T)0.5 * F(csum)(cx->tmpv2, cx->D, cx->lanes, cx->elems);
}

/* a plain left-to-right dot from +0: form 1's order for the U-turn dots. The
 * reference's `diff.dot(&vel)` (generic_nuts.rs:1375-1376) is
 * `mul(..).sum()` on a burn tensor (euclidean.rs:316-318, 400-403), whose
 * summation order is the backend's and not pinned by the reference; the
 * sequential order stands for "not the engine's lane butterfly". */
static T F(dot_lr)(const T* a, const T* b, int D) {
  T s = (T)0;
  for (int i = 0; i < D; ++i) s = s + a[i] * b[i];
  return s;
}

/* stop_criterion(_with_mass), identity (generic_nuts.rs:1343-1378). Form 0:
 * the dots in the engine's canonical order; form 1: left to right. */
static int F(no_uturn)(F(nctx)* cx, const T* qm, const T* qp, const T* pm, const T* pp) {
  const int D = cx->D;
  for (int i = 0; i < D; ++i) cx->tmpv[i] = qp[i] - qm[i];
  if (cx->form == 1) {
    const T dm = F(dot_lr)(cx->tmpv, pm, D), dp = F(dot_lr)(cx->tmpv, pp, D);
    return dm >= (T)0 && dp >= (T)0;
  }
  const T dm = F(dot)(cx->tmpv, pm, D, cx->lanes, cx->elems);
  const T dp = F(dot)(cx->tmpv, pp, D, cx->lanes, cx->elems);
  return dm >= (T)0 && dp >= (T)0;
}

/* stop_criterion_with_mass (:1354-1378): the top-level U-turn uses M^-1 p */
static int F(no_uturn_m)(F(nctx)* cx, const T* qm, const T* qp, const T* pm, const T* pp) {
  if (cx->M.kind == 0) return F(no_uturn)(cx, qm, qp, pm, pp);
  const int D = cx->D;
  T* vm = (T*)malloc(sizeof(T) * D);
  T* vp = (T*)malloc(sizeof(T) * D);
  T* d = (T*)malloc(sizeof(T) * D);
  for (int i = 0; i < D; ++i) d[i] = qp[i] - qm[i];
  F(inv_mul)(&cx->M, pm, vm, D, cx->form);
  F(inv_mul)(&cx->M, pp, vp, D, cx->form);
  const T dm = cx->form == 1 ? F(dot_lr)(d, vm, D) : F(dot)(d, vm, D, cx->lanes, cx->elems);
  const T dp = cx->form == 1 ? F(dot_lr)(d, vp, D) : F(dot)(d, vp, D, cx->lanes, cx->elems);
  free(vm); free(vp); free(d);
  return dm >= (T)0 && dp >= (T)0;
}

static T F(rust_min1)(T x) { return (x != x) ? (T)1 : (x < (T)1 ? x : (T)1); }

/* build_tree_with_mass (generic_nuts.rs:1153-1341), identity mass */
static void F(build_tree)(F(nctx)* cx, const T* q, const T* p, const T* g, const T* vq, const T* wq, T logu,
                          int v, int j, T eps, T joint0, F(tree)* out) {
  const int D = cx->D;
  const size_t vb = sizeof(T) * D;
  const int cv = cx->M.kind == 2 && cx->form == 0; /* carried M^-1 p, M^-1 g (the engine's form) */
  if (j == 0) {
    memcpy(out->qprime, q, vb);
    memcpy(out->pm, p, vb);
    memcpy(out->gprime, g, vb);
    if (cv) { memcpy(out->vm, vq, vb); memcpy(out->wm, wq, vb); }
    const T lp = F(leapfrog)(cx, out->qprime, out->pm, out->gprime, cv ? out->vm : NULL, cv ? out->wm : NULL,
                             (T)v * eps);
    const T joint = lp - (cv ? F(kinetic_v)(cx, out->pm, out->vm) : F(kinetic)(cx, out->pm));
    if (cv) { memcpy(out->vp, out->vm, vb); memcpy(out->wp, out->wm, vb); }
    out->n = (logu < joint) ? 1 : 0;
    out->s = (logu - (T)1000) < joint;
    memcpy(out->qm, out->qprime, vb);
    memcpy(out->qp, out->qprime, vb);
    memcpy(out->pp, out->pm, vb);
    memcpy(out->gm, out->gprime, vb);
    memcpy(out->gp, out->gprime, vb);
    out->logp_prime = lp;
    /* form 0, f64: the kernels' division-free min(1, exp(.)) (or_leaf_alpha_d) */
    out->alpha = (cx->form == 0 && sizeof(T) == 8) ? (T)or_leaf_alpha_d((double)(joint - joint0))
                                                   : F(rust_min1)(MEXP(cx->form, joint - joint0));
    out->n_alpha = 1;
    return;
  }
  F(build_tree)(cx, q, p, g, vq, wq, logu, v, j - 1, eps, joint0, out);
  if (out->s) {
    F(tree)* s2 = &cx->ws[j];
    if (v == -1) F(build_tree)(cx, out->qm, out->pm, out->gm, out->vm, out->wm, logu, v, j - 1, eps, joint0, s2);
    else F(build_tree)(cx, out->qp, out->pp, out->gp, out->vp, out->wp, logu, v, j - 1, eps, joint0, s2);
    if (v == -1) {
      memcpy(out->qm, s2->qm, vb);
      memcpy(out->pm, s2->pm, vb);
      memcpy(out->gm, s2->gm, vb);
      if (cv) { memcpy(out->vm, s2->vm, vb); memcpy(out->wm, s2->wm, vb); }
    } else {
      memcpy(out->qp, s2->qp, vb);
      memcpy(out->pp, s2->pp, vb);
      memcpy(out->gp, s2->gp, vb);
      if (cv) { memcpy(out->vp, s2->vp, vb); memcpy(out->wp, s2->wp, vb); }
    }
    const double u = or_nuts_u_d(cx->key, 64u + cx->merge_ctr++);
    const int64_t den = (out->n + s2->n) > 1 ? (out->n + s2->n) : 1;
    if (u < (double)s2->n / (double)den) {
      memcpy(out->qprime, s2->qprime, vb);
      memcpy(out->gprime, s2->gprime, vb);
      out->logp_prime = s2->logp_prime;
    }
    out->n += s2->n;
    out->s = out->s && s2->s && F(no_uturn)(cx, out->qm, out->qp, out->pm, out->pp);
    out->alpha = out->alpha + s2->alpha;
    out->n_alpha += s2->n_alpha;
  }
}

/* find_reasonable_epsilon_with_mass (generic_nuts.rs:1025-1102), identity */
static T F(find_eps)(F(nctx)* cx, const T* q0, const T* p0) {
  const F(mass) saved = cx->M;
  cx->M.kind = 0;  /* find_reasonable_epsilon always integrates with identity mass */
  const int D = cx->D;
  const size_t vb = sizeof(T) * D;
  const T half = (T)0.5;
  T eps = (T)1;
  T *g0 = malloc(vb), *q = malloc(vb), *p = malloc(vb), *g = malloc(vb);
  const T ulogp = F(logp_grad_impl)(cx->t, cx->lanes, cx->elems, q0, g0);
  memcpy(q, q0, vb); memcpy(p, p0, vb); memcpy(g, g0, vb);
  T ulogp1 = F(leapfrog)(cx, q, p, g, NULL, NULL, eps);
  T k = (T)1;
  for (int it = 0; it < 1100; ++it) {
    int fin = isfinite(ulogp1);
    for (int i = 0; i < D && fin; ++i) fin = isfinite(g[i]);
    if (fin) break;
    k = k * half;
    memcpy(q, q0, vb); memcpy(p, p0, vb); memcpy(g, g0, vb);
    ulogp1 = F(leapfrog)(cx, q, p, g, NULL, NULL, eps * k);
  }
  eps = half * k * eps;
  const T k0 = F(kinetic)(cx, p0);
  T la = ulogp1 - ulogp - (F(kinetic)(cx, p) - k0);
  const T a = (la > MLOG(cx->form, half)) ? (T)1 : (T)-1;
  const T ln2 = MLOG(cx->form, (T)2);
  for (int it = 0; it < 2200; ++it) {
    if (!(a * la > -a * ln2)) break;
    eps = eps * (a > (T)0 ? (T)2 : (T)0.5);
    memcpy(q, q0, vb); memcpy(p, p0, vb); memcpy(g, g0, vb);
    ulogp1 = F(leapfrog)(cx, q, p, g, NULL, NULL, eps);
    la = ulogp1 - ulogp - (F(kinetic)(cx, p) - k0);
  }
  free(g0); free(q); free(p); free(g);
  cx->M = saved;
  return eps;
}

/* ---- mass-matrix warm-up (generic_nuts.rs:81-172, 306-359, 948-997) ---- */
static int F(cholesky_spd)(const T* a, int dim, T* l) {
  for (int i = 0; i < dim * dim; ++i) l[i] = (T)0;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j <= i; ++j) {
      T sum = a[i * dim + j];
      for (int k = 0; k < j; ++k) sum = sum - l[i * dim + k] * l[j * dim + k];
      if (i == j) {
        if (sum <= (T)0 || !isfinite(sum)) return 0;
        l[i * dim + j] = SQRT(sum);
      } else {
        const T d = l[j * dim + j];
        if (d <= (T)0 || !isfinite(d)) return 0;
        l[i * dim + j] = sum / d;
      }
    }
  return 1;
}
static int F(invert_spd_from_cholesky)(const T* l, int dim, T* inv, T* inv_l) {
  for (int i = 0; i < dim * dim; ++i) inv_l[i] = (T)0;
  for (int i = 0; i < dim; ++i) {
    const T d = l[i * dim + i];
    if (d <= (T)0 || !isfinite(d)) return 0;
    inv_l[i * dim + i] = (T)1 / d;
    for (int j = i + 1; j < dim; ++j) {
      T sum = (T)0;
      for (int k = i; k < j; ++k) sum = sum + l[j * dim + k] * inv_l[k * dim + i];
      inv_l[j * dim + i] = -sum / l[j * dim + j];
    }
  }
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j <= i; ++j) {
      T sum = (T)0;
      for (int k = (i > j ? i : j); k < dim; ++k) sum = sum + inv_l[k * dim + i] * inv_l[k * dim + j];
      inv[i * dim + j] = sum;
      inv[j * dim + i] = sum;
    }
  return 1;
}
static T F(fmax_)(T a, T b) { return (a != a) ? b : (b != b) ? a : (a > b ? a : b); }  /* Float::max */

/* MassMatrix::diagonal_from_var (:205-216) into (inv, sq) */
static void F(diag_from_var)(const T* var, int D, T jitter, T* inv, T* sq) {
  for (int i = 0; i < D; ++i) {
    const T v = F(fmax_)(var[i], jitter);
    inv[i] = (T)1 / v;
    sq[i] = SQRT(v);
  }
}
/* MassMatrix::dense_from_cov (:218-236); 1 on success */
static int F(dense_from_cov)(const T* cov, int dim, T jitter, T* inv, T* chol) {
  T j = F(fmax_)(jitter, (T)1e-10);
  T* tr = (T*)malloc(sizeof(T) * dim * dim);
  T* il = (T*)malloc(sizeof(T) * dim * dim);
  int ok = 0;
  for (int t = 0; t < 8 && !ok; ++t) {
    memcpy(tr, cov, sizeof(T) * dim * dim);
    for (int d = 0; d < dim; ++d) tr[d * dim + d] = tr[d * dim + d] + j;
    if (F(cholesky_spd)(tr, dim, chol) && F(invert_spd_from_cholesky)(chol, dim, inv, il)) ok = 1;
    else j = j * (T)10;
  }
  free(tr);
  free(il);
  return ok;
}

/* RunningCov (:81-130) */
typedef struct {
  int64_t n;
  T *mean, *m2d, *m2, *delta;
} F(running);
static void F(running_reset)(F(running)* r, int D, int dense) {
  r->n = 0;
  memset(r->mean, 0, sizeof(T) * D);
  memset(r->m2d, 0, sizeof(T) * D);
  if (dense) memset(r->m2, 0, sizeof(T) * D * D);
}
static void F(running_update)(F(running)* r, const T* x, int D, int dense) {
  r->n += 1;
  const T ns = (T)r->n;
  for (int i = 0; i < D; ++i) {
    r->delta[i] = x[i] - r->mean[i];
    r->mean[i] = r->mean[i] + r->delta[i] / ns;
    const T d2 = x[i] - r->mean[i];
    r->m2d[i] = r->m2d[i] + r->delta[i] * d2;
  }
  if (dense)
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) r->m2[i * D + j] = r->m2[i * D + j] + r->delta[i] * (x[j] - r->mean[j]);
}

/* maybe_update_mass_matrix (:948-997) into the chain's mass; 1 if updated */
static int F(maybe_update)(const or_mass_cfg* cfg, const F(running)* r, int D, F(mass)* M, T* dinv,
                           T* dsq) {
  const int64_t n = r->n;
  if (n < 5) return 0;
  const T nd = (T)(n - 1);
  const T reg = (T)cfg->regularize;
  const T omr = (T)1 - reg;
  const T jitter = (T)(cfg->jitter > 1e-10 ? cfg->jitter : 1e-10);
  T* var = (T*)malloc(sizeof(T) * D * (cfg->mode == 2 ? D : 1));
  int updated = 0;
  if (cfg->mode == 1) {
    for (int i = 0; i < D; ++i) var[i] = F(fmax_)(omr * (r->m2d[i] / nd) + reg, jitter);
    F(diag_from_var)(var, D, jitter, dinv, dsq);
    M->kind = 1;
    updated = 1;
  } else if (cfg->mode == 2) {
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) {
        const T raw = r->m2[i * D + j] / nd;
        const T v = (i == j) ? F(fmax_)(omr * raw + reg, jitter) : omr * raw;
        var[i * D + j] = v;
        var[j * D + i] = v;
      }
    T* inv = (T*)malloc(sizeof(T) * D * D);
    T* chol = (T*)malloc(sizeof(T) * D * D);
    if (F(dense_from_cov)(var, D, jitter, inv, chol)) {
      memcpy(M->inv, inv, sizeof(T) * D * D);
      memcpy(M->chol, chol, sizeof(T) * D * D);
      M->kind = 2;
      updated = 1;
    } else if (M->kind == 0) {  /* identity -> diagonal_from_var(ones) */
      for (int i = 0; i < D; ++i) var[i] = (T)1;
      F(diag_from_var)(var, D, jitter, dinv, dsq);
      M->kind = 1;
      updated = 1;
    }
    free(inv);
    free(chol);
  }
  free(var);
  return updated;
}

/* MassMatrixWarmup::should_collect / note_if_window_end (:153-172) */
static int F(should_collect)(const or_mass_cfg* cfg, int64_t m, int64_t nw) {
  if (m == 0 || m > nw) return 0;
  if (m <= cfg->start_buffer) return 0;
  const int64_t lim = nw > cfg->end_buffer ? nw - cfg->end_buffer : 0;
  return m < lim;
}
static int F(note_window_end)(const or_mass_cfg* cfg, int64_t* sched, int64_t m, int64_t nw) {
  if (!F(should_collect)(cfg, m, nw)) return 0;
  const int64_t lim = nw > cfg->end_buffer ? nw - cfg->end_buffer : 0;
  if (m >= sched[0] || m + 1 >= lim) {
    sched[0] = sched[0] + sched[1];
    sched[1] = sched[1] * 2 < 400 ? sched[1] * 2 : 400;
    return 1;
  }
  return 0;
}

typedef struct {
  const or_target* t;
  int lanes, elems;
  int64_t C;
  int D;
  T *q, *eps, *eps_bar, *h_bar, *mu;
  double target_accept;
  int max_depth;
  uint64_t seed, init_step;
  uint32_t chain_offset;
  int64_t n_collect, n_discard;
  int progress;
  T* samples;
  int64_t *accepts, *n_leapfrog;
  const or_mass_cfg* mcfg; /* NULL or mode 0: identity, no warm-up */
  or_mass_state* ms;
  int64_t* sched_out;      /* [C][2] */
  int64_t m0;              /* progress == 2 (step): adaptation counter before the first step */
  int32_t* depth;          /* NULL or [C]: the tree depth of each chain's last transition */
} F(nuts_ctx);

static void F(nuts_chains)(void* vctx, int64_t c0, int64_t c1) {
  F(nuts_ctx)* a = (F(nuts_ctx)*)vctx;
  const int D = a->D;
  const size_t vb = sizeof(T) * D;
  F(nctx) cx;
  memset(&cx, 0, sizeof(cx));
  cx.t = a->t; cx.lanes = a->lanes; cx.elems = a->elems; cx.D = D; cx.seed = a->seed;
  cx.form = a->mcfg ? a->mcfg->form : 0;
  for (int k = 0; k < 32; ++k) F(tree_alloc)(&cx.ws[k], D);
  cx.tmpv = malloc(vb);
  cx.tmpv2 = malloc(vb);
  const int mmode = (a->mcfg && a->ms) ? a->mcfg->mode : 0;
  F(running) run;
  run.mean = malloc(vb); run.m2d = malloc(vb); run.delta = malloc(vb);
  run.m2 = mmode == 2 ? malloc(vb * D) : NULL;
  T* zb = malloc(vb);
  F(tree) top;
  F(tree_alloc)(&top, D);
  T *q = malloc(vb), *p0 = malloc(vb), *g0 = malloc(vb);
  T *qm = malloc(vb), *pm = malloc(vb), *gm = malloc(vb), *qp = malloc(vb), *pp = malloc(vb), *gp = malloc(vb);
  T *vm = malloc(vb), *wm = malloc(vb), *vp = malloc(vb), *wp = malloc(vb);
  const T gamma = (T)0.05, kappa = (T)0.75, delta = (T)a->target_accept;
  const int64_t t0c = 10;
  int64_t total, row_shift;
  const int step_mode = a->progress == 2; /* GenericNUTSChain::step (generic_nuts.rs:755): no init */
  if (step_mode) { total = a->n_collect; row_shift = INT64_MAX; }
  else if (a->progress) { total = a->n_discard + a->n_collect; row_shift = a->n_discard + 1; }
  else { total = a->n_discard + a->n_collect - 1; row_shift = a->n_discard; }
  for (int64_t c = c0; c < c1; ++c) {
    const uint32_t cid = a->chain_offset + (uint32_t)c;
    cx.cid = cid;
    memcpy(q, &a->q[c * D], vb);
    T eps = a->eps[c], eps_bar = a->eps_bar[c], h_bar = a->h_bar[c], mu = a->mu[c];
    int64_t sched[2] = {0, 0};
    T *dinv = NULL, *dsq = NULL;
    if (mmode) {
      cx.M.kind = a->ms->kind[c];
      dinv = (T*)a->ms->dinv + c * D;
      dsq = (T*)a->ms->dsqrt + c * D;
      if (mmode == 2) {
        cx.M.chol = (T*)a->ms->mchol + c * D * D;
        cx.M.inv = cx.M.kind == 2 ? (T*)a->ms->minv + c * D * D : dinv;
      } else {
        cx.M.inv = dinv;
      }
      cx.M.sq = dsq;
      sched[0] = a->ms->sched[0];
      sched[1] = a->ms->sched[1];
      F(running_reset)(&run, D, mmode == 2);
    } else {
      cx.M.kind = 0;
    }
    if (!step_mode) {
      /* init_chain_state (generic_nuts.rs:731-753) */
      for (int i = 0; i < D; ++i) zb[i] = NORMAL(a->seed, cid, a->init_step, TAG_NUTS_INIT, (uint32_t)i);
      F(momentum_from)(&cx.M, zb, p0, D);
      const T ae = eps + (T)1;
      if ((ae < (T)0 ? -ae : ae) <= MACH_EPS) eps = F(find_eps)(&cx, q, p0);
      mu = MLOG(cx.form, (T)10 * eps);
    }
    int64_t acc = 0;
    cx.nlf = 0;
    if (row_shift == 0 && a->samples) memcpy(&a->samples[(0 * a->C + c) * D], q, vb);
    for (int64_t s = 0; s < total; ++s) {
      const uint64_t st = a->init_step + (uint64_t)s;
      const int64_t m = (step_mode ? a->m0 : 0) + s + 1;
      cx.step = st;
      cx.merge_ctr = 0;
      uint32_t kw[4];
      cx.key = or_nuts_key(a->seed, cid, st, kw);
      /* GenericNUTSChain::step (generic_nuts.rs:755-925) */
      for (int i = 0; i < D; ++i) zb[i] = NORMAL(a->seed, cid, st, TAG_NUTS_MOM, (uint32_t)i);
      F(momentum_from)(&cx.M, zb, p0, D);
      const T logp = F(logp_grad_impl)(a->t, a->lanes, a->elems, q, g0);
      /* dense, form 0: carried M^-1 p0, M^-1 g0 at both ends */
      const int cv = cx.M.kind == 2 && cx.form == 0;
      if (cv) { F(inv_mul)(&cx.M, p0, vm, D, 0); F(inv_mul)(&cx.M, g0, wm, D, 0); }
      const T joint = logp - (cv ? F(kinetic_v)(&cx, p0, vm) : F(kinetic)(&cx, p0));
      const T logu = joint - NUTS_EXP1(kw);
      memcpy(qm, q, vb); memcpy(qp, q, vb); memcpy(pm, p0, vb); memcpy(pp, p0, vb);
      memcpy(gm, g0, vb); memcpy(gp, g0, vb);
      if (cv) { memcpy(vp, vm, vb); memcpy(wp, wm, vb); }
      int j = 0;
      int64_t n = 1;
      int sgo = 1;
      T alpha = (T)0;
      int64_t n_alpha = 0;
      while (sgo && j < a->max_depth) {
        const T u1 = NUTS_U(cx.key, 2u * (uint32_t)j);
        const int v = (u1 < (T)0.5) ? 1 : -1;
        if (v == -1) {
          F(build_tree)(&cx, qm, pm, gm, vm, wm, logu, v, j, eps, joint, &top);
          memcpy(qm, top.qm, vb); memcpy(pm, top.pm, vb); memcpy(gm, top.gm, vb);
          if (cv) { memcpy(vm, top.vm, vb); memcpy(wm, top.wm, vb); }
        } else {
          F(build_tree)(&cx, qp, pp, gp, vp, wp, logu, v, j, eps, joint, &top);
          memcpy(qp, top.qp, vb); memcpy(pp, top.pp, vb); memcpy(gp, top.gp, vb);
          if (cv) { memcpy(vp, top.vp, vb); memcpy(wp, top.wp, vb); }
        }
        alpha = top.alpha;
        n_alpha = top.n_alpha;
        const T tmp = F(rust_min1)((T)top.n / (T)n);
        const T u2 = NUTS_U(cx.key, 2u * (uint32_t)j + 1u);
        if (top.s && (u2 < tmp)) {
          memcpy(q, top.qprime, vb);
          ++acc;
        }
        n += top.n;
        /* dense: the ends' carried M^-1 p, as stop_criterion_with_mass's
         * products (identity form of no_uturn applied to them) */
        sgo = top.s && (cv ? F(no_uturn)(&cx, qm, qp, vm, vp) : F(no_uturn_m)(&cx, qm, qp, pm, pp));
        ++j;
      }
      if (a->depth) a->depth[c] = j;
      T eta = (T)1 / (T)(m + t0c);
      h_bar = ((T)1 - eta) * h_bar + eta * (delta - alpha / (T)n_alpha);
      if (m <= a->n_discard) {
        const T mf = (T)m;
        eps = MEXP(cx.form, mu - SQRT(mf) / gamma * h_bar);
        /* m.powf(-kappa): form 0 (the kernels) exp(-kappa ln m), form 1 the
         * C library's pow, as the reference */
        eta = cx.form == 1 ? RPOW(mf, -kappa) : EXP(-kappa * LOG(mf));
        eps_bar = MEXP(cx.form, ((T)1 - eta) * MLOG(cx.form, eps_bar) + eta * MLOG(cx.form, eps));
        if (mmode && F(should_collect)(a->mcfg, m, a->n_discard)) {  /* :897-921 */
          F(running_update)(&run, q, D, mmode == 2);
          if (F(note_window_end)(a->mcfg, sched, m, a->n_discard)) {
            F(mass) M2 = cx.M;
            if (mmode == 2) M2.inv = (T*)a->ms->minv + c * D * D;
            if (F(maybe_update)(a->mcfg, &run, D, &M2, dinv, dsq)) {
              if (M2.kind == 1) M2.inv = dinv;
              cx.M = M2;
              for (int i = 0; i < D; ++i) zb[i] = NORMAL(a->seed, cid, st, TAG_NUTS_PROBE, (uint32_t)i);
              T* probe = malloc(vb);
              F(momentum_from)(&cx.M, zb, probe, D);
              eps = F(find_eps)(&cx, q, probe);
              free(probe);
              mu = MLOG(cx.form, (T)10 * eps);
              eps_bar = eps;
              h_bar = (T)0;
              F(running_reset)(&run, D, mmode == 2);
            }
          }
        }
      } else {
        eps = eps_bar;
      }
      const int64_t row = step_mode ? -1 : (s + 1) - row_shift;
      if (row >= 0 && row < a->n_collect && a->samples) memcpy(&a->samples[(row * a->C + c) * D], q, vb);
    }
    memcpy(&a->q[c * D], q, vb);
    a->eps[c] = eps; a->eps_bar[c] = eps_bar; a->h_bar[c] = h_bar; a->mu[c] = mu;
    if (mmode) {
      a->ms->kind[c] = cx.M.kind;
      a->sched_out[2 * c] = sched[0];
      a->sched_out[2 * c + 1] = sched[1];
    }
    if (a->accepts) a->accepts[c] += acc;
    if (a->n_leapfrog) a->n_leapfrog[c] += cx.nlf;
  }
  for (int k = 0; k < 32; ++k) free(cx.ws[k].qm);
  free(top.qm); free(cx.tmpv); free(cx.tmpv2);
  free(run.mean); free(run.m2d); free(run.delta); free(run.m2); free(zb);
  free(q); free(p0); free(g0); free(qm); free(pm); free(gm); free(qp); free(pp); free(gp);
  free(vm); free(wm); free(vp); free(wp);
}

/* n_leap leapfrogs of leapfrog_with_mass under a dense M^-1 from (q, p), in
 * the engine's form (0: v = M^-1 p, w = M^-1 g carried by linearity, one fma
 * product per leapfrog, kinetic 0.5 sum p v in the canonical order) or the
 * reference's (1: M^-1 of the kicked momentum per leapfrog,
 * generic_nuts.rs:1409-1417; kinetic by fresh row products, :244-253). The
 * tolerance tests tie the two (tests/test_oracle_nuts_forms.py). */
int F(or_dense_traj)(const or_target* t, int lanes, int elems, int D, const T* inv, T* q, T* p,
                     double eps, int n_leap, int form, T* vel, T* out) {
  if (D < 1 || D > 1024 || lanes * elems < D || lanes > 64 || (form != 0 && form != 1)) return 1;
  F(nctx) cx;
  memset(&cx, 0, sizeof(cx));
  cx.t = t; cx.lanes = lanes; cx.elems = elems; cx.D = D; cx.form = form;
  cx.M.kind = 2;
  cx.M.inv = (T*)inv;
  const size_t vb = sizeof(T) * (size_t)(lanes * elems > D ? lanes * elems : D);
  T *g = malloc(vb), *w = malloc(vb);
  cx.tmpv = malloc(vb);
  cx.tmpv2 = malloc(vb);
  T lp = F(logp_grad_impl)(t, lanes, elems, q, g);
  if (form == 0) {
    F(inv_mul)(&cx.M, p, vel, D, 0);
    F(inv_mul)(&cx.M, g, w, D, 0);
    for (int l = 0; l < n_leap; ++l) lp = F(leapfrog)(&cx, q, p, g, vel, w, (T)eps);
    out[1] = F(kinetic_v)(&cx, p, vel);
  } else {
    for (int l = 0; l < n_leap; ++l) lp = F(leapfrog)(&cx, q, p, g, NULL, NULL, (T)eps);
    F(inv_mul)(&cx.M, p, vel, D, 1);
    out[1] = F(kinetic)(&cx, p);
  }
  out[0] = lp;
  free(g); free(w); free(cx.tmpv); free(cx.tmpv2);
  return 0;
}

int F(or_nuts_run)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, T* eps,
                   T* eps_bar, T* h_bar, T* mu, double target_accept, int max_depth,
                   uint64_t seed, uint64_t init_step, uint32_t chain_offset, int64_t n_collect,
                   int64_t n_discard, int progress, T* samples, int64_t* accepts,
                   int64_t* n_leapfrog, int threads) {
  /* lanes > 64: a chain over lanes/64 waves (the wide NUTS layouts), sums per wave then left to right */
  if (D < 1 || D > 1024 || lanes * elems < D || lanes * elems > 1024 || (lanes > 64 && lanes % 64) ||
      max_depth < 1 || max_depth > 30)
    return 1;
  if (!progress && n_collect == 0) return 0;
  F(nuts_ctx) a = {t, lanes, elems, C, D, q, eps, eps_bar, h_bar, mu, target_accept, max_depth,
                   seed, init_step, chain_offset, n_collect, n_discard, progress, samples,
                   accepts, n_leapfrog, NULL, NULL, NULL, 0};
  parallel_chains(C, threads, F(nuts_chains), &a);
  return 0;
}

/* NUTS::step / GenericNUTSChain::step (nuts.rs:431-433, generic_nuts.rs:755-925):
 * n_steps transitions continuing a chain's state, no init_chain_state, the
 * adaptation counter m running on from m0 against the last run's n_discard;
 * transition s draws at counter step0 + s. Nothing is collected. */
int F(or_nuts_step)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, T* eps,
                    T* eps_bar, T* h_bar, T* mu, double target_accept, int max_depth,
                    uint64_t seed, uint64_t step0, uint32_t chain_offset, int64_t n_steps,
                    int64_t m0, int64_t n_discard, int64_t* accepts, int64_t* n_leapfrog,
                    int threads) {
  /* lanes > 64: a chain over lanes/64 waves (the wide NUTS layouts), sums per wave then left to right */
  if (D < 1 || D > 1024 || lanes * elems < D || lanes * elems > 1024 || (lanes > 64 && lanes % 64) ||
      max_depth < 1 || max_depth > 30)
    return 1;
  if (n_steps <= 0) return 0;
  F(nuts_ctx) a = {t, lanes, elems, C, D, q, eps, eps_bar, h_bar, mu, target_accept, max_depth,
                   seed, step0, chain_offset, n_steps, n_discard, 2, NULL,
                   accepts, n_leapfrog, NULL, NULL, NULL, m0};
  parallel_chains(C, threads, F(nuts_chains), &a);
  return 0;
}

/* or_nuts_step that also returns the tree depth of every chain's last
 * transition (depth [C]); with n_steps = 1, the transition's. */
int F(or_nuts_step_depth)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, T* eps,
                          T* eps_bar, T* h_bar, T* mu, double target_accept, int max_depth,
                          uint64_t seed, uint64_t step0, uint32_t chain_offset, int64_t n_steps,
                          int64_t m0, int64_t n_discard, int64_t* accepts, int64_t* n_leapfrog,
                          int32_t* depth, int threads) {
  if (D < 1 || D > 1024 || lanes * elems < D || lanes * elems > 1024 || (lanes > 64 && lanes % 64) ||
      max_depth < 1 || max_depth > 30)
    return 1;
  if (n_steps <= 0) return 0;
  F(nuts_ctx) a = {t, lanes, elems, C, D, q, eps, eps_bar, h_bar, mu, target_accept, max_depth,
                   seed, step0, chain_offset, n_steps, n_discard, 2, NULL,
                   accepts, n_leapfrog, NULL, NULL, NULL, m0, depth};
  parallel_chains(C, threads, F(nuts_chains), &a);
  return 0;
}

int F(or_nuts_mass_run)(const or_target* t, int lanes, int elems, int64_t C, int D, T* q, T* eps,
                        T* eps_bar, T* h_bar, T* mu, double target_accept, int max_depth,
                        uint64_t seed, uint64_t init_step, uint32_t chain_offset, int64_t n_collect,
                        int64_t n_discard, int progress, T* samples, int64_t* accepts,
                        int64_t* n_leapfrog, const or_mass_cfg* cfg, or_mass_state* ms,
                        int threads) {
  /* lanes > 64: a chain over lanes/64 waves (the wide NUTS layouts), sums per wave then left to right */
  if (D < 1 || D > 1024 || lanes * elems < D || lanes * elems > 1024 || (lanes > 64 && lanes % 64) ||
      max_depth < 1 || max_depth > 30)
    return 1;
  if (!progress && n_collect == 0) return 0;
  int64_t* so = (int64_t*)malloc(sizeof(int64_t) * 2 * (C > 0 ? C : 1));
  F(nuts_ctx) a = {t, lanes, elems, C, D, q, eps, eps_bar, h_bar, mu, target_accept, max_depth,
                   seed, init_step, chain_offset, n_collect, n_discard, progress, samples,
                   accepts, n_leapfrog, cfg, ms, so, 0};
  parallel_chains(C, threads, F(nuts_chains), &a);
  if (cfg && cfg->mode && C > 0) {  /* the schedule is the same for every chain */
    ms->sched[0] = so[0];
    ms->sched[1] = so[1];
  }
  free(so);
  return 0;
}

#undef F
#undef MEXP
#undef MLOG
