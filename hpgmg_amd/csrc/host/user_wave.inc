/*
 * user_wave.inc -- hpgmg_user_wave_start / _wave_step / _get_velocity / _get_acceleration (include/hpgmg_fv.h): the wave equation
 *   alpha d2u/dt2 + sigma alpha du/dt = b div(beta grad u) + f
 * on a user problem by the implicit Newmark rule (DESIGN.md §11.12), the theta march's sibling (user_solver.inc).  With K = A0 - a alpha (the operator
 * without its a alpha term, homogeneous ghosts), T(g) the lift, q the acceleration, v the velocity and a = 1 / (beta dt^2) + sigma gamma / (beta dt):
 *   predictor   ut = u0 + dt v0 + dt^2 (1/2 - beta) q0,   vt = v0 + dt (1 - gamma) q0
 *   solve       A0 u1 = f1 + T(g1) + alpha (a ut - sigma vt)                                                                            (1)
 *   corrector   q1 = (u1 - ut) / (beta dt^2),   v1 = vt + gamma dt q1
 * and, r being the residual of (1) the solve stopped at,  K u1 = F - r - a alpha u1  exactly: the potential energy costs no stencil pass.  The fine-level
 * work besides the solve is the three hooks hpgmg_wave_predict / _correct / _init (host defaults: host/hooks_host.inc; HIP: host/plugin_wave.c).  The state
 * u (VECTOR_U), ut (uold_id), v (w_id) and q (q_id) stays on the finest level in the box layout between calls.  A part of host/driver.c's translation
 * unit, included there after user_eigs.inc.
 */

/* the unconditionally stable rules, and the shift they need; 0: refused */
static int user_wave_shift(double dt, double beta, double gamma, double sigma, double *a) {
  if (!isfinite(dt) || !(dt > 0.0) || !isfinite(sigma) || sigma < 0.0 || !isfinite(beta) || !isfinite(gamma) || !(gamma >= 0.5) || !(beta >= gamma / 2.0)) return 0;
  *a = 1.0 / (beta * (dt * dt)) + (sigma * gamma) / (beta * dt);
  return isfinite(*a) && *a > 0.0;
}
static void user_wave_energies(const hpgmg_user_solver *us, const double sums[2], hpgmg_user_wave_info *info) {
  const double h = us->s.level_h.h, half_h3 = 0.5 * (h * h * h);
  info->t = us->wave_t; info->kinetic = half_h3 * sums[0]; info->potential = half_h3 * sums[1];
}

int hpgmg_user_wave_start(hpgmg_user_solver *us, const double *u, const double *v, const double *f, const double *g, int where, double dt, double beta,
                          double gamma, double damping, hpgmg_user_wave_info *info) {
  if (!us || !u || !v || !f || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  double a, sums[2];
  if (s->a == 0.0 || !user_wave_shift(dt, beta, gamma, damping, &a)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!us->operator_ok) return HPGMG_USER_NOT_READY;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  invert_vector(L, VECTOR_TEMP, 1.0, VECTOR_ALPHA);                     /* q = (...) / alpha: alpha > 0 in every cell, by hpgmg_user_eigs' check */
  if (!isfinite(norm(L, VECTOR_TEMP))) { USER_LOUD(); return HPGMG_USER_OUT_OF_RANGE; }
  us->march = 0;
  if (!us->uold_id || !us->q_id) {       /* the first wave march: the theta march's two vectors if no start has made them, and one more */
    int next = L->numVectors;
    if (!us->uold_id) { us->uold_id = next; us->w_id = next + 1; next += 2; }
    us->q_id = next++;
    create_vectors(L, next);
  }
  int st = user_pack_status(hpgmg_dense_pack(L, VECTOR_U, u, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) st = user_pack_status(hpgmg_dense_pack(L, us->w_id, v, where, HPGMG_DENSE_CELL, HPGMG_DENSE_CHECK_FINITE));
  if (st == HPGMG_USER_OK) st = user_march_rhs(us, f, g, where);
  if (st == HPGMG_USER_OK && a != s->a) st = hpgmg_user_set_shift(us, a);      /* after the packs: a refused array leaves the operator as it was */
  if (st == HPGMG_USER_OK) {           /* q0 = (r + a alpha u) / alpha - sigma v with r = F - A0 u: start's route to f - L(u; g) */
    residual(L, VECTOR_TEMP, VECTOR_U, VECTOR_F, s->a, s->b);
    if (hpgmg_wave_init(L, us->q_id, VECTOR_TEMP, VECTOR_U, us->w_id, VECTOR_F, s->a, damping, sums) < 0) st = HPGMG_USER_BAD_ARGUMENT;
  }
  if (st == HPGMG_USER_OK) {
    us->dt = dt; us->wave_beta = beta; us->wave_gamma = gamma; us->wave_sigma = damping; us->wave_t = 0.0;
    us->march = 2;
    if (info) {                          /* no solve has run: vcycles = 0, converged = 0; the residual is that of the start's equation A0 u = F */
      info->norm_of_residual = norm(L, VECTOR_TEMP); info->norm_of_f = norm(L, VECTOR_F); info->mean_shift = 0.0;
      info->vcycles = 0; info->converged = 0;
      user_wave_energies(us, sums, info);
    }
  }
  USER_LOUD();
  return st;
}

int hpgmg_user_wave_step(hpgmg_user_solver *us, const double *f, const double *g, int where, double dt, double rtol, hpgmg_user_wave_info *info) {
  if (!us || !f || !(rtol > 0.0) || (where != HPGMG_WHERE_HOST && where != HPGMG_WHERE_PLUGIN)) return HPGMG_USER_BAD_ARGUMENT;
  hpgmg_solver *s = &us->s;
  level_type *L = &s->level_h;
  double a, sums[2];
  if (us->march != 2 || !us->operator_ok) return HPGMG_USER_NOT_READY;      /* no march, or a theta march */
  if (!(dt > 0.0)) dt = us->dt;          /* <= 0: as before */
  const double beta = us->wave_beta, gamma = us->wave_gamma, sigma = us->wave_sigma;
  if (!user_wave_shift(dt, beta, gamma, sigma, &a)) return HPGMG_USER_BAD_ARGUMENT;
  if (g && us->bc != BC_DIRICHLET) return HPGMG_USER_UNSUPPORTED;
  if (!user_config_ok()) return HPGMG_USER_CONFLICT;
  USER_QUIET(us);
  const int st = user_march_rhs(us, f, g, where);      /* F = f + T(g), g_l and phi_l: a refusal (f or g not finite) ends here, u, v, q and the march intact */
  if (st != HPGMG_USER_OK) { USER_LOUD(); return st; }
  if (a != s->a) {                       /* u, v and q do not depend on a: a new dt is a set_shift and nothing else */
    const int e = hpgmg_user_set_shift(us, a);
    if (e != HPGMG_USER_OK) { USER_LOUD(); return e; }
  }
  us->dt = dt;
  const int v0 = L->vcycles_from_this_level;
  const double cu = (dt * dt) * (0.5 - beta), cv = dt * (1.0 - gamma), cq = 1.0 / (beta * (dt * dt)), cg = gamma * dt;
  if (hpgmg_wave_predict(L, VECTOR_U, us->uold_id, us->w_id, VECTOR_F, us->q_id, dt, cu, cv, s->a, sigma) < 0) { USER_LOUD(); return HPGMG_USER_BAD_ARGUMENT; }
  us->rhs_ok = 0;                        /* VECTOR_F is no longer the caller's f + T(g): a solve needs its own set_rhs */
  /* hpgmg_user_step's warm start, from the predictor: u = ut + e with A e = F - A ut */
  residual(L, us->x_id, VECTOR_U, VECTOR_F, s->a, s->b);
  const double norm_of_F = norm(L, VECTOR_F), norm_of_r0 = norm(L, us->x_id);
  if (norm_of_r0 > 0.0) {
    MGSolve(&s->mg, 0, VECTOR_U, us->x_id, s->a, s->b, rtol * norm_of_F / norm_of_r0);
    add_vectors(L, VECTOR_U, 1.0, VECTOR_U, 1.0, us->uold_id);
  }
  residual(L, VECTOR_TEMP, VECTOR_U, VECTOR_F, s->a, s->b);
  const double r = norm(L, VECTOR_TEMP);
  hpgmg_wave_correct(L, us->q_id, us->w_id, VECTOR_U, us->uold_id, VECTOR_F, VECTOR_TEMP, s->a, cq, cg, sums);
  us->wave_t += dt;
  USER_LOUD();
  if (info) {
    info->norm_of_residual = r; info->norm_of_f = norm_of_F; info->mean_shift = 0.0;
    info->vcycles = L->vcycles_from_this_level - v0;
    info->converged = (r == 0.0) || (r < rtol * norm_of_F);
    user_wave_energies(us, sums, info);
  }
  return HPGMG_USER_OK;
}

static int user_wave_get(hpgmg_user_solver *us, int which, double *out, int where) {      /* which: 0 the velocity, 1 the acceleration */
  if (!us || !out) return HPGMG_USER_BAD_ARGUMENT;
  if (us->march != 2) return HPGMG_USER_NOT_READY;
  USER_QUIET(us);
  const int st = hpgmg_dense_unpack(&us->s.level_h, which ? us->q_id : us->w_id, out, where);
  USER_LOUD();
  return st < 0 ? HPGMG_USER_BAD_ARGUMENT : HPGMG_USER_OK;
}
int hpgmg_user_get_velocity(hpgmg_user_solver *us, double *out, int where) { return user_wave_get(us, 0, out, where); }
int hpgmg_user_get_acceleration(hpgmg_user_solver *us, double *out, int where) { return user_wave_get(us, 1, out, where); }
