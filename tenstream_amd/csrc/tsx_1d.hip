// tsx_1d.hip -- the 1-D column solvers of solve_pprts (src/pprts.F90:2560-2567, 2627-2638): twostream and schwarz
// (src/pprts_1D_solvers.F90:55-252, 418-582) and the scatter of the two-stream fluxes into the 3-D solver's solution storage
// (-initial_guess_from_2str).  fp64 throughout.
//
// Work split.  The optical properties arrive in the reference layout (level fastest), a column solver wants one lane per column
// with consecutive lanes on consecutive columns.  So a cell-parallel kernel (tsx_k_1d_prep) first evaluates everything that is
// local to a layer -- eddington_coeff_ec, the emitted sources emis * B_eff, or for schwarz dtau and planck -- into cell-indexed
// planes P[q][k * ncol + col] (column fastest); the column kernels then walk the layers twice from those planes (down, up) with
// every load and store of a wave contiguous.  The per-level temporaries of the recurrences (3 planes for the adding form, 2 for
// the block elimination) live in planes of the same scratch, which the solver owns and only ever grows (pool memory: no driver
// call after the first use).  No per-lane arrays: nothing spills to scratch memory (profiles/r07/onedim_resource_usage.txt).
//
// The fluxes are kept on the ATMOSPHERE's levels (Nz + c levels with collapse c), planes S / Edn / Eup [lev * ncol + col] in
// W/m2, followed by the absorption on the solver's Nz layers [k * ncol + col] in W/m3: that block is "the 1-D solution" which
// tsx_pprts_get_result transposes out and tsx_pprts_select_solution parks.
#include "tsx_host.hpp"
#include "tsx_kernels_1d.hpp"

namespace {
constexpr int OD_PLANES = 10;  // a11 a12 a13 a23 a33 su sd + 3 temporaries
constexpr double OD_PI = 3.14159265358979323846;

// layer-local part.  kind 0: twostream (planes 0..4 = a11 a12 a13 a23 a33; with planck 5 = emis * B_eff towards the top,
// 6 = towards the bottom, src/twostream.F90:108-115); kind 1: schwarz (plane 0 = dtau = dz * kabs, then planck on the nza + 1
// levels as a plane of its own).  kabs / ksca / g / dz: [k + nza * col], planck: [l + (nza + 1) * col].
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_1d_prep(int ncol, int nza, int kind, const double *__restrict__ kabs,
                                                           const double *__restrict__ ksca, const double *__restrict__ gas,
                                                           const double *__restrict__ dz, const double *__restrict__ planck,
                                                           double mu0, double *__restrict__ P) {
  const size_t nca = (size_t)nza * ncol;
  const double eps = 2.220446049250313e-16;
  const long long total = kind == 1 ? (long long)(nza + 1) * ncol : (long long)nca;
  for (long long c = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; c < total; c += (long long)gridDim.x * TSX_BLOCK) {
    const int col = (int)(c % ncol), k = (int)(c / ncol);
    if (kind == 1) {
      P[nca + c] = planck[(size_t)k + (size_t)(nza + 1) * col];
      if (k < nza) {
        const size_t r = (size_t)k + (size_t)nza * col;
        P[c] = dz[r] * kabs[r];
      }
      continue;
    }
    const size_t r = (size_t)k + (size_t)nza * col;
    const double kext = kabs[r] + ksca[r];  // src/pprts_1D_solvers.F90:134-137
    const double dtau = dz[r] * kext, w0 = ksca[r] / fmax(kext, eps);
    double tt, rr, rdir, sdir, tdir;
    tsx_eddington_ec(dtau, w0, gas[r], mu0, tt, rr, rdir, sdir, tdir);
    P[c] = tt;
    P[nca + c] = rr;
    P[2 * nca + c] = rdir;
    P[3 * nca + c] = sdir;
    P[4 * nca + c] = tdir;
    if (planck) {
      const size_t l = (size_t)k + (size_t)(nza + 1) * col;
      const double p0 = planck[l], p1 = planck[l + 1];
      const double emis = fmax(0.0, fmin(1.0, 1.0 - tt - rr)) * OD_PI;
      P[5 * nca + c] = emis * tsx_B_eff(p1, p0, dtau);
      P[6 * nca + c] = emis * tsx_B_eff(p0, p1, dtau);
    }
  }
}

// adding_delta_eddington_twostream (src/twostream.F90:335-390), statement for statement, one lane per column.  R / Sdir / Tdir of
// the layers go to planes 7..9 on the way down and are read back on the way up.  (T(k) of :368 feeds nothing and is left out.)
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_twostream_adding(int ncol, int ke, double S0, const double *__restrict__ albedo,
                                                                    double *__restrict__ P, double *__restrict__ Edir,
                                                                    double *__restrict__ Edn, double *__restrict__ Eup) {
  const int col = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (col >= ncol) return;
  const size_t n = (size_t)ncol, nca = (size_t)ke * n;
  const double *a11 = P, *a12 = P + nca, *a13 = P + 2 * nca, *a23 = P + 3 * nca, *a33 = P + 4 * nca;
  double *Rp = P + 7 * nca, *Sp = P + 8 * nca, *Tp = P + 9 * nca;
  const double Ag = albedo[col];
  Edir[col] = S0;
  Edn[col] = 0.0;
  double R = a12[col], Tdir = a33[col], Sdir = a23[col];
  Rp[col] = R, Sp[col] = Sdir, Tp[col] = Tdir;
  Edir[n + col] = Tdir * S0;
  for (int k = 0; k + 1 < ke; ++k) {
    const size_t q = (size_t)(k + 1) * n + col;
    const double b11 = a11[q], b12 = a12[q], b13 = a13[q], b23 = a23[q], b33 = a33[q];
    const double Rn = b12 + (R * b11 * b11) / (1.0 - R * b12);
    const double Sn = (b11 * Sdir + Tdir * b13 * R * b11) / (1.0 - R * b12) + Tdir * b23;
    Tdir = Tdir * b33;
    R = Rn, Sdir = Sn;
    Rp[q] = R, Sp[q] = Sdir, Tp[q] = Tdir;
    Edir[q + n] = Tdir * S0;
  }
  double edn = (Sdir + Tdir * R * Ag) / (1.0 - R * Ag) * S0;
  double eup = Ag * (edn + Tdir * S0);
  Edn[(size_t)ke * n + col] = edn;
  Eup[(size_t)ke * n + col] = eup;
  for (int t = ke - 1; t >= 1; --t) {
    const size_t q = (size_t)t * n + col;
    const double b11 = a11[q], b12 = a12[q], b13 = a13[q], Rm = Rp[q - n], Sm = Sp[q - n], ed = Edir[q];
    const double den = 1.0 - Rm * b12;
    edn = (Rm * b11 * eup + S0 * Sm + ed * b13 * Rm) / den;
    eup = (b11 * eup + S0 * Sm * b12 + ed * b13) / den;
    Edn[q] = edn;
    Eup[q] = eup;
  }
  Eup[col] = a11[col] * eup + a13[col] * S0;
}

// delta_eddington_twostream with planck (src/twostream.F90:50-184): the 2 (ke + 1) pentadiagonal system
//     Eup(k) - T_k Eup(k+1) - R_k Edn(k) = su_k,   Edn(k+1) - T_k Edn(k) - R_k Eup(k+1) = sd_k,   Edn(1) = 0,
//     Eup(ke1) - albedo Edn(ke1) = S(ke1) albedo + Bsrfc (1 - albedo) pi
// solved per lane by eliminating its 2 x 2 blocks from the top: with Edn(k) = Rc_k Eup(k) + Dc_k (Rc_1 = Dc_1 = 0),
//     Rc_{k+1} = R + T Rc T / (1 - R Rc),   Dc_{k+1} = T Dc + sd + T Rc (R Dc + su) / (1 - R Rc),
// the ground row gives Eup(ke1), and back-substitution Eup(k) = (T Eup(k+1) + R Dc_k + su) / (1 - R Rc_k).  Rc / Dc of the levels
// go to planes 7, 8.  The same system as DGBSV's, without pivoting: 1 - R Rc >= 1 - R > 0 for any physical layer.
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_twostream_planck(int ncol, int ke, double S0, double mu0, const double *__restrict__ albedo,
                                                                    const double *__restrict__ bsrfc, double *__restrict__ P,
                                                                    const double *__restrict__ planck, double *__restrict__ S,
                                                                    double *__restrict__ Edn, double *__restrict__ Eup) {
  const int col = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (col >= ncol) return;
  const size_t n = (size_t)ncol, nca = (size_t)ke * n;
  const double *a11 = P, *a12 = P + nca, *a13 = P + 2 * nca, *a23 = P + 3 * nca, *a33 = P + 4 * nca, *su = P + 5 * nca, *sd = P + 6 * nca;
  double *Rp = P + 7 * nca, *Dp = P + 8 * nca;
  const double Ag = albedo[col];
  double Sk = mu0 > 0.0 ? S0 : 0.0, Rc = 0.0, Dc = 0.0;
  S[col] = Sk;
  for (int k = 0; k < ke; ++k) {
    const size_t q = (size_t)k * n + col;
    const double T = a11[q], R = a12[q];
    double bu = Sk * a13[q], bd = Sk * a23[q];
    bu = bu + su[q];
    bd = bd + sd[q];
    Rp[q] = Rc, Dp[q] = Dc;
    const double den = 1.0 - R * Rc;
    const double Dn = T * Dc + bd + T * Rc * (R * Dc + bu) / den;
    Rc = R + T * Rc * T / den;
    Dc = Dn;
    Sk = mu0 > 0.0 ? Sk * a33[q] : 0.0;
    S[q + n] = Sk;
  }
  const double Bs = bsrfc ? bsrfc[col] : planck[(size_t)ke + (size_t)(ke + 1) * col];
  double bsr = Sk * Ag;
  bsr = bsr + Bs * (1.0 - Ag) * OD_PI;
  double eup = (Ag * Dc + bsr) / (1.0 - Ag * Rc);
  Eup[(size_t)ke * n + col] = eup;
  Edn[(size_t)ke * n + col] = Rc * eup + Dc;
  for (int k = ke - 1; k >= 0; --k) {
    const size_t q = (size_t)k * n + col;
    const double T = a11[q], R = a12[q], rc = Rp[q], dc = Dp[q];
    double bu = S[q] * a13[q];
    bu = bu + su[q];
    eup = (T * eup + R * dc + bu) / (1.0 - R * rc);
    Eup[q] = eup;
    Edn[q] = rc * eup + dc;
  }
}

struct OdQuad {
  double mu[16], w[16];
};

// schwarzschild, use_legendre branch (src/schwarzschild.F90:81-135): per node a march down from Ldn = 0 and, from the ground value
// Lup = Bsrfc (1 - albedo) + albedo Edn(ke1) 2, a march up.  The nodes are the outer loop as in the reference, so a level's sum
// takes its terms in the reference's order; it is kept in the output plane between nodes, and the last node's pass applies the
// final * 2 * pi.  P: plane 0 = dtau, then planck on the levels (tsx_k_1d_prep kind 1).
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_schwarz(int ncol, int ke, int nmu, OdQuad Q, const double *__restrict__ albedo,
                                                           const double *__restrict__ bsrfc, const double *__restrict__ P,
                                                           double *__restrict__ Edn, double *__restrict__ Eup) {
  const int col = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (col >= ncol) return;
  const size_t n = (size_t)ncol;
  const double *dtau = P, *pl = P + (size_t)ke * n;
  const double Ag = albedo[col];
  const double Bs = bsrfc ? bsrfc[col] : pl[(size_t)ke * n + col];
  double edn_ke = 0.0;
  Edn[col] = 0.0;
  for (int m = 0; m < nmu; ++m) {
    const double mu = Q.mu[m], w = Q.w[m];
    const bool first = m == 0, last = m == nmu - 1;
    double L = 0.0, pn = pl[col];
    for (int k = 0; k < ke; ++k) {
      const size_t q = (size_t)k * n + col;
      const double pf = pl[q + n];
      L = tsx_schwarzschild_radiance(dtau[q] / mu, pn, pf, L);
      pn = pf;
      const double acc = first ? 0.0 : Edn[q + n];
      const double v = acc + L * mu * w;
      if (k == ke - 1) edn_ke = v;
      Edn[q + n] = last ? v * 2 * OD_PI : v;
    }
  }
  for (int m = 0; m < nmu; ++m) {
    const double mu = Q.mu[m], w = Q.w[m];
    const bool first = m == 0, last = m == nmu - 1;
    double L = Bs * (1.0 - Ag) + Ag * edn_ke * 2;
    {
      const size_t q = (size_t)ke * n + col;
      const double acc = first ? 0.0 : Eup[q];
      const double v = acc + L * mu * w;
      Eup[q] = last ? v * 2 * OD_PI : v;
    }
    double pn = pl[(size_t)ke * n + col];
    for (int k = ke - 1; k >= 0; --k) {
      const size_t q = (size_t)k * n + col;
      const double pf = pl[q];
      L = tsx_schwarzschild_radiance(dtau[q] / mu, pn, pf, L);
      pn = pf;
      const double acc = first ? 0.0 : Eup[q];
      const double v = acc + L * mu * w;
      Eup[q] = last ? v * 2 * OD_PI : v;
    }
  }
}

// xv_abso (src/pprts_1D_solvers.F90:220-233) on the solver's layers: the levels atmk(k), atmk(k) + 1 of the atmosphere, divided by
// dz(atmk(k)); S null: thermal
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_1d_abso(int ncol, int Nz, int c, const double *__restrict__ dz, const double *__restrict__ S,
                                                           const double *__restrict__ Edn, const double *__restrict__ Eup,
                                                           double *__restrict__ abso) {
  const int nza = Nz + c - 1;
  const long long total = (long long)Nz * ncol;
  for (long long e = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * TSX_BLOCK) {
    const int col = (int)(e % ncol), k = (int)(e / ncol);
    const size_t q = (size_t)(k + c - 1) * ncol + col, q1 = q + ncol;
    double a = +Edn[q] - Edn[q1] - Eup[q] + Eup[q1];
    if (S) a = a + S[q] - S[q1];
    abso[e] = a / dz[(size_t)(k + c - 1) + (size_t)nza * col];
  }
}

// the 1-D solution -> pprts_get_result's arrays (src/pprts.F90:5850-5888): solver level 0 <- atmosphere level 0, level k >= 1 <-
// atmk(0) + k (src/pprts_1D_solvers.F90:201-218), times sun%mu for a solar solution; reference layout (level fastest).  A tile of
// 32 columns x 32 levels goes through LDS: read along the columns, written along the levels (as tsx_k_get_result).
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_1d_result(int ncol, int Nz, int c, double mu, const double *__restrict__ S,
                                                             const double *__restrict__ Edn, const double *__restrict__ Eup,
                                                             const double *__restrict__ abso, double *__restrict__ redir,
                                                             double *__restrict__ redn, double *__restrict__ reup, double *__restrict__ rabso) {
  constexpr int TC = 32, TK = 32;
  __shared__ double sm[4][TK][TC + 1];
  const int L = Nz + 1;
  const int c0 = blockIdx.x * TC, k0 = blockIdx.y * TK;
  for (int e = threadIdx.x; e < TC * TK; e += TSX_BLOCK) {
    const int cc = e % TC, kk = e / TC;
    const int col = c0 + cc, k = k0 + kk;
    double dn = 0.0, up = 0.0, di = 0.0, ab = 0.0;
    if (col < ncol && k < L) {
      const size_t q = (size_t)(k == 0 ? 0 : c - 1 + k) * ncol + col;
      dn = Edn[q] * mu;
      up = Eup[q] * mu;
      if (S) di = S[q] * mu;
      if (k < Nz) ab = abso[(size_t)k * ncol + col] * mu;
    }
    sm[0][kk][cc] = dn, sm[1][kk][cc] = up, sm[2][kk][cc] = di, sm[3][kk][cc] = ab;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TC * TK; e += TSX_BLOCK) {
    const int kk = e % TK, cc = e / TK;
    const int col = c0 + cc, k = k0 + kk;
    if (col >= ncol || k >= L) continue;
    const size_t o = (size_t)k + (size_t)L * col;
    redn[o] = sm[0][kk][cc];
    reup[o] = sm[1][kk][cc];
    if (redir) redir[o] = sm[2][kk][cc];
    if (k < Nz) rabso[(size_t)k + (size_t)Nz * col] = sm[3][kk][cc];
  }
}

// -initial_guess_from_2str: twostream's S / Edn / Eup into the 3-D solver's solution storage, in W per stream.  Every top-face
// diffuse dof of a level gets Edn or Eup by is_inward times difftop%area_divider / streams (= 1 / (ntop / 2)), every top-face direct
// dof S * dirtop%area_divider / streams (= 1) (src/pprts_1D_solvers.F90:201-218); then scale_flx(lWm2 = .false.)
// (src/pprts.F90:3901-3987): diffuse top faces * dx dy, direct top faces * dx dy / dirtop%area_divider.  The side dofs hold what the
// reference's `solution%ediff = zero` (:108) left there, and zero times a face area is zero: the caller clears x and E before.
// x: internal layout (tsx_internal.hpp), E: S planes over the Nz + 1 levels (null: thermal).
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_1d_scatter(int ncol, int Nz, int c, int D, int ntop, int dtop, double dxdy,
                                                              const double *__restrict__ S, const double *__restrict__ Edn,
                                                              const double *__restrict__ Eup, double *__restrict__ x, double *__restrict__ E) {
  const long long Nc = (long long)Nz * ncol, Ncl = (long long)(Nz + 1) * ncol;
  const double fac = 1.0 / (double)(ntop / 2);
  double *__restrict__ xt = x + (size_t)D * Nc;
  for (long long e = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; e < Ncl; e += (long long)gridDim.x * TSX_BLOCK) {
    const int col = (int)(e % ncol), k = (int)(e / ncol);
    const size_t q = (size_t)(k == 0 ? 0 : c - 1 + k) * ncol + col;
    const double dn = Edn[q] * fac * dxdy, up = Eup[q] * fac * dxdy;
    for (int d = 0; d < ntop; ++d) {
      if (tsx_inward(d)) {
        if (k >= 1) x[(size_t)d * Nc + (size_t)(k - 1) * ncol + col] = dn;
        else xt[(size_t)d * ncol + col] = dn;
      } else {
        if (k < Nz) x[(size_t)d * Nc + (size_t)k * ncol + col] = up;
        else xt[(size_t)d * ncol + col] = up;
      }
    }
    if (E) {
      const double di = S[q] * 1.0 * (dxdy / (double)dtop);
      for (int s = 0; s < dtop; ++s) E[(size_t)s * Ncl + e] = di;
    }
  }
}
}  // namespace

// Gauss-Legendre nodes and weights on (0, 1), ascending: what dgauss (src/schwarzschild.F90:173-290) returns, restated: Newton on
// the three-term recurrence of P_n from the Chebyshev-like first guess, weights 2 / ((1 - x^2) P_n'(x)^2), mapped from (-1, 1)
void tsx_gauss_legendre_01(int n, double *mu, double *w) {
  for (int i = 0; i < n; ++i) {
    double x = cos(OD_PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = x;
      for (int k = 2; k <= n; ++k) {
        const double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
        p0 = p1, p1 = p2;
      }
      if (n == 0) p1 = 1.0;
      dp = n * (x * p1 - p0) / (x * x - 1.0);
      const double dx = p1 / dp;
      x -= dx;
      if (fabs(dx) < 1e-16) break;
    }
    {  // P_n' at the converged root
      double p0 = 1.0, p1 = x;
      for (int k = 2; k <= n; ++k) {
        const double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
        p0 = p1, p1 = p2;
      }
      dp = n * (x * p1 - p0) / (x * x - 1.0);
    }
    const int o = n - 1 - i;  // the roots come out descending
    mu[o] = 0.5 * (x + 1.0);
    w[o] = 0.5 * (2.0 / ((1.0 - x * x) * dp * dp));
  }
}

// the atmosphere's fields as the handle holds them: with collapse the atmosphere-shaped scratch of set_optical_properties
// (collapse_scratch, tsx_pipeline.hip: kabs, ksca, g, dz, planck at the head of ca_buf), else the solver's own copies
static int od_atm_fields(tsx_solver *s, const double **kabs, const double **ksca, const double **g, const double **dz, const double **planck) {
  const size_t ncol = (size_t)s->geo.ncol;
  if (s->collapse > 1) {
    const size_t nca = (size_t)(s->geo.Nz + s->collapse - 1) * ncol;
    if (!s->ca_buf) {
      tsx_set_error("1-D solver: no optical properties (tsx_pprts_set_optical_properties)");
      return TSX_ERR_STATE;
    }
    *kabs = s->ca_buf, *ksca = s->ca_buf + nca, *g = s->ca_buf + 2 * nca, *dz = s->ca_buf + 3 * nca;
    *planck = s->ca_have_B ? s->ca_buf + 4 * nca : nullptr;
  } else {
    *kabs = s->d_kabs, *ksca = s->d_ksca, *g = s->d_g, *dz = s->d_dz, *planck = s->planck;
  }
  if (!*kabs || !*ksca || !*g || !*dz) {
    tsx_set_error("1-D solver: no optical properties (tsx_pprts_set_optical_properties)");
    return TSX_ERR_STATE;
  }
  return TSX_OK;
}

size_t tsx_1d_solution_doubles(const tsx_solver *s) {
  const size_t ncol = (size_t)s->geo.ncol, nza = (size_t)(s->geo.Nz + (s->collapse > 1 ? s->collapse - 1 : 0));
  return 3 * (nza + 1) * ncol + (size_t)s->geo.Nz * ncol;
}

// twostream (schwarz = 0) or schwarz (1) for every column of the handle, into s->od_flux.  Exchanges nothing, reduces nothing.
int tsx_1d_run(tsx_solver *s, double edirTOA, int lsolar, int schwarz) {
  const TsxGeo &g = s->geo;
  const int c = s->collapse > 1 ? s->collapse : 1, nza = g.Nz + c - 1, ncol = g.ncol;
  const size_t n = (size_t)ncol, nl = (size_t)(nza + 1) * n;
  const double *kabs, *ksca, *gas, *dz, *planck;
  int rc = od_atm_fields(s, &kabs, &ksca, &gas, &dz, &planck);
  if (rc) return rc;
  if (!s->have_albedo) {
    tsx_set_error("1-D solver: no surface albedo (tsx_pprts_set_optical_properties)");
    return TSX_ERR_STATE;
  }
  if (schwarz && lsolar) {  // src/pprts_1D_solvers.F90:470
    tsx_set_error("schwarzschild solver does not solve solar radiation (src/pprts_1D_solvers.F90:470)");
    return TSX_ERR_ARG;
  }
  if (!lsolar && !planck) {  // (:471; a thermal twostream without planck has no source at all)
    tsx_set_error("1-D solver: a thermal solve needs planck in tsx_pprts_set_optical_properties");
    return TSX_ERR_STATE;
  }
  if (lsolar && !s->have_sun) {
    tsx_set_error("1-D solver: call tsx_pprts_set_angles first");
    return TSX_ERR_STATE;
  }
  const size_t need = (size_t)OD_PLANES * nza * n, nsol = tsx_1d_solution_doubles(s);
  if (need > s->od_cap) {  // grow-only
    if (s->od_buf) HIPCHK(tsx_dev_free(s->od_buf));
    s->od_buf = nullptr, s->od_cap = 0;
    HIPCHK(tsx_dev_malloc(&s->od_buf, sizeof(double) * need));
    s->od_cap = need;
  }
  if (nsol > s->od_flux_cap) {
    if (s->od_flux) HIPCHK(tsx_dev_free(s->od_flux));
    s->od_flux = nullptr, s->od_flux_cap = 0;
    HIPCHK(tsx_dev_malloc(&s->od_flux, sizeof(double) * nsol));
    s->od_flux_cap = nsol;
  }
  double *P = s->od_buf, *S = s->od_flux, *Edn = S + nl, *Eup = Edn + nl, *abso = Eup + nl;
  const double mu0 = lsolar ? s->sun_mu : 0.0, inc = lsolar ? edirTOA : 0.0;  // src/pprts_1D_solvers.F90:115-122
  const unsigned ncb = (unsigned)((ncol + TSX_BLOCK - 1) / TSX_BLOCK);
  if (schwarz) {
    OdQuad Q;
    for (int q = 0; q < 16; ++q) Q.mu[q] = 1.0, Q.w[q] = 0.0;
    tsx_gauss_legendre_01(s->od_nmu, Q.mu, Q.w);
    hipLaunchKernelGGL(tsx_k_1d_prep, dim3(grid_for((long long)nl)), dim3(TSX_BLOCK), 0, s->stream, ncol, nza, 1, kabs, ksca, gas, dz, planck,
                       0.0, P);
    HIPCHK(hipMemsetAsync(S, 0, sizeof(double) * nl, s->stream));
    hipLaunchKernelGGL(tsx_k_schwarz, dim3(ncb), dim3(TSX_BLOCK), 0, s->stream, ncol, nza, s->od_nmu, Q, s->albedo, s->bsrfc, P, Edn, Eup);
  } else {
    hipLaunchKernelGGL(tsx_k_1d_prep, dim3(grid_for((long long)nza * ncol)), dim3(TSX_BLOCK), 0, s->stream, ncol, nza, 0, kabs, ksca, gas,
                       dz, planck, mu0, P);
    if (planck)
      hipLaunchKernelGGL(tsx_k_twostream_planck, dim3(ncb), dim3(TSX_BLOCK), 0, s->stream, ncol, nza, inc, mu0, s->albedo, s->bsrfc, P,
                         planck, S, Edn, Eup);
    else
      hipLaunchKernelGGL(tsx_k_twostream_adding, dim3(ncb), dim3(TSX_BLOCK), 0, s->stream, ncol, nza, inc, s->albedo, P, S, Edn, Eup);
  }
  hipLaunchKernelGGL(tsx_k_1d_abso, dim3(grid_for((long long)g.Nz * ncol)), dim3(TSX_BLOCK), 0, s->stream, ncol, g.Nz, c, dz,
                     lsolar ? S : (const double *)nullptr, Edn, Eup, abso);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// s->od_flux -> the result arrays (device pointers, reference layout); redir may be null
int tsx_1d_result(tsx_solver *s, int lsolar, double *redn, double *reup, double *rabso, double *redir) {
  const TsxGeo &g = s->geo;
  const int c = s->collapse > 1 ? s->collapse : 1, nza = g.Nz + c - 1;
  const size_t nl = (size_t)(nza + 1) * g.ncol;
  const double *S = s->od_flux, *Edn = S + nl, *Eup = Edn + nl, *abso = Eup + nl;
  if (redir && !lsolar) HIPCHK(hipMemsetAsync(redir, 0, sizeof(double) * (size_t)(g.Nz + 1) * g.ncol, s->stream));
  hipLaunchKernelGGL(tsx_k_1d_result, dim3((g.ncol + 31) / 32, (g.Nz + 1 + 31) / 32), dim3(TSX_BLOCK), 0, s->stream, g.ncol, g.Nz, c,
                     lsolar ? s->sun_mu : 1.0, lsolar ? S : (const double *)nullptr, Edn, Eup, abso, lsolar ? redir : (double *)nullptr,
                     redn, reup, rabso);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// s->od_flux (a twostream result) -> x (N doubles, internal layout) and, solar, E (S planes of (Nz + 1) * ncol)
int tsx_1d_scatter(tsx_solver *s, int lsolar, double dx, double dy, double *x, double *E) {
  const TsxGeo &g = s->geo;
  const int c = s->collapse > 1 ? s->collapse : 1, nza = g.Nz + c - 1;
  const size_t nl = (size_t)(nza + 1) * g.ncol, Ncl = (size_t)(g.Nz + 1) * g.ncol;
  const int dstreams = g.ntop == 2 ? 3 : 8, dtop = g.ntop == 2 ? 1 : 4;
  const double *S = s->od_flux, *Edn = S + nl, *Eup = Edn + nl;
  HIPCHK(hipMemsetAsync(x, 0, sizeof(double) * (size_t)g.N, s->stream));
  if (lsolar) HIPCHK(hipMemsetAsync(E, 0, sizeof(double) * dstreams * Ncl, s->stream));
  hipLaunchKernelGGL(tsx_k_1d_scatter, dim3(grid_for((long long)Ncl)), dim3(TSX_BLOCK), 0, s->stream, g.ncol, g.Nz, c, g.D, g.ntop, dtop,
                     dx * dy, S, Edn, Eup, x, lsolar ? E : (double *)nullptr);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}
