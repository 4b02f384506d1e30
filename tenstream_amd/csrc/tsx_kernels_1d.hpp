// tsx_kernels_1d.hpp -- the per-layer device functions of the 1-D physics, shared by the pipeline's kernels (tsx_pipeline.hpp:
// tsx_k_eddington, tsx_k_setup_b_thermal, tsx_k_collapse_adding) and the 1-D column solvers (tsx_1d.hip).  fp64 throughout.
#pragma once
#include "tsx_dev.hpp"

// eddington_coeff_ec (src/eddington.F90:173-241).  a11 = t, a12 = r, a13 = rdir, a23 = sdir, a33 = tdir.
__device__ __forceinline__ void tsx_eddington_ec(double dtau, double w0, double gg, double mu0, double &tt, double &rr, double &rdir,
                                                 double &sdir, double &tdir) {
  const double eps = 2.220446049250313e-16, tiny = 2.2250738585072014e-308;
  const double f = 0.75 * gg;
  const double g1 = 2.0 - w0 * (1.25 + f), g2 = w0 * (0.75 - f), g3 = 0.5 - mu0 * f;
  const double slant = fmax(dtau / fmax(sqrt(tiny), mu0), 0.0);
  if (slant > 1e-6) {
    const double g4 = 1.0 - g3;
    const double al1 = g1 * g4 + g2 * g3, al2 = g1 * g3 + g2 * g4;
    const double A = sqrt(fmax((g1 - g2) * (g1 + g2), 1e-12));
    double kmu = A * mu0;
    if (kmu <= 1.0 + 10.0 * eps && kmu >= 1.0 - 10.0 * eps) kmu = 1.0 - 10.0 * eps;  // approx(), helper_functions.fypp:1272
    const double kg3 = A * g3, kg4 = A * g4;
    const double e0 = exp(-slant), e = exp(-A * dtau), e2 = e * e, k2e = 2.0 * A * e;
    double beta = 1.0 / (A + g1 + (A - g1) * e2);
    rr = g2 * (1.0 - e2) * beta;
    tt = k2e * beta;
    beta = w0 * beta / (1.0 - kmu * kmu);
    sdir = beta * (k2e * (g4 + al1 * mu0) - e0 * ((1.0 + kmu) * (al1 + kg4) - (1.0 - kmu) * (al1 - kg4) * e2));
    rdir = beta * ((1.0 - kmu) * (al2 + kg3) - (1.0 + kmu) * (al2 - kg3) * e2 - k2e * (g3 - al2 * mu0) * e0);
    tdir = e0;
  } else {
    tt = 1.0 - g1 * dtau;
    rr = g2 * dtau;
    sdir = (1.0 - g3) * (w0 * dtau);
    rdir = g3 * (w0 * dtau);
    tdir = 1.0 - slant;
  }
}

// B_eff (src/schwarzschild.F90:36-67): 2-point Gauss-Legendre on (0,1)
__device__ __forceinline__ double tsx_B_eff(double B_far, double B_near, double tau) {
  const double pt[2] = {0.5 - 0.5 / 1.7320508075688772, 0.5 + 0.5 / 1.7320508075688772};
  double B = 0.0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double mu = pt[q];
    const double dtau = tau / mu;
    double bmu;
    if (dtau < 1e-3) {
      bmu = (B_far + B_near) * .5;
    } else {
      const double tm1 = expm1(-dtau);
      bmu = (-B_near + B_far * (tm1 + 1)) / (tm1) + ((B_far - B_near) * mu) / tau;
    }
    B += bmu * mu * 0.5;
  }
  return B * 2;
}

// schwarzschild_radiance (src/schwarzschild.F90:69-80)
__device__ __forceinline__ double tsx_schwarzschild_radiance(double tau, double B_near, double B_far, double L) {
  if (tau > 1e-3) {
    const double tm1 = expm1(-tau);
    return L * (tm1 + 1) + (B_far - B_near) - (B_near - (B_far - B_near) / tau) * tm1;
  }
  return (B_near + B_far) * .5 * tau + L * (1.0 - tau);
}
