// tsx_seam_api.inc -- the seam-level entries beside tsx_diff_* (included at the end of tsx_api.hip, after the pipeline):
//   * the direct seam of `pprts()` (src/pprts.F90:2698-2755): set_dir_coeff (:4493-4630) + explicit_edir
//     (src/pprts_explicit.F90:60-459) -> tsx_dir_set_coeffs / tsx_dir_solve, fed with solver%dir2dir / dir2diff in the
//     reference's own layout instead of optical properties + LUTs;
//   * setup_b (src/pprts.F90:4641-4987) on its own -> tsx_setup_b_solar / tsx_setup_b_thermal;
//   * every vector of the seam in the caller's real kind: ireals is real32 or real64 by build (src/data_parameters.F90) ->
//     tsx_diff_apply_r / tsx_diff_solve_r and the vec_kind argument of the entries above.  real32 arrays are widened on the
//     device (no host conversion); the arithmetic is what the real64 entries run.
// The kernels are the pipeline's (tsx_pipeline.hpp); only the way the coefficients arrive differs.

// reference layout (v fastest, then level, i, j) <-> planes [v][(k * ym + j) * xm + i]
// l1d != null (coefficient blocks): the cells of 1-D layers are never assigned by the reference -- alloc_coeff_dir2dir fills
// `if (.not. atm%l1d(atmk(atm, k)))` only (src/pprts.F90:3131), so solver%dir2dir / dir2diff hold uninitialised memory there (NaN,
// or values real32 cannot hold): they are not tested and come out as zero, like tsx_k_lut_diff2diff_ent writes them
template <typename T, typename PT>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_ref_to_planes(int nv, int nlev, int xm, int ym, const T *__restrict__ ref,
                                                                 PT *__restrict__ p, int *__restrict__ lossy,
                                                                 const uint8_t *__restrict__ l1d = nullptr) {
  const long long ncl = (long long)nlev * xm * ym, total = ncl * nv;
  int bad = 0;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * TSX_BLOCK) {
    const long long c = q % ncl;
    const int v = (int)(q / ncl);
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    if (l1d && l1d[k]) {
      p[q] = (PT)0;
      continue;
    }
    const T val = ref[(size_t)v + (size_t)nv * ((size_t)k + (size_t)nlev * ((size_t)i + (size_t)xm * j))];
    const PT o = (PT)val;
    if ((T)o != val) bad = 1;  // (NaN counts as lossy too)
    p[q] = o;
  }
  if (lossy && bad) atomicOr(lossy, 1);
}

// ---- arrays of the caller's real kind -------------------------------------------------------------------------------
// in: a device pointer to the array widened to real64 (the caller's own pointer when it is real64 on the device already)
struct TsxSeamIn {
  TsxDevTmp raw, dbl;
  const double *p = nullptr;
};
static int seam_in(tsx_solver *s, const void *src, size_t n, int kind, int where, TsxSeamIn *o) {
  ARGCHK(kind == 4 || kind == 8, "vec_kind must be 4 (real32) or 8 (real64)");
  const void *dev = src;
  if (where == TSX_HOST) {
    HIPCHK(o->raw.alloc(n * (size_t)kind));
    HIPCHK(hipMemcpyAsync(o->raw.p, src, n * (size_t)kind, hipMemcpyHostToDevice, s->stream));
    dev = o->raw.p;
  }
  if (kind == 8) {
    o->p = (const double *)dev;
    return TSX_OK;
  }
  HIPCHK(o->dbl.alloc(n * sizeof(double)));
  hipLaunchKernelGGL(tsx_k_to_f64, dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, (long long)n, (const float *)dev,
                     o->dbl.as<double>());
  HIPCHK(hipGetLastError());
  o->p = o->dbl.as<double>();
  return TSX_OK;
}
// out: a device real64 buffer the producer writes (the caller's own array when it is real64 on the device), delivered by
// seam_out_finish in the caller's kind and place
struct TsxSeamOut {
  TsxDevTmp dbl, raw;
  double *p = nullptr;
  void *dst = nullptr;
  size_t n = 0;
  int kind = 8, where = TSX_DEVICE;
};
static int seam_out_begin(tsx_solver *s, void *dst, size_t n, int kind, int where, TsxSeamOut *o) {
  (void)s;
  ARGCHK(kind == 4 || kind == 8, "vec_kind must be 4 (real32) or 8 (real64)");
  o->dst = dst;
  o->n = n;
  o->kind = kind;
  o->where = where;
  if (kind == 8 && where == TSX_DEVICE) {
    o->p = (double *)dst;
    return TSX_OK;
  }
  HIPCHK(o->dbl.alloc(n * sizeof(double)));
  o->p = o->dbl.as<double>();
  return TSX_OK;
}
static int seam_out_finish(tsx_solver *s, TsxSeamOut *o) {
  if (o->kind == 8 && o->where == TSX_DEVICE) return TSX_OK;
  const void *from = o->p;
  if (o->kind == 4) {
    float *f = (float *)o->dst;
    if (o->where == TSX_HOST) {
      HIPCHK(o->raw.alloc(o->n * sizeof(float)));
      f = o->raw.as<float>();
    }
    hipLaunchKernelGGL(tsx_k_to_f32, dim3(grid_for((long long)o->n)), dim3(TSX_BLOCK), 0, s->stream, (long long)o->n, o->p, f);
    HIPCHK(hipGetLastError());
    from = f;
  }
  if (o->where == TSX_HOST)
    HIPCHK(hipMemcpyAsync(o->dst, from, o->n * (size_t)o->kind, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}

// ---- the diffuse seam in the caller's real kind ------------------------------------------------------------------------
extern "C" int tsx_diff_apply_r(tsx_solver *s, const void *x, void *y, int vec_kind, int where) {
  ARGCHK(s && x && y, "tsx_diff_apply_r: null argument");
  if (vec_kind == 8) return tsx_diff_apply(s, (const double *)x, (double *)y, where);
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)s->geo.N;
  TsxSeamIn xi;
  TsxSeamOut yo;
  int rc;
  if ((rc = seam_in(s, x, n, vec_kind, where, &xi))) return rc;
  if ((rc = seam_out_begin(s, y, n, vec_kind, where, &yo))) return rc;
  if ((rc = tsx_diff_apply(s, xi.p, yo.p, TSX_DEVICE))) return rc;
  return seam_out_finish(s, &yo);
}

extern "C" int tsx_diff_solve_r(tsx_solver *s, const void *b, void *x, int vec_kind, int where, const tsx_ksp_opts *opts,
                                tsx_ksp_result *res) {
  ARGCHK(s && b && x, "tsx_diff_solve_r: null argument");
  if (vec_kind == 8) return tsx_diff_solve(s, (const double *)b, (double *)x, where, opts, res);
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)s->geo.N;
  TsxSeamIn bi, xi;
  TsxSeamOut xo;
  int rc;
  if ((rc = seam_in(s, b, n, vec_kind, where, &bi))) return rc;
  if ((rc = seam_out_begin(s, x, n, vec_kind, where, &xo))) return rc;  // real32: always a device real64 buffer
  if (!(opts && opts->initial_guess_zero)) {                            // the guess, widened into that buffer
    if ((rc = seam_in(s, x, n, vec_kind, where, &xi))) return rc;
    HIPCHK(hipMemcpyAsync(xo.p, xi.p, n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  }
  if ((rc = tsx_diff_solve(s, bi.p, xo.p, TSX_DEVICE, opts, res))) return rc;
  return seam_out_finish(s, &xo);
}

// ---- direct seam ------------------------------------------------------------------------------------------------------
static int seam_cellfield(tsx_solver *s, double **dst, const double *src, int where) { return keep_cellfield(s, dst, src, where); }

template <typename T>
static int seam_import_coeff(tsx_solver *s, const void *ref, int nv, float *planes, int where, const char *what) {
  const TsxGeo &g = s->geo;
  const size_t n = (size_t)nv * g.Nc;
  TsxDevTmp raw;
  const T *dev = (const T *)ref;
  if (where == TSX_HOST) {
    HIPCHK(raw.alloc(n * sizeof(T)));
    HIPCHK(hipMemcpyAsync(raw.p, ref, n * sizeof(T), hipMemcpyHostToDevice, s->stream));
    dev = raw.as<T>();
  }
  int *flag = &s->scal->aux_flag;
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s->stream));
  hipLaunchKernelGGL((tsx_k_ref_to_planes<T, float>), dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, nv, g.Nz, g.xm,
                     g.ym, dev, planes, flag, (const uint8_t *)s->l1d);  // (s->l1d: this call's, set before)
  HIPCHK(hipGetLastError());
  int lossy = 0;
  HIPCHK(hipMemcpyAsync(&lossy, flag, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (lossy) {
    // the direct tables are real32 (irealLUT) and the reference only widens them (src/pprts.F90:3121-3143, 3457): values that
    // real32 cannot hold did not come from get_coeff
    tsx_set_error(std::string("tsx_dir_set_coeffs: ") + what + " holds values that are not exactly representable in real32");
    return TSX_ERR_UNSUPPORTED;
  }
  return TSX_OK;
}

extern "C" int tsx_dir_set_coeffs(tsx_solver *s, const void *dir2dir, const void *dir2diff, int coeff_kind, const uint8_t *l1d,
                                  const double *a33, const double *a13, const double *a23, double dx, double dy, int where) {
  ARGCHK(s && dir2dir && l1d, "tsx_dir_set_coeffs: null argument");
  ARGCHK(coeff_kind == 4 || coeff_kind == 8, "tsx_dir_set_coeffs: coeff_kind must be 4 or 8");
  if (int rc_c = tsx_refuse_collapsed(s, "tsx_dir_set_coeffs")) return rc_c;
  ARGCHK(dx > 0 && dy > 0, "tsx_dir_set_coeffs: dx, dy must be positive");
  if (!s->have_sun) {
    tsx_set_error("tsx_dir_set_coeffs: call tsx_pprts_set_angles first (the sweep order and the coefficients depend on the sun)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  const int S = dir_streams(s);
  int rc;
  std::vector<uint8_t> l1d_h(g.Nz);
  if (where == TSX_HOST) memcpy(l1d_h.data(), l1d, g.Nz);
  else HIPCHK(hipMemcpy(l1d_h.data(), l1d, g.Nz, hipMemcpyDeviceToHost));
  bool any = false;
  int n1d = 0;
  for (int k = 0; k < g.Nz; ++k) {
    any |= l1d_h[k] != 0;
    n1d += l1d_h[k] != 0;
  }
  // every argument check before any state changes ...
  ARGCHK(!any || a33, "tsx_dir_set_coeffs: a33 required when any layer is 1-D");
  ARGCHK(!any || !dir2diff || (a13 && a23), "tsx_dir_set_coeffs: a13 / a23 required with dir2diff when any layer is 1-D");
  // ... and from here on the coefficients of an earlier call are gone: a call that fails below (values real32 cannot hold, a HIP
  // error) must not leave tsx_dir_solve / tsx_setup_b_solar running on a mix of old and rejected coefficients
  s->dir_coeffs_valid = false;
  s->dir_seam = s->dir_seam_S = false;
  HIPCHK(hipMemcpyAsync(s->l1d, l1d_h.data(), g.Nz, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));  // l1d_h is a local
  s->any_l1d = any;
  s->n1d = n1d;
  if (any) {  // 1-D layers: the beam's transmission a33 and its sources a13 / a23 (src/pprts.F90:4513-4520, 4709-4721)
    if ((rc = seam_cellfield(s, &s->a33, a33, where))) return rc;
    if (a13 && (rc = seam_cellfield(s, &s->a13, a13, where))) return rc;
    if (a23 && (rc = seam_cellfield(s, &s->a23, a23, where))) return rc;
  }
  if (!s->dirT) HIPCHK(tsx_dev_malloc((void **)&s->dirT, sizeof(float) * (size_t)S * S * g.Nc));
  if (!s->dirS) {
    HIPCHK(tsx_dev_malloc((void **)&s->dirS, sizeof(float) * (size_t)S * g.D * g.Nc));
    HIPCHK(hipMemsetAsync(s->dirS, 0, sizeof(float) * (size_t)S * g.D * g.Nc, s->stream));
  }
  rc = coeff_kind == 8 ? seam_import_coeff<double>(s, dir2dir, S * S, s->dirT, where, "dir2dir")
                       : seam_import_coeff<float>(s, dir2dir, S * S, s->dirT, where, "dir2dir");
  if (rc) return rc;
  s->dir_seam_S = false;
  if (dir2diff) {
    rc = coeff_kind == 8 ? seam_import_coeff<double>(s, dir2diff, S * g.D, s->dirS, where, "dir2diff")
                         : seam_import_coeff<float>(s, dir2diff, S * g.D, s->dirS, where, "dir2diff");
    if (rc) return rc;
    s->dir_seam_S = true;
  } else {  // no source coefficients handed over: none of an earlier call's stay behind
    HIPCHK(hipMemsetAsync(s->dirS, 0, sizeof(float) * (size_t)S * g.D * g.Nc, s->stream));
  }
  s->opt_dx = dx;
  s->opt_dy = dy;
  s->dir_coeffs_valid = true;
  s->dir_seam = true;
  return dir_halo_zero(s);
}

static int seam_edir_buffers(tsx_solver *s) {
  const size_t n = (size_t)dir_streams(s) * (size_t)(s->geo.Nz + 1) * s->geo.ncol;
  if (!s->edir_a) {
    HIPCHK(tsx_dev_malloc((void **)&s->edir_a, sizeof(double) * n));
    HIPCHK(hipMemsetAsync(s->edir_a, 0, sizeof(double) * n, s->stream));
  }
  if (!s->edir_b) {
    HIPCHK(tsx_dev_malloc((void **)&s->edir_b, sizeof(double) * n));
    HIPCHK(hipMemsetAsync(s->edir_b, 0, sizeof(double) * n, s->stream));
  }
  return TSX_OK;
}
static int seam_edir_import(tsx_solver *s, const void *edir, int kind, int where) {
  const TsxGeo &g = s->geo;
  const int S = dir_streams(s);
  const size_t n = (size_t)S * (size_t)(g.Nz + 1) * g.ncol;
  TsxSeamIn in;
  int rc;
  if ((rc = seam_edir_buffers(s))) return rc;
  if ((rc = seam_in(s, edir, n, kind, where, &in))) return rc;
  hipLaunchKernelGGL((tsx_k_ref_to_planes<double, double>), dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, S, g.Nz + 1,
                     g.xm, g.ym, in.p, s->edir_a, (int *)nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));  // `in` owns the staging buffers
  return dir_halo_zero(s);                  // faces received for another iterate mean nothing for this one
}

extern "C" int tsx_dir_solve(tsx_solver *s, double edirTOA, void *edir, int vec_kind, int where, double rtol, double atol,
                             int32_t maxit, int32_t *niter, double *residual, int32_t *converged) {
  ARGCHK(s && edir, "tsx_dir_solve: null argument");
  if (!s->dir_coeffs_valid || !s->dir_seam) {
    tsx_set_error("tsx_dir_solve: call tsx_dir_set_coeffs first");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  const int S = dir_streams(s);
  const size_t n = (size_t)S * (size_t)(g.Nz + 1) * g.ncol;
  int rc;
  if ((rc = seam_edir_import(s, edir, vec_kind, where))) return rc;  // v0 = solution%edir (src/pprts.F90:2722-2724, 2746)
  const double k_rt = s->dir_rtol, k_at = s->dir_atol;
  const int k_mx = s->dir_maxit;
  s->dir_rtol = rtol;
  s->dir_atol = atol;
  s->dir_maxit = maxit;
  // the tolerances are the caller's as they are (explicit_edir has applied -ksp_complete_initial_run to them already,
  // src/pprts_explicit.F90:106-121); an iteration limit that is reached is reported, not raised
  rc = PIPE_CALL(direct_solve, s, edirTOA, false, false);
  s->dir_rtol = k_rt;
  s->dir_atol = k_at;
  s->dir_maxit = k_mx;
  if (rc) return rc;
  const TsxDirScalars *dh = (const TsxDirScalars *)s->dsc_host;
  if (niter) *niter = dh->iter;
  if (residual) *residual = dh->res;
  if (converged) *converged = dh->converged;
  TsxSeamOut out;
  if ((rc = seam_out_begin(s, edir, n, vec_kind, where, &out))) return rc;
  hipLaunchKernelGGL(tsx_k_planes_to_ref, dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, S, g.Nz + 1, g.xm, g.ym,
                     s->edir_a, out.p);
  HIPCHK(hipGetLastError());
  s->last_lsolar = 1;
  return seam_out_finish(s, &out);
}

// b of the diffuse system from the direct beam (set_solar_source, src/pprts.F90:4684-4846)
template <int NTOP, int NSIDE, int DTOP, int DSIDE>
static int seam_b_solar_t(tsx_solver *s, double *b_dev) {
  const TsxGeo &g = s->geo;
  TsxDirHalo hb;
  int rc;
  if ((rc = dir_halo(s, &hb))) return rc;
  hipLaunchKernelGGL((tsx_k_setup_b_solar<NTOP, NSIDE, DTOP, DSIDE>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g, make_sun(s),
                     s->dirS, s->l1d, s->a13, s->a23, s->albedo, s->edir_a, s->vb, hb);
  HIPCHK(hipGetLastError());
  return export_vec<NTOP, NSIDE>(s, s->vb, b_dev);
}
extern "C" int tsx_setup_b_solar(tsx_solver *s, const void *edir, const double *albedo, void *b, int vec_kind, int where) {
  ARGCHK(s && b, "tsx_setup_b_solar: null argument");
  if (int rc_c = tsx_refuse_collapsed(s, "tsx_setup_b_solar")) return rc_c;
  if (!s->dir_coeffs_valid || !s->dir_seam || !s->dir_seam_S) {
    tsx_set_error("tsx_setup_b_solar: call tsx_dir_set_coeffs with dir2diff first");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  int rc;
  if (albedo) {
    HIPCHK(hipMemcpyAsync(s->albedo, albedo, sizeof(double) * g.ncol, where == TSX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                          s->stream));
    s->have_albedo = true;
  } else if (!s->have_albedo) {
    tsx_set_error("tsx_setup_b_solar: no albedo (pass it, or call tsx_diff_set_coeffs first)");
    return TSX_ERR_STATE;
  }
  if (edir) {
    if (!(g.wrap_x && g.wrap_y)) {
      tsx_set_error("tsx_setup_b_solar: on several ranks the beam is the one tsx_dir_solve left on the device (pass edir = NULL): "
                    "the faces the sweep exchanged belong to it");
      return TSX_ERR_UNSUPPORTED;
    }
    if ((rc = seam_edir_import(s, edir, vec_kind, where))) return rc;
  } else if (!s->edir_a) {
    tsx_set_error("tsx_setup_b_solar: no direct beam on the device (tsx_dir_solve) and none given");
    return TSX_ERR_STATE;
  }
  TsxSeamOut out;
  if ((rc = seam_out_begin(s, b, (size_t)g.N, vec_kind, where, &out))) return rc;
  if ((rc = PIPE_CALL(seam_b_solar_t, s, out.p))) return rc;
  return seam_out_finish(s, &out);
}

// b of the diffuse system from thermal emission (set_thermal_source, src/pprts.F90:4848-4987)
template <int NTOP, int NSIDE, int DTOP, int DSIDE>
static int seam_b_thermal_t(tsx_solver *s, double *b_dev) {
  const TsxGeo &g = s->geo;
  int rc;
  if ((rc = tsx_dedup_ensure(s))) return rc;
  const double *cs = s->dd_on ? s->dd_colsum : (const double *)nullptr;
  if (s->coef_bytes == 4)
    hipLaunchKernelGGL((tsx_k_setup_b_thermal<NTOP, NSIDE, float>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g,
                       (const float *)s->coef, s->l1d, s->a11, s->a12, s->albedo, s->planck, s->bsrfc, s->d_kabs, s->d_dz, s->opt_dx,
                       s->opt_dy, s->vb, cs, s->dd_cidx, (long long)s->dd_nent, (const double *)nullptr);
  else
    hipLaunchKernelGGL((tsx_k_setup_b_thermal<NTOP, NSIDE, double>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g,
                       (const double *)s->coef, s->l1d, s->a11, s->a12, s->albedo, s->planck, s->bsrfc, s->d_kabs, s->d_dz, s->opt_dx,
                       s->opt_dy, s->vb, (const double *)nullptr, (const int *)nullptr, 0ll, (const double *)nullptr);
  HIPCHK(hipGetLastError());
  return export_vec<NTOP, NSIDE>(s, s->vb, b_dev);
}
extern "C" int tsx_setup_b_thermal(tsx_solver *s, const double *planck, const double *planck_srfc, const double *kabs,
                                   const double *dz, double dx, double dy, void *b, int vec_kind, int where) {
  ARGCHK(s && planck && kabs && dz && b, "tsx_setup_b_thermal: null argument");
  ARGCHK(dx > 0 && dy > 0, "tsx_setup_b_thermal: dx, dy must be positive");
  if (int rc_c = tsx_refuse_collapsed(s, "tsx_setup_b_thermal")) return rc_c;
  if (!s->have_coeffs) {
    tsx_set_error("tsx_setup_b_thermal: call tsx_diff_set_coeffs first (emissivities come from the diffuse blocks, a11 / a12 and the albedo)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  int rc;
  if ((rc = keep_field(s, &s->planck, planck, (size_t)(g.Nz + 1) * g.ncol, where))) return rc;
  if ((rc = keep_planck_srfc(s, planck_srfc, where))) return rc;
  if ((rc = keep_field(s, &s->d_kabs, kabs, (size_t)g.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_dz, dz, (size_t)g.Nc, where))) return rc;
  s->cell_samp_src[0] = nullptr;  // d_kabs / d_dz were overwritten in place: the cached LUT coordinates (tsx_k_cell_samples) are of the old ones
  s->opt_dx = dx;
  s->opt_dy = dy;
  TsxSeamOut out;
  if ((rc = seam_out_begin(s, b, (size_t)g.N, vec_kind, where, &out))) return rc;
  if ((rc = PIPE_CALL(seam_b_thermal_t, s, out.p))) return rc;
  s->last_lsolar = 0;
  return seam_out_finish(s, &out);
}
