// tsx_pipeline.hip -- host side of the whole-g-point pipeline (tsx_pprts_*), and behind it the seam-level entries (tsx_dir_*, tsx_setup_b_*,
// the *_r entries): both launch the kernels of tsx_pipeline.hpp, which this unit alone includes.
// Solvers 3_10 (S = 3 direct streams: 1 top, 1 per side) and 8_16 (S = 8: 4 top with area_divider 4, 2 per side with
// area_divider 2; src/pprts.F90:413-425): the kernels are templates over the stream counts, PIPE_CALL picks the instance.
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <map>
#include <string>
#include <vector>

#include "tsx_host.hpp"
#include "tsx_peer.hpp"
#include "tsx_pipeline.hpp"

static int pipeline_guard(tsx_solver *s, const char *who) {
  (void)s;
  (void)who;
  return TSX_OK;
}
static inline int dir_streams(const tsx_solver *s) { return s->geo.ntop == 2 ? 3 : 8; }
static inline int dir_side_streams(const tsx_solver *s) { return s->geo.ntop == 2 ? 1 : 2; }
static inline int dir_top_div(const tsx_solver *s) { return s->geo.ntop == 2 ? 1 : 4; }
#define PIPE_CALL(fn, ...) (s->geo.ntop == 2 ? fn<2, 4, 1, 1>(__VA_ARGS__) : fn<8, 4, 4, 2>(__VA_ARGS__))

static TsxSun make_sun(const tsx_solver *s) {
  TsxSun u;
  u.phi = s->sun_phi;
  u.theta = s->sun_theta;
  u.mu = s->sun_mu;
  u.costheta = s->sun_costheta;
  u.symmetry_phi = s->sun_symphi;
  u.xinc = s->sun_xinc;
  u.yinc = s->sun_yinc;
  return u;
}

// TSX_DEBUG_CHECKS=<file prefix> (debugging a rare deviation, tests only): at a few points of a g-point the arrays that must not change
// between them -- the shared blocks in both layouts, their column sums, the indices, the preconditioner's packed records -- are
// copied to the host and hashed; one line per array and point is appended to <prefix>.<pid>.  Identical inputs give identical
// lines, so the odd line out over many runs names the array and the phase.
static void tsx_debug_checkpoint(tsx_solver *s, const char *label) {
  const char *pre = getenv("TSX_DEBUG_CHECKS");
  if (!pre || !*pre) return;
  if (hipStreamSynchronize(s->stream) != hipSuccess) return;
  char fn[512];
  snprintf(fn, sizeof(fn), "%s.%d", pre, (int)getpid());
  FILE *fh = fopen(fn, "a");
  if (!fh) return;
  const TsxGeo &g = s->geo;
  const long long Nc = g.Nc, nent = s->dd_nent;
  const int DD = g.D * g.D;
  struct Arr { const char *name; const void *p; size_t bytes; };
  const Arr arrs[] = {{"cidx", s->dd_cidx, sizeof(int) * (size_t)Nc},
                      {"cidx_split", s->dd_cidx_split, sizeof(int) * (size_t)Nc},
                      {"ent_cell", s->dd_ent_cell, sizeof(int) * (size_t)nent},
                      {"Cd", s->dd_coef, sizeof(float) * (size_t)DD * nent},
                      {"Ce", s->dd_coef_e, sizeof(float) * (size_t)DD * nent},
                      {"colsum", s->dd_colsum, sizeof(double) * (size_t)g.D * nent},
                      {"packed_records", s->coef_h, (size_t)16 * 9 * Nc},
                      {"l1d", s->l1d, (size_t)g.Nz},
                      {"b", s->vb, sizeof(double) * (size_t)g.N},
                      {"x", s->vx, sizeof(double) * (size_t)g.N}};
  for (const Arr &a : arrs) {
    unsigned long long h = 1469598103934665603ull;
    if (a.p && a.bytes && s->dd_on) {
      std::vector<unsigned char> host(a.bytes);
      if (hipMemcpy(host.data(), a.p, a.bytes, hipMemcpyDeviceToHost) == hipSuccess)
        for (unsigned char c : host) h = (h ^ c) * 1099511628211ull;
    }
    fprintf(fh, "rank %d %s %s nent %lld %016llx\n", s->grid.rank, label, a.name, nent, h);
  }
  if (s->dd_on && nent > 0 && nent <= 64) {  // small enough to print: the representatives, where the two layouts live, what they start with
    std::vector<int> ec((size_t)nent);
    std::vector<float> cd(8), ce(8);
    if (hipMemcpy(ec.data(), s->dd_ent_cell, sizeof(int) * (size_t)nent, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(cd.data(), s->dd_coef, sizeof(float) * 8, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(ce.data(), s->dd_coef_e, sizeof(float) * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(fh, "rank %d %s detail nent %lld cap %d Ce-Cd %lld ent_cell", s->grid.rank, label, nent, s->dd_cap,
              (long long)(s->dd_coef_e - s->dd_coef));
      for (long long q = 0; q < nent; ++q) fprintf(fh, " %d", ec[(size_t)q]);
      fprintf(fh, " Cd");
      for (float v : cd) fprintf(fh, " %.6g", v);
      fprintf(fh, " Ce");
      for (float v : ce) fprintf(fh, " %.6g", v);
      fprintf(fh, "\n");
    }
  }
  fclose(fh);
}

// face buffers of the direct beam (dirside%dof streams per face): allocated on first use, zero = "no beam yet"
static int dir_halo(tsx_solver *s, TsxDirHalo *hb) {
  const TsxGeo &g = s->geo;
  memset(hb, 0, sizeof(*hb));
  if (g.wrap_x && g.wrap_y) return TSX_OK;
  const size_t ds = (size_t)dir_side_streams(s);
  const size_t cnt[4] = {ds * g.Nz * g.ym, ds * g.Nz * g.ym, ds * g.Nz * g.xm, ds * g.Nz * g.xm};
  for (int q = 0; q < 4; ++q) {
    if (!s->dsend[q]) {
      HIPCHK(tsx_dev_malloc((void **)&s->dsend[q], sizeof(double) * cnt[q]));
      HIPCHK(hipMemsetAsync(s->dsend[q], 0, sizeof(double) * cnt[q], s->stream));
    }
    if (!s->drecv[q]) {
      HIPCHK(tsx_dev_malloc((void **)&s->drecv[q], sizeof(double) * cnt[q]));
      HIPCHK(hipMemsetAsync(s->drecv[q], 0, sizeof(double) * cnt[q], s->stream));
    }
  }
  hb->sendW = s->dsend[0]; hb->sendE = s->dsend[1]; hb->sendS = s->dsend[2]; hb->sendN = s->dsend[3];
  hb->recvW = s->drecv[0]; hb->recvE = s->drecv[1]; hb->recvS = s->drecv[2]; hb->recvN = s->drecv[3];
  return TSX_OK;
}
static int dir_halo_zero(tsx_solver *s) {
  const TsxGeo &g = s->geo;
  const size_t ds = (size_t)dir_side_streams(s);
  const size_t cnt[4] = {ds * g.Nz * g.ym, ds * g.Nz * g.ym, ds * g.Nz * g.xm, ds * g.Nz * g.xm};
  for (int q = 0; q < 4; ++q) {
    if (s->dsend[q]) HIPCHK(hipMemsetAsync(s->dsend[q], 0, sizeof(double) * cnt[q], s->stream));
    if (s->drecv[q]) HIPCHK(hipMemsetAsync(s->drecv[q], 0, sizeof(double) * cnt[q], s->stream));
  }
  return TSX_OK;
}

// setup_suninfo, src/pprts.F90:1118-1183
extern "C" int tsx_pprts_set_angles(tsx_solver *s, double phi0, double theta0) {
  ARGCHK(s, "tsx_pprts_set_angles: null");
  const double d2r = 3.14159265358979323846 / 180.0;
  s->sun_phi = phi0;
  s->sun_theta = theta0;
  s->sun_mu = fmax(cos(theta0 * d2r), 0.0);
  if (s->sun_theta >= 90.0) s->sun_theta = -1.0;
  s->sun_costheta = fmax(cos(s->sun_theta * d2r), 0.0);
  const double sp = acos(cos(phi0 * d2r));
  s->sun_symphi = fmin(90.0, fmax(0.0, asin(sin(sp)) / d2r));
  s->sun_xinc = sin(phi0 * d2r) > 0.0 ? 0 : 1;
  s->sun_yinc = cos(phi0 * d2r) < 0.0 ? 1 : 0;
  s->have_sun = true;
  if (dir_halo_zero(s)) return TSX_ERR_HIP;  // the faces exchanged for another sun direction mean something else
  // the coefficients depend on the sun: whatever was looked up or handed over (tsx_dir_set_coeffs) is void, and what the next
  // tsx_pprts_solve looks up must not pass for coefficients of the direct seam
  s->dir_coeffs_valid = false;
  s->dir_seam = s->dir_seam_S = false;
  return TSX_OK;
}

static int lut_upload(TsxLutHost &L, const float *table, int nvec, long long nentries, int ndim, const int32_t *n,
                      const float *axes_concat, int where) {
  long long nax = 0;
  for (int d = 0; d < ndim; ++d) nax += n[d];
  if (L.d_axes) HIPCHK(tsx_dev_free(L.d_axes));
  if (L.d_table) HIPCHK(tsx_dev_free(L.d_table));
  L = TsxLutHost();
  HIPCHK(tsx_dev_malloc((void **)&L.d_axes, sizeof(float) * nax));
  HIPCHK(tsx_dev_malloc((void **)&L.d_table, sizeof(float) * (size_t)nvec * nentries));
  const hipMemcpyKind mk = where == TSX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  HIPCHK(hipMemcpy(L.d_axes, axes_concat, sizeof(float) * nax, mk));
  HIPCHK(hipMemcpy(L.d_table, table, sizeof(float) * (size_t)nvec * nentries, mk));
  L.ndim = ndim;
  L.nvec = nvec;
  L.nentries = nentries;
  for (int d = 0; d < ndim; ++d) L.n[d] = n[d];
  L.ready = true;
  return TSX_OK;
}

static TsxLutDev lut_dev(const TsxLutHost &H) {
  TsxLutDev L;
  memset(&L, 0, sizeof(L));
  L.ndim = H.ndim;
  L.nvec = H.nvec;
  long long off = 1;
  int aoff = 0;
  for (int d = 0; d < H.ndim; ++d) {
    L.n[d] = H.n[d];
    L.axis_off[d] = aoff;
    aoff += H.n[d];
    L.offs[d] = off;
    off *= H.n[d];
  }
  L.axes = H.d_axes;
  L.table = H.d_table;
  return L;
}

extern "C" int tsx_lut_set_direct(tsx_solver *s, const float *Tdir, const float *Sdir, int64_t nentries, int32_t ndim,
                                  const int32_t *n, const float *axes_concat, int where) {
  ARGCHK(s && Tdir && Sdir && n && axes_concat, "tsx_lut_set_direct: null argument");
  ARGCHK(ndim == 6, "tsx_lut_set_direct: direct tables have 6 dimensions (tau, w0, aspect_zx, g, phi, theta)");
  int rc = pipeline_guard(s, "tsx_lut_set_direct");
  if (rc) return rc;
  long long prod = 1;
  for (int d = 0; d < ndim; ++d) {
    ARGCHK(n[d] >= 1, "tsx_lut_set_direct: empty axis");
    prod *= n[d];
  }
  ARGCHK(prod == nentries, "tsx_lut_set_direct: nentries != product of axis lengths");
  HIPCHK(hipSetDevice(s->device));
  const int S = dir_streams(s), D = s->geo.D;
  if ((rc = lut_upload(s->lut_T, Tdir, S * S, nentries, ndim, n, axes_concat, where))) return rc;
  if ((rc = lut_upload(s->lut_S, Sdir, S * D, nentries, ndim, n, axes_concat, where))) return rc;
  s->dir_coeffs_valid = false;
  return TSX_OK;
}

// map a `.mmap4` table (src/mmap.F90:129-203); returns base pointer (to munmap), data pointer and shape
static int mmap4_open(const char *path, void **base, size_t *maplen, const float **data, size_t *dim1, size_t *dim2) {
  const long pagesize = sysconf(_SC_PAGESIZE);
  int fd = open(path, O_RDONLY);
  if (fd < 0) {
    tsx_set_error(std::string("cannot open ") + path);
    return TSX_ERR_ARG;
  }
  std::vector<size_t> header((size_t)pagesize / sizeof(size_t));
  if (read(fd, header.data(), (size_t)pagesize) != pagesize) {
    close(fd);
    tsx_set_error(std::string("short mmap4 header: ") + path);
    return TSX_ERR_ARG;
  }
  if (header[0] != 4 || header[2] != 4 * header[1] || header[3] * header[4] != header[1] || header[5] != 0) {
    close(fd);
    tsx_set_error(std::string("not a 2-D real32 mmap4 table: ") + path);
    return TSX_ERR_ARG;
  }
  *maplen = header[2] + (size_t)pagesize;
  void *m = mmap(nullptr, *maplen, PROT_READ, MAP_PRIVATE | MAP_NORESERVE, fd, 0);
  close(fd);
  if (m == MAP_FAILED) {
    tsx_set_error(std::string("mmap failed: ") + path);
    return TSX_ERR_ARG;
  }
  *base = m;
  *data = (const float *)((const char *)m + pagesize);
  *dim1 = header[3];
  *dim2 = header[4];
  return TSX_OK;
}

// Tdir/Sdir from `.mmap4` files.  Axes: the LUT_3_10 direct preset (4 diffuse axes + phi19, theta19 = linspace(0, 90),
// src/optprop_base.F90:228-235) unless `<tdir_path>.axes` exists (text: ndim, then per axis: n v1 .. vn) -- the
// thinned tables tests and benches write carry that sidecar.
extern "C" int tsx_lut_load_direct_mmap4(tsx_solver *s, const char *tdir_path, const char *sdir_path) {
  ARGCHK(s && tdir_path && sdir_path, "tsx_lut_load_direct_mmap4: null argument");
  std::vector<int32_t> n;
  std::vector<float> axes;
  const std::string side = std::string(tdir_path) + ".axes";
  if (FILE *f = fopen(side.c_str(), "r")) {
    int ndim = 0;
    if (fscanf(f, "%d", &ndim) != 1 || ndim != 6) {
      fclose(f);
      tsx_set_error("bad axes sidecar: " + side);
      return TSX_ERR_ARG;
    }
    for (int d = 0; d < ndim; ++d) {
      int m = 0;
      if (fscanf(f, "%d", &m) != 1 || m < 1) {
        fclose(f);
        tsx_set_error("bad axes sidecar: " + side);
        return TSX_ERR_ARG;
      }
      n.push_back(m);
      for (int q = 0; q < m; ++q) {
        float v;
        if (fscanf(f, "%f", &v) != 1) {
          fclose(f);
          tsx_set_error("bad axes sidecar: " + side);
          return TSX_ERR_ARG;
        }
        axes.push_back(v);
      }
    }
    fclose(f);
  } else {
    n = {31, 20, 23, 6, 19, 19};
    axes.insert(axes.end(), tsx_preset_tau31, tsx_preset_tau31 + 31);
    axes.insert(axes.end(), tsx_preset_w020, tsx_preset_w020 + 20);
    axes.insert(axes.end(), tsx_preset_aspect23, tsx_preset_aspect23 + 23);
    axes.insert(axes.end(), tsx_preset_g6, tsx_preset_g6 + 6);
    for (int rep = 0; rep < 2; ++rep)
      for (int q = 0; q < 19; ++q) axes.push_back((float)(90.0 * q / 18.0));
  }
  void *bt = nullptr, *bs = nullptr;
  size_t lt = 0, ls = 0, t1, t2, s1, s2;
  const float *dt = nullptr, *ds = nullptr;
  int rc = mmap4_open(tdir_path, &bt, &lt, &dt, &t1, &t2);
  if (rc) return rc;
  if ((rc = mmap4_open(sdir_path, &bs, &ls, &ds, &s1, &s2))) {
    munmap(bt, lt);
    return rc;
  }
  const size_t S_ = (size_t)dir_streams(s);
  if (t2 != s2 || t1 != S_ * S_ || s1 != S_ * s->geo.D) {
    munmap(bt, lt);
    munmap(bs, ls);
    tsx_set_error("tsx_lut_load_direct_mmap4: table shapes do not fit this solver's stream counts");
    return TSX_ERR_ARG;
  }
  rc = tsx_lut_set_direct(s, dt, ds, (int64_t)t2, 6, n.data(), axes.data(), TSX_HOST);
  munmap(bt, lt);
  munmap(bs, ls);
  return rc;
}

// device-to-device copy on the solver's stream as a kernel of this library: hipMemcpyAsync's blit kernel moved the five fields of a
// g-point (168 MB) in 1.6 ms -- 9 % of config 4's device time (scripts/c4_profile.sh: __amd_rocclr_copyBuffer) -- a streaming
// copy with 16-byte accesses takes 0.07 ms
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_d2d16(long long n16, const uint4 *__restrict__ a, uint4 *__restrict__ b) {
  const long long stride = (long long)gridDim.x * TSX_BLOCK;
  long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x;
  for (; q + 3 * stride < n16; q += 4 * stride) {
    const uint4 v0 = a[q], v1 = a[q + stride], v2 = a[q + 2 * stride], v3 = a[q + 3 * stride];
    b[q] = v0;
    b[q + stride] = v1;
    b[q + 2 * stride] = v2;
    b[q + 3 * stride] = v3;
  }
  for (; q < n16; q += stride) b[q] = a[q];
}
static int tsx_d2d(tsx_solver *s, void *dst, const void *src, size_t bytes) {
  if (bytes >= 4096 && (((uintptr_t)dst | (uintptr_t)src | bytes) & 15) == 0) {
    const long long n16 = (long long)(bytes >> 4);
    hipLaunchKernelGGL(tsx_k_d2d16, dim3(grid_for(n16 / 4, 4096)), dim3(TSX_BLOCK), 0, s->stream, n16, (const uint4 *)src, (uint4 *)dst);
    HIPCHK(hipGetLastError());
    return TSX_OK;
  }
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->stream));
  return TSX_OK;
}
// upload (or alias-copy) one (k,i,j) reference-layout field
static int keep_field(tsx_solver *s, double **dst, const double *src, size_t n, int where) {
  if (!*dst) HIPCHK(tsx_dev_malloc((void **)dst, n * sizeof(double)));
  if (where != TSX_HOST) return tsx_d2d(s, *dst, src, n * sizeof(double));
  HIPCHK(hipMemcpyAsync(*dst, src, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return TSX_OK;
}

// atm%Bsrfc follows the optional argument planck_srfc of set_optical_properties: kept when present, dropped when absent
// (src/pprts.F90:1823-1829)
static int keep_planck_srfc(tsx_solver *s, const double *planck_srfc, int where) {
  if (planck_srfc) return keep_field(s, &s->bsrfc, planck_srfc, (size_t)s->geo.ncol, where);
  if (s->bsrfc) {
    HIPCHK(tsx_dev_free(s->bsrfc));
    s->bsrfc = nullptr;
  }
  return TSX_OK;
}

extern "C" int tsx_pprts_set_optprop(tsx_solver *s, const double *kabs, const double *ksca, const double *g,
                                     const double *dz, double dx, double dy, const double *albedo, const uint8_t *l1d,
                                     const double *a11, const double *a12, const double *a13, const double *a23,
                                     const double *a33, const double *planck, const double *planck_srfc, int where) {
  ARGCHK(s && kabs && ksca && g && dz && albedo && l1d, "tsx_pprts_set_optprop: null argument");
  ARGCHK(dx > 0 && dy > 0, "tsx_pprts_set_optprop: dx, dy must be positive");
  if (int rc_c = tsx_refuse_collapsed(s, "tsx_pprts_set_optprop")) return rc_c;
  if (s->mode_1d) {
    tsx_set_error("tsx_pprts_set_optprop: a handle with a 1-D solver takes tsx_pprts_set_optical_properties");
    return TSX_ERR_STATE;
  }
  if (s->bld_nfaces > 0) {  // the blocks are patched inside tsx_pprts_set_optical_properties only
    tsx_set_error("tsx_pprts_set_optprop: not available with buildings attached (tsx_pprts_set_buildings); use "
                  "tsx_pprts_set_optical_properties");
    return TSX_ERR_UNSUPPORTED;
  }
  int rc = pipeline_guard(s, "tsx_pprts_set_optprop");
  if (rc) return rc;
  HIPCHK(hipSetDevice(s->device));
  TsxLogScope log_scope(s, TSX_EV_SET_OPTPROP);  // set_optprop, src/pprts.F90:1785-2077
  const TsxGeo &gm = s->geo;
  // diffuse blocks + l1d/a11/a12/albedo exactly as the seam-level call does
  if ((rc = tsx_diff_set_optprop(s, kabs, ksca, g, dz, dx, l1d, a11, a12, albedo, where))) return rc;
  if ((rc = keep_field(s, &s->d_kabs, kabs, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_ksca, ksca, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_g, g, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_dz, dz, (size_t)gm.Nc, where))) return rc;
  if (s->any_l1d) {
    ARGCHK(a13 && a23 && a33, "tsx_pprts_set_optprop: a13/a23/a33 required when any layer is 1-D");
    if ((rc = tsx_keep_cellfield(s, &s->a13, a13, where))) return rc;
    if ((rc = tsx_keep_cellfield(s, &s->a23, a23, where))) return rc;
    if ((rc = tsx_keep_cellfield(s, &s->a33, a33, where))) return rc;
  }
  if (planck) {
    if ((rc = keep_field(s, &s->planck, planck, (size_t)(gm.Nz + 1) * gm.ncol, where))) return rc;
  } else if (s->planck) {
    HIPCHK(tsx_dev_free(s->planck));
    s->planck = nullptr;
  }
  if ((rc = keep_planck_srfc(s, planck_srfc, where))) return rc;
  HIPCHK(hipStreamSynchronize(s->stream));
  s->opt_dx = dx;
  s->opt_dy = dy;
  s->have_optprop = true;
  s->dir_coeffs_valid = false;
  s->dir_seam = false;
  return TSX_OK;
}

// 1-D layers of a column of nz layers from the per-layer flags of tsx_k_flag_1d: the bottom layer on its own; the lowest other layer
// that exceeds drags every layer above it along (src/pprts.F90:670-677); with collapse the top `collapse` layers are 1-D whatever the
// flags say (:693-705: the reference only warns); then the count of 1-D layers is applied from the top, as the maximum over the ranks
// (:708-719).  Returns the count (unconstrained_fraction, :721-723).
static int l1d_from_flags(tsx_solver *s, const std::vector<int> &flags, int collapse, std::vector<uint8_t> &l1d, int *n1d) {
  const int nz = (int)flags.size();
  l1d.assign(nz, 0);
  l1d[nz - 1] = flags[nz - 1] != 0;
  for (int k = nz - 2; k >= 0; --k)
    if (flags[k]) {
      for (int q = 0; q <= k; ++q) l1d[q] = 1;
      break;
    }
  for (int k = 0; k < collapse && k < nz; ++k) l1d[k] = 1;
  int n = 0;
  for (int k = 0; k < nz; ++k) n += l1d[k];
  for (int k = 0; k < n; ++k) l1d[k] = 1;
  if (s->grid.nranks > 1) {  // the local sets are prefixes, so OR them
    for (int k0 = 0; k0 < nz; k0 += TSX_NSLOTS) {
      double v[TSX_NSLOTS] = {0};
      const int m = nz - k0 < TSX_NSLOTS ? nz - k0 : TSX_NSLOTS;
      for (int q = 0; q < m; ++q) v[q] = l1d[k0 + q];
      int rc = tsx_allreduce_host(s, v, m);
      if (rc) return rc;
      for (int q = 0; q < m; ++q) l1d[k0 + q] = v[q] > 0.0;
    }
  }
  n = 0;
  for (int k = 0; k < nz; ++k) n += l1d[k];
  *n1d = n;
  return TSX_OK;
}

// The atmosphere-shaped scratch of a collapsed set (pool, allocated on first use, grow-only), for nz_atm layers of ncol columns:
// kabs, ksca, g, dz [nz_atm * ncol] (reference layout), planck [(nz_atm + 1) * ncol], a11, a12, a13, a23, a33 [nz_atm * ncol] (cell
// order), l1d [nz_atm] bytes
struct TsxCollapseScratch {
  double *kabs, *ksca, *g, *dz, *planck, *a[5];
  uint8_t *l1d;
};
static int collapse_scratch(tsx_solver *s, int nz_atm, TsxCollapseScratch *cs) {
  const size_t ncol = (size_t)s->geo.ncol, nc = (size_t)nz_atm * ncol;
  if (nz_atm > s->ca_nz_cap) {
    if (s->ca_buf) HIPCHK(tsx_dev_free(s->ca_buf));
    s->ca_buf = nullptr;
    s->ca_nz_cap = 0;
    HIPCHK(tsx_dev_malloc((void **)&s->ca_buf, sizeof(double) * (9 * nc + (nz_atm + 1) * ncol + ((size_t)nz_atm + 7) / 8)));
    s->ca_nz_cap = nz_atm;
  }
  if (!s->ca_B) HIPCHK(tsx_dev_malloc((void **)&s->ca_B, sizeof(double) * 2 * ncol));
  double *p = s->ca_buf;
  cs->kabs = p, p += nc;
  cs->ksca = p, p += nc;
  cs->g = p, p += nc;
  cs->dz = p, p += nc;
  cs->planck = p, p += (nz_atm + 1) * ncol;
  for (int q = 0; q < 5; ++q) cs->a[q] = p, p += nc;
  cs->l1d = (uint8_t *)p;
  return TSX_OK;
}

// tsx_pprts_set_optical_properties with collapse (src/pprts.F90:1764-2077 with atm%lcollapse): delta scaling, 1-D detection and the
// Eddington coefficients on the atmosphere's Nz + c - 1 layers, handle_atm_collapse (:2080-2123) by tsx_k_collapse_adding, then the
// solver's fields as the atmosphere's at atmk(k) = k + c - 1.  Leaves what the uncollapsed branch leaves: d_kabs .. d_dz, l1d,
// a11 .. a33, planck (when given), n1d / any_l1d, the albedo; and atm%Btop / Bbot in ca_B.
static int collapse_optprop(tsx_solver *s, const double *albedo, const double *kabs, const double *ksca, const double *g,
                            const double *dz, const double *planck, double dx, int ldelta_scaling, int where) {
  const TsxGeo &gm = s->geo;
  const int c = s->collapse, nz_atm = gm.Nz + c - 1;
  const size_t ncol = (size_t)gm.ncol, nca = (size_t)nz_atm * ncol;
  const hipMemcpyKind mk = where == TSX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  int rc;
  TsxCollapseScratch A;
  if ((rc = collapse_scratch(s, nz_atm, &A))) return rc;
  if ((rc = keep_field(s, &A.kabs, kabs, nca, where))) return rc;
  if ((rc = keep_field(s, &A.ksca, ksca, nca, where))) return rc;
  if ((rc = keep_field(s, &A.g, g, nca, where))) return rc;
  if ((rc = keep_field(s, &A.dz, dz, nca, where))) return rc;
  if (planck && (rc = keep_field(s, &A.planck, planck, (size_t)(nz_atm + 1) * ncol, where))) return rc;
  HIPCHK(hipMemcpyAsync(s->albedo, albedo, sizeof(double) * ncol, mk, s->stream));
  s->have_albedo = true;
  if (ldelta_scaling)
    hipLaunchKernelGGL(tsx_k_delta_scale, dim3(grid_for((long long)nca)), dim3(TSX_BLOCK), 0, s->stream, (long long)nca, A.kabs, A.ksca, A.g);
  std::vector<int> flags(nz_atm, 0);
  int *dflags = (int *)s->partials;  // scratch
  HIPCHK(hipMemsetAsync(dflags, 0, sizeof(int) * nz_atm, s->stream));
  hipLaunchKernelGGL(tsx_k_flag_1d, dim3(grid_for((long long)nca)), dim3(TSX_BLOCK), 0, s->stream, (long long)nca, nz_atm, A.dz, dx, 2.0, dflags);
  HIPCHK(hipMemcpyAsync(flags.data(), dflags, sizeof(int) * nz_atm, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  std::vector<uint8_t> l1d;
  if ((rc = l1d_from_flags(s, flags, c, l1d, &s->n1d))) return rc;
  s->any_l1d = true;  // layer 0 at least
  HIPCHK(hipMemcpyAsync(A.l1d, l1d.data(), nz_atm, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(s->l1d, l1d.data() + (c - 1), gm.Nz, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));  // l1d (host vector) must outlive the copies
  TsxGeo ga = gm;
  ga.Nz = nz_atm;
  ga.Nc = (long long)nca;
  hipLaunchKernelGGL(tsx_k_eddington, dim3(grid_for(ga.Nc)), dim3(TSX_BLOCK), 0, s->stream, ga, A.kabs, A.ksca, A.g, A.dz,
                     s->sun_costheta, A.l1d, A.a[0], A.a[1], A.a[2], A.a[3], A.a[4]);
  double **fields[5] = {&s->a11, &s->a12, &s->a13, &s->a23, &s->a33};
  for (double **f : fields)
    if (!*f) HIPCHK(tsx_dev_malloc((void **)f, sizeof(double) * gm.Nc));
  double **views[4] = {&s->d_kabs, &s->d_ksca, &s->d_g, &s->d_dz};
  for (double **f : views)
    if (!*f) HIPCHK(tsx_dev_malloc((void **)f, sizeof(double) * gm.Nc));
  if (planck && !s->planck) HIPCHK(tsx_dev_malloc((void **)&s->planck, sizeof(double) * (gm.Nz + 1) * ncol));
  if (!planck) HIPCHK(hipMemsetAsync(s->ca_B, 0xff, sizeof(double) * 2 * ncol, s->stream));  // NaN: no thermal terms
  hipLaunchKernelGGL(tsx_k_collapse_adding, dim3((unsigned)((ncol + TSX_BLOCK - 1) / TSX_BLOCK)), dim3(TSX_BLOCK), 0, s->stream,
                     (int)ncol, c, nz_atm, A.a[0], A.a[1], A.a[2], A.a[3], A.a[4], A.kabs, A.dz, planck ? A.planck : (const double *)nullptr,
                     s->a11, s->a12, s->a13, s->a23, s->a33, s->ca_B);
  // solver layers k >= 1: atmosphere layers k + c - 1 of the cell-indexed planes
  if (gm.Nz > 1)
    for (int q = 0; q < 5; ++q)
      if ((rc = tsx_d2d(s, *fields[q] + ncol, A.a[q] + (size_t)c * ncol, sizeof(double) * (gm.Nz - 1) * ncol))) return rc;
  const long long nv = (long long)gm.Nz * ncol + (planck ? (long long)(gm.Nz + 1) * ncol : 0);
  hipLaunchKernelGGL(tsx_k_collapse_views, dim3(grid_for(nv)), dim3(TSX_BLOCK), 0, s->stream, (int)ncol, gm.Nz, c, A.kabs, A.ksca, A.g,
                     A.dz, planck ? A.planck : (const double *)nullptr, s->d_kabs, s->d_ksca, s->d_g, s->d_dz, s->planck);
  HIPCHK(hipGetLastError());
  s->ca_have_B = planck != nullptr;
  return TSX_OK;
}

// tsx_pprts_set_optical_properties on a handle with a 1-D solver (tsx_pprts_set_1d_solver): the fields of the atmosphere's
// Nz + c - 1 layers, delta-scaled, and the surface terms -- "dont need LUT, we just compute Twostream anyway" (src/pprts.F90:536).
// No 1-D detection, no coefficient lookups, no preconditioner set-up, and so no reduction over the ranks either.
static int optprop_1d(tsx_solver *s, const double *albedo, const double *kabs, const double *ksca, const double *g, const double *dz,
                      const double *planck, const double *planck_srfc, double dx, double dy, int ldelta_scaling, int where) {
  const TsxGeo &gm = s->geo;
  const int c = s->collapse > 1 ? s->collapse : 1, nz_atm = gm.Nz + c - 1;
  const size_t ncol = (size_t)gm.ncol, nca = (size_t)nz_atm * ncol;
  const hipMemcpyKind mk = where == TSX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  int rc;
  TsxLogScope log_scope(s, TSX_EV_SET_OPTPROP);
  double *pk = nullptr, *ps = nullptr, *pg = nullptr;
  if (c > 1) {
    TsxCollapseScratch A;
    if ((rc = collapse_scratch(s, nz_atm, &A))) return rc;
    if ((rc = keep_field(s, &A.kabs, kabs, nca, where))) return rc;
    if ((rc = keep_field(s, &A.ksca, ksca, nca, where))) return rc;
    if ((rc = keep_field(s, &A.g, g, nca, where))) return rc;
    if ((rc = keep_field(s, &A.dz, dz, nca, where))) return rc;
    if (planck && (rc = keep_field(s, &A.planck, planck, (size_t)(nz_atm + 1) * ncol, where))) return rc;
    s->ca_have_B = planck != nullptr;  // (here: "the atmosphere's planck is held"; atm%Btop / Bbot are not needed by a 1-D solver)
    pk = A.kabs, ps = A.ksca, pg = A.g;
  } else {
    if ((rc = keep_field(s, &s->d_kabs, kabs, nca, where))) return rc;
    if ((rc = keep_field(s, &s->d_ksca, ksca, nca, where))) return rc;
    if ((rc = keep_field(s, &s->d_g, g, nca, where))) return rc;
    if ((rc = keep_field(s, &s->d_dz, dz, nca, where))) return rc;
    if (planck) {
      if ((rc = keep_field(s, &s->planck, planck, (size_t)(nz_atm + 1) * ncol, where))) return rc;
    } else if (s->planck) {
      HIPCHK(tsx_dev_free(s->planck));
      s->planck = nullptr;
    }
    pk = s->d_kabs, ps = s->d_ksca, pg = s->d_g;
  }
  HIPCHK(hipMemcpyAsync(s->albedo, albedo, sizeof(double) * ncol, mk, s->stream));
  s->have_albedo = true;
  if (ldelta_scaling)
    hipLaunchKernelGGL(tsx_k_delta_scale, dim3(grid_for((long long)nca)), dim3(TSX_BLOCK), 0, s->stream, (long long)nca, pk, ps, pg);
  HIPCHK(hipGetLastError());
  if ((rc = keep_planck_srfc(s, planck_srfc, where))) return rc;
  HIPCHK(hipStreamSynchronize(s->stream));
  s->have_coeffs = false;
  s->pcx_valid = s->coef_h_valid = false;
  s->opt_dx = dx;
  s->opt_dy = dy;
  s->have_optprop = true;
  s->dir_coeffs_valid = false;
  s->dir_seam = false;
  return TSX_OK;
}

// set_optical_properties (src/pprts.F90:1764-2000) on the device: delta scaling (:1903-1917), which layers are 1-D
// (:669-677), their Eddington coefficients (:1962-1992), then the coefficient lookups.  Raw (unscaled) fields in.
extern "C" int tsx_pprts_set_optical_properties(tsx_solver *s, const double *albedo, const double *kabs, const double *ksca,
                                                const double *g, const double *dz, const double *planck,
                                                const double *planck_srfc, double dx, double dy, int ldelta_scaling, int where) {
  ARGCHK(s && kabs && ksca && g && dz && albedo, "tsx_pprts_set_optical_properties: null argument");
  ARGCHK(dx > 0 && dy > 0, "tsx_pprts_set_optical_properties: dx, dy must be positive");
  int rc = pipeline_guard(s, "tsx_pprts_set_optical_properties");
  if (rc) return rc;
  if (s->bld_nfaces > 0 && (rc = tsx_buildings_refuse(s, "tsx_pprts_set_optical_properties"))) return rc;
  if (s->mode_1d) {
    HIPCHK(hipSetDevice(s->device));
    return optprop_1d(s, albedo, kabs, ksca, g, dz, planck, planck_srfc, dx, dy, ldelta_scaling, where);
  }
  if (!s->have_sun) {
    tsx_set_error("tsx_pprts_set_optical_properties: call tsx_pprts_set_angles first (Eddington coefficients need mu0)");
    return TSX_ERR_STATE;
  }
  if (!s->lut_diff.ready) {
    tsx_set_error("tsx_pprts_set_optical_properties: load the diffuse LUT first");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  TsxLogScope log_scope(s, TSX_EV_SET_OPTPROP);  // set_optprop, src/pprts.F90:1785-2077
  const TsxGeo &gm = s->geo;
  const hipMemcpyKind mk = where == TSX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (s->collapse > 1) {
    if ((rc = collapse_optprop(s, albedo, kabs, ksca, g, dz, planck, dx, ldelta_scaling, where))) return rc;
  } else {
  if ((rc = keep_field(s, &s->d_kabs, kabs, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_ksca, ksca, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_g, g, (size_t)gm.Nc, where))) return rc;
  if ((rc = keep_field(s, &s->d_dz, dz, (size_t)gm.Nc, where))) return rc;
  HIPCHK(hipMemcpyAsync(s->albedo, albedo, sizeof(double) * gm.ncol, mk, s->stream));
  s->have_albedo = true;
  if (ldelta_scaling)
    hipLaunchKernelGGL(tsx_k_delta_scale, dim3(grid_for(gm.Nc)), dim3(TSX_BLOCK), 0, s->stream, gm.Nc, s->d_kabs, s->d_ksca, s->d_g);
  // 1-D layers: dz/dx > twostr_ratio anywhere in the layer, and then every layer above it
  std::vector<int> flags(gm.Nz, 0);
  int *dflags = (int *)s->partials;  // scratch
  HIPCHK(hipMemsetAsync(dflags, 0, sizeof(int) * gm.Nz, s->stream));
  hipLaunchKernelGGL(tsx_k_flag_1d, dim3(grid_for(gm.Nc)), dim3(TSX_BLOCK), 0, s->stream, gm.Nc, gm.Nz, s->d_dz, dx, 2.0, dflags);
  HIPCHK(hipMemcpyAsync(flags.data(), dflags, sizeof(int) * gm.Nz, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  // the bottom layer on its own; the lowest other layer that exceeds drags every layer above it along; then the count
  // of 1-D layers is applied from the top (src/pprts.F90:670-677, 708-719)
  std::vector<uint8_t> l1d(gm.Nz, 0);
  l1d[gm.Nz - 1] = flags[gm.Nz - 1] != 0;
  for (int k = gm.Nz - 2; k >= 0; --k)
    if (flags[k]) {
      for (int q = 0; q <= k; ++q) l1d[q] = 1;
      break;
    }
  s->n1d = 0;
  for (int k = 0; k < gm.Nz; ++k) s->n1d += l1d[k];
  for (int k = 0; k < s->n1d; ++k) l1d[k] = 1;
  if (s->grid.nranks > 1) {  // N1dlayers_max over the ranks (:708-719): the local sets are prefixes, so OR them
    for (int k0 = 0; k0 < gm.Nz; k0 += TSX_NSLOTS) {
      double v[TSX_NSLOTS] = {0};
      const int n = gm.Nz - k0 < TSX_NSLOTS ? gm.Nz - k0 : TSX_NSLOTS;
      for (int q = 0; q < n; ++q) v[q] = l1d[k0 + q];
      if ((rc = tsx_allreduce_host(s, v, n))) return rc;
      for (int q = 0; q < n; ++q) l1d[k0 + q] = v[q] > 0.0;
    }
  }
  // unconstrained_fraction counts .not. l1d after the prefix has been applied (src/pprts.F90:719-723)
  s->n1d = 0;
  for (int k = 0; k < gm.Nz; ++k) s->n1d += l1d[k];
  s->any_l1d = s->n1d > 0;
  HIPCHK(hipMemcpyAsync(s->l1d, l1d.data(), gm.Nz, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));  // l1d (stack) must outlive the copy
  if (s->bld_nfaces > 0 && (rc = tsx_buildings_check_layers(s, l1d.data()))) {
    s->have_optprop = s->have_coeffs = false;  // the fields above are already the new ones
    return rc;
  }
  if (s->any_l1d) {
    double **fields[5] = {&s->a11, &s->a12, &s->a13, &s->a23, &s->a33};
    for (double **f : fields)
      if (!*f) HIPCHK(tsx_dev_malloc((void **)f, sizeof(double) * gm.Nc));
    hipLaunchKernelGGL(tsx_k_eddington, dim3(grid_for(gm.Nc)), dim3(TSX_BLOCK), 0, s->stream, gm, s->d_kabs, s->d_ksca, s->d_g,
                       s->d_dz, s->sun_costheta, s->l1d, s->a11, s->a12, s->a13, s->a23, s->a33);
  }
  }
  if ((rc = tsx_ensure_coef_storage(s, 4))) return rc;
  // buildings: set_buildings_coeff of alloc_coeff_diff2diff (src/pprts.F90:3579-3677) behind the lookup, before the blocks are shared
  if ((rc = tsx_lut_diffuse_launch(s, s->d_kabs, s->d_ksca, s->d_g, s->d_dz, dx, s->bld_nfaces > 0))) return rc;
  HIPCHK(hipGetLastError());
  if (planck) {
    if (s->collapse <= 1 && (rc = keep_field(s, &s->planck, planck, (size_t)(gm.Nz + 1) * gm.ncol, where))) return rc;
  } else if (s->planck) {
    HIPCHK(tsx_dev_free(s->planck));
    s->planck = nullptr;
  }
  if ((rc = keep_planck_srfc(s, planck_srfc, where))) return rc;
  HIPCHK(hipStreamSynchronize(s->stream));
  s->have_coeffs = true;
  s->pcx_valid = false;
  s->coef_h_valid = false;   // (the shared-storage state was reset / set by tsx_lut_diffuse_launch)
  s->opt_dx = dx;
  s->opt_dy = dy;
  s->have_optprop = true;
  s->dir_coeffs_valid = false;
  s->dir_seam = false;
  tsx_debug_checkpoint(s, "after_set_optprop");
  return TSX_OK;
}

// ---- solver%solutions(uid): one stored solution per uid (src/pprts.F90:2487-2558, get_solution_uid).  The working
// vectors belong to one uid at a time; selecting another one parks the current solution (as real32 -- the reference
// optionally compresses stored solutions too, lcompress_solutions) and brings in that uid's previous solution as the
// initial guess, or -- for a uid that was never solved -- the previous uid's (-initial_guess_from_last_uid, default on),
// or zero.  Results are read right after their solve, as pprts_rrtmg does (rrtmg/rrtmg/pprts_rrtmg.F90:999-1055).
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_to_f32(long long n, const double *__restrict__ a, float *__restrict__ o) {
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < n; q += (long long)gridDim.x * TSX_BLOCK) o[q] = (float)a[q];
}
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_to_f64(long long n, const float *__restrict__ a, double *__restrict__ o) {
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < n; q += (long long)gridDim.x * TSX_BLOCK) o[q] = (double)a[q];
}

void tsx_slots_free(tsx_solver *s) {
  auto *m = (std::map<int, TsxSolSlot> *)s->slots;
  if (!m) return;
  for (auto &kv : *m) {
    if (kv.second.x32) (void)tsx_dev_free(kv.second.x32);
    if (kv.second.e32) (void)tsx_dev_free(kv.second.e32);
    if (kv.second.od) (void)tsx_dev_free(kv.second.od);
  }
  delete m;
  s->slots = nullptr;
}

extern "C" int tsx_pprts_select_solution(tsx_solver *s, int32_t uid) {
  ARGCHK(s, "tsx_pprts_select_solution: null");
  HIPCHK(hipSetDevice(s->device));
  if (!s->slots) s->slots = new std::map<int, TsxSolSlot>();
  auto &m = *(std::map<int, TsxSolSlot> *)s->slots;
  if (uid == s->cur_uid && m.count(uid)) return TSX_OK;
  if (s->mode_1d) {  // 1-D solutions: W/m2 fluxes + absorption, parked as they are (nothing warm-starts from them)
    const size_t nb = sizeof(double) * tsx_1d_solution_doubles(s);
    if (s->have_solution && s->sol_is_1d) {
      TsxSolSlot &cur = m[s->cur_uid];
      if (!cur.od) HIPCHK(tsx_dev_malloc((void **)&cur.od, nb));
      int rc = tsx_d2d(s, cur.od, s->od_flux, nb);
      if (rc) return rc;
      cur.lsolar = s->last_lsolar;
    }
    auto it1 = m.find(uid);
    if (it1 != m.end() && it1->second.od) {
      int rc = tsx_d2d(s, s->od_flux, it1->second.od, nb);
      if (rc) return rc;
      s->have_solution = s->sol_is_1d = true;
      s->last_lsolar = it1->second.lsolar;
    } else {
      s->have_solution = s->sol_is_1d = false;
    }
    s->guess_foreign = false;
    HIPCHK(hipStreamSynchronize(s->stream));
    s->cur_uid = uid;
    if (!m.count(uid)) m[uid] = TsxSolSlot{nullptr, nullptr, 0};
    return TSX_OK;
  }
  const TsxGeo &g = s->geo;
  const long long ne = (long long)dir_streams(s) * (g.Nz + 1) * g.ncol;
  // park the working solution under the uid it belongs to
  if (s->have_solution && !s->guess_foreign) {
    TsxSolSlot &cur = m[s->cur_uid];
    if (!cur.x32) HIPCHK(tsx_dev_malloc((void **)&cur.x32, sizeof(float) * (size_t)g.N));
    hipLaunchKernelGGL(tsx_k_to_f32, dim3(grid_for(g.N)), dim3(TSX_BLOCK), 0, s->stream, g.N, s->vx, cur.x32);
    cur.lsolar = s->last_lsolar;
    if (s->last_lsolar && s->edir_a) {
      if (!cur.e32) HIPCHK(tsx_dev_malloc((void **)&cur.e32, sizeof(float) * (size_t)ne));
      hipLaunchKernelGGL(tsx_k_to_f32, dim3(grid_for(ne)), dim3(TSX_BLOCK), 0, s->stream, ne, s->edir_a, cur.e32);
    }
  }
  // bring in the guess for `uid`: its own previous solution, else the previous uid's, else zero
  auto it = m.find(uid);
  const bool own = it != m.end() && it->second.x32;
  if (!own) it = m.find(uid - 1);
  if (it != m.end() && it->second.x32) {
    const TsxSolSlot &src = it->second;
    hipLaunchKernelGGL(tsx_k_to_f64, dim3(grid_for(g.N)), dim3(TSX_BLOCK), 0, s->stream, g.N, src.x32, s->vx);
    if (src.lsolar && src.e32) {
      if (!s->edir_a) {
        HIPCHK(tsx_dev_malloc((void **)&s->edir_a, sizeof(double) * (size_t)ne));
      }
      hipLaunchKernelGGL(tsx_k_to_f64, dim3(grid_for(ne)), dim3(TSX_BLOCK), 0, s->stream, ne, src.e32, s->edir_a);
    }
    s->have_solution = true;
    s->x_is_zero = false;  // vx now holds a stored solution (a zero_guess before this select must not survive it)
    s->last_lsolar = src.lsolar;
    s->guess_foreign = !own;
    int rc = dir_halo_zero(s);
    if (rc) return rc;
  } else {
    int rc = tsx_pprts_zero_guess(s);
    if (rc) return rc;
    s->have_solution = false;
    s->guess_foreign = false;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  s->cur_uid = uid;
  if (!m.count(uid)) m[uid] = TsxSolSlot{nullptr, nullptr, 0};
  return TSX_OK;
}

extern "C" int tsx_pprts_set_direct_tolerances(tsx_solver *s, double rtol, double atol, int32_t maxit) {
  ARGCHK(s, "tsx_pprts_set_direct_tolerances: null");
  s->dir_rtol = rtol;
  s->dir_atol = atol;
  s->dir_maxit = maxit;
  return TSX_OK;
}

extern "C" int tsx_pprts_zero_guess(tsx_solver *s) {
  ARGCHK(s, "tsx_pprts_zero_guess: null");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemsetAsync(s->vx, 0, sizeof(double) * s->geo.N, s->stream));
  s->x_is_zero = true;
  if (s->edir_a)
    HIPCHK(hipMemsetAsync(s->edir_a, 0, sizeof(double) * dir_streams(s) * (size_t)(s->geo.Nz + 1) * s->geo.ncol, s->stream));
  {
    int rc = dir_halo_zero(s);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}

// init_pprts(..., collapseindex) (src/pprts.F90:213, 229, 849-853, 1067-1078): from the next tsx_pprts_set_optical_properties on,
// the caller's fields describe Nz + c - 1 atmosphere layers and the top c of them are merged into solver layer 0.  A changed c is a
// new atmosphere, as a new init_pprts would be: coefficients, stored solutions and the initial guess are dropped.
extern "C" int tsx_pprts_set_collapse(tsx_solver *s, int32_t collapseindex) {
  ARGCHK(s, "tsx_pprts_set_collapse: null");
  const int c = collapseindex > 1 ? (int)collapseindex : 1;
  if (c == s->collapse) return TSX_OK;
  HIPCHK(hipSetDevice(s->device));
  s->collapse = c;
  s->have_optprop = s->have_coeffs = false;
  s->dir_coeffs_valid = s->dir_seam = s->dir_seam_S = false;
  s->pcx_valid = s->coef_h_valid = false;
  s->ca_have_B = false;
  s->dd_from_coords = false;  // no grouping is taken over from the other atmosphere's coefficients
  s->pcr_have_R = 0;
  tsx_slots_free(s);
  s->cur_uid = 0;
  s->have_solution = s->guess_foreign = s->sol_is_1d = false;
  s->its_hint_cold = s->its_hint_warm = 0;
  s->its_hint_key = 0;
  return tsx_pprts_zero_guess(s);
}

// t_solver_2str / -schwarzschild (src/pprts.F90:2627-2638): from the next tsx_pprts_set_optical_properties on, tsx_pprts_solve
// answers with the 1-D column solver.  A changed mode is another solver: coefficients, optical properties, stored solutions and the
// initial guess are dropped, as tsx_pprts_set_collapse drops them.  A changed nmu alone keeps them (it enters at the next solve).
extern "C" int tsx_pprts_set_1d_solver(tsx_solver *s, int32_t mode, int32_t nmu) {
  ARGCHK(s, "tsx_pprts_set_1d_solver: null");
  ARGCHK(mode == TSX_1D_OFF || mode == TSX_1D_TWOSTREAM || mode == TSX_1D_SCHWARZSCHILD,
         "tsx_pprts_set_1d_solver: mode must be TSX_1D_OFF, TSX_1D_TWOSTREAM or TSX_1D_SCHWARZSCHILD");
  ARGCHK(nmu >= 1 && nmu <= 16, "tsx_pprts_set_1d_solver: nmu must be 1..16");
  s->od_nmu = nmu;
  if (mode == s->mode_1d) return TSX_OK;
  HIPCHK(hipSetDevice(s->device));
  s->mode_1d = mode;
  s->have_optprop = s->have_coeffs = false;
  s->dir_coeffs_valid = s->dir_seam = s->dir_seam_S = false;
  s->pcx_valid = s->coef_h_valid = false;
  s->ca_have_B = false;
  s->dd_from_coords = false;
  s->pcr_have_R = 0;
  tsx_slots_free(s);
  s->cur_uid = 0;
  s->have_solution = s->guess_foreign = s->sol_is_1d = false;
  s->its_hint_cold = s->its_hint_warm = 0;
  s->its_hint_key = 0;
  return tsx_pprts_zero_guess(s);
}

// -initial_guess_from_2str (src/pprts.F90:2560-2567): twostream on the optical properties the handle holds, scattered into the
// solution storage in W per stream (tsx_1d.hip); the next tsx_pprts_solve starts from it, still as the first solve of its uid
// (-ksp_complete_initial_run applies: the guess is made inside `.not. solution%lset`).
extern "C" int tsx_pprts_guess_from_2str(tsx_solver *s, double edirTOA, int lsolar) {
  ARGCHK(s, "tsx_pprts_guess_from_2str: null");
  if (s->mode_1d) {
    tsx_set_error("tsx_pprts_guess_from_2str: this handle solves with a 1-D solver, there is no 3-D solve to start");
    return TSX_ERR_STATE;
  }
  if (!s->have_optprop) {
    tsx_set_error("tsx_pprts_guess_from_2str: call tsx_pprts_set_optical_properties first");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  int rc;
  {
    TsxLogScope log_scope(s, TSX_EV_SOLVE_TWOSTREAM);
    if ((rc = tsx_1d_run(s, edirTOA, lsolar, 0))) return rc;
    if (lsolar && !s->edir_a)
      HIPCHK(tsx_dev_malloc((void **)&s->edir_a, sizeof(double) * dir_streams(s) * (size_t)(g.Nz + 1) * g.ncol));
    if ((rc = tsx_1d_scatter(s, lsolar, s->opt_dx, s->opt_dy, s->vx, s->edir_a))) return rc;
  }
  if ((rc = dir_halo_zero(s))) return rc;  // faces exchanged for an earlier beam do not belong to this guess
  HIPCHK(hipStreamSynchronize(s->stream));
  s->x_is_zero = false;
  s->sol_is_1d = false;
  s->have_solution = true;   // the working vectors hold a guess that is not this uid's solution: the solve that follows is the
  s->guess_foreign = true;   // first of its uid, keeps the guess whatever its kind, and nothing parks it (src/pprts.F90:2532-2575)
  s->last_lsolar = lsolar;
  return TSX_OK;
}

__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_asum(long long n, const double *__restrict__ v, double *__restrict__ partials) {
  double sum[1] = {0.0};
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < n; q += (long long)gridDim.x * TSX_BLOCK) sum[0] += fabs(v[q]);
  tsx_block_reduce_store<1>(sum, partials);
}

template <int NTOP, int NSIDE, int DTOP, int DSIDE>
static int direct_solve(tsx_solver *s, double edirTOA, bool first_of_uid, bool strict = true) {
  const TsxGeo &g = s->geo;
  constexpr int S = DTOP + 2 * DSIDE, D = NTOP + 2 * NSIDE;
  const size_t Ncl = (size_t)(g.Nz + 1) * g.ncol;
  int rc;
  if (!s->dir_coeffs_valid && (!s->lut_T.ready || !s->lut_S.ready)) {  // (valid: tsx_dir_set_coeffs has handed the blocks over)
    tsx_set_error("tsx_pprts_solve: solar solve needs the direct LUT (tsx_lut_set_direct)");
    return TSX_ERR_STATE;
  }
  if (!s->have_sun) {
    tsx_set_error("tsx_pprts_solve: call tsx_pprts_set_angles first");
    return TSX_ERR_STATE;
  }
  const TsxSun sun = make_sun(s);
  TsxLogScope log_scope(s, TSX_EV_COMPUTE_EDIR);  // compute_Edir, src/pprts.F90:2694-2756
  if (!s->dirT) HIPCHK(tsx_dev_malloc((void **)&s->dirT, sizeof(float) * (size_t)S * S * g.Nc));
  if (!s->dirS) HIPCHK(tsx_dev_malloc((void **)&s->dirS, sizeof(float) * (size_t)S * g.D * g.Nc));
  if (!s->dir_coeffs_valid) {  // alloc_coeff_dir2dir / dir2diff (src/pprts.F90:3088-3391)
    TsxLogScope log_lut(s, TSX_EV_GET_COEFF_DIR2DIR);  // get_coeff_dir2dir + get_coeff_dir2diff, :3116-3185, 3257-3392
    const int nbk = grid_for(g.Nc, 8192);
    // the diffuse lookup of these optical properties (tsx_pprts_set_optprop) has left the cells' LUT coordinates
    const bool have = s->cell_samp && s->cell_samp_src[0] == s->d_kabs && s->cell_samp_src[1] == s->d_ksca &&
                      s->cell_samp_src[2] == s->d_g && s->cell_samp_src[3] == s->d_dz && s->cell_samp_dx == s->opt_dx;
    if (!have && (rc = tsx_cell_samples(s, s->d_kabs, s->d_ksca, s->d_g, s->d_dz, s->opt_dx))) return rc;
    const float4 *samp = (const float4 *)s->cell_samp;
    hipLaunchKernelGGL((tsx_k_lut_dir<S * S, S, false>), dim3(nbk), dim3(TSX_BLOCK), 0, s->stream, g, lut_dev(s->lut_T), s->d_kabs,
                       s->d_ksca, s->d_g, s->d_dz, s->opt_dx, (float)sun.symmetry_phi, (float)sun.theta, sun.xinc == 0,
                       sun.yinc == 0, s->l1d, s->dirT, samp);
    hipLaunchKernelGGL((tsx_k_lut_dir<S * D, S, true>), dim3(nbk), dim3(TSX_BLOCK), 0, s->stream, g, lut_dev(s->lut_S), s->d_kabs,
                       s->d_ksca, s->d_g, s->d_dz, s->opt_dx, (float)sun.symmetry_phi, (float)sun.theta, sun.xinc == 0,
                       sun.yinc == 0, s->l1d, s->dirS, samp);
    HIPCHK(hipGetLastError());
    // buildings: set_buildings_coeff of alloc_coeff_dir2dir (src/pprts.F90:3194-3212), behind the lookup (and its quadrant relabelling)
    if (s->bld_nfaces > 0 && (rc = tsx_buildings_zero_dir(s))) return rc;
    s->dir_coeffs_valid = true;
  }
  if (!s->edir_a) {
    HIPCHK(tsx_dev_malloc((void **)&s->edir_a, sizeof(double) * S * Ncl));
    HIPCHK(hipMemsetAsync(s->edir_a, 0, sizeof(double) * S * Ncl, s->stream));
  }
  if (!s->edir_b) {
    HIPCHK(tsx_dev_malloc((void **)&s->edir_b, sizeof(double) * S * Ncl));
    HIPCHK(hipMemsetAsync(s->edir_b, 0, sizeof(double) * S * Ncl, s->stream));
  }
  if (!s->dsc) HIPCHK(tsx_dev_malloc(&s->dsc, sizeof(TsxDirScalars)));
  if (!s->dsc_host) HIPCHK(hipHostMalloc(&s->dsc_host, sizeof(TsxDirScalars), hipHostMallocDefault));
  TsxDirScalars *dh = (TsxDirScalars *)s->dsc_host, *dd = (TsxDirScalars *)s->dsc;
  memset(dh, 0, sizeof(*dh));
  // determine_ksp_tolerances on C_dir (glob_zm = Nz+1) and explicit_edir's default_max_it (+2: complete initial run);
  // the caller's -solar_dir_ksp_rtol / _atol / _max_it (tsx_pprts_set_direct_tolerances) as explicit_edir reads them
  // (src/pprts_explicit.F90:94-121): the first solve of a uid never runs looser than the defaults
  const double rt_def = 1e-5, at_def = fmax(1e-8, 1e-4 * (double)s->grid.glob_xm * s->grid.glob_ym * (g.Nz + 1));
  dh->rtol = s->dir_rtol > 0 ? (first_of_uid ? fmin(s->dir_rtol, rt_def) : s->dir_rtol) : rt_def;
  dh->atol = s->dir_atol > 0 ? (first_of_uid ? fmin(s->dir_atol, at_def) : s->dir_atol) : at_def;
  dh->maxit = s->dir_maxit > 0 && !first_of_uid ? s->dir_maxit : 1002;
  HIPCHK(hipMemcpyAsync(dd, dh, sizeof(*dh), hipMemcpyHostToDevice, s->stream));
  const double inc = edirTOA * s->opt_dx * s->opt_dy / (double)dir_top_div(s);  // setup_incSolar: / dirtop%area_divider
  // tiled sweep (tsx_k_edir_sweep_tiled, the default): a wave per 8 x 8 columns, the beam crosses a tile per sweep instead of a
  // column; TSX_EDIR_TILED=0: one thread per column (the round-1 kernel)
  const char *te = getenv("TSX_EDIR_TILED");  // read per call: tests switch it
  const bool tiled = !(te && atoi(te) == 0);
  const int tiles_x = (g.xm + 7) / 8, tiles_y = (g.ym + 7) / 8;
  const int nb = tiled ? tiles_x * tiles_y : (g.ncol + 63) / 64;
  const int batch = tiled ? 3 : 8;  // sweeps between two looks at the stop flag
  if (nb > TSX_MAX_PARTIAL_BLOCKS * TSX_NSLOTS - 64) {
    tsx_set_error("tsx_pprts_solve: too many columns for the partial buffer");
    return TSX_ERR_UNSUPPORTED;
  }
  // several ranks: one face exchange (exchange_direct_boundary) + unpack per sweep, residual = mean over ranks of the
  // local norms (imp_allreduce_mean, src/pprts_explicit.F90:184)
  const bool multi = !(g.wrap_x && g.wrap_y);
  TsxDirHalo hb;
  if ((rc = dir_halo(s, &hb))) return rc;
  const size_t cx = (size_t)DSIDE * g.Nz * g.ym, cy = (size_t)DSIDE * g.Nz * g.xm;
  const int nbu = multi ? grid_for((long long)(cx + cy), 64) : 0;
  const int nranks = s->grid.nranks > 1 ? s->grid.nranks : 1;
  bool done = false;
  TsxLogScope log_sweeps(s, TSX_EV_SOLVE_MDIR);  // solve_Mdir, src/pprts.F90:2903-2912 (here: explicit_edir's sweeps)
  while (!done) {
    for (int q = 0; q < batch; ++q) {
      if (tiled)
        hipLaunchKernelGGL((tsx_k_edir_sweep_tiled<DTOP, DSIDE>), dim3(nb), dim3(64), 0, s->stream, g, sun, s->dirT, s->l1d, s->a33,
                           inc, s->edir_a, s->edir_b, s->partials, &dd->done, hb, tiles_x);
      else
        hipLaunchKernelGGL((tsx_k_edir_sweep<DTOP, DSIDE>), dim3(nb), dim3(64), 0, s->stream, g, sun, s->dirT, s->l1d, s->a33, inc,
                           s->edir_a, s->edir_b, s->partials, &dd->done, hb);
      if (multi) {
        if ((rc = tsx_face_exchange_bufs(s, s->stream, s->dsend, s->drecv, cx, cy))) return rc;
        hipLaunchKernelGGL((tsx_k_edir_unpack<DTOP, DSIDE>), dim3(nbu), dim3(TSX_BLOCK), 0, s->stream, g, sun, s->l1d, s->edir_a, s->edir_b,
                           hb, s->partials + nb, &dd->done);
      }
      if (nranks > 1) {
        hipLaunchKernelGGL(tsx_k_edir_scalar, dim3(1), dim3(1024), 0, s->stream, dd, s->partials, nb + nbu, 1, 1.0);
        if ((rc = tsx_allreduce_dev1(s, &dd->res))) return rc;
        hipLaunchKernelGGL(tsx_k_edir_scalar, dim3(1), dim3(1024), 0, s->stream, dd, s->partials, nb + nbu, 2, 1.0 / nranks);
      } else {
        hipLaunchKernelGGL(tsx_k_edir_scalar, dim3(1), dim3(1024), 0, s->stream, dd, s->partials, nb + nbu, 3, 1.0);
      }
      // ping-pong: after a converged sweep `done` freezes further sweeps, so track which buffer is current on the host
      std::swap(s->edir_a, s->edir_b);
    }
    HIPCHK(hipMemcpyAsync(dh, dd, sizeof(*dh), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    done = dh->done != 0;
  }
  // the last *executed* sweep wrote into the buffer that was `edir_b` at sweep number dh->iter; sweeps after `done`
  // were no-ops but the host kept swapping: recover the right buffer from the parity of skipped sweeps
  {
    static_assert(true, "");
    const int launched = ((dh->iter + batch - 1) / batch) * batch;
    if ((launched - dh->iter) & 1) std::swap(s->edir_a, s->edir_b);
  }
  s->niter_dir = dh->iter;
  if (!dh->converged && strict) {
    tsx_set_error("tsx_pprts_solve: direct sweep did not converge");
    return TSX_ERR_STATE;
  }
  (void)rc;
  return TSX_OK;
}

template <int NTOP, int NSIDE, int DTOP, int DSIDE>
static int pprts_solve_t(tsx_solver *s, double edirTOA, int lsolar, const tsx_ksp_opts *opts, tsx_ksp_result *res) {
  int rc;
  if (!s->have_optprop) {
    tsx_set_error("tsx_pprts_solve: call tsx_pprts_set_optprop first");
    return TSX_ERR_STATE;
  }
  ARGCHK(lsolar || s->planck, "tsx_pprts_solve: thermal solve needs planck in tsx_pprts_set_optprop");
  tsx_ksp_opts o;
  const bool first_solve = !s->have_solution || s->guess_foreign || s->last_lsolar != lsolar;
  if (opts) {
    if ((rc = tsx_prepare_ksp(s, opts, &o))) return rc;
    // -ksp_complete_initial_run (default on, src/pprts.F90:4245-4256): the first solve of a solution uid never runs with
    // looser tolerances than determine_ksp_tolerances gives, whatever the caller set for the later (warm-started) ones
    const bool first_of_uid = !s->have_solution || s->guess_foreign || s->last_lsolar != lsolar;
    if (first_of_uid && !opts->skip_complete_initial_run) {
      double rt, at;
      int32_t mx;
      tsx_determine_ksp_tolerances(s, tsx_unconstrained_fraction(s), &rt, &at, &mx);
      o.rtol = fmin(o.rtol, rt);
      o.atol = fmin(o.atol, at);
      o.maxit = o.maxit > mx ? o.maxit : mx;
    }
  } else {  // reference defaults: determine_ksp_tolerances + this back-end's default preconditioner
    tsx_ksp_opts d;
    tsx_default_ksp_opts(&d);
    int32_t mx;
    tsx_determine_ksp_tolerances(s, tsx_unconstrained_fraction(s), &d.rtol, &d.atol, &mx);
    d.maxit = mx;
    d.pc = TSX_PC_REDBLACK;
    d.pc_sweeps = 0;  // automatic, see tsx_prepare_ksp
    if ((rc = tsx_prepare_ksp(s, &d, &o))) return rc;
  }
  const TsxGeo &g = s->geo;
  const TsxSun sun = make_sun(s);
  if (s->have_solution && s->last_lsolar != lsolar && !s->guess_foreign) {
    // same uid, other kind of radiation: the reference destroys the solution and starts from zero
    // (solution%lsolar_rad .neqv. derived_lsolar, src/pprts.F90:2585-2590); a guess taken over from the previous uid is
    // kept whatever its kind (:2540-2552)
    if ((rc = tsx_pprts_zero_guess(s))) return rc;
  }
  s->guess_foreign = false;
  TsxDirHalo hb;
  if ((rc = dir_halo(s, &hb))) return rc;
  if (lsolar && (rc = direct_solve<NTOP, NSIDE, DTOP, DSIDE>(s, edirTOA, first_solve))) return rc;
  TsxLogScope log_ediff(s, TSX_EV_COMPUTE_EDIFF);  // compute_Ediff, src/pprts.F90:2760-2818: setup_b + the diffuse solve
  {
  TsxLogScope log_src(s, TSX_EV_SETUP_DIFF_SRC);  // setup_diff_src (setup_b, :4641-4987)
  if (lsolar) {
    hipLaunchKernelGGL((tsx_k_setup_b_solar<NTOP, NSIDE, DTOP, DSIDE>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g, sun, s->dirS,
                       s->l1d, s->a13, s->a23, s->albedo, s->edir_a, s->vb, hb);
  } else {
    // the blocks' column sums per distinct block, where blocks are shared (built here already: the solve needs them anyway)
    if ((rc = tsx_dedup_ensure(s))) return rc;
    const double *cs = s->dd_on ? s->dd_colsum : (const double *)nullptr;
    const double *cB = s->collapse > 1 && s->ca_have_B ? s->ca_B : (const double *)nullptr;  // layer 0 of a collapsed atmosphere
    if (s->coef_bytes == 4)
      hipLaunchKernelGGL((tsx_k_setup_b_thermal<NTOP, NSIDE, float>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g,
                         (const float *)s->coef, s->l1d, s->a11, s->a12, s->albedo, s->planck, s->bsrfc, s->d_kabs, s->d_dz, s->opt_dx,
                         s->opt_dy, s->vb, cs, s->dd_cidx, (long long)s->dd_nent, cB);
    else
      hipLaunchKernelGGL((tsx_k_setup_b_thermal<NTOP, NSIDE, double>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g,
                         (const double *)s->coef, s->l1d, s->a11, s->a12, s->albedo, s->planck, s->bsrfc, s->d_kabs, s->d_dz, s->opt_dx,
                         s->opt_dy, s->vb, (const double *)nullptr, (const int *)nullptr, 0ll, cB);
  }
  HIPCHK(hipGetLastError());
  // buildings: set_buildings_reflection / set_buildings_emission overwrite the faces' leaving dofs (src/pprts.F90:4669-4672)
  if (s->bld_nfaces > 0 && (rc = tsx_buildings_source(s, lsolar))) return rc;
  }
  s->last_lsolar = lsolar;
  // b_norm = sum |b| < atol -> skip the diffuse solve, ediff = b (src/pprts.F90:2773-2784)
  const int nbv = grid_for(g.N);
  hipLaunchKernelGGL(tsx_k_asum, dim3(nbv), dim3(TSX_BLOCK), 0, s->stream, g.N, s->vb, s->partials);
  std::vector<double> part(nbv);
  HIPCHK(hipMemcpyAsync(part.data(), s->partials, sizeof(double) * nbv, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  double bnorm = 0;
  for (double v : part) bnorm += v;
  if ((rc = tsx_allreduce_host(s, &bnorm, 1))) return rc;  // VecNorm(b, NORM_1) is global
  if (bnorm < o.atol) {
    s->x_is_zero = false;
    HIPCHK(hipMemcpyAsync(s->vx, s->vb, sizeof(double) * g.N, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (res) {
      memset(res, 0, sizeof(*res));
      res->reason = 3;
      res->res_hist[0] = o.atol;
      res->nhist = 1;
    }
  } else {
    tsx_debug_checkpoint(s, lsolar ? "solar_before_solve" : "thermal_before_solve");
    if ((rc = tsx_krylov_run_with_retry(s, &o))) return rc;
    tsx_debug_checkpoint(s, lsolar ? "solar_after_solve" : "thermal_after_solve");
    HIPCHK(hipStreamSynchronize(s->stream));
    if ((rc = tsx_fill_result(s, res))) return rc;
  }
  s->have_solution = true;
  s->x_is_zero = false;  // whatever path ran, vx is a solution now: only tsx_pprts_zero_guess / the retry may set the flag
  return TSX_OK;
}

extern "C" int tsx_pprts_solve(tsx_solver *s, double edirTOA, int lsolar, const tsx_ksp_opts *opts, tsx_ksp_result *res) {
  ARGCHK(s, "tsx_pprts_solve: null");
  if (s->mode_1d) {  // class is (t_solver_2str), src/pprts.F90:2627-2638
    if (!s->have_optprop) {
      tsx_set_error("tsx_pprts_solve: call tsx_pprts_set_optical_properties first");
      return TSX_ERR_STATE;
    }
    HIPCHK(hipSetDevice(s->device));
    const int schwarz = s->mode_1d == TSX_1D_SCHWARZSCHILD && !lsolar;
    hipEvent_t e0 = s->ev0, e1 = s->ev1;
    HIPCHK(hipEventRecord(e0, s->stream));
    {
      TsxLogScope log_scope(s, schwarz ? TSX_EV_SOLVE_SCHWARZSCHILD : TSX_EV_SOLVE_TWOSTREAM);
      int rc = tsx_1d_run(s, edirTOA, lsolar, schwarz);
      if (rc) return rc;
    }
    HIPCHK(hipEventRecord(e1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->last_lsolar = lsolar;
    s->have_solution = s->sol_is_1d = true;
    s->guess_foreign = false;
    if (res) {
      memset(res, 0, sizeof(*res));
      res->reason = schwarz ? TSX_REASON_1D_SCHWARZSCHILD : TSX_REASON_1D_TWOSTREAM;
      float ms = 0;
      if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) res->solve_ms = ms;
    }
    return TSX_OK;
  }
  return PIPE_CALL(pprts_solve_t, s, edirTOA, lsolar, opts, res);
}

template <int NTOP, int NSIDE, int DTOP, int DSIDE>
static int pprts_get_result_t(tsx_solver *s, double *edn, double *eup, double *abso, double *edir, int where) {
  int rc;
  if (!s->have_solution) {
    tsx_set_error("tsx_pprts_get_result: no solution (call tsx_pprts_solve)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  const TsxSun sun = make_sun(s);
  const size_t nl = (size_t)(g.Nz + 1) * g.ncol, nc = (size_t)g.Nc;
  double *d_dn = edn, *d_up = eup, *d_ab = abso, *d_di = edir;
  TsxDevTmp tmp_guard;
  double *tmp = nullptr;
  if (where == TSX_HOST) {
    HIPCHK(tmp_guard.alloc(sizeof(double) * (3 * nl + nc)));
    tmp = tmp_guard.as<double>();
    d_dn = tmp;
    d_up = tmp + nl;
    d_di = edir ? tmp + 2 * nl : nullptr;
    d_ab = tmp + 3 * nl;
  }
  const int lsolar = s->last_lsolar;
  TsxDirHalo hb;
  if ((rc = dir_halo(s, &hb))) return rc;
  tsx_debug_checkpoint(s, lsolar ? "solar_get_result" : "thermal_get_result");
  TsxLogScope log_res(s, TSX_EV_GET_RESULT);  // get_result (pprts_get_result, src/pprts.F90:5799-5888), the absorption inside it
  {
  TsxLogScope log_abso(s, TSX_EV_COMPUTE_ABSORPTION);  // compute_absorption (calc_flx_div, :5197-5479)
  // the diffuse streams entering through rank faces: one halo update of the solution, as before an operator apply
  if (!(g.wrap_x && g.wrap_y) && (rc = halo_update<NTOP, NSIDE>(s, s->vx, false))) return rc;
  if (s->coef_bytes == 4)
    hipLaunchKernelGGL((tsx_k_flx_div<NTOP, NSIDE, DTOP, DSIDE, float>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g, sun, lsolar,
                       !lsolar, (const float *)s->coef, s->dirT, s->dirS, s->l1d, s->a11, s->a12, s->d_kabs, s->d_dz, s->opt_dx,
                       s->opt_dy, s->edir_a, s->vx, s->vb, d_ab, hb, s->recvW, s->recvE, s->recvS, s->recvN,
                       s->dd_on && s->dd_valid ? s->dd_colsum : (const double *)nullptr, s->dd_cidx, (long long)s->dd_nent);
  else
    hipLaunchKernelGGL((tsx_k_flx_div<NTOP, NSIDE, DTOP, DSIDE, double>), dim3(grid_for(g.Nc)), dim3(TSX_BLOCK), 0, s->stream, g, sun, lsolar,
                       !lsolar, (const double *)s->coef, s->dirT, s->dirS, s->l1d, s->a11, s->a12, s->d_kabs, s->d_dz, s->opt_dx,
                       s->opt_dy, s->edir_a, s->vx, s->vb, d_ab, hb, s->recvW, s->recvE, s->recvS, s->recvN, (const double *)nullptr,
                       (const int *)nullptr, 0ll);
  }
  hipLaunchKernelGGL((tsx_k_get_result<NTOP, NSIDE, DTOP, DSIDE>), dim3((g.ncol + 31) / 32, (g.Nz + 1 + 31) / 32), dim3(TSX_BLOCK), 0, s->stream, g, sun,
                     lsolar, s->opt_dx, s->opt_dy, dir_top_div(s), s->edir_a, s->vx, d_di, d_dn, d_up, d_ab);
  HIPCHK(hipGetLastError());
  // -pprts_set_abso_in_buildings (src/pprts.F90:5986-6009).  The reference overwrites solution%abso behind the copy into rabso
  // (:5881, 5909), so there the value shows in the dump and from the next pprts_get_result on; here it is in the array returned
  if (s->bld_nfaces > 0 && s->bld_abso_on && (rc = tsx_buildings_abso(s, d_ab))) return rc;
  if (where == TSX_HOST) {
    HIPCHK(hipMemcpyAsync(edn, d_dn, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(eup, d_up, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
    if (edir) HIPCHK(hipMemcpyAsync(edir, d_di, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(abso, d_ab, sizeof(double) * nc, hipMemcpyDeviceToHost, s->stream));
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}

extern "C" int tsx_pprts_get_result(tsx_solver *s, double *edn, double *eup, double *abso, double *edir, int where) {
  ARGCHK(s && edn && eup && abso, "tsx_pprts_get_result: null argument");
  if (s->have_solution && s->sol_is_1d) {
    // a 1-D solution is lWm2 = .true. and lchanged = .false. (src/pprts_1D_solvers.F90:241-245): restore_solution neither scales
    // it nor computes a flux divergence; pprts_get_result's `* sun%mu` (src/pprts.F90:5883-5888) applies
    HIPCHK(hipSetDevice(s->device));
    const TsxGeo &g = s->geo;
    const size_t nl = (size_t)(g.Nz + 1) * g.ncol, nc = (size_t)g.Nc;
    double *d_dn = edn, *d_up = eup, *d_ab = abso, *d_di = edir;
    TsxDevTmp tmp_guard;
    if (where == TSX_HOST) {
      HIPCHK(tmp_guard.alloc(sizeof(double) * (3 * nl + nc)));
      double *tmp = tmp_guard.as<double>();
      d_dn = tmp, d_up = tmp + nl, d_di = edir ? tmp + 2 * nl : nullptr, d_ab = tmp + 3 * nl;
    }
    TsxLogScope log_res(s, TSX_EV_GET_RESULT);
    int rc = tsx_1d_result(s, s->last_lsolar, d_dn, d_up, d_ab, d_di);
    if (rc) return rc;
    if (where == TSX_HOST) {
      HIPCHK(hipMemcpyAsync(edn, d_dn, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
      HIPCHK(hipMemcpyAsync(eup, d_up, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
      if (edir) HIPCHK(hipMemcpyAsync(edir, d_di, sizeof(double) * nl, hipMemcpyDeviceToHost, s->stream));
      HIPCHK(hipMemcpyAsync(abso, d_ab, sizeof(double) * nc, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return TSX_OK;
  }
  if (s->mode_1d && !s->have_solution) {
    tsx_set_error("tsx_pprts_get_result: no solution (call tsx_pprts_solve)");
    return TSX_ERR_STATE;
  }
  return PIPE_CALL(pprts_get_result_t, s, edn, eup, abso, edir, where);
}

// planes [nv][ (k*ym+j)*xm + i ] over `nlev` levels -> reference layout (v fastest, then k, i, j)
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_planes_to_ref(int nv, int nlev, int xm, int ym, const double *__restrict__ p,
                                                                 double *__restrict__ ref) {
  const long long ncl = (long long)nlev * xm * ym, total = ncl * nv;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * TSX_BLOCK) {
    const long long c = q % ncl;
    const int v = (int)(q / ncl);
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    ref[(size_t)v + (size_t)nv * ((size_t)k + (size_t)nlev * ((size_t)i + (size_t)xm * j))] = p[q];
  }
}
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_fplanes_to_ref(int nv, int nlev, int xm, int ym, const float *__restrict__ p,
                                                                  double *__restrict__ ref) {
  const long long ncl = (long long)nlev * xm * ym, total = ncl * nv;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * TSX_BLOCK) {
    const long long c = q % ncl;
    const int v = (int)(q / ncl);
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    ref[(size_t)v + (size_t)nv * ((size_t)k + (size_t)nlev * ((size_t)i + (size_t)xm * j))] = (double)p[q];
  }
}

// cell order (i fastest) -> reference layout (k fastest); cells of layers that hold no value (3-D layers for the Eddington
// coefficients) come out as NaN
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_export_cellfield(TsxGeo g, const double *__restrict__ cell, const uint8_t *__restrict__ l1d,
                                                                    double *__restrict__ ref) {
  const int xm = g.xm, ym = g.ym, Nz = g.Nz;
  for (long long c = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; c < g.Nc; c += (long long)gridDim.x * TSX_BLOCK) {
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    ref[(size_t)k + (size_t)Nz * ((size_t)i + (size_t)xm * j)] = l1d[k] ? cell[c] : __longlong_as_double(0x7ff8000000000000ll);
  }
}

extern "C" int tsx_pprts_get_field(tsx_solver *s, int which, double *out, int where) {
  ARGCHK(s && out, "tsx_pprts_get_field: null");
  ARGCHK(which >= 0 && which <= 14, "tsx_pprts_get_field: which must be 0..14");
  if (which >= 13) {  // atm%Btop / atm%Bbot of a collapsed atmosphere (src/pprts.F90:2192-2196), (xs:xe, ys:ye); NaN without them
    HIPCHK(hipSetDevice(s->device));
    const size_t nb = sizeof(double) * (size_t)s->geo.ncol;
    if (s->collapse > 1 && s->ca_have_B && s->have_optprop && !s->mode_1d) {
      HIPCHK(hipMemcpyAsync(out, s->ca_B + (which == 14 ? s->geo.ncol : 0), nb,
                            where == TSX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s->stream));
    } else if (where == TSX_HOST) {
      std::vector<double> nan((size_t)s->geo.ncol, std::numeric_limits<double>::quiet_NaN());
      memcpy(out, nan.data(), nb);
    } else {
      HIPCHK(hipMemsetAsync(out, 0xff, nb, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return TSX_OK;
  }
  if (which >= 5) {  // what set_optical_properties derived on the device: delta-scaled properties, Eddington coefficients
    HIPCHK(hipSetDevice(s->device));
    const TsxGeo &gq = s->geo;
    if (!s->have_optprop || !s->d_kabs) {
      tsx_set_error("tsx_pprts_get_field: no optical properties (tsx_pprts_set_optical_properties)");
      return TSX_ERR_STATE;
    }
    const size_t nb = sizeof(double) * (size_t)gq.Nc;
    if (which <= 7) {
      const double *src = which == 5 ? s->d_kabs : (which == 6 ? s->d_ksca : s->d_g);
      HIPCHK(hipMemcpyAsync(out, src, nb, where == TSX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s->stream));
      HIPCHK(hipStreamSynchronize(s->stream));
      return TSX_OK;
    }
    const double *cellf[5] = {s->a11, s->a12, s->a13, s->a23, s->a33};
    const double *cf = cellf[which - 8];
    TsxDevTmp tmpq;
    double *devq = out;
    if (where == TSX_HOST) {
      HIPCHK(tmpq.alloc(nb));
      devq = tmpq.as<double>();
    }
    if (!s->any_l1d || !cf) {
      std::vector<uint8_t> none;  // no 1-D layer: every cell NaN
      HIPCHK(hipMemsetAsync(devq, 0xff, nb, s->stream));
    } else {
      hipLaunchKernelGGL(tsx_k_export_cellfield, dim3(grid_for(gq.Nc)), dim3(TSX_BLOCK), 0, s->stream, gq, cf, s->l1d, devq);
      HIPCHK(hipGetLastError());
    }
    if (where == TSX_HOST) HIPCHK(hipMemcpyAsync(out, devq, nb, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return TSX_OK;
  }
  int rc = pipeline_guard(s, "tsx_pprts_get_field");
  if (rc) return rc;
  if (s->mode_1d) {  // a 1-D solution has no stream vectors, no source vector and no direct coefficients
    tsx_set_error("tsx_pprts_get_field: fields 0..4 do not exist on a handle with a 1-D solver (tsx_pprts_set_1d_solver)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  const TsxGeo &g = s->geo;
  size_t n = 0;
  const int S = dir_streams(s);
  if (which == 0) n = (size_t)S * (g.Nz + 1) * g.ncol;
  else if (which == 1 || which == 2) n = (size_t)g.N;
  else if (which == 3) n = (size_t)S * S * g.Nc;
  else n = (size_t)S * g.D * g.Nc;
  double *dev = out;
  TsxDevTmp tmp_guard;
  double *tmp = nullptr;
  if (where == TSX_HOST) {
    HIPCHK(tmp_guard.alloc(n * sizeof(double)));
    tmp = tmp_guard.as<double>();
    dev = tmp;
  }
  if (which == 0) {
    ARGCHK(s->edir_a, "tsx_pprts_get_field: no direct solution");
    hipLaunchKernelGGL(tsx_k_planes_to_ref, dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, S, g.Nz + 1, g.xm, g.ym,
                       s->edir_a, dev);
  } else if (which == 1 || which == 2) {
    if ((rc = tsx_export_vec(s, which == 1 ? s->vb : s->vx, dev))) return rc;
  } else if (which == 3) {
    ARGCHK(s->dirT && s->dir_coeffs_valid, "tsx_pprts_get_field: no direct coefficients");
    hipLaunchKernelGGL(tsx_k_fplanes_to_ref, dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, S * S, g.Nz, g.xm, g.ym,
                       s->dirT, dev);
  } else {
    ARGCHK(s->dirS && s->dir_coeffs_valid, "tsx_pprts_get_field: no direct coefficients");
    hipLaunchKernelGGL(tsx_k_fplanes_to_ref, dim3(grid_for((long long)n)), dim3(TSX_BLOCK), 0, s->stream, S * g.D, g.Nz, g.xm, g.ym,
                       s->dirS, dev);
  }
  HIPCHK(hipGetLastError());
  if (where == TSX_HOST) HIPCHK(hipMemcpyAsync(out, dev, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}


// ---- pprts_f2c_opp_*: coefficient probe (c_wrapper/f2c_pprts.h:54-83)
extern "C" int tsx_opp_get_coeff(tsx_solver *s, float tauz, float w0, float g, float aspect_zx, float phi, float theta,
                                 int imode, int lswitch_east, int lswitch_north, int ncoeff, float *coeff) {
  ARGCHK(s && coeff, "tsx_opp_get_coeff: null argument");
  ARGCHK(imode >= 1 && imode <= 3, "tsx_opp_get_coeff: imode must be 1 (dir2dir), 2 (dir2diff) or 3 (diff2diff)");
  const TsxLutHost &H = imode == 1 ? s->lut_T : (imode == 2 ? s->lut_S : s->lut_diff);
  if (!H.ready) {
    tsx_set_error("tsx_opp_get_coeff: the table for this imode is not loaded");
    return TSX_ERR_STATE;
  }
  ARGCHK(ncoeff == H.nvec, "tsx_opp_get_coeff: Ncoeff differs from the table's coefficient count");
  HIPCHK(hipSetDevice(s->device));
  TsxDevTmp out;
  HIPCHK(out.alloc(sizeof(float) * (size_t)H.nvec));
  const int S = dir_streams(s);
  if (imode == 3)
    hipLaunchKernelGGL((tsx_k_opp_point<4>), dim3(1), dim3(64), 0, s->stream, lut_dev(H), tauz, w0, g, aspect_zx, 0.0f, 0.0f, S, 0, 0,
                       0, out.as<float>());
  else
    hipLaunchKernelGGL((tsx_k_opp_point<6>), dim3(1), dim3(64), 0, s->stream, lut_dev(H), tauz, w0, g, aspect_zx, phi, theta, S,
                       imode == 2, lswitch_east != 0, lswitch_north != 0, out.as<float>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(coeff, out.p, sizeof(float) * (size_t)H.nvec, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}

// pprts_f2c_opp_get_info: stream counts and the [min, max] of every table axis; ranges[0..3] = diffuse tau, w0, g,
// aspect_zx; ranges[4..9] = direct tau, w0, g, aspect_zx, phi, theta
extern "C" int tsx_opp_get_info(tsx_solver *s, int32_t *Ndir, int32_t *Ndiff, float *ranges20) {
  ARGCHK(s && Ndir && Ndiff && ranges20, "tsx_opp_get_info: null argument");
  *Ndir = dir_streams(s);
  *Ndiff = s->geo.D;
  HIPCHK(hipSetDevice(s->device));
  auto axis_range = [&](const TsxLutHost &H, int dim, float *r) -> int {
    r[0] = r[1] = 0.0f;
    if (!H.ready) return TSX_OK;
    int off = 0;
    for (int d = 0; d < dim; ++d) off += H.n[d];
    HIPCHK(hipMemcpy(&r[0], H.d_axes + off, sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&r[1], H.d_axes + off + H.n[dim] - 1, sizeof(float), hipMemcpyDeviceToHost));
    return TSX_OK;
  };
  // table axis order: tau, w0, aspect_zx, g (, phi, theta); reported order: tau, w0, g, aspect_zx (, phi, theta)
  const int order[6] = {0, 1, 3, 2, 4, 5};
  int rc;
  for (int q = 0; q < 4; ++q)
    if ((rc = axis_range(s->lut_diff, order[q], ranges20 + 2 * q))) return rc;
  for (int q = 0; q < 6; ++q)
    if ((rc = axis_range(s->lut_T, order[q], ranges20 + 8 + 2 * q))) return rc;
  return TSX_OK;
}

// ================================================================================================
// the seam-level entries beside tsx_diff_*:
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
static int seam_cellfield(tsx_solver *s, double **dst, const double *src, int where) { return tsx_keep_cellfield(s, dst, src, where); }

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
  return tsx_export_vec(s, s->vb, b_dev);
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
  return tsx_export_vec(s, s->vb, b_dev);
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

TSX_CODE_PROBE(pipeline)  // tsx_host.hpp: this unit's code object as it sits in device memory (diagnostics)
