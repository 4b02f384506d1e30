// tsx_buildings.hip -- buildings in the whole-g-point pipeline: opaque, diffusely reflecting, emitting cell faces
// (opt_buildings of solve_pprts / pprts_get_result; t_pprts_buildings, src/buildings.F90:39-74).
//
// A building is a list of cell faces iface(m): the reference's 1-based linear index over [face_id, k, i, j] with sizes
// [6, Nz, xm, ym], first dimension fastest (faceidx_by_cell_plus_offset, src/buildings.F90:217-222; ind_1d_to_nd,
// src/helper_functions.fypp:2392-2414); face ids 1..6 = TOP, BOT, LEFT, RIGHT, REAR, FRONT (src/boxmc_geometry.F90:46-51), stored
// here as 0..5.  What the reference does with them, and where it happens here:
//   dir2dir   (src/pprts.F90:3194-3212)        the whole block of a cell that owns a face -> 0            tsx_k_bld_zero_dir
//   diff2diff (:3579-3677)                     per face: every coefficient into the dofs that LEAVE the cell through it -> 0, the
//                                              ones from the dofs entering through it -> albedo / streams  tsx_k_bld_patch_diffuse
//   setup_b   (:4989-5145)                     per face the source of the leaving dofs is overwritten      tsx_k_bld_source
//   results   (:6011-6247 fill_buildings_arr)  per face edir, incoming, outgoing in W/m2                   tsx_k_bld_results
//   -pprts_set_abso_in_buildings (:5986-6009)                                                              tsx_k_bld_abso
//
// Storage.  An unknown is stored at the cell whose block writes it (tsx_internal.hpp), and the dofs that leave a cell through a
// face are exactly the ones that cell writes: TOP -> the upward top dofs at level k, BOT -> the downward ones at level k + 1,
// LEFT / REAR -> the side dofs pointing to lower i / j at (i, j), RIGHT / FRONT -> the ones pointing to higher i / j at i + 1 /
// j + 1.  So every patched coefficient column and every overwritten source entry of a face of cell c sits at index c; only what
// ENTERS through a face (and the direct beam, which is stored on the column it sits on) is read from a neighbour.
//
// fp64 except the stored coefficients (the blocks are fp32: the reflected entry is float(albedo / streams)).  One pool allocation,
// grow-only, freed in tsx_destroy; every word a kernel reads is written by the decode before (correct on recycled memory,
// TSX_POOL_POISON).  No per-lane arrays: nothing spills to scratch memory (profiles/r07/buildings_resource_usage.txt).
#include <string.h>

#include <algorithm>
#include <vector>

#include "tsx_host.hpp"

struct TsxBuildings {
  std::vector<long long> iface;  // the attached face list as handed over (a changed list is what triggers a new decode)
  std::vector<int> face_k;       // layer of every face, 0-based (the 1-D layer check of tsx_pprts_set_optical_properties)
  int ncells = 0;                // distinct cells that own a face
  bool have_planck = false;
  size_t cap = 0;                // faces the device allocation holds
  char *dev = nullptr;
  // slices of dev
  long long *d_iface = nullptr;  // [cap]
  int4 *d_ftup = nullptr;        // [cap] (face 0..5, k, i, j), 0-based
  int *d_fslot = nullptr;        // [cap] the face's cell record
  double *d_falb = nullptr;      // [cap]
  double *d_fplk = nullptr;      // [cap]
  double *d_out = nullptr;       // [3][cap] staging of tsx_pprts_get_buildings for host callers
  int *d_ccell = nullptr;        // [cap] cell records: cell index (k * ym + j) * xm + i ...
  unsigned *d_cmask = nullptr;   // [cap] ... 6-bit face mask ...
  double *d_calb = nullptr;      // [cap][6] ... and the six albedos
};

namespace {
constexpr double BLD_PI = 3.14159265358979323846;

// the face a destination dof leaves its cell through (is_inward = [F, T, ...] on every face group, tsx_inward)
template <int NTOP, int NSIDE>
__device__ __forceinline__ int bld_face_of_dst(int d) {
  if (d < NTOP) return tsx_inward(d) ? 1 : 0;
  if (d < NTOP + NSIDE) return tsx_inward(d - NTOP) ? 3 : 2;
  return tsx_inward(d - NTOP - NSIDE) ? 5 : 4;
}

// one lane per face: iface -> (face, k, i, j); the face's cell record gets the cell index and the face's bit.  Faces of one cell
// store the same cell index (benign) and OR their bits in; cmask was zeroed before the launch.
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_decode(TsxGeo g, int nfaces, const long long *__restrict__ iface,
                                                              const int *__restrict__ fslot, int4 *__restrict__ ftup,
                                                              int *__restrict__ ccell, unsigned *__restrict__ cmask) {
  const int m = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (m >= nfaces) return;
  long long r = iface[m] - 1;  // ind_1d_to_nd, 1-based
  const int f = (int)(r % 6);
  r /= 6;
  const int k = (int)(r % g.Nz);
  r /= g.Nz;
  const int i = (int)(r % g.xm);
  const int j = (int)(r / g.xm);
  ftup[m] = make_int4(f, k, i, j);
  const int slot = fslot[m];
  ccell[slot] = (k * g.ym + j) * g.xm + i;
  atomicOr(&cmask[slot], 1u << f);
}
// one lane per face: the albedo into its cell record (calb was zeroed before the launch: faces not listed hold 0)
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_albedo(int nfaces, const int4 *__restrict__ ftup, const int *__restrict__ fslot,
                                                              const double *__restrict__ falb, double *__restrict__ calb) {
  const int m = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (m >= nfaces) return;
  calb[(size_t)fslot[m] * 6 + ftup[m].x] = falb[m];
}

// set_buildings_coeff of alloc_coeff_diff2diff (src/pprts.F90:3579-3677): a wave per building cell, lane d = destination dof.
// The column of a dof that leaves through a listed face becomes 0, except from the dofs entering through the same face:
// albedo / streams.  Faces of one cell touch disjoint columns.  Then lane 0 hashes the patched block with the functions the
// lookup kernel uses (tsx_k_lut_diff2diff), so that building cells with equal blocks still share an entry and no stale hash pairs
// a patched block with an unpatched one (tsx_dedup.hip compares exactly in any case).
template <int NTOP, int NSIDE>
__global__ __launch_bounds__(64) void tsx_k_bld_patch_diffuse(long long Nc, int ncells, const int *__restrict__ ccell,
                                                              const unsigned *__restrict__ cmask, const double *__restrict__ calb,
                                                              float *C, unsigned long long *hash) {
  constexpr int D = NTOP + 2 * NSIDE;
  static_assert(D <= 64, "one lane per destination dof");
  const int r = blockIdx.x;
  if (r >= ncells) return;
  const long long c = ccell[r];
  const unsigned mask = cmask[r];
  const int d = threadIdx.x;
  if (d < D) {
    const int f = bld_face_of_dst<NTOP, NSIDE>(d);
    if (mask & (1u << f)) {
      const int lo = f < 2 ? 0 : (f < 4 ? NTOP : NTOP + NSIDE), n = f < 2 ? NTOP : NSIDE;
      const float refl = (float)(calb[(size_t)r * 6 + f] / (double)(n / 2));  // difftop%streams / diffside%streams = dof / 2
      for (int s = 0; s < D; ++s) {
        const bool same_face = s >= lo && s < lo + n;
        C[(size_t)(d * D + s) * Nc + c] = (same_face && tsx_inward(s - lo) != tsx_inward(d - lo)) ? refl : 0.0f;
      }
    }
  }
  __syncthreads();  // the block's stores are visible to lane 0
  if (hash && d == 0) {
    unsigned long long hv = TSX_DD_SEED;
    for (int q = 0; q < D * D; ++q) hv = tsx_dd_hash_step(hv, q, C[(size_t)q * Nc + c]);
    hash[c] = tsx_dd_hash_final(hv);
  }
}

// set_buildings_coeff of alloc_coeff_dir2dir (src/pprts.F90:3194-3212): the dir2dir block of every building cell -> 0
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_zero_dir(long long Nc, int ncells, int SS, const int *__restrict__ ccell,
                                                                float *__restrict__ T) {
  const long long n = (long long)ncells * SS;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < n; q += (long long)gridDim.x * TSX_BLOCK) {
    const int r = (int)(q / SS), e = (int)(q - (long long)r * SS);
    T[(size_t)e * Nc + ccell[r]] = 0.0f;
  }
}

// set_buildings_reflection / set_buildings_emission (src/pprts.F90:4989-5145), one lane per face, behind tsx_k_setup_b_*.
// Solar: the leaving dofs' source = 0 + sum of the face's direct dofs * albedo / streams.  Thermal with planck:
// A_face * pi * planck * (1 - albedo) / streams, assigned.  The source of a dof leaving cell c through a face is stored at c
// (see the head of this file), also for BOT / RIGHT / FRONT whose dofs the reference addresses at k + 1 / i + 1 / j + 1.  On the
// single periodic rank i + 1 / j + 1 wrap: the reference writes the entry into its ghost column and halo_reduce_5pt adds it to
// column 0 (:4676), and that entry has no other contributor -- a dof pointing to higher i at face i + 1 is fed by cell i only.
// The direct beam is stored on the column it sits on, so ITS face index wraps here.
template <int NTOP, int NSIDE, int DTOP, int DSIDE>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_source(TsxGeo g, int nfaces, int lsolar, const int4 *__restrict__ ftup,
                                                              const double *__restrict__ falb, const double *__restrict__ fplk,
                                                              const double *__restrict__ E, const double *__restrict__ dz, double dx,
                                                              double dy, double *__restrict__ b) {
  const int m = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (m >= nfaces) return;
  const int4 t = ftup[m];
  const int f = t.x, k = t.y, i = t.z, j = t.w;
  const int xm = g.xm, ym = g.ym, ncol = g.ncol;
  const long long Nc = g.Nc, Ncl = (long long)(g.Nz + 1) * ncol;
  const size_t c = ((size_t)k * ym + j) * xm + i;
  const int lo = f < 2 ? 0 : (f < 4 ? NTOP : NTOP + NSIDE), n = f < 2 ? NTOP : NSIDE;
  const double streams = (double)(n / 2), alb = falb[m];
  const bool inward = (f & 1) != 0;  // BOT, RIGHT, FRONT: the leaving dofs are the inward ones
  double v;
  if (lsolar) {
    // where the face's direct dofs sit: level k (+ 1 for BOT), column i (+ 1 for RIGHT), row j (+ 1 for FRONT), periodic
    const int kk = f == 1 ? k + 1 : k;
    const int ii = f == 3 ? (i + 1 == xm ? 0 : i + 1) : i;
    const int jj = f == 5 ? (j + 1 == ym ? 0 : j + 1) : j;
    const size_t at = (size_t)kk * ncol + (size_t)jj * xm + ii;
    const int s0 = f < 2 ? 0 : (f < 4 ? DTOP : DTOP + DSIDE), ns = f < 2 ? DTOP : DSIDE;
    v = 0.0;
    for (int q = 0; q < ns; ++q) v += E[(size_t)(s0 + q) * Ncl + at] * alb / streams;
  } else {
    if (!fplk) return;  // no planck given: the thermal source stays as set_thermal_source left it (:5086)
    const double dzz = dz[(size_t)k + (size_t)g.Nz * ((size_t)i + (size_t)xm * j)];
    const double area = f < 2 ? dx * dy : (f < 4 ? dy * dzz : dx * dzz);  // diffuse area dividers are 1 (:250-251)
    const double emis = BLD_PI * fplk[m] * (1.0 - alb);
    v = area * emis / streams;
  }
  for (int q = 0; q < n; ++q)
    if (tsx_inward(q) == inward) b[(size_t)(lo + q) * Nc + c] = v;
}

// fill_buildings_arr (src/pprts.F90:6011-6247) without the -pprts_fill_1D_side_walls branches: one lane per face gathers from the
// solution (stored in W per stream) what restore_solution's W/m2 arrays hold at the face: every dof divided by the area of the
// face it sits on (scale_flx: Az, or dy dz / dx dz with dz of the column the REFERENCE stores the dof on, :3915-3976), the
// direct dofs by the face area / area_divider and their sum by area_divider (:6043-6064); solar results times sun%mu (:6034,
// 6119).  incoming = the dofs entering through the face, outgoing = the ones leaving (is_inward as written there).
template <int NTOP, int NSIDE, int DTOP, int DSIDE>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_results(TsxGeo g, int nfaces, int lsolar, double mu, const int4 *__restrict__ ftup,
                                                               const double *__restrict__ E, const double *__restrict__ x,
                                                               const double *__restrict__ dz, double dx, double dy,
                                                               double *__restrict__ edir, double *__restrict__ incoming,
                                                               double *__restrict__ outgoing) {
  constexpr int D = NTOP + 2 * NSIDE;
  const int m = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (m >= nfaces) return;
  const int4 t = ftup[m];
  const int f = t.x, k = t.y, i = t.z, j = t.w;
  const int xm = g.xm, ym = g.ym, Nz = g.Nz, ncol = g.ncol;
  const long long Nc = g.Nc, Ncl = (long long)(Nz + 1) * ncol;
  const double *__restrict__ xt = x + (size_t)D * Nc;
  const size_t c = ((size_t)k * ym + j) * xm + i;
  const int col = j * xm + i;
  // the column the reference stores the face's dofs on
  const int ii = f == 3 ? (i + 1 == xm ? 0 : i + 1) : i;
  const int jj = f == 5 ? (j + 1 == ym ? 0 : j + 1) : j;
  const int kk = f == 1 ? k + 1 : k;
  const double dzz = f < 2 ? 0.0 : dz[(size_t)k + (size_t)Nz * ((size_t)ii + (size_t)xm * jj)];
  const double area = f < 2 ? dx * dy : (f < 4 ? dy * dzz : dx * dzz);
  const double scale = (lsolar ? mu : 1.0) / area;
  if (edir) {
    double e = 0.0;
    if (lsolar) {
      const size_t at = (size_t)kk * ncol + (size_t)jj * xm + ii;
      const int s0 = f < 2 ? 0 : (f < 4 ? DTOP : DTOP + DSIDE), ns = f < 2 ? DTOP : DSIDE;
      for (int q = 0; q < ns; ++q) e += E[(size_t)(s0 + q) * Ncl + at];
      e *= scale;  // (E / (area / div)) summed and / div
    }
    edir[m] = e;
  }
  const int lo = f < 2 ? 0 : (f < 4 ? NTOP : NTOP + NSIDE), n = f < 2 ? NTOP : NSIDE;
  const bool leaving_inward = (f & 1) != 0;
  double in = 0.0, out = 0.0;
  for (int q = 0; q < n; ++q) {
    const int d = lo + q;
    if (tsx_inward(q) == leaving_inward) {
      out += x[(size_t)d * Nc + c];  // written by this cell
      continue;
    }
    // entering: written by the cell on the other side of the face (the tail rows at TOA / the ground)
    double v;
    if (f == 0) v = k >= 1 ? x[(size_t)d * Nc + c - ncol] : xt[(size_t)d * ncol + col];
    else if (f == 1) v = k + 1 < Nz ? x[(size_t)d * Nc + c + ncol] : xt[(size_t)d * ncol + col];
    else if (f == 2) v = x[(size_t)d * Nc + c + (i > 0 ? -1 : xm - 1)];
    else if (f == 3) v = x[(size_t)d * Nc + c + (i + 1 < xm ? 1 : -(xm - 1))];
    else if (f == 4) v = x[(size_t)d * Nc + c + (j > 0 ? -(long long)xm : (long long)(ym - 1) * xm)];
    else v = x[(size_t)d * Nc + c + (j + 1 < ym ? (long long)xm : -(long long)(ym - 1) * xm)];
    in += v;
  }
  incoming[m] = in * scale;
  outgoing[m] = out * scale;
}

// set_abso_in_buildings (src/pprts.F90:5986-6009): abso (reference layout, level fastest) of every building cell = val
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_bld_abso(TsxGeo g, int ncells, const int *__restrict__ ccell, double val,
                                                            double *__restrict__ abso) {
  const int r = blockIdx.x * TSX_BLOCK + threadIdx.x;
  if (r >= ncells) return;
  const int c = ccell[r];
  const int i = c % g.xm, t = c / g.xm;
  const int j = t % g.ym, k = t / g.ym;
  abso[(size_t)k + (size_t)g.Nz * ((size_t)i + (size_t)g.xm * j)] = val;
}

int bld_grow(tsx_solver *s, TsxBuildings *B, size_t nfaces) {
  if (nfaces <= B->cap) return TSX_OK;
  if (B->dev) HIPCHK(tsx_dev_free(B->dev));
  B->dev = nullptr;
  B->cap = 0;
  const size_t cap = nfaces + nfaces / 4 + 16;
  // slices in units of 16 bytes: iface 8, ftup 16, fslot 4, falb 8, fplk 8, out 24, ccell 4, cmask 4, calb 48 bytes per face
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t sz[9] = {al(8 * cap), al(16 * cap), al(4 * cap), al(8 * cap), al(8 * cap), al(24 * cap), al(4 * cap), al(4 * cap), al(48 * cap)};
  size_t tot = 0;
  for (size_t v : sz) tot += v;
  HIPCHK(tsx_dev_malloc((void **)&B->dev, tot));
  char *p = B->dev;
  B->d_iface = (long long *)p, p += sz[0];
  B->d_ftup = (int4 *)p, p += sz[1];
  B->d_fslot = (int *)p, p += sz[2];
  B->d_falb = (double *)p, p += sz[3];
  B->d_fplk = (double *)p, p += sz[4];
  B->d_out = (double *)p, p += sz[5];
  B->d_ccell = (int *)p, p += sz[6];
  B->d_cmask = (unsigned *)p, p += sz[7];
  B->d_calb = (double *)p;
  B->cap = cap;
  B->iface.clear();  // the records are gone with the old allocation: decode again
  (void)s;
  return TSX_OK;
}

// whatever was derived from the previous face list / albedos is void: the next solve wants new optical properties
void bld_invalidate(tsx_solver *s) {
  s->have_optprop = s->have_coeffs = false;
  s->dir_coeffs_valid = false;
  s->pcx_valid = s->coef_h_valid = false;
  s->dd_from_coords = false;
}
}  // namespace

void tsx_buildings_free(tsx_solver *s) {
  if (!s->bld) return;
  if (s->bld->dev) (void)tsx_dev_free(s->bld->dev);
  delete s->bld;
  s->bld = nullptr;
  s->bld_nfaces = 0;
}

// what this path does not cover (DESIGN.md "Buildings"): several ranks, a collapsed atmosphere, the 1-D solvers
int tsx_buildings_refuse(const tsx_solver *s, const char *who) {
  const char *why = nullptr;
  if (s->grid.nranks > 1 || !(s->geo.wrap_x && s->geo.wrap_y)) why = "on a handle with more than one rank (or force_halo)";
  else if (s->collapse > 1) why = "with a collapsed atmosphere (tsx_pprts_set_collapse > 1)";
  else if (s->mode_1d) why = "on a handle with a 1-D solver (tsx_pprts_set_1d_solver)";
  if (!why) return TSX_OK;
  tsx_set_error(std::string(who) + ": buildings are not supported " + why);
  return TSX_ERR_UNSUPPORTED;
}

// a building face in a layer that the solve treats as 1-D: the reference ignores the patched block there but still overwrites
// the source -- refused
int tsx_buildings_check_layers(const tsx_solver *s, const uint8_t *l1d_host) {
  const TsxBuildings *B = s->bld;
  for (size_t m = 0; m < B->face_k.size(); ++m)
    if (l1d_host[B->face_k[m]]) {
      tsx_set_error("tsx_pprts_set_optical_properties: building face " + std::to_string(m) + " lies in layer " +
                    std::to_string(B->face_k[m]) + ", which is solved 1-D (dz / dx > 2): not supported");
      return TSX_ERR_UNSUPPORTED;
    }
  return TSX_OK;
}

extern "C" int tsx_pprts_set_buildings(tsx_solver *s, int64_t nfaces, const int64_t *iface, const double *albedo, const double *planck,
                                       int where) {
  ARGCHK(s, "tsx_pprts_set_buildings: null");
  ARGCHK(nfaces >= 0, "tsx_pprts_set_buildings: nfaces < 0");
  if (nfaces == 0) {  // detach
    if (s->bld_nfaces > 0) bld_invalidate(s);
    s->bld_nfaces = 0;
    return TSX_OK;
  }
  ARGCHK(iface && albedo, "tsx_pprts_set_buildings: null argument");
  if (int rc = tsx_buildings_refuse(s, "tsx_pprts_set_buildings")) return rc;
  const TsxGeo &g = s->geo;
  if (g.Nc >= (1ll << 31)) {  // the cell records index cells with ints
    tsx_set_error("tsx_pprts_set_buildings: buildings are not supported on grids of 2^31 cells or more");
    return TSX_ERR_UNSUPPORTED;
  }
  const long long nmax = 6ll * g.Nc;
  ARGCHK(nfaces <= nmax, "tsx_pprts_set_buildings: more faces than the grid has");
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)nfaces;
  std::vector<long long> hi(n);
  std::vector<double> ha(n), hp(planck ? n : 0);
  if (where == TSX_HOST) {
    for (size_t m = 0; m < n; ++m) hi[m] = iface[m];
    memcpy(ha.data(), albedo, sizeof(double) * n);
    if (planck) memcpy(hp.data(), planck, sizeof(double) * n);
  } else {
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(hi.data(), iface, sizeof(long long) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ha.data(), albedo, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (planck) HIPCHK(hipMemcpy(hp.data(), planck, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  // validation on the host: index in range (face id and cell follow from it), albedo in [0, 1], no face twice
  for (size_t m = 0; m < n; ++m) {
    if (hi[m] < 1 || hi[m] > nmax) {
      tsx_set_error("tsx_pprts_set_buildings: iface[" + std::to_string(m) + "] = " + std::to_string(hi[m]) + " is outside 1 .. 6 * Nz * xm * ym = " +
                    std::to_string(nmax) + " (face id or cell out of range)");
      return TSX_ERR_ARG;
    }
    if (!(ha[m] >= 0.0 && ha[m] <= 1.0)) {
      tsx_set_error("tsx_pprts_set_buildings: albedo[" + std::to_string(m) + "] = " + std::to_string(ha[m]) + " is outside [0, 1]");
      return TSX_ERR_ARG;
    }
  }
  std::vector<size_t> order(n);
  for (size_t m = 0; m < n; ++m) order[m] = m;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return hi[a] != hi[b] ? hi[a] < hi[b] : a < b; });
  {
    size_t first_dup = n;
    for (size_t q = 1; q < n; ++q)
      if (hi[order[q]] == hi[order[q - 1]] && order[q] < first_dup) first_dup = order[q];
    if (first_dup < n) {
      tsx_set_error("tsx_pprts_set_buildings: iface[" + std::to_string(first_dup) + "] = " + std::to_string(hi[first_dup]) + " is listed twice");
      return TSX_ERR_ARG;
    }
  }
  if (!s->bld) s->bld = new TsxBuildings();
  TsxBuildings *B = s->bld;
  if (int rc = bld_grow(s, B, n)) return rc;
  const int nb = (int)((n + TSX_BLOCK - 1) / TSX_BLOCK);
  if (B->iface != hi) {  // a new face list: decode it.  Sorted by index the faces of a cell are neighbours (the face id runs fastest)
    std::vector<int> slot(n);
    B->face_k.assign(n, 0);
    int ncells = 0;
    long long prev_cell = -1;
    for (size_t q = 0; q < n; ++q) {
      const size_t m = order[q];
      const long long cell = (hi[m] - 1) / 6;
      if (cell != prev_cell) ++ncells, prev_cell = cell;
      slot[m] = ncells - 1;
      B->face_k[m] = (int)(cell % g.Nz);
    }
    HIPCHK(hipMemcpyAsync(B->d_iface, hi.data(), sizeof(long long) * n, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(B->d_fslot, slot.data(), sizeof(int) * n, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemsetAsync(B->d_cmask, 0, sizeof(unsigned) * (size_t)ncells, s->stream));
    hipLaunchKernelGGL(tsx_k_bld_decode, dim3(nb), dim3(TSX_BLOCK), 0, s->stream, g, (int)n, B->d_iface, B->d_fslot, B->d_ftup, B->d_ccell,
                       B->d_cmask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));  // slot (host vector) must outlive the copy
    B->ncells = ncells;
    B->iface = hi;
  }
  HIPCHK(hipMemcpyAsync(B->d_falb, ha.data(), sizeof(double) * n, hipMemcpyHostToDevice, s->stream));
  if (planck) HIPCHK(hipMemcpyAsync(B->d_fplk, hp.data(), sizeof(double) * n, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipMemsetAsync(B->d_calb, 0, sizeof(double) * 6 * (size_t)B->ncells, s->stream));
  hipLaunchKernelGGL(tsx_k_bld_albedo, dim3(nb), dim3(TSX_BLOCK), 0, s->stream, (int)n, B->d_ftup, B->d_fslot, B->d_falb, B->d_calb);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  B->have_planck = planck != nullptr;
  s->bld_nfaces = (int)n;
  bld_invalidate(s);
  return TSX_OK;
}

extern "C" int tsx_pprts_set_abso_in_buildings(tsx_solver *s, int on, double val) {
  ARGCHK(s, "tsx_pprts_set_abso_in_buildings: null");
  s->bld_abso_on = on != 0;
  s->bld_abso_val = val;
  return TSX_OK;
}

// behind tsx_k_lut_diff2diff, before the blocks are shared: patch the dense planes and renew the patched cells' hashes
int tsx_buildings_patch_diffuse(tsx_solver *s, unsigned long long *hash) {
  const TsxBuildings *B = s->bld;
  const TsxGeo &g = s->geo;
  if (g.ntop == 2)
    hipLaunchKernelGGL((tsx_k_bld_patch_diffuse<2, 4>), dim3(B->ncells), dim3(64), 0, s->stream, g.Nc, B->ncells, B->d_ccell, B->d_cmask, B->d_calb,
                       (float *)s->coef, hash);
  else
    hipLaunchKernelGGL((tsx_k_bld_patch_diffuse<8, 4>), dim3(B->ncells), dim3(64), 0, s->stream, g.Nc, B->ncells, B->d_ccell, B->d_cmask, B->d_calb,
                       (float *)s->coef, hash);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// behind tsx_k_lut_dir, before the sweep
int tsx_buildings_zero_dir(tsx_solver *s) {
  const TsxBuildings *B = s->bld;
  const int S = s->geo.ntop == 2 ? 3 : 8;
  hipLaunchKernelGGL(tsx_k_bld_zero_dir, dim3(grid_for((long long)B->ncells * S * S)), dim3(TSX_BLOCK), 0, s->stream, s->geo.Nc, B->ncells, S * S,
                     B->d_ccell, s->dirT);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// behind tsx_k_setup_b_solar / tsx_k_setup_b_thermal
int tsx_buildings_source(tsx_solver *s, int lsolar) {
  const TsxBuildings *B = s->bld;
  const TsxGeo &g = s->geo;
  const int n = s->bld_nfaces, nb = (n + TSX_BLOCK - 1) / TSX_BLOCK;
  const double *plk = B->have_planck ? B->d_fplk : (const double *)nullptr;
  if (g.ntop == 2)
    hipLaunchKernelGGL((tsx_k_bld_source<2, 4, 1, 1>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, g, n, lsolar, B->d_ftup, B->d_falb, plk, s->edir_a,
                       s->d_dz, s->opt_dx, s->opt_dy, s->vb);
  else
    hipLaunchKernelGGL((tsx_k_bld_source<8, 4, 4, 2>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, g, n, lsolar, B->d_ftup, B->d_falb, plk, s->edir_a,
                       s->d_dz, s->opt_dx, s->opt_dy, s->vb);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// tsx_pprts_get_result with -pprts_set_abso_in_buildings: abso is the result array on the device (reference layout)
int tsx_buildings_abso(tsx_solver *s, double *abso_dev) {
  const TsxBuildings *B = s->bld;
  hipLaunchKernelGGL(tsx_k_bld_abso, dim3((B->ncells + TSX_BLOCK - 1) / TSX_BLOCK), dim3(TSX_BLOCK), 0, s->stream, s->geo, B->ncells, B->d_ccell,
                     s->bld_abso_val, abso_dev);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

extern "C" int tsx_pprts_get_buildings(tsx_solver *s, double *edir, double *incoming, double *outgoing, int where) {
  ARGCHK(s && incoming && outgoing, "tsx_pprts_get_buildings: null argument");
  if (s->bld_nfaces <= 0) {
    tsx_set_error("tsx_pprts_get_buildings: no buildings attached (tsx_pprts_set_buildings)");
    return TSX_ERR_STATE;
  }
  if (!s->have_solution || s->sol_is_1d || !s->have_optprop) {
    tsx_set_error("tsx_pprts_get_buildings: no solution with these buildings (call tsx_pprts_set_optical_properties and tsx_pprts_solve)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  TsxBuildings *B = s->bld;
  const TsxGeo &g = s->geo;
  const int n = s->bld_nfaces, nb = (n + TSX_BLOCK - 1) / TSX_BLOCK;
  const int lsolar = s->last_lsolar;
  double *d_e = edir, *d_i = incoming, *d_o = outgoing;
  if (where == TSX_HOST) d_e = edir ? B->d_out : nullptr, d_i = B->d_out + B->cap, d_o = B->d_out + 2 * B->cap;
  TsxLogScope log_res(s, TSX_EV_GET_RESULT);  // fill_buildings_arr runs inside pprts_get_result (src/pprts.F90:5906-5910)
  if (g.ntop == 2)
    hipLaunchKernelGGL((tsx_k_bld_results<2, 4, 1, 1>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, g, n, lsolar, s->sun_mu, B->d_ftup, s->edir_a, s->vx,
                       s->d_dz, s->opt_dx, s->opt_dy, d_e, d_i, d_o);
  else
    hipLaunchKernelGGL((tsx_k_bld_results<8, 4, 4, 2>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, g, n, lsolar, s->sun_mu, B->d_ftup, s->edir_a, s->vx,
                       s->d_dz, s->opt_dx, s->opt_dy, d_e, d_i, d_o);
  HIPCHK(hipGetLastError());
  if (where == TSX_HOST) {
    if (edir) HIPCHK(hipMemcpyAsync(edir, d_e, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(incoming, d_i, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(outgoing, d_o, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  return TSX_OK;
}
