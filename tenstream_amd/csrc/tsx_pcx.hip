// tsx_pcx.hip -- the red-black column-block preconditioner in the reference's default arithmetic: exact blocks, fp64 iterates,
// fp64 recurrences -- as a segmented scan over the levels (round 6).
//
// The reference preconditions in `ireals` (real64 by default: PCILU / PCBJACOBI + ILU(0) on the assembled matrix,
// src/pprts.F90:4350-4371).  Until round 5 the only preconditioner of this library that rounded nothing was round 1's zebra-row
// sweep with one lane per column (tsx_k_pc_column_h1: 14 iterations, 36 M cells/s on the metric domain) -- what
// `fp32_directions = 0, pc_coeff_fp16 = 0` got, and what the retry after a failed solve ran (krylov_run_with_retry).  This is the
// same M^-1 as the mixed-precision scan kernels apply (tsx_kernels_pcs.hpp: exact two-stream solve per column, colours
// (i + j) & 1 alternately, the other colour's latest side streams on the right-hand side), evaluated the same way -- the column
// recurrences split into a matrix-only part (tsx_k_pcx_pack_col, once per coefficient set) and affine recurrences that NSEG
// segments of a column scan concurrently -- but on the operator's own blocks (fp32 as the LUT delivers them, lossless, or fp64)
// with every intermediate in fp64, directly in the Krylov vectors' dst-owned layout: a pass reads the other colour's side streams
// from z where the operator would read them from x (tsx_k_spmv_w's gather) and writes its colour's ten streams to z.  Nothing is
// packed, nothing is rounded; rank faces are treated like the reference's PCBJACOBI treats them (couplings across them dropped).
//     upward    B_k     = (ru_k + F_k rd_k) + E_k B_{k+1}       B_Nz = ru_Nz        U_k = A_k V_k + B_k
//     downward  V_{k+1} = (G_k rd_k + H_k B_{k+1}) + GT_k V_k   V_0  = rd_TOA
//     E = Tuu G, F = Tuu A_{k+1} G, G = 1 / (1 - Rdu A_{k+1}), H = G Rdu, GT = G Tdd, A_k = Rud + Tuu A_{k+1} GT, A_Nz = albedo
// The passes work on colour-split copies of v and z (within a row the xm / 2 columns of colour 0, then colour 1: tsx_split_pos) and on
// recurrence planes in the same order, so that a pass over one colour reads and writes contiguous memory -- in the Krylov vectors'
// natural order the lanes sit on every other column, every access touches twice the cache lines it uses, and the first version of
// this kernel was bound by exactly that (0.31 ms per pass, profiles/r06/exact_pc_bench.txt); two permuting copies per application.
// 8_16 (H = 4 up/down pairs: 4-vectors and 4 x 4 blocks) has kernels of its own below, tsx_k_pcx16_pack_col / tsx_k_pcx16_rb;
// tsx_pcx_apply dispatches on geo.ntop.  Odd grids keep the zebra rows, for both solvers.
#include "tsx_host.hpp"
#include "tsx_pack.hpp"

namespace {
constexpr int PCX_CW = 16, PCX_NSEG = 16, PCX_REC = 7;

// matrix-only part, one lane per column: rec[q * Nc + c], q = E F G H GT A_{k+1} A_k (natural cell order)
template <typename CT, bool IDX>
__global__ __launch_bounds__(64) void tsx_k_pcx_pack_col(TsxGeo g, const CT *__restrict__ C, const int *__restrict__ cidx,
                                                         const uint8_t *__restrict__ l1d, const double *__restrict__ a11,
                                                         const double *__restrict__ a12, const double *__restrict__ albedo,
                                                         double *__restrict__ rec) {
  constexpr int D = 10;
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= g.ncol) return;
  const size_t Nc = (size_t)g.Nc;
  const size_t sp = (size_t)tsx_split_col(col % g.xm, col / g.xm, g.xm);  // the records live in colour-split order
  double A = albedo[col];
  for (int k = g.Nz - 1; k >= 0; --k) {
    const size_t c = (size_t)k * g.ncol + col;
    const size_t o = (size_t)k * g.ncol + sp;
    double tuu, rud, rdu, tdd;
    if (l1d[k]) {
      tuu = tdd = a11[c];
      rud = rdu = a12[c];
    } else if (IDX) {  // entry-major shared blocks Ce[id * D*D + dst * D + src]
      const CT *b = C + (size_t)cidx[c] * (D * D);
      tuu = (double)b[0 * D + 0];
      rud = (double)b[0 * D + 1];
      rdu = (double)b[1 * D + 0];
      tdd = (double)b[1 * D + 1];
    } else {
      tuu = (double)C[(size_t)(0 * D + 0) * Nc + c];
      rud = (double)C[(size_t)(0 * D + 1) * Nc + c];
      rdu = (double)C[(size_t)(1 * D + 0) * Nc + c];
      tdd = (double)C[(size_t)(1 * D + 1) * Nc + c];
    }
    const double G = 1.0 / (1.0 - rdu * A);
    const double GT = G * tdd;
    const double Ao = rud + tuu * A * GT;
    rec[0 * Nc + o] = tuu * G;
    rec[1 * Nc + o] = tuu * A * G;
    rec[2 * Nc + o] = G;
    rec[3 * Nc + o] = G * rdu;
    rec[4 * Nc + o] = GT;
    rec[5 * Nc + o] = A;
    rec[6 * Nc + o] = Ao;
    A = Ao;
  }
}

// o[split position] = a[natural position] (to_split) or the reverse, over the N unknowns (body planes and tail rows)
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_pcx_permute(TsxGeo g, int to_split, const double *__restrict__ a, double *__restrict__ o,
                                                               const int *__restrict__ done) {
  if (done && *done) return;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < g.N; q += (long long)gridDim.x * TSX_BLOCK) {
    const long long p = tsx_split_pos(q, g);
    if (to_split) o[p] = a[q];
    else o[q] = a[p];
  }
}

// one half-grid pass: the columns of colour rbc.  r, z, zo, rec: colour-split order; C (dense planes) and cidx: natural order.  gs: the other colour's side streams (from z) enter the right-hand side
template <typename CT, int LSEG, bool IDX, bool GS>
__global__ __launch_bounds__(PCX_CW *PCX_NSEG) void tsx_k_pcx_rb(TsxGeo g, const CT *__restrict__ C, const int *__restrict__ cidx,
                                                                 const double *__restrict__ rec, const uint8_t *__restrict__ l1d,
                                                                 const double *__restrict__ r, double *__restrict__ z,
                                                                 const double *__restrict__ zo, const int *__restrict__ done, int rbc) {
  constexpr bool gs = GS;
  // zo aliases z; it is only read at columns of the OTHER colour, which this launch never writes (a separate restrict pointer
  // lets the compiler issue those loads ahead of the stores to z)
  constexpr int D = 10, CW = PCX_CW, NSEG = PCX_NSEG;
  __shared__ double2 sS[NSEG][CW];
  if (done && *done) return;
  const int xm = g.xm, ym = g.ym, Nz = g.Nz, ncol = g.ncol;
  const size_t Nc = (size_t)g.Nc;
  const int h = xm >> 1;
  const int cl = threadIdx.x % CW, sg = threadIdx.x / CW;
  int t = blockIdx.x * CW + cl;
  const bool live = t < ym * h;
  if (!live) t = ym * h - 1;
  const int jrow = t / h, qh = t - jrow * h;
  const int par = (jrow + rbc) & 1;
  const int i = 2 * qh + par;
  const int coln = jrow * xm + i;            // natural column (dense coefficient planes, per-cell index)
  const int col = jrow * xm + rbc * h + qh;  // colour-split column (r, z, rec)
  // the neighbour a side source stream comes from (tsx_k_spmv_w's gather): inward x streams from the west, the others from the
  // east; inward y streams from the south, the others from the north -- all of the other colour, i.e. in the other half of a row
  // in split order (as tsx_pcs_rb_body addresses them).  0 = no neighbour (rank face, or gs off)
  const int oc = (1 - 2 * rbc) * h;
  const int jn = jrow + 1 < ym ? jrow + 1 : (g.wrap_y ? 0 : -1), js = jrow > 0 ? jrow - 1 : (g.wrap_y ? ym - 1 : -1);
  const int qw = par ? qh : (qh > 0 ? qh - 1 : (g.wrap_x ? h - 1 : -1)), qe = par ? (qh + 1 < h ? qh + 1 : (g.wrap_x ? 0 : -1)) : qh;
  long long offN = jn >= 0 ? (long long)(jn - jrow) * xm + oc : 0, offS = js >= 0 ? (long long)(js - jrow) * xm + oc : 0;
  long long offE = qe >= 0 ? (long long)oc + (qe - qh) : 0, offW = qw >= 0 ? (long long)oc + (qw - qh) : 0;
  if (g.pc_tile_x > 0) {
    if ((i + 1) % g.pc_tile_x == 0) offE = 0;
    if (i % g.pc_tile_x == 0) offW = 0;
  }
  if (g.pc_tile_y > 0) {
    if ((jrow + 1) % g.pc_tile_y == 0) offN = 0;
    if (jrow % g.pc_tile_y == 0) offS = 0;
  }
  if (!gs) offW = offE = offS = offN = 0;
  const long long soff[8] = {offE, offW, offE, offW, offN, offS, offN, offS};  // source stream 2 + q: tsx_inward(q) = q & 1
  const double *__restrict__ rt = r + (size_t)D * Nc;
  double *__restrict__ zt = z + (size_t)D * Nc;
  const int k0 = sg * LSEG;
  auto lev = [&](int l) { return k0 + l < Nz ? k0 + l : Nz - 1; };
  // src 2..9 of row dst (the couplings to the side streams that enter from the neighbouring columns) and src 0, 1 (the column's own
  // top streams), all loads unconditional -- a load under a branch ends a basic block and costs a full wait per level;
  // shared blocks are entry-major, a row is 40 contiguous bytes: five 8-byte loads instead of ten 4-byte ones
  auto row = [&](size_t c, int id, int dst, double(&top)[2], double(&side)[8]) {
    if constexpr (IDX && sizeof(CT) == 4) {
      const float2 *rw = reinterpret_cast<const float2 *>(C + (size_t)id * (D * D) + dst * D);
      const float2 t = rw[0];
      top[0] = (double)t.x;
      top[1] = (double)t.y;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float2 v = rw[1 + q];
        side[2 * q] = (double)v.x;
        side[2 * q + 1] = (double)v.y;
      }
    } else {
      top[0] = (double)C[(size_t)(dst * D + 0) * Nc + c];
      top[1] = (double)C[(size_t)(dst * D + 1) * Nc + c];
#pragma unroll
      for (int q = 0; q < 8; ++q) side[q] = (double)C[(size_t)(dst * D + 2 + q) * Nc + c];
    }
  };
  auto nbrs = [&](size_t c, double(&zn)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = zo[(size_t)(2 + q) * Nc + c + soff[q]];  // unconditional load from a valid address, then select
      zn[q] = soff[q] ? v : 0.0;
    }
  };
  // ---- phase 1: local upward scan with zero inflow
  double beta[LSEG], rdv[LSEG], Ek[LSEG];
  {
    double Bl = 0.0, Pe = 1.0;
#pragma unroll
    for (int l = LSEG - 1; l >= 0; --l) {
      const bool act = k0 + l < Nz;
      const int k = lev(l);
      const size_t c = (size_t)k * ncol + col;
      double ru = r[0 * Nc + c], rd = r[1 * Nc + c];
      if constexpr (GS) {
        const bool one = l1d[k] != 0;
        const size_t cn = (size_t)k * ncol + coln;
        const int id = IDX ? cidx[cn] : 0;
        double zn[8], t0[2], t1[2], c0[8], c1[8];
        nbrs(c, zn);
        row(cn, id, 0, t0, c0);
        row(cn, id, 1, t1, c1);
        double gu = 0.0, gd = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          gu += c0[q] * zn[q];
          gd += c1[q] * zn[q];
        }
        ru += one ? 0.0 : gu;  // (a select, not a product: a 1-D layer's block may hold anything)
        rd += one ? 0.0 : gd;
      }
      const double E = rec[0 * Nc + c], F = rec[1 * Nc + c];
      Ek[l] = E;
      rdv[l] = rd;
      beta[l] = act ? ru + F * rd : 0.0;
      if (act) {
        Bl = beta[l] + E * Bl;
        Pe = E * Pe;
      }
    }
    sS[sg][cl] = make_double2(Bl, Pe);
  }
  __syncthreads();
  double Bin = rt[(size_t)0 * ncol + col];  // B_Nz = ru_Nz
  for (int s2 = NSEG - 1; s2 > sg; --s2) {
    const double2 m = sS[s2][cl];
    Bin = m.x + m.y * Bin;
  }
  // ---- phase 2: the true B of every level
  double Bk[LSEG];
  {
    double Bc = Bin;
#pragma unroll
    for (int l = LSEG - 1; l >= 0; --l) {
      if (k0 + l < Nz) Bc = beta[l] + Ek[l] * Bc;
      Bk[l] = Bc;
    }
  }
  __syncthreads();  // the upward summaries have been read: the buffer is free for the downward ones
  // ---- phase 3: local downward scan with zero inflow
  double gam[LSEG], GTk[LSEG];
  {
    double Vl = 0.0, Q = 1.0;
#pragma unroll
    for (int l = 0; l < LSEG; ++l) {
      const bool act = k0 + l < Nz;
      const size_t c = (size_t)lev(l) * ncol + col;
      const double Bn = l + 1 < LSEG ? Bk[l + 1 < LSEG ? l + 1 : l] : Bin;
      const double G = rec[2 * Nc + c], H = rec[3 * Nc + c], GT = rec[4 * Nc + c];
      GTk[l] = GT;
      gam[l] = act ? G * rdv[l] + H * Bn : 0.0;
      if (act) {
        Vl = gam[l] + GT * Vl;
        Q = GT * Q;
      }
    }
    sS[sg][cl] = make_double2(Vl, Q);
  }
  __syncthreads();
  double V = rt[(size_t)1 * ncol + col];  // V_0 = rd_TOA
  if (sg == 0 && live) {  // tail rows: the TOA identity row and the side dummies at level Nz
    zt[(size_t)1 * ncol + col] = V;
#pragma unroll
    for (int d = 2; d < D; ++d) zt[(size_t)d * ncol + col] = rt[(size_t)d * ncol + col];
  }
  for (int s2 = 0; s2 < sg; ++s2) {
    const double2 m = sS[s2][cl];
    V = m.x + m.y * V;
  }
  // ---- phase 4: true V, U; side streams; stores
  // (no early exit from the level loop: a branch between the levels fences their loads off from each other -- the loads of absent
  // levels go to the clamped level and only the stores are predicated)
#pragma unroll
  for (int l = 0; l < LSEG; ++l) {
    const bool act = k0 + l < Nz;
    const bool st = live && act;
    const int k = lev(l);
    const size_t c = (size_t)k * ncol + col;
    const double Bn = l + 1 < LSEG ? Bk[l + 1 < LSEG ? l + 1 : l] : Bin;
    const double Vn = gam[l] + GTk[l] * V;
    const double Un = rec[5 * Nc + c] * Vn + Bn;      // U_{k+1} = A_{k+1} V_{k+1} + B_{k+1}
    const double Uk = rec[6 * Nc + c] * V + Bk[l];    // U_k
    if (st) {
      z[0 * Nc + c] = Uk;
      z[1 * Nc + c] = Vn;
    }
    const bool one = l1d[k] != 0;
    const size_t cn = (size_t)k * ncol + coln;
    const int id = IDX ? cidx[cn] : 0;
    double zn[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (GS) nbrs(c, zn);
#pragma unroll
    for (int d = 2; d < D; ++d) {
      double tp[2], sd[8];
      row(cn, id, d, tp, sd);
      double acc = tp[0] * Un + tp[1] * V;
      if constexpr (GS) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += sd[q] * zn[q];
      }
      acc = r[(size_t)d * Nc + c] + (one ? 0.0 : acc);
      if (st) z[(size_t)d * Nc + c] = acc;
    }
    if (k0 + l == Nz - 1 && live) zt[(size_t)0 * ncol + col] = Un;  // U_Nz = albedo V_Nz + ru_Nz: the surface row
    V = act ? Vn : V;
  }
}

// ---- 8_16: the same scan with H = 4 up/down pairs (the recurrences of tsx_k_pcsh_pack_col / tsx_k_pcsh_rb, every intermediate in
// fp64).  U, V, B are 4-vectors (top dofs 2a up, 2a + 1 down), the matrix-only quantities 4 x 4 blocks:
//     G = (I - Rdu A_{k+1})^-1,  GT = G Tdd,  H = G Rdu,  F = Tuu A_{k+1} G,  E = Tuu + F Rdu,  A_k = Rud + F Tdd,  A_Nz = albedo / 4
// Records: rec[(q * 16 + 4 a + b) * Nc + cell], q = E F G H GT A_{k+1} A_k, colour-split order (896 B per cell).  A segment's
// summary is (4-vector, 4 x 4 product), 160 B through LDS.  The blocks are not held across phases: every phase re-reads the
// records it needs (a level's 4 x 4 blocks in registers would cost 32 VGPRs each); only 4-vectors per level stay live.  Levels per
// thread are fixed (PCX16_LSEG); taller columns get more segments per column and fewer columns per workgroup.
constexpr int PCX16_LSEG = 4, PCX16_NTHR = 256, PCX16_REC = 7 * 16;

template <typename CT, bool IDX>
__global__ __launch_bounds__(64) void tsx_k_pcx16_pack_col(TsxGeo g, const CT *__restrict__ C, const int *__restrict__ cidx,
                                                           const uint8_t *__restrict__ l1d, const double *__restrict__ a11,
                                                           const double *__restrict__ a12, const double *__restrict__ albedo,
                                                           double *__restrict__ rec) {
  constexpr int D = 16, H = 4;
  using SM = TsxSm<H>;
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= g.ncol) return;
  const size_t Nc = (size_t)g.Nc;
  const size_t sp = (size_t)tsx_split_col(col % g.xm, col / g.xm, g.xm);
  double A[H][H];
#pragma unroll
  for (int a = 0; a < H; ++a)
#pragma unroll
    for (int b = 0; b < H; ++b) A[a][b] = albedo[col] / (double)H;  // assembled surface row: albedo / streams on every pair
  for (int k = g.Nz - 1; k >= 0; --k) {
    const size_t c = (size_t)k * g.ncol + col;
    const size_t o = (size_t)k * g.ncol + sp;
    double Tuu[H][H], Rud[H][H], Rdu[H][H], Tdd[H][H];
    if (l1d[k]) {
      const double t11 = a11[c], t12 = a12[c];
#pragma unroll
      for (int a = 0; a < H; ++a)
#pragma unroll
        for (int b = 0; b < H; ++b) {
          Tuu[a][b] = Tdd[a][b] = a == b ? t11 : 0.0;
          Rud[a][b] = Rdu[a][b] = a == b ? t12 : 0.0;
        }
    } else {
      auto cf = [&](int dst, int src) {
        if constexpr (IDX) return (double)C[(size_t)cidx[c] * (D * D) + dst * D + src];  // entry-major shared blocks
        else return (double)C[(size_t)(dst * D + src) * Nc + c];
      };
#pragma unroll
      for (int a = 0; a < H; ++a)
#pragma unroll
        for (int b = 0; b < H; ++b) {
          Tuu[a][b] = cf(2 * a, 2 * b);
          Rud[a][b] = cf(2 * a, 2 * b + 1);
          Rdu[a][b] = cf(2 * a + 1, 2 * b);
          Tdd[a][b] = cf(2 * a + 1, 2 * b + 1);
        }
    }
    double RA[H][H], G[H][H], GT[H][H], Hm[H][H], TA[H][H], F[H][H], FR[H][H], E[H][H], FT[H][H], Ao[H][H];
    SM::matmul(Rdu, A, RA);
    SM::inv_i_minus(RA, G);
    SM::matmul(G, Tdd, GT);
    SM::matmul(G, Rdu, Hm);
    SM::matmul(Tuu, A, TA);
    SM::matmul(TA, G, F);
    SM::matmul(F, Rdu, FR);
    SM::matmul(F, Tdd, FT);
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) {
        E[a][b] = Tuu[a][b] + FR[a][b];
        Ao[a][b] = Rud[a][b] + FT[a][b];
      }
    auto put = [&](int q, const double(&M)[H][H]) {
#pragma unroll
      for (int a = 0; a < H; ++a)
#pragma unroll
        for (int b = 0; b < H; ++b) rec[(size_t)(q * 16 + 4 * a + b) * Nc + o] = M[a][b];
    };
    put(0, E);
    put(1, F);
    put(2, G);
    put(3, Hm);
    put(4, GT);
    put(5, A);
    put(6, Ao);
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) A[a][b] = Ao[a][b];
  }
}

// one half-grid pass of 8_16, as tsx_k_pcx_rb: NSEG segments of PCX16_LSEG levels per column, PCX16_NTHR / NSEG columns per workgroup
template <typename CT, int NSEG, bool IDX, bool GS>
__global__ __launch_bounds__(PCX16_NTHR) void tsx_k_pcx16_rb(TsxGeo g, const CT *__restrict__ C, const int *__restrict__ cidx,
                                                             const double *__restrict__ rec, const uint8_t *__restrict__ l1d,
                                                             const double *__restrict__ r, double *__restrict__ z,
                                                             const double *__restrict__ zo, const int *__restrict__ done, int rbc) {
  constexpr int D = 16, H = 4, NTOP = 8, LSEG = PCX16_LSEG, CW = PCX16_NTHR / NSEG;
  using SM = TsxSm<H>;
  __shared__ double sS[NSEG][20][CW];  // a segment's summary: 4-vector, then the 4 x 4 product row-major (reused by both scans)
  if (done && *done) return;
  const int xm = g.xm, ym = g.ym, Nz = g.Nz, ncol = g.ncol;
  const size_t Nc = (size_t)g.Nc;
  const int h = xm >> 1;
  const int cl = threadIdx.x % CW, sg = threadIdx.x / CW;
  int t = blockIdx.x * CW + cl;
  const bool live = t < ym * h;
  if (!live) t = ym * h - 1;
  const int jrow = t / h, qh = t - jrow * h;
  const int par = (jrow + rbc) & 1;
  const int i = 2 * qh + par;
  const int coln = jrow * xm + i;            // natural column (dense coefficient planes, per-cell index)
  const int col = jrow * xm + rbc * h + qh;  // colour-split column (r, z, rec)
  // neighbours as in tsx_k_pcx_rb: source streams 8 + q (x) and 12 + q (y), tsx_inward(q) from the west / south
  const int oc = (1 - 2 * rbc) * h;
  const int jn = jrow + 1 < ym ? jrow + 1 : (g.wrap_y ? 0 : -1), js = jrow > 0 ? jrow - 1 : (g.wrap_y ? ym - 1 : -1);
  const int qw = par ? qh : (qh > 0 ? qh - 1 : (g.wrap_x ? h - 1 : -1)), qe = par ? (qh + 1 < h ? qh + 1 : (g.wrap_x ? 0 : -1)) : qh;
  long long offN = jn >= 0 ? (long long)(jn - jrow) * xm + oc : 0, offS = js >= 0 ? (long long)(js - jrow) * xm + oc : 0;
  long long offE = qe >= 0 ? (long long)oc + (qe - qh) : 0, offW = qw >= 0 ? (long long)oc + (qw - qh) : 0;
  if (g.pc_tile_x > 0) {
    if ((i + 1) % g.pc_tile_x == 0) offE = 0;
    if (i % g.pc_tile_x == 0) offW = 0;
  }
  if (g.pc_tile_y > 0) {
    if ((jrow + 1) % g.pc_tile_y == 0) offN = 0;
    if (jrow % g.pc_tile_y == 0) offS = 0;
  }
  if (!GS) offW = offE = offS = offN = 0;
  const long long soff[8] = {offE, offW, offE, offW, offN, offS, offN, offS};
  const double *__restrict__ rt = r + (size_t)D * Nc;
  double *__restrict__ zt = z + (size_t)D * Nc;
  const int k0 = sg * LSEG;
  auto lev = [&](int l) { return k0 + l < Nz ? k0 + l : Nz - 1; };
  // o[n] = c(dst, s0 + n) of the cell; shared blocks are entry-major (a row is 64 contiguous bytes: 16-byte loads)
  auto row = [&](size_t cn, int id, int dst, int s0, auto &o) {
    constexpr int N = std::extent<std::remove_reference_t<decltype(o)>>::value;
    if constexpr (IDX && sizeof(CT) == 4) {
      const float4 *rw = reinterpret_cast<const float4 *>(C + (size_t)id * (D * D) + dst * D + s0);
#pragma unroll
      for (int q = 0; q < N / 4; ++q) {
        const float4 v = rw[q];
        o[4 * q] = (double)v.x;
        o[4 * q + 1] = (double)v.y;
        o[4 * q + 2] = (double)v.z;
        o[4 * q + 3] = (double)v.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < N; ++q) o[q] = (double)C[(size_t)(dst * D + s0 + q) * Nc + cn];
    }
  };
  auto nbrs = [&](size_t c, double(&zn)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = zo[(size_t)(NTOP + q) * Nc + c + soff[q]];  // unconditional load from a valid address, then select
      zn[q] = soff[q] ? v : 0.0;
    }
  };
  auto mat = [&](int q, size_t c, double(&M)[H][H]) {
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) M[a][b] = rec[(size_t)(q * 16 + 4 * a + b) * Nc + c];
  };
  auto put_summary = [&](const double(&v)[H], const double(&M)[H][H]) {
#pragma unroll
    for (int a = 0; a < H; ++a) sS[sg][a][cl] = v[a];
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) sS[sg][H + 4 * a + b][cl] = M[a][b];
  };
  auto chain = [&](int s2, double(&x)[H]) {  // x <- v(s2) + M(s2) x
    double o[H];
#pragma unroll
    for (int a = 0; a < H; ++a) {
      double acc = sS[s2][a][cl];
#pragma unroll
      for (int b = 0; b < H; ++b) acc += sS[s2][H + 4 * a + b][cl] * x[b];
      o[a] = acc;
    }
#pragma unroll
    for (int a = 0; a < H; ++a) x[a] = o[a];
  };
  // ---- phase 1: local upward scan with zero inflow; keeps beta and rd + couplings of its levels (4-vectors)
  double bk[LSEG][H], rg[LSEG][H];  // beta, then the true B_k (phase 2) | rd + couplings, then gamma (phase 3)
  {
    double Bl[H] = {0.0, 0.0, 0.0, 0.0}, Pc[H][H];
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) Pc[a][b] = a == b ? 1.0 : 0.0;
#pragma unroll
    for (int l = LSEG - 1; l >= 0; --l) {
      const bool act = k0 + l < Nz;
      const int k = lev(l);
      const size_t c = (size_t)k * ncol + col;
      double ru[H], rd[H];
#pragma unroll
      for (int a = 0; a < H; ++a) {
        ru[a] = r[(size_t)(2 * a) * Nc + c];
        rd[a] = r[(size_t)(2 * a + 1) * Nc + c];
      }
      if constexpr (GS) {
        const bool one = l1d[k] != 0;
        const size_t cn = (size_t)k * ncol + coln;
        const int id = IDX ? cidx[cn] : 0;
        double zn[8];
        nbrs(c, zn);
#pragma unroll
        for (int tt = 0; tt < NTOP; ++tt) {
          double cs[8];
          row(cn, id, tt, NTOP, cs);
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 8; ++q) acc += cs[q] * zn[q];
          acc = one ? 0.0 : acc;  // (a select, not a product: a 1-D layer's block may hold anything)
          if (tt & 1) rd[tt >> 1] += acc;
          else ru[tt >> 1] += acc;
        }
      }
      double M[H][H], Fr[H], EB[H], EP[H][H];
      mat(1, c, M);  // F
      SM::matvec(M, rd, Fr);
      mat(0, c, M);  // E
      SM::matvec(M, Bl, EB);
      SM::matmul(M, Pc, EP);
#pragma unroll
      for (int a = 0; a < H; ++a) {
        bk[l][a] = act ? ru[a] + Fr[a] : 0.0;
        rg[l][a] = rd[a];
        Bl[a] = act ? bk[l][a] + EB[a] : Bl[a];
#pragma unroll
        for (int b = 0; b < H; ++b) Pc[a][b] = act ? EP[a][b] : Pc[a][b];
      }
    }
    put_summary(Bl, Pc);
  }
  __syncthreads();
  double Bin[H];
#pragma unroll
  for (int a = 0; a < H; ++a) Bin[a] = rt[(size_t)(2 * a) * ncol + col];  // B_Nz = ru_Nz
  for (int s2 = NSEG - 1; s2 > sg; --s2) chain(s2, Bin);
  // ---- phase 2: the true B of every level (E re-read)
  {
    double Bc[H] = {Bin[0], Bin[1], Bin[2], Bin[3]};
#pragma unroll
    for (int l = LSEG - 1; l >= 0; --l) {
      const bool act = k0 + l < Nz;
      double E[H][H], EB[H];
      mat(0, (size_t)lev(l) * ncol + col, E);
      SM::matvec(E, Bc, EB);
#pragma unroll
      for (int a = 0; a < H; ++a) {
        Bc[a] = act ? bk[l][a] + EB[a] : Bc[a];
        bk[l][a] = Bc[a];
      }
    }
  }
  __syncthreads();  // the upward summaries have been read: the buffer is free for the downward ones
  // ---- phase 3: local downward scan with zero inflow
  {
    double Vl[H] = {0.0, 0.0, 0.0, 0.0}, Q[H][H];
#pragma unroll
    for (int a = 0; a < H; ++a)
#pragma unroll
      for (int b = 0; b < H; ++b) Q[a][b] = a == b ? 1.0 : 0.0;
#pragma unroll
    for (int l = 0; l < LSEG; ++l) {
      const bool act = k0 + l < Nz;
      const size_t c = (size_t)lev(l) * ncol + col;
      double Bn[H], M[H][H], Gr[H], HB[H], GV[H], GQ[H][H];
#pragma unroll
      for (int a = 0; a < H; ++a) Bn[a] = l + 1 < LSEG ? bk[l + 1 < LSEG ? l + 1 : l][a] : Bin[a];
      mat(2, c, M);  // G
      SM::matvec(M, rg[l], Gr);
      mat(3, c, M);  // H
      SM::matvec(M, Bn, HB);
      mat(4, c, M);  // GT
      SM::matvec(M, Vl, GV);
      SM::matmul(M, Q, GQ);
#pragma unroll
      for (int a = 0; a < H; ++a) {
        rg[l][a] = act ? Gr[a] + HB[a] : 0.0;
        Vl[a] = act ? rg[l][a] + GV[a] : Vl[a];
#pragma unroll
        for (int b = 0; b < H; ++b) Q[a][b] = act ? GQ[a][b] : Q[a][b];
      }
    }
    put_summary(Vl, Q);
  }
  __syncthreads();
  double V[H];
#pragma unroll
  for (int a = 0; a < H; ++a) V[a] = rt[(size_t)(2 * a + 1) * ncol + col];  // V_0 = rd_TOA
  if (sg == 0 && live) {  // tail rows: the TOA identity rows and the side dummies at level Nz
#pragma unroll
    for (int a = 0; a < H; ++a) zt[(size_t)(2 * a + 1) * ncol + col] = V[a];
#pragma unroll
    for (int d = NTOP; d < D; ++d) zt[(size_t)d * ncol + col] = rt[(size_t)d * ncol + col];
  }
  for (int s2 = 0; s2 < sg; ++s2) chain(s2, V);
  // ---- phase 4: true V, U; side streams; stores (loads of absent levels go to the clamped level, only the stores are predicated)
#pragma unroll
  for (int l = 0; l < LSEG; ++l) {
    const bool act = k0 + l < Nz;
    const bool st = live && act;
    const int k = lev(l);
    const size_t c = (size_t)k * ncol + col;
    double Bn[H], M[H][H], GV[H], Vn[H], AV[H], Un[H], Uk[H];
#pragma unroll
    for (int a = 0; a < H; ++a) Bn[a] = l + 1 < LSEG ? bk[l + 1 < LSEG ? l + 1 : l][a] : Bin[a];
    mat(4, c, M);  // GT
    SM::matvec(M, V, GV);
#pragma unroll
    for (int a = 0; a < H; ++a) Vn[a] = rg[l][a] + GV[a];
    mat(5, c, M);  // A_{k+1}
    SM::matvec(M, Vn, AV);
#pragma unroll
    for (int a = 0; a < H; ++a) Un[a] = AV[a] + Bn[a];  // U_{k+1} = A_{k+1} V_{k+1} + B_{k+1}
    mat(6, c, M);  // A_k
    SM::matvec(M, V, AV);
#pragma unroll
    for (int a = 0; a < H; ++a) Uk[a] = AV[a] + bk[l][a];
    if (st) {
#pragma unroll
      for (int a = 0; a < H; ++a) {
        z[(size_t)(2 * a) * Nc + c] = Uk[a];
        z[(size_t)(2 * a + 1) * Nc + c] = Vn[a];
      }
    }
    const bool one = l1d[k] != 0;
    const size_t cn = (size_t)k * ncol + coln;
    const int id = IDX ? cidx[cn] : 0;
    double zn[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (GS) nbrs(c, zn);
#pragma unroll
    for (int d = NTOP; d < D; ++d) {
      double cs[D];
      row(cn, id, d, 0, cs);
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < H; ++a) acc += cs[2 * a] * Un[a] + cs[2 * a + 1] * V[a];
      if constexpr (GS) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += cs[NTOP + q] * zn[q];
      }
      acc = r[(size_t)d * Nc + c] + (one ? 0.0 : acc);
      if (st) z[(size_t)d * Nc + c] = acc;
    }
    if (k0 + l == Nz - 1 && live) {  // U_Nz = (albedo / 4) sum V_Nz + ru_Nz: the surface rows
#pragma unroll
      for (int a = 0; a < H; ++a) zt[(size_t)(2 * a) * ncol + col] = Un[a];
    }
#pragma unroll
    for (int a = 0; a < H; ++a) V[a] = act ? Vn[a] : V[a];
  }
}
}  // namespace

// exact scan passes available for this solver's grid?  (3_10 or 8_16, an even number of columns per row, an even number of rows where
// the rank wraps onto itself in y, at most 256 levels); elsewhere the zebra rows
bool tsx_pcx_eligible(const tsx_solver *s) {
  const TsxGeo &g = s->geo;
  return (g.ntop == 2 || g.ntop == 8) && g.xm % 2 == 0 && g.xm >= 2 && (!g.wrap_y || g.ym % 2 == 0) && g.Nz <= 16 * PCX_NSEG &&
         g.Nz <= 64 * PCX16_LSEG && g.Nc < (1ll << 31);
}

// 8_16: the same sequence -- records once per coefficient set, colour-split copies, pc_sweeps + 1 passes, copy back
template <typename CT>
static int pcx16_apply_t(tsx_solver *s, const CT *C, bool idx, const double *v, double *z, const int *done) {
  const TsxGeo &g = s->geo;
  if (!s->pcx_rec) HIPCHK(tsx_dev_malloc((void **)&s->pcx_rec, sizeof(double) * (size_t)PCX16_REC * g.Nc));
  const int *cidx = idx ? (const int *)s->dd_cidx : (const int *)nullptr;
  if (!s->pcx_valid) {
    const int nbc = (g.ncol + 63) / 64;
    if (idx)
      hipLaunchKernelGGL((tsx_k_pcx16_pack_col<CT, true>), dim3(nbc), dim3(64), 0, s->stream, g, C, cidx, s->l1d, s->a11, s->a12,
                         s->albedo, s->pcx_rec);
    else
      hipLaunchKernelGGL((tsx_k_pcx16_pack_col<CT, false>), dim3(nbc), dim3(64), 0, s->stream, g, C, cidx, s->l1d, s->a11, s->a12,
                         s->albedo, s->pcx_rec);
    HIPCHK(hipGetLastError());
    s->pcx_valid = true;
  }
  if (!s->pcx_vz) HIPCHK(tsx_dev_malloc((void **)&s->pcx_vz, sizeof(double) * 2 * (size_t)g.N));
  double *vs = s->pcx_vz, *zs = s->pcx_vz + (size_t)g.N;
  hipLaunchKernelGGL(tsx_k_pcx_permute, dim3(grid_for(g.N, 8192)), dim3(TSX_BLOCK), 0, s->stream, g, 1, v, vs, done);
  const int nthr = g.ym * (g.xm / 2), P = s->pc_sweeps + 1;
  auto go = [&](auto nseg_tag, int pass) {
    constexpr int NSEG = decltype(nseg_tag)::value, CW = PCX16_NTHR / NSEG;
    const int nb = (nthr + CW - 1) / CW;
    const double *rec = s->pcx_rec, *zc = zs;
    if (idx && pass > 0)
      hipLaunchKernelGGL((tsx_k_pcx16_rb<CT, NSEG, true, true>), dim3(nb), dim3(PCX16_NTHR), 0, s->stream, g, C, cidx, rec, s->l1d, vs, zs,
                         zc, done, pass & 1);
    else if (idx)
      hipLaunchKernelGGL((tsx_k_pcx16_rb<CT, NSEG, true, false>), dim3(nb), dim3(PCX16_NTHR), 0, s->stream, g, C, cidx, rec, s->l1d, vs,
                         zs, zc, done, pass & 1);
    else if (pass > 0)
      hipLaunchKernelGGL((tsx_k_pcx16_rb<CT, NSEG, false, true>), dim3(nb), dim3(PCX16_NTHR), 0, s->stream, g, C, cidx, rec, s->l1d, vs,
                         zs, zc, done, pass & 1);
    else
      hipLaunchKernelGGL((tsx_k_pcx16_rb<CT, NSEG, false, false>), dim3(nb), dim3(PCX16_NTHR), 0, s->stream, g, C, cidx, rec, s->l1d, vs,
                         zs, zc, done, pass & 1);
  };
  for (int pass = 0; pass < P; ++pass) {
    if (g.Nz <= 16 * PCX16_LSEG) go(std::integral_constant<int, 16>{}, pass);
    else if (g.Nz <= 32 * PCX16_LSEG) go(std::integral_constant<int, 32>{}, pass);
    else go(std::integral_constant<int, 64>{}, pass);
  }
  hipLaunchKernelGGL(tsx_k_pcx_permute, dim3(grid_for(g.N, 8192)), dim3(TSX_BLOCK), 0, s->stream, g, 0, (const double *)zs, z, done);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

template <typename CT>
static int pcx_apply_t(tsx_solver *s, const CT *C, bool idx, const double *v, double *z, const int *done) {
  const TsxGeo &g = s->geo;
  if (g.ntop == 8) return pcx16_apply_t<CT>(s, C, idx, v, z, done);
  if (!s->pcx_rec) HIPCHK(tsx_dev_malloc((void **)&s->pcx_rec, sizeof(double) * (size_t)PCX_REC * g.Nc));
  const int *cidx = idx ? (const int *)s->dd_cidx : (const int *)nullptr;
  if (!s->pcx_valid) {
    const int nbc = (g.ncol + 63) / 64;
    if (idx)
      hipLaunchKernelGGL((tsx_k_pcx_pack_col<CT, true>), dim3(nbc), dim3(64), 0, s->stream, g, C, cidx, s->l1d, s->a11, s->a12, s->albedo,
                         s->pcx_rec);
    else
      hipLaunchKernelGGL((tsx_k_pcx_pack_col<CT, false>), dim3(nbc), dim3(64), 0, s->stream, g, C, cidx, s->l1d, s->a11, s->a12, s->albedo,
                         s->pcx_rec);
    HIPCHK(hipGetLastError());
    s->pcx_valid = true;
  }
  const int nthr = g.ym * (g.xm / 2), nb = (nthr + PCX_CW - 1) / PCX_CW;
  const int P = s->pc_sweeps + 1;
  // colour-split copies of the right-hand side and the iterate (one allocation: [v | z])
  if (!s->pcx_vz) HIPCHK(tsx_dev_malloc((void **)&s->pcx_vz, sizeof(double) * 2 * (size_t)g.N));
  double *vs = s->pcx_vz, *zs = s->pcx_vz + (size_t)g.N;
  hipLaunchKernelGGL(tsx_k_pcx_permute, dim3(grid_for(g.N, 8192)), dim3(TSX_BLOCK), 0, s->stream, g, 1, v, vs, done);
  const double *vin = v;
  double *zout = z;
  v = vs;
  z = zs;
#define TSX_PCX_GO(L)                                                                                                                    \
  do {                                                                                                                                   \
    if (idx && pass > 0)                                                                                                                 \
      hipLaunchKernelGGL((tsx_k_pcx_rb<CT, L, true, true>), dim3(nb), dim3(PCX_CW *PCX_NSEG), 0, s->stream, g, C, cidx,                   \
                         (const double *)s->pcx_rec, s->l1d, v, z, (const double *)z, done, pass & 1);                                    \
    else if (idx)                                                                                                                        \
      hipLaunchKernelGGL((tsx_k_pcx_rb<CT, L, true, false>), dim3(nb), dim3(PCX_CW *PCX_NSEG), 0, s->stream, g, C, cidx,                  \
                         (const double *)s->pcx_rec, s->l1d, v, z, (const double *)z, done, pass & 1);                                    \
    else if (pass > 0)                                                                                                                   \
      hipLaunchKernelGGL((tsx_k_pcx_rb<CT, L, false, true>), dim3(nb), dim3(PCX_CW *PCX_NSEG), 0, s->stream, g, C, cidx,                  \
                         (const double *)s->pcx_rec, s->l1d, v, z, (const double *)z, done, pass & 1);                                    \
    else                                                                                                                                 \
      hipLaunchKernelGGL((tsx_k_pcx_rb<CT, L, false, false>), dim3(nb), dim3(PCX_CW *PCX_NSEG), 0, s->stream, g, C, cidx,                 \
                         (const double *)s->pcx_rec, s->l1d, v, z, (const double *)z, done, pass & 1);                                    \
  } while (0)
  for (int pass = 0; pass < P; ++pass) {
    if (g.Nz <= 4 * PCX_NSEG) TSX_PCX_GO(4);
    else if (g.Nz <= 8 * PCX_NSEG) TSX_PCX_GO(8);
    else TSX_PCX_GO(16);
  }
#undef TSX_PCX_GO
  (void)vin;
  hipLaunchKernelGGL(tsx_k_pcx_permute, dim3(grid_for(g.N, 8192)), dim3(TSX_BLOCK), 0, s->stream, g, 0, (const double *)zs, zout, done);
  HIPCHK(hipGetLastError());
  return TSX_OK;
}

// z = M^-1 v, both fp64 in the Krylov layout; pc_sweeps + 1 half-grid passes, colours alternately
int tsx_pcx_apply(tsx_solver *s, const double *v, double *z, const int *done) {
  if (s->dd_on && s->coef_bytes == 4) return pcx_apply_t<float>(s, (const float *)s->dd_coef_e, true, v, z, done);
  if (!s->coef_dense_valid) {
    tsx_set_error("exact scan preconditioner: neither shared blocks nor dense planes are valid (internal state error)");
    return TSX_ERR_STATE;
  }
  if (s->coef_bytes == 4) return pcx_apply_t<float>(s, (const float *)s->coef, false, v, z, done);
  return pcx_apply_t<double>(s, (const double *)s->coef, false, v, z, done);
}
