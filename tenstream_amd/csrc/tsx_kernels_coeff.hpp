// tsx_kernels_coeff.hpp -- kernels of the diffuse coefficients: the cells' LUT coordinates, the lookup of every cell's block, the
// conversion of blocks and cell fields between the reference's layout and the planes.  Included by tsx_coeff.hip only (the kernels
// without template parameters would otherwise be defined twice).
#pragma once
#include "tsx_dev.hpp"
#include "tsx_lut_dev.hpp"  // TsxLutDev, bisection, N-linear weights, one block's interpolation (shared with tsx_dedup.hip)

// The LUT coordinates of every cell before clamping, (aspect, w0, tauz, g) as float32 exactly as src/pprts_base.F90:1517-1533
// forms them, in CELL order: the optical properties arrive level-fastest, the coefficient kernels run column-fastest, and a lane
// that fetches four doubles 512 bytes apart from its neighbour's moves 64 bytes for every 8 it uses (1 GB for 134 MB at
// 256 x 256 x 64).  A tile of 32 columns x 32 levels goes through LDS: read along the levels, written along the columns.
// Grid: (ceil(ncol / 32), ceil(Nz / 32)), 256 threads.
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_cell_samples(TsxGeo g, const double *__restrict__ kabs, const double *__restrict__ ksca,
                                                                const double *__restrict__ gg, const double *__restrict__ dz, double dx,
                                                                float4 *__restrict__ out) {
  constexpr int TC = 32, TK = 32;
  __shared__ float4 tile[TK][TC + 1];
  const int Nz = g.Nz, ncol = g.ncol;
  const int c0 = blockIdx.x * TC, k0 = blockIdx.y * TK;
  for (int e = threadIdx.x; e < TC * TK; e += TSX_BLOCK) {
    const int kk = e % TK, cc = e / TK;
    const int col = c0 + cc, k = k0 + kk;
    if (col >= ncol || k >= Nz) continue;
    const size_t r = (size_t)k + (size_t)Nz * col;  // col = i + xm * j
    const double ka = kabs[r], ks = ksca[r], dzz = dz[r];
    tile[kk][cc] = make_float4((float)(dzz / dx), (float)(ks / fmax(ka + ks, 2.220446049250313e-16)), (float)((ka + ks) * dzz), (float)gg[r]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TC * TK; e += TSX_BLOCK) {
    const int cc = e % TC, kk = e / TC;
    const int col = c0 + cc, k = k0 + kk;
    if (col >= ncol || k >= Nz) continue;
    out[(size_t)k * ncol + col] = tile[kk][cc];
  }
}

// diffuse coefficients for every 3-D cell -> planes C[q*Nc + cell] (float).  Inputs in reference layout (k fastest), or -- samp
// != null -- the cells' LUT coordinates from tsx_k_cell_samples.
template <int DD>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_lut_diff2diff(TsxGeo g, TsxLutDev L, const double *__restrict__ kabs,
                                                                 const double *__restrict__ ksca, const double *__restrict__ gg,
                                                                 const double *__restrict__ dz, double dx,
                                                                 const uint8_t *__restrict__ l1d, float *__restrict__ C,
                                                                 unsigned long long *__restrict__ hash,
                                                                 const float4 *__restrict__ samp) {
  // hash (nullable): the block's 64-bit hash for the shared storage, taken while the block is in registers (tsx_dedup.hip
  // would otherwise read all planes again for it)
  const int xm = g.xm, ym = g.ym, Nz = g.Nz;
  const long long Nc = g.Nc;
  for (long long c = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; c < Nc; c += (long long)gridDim.x * TSX_BLOCK) {
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    if (l1d[k]) {  // no block in a 1-D layer: zeros, as the shared storage's 1-D entry holds (the operator never reads them; the
                   // export does -- the planes come from the pool and may hold anything)
#pragma unroll
      for (int q = 0; q < DD; ++q) C[(size_t)q * Nc + c] = 0.0f;
      if (hash) hash[c] = TSX_DD_H1D;
      continue;
    }
    // src/pprts_base.F90:1517-1533
    float aspect, w0, tauz, gcell;
    if (samp) {
      const float4 v = samp[c];
      aspect = v.x, w0 = v.y, tauz = v.z, gcell = v.w;
    } else {
      const size_t r = (size_t)k + (size_t)Nz * ((size_t)i + (size_t)xm * j);
      const double ka = kabs[r], ks = ksca[r], dzz = dz[r];
      aspect = (float)(dzz / dx);
      w0 = (float)(ks / fmax(ka + ks, 2.220446049250313e-16));
      tauz = (float)((ka + ks) * dzz);
      gcell = (float)gg[r];
    }
    float acc[DD];
    tsx_lut_diff_block<DD>(L, tsx_lut_diff_clamp(L, make_float4(aspect, w0, tauz, gcell)), acc);
#pragma unroll
    for (int q = 0; q < DD; ++q) C[(size_t)q * Nc + c] = acc[q];
    if (hash) {
      unsigned long long hv = TSX_DD_SEED;
#pragma unroll
      for (int q = 0; q < DD; ++q) hv = tsx_dd_hash_step(hv, q, acc[q]);
      hash[c] = tsx_dd_hash_final(hv);
    }
  }
}

// planes -> reference block layout (c fastest, then k, i, j), as real64: what solver%diff2diff holds
template <typename CT>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_export_coeff(TsxGeo g, int DD, const CT *__restrict__ C,
                                                                double *__restrict__ ref) {
  const int xm = g.xm, ym = g.ym, Nz = g.Nz;
  const long long total = g.Nc * DD;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * TSX_BLOCK) {
    const long long c = q % g.Nc;
    const int cc = (int)(q / g.Nc);
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    ref[(size_t)cc + (size_t)DD * ((size_t)k + (size_t)Nz * ((size_t)i + (size_t)xm * j))] = (double)C[q];
  }
}

// ------------------------------------------------------------------------------------------------
// Operator values: reference block layout (c = dst*D+src fastest, then k, i, j) -> one plane per c,
// x fastest.  LDS-tiled transpose so both sides coalesce.
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_import_coeff(TsxGeo g, int DD, int TI, const TIN *__restrict__ ref,
                                                                TOUT *__restrict__ C) {
  // one block per (j,k, tile of TI i): tile[TI][DD+1]
  extern __shared__ unsigned char smem_raw[];
  TOUT *tile = reinterpret_cast<TOUT *>(smem_raw);
  const int xm = g.xm, ym = g.ym, Nz = g.Nz;
  const int tiles_x = (xm + TI - 1) / TI;
  const long long nt = (long long)tiles_x * ym * Nz;
  for (long long b = blockIdx.x; b < nt; b += gridDim.x) {
    const int tx = (int)(b % tiles_x);
    const int j = (int)((b / tiles_x) % ym);
    const int k = (int)(b / ((long long)tiles_x * ym));
    const int i0 = tx * TI;
    const int ni = xm - i0 < TI ? xm - i0 : TI;
    for (int q = threadIdx.x; q < ni * DD; q += TSX_BLOCK) {
      const int ii = q / DD, c = q % DD;
      tile[ii * (DD + 1) + c] =
          (TOUT)ref[(size_t)c + (size_t)DD * ((size_t)k + (size_t)Nz * ((size_t)(i0 + ii) + (size_t)xm * j))];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < ni * DD; q += TSX_BLOCK) {
      const int c = q / ni, ii = q % ni;
      C[(size_t)c * g.Nc + ((size_t)k * ym + j) * xm + i0 + ii] = tile[ii * (DD + 1) + c];
    }
    __syncthreads();
  }
}

// flag[0] |= 1 if any value is not exactly representable in fp32
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_check_fp32_lossless(long long n, const double *__restrict__ v,
                                                                       int *__restrict__ flag) {
  int bad = 0;
  for (long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; q < n; q += (long long)gridDim.x * TSX_BLOCK) {
    const double a = v[q];
    if ((double)(float)a != a) bad = 1;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// (k,i,j) reference scalar field (z fastest) -> cell-indexed (i fastest)
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_import_cellfield(TsxGeo g, const double *__restrict__ ref,
                                                                    double *__restrict__ out) {
  const int xm = g.xm, ym = g.ym, Nz = g.Nz;
  for (long long c = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x; c < g.Nc; c += (long long)gridDim.x * TSX_BLOCK) {
    const int i = (int)(c % xm);
    const long long t = c / xm;
    const int j = (int)(t % ym);
    const int k = (int)(t / ym);
    out[c] = ref[(size_t)k + (size_t)Nz * ((size_t)i + (size_t)xm * j)];
  }
}

