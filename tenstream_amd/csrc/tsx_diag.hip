// tsx_diag.hip -- measurements and diagnostics beside the solver: the bandwidth probes, the log events with their roctx ranges, and
// the reader of a code object as it sits in device memory.
#include <dlfcn.h>
#include <stdlib.h>

#include "tsx_host.hpp"

// ---- bandwidth probes: what this device's memory system delivers to plain streaming kernels, as a ceiling to report the
// rooflines against beside the nominal 8 TB/s (MI355X_MICROARCH.md: about 6.3 TB/s achievable).  U independent 16-byte
// accesses per lane in flight, a capped grid with a grid-stride loop, optionally non-temporal; the best variant counts.
typedef float tsx_f4v __attribute__((ext_vector_type(4)));  // a native vector: the non-temporal builtins take no HIP_vector_type
template <int U, bool NT>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_copy16u(long long n, const tsx_f4v *__restrict__ a, tsx_f4v *__restrict__ b) {
  const long long stride = (long long)gridDim.x * TSX_BLOCK;
  long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x;
  for (; q + (U - 1) * stride < n; q += U * stride) {
    tsx_f4v v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(&a[q + u * stride]) : a[q + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (NT) __builtin_nontemporal_store(v[u], &b[q + u * stride]);
      else b[q + u * stride] = v[u];
    }
  }
  for (; q < n; q += stride) b[q] = a[q];
}
template <int U, bool NT>
__global__ __launch_bounds__(TSX_BLOCK) void tsx_k_read16u(long long n, const tsx_f4v *__restrict__ a, float *__restrict__ out) {
  const long long stride = (long long)gridDim.x * TSX_BLOCK;
  long long q = (long long)blockIdx.x * TSX_BLOCK + threadIdx.x;
  float acc = 0.0f;
  for (; q + (U - 1) * stride < n; q += U * stride) {
    tsx_f4v v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(&a[q + u * stride]) : a[q + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) acc += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
  }
  for (; q < n; q += stride) acc += a[q][0];
  if (acc == 123.456f) out[blockIdx.x] = acc;  // keeps the loads alive; the buffer holds a different constant
}

// best copy (read + write bytes) and best read rate over the variants, GB/s; variant ids for the record
static int probe_bandwidth(tsx_solver *s, size_t bytes, int reps, double *copy_gbps, double *read_gbps, int *copy_variant,
                           int *read_variant) {
  HIPCHK(hipSetDevice(s->device));
  TsxDevTmp A, B;
  HIPCHK(A.alloc(bytes));
  HIPCHK(B.alloc(bytes));
  HIPCHK(hipMemsetAsync(A.p, 1, bytes, s->stream));
  HIPCHK(hipMemsetAsync(B.p, 0, bytes, s->stream));
  const long long n = (long long)(bytes / 16);
  const tsx_f4v *a = A.as<tsx_f4v>();
  tsx_f4v *b = B.as<tsx_f4v>();
  const int grids[3] = {2048, 4096, 16384};
  double best_c = 0, best_r = 0;
  int vc = -1, vr = -1;
  auto timed = [&](auto launch, double moved, double *best, int *bv, int id) -> int {
    launch();  // warm
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    for (int q = 0; q < reps; ++q) launch();
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    const double g = moved * reps / (ms * 1e-3) / 1e9;
    if (g > *best) {
      *best = g;
      *bv = id;
    }
    return TSX_OK;
  };
  int rc;
  for (int gi = 0; gi < 3; ++gi) {
    const int nb = (int)(n / TSX_BLOCK < grids[gi] ? (n / TSX_BLOCK > 0 ? n / TSX_BLOCK : 1) : grids[gi]);
#define TSX_PROBE(U, NT, ID)                                                                                                        \
  if ((rc = timed([&] { hipLaunchKernelGGL((tsx_k_copy16u<U, NT>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, n, a, b); },            \
                  2.0 * (double)(n * 16), &best_c, &vc, gi * 10 + ID)))                                                             \
    return rc;                                                                                                                      \
  if ((rc = timed([&] { hipLaunchKernelGGL((tsx_k_read16u<U, NT>), dim3(nb), dim3(TSX_BLOCK), 0, s->stream, n, a, (float *)b); },   \
                  (double)(n * 16), &best_r, &vr, gi * 10 + ID)))                                                                   \
    return rc;
    TSX_PROBE(1, false, 0)
    TSX_PROBE(4, false, 1)
    TSX_PROBE(8, false, 2)
    TSX_PROBE(4, true, 3)
    TSX_PROBE(8, true, 4)
#undef TSX_PROBE
  }
  HIPCHK(hipGetLastError());
  *copy_gbps = best_c;
  *read_gbps = best_r;
  if (copy_variant) *copy_variant = vc;
  if (read_variant) *read_variant = vr;
  return TSX_OK;
}

extern "C" int tsx_probe_copy_bandwidth(tsx_solver *s, size_t bytes, int reps, double *gbps) {
  ARGCHK(s && gbps && reps >= 1 && bytes >= 16, "tsx_probe_copy_bandwidth: bad argument");
  double r = 0;
  return probe_bandwidth(s, bytes, reps, gbps, &r, nullptr, nullptr);
}
// out4: best copy GB/s (bytes read + written), best read GB/s, and the variants that gave them (grid index * 10 + kernel id:
// kernel 0 one access per lane, 1 / 2 four / eight in flight, 3 / 4 the same non-temporal; grids 2048, 4096, 16384 workgroups)
extern "C" int tsx_probe_bandwidth(tsx_solver *s, size_t bytes, int reps, double *out4) {
  ARGCHK(s && out4 && reps >= 1 && bytes >= 16, "tsx_probe_bandwidth: bad argument");
  int vc = -1, vr = -1;
  int rc = probe_bandwidth(s, bytes, reps, &out4[0], &out4[1], &vc, &vr);
  out4[2] = vc;
  out4[3] = vr;
  return rc;
}

// ---- log events + roctx ranges (TsxLog, tsx_internal.hpp).  roctx comes from librocprofiler-sdk-roctx (ROCm 7; libroctx64 before
// it), bound at run time on first use: libtsx links neither, and without the library the ranges are no-ops.
static const char *const kLogNames[TSX_EV_TOTAL] = {"set_optprop", "get_coeff_diff2diff", "get_coeff_dir2dir", "compute_Edir", "solve_Mdir",
                                                   "setup_diff_src", "compute_Ediff", "setup_Mdiff", "solve_Mdiff", "compute_absorption",
                                                   "get_result", "solve_twostream", "solve_schwarzschild"};
struct TsxRoctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  TsxRoctx() {
    void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static TsxRoctx &tsx_roctx() {
  static TsxRoctx r;
  return r;
}
static void tsx_log_retire(tsx_solver *s, bool wait) {
  TsxLog *L = s->log;
  size_t keep = 0;
  for (size_t q = 0; q < L->pending.size(); ++q) {
    TsxLogPending &p = L->pending[q];
    bool ready = hipEventQuery(p.b) == hipSuccess;
    if (!ready && wait) ready = hipEventSynchronize(p.b) == hipSuccess;
    float ms = 0;
    if (ready && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      L->ms[p.ev] += ms;
      L->pool.push_back(p.a);
      L->pool.push_back(p.b);
    } else if (ready) {  // (an event pair that cannot be read: drop it)
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    } else {
      L->pending[keep++] = p;
    }
  }
  L->pending.resize(keep);
  (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error of the caller
}
static hipEvent_t tsx_log_event(TsxLog *L) {
  hipEvent_t e = nullptr;
  if (!L->pool.empty()) {
    e = L->pool.back();
    L->pool.pop_back();
  } else if (hipEventCreate(&e) != hipSuccess) {
    e = nullptr;
  }
  return e;
}
void tsx_log_begin(tsx_solver *s, int ev, hipEvent_t *a) {
  TsxRoctx &r = tsx_roctx();
  if (r.push) r.push(kLogNames[ev]);
  *a = tsx_log_event(s->log);
  if (*a) (void)hipEventRecord(*a, s->stream);
}
void tsx_log_end(tsx_solver *s, int ev, hipEvent_t a) {
  TsxLog *L = s->log;
  TsxRoctx &r = tsx_roctx();
  L->count[ev] += 1;
  hipEvent_t b = a ? tsx_log_event(L) : nullptr;
  if (b && hipEventRecord(b, s->stream) == hipSuccess) {
    L->pending.push_back({ev, a, b});
    if (L->pending.size() > 256) tsx_log_retire(s, false);
  }
  if (r.pop) r.pop();
}
void tsx_log_free(tsx_solver *s) {
  if (!s->log) return;
  tsx_log_retire(s, true);
  for (hipEvent_t e : s->log->pool) (void)hipEventDestroy(e);
  delete s->log;
  s->log = nullptr;
}
extern "C" int tsx_log_enable(tsx_solver *s, int on) {
  ARGCHK(s, "tsx_log_enable: null");
  HIPCHK(hipSetDevice(s->device));
  if (on && !s->log) s->log = new TsxLog();
  if (!on) tsx_log_free(s);
  return TSX_OK;
}
extern "C" int tsx_log_get(tsx_solver *s, int32_t *nevents, const char **names, int64_t *counts, double *ms) {
  ARGCHK(s && nevents, "tsx_log_get: null");
  *nevents = TSX_EV_COUNT;
  if (!s->log) {
    tsx_set_error("tsx_log_get: log events are off (tsx_log_enable, or TSX_LOG=1 at tsx_create)");
    return TSX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  tsx_log_retire(s, true);
  int n = 0;
  for (int q = 0; q < TSX_EV_TOTAL; ++q) {
    if (q >= TSX_EV_COUNT && s->log->count[q] == 0) continue;  // the 1-D solvers' events: listed once they have fired
    if (names) names[n] = kLogNames[q];
    if (counts) counts[n] = s->log->count[q];
    if (ms) ms[n] = s->log->ms[q];
    ++n;
  }
  *nevents = n;
  return TSX_OK;
}

// ---- diagnostics: a translation unit's code as it sits in device memory (TSX_CODE_PROBE, tsx_host.hpp).  unit 0..10 = api, spmv310,
// spmv816, pc, pcs, pcsflow, dedup, peer, coeff, pipeline, diag (the order of the code objects in libtsx.so is the link order, scripts/code_verify.py finds
// them by the probe's symbol).  Copies nwords 32-bit words from (probe's pc + delta) to host_out and returns the pc in *pc_out; with
// nwords = 0 only the pc.  The caller is responsible for the range lying inside the loaded code object.
extern "C" int tsx_debug_code_read(int device, int unit, long long delta, long long nwords, void *host_out, unsigned long long *pc_out) {
  ARGCHK(unit >= 0 && unit < 11 && nwords >= 0 && pc_out && (nwords == 0 || host_out), "tsx_debug_code_read: bad arguments");
  if (device >= 0) HIPCHK(hipSetDevice(device));
  typedef int (*probe_fn)(long long, long long, unsigned *, unsigned long long *, hipStream_t);
  static const probe_fn probes[11] = {tsx_code_probe_api, tsx_code_probe_spmv310, tsx_code_probe_spmv816, tsx_code_probe_pc,
                                      tsx_code_probe_pcs, tsx_code_probe_pcsflow, tsx_code_probe_dedup, tsx_code_probe_peer,
                                      tsx_code_probe_coeff, tsx_code_probe_pipeline, tsx_code_probe_diag};
  TsxDevTmp out, pc;
  HIPCHK(out.alloc(sizeof(unsigned) * (size_t)(nwords > 0 ? nwords : 1)));
  HIPCHK(pc.alloc(sizeof(unsigned long long)));
  if (probes[unit](delta, nwords, out.as<unsigned>(), pc.as<unsigned long long>(), nullptr)) {
    tsx_set_error("tsx_debug_code_read: launch failed");
    return TSX_ERR_HIP;
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(pc_out, pc.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (nwords > 0) HIPCHK(hipMemcpy(host_out, out.p, sizeof(unsigned) * (size_t)nwords, hipMemcpyDeviceToHost));
  return TSX_OK;
}

TSX_CODE_PROBE(diag)  // tsx_host.hpp: this unit's code object as it sits in device memory (diagnostics)
