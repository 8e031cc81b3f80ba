// amg_api.cpp -- C-ABI: context, matrices, vectors and the per-kernel entry
// points that replace the reference's SEQ_* / SMEM_* kernels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "amg_async.h"
#include "amg_eig.h"

#include <csignal>
#include <execinfo.h>
#include <unistd.h>

// AMG_SEGV_TRACE=1: a host SIGSEGV / SIGBUS / SIGABRT prints the native backtrace
// (frames as libamg_mi355x.so(+offset), for addr2line), then hands the signal
// to the handler that was installed before (Python's faulthandler prints the
// threads' Python stacks) -- the diagnostic for teardown faults of multi-rank
// tests.  backtrace() is called once at install so that libgcc is loaded
// before any fault (loading it inside the handler would allocate).
namespace {
struct sigaction g_prev_segv, g_prev_bus, g_prev_abrt;
void amg_fault_trace(int sig, siginfo_t *si, void *uc)
{
   char msg[96];
   const int m = snprintf(msg, sizeof(msg), "[amg] signal %d at address %p, native backtrace:\n", sig, si->si_addr);
   if (m > 0) (void)!write(2, msg, (size_t)m);
   void *buf[64];
   const int n = backtrace(buf, 64);
   backtrace_symbols_fd(buf, n, 2);
   const struct sigaction &prev = sig == SIGSEGV ? g_prev_segv : sig == SIGBUS ? g_prev_bus : g_prev_abrt;
   if ((prev.sa_flags & SA_SIGINFO) && prev.sa_sigaction) {
      prev.sa_sigaction(sig, si, uc);
   } else if (prev.sa_handler != SIG_DFL && prev.sa_handler != SIG_IGN && prev.sa_handler) {
      prev.sa_handler(sig);
   }
   signal(sig, SIG_DFL);
   raise(sig);
}
__attribute__((constructor)) void amg_fault_trace_init()
{
   const char *e = std::getenv("AMG_SEGV_TRACE");
   if (!e || std::atoi(e) == 0) return;
   void *warm[4];
   (void)backtrace(warm, 4);
   struct sigaction sa;
   std::memset(&sa, 0, sizeof(sa));
   sa.sa_sigaction = amg_fault_trace;
   sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
   sigaction(SIGSEGV, &sa, &g_prev_segv);
   sigaction(SIGBUS, &sa, &g_prev_bus);
   sigaction(SIGABRT, &sa, &g_prev_abrt); // heap-check / assertion aborts
}
} // namespace

static thread_local std::string g_last_error;

int amg_set_error(int code, const char *fmt, ...)
{
   char buf[1024];
   va_list ap;
   va_start(ap, fmt);
   vsnprintf(buf, sizeof(buf), fmt, ap);
   va_end(ap);
   g_last_error = buf;
   return code;
}

extern "C" const char *amg_last_error(void) { return g_last_error.c_str(); }
extern "C" int amg_version(void) { return 1; }

extern "C" void amg_opts_default(amg_opts *o)
{
   std::memset(o, 0, sizeof(*o));
   // SMEM_Main.cpp:65-105
   o->solver = AMG_MULT;
   o->smoother = AMG_JACOBI;
   o->num_pre_smooth_sweeps = 1;
   o->num_post_smooth_sweeps = 1;
   o->num_fine_smooth_sweeps = 1;
   o->num_coarse_smooth_sweeps = 1;
   o->smooth_weight = 1.0;
   o->num_cycles = 20;
   o->tol = 1e-9;
   o->check_resnorm = 1;
   o->cheby_flag = 0;
   o->num_threads = 1;
   o->jgs_block_rows = 64;
   o->reuse_outer_residual = 0;
   o->async_type = AMG_FULL_ASYNC;
   o->profile = 0;
   o->accel_type = AMG_NO_ACCEL; // DMEM_Main.cpp:130
   o->cheby_grid = 0;            // DMEM_Main.cpp:142
   o->delay_type = AMG_DELAY_NONE; // SMEM_Main.cpp:98-101
   o->delay_usec = 0;
   o->delay_frac = 0.0;
   o->fail_iter = 0;
   o->delay_rank = -1; // DMEM_DelayProc: every rank (DMEM_Misc.cpp:670-676)
   o->max_inflight = 1;            // DMEM_Main.cpp:113
   o->async_comm_save_divisor = 1; // DMEM_Main.cpp:123
   o->sps_probability_type = AMG_SPS_EXPONENTIAL; // DMEM_Main.cpp:119-121
   o->sps_alpha = 1.0;
   o->sps_min_prob = 0.0;
   o->delay_level = -1;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int amg_init(amg_ctx **out, int device, int nstreams)
{
   AMG_ARG(out, "amg_init: null out");
   int ndev = 0;
   AMG_HIP(hipGetDeviceCount(&ndev));
   AMG_ARG(device >= 0 && device < ndev, "amg_init: device %d of %d", device, ndev);
   AMG_HIP(hipSetDevice(device));
   amg_ctx *c = new amg_ctx();
   c->device = device;
   AMG_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
   // AMG_COMM_PRIORITY=1: the communication stream at the greatest priority
   // (a hardware queue of its own).  Measured at 512^3, 2 ranks, the box's
   // default 4 queues (profiles/r06/ajac): high priority 0.67-0.92 of each
   // sweep's exchange hidden with 0.10 ms exchange windows, normal priority
   // 0.92 with 0.02-0.03 ms windows -- normal is the default
   {
      int least = 0, greatest = 0;
      const char *v = std::getenv("AMG_COMM_PRIORITY");
      const bool hi = v && std::atoi(v) != 0;
      if (hi && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least) {
         AMG_HIP(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, greatest));
      } else {
         (void)hipGetLastError();
         AMG_HIP(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
      }
   }
   for (int i = 0; i < std::max(0, nstreams); i++) {
      hipStream_t s;
      AMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      c->level_streams.push_back(s);
   }
   AMG_HIP(hipMalloc(&c->d_scalars, 8192 * sizeof(double)));
   AMG_HIP(hipMemset(c->d_scalars, 0, 8192 * sizeof(double)));
   AMG_HIP(hipMalloc(&c->d_err, 64));
   AMG_HIP(hipMemset(c->d_err, 0, 64));
   AMG_HIP(hipHostMalloc(&c->h_pinned, 1024 * sizeof(double)));
   hipDeviceProp_t prop;
   if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
   if (hipDeviceGetAttribute(&c->wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || c->wall_khz <= 0)
      c->wall_khz = 100000; // gfx9 s_memrealtime: 100 MHz
   if (const char *v = std::getenv("AMG_VALUE_INDEX")) c->value_index = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_DICT_INDEX")) c->dict_index = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_ROW_PATTERN")) c->row_pattern = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_PAIR_PATTERN")) c->pair_pattern = std::min(2, std::max(0, std::atoi(v)));
   if (const char *v = std::getenv("AMG_MASTER_PATTERN")) c->master_pattern = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_PAIR_ANCHOR16")) c->pair_anchor16 = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_PLANE_MARCH")) {
      c->plane_march = std::atoi(v) > 0;
      if (std::atoi(v) > 1) c->mz_zc = std::min(std::atoi(v), 64), c->mz_zc_auto = 0;
   }
   if (const char *v = std::getenv("AMG_PLANE_MARCH_XCD")) c->mz_xcd = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_FUSE_TRANSFER")) c->fuse_transfer = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_FUSE_XFER")) c->fuse_xfer = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_GRAPHS")) c->graphs = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_LONG_FORM")) c->long_form = std::max(0, std::min(2, std::atoi(v)));
   if (const char *v = std::getenv("AMG_LONG_XCD")) c->long_xcd = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_OUTER_SLAB")) c->outer_slab = std::max(1, std::atoi(v));
   if (const char *v = std::getenv("AMG_FUSE_OUTER")) c->fuse_outer = std::max(0, std::min(4, std::atoi(v)));
   if (const char *v = std::getenv("AMG_FUSE_XFP_SLAB")) c->fuse_xfp_slab = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_FUSE_PROLONG")) c->fuse_prolong = std::max(0, std::min(7, std::atoi(v)));
   if (const char *v = std::getenv("AMG_JGS_SMALL")) c->jgs_small = std::max(0, std::min(2, std::atoi(v)));
   if (const char *v = std::getenv("AMG_JGS_WAVE")) c->jgs_wave = std::max(0, std::min(3, std::atoi(v)));
   if (const char *v = std::getenv("AMG_JGS_FOLD")) c->jgs_fold = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_BSR3")) c->bsr3 = std::max(0, std::min(std::atoi(v), 2));
   if (const char *v = std::getenv("AMG_BSR3_XS")) c->bsr3_xs = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_MZ_EDGE")) c->mz_edge = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_MZ27_OCC")) c->mz27_occ = std::max(-1, std::min(8, std::atoi(v)));
   if (const char *v = std::getenv("AMG_MZ_OCC")) c->mz_occ = std::max(-1, std::min(8, std::atoi(v)));
   if (const char *v = std::getenv("AMG_MZ_PF")) c->mz_pf = std::atoi(v) == 2 ? 2 : (std::atoi(v) == 1 ? 1 : 3);
   if (const char *v = std::getenv("AMG_MZ27_PF")) c->mz27_pf = std::atoi(v) == 1 ? 1 : (std::atoi(v) == 3 ? 3 : 2);
   if (const char *v = std::getenv("AMG_RR_LINES")) c->rr_lines = std::atoi(v) == 2 ? 2 : 1;
   if (const char *v = std::getenv("AMG_RR_OCC")) c->rr_occ = std::atoi(v);
   if (const char *v = std::getenv("AMG_RR_FPF")) c->rr_fpf = std::atoi(v);
   if (const char *v = std::getenv("AMG_RR_ZC")) c->rr_zc = std::max(0, std::min(std::atoi(v), 32));
   if (const char *v = std::getenv("AMG_RR_RING")) c->rr_ring = std::atoi(v) != 0;
   if (const char *v = std::getenv("AMG_MZ_NT")) c->mz_nt = std::atoi(v) & 3;
   if (const char *v = std::getenv("AMG_MZ_LINES")) c->mz_lines = std::atoi(v) == 4 ? 4 : std::atoi(v) == 2 ? 2 : 1;
   if (const char *v = std::getenv("AMG_MZ_LINES_GEMV"))
      c->mz_lines_gemv = std::atoi(v) == 4 ? 4 : std::atoi(v) == 2 ? 2 : 1;
   *out = c;
   return AMG_OK;
}

// one process-wide lock around teardown (contexts, hierarchies, matrices):
// ranks that are threads of one process free concurrently, and the runtime's
// free / destroy paths are kept out of each other's way
std::recursive_mutex &amg_teardown_mutex()
{
   static std::recursive_mutex m;
   return m;
}

extern "C" int amg_finalize(amg_ctx *c)
{
   if (!c) return AMG_OK;
   std::lock_guard<std::recursive_mutex> td(amg_teardown_mutex());
   hipSetDevice(c->device);
   hipStreamSynchronize(c->stream);
   if (c->comm_stream) hipStreamSynchronize(c->comm_stream);
   for (auto s : c->level_streams) {
      hipStreamSynchronize(s);
      hipStreamDestroy(s);
   }
   if (c->comm_stream) hipStreamDestroy(c->comm_stream);
   hipStreamDestroy(c->stream);
   hipFree(c->d_partials);
   hipFree(c->d_scalars);
   hipFree(c->d_err);
   hipHostFree(c->h_pinned);
   delete c;
   return AMG_OK;
}

// device-side range-check flags since the last call (bit 0: a zero-guess fold
// write outside the coarse level's rows, dropped), cleared on read
extern "C" int amg_device_errors(amg_ctx *c, int *flags)
{
   AMG_ARG(c && flags, "amg_device_errors: null argument");
   int h[16];
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_HIP(hipMemcpy(h, c->d_err, sizeof(h), hipMemcpyDeviceToHost));
   AMG_HIP(hipMemset(c->d_err, 0, sizeof(h)));
   *flags = h[0];
   return AMG_OK;
}

extern "C" int amg_sync(amg_ctx *c)
{
   AMG_ARG(c, "amg_sync: null ctx");
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

int amg_ctx_partials(amg_ctx *c, size_t n, double **out)
{
   if (n > c->partials_cap) {
      // grow only at points where the stream may be synchronised
      AMG_HIP(hipStreamSynchronize(c->stream));
      hipFree(c->d_partials);
      c->d_partials = nullptr;
      size_t cap = std::max<size_t>(n, 1 << 16);
      AMG_HIP(hipMalloc(&c->d_partials, cap * sizeof(double)));
      c->partials_cap = cap;
   }
   *out = c->d_partials;
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// matrices
// ---------------------------------------------------------------------------
static int mat_alloc(amg_ctx *c, int nrows, int ncols, long long nnz, amg_mat **out)
{
   amg_mat_ptr A(new amg_mat());
   A->ctx = c;
   A->nrows = nrows;
   A->ncols = ncols;
   A->nnz = nnz;
   size_t np = (size_t)nnz + AMG_NNZ_PAD;
   hipError_t e = hipMalloc(&A->rowptr, ((size_t)nrows + 1) * sizeof(int));
   if (e == hipSuccess) e = hipMalloc(&A->col, np * sizeof(int));
   if (e == hipSuccess) e = hipMalloc(&A->val, np * sizeof(double));
   if (e == hipSuccess) e = hipMalloc(&A->diag, std::max(1, nrows) * sizeof(double));
   if (e != hipSuccess)
      return amg_set_error(AMG_ERR_OOM, "amg_csr_register: device allocation of %lld nnz failed: %s",
                           nnz, hipGetErrorString(e));
   // padding: col 0 (a valid x index), val 0
   AMG_HIP(hipMemsetAsync(A->col + nnz, 0, AMG_NNZ_PAD * sizeof(int), c->stream));
   AMG_HIP(hipMemsetAsync(A->val + nnz, 0, AMG_NNZ_PAD * sizeof(double), c->stream));
   *out = A.release();
   return AMG_OK;
}

extern "C" int amg_set_jgs_wave(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_jgs_wave: null context");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->jgs_wave = std::max(0, std::min(3, enable));
   return AMG_OK;
}

extern "C" int amg_set_jgs_small(amg_ctx *c, int form)
{
   AMG_ARG(c, "amg_set_jgs_small: null context");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->jgs_small = std::max(0, std::min(2, form));
   return AMG_OK;
}

extern "C" int amg_set_jgs_fold(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_jgs_fold: null context");
   c->knob_gen++;
   c->jgs_fold = enable != 0;
   return AMG_OK;
}

extern "C" int amg_set_fuse_prolong(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_fuse_prolong: null context");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->fuse_prolong = std::max(0, std::min(7, enable));
   return AMG_OK;
}

extern "C" int amg_set_march_lines(amg_ctx *c, int lines)
{
   AMG_ARG(c && (lines == 1 || lines == 2 || lines == 4), "amg_set_march_lines: lines must be 1, 2 or 4");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->mz_lines = lines;
   c->mz_lines_gemv = lines;
   return AMG_OK;
}

extern "C" int amg_set_march_lines_gemv(amg_ctx *c, int lines)
{
   AMG_ARG(c && (lines == 1 || lines == 2 || lines == 4), "amg_set_march_lines_gemv: lines must be 1, 2 or 4");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->mz_lines_gemv = lines;
   return AMG_OK;
}

extern "C" int amg_set_fuse_outer(amg_ctx *c, int mode)
{
   AMG_ARG(c && mode >= 0 && mode <= 4, "amg_set_fuse_outer: mode 0, 1, 2, 3 or 4");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->fuse_outer = mode;
   return AMG_OK;
}

extern "C" int amg_set_outer_slab(amg_ctx *c, int planes)
{
   AMG_ARG(c && planes >= 1, "amg_set_outer_slab: planes must be >= 1");
   c->knob_gen++;
   c->outer_slab = planes;
   return AMG_OK;
}

extern "C" int amg_set_long_form(amg_ctx *c, int form, int xcd)
{
   AMG_ARG(c && form >= 0 && form <= 2, "amg_set_long_form: form 0, 1 or 2");
   c->knob_gen++;
   c->long_form = form;
   c->long_xcd = xcd != 0;
   return AMG_OK;
}

extern "C" int amg_set_graphs(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_graphs: null context");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->graphs = enable != 0;
   return AMG_OK;
}

extern "C" int amg_set_march_tuning(amg_ctx *c, int mz_pf, int mz27_pf, int mz_occ, int mz27_occ)
{
   AMG_ARG(c, "amg_set_march_tuning: null context");
   AMG_ARG(mz_pf == -2 || (mz_pf >= 1 && mz_pf <= 3), "amg_set_march_tuning: 7-pt prefetch distance %d", mz_pf);
   AMG_ARG(mz27_pf == -2 || mz27_pf == 1 || mz27_pf == 2 || mz27_pf == 3,
           "amg_set_march_tuning: 27-pt prefetch distance %d (3: the LDS plane ring)",
           mz27_pf);
   AMG_ARG(mz_occ >= -2 && mz_occ <= 8 && mz27_occ >= -2 && mz27_occ <= 8,
           "amg_set_march_tuning: occupancy %d / %d outside [-1, 8]", mz_occ, mz27_occ);
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   if (mz_pf != -2) c->mz_pf = mz_pf;
   if (mz27_pf != -2) c->mz27_pf = mz27_pf;
   if (mz_occ != -2) c->mz_occ = mz_occ;
   if (mz27_occ != -2) c->mz27_occ = mz27_occ;
   return AMG_OK;
}

extern "C" int amg_set_fuse_transfer(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_fuse_transfer: null context");
   c->knob_gen++; // cached hipGraphs were captured with the old setting
   c->fuse_transfer = enable ? 1 : 0;
   return AMG_OK;
}

int amg_mat_create_device(amg_ctx *c, int nrows, int ncols, long long nnz, amg_mat **out)
{
   return mat_alloc(c, nrows, ncols, nnz, out);
}

extern "C" int amg_csr_register(amg_ctx *c, int nrows, int ncols, long long nnz, const int *rowptr,
                                const int *col, const double *val, int diag_first, amg_mat **out)
{
   AMG_ARG(c && out && rowptr && (nnz == 0 || (col && val)), "amg_csr_register: null argument");
   AMG_ARG(nrows >= 0 && ncols >= 0 && nnz >= 0, "amg_csr_register: negative size");
   AMG_ARG(nnz < (1LL << 31) - AMG_NNZ_PAD, "amg_csr_register: nnz %lld exceeds int32 CSR", nnz);
   AMG_ARG(rowptr[nrows] == nnz && rowptr[0] == 0, "amg_csr_register: rowptr[0]=%d rowptr[n]=%d nnz=%lld",
           rowptr[0], rowptr[nrows], nnz);
   AMG_ARG(nrows == 0 || ncols > 0, "amg_csr_register: ncols must be positive");
   amg_mat *raw = nullptr;
   AMG_TRY(mat_alloc(c, nrows, ncols, nnz, &raw));
   amg_mat_ptr A(raw); // freed when a later step fails
   A->diag_first = diag_first;
   AMG_HIP(hipMemcpyAsync(A->rowptr, rowptr, ((size_t)nrows + 1) * sizeof(int),
                          hipMemcpyHostToDevice, c->stream));
   if (nnz) {
      AMG_HIP(hipMemcpyAsync(A->col, col, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, c->stream));
      AMG_HIP(hipMemcpyAsync(A->val, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice,
                             c->stream));
   }
   AMG_TRY(amg_mat_finish(A.get()));
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_TRY(amg_mat_build_bsr3(A.get(), rowptr, col, val));
   *out = A.release();
   return AMG_OK;
}

extern "C" int amg_mat_free(amg_mat *A)
{
   std::lock_guard<std::recursive_mutex> td(amg_teardown_mutex());
   if (!A) return AMG_OK;
   if (A->trans) amg_mat_free(A->trans);
   hipFree(A->rowptr);
   hipFree(A->col);
   hipFree(A->val);
   hipFree(A->diag);
   amg_mat_drop_forms(A);
   delete A;
   return AMG_OK;
}

extern "C" int amg_mat_info(const amg_mat *A, int *nrows, int *ncols, long long *nnz)
{
   AMG_ARG(A, "amg_mat_info: null matrix");
   if (nrows) *nrows = A->nrows;
   if (ncols) *ncols = A->ncols;
   if (nnz) *nnz = A->nnz;
   return AMG_OK;
}

extern "C" int amg_mat_download(amg_ctx *c, const amg_mat *A, int *rowptr, int *col, double *val)
{
   AMG_ARG(c && A, "amg_mat_download: null argument");
   AMG_HIP(hipStreamSynchronize(c->stream));
   if (rowptr)
      AMG_HIP(hipMemcpy(rowptr, A->rowptr, ((size_t)A->nrows + 1) * sizeof(int), hipMemcpyDeviceToHost));
   if (col && A->nnz) AMG_HIP(hipMemcpy(col, A->col, (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToHost));
   if (val && A->nnz) AMG_HIP(hipMemcpy(val, A->val, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// vectors
// ---------------------------------------------------------------------------
extern "C" int amg_vec_create(amg_ctx *c, int n, amg_vec **out)
{
   AMG_ARG(c && out && n >= 0, "amg_vec_create: bad argument");
   amg_vec *v = new amg_vec();
   v->ctx = c;
   v->n = n;
   hipError_t e = hipMalloc(&v->d, std::max(1, n) * sizeof(double));
   if (e != hipSuccess) {
      delete v;
      return amg_set_error(AMG_ERR_OOM, "amg_vec_create(%d): %s", n, hipGetErrorString(e));
   }
   AMG_HIP(hipMemsetAsync(v->d, 0, std::max(1, n) * sizeof(double), c->stream));
   *out = v;
   return AMG_OK;
}

extern "C" int amg_vec_free(amg_vec *v)
{
   if (!v) return AMG_OK;
   if (v->owns) hipFree(v->d);
   delete v;
   return AMG_OK;
}

extern "C" int amg_vec_size(const amg_vec *v) { return v ? v->n : -1; }

extern "C" int amg_vec_upload(amg_ctx *c, amg_vec *v, const double *h)
{
   AMG_ARG(c && v && h, "amg_vec_upload: null argument");
   AMG_HIP(hipMemcpyAsync(v->d, h, (size_t)v->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

extern "C" int amg_vec_download(amg_ctx *c, const amg_vec *v, double *h)
{
   AMG_ARG(c && v && h, "amg_vec_download: null argument");
   AMG_HIP(hipMemcpyAsync(h, v->d, (size_t)v->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

extern "C" int amg_vec_set(amg_ctx *c, amg_vec *v, double a)
{
   AMG_ARG(c && v, "amg_vec_set: null argument");
   amgk::vset(c->stream, v->d, a, 0, v->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_vec_copy(amg_ctx *c, const amg_vec *x, amg_vec *y)
{
   AMG_ARG(c && x && y && x->n == y->n, "amg_vec_copy: size mismatch");
   amgk::vcopy(c->stream, x->d, y->d, 0, x->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_vec_axpy(amg_ctx *c, double a, const amg_vec *x, amg_vec *y)
{
   AMG_ARG(c && x && y && x->n == y->n, "amg_vec_axpy: size mismatch");
   amgk::vaxpy(c->stream, a, x->d, y->d, 0, x->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_vec_ivaxpy(amg_ctx *c, const amg_vec *x, const amg_vec *s, amg_vec *y)
{
   AMG_ARG(c && x && s && y && x->n == y->n && s->n == y->n, "amg_vec_ivaxpy: size mismatch");
   amgk::vivaxpy(c->stream, x->d, s->d, y->d, 0, y->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_vec_scale(amg_ctx *c, double a, amg_vec *y)
{
   AMG_ARG(c && y, "amg_vec_scale: null argument");
   amgk::vscale(c->stream, a, y->d, 0, y->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

int amg_reduce_to_host(amg_ctx *c, const double *partials, int np, int do_sqrt, double *out)
{
   amgk::reduce_partials(c->stream, partials, np, c->d_scalars, do_sqrt, c->d_scalars + 4096);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipMemcpyAsync(c->h_pinned, c->d_scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   *out = c->h_pinned[0];
   return AMG_OK;
}

extern "C" int amg_vec_norm2(amg_ctx *c, const amg_vec *x, double *out)
{
   AMG_ARG(c && x && out, "amg_vec_norm2: null argument");
   double *p;
   AMG_TRY(amg_ctx_partials(c, 1024, &p));
   int np = 0;
   amgk::sumsq_partials(c->stream, x->d, x->n, p, &np);
   return amg_reduce_to_host(c, p, np, 1, out);
}

extern "C" int amg_vec_dot(amg_ctx *c, const amg_vec *x, const amg_vec *y, double *out)
{
   AMG_ARG(c && x && y && out && x->n == y->n, "amg_vec_dot: size mismatch");
   double *p;
   AMG_TRY(amg_ctx_partials(c, 1024, &p));
   int np = 0;
   amgk::dot_partials(c->stream, x->d, y->d, x->n, p, &np);
   return amg_reduce_to_host(c, p, np, 0, out);
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
static int check_range(const amg_mat *A, int rb, int re)
{
   AMG_ARG(rb >= 0 && re <= A->nrows && rb <= re, "row range [%d,%d) outside [0,%d)", rb, re,
           A->nrows);
   return AMG_OK;
}

extern "C" int amg_matvec(amg_ctx *c, const amg_mat *A, const amg_vec *x, amg_vec *y, int rb, int re)
{
   AMG_ARG(c && A && x && y, "amg_matvec: null argument");
   AMG_ARG(x->n >= A->ncols && y->n >= A->nrows, "amg_matvec: vector sizes %d/%d vs %dx%d", x->n,
           y->n, A->nrows, A->ncols);
   AMG_TRY(check_range(A, rb, re));
   amgk::spgemv(c->stream, A, x->d, nullptr, amgk::gemv_mode(1.0, 0.0), y->d, rb, re, nullptr);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_matvec_timed(amg_ctx *c, const amg_mat *A, const amg_vec *x, amg_vec *y,
                                int reps, double *ms)
{
   AMG_ARG(c && A && x && y && ms && reps >= 1, "amg_matvec_timed: bad argument");
   AMG_ARG(x->n >= A->ncols && y->n >= A->nrows, "amg_matvec_timed: vector sizes");
   const amgk::Gemv g = amgk::gemv_mode(1.0, 0.0);
   auto spmv = [&] {
      amgk::spgemv(c->stream, A, x->d, nullptr, g, y->d, 0, A->nrows, nullptr);
      return AMG_OK;
   };
   return amg_timed_reps(c->stream, reps, spmv, ms);
}

// ---------------------------------------------------------------------------
// CG-Lanczos eigenvalue estimate (amg_eig.h; DMEM_Setup.cpp:77-87)
// ---------------------------------------------------------------------------
extern "C" int amg_lehmer_stream(long long seed, long long skip, long long n, double *out)
{
   constexpr unsigned long long m = 2147483647ULL, a = 16807ULL;
   AMG_ARG(seed >= 1 && seed < (long long)m && skip >= 0 && n >= 0 && (out || n == 0),
           "amg_lehmer_stream: seed %lld outside [1, 2^31 - 2], or skip %lld / n %lld negative, or null out", seed,
           skip, n);
   // w <- a^skip w mod m by squaring (every product below 2^62)
   unsigned long long w = (unsigned long long)seed, f = a;
   for (unsigned long long e = (unsigned long long)skip; e; e >>= 1) {
      if (e & 1) w = w * f % m;
      f = f * f % m;
   }
   for (long long i = 0; i < n; i++) {
      w = a * w % m;
      out[i] = (double)w / 2147483647.0;
   }
   return AMG_OK;
}

// eigenvalues of the k x k tridiagonal (td, to) below x, a zero pivot taken as -DBL_MIN
static int sturm_count(int k, const double *td, const double *to, double x)
{
   int cnt = 0;
   double q = td[0] - x;
   if (q == 0.0) q = -DBL_MIN;
   if (q < 0.0) cnt++;
   for (int i = 1; i < k; i++) {
      q = (td[i] - x) - (to[i] * to[i]) / q;
      if (q == 0.0) q = -DBL_MIN;
      if (q < 0.0) cnt++;
   }
   return cnt;
}

extern "C" int amg_lanczos_extremes(int k, const double *alpha, const double *beta, double *tridiag,
                                    double *trioffd, double *eig_max, double *eig_min)
{
   AMG_ARG(alpha && beta && tridiag && trioffd && eig_max && eig_min, "amg_lanczos_extremes: null argument");
   if (k < 1)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "amg_lanczos_extremes: k = %d: no iteration to estimate from", k);
   for (int i = 0; i < k; i++)
      AMG_ARG(std::isfinite(alpha[i]) && alpha[i] != 0.0 && (i == k - 1 || (std::isfinite(beta[i]) && beta[i] >= 0.0)),
              "amg_lanczos_extremes: alpha[%d] = %g, beta[%d] = %g: alpha must be finite and non-zero, beta finite "
              "and not negative", i, alpha[i], i, beta[i]);
   tridiag[0] = 1.0 / alpha[0];
   trioffd[0] = 0.0;
   for (int i = 1; i < k; i++) {
      const double ia = 1.0 / alpha[i - 1];
      tridiag[i] = ia * beta[i - 1] + 1.0 / alpha[i];
      trioffd[i] = ia * std::sqrt(beta[i - 1]);
   }
   double lo = 0.0, hi = 0.0;
   for (int i = 0; i < k; i++) {
      const double rad = std::fabs(trioffd[i]) + (i + 1 < k ? std::fabs(trioffd[i + 1]) : 0.0);
      const double a = tridiag[i] - rad, b = tridiag[i] + rad;
      if (i == 0 || a < lo) lo = a;
      if (i == 0 || b > hi) hi = b;
   }
   AMG_ARG(std::isfinite(lo) && std::isfinite(hi), "amg_lanczos_extremes: the tridiagonal is not finite");
   // bisect [l, h] until the midpoint is one of its ends; below(m): m replaces h, else l
   auto bisect = [&](auto below, double *l, double *h) {
      *l = lo, *h = hi;
      for (double m = 0.5 * (*l + *h); *l < m && m < *h; m = 0.5 * (*l + *h)) *(below(m) ? h : l) = m;
   };
   double l, h;
   bisect([&](double m) { return sturm_count(k, tridiag, trioffd, m) == k; }, &l, &h);
   *eig_max = h; // the upper end: every eigenvalue lies below it
   bisect([&](double m) { return sturm_count(k, tridiag, trioffd, m) >= 1; }, &l, &h);
   *eig_min = l; // the lower end: no eigenvalue lies below it
   return AMG_OK;
}

namespace {
// amg_eig.h's binding: one registered matrix on one GPU; everything it allocates
// lives for one call
struct EigBind {
   amg_ctx *c;
   const amg_mat *A;
   std::vector<void *> owned;
   static constexpr bool gathers = false;
   ~EigBind()
   {
      for (void *p : owned) (void)hipFree(p);
   }
   int n() const { return A->nrows; }
   const double *diag() const { return A->diag; }
   int alloc(size_t m, double **p)
   {
      const size_t bytes = std::max<size_t>(m, 1) * sizeof(double);
      hipError_t e = hipMalloc(p, bytes);
      if (e != hipSuccess)
         return amg_set_error(AMG_ERR_OOM, "amg_eigs_cg: allocation of %zu doubles: %s", m, hipGetErrorString(e));
      owned.push_back(*p);
      AMG_HIP(hipMemsetAsync(*p, 0, bytes, c->stream));
      return AMG_OK;
   }
   int alloc_vec(double **p) { return alloc((size_t)A->ncols, p); }
   int apply_A(const double *x, double *y)
   {
      amgk::spgemv(c->stream, A, x, nullptr, amgk::gemv_mode(1.0, 0.0), y, 0, A->nrows, nullptr);
      return AMG_OK;
   }
};
} // namespace

int amg_eig_start_vector(hipStream_t s, double *r, const double *r0, long long row0, int n)
{
   std::vector<double> u;
   if (!r0) {
      u.resize(std::max(n, 1));
      AMG_TRY(amg_lehmer_stream(1, row0, n, u.data()));
      for (int i = 0; i < n; i++) u[i] = 2.0 * u[i] - 1.0;
      r0 = u.data();
   }
   if (n > 0) AMG_HIP(hipMemcpyAsync(r, r0, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
   AMG_HIP(hipStreamSynchronize(s)); // u is released on return
   return AMG_OK;
}

extern "C" int amg_eigs_cg(amg_ctx *c, const amg_mat *A, int scale, int max_iter, const double *r0, double *eig_max,
                           double *eig_min, double *alpha, double *beta, double *gamma, int *iters)
{
   AMG_ARG(c && A && eig_max && eig_min, "amg_eigs_cg: null argument");
   AMG_ARG(A->nrows == A->ncols && A->nrows >= 1, "amg_eigs_cg: the matrix is %d x %d (square, not empty)", A->nrows,
           A->ncols);
   AMG_ARG((scale == 0 || scale == 1) && max_iter >= 1 && max_iter <= amgk::PCG_RING,
           "amg_eigs_cg: scale %d (0 or 1), max_iter %d (1 .. %d)", scale, max_iter, amgk::PCG_RING);
   EigBind b{c, A, {}};
   AmgEig g;
   const int st = amg_eig::run(b, g, "amg_eigs_cg", scale, max_iter, [&](double *r) {
      return amg_eig_start_vector(c->stream, r, r0, 0, A->nrows);
   }, eig_max, eig_min, alpha, beta, gamma, iters);
   (void)hipStreamSynchronize(c->stream); // nothing of g is in flight when b frees it
   return st;
}

// measurement helpers (declared in the header): PMC calibration streams
// (tools/pmc_traffic.py) and the STREAM-triad ceiling bench.py reports
extern "C" int amg_pmc_calib(amg_ctx *c, int mode, long long bytes)
{
   AMG_ARG(c && mode >= 0 && mode <= 4 && bytes > 0, "amg_pmc_calib: bad argument");
   void *buf = nullptr;
   AMG_HIP(hipMalloc(&buf, (size_t)bytes));
   AMG_HIP(hipMemsetAsync(buf, 1, (size_t)bytes, c->stream));
   amgk::calib_stream(c->stream, mode, buf, bytes, c->d_scalars + 8000);
   AMG_HIP(hipStreamSynchronize(c->stream));
   hipFree(buf);
   return AMG_OK;
}

extern "C" int amg_stream_triad(amg_ctx *c, long long n, int reps, double *gbs)
{
   AMG_ARG(c && n >= 2 && reps >= 1 && gbs, "amg_stream_triad: bad argument");
   n &= ~1LL;
   double *a = nullptr, *b = nullptr, *d = nullptr;
   AMG_HIP(hipMalloc(&a, (size_t)n * 8));
   if (hipMalloc(&b, (size_t)n * 8) != hipSuccess || hipMalloc(&d, (size_t)n * 8) != hipSuccess) {
      hipFree(a);
      hipFree(b);
      return amg_set_error(AMG_ERR_OOM, "amg_stream_triad: %lld doubles", n);
   }
   hipMemsetAsync(b, 0, (size_t)n * 8, c->stream);
   hipMemsetAsync(d, 0, (size_t)n * 8, c->stream);
   auto triad = [&] {
      amgk::stream_triad(c->stream, a, b, d, 3.0, n);
      return AMG_OK;
   };
   triad(); // warm
   double best = 1e30, ms = 0.0;
   int st = AMG_OK;
   for (int r = 0; r < reps && st == AMG_OK; r++) {
      st = amg_timed_reps(c->stream, 1, triad, &ms);
      best = std::min(best, ms);
   }
   const hipError_t err = hipGetLastError();
   hipFree(a);
   hipFree(b);
   hipFree(d);
   AMG_TRY(st);
   AMG_HIP(err);
   *gbs = 24.0 * (double)n / (best * 1e-3) / 1e9;
   return AMG_OK;
}

#ifdef AMG_DEV_TUNE
// development-only tuning entry points (tools/tune_spmv.py), only in the
// development build lib/libamg_mi355x_dev.so (make dev); not in the header
namespace amgk {
int num_tune_variants();
const char *tune_variant_name(int v);
void launch_tune_variant(hipStream_t s, int v, const amg_mat *A, const double *x, double *y);
} // namespace amgk

extern "C" int amg_dev_tune_count(void) { return amgk::num_tune_variants(); }

extern "C" const char *amg_dev_tune_name(int v) { return amgk::tune_variant_name(v); }
extern "C" int amg_dev_tune_spmv(amg_ctx *c, const amg_mat *A, const amg_vec *x, amg_vec *y,
                                 int variant, int reps, double *ms)
{
   AMG_ARG(c && A && x && y && ms && reps >= 1, "amg_dev_tune_spmv: bad argument");
   AMG_ARG(variant >= 0 && variant < amgk::num_tune_variants(), "amg_dev_tune_spmv: variant");
   auto launch = [&] {
      amgk::launch_tune_variant(c->stream, variant, A, x->d, y->d);
      return AMG_OK;
   };
   AMG_TRY(amg_timed_reps(c->stream, reps, launch, ms));
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}
#endif // AMG_DEV_TUNE

extern "C" int amg_spgemv(amg_ctx *c, const amg_mat *A, const amg_vec *x, const amg_vec *b,
                          double alpha, double beta, amg_vec *y, int rb, int re)
{
   AMG_ARG(c && A && x && y, "amg_spgemv: null argument");
   AMG_ARG(x->n >= A->ncols && y->n >= A->nrows, "amg_spgemv: vector sizes");
   AMG_TRY(check_range(A, rb, re));
   amgk::Gemv g = amgk::gemv_mode(alpha, beta);
   AMG_ARG(g.init == 0 || (b && b->n >= A->nrows), "amg_spgemv: b required when beta != 0");
   amgk::spgemv(c->stream, A, x->d, b ? b->d : nullptr, g, y->d, rb, re, nullptr);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_residual(amg_ctx *c, const amg_mat *A, const amg_vec *b, const amg_vec *x,
                            amg_vec *y, amg_vec *r, int rb, int re)
{
   AMG_ARG(c && A && b && x && y && r, "amg_residual: null argument");
   AMG_TRY(check_range(A, rb, re));
   // SMEM_Residual: y = A x over [rb,re), then r = b - y
   amgk::spgemv(c->stream, A, x->d, nullptr, amgk::gemv_mode(1.0, 0.0), y->d, rb, re, nullptr);
   amgk::vsub(c->stream, b->d, y->d, r->d, rb, re);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

static int build_transpose(amg_mat *A);

extern "C" int amg_matvec_t(amg_ctx *c, const amg_mat *A, const amg_vec *x, amg_vec *y, int T)
{
   AMG_ARG(c && A && x && y, "amg_matvec_t: null argument");
   AMG_ARG(x->n >= A->nrows && y->n >= A->ncols, "amg_matvec_t: vector sizes");
   amg_mat *Am = const_cast<amg_mat *>(A);
   if (!Am->trans) AMG_TRY(build_transpose(Am));
   amgk::matvec_t_chunked(c->stream, Am->trans, x->d, y->d, A->nrows, T);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

// transpose on the host once (setup-time; rows of A^T list source rows ascending)
static int build_transpose(amg_mat *A)
{
   amg_ctx *c = A->ctx;
   std::vector<int> rp(A->nrows + 1), cj(A->nnz);
   std::vector<double> cv(A->nnz);
   AMG_TRY(amg_mat_download(c, A, rp.data(), cj.data(), cv.data()));
   std::vector<int> trp(A->ncols + 1, 0), tcj(A->nnz);
   std::vector<double> tcv(A->nnz);
   for (long long k = 0; k < A->nnz; k++) trp[cj[k] + 1]++;
   for (int i = 0; i < A->ncols; i++) trp[i + 1] += trp[i];
   std::vector<int> pos(trp.begin(), trp.end());
   for (int r = 0; r < A->nrows; r++)
      for (int k = rp[r]; k < rp[r + 1]; k++) {
         int col = cj[k];
         tcj[pos[col]] = r;
         tcv[pos[col]] = cv[k];
         pos[col]++;
      }
   return amg_csr_register(c, A->ncols, A->nrows, A->nnz, trp.data(), tcj.data(), tcv.data(), 0,
                           &A->trans);
}

extern "C" int amg_jacobi(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                          amg_vec *u_prev, double omega, int sweeps, int zero_first, int rb,
                          int re, int variant)
{
   AMG_ARG(c && A && f && u && u_prev, "amg_jacobi: null argument");
   AMG_TRY(check_range(A, rb, re));
   for (int k = 0; k < sweeps; k++) {
      if (k == 0 && zero_first == 1) {
         amgk::jacobi_zero(c->stream, A->diag, f->d, nullptr, omega, u->d, rb, re, variant);
      } else {
         // u_prev = u; u = J(u_prev) (SMEM_Smooth.cpp:33-46)
         amgk::vcopy(c->stream, u->d, u_prev->d, 0, u->n);
         amgk::jacobi_sweep(c->stream, A, f->d, u_prev->d, nullptr, omega, u->d, rb, re);
      }
   }
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_l1_jacobi(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                             amg_vec *u_prev, const amg_vec *l1, int sweeps, int zero_first,
                             int rb, int re, int variant)
{
   AMG_ARG(c && A && f && u && u_prev && l1, "amg_l1_jacobi: null argument");
   AMG_TRY(check_range(A, rb, re));
   for (int k = 0; k < sweeps; k++) {
      if (k == 0 && zero_first == 1) {
         amgk::jacobi_zero(c->stream, A->diag, f->d, l1->d, 1.0, u->d, rb, re, variant);
      } else {
         amgk::vcopy(c->stream, u->d, u_prev->d, 0, u->n);
         amgk::jacobi_sweep(c->stream, A, f->d, u_prev->d, l1->d, 1.0, u->d, rb, re);
      }
   }
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

int amg_hybrid_jgs_dev(amg_ctx *c, hipStream_t s, const amg_mat *A, const double *f, double *u,
                       double *u_prev, int n_vec, const int *d_blk, int nblk, int blk_lo,
                       int blk_hi, const double *ds, double weight, int sweeps, int zero_first,
                       int reverse, double *apply_u = nullptr, double *apply_priv = nullptr,
                       bool *applied = nullptr, unsigned long long *stamp = nullptr)
{
   bool ap = false;
   for (int k = 0; k < sweeps; k++) {
      const int zero = (k == 0 && zero_first == 1);
      if (!zero) amgk::vcopy(s, u, u_prev, blk_lo, blk_hi);
      const bool last = k == sweeps - 1;
      ap = amgk::hybrid_jgs(s, A, f, u, u_prev, d_blk, nblk, ds, weight, zero, reverse, last ? apply_u : nullptr,
                            last ? apply_priv : nullptr, last ? stamp : nullptr);
   }
   if (applied) *applied = ap;
   (void)n_vec;
   (void)c;
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_hybrid_jgs(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                              amg_vec *u_prev, const int *blk, int nblk, const amg_vec *diag_scale,
                              double weight, int sweeps, int zero_first, int reverse)
{
   AMG_ARG(c && A && f && u && u_prev && blk && nblk > 0, "amg_hybrid_jgs: null argument");
   for (int b = 0; b < nblk; b++)
      AMG_ARG(blk[b] <= blk[b + 1] && blk[b] >= 0 && blk[b + 1] <= A->nrows,
              "amg_hybrid_jgs: bad block %d [%d,%d)", b, blk[b], blk[b + 1]);
   int *d_blk = nullptr;
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_HIP(hipMalloc((void **)&d_blk, (nblk + 1) * sizeof(int)));
   AMG_HIP(hipMemcpyAsync(d_blk, blk, (nblk + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   int s = amg_hybrid_jgs_dev(c, c->stream, A, f->d, u->d, u_prev->d, u->n, d_blk, nblk, blk[0],
                              blk[nblk], diag_scale ? diag_scale->d : nullptr, weight, sweeps,
                              zero_first, reverse);
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_HIP(hipFree(d_blk));
   return s;
}

extern "C" int amg_gauss_seidel(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                                int sweeps)
{
   AMG_ARG(c && A && f && u, "amg_gauss_seidel: null argument");
   // SEQ_GaussSeidel == one hybrid block covering every row (no out-of-block terms)
   int blk[2] = {0, A->nrows};
   return amg_hybrid_jgs(c, A, f, u, u, blk, 1, nullptr, 1.0, sweeps, 0, 0);
}

extern "C" int amg_async_gauss_seidel(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                                      const int *blk, int nblk, int sweeps, int semi, int reverse)
{
   AMG_ARG(c && A && f && u && blk && nblk > 0 && sweeps >= 0, "amg_async_gauss_seidel: bad argument");
   AMG_ARG(f->n >= A->nrows && u->n >= A->nrows && A->nrows == A->ncols,
           "amg_async_gauss_seidel: square matrix and vectors of its size");
   for (int b = 0; b < nblk; b++)
      AMG_ARG(blk[b] <= blk[b + 1] && blk[b] >= 0 && blk[b + 1] <= A->nrows,
              "amg_async_gauss_seidel: bad block %d [%d,%d)", b, blk[b], blk[b + 1]);
   int *d_blk = nullptr;
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_HIP(hipMalloc((void **)&d_blk, (nblk + 1) * sizeof(int)));
   AMG_HIP(hipMemcpyAsync(d_blk, blk, (nblk + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
   amgk::async_gs(c->stream, A, f->d, u->d, d_blk, nblk, sweeps, semi, reverse);
   AMG_HIP(hipStreamSynchronize(c->stream));
   AMG_HIP(hipFree(d_blk));
   return AMG_OK;
}

int amg_sym_jacobi_dev(hipStream_t s, const amg_mat *A, const double *f, double *u, double *y,
                       double *r, double omega, const double *l1, int sweeps, int zero_first,
                       int rb, int re, int variant)
{
   const int seq = (variant == 1);
   amgk::Gemv mv = amgk::gemv_mode(1.0, 0.0);
   int k = 0;
   if (seq || zero_first == 1) {
      amgk::vcopy(s, f, r, rb, re);
   } else {
      amgk::spgemv(s, A, u, nullptr, mv, y, rb, re, nullptr);
      amgk::vsub(s, f, y, r, rb, re);
   }
   while (true) {
      amgk::sym_scale(s, A->diag, l1, omega, r, rb, re, seq);
      amgk::spgemv(s, A, r, nullptr, mv, y, rb, re, nullptr);
      amgk::sym_update(s, A->diag, l1, omega, r, y, u, rb, re, seq, (!seq && zero_first == 1));
      k++;
      if (k == sweeps) break;
      amgk::spgemv(s, A, u, nullptr, mv, y, rb, re, nullptr);
      amgk::vsub(s, f, y, r, rb, re);
   }
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_sym_jacobi(amg_ctx *c, const amg_mat *A, const amg_vec *f, amg_vec *u,
                              amg_vec *y, amg_vec *r, double omega, const amg_vec *l1, int sweeps,
                              int zero_first, int rb, int re, int variant)
{
   AMG_ARG(c && A && f && u && y && r && sweeps >= 1, "amg_sym_jacobi: bad argument");
   AMG_TRY(check_range(A, rb, re));
   return amg_sym_jacobi_dev(c->stream, A, f->d, u->d, y->d, r->d, omega, l1 ? l1->d : nullptr,
                             sweeps, zero_first, rb, re, variant);
}

extern "C" int amg_l1_norms(amg_ctx *c, const amg_mat *A, amg_vec *out)
{
   AMG_ARG(c && A && out && out->n >= A->nrows, "amg_l1_norms: bad argument");
   amgk::l1_norms(c->stream, A, out->d);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_a_diag(amg_ctx *c, const amg_mat *A, double omega, amg_vec *out)
{
   AMG_ARG(c && A && out && out->n >= A->nrows, "amg_a_diag: bad argument");
   amgk::a_diag(c->stream, A->diag, omega, out->d, A->nrows);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}
