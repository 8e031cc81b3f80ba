// amg_mrhs.cpp -- several right-hand sides at once: the multivector entry points
// (amg_mvec_*), the row operators over k columns (amg_mrhs_spgemv, ...) and the
// hierarchy's cycle, stationary solve and preconditioned CG on k columns
// (amg_mrhs_precond_apply, amg_mrhs_solve, amg_mrhs_pcg_solve).  The kernels are
// amg_mrhs.hip's; per column they do the arithmetic of the single-vector kernels, and
// the sequences below are the plain ones of amg_solver.cpp -- SMEM_Sync_Parfor_Vcycle
// as vcycle() runs it without its fused, geometric and reuse branches (bit-identical
// shortcuts), SMEM_Solve's outer loop, amg_pcg.h's recurrence -- so column j of a
// result carries the bits of the single-vector solve of column j.  The level
// multivectors and the PCG state are the hierarchy's own, apart from its single-vector
// state (amg_hier_view: nothing of that is written here).
// Out of scope: additive and asynchronous solvers, BPX, the hybrid JGS and
// Gauss-Seidel smoothers, Chebyshev acceleration, delays, the distributed hierarchy.
#include <algorithm>
#include <vector>

#include "amg_internal.h"

// ---------------------------------------------------------------------------
// multivectors
// ---------------------------------------------------------------------------
extern "C" int amg_mvec_create(amg_ctx *c, int n, int k, amg_mvec **out)
{
   AMG_ARG(c && out && n >= 0, "amg_mvec_create: bad argument");
   AMG_ARG(amgk::mrhs_width_ok(k), "amg_mvec_create: width %d (2, 4 or 8)", k);
   const size_t len = std::max<size_t>((size_t)n * k, 1);
   double *d = nullptr;
   hipError_t e = hipMalloc(&d, len * sizeof(double));
   if (e != hipSuccess) return amg_set_error(AMG_ERR_OOM, "amg_mvec_create(%d, %d): %s", n, k, hipGetErrorString(e));
   e = hipMemsetAsync(d, 0, len * sizeof(double), c->stream);
   if (e != hipSuccess) {
      hipFree(d);
      return amg_set_error(AMG_ERR_HIP, "amg_mvec_create: memset: %s", hipGetErrorString(e));
   }
   amg_mvec *v = new amg_mvec();
   v->ctx = c;
   v->n = n;
   v->k = k;
   v->d = d;
   *out = v;
   return AMG_OK;
}

extern "C" int amg_mvec_free(amg_mvec *v)
{
   if (!v) return AMG_OK;
   hipFree(v->d);
   delete v;
   return AMG_OK;
}

extern "C" int amg_mvec_size(const amg_mvec *v, int *n, int *k)
{
   AMG_ARG(v, "amg_mvec_size: null argument");
   if (n) *n = v->n;
   if (k) *k = v->k;
   return AMG_OK;
}

extern "C" int amg_mvec_upload(amg_ctx *c, amg_mvec *v, const double *h)
{
   AMG_ARG(c && v && h, "amg_mvec_upload: null argument");
   AMG_HIP(hipMemcpyAsync(v->d, h, (size_t)v->n * v->k * sizeof(double), hipMemcpyHostToDevice, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

extern "C" int amg_mvec_download(amg_ctx *c, const amg_mvec *v, double *h)
{
   AMG_ARG(c && v && h, "amg_mvec_download: null argument");
   AMG_HIP(hipMemcpyAsync(h, v->d, (size_t)v->n * v->k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

extern "C" int amg_mvec_set_col(amg_ctx *c, amg_mvec *v, int j, const amg_vec *x)
{
   AMG_ARG(c && v && x, "amg_mvec_set_col: null argument");
   AMG_ARG(j >= 0 && j < v->k && x->n == v->n, "amg_mvec_set_col: column %d of %d, %d rows against %d", j, v->k,
           x->n, v->n);
   amgk::mrhs_set_col(c->stream, v->k, j, x->d, v->d, v->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mvec_get_col(amg_ctx *c, const amg_mvec *v, int j, amg_vec *x)
{
   AMG_ARG(c && v && x, "amg_mvec_get_col: null argument");
   AMG_ARG(j >= 0 && j < v->k && x->n == v->n, "amg_mvec_get_col: column %d of %d, %d rows against %d", j, v->k,
           x->n, v->n);
   amgk::mrhs_get_col(c->stream, v->k, j, v->d, x->d, v->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mvec_set(amg_ctx *c, amg_mvec *v, double a)
{
   AMG_ARG(c && v, "amg_mvec_set: null argument");
   amgk::mrhs_set(c->stream, v->d, a, (long long)v->n * v->k);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mvec_axpy(amg_ctx *c, const double *alpha, const amg_mvec *x, amg_mvec *y)
{
   AMG_ARG(c && alpha && x && y, "amg_mvec_axpy: null argument");
   AMG_ARG(x->n == y->n && x->k == y->k, "amg_mvec_axpy: %d x %d against %d x %d", x->n, x->k, y->n, y->k);
   amgk::MrhsScal a{};
   for (int j = 0; j < x->k; j++) a.a[j] = alpha[j];
   amgk::mrhs_axpy(c->stream, x->k, a, x->d, y->d, x->n);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

// out[j] = column j's dot product (y null: sum of squares; do_sqrt: its root), host sync
static int mvec_reduce(amg_ctx *c, const amg_mvec *x, const amg_mvec *y, int do_sqrt, double *out)
{
   double *p;
   AMG_TRY(amg_ctx_partials(c, 1024 * amgk::MRHS_MAXK, &p));
   int np = 0;
   amgk::mrhs_dot_partials(c->stream, x->k, x->d, y ? y->d : nullptr, x->n, p, &np);
   amgk::mrhs_reduce_partials(c->stream, x->k, p, np, c->d_scalars, do_sqrt);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipMemcpyAsync(c->h_pinned, c->d_scalars, x->k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   for (int j = 0; j < x->k; j++) out[j] = c->h_pinned[j];
   return AMG_OK;
}

extern "C" int amg_mvec_dot(amg_ctx *c, const amg_mvec *x, const amg_mvec *y, double *out)
{
   AMG_ARG(c && x && y && out, "amg_mvec_dot: null argument");
   AMG_ARG(x->n == y->n && x->k == y->k, "amg_mvec_dot: %d x %d against %d x %d", x->n, x->k, y->n, y->k);
   return mvec_reduce(c, x, y, 0, out);
}

extern "C" int amg_mvec_norm2(amg_ctx *c, const amg_mvec *x, double *out)
{
   AMG_ARG(c && x && out, "amg_mvec_norm2: null argument");
   return mvec_reduce(c, x, nullptr, 1, out);
}

// ---------------------------------------------------------------------------
// row operators over k columns
// ---------------------------------------------------------------------------
extern "C" int amg_mrhs_spgemv(amg_ctx *c, const amg_mat *A, const amg_mvec *x, const amg_mvec *b, double alpha,
                               double beta, amg_mvec *y, int rb, int re)
{
   AMG_ARG(c && A && x && y, "amg_mrhs_spgemv: null argument");
   AMG_ARG(x->n == A->ncols && y->n == A->nrows, "amg_mrhs_spgemv: x has %d rows, y %d, A is %d x %d", x->n, y->n,
           A->nrows, A->ncols);
   AMG_ARG(x->k == y->k && (!b || b->k == y->k), "amg_mrhs_spgemv: widths differ");
   AMG_ARG(x->d != y->d, "amg_mrhs_spgemv: x may not alias y");
   AMG_ARG(rb >= 0 && re <= A->nrows && rb <= re, "row range [%d,%d) outside [0,%d)", rb, re, A->nrows);
   const amgk::Gemv g = amgk::gemv_mode(alpha, beta);
   AMG_ARG(g.init == 0 || (b && b->n == A->nrows), "amg_mrhs_spgemv: b (A's rows) required when beta != 0");
   amgk::mrhs_spgemv(c->stream, y->k, A, x->d, b ? b->d : nullptr, g, y->d, rb, re);
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mrhs_matvec(amg_ctx *c, const amg_mat *A, const amg_mvec *x, amg_mvec *y)
{
   AMG_ARG(A, "amg_mrhs_matvec: null argument");
   return amg_mrhs_spgemv(c, A, x, nullptr, 1.0, 0.0, y, 0, A->nrows);
}

static int mrhs_smooth_args(const char *who, const amg_mat *A, const amg_mvec *f, const amg_mvec *u,
                            const amg_mvec *u_prev)
{
   AMG_ARG(A->nrows == A->ncols, "%s: A must be square", who);
   AMG_ARG(f->n == A->nrows && u->n == A->nrows && u_prev->n == A->nrows, "%s: %d / %d / %d rows against A's %d", who,
           f->n, u->n, u_prev->n, A->nrows);
   AMG_ARG(f->k == u->k && u_prev->k == u->k, "%s: widths differ", who);
   AMG_ARG(u->d != u_prev->d, "%s: u_prev may not alias u", who);
   return AMG_OK;
}

// amg_jacobi / amg_l1_jacobi, variant 0 on all rows: u_prev = u; u = J(u_prev)
static int mrhs_sweeps(amg_ctx *c, const amg_mat *A, const amg_mvec *f, amg_mvec *u, amg_mvec *u_prev,
                       const double *l1, double omega, int sweeps, int zero_first)
{
   const int K = u->k;
   for (int k = 0; k < sweeps; k++) {
      if (k == 0 && zero_first == 1) {
         amgk::mrhs_jacobi_zero(c->stream, K, A->diag, f->d, l1, omega, u->d, u->n);
      } else {
         AMG_HIP(hipMemcpyAsync(u_prev->d, u->d, (size_t)u->n * K * sizeof(double), hipMemcpyDeviceToDevice,
                                c->stream));
         amgk::mrhs_jacobi_sweep(c->stream, K, A, f->d, u_prev->d, l1, omega, u->d);
      }
   }
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mrhs_jacobi(amg_ctx *c, const amg_mat *A, const amg_mvec *f, amg_mvec *u, amg_mvec *u_prev,
                               double omega, int sweeps, int zero_first)
{
   AMG_ARG(c && A && f && u && u_prev, "amg_mrhs_jacobi: null argument");
   AMG_TRY(mrhs_smooth_args("amg_mrhs_jacobi", A, f, u, u_prev));
   return mrhs_sweeps(c, A, f, u, u_prev, nullptr, omega, sweeps, zero_first);
}

extern "C" int amg_mrhs_l1_jacobi(amg_ctx *c, const amg_mat *A, const amg_mvec *f, amg_mvec *u, amg_mvec *u_prev,
                                  const amg_vec *l1, int sweeps, int zero_first)
{
   AMG_ARG(c && A && f && u && u_prev && l1, "amg_mrhs_l1_jacobi: null argument");
   AMG_TRY(mrhs_smooth_args("amg_mrhs_l1_jacobi", A, f, u, u_prev));
   AMG_ARG(l1->n == A->nrows, "amg_mrhs_l1_jacobi: l1 has %d rows, A %d", l1->n, A->nrows);
   return mrhs_sweeps(c, A, f, u, u_prev, l1->d, 1.0, sweeps, zero_first);
}

// ---------------------------------------------------------------------------
// the hierarchy on k columns
// ---------------------------------------------------------------------------
namespace {
struct MLevel {
   double *f = nullptr, *u = nullptr, *u_alt = nullptr, *r = nullptr;
};
} // namespace

struct amg_mrhs_state {
   int K = 0;
   std::vector<MLevel> lv;
   double *r0 = nullptr; // the outer residual; PCG's r (z is lv[0].u, where the cycle leaves it)
   double *hist = nullptr; // device history of residual norms, K per iteration
   size_t hist_cap = 0;
   // PCG (allocated by the first amg_mrhs_pcg_solve of this width)
   double *x = nullptr, *p = nullptr, *q = nullptr;
   double *sc = nullptr, *part_rr = nullptr, *part_dot = nullptr;
   double *ring = nullptr; // scalar a (alpha, beta, rho) of column j: ring[(MRHS_MAXK a + j) PCG_RING + slot]
   int iter = 0;
   bool pcg_on = false;
   std::vector<void *> allocs;
};

void amg_mrhs_state_free(amg_mrhs_state *st)
{
   if (!st) return;
   for (void *p : st->allocs) hipFree(p);
   hipFree(st->hist);
   delete st;
}

namespace {

int malloc0(amg_ctx *c, amg_mrhs_state *st, size_t n, double **p)
{
   n = std::max<size_t>(n, 1);
   hipError_t e = hipMalloc(p, n * sizeof(double));
   if (e != hipSuccess)
      return amg_set_error(AMG_ERR_OOM, "amg_mrhs: allocation of %zu doubles: %s", n, hipGetErrorString(e));
   st->allocs.push_back(*p);
   AMG_HIP(hipMemsetAsync(*p, 0, n * sizeof(double), c->stream));
   return AMG_OK;
}

// the combinations the multi-vector cycle restates; refused before anything is launched
int check_supported(const amg_hier_view &hv, const char *who)
{
   const amg_opts &o = *hv.o;
   if (o.solver != AMG_MULT)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: solver %d (AMG_MULT hierarchies only)", who, o.solver);
   if (o.smoother != AMG_JACOBI && o.smoother != AMG_L1_JACOBI)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: smoother %d (AMG_JACOBI and AMG_L1_JACOBI only)", who,
                           o.smoother);
   if (o.cheby_flag != 0)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: Chebyshev acceleration is not supported", who);
   if (o.delay_type != AMG_DELAY_NONE)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: delay injection is not supported", who);
   return AMG_OK;
}

// operands of a hierarchy call: n0 rows, one width of 2, 4 or 8
int check_operands(const amg_hier_view &hv, const char *who, const amg_mvec *a, const amg_mvec *b)
{
   AMG_ARG(a->n == hv.lv[0].n && b->n == hv.lv[0].n, "%s: %d / %d rows against the hierarchy's %d", who, a->n, b->n,
           hv.lv[0].n);
   AMG_ARG(a->k == b->k && amgk::mrhs_width_ok(a->k), "%s: widths %d / %d (equal, and 2, 4 or 8)", who, a->k, b->k);
   return AMG_OK;
}

// the state of width K: allocated by the first call, anew when the width changes
int ensure_state(const amg_hier_view &hv, int K, amg_mrhs_state **out)
{
   amg_mrhs_state *st = *hv.mrhs;
   if (st && st->K == K) {
      *out = st;
      return AMG_OK;
   }
   if (st) {
      AMG_HIP(hipStreamSynchronize(hv.ctx->stream));
      amg_mrhs_state_free(st);
      *hv.mrhs = nullptr;
   }
   st = new amg_mrhs_state();
   *hv.mrhs = st; // owned by the hierarchy from here on, whatever fails below
   st->K = K;
   st->lv.resize(hv.L);
   for (int l = 0; l < hv.L; l++) {
      const size_t len = (size_t)hv.lv[l].n * K;
      for (double **v : {&st->lv[l].f, &st->lv[l].u, &st->lv[l].u_alt, &st->lv[l].r})
         AMG_TRY(malloc0(hv.ctx, st, len, v));
   }
   AMG_TRY(malloc0(hv.ctx, st, (size_t)hv.lv[0].n * K, &st->r0));
   *out = st;
   return AMG_OK;
}

int ensure_hist(amg_ctx *c, amg_mrhs_state *st, size_t need)
{
   if (need <= st->hist_cap) return AMG_OK;
   AMG_HIP(hipStreamSynchronize(c->stream));
   hipFree(st->hist);
   st->hist = nullptr;
   st->hist_cap = 0;
   hipError_t e = hipMalloc(&st->hist, need * sizeof(double));
   if (e != hipSuccess)
      return amg_set_error(AMG_ERR_OOM, "amg_mrhs: history of %zu doubles: %s", need, hipGetErrorString(e));
   st->hist_cap = need;
   return AMG_OK;
}

int dcopy(hipStream_t s, const double *src, double *dst, size_t len)
{
   if (len) AMG_HIP(hipMemcpyAsync(dst, src, len * sizeof(double), hipMemcpyDeviceToDevice, s));
   return AMG_OK;
}

// smooth_one_level's Jacobi / L1 Jacobi branch: the zero-guess sweep first where zf, every
// other sweep u_alt = J(u) and a swap
void smooth(const amg_hier_view &hv, amg_mrhs_state *st, int l, const double *f, int sweeps, bool zf)
{
   hipStream_t s = hv.ctx->stream;
   const amg_opts &o = *hv.o;
   const amg_hier_level_view &v = hv.lv[l];
   MLevel &m = st->lv[l];
   const double *l1 = o.smoother == AMG_L1_JACOBI ? v.l1 : nullptr;
   for (int k = 0; k < sweeps; k++) {
      if (k == 0 && zf) {
         amgk::mrhs_jacobi_zero(s, st->K, v.A->diag, f, l1, o.smooth_weight, m.u, v.n);
      } else {
         amgk::mrhs_jacobi_sweep(s, st->K, v.A, f, m.u, l1, o.smooth_weight, m.u_alt);
         std::swap(m.u, m.u_alt);
      }
   }
}

// SMEM_Sync_Parfor_Vcycle (SMEM_Sync_AMG.cpp:8-145) as vcycle() runs it.  precond: level
// 0 reads its right-hand side from r0 and starts from the zero-guess sweep.  As there,
// the coarsest level runs its pre + post sweeps as ordinary sweeps on its own iterate.
void cycle(const amg_hier_view &hv, amg_mrhs_state *st, bool precond)
{
   hipStream_t s = hv.ctx->stream;
   const amg_opts &o = *hv.o;
   const int L = hv.L, K = st->K;
   const amgk::Gemv res_mode = amgk::gemv_mode(-1.0, 1.0);
   const amgk::Gemv mv_mode = amgk::gemv_mode(1.0, 0.0);
   const amgk::Gemv pro_mode = amgk::gemv_mode(1.0, 1.0);
   for (int l = 0; l < L - 1; l++) {
      MLevel &m = st->lv[l];
      const double *f_fine = (l == 0 && precond) ? st->r0 : m.f;
      smooth(hv, st, l, f_fine, o.num_pre_smooth_sweeps, !(l == 0 && !precond));
      amgk::mrhs_spgemv(s, K, hv.lv[l].A, m.u, f_fine, res_mode, m.r, 0, hv.lv[l].n);
      amgk::mrhs_spgemv(s, K, hv.lv[l].R, m.r, nullptr, mv_mode, st->lv[l + 1].f, 0, hv.lv[l + 1].n);
   }
   // a one-level cycle in preconditioner mode smooths r0, as amg_precond_apply does
   smooth(hv, st, L - 1, (L == 1 && precond) ? st->r0 : st->lv[L - 1].f,
          o.num_pre_smooth_sweeps + o.num_post_smooth_sweeps, false);
   for (int l = L - 2; l >= 0; l--) {
      MLevel &m = st->lv[l];
      const double *f_fine = (l == 0 && precond) ? st->r0 : m.f;
      amgk::mrhs_spgemv(s, K, hv.lv[l].P, st->lv[l + 1].u, m.u, pro_mode, m.u, 0, hv.lv[l].n);
      smooth(hv, st, l, f_fine, o.num_post_smooth_sweeps, false);
   }
}

// lv[0].u = M^-1 r0: every level's iterate cleared, then one cycle in preconditioner mode
void precond(const amg_hier_view &hv, amg_mrhs_state *st)
{
   for (int l = 0; l < hv.L; l++) amgk::mrhs_set(hv.ctx->stream, st->lv[l].u, 0.0, (long long)hv.lv[l].n * st->K);
   cycle(hv, st, true);
}

// amg_solve's stop rule on every column, plus the zero column
bool all_done(const double *h0, const double *hk, int K, double tol)
{
   for (int j = 0; j < K; j++)
      if (!(h0[j] == 0.0 || hk[j] / h0[j] < tol)) return false;
   return true;
}

// the K norms of iteration `it` from the device history (host sync)
int read_norms(amg_ctx *c, const amg_mrhs_state *st, int it, double *out)
{
   AMG_HIP(hipMemcpyAsync(c->h_pinned, st->hist + (size_t)it * st->K, st->K * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   for (int j = 0; j < st->K; j++) out[j] = c->h_pinned[j];
   return AMG_OK;
}

// column j's 2-norm of v into hist[it][j], summed in amg_vec_norm2's order
int norms_to_hist(amg_ctx *c, amg_mrhs_state *st, const double *v, int n, int it)
{
   double *p;
   AMG_TRY(amg_ctx_partials(c, 1024 * amgk::MRHS_MAXK, &p));
   int np = 0;
   amgk::mrhs_dot_partials(c->stream, st->K, v, nullptr, n, p, &np);
   amgk::mrhs_reduce_partials(c->stream, st->K, p, np, st->hist + (size_t)it * st->K, 1);
   return AMG_OK;
}

// the history of iterations 0 .. done into reshist; under check_resnorm 1 it is there already
int fetch_hist(amg_ctx *c, const amg_mrhs_state *st, int done, double *reshist)
{
   if (!reshist) return AMG_OK;
   AMG_HIP(hipMemcpyAsync(reshist, st->hist, (size_t)(done + 1) * st->K * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   return AMG_OK;
}

} // namespace

extern "C" int amg_mrhs_precond_apply(amg_hier *H, const amg_mvec *r, amg_mvec *z)
{
   AMG_ARG(H && r && z, "amg_mrhs_precond_apply: null argument");
   amg_hier_view hv;
   amg_hier_get_view(H, &hv);
   AMG_TRY(check_operands(hv, "amg_mrhs_precond_apply", r, z));
   AMG_TRY(check_supported(hv, "amg_mrhs_precond_apply"));
   amg_mrhs_state *st;
   AMG_TRY(ensure_state(hv, r->k, &st));
   hipStream_t s = hv.ctx->stream;
   const size_t len = (size_t)r->n * r->k;
   st->pcg_on = false; // r0 and lv[0].u are PCG's r and z
   AMG_TRY(dcopy(s, r->d, st->r0, len));
   precond(hv, st);
   AMG_TRY(dcopy(s, st->lv[0].u, z->d, len));
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

extern "C" int amg_mrhs_solve(amg_hier *H, const amg_mvec *f, amg_mvec *u, double *reshist, int *cycles_done)
{
   AMG_ARG(H && f && u, "amg_mrhs_solve: null argument");
   amg_hier_view hv;
   amg_hier_get_view(H, &hv);
   AMG_TRY(check_operands(hv, "amg_mrhs_solve", f, u));
   AMG_TRY(check_supported(hv, "amg_mrhs_solve"));
   const amg_opts &o = *hv.o;
   AMG_ARG(o.num_cycles >= 0, "amg_mrhs_solve: num_cycles %d", o.num_cycles);
   amg_mrhs_state *st;
   AMG_TRY(ensure_state(hv, f->k, &st));
   amg_ctx *c = hv.ctx;
   hipStream_t s = c->stream;
   const int K = st->K, n0 = hv.lv[0].n;
   const size_t len0 = (size_t)n0 * K;
   AMG_TRY(ensure_hist(c, st, ((size_t)o.num_cycles + 1) * K));
   st->pcg_on = false;
   // InitVectors (Misc.cpp:565-692): every level vector zero, then f and the first iterate
   for (int l = 0; l < hv.L; l++) {
      const long long len = (long long)hv.lv[l].n * K;
      for (double *v : {st->lv[l].f, st->lv[l].u, st->lv[l].u_alt, st->lv[l].r}) amgk::mrhs_set(s, v, 0.0, len);
   }
   AMG_TRY(dcopy(s, f->d, st->lv[0].f, len0));
   AMG_TRY(dcopy(s, u->d, st->lv[0].u, len0));
   const amgk::Gemv res_mode = amgk::gemv_mode(-1.0, 1.0);
   auto outer_residual = [&](int it) {
      amgk::mrhs_spgemv(s, K, hv.lv[0].A, st->lv[0].u, st->lv[0].f, res_mode, st->r0, 0, n0);
      return norms_to_hist(c, st, st->r0, n0, it);
   };
   AMG_TRY(outer_residual(0));
   double h0[amgk::MRHS_MAXK], hk[amgk::MRHS_MAXK];
   if (o.check_resnorm == 1) AMG_TRY(read_norms(c, st, 0, h0));
   int done = 0;
   for (int k = 1; k <= o.num_cycles; k++) {
      cycle(hv, st, false);
      AMG_TRY(outer_residual(k));
      done = k;
      if (o.check_resnorm == 1) {
         AMG_TRY(read_norms(c, st, k, hk));
         if (all_done(h0, hk, K, o.tol)) break;
      }
   }
   AMG_TRY(dcopy(s, st->lv[0].u, u->d, len0));
   AMG_HIP(hipGetLastError());
   AMG_TRY(fetch_hist(c, st, done, reshist));
   AMG_HIP(hipStreamSynchronize(s));
   if (cycles_done) *cycles_done = done;
   return AMG_OK;
}

namespace {

// rho (and beta) from r . z, ||r|| into the history from the r . r partials (amg_cg::finish_dots)
void pcg_finish_dots(const amg_hier_view &hv, amg_mrhs_state *st, int first)
{
   using amgk::MRHS_MAXK;
   using amgk::PCG_RING;
   hipStream_t s = hv.ctx->stream;
   int np = 0;
   amgk::mrhs_dot_partials(s, st->K, st->r0, st->lv[0].u, hv.lv[0].n, st->part_dot, &np);
   const int slot = first ? 0 : (st->iter - 1) % PCG_RING;
   amgk::mrhs_pcg_beta(s, st->K, st->part_rr, st->part_dot, np, st->sc, st->hist + (size_t)st->iter * st->K,
                       st->ring + (size_t)MRHS_MAXK * PCG_RING + slot,
                       st->ring + 2 * (size_t)MRHS_MAXK * PCG_RING + slot, first);
}

// amg_cg::start: r = f - A x0; z = M^-1 r; p = z; rho = r . z; hist[0] = ||r||
int pcg_start(const amg_hier_view &hv, amg_mrhs_state *st, const amg_mvec *f, const amg_mvec *x0)
{
   using amgk::MRHS_MAXK;
   amg_ctx *c = hv.ctx;
   hipStream_t s = c->stream;
   const int K = st->K, n0 = hv.lv[0].n;
   const size_t len0 = (size_t)n0 * K;
   for (double **v : {&st->x, &st->p, &st->q})
      if (!*v) AMG_TRY(malloc0(c, st, len0, v));
   if (!st->sc) AMG_TRY(malloc0(c, st, (size_t)amgk::PCG_NSCALARS * MRHS_MAXK, &st->sc));
   if (!st->part_rr) AMG_TRY(malloc0(c, st, 1024 * (size_t)MRHS_MAXK, &st->part_rr));
   if (!st->part_dot) AMG_TRY(malloc0(c, st, 1024 * (size_t)MRHS_MAXK, &st->part_dot));
   if (!st->ring) AMG_TRY(malloc0(c, st, 3 * (size_t)MRHS_MAXK * amgk::PCG_RING, &st->ring));
   st->pcg_on = false;
   st->iter = 0;
   AMG_TRY(dcopy(s, x0->d, st->x, len0));
   amgk::mrhs_spgemv(s, K, hv.lv[0].A, st->x, f->d, amgk::gemv_mode(-1.0, 1.0), st->r0, 0, n0);
   precond(hv, st);
   int np = 0;
   amgk::mrhs_dot_partials(s, K, st->r0, nullptr, n0, st->part_rr, &np);
   pcg_finish_dots(hv, st, 1);
   AMG_TRY(dcopy(s, st->lv[0].u, st->p, len0));
   AMG_HIP(hipGetLastError());
   st->pcg_on = true;
   return AMG_OK;
}

// amg_cg::step: q = A p; alpha = rho / p.q; x += alpha p; r -= alpha q; hist = ||r||;
// z = M^-1 r; rho' = r.z; beta = rho' / rho; rho = rho'; p = z + beta p
void pcg_step(const amg_hier_view &hv, amg_mrhs_state *st)
{
   using amgk::PCG_RING;
   hipStream_t s = hv.ctx->stream;
   const int K = st->K, n0 = hv.lv[0].n;
   int np = 0;
   amgk::mrhs_spgemv(s, K, hv.lv[0].A, st->p, nullptr, amgk::gemv_mode(1.0, 0.0), st->q, 0, n0);
   amgk::mrhs_dot_partials(s, K, st->p, st->q, n0, st->part_dot, &np);
   amgk::mrhs_pcg_alpha(s, K, st->part_dot, np, st->sc, st->ring + st->iter % PCG_RING);
   amgk::mrhs_pcg_update_xr(s, K, st->x, st->p, st->r0, st->q, n0, st->sc, st->part_rr, &np);
   st->iter++;
   precond(hv, st);
   pcg_finish_dots(hv, st, 0);
   amgk::mrhs_pcg_update_p(s, K, st->lv[0].u, st->p, n0, st->sc);
}

} // namespace

extern "C" int amg_mrhs_pcg_solve(amg_hier *H, const amg_mvec *f, amg_mvec *x, double *reshist, int *iters_done)
{
   AMG_ARG(H && f && x, "amg_mrhs_pcg_solve: null argument");
   amg_hier_view hv;
   amg_hier_get_view(H, &hv);
   AMG_TRY(check_operands(hv, "amg_mrhs_pcg_solve", f, x));
   AMG_TRY(check_supported(hv, "amg_mrhs_pcg_solve"));
   const amg_opts &o = *hv.o;
   AMG_ARG(o.num_cycles >= 0, "amg_mrhs_pcg_solve: num_cycles %d", o.num_cycles);
   amg_mrhs_state *st;
   AMG_TRY(ensure_state(hv, f->k, &st));
   amg_ctx *c = hv.ctx;
   const int K = st->K;
   AMG_TRY(ensure_hist(c, st, ((size_t)o.num_cycles + 1) * K));
   AMG_TRY(pcg_start(hv, st, f, x));
   double h0[amgk::MRHS_MAXK], hk[amgk::MRHS_MAXK];
   if (o.check_resnorm == 1) AMG_TRY(read_norms(c, st, 0, h0));
   int done = 0;
   for (int k = 1; k <= o.num_cycles; k++) {
      pcg_step(hv, st);
      done = k;
      if (o.check_resnorm == 1) {
         AMG_TRY(read_norms(c, st, k, hk));
         if (all_done(h0, hk, K, o.tol)) break;
      }
   }
   AMG_TRY(dcopy(c->stream, st->x, x->d, (size_t)x->n * K));
   AMG_HIP(hipGetLastError());
   AMG_TRY(fetch_hist(c, st, done, reshist));
   AMG_HIP(hipStreamSynchronize(c->stream));
   if (iters_done) *iters_done = done;
   return AMG_OK;
}

extern "C" int amg_mrhs_pcg_scalars(const amg_hier *H, int col, double *alpha, double *beta, double *rho, int cap,
                                    int *count)
{
   using amgk::MRHS_MAXK;
   using amgk::PCG_RING;
   AMG_ARG(H && count && cap >= 0, "amg_mrhs_pcg_scalars: bad argument");
   amg_hier_view hv;
   amg_hier_get_view(const_cast<amg_hier *>(H), &hv);
   const amg_mrhs_state *st = *hv.mrhs;
   AMG_ARG(st && st->pcg_on, "amg_mrhs_pcg_scalars: no multi-vector PCG state");
   AMG_ARG(col >= 0 && col < st->K, "amg_mrhs_pcg_scalars: column %d of %d", col, st->K);
   hipStream_t s = hv.ctx->stream;
   const int m = std::min(std::min(st->iter, cap), PCG_RING);
   double *out[3] = {alpha, beta, rho};
   for (int a = 0; a < 3; a++) {
      if (!out[a]) continue;
      const double *ring = st->ring + ((size_t)MRHS_MAXK * a + col) * PCG_RING;
      for (int j = 0; j < m;) { // the ring may wrap
         const int slot = (st->iter - m + j) % PCG_RING;
         const int run = std::min(m - j, PCG_RING - slot);
         AMG_HIP(hipMemcpyAsync(out[a] + j, ring + slot, run * sizeof(double), hipMemcpyDeviceToHost, s));
         j += run;
      }
   }
   AMG_HIP(hipStreamSynchronize(s));
   *count = m;
   return AMG_OK;
}
