// amg_pcg.h -- the AMG-preconditioned conjugate-gradient recurrence, once, for
// one GPU (amg_pcg_* in amg_solver.cpp) and for the distributed hierarchy
// (amg_dist_pcg_* in amg_dist.cpp).  Host only, not part of the C-ABI.
// HYPRE's two-norm PCG, every statement a separately rounded fp64 operation:
//    r = f - A x0;  z = M^-1 r;  p = z;  rho = r.z;  hist[0] = sqrt(r.r)
//    q = A p;  alpha = rho / p.q;  x += alpha p;  r -= alpha q;  hist[k] = sqrt(r.r)
//    z = M^-1 r;  rho' = r.z;  beta = rho' / rho;  rho = rho';  p = z + beta p
// (alpha, beta = 0 where their divisor is 0: a zero right-hand side stays zero).
// Neither hierarchy type is known here.  Each file supplies a binding B:
//    c                            the context: its stream and pinned scalar
//    gathers                      constexpr: a dot product is this rank's sum, gathered and
//                                 added in rank order (else finished in one launch)
//    n(), r(), z()                the rows; r, where every cycle reads its right-hand side
//                                 and none writes; z, where the cycle leaves it
//    hist(), hist_cap()           the device ring of residual norms
//    alloc_vec(&p), alloc(m, &p)  an operand of A; m doubles
//    apply_A(x, b, mode, y)       y = mode(A x, b) on the rows (an int status)
//    precond(zero0_done)          z = M^-1 r; zero0_done: z already holds the cycle's first
//                                 level-0 sweep on r, written by the residual update
//    fuse_zero(), zero_sweep()    does it ride there, and on which operands (amgk::PcgZero)
//    nranks(), gather(slot, gath, k)  with gathers: every rank's k doubles, in rank order
#pragma once

#include "amg_internal.h"

struct AmgPcg {
   double *x = nullptr, *p = nullptr, *q = nullptr; // x, p: operands of A
   double *sc = nullptr;                            // the device scalar block (amgk::PCG_*)
   double *part_rr = nullptr, *part_dot = nullptr;  // partials of r.r and of p.q / r.z
   double *ring = nullptr;                          // alpha | beta | rho of the last PCG_RING iterations
   // with a gather: this rank's one or two sums of a dot product; every rank's, in rank order
   double *slot = nullptr, *gath = nullptr;
   int iter = 0;
   bool on = false;
   double r0norm = 0.0;
};

namespace amg_cg {

// where the norm of iteration g.iter's residual lies in the history ring
template <class B>
int hist_slot(B &b, const AmgPcg &g) { return g.iter % (b.hist_cap() - 1); }

// rho (and beta) from r . z, ||r|| into the history from the r.r partials
template <class B>
int finish_dots(B &b, AmgPcg &g, int first)
{
   using amgk::PCG_RING;
   hipStream_t s = b.c->stream;
   int np = 0;
   amgk::dot_partials(s, b.r(), b.z(), b.n(), g.part_dot, &np); // the r.r partials' grid too
   const int slot = first ? 0 : (g.iter - 1) % PCG_RING;
   double *norm = b.hist() + hist_slot(b, g), *ring_beta = g.ring + PCG_RING + slot,
          *ring_rho = g.ring + 2 * PCG_RING + slot;
   if constexpr (B::gathers) {
      amgk::pcg_rank_sum(s, g.part_rr, g.part_dot, np, g.slot);
      AMG_TRY(b.gather(g.slot, g.gath, 2));
      amgk::pcg_beta_ranks(s, g.gath, b.nranks(), g.sc, norm, ring_beta, ring_rho, first);
   } else {
      amgk::pcg_beta(s, g.part_rr, g.part_dot, np, g.sc, norm, ring_beta, ring_rho, first);
   }
   return AMG_OK;
}

template <class B>
int resnorm(B &b, const AmgPcg &g, double *out)
{
   amg_ctx *c = b.c;
   AMG_HIP(hipMemcpyAsync(c->h_pinned, b.hist() + hist_slot(b, g), sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
   AMG_HIP(hipStreamSynchronize(c->stream));
   *out = c->h_pinned[0];
   return AMG_OK;
}

// load(&f): the binding's own first steps -- x0 into g.x and the device
// right-hand side into *f.  Everything is allocated by the first start
template <class B, class Load>
int start(B &b, AmgPcg &g, Load load, double *r0norm)
{
   for (double **v : {&g.x, &g.p, &g.q})
      if (!*v) AMG_TRY(b.alloc_vec(v));
   if (!g.sc) AMG_TRY(b.alloc(amgk::PCG_NSCALARS, &g.sc));
   if (!g.part_rr) AMG_TRY(b.alloc(1024, &g.part_rr));
   if (!g.part_dot) AMG_TRY(b.alloc(1024, &g.part_dot));
   if (!g.ring) AMG_TRY(b.alloc(3 * (size_t)amgk::PCG_RING, &g.ring));
   if constexpr (B::gathers) {
      if (!g.slot) AMG_TRY(b.alloc(2, &g.slot));
      if (!g.gath) AMG_TRY(b.alloc(2 * (size_t)b.nranks(), &g.gath));
   }
   hipStream_t s = b.c->stream;
   g.on = false;
   g.iter = 0;
   const double *f = nullptr;
   AMG_TRY(load(&f));
   AMG_TRY(b.apply_A(g.x, f, amgk::gemv_mode(-1.0, 1.0), b.r()));
   AMG_TRY(b.precond(false));
   int np = 0;
   amgk::sumsq_partials(s, b.r(), b.n(), g.part_rr, &np);
   AMG_TRY(finish_dots(b, g, 1));
   amgk::vcopy(s, b.z(), g.p, 0, b.n());
   AMG_HIP(hipGetLastError());
   AMG_TRY(resnorm(b, g, &g.r0norm));
   g.on = true;
   if (r0norm) *r0norm = g.r0norm;
   return AMG_OK;
}

// one iteration; zg.u: the cycle's first level-0 sweep rides on the residual update
template <class B>
int step(B &b, AmgPcg &g, const amgk::PcgZero &zg)
{
   using amgk::PCG_RING;
   hipStream_t s = b.c->stream;
   const int n = b.n();
   int np = 0, np_rr = 0;
   AMG_TRY(b.apply_A(g.p, nullptr, amgk::gemv_mode(1.0, 0.0), g.q));
   amgk::dot_partials(s, g.p, g.q, n, g.part_dot, &np);
   if constexpr (B::gathers) {
      amgk::pcg_rank_sum(s, g.part_dot, nullptr, np, g.slot);
      AMG_TRY(b.gather(g.slot, g.gath, 1));
      amgk::pcg_alpha_ranks(s, g.gath, b.nranks(), g.sc, g.ring + g.iter % PCG_RING);
   } else {
      amgk::pcg_alpha(s, g.part_dot, np, g.sc, g.ring + g.iter % PCG_RING);
   }
   amgk::pcg_update_xr(s, g.x, g.p, b.r(), g.q, n, g.sc, g.part_rr, &np_rr, zg);
   g.iter++;
   AMG_TRY(b.precond(zg.u != nullptr));
   AMG_TRY(finish_dots(b, g, 0));
   amgk::pcg_update_p(s, b.z(), g.p, n, g.sc);
   return AMG_OK;
}

// k iterations; a failure inside one ends the solve (g.on)
template <class B>
int iterate(B &b, AmgPcg &g, int k)
{
   // the cycle's first level-0 sweep rides on the residual update where it is
   // the zero-guess Jacobi sweep (one pass over r and one clear of u fewer)
   const bool fz = b.fuse_zero();
   amgk::PcgZero zg = b.zero_sweep();
   for (int i = 0; i < k; i++) {
      zg.u = fz ? b.z() : nullptr; // a cycle may swap its level's vectors: z anew every time
      const int st = step(b, g, zg);
      if (st != AMG_OK) {
         g.on = false;
         return st;
      }
   }
   AMG_HIP(hipGetLastError());
   return AMG_OK;
}

// alpha, beta, rho of iterations iter - m + 1 .. iter, m = min(iter, cap,
// PCG_RING), oldest first (null: not wanted)
inline int scalars(hipStream_t s, const AmgPcg &g, double *alpha, double *beta, double *rho, int cap,
                   int *count)
{
   using amgk::PCG_RING;
   const int m = std::min(std::min(g.iter, cap), PCG_RING);
   double *out[3] = {alpha, beta, rho};
   for (int a = 0; a < 3; a++) {
      if (!out[a]) continue;
      for (int j = 0; j < m;) { // the ring may wrap
         const int slot = (g.iter - m + j) % PCG_RING;
         const int run = std::min(m - j, PCG_RING - slot);
         AMG_HIP(hipMemcpyAsync(out[a] + j, g.ring + a * PCG_RING + slot, run * sizeof(double),
                                hipMemcpyDeviceToHost, s));
         j += run;
      }
   }
   AMG_HIP(hipStreamSynchronize(s));
   *count = m;
   return AMG_OK;
}

// from a started state: up to o.num_cycles iterations, stopping at o.tol under
// check_resnorm 1 (every rank reads the same bits, so all stop together);
// reshist[0 .. *done] when not null
template <class B>
int run(B &b, AmgPcg &g, const amg_opts &o, double *reshist, int *done)
{
   if (reshist) reshist[0] = g.r0norm;
   *done = 0;
   for (int k = 1; k <= o.num_cycles; k++) {
      AMG_TRY(iterate(b, g, 1));
      *done = k;
      if (o.check_resnorm == 1) {
         double rn;
         AMG_TRY(resnorm(b, g, &rn));
         if (reshist) reshist[k] = rn;
         if (rn / g.r0norm < o.tol) break;
      }
   }
   // without the per-iteration read the history comes from the device ring
   // in one copy (as long as it has not wrapped)
   if (reshist && o.check_resnorm != 1 && *done > 0 && *done < b.hist_cap() - 1) {
      AMG_HIP(hipMemcpyAsync(reshist + 1, b.hist() + 1, *done * sizeof(double), hipMemcpyDeviceToHost, b.c->stream));
      AMG_HIP(hipStreamSynchronize(b.c->stream));
   }
   return AMG_OK;
}

} // namespace amg_cg
