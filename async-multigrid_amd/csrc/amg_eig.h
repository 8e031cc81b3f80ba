// amg_eig.h -- the CG-Lanczos eigenvalue estimate (hypre_ParCSRMaxEigEstimateCG's
// role, DMEM_Setup.cpp:77-87), once, for one GPU (amg_eigs_cg in amg_api.cpp) and
// for the distributed level-0 operator (amg_dist_eigs_cg in amg_dist.cpp).  Host
// only, not part of the C-ABI.  Conjugate gradients on A preconditioned by its
// diagonal d, with no right-hand side and no iterate, every statement a
// separately rounded fp64 operation:
//    gamma_0 = r . (r ./ d)
//    iteration i:  p = r ./ d (i = 0),  p = r ./ d + beta_{i-1} p (i > 0);  q = A p
//                  alpha_i = gamma_i / p.q;  r -= alpha_i q
//                  gamma_{i+1} = r . (r ./ d);  beta_i = gamma_{i+1} / gamma_i
// (alpha, beta = 0 where their divisor is 0, pcg_alpha_q / pcg_beta_q).  In exact
// arithmetic these are the alpha / beta / gamma of CG on D^-1/2 A D^-1/2, whose
// Lanczos tridiagonal amg_lanczos_extremes forms; scale 0 is d = 1 without the
// division.  The scalars stay on the device (rings of max_iter entries, gamma one
// more) and nothing is read back inside the loop: the iterations that count are
// chosen afterwards (valid_iterations).  The binding B supplies
//    c                            the context: its stream
//    gathers                      constexpr: a dot product is this rank's sum, gathered and
//                                 added in rank order (else finished in one launch)
//    n(), diag()                  the rows and their a_ii
//    alloc_vec(&p), alloc(m, &p)  an operand of A; m doubles (both zeroed)
//    apply_A(x, y)                y = A x on the rows (an int status)
//    nranks(), gather(slot, gath, k)  with gathers: every rank's k doubles, in rank order;
//    gather_bytes(send, recv, bytes)  the same for any bytes
#pragma once

#include <cfloat>
#include <cmath>

#include "amg_internal.h"
#include "amg_pcg.h"

struct AmgEig {
   double *r = nullptr, *p = nullptr, *q = nullptr; // p: an operand of A
   double *sc = nullptr;                            // the device scalar block (amgk::PCG_*, gamma in PCG_RHO)
   double *part_dot = nullptr, *part_g = nullptr;   // partials of p.q and of r . (r ./ d)
   double *ring = nullptr;                          // alpha | beta | gamma (PCG_RING + 1)
   double *slot = nullptr, *gath = nullptr;         // with a gather: this rank's sum; every rank's
   int *bad = nullptr;                              // rows with a_ii <= 0: this rank's, then every rank's
};

// the start vector of this rank's n rows from global row row0 into r (device): r0
// (host) or, where null, 2 u_g - 1 of amg_lehmer_stream(1, ...) by global row g
int amg_eig_start_vector(hipStream_t s, double *r, const double *r0, long long row0, int n);

namespace amg_eig {

// hypre's break and a usable step: the leading iterations i with gamma_i >=
// DBL_EPSILON whose alpha_i is finite and positive
inline int valid_iterations(int m, const double *alpha, const double *gamma)
{
   int k = 0;
   while (k < m && gamma[k] >= DBL_EPSILON && std::isfinite(alpha[k]) && alpha[k] > 0.0) k++;
   return k;
}

// the extremes of the leading valid iterations' tridiagonal; *iters = their number
inline int extremes(const char *who, int m, const double *alpha, const double *beta, const double *gamma,
                    double *eig_max, double *eig_min, int *iters)
{
   const int k = valid_iterations(m, alpha, gamma);
   if (iters) *iters = k;
   if (k == 0)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: no valid iteration (gamma_0 = %g, alpha_0 = %g): nothing to "
                           "estimate from", who, m > 0 ? gamma[0] : 0.0, m > 0 ? alpha[0] : 0.0);
   std::vector<double> td(k), to(k);
   return amg_lanczos_extremes(k, alpha, beta, td.data(), to.data(), eig_max, eig_min);
}

// gamma (and beta) from the partials of r . (r ./ d)
template <class B>
int finish_gamma(B &b, AmgEig &g, int np, double *ring_beta, double *ring_gamma, int first)
{
   hipStream_t s = b.c->stream;
   if constexpr (B::gathers) {
      amgk::pcg_rank_sum(s, g.part_g, nullptr, np, g.slot);
      AMG_TRY(b.gather(g.slot, g.gath, 1));
      amgk::eig_gamma_ranks(s, g.gath, b.nranks(), g.sc, ring_beta, ring_gamma, first);
   } else {
      amgk::eig_gamma(s, g.part_g, np, g.sc, ring_beta, ring_gamma, first);
   }
   return AMG_OK;
}

// load(r): the binding's start vector into g.r.  alpha / beta / gamma (host,
// null: not wanted): the whole history, max_iter / max_iter / max_iter + 1 entries
template <class B, class Load>
int run(B &b, AmgEig &g, const char *who, int scale, int max_iter, Load load, double *eig_max, double *eig_min,
        double *alpha, double *beta, double *gamma, int *iters)
{
   using amgk::PCG_RING;
   hipStream_t s = b.c->stream;
   const int n = b.n();
   for (double **v : {&g.r, &g.q})
      if (!*v) AMG_TRY(b.alloc((size_t)n, v));
   if (!g.p) AMG_TRY(b.alloc_vec(&g.p));
   if (!g.sc) AMG_TRY(b.alloc(amgk::PCG_NSCALARS, &g.sc));
   if (!g.part_dot) AMG_TRY(b.alloc(1024, &g.part_dot));
   if (!g.part_g) AMG_TRY(b.alloc(1024, &g.part_g));
   if (!g.ring) AMG_TRY(b.alloc(3 * (size_t)PCG_RING + 1, &g.ring));
   int nr = 1;
   if constexpr (B::gathers) {
      nr = b.nranks();
      if (!g.slot) AMG_TRY(b.alloc(1, &g.slot));
      if (!g.gath) AMG_TRY(b.alloc((size_t)nr, &g.gath));
   }
   if (!g.bad) {
      double *w = nullptr;
      AMG_TRY(b.alloc((size_t)nr + 1, &w)); // ints in it
      g.bad = reinterpret_cast<int *>(w);
   }
   const double *d = scale ? b.diag() : nullptr;
   if (scale) {
      // every rank learns every rank's count before anyone refuses: no peer is left waiting
      std::vector<int> bad(nr, 0);
      AMG_HIP(hipMemsetAsync(g.bad, 0, sizeof(int), s));
      amgk::eig_count_bad_diag(s, d, n, g.bad);
      if constexpr (B::gathers) {
         AMG_TRY(b.gather_bytes(g.bad, g.bad + 1, sizeof(int)));
         AMG_HIP(hipMemcpyAsync(bad.data(), g.bad + 1, nr * sizeof(int), hipMemcpyDeviceToHost, s));
      } else {
         AMG_HIP(hipMemcpyAsync(bad.data(), g.bad, sizeof(int), hipMemcpyDeviceToHost, s));
      }
      AMG_HIP(hipStreamSynchronize(s));
      long long total = 0;
      for (int v : bad) total += v;
      AMG_ARG(total == 0, "%s: scale = 1 needs a positive diagonal: %lld row(s) with a_ii <= 0", who, total);
   }
   AMG_TRY(load(g.r));
   double *ra = g.ring, *rb = g.ring + PCG_RING, *rg = g.ring + 2 * PCG_RING;
   int np = 0;
   amgk::eig_update_r(s, g.r, nullptr, d, n, g.sc, g.part_g, &np);
   AMG_TRY(finish_gamma(b, g, np, nullptr, rg, 1));
   for (int i = 0; i < max_iter; i++) {
      amgk::eig_update_p(s, g.r, d, g.p, n, g.sc, i == 0);
      AMG_TRY(b.apply_A(g.p, g.q));
      amgk::dot_partials(s, g.p, g.q, n, g.part_dot, &np);
      if constexpr (B::gathers) {
         amgk::pcg_rank_sum(s, g.part_dot, nullptr, np, g.slot);
         AMG_TRY(b.gather(g.slot, g.gath, 1));
         amgk::pcg_alpha_ranks(s, g.gath, nr, g.sc, ra + i);
      } else {
         amgk::pcg_alpha(s, g.part_dot, np, g.sc, ra + i);
      }
      amgk::eig_update_r(s, g.r, g.q, d, n, g.sc, g.part_g, &np);
      AMG_TRY(finish_gamma(b, g, np, rb + i, rg + i + 1, 0));
   }
   AMG_HIP(hipGetLastError());
   std::vector<double> h(3 * (size_t)max_iter + 1);
   double *ha = h.data(), *hb = ha + max_iter, *hg = hb + max_iter;
   AMG_HIP(hipMemcpyAsync(ha, ra, max_iter * sizeof(double), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(hb, rb, max_iter * sizeof(double), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(hg, rg, ((size_t)max_iter + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   if (alpha) std::copy(ha, ha + max_iter, alpha);
   if (beta) std::copy(hb, hb + max_iter, beta);
   if (gamma) std::copy(hg, hg + max_iter + 1, gamma);
   return extremes(who, max_iter, ha, hb, hg, eig_max, eig_min, iters);
}

// the extremes of M^-1 A from a running PCG's alpha / beta ring (amg_pcg.h): gamma_0
// is the start's rho (sc[PCG_RHO0]), gamma_i the ring's rho of iteration i - 1
inline int pcg_extremes(const char *who, hipStream_t s, const AmgPcg &g, double *eig_max, double *eig_min,
                        int *iters)
{
   using amgk::PCG_RING;
   if (g.iter > PCG_RING)
      return amg_set_error(AMG_ERR_UNSUPPORTED, "%s: %d iterations have overwritten the first of the ring's %d", who,
                           g.iter, PCG_RING);
   const int m = g.iter;
   std::vector<double> h(3 * (size_t)m + 1);
   double *ha = h.data(), *hb = ha + m, *hg = hb + m;
   AMG_HIP(hipMemcpyAsync(hg, g.sc + amgk::PCG_RHO0, sizeof(double), hipMemcpyDeviceToHost, s));
   if (m > 0) {
      AMG_HIP(hipMemcpyAsync(ha, g.ring, m * sizeof(double), hipMemcpyDeviceToHost, s));
      AMG_HIP(hipMemcpyAsync(hb, g.ring + PCG_RING, m * sizeof(double), hipMemcpyDeviceToHost, s));
      AMG_HIP(hipMemcpyAsync(hg + 1, g.ring + 2 * PCG_RING, m * sizeof(double), hipMemcpyDeviceToHost, s));
   }
   AMG_HIP(hipStreamSynchronize(s));
   return extremes(who, m, ha, hb, hg, eig_max, eig_min, iters);
}

} // namespace amg_eig
