// amg_eig.hip -- the vector kernels of the CG-Lanczos eigenvalue estimate
// (amg_eig.h, which amg_eigs_cg in amg_api.cpp and amg_dist_eigs_cg in
// amg_dist.cpp both run): conjugate gradients on A preconditioned by its
// diagonal d, with no right-hand side and no iterate,
//    p = r ./ d (+ beta p);  q = A p;  alpha = gamma / p.q;  r -= alpha q;
//    gamma' = r . (r ./ d);  beta = gamma' / gamma
// Beside the product that is three passes: eig_p_k (32n bytes, 24n unscaled),
// dot_partials (16n) and eig_r_k (32n, 24n), which forms gamma' from the r it
// still holds in registers.  Every statement is one rounded fp64 operation
// (-ffp-contract=off), r_i / d_i an IEEE division, no square root anywhere; the
// sums run in amg_vec_dot's order (red_blocks(n) workgroups of 256 lanes, a lane
// adding in index order, block_sum_256) and the quotients are pcg_alpha_q /
// pcg_beta_q, so the whole alpha / beta / gamma history can be restated on the
// host to the bit.
#include <algorithm>

#include "amg_internal.h"

namespace amgk {

__global__ __launch_bounds__(256) void eig_bad_diag_k(const double *__restrict__ d, int n, int *__restrict__ count)
{
   const long long st = (long long)gridDim.x * 256;
   int bad = 0;
   for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) bad += !(d[i] > 0.0);
   if (bad) atomicAdd(count, bad);
}

// p = r ./ d (FIRST) or r ./ d + beta p; SCALE false: d = 1.  Four grid strides
// are loaded ahead
template <bool SCALE, bool FIRST>
__global__ __launch_bounds__(256) void eig_p_k(const double *__restrict__ r, const double *__restrict__ d,
                                               double *__restrict__ p, int n, const double *__restrict__ sc)
{
   const double beta = FIRST ? 0.0 : sc[PCG_BETA];
   const long long st = (long long)gridDim.x * 256;
   long long i = (long long)blockIdx.x * 256 + threadIdx.x;
   for (; i + 3 * st < n; i += 4 * st) {
      double rv[4], dv[4], pv[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
         rv[k] = r[i + k * st];
         if (SCALE) dv[k] = d[i + k * st];
         if (!FIRST) pv[k] = p[i + k * st];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
         const double z = SCALE ? rv[k] / dv[k] : rv[k];
         p[i + k * st] = FIRST ? z : z + beta * pv[k];
      }
   }
   for (; i < n; i += st) {
      const double z = SCALE ? r[i] / d[i] : r[i];
      p[i] = FIRST ? z : z + beta * p[i];
   }
}

// r -= alpha q (UPDATE) and the partials of r . (r ./ d) on the reduction grid
// from the r in registers.  Four grid strides are loaded ahead; a lane still adds
// its products in index order
template <bool SCALE, bool UPDATE>
__global__ __launch_bounds__(256) void eig_r_k(double *__restrict__ r, const double *__restrict__ q,
                                               const double *__restrict__ d, int n,
                                               const double *__restrict__ sc, double *__restrict__ partials)
{
   __shared__ double red[4];
   const double alpha = UPDATE ? sc[PCG_ALPHA] : 0.0;
   const long long st = (long long)gridDim.x * 256;
   long long i = (long long)blockIdx.x * 256 + threadIdx.x;
   double s = 0.0;
   for (; i + 3 * st < n; i += 4 * st) {
      double rv[4], qv[4], dv[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
         rv[k] = r[i + k * st];
         if (UPDATE) qv[k] = q[i + k * st];
         if (SCALE) dv[k] = d[i + k * st];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
         double ri = rv[k];
         if (UPDATE) {
            ri = rv[k] - alpha * qv[k];
            r[i + k * st] = ri;
         }
         s += ri * (SCALE ? ri / dv[k] : ri);
      }
   }
   for (; i < n; i += st) {
      double ri = r[i];
      if (UPDATE) {
         ri = ri - alpha * q[i];
         r[i] = ri;
      }
      s += ri * (SCALE ? ri / d[i] : ri);
   }
   s = block_sum_256(s, red);
   if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// pcg_beta_q on gamma' (no norm); the ring keeps gamma_0 too
__device__ __forceinline__ void eig_gamma_q(double gam, double *__restrict__ sc, double *__restrict__ ring_beta,
                                            double *__restrict__ ring_gamma, int first)
{
   pcg_beta_q(gam, gam, sc, nullptr, ring_beta, ring_gamma, first);
   if (first) *ring_gamma = gam;
}

__global__ __launch_bounds__(256) void eig_gamma_k(const double *__restrict__ part, int np, double *__restrict__ sc,
                                                   double *__restrict__ ring_beta, double *__restrict__ ring_gamma,
                                                   int first)
{
   __shared__ double red[4];
   const double gam = pcg_sum_partials(part, np, red);
   if (threadIdx.x == 0) eig_gamma_q(gam, sc, ring_beta, ring_gamma, first);
}

// on the gathered rank values v[r], added in rank order (amg_pcg.hip)
__global__ __launch_bounds__(256) void eig_gamma_ranks_k(const double *__restrict__ v, int nranks,
                                                         double *__restrict__ sc, double *__restrict__ ring_beta,
                                                         double *__restrict__ ring_gamma, int first)
{
   if (threadIdx.x == 0) {
      double gam = 0.0;
      for (int r = 0; r < nranks; r++) gam += v[r];
      eig_gamma_q(gam, sc, ring_beta, ring_gamma, first);
   }
}

void eig_count_bad_diag(hipStream_t s, const double *d, int n, int *count)
{
   if (n > 0) eig_bad_diag_k<<<std::min((n + 255) / 256, 1024), 256, 0, s>>>(d, n, count);
}

void eig_update_p(hipStream_t s, const double *r, const double *d, double *p, int n, const double *sc, int first)
{
   if (n <= 0) return;
   const int nb = std::min((n + 1023) / 1024, 2048);
   if (d) {
      if (first)
         eig_p_k<true, true><<<nb, 256, 0, s>>>(r, d, p, n, sc);
      else
         eig_p_k<true, false><<<nb, 256, 0, s>>>(r, d, p, n, sc);
   } else {
      if (first)
         eig_p_k<false, true><<<nb, 256, 0, s>>>(r, d, p, n, sc);
      else
         eig_p_k<false, false><<<nb, 256, 0, s>>>(r, d, p, n, sc);
   }
}

void eig_update_r(hipStream_t s, double *r, const double *q, const double *d, int n, const double *sc,
                  double *partials, int *nparts)
{
   const int nb = red_blocks(n);
   if (d) {
      if (q)
         eig_r_k<true, true><<<nb, 256, 0, s>>>(r, q, d, n, sc, partials);
      else
         eig_r_k<true, false><<<nb, 256, 0, s>>>(r, q, d, n, sc, partials);
   } else {
      if (q)
         eig_r_k<false, true><<<nb, 256, 0, s>>>(r, q, d, n, sc, partials);
      else
         eig_r_k<false, false><<<nb, 256, 0, s>>>(r, q, d, n, sc, partials);
   }
   *nparts = nb;
}

void eig_gamma(hipStream_t s, const double *part, int np, double *sc, double *ring_beta, double *ring_gamma,
               int first)
{
   eig_gamma_k<<<1, 256, 0, s>>>(part, np, sc, ring_beta, ring_gamma, first);
}

void eig_gamma_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *ring_beta,
                     double *ring_gamma, int first)
{
   eig_gamma_ranks_k<<<1, 256, 0, s>>>(v, nranks, sc, ring_beta, ring_gamma, first);
}

} // namespace amgk
