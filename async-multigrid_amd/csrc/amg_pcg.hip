// amg_pcg.hip -- the kernels of the preconditioned conjugate-gradient
// recurrence (amg_pcg.h, which amg_pcg_* in amg_solver.cpp and amg_dist_pcg_*
// in amg_dist.cpp both run).  alpha, beta and rho never leave the device: a
// single-workgroup kernel finishes each dot product and forms the quotient in
// the same launch (pcg_alpha_q / pcg_beta_q, whether the sum came from this
// GPU's partials or from the ranks' gathered values), and the vector kernels
// read the scalars from device memory.  Every product and sum is rounded on its
// own (-ffp-contract=off), the quotients are IEEE divisions, and the three dot
// products are summed in amg_vec_dot's order: red_blocks(n) workgroups of 256
// lanes and block_sum_256's tree (amg_internal.h, the same functions
// partials_k / sum_partials_k call), then the workgroup partials through the
// same lane-strided sum in one workgroup.
#include <algorithm>

#include "amg_internal.h"

namespace amgk {

// pcg_alpha_q on pq = sum(part)
__global__ __launch_bounds__(256) void pcg_alpha_k(const double *__restrict__ part, int np,
                                                   double *__restrict__ sc, double *__restrict__ ring_alpha)
{
   __shared__ double red[4];
   const double pq = pcg_sum_partials(part, np, red);
   if (threadIdx.x == 0) pcg_alpha_q(pq, sc, ring_alpha);
}

// pcg_beta_q on rr = sum(part_rr), rz = sum(part_rz)
__global__ __launch_bounds__(256) void pcg_beta_k(const double *__restrict__ part_rr,
                                                  const double *__restrict__ part_rz, int np,
                                                  double *__restrict__ sc, double *__restrict__ norm,
                                                  double *__restrict__ ring_beta, double *__restrict__ ring_rho,
                                                  int first)
{
   __shared__ double red[4];
   const double rr = pcg_sum_partials(part_rr, np, red);
   const double rz = pcg_sum_partials(part_rz, np, red);
   if (threadIdx.x == 0) pcg_beta_q(rr, rz, sc, norm, ring_beta, ring_rho, first);
}

// ---- across ranks -----------------------------------------------------------------
// Each rank sums its own rows exactly as above and writes the one double per
// dot product into its slot; the slots are all-gathered and every rank adds
// them in rank order, s = 0.0; s += v[r], so all ranks hold the same bits
// whatever the transport, and one rank holds the bits of the kernels above.

// this rank's sums: slot[0] = sum(part_a), slot[1] = sum(part_b) (part_b may be null)
__global__ __launch_bounds__(256) void pcg_rank_sum_k(const double *__restrict__ part_a,
                                                      const double *__restrict__ part_b, int np,
                                                      double *__restrict__ slot)
{
   __shared__ double red[4];
   const double a = pcg_sum_partials(part_a, np, red);
   if (threadIdx.x == 0) slot[0] = a;
   if (part_b) {
      const double b = pcg_sum_partials(part_b, np, red);
      if (threadIdx.x == 0) slot[1] = b;
   }
}

// pcg_alpha_q on the gathered rank values v[r] of p.q
__global__ __launch_bounds__(256) void pcg_alpha_ranks_k(const double *__restrict__ v, int nranks,
                                                         double *__restrict__ sc, double *__restrict__ ring_alpha)
{
   if (threadIdx.x == 0) {
      double pq = 0.0;
      for (int r = 0; r < nranks; r++) pq += v[r];
      pcg_alpha_q(pq, sc, ring_alpha);
   }
}

// pcg_beta_q on the gathered rank values (v[2 r], v[2 r + 1]) of (r.r, r.z)
__global__ __launch_bounds__(256) void pcg_beta_ranks_k(const double *__restrict__ v, int nranks,
                                                        double *__restrict__ sc, double *__restrict__ norm,
                                                        double *__restrict__ ring_beta,
                                                        double *__restrict__ ring_rho, int first)
{
   if (threadIdx.x == 0) {
      double rr = 0.0, rz = 0.0;
      for (int r = 0; r < nranks; r++) rr += v[2 * r];
      for (int r = 0; r < nranks; r++) rz += v[2 * r + 1];
      pcg_beta_q(rr, rz, sc, norm, ring_beta, ring_rho, first);
   }
}

// the cycle's zero-guess Jacobi sweep on the new residual, written where r is
// still in registers (PcgZero, amg_internal.h)
__device__ __forceinline__ void pcg_zero_sweep(const PcgZero &zg, long long i, double ri)
{
   if (zg.l1) {
      zg.u[i] = ri / zg.l1[i];
   } else {
      const double a = zg.diag ? zg.diag[i] : zg.a;
      zg.u[i] = a != 0.0 ? zg.w * ri / a : 0.0;
   }
}

// x += alpha p;  r -= alpha q;  the partials of r.r on the reduction grid.  Four
// grid strides are loaded ahead; a lane still adds its squares in index order.
template <bool ZG>
__global__ __launch_bounds__(256) void pcg_xr_k(double *__restrict__ x, const double *__restrict__ p,
                                                double *__restrict__ r, const double *__restrict__ q, int n,
                                                const double *__restrict__ sc, double *__restrict__ partials,
                                                PcgZero zg)
{
   __shared__ double red[4];
   const double alpha = sc[PCG_ALPHA];
   const long long st = (long long)gridDim.x * 256;
   long long i = (long long)blockIdx.x * 256 + threadIdx.x;
   double s = 0.0;
   for (; i + 3 * st < n; i += 4 * st) {
      double xv[4], pv[4], rv[4], qv[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
         xv[k] = x[i + k * st];
         pv[k] = p[i + k * st];
         rv[k] = r[i + k * st];
         qv[k] = q[i + k * st];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
         x[i + k * st] = xv[k] + alpha * pv[k];
         const double ri = rv[k] - alpha * qv[k];
         r[i + k * st] = ri;
         if (ZG) pcg_zero_sweep(zg, i + k * st, ri);
         s += ri * ri;
      }
   }
   for (; i < n; i += st) {
      x[i] = x[i] + alpha * p[i];
      const double ri = r[i] - alpha * q[i];
      r[i] = ri;
      if (ZG) pcg_zero_sweep(zg, i, ri);
      s += ri * ri;
   }
   s = block_sum_256(s, red);
   if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// p = z + beta p
__global__ __launch_bounds__(256) void pcg_p_k(const double *__restrict__ z, double *__restrict__ p, int n,
                                               const double *__restrict__ sc)
{
   const double beta = sc[PCG_BETA];
   const long long st = (long long)gridDim.x * 256;
   for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += st) p[i] = z[i] + beta * p[i];
}

void pcg_alpha(hipStream_t s, const double *part, int np, double *sc, double *ring_alpha)
{
   pcg_alpha_k<<<1, 256, 0, s>>>(part, np, sc, ring_alpha);
}

void pcg_beta(hipStream_t s, const double *part_rr, const double *part_rz, int np, double *sc, double *norm,
              double *ring_beta, double *ring_rho, int first)
{
   pcg_beta_k<<<1, 256, 0, s>>>(part_rr, part_rz, np, sc, norm, ring_beta, ring_rho, first);
}

void pcg_rank_sum(hipStream_t s, const double *part_a, const double *part_b, int np, double *slot)
{
   pcg_rank_sum_k<<<1, 256, 0, s>>>(part_a, part_b, np, slot);
}

void pcg_alpha_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *ring_alpha)
{
   pcg_alpha_ranks_k<<<1, 256, 0, s>>>(v, nranks, sc, ring_alpha);
}

void pcg_beta_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *norm, double *ring_beta,
                    double *ring_rho, int first)
{
   pcg_beta_ranks_k<<<1, 256, 0, s>>>(v, nranks, sc, norm, ring_beta, ring_rho, first);
}

void pcg_update_xr(hipStream_t s, double *x, const double *p, double *r, const double *q, int n,
                   const double *sc, double *partials, int *nparts, const PcgZero &zg)
{
   const int nb = red_blocks(n);
   if (zg.u)
      pcg_xr_k<true><<<nb, 256, 0, s>>>(x, p, r, q, n, sc, partials, zg);
   else
      pcg_xr_k<false><<<nb, 256, 0, s>>>(x, p, r, q, n, sc, partials, PcgZero{});
   *nparts = nb;
}

void pcg_update_p(hipStream_t s, const double *z, double *p, int n, const double *sc)
{
   if (n > 0) pcg_p_k<<<std::min((n + 255) / 256, 1024), 256, 0, s>>>(z, p, n, sc);
}

} // namespace amgk
