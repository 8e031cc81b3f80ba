// amg_mrhs.hip -- the row operators, reductions and PCG updates over K right-hand
// sides at once (K = 2, 4, 8).  A multivector is n x K row-major, so the K values
// of a row are one contiguous 8 K-byte segment: every entry's gather x[col] is one
// segment load, and the matrix -- rowptr, col, val of the plain CSR form -- is read
// once per launch for all K columns.  Per column the arithmetic is the single-vector
// tile kernel's (amg_kernels.hip): the accumulator starts at the epilogue's init,
// each product a_ik x_k is rounded on its own (-ffp-contract=off), the products are
// added or subtracted in storage order, then the epilogue's finish; the dot products
// are summed in amg_vec_dot's order.  Column j of every result therefore carries the
// bits of the single-vector entry point on column j, whatever storage form that one
// picks.  Out of scope here: the compressed matrix forms, other widths.
#include <algorithm>

#include "amg_internal.h"

namespace amgk {

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

// K consecutive doubles at a 16-byte aligned address (a multivector row), as
// K / 2 16-byte loads / stores
template <int K>
__device__ __forceinline__ void ldk(const double *p, double (&v)[K])
{
#pragma unroll
   for (int j = 0; j < K; j += 2) {
      const v2d t = *reinterpret_cast<const v2d *>(p + j);
      v[j] = t.x;
      v[j + 1] = t.y;
   }
}

template <int K>
__device__ __forceinline__ void stk(double *p, const double (&v)[K])
{
#pragma unroll
   for (int j = 0; j < K; j += 2) *reinterpret_cast<v2d *>(p + j) = v2d{v[j], v[j + 1]};
}

// entries per LDS chunk: 4096 products (32 KiB) for every K, so each instance
// leaves five workgroups per CU
template <int K>
struct MrhsCfg {
   static constexpr int ch = 4096 / K;
};

// ---- epilogues: init(row, acc) the accumulators' start; pf(row, v) operands issued
// before the stream; finish(row, acc, a_ii, pf) writes the row's K outputs ----

// EpiGemv per column (SMEM_MatVec.cpp:140-258).  b may alias y: the row's K values
// of b are in registers before its outputs are written, by the same lane
template <int K>
struct MEpiGemv {
   const double *b;
   double *y;
   int imode, scale;
   double alpha, temp;
   __device__ __forceinline__ void init(int i, double (&acc)[K]) const
   {
      if (imode == 0) {
#pragma unroll
         for (int j = 0; j < K; j++) acc[j] = 0.0;
         return;
      }
      double bb[K];
      ldk<K>(b + (size_t)i * K, bb);
#pragma unroll
      for (int j = 0; j < K; j++) {
         switch (imode) {
         case 1: acc[j] = bb[j]; break;
         case 2: acc[j] = -bb[j]; break;
         case 3: acc[j] = bb[j] * temp; break;
         default: acc[j] = -bb[j] * temp; break;
         }
      }
   }
   __device__ __forceinline__ void pf(int, double (&)[K]) const {}
   __device__ __forceinline__ void finish(int i, const double (&acc)[K], double, const double (&)[K]) const
   {
      double v[K];
#pragma unroll
      for (int j = 0; j < K; j++) v[j] = scale ? alpha * acc[j] : acc[j];
      stk<K>(y + (size_t)i * K, v);
   }
   // one column of the row (the long-row kernel: a lane per (row, column))
   __device__ __forceinline__ double init1(int i, int j) const
   {
      if (imode == 0) return 0.0;
      const double bb = b[(size_t)i * K + j];
      switch (imode) {
      case 1: return bb;
      case 2: return -bb;
      case 3: return bb * temp;
      default: return -bb * temp;
      }
   }
   __device__ __forceinline__ double pf1(int, int) const { return 0.0; }
   __device__ __forceinline__ void finish1(int i, int j, double acc, double, double) const
   {
      y[(size_t)i * K + j] = scale ? alpha * acc : acc;
   }
};

// EpiJacobi per column (SMEM_Smooth.cpp:35-45): u_new = u + (w res) / a where a != 0
template <int K>
struct MEpiJacobi {
   const double *f;
   const double *x;
   double *out;
   double omega;
   __device__ __forceinline__ void init(int i, double (&acc)[K]) const { ldk<K>(f + (size_t)i * K, acc); }
   __device__ __forceinline__ void pf(int i, double (&v)[K]) const { ldk<K>(x + (size_t)i * K, v); }
   __device__ __forceinline__ void finish(int i, const double (&res)[K], double a, const double (&xi)[K]) const
   {
      double v[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
         const double q = (omega * res[j]) / a;
         v[j] = (a != 0.0) ? xi[j] + q : xi[j];
      }
      stk<K>(out + (size_t)i * K, v);
   }
   __device__ __forceinline__ double init1(int i, int j) const { return f[(size_t)i * K + j]; }
   __device__ __forceinline__ double pf1(int i, int j) const { return x[(size_t)i * K + j]; }
   __device__ __forceinline__ void finish1(int i, int j, double res, double a, double xi) const
   {
      const double q = (omega * res) / a;
      out[(size_t)i * K + j] = (a != 0.0) ? xi + q : xi;
   }
};

// EpiL1Jacobi per column (SMEM_Smooth.cpp:122-130): u_new = u + res / l1, one l1 per row
template <int K>
struct MEpiL1Jacobi {
   const double *f;
   const double *x;
   const double *l1;
   double *out;
   __device__ __forceinline__ void init(int i, double (&acc)[K]) const { ldk<K>(f + (size_t)i * K, acc); }
   __device__ __forceinline__ void pf(int i, double (&v)[K]) const { ldk<K>(x + (size_t)i * K, v); }
   __device__ __forceinline__ void finish(int i, const double (&res)[K], double, const double (&xi)[K]) const
   {
      const double l = l1[i];
      double v[K];
#pragma unroll
      for (int j = 0; j < K; j++) v[j] = xi[j] + res[j] / l;
      stk<K>(out + (size_t)i * K, v);
   }
   __device__ __forceinline__ double init1(int i, int j) const { return f[(size_t)i * K + j]; }
   __device__ __forceinline__ double pf1(int i, int j) const { return x[(size_t)i * K + j]; }
   __device__ __forceinline__ void finish1(int i, int j, double res, double, double xi) const
   {
      out[(size_t)i * K + j] = xi + res / l1[i];
   }
};

// a chunk's products into LDS as [entry][K]: lane t stages entries cs + t, + 256, ... (col
// and val coalesced), two at a time, each as one 8 K-byte load of x's row col and K
// rounded products
template <int K>
__device__ __forceinline__ void stage_chunk(const int *__restrict__ col, const double *__restrict__ val,
                                            const double *__restrict__ x, int cs, int ce, double *prod)
{
   for (int k = cs + (int)threadIdx.x; k < ce; k += 2 * 256) {
      const int k2 = k + 256;
      const bool has2 = k2 < ce;
      const int c0 = col[k];
      const double v0 = val[k];
      int c1 = 0;
      double v1 = 0.0;
      if (has2) {
         c1 = col[k2];
         v1 = val[k2];
      }
      double x0[K], x1[K];
      ldk<K>(x + (size_t)c0 * K, x0);
      if (has2) ldk<K>(x + (size_t)c1 * K, x1);
#pragma unroll
      for (int j = 0; j < K; j++) x0[j] = v0 * x0[j];
      stk<K>(prod + (k - cs) * K, x0);
      if (has2) {
#pragma unroll
         for (int j = 0; j < K; j++) x1[j] = v1 * x1[j];
         stk<K>(prod + (k2 - cs) * K, x1);
      }
   }
}

// Short rows.  One 256-row tile per workgroup, one row per lane with K accumulators.  The
// tile's entries are walked in chunks of MrhsCfg<K>::ch (stage_chunk); then every lane adds
// its own row's products of the chunk in CSR order.  A row longer than a chunk carries its
// accumulators from chunk to chunk.  Rows [rb, re), re <= nrows.
template <int K, int NEG, bool NEED_DIAG, class Epi>
__global__ __launch_bounds__(256) void csr_mrhs_kernel(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const double *__restrict__ val,
                                                       const double *__restrict__ x, int rb, int re, Epi epi)
{
   constexpr int CH = MrhsCfg<K>::ch;
   __shared__ __attribute__((aligned(16))) double prod[CH * K];
   const int tid = (int)threadIdx.x;
   const int r0 = rb + (int)blockIdx.x * 256;
   const int r1 = min(r0 + 256, re);
   const int row = r0 + tid;
   const int tb = rowptr[r0], te = rowptr[r1];
   int rs = 0, rend = 0;
   double acc[K], pf[K], dg = 0.0;
#pragma unroll
   for (int j = 0; j < K; j++) acc[j] = pf[j] = 0.0;
   if (row < r1) {
      rs = rowptr[row];
      rend = rowptr[row + 1];
      epi.init(row, acc);
      epi.pf(row, pf);
      if (NEED_DIAG) dg = val[rs]; // a_ii := A_data[A_i[i]]
   }
   for (int cs = tb; cs < te; cs += CH) {
      const int ce = min(cs + CH, te);
      stage_chunk<K>(col, val, x, cs, ce, prod);
      __syncthreads();
      const int a = max(rs, cs), e = min(rend, ce);
      for (int k = a; k < e; ++k) {
         double p[K];
         ldk<K>(prod + (k - cs) * K, p);
#pragma unroll
         for (int j = 0; j < K; j++) {
            if (NEG)
               acc[j] -= p[j];
            else
               acc[j] += p[j];
         }
      }
      __syncthreads(); // WAR on prod before the next chunk
   }
   if (row < r1) epi.finish(row, acc, dg, pf);
}

// Long rows (classical coarse levels, elasticity).  A (row, column) sum is one serial chain
// of rounded additions in CSR order, so what bounds a workgroup is how many chains it
// advances at once.  A chunk of contiguous entries covers only a few long rows and leaves
// most lanes without work; here a chunk is the next S = 16 entries of EVERY row of the tile
// instead.  The tile is R = 256 / K rows and a lane owns one chain -- lane t row t / K,
// column t % K -- so in every chunk all 256 lanes stage (entry slot (row, s) = lane t + 256 i,
// row (t + 256 i) / S: 16 consecutive entries of a row per 16 lanes) and all 256 add.  The
// products lie in LDS as [row][S + 1][K]: the spare slot turns the row stride into 8 (K = 4)
// banks mod 64, so the rows of a wave read different banks.  The tile runs
// ceil(longest row / S) chunks.  The epilogue's loads and stores are contiguous over the lanes.
template <int K, int NEG, bool NEED_DIAG, class Epi>
__global__ __launch_bounds__(256) void csr_mrhs_long_kernel(const int *__restrict__ rowptr,
                                                            const int *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ x, int rb, int re, Epi epi)
{
   constexpr int R = 256 / K, S = 16, ST = (S + 1) * K;
   __shared__ __attribute__((aligned(16))) double prod[R * ST];
   __shared__ int rp[R + 1];
   __shared__ int longest;
   const int tid = (int)threadIdx.x;
   const int r0 = rb + (int)blockIdx.x * R;
   const int r1 = min(r0 + R, re), nr = r1 - r0;
   if (tid == 0) longest = 0;
   if (tid <= nr) rp[tid] = rowptr[r0 + tid];
   __syncthreads();
   if (tid < nr) atomicMax(&longest, rp[tid + 1] - rp[tid]);
   __syncthreads();
   const int maxlen = longest;
   const int lr = tid / K, j = tid % K, row = r0 + lr;
   const bool own = lr < nr;
   int len = 0;
   double acc = 0.0, pf = 0.0, dg = 0.0;
   if (own) {
      const int rs = rp[lr];
      len = rp[lr + 1] - rs;
      acc = epi.init1(row, j);
      pf = epi.pf1(row, j);
      if (NEED_DIAG) dg = val[rs]; // a_ii := A_data[A_i[i]]
   }
   for (int c0 = 0; c0 < maxlen; c0 += S) {
      for (int e = tid; e < R * S; e += 2 * 256) {
         const int e2 = e + 256;
         const int ra = e / S, sa = e % S, rb2 = e2 / S, sb = e2 % S;
         const bool va = ra < nr && c0 + sa < rp[ra + 1] - rp[ra];
         const bool vb = e2 < R * S && rb2 < nr && c0 + sb < rp[rb2 + 1] - rp[rb2];
         int ca = 0, cb = 0;
         double wa = 0.0, wb = 0.0;
         if (va) {
            const int k = rp[ra] + c0 + sa;
            ca = col[k];
            wa = val[k];
         }
         if (vb) {
            const int k = rp[rb2] + c0 + sb;
            cb = col[k];
            wb = val[k];
         }
         double xa[K], xb[K];
         if (va) ldk<K>(x + (size_t)ca * K, xa);
         if (vb) ldk<K>(x + (size_t)cb * K, xb);
         if (va) {
#pragma unroll
            for (int q = 0; q < K; q++) xa[q] = wa * xa[q];
            stk<K>(prod + ra * ST + sa * K, xa);
         }
         if (vb) {
#pragma unroll
            for (int q = 0; q < K; q++) xb[q] = wb * xb[q];
            stk<K>(prod + rb2 * ST + sb * K, xb);
         }
      }
      __syncthreads();
      const int m = len - c0; // this row's entries left; the chunk holds the first S of them
#pragma unroll
      for (int sl = 0; sl < S; sl++) {
         if (sl < m) {
            if (NEG)
               acc -= prod[lr * ST + sl * K + j];
            else
               acc += prod[lr * ST + sl * K + j];
         }
      }
      __syncthreads(); // WAR on prod before the next chunk
   }
   if (own) epi.finish1(row, j, acc, dg, pf);
}

// operators of at least this many entries per row on average take the long-row kernel
// (measured: the 27-point coarse levels of the 7-pt hierarchy run faster in tiles)
constexpr int MRHS_LONG_ROW = 32;

template <int K, int NEG, bool NEED_DIAG, class Epi>
void launch_mrhs(hipStream_t s, const amg_mat *A, const double *x, int rb, int re, const Epi &epi)
{
   if (re <= rb) return;
   const long long avg = A->nrows > 0 ? A->nnz / A->nrows : 0;
   if (avg < MRHS_LONG_ROW) {
      csr_mrhs_kernel<K, NEG, NEED_DIAG, Epi>
         <<<(re - rb + 255) / 256, 256, 0, s>>>(A->rowptr, A->col, A->val, x, rb, re, epi);
      return;
   }
   constexpr int R = 256 / K;
   csr_mrhs_long_kernel<K, NEG, NEED_DIAG, Epi>
      <<<(re - rb + R - 1) / R, 256, 0, s>>>(A->rowptr, A->col, A->val, x, rb, re, epi);
}

template <int K>
void spgemv_k(hipStream_t s, const amg_mat *A, const double *x, const double *b, const Gemv &g, double *y, int rb,
              int re)
{
   const MEpiGemv<K> epi{b, y, g.init, g.scale, g.alpha, g.temp};
   if (g.negacc)
      launch_mrhs<K, 1, false>(s, A, x, rb, re, epi);
   else
      launch_mrhs<K, 0, false>(s, A, x, rb, re, epi);
}

template <int K>
void jacobi_k(hipStream_t s, const amg_mat *A, const double *f, const double *x, const double *l1, double omega,
              double *out)
{
   if (l1)
      launch_mrhs<K, 1, false>(s, A, x, 0, A->nrows, MEpiL1Jacobi<K>{f, x, l1, out});
   else
      launch_mrhs<K, 1, true>(s, A, x, 0, A->nrows, MEpiJacobi<K>{f, x, out, omega});
}

// grid of an element-wise kernel over len elements
inline int ew_grid(long long len) { return (int)std::min<long long>((len + 255) / 256, 65536); }

#define MRHS_EW_LOOP(e, len)                                                                   \
   for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < (len); e += (long long)gridDim.x * 256)

// jacobi_zero_k, variant 0, per column: row e / K, its a_ii and l1 shared by the columns
template <int K>
__global__ __launch_bounds__(256) void mrhs_jacobi_zero_k(const double *__restrict__ diag,
                                                          const double *__restrict__ f,
                                                          const double *__restrict__ l1, double omega,
                                                          double *__restrict__ u, long long len)
{
   MRHS_EW_LOOP(e, len)
   {
      const long long i = e / K;
      if (l1) {
         u[e] = f[e] / l1[i];
      } else {
         const double a = diag[i];
         if (a != 0.0) u[e] = omega * f[e] / a;
      }
   }
}

__global__ __launch_bounds__(256) void mrhs_set_k(double *__restrict__ y, double a, long long len)
{
   MRHS_EW_LOOP(e, len) y[e] = a;
}

__global__ __launch_bounds__(256) void mrhs_set_col_k(int K, int j, const double *__restrict__ x,
                                                      double *__restrict__ v, int n)
{
   MRHS_EW_LOOP(i, n) v[i * K + j] = x[i];
}

__global__ __launch_bounds__(256) void mrhs_get_col_k(int K, int j, const double *__restrict__ v,
                                                      double *__restrict__ x, int n)
{
   MRHS_EW_LOOP(i, n) x[i] = v[i * K + j];
}

// vaxpy_k with column e % K's scalar
__global__ __launch_bounds__(256) void mrhs_axpy_k(int K, MrhsScal alpha, const double *__restrict__ x,
                                                   double *__restrict__ y, long long len)
{
   MRHS_EW_LOOP(e, len) y[e] += alpha.a[e & (K - 1)] * x[e];
}

// partials_k with K accumulators: lane t of workgroup b adds rows 256 b + t, += 256
// gridDim, then block_sum_256 per column; column j's partial of workgroup b at
// part[1024 j + b].  DOT 0: x . x
template <int K, int DOT>
__global__ __launch_bounds__(256) void mrhs_partials_k(const double *__restrict__ x, const double *__restrict__ y,
                                                       int n, double *__restrict__ part)
{
   __shared__ double red[4];
   double s[K];
#pragma unroll
   for (int j = 0; j < K; j++) s[j] = 0.0;
   for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
      double xv[K], yv[K];
      ldk<K>(x + i * K, xv);
      if (DOT) ldk<K>(y + i * K, yv);
#pragma unroll
      for (int j = 0; j < K; j++) s[j] += DOT ? xv[j] * yv[j] : xv[j] * xv[j];
   }
#pragma unroll
   for (int j = 0; j < K; j++) {
      const double t = block_sum_256(s[j], red);
      if (threadIdx.x == 0) part[1024 * j + blockIdx.x] = t;
   }
}

// sum_partials_k<<<1, 256>>> per column
__global__ __launch_bounds__(256) void mrhs_reduce_k(int K, const double *__restrict__ part, int np,
                                                     double *__restrict__ out, int do_sqrt)
{
   __shared__ double red[4];
   for (int j = 0; j < K; j++) {
      const double t = pcg_sum_partials(part + 1024 * j, np, red);
      if (threadIdx.x == 0) out[j] = do_sqrt ? sqrt(t) : t;
   }
}

// ---- preconditioned CG on K columns (the statements of amg_pcg.hip per column) ----

// pcg_alpha_k per column
__global__ __launch_bounds__(256) void mrhs_pcg_alpha_k(int K, const double *__restrict__ part, int np,
                                                        double *__restrict__ sc, double *__restrict__ ring_alpha)
{
   __shared__ double red[4];
   for (int j = 0; j < K; j++) {
      const double pq = pcg_sum_partials(part + 1024 * j, np, red);
      if (threadIdx.x == 0) {
         const double alpha = pq != 0.0 ? sc[MRHS_MAXK * PCG_RHO + j] / pq : 0.0;
         sc[MRHS_MAXK * PCG_PQ + j] = pq;
         sc[MRHS_MAXK * PCG_ALPHA + j] = alpha;
         ring_alpha[(size_t)PCG_RING * j] = alpha;
      }
   }
}

// pcg_beta_k per column
__global__ __launch_bounds__(256) void mrhs_pcg_beta_k(int K, const double *__restrict__ part_rr,
                                                       const double *__restrict__ part_rz, int np,
                                                       double *__restrict__ sc, double *__restrict__ norm,
                                                       double *__restrict__ ring_beta,
                                                       double *__restrict__ ring_rho, int first)
{
   __shared__ double red[4];
   for (int j = 0; j < K; j++) {
      const double rr = pcg_sum_partials(part_rr + 1024 * j, np, red);
      const double rz = pcg_sum_partials(part_rz + 1024 * j, np, red);
      if (threadIdx.x == 0) {
         norm[j] = sqrt(rr);
         sc[MRHS_MAXK * PCG_RR + j] = rr;
         if (!first) {
            const double rho = sc[MRHS_MAXK * PCG_RHO + j];
            const double beta = rho != 0.0 ? rz / rho : 0.0;
            sc[MRHS_MAXK * PCG_BETA + j] = beta;
            ring_beta[(size_t)PCG_RING * j] = beta;
            ring_rho[(size_t)PCG_RING * j] = rz;
         } else {
            sc[MRHS_MAXK * PCG_RHO0 + j] = rz;
         }
         sc[MRHS_MAXK * PCG_RHO + j] = rz;
      }
   }
}

// pcg_xr_k per column: x += alpha_j p; r -= alpha_j q; the partials of r . r, a lane
// adding its rows' squares in index order
template <int K>
__global__ __launch_bounds__(256) void mrhs_pcg_xr_k(double *__restrict__ x, const double *__restrict__ p,
                                                     double *__restrict__ r, const double *__restrict__ q, int n,
                                                     const double *__restrict__ sc, double *__restrict__ part)
{
   __shared__ double red[4];
   double alpha[K], s[K];
#pragma unroll
   for (int j = 0; j < K; j++) {
      alpha[j] = sc[MRHS_MAXK * PCG_ALPHA + j];
      s[j] = 0.0;
   }
   for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
      double xv[K], pv[K], rv[K], qv[K];
      ldk<K>(x + i * K, xv);
      ldk<K>(p + i * K, pv);
      ldk<K>(r + i * K, rv);
      ldk<K>(q + i * K, qv);
#pragma unroll
      for (int j = 0; j < K; j++) {
         xv[j] = xv[j] + alpha[j] * pv[j];
         rv[j] = rv[j] - alpha[j] * qv[j];
         s[j] += rv[j] * rv[j];
      }
      stk<K>(x + i * K, xv);
      stk<K>(r + i * K, rv);
   }
#pragma unroll
   for (int j = 0; j < K; j++) {
      const double t = block_sum_256(s[j], red);
      if (threadIdx.x == 0) part[1024 * j + blockIdx.x] = t;
   }
}

// pcg_p_k per column: p = z + beta_j p
__global__ __launch_bounds__(256) void mrhs_pcg_p_k(int K, const double *__restrict__ z, double *__restrict__ p,
                                                    long long len, const double *__restrict__ sc)
{
   MRHS_EW_LOOP(e, len) p[e] = z[e] + sc[MRHS_MAXK * PCG_BETA + (e & (K - 1))] * p[e];
}

} // namespace

#define MRHS_DISPATCH(K, call2, call4, call8) \
   do {                                        \
      if ((K) == 2)                            \
         call2;                                \
      else if ((K) == 4)                       \
         call4;                                \
      else                                     \
         call8;                                \
   } while (0)

void mrhs_spgemv(hipStream_t s, int K, const amg_mat *A, const double *x, const double *b, const Gemv &g,
                 double *y, int rb, int re)
{
   MRHS_DISPATCH(K, spgemv_k<2>(s, A, x, b, g, y, rb, re), spgemv_k<4>(s, A, x, b, g, y, rb, re),
                 spgemv_k<8>(s, A, x, b, g, y, rb, re));
}

void mrhs_jacobi_sweep(hipStream_t s, int K, const amg_mat *A, const double *f, const double *x,
                       const double *l1, double omega, double *out)
{
   MRHS_DISPATCH(K, jacobi_k<2>(s, A, f, x, l1, omega, out), jacobi_k<4>(s, A, f, x, l1, omega, out),
                 jacobi_k<8>(s, A, f, x, l1, omega, out));
}

void mrhs_jacobi_zero(hipStream_t s, int K, const double *diag, const double *f, const double *l1, double omega,
                      double *u, int n)
{
   const long long len = (long long)n * K;
   if (len <= 0) return;
   const int g = ew_grid(len);
   MRHS_DISPATCH(K, (mrhs_jacobi_zero_k<2><<<g, 256, 0, s>>>(diag, f, l1, omega, u, len)),
                 (mrhs_jacobi_zero_k<4><<<g, 256, 0, s>>>(diag, f, l1, omega, u, len)),
                 (mrhs_jacobi_zero_k<8><<<g, 256, 0, s>>>(diag, f, l1, omega, u, len)));
}

void mrhs_set(hipStream_t s, double *y, double a, long long len)
{
   if (len > 0) mrhs_set_k<<<ew_grid(len), 256, 0, s>>>(y, a, len);
}

void mrhs_set_col(hipStream_t s, int K, int j, const double *x, double *v, int n)
{
   if (n > 0) mrhs_set_col_k<<<ew_grid(n), 256, 0, s>>>(K, j, x, v, n);
}

void mrhs_get_col(hipStream_t s, int K, int j, const double *v, double *x, int n)
{
   if (n > 0) mrhs_get_col_k<<<ew_grid(n), 256, 0, s>>>(K, j, v, x, n);
}

void mrhs_axpy(hipStream_t s, int K, const MrhsScal &alpha, const double *x, double *y, int n)
{
   const long long len = (long long)n * K;
   if (len > 0) mrhs_axpy_k<<<ew_grid(len), 256, 0, s>>>(K, alpha, x, y, len);
}

void mrhs_dot_partials(hipStream_t s, int K, const double *x, const double *y, int n, double *part, int *nparts)
{
   const int nb = red_blocks(n);
   if (y)
      MRHS_DISPATCH(K, (mrhs_partials_k<2, 1><<<nb, 256, 0, s>>>(x, y, n, part)),
                    (mrhs_partials_k<4, 1><<<nb, 256, 0, s>>>(x, y, n, part)),
                    (mrhs_partials_k<8, 1><<<nb, 256, 0, s>>>(x, y, n, part)));
   else
      MRHS_DISPATCH(K, (mrhs_partials_k<2, 0><<<nb, 256, 0, s>>>(x, nullptr, n, part)),
                    (mrhs_partials_k<4, 0><<<nb, 256, 0, s>>>(x, nullptr, n, part)),
                    (mrhs_partials_k<8, 0><<<nb, 256, 0, s>>>(x, nullptr, n, part)));
   *nparts = nb;
}

void mrhs_reduce_partials(hipStream_t s, int K, const double *part, int np, double *out, int do_sqrt)
{
   mrhs_reduce_k<<<1, 256, 0, s>>>(K, part, np, out, do_sqrt);
}

void mrhs_pcg_alpha(hipStream_t s, int K, const double *part, int np, double *sc, double *ring_alpha)
{
   mrhs_pcg_alpha_k<<<1, 256, 0, s>>>(K, part, np, sc, ring_alpha);
}

void mrhs_pcg_beta(hipStream_t s, int K, const double *part_rr, const double *part_rz, int np, double *sc,
                   double *norm, double *ring_beta, double *ring_rho, int first)
{
   mrhs_pcg_beta_k<<<1, 256, 0, s>>>(K, part_rr, part_rz, np, sc, norm, ring_beta, ring_rho, first);
}

void mrhs_pcg_update_xr(hipStream_t s, int K, double *x, const double *p, double *r, const double *q, int n,
                        const double *sc, double *part, int *nparts)
{
   const int nb = red_blocks(n);
   MRHS_DISPATCH(K, (mrhs_pcg_xr_k<2><<<nb, 256, 0, s>>>(x, p, r, q, n, sc, part)),
                 (mrhs_pcg_xr_k<4><<<nb, 256, 0, s>>>(x, p, r, q, n, sc, part)),
                 (mrhs_pcg_xr_k<8><<<nb, 256, 0, s>>>(x, p, r, q, n, sc, part)));
   *nparts = nb;
}

void mrhs_pcg_update_p(hipStream_t s, int K, const double *z, double *p, int n, const double *sc)
{
   const long long len = (long long)n * K;
   if (len > 0) mrhs_pcg_p_k<<<ew_grid(len), 256, 0, s>>>(K, z, p, len, sc);
}

} // namespace amgk
