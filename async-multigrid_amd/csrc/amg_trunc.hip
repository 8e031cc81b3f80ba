// amg_trunc.hip -- interpolation truncation on the GPU: the rule of hypre's
// hypre_BoomerAMGInterpTruncation behind the reference's -P_max_elmts /
// -add_P_max_elmts / -add_trunc_factor (DMEM_Main.cpp:49-51,519-531,
// DMEM_Setup.cpp:541,573,591-592, SMEM_Setup.cpp:1686), restated host-side in
// amg_classical.cpp::truncate_rows (hypre is not in the reference tree: parity
// unpinned).  Device CSR in, device CSR out, bit-identical to the host.
//
// One wavefront per row, rows of any length walked in chunks of 64 entries:
//   threshold pass  m = max |v| (wave reduction: exact in any order); entries
//                   with |v| < trunc_factor m go; s = sum of the row, k = sum of
//                   the kept entries, both serial in storage order; f1 = s / k
//   count pass      on w = v f1: rank of an entry = how many entries precede it
//                   in the total order (|w| descending, column ascending,
//                   position ascending), counted against every chunk of the
//                   row broadcast lane by lane -- exact, no sort; the max_elmts
//                   entries of rank < max_elmts stay; s, k as above; f2 = s / k
// The serial sums are formed by every lane alike from wave-uniform broadcasts
// of the chunk's values in storage order, so they are the host's sums.  The
// row kernel leaves one keep flag per entry, the kept count and (f1, f2) per
// row; the counts are scanned on the host (amg_csr.h's rowptr_of_counts: the
// entry count sizes the output) and the pack kernel writes kept entries in column
// order with their value rescaled by one multiply per pass that dropped.
#include <algorithm>
#include <vector>

#include "amg_csr.h"

namespace {

constexpr int TRUNC_BLOCK = 256; // 4 wavefronts: 4 rows in flight per workgroup

__device__ inline bool trunc_precedes(double at, int ct, int pt, double ai, int ci, int pi)
{
   return at > ai || (at == ai && (ct < ci || (ct == ci && pt < pi)));
}

// keep[k] for every entry, cnt[r], fac[2 r] = f1, fac[2 r + 1] = f2, mode[r]
// bit 0 / 1: pass 1 / 2 rescales
__global__ __launch_bounds__(TRUNC_BLOCK) void trunc_row_k(const int *__restrict__ rp, const int *__restrict__ cj,
                                                           const double *__restrict__ v, int n, double tf, int maxel,
                                                           unsigned char *__restrict__ keep, int *__restrict__ cnt,
                                                           double *__restrict__ fac, int *__restrict__ mode)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = rp[r], len = rp[r + 1] - b;
      const bool p1 = tf > 0.0 && len > 1; // a row of one entry keeps it: |v| < tf |v| never holds
      double thr = 0.0, f1 = 1.0, f2 = 1.0;
      int m1 = 0, m2 = 0, n1 = len;
      if (p1) {
         double m = 0.0;
         for (int i = lane; i < len; i += 64) m = fmax(m, fabs(v[b + i]));
         for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
         thr = tf * m;
         double s = 0.0, k = 0.0;
         n1 = 0;
         for (int c0 = 0; c0 < len; c0 += 64) {
            const int i = c0 + lane;
            const double x = i < len ? v[b + i] : 0.0;
            const unsigned long long km = __ballot(i < len && !(fabs(x) < thr));
            const int cl = min(64, len - c0);
            for (int t = 0; t < cl; t++) {
               const double xt = __shfl(x, t, 64);
               s += xt;
               if ((km >> t) & 1ull) k += xt;
            }
            n1 += __popcll(km);
         }
         if (n1 < len && k != 0.0) {
            f1 = s / k;
            m1 = 1;
         }
      }
      int n2 = n1;
      if (maxel > 0 && n1 > maxel) {
         double s = 0.0, k = 0.0;
         n2 = 0;
         for (int c0 = 0; c0 < len; c0 += 64) {
            const int i = c0 + lane;
            const double x = i < len ? v[b + i] : 0.0;
            const int ci = i < len ? cj[b + i] : 0;
            const bool in1 = i < len && !(p1 && fabs(x) < thr);
            const double w = m1 ? x * f1 : x;
            const double ai = in1 ? fabs(w) : -1.0;
            int rank = 0;
            for (int d0 = 0; d0 < len; d0 += 64) {
               const int j = d0 + lane;
               const double xj = j < len ? v[b + j] : 0.0;
               const int cjj = j < len ? cj[b + j] : 0;
               const bool jn1 = j < len && !(p1 && fabs(xj) < thr);
               const double aj = jn1 ? fabs(m1 ? xj * f1 : xj) : -1.0; // -1: precedes nothing
               const int dl = min(64, len - d0);
               for (int t = 0; t < dl; t++)
                  rank += trunc_precedes(__shfl(aj, t, 64), __shfl(cjj, t, 64), d0 + t, ai, ci, i) ? 1 : 0;
            }
            const bool kp = in1 && rank < maxel;
            const unsigned long long k1 = __ballot(in1), k2 = __ballot(kp);
            const int cl = min(64, len - c0);
            for (int t = 0; t < cl; t++) {
               const double wt = __shfl(w, t, 64);
               if ((k1 >> t) & 1ull) s += wt;
               if ((k2 >> t) & 1ull) k += wt;
            }
            if (i < len) keep[b + i] = kp ? 1 : 0;
            n2 += __popcll(k2);
         }
         if (k != 0.0) {
            f2 = s / k;
            m2 = 2;
         }
      } else {
         for (int i = lane; i < len; i += 64) keep[b + i] = (p1 && fabs(v[b + i]) < thr) ? 0 : 1;
      }
      if (lane == 0) {
         cnt[r] = n2;
         fac[2 * (size_t)r] = f1;
         fac[2 * (size_t)r + 1] = f2;
         mode[r] = m1 | m2;
      }
   }
}

// kept entries of row r to orp[r]..orp[r + 1], in storage order
__global__ __launch_bounds__(TRUNC_BLOCK) void trunc_pack_k(const int *__restrict__ rp, const int *__restrict__ cj,
                                                            const double *__restrict__ v, int n,
                                                            const unsigned char *__restrict__ keep,
                                                            const int *__restrict__ orp, const double *__restrict__ fac,
                                                            const int *__restrict__ mode, int *__restrict__ ocj,
                                                            double *__restrict__ ov)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = rp[r], len = rp[r + 1] - b, md = mode[r];
      const double f1 = fac[2 * (size_t)r], f2 = fac[2 * (size_t)r + 1];
      int o = orp[r];
      for (int c0 = 0; c0 < len; c0 += 64) {
         const int i = c0 + lane;
         const bool kp = i < len && keep[b + i] != 0;
         const unsigned long long km = __ballot(kp);
         if (kp) {
            const int p = o + __popcll(km & ((1ull << lane) - 1ull));
            double x = v[b + i];
            if (md & 1) x = x * f1;
            if (md & 2) x = x * f2;
            ocj[p] = cj[b + i];
            ov[p] = x;
         }
         o += __popcll(km);
      }
   }
}

} // namespace

// rows of a device CSR truncated (trunc_factor, max_elmts); T's arrays are allocated here
int trunc_dev(hipStream_t s, const DCsr &M, double tf, int maxel, DCsr &T)
{
   const int n = M.n;
   DBuf<unsigned char> d_keep;
   DBuf<int> d_cnt, d_mode;
   DBuf<double> d_fac;
   AMG_TRY(d_keep.alloc((size_t)M.nnz));
   AMG_TRY(d_cnt.alloc((size_t)n));
   AMG_TRY(d_mode.alloc((size_t)n));
   AMG_TRY(d_fac.alloc(2 * (size_t)n));
   const int wpb = TRUNC_BLOCK / 64;
   const int grid = (int)std::min<long long>(((long long)n + wpb - 1) / wpb, 8192);
   trunc_row_k<<<grid, TRUNC_BLOCK, 0, s>>>(M.rp, M.cj, M.v, n, tf, maxel, d_keep, d_cnt, d_fac, d_mode);
   AMG_HIP(hipGetLastError());
   std::vector<int> rp;
   AMG_TRY(rowptr_of_counts(s, d_cnt, n, rp, T.rp));
   T.n = M.n, T.m = M.m, T.nnz = rp[n];
   AMG_TRY(T.cj.alloc((size_t)T.nnz));
   AMG_TRY(T.v.alloc((size_t)T.nnz));
   trunc_pack_k<<<grid, TRUNC_BLOCK, 0, s>>>(M.rp, M.cj, M.v, n, d_keep, T.rp, d_fac, d_mode, T.cj, T.v);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipStreamSynchronize(s)); // rp leaves scope
   return AMG_OK;
}

// host CSR in and out through device `device` (bit-identical to truncate_rows)
int amg_truncate_device(int device, const HCsrView &M, double tf, int maxel, HCsr &T)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dM, dT;
   AMG_TRY(upload_csr(ss.s, M, true, dM));
   AMG_TRY(trunc_dev(ss.s, dM, tf, maxel, dT));
   AMG_TRY(download_csr(ss.s, dT, true, T));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}
