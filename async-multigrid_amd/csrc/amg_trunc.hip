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
// row; the counts are scanned on the host (spgemm_dev's scheme: the entry
// count sizes the output) and the pack kernel writes kept entries in column
// order with their value rescaled by one multiply per pass that dropped.
#include <algorithm>
#include <vector>

#include "amg_internal.h"

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

// rows of a device CSR truncated (trunc_factor, max_elmts): the result's rowptr /
// col / val are allocated here and its entry count returned in *onnz
int amg_trunc_dev(hipStream_t s, int n, const int *d_rp, const int *d_cj, const double *d_v, long long nnz, double tf,
                  int maxel, int **d_orp, int **d_ocj, double **d_ov, long long *onnz)
{
   unsigned char *d_keep = nullptr;
   int *d_cnt = nullptr, *d_mode = nullptr, *orp = nullptr, *ocj = nullptr;
   double *d_fac = nullptr, *ov = nullptr;
   auto run = [&]() -> int {
      AMG_HIP(hipMalloc(&d_keep, (size_t)std::max(nnz, 1LL)));
      AMG_HIP(hipMalloc(&d_cnt, (size_t)n * sizeof(int)));
      AMG_HIP(hipMalloc(&d_mode, (size_t)n * sizeof(int)));
      AMG_HIP(hipMalloc(&d_fac, 2 * (size_t)n * sizeof(double)));
      const int wpb = TRUNC_BLOCK / 64;
      const int grid = (int)std::min<long long>(((long long)n + wpb - 1) / wpb, 8192);
      trunc_row_k<<<grid, TRUNC_BLOCK, 0, s>>>(d_rp, d_cj, d_v, n, tf, maxel, d_keep, d_cnt, d_fac, d_mode);
      AMG_HIP(hipGetLastError());
      std::vector<int> cnt(n), rp(n + 1, 0);
      AMG_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
      AMG_HIP(hipStreamSynchronize(s));
      for (int r = 0; r < n; r++) rp[r + 1] = rp[r] + cnt[r];
      AMG_HIP(hipMalloc(&orp, ((size_t)n + 1) * sizeof(int)));
      AMG_HIP(hipMalloc(&ocj, (size_t)std::max(rp[n], 1) * sizeof(int)));
      AMG_HIP(hipMalloc(&ov, (size_t)std::max(rp[n], 1) * sizeof(double)));
      AMG_HIP(hipMemcpyAsync(orp, rp.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, s));
      trunc_pack_k<<<grid, TRUNC_BLOCK, 0, s>>>(d_rp, d_cj, d_v, n, d_keep, orp, d_fac, d_mode, ocj, ov);
      AMG_HIP(hipGetLastError());
      AMG_HIP(hipStreamSynchronize(s)); // rp leaves scope
      *onnz = rp[n];
      return AMG_OK;
   };
   const int st = run();
   hipStreamSynchronize(s);
   for (void *p : {(void *)d_keep, (void *)d_cnt, (void *)d_mode, (void *)d_fac}) hipFree(p);
   if (st != AMG_OK) {
      for (void *p : {(void *)orp, (void *)ocj, (void *)ov}) hipFree(p);
      return st;
   }
   *d_orp = orp;
   *d_ocj = ocj;
   *d_ov = ov;
   return AMG_OK;
}

// host CSR in and out through device `device` (bit-identical to truncate_rows)
int amg_truncate_device(int device, int n, const int *rp, const int *cj, const double *v, double tf, int maxel,
                        std::vector<int> &orp, std::vector<int> &ocj, std::vector<double> &ov)
{
   AMG_HIP(hipSetDevice(device));
   hipStream_t s;
   AMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
   const long long nnz = rp[n];
   int *d_rp = nullptr, *d_cj = nullptr, *d_orp = nullptr, *d_ocj = nullptr;
   double *d_v = nullptr, *d_ov = nullptr;
   long long onnz = 0;
   auto run = [&]() -> int {
      AMG_HIP(hipMalloc(&d_rp, ((size_t)n + 1) * sizeof(int)));
      AMG_HIP(hipMalloc(&d_cj, (size_t)std::max(nnz, 1LL) * sizeof(int)));
      AMG_HIP(hipMalloc(&d_v, (size_t)std::max(nnz, 1LL) * sizeof(double)));
      AMG_HIP(hipMemcpyAsync(d_rp, rp, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, s));
      if (nnz) {
         AMG_HIP(hipMemcpyAsync(d_cj, cj, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
         AMG_HIP(hipMemcpyAsync(d_v, v, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, s));
      }
      AMG_TRY(amg_trunc_dev(s, n, d_rp, d_cj, d_v, nnz, tf, maxel, &d_orp, &d_ocj, &d_ov, &onnz));
      orp.resize((size_t)n + 1);
      ocj.resize((size_t)onnz);
      ov.resize((size_t)onnz);
      AMG_HIP(hipMemcpyAsync(orp.data(), d_orp, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
      if (onnz) {
         AMG_HIP(hipMemcpyAsync(ocj.data(), d_ocj, (size_t)onnz * sizeof(int), hipMemcpyDeviceToHost, s));
         AMG_HIP(hipMemcpyAsync(ov.data(), d_ov, (size_t)onnz * sizeof(double), hipMemcpyDeviceToHost, s));
      }
      AMG_HIP(hipStreamSynchronize(s));
      return AMG_OK;
   };
   const int st = run();
   hipStreamSynchronize(s);
   for (void *p : {(void *)d_rp, (void *)d_cj, (void *)d_v, (void *)d_orp, (void *)d_ocj, (void *)d_ov}) hipFree(p);
   hipStreamDestroy(s);
   return st;
}
