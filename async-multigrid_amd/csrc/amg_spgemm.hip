// amg_spgemm.hip -- Galerkin products of the classical setup on the GPU
// (the R (A P) of HYPRE_BoomerAMGSetup's hypre_BoomerAMGBuildCoarseOperator,
// SMEM_Setup.cpp:55-70 / DMEM_Setup.cpp:169-173, restated host-side in
// amg_classical.cpp::spgemm).
//
// C = A B with one lane per row of C, exactly the host's Gustavson order: the
// lane walks its row's (A entry, B entry) products in order and adds each into
// its column's slot of an open-addressing table in global scratch (a column's
// first contribution lands on 0.0, like the host's acc[c] = 0.0), so every
// entry of C is the same sum of the same rounded products in the same order --
// bit-identical to the host.  The row's distinct columns are then sorted
// ascending (shell sort in the lane's scratch), the diagonal moved first for
// square products, and rows packed by an exclusive scan of their counts.  Rows
// run in batches sized to a scratch budget (upper bound per row: the sum of
// the B rows its A entries name).
// spgemm_dev works on device CSRs (amg_csr.h's DCsr); the amg_*_device entry
// points below it take host CSRs through a stream of their own.
#include <algorithm>
#include <atomic>
#include <numeric>
#include <vector>

#include "amg_csr.h"

namespace {

// scratch budget of one batch of spgemm_dev, in table slots (amg_set_spgemm_scratch)
constexpr long long SPGEMM_BUDGET = 1LL << 29;
std::atomic<long long> g_budget{SPGEMM_BUDGET};

// ub[r] = sum of |B row k| over the entries (r, k) of A
__global__ void spgemm_ub_k(const int *__restrict__ arp, const int *__restrict__ acj, const int *__restrict__ brp,
                            int n, long long *__restrict__ ub)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= n) return;
   long long s = 0;
   for (int k = arp[r]; k < arp[r + 1]; k++) s += brp[acj[k] + 1] - brp[acj[k]];
   ub[r] = s;
}

// rows [r0, r0 + nr): the hash tables at hoff[r - r0] (capacity cap = power of
// two >= 2 ub), then the row's sorted entries at the table's start; cnt[r - r0]
__global__ void spgemm_row_k(const int *__restrict__ arp, const int *__restrict__ acj,
                             const double *__restrict__ av, const int *__restrict__ brp,
                             const int *__restrict__ bcj, const double *__restrict__ bv, int r0, int nr,
                             const long long *__restrict__ hoff, int *__restrict__ hcol,
                             double *__restrict__ hval, int *__restrict__ cnt, int square)
{
   const int q = blockIdx.x * blockDim.x + threadIdx.x;
   if (q >= nr) return;
   const int r = r0 + q;
   const long long base = hoff[q];
   const int cap = (int)(hoff[q + 1] - base);
   int *hc = hcol + base;
   double *hv = hval + base;
   for (int i = 0; i < cap; i++) hc[i] = -1;
   const unsigned mask = (unsigned)cap - 1u;
   for (int ka = arp[r]; ka < arp[r + 1]; ka++) {
      const int k = acj[ka];
      const double a = av[ka];
      for (int kb = brp[k]; kb < brp[k + 1]; kb++) {
         const int c = bcj[kb];
         unsigned h = ((unsigned)c * 2654435761u) & mask;
         while (hc[h] != c && hc[h] != -1) h = (h + 1) & mask;
         if (hc[h] == -1) {
            hc[h] = c;
            hv[h] = 0.0;
         }
         hv[h] += a * bv[kb];
      }
   }
   // compact the occupied slots to the table's start (scan order), then sort
   int m = 0;
   for (int i = 0; i < cap; i++)
      if (hc[i] != -1) {
         const int c = hc[i];
         const double v = hv[i];
         hc[m] = c;
         hv[m] = v;
         m++;
      }
   // shell sort by column (columns are distinct)
   for (int gap = m / 2; gap > 0; gap /= 2)
      for (int i = gap; i < m; i++) {
         const int c = hc[i];
         const double v = hv[i];
         int j = i;
         for (; j >= gap && hc[j - gap] > c; j -= gap) {
            hc[j] = hc[j - gap];
            hv[j] = hv[j - gap];
         }
         hc[j] = c;
         hv[j] = v;
      }
   if (square) {
      // diag_first: the diagonal moved to the front, the rest keeping order
      for (int i = 0; i < m; i++)
         if (hc[i] == r) {
            const double v = hv[i];
            for (int j = i; j > 0; j--) {
               hc[j] = hc[j - 1];
               hv[j] = hv[j - 1];
            }
            hc[0] = r;
            hv[0] = v;
            break;
         }
   }
   cnt[q] = m;
}

__global__ void spgemm_pack_k(const long long *__restrict__ hoff, const int *__restrict__ hcol,
                              const double *__restrict__ hval, const long long *__restrict__ ooff, int nr,
                              int *__restrict__ ocol, double *__restrict__ oval)
{
   const int q = blockIdx.x;
   if (q >= nr) return;
   const long long b = hoff[q], o = ooff[q], m = ooff[q + 1] - o;
   for (long long i = threadIdx.x; i < m; i += blockDim.x) {
      ocol[o + i] = hcol[b + i];
      oval[o + i] = hval[b + i];
   }
}

} // namespace

// C = A B with every operand on the device; C's arrays are allocated here
int spgemm_dev(hipStream_t s, const DCsr &A, const DCsr &B, DCsr &C)
{
   const int An = A.n;
   DBuf<long long> d_ub, d_hoff, d_ooff;
   DBuf<int> d_hcol, d_cnt, d_ocol, c_col;
   DBuf<double> d_hval, d_oval, c_val;
   long long c_cap = 0;
   AMG_TRY(d_ub.alloc((size_t)An));
   if (An > 0) spgemm_ub_k<<<(An + 255) / 256, 256, 0, s>>>(A.rp, A.cj, B.rp, An, d_ub);
   std::vector<long long> ub;
   AMG_TRY(download(s, d_ub.p, (size_t)An, ub));
   AMG_HIP(hipStreamSynchronize(s));
   // table capacity per row: a power of two >= 2 ub (>= 2)
   std::vector<long long> capr(An);
   for (int r = 0; r < An; r++) {
      long long c = 2;
      while (c < 2 * ub[r]) c <<= 1;
      capr[r] = c;
   }
   // batches of rows within the scratch budget (12 bytes per slot: 6 GiB by default)
   const std::vector<int> cut = batch_bounds(capr, g_budget.load());
   long long maxb = 1;
   for (size_t b = 0; b + 1 < cut.size(); b++)
      maxb = std::max(maxb, std::accumulate(capr.begin() + cut[b], capr.begin() + cut[b + 1], 0LL));
   AMG_TRY(d_hcol.alloc((size_t)maxb));
   AMG_TRY(d_hval.alloc((size_t)maxb));
   AMG_TRY(d_hoff.alloc((size_t)An + 1));
   AMG_TRY(d_ooff.alloc((size_t)An + 1));
   AMG_TRY(d_cnt.alloc((size_t)An));
   AMG_TRY(d_ocol.alloc((size_t)maxb));
   AMG_TRY(d_oval.alloc((size_t)maxb));
   std::vector<int> crp(An + 1, 0);
   long long used = 0;
   for (size_t b = 0; b + 1 < cut.size(); b++) {
      const int r0 = cut[b], nr = cut[b + 1] - r0;
      std::vector<long long> hoff(nr + 1, 0);
      for (int q = 0; q < nr; q++) hoff[q + 1] = hoff[q] + capr[r0 + q];
      AMG_HIP(hipMemcpyAsync(d_hoff, hoff.data(), (nr + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
      spgemm_row_k<<<(nr + 127) / 128, 128, 0, s>>>(A.rp, A.cj, A.v, B.rp, B.cj, B.v, r0, nr, d_hoff, d_hcol, d_hval,
                                                    d_cnt, A.n == B.m ? 1 : 0);
      AMG_HIP(hipGetLastError());
      std::vector<int> cnt;
      AMG_TRY(download(s, d_cnt.p, (size_t)nr, cnt));
      AMG_HIP(hipStreamSynchronize(s));
      std::vector<long long> ooff(nr + 1, 0);
      for (int q = 0; q < nr; q++) ooff[q + 1] = ooff[q] + cnt[q];
      AMG_HIP(hipMemcpyAsync(d_ooff, ooff.data(), (nr + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
      spgemm_pack_k<<<nr, 64, 0, s>>>(d_hoff, d_hcol, d_hval, d_ooff, nr, d_ocol, d_oval);
      // append the batch to C (grown by doubling, device to device)
      if (used + ooff[nr] > c_cap) {
         const long long cap = std::max(used + ooff[nr], 2 * c_cap);
         DBuf<int> nc;
         DBuf<double> nv;
         AMG_TRY(nc.alloc((size_t)cap));
         if (nv.alloc((size_t)cap) != AMG_OK) return amg_set_error(AMG_ERR_OOM, "spgemm_dev: %lld entries", cap);
         if (used) {
            AMG_HIP(hipMemcpyAsync(nc, c_col, used * sizeof(int), hipMemcpyDeviceToDevice, s));
            AMG_HIP(hipMemcpyAsync(nv, c_val, used * sizeof(double), hipMemcpyDeviceToDevice, s));
         }
         AMG_HIP(hipStreamSynchronize(s));
         c_col = std::move(nc);
         c_val = std::move(nv);
         c_cap = cap;
      }
      if (ooff[nr]) {
         AMG_HIP(hipMemcpyAsync(c_col.p + used, d_ocol, ooff[nr] * sizeof(int), hipMemcpyDeviceToDevice, s));
         AMG_HIP(hipMemcpyAsync(c_val.p + used, d_oval, ooff[nr] * sizeof(double), hipMemcpyDeviceToDevice, s));
      }
      AMG_HIP(hipStreamSynchronize(s));
      AMG_TRY(scan_counts(cnt.data(), nr, &crp[r0]));
      used += ooff[nr];
   }
   if (!c_col.p) {
      AMG_TRY(c_col.alloc(0));
      AMG_TRY(c_val.alloc(0));
   }
   AMG_TRY(upload(s, crp.data(), crp.size(), C.rp));
   AMG_HIP(hipStreamSynchronize(s)); // crp leaves scope
   C.n = A.n, C.m = B.m, C.nnz = used;
   C.cj = std::move(c_col);
   C.v = std::move(c_val);
   return AMG_OK;
}

extern "C" int amg_set_spgemm_scratch(long long slots)
{
   AMG_ARG(slots >= 0, "amg_set_spgemm_scratch: %lld slots", slots);
   g_budget.store(slots ? slots : SPGEMM_BUDGET);
   return AMG_OK;
}

// C = A B on device `device` (bit-identical to the host Gustavson spgemm)
int amg_spgemm_device(int device, const HCsr &A, const HCsr &B, HCsr &C)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dA, dB, dC;
   AMG_TRY(upload_csr(ss.s, view(A), true, dA));
   AMG_TRY(upload_csr(ss.s, view(B), true, dB));
   AMG_TRY(spgemm_dev(ss.s, dA, dB, dC));
   AMG_TRY(download_csr(ss.s, dC, true, C));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

// A_c = R (A P) on device `device`: A, P, R uploaded once, A P kept on the
// device between the two products, only A_c downloaded (bit-identical to the
// host's two Gustavson products)
int amg_rap_device(int device, const HCsr &A, const HCsr &P, const HCsr &R, HCsr &Ac)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dA, dP, dR, dAP, dAc;
   AMG_TRY(upload_csr(ss.s, view(A), true, dA));
   AMG_TRY(upload_csr(ss.s, view(P), true, dP));
   AMG_TRY(spgemm_dev(ss.s, dA, dP, dAP));
   // A is not needed any more: give its memory back before the second product
   AMG_HIP(hipStreamSynchronize(ss.s));
   dA.cj.release();
   dA.v.release();
   AMG_TRY(upload_csr(ss.s, view(R), true, dR));
   AMG_TRY(spgemm_dev(ss.s, dR, dAP, dAc));
   AMG_TRY(download_csr(ss.s, dAc, true, Ac));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

namespace {

// SmoothTransfer's Jacobi factors on A's pattern (A diagonal first), one
// wavefront per row: g = I - w D^-1 A (first entry 1 - w, else (-w a_ij) / a_ii)
// and gt, its transpose's values (else (-w a_ij) / a_jj)
__global__ __launch_bounds__(256) void smooth_factor_k(const int *__restrict__ arp, const int *__restrict__ acj,
                                                       const double *__restrict__ av, int n, double w,
                                                       double *__restrict__ g, double *__restrict__ gt)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = arp[r], e = arp[r + 1];
      if (b == e) continue;
      const double d = av[b];
      for (int k = b + lane; k < e; k += 64) {
         if (k == b) {
            g[k] = gt[k] = 1.0 - w;
         } else {
            g[k] = -w * av[k] / d;
            gt[k] = -w * av[k] / av[arp[acj[k]]];
         }
      }
   }
}

} // namespace

// SmoothTransfer (Jacobi) of one level on device `device`: P~ = G P and, with
// the add_* options off, R~ = P^T GT by spgemm_dev (bit-identical to the host
// products); with one of them on, P~ is truncated on the device before it is
// downloaded and R~ is left to the caller (the transpose of the truncated P~).
// R is P^T.
int amg_smooth_transfer_device(int device, const HCsr &A, const HCsr &P, const HCsr &R, double w, int add_max,
                               double add_tf, HCsr &Ps, HCsr &Rs)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr G, dP, dR, dPs, dT, dRs; // G: A, then A's pattern with the values g, then gt
   DBuf<double> d_g, d_gt;
   AMG_TRY(upload_csr(ss.s, view(A), true, G));
   AMG_TRY(upload_csr(ss.s, view(P), true, dP));
   AMG_TRY(d_g.alloc((size_t)G.nnz));
   AMG_TRY(d_gt.alloc((size_t)G.nnz));
   smooth_factor_k<<<std::min((A.n + 3) / 4, 8192), 256, 0, ss.s>>>(G.rp, G.cj, G.v, A.n, w, d_g, d_gt);
   AMG_HIP(hipGetLastError());
   std::swap(G.v, d_g);
   AMG_TRY(spgemm_dev(ss.s, G, dP, dPs));
   if (add_max > 0 || add_tf > 0.0) {
      AMG_TRY(trunc_dev(ss.s, dPs, add_tf, add_max, dT));
      AMG_TRY(download_csr(ss.s, dT, true, Ps));
   } else {
      AMG_TRY(download_csr(ss.s, dPs, true, Ps));
      AMG_TRY(upload_csr(ss.s, view(R), true, dR));
      std::swap(G.v, d_gt);
      AMG_TRY(spgemm_dev(ss.s, dR, G, dRs));
      AMG_TRY(download_csr(ss.s, dRs, true, Rs));
   }
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}
