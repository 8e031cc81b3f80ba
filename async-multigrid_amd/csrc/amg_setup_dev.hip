// amg_setup_dev.hip -- the classical setup's strength, pattern / valued
// transpose, PMIS and interpolation on the GPU, and the level loop that keeps a
// hierarchy resident on the device while it is built (amg_classical_opts.
// setup_on_device).  Each phase restates its host function in amg_classical.cpp
// (strength, transpose_pattern / transpose, coarsen_pmis, interpolation) and is
// bit-identical to it: every floating-point sum is formed in the host's order,
// min / max and integer counts are the only reductions that run in any order,
// integer atomics count but never decide a stored order, and there are no
// floating-point atomics.
//
//   strength   one wavefront per row: the diagonal (the row's last entry of
//              column i, as the host loop leaves it), the row scale (min / max:
//              exact in any order) and, with max_row_sum < 1, the row sum as a
//              serial chain of wave-uniform broadcasts; one keep flag per entry,
//              rows packed in storage order (amg_trunc.hip's flag / pack scheme)
//   transpose  integer atomics count the columns and hand out slots; each slot
//              holds the key (source row, position in it), and an entry's place
//              in its result row is its key's rank there, so rows hold ascending
//              source rows in storage order -- the host's counting sort
//   PMIS       measure |S^T_i| + the splitmix64 draw; a round is two kernels:
//              select reads the C/F state of the round's start and writes the
//              new C points to a flag array of its own, apply makes them C and
//              every undecided point with a new C point in its S row F (the
//              host's loop over S^T rows, pulled instead of pushed: no atomics
//              on the marker).  The host reads two counters per round.
//   interp     one wavefront (one workgroup) per F row.  C^_i is gathered into
//              the row's scratch, rank-sorted and made unique; lane p % 64 owns
//              target p (the first 64 in registers, the rest in scratch only
//              their owner touches).  The walk over the row's entries q, and
//              inside a strong F neighbour's row over r, is wave-uniform and in
//              storage order, so num[j], d_k and atil are the host's chains.
//              Scratch per row is its upper bound |S_i| + sum of |S_k| over the
//              strong F neighbours; rows run in batches under a slot budget
//              (amg_set_setup_scratch), a row larger than the budget alone.
// The two rank sorts (a transposed row's keys, a row's C^_i candidates) compare
// every entry with the whole row, 64 entries at a time: exact and without
// atomics, quadratic in a row's length, which is tens of entries on the setup's
// operators and a few hundred at a hub.
// Offsets are 32-bit, as everywhere in the classical setup.  The phases take and
// return device CSRs (amg_csr.h's DCsr, with the buffers, uploads, count scan and
// row batching they share with amg_spgemm.hip and amg_trunc.hip).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "amg_csr.h"

namespace {

constexpr int WBLOCK = 256; // 4 wavefronts: 4 rows in flight per workgroup

// scratch budget of one batch of interp_dev, in slots of 16 bytes (amg_set_setup_scratch)
constexpr long long SETUP_BUDGET = 1LL << 27;
std::atomic<long long> g_setup_budget{SETUP_BUDGET};

int wave_grid(int n) { return (int)std::max<long long>(1, std::min<long long>(((long long)n + 3) / 4, 8192)); }

// ---- strength -------------------------------------------------------------------
__global__ __launch_bounds__(WBLOCK) void strength_flag_k(const int *__restrict__ rp, const int *__restrict__ cj,
                                                          const double *__restrict__ v, int n, double theta,
                                                          double max_row_sum, int nfun, unsigned char *__restrict__ keep,
                                                          int *__restrict__ cnt)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = rp[r], len = rp[r + 1] - b;
      // the diagonal: the host loop keeps the last entry of column r
      int kd = -1;
      for (int i = lane; i < len; i += 64)
         if (cj[b + i] == r) kd = i;
      for (int o = 32; o > 0; o >>= 1) kd = max(kd, __shfl_xor(kd, o, 64));
      const double diag = kd >= 0 ? v[b + kd] : 0.0;
      const bool neg = diag < 0;
      double sc = 0.0;
      for (int i = lane; i < len; i += 64) {
         const int j = cj[b + i];
         const double x = v[b + i];
         if (j == r || j % nfun != r % nfun) continue;
         sc = neg ? (sc < x ? x : sc) : (x < sc ? x : sc);
      }
      for (int o = 32; o > 0; o >>= 1) {
         const double y = __shfl_xor(sc, o, 64);
         sc = neg ? (sc < y ? y : sc) : (y < sc ? y : sc);
      }
      bool all_weak = false;
      if (max_row_sum < 1.0) {
         double sum = 0.0; // storage order: every lane forms the same chain
         for (int c0 = 0; c0 < len; c0 += 64) {
            const int i = c0 + lane;
            const double x = i < len ? v[b + i] : 0.0;
            const int cl = min(64, len - c0);
            for (int t = 0; t < cl; t++) sum += __shfl(x, t, 64);
         }
         all_weak = fabs(sum) > fabs(diag) * max_row_sum;
      }
      const double thr = theta * sc;
      int m = 0;
      for (int c0 = 0; c0 < len; c0 += 64) {
         const int i = c0 + lane;
         bool strong = false;
         if (i < len && !all_weak) {
            const int j = cj[b + i];
            const double x = v[b + i];
            if (j != r && j % nfun == r % nfun) strong = neg ? x > thr : x < thr;
         }
         if (i < len) keep[b + i] = strong ? 1 : 0;
         m += __popcll(__ballot(strong));
      }
      if (lane == 0) cnt[r] = m;
   }
}

// flagged columns of row r to orp[r].., in storage order
__global__ __launch_bounds__(WBLOCK) void pack_cols_k(const int *__restrict__ rp, const int *__restrict__ cj, int n,
                                                      const unsigned char *__restrict__ keep,
                                                      const int *__restrict__ orp, int *__restrict__ ocj)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = rp[r], len = rp[r + 1] - b;
      int o = orp[r];
      for (int c0 = 0; c0 < len; c0 += 64) {
         const int i = c0 + lane;
         const bool kp = i < len && keep[b + i] != 0;
         const unsigned long long km = __ballot(kp);
         if (kp) ocj[o + __popcll(km & ((1ull << lane) - 1ull))] = cj[b + i];
         o += __popcll(km);
      }
   }
}

int strength_dev(hipStream_t s, const DCsr &A, double theta, double max_row_sum, int nfun, DCsr &S)
{
   DBuf<unsigned char> d_keep;
   DBuf<int> d_cnt;
   std::vector<int> rp;
   S = DCsr();
   S.n = S.m = A.n;
   AMG_TRY(d_keep.alloc((size_t)A.nnz));
   AMG_TRY(d_cnt.alloc((size_t)A.n));
   strength_flag_k<<<wave_grid(A.n), WBLOCK, 0, s>>>(A.rp, A.cj, A.v, A.n, theta, max_row_sum, nfun, d_keep, d_cnt);
   AMG_HIP(hipGetLastError());
   AMG_TRY(rowptr_of_counts(s, d_cnt, A.n, rp, S.rp));
   S.nnz = rp[A.n];
   AMG_TRY(S.cj.alloc((size_t)S.nnz));
   pack_cols_k<<<wave_grid(A.n), WBLOCK, 0, s>>>(A.rp, A.cj, A.n, d_keep, S.rp, S.cj);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipStreamSynchronize(s)); // rp leaves scope
   return AMG_OK;
}

// ---- transpose ------------------------------------------------------------------
__global__ void tr_count_k(const int *__restrict__ cj, long long nnz, int *__restrict__ cnt)
{
   const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
   if (k < nnz) atomicAdd(&cnt[cj[k]], 1);
}

// slots of a result row are handed out in any order; what is stored is the key
__global__ __launch_bounds__(WBLOCK) void tr_fill_k(const int *__restrict__ rp, const int *__restrict__ cj, int n,
                                                    int *__restrict__ pos, long long *__restrict__ key)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n; r += gridDim.x * wpb) {
      const int b = rp[r], len = rp[r + 1] - b;
      for (int i = lane; i < len; i += 64) {
         const int p = atomicAdd(&pos[cj[b + i]], 1);
         key[p] = ((long long)r << 32) | (long long)i;
      }
   }
}

// result row c: every entry goes to the rank of its key (keys are distinct)
__global__ __launch_bounds__(WBLOCK) void tr_place_k(const int *__restrict__ trp, const long long *__restrict__ key,
                                                     int m, const int *__restrict__ rp, const double *__restrict__ v,
                                                     int *__restrict__ tcj, double *__restrict__ tv)
{
   const int lane = threadIdx.x & 63;
   const int wpb = blockDim.x >> 6;
   for (int c = blockIdx.x * wpb + (threadIdx.x >> 6); c < m; c += gridDim.x * wpb) {
      const int b = trp[c], len = trp[c + 1] - b;
      for (int e = lane; e < len; e += 64) {
         const long long k = key[b + e];
         int rank = 0;
         for (int t = 0; t < len; t++) rank += key[b + t] < k ? 1 : 0;
         const int r = (int)(k >> 32);
         tcj[b + rank] = r;
         if (tv) tv[b + rank] = v[rp[r] + (int)(k & 0xffffffffLL)];
      }
   }
}

int transpose_dev(hipStream_t s, const DCsr &A, bool values, DCsr &T)
{
   DBuf<int> d_cnt, d_pos;
   DBuf<long long> d_key;
   std::vector<int> trp;
   T = DCsr();
   T.n = A.m, T.m = A.n;
   AMG_TRY(d_cnt.alloc((size_t)A.m));
   AMG_HIP(hipMemsetAsync(d_cnt, 0, std::max<size_t>(A.m, 1) * sizeof(int), s));
   if (A.nnz) tr_count_k<<<(unsigned)((A.nnz + 255) / 256), 256, 0, s>>>(A.cj, A.nnz, d_cnt);
   AMG_HIP(hipGetLastError());
   AMG_TRY(rowptr_of_counts(s, d_cnt, A.m, trp, T.rp));
   T.nnz = trp[A.m];
   AMG_TRY(d_pos.alloc((size_t)A.m));
   if (A.m) AMG_HIP(hipMemcpyAsync(d_pos, T.rp, (size_t)A.m * sizeof(int), hipMemcpyDeviceToDevice, s));
   AMG_TRY(d_key.alloc((size_t)A.nnz));
   AMG_TRY(T.cj.alloc((size_t)A.nnz));
   if (values) AMG_TRY(T.v.alloc((size_t)A.nnz));
   if (A.n) tr_fill_k<<<wave_grid(A.n), WBLOCK, 0, s>>>(A.rp, A.cj, A.n, d_pos, d_key);
   AMG_HIP(hipGetLastError());
   if (A.m) tr_place_k<<<wave_grid(A.m), WBLOCK, 0, s>>>(T.rp, d_key, A.m, A.rp, A.v, T.cj, T.v);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipStreamSynchronize(s)); // trp leaves scope
   return AMG_OK;
}

// ---- PMIS -----------------------------------------------------------------------
// ctr[1] += the points left undecided
__global__ void pmis_init_k(const int *__restrict__ strp, int n, unsigned long long seed, double *__restrict__ meas,
                            int *__restrict__ cf, int *__restrict__ ctr)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   bool und = false;
   if (i < n) {
      const double r =
         (double)(splitmix64(seed ^ (unsigned long long)i * 0x2545f4914f6cdd1dULL) >> 11) * 0x1.0p-53;
      const double ms = (strp[i + 1] - strp[i]) + r;
      meas[i] = ms;
      und = !(ms < 1.0);
      cf[i] = und ? CF_U : CF_F;
   }
   const int c = __popcll(__ballot(und));
   if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctr[1], c);
}

// newc[i] = 1 for every undecided point that beats all undecided neighbours in
// S and S^T; cf is only read: the state of the round's start.  ctr[0] += new C
__global__ void pmis_select_k(const int *__restrict__ srp, const int *__restrict__ scj,
                              const int *__restrict__ strp, const int *__restrict__ stcj, int n,
                              const int *__restrict__ cf, const double *__restrict__ meas,
                              unsigned char *__restrict__ newc, int *__restrict__ ctr)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   bool best = false;
   if (i < n) {
      best = cf[i] == CF_U;
      const double mi = meas[i];
      for (int a = srp[i]; best && a < srp[i + 1]; a++) {
         const int j = scj[a];
         if (cf[j] == CF_U && meas[j] >= mi) best = false;
      }
      for (int a = strp[i]; best && a < strp[i + 1]; a++) {
         const int j = stcj[a];
         if (cf[j] == CF_U && meas[j] >= mi) best = false;
      }
      newc[i] = best ? 1 : 0;
   }
   const int c = __popcll(__ballot(best));
   if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctr[0], c);
}

// new C points become C; an undecided point that depends on one becomes F (two
// new C points are never neighbours, so no new C point is made F).  ctr[1] +=
// the points decided
__global__ void pmis_apply_k(const int *__restrict__ srp, const int *__restrict__ scj, int n,
                             const unsigned char *__restrict__ newc, int *__restrict__ cf, int *__restrict__ ctr)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   bool dec = false;
   if (i < n) {
      if (newc[i]) {
         cf[i] = CF_C;
         dec = true;
      } else if (cf[i] == CF_U) {
         for (int a = srp[i]; a < srp[i + 1]; a++)
            if (newc[scj[a]]) {
               cf[i] = CF_F;
               dec = true;
               break;
            }
      }
   }
   const int c = __popcll(__ballot(dec));
   if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctr[1], c);
}

__global__ void pmis_rest_k(int n, int *__restrict__ cf)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n && cf[i] == CF_U) cf[i] = CF_F;
}

// d_cf: n ints, allocated by the caller
int pmis_dev(hipStream_t s, const DCsr &S, const DCsr &ST, unsigned long long seed, int *d_cf, int *rounds_out)
{
   const int n = S.n;
   DBuf<double> d_meas;
   DBuf<unsigned char> d_newc;
   DBuf<int> d_ctr;
   AMG_TRY(d_meas.alloc((size_t)n));
   AMG_TRY(d_newc.alloc((size_t)n));
   AMG_TRY(d_ctr.alloc(2));
   const int grid = (n + 255) / 256;
   int ctr[2] = {0, 0};
   AMG_HIP(hipMemsetAsync(d_ctr, 0, 2 * sizeof(int), s));
   pmis_init_k<<<grid, 256, 0, s>>>(ST.rp, n, seed, d_meas, d_cf, d_ctr);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipMemcpyAsync(ctr, d_ctr, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   long long left = ctr[1];
   int rounds = 0;
   // a round decides at least one point or ends the loop; n + 1 is a hard cap
   for (long long it = 0; left > 0 && it <= n; it++) {
      AMG_HIP(hipMemsetAsync(d_ctr, 0, 2 * sizeof(int), s));
      pmis_select_k<<<grid, 256, 0, s>>>(S.rp, S.cj, ST.rp, ST.cj, n, d_cf, d_meas, d_newc, d_ctr);
      pmis_apply_k<<<grid, 256, 0, s>>>(S.rp, S.cj, n, d_newc, d_cf, d_ctr);
      AMG_HIP(hipGetLastError());
      AMG_HIP(hipMemcpyAsync(ctr, d_ctr, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
      AMG_HIP(hipStreamSynchronize(s));
      if (ctr[0] == 0) break; // the host's `break`: the rest become F
      left -= ctr[1];
      rounds++;
   }
   pmis_rest_k<<<grid, 256, 0, s>>>(n, d_cf);
   AMG_HIP(hipGetLastError());
   AMG_HIP(hipStreamSynchronize(s));
   if (rounds_out) *rounds_out = rounds;
   return AMG_OK;
}

// ---- interpolation --------------------------------------------------------------
// ub[i]: scratch slots of row i -- 0 for a C row, else |S_i| (+ |S_k| over the
// strong F neighbours k for extended+i): every candidate of C^_i has a slot
__global__ void interp_ub_k(const int *__restrict__ srp, const int *__restrict__ scj, const int *__restrict__ cf,
                            int n, int type, long long *__restrict__ ub)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   long long u = 0;
   if (cf[i] != CF_C) {
      u = srp[i + 1] - srp[i];
      if (type == 6)
         for (int a = srp[i]; a < srp[i + 1]; a++) {
            const int k = scj[a];
            if (cf[k] != CF_C) u += srp[k + 1] - srp[k];
         }
   }
   ub[i] = u;
}

// a_kl of the first entry of column `col` in a row (0.0 without one): wave-uniform
__device__ inline double first_match(const int *__restrict__ cj, const double *__restrict__ v, int b, int len, int col,
                                     int lane)
{
   for (int c0 = 0; c0 < len; c0 += 64) {
      const int e = c0 + lane;
      const bool hit = e < len && cj[b + e] == col;
      const double x = e < len ? v[b + e] : 0.0;
      const unsigned long long m = __ballot(hit);
      if (m) return __shfl(x, __ffsll((long long)m) - 1, 64);
   }
   return 0.0;
}

// position of j in the sorted targets t[0..nu) or -1, any j per lane
__device__ inline int target_of(const int *__restrict__ t, int nu, int j)
{
   int lo = 0, hi = nu;
   while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < j)
         lo = mid + 1;
      else
         hi = mid;
   }
   return lo < nu && t[lo] == j ? lo : -1;
}

// the same for a wave-uniform j: the first 64 targets are in the lanes' j0
__device__ inline int target_uniform(const int *__restrict__ t, int nu, int j0, int j)
{
   const unsigned long long m = __ballot(j0 == j);
   if (m) return __ffsll((long long)m) - 1;
   if (nu <= 64) return -1;
   const int p = target_of(t + 64, nu - 64, j);
   return p < 0 ? -1 : p + 64;
}

// num[pos] += x by the lane that owns target pos (no other lane touches it)
__device__ inline void target_add(int pos, double x, int lane, double &n0, double *__restrict__ nm)
{
   if ((pos & 63) == lane) {
      if (pos < 64)
         n0 += x;
      else
         nm[pos] += x;
   }
}

// candidates of one S row (the C points in it) appended to cd[nc..)
__device__ inline int gather_c(const int *__restrict__ scj, int b, int len, const int *__restrict__ cf,
                               int *__restrict__ cd, int nc, int lane)
{
   for (int c0 = 0; c0 < len; c0 += 64) {
      const int e = c0 + lane;
      const int j = e < len ? scj[b + e] : 0;
      const bool isc = e < len && cf[j] == CF_C;
      const unsigned long long m = __ballot(isc);
      if (isc) cd[nc + __popcll(m & ((1ull << lane) - 1ull))] = j;
      nc += __popcll(m);
   }
   return nc;
}

// rows [r0, r0 + nr), one workgroup of one wavefront each; row q's scratch is
// cand / chat / num at hoff[q]..hoff[q + 1].  On return chat / num hold the
// row's cnt[q] entries (coarse column, weight) in column order; C rows only
// set cnt = 1 (the pack kernel writes their injection).
__global__ __launch_bounds__(64) void interp_row_k(const int *__restrict__ arp, const int *__restrict__ acj,
                                                   const double *__restrict__ av, const int *__restrict__ srp,
                                                   const int *__restrict__ scj, const int *__restrict__ cf,
                                                   const int *__restrict__ cidx, int r0, int nr,
                                                   const long long *__restrict__ hoff, int *cand, int *chat,
                                                   double *num, int *__restrict__ cnt, int type, int nfun)
{
   const int q = blockIdx.x;
   if (q >= nr) return;
   const int i = r0 + q, lane = threadIdx.x;
   if (cf[i] == CF_C) {
      if (lane == 0) cnt[q] = 1;
      return;
   }
   const long long base = hoff[q];
   int *cd = cand + base, *ch = chat + base;
   double *nm = num + base;
   const int sb = srp[i], sl = srp[i + 1] - sb;
   // C^_i with repeats, in cd
   int nc = gather_c(scj, sb, sl, cf, cd, 0, lane);
   if (type == 6)
      for (int a = 0; a < sl; a++) {
         const int k = scj[sb + a];
         if (cf[k] == CF_C) continue;
         nc = gather_c(scj, srp[k], srp[k + 1] - srp[k], cf, cd, nc, lane);
      }
   __syncthreads();
   // sorted (rank of (value, position)) into ch
   for (int e = lane; e < nc; e += 64) {
      const int x = cd[e];
      int rank = 0;
      for (int t = 0; t < nc; t++) {
         const int u = cd[t];
         rank += (u < x || (u == x && t < e)) ? 1 : 0;
      }
      ch[rank] = x;
   }
   __syncthreads();
   // unique, back into cd: cd[0..nu) = C^_i ascending
   int nu = 0;
   for (int c0 = 0; c0 < nc; c0 += 64) {
      const int p = c0 + lane;
      const bool f = p < nc && (p == 0 || ch[p] != ch[p - 1]);
      const unsigned long long m = __ballot(f);
      if (f) cd[nu + __popcll(m & ((1ull << lane) - 1ull))] = ch[p];
      nu += __popcll(m);
   }
   __syncthreads();
   const int j0 = lane < nu ? cd[lane] : -1;
   double n0 = 0.0;
   for (int p = lane + 64; p < nu; p += 64) nm[p] = 0.0;
   const int ab = arp[i], al = arp[i + 1] - ab;
   const double aii = first_match(acj, av, ab, al, i, lane);
   bool emit;
   double scale_num = 0.0, scale_den = 1.0; // weight = scale_num * num / scale_den
   if (type == 3) {
      double sum_all = 0.0, sum_c = 0.0;
      for (int c0 = 0; c0 < al; c0 += 64) {
         const int e = c0 + lane;
         const int j = e < al ? acj[ab + e] : i;
         const double aij = e < al ? av[ab + e] : 0.0;
         unsigned long long live = __ballot(e < al && j != i && j % nfun == i % nfun);
         while (live) {
            const int t = __ffsll((long long)live) - 1;
            live &= live - 1;
            const int jt = __shfl(j, t, 64);
            const double at = __shfl(aij, t, 64);
            sum_all += at;
            const int pos = target_uniform(cd, nu, j0, jt);
            if (pos >= 0) {
               target_add(pos, at, lane, n0, nm);
               sum_c += at;
            }
         }
      }
      emit = sum_c != 0.0 && aii != 0.0;
      if (emit) {
         scale_num = -(sum_all / sum_c);
         scale_den = aii;
      }
   } else {
      double atil = aii;
      for (int c0 = 0; c0 < al; c0 += 64) {
         const int e = c0 + lane;
         const int j = e < al ? acj[ab + e] : i;
         const double aij = e < al ? av[ab + e] : 0.0;
         const bool lv = e < al && j != i && j % nfun == i % nfun;
         // strong F neighbour: j in S_i (as a set) and F
         bool sf = false;
         if (lv && cf[j] != CF_C)
            for (int a = 0; a < sl; a++) sf |= scj[sb + a] == j;
         const unsigned long long sfm = __ballot(sf);
         unsigned long long live = __ballot(lv);
         while (live) {
            const int t = __ffsll((long long)live) - 1;
            live &= live - 1;
            const int jt = __shfl(j, t, 64);
            const double at = __shfl(aij, t, 64);
            const int pos = target_uniform(cd, nu, j0, jt);
            if (pos >= 0) { // j in C^_i: interpolation target
               target_add(pos, at, lane, n0, nm);
               continue;
            }
            if (!((sfm >> t) & 1ull)) { // weak neighbour outside C^_i
               atil += at;
               continue;
            }
            // strong F neighbour k: distribute over C^_i u {i}
            const int k = jt;
            const int kb = arp[k], kl = arp[k + 1] - kb;
            const double akk = first_match(acj, av, kb, kl, k, lane);
            double dk = 0.0;
            for (int d0 = 0; d0 < kl; d0 += 64) {
               const int e2 = d0 + lane;
               const int l = e2 < kl ? acj[kb + e2] : -1;
               const double akl = e2 < kl ? av[kb + e2] : 0.0;
               const bool mem = e2 < kl && akl * akk < 0.0 && (l == i || target_of(cd, nu, l) >= 0);
               unsigned long long mm = __ballot(mem);
               while (mm) {
                  const int u = __ffsll((long long)mm) - 1;
                  mm &= mm - 1;
                  dk += __shfl(akl, u, 64);
               }
            }
            if (dk == 0.0) {
               atil += at;
               continue;
            }
            for (int d0 = 0; d0 < kl; d0 += 64) {
               const int e2 = d0 + lane;
               const int l = e2 < kl ? acj[kb + e2] : -1;
               const double akl = e2 < kl ? av[kb + e2] : 0.0;
               int pl = -2; // -1: l == i, >= 0: target, -2: neither
               if (e2 < kl && !(akl * akk >= 0.0)) {
                  if (l == i) {
                     pl = -1;
                  } else {
                     const int p = target_of(cd, nu, l);
                     pl = p >= 0 ? p : -2;
                  }
               }
               const double w = at * akl / dk;
               unsigned long long mm = __ballot(pl != -2);
               while (mm) {
                  const int u = __ffsll((long long)mm) - 1;
                  mm &= mm - 1;
                  const int pu = __shfl(pl, u, 64);
                  const double wu = __shfl(w, u, 64);
                  if (pu == -1)
                     atil += wu;
                  else
                     target_add(pu, wu, lane, n0, nm);
               }
            }
         }
      }
      emit = atil != 0.0;
      if (emit) {
         scale_num = -1.0;
         scale_den = atil;
      }
   }
   if (emit) {
      // direct: -alpha * num / a_ii; extended+i: -num / atil (-1.0 * x is -x exactly)
      if (lane < nu) {
         ch[lane] = cidx[j0];
         nm[lane] = scale_num * n0 / scale_den;
      }
      for (int p = lane + 64; p < nu; p += 64) {
         ch[p] = cidx[cd[p]];
         nm[p] = scale_num * nm[p] / scale_den;
      }
   }
   if (lane == 0) cnt[q] = emit ? nu : 0;
}

__global__ __launch_bounds__(64) void interp_pack_k(const int *__restrict__ cf, const int *__restrict__ cidx, int r0,
                                                    int nr, const long long *__restrict__ hoff,
                                                    const int *__restrict__ chat, const double *__restrict__ num,
                                                    const long long *__restrict__ ooff, int *__restrict__ ocj,
                                                    double *__restrict__ ov)
{
   const int q = blockIdx.x;
   if (q >= nr) return;
   const int i = r0 + q;
   const long long o = ooff[q], m = ooff[q + 1] - o;
   if (cf[i] == CF_C) {
      if (threadIdx.x == 0) {
         ocj[o] = cidx[i];
         ov[o] = 1.0;
      }
      return;
   }
   const long long b = hoff[q];
   for (long long p = threadIdx.x; p < m; p += 64) {
      ocj[o + p] = chat[b + p];
      ov[o + p] = num[b + p];
   }
}

// cf: the marker on the host as well (its scan is cidx)
int interp_dev(hipStream_t s, const DCsr &A, const DCsr &S, const int *d_cf, const std::vector<int> &cf, int type,
               int nfun, DCsr &P)
{
   const int n = A.n;
   DBuf<int> d_cidx, d_cand, d_chat, d_cnt;
   DBuf<long long> d_ub, d_hoff, d_ooff;
   DBuf<double> d_num;
   struct Part {
      DBuf<int> cj;
      DBuf<double> v;
      long long nz = 0;
   };
   std::vector<Part> parts;
   P = DCsr();
   std::vector<int> cidx(n, -1);
   int nc = 0;
   for (int i = 0; i < n; i++)
      if (cf[i] == CF_C) cidx[i] = nc++;
   P.n = n, P.m = nc;
   AMG_TRY(upload(s, cidx.data(), (size_t)n, d_cidx));
   AMG_TRY(d_ub.alloc((size_t)n));
   interp_ub_k<<<(n + 255) / 256, 256, 0, s>>>(S.rp, S.cj, d_cf, n, type, d_ub);
   AMG_HIP(hipGetLastError());
   std::vector<long long> ub;
   AMG_TRY(download(s, d_ub.p, (size_t)n, ub));
   AMG_HIP(hipStreamSynchronize(s));
   const std::vector<int> cut = batch_bounds(ub, g_setup_budget.load());
   long long maxb = 1;
   int maxr = 1;
   for (size_t b = 0; b + 1 < cut.size(); b++) {
      maxb = std::max(maxb, std::accumulate(ub.begin() + cut[b], ub.begin() + cut[b + 1], 0LL));
      maxr = std::max(maxr, cut[b + 1] - cut[b]);
   }
   AMG_TRY(d_cand.alloc((size_t)maxb));
   AMG_TRY(d_chat.alloc((size_t)maxb));
   AMG_TRY(d_num.alloc((size_t)maxb));
   AMG_TRY(d_hoff.alloc((size_t)maxr + 1));
   AMG_TRY(d_ooff.alloc((size_t)maxr + 1));
   AMG_TRY(d_cnt.alloc((size_t)maxr));
   std::vector<int> prp((size_t)n + 1, 0);
   long long used = 0;
   for (size_t b = 0; b + 1 < cut.size(); b++) {
      const int r0 = cut[b], nr = cut[b + 1] - r0;
      std::vector<long long> hoff((size_t)nr + 1, 0), ooff((size_t)nr + 1, 0);
      for (int q = 0; q < nr; q++) hoff[q + 1] = hoff[q] + ub[r0 + q];
      AMG_HIP(hipMemcpyAsync(d_hoff, hoff.data(), ((size_t)nr + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
      interp_row_k<<<nr, 64, 0, s>>>(A.rp, A.cj, A.v, S.rp, S.cj, d_cf, d_cidx, r0, nr, d_hoff, d_cand, d_chat, d_num,
                                     d_cnt, type, nfun);
      AMG_HIP(hipGetLastError());
      std::vector<int> cnt;
      AMG_TRY(download(s, d_cnt.p, (size_t)nr, cnt));
      AMG_HIP(hipStreamSynchronize(s));
      for (int q = 0; q < nr; q++) ooff[q + 1] = ooff[q] + cnt[q];
      if (used + ooff[nr] > INT_MAX)
         return amg_set_error(AMG_ERR_ARG, "classical setup on the device: P has more than 2^31 - 1 entries");
      parts.emplace_back();
      Part &pt = parts.back();
      pt.nz = ooff[nr];
      AMG_TRY(pt.cj.alloc((size_t)pt.nz));
      AMG_TRY(pt.v.alloc((size_t)pt.nz));
      AMG_HIP(hipMemcpyAsync(d_ooff, ooff.data(), ((size_t)nr + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
      interp_pack_k<<<nr, 64, 0, s>>>(d_cf, d_cidx, r0, nr, d_hoff, d_chat, d_num, d_ooff, pt.cj, pt.v);
      AMG_HIP(hipGetLastError());
      AMG_HIP(hipStreamSynchronize(s)); // hoff / ooff leave scope, the scratch is reused
      AMG_TRY(scan_counts(cnt.data(), nr, &prp[r0]));
      used += ooff[nr];
   }
   P.nnz = used;
   AMG_TRY(upload(s, prp.data(), (size_t)n + 1, P.rp));
   if (parts.size() == 1) { // one batch: its output is P
      P.cj = std::move(parts[0].cj);
      P.v = std::move(parts[0].v);
   } else {
      AMG_TRY(P.cj.alloc((size_t)used));
      AMG_TRY(P.v.alloc((size_t)used));
      long long o = 0;
      for (const Part &pt : parts) {
         if (pt.nz) {
            AMG_HIP(hipMemcpyAsync(P.cj.p + o, pt.cj, (size_t)pt.nz * sizeof(int), hipMemcpyDeviceToDevice, s));
            AMG_HIP(hipMemcpyAsync(P.v.p + o, pt.v, (size_t)pt.nz * sizeof(double), hipMemcpyDeviceToDevice, s));
         }
         o += pt.nz;
      }
   }
   AMG_HIP(hipStreamSynchronize(s)); // prp and cidx leave scope
   return AMG_OK;
}

} // namespace

extern "C" int amg_set_setup_scratch(long long slots)
{
   AMG_ARG(slots >= 0, "amg_set_setup_scratch: %lld slots", slots);
   g_setup_budget.store(slots ? slots : SETUP_BUDGET);
   return AMG_OK;
}

// ---- host CSR in and out --------------------------------------------------------
int amg_strength_device(int device, const HCsrView &A, double theta, double max_row_sum, int nfun, HCsr &S)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dA, dS;
   AMG_TRY(upload_csr(ss.s, A, true, dA));
   AMG_TRY(strength_dev(ss.s, dA, theta, max_row_sum, nfun, dS));
   AMG_TRY(download_csr(ss.s, dS, false, S));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

int amg_transpose_device(int device, const HCsrView &A, HCsr &T)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dA, dT;
   AMG_TRY(upload_csr(ss.s, A, A.v != nullptr, dA));
   AMG_TRY(transpose_dev(ss.s, dA, A.v != nullptr, dT));
   AMG_TRY(download_csr(ss.s, dT, A.v != nullptr, T));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

int amg_pmis_device(int device, const HCsrView &S, unsigned long long seed, int *cf, int *rounds)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dS, dST;
   DBuf<int> d_cf;
   AMG_TRY(upload_csr(ss.s, S, false, dS));
   AMG_TRY(transpose_dev(ss.s, dS, false, dST));
   AMG_TRY(d_cf.alloc((size_t)S.n));
   AMG_TRY(pmis_dev(ss.s, dS, dST, seed, d_cf, rounds));
   AMG_HIP(hipMemcpyAsync(cf, d_cf, (size_t)S.n * sizeof(int), hipMemcpyDeviceToHost, ss.s));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

int amg_interp_device(int device, const HCsrView &A, const HCsrView &S, const int *cf, int type, int nfun, HCsr &P)
{
   Session ss;
   AMG_TRY(ss.open(device));
   DCsr dA, dS, dP;
   DBuf<int> d_cf;
   AMG_TRY(upload_csr(ss.s, A, true, dA));
   AMG_TRY(upload_csr(ss.s, S, false, dS));
   AMG_TRY(upload(ss.s, cf, (size_t)A.n, d_cf));
   const std::vector<int> hcf(cf, cf + A.n);
   AMG_TRY(interp_dev(ss.s, dA, dS, d_cf, hcf, type, nfun, dP));
   AMG_TRY(download_csr(ss.s, dP, true, P));
   AMG_HIP(hipStreamSynchronize(ss.s));
   return AMG_OK;
}

// The level loop of amg_classical_setup with the hierarchy resident on the
// device: A_0 is uploaded once, every phase of a level runs on device arrays,
// A_{l+1} stays there as the next level's input, and a level's cf, P, R and
// A_{l+1} are what is downloaded.  HMIS coarsens on the host (hmis: S in, cf
// out).  Stall and stop rules as on the host.
int amg_classical_setup_device(const amg_classical_opts *o, const HCsr &A0, const amg_hmis_fn &hmis,
                               std::vector<amg_setup_dev_level> &levels)
{
   Session ss;
   AMG_TRY(ss.open(o->device));
   hipStream_t s = ss.s;
   DCsr A, S, ST, P, R, AP, Ac;
   DBuf<int> d_cf;
   const bool tm = std::getenv("AMG_CLASSICAL_TIMING") != nullptr;
   auto now = [&] {
      hipStreamSynchronize(s);
      return std::chrono::steady_clock::now();
   };
   const uint64_t seed = o->coarsen_type == AMG_COARSEN_PMIS ? o->seed + 0x9e37ULL : o->seed;
   AMG_TRY(upload_csr(s, view(A0), true, A));
   for (int l = 0; l + 1 < o->max_levels; l++) {
      if (A.n <= o->max_coarse_size) break;
      const int nfun = A.n % o->num_functions == 0 ? o->num_functions : 1;
      auto t0 = now();
      AMG_TRY(strength_dev(s, A, o->strong_threshold, o->max_row_sum, nfun, S));
      amg_setup_dev_level L;
      AMG_TRY(d_cf.alloc((size_t)A.n));
      std::chrono::steady_clock::time_point t1;
      int rounds = 0;
      if (o->coarsen_type == AMG_COARSEN_HMIS) {
         t1 = now();
         HCsr Sh;
         AMG_TRY(download_csr(s, S, false, Sh));
         AMG_HIP(hipStreamSynchronize(s));
         hmis(Sh, L.cf);
         AMG_HIP(hipMemcpyAsync(d_cf, L.cf.data(), (size_t)A.n * sizeof(int), hipMemcpyHostToDevice, s));
      } else {
         AMG_TRY(transpose_dev(s, S, false, ST));
         t1 = now();
         AMG_TRY(pmis_dev(s, S, ST, seed + (uint64_t)l * 7919ULL, d_cf, &rounds));
         AMG_TRY(download(s, d_cf.p, (size_t)A.n, L.cf));
         ST.release();
      }
      auto t2 = now();
      int nc = 0;
      for (int c : L.cf) nc += c == CF_C;
      if (nc == 0 || nc == A.n) break; // coarsening stalled
      AMG_TRY(interp_dev(s, A, S, d_cf, L.cf, o->interp_type, nfun, P));
      S.release();
      d_cf.release();
      auto t3 = now();
      if (o->P_max_elmts > 0 || o->trunc_factor > 0.0) {
         DCsr T;
         AMG_TRY(trunc_dev(s, P, o->trunc_factor, o->P_max_elmts, T));
         P = std::move(T);
      }
      AMG_TRY(transpose_dev(s, P, true, R));
      AMG_TRY(spgemm_dev(s, A, P, AP));
      A.release(); // A_l is on the host already: make room for the second product
      AMG_TRY(spgemm_dev(s, R, AP, Ac));
      AP.release();
      AMG_TRY(download_csr(s, P, true, L.P));
      AMG_HIP(hipStreamSynchronize(s));
      AMG_TRY(download_csr(s, R, true, L.R));
      AMG_HIP(hipStreamSynchronize(s));
      AMG_TRY(download_csr(s, Ac, true, L.Ac));
      AMG_HIP(hipStreamSynchronize(s));
      P.release(), R.release();
      A = std::move(Ac);
      auto t4 = now();
      if (tm) {
         auto d = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
         std::fprintf(stderr,
                      "[classical] level %d n=%d: strength %.3fs coarsen %.3fs interp %.3fs RAP %.3fs "
                      "(device, %d PMIS rounds)\n",
                      l, L.P.n, d(t0, t1), d(t1, t2), d(t2, t3), d(t3, t4), rounds);
      }
      levels.push_back(std::move(L));
   }
   return AMG_OK;
}
