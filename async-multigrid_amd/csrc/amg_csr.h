// amg_csr.h -- what the classical setup's files share (amg_classical.cpp,
// amg_spgemm.hip, amg_trunc.hip, amg_setup_dev.hip; DBuf also amg_format.hip; not part of the C-ABI): the
// host and device CSR types, owning device buffers, the per-call stream, upload /
// download, the count scan, the row batching, and the entry points the files
// call across each other.  Device memory is owned: a DBuf or DCsr frees in its
// destructor, so a function that returns early on an error leaks nothing.
#pragma once

#include <algorithm>
#include <climits>
#include <vector>

#include "amg_internal.h"

constexpr int CF_U = 0, CF_C = 1, CF_F = -1; // the C/F marker: undecided, coarse, fine

__host__ __device__ inline uint64_t splitmix64(uint64_t x)
{
   x += 0x9e3779b97f4a7c15ULL;
   x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
   x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
   return x ^ (x >> 31);
}

struct HCsr {
   int n = 0, m = 0;
   std::vector<int> rp{0}, cj;
   std::vector<double> v;
   long long nnz() const { return (long long)cj.size(); }
};

// a host CSR that someone else owns: the C-ABI's pointers or an HCsr (v null: pattern only)
struct HCsrView {
   int n, m;
   const int *rp, *cj;
   const double *v;
   long long nnz() const { return rp[n]; }
};
inline HCsrView view(const HCsr &M)
{
   return {M.n, M.m, M.rp.data(), M.cj.data(), M.v.empty() ? nullptr : M.v.data()};
}

// device array of at least one element, freed with its owner (move-only)
template <class T>
struct DBuf {
   T *p = nullptr;
   DBuf() = default;
   DBuf(DBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
   DBuf &operator=(DBuf &&o) noexcept
   {
      if (this != &o) {
         release();
         p = o.p;
         o.p = nullptr;
      }
      return *this;
   }
   ~DBuf() { release(); }
   int alloc(size_t count)
   {
      release();
      AMG_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
      return AMG_OK;
   }
   // the soft form: false when the device has no room, with the HIP error
   // cleared and no library error set (the caller does without the array)
   bool try_alloc(size_t count)
   {
      release();
      if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) == hipSuccess) return true;
      p = nullptr;
      (void)hipGetLastError();
      return false;
   }
   void release()
   {
      if (p) hipFree(p);
      p = nullptr;
   }
   // the array handed over to the caller, who frees it
   T *take()
   {
      T *q = p;
      p = nullptr;
      return q;
   }
   operator T *() const { return p; }
};

// device CSR, n x m (v unallocated: pattern only); release() frees before the scope ends
struct DCsr {
   int n = 0, m = 0;
   long long nnz = 0;
   DBuf<int> rp, cj;
   DBuf<double> v;
   void release()
   {
      rp.release(), cj.release(), v.release();
      nnz = 0;
   }
};

// the device selected and a stream of the call's own, drained and destroyed with
// the object: declare it before the buffers that its work uses
struct Session {
   hipStream_t s = nullptr;
   Session() = default;
   Session(const Session &) = delete;
   Session &operator=(const Session &) = delete;
   int open(int device)
   {
      AMG_HIP(hipSetDevice(device));
      AMG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      return AMG_OK;
   }
   ~Session()
   {
      if (s) {
         hipStreamSynchronize(s);
         hipStreamDestroy(s);
      }
   }
};

// d allocated here; the copy is asynchronous: h outlives the next synchronisation
template <class T>
int upload(hipStream_t s, const T *h, size_t count, DBuf<T> &d)
{
   AMG_TRY(d.alloc(count));
   if (count) AMG_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, s));
   return AMG_OK;
}

// asynchronous as well: h is valid after the next synchronisation
template <class T>
int download(hipStream_t s, const T *d, size_t count, std::vector<T> &h)
{
   h.resize(count);
   if (count) AMG_HIP(hipMemcpyAsync(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, s));
   return AMG_OK;
}

inline int upload_csr(hipStream_t s, const HCsrView &H, bool values, DCsr &D)
{
   D.n = H.n, D.m = H.m, D.nnz = H.nnz();
   AMG_TRY(upload(s, H.rp, (size_t)H.n + 1, D.rp));
   AMG_TRY(upload(s, H.cj, (size_t)D.nnz, D.cj));
   if (values) AMG_TRY(upload(s, H.v, (size_t)D.nnz, D.v));
   return AMG_OK;
}

inline int download_csr(hipStream_t s, const DCsr &D, bool values, HCsr &H)
{
   H.n = D.n, H.m = D.m;
   AMG_TRY(download(s, D.rp.p, (size_t)D.n + 1, H.rp));
   AMG_TRY(download(s, D.cj.p, (size_t)D.nnz, H.cj));
   if (values)
      AMG_TRY(download(s, D.v.p, (size_t)D.nnz, H.v));
   else
      H.v.clear();
   return AMG_OK;
}

// rp[i + 1] = rp[i] + cnt[i] for n rows from the caller's rp[0]; offsets are 32-bit
inline int scan_counts(const int *cnt, int n, int *rp)
{
   long long t = rp[0];
   for (int i = 0; i < n; i++) {
      t += cnt[i];
      if (t > INT_MAX) return amg_set_error(AMG_ERR_ARG, "classical setup on the device: more than 2^31 - 1 entries");
      rp[i + 1] = (int)t;
   }
   return AMG_OK;
}

// rowptr of n rows from their counts on the device, scanned on the host (its
// total sizes the output): rp on the host, which has to outlive the caller's
// next synchronisation, and d_rp, allocated here
inline int rowptr_of_counts(hipStream_t s, const int *d_cnt, int n, std::vector<int> &rp, DBuf<int> &d_rp)
{
   std::vector<int> cnt;
   AMG_TRY(download(s, d_cnt, (size_t)n, cnt));
   AMG_HIP(hipStreamSynchronize(s));
   rp.assign((size_t)n + 1, 0);
   AMG_TRY(scan_counts(cnt.data(), n, rp.data()));
   return upload(s, rp.data(), (size_t)n + 1, d_rp);
}

// rows in batches under a budget: batch b is rows cut[b]..cut[b + 1], as many as
// keep the sum of their costs within the budget, a row over it a batch of its own
inline std::vector<int> batch_bounds(const std::vector<long long> &cost, long long budget)
{
   const int n = (int)cost.size();
   std::vector<int> cut{0};
   for (int r0 = 0; r0 < n;) {
      long long tot = 0;
      int r1 = r0;
      while (r1 < n && (r1 == r0 || tot + cost[r1] <= budget)) tot += cost[r1++];
      cut.push_back(r0 = r1);
   }
   return cut;
}

// ---- amg_spgemm.hip: Gustavson products, bit-identical to amg_classical.cpp's spgemm()
// C = A B with every operand on the device
int spgemm_dev(hipStream_t s, const DCsr &A, const DCsr &B, DCsr &C);
// host CSR in and out through device `device`: C = A B; A_c = R (A P) with A P
// kept on the device; one level's SmoothTransfer (P~ truncated there when an
// add_* option is set, R~ then left to the caller)
int amg_spgemm_device(int device, const HCsr &A, const HCsr &B, HCsr &C);
int amg_rap_device(int device, const HCsr &A, const HCsr &P, const HCsr &R, HCsr &Ac);
int amg_smooth_transfer_device(int device, const HCsr &A, const HCsr &P, const HCsr &R, double w, int add_max,
                               double add_tf, HCsr &Ps, HCsr &Rs);

// ---- amg_trunc.hip: rows truncated, bit-identical to truncate_rows()
int trunc_dev(hipStream_t s, const DCsr &M, double tf, int maxel, DCsr &T);
int amg_truncate_device(int device, const HCsrView &M, double tf, int maxel, HCsr &T);

// ---- amg_setup_dev.hip: strength, transposes (with values when A has them), PMIS
// and interpolation (P.m = the coarse points) on a GPU, host CSR in and out, each
// bit-identical to its host function, and the level loop that keeps the
// hierarchy on the device (setup_on_device)
int amg_strength_device(int device, const HCsrView &A, double theta, double max_row_sum, int nfun, HCsr &S);
int amg_transpose_device(int device, const HCsrView &A, HCsr &T);
int amg_pmis_device(int device, const HCsrView &S, unsigned long long seed, int *cf, int *rounds);
int amg_interp_device(int device, const HCsrView &A, const HCsrView &S, const int *cf, int type, int nfun, HCsr &P);

// what the level loop hands back per level -- the C/F marker, P (n x nc),
// R = P^T and the coarse operator -- and the host coarsening it calls for HMIS
// (S in, marker out)
struct amg_setup_dev_level {
   std::vector<int> cf;
   HCsr P, R, Ac;
};
using amg_hmis_fn = std::function<void(const HCsr &S, std::vector<int> &cf)>;
int amg_classical_setup_device(const amg_classical_opts *o, const HCsr &A0, const amg_hmis_fn &hmis,
                               std::vector<amg_setup_dev_level> &levels);
