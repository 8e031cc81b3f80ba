// amg_format.hip -- the ladder of lossless compressed forms a registered matrix
// is read through: value index, (offset, value) dictionary,
// row patterns, paired-row patterns, master pattern with the 7-pt / 27-pt plane
// march, and the 3x3 block form.  Setup code, none of it hot: the collect /
// table / encode kernels, the host builders, amg_mat_finish and the forms'
// setters and getters.  A form's arrays are built in owned buffers (DBuf) and
// handed to the amg_mat only when the form is complete, so every early return
// leaves the matrix in the form below and frees what it allocated.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "amg_csr.h"

namespace {

// ---------------------------------------------------------------------------
// The one dictionary: at most DICT_MAX distinct 64-bit keys collected into a
// device hash set of DICT_SLOTS slots (open addressing), sorted on the host,
// then found again by the encoders with a lower bound over the sorted keys in
// LDS.  The value index, the (offset, value) dictionary and the row patterns
// differ in their keys only.
// ---------------------------------------------------------------------------
constexpr int DICT_SLOTS = 4096;
constexpr int DICT_MAX = 256;
constexpr unsigned long long DICT_EMPTY = ~0ULL; // an empty slot; never a key
constexpr int DICT_COUNTERS = 4;                 // [0]: keys in the table, the others the collector's own

__device__ __forceinline__ unsigned int dict_hash(unsigned long long k)
{
   k ^= k >> 33;
   k *= 0xff51afd7ed558ccdULL;
   k ^= k >> 33;
   return (unsigned int)k;
}

// more than DICT_MAX keys: the table is already useless (and a nearly full
// table would cost DICT_SLOTS probes per new key)
__device__ __forceinline__ bool dict_useless(const int *count)
{
   return __atomic_load_n(count, __ATOMIC_RELAXED) > DICT_MAX;
}

// key into the table; the slot's index if this lane created it, else -1
__device__ __forceinline__ int dict_insert(unsigned long long key, unsigned long long *slots, int *count)
{
   unsigned int h = dict_hash(key) & (DICT_SLOTS - 1);
   for (int probe = 0; probe < DICT_SLOTS; probe++) {
      const unsigned long long cur = __atomic_load_n(&slots[h], __ATOMIC_RELAXED);
      if (cur == key) return -1;
      if (cur == DICT_EMPTY) {
         const unsigned long long prev = atomicCAS(&slots[h], DICT_EMPTY, key);
         if (prev == DICT_EMPTY) {
            atomicAdd(count, 1);
            return (int)h;
         }
         if (prev == key) return -1;
      }
      h = (h + 1) & (DICT_SLOTS - 1);
   }
   return -1;
}

// the T sorted keys of a workgroup of >= DICT_MAX lanes, in LDS
struct DictKeys {
   unsigned long long tk[DICT_MAX];
   __device__ __forceinline__ void load(const unsigned long long *__restrict__ keys, int T)
   {
      if (threadIdx.x < DICT_MAX) tk[threadIdx.x] = threadIdx.x < T ? keys[threadIdx.x] : DICT_EMPTY;
      __syncthreads();
   }
   // index of the first key >= key (the key's own index when it is in the table)
   __device__ __forceinline__ int find(unsigned long long key, int T) const
   {
      int lo = 0, hi = T - 1;
      while (lo < hi) {
         const int mid = (lo + hi) >> 1;
         if (tk[mid] < key)
            lo = mid + 1;
         else
            hi = mid;
      }
      return lo;
   }
};

// A collection's scratch and result.  On the device: `slots`, the table, after
// dict_collect the T sorted keys; `aux`, the counters and (with_rep) one int
// per slot, after dict_collect one per sorted key.
struct Dict {
   DBuf<unsigned long long> slots;
   DBuf<int> aux;
   std::vector<unsigned long long> keys; // ascending as unsigned 64-bit; empty: no table (none or > DICT_MAX keys)
   std::vector<int> rep;                 // the companion of each key
   int counter[DICT_COUNTERS] = {};      // as the collector left them
   int T() const { return (int)keys.size(); }
   int *count() const { return aux.p; }
   int *rep_dev() const { return aux.p + DICT_COUNTERS; }
};

// Runs launch(slots, count, rep) on cleared scratch and brings the table back
// sorted: d.keys (with_rep: and d.rep) on the host and on the device.
template <class Launch>
int dict_collect(hipStream_t s, bool with_rep, Launch &&launch, Dict &d)
{
   AMG_TRY(d.slots.alloc(DICT_SLOTS));
   AMG_TRY(d.aux.alloc(DICT_COUNTERS + (with_rep ? DICT_SLOTS : 0)));
   AMG_HIP(hipMemsetAsync(d.slots, 0xff, DICT_SLOTS * sizeof(unsigned long long), s));
   AMG_HIP(hipMemsetAsync(d.aux, 0, DICT_COUNTERS * sizeof(int), s));
   launch(d.slots.p, d.count(), d.rep_dev());
   std::vector<unsigned long long> h(DICT_SLOTS);
   std::vector<int> hr(with_rep ? DICT_SLOTS : 0);
   AMG_TRY(download(s, d.slots.p, h.size(), h));
   AMG_TRY(download(s, d.rep_dev(), hr.size(), hr));
   AMG_HIP(hipMemcpyAsync(d.counter, d.count(), sizeof(d.counter), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   if (d.counter[0] < 1 || d.counter[0] > DICT_MAX) return AMG_OK;
   std::vector<std::pair<unsigned long long, int>> kr;
   for (int i = 0; i < DICT_SLOTS; i++)
      if (h[i] != DICT_EMPTY) kr.push_back({h[i], with_rep ? hr[i] : 0});
   std::sort(kr.begin(), kr.end()); // the keys are distinct
   for (const auto &p : kr) {
      d.keys.push_back(p.first);
      d.rep.push_back(p.second);
   }
   AMG_HIP(hipMemcpyAsync(d.slots, d.keys.data(), d.T() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
   if (with_rep) AMG_HIP(hipMemcpyAsync(d.rep_dev(), d.rep.data(), d.T() * sizeof(int), hipMemcpyHostToDevice, s));
   return AMG_OK;
}

// collect / encode grids: up to 8192 workgroups of 256 lanes, one item per lane
inline int dict_grid(long long items) { return (int)std::min<long long>(8192, (items + 255) / 256); }

// ---------------------------------------------------------------------------
// value-indexed CSR (CSR-VI): when the matrix holds at most 256 distinct
// values (by bit pattern) the hot kernels stream one byte per entry instead
// of eight and read the value from an LDS table -- bit-identical products.
// val stays resident for the other kernels and for amg_mat_download.
// ---------------------------------------------------------------------------
__global__ void vi_collect_k(const double *__restrict__ val, long long nnz, unsigned long long *slots, int *count)
{
   unsigned long long last0 = DICT_EMPTY, last1 = DICT_EMPTY;
   const long long stride = (long long)gridDim.x * blockDim.x;
   for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nnz; i += stride) {
      const unsigned long long key = (unsigned long long)__double_as_longlong(val[i]);
      // before the repeat filter, which starts out holding this very pattern
      if (key == DICT_EMPTY) {
         // the empty marker's own pattern: give up on the table (a bit above any key
         // count, set and not added, so that no number of such entries wraps it away)
         atomicOr(count, 1 << 20);
         return;
      }
      if (key == last0 || key == last1) continue;
      last1 = last0;
      last0 = key;
      if (dict_useless(count)) return; // many distinct values: stop reading (keeps registration fast)
      dict_insert(key, slots, count);
   }
}

__global__ void vi_encode_k(const double *__restrict__ val, long long nnz,
                            const unsigned long long *__restrict__ keys, int T,
                            unsigned char *__restrict__ vidx)
{
   __shared__ DictKeys dk;
   dk.load(keys, T);
   const long long stride = (long long)gridDim.x * blockDim.x;
   for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nnz; i += stride)
      vidx[i] = (unsigned char)dk.find((unsigned long long)__double_as_longlong(val[i]), T);
}

int build_value_index(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   Dict d;
   AMG_TRY(dict_collect(s, false, [&](unsigned long long *slots, int *count, int *) {
      vi_collect_k<<<dict_grid(A->nnz), 256, 0, s>>>(A->val, A->nnz, slots, count);
   }, d));
   const int T = d.T();
   if (!T) return AMG_OK; // plain CSR
   std::vector<double> tab(256, 0.0);
   std::memcpy(tab.data(), d.keys.data(), T * sizeof(double));
   DBuf<unsigned char> vidx;
   DBuf<double> vtab;
   if (!vidx.try_alloc((size_t)A->nnz + 64) || !vtab.try_alloc(256)) return AMG_OK; // no room: keep plain CSR
   AMG_HIP(hipMemcpyAsync(vtab, tab.data(), 256 * sizeof(double), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemsetAsync(vidx.p + A->nnz, 0, 64, s));
   vi_encode_k<<<dict_grid(A->nnz), 256, 0, s>>>(A->val, A->nnz, d.slots, T, vidx);
   AMG_HIP(hipStreamSynchronize(s));
   A->vidx = vidx.take();
   A->vtab = vtab.take();
   A->vi_n = T;
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// dictionary-coded CSR (CSR-DC) on top of the value index: when every entry's
// (col - anchor, value) pair comes from at most 256 distinct pairs and no row
// holds more than AMG_DC_MAXROW entries, each entry becomes one byte and the
// lane-per-row kernel reads x[anchor + off] coalesced across a wave.
// ---------------------------------------------------------------------------
// keys: (col - anchor) in the high bits, the value-index byte low
__device__ __forceinline__ unsigned long long dc_key(int off, unsigned char b)
{
   return ((unsigned long long)(unsigned int)off << 8) | b;
}

// anchor of row i: its first column (the diagonal for diag-first square
// operators, the parent coarse point for interpolation rows).
// count[1] = the longest row, count[2] = some row's anchor is not its own index
__global__ void dc_collect_k(const int *__restrict__ rowptr, const int *__restrict__ col,
                             const unsigned char *__restrict__ vidx, int n, unsigned long long *slots, int *count)
{
   // the repeat filter starts at DICT_EMPTY, which no key equals: dc_key has 40 bits
   unsigned long long last0 = DICT_EMPTY, last1 = DICT_EMPTY;
   int ml = 0, offrow = 0;
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int rs = rowptr[i], re = rowptr[i + 1];
      ml = max(ml, re - rs);
      const int anc = rs < re ? col[rs] : i;
      offrow |= (anc != i);
      for (int k = rs; k < re; k++) {
         const unsigned long long key = dc_key(col[k] - anc, vidx[k]);
         if (key == last0 || key == last1) continue;
         last1 = last0;
         last0 = key;
         if (dict_useless(count)) continue; // only the longest row and the anchors from here on
         dict_insert(key, slots, count);
      }
   }
   atomicMax(count + 1, ml);
   if (offrow) atomicOr(count + 2, 1);
}

__global__ void dc_encode_k(const int *__restrict__ rowptr, const int *__restrict__ col,
                            const unsigned char *__restrict__ vidx, int n,
                            const unsigned long long *__restrict__ keys, int T,
                            unsigned char *__restrict__ didx, int *__restrict__ anch)
{
   __shared__ DictKeys dk;
   dk.load(keys, T);
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int rs = rowptr[i], re = rowptr[i + 1];
      const int anc = rs < re ? col[rs] : i;
      if (anch) anch[i] = anc;
      for (int k = rs; k < re; k++) didx[k] = (unsigned char)dk.find(dc_key(col[k] - anc, vidx[k]), T);
   }
}

int build_dict_index(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   const int n = A->nrows;
   Dict d;
   AMG_TRY(dict_collect(s, false, [&](unsigned long long *slots, int *count, int *) {
      if (n > 0) dc_collect_k<<<dict_grid(n), 256, 0, s>>>(A->rowptr, A->col, A->vidx, n, slots, count);
   }, d));
   const int T = d.T(), maxrow = d.counter[1];
   if (!T || maxrow > AMG_DC_MAXROW) return AMG_OK;
   std::vector<double> vt(256, 0.0);
   AMG_HIP(hipMemcpy(vt.data(), A->vtab, 256 * sizeof(double), hipMemcpyDeviceToHost));
   std::vector<int> off(256, 0);
   std::vector<double> dv(256, 0.0);
   for (int t = 0; t < T; t++) {
      off[t] = (int)(unsigned int)(d.keys[t] >> 8);
      dv[t] = vt[d.keys[t] & 0xff];
   }
   // anchors only where some row does not start at its own index (the
   // transfers); a distributed slab [owned | ghost] keeps anchor = row
   const bool need_anchor = d.counter[2] != 0;
   DBuf<unsigned char> didx;
   DBuf<int> doff, danch;
   DBuf<double> dval;
   if (!didx.try_alloc((size_t)A->nnz + 64) || !doff.try_alloc(256) || !dval.try_alloc(256) ||
       (need_anchor && !danch.try_alloc(n)))
      return AMG_OK;
   AMG_HIP(hipMemcpyAsync(doff, off.data(), 256 * sizeof(int), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(dval, dv.data(), 256 * sizeof(double), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemsetAsync(didx.p + A->nnz, 0, 64, s));
   dc_encode_k<<<dict_grid(n), 256, 0, s>>>(A->rowptr, A->col, A->vidx, n, d.slots, T, didx, danch);
   AMG_HIP(hipStreamSynchronize(s));
   A->didx = didx.take();
   A->doff = doff.take();
   A->dval = dval.take();
   A->danch = danch.take();
   A->dc_n = T;
   A->dc_maxrow = maxrow;
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// row-pattern-coded CSR: when every row is non-empty and the rows' dictionary
// sequences take at most 256 distinct values, one byte per row names the
// sequence.  Lossless: the kernels walk the same entries in
// the same order.
// ---------------------------------------------------------------------------
// key of row i's dictionary sequence: exact for <= 7 entries (length byte +
// the entries), else a 56-bit hash above the length byte (verified after
// encoding, so a collision only disables the format)
__device__ __forceinline__ unsigned long long rp_key(const unsigned char *__restrict__ didx, int rs, int len)
{
   if (len <= 7) {
      unsigned long long k = (unsigned long long)len;
      for (int j = 0; j < len; j++) k |= (unsigned long long)didx[rs + j] << (8 * (j + 1));
      return k;
   }
   unsigned long long h = 0xcbf29ce484222325ULL ^ (unsigned long long)len;
   for (int j = 0; j < len; j++) h = (h ^ didx[rs + j]) * 0x100000001b3ULL;
   h ^= h >> 29;
   h *= 0xbf58476d1ce4e5b9ULL;
   h ^= h >> 32;
   return (h << 8) | (unsigned long long)len;
}

// distinct row keys into slots (the row that created a slot into rep), and in
// count[1] the rows that cannot be coded (empty or longer than AMG_DC_MAXROW)
__global__ void rp_collect_k(const int *__restrict__ rowptr, const unsigned char *__restrict__ didx, int n,
                             unsigned long long *slots, int *rep, int *count)
{
   // DICT_EMPTY is no key here either: rp_key's low byte is a length of at most 32
   unsigned long long last = DICT_EMPTY;
   int nbad = 0;
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int rs = rowptr[i], len = rowptr[i + 1] - rs;
      if (len < 1 || len > AMG_DC_MAXROW) {
         nbad++;
         continue;
      }
      const unsigned long long key = rp_key(didx, rs, len);
      if (key == last) continue;
      last = key;
      if (dict_useless(count)) continue; // too many patterns: only count bad rows
      const int slot = dict_insert(key, slots, count);
      if (slot >= 0) rep[slot] = i;
   }
   if (nbad) atomicAdd(count + 1, nbad);
}

// pattern table: entry t = [length, dictionary bytes of representative row rep[t]]
__global__ void rp_table_k(const int *__restrict__ rowptr, const unsigned char *__restrict__ didx,
                           const int *__restrict__ rep, int T, unsigned char *__restrict__ ptab)
{
   const int t = blockIdx.x * blockDim.x + threadIdx.x;
   if (t >= T) return;
   const int rs = rowptr[rep[t]], len = rowptr[rep[t] + 1] - rs;
   unsigned char *pp = ptab + t * AMG_RP_STRIDE;
   pp[0] = (unsigned char)len;
   for (int j = 0; j < AMG_DC_MAXROW; j++) pp[1 + j] = j < len ? didx[rs + j] : 0;
}

// rpat[i] = index of row i's key among the T sorted keys; rows whose bytes
// differ from their pattern (a hash collision) are counted in bad
__global__ void rp_encode_k(const int *__restrict__ rowptr, const unsigned char *__restrict__ didx, int n,
                            const unsigned long long *__restrict__ keys, int T,
                            const unsigned char *__restrict__ ptab, unsigned char *__restrict__ rpat,
                            int *bad)
{
   __shared__ DictKeys dk;
   dk.load(keys, T);
   int nbad = 0;
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int rs = rowptr[i], len = rowptr[i + 1] - rs;
      const unsigned long long key = rp_key(didx, rs, len);
      const int lo = dk.find(key, T);
      rpat[i] = (unsigned char)lo;
      const unsigned char *pp = ptab + lo * AMG_RP_STRIDE;
      bool ok = dk.tk[lo] == key && pp[0] == len;
      for (int j = 0; ok && j < len; j++) ok = pp[1 + j] == didx[rs + j];
      nbad += !ok;
   }
   if (nbad) atomicAdd(bad, nbad);
}

int build_row_pattern(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   const int n = A->nrows;
   Dict d;
   AMG_TRY(dict_collect(s, true, [&](unsigned long long *slots, int *count, int *rep) {
      if (n > 0) rp_collect_k<<<dict_grid(n), 256, 0, s>>>(A->rowptr, A->didx, n, slots, rep, count);
   }, d));
   const int T = d.T();
   if (!T || d.counter[1] != 0) return AMG_OK; // too many patterns, or a row that cannot be coded
   DBuf<unsigned char> rpat, ptab;
   if (!rpat.try_alloc(n) || !ptab.try_alloc(256 * AMG_RP_STRIDE)) return AMG_OK;
   AMG_HIP(hipMemsetAsync(ptab, 0, 256 * AMG_RP_STRIDE, s));
   int *bad = d.count() + 1; // zero: no row was bad
   rp_table_k<<<1, 256, 0, s>>>(A->rowptr, A->didx, d.rep_dev(), T, ptab);
   rp_encode_k<<<dict_grid(n), 256, 0, s>>>(A->rowptr, A->didx, n, d.slots, T, ptab, rpat, bad);
   int nbad = 0;
   AMG_HIP(hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   if (nbad != 0) return AMG_OK; // a hash collision: keep the dictionary-coded form
   A->rpat = rpat.take();
   A->ptab = ptab.take();
   A->rp_n = T;
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// paired-row-pattern CSR on top of the row patterns: rows 2t and 2t+1 share
// one merged entry list in which an entry of row 2t at column c and an entry
// of row 2t+1 at column c + 1 are one 16-byte x load.
// Columns are relative to row 2t's anchor (the row itself for square
// diagonal-first operators); row 2t+1's anchor is da further.  The merge is a
// shortest common supersequence of the two rows' entry lists (matched on
// column), so each row still sums its own entries in its CSR order:
// bit-identical to the single-row kernel.
// ---------------------------------------------------------------------------
void pair_merge(const unsigned char *a, int la, const unsigned char *b, int lb, int da, const std::vector<int> &off,
                std::vector<unsigned int> &out)
{
   int dp[AMG_PP_MAXROW + 2][AMG_PP_MAXROW + 2] = {};
   auto match = [&](int i, int j) { return off[b[j]] + da == off[a[i]] + 1; };
   for (int i = la - 1; i >= 0; i--)
      for (int j = lb - 1; j >= 0; j--)
         dp[i][j] = match(i, j) ? dp[i + 1][j + 1] + 1 : std::max(dp[i + 1][j], dp[i][j + 1]);
   int i = 0, j = 0;
   while (i < la || j < lb) {
      if (i < la && j < lb && match(i, j) && dp[i][j] == dp[i + 1][j + 1] + 1) {
         out.push_back(a[i] | (unsigned)b[j] << 8 | 3u << 16);
         i++;
         j++;
      } else if (j >= lb || (i < la && dp[i + 1][j] >= dp[i][j + 1])) {
         out.push_back(a[i] | 1u << 16);
         i++;
      } else {
         out.push_back((unsigned)b[j] << 8 | 2u << 16);
         j++;
      }
   }
}

// pair key: (pattern of row 2t, of row 2t+1 or 256 if none, anchor delta
// da = anch[2t+1] - anch[2t] + AMG_PP_DA0 in [0, AMG_PP_NDA)); a delta out of
// range flags the matrix (flags[AMG_PP_NK])
__device__ __forceinline__ int pp_key(const unsigned char *__restrict__ rpat, const int *__restrict__ anch, int n,
                                      int t)
{
   const bool two = 2 * t + 1 < n;
   const int da = (two && anch) ? anch[2 * t + 1] - anch[2 * t] + AMG_PP_DA0 : AMG_PP_DA0;
   if (da < 0 || da >= AMG_PP_NDA) return -1;
   return (rpat[2 * t] * 257 + (two ? rpat[2 * t + 1] : 256)) * AMG_PP_NDA + da;
}

__global__ void pp_collect_k(const unsigned char *__restrict__ rpat, const int *__restrict__ anch, int n,
                             unsigned char *flags)
{
   const int np = (n + 1) / 2;
   for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < np; t += gridDim.x * blockDim.x) {
      int k = pp_key(rpat, anch, n, t);
      if (k < 0) k = AMG_PP_NK;
      if (!flags[k]) flags[k] = 1;
   }
}

// ppat[t] = the pair's table index; counts[p] += pairs of pattern p
__global__ __launch_bounds__(256) void pp_encode_k(const unsigned char *__restrict__ rpat,
                                                   const int *__restrict__ anch, int n,
                                                   const unsigned char *__restrict__ map,
                                                   unsigned char *__restrict__ ppat,
                                                   unsigned long long *__restrict__ counts)
{
   __shared__ unsigned int hist[256];
   hist[threadIdx.x] = 0;
   __syncthreads();
   const int np = (n + 1) / 2;
   for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < np; t += gridDim.x * blockDim.x) {
      const unsigned char p = map[pp_key(rpat, anch, n, t)];
      ppat[t] = p;
      atomicAdd(&hist[p], 1u);
   }
   __syncthreads();
   if (hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

inline int pp_grid(int nrows) { return std::min(8192, (nrows + 511) / 512); }

// one workgroup per 512-row slab: least anchor of its even rows, then each
// pair's 16-bit delta from it
__global__ __launch_bounds__(256) void pp_anchor_k(const int *__restrict__ anch, int n, int *__restrict__ pbase,
                                                  unsigned short *__restrict__ pdelta, int *__restrict__ ok)
{
   __shared__ int red[2][256];
   const int slab = (int)blockIdx.x, tid = (int)threadIdx.x;
   const long long row = (long long)slab * 512 + 2 * tid;
   const int a = row < n ? anch[row] : INT_MAX;
   red[0][tid] = a;
   red[1][tid] = row < n ? a : INT_MIN;
   __syncthreads();
   for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) {
         red[0][tid] = min(red[0][tid], red[0][tid + w]);
         red[1][tid] = max(red[1][tid], red[1][tid + w]);
      }
      __syncthreads();
   }
   const int lo = red[0][0], hi = red[1][0];
   if (tid == 0) {
      pbase[slab] = lo;
      if ((long long)hi - lo > 65535) *ok = 0;
   }
   if (row < n) pdelta[row >> 1] = (unsigned short)(a - lo);
}

// Slab-compressed anchors for the paired kernel (amg_internal.h): anchor(2t)
// = pbase[2t >> 9] + pdelta[t].  Kept only when every 512-row slab's anchors
// span at most 65535 (interpolation: a fine line maps to half a coarse line).
// A has rows and an anchor array.
int compress_pair_anchors(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   const int ns = (A->nrows + 511) / 512;
   DBuf<int> pbase, ok;
   DBuf<unsigned short> pdelta;
   if (!pbase.try_alloc(ns) || !pdelta.try_alloc(((size_t)A->nrows + 1) / 2) || !ok.try_alloc(1)) return AMG_OK;
   const int one = 1;
   int okh = 0;
   AMG_HIP(hipMemcpyAsync(ok, &one, sizeof(int), hipMemcpyHostToDevice, s));
   pp_anchor_k<<<ns, 256, 0, s>>>(A->danch, A->nrows, pbase, pdelta, ok);
   AMG_HIP(hipMemcpyAsync(&okh, ok, sizeof(int), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   if (!okh) return AMG_OK;
   A->pbase = pbase.take();
   A->pdelta = pdelta.take();
   return AMG_OK;
}

int build_pair_pattern(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   const int n = A->nrows;
   constexpr int NK = AMG_PP_NK;
   // scratch: NK + 1 flags, the NK-byte key -> pattern map, 256 pair counts (8-aligned)
   DBuf<unsigned char> flags;
   AMG_TRY(flags.alloc(2 * (size_t)NK + 1 + 256 * sizeof(unsigned long long) + 8));
   unsigned char *map = flags.p + NK + 1;
   unsigned long long *counts = reinterpret_cast<unsigned long long *>(
      (reinterpret_cast<uintptr_t>(map + NK) + 7) & ~(uintptr_t)7);
   AMG_HIP(hipMemsetAsync(flags, 0, NK + 1, s));
   if (n > 0) pp_collect_k<<<pp_grid(n), 256, 0, s>>>(A->rpat, A->danch, n, flags);
   std::vector<unsigned char> hf(NK + 1), pt(256 * AMG_RP_STRIDE);
   std::vector<int> off(256);
   AMG_HIP(hipMemcpyAsync(hf.data(), flags, NK + 1, hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(pt.data(), A->ptab, pt.size(), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(off.data(), A->doff, 256 * sizeof(int), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   std::vector<unsigned char> hm(NK, 0);
   std::vector<unsigned int> tab;
   const int PS = amg_pp_stride(A->dc_maxrow);
   int T = hf[NK] ? 257 : 0; // an anchor delta out of range: not pair-coded
   bool centre0 = !A->danch; // square diagonal-first: is entry 0 the diagonal of both rows?
   std::vector<int> msz(256, 0), ssz(256, 0); // per pattern: merged entries, the longer row's
   for (int k = 0; k < NK && T <= 256; k++) {
      if (!hf[k]) continue;
      if (T == 256) {
         T++;
         break;
      }
      const int pk = k / AMG_PP_NDA, da = k % AMG_PP_NDA - AMG_PP_DA0;
      const int p0 = pk / 257, p1 = pk % 257;
      const unsigned char *a = pt.data() + p0 * AMG_RP_STRIDE;
      std::vector<unsigned int> el;
      if (p1 < 256) {
         const unsigned char *b = pt.data() + p1 * AMG_RP_STRIDE;
         pair_merge(a + 1, a[0], b + 1, b[0], A->danch ? da : 1, off, el);
         msz[T] = (int)el.size();
         ssz[T] = std::max<int>(a[0], b[0]);
      } else {
         for (int j = 0; j < a[0]; j++) el.push_back(a[1 + j] | 1u << 16);
      }
      // header: nel | first dictionary entry of row 2t << 8 | of row 2t+1 << 16
      // | row 2t+1 present << 24 | (anchor delta + 16) << 25
      std::vector<unsigned int> w(PS, 0);
      w[0] = (unsigned)el.size() | (unsigned)a[1] << 8 |
             (p1 < 256 ? (unsigned)pt[p1 * AMG_RP_STRIDE + 1] << 16 | 1u << 24 : 0u) |
             (unsigned)(da + 16) << 25;
      for (size_t e = 0; e < el.size(); e++) w[1 + e] = el[e];
      centre0 = centre0 && !el.empty() && off[el[0] & 0xff] == 0 && (el[0] >> 16 & 1) &&
                (p1 == 256 || (el[0] >> 16 & 3) == 3);
      tab.insert(tab.end(), w.begin(), w.end());
      hm[k] = (unsigned char)T++;
   }
   if (T < 1 || T > 256 || (size_t)T * PS * 4 > (size_t)AMG_PP_LDS) return AMG_OK;
   DBuf<unsigned char> ppat;
   DBuf<unsigned int> pptab;
   if (!ppat.try_alloc(((size_t)n + 1) / 2) || !pptab.try_alloc(tab.size())) return AMG_OK;
   AMG_HIP(hipMemcpyAsync(map, hm.data(), NK, hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(pptab, tab.data(), tab.size() * sizeof(unsigned int), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemsetAsync(counts, 0, 256 * sizeof(unsigned long long), s));
   if (n > 0) pp_encode_k<<<pp_grid(n), 256, 0, s>>>(A->rpat, A->danch, n, map, ppat, counts);
   std::vector<unsigned long long> cnt(256);
   AMG_HIP(hipMemcpyAsync(cnt.data(), counts, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   // a pair lane walks the merged list: worth it only when it is hardly
   // longer than the longer of its rows, counted over all row pairs (7-pt /
   // 27-pt operators and interpolation: as long; restriction, anchors 2
   // apart: 4/3 as long, and slower than one row per lane)
   double merged = 0.0, single = 0.0;
   for (int t = 0; t < T; t++) {
      merged += (double)cnt[t] * msz[t];
      single += (double)cnt[t] * ssz[t];
   }
   if (merged > AMG_PP_MAXFILL * single) return AMG_OK;
   A->ppat = ppat.take();
   A->pptab = pptab.take();
   A->pp_n = T;
   A->pp_stride = PS;
   A->pp_centre0 = centre0 ? 1 : 0;
   if (A->ctx->pair_anchor16 && A->danch && n > 0) AMG_TRY(compress_pair_anchors(A));
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// Master-pattern form on top of the pair patterns of a square,
// diagonal-first operator: every row's column offsets (relative to the row)
// must follow the master order -- 0 first, then ascending -- so a row's
// entries are an ordered subsequence of the master list and walking the
// master with per-row use bits adds exactly the row's products in its CSR
// order (bit-identical).  Offsets then become wave-uniform scalars and the
// per-entry LDS lookups of the pair kernel disappear.
// ---------------------------------------------------------------------------
// what the march detection reads of a master-coded matrix, on the host
struct MasterTab {
   std::vector<int> mo;                  // master order of the column offsets
   std::vector<unsigned long long> mask; // per pair pattern: the row-use bits
   std::vector<double> mv;               // per pair pattern and master entry: the two rows' values
};

// the master order, use masks and values: A->mp_J = 0 when A is not master-coded
int master_tables(amg_mat *A, MasterTab &m)
{
   hipStream_t s = A->ctx->stream;
   const int T = A->pp_n, PS = A->pp_stride, D = A->dc_n;
   std::vector<unsigned int> tab((size_t)T * PS);
   std::vector<int> off(256);
   std::vector<double> val(256);
   AMG_HIP(hipMemcpyAsync(tab.data(), A->pptab, tab.size() * 4, hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(off.data(), A->doff, 256 * sizeof(int), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipMemcpyAsync(val.data(), A->dval, 256 * sizeof(double), hipMemcpyDeviceToHost, s));
   AMG_HIP(hipStreamSynchronize(s));
   std::vector<int> &mo = m.mo;
   for (int d = 0; d < D; d++) mo.push_back(off[d]);
   std::sort(mo.begin(), mo.end());
   mo.erase(std::unique(mo.begin(), mo.end()), mo.end());
   auto z = std::find(mo.begin(), mo.end(), 0);
   if (z == mo.end() || (int)mo.size() > AMG_MP_MAXJ) return AMG_OK;
   mo.erase(z);
   mo.insert(mo.begin(), 0);
   const int J = (int)mo.size();
   auto pos = [&](int o) { return (int)(std::find(mo.begin(), mo.end(), o) - mo.begin()); };
   std::vector<unsigned long long> &mask = m.mask;
   std::vector<double> &mv = m.mv;
   mask.assign(T, 0);
   mv.assign((size_t)T * J * 2, 0.0);
   std::vector<unsigned long long> uni_bits(J, 0);
   std::vector<int> uni_set(J, 0);
   bool uni = true;
   for (int t = 0; t < T; t++) {
      const unsigned int *w = tab.data() + (size_t)t * PS;
      const int nel = w[0] & 0xff;
      const bool two = (w[0] >> 24) & 1;
      int last[2] = {-1, -1};
      for (int e = 0; e < nel; e++) {
         const unsigned int en = w[1 + e];
         for (int r = 0; r < 2; r++) {
            if (!(en >> (16 + r) & 1)) continue;
            const int d = r ? (en >> 8 & 0xff) : (en & 0xff);
            const int j = pos(off[d]);
            if (j <= last[r]) return AMG_OK; // not an ordered subsequence of the master
            last[r] = j;
            mask[t] |= 1ULL << (2 * j + r);
            mv[((size_t)t * J + j) * 2 + r] = val[d];
            unsigned long long bits;
            std::memcpy(&bits, &val[d], 8);
            if (!uni_set[j]) {
               uni_set[j] = 1;
               uni_bits[j] = bits;
            } else if (uni_bits[j] != bits) {
               uni = false;
            }
         }
      }
      // a_ii = A_data[A_i[i]] and x_i come from master entry 0 (the diagonal)
      if (!(mask[t] & 1ULL) || (two && !(mask[t] & 2ULL))) return AMG_OK;
   }
   if (!uni && (size_t)T * J * 16 > (size_t)AMG_MP_LDS) return AMG_OK;
   DBuf<unsigned long long> mpmask;
   DBuf<double> mpval;
   if (!mpmask.try_alloc(T) || (!uni && !mpval.try_alloc(mv.size()))) return AMG_OK;
   AMG_HIP(hipMemcpyAsync(mpmask, mask.data(), (size_t)T * 8, hipMemcpyHostToDevice, s));
   if (!uni) AMG_HIP(hipMemcpyAsync(mpval, mv.data(), mv.size() * 8, hipMemcpyHostToDevice, s));
   AMG_HIP(hipStreamSynchronize(s));
   A->mpmask = mpmask.take();
   A->mpval = mpval.take();
   for (int j = 0; j < J; j++) {
      A->mp_off[j] = mo[j];
      std::memcpy(&A->mp_val[j], &uni_bits[j], 8);
   }
   A->mp_uni = uni ? 1 : 0;
   A->mp_J = J;
   return AMG_OK;
}

// plane-marching form: master [0, -P, -S, -1, +1, +S, +P], whole planes of
// P rows (P % 512 == 0: a workgroup's 512 positions never straddle planes)
// (S even: every pair's +-S operand pair is one aligned-in-range 16-byte load)
void detect_march7(amg_mat *A, const std::vector<int> &mo)
{
   if (A->ctx->plane_march && A->mp_J == 7 && mo[3] == -1 && mo[4] == 1 && mo[1] == -mo[6] &&
       mo[2] == -mo[5] && mo[5] > 1 && mo[5] % 2 == 0 && mo[6] > mo[5] && mo[6] % 512 == 0 &&
       A->nrows % mo[6] == 0 && A->nrows / mo[6] >= 2 && A->nrows < (1 << 29)) { // 32-bit byte offsets
      A->mz_P = mo[6];
      A->mz_S = mo[5];
   }
}

// 27-pt plane march: master [0, dz P + dy S + dx ascending (centre skipped)]
int detect_march27(amg_mat *A, const MasterTab &m)
{
   const std::vector<int> &mo = m.mo;
   const std::vector<unsigned long long> &mask = m.mask;
   const std::vector<double> &mv = m.mv;
   const int T = A->pp_n, J = A->mp_J;
   const bool uni = A->mp_uni;
   if (!(A->ctx->plane_march && J == 27 && A->nrows < (1 << 29) && (uni || T <= 64))) return AMG_OK;
   const int S = mo[16], P = mo[22];
   bool ok = S >= 4 && S % 2 == 0 && P % 512 == 0 && P % S == 0 && P / S >= 3 && A->nrows % P == 0 &&
             A->nrows / P >= 2;
   for (int L = 0, j = 1; ok && L < 27; L++) {
      if (L == 13) continue;
      const int o = (L / 9 - 1) * P + ((L / 3) % 3 - 1) * S + (L % 3 - 1);
      ok = mo[j++] == o;
   }
   int dom = -1;
   if (ok && !uni) {
      // the most frequent pattern using all 27 entries in both rows with
      // bit-equal values in the two rows
      std::vector<unsigned char> pp((size_t)(A->nrows / 2));
      AMG_HIP(hipMemcpy(pp.data(), A->ppat, pp.size(), hipMemcpyDeviceToHost));
      std::vector<long long> cnt(T, 0);
      for (unsigned char q : pp) cnt[q]++;
      const unsigned long long full = (1ull << 54) - 1;
      for (int t = 0; t < T; t++) {
         if (mask[t] != full) continue;
         bool same = true;
         for (int j = 0; j < J && same; j++)
            same = std::memcmp(&mv[((size_t)t * J + j) * 2], &mv[((size_t)t * J + j) * 2 + 1], 8) == 0;
         if (same && (dom < 0 || cnt[t] > cnt[dom])) dom = t;
      }
      if (dom >= 0)
         for (int j = 0; j < J; j++) A->mz_domval[j] = mv[((size_t)dom * J + j) * 2];
      // x-edge pair patterns (the waves at both ends of every line)
      if (dom >= 0) {
         unsigned long long lo_x = 0, hi_y = 0; // row 2t's mask without dx = -1, row 2t+1's without +1
         for (int j = 0; j < 27; j++) {
            const int L = j == 0 ? 13 : (j <= 13 ? j - 1 : j), dx = L % 3 - 1;
            if (dx != -1) lo_x |= 1ull << (2 * j);
            if (dx != 1) hi_y |= 2ull << (2 * j);
         }
         const unsigned long long even = 0x5555555555555555ull & full, odd = 0xAAAAAAAAAAAAAAAAull & full;
         long long best_lo = 0, best_hi = 0;
         for (int t = 0; t < T; t++) {
            auto same = [&](int j, int r) {
               return std::memcmp(&mv[((size_t)t * J + j) * 2 + r], &A->mz_domval[j], 8) == 0;
            };
            if (mask[t] == (lo_x | odd) && cnt[t] > best_lo) {
               bool ok = true;
               for (int j = 0; j < J && ok; j++) ok = same(j, 1) && (!((lo_x >> (2 * j)) & 1) || same(j, 0));
               if (ok) A->mz_xlo = t, best_lo = cnt[t];
            }
            if (mask[t] == (even | hi_y) && cnt[t] > best_hi) {
               bool ok = true;
               for (int j = 0; j < J && ok; j++) ok = same(j, 0);
               if (ok) {
                  A->mz_xhi = t, best_hi = cnt[t];
                  for (int j = 0; j < J; j++) A->mz_hival[j] = mv[((size_t)t * J + j) * 2 + 1];
               }
            }
         }
      }
   }
   if (ok) {
      A->mz_P = P;
      A->mz_S = S;
      A->mz27 = 1;
      A->mz_dom = dom;
   }
   return AMG_OK;
}

int build_master_pattern(amg_mat *A)
{
   if (!A->ppat || A->danch || A->nrows != A->ncols || A->nrows < 2 || A->pp_n < 1) return AMG_OK;
   MasterTab m;
   AMG_TRY(master_tables(A, m));
   if (!A->mp_J) return AMG_OK;
   detect_march7(A, m.mo);
   return detect_march27(A, m);
}

// ---------------------------------------------------------------------------
// one drop function per form: its arrays freed, its fields back to "not coded"
// ---------------------------------------------------------------------------
template <class T>
void dfree(T *&p)
{
   hipFree(p);
   p = nullptr;
}

void drop_value_index(amg_mat *A)
{
   dfree(A->vidx), dfree(A->vtab);
   A->vi_n = 0;
}

void drop_dict_index(amg_mat *A)
{
   dfree(A->didx), dfree(A->doff), dfree(A->dval), dfree(A->danch);
   A->dc_n = A->dc_maxrow = 0;
}

void drop_row_pattern(amg_mat *A)
{
   dfree(A->rpat), dfree(A->ptab);
   A->rp_n = 0;
}

// back to the row-pattern form (pair / master / march forms dropped)
void drop_pair_forms(amg_mat *A)
{
   dfree(A->ppat), dfree(A->pptab), dfree(A->pbase), dfree(A->pdelta), dfree(A->mpmask), dfree(A->mpval);
   A->pp_n = A->pp_stride = A->pp_centre0 = 0;
   A->mp_J = A->mp_uni = 0;
   A->mz_P = A->mz_S = A->mz27 = 0;
   A->mz_dom = -1;
   A->mz_xlo = A->mz_xhi = -1;
}

void drop_bsr3(amg_mat *A)
{
   dfree(A->soff), dfree(A->bcol), dfree(A->bdiag), dfree(A->bmode), dfree(A->bvi), dfree(A->bval);
   A->bsr3 = 0;
}

} // namespace

void amg_mat_drop_forms(amg_mat *A)
{
   drop_bsr3(A);
   drop_pair_forms(A);
   drop_row_pattern(A);
   drop_dict_index(A);
   drop_value_index(A);
}

int amg_mat_finish(amg_mat *A)
{
   hipStream_t s = A->ctx->stream;
   amgk::extract_diag(s, A);
   AMG_HIP(hipGetLastError());
   {
      DBuf<int> d;
      AMG_TRY(d.alloc(2));
      AMG_HIP(hipMemsetAsync(d, 0, 2 * sizeof(int), s));
      amgk::row_max(s, A, d);
      amgk::diag_uniform(s, A, d.p + 1);
      int h[2] = {0, 0};
      double d0 = 0.0;
      AMG_HIP(hipMemcpyAsync(h, d, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
      if (A->nrows > 0) AMG_HIP(hipMemcpyAsync(&d0, A->diag, sizeof(double), hipMemcpyDeviceToHost, s));
      AMG_HIP(hipStreamSynchronize(s));
      A->maxrow = h[0];
      A->diag_uni = A->nrows > 0 && h[1] == 0;
      A->diag_u = d0;
   }
   if (A->ctx->value_index && A->nnz > 0) AMG_TRY(build_value_index(A));
   if (A->ctx->dict_index && A->vidx) AMG_TRY(build_dict_index(A));
   if (A->ctx->row_pattern && A->didx) AMG_TRY(build_row_pattern(A));
   const bool pp = A->dc_maxrow <= 8 || A->nrows >= AMG_PP_LONG_MIN_ROWS || A->ctx->pair_pattern == 2;
   // long-row operators below the pair-coding size still try the 27-pt march
   // (kept only if it applies: the pair kernel itself is slower there)
   const bool try27 = !pp && A->ctx->plane_march && A->ctx->master_pattern;
   if (A->ctx->pair_pattern && A->rpat && A->dc_maxrow <= AMG_PP_MAXROW && (pp || try27))
      AMG_TRY(build_pair_pattern(A));
   if (A->ctx->master_pattern && A->ppat) AMG_TRY(build_master_pattern(A));
   if (try27 && A->ppat && !A->mz27 && !A->pbase) drop_pair_forms(A);
   return AMG_OK;
}

// 3x3 block form of a square, diagonal-first operator with num_functions = 3
// (dofs byVDIM: rows 3t..3t+2 are the three components of node t, e.g. the
// DMEM elasticity problem, DMEM_BuildMatrix.cpp:442-719): block row t is
// blocked when its three rows hold exactly the columns 3j..3j+2 of the same
// node set {j} -- each row diagonal first, then ascending, so walking the
// blocks (ascending j, components ascending) with the diagonal taken first
// adds every row's products in its CSR order (bit-identical).  Other block
// rows (the identity rows of fixed dofs) keep the CSR form.  Used only when
// at least 90% of the block rows are blocked.  From the host CSR of a finished
// matrix whose stream is synchronised (amg_csr_register).
int amg_mat_build_bsr3(amg_mat *A, const int *rowptr, const int *col, const double *val)
{
   const int n = A->nrows, nb = n / 3;
   if (!A->ctx->bsr3 || n % 3 || n != A->ncols || !A->diag_first || n < 3 || A->nnz < 24LL * n) return AMG_OK;
   std::vector<int> bptr(nb + 1, 0), bdiag(nb, -1), bcol;
   std::vector<unsigned char> mode(nb, 1);
   std::vector<long long> src; // CSR position of every block entry (row-major 3x3), -1 unused
   std::vector<int> js;
   long long blocked = 0;
   for (int t = 0; t < nb; t++) {
      bptr[t + 1] = bptr[t];
      const int r0 = 3 * t;
      const int len = rowptr[r0 + 1] - rowptr[r0];
      if (len < 3 || len % 3) continue;
      bool ok = true;
      js.clear();
      for (int c = 0; c < 3 && ok; c++) {
         const int r = r0 + c, b = rowptr[r], e = rowptr[r + 1];
         ok = e - b == len && col[b] == r;
         // the row minus its diagonal, ascending, with the diagonal reinserted
         // at its sorted place: 3j, 3j+1, 3j+2 per node j
         int prev = -1, k = b + 1;
         std::vector<int> cols;
         cols.reserve(len);
         bool ins = false;
         for (int q = 0; q < len - 1 && ok; q++, k++) {
            const int cc = col[k];
            if (!ins && r < cc) cols.push_back(r), ins = true;
            ok = cc > prev && cc != r;
            prev = cc;
            cols.push_back(cc);
         }
         if (!ins) cols.push_back(r);
         for (int q = 0; q < len && ok; q += 3) {
            ok = cols[q] % 3 == 0 && cols[q + 1] == cols[q] + 1 && cols[q + 2] == cols[q] + 2;
            if (ok && c == 0) js.push_back(cols[q] / 3);
            if (ok && c > 0) ok = js[q / 3] == cols[q] / 3;
         }
      }
      if (!ok) continue;
      mode[t] = 0;
      blocked++;
      for (size_t q = 0; q < js.size(); q++) {
         if (js[q] == t) bdiag[t] = bptr[t + 1];
         bcol.push_back(js[q]);
         bptr[t + 1]++;
      }
      if (bdiag[t] < 0) return AMG_OK; // unreachable: every row holds its diagonal
      // CSR positions: row r's entry for column 3j + cc
      const size_t base = src.size();
      src.resize(base + js.size() * 9, -1);
      for (int c = 0; c < 3; c++) {
         const int r = r0 + c, b = rowptr[r], e = rowptr[r + 1];
         for (int k = b; k < e; k++) {
            const int j = col[k] / 3, cc = col[k] % 3;
            const size_t q = std::lower_bound(js.begin(), js.end(), j) - js.begin();
            src[base + q * 9 + 3 * c + cc] = k;
         }
      }
   }
   if (blocked * 10 < 9LL * nb) return AMG_OK;
   // sliced layout (21 block rows per slice -- a lane per row -- or, value-indexed
   // with ctx->bsr3 == 2, 64 -- a lane per block row; padded to the slice's longest)
   const int SL = A->ctx->bsr3 == 2 && A->vidx ? 64 : 21;
   const int ns = (nb + SL - 1) / SL;
   std::vector<long long> soff(ns + 1, 0);
   for (int sl = 0; sl < ns; sl++) {
      int w = 0;
      for (int t = sl * SL; t < std::min(nb, (sl + 1) * SL); t++) w = std::max(w, bptr[t + 1] - bptr[t]);
      soff[sl + 1] = soff[sl] + (long long)w * SL;
   }
   const size_t nslot = (size_t)soff[ns];
   std::vector<int> scol(std::max<size_t>(nslot, 1), 0), bdk(nb, 0);
   std::vector<unsigned char> bcnt(nb, 0);
   for (int t = 0; t < nb; t++) {
      const int cnt = bptr[t + 1] - bptr[t];
      if (cnt > 255) return AMG_OK; // block rows of more than 255 blocks: keep CSR
      bcnt[t] = mode[t] ? 0 : (unsigned char)cnt;
      bdk[t] = mode[t] ? 0 : bdiag[t] - bptr[t];
      const int sl = t / SL, q = t % SL;
      const int w = (int)((soff[sl + 1] - soff[sl]) / SL);
      for (int k = 0; k < w; k++) scol[(size_t)soff[sl] + (size_t)k * SL + q] = k < cnt ? bcol[bptr[t] + k] : t;
   }
   // slot of block k of block row t
   auto slot = [&](int t, int k) { return (size_t)soff[t / SL] + (size_t)k * SL + t % SL; };
   // block entries as indices into the value table (3 rows x 4 bytes), or as fp64
   std::vector<unsigned int> bvi;
   std::vector<double> bv;
   if (A->vidx) {
      std::vector<double> tab(256);
      AMG_HIP(hipMemcpy(tab.data(), A->vtab, 256 * sizeof(double), hipMemcpyDeviceToHost));
      std::vector<unsigned long long> keys(A->vi_n);
      std::memcpy(keys.data(), tab.data(), A->vi_n * 8);
      bvi.assign(std::max<size_t>(nslot * 3, 1), 0);
      for (int t = 0; t < nb; t++)
         for (int k = 0; k < bptr[t + 1] - bptr[t]; k++)
            for (int q = 0; q < 9; q++) {
               const long long sp = src[(size_t)(bptr[t] + k) * 9 + q];
               if (sp < 0) continue;
               unsigned long long b;
               std::memcpy(&b, &val[sp], 8);
               const size_t idx = std::lower_bound(keys.begin(), keys.end(), b) - keys.begin();
               bvi[slot(t, k) * 3 + q / 3] |= (unsigned int)idx << (8 * (q % 3));
            }
   } else {
      bv.assign(std::max<size_t>(nslot * 9, 1), 0.0);
      for (int t = 0; t < nb; t++)
         for (int k = 0; k < bptr[t + 1] - bptr[t]; k++)
            for (int q = 0; q < 9; q++) {
               const long long sp = src[(size_t)(bptr[t] + k) * 9 + q];
               if (sp >= 0) bv[slot(t, k) * 9 + q] = val[sp];
            }
   }
   hipStream_t s = A->ctx->stream;
   DBuf<long long> d_soff;
   DBuf<int> d_bcol, d_bdiag;
   DBuf<unsigned char> d_bmode;
   DBuf<unsigned int> d_bvi;
   DBuf<double> d_bval;
   if (!d_soff.try_alloc(ns + 1) || !d_bcol.try_alloc(scol.size()) || !d_bdiag.try_alloc(nb) || !d_bmode.try_alloc(nb) ||
       (A->vidx ? !d_bvi.try_alloc(bvi.size()) : !d_bval.try_alloc(bv.size())))
      return AMG_OK; // not enough room: keep the CSR forms
   if (A->vidx)
      AMG_HIP(hipMemcpyAsync(d_bvi, bvi.data(), bvi.size() * 4, hipMemcpyHostToDevice, s));
   else
      AMG_HIP(hipMemcpyAsync(d_bval, bv.data(), bv.size() * 8, hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(d_soff, soff.data(), (ns + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(d_bcol, scol.data(), scol.size() * sizeof(int), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(d_bdiag, bdk.data(), nb * sizeof(int), hipMemcpyHostToDevice, s));
   AMG_HIP(hipMemcpyAsync(d_bmode, bcnt.data(), nb, hipMemcpyHostToDevice, s));
   AMG_HIP(hipStreamSynchronize(s));
   A->soff = d_soff.take();
   A->bcol = d_bcol.take();
   A->bdiag = d_bdiag.take();
   A->bmode = d_bmode.take();
   A->bvi = d_bvi.take();
   A->bval = d_bval.take();
   A->bsl = SL;
   A->bsr3 = A->vidx ? 1 : 2;
   return AMG_OK;
}

// ---------------------------------------------------------------------------
// the forms' switches (every setter bumps knob_gen: cached hipGraphs were
// captured with the old setting) and what a registered matrix took
// ---------------------------------------------------------------------------
extern "C" int amg_set_value_index(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_value_index: null context");
   c->knob_gen++;
   c->value_index = enable ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_value_index(const amg_mat *A) { return A ? A->vi_n : 0; }

extern "C" int amg_set_dict_index(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_dict_index: null context");
   c->knob_gen++;
   c->dict_index = enable ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_dict_index(const amg_mat *A) { return A ? A->dc_n : 0; }

extern "C" int amg_set_row_pattern(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_row_pattern: null context");
   c->knob_gen++;
   c->row_pattern = enable ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_row_pattern(const amg_mat *A) { return A ? A->rp_n : 0; }

extern "C" int amg_set_pair_pattern(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_pair_pattern: null context");
   c->knob_gen++;
   c->pair_pattern = enable < 0 ? 0 : enable > 2 ? 2 : enable;
   return AMG_OK;
}

extern "C" int amg_mat_pair_pattern(const amg_mat *A) { return A ? A->pp_n : 0; }

extern "C" int amg_set_pair_anchor16(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_pair_anchor16: null context");
   c->knob_gen++;
   c->pair_anchor16 = enable ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_pair_anchor16(const amg_mat *A) { return (A && A->pdelta) ? 1 : 0; }

extern "C" int amg_set_master_pattern(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_master_pattern: null context");
   c->knob_gen++;
   c->master_pattern = enable ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_master_pattern(const amg_mat *A) { return A ? A->mp_J * (A->mp_uni ? -1 : 1) : 0; }

extern "C" int amg_set_plane_march(amg_ctx *c, int enable, int zc, int xcd)
{
   AMG_ARG(c, "amg_set_plane_march: null context");
   AMG_ARG(zc >= -1 && zc <= 64, "amg_set_plane_march: planes per chunk %d outside [1, 64] (0: keep, -1: auto)",
           zc);
   c->knob_gen++;
   c->plane_march = enable ? 1 : 0;
   if (zc > 0) c->mz_zc = zc, c->mz_zc_auto = 0;
   if (zc == -1) c->mz_zc = 16, c->mz_zc_auto = 1;
   if (xcd >= 0) c->mz_xcd = xcd ? 1 : 0;
   return AMG_OK;
}

extern "C" int amg_mat_plane_march(const amg_mat *A) { return A ? A->mz_P : 0; }

extern "C" int amg_mat_march_points(const amg_mat *A) { return (A && A->mz_P) ? (A->mz27 ? 27 : 7) : 0; }

extern "C" int amg_set_bsr3(amg_ctx *c, int enable)
{
   AMG_ARG(c, "amg_set_bsr3: null context");
   c->knob_gen++;
   c->bsr3 = enable == 2 ? 2 : (enable ? 1 : 0);
   return AMG_OK;
}

extern "C" int amg_mat_bsr3(const amg_mat *A) { return A ? A->bsr3 : 0; }

extern "C" int amg_mat_bsr3_slice(const amg_mat *A) { return A && A->bsr3 ? A->bsl : 0; }

extern "C" int amg_mat_bsr3_counts(const amg_mat *A, unsigned char *out)
{
   AMG_ARG(A && out, "amg_mat_bsr3_counts: null argument");
   AMG_ARG(A->bsr3 && A->bmode, "amg_mat_bsr3_counts: the matrix is not in 3x3 block form");
   AMG_HIP(hipStreamSynchronize(A->ctx->stream));
   AMG_HIP(hipMemcpy(out, A->bmode, (size_t)(A->nrows / 3), hipMemcpyDeviceToHost));
   return AMG_OK;
}
