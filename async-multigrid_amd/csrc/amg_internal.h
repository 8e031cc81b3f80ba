// amg_internal.h -- shared internals of libamg_mi355x (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <limits>
#include <memory>
#include <vector>

#include "amg_mi355x.h"

// ---------------------------------------------------------------------------
// error plumbing: every C-ABI entry returns AMG_OK or a negative status and
// leaves a thread-local message for amg_last_error().
// ---------------------------------------------------------------------------
int amg_set_error(int code, const char *fmt, ...);

#define AMG_HIP(call)                                                                      \
   do {                                                                                    \
      hipError_t _e = (call);                                                              \
      if (_e != hipSuccess)                                                                \
         return amg_set_error(AMG_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,   \
                              hipGetErrorString(_e));                                      \
   } while (0)

#define AMG_TRY(call)                                                                      \
   do {                                                                                    \
      int _s = (call);                                                                     \
      if (_s != AMG_OK) return _s;                                                         \
   } while (0)

#define AMG_ARG(cond, ...)                                                                 \
   do {                                                                                    \
      if (!(cond)) return amg_set_error(AMG_ERR_ARG, __VA_ARGS__);                         \
   } while (0)

// rows handled by one workgroup of the CSR tile kernels (one row per lane)
constexpr int AMG_TILE_ROWS = 256;
// products staged per LDS chunk in the CSR tile kernels (16 KiB of fp64)
constexpr int AMG_CHUNK = 2048;
// device arrays of col/val are padded so 16-byte vector loads past nnz stay in bounds
constexpr int AMG_NNZ_PAD = 8;
// longest row the dictionary-coded kernel stages in LDS
constexpr int AMG_DC_MAXROW = 32;
// bytes per row pattern of the row-pattern-coded form: length + entries (x4 aligned)
constexpr int AMG_RP_STRIDE = 36;
// paired row patterns (rows 2t, 2t+1 of operators whose rows hold <= 32
// entries): one header word + up to 2 * maxrow merged entry words per pair
// pattern, maxrow = 8 (7-pt) or 32 (27-pt Galerkin); the table must fit
// AMG_PP_LDS bytes of LDS
constexpr int AMG_PP_MAXROW = 32;
constexpr int AMG_PP_LDS = 32 * 1024;
// rows of > 8 entries are pair-coded from this size up (a pair lane walks
// twice the entries: latency-bound grids below it run faster one row per lane)
constexpr int AMG_PP_LONG_MIN_ROWS = 1 << 22;
inline int amg_pp_stride(int maxrow) { return 1 + 2 * (maxrow <= 8 ? 8 : AMG_PP_MAXROW); }

// anchored operators (interpolation, restriction): row 2t+1's anchor minus
// row 2t's, + AMG_PP_DA0, must lie in [0, AMG_PP_NDA)
constexpr int AMG_PP_NDA = 16;
constexpr int AMG_PP_DA0 = 8;
constexpr int AMG_PP_NK = 256 * 257 * AMG_PP_NDA; // pair keys
// pair-coded only if the merged lists are at most this factor longer than the
// longer row of each pair (summed over all row pairs)
constexpr double AMG_PP_MAXFILL = 1.15;
// paired kernel epilogue form (csr_rpp_kernel OPT, tools/tune_spmv.py ABL_jac_o*):
// bit 1 = a_ii from the header word
constexpr int AMG_RPP_OPT = 2;
// master-pattern form: longest master list, LDS budget of the per-pattern
// value table (pp_n * J * 16 bytes)
constexpr int AMG_MP_MAXJ = 32;
constexpr int AMG_MP_LDS = 48 * 1024;

struct amg_transport; // amg_dist.cpp: RCCL communicator or host-callback test transport

struct amg_ctx {
   amg_transport *xport = nullptr;
   long long replicate_rows = 1LL << 18;
   int device = 0;
   hipStream_t stream = nullptr;           // compute stream (all sync work)
   std::vector<hipStream_t> level_streams; // async additive: one per level
   hipStream_t comm_stream = nullptr;      // halo exchange (distributed)
   double *d_partials = nullptr;           // per-workgroup partial sums
   size_t partials_cap = 0;
   double *d_scalars = nullptr;            // device scalars (norms, dots)
   int *d_err = nullptr;                   // device-side range-check flags (amg_device_errors)
   double *h_pinned = nullptr;             // pinned host mirror of scalars
   int num_cus = 256;
   int wall_khz = 100000;  // device wall clock (wall_clock64) rate, for injected delays
   int value_index = 1; // build value-indexed CSR for matrices with <= 256 distinct values
   int dict_index = 1;  // build dictionary-coded CSR for stencil-like square operators
   int row_pattern = 1; // build row-pattern-coded CSR on top of the dictionary
   int pair_pattern = 1; // paired-row-pattern CSR: 0 off, 1 size-gated for long rows, 2 always
   int master_pattern = 1; // master-pattern form of square pair-coded operators
   int pair_anchor16 = 0;  // slab-compressed anchors of pair-coded P/R (measured slower: off)
   int plane_march = 1;    // plane-marching kernel for 7-pt box-grid masters (csr_mz_kernel)
   int mz_zc = 16;         // planes per workgroup chunk of the plane-marching kernel
   int mz_edge = 1;        // x-edge pair patterns on the 27-pt march's fast path
   int mz_zc_auto = 1;     // shorten the chunks of small levels to keep >= 2048 workgroups
   // 27-pt march: chunks sized so the grid is one round of resident
   // workgroups (mz27_occ > 0: workgroups per CU; 0: mz_chunk's rule) and the
   // prefetch distance in planes (1 or 2)
   // (> 0: that many per CU; < 0: the kernel's own occupancy from the runtime)
   int mz27_occ = -1;
   int mz_occ = 0; // the same for the 7-pt march (AMG_MZ_OCC; 0: mz_chunk's rule)
   int mz_pf = 3;  // 7-pt march prefetch distance in planes (AMG_MZ_PF: 1 or 2; 3: 1 + halo operands and rhs ahead)
   int mz27_pf = 2;
   int mz_xcd = 1;         // XCD-contiguous workgroup order of the plane-marching kernel
   int fuse_transfer = 1;  // fused level-0 residual + restriction on geometric hierarchies
   int bsr3 = 2;           // 3x3 block form of num_functions = 3 operators (1: lane per row; 2: lane per block row when value-indexed)
   unsigned knob_gen = 0;  // bumped by every amg_set_* knob: captured hipGraphs older than it are dropped
   int graphs = 0;         // hipGraphs of the additive cycles' launch-bound loops (AMG_GRAPHS)
   int fuse_xfer = 1;      // composed smoothed transfers of marched 7-pt levels in one pass each
   int fuse_xfp_slab = 0;  // ... and the slab async solve's fused prolongation + atomic (AMG_FUSE_XFP_SLAB)
   int fuse_prolong = 0;   // prolongation fused into the first post sweep (measured slower: off)
   int bsr3_xs = 1;        // 3x3 block kernel: one x load per lane, shared over the triplet (AMG_BSR3_XS)
   int fuse_outer = 4;     // level 0's last post sweep + the outer residual as one march (AMG_FUSE_OUTER;
                           // 1: u' stored every step, 2: only at the end of an iterate batch;
                           // 3: the two sweeps slab by slab over z through the Infinity Cache, u' as in 2;
                           // 4: the register march mz_two_sweep_kernel, u' as in 2)
   int outer_slab = 32;    // planes per z-slab of fuse_outer 3 (AMG_OUTER_SLAB): a slab's u, f and u'
                           // (3 x 32 x 2 MB at 512^2 planes) stay in the 256 MiB Infinity Cache
   int rr_lines = 1;       // coarse lines per lane of the fused residual + restriction (1 or 2)
   int mz_lines = 1;       // 7-pt plane march: lines per lane (1, 2 or 4, AMG_MZ_LINES)
   int mz_lines_gemv = 2;  // the same for SpMV / SpGEMV (AMG_MZ_LINES_GEMV; 2: -8 % on the 512^3 SpMV)
   int mz_nt = 0;          // streaming hints on > 512 MB levels: 1 NT stores, 2 NT rhs loads
   int rr_ring = 0;        // wave-edge residuals through a flag-ordered LDS ring (measured slower: off)
   int rr_occ = 0;         // 5: the fused residual + restriction compiled for 5 waves / SIMD
   int rr_fpf = 0;         // 1: its right-hand side a fine plane ahead (AMG_RR_FPF)
   int long_form = 0;      // long-row CSR kernel: 0 workgroup chunks (csr_long_kernel), 1 / 2 wave-independent
                           // chunks of 8 / 16 entries per lane (csr_longw_kernel; AMG_LONG_FORM)
   int long_xcd = 1;       // ... with XCD-contiguous row blocks (AMG_LONG_XCD)
   int rr_zc = 0;          // coarse planes per chunk of the fused residual + restriction (0: mz_zc / 2)
   int jgs_wave = 1;       // hybrid JGS form: 1 8 blocks per wave, 2 one wave per block, 0 one lane per block, 3 LDS tile
   int jgs_small = 2;      // small levels' hybrid JGS form (amg_set_jgs_small)
   int jgs_fold = 0;       // FULL_ASYNC level-0 correction folded into the last JGS sweep (amg_set_jgs_fold)
};

struct amg_mat {
   amg_ctx *ctx = nullptr;
   int nrows = 0, ncols = 0;
   long long nnz = 0;
   int *rowptr = nullptr;
   int *col = nullptr;
   double *val = nullptr;
   double *diag = nullptr; // val[rowptr[i]] (the reference's a_ii; the zero pad after the last row)
   int diag_first = 1;
   int maxrow = -1;          // longest row (amg_mat_finish)
   amg_mat *trans = nullptr; // lazily built transpose for amg_matvec_t
   // value-indexed form (the hot kernels' format when the matrix has at most
   // 256 distinct values): vidx[k] indexes vtab (256 doubles, sorted by bits)
   unsigned char *vidx = nullptr;
   double *vtab = nullptr;
   int vi_n = 0;
   // dictionary-coded form (operators whose (col - anchor, value) pairs fit
   // 256 entries and whose rows hold <= AMG_DC_MAXROW entries; the anchor of a
   // row is its first column -- the row itself for diag-first square operators,
   // then danch is null): col = anchor + doff[didx[k]], a_ik = dval[didx[k]]
   unsigned char *didx = nullptr;
   int *doff = nullptr;
   double *dval = nullptr;
   int *danch = nullptr;
   int dc_n = 0;
   int dc_maxrow = 0; // longest row (selects the LDS staging size)
   // row-pattern-coded form (dictionary-coded operators with <= 256 distinct
   // rows, none empty): rpat[i] names row i's dictionary sequence in ptab
   // (AMG_RP_STRIDE bytes per pattern: length, then the entries)
   unsigned char *rpat = nullptr;
   unsigned char *ptab = nullptr;
   int rp_n = 0;
   // paired-row-pattern form (row-pattern-coded operators with rows of <= 32
   // entries and <= 256 distinct (pattern of row 2t, pattern of row 2t+1,
   // anchor delta) pairs): ppat[t] names the pair's merged entry list in
   // pptab (pp_stride words per pair: header nel | first entry of row 2t << 8
   // | of row 2t+1 << 16 | row 2t+1 present << 24 | (da + 16) << 25, then
   // entries d0 | d1 << 8 | has0 << 16 | has1 << 17).  An entry present in
   // both rows reads x[base + off], x[base + off + 1] with one 16-byte load.
   unsigned char *ppat = nullptr;
   unsigned int *pptab = nullptr;
   int pp_n = 0;
   int pp_stride = 0; // words per pair pattern (amg_pp_stride)
   int pp_centre0 = 0; // every pair's first merged entry is both rows' diagonal
   // master-pattern form (square, diagonal-first pair-coded operators whose
   // rows are all ordered subsequences of one master list of column offsets:
   // the diagonal, then the offsets ascending).  The offsets are wave-uniform
   // kernel arguments; mpmask[p] holds pair pattern p's row-use bits (bit 2j:
   // row 2t uses master entry j, bit 2j+1: row 2t+1).  mp_uni: one value per
   // offset over the whole matrix (values are kernel arguments too), else
   // mpval[p * mp_J + j] = {row 2t's value, row 2t+1's value}.
   // slab-compressed anchors of pair-coded operators with an anchor array:
   // anchor(2t) = pbase[2t >> 9] + pdelta[t] (every 512-row slab's anchors
   // within 65535 of its least), 2 bytes per row pair instead of 4 per row
   int *pbase = nullptr;
   unsigned short *pdelta = nullptr;
   int mp_J = 0; // master length (0: not master-coded)
   int mp_uni = 0;
   // every row's diagonal (A->diag) is the same value diag_u (amg_mat_finish)
   int diag_uni = 0;
   double diag_u = 0.0;
   int mp_off[AMG_MP_MAXJ] = {};
   double mp_val[AMG_MP_MAXJ] = {};
   unsigned long long *mpmask = nullptr;
   double *mpval = nullptr;
   // plane-marching form (csr_mz_kernel): the master list is [0, -P, -S, -1, +1,
   // +S, +P] with P % 512 == 0 and nrows = nz * P (0: not applicable)
   int mz_P = 0, mz_S = 0;
   // 27-pt plane march (csr_mz27_kernel): master list [0, the 26 offsets
   // dz P + dy S + dx ascending]; mz_dom = the most frequent pair pattern that
   // uses every entry with one value per entry in both rows (-1: none), its
   // values in master order (wave-uniform fast path)
   int mz27 = 0;
   int mz_dom = -1;
   double mz_domval[27] = {};
   // x-edge pair patterns of the fast path: mz_xlo = row 2t at the box's low
   // x face (its dx = -1 entries unused, values the dominant ones), row 2t+1
   // dominant; mz_xhi = row 2t dominant, row 2t+1 at the high x face (dx = +1
   // unused, values mz_hival); -1: none
   int mz_xlo = -1, mz_xhi = -1;
   double mz_hival[27] = {};
   // 3x3 block form (num_functions = 3 operators, byVDIM): block row t = rows
   // 3t..3t+2 whose three rows hold the same block columns, each block dense;
   // bmode[t] = 1: the block row keeps the CSR form (identity rows of fixed
   // dofs, irregular rows).  Block values as value-table indices (bvi: 3 rows
   // x 4 bytes, the 4th unused) when the matrix is value-indexed, else fp64
   // (bval: 9 per block, row-major)
   // Sliced layout: slice s = block rows 21s..21s+20 (one wave), padded to
   // its longest block row; block k of the slice's block row q sits at slot
   // soff[s] + 21 k + q, so a wave's loads of block k are contiguous.
   // bcnt[t] = blocks of block row t (0: CSR form), bdiag[t] = its diagonal
   // block's index k
   int bsr3 = 0; // 1: value-indexed blocks, 2: fp64 blocks
   int bsl = 21; // block rows per slice: 21 (lane per row, bsr3_kernel) or 64 (lane per block row, bsr3_row_kernel)
   long long *soff = nullptr;
   int *bcol = nullptr, *bdiag = nullptr;
   unsigned char *bmode = nullptr;
   unsigned int *bvi = nullptr;
   double *bval = nullptr;
};

struct amg_vec {
   amg_ctx *ctx = nullptr;
   int n = 0;
   double *d = nullptr;
   bool owns = true;
};

// n x k fp64, row-major: element (i, j) at d[i * k + j]; k is 2, 4 or 8
struct amg_mvec {
   amg_ctx *ctx = nullptr;
   int n = 0, k = 0;
   double *d = nullptr;
};

// what the multi-vector cycle (amg_mrhs.cpp) reads of a hierarchy (amg_solver.cpp): the
// level operators, the L1 row norms, the options as they stand now, and the slot of the
// hierarchy's multi-vector state, which amg_hier_free hands to amg_mrhs_state_free
struct amg_mrhs_state;
struct amg_hier_level_view {
   const amg_mat *A, *P, *R;
   int n;
   const double *l1;
};
struct amg_hier_view {
   amg_ctx *ctx;
   int L;
   const amg_opts *o;
   amg_mrhs_state **mrhs;
   std::vector<amg_hier_level_view> lv;
};
void amg_hier_get_view(amg_hier *H, amg_hier_view *out);
void amg_mrhs_state_free(amg_mrhs_state *st);

// workspace
int amg_ctx_partials(amg_ctx *ctx, size_t n, double **out);
// device CSR allocation (+ diagonal extraction) for in-library builders
int amg_mat_create_device(amg_ctx *c, int nrows, int ncols, long long nnz, amg_mat **out);
// a matrix under construction: freed (amg_mat_free) unless released to the caller
struct amg_mat_deleter {
   void operator()(amg_mat *A) const { amg_mat_free(A); }
};
using amg_mat_ptr = std::unique_ptr<amg_mat, amg_mat_deleter>;
// the compressed forms (amg_format.hip): the diagonal and the ladder of forms of
// a matrix whose CSR arrays are on the device (or on their way there on the
// context's stream); the 3x3 block form from the host CSR of a finished matrix,
// the stream synchronised; every form's arrays freed (amg_mat_free)
int amg_mat_finish(amg_mat *A);
int amg_mat_build_bsr3(amg_mat *A, const int *rowptr, const int *col, const double *val);
void amg_mat_drop_forms(amg_mat *A);
// coarse sub-cycle of a hierarchy whose level 0 is an inner level of a larger
// one: f_dev -> level-0 correction (zero start, SMEM_Sync_Parfor_Vcycle from
// that level down); returns the level-0 iterate pointer in *u_dev
int amg_hier_subcycle(amg_hier *H, hipStream_t s, const double *f_dev, const double **u_dev);
// InitVectors: zero every level vector of H (start of a new solve)
int amg_hier_reset(amg_hier *H);
// every level's iterate u back to zero: the state one preconditioner
// application starts from (the coarsest iterate otherwise carries over)
int amg_hier_zero_iterates(amg_hier *H);

// ---------------------------------------------------------------------------
// kernel launchers (amg_kernels.hip); all asynchronous on stream s
// ---------------------------------------------------------------------------
namespace amgk {

// SMEM_SpGEMV branch selection (SMEM_MatVec.cpp:140-258)
struct Gemv {
   int init;     // 0: 0.0, 1: b, 2: -b, 3: b*temp, 4: -b*temp
   int negacc;   // 1: tempx -= a*x ; 0: tempx += a*x
   int scale;    // 1: y = alpha*tempx
   double alpha, temp;
};
Gemv gemv_mode(double alpha, double beta);

// y[rb,re) per the Gemv mode; if partials != nullptr also writes per-workgroup
// sum of y_i^2 to partials[0..nblocks) (fixed order)
void spgemv(hipStream_t s, const amg_mat *A, const double *x, const double *b, const Gemv &g,
            double *y, int rb, int re, double *partials);
// r = b - (A x) over [0, n): SMEM_Residual's y = A x; r = b - y (the sum
// rounded first, then subtracted) in one pass without y where A is
// dictionary-coded, else the two passes through y (bit-identical either way)
void residual_fsub(hipStream_t s, const amg_mat *A, const double *x, const double *b, double *y, double *r, int n);
int tile_blocks(int rb, int re);

// Jacobi sweep out[i] = x[i] + (omega*(f_i - sum a_ij x_j))/a_ii  (a_ii != 0)
//   l1 != nullptr: out[i] = x[i] + (f_i - sum)/l1[i]   (no a_ii test)
void jacobi_sweep(hipStream_t s, const amg_mat *A, const double *f, const double *x,
                  const double *l1, double omega, double *out, int rb, int re);
// outer residual r = f - A x fused with the next cycle's first Jacobi sweep on
// the same x: unext = x + w r / a_ii (l1: x + r / l1); partials of sum r_i^2
void residual_jacobi(hipStream_t s, const amg_mat *A, const double *f, const double *x,
                     const double *l1, double omega, double *r, double *unext, int rb, int re,
                     double *partials);
// level 0's last post-smoothing sweep and the outer residual + next first
// sweep as ONE plane march (7-pt master form, S = 512): u1out = u' (null: not
// stored), rout = r (null: not stored), unext = u'', partials of sum r_i^2
bool mz_sweep_outer_ok(const amg_mat *A);
void mz_sweep_outer(hipStream_t s, const amg_mat *A, const double *f, const double *u, double *u1out,
                    double *rout, double *unext, double omega, double *partials);
// zero-guess sweep: variant 0 (SMEM) u = omega*f/a (a != 0) | u = f/l1
//                   variant 1 (SEQ)  u += omega*f/a (a != 0) | u += f/l1 (a != 0)
void jacobi_zero(hipStream_t s, const double *diag, const double *f, const double *l1,
                 double omega, double *u, int rb, int re, int variant);
// u_new = u + (omega*r)/a (a != 0): Jacobi sweep from a precomputed residual
void jacobi_from_residual(hipStream_t s, const double *diag, const double *r, const double *l1,
                          double omega, double *u, int rb, int re);
// hybrid JGS: one wave (rows <= 32 entries) or one lane per block, blocks d_blk[0..nblk] (device), in place on u.
// apply_u (the LDS tile form only): the FULL_ASYNC correction of the sweep's result folded into its
// write-out -- apply_u += u by device-scope atomics, apply_priv = the value after it (atomic_correct);
// returns whether it was applied
bool hybrid_jgs(hipStream_t s, const amg_mat *A, const double *f, double *u, const double *u_prev,
                const int *d_blk, int nblk, const double *diag_scale, double weight, int zero,
                int reverse, double *apply_u = nullptr, double *apply_priv = nullptr,
                unsigned long long *stamp = nullptr);
// *d_out = max(*d_out, longest row of A)
void row_max(hipStream_t s, const amg_mat *A, int *d_out);
// asynchronous / semi-asynchronous Gauss-Seidel, one lane per block, live u
void async_gs(hipStream_t s, const amg_mat *A, const double *f, double *u, const int *d_blk, int nblk,
              int sweeps, int semi, int reverse);
// geometric transfers of a marched level (R_0 = P_0^T of an nx*ny*nz box):
// coarse K couples to fine 2K + d, d in {0,1,2}^3, weight w[dz*9 + dy*3 + dx]
struct GeoT {
   double w[27];
   int nx, ny, nz;
};
// *bad |= 1 unless every row of M equals the geometric form (mode 0: M = R,
// coarse rows; mode 1: M = P, fine rows): lengths, columns, value bits
// z-slab forms (rows / columns of an extended slab operator): local rows [rb, re)
// are global rows + row_g0, local columns global columns + col_g0 (re < 0: all rows)
void geo_check(hipStream_t s, const amg_mat *M, int mode, const GeoT &g, int *bad, int rb = 0, int re = -1,
               long long row_g0 = 0, long long col_g0 = 0);
// fc = R (f - A u) for a plane-marched A with geometric R, without the fine
// residual vector (bit-identical to the residual SpGEMV + R SpMV).  Slab form:
// coarse planes [Kb, Ke) (Ke < 0: all), u / f plane 0 = fine plane fz0 (A's
// rows are those vectors' planes), fc plane 0 = coarse plane cz0
// the coarse level's zero-guess Jacobi sweep folded into a restriction: where
// u != null, u[i] = w fc[i] / d[i] for d[i] != 0 (jacobi_zero variant 0, no L1)
struct ZeroGuess {
   const double *d = nullptr;
   double w = 0.0;
   double *u = nullptr;
   // indices the fold may write: [lo, hi) (hi < 0: unchecked); a write outside
   // is dropped and flagged in *err (amg_device_errors)
   long long lo = 0, hi = -1;
   int *err = nullptr;
};
void mz_residual_restrict(hipStream_t s, const amg_mat *A, const double *f, const double *u, const GeoT &g,
                          const double *wdev, double *fc, int Kb = 0, int Ke = -1, int fz0 = 0, int cz0 = 0,
                          ZeroGuess zg = ZeroGuess());
// f_c = R r for the checked geometric R of GeoT g (bit-identical to the SpMV);
// coarse planes [Kb, Ke), r plane 0 = fine plane fz0, fc plane 0 = coarse cz0
void geo_restrict(hipStream_t s, const GeoT &g, const double *wdev, const double *r, double *fc, int Kb = 0,
                  int Ke = -1, int fz0 = 0, int cz0 = 0, ZeroGuess zg = ZeroGuess());
// u += P e for the checked geometric P of GeoT g (bit-identical to the SpGEMV);
// fine planes [zb, ze), u plane 0 = fine plane fz0, e plane 0 = coarse cz0;
// assign: u = P e (the SpMV, alpha 1 beta 0)
void geo_prolong(hipStream_t s, const GeoT &g, const double *wdev, const double *e, double *u, int zb = 0,
                 int ze = -1, int fz0 = 0, int cz0 = 0, int assign = 0);
// DMEM_AddSmooth scale vectors: s = a_ii / w (1 where a_ii = 0) or the L1 row
// norm l1 (l1 != nullptr), ns = -s (DMEM_Setup.cpp:423-482)
void dmem_scale(hipStream_t s, const double *diag, const double *l1, double omega, double *sc, double *nsc, int n);
// the stream waits usec microseconds (device wall clock at wall_khz)
void delay(hipStream_t s, double usec, int wall_khz);
// u_out = first Jacobi (l1 == nullptr) / L1 Jacobi sweep of A on uc = u + P e,
// P the checked geometric transfer of marched 7-pt level A (uc never stored)
void mz_prolong_sweep(hipStream_t s, const amg_mat *A, const double *f, const double *u, const double *ec,
                      const GeoT &g, const double *wdev, const double *l1, double omega, double *uout);
// composed smoothed transfers of a marched 7-pt level with geometric R / P in
// one pass each (bit-identical to xfer_div + SpMV + xfer_sub + R, and to
// P + SpMV + xfer_corr): rc = R (r + (-w) A (r ./ a)) (uniform operators only);
// ef = P ec + (-w) (A P ec) ./ a, then mode 0: out = ef; 1: atomic_correct(out =
// u, ef, u_priv); 2: out = u + ef
void mz_xfer_restrict(hipStream_t s, const amg_mat *A, const double *r, const GeoT &g, const double *wdev,
                      double omega, double *rc, int Kb = 0, int Ke = -1, int fz0 = 0, int cz0 = 0);
void mz_xfer_prolong(hipStream_t s, const amg_mat *A, const double *ec, const GeoT &g, const double *wdev,
                     double omega, int mode, double *out, double *u_priv, int zlo = 0, int zhi = -1, int fz0 = 0,
                     int cz0 = 0, unsigned long long *stamp = nullptr);
// transpose-product with the expansion-buffer order of T static chunks
void matvec_t_chunked(hipStream_t s, const amg_mat *AT, const double *x, double *y, int n_src,
                      int T);

// vector kernels
void vcopy(hipStream_t s, const double *x, double *y, int rb, int re);
void vset(hipStream_t s, double *y, double a, int rb, int re);
void vaxpy(hipStream_t s, double a, const double *x, double *y, int rb, int re);
void vivaxpy(hipStream_t s, const double *x, const double *sc, double *y, int rb, int re);
void vscale(hipStream_t s, double a, double *y, int rb, int re);
void vsub(hipStream_t s, const double *b, const double *y, double *r, int rb, int re); // r = b - y
// composed smoothed transfers: out = x ./ diag;  z = r + (-w) y;  e = e + (-w) (y ./ diag)
void xfer_div(hipStream_t s, const double *diag, const double *x, double *out, int rb, int re);
void xfer_sub(hipStream_t s, double w, const double *r, const double *y, double *z, int rb, int re);
void xfer_corr(hipStream_t s, double w, const double *y, const double *diag, double *e, int rb, int re);
void vadd_into(hipStream_t s, const double *r, double *u, int rb, int re, int overwrite);
void l1_norms(hipStream_t s, const amg_mat *A, double *out);
void a_diag(hipStream_t s, const double *diag, double omega, double *out, int n);
void extract_diag(hipStream_t s, const amg_mat *A);
// *d_flag = 1 unless every diag[i] has diag[0]'s bits
void diag_uniform(hipStream_t s, const amg_mat *A, int *d_flag);
// symmetric Jacobi pieces (SMEM_Smooth.cpp:665,682-683 / SEQ_Smooth.cpp:136,144-145)
void sym_scale(hipStream_t s, const double *diag, const double *l1, double omega, double *r,
               int rb, int re, int seq);
void sym_update(hipStream_t s, const double *diag, const double *l1, double omega, double *r,
                const double *y, double *u, int rb, int re, int seq, int overwrite);
// Chebyshev outer update SMEM_Solve.cpp:179-186
void cheby_update(hipStream_t s, double *u, double *u_outer, double *y_outer, double omega,
                  double delta, int n);
// DMEM_ChebyUpdate (DMEM_Misc.cpp:612-666) after the first cycle; branch 0 sync
// (d only), 1 async cheby_grid (d and u), 2 async other grid (u only)
void dmem_cheby_update(hipStream_t s, double *d, double *u, int n, int branch, double om1, double omd);
// DMEM_Mult accelerated update: x += e; d = first ? e : om1 d + omd e; x += d
void dmem_mult_accel(hipStream_t s, double *x, const double *e, double *d, int n, int first, double om1,
                     double omd);
// atomic correction: u += e (device-scope fp64 atomics), u_priv = value after the add
// stamp (nullable, every update kernel of a free race): stamp[0] = min, stamp[1] = max of the
// device wall clock over the kernel's workgroups -- its actual execution window (stamp_init)
void atomic_correct(hipStream_t s, double *u, const double *e, double *u_priv, int n,
                    unsigned long long *stamp = nullptr);
// stamps[0 .. 2n): starts ~0, ends 0
void stamp_init(hipStream_t s, unsigned long long *stamps, int n);
// serialised (SEMI_ASYNC) form: u += e; u_priv = u (u_priv may be null)
void semi_correct(hipStream_t s, double *u, const double *e, double *u_priv, int n);
// READ_RES: r -= y (atomic or serialised), r_priv = the updated value
void res_update(hipStream_t s, double *r, const double *y, double *r_priv, int n, int atomic,
                unsigned long long *stamp = nullptr);
// u[rb, re) += x[rb, re), device-scope atomics
void atomic_add(hipStream_t s, double *u, const double *x, int rb, int re);

// STREAM triad a = b + q c over n doubles (n even)
void stream_triad(hipStream_t s, double *a, const double *b, const double *c, double q, long long n);
// PMC calibration streams: mode 0/1/2/3 = read bytes with 16/8/4/1-byte lanes, 4 = 8-byte writes
void calib_stream(hipStream_t s, int mode, void *buf, long long bytes, double *out);

// deterministic reductions: red_blocks(n) workgroups of 256 lanes, lane t of
// workgroup b adding i = 256 b + t, += 256 gridDim, then block_sum_256's tree
inline int red_blocks(int n) { return std::max(1, std::min(1024, (n + 2047) / 2048)); }
// the workgroup's sum of one double per lane (256 lanes), valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double *lds4)
{
#pragma unroll
   for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
   const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
   __syncthreads();
   if (lane == 0) lds4[wid] = v;
   __syncthreads();
   double s = 0.0;
   if (threadIdx.x == 0) s = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
   return s;
}
void sumsq_partials(hipStream_t s, const double *x, int n, double *partials, int *nparts);
void abssum_partials(hipStream_t s, const double *x, int n, double *partials, int *nparts);
void dot_partials(hipStream_t s, const double *x, const double *y, int n, double *partials,
                  int *nparts);
// out[0] = sum(partials[0..np)) in fixed order; if do_sqrt, out[0] = sqrt(sum)
void reduce_partials(hipStream_t s, const double *partials, int np, double *out, int do_sqrt,
                     double *scratch);

// preconditioned CG (amg_pcg.hip): the device scalar block sc and the kernels
// that read and write it; np <= 1024 partials of the reduction grid
enum { PCG_RHO = 0, PCG_ALPHA = 1, PCG_BETA = 2, PCG_PQ = 3, PCG_RR = 4, PCG_RHO0 = 5, PCG_NSCALARS = 8 };
constexpr int PCG_RING = 4096; // alpha / beta / rho of the last PCG_RING iterations
// The finish of a dot product and the one definition of each quotient rule, shared by
// amg_pcg.hip and amg_eig.hip.
// sum of p[0..np) in sum_partials_k<<<1, 256>>>'s order (valid in thread 0)
__device__ __forceinline__ double pcg_sum_partials(const double *__restrict__ p, int np, double *lds4)
{
   double s = 0.0;
   for (int i = threadIdx.x; i < np; i += 256) s += p[i];
   return block_sum_256(s, lds4);
}

// the quotient rule (one thread).  alpha = rho / pq (0 where pq = 0: a zero
// right-hand side)
__device__ __forceinline__ void pcg_alpha_q(double pq, double *__restrict__ sc, double *__restrict__ ring_alpha)
{
   const double alpha = pq != 0.0 ? sc[PCG_RHO] / pq : 0.0;
   sc[PCG_PQ] = pq;
   sc[PCG_ALPHA] = alpha;
   if (ring_alpha) *ring_alpha = alpha;
}

// ||r|| = sqrt(rr) into *norm (null: not wanted); rho' = rz; beta = rho' / rho
// (0 where rho = 0); rho = rho'.  first: the start of a solve (rho only, kept in
// sc[PCG_RHO0] as well: the ring holds the later ones)
__device__ __forceinline__ void pcg_beta_q(double rr, double rz, double *__restrict__ sc,
                                           double *__restrict__ norm, double *__restrict__ ring_beta,
                                           double *__restrict__ ring_rho, int first)
{
   if (norm) *norm = sqrt(rr);
   sc[PCG_RR] = rr;
   if (!first) {
      const double rho = sc[PCG_RHO];
      const double beta = rho != 0.0 ? rz / rho : 0.0;
      sc[PCG_BETA] = beta;
      *ring_beta = beta;
      *ring_rho = rz;
   } else {
      sc[PCG_RHO0] = rz;
   }
   sc[PCG_RHO] = rz;
}

// pq = sum(part); sc[ALPHA] = sc[RHO] / pq (0 where pq = 0), also into *ring_alpha
void pcg_alpha(hipStream_t s, const double *part, int np, double *sc, double *ring_alpha);
// *norm = sqrt(sum(part_rr)); rho' = sum(part_rz); sc[BETA] = rho' / sc[RHO] (0 where
// rho = 0), sc[RHO] = rho', both also into the rings; first: sc[RHO] = rho' only
void pcg_beta(hipStream_t s, const double *part_rr, const double *part_rz, int np, double *sc, double *norm,
              double *ring_beta, double *ring_rho, int first);
// the zero-guess Jacobi sweep of a level's rows into a cleared u (jacobi_zero variant 0):
// u = w r / a for a != 0 and 0 elsewhere, or u = r / l1 under L1 Jacobi
struct PcgZero {
   double *u;          // null: no sweep
   const double *diag; // a_ii (null: the one value a)
   const double *l1;
   double a, w;
};
// x += sc[ALPHA] p; r -= sc[ALPHA] q; partials of r.r in dot_partials' order; zg.u != null:
// also that sweep on the new r
void pcg_update_xr(hipStream_t s, double *x, const double *p, double *r, const double *q, int n,
                   const double *sc, double *partials, int *nparts, const PcgZero &zg);
// across ranks: slot[0] = sum(part_a), slot[1] = sum(part_b) (null: one sum) in
// reduce_partials' order; after the all-gather of the slots, pcg_alpha / pcg_beta on the
// gathered values v (one per rank; (r.r, r.z) pairs for beta) added in rank order
void pcg_rank_sum(hipStream_t s, const double *part_a, const double *part_b, int np, double *slot);
void pcg_alpha_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *ring_alpha);
void pcg_beta_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *norm, double *ring_beta,
                    double *ring_rho, int first);
// p = z + sc[BETA] p
void pcg_update_p(hipStream_t s, const double *z, double *p, int n, const double *sc);

// ---- several right-hand sides at once (amg_mrhs.hip) ---------------------------------
// Every vector is n x K row-major (amg_mvec), K in {2, 4, 8}; per column the arithmetic
// of the single-vector launcher of the same name.  The row operators read A's plain CSR
// arrays (rowptr, col, val), once per launch for all K columns.
constexpr int MRHS_MAXK = 8;
inline bool mrhs_width_ok(int K) { return K == 2 || K == 4 || K == 8; }
// y[rb, re) per the Gemv mode; b may alias y, x may not
void mrhs_spgemv(hipStream_t s, int K, const amg_mat *A, const double *x, const double *b, const Gemv &g,
                 double *y, int rb, int re);
// out = x + (omega (f - A x)) / a_ii where a_ii != 0 (l1: x + (f - A x) / l1[i]), all rows
void mrhs_jacobi_sweep(hipStream_t s, int K, const amg_mat *A, const double *f, const double *x,
                       const double *l1, double omega, double *out);
// jacobi_zero variant 0 on n rows: u = omega f / a where a != 0 | u = f / l1
void mrhs_jacobi_zero(hipStream_t s, int K, const double *diag, const double *f, const double *l1, double omega,
                      double *u, int n);
void mrhs_set(hipStream_t s, double *y, double a, long long len);
void mrhs_set_col(hipStream_t s, int K, int j, const double *x, double *v, int n); // v(:, j) = x
void mrhs_get_col(hipStream_t s, int K, int j, const double *v, double *x, int n); // x = v(:, j)
struct MrhsScal {
   double a[MRHS_MAXK];
};
void mrhs_axpy(hipStream_t s, int K, const MrhsScal &alpha, const double *x, double *y, int n);
// column j's partials of x . y (y null: x . x) on dot_partials' grid at part[1024 j ..]
void mrhs_dot_partials(hipStream_t s, int K, const double *x, const double *y, int n, double *part, int *nparts);
// out[j] = the sum of column j's partials in reduce_partials' order (do_sqrt: its root)
void mrhs_reduce_partials(hipStream_t s, int K, const double *part, int np, double *out, int do_sqrt);
// the PCG scalar block of K columns: scalar q of column j at sc[MRHS_MAXK q + j]; the
// quotient rules are pcg_alpha_q / pcg_beta_q per column.  ring_*: column j's entry at
// ring_*[PCG_RING j]; norm: K contiguous values
void mrhs_pcg_alpha(hipStream_t s, int K, const double *part, int np, double *sc, double *ring_alpha);
void mrhs_pcg_beta(hipStream_t s, int K, const double *part_rr, const double *part_rz, int np, double *sc,
                   double *norm, double *ring_beta, double *ring_rho, int first);
// x += alpha_j p; r -= alpha_j q; the partials of r . r as mrhs_dot_partials lays them
void mrhs_pcg_update_xr(hipStream_t s, int K, double *x, const double *p, double *r, const double *q, int n,
                        const double *sc, double *part, int *nparts);
// p = z + beta_j p
void mrhs_pcg_update_p(hipStream_t s, int K, const double *z, double *p, int n, const double *sc);

// CG-Lanczos eigenvalue estimate (amg_eig.hip; the recurrence is amg_eig.h): CG on A
// preconditioned by its diagonal d (null: d = 1, no division), no right-hand side and no
// iterate.  sc is a PCG scalar block with gamma = r . (r ./ d) in sc[PCG_RHO]; p . q is
// finished by pcg_alpha / pcg_alpha_ranks
// *count += the rows whose d[i] is not positive (zero, negative or NaN)
void eig_count_bad_diag(hipStream_t s, const double *d, int n, int *count);
// p = r ./ d (first) or r ./ d + sc[BETA] p
void eig_update_p(hipStream_t s, const double *r, const double *d, double *p, int n, const double *sc, int first);
// q != null: r -= sc[ALPHA] q.  The partials of r . (r ./ d) from the r in registers, in
// dot_partials' order
void eig_update_r(hipStream_t s, double *r, const double *q, const double *d, int n, const double *sc,
                  double *partials, int *nparts);
// gamma' = sum(part): sc[BETA] = gamma' / sc[RHO] (0 where gamma = 0) into *ring_beta, sc[RHO] =
// gamma' into *ring_gamma; first: gamma_0 (no beta).  _ranks: on the gathered rank values v
void eig_gamma(hipStream_t s, const double *part, int np, double *sc, double *ring_beta, double *ring_gamma,
               int first);
void eig_gamma_ranks(hipStream_t s, const double *v, int nranks, double *sc, double *ring_beta,
                     double *ring_gamma, int first);

} // namespace amgk

// process-wide lock held by the teardown entry points (amg_api.cpp)
#include <mutex>
std::recursive_mutex &amg_teardown_mutex();
