// amg_async.h -- what the asynchronous additive solves and the measurement
// paths share (amg_solver.cpp, amg_dist*.cpp, amg_slab.cpp, amg_api.cpp; host
// only, not part of the C-ABI): the owning event, the timed-repetitions
// helper, the profiling log, the race records and the turn order of the
// deterministic schedules.  An AmgEvent destroys itself, so a function that
// returns early on an error leaks none.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <utility>

#include "amg_internal.h"

// HIP event destroyed with its owner (move-only); converts to hipEvent_t
struct AmgEvent {
   hipEvent_t e = nullptr;
   AmgEvent() = default;
   AmgEvent(AmgEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
   AmgEvent &operator=(AmgEvent &&o) noexcept
   {
      std::swap(e, o.e);
      return *this;
   }
   ~AmgEvent()
   {
      if (e) hipEventDestroy(e);
   }
   // no-op on an event that exists (members created on first use)
   int create(unsigned flags = hipEventDefault)
   {
      if (!e) AMG_HIP(hipEventCreateWithFlags(&e, flags));
      return AMG_OK;
   }
   operator hipEvent_t() const { return e; }
};

// *ms = the time of reps calls of body() (an int status) on stream s between
// two events, per call
template <class F>
int amg_timed_reps(hipStream_t s, int reps, F body, double *ms)
{
   AmgEvent a, b;
   AMG_TRY(a.create());
   AMG_TRY(b.create());
   AMG_HIP(hipEventRecord(a, s));
   for (int r = 0; r < reps; r++) AMG_TRY(body());
   AMG_HIP(hipEventRecord(b, s));
   AMG_HIP(hipEventSynchronize(b));
   float t = 0.f;
   AMG_HIP(hipEventElapsedTime(&t, a, b));
   *ms = (double)t / reps;
   return AMG_OK;
}

// per-category device times of a hierarchy's cycle (opts.profile): [0] fine
// residual / SpMV, [1] fine smoother, [2] R0, [3] P0, [4] outer residual
constexpr int AMG_PROF_NCAT = 5;
struct AmgProfLog {
   std::vector<std::pair<AmgEvent, AmgEvent>> pend[AMG_PROF_NCAT];
   double ms[AMG_PROF_NCAT] = {};
   long long n[AMG_PROF_NCAT] = {};
   // an event pair around the scope's launches on stream s, left pending
   struct Scope {
      AmgProfLog *log;
      int cat;
      hipStream_t s;
      AmgEvent a, b;
      Scope(AmgProfLog &log_, int cat_, hipStream_t s_, bool enabled) : log(enabled ? &log_ : nullptr), cat(cat_), s(s_)
      {
         if (log && a.create() == AMG_OK && b.create() == AMG_OK) hipEventRecord(a, s);
      }
      ~Scope()
      {
         if (!log) return;
         hipEventRecord(b, s);
         log->pend[cat].emplace_back(std::move(a), std::move(b));
      }
   };
   // the pending pairs into ms / n (waits for each pair's end)
   void drain()
   {
      for (int c = 0; c < AMG_PROF_NCAT; c++) {
         for (auto &p : pend[c]) {
            float t = 0.f;
            hipEventSynchronize(p.second);
            if (hipEventElapsedTime(&t, p.first, p.second) == hipSuccess) {
               ms[c] += t;
               n[c] += 1;
            }
         }
         pend[c].clear();
      }
   }
   void read(double *ms_out, long long *launches, int reset)
   {
      drain();
      for (int c = 0; c < AMG_PROF_NCAT; c++) {
         if (ms_out) ms_out[c] = ms[c];
         if (launches) launches[c] = n[c];
         if (reset) ms[c] = 0, n[c] = 0;
      }
   }
};

// AMG_SCHED_TIMED: the end time of a level's correction j (0-based) -- its
// recorded end times t (the replay of a measured race; past the table the
// last interval repeats) or, without a table, (j + 1) dur.  The oracle's
// timed_end (or_set_async_durations / or_set_async_times), the same doubles.
inline double amg_timed_end(const std::vector<double> &t, double dur, int j)
{
   const int n = (int)t.size();
   if (n == 0) return (double)(j + 1) * dur;
   if (j < n) return t[j];
   const double dt = n > 1 ? t[n - 1] - t[n - 2] : t[0];
   return t[n - 1] + (double)(j - n + 1) * dt;
}

// per-correction end events of a free race (one pool per level, grown on use)
// (the update point of correction j: its start event `record_start`, before
// the kernel that adds it into the shared iterate, and its end event `record`,
// after it -- a window in which other levels' updates may interleave row by row)
struct AmgCorrTimes {
   std::vector<std::vector<AmgEvent>> ev, ev0; // [level][correction]: update end / start
   std::vector<std::vector<double>> ms, ms0;   // [level][correction], after the solve
   static int rec(std::vector<AmgEvent> &v, int j, hipStream_t s)
   {
      while ((int)v.size() <= j) {
         AmgEvent e;
         if (e.create() != AMG_OK) return -1;
         v.push_back(std::move(e));
      }
      return hipEventRecord(v[j], s) == hipSuccess ? 0 : -1;
   }
   int record(int k, int j, hipStream_t s) { return rec(ev[k], j, s); }
   int record_start(int k, int j, hipStream_t s) { return rec(ev0[k], j, s); }
   void reset(int L)
   {
      ev.resize(L);
      ev0.resize(L);
      ms.assign(L, {});
      ms0.assign(L, {});
   }
   // elapsed ms of the first cnt[k] events of every level from t0
   int collect(hipEvent_t t0, const std::vector<int> &cnt)
   {
      ms.assign(ev.size(), {});
      ms0.assign(ev.size(), {});
      for (size_t k = 0; k < ev.size() && k < cnt.size(); k++)
         for (int j = 0; j < cnt[k] && j < (int)ev[k].size(); j++) {
            float m = 0.f;
            if (hipEventElapsedTime(&m, t0, ev[k][j]) != hipSuccess) return -1;
            ms[k].push_back(m);
            if (j < (int)ev0[k].size()) {
               if (hipEventElapsedTime(&m, t0, ev0[k][j]) != hipSuccess) return -1;
               ms0[k].push_back(m);
            }
         }
      return 0;
   }
   // device execution windows of the update kernels (stamp_begin / stamp_end
   // in the kernel that adds correction j of level k into the shared vector):
   // [k][j] start / end in ms of the device wall clock (an arbitrary origin
   // common to every stream and process on the device); NaN: not stamped.
   // Record of correction (k, j): 4 words -- window start, window end, the
   // device address of its per-row stamp array (0: none), unused.
   unsigned long long *d_st = nullptr;
   int st_cap = 0, st_L = 0;
   std::vector<std::vector<double>> w0, w1;
   // per-row update times (stamp_row: the low 32 bits of the device wall clock
   // at which row i's add + read of the shared vector completed) of the first
   // rows_j corrections of every level; rows_ms[k][j]: nrow times in ms, on the
   // window clock (empty: not recorded)
   unsigned *d_rows = nullptr;
   double *d_vals = nullptr; // per row: the value each add replaced and the value it left
   size_t rows_alloc = 0;
   int nrow = 0, rows_j = 0;
   std::vector<std::vector<std::vector<double>>> rows_ms, rows_vals;
   std::vector<unsigned long long> h_init;
   // row stamps are taken while nrow * L * rows_j * 20 B stays within this
   static constexpr size_t kRowBudget = (size_t)512 << 20;
   // koff[k]: the index of owned row 0 in the vector the update kernel of
   // level k indexes (a slab level-0 vector with its ghost planes in front)
   int stamps_begin(hipStream_t s, int L, int cap, int n_rows = 0, const std::vector<long long> &koff = {})
   {
      if (!d_st || L * cap > st_L * st_cap) {
         if (d_st) hipFree(d_st);
         d_st = nullptr;
         if (hipMalloc((void **)&d_st, (size_t)4 * L * cap * sizeof(unsigned long long)) != hipSuccess) return -1;
      }
      st_L = L;
      st_cap = cap;
      nrow = n_rows > 0 ? n_rows : 0;
      rows_j = nrow > 0 ? (int)std::min<size_t>(cap, kRowBudget / ((size_t)nrow * L * 20)) : 0;
      const size_t need = (size_t)nrow * L * rows_j;
      if (need > rows_alloc) {
         if (d_rows) hipFree(d_rows);
         if (d_vals) hipFree(d_vals);
         d_rows = nullptr;
         d_vals = nullptr;
         rows_alloc = 0;
         if (hipMalloc((void **)&d_rows, need * sizeof(unsigned)) != hipSuccess ||
             hipMalloc((void **)&d_vals, 2 * need * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            rows_j = 0;
         } else {
            rows_alloc = need;
         }
      }
      if (rows_j == 0) {
         // no row arrays: the records set on the device, in stream order (a
         // pageable host copy per solve serialises the ranks sharing a GPU)
         amgk::stamp_init(s, d_st, L * cap);
         return 0;
      }
      h_init.assign((size_t)4 * L * cap, 0ull);
      for (int k = 0; k < L; k++)
         for (int j = 0; j < cap; j++) {
            unsigned long long *w = &h_init[4 * ((size_t)k * cap + j)];
            w[0] = ~0ull;
            if (j < rows_j) {
               const long long o = k < (int)koff.size() ? koff[k] : 0;
               w[2] = (unsigned long long)(uintptr_t)(d_rows + ((size_t)k * rows_j + j) * nrow - o);
               w[3] = (unsigned long long)(uintptr_t)(d_vals + 2 * (((size_t)k * rows_j + j) * nrow - o));
            }
         }
      if (hipMemcpyAsync(d_st, h_init.data(), h_init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice,
                         s) != hipSuccess)
         return -1;
      if (rows_j > 0 && hipMemsetAsync(d_rows, 0, need * sizeof(unsigned), s) != hipSuccess) return -1;
      // NaN: a row whose update recorded no values (the no-return form)
      if (rows_j > 0 && hipMemsetAsync(d_vals, 0xff, 2 * need * sizeof(double), s) != hipSuccess) return -1;
      return 0;
   }
   unsigned long long *stamp(int k, int j) const
   {
      if (!(d_st && k >= 0 && k < st_L && j >= 0 && j < st_cap)) return nullptr;
      unsigned long long *p = d_st + 4 * ((size_t)k * st_cap + j);
      // low bit: the record carries row arrays (stamp_rows reads them only then)
      return (j < rows_j && nrow > 0) ? reinterpret_cast<unsigned long long *>(reinterpret_cast<uintptr_t>(p) | 1)
                                      : p;
   }
   // after the solve (the stream has finished): windows of the first cnt[k]
   // corrections of every level, and their row times where recorded
   int stamps_collect(const std::vector<int> &cnt, int wall_khz)
   {
      w0.assign(st_L, {});
      w1.assign(st_L, {});
      rows_ms.assign(st_L, {});
      rows_vals.assign(st_L, {});
      if (!d_st) return 0;
      std::vector<unsigned long long> h((size_t)4 * st_L * st_cap);
      if (hipMemcpy(h.data(), d_st, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
         return -1;
      const double tpm = wall_khz > 0 ? (double)wall_khz : 1e5; // ticks per ms
      // the host copy of a correction's row times only where rows were
      // recorded (nrow is the level-0 row count: a per-solve zero-filled
      // buffer of that size cost 12 % of config 3's asynchronous cycle)
      std::vector<unsigned> hr;
      if (rows_j > 0) hr.resize((size_t)nrow);
      for (int k = 0; k < st_L && k < (int)cnt.size(); k++)
         for (int j = 0; j < cnt[k] && j < st_cap; j++) {
            const unsigned long long a = h[4 * ((size_t)k * st_cap + j)], b = h[4 * ((size_t)k * st_cap + j) + 1];
            const bool ok = a != ~0ull && b != 0ull;
            w0[k].push_back(ok ? (double)a / tpm : std::numeric_limits<double>::quiet_NaN());
            w1[k].push_back(ok ? (double)b / tpm : std::numeric_limits<double>::quiet_NaN());
            if (!ok || j >= rows_j || nrow == 0) continue;
            if (hipMemcpy(hr.data(), d_rows + ((size_t)k * rows_j + j) * nrow, (size_t)nrow * sizeof(unsigned),
                          hipMemcpyDeviceToHost) != hipSuccess)
               return -1;
            // unwrap the low 32 bits around the window start (|dt| < 21 s)
            if ((int)rows_ms[k].size() != j) continue;
            std::vector<double> t((size_t)nrow);
            for (int i = 0; i < nrow; i++) {
               const int d = (int)(hr[i] - (unsigned)a);
               t[i] = ((double)a + (double)d) / tpm;
            }
            rows_ms[k].push_back(std::move(t));
            std::vector<double> v((size_t)2 * nrow);
            if (hipMemcpy(v.data(), d_vals + 2 * ((size_t)k * rows_j + j) * nrow, v.size() * sizeof(double),
                          hipMemcpyDeviceToHost) != hipSuccess)
               return -1;
            rows_vals[k].push_back(std::move(v));
         }
      return 0;
   }
   // per-row times of correction j of level k: nrow values, or 0 if not
   // recorded; vals: the 2 nrow (old, new) values instead
   int rows_of(int k, int j, double *out, int cap, bool vals = false) const
   {
      const auto &src = vals ? rows_vals : rows_ms;
      if (k < 0 || k >= (int)src.size() || j < 0 || j >= (int)src[k].size()) return 0;
      const int n = std::min(cap, (int)src[k][j].size());
      if (out) std::copy(src[k][j].begin(), src[k][j].begin() + n, out);
      return n;
   }
   ~AmgCorrTimes()
   {
      if (d_st) hipFree(d_st);
      if (d_rows) hipFree(d_rows);
      if (d_vals) hipFree(d_vals);
   }
};

// what an asynchronous solve is told about the race and what it records of
// it, the same for amg_hier and amg_dist_hier: the AMG_SCHED_TIMED level
// speeds (dur: per-level correction time; t: recorded end times, the replay),
// each level's finish and every correction's times of the last solve.  The
// copy-out methods take the C-ABI's cap (cap < 0: the start times or the row
// values, -cap entries) and `who`, the entry point named in error texts.
struct AmgRaceRecord {
   std::vector<double> dur;
   std::vector<std::vector<double>> t;
   std::vector<double> level_ms; // ms from the solve's start to each level's last correction
   AmgCorrTimes corr;
   bool timed_ready(int L) const { return (int)dur.size() >= L && (int)t.size() >= L; }
   int set_durations(const char *who, const double *ms, int L)
   {
      for (int k = 0; k < L; k++) AMG_ARG(ms[k] > 0.0, "%s: level %d: %g", who, k, ms[k]);
      dur.assign(ms, ms + L);
      t.assign(L, {});
      return AMG_OK;
   }
   int set_times(const char *who, const double *times, const int *n, int L)
   {
      t.assign(L, {});
      dur.assign(L, 1.0);
      for (int k = 0, off = 0; k < L; off += n[k], k++) {
         AMG_ARG(n[k] >= 0, "%s: level %d: %d entries", who, k, n[k]);
         t[k].assign(times + off, times + off + n[k]);
      }
      return AMG_OK;
   }
   static void copy_out(const std::vector<std::vector<double>> &vv, int level, double *ms, int cap, int *count)
   {
      const auto &v = level < (int)vv.size() ? vv[level] : std::vector<double>();
      *count = (int)v.size();
      for (int j = 0; j < (int)v.size() && j < cap && ms; j++) ms[j] = v[j];
   }
   void correction_ms(int level, double *ms, int cap, int *count) const
   {
      copy_out(cap < 0 ? corr.ms0 : corr.ms, level, ms, std::abs(cap), count);
   }
   void update_windows(int level, double *ms, int cap, int *count) const
   {
      copy_out(cap < 0 ? corr.w0 : corr.w1, level, ms, std::abs(cap), count);
   }
   void update_rows(int level, int j, double *ms, int cap, int *count) const
   {
      *count = corr.rows_of(level, j, ms, std::abs(cap), cap < 0);
   }
   int copy_level_ms(const char *who, double *ms, int L) const
   {
      AMG_ARG(!level_ms.empty(), "%s: no asynchronous solve yet", who);
      for (int k = 0; k < L; k++) ms[k] = level_ms[k];
      return AMG_OK;
   }
};

// The turn order of the deterministic schedules (the oracle's
// or_set_async_schedule): which level group takes the next whole correction.
// Groups [k_lo, k_hi) correct; groups [k_hi, ngroups) are idle (the
// reference's coarsest group under LOCAL residuals, whose correction is
// zero): they take their turns here, counted but never yielded.
//   FINEST_FIRST / COARSEST_FIRST: the groups one after another;
//   ROUND_ROBIN (and the free race's issue order under converge LOCAL): the
//     groups in turn, finest first, a stopped group skipped;
//   TIMED: the race at fixed level speeds -- group k's correction j ends at
//     amg_timed_end(t[k], dur[k], j); whole corrections in the order of their
//     end times, ties to the finer group.
// Converge LOCAL: a group stops after num_cycles corrections, its last is the
// num_cycles-th.  Converge GLOBAL (Misc.cpp:418-441): group k_lo raises the
// flag after its own update once every group, the idle ones too, has
// num_cycles (that update counted); a group stops at the first of its
// corrections that sees the flag, which is its last.  An idle group runs its
// turn after the last correcting group, so under round robin it has one
// correction fewer than the round's number when k_lo checks.
struct AmgAsyncTurns {
   int sched, k_lo, k_hi, ngroups, N;
   bool conv_global;
   const AmgRaceRecord &race;
   std::vector<int> cnt, stopped; // per group: corrections taken, stopped
   bool flag = false;
   int prev;
   AmgAsyncTurns(int sched_, int k_lo_, int k_hi_, int ngroups_, int num_cycles, bool conv_global_,
                 const AmgRaceRecord &race_)
      : sched(sched_), k_lo(k_lo_), k_hi(k_hi_), ngroups(std::max(k_hi_, ngroups_)), N(num_cycles),
        conv_global(conv_global_), race(race_), cnt(ngroups, 0), stopped(ngroups, !conv_global_ && num_cycles <= 0),
        prev(ngroups - 1)
   {
   }
   // the group whose turn it is (-1: every group has stopped)
   int pick() const
   {
      int best = -1;
      double tb = 0.0;
      for (int q = 0; q < ngroups - k_lo; q++) {
         int k = k_lo + q;
         if (sched == AMG_SCHED_COARSEST_FIRST) k = ngroups - 1 - q;
         if (sched == AMG_SCHED_ROUND_ROBIN || sched == AMG_SCHED_FREE) k = k_lo + (prev + 1 - k_lo + q) % (ngroups - k_lo);
         if (stopped[k]) continue;
         if (sched != AMG_SCHED_TIMED) return k;
         const double te = amg_timed_end(race.t[k], race.dur[k], cnt[k]);
         if (best < 0 || te < tb) best = k, tb = te;
      }
      return best;
   }
   // *k: the group to issue, *last: this correction is that group's last;
   // false: every group has stopped
   bool next(int *k_out, bool *last)
   {
      for (;;) {
         const int k = pick();
         if (k < 0) return false;
         bool raise = false;
         if (conv_global && k == k_lo && !flag) {
            raise = true;
            for (int l = k_lo; l < ngroups; l++)
               if (cnt[l] + (l == k ? 1 : 0) < N) raise = false;
         }
         *last = conv_global ? flag || raise : cnt[k] + 1 >= N;
         cnt[k]++;
         prev = k;
         if (raise) flag = true;
         if (conv_global ? flag : cnt[k] >= N) stopped[k] = 1;
         *k_out = k;
         if (k < k_hi) return true;
      }
   }
};
