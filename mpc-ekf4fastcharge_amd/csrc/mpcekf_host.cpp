// mpcekf_host.cpp -- C-ABI (include/mpcekf.h) over the gfx950 kernels.
//
// Owns: ROM validation (initKF.m:66-91, iterEKF.m:692-734, OB_step.m:140-158),
// the output-row permutation and LDS blobs, device state allocation, per-cell
// initialisation (initKF/initMPC/first OB_step), the fused step loop and the
// stage entry points.  No C++ exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mpcekf.h"
#include "mpcekf_aging.hpp"
#include "mpcekf_eig.hpp"
#include "mpcekf_kernels.hpp"
#include "mpcekf_balance.hpp"
#include "mpcekf_charger.hpp"
#include "mpcekf_pack.hpp"
#include "mpcekf_term.hpp"
#include "mpcekf_summary.hpp"
#include "mpcekf_thermal.hpp"
#include "mpcekf_thermal_sched.hpp"
#include "mpcekf_limit_map.hpp"
#include "mpcekf_thermal_couple.hpp"

using namespace mk;
namespace mk {
int launch_rows(const double *src, int64_t n, const int *rows, int k, double *dst, void *stream);  // mpcekf_io.hip
}

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) return fail(MPCEKF_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

constexpr int NCON_BUILT = 4 * 2 + 3 * 5;  // Np = 5, Nc = 2 compiled into the lane-per-cell kernels
int ncon_of(int Np, int Nc) { return 4 * Nc + 3 * Np; }  // constraintsMPC.m, all switches on
// initMPC.m's opts.constraints as the kernels' mask: bit 0 useCurrent, 1 useVoltage, 2 useEta
int sw_of(const mpcekf_config *c) { return (c->use_current ? 1 : 0) | (c->use_voltage ? 2 : 0) | (c->use_eta ? 4 : 0); }
// does all-on row i (of [Cu; -Cu; I; -I; G_v; -G_e; G_soc]) belong to an enabled block
bool row_enabled(int Np, int Nc, int sw, int i) {
  return i < 4 * Nc ? (sw & 1) != 0 : i < 4 * Nc + Np ? (sw & 2) != 0 : i < 4 * Nc + 2 * Np ? (sw & 4) != 0 : true;
}
// nC of constraintsMPC.m:15-101: the enabled blocks' rows, G_soc always
int ncon_sw_of(int Np, int Nc, int sw) { return (sw & 1 ? 4 * Nc : 0) + (sw & 2 ? Np : 0) + (sw & 4 ? Np : 0) + Np; }

template <class T>
int dalloc(T **p, size_t n) {
  *p = nullptr;
  if (n == 0) return MPCEKF_OK;
  HIPCHK(hipMalloc((void **)p, n * sizeof(T)));
  return MPCEKF_OK;
}

// The output side of the stage calls' host copies (round 6): a pool of worker threads that
// copy device-to-host chunks out of the pinned bounce buffer as their DMA completes.  A call
// enqueues each output as chunks of `chunk` bytes, an event recorded after each chunk's DMA;
// a worker waits for that event and copies the chunk to the caller's array.  So the DMA of
// chunk k + 1 overlaps the copy of chunk k, several threads take the page faults of a
// caller's freshly allocated array at once, and an _async call returns with its copies still
// in flight (finished by the next synchronisation).
struct Copier {
  struct Job {
    hipEvent_t ev;
    const char *src;
    char *dst;
    size_t bytes;
  };
  std::mutex mu;
  std::condition_variable cv, idle;
  std::deque<Job> q;
  size_t busy = 0;
  bool stop = false;
  hipError_t err = hipSuccess;
  std::vector<std::thread> th;
  int device = 0;
  void start(int n, int dev) {
    device = dev;
    for (int i = 0; i < n; ++i) {
      try {
        th.emplace_back([this]() { run(); });
      } catch (...) {  // no thread: the remaining jobs are copied by drain() itself
        break;
      }
    }
  }
  void run() {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || !q.empty(); });
      if (q.empty()) return;  // stop
      Job j = q.front();
      q.pop_front();
      ++busy;
      lk.unlock();
      do_job(j);
      lk.lock();
      --busy;
      if (q.empty() && !busy) idle.notify_all();
    }
  }
  void do_job(const Job &j) {
    hipError_t e = hipEventSynchronize(j.ev);
    if (e == hipSuccess) std::memcpy(j.dst, j.src, j.bytes);
    else {
      std::lock_guard<std::mutex> g(mu);
      if (err == hipSuccess) err = e;
    }
  }
  void push(const Job &j) {
    if (th.empty()) {  // no worker: copied at the synchronisation, in order
      std::lock_guard<std::mutex> g(mu);
      q.push_back(j);
      return;
    }
    {
      std::lock_guard<std::mutex> g(mu);
      q.push_back(j);
    }
    cv.notify_one();
  }
  // every queued copy done; returns (and clears) the first HIP error a worker met
  hipError_t drain() {
    std::unique_lock<std::mutex> lk(mu);
    if (th.empty()) {
      while (!q.empty()) {
        Job j = q.front();
        q.pop_front();
        lk.unlock();
        do_job(j);
        lk.lock();
      }
    } else {
      idle.wait(lk, [&] { return q.empty() && !busy; });
    }
    hipError_t e = err;
    err = hipSuccess;
    return e;
  }
  ~Copier() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    for (std::thread &t : th) t.join();
  }
};

// MPCEKF_COPY_THREADS, else the CPUs this process may use, 1..16 (the workers sleep on their
// events; at 65,536 cells 16 beat 8 by 15 % on the drop-in route, profiles/r06b_*)
int copy_threads() {
  if (const char *e = std::getenv("MPCEKF_COPY_THREADS")) return std::max(0, std::min(64, std::atoi(e)));
  cpu_set_t set;
  int n = 8;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  return std::max(1, std::min(16, n));
}

// The output fields of a fused call, in the order of step_impl's f[]: the order of the staging
// blocks in d_tmp and of the device-to-host copies.
enum {
  F_U, F_V, F_SOC, F_PHISE, F_NEXEC, F_X, F_ZK, F_ZBK, F_JUNC, F_JFIN, F_NORMDU, F_NVIOL, F_POLES, F_SV, F_OBS,
  F_TEMP, F_HEAT,                          // k_thermal's rows
  F_UCMD, F_LIMITER,                       // k_pack's
  F_RATE,                                  // k_aging's
  F_COND,                                  // k_thermal_couple's
  F_BLEED, F_ZMIN,                         // k_pack_bal's
  F_VSTR, F_ISTR, F_CAPBY,                 // k_charger's
  F_LIM,                                   // the limit map's kernels'
  NF
};

// What the launches of a captured fused call depend on (mpcekf_set_graph): kernel arguments are
// call-relative (lazy_t = 1..nsteps, the flush schedule, the output rows), so a call whose key
// equals a cached one replays that graph.  `call` is the call's shape; every other part belongs
// to one context extension and is all 0 for a call that runs without it, so the extension's
// _end retires the graphs that name its buffers by asking for its part (retire_graphs).  Every
// member is one word, so the parts compare as bytes.
struct GraphParts {
  using W = uintptr_t;
  struct {
    W nsteps, dtc, diag, bounds;
    W rows[NF];   // the device rows of the output fields
    W obs_plan;   // a regrown plan buffer: the graphs that named the old one are not replayed
    W nslots;
    W lim;        // set / clear change the launch sequence: graphs of the other one are not replayed
    W hot, hotp;  // the corner window and the plant window the captured kernels name (null: none)
  } call;
  struct { W rec, series; } pack;
  struct { W rec, shape, phi, obs; } aging;    // shape: nreact and sources, which a second begin may change
  struct { W rec, link, snap; } couple;
  struct { W rec, hold, soc; } term;
  struct { W rec, par, on, comp, soc; } balance;
  struct { W rec, par; } charger;
  struct { W hdr, tab; } sched;                // mpcekf_thermal_schedule may regrow the tables
  struct { W rec, tab, soc, nf; } map;         // mpcekf_limit_map may regrow the tables; nf: the lim rows' length
  struct { W ocv, nocv, rec; } thermal;
  struct { W reach, rec; } summary;
};
static_assert(std::has_unique_object_representations_v<GraphParts>, "GraphKey compares the parts as bytes");
struct GraphKey {
  GraphParts p{};
  std::vector<int32_t> slots;  // the call's obs slots
  bool operator==(const GraphKey &o) const { return !std::memcmp(&p, &o.p, sizeof p) && slots == o.slots; }
};

}  // namespace

struct mpcekf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t n = 0;
  int NM = 0, nz = 0, nzp = 0;
  // ncon: nC of the configuration's switches (what ctx_info, get_state and set_state speak);
  // ncon_dev: the all-on row count, whose slots s.lam keeps (a disabled row's stays 0).
  // sw: the switch mask (sw_of); != 7 only at Np = 5 / Nc = 2 (mpcekf_switch.hip)
  int ncon = 0, ncon_dev = 0, sw = 7;
  bool initialized = false;
  KRom r{};
  KCfg k{};
  KState s{};
  mpcekf_config cfg{};
  // device buffers owned by the context
  double *d_cell_blob = nullptr, *d_plant_blob = nullptr, *d_bulk = nullptr, *d_poly = nullptr;
  double *d_const = nullptr;  // 8 per-cell constant arrays
  double *d_mb = nullptr;     // model-blend EKF state [n][MBREC] (method MB)
  bool mb = false;
  double *d_scal = nullptr;   // 8 scalar state arrays + J_unc, J_fin
  int *d_int = nullptr;       // warn, status, nviol, hflag
  double *d_prob = nullptr;   // k_cell -> k_hild problem records
  double *d_zk = nullptr, *d_zbk = nullptr;
  double *d_bnd = nullptr;    // k_cell -> k_bounds records [NBND][n]
  int *d_xm = nullptr;        // fused step: Xind hand-off iterEKF kernel -> EKFmatsHandler kernel
  double *d_xg = nullptr;
  bool split_cell = false;    // fused step: k_cell as two kernels (MPCEKF_SPLIT_CELL=1; slower, 0.125 vs 0.118 ms)
  bool quad = false;          // fused step: iterEKF in k_ekf4 (lane quad per cell), then k_cell<P_MPC>
  int ekf4_block = 256;       // k_ekf4 launch bound (MPCEKF_EKF4_BLOCK=512 / 1024: 256 / 128 VGPRs)
  int *d_ts = nullptr;        // deferred time update: ts_ekf, ts_plant [n][NM]
  double *d_hist = nullptr;   // input rings hist_p, hist_u [LAZY_H][n]
  // the corner window (KState::hot_*): d_hot [4][REC][n] doubles, d_hot_i the
  // tags and timestamps [2][4][n].  Allocated for 'OB' contexts whose fused step runs iterEKF in
  // the lane-per-cell k_cell with the whole-batch flush (MPCEKF_HOT_CORNERS=0 turns it off);
  // null otherwise, and the kernels then do what they did without one
  double *d_hot = nullptr;
  int *d_hot_i = nullptr;
  // the plant window (KState::hotp_*): d_hotp [4][6][n] doubles, d_hotp_i its tags and timestamps
  // [2][4][n].  For the contexts that may have a corner window, when the plant runs inside k_cell
  // (KRom::cell_plant); MPCEKF_HOT_PLANT=0 turns it off on its own
  double *d_hotp = nullptr;
  int *d_hotp_i = nullptr;
  int hot_clear() {  // every slot of both windows empty (context creation, init_cells, set_state)
    if (d_hot_i) HIPCHK(hipMemsetAsync(d_hot_i, 0xFF, (size_t)n * 4 * sizeof(int), stream));
    if (d_hotp_i) HIPCHK(hipMemsetAsync(d_hotp_i, 0xFF, (size_t)n * 4 * sizeof(int), stream));
    return MPCEKF_OK;
  }
  long long *d_stamps = nullptr;  // profiling builds: k_cell section stamps
  // wide horizons (Np = 20, Nc = 10; mpcekf_wide.hip): k_cell hands the linearisation over
  bool wide = false;
  KWide w{};
  double *d_lin = nullptr, *d_zsoc = nullptr;  // [n][35], [n]
  // mpcekf_set_limits (runMPC.m:30-44 per cell): h_lim [MPCEKF_NLIM][n] in mpcekf_config's
  // units (what mpcekf_get_limits returns; empty until the first set), d_lim [NLIMK][n] the
  // kernels' record, allocated by the first set and kept to the end (a captured graph may name
  // it).  percell: the MPC stages launch the per-cell kernel variants
  // lim_set: a mpcekf_set_limits is in force; a temperature schedule (sched, below) keeps the
  // context on the per-cell sequence too, and so does a limit map (lmap): percell = lim_set ||
  // sched || lmap
  std::vector<double> h_lim;
  double *d_lim = nullptr;
  bool percell = false, lim_set = false;
  const double *lim() const { return percell ? d_lim : nullptr; }
  // mpcekf_summary_begin .. _end: the record [NSUM][n], the thresholds [n] and the window the
  // fused step's output rows land in during mpcekf_step_summary, SUM_WIN rows of u, v, soc,
  // phise (double) and nexec (int) in d_sum_ring, one obs slot's in d_sum_obs (allocated by the
  // first begin that names a slot).  Their sizes depend on n alone, never on a call's nsteps.
  double *d_sum = nullptr, *d_sum_reach = nullptr, *d_sum_obs = nullptr;
  char *d_sum_ring = nullptr;
  int32_t sum_slot = -1;
  size_t sum_row() const { return (((size_t)SUM_WIN * (size_t)n * 8) + 255) & ~(size_t)255; }  // one field's rows
  // mpcekf_thermal_begin .. _end: the parameters [NTH][n], the record [NTHR][n], the current
  // the running step applied [n] and the OCV table [th_nocv].  d_th != nullptr: every fused
  // step ends with k_thermal.
  double *d_th = nullptr, *d_th_par = nullptr, *d_th_i = nullptr, *d_th_ocv = nullptr;
  int32_t th_nocv = 0;
  // mpcekf_thermal_schedule .. _schedule_end: the header, each cell's table set [n] and the
  // values in force [SCHED_MAXF][n] are allocated once; the tables [nsets][nf][ntab] grow on
  // demand (sch_cap doubles).  sched: every fused call evaluates the schedule (h_sch: the
  // header's host copy, row i of d_sch_val = field h_sch_field[i])
  SchedHdr *d_sch_hdr = nullptr;
  double *d_sch_tab = nullptr, *d_sch_val = nullptr;
  int *d_sch_set = nullptr;
  size_t sch_cap = 0;
  bool sched = false;
  SchedHdr h_sch{};
  int32_t h_sch_field[SCHED_MAXF] = {};
  int sched_row(int field) const {  // the row of a scheduled field, -1: not scheduled
    for (int i = 0; sched && i < h_sch.nf; ++i)
      if (h_sch_field[i] == field) return i;
    return -1;
  }
  KSched ksched() const {
    KSched g{};
    g.hdr = d_sch_hdr;
    g.tab = d_sch_tab;
    g.set = d_sch_set;
    g.Tc = s.Tc;
    g.lim = d_lim;
    g.val = d_sch_val;
    g.n = n;
    return g;
  }
  // mpcekf_limit_map .. _map_end: the header, each cell's table set [n], the values in force
  // [MAP_MAXF][n], the record [NLMR][n] and the soc row the map's kernels read when the call has
  // none of its own (and no other extension's stands in) are allocated once; the tables
  // [nsets][nf][nt][nz] grow on demand (lm_cap doubles).  lmap: every fused call evaluates the map
  // (h_lm: the header's host copy, row i of d_lm_val = field h_lm_field[i])
  MapHdr *d_lm_hdr = nullptr;
  double *d_lm_tab = nullptr, *d_lm_val = nullptr, *d_lm = nullptr, *d_lm_soc = nullptr;
  int *d_lm_set = nullptr;
  size_t lm_cap = 0;
  bool lmap = false;
  MapHdr h_lm{};
  int32_t h_lm_field[MAP_MAXF] = {};
  int map_row(int field) const {  // the row of a mapped field, -1: not mapped
    for (int i = 0; lmap && i < h_lm.nf; ++i)
      if (h_lm_field[i] == field) return i;
    return -1;
  }
  KMap kmap() const {
    KMap g{};
    g.hdr = d_lm_hdr;
    g.tab = d_lm_tab;
    g.set = d_lm_set;
    g.Tc = s.Tc;
    g.lim = d_lim;
    g.val = d_lm_val;
    g.rec = d_lm;
    g.n = n;
    return g;
  }
  // mpcekf_pack_begin .. _end: the record [NPKR][n] and the cells per string.  d_pk != nullptr:
  // every fused step couples its strings with k_pack after Hildreth.
  double *d_pk = nullptr;
  int32_t pk_series = 0;
  // mpcekf_thermal_couple .. _couple_end (needs a model and a pack): the record [NTCR][n], the
  // links [n] and the snapshot pair [2][n] the neighbours are read from (mpcekf_thermal_couple.hip).
  // d_tc != nullptr: every fused call seeds the snapshot and every step ends with
  // k_thermal_couple(_sched) in k_thermal(_sched)'s place.
  double *d_tc = nullptr, *d_tc_link = nullptr, *d_tc_snap = nullptr;
  // mpcekf_aging_begin .. _end: the record [AG_ROWS][n], the parameters [ag_nreact][NAGP][n]
  // (room for AG_MAXR), and the rows k_aging reads when the call has none of its own: the
  // step's phise row [n] (source EST, no traj.phise) and the plant's negPhise0 row [n] (source
  // PLANT, negPhise0 not among the call's slots; d_ag_plan: that one-position plan of
  // k_obs_traj, ag_need its OBS_NEED_* bits, ag_slot the record slot).  d_ag != nullptr: every
  // fused step runs k_aging before k_thermal.
  double *d_ag = nullptr, *d_ag_par = nullptr, *d_ag_phi = nullptr, *d_ag_obs = nullptr;
  int *d_ag_plan = nullptr;
  int32_t ag_nreact = 0, ag_sources = 0, ag_slot = -1, ag_need = 0;
  // mpcekf_term_begin .. _end: the record [NTMR][n], the thresholds [NTMP][n], the soc row k_term
  // reads when the call has none of its own, and the integers [4 n + 1]: the taper counters
  // [2][n], the string flags' pair [2][n] (room for series = 1) and the open counter.
  // d_tm != nullptr: every fused step runs k_term after Hildreth, before k_pack.
  double *d_tm = nullptr, *d_tm_par = nullptr, *d_tm_soc = nullptr;
  int *d_tm_int = nullptr;
  int32_t tm_hold = 0;
  int *tm_cnt() const { return d_tm_int; }
  int *tm_flag(int half) const { return d_tm_int + (size_t)(2 + half) * std::max<size_t>((size_t)n, 1); }
  int *tm_open() const { return d_tm_int + 4 * std::max<size_t>((size_t)n, 1); }
  // mpcekf_balance_begin .. _end (needs a pack): the record [NBLR][n], the parameters [NBLP][n],
  // the flags [n], the compensate switch and the soc row k_pack_bal reads when the call has none of
  // its own (and k_term's d_tm_soc does not stand in).  d_bl != nullptr: every fused step runs
  // k_pack_bal in k_pack's place.
  double *d_bl = nullptr, *d_bl_par = nullptr, *d_bl_soc = nullptr;
  int *d_bl_on = nullptr;
  int32_t bl_comp = 0;
  // mpcekf_charger_begin .. _end (needs a pack): the record [NCHR][nstrings] and the parameters
  // [NCHP][nstrings], for the pk_series the begin found (a pack_begin with another ends the
  // charger).  d_ch != nullptr: every fused step runs k_charger in k_pack's / k_pack_bal's place.
  double *d_ch = nullptr, *d_ch_par = nullptr;
  double *d_uk1p = nullptr;                      // [n] uk_1 before the step (poles / sv)
  int flush_period = LAZY_H;      // steps between all-model flushes (<= LAZY_H)
  // rolling flush (MPCEKF_FLUSH_ROLL=1, off by default): step t flushes the cell slice
  // t % flush_period on fstream, forked after k_cell and joined before the next step's k_plant.
  // Measured slower (0.287 vs 0.257 ms per step at 65,536 cells, profiles/r03m_roll_ab.txt):
  // every kernel of the step slows by 5-10 us once the step crosses streams.
  bool flush_roll = false;
  hipStream_t fstream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // batches of ncells <= MPCEKF_BOUNDS_SIDE (default 0: off): k_bounds on fstream beside
  // Hildreth.  Both read only what k_cell wrote and neither writes what the other reads.
  // On by default up to 16,384 cells in rounds 4-5 (+1-3 %); with round 6's shorter k_hild the
  // cross-stream fork and join cost more than the overlap at every size (256-16,384 cells,
  // profiles/r06ab_bounds_side_small.txt), so it is an option.
  bool bounds_side = false;
  hipEvent_t ev_bfork = nullptr, ev_bjoin = nullptr;
  // staging for host trajectories / stage IO (grown on demand)
  double *d_tmp = nullptr;
  size_t tmp_bytes = 0;
  // pinned host bounce buffer of the stage entry points' host copies (Xfer), grown on
  // demand; copies above bounce_max bytes (MPCEKF_BOUNCE_MAX, default 256 MiB: every copy of
  // a 65,536-cell stage call is below 15 MiB) go to / from the caller's memory directly
  char *h_bounce = nullptr;
  size_t h_bytes = 0, bounce_max = (size_t)256 << 20;
  // round 6: the buffer is bump-allocated over the calls up to the next synchronisation
  // (xoff), so _async calls keep their regions until their copies finish; outputs leave it
  // in chunks of xchunk bytes (MPCEKF_CHUNK, default 4 MiB), one event each (xev, reused
  // after the synchronisation), copied out by the worker pool `copier`
  size_t xoff = 0, xchunk = (size_t)4 << 20, xhwm = 0;
  std::vector<hipEvent_t> xev;
  size_t xev_used = 0;
  bool xpending = false;
  Copier *copier = nullptr;
  hipError_t next_event(hipEvent_t *e) {
    if (xev_used == xev.size()) {
      hipEvent_t ne = nullptr;
      hipError_t r = hipEventCreateWithFlags(&ne, hipEventDisableTiming);
      if (r != hipSuccess) return r;
      xev.push_back(ne);
    }
    *e = xev[xev_used++];
    return hipSuccess;
  }
  // the synchronisation every synchronous stage call (and mpcekf_sync) ends with: the
  // stream, then every output copy still queued; the bounce buffer and events free again
  int drain() {
    hipError_t e = hipStreamSynchronize(stream);
    hipError_t c = copier ? copier->drain() : hipSuccess;
    xoff = 0;
    xev_used = 0;
    xpending = false;
    if (e != hipSuccess) return fail(MPCEKF_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    if (c != hipSuccess) return fail(MPCEKF_E_HIP, "output copy: %s", hipGetErrorString(c));
    return MPCEKF_OK;
  }
  // per-kernel HIP-event timing (mpcekf_set_timing)
  bool timing = false;
  int timing_every = 1;  // sample every timing_every-th step (1 = every step)
  std::vector<hipEvent_t> ev;
  double t_ms[MPCEKF_NKERNELS] = {};
  int64_t t_n[MPCEKF_NKERNELS] = {};
  // soc(z,T) ends and the table temperatures, for SOC0n/p at init (OB_step.m:63-65)
  std::vector<double> tabT, soc_end[2][2];

  // mpcekf_set_graph: fused calls captured into hipGraphs, keyed by the call shape
  bool graph = false;
  struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec;
  };
  std::vector<GraphEntry> graphs;
  // the graphs whose key's parts `pred` selects are destroyed: they name buffers about to be
  // freed or replaced.  The caller has waited for the stream.
  template <class Pred>
  void retire_graphs(Pred &&pred) {
    for (size_t i = graphs.size(); i-- > 0;)
      if (pred(graphs[i].key.p)) {
        (void)hipGraphExecDestroy(graphs[i].exec);
        graphs.erase(graphs.begin() + (std::ptrdiff_t)i);
      }
  }
  template <class Fn>
  int graph_launch(const GraphKey &key, Fn &&launch) {
    for (const GraphEntry &g : graphs)
      if (g.key == key) {
        HIPCHK(hipGraphLaunch(g.exec, stream));
        return MPCEKF_OK;
      }
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int rc = launch();
    hipGraph_t gr = nullptr;
    hipError_t e = hipStreamEndCapture(stream, &gr);
    if (rc) {
      if (gr) (void)hipGraphDestroy(gr);
      return rc;
    }
    if (e != hipSuccess) return fail(MPCEKF_E_HIP, "graph capture: %s", hipGetErrorString(e));
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    if (e != hipSuccess) return fail(MPCEKF_E_HIP, "graph instantiate: %s", hipGetErrorString(e));
    if (graphs.size() >= 16) {  // a small cache: oldest shape out
      (void)hipGraphExecDestroy(graphs.front().exec);
      graphs.erase(graphs.begin());
    }
    graphs.push_back({key, ex});
    HIPCHK(hipGraphLaunch(ex, stream));
    return MPCEKF_OK;
  }
  // the stage route's device-resident hand-offs (runMPC.m:88-103 as the drop-ins call it):
  // the last mpcekf_ekf_step's zk and Xind, the last mpcekf_linearize's records, so the next
  // stage call can take NULL for them instead of a host round trip (valid until a fused step,
  // set_state or init_cells; stage_zk / stage_lin say which are current)
  double *d_szk = nullptr, *d_sxg = nullptr, *d_slin = nullptr, *d_sv = nullptr;
  int *d_sxm = nullptr, *d_zslot = nullptr;  // d_zslot: zk(end)'s slot, nz + 1 (mpc_step's NULL soc_k1)
  bool stage_zk = false, stage_lin = false, stage_v = false;
  // mpcekf_plant_step_obs (OB_step's obs output): the layout and the obs blob are made by
  // build_rom on the host; the blob's device copy and the record [nobs][n] are allocated by
  // the first obs call (a context that never asks for obs holds neither)
  int32_t obs_off[MPCEKF_OBS_COUNT + 1] = {};
  std::vector<double> h_obs_blob;
  KObs ko{};
  double *d_obs_blob = nullptr, *d_obs = nullptr;
  bool stage_obs = false;  // d_obs holds the record of an obs call since init / fused step / set_state
  // mpcekf_step_ex_obs: the call's slot plan for k_obs_traj (KObsSel::plan), its host copy
  // (alive until the call's synchronisation) and the permuted row behind each record slot
  int *d_obs_plan = nullptr;
  size_t obs_plan_cap = 0;
  std::vector<int> h_obs_plan, obs_slot_src;
  int obs_blob_buf() {
    if (!d_obs_blob) {
      HIPCHK(hipMalloc((void **)&d_obs_blob, h_obs_blob.size() * sizeof(double)));
      HIPCHK(hipMemcpy(d_obs_blob, h_obs_blob.data(), h_obs_blob.size() * sizeof(double), hipMemcpyHostToDevice));
      ko.blob = d_obs_blob;
    }
    return MPCEKF_OK;
  }
  int obs_bufs() {
    int rc = obs_blob_buf();
    if (rc) return rc;
    if (!d_obs) HIPCHK(hipMalloc((void **)&d_obs, (size_t)ko.nobs * (size_t)n * sizeof(double)));
    ko.rec = d_obs;
    return MPCEKF_OK;
  }
  int stage_bufs() {
    const size_t nzz = (size_t)nz + 2;
    if (!d_sv) HIPCHK(hipMalloc((void **)&d_sv, (size_t)n * sizeof(double)));
    if (!d_zslot) {
      const int zs = nz + 1;
      HIPCHK(hipMalloc((void **)&d_zslot, sizeof(int)));
      HIPCHK(hipMemcpy(d_zslot, &zs, sizeof(int), hipMemcpyHostToDevice));
    }
    if (!d_szk) HIPCHK(hipMalloc((void **)&d_szk, (size_t)n * nzz * sizeof(double)));
    if (!d_sxg) HIPCHK(hipMalloc((void **)&d_sxg, (size_t)n * 4 * sizeof(double)));
    if (!d_sxm) HIPCHK(hipMalloc((void **)&d_sxm, (size_t)n * 4 * sizeof(int)));
    if (!d_slin) HIPCHK(hipMalloc((void **)&d_slin, (size_t)n * MPCEKF_LIN_SIZE * sizeof(double)));
    return MPCEKF_OK;
  }
  int diag_bufs() {  // the linearisation records and uk_1 copy of the poles / sv diagnostics
    if (!d_lin) HIPCHK(hipMalloc((void **)&d_lin, (size_t)n * MPCEKF_LIN_SIZE * sizeof(double)));
    if (!d_uk1p) HIPCHK(hipMalloc((void **)&d_uk1p, (size_t)n * sizeof(double)));
    return MPCEKF_OK;
  }
  // room for `bytes` more of the current epoch's copies: when the buffer is too small, the
  // pending calls are completed first (drain) and the buffer regrown.  A failed pinned
  // allocation is not an error: the buffer stays empty and every copy goes direct (Xfer::fits).
  int bounce(size_t bytes) {
    if (xoff + bytes <= h_bytes) return MPCEKF_OK;
    // grown to the largest epoch seen (a step's _async calls together), so a steady
    // sequence of calls between synchronisations never drains early
    const size_t want = std::max(xoff + bytes, xhwm);
    xhwm = want;
    if (xpending || xoff) {
      int rc = drain();
      if (rc) return rc;
    }
    bytes = want;
    if (bytes <= h_bytes) return MPCEKF_OK;
    if (h_bounce) (void)hipHostFree(h_bounce);
    h_bounce = nullptr;
    h_bytes = 0;
    if (hipHostMalloc((void **)&h_bounce, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      h_bounce = nullptr;
      return MPCEKF_OK;
    }
    h_bytes = bytes;
    return MPCEKF_OK;
  }
  int tmp(size_t bytes) {
    if (bytes <= tmp_bytes) return MPCEKF_OK;
    if (d_tmp) (void)hipFree(d_tmp);
    d_tmp = nullptr;
    tmp_bytes = 0;
    HIPCHK(hipMalloc((void **)&d_tmp, bytes));
    tmp_bytes = bytes;
    return MPCEKF_OK;
  }
};

extern "C" {

int mpcekf_abi_version(void) { return MPCEKF_ABI_VERSION; }

#ifndef MPCEKF_SRC_HASH
#define MPCEKF_SRC_HASH "unknown"
#endif
const char *mpcekf_build_id(void) { return MPCEKF_SRC_HASH; }

const char *mpcekf_last_error(void) { return g_err.c_str(); }

void mpcekf_config_defaults(mpcekf_config *c) {
  std::memset(c, 0, sizeof(*c));
  c->Np = 5;                  // runMPC.m:28
  c->Nc = 2;                  // runMPC.m:29
  c->target_soc = 95;         // runMPC.m:30
  c->Crate = 2;               // runMPC.m:36
  c->u_max = 2;               // runMPC.m:37
  c->du_min = -50;            // runMPC.m:38
  c->du_max = 50;             // runMPC.m:39
  c->v_min = 3.4;             // runMPC.m:40 (not enforced by constraintsMPC.m)
  c->v_max = 4.1;             // runMPC.m:41
  c->phise_min = 0.08;        // runMPC.m:42
  c->z_max = 95.0 / 100;      // runMPC.m:43
  c->z_tol = 0 * 5.0 / 100;   // runMPC.m:44
  c->use_current = c->use_voltage = c->use_eta = 1;  // runMPC.m:33
  c->max_hild = 100;          // initMPC.m:47
  c->hild_tol = 1e-6;         // hildreth.m:39
  c->SigmaV = 1e-3;           // runMPC.m:19
  c->SigmaW = 1e2;            // runMPC.m:18
  for (int i = 0; i < 5; ++i) c->SigmaX0[i] = 1;
  c->SigmaX0[5] = 2e6;        // runMPC.m:17
  c->max_warn = 10;           // iterEKF.m:55
  c->flags = 0;
  c->method = MPCEKF_METHOD_OB;  // runMPC.m:16 blend = 'OutB'
}

// ---------------------------------------------------------------------------
// ROM validation and packing
// ---------------------------------------------------------------------------
static int build_rom(mpcekf_ctx *X, const mpcekf_rom *R) {
  if (!R || !R->T_degC || !R->SOC_pct || !R->A || !R->C || !R->D || !R->tf_code || !R->tf_xloc)
    return fail(MPCEKF_E_ARG, "rom: null array");
  if (R->n != NX) return fail(MPCEKF_E_UNSUPPORTED, "rom: n = %d transient states, kernels are built for 5", R->n);
  if (R->nT < 1 || R->nT > MAXT || R->nZ < 1 || R->nZ > MAXZ)
    return fail(MPCEKF_E_UNSUPPORTED, "rom: grid %dx%d exceeds %dx%d", R->nT, R->nZ, MAXT, MAXZ);
  if (R->nz < NROLE || R->nz > MAXROWS) return fail(MPCEKF_E_UNSUPPORTED, "rom: nz = %d outside [11, 64]", R->nz);
  if (R->tab_ntheta < 2 || R->tab_ntemp < 1 || R->tab_ntemp > MAXTT || !R->tab_T_K)
    return fail(MPCEKF_E_UNSUPPORTED, "rom: electrode tables need ntheta >= 2 and 1 <= ntemp <= %d", MAXTT);
  for (int j = 0; j < R->tab_ntemp; ++j)
    if (!std::isfinite(R->tab_T_K[j]) || (j && !(R->tab_T_K[j] > R->tab_T_K[j - 1])))
      return fail(MPCEKF_E_ROM, "rom: electrode table temperatures must be finite and ascending");
  for (const mpcekf_electrode *e : {&R->neg, &R->pos})
    if (!e->soc0 || !e->soc100 || !e->Uocp || !e->dUocp || !e->k0 || !e->Rf || !e->Cdleff || !e->Uocp1)
      return fail(MPCEKF_E_ROM, "rom: electrode table missing");
  // ABI v3: theta polynomials (both electrodes, every function) and Arrhenius energies
  if (R->tab_npoly != 0 && R->tab_npoly != 4 && R->tab_npoly != KPOLY)
    return fail(MPCEKF_E_ARG, "rom: tab_npoly = %d (0: linear tables, 4: cubic, 6: quintic)", R->tab_npoly);
  for (const mpcekf_electrode *e : {&R->neg, &R->pos}) {
    const double *ps[6] = {e->Uocp_p, e->dUocp_p, e->k0_p, e->Rf_p, e->Cdleff_p, e->Uocp1_p};
    for (int f = 0; f < 6; ++f) {
      const int m = e->nnode[f];
      if (m != 0 && (!R->tab_npoly || m < 2 || !e->node[f] || !e->node_p[f]))
        return fail(MPCEKF_E_ROM, "rom: nnode[%d] = %d needs tab_npoly, >= 2 nodes and their tables", f, m);
      if (R->tab_npoly && m == 0 && !ps[f])
        return fail(MPCEKF_E_ROM, "rom: tab_npoly = %d but polynomial table %d is missing", R->tab_npoly, f);
      for (int j = 0; j < m; ++j)  // strictly ascending, finite; interior nodes inside (0, 1)
        if (!std::isfinite(e->node[f][j]) || (j && !(e->node[f][j] > e->node[f][j - 1])) ||
            (j > 0 && j < m - 1 && !(e->node[f][j] > 0.0 && e->node[f][j] < 1.0)))
          return fail(MPCEKF_E_ROM, "rom: theta nodes of table %d must be finite, ascending, interior in (0, 1)", f);
    }
    for (int f = 0; f < 5; ++f)
      if (!std::isfinite(e->Ea[f])) return fail(MPCEKF_E_ROM, "rom: Ea[%d] is not finite", f);
  }
  for (int i = 1; i < R->nT; ++i)
    if (!(R->T_degC[i] > R->T_degC[i - 1])) return fail(MPCEKF_E_ROM, "rom: T set-points not ascending");
  for (int i = 1; i < R->nZ; ++i)
    if (!(R->SOC_pct[i] > R->SOC_pct[i - 1])) return fail(MPCEKF_E_ROM, "rom: SOC set-points not ascending");
  const int nT = R->nT, nZ = R->nZ, NM = nT * nZ, nz = R->nz, n1 = NX + 1;
  for (int m = 0; m < NM; ++m)
    if (R->A[(size_t)m * n1 + NX] != 1.0) return fail(MPCEKF_E_ROM, "A for model %d has no integrator state (initKF.m:74)", m);
  for (int q = 0; q < nz; ++q)
    if (R->tf_code[q] < 0 || R->tf_code[q] >= MPCEKF_TF_COUNT) return fail(MPCEKF_E_ROM, "rom: bad tf code at row %d", q);

  // --- index resolution (iterEKF.m:610-735) ---
  auto rows_of = [&](int code) {
    std::vector<int> v;
    for (int q = 0; q < nz; ++q)
      if (R->tf_code[q] == code) v.push_back(q);
    return v;
  };
  auto cat = [](std::vector<int> a, const std::vector<int> &b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
  };
  const double *loc = R->tf_xloc;
  auto at = [&](const std::vector<int> &v, double x) {
    std::vector<int> o;
    for (int q : v)
      if (loc[q] == x) o.push_back(q);
    return o;
  };
  std::vector<int> Ifdl = cat(rows_of(MPCEKF_TF_negIfdl), rows_of(MPCEKF_TF_posIfdl));
  std::vector<int> If = cat(rows_of(MPCEKF_TF_negIf), rows_of(MPCEKF_TF_posIf));
  std::vector<int> Thss = cat(rows_of(MPCEKF_TF_negThetass), rows_of(MPCEKF_TF_posThetass));
  std::vector<int> Phise = cat(rows_of(MPCEKF_TF_negPhise), rows_of(MPCEKF_TF_posPhise));
  std::vector<int> Phie = cat(cat(rows_of(MPCEKF_TF_negPhie), rows_of(MPCEKF_TF_sepPhie)), rows_of(MPCEKF_TF_posPhie));
  std::vector<int> Thetae =
      cat(cat(rows_of(MPCEKF_TF_negThetae), rows_of(MPCEKF_TF_sepThetae)), rows_of(MPCEKF_TF_posThetae));
  struct {
    const char *name;
    std::vector<int> v;
  } singles[] = {{"ifdl at negative-collector", at(Ifdl, 0)}, {"ifdl at positive-collector", at(Ifdl, 3)},
                 {"if at negative-collector", at(If, 0)},     {"if at positive-collector", at(If, 3)},
                 {"thetass at negative-collector", at(Thss, 0)}, {"thetass at positive-collector", at(Thss, 3)},
                 {"phise at negative-collector", at(Phise, 0)}};
  for (auto &s : singles)
    if (s.v.size() != 1) return fail(MPCEKF_E_ROM, "Simulation requires exactly one %s (iterEKF.m:692-725)", s.name);
  const double eps = 2.220446049250313e-16;
  if (Thetae.empty() || loc[Thetae.front()] > 0) return fail(MPCEKF_E_ROM, "Simulation requires thetae at negative-collector!");
  if (loc[Thetae.back()] > 3 + eps || loc[Thetae.back()] < 3 - eps)
    return fail(MPCEKF_E_ROM, "Simulation requires thetae at positive-collector!");
  if (!Phie.empty() && loc[Phie.front()] == 0) Phie.erase(Phie.begin());  // iterEKF.m:728-731
  if (Phie.empty() || loc[Phie.back()] > 3 + eps || loc[Phie.back()] < 3 - eps)
    return fail(MPCEKF_E_ROM, "Simulation requires phie at positive-collector!");
  std::vector<int> negPhise = rows_of(MPCEKF_TF_negPhise);
  if (negPhise.size() < 2) return fail(MPCEKF_E_ROM, "EKFmatsHandler.m:97 needs ind.negPhise(2)");
  // OB_step's own lookups (OB_step.m:131-137) must agree
  auto negat = [&](int code, double x) { return at(rows_of(code), x); };
  if (negat(MPCEKF_TF_negIfdl, 0) != singles[0].v || negat(MPCEKF_TF_posIfdl, 3) != singles[1].v ||
      negat(MPCEKF_TF_negIf, 0) != singles[2].v || negat(MPCEKF_TF_posIf, 3) != singles[3].v ||
      negat(MPCEKF_TF_negThetass, 0) != singles[4].v || negat(MPCEKF_TF_posThetass, 3) != singles[5].v)
    return fail(MPCEKF_E_ROM, "OB_step and iterEKF resolve collector rows differently");
  int role[NROLE];
  role[R_IFDL0] = singles[0].v[0];
  role[R_IFDL3] = singles[1].v[0];
  role[R_IF0] = singles[2].v[0];
  role[R_IF3] = singles[3].v[0];
  role[R_TH0] = singles[4].v[0];
  role[R_TH3] = singles[5].v[0];
  role[R_TE1] = Thetae.front();
  role[R_TEE] = Thetae.back();
  role[R_PHIE] = Phie.back();
  role[R_PHISE0] = singles[6].v[0];
  role[R_NPHISE2] = negPhise[1];
  for (int a = 0; a < NROLE; ++a)
    for (int b = a + 1; b < NROLE; ++b)
      if (role[a] == role[b]) return fail(MPCEKF_E_UNSUPPORTED, "rom: role rows %d and %d coincide", a, b);
  std::vector<int> perm(role, role + NROLE);
  for (int q = 0; q < nz; ++q)
    if (std::find(perm.begin(), perm.end(), q) == perm.end()) perm.push_back(q);
  int nzp = 0;
  for (int cand : {26, 32})
    if (nz <= cand && cell_kernel_supported(cand)) { nzp = cand; break; }
  if (!nzp) return fail(MPCEKF_E_UNSUPPORTED, "rom: nz = %d not built (kernels: 26, 32)", nz);

  unsigned char flags[MAXROWS] = {0}, c0k[MAXROWS] = {0};
  std::vector<unsigned> fl(nz, 0u);
  std::vector<int> c0(nz, C0_ZERO);
  for (int q : rows_of(MPCEKF_TF_negThetass)) fl[q] |= G_NTH;
  for (int q : rows_of(MPCEKF_TF_posThetass)) fl[q] |= G_PTH;
  for (int q : rows_of(MPCEKF_TF_negPhise)) fl[q] |= G_NPHISE;
  for (int q : rows_of(MPCEKF_TF_posPhise)) fl[q] |= G_PPHISE;
  for (int q : Phie) fl[q] |= G_PHIE | (loc[q] == 0 ? G_PHIE0 : 0u);
  for (int q : Thetae) fl[q] |= G_THETAE;
  for (int q : rows_of(MPCEKF_TF_posPhis)) fl[q] |= G_PPHIS;
  for (int q : rows_of(MPCEKF_TF_posPhis)) c0[q] = C0_CHATV0;  // iterEKF.m:553-586 order
  for (int q : rows_of(MPCEKF_TF_negThetass)) c0[q] = C0_RES0N;
  for (int q : rows_of(MPCEKF_TF_posThetass)) c0[q] = C0_RES0P;
  for (int q : rows_of(MPCEKF_TF_negPhise)) c0[q] = C0_DUN;
  for (int q : rows_of(MPCEKF_TF_posPhise)) c0[q] = C0_DUP;
  for (int q : Phie) c0[q] = C0_MDUN;
  KRom &r = X->r;
  std::memset(&r, 0, sizeof(r));
  for (int q = 0; q < nz; ++q) {
    flags[q] = (unsigned char)fl[perm[q]];
    c0k[q] = (unsigned char)c0[perm[q]];
    r.perm[q] = (short)perm[q];
  }
  std::memcpy(r.flags, flags, sizeof flags);
  for (int q = 0; q < nz && q < 32; ++q)  // nz <= nzp <= 32 (checked above)
    for (int b = 0; b < 8; ++b)
      if (flags[q] >> b & 1) r.fmask[b] |= 1u << q;
  std::memcpy(r.c0k, c0k, sizeof c0k);
  r.NM = NM; r.nT = nT; r.nZ = nZ; r.nz = nz; r.nzp = nzp;
  r.nth = R->tab_ntheta; r.nte = R->tab_ntemp;
  r.Ts = R->Ts; r.Q = R->Q; r.F = R->F; r.R = R->R; r.Rc = R->Rc; r.Tref = R->Tref;
  r.th0n = R->neg.theta0; r.th100n = R->neg.theta100; r.th0p = R->pos.theta0; r.th100p = R->pos.theta100;

  // --- electrode tables (mpcekf_kernels.hip ETab): header, then [fn][side][nte][nth] ---
  // (v3: the header without Uocp1, and the rows as polynomials in a global table)
  const int nth = r.nth, nte = r.nte;
  const bool poly = R->tab_npoly != 0;
  const mpcekf_electrode *els[2] = {&R->neg, &R->pos};
  std::vector<double> tabs;
  if (!poly)
    for (const mpcekf_electrode *e : els) tabs.insert(tabs.end(), e->Uocp1, e->Uocp1 + nth);
  for (int j = 0; j < MAXTT; ++j) tabs.push_back(j < nte ? R->tab_T_K[j] : 0.0);
  X->tabT.assign(R->tab_T_K, R->tab_T_K + nte);
  for (int e = 0; e < 2; ++e)
    for (int one = 0; one < 2; ++one) {
      const double *src = one ? els[e]->soc100 : els[e]->soc0;
      X->soc_end[e][one].assign(src, src + nte);
      for (int j = 0; j < MAXTT; ++j) tabs.push_back(j < nte ? src[j] : 0.0);
    }
  // v3 device layout (mpcekf_kernels.hip ETab::f): per function and electrode the nte rows of
  // each theta interval adjacent, [nth-1][nte][KPOLY] (cubics padded with c4 = c5 = 0), or
  // [nth-1][1][KPOLY] when every row is equal (T-invariant: the row blended with itself, the
  // same value); Uocp1 last
  std::vector<double> ptab;
  const int np = R->tab_npoly;
  const size_t nint = (size_t)(nth - 1);
  // the kernels' lookup descriptors (mpcekf_kernels.hip etab_desc): per function and side
  // Ea/R, (off, istride), (jstride, ro), (mapoff, nu) in doubles of ptab; Uocp1 of each side last
  double desc[12][KDESC] = {};
  bool any_nodes = false;
  auto pack2 = [](long long lo, long long hi) {
    const unsigned long long w = (unsigned long long)(uint32_t)lo | (unsigned long long)(uint32_t)hi << 32;
    double d;
    std::memcpy(&d, &w, sizeof d);
    return d;
  };
  auto add_poly = [&](const double *src, int rows) {  // src [rows][nth-1][np] (ABI order)
    for (size_t i = 0; i < nint; ++i)
      for (int j = 0; j < rows; ++j)
        for (int c = 0; c < KPOLY; ++c) ptab.push_back(c < np ? src[((size_t)j * nint + i) * np + c] : 0.0);
  };
  // ABI v4: a function on its own nodes -- its rows [rows][m-1][np] interval-major like v3's,
  // and a bucket map: nu (a power of two) buckets over [0, 1] with at most one interior node
  // inside each, so that floor(theta nu) and one compare give the oracle's segment
  // k = #{j in 1..m-2 : x_j <= theta}; entry u = (k of u / nu, x_k, x_k+1 or +inf, 0)
  auto add_nodes = [&](double *d, const double *x, int m, const double *src, int rows) -> int {
    const int nseg = m - 1;
    int nu = 1;
    for (;; nu *= 2) {
      bool ok = true;
      for (int j = 2; j < m - 1 && ok; ++j)  // interior nodes j-1, j in one bucket?
        ok = std::floor(x[j] * nu) != std::floor(x[j - 1] * nu);
      if (ok) break;
      if (nu >= (1 << 20)) return fail(MPCEKF_E_ROM, "rom: theta nodes closer than 2^-20");
    }
    d[1] = pack2((long long)ptab.size(), (long long)rows * KPOLY);
    d[2] = pack2(rows > 1 ? KPOLY : 0, rows > 1 ? KPOLY : 0);
    for (int i = 0; i < nseg; ++i)
      for (int j = 0; j < rows; ++j)
        for (int c = 0; c < KPOLY; ++c) ptab.push_back(c < np ? src[((size_t)j * nseg + i) * np + c] : 0.0);
    if (ptab.size() & 1) ptab.push_back(0.0);  // 16-byte map entries
    d[3] = pack2((long long)ptab.size(), nu);
    for (int u = 0; u < nu; ++u) {
      const double e = (double)u / nu;  // exact: nu is a power of two
      int k = 0;
      while (k + 1 <= m - 2 && x[k + 1] <= e) ++k;
      ptab.push_back((double)k);
      ptab.push_back(x[k]);
      ptab.push_back(k + 1 <= m - 2 ? x[k + 1] : HUGE_VAL);
      ptab.push_back(0.0);
    }
    any_nodes = true;
    return MPCEKF_OK;
  };
  bool theta_const = true;
  if (const char *ev = std::getenv("MPCEKF_THETA_CONST")) theta_const = std::atoi(ev) != 0;
  for (int fn = 0; fn < 5 && poly; ++fn)  // EF_U, EF_DU, EF_K0, EF_RF, EF_CDL
    for (int sd = 0; sd < 2; ++sd) {
      const mpcekf_electrode *e = els[sd];
      if (e->nnode[fn] >= 2) {  // v4: on its own nodes
        const int m = e->nnode[fn];
        const double *src = e->node_p[fn];
        const size_t rl = (size_t)(m - 1) * np;
        bool same = nte > 1;
        for (int j = 1; j < nte && same; ++j) same = std::memcmp(src, src + j * rl, rl * sizeof(double)) == 0;
        double *d = desc[fn * 2 + sd];
        d[0] = e->Ea[fn] != 0.0 ? e->Ea[fn] / R->R : 0.0;
        int rc = add_nodes(d, e->node[fn], m, src, same ? 1 : nte);
        if (rc) return rc;
        continue;
      }
      const double *src =
          fn == 0 ? e->Uocp_p : fn == 1 ? e->dUocp_p : fn == 2 ? e->k0_p : fn == 3 ? e->Rf_p : e->Cdleff_p;
      bool same = nte > 1;
      for (int j = 1; j < nte && same; ++j)
        same = std::memcmp(src, src + (size_t)j * nint * np, nint * np * sizeof(double)) == 0;
      double *d = desc[fn * 2 + sd];
      const double ea = e->Ea[fn];
      d[0] = ea != 0.0 ? ea / R->R : 0.0;  // oracle: (Ea / R) * (1/Tref - 1/T)
      const int rows = same ? 1 : nte;
      // a theta-invariant function (every interval's coefficients those of interval 0, e.g.
      // a Cdleff or an Arrhenius k0 that depends on T only): istride 0, so every lane reads
      // interval 0's rows -- one broadcast line instead of a 64-lane gather -- and evaluates
      // them at its own s, the same coefficients and the same s as the oracle's interval:
      // the same bits.  MPCEKF_THETA_CONST=0 keeps the gather (A/B).
      bool thc = nint > 1 && theta_const;
      for (int jr = 0; jr < rows && thc; ++jr)
        for (size_t i = 1; i < nint && thc; ++i)
          thc = std::memcmp(src + ((size_t)jr * nint + i) * np, src + (size_t)jr * nint * np, np * sizeof(double)) == 0;
      d[1] = pack2((long long)ptab.size(), thc ? 0 : (long long)rows * KPOLY);  // off, istride
      d[2] = pack2(same ? 0 : KPOLY, (same || nte == 1) ? 0 : KPOLY);          // jstride, ro
      add_poly(src, rows);
    }
  if (!poly)  // v2: [fn][side][nte][nth] in the LDS blob
    for (int fn = 0; fn < 5; ++fn)
      for (const mpcekf_electrode *e : els) {
        const double *t = fn == 0 ? e->Uocp : fn == 1 ? e->dUocp : fn == 2 ? e->k0 : fn == 3 ? e->Rf : e->Cdleff;
        tabs.insert(tabs.end(), t, t + (size_t)nte * nth);
      }
  if (poly)
    for (int sd = 0; sd < 2; ++sd) {
      if (els[sd]->nnode[5] >= 2) {
        int rc = add_nodes(desc[10 + sd], els[sd]->node[5], els[sd]->nnode[5], els[sd]->node_p[5], 1);
        if (rc) return rc;
        continue;
      }
      desc[10 + sd][1] = pack2((long long)ptab.size(), KPOLY);
      add_poly(els[sd]->Uocp1_p, 1);
    }
  if (poly) {
    if (ptab.size() >= (size_t)INT32_MAX) return fail(MPCEKF_E_ROM, "rom: v3 tables exceed 2^31 doubles");
    for (auto &d : desc) tabs.insert(tabs.end(), d, d + KDESC);
  }
  r.npoly = poly ? KPOLY : 0;
  r.nodes = any_nodes ? 1 : 0;
  r.arr = 0;
  for (int f = 0; f < 5; ++f)
    for (int sd = 0; sd < 2; ++sd) r.arr |= poly && els[sd]->Ea[f] != 0.0;
  // k_cell / k_bounds need no Cdleff table, unless k_cell also runs the plant (cell_plant)
  const char *cpe = getenv("MPCEKF_CELL_PLANT");
  bool cell_plant = !(cpe && atoi(cpe) == 0);
  auto cell_tablen_of = [&](bool cp) { return tabs.size() - (cp || poly ? 0 : (size_t)2 * nte * nth); };
  std::vector<double> pts(MAXT + MAXZ, 0.0);
  for (int t = 0; t < nT; ++t) pts[t] = R->T_degC[t] + 273.15;  // ROMmdls(t,z).T (initKF.m:58)
  for (int z = 0; z < nZ; ++z) pts[MAXT + z] = R->SOC_pct[z] / 100;  // ROMmdls(t,z).SOC
  auto Cval = [&](int m, int q, int k) { return R->C[((size_t)m * nz + q) * n1 + k]; };
  auto Dval = [&](int m, int q) { return R->D[(size_t)m * nz + q]; };
  // cell blob: per model [C nzp x 5][D nzp][a 5][a_p a_q, packed Sigma order 15]
  // (+ [res0 of the 9 plant rows] when k_cell runs the plant).  An odd stride in doubles:
  // lanes reading one offset of different models then spread over all LDS banks (an even
  // stride such as 176 folds them onto 2 bank positions).
  int pr[NPK], pc[NPK];
  for (int p = 0, i = 0; p < NX; ++p)
    for (int q = p; q < NX; ++q, ++i) { pr[i] = p; pc[i] = q; }
  std::vector<double> cb;
  auto make_cell_blob = [&](bool cp) {
    r.cell_stride = (nzp * NX + nzp + NX + NPK + (cp ? NPLANT : 0)) | 1;
    cb.assign((size_t)NM * r.cell_stride, 0.0);
    for (int m = 0; m < NM; ++m) {
      double *b = cb.data() + (size_t)m * r.cell_stride;
      for (int q = 0; q < nz; ++q) {
        for (int k = 0; k < NX; ++k) b[q * NX + k] = Cval(m, perm[q], k);  // initKF.m:91 strips res0
        b[nzp * NX + q] = Dval(m, perm[q]);
      }
      for (int k = 0; k < NX; ++k) b[nzp * NX + nzp + k] = R->A[(size_t)m * n1 + k];
      for (int i = 0; i < NPK; ++i)  // Sigma time update coefficients (iterEKF.m:78)
        b[nzp * NX + nzp + NX + i] = R->A[(size_t)m * n1 + pr[i]] * R->A[(size_t)m * n1 + pc[i]];
      if (cp)  // the plant's res0 column (OB_step.m:272-275; Phise rows are not among the 9)
        for (int q = 0; q < NPLANT; ++q) b[nzp * NX + nzp + NX + NPK + q] = Cval(m, perm[q], NX);
    }
    if (cb.size() & 1) cb.push_back(0.0);  // tables at an even offset: 16-byte staging in rom_global mode
    r.cell_tab = (int)cb.size();
    r.cell_tablen = (int)cell_tablen_of(cp);
    cb.insert(cb.end(), tabs.begin(), tabs.begin() + r.cell_tablen);
    cb.insert(cb.end(), pts.begin(), pts.end());
    r.cell_len = (int)cb.size();
    r.cell_plant = cp;
  };
  make_cell_blob(cell_plant);
  // plant blob: per model [C 9 x 5][res0 9][D 9] over role rows 0..8
  std::vector<double> pb((size_t)NM * PREC, 0.0);
  for (int m = 0; m < NM; ++m) {
    double *b = pb.data() + (size_t)m * PREC;
    for (int q = 0; q < NPLANT; ++q) {
      for (int k = 0; k < NX; ++k) b[q * NX + k] = Cval(m, perm[q], k);
      b[NPLANT * NX + q] = Cval(m, perm[q], NX);  // res0 column (Phise rows are not among these)
      b[NPLANT * NX + NPLANT + q] = Dval(m, perm[q]);
    }
    for (int e = 0; e < 6; ++e) b[NPLANT * NX + 2 * NPLANT + e] = R->A[(size_t)m * n1 + e];  // bigA column
  }
  if (pb.size() & 1) pb.push_back(0.0);
  r.plant_tab = (int)pb.size();
  r.plant_tablen = (int)tabs.size();
  pb.insert(pb.end(), tabs.begin(), tabs.end());
  pb.insert(pb.end(), pts.begin(), pts.end());
  r.plant_len = (int)pb.size();
  // bulk tables: the time-update coefficient of every EKF record element (a for xhat,
  // a_p a_q for Sigma) and of every plant state (bigA)
  std::vector<double> bt((size_t)NM * (REC + 6));
  double *cC = bt.data(), *cP = cC + (size_t)NM * REC;
  for (int m = 0; m < NM; ++m) {
    const double *a = R->A + (size_t)m * n1;
    for (int e = 0; e < NX; ++e) cC[m * REC + e] = a[e];
    for (int i = 0; i < NPK; ++i) cC[m * REC + NX + i] = a[pr[i]] * a[pc[i]];
    for (int e = 0; e < 6; ++e) cP[m * 6 + e] = a[e];
  }
  // Model rows and tables staged in LDS when they fit; otherwise (NM above ~75 at the
  // default grid, or MPCEKF_ROM_GLOBAL=1) only the tables are, and the model rows are read
  // from the global blob (L2-resident).  Same arithmetic either way.
  auto lds_need = [&]() { return std::max(std::max(cell_lds_bytes(r), bounds_lds_bytes(r, 1024)), plant_lds_bytes(r)); };
  const char *gev = getenv("MPCEKF_ROM_GLOBAL");
  r.rom_global = gev && atoi(gev) == 1;
  // the plant's extras (res0 column, Cdleff tables) only while the whole cell blob still
  // fits the LDS; otherwise the plain blob and the separate k_plant
  if (cell_plant && !r.rom_global && cell_lds_bytes(r) > 160 * 1024) make_cell_blob(false);
  if (lds_need() > 160 * 1024) r.rom_global = 1;
  if (lds_need() > 160 * 1024)
    return fail(MPCEKF_E_UNSUPPORTED, "rom: %d bytes of electrode tables exceed the 160 KiB LDS", lds_need());
  // --- OB_step's obs output (mpcekf_plant_step_obs): record layout, row descriptors and a
  // blob of its own with every row's C, res0 and D (the plant and cell blobs stay as they
  // are); host memory only, uploaded by the first obs call ---
  {
    int32_t *off = X->obs_off;
    static const int vec_field[MPCEKF_TF_COUNT] = {
        MPCEKF_OBS_negIfdl, MPCEKF_OBS_posIfdl, MPCEKF_OBS_negIf, MPCEKF_OBS_posIf, MPCEKF_OBS_negIdl,
        MPCEKF_OBS_posIdl, MPCEKF_OBS_negPhis, MPCEKF_OBS_posPhis, MPCEKF_OBS_negPhise, MPCEKF_OBS_posPhise,
        MPCEKF_OBS_negThetass, MPCEKF_OBS_posThetass, MPCEKF_OBS_Phie, MPCEKF_OBS_Phie, MPCEKF_OBS_Phie,
        MPCEKF_OBS_Thetae, MPCEKF_OBS_Thetae, MPCEKF_OBS_Thetae};
    static const int row_kind[MPCEKF_TF_COUNT] = {
        OBS_PLAIN, OBS_PLAIN, OBS_PLAIN, OBS_PLAIN, OBS_PLAIN, OBS_PLAIN, OBS_PLAIN, OBS_PPHIS, OBS_NPHISE,
        OBS_PPHISE, OBS_NTHSS, OBS_PTHSS, OBS_PHIE, OBS_PHIE, OBS_PHIE, OBS_THETAE, OBS_THETAE, OBS_THETAE};
    int len[MPCEKF_OBS_COUNT];
    for (int f = 0; f < MPCEKF_OBS_COUNT; ++f) len[f] = 1;  // the scalars; the vector fields follow
    for (int code = 0; code <= MPCEKF_TF_posThetass; ++code) len[vec_field[code]] = (int)rows_of(code).size();
    len[MPCEKF_OBS_Phie] = (int)Phie.size() + 1;  // OB_step.m:320
    len[MPCEKF_OBS_Thetae] = (int)Thetae.size();
    off[0] = 0;
    for (int f = 0; f < MPCEKF_OBS_COUNT; ++f) off[f + 1] = off[f] + len[f];
    KObs &ko = X->ko;
    ko = KObs{};
    ko.nobs = off[MPCEKF_OBS_COUNT];
    ko.slot_phie0 = off[MPCEKF_OBS_Phie];
    std::vector<int> slot1(nz, -1), slot2(nz, -1);
    for (int code = 0; code <= MPCEKF_TF_posThetass; ++code) {
      const std::vector<int> v = rows_of(code);
      for (size_t i = 0; i < v.size(); ++i) slot1[v[i]] = off[vec_field[code]] + (int)i;
    }
    for (size_t i = 0; i < Phie.size(); ++i) slot1[Phie[i]] = off[MPCEKF_OBS_Phie] + 1 + (int)i;
    for (size_t i = 0; i < Thetae.size(); ++i) slot1[Thetae[i]] = off[MPCEKF_OBS_Thetae] + (int)i;
    slot2[role[R_IFDL0]] = off[MPCEKF_OBS_negIfdl0];
    slot2[role[R_IFDL3]] = off[MPCEKF_OBS_posIfdl3];
    slot2[role[R_IF0]] = off[MPCEKF_OBS_negIf0];
    slot2[role[R_IF3]] = off[MPCEKF_OBS_posIf3];
    slot2[role[R_TH0]] = off[MPCEKF_OBS_negThetass0];
    slot2[role[R_TH3]] = off[MPCEKF_OBS_posThetass3];
    slot2[role[R_PHISE0]] = off[MPCEKF_OBS_negPhise0];
    if (nz > OBS_MAXROWS || ko.nobs > 1023) return fail(MPCEKF_E_UNSUPPORTED, "rom: nz = %d rows exceed the obs record", nz);
    for (int p = 0; p < nz; ++p) {
      const int q = perm[p];
      ko.desc[p] = (unsigned)row_kind[R->tf_code[q]] | (unsigned)(slot1[q] + 1) << 4 | (unsigned)(slot2[q] + 1) << 14;
    }
    // mpcekf_step_ex_obs: where each record slot comes from (a permuted row or OBS_SRC_*)
    X->obs_slot_src.assign((size_t)ko.nobs, OBS_SRC_VCELL);
    for (int p = 0; p < nz; ++p) {
      if (slot1[perm[p]] >= 0) X->obs_slot_src[slot1[perm[p]]] = p;
      if (slot2[perm[p]] >= 0) X->obs_slot_src[slot2[perm[p]]] = p;
    }
    X->obs_slot_src[OBS_S_NEGSOC] = OBS_SRC_NEGSOC;
    X->obs_slot_src[OBS_S_POSSOC] = OBS_SRC_POSSOC;
    X->obs_slot_src[OBS_S_CELLSOC] = OBS_SRC_CELLSOC;
    X->obs_slot_src[ko.slot_phie0] = OBS_SRC_PHIE0;
    ko.stride = nz * OBS_ROW;
    std::vector<double> &ob = X->h_obs_blob;
    ob.assign((size_t)NM * ko.stride, 0.0);
    for (int m = 0; m < NM; ++m)
      for (int p = 0; p < nz; ++p) {
        double *b = ob.data() + (size_t)m * ko.stride + (size_t)p * OBS_ROW;
        const int q = perm[p], code = R->tf_code[q];
        for (int k = 0; k < NX; ++k) b[k] = Cval(m, q, k);
        // OB_step.m:178-181: res0 removed from the Phise rows
        b[NX] = (code == MPCEKF_TF_negPhise || code == MPCEKF_TF_posPhise) ? 0.0 : Cval(m, q, NX);
        b[NX + 1] = Dval(m, q);
      }
    ko.tab = (int)ob.size();  // NM * nz * 8: even
    ko.tablen = (int)tabs.size();
    ob.insert(ob.end(), tabs.begin(), tabs.end());
    ob.insert(ob.end(), pts.begin(), pts.end());
    ko.len = (int)ob.size();
    ko.global = r.rom_global;
    if (obs_lds_bytes(ko) > 160 * 1024) ko.global = 1;  // the tables alone fit: lds_need above
  }
  int rc;
  if (poly) {
    if ((rc = dalloc(&X->d_poly, ptab.size()))) return rc;
    HIPCHK(hipMemcpy(X->d_poly, ptab.data(), ptab.size() * 8, hipMemcpyHostToDevice));
    r.poly = X->d_poly;
  }
  if ((rc = dalloc(&X->d_cell_blob, cb.size()))) return rc;
  if ((rc = dalloc(&X->d_plant_blob, pb.size()))) return rc;
  if ((rc = dalloc(&X->d_bulk, bt.size()))) return rc;
  HIPCHK(hipMemcpy(X->d_cell_blob, cb.data(), cb.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(X->d_plant_blob, pb.data(), pb.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(X->d_bulk, bt.data(), bt.size() * 8, hipMemcpyHostToDevice));
  r.cell_blob = X->d_cell_blob;
  r.plant_blob = X->d_plant_blob;
  r.bulk_tab = X->d_bulk;
  X->NM = NM;
  X->nz = nz;
  X->nzp = nzp;
  return MPCEKF_OK;
}

static int check_cfg(const mpcekf_config *c) {
  if (!(c->Np == 5 && c->Nc == 2) && !wide_supported(c->Np, c->Nc))
    return fail(MPCEKF_E_UNSUPPORTED, "Np=%d Nc=%d: this build compiles the GPU step for Np/Nc = 5/2 and 20/10",
                c->Np, c->Nc);
  if (sw_of(c) != 7 && !(c->Np == 5 && c->Nc == 2))
    return fail(MPCEKF_E_UNSUPPORTED,
                "Np=%d Nc=%d with a constraint switch off: the switches are built for Np/Nc = 5/2 only "
                "(this horizon needs all three on)", c->Np, c->Nc);
  if (c->max_hild < 1) return fail(MPCEKF_E_ARG, "max_hild < 1");
  if (c->method != MPCEKF_METHOD_OB && c->method != MPCEKF_METHOD_MB)
    return fail(MPCEKF_E_ARG, "method %d: expected MPCEKF_METHOD_OB or _MB (initKF.m:44-49)", c->method);
  return MPCEKF_OK;
}

static void fill_kcfg(const mpcekf_config *c, double Q, KCfg &k) {
  k.SigmaV = c->SigmaV;
  k.SigmaW = c->SigmaW;
  k.ref = c->target_soc;
  k.u_max = c->u_max;
  k.u_min = -Q * c->Crate;  // initMPC.m:66-67
  k.du_min = c->du_min;
  k.du_max = c->du_max;
  k.v_max = c->v_max;
  k.phise_min = c->phise_min;
  k.zmax = c->z_max + c->z_tol;  // constraintsMPC.m:90-91
  k.hild_tol = c->hild_tol;
  k.max_warn = c->max_warn;
  k.max_hild = c->max_hild;
  k.flags = c->flags | (c->method == MPCEKF_METHOD_MB ? KF_MB : 0);
}

int mpcekf_ctx_create(const mpcekf_rom *rom, const mpcekf_config *cfg, int device, int64_t ncells,
                      mpcekf_ctx **out) {
  if (!out || !cfg || ncells < 0) return fail(MPCEKF_E_ARG, "ctx_create: bad argument");
  *out = nullptr;
  int rc = check_cfg(cfg);
  if (rc) return rc;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPCEKF_E_ARG, "device %d of %d", device, ndev);
  HIPCHK(hipSetDevice(device));
  mpcekf_ctx *X = new (std::nothrow) mpcekf_ctx();
  if (!X) return fail(MPCEKF_E_ARG, "out of host memory");
  X->device = device;
  X->n = ncells;
  X->cfg = *cfg;
  X->sw = sw_of(cfg);
  X->ncon_dev = ncon_of(cfg->Np, cfg->Nc);
  X->ncon = ncon_sw_of(cfg->Np, cfg->Nc, X->sw);
  X->wide = wide_supported(cfg->Np, cfg->Nc);
  X->mb = cfg->method == MPCEKF_METHOD_MB;
  if ((rc = build_rom(X, rom))) { mpcekf_ctx_destroy(X); return rc; }
  fill_kcfg(cfg, rom->Q, X->k);
  // Diagnostic override (tests/test_gpu_parity.py shows results do not depend on it):
  // MPCEKF_FLUSH_PERIOD in [1, LAZY_H].
  if (const char *e = std::getenv("MPCEKF_FLUSH_PERIOD")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= LAZY_H) X->flush_period = v;
  }
  // MPCEKF_SPLIT_CELL=1: the fused step's k_cell as two kernels (results identical).
  if (const char *e = std::getenv("MPCEKF_SPLIT_CELL")) X->split_cell = std::atoi(e) != 0;
  // k_ekf4 (a lane quad per cell for iterEKF; needs four distinct corners: nT > 1, nZ > 1).
  // Round 2 measured it against k_cell under 128 / 256-register budgets (512- / 1024-thread
  // blocks): it lost at every batch size (0.080 vs 0.075 ms at 1,024 cells, 0.20 vs 0.11 at
  // 65,536; profiles/r02g_*).  Round 5's small-batch mapping is the 256-thread instantiation
  // (512 registers, no spills) spread one wave per CU, chosen for batches up to
  // MPCEKF_QUAD_MAX cells, default 8,192 (results identical whichever path runs; same-box
  // A/B, profiles/r05e_small_batch.txt: 1,024 cells 0.173 -> 0.160 ms per step, 4,096 0.176
  // -> 0.164, 16,384 0.189 either way).  MPCEKF_QUAD=0/1 forces it.
  // A context with a constraint switch off runs k_cell<P_EKF | P_LIN> + mpcekf_switch.hip's
  // kernels at every batch size (no k_ekf4 mapping, no MPCEKF_SPLIT_CELL form).
  if (X->sw != 7) X->split_cell = false;
  const bool quad_ok = rom->nT > 1 && rom->nZ > 1 && cfg->method == MPCEKF_METHOD_OB && !X->wide && X->sw == 7;
  {
    int64_t quad_max = 8192;
    if (const char *e = std::getenv("MPCEKF_QUAD_MAX")) quad_max = std::atoll(e);
    X->quad = quad_ok && ncells <= quad_max;
  }
  X->ekf4_block = 256;
  if (const char *e = std::getenv("MPCEKF_QUAD")) X->quad = quad_ok && std::atoi(e) != 0;
  if (const char *e = std::getenv("MPCEKF_EKF4_BLOCK")) {
    const int v = std::atoi(e);
    X->ekf4_block = v == 1024 || v == 512 ? v : 256;
  }
  if (const char *e = std::getenv("MPCEKF_GRAPH")) X->graph = std::atoi(e) != 0;  // as mpcekf_set_graph
  // MPCEKF_FLUSH_ROLL=1: the rolling flush schedule (results identical)
  if (const char *e = std::getenv("MPCEKF_FLUSH_ROLL")) X->flush_roll = std::atoi(e) != 0;
  {
    int64_t side_max = 0;
    if (const char *e = std::getenv("MPCEKF_BOUNDS_SIDE")) side_max = std::atoll(e);
    if (const char *e = std::getenv("MPCEKF_BOUNCE_MAX")) X->bounce_max = (size_t)std::atoll(e);
    if (const char *e = std::getenv("MPCEKF_CHUNK")) X->xchunk = std::max<size_t>((size_t)std::atoll(e), 4096);
    X->bounds_side = ncells <= side_max;
  }
  X->copier = new (std::nothrow) Copier();
  if (!X->copier) { mpcekf_ctx_destroy(X); return fail(MPCEKF_E_HIP, "out of host memory"); }
  X->copier->start(copy_threads(), device);
  hipError_t e = hipStreamCreateWithFlags(&X->stream, hipStreamNonBlocking);
  if (e == hipSuccess && (X->flush_roll || X->bounds_side)) {
    e = hipStreamCreateWithFlags(&X->fstream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&X->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&X->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&X->ev_bfork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&X->ev_bjoin, hipEventDisableTiming);
  }
  if (e != hipSuccess) { mpcekf_ctx_destroy(X); return fail(MPCEKF_E_HIP, "stream: %s", hipGetErrorString(e)); }
  const size_t n = (size_t)ncells, NM = (size_t)X->NM;
  KState &s = X->s;
  s.n = ncells;
  if ((rc = dalloc(&s.bigx, n * NM * 6)) || (rc = dalloc(&s.ekf, n * NM * REC)) ||
      (rc = dalloc(&X->d_scal, n * 10)) || (rc = dalloc(&s.lam, n * X->ncon_dev)) ||
      (rc = hipMalloc((void **)&X->d_int, (n * 4 + 1) * sizeof(int)) == hipSuccess ? 0 : MPCEKF_E_HIP) || (rc = dalloc(&X->d_prob, n * PROB_DOUBLES)) || (rc = dalloc(&X->d_const, n * 8)) ||
      (rc = dalloc(&X->d_zk, n * (X->nz + 2))) || (rc = dalloc(&X->d_zbk, n * (X->nz + 2))) ||
      (rc = dalloc(&X->d_bnd, n * NBND)) || (rc = dalloc(&X->d_xg, n * 4)) ||
      (rc = hipMalloc((void **)&X->d_xm, n * 4 * sizeof(int)) == hipSuccess ? 0 : MPCEKF_E_HIP) ||
      (rc = dalloc(&X->d_ts, n * NM * 2)) || (rc = dalloc(&X->d_hist, n * LAZY_H * 2)) ||
      (X->mb && (rc = dalloc(&X->d_mb, n * MBREC)))
#ifdef MPCEKF_STAMPS
      || (rc = dalloc(&X->d_stamps, n * NSTAMPS))
#endif
  ) {
    mpcekf_ctx_destroy(X);
    return rc;
  }
  double *sc = X->d_scal;
  s.SOCn = sc; s.SOCp = sc + n; s.x0 = sc + 2 * n; s.S0 = sc + 3 * n; s.priorI = sc + 4 * n;
  s.uk_1 = sc + 5 * n; s.uk = sc + 6 * n; s.vk = sc + 7 * n; s.J_unc = sc + 8 * n; s.J_fin = sc + 9 * n;
  s.warn = X->d_int; s.status = X->d_int + n; s.nviol = X->d_int + 2 * n; s.hflag = X->d_int + 3 * n;
  s.hslow = X->d_int + 4 * n;
  HIPCHK(hipMemset(s.hslow, 0, sizeof(int)));
  s.prob = X->d_prob;
  s.ts_ekf = X->d_ts; s.ts_plant = X->d_ts + n * NM;
  s.hist_p = X->d_hist; s.hist_u = X->d_hist + n * LAZY_H;
  s.mb = X->d_mb;
  s.stamps = X->d_stamps;
  {
    // MPCEKF_HOT_CORNERS=0/1: the corner window off / on where eligible (default on).  The
    // quad route's k_ekf4 and the MB filter do not know it, and the rolling flush runs its
    // slices beside k_bounds, which reads the window.  An allocation that fails leaves the
    // context without a window, not without a context.
    bool hot = true;
    if (const char *e = std::getenv("MPCEKF_HOT_CORNERS")) hot = std::atoi(e) != 0;
    if (hot && !X->mb && !X->quad && !X->flush_roll && n > 0) {
      if (hipMalloc((void **)&X->d_hot, n * 4 * REC * sizeof(double)) != hipSuccess ||
          hipMalloc((void **)&X->d_hot_i, n * 8 * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        if (X->d_hot) (void)hipFree(X->d_hot);
        if (X->d_hot_i) (void)hipFree(X->d_hot_i);
        X->d_hot = nullptr;
        X->d_hot_i = nullptr;
      } else {
        s.hot_rec = X->d_hot;
        s.hot_m = X->d_hot_i;
        s.hot_ts = X->d_hot_i + n * 4;
      }
    }
    // MPCEKF_HOT_PLANT=0/1: the plant window, for the same contexts when cell_plant runs the
    // plant in k_cell (a ROM whose plant stays in k_plant4 gets none)
    bool hotp = true;
    if (const char *e = std::getenv("MPCEKF_HOT_PLANT")) hotp = std::atoi(e) != 0;
    if (hotp && !X->mb && !X->quad && !X->flush_roll && X->r.cell_plant && n > 0) {
      if (hipMalloc((void **)&X->d_hotp, n * 4 * 6 * sizeof(double)) != hipSuccess ||
          hipMalloc((void **)&X->d_hotp_i, n * 8 * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        if (X->d_hotp) (void)hipFree(X->d_hotp);
        if (X->d_hotp_i) (void)hipFree(X->d_hotp_i);
        X->d_hotp = nullptr;
        X->d_hotp_i = nullptr;
      } else {
        s.hotp_x = X->d_hotp;
        s.hotp_m = X->d_hotp_i;
        s.hotp_ts = X->d_hotp_i + n * 4;
      }
    }
    if ((rc = X->hot_clear())) { mpcekf_ctx_destroy(X); return rc; }
  }
  // rows the current launch sequence does not write (k_plant's 12..19 when the plant runs
  // inside k_cell) read back as zero, never as stale allocation contents
  if (X->d_stamps) HIPCHK(hipMemset(X->d_stamps, 0, (size_t)n * NSTAMPS * sizeof(long long)));
  double *cs = X->d_const;
  s.Tc = cs; s.SOC0 = cs + n; s.SOC0n = cs + 2 * n; s.SOC0p = cs + 3 * n;
  if (X->sw != 7 && ((rc = dalloc(&X->d_lin, n * MPCEKF_LIN_SIZE)) || (rc = dalloc(&X->d_zsoc, n)))) {
    mpcekf_ctx_destroy(X);  // the hand-off k_cell<P_EKF | P_LIN> -> k_mpc_sw
    return rc;
  }
  if (X->wide) {
    KWide &w = X->w;
    w.Np = cfg->Np; w.Nc = cfg->Nc; w.ncon = X->ncon;
    const size_t nc = (size_t)X->ncon;
    if ((rc = dalloc(&w.prob, n * wide_prob_doubles(w.Np, w.Nc))) || (rc = dalloc(&w.X, nc * n * w.Nc)) ||
        (rc = dalloc(&w.R, (size_t)n * (w.Nc * (w.Nc + 1) / 2))) || (rc = dalloc(&w.K, nc * n)) || (rc = dalloc(&w.hii, nc * n)) || (rc = dalloc(&w.it, n)) ||
        (rc = dalloc(&w.smin, (size_t)w.Nc * w.Nc + 1)) || (rc = dalloc(&X->d_lin, n * MPCEKF_LIN_SIZE)) ||
        (rc = dalloc(&w.q, 1)) || (rc = dalloc(&w.list, n)) || (rc = dalloc(&w.hist, 128)) ||
        (rc = dalloc(&X->d_zsoc, n))) {
      mpcekf_ctx_destroy(X);
      return rc;
    }
    HIPCHK(hipMemset(w.q, 0, sizeof(int)));
    HIPCHK(hipMemset(w.hist, 0, 128 * sizeof(int)));
    HIPCHK(hipMemset(w.it, 0, n * sizeof(int)));  // the first step's sweep prediction
    // mpc_setup's sigma_min cache: GsocT*Gsoc for Csoc = [0 0 0 0 0 -Ts/(3600 Q)] (EKFmatsHandler.m:43-45)
    rc = launch_wide_smin(w, -rom->Ts / (3600 * rom->Q), rom->A, X->stream);
    if (rc) { mpcekf_ctx_destroy(X); return fail(MPCEKF_E_HIP, "smin kernel: %s", hipGetErrorString((hipError_t)rc)); }
    HIPCHK(hipStreamSynchronize(X->stream));
  }
  *out = X;
  return MPCEKF_OK;
}

int mpcekf_ctx_destroy(mpcekf_ctx *X) {
  if (!X) return MPCEKF_OK;
  (void)hipSetDevice(X->device);
  if (X->stream) (void)X->drain();  // pending _async copies finish before their buffers go
  if (X->fstream) (void)hipStreamSynchronize(X->fstream);
  delete X->copier;
  X->copier = nullptr;
  for (hipEvent_t e : X->xev) (void)hipEventDestroy(e);
  for (hipEvent_t e : X->ev) (void)hipEventDestroy(e);
  if (X->ev_fork) (void)hipEventDestroy(X->ev_fork);
  if (X->ev_join) (void)hipEventDestroy(X->ev_join);
  if (X->ev_bfork) (void)hipEventDestroy(X->ev_bfork);
  if (X->ev_bjoin) (void)hipEventDestroy(X->ev_bjoin);
  void *ptrs[] = {X->d_prob, X->d_cell_blob, X->d_plant_blob, X->d_bulk, X->d_const, X->d_scal, X->d_int, X->d_zk,
                  X->d_zbk,       X->d_tmp,        X->s.bigx, X->s.ekf,   X->s.lam,   X->d_ts, X->d_hist, X->d_stamps, X->d_bnd, X->d_xm, X->d_xg,
                  X->w.prob, X->w.X, X->w.R, X->w.K, X->w.hii, X->w.it, X->w.smin, X->d_lin, X->d_zsoc, X->d_mb, X->d_uk1p,
                  X->w.q, X->w.list, X->w.hist, X->d_poly, X->d_szk, X->d_sxg, X->d_sxm, X->d_slin, X->d_sv, X->d_zslot,
                  X->d_obs_blob, X->d_obs, X->d_obs_plan, X->d_lim, X->d_sch_hdr, X->d_sch_tab, X->d_sch_val, X->d_sch_set, X->d_lm_hdr, X->d_lm_tab, X->d_lm_val, X->d_lm_set, X->d_lm, X->d_lm_soc, X->d_sum, X->d_sum_reach, X->d_sum_obs,
                  X->d_sum_ring, X->d_pk, X->d_tc, X->d_tc_link, X->d_tc_snap, X->d_ag, X->d_ag_par, X->d_ag_phi, X->d_ag_obs, X->d_ag_plan, X->d_tm, X->d_tm_par, X->d_tm_soc, X->d_tm_int, X->d_bl, X->d_bl_par, X->d_bl_soc, X->d_bl_on, X->d_ch, X->d_ch_par, X->d_th, X->d_th_par, X->d_th_i, X->d_th_ocv, X->d_hot, X->d_hot_i, X->d_hotp, X->d_hotp_i};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (auto &g : X->graphs) (void)hipGraphExecDestroy(g.exec);
  if (X->h_bounce) (void)hipHostFree(X->h_bounce);
  if (X->fstream) (void)hipStreamDestroy(X->fstream);
  if (X->stream) (void)hipStreamDestroy(X->stream);
  delete X;
  return MPCEKF_OK;
}

int mpcekf_ctx_config(const mpcekf_ctx *X, mpcekf_config *cfg) {
  if (!X || !cfg) return fail(MPCEKF_E_ARG, "ctx_config: null argument");
  *cfg = X->cfg;
  return MPCEKF_OK;
}

int mpcekf_ctx_info(const mpcekf_ctx *X, int64_t *ncells, int32_t *nmodels, int32_t *nz, int32_t *ncon) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  if (ncells) *ncells = X->n;
  if (nmodels) *nmodels = X->NM;
  if (nz) *nz = X->nz;
  if (ncon) *ncon = X->ncon;
  return MPCEKF_OK;
}

// soc(z,T) on the host, the sequence of ETab::bracket / ETab::soc (and orc tidx / fsoc)
static double host_soc(const mpcekf_ctx *X, int side, double z, double T) {
  const std::vector<double> &tk = X->tabT;
  const int nte = (int)tk.size();
  const std::vector<double> &a = X->soc_end[side][0], &b = X->soc_end[side][1];
  if (nte == 1) return a[0] + z * (b[0] - a[0]);
  const double Tc = std::fmin(std::fmax(T, tk[0]), tk[nte - 1]);
  int j = 0;
  while (j < nte - 2 && Tc >= tk[j + 1]) ++j;
  const double g = (Tc - tk[j]) / (tk[j + 1] - tk[j]);
  const double s0 = a[j] + g * (a[j + 1] - a[j]), s1 = b[j] + g * (b[j + 1] - b[j]);
  return s0 + z * (s1 - s0);
}

static int check_tc(const double *tc, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!(tc[i] <= 100) || !std::isfinite(tc[i]))
      return fail(MPCEKF_E_ARG, "temperature %zu = %g: must be finite and in degC (iterEKF.m:62)", i, tc[i]);
  return MPCEKF_OK;
}

// A stage call's temperature argument (OB_step's Tc, iterEKF's / EKFmatsHandler's Tk)
// becomes the cell's temperature for this and later calls.
static int set_tc(mpcekf_ctx *X, const double *tc, struct Xfer *xf = nullptr);

// initKF.m:30-136, initMPC.m:29-74 and OB_step.m:39-72 for every cell.
int mpcekf_init_cells(mpcekf_ctx *X, const double *soc0_pct, const double *tc_degC) {
  if (X) X->stage_zk = X->stage_lin = X->stage_v = X->stage_obs = false;  // the stage route's device hand-offs are stale
  if (!X || ((!soc0_pct || !tc_degC) && X->n)) return fail(MPCEKF_E_ARG, "init_cells: null argument");
  HIPCHK(hipSetDevice(X->device));
  const size_t n = (size_t)X->n;
  int rc0 = 0;
  if ((X->n && (rc0 = check_tc(tc_degC, n)))) return rc0;
  std::vector<double> cst(n * 8), sc(n * 10, 0.0);
  for (size_t c = 0; c < n; ++c) {
    double tc = tc_degC[c], soc0 = soc0_pct[c];
    double T = tc + 273.15;  // OB_step.m:63
    double z = soc0 / 100;
    cst[0 * n + c] = tc;
    cst[1 * n + c] = z;                              // ekfData.SOC0 (initKF.m:133)
    cst[2 * n + c] = host_soc(X, 0, z, T);           // SOC0n = soc(SOC0/100, Tk1) (OB_step.m:64)
    cst[3 * n + c] = host_soc(X, 1, z, T);           // SOC0p
    sc[0 * n + c] = cst[2 * n + c];  // SOCnAvg
    sc[1 * n + c] = cst[3 * n + c];  // SOCpAvg
    sc[3 * n + c] = X->cfg.SigmaX0[5];  // ekfData.SigmaX0 (initKF.m:99)
  }
  HIPCHK(hipMemcpyAsync(X->d_const, cst.data(), cst.size() * 8, hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipMemcpyAsync(X->d_scal, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipMemsetAsync(X->s.lam, 0, n * X->ncon_dev * 8, X->stream));
  HIPCHK(hipMemsetAsync(X->d_int, 0, n * 4 * sizeof(int), X->stream));
  HIPCHK(hipMemsetAsync(X->d_ts, 0, n * X->NM * 2 * sizeof(int), X->stream));  // every model current
  if ((rc0 = X->hot_clear())) return rc0;  // and every record in s.ekf
  int rc = launch_init_state(X->n, X->NM, X->s.ekf, X->s.bigx, X->cfg.SigmaX0, X->stream);
  if (rc) return fail(MPCEKF_E_HIP, "init kernel: %s", hipGetErrorString((hipError_t)rc));
  if (X->mb) {  // initKF.m:47-48,111-112: xhat = 0, SigmaX = SigmaX0 (6x6)
    std::vector<double> mbs(n * MBREC, 0.0);
    for (size_t c = 0; c < n; ++c)
      for (int p = 0; p <= NX; ++p) mbs[c * MBREC + 6 + p * (NX + 1) + p] = X->cfg.SigmaX0[p];
    HIPCHK(hipMemcpyAsync(X->d_mb, mbs.data(), mbs.size() * 8, hipMemcpyHostToDevice, X->stream));
    HIPCHK(hipStreamSynchronize(X->stream));
  }
  HIPCHK(hipStreamSynchronize(X->stream));
  X->initialized = true;
  return MPCEKF_OK;
}

static int need_init(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  if (!X->initialized) return fail(MPCEKF_E_STATE, "call mpcekf_init_cells first");
  HIPCHK(hipSetDevice(X->device));
  return MPCEKF_OK;
}

static int lerr(int rc, const char *what) {
  if (rc) return fail(MPCEKF_E_HIP, "%s launch: %s", what, hipGetErrorString((hipError_t)rc));
  return MPCEKF_OK;
}

// What a fused call returns beyond mpcekf_traj and the obs rows: every entry point fills the
// members it has, by name.
struct StepOut {
  bool sum = false;  // mpcekf_step_summary's call: the rows go to the context's window
  double *temp = nullptr, *heat = nullptr, *ucmd = nullptr;
  int32_t *limiter = nullptr;
  double *rate = nullptr, *cond = nullptr, *bleed = nullptr, *zmin = nullptr, *vstr = nullptr, *istr = nullptr;
  int32_t *capby = nullptr;
  double *lim = nullptr;  // [nsteps][nf][ncells] of the map in force
};

// runMPC.m:84-111, nsteps times: OB_step -> (all-model advance + EKF time
// update) -> iterEKF measurement update -> EKFmatsHandler -> iterMPC.
// nslots > 0 (mpcekf_step_ex_obs): k_obs_traj first in every step, its rows one more output
// field; nslots == 0 is mpcekf_step_ex: the same launches, allocations and copies as ever.
// sum (mpcekf_step_summary): no trajectory leaves the call; the u, v, soc, phise, nexec rows
// (and the record's obs slot) of step k go to row k % SUM_WIN of the context's window, which
// k_summary folds into the record every SUM_WIN steps and after the last.  The per-step
// temperatures are uploaded a window at a time, so no device buffer of the call grows with
// nsteps.
// A thermal context (mpcekf_thermal_begin): k_thermal last in every step advances s.Tc, which
// the next step's kernels read (tc_in stays null); temp / heat (mpcekf_step_ex_thermal) are two
// more [nsteps][ncells] output fields, written by k_thermal.
// A pack context (mpcekf_pack_begin): k_pack after Hildreth and k_cl_diag replaces each cell's
// command in s.uk, s.uk_1 and the u row by its string's current, before the summary fold and
// k_thermal read them; ucmd [nsteps][ncells] and limiter [nsteps][ncells / series]
// (mpcekf_step_ex_pack) are two more output fields, written by k_pack.
// An aging context (mpcekf_aging_begin): k_aging before k_thermal reads the step's phise row
// (source EST; the context's own row when the call has none) and the step's negPhise0 row
// (source PLANT; from the call's obs rows when its slots name it, else from a one-position
// k_obs_traj launch of the context's own, which leaves the caller's rows what they were); rate
// [nsteps][nsrc * nreact][ncells] (mpcekf_step_ex_aging) is one more output field, written by
// k_aging.
// A terminating context (mpcekf_term_begin): k_term after Hildreth and k_cl_diag, before k_pack,
// applies the termination rule to every cell and rests the latched ones (+0.0 in s.uk, s.uk_1
// and the u row); it reads the step's soc row (the context's own when the call has none) and,
// on a pack, the string flags of the step's call-relative parity, seeded once per call.
// A balancing context (mpcekf_balance_begin, on a pack): k_pack_bal in k_pack's place reads the
// step's soc row (the context's own when the call has none) and the cells' flags, and stores the
// applied currents; bleed [nsteps][ncells] and zmin [nsteps][ncells / series]
// (mpcekf_step_ex_balance) are two more output fields, written by that kernel.
// A charger context (mpcekf_charger_begin, on a pack): k_charger in k_pack's or k_pack_bal's place
// also reads s.vk and stores the applied currents after the charger's caps; vstr, istr
// [nsteps][ncells / series] and capby likewise (mpcekf_step_ex_charger) are three more output
// fields, written by that kernel.
// A coupled context (mpcekf_thermal_couple): k_couple_seed once before the call's first step,
// and k_thermal_couple(_sched) in k_thermal(_sched)'s place reads each cell's neighbours from
// the snapshot of the step's parity; cond [nsteps][ncells] (mpcekf_step_ex_couple) is one more
// output field, written by that kernel.
// A mapped context (mpcekf_limit_map): k_map once before the call's first step; every step ends
// with k_thermal_map in k_thermal's place (a model), k_map_step after k_thermal_couple (links) or
// k_map_step alone (no model), which reads the step's soc row (the context's own when the call has
// none); lim [nsteps][nf][ncells] (mpcekf_step_ex_map) is one more output field: step k's block is
// written by the launch that evaluated the values step k reads.
static int step_impl(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                     const int32_t *slots, int32_t nslots, double *obs, int32_t outputs_on_device,
                     const StepOut &o = StepOut()) {
  const bool sum = o.sum;
  // a thermal context owns the temperature: refused before anything of the context changes
  if (X && X->d_th && tc_degC)
    return fail(MPCEKF_E_ARG, "step: tc_degC on a thermal context (mpcekf_thermal_begin): the model sets the temperature");
  if (X) X->stage_zk = X->stage_lin = X->stage_v = X->stage_obs = false;  // the stage route's device hand-offs are stale
  int rc = need_init(X);
  if (rc) return rc;
  if (nsteps < 0) return fail(MPCEKF_E_ARG, "nsteps < 0");
  const bool thermal = X->d_th != nullptr;
  const bool pack = X->d_pk != nullptr;
  const bool aging = X->d_ag != nullptr;
  const bool coupled = X->d_tc != nullptr;  // thermal && pack: either's end ends the coupling
  const bool term = X->d_tm != nullptr;
  const bool balance = pack && X->d_bl != nullptr;
  const bool charger = pack && X->d_ch != nullptr;
  const bool term_str = term && pack && X->pk_series > 1;  // strings whose cells follow their first latched one
  const bool ag_est = aging && (X->ag_sources & MPCEKF_AG_SRC_EST), ag_plant = aging && (X->ag_sources & MPCEKF_AG_SRC_PLANT);
  if (sum && X->sum_slot >= 0) {  // checked by mpcekf_summary_begin
    slots = &X->sum_slot;
    nslots = 1;
    obs = X->d_sum_obs;
  }
  if (nslots < 0 || (nslots && (!slots || !obs))) return fail(MPCEKF_E_ARG, "step_ex_obs: nslots < 0 or a null slots / obs");
  for (int i = 0; i < nslots; ++i)
    if (slots[i] < 0 || slots[i] >= X->ko.nobs)
      return fail(MPCEKF_E_ARG, "step_ex_obs: slot %d outside 0..%d", slots[i], X->ko.nobs - 1);
  if (tc_degC && !outputs_on_device && (rc = check_tc(tc_degC, (size_t)X->n * (size_t)nsteps))) return rc;
  mpcekf_traj none{};
  if (!tr) tr = &none;
  const bool bounds = X->cfg.flags & MPCEKF_CF_BOUNDS;
  if (tr->zbk && !bounds) return fail(MPCEKF_E_ARG, "step_ex: a boundzk trajectory needs MPCEKF_CF_BOUNDS");
  // boundzk from k_cell's / k_ekf4's hand-off record in k_bounds (MB writes boundzk in
  // k_cell, from its one 6x6 covariance), on the steps that can be read (below)
  // per-cell limits (mpcekf_set_limits): the split route at every batch size, no k_ekf4 mapping
  const double *lim = X->lim();
  const bool quad = X->quad && !lim, split_cell = X->split_cell && !lim;
  const bool bnd_kernel = bounds && !X->mb;
  // OB_step's simStep inside k_cell (KRom::cell_plant): no k_plant launch
  const bool plant_in_cell = X->r.cell_plant && !X->mb;  // k_cell, or k_ekf4's lane quad (quad_plant)
  // a constraint block off, or per-cell limits at Np = 5: the split route of mpcekf_switch.hip
  const bool switched = X->sw != 7 || (lim && !X->wide);
  const size_t n = (size_t)X->n, per = n * (size_t)nsteps, nzz = (size_t)X->nz + 2;
  // the output fields (F_*), their element size and elements per cell-step (rows: elements of
  // `width` per step where that is not ncells)
  const size_t nstr = pack ? n / (size_t)X->pk_series : 0;  // a string field has one element per string and step
  struct F {
    void *host;
    size_t esz, width;
    char *dev;
    size_t rows;
  } f[] = {{tr->u, 8, 1, nullptr},       {tr->v, 8, 1, nullptr},      {tr->soc, 8, 1, nullptr},
           {tr->phise, 8, 1, nullptr},   {tr->nexec, 4, 1, nullptr},  {tr->x, 8, 6, nullptr},
           {tr->zk, 8, nzz, nullptr},    {tr->zbk, 8, nzz, nullptr},  {tr->J_unc, 8, 1, nullptr},
           {tr->J_fin, 8, 1, nullptr},   {tr->norm_du, 8, 1, nullptr}, {tr->nviol, 4, 1, nullptr},
           {tr->poles, 8, 2 * NA, nullptr}, {tr->sv, 8, NA, nullptr},
           {nslots ? obs : nullptr, 8, (size_t)nslots, nullptr},  // [nsteps][nslots][ncells]
           {o.temp, 8, 1, nullptr},      {o.heat, 8, 1, nullptr},  // a thermal context's only
           {o.ucmd, 8, 1, nullptr},                                // a pack context's only
           {o.limiter, 4, 1, nullptr, nstr},
           // an aging context's only: [nsteps][nsrc * nreact][ncells]
           {o.rate, 8, aging ? (size_t)(((int)ag_est + (int)ag_plant) * X->ag_nreact) : 0, nullptr},
           {o.cond, 8, 1, nullptr},   // a coupled context's only
           {o.bleed, 8, 1, nullptr},  // a balancing context's only
           {o.zmin, 8, 1, nullptr, nstr},
           // a charger context's only
           {o.vstr, 8, 1, nullptr, nstr},
           {o.istr, 8, 1, nullptr, nstr},
           {o.capby, 4, 1, nullptr, nstr},
           {o.lim, 8, X->lmap ? (size_t)X->h_lm.nf : 0, nullptr}};  // a mapped context's only
  static_assert(sizeof(f) / sizeof(F) == NF, "f[] has one entry per F_* name, in that order");
  auto step_bytes = [&](const F &e) -> size_t { return (e.rows ? e.rows : n) * e.width * e.esz; };  // one step's block
  const double *dtc = tc_degC;  // [nsteps][n] device copy of the per-step temperatures
  // sum: rows of the window instead of rows of a trajectory, for outputs and temperatures alike
  const size_t ring = sum ? (size_t)SUM_WIN : 0;
  const bool tc_windows = sum && tc_degC && (size_t)nsteps > ring;  // uploaded window by window
  if (sum) {
    f[F_OBS].host = nullptr;  // the obs rows stay on the device
    for (int i = F_U; i <= F_NEXEC; ++i) f[i].dev = X->d_sum_ring + (size_t)(i - F_U) * X->sum_row();  // u .. nexec
    f[F_OBS].dev = nslots ? (char *)obs : nullptr;
    if (tc_degC) {
      const size_t rows = std::min((size_t)nsteps, ring);
      if ((rc = X->tmp(rows * n * 8 + 256))) return rc;
      if (!tc_windows) HIPCHK(hipMemcpyAsync(X->d_tmp, tc_degC, per * 8, hipMemcpyHostToDevice, X->stream));
      dtc = X->d_tmp;
    }
  } else if (outputs_on_device) {
    for (F &e : f) e.dev = (char *)e.host;
  } else {
    size_t need = tc_degC ? ((per * 8 + 255) & ~(size_t)255) : 0;
    for (F &e : f) need += e.host ? (((size_t)nsteps * step_bytes(e) + 255) & ~(size_t)255) : 0;
    if ((rc = X->tmp(need + 256))) return rc;
    char *p = (char *)X->d_tmp;
    for (F &e : f)
      if (e.host) { e.dev = p; p += ((size_t)nsteps * step_bytes(e) + 255) & ~(size_t)255; }
    if (tc_degC) {
      HIPCHK(hipMemcpyAsync(p, tc_degC, per * 8, hipMemcpyHostToDevice, X->stream));
      dtc = (const double *)p;
    }
  }
  auto row = [&](int i, int k) -> char * {  // step k's [ncells][width] block of field i
    return f[i].dev ? f[i].dev + (ring ? (size_t)k % ring : (size_t)k) * step_bytes(f[i]) : nullptr;
  };
  auto tc_row = [&](int k) -> const double * {  // step k's temperatures
    return dtc ? dtc + (ring ? (size_t)k % ring : (size_t)k) * n : nullptr;
  };
  // iterMPC.m:53-60 diagnostics: k_cl_diag after the step from its linearisation records
  // and the uk_1 the step's iterMPC used
  const bool diag = f[F_POLES].dev || f[F_SV].dev;
  if (diag && (rc = X->diag_bufs())) return rc;
  // the obs selection: each position's source and the shared values some position reads,
  // uploaded on the step's stream before the loop (and before a graph replay)
  KObsSel osel{};
  if (nslots) {
    if ((rc = X->obs_blob_buf())) return rc;
    if (X->obs_plan_cap < (size_t)nslots) {
      if (X->d_obs_plan) (void)hipFree(X->d_obs_plan);
      X->d_obs_plan = nullptr;
      X->obs_plan_cap = 0;
      const size_t cap = std::max((size_t)nslots, (size_t)X->ko.nobs);  // duplicates may exceed nobs
      HIPCHK(hipMalloc((void **)&X->d_obs_plan, cap * sizeof(int)));
      X->obs_plan_cap = cap;
    }
    std::vector<int> &plan = X->h_obs_plan;
    plan.resize((size_t)nslots);
    for (int i = 0; i < nslots; ++i) {
      const int src = plan[i] = X->obs_slot_src[slots[i]];
      const int kind = src >= 0 ? (int)(X->ko.desc[src] & 15u) : -1;
      if (src == OBS_SRC_VCELL || kind == OBS_PPHIS) osel.need |= OBS_NEED_V;
      if (src == OBS_SRC_PHIE0 || kind == OBS_NPHISE || kind == OBS_PHIE) osel.need |= OBS_NEED_UN;
      if (kind == OBS_PPHISE) osel.need |= OBS_NEED_UP;
    }
    HIPCHK(hipMemcpyAsync(X->d_obs_plan, plan.data(), (size_t)nslots * sizeof(int), hipMemcpyHostToDevice, X->stream));
    osel.plan = X->d_obs_plan;
    osel.nsel = nslots;
  }
  // source PLANT: the position of negPhise0 among the call's slots, or the context's own launch
  int ag_pos = -1;
  if (ag_plant) {
    for (int i = 0; i < nslots && ag_pos < 0; ++i)
      if (slots[i] == X->ag_slot) ag_pos = i;
    if (ag_pos < 0 && (rc = X->obs_blob_buf())) return rc;
  }
  constexpr int NEV = 8;  // events per step: plant | cell | bounds | hild (+ diag) |, then | flush |, hild start (side)
  if (X->timing && X->ev.size() < (size_t)nsteps * NEV) {
    size_t old = X->ev.size();
    X->ev.resize((size_t)nsteps * NEV);
    for (size_t i = old; i < X->ev.size(); ++i) HIPCHK(hipEventCreate(&X->ev[i]));
  }
  // Deferred all-model time update: step t advances only the models it
  // touches (k_plant: plant corners, k_cell: EKF corners); k_flush brings every model
  // current each LAZY_H steps and at the end of the call, so between calls (stage entry
  // points, get/set_state) every model is current, exactly as after eager updates.
  //
  // Rolling schedule (flush_roll, MPCEKF_FLUSH_ROLL=1): step t < nsteps flushes only the cells of
  // slice t % P (P = flush_period; slice j = [j n / P, (j + 1) n / P)), so each cell is still
  // flushed every P steps and no replay needs more than P <= LAZY_H ring entries.  The slice
  // runs on fstream, forked after k_cell and joined before the next step's k_plant: k_bounds
  // and Hildreth read no timestamp, ring or model record that k_flush writes (k_flush stores
  // only records older than t, and k_bounds reads the corner k_cell updated at t), and
  // k_plant(t + 1) overwrites the ring slot of step t + 1 - LAZY_H only after the join.  The
  // last step flushes every cell on the step's stream (timestamps 0, as before).  Under graph
  // capture the slices stay on the step's stream (same bits, no overlap).
  // (a summary call that uploads its temperatures window by window is not captured: the
  // uploads read the caller's array)
  const bool capturing = X->graph && !X->timing && nsteps > 0 && !tc_windows;
  const bool roll = X->flush_roll;
  const bool fork = roll && X->fstream && !capturing;
  // k_bounds beside Hildreth (bounds_side); under graph capture it stays on the step's stream
  const bool side = X->bounds_side && bnd_kernel && X->fstream && !capturing;
  const int hstart = side ? 7 : 3;  // the event that opens the Hildreth interval
  const int P = X->flush_period;
  std::vector<char> flushed((size_t)nsteps, 0);
  // boundzk and zk only where they can be read: on every step when the call has
  // their trajectory, else on the call's last step, whose values mpcekf_get_zk returns.  zk also
  // on every step of the two-kernel routes, whose k_cell<P_MPC> reads it back (io2.zk_in)
  const bool zk_readback = !(X->wide || switched) && (split_cell || quad);
  std::vector<char> bounded((size_t)nsteps, 0);  // the steps that launched k_bounds
  const bool sched = thermal && X->sched;
  const KSched ksch = X->ksched();
  const bool lmap = X->lmap;
  auto kmap_of = [&](int k_for, const double *soc, bool eval) {  // the evaluation whose values step k_for reads
    KMap g = X->kmap();
    g.soc = soc;
    g.eval = eval;
    g.count = 1;
    g.out = eval && k_for < nsteps ? (double *)row(F_LIM, k_for) : nullptr;
    return g;
  };
  auto run_steps = [&]() -> int {
    // the schedule at the temperature the call's first step finds (mpcekf_thermal_sched.hip);
    // before the first timing event, so no slot of mpcekf_set_timing counts it
    if (sched && nsteps > 0 && (rc = lerr(launch_sched(ksch, X->stream), "sched"))) return rc;
    // the map at Z_LAST and the temperature the call's first step finds (mpcekf_limit_map.hip)
    if (lmap && nsteps > 0 && (rc = lerr(launch_map(kmap_of(0, nullptr, true), X->stream), "map"))) return rc;
    // the temperatures the call's first step finds, for its neighbours (mpcekf_thermal_couple.hip)
    if (coupled && nsteps > 0 && (rc = lerr(launch_couple_seed(X->s.Tc, X->d_tc_snap, X->n, X->stream), "couple_seed")))
      return rc;
    // the strings that hold a latched cell as the call's first step finds them (mpcekf_term.hip)
    if (term_str && nsteps > 0) {
      HIPCHK(hipMemsetAsync(X->tm_flag(0), 0, 2 * n * sizeof(int), X->stream));
      if ((rc = lerr(launch_term_seed(X->d_tm, X->tm_flag(0), X->n, X->pk_series, X->stream), "term_seed"))) return rc;
    }
    for (int k = 0; k < nsteps; ++k) {
      const int t = k + 1;
      // sampled steps: every timing_every-th (k = every-1, 2 every-1, ...: with every dividing
      // the flush period these include the flush steps) and the last
      const bool sample = X->timing && ((k + 1) % X->timing_every == 0 || k == nsteps - 1);
      hipEvent_t *E = sample ? &X->ev[(size_t)k * NEV] : nullptr;
      if (E) HIPCHK(hipEventRecord(E[0], X->stream));
      if (tc_windows && (size_t)k % ring == 0)  // the window's temperatures, after the last window's kernels
        HIPCHK(hipMemcpyAsync(X->d_tmp, tc_degC + (size_t)k * n, std::min(ring, (size_t)(nsteps - k)) * n * 8,
                              hipMemcpyHostToDevice, X->stream));
      if (diag) HIPCHK(hipMemcpyAsync(X->d_uk1p, X->s.uk_1, n * 8, hipMemcpyDeviceToDevice, X->stream));
      // the current the call's first step applies, before a kernel overwrites s.uk; k_thermal
      // carries it from step to step (mpcekf_thermal.hip)
      if (thermal && k == 0) HIPCHK(hipMemcpyAsync(X->d_th_i, X->s.uk, n * 8, hipMemcpyDeviceToDevice, X->stream));
      if (nslots) {  // the plant's observables of step t, before anything advances the plant
        KObsSel ok = osel;
        ok.out = (double *)row(F_OBS, k);
        if ((rc = lerr(launch_obs_traj(X->r, X->s, X->ko, ok, t, tc_row(k), X->stream), "obs_traj"))) return rc;
      }
      if (ag_plant && ag_pos < 0) {  // the plant's negPhise0 of step t for k_aging, into the context's row
        KObsSel ok{};
        ok.plan = X->d_ag_plan;
        ok.nsel = 1;
        ok.need = X->ag_need;
        ok.out = X->d_ag_obs;
        if ((rc = lerr(launch_obs_traj(X->r, X->s, X->ko, ok, t, tc_row(k), X->stream), "obs_traj (aging)"))) return rc;
      }
      if (!plant_in_cell && (rc = lerr(launch_plant(X->r, X->s, X->s.uk, X->s.vk, t, tc_row(k), X->stream), "plant")))
        return rc;
      if (E) HIPCHK(hipEventRecord(E[1], X->stream));
      KIO io{};
      io.mode = MODE_FUSED;
      io.lazy_t = t;
      io.plant = plant_in_cell;
      io.tc_in = plant_in_cell ? tc_row(k) : nullptr;
      io.stamps = X->d_stamps;
      io.u = (double *)row(F_U, k);
      io.v = (double *)row(F_V, k);
      io.soc = (double *)row(F_SOC, k);
      io.phise = (double *)row(F_PHISE, k);
      if (ag_est && !io.phise) io.phise = X->d_ag_phi;  // k_aging's input when the call asks for no phise row
      if (term && !io.soc) io.soc = X->d_tm_soc;         // k_term's input when the call asks for no soc row
      if (balance && !io.soc) io.soc = X->d_bl_soc;      // k_pack_bal's likewise
      if (lmap && !io.soc) io.soc = X->d_lm_soc;         // the map's kernels' likewise
      io.nexec = (int *)row(F_NEXEC, k);
      io.x_out = (double *)row(F_X, k);
      const bool last = k == nsteps - 1;
      io.zk = f[F_ZK].dev ? (double *)row(F_ZK, k) : last || zk_readback ? X->d_zk : nullptr;
      double *zbk_k = f[F_ZBK].dev ? (double *)row(F_ZBK, k) : X->d_zbk;
      const bool zbk_step = bounds && (f[F_ZBK].dev || last);
      const bool bnd_step = bnd_kernel && zbk_step;  // k_cell's record and the k_bounds launch that reads it
      io.zbk = zbk_step ? zbk_k : nullptr;
      io.bnd = bnd_step ? X->d_bnd : nullptr;
      io.junc_out = (double *)row(F_JUNC, k);
      io.jfin_out = (double *)row(F_JFIN, k);
      io.normdu_out = (double *)row(F_NORMDU, k);
      io.nviol_out = (int *)row(F_NVIOL, k);
      if (diag) io.lin_out = X->d_lin;
      // wide horizons, or a constraint switch off: iterMPC in mpcekf_wide.hip / mpcekf_switch.hip
      // from the linearisation record
      KIO iow{};
      if (X->wide || switched) {
        io.lin_out = X->d_lin;
        io.zsoc_out = X->d_zsoc;
        if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream, P_EKF | P_LIN), "cell"))) return rc;
        iow.mode = MODE_FUSED;
        iow.lin_in = X->d_lin;
        iow.soc_k1_in = X->d_zsoc;
        iow.u = io.u;
        iow.nexec = io.nexec;
        iow.junc_out = io.junc_out;
        iow.jfin_out = io.jfin_out;
        iow.normdu_out = io.normdu_out;
        iow.nviol_out = io.nviol_out;
        if (switched) {
          if ((rc = lerr(launch_mpc_sw(X->sw, X->k, X->s, iow, X->stream, lim), "mpc_sw"))) return rc;
        } else if ((rc = lerr(launch_mpc_wide(X->k, X->s, iow, X->w, X->stream, lim), "mpc_wide"))) {
          return rc;
        }
      } else if (split_cell || quad) {  // iterEKF, then EKFmatsHandler + iterMPC from zk and Xind in HBM
        io.xm_out = X->d_xm;
        io.xg_out = X->d_xg;
        if (quad) {
          if ((rc = lerr(launch_ekf4(X->r, X->k, X->s, io, X->stream, X->ekf4_block), "ekf4"))) return rc;
        } else if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream, P_EKF), "cell"))) {
          return rc;
        }
        KIO io2 = io;
        io2.zk = nullptr;
        io2.zbk = nullptr;
        io2.bnd = nullptr;
        io2.xm_out = nullptr;
        io2.xg_out = nullptr;
        io2.zk_in = io.zk;
        io2.plant = 0;
        io2.tc_in = nullptr;
        io2.xm_in = X->d_xm;
        io2.xg_in = X->d_xg;
        if ((rc = lerr(launch_cell(X->r, X->k, X->s, io2, X->stream, P_MPC), "cell"))) return rc;
      } else if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream), "cell"))) {
        return rc;
      }
      if (E) HIPCHK(hipEventRecord(E[2], X->stream));
      const bool slice = roll && t < nsteps;
      if (slice) {
        const int j = t % P;
        const int64_t lo = n * j / P, hi = n * (j + 1) / P;
        hipStream_t fs = X->stream;
        if (fork) {
          HIPCHK(hipEventRecord(X->ev_fork, X->stream));
          HIPCHK(hipStreamWaitEvent(X->fstream, X->ev_fork, 0));
          fs = X->fstream;
        }
        if (E) HIPCHK(hipEventRecord(E[5], fs));
        if ((rc = lerr(launch_flush(X->r, X->k, X->s, t, t, fs, lo, hi), "flush"))) return rc;
        if (E) HIPCHK(hipEventRecord(E[6], fs));
        if (fork) HIPCHK(hipEventRecord(X->ev_join, fs));
        flushed[k] = hi > lo;
      }
      // MB: k_cell writes boundzk itself (one 6x6 covariance per cell)
      if (bnd_step) {
        hipStream_t bs = X->stream;
        if (side) {
          HIPCHK(hipEventRecord(X->ev_bfork, X->stream));
          HIPCHK(hipStreamWaitEvent(X->fstream, X->ev_bfork, 0));
          bs = X->fstream;
        }
        if ((rc = lerr(launch_bounds(X->r, X->s, X->d_bnd, zbk_k, bs), "bounds"))) return rc;
        if (E && side) HIPCHK(hipEventRecord(E[3], bs));
        if (side) HIPCHK(hipEventRecord(X->ev_bjoin, bs));
        bounded[k] = 1;
      }
      if (E) HIPCHK(hipEventRecord(E[hstart], X->stream));
      if (X->wide) {
        if ((rc = lerr(launch_hild_wide(X->k, X->s, iow, X->w, X->stream), "hild_wide"))) return rc;
      } else if (switched && X->sw == 7) {  // per-cell, every switch on: k_mpc_pc<7> left k_cell's hand-off
        if ((rc = lerr(launch_hild(X->k, X->s, iow, X->stream), "hild"))) return rc;
      } else if (switched) {
        if ((rc = lerr(launch_hild_sw(X->sw, X->k, X->s, iow, X->stream), "hild_sw"))) return rc;
      } else if ((rc = lerr(launch_hild(X->k, X->s, io, X->stream), "hild"))) {
        return rc;
      }
      if (diag) {
        double *pk = (double *)row(F_POLES, k), *sk = (double *)row(F_SV, k);
        rc = X->wide ? launch_cl_diag_wide(X->k, X->n, X->d_lin, X->d_uk1p, pk, sk, X->stream, lim)
                     : launch_cl_diag(X->k, X->n, X->d_lin, X->d_uk1p, pk, sk, X->stream, lim);
        if ((rc = lerr(rc, "cl_diag"))) return rc;
      }
      if (E) HIPCHK(hipEventRecord(E[4], X->stream));
      if (term) {  // the termination rule on every cell's own command, before the strings' reduction
        KTerm q{};
        q.uk = X->s.uk;
        q.uk_1 = X->s.uk_1;
        q.u = (double *)row(F_U, k);
        q.soc = io.soc;
        q.Tc = X->s.Tc;
        q.par = X->d_tm_par;
        q.rec = X->d_tm;
        q.cnt = X->tm_cnt();
        q.flag_in = term_str ? X->tm_flag(k & 1) : nullptr;
        q.flag_out = term_str ? X->tm_flag((k + 1) & 1) : nullptr;
        q.open = X->tm_open();
        q.n = X->n;
        q.series = pack ? X->pk_series : 1;
        q.hold = X->tm_hold;
        if ((rc = lerr(launch_term(q, X->stream), "term"))) return rc;
      }
      if (pack) {  // the strings' currents, once every cell's command stands in s.uk
        KPack q{};
        q.uk = X->s.uk;
        q.uk_1 = X->s.uk_1;
        q.u = (double *)row(F_U, k);
        q.ucmd = (double *)row(F_UCMD, k);
        q.limiter = (int *)row(F_LIMITER, k);
        q.rec = X->d_pk;
        q.n = X->n;
        q.series = X->pk_series;
        KPackBal b{};
        b.p = q;
        if (balance) {
          b.soc = io.soc;
          b.par = X->d_bl_par;
          b.on = X->d_bl_on;
          b.rec = X->d_bl;
          b.bleed = (double *)row(F_BLEED, k);
          b.zmin = (double *)row(F_ZMIN, k);
          b.compensate = X->bl_comp;
        }
        if (charger) {  // the strings' voltages and caps, the bleeders' switching and the currents in one launch
          KCharger h{};
          h.b = b;
          h.vk = X->s.vk;
          h.par = X->d_ch_par;
          h.rec = X->d_ch;
          h.vstr = (double *)row(F_VSTR, k);
          h.istr = (double *)row(F_ISTR, k);
          h.capby = (int *)row(F_CAPBY, k);
          if ((rc = lerr(launch_charger(h, X->stream), "charger"))) return rc;
        } else if (balance) {  // the bleeders' switching and the strings' currents in one launch
          if ((rc = lerr(launch_pack_bal(b, X->stream), "pack_bal"))) return rc;
        } else if ((rc = lerr(launch_pack(q, X->stream), "pack"))) {
          return rc;
        }
      }
      // k_bounds done before k_flush or the next step's k_cell rewrites the records it reads
      if (side && bnd_step) HIPCHK(hipStreamWaitEvent(X->stream, X->ev_bjoin, 0));
      if (slice && fork) HIPCHK(hipStreamWaitEvent(X->stream, X->ev_join, 0));
      if (roll ? t == nsteps : (t % P == 0 || t == nsteps)) {
        const bool timed = E && !roll;  // the rolling schedule times its slices only
        if (timed) HIPCHK(hipEventRecord(E[5], X->stream));
        if ((rc = lerr(launch_flush(X->r, X->k, X->s, t, t == nsteps ? 0 : t, X->stream), "flush"))) return rc;
        if (timed) HIPCHK(hipEventRecord(E[6], X->stream));
        flushed[k] = timed;
      }
      if (sum && ((size_t)t % ring == 0 || t == nsteps)) {  // the window is full, or the call ends
        KSum q{};
        q.rec = X->d_sum;
        q.reach = X->d_sum_reach;
        q.u = (const double *)f[F_U].dev;
        q.v = (const double *)f[F_V].dev;
        q.soc = (const double *)f[F_SOC].dev;
        q.phise = (const double *)f[F_PHISE].dev;
        q.nexec = (const int *)f[F_NEXEC].dev;
        q.obs = (const double *)f[F_OBS].dev;
        q.n = X->n;
        q.nrows = (int)((size_t)k % ring) + 1;
        q.max_hild = X->cfg.max_hild;
        if ((rc = lerr(launch_summary(q, X->stream), "summary"))) return rc;
      }
      if (aging) {  // before k_thermal: s.Tc is still the temperature the step used
        KAging q{};
        q.Tc = X->s.Tc;
        q.phi[AG_SRC_EST] = ag_est ? io.phise : nullptr;
        q.phi[AG_SRC_PLANT] = !ag_plant ? nullptr : ag_pos < 0 ? X->d_ag_obs : (const double *)row(F_OBS, k) + (size_t)ag_pos * n;
        q.par = X->d_ag_par;
        q.rec = X->d_ag;
        q.rate = (double *)row(F_RATE, k);
        q.n = X->n;
        q.nreact = X->ag_nreact;
        q.F = X->r.F;
        q.R = X->r.R;
        q.Tref = X->r.Tref;
        if ((rc = lerr(launch_aging(q, X->stream), "aging"))) return rc;
      }
      if (thermal) {  // last: after Hildreth stored the next command and the flush
        KTherm q{};
        q.Tc = X->s.Tc;
        q.vk = X->s.vk;
        q.SOCn = X->s.SOCn;
        q.status = X->s.status;
        q.uk = X->s.uk;
        q.iapp = X->d_th_i;
        q.par = X->d_th_par;
        q.ocv = X->d_th_ocv;
        q.rec = X->d_th;
        q.temp = (double *)row(F_TEMP, k);
        q.heat = (double *)row(F_HEAT, k);
        q.n = X->n;
        q.nocv = X->th_nocv;
        q.th0n = X->r.th0n;
        q.th100n = X->r.th100n;
        q.Ts = X->r.Ts;
        // a schedule: the next step's limits at the temperature this launch leaves; links: the
        // neighbours from the snapshot of the call-relative parity
        if (coupled) {
          KCouple h{};
          h.rlink = X->d_tc_link;
          h.rec = X->d_tc;
          h.snap_in = X->d_tc_snap + (size_t)(k & 1) * n;
          h.snap_out = X->d_tc_snap + (size_t)((k + 1) & 1) * n;
          h.cond = (double *)row(F_COND, k);
          h.series = X->pk_series;
          rc = sched && k + 1 < nsteps ? lerr(launch_thermal_couple_sched(q, h, ksch, X->stream), "thermal_couple_sched")
                                       : lerr(launch_thermal_couple(q, h, X->stream), "thermal_couple");
          if (rc) return rc;
          // a map: Z_LAST, and the next step's limits at the temperature the launch above left
          if (lmap && (rc = lerr(launch_map_step(kmap_of(k + 1, io.soc, k + 1 < nsteps), X->stream), "map_step")))
            return rc;
        } else if (lmap) {  // the model's step, Z_LAST, and the next step's limits in one launch
          if ((rc = lerr(launch_thermal_map(q, kmap_of(k + 1, io.soc, k + 1 < nsteps), X->stream), "thermal_map")))
            return rc;
        } else if (sched && k + 1 < nsteps) {
          if ((rc = lerr(launch_thermal_sched(q, ksch, X->stream), "thermal_sched"))) return rc;
        } else if ((rc = lerr(launch_thermal(q, X->stream), "thermal"))) {
          return rc;
        }
      } else if (lmap) {  // no model: Z_LAST and the next step's limits, the step's last launch
        if ((rc = lerr(launch_map_step(kmap_of(k + 1, io.soc, k + 1 < nsteps), X->stream), "map_step"))) return rc;
      }
    }
    return MPCEKF_OK;
  };
  if (capturing) {
    // a repeated call shape replays one instantiated graph instead of 5-7 launches per step.
    // An extension's rows (ucmd, rate, cond, ...) are among call.rows; its part holds the
    // context's own buffers and switches that the launches name
    using W = GraphParts::W;
    GraphKey key;
    GraphParts &p = key.p;
    p.call.nsteps = (W)nsteps;
    p.call.dtc = (W)dtc;
    p.call.diag = (W)diag;
    p.call.bounds = (W)bounds;
    for (int i = 0; i < NF; ++i) p.call.rows[i] = (W)f[i].dev;
    p.call.obs_plan = (W)osel.plan;
    p.call.nslots = (W)nslots;
    p.call.lim = (W)lim;
    p.call.hot = (W)X->s.hot_rec;
    p.call.hotp = (W)X->s.hotp_x;
    key.slots.assign(slots, slots + nslots);
    p.pack = {(W)X->d_pk, (W)X->pk_series};
    p.aging = {(W)X->d_ag, (W)(X->ag_nreact | X->ag_sources << 8), (W)(aging ? X->d_ag_phi : nullptr),
               (W)(aging ? X->d_ag_obs : nullptr)};
    p.couple = {(W)X->d_tc, (W)X->d_tc_link, (W)X->d_tc_snap};
    p.term = {(W)X->d_tm, (W)X->tm_hold, (W)(term ? X->d_tm_soc : nullptr)};
    if (balance) p.balance = {(W)X->d_bl, (W)X->d_bl_par, (W)X->d_bl_on, (W)X->bl_comp, (W)X->d_bl_soc};
    if (charger) p.charger = {(W)X->d_ch, (W)X->d_ch_par};
    if (sched) p.sched = {(W)X->d_sch_hdr, (W)X->d_sch_tab};  // the schedule's launches are part of the graph
    // and so are the map's; the launches hold the lim rows' stride, nf blocks of ncells per step
    if (lmap) p.map = {(W)X->d_lm, (W)X->d_lm_tab, (W)X->d_lm_soc, (W)X->h_lm.nf};
    p.thermal = {(W)X->d_th_ocv, (W)X->th_nocv, (W)X->d_th};
    if (sum) p.summary = {(W)X->d_sum_reach, (W)X->d_sum};  // the fold's launches are part of the graph
    if ((rc = X->graph_launch(key, run_steps))) return rc;
  } else if ((rc = run_steps())) {
    return rc;
  }
  if (!outputs_on_device)
    for (int i = 0; i < NF; ++i)
      if (f[i].host)
        HIPCHK(hipMemcpyAsync(f[i].host, f[i].dev, (size_t)nsteps * step_bytes(f[i]), hipMemcpyDeviceToHost, X->stream));
  // mpcekf_get_zk returns the last step's zk / boundzk whichever buffers the steps wrote
  if (nsteps > 0 && f[F_ZK].dev)
    HIPCHK(hipMemcpyAsync(X->d_zk, row(F_ZK, nsteps - 1), n * nzz * 8, hipMemcpyDeviceToDevice, X->stream));
  if (nsteps > 0 && f[F_ZBK].dev)
    HIPCHK(hipMemcpyAsync(X->d_zbk, row(F_ZBK, nsteps - 1), n * nzz * 8, hipMemcpyDeviceToDevice, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  if (X->timing) {
    // (start, end) events of plant, cell, bounds, hild, flush
    static const int slot[5] = {MPCEKF_K_PLANT, MPCEKF_K_CELL, MPCEKF_K_BOUNDS, MPCEKF_K_HILD, MPCEKF_K_FLUSH};
    static const int e0[5] = {0, 1, 2, 3, 5};
    for (int k = 0; k < nsteps; ++k)
      for (int j = 0; j < 5; ++j) {
        if ((k + 1) % X->timing_every != 0 && k != nsteps - 1) continue;
        if ((j == 4 && !flushed[k]) || (j == 2 && !bounded[k]) || (j == 0 && plant_in_cell && !nslots)) continue;
        float ms = 0;
        const int a = j == 3 ? hstart : e0[j], b = j == 3 ? 4 : e0[j] + 1;
        HIPCHK(hipEventElapsedTime(&ms, X->ev[(size_t)k * NEV + a], X->ev[(size_t)k * NEV + b]));
        X->t_ms[slot[j]] += ms;
        X->t_n[slot[j]] += 1;
      }
  }
  return MPCEKF_OK;
}

int mpcekf_step_ex(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                   int32_t outputs_on_device) {
  return step_impl(X, nsteps, tc_degC, tr, nullptr, 0, nullptr, outputs_on_device);
}

int mpcekf_step_ex_obs(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                       const int32_t *slots, int32_t nslots, double *obs, int32_t outputs_on_device) {
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device);
}

int mpcekf_cl_eig(int32_t n, const double *a, double *re, double *im, double *sv) {
  if (n < 1 || n > mk::eig::MAXN || !a) return fail(MPCEKF_E_ARG, "cl_eig: n must be 1..%d", mk::eig::MAXN);
  double r[mk::eig::MAXN], m[mk::eig::MAXN], s[mk::eig::MAXN];
  if (re || im) mk::eig::eigvals(n, a, r, m);
  if (sv) mk::eig::singvals(n, a, s);
  for (int i = 0; i < n; ++i) {
    if (re) re[i] = r[i];
    if (im) im[i] = m[i];
    if (sv) sv[i] = s[i];
  }
  return MPCEKF_OK;
}

int mpcekf_step(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, double *traj_u, double *traj_v,
                double *traj_soc, double *traj_phise, int32_t *traj_nexec, int32_t outputs_on_device) {
  mpcekf_traj tr{};
  tr.u = traj_u;
  tr.v = traj_v;
  tr.soc = traj_soc;
  tr.phise = traj_phise;
  tr.nexec = traj_nexec;
  return mpcekf_step_ex(X, nsteps, tc_degC, &tr, outputs_on_device);
}

int mpcekf_set_graph(mpcekf_ctx *X, int32_t enable) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  X->graph = enable != 0;
  return MPCEKF_OK;
}

// ---- per-cell limits (runMPC.m:30-44 / initMPC.m:66-67 / constraintsMPC.m:90-91 per cell) ----
static double cfg_limit(const mpcekf_config &c, int f) {
  switch (f) {
    case MPCEKF_LIM_TARGET_SOC: return c.target_soc;
    case MPCEKF_LIM_CRATE: return c.Crate;
    case MPCEKF_LIM_U_MAX: return c.u_max;
    case MPCEKF_LIM_DU_MIN: return c.du_min;
    case MPCEKF_LIM_DU_MAX: return c.du_max;
    case MPCEKF_LIM_V_MAX: return c.v_max;
    case MPCEKF_LIM_PHISE_MIN: return c.phise_min;
    case MPCEKF_LIM_Z_MAX: return c.z_max;
    default: return c.z_tol;
  }
}

// nfields / fields of mpcekf_set_limits and mpcekf_get_limits
static int check_limit_fields(const char *who, int32_t nfields, const int32_t *fields) {
  if (nfields < 1 || nfields > MPCEKF_NLIM)
    return fail(MPCEKF_E_ARG, "%s: nfields = %d outside 1..%d", who, nfields, (int)MPCEKF_NLIM);
  if (!fields) return fail(MPCEKF_E_ARG, "%s: null fields", who);
  unsigned seen = 0;
  for (int i = 0; i < nfields; ++i) {
    if (fields[i] < 0 || fields[i] >= MPCEKF_NLIM)
      return fail(MPCEKF_E_ARG, "%s: fields[%d] = %d is not a MPCEKF_LIM_* id (0..%d)", who, i, fields[i],
                  (int)MPCEKF_NLIM - 1);
    if (seen >> fields[i] & 1) return fail(MPCEKF_E_ARG, "%s: fields: id %d given twice", who, fields[i]);
    seen |= 1u << fields[i];
  }
  return MPCEKF_OK;
}

// The limits record's buffers and the host copy of the values (the configuration's scalars until
// a set names a field): what the first mpcekf_set_limits or mpcekf_thermal_schedule needs.
static int limits_bufs(mpcekf_ctx *X) {
  int rc;
  const size_t n = (size_t)X->n;
  if (!X->d_lim && (rc = dalloc(&X->d_lim, std::max<size_t>(n, 1) * NLIMK))) return rc;
  // the split route's hand-off k_cell<P_EKF | P_LIN> -> k_mpc_pc (a switched or wide context has it)
  if (!X->d_lin && (rc = dalloc(&X->d_lin, std::max<size_t>(n, 1) * MPCEKF_LIN_SIZE))) return rc;
  if (!X->d_zsoc && (rc = dalloc(&X->d_zsoc, std::max<size_t>(n, 1)))) return rc;
  if (X->h_lim.empty()) {
    X->h_lim.resize((size_t)MPCEKF_NLIM * n);
    for (int f = 0; f < MPCEKF_NLIM; ++f) std::fill_n(X->h_lim.begin() + (size_t)f * n, n, cfg_limit(X->cfg, f));
  }
  return MPCEKF_OK;
}

// h_lim -> the kernels' record by fill_kcfg's expressions (an array constant at the
// configuration's value gives the scalar's bits), then, with a schedule, its fields at every
// cell's temperature as it stands.  Waits for the stream.
static int limits_upload(mpcekf_ctx *X) {
  int rc;
  const size_t n = (size_t)X->n;
  std::vector<double> rec((size_t)NLIMK * n);
  const double *h = X->h_lim.data();
  const double Q = X->r.Q;
  for (size_t c = 0; c < n; ++c) {
    rec[LK_REF * n + c] = h[MPCEKF_LIM_TARGET_SOC * n + c];
    rec[LK_U_MAX * n + c] = h[MPCEKF_LIM_U_MAX * n + c];
    rec[LK_U_MIN * n + c] = -Q * h[MPCEKF_LIM_CRATE * n + c];  // initMPC.m:66-67
    rec[LK_DU_MIN * n + c] = h[MPCEKF_LIM_DU_MIN * n + c];
    rec[LK_DU_MAX * n + c] = h[MPCEKF_LIM_DU_MAX * n + c];
    rec[LK_V_MAX * n + c] = h[MPCEKF_LIM_V_MAX * n + c];
    rec[LK_PHISE_MIN * n + c] = h[MPCEKF_LIM_PHISE_MIN * n + c];
    rec[LK_ZMAX * n + c] = h[MPCEKF_LIM_Z_MAX * n + c] + h[MPCEKF_LIM_Z_TOL * n + c];  // constraintsMPC.m:90-91
  }
  // on the context's stream, after every launch already queued; the wait makes rec's lifetime safe
  if (n) HIPCHK(hipMemcpyAsync(X->d_lim, rec.data(), rec.size() * 8, hipMemcpyHostToDevice, X->stream));
  if (X->sched && (rc = lerr(launch_sched(X->ksched(), X->stream), "sched"))) return rc;
  // a map likewise, at Z_LAST and the temperature as they stand; not an evaluation of a fused step
  if (X->lmap && (rc = lerr(launch_map(X->kmap(), X->stream), "map"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_set_limits(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, const double *values) {
  if (!X) return fail(MPCEKF_E_ARG, "set_limits: null ctx");
  int rc = check_limit_fields("set_limits", nfields, fields);
  if (rc) return rc;
  if (!values) return fail(MPCEKF_E_ARG, "set_limits: null values");
  for (int i = 0; i < nfields; ++i)
    if (X->sched_row(fields[i]) >= 0)
      return fail(MPCEKF_E_ARG, "set_limits: fields[%d] = %d is scheduled over temperature (mpcekf_thermal_schedule)", i,
                  fields[i]);
  for (int i = 0; i < nfields; ++i)
    if (X->map_row(fields[i]) >= 0)
      return fail(MPCEKF_E_ARG, "set_limits: fields[%d] = %d is mapped over SOC and temperature (mpcekf_limit_map)", i,
                  fields[i]);
  // check_cfg puts no condition on the scalar form of any of these fields, so none is put on
  // an element either (a negative du_max is a legitimate configuration)
  HIPCHK(hipSetDevice(X->device));
  const size_t n = (size_t)X->n;
  if ((rc = limits_bufs(X))) return rc;
  for (int i = 0; i < nfields; ++i) std::copy_n(values + (size_t)i * n, n, X->h_lim.begin() + (size_t)fields[i] * n);
  if ((rc = limits_upload(X))) return rc;
  X->percell = X->lim_set = true;
  return MPCEKF_OK;
}

int mpcekf_get_limits(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  if (!X) return fail(MPCEKF_E_ARG, "get_limits: null ctx");
  int rc = check_limit_fields("get_limits", nfields, fields);
  if (rc) return rc;
  if (!values) return fail(MPCEKF_E_ARG, "get_limits: null values");
  const size_t n = (size_t)X->n;
  bool wait = false;
  for (int i = 0; i < nfields; ++i) {
    const int row = X->sched_row(fields[i]), mrow = X->map_row(fields[i]);
    if (row >= 0 || mrow >= 0) {  // a scheduled or mapped field: the value of the last evaluation, kept on the device
      const double *src = row >= 0 ? X->d_sch_val + (size_t)row * n : X->d_lm_val + (size_t)mrow * n;
      if (!wait) HIPCHK(hipSetDevice(X->device));
      if (n) HIPCHK(hipMemcpyAsync(values + (size_t)i * n, src, n * 8, hipMemcpyDeviceToHost, X->stream));
      wait = true;
    } else if (X->percell) {
      std::copy_n(X->h_lim.begin() + (size_t)fields[i] * n, n, values + (size_t)i * n);
    } else {
      std::fill_n(values + (size_t)i * n, n, cfg_limit(X->cfg, fields[i]));
    }
  }
  if (wait) HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_clear_limits(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "clear_limits: null ctx");
  if (X->sched)
    return fail(MPCEKF_E_STATE, "clear_limits: a temperature schedule is active (mpcekf_thermal_schedule_end first)");
  if (X->lmap) return fail(MPCEKF_E_STATE, "clear_limits: a limit map is active (mpcekf_limit_map_end first)");
  X->percell = X->lim_set = false;  // the buffers stay: a graph captured per-cell names d_lim until the context goes
  X->h_lim.clear();
  return MPCEKF_OK;
}

// ---- the record getters (mpcekf_get_summary and every extension's _get) ----
// Their arguments, in the order every getter refuses them, before any HIP call: the context,
// nfields in 1..nrows, fields, values, every id in 0..nrows-1 (the MPCEKF_<ids>_* of the header)
// and given once.  who: the getter's short name.  The getter's own state check follows.
static int check_rows(const mpcekf_ctx *X, const char *who, const char *ids, int nrows, int32_t nfields,
                      const int32_t *fields, const double *values) {
  if (!X) return fail(MPCEKF_E_ARG, "%s: null ctx", who);
  if (nfields < 1 || nfields > nrows) return fail(MPCEKF_E_ARG, "%s: nfields = %d outside 1..%d", who, nfields, nrows);
  if (!fields) return fail(MPCEKF_E_ARG, "%s: null fields", who);
  if (!values) return fail(MPCEKF_E_ARG, "%s: null values", who);
  unsigned seen = 0;
  for (int i = 0; i < nfields; ++i) {
    if (fields[i] < 0 || fields[i] >= nrows)
      return fail(MPCEKF_E_ARG, "%s: fields[%d] = %d is not a MPCEKF_%s_* id (0..%d)", who, i, fields[i], ids, nrows - 1);
    if (seen >> fields[i] & 1) return fail(MPCEKF_E_ARG, "%s: fields: id %d given twice", who, fields[i]);
    seen |= 1u << fields[i];
  }
  return MPCEKF_OK;
}

// values [nfields][len] = rows fields[i] of the slot-major record at rec, each of len doubles; row
// `alt_id`, if any, lives at `alt` instead.  Waits for the copies.
static int get_rows(mpcekf_ctx *X, const double *rec, size_t len, int32_t nfields, const int32_t *fields, double *values,
                    int alt_id = -1, const double *alt = nullptr) {
  HIPCHK(hipSetDevice(X->device));
  for (int i = 0; i < nfields && len; ++i) {
    const double *src = fields[i] == alt_id ? alt : rec + (size_t)fields[i] * len;
    HIPCHK(hipMemcpyAsync(values + (size_t)i * len, src, len * 8, hipMemcpyDeviceToHost, X->stream));
  }
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

// ---- per-cell charge summary along the fused loop (mpcekf_summary.hip) ----
static_assert(NSUM == MPCEKF_NSUM && SUM_WIN == MPCEKF_SUM_WIN && SUM_SEEN == MPCEKF_SUM_SEEN &&
                  SUM_T_REACH == MPCEKF_SUM_T_REACH && SUM_U_MAX == MPCEKF_SUM_U_MAX && SUM_V_MIN == MPCEKF_SUM_V_MIN &&
                  SUM_PHISE_MIN_STEP == MPCEKF_SUM_PHISE_MIN_STEP && SUM_PHISE_LAST == MPCEKF_SUM_PHISE_LAST &&
                  SUM_U_SUM == MPCEKF_SUM_U_SUM && SUM_NSAT == MPCEKF_SUM_NSAT && SUM_OBS_MIN == MPCEKF_SUM_OBS_MIN &&
                  SUM_OBS_MAX_STEP == MPCEKF_SUM_OBS_MAX_STEP,
              "mpcekf_summary.hpp's rows are include/mpcekf.h's MPCEKF_SUM_*");

int mpcekf_summary_begin(mpcekf_ctx *X, const double *soc_reach, int32_t obs_slot) {
  if (!X) return fail(MPCEKF_E_ARG, "summary_begin: null ctx");
  if (obs_slot < -1 || obs_slot >= X->ko.nobs)
    return fail(MPCEKF_E_ARG, "summary_begin: obs_slot %d outside -1..%d", obs_slot, X->ko.nobs - 1);
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>((size_t)X->n, 1);
  int rc;
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_sum, *reach = X->d_sum_reach, *ob = X->d_sum_obs;
  char *ringp = X->d_sum_ring;
  if (!rec && (rc = dalloc(&rec, n * NSUM))) return rc;
  if (!reach && (rc = dalloc(&reach, n))) return rc;
  if (!ringp && (rc = dalloc(&ringp, 5 * X->sum_row() + 256))) return rc;
  if (obs_slot >= 0 && !ob && (rc = dalloc(&ob, (size_t)SUM_WIN * n))) return rc;
  X->d_sum = rec;
  X->d_sum_reach = reach;
  X->d_sum_ring = ringp;
  X->d_sum_obs = ob;
  X->sum_slot = obs_slot;
  if (soc_reach && X->n)
    HIPCHK(hipMemcpyAsync(reach, soc_reach, (size_t)X->n * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_summary_reset(rec, reach, !soc_reach, X->n, X->stream), "summary_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_step_summary(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC) {
  if (!X) return fail(MPCEKF_E_ARG, "step_summary: null ctx");
  if (!X->d_sum) return fail(MPCEKF_E_STATE, "step_summary: call mpcekf_summary_begin first");
  StepOut o;
  o.sum = true;
  return step_impl(X, nsteps, tc_degC, nullptr, nullptr, 0, nullptr, 0, o);
}

int mpcekf_get_summary(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "get_summary", "SUM", MPCEKF_NSUM, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_sum) return fail(MPCEKF_E_STATE, "get_summary: call mpcekf_summary_begin first");
  return get_rows(X, X->d_sum, (size_t)X->n, nfields, fields, values);
}

int mpcekf_summary_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "summary_end: null ctx");
  if (!X->d_sum) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured from summary calls name the buffers freed below
  X->retire_graphs([](const GraphParts &k) { return k.summary.rec != 0; });
  void *ptrs[] = {X->d_sum, X->d_sum_reach, X->d_sum_obs, X->d_sum_ring};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  X->d_sum = X->d_sum_reach = X->d_sum_obs = nullptr;
  X->d_sum_ring = nullptr;
  X->sum_slot = -1;
  return MPCEKF_OK;
}

// ---- per-cell lumped thermal model along the fused loop (mpcekf_thermal.hip) ----
static_assert(NTH == MPCEKF_NTH && TH_CTH == MPCEKF_TH_CTH && TH_RTH == MPCEKF_TH_RTH && TH_TAMB == MPCEKF_TH_TAMB &&
                  NTHR == MPCEKF_NTHR && THR_T == MPCEKF_THR_T && THR_T_MAX == MPCEKF_THR_T_MAX &&
                  THR_T_MAX_STEP == MPCEKF_THR_T_MAX_STEP && THR_T_MIN == MPCEKF_THR_T_MIN &&
                  THR_HEAT_SUM == MPCEKF_THR_HEAT_SUM && THR_STEPS == MPCEKF_THR_STEPS &&
                  THR_NHELD == MPCEKF_THR_NHELD,
              "mpcekf_thermal.hpp's rows are include/mpcekf.h's MPCEKF_TH_* / MPCEKF_THR_*");

// the graphs captured on a thermal context launch k_thermal on the model's buffers: retired
// before any of those buffers is freed
static void retire_thermal_graphs(mpcekf_ctx *X) {
  X->retire_graphs([](const GraphParts &k) { return k.thermal.rec != 0; });
}

int mpcekf_thermal_begin(mpcekf_ctx *X, const double *params, int32_t nocv, const double *ocv, const double *t0_degC) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_begin: null ctx");
  if (!params) return fail(MPCEKF_E_ARG, "thermal_begin: null params");
  if (!ocv) return fail(MPCEKF_E_ARG, "thermal_begin: null ocv");
  if (nocv < 2) return fail(MPCEKF_E_ARG, "thermal_begin: nocv = %d: the table needs 2 entries or more", nocv);
  for (int i = 0; i < nocv; ++i)
    if (!std::isfinite(ocv[i])) return fail(MPCEKF_E_ARG, "thermal_begin: ocv[%d] = %g is not finite", i, ocv[i]);
  const size_t nc = (size_t)X->n;
  for (size_t c = 0; c < nc; ++c) {
    const double Cth = params[MPCEKF_TH_CTH * nc + c], Rth = params[MPCEKF_TH_RTH * nc + c];
    if (!std::isfinite(Cth) || !(Cth > 0))
      return fail(MPCEKF_E_ARG, "thermal_begin: Cth[%zu] = %g: must be finite and > 0 (J/K)", c, Cth);
    if (!(Rth > 0)) return fail(MPCEKF_E_ARG, "thermal_begin: Rth[%zu] = %g: must be > 0 (K/W; +inf: adiabatic)", c, Rth);
  }
  // check_tc's rule, with the argument named
  for (size_t c = 0; c < nc; ++c) {
    const double Tamb = params[MPCEKF_TH_TAMB * nc + c];
    if (!(Tamb <= 100) || !std::isfinite(Tamb))
      return fail(MPCEKF_E_ARG, "thermal_begin: Tamb[%zu] = %g: must be finite and in degC (iterEKF.m:62)", c, Tamb);
    if (t0_degC && (!(t0_degC[c] <= 100) || !std::isfinite(t0_degC[c])))
      return fail(MPCEKF_E_ARG, "thermal_begin: t0[%zu] = %g: must be finite and in degC (iterEKF.m:62)", c, t0_degC[c]);
  }
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_th, *par = X->d_th_par, *ia = X->d_th_i, *tab = X->d_th_ocv;
  const bool new_tab = !tab || X->th_nocv != nocv;
  if (!rec && (rc = dalloc(&rec, n * NTHR))) return rc;
  if (!par && (rc = dalloc(&par, n * NTH))) return rc;
  if (!ia && (rc = dalloc(&ia, n))) return rc;
  if (new_tab) {
    double *t = nullptr;
    if ((rc = dalloc(&t, (size_t)nocv))) return rc;
    if (tab) {  // no launch in flight reads the old table, and no graph names it any more
      HIPCHK(hipStreamSynchronize(X->stream));
      retire_thermal_graphs(X);
      (void)hipFree(tab);
    }
    tab = t;
  }
  X->d_th = rec;
  X->d_th_par = par;
  X->d_th_i = ia;
  X->d_th_ocv = tab;
  X->th_nocv = nocv;
  if (nc) HIPCHK(hipMemcpyAsync(par, params, nc * NTH * 8, hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipMemcpyAsync(tab, ocv, (size_t)nocv * 8, hipMemcpyHostToDevice, X->stream));
  if (nc && t0_degC) HIPCHK(hipMemcpyAsync(X->s.Tc, t0_degC, nc * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_thermal_reset(rec, X->n, X->stream), "thermal_reset"))) return rc;
  // a second begin keeps the links; the coupling's step indices are the model's, so its record restarts too
  if (X->d_tc && (rc = lerr(launch_couple_reset(X->d_tc, X->n, X->stream), "couple_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_thermal_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "thermal_get", "THR", MPCEKF_NTHR, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_th) return fail(MPCEKF_E_STATE, "thermal_get: call mpcekf_thermal_begin first");
  return get_rows(X, X->d_th, (size_t)X->n, nfields, fields, values, MPCEKF_THR_T, X->s.Tc);  // the temperature is the state's
}

int mpcekf_thermal_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_end: null ctx");
  if (!X->d_th) return MPCEKF_OK;
  int rc = mpcekf_thermal_schedule_end(X);  // the scheduled fields back to set_limits' / the configuration's values
  if (rc) return rc;
  if (X->lmap && X->h_lm.nt > 1 && (rc = mpcekf_limit_map_end(X))) return rc;  // a temperature axis needs a model
  if ((rc = mpcekf_thermal_couple_end(X))) return rc;  // links need a model
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  retire_thermal_graphs(X);
  void *ptrs[] = {X->d_th, X->d_th_par, X->d_th_i, X->d_th_ocv};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  X->d_th = X->d_th_par = X->d_th_i = X->d_th_ocv = nullptr;
  X->th_nocv = 0;
  return MPCEKF_OK;
}

// ---- the MPC limits scheduled over the model's temperature (mpcekf_thermal_sched.hip) ----
int mpcekf_thermal_schedule(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, int32_t ntab, double T_lo_degC,
                            double T_hi_degC, int32_t nsets, const double *tables, const int32_t *set_of_cell) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_schedule: null ctx");
  if (nfields < 1 || nfields > SCHED_MAXF)
    return fail(MPCEKF_E_ARG, "thermal_schedule: nfields = %d outside 1..%d", nfields, (int)SCHED_MAXF);
  if (!fields) return fail(MPCEKF_E_ARG, "thermal_schedule: null fields");
  if (!tables) return fail(MPCEKF_E_ARG, "thermal_schedule: null tables");
  SchedHdr h{};
  unsigned seen = 0;
  for (int i = 0; i < nfields; ++i) {
    int slot;
    switch (fields[i]) {
      case MPCEKF_LIM_CRATE: slot = LK_U_MIN; break;
      case MPCEKF_LIM_U_MAX: slot = LK_U_MAX; break;
      case MPCEKF_LIM_DU_MIN: slot = LK_DU_MIN; break;
      case MPCEKF_LIM_DU_MAX: slot = LK_DU_MAX; break;
      case MPCEKF_LIM_V_MAX: slot = LK_V_MAX; break;
      case MPCEKF_LIM_PHISE_MIN: slot = LK_PHISE_MIN; break;
      default:
        return fail(MPCEKF_E_ARG, "thermal_schedule: fields[%d] = %d cannot be scheduled (CRATE, U_MAX, DU_MIN, DU_MAX, "
                    "V_MAX, PHISE_MIN can)", i, fields[i]);
    }
    if (seen >> fields[i] & 1) return fail(MPCEKF_E_ARG, "thermal_schedule: fields: id %d given twice", fields[i]);
    seen |= 1u << fields[i];
    h.slot[i] = slot;
    h.crate[i] = fields[i] == MPCEKF_LIM_CRATE;
  }
  if (ntab < 2) return fail(MPCEKF_E_ARG, "thermal_schedule: ntab = %d: a table needs 2 entries or more", ntab);
  if (!std::isfinite(T_lo_degC) || !std::isfinite(T_hi_degC) || !(T_hi_degC > T_lo_degC))
    return fail(MPCEKF_E_ARG, "thermal_schedule: grid [%g, %g] degC: finite ends with T_hi > T_lo", T_lo_degC, T_hi_degC);
  if (nsets < 1) return fail(MPCEKF_E_ARG, "thermal_schedule: nsets = %d: 1 or more", nsets);
  const size_t ntabs = (size_t)nsets * (size_t)nfields * (size_t)ntab;
  for (size_t i = 0; i < ntabs; ++i)
    if (!std::isfinite(tables[i]))
      return fail(MPCEKF_E_ARG, "thermal_schedule: tables[%zu] = %g is not finite (set %zu, field %zu, entry %zu)", i,
                  tables[i], i / ((size_t)nfields * ntab), i / ntab % nfields, i % ntab);
  const size_t nc = (size_t)X->n;
  for (size_t c = 0; set_of_cell && c < nc; ++c)
    if (set_of_cell[c] < 0 || set_of_cell[c] >= nsets)
      return fail(MPCEKF_E_ARG, "thermal_schedule: set_of_cell[%zu] = %d outside 0..%d", c, set_of_cell[c], nsets - 1);
  if (!X->d_th) return fail(MPCEKF_E_STATE, "thermal_schedule: call mpcekf_thermal_begin first");
  if (X->lmap) return fail(MPCEKF_E_STATE, "thermal_schedule: a limit map is active (mpcekf_limit_map_end first)");
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // every buffer before anything is stored: a failed allocation leaves the schedule as it was
  if (!X->d_sch_hdr && (rc = dalloc(&X->d_sch_hdr, 1))) return rc;
  if (!X->d_sch_set && (rc = dalloc(&X->d_sch_set, n))) return rc;
  if (!X->d_sch_val && (rc = dalloc(&X->d_sch_val, n * SCHED_MAXF))) return rc;
  if (X->sch_cap < ntabs) {
    double *t = nullptr;
    if ((rc = dalloc(&t, ntabs))) return rc;
    if (X->d_sch_tab) {  // no launch in flight reads the old tables, and no graph names them any more
      HIPCHK(hipStreamSynchronize(X->stream));
      retire_thermal_graphs(X);
      (void)hipFree(X->d_sch_tab);
    }
    X->d_sch_tab = t;
    X->sch_cap = ntabs;
  }
  if ((rc = limits_bufs(X))) return rc;
  h.T_lo = T_lo_degC;
  h.T_hi = T_hi_degC;
  h.Q = X->r.Q;
  h.nf = nfields;
  h.ntab = ntab;
  h.nsets = nsets;
  X->h_sch = h;
  std::copy_n(fields, nfields, X->h_sch_field);
  HIPCHK(hipMemcpyAsync(X->d_sch_hdr, &X->h_sch, sizeof(SchedHdr), hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipMemcpyAsync(X->d_sch_tab, tables, ntabs * 8, hipMemcpyHostToDevice, X->stream));
  if (nc && set_of_cell) HIPCHK(hipMemcpyAsync(X->d_sch_set, set_of_cell, nc * 4, hipMemcpyHostToDevice, X->stream));
  if (nc && !set_of_cell) HIPCHK(hipMemsetAsync(X->d_sch_set, 0, nc * 4, X->stream));
  // the record from the values set_limits or the configuration gave (a replaced schedule's fields
  // go back to them), then the new schedule's fields at the temperatures as they stand
  X->sched = true;
  X->percell = true;
  return limits_upload(X);
}

int mpcekf_thermal_schedule_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_schedule_end: null ctx");
  if (!X->sched) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  X->sched = false;  // the buffers stay: a graph captured with the schedule names them until thermal_end
  X->h_sch.nf = 0;
  if (X->lim_set) return limits_upload(X);  // the scheduled fields back to what set_limits gave them
  X->percell = false;
  X->h_lim.clear();
  return MPCEKF_OK;
}

// ---- the MPC limits mapped over the SOC estimate and the temperature (mpcekf_limit_map.hip) ----
static_assert(NLMR == MPCEKF_NLM && LM_Z_LAST == MPCEKF_LM_Z_LAST && LM_NEVAL == MPCEKF_LM_NEVAL &&
                  LM_NCLAMP_Z == MPCEKF_LM_NCLAMP_Z && LM_NCLAMP_T == MPCEKF_LM_NCLAMP_T,
              "mpcekf_limit_map.hpp's rows are include/mpcekf.h's MPCEKF_LM_*");

int mpcekf_limit_map(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, int32_t nz, double z_lo, double z_hi,
                     int32_t nt, double T_lo_degC, double T_hi_degC, int32_t interp_z, int32_t nsets,
                     const double *tables, const int32_t *set_of_cell, const double *z0) {
  if (!X) return fail(MPCEKF_E_ARG, "limit_map: null ctx");
  if (nfields < 1 || nfields > MAP_MAXF)
    return fail(MPCEKF_E_ARG, "limit_map: nfields = %d outside 1..%d", nfields, (int)MAP_MAXF);
  if (!fields) return fail(MPCEKF_E_ARG, "limit_map: null fields");
  if (!tables) return fail(MPCEKF_E_ARG, "limit_map: null tables");
  MapHdr h{};
  unsigned seen = 0;
  for (int i = 0; i < nfields; ++i) {
    int slot;
    switch (fields[i]) {
      case MPCEKF_LIM_CRATE: slot = LK_U_MIN; break;
      case MPCEKF_LIM_U_MAX: slot = LK_U_MAX; break;
      case MPCEKF_LIM_DU_MIN: slot = LK_DU_MIN; break;
      case MPCEKF_LIM_DU_MAX: slot = LK_DU_MAX; break;
      case MPCEKF_LIM_V_MAX: slot = LK_V_MAX; break;
      case MPCEKF_LIM_PHISE_MIN: slot = LK_PHISE_MIN; break;
      default:
        return fail(MPCEKF_E_ARG, "limit_map: fields[%d] = %d cannot be mapped (CRATE, U_MAX, DU_MIN, DU_MAX, V_MAX, "
                    "PHISE_MIN can)", i, fields[i]);
    }
    if (seen >> fields[i] & 1) return fail(MPCEKF_E_ARG, "limit_map: fields: id %d given twice", fields[i]);
    seen |= 1u << fields[i];
    h.slot[i] = slot;
    h.crate[i] = fields[i] == MPCEKF_LIM_CRATE;
  }
  if (nz < 1 || nt < 1 || (nz == 1 && nt == 1))
    return fail(MPCEKF_E_ARG, "limit_map: nz = %d, nt = %d: 1 or more each, and 2 or more on one axis", nz, nt);
  if (!std::isfinite(z_lo) || !std::isfinite(z_hi) || !(z_hi > z_lo))
    return fail(MPCEKF_E_ARG, "limit_map: SOC grid [%g, %g]: finite ends with z_hi > z_lo", z_lo, z_hi);
  if (nt > 1 && (!std::isfinite(T_lo_degC) || !std::isfinite(T_hi_degC) || !(T_hi_degC > T_lo_degC)))
    return fail(MPCEKF_E_ARG, "limit_map: temperature grid [%g, %g] degC: finite ends with T_hi > T_lo", T_lo_degC,
                T_hi_degC);
  if (interp_z != 0 && interp_z != 1)
    return fail(MPCEKF_E_ARG, "limit_map: interp_z = %d: 0 (linear) or 1 (hold)", interp_z);
  if (nsets < 1) return fail(MPCEKF_E_ARG, "limit_map: nsets = %d: 1 or more", nsets);
  const size_t plane = (size_t)nt * (size_t)nz, ntabs = (size_t)nsets * (size_t)nfields * plane;
  for (size_t i = 0; i < ntabs; ++i)
    if (!std::isfinite(tables[i]))
      return fail(MPCEKF_E_ARG, "limit_map: tables[%zu] = %g is not finite (set %zu, field %zu, T node %zu, SOC node %zu)",
                  i, tables[i], i / ((size_t)nfields * plane), i / plane % nfields, i / nz % nt, i % nz);
  const size_t nc = (size_t)X->n;
  for (size_t c = 0; set_of_cell && c < nc; ++c)
    if (set_of_cell[c] < 0 || set_of_cell[c] >= nsets)
      return fail(MPCEKF_E_ARG, "limit_map: set_of_cell[%zu] = %d outside 0..%d", c, set_of_cell[c], nsets - 1);
  for (size_t c = 0; z0 && c < nc; ++c)
    if (std::isinf(z0[c])) return fail(MPCEKF_E_ARG, "limit_map: z0[%zu] = %g: finite, or NaN for no estimate", c, z0[c]);
  if (X->sched)
    return fail(MPCEKF_E_STATE, "limit_map: a temperature schedule is active (mpcekf_thermal_schedule_end first)");
  if (nt > 1 && !X->d_th) return fail(MPCEKF_E_STATE, "limit_map: nt = %d: call mpcekf_thermal_begin first", nt);
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // every buffer before anything is stored: a failed allocation leaves the map as it was
  if (!X->d_lm_hdr && (rc = dalloc(&X->d_lm_hdr, 1))) return rc;
  if (!X->d_lm_set && (rc = dalloc(&X->d_lm_set, n))) return rc;
  if (!X->d_lm_val && (rc = dalloc(&X->d_lm_val, n * MAP_MAXF))) return rc;
  if (!X->d_lm_soc && (rc = dalloc(&X->d_lm_soc, n))) return rc;
  if (!X->d_lm && (rc = dalloc(&X->d_lm, n * NLMR))) return rc;
  if (X->lm_cap < ntabs) {
    double *t = nullptr;
    if ((rc = dalloc(&t, ntabs))) return rc;
    if (X->d_lm_tab) {  // no launch in flight reads the old tables, and no graph names them any more
      HIPCHK(hipStreamSynchronize(X->stream));
      X->retire_graphs([](const GraphParts &k) { return k.map.rec != 0; });
      (void)hipFree(X->d_lm_tab);
    }
    X->d_lm_tab = t;
    X->lm_cap = ntabs;
  }
  if ((rc = limits_bufs(X))) return rc;
  h.z_lo = z_lo;
  h.z_hi = z_hi;
  h.T_lo = nt > 1 ? T_lo_degC : 0.0;
  h.T_hi = nt > 1 ? T_hi_degC : 1.0;
  h.Q = X->r.Q;
  h.nz = nz;
  h.nt = nt;
  h.interp_z = interp_z;
  h.nf = nfields;
  h.nsets = nsets;
  X->h_lm = h;
  std::copy_n(fields, nfields, X->h_lm_field);
  HIPCHK(hipMemcpyAsync(X->d_lm_hdr, &X->h_lm, sizeof(MapHdr), hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipMemcpyAsync(X->d_lm_tab, tables, ntabs * 8, hipMemcpyHostToDevice, X->stream));
  if (nc && set_of_cell) HIPCHK(hipMemcpyAsync(X->d_lm_set, set_of_cell, nc * 4, hipMemcpyHostToDevice, X->stream));
  if (nc && !set_of_cell) HIPCHK(hipMemsetAsync(X->d_lm_set, 0, nc * 4, X->stream));
  // the record restarts; Z_LAST from z0, or NaN, or -- replacing an active map without a z0 -- kept
  if (nc && z0) HIPCHK(hipMemcpyAsync(X->d_lm + (size_t)LM_Z_LAST * nc, z0, nc * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_map_reset(X->d_lm, z0 || X->lmap, X->n, X->stream), "map_reset"))) return rc;
  // the limits record from the values set_limits or the configuration gave (a replaced map's fields
  // go back to them), then the new map's fields at Z_LAST and the temperatures as they stand
  X->lmap = true;
  X->percell = true;
  return limits_upload(X);
}

int mpcekf_limit_map_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "limit_map_get", "LM", MPCEKF_NLM, nfields, fields, values);
  if (rc) return rc;
  if (!X->lmap) return fail(MPCEKF_E_STATE, "limit_map_get: call mpcekf_limit_map first");
  return get_rows(X, X->d_lm, (size_t)X->n, nfields, fields, values);
}

int mpcekf_limit_map_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "limit_map_end: null ctx");
  if (!X->lmap) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured with the map launch its kernels: none is replayed on a context without one
  X->retire_graphs([](const GraphParts &k) { return k.map.rec != 0; });
  X->lmap = false;  // the buffers stay to the context's end
  X->h_lm.nf = 0;
  if (X->lim_set) return limits_upload(X);  // the mapped fields back to what set_limits gave them
  X->percell = false;
  X->h_lim.clear();
  return MPCEKF_OK;
}

int mpcekf_step_ex_map(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr, const int32_t *slots,
                       int32_t nslots, double *obs, double *temp, double *heat, double *ucmd, int32_t *limiter,
                       double *bleed, double *zmin, double *vstr, double *istr, int32_t *capby, double *lim,
                       int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_map: null ctx");
  if (!X->lmap) return fail(MPCEKF_E_STATE, "step_ex_map: call mpcekf_limit_map first");
  if ((temp || heat) && !X->d_th)
    return fail(MPCEKF_E_STATE, "step_ex_map: temp / heat rows: call mpcekf_thermal_begin first");
  if ((ucmd || limiter) && !X->d_pk)
    return fail(MPCEKF_E_STATE, "step_ex_map: ucmd / limiter rows: call mpcekf_pack_begin first");
  if ((bleed || zmin) && !(X->d_pk && X->d_bl))
    return fail(MPCEKF_E_STATE, "step_ex_map: bleed / zmin rows: call mpcekf_balance_begin first");
  if ((vstr || istr || capby) && !(X->d_pk && X->d_ch))
    return fail(MPCEKF_E_STATE, "step_ex_map: vstr / istr / capby rows: call mpcekf_charger_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  o.bleed = bleed;
  o.zmin = zmin;
  o.vstr = vstr;
  o.istr = istr;
  o.capby = capby;
  o.lim = lim;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

int mpcekf_step_ex_thermal(mpcekf_ctx *X, int32_t nsteps, const mpcekf_traj *tr, const int32_t *slots, int32_t nslots,
                           double *obs, double *temp, double *heat, int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_thermal: null ctx");
  if (!X->d_th) return fail(MPCEKF_E_STATE, "step_ex_thermal: call mpcekf_thermal_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  return step_impl(X, nsteps, nullptr, tr, slots, nslots, obs, outputs_on_device, o);
}

// ---- series strings along the fused loop (mpcekf_pack.hip) ----
static_assert(NPKR == MPCEKF_NPK && PK_NLIM == MPCEKF_PK_NLIM && PK_STEPS == MPCEKF_PK_STEPS &&
                  PK_HEADROOM == MPCEKF_PK_HEADROOM,
              "mpcekf_pack.hpp's rows are include/mpcekf.h's MPCEKF_PK_*");

int mpcekf_pack_begin(mpcekf_ctx *X, int32_t series) {
  if (!X) return fail(MPCEKF_E_ARG, "pack_begin: null ctx");
  if (series < 1) return fail(MPCEKF_E_ARG, "pack_begin: series = %d: a string has 1 cell or more", series);
  if (X->n % series)
    return fail(MPCEKF_E_ARG, "pack_begin: series = %d does not divide ncells = %lld", series, (long long)X->n);
  int rc;
  // the charger's arrays are per string: another string length ends it
  if (X->d_ch && series != X->pk_series && (rc = mpcekf_charger_end(X))) return rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>((size_t)X->n, 1);
  double *rec = X->d_pk;
  if (!rec && (rc = dalloc(&rec, n * NPKR))) return rc;
  // all bits 0 is +0.0: the record's reset, behind every launch of an earlier call
  HIPCHK(hipMemsetAsync(rec, 0, n * NPKR * 8, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  X->d_pk = rec;
  X->pk_series = series;
  return MPCEKF_OK;
}

int mpcekf_pack_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "pack_get", "PK", MPCEKF_NPK, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_pk) return fail(MPCEKF_E_STATE, "pack_get: call mpcekf_pack_begin first");
  return get_rows(X, X->d_pk, (size_t)X->n, nfields, fields, values);
}

int mpcekf_pack_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "pack_end: null ctx");
  if (!X->d_pk) return MPCEKF_OK;
  int rc = mpcekf_thermal_couple_end(X);  // links need strings
  if (rc) return rc;
  if ((rc = mpcekf_balance_end(X))) return rc;  // and so does a balancer
  if ((rc = mpcekf_charger_end(X))) return rc;  // and a charger
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured on a pack context launch k_pack on the record: retired before it is freed
  X->retire_graphs([](const GraphParts &k) { return k.pack.rec != 0; });
  (void)hipFree(X->d_pk);
  X->d_pk = nullptr;
  X->pk_series = 0;
  return MPCEKF_OK;
}

int mpcekf_step_ex_pack(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                        const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                        int32_t *limiter, int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_pack: null ctx");
  if (!X->d_pk) return fail(MPCEKF_E_STATE, "step_ex_pack: call mpcekf_pack_begin first");
  if ((temp || heat) && !X->d_th)
    return fail(MPCEKF_E_STATE, "step_ex_pack: temp / heat rows: call mpcekf_thermal_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

// ---- passive balancing of pack strings along the fused loop (mpcekf_balance.hip) ----
static_assert(NBLP == MPCEKF_NBLP && BLP_I_BLEED == MPCEKF_BLP_I_BLEED && BLP_DZ_ON == MPCEKF_BLP_DZ_ON &&
                  BLP_DZ_OFF == MPCEKF_BLP_DZ_OFF && NBLR == MPCEKF_NBL && BL_STEPS_ON == MPCEKF_BL_STEPS_ON &&
                  BL_Q_BLEED == MPCEKF_BL_Q_BLEED && BL_SWITCHES == MPCEKF_BL_SWITCHES && BL_DZ_MAX == MPCEKF_BL_DZ_MAX &&
                  BL_DZ_LAST == MPCEKF_BL_DZ_LAST && BL_STEPS == MPCEKF_BL_STEPS,
              "mpcekf_balance.hpp's rows are include/mpcekf.h's MPCEKF_BLP_* / MPCEKF_BL_*");

int mpcekf_balance_begin(mpcekf_ctx *X, const double *params, int32_t compensate) {
  if (!X) return fail(MPCEKF_E_ARG, "balance_begin: null ctx");
  if (!params) return fail(MPCEKF_E_ARG, "balance_begin: null params");
  if (compensate != 0 && compensate != 1)
    return fail(MPCEKF_E_ARG, "balance_begin: compensate = %d is not 0 / 1", compensate);
  if (!X->d_pk) return fail(MPCEKF_E_STATE, "balance_begin: call mpcekf_pack_begin first");
  const size_t nc = (size_t)X->n;
  for (size_t c = 0; c < nc; ++c) {
    const double ib = params[BLP_I_BLEED * nc + c], on = params[BLP_DZ_ON * nc + c], off = params[BLP_DZ_OFF * nc + c];
    if (!(ib >= 0.0)) return fail(MPCEKF_E_ARG, "balance_begin: i_bleed[%zu] = %g: a current >= 0", c, ib);
    if (!(on > 0.0)) return fail(MPCEKF_E_ARG, "balance_begin: dz_on[%zu] = %g: a SOC fraction > 0", c, on);
    if (!(off >= 0.0 && off <= on))
      return fail(MPCEKF_E_ARG, "balance_begin: dz_off[%zu] = %g outside [0, dz_on = %g]", c, off, on);
  }
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_bl, *par = X->d_bl_par, *soc = X->d_bl_soc;
  int *on = X->d_bl_on;
  if ((!rec && (rc = dalloc(&rec, n * NBLR))) || (!par && (rc = dalloc(&par, n * NBLP))) ||
      (!soc && (rc = dalloc(&soc, n))) || (!on && (rc = dalloc(&on, n)))) {
    if (rec != X->d_bl) (void)hipFree(rec);
    if (par != X->d_bl_par) (void)hipFree(par);
    if (soc != X->d_bl_soc) (void)hipFree(soc);
    return rc;
  }
  // a first begin changes the launch sequence: the graphs of the balancer-free pack are not
  // replayed (their key holds 0 where these buffers now stand), so nothing is retired here
  X->d_bl = rec;
  X->d_bl_par = par;
  X->d_bl_soc = soc;
  X->d_bl_on = on;
  X->bl_comp = compensate;
  // behind every launch of an earlier call, which the stream orders before these
  if (nc) HIPCHK(hipMemcpyAsync(par, params, nc * NBLP * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_bal_reset(rec, on, X->n, X->stream), "bal_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_balance_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "balance_get", "BL", MPCEKF_NBL, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_bl) return fail(MPCEKF_E_STATE, "balance_get: call mpcekf_balance_begin first");
  return get_rows(X, X->d_bl, (size_t)X->n, nfields, fields, values);
}

int mpcekf_balance_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "balance_end: null ctx");
  if (!X->d_bl) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured on a balancing context launch k_pack_bal on these buffers: retired before
  // they are freed
  X->retire_graphs([](const GraphParts &k) { return k.balance.rec != 0; });
  void *ptrs[] = {X->d_bl, X->d_bl_par, X->d_bl_soc, X->d_bl_on};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  X->d_bl = X->d_bl_par = X->d_bl_soc = nullptr;
  X->d_bl_on = nullptr;
  X->bl_comp = 0;
  return MPCEKF_OK;
}

int mpcekf_step_ex_balance(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                           const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                           int32_t *limiter, double *bleed, double *zmin, int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_balance: null ctx");
  if (!X->d_pk || !X->d_bl) return fail(MPCEKF_E_STATE, "step_ex_balance: call mpcekf_balance_begin first");
  if ((temp || heat) && !X->d_th)
    return fail(MPCEKF_E_STATE, "step_ex_balance: temp / heat rows: call mpcekf_thermal_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  o.bleed = bleed;
  o.zmin = zmin;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

// ---- charger limits on pack strings along the fused loop (mpcekf_charger.hip) ----
static_assert(NCHP == MPCEKF_NCHP && CHP_I_MAX == MPCEKF_CHP_I_MAX && CHP_P_MAX == MPCEKF_CHP_P_MAX &&
                  NCHR == MPCEKF_NCH && CH_STEPS == MPCEKF_CH_STEPS && CH_NCAP_I == MPCEKF_CH_NCAP_I &&
                  CH_NCAP_P == MPCEKF_CH_NCAP_P && CH_Q == MPCEKF_CH_Q && CH_E == MPCEKF_CH_E &&
                  CH_CURTAIL == MPCEKF_CH_CURTAIL && CH_P_MIN == MPCEKF_CH_P_MIN && CH_V_PEAK == MPCEKF_CH_V_PEAK &&
                  CH_NVALID_MIN == MPCEKF_CH_NVALID_MIN,
              "mpcekf_charger.hpp's rows are include/mpcekf.h's MPCEKF_CHP_* / MPCEKF_CH_*");

int mpcekf_charger_begin(mpcekf_ctx *X, const double *params) {
  if (!X) return fail(MPCEKF_E_ARG, "charger_begin: null ctx");
  if (!params) return fail(MPCEKF_E_ARG, "charger_begin: null params");
  if (!X->d_pk) return fail(MPCEKF_E_STATE, "charger_begin: call mpcekf_pack_begin first");
  const size_t ns = (size_t)X->n / (size_t)X->pk_series;
  for (size_t g = 0; g < ns; ++g) {
    const double im = params[CHP_I_MAX * ns + g], pm = params[CHP_P_MAX * ns + g];
    if (im == im && !(im >= 0.0)) return fail(MPCEKF_E_ARG, "charger_begin: i_max[%zu] = %g: a current >= 0, or NaN", g, im);
    if (pm == pm && !(pm > 0.0)) return fail(MPCEKF_E_ARG, "charger_begin: p_max[%zu] = %g: a power > 0, or NaN", g, pm);
  }
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(ns, 1);
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_ch, *par = X->d_ch_par;
  if ((!rec && (rc = dalloc(&rec, n * NCHR))) || (!par && (rc = dalloc(&par, n * NCHP)))) {
    if (rec != X->d_ch) (void)hipFree(rec);
    return rc;
  }
  // a first begin changes the launch sequence: the graphs of the charger-free pack are not
  // replayed (their key holds 0 where these buffers now stand), so nothing is retired here
  X->d_ch = rec;
  X->d_ch_par = par;
  // behind every launch of an earlier call, which the stream orders before these
  if (ns) HIPCHK(hipMemcpyAsync(par, params, ns * NCHP * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_charger_reset(rec, (int64_t)ns, X->stream), "charger_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_charger_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "charger_get", "CH", MPCEKF_NCH, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_pk || !X->d_ch) return fail(MPCEKF_E_STATE, "charger_get: call mpcekf_charger_begin first");
  return get_rows(X, X->d_ch, (size_t)X->n / (size_t)X->pk_series, nfields, fields, values);  // a row per string
}

int mpcekf_charger_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "charger_end: null ctx");
  if (!X->d_ch) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured on a charger context launch k_charger on these buffers: retired before
  // they are freed
  X->retire_graphs([](const GraphParts &k) { return k.charger.rec != 0; });
  (void)hipFree(X->d_ch);
  if (X->d_ch_par) (void)hipFree(X->d_ch_par);
  X->d_ch = X->d_ch_par = nullptr;
  return MPCEKF_OK;
}

int mpcekf_step_ex_charger(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                           const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                           int32_t *limiter, double *bleed, double *zmin, double *vstr, double *istr, int32_t *capby,
                           int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_charger: null ctx");
  if (!X->d_pk || !X->d_ch) return fail(MPCEKF_E_STATE, "step_ex_charger: call mpcekf_charger_begin first");
  if ((bleed || zmin) && !X->d_bl)
    return fail(MPCEKF_E_STATE, "step_ex_charger: bleed / zmin rows: call mpcekf_balance_begin first");
  if ((temp || heat) && !X->d_th)
    return fail(MPCEKF_E_STATE, "step_ex_charger: temp / heat rows: call mpcekf_thermal_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  o.bleed = bleed;
  o.zmin = zmin;
  o.vstr = vstr;
  o.istr = istr;
  o.capby = capby;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

// ---- charge termination along the fused loop (mpcekf_term.hip) ----
static_assert(NTMR == MPCEKF_NTM && TM_STATE == MPCEKF_TM_STATE && TM_DONE_STEP == MPCEKF_TM_DONE_STEP &&
                  TM_REASON == MPCEKF_TM_REASON && TM_SOC_DONE == MPCEKF_TM_SOC_DONE && TM_U_DONE == MPCEKF_TM_U_DONE &&
                  TM_T_DONE == MPCEKF_TM_T_DONE && TM_REST == MPCEKF_TM_REST && TM_STEPS == MPCEKF_TM_STEPS &&
                  NTMP == MPCEKF_NTMP && TMP_SOC_STOP == MPCEKF_TMP_SOC_STOP && TMP_I_TAPER == MPCEKF_TMP_I_TAPER &&
                  TMP_T_CUT == MPCEKF_TMP_T_CUT && TERM_OPEN == MPCEKF_TERM_OPEN && TERM_LATCHED == MPCEKF_TERM_LATCHED &&
                  TERM_DEAD == MPCEKF_TERM_DEAD,
              "mpcekf_term.hpp's rows are include/mpcekf.h's MPCEKF_TM_* / MPCEKF_TMP_* / MPCEKF_TERM_*");

int mpcekf_term_begin(mpcekf_ctx *X, const double *params, int32_t hold) {
  if (!X) return fail(MPCEKF_E_ARG, "term_begin: null ctx");
  if (!params) return fail(MPCEKF_E_ARG, "term_begin: null params");
  if (hold < 1) return fail(MPCEKF_E_ARG, "term_begin: hold = %d: a taper holds for 1 step or more", hold);
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>((size_t)X->n, 1);
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_tm, *par = X->d_tm_par, *soc = X->d_tm_soc;
  int *ints = X->d_tm_int;
  if ((!rec && (rc = dalloc(&rec, n * NTMR))) || (!par && (rc = dalloc(&par, n * NTMP))) ||
      (!soc && (rc = dalloc(&soc, n))) || (!ints && (rc = dalloc(&ints, 4 * n + 1)))) {
    if (rec != X->d_tm) (void)hipFree(rec);
    if (par != X->d_tm_par) (void)hipFree(par);
    if (soc != X->d_tm_soc) (void)hipFree(soc);
    return rc;
  }
  X->d_tm = rec;
  X->d_tm_par = par;
  X->d_tm_soc = soc;
  X->d_tm_int = ints;
  X->tm_hold = hold;
  // behind every launch of an earlier call, which the stream orders before these
  if (X->n) HIPCHK(hipMemcpyAsync(par, params, (size_t)X->n * NTMP * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_term_reset(rec, X->tm_cnt(), X->tm_flag(0), X->tm_open(), X->n, X->stream), "term_reset")))
    return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_term_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "term_get", "TM", MPCEKF_NTM, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_tm) return fail(MPCEKF_E_STATE, "term_get: call mpcekf_term_begin first");
  return get_rows(X, X->d_tm, (size_t)X->n, nfields, fields, values);
}

int mpcekf_term_open(mpcekf_ctx *X, int64_t *open_cells) {
  if (!X) return fail(MPCEKF_E_ARG, "term_open: null ctx");
  if (!open_cells) return fail(MPCEKF_E_ARG, "term_open: null open_cells");
  if (!X->d_tm) return fail(MPCEKF_E_STATE, "term_open: call mpcekf_term_begin first");
  HIPCHK(hipSetDevice(X->device));
  int v = 0;
  HIPCHK(hipMemcpyAsync(&v, X->tm_open(), sizeof(int), hipMemcpyDeviceToHost, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  *open_cells = v;
  return MPCEKF_OK;
}

int mpcekf_term_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "term_end: null ctx");
  if (!X->d_tm) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured on a terminating context launch k_term on these buffers: retired before
  // they are freed
  X->retire_graphs([](const GraphParts &k) { return k.term.rec != 0; });
  void *ptrs[] = {X->d_tm, X->d_tm_par, X->d_tm_soc, X->d_tm_int};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  X->d_tm = X->d_tm_par = X->d_tm_soc = nullptr;
  X->d_tm_int = nullptr;
  X->tm_hold = 0;
  return MPCEKF_OK;
}

int mpcekf_step_until(mpcekf_ctx *X, int32_t max_steps, int32_t chunk, const double *tc_degC, int32_t *steps_run,
                      int64_t *open_cells) {
  if (!X) return fail(MPCEKF_E_ARG, "step_until: null ctx");
  if (max_steps < 0) return fail(MPCEKF_E_ARG, "step_until: max_steps = %d < 0", max_steps);
  if (chunk < 1) return fail(MPCEKF_E_ARG, "step_until: chunk = %d: 1 step or more per call", chunk);
  if (!X->d_tm) return fail(MPCEKF_E_STATE, "step_until: call mpcekf_term_begin first");
  if (!X->initialized) return fail(MPCEKF_E_STATE, "step_until: call mpcekf_init_cells first");
  if (X->d_th && tc_degC)
    return fail(MPCEKF_E_ARG, "step_until: tc_degC on a thermal context (mpcekf_thermal_begin): the model sets the temperature");
  int rc;
  const size_t n = (size_t)X->n;
  if (tc_degC && (rc = check_tc(tc_degC, n))) return rc;
  // the same row for every step of a chunk; the calls' shape repeats, so one graph replays
  std::vector<double> tcs;
  if (tc_degC)
    for (int k = 0; k < std::min(chunk, max_steps); ++k) tcs.insert(tcs.end(), tc_degC, tc_degC + n);
  const double *tcp = tc_degC ? tcs.data() : nullptr;
  int32_t run = 0;
  int64_t open = 0;
  if ((rc = mpcekf_term_open(X, &open))) return rc;
  StepOut o;
  o.sum = X->d_sum != nullptr;  // with a summary begun the record folds as in mpcekf_step_summary
  while (run < max_steps) {
    const int32_t m = std::min(chunk, max_steps - run);
    if ((rc = step_impl(X, m, tcp, nullptr, nullptr, 0, nullptr, 0, o))) return rc;
    run += m;
    if ((rc = mpcekf_term_open(X, &open))) return rc;  // one 4-byte copy
    if (open == 0) break;
  }
  if (steps_run) *steps_run = run;
  if (open_cells) *open_cells = open;
  return MPCEKF_OK;
}

// ---- side-reaction losses along the fused loop (mpcekf_aging.hip) ----
static_assert(NAGP == MPCEKF_NAGP && AG_I0 == MPCEKF_AG_I0 && AG_U == MPCEKF_AG_U && AG_ALPHA == MPCEKF_AG_ALPHA &&
                  AG_EA == MPCEKF_AG_EA && AG_GATE == MPCEKF_AG_GATE && NAGR == MPCEKF_NAGR &&
                  AGR_Q_SUM == MPCEKF_AGR_Q_SUM && AGR_J_MAX == MPCEKF_AGR_J_MAX &&
                  AGR_J_MAX_STEP == MPCEKF_AGR_J_MAX_STEP && AGR_N_ON == MPCEKF_AGR_N_ON &&
                  AGR_STEPS == MPCEKF_AGR_STEPS && AGR_NSKIP == MPCEKF_AGR_NSKIP && AG_MAXR == MPCEKF_AG_MAXREACT &&
                  (1 << AG_SRC_EST) == MPCEKF_AG_SRC_EST && (1 << AG_SRC_PLANT) == MPCEKF_AG_SRC_PLANT,
              "mpcekf_aging.hpp's rows are include/mpcekf.h's MPCEKF_AG_* / MPCEKF_AGR_*");

// the graphs captured on an aging context launch k_aging on the record and the rows: retired
// before any of them is freed, or when the launches they hold no longer fit nreact / sources
static void retire_aging_graphs(mpcekf_ctx *X) {
  X->retire_graphs([](const GraphParts &k) { return k.aging.rec != 0; });
}

int mpcekf_aging_begin(mpcekf_ctx *X, int32_t nreact, int32_t sources, const double *params) {
  if (!X) return fail(MPCEKF_E_ARG, "aging_begin: null ctx");
  if (!params) return fail(MPCEKF_E_ARG, "aging_begin: null params");
  if (nreact < 1 || nreact > MPCEKF_AG_MAXREACT)
    return fail(MPCEKF_E_ARG, "aging_begin: nreact = %d outside 1..%d", nreact, (int)MPCEKF_AG_MAXREACT);
  if (sources < 1 || sources > (MPCEKF_AG_SRC_EST | MPCEKF_AG_SRC_PLANT))
    return fail(MPCEKF_E_ARG, "aging_begin: sources = %d outside 1..3 (MPCEKF_AG_SRC_EST | MPCEKF_AG_SRC_PLANT)", sources);
  const size_t nc = (size_t)X->n;
  for (int r = 0; r < nreact; ++r) {
    const double *P = params + (size_t)r * MPCEKF_NAGP * nc;
    for (size_t c = 0; c < nc; ++c) {
      const double i0 = P[MPCEKF_AG_I0 * nc + c], U = P[MPCEKF_AG_U * nc + c], al = P[MPCEKF_AG_ALPHA * nc + c];
      const double Ea = P[MPCEKF_AG_EA * nc + c], gate = P[MPCEKF_AG_GATE * nc + c];
      if (!std::isfinite(i0) || i0 < 0)
        return fail(MPCEKF_E_ARG, "aging_begin: reaction %d: i0[%zu] = %g: must be finite and >= 0 (A)", r, c, i0);
      if (!std::isfinite(U)) return fail(MPCEKF_E_ARG, "aging_begin: reaction %d: U[%zu] = %g is not finite", r, c, U);
      if (!std::isfinite(al) || !(al > 0))
        return fail(MPCEKF_E_ARG, "aging_begin: reaction %d: alpha[%zu] = %g: must be finite and > 0", r, c, al);
      if (!std::isfinite(Ea)) return fail(MPCEKF_E_ARG, "aging_begin: reaction %d: Ea[%zu] = %g is not finite", r, c, Ea);
      if (gate != gate) return fail(MPCEKF_E_ARG, "aging_begin: reaction %d: gate[%zu] is NaN (+inf: always on)", r, c);
    }
  }
  // mpcekf_ctx_create accepts only a ROM with exactly one phise row at the negative collector
  // (MPCEKF_E_ROM otherwise, iterEKF.m:692-725), so every context's obs layout has the negPhise0
  // slot and this refusal cannot be reached today; it guards the plan below against a layout
  // that ever drops the field
  const int slot = X->obs_off[MPCEKF_OBS_negPhise0];
  if ((sources & MPCEKF_AG_SRC_PLANT) && X->obs_off[MPCEKF_OBS_negPhise0 + 1] <= slot)
    return fail(MPCEKF_E_UNSUPPORTED, "aging_begin: source PLANT: this ROM's obs layout has no negPhise0");
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // Every buffer before anything is stored: a failed allocation frees what this call allocated
  // and leaves the context as it was.  The phise row only for source EST, the negPhise0 row and
  // its plan only for source PLANT (a row an earlier begin allocated stays until mpcekf_aging_end).
  double *rec = X->d_ag, *par = X->d_ag_par, *phi = X->d_ag_phi, *ob = X->d_ag_obs;
  int *plan = X->d_ag_plan;
  const bool want_phi = sources & MPCEKF_AG_SRC_EST, want_ob = sources & MPCEKF_AG_SRC_PLANT;
  rc = MPCEKF_OK;
  if (!rc && !rec) rc = dalloc(&rec, n * AG_ROWS);
  if (!rc && !par) rc = dalloc(&par, n * AG_MAXR * NAGP);
  if (!rc && want_phi && !phi) rc = dalloc(&phi, n);
  if (!rc && want_ob && !ob) rc = dalloc(&ob, n);
  if (!rc && want_ob && !plan) rc = dalloc(&plan, 1);
  if (rc) {
    if (rec != X->d_ag) (void)hipFree(rec);
    if (par != X->d_ag_par) (void)hipFree(par);
    if (phi != X->d_ag_phi) (void)hipFree(phi);
    if (ob != X->d_ag_obs) (void)hipFree(ob);
    if (plan != X->d_ag_plan) (void)hipFree(plan);
    return rc;
  }
  if (X->d_ag && (X->ag_nreact != nreact || X->ag_sources != sources)) {
    HIPCHK(hipStreamSynchronize(X->stream));
    retire_aging_graphs(X);
  }
  X->d_ag = rec;
  X->d_ag_par = par;
  X->d_ag_phi = phi;
  X->d_ag_obs = ob;
  X->d_ag_plan = plan;
  X->ag_nreact = nreact;
  X->ag_sources = sources;
  X->ag_slot = -1;
  X->ag_need = 0;
  int src = 0;
  if (sources & MPCEKF_AG_SRC_PLANT) {  // the one-position plan, as step_impl forms a caller's
    X->ag_slot = slot;
    src = X->obs_slot_src[(size_t)slot];
    const int kind = src >= 0 ? (int)(X->ko.desc[src] & 15u) : -1;
    if (src == OBS_SRC_VCELL || kind == OBS_PPHIS) X->ag_need |= OBS_NEED_V;
    if (src == OBS_SRC_PHIE0 || kind == OBS_NPHISE || kind == OBS_PHIE) X->ag_need |= OBS_NEED_UN;
    if (kind == OBS_PPHISE) X->ag_need |= OBS_NEED_UP;
  }
  if (plan) HIPCHK(hipMemcpyAsync(plan, &src, sizeof(int), hipMemcpyHostToDevice, X->stream));
  if (nc) HIPCHK(hipMemcpyAsync(par, params, nc * (size_t)nreact * NAGP * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_aging_reset(rec, X->n, X->stream), "aging_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_aging_get(mpcekf_ctx *X, int32_t source, int32_t react, int32_t nfields, const int32_t *fields,
                     double *values) {
  int rc = check_rows(X, "aging_get", "AGR", MPCEKF_NAGR, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_ag) return fail(MPCEKF_E_STATE, "aging_get: call mpcekf_aging_begin first");
  if ((source != MPCEKF_AG_SRC_EST && source != MPCEKF_AG_SRC_PLANT) || !(X->ag_sources & source))
    return fail(MPCEKF_E_ARG, "aging_get: source = %d is not a source this context's begin enabled (mask %d)", source,
                X->ag_sources);
  if (react < 0 || react >= X->ag_nreact)
    return fail(MPCEKF_E_ARG, "aging_get: react = %d outside 0..%d", react, X->ag_nreact - 1);
  const int s = source == MPCEKF_AG_SRC_EST ? AG_SRC_EST : AG_SRC_PLANT;
  int32_t rows[MPCEKF_NAGR];  // the record rows of this source's and reaction's fields
  for (int i = 0; i < nfields; ++i) rows[i] = ag_row(s, react, fields[i]);
  return get_rows(X, X->d_ag, (size_t)X->n, nfields, rows, values);
}

int mpcekf_aging_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "aging_end: null ctx");
  if (!X->d_ag) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  retire_aging_graphs(X);
  void *ptrs[] = {X->d_ag, X->d_ag_par, X->d_ag_phi, X->d_ag_obs, X->d_ag_plan};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  X->d_ag = X->d_ag_par = X->d_ag_phi = X->d_ag_obs = nullptr;
  X->d_ag_plan = nullptr;
  X->ag_nreact = X->ag_sources = X->ag_need = 0;
  X->ag_slot = -1;
  return MPCEKF_OK;
}

int mpcekf_step_ex_aging(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                         const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                         int32_t *limiter, double *rate, int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_aging: null ctx");
  if (!X->d_ag) return fail(MPCEKF_E_STATE, "step_ex_aging: call mpcekf_aging_begin first");
  if ((temp || heat) && !X->d_th)
    return fail(MPCEKF_E_STATE, "step_ex_aging: temp / heat rows: call mpcekf_thermal_begin first");
  if ((ucmd || limiter) && !X->d_pk)
    return fail(MPCEKF_E_STATE, "step_ex_aging: ucmd / limiter rows: call mpcekf_pack_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  o.rate = rate;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

// ---- heat conduction between neighbouring cells of a pack string (mpcekf_thermal_couple.hip) ----
static_assert(NTCR == MPCEKF_NTCR && TCR_NB_SUM == MPCEKF_TCR_NB_SUM && TCR_DT_MAX == MPCEKF_TCR_DT_MAX &&
                  TCR_DT_MAX_STEP == MPCEKF_TCR_DT_MAX_STEP,
              "mpcekf_thermal_couple.hpp's rows are include/mpcekf.h's MPCEKF_TCR_*");

int mpcekf_thermal_couple(mpcekf_ctx *X, const double *r_link) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_couple: null ctx");
  if (!r_link) return fail(MPCEKF_E_ARG, "thermal_couple: null r_link");
  const size_t nc = (size_t)X->n;
  // every entry, the string ends' included: a later mpcekf_pack_begin may make any of them a link
  for (size_t c = 0; c < nc; ++c)
    if (!(r_link[c] > 0))
      return fail(MPCEKF_E_ARG, "thermal_couple: r_link[%zu] = %g: must be > 0 (K/W; +inf: no link)", c, r_link[c]);
  if (!X->d_th) return fail(MPCEKF_E_STATE, "thermal_couple: call mpcekf_thermal_begin first");
  if (!X->d_pk) return fail(MPCEKF_E_STATE, "thermal_couple: call mpcekf_pack_begin first");
  int rc;
  HIPCHK(hipSetDevice(X->device));
  const size_t n = std::max<size_t>(nc, 1);
  // every buffer before anything is stored: a failed allocation leaves the context as it was
  double *rec = X->d_tc, *link = X->d_tc_link, *snap = X->d_tc_snap;
  rc = MPCEKF_OK;
  if (!rc && !rec) rc = dalloc(&rec, n * NTCR);
  if (!rc && !link) rc = dalloc(&link, n);
  if (!rc && !snap) rc = dalloc(&snap, n * 2);
  if (rc) {
    if (rec != X->d_tc) (void)hipFree(rec);
    if (link != X->d_tc_link) (void)hipFree(link);
    if (snap != X->d_tc_snap) (void)hipFree(snap);
    return rc;
  }
  X->d_tc = rec;
  X->d_tc_link = link;
  X->d_tc_snap = snap;
  // behind every launch of an earlier call on the stream; a captured graph reads the links from
  // this buffer, so a replaced set needs no new graph
  if (nc) HIPCHK(hipMemcpyAsync(link, r_link, nc * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = lerr(launch_couple_reset(rec, X->n, X->stream), "couple_reset"))) return rc;
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_thermal_couple_get(mpcekf_ctx *X, int32_t nfields, const int32_t *fields, double *values) {
  int rc = check_rows(X, "thermal_couple_get", "TCR", MPCEKF_NTCR, nfields, fields, values);
  if (rc) return rc;
  if (!X->d_tc) return fail(MPCEKF_E_STATE, "thermal_couple_get: call mpcekf_thermal_couple first");
  return get_rows(X, X->d_tc, (size_t)X->n, nfields, fields, values);
}

int mpcekf_thermal_couple_end(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "thermal_couple_end: null ctx");
  if (!X->d_tc) return MPCEKF_OK;
  HIPCHK(hipSetDevice(X->device));
  HIPCHK(hipStreamSynchronize(X->stream));
  // the graphs captured on a coupled context launch its kernels on these buffers: retired before
  // they are freed
  X->retire_graphs([](const GraphParts &k) { return k.couple.rec != 0; });
  void *ptrs[] = {X->d_tc, X->d_tc_link, X->d_tc_snap};
  for (void *p : ptrs) (void)hipFree(p);
  X->d_tc = X->d_tc_link = X->d_tc_snap = nullptr;
  return MPCEKF_OK;
}

int mpcekf_step_ex_couple(mpcekf_ctx *X, int32_t nsteps, const double *tc_degC, const mpcekf_traj *tr,
                          const int32_t *slots, int32_t nslots, double *obs, double *temp, double *heat, double *ucmd,
                          int32_t *limiter, double *rate, double *cond, int32_t outputs_on_device) {
  if (!X) return fail(MPCEKF_E_ARG, "step_ex_couple: null ctx");
  if (!X->d_tc) return fail(MPCEKF_E_STATE, "step_ex_couple: call mpcekf_thermal_couple first");
  if (rate && !X->d_ag) return fail(MPCEKF_E_STATE, "step_ex_couple: rate rows: call mpcekf_aging_begin first");
  StepOut o;
  o.temp = temp;
  o.heat = heat;
  o.ucmd = ucmd;
  o.limiter = limiter;
  o.rate = rate;
  o.cond = cond;
  return step_impl(X, nsteps, tc_degC, tr, slots, nslots, obs, outputs_on_device, o);
}

int mpcekf_set_timing(mpcekf_ctx *X, int32_t enable) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  X->timing = enable != 0;
  X->timing_every = enable > 1 ? enable : 1;
  return MPCEKF_OK;
}

int mpcekf_get_timing(mpcekf_ctx *X, double *ms_sum, int64_t *launches) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  for (int j = 0; j < MPCEKF_NKERNELS; ++j) {
    if (ms_sum) ms_sum[j] = X->t_ms[j];
    if (launches) launches[j] = X->t_n[j];
    X->t_ms[j] = 0;
    X->t_n[j] = 0;
  }
  return MPCEKF_OK;
}

// ---- device memory owned by the library ---------------------------------------
// Callers that keep trajectories on the device (bench.py, the GPU tests, a MEX host)
// allocate them here, so a process holds exactly one HIP runtime: the one this
// library links.  A second runtime (e.g. a framework's bundled copy) in the same
// process owns its own HSA queues and address-space bookkeeping; pointers must not
// cross between the two.
int mpcekf_dev_alloc(int device, int64_t bytes, void **ptr) {
  if (!ptr || bytes < 0) return fail(MPCEKF_E_ARG, "dev_alloc: bad argument");
  *ptr = nullptr;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPCEKF_E_ARG, "dev_alloc: device %d of %d", device, ndev);
  if (bytes == 0) return MPCEKF_OK;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(ptr, (size_t)bytes));
  return MPCEKF_OK;
}

int mpcekf_dev_free(void *ptr) {
  if (ptr) HIPCHK(hipFree(ptr));
  return MPCEKF_OK;
}

static hipMemcpyKind copy_kind(int32_t kind) {
  return kind == MPCEKF_COPY_H2D ? hipMemcpyHostToDevice
       : kind == MPCEKF_COPY_D2H ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
}

int mpcekf_dev_copy(void *dst, const void *src, int64_t bytes, int32_t kind) {
  if (bytes < 0 || kind < MPCEKF_COPY_H2D || kind > MPCEKF_COPY_D2D || (bytes && (!dst || !src)))
    return fail(MPCEKF_E_ARG, "dev_copy: bad argument");
  if (bytes) HIPCHK(hipMemcpy(dst, src, (size_t)bytes, copy_kind(kind)));
  return MPCEKF_OK;
}

int mpcekf_dev_copy2d(void *dst, int64_t dpitch, const void *src, int64_t spitch, int64_t width, int64_t height,
                      int32_t kind) {
  if (width < 0 || height < 0 || dpitch < width || spitch < width || kind < MPCEKF_COPY_H2D ||
      kind > MPCEKF_COPY_D2D || (width && height && (!dst || !src)))
    return fail(MPCEKF_E_ARG, "dev_copy2d: bad argument");
  if (width && height)
    HIPCHK(hipMemcpy2D(dst, (size_t)dpitch, src, (size_t)spitch, (size_t)width, (size_t)height, copy_kind(kind)));
  return MPCEKF_OK;
}

int mpcekf_sync(mpcekf_ctx *X) {
  if (!X) return fail(MPCEKF_E_ARG, "null ctx");
  HIPCHK(hipSetDevice(X->device));
  int rc = X->drain();  // the _async stage calls' host outputs are written when this returns
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  return MPCEKF_OK;
}

int mpcekf_get_zk(mpcekf_ctx *X, double *zk, double *boundzk) {
  int rc = need_init(X);
  if (rc) return rc;
  size_t bytes = (size_t)X->n * (X->nz + 2) * 8;
  if (zk) HIPCHK(hipMemcpyAsync(zk, X->d_zk, bytes, hipMemcpyDeviceToHost, X->stream));
  if (boundzk) HIPCHK(hipMemcpyAsync(boundzk, X->d_zbk, bytes, hipMemcpyDeviceToHost, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

// ---- stage entry points ----------------------------------------------------
}  // extern "C"
// Host arrays are staged through one device scratch slab.
struct Slab {
  char *base;
  size_t off = 0;
  template <class T>
  T *take(size_t count) {
    T *p = (T *)(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};
// A stage call's host copies, through the context's pinned bounce buffer: inputs are copied
// into it and sent from there; outputs are DMA'd into it in chunks and copied out by the
// context's worker pool as each chunk's event completes (Copier), which the call's
// synchronisation (finish) waits for -- or, for an _async call (finish_async), the next one.
// Copies straight from / into the caller's pageable arrays let the runtime pin and cache
// those pages; the drop-ins' callers (MATLAB's mxArrays, numpy) free and reallocate their
// arrays every call, and the stage sequence then stalled 10-20 ms in whichever call came
// next (tools/dropin_probe.py: 0.6 ms with every array kept alive, 10-14 ms when freed,
// reused or not allocated; profiles/r05e_dropin_probe.jsonl).
struct Xfer {
  mpcekf_ctx *X;
  // bounced when below the cap and inside the buffer reserved (a copy beyond the
  // reservation goes direct rather than past the buffer's end)
  bool fits(size_t b) const { return b <= X->bounce_max && X->xoff + pad(b) <= X->h_bytes; }
  static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
  // capacity for the call's copies: pad(bytes) summed over those that will be bounced
  // (bounce_max caps a copy; MPCEKF_BOUNCE_MAX=0 pins nothing)
  int reserve(const std::vector<size_t> &copies) {
    size_t sum = 0;
    for (size_t b : copies)
      if (b && b <= X->bounce_max) sum += pad(b);
    return sum ? X->bounce(sum) : MPCEKF_OK;
  }
  hipError_t in(void *d, const void *h, size_t b) {
    if (!b) return hipSuccess;
    if (!fits(b)) return hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, X->stream);
    char *p = X->h_bounce + X->xoff;
    X->xoff += pad(b);
    std::memcpy(p, h, b);
    return hipMemcpyAsync(d, p, b, hipMemcpyHostToDevice, X->stream);
  }
  hipError_t out(void *h, const void *d, size_t b) {
    if (!b) return hipSuccess;
    if (!fits(b)) return hipMemcpyAsync(h, d, b, hipMemcpyDeviceToHost, X->stream);
    char *p = X->h_bounce + X->xoff;
    X->xoff += pad(b);
    for (size_t o = 0; o < b; o += X->xchunk) {
      const size_t len = std::min(X->xchunk, b - o);
      hipError_t e = hipMemcpyAsync(p + o, (const char *)d + o, len, hipMemcpyDeviceToHost, X->stream);
      hipEvent_t ev = nullptr;
      if (e == hipSuccess) e = X->next_event(&ev);
      if (e == hipSuccess) e = hipEventRecord(ev, X->stream);
      if (e != hipSuccess) return e;
      X->copier->push({ev, p + o, (char *)h + o, len});
    }
    return hipSuccess;
  }
  // the synchronous call's end: every output (this call's and any earlier _async call's) written
  int finish() { return X->drain(); }
  // an _async call's end: its copies stay in flight until mpcekf_sync or a synchronous call
  int finish_async() {
    X->xpending = true;
    return MPCEKF_OK;
  }
  int end(bool async) { return async ? finish_async() : finish(); }
};
static int set_tc(mpcekf_ctx *X, const double *tc, Xfer *xf) {
  if (!tc) return MPCEKF_OK;
  int rc = check_tc(tc, (size_t)X->n);
  if (rc) return rc;
  if (xf) HIPCHK(xf->in(X->s.Tc, tc, (size_t)X->n * 8));
  else HIPCHK(hipMemcpyAsync(X->s.Tc, tc, (size_t)X->n * 8, hipMemcpyHostToDevice, X->stream));
  return MPCEKF_OK;
}
extern "C" {

static int plant_step_impl(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!iapp) return fail(MPCEKF_E_ARG, "plant_step: null argument");
  size_t n = (size_t)X->n;
  Xfer xf{X};
  if ((rc = xf.reserve({n * 8, n * 8, n * 8}))) return rc;
  if ((rc = set_tc(X, tc_degC, &xf))) return rc;
  if ((rc = X->tmp(2 * n * 8 + 512)) || (rc = X->stage_bufs())) return rc;
  Slab sl{(char *)X->d_tmp};
  // Vcell also stays on the device for the next mpcekf_ekf_step (vk = NULL there: runMPC.m:88
  // -> :91 without a host round trip, which an _async plant call needs); vcell may be NULL
  double *di = sl.take<double>(n), *dv = X->d_sv;
  X->stage_v = false;
  HIPCHK(xf.in(di, iapp, n * 8));
  if ((rc = lerr(launch_plant(X->r, X->s, di, dv, 0, nullptr, X->stream), "plant"))) return rc;
  if ((rc = lerr(launch_bulk(X->r, X->k, X->s, di, 1, 0, X->stream), "bulk"))) return rc;
  if (vcell) HIPCHK(xf.out(vcell, dv, n * 8));
  if ((rc = xf.end(async))) return rc;
  X->stage_v = true;
  return MPCEKF_OK;
}
int mpcekf_plant_step(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell) {
  return plant_step_impl(X, iapp, tc_degC, vcell, false);
}
int mpcekf_plant_step_async(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell) {
  return plant_step_impl(X, iapp, tc_degC, vcell, true);
}

int mpcekf_obs_layout(const mpcekf_ctx *X, int32_t off[MPCEKF_OBS_COUNT + 1]) {
  if (!X || !off) return fail(MPCEKF_E_ARG, "obs_layout: null argument");
  std::memcpy(off, X->obs_off, sizeof X->obs_off);
  return MPCEKF_OK;
}

// mpcekf_plant_step with k_plant_obs in front: it reads the state of step t-1 that k_plant4
// is about to overwrite (SOCn / SOCp) and k_bulk to advance (bigx), on the same stream
static int plant_step_obs_impl(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell, double *obs,
                               bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!iapp) return fail(MPCEKF_E_ARG, "plant_step_obs: null argument");
  const size_t n = (size_t)X->n, ob = (size_t)X->ko.nobs * n * 8;
  Xfer xf{X};
  if ((rc = xf.reserve({n * 8, n * 8, n * 8, obs ? ob : 0}))) return rc;
  if ((rc = set_tc(X, tc_degC, &xf))) return rc;
  if ((rc = X->tmp(2 * n * 8 + 512)) || (rc = X->stage_bufs()) || (rc = X->obs_bufs())) return rc;
  Slab sl{(char *)X->d_tmp};
  double *di = sl.take<double>(n), *dv = X->d_sv;
  X->stage_v = X->stage_obs = false;
  HIPCHK(xf.in(di, iapp, n * 8));
  if ((rc = lerr(launch_plant_obs(X->r, X->s, X->ko, di, X->stream), "plant_obs"))) return rc;
  if ((rc = lerr(launch_plant(X->r, X->s, di, dv, 0, nullptr, X->stream), "plant"))) return rc;
  if ((rc = lerr(launch_bulk(X->r, X->k, X->s, di, 1, 0, X->stream), "bulk"))) return rc;
  if (vcell) HIPCHK(xf.out(vcell, dv, n * 8));
  if (obs) HIPCHK(xf.out(obs, X->d_obs, ob));
  if ((rc = xf.end(async))) return rc;
  X->stage_v = X->stage_obs = true;
  return MPCEKF_OK;
}
int mpcekf_plant_step_obs(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell, double *obs) {
  return plant_step_obs_impl(X, iapp, tc_degC, vcell, obs, false);
}
int mpcekf_plant_step_obs_async(mpcekf_ctx *X, const double *iapp, const double *tc_degC, double *vcell,
                                double *obs) {
  return plant_step_obs_impl(X, iapp, tc_degC, vcell, obs, true);
}

// the record is slot-major, so a slot is one contiguous [ncells] vector: a copy each, no kernel
static int plant_obs_slots_impl(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *out, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!X->stage_obs) return fail(MPCEKF_E_STATE, "plant_obs_slots: no mpcekf_plant_step_obs record on the device");
  if (nslots < 0 || (nslots && (!slots || !out))) return fail(MPCEKF_E_ARG, "plant_obs_slots: null argument");
  for (int i = 0; i < nslots; ++i)
    if (slots[i] < 0 || slots[i] >= X->ko.nobs)
      return fail(MPCEKF_E_ARG, "plant_obs_slots: slot %d outside 0..%d", slots[i], X->ko.nobs - 1);
  if (!nslots) return MPCEKF_OK;
  const size_t n = (size_t)X->n;
  Xfer xf{X};
  if ((rc = xf.reserve(std::vector<size_t>((size_t)nslots, n * 8)))) return rc;
  for (int i = 0; i < nslots; ++i) HIPCHK(xf.out(out + (size_t)i * n, X->d_obs + (size_t)slots[i] * n, n * 8));
  return xf.end(async);
}
int mpcekf_plant_obs_slots(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *out) {
  return plant_obs_slots_impl(X, slots, nslots, out, false);
}
int mpcekf_plant_obs_slots_async(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *out) {
  return plant_obs_slots_impl(X, slots, nslots, out, true);
}

static int ekf_step_impl(mpcekf_ctx *X, const double *vk, const double *ik, const double *tk_degC, double *zk,
                    double *boundzk, int32_t *xind_model, double *xind_gamma, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!ik) return fail(MPCEKF_E_ARG, "ekf_step: null argument");
  if (!vk && !X->stage_v) return fail(MPCEKF_E_STATE, "ekf_step: NULL vk but no mpcekf_plant_step before it");
  size_t n = (size_t)X->n, nzz = (size_t)X->nz + 2;
  Xfer xf{X};
  if ((rc = xf.reserve({n * 8, n * 8, n * 8, n * nzz * 8, n * nzz * 8, 16 * n, 32 * n})))
    return rc;
  if ((rc = set_tc(X, tk_degC, &xf))) return rc;
  if ((rc = X->tmp((2 * n + n * nzz) * 8 + 2048)) || (rc = X->stage_bufs())) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dvk = sl.take<double>(n), *dik = sl.take<double>(n), *dzb = sl.take<double>(n * nzz);
  // zk and Xind stay on the device for the next mpcekf_linearize (NULL there); each host
  // output is copied only when given
  double *dzk = X->d_szk, *dxg = X->d_sxg;
  int *dxm = X->d_sxm;
  X->stage_zk = X->stage_lin = false;
  if (vk) HIPCHK(xf.in(dvk, vk, n * 8));
  else dvk = X->d_sv;  // the last mpcekf_plant_step's Vcell, on the device
  HIPCHK(xf.in(dik, ik, n * 8));
  // iterEKF.m:55 lock-out must see the state before the time update: the bulk
  // update of a locked-out cell is harmless because the cell is stopped.
  // OB: the all-model time update (iterEKF.m:73-84); MB updates only its blended model (in k_cell)
  if (!X->mb && (rc = lerr(launch_bulk(X->r, X->k, X->s, nullptr, 0, 1, X->stream), "bulk"))) return rc;
  KIO io{};
  io.mode = MODE_EKF;
  io.vk_in = dvk;
  io.ik_in = dik;
  io.zk = dzk;
  io.zbk = boundzk ? dzb : nullptr;
  const bool bnd_kernel = boundzk && !X->mb;  // k_bounds from k_cell's record (MB: k_cell itself)
  io.bnd = bnd_kernel ? X->d_bnd : nullptr;
  io.xm_out = dxm;
  io.xg_out = dxg;
  if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream), "cell"))) return rc;
  if (bnd_kernel && (rc = lerr(launch_bounds(X->r, X->s, X->d_bnd, dzb, X->stream), "bounds"))) return rc;
  if (zk) HIPCHK(xf.out(zk, dzk, n * nzz * 8));
  if (boundzk) HIPCHK(xf.out(boundzk, dzb, n * nzz * 8));
  if (xind_model) HIPCHK(xf.out(xind_model, dxm, 4 * n * 4));
  if (xind_gamma) HIPCHK(xf.out(xind_gamma, dxg, 4 * n * 8));
  if ((rc = xf.end(async))) return rc;
  X->stage_zk = true;
  return MPCEKF_OK;
}
int mpcekf_ekf_step(mpcekf_ctx *X, const double *vk, const double *ik, const double *tk_degC, double *zk,
                    double *boundzk, int32_t *xind_model, double *xind_gamma) {
  return ekf_step_impl(X, vk, ik, tk_degC, zk, boundzk, xind_model, xind_gamma, false);
}
int mpcekf_ekf_step_async(mpcekf_ctx *X, const double *vk, const double *ik, const double *tk_degC, double *zk,
                    double *boundzk, int32_t *xind_model, double *xind_gamma) {
  return ekf_step_impl(X, vk, ik, tk_degC, zk, boundzk, xind_model, xind_gamma, true);
}

static int linearize_impl(mpcekf_ctx *X, const double *zk, const int32_t *xind_model, const double *xind_gamma,
                     const double *tk_degC, double *lin, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!zk != !xind_model || !xind_model != !xind_gamma)
    return fail(MPCEKF_E_ARG, "linearize: zk, xind_model and xind_gamma are all given or all NULL");
  if (!zk && !X->stage_zk) return fail(MPCEKF_E_STATE, "linearize: NULL zk / Xind but no mpcekf_ekf_step before it");
  size_t n = (size_t)X->n, nzz = (size_t)X->nz + 2;
  Xfer xf{X};
  if ((rc = xf.reserve({n * 8, n * nzz * 8, 16 * n, 32 * n, n * MPCEKF_LIN_SIZE * 8})))
    return rc;
  if ((rc = set_tc(X, tk_degC, &xf))) return rc;
  if ((rc = X->tmp((n * nzz + 4 * n) * 8 + 4 * n * 4 + 2048)) || (rc = X->stage_bufs())) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dzk = X->d_szk, *dxg = X->d_sxg, *dl = X->d_slin;
  int *dxm = X->d_sxm;
  if (zk) {  // the caller's zk / Xind (a host that changed them after iterEKF)
    dzk = sl.take<double>(n * nzz);
    dxg = sl.take<double>(4 * n);
    dxm = sl.take<int>(4 * n);
    HIPCHK(xf.in(dzk, zk, n * nzz * 8));
    HIPCHK(xf.in(dxm, xind_model, 4 * n * 4));
    HIPCHK(xf.in(dxg, xind_gamma, 4 * n * 8));
  }
  KIO io{};
  io.mode = MODE_LIN;
  io.zk_in = dzk;
  io.xm_in = dxm;
  io.xg_in = dxg;
  io.lin_out = dl;
  X->stage_lin = false;
  if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream), "cell"))) return rc;
  if (lin) HIPCHK(xf.out(lin, dl, n * MPCEKF_LIN_SIZE * 8));
  if ((rc = xf.end(async))) return rc;
  X->stage_lin = true;
  return MPCEKF_OK;
}
int mpcekf_linearize(mpcekf_ctx *X, const double *zk, const int32_t *xind_model, const double *xind_gamma,
                     const double *tk_degC, double *lin) {
  return linearize_impl(X, zk, xind_model, xind_gamma, tk_degC, lin, false);
}
int mpcekf_linearize_async(mpcekf_ctx *X, const double *zk, const int32_t *xind_model, const double *xind_gamma,
                     const double *tk_degC, double *lin) {
  return linearize_impl(X, zk, xind_model, xind_gamma, tk_degC, lin, true);
}

static int lin_fields_impl(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, const double *set, double *out, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!X->stage_lin) return fail(MPCEKF_E_STATE, "lin_fields: no mpcekf_linearize record on the device");
  if (nslots < 0 || nslots > MPCEKF_LIN_SIZE || (nslots && !slots)) return fail(MPCEKF_E_ARG, "lin_fields: bad slots");
  uint64_t seen = 0;  // a repeated slot would have several threads scatter into one record element
  for (int i = 0; i < nslots; ++i) {
    if (slots[i] < 0 || slots[i] >= MPCEKF_LIN_SIZE) return fail(MPCEKF_E_ARG, "lin_fields: slot %d", slots[i]);
    if (seen >> slots[i] & 1) return fail(MPCEKF_E_ARG, "lin_fields: slot %d given twice", slots[i]);
    seen |= (uint64_t)1 << slots[i];
  }
  if (!nslots || (!set && !out)) return MPCEKF_OK;
  // the slots gathered into / scattered from a compact [ncells][nslots] device buffer, which
  // crosses PCIe in one copy: only the named doubles move (per-slot pitched copies of 8-byte
  // columns cost 3.7 ms for 14 slots at 65,536 cells, profiles/r05b_dropin_capi_65536.json)
  const size_t n = (size_t)X->n, bytes = n * (size_t)nslots * 8;
  if ((rc = X->tmp(bytes + 1024))) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dc = sl.take<double>(n * (size_t)nslots);
  int *ds = sl.take<int>((size_t)nslots);
  Xfer xf{X};
  if ((rc = xf.reserve({(size_t)nslots * sizeof(int), bytes, bytes}))) return rc;
  HIPCHK(xf.in(ds, slots, (size_t)nslots * sizeof(int)));
  if (set) {
    HIPCHK(xf.in(dc, set, bytes));
    if ((rc = lerr(launch_cols(X->d_slin, X->n, MPCEKF_LIN_SIZE, ds, nslots, dc, true, X->stream), "cols"))) return rc;
  }
  if (out) {
    if ((rc = lerr(launch_cols(X->d_slin, X->n, MPCEKF_LIN_SIZE, ds, nslots, dc, false, X->stream), "cols"))) return rc;
    HIPCHK(xf.out(out, dc, bytes));
  }
  return xf.end(async);
}
int mpcekf_lin_fields(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, const double *set, double *out) {
  return lin_fields_impl(X, slots, nslots, set, out, false);
}
int mpcekf_lin_fields_async(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, const double *set, double *out) {
  return lin_fields_impl(X, slots, nslots, set, out, true);
}

int mpcekf_mpc_step(mpcekf_ctx *X, const double *lin, const double *soc_k1, double *uk, int32_t *nexec) {
  return mpcekf_mpc_step_ex(X, lin, soc_k1, uk, nexec, nullptr, nullptr, nullptr, nullptr);
}
int mpcekf_mpc_step_async(mpcekf_ctx *X, const double *lin, const double *soc_k1, double *uk, int32_t *nexec) {
  return mpcekf_mpc_step_ex_async(X, lin, soc_k1, uk, nexec, nullptr, nullptr, nullptr, nullptr);
}

static int mpc_step_ex_impl(mpcekf_ctx *X, const double *lin, const double *soc_k1, double *uk, int32_t *nexec,
                       double *J_unc, double *J_fin, double *norm_du, int32_t *nviol, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!uk) return fail(MPCEKF_E_ARG, "mpc_step: null argument");
  if (!lin && !X->stage_lin) return fail(MPCEKF_E_STATE, "mpc_step: NULL lin but no mpcekf_linearize record");
  if (!soc_k1 && !X->stage_zk) return fail(MPCEKF_E_STATE, "mpc_step: NULL soc_k1 but no mpcekf_ekf_step zk");
  size_t n = (size_t)X->n;
  if ((rc = X->tmp((n * MPCEKF_LIN_SIZE + 5 * n) * 8 + 2 * n * 4 + 4096))) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dl = sl.take<double>(n * MPCEKF_LIN_SIZE), *ds = sl.take<double>(n), *du = sl.take<double>(n);
  double *dju = sl.take<double>(n), *djf = sl.take<double>(n), *dnd = sl.take<double>(n);
  int *dn = sl.take<int>(n), *dv = sl.take<int>(n);
  Xfer xf{X};
  if ((rc = xf.reserve({n * MPCEKF_LIN_SIZE * 8, n * 8, n * 8, n * 8, n * 8, n * 8, n * 4, n * 4}))) return rc;
  if (lin) HIPCHK(xf.in(dl, lin, n * MPCEKF_LIN_SIZE * 8));
  else dl = X->d_slin;  // the device-resident record of the last mpcekf_linearize
  if (soc_k1) HIPCHK(xf.in(ds, soc_k1, n * 8));
  else if ((rc = lerr(launch_cols(X->d_szk, X->n, X->nz + 2, X->d_zslot, 1, ds, false, X->stream), "cols")))
    return rc;  // runMPC.m:99 mpcData.SOCk_1 = zk(end), from the last mpcekf_ekf_step's device zk
  KIO io{};
  io.mode = MODE_MPC;
  io.lin_in = dl;
  io.soc_k1_in = ds;
  io.uk_out = du;
  io.nexec = dn;
  // iterMPC.m:89-95's cost log (mpcData.cost) of this call
  io.junc_out = J_unc ? dju : nullptr;
  io.jfin_out = J_fin ? djf : nullptr;
  io.normdu_out = norm_du ? dnd : nullptr;
  io.nviol_out = nviol ? dv : nullptr;
  const double *lim = X->lim();
  if (X->wide) {
    if ((rc = lerr(launch_mpc_wide(X->k, X->s, io, X->w, X->stream, lim), "mpc_wide"))) return rc;
    if ((rc = lerr(launch_hild_wide(X->k, X->s, io, X->w, X->stream), "hild_wide"))) return rc;
  } else if (X->sw != 7) {
    if ((rc = lerr(launch_mpc_sw(X->sw, X->k, X->s, io, X->stream, lim), "mpc_sw"))) return rc;
    if ((rc = lerr(launch_hild_sw(X->sw, X->k, X->s, io, X->stream), "hild_sw"))) return rc;
  } else if (lim) {  // per-cell limits, every switch on: k_mpc_pc<7>, then k_cell's Hildreth pair
    if ((rc = lerr(launch_mpc_sw(7, X->k, X->s, io, X->stream, lim), "mpc_sw"))) return rc;
    if ((rc = lerr(launch_hild(X->k, X->s, io, X->stream), "hild"))) return rc;
  } else {
    if ((rc = lerr(launch_cell(X->r, X->k, X->s, io, X->stream), "cell"))) return rc;
    if ((rc = lerr(launch_hild(X->k, X->s, io, X->stream), "hild"))) return rc;
  }
  HIPCHK(xf.out(uk, du, n * 8));
  if (nexec) HIPCHK(xf.out(nexec, dn, n * 4));
  if (J_unc) HIPCHK(xf.out(J_unc, dju, n * 8));
  if (J_fin) HIPCHK(xf.out(J_fin, djf, n * 8));
  if (norm_du) HIPCHK(xf.out(norm_du, dnd, n * 8));
  if (nviol) HIPCHK(xf.out(nviol, dv, n * 4));
  return xf.end(async);
}
int mpcekf_mpc_step_ex(mpcekf_ctx *X, const double *lin, const double *soc_k1, double *uk, int32_t *nexec,
                       double *J_unc, double *J_fin, double *norm_du, int32_t *nviol) {
  return mpc_step_ex_impl(X, lin, soc_k1, uk, nexec, J_unc, J_fin, norm_du, nviol, false);
}
int mpcekf_mpc_step_ex_async(mpcekf_ctx *X, const double *lin, const double *soc_k1, double *uk, int32_t *nexec,
                       double *J_unc, double *J_fin, double *norm_du, int32_t *nviol) {
  return mpc_step_ex_impl(X, lin, soc_k1, uk, nexec, J_unc, J_fin, norm_du, nviol, true);
}

static int mpc_diag_impl(mpcekf_ctx *X, const double *lin, const double *uk_1, double *poles, double *sv, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!lin && !X->stage_lin) return fail(MPCEKF_E_STATE, "mpc_diag: NULL lin but no mpcekf_linearize record");
  if (!poles && !sv) return MPCEKF_OK;
  size_t n = (size_t)X->n;
  if ((rc = X->tmp((n * MPCEKF_LIN_SIZE + n + n * 3 * NA) * 8 + 2048))) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dl = sl.take<double>(n * MPCEKF_LIN_SIZE), *du = sl.take<double>(n), *dp = sl.take<double>(n * 2 * NA),
         *ds = sl.take<double>(n * NA);
  Xfer xf{X};
  if ((rc = xf.reserve({n * MPCEKF_LIN_SIZE * 8, n * 8, n * 2 * NA * 8, n * NA * 8})))
    return rc;
  if (lin) HIPCHK(xf.in(dl, lin, n * MPCEKF_LIN_SIZE * 8));
  else dl = X->d_slin;
  if (uk_1) HIPCHK(xf.in(du, uk_1, n * 8));
  else HIPCHK(hipMemcpyAsync(du, X->s.uk_1, n * 8, hipMemcpyDeviceToDevice, X->stream));
  rc = X->wide ? launch_cl_diag_wide(X->k, X->n, dl, du, poles ? dp : nullptr, sv ? ds : nullptr, X->stream, X->lim())
               : launch_cl_diag(X->k, X->n, dl, du, poles ? dp : nullptr, sv ? ds : nullptr, X->stream, X->lim());
  if ((rc = lerr(rc, "cl_diag"))) return rc;
  if (poles) HIPCHK(xf.out(poles, dp, n * 2 * NA * 8));
  if (sv) HIPCHK(xf.out(sv, ds, n * NA * 8));
  return xf.end(async);
}
int mpcekf_mpc_diag(mpcekf_ctx *X, const double *lin, const double *uk_1, double *poles, double *sv) {
  return mpc_diag_impl(X, lin, uk_1, poles, sv, false);
}
int mpcekf_mpc_diag_async(mpcekf_ctx *X, const double *lin, const double *uk_1, double *poles, double *sv) {
  return mpc_diag_impl(X, lin, uk_1, poles, sv, true);
}

// ---- context-free kernels ----------------------------------------------------
}  // extern "C"
namespace {
struct DevScope {
  hipStream_t st = nullptr;
  char *buf = nullptr;
  ~DevScope() {
    if (st) (void)hipStreamSynchronize(st);
    if (buf) (void)hipFree(buf);
    if (st) (void)hipStreamDestroy(st);
  }
};
}  // namespace
extern "C" {

int mpcekf_predmat(int device, int64_t n, int32_t Np, int32_t Nc, const double *a, const double *C, const double *D,
                   double *Phi, double *G) {
  if (n < 0 || (n && (!a || !C || !D || !Phi || !G))) return fail(MPCEKF_E_ARG, "predmat: bad argument");
  const bool wide = wide_supported(Np, Nc);
  if (!(Np == 5 && Nc == 2) && !wide) return fail(MPCEKF_E_UNSUPPORTED, "predmat: built for Np/Nc = 5/2 and 20/10");
  if (n == 0) return MPCEKF_OK;
  HIPCHK(hipSetDevice(device));
  DevScope d;
  HIPCHK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  size_t b_in = (size_t)n * 13 * 8, b_out = (size_t)n * (Np * 7 + Np * Nc) * 8;
  HIPCHK(hipMalloc((void **)&d.buf, b_in + b_out + 1024));
  double *da = (double *)d.buf, *dC = da + n * 6, *dD = dC + n * 6, *dP = dD + n, *dG = dP + n * Np * 7;
  HIPCHK(hipMemcpyAsync(da, a, n * 6 * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dC, C, n * 6 * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dD, D, n * 8, hipMemcpyHostToDevice, d.st));
  int rc = lerr(wide ? launch_predmat_wide(n, Np, Nc, da, dC, dD, dP, dG, d.st)
                     : launch_predmat(n, Np, Nc, da, dC, dD, dP, dG, d.st), "predmat");
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(Phi, dP, n * Np * 7 * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(G, dG, n * Np * Nc * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipStreamSynchronize(d.st));
  return MPCEKF_OK;
}

int mpcekf_constraints(int device, const mpcekf_config *cfg, double Q, int64_t n, const double *lin,
                       const double *uk_1, const double *soc_k1, double *M, double *gamma) {
  if (!cfg || n < 0 || (n && (!lin || !uk_1 || !soc_k1 || !M || !gamma)))
    return fail(MPCEKF_E_ARG, "constraints: bad argument");
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (n == 0) return MPCEKF_OK;
  KCfg k{};
  fill_kcfg(cfg, Q, k);
  HIPCHK(hipSetDevice(device));
  DevScope d;
  HIPCHK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  const int sw = sw_of(cfg), ncon = ncon_sw_of(cfg->Np, cfg->Nc, sw), Nc = cfg->Nc;  // check_cfg: sw != 7 only at 5/2
  HIPCHK(hipMalloc((void **)&d.buf, (size_t)n * (MPCEKF_LIN_SIZE + 2 + ncon * Nc + ncon) * 8 + 1024));
  double *dl = (double *)d.buf, *du = dl + n * MPCEKF_LIN_SIZE, *ds = du + n, *dM = ds + n, *dg = dM + n * ncon * Nc;
  HIPCHK(hipMemcpyAsync(dl, lin, n * MPCEKF_LIN_SIZE * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(du, uk_1, n * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(ds, soc_k1, n * 8, hipMemcpyHostToDevice, d.st));
  if ((rc = lerr(wide_supported(cfg->Np, Nc) ? launch_constraints_wide(k, cfg->Np, Nc, n, dl, du, ds, dM, dg, d.st)
                 : sw != 7                   ? launch_constraints_sw(sw, k, n, dl, du, ds, dM, dg, d.st)
                                             : launch_constraints(k, n, dl, du, ds, dM, dg, d.st),
                 "constraints")))
    return rc;
  HIPCHK(hipMemcpyAsync(M, dM, n * ncon * Nc * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(gamma, dg, n * ncon * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipStreamSynchronize(d.st));
  return MPCEKF_OK;
}

int mpcekf_hildreth(int device, int64_t n, int32_t Nc, int32_t ncon, const double *E, const double *F,
                    const double *M, const double *gamma, double *lambda, int32_t max_iter, double tol, double *DU,
                    int32_t *nexec) {
  if (n < 0 || (n && (!E || !F || !M || !gamma || !lambda || !DU || !nexec)))
    return fail(MPCEKF_E_ARG, "hildreth: bad argument");
  if (Nc < 1 || Nc > 10 || ncon < 1 || ncon > 100)
    return fail(MPCEKF_E_UNSUPPORTED, "hildreth: Nc must be 1..10 and the constraint count 1..100");
  if (max_iter < 1) return fail(MPCEKF_E_ARG, "hildreth: max_iter < 1");
  if (n == 0) return MPCEKF_OK;
  HIPCHK(hipSetDevice(device));
  DevScope d;
  HIPCHK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  size_t per = (size_t)(Nc * Nc + Nc + ncon * Nc + ncon + ncon + Nc);
  const bool any = Nc != 2 || ncon != NCON_BUILT;
  const size_t scr = any ? hildreth_any_scratch(n, Nc, ncon) : 0;
  HIPCHK(hipMalloc((void **)&d.buf, (size_t)n * per * 8 + (size_t)n * 4 + scr * 8 + 1024));
  double *dE = (double *)d.buf, *dF = dE + n * Nc * Nc, *dM = dF + n * Nc, *dg = dM + n * ncon * Nc,
         *dl = dg + n * ncon, *dD = dl + n * ncon;
  int *dn = (int *)(dD + n * Nc);
  HIPCHK(hipMemcpyAsync(dE, E, n * Nc * Nc * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dF, F, n * Nc * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dM, M, n * ncon * Nc * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dg, gamma, n * ncon * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dl, lambda, n * ncon * 8, hipMemcpyHostToDevice, d.st));
  double *dscr = any ? (double *)(((uintptr_t)(dn + n) + 255) & ~(uintptr_t)255) : nullptr;
  int rc = lerr(launch_hildreth(n, Nc, ncon, dE, dF, dM, dg, dl, max_iter, tol, dD, dn, d.st, dscr), "hildreth");
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(lambda, dl, n * ncon * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(DU, dD, n * Nc * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(nexec, dn, n * 4, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipStreamSynchronize(d.st));
  return MPCEKF_OK;
}

int mpcekf_hildreth_structured(int device, int64_t n, const double *E, const double *F, const double *Hv,
                               const double *He, const double *Hs, const double *gamma, double *lambda,
                               int32_t max_iter, double tol, double *DU, int32_t *nexec) {
  if (n < 0 || (n && (!E || !F || !Hv || !He || !Hs || !gamma || !lambda || !DU || !nexec)))
    return fail(MPCEKF_E_ARG, "hildreth_structured: bad argument");
  if (max_iter < 1) return fail(MPCEKF_E_ARG, "hildreth_structured: max_iter < 1");
  if (n == 0) return MPCEKF_OK;
  HIPCHK(hipSetDevice(device));
  DevScope d;
  HIPCHK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  const size_t NCn = 2, NPn = 5, NCONn = NCON_BUILT;
  const size_t per = NCn * NCn + NCn + 3 * NPn + NCONn + NCONn + NCn;
  HIPCHK(hipMalloc((void **)&d.buf, (size_t)n * per * 8 + (size_t)n * 4 + 1024));
  double *dE = (double *)d.buf, *dF = dE + n * NCn * NCn, *dHv = dF + n * NCn, *dHe = dHv + n * NPn,
         *dHs = dHe + n * NPn, *dg = dHs + n * NPn, *dl = dg + n * NCONn, *dD = dl + n * NCONn;
  int *dn = (int *)(dD + n * NCn);
  HIPCHK(hipMemcpyAsync(dE, E, n * NCn * NCn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dF, F, n * NCn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dHv, Hv, n * NPn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dHe, He, n * NPn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dHs, Hs, n * NPn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dg, gamma, n * NCONn * 8, hipMemcpyHostToDevice, d.st));
  HIPCHK(hipMemcpyAsync(dl, lambda, n * NCONn * 8, hipMemcpyHostToDevice, d.st));
  int rc = lerr(launch_hildreth_structured(n, dE, dF, dHv, dHe, dHs, dg, dl, max_iter, tol, dD, dn, d.st),
                "hildreth_structured");
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(lambda, dl, n * NCONn * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(DU, dD, n * NCn * 8, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipMemcpyAsync(nexec, dn, n * 4, hipMemcpyDeviceToHost, d.st));
  HIPCHK(hipStreamSynchronize(d.st));
  return MPCEKF_OK;
}

int mpcekf_get_hild_problems(mpcekf_ctx *X, double *prob, int32_t *hflag) {
  int rc = need_init(X);
  if (rc) return rc;
  static_assert(MPCEKF_PROB_DOUBLES == PROB_DOUBLES, "problem record size");
  if (X->wide) return fail(MPCEKF_E_UNSUPPORTED, "get_hild_problems: Np = 5 / Nc = 2 records only");
  const size_t n = (size_t)X->n;
  if (prob) HIPCHK(hipMemcpyAsync(prob, X->s.prob, n * PROB_DOUBLES * 8, hipMemcpyDeviceToHost, X->stream));
  if (hflag) HIPCHK(hipMemcpyAsync(hflag, X->s.hflag, n * 4, hipMemcpyDeviceToHost, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

int mpcekf_get_stamps(mpcekf_ctx *X, int64_t *stamps, int32_t *nstamps) {
  int rc = need_init(X);
  if (rc) return rc;
  static_assert(MPCEKF_NSTAMPS == NSTAMPS, "stamp count");
  if (nstamps) *nstamps = X->d_stamps ? NSTAMPS : 0;
  if (X->d_stamps && stamps) {
    HIPCHK(hipMemcpyAsync(stamps, X->d_stamps, (size_t)X->n * NSTAMPS * 8, hipMemcpyDeviceToHost, X->stream));
    HIPCHK(hipStreamSynchronize(X->stream));
  }
  return MPCEKF_OK;
}

// ---- state access ------------------------------------------------------------
static const int kScalMap[MPCEKF_NSCAL] = {0, 1, 2, 3, 4, 5, 6, 7};  // MPCEKF_S_* -> d_scal slot

int mpcekf_get_state(mpcekf_ctx *X, mpcekf_state *st) {
  int rc = need_init(X);
  if (rc) return rc;
  if (!st) return fail(MPCEKF_E_ARG, "get_state: null");
  const size_t n = (size_t)X->n, NM = (size_t)X->NM, nc = (size_t)X->ncon, ncd = (size_t)X->ncon_dev;
  if (st->bigX) HIPCHK(hipMemcpyAsync(st->bigX, X->s.bigx, n * NM * 6 * 8, hipMemcpyDeviceToHost, X->stream));
  if (st->ekf) HIPCHK(hipMemcpyAsync(st->ekf, X->s.ekf, n * NM * REC * 8, hipMemcpyDeviceToHost, X->stream));
  if (st->mb && X->mb) HIPCHK(hipMemcpyAsync(st->mb, X->d_mb, n * MBREC * 8, hipMemcpyDeviceToHost, X->stream));
  // only the requested fields cross PCIe (a MEX drop-in reading SOCnAvg/SOCpAvg each
  // step moves the 64-B scalar block per cell, not the NM-model records)
  std::vector<double> sc(st->scal ? n * 8 : 0), lam(st->lambda ? n * ncd : 0);
  std::vector<int> iv(st->warn || st->status ? n * 2 : 0);
  if (st->scal) HIPCHK(hipMemcpyAsync(sc.data(), X->d_scal, n * 8 * 8, hipMemcpyDeviceToHost, X->stream));
  if (st->lambda) HIPCHK(hipMemcpyAsync(lam.data(), X->s.lam, n * ncd * 8, hipMemcpyDeviceToHost, X->stream));
  if (!iv.empty()) HIPCHK(hipMemcpyAsync(iv.data(), X->d_int, n * 2 * 4, hipMemcpyDeviceToHost, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  for (size_t c = 0; c < n; ++c) {
    if (st->scal)
      for (int k = 0; k < MPCEKF_NSCAL; ++k) st->scal[c * MPCEKF_NSCAL + k] = sc[kScalMap[k] * n + c];
    if (st->lambda)  // the enabled rows in the reference's order (mpcData.lambda): [ncells][nC]
      for (size_t i = 0, ci = 0; i < ncd; ++i)
        if (row_enabled(X->cfg.Np, X->cfg.Nc, X->sw, (int)i)) st->lambda[c * nc + ci++] = lam[i * n + c];
    if (st->warn) st->warn[c] = iv[c];
    if (st->status) st->status[c] = iv[n + c];
  }
  return MPCEKF_OK;
}

static int get_scalars_impl(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *scal, int32_t *warn,
                            int32_t *status, bool async) {
  int rc = need_init(X);
  if (rc) return rc;
  if (nslots < 0 || nslots > MPCEKF_NSCAL || (nslots && (!slots || !scal)))
    return fail(MPCEKF_E_ARG, "get_scalars: bad slot list");
  for (int j = 0; j < nslots; ++j)
    if (slots[j] < 0 || slots[j] >= MPCEKF_NSCAL) return fail(MPCEKF_E_ARG, "get_scalars: slot %d", slots[j]);
  const size_t n = (size_t)X->n;
  // the SoA scalar block holds each slot as one contiguous [ncells] vector; a gather kernel
  // (k_rows) lays the requested ones out cell-major, so exactly those bytes cross PCIe in one
  // copy and the host does no transposition (nor the _async form at its synchronisation)
  int rows[MPCEKF_NSCAL];
  for (int j = 0; j < nslots; ++j) rows[j] = kScalMap[slots[j]];
  if ((rc = X->tmp(n * (size_t)nslots * 8 + 1024))) return rc;
  Slab sl{(char *)X->d_tmp};
  double *dc = sl.take<double>(n * (size_t)nslots);
  int *dr = sl.take<int>(MPCEKF_NSCAL);
  Xfer xf{X};
  if ((rc = xf.reserve({sizeof rows, n * (size_t)nslots * 8, n * 4, n * 4}))) return rc;
  if (nslots) {
    HIPCHK(xf.in(dr, rows, (size_t)nslots * sizeof(int)));
    if ((rc = lerr(launch_rows(X->d_scal, X->n, dr, nslots, dc, X->stream), "rows"))) return rc;
    HIPCHK(xf.out(scal, dc, n * (size_t)nslots * 8));
  }
  if (warn) HIPCHK(xf.out(warn, X->s.warn, n * 4));
  if (status) HIPCHK(xf.out(status, X->s.status, n * 4));
  return xf.end(async);
}
int mpcekf_get_scalars(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *scal, int32_t *warn,
                       int32_t *status) {
  return get_scalars_impl(X, slots, nslots, scal, warn, status, false);
}
int mpcekf_get_scalars_async(mpcekf_ctx *X, const int32_t *slots, int32_t nslots, double *scal, int32_t *warn,
                             int32_t *status) {
  return get_scalars_impl(X, slots, nslots, scal, warn, status, true);
}

int mpcekf_set_state(mpcekf_ctx *X, const mpcekf_state *st) {
  if (X) X->stage_zk = X->stage_lin = X->stage_v = X->stage_obs = false;  // the stage route's device hand-offs are stale
  int rc = need_init(X);
  if (rc) return rc;
  if (!st) return fail(MPCEKF_E_ARG, "set_state: null");
  const size_t n = (size_t)X->n, NM = (size_t)X->NM, nc = (size_t)X->ncon, ncd = (size_t)X->ncon_dev;
  if (st->bigX) HIPCHK(hipMemcpyAsync(X->s.bigx, st->bigX, n * NM * 6 * 8, hipMemcpyHostToDevice, X->stream));
  if (st->ekf) HIPCHK(hipMemcpyAsync(X->s.ekf, st->ekf, n * NM * REC * 8, hipMemcpyHostToDevice, X->stream));
  if ((rc = X->hot_clear())) return rc;  // both windows are empty between fused calls: they stay so
  if (st->mb && X->mb) HIPCHK(hipMemcpyAsync(X->d_mb, st->mb, n * MBREC * 8, hipMemcpyHostToDevice, X->stream));
  // scal and lambda are whole blocks (every slot given); warn and status share one block,
  // read back first when only one of them is given
  std::vector<double> sc(st->scal ? n * 8 : 0), lam(st->lambda ? n * ncd : 0);  // a disabled row's slot: 0
  std::vector<int> iv(st->warn || st->status ? n * 2 : 0);
  if (!iv.empty() && !(st->warn && st->status)) {
    HIPCHK(hipMemcpyAsync(iv.data(), X->d_int, n * 2 * 4, hipMemcpyDeviceToHost, X->stream));
    HIPCHK(hipStreamSynchronize(X->stream));
  }
  for (size_t c = 0; c < n; ++c) {
    if (st->scal)
      for (int k = 0; k < MPCEKF_NSCAL; ++k) sc[kScalMap[k] * n + c] = st->scal[c * MPCEKF_NSCAL + k];
    if (st->lambda)
      for (size_t i = 0, ci = 0; i < ncd; ++i)
        if (row_enabled(X->cfg.Np, X->cfg.Nc, X->sw, (int)i)) lam[i * n + c] = st->lambda[c * nc + ci++];
    if (st->warn) iv[c] = st->warn[c];
    if (st->status) iv[n + c] = st->status[c];
  }
  if (st->scal) HIPCHK(hipMemcpyAsync(X->d_scal, sc.data(), n * 8 * 8, hipMemcpyHostToDevice, X->stream));
  if (st->lambda) HIPCHK(hipMemcpyAsync(X->s.lam, lam.data(), n * ncd * 8, hipMemcpyHostToDevice, X->stream));
  if (!iv.empty()) HIPCHK(hipMemcpyAsync(X->d_int, iv.data(), n * 2 * 4, hipMemcpyHostToDevice, X->stream));
  HIPCHK(hipStreamSynchronize(X->stream));
  return MPCEKF_OK;
}

}  // extern "C"
