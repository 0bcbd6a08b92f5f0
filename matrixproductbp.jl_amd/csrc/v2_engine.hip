// Host side of the batched gauge sweep (v2_kernels.h): plans every time step of a lock-step batch on the host (all
// dimensions follow from the bond tables of the operands), uploads the per-problem descriptors and issues the launches.
#include "wg_common.h"
#define WG_THREADS 512
#define WG_WAVES 8
namespace v512 {
#include "wg_blocks.h"
}
#undef WG_THREADS
#undef WG_WAVES
#include "engine_types.h"
#include "v2_kernels.h"
#include "cq_kernels.h"
#include "ctx.h"
#include "v2_engine.h"
#include <mutex>

namespace {

inline int r16i(int x) { return (x + 15) & ~15; }
inline int r32i(int x) { return (x + 31) & ~31; }

struct QrDims { int rows, cols, kmax; };

// columns per block of the two-level Jacobi for factors of m rows, n columns: a block pair (2 nb columns, odd leading
// dimension) fits 150 KB of LDS, about eight blocks per factor (four workgroups per problem, seven launches per sweep), at
// most 32 columns (an inner sweep is 2 nb - 1 rounds with a barrier each); 0: does not fit (m > 1200)
inline int jac_block_nb(int m, int n) {
  static const int forced = [] { const char* e = getenv("MPBP_JACOBI_NB"); return e ? atoi(e) : 0; }();
  const int fit = (int)((150 * 1024 / 8 - 32) / (2 * (int64_t)(m | 1)));
  if (fit < 4) return 0;
  int nb = forced > 0 ? forced : std::max(8, (n + 7) / 8);
  nb = std::min(std::min(nb, 32), fit);
  return std::max(nb, 2);
}

// ------------------------------------------------------------------------------------------------------------------
// Look-ahead for the latency-bound case (one or two LARGE problems per launch: configs[3] hubs, configs[4]): the panel
// factorisation of block k+1 (17 cooperative column steps + Gram + T per 16 columns, ~25 launches per 64 columns, a
// handful of workgroups each) runs BESIDE the trailing update of block k instead of after it.  Two internal streams with
// disjoint CU masks (hipExtStreamCreateWithCUMask): the panel chain owns LA_RESERVED CUs - so the cooperative kernel's
// workgroups are co-resident by construction and its VALU-bound column steps do not share SIMDs with the trailing
// update's MFMA streams (which would slow them 3x, profiles/r03_dp_pipe_probe.txt) - the trailing update the rest.
//   stream B:  panel chain of block k   record(b)   wait(a: part 2 of block k-1)   part 1 of block k   ...block k+1
//   stream A:  wait(b)   part 2 of block k   record(a)
// part 1 = the next block's four panel tiles, updated in the fine-grained form of the in-block updates (quarter row
// chunks, ~90 us; the (8 tiles x row chunk) form takes ~340 us whatever the tile count: its time is one workgroup's pass
// over its 2048 rows), part 2 = all other tiles in the (8 tiles x row chunk) form.  Part 1 of block k needs part 2 of
// block k-1 (which brought those columns up to block k-1); block k+1's chain writes the second copy of the per-problem
// scratch (shift_auxlay) while part 2 of block k reads the first.
// ------------------------------------------------------------------------------------------------------------------
static const int LA_RESERVED = [] { const char* e = getenv("MPBP_LA_RESERVED"); const int v = e ? atoi(e) : 64; return (v >= 16 && v <= 128) ? v : 64; }();      // CUs of the panel stream
constexpr int LA_MAX_WGS = 24;       // look-ahead only while the batch is latency bound: row-chunk workgroups of all its problems (6400 x 1600 x 16 with 64 of them is throughput bound and loses 20 % to the reserved CUs)
struct LookAhead {
  hipStream_t sa = nullptr, sb = nullptr;
  hipEvent_t e_in = nullptr, e_a[2] = {nullptr, nullptr}, e_b = nullptr, e_out_a = nullptr, e_out_b = nullptr;
  bool ok = false, tried = false;
};
// Per-device state shared by every context (and self test) of the process on that device: the two CU-masked streams and
// six events of the look-ahead, and the "function attributes are set" flag.  Reference counted: mpbp_create /
// mpbp_selftest_qr_batched* acquire, mpbp_destroy / the end of the self test release, and the LAST release destroys the
// streams and events - so nothing of ours is alive when static destructors (and a profiler's finaliser) run at exit
// (round-3 review item 5).  The mutex makes creation safe for contexts of several host threads on one device; the streams
// themselves are used by one qr_batch at a time (include/mpbp_hip.h: contexts on one device share them - calls into
// different contexts of one device must not overlap in time).
struct DeviceShared { std::mutex mu; int refs = 0; bool attrs = false; LookAhead la; };
constexpr int MAX_DEV = 16;
static DeviceShared g_dev[MAX_DEV];

static void la_destroy(LookAhead& l) {
  if (l.sa) { (void)hipStreamSynchronize(l.sa); (void)hipStreamDestroy(l.sa); }
  if (l.sb) { (void)hipStreamSynchronize(l.sb); (void)hipStreamDestroy(l.sb); }
  for (hipEvent_t e : {l.e_in, l.e_a[0], l.e_a[1], l.e_b, l.e_out_a, l.e_out_b}) if (e) (void)hipEventDestroy(e);
  l = LookAhead{};
}
static LookAhead* lookahead_streams() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
  DeviceShared& D = g_dev[dev];
  std::lock_guard<std::mutex> lk(D.mu);
  if (D.refs <= 0) return nullptr;             // nobody holds the device: there would be no one to release the streams
  LookAhead& l = D.la;
  if (!l.tried) {
    l.tried = true;
    if (getenv("MPBP_DEBUG_NO_LOOKAHEAD")) return nullptr;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return nullptr;
    const int ncu = pr.multiProcessorCount, words = (ncu + 31) / 32;
    if (ncu < 2 * LA_RESERVED) return nullptr;
    std::vector<uint32_t> mb(words, 0u), ma(words, 0u);
    for (int i = 0; i < ncu; i++) (i < LA_RESERVED ? mb : ma)[i / 32] |= 1u << (i % 32);
    if (hipExtStreamCreateWithCUMask(&l.sa, words, ma.data()) != hipSuccess) { (void)hipGetLastError(); l.sa = nullptr; return nullptr; }
    if (hipExtStreamCreateWithCUMask(&l.sb, words, mb.data()) != hipSuccess) { (void)hipGetLastError(); l.sb = nullptr; la_destroy(l); l.tried = true; return nullptr; }
    bool ev = true;
    for (hipEvent_t* e : {&l.e_in, &l.e_a[0], &l.e_a[1], &l.e_b, &l.e_out_a, &l.e_out_b}) ev = ev && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    l.ok = ev;
  }
  return l.ok ? &l : nullptr;
}
// dynamic-LDS limits of the batched QR's kernels: an attribute belongs to the (function, device) pair, so it is set once
// per device (it used to be set 6-7 times per qr_batch call, ~400 intercepted API calls per gauge sweep).  The flag is
// published only after every call has succeeded, under the mutex, so that no thread launches before they have run.
static hipError_t set_func_attrs() {
  const std::pair<const void*, int> lim[] = {
      {(const void*)v2::k_fpanel, (int)v2::fpanel_lds_bytes(3)},
      {(const void*)cq::k_cq_upd<256>, cq::UPD_LDS_DOUBLES * 8},
      {(const void*)cq::k_cq_updfac, cq::UPD_LDS_DOUBLES * 8},
      {(const void*)cq::k_cq_fac2, cq::FAC_LDS_DOUBLES * 8},
      {(const void*)v2::k_jac_block, 152 * 1024}};
  for (const auto& l : lim) {
    const hipError_t e = hipFuncSetAttribute(l.first, hipFuncAttributeMaxDynamicSharedMemorySize, l.second);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
static hipError_t set_func_attrs_once() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return set_func_attrs();
  std::lock_guard<std::mutex> lk(g_dev[dev].mu);
  if (g_dev[dev].attrs) return hipSuccess;
  const hipError_t e = set_func_attrs();
  g_dev[dev].attrs = e == hipSuccess;
  return e;
}

// ------------------------------------------------------------------------------------------------------------------
// Debug and tuning switches of the batched QR and of the gauge sweep, read from the environment once per
// v2_gauge_sweep call and once per self-test call and passed down: tests switch them between calls of one process, so
// none is cached for the process.  (Read where they are used, once per device or process: MPBP_LA_RESERVED,
// MPBP_JACOBI_NB, MPBP_DEBUG_NO_LOOKAHEAD, MPBP_V2_TIMING.)
// ------------------------------------------------------------------------------------------------------------------
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
struct QrEnv {
  bool no_coop_panel;    // MPBP_DEBUG_NO_COOP_PANEL: one launch per column step instead of the cooperative panel kernel
  int coop_nt;           // MPBP_COOP_NT=2: two tiles per wave in the (tiles x row chunk) trailing update
  bool no_caqr;          // MPBP_DEBUG_NO_CAQR: never the communication-avoiding form
  int cq_min_rows;       // MPBP_CQ_MIN_ROWS: the communication-avoiding form above this many rows (default one row chunk)
  bool cq_nofuse;        // MPBP_DEBUG_CQ_NOFUSE: update and next level's factorisation as two launches
  double cq_img_us;      // MPBP_CQ_IMG_US: fixed cost of a tile-update workgroup in cq_tiles_per_group
  bool no_coop_trail;    // MPBP_DEBUG_NO_COOP_TRAIL: no (tiles x row chunk) trailing update, hence no look-ahead
  bool no_fused_trail;   // MPBP_DEBUG_NO_FUSED_TRAIL: no one-wave-per-tile-pair trailing update
  int trail_nt;          // MPBP_TRAIL_NT=1: one tile pair per wave in that form
};
QrEnv read_qr_env() {
  const char* img = getenv("MPBP_CQ_IMG_US");
  return QrEnv{env_set("MPBP_DEBUG_NO_COOP_PANEL"), env_int("MPBP_COOP_NT", 0), env_set("MPBP_DEBUG_NO_CAQR"), env_int("MPBP_CQ_MIN_ROWS", v2::CH),
               env_set("MPBP_DEBUG_CQ_NOFUSE"), img ? atof(img) : 30.0, env_set("MPBP_DEBUG_NO_COOP_TRAIL"), env_set("MPBP_DEBUG_NO_FUSED_TRAIL"),
               env_int("MPBP_TRAIL_NT", 2)};
}
enum JacobiForm { JAC_AUTO, JAC_WG, JAC_GRID, JAC_BLOCK };
struct JacobiEnv {
  bool force_tall;       // MPBP_DEBUG_FORCE_TALL=1: column-step panels in every QR of the sweep, even where register panels fit
  JacobiForm form;       // MPBP_JACOBI_FORM = wg | grid | block (choose_jacobi)
  int grid_sweeps;       // MPBP_JACOBI_GRID_SWEEPS: sweep limit of the block and grid forms
  int grid_min, grid_maxp, block_min, block_maxp;   // MPBP_JACOBI_GRID_MIN / _GRID_MAXP / _BLOCK_MIN / _BLOCK_MAXP
};
JacobiEnv read_jacobi_env() {
  const char* tall = getenv("MPBP_DEBUG_FORCE_TALL");
  const char* f = getenv("MPBP_JACOBI_FORM");
  const JacobiForm form = !f ? JAC_AUTO : !strcmp(f, "wg") ? JAC_WG : !strcmp(f, "grid") ? JAC_GRID : !strcmp(f, "block") ? JAC_BLOCK : JAC_AUTO;
  return JacobiEnv{tall && tall[0] == '1', form, env_int("MPBP_JACOBI_GRID_SWEEPS", 60), env_int("MPBP_JACOBI_GRID_MIN", 384),
                   env_int("MPBP_JACOBI_GRID_MAXP", 4), env_int("MPBP_JACOBI_BLOCK_MIN", 320), env_int("MPBP_JACOBI_BLOCK_MAXP", 32)};
}

// ------------------------------------------------------------------------------------------------------------------
// One R-only QR over a batch whose dimensions are known on the host: qr_batch picks the form, qr_tree / qr_lookahead_block
// / qr_panel_block hold the launch sequences.
// ------------------------------------------------------------------------------------------------------------------
// what the launch sequences share.  lay[1]: the second copy of every problem's scratch (the look-ahead's)
struct QrBatch {
  hipStream_t st; const v2::QrProb* d_probs; int P, nchunk; v2::AuxLay lay[2]; int* coop_err; const QrEnv& env;
  int kmax_max, kmax_min, rows32_max, cols_max;
};
// the kernels that are compiled once per number of panels NP applied, indexed by NP - 1
decltype(&v2::k_inblock<1>) const kInblock[3] = {v2::k_inblock<1>, v2::k_inblock<2>, v2::k_inblock<3>};
struct TrailKernels { decltype(&v2::k_trailW<1>) W; decltype(&v2::k_trailU<1>) U; };
const TrailKernels kTrail[4] = {{v2::k_trailW<1>, v2::k_trailU<1>}, {v2::k_trailW<2>, v2::k_trailU<2>}, {v2::k_trailW<3>, v2::k_trailU<3>}, {v2::k_trailW<4>, v2::k_trailU<4>}};
// W = T^T (V^T C - S W) of np panels of block jb, then C -= V W, over `grid` (k_trailW / k_trailU for the arguments)
void launch_trail(int np, dim3 grid, hipStream_t s, const QrBatch& b, const v2::AuxLay& L, int jb, int inblock, int tw, int only_short) {
  hipLaunchKernelGGL(kTrail[np - 1].W, grid, dim3(256), 0, s, b.d_probs, L, jb, inblock, tw, only_short, 0);
  hipLaunchKernelGGL(kTrail[np - 1].U, grid, dim3(256), 0, s, b.d_probs, L, jb, inblock, tw, only_short, 0);
}

// the panel chain of block jb (npmax panels: in-block update, column steps, Gram, T) on stream s with scratch layout L
void panel_chain(const QrBatch& b, hipStream_t s, const v2::AuxLay& L, int jb, int npmax, bool tall, int coop_wgs) {
  const int P = b.P, nchunk = b.nchunk;
  for (int p = 0; p < npmax; p++) {
    const int jp = jb + 16 * p;
    if (p > 0 && !tall) hipLaunchKernelGGL(kInblock[p - 1], dim3(P), dim3(512), 0, s, b.d_probs, L, jb);
    if (p > 0 && tall) {
      // few problems: a quarter chunk per workgroup (tw = 0, grid.x = 4); many: a chunk per workgroup (tw = 1)
      const int twi = ((int64_t)nchunk * P <= 128) ? 0 : 1;
      launch_trail(p, dim3(twi == 0 ? 4 : 1, nchunk, P), s, b, L, jb, 1, twi, 0);
    }
    if (!tall) {
      hipLaunchKernelGGL(v2::k_fpanel, dim3(P), dim3(512), v2::fpanel_lds_bytes(p), s, b.d_probs, L, jb, p);
      continue;
    }
    // every row-chunk workgroup resident at once: one launch with arrival counters; else one launch per column
    // (the cooperative kernel needs all the row-chunk workgroups of a problem resident together: a batch too large
    // for that goes through it in groups of problems, as long as that takes fewer launches than the 17 column steps)
    const int pb = (nchunk > 0) ? coop_wgs / nchunk : 0;          // problems per cooperative launch
    if (b.coop_err && !b.env.no_coop_panel && pb >= 1 && (P + pb - 1) / pb <= 8) {
      for (int p0 = 0; p0 < P; p0 += pb)
        hipLaunchKernelGGL(v2::k_colsteps_coop, dim3(nchunk, std::min(pb, P - p0)), dim3(512), 0, s, b.d_probs + p0, L, jp, p, b.coop_err);
    } else
      for (int jj = 0; jj <= 16; jj++)
        hipLaunchKernelGGL(v2::k_colstep, dim3(nchunk, P), dim3(512), 0, s, b.d_probs, L, jp, jj, p);
    hipLaunchKernelGGL(v2::k_gram, dim3(nchunk * v2::GSUB, P), dim3(512), 0, s, b.d_probs, L, jb, p);
    hipLaunchKernelGGL(v2::k_build_T, dim3(P), dim3(256), 0, s, b.d_probs, L, jb, p);
  }
}
// tiles [t0, t1) of the 4-panel trailing update in the (8 tiles x row chunk) form
void trail_coop(const QrBatch& b, hipStream_t s, const v2::AuxLay& L, int jb, int t0, int t1) {
  if (t1 <= t0) return;
  if (b.env.coop_nt != 2) {   // one tile per wave measured 8-20 % faster at every size tried (two workgroups per CU)
    const dim3 gc((t1 - t0 + 7) / 8, b.nchunk, b.P);
    hipLaunchKernelGGL(v2::k_trailW_coop<1>, gc, dim3(512), 0, s, b.d_probs, L, jb, t0, t1);
    hipLaunchKernelGGL(v2::k_trailU_coop<1>, gc, dim3(512), 0, s, b.d_probs, L, jb, t0, t1);
  } else {
    const dim3 gc((t1 - t0 + 15) / 16, b.nchunk, b.P);
    hipLaunchKernelGGL(v2::k_trailW_coop<2>, gc, dim3(512), 0, s, b.d_probs, L, jb, t0, t1);
    hipLaunchKernelGGL(v2::k_trailU_coop<2>, gc, dim3(512), 0, s, b.d_probs, L, jb, t0, t1);
  }
}

// Tiles per workgroup of a communication-avoiding update over ntl tiles, n nodes, P problems: one tile per wave for the
// small upper levels; else the number of tile groups with the fewest (rounds over the CUs) x (time of a workgroup: a fixed
// part + 6.2 us per tile, measured with the chip full) - it decides how the last round is filled.  The fixed part: ~15 us
// of image load + the first tile's wait; swept 4 ... 50 us on four shapes (round 4, with the rewritten tile update): flat
// within 1 % from 8 to 50 on the many-problem shapes, 6400 x 1600 x 16 22.0 -> 21.4 ms and 16384 x 4096 26.9 -> 26.7 ms
// at 30.  Four-wave workgroups always: the fused update + factor launch needs that shape, and the two-waves-per-SIMD build
// of the update alone (cq_kernels.h, compute_tile) wins only at >= 128 problems (profiles/r04_cq_upd_probe.txt).
int cq_tiles_per_group(int ntl, int n, int P, int ncu, double img_us) {
  if ((int64_t)ntl * n * P <= 4 * ncu) return 4;
  int tpg = 8;
  double best = 1e30;
  for (int g = 1; g <= (ntl + 7) / 8; g++) {
    const int t = (ntl + g - 1) / g;
    if (t > 64) continue;
    const int64_t wgs = (int64_t)((ntl + t - 1) / t) * n * P;
    const double cost = (double)((wgs + ncu - 1) / ncu) * (img_us + 6.2 * t);
    if (cost < best) { best = cost; tpg = t; }
  }
  return tpg;
}
// Communication-avoiding form (cq_kernels.h): tall problems, every one with rows >= cols; the node slots live in the
// per-problem scratch behind the fixed headers of BOTH copies (which sit together at the front: lay.part on = the partial
// products / Grams / W0 of the other form, first and second copy back to back), so a call never touches the arrival
// counters a later look-ahead call on the same scratch relies on (round-3 advisor).
bool qr_tree_applies(const QrBatch& b, const std::vector<QrDims>& dims, bool force_tall, int64_t aux2) {
  bool tall_all = true;
  for (const QrDims& d : dims) tall_all = tall_all && d.rows >= d.cols;
  int64_t slots = 0;
  for (int n = (b.rows32_max + 255) / 256;; n = (n + 3) / 4) { slots += n; if (n == 1) break; }
  return !b.env.no_caqr && !force_tall && aux2 > 0 && tall_all && b.rows32_max > b.env.cq_min_rows && b.lay[0].part + slots * cq::IMG_DOUBLES <= 2 * aux2;
}
// One stream, one launch after the other.  Measured and dropped (round 3): (a) the upper-level factorisations of a
// single problem on a CU-masked stream beside the updates - the 20-40 us per event hand-over and the CUs taken from
// the updates cost what the overlap gained (16384 x 4096: 43.9 against 44.4 ms at the time); (b) the batch cut into
// 2 / 4 groups of problems on their own streams, so that one group's narrow launches fill CUs beside another's wide
// ones: 6400 x 1600 x 16 26.9 -> 28.0 / 34.5 ms, 7200 x 900 x 128 69.9 -> 67.1 / 71.6 ms.
// Per block: F_0, then one launch per level with the update U_l and the next level's factorisation F_{l+1} (k_cq_updfac).
void qr_tree(const QrBatch& b, int ncu) {
  const int P = b.P, cols16_max = r16i(b.cols_max);
  const int64_t ws_off = b.lay[0].part;
  for (int jb = 0; jb < b.kmax_max; jb += 64) {
    const int ntl = cols16_max > jb + 64 ? (cols16_max - jb - 64) / 16 : 0;
    int nl[12], nlev = 0;
    for (int n = (b.rows32_max - jb + 255) / 256; nlev < 12; n = (n + 3) / 4) { nl[nlev++] = n; if (n == 1) break; }
    int slot = 0;
    // (Round 3 had a second build of this kernel at two waves per SIMD for launches with more nodes than CUs.  Since the
    //  column steps are straight-line code the one-per-CU build is as fast per CU - 7200 x 900 x 128: 63.5 against 63.8 ms,
    //  21600 x 900 x 16: 28.1 / 28.2, 6400 x 1600 x 16: 22.5 / 22.4 - and the other one carried 1072 spills: removed.)
    hipLaunchKernelGGL(cq::k_cq_fac2, dim3(nl[0], P), dim3(256), cq::FAC_LDS_DOUBLES * 8, b.st, b.d_probs, ws_off, jb, 0, 0, 0);
    for (int level = 0; level < nlev; level++) {
      const int n = nl[level];
      const bool more = level + 1 < nlev;
      const int tpg = ntl > 0 ? cq_tiles_per_group(ntl, n, P, ncu, b.env.cq_img_us) : 8;
      const int ntg = ntl > 0 ? (ntl + tpg - 1) / tpg : 0;
      if (ntl > 0 && more && !b.env.cq_nofuse) {
        const int64_t wgs = (int64_t)P * nl[level + 1] + (int64_t)P * n * ntg;
        hipLaunchKernelGGL(cq::k_cq_updfac, dim3((unsigned)wgs), dim3(256), cq::UPD_LDS_DOUBLES * 8, b.st, b.d_probs, P, ws_off, jb, level, slot, n, ntg,
                           tpg, slot + n, nl[level + 1]);
      } else {
        if (ntl > 0)
          hipLaunchKernelGGL(cq::k_cq_upd<256>, dim3(ntg, n, P), dim3(256), cq::UPD_LDS_DOUBLES * 8, b.st, b.d_probs, ws_off, jb, level, slot, tpg, 0);
        if (more)
          hipLaunchKernelGGL(cq::k_cq_fac2, dim3(nl[level + 1], P), dim3(256), cq::FAC_LDS_DOUBLES * 8, b.st, b.d_probs, ws_off, jb, level + 1, slot + n, 0);
      }
      slot += n;
    }
  }
}

// the look-ahead's position in its two-stream pipeline: entered (the internal streams wait for the caller's) and which
// scratch copy the next block's chain writes
struct LaState { LookAhead* la = nullptr; bool on = false; int par = 0; };
// back to the caller's stream
void la_leave(const QrBatch& b, LaState& s) {
  if (!s.on) return;
  hipEventRecord(s.la->e_out_a, s.la->sa); hipEventRecord(s.la->e_out_b, s.la->sb);
  hipStreamWaitEvent(b.st, s.la->e_out_a, 0); hipStreamWaitEvent(b.st, s.la->e_out_b, 0);
  s.on = false;
}
// block jb in the look-ahead form (the comment at LookAhead): its panel chain on stream B, part 2 of its trailing update
// on stream A beside the next block's chain, part 1 (the next block's panel tiles) on B behind part 2 of the previous block
void qr_lookahead_block(const QrBatch& b, LaState& s, int jb, int ntile4) {
  LookAhead* la = s.la;
  const bool first = !s.on;
  if (first) {
    hipEventRecord(la->e_in, b.st);
    hipStreamWaitEvent(la->sa, la->e_in, 0); hipStreamWaitEvent(la->sb, la->e_in, 0);
    s.on = true; s.par = 0;
  }
  const v2::AuxLay& L = b.lay[s.par];
  panel_chain(b, la->sb, L, jb, 4, true, LA_RESERVED);
  hipEventRecord(la->e_b, la->sb);
  // part 2 beside the next block's chain
  hipStreamWaitEvent(la->sa, la->e_b, 0);
  trail_coop(b, la->sa, L, jb, 4, ntile4);
  hipEventRecord(la->e_a[s.par], la->sa);
  // part 1 (the next block's panel tiles) behind part 2 of the previous block.  (Tiles 1..3 on a second stream of the
  // same CUs beside the next panel's column steps: measured no faster, 41.9 against 41.0 ms.)
  if (!first) hipStreamWaitEvent(la->sb, la->e_a[s.par ^ 1], 0);
  launch_trail(4, dim3(16, b.nchunk, b.P), la->sb, b, L, jb, 0, 0, 0);
  s.par ^= 1;
}
// block jb with one launch sequence after the other on the caller's stream: the panel chain, then the trailing update
void qr_panel_block(const QrBatch& b, int jb, int npmax, bool tall, int ntile4, int coop_max_wgs) {
  const v2::AuxLay& lay = b.lay[0];
  panel_chain(b, b.st, lay, jb, npmax, tall, coop_max_wgs);
  const int c0min = jb + 16;     // a problem with one panel left starts its trailing tiles here
  const int ntile_max = b.cols_max > c0min ? (b.cols_max - c0min + 15) / 16 : 0;
  if (ntile_max == 0) return;
  // Many problems: one wave per tile pair over all rows (fused, the tuned wg::qr_trail4); few: tiles x row chunks
  // over the grid in two launches.  Problems with fewer than four panels left always take the second form.
  const bool fused = npmax == 4 && ntile4 > 0 && (int64_t)b.P * ((ntile4 + 1) / 2) >= 1024 && !b.env.no_fused_trail;
  if (fused) {
    if (b.env.trail_nt == 1) hipLaunchKernelGGL(v2::k_trail4f<1>, dim3((ntile4 + 3) / 4, b.P), dim3(256), 0, b.st, b.d_probs, lay, jb);
    else hipLaunchKernelGGL(v2::k_trail4f<2>, dim3((ntile4 + 7) / 8, b.P), dim3(256), 0, b.st, b.d_probs, lay, jb);
  }
  // few large problems: (16 tiles x row chunk) workgroups with the panels shared through LDS, two launches
  const bool coop = !fused && npmax == 4 && ntile4 > 0 && !b.env.no_coop_trail;
  if (coop) trail_coop(b, b.st, lay, jb, 0, ntile4);
  if ((!fused && !coop) || b.kmax_min - jb < 64)
    launch_trail(npmax, dim3((ntile_max + 3) / 4, b.nchunk, b.P), b.st, b, lay, jb, 0, 4, (fused || coop) ? 1 : 0);
}

// Launch sequence of one R-only QR over a batch whose dimensions `dims` are known on the host.
// d_probs: device array of v2::QrProb (same order as dims).  force_tall: column-step panels even when they would fit.
// aux2: every problem's scratch holds TWO AuxLay copies (auxd doubles apart) - required for the look-ahead.
// path: which form ran (self tests): 1 communication-avoiding, 2 look-ahead, 0 launch per panel.
// (Tried and measured slower, round 3: cutting a many-problem batch into four groups that run this sequence on their own
// streams, so that one group's panel chain runs beside another's trailing update - 6400 x 1600 x 16: 49.3 against 28.3 ms,
// 7200 x 900 x 128: 82.5 against 73.6 ms; without disjoint CUs the chains' VALU-bound kernels share SIMDs with MFMA streams
// and run at a third of their speed, profiles/r03_dp_pipe_probe.txt.)
int qr_batch(hipStream_t st, const v2::QrProb* d_probs, const std::vector<QrDims>& dims, const v2::AuxLay& lay, bool force_tall,
             const QrEnv& env, int* coop_err = nullptr, int coop_max_wgs = 128, int64_t aux2 = 0, int ncu = 256, int* path = nullptr) {
  if (path) *path = 0;
  if (dims.empty()) return 0;
  QrBatch b{st, d_probs, (int)dims.size(), 0, {lay, v2::second_auxlay(lay, aux2)}, coop_err, env, 0, 1 << 30, 0, 0};
  for (const QrDims& d : dims) {
    b.kmax_max = std::max(b.kmax_max, d.kmax); b.kmax_min = std::min(b.kmax_min, d.kmax);
    b.rows32_max = std::max(b.rows32_max, r32i(d.rows)); b.cols_max = std::max(b.cols_max, d.cols);
  }
  b.nchunk = (b.rows32_max + v2::CH - 1) / v2::CH;
  if (b.nchunk > lay.nchunk) return -1;
  if (set_func_attrs_once() != hipSuccess) return -2;
  if (qr_tree_applies(b, dims, force_tall, aux2)) {
    qr_tree(b, ncu);
    if (path) *path = 1;
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  // look-ahead: uniform large problems only (every block has four full panels for every problem, the cooperative panel
  // kernel fits the reserved CUs, the trailing matrix is wide enough to have a part 2); the streams are created on first
  // use - only when a batch has the look-ahead's shape, after the tree form declined
  const bool la_cand = aux2 > 0 && coop_err && !env.no_coop_panel && !env.no_coop_trail &&
                       (int64_t)b.nchunk * b.P <= LA_MAX_WGS && b.rows32_max > 2 * v2::CH && b.kmax_min == b.kmax_max;
  LaState las;
  las.la = la_cand ? lookahead_streams() : nullptr;
  for (int jb = 0; jb < b.kmax_max; jb += 64) {
    const int npmax = std::min(4, (b.kmax_max - jb + 15) / 16);
    // register panels / one workgroup per problem for the in-block updates while the rows below the diagonal fit
    const bool tall = force_tall || b.rows32_max - jb > v2::CH;
    const int ntile4 = b.cols_max > jb + 64 ? (b.cols_max - jb - 64 + 15) / 16 : 0;
    if (las.la && tall && npmax == 4 && b.kmax_min - jb >= 64 && ntile4 > 8 && b.rows32_max - jb > 2 * v2::CH) {
      if (path) *path = 2;
      qr_lookahead_block(b, las, jb, ntile4);
      continue;
    }
    la_leave(b, las);
    qr_panel_block(b, jb, npmax, tall, ntile4, coop_max_wgs);
  }
  la_leave(b, las);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

void v2_device_acquire(int dev) {
  if (dev < 0 || dev >= MAX_DEV) return;
  std::lock_guard<std::mutex> lk(g_dev[dev].mu);
  g_dev[dev].refs++;
}
void v2_device_release(int dev) {
  if (dev < 0 || dev >= MAX_DEV) return;
  DeviceShared& D = g_dev[dev];
  std::lock_guard<std::mutex> lk(D.mu);
  if (D.refs > 0 && --D.refs == 0) { int cur = 0; (void)hipGetDevice(&cur); (void)hipSetDevice(dev); la_destroy(D.la); (void)hipSetDevice(cur); }
}
namespace { struct DeviceHold { int dev; explicit DeviceHold(int d) : dev(d) { v2_device_acquire(d); } ~DeviceHold() { v2_device_release(dev); } }; }

// ================================================================================================
// self test: nprob independent rows x cols matrices through the batched QR; R[p] = [kmax x cols] (ld kmax)
// ================================================================================================
static int st2_fail(const char* what, hipError_t e) { g_create_error = std::string(what) + ": " + hipGetErrorString(e); return MPBP_EHIP; }
#define ST2CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return st2_fail(#call, e_); } while (0)

namespace {
// device allocations and an event pair of a self test, released on every return
struct DevMem {
  std::vector<void*> ptrs;
  ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> hipError_t alloc(T** p, size_t count) {
    const hipError_t e = hipMalloc((void**)p, sizeof(T) * count);
    if (e == hipSuccess) ptrs.push_back(*p);
    return e;
  }
};
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
};
int device_cus(int device) {
  hipDeviceProp_t pr;
  return hipGetDeviceProperties(&pr, device) == hipSuccess ? pr.multiProcessorCount : 256;
}
// column-major A [rows x cols] into the zero-filled Y with leading dimension ld
void pad_matrix(const double* A, int rows, int cols, int ld, std::vector<double>& Y) {
  std::fill(Y.begin(), Y.end(), 0.0);
  for (int j = 0; j < cols; j++) for (int i = 0; i < rows; i++) Y[i + (size_t)ld * j] = A[i + (size_t)rows * j];
}
// the upper triangle of the first kmax rows of Y (leading dimension ld) -> R [kmax x cols], zeros below the diagonal
void read_upper(const std::vector<double>& Y, int ld, int kmax, int cols, double* R) {
  for (int j = 0; j < cols; j++) for (int i = 0; i < kmax; i++) R[i + (size_t)kmax * j] = (j >= i) ? Y[i + (size_t)ld * j] : 0.0;
}
}  // namespace

extern "C" int mpbp_selftest_qr_batched(int32_t device, int32_t rows, int32_t cols, int32_t nprob, int32_t force_tall,
                                        const double* A, double* R, double* ms_out) {
  ST2CHK(hipSetDevice(device));
  if (rows < 1 || cols < 1 || nprob < 1) { g_create_error = "bad shape"; return MPBP_EINVAL; }
  DeviceHold hold(device);
  const QrEnv env = read_qr_env();
  const int ld = r32i(rows), c16 = r16i(cols) + 16, kmax = std::min(rows, cols);
  const size_t per = (size_t)ld * c16;
  const int nchunk = (ld + v2::CH - 1) / v2::CH, ntile = c16 / 16;
  const v2::AuxLay lay = v2::make_auxlay(nchunk, ntile);
  const size_t auxd = (size_t)v2::auxlay_doubles(nchunk, ntile);
  DevMem mem; EventPair ev;
  double *dY = nullptr, *dAux = nullptr; v2::QrProb* dP = nullptr; int* dErr = nullptr;
  ST2CHK(mem.alloc(&dY, per * nprob));
  ST2CHK(mem.alloc(&dAux, 2 * auxd * nprob));          // two scratch copies per problem: look-ahead of qr_batch
  ST2CHK(mem.alloc(&dP, nprob));
  ST2CHK(hipMemset(dAux, 0, sizeof(double) * 2 * auxd * nprob));
  std::vector<double> Y(per);
  std::vector<v2::QrProb> hp(nprob);
  const std::vector<QrDims> dims(nprob, QrDims{rows, cols, kmax});
  for (int p = 0; p < nprob; p++) {
    pad_matrix(A + (size_t)p * rows * cols, rows, cols, ld, Y);
    ST2CHK(hipMemcpy(dY + per * p, Y.data(), sizeof(double) * per, hipMemcpyHostToDevice));
    hp[p] = v2::QrProb{dY + per * p, dAux + 2 * auxd * p, ld, rows, cols, kmax};
  }
  ST2CHK(hipMemcpy(dP, hp.data(), sizeof(v2::QrProb) * nprob, hipMemcpyHostToDevice));
  (void)lookahead_streams();          // a context creates them once in its life: keep that out of the timed region
  ST2CHK(ev.create());
  hipEventRecord(ev.e0, 0);
  ST2CHK(mem.alloc(&dErr, 1));
  ST2CHK(hipMemset(dErr, 0, sizeof(int)));
  const int ncu = device_cus(device);
  const int rc = qr_batch(0, dP, dims, lay, force_tall != 0, env, dErr, 128, (int64_t)auxd, ncu);
  hipEventRecord(ev.e1, 0);
  ST2CHK(hipDeviceSynchronize());
  if (rc != 0) { g_create_error = "qr_batch launch failed"; return MPBP_EHIP; }
  int herr = 0;
  ST2CHK(hipMemcpy(&herr, dErr, sizeof(int), hipMemcpyDeviceToHost));
  if (herr) { g_create_error = "cooperative panel: an arrival counter timed out"; return MPBP_EHIP; }
  float ms = 0; hipEventElapsedTime(&ms, ev.e0, ev.e1);
  if (ms_out) *ms_out = ms;
  for (int p = 0; p < nprob; p++) {
    ST2CHK(hipMemcpy(Y.data(), dY + per * p, sizeof(double) * per, hipMemcpyDeviceToHost));
    read_upper(Y, ld, kmax, cols, R + (size_t)p * kmax * cols);
  }
  return MPBP_OK;
}

// self test: ONE matrix per call, the calls of a sequence sharing one scratch sized for the largest (as the time steps of a
// gauge sweep do): rows[s] x cols, A / R concatenated; path[s] = the form qr_batch took (1 communication-avoiding, 2
// look-ahead, 0 launch per panel).  Pins that a communication-avoiding call leaves the arrival counters of a later
// look-ahead call intact (round-3 advisor: its node slots used to run over the second scratch copy's header).
extern "C" int mpbp_selftest_qr_batched_seq(int32_t device, int32_t nshape, const int32_t* rows, int32_t cols, const double* A, double* R, int32_t* path) {
  ST2CHK(hipSetDevice(device));
  if (nshape < 1 || cols < 1 || !rows) { g_create_error = "bad shape"; return MPBP_EINVAL; }
  DeviceHold hold(device);
  const QrEnv env = read_qr_env();
  int rmax = 0;
  for (int s = 0; s < nshape; s++) { if (rows[s] < 1) { g_create_error = "bad shape"; return MPBP_EINVAL; } rmax = std::max(rmax, rows[s]); }
  const int ldmax = r32i(rmax), c16 = r16i(cols) + 16;
  const int nchunk = (ldmax + v2::CH - 1) / v2::CH, ntile = c16 / 16;
  const v2::AuxLay lay = v2::make_auxlay(nchunk, ntile);
  const size_t auxd = (size_t)v2::auxlay_doubles(nchunk, ntile);
  DevMem mem;
  double *dY = nullptr, *dAux = nullptr; v2::QrProb* dP = nullptr; int* dErr = nullptr;
  ST2CHK(mem.alloc(&dY, (size_t)ldmax * c16));
  ST2CHK(mem.alloc(&dAux, 2 * auxd));
  ST2CHK(mem.alloc(&dP, 1));
  ST2CHK(mem.alloc(&dErr, 1));
  ST2CHK(hipMemset(dAux, 0, sizeof(double) * 2 * auxd));                 // once, as v2_gauge_sweep does
  ST2CHK(hipMemset(dErr, 0, sizeof(int)));
  const int ncu = device_cus(device);
  std::vector<double> Y((size_t)ldmax * c16);
  size_t aoff = 0, roff = 0;
  int rc_all = MPBP_OK;
  for (int s = 0; s < nshape && rc_all == MPBP_OK; s++) {
    const int m = rows[s], ld = r32i(m), kmax = std::min(m, cols);
    pad_matrix(A + aoff, m, cols, ld, Y);
    ST2CHK(hipMemcpy(dY, Y.data(), sizeof(double) * (size_t)ld * c16, hipMemcpyHostToDevice));
    const v2::QrProb hp{dY, dAux, ld, m, cols, kmax};
    ST2CHK(hipMemcpy(dP, &hp, sizeof hp, hipMemcpyHostToDevice));
    int pth = 0;
    const int rc = qr_batch(0, dP, {QrDims{m, cols, kmax}}, lay, false, env, dErr, ncu * 3 / 4, (int64_t)auxd, ncu, &pth);
    ST2CHK(hipDeviceSynchronize());
    if (path) path[s] = pth;
    int herr = 0; ST2CHK(hipMemcpy(&herr, dErr, sizeof(int), hipMemcpyDeviceToHost));
    if (rc != 0) { g_create_error = "qr_batch launch failed"; rc_all = MPBP_EHIP; }
    else if (herr) { g_create_error = "cooperative panel: an arrival counter timed out"; rc_all = MPBP_EHIP; }
    ST2CHK(hipMemcpy(Y.data(), dY, sizeof(double) * (size_t)ld * c16, hipMemcpyDeviceToHost));
    read_upper(Y, ld, kmax, cols, R + roff);
    aoff += (size_t)m * cols; roff += (size_t)kmax * cols;
  }
  return rc_all;
}

// self test of the multi-launch Jacobi (k_jac_round / k_jac_check): A [m x n] (ld m|1 inside) -> column norms after
// convergence (= singular values, unsorted) and the number of sweeps (-1: not converged within maxsweeps)
static int jacobi_selftest(int32_t device, int32_t m, int32_t n, const double* A, double* sigma, int32_t maxsweeps, int32_t* sweeps, bool block) {
  ST2CHK(hipSetDevice(device));
  if (m < 1 || n < 1 || n > m || m > 1024) { g_create_error = "need 1 <= n <= m <= 1024"; return MPBP_EINVAL; }
  const int ldJ = v2::jac_ld(m);
  std::vector<double> JA((size_t)ldJ * n);
  pad_matrix(A, m, n, ldJ, JA);
  double fro2 = 0.0;
  for (int c = 0; c < n; c++) for (int r = 0; r < m; r++) { const double v = A[r + (size_t)m * c]; fro2 += v * v; }
  DevMem mem;
  double *dJA = nullptr, *dscal = nullptr; v2::SvdDesc* dd = nullptr; int32_t* dact = nullptr;
  ST2CHK(mem.alloc(&dJA, JA.size())); ST2CHK(mem.alloc(&dscal, 64)); ST2CHK(mem.alloc(&dd, 1)); ST2CHK(mem.alloc(&dact, n));
  ST2CHK(hipMemcpy(dJA, JA.data(), sizeof(double) * JA.size(), hipMemcpyHostToDevice));
  double hs[8] = {0, 0, 0, fro2, 0, 0, (n < 2) ? 1.0 : 0.0, (double)n};
  ST2CHK(hipMemcpy(dscal, hs, sizeof hs, hipMemcpyHostToDevice));
  { std::vector<int32_t> ha(n); for (int i = 0; i < n; i++) ha[i] = i; ST2CHK(hipMemcpy(dact, ha.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
  v2::SvdDesc D{};
  D.JA = dJA; D.Rr = m; D.r1 = n; D.scal = dscal; D.act = dact;
  ST2CHK(hipMemcpy(dd, &D, sizeof D, hipMemcpyHostToDevice));
  if (block) {
    ST2CHK(set_func_attrs_once());
    const int nb = jac_block_nb(m, n);
    if (nb < 2) { g_create_error = "factor too tall for an LDS-resident block pair"; return MPBP_EUNSUPPORTED; }
    const int nblk = (n + nb - 1) / nb, ne = (nblk + 1) & ~1;
    const size_t jlds = sizeof(double) * ((size_t)(m | 1) * 2 * nb + 32);
    for (int sw = 0; sw < maxsweeps; sw++) {
      for (int r = 0; r < std::max(1, ne - 1); r++) hipLaunchKernelGGL(v2::k_jac_block, dim3(ne / 2, 1), dim3(512), jlds, 0, (const v2::SvdDesc*)dd, r, nb);
      hipLaunchKernelGGL(v2::k_jac_deflate, dim3(1), dim3(512), 0, 0, (const v2::SvdDesc*)dd);
    }
  } else {
    const int ne = (n + 1) & ~1;
    for (int sw = 0; sw < maxsweeps; sw++) {
      for (int r = 0; r < ne - 1; r++) hipLaunchKernelGGL(v2::k_jac_round, dim3((ne / 2 + 15) / 16, 1), dim3(512), 0, 0, (const v2::SvdDesc*)dd, r);
      hipLaunchKernelGGL(v2::k_jac_check, dim3(1), dim3(64), 0, 0, (const v2::SvdDesc*)dd, 1);
    }
  }
  ST2CHK(hipDeviceSynchronize());
  ST2CHK(hipGetLastError());
  ST2CHK(hipMemcpy(JA.data(), dJA, sizeof(double) * JA.size(), hipMemcpyDeviceToHost));
  ST2CHK(hipMemcpy(hs, dscal, sizeof hs, hipMemcpyDeviceToHost));
  for (int c = 0; c < n; c++) { double s = 0; for (int r = 0; r < m; r++) s += JA[r + (size_t)ldJ * c] * JA[r + (size_t)ldJ * c]; sigma[c] = sqrt(s); }
  *sweeps = hs[6] != 0.0 ? (int)hs[5] : -1;
  return MPBP_OK;
}
extern "C" int mpbp_selftest_jacobi_grid(int32_t device, int32_t m, int32_t n, const double* A, double* sigma, int32_t maxsweeps, int32_t* sweeps) {
  return jacobi_selftest(device, m, n, A, sigma, maxsweeps, sweeps, false);
}
// the two-level (block) Jacobi of the truncating sweep (v2::k_jac_block) on one m x n matrix, same outputs
extern "C" int mpbp_selftest_jacobi_block(int32_t device, int32_t m, int32_t n, const double* A, double* sigma, int32_t maxsweeps, int32_t* sweeps) {
  return jacobi_selftest(device, m, n, A, sigma, maxsweeps, sweeps, true);
}

// ================================================================================================
// the batched gauge sweep
// ================================================================================================
namespace {

struct StepDims { int a, an, b, bn, r1, rows, cols, kmax; };

struct ProbPlan {
  std::vector<StepDims> st;        // [L]; entries 1 .. L-1 used
  std::vector<int64_t> lfoff;      // [L+1]
  std::vector<int32_t> rdim;       // [L+1]
  int64_t lf_doubles = 0, y_doubles = 0, z_doubles = 0, e_doubles = 0;
  int rows32_max = 0, cols_max = 0;
  // truncating sweep (planned when the kept ranks follow from the dimensions)
  std::vector<int> kc;             // [L+1]: left bond of output core t
  int64_t c_doubles = 0, t1_doubles = 0, nt_doubles = 0, mt_doubles = 0, ja_doubles = 0, u_doubles = 0;
  int rr_max = 0;
};

inline v2::Map2 lin(int64_t s) { return v2::Map2{1 << 30, s, 0}; }


}  // namespace

int v2_gather_bonds(mpbp_ctx* c, const EngProb* probs, int n, std::vector<int32_t>& hb) {
  const int L = c->L;
  hipStream_t st = c->stream;
  hb.resize((size_t)n * 2 * (L + 1));
  if (n <= 0) return MPBP_OK;
  std::vector<v2::BondSrc> src(n);
  for (int i = 0; i < n; i++) src[i] = v2::BondSrc{probs[i].bond1, probs[i].bond2};
  const size_t bsrc = (sizeof(v2::BondSrc) * n + 255) & ~size_t(255), bout = sizeof(int32_t) * hb.size();
  int rc = ensure_arena(c, c->v2arena, bsrc + bout + 4096);
  if (rc != MPBP_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->v2arena.base, src.data(), sizeof(v2::BondSrc) * n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(v2::k_gather_bonds, dim3(n), dim3(64), 0, st, (const v2::BondSrc*)c->v2arena.base, (int32_t*)(c->v2arena.base + bsrc), L);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(hb.data(), c->v2arena.base + bsrc, bout, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MPBP_OK;
}


// MPBP_V2_TIMING=1: device time of the batched sweeps by section (HIP events on the stream, read once per call) on stderr
struct V2Timing {
  bool on; hipStream_t st; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[4]; hipEvent_t cur;
  explicit V2Timing(hipStream_t s) : on(getenv("MPBP_V2_TIMING") != nullptr), st(s), cur(nullptr) {}
  void begin() { if (on) { (void)hipEventCreate(&cur); (void)hipEventRecord(cur, st); } }
  void end(int cat) { if (on) { hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, st); ev[cat].push_back({cur, e}); } }
  void report(int P, int L) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    const char* nm[4] = {"sweep 1 (assembly + QR + Lf)", "sweep 2 contractions + scaling", "sweep 2 QR of M_t", "sweep 2 Jacobi + truncation"};
    for (int k = 0; k < 4; k++) {
      double ms = 0;
      for (auto& pr : ev[k]) { float x = 0; (void)hipEventElapsedTime(&x, pr.first, pr.second); ms += x; (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
      if (!ev[k].empty()) fprintf(stderr, "[v2 timing] P=%d L=%d  %-34s %10.1f ms\n", P, L, nm[k], ms);
    }
  }
};

namespace {

// ---------------------------------------------------------------- planning (host only)
// dimensions of every time step of one problem; they follow from the bond tables b1, b2 of its operands
ProbPlan plan_problem(const EngProb& P, const int32_t* b1, const int32_t* b2, int L, const mpbp_trunc* trunc2) {
  ProbPlan pp;
  pp.st.resize(L); pp.lfoff.assign(L + 1, 0); pp.rdim.assign(L + 1, 1);
  int64_t off = 0;
  pp.lfoff[L] = off; off += 4;                      // Lf_L = [1]
  for (int t = L - 1; t >= 1; t--) {
    StepDims d;
    d.a = b1[t]; d.an = b1[t + 1]; d.b = b2[t]; d.bn = b2[t + 1];
    d.r1 = pp.rdim[t + 1];
    d.rows = d.r1 * P.ny * P.q; d.cols = d.a * d.b; d.kmax = std::min(d.rows, d.cols);
    pp.rdim[t] = d.kmax;
    pp.st[t] = d;
    pp.lfoff[t] = off; off += ((int64_t)d.kmax * d.cols + 3) & ~int64_t(3);
    pp.y_doubles = std::max<int64_t>(pp.y_doubles, (int64_t)r32i(d.rows) * (r16i(d.cols) + 16));
    pp.z_doubles = std::max<int64_t>(pp.z_doubles, (int64_t)d.a * P.ny1 * P.q * d.r1 * d.bn);
    pp.e_doubles = std::max<int64_t>(pp.e_doubles, (int64_t)P.q * d.b * P.ny * d.bn * P.ny1);
    pp.rows32_max = std::max(pp.rows32_max, r32i(d.rows)); pp.cols_max = std::max(pp.cols_max, d.cols);
  }
  pp.e_doubles = std::max<int64_t>(pp.e_doubles, (int64_t)P.q * b2[0] * P.ny * b2[1] * P.ny1);
  pp.lf_doubles = off;
  if (!trunc2) return pp;
  // sweep 2, t = 0 .. L-1: kc_0 = 1, Rr = kc ny q, kept rank min(Rr, r_{t+1}, mprime, cap_out)
  pp.kc.assign(L + 1, 1);
  for (int t = 0; t < L; t++) {
    const int a = b1[t], an = b1[t + 1], b = b2[t], bn = b2[t + 1];
    const int kc = pp.kc[t], Rr = kc * P.ny * P.q;
    const int64_t Bn = (int64_t)an * bn;
    pp.rr_max = std::max(pp.rr_max, Rr);
    pp.c_doubles = std::max<int64_t>(pp.c_doubles, (int64_t)kc * a * b);
    pp.t1_doubles = std::max<int64_t>(pp.t1_doubles, (int64_t)kc * b * an * P.ny1 * P.q);
    pp.nt_doubles = std::max<int64_t>(pp.nt_doubles, (int64_t)Rr * Bn);
    if (t == L - 1) break;
    const int r1 = pp.rdim[t + 1];
    int kp = std::min(std::min(Rr, r1), trunc2->mprime);
    kp = std::max(1, std::min(kp, (int)P.cap_out));
    pp.kc[t + 1] = kp;
    pp.c_doubles = std::max<int64_t>(pp.c_doubles, (int64_t)kp * Bn);
    pp.mt_doubles = std::max<int64_t>(pp.mt_doubles, (int64_t)r32i(r1) * (r16i(Rr) + 16));
    pp.ja_doubles = std::max<int64_t>(pp.ja_doubles, (int64_t)v2::jac_ld(Rr) * std::min(r1, Rr));
    pp.u_doubles = std::max<int64_t>(pp.u_doubles, (int64_t)Rr * kp);
    pp.rows32_max = std::max(pp.rows32_max, r32i(r1)); pp.cols_max = std::max(pp.cols_max, Rr);
  }
  return pp;
}

inline size_t al(int64_t doubles) { return ((size_t)doubles * 8 + 255) & ~size_t(255); }
// The longest prefix of the problems whose buffers and descriptors fit `budget` bytes (at least one problem; the caller
// compares bytes with the budget), and the scratch geometry of that batch.  `bytes` is an upper estimate of what carve and
// the uploads take.  P decides the QR and Jacobi forms of every step, so this formula is part of the results on the
// large configurations.
struct BatchFit { int P = 0; size_t bytes = 0; int nchunk = 1, ntile = 1; };
BatchFit fit_batch(const std::vector<ProbPlan>& plan, int L, int q, bool trunc2, size_t budget) {
  BatchFit f;
  for (int i = 0; i < (int)plan.size(); i++) {
    const int nc = std::max(f.nchunk, (plan[i].rows32_max + v2::CH - 1) / v2::CH), nt = std::max(f.ntile, r16i(plan[i].cols_max) / 16 + 1);
    // aux is sized by the batch maxima: recompute the total when they grow
    size_t tot = 0;
    for (int k = 0; k <= i; k++)
      tot += al(plan[k].y_doubles) + al(plan[k].z_doubles) + al(plan[k].e_doubles) + al(plan[k].lf_doubles) + al(2 * v2::auxlay_doubles(nc, nt)) +
             (((size_t)(L + 1) * 12 + 255) & ~size_t(255)) +
             (trunc2 ? 2 * al(plan[k].c_doubles) + al(plan[k].t1_doubles) + al(plan[k].nt_doubles) + al(plan[k].mt_doubles) + al(plan[k].ja_doubles) + al(plan[k].u_doubles) + 512 + (((size_t)plan[k].rr_max * 4 + 255) & ~size_t(255)) + 256 : 0);
    const size_t desc = (size_t)(i + 1) * L * (sizeof(v2::QrProb) * 2 + sizeof(v2::GemmDesc) * (4 + 2 * q) + sizeof(v2::EDesc) + sizeof(v2::LfDesc) + sizeof(v2::ScaleDesc) + sizeof(v2::SvdDesc)) + 65536;
    if (i > 0 && tot + desc > budget) break;
    f.P = i + 1; f.bytes = tot + desc; f.nchunk = nc; f.ntile = nt;
  }
  return f;
}

// ---------------------------------------------------------------- the arena: buffers and descriptor uploads
struct Carver {
  char* base; size_t cap, used = 0;
  char* take(size_t b) { char* p = base + used; used += (b + 255) & ~size_t(255); return p; }
  bool over() const { return used > cap; }
};
struct Bufs { double *Y, *Z, *E, *aux, *lf; int64_t* lfoff; int32_t* rdim; double *C0, *C1, *T1, *Nt, *Mt, *JA, *U, *scal; int32_t* act; };
std::vector<Bufs> carve(Carver& ar, const std::vector<ProbPlan>& plan, int P, int L, int64_t auxd, bool trunc2) {
  std::vector<Bufs> bf(P);
  for (int i = 0; i < P; i++) {
    Bufs& B = bf[i];
    const ProbPlan& pl = plan[i];
    B.Y = (double*)ar.take(al(pl.y_doubles)); B.Z = (double*)ar.take(al(pl.z_doubles)); B.E = (double*)ar.take(al(pl.e_doubles));
    B.aux = (double*)ar.take(al(2 * auxd));          // two scratch copies: look-ahead of qr_batch
    B.lf = (double*)ar.take(al(pl.lf_doubles));
    char* tb = ar.take((size_t)(L + 1) * 12);
    B.lfoff = (int64_t*)tb; B.rdim = (int32_t*)(tb + (size_t)(L + 1) * 8);
    if (!trunc2) continue;
    B.C0 = (double*)ar.take(al(pl.c_doubles)); B.C1 = (double*)ar.take(al(pl.c_doubles));
    B.T1 = (double*)ar.take(al(pl.t1_doubles)); B.Nt = (double*)ar.take(al(pl.nt_doubles));
    B.Mt = (double*)ar.take(al(pl.mt_doubles)); B.JA = (double*)ar.take(al(pl.ja_doubles));
    B.U = (double*)ar.take(al(pl.u_doubles)); B.scal = (double*)ar.take(512);     // [0] max slot, [1] log c
    B.act = (int32_t*)ar.take(sizeof(int32_t) * (size_t)std::max(1, pl.rr_max));
  }
  return bf;
}
// Takes room for the host vector behind what is carved and starts its copy.  The vector must stay alive until the stream
// has been synchronised.  Past the end of the arena nothing is copied: the caller checks Carver::over() after its uploads.
template <class T> hipError_t upload(Carver& ar, hipStream_t st, const std::vector<T>& h, const T** d) {
  *d = (const T*)ar.take(sizeof(T) * h.size());
  return ar.over() ? hipSuccess : hipMemcpyAsync((void*)*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st);
}

// what the stages of one batch share
struct Batch {
  mpbp_ctx* c; const EngProb* probs; const int32_t* hb; const std::vector<ProbPlan>& plan; const std::vector<Bufs>& bf;
  int P, L, q; v2::AuxLay lay; int64_t auxd; int* coop_err; const QrEnv& qenv; const JacobiEnv& jenv;
  const int32_t* b1(int i) const { return hb + (size_t)i * 2 * (L + 1); }
  const int32_t* b2(int i) const { return b1(i) + (L + 1); }
};

// ---------------------------------------------------------------- the six contractions as k_gemm descriptors
// (O[oro(m) + oco(n)] = sum_k S[sro(m) + sco(k)] X[xro(k) + xco(n)]; cores are stored [a][an][y1 x], factors [r][a b])
// sweep 1:  Z[(a,y1,x), (r,bn)] = sum_an A1_t[a, an, (y1,x)] Lf_{t+1}[r, (an,bn)]
v2::GemmDesc gemm_z(const EngProb& Pr, const Bufs& B, const ProbPlan& pl, int t, int q) {
  const StepDims& d = pl.st[t];
  v2::GemmDesc g{};
  g.S = Pr.A1 + (int64_t)t * Pr.stride1; g.X = B.lf + pl.lfoff[t + 1]; g.O = B.Z;
  g.M = d.a * Pr.ny1 * q; g.N = d.r1 * d.bn; g.K = d.an;
  g.sro = v2::Map2{d.a, 1, (int64_t)d.a * d.an}; g.sco = lin(d.a);
  g.xro = lin(d.r1); g.xco = v2::Map2{d.r1, 1, (int64_t)d.r1 * d.an};
  g.oro = lin((int64_t)d.r1 * d.bn); g.oco = lin(1);
  return g;
}
// sweep 1:  Y_t[(r,y,x), (a,b)] = sum_(bn,y1) E_x[(b,y), (bn,y1)] Z[(a,y1,x), (r,bn)], one product per x
v2::GemmDesc gemm_y(const EngProb& Pr, const Bufs& B, const ProbPlan& pl, int t, int xi) {
  const StepDims& d = pl.st[t];
  const int M2 = d.b * Pr.ny, K2 = d.bn * Pr.ny1, ldY = r32i(d.rows);
  const int64_t zld = (int64_t)d.r1 * d.bn;
  v2::GemmDesc h{};
  h.S = B.E + (int64_t)xi * M2 * K2; h.X = B.Z + zld * d.a * Pr.ny1 * xi; h.O = B.Y + (int64_t)d.r1 * Pr.ny * xi;
  h.M = M2; h.N = d.r1 * d.a; h.K = K2;
  h.sro = lin(1); h.sco = lin(M2);
  h.xro = v2::Map2{d.bn, d.r1, zld * d.a}; h.xco = v2::Map2{d.r1, 1, zld};
  h.oro = v2::Map2{d.b, (int64_t)ldY * d.a, d.r1}; h.oco = v2::Map2{d.r1, 1, ldY};
  return h;
}
// dimensions of step t of the truncating sweep
struct Step2Dims { int a, an, b, bn, kc, Rr; int64_t Bn, tld; };
Step2Dims step2_dims(const EngProb& Pr, const ProbPlan& pl, const int32_t* b1, const int32_t* b2, int t, int q) {
  const int kc = pl.kc[t];
  return Step2Dims{b1[t], b1[t + 1], b2[t], b2[t + 1], kc, kc * Pr.ny * q, (int64_t)b1[t + 1] * b2[t + 1], (int64_t)kc * b2[t]};
}
// sweep 2:  T1[(an,y1,x), (kc,b)] = sum_a A1_t[a, an, (y1,x)] C_t[kc, (a,b)]
v2::GemmDesc gemm_t1(const EngProb& Pr, const Bufs& B, const Step2Dims& d, int t, int q) {
  v2::GemmDesc g{};
  g.S = Pr.A1 + (int64_t)t * Pr.stride1; g.X = (t & 1) ? B.C1 : B.C0; g.O = B.T1;
  g.M = d.an * Pr.ny1 * q; g.N = d.kc * d.b; g.K = d.a;
  g.sro = v2::Map2{d.an, d.a, (int64_t)d.a * d.an}; g.sco = lin(1);
  g.xro = lin(d.kc); g.xco = v2::Map2{d.kc, 1, (int64_t)d.kc * d.a};
  g.oro = lin(d.tld); g.oco = lin(1);
  return g;
}
// sweep 2:  N_t[(kc,y,x), (an,bn)] = sum_(b,y1) E_x[(b,y), (bn,y1)] T1[(an,y1,x), (kc,b)], one product per x
v2::GemmDesc gemm_nt(const EngProb& Pr, const Bufs& B, const Step2Dims& d, int xi) {
  const int M2 = d.b * Pr.ny, K2 = d.bn * Pr.ny1;
  v2::GemmDesc h{};
  h.S = B.E + (int64_t)xi * M2 * K2; h.X = B.T1 + d.tld * d.an * Pr.ny1 * xi; h.O = B.Nt + (int64_t)d.kc * Pr.ny * xi;
  h.M = d.bn * Pr.ny; h.N = d.kc * d.an; h.K = d.b * Pr.ny1;
  h.sro = v2::Map2{d.bn, M2, d.b}; h.sco = v2::Map2{d.b, 1, (int64_t)M2 * d.bn};
  h.xro = v2::Map2{d.b, d.kc, d.tld * d.an}; h.xco = v2::Map2{d.kc, 1, d.tld};
  h.oro = v2::Map2{d.bn, (int64_t)d.Rr * d.an, d.kc}; h.oco = v2::Map2{d.kc, 1, d.Rr};
  return h;
}
// sweep 2:  M_t^T[r, (kc,y,x)] = sum_(an,bn) Lf_{t+1}[r, (an,bn)] N_t[(kc,y,x), (an,bn)], leading dimension ldM
v2::GemmDesc gemm_mt(const Bufs& B, const ProbPlan& pl, const Step2Dims& d, int t) {
  const int r1 = pl.rdim[t + 1];
  v2::GemmDesc m{};
  m.S = B.Nt; m.X = B.lf + pl.lfoff[t + 1]; m.O = B.Mt;
  m.M = d.Rr; m.N = r1; m.K = (int)d.Bn;
  m.sro = lin(1); m.sco = lin(d.Rr); m.xro = lin(r1); m.xco = lin(1); m.oro = lin(r32i(r1)); m.oco = lin(1);
  return m;
}
// sweep 2:  C_{t+1}[kp, (an,bn)] = sum_(kc,y,x) U[(kc,y,x), kp] N_t[(kc,y,x), (an,bn)]   (the carry U^T N_t)
v2::GemmDesc gemm_carry(const Bufs& B, const Step2Dims& d, int t, int kp) {
  v2::GemmDesc cr{};
  cr.S = B.U; cr.X = B.Nt; cr.O = (t & 1) ? B.C0 : B.C1;
  cr.M = kp; cr.N = (int)d.Bn; cr.K = d.Rr;
  cr.sro = lin(d.Rr); cr.sco = lin(1); cr.xro = lin(1); cr.xco = lin(d.Rr); cr.oro = lin(1); cr.oco = lin(kp);
  return cr;
}

// ---------------------------------------------------------------- sweep 1: descriptors, per-step launch sizes, launches
// host descriptors of every time step ([t][problem]) and where they went on the device; lives until the stream has been
// synchronised behind the uploads
struct Sweep1Descs {
  std::vector<v2::QrProb> hq; std::vector<v2::GemmDesc> hg1, hg2; std::vector<v2::EDesc> he; std::vector<v2::LfDesc> hl;
  std::vector<v2::SetOne> hone; std::vector<char> htab;
  const v2::QrProb* dq; const v2::GemmDesc *dg1, *dg2; const v2::EDesc* de; const v2::LfDesc* dl; const v2::SetOne* done;
};
void build_sweep1_descs(const Batch& b, Sweep1Descs& D) {
  const int P = b.P, L = b.L, q = b.q;
  D.hq.resize((size_t)P * L); D.hg1.resize((size_t)P * L); D.hg2.resize((size_t)P * L * q); D.he.resize((size_t)P * L); D.hl.resize((size_t)P * L);
  D.hone.resize(P); D.htab.resize((size_t)P * (L + 1) * 12);
  for (int i = 0; i < P; i++) {
    const EngProb& Pr = b.probs[i];
    const ProbPlan& pl = b.plan[i];
    const Bufs& B = b.bf[i];
    memcpy(D.htab.data() + (size_t)i * (L + 1) * 12, pl.lfoff.data(), (size_t)(L + 1) * 8);
    memcpy(D.htab.data() + (size_t)i * (L + 1) * 12 + (size_t)(L + 1) * 8, pl.rdim.data(), (size_t)(L + 1) * 4);
    D.hone[i].p = B.lf + pl.lfoff[L];
    const int32_t* b2 = b.b2(i);
    for (int t = 0; t < L; t++)      // the coupling table of every time step (the truncating sweep starts at t = 0)
      D.he[(size_t)t * P + i] = v2::EDesc{Pr.A2 + (int64_t)t * Pr.stride2, Pr.pyy + (int64_t)t * Pr.pyy_tstride, B.E, (int)b2[t], (int)b2[t + 1], Pr.ny, Pr.ny1, Pr.ny2, q};
    for (int t = 1; t < L; t++) {
      const StepDims& d = pl.st[t];
      const size_t k = (size_t)t * P + i;
      D.hq[k] = v2::QrProb{B.Y, B.aux, r32i(d.rows), d.rows, d.cols, d.kmax};
      D.hl[k].Lf = B.lf + pl.lfoff[t];
      D.hg1[k] = gemm_z(Pr, B, pl, t, q);
      for (int xi = 0; xi < q; xi++) D.hg2[k * q + xi] = gemm_y(Pr, B, pl, t, xi);
    }
  }
}
// grid sizes of one time step: maxima over the problems of the batch
struct StepGrid {
  std::vector<QrDims> dims;                            // the step's QR
  int maxN1 = 0, maxN2 = 0, maxNm = 0, maxNc = 0, rows32m = 0, colsm = 0, rrt = 1, k2t = 1;
  int64_t maxE = 0, maxNt = 0;
};
StepGrid sweep1_grid(const Batch& b, int t) {
  StepGrid g;
  g.dims.resize(b.P);
  for (int i = 0; i < b.P; i++) {
    const StepDims& d = b.plan[i].st[t];
    g.dims[i] = QrDims{d.rows, d.cols, d.kmax};
    g.maxN1 = std::max(g.maxN1, d.r1 * d.bn); g.maxN2 = std::max(g.maxN2, d.r1 * d.a);
    g.maxE = std::max<int64_t>(g.maxE, (int64_t)b.q * d.b * b.probs[i].ny * d.bn * b.probs[i].ny1);
    g.rows32m = std::max(g.rows32m, r32i(d.rows)); g.colsm = std::max(g.colsm, d.cols);
  }
  return g;
}
int qr_step(const Batch& b, const v2::QrProb* dq, const StepGrid& g) {
  mpbp_ctx* c = b.c;
  if (qr_batch(c->stream, dq, g.dims, b.lay, b.jenv.force_tall, b.qenv, b.coop_err, c->num_cu * 3 / 4, b.auxd, c->num_cu) != 0)
    return c->fail(MPBP_EHIP, "batched QR launch failed: %s", hipGetErrorString(hipGetLastError()));
  return MPBP_OK;
}
// step t of sweep 1: E, Z, Y_t, its QR, Lf_t
int run_sweep1_step(const Batch& b, const Sweep1Descs& D, int t) {
  const StepGrid g = sweep1_grid(b, t);
  const int P = b.P, q = b.q;
  hipStream_t st = b.c->stream;
  const size_t o = (size_t)t * P;
  hipLaunchKernelGGL(v2::k_build_E, dim3((unsigned)std::min<int64_t>(64, (g.maxE + 255) / 256), P), dim3(256), 0, st, D.de + o);
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxN1 + 127) / 128), P), dim3(512), 0, st, D.dg1 + o);
  hipLaunchKernelGGL(v2::k_zero_pads, dim3(std::min(256, std::max(1, g.rows32m / 8)), P), dim3(256), 0, st, D.dq + o, b.lay);
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxN2 + 127) / 128), P * q), dim3(512), 0, st, D.dg2 + o * q);
  const int rc = qr_step(b, D.dq + o, g);
  if (rc != MPBP_OK) return rc;
  const int gw = std::min(256, std::max(1, (g.colsm + 3) / 4));
  hipLaunchKernelGGL(v2::k_maxabs, dim3(gw, P), dim3(256), 0, st, D.dq + o, b.lay);
  hipLaunchKernelGGL(v2::k_lf_write, dim3(gw, P), dim3(256), 0, st, D.dq + o, D.dl + o, b.lay);
  return MPBP_OK;
}
// uploads the descriptors (D: the caller's, the truncating sweep reads its coupling-table descriptors again), zeroes the
// counters, then the time steps L-1 .. 1
int run_sweep1(const Batch& b, Sweep1Descs& D, Carver& ar, V2Timing& tm) {
  mpbp_ctx* c = b.c;
  hipStream_t st = c->stream;
  const int P = b.P, L = b.L;
  build_sweep1_descs(b, D);
  HIPCHK(c, upload(ar, st, D.hq, &D.dq)); HIPCHK(c, upload(ar, st, D.hg1, &D.dg1)); HIPCHK(c, upload(ar, st, D.hg2, &D.dg2));
  HIPCHK(c, upload(ar, st, D.he, &D.de)); HIPCHK(c, upload(ar, st, D.hl, &D.dl)); HIPCHK(c, upload(ar, st, D.hone, &D.done));
  if (!ar.over())
    for (int i = 0; i < P; i++)
      HIPCHK(c, hipMemcpyAsync(b.bf[i].lfoff, D.htab.data() + (size_t)i * (L + 1) * 12, (size_t)(L + 1) * 12, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));     // D's vectors outlive their copies
  if (ar.over()) return c->fail(MPBP_ENOMEM, "internal: gauge-sweep arena accounting (%zu > %zu)", ar.used, ar.cap);
  hipLaunchKernelGGL(v2::k_set_one, dim3((P + 63) / 64), dim3(64), 0, st, D.done, P);
  for (int i = 0; i < P; i++)                                                         // counters, T/S of both scratch copies (the two headers)
    HIPCHK(c, hipMemsetAsync(b.bf[i].aux, 0, sizeof(double) * (size_t)(2 * v2::AUX_HDR), st));
  HIPCHK(c, hipMemsetAsync(c->d_counter + 8, 0, sizeof(int), st));
  tm.begin();
  for (int t = L - 1; t >= 1; t--) {
    const int rc = run_sweep1_step(b, D, t);
    if (rc != MPBP_OK) return rc;
  }
  tm.end(0);
  HIPCHK(c, hipGetLastError());
  return MPBP_OK;
}

// ---------------------------------------------------------------- sweep 2: the Jacobi forms
// Form of the Jacobi (MPBP_JACOBI_FORM = wg | grid | block forces one):
//   wg     one workgroup per problem (wg::jacobi_rsv inside k_svd_trunc): the default for factors below 320 columns and for
//          batches of more than 32 problems - with a CU per problem the chip is full, and no pair is met twice per sweep;
//   block  two-level (v2::k_jac_block + k_jac_deflate): block pairs LDS resident, blocks / 2 workgroups per problem, one
//          launch per round of the block tournament: the default for factors of >= 320 columns in batches of <= 32
//          problems - the hub levels of configs[2], where one CU per problem rotates 400 ... 780-column factors out of HBM
//          while the rest of the chip idles.  Round 4, one configs[2] node block on one box (profiles/r04_jacobi_forms.txt):
//          Jacobi + truncation in the batches of 2 - 4 problems 7.5 -> 2.4 s (the grid form's regime in round 3), of 5 - 32
//          problems 9.8 -> 6.0 s, sweep 219.8 -> 212.8 s.  Below 320 columns it does not pay: configs[3] (160 columns) 89.1
//          against 91.7 s, configs[4] (256 columns, <= 3 problems) 26.0 / 27.0 against 24.8 / 26.5 s per iteration.  It NEEDS
//          the deflation of wg::jacobi_rsv (BP factors: numerical rank ~2/3, most columns null after two sweeps): without
//          it the same configs[2] block took 351 s.  And only while one workgroup per problem leaves most of the chip idle:
//          with a CU per problem for a whole batch the one-workgroup form is at full occupancy and does fewer rotations.
//   grid   one launch per tournament round over the grid (k_jac_round, no deflation; round 3's form for >= 384 columns and
//          <= 4 problems): superseded by block, kept selectable and tested.  Only for a handful of problems: with many, one
//          workgroup per problem keeps every CU busy and the 659 launches per sweep (at 660 columns) only add latency
//          (configs[2] shard: 498 s with the grid form on every level, 327 s without).
// rrt, k2t: the most rows and columns of any problem's transposed triangular factor; nb: columns per block of the block form
struct JacobiChoice { JacobiForm form; int nb; };
JacobiChoice choose_jacobi(const JacobiEnv& e, int rrt, int k2t, int P) {
  int nb = 0;
  if ((e.form == JAC_AUTO || e.form == JAC_BLOCK) && k2t >= (e.form == JAC_BLOCK ? 96 : e.block_min) && rrt <= 1024 && P <= e.block_maxp) nb = jac_block_nb(rrt, k2t);
  if (nb) return JacobiChoice{JAC_BLOCK, nb};
  const bool grid = e.form == JAC_GRID && rrt <= 1024 && k2t >= e.grid_min && P <= e.grid_maxp;
  return JacobiChoice{grid ? JAC_GRID : JAC_WG, 0};
}
// what the three forms take: the step's SVD descriptors, the LDS of k_svd_trunc, the step's largest factor
struct JacobiStep { const v2::SvdDesc* dsv; size_t svd_lds; int rrt, k2t; };
void svd_trunc(const Batch& b, const JacobiStep& j, int phase) {      // 0 all of it, 1 before / 2 after a multi-launch Jacobi
  hipLaunchKernelGGL(v2::k_svd_trunc, dim3(b.P), dim3(512), j.svd_lds, b.c->stream, j.dsv, b.c->d_stats, phase);
}
int jacobi_wg(const Batch& b, const JacobiStep& j) {
  svd_trunc(b, j, 0);
  return MPBP_OK;
}
int jacobi_block(const Batch& b, const JacobiStep& j, int nb) {
  mpbp_ctx* c = b.c;
  hipStream_t st = c->stream;
  svd_trunc(b, j, 1);
  const size_t jlds = sizeof(double) * ((size_t)(j.rrt | 1) * 2 * nb + 32);
  int nact = j.k2t;                  // the most active columns of any unconverged problem (read back after every sweep:
  for (int sweep = 0; sweep < b.jenv.grid_sweeps; sweep++) {      //  the later sweeps run over a fraction of the blocks)
    const int nblk = (nact + nb - 1) / nb, ne = (nblk + 1) & ~1;
    for (int r = 0; r < std::max(1, ne - 1); r++)
      hipLaunchKernelGGL(v2::k_jac_block, dim3(ne / 2, b.P), dim3(512), jlds, st, j.dsv, r, nb);
    hipLaunchKernelGGL(v2::k_jac_deflate, dim3(b.P), dim3(512), 0, st, j.dsv);
    int pending[2] = {0, 0};
    hipLaunchKernelGGL(v2::k_jac_pending2, dim3(1), dim3(256), 0, st, j.dsv, b.P, c->d_counter + 9);
    HIPCHK(c, hipMemcpyAsync(pending, c->d_counter + 9, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (pending[0] == 0) break;
    nact = std::max(2, std::min(nact, pending[1]));
  }
  svd_trunc(b, j, 2);
  return MPBP_OK;
}
int jacobi_grid(const Batch& b, const JacobiStep& j) {
  mpbp_ctx* c = b.c;
  hipStream_t st = c->stream;
  svd_trunc(b, j, 1);
  const int ne = (j.k2t + 1) & ~1;
  // up to 60 sweeps, as the one-workgroup form allows; the host looks at the convergence flags every 4 sweeps
  // (one 4-byte copy) so that the ~6-10 sweeps of the usual case are not followed by 50 sweeps of empty launches
  for (int sweep = 0; sweep < b.jenv.grid_sweeps; sweep++) {
    for (int r = 0; r < ne - 1; r++)
      hipLaunchKernelGGL(v2::k_jac_round, dim3((ne / 2 + 15) / 16, b.P), dim3(512), 0, st, j.dsv, r);
    hipLaunchKernelGGL(v2::k_jac_check, dim3((b.P + 63) / 64), dim3(64), 0, st, j.dsv, b.P);
    if ((sweep & 3) != 3) continue;
    int pending = 0;
    hipLaunchKernelGGL(v2::k_jac_pending, dim3(1), dim3(256), 0, st, j.dsv, b.P, c->d_counter + 9);
    HIPCHK(c, hipMemcpyAsync(&pending, c->d_counter + 9, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (pending == 0) break;
  }
  svd_trunc(b, j, 2);
  return MPBP_OK;
}

// ---------------------------------------------------------------- sweep 2: descriptors, per-step launch sizes, launches
struct Sweep2Descs {
  std::vector<v2::GemmDesc> gn1, gn2, gmt, gcr; std::vector<v2::QrProb> q2; std::vector<v2::ScaleDesc> sc; std::vector<v2::SvdDesc> sv;
  std::vector<v2::LastDesc> last; std::vector<v2::NormDesc> nrm; std::vector<v2::SetOne> one;
  const v2::GemmDesc *dn1, *dn2, *dmt, *dcr; const v2::QrProb* dq2; const v2::ScaleDesc* dsc; const v2::SvdDesc* dsv;
  const v2::LastDesc* dlast; const v2::NormDesc* dnrm; const v2::SetOne* done;
};
void build_sweep2_descs(const Batch& b, const mpbp_trunc& trunc, Sweep2Descs& D) {
  const int P = b.P, L = b.L, q = b.q;
  D.gn1.resize((size_t)P * L); D.gn2.resize((size_t)P * L * q); D.gmt.resize((size_t)P * L); D.gcr.resize((size_t)P * L);
  D.q2.resize((size_t)P * L); D.sc.resize((size_t)P * L); D.sv.resize((size_t)P * L);
  D.last.resize(P); D.nrm.resize(P); D.one.resize(P);
  for (int i = 0; i < P; i++) {
    const EngProb& Pr = b.probs[i];
    const ProbPlan& pl = b.plan[i];
    const Bufs& B = b.bf[i];
    D.one[i].p = B.C0;
    D.last[i] = v2::LastDesc{B.Nt, Pr.out + (int64_t)(L - 1) * Pr.ostride, Pr.obond, pl.kc[L - 1] * Pr.ny * q, L};
    D.nrm[i] = v2::NormDesc{Pr.out, Pr.obond, Pr.ostride, Pr.logz1, Pr.logz2, B.scal + 2, Pr.ologz, Pr.ny * q, L};
    for (int t = 0; t < L; t++) {
      const size_t k = (size_t)t * P + i;
      const Step2Dims d = step2_dims(Pr, pl, b.b1(i), b.b2(i), t, q);
      D.gn1[k] = gemm_t1(Pr, B, d, t, q);
      for (int xi = 0; xi < q; xi++) D.gn2[k * q + xi] = gemm_nt(Pr, B, d, xi);
      D.sc[k] = v2::ScaleDesc{B.Nt, (int64_t)d.Rr * d.Bn, B.scal + (t & 1), B.scal + 2, B.scal + ((t + 1) & 1)};
      if (t == L - 1) continue;
      const int r1 = pl.rdim[t + 1], kp = pl.kc[t + 1], ldM = r32i(r1);
      D.gmt[k] = gemm_mt(B, pl, d, t);
      D.q2[k] = v2::QrProb{B.Mt, B.aux, ldM, r1, d.Rr, std::min(r1, d.Rr)};
      D.sv[k] = v2::SvdDesc{B.Mt, B.JA, B.U, Pr.out + (int64_t)t * Pr.ostride, Pr.obond,
                            ldM, r1, d.Rr, d.kc, kp, t, L, trunc.kind, trunc.mprime, Pr.cap_out, B.scal, B.act};
      D.gcr[k] = gemm_carry(B, d, t, kp);
    }
  }
}
StepGrid sweep2_grid(const Batch& b, int t) {
  StepGrid g;
  g.dims.resize(b.P);
  for (int i = 0; i < b.P; i++) {
    const EngProb& Pr = b.probs[i];
    const Step2Dims d = step2_dims(Pr, b.plan[i], b.b1(i), b.b2(i), t, b.q);
    g.maxN1 = std::max(g.maxN1, d.kc * d.b); g.maxN2 = std::max(g.maxN2, d.kc * d.an);
    g.maxE = std::max<int64_t>(g.maxE, (int64_t)b.q * d.b * Pr.ny * d.bn * Pr.ny1);
    g.maxNt = std::max<int64_t>(g.maxNt, (int64_t)d.Rr * d.an * d.bn);
    g.maxNc = std::max(g.maxNc, d.an * d.bn);
    if (t == b.L - 1) continue;
    const int r1 = b.plan[i].rdim[t + 1];
    g.dims[i] = QrDims{r1, d.Rr, std::min(r1, d.Rr)};
    g.maxNm = std::max(g.maxNm, r1); g.rows32m = std::max(g.rows32m, r32i(r1));
    g.rrt = std::max(g.rrt, d.Rr); g.k2t = std::max(g.k2t, std::min(d.Rr, r1));
  }
  return g;
}
// step t of sweep 2: E, N_t and its rescale; then (t < L-1) M_t^T, its QR, the SVD of the triangular factor - inside one
// workgroup, or for factors of several hundred columns as rounds of rotations over the grid (choose_jacobi) - and the
// carry; the last step writes the last core instead
int run_sweep2_step(const Batch& b, const v2::EDesc* de, const Sweep2Descs& D, int t, size_t svd_lds, V2Timing& tm) {
  const StepGrid g = sweep2_grid(b, t);
  mpbp_ctx* c = b.c;
  hipStream_t st = c->stream;
  const int P = b.P, q = b.q;
  const size_t o = (size_t)t * P;
  tm.begin();
  hipLaunchKernelGGL(v2::k_build_E, dim3((unsigned)std::min<int64_t>(64, (g.maxE + 255) / 256), P), dim3(256), 0, st, de + o);
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxN1 + 127) / 128), P), dim3(512), 0, st, D.dn1 + o);
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxN2 + 127) / 128), P * q), dim3(512), 0, st, D.dn2 + o * q);
  const unsigned gsc = (unsigned)std::min<int64_t>(256, (g.maxNt + 2047) / 2048);
  hipLaunchKernelGGL(v2::k_absmax, dim3(gsc, P), dim3(256), 0, st, D.dsc + o);
  hipLaunchKernelGGL(v2::k_scale, dim3(gsc, P), dim3(256), 0, st, D.dsc + o, c->d_stats);
  if (t == b.L - 1) {
    hipLaunchKernelGGL(v2::k_lastcore, dim3(P), dim3(256), 0, st, D.dlast);
    tm.end(1);
    return MPBP_OK;
  }
  hipLaunchKernelGGL(v2::k_zero_pads, dim3(std::min(256, std::max(1, g.rows32m / 8)), P), dim3(256), 0, st, D.dq2 + o, b.lay);
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxNm + 127) / 128), P), dim3(512), 0, st, D.dmt + o);
  tm.end(1); tm.begin();
  int rc = qr_step(b, D.dq2 + o, g);
  if (rc != MPBP_OK) return rc;
  tm.end(2); tm.begin();
  const JacobiChoice jc = choose_jacobi(b.jenv, g.rrt, g.k2t, P);
  const JacobiStep js{D.dsv + o, svd_lds, g.rrt, g.k2t};
  rc = jc.form == JAC_BLOCK ? jacobi_block(b, js, jc.nb) : jc.form == JAC_GRID ? jacobi_grid(b, js) : jacobi_wg(b, js);
  if (rc != MPBP_OK) return rc;
  tm.end(3); tm.begin();
  hipLaunchKernelGGL(v2::k_gemm, dim3(std::min(1024, (g.maxNc + 127) / 128), P), dim3(512), 0, st, D.dcr + o);
  tm.end(1);
  return MPBP_OK;
}
// the truncating sweep on the grid: uploads its descriptors, then the time steps 0 .. L-1 and the normalisation
int run_sweep2(const Batch& b, const v2::EDesc* de, const mpbp_trunc& trunc, Carver& ar, V2Timing& tm) {
  mpbp_ctx* c = b.c;
  hipStream_t st = c->stream;
  const int P = b.P, L = b.L;
  Sweep2Descs D;
  build_sweep2_descs(b, trunc, D);
  HIPCHK(c, upload(ar, st, D.gn1, &D.dn1)); HIPCHK(c, upload(ar, st, D.gn2, &D.dn2)); HIPCHK(c, upload(ar, st, D.gmt, &D.dmt));
  HIPCHK(c, upload(ar, st, D.gcr, &D.dcr)); HIPCHK(c, upload(ar, st, D.q2, &D.dq2)); HIPCHK(c, upload(ar, st, D.sc, &D.dsc));
  HIPCHK(c, upload(ar, st, D.sv, &D.dsv)); HIPCHK(c, upload(ar, st, D.last, &D.dlast)); HIPCHK(c, upload(ar, st, D.nrm, &D.dnrm));
  HIPCHK(c, upload(ar, st, D.one, &D.done));
  for (int i = 0; i < P; i++) HIPCHK(c, hipMemsetAsync(b.bf[i].scal, 0, 64, st));
  HIPCHK(c, hipStreamSynchronize(st));     // D's vectors outlive their copies
  if (ar.over()) return c->fail(MPBP_ENOMEM, "internal: gauge-sweep arena accounting (%zu > %zu)", ar.used, ar.cap);
  hipLaunchKernelGGL(v2::k_set_one, dim3((P + 63) / 64), dim3(64), 0, st, D.done, P);
  // the LDS of k_svd_trunc follows from the batch, so its limit is set per call (the other kernels: set_func_attrs_once)
  int rrm = 1;
  for (int i = 0; i < P; i++) rrm = std::max(rrm, b.plan[i].rr_max);
  const size_t svd_lds = sizeof(double) * (32 + (size_t)rrm + (rrm + 1) / 2 + 4);
  HIPCHK(c, hipFuncSetAttribute((const void*)v2::k_svd_trunc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)svd_lds));
  for (int t = 0; t < L; t++) {
    const int rc = run_sweep2_step(b, de, D, t, svd_lds, tm);
    if (rc != MPBP_OK) return rc;
  }
  hipLaunchKernelGGL(v2::k_normalize_out, dim3(P), dim3(256), 0, st, D.dnrm, c->d_stats);
  HIPCHK(c, hipGetLastError());
  return MPBP_OK;
}

}  // namespace

int v2_gauge_sweep(mpbp_ctx* c, EngProb* probs, int n, const int32_t* hb, const mpbp_trunc* trunc2, int* n_done, int* did_sweep2) {
  *did_sweep2 = 0;
  *n_done = 0;
  if (n <= 0) return MPBP_OK;
  const int L = c->L, q = probs[0].q;
  for (int i = 0; i < n; i++)
    if (probs[i].mirror) return c->fail(MPBP_EINVAL, "internal: mirrored problem in the batched gauge sweep");
  const QrEnv qenv = read_qr_env();
  const JacobiEnv jenv = read_jacobi_env();
  // ---- dimensions of every time step, and how many problems fit
  std::vector<ProbPlan> plan(n);
  for (int i = 0; i < n; i++) plan[i] = plan_problem(probs[i], hb + (size_t)i * 2 * (L + 1), hb + (size_t)i * 2 * (L + 1) + (L + 1), L, trunc2);
  size_t freeb = 0, totb = 0;
  hipMemGetInfo(&freeb, &totb);
  const size_t budget = (size_t)((double)(freeb + c->v2arena.cap) * 0.80);
  const BatchFit fit = fit_batch(plan, L, c->q, trunc2 != nullptr, budget);
  if (fit.bytes > budget) return c->fail(MPBP_ENOMEM, "batched gauge sweep: one problem needs %zu MiB, %zu MiB available", fit.bytes >> 20, budget >> 20);
  const int P = fit.P;
  for (int i = 0; i < P; i++)
    if (probs[i].q != q) return c->fail(MPBP_EINVAL, "internal: mixed q in one batch");
  const int rc = ensure_arena(c, c->v2arena, fit.bytes + 65536);
  if (rc != MPBP_OK) return rc;
  // ---- the arena: buffers first, each sweep's descriptors behind them
  Carver ar{c->v2arena.base, c->v2arena.cap};
  const int64_t auxd = v2::auxlay_doubles(fit.nchunk, fit.ntile);
  const std::vector<Bufs> bf = carve(ar, plan, P, L, auxd, trunc2 != nullptr);
  // cooperative panels only while no launch of this context has timed out (launch_grid repeats a failed batch without them)
  int* coop_err = c->no_coop_panel ? nullptr : c->d_counter + 8;
  const Batch b{c, probs, hb, plan, bf, P, L, q, v2::make_auxlay(fit.nchunk, fit.ntile), auxd, coop_err, qenv, jenv};
  V2Timing tm(c->stream);
  Sweep1Descs s1;
  int rc1 = run_sweep1(b, s1, ar, tm);
  if (rc1 != MPBP_OK) return rc1;
  for (int i = 0; i < P; i++) { probs[i].lf = bf[i].lf; probs[i].lfoff = bf[i].lfoff; probs[i].rdim = bf[i].rdim; }
  *n_done = P;
  if (trunc2) {
    rc1 = run_sweep2(b, s1.de, *trunc2, ar, tm);
    if (rc1 != MPBP_OK) return rc1;
    *did_sweep2 = 1;
  }
  tm.report(P, L);
  return MPBP_OK;
}
