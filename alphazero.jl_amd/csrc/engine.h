// engine.h -- what the translation units of libazhip.so share: the engine record, error / launch macros, the
// profiling helpers, the entry points of net.hip (network launches) used by azhip.hip, memory.hip and train.hip, the records of
// the replay memories and their data set (with the frame all three data-set creators share), the check that makes a device
// current (use_device) and the scoped owner of a call's device scratch (Scratch).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <unordered_set>

#include "../../include/az_numerics.h"
#include "../../include/azhip.h"
#include "env.h"
#include "games.h"
#include "net_layout.h"
#include "phase_books.h"
#include "resnet.h"
#include "resnet16.h"
#include "resnet16b.h"
#include "ring_books.h"
#include "simplenet.h"
#include "tower_choice.h"
#include "tree.h"

// ------------------------------------------------------------------------------- errors
int fail(int code, const char* fmt, ...);   // sets az_last_error() (thread-local), returns code; defined in azhip.hip
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t _e = (x);                                                                            \
    if (_e != hipSuccess) return fail(AZ_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define AZCHK(x)            \
  do {                      \
    int _s = (x);           \
    if (_s != AZ_OK) return _s; \
  } while (0)


#define DISPATCH_GAME(gid, ...)                                   \
  switch (gid) {                                                  \
    case AZ_GAME_CONNECT_FOUR: { using Gm = ConnectFour; __VA_ARGS__; break; } \
    case AZ_GAME_TICTACTOE: { using Gm = TicTacToe; __VA_ARGS__; break; }      \
    case AZ_GAME_MANCALA: { using Gm = Mancala; __VA_ARGS__; break; }          \
    default: return fail(AZ_ERR_BAD_ARG, "unknown game id %d", (int)(gid));    \
  }

// The four NETWORK geometries: the three device twins and the 9x9x4 plane geometry, which has no rules (games.h Go9Planes).  For code
// that reads tensors only -- the optimiser step's MFMA kernels (train.hip); the tree, the replay memory and everything else that
// calls a game's rules stay on DISPATCH_GAME.
#define DISPATCH_GEOMETRY(gid, ...)                               \
  switch (gid) {                                                  \
    case AZ_GAME_CONNECT_FOUR: { using Gm = ConnectFour; __VA_ARGS__; break; } \
    case AZ_GAME_TICTACTOE: { using Gm = TicTacToe; __VA_ARGS__; break; }      \
    case AZ_GAME_MANCALA: { using Gm = Mancala; __VA_ARGS__; break; }          \
    case AZ_GAME_GO9_PLANES: { using Gm = Go9Planes; __VA_ARGS__; break; }     \
    default: return fail(AZ_ERR_BAD_ARG, "unknown game id %d", (int)(gid));    \
  }

struct GameInfo { int A, APAD, W, H, C, P, max_plies, node_bytes; };
inline bool game_info(int gid, GameInfo* gi) {
  switch (gid) {
    case AZ_GAME_CONNECT_FOUR: *gi = {ConnectFour::A, ConnectFour::APAD, ConnectFour::W, ConnectFour::H, ConnectFour::C, ConnectFour::P, ConnectFour::MAX_PLIES, NodeL<ConnectFour>::BYTES}; return true;
    case AZ_GAME_TICTACTOE: *gi = {TicTacToe::A, TicTacToe::APAD, TicTacToe::W, TicTacToe::H, TicTacToe::C, TicTacToe::P, TicTacToe::MAX_PLIES, NodeL<TicTacToe>::BYTES}; return true;
    case AZ_GAME_MANCALA: *gi = {Mancala::A, Mancala::APAD, Mancala::W, Mancala::H, Mancala::C, Mancala::P, Mancala::MAX_PLIES, NodeL<Mancala>::BYTES}; return true;
    case AZ_GAME_GO9_PLANES: *gi = {Go9Planes::A, Go9Planes::APAD, Go9Planes::W, Go9Planes::H, Go9Planes::C, Go9Planes::P, Go9Planes::MAX_PLIES, 64}; return true;   // network-only geometry: no tree
  }
  return false;
}

// where each piece of a ResNet engine's parameter blob lies (net_layout.h)
inline NetLayout net_layout(const GameInfo& gi, const az_engine_cfg& c) {
  return NetLayout(NetShape{gi.C, gi.P, gi.A, gi.APAD, c.num_blocks, c.num_filters, c.num_policy_head_filters, c.num_value_head_filters});
}

// where each piece of a SimpleNet engine's parameter blob lies (net_layout.h)
inline SimpleLayout simple_layout(const GameInfo& gi, const az_simplenet_hp& h) {
  return SimpleLayout(SimpleShape{gi.C * gi.P, gi.A, h.width, h.depth_common, h.depth_phead, h.depth_vhead, h.use_batch_norm});
}
// "the engine's oracle is its network": what the search, the arena, the replay memory, the learning status, the trainer, the broadcast
// and the host-stepped trees ask before they use az_net_* machinery
inline bool oracle_is_net(const az_engine_cfg& c) { return c.oracle == AZ_ORACLE_RESNET || c.oracle == AZ_ORACLE_SIMPLENET; }

// ------------------------------------------------------------------------------- engine
// AZ_MAX_GROUPS: tree.h
// Everything that describes ONE self-play phase; the default value means "no phase".  az_selfplay_begin assigns a fresh record, so no
// member carries over; az_selfplay_end leaves it (statistics, aborted ids, uncollected and device-resident games are read after it).
// Buffers, streams, events and what explores outside a phase use as well (group_active, pending, wave_par) are az_engine's.
struct Phase {
  bool running = false;
  bool fr_on = false;                // free-running (az_engine_cfg.lock_step = 0): the device hands out game ids and moves by itself
  bool host_moves = true;            // the caller wants the move records on the host (false: az_selfplay_run with out->moves == NULL)
  GameIds ids;                       // phase_books.h; a free-running phase's device counter (FRState::next_game) is mirrored at every look
  int games_done = 0, wave_in_move = 0, active_slots = 0;
  int fr_k = 0, fr_kbg = 0, fr_round_waves = 0;  // simulations a slot may select per wave launch / per background launch (DView::run_k); waves between two looks of the host
  int fr_prev_done = 0, fr_since_round = 0, fr_given_up = 0; long long fr_prev_recs = 0;
  int fr_look_waves = 0, fr_since_look = 0;      // mapped-on-demand pool: waves between two looks at the node counts (fr_look, azhip.hip; <= fr_round_waves) / since the last one
  std::vector<az_game_rec> q_games;  // finished, not yet collected (az_selfplay_collect) ...
  std::vector<az_move_rec> q_moves;  // ... and their move records where they come to the host
  std::vector<az_game_rec> dev_games;   // a bounded phase's finished games, in finishing order ...
  std::vector<int64_t> dev_off; int64_t dev_n = 0;   // ... the offset of each one's first move record in d_phase; records in use
  std::vector<int32_t> aborted_ids;  // games retired because their slot ran out of nodes / move records (az_selfplay_aborted)
  az_selfplay_stats stats = {};
  std::chrono::steady_clock::time_point t_begin;
};
struct ProfRec { hipEvent_t a = nullptr, b = nullptr; int cls = 0; };
// Every member has its initial value here: az_engine_create builds the record step by step and az_engine_destroy takes it apart at
// any point in between.  DView / DParams go to the kernels by value and stay trivially copyable (memset by the step that fills them).
struct az_engine {
  az_engine_cfg cfg = {};
  az_simplenet_hp shp = {};         // cfg.oracle == AZ_ORACLE_SIMPLENET: the network's hyperparameters (the ResNet fields of cfg are unused)
  GameInfo gi = {};
  EnvCreate env;                 // the AZHIP_* overrides, read when az_engine_create constructs this record (env.h): forced kernels, experiments, test knobs
  int device = 0;
  hipStream_t stream = nullptr;
  DView v = {};                     // global view over all G slots (start / move / hooks)
  DParams p = {};
  // slot groups: num_workers / batch_size interleaved half-batches, each with its own stream, so the
  // tree kernels of one group run under the network of another (the device form of the reference's
  // num_workers = 2 x batch_size, games/connect-four/params.jl:18-19)
  int ngroups = 0;
  DView gv[AZ_MAX_GROUPS] = {};
  hipStream_t gs[AZ_MAX_GROUPS] = {};      // tree-kernel stream of the group (high priority when ngroups > 1)
  hipStream_t gt[AZ_MAX_GROUPS] = {};      // network stream of the group
  hipEvent_t ev_tree[AZ_MAX_GROUPS] = {}, ev_net[AZ_MAX_GROUPS] = {};
  float* g_hfeat[AZ_MAX_GROUPS] = {};
  // k_tower16s (split tower, 128 filters): publish areas per feature buffer (slot g = group g, AZ_MAX_GROUPS = d_hfeat), launch epoch
  unsigned long long* xch[AZ_MAX_GROUPS + 1] = {}; unsigned long long xch_epoch = 0;   // (first epoch: env.xch_epoch0)
  // (r4) a split tower whose exchange gives up degrades instead of failing the phase (azhip.hip recover_split)
  int* d_xerr = nullptr; int* d_skipped = nullptr;   // [AZ_MAX_GROUPS + 1] exchange words, [..][2] counters of idle k_tree launches (DView::xerr / skipped)
  int* h_needy = nullptr; int* d_needy = nullptr;    // [AZ_MAX_GROUPS] host-mapped: slots each group's previous wave launch left to the background search (tree.h DView::needy_host)
  int* h_nleaf = nullptr; int* d_nleaf = nullptr;    // [AZ_MAX_GROUPS] host-mapped: network batch of each group's previous wave (k_tree writes, choose_wave_tower's estimate reads); -1 = nothing reported yet
  int* h_xflag = nullptr; int* d_xflag = nullptr;    // host-mapped word the kernel sets when an exchange gives up; looked at before every launch
  bool split_off = false;        // the split is disabled for this engine after the first time
  long long xch_launches = 0;    // split launches so far (env.xch_fail_at: the n-th loses a partner)
  int split_registered = 0;      // streams this engine contributes to the device's count of split-tower users
  std::vector<void*> allocs;
  size_t alloc_bytes = 0;          // device bytes behind `allocs` (az_engine_device_bytes)
  std::vector<void*> host_allocs;  // hipHostMalloc'ed: the host-mapped words (halloc_mapped) and the pinned staging buffers (halloc_pinned)
  // node pool mapped on demand (azhip.hip "node pool"): a virtual range of rows x G chunks of 2 MB; chunk (row r, slot s) is
  // backed when slot s is about to need it.  vm_rows = 0: plain hipMalloc pool.
  char* vm_base = nullptr; size_t vm_bytes = 0, vm_chunk = 0; int vm_rows = 0, vm_chunk_nodes = 0;
  std::vector<hipMemGenericAllocationHandle_t> vm_handles; std::vector<char*> vm_at;
  std::vector<int> h_slot_cap, h_node_count; int* d_slot_cap = nullptr; int* d_node_count = nullptr; size_t vm_budget = 0, vm_mapped = 0;
  // (r5) the side records of a mapped-on-demand pool follow the node chunks: a second virtual range of rows x G pieces of
  // vm_chunk_nodes x 32 B, backed by 2 MB granules (vmk_granule[i] = granule i is mapped); vmk_base = NULL: dense [G][cap][4] array
  char* vmk_base = nullptr; size_t vmk_bytes = 0, vmk_piece = 0; std::vector<uint8_t> vmk_granule;
  // (r5 experiments) env.tree_sort: slot order of k_tree by the depth of the last explore! (d_perm [G] order | [G] keys,
  // d_perm_prev [G][2] totals at the last move step)
  int* d_perm = nullptr; long long* d_perm_prev = nullptr;
  // evaluation cache (tree.h ECEnt): one table per engine = per network; az_net_set_params empties it
  ECEnt* d_ec = nullptr; size_t ec_entries = 0; uint32_t ec_seq = 0; int* d_ec_claim = nullptr; float* d_Phit = nullptr; float* d_Vhit = nullptr;
  size_t stat_words = 0; std::vector<long long> h_stat;   // per-workgroup statistics accumulators of k_tree (DView::stat), summed on request
  std::vector<void*> net_allocs;   // device copies of the packed network (replaced by az_net_set_params)
  // network
  bool net_loaded = false;
  std::vector<float> blob;
  std::unique_ptr<const NetMaps> net_maps;   // net_layout.h: the index maps of the arrays below; they depend on cfg only, so the first az_net_set_params builds them for all
  std::vector<unsigned char> trainable;      // net_layout.h trainable_mask: built with net_maps; the regularisation sum of az_learning_status walks it
  NetDev net = {};
  std::unique_ptr<const SimpleMaps> simple_maps;   // SimpleNet engines: net_layout.h, built by the first az_net_set_params
  SimpleDev snet = {};           // k_simplenet's fragments, folded batch norms and layer table (SimpleNet engines)
  Net16bDev net16b = {};         // bf16 fragments (cfg.net_bf16)
  Net16Dev net16 = {};           // k_tower16 fragments (64 filters)
  uint16_t* d_geo[GEO_COUNT] = {};   // Geo16 tables by GeoSlot (resnet16.h); GEO_NTM is NULL where the game has no exact-fit variant
  long long tower_hist[4] = {};  // network launches served by: the split tower, the 3-row-tile form, the packed 11 / 21-tile forms, others (AZHIP_TRACE_ARENA)
  char last_tower[96] = {};      // name of the tower kernel that served the most recent network launch (az_net_last_kernel)
  int num_cu = 0;
  int nn_cap = 0;
  float* d_hfeat = nullptr; float* d_X = nullptr; float* d_A = nullptr; float* d_P = nullptr; float* d_V = nullptr; float* d_Pinv = nullptr;
  GEnv* d_tmp_env = nullptr; int* d_iota = nullptr; int* d_ntmp = nullptr;
  // pinned staging of the key-based network seam (az_net_evaluate_keys): states + count in, P / V out -- pageable copies were most of a call
  GEnv* h_env = nullptr; int* h_n = nullptr; float* h_pv = nullptr;
  // staging
  int* d_slots = nullptr; uint32_t* d_gids = nullptr; GEnv* d_roots = nullptr; uint32_t* d_moves = nullptr; double* d_eta = nullptr; int* d_offsets = nullptr;
  az_move_rec* d_stage = nullptr; unsigned long long* d_keys = nullptr; int* d_actions = nullptr; unsigned long long* d_next = nullptr; signed char* d_term = nullptr; float* d_reward = nullptr;
  char* d_nodebuf = nullptr;
  int* d_visits = nullptr;
  int io_cap = 0;
  Phase ph;                      // the self-play phase in progress, or the last one's leavings (above)
  // hipGraphs of wave pairs (env.use_graphs, one slot group only): key = upper bound of the leaves of a launch (decides the tower
  // kernel and its grid); rebuilt after az_net_set_params (new device pointers)
  std::map<int, hipGraphExec_t> wave_graphs;
  bool pending[AZ_MAX_GROUPS] = {};       // the group's last wave awaits its expand + backup (flush_pending)
  int wave_par[AZ_MAX_GROUPS] = {};       // parity of the group's last wave: which of its two leaf counters is current
  int group_active[AZ_MAX_GROUPS] = {};   // active slots per slot group (host count; bounds the leaves of a network launch)
  // (r6) free-running phases (az_engine_cfg.lock_step = 0; tree.h k_tree / k_move_fr): the device hands out game ids and writes
  // finished games into the phase buffer itself; the host looks every fr_round_waves waves (fr_round, azhip.hip)
  hipStream_t fr_s[4] = {}; hipEvent_t fr_ev[4] = {};   // one slot group: the streams and events of its free-running phases (gs[0] = gt[0] = fr_s[0] meanwhile): [0] the wave, [1] background search, [2] move step, [3] k_set_word behind a tower form that does not raise the stop word itself
  FRState* d_fr = nullptr; az_game_rec* d_done = nullptr; long long* d_done_off = nullptr; int done_cap = 0;
  int* h_busy = nullptr; int* d_busy = nullptr;      // [AZ_MAX_GROUPS] host-mapped: slots of each group still inside an explore! that runs ahead (DView::busy_host); -1 = no report
  int* d_bg_stop = nullptr; int bg_seq = 0; bool bg_signal = false;   // the background search's stop word: raised to bg_seq by the wave's tower near its end (paired forms) or by k_set_word behind it (bg_signal: this wave has one)
  int* h_fr_words = nullptr; int* d_fr_words = nullptr;  // host-mapped: finished games / searching slots as of the previous wave (FRArgs::host_words)
  std::vector<az_game_rec> h_done; std::vector<long long> h_done_off;   // a look's finished games where they outgrow h_fetch
  // the step report (tree.h StepReport, pinned and host-mapped: k_step_report writes it behind the wave, fr_round reads it after one
  // synchronisation); report_fresh: no kernel has been launched since it was written, so az_selfplay_get_stats may take its sums from it
  // (report_fresh holds only while EVERY launch that can write the statistics accumulators clears it: today that is k_tree alone, and all
  // its launches go through LAUNCH_ON, which clears it, or through the graph replay in run_waves, which does so by hand.  A launch added
  // outside the macro that touches DView::stat must clear it too.)
  StepReport* h_report = nullptr; StepReport* d_report = nullptr; bool report_fresh = false;
  char* h_fetch = nullptr;           // pinned staging of a look's finished games: records, offsets, move records (FETCH_BYTES; larger batches go straight to the vectors)
  // device-resident records of the current phase (az_selfplay_run / begin with num_games > 0): the move records of every
  // finished game stay in HBM (d_phase, game after game in finishing order; Phase::dev_games says where)
  az_move_rec* d_phase = nullptr; int64_t phase_cap = 0;
  // profiling
  bool prof_on = false;
  int prof_mask = 0;             // 0 = every kernel class, else bit per az_kernel_class
  std::vector<ProfRec> prof_pool;
  size_t prof_used = 0;
  az_prof prof = {};
  double next_exec = 1.0;        // executed-product fraction of the NEXT profiled launch (set by the tower launches, consumed by prof_begin)
  std::vector<int> h_finished;
  std::vector<az_game_rec> h_grec;
  // MinMax player (minmax.hip): mm_on = az_arena_run treats this engine as MinMax.Player(mm); staging for mm_cap roots
  bool mm_on = false;
  az_minmax_cfg mm = {};
  GEnv* d_mm_roots = nullptr; double* d_mm_q = nullptr; int mm_cap = 0;
  // Connect Four solver (solver.hip): staging for sv_cap states -- keys in, 7 q-values and 7 node counts per state out
  unsigned long long* d_sv_keys = nullptr; int8_t* d_sv_q = nullptr; long long* d_sv_nodes = nullptr; int sv_cap = 0;
};

template <class T> inline int dalloc(az_engine* e, T** p, size_t n, bool zero = true) {
  void* q = nullptr;
  size_t bytes = std::max<size_t>(n * sizeof(T), 16);
  hipError_t r = hipMalloc(&q, bytes);
  if (r != hipSuccess) return fail(AZ_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(r));
  e->allocs.push_back(q);
  e->alloc_bytes += bytes;
  if (zero) HIPCHK(hipMemsetAsync(q, 0, bytes, e->stream));
  *p = (T*)q;
  return AZ_OK;
}

// pinned staging: copies from / to it are real asynchronous DMA
template <class T> inline int halloc_pinned(az_engine* e, T** h, size_t n, unsigned flags = hipHostMallocDefault) {
  HIPCHK(hipHostMalloc((void**)h, sizeof(T) * n, flags));
  e->host_allocs.push_back(*h);
  return AZ_OK;
}
// `n` host-mapped words the kernels write (or read) and the host polls without a sync, all set to `fill`; *d = their device address
inline int halloc_mapped(az_engine* e, int** h, int** d, int n, int fill) {
  AZCHK(halloc_pinned(e, h, (size_t)n, hipHostMallocMapped));
  std::fill_n(*h, n, fill);
  HIPCHK(hipHostGetDevicePointer((void**)d, *h, 0));
  return AZ_OK;
}

inline int sync_groups(az_engine* e) {
  for (int g = 0; g < e->ngroups; ++g) if (e->gs[g] != e->stream) {
    HIPCHK(hipStreamSynchronize(e->gt[g]));
    HIPCHK(hipStreamSynchronize(e->gs[g]));
  }
  if (e->ph.fr_on && e->fr_s[1]) for (int i = 1; i < 4; ++i) HIPCHK(hipStreamSynchronize(e->fr_s[i]));   // one slot group, free-running: the side stream (move step, background search)
  return AZ_OK;
}
inline int sync_all(az_engine* e) {
  AZCHK(sync_groups(e));
  HIPCHK(hipStreamSynchronize(e->stream));
  return AZ_OK;
}
inline int prof_flush(az_engine* e) {
  if (!e->prof_used) return AZ_OK;
  AZCHK(sync_all(e));
  for (size_t i = 0; i < e->prof_used; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->prof_pool[i].a, e->prof_pool[i].b));
    e->prof.ms[e->prof_pool[i].cls] += ms;
  }
  e->prof_used = 0;
  return AZ_OK;
}
inline int prof_begin(az_engine* e, hipStream_t st, int cls, int64_t units) {
  if (!e->prof_on || (e->prof_mask && !((e->prof_mask >> cls) & 1))) return AZ_OK;
  if (e->prof_used == e->prof_pool.size()) AZCHK(prof_flush(e));
  ProfRec& r = e->prof_pool[e->prof_used];
  r.cls = cls;
  e->prof.launches[cls] += 1;
  e->prof.units[cls] += units;
  e->prof.exec_units[cls] += (double)units * e->next_exec;          // the tower launches set next_exec (the form's frac(), net_impl.h); everything else counts in full
  e->next_exec = 1.0;
  HIPCHK(hipEventRecord(r.a, st));
  return AZ_OK;
}
inline int prof_end(az_engine* e, hipStream_t st, int cls) {
  if (!e->prof_on || (e->prof_mask && !((e->prof_mask >> cls) & 1))) return AZ_OK;
  HIPCHK(hipEventRecord(e->prof_pool[e->prof_used].b, st));
  e->prof_used++;
  return AZ_OK;
}
#define LAUNCH_ON(e, st, cls, units, kern, grid, block, shmem, ...)         \
  do {                                                                      \
    AZCHK(prof_begin(e, st, cls, units));                                   \
    (e)->report_fresh = false;                                              \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), shmem, st, __VA_ARGS__); \
    AZCHK(prof_end(e, st, cls));                                            \
  } while (0)
#define LAUNCH(e, cls, units, kern, grid, block, shmem, ...) LAUNCH_ON(e, (e)->stream, cls, units, kern, grid, block, shmem, __VA_ARGS__)

#define ENGINE(e)                                              \
  if (!(e)) return fail(AZ_ERR_BAD_ARG, "engine is NULL");      \
  HIPCHK(hipSetDevice((e)->device))

// the engine's last bounded phase as memory_push_device takes it: game k in id order (games[k], when asked for) = d_phase[first[k] .. + cnt[k])
inline void phase_games_by_id(const az_engine* e, std::vector<long long>* first, std::vector<int>* cnt, std::vector<az_game_rec>* games = nullptr) {
  for (int i : order_by_game_id(e->ph.dev_games)) {
    first->push_back(e->ph.dev_off[(size_t)i]); cnt->push_back(e->ph.dev_games[(size_t)i].num_moves);
    if (games) games->push_back(e->ph.dev_games[(size_t)i]);
  }
}

// azhip.hip: waits for the engine's streams and turns a device-side error code (tree.h DERR_*, resnet16.h DERR_EXCHANGE) into a status
int check_device_error(az_engine* e);

// azhip.hip: one launch of the network seam on the engine's stream over the m <= nn_cap rows in d_X / d_A (what az_net_forward launches); P in d_P
// (stride gi.A), V in d_V.  The device trees of a host-stepped game (host_tree.hip) evaluate their new states with it.
int net_seam_planes(az_engine* e, int m);

// azhip.hip: how many streams of this process may launch split towers on `device` at the same time (all engines with 128 filters)
int split_streams_on_device(int device);

// ---- minmax.hip: the MinMax player's think for the arena.  minmax_launch enqueues the walk of `roots` on the engine's stream (so it
// runs beside the other player's search), minmax_fetch waits for it: Q [n][AZ_MAX_ACTIONS] by full action index (NaN: unavailable)
int minmax_launch(az_engine* e, const std::vector<GEnv>& roots);
int minmax_fetch(az_engine* e, int n, std::vector<double>& Q);

// ---- net.hip: every instantiation of the tower / heads kernels lives there ----------------------------------
int net_set_kernel_attrs(az_engine* e);   // + uploads the row permutation tables of the tower kernels (e->d_geo)
// tower + heads on n_max boards (device count in n_ptr when given): from_planes ? X / Amask : envs[eslots[i]]
int net_launch(az_engine* e, hipStream_t st, bool from_planes, float* hfeat, const GEnv* envs, const int* eslots, const int* n_ptr,
               int n_max, const float* X, const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride);
// the network part of one search wave of slot group g (at most nmax leaves)
int net_wave(az_engine* e, int g, bool split, int nmax);

// ---- devices and device memory ---------------------------------------------------------------------------------------------------
// "is `device` a visible device; make it current": every creator's first step
inline int use_device(int device) {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(AZ_ERR_BAD_ARG, "device %d not available (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  return AZ_OK;
}
// n elements of device memory (at least 16 bytes), remembered in *keep when given: the owner frees what `keep` lists
template <class T> inline int mem_alloc(std::vector<void*>* keep, T** p, size_t n) {
  void* q = nullptr;
  size_t bytes = std::max<size_t>(n * sizeof(T), 16);
  hipError_t r = hipMalloc(&q, bytes);
  if (r != hipSuccess) return fail(AZ_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(r));
  if (keep) keep->push_back(q);
  *p = (T*)q;
  return AZ_OK;
}
// The device memory of ONE call: alloc() as mem_alloc, the destructor frees (in allocation order) on whichever path the call leaves,
// so its body is straight-line code with AZCHK / HIPCHK.  Declare it before the first use of its memory and let it live until the
// stream has been waited for.  scratch_live_bytes: what all Scratch objects of the process hold right now (az_debug_scratch_live_bytes;
// 0 between calls, or a call leaked).
inline std::atomic<long long> scratch_live_bytes{0};
class Scratch {
 public:
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    for (void* p : held) (void)hipFree(p);
    scratch_live_bytes -= bytes;
  }
  template <class T> int alloc(T** p, size_t n) {
    AZCHK(mem_alloc(&held, p, n));
    const long long b = (long long)std::max<size_t>(n * sizeof(T), 16);
    bytes += b; scratch_live_bytes += b;
    return AZ_OK;
  }
 private:
  std::vector<void*> held;
  long long bytes = 0;
};
// Debug seam (not in azhip.h, no environment switch; azhip.hip): the process-wide count above.  tests/test_scratch_gpu.py reads 0 after
// calls that succeed and calls that are refused half way.
extern "C" int az_debug_scratch_live_bytes(int64_t* bytes);

// ---- replay memory records shared by memory.hip, plane_memory.hip, comm.hip and train.hip -------------------------------------
// Every member has its initial value here, as az_engine's: a creator fills the record step by step and the record's destroy takes it
// apart at any point in between.
struct az_memory {
  int game = 0, device = 0;
  GameInfo gi = {};
  hipStream_t stream = nullptr;
  az_sample* d_buf = nullptr;         // [ring.cap]
  Ring ring;                          // ring_books.h
};
struct az_dataset {
  int game = 0, device = 0;
  GameInfo gi = {};
  hipStream_t stream = nullptr;
  int64_t n = 0, sum_n = 0;
  double Wtot = 0.0;
  float Wmean = 0.f, Hp = 0.f;
  az_sample* d_samples = nullptr;
  GEnv* d_envs = nullptr;
  float *d_W = nullptr, *d_X = nullptr, *d_A = nullptr, *d_P = nullptr, *d_V = nullptr;
  std::vector<void*> allocs;
  bool own_stream = false;           // made from tensors or planes: no memory behind it whose stream it could share; d_samples and d_envs are NULL
};
// The empty data set every builder starts from (az_dataset_destroy takes it from here at any stage).  share != NULL: the data set
// works on that stream, its memory's; otherwise it owns the stream its builder creates for it.
inline int dataset_new(int game, int device, const GameInfo& gi, hipStream_t share, az_dataset** out) {
  az_dataset* d = new (std::nothrow) az_dataset();
  if (!d) return fail(AZ_ERR_HIP, "out of host memory");
  d->game = game; d->device = device; d->gi = gi; d->stream = share; d->own_stream = !share;
  *out = d;
  return AZ_OK;
}
// ---- the frame of the three data-set creators (from a keyed memory, from a plane memory, from caller tensors) ----
// what all of them ask of `which` and of samples_weighing_policy
inline int dataset_check_args(int which, int weighing_policy) {
  if (which != 0 && which != 1) return fail(AZ_ERR_BAD_ARG, "which must be 0 (get_experience) or 1 (last_batch)");
  if (weighing_policy < AZ_WEIGHT_CONSTANT || weighing_policy > AZ_WEIGHT_LINEAR) return fail(AZ_ERR_BAD_ARG, "unknown samples_weighing_policy %d", weighing_policy);
  return AZ_OK;
}
// dataset_new, then build(d); *out gets the data set if that succeeded, otherwise it is destroyed and *out stays NULL
template <class Build> inline int dataset_create(int game, int device, const GameInfo& gi, hipStream_t share, az_dataset** out, Build build) {
  az_dataset* d = nullptr;
  AZCHK(dataset_new(game, device, gi, share, &d));
  const int st = build(d);
  if (st != AZ_OK) { az_dataset_destroy(d); return st; }
  *out = d;
  return AZ_OK;
}
// the five tensors of convert_samples for n rows of d's geometry
inline int dataset_alloc_tensors(az_dataset* d, int64_t n) {
  const size_t N = (size_t)n, nA = (size_t)d->gi.A, xs = (size_t)d->gi.C * d->gi.P;
  AZCHK(mem_alloc(&d->allocs, &d->d_W, N)); AZCHK(mem_alloc(&d->allocs, &d->d_V, N));
  AZCHK(mem_alloc(&d->allocs, &d->d_A, N * nA)); AZCHK(mem_alloc(&d->allocs, &d->d_P, N * nA)); AZCHK(mem_alloc(&d->allocs, &d->d_X, N * xs));
  return AZ_OK;
}
// plane_memory.hip: MemoryBuffer for a host-stepped game.  A sample is what the network sees -- the row (X, A) of RW = C*H*W + nA
// Float32 words -- plus ND = nA + 2 doubles (pi by full action index, z, t) and n.
struct az_plane_memory {
  int game = 0, device = 0;
  GameInfo gi = {};
  hipStream_t stream = nullptr;
  int xs = 0, nA = 0, RW = 0, ND = 0;
  float* d_XA = nullptr;             // [cap][RW]
  double* d_D = nullptr;             // [cap][ND]
  long long* d_n = nullptr;          // [cap]
  Ring ring;                         // ring_books.h; d_XA, d_D and d_n have ring.cap rows
  int hash_bits = 128;               // az_debug_plane_memory_hash_bits lowers it
  // GI.symmetries as the host declared them (az_plane_memory_set_symmetries): symmetry k as ONE gather over the row's RW words,
  // perm[k][w] = xperm[k][w] for w < xs, xs + aperm[k][w - xs] after; 16 bits hold an index below RW <= xs + 126
  int nsym = 0;                      // 0: none declared
  unsigned short* d_perm = nullptr;  // [AZ_PLANE_MAX_SYMMETRIES][RW], rows [0, nsym) valid
};
static constexpr int PM_WAVES = 4;    // wavefronts per workgroup of the plane kernels (plane_memory.hip, comm.hip): one sample / pair / group each
static inline unsigned pm_grid(long long n) { return (unsigned)((n + PM_WAVES - 1) / PM_WAVES); }
// Debug seams of comm.hip (not in azhip.h, no environment switch).  az_debug_comm_plane_round_rows: az_comm_gather_push_planes sends at
// most `rows` records per rank and round (0: the default of plane_gather.h; never more than it) -- the same value on every rank.
// az_debug_comm_plane_kernel_ms: HIP-event time of k_pg_pack and k_pg_scatter, summed over the rounds of the communicator's last
// az_comm_gather_push_planes (tools/plane_gather_bench.py).
struct az_comm;
extern "C" int az_debug_comm_plane_round_rows(az_comm* c, int64_t rows);
extern "C" int az_debug_comm_plane_kernel_ms(az_comm* c, double* pack_ms, double* scatter_ms);
// the weight convert_samples gives a sample seen n times (learning.jl:17-25): every data-set builder's
__device__ __forceinline__ float sample_weight(int policy, long long n) {
  return policy == AZ_WEIGHT_CONSTANT ? 1.0f : policy == AZ_WEIGHT_LOG ? (float)(az_log2((double)n) + 1.0) : (float)n;
}
// What is wrong with a sample of caller-supplied tensors: k_ds_check (memory.hip) and k_pm_check (plane_memory.hip) leave the smallest
// (sample << 3 | clause) that failed in one word that starts as ~0, so the message does not depend on scheduling.  Clause 2 is the
// checker's own (W <= 0 there, n < 1 here): its text comes from the caller.
enum SampleFault { SF_NONFINITE = 1, SF_OWN = 2, SF_A01 = 3, SF_NOLEGAL = 4, SF_PNEG = 5, SF_PILLEGAL = 6 };
__device__ __forceinline__ void sample_fault_raise(unsigned long long* bad, long long sample, int clause) {
  atomicMin(bad, ((unsigned long long)sample << 3) | (unsigned long long)clause);
}
inline int sample_fault_status(unsigned long long bad, const char* own_clause) {
  if (bad == ~0ull) return AZ_OK;
  const char* const what[] = {"", "a non-finite value", own_clause, "an entry of A outside {0, 1}", "no legal action (a row of A without a 1)",
                              "P < 0", "P > 0 where A == 0 (the loss takes the logarithm of the masked policy there)"};
  return fail(AZ_ERR_BAD_ARG, "sample %lld: %s", (long long)(bad >> 3), what[bad & 7]);
}
// memory.hip: checks the (W, X, A, P, V) tensors of a data set on the device as az_dataset_create_from_tensors documents
// (AZ_ERR_BAD_ARG naming the first offending sample) and sets Wtot, Wmean and Hp from them
int dataset_tensor_stats(az_dataset* d, hipStream_t st);
// push_trace! (memory.jl:74-87) of ng games whose move records are ALREADY on the device: game g = d_moves[first[g] .. +cnt[g])
int memory_push_device(az_memory* m, const az_move_rec* d_moves, const std::vector<long long>& first, const std::vector<int>& cnt, double gamma);
