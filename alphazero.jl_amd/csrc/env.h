// env.h -- every AZHIP_* override libazhip.so reads, and the only file of csrc/ that calls getenv.  Plain C++ (no device
// runtime): a host compiler builds it alone (tests/env_driver.cpp).  The overrides are diagnostics, A/B aids and test knobs; the
// product path sets none of them.
// One struct per MOMENT the environment is read.  A member's initialiser IS its reader -- name, parsing, default and range rule on
// one line, purpose beside it -- so constructing the struct reads all of that moment's overrides together, and the names inside
// `struct EnvCreate` are the creation-time set (azhip/engine.py CREATE_ENV), the names in the file all there are (DESIGN.md
// "Environment overrides" is the same table for readers; tests/test_env_overrides.py holds the three to each other).
// Parsing and range rules live here; decisions that also depend on the configuration or the device stay at their point of use.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdlib>

inline const char* env_str(const char* name, const char* unset) { const char* s = getenv(name); return s ? s : unset; }
inline bool env_set(const char* name) { return getenv(name) != nullptr; }                                       // presence only: "=0" and "" count
inline int env_int(const char* name, int unset) { const char* s = getenv(name); return s ? atoi(s) : unset; }
inline bool env_on(const char* name) { return env_int(name, 0) != 0; }                                          // off unless set to a non-zero number
inline bool env_not_off(const char* name) { return env_int(name, 1) != 0; }                                     // on unless set to 0 (or to no number)
inline int env_tri(const char* name) { return env_set(name) ? (int)env_on(name) : -1; }                         // 0 | 1, -1 = unset: decided at the point of use
// `unset` as it is when the variable is not there, else its number brought into lo .. hi
inline int env_clamp(const char* name, int unset, int lo, int hi) { const int x = env_int(name, lo); return !env_set(name) ? unset : x < lo ? lo : x > hi ? hi : x; }
// the variable's number where it lies in lo .. hi, else `other`
inline long env_within(const char* name, long other, long lo, long hi) { const long x = atol(env_str(name, "")); return env_set(name) && x >= lo && x <= hi ? x : other; }

struct EnvCreate {               // az_engine_create (az_engine::env)
  int tower_pick = env_int("AZHIP_TOWER", 0);                        // a TowerForm value (2 | 3 | 7 | 16 | 19 | 20 | 21 | 22 | 32) forces that form where it exists; 0 = choose per launch
  bool tower_mixed = env_on("AZHIP_TOWER_MIXED");                    // a free-running wave of 15 .. 16 boards per CU goes out as one k_tower16x2m launch (measured slower: wave_net_f)
  int heads_pick = env_int("AZHIP_HEADS", 0);                        // 16 | 32 forces k_heads16 / k_heads_mfma; 0 = by launch size
  int use_graphs = env_int("AZHIP_GRAPH", 0);                        // wave pairs of a one-group engine are replayed as hipGraphs (lock step, no evaluation cache)
  bool tree_sort = env_on("AZHIP_TREE_SORT");                        // k_tree experiment: the slots of a launch in depth order, re-sorted at every move step
  int bk_mode = (int)env_within("AZHIP_TREE_ATOMIC", 0, 1, 2);       // k_tree experiment: 1 | 2 = backups as no-return atomics (DView::bk_mode)
  int explore_k = env_int("AZHIP_EXPLORE_K", 8);                     // simulations per slot and launch inside MCTS.explore! of the hooks and the arena; 0 / 1 = lock step
  long long xch_fail_at = atoll(env_str("AZHIP_XCH_FAIL_AT", "0"));  // tests: the n-th split launch loses a partner (fault injection); 0 = never
  unsigned long long xch_epoch0 = strtoull(env_str("AZHIP_XCH_EPOCH0", "0"), nullptr, 0);   // tests (hex accepted): first launch epoch of k_tower16s, to start near its 24-bit wrap
  bool pooled_queue = env_set("AZHIP_POOLED_QUEUE");                 // the engine's stream stays in the runtime's pool of hardware queues instead of getting a queue of its own
  uint32_t tag_mask = (1u << env_clamp("AZHIP_HT_TAG_BITS", 16, 0, 16)) - 1u;   // tests: tag bits of a hash-table entry; fewer make unequal states share tags, 0 leaves the exact key compare
  uint32_t epoch0 = (uint32_t)env_within("AZHIP_HT_EPOCH0", 1, 1, 0xfffe);     // tests: first 16-bit table epoch -- near the wrap a reset really clears the table
  int vmm = env_tri("AZHIP_VMM");                                    // 0 | 1 forces the plain / mapped-on-demand node pool; unset = by pool size
  bool vmm_keys = env_not_off("AZHIP_VMM_KEYS");                     // 0 keeps the dense side-record array beside a mapped pool
  int eval_cache = env_tri("AZHIP_EVAL_CACHE");                      // 0 = no evaluation cache, 1 = also for the exact synthetic oracles; unset = ResNet oracle only
  int eval_cache_log2 = env_clamp("AZHIP_EVAL_CACHE_LOG2", 0, 4, 28);   // log2 of the cache's 64-byte entries; 0 (unset) = sized from slots x simulations
  double pool_gb = atof(env_str("AZHIP_POOL_GB", "-1"));             // GB of physical memory a mapped-on-demand pool may take; < 0 (unset) = free memory minus a margin
};
struct EnvPhase {                // az_selfplay_begin: every phase
  int free_run = env_tri("AZHIP_FREE_RUN");                          // 0 | 1 overrides az_engine_cfg.lock_step; unset = what the configuration says
  int run_k = env_clamp("AZHIP_RUN_K", 3, 1, INT_MAX);               // simulations a slot may select per wave launch of a free-running phase
  int run_kbg = env_clamp("AZHIP_RUN_KBG", -1, 0, INT_MAX);          // ... per background launch; -1 (unset) = 32 with one slot group, else 8
  int round_waves = env_clamp("AZHIP_FR_ROUND", 128, 1, INT_MAX);    // waves between two looks of the host
};
struct EnvProcess {              // once per process, at the first free-running wave (env_process)
  bool bg_stop = env_not_off("AZHIP_BG_STOP");                       // 0 switches the background search's stop word off (A/B: without it a background launch outlasts a short tower)
  int bg_prio = env_int("AZHIP_BG_PRIO", 0);                         // A/B aid: non-zero = the background launches keep the wave launches' priority
};
inline const EnvProcess& env_process() { static const EnvProcess p; return p; }
struct EnvArena {                // az_arena_run: every call
  bool trace = env_set("AZHIP_TRACE_ARENA");                         // print which tower forms served the evaluation, and who else counted as a split-tower user
};
struct EnvTrainer {              // az_trainer_create (az_trainer::env)
  bool fin_inside = env_on("AZHIP_TRAIN_FINISH_INSIDE");             // second stage of the column sums in the producer's last workgroup (measured slower: off)
  bool conv_nt6 = env_not_off("AZHIP_TRAIN_NT6");                    // 0 switches the 6-tile layer kernel off (A/B)
  bool one_stream = env_on("AZHIP_TRAIN_ONE_STREAM");                // diagnosis: the weight gradients in line with everything else, on the step's own stream
  bool wg_late = env_on("AZHIP_TRAIN_WG_LATE");                      // diagnosis: k_wgrad16(l) only after the data gradient of layer l, not beside it
};
struct EnvComm {                 // comm.hip rc::load: the first az_comm_* call
  const char* rccl_lib = env_str("AZHIP_RCCL_LIB", nullptr);         // path of a librccl*: what az_comm_* loads instead of RCCL (tests/rccl_stub: several ranks on one GPU)
};
