/*
 * azhip.h -- C ABI of the MI355X-native self-play engine (libazhip.so).
 *
 * This is the drop-in boundary for ONE path of jonathan-laurent/AlphaZero.jl: the batched
 * MCTS self-play loop plus the ResNet oracle forward.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repository) -- see
 * INTEGRATION.md for the Julia `ccall` glue a maintainer would add.
 *
 * Conventions
 *   - every function returns an int status: AZ_OK (0) or a negative az_status; no C++
 *     exception crosses the boundary; az_last_error() gives a thread-local message that
 *     stays valid until the next call on that thread;
 *   - the caller allocates and frees every host buffer and passes capacities; the engine
 *     owns all device memory and frees it in az_engine_destroy();
 *   - one engine per GPU, not thread-safe, calls block until their results are ready;
 *   - callbacks are invoked synchronously on the calling thread only.
 *
 * State keys.  A game state (the reference's `(board=…, curplayer=…)` named tuple) crosses
 * the ABI as two 64-bit words `key[0], key[1]`; bit 63 of key[0] is set when BLACK is to move.
 *   Connect-Four  key[0] bits col*7+row = WHITE stones, key[1] same for BLACK
 *                 (col 0..6, row 0..5, row 0 = bottom; games/connect-four/game.jl:19,87-93)
 *   Tic-tac-toe   key[0] bits pos = WHITE marks, key[1] bits pos = BLACK marks
 *                 (pos = (y-1)*3 + x - 1; games/tictactoe/game.jl:39)
 *   Mancala       key[0] bytes 0..5 = WHITE houses 1..6, byte 6 = WHITE store;
 *                 key[1] the same for BLACK (games/mancala/game.jl:20-31)
 *
 * fp32 contract of the network (what "the same result" means, bit for bit).  Every output
 * of a convolution or dense layer is ONE fp32 fused-multiply-add chain starting from +0:
 *   3x3 conv (Cin even): taps t = 0..8 with (dy,dx) = (t/3-1, t%3-1); inside a tap the
 *                        channels in the order c = j, Cin/2 + j for j = 0..Cin/2-1 (the K
 *                        order of v_mfma_f32_32x32x2_f32: lanes 0-31 then lanes 32-63)
 *   stem conv          : k = t*Cin + c, K = 9*Cin; order k = j, K2 + j for j = 0..K2-1 with
 *                        K2 = ceil(K/2) (same MFMA, K padded to even with a zero)
 *   1x1 conv           : c = j, Cin/2 + j
 *   dense              : k = p*nf + f ascending (p = x + W*y, f = head filter)
 * followed by y = fma(acc, scale, shift), scale = gamma / sqrtf(var + 1e-5f),
 * shift = fma(bias - mean, scale, beta) (test-mode BatchNorm folded), `+ residual`, ReLU;
 * dense layers add their bias after the chain.  softmax/tanh use az_expf/az_tanhf of
 * az_numerics.h.  The reference (Flux/NNlib/cuDNN) defines no summation order; any order
 * is within the 1e-5 tolerance BASELINE.json states, this one is also reproducible.
 *
 * Environment: the product path sets no variable.  The library reads AZHIP_* overrides for diagnostics, A/B runs and tests; the
 * ones a host may meet are AZHIP_FREE_RUN=0|1 (lock-step / free-running phases whatever az_engine_cfg.lock_step says, read at
 * az_selfplay_begin), AZHIP_EVAL_CACHE=0 (no evaluation cache), AZHIP_VMM=0|1 and AZHIP_POOL_GB (form and physical bound of the
 * node pool; all three read at az_engine_create) and AZHIP_RCCL_LIB=<path> (the library az_comm_* loads).  DESIGN.md
 * "Environment overrides" lists every one with its values, default and the moment it is read; csrc/env.h reads them.
 *
 * RNG contract: include/az_numerics.h (philox4x32-10 keyed by seed, counter = game id,
 * move index, purpose, draw index).
 */
#ifndef AZHIP_H
#define AZHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_ABI_VERSION 4   /* 4 (round 6): az_engine_cfg.lock_step, az_selfplay_stats.slot_launches; 3 (round 5): az_gather_stats.replaced_games, az_selfplay_stats.evals_reused; 2 (round 4): az_selfplay_stats.aborted_games, az_gather_stats' report fields, az_prof.exec_units, az_comm_version */

typedef enum {
  AZ_OK = 0,
  AZ_ERR_BAD_ARG = -1,   /* invalid argument / unsupported configuration */
  AZ_ERR_CAPACITY = -2,  /* node pool, hash table, path, trace or caller buffer too small */
  AZ_ERR_HIP = -3,       /* a HIP runtime call failed */
  AZ_ERR_STATE = -4,     /* call made in the wrong engine state */
  AZ_ERR_COMM = -5       /* an RCCL call failed / librccl.so could not be loaded */
} az_status;

typedef enum {
  AZ_GAME_CONNECT_FOUR = 0, AZ_GAME_TICTACTOE = 1, AZ_GAME_MANCALA = 2,
  /* Network-only tensor geometry, no device twin: GI.state_dim = (9, 9, 4), 82 actions -- OpenSpiel 9x9 Go through
   * src/openspiel.jl (BASELINE configs[4]).  Rules and tree stay on the host; the engine serves az_net_set_params /
   * az_net_forward (Network.forward_normalized) for it, keeps its samples in a replay memory of planes (az_plane_memory_*), trains it on a
   * data set made from that memory or from tensors (az_dataset_create_from_plane_memory, az_dataset_create_from_tensors, az_trainer_*,
   * az_learning_status) and rejects every search, game, key-based and keyed replay-memory (az_memory_*) entry point. */
  AZ_GAME_GO9_PLANES = 3
} az_game_id;

/* Which oracle the search consults (src/mcts.jl:6-17). */
typedef enum {
  AZ_ORACLE_UNIFORM = 0, /* MCTS.RandomOracle (src/mcts.jl:62-72): uniform prior, V = 0 */
  AZ_ORACLE_HASH = 1,    /* synthetic, exact: priors/value derived from the state key (tests) */
  AZ_ORACLE_RESNET = 2,  /* the two-headed ResNet (src/networks/architectures/resnet.jl) */
  AZ_ORACLE_ROLLOUT = 3, /* MCTS.RolloutOracle (src/mcts.jl:35-60), gamma = 1 as Benchmark.MctsRollouts builds it
                            (src/benchmark.jl:141-143): uniform prior, V = outcome of one random playout */
  AZ_ORACLE_SIMPLENET = 4 /* NetLib.SimpleNet (src/networks/architectures/simplenet.jl:37-64), the dense two-headed network of the
                            tictactoe, ospiel_ttt and grid-world experiments: engines made by az_engine_create_simplenet only */
} az_oracle_kind;

#define AZ_MAX_ACTIONS 9
#define AZ_SCHED_MAX 8

/* MctsParams (src/params.jl:49-57) + SimParams (src/params.jl:92-101) + ResNetHP
 * (src/networks/architectures/resnet.jl:30-37).  Fill with az_engine_cfg_init() first. */
typedef struct {
  int32_t struct_size;        /* sizeof(az_engine_cfg), set by az_engine_cfg_init */
  int32_t device;             /* HIP device ordinal */
  int32_t game;               /* az_game_id */
  int32_t oracle;             /* az_oracle_kind */
  /* MctsParams */
  double gamma;               /* reward discount */
  double cpuct;
  double dirichlet_noise_eps;
  double dirichlet_noise_alpha;
  double prior_temperature;
  int32_t num_iters_per_turn; /* >= 2; 0 = NetworkPlayer, no search (az_arena_run only, ResNet oracle) */
  int32_t temperature_len;    /* PLSchedule breakpoints; 1 == ConstSchedule */
  int32_t temperature_xs[AZ_SCHED_MAX];
  double temperature_ys[AZ_SCHED_MAX];
  /* SimParams */
  int32_t num_workers;        /* number of device game slots searched in lock-step */
  int32_t batch_size;         /* must be <= num_workers (src/params.jl:361-384); the device path
                                 evaluates every pending leaf of a wave in one pass */
  int32_t reset_every;        /* reset a slot's tree every n games; 0 = never (`nothing`) */
  int32_t fill_batches;       /* accepted, no effect: test-mode BN is per sample (Appendix A.13) */
  double flip_probability;    /* play.jl:305-307; honoured by az_selfplay_* (on the device) and az_arena_run */
  uint64_t seed;
  /* capacities; 0 = derive from the game and num_iters_per_turn */
  int32_t max_nodes_per_slot;
  int32_t max_moves_per_game;
  /* ResNetHP (kernel 3x3) */
  int32_t num_blocks;
  int32_t num_filters;
  int32_t num_policy_head_filters;
  int32_t num_value_head_filters;
  /* 0: fp32 tower, the fp32 contract above (default).  1: the residual tower runs in bfloat16 (weights and activations
   * rounded to bf16, fp32 accumulation, csrc/resnet16b.h) -- BASELINE configs[4] "ResNet 10x128 bf16"; outputs agree with
   * the fp32 network to bf16 accuracy, not bit for bit, so searches are not comparable move for move with the oracle. */
  int32_t net_bf16;
  /* How az_selfplay_* schedules the workers (round 6).
   * 0 (default): FREE-RUNNING.  A worker of the reference runs its simulations and its games at its own pace (simulations.jl:216-243,
   *   util.jl:169-200: the next game id is taken under a lock by whichever worker finishes first).  So does a slot: within one launch
   *   of the tree kernel it completes every simulation that ends on a terminal state or on a state the engine has evaluated before,
   *   and stops only where it needs the network; it plays its move when ITS explore! is complete and takes the next game id from an
   *   atomic counter when ITS game ends.  Every network launch then holds one board of every searching slot.  A game's records depend
   *   on its id and on the games that shared its tree; with reset_every = 1 on the id alone, whatever the schedule.  With
   *   reset_every != 1 the slot -> game assignment (az_game_rec.slot; a slot plays its games in increasing id order) is one outcome
   *   of the reference's own race and can differ from run to run; the parity tests hand the assignment the device reports to the oracle.
   * 1: LOCK STEP, rounds 1-5: one simulation per slot and wave, all slots move together every num_iters_per_turn waves, finished
   *   slots take the next ids in slot order -- a fixed assignment, reproducible for every reset_every.
   * The hooks (az_mcts_explore), the arena, the rollout oracle and hipGraph replay always run in lock step.  AZHIP_FREE_RUN=0|1
   * overrides the field (tests, A/B runs). */
  int32_t lock_step;
} az_engine_cfg;

typedef struct az_engine az_engine;

const char* az_last_error(void);
int az_abi_version(void);
/* sizeof() of a struct of this header as the LIBRARY was compiled (which = az_struct_id), -1 for an unknown id: a host mirror
 * (ctypes, Julia isbits structs) asserts its own sizes against these, so that a stale mirror fails at load time instead of
 * being written out of bounds. */
typedef enum {
  AZ_STRUCT_ENGINE_CFG = 0, AZ_STRUCT_MOVE_REC = 1, AZ_STRUCT_GAME_REC = 2, AZ_STRUCT_TRACE_BUF = 3, AZ_STRUCT_SELFPLAY_STATS = 4,
  AZ_STRUCT_SAMPLE = 5, AZ_STRUCT_DATASET_INFO = 6, AZ_STRUCT_LEARNING_STATUS = 7, AZ_STRUCT_TRAIN_CFG = 8, AZ_STRUCT_GATHER_STATS = 9,
  AZ_STRUCT_PROF = 10, AZ_STRUCT_MINMAX_CFG = 11, AZ_STRUCT_SOLVER_CFG = 12, AZ_STRUCT_HOST_TREE_CFG = 13, AZ_STRUCT_HOST_TREE_STATS = 14,
  AZ_STRUCT_SIMPLENET_HP = 15
} az_struct_id;
int az_abi_struct_size(int32_t which);

/* Defaults = games/connect-four/params.jl:5-30 with the 64-filter trunk. */
int az_engine_cfg_init(az_engine_cfg* cfg);
int az_engine_create(const az_engine_cfg* cfg, az_engine** out);
/* SimpleNetHP (src/networks/architectures/simplenet.jl:15-22); the batch-norm momentum is az_train_cfg's. */
typedef struct {
  int32_t struct_size;        /* sizeof(az_simplenet_hp), set by az_simplenet_hp_init */
  int32_t width;              /* 1 .. 256 */
  int32_t depth_common;       /* each depth 0 .. 16 */
  int32_t depth_phead;
  int32_t depth_vhead;
  int32_t use_batch_norm;     /* 0 or 1 */
} az_simplenet_hp;
/* Defaults = games/tictactoe/params.jl: width 200, depth_common 6, batch norm, head depths 1. */
int az_simplenet_hp_init(az_simplenet_hp* hp);
/* An engine whose oracle is a SimpleNet (cfg->oracle is taken as AZ_ORACLE_SIMPLENET, the ResNet fields of cfg are ignored, net_bf16
 * must be 0; not for AZ_GAME_GO9_PLANES).  It serves what a ResNet engine serves -- az_net_*, az_mcts_*, az_selfplay_*, az_arena_run
 * (num_iters_per_turn = 0 included, and against a ResNet engine), az_memory_push_engine, az_learning_status, az_comm_broadcast_params,
 * az_host_tree_*, az_trainer_* (a dense chain; batch_norm_momentum from az_train_cfg).  az_engine_create with AZ_ORACLE_SIMPLENET fails
 * and names this constructor. */
int az_engine_create_simplenet(const az_engine_cfg* cfg, const az_simplenet_hp* hp, az_engine** out);
int az_engine_destroy(az_engine* e);
/* Device memory the engine holds (node pools, tables, network buffers, the phase buffer): a host that keeps engines alive
 * between phases (the reference rebuilds its MCTS.Env per phase, src/simulations.jl:216-218) budgets with it. */
int az_engine_device_bytes(az_engine* e, int64_t* bytes);
/* Frees the device-resident records of the last phase (up to 64 B x num_games x max_moves) once they have been pushed /
 * gathered; the next az_selfplay_run / az_selfplay_begin allocates again. */
int az_engine_release_phase(az_engine* e);

/* ---- game plugin, device twins (GameInterface, src/game.jl:34-336) -------------------- */
int az_game_num_actions(int game, int32_t* num_actions);
int az_game_state_dim(int game, int32_t* w, int32_t* h, int32_t* c); /* GI.state_dim */
int az_game_init_key(int game, uint64_t key[2]);                   /* current_state(init(gspec)) */
/* GI.vectorize_state + GI.actions_mask(GI.init(gspec, s)) for n states, computed on the GPU.
 * X: n*C*H*W floats (per state the Julia W x H x C array in memory order), A: n*num_actions. */
int az_game_encode(az_engine* e, const uint64_t* keys, int32_t n, float* X, float* A);
/* GI.init(gspec, s); GI.play!(g, a): next state, game_terminated, white_reward, on the GPU.
 * actions are 0-based; action -1 = no move (status of GI.init(gspec, s) only).  States that are
 * already terminal are returned unchanged. */
int az_game_play(az_engine* e, const uint64_t* keys, const int32_t* actions, int32_t n,
                 uint64_t* next_keys, int8_t* terminated, float* white_reward);

/* ---- network plugin (Network interface, src/networks/network.jl:30-206) ---------------- */
/* Number of fp32 values in the parameter blob.  Layout, Flux array memory order:
 *   stem   conv W(3,3,C,F) b(F)  bn gamma,beta,mean,var (F each)
 *   block  x num_blocks: conv1 W(3,3,F,F) b bn(4F)  conv2 W(3,3,F,F) b bn(4F)
 *   phead  conv W(1,1,F,npf) b bn(4npf)  dense W(A, P*npf) b(A)
 *   vhead  conv W(1,1,F,nvf) b bn(4nvf)  dense W(F, P*nvf) b(F)  dense W(1,F) b(1)
 * The library's own statement of this layout, and of every reordering of the weights for its kernels, is csrc/net_layout.h (NetLayout). */
int az_net_num_params(const az_engine* e, int64_t* n);
int az_net_set_params(az_engine* e, const float* blob, int64_t n); /* Network.copy(nn; on_gpu=true, test_mode=true) */
int az_net_get_params(const az_engine* e, float* blob, int64_t n);
/* Network.forward_normalized (network.jl:264-271) on host arrays: X W*H*C*N, A nA*N ->
 * P nA*N, V N, Pinv N. */
int az_net_forward(az_engine* e, const float* X, const float* A, int32_t N, float* P, float* V, float* Pinv);
/* Network.evaluate_batch (network.jl:308-315) from state keys: encode + forward on the GPU.
 * P is full width (0 on unavailable actions). */
int az_net_evaluate_keys(az_engine* e, const uint64_t* keys, int32_t N, float* P, float* V);

/* ---- MCTS hooks (src/mcts.jl:239-281; parity + explorer UI, src/ui/explorer.jl:70-86) -- */
int az_mcts_reset(az_engine* e);  /* MCTS.reset! on every slot (counters kept) */
/* MCTS.explore!(env, GI.init(gspec, root), nsims) on slots 0..nslots-1, one root per slot.
 * eta: nslots*AZ_MAX_ACTIONS Dirichlet noise by FULL action index, or NULL to draw it from the
 * RNG contract with (seed, game_ids[i], moves[i]). */
int az_mcts_explore(az_engine* e, const uint64_t* root_keys, int32_t nslots, int32_t nsims,
                    const double* eta, const uint32_t* game_ids, const uint32_t* moves);
/* tree[state] of one slot: per FULL action index (unavailable: N = 0, P = 0); returns
 * AZ_ERR_BAD_ARG if the state is not in the tree. mask = availability bitmask. */
int az_mcts_node_stats(az_engine* e, int32_t slot, const uint64_t key[2], int32_t* N, double* W,
                       float* P, float* Vest, uint32_t* mask);
int az_mcts_counters(az_engine* e, int32_t slot, int64_t* total_simulations,
                     int64_t* total_nodes_traversed, int64_t* num_nodes);

/* ---- self-play (simulate, src/simulations.jl:207-244; play_game, src/play.jl:298-315) --- */
/* One record per move: state BEFORE the move, visit counts by full action index (policy =
 * N / sum N, src/mcts.jl:255-271), the action played (0-based), white reward after it.
 * Self-play with flip_probability > 0 (play.jl:305-307): key is trace.states[i], the state BEFORE the turn's random
 * symmetry; N[AZ_MAX_ACTIONS] = 1 + the symmetry's index in GI.symmetries (0 = the turn was not flipped); `action` is
 * the action played on the IMAGE; N[0..A) hold the image's visit counts placed on the AVAILABLE actions of `key` by
 * rank -- what the reference's convert_sample does with the trace's policy vector (learning.jl:31-33, memory.jl:115-118),
 * so az_memory_push* read a flipped trace like any other. */
typedef struct {
  uint64_t key[2];
  int32_t N[AZ_MAX_ACTIONS + 1];
  int32_t action;
  float reward;
} az_move_rec;
/* One record per game (Trace + self_play_measurements, src/training.jl:269-273). */
typedef struct {
  int32_t game_id;
  int32_t slot;
  int32_t num_moves;
  int32_t first_move;               /* index of the game's first az_move_rec */
  int64_t nodes;                    /* length(env.tree) at the end of the game */
  int64_t total_simulations;        /* cumulative per slot (src/mcts.jl:136-137) */
  int64_t total_nodes_traversed;
  uint64_t final_key[2];
} az_game_rec;
typedef struct {
  az_game_rec* games; int64_t games_cap; int64_t num_games;
  az_move_rec* moves; int64_t moves_cap; int64_t num_moves;
} az_trace_buf;
typedef struct {
  int64_t simulations;              /* MCTS simulations run (src/mcts.jl:242) */
  int64_t nodes_traversed;          /* src/mcts.jl:222 */
  int64_t leaf_evals;               /* oracle calls */
  int64_t moves;                    /* samples */
  int64_t games;
  int64_t waves;                    /* launches of the wave sequence (tree kernel, network) per slot group */
  double seconds;
  int64_t aborted_games;            /* games whose slot ran out of tree nodes (max_nodes_per_slot / device memory) or of move
                                     * records (max_moves_per_game): the slot is retired, the game dropped and counted here
                                     * (ids: az_selfplay_aborted), the phase goes on.  A bounded phase still returns num_games
                                     * games: the slot plays ONE replacement game with id = aborted id | AZ_REPLACEMENT_GAME_BIT
                                     * (its own RNG streams); if that overflows as well the game is given up (both ids reported,
                                     * the phase returns one game fewer).  The reference's Dict has no such limit
                                     * (src/mcts.jl:124-151); with the default pool sizes this stays 0.  Hosts should warn when
                                     * it is not (azhip/training.py, julia/AlphaZeroHIP.jl do). */
  int64_t tower_fallbacks;          /* times the split tower of small launches (k_tower16s: two workgroups per board exchanging halves
                                     * of every layer) gave up waiting for a partner that was not co-resident and the engine fell back
                                     * to the unsplit kernel for good: results are unaffected, small launches get slower.  0 unless
                                     * something else (a trainer, another process) holds the device's CUs. */
  int64_t evals_reused;             /* of leaf_evals: oracle answers taken from the engine's evaluation cache -- the same state already
                                     * evaluated for another slot in this wave, or in an earlier wave since az_net_set_params -- instead
                                     * of a network evaluation.  The reference evaluates every query on its own
                                     * (src/simulations.jl:23-38, src/networks/network.jl:308-315); a test-mode evaluation is a pure
                                     * function of the state and every tower form gives the same bits, so the answers -- and with them
                                     * every record of the phase -- are unchanged (tests/test_eval_cache_gpu.py).  leaf_evals -
                                     * evals_reused = boards the network evaluated.  0 when the cache is off (AZHIP_EVAL_CACHE=0). */
  int64_t slot_launches;            /* sum over the waves of the slots that searched in them: simulations / slot_launches = simulations a slot
                                     * completes per launch of the tree kernel (1 in lock step, ~2 free-running with the evaluation cache) */
} az_selfplay_stats;
#define AZ_REPLACEMENT_GAME_BIT 0x40000000   /* game ids handed to az_selfplay_* must stay below it */
typedef void (*az_progress_cb)(void* user);   /* game_simulated(), once per finished game */

/* simulate(simulator, gspec, SimParams(num_games=…)): plays num_games games with global ids
 * first_game_id .. first_game_id+num_games-1 (so a sharded run is independent of the shard
 * count) and writes the traces sorted by game id. */
int az_selfplay_run(az_engine* e, int32_t num_games, int32_t first_game_id, az_trace_buf* out,
                    az_progress_cb cb, void* user, az_selfplay_stats* stats);
/* Stepping form of the same loop (bench, polling): begin, step `nwaves` search waves, collect finished games, end.
 * num_games < 0 = refill slots forever.  Lock step (az_engine_cfg.lock_step): one simulation per active slot per wave, the move
 * step runs after every num_iters_per_turn waves.  Free-running: a wave carries every slot to its next network evaluation; az_selfplay_step
 * returns with the device idle and every game that ended collectable. */
int az_selfplay_begin(az_engine* e, int32_t num_games, int32_t first_game_id);
int az_selfplay_step(az_engine* e, int32_t nwaves);
int az_selfplay_collect(az_engine* e, az_trace_buf* out);   /* finished, not yet collected */
int az_selfplay_get_stats(az_engine* e, az_selfplay_stats* stats);
int az_selfplay_active(az_engine* e, int32_t* active_slots);
/* ids of the games the current / last phase aborted (see az_selfplay_stats.aborted_games); cap = 0 only counts. */
int az_selfplay_aborted(az_engine* e, int32_t* game_ids, int32_t cap, int32_t* n);
int az_selfplay_end(az_engine* e);

/* ---- arena (pit_networks, src/training.jl:130-144; TwoPlayers, src/play.jl:248-282) ------ */
/* simulate() over TwoPlayers(MctsPlayer(contender), MctsPlayer(baseline)): each engine is one
 * player (its own network, MctsParams and per-worker trees); workers = min(contender's
 * num_workers, num_games); reset_every, flip_probability, gamma and the flip RNG seed are the
 * contender's.  alternate_colors != 0 swaps the colours of the games with odd 1-based sim_id
 * (simulations.jl:221-223): sim_id = game id - first_game_id + 1, the index within this call.  rewards[i] (may be NULL) = total reward of
 * game first_game_id+i from the CONTENDER's side (rewards_and_redundancy, simulations.jl:302-311),
 * *redundancy = 1 - #unique states / #states over all traces.  `out` (may be NULL) receives the
 * traces sorted by game id: az_move_rec.key is trace.states[i] (the state BEFORE the turn's random
 * symmetry), N / action refer to the state the player saw (after it), N[AZ_MAX_ACTIONS] = 1 + index
 * of the symmetry applied that turn (0: none); az_game_rec.nodes / total_* are 0.
 * Benchmark.Duel players (src/benchmark.jl:124-192): Full = ResNet oracle, MctsRollouts = AZ_ORACLE_ROLLOUT,
 * NetworkOnly(tau) = an engine with num_iters_per_turn = 0 (NetworkPlayer, src/play.jl:226-235, under
 * PlayerWithTemperature(ConstSchedule(tau))): its moves carry the policy's Float32 bits in N[0..A) and
 * bit 8 of N[AZ_MAX_ACTIONS].  MinMaxTS = an engine after az_engine_set_minmax (below): no search, think()'s pi as Float32
 * bits in N[0..A), bits 8 and 9 (0x300) of N[AZ_MAX_ACTIONS] beside the symmetry index; either side may be one. */
int az_arena_run(az_engine* contender, az_engine* baseline, int32_t num_games, int32_t first_game_id,
                 int32_t alternate_colors, az_trace_buf* out, double* rewards, double* redundancy,
                 az_progress_cb cb, void* user);

/* ---- MinMax player (Benchmark.MinMaxTS, src/benchmark.jl:179-194 -> MinMax.Player, src/minmax.jl:14-114) ------------------
 * The baseline that needs neither a network nor MCTS: an exhaustive depth-limited tree walk on the device (csrc/minmax.hip).
 * Contract, operation by operation; every Float64 step is ONE IEEE operation (no contraction), so results are defined bit
 * for bit.  As with every other "bit-exact" of this project this is parity with THIS restatement and its CPU twin
 * (tests/minmax_ref.py): the reference itself has never been run against it (no Julia where this was written) -- unpinned.
 *   value(game, d)       (minmax.jl:17-26)  0. if game_terminated; heuristic_value(game) if d == 0; else maximum of
 *                        qvalue(game, a, d) over the available actions (Julia's max: -0.0 < 0.0).
 *   qvalue(game, a, d)   (minmax.jl:28-42)  next = play!(clone(game), a); wr = white_reward(next); r = white_playing(game) ? wr :
 *                        -wr (so a BLACK mover's zero reward is -0.0); with amplify_rewards a non-zero r becomes Inf * sign(r)
 *                        (minmax.jl:14); nextv = value(next, d - 1), negated ONLY IF the player to move changed (Mancala's
 *                        extra turns do not negate; negating a terminal child's 0. gives -0.0 and that is what is added);
 *                        q = r + gamma * nextv: one multiplication, one addition.
 *   heuristic_value      Connect Four (games/connect-four/game.jl:174-220): mine - yours; each side the sequential
 *                        left-to-right sum, from the first term, over the 69 alignments in the order axes (1,1), (1,-1), (0,1),
 *                        (1,0), within an axis x outer 1..7, y inner 1..6 (alignments that leave the board dropped); an alignment
 *                        holding a stone of the other side gives 0., else 0.1^(3 - N) for N own stones, from the table {1.0, 0.1,
 *                        0.1*0.1, (0.1*0.1)*0.1} (= the correctly rounded powers 0.010000000000000002, 0.0010000000000000002).
 *                        Tic-tac-toe (games/tictactoe/game.jl:43-51,98-120): the same with 0.3^(2 - N), table {1.0, 0.3,
 *                        0.3*0.3}, alignments (0,3,6) (1,4,7) (2,5,8), (0,1,2) (3,4,5) (6,7,8), (0,4,8), (2,4,6).
 *                        Mancala (games/mancala/game.jl:213-218): Float64(store of the mover - store of the other side).
 *                        The order shows in the last bits (Connect-Four opening, depth 5: 0.27000000000000013 for columns 3 and
 *                        4 counted from 1, 0.27 for column 5) and those bits decide ties at tau = 0.
 *   think                (minmax.jl:87-114) pi over the available actions: some q == +Inf -> 1 on those, 0 elsewhere; else every
 *                        q == -Inf -> all 1; else tau == 0 -> 1 on every q == the maximum; else C = max |q| over the q > -Inf +
 *                        eps(Float64), pi = az_exp((q - qmax) / C) with an explicit 0 for q == -Inf, then az_pow(pi, 1 / tau);
 *                        finally every entry divided by the sequential sum.
 *   move                 the default select_move (src/play.jl:48-53): player_temperature is 1.0 whatever the engine's temperature
 *                        schedule says, then fix_probvec + rand_categorical with the AZ_RNG_MOVE stream of (seed, game id, move).
 * The walk is exhaustive like the reference's (no pruning): max and negation are exact, so only the leaf heuristic and
 * r + gamma * v round and the result does not depend on how the tree is split over the device. */
#define AZ_MINMAX_MAX_DEPTH 9          /* 9 solves Tic-tac-toe */
typedef struct {
  int32_t struct_size;        /* sizeof(az_minmax_cfg), set by az_minmax_cfg_init */
  int32_t depth;              /* 1..AZ_MINMAX_MAX_DEPTH */
  int32_t amplify_rewards;
  int32_t reserved;           /* 0 */
  double tau;                 /* >= 0, finite */
  double gamma;               /* > 0, finite */
} az_minmax_cfg;
int az_minmax_cfg_init(az_minmax_cfg* cfg);                 /* depth 5, amplify 0, tau 0, gamma 1 */
/* GI.heuristic_value(GI.init(gspec, s)) for n states, on the device */
int az_game_heuristic(az_engine* e, const uint64_t* keys, int32_t n, double* h);
/* [qvalue(p, game, a, p.depth) for a] by FULL action index (Q: n*num_actions, unavailable: NaN) and, if pi != NULL, think()'s pi
 * (n*num_actions, unavailable: 0) for n non-terminal states, on the device; a terminated state is AZ_ERR_BAD_ARG naming its
 * index and nothing is launched.  The configuration is checked before the engine; n = 0 is AZ_OK. */
int az_minmax_qvalues(az_engine* e, const az_minmax_cfg* cfg, const uint64_t* keys, int32_t n, double* Q, double* pi);
/* think()'s pi from the n q-values of the available actions: pure host, no engine (the function az_arena_run and
 * az_minmax_qvalues use); 1 <= n <= AZ_MAX_ACTIONS, no NaN */
int az_minmax_policy(const double* q, int32_t n, double tau, double* pi);
/* From now on az_arena_run treats this engine as MinMax.Player(cfg) (its oracle, search parameters and temperature schedule are
 * not consulted); NULL = an MCTS / network player again.  While it is one, az_selfplay_begin / az_selfplay_run and
 * az_mcts_explore return AZ_ERR_STATE.  AZ_ERR_BAD_ARG for a depth outside 1..AZ_MINMAX_MAX_DEPTH, tau < 0 or not finite,
 * gamma <= 0 or not finite, a wrong struct_size, and AZ_GAME_GO9_PLANES (no device twin). */
int az_engine_set_minmax(az_engine* e, const az_minmax_cfg* cfg);

/* ---- Connect Four solver (Solver.Player, games/connect-four/solver.jl:17-99; the judge of scripts/pons_benchmark.jl) --------
 * The reference pipes every position to an external program (Pascal Pons' solver) that it does not ship.  Here the exact search
 * runs on the device (csrc/solver.hip): alpha-beta to the end of the game over bitboards, one query per lane, without
 * (az_c4_solve) or with (az_c4_solve_table) a transposition table.  This is parity
 * with the scores the reference ships (the second column of games/connect-four/benchmark/Test_L*_R*), not with a run of the
 * reference: its solver has never been executed against this one.
 *   score                (solver.jl:58-89) Pons' convention, seen from the player to move: 0 a draw, +k he wins with his k-th stone
 *                        counted from his last (22 - the stones he has played when he connects four), -k the opponent does.
 *   value(game)          a terminal game: 0 for a full board, else remaining_stones(winner) + 1 = 22 - the winner's stones,
 *                        negated because the side to move is the one that lost; otherwise the maximum of qvalue over the available
 *                        actions (what the external solver answers).
 *   qvalue(game, a)      next = play!(clone(game), a); -value(next) (the turn always changes).  A child that ends the game takes
 *                        value's terminal branch: 0 for a full board, 21 - nstones / 2 (integer division, = (43 - nstones) / 2) for
 *                        the mover who connects four with nstones on the board before his move.
 *   query                one (state, action); a state is at most 7 of them, searched independently, each with its own node_budget.
 *   strong / weak        weak = 0: exact scores.  weak != 0: only their sign, -1 / 0 / 1 (all the Pons benchmark needs): the same
 *                        null-window passes, stopped as soon as the sign is known.
 *   node_budget          nodes one search may enter.  A child that is terminal, or whose mover wins with his next stone, is
 *                        decided without a node.  Every other child is searched: a position counts as a node each time it is
 *                        entered (only once its mover is known to have no winning move; it returns at once where every move
 *                        loses to the opponent's next stone or two cells are left), and the search closes in on the score with
 *                        null-window passes from the child, so the child itself is entered once per pass.  A query whose search
 *                        would enter more than node_budget nodes comes back AZ_SOLVER_UNSOLVED.  A solved query is exact,
 *                        whatever the budget: a number that might be wrong is never returned.
 *   value with unsolved  the maximum of the solved q is still the state's value if every unsolved move is PROVEN to be no better.
 *   moves                In weak mode a solved +1 proves that.  Otherwise each unsolved query gets a second search that only asks
 *                        whether its q exceeds the best solved one, again with node_budget nodes: the expensive moves are mostly
 *                        the bad ones beside a quick win, whose exact score nobody needs.  The q of such a move stays
 *                        AZ_SOLVER_UNSOLVED; only value[] profits.
 *   determinism          az_c4_solve ONLY: the outputs for a state depend on (state, cfg) alone -- not on the rest of the batch, on
 *                        earlier calls or on timing: it has no transposition table, no state is kept between calls, and what the
 *                        lanes of a state exchange is that state's own results.  Node counts are reported for information and are
 *                        not part of the contract.  az_c4_solve_table gives this up for reach: see "table" below.
 *   table                az_c4_solve_table searches with a transposition table (az_solver_table) that every lane of the call reads
 *                        and writes, and that stays filled for the next call, and tries the moves in the order of the threats
 *                        they create.  EXACT OR UNSOLVED holds as it does without one: a solved q or value is exact whatever the
 *                        table held when the call began and whoever else was writing to it meanwhile (an entry carries the whole
 *                        key of its position, says something that is true of that position alone -- for any window, mode, budget
 *                        and caller -- and is read and written as one 64-bit word); AZ_SOLVER_UNSOLVED otherwise.  WHICH queries
 *                        come in under node_budget, and the node counts, are no longer fixed: they depend on the table's contents
 *                        (its size, earlier calls, the rest of the batch) and on timing.  A position that was solved may, with
 *                        another table or at another time, come back unsolved and the other way round; two solved answers for
 *                        one position never differ.  Terminal states, children decided without a node, AZ_SOLVER_NA and the
 *                        argument checks are those of az_c4_solve.
 *   think                (solver.jl:91-99) pi uniform over the available actions whose q equals the maximum, 0 elsewhere.
 * The solver is not an arena player (no az_engine_set_solver): a duel starts on the empty board, which no per-move search reaches
 * without an opening book -- the reference's own solver needs minutes there. */
#define AZ_SOLVER_NA (-128)            /* q of a full column, and every q of a terminal state */
#define AZ_SOLVER_UNSOLVED 127         /* the query needs more than node_budget nodes */
/* Default budget, chosen from tools/solver_bench.py on an MI355X (profiles/solver/): at 2^20 nodes per query a call
 * over 1000 positions takes at most about 3 s whichever Pons set it is, the end / easy and middle / easy sets get every value, and
 * the others as far as a search without a transposition table goes (middle / medium 75 %, beginning / easy 96 %, beginning /
 * medium 6 %, beginning / hard 0 % of the values).  2^16 is 16 times quicker but loses half of middle / medium; 2^23 costs 11-23 s
 * a call for a few per cent more.  az_c4_solve_table takes the same default: with a table of 2^23 entries it gets every value of
 * middle / medium and beginning / easy and 66 % of beginning / medium's (profiles/solver/solver_sets_table.json), at 11-28 s a call
 * where lanes run out of budget, because a node costs more there; the budget still is what bounds a call. */
#define AZ_SOLVER_DEFAULT_BUDGET (1LL << 20)
typedef struct {
  int32_t struct_size;        /* sizeof(az_solver_cfg), set by az_solver_cfg_init */
  int32_t weak;               /* 0: exact scores, else their sign */
  int64_t node_budget;        /* > 0, per query */
} az_solver_cfg;
int az_solver_cfg_init(az_solver_cfg* cfg);                 /* strong, AZ_SOLVER_DEFAULT_BUDGET */
/* Solver.value and Solver.qvalue of n Connect-Four states, on the device.  q: n*7 by FULL action index, AZ_SOLVER_NA for a full
 * column, AZ_SOLVER_UNSOLVED for a query over budget.  value[i]: the maximum of q[i], or AZ_SOLVER_UNSOLVED if one of them is
 * unsolved -- unless the solved ones already prove the maximum ("value with unsolved moves" above).  A terminal state gets value's terminal
 * branch and q all AZ_SOLVER_NA.  nodes (n, or NULL): nodes searched below the state's queries.  The configuration is checked
 * before the engine; AZ_ERR_BAD_ARG for a NULL cfg or buffer, a wrong struct_size, node_budget <= 0, n < 0 and an engine of
 * another game (the message names it); n = 0 is AZ_OK. */
int az_c4_solve(az_engine* e, const az_solver_cfg* cfg, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q, int64_t* nodes);
/* The transposition table of az_c4_solve_table: 2^log2_entries entries of 8 bytes in the memory of `device`, zeroed (empty).  It
 * belongs to the caller, as an az_memory does, and is tied to no engine, call or mode: any engine of its device may be given it, in
 * strong and weak calls in any order, and what one call learns the next one finds -- the 7000 queries of a Pons set are positions of
 * the same few openings.  log2_entries 0..30 (AZ_ERR_BAD_ARG outside; 23 = 64 MB is what the Python host takes); a table of one
 * entry is legal and merely replaces on every store.  clear empties it.  info: any of the three pointers may be NULL; occupied =
 * the entries that are not empty, counted on the device when asked for.  destroy(NULL) is AZ_OK.  No call that uses a table may
 * run while it is cleared or destroyed. */
typedef struct az_solver_table az_solver_table;
int az_solver_table_create(int32_t device, int32_t log2_entries, az_solver_table** out);
int az_solver_table_destroy(az_solver_table* t);
int az_solver_table_clear(az_solver_table* t);
int az_solver_table_info(az_solver_table* t, int32_t* log2_entries, int64_t* bytes, int64_t* occupied);
/* az_c4_solve with the table `t` ("table" above): the same outputs, the same argument checks in the same order, and after the
 * engine's game AZ_ERR_BAD_ARG for a NULL table and for a table of another device than the engine's (the message names both).
 * Exact or unsolved as az_c4_solve; which queries finish within node_budget, and nodes[], depend on the table and on timing. */
int az_c4_solve_table(az_engine* e, const az_solver_cfg* cfg, az_solver_table* t, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q,
                      int64_t* nodes);
/* think()'s pi from the q-values by FULL action index (AZ_SOLVER_NA: unavailable, pi 0): pure host, no engine.
 * AZ_ERR_BAD_ARG if an entry is AZ_SOLVER_UNSOLVED, or n_actions outside 1..AZ_MAX_ACTIONS. */
int az_solver_policy(const int8_t* q, int32_t n_actions, double* pi);

/* push_trace! (src/memory.jl:74-87): z (discounted, side relative) and t per move record. */
int az_push_trace(const az_move_rec* moves, int32_t n, double gamma, double* z, double* t);

/* Device-only phase: az_selfplay_run with out->moves == NULL keeps the move records in HBM (the engine's phase buffer) and
 * returns the game records only (first_move = -1); az_memory_push_engine / az_comm_gather_push consume them there. */

/* ---- replay memory (src/memory.jl) and learning status (src/learning.jl) on the device ---- */
typedef struct az_memory az_memory;      /* MemoryBuffer (src/memory.jl:34-45): circular buffer of samples in HBM */
typedef struct az_dataset az_dataset;    /* Trainer's converted data (src/learning.jl:98-121), device resident */
/* TrainingSample (src/memory.jl:20-26); pi by FULL action index (0 where the action is unavailable). 112 bytes. */
typedef struct {
  uint64_t key[2];
  double pi[AZ_MAX_ACTIONS];
  double z, t;
  int64_t n;
} az_sample;
typedef enum { AZ_WEIGHT_CONSTANT = 0, AZ_WEIGHT_LOG = 1, AZ_WEIGHT_LINEAR = 2 } az_weighing_policy;   /* params.jl:177 */
int az_memory_create(int32_t game, int32_t device, int64_t capacity, az_memory** out);
int az_memory_destroy(az_memory* m);
/* push_trace!(mem, trace, gamma) (src/memory.jl:74-87) for every game of `traces` in buffer order: one sample
 * per move record, pi = MCTS.policy of the recorded visit counts, z / t as az_push_trace. */
int az_memory_push(az_memory* m, const az_trace_buf* traces, double gamma);
/* self_play_step!'s push loop (src/training.jl:284-299) without the host hop: push_trace!(mem, trace, gamma) for every game
 * of the engine's last bounded self-play phase (az_selfplay_run, or az_selfplay_begin with num_games > 0), in game-id
 * order, reading the move records from the engine's device-resident phase buffer. */
int az_memory_push_engine(az_memory* m, az_engine* e, double gamma);
/* push!(mem.buf, sample) for samples that live on the host (a reference-side MemoryBuffer, a game-stage subset of
 * memory_report, src/learning.jl:192-216); does not advance cur_batch_size. */
int az_memory_push_samples(az_memory* m, const az_sample* samples, int64_t n);
int az_memory_length(az_memory* m, int64_t* length, int64_t* cur_batch_size);   /* length, cur_batch_size (:53-59) */
int az_memory_new_batch(az_memory* m);                                            /* new_batch! (:55) */
int az_memory_empty(az_memory* m);                                                /* empty! (:57-60) */
/* The data of a Trainer: which = 0 get_experience / 1 last_batch (:47-51); use_symmetries =
 * augment_with_symmetries (:116-138, applied by learning_step!, src/training.jl:199-202) ; use_position_averaging =
 * merge_by_state (:98-114; samples of a state are averaged in buffer order, output sorted by key);
 * convert_samples (src/learning.jl:17-51) with the weighing policy.  Everything stays on the device. */
int az_dataset_create(az_memory* m, int32_t which, int32_t use_symmetries, int32_t use_position_averaging,
                      int32_t weighing_policy, az_dataset** out);
/* The data of a Trainer from tensors the caller converted itself (convert_samples, src/learning.jl:17-51): a host that steps its own
 * game and keeps its samples itself -- any GameInterface game of a supported geometry, AZ_GAME_GO9_PLANES included; az_plane_memory below
 * keeps them on the device instead -- or one that labels positions by other means.  Host arrays, sample index first: W [n], X [n][C][H][W] (the layout of az_net_forward), A [n][nA],
 * P [n][nA], V [n] (the layouts az_dataset_read writes).  AZ_ERR_BAD_ARG with the first offending sample in az_last_error() for n < 1,
 * a NULL pointer, a non-finite value, W <= 0, an entry of A outside {0, 1}, a row of A without a legal action, P < 0, or P > 0 where
 * A == 0 (the loss takes the logarithm of the masked network policy there).  Wtot, Wmean and Hp = entropy_wmean(P, W)
 * (src/learning.jl:63,111) are computed on the device; num_samples = sum_n = n.  No az_sample records stand behind such a data set. */
int az_dataset_create_from_tensors(int32_t game, int32_t device, int64_t n, const float* W, const float* X, const float* A,
                                   const float* P, const float* V, az_dataset** out);
int az_dataset_destroy(az_dataset* d);
typedef struct {
  int64_t num_samples;   /* length(samples) after symmetries / merging (= num_boards when merged) */
  int64_t sum_n;         /* sum(e.n), Report.Samples.num_samples (src/learning.jl:186) */
  double Wtot;           /* sum(W) */
  float Wmean, Hp;       /* mean(W), entropy_wmean(P, W) (src/learning.jl:110-111) */
} az_dataset_info;
int az_dataset_get_info(az_dataset* d, az_dataset_info* out);
/* samples / tensors [first, first+count) to host buffers (any pointer may be NULL): W [n], X [n][C][H][W]
 * (= Julia WHCN memory), A [n][nA], P [n][nA], V [n].  A data set made from tensors has no samples: AZ_ERR_BAD_ARG if `samples` is
 * not NULL. */
int az_dataset_read(az_dataset* d, int64_t first, int64_t count, az_sample* samples, float* W, float* X, float* A,
                    float* P, float* V);
/* learning_status(tr) (src/learning.jl:158-181): `losses` (:67-90) per batch of loss_computation_batch_size samples
 * (partial last batch kept) with the engine's network in test mode, batches weighted by their total weight. */
typedef struct { float L, Lp, Lv, Lreg, Linv, Hp, Hpnet; } az_learning_status_t;   /* Report.LearningStatus */
int az_learning_status(az_engine* e, az_dataset* d, double l2_regularization, double nonvalidity_penalty,
                       double rewards_renormalization, int64_t loss_computation_batch_size, az_learning_status_t* out);

/* ---- replay memory of plane samples: MemoryBuffer (src/memory.jl) for a host-stepped game ----------------------------------
 * az_memory stores state keys and re-encodes them with the game's device twin.  A game whose rules live on the host -- any
 * GameInterface game of a supported geometry, AZ_GAME_GO9_PLANES above all -- has no twin, so this memory stores what the host can
 * give: per sample the planes X [C][H][W] (Float32, the layout of az_net_forward) and the mask A [nA] (Float32 in {0, 1}) the
 * network sees, pi [nA] (Float64, by FULL action index), z, t (Float64) and n (Int64).  A circular buffer in HBM with
 * MemoryBuffer's semantics (memory.jl:35-65): a push over capacity overwrites the oldest sample, cur_batch_size = min(samples
 * pushed by push_trace since new_batch, length).  All four geometries are accepted.
 *   state identity       The device never sees the host's state: two samples are ONE state when their (X, A) rows are bit-identical
 *                        (0.0 and -0.0 differ), which is what the network can tell apart.  For a game whose vectorize_state is
 *                        injective this is merge_by_state's grouping (memory.jl:98-112); otherwise it groups more.
 *   merging              pi, z, t of a merged row are the sums over its samples, accumulated one by one in buffer order in Float64
 *                        starting from the first, divided by the count (the order az_dataset_create keeps); n is the sum.  Rows
 *                        come out in the order of each state's first occurrence in the buffer (the reference's values(dict) order
 *                        is unspecified); without merging in buffer order.
 *   hashing              Rows are brought together by a 128-bit hash and then compared word by word; a hash never decides that
 *                        two rows are equal.  Two different rows with one hash make the call fail with AZ_ERR_STATE ("plane hash
 *                        collision"); rows are never merged wrongly or split silently.
 *   convert_samples      (learning.jl:17-51) W from n by the weighing policy as az_dataset_create computes it, X / A the first
 *                        sample's of the state, P = Float32(pi), V = Float32(z).  t stays in the memory: a data set does not carry it. */
typedef struct az_plane_memory az_plane_memory;
int az_plane_memory_create(int32_t game, int32_t device, int64_t capacity, az_plane_memory** out);   /* capacity 1..2^31-1 */
int az_plane_memory_destroy(az_plane_memory* m);
/* push!(mem.buf, e) for n samples on the host, sample index first: X [n][C][H][W], A [n][nA], P [n][nA] (= pi), z [n], t [n], nvis [n]
 * (= n of each sample; NULL: 1).  Does not advance cur_batch_size (as az_memory_push_samples).  Checked on the device before
 * anything is stored: AZ_ERR_BAD_ARG with the first offending sample in az_last_error() for a non-finite value, nvis < 1, an entry
 * of A outside {0, 1}, a row of A without a legal action, P < 0, or P > 0 where A == 0; the memory is then unchanged.  n = 0 is AZ_OK. */
int az_plane_memory_push_samples(az_plane_memory* m, int64_t n, const float* X, const float* A, const double* P, const double* z,
                                 const double* t, const int64_t* nvis);
/* push_trace!(mem, trace, gamma) (memory.jl:74-87) for ONE game of len positions in playing order: rewards[i] is white's reward
 * after move i, white_playing[i] != 0 where white is to move in position i.  Samples are pushed for i = len .. 1 (counted from 1), in
 * that order: wr = gamma * wr + rewards[i], z = white_playing[i] ? wr : -wr, t = len - i + 1, n = 1; cur_batch_size += len.  The
 * checks of az_plane_memory_push_samples apply (sample = position, counted from 0), rewards and gamma must be finite. */
int az_plane_memory_push_trace(az_plane_memory* m, int32_t len, const float* X, const float* A, const double* P, const double* rewards,
                               const uint8_t* white_playing, double gamma);
/* Samples [first, first + count) of the buffer, oldest first, to host arrays in the layouts of az_plane_memory_push_samples (any
 * pointer may be NULL): what get_experience returns, e.g. to slice the samples by t (memory_report) or to save the memory. */
int az_plane_memory_read(az_plane_memory* m, int64_t first, int64_t count, float* X, float* A, double* P, double* z, double* t, int64_t* nvis);
int az_plane_memory_length(az_plane_memory* m, int64_t* length, int64_t* cur_batch_size);   /* length, cur_batch_size (:53-59) */
int az_plane_memory_new_batch(az_plane_memory* m);                                            /* new_batch! (:55) */
int az_plane_memory_empty(az_plane_memory* m);                                                /* empty! (:57-60) */
/* The data of a Trainer from the memory, built on the device: which = 0 get_experience / 1 last_batch, use_position_averaging =
 * merge_by_state over rows ("state identity", "merging" above), convert_samples with the weighing policy.  The result is the kind of
 * data set az_dataset_create_from_tensors makes (no az_sample records; Wtot, Wmean and Hp computed by the same code) and owns its
 * memory: the az_plane_memory may be pushed to or destroyed afterwards.  num_samples = rows after merging, sum_n = sum of n.
 * AZ_ERR_STATE when there is no sample to take (an empty memory; which = 1 with an empty batch) and for a hash collision. */
int az_dataset_create_from_plane_memory(az_plane_memory* m, int32_t which, int32_t use_position_averaging, int32_t weighing_policy,
                                        az_dataset** out);
#define AZ_PLANE_MAX_SYMMETRIES 15
/* GI.symmetries for a memory whose game lives on the host: nsym non-identical symmetries, each a pair of gather permutations
 *   X'[w] = X[xperm[k][w]]  (w over the C*H*W words of a sample's planes, layout of az_net_forward)
 *   A'[j] = A[aperm[k][j]], pi'[j] = pi[aperm[k][j]]   (game.jl:192 "mask2 == mask1[sigma]", memory.jl:119)
 * z, t, n are the sample's.  nsym = 0 (pointers may be NULL) clears them.  The symmetries belong to the game, not to the samples: the
 * call may come at any time, on an empty or a full memory, and nothing is stored per sample.  AZ_ERR_BAD_ARG for nsym outside
 * 0..AZ_PLANE_MAX_SYMMETRIES, a NULL table with nsym > 0, and any row that is not a bijection of its range (az_last_error() names the
 * symmetry, the table and the first offending index: out of range, or a source that an earlier index already took); the set declared
 * before is then unchanged.  An identity permutation is not refused (the reference does not refuse one either). */
int az_plane_memory_set_symmetries(az_plane_memory* m, int32_t nsym, const int32_t* xperm /*[nsym][C*H*W]*/, const int32_t* aperm /*[nsym][nA]*/);
int az_plane_memory_num_symmetries(az_plane_memory* m, int32_t* nsym);
/* az_dataset_create_from_plane_memory with augment_with_symmetries (memory.jl:114-130) in front of the merge.  use_symmetries == 0: exactly
 * that call.  Otherwise the n0 selected samples (oldest first) become the sequence [samples ; images] of n1 = n0 * (1 + nsym) rows,
 * image k of sample i at buffer index n0 + i * nsym + k, and everything promised above ("state identity", "merging", "hashing",
 * "convert_samples") holds over that sequence in that buffer order; num_samples = rows after merging, sum_n = (1 + nsym) * sum of n.
 * The images are never stored: every kernel reads them through the permutations.  AZ_ERR_BAD_ARG when use_symmetries != 0 and no
 * symmetries were declared for this memory (game.jl:332), and when n1 > 2^31 - 1. */
int az_dataset_create_from_plane_memory_sym(az_plane_memory* m, int32_t which, int32_t use_symmetries, int32_t use_position_averaging,
                                            int32_t weighing_policy, az_dataset** out);

/* ---- device search trees for a host-stepped game: MCTS.Env (src/mcts.jl:124-226) whose rules the caller owns --------------------
 * W independent per-worker trees in HBM.  The device selects, expands, backs up and looks transpositions up; the host is asked at
 * most one question per simulation -- "play this action in this node's state" -- and answers with the key, the reward and, for a
 * state the worker has not met, what the network sees of it.  An edge that has been walked once is remembered (child node or
 * terminal, the mover's reward, whether the player changed), so the rules are consulted once per (state, action) and worker.
 *   oracle        engine mode (e != NULL: a ResNet engine with its parameters set, num_actions == the engine's): the rows of the
 *                 non-terminal replies are evaluated by the engine's network on the device, in reply order, in ONE launch of the
 *                 seam az_net_forward uses; P / V never leave the device.  Host-oracle mode (e == NULL): the caller supplies P (full
 *                 width) and V with each non-terminal reply (MCTS.RandomOracle-style players; exact tests without a network).
 *   state key     128 bits the host chooses; both words are compared.  Two states with one key are the caller's affair, as with a Dict.
 *   node          by RANK among the available actions (mcts.jl:78-87): P (Float32), W (Float64), N (Int32), the action id, and the
 *                 memo of the edge: child node, terminal flag, the mover's reward (Float64 of the Float32 given), pswitch; per node
 *                 Vest and white_playing.  Node ids count from 0 per worker in creation order; az_host_tree_reset restarts them.
 *   scores        (mcts.jl:180-188) Ntot = sum N (integer); s = sqrt(Float64(Ntot)); Q = W / Float64(max(N, 1)); Pd = Float64(P), at the
 *                 root (empty path) with eps != 0: Pd = (1 - eps) * Pd + eps * eta[rank]; score = Q + ((cpuct * Pd) * s) / Float64(N + 1);
 *                 the first maximum is taken.  Every step is one IEEE Float64 operation, no contraction.
 *   noise         eta = az_dirichlet over the root's n with the stream (seed, game id, move, AZ_RNG_NOISE) of az_numerics.h, drawn on
 *                 the device the first time the root is selected from after an az_host_tree_explore; not drawn when eps == 0.
 *   backup        (mcts.jl:216-223) a new node's value is q = Float64(Vest), a terminal state's 0.0; then, last path entry first:
 *                 qn = pswitch ? -q : q; q = r + gamma * qn; W += q; N += 1.
 *   protocol      az_host_tree_explore arms workers with a quota of simulations; every az_host_tree_step absorbs the replies to the
 *                 requests of the step before (same order: worker order, compacted) and carries every armed worker to its next
 *                 request or to the end of its quota, in one call with one synchronisation.  A reply to AZ_HT_PLAY describes the
 *                 state after the move: terminal -> the simulation is backed up with 0.0; a key the worker's table holds -> the edge
 *                 is linked to that node (a transposition; an evaluation made for it is discarded and counted) and the simulation
 *                 goes on from there in the same step, as run_simulation! would; otherwise the node is created and the simulation
 *                 backed up.  Edges known to lead to a node are descended, edges known to be terminal finish the simulation on the
 *                 device.  A worker whose root is unknown (first explore, after a reset, after an advance along an unwalked edge)
 *                 asks AZ_HT_ROOT: describe the root state; a new root's first simulation returns Vest, as in the reference.
 *   requests      {worker, node, action (full index), kind}.  AZ_HT_FULL (node pool or edge pool exhausted) and AZ_HT_DEPTH (the path
 *                 would exceed max_depth) are reports, not questions: the simulation is abandoned, nothing of it is stored or backed
 *                 up, the worker is disarmed, other workers are untouched, and no reply is given for them.  new_nodes[i] = the node
 *                 reply i created or was linked to (-1 for a terminal reply, and where the pools were exhausted).
 *   refusals      checked before anything is stored, az_last_error() names the offender: a reply count other than the outstanding
 *                 requests', a non-finite reward or V, a terminal root, an A row with no legal action or entries outside {0, 1},
 *                 P < 0 or not finite or P > 0 where A == 0 (host-oracle mode), a worker index out of range, az_host_tree_explore
 *                 on an armed worker (or naming one twice), root_stats / advance / reset on an armed worker (AZ_ERR_STATE), an
 *                 advance by an action the root does not have, a bit of az_host_tree_cfg.flags nobody defined (az_host_tree_create
 *                 names it).  The tree is unchanged and the outstanding requests stay outstanding.
 *   chance        flags & AZ_HOST_TREE_CHANCE: a game whose play! may give another state every time it is called (a stochastic MDP,
 *                 games/grid-world), searched as mcts.jl:199-226 searches it: the rules are consulted at every ply of every
 *                 simulation, the statistics stay per (state, action), and the backup runs along the states actually met.
 *                 protocol: no edge is ever remembered; every descent through an edge ends the step with AZ_HT_PLAY, one ply per
 *                 step, request.node = the node of the state the simulation stands in.  reply: the state reached THIS time; the
 *                 mover's reward (white_playing of the node ? wr : -wr, Float64 of the Float32) and pswitch (the node's white_playing
 *                 != the reply's) belong to this path entry, not to the edge.  Terminal -> backed up with 0.0; a key the worker's
 *                 table holds -> the descent goes on from that node in the same step (its evaluation is discarded and counted in
 *                 transposition_hits); otherwise the node is created and backed up with Float64(Vest).  backup: the same recurrence
 *                 with the entry's r and pswitch; an edge may stand on one path several times with different rewards, and is then
 *                 updated one entry at a time, last entry first.  advance: the device cannot know where the real move led, so the
 *                 root becomes unknown (the action must still be one the root has) and the tree is kept; the next explore asks
 *                 AZ_HT_ROOT and the reply's key finds the node if the worker has met that state -- the tree is reused as the
 *                 reference reuses env.tree.  AZ_HT_FULL, AZ_HT_DEPTH, the noise at the root and the refusals are those above;
 *                 sims_without_host counts only simulations that never asked.  Cost: one host round trip per ply, and every
 *                 non-terminal reply's row is evaluated although most land on nodes the worker knows.
 * Not built, in either mode: prior_temperature != 1 (refused by az_host_tree_create), more than AZ_HOST_TREE_MAX_ACTIONS actions,
 * freeing the subtrees an advance leaves unreachable (the tree is kept, as the reference keeps it between the moves of a game).
 * Not built in chance mode: outcome lists sampled on the device, skipping the evaluation of a reply that lands on a known node. */
#define AZ_HOST_TREE_MAX_ACTIONS 128
#define AZ_HOST_TREE_CHANCE 1   /* az_host_tree_cfg.flags: "chance" above */
typedef struct az_host_tree az_host_tree;
typedef struct {
  int32_t struct_size;        /* sizeof(az_host_tree_cfg), set by az_host_tree_cfg_init */
  int32_t flags;              /* 0, or AZ_HOST_TREE_CHANCE; any other bit is refused */
  double gamma, cpuct, dirichlet_noise_eps, dirichlet_noise_alpha;   /* MctsParams (src/params.jl:49-57) */
  double prior_temperature;   /* must be 1 */
  uint64_t seed;
} az_host_tree_cfg;
typedef enum { AZ_HT_PLAY = 0, AZ_HT_ROOT = 1, AZ_HT_FULL = 2, AZ_HT_DEPTH = 3 } az_host_tree_request_kind;
typedef struct { int32_t worker, node, action, kind; } az_host_tree_request;   /* AZ_HT_ROOT: node = action = -1 */
typedef struct {
  uint64_t key[2];            /* the state after the move (AZ_HT_PLAY) / the root state (AZ_HT_ROOT) */
  float white_reward;         /* GI.white_reward after the move; ignored for AZ_HT_ROOT */
  uint8_t terminal;           /* GI.game_terminated */
  uint8_t white_playing;      /* GI.white_playing of that state */
  uint8_t reserved[2];
} az_host_tree_reply;
typedef struct {
  int64_t simulations;            /* completed (src/mcts.jl:242) */
  int64_t nodes_traversed;        /* src/mcts.jl:222 */
  int64_t evaluations;            /* non-terminal replies = rows the oracle evaluated */
  int64_t transposition_hits;     /* of them: the key was already in the worker's table, the evaluation was discarded */
  int64_t sims_without_host;      /* simulations that began and ended on the device without a request */
  int64_t max_nodes, max_edge_slots, max_path;   /* high-water marks over the workers (they survive a reset) */
  int64_t steps;                  /* az_host_tree_step calls that launched */
} az_host_tree_stats;
int az_host_tree_cfg_init(az_host_tree_cfg* cfg);   /* flags 0, gamma 1, cpuct 1, eps 0, alpha 1, prior_temperature 1, seed 0 */
/* num_actions 1..AZ_HOST_TREE_MAX_ACTIONS, num_workers 1..2^20, nodes_per_worker >= 1, edge_slots_per_worker >= num_actions,
 * max_depth >= 1.  Engine mode: num_workers must not exceed what one network launch of the engine takes; the engine must outlive the
 * tree, and the tree uses the engine's stream.  `device` is ignored in engine mode (the engine's is taken). */
int az_host_tree_create(az_engine* e_or_null, int32_t device, int32_t num_actions, int32_t num_workers, int32_t nodes_per_worker,
                        int32_t edge_slots_per_worker, int32_t max_depth, const az_host_tree_cfg* cfg, az_host_tree** out);
int az_host_tree_destroy(az_host_tree* t);
/* MCTS.explore!(env, game, nsims) begins for n workers: each gets a quota of nsims >= 1 simulations and the noise stream of
 * (seed, game_ids[i], moves[i]).  Nothing runs until the next az_host_tree_step. */
int az_host_tree_explore(az_host_tree* t, int32_t n, const int32_t* workers, const uint32_t* game_ids, const uint32_t* moves, int32_t nsims);
/* One step ("protocol" above).  replies [nreplies]; X [nreplies][C][H][W] (engine mode only, the layout of az_net_forward), A
 * [nreplies][num_actions], P [nreplies][num_actions] and V [nreplies] (host-oracle mode only) are indexed by reply; the rows of
 * terminal replies are not read.  requests and new_nodes must hold num_workers entries; *nrequests = requests written. */
int az_host_tree_step(az_host_tree* t, int32_t nreplies, const az_host_tree_reply* replies, const float* X, const float* A, const float* P,
                      const float* V, az_host_tree_request* requests, int32_t* nrequests, int32_t* new_nodes);
/* The path length at which each outstanding request (AZ_HT_PLAY / AZ_HT_ROOT) of the last step was asked, in the order of the requests:
 * 0 for AZ_HT_ROOT and for a question about the root's own move ("this simulation starts"), k where k edges were walked before.  It
 * came with the step's output: no launch, no synchronisation.  *n = their number; AZ_ERR_CAPACITY when cap is below it.  Both modes.
 * A host whose environment carries more than the state (grid-world's time) needs it: a node id does not name an environment there. */
int az_host_tree_request_depths(az_host_tree* t, int32_t* depths, int32_t cap, int32_t* n);
/* tree[root] of n workers by FULL action index (unavailable: 0): N [n][num_actions], W, P, Vest [n], root_node [n] (-1 and zeros
 * where the root is unknown); any pointer may be NULL.  What MCTS.policy (mcts.jl:255-271) and the explorer need. */
int az_host_tree_root_stats(az_host_tree* t, int32_t n, const int32_t* workers, int32_t* N, double* W, float* P, float* Vest, int32_t* root_node);
/* The root becomes the child the edge `actions[i]` leads to if that is a known node, else unknown (chance mode: always unknown); the tree is kept. */
int az_host_tree_advance(az_host_tree* t, int32_t n, const int32_t* workers, const int32_t* actions);
int az_host_tree_reset(az_host_tree* t, int32_t n, const int32_t* workers);   /* MCTS.reset!: the tree is emptied, node ids restart at 0, counters are kept */
int az_host_tree_get_stats(az_host_tree* t, az_host_tree_stats* stats);

/* ---- the optimiser step (src/learning.jl:123-141, src/networks/flux.jl:68-95) --------------- */
typedef struct az_trainer az_trainer;   /* Trainer (src/learning.jl:98-121): network in train mode + optimiser state */
typedef enum { AZ_OPT_ADAM = 0, AZ_OPT_CYCLIC_NESTEROV = 1 } az_optimiser;   /* src/networks/network.jl:163-190 */
typedef struct {
  int32_t struct_size;        /* = sizeof(az_train_cfg), set by az_train_cfg_init */
  int32_t optimiser;          /* az_optimiser */
  float lr;                   /* Adam(lr) */
  float lr_base, lr_high, lr_low, momentum_low, momentum_high;   /* CyclicNesterov */
  double l2_regularization, nonvalidity_penalty, rewards_renormalization;   /* LearningParams, src/params.jl:235-248 */
  int32_t batch_size;         /* min(batch_size, #samples) is used (src/learning.jl:113) */
  float batch_norm_momentum;  /* ResNetHP.batch_norm_momentum (resnet.jl:30-37) */
  uint64_t seed;              /* batch shuffling (AZ_RNG_SHUFFLE) */
} az_train_cfg;
int az_train_cfg_init(az_train_cfg* cfg);
/* Trainer(gspec, network, samples, params): the engine supplies the architecture and the initial parameters, the
 * data set (az_dataset_create, az_dataset_create_from_tensors or az_dataset_create_from_plane_memory) the converted samples, Wmean
 * and Hp.  All four network geometries train, AZ_GAME_GO9_PLANES through a data set made from tensors or from a plane memory.  The engine's own network is not modified:
 * fetch the result with az_trainer_get_params and install it with az_net_set_params.  The engine and the data set
 * must outlive the trainer. */
int az_trainer_create(az_engine* e, az_dataset* d, const az_train_cfg* cfg, az_trainer** out);
int az_trainer_destroy(az_trainer* t);
/* batch_updates!(tr, n): n optimiser steps (forward in train mode = BatchNorm with batch statistics, `losses`,
 * backward, Adam / Nesterov with the L2 term, running statistics) on successive shuffled batches (DataLoader
 * partial = false, cycled); losses[i] = L of step i before its update (Network.train! callback).  Like the reference
 * (Flux.setup inside train!), every call starts from a fresh optimiser state; the batch stream continues. */
int az_trainer_batch_updates(az_trainer* t, int32_t n, float* losses);
int az_trainer_get_params(az_trainer* t, float* blob, int64_t n);   /* get_trained_network (src/learning.jl:127-129) */
/* Parity hook: loss and data gradient (Flux parameter order, running-statistics entries 0, L2 term excluded) of the batch
 * made of the given batch_size sample indices; no update, running statistics untouched.
 * parts (may be NULL) = Lp, Lv, Lreg, Linv, mean(W)/Wmean. */
int az_trainer_gradients(az_trainer* t, const int32_t* sample_idx, float* loss, float* parts, float* grad, int64_t n);

/* ---- multi-GPU exchange (simulate_distributed, src/simulations.jl:252-290; one process per GPU) ---------------------- */
/* RCCL over xGMI.  Self-play needs no communication (games are sharded by global game id: az_selfplay_run's
 * first_game_id); afterwards every rank's records are all-gathered device to device and pushed into the replay memory,
 * and new network parameters are broadcast before the next phase.  librccl.so is loaded on first use. */
#define AZ_COMM_ID_BYTES 128
typedef struct az_comm az_comm;
typedef struct {
  int64_t games, moves;             /* over all ranks */
  int64_t bytes;                    /* received per rank by the all-gathers */
  double gather_ms, total_ms;       /* pack + all-gathers + game-record read-back; plus the push into the memory */
  /* Report.SelfPlay's inputs over ALL ranks' games (src/training.jl:293-296): mean over games of average_exploration_depth,
   * the largest tree (nodes; x memory_footprint_per_node = mcts_memory_footprint), and the raw totals */
  int64_t ranks, total_simulations, total_nodes_traversed, max_nodes;
  double mean_game_depth;
  int64_t replaced_games;           /* gathered games whose id carries AZ_REPLACEMENT_GAME_BIT: games some rank aborted and played again.
                                     * Every rank sees the same number, so a host can apply its abort policy AFTER the collective and
                                     * fail on all ranks together (asked games - `games` = games given up for good) */
} az_gather_stats;
/* ncclGetUniqueId on ONE rank; the 128 bytes go to the other ranks by the host's own means (Distributed, MPI, a file). */
int az_comm_unique_id(uint8_t id[AZ_COMM_ID_BYTES]);
/* Which collective library az_comm_* bound: ncclGetVersion's code (e.g. 22105 = 2.21.5; 0 if the library does not say)
 * and the path of the shared object (librccl.so next to the HIP runtime, or AZHIP_RCCL_LIB).  No reference counterpart:
 * evidence for bench.py's `gather` object. */
int az_comm_version(int32_t* version, char* path, int32_t cap);
/* ncclCommInitRank: collective over all `world` ranks, each on its own device. */
int az_comm_init(int32_t device, int32_t rank, int32_t world, const uint8_t id[AZ_COMM_ID_BYTES], az_comm** out);
int az_comm_destroy(az_comm* c);
/* Collective.  A rank that cannot take part (no phase held, wrong device, allocation failure) still enters the first
 * all-gather with its status, and EVERY rank then returns an error together (the failing rank its own, the others
 * AZ_ERR_COMM) -- no rank is left waiting; a collective that fails half way aborts the communicator (later calls
 * return AZ_ERR_COMM).  All-gathers the ranks' device-resident phase records (the `fetch` + `vcat` of simulations.jl:280-289) and,
 * where `m` is not NULL, runs push_trace! (src/memory.jl:74-87) for ALL games in global game-id order into m: every rank
 * that passes a memory ends up with the same samples a single-GPU run of all the games would have pushed. */
int az_comm_gather_push(az_comm* c, az_engine* e, az_memory* m, double gamma, az_gather_stats* stats);
/* az_comm_gather_push for a host-stepped game: collective over all ranks of c (same failure agreement).  `src` is this rank's outbox:
 * its current batch is its newest B = sum(game_lens) samples, num_games consecutive runs in push order, run k being the game_lens[k]
 * (>= 1) samples of game game_ids[k] (>= 0) as az_plane_memory_push_trace stored them.  B must equal the raw count push_trace has
 * advanced since new_batch, and none of the batch may have been overwritten (B <= capacity); num_games = 0 with NULL arrays is a valid
 * contribution.  Game ids are global and must be distinct over all ranks.  Where `dst` is not NULL it ends up as if ONE process had
 * called az_plane_memory_push_trace on it for every game of every rank in ascending game id: the runs are appended in id order, the
 * samples of a run keep the order src stores them in (push_trace has already reversed them), every word of X, A, pi, z, t and n is
 * bit-identical, length and cur_batch_size advance by the total T over all ranks; when T exceeds dst's capacity only the newest
 * `capacity` samples are stored, and the ring wraps where it must.  dst == NULL takes part and stores nothing; src is never modified;
 * dst == src is refused.  src, dst and c must be on one device; src and dst must have one geometry, the same on every rank.
 * Symmetries belong to a memory and are not transported; samples are not checked again (they were when pushed).
 *   exchange   a sample travels device to device as one record of rb = 8 ceil(4 RW / 8) + 8 (nA + 2) + 8 bytes (RW = C*H*W + nA row
 *              words padded to 8 bytes, the doubles, n: 2304 bytes for 9x9 Go), in rounds of at most R rows per rank with
 *              W * R * rb <= 256 MiB of staging per rank; every rank runs ceil(max_r B_r / R) rounds.
 *   failures   every local reason to refuse (NULL src, wrong device, geometry, B mismatch, an overwritten batch, a length < 1, an
 *              id < 0) travels as a status word with the first all-gather, a failed allocation of the staging (sized by the largest
 *              rank) with a second one: the failing rank returns its own error, the others AZ_ERR_COMM naming the rank, nothing is
 *              exchanged and the communicator stays usable.  Ranks of different geometry: AZ_ERR_BAD_ARG on every rank.  A duplicate
 *              game id, on one rank or across ranks, is found after the game tables have been gathered: every rank returns
 *              AZ_ERR_BAD_ARG naming the id, and nothing is pushed anywhere.
 *   stats      games, moves (= samples), bytes, gather_ms (everything but the push into dst), total_ms and ranks; the tree fields
 *              and replaced_games are 0. */
int az_comm_gather_push_planes(az_comm* c, az_plane_memory* src, az_plane_memory* dst, const int32_t* game_ids, const int32_t* game_lens,
                               int32_t num_games, az_gather_stats* stats);
/* Collective (same failure agreement as az_comm_gather_push).  ncclBroadcast of `root`'s parameter blob, then az_net_set_params on every rank (the network shipped to the
 * workers before a phase, src/training.jl:278-282). */
int az_comm_broadcast_params(az_comm* c, az_engine* e, int32_t root);

/* ---- profiling (bench.py roofline): HIP-event time per kernel class ---------------------- */
#define AZ_PROF_NUM 8
typedef enum {
  AZ_K_SELECT = 0, AZ_K_COMPACT = 1, AZ_K_TOWER = 2, AZ_K_HEADS = 3,
  AZ_K_EXPAND = 4, AZ_K_MOVE = 5, AZ_K_SYNTH = 6, AZ_K_START = 7
} az_kernel_class;
typedef struct {
  int64_t launches[AZ_PROF_NUM];
  double ms[AZ_PROF_NUM];
  int64_t units[AZ_PROF_NUM];       /* boards (tower/heads) or slots processed (upper bound known to the host at launch) */
  double exec_units[AZ_PROF_NUM];   /* tower: sum over launches of units x the fraction of the 3x3 convolutions' (row tile, tap)
                                       products the kernel that ran really executes (the others fall off the board for a whole
                                       tile and are skipped); other classes: = units.  exec_units / units = the average executed
                                       fraction of the timed launches */
} az_prof;
int az_prof_enable(az_engine* e, int32_t on);   /* 1: wrap every launch in a HIP event pair; 1 | (mask << 1):
                                                   only the kernel classes whose bit is set in mask; 0: off */
int az_prof_get(az_engine* e, az_prof* out);    /* synchronises, accumulates, returns totals */
int az_prof_reset(az_engine* e);
int az_device_info(az_engine* e, char* name, int32_t name_cap, int32_t* num_cu, int64_t* hbm_bytes);
/* Name of the tower kernel the engine chose for its most recent network launch ("" before the first one): the
 * kernel is picked per launch size (choose_tower, csrc/tower_choice.h), bench.py reports the one that actually ran. */
int az_net_last_kernel(const az_engine* e, char* name, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* AZHIP_H */
