// eval_cache_rule.h -- the rules of the evaluation cache (tree.h ECEnt), written once for the kernel that looks and claims (k_tree)
// and the host that sizes the table (create_eval_cache).  Plain C++ (no device runtime, no engine.h): a host compiler builds it
// alone and sweeps it (tests/eval_cache_rule_driver.cpp; tests/test_eval_cache_rule_cpu.py holds it to a Python restatement).
//
// The table is two-way set-associative: a state hashes to a SET, the set's two 64-byte entries (2 set, 2 set + 1) are the two
// halves of ONE 128-byte line (hipMalloc aligns the base far beyond that), so a look fetches the line it always fetched and now
// uses all of it.
//   ec_set_of       the state's set
//   ec_checksum     what a READY entry's cs word must be
//   ec_way_hit      does this way answer the state: READY, above the floor, the state's key, the checksum
//   ec_pick_victim  which way a state that found no answer may claim for the one the network will give: 0, 1 or -1 (none)
//   ec_size_log2    log2 of the table's entries for an engine of G slots and `sims` simulations per move
// Hits are read-only (no use stamp, so a hit issues no store); replacement among two answered ways goes by the claim number: FIFO
// within a set.
#pragma once
#include <cstdint>

#include "../../include/az_numerics.h"

#ifdef __HIPCC__
#define EC_HD __host__ __device__ inline
#else
#define EC_HD inline
#endif

// meta = claim number << 2 | state; a claim number at or below the table's floor makes the entry EMPTY whatever its state says
enum { EC_EMPTY = 0, EC_PENDING = 1, EC_READY = 2, EC_FILLING = 3, EC_STALE_AFTER = 64 };
enum { EC_ENTRY_BYTES = 64, EC_WAYS = 2, EC_LINE_BYTES = EC_ENTRY_BYTES * EC_WAYS };

// the set of a state from its key hash (az_hash_key): other bits than the slot table's position (low) -- and than its tag where the mask allows
EC_HD uint32_t ec_set_of_hash(uint64_t hk, uint32_t set_mask) { return (uint32_t)(hk >> 17) & set_mask; }
EC_HD uint32_t ec_set_of(uint64_t ka, uint64_t kb, uint32_t set_mask) { return ec_set_of_hash(az_hash_key(ka, kb), set_mask); }

// px: the xor of the lanes' prior terms (tree.h ec_term); hk = az_hash_key of the entry's key; ready_meta: the READY value of the claim
EC_HD uint32_t ec_checksum(uint32_t px, uint64_t hk, float V, uint32_t ready_meta) {
  uint64_t h = az_mix64(hk ^ (((uint64_t)px << 32) | (uint64_t)az_f2u(V)));
  h = az_mix64(h + (uint64_t)ready_meta);
  return (uint32_t)(h >> 32) ^ (uint32_t)h;
}

// One way as one look read it (meta, ka, kb, V, cs; px from the P words of the same look) against the state (key_a, key_b), whose
// hash is hk.  A look that straddles an eviction + refill -- a mixture of two claims' words -- fails the checksum.
EC_HD bool ec_way_hit(uint32_t meta, uint32_t floor, uint64_t ka, uint64_t kb, float V, uint32_t cs, uint32_t px,
                      uint64_t key_a, uint64_t key_b, uint64_t hk) {
  return (meta & 3u) == EC_READY && (meta >> 2) > floor && ka == key_a && kb == key_b && cs == ec_checksum(px, hk, V, meta);
}

// The way a state that found no answer claims, from the two meta words of its look; same0 / same1: the way's key words are the
// state's own.  seq: the number of this launch; launches of other slot groups run side by side and may carry a HIGHER number, so
// the age of a claim is signed and a claim "from the future" is fresh.
//   1. a way that is EMPTY or at or below the floor (way 0 first);
//   2. a PENDING or FILLING claim older than EC_STALE_AFTER launches: its slot has gone away (a phase that ended, a retired slot);
//   3. the READY way with the older claim number (way 0 on a tie): the older answer makes room;
//   a fresh PENDING or FILLING way is never taken: -1 where nothing else is left, the state goes to the network without a claim.
//   A fresh claim under the state's OWN key (another slot asked the same question in a launch nearby) also gives -1: its answer is
//   on the way, the other way must not come to hold the same state.
enum { EC_WAY_FREE = 0, EC_WAY_STALE = 1, EC_WAY_ANSWERED = 2, EC_WAY_FRESH = 3 };   // in the order a victim is looked for
EC_HD int ec_way_class(uint32_t meta, uint32_t seq, uint32_t floor) {
  const uint32_t n = meta >> 2;
  return meta == 0u || n <= floor ? EC_WAY_FREE : (meta & 3u) == EC_READY ? EC_WAY_ANSWERED
       : (int32_t)(seq - n) > (int32_t)EC_STALE_AFTER ? EC_WAY_STALE : EC_WAY_FRESH;
}
EC_HD int ec_pick_victim(uint32_t meta0, uint32_t meta1, bool same0, bool same1, uint32_t seq, uint32_t floor) {
  const int c0 = ec_way_class(meta0, seq, floor), c1 = ec_way_class(meta1, seq, floor);
  const bool barred = (c0 == EC_WAY_FRESH && (same0 || c1 == EC_WAY_FRESH)) || (c1 == EC_WAY_FRESH && same1);
  const bool second_is_older = (int32_t)(seq - (meta1 >> 2)) > (int32_t)(seq - (meta0 >> 2));
  const int w = c0 != c1 ? (c0 < c1 ? 0 : 1) : (c0 == EC_WAY_ANSWERED && second_is_older) ? 1 : 0;   // both answered: the older claim goes
  return barred ? -1 : w;
}

// log2 of the table's entries.  override_log2: AZHIP_EVAL_CACHE_LOG2 as env.h read it (0 = unset, else 4 .. 28; clamped here again
// for callers that did not), taken as it is.  Otherwise from the workload: 8 x slots x simulations per move, 2^16 (4 MB) at the
// least -- an 8-slot test engine and the 128-worker arena players hold a few MB -- up to 2^24 (1 GB), which is about one game
// length of a phase's insertions (a move inserts ~0.46 answers per simulation, a Connect-Four game has ~23 moves).  An engine whose
// 8 x needs the whole 2^24 is a self-play engine that runs phases of many game lengths on fixed weights: there the table is sized
// to EC_BIG_MULT x slots x simulations, at most 2^EC_BIG_CAP_LOG2 entries (8 GB), so that it holds a phase -- the ~3 x 10^7 network
// evaluations of 5000 games x 600 simulations fill a quarter of it -- and an answer outlives the games that share it
// (profiles/eval_cache/README.md has the capacity curve the two figures come from: 4096 slots x 400 simulations gained with every
// doubling up to 2^27).  Never more than 1/8 of the device memory that is free when the engine is created.
enum { EC_MIN_LOG2 = 16, EC_SMALL_CAP_LOG2 = 24, EC_BIG_MULT = 64, EC_BIG_CAP_LOG2 = 27 };
inline int ec_size_log2(int G, int sims, int override_log2, unsigned long long free_bytes) {
  if (override_log2 > 0) return override_log2 < 4 ? 4 : override_log2 > 28 ? 28 : override_log2;
  const long long work = (long long)(G > 0 ? G : 1) * (sims > 0 ? sims : 1);
  int lg = EC_MIN_LOG2;
  while (lg < EC_SMALL_CAP_LOG2 && (1LL << lg) < 8LL * work) ++lg;
  if (lg == EC_SMALL_CAP_LOG2)
    while (lg < EC_BIG_CAP_LOG2 && (1LL << lg) < (long long)EC_BIG_MULT * work) ++lg;
  while (lg > EC_MIN_LOG2 && ((unsigned long long)EC_ENTRY_BYTES << lg) > free_bytes / 8) --lg;
  return lg;
}
