// phase_books.h -- the host's book-keeping rules of a self-play phase: which game id comes next, what becomes of a retired slot, the
// order in which finished games are handed over.  Plain C++ (no HIP types): a host compiler builds it alone (tests/phase_books_driver.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/azhip.h"
// the game ids of a phase: first_game_id + 0, 1, ... in the order slots ask for them; total_games < 0 = unbounded (bench, polling)
struct GameIds {
  int total_games = 0, first_game_id = 0, next_game = 0;
  // another id to hand out?  An unbounded phase stops refilling before its ids reach the replacement bit.
  bool more() const { return total_games < 0 ? (long long)first_game_id + next_game < (long long)AZ_REPLACEMENT_GAME_BIT : next_game < total_games; }
  uint32_t take() { return (uint32_t)(first_game_id + next_game++); }
};
// What becomes of the slots a look found retired (`finished` word 2: node pool or move records full).
struct Retirement {
  std::vector<int> slots; std::vector<uint32_t> gids;   // the slots that play on, in slot order, each with an empty tree, and the ids they play
  int given_up = 0;                  // replacement games that retired as well: they count as done
  std::vector<int> idle;             // per slot group: retired slots that stay idle (the group's active count drops by as many)
};
// The one rule, for both schedules.  A retired slot's game is reported as aborted.  If its id is an original one the phase still
// owes the caller this game: ONE replacement with its own RNG streams (id | bit 30) takes the slot, so that num_games games come
// back and every game_simulated() callback a host waits for arrives.  If the replacement overflowed too it is given
// up and counted as done, and the slot takes the phase's next id while there is one.
// slots: ascending; game_id: by slot; ids: the phase's counter, advanced by the ids handed out; aborted: takes the retired ids, in slot order.
inline Retirement retire_slots(const std::vector<int>& slots, const uint32_t* game_id, int slots_per_group, int ngroups, GameIds* ids,
                               std::vector<int32_t>* aborted) {
  Retirement r;
  r.idle.assign((size_t)ngroups, 0);
  for (int sl : slots) {
    const int32_t id = (int32_t)game_id[sl];
    const bool original = !(id & AZ_REPLACEMENT_GAME_BIT);
    aborted->push_back(id);
    if (!original) r.given_up++;
    if (original || ids->more()) {
      r.slots.push_back(sl); r.gids.push_back(original ? (uint32_t)(id | AZ_REPLACEMENT_GAME_BIT) : ids->take());
    } else r.idle[(size_t)(sl / slots_per_group)]++;
  }
  return r;
}
// the order of `games` by game id (games with one id keep their order: a phase never has two)
inline std::vector<int> order_by_game_id(const std::vector<az_game_rec>& games) {
  std::vector<int> ord(games.size());
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return games[(size_t)a].game_id < games[(size_t)b].game_id; });
  return ord;
}
