// phase_books_driver.cpp -- TEST INFRASTRUCTURE: prints what csrc/phase_books.h decides, built by a host compiler from that header alone
// (tests/test_phase_books_cpu.py).
//   phase_books_driver retire <total_games> <first_game_id> <next_game> <slots per group> <groups> <slot>:<game id> ...
//     the retired slots in slot order.  Output: aborted <ids>, refill <slot>:<id> ..., given_up <n>, idle <per group>, next_game <n>
//   phase_books_driver order <game id> ...                          output: order <indices>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../alphazero.jl_amd/csrc/phase_books.h"

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "order") == 0) {
    std::vector<az_game_rec> games((size_t)(argc - 2));
    for (int a = 2; a < argc; ++a) { memset(&games[(size_t)(a - 2)], 0, sizeof(az_game_rec)); games[(size_t)(a - 2)].game_id = (int32_t)atoll(argv[a]); }
    printf("order");
    for (int i : order_by_game_id(games)) printf(" %d", i);
    printf("\n");
    return 0;
  }
  if (argc < 7 || strcmp(argv[1], "retire") != 0) { fprintf(stderr, "usage: %s retire ... | order ...\n", argv[0]); return 2; }
  GameIds ids;
  ids.total_games = atoi(argv[2]); ids.first_game_id = atoi(argv[3]); ids.next_game = atoi(argv[4]);
  const int per_group = atoi(argv[5]), ngroups = atoi(argv[6]);
  std::vector<int> slots;
  std::vector<uint32_t> game_id((size_t)per_group * (size_t)ngroups, 0u);
  for (int a = 7; a < argc; ++a) {
    int slot = 0; long long id = 0;
    if (sscanf(argv[a], "%d:%lld", &slot, &id) != 2 || slot < 0 || slot >= per_group * ngroups) { fprintf(stderr, "bad slot entry %s\n", argv[a]); return 2; }
    slots.push_back(slot); game_id[(size_t)slot] = (uint32_t)id;
  }
  std::vector<int32_t> aborted;
  const Retirement r = retire_slots(slots, game_id.data(), per_group, ngroups, &ids, &aborted);
  printf("aborted");
  for (int32_t id : aborted) printf(" %d", (int)id);
  printf("\nrefill");
  for (size_t i = 0; i < r.slots.size(); ++i) printf(" %d:%u", r.slots[i], (unsigned)r.gids[i]);
  printf("\ngiven_up %d\nidle", r.given_up);
  for (int n : r.idle) printf(" %d", n);
  printf("\nnext_game %d\n", ids.next_game);
  return 0;
}
