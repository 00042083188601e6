// plane_gather_driver.cpp -- TEST INFRASTRUCTURE: prints the plan csrc/plane_gather.h makes for given per-rank game tables, built by a
// host compiler from that header alone (tests/test_plane_gather_plan_cpu.py).
//   plane_gather_driver <round rows> <destination capacity> <table of rank 0> <table of rank 1> ...
// a table is "id:len,id:len,..." in push order, "-" for a rank without a game.  Output, one item per line:
//   plan W T maxB R rounds skip dup dup_id
//   game <rank> <k> <id> <len> <src> <prefix> <start>     the rank's games in packed (ascending id) order
//   row <rank> <s> <round> <batch sample> <q>              every row of the rank's packed batch, found as the kernels find it
//   send <rank> <round> <rows>
//   rb <RW> <ND> <bytes>                                   the record of the four geometries
//   rows <W> <rb> <default round rows>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../alphazero.jl_amd/csrc/plane_gather.h"

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <round rows> <capacity> <table>...\n", argv[0]); return 2; }
  const long long R = atoll(argv[1]), cap = atoll(argv[2]);
  std::vector<std::vector<pg::Game>> tables;
  for (int a = 3; a < argc; ++a) {
    std::vector<pg::Game> t;
    if (strcmp(argv[a], "-") != 0) {
      std::string s(argv[a]);
      size_t at = 0;
      while (at < s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        int id = 0, len = 0;
        if (sscanf(s.substr(at, end - at).c_str(), "%d:%d", &id, &len) != 2) { fprintf(stderr, "bad table entry in %s\n", argv[a]); return 2; }
        t.push_back(pg::Game{id, len});
        at = end + 1;
      }
    }
    tables.push_back(t);
  }
  const pg::Plan p = pg::make_plan(tables, R, cap);
  printf("plan %d %lld %lld %lld %lld %lld %d %d\n", p.W, p.T, p.maxB, p.R, p.rounds, p.skip, p.dup ? 1 : 0, (int)p.dup_id);
  for (int r = 0; r < p.W; ++r) {
    const pg::RankPlan& rp = p.ranks[(size_t)r];
    const int ng = (int)rp.order.size();
    for (int k = 0; k < ng; ++k) {
      const pg::Game& g = tables[(size_t)r][(size_t)rp.order[(size_t)k]];
      printf("game %d %d %d %d %lld %lld %lld\n", r, k, (int)g.id, (int)g.len, rp.src[(size_t)k], rp.prefix[(size_t)k], rp.start[(size_t)k]);
    }
    for (long long s = 0; s < rp.B; ++s) {
      const int g = pg::find_game(rp.prefix.data(), ng, s);
      const long long off = s - rp.prefix[(size_t)g];
      printf("row %d %lld %lld %lld %lld\n", r, s, s / p.R, rp.src[(size_t)g] + off, rp.start[(size_t)g] + off);
    }
    for (long long k = 0; k < p.rounds; ++k) printf("send %d %lld %lld\n", r, k, pg::round_rows_of(p, r, k));
  }
  const int geom[4][2] = {{36, 11}, {133, 9}, {76, 8}, {406, 84}};   // Tic-tac-toe, Connect Four, Mancala, 9x9 Go: (RW, ND)
  for (const auto& g : geom) printf("rb %d %d %lld\n", g[0], g[1], pg::record_bytes(g[0], g[1]));
  for (int W : {1, 3, 8}) printf("rows %d %d %lld\n", W, 2304, pg::default_round_rows(W, 2304));
  return 0;
}
