// solver_table_driver.cpp -- the host side of the Connect Four solver (alphazero.jl_amd/csrc/solver_search.h, no HIP) run the way
// the kernels of csrc/solver.h run it: per state 7 queries, a first pass each, then the second pass of the queries that stayed
// unsolved, over a table that is a plain std::vector<uint64_t>.  tests/test_solver_table_cpu.py builds it with g++ and feeds it.
//
// stdin, one item per line:
//   #table N     a new, empty table of 2^N entries from here on; N = -1: no table (sv_search<false>, the tableless path)
//   #clear       empty the table
//   #budget N    nodes per query from here on            #weak 0|1    strong / weak mode from here on
//   <moves>      a position as the string of 1-based columns played from the empty board: solve it
// stdout, one line per position: value q[0] .. q[6] nodes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../alphazero.jl_amd/csrc/solver_search.h"

struct HostStack {
  uint32_t* base;
  uint32_t& operator()(int ply) const { return base[ply]; }
};
struct HostTable {
  uint64_t* words;
  int log2;
  int bits() const { return log2; }
  uint64_t load(uint64_t slot) const { return words[slot]; }
  void store(uint64_t slot, uint64_t w) const { words[slot] = w; }
};

template <bool TT, class Table>
static void solve_state(uint64_t a, uint64_t b, int weak, long long budget, Table table) {
  uint32_t frames[SV_PLIES];
  const HostStack stack{frames};
  uint64_t cur[7], all[7];
  int stones[7];
  int8_t q[7], bounded[7];
  long long nodes = 0;
  for (int act = 0; act < 7; ++act) {
    int r = SV_NA;
    if (!sv_child(a, b, act, weak, &cur[act], &all[act], &stones[act], &r)) r = sv_solve<TT>(cur[act], all[act], stones[act], weak, budget, stack, table, &nodes);
    q[act] = (int8_t)r;
    bounded[act] = 0;
  }
  int best = SV_NA;
  for (int act = 0; act < 7; ++act)
    if (q[act] != SV_UNSOLVED && q[act] > best) best = q[act];
  for (int act = 0; act < 7; ++act)
    if (q[act] == SV_UNSOLVED && best != SV_NA) bounded[act] = (int8_t)sv_bounded<TT>(cur[act], all[act], stones[act], weak, best, budget, stack, table, &nodes);
  std::printf("%d", sv_state_value(a, b, q, bounded));
  for (int act = 0; act < 7; ++act) std::printf(" %d", (int)q[act]);
  std::printf(" %lld\n", nodes);
}

int main() {
  std::vector<uint64_t> table;
  int log2 = -1, weak = 0;
  long long budget = AZ_SOLVER_DEFAULT_BUDGET;
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    std::string s(line);
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
    if (s.empty()) continue;
    if (s[0] == '#') {
      if (!s.compare(0, 7, "#table ")) {
        log2 = std::atoi(s.c_str() + 7);
        if (log2 < -1 || log2 > 30) { std::fprintf(stderr, "bad table size: %s\n", s.c_str()); return 2; }
        table.assign(log2 < 0 ? 0 : (size_t)1 << log2, 0);
      } else if (s == "#clear") table.assign(table.size(), 0);
      else if (!s.compare(0, 8, "#budget ")) budget = std::atoll(s.c_str() + 8);
      else if (!s.compare(0, 6, "#weak ")) weak = std::atoi(s.c_str() + 6) != 0;
      else { std::fprintf(stderr, "unknown directive: %s\n", s.c_str()); return 2; }
      continue;
    }
    GEnv g = ConnectFour::init();
    for (char c : s) {
      if (c < '1' || c > '7' || (g.fin & 1) || !((ConnectFour::mask(g) >> (c - '1')) & 1)) { std::fprintf(stderr, "bad position: %s\n", s.c_str()); return 2; }
      ConnectFour::play(g, c - '1');
    }
    if (log2 < 0) solve_state<false>(g.a, g.b, weak, budget, SvNoTable{});
    else solve_state<true>(g.a, g.b, weak, budget, HostTable{table.data(), log2});
  }
  return 0;
}
