// Host-only driver of tests/test_tower_choice_cpu.py: the rule of csrc/tower_choice.h over the facts net_impl.h takes from the real
// form descriptors of the four geometries.  Built with hipcc --offload-host-only; it makes no HIP runtime call.
//   table   the facts and sweeps A (automatic choice), B (split tower), C (forced forms): break-points "from n on: form"
//   wave    sweep D, choose_wave_tower over the previous wave's reported counts: break-points "from seen on: form mixed stops"
//   heads   sweep E, choose_heads: break-points "from n_max on: kernel"
#include <climits>
#include <cstdio>
#include <cstring>

#include "net_impl.h"

template <class Gm, int F> static void print_facts(const char* name) {
  const TowerTable t = tower_table<Gm, F>();
  for (int i = 0; i < t.count; ++i) {
    const TowerFacts& f = t.forms[i];
    if (!f.exists) printf("facts %s F=%d id=%d bf16=%d exists=0\n", name, F, f.id, (int)f.bf16);
    else printf("facts %s F=%d id=%d bf16=%d exists=1 stops=%d TB=%d rows=%d frac=%.17g per_cu=%d\n", name, F, f.id, (int)f.bf16, (int)f.stops, f.TB, f.rows, f.frac, f.per_cu);
  }
}
// the form of every n = 1 .. n1 (nb = nbmul * n), printed where it changes
static void breaks(const TowerTable& t, TowerAsk a, int n1, int nbmul) {
  int last = INT_MIN;
  for (int n = 1; n <= n1; ++n) {
    a.n = n; a.nb = nbmul * n;
    const int f = choose_tower(t, a);
    if (f != last) { printf("  %d %d\n", n, f); last = f; }
  }
}
static TowerAsk base_ask() { TowerAsk a; a.num_cu = 256; a.num_blocks = 5; return a; }
template <class Gm, int F> static void sweep_a(const char* name) {
  for (int bf16 = 0; bf16 < 2; ++bf16) for (int groups = 1; groups <= 2; ++groups) for (int cu : {256, 64, 0}) {
    printf("A %s F=%d bf16=%d groups=%d cu=%d\n", name, F, bf16, groups, cu);
    TowerAsk a = base_ask(); a.bf16 = bf16; a.ngroups = groups; a.num_cu = cu;
    breaks(tower_table<Gm, F>(), a, 8192, 1);
  }
}
template <class Gm> static void sweep_b(const char* name) {
  static const char* const toggles[] = {"none", "split_off", "use_graphs", "num_blocks=128", "tower_pick=2", "tower_pick=3"};
  for (int groups : {1, 2, 4}) for (int streams : {0, 1, 2, 4}) for (int nbmul = 1; nbmul <= 2; ++nbmul) for (int t = 0; t < 6; ++t) {
    printf("B %s groups=%d streams=%d nb=%dn toggle=%s\n", name, groups, streams, nbmul, toggles[t]);
    TowerAsk a = base_ask(); a.ngroups = groups; a.split_streams = streams;
    if (t == 1) a.split_off = true;
    if (t == 2) a.use_graphs = true;
    if (t == 3) a.num_blocks = 128;
    if (t == 4) a.tower_pick = TW_SPLIT;
    if (t == 5) a.tower_pick = TW_NTS;
    breaks(tower_table<Gm, 128>(), a, 600, nbmul);
  }
}
template <class Gm, int F> static void sweep_c(const char* name) {
  for (int bf16 = 0; bf16 < 2; ++bf16) for (int pick : {2, 3, 5, 7, 16, 19, 20, 21, 22, 32}) {
    printf("C %s F=%d bf16=%d pick=%d:", name, F, bf16, pick);
    for (int n : {1, 300, 4096}) { TowerAsk a = base_ask(); a.bf16 = bf16; a.tower_pick = pick; a.n = a.nb = n; printf(" %d", choose_tower(tower_table<Gm, F>(), a)); }
    printf("\n");
  }
}
template <class Gm> static void table(const char* name) {
  print_facts<Gm, 64>(name); print_facts<Gm, 128>(name);
  sweep_a<Gm, 64>(name); sweep_a<Gm, 128>(name);
  sweep_b<Gm>(name);
  sweep_c<Gm, 64>(name); sweep_c<Gm, 128>(name);
}

// D: Connect Four, 64 filters, a wave of up to 4096 leaves on 256 CUs; every gate of the two wave rules on, then each off in turn
static void sweep_d() {
  static const char* const gates[] = {"none", "fr_on", "groups", "fr_kbg", "tower_pick", "tower_mixed", "bg_signal", "needy_on"};
  const TowerTable t = tower_table<ConnectFour, 64>();
  printf("D APAD=%d N=4096 cu=256\n", t.APAD);
  for (int off = 0; off < 8; ++off) for (int needy : {-1, 0, 64, 256, 1024}) {
    TowerAsk a = base_ask();
    a.n = 4096; a.fr_on = off != 1; a.ngroups = off == 2 ? 2 : 1; a.fr_kbg = off == 3 ? 0 : 32; a.tower_pick = off == 4 ? TW_P21 : TW_AUTO;
    a.tower_mixed = off != 5; a.bg_signal = off != 6; a.needy_on = off != 7; a.needy = needy;
    printf("D off=%s needy=%d\n", gates[off], needy);
    int last[3] = {INT_MIN, 0, 0};
    for (int seen = -1; seen <= 4096; ++seen) {
      a.seen = seen;
      const WaveTower w = choose_wave_tower(t, a);
      const int now[3] = {w.form, (int)w.mixed, (int)w.tower_stops};
      if (memcmp(now, last, sizeof now)) { printf("  %d %d %d %d\n", seen, now[0], now[1], now[2]); memcpy(last, now, sizeof now); }
    }
  }
}
// E
static void sweep_e() {
  for (int pick : {0, 16, 32}) for (int hd16 = 0; hd16 < 2; ++hd16) for (int hd = 0; hd < 2; ++hd) for (int groups = 1; groups <= 2; ++groups) for (int cu : {256, 64, 0}) {
    printf("E heads_pick=%d hd16_ok=%d hd_ok=%d groups=%d cu=%d\n", pick, hd16, hd, groups, cu);
    int last = INT_MIN;
    for (int n = 1; n <= 4200; ++n) {
      const int k = choose_heads(pick, hd16, hd, n, groups, cu);
      if (k != last) { printf("  %d %d\n", n, k); last = k; }
    }
  }
}

int main(int argc, char** argv) {
  const char* what = argc > 1 ? argv[1] : "";
  if (!strcmp(what, "table")) { table<ConnectFour>("ConnectFour"); table<TicTacToe>("TicTacToe"); table<Mancala>("Mancala"); table<Go9Planes>("Go9Planes"); }
  else if (!strcmp(what, "wave")) sweep_d();
  else if (!strcmp(what, "heads")) sweep_e();
  else { fprintf(stderr, "usage: %s table | wave | heads\n", argv[0]); return 2; }
  return 0;
}
