// tower_choice.h -- which network kernel serves a launch: the tower form of a launch (choose_tower), of a search wave
// (choose_wave_tower) and the dense heads' kernel (choose_heads).  Plain C++ (no device runtime, no engine record): a host
// program builds it alone and sweeps it (tests/tower_choice_driver.hip, tests/test_tower_choice_cpu.py).  What the rule knows of
// a form is its TowerFacts, which net_impl.h takes from the form's descriptor; what it knows of a launch is the TowerAsk its
// caller fills.
#pragma once
#include <algorithm>

// The tower forms.  The values are the AZHIP_TOWER numbers (az_engine::env.tower_pick); net_impl.h holds one descriptor per form
// (kernel, layout, geometry table, availability, name, tower_hist bucket), the rule below chooses among them.
enum TowerForm : int {
  TW_AUTO = 0,     // AZHIP_TOWER unset: choose_tower chooses per launch
  TW_SPLIT = 2,    // k_tower16s: two workgroups per board tile (fp32, 128 filters, where the pairs can be co-resident)
  TW_NTS = 3,      // k_tower16 / k_tower16b with the game's latency tile count NTS
  TW_NTM = 7,      // k_tower16 with the game's exact-fit tile count NTM (fp32, games that have one)
  TW_11 = 16,      // k_tower16 / k_tower16b with 11 row tiles
  TW_P19 = 19,     // k_tower16x2 with 10 + 9 row tiles (fp32, 64 filters)
  TW_P21C = 20,    // k_tower16x2c: 11 + 10 row tiles within 176 registers (fp32, 64 filters)
  TW_P21 = 21,     // k_tower16x2 with 11 + 10 row tiles (fp32, 64 filters)
  TW_B22 = 22,     // k_tower16b with 22 row tiles (bf16, 128 filters)
  TW_32 = 32,      // k_tower (32x32x2 MFMA, every tap; fp32)
  TW_MIXED = -1    // k_tower16x2m: not an AZHIP_TOWER value -- a wave launches it where AZHIP_TOWER_MIXED allows
};

// the compute units a launch is priced for (0: the device did not say)
inline int cus(int num_cu) { return num_cu > 0 ? num_cu : 256; }

// What pricing and forcing need to know of one form (net_impl.h facts<D>()): TB boards and `rows` rows per workgroup (the layout's
// RPAD; k_tower: TOWER_ROWS), `frac` the fraction of the (row tile, tap) products it executes, per_cu the workgroups per CU its price
// assumes (2 for the bf16 forms at 64 filters, else 1), stops: it raises the background search's stop word itself.
struct TowerFacts {
  int id = 0; bool bf16 = false, exists = false, stops = false;
  int TB = 0, rows = 0; double frac = 0.0; int per_cu = 1;
};
// the forms of one geometry (P board positions, APAD policy words per slot) and filter count F
struct TowerTable {
  const TowerFacts* forms; int count, F, P, APAD;
  // form `id` of the fp32 / bf16 network; exists = false where the table has none
  TowerFacts form(int id, bool bf16) const {
    for (int i = 0; i < count; ++i) if (forms[i].id == id && forms[i].bf16 == bf16) return forms[i];
    return TowerFacts{};
  }
};
// What a launch asks with.  n = boards the launch is expected to hold (what the forms are priced with; a wave: the upper bound of its
// leaves), nb >= n = the most it can hold (what the split tower's co-residency needs; the grid is sized for nb in any case and
// workgroups beyond the device's count leave at once).
struct TowerAsk {
  int n = 0, nb = -1, num_cu = 0, ngroups = 1;
  bool bf16 = false; int num_blocks = 0, tower_pick = TW_AUTO; bool use_graphs = false, split_off = false;
  int split_streams = 0;           // streams of this process that may launch split towers on the device at the same time
  // a wave: free-running, simulations per background launch, AZHIP_TOWER_MIXED, this wave has a stop word
  bool fr_on = false; int fr_kbg = 0; bool tower_mixed = false, bg_signal = false;
  // ... and what the device reported for the group's previous wave, each word read ONCE per wave by the caller: seen = its network
  // batch (-1: nothing reported, or no such word), needy = the slots it left to the background search (needy_on: there is such a word)
  int seen = -1, needy = -1; bool needy_on = false;
};

// A workgroup's layer chain is sequential and the MFMA pipe of a CU is shared by its resident workgroups, so a launch of n boards
// costs (workgroups per CU, rounded up) x (rows per workgroup) x (fraction of the tile-tap products it executes): k_tower16 packs 176
// rows (4 Connect-Four boards), k_tower 128 (3 boards, every tap), k_tower16 with 3 row tiles 48 (1 board).  `pen` = what the form
// costs beyond that.  (The penalty multiplies first; the paired form's multiplies last, at its call: the two orders round differently.)
inline double tower_price(const TowerFacts& f, int n, int cu, double pen = 1.0) {
  const long wgs = (n + f.TB - 1) / f.TB, per = (long)f.per_cu * cu;
  return pen * (double)((wgs + per - 1) / per) * f.rows * f.frac;
}

// Which tower form serves a launch of up to a.n boards.  Measured round 2 (tools/run_config.py): Mancala 8192 slots 13.5 M sims/s on
// k_tower, 21.5 M on k_tower16 (31 of 99 products); 5x128 two groups 1.10 vs 1.20 M.  Returns a TowerForm.
// INVARIANT: the choice depends on a launch size the host reads from a device-written word WITHOUT synchronising
// (TowerAsk::seen), so which form serves a wave differs from run to run.  Results do not, because every fp32 tower form
// computes the same bits and every bf16 form the same bits (tests/test_net.py, tests/test_net_bf16_gpu.py force each form and compare).
// A new form must pass those cross-form equality tests before it may be returned from here.
inline int choose_tower(const TowerTable& t, const TowerAsk& a) {
  const int n = a.n, nb = std::max(a.nb, a.n), cu = cus(a.num_cu);
  const TowerFacts nts = t.form(TW_NTS, a.bf16), t11 = t.form(TW_11, a.bf16);
  // split tower (k_tower16s, 128 filters): both workgroups of every pair must be resident at once -> all slot groups'
  // launches together at most num_cu workgroups (beyond that the towers queue for CUs and the split only costs: 256
  // slots in two groups 0.62 vs 0.71 M sims/s); its kernel arguments change per launch (epoch): not under hipGraph replay
  // (r4) the count runs over ALL engines of the process on this device that may launch split towers side by side (an arena has
  // two); an engine whose exchange has given up once (another process, a trainer: work this count cannot see) stays unsplit
  const TowerFacts split = t.form(TW_SPLIT, a.bf16);
  const bool can_split = split.exists && !a.use_graphs && a.num_blocks <= 127 && !a.split_off &&
                         2 * std::max(std::max(1, a.ngroups), a.split_streams) * ((nb + split.TB - 1) / split.TB) <= cu;
  // a forced form: where a descriptor with this ID exists for this network (the split tower: where it can run)
  if (a.tower_pick == TW_SPLIT ? can_split : t.form(a.tower_pick, a.bf16).exists) return a.tower_pick;
  if (a.bf16) {                                                    // k_tower16b: 22 (128 filters), 11 or 3 row tiles
    const double d16 = tower_price(t11, n, cu), d3 = tower_price(nts, n, cu, 1.1);   // (3 tiles +10 %: a third of the weight reuse, more barriers per row)
    const TowerFacts b22 = t.form(TW_B22, true);
    if (b22.exists) {
      // 22 row tiles = twice the boards per workgroup: each weight fragment serves twice the rows (10x128, 4096 boards: 578
      // vs 684 us); only where it does not leave CUs idle that the 11-tile form would use
      const double d22 = tower_price(b22, n, cu, 0.9);
      if (d22 <= d16 && d22 <= d3) return TW_B22;
    }
    return d3 <= d16 ? TW_NTS : TW_11;
  }
  // the k_tower16 family executes only the (tile, tap) products that touch the board (Geo16); k_tower (32x32x2) computes every tap
  const double c16 = tower_price(t11, n, cu), c32 = tower_price(t.form(TW_32, false), n, cu);
  const double c3 = tower_price(nts, n, cu, 1.1);                  // +10 %: a third of the weight reuse, more barriers per row
  if (c3 <= c16 && c3 <= c32) return can_split ? TW_SPLIT : TW_NTS;
  const TowerFacts ntm = t.form(TW_NTM, false), p21 = t.form(TW_P21, false);
  // (r4) the exact-fit variant (NTM tiles: whole boards, no padding rows): where its workgroups fill the CUs evenly it beats
  // the 11-tile form by the padding rows and by the last, partly filled round of workgroups
  if (ntm.exists) {
    // +3 %: fewer rows per weight fragment; the half-size form at 128 filters +20 %: half the rows per weight fragment there (the
    // vector-memory path that streams the weights is what a 128-filter layer waits for: DESIGN.md 4d, the trainer's 6-tile layer)
    const double cm = tower_price(ntm, n, cu, t.P == 42 && t.F == 128 ? 1.2 : 1.03);
    if (cm < c16 && cm < c32 && (!p21.exists || cm < tower_price(p21, n, cu))) return TW_NTM;
  }
  // paired k_tower16x2: 336 rows = 8 Connect-Four boards per workgroup, no padding rows.  Its 92 KB of LDS allow one
  // workgroup per CU, so with several slot groups the groups' towers cannot interleave on a CU (Connect-Four, two groups:
  // 3.80 vs 4.11 M sims/s in round 1): +8 % on its cost there
  if (p21.exists) {
    const double c21 = tower_price(p21, n, cu) * (a.ngroups > 1 ? 1.08 : 1.0);
    if (c21 < c16 && c21 < c32) return TW_P21;
  }
  return c16 <= c32 ? TW_11 : TW_32;
}

// The tower of one search wave: `form`, or the mixed launch of both paired forms (mixed; `form` stays TW_P21, whose layout the
// launch's first workgroups have); tower_stops: the launch raises the background search's stop word itself.
struct WaveTower { int form; bool mixed, tower_stops; };
inline WaveTower choose_wave_tower(const TowerTable& t, const TowerAsk& a) {
  const int N = a.n, cu = cus(a.num_cu);
  // how many boards the launch will really hold: with the evaluation cache answering part of every wave, what the device
  // reported for the group's last completed wave (+ 1/8: a launch priced too small costs more than one priced too large)
  TowerAsk b = a;
  b.nb = N;
  if (a.seen >= 0) b.n = std::max(1, std::min(N, a.seen + a.seen / 8 + 8));
  WaveTower w{choose_tower(t, b), false, false};
  const TowerFacts p21 = t.form(TW_P21, a.bf16);
  if (w.form == TW_P21 && a.fr_on && a.ngroups == 1 && a.tower_pick == TW_AUTO && a.fr_kbg > 0 && a.needy_on && a.seen > 0) {
    // The paired tower beside the side streams' kernels (resnet16.h k_tower16x2c): a CU that holds a workgroup of the background search
    // (256 threads = 32 Connect-Four slots of the needy list) takes no workgroup of the 198-register form for as long as that search
    // runs.  Measured: in the steady state (~8 such workgroups on average, more in some waves) the launch gains a round of workgroups
    // beyond ~478 of its 512; the margin of 14 is that measurement (the move step is not part of it: within 96 registers it changes
    // nothing).  Where the counts the device reported for the previous wave say that this adds a round, the 176-register form serves
    // the launch.
    const int wgs = (a.seen + p21.TB - 1) / p21.TB, rounds = (wgs + cu - 1) / cu, bg = (std::max(a.needy, 0) * t.APAD + 255) / 256;
    if (wgs > rounds * (cu - bg) - 14) w.form = TW_P21C;
  }
  // (r6, measured, off unless AZHIP_TOWER_MIXED=1) A batch between 15 and 16 boards per CU (a free-running wave's ~3800 boards at 4096 slots on
  // 256 CUs) costs two rounds of the 8-board form whatever its size.  As ONE launch of cu 8-board workgroups and up to cu 7-board ones
  // (k_tower16x2m) it is slower, 1.09 ms per wave instead of 0.80 (profiles/r6/README.md): a workgroup's time hardly shrinks with its
  // boards, because every workgroup streams the same 1.5 MB of weights through its CU's vector-memory path.
  const int first = cu * p21.TB;
  w.mixed = w.form == TW_P21 && a.tower_mixed && a.tower_pick == TW_AUTO && N > first && a.seen > first &&
            a.seen + 16 <= first + cu * t.form(TW_P19, a.bf16).TB;
  // the background search's stop word: a paired form raises it itself, from its last round of workgroups (resnet16.h tower16x2_body)
  w.tower_stops = a.bg_signal && t.form(w.form, a.bf16).stops;
  return w;
}

// Dense heads of n_max boards: 16-board tiles (k_heads16: a quarter of the chain latency, 23 instead of 43 us per launch
// at 64 filters whatever the size) unless several slot groups run big launches side by side -- there the heads hide
// under the other group's tower anyway and twice as many workgroups asking for a CU cost 1 % (0.867 vs 0.857 ms per
// step, two groups of 2048): 32-board tiles (k_heads_mfma).  The vector-ALU kernel when the head filters do not fit
// the MFMA fragments.
static constexpr int HEADS16_MAX_BOARDS = 1024;
enum HeadsForm : int {
  HD_16_STAGED,    // k_heads16<.., true>: value and policy tiles in two workgroups, features staged in LDS
  HD_16,           // k_heads16<.., false>
  HD_MFMA,         // k_heads_mfma: 32-board tiles
  HD_VALU          // k_heads: the vector ALU
};
// heads_pick = AZHIP_HEADS; hd16_ok / hd_ok: the head filters fit k_heads16's / k_heads_mfma's fragments (NetDev)
inline HeadsForm choose_heads(int heads_pick, bool hd16_ok, bool hd_ok, int n_max, int ngroups, int num_cu) {
  const bool small = heads_pick == 16 || (heads_pick != 32 && (n_max <= HEADS16_MAX_BOARDS || ngroups == 1));
  const int tiles = (n_max + 15) / 16;
  if (hd16_ok && small) return 2 * tiles <= cus(num_cu) ? HD_16_STAGED : HD_16;
  return hd_ok ? HD_MFMA : HD_VALU;
}
