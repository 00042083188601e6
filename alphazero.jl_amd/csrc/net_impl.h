// net_impl.h -- launch logic of the network kernels (resnet.h, resnet16.h), templated on the game: which tower kernel
// serves a launch (pick_tower) and the launches themselves.  Instantiated once per game in net_c4.hip / net_ttt.hip /
// net_mancala.hip (three translation units, so that the big fully unrolled tower kernels compile in parallel);
// net.hip dispatches on the engine's game.
#pragma once
#include "engine.h"

// ---- the tower forms --------------------------------------------------------------------------------------------------------
// One descriptor per form, templated on the game and the filter count, states everything a launch needs:
//   ID, OK   its TowerForm (engine.h) and whether the form exists for this game and F
//   BF16     which network it serves (pick_tower returns TW_NTS / TW_11 for both: the engine's network decides between the two descriptors)
//   T        its layout struct: T::TB boards per workgroup, T::THREADS, T::BYTES of LDS, T::Geo / T::GEO its row permutation table
//   K        its kernel, for FROM_PLANES false and true;  net(e): the fragments that kernel takes
//   frac()   the fraction of a 3x3 convolution's (row tile, tap) products it executes (Geo16 skips the products whose tap falls off the
//            board for a whole tile; k_tower computes every tap).  az_prof.exec_units weighs a launch's boards with it, so that a roofline
//            can count the work DONE instead of the dense convolution's
//   HIST     its tower_hist bucket;  name(): its az_net_last_kernel spelling
//   STOP     its kernel takes the background search's stop word (TowerIn::stop) and raises it from its last round of workgroups
// set_kernel_attrs_f and launch_tower walk Forms<Gm, F>; a form's properties are stated nowhere else.
template <class T> static constexpr double geo_frac() { return T::Geo::tab.cost / (9.0 * (T::RPAD / 16)); }
// what the k_tower16 family of the fp32 network shares
template <class T_, int ID_, bool OK_, int HIST_> struct FormFp32 {
  using T = T_;
  static constexpr int ID = ID_, HIST = HIST_;
  static constexpr bool OK = OK_, BF16 = false, STOP = false;
  static const Net16Dev& net(const az_engine* e) { return e->net16; }
  static constexpr double frac() { return geo_frac<T>(); }
};
template <class Gm, int F, int NT, int ID_, int HIST_> struct Form16 : FormFp32<T16<Gm, F, NT>, ID_, (NT > 0), HIST_> {
  template <bool FP> static constexpr auto K = &k_tower16<Gm, F, FP, NT>;
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower16<%s,%d,NT=%d>", g, F, NT); }
};
template <class Gm, int F> struct FormSplit : FormFp32<T16S<Gm, F>, TW_SPLIT, F == 128, 0> {
  template <bool FP> static constexpr auto K = &k_tower16s<Gm, F, FP>;
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower16s<%s,%d>", g, F); }
};
template <class Gm, int F, int NT0, int NT1, int ID_> struct FormPaired : FormFp32<T16P<Gm, F, NT0, NT1>, ID_, F == 64, 2> {
  template <bool FP> static constexpr auto K = &k_tower16x2<Gm, F, FP, NT0, NT1>;
  static constexpr bool STOP = true;
  static void name(char* s, size_t n, const char* g) {
    if (NT0 == 11) snprintf(s, n, "k_tower16x2<%s,%d>", g, F);
    else snprintf(s, n, "k_tower16x2<%s,%d,NT=%d>", g, F, NT0 + NT1);
  }
};
template <class Gm, int F> struct FormPairedC : FormFp32<T16P<Gm, F>, TW_P21C, F == 64, 2> {
  template <bool FP> static constexpr auto K = &k_tower16x2c<Gm, F, FP>;
  static constexpr bool STOP = true;
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower16x2c<%s,%d>", g, F); }
};
// both paired forms in one launch (workgroups 0 .. first - 1 of T, the rest of T7); launched by wave_net_f only, never FROM_PLANES, and
// priced there by the two forms' shares of the batch
template <class Gm, int F> struct FormMixed : FormFp32<T16P<Gm, F>, TW_MIXED, F == 64, 2> {
  using T7 = T16P<Gm, F, 10, 9>;
  template <bool FP> static constexpr auto K = &k_tower16x2m<Gm, F, FP>;
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower16x2m<%s,%d>", g, F); }
};
template <class Gm, int F> struct Form32 {
  struct T { static constexpr int TB = TOWER_ROWS / Gm::P, THREADS = TowerCfg<F>::THREADS, BYTES = TowerLds<F>::BYTES; };
  static constexpr int ID = TW_32, HIST = 3;
  static constexpr bool OK = true, BF16 = false, STOP = false;
  template <bool FP> static constexpr auto K = &k_tower<Gm, F, FP>;
  static const NetDev& net(const az_engine* e) { return e->net; }
  static constexpr double frac() { return 1.0; }
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower<%s,%d>", g, F); }
};
template <class Gm, int F, int NT, int ID_, int HIST_> struct Form16b {
  using T = T16B<Gm, F, NT>;
  static constexpr int ID = ID_, HIST = HIST_;
  static constexpr bool OK = NT != 22 || F == 128, BF16 = true, STOP = false;
  template <bool FP> static constexpr auto K = &k_tower16b<Gm, F, FP, NT>;
  static const Net16bDev& net(const az_engine* e) { return e->net16b; }
  static constexpr double frac() { return geo_frac<T>(); }
  static void name(char* s, size_t n, const char* g) { snprintf(s, n, "k_tower16b<%s,%d,NT=%d>", g, F, NT); }
};
template <class... D> struct FormList {};
template <class Gm, int F> using Forms = FormList<
    FormSplit<Gm, F>, Form16<Gm, F, NTS<Gm>, TW_NTS, 1>, Form16<Gm, F, NTM<Gm>, TW_NTM, 3>, Form16<Gm, F, 11, TW_11, 2>,
    FormPaired<Gm, F, 11, 10, TW_P21>, FormPaired<Gm, F, 10, 9, TW_P19>, FormPairedC<Gm, F>, Form32<Gm, F>,
    Form16b<Gm, F, NTS<Gm>, TW_NTS, 1>, Form16b<Gm, F, 11, TW_11, 2>, Form16b<Gm, F, 22, TW_B22, 3>>;

template <class D, bool FP> static int set_form_attr() {
  if constexpr (D::OK) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(D::template K<FP>), hipFuncAttributeMaxDynamicSharedMemorySize, D::T::BYTES));
  return AZ_OK;
}
template <class Gm, int F, class... D> static int set_kernel_attrs_f(FormList<D...>) {
  int r = AZ_OK;
  (void)(((r = set_form_attr<D, false>()) == AZ_OK && (r = set_form_attr<D, true>()) == AZ_OK) && ...);
  AZCHK(r);
  AZCHK((set_form_attr<FormMixed<Gm, F>, false>()));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_heads16<Gm, F, true>), hipFuncAttributeMaxDynamicSharedMemorySize, H16<Gm, F, true>::BYTES));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_heads16<Gm, F, false>), hipFuncAttributeMaxDynamicSharedMemorySize, H16<Gm, F, false>::BYTES));
  return AZ_OK;
}
// (Re-arranging the cells inside Geo16's class constraint so that the tap-shifted rows of every ds_read_b128 pass are
// distinct mod 8 -- a host-side descent took the excess lanes of the Connect-Four layout from 186 to 68 over 170 passes --
// changed no kernel time: 844 vs 845 us per 4096 boards, bf16 10x128 4.88 vs 4.83 M sims/s.  The A reads are not what a
// tower waits for; the tables stay Geo16's own.)
// the row permutation table of layout T (Geo16, resnet16.h) goes to the device once per engine, into the slot T names
template <class T> static int upload_geo(az_engine* e) {
  using G = typename T::Geo;
  if (e->d_geo[T::GEO]) return AZ_OK;                               // two layouts with one tile count share a table
  std::vector<uint16_t> h((size_t)10 * G::RPAD);
  for (int i = 0; i < G::RPAD; ++i) h[i] = G::tab.pos[i];
  for (int i = 0; i < 9 * G::RPAD; ++i) h[G::RPAD + i] = G::tab.nbr[i];
  uint16_t* d = nullptr;
  AZCHK(dalloc(e, &d, h.size(), false));
  HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(uint16_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->d_geo[T::GEO] = d;
  return AZ_OK;
}
template <class G> static int geometry_out(uint16_t* out, int64_t cap, int* rows, int* products) {
  if (cap < (int64_t)10 * G::RPAD) return fail(AZ_ERR_CAPACITY, "need %d words", 10 * G::RPAD);
  for (int i = 0; i < G::RPAD; ++i) out[i] = G::tab.pos[i];
  for (int i = 0; i < 9 * G::RPAD; ++i) out[G::RPAD + i] = G::tab.nbr[i];
  *rows = G::RPAD; *products = G::tab.cost;
  return AZ_OK;
}
static const char* game_name(const az_engine* e);
// The background search's stop word behind a network launch that does not raise it itself (every form but the paired towers, and
// k_simplenet): set from a stream of its own behind an event on the launch's stream `sn` (a one-thread launch IN the wave's stream sat
// 7.6 us between tower and heads)
static int raise_stop_word(az_engine* e, hipStream_t sn) {
  HIPCHK(hipEventRecord(e->fr_ev[3], sn));
  HIPCHK(hipStreamWaitEvent(e->fr_s[3], e->fr_ev[3], 0));
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, e->fr_s[3], e->d_bg_stop, e->bg_seq);
  return AZ_OK;
}
// ---- SimpleNet engines (simplenet.h): one kernel, one launch per batch ------------------------------------------------------------
template <class Gm> static constexpr bool SIMPLE_OK = Gm::A <= 16;   // one policy tile: the three device twins (the plane geometry is refused at create)
template <class Gm> static int simple_set_kernel_attrs() {
  if constexpr (SIMPLE_OK<Gm>) {
    const int most = (int)sn_lds_bytes(sn_row_words(16 * SN_WAVES * SN_TPW));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_simplenet<Gm, false>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_simplenet<Gm, true>), hipFuncAttributeMaxDynamicSharedMemorySize, most));
  }
  return AZ_OK;
}
// the whole network on up to n_max boards (device count in n_ptr when given); the arguments of launch_heads
template <class Gm, bool FROM_PLANES>
static int launch_simple(az_engine* e, hipStream_t st, const GEnv* envs, const int* eslots, const int* n_ptr, int n_max, const float* X,
                         const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride) {
  if constexpr (!SIMPLE_OK<Gm>) return fail(AZ_ERR_STATE, "no SimpleNet kernel for this geometry");
  else {
    if (n_max <= 0) return AZ_OK;
    snprintf(e->last_tower, sizeof e->last_tower, "k_simplenet<%s>", game_name(e));
    e->tower_hist[3]++;
    LAUNCH_ON(e, st, AZ_K_TOWER, n_max, (k_simplenet<Gm, FROM_PLANES>), (n_max + SN_ROWS - 1) / SN_ROWS, SN_THREADS, sn_lds_bytes(e->snet.rs), e->snet,
              envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride);
    return AZ_OK;
  }
}
// The network part of a wave: the one launch takes the place of tower + heads on the group's network stream; the streams meet as in
// wave_net_f, and the background search's stop word is raised behind the launch (k_simplenet does not raise it itself).
template <class Gm> static int wave_simple(az_engine* e, int g, bool split, int nmax) {
  const DView& v = e->gv[g];
  hipStream_t st = e->gs[g], sn = e->gt[g];
  if (split) { HIPCHK(hipEventRecord(e->ev_tree[g], st)); HIPCHK(hipStreamWaitEvent(sn, e->ev_tree[g], 0)); }
  const int N = std::max(1, std::min(v.G, nmax));
  const int* nev = v.n_eval + e->wave_par[g];
  const int* const eslots = v.eval_slots + (size_t)e->wave_par[g] * v.eval_stride;
  AZCHK((launch_simple<Gm, false>(e, sn, v.leaf_env, eslots, nev, N, nullptr, nullptr, v.Pout, v.Vout, nullptr, Gm::APAD)));
  if (e->bg_signal) AZCHK(raise_stop_word(e, sn));
  if (split) {
    HIPCHK(hipEventRecord(e->ev_net[g], sn));
    if (!e->ph.fr_on) HIPCHK(hipStreamWaitEvent(st, e->ev_net[g], 0));   // (a free-running wave_group waits for ev_net at its end)
  }
  return AZ_OK;
}

template <class Gm> static int set_kernel_attrs(az_engine* e) {
  if (e->cfg.oracle == AZ_ORACLE_SIMPLENET) return simple_set_kernel_attrs<Gm>();
  AZCHK((set_kernel_attrs_f<Gm, 64>(Forms<Gm, 64>{})));
  AZCHK((set_kernel_attrs_f<Gm, 128>(Forms<Gm, 128>{})));
  memset(e->d_geo, 0, sizeof e->d_geo);
  AZCHK((upload_geo<T16<Gm, 64, 11>>(e)));
  AZCHK((upload_geo<T16<Gm, 64, NTS<Gm>>>(e)));
  AZCHK((upload_geo<T16P<Gm, 64>>(e)));
  AZCHK((upload_geo<T16P<Gm, 64, 10, 9>>(e)));
  AZCHK((upload_geo<T16B<Gm, 128, 22>>(e)));
  if constexpr (NTM<Gm> > 0) AZCHK((upload_geo<T16<Gm, 64, NTM<Gm>>>(e)));
  AZCHK((upload_geo<T16<Gm, 64, 6>>(e)));
  return AZ_OK;
}

// Which tower kernel serves a launch of up to n boards.  A workgroup's layer chain is sequential and the MFMA
// pipe of a CU is shared by its resident workgroups, so the launch costs (workgroups per CU, rounded up) x (rows
// per workgroup) x (fraction of the tile-tap products it executes): k_tower16 packs 176 rows (4 Connect-Four boards),
// k_tower 128 (3 boards, every tap), k_tower16 with 3 row tiles 48 (1 board; +10 %: a third of the weight reuse, more
// barriers per row).  Measured round 2 (tools/run_config.py): Mancala 8192 slots 13.5 M sims/s on k_tower, 21.5 M on
// k_tower16 (31 of 99 products); 5x128 two groups 1.10 vs 1.20 M.  Returns a TowerForm.
// n = boards the launch is expected to hold (what the forms are priced with), nb >= n = the most it can hold (what the split
// tower's co-residency needs; the grid is sized for nb in any case and workgroups beyond the device's count leave at once).
// INVARIANT: the choice depends on a launch size the host reads from a device-written word WITHOUT synchronising
// (wave_net_f: h_nleaf), so which form serves a wave differs from run to run.  Results do not, because every fp32 tower form
// computes the same bits and every bf16 form the same bits (tests/test_net.py, tests/test_net_bf16_gpu.py force each form and compare).
// A new form must pass those cross-form equality tests before it may be returned from here.
template <class Gm, int F> static int pick_tower(const az_engine* e, int n, int nb = -1) {
  if (nb < n) nb = n;
  // split tower (k_tower16s, 128 filters): both workgroups of every pair must be resident at once -> all slot groups'
  // launches together at most num_cu workgroups (beyond that the towers queue for CUs and the split only costs: 256
  // slots in two groups 0.62 vs 0.71 M sims/s); its kernel arguments change per launch (epoch): not under hipGraph replay
  // (r4) the count runs over ALL engines of the process on this device that may launch split towers side by side (an arena has
  // two); an engine whose exchange has given up once (another process, a trainer: work this count cannot see) stays unsplit
  const bool can_split = F == 128 && !e->cfg.net_bf16 && !e->env.use_graphs && e->cfg.num_blocks <= 127 && !e->split_off &&
                         2 * std::max(std::max(1, e->ngroups), split_streams_on_device(e->device)) * ((nb + T16<Gm, F, NTS<Gm>>::TB - 1) / T16<Gm, F, NTS<Gm>>::TB) <= (e->num_cu > 0 ? e->num_cu : 256);
  if (e->env.tower_pick == TW_SPLIT && can_split) return TW_SPLIT;
  if (!e->cfg.net_bf16 && (e->env.tower_pick == TW_11 || e->env.tower_pick == TW_32 || e->env.tower_pick == TW_NTS || ((e->env.tower_pick == TW_P21 || e->env.tower_pick == TW_P19 || e->env.tower_pick == TW_P21C) && F == 64) || (e->env.tower_pick == TW_NTM && NTM<Gm> > 0))) return e->env.tower_pick;
  if (e->cfg.net_bf16) {                                           // k_tower16b: 22 (128 filters), 11 or 3 row tiles
    if (e->env.tower_pick == TW_NTS || e->env.tower_pick == TW_11) return e->env.tower_pick;
    if (e->env.tower_pick == TW_B22 && F == 128) return TW_B22;
    const long cu2 = e->num_cu > 0 ? e->num_cu : 256;
    const long a16 = (n + T16B<Gm, F>::TB - 1) / T16B<Gm, F>::TB, a3 = (n + T16B<Gm, F, NTS<Gm>>::TB - 1) / T16B<Gm, F, NTS<Gm>>::TB;
    const long per = F == 64 ? 2 : 1;                               // workgroups per CU
    // rounds x rows per workgroup x fraction of the tile-tap products executed (Geo16)
    constexpr double g16 = T16B<Gm, F>::Geo::tab.cost / (9.0 * 11), g3 = T16B<Gm, F, NTS<Gm>>::Geo::tab.cost / (9.0 * NTS<Gm>);
    const double d16 = (double)((a16 + per * cu2 - 1) / (per * cu2)) * T16B<Gm, F>::RPAD * g16;
    const double d3 = 1.1 * (double)((a3 + per * cu2 - 1) / (per * cu2)) * T16B<Gm, F, NTS<Gm>>::RPAD * g3;
    if constexpr (F == 128) {
      // 22 row tiles = twice the boards per workgroup: each weight fragment serves twice the rows (10x128, 4096 boards: 578
      // vs 684 us); only where it does not leave CUs idle that the 11-tile form would use
      constexpr double g22 = T16B<Gm, F, 22>::Geo::tab.cost / (9.0 * 22);
      const long a22 = (n + T16B<Gm, F, 22>::TB - 1) / T16B<Gm, F, 22>::TB;
      const double d22 = 0.9 * (double)((a22 + cu2 - 1) / cu2) * T16B<Gm, F, 22>::RPAD * g22;
      if (d22 <= d16 && d22 <= d3) return TW_B22;
    }
    return d3 <= d16 ? TW_NTS : TW_11;
  }
  const long cu = e->num_cu > 0 ? e->num_cu : 256;
  const long b16 = (n + T16<Gm, F>::TB - 1) / T16<Gm, F>::TB, b32 = (n + TOWER_ROWS / Gm::P - 1) / (TOWER_ROWS / Gm::P);
  const long b3 = (n + T16<Gm, F, NTS<Gm>>::TB - 1) / T16<Gm, F, NTS<Gm>>::TB;
  // the k_tower16 family executes only the (tile, tap) products that touch the board (Geo16): cost x executed fraction
  constexpr double f16 = T16<Gm, F>::Geo::tab.cost / (9.0 * T16<Gm, F>::NTILE), f3 = T16<Gm, F, NTS<Gm>>::Geo::tab.cost / (9.0 * NTS<Gm>),
                   f21 = T16P<Gm, 64>::Geo::tab.cost / (9.0 * T16P<Gm, 64>::NTW);
  const double c16 = (double)((b16 + cu - 1) / cu) * T16<Gm, F>::RPAD * f16;
  const double c32 = (double)((b32 + cu - 1) / cu) * TOWER_ROWS;     // k_tower (32x32x2) computes every tap
  const double c3 = 1.1 * (double)((b3 + cu - 1) / cu) * T16<Gm, F, NTS<Gm>>::RPAD * f3;
  if (c3 <= c16 && c3 <= c32) return can_split && e->env.tower_pick != TW_NTS ? TW_SPLIT : TW_NTS;
  // (r4) the exact-fit variant (NTM tiles: whole boards, no padding rows): where its workgroups fill the CUs evenly it beats
  // the 11-tile form by the padding rows and by the last, partly filled round of workgroups
  if constexpr (NTM<Gm> > 0) {
    using TM = T16<Gm, F, NTM<Gm>>;
    constexpr double fm = TM::Geo::tab.cost / (9.0 * NTM<Gm>);
    const long bm = (n + TM::TB - 1) / TM::TB;
    // +3 %: fewer rows per weight fragment; the half-size form at 128 filters +20 %: half the rows per weight fragment there (the
    // vector-memory path that streams the weights is what a 128-filter layer waits for: DESIGN.md 4d, the trainer's 6-tile layer)
    const double cm = (Gm::P == 42 && F == 128 ? 1.2 : 1.03) * (double)((bm + cu - 1) / cu) * TM::RPAD * fm;
    if (cm < c16 && cm < c32 && (F != 64 || cm < (double)(((n + T16P<Gm, 64>::TB - 1) / T16P<Gm, 64>::TB + cu - 1) / cu) * T16P<Gm, 64>::RPAD * f21)) return TW_NTM;
  }
  // paired k_tower16x2: 336 rows = 8 Connect-Four boards per workgroup, no padding rows.  Its 92 KB of LDS allow one
  // workgroup per CU, so with several slot groups the groups' towers cannot interleave on a CU (Connect-Four, two groups:
  // 3.80 vs 4.11 M sims/s in round 1): +8 % on its cost there
  if (F == 64) {
    const long b21 = (n + T16P<Gm, 64>::TB - 1) / T16P<Gm, 64>::TB;
    const double c21 = (double)((b21 + cu - 1) / cu) * T16P<Gm, 64>::RPAD * f21 * (e->ngroups > 1 ? 1.08 : 1.0);
    if (c21 < c16 && c21 < c32) return TW_P21;
  }
  return c16 <= c32 ? TW_11 : TW_32;
}
// publish areas of k_tower16s for the launches that write `hfeat` (one feature buffer = one stream at a time)
template <class Gm> static int xch_slot(az_engine* e, const float* hfeat, unsigned long long** xch, unsigned long long* epoch) {
  using T = T16S<Gm, 128>;
  const size_t words = (size_t)(e->num_cu > 0 ? e->num_cu : 256) * T::XCH_WORDS;
  int slot = AZ_MAX_GROUPS;
  for (int g = 0; g < e->ngroups; ++g) if (hfeat == e->g_hfeat[g]) slot = g;
  if (!e->xch[slot]) {
    // zeroed: tag 0 is never expected.  The clear runs on e->stream while the launch that follows is on the group's own
    // (non-blocking) stream: it must have finished before that kernel polls the area -- recycled device memory can hold an
    // earlier engine's words, and every engine's epochs start at 1, so stale tags WOULD match (seen once in a full test
    // run: a two-group engine created after other engines had been freed evaluated garbage)
    AZCHK(dalloc(e, &e->xch[slot], words));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  // a tag carries 24 bits of the launch epoch: before they repeat, every area is cleared (an area that a long run of
  // smaller launches has not touched could otherwise still hold words with the tag of exactly 2^24 launches ago)
  if (((e->xch_epoch + 1) & 0xFFFFFFull) == 0) {
    AZCHK(sync_all(e));
    for (int k = 0; k <= AZ_MAX_GROUPS; ++k) if (e->xch[k]) HIPCHK(hipMemset(e->xch[k], 0, words * sizeof(unsigned long long)));
    ++e->xch_epoch;                                                  // skip the epoch whose tags would start at 0
  }
  *xch = e->xch[slot];
  *epoch = ++e->xch_epoch;
  if (e->env.xch_fail_at > 0 && ++e->xch_launches == e->env.xch_fail_at) *epoch |= 1ull << 63;   // tests: this launch loses a partner (AZHIP_XCH_FAIL_AT)
  return AZ_OK;
}
// Dense heads of n_max boards: 16-board tiles (k_heads16: a quarter of the chain latency, 23 instead of 43 us per launch
// at 64 filters whatever the size) unless several slot groups run big launches side by side -- there the heads hide
// under the other group's tower anyway and twice as many workgroups asking for a CU cost 1 % (0.867 vs 0.857 ms per
// step, two groups of 2048): 32-board tiles (k_heads_mfma).  The vector-ALU kernel when the head filters do not fit
// the MFMA fragments.
static constexpr int HEADS16_MAX_BOARDS = 1024;
template <class Gm, int F>
static int launch_heads(az_engine* e, hipStream_t st, const float* hfeat, const GEnv* envs, const int* eslots, const int* n_ptr, int n_max,
                        const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride) {
  const bool small = e->env.heads_pick == 16 || (e->env.heads_pick != 32 && (n_max <= HEADS16_MAX_BOARDS || e->ngroups == 1));
  const int tiles = (n_max + 15) / 16;
  if (e->net.hd16_ok && small && 2 * tiles <= (e->num_cu > 0 ? e->num_cu : 256))    // value and policy tiles in two workgroups, features staged in LDS
    LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads16<Gm, F, true>), 2 * tiles, (H16<Gm, F, true>::THREADS), (H16<Gm, F, true>::BYTES), e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
  else if (e->net.hd16_ok && small)
    LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads16<Gm, F, false>), tiles, (H16<Gm, F, false>::THREADS), (H16<Gm, F, false>::BYTES), e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
  else if (e->net.hd_ok)
    LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads_mfma<Gm, F>), (n_max + 31) / 32, 64 * (F / 32 + HEADS_NPT<Gm>), 0, e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
  else
    LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads<Gm, F>), (n_max + 3) / 4, 4 * (F + HEADS_LP<Gm>), 0, e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
  return AZ_OK;
}
// Where a tower launch finds its boards (envs[eslots[i]], device count in n_ptr; FROM_PLANES: X) and leaves the head features; xerr = the
// error word a split tower's exchange reports to (e->v.err in the network seam, the group's DView::xerr in a wave)
// stop / stop_val: the stop word of the background search this launch runs over and the value that raises it (forms with STOP; NULL: none)
struct TowerIn { float* hfeat; const GEnv* envs; const int* eslots; const int* n_ptr; const float* X; int* xerr; int* stop = nullptr; int stop_val = 0; };
static const char* game_name(const az_engine* e) {
  static const char* const gn[] = {"ConnectFour", "TicTacToe", "Mancala", "Go9Planes"};
  return gn[e->cfg.game];
}
template <class D, bool FROM_PLANES> static int launch_form(az_engine* e, hipStream_t st, int n, const TowerIn& in) {
  if constexpr (!D::OK) return fail(AZ_ERR_STATE, "tower form %d does not exist for this network", (int)D::ID);
  else {
    using T = typename D::T;
    D::name(e->last_tower, sizeof e->last_tower, game_name(e));
    e->tower_hist[D::HIST]++;
    e->next_exec = D::frac();
    const int tiles = (n + T::TB - 1) / T::TB;
    if constexpr (D::ID == TW_SPLIT) {
      unsigned long long* xa; unsigned long long ep;
      AZCHK(xch_slot<typename T::Game>(e, in.hfeat, &xa, &ep));
      LAUNCH_ON(e, st, AZ_K_TOWER, n, (D::template K<FROM_PLANES>), T::SPLIT * tiles, T::THREADS, T::BYTES, D::net(e), in.envs, in.eslots, in.n_ptr, n, in.X, in.hfeat,
                xa, ep, in.xerr, e->d_xflag);
    } else if constexpr (D::STOP)
      LAUNCH_ON(e, st, AZ_K_TOWER, n, (D::template K<FROM_PLANES>), tiles, T::THREADS, T::BYTES, D::net(e), in.envs, in.eslots, in.n_ptr, n, in.X, in.hfeat,
                in.stop, in.stop_val, e->num_cu > 0 ? e->num_cu : 256);
    else
      LAUNCH_ON(e, st, AZ_K_TOWER, n, (D::template K<FROM_PLANES>), tiles, T::THREADS, T::BYTES, D::net(e), in.envs, in.eslots, in.n_ptr, n, in.X, in.hfeat);
    return AZ_OK;
  }
}
// The one tower launch: form `form` (what pick_tower returned) of the engine's network on up to n boards.  Sets last_tower, tower_hist
// and next_exec; the grid is sized for n and workgroups beyond the device's count leave at once.
template <class Gm, int F, bool FROM_PLANES, class... D>
static int launch_tower(FormList<D...>, az_engine* e, hipStream_t st, int form, int n, const TowerIn& in) {
  const bool bf16 = e->cfg.net_bf16 != 0;
  int r = 1;                                                        // > 0: no descriptor matched
  (void)((D::ID == form && D::BF16 == bf16 && ((r = launch_form<D, FROM_PLANES>(e, st, n, in)), true)) || ...);
  return r <= 0 ? r : fail(AZ_ERR_STATE, "no tower form %d", form);
}
template <class Gm, int F, bool FROM_PLANES> static int launch_tower(az_engine* e, hipStream_t st, int form, int n, const TowerIn& in) {
  return launch_tower<Gm, F, FROM_PLANES>(Forms<Gm, F>{}, e, st, form, n, in);
}
template <class Gm, int F, bool FROM_PLANES>
static int launch_net_f(az_engine* e, hipStream_t st, float* hfeat, const GEnv* envs, const int* eslots, const int* n_ptr, int n_max, const float* X,
                        const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride) {
  if (n_max <= 0) return AZ_OK;
  AZCHK((launch_tower<Gm, F, FROM_PLANES>(e, st, pick_tower<Gm, F>(e, n_max), n_max, TowerIn{hfeat, envs, eslots, n_ptr, X, e->v.err})));
  return launch_heads<Gm, F>(e, st, hfeat, envs, eslots, n_ptr, n_max, Amask, Pout, Vout, Pinv, pstride);
}
// launches tower + heads on `n` boards (device count in n_ptr when given)
template <class Gm, bool FROM_PLANES>
static int launch_net(az_engine* e, hipStream_t st, float* hfeat, const GEnv* envs, const int* eslots, const int* n_ptr, int n_max, const float* X,
                      const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride) {
  if (e->cfg.oracle == AZ_ORACLE_SIMPLENET) return launch_simple<Gm, FROM_PLANES>(e, st, envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride);
  if (e->cfg.num_filters == 128) return launch_net_f<Gm, 128, FROM_PLANES>(e, st, hfeat, envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride);
  return launch_net_f<Gm, 64, FROM_PLANES>(e, st, hfeat, envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride);
}


template <class Gm, int F> static int wave_net_f(az_engine* e, int g, bool split, int nmax) {
  constexpr int L = Gm::APAD;
  const DView& v = e->gv[g];
  hipStream_t st = e->gs[g], sn = e->gt[g];
  const int G = v.G;
  if (split) { HIPCHK(hipEventRecord(e->ev_tree[g], st)); HIPCHK(hipStreamWaitEvent(sn, e->ev_tree[g], 0)); }
  // N = upper bound of this wave's leaves: the group's active slots (a draining phase or a partial explore! launches
  // -- and picks its tower kernel -- for what is left, not for the group's capacity)
  const int N = std::max(1, std::min(G, nmax));
  const int* nev = v.n_eval + e->wave_par[g];                      // the leaf counter of this wave (k_tree)
  const int* const eslots = v.eval_slots + (size_t)e->wave_par[g] * v.eval_stride;   // ... and its batch -> slot list
  // how many boards the launch will really hold: with the evaluation cache answering part of every wave, what the device
  // reported for the group's last completed wave (+ 1/8: a launch priced too small costs more than one priced too large)
  int npick = N;
  if (v.nleaf_host) { const int seen = ((volatile int*)e->h_nleaf)[g]; if (seen >= 0) npick = std::max(1, std::min(N, seen + seen / 8 + 8)); }
  int tw = pick_tower<Gm, F>(e, npick, N);
  if (tw == TW_P21 && e->ph.fr_on && e->ngroups == 1 && e->env.tower_pick == 0 && e->ph.fr_kbg > 0 && v.nleaf_host && v.needy_host) {
    // The paired tower beside the side streams' kernels (resnet16.h k_tower16x2c): a CU that holds a workgroup of the background search
    // (256 threads = 32 Connect-Four slots of the needy list) takes no workgroup of the 198-register form for as long as that search
    // runs.  Measured: in the steady state (~8 such workgroups on average, more in some waves) the launch gains a round of workgroups
    // beyond ~478 of its 512; the margin of 14 is that measurement (the move step is not part of it: within 96 registers it changes
    // nothing).  Where the counts the device reported for the previous wave say that this adds a round, the 176-register form serves
    // the launch.
    const int cu = e->num_cu > 0 ? e->num_cu : 256;
    const int seen = ((volatile int*)e->h_nleaf)[g], needy = ((volatile int*)e->h_needy)[g];
    if (seen > 0) {
      constexpr int TB21 = T16P<Gm, 64>::TB;
      const int wgs = (seen + TB21 - 1) / TB21, rounds = (wgs + cu - 1) / cu, bg = (std::max(needy, 0) * L + 255) / 256;
      if (wgs > rounds * (cu - bg) - 14) tw = TW_P21C;
    }
  }
  // the background search's stop word: a paired form raises it itself, from its last round of workgroups (resnet16.h tower16x2_body)
  const bool tower_stops = e->bg_signal && F == 64 && !e->cfg.net_bf16 && (tw == TW_P21 || tw == TW_P19 || tw == TW_P21C);
  TowerIn in{e->g_hfeat[g], v.leaf_env, eslots, nev, nullptr, v.xerr};
  if (tower_stops) { in.stop = e->d_bg_stop; in.stop_val = e->bg_seq; }
  bool mixed = false;
  if constexpr (FormMixed<Gm, F>::OK) {
    // (r6, measured, off unless AZHIP_TOWER_MIXED=1) A batch between 15 and 16 boards per CU (a free-running wave's ~3800 boards at 4096 slots on
    // 256 CUs) costs two rounds of the 8-board form whatever its size.  As ONE launch of cu 8-board workgroups and up to cu 7-board ones
    // (k_tower16x2m) it is slower, 1.09 ms per wave instead of 0.80 (profiles/r6/README.md): a workgroup's time hardly shrinks with its
    // boards, because every workgroup streams the same 1.5 MB of weights through its CU's vector-memory path.
    using M = FormMixed<Gm, F>;
    using T8 = typename M::T; using T7 = typename M::T7;
    const int cu = e->num_cu > 0 ? e->num_cu : 256, first = cu * T8::TB;
    const int seen = v.nleaf_host ? ((volatile int*)e->h_nleaf)[g] : -1;
    if (tw == TW_P21 && e->env.tower_mixed && e->env.tower_pick == 0 && N > first && seen > first && seen + 16 <= first + cu * T7::TB) {
      mixed = true;
      M::name(e->last_tower, sizeof e->last_tower, game_name(e));
      e->tower_hist[M::HIST]++;
      // the launch holds boards of both forms: price the executed fraction by their shares of the expected batch
      e->next_exec = (first * geo_frac<T8>() + (seen - first) * geo_frac<T7>()) / (double)seen;
      LAUNCH_ON(e, sn, AZ_K_TOWER, N, (M::template K<false>), cu + (N - first + T7::TB - 1) / T7::TB, T8::THREADS, T8::BYTES, M::net(e), in.envs, in.eslots, in.n_ptr, N, in.X, in.hfeat, cu, in.stop, in.stop_val);
    }
  }
  if (!mixed) AZCHK((launch_tower<Gm, F, false>(e, sn, tw, N, in)));
  // Free-running phase: the heads follow the tower on the network stream and the tree stream is NOT made to wait here -- the caller
  // (wave_group, azhip.hip) first queues the group's move step and its background search behind k_tree, then the wait for ev_net: both
  // run under this tower.
  const bool fr = e->ph.fr_on && split;
  if (e->bg_signal && !tower_stops) {
    // a form that does not raise the word itself.  The tower has run: the background search of this wave winds up while the heads run.  The
    // word is set from a stream of its own behind an event (a one-thread launch IN the wave's stream sat 7.6 us between tower and heads)
    AZCHK(raise_stop_word(e, sn));
  }
  if (split && !fr) { HIPCHK(hipEventRecord(e->ev_net[g], sn)); HIPCHK(hipStreamWaitEvent(st, e->ev_net[g], 0)); }
  AZCHK((launch_heads<Gm, F>(e, fr ? sn : st, e->g_hfeat[g], v.leaf_env, eslots, nev, N, (const float*)nullptr, v.Pout, v.Vout, (float*)nullptr, L)));
  if (fr) HIPCHK(hipEventRecord(e->ev_net[g], sn));
  return AZ_OK;
}
template <class Gm> static int wave_net(az_engine* e, int g, bool split, int nmax) {
  if (e->cfg.oracle == AZ_ORACLE_SIMPLENET) return wave_simple<Gm>(e, g, split, nmax);
  return e->cfg.num_filters == 128 ? wave_net_f<Gm, 128>(e, g, split, nmax) : wave_net_f<Gm, 64>(e, g, split, nmax);
}

// the three entry points of one game's translation unit
#define AZ_NET_GAME_TU(Gm, sfx)                                                                                              \
  int net_set_kernel_attrs_##sfx(az_engine* e) { return set_kernel_attrs<Gm>(e); }                                                      \
  int net_launch_##sfx(az_engine* e, hipStream_t st, bool from_planes, float* hfeat, const GEnv* envs, const int* eslots,    \
                       const int* n_ptr, int n_max, const float* X, const float* Amask, float* Pout, float* Vout, float* Pinv, \
                       int pstride) {                                                                                        \
    return from_planes ? launch_net<Gm, true>(e, st, hfeat, envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride)  \
                       : launch_net<Gm, false>(e, st, hfeat, envs, eslots, n_ptr, n_max, X, Amask, Pout, Vout, Pinv, pstride); \
  }                                                                                                                          \
  int net_wave_##sfx(az_engine* e, int g, bool split, int nmax) { return wave_net<Gm>(e, g, split, nmax); }                  \
  int net_geometry_##sfx(int which, uint16_t* out, int64_t cap, int* rows, int* products) {                                  \
    return which == 0 ? geometry_out<typename T16<Gm, 64, 11>::Geo>(out, cap, rows, products)                                \
         : which == 1 ? geometry_out<typename T16<Gm, 64, NTS<Gm>>::Geo>(out, cap, rows, products)                                 \
         : which == 2 ? geometry_out<typename T16P<Gm, 64>::Geo>(out, cap, rows, products)                                   \
                      : geometry_out<typename T16B<Gm, 128, 22>::Geo>(out, cap, rows, products);                             \
  }
