// net_impl.h -- the launches of the network kernels (resnet.h, resnet16.h), templated on the game: the tower forms' descriptors and
// the launch of what tower_choice.h chooses among them.  Instantiated once per game in net_c4.hip / net_ttt.hip /
// net_mancala.hip (three translation units, so that the big fully unrolled tower kernels compile in parallel);
// net.hip dispatches on the engine's game.
#pragma once
#include "engine.h"

// ---- the tower forms --------------------------------------------------------------------------------------------------------
// One descriptor per form, templated on the game and the filter count, states everything a launch needs:
//   ID, OK   its TowerForm (tower_choice.h) and whether the form exists for this game and F
//   BF16     which network it serves (choose_tower returns TW_NTS / TW_11 for both: the engine's network decides between the two descriptors)
//   T        its layout struct: T::TB boards and T::RPAD rows per workgroup, T::THREADS, T::BYTES of LDS, T::Geo / T::GEO its row permutation table
//   K        its kernel, for FROM_PLANES false and true;  net(e): the fragments that kernel takes
//   frac()   the fraction of a 3x3 convolution's (row tile, tap) products it executes (Geo16 skips the products whose tap falls off the
//            board for a whole tile; k_tower computes every tap).  az_prof.exec_units weighs a launch's boards with it, so that a roofline
//            can count the work DONE instead of the dense convolution's
//   HIST     its tower_hist bucket;  name(): its az_net_last_kernel spelling
//   STOP     its kernel takes the background search's stop word (TowerIn::stop) and raises it from its last round of workgroups
// set_kernel_attrs_f, upload_geos, tower_table and launch_tower walk Forms<Gm, F>; a form's properties are stated nowhere else.
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
  struct T { static constexpr int RPAD = TOWER_ROWS, TB = RPAD / Gm::P, THREADS = TowerCfg<F>::THREADS, BYTES = TowerLds<F>::BYTES; };
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
// what the choice (tower_choice.h) knows of form D, and of all forms of one game and F
template <class D, int F> static constexpr TowerFacts facts() {
  if constexpr (!D::OK) return TowerFacts{D::ID, D::BF16};
  else return TowerFacts{D::ID, D::BF16, true, D::STOP, D::T::TB, D::T::RPAD, D::frac(), D::BF16 && F == 64 ? 2 : 1};
}
template <class Gm, int F, class... D> static TowerTable tower_table(FormList<D...>) {
  static constexpr TowerFacts forms[] = {facts<D, F>()...};
  return TowerTable{forms, (int)sizeof...(D), F, Gm::P, Gm::APAD};
}
template <class Gm, int F> static TowerTable tower_table() { return tower_table<Gm, F>(Forms<Gm, F>{}); }

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
// ... of every form that exists (k_tower has no table)
template <class D> static int upload_form_geo(az_engine* e) {
  if constexpr (D::OK && D::ID != TW_32) AZCHK((upload_geo<typename D::T>(e)));
  return AZ_OK;
}
template <class... D> static int upload_geos(az_engine* e, FormList<D...>) {
  int r = AZ_OK;
  (void)(((r = upload_form_geo<D>(e)) == AZ_OK) && ...);
  return r;
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
// The network part of one search wave of slot group g, for both kinds of engine: the group's network stream `sn` starts behind its tree
// stream (split: they are two), net(sn) launches the network there and sees to the stop word, and ev_net marks its end.  The tree stream
// waits for that here -- but not in a free-running phase: there the caller (wave_group, azhip.hip) first queues the group's move step and
// its background search behind k_tree, then the wait for ev_net: both run under this network.
template <class Net> static int wave_frame(az_engine* e, int g, bool split, Net net) {
  hipStream_t st = e->gs[g], sn = e->gt[g];
  if (split) { HIPCHK(hipEventRecord(e->ev_tree[g], st)); HIPCHK(hipStreamWaitEvent(sn, e->ev_tree[g], 0)); }
  AZCHK(net(sn));
  if (split) {
    HIPCHK(hipEventRecord(e->ev_net[g], sn));
    if (!e->ph.fr_on) HIPCHK(hipStreamWaitEvent(st, e->ev_net[g], 0));
  }
  return AZ_OK;
}
// The leaves of that wave.  N = their upper bound: the group's active slots (a draining phase or a partial explore! launches -- and picks
// its tower kernel -- for what is left, not for the group's capacity); nev = the leaf counter of this wave (k_tree), eslots = its batch ->
// slot list
struct WaveLeaves { int N; const int* nev; const int* eslots; };
static WaveLeaves wave_leaves(const az_engine* e, int g, int nmax) {
  const DView& v = e->gv[g];
  return WaveLeaves{std::max(1, std::min(v.G, nmax)), v.n_eval + e->wave_par[g], v.eval_slots + (size_t)e->wave_par[g] * v.eval_stride};
}
// SimpleNet: the one launch takes the place of tower + heads, and the background search's stop word is raised behind it (k_simplenet does
// not raise it itself).
template <class Gm> static int wave_simple(az_engine* e, int g, bool split, int nmax) {
  const DView& v = e->gv[g];
  const WaveLeaves w = wave_leaves(e, g, nmax);
  return wave_frame(e, g, split, [&](hipStream_t sn) -> int {
    AZCHK((launch_simple<Gm, false>(e, sn, v.leaf_env, w.eslots, w.nev, w.N, nullptr, nullptr, v.Pout, v.Vout, nullptr, Gm::APAD)));
    if (e->bg_signal) AZCHK(raise_stop_word(e, sn));
    return AZ_OK;
  });
}

template <class Gm> static int set_kernel_attrs(az_engine* e) {
  if (e->cfg.oracle == AZ_ORACLE_SIMPLENET) return simple_set_kernel_attrs<Gm>();
  AZCHK((set_kernel_attrs_f<Gm, 64>(Forms<Gm, 64>{})));
  AZCHK((set_kernel_attrs_f<Gm, 128>(Forms<Gm, 128>{})));
  memset(e->d_geo, 0, sizeof e->d_geo);
  AZCHK(upload_geos(e, Forms<Gm, 64>{}));
  AZCHK(upload_geos(e, Forms<Gm, 128>{}));
  AZCHK((upload_geo<typename FormMixed<Gm, 64>::T7>(e)));
  AZCHK((upload_geo<T16<Gm, 64, 6>>(e)));                           // the trainer's 6-tile layer (train.hip k_conv16_layer)
  return AZ_OK;
}

// What a launch of up to n boards of this engine asks the choice (tower_choice.h) with; a wave adds its own fields
static TowerAsk tower_ask(const az_engine* e, int n) {
  TowerAsk a;
  a.n = n; a.num_cu = e->num_cu; a.ngroups = e->ngroups;
  a.bf16 = e->cfg.net_bf16 != 0; a.num_blocks = e->cfg.num_blocks; a.tower_pick = e->env.tower_pick; a.use_graphs = e->env.use_graphs != 0; a.split_off = e->split_off;
  a.split_streams = split_streams_on_device(e->device);
  return a;
}
// publish areas of k_tower16s for the launches that write `hfeat` (one feature buffer = one stream at a time)
template <class Gm> static int xch_slot(az_engine* e, const float* hfeat, unsigned long long** xch, unsigned long long* epoch) {
  using T = T16S<Gm, 128>;
  const size_t words = (size_t)cus(e->num_cu) * T::XCH_WORDS;
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
// the dense heads of n_max boards, by the kernel choose_heads (tower_choice.h) names
template <class Gm, int F>
static int launch_heads(az_engine* e, hipStream_t st, const float* hfeat, const GEnv* envs, const int* eslots, const int* n_ptr, int n_max,
                        const float* Amask, float* Pout, float* Vout, float* Pinv, int pstride) {
  const int tiles = (n_max + 15) / 16;
  switch (choose_heads(e->env.heads_pick, e->net.hd16_ok, e->net.hd_ok, n_max, e->ngroups, e->num_cu)) {
    case HD_16_STAGED:
      LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads16<Gm, F, true>), 2 * tiles, (H16<Gm, F, true>::THREADS), (H16<Gm, F, true>::BYTES), e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
      break;
    case HD_16:
      LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads16<Gm, F, false>), tiles, (H16<Gm, F, false>::THREADS), (H16<Gm, F, false>::BYTES), e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
      break;
    case HD_MFMA:
      LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads_mfma<Gm, F>), (n_max + 31) / 32, 64 * (F / 32 + HEADS_NPT<Gm>), 0, e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
      break;
    case HD_VALU:
      LAUNCH_ON(e, st, AZ_K_HEADS, n_max, (k_heads<Gm, F>), (n_max + 3) / 4, 4 * (F + HEADS_LP<Gm>), 0, e->net, envs, eslots, n_ptr, n_max, Amask, hfeat, Pout, Vout, Pinv, pstride);
      break;
  }
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
                in.stop, in.stop_val, cus(e->num_cu));
    else
      LAUNCH_ON(e, st, AZ_K_TOWER, n, (D::template K<FROM_PLANES>), tiles, T::THREADS, T::BYTES, D::net(e), in.envs, in.eslots, in.n_ptr, n, in.X, in.hfeat);
    return AZ_OK;
  }
}
// The one tower launch: form `form` (what choose_tower returned) of the engine's network on up to n boards.  Sets last_tower, tower_hist
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
  AZCHK((launch_tower<Gm, F, FROM_PLANES>(e, st, choose_tower(tower_table<Gm, F>(), tower_ask(e, n_max)), n_max, TowerIn{hfeat, envs, eslots, n_ptr, X, e->v.err})));
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


// ResNet: tower, then heads.  The tower runs on the network stream.  Outside a free-running phase the heads follow on the tree stream, once it
// has met the network stream; in one they follow the tower on the network stream, so that the tree stream is free meanwhile (wave_frame).
template <class Gm, int F> static int wave_net_f(az_engine* e, int g, bool split, int nmax) {
  const DView& v = e->gv[g];
  const WaveLeaves w = wave_leaves(e, g, nmax);
  const bool fr = e->ph.fr_on && split;
  auto heads = [&](hipStream_t s) -> int {
    return launch_heads<Gm, F>(e, s, e->g_hfeat[g], v.leaf_env, w.eslots, w.nev, w.N, (const float*)nullptr, v.Pout, v.Vout, (float*)nullptr, Gm::APAD);
  };
  AZCHK(wave_frame(e, g, split, [&](hipStream_t sn) -> int {
    TowerAsk ask = tower_ask(e, w.N);
    ask.fr_on = e->ph.fr_on; ask.fr_kbg = e->ph.fr_kbg; ask.tower_mixed = e->env.tower_mixed; ask.bg_signal = e->bg_signal;
    // the device writes these words while the host reads them: ONE read of each per wave, so that every rule sees the same numbers
    if (v.nleaf_host) ask.seen = ((volatile int*)e->h_nleaf)[g];
    if (v.needy_host) { ask.needy = ((volatile int*)e->h_needy)[g]; ask.needy_on = true; }
    const WaveTower tw = choose_wave_tower(tower_table<Gm, F>(), ask);
    TowerIn in{e->g_hfeat[g], v.leaf_env, w.eslots, w.nev, nullptr, v.xerr};
    if (tw.tower_stops) { in.stop = e->d_bg_stop; in.stop_val = e->bg_seq; }
    if constexpr (FormMixed<Gm, F>::OK) {
      if (tw.mixed) {
        // workgroups 0 .. cu - 1 hold 8 boards each, the rest 7
        using M = FormMixed<Gm, F>;
        using T8 = typename M::T; using T7 = typename M::T7;
        const int cu = cus(e->num_cu), first = cu * T8::TB;
        M::name(e->last_tower, sizeof e->last_tower, game_name(e));
        e->tower_hist[M::HIST]++;
        // the launch holds boards of both forms: price the executed fraction by their shares of the expected batch
        e->next_exec = (first * geo_frac<T8>() + (ask.seen - first) * geo_frac<T7>()) / (double)ask.seen;
        LAUNCH_ON(e, sn, AZ_K_TOWER, w.N, (M::template K<false>), cu + (w.N - first + T7::TB - 1) / T7::TB, T8::THREADS, T8::BYTES, M::net(e), in.envs, in.eslots, in.n_ptr, w.N, in.X, in.hfeat, cu, in.stop, in.stop_val);
      }
    }
    if (!tw.mixed) AZCHK((launch_tower<Gm, F, false>(e, sn, tw.form, w.N, in)));
    // a form that does not raise the word itself.  The tower has run: the background search of this wave winds up while the heads run
    if (e->bg_signal && !tw.tower_stops) AZCHK(raise_stop_word(e, sn));
    return fr ? heads(sn) : AZ_OK;
  }));
  return fr ? AZ_OK : heads(e->gs[g]);
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
