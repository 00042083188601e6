// minmax.hip -- host side of the MinMax player (Benchmark.MinMaxTS, src/benchmark.jl:179-194 -> src/minmax.jl): the entry points
// az_minmax_* / az_game_heuristic / az_engine_set_minmax of include/azhip.h and the launches az_arena_run uses.  Kernels: minmax.h.
#include "minmax.h"

static int check_minmax_cfg(const az_minmax_cfg* c) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "az_minmax_cfg is NULL");
  if (c->struct_size != (int32_t)sizeof(az_minmax_cfg)) return fail(AZ_ERR_BAD_ARG, "az_minmax_cfg.struct_size = %d, expected %d (call az_minmax_cfg_init)", (int)c->struct_size, (int)sizeof(az_minmax_cfg));
  if (c->depth < 1 || c->depth > AZ_MINMAX_MAX_DEPTH) return fail(AZ_ERR_BAD_ARG, "minmax depth %d outside 1..%d", (int)c->depth, AZ_MINMAX_MAX_DEPTH);
  if (!std::isfinite(c->tau) || c->tau < 0.0) return fail(AZ_ERR_BAD_ARG, "minmax tau must be finite and >= 0");
  if (!std::isfinite(c->gamma) || c->gamma <= 0.0) return fail(AZ_ERR_BAD_ARG, "minmax gamma must be finite and > 0");
  return AZ_OK;
}
static int check_minmax_game(const az_engine* e) {
  if (e->cfg.game == AZ_GAME_GO9_PLANES) return fail(AZ_ERR_BAD_ARG, "the 9x9x4 plane geometry has no device twin: no MinMax player for game %d", (int)e->cfg.game);
  return AZ_OK;
}

extern "C" int az_minmax_cfg_init(az_minmax_cfg* cfg) {
  if (!cfg) return fail(AZ_ERR_BAD_ARG, "az_minmax_cfg is NULL");
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (int32_t)sizeof(az_minmax_cfg);
  cfg->depth = 5;
  cfg->amplify_rewards = 0;
  cfg->tau = 0.0;
  cfg->gamma = 1.0;
  return AZ_OK;
}

extern "C" int az_minmax_policy(const double* q, int32_t n, double tau, double* pi) {
  if (!q || !pi) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  if (n < 1 || n > AZ_MAX_ACTIONS) return fail(AZ_ERR_BAD_ARG, "n = %d outside 1..%d", (int)n, AZ_MAX_ACTIONS);
  if (!std::isfinite(tau) || tau < 0.0) return fail(AZ_ERR_BAD_ARG, "minmax tau must be finite and >= 0");
  for (int i = 0; i < n; ++i) if (q[i] != q[i]) return fail(AZ_ERR_BAD_ARG, "q[%d] is NaN", i);
  minmax_policy(q, n, tau, pi);
  return AZ_OK;
}

extern "C" int az_engine_set_minmax(az_engine* e, const az_minmax_cfg* cfg) {
  if (cfg) AZCHK(check_minmax_cfg(cfg));
  ENGINE(e);
  if (e->ph.running) return fail(AZ_ERR_STATE, "self-play in progress");
  if (!cfg) { e->mm_on = false; return AZ_OK; }
  AZCHK(check_minmax_game(e));
  e->mm = *cfg;
  e->mm_on = true;
  return AZ_OK;
}

// room for n roots and their q-values
static int mm_reserve(az_engine* e, int n) {
  if (n <= e->mm_cap) return AZ_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  for (void* old : {(void*)e->d_mm_roots, (void*)e->d_mm_q}) if (old) {
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), old), e->allocs.end());
    (void)hipFree(old);
  }
  e->alloc_bytes -= (size_t)e->mm_cap * (sizeof(GEnv) + sizeof(double) * AZ_MAX_ACTIONS);
  e->d_mm_roots = nullptr; e->d_mm_q = nullptr; e->mm_cap = 0;
  const int cap = std::max(n, 256);
  AZCHK(dalloc(e, &e->d_mm_roots, (size_t)cap, false));
  AZCHK(dalloc(e, &e->d_mm_q, (size_t)cap * AZ_MAX_ACTIONS, false));
  e->mm_cap = cap;
  return AZ_OK;
}

template <class Gm>
static int mm_launch(az_engine* e, const az_minmax_cfg& c, const GEnv* roots, int n) {
  AZCHK(mm_reserve(e, n));
  HIPCHK(hipMemcpyAsync(e->d_mm_roots, roots, sizeof(GEnv) * (size_t)n, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL((k_minmax<Gm>), dim3((unsigned)n * (unsigned)Gm::A), dim3(MM_THREADS), 0, e->stream,
                     (const GEnv*)e->d_mm_roots, n, (int)c.depth, (int)(c.amplify_rewards != 0), c.gamma, e->d_mm_q);
  HIPCHK(hipGetLastError());
  return AZ_OK;
}

int minmax_launch(az_engine* e, const std::vector<GEnv>& roots) {
  if (roots.empty()) return AZ_OK;
  DISPATCH_GAME(e->cfg.game, AZCHK(mm_launch<Gm>(e, e->mm, roots.data(), (int)roots.size())));
  return AZ_OK;
}
int minmax_fetch(az_engine* e, int n, std::vector<double>& Q) {
  Q.resize((size_t)n * AZ_MAX_ACTIONS);
  if (!n) return AZ_OK;
  HIPCHK(hipMemcpyAsync(Q.data(), e->d_mm_q, sizeof(double) * Q.size(), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return AZ_OK;
}

extern "C" int az_minmax_qvalues(az_engine* e, const az_minmax_cfg* cfg, const uint64_t* keys, int32_t n, double* Q, double* pi) {
  AZCHK(check_minmax_cfg(cfg));
  ENGINE(e);
  AZCHK(check_minmax_game(e));
  if (n < 0 || (n > 0 && (!keys || !Q))) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  if (n == 0) return AZ_OK;
  if ((long long)n * e->gi.A > 0x7fffffffLL) return fail(AZ_ERR_BAD_ARG, "n = %d states are more than one launch takes", (int)n);
  std::vector<GEnv> roots((size_t)n);
  DISPATCH_GAME(e->cfg.game, {
    for (int i = 0; i < n; ++i) {
      roots[i] = Gm::from_key(keys[2 * i], keys[2 * i + 1]);
      if (roots[i].fin & 1) return fail(AZ_ERR_BAD_ARG, "state %d is terminated: qvalue needs a state with a move to play (minmax.jl:29)", i);
    }
    AZCHK(mm_launch<Gm>(e, *cfg, roots.data(), n));
  });
  std::vector<double> q;
  AZCHK(minmax_fetch(e, n, q));
  const int A = e->gi.A;
  for (int i = 0; i < n; ++i) {
    double qa[AZ_MAX_ACTIONS], pa[AZ_MAX_ACTIONS];
    int acts[AZ_MAX_ACTIONS], na = 0;
    for (int a = 0; a < A; ++a) {
      const double v = q[(size_t)i * AZ_MAX_ACTIONS + a];
      Q[(size_t)i * A + a] = v;
      if (v == v) { qa[na] = v; acts[na++] = a; }
    }
    if (pi) {
      for (int a = 0; a < A; ++a) pi[(size_t)i * A + a] = 0.0;
      if (na) minmax_policy(qa, na, cfg->tau, pa);
      for (int k = 0; k < na; ++k) pi[(size_t)i * A + acts[k]] = pa[k];
    }
  }
  return AZ_OK;
}

extern "C" int az_game_heuristic(az_engine* e, const uint64_t* keys, int32_t n, double* h) {
  ENGINE(e);
  AZCHK(check_minmax_game(e));
  if (n < 0 || (n > 0 && (!keys || !h))) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  for (int off = 0; off < n; off += e->io_cap) {
    const int m = std::min(e->io_cap, n - off);
    AZCHK(mm_reserve(e, (m + AZ_MAX_ACTIONS - 1) / AZ_MAX_ACTIONS));
    HIPCHK(hipMemcpyAsync(e->d_keys, keys + 2 * (size_t)off, sizeof(uint64_t) * 2 * m, hipMemcpyHostToDevice, e->stream));
    DISPATCH_GAME(e->cfg.game, hipLaunchKernelGGL((k_heuristic<Gm>), dim3((m + 255) / 256), dim3(256), 0, e->stream, (const unsigned long long*)e->d_keys, m, e->d_mm_q));
    HIPCHK(hipMemcpyAsync(h + off, e->d_mm_q, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  HIPCHK(hipGetLastError());
  return AZ_OK;
}
