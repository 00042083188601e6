// solver.hip -- host side of the Connect Four solver (Solver.Player, games/connect-four/solver.jl): the entry points az_solver_cfg_init /
// az_c4_solve / az_solver_policy of include/azhip.h.  Kernel: solver.h.
#include "solver.h"

static int check_solver_cfg(const az_solver_cfg* c) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "az_solver_cfg is NULL");
  if (c->struct_size != (int32_t)sizeof(az_solver_cfg)) return fail(AZ_ERR_BAD_ARG, "az_solver_cfg.struct_size = %d, expected %d (call az_solver_cfg_init)", (int)c->struct_size, (int)sizeof(az_solver_cfg));
  if (c->node_budget <= 0) return fail(AZ_ERR_BAD_ARG, "solver node_budget %lld must be > 0", (long long)c->node_budget);
  return AZ_OK;
}

extern "C" int az_solver_cfg_init(az_solver_cfg* cfg) {
  if (!cfg) return fail(AZ_ERR_BAD_ARG, "az_solver_cfg is NULL");
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (int32_t)sizeof(az_solver_cfg);
  cfg->weak = 0;
  cfg->node_budget = AZ_SOLVER_DEFAULT_BUDGET;
  return AZ_OK;
}

extern "C" int az_solver_policy(const int8_t* q, int32_t n_actions, double* pi) {
  if (!q || !pi) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  if (n_actions < 1 || n_actions > AZ_MAX_ACTIONS) return fail(AZ_ERR_BAD_ARG, "n_actions = %d outside 1..%d", (int)n_actions, AZ_MAX_ACTIONS);
  int best = AZ_SOLVER_NA, cnt = 0;
  for (int a = 0; a < n_actions; ++a) {
    if (q[a] == AZ_SOLVER_UNSOLVED) return fail(AZ_ERR_BAD_ARG, "q[%d] is AZ_SOLVER_UNSOLVED: think needs the score of every available action", a);
    if (q[a] != AZ_SOLVER_NA && q[a] > best) best = q[a];
  }
  for (int a = 0; a < n_actions; ++a) cnt += q[a] != AZ_SOLVER_NA && q[a] == best;
  for (int a = 0; a < n_actions; ++a) pi[a] = (q[a] != AZ_SOLVER_NA && q[a] == best) ? 1.0 / (double)cnt : 0.0;   // solver.jl:94-97
  return AZ_OK;
}

// room for n states, their 7 q-values, "bounded" flags and node counts
static int sv_reserve(az_engine* e, int n) {
  if (n <= e->sv_cap) return AZ_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  for (void* old : {(void*)e->d_sv_keys, (void*)e->d_sv_q, (void*)e->d_sv_nodes}) if (old) {   // d_sv_q: [cap][7] q, then [cap][7] flags
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), old), e->allocs.end());
    (void)hipFree(old);
  }
  e->alloc_bytes -= (size_t)e->sv_cap * (2 * sizeof(uint64_t) + 7 * (2 * sizeof(int8_t) + sizeof(long long)));
  e->d_sv_keys = nullptr; e->d_sv_q = nullptr; e->d_sv_nodes = nullptr; e->sv_cap = 0;
  const int cap = std::max(n, 1024);
  AZCHK(dalloc(e, &e->d_sv_keys, (size_t)cap * 2, false));
  AZCHK(dalloc(e, &e->d_sv_q, (size_t)cap * 14, false));
  AZCHK(dalloc(e, &e->d_sv_nodes, (size_t)cap * 7, false));
  e->sv_cap = cap;
  return AZ_OK;
}

extern "C" int az_c4_solve(az_engine* e, const az_solver_cfg* cfg, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q, int64_t* nodes) {
  AZCHK(check_solver_cfg(cfg));
  ENGINE(e);
  if (e->cfg.game != AZ_GAME_CONNECT_FOUR) {
    static const char* const names[] = {"Connect Four", "Tic-tac-toe", "Mancala", "the 9x9x4 plane geometry"};
    const int gid = (int)e->cfg.game;
    return fail(AZ_ERR_BAD_ARG, "the solver solves Connect Four; this engine plays %s (game %d)", gid >= 0 && gid < 4 ? names[gid] : "another game", gid);
  }
  if (n < 0) return fail(AZ_ERR_BAD_ARG, "n = %d states", (int)n);
  if (n == 0) return AZ_OK;
  if (!keys || !value || !q) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  static_assert(ConnectFour::A == 7, "seven queries per state");
  const size_t nq = (size_t)n * 7;
  AZCHK(sv_reserve(e, n));
  HIPCHK(hipMemcpyAsync(e->d_sv_keys, keys, sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyHostToDevice, e->stream));
  signed char* d_bounded = (signed char*)e->d_sv_q + (size_t)e->sv_cap * 7;
  hipLaunchKernelGGL(k_c4_solve, dim3((unsigned)((n + SV_STATES - 1) / SV_STATES)), dim3(SV_LANES), 0, e->stream,
                     (const unsigned long long*)e->d_sv_keys, (int)n, (int)(cfg->weak != 0), (long long)cfg->node_budget, (signed char*)e->d_sv_q, d_bounded, e->d_sv_nodes);
  HIPCHK(hipGetLastError());
  std::vector<long long> qn(nodes ? nq : 0);
  std::vector<int8_t> bounded(nq);
  HIPCHK(hipMemcpyAsync(q, e->d_sv_q, nq, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(bounded.data(), d_bounded, nq, hipMemcpyDeviceToHost, e->stream));
  if (nodes) HIPCHK(hipMemcpyAsync(qn.data(), e->d_sv_nodes, sizeof(long long) * nq, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; ++i) {
    const int8_t* qi = q + (size_t)i * 7;
    const GEnv g = ConnectFour::from_key(keys[2 * (size_t)i], keys[2 * (size_t)i + 1]);
    if (g.fin & 1) {                                                 // Solver.value's terminal branch (solver.jl:69-77): the side to move has lost, or a draw
      const int stones = az_popc64((g.a | g.b) & ~AZ_BLACK_BIT);
      value[i] = (g.fin >> 1) ? (int8_t)-(22 - (stones + 1) / 2) : (int8_t)0;
    } else {
      int best = AZ_SOLVER_NA;
      bool open = false;                                             // an unsolved q that is not known to be <= the best solved one
      for (int a = 0; a < 7; ++a) {
        if (qi[a] == AZ_SOLVER_UNSOLVED) open = open || !bounded[(size_t)i * 7 + a];
        else if (qi[a] != AZ_SOLVER_NA && qi[a] > best) best = qi[a];
      }
      value[i] = (open || best == AZ_SOLVER_NA) ? (int8_t)AZ_SOLVER_UNSOLVED : (int8_t)best;
    }
    if (nodes) {
      long long s = 0;
      for (int a = 0; a < 7; ++a) s += qn[(size_t)i * 7 + a];
      nodes[i] = s;
    }
  }
  return AZ_OK;
}
