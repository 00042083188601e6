// solver.hip -- host side of the Connect Four solver (Solver.Player, games/connect-four/solver.jl): the entry points az_solver_cfg_init /
// az_c4_solve / az_solver_policy and the transposition table az_solver_table_* / az_c4_solve_table of include/azhip.h.  Kernels: solver.h.
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

// az_solver_table: 2^log2 entries of 8 bytes in the HBM of one device (sv_entry, solver_search.h).  It belongs to its caller and
// knows no engine: every az_c4_solve_table call of that device may be given it.
struct az_solver_table {
  int device = 0, log2 = 0;
  unsigned long long* d_words = nullptr;
  unsigned long long* d_count = nullptr;                             // az_solver_table_info's counter
};
#define TABLE(t) if (!(t)) return fail(AZ_ERR_BAD_ARG, "solver table is NULL"); HIPCHK(hipSetDevice((t)->device))

extern "C" int az_solver_table_create(int32_t device, int32_t log2_entries, az_solver_table** out) {
  if (!out) return fail(AZ_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (log2_entries < 0 || log2_entries > 30) return fail(AZ_ERR_BAD_ARG, "solver table log2_entries = %d outside 0..30", (int)log2_entries);
  AZCHK(use_device(device));
  az_solver_table* t = new (std::nothrow) az_solver_table();
  if (!t) return fail(AZ_ERR_HIP, "out of host memory");
  t->device = device; t->log2 = log2_entries;
  const size_t bytes = sizeof(unsigned long long) << log2_entries;
  hipError_t err = hipMalloc((void**)&t->d_words, bytes);
  if (err == hipSuccess) err = hipMalloc((void**)&t->d_count, sizeof(unsigned long long));
  if (err == hipSuccess) err = hipMemset(t->d_words, 0, bytes);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    if (t->d_words) (void)hipFree(t->d_words);
    if (t->d_count) (void)hipFree(t->d_count);
    delete t;
    return fail(AZ_ERR_HIP, "a solver table of 2^%d entries (%zu bytes) on device %d: %s", (int)log2_entries, bytes, (int)device, hipGetErrorString(err));
  }
  *out = t;
  return AZ_OK;
}

extern "C" int az_solver_table_destroy(az_solver_table* t) {
  if (!t) return AZ_OK;
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();                                      // no call that was given the table is still running
  if (t->d_words) (void)hipFree(t->d_words);
  if (t->d_count) (void)hipFree(t->d_count);
  delete t;
  return AZ_OK;
}

extern "C" int az_solver_table_clear(az_solver_table* t) {
  TABLE(t);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(t->d_words, 0, sizeof(unsigned long long) << t->log2));
  HIPCHK(hipDeviceSynchronize());
  return AZ_OK;
}

extern "C" int az_solver_table_info(az_solver_table* t, int32_t* log2_entries, int64_t* bytes, int64_t* occupied) {
  TABLE(t);
  if (log2_entries) *log2_entries = t->log2;
  if (bytes) *bytes = (int64_t)sizeof(unsigned long long) << t->log2;
  if (occupied) {                                                    // counted now, on the device
    const long long entries = 1LL << t->log2;
    unsigned long long cnt = 0;
    HIPCHK(hipMemset(t->d_count, 0, sizeof cnt));
    hipLaunchKernelGGL(k_sv_table_count, dim3((unsigned)std::min<long long>((entries + 255) / 256, 4096)), dim3(256), 0, 0,
                       (const unsigned long long*)t->d_words, entries, t->d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&cnt, t->d_count, sizeof cnt, hipMemcpyDeviceToHost));
    *occupied = (int64_t)cnt;
  }
  return AZ_OK;
}

// az_c4_solve (t == NULL, with_table false) and az_c4_solve_table
static int c4_solve(az_engine* e, const az_solver_cfg* cfg, bool with_table, az_solver_table* t, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q, int64_t* nodes) {
  AZCHK(check_solver_cfg(cfg));
  ENGINE(e);
  if (e->cfg.game != AZ_GAME_CONNECT_FOUR) {
    static const char* const names[] = {"Connect Four", "Tic-tac-toe", "Mancala", "the 9x9x4 plane geometry"};
    const int gid = (int)e->cfg.game;
    return fail(AZ_ERR_BAD_ARG, "the solver solves Connect Four; this engine plays %s (game %d)", gid >= 0 && gid < 4 ? names[gid] : "another game", gid);
  }
  if (with_table) {
    if (!t) return fail(AZ_ERR_BAD_ARG, "solver table is NULL");
    if (t->device != e->device) return fail(AZ_ERR_BAD_ARG, "the solver table lives on device %d, the engine on device %d", t->device, e->device);
  }
  if (n < 0) return fail(AZ_ERR_BAD_ARG, "n = %d states", (int)n);
  if (n == 0) return AZ_OK;
  if (!keys || !value || !q) return fail(AZ_ERR_BAD_ARG, "NULL buffer");
  static_assert(ConnectFour::A == 7, "seven queries per state");
  const size_t nq = (size_t)n * 7;
  AZCHK(sv_reserve(e, n));
  HIPCHK(hipMemcpyAsync(e->d_sv_keys, keys, sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyHostToDevice, e->stream));
  signed char* d_bounded = (signed char*)e->d_sv_q + (size_t)e->sv_cap * 7;
  const dim3 grid((unsigned)((n + SV_STATES - 1) / SV_STATES));
  if (with_table)
    hipLaunchKernelGGL(k_c4_solve_table, grid, dim3(SV_LANES), 0, e->stream, t->d_words, t->log2,
                       (const unsigned long long*)e->d_sv_keys, (int)n, (int)(cfg->weak != 0), (long long)cfg->node_budget, (signed char*)e->d_sv_q, d_bounded, e->d_sv_nodes);
  else
    hipLaunchKernelGGL(k_c4_solve, grid, dim3(SV_LANES), 0, e->stream,
                       (const unsigned long long*)e->d_sv_keys, (int)n, (int)(cfg->weak != 0), (long long)cfg->node_budget, (signed char*)e->d_sv_q, d_bounded, e->d_sv_nodes);
  HIPCHK(hipGetLastError());
  std::vector<long long> qn(nodes ? nq : 0);
  std::vector<int8_t> bounded(nq);
  HIPCHK(hipMemcpyAsync(q, e->d_sv_q, nq, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(bounded.data(), d_bounded, nq, hipMemcpyDeviceToHost, e->stream));
  if (nodes) HIPCHK(hipMemcpyAsync(qn.data(), e->d_sv_nodes, sizeof(long long) * nq, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; ++i) {
    value[i] = (int8_t)sv_state_value(keys[2 * (size_t)i], keys[2 * (size_t)i + 1], q + (size_t)i * 7, bounded.data() + (size_t)i * 7);
    if (nodes) {
      long long s = 0;
      for (int a = 0; a < 7; ++a) s += qn[(size_t)i * 7 + a];
      nodes[i] = s;
    }
  }
  return AZ_OK;
}

extern "C" int az_c4_solve(az_engine* e, const az_solver_cfg* cfg, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q, int64_t* nodes) {
  return c4_solve(e, cfg, false, nullptr, keys, n, value, q, nodes);
}

extern "C" int az_c4_solve_table(az_engine* e, const az_solver_cfg* cfg, az_solver_table* t, const uint64_t* keys, int32_t n, int8_t* value, int8_t* q, int64_t* nodes) {
  return c4_solve(e, cfg, true, t, keys, n, value, q, nodes);
}
