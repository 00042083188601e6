// solver.h -- Solver.Player's scores (games/connect-four/solver.jl:58-89) on the device: the exact alpha-beta search to the end of the
// game behind az_c4_solve and az_c4_solve_table.  The contract (score convention, terminal children, budget, determinism, the table)
// is in include/azhip.h "Connect Four solver"; the search itself, which the host can run too, is in solver_search.h.
//
// k_c4_solve / k_c4_solve_table: ONE LANE PER QUERY, a query being (state, action).  A workgroup is one wavefront and holds 9 states:
// lanes 7g .. 7g + 6 are the 7 actions of its g-th state, lane 63 idles.  A lane searches the position AFTER its action
// (solver_search.h):
//   * the recursion is an explicit stack of one 32-bit word per ply and lane in LDS ([ply][lane], so the 64 lanes of a step hit 64
//     different banks) -- a private array indexed by the ply would live in scratch memory;
//   * a lane that has finished waits for the longest search of its wavefront, which is what the node budget bounds.
// Second pass, same kernel: the 7 lanes of a state exchange their results; a lane whose query ran over the budget then asks the much
// cheaper question "is this move better than the best solved one?" (sv_bounded) with a fresh budget.  If none is, the
// state's value is known although that q is not (bad moves next to a quick win are the expensive queries and the irrelevant ones).
// k_c4_solve has no transposition table: what it returns for a state depends on (state, weak, node_budget) and on nothing else.
// k_c4_solve_table is the same kernel over sv_search<true>: every lane of every wavefront, and every call that is given the same
// az_solver_table, reads and writes one table in HBM, an entry with one relaxed agent-scope 64-bit load or store (global_load /
// global_store_dwordx2 sc1: past the CU's L1, so an entry another CU wrote is seen; whole, so an entry is never torn).  No ordering is
// asked for and none is needed: an entry says something about the one position whose whole key it carries and is true whenever it is read.
#pragma once
#include "engine.h"
#include "solver_search.h"

constexpr int SV_LANES = 64;              // one wavefront per workgroup
constexpr int SV_STATES = 9;              // states of a workgroup: 63 lanes

#if defined(__HIPCC__)
struct SvLdsStack {
  uint32_t* base;                                                    // &s_stack[0][lane]
  __device__ __forceinline__ uint32_t& operator()(int ply) const { return base[ply * SV_LANES]; }
};
struct SvDevTable {
  unsigned long long* words;                                         // 2^log2 of them, in HBM
  int log2;
  __device__ __forceinline__ int bits() const { return log2; }
  __device__ __forceinline__ uint64_t load(uint64_t slot) const { return __hip_atomic_load(words + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(uint64_t slot, uint64_t w) const { __hip_atomic_store(words + slot, (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// q [n][7] (SV_NA: full column or terminal state; SV_UNSOLVED: over budget), bounded [n][7] (1: q is unsolved but proven to be no
// more than the state's best solved q), nodes [n][7]
template <bool TT, class Table>
__device__ __forceinline__ void sv_kernel(uint32_t (*s_stack)[SV_LANES], Table table, const unsigned long long* __restrict__ keys, int n, int weak,
                                          long long budget, signed char* __restrict__ q, signed char* __restrict__ bounded,
                                          long long* __restrict__ nodes_out) {
  const int lane = threadIdx.x, grp = lane / 7, act = lane % 7;
  const long long state = (long long)blockIdx.x * SV_STATES + grp;
  const bool active = grp < SV_STATES && state < n;
  const SvLdsStack stack{&s_stack[0][lane]};
  uint64_t cur = 0, all = 0;
  int stones = 0, result = SV_NA;
  long long nodes = 0;
  if (active && !sv_child(keys[2 * state], keys[2 * state + 1], act, weak, &cur, &all, &stones, &result))
    result = sv_solve<TT>(cur, all, stones, weak, budget, stack, table, &nodes);
  // every lane of the wavefront is here again: the best solved q of the lane's state
  int best = SV_NA;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int r = __shfl(result, (grp * 7 + j) & (SV_LANES - 1));
    if (r != SV_UNSOLVED && r > best) best = r;
  }
  bool bound = false;
  if (active && result == SV_UNSOLVED && best != SV_NA) bound = sv_bounded<TT>(cur, all, stones, weak, best, budget, stack, table, &nodes);
  if (active) {
    q[state * 7 + act] = (signed char)result;
    bounded[state * 7 + act] = (signed char)bound;
    nodes_out[state * 7 + act] = nodes;
  }
}

__global__ __launch_bounds__(SV_LANES) void k_c4_solve(const unsigned long long* __restrict__ keys, int n, int weak, long long budget,
                                                       signed char* __restrict__ q, signed char* __restrict__ bounded,
                                                       long long* __restrict__ nodes_out) {
  __shared__ uint32_t s_stack[SV_PLIES][SV_LANES];
  sv_kernel<false>(s_stack, SvNoTable{}, keys, n, weak, budget, q, bounded, nodes_out);
}
__global__ __launch_bounds__(SV_LANES) void k_c4_solve_table(unsigned long long* table, int log2_entries, const unsigned long long* __restrict__ keys,
                                                             int n, int weak, long long budget, signed char* __restrict__ q,
                                                             signed char* __restrict__ bounded, long long* __restrict__ nodes_out) {
  __shared__ uint32_t s_stack[SV_PLIES][SV_LANES];
  sv_kernel<true>(s_stack, SvDevTable{table, log2_entries}, keys, n, weak, budget, q, bounded, nodes_out);
}
// *count += the entries of words[0 .. entries) that are not empty
__global__ __launch_bounds__(256) void k_sv_table_count(const unsigned long long* __restrict__ words, long long entries, unsigned long long* count) {
  long long mine = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < entries; i += (long long)gridDim.x * blockDim.x) mine += words[i] != 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
}
#endif
