// minmax.h -- MinMax.Player (src/minmax.jl:14-114) on the device: the exhaustive depth-limited walk behind az_minmax_qvalues and
// the arena's MinMax player.  The contract (recursion, heuristics, think, move selection) is in include/azhip.h "MinMax player".
//
// k_minmax<Gm>: one workgroup per (root, root action) -- a 128-game ply of Connect Four is 896 workgroups.  Inside a workgroup
//   1. the plies below the root action are expanded breadth-first into an LDS frontier (one record per node: state, parent, reward
//      of the edge, whether the turn changed on it) until a level holds at least MM_THREADS nodes, the depth is used up or the next
//      level might not fit; terminal nodes stay as finished entries (value 0.);
//   2. every lane walks the remaining plies below its frontier nodes depth-first, with the remaining depth as a TEMPLATE parameter:
//      the recursion is unrolled at compile time into nested loops over the action mask, all state in registers (no runtime-indexed
//      per-thread array, no stack);
//   3. the expanded plies are reduced back up, a level at a time, with an LDS atomic max per child.
// max and negation are exact and Julia's max orders -0.0 below 0.0, so a value travels as a 64-bit key whose unsigned order is that
// order (mm_key) and the result does not depend on the partition or on the order the atomics arrive in; the only rounding steps are
// the leaf heuristic and q = r + gamma * v (one multiplication, one addition: __dmul_rn / __dadd_rn on the device).
// The first three plies always fit the frontier (1 + 9 + 81 + 729 <= MM_CAP), so a lane walks at most AZ_MINMAX_MAX_DEPTH - 4 = 5.
#pragma once
#include "engine.h"

constexpr int MM_THREADS = 256;
constexpr int MM_CAP = 1024;        // nodes of a workgroup's frontier: 35 KB of LDS
constexpr int MM_LANE_DEPTH = 5;    // deepest walk below a frontier node
static_assert(AZ_MINMAX_MAX_DEPTH - 1 - 3 <= MM_LANE_DEPTH, "a lane's walk is instantiated up to MM_LANE_DEPTH plies");
static_assert(1 + AZ_MAX_ACTIONS + AZ_MAX_ACTIONS * AZ_MAX_ACTIONS * (1 + AZ_MAX_ACTIONS) <= MM_CAP, "three plies always fit the frontier");

// think()'s pi (minmax.jl:87-114) from the q-values of the n available actions; host only
inline void minmax_policy(const double* q, int n, double tau, double* pi) {
  const double inf = __builtin_inf();
  bool winning = false, notlosing = false;
  for (int i = 0; i < n; ++i) { winning = winning || q[i] == inf; notlosing = notlosing || q[i] > -inf; }
  if (winning) for (int i = 0; i < n; ++i) pi[i] = q[i] == inf ? 1.0 : 0.0;
  else if (!notlosing) for (int i = 0; i < n; ++i) pi[i] = 1.0;
  else {
    double qmax = q[0];
    for (int i = 1; i < n; ++i) if (q[i] > qmax) qmax = q[i];
    if (tau == 0.0) for (int i = 0; i < n; ++i) pi[i] = q[i] == qmax ? 1.0 : 0.0;
    else {
      double C = 0.0;
      for (int i = 0; i < n; ++i) if (q[i] > -inf && __builtin_fabs(q[i]) > C) C = __builtin_fabs(q[i]);
      C = C + 2.220446049250313e-16;                                  // eps(Float64)
      const double inv = 1.0 / tau;
      for (int i = 0; i < n; ++i) {
        const double x = q[i] == -inf ? 0.0 : az_exp((q[i] - qmax) / C);
        pi[i] = az_pow(x, inv);
      }
    }
  }
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + pi[i];
  for (int i = 0; i < n; ++i) pi[i] = pi[i] / s;
}

#if defined(__HIPCC__)
// order-preserving map of the non-NaN doubles onto unsigned integers (-0.0 below 0.0, as Julia's max has it); 0 is no value's key
__device__ __forceinline__ unsigned long long mm_key(double d) {
  const unsigned long long u = az_d2u(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double mm_unkey(unsigned long long k) {
  return az_u2d((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k);
}
// r of qvalue (minmax.jl:32-36): the white reward after the move, seen from the mover (`wp`), amplified on request
template <class Gm>
__device__ __forceinline__ double mm_reward(const GEnv& next, bool wp, bool amplify) {
  const double wr = (double)Gm::white_reward(next);
  double r = wp ? wr : -wr;
  if (amplify && r != 0.0) r = r > 0.0 ? __builtin_inf() : -__builtin_inf();
  return r;
}
// q = r + gamma * (turn changed ? -v : v), minmax.jl:38-41
__device__ __forceinline__ double mm_q(double r, double gamma, double v, bool turn_changed) {
  return __dadd_rn(r, __dmul_rn(gamma, turn_changed ? -v : v));
}

// value(player, game, D) (minmax.jl:17-26)
template <class Gm, int D>
__device__ __forceinline__ double mm_value(const GEnv& g, bool amplify, double gamma) {
  if (g.fin & 1) return 0.0;
  if constexpr (D == 0) return Gm::heuristic(g);
  else {
    const bool wp = Gm::white_playing(g);
    uint32_t m = Gm::mask(g);
    unsigned long long best = 0;
    while (m) {
      const int a = __builtin_ctz(m);
      m &= m - 1;
      GEnv nx = g;
      Gm::play(nx, a);
      const double r = mm_reward<Gm>(nx, wp, amplify);
      const double v = mm_value<Gm, D - 1>(nx, amplify, gamma);
      const unsigned long long k = mm_key(mm_q(r, gamma, v, wp != Gm::white_playing(nx)));
      best = k > best ? k : best;
    }
    return best ? mm_unkey(best) : 0.0;
  }
}

template <class Gm>
__global__ __launch_bounds__(MM_THREADS) void k_minmax(const GEnv* __restrict__ roots, int n, int depth, int amplify_i, double gamma,
                                                       double* __restrict__ Q /* [n][AZ_MAX_ACTIONS] */) {
  __shared__ unsigned long long s_a[MM_CAP], s_b[MM_CAP];   // the node's state
  __shared__ unsigned long long s_val[MM_CAP];              // mm_key of its value; 0 = none of its children has reported yet
  __shared__ double s_r[MM_CAP];                            // r of the edge from its parent
  __shared__ unsigned short s_parent[MM_CAP];
  __shared__ unsigned char s_meta[MM_CAP];                  // bits 0..2 GEnv::fin, bit 3 the turn changed on the edge from its parent
  __shared__ int s_first[AZ_MINMAX_MAX_DEPTH + 2];          // first node of every level
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const int root = (int)(blockIdx.x / (unsigned)Gm::A), act = (int)(blockIdx.x % (unsigned)Gm::A);
  if (root >= n) return;
  const bool amplify = amplify_i != 0;
  const GEnv g0 = roots[root];
  double* out = Q + (size_t)root * AZ_MAX_ACTIONS + act;
  if (!((Gm::mask(g0) >> act) & 1) || (g0.fin & 1)) {       // uniform over the workgroup
    if (tid == 0) *out = __builtin_nan("");
    return;
  }
  if (tid == 0) {
    GEnv nx = g0;
    Gm::play(nx, act);
    const bool wp = Gm::white_playing(g0);
    s_a[0] = nx.a; s_b[0] = nx.b; s_r[0] = mm_reward<Gm>(nx, wp, amplify);
    s_meta[0] = (unsigned char)((nx.fin & 7) | (wp != Gm::white_playing(nx) ? 8 : 0));
    s_parent[0] = 0;
    s_val[0] = (nx.fin & 1) ? mm_key(0.0) : 0ULL;
    s_first[0] = 0;
    s_count = 1;
  }
  __syncthreads();
  // 1. breadth first
  int L = 0, rem = depth - 1, first = 0, end = 1;
  while (rem > 0 && end > first && end - first < MM_THREADS && end + (end - first) * Gm::A <= MM_CAP) {
    for (int i = first + tid; i < end; i += MM_THREADS) {
      if (s_meta[i] & 1) continue;
      const GEnv g{s_a[i], s_b[i], (uint32_t)(s_meta[i] & 7)};
      const bool wp = Gm::white_playing(g);
      uint32_t m = Gm::mask(g);
      while (m) {
        const int a = __builtin_ctz(m);
        m &= m - 1;
        GEnv nx = g;
        Gm::play(nx, a);
        const int j = atomicAdd(&s_count, 1);               // < MM_CAP: the loop condition left room for (end - first) * A children
        s_a[j] = nx.a; s_b[j] = nx.b; s_r[j] = mm_reward<Gm>(nx, wp, amplify);
        s_meta[j] = (unsigned char)((nx.fin & 7) | (wp != Gm::white_playing(nx) ? 8 : 0));
        s_parent[j] = (unsigned short)i;
        s_val[j] = (nx.fin & 1) ? mm_key(0.0) : 0ULL;
      }
    }
    __syncthreads();
    first = end;
    end = s_count;
    ++L; --rem;
    if (tid == 0) s_first[L] = first;
    __syncthreads();                                        // s_count is read by everyone before the next level adds to it
  }
  // 2. every lane walks the rest below its nodes of the last level
  for (int i = first + tid; i < end; i += MM_THREADS) {
    const GEnv g{s_a[i], s_b[i], (uint32_t)(s_meta[i] & 7)};
    double v;
    switch (rem) {
      case 0: v = mm_value<Gm, 0>(g, amplify, gamma); break;
      case 1: v = mm_value<Gm, 1>(g, amplify, gamma); break;
      case 2: v = mm_value<Gm, 2>(g, amplify, gamma); break;
      case 3: v = mm_value<Gm, 3>(g, amplify, gamma); break;
      case 4: v = mm_value<Gm, 4>(g, amplify, gamma); break;
      case 5: v = mm_value<Gm, 5>(g, amplify, gamma); break;
      default: v = __builtin_nan(""); break;                // unreachable: see the static_asserts above
    }
    s_val[i] = mm_key(v);
  }
  __syncthreads();
  // 3. back up: maximum(qs) per parent, a level at a time
  for (int l = L; l >= 1; --l) {
    const int lo = s_first[l], hi = l == L ? end : s_first[l + 1];
    for (int i = lo + tid; i < hi; i += MM_THREADS) {
      const unsigned long long k = s_val[i];
      const double v = k ? mm_unkey(k) : 0.0;               // (a state that is not terminal has a child: k != 0)
      atomicMax(&s_val[s_parent[i]], mm_key(mm_q(s_r[i], gamma, v, (s_meta[i] & 8) != 0)));
    }
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long k = s_val[0];
    *out = mm_q(s_r[0], gamma, k ? mm_unkey(k) : 0.0, (s_meta[0] & 8) != 0);
  }
}

// GI.heuristic_value of n states
template <class Gm>
__global__ void k_heuristic(const unsigned long long* __restrict__ keys, int n, double* __restrict__ h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  h[i] = Gm::heuristic(Gm::from_key(keys[2 * i], keys[2 * i + 1]));
}
#endif
