// solver.h -- Solver.Player's scores (games/connect-four/solver.jl:58-89) on the device: the exact alpha-beta search to the end of the
// game behind az_c4_solve.  The contract (score convention, terminal children, budget, determinism) is in include/azhip.h "Connect
// Four solver".
//
// k_c4_solve: ONE LANE PER QUERY, a query being (state, action).  A workgroup is one wavefront and holds 9 states: lanes 7g .. 7g + 6
// are the 7 actions of its g-th state, lane 63 idles.  A lane searches the position AFTER its action with a negamax over bitboards
// (games.h's 7 bits per column):
//   * `cur` = the stones of the player to move, `all` = every stone; a move is cur ^= all, all |= bit; it is undone by the same two
//     steps backwards, so a ply keeps no board;
//   * a node is only entered when its mover has no winning move (the parent has looked), so what a node does first is to list the moves
//     that do not lose at once: the opponent's winning cells (sv_winning, the shifts of the four axes) that can be played now are
//     forced, two of them lose, and no move may be played right below one.  No such move = the opponent wins with his next stone;
//   * the window is cut to what the remaining cells allow, the moves are tried centre first (SV_ORDER, the order of the test suite's
//     CPU negamax);
//   * the value is closed in on by null-window passes from the root (sv_search), the windows far from 0 first: those are shallow
//     searches, and weak mode stops as soon as the sign is known;
//   * the recursion is an explicit stack of one 32-bit word per ply and lane in LDS (alpha, beta, the columns still to try, the column
//     being tried: [ply][lane], so the 64 lanes of a step hit 64 different banks) -- a private array indexed by the ply would live in
//     scratch memory;
//   * every trip of the loop is one step of the same shape for every lane -- take the child's score, pick the next column, play it,
//     enter the child -- so lanes at different depths of different trees still share the instruction stream; a lane that has finished
//     waits for the longest search of its wavefront, which is what the node budget bounds.
// Second pass, same kernel: the 7 lanes of a state exchange their results; a lane whose query ran over the budget then asks the much
// cheaper question "is this move better than the best solved one?" (sv_bounded) with a fresh budget.  If none is, the
// state's value is known although that q is not (bad moves next to a quick win are the expensive queries and the irrelevant ones).
// There is no transposition table: what is returned for a state depends on (state, weak, node_budget) and on nothing else.
#pragma once
#include "engine.h"

constexpr int SV_LANES = 64;              // one wavefront per workgroup
constexpr int SV_STATES = 9;              // states of a workgroup: 63 lanes
constexpr int SV_PLIES = 42;              // frames of a lane: the search starts with at least one stone on the board and a node with 40 or more stones returns at once
constexpr int SV_NA = AZ_SOLVER_NA, SV_UNSOLVED = AZ_SOLVER_UNSOLVED;
constexpr uint64_t SV_BOTTOM = (1ULL << 0) | (1ULL << 7) | (1ULL << 14) | (1ULL << 21) | (1ULL << 28) | (1ULL << 35) | (1ULL << 42);
constexpr uint64_t SV_BOARD = SV_BOTTOM * 0x3fULL;
constexpr uint32_t SV_ORDER = 0x6051423u; // nibble k = the k-th column tried: 3, 2, 4, 1, 5, 0, 6

// the empty cells where a stone of `p` would complete four in a row (whether they can be played yet or not)
AZ_GHD uint64_t sv_winning(uint64_t p, uint64_t all) {
  uint64_t r = (p << 1) & (p << 2) & (p << 3);                       // below a vertical three
#pragma unroll
  for (int s = 6; s <= 8; ++s) {                                     // the two diagonals and the rows: steps of 6, 7 and 8 bits
    uint64_t t = (p << s) & (p << 2 * s);
    r |= t & (p << 3 * s);
    r |= t & (p >> s);
    t = (p >> s) & (p >> 2 * s);
    r |= t & (p << s);
    r |= t & (p >> 3 * s);
  }
  return r & (SV_BOARD ^ all);
}
AZ_GHD uint64_t sv_possible(uint64_t all) { return (all + SV_BOTTOM) & SV_BOARD; }   // the lowest empty cell of every column that has one
// the playable cells that do not hand the opponent a win with his next stone; the mover himself has no winning cell to play
AZ_GHD uint64_t sv_nonlosing(uint64_t cur, uint64_t all) {
  uint64_t possible = sv_possible(all);
  const uint64_t opp = sv_winning(cur ^ all, all);
  const uint64_t forced = possible & opp;
  if (forced) {
    if (forced & (forced - 1)) return 0;                             // two threats: one of them stays open
    possible = forced;
  }
  return possible & ~(opp >> 1);
}
// bit k: the k-th column of SV_ORDER has a cell in `cells`
AZ_GHD uint32_t sv_columns(uint64_t cells) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) m |= (uint32_t)(((cells >> (7 * ((SV_ORDER >> (4 * k)) & 7u))) & 0x7f) != 0) << k;
  return m;
}
// frame word: bits 0..7 alpha, 8..15 beta (both + 64), 16..22 columns still to try (sv_columns order), 24..26 the column being tried
AZ_GHD uint32_t sv_frame(int alpha, int beta, uint32_t cols, int col) {
  return (uint32_t)(alpha + 64) | ((uint32_t)(beta + 64) << 8) | (cols << 16) | ((uint32_t)col << 24);
}
AZ_GHD int sv_out(int score, int weak) { return weak ? (score > 0) - (score < 0) : score; }   // weak mode answers with the sign
// the next null window (med, med + 1) inside [mn, mx]: the middle, moved towards 0 where the interval allows
AZ_GHD int sv_med(int mn, int mx) {
  int med = mn + (mx - mn) / 2;
  if (med <= 0 && mn / 2 < med) med = mn / 2;
  else if (med >= 0 && mx / 2 > med) med = mx / 2;
  return med;
}

// The query of action `act` in the state (a, b): true = decided without search, *q is its q-value or SV_NA (full column, terminal
// state); false = (*cur, *all, *stones) is the position after the action, whose mover has no winning move.
AZ_GHD bool sv_child(uint64_t a, uint64_t b, int act, int weak, uint64_t* cur_out, uint64_t* all_out, int* stones_out, int* q) {
  const GEnv g0 = ConnectFour::from_key(a, b);
  const uint64_t w = g0.a & ~AZ_BLACK_BIT;
  uint64_t all = w | g0.b;
  uint64_t cur = ConnectFour::white_playing(g0) ? w : g0.b;
  int stones = az_popc64(all);
  const uint64_t move0 = sv_possible(all) & (0x7fULL << (7 * act));
  *cur_out = 0; *all_out = 0; *stones_out = 0;
  if ((g0.fin & 1) || !move0) { *q = SV_NA; return true; }
  if (ConnectFour::has4(cur | move0)) { *q = sv_out(21 - stones / 2, weak); return true; }   // Solver.value's terminal branch: remaining_stones(winner) + 1
  if (stones == 41) { *q = 0; return true; }                         // the last cell, no alignment: a full board
  cur ^= all; all |= move0; ++stones;                                // the child: its mover is the opponent
  if (sv_winning(cur, all) & sv_possible(all)) { *q = sv_out(-((43 - stones) / 2), weak); return true; }   // he wins with his next stone
  *cur_out = cur; *all_out = all; *stones_out = stones;
  return false;
}

// The value of the position (cur, all, stones), known to lie in [mn, mx] and whose mover has no winning move, seen from its mover:
// null-window passes (med, med + 1) from the root, each moving one end of the interval to the result of the pass, until the interval is
// a point, or lies at or above stop_hi, or at or below stop_lo (a caller that only asks on which side of a score the value lies).
// A window away from 0 is cheap -- no position deeper than the stone that score speaks of is entered -- and the passes come to 0 from
// outside (sv_med), so the full-depth windows around 0 are searched last, or never.  [*lo, *hi] = the interval reached (given
// mx = mn + 1 there is one pass, and an end may move past the other: the value lies beyond the window on that side).  false = the
// passes would have entered more than `budget` nodes: nothing is known.  *nodes_io grows by the nodes entered (by `budget` then).
// `stack(ply)` is the lane's frame word of that ply (LDS on the device; a plain array where the host runs the same code).
template <class Stack>
AZ_GHD bool sv_search(uint64_t cur, uint64_t all, int stones, int mn, int mx, int stop_lo, int stop_hi, long long budget, Stack stack,
                       long long* nodes_io, int* lo_out, int* hi_out) {
  long long nodes = 0;
  int med = sv_med(mn, mx);
  int sp = 0, ret = 0, alpha = med, beta = med + 1;                  // ret: the score of the node just left (seen from its mover); sp: the ply of the open frame
  bool returning = false, over = false, entering = true;            // the root is entered first
  uint32_t cols = 0;
  while (true) {
    if (entering) {                                                  // the node at ply sp with (alpha, beta): a leaf sets ret, else its frame is opened
      entering = false;
      returning = true;
      if (++nodes > budget) { over = true; break; }
      const uint64_t next = sv_nonlosing(cur, all);
      const int lo = -((40 - stones) / 2), hi = (41 - stones) / 2;   // not lost before the stone after next / not won before the next but one
      if (!next) ret = -((42 - stones) / 2);                         // every move loses to the opponent's next stone
      else if (stones >= 40) ret = 0;                                // two cells left and nobody can win: a draw
      else {
        if (alpha < lo) alpha = lo;
        if (beta > hi) beta = hi;
        if (alpha >= beta) ret = alpha == lo ? alpha : beta;         // the window closed from below (alpha raised to beta or above) or from above
        else { cols = sv_columns(next); returning = false; }
      }
    }
    if (returning) {                                                 // the node at ply sp is finished with score ret
      if (sp == 0) {                                                 // a pass is over: ret bounds the value from the side it fell on
        if (ret <= med) mx = ret; else mn = ret;
        if (mn >= mx || mn >= stop_hi || mx <= stop_lo) break;
        med = sv_med(mn, mx); alpha = med; beta = med + 1;
        entering = true;
        continue;
      }
      --sp;
      const uint32_t f = stack(sp);
      const int col = (int)(f >> 24) & 7;
      const uint64_t top = ((all + (1ULL << (7 * col))) >> 1) & (0x3fULL << (7 * col));   // the stone the move put there
      all ^= top; cur ^= all; --stones;
      alpha = (int)(f & 0xff) - 64; beta = (int)((f >> 8) & 0xff) - 64; cols = (f >> 16) & 0x7f;
      const int s = -ret;
      if (s >= beta) { ret = s; continue; }                          // cut: this node is finished too
      if (s > alpha) alpha = s;
      returning = false;
    }
    if (!cols) { ret = alpha; returning = true; continue; }          // every move tried
    const int col = (int)(SV_ORDER >> (4 * __builtin_ctz(cols))) & 7;
    cols &= cols - 1;
    if (sp >= SV_PLIES) { over = true; break; }                      // cannot happen (see SV_PLIES); never write past the stack
    stack(sp) = sv_frame(alpha, beta, cols, col);
    const uint64_t bit = sv_possible(all) & (0x7fULL << (7 * col));
    cur ^= all; all |= bit; ++stones; ++sp;
    const int na = -beta; beta = -alpha; alpha = na;
    entering = true;
  }
  *nodes_io += over ? budget : nodes;
  *lo_out = mn; *hi_out = mx;
  return !over;
}

// first pass of a query whose child (cur, all, stones) needs a search: its q-value or SV_UNSOLVED.  Weak mode stops as soon as the
// sign is known.
template <class Stack>
AZ_GHD int sv_solve(uint64_t cur, uint64_t all, int stones, int weak, long long budget, Stack stack, long long* nodes) {
  int lo, hi;
  if (!sv_search(cur, all, stones, -((42 - stones) / 2), (41 - stones) / 2, weak ? -1 : -64, weak ? 1 : 64, budget, stack, nodes, &lo, &hi)) return SV_UNSOLVED;
  return -(weak ? (lo >= 1) - (hi <= -1) : lo);                      // the child's value is seen from its mover
}
// second pass of a query that stayed unsolved beside a best solved q-value `best`: is q <= best proven?  The child's value v = -q, so
// the question is v >= -best.  Strong mode: one pass with the window (-best - 1, -best).  Weak mode (`best` is a sign; +1 bounds
// everything): that score is 0 or 1, the expensive neighbourhood, so the interval is narrowed from outside until it lies on one side.
template <class Stack>
AZ_GHD bool sv_bounded(uint64_t cur, uint64_t all, int stones, int weak, int best, long long budget, Stack stack, long long* nodes) {
  if (weak && best >= 1) return true;
  int lo, hi;
  const bool ok = weak ? sv_search(cur, all, stones, -((42 - stones) / 2), (41 - stones) / 2, -best - 1, -best, budget, stack, nodes, &lo, &hi)
                       : sv_search(cur, all, stones, -best - 1, -best, -64, 64, budget, stack, nodes, &lo, &hi);
  return ok && lo >= -best;
}

#if defined(__HIPCC__)
struct SvLdsStack {
  uint32_t* base;                                                    // &s_stack[0][lane]
  __device__ __forceinline__ uint32_t& operator()(int ply) const { return base[ply * SV_LANES]; }
};

// q [n][7] (SV_NA: full column or terminal state; SV_UNSOLVED: over budget), bounded [n][7] (1: q is unsolved but proven to be no
// more than the state's best solved q), nodes [n][7]
__global__ __launch_bounds__(SV_LANES) void k_c4_solve(const unsigned long long* __restrict__ keys, int n, int weak, long long budget,
                                                       signed char* __restrict__ q, signed char* __restrict__ bounded,
                                                       long long* __restrict__ nodes_out) {
  __shared__ uint32_t s_stack[SV_PLIES][SV_LANES];
  const int lane = threadIdx.x, grp = lane / 7, act = lane % 7;
  const long long state = (long long)blockIdx.x * SV_STATES + grp;
  const bool active = grp < SV_STATES && state < n;
  const SvLdsStack stack{&s_stack[0][lane]};
  uint64_t cur = 0, all = 0;
  int stones = 0, result = SV_NA;
  long long nodes = 0;
  if (active && !sv_child(keys[2 * state], keys[2 * state + 1], act, weak, &cur, &all, &stones, &result))
    result = sv_solve(cur, all, stones, weak, budget, stack, &nodes);
  // every lane of the wavefront is here again: the best solved q of the lane's state
  int best = SV_NA;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int r = __shfl(result, (grp * 7 + j) & (SV_LANES - 1));
    if (r != SV_UNSOLVED && r > best) best = r;
  }
  bool bound = false;
  if (active && result == SV_UNSOLVED && best != SV_NA) bound = sv_bounded(cur, all, stones, weak, best, budget, stack, &nodes);
  if (active) {
    q[state * 7 + act] = (signed char)result;
    bounded[state * 7 + act] = (signed char)bound;
    nodes_out[state * 7 + act] = nodes;
  }
}
#endif
