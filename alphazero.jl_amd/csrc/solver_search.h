// solver_search.h -- the device-free part of the Connect Four solver: the bitboard helpers, the negamax (sv_search) and what a state's
// 7 queries add up to.  Everything here is AZ_GHD and needs no HIP header, so a host compiler can include it alone (the CPU test
// driver tests/solver_table_driver.cpp does); the kernels that run it on the device are in solver.h.  The contract (score
// convention, terminal children, budget, the table) is in include/azhip.h "Connect Four solver".
//
// A lane searches the position AFTER its action with a negamax over bitboards (games.h's 7 bits per column):
//   * `cur` = the stones of the player to move, `all` = every stone; a move is cur ^= all, all |= bit; it is undone by the same two
//     steps backwards, so a ply keeps no board;
//   * a node is only entered when its mover has no winning move (the parent has looked), so what a node does first is to list the moves
//     that do not lose at once: the opponent's winning cells (sv_winning, the shifts of the four axes) that can be played now are
//     forced, two of them lose, and no move may be played right below one.  No such move = the opponent wins with his next stone;
//   * the window is cut to what the remaining cells allow;
//   * the value is closed in on by null-window passes from the root (sv_search), the windows far from 0 first: those are shallow
//     searches, and weak mode stops as soon as the sign is known;
//   * the recursion is an explicit stack of one 32-bit word per ply (`stack(ply)`: LDS on the device, a plain array on the host);
//   * every trip of the loop is one step of the same shape for every lane -- take the child's score, pick the next column, play it,
//     enter the child -- so lanes at different depths of different trees still share the instruction stream.
// Two forms, chosen at compile time (template parameter TT; no runtime branch, the tableless form is the code it was):
//   TT = false   no table; the moves are tried centre first (SV_ORDER, the order of the test suite's CPU negamax).  What is returned
//                depends on (position, weak, budget) and on nothing else.
//   TT = true    a transposition table shared by every lane and call (sv_entry: one 64-bit word = the position's whole key and one
//                bound), probed when a node is entered and written when it is finished, and the moves ordered by the number of
//                winning cells they create (sv_ordered), ties centre first.  Every word ever written is a true statement about
//                the position whose key it carries, and a word is read and written whole, so whatever the table holds and whoever
//                else writes to it, a result is exact; which searches finish within the budget does depend on it.
#pragma once
#include "../../include/azhip.h"
#include "games.h"

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
// frame word, TT = false: bits 0..7 alpha, 8..15 beta (both + 64), 16..22 columns still to try (sv_columns order), 24..26 the column being tried
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

// ---- the table (TT = true) ----
// A position's key: unique per position (Pons' key: in every column the stones of the mover below one bit that marks its height),
// 49 bits, never 0.
constexpr int SV_KEY_BITS = 49;
constexpr uint64_t SV_KEY_MASK = (1ULL << SV_KEY_BITS) - 1;
AZ_GHD uint64_t sv_key(uint64_t cur, uint64_t all) { return cur + all + SV_BOTTOM; }
// The entry of a key in a table of 2^bits words: a multiplicative mix, of which the TOP bits are taken -- the keys of related positions
// share their low bits.
AZ_GHD uint64_t sv_slot(uint64_t key, int bits) {
  uint64_t h = key * 0x9E3779B97F4A7C15ULL;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ULL;
  return bits ? h >> (64 - bits) : 0;
}
// One entry: bits 0..48 the key, bits 49..56 one bound of the position's score, seen from its mover, in true score units (-21..21):
// score <= u is stored as u + 32 (11..53), score >= l as l + 96 (75..117).  0 = empty.  Any other byte is no bound and is ignored.
AZ_GHD uint64_t sv_entry(uint64_t key, int bound, bool lower) { return key | ((uint64_t)(bound + (lower ? 96 : 32)) << SV_KEY_BITS); }
// what a lane without a table hands to sv_search<false>: never called
struct SvNoTable {
  AZ_GHD int bits() const { return 0; }
  AZ_GHD uint64_t load(uint64_t) const { return 0; }
  AZ_GHD void store(uint64_t, uint64_t) const {}
};
// The moves `next` (one cell per column) of the mover `cur`, best first: by the number of winning cells his stones have with the move
// on the board, ties centre first.  Bits 0..20: the columns, 3 bits each, the first to try lowest; bits 21..23: how many.
// Ranks, not a sort: every index below is a constant once the loops are unrolled, so the seven keys stay in registers.
AZ_GHD uint32_t sv_ordered(uint64_t cur, uint64_t all, uint64_t next) {
  uint32_t key[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const uint64_t bit = next & (0x7fULL << (7 * ((SV_ORDER >> (4 * k)) & 7u)));
    key[k] = bit ? ((uint32_t)az_popc64(sv_winning(cur | bit, all | bit)) << 3) | (uint32_t)(7 - k) : 0u;   // distinct where present
  }
  uint32_t q = 0, n = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    uint32_t rank = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) rank += (uint32_t)(key[j] > key[k]);
    if (key[k]) { q |= ((SV_ORDER >> (4 * k)) & 7u) << (3 * rank); ++n; }
  }
  return q | (n << 21);
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
//
// TT = true.  `table`: bits(), load(slot), store(slot, word) over 2^bits() words (relaxed agent-scope atomics on the device, a plain
// array on the host).  Every window of every node is a null window (alpha, alpha + 1) -- a pass starts with one, a child gets
// (-beta, -alpha), and a bound that reaches into a null window closes it -- so the frame word needs alpha alone: bits 0..7 alpha + 64,
// bits 8..31 the moves from the one being tried on (sv_ordered's word).  A node that has tried every move without a cut stores
// "score <= alpha", a node that is cut by a child's score s stores "score >= s": both are statements about the position alone, true
// for any window, mode and caller.  A node left because the budget ran out stores nothing.
template <bool TT, class Stack, class Table>
AZ_GHD bool sv_search(uint64_t cur, uint64_t all, int stones, int mn, int mx, int stop_lo, int stop_hi, long long budget, Stack stack,
                       Table table, long long* nodes_io, int* lo_out, int* hi_out) {
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
        else if constexpr (TT) {
          const uint64_t key = sv_key(cur, all);
          const uint64_t w = table.load(sv_slot(key, table.bits()));
          const int b = (int)(w >> SV_KEY_BITS) & 0xff;
          const bool hit = (w & SV_KEY_MASK) == key;                 // the whole key: never another position's bound
          if (hit && b >= 75 && b <= 117 && b - 96 >= beta) ret = b - 96;        // score >= the bound >= beta
          else if (hit && b >= 11 && b <= 53 && b - 32 <= alpha) ret = b - 32;   // score <= the bound <= alpha
          else { cols = sv_ordered(cur, all, next); returning = false; }
        } else { cols = sv_columns(next); returning = false; }
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
      int col;
      if constexpr (TT) col = (int)(f >> 8) & 7; else col = (int)(f >> 24) & 7;
      const uint64_t top = ((all + (1ULL << (7 * col))) >> 1) & (0x3fULL << (7 * col));   // the stone the move put there
      all ^= top; cur ^= all; --stones;
      if constexpr (TT) {
        alpha = (int)(f & 0xff) - 64; beta = alpha + 1;
        cols = (((f >> 8) & 0x1fffffu) >> 3) | (((f >> 29) - 1u) << 21);   // the move tried leaves the queue
      } else {
        alpha = (int)(f & 0xff) - 64; beta = (int)((f >> 8) & 0xff) - 64; cols = (f >> 16) & 0x7f;
      }
      const int s = -ret;
      if (s >= beta) {                                               // cut: this node is finished too
        ret = s;
        if constexpr (TT) { const uint64_t key = sv_key(cur, all); table.store(sv_slot(key, table.bits()), sv_entry(key, s, true)); }
        continue;
      }
      if (s > alpha) alpha = s;
      returning = false;
    }
    if (!cols) {                                                     // every move tried
      ret = alpha; returning = true;
      if constexpr (TT) { const uint64_t key = sv_key(cur, all); table.store(sv_slot(key, table.bits()), sv_entry(key, alpha, false)); }
      continue;
    }
    if (sp >= SV_PLIES) { over = true; break; }                      // cannot happen (see SV_PLIES); never write past the stack
    int col;
    if constexpr (TT) {
      col = (int)cols & 7;
      stack(sp) = (uint32_t)(alpha + 64) | (cols << 8);              // with the move being tried still at the head of the queue
    } else {
      col = (int)(SV_ORDER >> (4 * __builtin_ctz(cols))) & 7;
      cols &= cols - 1;
      stack(sp) = sv_frame(alpha, beta, cols, col);
    }
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
template <bool TT, class Stack, class Table>
AZ_GHD int sv_solve(uint64_t cur, uint64_t all, int stones, int weak, long long budget, Stack stack, Table table, long long* nodes) {
  int lo, hi;
  if (!sv_search<TT>(cur, all, stones, -((42 - stones) / 2), (41 - stones) / 2, weak ? -1 : -64, weak ? 1 : 64, budget, stack, table, nodes, &lo, &hi)) return SV_UNSOLVED;
  return -(weak ? (lo >= 1) - (hi <= -1) : lo);                      // the child's value is seen from its mover
}
// second pass of a query that stayed unsolved beside a best solved q-value `best`: is q <= best proven?  The child's value v = -q, so
// the question is v >= -best.  Strong mode: one pass with the window (-best - 1, -best).  Weak mode (`best` is a sign; +1 bounds
// everything): that score is 0 or 1, the expensive neighbourhood, so the interval is narrowed from outside until it lies on one side.
// With a table the pass starts from the bounds the first pass left there.
template <bool TT, class Stack, class Table>
AZ_GHD bool sv_bounded(uint64_t cur, uint64_t all, int stones, int weak, int best, long long budget, Stack stack, Table table, long long* nodes) {
  if (weak && best >= 1) return true;
  int lo, hi;
  const bool ok = weak ? sv_search<TT>(cur, all, stones, -((42 - stones) / 2), (41 - stones) / 2, -best - 1, -best, budget, stack, table, nodes, &lo, &hi)
                       : sv_search<TT>(cur, all, stones, -best - 1, -best, -64, 64, budget, stack, table, nodes, &lo, &hi);
  return ok && lo >= -best;
}

// The value of the state (a, b) from its 7 q-values and "bounded" flags (1: q is unsolved but proven to be no more than the state's
// best solved q): Solver.value's terminal branch (solver.jl:69-77: the side to move has lost, or a draw), else the maximum of the
// q-values, or SV_UNSOLVED where an unsolved one might exceed it.
AZ_GHD int sv_state_value(uint64_t a, uint64_t b, const int8_t* q, const int8_t* bounded) {
  const GEnv g = ConnectFour::from_key(a, b);
  if (g.fin & 1) {
    const int stones = az_popc64((g.a | g.b) & ~AZ_BLACK_BIT);
    return (g.fin >> 1) ? -(22 - (stones + 1) / 2) : 0;
  }
  int best = SV_NA;
  bool open = false;                                                 // an unsolved q that is not known to be <= the best solved one
  for (int a7 = 0; a7 < 7; ++a7) {
    if (q[a7] == SV_UNSOLVED) open = open || !bounded[a7];
    else if (q[a7] != SV_NA && q[a7] > best) best = q[a7];
  }
  return (open || best == SV_NA) ? SV_UNSOLVED : best;
}
