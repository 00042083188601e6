// plane_gather.h -- the plan of az_comm_gather_push_planes, written once.  Plain C++ (no device runtime, no engine.h): a host compiler
// builds it alone (tests/plane_gather_driver.cpp; tests/test_plane_gather_plan_cpu.py holds it to a numpy restatement).
//   record_bytes        how a sample travels: its RW row words padded to 8 bytes, its ND = nA + 2 doubles, n
//   default_round_rows  rows per rank and round R such that the W segments of a round fit STAGING_BYTES
//   make_plan           from the gathered per-rank game tables (id and length per game, in push order): T, the duplicate-id verdict,
//                       per rank the order it packs its games in (ascending id), where each of them lies in its batch, their prefix
//                       sums in packed order and their global start in the id-ordered sequence of ALL ranks' samples; the round split
//   find_game           the game a packed row belongs to (binary search in a rank's prefix sums): what k_pg_pack and k_pg_scatter run
// Every rank computes the same plan from the same tables, so no rank needs to be told where a sample goes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif

namespace pg {

constexpr long long STAGING_BYTES = 256LL << 20;   // most a round receives: W segments of R records

inline long long record_bytes(int RW, int ND) { return 8LL * ((4LL * RW + 7) / 8) + 8LL * ND + 8; }
inline long long default_round_rows(int W, long long rb) { return std::max<long long>(1, STAGING_BYTES / ((long long)W * rb)); }

struct Game { int32_t id, len; };

struct RankPlan {
  long long B = 0;                   // samples of the rank's batch
  std::vector<int> order;            // order[k]: index in the rank's table of its k-th smallest id
  std::vector<long long> src;        // src[k]: where that game's samples begin in the batch, in push order
  std::vector<long long> prefix;     // [games + 1] prefix[k]: rows before it in the id-sorted batch; prefix[games] = B
  std::vector<long long> start;      // start[k]: position of its first sample in the id-ordered sequence of all ranks
};
struct Plan {
  int W = 0;
  long long T = 0, maxB = 0;         // samples of all ranks, of the largest rank
  long long R = 1, rounds = 0;       // rows per rank and round; ceil(maxB / R), the same on every rank
  long long skip = 0;                // positions q < skip are not stored: max(0, T - capacity of the destination)
  bool dup = false;                  // some id occurs twice (on one rank or on two)
  int32_t dup_id = -1;               // the smallest such id
  std::vector<RankPlan> ranks;
};

// largest k in [0, ng) with prefix[k] <= s; needs ng >= 1, 0 <= s < prefix[ng] (lengths are >= 1: prefix is strictly increasing)
PG_HD inline int find_game(const long long* prefix, int ng, long long s) {
  int lo = 0, hi = ng - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// rows the rank sends in round k: [k R, min((k + 1) R, B)), the rest of its segment is padding
inline long long round_rows_of(const Plan& p, int rank, long long k) {
  return std::max<long long>(0, std::min(p.R, p.ranks[(size_t)rank].B - k * p.R));
}

inline Plan make_plan(const std::vector<std::vector<Game>>& tables, long long round_rows, long long cap_dst) {
  Plan p;
  p.W = (int)tables.size();
  p.ranks.resize(tables.size());
  struct Ref { int32_t id; int rank, k; };
  std::vector<Ref> all;
  for (int r = 0; r < p.W; ++r) {
    const std::vector<Game>& t = tables[(size_t)r];
    RankPlan& rp = p.ranks[(size_t)r];
    const int ng = (int)t.size();
    std::vector<long long> off((size_t)ng);                           // push order
    for (int i = 0; i < ng; ++i) { off[(size_t)i] = rp.B; rp.B += t[(size_t)i].len; }
    rp.order.resize((size_t)ng);
    for (int i = 0; i < ng; ++i) rp.order[(size_t)i] = i;
    std::stable_sort(rp.order.begin(), rp.order.end(), [&](int a, int b) { return t[(size_t)a].id < t[(size_t)b].id; });
    rp.src.resize((size_t)ng); rp.prefix.assign((size_t)ng + 1, 0); rp.start.assign((size_t)ng, 0);
    for (int k = 0; k < ng; ++k) {
      const int i = rp.order[(size_t)k];
      rp.src[(size_t)k] = off[(size_t)i];
      rp.prefix[(size_t)k + 1] = rp.prefix[(size_t)k] + t[(size_t)i].len;
      all.push_back(Ref{t[(size_t)i].id, r, k});
    }
    p.T += rp.B;
    p.maxB = std::max(p.maxB, rp.B);
  }
  std::stable_sort(all.begin(), all.end(), [](const Ref& a, const Ref& b) { return a.id < b.id; });
  long long at = 0;
  for (size_t i = 0; i < all.size(); ++i) {
    if (i > 0 && all[i].id == all[i - 1].id && !p.dup) { p.dup = true; p.dup_id = all[i].id; }
    RankPlan& rp = p.ranks[(size_t)all[i].rank];
    rp.start[(size_t)all[i].k] = at;
    at += rp.prefix[(size_t)all[i].k + 1] - rp.prefix[(size_t)all[i].k];
  }
  p.R = std::max<long long>(1, round_rows);
  p.rounds = (p.maxB + p.R - 1) / p.R;
  p.skip = cap_dst > 0 ? std::max<long long>(0, p.T - cap_dst) : p.T;
  return p;
}

}  // namespace pg
