// ring_books.h -- the books of a replay memory's circular buffer (MemoryBuffer, src/memory.jl:20-87), written once for the keyed memory
// (memory.hip), the plane memory (plane_memory.hip) and the collective that pushes into one (comm.hip).  Plain C++ (no device runtime,
// no engine.h): a host compiler builds it alone (tests/ring_books_driver.cpp; tests/test_ring_books_cpu.py holds it to a deque).
//
// The sample with sequence number q sits in slot q % cap; the buffer holds the newest len() of the `total` pushed since the last empty().
// The kernels keep taking cap, total, seq0, skip and min_seq as scalars and compute q % cap themselves.  All arithmetic is 64-bit.
//
// What the callers rely on, said here and nowhere else:
//   cur_batch   is stored UNCLAMPED (mem.cur_batch_size) and clamped only where it is read: batch(), select(1).  The plane gather
//               (comm.hip) compares its table with the stored value and refuses a batch larger than cap on its own.
//   pushed      takes all n of a push, the skip(n) that were never stored included.  advance_batch: push_trace! and both gathers
//               (memory.jl:86); a push of samples (push!(mem.buf, sample)) leaves cur_batch alone, so last_batch then selects the
//               newest cur_batch samples whatever pushed them, as the reference's does.
#pragma once
#include <algorithm>
#include <cstdint>

struct Ring {
  int64_t cap = 0, total = 0, cur_batch = 0;

  struct Selection { int64_t n0, seq0; };          // the newest n0 samples, oldest first: sequence numbers seq0 .. seq0 + n0
  struct Run { int64_t pos, run; };                // slots pos .. pos + run, contiguous
  struct Runs {
    Run r[2];
    int n = 0;
    const Run* begin() const { return r; }
    const Run* end() const { return r + n; }
  };

  int64_t len() const { return std::min(total, cap); }
  int64_t batch() const { return std::min(cur_batch, len()); }                       // memory.jl:53
  // which = 0: get_experience, everything held; which = 1: last_batch, the current batch as far as it is still held
  Selection select(int which) const {
    const int64_t n0 = which == 1 ? batch() : len();
    return Selection{n0, total - n0};
  }
  // one push of n: its first skip(n) samples would be overwritten within the very call and are not stored; afterwards the samples
  // with sequence numbers below min_seq(n) are gone.  skip(n) > 0 implies min_seq(n) = total + skip(n).
  int64_t skip(int64_t n) const { return std::max<int64_t>(0, n - cap); }
  int64_t min_seq(int64_t n) const { return std::max<int64_t>(0, total + n - cap); }
  // the slots of sequence numbers seq .. seq + count (0 <= count <= cap), in order: at most two contiguous runs, none of them empty
  Runs runs(int64_t seq, int64_t count) const {
    Runs out;
    while (count > 0) {
      const int64_t pos = seq % cap, run = std::min(count, cap - pos);
      out.r[out.n++] = Run{pos, run};
      seq += run; count -= run;
    }
    return out;
  }
  void pushed(int64_t n, bool advance_batch) { total += n; if (advance_batch) cur_batch += n; }
  void new_batch() { cur_batch = 0; }
  void empty() { total = 0; cur_batch = 0; }
};
