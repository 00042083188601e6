// ring_books_driver.cpp -- TEST INFRASTRUCTURE: replays a script through csrc/ring_books.h, built by a host compiler from that header
// alone (tests/test_ring_books_cpu.py).
//   ring_books_driver <cap> <op> ...      op = push:<n>:<0|1 advance the batch> | new_batch | empty | set:<total>:<cur_batch>
// Output, one line each: per push "push <n> <skip> <min_seq> <total before>" (skip and min_seq asked BEFORE the push is booked, as the
// callers do), then "len", "batch", "stored_batch", "total", "select0 <n0> <seq0>", "select1 <n0> <seq0>" and, for either selection,
// "runs0" / "runs1" with the <pos>:<run> pieces that read it.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../alphazero.jl_amd/csrc/ring_books.h"

static void print_runs(const char* name, const Ring& ring, const Ring::Selection& s) {
  printf("%s", name);
  for (const Ring::Run& r : ring.runs(s.seq0, s.n0)) printf(" %" PRId64 ":%" PRId64, r.pos, r.run);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <cap> <op> ...\n", argv[0]); return 2; }
  Ring ring;
  ring.cap = (int64_t)atoll(argv[1]);
  if (ring.cap < 1) { fprintf(stderr, "cap must be >= 1\n"); return 2; }
  for (int a = 2; a < argc; ++a) {
    long long x = 0, y = 0;
    if (sscanf(argv[a], "push:%lld:%lld", &x, &y) == 2) {
      printf("push %lld %" PRId64 " %" PRId64 " %" PRId64 "\n", x, ring.skip(x), ring.min_seq(x), ring.total);
      ring.pushed(x, y != 0);
    } else if (sscanf(argv[a], "set:%lld:%lld", &x, &y) == 2) {
      ring.total = x; ring.cur_batch = y;
    } else if (strcmp(argv[a], "new_batch") == 0) ring.new_batch();
    else if (strcmp(argv[a], "empty") == 0) ring.empty();
    else { fprintf(stderr, "bad op %s\n", argv[a]); return 2; }
  }
  const Ring::Selection all = ring.select(0), last = ring.select(1);
  printf("len %" PRId64 "\nbatch %" PRId64 "\nstored_batch %" PRId64 "\ntotal %" PRId64 "\n", ring.len(), ring.batch(), ring.cur_batch, ring.total);
  printf("select0 %" PRId64 " %" PRId64 "\nselect1 %" PRId64 " %" PRId64 "\n", all.n0, all.seq0, last.n0, last.seq0);
  print_runs("runs0", ring, all);
  print_runs("runs1", ring, last);
  return 0;
}
