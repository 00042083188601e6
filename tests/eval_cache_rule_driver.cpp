// eval_cache_rule_driver.cpp -- TEST INFRASTRUCTURE: answers queries about csrc/eval_cache_rule.h, built by a host compiler from
// that header alone (tests/test_eval_cache_rule_cpu.py).  One query per line of standard input, one answer per line of output:
//   victim <meta0> <meta1> <same0> <same1> <seq> <floor>       -> ec_pick_victim: 0 | 1 | -1
//   size <G> <sims> <override_log2> <free_bytes>               -> ec_size_log2
//   set <ka> <kb> <set_mask>                                   -> ec_set_of, then the byte offsets of the set's two entries
//   hit <meta> <floor> <ka> <kb> <V bits> <cs> <px> <key_a> <key_b>   -> ec_way_hit: 0 | 1 (the hash is taken from key_a, key_b)
//   checksum <px> <ka> <kb> <V bits> <ready_meta>              -> ec_checksum
// Numbers are decimal or 0x-hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../alphazero.jl_amd/csrc/eval_cache_rule.h"

int main() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char op[16] = {0};
    unsigned long long x[9] = {0};
    char w[9][40];
    const int n = sscanf(line, "%15s %39s %39s %39s %39s %39s %39s %39s %39s %39s", op, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]) - 1;
    for (int i = 0; i < n; ++i) x[i] = strtoull(w[i], nullptr, 0);
    if (!strcmp(op, "victim") && n == 6) {
      printf("%d\n", ec_pick_victim((uint32_t)x[0], (uint32_t)x[1], x[2] != 0, x[3] != 0, (uint32_t)x[4], (uint32_t)x[5]));
    } else if (!strcmp(op, "size") && n == 4) {
      printf("%d\n", ec_size_log2((int)x[0], (int)x[1], (int)x[2], x[3]));
    } else if (!strcmp(op, "set") && n == 3) {
      const uint32_t s = ec_set_of(x[0], x[1], (uint32_t)x[2]);
      printf("%" PRIu32 " %llu %llu\n", s, (unsigned long long)(2ull * s) * EC_ENTRY_BYTES, (unsigned long long)(2ull * s + 1) * EC_ENTRY_BYTES);
    } else if (!strcmp(op, "hit") && n == 9) {
      printf("%d\n", ec_way_hit((uint32_t)x[0], (uint32_t)x[1], x[2], x[3], az_u2f((uint32_t)x[4]), (uint32_t)x[5], (uint32_t)x[6], x[7], x[8],
                                az_hash_key(x[7], x[8])) ? 1 : 0);
    } else if (!strcmp(op, "checksum") && n == 5) {
      printf("%" PRIu32 "\n", ec_checksum((uint32_t)x[0], az_hash_key(x[1], x[2]), az_u2f((uint32_t)x[3]), (uint32_t)x[4]));
    } else {
      fprintf(stderr, "bad query: %s", line);
      return 2;
    }
  }
  return 0;
}
