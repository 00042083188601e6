// Prints what csrc/net_layout.h says about one network shape (tests/test_net_layout_cpu.py): the layout table as `at NAME OFFSET` lines
// (names as azhip.network.param_layout's), the trainer's working offsets as `wk NAME OFFSET`, and for every index map a line
// `map NAME COUNT`; the maps themselves go, in that order, as raw int32 into the file named last.  Every index is checked to lie in
// [-1, nparams) (train_scat: in the working array).  Host compiler, net_layout.h only: no HIP, no library.
//   net_layout_driver C P A APAD num_blocks F npf nvf bf16 OUT
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../alphazero.jl_amd/csrc/net_layout.h"

static FILE* g_out;
static long long g_total;
static void put_map(const char* name, const IndexMap& m, long long limit = -1) {   // limit: the indexed array's size where that is not the blob
  if (limit < 0) limit = g_total;
  for (int32_t v : m)
    if (v < -1 || v >= limit) { fprintf(stderr, "%s: index %d outside [-1, %lld)\n", name, (int)v, limit); exit(1); }
  printf("map %s %zu\n", name, m.size());
  if (!m.empty() && fwrite(m.data(), sizeof(int32_t), m.size(), g_out) != m.size()) { perror(name); exit(1); }
}
static void put_conv(const std::string& conv, const std::string& bn, const ConvAt& c) {
  printf("at %s.W %zu\nat %s.b %zu\n", conv.c_str(), c.w, conv.c_str(), c.b);
  printf("at %s.gamma %zu\nat %s.beta %zu\nat %s.mean %zu\nat %s.var %zu\n", bn.c_str(), c.bn_vec(0), bn.c_str(), c.bn_vec(1), bn.c_str(), c.bn_vec(2), bn.c_str(), c.bn_vec(3));
}

int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: %s C P A APAD num_blocks F npf nvf bf16 OUT\n", argv[0]); return 2; }
  int a[9];
  for (int i = 0; i < 9; ++i) a[i] = atoi(argv[1 + i]);
  const NetLayout L(NetShape{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]});
  g_total = (long long)L.total;
  g_out = fopen(argv[10], "wb");
  if (!g_out) { perror(argv[10]); return 1; }
  put_conv("stem.conv", "stem.bn", L.stem());
  for (int l = 0; l < L.ntower(); ++l) {
    const std::string b = "block" + std::to_string(l / 2), k = std::to_string(l % 2 + 1);
    put_conv(b + ".conv" + k, b + ".bn" + k, L.tower(l));
  }
  put_conv("phead.conv", "phead.bn", L.phead());
  printf("at phead.dense.W %zu\nat phead.dense.b %zu\n", L.pd_w, L.pd_b);
  put_conv("vhead.conv", "vhead.bn", L.vhead());
  printf("at vhead.dense1.W %zu\nat vhead.dense1.b %zu\nat vhead.dense2.W %zu\nat vhead.dense2.b %zu\nat total %zu\n", L.v1_w, L.v1_b, L.v2_w, L.v2_b, L.total);

  const NetMaps M(L, a[8] != 0);
  printf("hd_ok %d\nhd16_ok %d\n", (int)M.hd_ok, (int)M.hd16_ok);
  put_map("stem_w", M.stem_w); put_map("s16_w", M.s16_w); put_map("conv_w", M.conv_w); put_map("c16_w", M.c16_w); put_map("c16b_w", M.c16b_w);
  put_map("head_w", M.head_w); put_map("h16_w", M.h16_w); put_map("h16b_w", M.h16b_w); put_map("head_b", M.head_b); put_map("head_bn", M.head_bn);
  put_map("pol_w", M.pol_w); put_map("pol_b", M.pol_b); put_map("val_w", M.val_w); put_map("val_b", M.val_b); put_map("val2_w", M.val2_w);
  put_map("hd_w", M.hd_w); put_map("hd16_w", M.hd16_w);

  const TrainMaps T(L);
  for (size_t l = 0; l < T.conv.size(); ++l) printf("wk conv%zu %zu %zu %zu\n", l, T.conv[l].wm, T.conv[l].ffwd, T.conv[l].fdg);
  printf("wk dense %zu %zu %zu\n", T.pd, T.v1, T.v2);
  put_map("train_map", T.map); put_map("train_scat", T.scat, (long long)T.map.size());
  const std::vector<unsigned char> tr = trainable_mask(L);
  put_map("trainable", IndexMap(tr.begin(), tr.end()), 2);
  if (fclose(g_out) != 0) { perror(argv[10]); return 1; }
  return 0;
}
