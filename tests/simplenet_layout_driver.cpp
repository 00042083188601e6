// Prints what csrc/net_layout.h says about one SimpleNet shape (tests/test_simplenet_layout_cpu.py): per dense layer a line
// `at L W B BN IN OUT HASBN LAST` (offsets of W, b and the first batch-norm vector; BN = 0 without batch norm), `at total N`, the trainer's
// working offsets as `wk L OFFSET`, and for every index map a line `map NAME COUNT`; the maps themselves go, in that order, as raw int32
// into the file named last.  Every index is checked to lie in [-1, nparams) (train_scat: in the working array).  Host compiler,
// net_layout.h only: no HIP, no library.
//   simplenet_layout_driver indim A width depth_common depth_phead depth_vhead use_batch_norm OUT
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../alphazero.jl_amd/csrc/net_layout.h"

static FILE* g_out;
static long long g_total;
static void put_map(const std::string& name, const IndexMap& m, long long limit = -1) {
  if (limit < 0) limit = g_total;
  for (int32_t v : m)
    if (v < -1 || v >= limit) { fprintf(stderr, "%s: index %d outside [-1, %lld)\n", name.c_str(), (int)v, limit); exit(1); }
  printf("map %s %zu\n", name.c_str(), m.size());
  if (!m.empty() && fwrite(m.data(), sizeof(int32_t), m.size(), g_out) != m.size()) { perror(name.c_str()); exit(1); }
}

int main(int argc, char** argv) {
  if (argc != 9) { fprintf(stderr, "usage: %s indim A width depth_common depth_phead depth_vhead use_batch_norm OUT\n", argv[0]); return 2; }
  int a[7];
  for (int i = 0; i < 7; ++i) a[i] = atoi(argv[1 + i]);
  const SimpleLayout L(SimpleShape{a[0], a[1], a[2], a[3], a[4], a[5], a[6]});
  g_total = (long long)L.total;
  g_out = fopen(argv[8], "wb");
  if (!g_out) { perror(argv[8]); return 1; }
  for (size_t l = 0; l < L.dense.size(); ++l) {
    const DenseAt& d = L.dense[l];
    printf("at %zu %zu %zu %zu %d %d %d %d\n", l, d.w, d.b, d.bn ? d.bn_vec(0) : (size_t)0, d.in, d.out, (int)d.bn, (int)d.last);
  }
  printf("at total %zu\n", L.total);
  printf("heads %d %d %d\n", L.ncommon(), L.pfirst(), L.vfirst());
  const SimpleMaps M(L);
  for (size_t l = 0; l < M.layer.size(); ++l) {
    const std::string p = "l" + std::to_string(l);
    put_map(p + ".w", M.layer[l].w); put_map(p + ".b", M.layer[l].b);
    for (int k = 0; k < 4; ++k) put_map(p + ".bn" + std::to_string(k), M.layer[l].bn[k]);
  }
  const SimpleTrainMaps T(L);
  for (size_t l = 0; l < T.wm.size(); ++l) printf("wk %zu %zu\n", l, T.wm[l]);
  put_map("train_map", T.map); put_map("train_scat", T.scat, (long long)T.map.size());
  const std::vector<unsigned char> tr = trainable_mask(L);
  put_map("trainable", IndexMap(tr.begin(), tr.end()), 2);
  if (fclose(g_out) != 0) { perror(argv[8]); return 1; }
  return 0;
}
