// Prints every field of every struct of csrc/env.h as read from the environment it is started in (tests/test_env_semantics.py).
// Host compiler, env.h only: no HIP, no library.
#include <cstdio>

#include "../alphazero.jl_amd/csrc/env.h"

int main() {
  const EnvCreate c;
  printf("tower_pick=%d\ntower_mixed=%d\nheads_pick=%d\nuse_graphs=%d\ntree_sort=%d\nbk_mode=%d\nexplore_k=%d\n", c.tower_pick, (int)c.tower_mixed,
         c.heads_pick, c.use_graphs, (int)c.tree_sort, c.bk_mode, c.explore_k);
  printf("xch_fail_at=%lld\nxch_epoch0=%llu\npooled_queue=%d\ntag_mask=%u\nepoch0=%u\nvmm=%d\nvmm_keys=%d\n", c.xch_fail_at, c.xch_epoch0,
         (int)c.pooled_queue, (unsigned)c.tag_mask, (unsigned)c.epoch0, c.vmm, (int)c.vmm_keys);
  printf("eval_cache=%d\neval_cache_log2=%d\npool_gb=%g\n", c.eval_cache, c.eval_cache_log2, c.pool_gb);
  const EnvPhase p;
  printf("free_run=%d\nrun_k=%d\nrun_kbg=%d\nround_waves=%d\n", p.free_run, p.run_k, p.run_kbg, p.round_waves);
  const EnvProcess& q = env_process();
  printf("bg_stop=%d\nbg_prio=%d\n", (int)q.bg_stop, q.bg_prio);
  printf("trace=%d\n", (int)EnvArena().trace);
  const EnvTrainer t;
  printf("fin_inside=%d\nconv_nt6=%d\none_stream=%d\nwg_late=%d\n", (int)t.fin_inside, (int)t.conv_nt6, (int)t.one_stream, (int)t.wg_late);
  const EnvComm m;
  printf("rccl_lib=%s\n", m.rccl_lib ? m.rccl_lib : "(null)");
  return 0;
}
