// host_tree.hip -- device search trees for a host-stepped game (include/azhip.h "device search trees"): W per-worker MCTS trees in
// HBM for a game whose rules live on the host.  Select, expand, backup and the transposition lookup run here; the host answers
// "play this action in this node's state" at most once per simulation.  DESIGN.md 4e has the protocol, the layout and the figures.
//
// Layout (struct of arrays, per worker a slice of every array):
//   nodes  [W][NPW]   key (2 x u64), first edge slot, n, Vest, white_playing
//   edges  [W][EPW]   bump-allocated runs of n slots by RANK: P f32, W f64, N i32, action, child, r f64, flags (known / terminal / pswitch)
//   table  [W][HS]    open addressing on az_hash_key(key), entries = node ids, HS = a power of two >= max(64, 2 NPW): never full
//   path   [W][max_depth]  edge slots of the simulation in progress;  eta [W][128] the root's noise;  ws [W] the worker's state
//   pr, pps [W][max_depth] chance mode only (AZ_HOST_TREE_CHANCE): the mover's reward and pswitch of every path entry -- there they
//                          belong to the entry, not to the edge, whose memo (child, r, flags) is never written
// One wavefront per worker (k_ht_step): lanes run over ranks, two per lane beyond 64, so a select is one coalesced load per array.
// Everything a wavefront decides is wave-uniform; values that lanes hand to each other through memory are separated by a barrier
// of the one-wave workgroup.
#include "engine.h"
#include "prims.h"

namespace {
constexpr int HT_MAXA = AZ_HOST_TREE_MAX_ACTIONS;
constexpr int EF_KNOWN = 1, EF_TERMINAL = 2, EF_PSWITCH = 4;
constexpr int PEND_NONE = 0, PEND_PLAY = 1, PEND_ROOT = 2;

struct HTWorker {
  int root, cur, plen, quota;           // root / current node (-1: unknown), path length, simulations still to run (0: disarmed)
  int pending, nnodes, nedges, eta_ok;  // PEND_*, pool fill, the root's noise has been drawn for this explore
  uint32_t game, move;
  int touched, pad;                     // the simulation in progress has asked the host
  long long sims, traversed, evals, thits, nohost;
  int hw_nodes, hw_edges, hw_path, pad2;
};
struct HTReply { unsigned long long k0, k1; float wr; int row; int terminal; int wp; };   // row: index among the non-terminal replies
struct HTArm { int worker, nsims; uint32_t game, move; };

struct HTView {
  int W, nA, NPW, EPW, HS, max_depth, chance;
  double gamma, cpuct, eps, alpha;
  unsigned long long seed;
  unsigned long long* nkey; int* nbase; int* ncount; float* nvest; unsigned char* nwp;
  float* eP; double* eW; int* eN; short* eact; int* echild; double* er; unsigned char* eflag;
  int* table; int* path; double* eta; HTWorker* ws;
  double* pr; unsigned char* pps;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t > v ? t : v; }
  return v;
}
__device__ __forceinline__ int first_lane(unsigned long long b) { return b ? __ffsll((unsigned long long)b) - 1 : 64; }

// the worker's table: node id of (k0, k1) or -1, then *pos = the empty entry an insertion takes
__device__ __forceinline__ int ht_find(const HTView& v, int w, unsigned long long k0, unsigned long long k1, int lane, int* pos) {
  const unsigned mask = (unsigned)v.HS - 1u;
  const unsigned h = (unsigned)az_hash_key(k0, k1);
  const int* tb = v.table + (size_t)w * v.HS;
  const unsigned long long* nk = v.nkey + (size_t)w * v.NPW * 2;
  for (int off = 0; off < v.HS; off += 64) {
    const unsigned slot = (h + (unsigned)off + (unsigned)lane) & mask;
    const int ent = tb[slot];
    const bool empty = ent < 0;
    const bool match = !empty && ent < v.NPW && nk[2 * (size_t)ent] == k0 && nk[2 * (size_t)ent + 1] == k1;
    const int pm = first_lane(__ballot(match)), pe = first_lane(__ballot(empty));
    if (pm < pe) return __shfl(ent, pm);
    if (pe < 64) { *pos = (int)((h + (unsigned)off + (unsigned)pe) & mask); return -1; }
  }
  *pos = -1;                                                        // cannot happen: HS >= 2 NPW
  return -1;
}

// A new node from the row (A, P) and V: ranks by ballot.  false (nothing stored) when a pool is exhausted.
__device__ __forceinline__ bool ht_create(const HTView& v, int w, HTWorker& s, const HTReply& R, const float* Arow, const float* Prow, float vest,
                                          int pos, int lane, int* id_out) {
  const bool l0 = lane < v.nA && Arow[lane] != 0.f;
  const bool l1 = lane + 64 < v.nA && Arow[lane + 64] != 0.f;
  const unsigned long long b0 = __ballot(l0), b1 = __ballot(l1);
  const int n0 = __popcll(b0), n = n0 + __popcll(b1);
  if (s.nnodes >= v.NPW || s.nedges + n > v.EPW || pos < 0) return false;
  const int id = s.nnodes, eb = s.nedges;
  const size_t E = (size_t)w * v.EPW + eb;
  const unsigned long long lt = (1ULL << lane) - 1ULL;
  if (l0) {
    const size_t i = E + __popcll(b0 & lt);
    v.eP[i] = Prow[lane]; v.eW[i] = 0.0; v.eN[i] = 0; v.eact[i] = (short)lane; v.echild[i] = -1; v.er[i] = 0.0; v.eflag[i] = 0;
  }
  if (l1) {
    const size_t i = E + n0 + __popcll(b1 & lt);
    v.eP[i] = Prow[lane + 64]; v.eW[i] = 0.0; v.eN[i] = 0; v.eact[i] = (short)(lane + 64); v.echild[i] = -1; v.er[i] = 0.0; v.eflag[i] = 0;
  }
  if (lane == 0) {
    const size_t nd = (size_t)w * v.NPW + id;
    v.nkey[2 * nd] = R.k0; v.nkey[2 * nd + 1] = R.k1;
    v.nbase[nd] = eb; v.ncount[nd] = n; v.nvest[nd] = vest; v.nwp[nd] = (unsigned char)(R.wp != 0);
    v.table[(size_t)w * v.HS + pos] = id;
  }
  s.nnodes = id + 1; s.nedges = eb + n;
  s.hw_nodes = max(s.hw_nodes, s.nnodes); s.hw_edges = max(s.hw_edges, s.nedges);
  *id_out = id;
  __syncthreads();
  return true;
}

// What the reply R says about the move along the path's last entry (edge slot e, out of a node whose mover is white iff wpp): the mover's
// reward and pswitch, and child = the node it led to or -1 for a terminal state.  Chance mode keeps them with the entry, the
// deterministic mode remembers them on the edge.
__device__ __forceinline__ void ht_record(const HTView& v, int w, int plen, int e, bool wpp, const HTReply& R, int child) {
  const double r = wpp ? (double)R.wr : -(double)R.wr;
  const bool ps = wpp != (R.wp != 0);
  if (v.chance) {
    const size_t i = (size_t)w * v.max_depth + plen - 1;
    v.pr[i] = r; v.pps[i] = (unsigned char)(ps ? EF_PSWITCH : 0);
    return;
  }
  const size_t i = (size_t)w * v.EPW + e;
  v.er[i] = r;
  if (child >= 0) v.echild[i] = child;
  v.eflag[i] = (unsigned char)(EF_KNOWN | (child < 0 ? EF_TERMINAL : 0) | (ps ? EF_PSWITCH : 0));
}

// mcts.jl:216-223 over the path, last entry first; q = the leaf's value.  The chain of q runs in every lane (shuffles), lane k
// updates entry k.  An edge that is on the path twice (a line of play that repeats a state) is updated one entry at a time.
// r and pswitch are the edge's memo, or in chance mode the path entry's own: the mode selects the two base pointers once per call and
// the index per lane (path position or edge slot), so either mode does one load of each and the loop has no mode branch.  The selects
// are not free: DESIGN.md 4e has the deterministic step's time with them and with them compiled out.
__device__ __forceinline__ void ht_unwind(const HTView& v, int w, int plen, double q, int lane) {
  const int* pp = v.path + (size_t)w * v.max_depth;
  const size_t E = (size_t)w * v.EPW;
  const double* rsrc = v.chance ? v.pr + (size_t)w * v.max_depth : v.er + E;
  const unsigned char* fsrc = v.chance ? v.pps + (size_t)w * v.max_depth : v.eflag + E;
  for (int hi = plen; hi > 0; hi -= 64) {
    const int cnt = hi < 64 ? hi : 64;
    int e = -1 - lane; double r = 0.0; int ps = 0;
    if (lane < cnt) { e = pp[hi - 1 - lane]; const int i = v.chance ? hi - 1 - lane : e; r = rsrc[i]; ps = fsrc[i] & EF_PSWITCH; }
    bool dup = false;
    double myq = 0.0;
    for (int k = 0; k < cnt; ++k) {
      const int ek = __shfl(e, k);
      const double rk = __shfl(r, k);
      const int pk = __shfl(ps, k);
      if (k < lane && ek == e) dup = true;
      const double qn = pk ? -q : q;
      q = rk + v.gamma * qn;
      if (lane == k) myq = q;
    }
    if (!__ballot(dup)) {
      if (lane < cnt) { v.eW[E + e] += myq; v.eN[E + e] += 1; }
    } else {
      for (int k = 0; k < cnt; ++k) {
        if (lane == k) { v.eW[E + e] += myq; v.eN[E + e] += 1; }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) k_ht_arm(HTView v, const HTArm* arms, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const HTArm a = arms[i];
  if (a.worker < 0 || a.worker >= v.W) return;
  HTWorker& s = v.ws[a.worker];
  s.quota = a.nsims; s.game = a.game; s.move = a.move; s.eta_ok = 0; s.plen = 0; s.pending = PEND_NONE; s.touched = 0; s.cur = s.root;
}

// One wavefront per active worker: absorb its reply, then unwind / select until it needs the host or its quota is spent.
// active[j] = {worker, index of its reply or -1}; reqtmp[j] = its request (kind -1: none), deptmp[j] = the path length it was asked at.
// Chance mode: the reply to AZ_HT_PLAY gives the path entry its reward and pswitch (ht_record); no edge is ever marked known, so every
// select asks and az_host_tree_advance always forgets the root.
__global__ void __launch_bounds__(64) k_ht_step(HTView v, const int2* active, int nactive, const HTReply* replies, const float* Arows, const float* Prows,
                                                int pstride, const float* Vrows, az_host_tree_request* reqtmp, int* deptmp, int* new_nodes) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= nactive) return;
  const int w = active[j].x, ri = active[j].y;
  if (w < 0 || w >= v.W) return;
  HTWorker s = v.ws[w];
  const size_t NB = (size_t)w * v.NPW, E = (size_t)w * v.EPW;
  int* pp = v.path + (size_t)w * v.max_depth;
  az_host_tree_request rq = {w, -1, -1, -1};
  int rdepth = 0;
  bool unwind = false, descending = false, stop = false;
  double q = 0.0;

  int nn = -1;
  if (ri >= 0 && s.pending != PEND_NONE) {
    const HTReply R = replies[ri];
    if (R.terminal) {                                               // AZ_HT_PLAY only (the host refuses a terminal root)
      if (s.pending == PEND_PLAY && s.plen > 0) {
        const int e = pp[s.plen - 1];
        const bool wpp = v.nwp[NB + s.cur] != 0;
        if (lane == 0) ht_record(v, w, s.plen, e, wpp, R, -1);
        __syncthreads();
        q = 0.0; unwind = true;
      }
    } else {
      s.evals += 1;
      int pos = -1;
      int id = ht_find(v, w, R.k0, R.k1, lane, &pos);
      const bool found = id >= 0;
      bool ok = true;
      if (!found) ok = ht_create(v, w, s, R, Arows + (size_t)R.row * v.nA, Prows + (size_t)R.row * pstride, Vrows[R.row], pos, lane, &id);
      else s.thits += 1;
      if (!ok) {                                                    // AZ_HT_FULL: the simulation is abandoned, nothing of it is stored
        rq.node = s.pending == PEND_PLAY ? s.cur : -1;
        rq.action = s.pending == PEND_PLAY && s.plen > 0 ? (int)v.eact[E + pp[s.plen - 1]] : -1;
        rq.kind = AZ_HT_FULL;
        s.quota = 0; s.plen = 0; stop = true;
      } else {
        nn = id;
        if (s.pending == PEND_PLAY && s.plen > 0) {
          const int e = pp[s.plen - 1];
          const bool wpp = v.nwp[NB + s.cur] != 0;
          if (lane == 0) ht_record(v, w, s.plen, e, wpp, R, id);
          __syncthreads();
        } else {
          s.root = id;
        }
        if (found) { s.cur = id; descending = true; }               // a transposition: the descent goes on from that node
        else { q = (double)Vrows[R.row]; unwind = true; }
      }
    }
    s.pending = PEND_NONE;
  }
  if (ri >= 0 && lane == 0) new_nodes[ri] = nn;

  while (!stop) {
    if (unwind) {
      ht_unwind(v, w, s.plen, q, lane);
      s.sims += 1; s.traversed += s.plen; s.quota -= 1;
      if (!s.touched) s.nohost += 1;
      s.hw_path = max(s.hw_path, s.plen);
      s.plen = 0; unwind = false; descending = false;
    }
    if (!descending) {
      if (s.quota <= 0) { s.quota = 0; break; }
      s.touched = 0; s.plen = 0;
      if (s.root < 0) { rq.kind = AZ_HT_ROOT; s.pending = PEND_ROOT; s.touched = 1; break; }
      s.cur = s.root; descending = true;
    }
    // ---- select at s.cur (mcts.jl:180-188)
    const int nb = v.nbase[NB + s.cur], n = v.ncount[NB + s.cur];
    const bool noise = s.plen == 0 && v.eps != 0.0;
    double* eta = v.eta + (size_t)w * HT_MAXA;
    if (noise && !s.eta_ok) {
      if (lane == 0) { az_rng g = az_rng_make(v.seed, s.game, s.move, AZ_RNG_NOISE); az_dirichlet(&g, n, v.alpha, eta); }
      s.eta_ok = 1;
      __syncthreads();
    }
    const int i0 = lane, i1 = lane + 64;
    const bool h0 = i0 < n, h1 = i1 < n;
    const int N0 = h0 ? v.eN[E + nb + i0] : 0, N1 = h1 ? v.eN[E + nb + i1] : 0;
    const double s_ = __builtin_sqrt((double)wave_sum_i(N0 + N1));
    double sc0 = -__builtin_inf(), sc1 = -__builtin_inf();
    if (h0) {
      const double Q = v.eW[E + nb + i0] / (double)max(N0, 1);
      double Pd = (double)v.eP[E + nb + i0];
      if (noise) Pd = (1.0 - v.eps) * Pd + v.eps * eta[i0];
      sc0 = Q + ((v.cpuct * Pd) * s_) / (double)(N0 + 1);
    }
    if (h1) {
      const double Q = v.eW[E + nb + i1] / (double)max(N1, 1);
      double Pd = (double)v.eP[E + nb + i1];
      if (noise) Pd = (1.0 - v.eps) * Pd + v.eps * eta[i1];
      sc1 = Q + ((v.cpuct * Pd) * s_) / (double)(N1 + 1);
    }
    const double m = wave_max_d(sc0 > sc1 ? sc0 : sc1);
    const unsigned long long b0 = __ballot(h0 && sc0 == m), b1 = __ballot(h1 && sc1 == m);
    const int best = b0 ? first_lane(b0) : b1 ? 64 + first_lane(b1) : 0;      // the first maximum
    const int e = nb + best;
    if (s.plen >= v.max_depth) {                                    // AZ_HT_DEPTH: abandoned, nothing backed up
      rq.node = s.cur; rq.action = (int)v.eact[E + e]; rq.kind = AZ_HT_DEPTH;
      s.quota = 0; s.plen = 0; break;
    }
    if (lane == 0) pp[s.plen] = e;
    s.plen += 1;
    __syncthreads();
    const int fl = v.eflag[E + e];
    if (!(fl & EF_KNOWN)) {                                         // chance mode: always, no edge is ever marked known
      rq.node = s.cur; rq.action = (int)v.eact[E + e]; rq.kind = AZ_HT_PLAY; rdepth = s.plen - 1;
      s.pending = PEND_PLAY; s.touched = 1;
      break;
    }
    if (fl & EF_TERMINAL) { q = 0.0; unwind = true; continue; }
    s.cur = v.echild[E + e];
  }
  if (lane == 0) { v.ws[w] = s; reqtmp[j] = rq; deptmp[j] = rdepth; }
}

// requests of the active workers and their depths, compacted in worker order: out[0] = count, reqs[0 .. count), deps[0 .. count)
__global__ void __launch_bounds__(256) k_ht_compact(const az_host_tree_request* reqtmp, const int* deptmp, int nactive, int* count, az_host_tree_request* reqs,
                                                    int* deps) {
  __shared__ int s_wave[4];
  int base = 0;
  for (int t0 = 0; t0 < nactive; t0 += 256) {
    const int i = t0 + threadIdx.x;
    const bool has = i < nactive && reqtmp[i].kind >= 0;
    int total;
    const int off = prims::block_excl_scan(has ? 1 : 0, s_wave, &total);
    if (has) { reqs[base + off] = reqtmp[i]; deps[base + off] = deptmp[i]; }
    base += total;
  }
  if (threadIdx.x == 0) *count = base;
}

// tree[root] of one worker by full action index
__global__ void __launch_bounds__(64) k_ht_root_stats(HTView v, const int* workers, int n, int* N, double* Wt, float* P, float* Vest, int* root) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const int w = workers[i];
  if (w < 0 || w >= v.W) return;
  for (int a = lane; a < v.nA; a += 64) { N[(size_t)i * v.nA + a] = 0; Wt[(size_t)i * v.nA + a] = 0.0; P[(size_t)i * v.nA + a] = 0.f; }
  __syncthreads();
  const int r = v.ws[w].root;
  if (lane == 0) { root[i] = r; Vest[i] = r >= 0 ? v.nvest[(size_t)w * v.NPW + r] : 0.f; }
  if (r < 0) return;
  const int nb = v.nbase[(size_t)w * v.NPW + r], cnt = v.ncount[(size_t)w * v.NPW + r];
  const size_t E = (size_t)w * v.EPW + nb;
  for (int k = lane; k < cnt; k += 64) {
    const int a = v.eact[E + k];
    if (a < 0 || a >= v.nA) continue;
    N[(size_t)i * v.nA + a] = v.eN[E + k]; Wt[(size_t)i * v.nA + a] = v.eW[E + k]; P[(size_t)i * v.nA + a] = v.eP[E + k];
  }
}

// apply == 0: res[i] = 1 where the root of workers[i] is known and has no edge `actions[i]`; apply != 0: the root moves along it
// (chance mode: to "unknown" for every action the root has -- the device cannot know where the real move led)
__global__ void __launch_bounds__(64) k_ht_advance(HTView v, const int* workers, const int* actions, int n, int apply, int* res) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int w = workers[i];
  if (w < 0 || w >= v.W) return;
  HTWorker& s = v.ws[w];
  int r = s.root, bad = 0, next = -1;
  if (r >= 0) {
    const int nb = v.nbase[(size_t)w * v.NPW + r], cnt = v.ncount[(size_t)w * v.NPW + r];
    const size_t E = (size_t)w * v.EPW + nb;
    int k = 0;
    while (k < cnt && v.eact[E + k] != actions[i]) ++k;
    if (k == cnt) bad = 1;
    else if (!v.chance && (v.eflag[E + k] & (EF_KNOWN | EF_TERMINAL)) == EF_KNOWN) next = v.echild[E + k];
  }
  if (!apply) { res[i] = bad; return; }
  if (!bad) { s.root = next; s.cur = next; s.plen = 0; }
}

__global__ void __launch_bounds__(64) k_ht_reset(HTView v, const int* workers, int n) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const int w = workers[i];
  if (w < 0 || w >= v.W) return;
  int* tb = v.table + (size_t)w * v.HS;
  for (int k = threadIdx.x; k < v.HS; k += 64) tb[k] = -1;
  if (threadIdx.x == 0) {
    HTWorker& s = v.ws[w];
    s.root = -1; s.cur = -1; s.plen = 0; s.quota = 0; s.pending = PEND_NONE; s.nnodes = 0; s.nedges = 0; s.eta_ok = 0; s.touched = 0;
  }
}
}  // namespace

// ------------------------------------------------------------------------------- host side
struct az_host_tree {
  az_engine* e = nullptr;
  int device = 0;
  hipStream_t stream = nullptr; bool own_stream = false;
  az_host_tree_cfg cfg = {};
  HTView v = {};
  int xs = 0;                                // engine mode: C*H*W
  std::vector<void*> allocs;
  char* h_in = nullptr; char* d_in = nullptr; size_t in_bytes = 0;      // pinned / device staging of a step's input, one layout
  char* h_out = nullptr; char* d_out = nullptr; size_t out_bytes = 0;   // count, new_nodes, requests (and the results of the other calls)
  float* h_X = nullptr;                      // engine mode: pinned rows for the engine's d_X
  az_host_tree_request* d_reqtmp = nullptr; int* d_deptmp = nullptr;
  std::vector<az_host_tree_request> outstanding;   // AZ_HT_PLAY / AZ_HT_ROOT requests of the last step, in order
  std::vector<int32_t> depths;                     // the path length each of them was asked at (az_host_tree_request_depths)
  std::vector<uint8_t> armed;
  std::vector<HTArm> arms;                   // az_host_tree_explore since the last step
  long long steps = 0;
  // az_debug_host_tree_profile: HIP events around the tree kernels of a step (arm, step, compact), summed after the step's synchronisation
  bool prof = false; hipEvent_t ev[2] = {nullptr, nullptr}; double kernel_ms = 0; long long prof_steps = 0;
};

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
template <class T> static int ht_alloc(az_host_tree* t, T** p, size_t n) { return mem_alloc(&t->allocs, p, n); }

extern "C" int az_host_tree_cfg_init(az_host_tree_cfg* cfg) {
  if (!cfg) return fail(AZ_ERR_BAD_ARG, "cfg is NULL");
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (int32_t)sizeof *cfg;
  cfg->gamma = 1.0; cfg->cpuct = 1.0; cfg->dirichlet_noise_eps = 0.0; cfg->dirichlet_noise_alpha = 1.0; cfg->prior_temperature = 1.0;
  return AZ_OK;
}

extern "C" int az_host_tree_destroy(az_host_tree* t) {
  if (!t) return AZ_OK;
  (void)hipSetDevice(t->device);
  if (t->own_stream && t->stream) (void)hipStreamSynchronize(t->stream);   // every call returns with its stream idle; the engine's may be gone by now
  for (void* p : t->allocs) (void)hipFree(p);
  if (t->h_in) (void)hipHostFree(t->h_in);
  if (t->h_out) (void)hipHostFree(t->h_out);
  if (t->h_X) (void)hipHostFree(t->h_X);
  for (hipEvent_t ev : t->ev) if (ev) (void)hipEventDestroy(ev);
  if (t->own_stream && t->stream) (void)hipStreamDestroy(t->stream);
  delete t;
  return AZ_OK;
}

static int ht_create_body(az_host_tree* t) {
  HTView& v = t->v;
  const size_t W = (size_t)v.W, NN = W * v.NPW, NE = W * v.EPW;
  AZCHK(ht_alloc(t, &v.nkey, NN * 2)); AZCHK(ht_alloc(t, &v.nbase, NN)); AZCHK(ht_alloc(t, &v.ncount, NN)); AZCHK(ht_alloc(t, &v.nvest, NN)); AZCHK(ht_alloc(t, &v.nwp, NN));
  AZCHK(ht_alloc(t, &v.eP, NE)); AZCHK(ht_alloc(t, &v.eW, NE)); AZCHK(ht_alloc(t, &v.eN, NE)); AZCHK(ht_alloc(t, &v.eact, NE)); AZCHK(ht_alloc(t, &v.echild, NE));
  AZCHK(ht_alloc(t, &v.er, NE)); AZCHK(ht_alloc(t, &v.eflag, NE));
  AZCHK(ht_alloc(t, &v.table, W * v.HS)); AZCHK(ht_alloc(t, &v.path, W * v.max_depth)); AZCHK(ht_alloc(t, &v.eta, W * HT_MAXA)); AZCHK(ht_alloc(t, &v.ws, W));
  AZCHK(ht_alloc(t, &t->d_reqtmp, W)); AZCHK(ht_alloc(t, &t->d_deptmp, W));
  if (v.chance) { AZCHK(ht_alloc(t, &v.pr, W * v.max_depth)); AZCHK(ht_alloc(t, &v.pps, W * v.max_depth)); }
  // a step's input: active [W] int2, arms [W], replies [W], V [W], A [W][nA], P [W][nA]; the other calls use the front of it
  t->in_bytes = al16(W * sizeof(int2)) + al16(W * sizeof(HTArm)) + al16(W * sizeof(HTReply)) + al16(W * 4) + 2 * al16(W * v.nA * 4);
  // a step's output: count (16 bytes), new_nodes [W], requests [W], their depths [W]; root_stats: N, W, P [W][nA], Vest, root [W]
  t->out_bytes = std::max(16 + 2 * al16(W * 4) + al16(W * sizeof(az_host_tree_request)), al16(W * v.nA * 8) + 2 * al16(W * v.nA * 4) + 2 * al16(W * 4));
  AZCHK(ht_alloc(t, &t->d_in, t->in_bytes)); AZCHK(ht_alloc(t, &t->d_out, t->out_bytes));
  HIPCHK(hipHostMalloc((void**)&t->h_in, t->in_bytes, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&t->h_out, t->out_bytes, hipHostMallocDefault));
  if (t->e) HIPCHK(hipHostMalloc((void**)&t->h_X, W * t->xs * sizeof(float), hipHostMallocDefault));
  HIPCHK(hipMemsetAsync(v.table, 0xff, W * v.HS * sizeof(int), t->stream));
  HIPCHK(hipMemsetAsync(v.eflag, 0, NE, t->stream));
  std::vector<HTWorker> ws(W);
  for (auto& s : ws) { memset(&s, 0, sizeof s); s.root = -1; s.cur = -1; }
  HIPCHK(hipMemcpyAsync(v.ws, ws.data(), W * sizeof(HTWorker), hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  t->armed.assign(W, 0);
  return AZ_OK;
}

extern "C" int az_host_tree_create(az_engine* e, int32_t device, int32_t num_actions, int32_t num_workers, int32_t nodes_per_worker,
                                   int32_t edge_slots_per_worker, int32_t max_depth, const az_host_tree_cfg* cfg, az_host_tree** out) {
  if (!out) return fail(AZ_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!cfg || cfg->struct_size != (int32_t)sizeof(az_host_tree_cfg)) return fail(AZ_ERR_BAD_ARG, "az_host_tree_cfg: NULL or wrong struct_size (use az_host_tree_cfg_init)");
  if (const unsigned unknown = (unsigned)cfg->flags & ~(unsigned)AZ_HOST_TREE_CHANCE)   // names the lowest bit nobody defined
    return fail(AZ_ERR_BAD_ARG, "az_host_tree_cfg.flags = 0x%x: bit 0x%x is not defined (AZ_HOST_TREE_CHANCE = 0x%x is the only one)", (unsigned)cfg->flags,
                unknown & (0u - unknown), (unsigned)AZ_HOST_TREE_CHANCE);
  if (cfg->prior_temperature != 1.0) return fail(AZ_ERR_BAD_ARG, "prior_temperature = %g: only 1 is built for the device trees of a host-stepped game", cfg->prior_temperature);
  if (!std::isfinite(cfg->gamma) || !std::isfinite(cfg->cpuct)) return fail(AZ_ERR_BAD_ARG, "gamma / cpuct must be finite");
  if (!(cfg->dirichlet_noise_eps >= 0.0 && cfg->dirichlet_noise_eps <= 1.0)) return fail(AZ_ERR_BAD_ARG, "dirichlet_noise_eps = %g outside [0, 1]", cfg->dirichlet_noise_eps);
  if (cfg->dirichlet_noise_eps != 0.0 && !(cfg->dirichlet_noise_alpha > 0.0 && std::isfinite(cfg->dirichlet_noise_alpha))) return fail(AZ_ERR_BAD_ARG, "dirichlet_noise_alpha = %g must be positive", cfg->dirichlet_noise_alpha);
  if (num_actions < 1 || num_actions > HT_MAXA) return fail(AZ_ERR_BAD_ARG, "num_actions = %d outside 1..%d (AZ_HOST_TREE_MAX_ACTIONS)", num_actions, HT_MAXA);
  if (num_workers < 1 || num_workers > (1 << 20)) return fail(AZ_ERR_BAD_ARG, "num_workers = %d outside 1..2^20", num_workers);
  if (nodes_per_worker < 1 || nodes_per_worker > (1 << 28)) return fail(AZ_ERR_BAD_ARG, "nodes_per_worker = %d outside 1..2^28", nodes_per_worker);
  if (edge_slots_per_worker < num_actions) return fail(AZ_ERR_BAD_ARG, "edge_slots_per_worker = %d below num_actions = %d", edge_slots_per_worker, num_actions);
  if (max_depth < 1) return fail(AZ_ERR_BAD_ARG, "max_depth = %d below 1", max_depth);
  if (e) {
    if (!oracle_is_net(e->cfg)) return fail(AZ_ERR_BAD_ARG, "engine mode needs an engine with a network oracle");
    if (!e->net_loaded) return fail(AZ_ERR_STATE, "az_net_set_params has not been called");
    if (num_actions != e->gi.A) return fail(AZ_ERR_BAD_ARG, "num_actions = %d, the engine's game has %d", num_actions, e->gi.A);
    if (num_workers > e->nn_cap) return fail(AZ_ERR_BAD_ARG, "num_workers = %d above the %d rows one network launch of the engine takes", num_workers, e->nn_cap);
    device = e->device;
  }
  AZCHK(use_device(device));
  az_host_tree* t = new (std::nothrow) az_host_tree;
  if (!t) return fail(AZ_ERR_HIP, "out of host memory");
  t->e = e; t->device = device; t->cfg = *cfg;
  if (e) { t->stream = e->stream; t->xs = e->gi.C * e->gi.P; }
  else {
    hipError_t r = hipStreamCreate(&t->stream);
    if (r != hipSuccess) { delete t; return fail(AZ_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(r)); }
    t->own_stream = true;
  }
  HTView& v = t->v;
  v.W = num_workers; v.nA = num_actions; v.NPW = nodes_per_worker; v.EPW = edge_slots_per_worker; v.max_depth = max_depth;
  v.HS = 64; while (v.HS < 2 * (long long)nodes_per_worker) v.HS <<= 1;
  v.chance = (cfg->flags & AZ_HOST_TREE_CHANCE) != 0;
  v.gamma = cfg->gamma; v.cpuct = cfg->cpuct; v.eps = cfg->dirichlet_noise_eps; v.alpha = cfg->dirichlet_noise_alpha; v.seed = cfg->seed;
  const int st = ht_create_body(t);
  if (st != AZ_OK) { const std::string keep = az_last_error(); az_host_tree_destroy(t); return fail(st, "%s", keep.c_str()); }
  *out = t;
  return AZ_OK;
}

#define HTREE(t)                                                  \
  if (!(t)) return fail(AZ_ERR_BAD_ARG, "host tree is NULL");     \
  HIPCHK(hipSetDevice((t)->device))

// workers[0 .. n): in range, and (unless armed_ok) not armed; names the first offender
static int ht_check_workers(az_host_tree* t, const char* who, int32_t n, const int32_t* workers) {
  if (n < 0 || n > t->v.W || (n > 0 && !workers)) return fail(AZ_ERR_BAD_ARG, "%s: n = %d outside 0..%d, or workers is NULL", who, n, t->v.W);
  for (int i = 0; i < n; ++i)
    if (workers[i] < 0 || workers[i] >= t->v.W) return fail(AZ_ERR_BAD_ARG, "%s: workers[%d] = %d outside 0..%d", who, i, workers[i], t->v.W - 1);
  for (int i = 0; i < n; ++i)
    if (t->armed[workers[i]]) return fail(AZ_ERR_STATE, "%s: worker %d (workers[%d]) is armed: its explore has not finished", who, workers[i], i);
  return AZ_OK;
}

extern "C" int az_host_tree_explore(az_host_tree* t, int32_t n, const int32_t* workers, const uint32_t* game_ids, const uint32_t* moves, int32_t nsims) {
  HTREE(t);
  AZCHK(ht_check_workers(t, "az_host_tree_explore", n, workers));
  if (n > 0 && (!game_ids || !moves)) return fail(AZ_ERR_BAD_ARG, "az_host_tree_explore: game_ids / moves is NULL");
  if (nsims < 1) return fail(AZ_ERR_BAD_ARG, "az_host_tree_explore: nsims = %d below 1", nsims);
  for (int i = 0; i < n; ++i) {                                      // a worker named twice: the marks are taken back before anything is kept
    if (t->armed[workers[i]]) {
      for (int k = 0; k < i; ++k) t->armed[workers[k]] = 0;
      return fail(AZ_ERR_STATE, "az_host_tree_explore: worker %d (workers[%d]) is named twice", workers[i], i);
    }
    t->armed[workers[i]] = 1;
  }
  for (int i = 0; i < n; ++i) t->arms.push_back(HTArm{workers[i], nsims, game_ids[i], moves[i]});
  return AZ_OK;
}

extern "C" int az_host_tree_step(az_host_tree* t, int32_t nreplies, const az_host_tree_reply* replies, const float* X, const float* A, const float* P,
                                 const float* V, az_host_tree_request* requests, int32_t* nrequests, int32_t* new_nodes) {
  HTREE(t);
  const HTView& v = t->v;
  const int nA = v.nA;
  if (!requests || !nrequests || !new_nodes) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: requests / nrequests / new_nodes is NULL");
  if (nreplies != (int32_t)t->outstanding.size())
    return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: %d replies for %d outstanding requests", nreplies, (int)t->outstanding.size());
  if (nreplies > 0 && !replies) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: replies is NULL");
  // ---- every refusal comes before anything is staged or stored
  int nrows = 0;
  for (int i = 0; i < nreplies; ++i) {
    const az_host_tree_reply& r = replies[i];
    const az_host_tree_request& q = t->outstanding[i];
    if (!std::isfinite(r.white_reward)) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): white_reward is not finite", i, q.worker);
    if (r.terminal > 1 || r.white_playing > 1) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): terminal / white_playing outside {0, 1}", i, q.worker);
    if (r.terminal) {
      if (q.kind == AZ_HT_ROOT) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): a terminal root cannot be explored", i, q.worker);
      continue;
    }
    if (!A || (t->e ? !X : (!P || !V))) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d is not terminal and %s is NULL", i, !A ? "A" : t->e ? "X" : "P or V");
    const float* a = A + (size_t)i * nA;
    int legal = 0;
    for (int k = 0; k < nA; ++k) {
      if (a[k] != 0.f && a[k] != 1.f) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): A[%d] = %g outside {0, 1}", i, q.worker, k, (double)a[k]);
      legal += a[k] == 1.f;
    }
    if (!legal) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): the A row has no legal action", i, q.worker);
    if (!t->e) {
      const float* p = P + (size_t)i * nA;
      for (int k = 0; k < nA; ++k) {
        if (!std::isfinite(p[k]) || p[k] < 0.f) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): P[%d] = %g is negative or not finite", i, q.worker, k, (double)p[k]);
        if (p[k] > 0.f && a[k] == 0.f) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): P[%d] = %g > 0 where A == 0", i, q.worker, k, (double)p[k]);
      }
      if (!std::isfinite(V[i])) return fail(AZ_ERR_BAD_ARG, "az_host_tree_step: reply %d (worker %d): V is not finite", i, q.worker);
    }
    ++nrows;
  }
  if (t->e && nrows > 0 && !t->e->net_loaded) return fail(AZ_ERR_STATE, "az_net_set_params has not been called");
  // ---- the active workers in worker order: those that are answered and those armed since the last step
  const int narms = (int)t->arms.size();
  const int nactive = nreplies + narms;
  *nrequests = 0;
  if (nactive == 0) return AZ_OK;
  const size_t W = (size_t)v.W;
  size_t o = 0;
  int2* h_active = (int2*)(t->h_in + o); const size_t o_active = o; o += al16(W * sizeof(int2));
  HTArm* h_arms = (HTArm*)(t->h_in + o); const size_t o_arms = o; o += al16((size_t)narms * sizeof(HTArm));
  HTReply* h_rep = (HTReply*)(t->h_in + o); const size_t o_rep = o; o += al16((size_t)nreplies * sizeof(HTReply));
  float* h_V = (float*)(t->h_in + o); const size_t o_V = o; o += al16((size_t)nrows * 4);
  float* h_A = (float*)(t->h_in + o); const size_t o_A = o; o += al16((size_t)nrows * nA * 4);
  float* h_P = (float*)(t->h_in + o); const size_t o_P = o; if (!t->e) o += al16((size_t)nrows * nA * 4);
  // (sections are laid out for the counts of this step; o <= in_bytes because every count is <= W)
  for (int i = 0; i < nreplies; ++i) h_active[i] = make_int2(t->outstanding[i].worker, i);
  for (int i = 0; i < narms; ++i) { h_active[nreplies + i] = make_int2(t->arms[i].worker, -1); h_arms[i] = t->arms[i]; }
  std::sort(h_active, h_active + nactive, [](const int2& a, const int2& b) { return a.x < b.x; });
  int row = 0;
  for (int i = 0; i < nreplies; ++i) {
    const az_host_tree_reply& r = replies[i];
    HTReply& d = h_rep[i];
    d.k0 = r.key[0]; d.k1 = r.key[1]; d.wr = r.white_reward; d.terminal = r.terminal; d.wp = r.white_playing; d.row = r.terminal ? -1 : row;
    if (r.terminal) continue;
    memcpy(h_A + (size_t)row * nA, A + (size_t)i * nA, sizeof(float) * nA);
    if (t->e) memcpy(t->h_X + (size_t)row * t->xs, X + (size_t)i * t->xs, sizeof(float) * t->xs);
    else { memcpy(h_P + (size_t)row * nA, P + (size_t)i * nA, sizeof(float) * nA); h_V[row] = V[i]; }
    ++row;
  }
  hipStream_t st = t->stream;
  HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, o, hipMemcpyHostToDevice, st));
  const float* d_A = (const float*)(t->d_in + o_A); const float* d_P = (const float*)(t->d_in + o_P); const float* d_V = (const float*)(t->d_in + o_V);
  int pstride = nA;
  if (t->e && nrows > 0) {                                           // the network on every non-terminal row, in reply order, one launch
    az_engine* e = t->e;
    HIPCHK(hipMemcpyAsync(e->d_X, t->h_X, sizeof(float) * (size_t)nrows * t->xs, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->d_A, t->d_in + o_A, sizeof(float) * (size_t)nrows * nA, hipMemcpyDeviceToDevice, st));
    AZCHK(net_seam_planes(e, nrows));
    d_P = e->d_P; d_V = e->d_V; pstride = e->gi.A;
  }
  if (t->prof) HIPCHK(hipEventRecord(t->ev[0], st));
  if (narms) hipLaunchKernelGGL(k_ht_arm, dim3((narms + 63) / 64), dim3(64), 0, st, t->v, (const HTArm*)(t->d_in + o_arms), narms);
  int* d_count = (int*)t->d_out; int* d_nn = (int*)(t->d_out + 16);
  const size_t o_req = 16 + al16((size_t)nreplies * 4), o_dep = o_req + (size_t)nactive * sizeof(az_host_tree_request);
  az_host_tree_request* d_req = (az_host_tree_request*)(t->d_out + o_req);
  hipLaunchKernelGGL(k_ht_step, dim3(nactive), dim3(64), 0, st, t->v, (const int2*)(t->d_in + o_active), nactive, (const HTReply*)(t->d_in + o_rep), d_A, d_P,
                     pstride, d_V, t->d_reqtmp, t->d_deptmp, d_nn);
  hipLaunchKernelGGL(k_ht_compact, dim3(1), dim3(256), 0, st, (const az_host_tree_request*)t->d_reqtmp, (const int*)t->d_deptmp, nactive, d_count, d_req,
                     (int*)(t->d_out + o_dep));
  if (t->prof) HIPCHK(hipEventRecord(t->ev[1], st));
  const size_t ob = o_dep + (size_t)nactive * sizeof(int);
  HIPCHK(hipMemcpyAsync(t->h_out, t->d_out, ob, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (t->e && t->e->xch_epoch) AZCHK(check_device_error(t->e));
  t->steps += 1;
  if (t->prof) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, t->ev[0], t->ev[1])); t->kernel_ms += ms; t->prof_steps += 1; }
  // ---- the step happened: bookkeeping of who is armed, the outstanding requests
  const int nreq = std::min(std::max(*(int*)t->h_out, 0), nactive);
  const az_host_tree_request* hr = (const az_host_tree_request*)(t->h_out + o_req);
  const int32_t* hd = (const int32_t*)(t->h_out + o_dep);
  for (int i = 0; i < nactive; ++i) t->armed[h_active[i].x] = 0;
  t->arms.clear();
  t->outstanding.clear(); t->depths.clear();
  for (int i = 0; i < nreq; ++i) {
    requests[i] = hr[i];
    if (hr[i].kind == AZ_HT_PLAY || hr[i].kind == AZ_HT_ROOT) { t->outstanding.push_back(hr[i]); t->depths.push_back(hd[i]); t->armed[hr[i].worker] = 1; }
  }
  memcpy(new_nodes, t->h_out + 16, sizeof(int32_t) * (size_t)nreplies);
  *nrequests = nreq;
  return AZ_OK;
}

extern "C" int az_host_tree_request_depths(az_host_tree* t, int32_t* depths, int32_t cap, int32_t* n) {
  if (!t) return fail(AZ_ERR_BAD_ARG, "host tree is NULL");
  if (!n) return fail(AZ_ERR_BAD_ARG, "az_host_tree_request_depths: n is NULL");
  *n = (int32_t)t->depths.size();
  if (*n == 0) return AZ_OK;
  if (!depths || cap < *n) return fail(AZ_ERR_CAPACITY, "az_host_tree_request_depths: %d outstanding requests, room for %d", *n, depths ? cap : 0);
  memcpy(depths, t->depths.data(), sizeof(int32_t) * (size_t)*n);
  return AZ_OK;
}

extern "C" int az_host_tree_root_stats(az_host_tree* t, int32_t n, const int32_t* workers, int32_t* N, double* Wt, float* P, float* Vest, int32_t* root_node) {
  HTREE(t);
  AZCHK(ht_check_workers(t, "az_host_tree_root_stats", n, workers));
  if (n == 0) return AZ_OK;
  const int nA = t->v.nA;
  const size_t W = (size_t)t->v.W;
  const size_t oW = 0, oN = al16(W * nA * 8), oP = oN + al16(W * nA * 4), oV = oP + al16(W * nA * 4), oR = oV + al16(W * 4);
  memcpy(t->h_in, workers, sizeof(int32_t) * (size_t)n);
  hipStream_t st = t->stream;
  HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ht_root_stats, dim3(n), dim3(64), 0, st, t->v, (const int*)t->d_in, (int)n, (int*)(t->d_out + oN), (double*)(t->d_out + oW),
                     (float*)(t->d_out + oP), (float*)(t->d_out + oV), (int*)(t->d_out + oR));
  HIPCHK(hipMemcpyAsync(t->h_out, t->d_out, oR + sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (N) memcpy(N, t->h_out + oN, sizeof(int32_t) * (size_t)n * nA);
  if (Wt) memcpy(Wt, t->h_out + oW, sizeof(double) * (size_t)n * nA);
  if (P) memcpy(P, t->h_out + oP, sizeof(float) * (size_t)n * nA);
  if (Vest) memcpy(Vest, t->h_out + oV, sizeof(float) * (size_t)n);
  if (root_node) memcpy(root_node, t->h_out + oR, sizeof(int32_t) * (size_t)n);
  return AZ_OK;
}

extern "C" int az_host_tree_advance(az_host_tree* t, int32_t n, const int32_t* workers, const int32_t* actions) {
  HTREE(t);
  AZCHK(ht_check_workers(t, "az_host_tree_advance", n, workers));
  if (n == 0) return AZ_OK;
  if (!actions) return fail(AZ_ERR_BAD_ARG, "az_host_tree_advance: actions is NULL");
  for (int i = 0; i < n; ++i)
    if (actions[i] < 0 || actions[i] >= t->v.nA) return fail(AZ_ERR_BAD_ARG, "az_host_tree_advance: actions[%d] = %d outside 0..%d (worker %d)", i, actions[i], t->v.nA - 1, workers[i]);
  int32_t* hw = (int32_t*)t->h_in; int32_t* ha = hw + n;
  memcpy(hw, workers, sizeof(int32_t) * (size_t)n); memcpy(ha, actions, sizeof(int32_t) * (size_t)n);
  hipStream_t st = t->stream;
  HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
  const int* dw = (const int*)t->d_in; const int* da = dw + n;
  hipLaunchKernelGGL(k_ht_advance, dim3((n + 63) / 64), dim3(64), 0, st, t->v, dw, da, (int)n, 0, (int*)t->d_out);
  HIPCHK(hipMemcpyAsync(t->h_out, t->d_out, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i)
    if (((int32_t*)t->h_out)[i]) return fail(AZ_ERR_BAD_ARG, "az_host_tree_advance: worker %d (workers[%d]): its root has no action %d", workers[i], i, actions[i]);
  hipLaunchKernelGGL(k_ht_advance, dim3((n + 63) / 64), dim3(64), 0, st, t->v, dw, da, (int)n, 1, (int*)t->d_out);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return AZ_OK;
}

extern "C" int az_host_tree_reset(az_host_tree* t, int32_t n, const int32_t* workers) {
  HTREE(t);
  AZCHK(ht_check_workers(t, "az_host_tree_reset", n, workers));
  if (n == 0) return AZ_OK;
  memcpy(t->h_in, workers, sizeof(int32_t) * (size_t)n);
  hipStream_t st = t->stream;
  HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ht_reset, dim3(n), dim3(64), 0, st, t->v, (const int*)t->d_in, (int)n);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return AZ_OK;
}

extern "C" int az_host_tree_get_stats(az_host_tree* t, az_host_tree_stats* stats) {
  HTREE(t);
  if (!stats) return fail(AZ_ERR_BAD_ARG, "stats is NULL");
  std::vector<HTWorker> ws((size_t)t->v.W);
  HIPCHK(hipMemcpyAsync(ws.data(), t->v.ws, ws.size() * sizeof(HTWorker), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  memset(stats, 0, sizeof *stats);
  for (const HTWorker& s : ws) {
    stats->simulations += s.sims; stats->nodes_traversed += s.traversed; stats->evaluations += s.evals; stats->transposition_hits += s.thits;
    stats->sims_without_host += s.nohost;
    stats->max_nodes = std::max<int64_t>(stats->max_nodes, s.hw_nodes); stats->max_edge_slots = std::max<int64_t>(stats->max_edge_slots, s.hw_edges);
    stats->max_path = std::max<int64_t>(stats->max_path, s.hw_path);
  }
  stats->steps = t->steps;
  return AZ_OK;
}

// Debug seams (not in azhip.h; a caller declares them itself): HIP-event time of the tree kernels alone -- arm, step, compact; not the copies, not
// the network -- summed over the steps since profiling was switched on (examples/host_stepped_go9 --device-trees reports it).
extern "C" int az_debug_host_tree_profile(az_host_tree* t, int32_t on) {
  HTREE(t);
  if (on && !t->ev[0]) { HIPCHK(hipEventCreate(&t->ev[0])); HIPCHK(hipEventCreate(&t->ev[1])); }
  t->prof = on != 0; t->kernel_ms = 0; t->prof_steps = 0;
  return AZ_OK;
}
extern "C" int az_debug_host_tree_kernel_ms(az_host_tree* t, double* ms, int64_t* steps) {
  HTREE(t);
  if (ms) *ms = t->kernel_ms;
  if (steps) *steps = t->prof_steps;
  return AZ_OK;
}
