// comm.hip -- the multi-GPU exchange of the path, behind the C ABI: RCCL over xGMI, one process per GPU.
//
//   simulate_distributed (src/simulations.jl:252-290): the games are split over the workers, every worker simulates its share
//     with NO communication (az_selfplay_run with global game ids), then the results are fetched and concatenated;
//   self_play_step! (src/training.jl:284-299) pushes every trace into the replay memory (push_trace!, src/memory.jl:74-87);
//   the new network goes out to the workers before the next phase (the closure serialised by Distributed, training.jl:278-282).
//
// Here: az_comm_gather_push = ONE all-gather of the ranks' device-resident move records (64 B per position) + one of
// their game records (56 B per game), straight from the engines' phase buffers into every rank's device buffer, and
// push_trace! of all games in global game-id order into the rank's az_memory -- no record visits the host, only the
// game records come back (they carry the counts).  az_comm_broadcast_params = ncclBroadcast of the parameter blob.
// az_comm_gather_push_planes is the same exchange for a host-stepped game, whose samples are rows of planes in an az_plane_memory
// (plane_memory.hip): the ranks' current batches travel as records of rb bytes, in rounds that bound the staging, and land in every
// rank's destination memory in global game-id order (plane_gather.h has the plan, k_pg_pack / k_pg_scatter below move the rows).
// RCCL is dlopen'ed by path next to the HIP runtime this library uses (a process that also imports PyTorch holds a second,
// bundled RCCL: binding by soname could hand our communicator to that copy's HIP runtime), on first use only: single-GPU
// users never load it.  The unique id travels between the processes by whatever the host has (Julia's Distributed, MPI,
// a file; bench.py uses torch.distributed's gloo store).
//
// Transport seam: AZHIP_RCCL_LIB=<path> makes rc::load() open that library instead of RCCL.  It exists so that the W > 1
// branches below (padding, per-rank offsets, the re-ordering by global game id) can be EXECUTED on a box with one GPU, where
// RCCL itself refuses two ranks per device: tests/rccl_stub/ builds a test-only library with the same six entry points that
// moves the bytes through host shared memory.  The product never sets the variable.
//
// Failure agreement: every local reason to refuse (no phase, wrong device, allocation failure, the root without parameters)
// is turned into a status word that travels with the first all-gather of a call, so all ranks leave together instead of one
// rank returning while the others wait inside ncclAllGather for ever; a failing collective aborts the communicator.
#include "engine.h"
#include "plane_gather.h"

#include <dlfcn.h>

// The part of RCCL's C ABI this file binds (rccl.h, NCCL 2.x ABI: stable enum values), declared here so that building
// libazhip.so does not need the RCCL development headers -- the library is dlopen'ed on first use only.
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclInt64 = 4, ncclFloat32 = 7 } ncclDataType_t;
}

namespace rc {
struct Lib {
  void* so = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;      // optional
  std::string path;                                // what was loaded (az_comm_version)
};
static Lib g;
static int load() {
  if (g.so) return AZ_OK;
  void* so = nullptr;
  Dl_info info;
  const char* forced = EnvComm().rccl_lib;
  if (forced && *forced) {
    // a transport seam for the tests (several ranks on one GPU: tests/rccl_stub), not a plug-in point: only a library that calls
    // itself librccl* is accepted, and it must export the NCCL entry points below like the real one
    const char* base = strrchr(forced, '/');
    base = base ? base + 1 : forced;
    if (strncmp(base, "librccl", 7) != 0) return fail(AZ_ERR_COMM, "AZHIP_RCCL_LIB=%s: not a librccl* library", forced);
    so = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    if (!so) return fail(AZ_ERR_COMM, "cannot load AZHIP_RCCL_LIB=%s (%s)", forced, dlerror());
  }
  if (!so && dladdr(reinterpret_cast<void*>(&hipGetLastError), &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    const size_t k = p.rfind('/');
    if (k != std::string::npos) so = dlopen((p.substr(0, k) + "/librccl.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!so && k != std::string::npos) so = dlopen((p.substr(0, k) + "/librccl.so.1").c_str(), RTLD_NOW | RTLD_LOCAL);
  }
  if (!so) so = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!so) so = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!so) return fail(AZ_ERR_COMM, "cannot load librccl.so (%s)", dlerror());
  g.GetUniqueId = (decltype(g.GetUniqueId))dlsym(so, "ncclGetUniqueId");
  g.CommInitRank = (decltype(g.CommInitRank))dlsym(so, "ncclCommInitRank");
  g.CommDestroy = (decltype(g.CommDestroy))dlsym(so, "ncclCommDestroy");
  g.CommAbort = (decltype(g.CommAbort))dlsym(so, "ncclCommAbort");
  g.AllGather = (decltype(g.AllGather))dlsym(so, "ncclAllGather");
  g.Broadcast = (decltype(g.Broadcast))dlsym(so, "ncclBroadcast");
  g.GetErrorString = (decltype(g.GetErrorString))dlsym(so, "ncclGetErrorString");
  g.GetVersion = (decltype(g.GetVersion))dlsym(so, "ncclGetVersion");
  if (Dl_info li; g.GetUniqueId && dladdr(reinterpret_cast<void*>(g.GetUniqueId), &li) && li.dli_fname) g.path = li.dli_fname;
  if (!g.GetUniqueId || !g.CommInitRank || !g.CommDestroy || !g.AllGather || !g.Broadcast || !g.GetErrorString)
    return fail(AZ_ERR_COMM, "librccl.so lacks the expected symbols");
  g.so = so;
  return AZ_OK;
}
}  // namespace rc

#define RCCLCHK(x)                                                                                              \
  do {                                                                                                          \
    ncclResult_t _r = (x);                                                                                      \
    if (_r != ncclSuccess) return fail(AZ_ERR_COMM, "%s failed: %s (%s:%d)", #x, rc::g.GetErrorString(_r), __FILE__, __LINE__); \
  } while (0)

struct az_comm {                                    // every member starts here: az_comm_destroy takes a half-made record apart
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1, device = 0;
  hipStream_t stream = nullptr;
  // status / count words of the failure agreement, allocated ONCE at az_comm_init: a collective call must not be able to fail
  // locally (an allocation) before it has entered the first all-gather, or the other ranks would wait in it for ever
  long long *d_word_send = nullptr, *d_word_all = nullptr;   // [COMM_WORDS], [COMM_WORDS * world]
  // az_comm_gather_push_planes: rows per rank and round forced by az_debug_comm_plane_round_rows (0: the default), the events that
  // time its kernels (created here for the same reason as the words) and the sums of its last call
  int64_t plane_round_rows = 0;
  hipEvent_t ev[4] = {};
  double pack_ms = 0.0, scatter_ms = 0.0;
};
static constexpr int COMM_WORDS = 4;               // az_comm_gather_push_planes sends four (count, samples, status, geometry), the others three or one
static_assert(sizeof(ncclUniqueId) == AZ_COMM_ID_BYTES, "ncclUniqueId size");

extern "C" int az_comm_unique_id(uint8_t* id) {
  if (!id) return fail(AZ_ERR_BAD_ARG, "NULL");
  AZCHK(rc::load());
  ncclUniqueId u;
  RCCLCHK(rc::g.GetUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return AZ_OK;
}

extern "C" int az_comm_version(int32_t* version, char* path, int32_t cap) {
  AZCHK(rc::load());
  int v = 0;
  if (rc::g.GetVersion && rc::g.GetVersion(&v) != ncclSuccess) v = 0;
  if (version) *version = v;
  if (path && cap > 0) { strncpy(path, rc::g.path.c_str(), (size_t)cap - 1); path[cap - 1] = 0; }
  return AZ_OK;
}

extern "C" int az_comm_destroy(az_comm* c) {
  if (!c) return AZ_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)rc::g.CommDestroy(c->comm);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->d_word_send) (void)hipFree(c->d_word_send);
  if (c->d_word_all) (void)hipFree(c->d_word_all);
  for (hipEvent_t ev : c->ev) if (ev) (void)hipEventDestroy(ev);
  delete c;
  return AZ_OK;
}

extern "C" int az_comm_init(int32_t device, int32_t rank, int32_t world, const uint8_t* id, az_comm** out) {
  if (!id || !out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world) return fail(AZ_ERR_BAD_ARG, "rank %d of %d", rank, world);
  AZCHK(rc::load());
  AZCHK(use_device(device));
  az_comm* c = new (std::nothrow) az_comm();
  if (!c) return fail(AZ_ERR_HIP, "out of host memory");
  c->rank = rank; c->world = world; c->device = device;
  int st = [&]() -> int {
    HIPCHK(hipStreamCreate(&c->stream));
    HIPCHK(hipMalloc((void**)&c->d_word_send, COMM_WORDS * sizeof(long long)));
    HIPCHK(hipMalloc((void**)&c->d_word_all, (size_t)COMM_WORDS * world * sizeof(long long)));
    for (hipEvent_t& ev : c->ev) HIPCHK(hipEventCreate(&ev));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCLCHK(rc::g.CommInitRank(&c->comm, world, u, rank));
    return AZ_OK;
  }();
  if (st != AZ_OK) { az_comm_destroy(c); return st; }
  *out = c;
  return AZ_OK;
}

// packs the phase's move records in game-id order: game i of the order -> out[dst[i] ..), from d_phase[src[i] ..)
static __global__ void k_pack_moves(const az_move_rec* __restrict__ phase, const long long* __restrict__ src, const long long* __restrict__ dst,
                                    const int* __restrict__ cnt, int ngames, az_move_rec* __restrict__ out) {
  const int g = blockIdx.x;
  if (g >= ngames) return;
  const uint4* s = (const uint4*)(phase + src[g]);
  uint4* d = (uint4*)(out + dst[g]);
  for (int k = threadIdx.x; k < cnt[g] * 4; k += blockDim.x) d[k] = s[k];
}

// ---- the failure agreement ----------------------------------------------------------------------------------------------------------
// a collective failed half way: the other ranks may be inside it -- tear the communicator down so that they fail too
static void abort_comm(az_comm* c) {
  if (c->comm && rc::g.CommAbort) { (void)rc::g.CommAbort(c->comm); c->comm = nullptr; }
}
#define COMM_ALIVE(c) if (!(c)->comm) return fail(AZ_ERR_COMM, "the communicator was aborted by an earlier failed collective")
// A collective step: what `body` issues is what the other ranks wait for, so a failure inside it aborts the communicator.  Whatever
// an entry point does outside a step fails locally and leaves the communicator alone -- where a failure happens decides, nothing else.
template <class F> static int collective(az_comm* c, F&& body) {
  const int st = body();
  if (st != AZ_OK) abort_comm(c);
  return st;
}
// every collective call's first step after its argument checks
static int comm_device(az_comm* c) {
  return collective(c, [&]() -> int {
    if (hipSetDevice(c->device) != hipSuccess) return fail(AZ_ERR_HIP, "hipSetDevice(%d) failed; communicator aborted", c->device);
    return AZ_OK;
  });
}
// What a rank found wrong before an exchange; its status word travels, its message stays for the rank's own report.
struct Verdict {
  int status;
  std::string msg;
  explicit Verdict(int st) : status(st), msg(st != AZ_OK ? az_last_error() : "") {}
};
// One exchange: nw <= COMM_WORDS words of every rank, all[nw * r ..) = rank r's.  The words live in buffers allocated at az_comm_init,
// so nothing can fail locally before the all-gather.
static int exchange_words(az_comm* c, const long long* words, int nw, std::vector<long long>* all) {
  all->resize((size_t)nw * c->world);
  return collective(c, [&]() -> int {
    HIPCHK(hipMemcpyAsync(c->d_word_send, words, sizeof(long long) * nw, hipMemcpyHostToDevice, c->stream));
    RCCLCHK(rc::g.AllGather(c->d_word_send, c->d_word_all, (size_t)nw, ncclInt64, c->comm, c->stream));
    HIPCHK(hipMemcpyAsync(all->data(), c->d_word_all, sizeof(long long) * all->size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return AZ_OK;
  });
}
// After an exchange whose word `at` is each rank's status: a failing rank reports its own reason, the others name the first rank that
// failed through others(rank, its status word); AZ_OK when every rank is fine.  All ranks leave together either way.
template <class F> static int settle(const Verdict& mine, const std::vector<long long>& all, int nw, int at, F&& others) {
  if (mine.status != AZ_OK) return fail(mine.status, "%s", mine.msg.c_str());
  for (size_t r = 0; r * nw < all.size(); ++r)
    if (all[r * nw + at] != AZ_OK) return others((int)r, all[r * nw + at]);
  return AZ_OK;
}
// The buffers of a gather are sized by the largest rank: a rank that cannot allocate them says so before anything is exchanged.
// One rank has nobody to tell.
static int agree_allocated(az_comm* c, int alloc_status) {
  if (c->world == 1) return alloc_status;
  const Verdict own(alloc_status);
  const long long word = alloc_status;
  std::vector<long long> all;
  AZCHK(exchange_words(c, &word, 1, &all));
  return settle(own, all, 1, 0, [](int r, long long) { return fail(AZ_ERR_COMM, "rank %d could not allocate the gather buffers; nothing was exchanged", r); });
}

extern "C" int az_comm_gather_push(az_comm* c, az_engine* e, az_memory* m, double gamma, az_gather_stats* stats) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "NULL communicator");
  COMM_ALIVE(c);
  AZCHK(comm_device(c));
  // local validation first; its verdict travels with the counts, so that every rank returns together (never one rank
  // leaving while the others sit in ncclAllGather)
  int local = AZ_OK;
  if (!e) local = fail(AZ_ERR_BAD_ARG, "NULL engine");
  else if (e->device != c->device || (m && m->device != c->device)) local = fail(AZ_ERR_BAD_ARG, "engine / memory / communicator are on different devices");
  else if (m && m->game != e->cfg.game) local = fail(AZ_ERR_BAD_ARG, "memory and engine differ in game");
  else if (e->ph.running) local = fail(AZ_ERR_STATE, "self-play in progress");
  else if (!e->d_phase) local = fail(AZ_ERR_STATE, "the engine holds no device-resident phase (az_selfplay_run first)");
  else local = sync_all(e);
  const Verdict own(local);
  const auto t0 = std::chrono::steady_clock::now();
  const int W = c->world;
  std::vector<long long> src, dst;
  std::vector<int> cnt;
  std::vector<az_game_rec> gsend;
  if (local == AZ_OK) phase_games_by_id(e, &src, &cnt, &gsend);
  const size_t ng = gsend.size();
  long long nm = 0;
  for (size_t i = 0; i < ng; ++i) { dst.push_back(nm); gsend[i].first_move = (int32_t)nm; nm += cnt[i]; }
  // 1. counts and status of every rank
  const long long hc[3] = {(long long)ng, nm, (long long)local};
  std::vector<long long> all;
  AZCHK(exchange_words(c, hc, 3, &all));
  AZCHK(settle(own, all, 3, 2, [](int r, long long status) {
    return fail(AZ_ERR_COMM, "rank %d cannot take part in the gather (status %lld); nothing was exchanged", r, status);
  }));
  long long maxg = 1, maxm = 1, totg = 0, totm = 0;
  for (int r = 0; r < W; ++r) { maxg = std::max(maxg, all[3 * r]); maxm = std::max(maxm, all[3 * r + 1]); totg += all[3 * r]; totm += all[3 * r + 1]; }
  // 2. this rank's records packed in game-id order, then the two all-gathers (equal, padded segments per rank)
  Scratch tmp;
  az_move_rec *d_msend = nullptr, *d_mall = nullptr; az_game_rec *d_gsend = nullptr, *d_gall = nullptr; long long *d_src = nullptr, *d_dst = nullptr; int* d_n = nullptr;
  AZCHK(agree_allocated(c, [&]() -> int {
    AZCHK(tmp.alloc(&d_msend, (size_t)maxm)); AZCHK(tmp.alloc(&d_mall, (size_t)maxm * W));
    AZCHK(tmp.alloc(&d_gsend, (size_t)maxg)); AZCHK(tmp.alloc(&d_gall, (size_t)maxg * W));
    AZCHK(tmp.alloc(&d_src, std::max<size_t>(ng, 1))); AZCHK(tmp.alloc(&d_dst, std::max<size_t>(ng, 1))); AZCHK(tmp.alloc(&d_n, std::max<size_t>(ng, 1)));
    return AZ_OK;
  }()));
  // 3. the game records (56 B per game) tell where every game's records sit in the gathered buffer
  std::vector<az_game_rec> gall((size_t)maxg * W);
  AZCHK(collective(c, [&]() -> int {
    if (ng) {
      HIPCHK(hipMemcpyAsync(d_src, src.data(), sizeof(long long) * ng, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(d_dst, dst.data(), sizeof(long long) * ng, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(d_n, cnt.data(), sizeof(int) * ng, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(d_gsend, gsend.data(), sizeof(az_game_rec) * ng, hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(k_pack_moves, dim3((unsigned)ng), dim3(64), 0, c->stream, e->d_phase, d_src, d_dst, d_n, (int)ng, d_msend);
    }
    RCCLCHK(rc::g.AllGather(d_msend, d_mall, (size_t)maxm * sizeof(az_move_rec), ncclInt8, c->comm, c->stream));
    RCCLCHK(rc::g.AllGather(d_gsend, d_gall, (size_t)maxg * sizeof(az_game_rec), ncclInt8, c->comm, c->stream));
    HIPCHK(hipMemcpyAsync(gall.data(), d_gall, sizeof(az_game_rec) * gall.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return AZ_OK;
  }));
  const auto t1 = std::chrono::steady_clock::now();
  struct Ref { int32_t id; long long first; int n; };
  std::vector<Ref> refs;
  refs.reserve((size_t)totg);
  for (int r = 0; r < W; ++r)
    for (long long i = 0; i < all[3 * r]; ++i) {
      const az_game_rec& gr = gall[(size_t)r * maxg + i];
      refs.push_back({gr.game_id, (long long)r * maxm + gr.first_move, gr.num_moves});   // rank r's segment starts at r * maxm
    }
  std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return a.id < b.id; });
  if (m) {
    std::vector<long long> first(refs.size());
    std::vector<int> n(refs.size());
    for (size_t i = 0; i < refs.size(); ++i) { first[i] = refs[i].first; n[i] = refs[i].n; }
    AZCHK(memory_push_device(m, d_mall, first, n, gamma));
  }
  if (stats) {
    stats->games = totg; stats->moves = totm;
    stats->bytes = (int64_t)W * (maxm * (long long)sizeof(az_move_rec) + maxg * (long long)sizeof(az_game_rec) + 24);
    stats->gather_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // Report.SelfPlay wants mean depth and the largest tree over ALL games (training.jl:293-296), not the rank's own
    long long sims = 0, trav = 0, nodes = 0, repl = 0;
    for (int r = 0; r < W; ++r)
      for (long long i = 0; i < all[3 * r]; ++i) {
        const az_game_rec& gr = gall[(size_t)r * maxg + i];
        repl += (gr.game_id & AZ_REPLACEMENT_GAME_BIT) != 0;
        sims += gr.total_simulations; trav += gr.total_nodes_traversed; nodes = std::max<long long>(nodes, gr.nodes);
      }
    double dsum = 0.0;                 // mean over games of each game's average depth, in global game-id order
    {
      std::vector<std::pair<int32_t, double>> dep;
      dep.reserve((size_t)totg);
      for (int r = 0; r < W; ++r)
        for (long long i = 0; i < all[3 * r]; ++i) {
          const az_game_rec& gr = gall[(size_t)r * maxg + i];
          dep.push_back({gr.game_id, gr.total_simulations ? (double)gr.total_nodes_traversed / (double)gr.total_simulations : 0.0});
        }
      std::sort(dep.begin(), dep.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
      for (const auto& d : dep) dsum += d.second;
    }
    stats->ranks = W;
    stats->total_simulations = sims; stats->total_nodes_traversed = trav; stats->max_nodes = nodes;
    stats->mean_game_depth = totg ? dsum / (double)totg : 0.0;
    stats->replaced_games = repl;
  }
  return AZ_OK;
}

extern "C" int az_comm_broadcast_params(az_comm* c, az_engine* e, int32_t root) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "NULL communicator");
  COMM_ALIVE(c);
  if (root < 0 || root >= c->world) return fail(AZ_ERR_BAD_ARG, "root %d of %d", root, c->world);   // the same argument on every rank
  AZCHK(comm_device(c));
  int local = AZ_OK;
  int64_t n = 0;
  if (!e) local = fail(AZ_ERR_BAD_ARG, "NULL engine");
  else if (e->device != c->device) local = fail(AZ_ERR_BAD_ARG, "engine and communicator are on different devices");
  else if (!oracle_is_net(e->cfg)) local = fail(AZ_ERR_STATE, "engine was created without a network oracle");
  else if (c->rank == root && !e->net_loaded) local = fail(AZ_ERR_STATE, "the root has no parameters loaded");
  else local = az_net_num_params(e, &n);
  std::vector<float> h;
  {                                  // the staging buffer is freed before the engine allocates its packed copies
    Scratch tmp;
    float* d = nullptr;
    if (local == AZ_OK) local = tmp.alloc(&d, (size_t)n);
    const Verdict own(local);
    const long long word = local;
    std::vector<long long> all;
    AZCHK(exchange_words(c, &word, 1, &all));
    AZCHK(settle(own, all, 1, 0, [&](int r, long long) {
      return fail(AZ_ERR_COMM, "rank %d cannot take part in the broadcast%s; nothing was sent", r, r == root ? " (the root has no parameters?)" : "");
    }));
    h.resize((size_t)n);
    AZCHK(collective(c, [&]() -> int {
      if (c->rank == root) HIPCHK(hipMemcpyAsync(d, e->blob.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
      RCCLCHK(rc::g.Broadcast(d, d, (size_t)n, ncclFloat32, root, c->comm, c->stream));
      HIPCHK(hipMemcpyAsync(h.data(), d, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      return AZ_OK;
    }));
  }
  // Network.copy(nn; on_gpu = true, test_mode = true) on every rank: the kernels want their packed fragments
  return az_net_set_params(e, h.data(), n);
}

// ---- plane samples: az_comm_gather_push_planes ---------------------------------------------------------------------------------------
// A record = [RW row words, padded to 8 bytes][ND doubles][n]: rb = pg::record_bytes bytes, 8-byte aligned.  Both kernels follow
// k_pm_store: one wavefront per row, lanes over words.  V is the widest word both sides of the ROW copy are aligned to: ring rows are
// 4 RW bytes apart, records rb bytes (uint4 for Tic-tac-toe, uint2 for Mancala and Go, one word for Connect Four's odd RW); the doubles
// and n go as 8-byte words.
template <typename V> struct PgVec { static constexpr int WORDS = (int)(sizeof(V) / 4); };

// Row i of the round = row s = base + i of the rank's id-sorted batch: game g = find_game(prefix, s), batch sample j = src[g] + (s -
// prefix[g]) in push order, ring slot (seq0 + j) % cap with seq0 = total - B (the batch may straddle the ring's end).
template <typename V>
__global__ void __launch_bounds__(64 * PM_WAVES) k_pg_pack(const float* __restrict__ XA, const double* __restrict__ D, const long long* __restrict__ N,
                                                           long long cap, long long seq0, long long base, long long nrows,
                                                           const long long* __restrict__ prefix, const long long* __restrict__ src, int ng,
                                                           int RW, int ND, long long rb, unsigned char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (i >= nrows) return;
  const long long s = base + i;
  const int g = pg::find_game(prefix, ng, s);
  const size_t slot = (size_t)((seq0 + src[g] + (s - prefix[g])) % cap);
  unsigned char* rec = out + (size_t)i * (size_t)rb;
  const V* xs = (const V*)(XA + slot * RW);
  V* xd = (V*)rec;
  const int nv = RW / PgVec<V>::WORDS;
  for (int w = lane; w < nv; w += 64) xd[w] = xs[w];
  if ((RW & 1) && lane == 0) ((unsigned int*)rec)[RW] = 0u;          // the padding word travels as zero
  const unsigned long long* ds = (const unsigned long long*)(D + slot * ND);
  unsigned long long* dd = (unsigned long long*)rec + (RW + 1) / 2;
  for (int w = lane; w < ND; w += 64) dd[w] = ds[w];
  if (lane == 0) dd[ND] = (unsigned long long)N[slot];
}
// One wavefront per received row: segment r = row / R of the round holds rank r's rows [base, base + R) of ITS sorted batch, the ones
// at or past B[r] being padding.  q = start[r][g] + offset is the sample's position in the id-ordered sequence of all T samples:
// q < skip would be overwritten within this very call (k_pm_store's skip), the others land in slot (total + q) % cap.  q is a
// bijection onto [0, T): no slot is written twice, no atomics.
template <typename V>
__global__ void __launch_bounds__(64 * PM_WAVES) k_pg_scatter(const unsigned char* __restrict__ in, long long R, long long base, int W,
                                                              const long long* __restrict__ B, const long long* __restrict__ goff,
                                                              const long long* __restrict__ prefix_all, const long long* __restrict__ start_all,
                                                              long long skip, long long total, long long cap, int RW, int ND, long long rb,
                                                              float* __restrict__ XA, double* __restrict__ D, long long* __restrict__ N) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (row >= (long long)W * R) return;
  const int r = (int)(row / R);
  const long long s = base + row % R;
  if (s >= B[r]) return;
  const long long g0 = goff[r];
  const long long* prefix = prefix_all + g0 + r;                      // rank r's games + 1 prefix sums
  const int g = pg::find_game(prefix, (int)(goff[r + 1] - g0), s);
  const long long q = start_all[g0 + g] + (s - prefix[g]);
  if (q < skip) return;
  const size_t slot = (size_t)((total + q) % cap);
  const unsigned char* rec = in + (size_t)row * (size_t)rb;
  const V* xs = (const V*)rec;
  V* xd = (V*)(XA + slot * RW);
  const int nv = RW / PgVec<V>::WORDS;
  for (int w = lane; w < nv; w += 64) xd[w] = xs[w];
  const unsigned long long* ds = (const unsigned long long*)rec + (RW + 1) / 2;
  unsigned long long* dd = (unsigned long long*)(D + slot * ND);
  for (int w = lane; w < ND; w += 64) dd[w] = ds[w];
  if (lane == 0) N[slot] = (long long)ds[ND];
}

extern "C" int az_debug_comm_plane_round_rows(az_comm* c, int64_t rows) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "NULL communicator");
  if (rows < 0) return fail(AZ_ERR_BAD_ARG, "rows must be >= 0");
  c->plane_round_rows = rows;
  return AZ_OK;
}
extern "C" int az_debug_comm_plane_kernel_ms(az_comm* c, double* pack_ms, double* scatter_ms) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "NULL communicator");
  if (pack_ms) *pack_ms = c->pack_ms;
  if (scatter_ms) *scatter_ms = c->scatter_ms;
  return AZ_OK;
}

extern "C" int az_comm_gather_push_planes(az_comm* c, az_plane_memory* src, az_plane_memory* dst, const int32_t* game_ids, const int32_t* game_lens,
                                          int32_t num_games, az_gather_stats* stats) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "NULL communicator");
  COMM_ALIVE(c);
  AZCHK(comm_device(c));
  // local validation first; its verdict travels with the counts and the geometry (az_comm_gather_push)
  long long B = 0;
  int local = [&]() -> int {
    if (!src) return fail(AZ_ERR_BAD_ARG, "NULL source memory");
    if (dst == src) return fail(AZ_ERR_BAD_ARG, "the destination is the source memory: an outbox cannot receive its own batch");
    if (src->device != c->device || (dst && dst->device != c->device)) return fail(AZ_ERR_BAD_ARG, "source / destination memory and communicator are on different devices");
    if (dst && (dst->xs != src->xs || dst->nA != src->nA)) return fail(AZ_ERR_BAD_ARG, "source and destination memory differ in geometry (%d + %d and %d + %d words per row)", src->xs, src->nA, dst->xs, dst->nA);
    if (num_games < 0 || (num_games > 0 && (!game_ids || !game_lens))) return fail(AZ_ERR_BAD_ARG, num_games < 0 ? "num_games must be >= 0" : "NULL game table");
    for (int k = 0; k < num_games; ++k) {
      if (game_lens[k] < 1) return fail(AZ_ERR_BAD_ARG, "game %d of the table (id %d) has length %d: must be >= 1", k, (int)game_ids[k], (int)game_lens[k]);
      if (game_ids[k] < 0) return fail(AZ_ERR_BAD_ARG, "game %d of the table has the negative id %d", k, (int)game_ids[k]);
      B += game_lens[k];
    }
    // the table must account for the batch as it was pushed (the stored, unclamped count), and all of it must still be held
    if (B != src->ring.cur_batch) return fail(AZ_ERR_BAD_ARG, "the table's lengths sum to %lld, the source's current batch holds %lld samples", B, (long long)src->ring.cur_batch);
    if (B > src->ring.cap) return fail(AZ_ERR_STATE, "the source's batch of %lld samples was partly overwritten (capacity %lld)", B, (long long)src->ring.cap);
    HIPCHK(hipStreamSynchronize(src->stream));
    if (dst) HIPCHK(hipStreamSynchronize(dst->stream));
    return AZ_OK;
  }();
  const Verdict own(local);
  const auto t0 = std::chrono::steady_clock::now();
  const int W = c->world;
  const long long ng = local == AZ_OK ? num_games : 0;
  if (local != AZ_OK) B = 0;
  c->pack_ms = c->scatter_ms = 0.0;
  // 1. counts, status and geometry of every rank
  const long long hc[COMM_WORDS] = {ng, B, (long long)local, src ? ((long long)src->xs << 16) | (long long)src->nA : 0LL};
  std::vector<long long> all;
  AZCHK(exchange_words(c, hc, COMM_WORDS, &all));
  AZCHK(settle(own, all, COMM_WORDS, 2, [](int r, long long status) {
    return fail(AZ_ERR_COMM, "rank %d cannot take part in the plane gather (status %lld); nothing was exchanged", r, status);
  }));
  long long maxg = 1, maxB = 1, totg = 0;
  for (int r = 0; r < W; ++r) {
    const long long* w = &all[(size_t)COMM_WORDS * r];
    maxg = std::max(maxg, w[0]); maxB = std::max(maxB, w[1]); totg += w[0];
  }
  for (int r = 1; r < W; ++r)
    if (all[(size_t)COMM_WORDS * r + 3] != all[3]) return fail(AZ_ERR_BAD_ARG, "rank %d's plane geometry differs from rank 0's; nothing was exchanged", r);
  const int RW = src->RW, ND = src->ND;
  const long long rb = pg::record_bytes(RW, ND);
  long long R = pg::default_round_rows(W, rb);
  if (c->plane_round_rows > 0) R = std::min<long long>(R, c->plane_round_rows);
  R = (maxB + (maxB + R - 1) / R - 1) / ((maxB + R - 1) / R);         // the same number of rounds, evenly filled: the last one sends little padding
  // 2. buffers, sized by what all ranks hold together: a rank that cannot allocate them says so before anything is exchanged
  pg::Game *d_tsend = nullptr, *d_tall = nullptr;
  unsigned char *d_rsend = nullptr, *d_rall = nullptr;
  long long *d_plan = nullptr;
  const size_t n_prefix = (size_t)(totg + W), n_start = (size_t)std::max<long long>(totg, 1), n_src = (size_t)std::max<long long>(ng, 1);
  const size_t n_plan = n_prefix + n_start + (size_t)(W + 1) + (size_t)W + n_src;   // prefix_all, start_all, goff, B, src
  Scratch tmp;
  AZCHK(agree_allocated(c, [&]() -> int {
    AZCHK(tmp.alloc(&d_tsend, (size_t)maxg)); AZCHK(tmp.alloc(&d_tall, (size_t)maxg * W));
    AZCHK(tmp.alloc(&d_rsend, (size_t)(R * rb))); AZCHK(tmp.alloc(&d_rall, (size_t)(R * rb) * W));
    AZCHK(tmp.alloc(&d_plan, n_plan));
    return AZ_OK;
  }()));
  // 3. the game tables (8 B per game, padded to the largest rank), then the plan: the same on every rank
  std::vector<pg::Game> tsend((size_t)maxg, pg::Game{0, 0});
  for (long long k = 0; k < ng; ++k) tsend[(size_t)k] = pg::Game{game_ids[k], game_lens[k]};
  std::vector<pg::Game> tall((size_t)maxg * W);
  AZCHK(collective(c, [&]() -> int {
    HIPCHK(hipMemcpyAsync(d_tsend, tsend.data(), sizeof(pg::Game) * tsend.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_rsend, 0, (size_t)(R * rb), c->stream));   // what a rank with nothing left sends
    RCCLCHK(rc::g.AllGather(d_tsend, d_tall, (size_t)maxg, ncclInt64, c->comm, c->stream));
    HIPCHK(hipMemcpyAsync(tall.data(), d_tall, sizeof(pg::Game) * tall.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return AZ_OK;
  }));
  std::vector<std::vector<pg::Game>> tables((size_t)W);
  for (int r = 0; r < W; ++r) tables[(size_t)r].assign(tall.begin() + (size_t)r * maxg, tall.begin() + (size_t)r * maxg + (size_t)all[(size_t)COMM_WORDS * r]);
  const pg::Plan plan = pg::make_plan(tables, R, dst ? (long long)dst->ring.cap : 0);
  if (plan.dup) return fail(AZ_ERR_BAD_ARG, "game id %d occurs twice in the ranks' tables (ids are global and must be distinct); nothing was pushed", (int)plan.dup_id);
  std::vector<long long> hplan(n_plan, 0);
  long long *h_prefix = hplan.data(), *h_start = h_prefix + n_prefix, *h_goff = h_start + n_start, *h_B = h_goff + (W + 1), *h_src = h_B + W;
  long long g0 = 0;
  for (int r = 0; r < W; ++r) {
    const pg::RankPlan& rp = plan.ranks[(size_t)r];
    h_goff[r] = g0; h_B[r] = rp.B;
    std::copy(rp.prefix.begin(), rp.prefix.end(), h_prefix + g0 + r);
    std::copy(rp.start.begin(), rp.start.end(), h_start + g0);
    g0 += (long long)rp.start.size();
  }
  h_goff[W] = g0;
  const pg::RankPlan& mine = plan.ranks[(size_t)c->rank];
  std::copy(mine.src.begin(), mine.src.end(), h_src);
  const long long *d_prefix = d_plan, *d_start = d_prefix + n_prefix, *d_goff = d_start + n_start, *d_B = d_goff + (W + 1), *d_src = d_B + W;
  const long long* d_myprefix = d_prefix + h_goff[c->rank] + c->rank;
  // 4. rounds: pack -> all-gather -> scatter, R rows per rank; every rank runs plan.rounds of them
  const int vec = (RW % 4 == 0 && rb % 16 == 0) ? 4 : RW % 2 == 0 ? 2 : 1;
  const long long seq0 = src->ring.select(1).seq0;                     // last_batch: exactly the B samples, after the two checks above
  const auto rounds = [&]() -> int {
    HIPCHK(hipMemcpyAsync(d_plan, hplan.data(), sizeof(long long) * n_plan, hipMemcpyHostToDevice, c->stream));
    for (long long k = 0; k < plan.rounds; ++k) {
      const long long base = k * R, nrows = pg::round_rows_of(plan, c->rank, k);
      HIPCHK(hipEventRecord(c->ev[0], c->stream));
      if (nrows > 0) {
#define PG_PACK(V) hipLaunchKernelGGL(k_pg_pack<V>, dim3(pm_grid(nrows)), dim3(64 * PM_WAVES), 0, c->stream, src->d_XA, src->d_D, src->d_n, (long long)src->ring.cap, \
                                      seq0, base, nrows, d_myprefix, d_src, (int)ng, RW, ND, rb, d_rsend)
        if (vec == 4) PG_PACK(uint4); else if (vec == 2) PG_PACK(uint2); else PG_PACK(unsigned int);
#undef PG_PACK
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipEventRecord(c->ev[1], c->stream));
      RCCLCHK(rc::g.AllGather(d_rsend, d_rall, (size_t)(R * rb), ncclInt8, c->comm, c->stream));
      HIPCHK(hipEventRecord(c->ev[2], c->stream));
      if (dst && plan.T > plan.skip) {
#define PG_SCATTER(V) hipLaunchKernelGGL(k_pg_scatter<V>, dim3(pm_grid((long long)W * R)), dim3(64 * PM_WAVES), 0, c->stream, d_rall, R, base, W, d_B, d_goff, \
                                         d_prefix, d_start, plan.skip, (long long)dst->ring.total, (long long)dst->ring.cap, RW, ND, rb, dst->d_XA, dst->d_D, dst->d_n)
        if (vec == 4) PG_SCATTER(uint4); else if (vec == 2) PG_SCATTER(uint2); else PG_SCATTER(unsigned int);
#undef PG_SCATTER
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipEventRecord(c->ev[3], c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));                          // the events and the send buffer are the next round's too
      float pm = 0.f, sm = 0.f;
      HIPCHK(hipEventElapsedTime(&pm, c->ev[0], c->ev[1]));
      HIPCHK(hipEventElapsedTime(&sm, c->ev[2], c->ev[3]));
      c->pack_ms += pm; c->scatter_ms += sm;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return AZ_OK;
  };
  AZCHK(collective(c, rounds));
  if (dst) dst->ring.pushed(plan.T, true);                           // push_trace! of every game
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->games = totg; stats->moves = plan.T; stats->ranks = W;
    stats->bytes = (int64_t)W * (COMM_WORDS * 8 + maxg * (long long)sizeof(pg::Game) + plan.rounds * R * rb);
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->gather_ms = std::max(0.0, stats->total_ms - c->scatter_ms);  // everything but the push into the memory
  }
  return AZ_OK;
}
