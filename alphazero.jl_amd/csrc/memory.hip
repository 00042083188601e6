// memory.hip -- the replay memory and the learning-status evaluation on the device.
//
//   MemoryBuffer / push_trace! / get_experience / last_batch            src/memory.jl:20-87
//   augment_with_symmetries, merge_by_state                              src/memory.jl:89-138
//   convert_samples (W, X, A, P, V), Trainer's Wmean / Hp                src/learning.jl:17-51,98-121
//   losses, learning_status, mean_learning_status                        src/learning.jl:59-90,148-181
//
// Samples never leave HBM: the move records of a self-play phase go up once (64 B per position), the ring
// buffer, the symmetric images, the by-state merge (two stable radix sorts + one segment walk, so the averages
// are accumulated in buffer order like the reference's), the Float32 tensors and the loss terms are all device
// arrays.  The network forward of the loss is the same fused tower + heads as self-play (test mode).
// The loss's network forward goes through net_launch (engine.h).
#include "engine.h"
#include "prims.h"

// push_trace! (memory.jl:74-87): one thread per game walks its records from the last position to the first
template <class Gm>
__global__ void __launch_bounds__(256) k_mem_push(const az_move_rec* __restrict__ moves, const long long* __restrict__ first,
                                                  const int* __restrict__ nmoves, const long long* __restrict__ seq0, int ngames,
                                                  double gamma, az_sample* __restrict__ buf, long long cap, long long min_seq) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngames) return;
  const int n = nmoves[g];
  const az_move_rec* mv = moves + first[g];
  double wr = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    wr = gamma * wr + (double)mv[i].reward;
    const long long seq = seq0[g] + (n - 1 - i);
    if (seq < min_seq) continue;                                   // would be overwritten within this very call
    const GEnv env = Gm::from_key(mv[i].key[0], mv[i].key[1]);
    const uint32_t m = Gm::mask(env);
    az_sample e;
    e.key[0] = mv[i].key[0]; e.key[1] = mv[i].key[1];
    double ntot = 0.0, s = 0.0;
    for (int a = 0; a < Gm::A; ++a) if ((m >> a) & 1) ntot += (double)mv[i].N[a];
    for (int a = 0; a < AZ_MAX_ACTIONS; ++a) {
      const bool ok = a < Gm::A && ((m >> a) & 1);
      e.pi[a] = ok ? (double)mv[i].N[a] / ntot : 0.0;
      if (ok) s += e.pi[a];
    }
    for (int a = 0; a < Gm::A; ++a) if ((m >> a) & 1) e.pi[a] = e.pi[a] / s;
    e.z = Gm::white_playing(env) ? wr : -wr;
    e.t = (double)(n - i);
    e.n = 1;
    buf[seq % cap] = e;
  }
}
__global__ void k_mem_gather(const az_sample* __restrict__ buf, long long cap, long long seq0, long long n, az_sample* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = buf[(seq0 + i) % cap];
}
// augment_with_symmetries (memory.jl:116-138): image k of sample i lands at n + i*NSYM + k
template <class Gm>
__global__ void k_mem_augment(const az_sample* __restrict__ in, long long n, az_sample* __restrict__ out) {
  constexpr int NS = Gm::NSYM > 0 ? Gm::NSYM : 1;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * NS) return;
  const long long i = t / NS;
  const int k = (int)(t % NS);
  az_sample e = in[i];
  const GEnv s = Gm::sym(GEnv{e.key[0], e.key[1], 0}, k);
  az_sample o = e;
  o.key[0] = s.a; o.key[1] = s.b;
  for (int j = 0; j < Gm::A; ++j) o.pi[j] = e.pi[Gm::sym_action(k, j)];
  out[n + t] = o;
}
__global__ void k_mem_keys(const az_sample* __restrict__ s, long long n, unsigned long long* k0, unsigned long long* k1, unsigned int* idx) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  k0[i] = s[i].key[0]; k1[i] = s[i].key[1]; idx[i] = (unsigned int)i;
}
__global__ void k_mem_heads(const az_sample* __restrict__ s, const unsigned int* __restrict__ order, long long n, int* head) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool h = true;
  if (i > 0) {
    const az_sample &a = s[order[i]], &b = s[order[i - 1]];
    h = a.key[0] != b.key[0] || a.key[1] != b.key[1];
  }
  head[i] = h ? 1 : 0;
}
static constexpr long long MERGE_LONG = 256;
// merge_samples (memory.jl:89-96): 16 lanes per segment head, lane f owns the f-th 8-byte word of the sample
// (key, key, pi[0..8], z, t, n) and accumulates it over the segment in buffer order -- every field's sum is the
// reference's sequential one, the loads of a record coalesce over the lanes and pipeline over the (unrolled) loop.
__global__ void __launch_bounds__(256) k_mem_merge(const az_sample* __restrict__ s, const unsigned int* __restrict__ order,
                                                   const int* __restrict__ head, const int* __restrict__ segid, long long n,
                                                   az_sample* __restrict__ out, int* __restrict__ long_count,
                                                   long long* __restrict__ long_list) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i = gid >> 4;
  const int f = (int)(gid & 15);
  if (i >= n || !head[i] || f >= 14) return;
  const int sg = segid[i];
  long long lo = i + 1, hi = n;                                    // first position of the next segment
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (segid[mid] > sg) hi = mid; else lo = mid + 1; }
  const long long end = lo, cnt = end - i;
  if (cnt >= MERGE_LONG) {                                         // k_mem_merge_long takes the big segments
    if (f == 0) { const int k = atomicAdd(long_count, 1); long_list[2 * k] = i; long_list[2 * k + 1] = end; }
    return;
  }
  const unsigned long long* base = (const unsigned long long*)s;
  unsigned long long* o = (unsigned long long*)(out + (sg - 1));
  const unsigned long long w0 = base[(size_t)order[i] * 14 + f];
  if (f < 2) { o[f] = w0; return; }
  if (f == 13) {
    long long acc = (long long)w0;
#pragma unroll 8
    for (long long j = i + 1; j < end; ++j) acc += (long long)base[(size_t)order[j] * 14 + 13];
    o[13] = (unsigned long long)acc;
    return;
  }
  double acc = az_u2d(w0);
#pragma unroll 8
  for (long long j = i + 1; j < end; ++j) acc += az_u2d(base[(size_t)order[j] * 14 + f]);
  o[f] = az_d2u(acc / (double)cnt);
}
// Segments of MERGE_LONG or more samples (the opening positions: one sample per game): a workgroup of 14
// wavefronts per segment, wavefront f owns word f.  The 64 lanes load 64 consecutive samples at once (all the
// memory parallelism the serial walk lacks); the additions stay strictly in buffer order -- the reference's mean over a
// generator is a sequential fold (memory.jl:89-96), and a Float64 sum in another order is another number.
// (r4) The 64 loaded words go through LDS and every lane adds them in order from broadcast reads (independent, pipelined; the
// dependent chain is one v_add_f64 per sample).  Round 3 fetched lane k's word with two v_readlane per sample inside a
// predicated, fully unrolled loop: 1.5 ms for the 32 768-sample segment of the opening position (16 384 games x 2 images),
// a third of the whole data-set build of bench.py's memory block.
__global__ void __launch_bounds__(14 * 64) k_mem_merge_long(const az_sample* __restrict__ s, const unsigned int* __restrict__ order,
                                                            const int* __restrict__ segid, const int* __restrict__ long_count,
                                                            const long long* __restrict__ long_list, az_sample* __restrict__ out) {
  if ((int)blockIdx.x >= *long_count) return;
  __shared__ unsigned long long sh[14][64];
  const long long i = long_list[2 * blockIdx.x], end = long_list[2 * blockIdx.x + 1], cnt = end - i;
  const int f = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long* base = (const unsigned long long*)s;
  unsigned long long* o = (unsigned long long*)(out + (segid[i] - 1));
  double acc = 0.0;
  long long iacc = 0;
  unsigned long long wn = i + lane < end ? base[(size_t)order[i + lane] * 14 + f] : 0ULL;
  for (long long j0 = i; j0 < end; j0 += 64) {                       // uniform over the workgroup: every wavefront walks the same segment
    sh[f][lane] = wn;
    const long long jn = j0 + 64 + lane;                             // the next 64 samples travel while these are added
    wn = jn < end ? base[(size_t)order[jn] * 14 + f] : 0ULL;
    __syncthreads();
    const int m = (int)((end - j0) < 64 ? (end - j0) : 64);
    if (f >= 2 && f < 13) {
      int k = 0;
      if (j0 == i) { acc = az_u2d(sh[f][0]); k = 1; }                // the sum STARTS with the first sample (keeps -0.0)
      if (m == 64) {
#pragma unroll
        for (int q = 0; q < 64; ++q) if (q >= k) acc += az_u2d(sh[f][q]);
      } else for (; k < m; ++k) acc += az_u2d(sh[f][k]);
    } else if (f == 13) {
      for (int k = 0; k < m; ++k) iacc += (long long)sh[f][k];
    }
    __syncthreads();
  }
  if (lane == 0) {
    if (f < 2) o[f] = base[(size_t)order[i] * 14 + f];
    else o[f] = f == 13 ? (unsigned long long)iacc : az_d2u(acc / (double)cnt);
  }
}
// convert_samples (learning.jl:17-51) + per-sample entropy term of Hp (learning.jl:65,111)
template <class Gm>
__global__ void k_mem_convert(const az_sample* __restrict__ s, long long n, int policy, GEnv* envs, float* W, float* A, float* P, float* V,
                              double* t_w, double* t_hp, long long* t_n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const az_sample e = s[i];
  const GEnv env = Gm::from_key(e.key[0], e.key[1]);
  envs[i] = env;
  const float w = sample_weight(policy, (long long)e.n);
  W[i] = w;
  const uint32_t m = Gm::mask(env);
  double hp = 0.0;
  for (int a = 0; a < Gm::A; ++a) {
    const float p = (float)e.pi[a];
    A[i * Gm::A + a] = (float)((m >> a) & 1);
    P[i * Gm::A + a] = p;
    hp += (double)(p * az_logf(p + 1.1920929e-07f) * w);
  }
  V[i] = (float)e.z;
  t_w[i] = (double)w; t_hp[i] = hp; t_n[i] = (long long)e.n;
}
template <class Gm>
__global__ void k_mem_planes(const GEnv* __restrict__ envs, long long n, float* __restrict__ X) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int E = Gm::C * Gm::P;
  if (t >= n * E) return;
  const long long i = t / E;
  const int r = (int)(t % E);
  X[t] = Gm::plane(envs[i], r % Gm::P, r / Gm::P);
}
// per-sample terms of `losses` and of Hpnet (learning.jl:59-90,158-168), Float32 like the reference's arrays
__global__ void k_loss_terms(const float* __restrict__ W, const float* __restrict__ P, const float* __restrict__ V, const float* __restrict__ Ph,
                             const float* __restrict__ Vh, const float* __restrict__ Pinv, long long n, int A, float renorm,
                             double* t_kl, double* t_hn, double* t_mse, double* t_inv) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = W[i];
  double kl = 0.0, hn = 0.0;
  for (int a = 0; a < A; ++a) {
    const float ph = Ph[i * A + a];
    const float lg = az_logf(ph + 1.1920929e-07f);
    kl += (double)(P[i * A + a] * lg * w);
    hn += (double)(ph * lg * w);
  }
  const float d = Vh[i] / renorm - V[i] / renorm;
  t_kl[i] = kl; t_hn[i] = hn; t_mse[i] = (double)(d * d * w); t_inv[i] = (double)(Pinv[i] * w);
}

__global__ void k_f32_to_f64(const float* __restrict__ in, long long n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// Five sums per loss batch in one launch: block b reduces samples [b*batch, min(n, (b+1)*batch)) of the five term
// arrays with a fixed-shape tree (thread-strided partial sums, then shared-memory halving), so the result does not
// depend on scheduling.  out[b][0..5) = sum w, kl, hn, mse, inv.
__global__ void __launch_bounds__(256) k_batch_sums(const double* __restrict__ tw, const double* __restrict__ tkl, const double* __restrict__ thn,
                                                    const double* __restrict__ tmse, const double* __restrict__ tinv, long long n, long long batch,
                                                    double* __restrict__ out) {
  __shared__ double sh[5][256];
  const long long b0 = (long long)blockIdx.x * batch;
  const long long m = (n - b0) < batch ? (n - b0) : batch;
  const double* src[5] = {tw, tkl, thn, tmse, tinv};
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < m; i += 256)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[k] += src[k][b0 + i];
#pragma unroll
  for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 5) out[(size_t)blockIdx.x * 5 + threadIdx.x] = sh[threadIdx.x][0];
}

// the sum of sum(e.n) (DevReducer, prims.h), instantiated ahead of the per-game templates: the unit's kernels keep the order its code object had
template int DevReducer::sum<long long>(const long long*, long long, hipStream_t, long long*);

#define MEMORY(m) if (!(m)) return fail(AZ_ERR_BAD_ARG, "memory is NULL"); HIPCHK(hipSetDevice((m)->device))

extern "C" int az_memory_create(int32_t game, int32_t device, int64_t capacity, az_memory** out) {
  if (!out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  GameInfo gi;
  if (!game_info(game, &gi)) return fail(AZ_ERR_BAD_ARG, "unknown game id %d", game);
  if (game == AZ_GAME_GO9_PLANES) return fail(AZ_ERR_BAD_ARG, "game id %d is a network-only tensor geometry (no device twin): the device replay memory needs the game's state keys; az_dataset_create_from_tensors takes the converted samples of such a game", game);
  if (capacity < 1 || capacity > (1LL << 31) - 1) return fail(AZ_ERR_BAD_ARG, "capacity must be in 1..2^31-1");
  AZCHK(use_device(device));
  az_memory* m = new (std::nothrow) az_memory();
  if (!m) return fail(AZ_ERR_HIP, "out of host memory");
  m->game = game; m->device = device; m->gi = gi; m->ring.cap = capacity;
  int st = [&]() -> int {
    HIPCHK(hipStreamCreate(&m->stream));
    AZCHK(mem_alloc<az_sample>(nullptr, &m->d_buf, (size_t)capacity));
    return AZ_OK;
  }();
  if (st != AZ_OK) { az_memory_destroy(m); return st; }
  *out = m;
  return AZ_OK;
}
extern "C" int az_memory_destroy(az_memory* m) {
  if (!m) return AZ_OK;
  (void)hipSetDevice(m->device);
  if (m->d_buf) (void)hipFree(m->d_buf);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return AZ_OK;
}
int memory_push_device(az_memory* m, const az_move_rec* d_moves, const std::vector<long long>& first, const std::vector<int>& cnt, double gamma) {
  const int ng = (int)first.size();
  if (!ng) return AZ_OK;
  std::vector<long long> seq0(ng);
  long long tot = 0;
  for (int g = 0; g < ng; ++g) { seq0[g] = m->ring.total + tot; tot += cnt[g]; }
  long long *d_first, *d_seq; int* d_cnt;
  Scratch tmp;
  AZCHK(tmp.alloc(&d_first, ng)); AZCHK(tmp.alloc(&d_cnt, ng)); AZCHK(tmp.alloc(&d_seq, ng));
  HIPCHK(hipMemcpyAsync(d_first, first.data(), sizeof(long long) * ng, hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipMemcpyAsync(d_cnt, cnt.data(), sizeof(int) * ng, hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipMemcpyAsync(d_seq, seq0.data(), sizeof(long long) * ng, hipMemcpyHostToDevice, m->stream));
  DISPATCH_GAME(m->game, hipLaunchKernelGGL((k_mem_push<Gm>), dim3((ng + 255) / 256), dim3(256), 0, m->stream, d_moves, d_first, d_cnt, d_seq, ng, gamma, m->d_buf, (long long)m->ring.cap, (long long)m->ring.min_seq(tot)));
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(hipGetLastError());
  m->ring.pushed(tot, true);
  return AZ_OK;
}
extern "C" int az_memory_push(az_memory* m, const az_trace_buf* tr, double gamma) {
  MEMORY(m);
  if (!tr || tr->num_games < 0 || (tr->num_games > 0 && (!tr->games || !tr->moves))) return fail(AZ_ERR_BAD_ARG, "NULL trace buffers");
  const int ng = (int)tr->num_games;
  if (!ng) return AZ_OK;
  std::vector<long long> first(ng);
  std::vector<int> cnt(ng);
  for (int g = 0; g < ng; ++g) {
    const az_game_rec& r = tr->games[g];
    if (r.num_moves < 0 || r.first_move < 0 || (int64_t)r.first_move + r.num_moves > tr->num_moves) return fail(AZ_ERR_BAD_ARG, "game record %d points outside the move records", g);
    first[g] = r.first_move; cnt[g] = r.num_moves;
  }
  az_move_rec* d_moves = nullptr;
  Scratch tmp;
  AZCHK(tmp.alloc(&d_moves, (size_t)tr->num_moves));
  HIPCHK(hipMemcpyAsync(d_moves, tr->moves, sizeof(az_move_rec) * (size_t)tr->num_moves, hipMemcpyHostToDevice, m->stream));
  return memory_push_device(m, d_moves, first, cnt, gamma);
}
// push_trace! for every game of the engine's last self-play phase, in game-id order, straight from the engine's
// device-resident move records (src/training.jl:284-299 -> src/memory.jl:74-87 without the 64 B per position ever
// visiting the host)
extern "C" int az_memory_push_engine(az_memory* m, az_engine* e, double gamma) {
  MEMORY(m);
  if (!e) return fail(AZ_ERR_BAD_ARG, "engine is NULL");
  if (e->ph.running) return fail(AZ_ERR_STATE, "self-play in progress");
  if (e->cfg.game != m->game || e->device != m->device) return fail(AZ_ERR_BAD_ARG, "memory and engine differ in game or device");
  if (!e->d_phase) return fail(AZ_ERR_STATE, "the engine holds no device-resident phase (az_selfplay_run / az_selfplay_begin with num_games > 0 first)");
  std::vector<long long> first;
  std::vector<int> cnt;
  phase_games_by_id(e, &first, &cnt);
  AZCHK(sync_all(e));
  return memory_push_device(m, e->d_phase, first, cnt, gamma);
}
// push!(mem.buf, sample) for host-resident TrainingSamples (a reference-side MemoryBuffer, or subsets such as the game
// stages of memory_report, src/learning.jl:192-216)
extern "C" int az_memory_push_samples(az_memory* m, const az_sample* samples, int64_t n) {
  MEMORY(m);
  if (n < 0 || (n > 0 && !samples)) return fail(AZ_ERR_BAD_ARG, "NULL samples");
  // keep only what survives in the ring, oldest first
  const int64_t skip = m->ring.skip(n);
  const az_sample* src = samples + skip;
  for (const Ring::Run& r : m->ring.runs(m->ring.total + skip, n - skip)) {
    HIPCHK(hipMemcpyAsync(m->d_buf + r.pos, src, sizeof(az_sample) * (size_t)r.run, hipMemcpyHostToDevice, m->stream));
    src += r.run;
  }
  HIPCHK(hipStreamSynchronize(m->stream));
  m->ring.pushed(n, false);
  return AZ_OK;
}

extern "C" int az_memory_length(az_memory* m, int64_t* length, int64_t* cur_batch_size) {
  MEMORY(m);
  if (length) *length = m->ring.len();
  if (cur_batch_size) *cur_batch_size = m->ring.batch();
  return AZ_OK;
}
extern "C" int az_memory_new_batch(az_memory* m) { MEMORY(m); m->ring.new_batch(); return AZ_OK; }
extern "C" int az_memory_empty(az_memory* m) { MEMORY(m); m->ring.empty(); return AZ_OK; }

template <class Gm>
static int dataset_build(az_memory* m, az_dataset* d, int which, bool use_sym, bool merge, int policy) {
  hipStream_t st = m->stream;
  const Ring::Selection sel = m->ring.select(which);               // may be empty: the data set then has n = 0
  const int64_t n0 = sel.n0;
  const int nsym = use_sym ? Gm::NSYM : 0;
  const int64_t n1 = n0 * (1 + nsym);
  if (n1 > (1LL << 31) - 1) return fail(AZ_ERR_CAPACITY, "data set too large");
  Scratch tmp;
  az_sample* s1;
  AZCHK(tmp.alloc(&s1, (size_t)n1));
  if (n0) hipLaunchKernelGGL(k_mem_gather, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, m->d_buf, (long long)m->ring.cap, (long long)sel.seq0, (long long)n0, s1);
  if (nsym && n0) hipLaunchKernelGGL((k_mem_augment<Gm>), dim3((unsigned)((n0 * nsym + 255) / 256)), dim3(256), 0, st, s1, (long long)n0, s1);
  int64_t n2 = n1;
  if (merge && n1 > 0) {
    const unsigned gb = (unsigned)((n1 + 255) / 256);
    Grouping g;
    AZCHK(group_by_key(tmp, n1, st,
                       [&](unsigned long long* k0, unsigned long long* k1, unsigned int* idx) { hipLaunchKernelGGL(k_mem_keys, dim3(gb), dim3(256), 0, st, s1, (long long)n1, k0, k1, idx); },
                       [&](const unsigned long long*, const unsigned int* order, int* head) { hipLaunchKernelGGL(k_mem_heads, dim3(gb), dim3(256), 0, st, s1, order, (long long)n1, head); },
                       &g));
    int nseg = 0;
    HIPCHK(hipMemcpyAsync(&nseg, g.seg + (n1 - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    n2 = nseg;
    AZCHK(mem_alloc(&d->allocs, &d->d_samples, (size_t)n2));
    static_assert(sizeof(az_sample) == 14 * 8, "k_mem_merge walks az_sample as 14 words");
    int* long_count; long long* long_list;
    const long long max_long = n1 / MERGE_LONG + 1;
    AZCHK(tmp.alloc(&long_count, 1)); AZCHK(tmp.alloc(&long_list, (size_t)(2 * max_long)));
    HIPCHK(hipMemsetAsync(long_count, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_mem_merge, dim3((unsigned)((n1 * 16 + 255) / 256)), dim3(256), 0, st, s1, g.order, g.head, g.seg, (long long)n1, d->d_samples, long_count, long_list);
    hipLaunchKernelGGL(k_mem_merge_long, dim3((unsigned)max_long), dim3(14 * 64), 0, st, s1, g.order, g.seg, long_count, long_list, d->d_samples);
  } else {
    AZCHK(mem_alloc(&d->allocs, &d->d_samples, (size_t)n2));
    if (n2) HIPCHK(hipMemcpyAsync(d->d_samples, s1, sizeof(az_sample) * (size_t)n2, hipMemcpyDeviceToDevice, st));
  }
  d->n = n2;
  AZCHK(mem_alloc(&d->allocs, &d->d_envs, (size_t)n2));
  AZCHK(dataset_alloc_tensors(d, n2));
  if (n2) {
    double *tw, *thp; long long* tn;
    AZCHK(tmp.alloc(&tw, (size_t)n2)); AZCHK(tmp.alloc(&thp, (size_t)n2)); AZCHK(tmp.alloc(&tn, (size_t)n2));
    hipLaunchKernelGGL((k_mem_convert<Gm>), dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, d->d_samples, (long long)n2, policy, d->d_envs, d->d_W, d->d_A, d->d_P, d->d_V, tw, thp, tn);
    const long long ne = (long long)n2 * Gm::C * Gm::P;
    hipLaunchKernelGGL((k_mem_planes<Gm>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, d->d_envs, (long long)n2, d->d_X);
    DevReducer red;
    AZCHK(red.init(n2));
    double sw, shp; long long sn;
    AZCHK(red.sum(tw, n2, st, &sw)); AZCHK(red.sum(thp, n2, st, &shp)); AZCHK(red.sum(tn, n2, st, &sn));
    d->Wtot = sw; d->sum_n = (int64_t)sn;
    d->Wmean = (float)(sw / (double)n2);                         // mean(W), learning.jl:110
    d->Hp = (float)(-shp / sw);                                  // entropy_wmean(P, W), learning.jl:111
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return AZ_OK;
}

extern "C" int az_dataset_destroy(az_dataset* d) {
  if (!d) return AZ_OK;
  (void)hipSetDevice(d->device);
  for (void* p : d->allocs) (void)hipFree(p);
  if (d->own_stream && d->stream) (void)hipStreamDestroy(d->stream);
  delete d;
  return AZ_OK;
}
extern "C" int az_dataset_create(az_memory* m, int32_t which, int32_t use_symmetries, int32_t use_position_averaging,
                                 int32_t weighing_policy, az_dataset** out) {
  MEMORY(m);
  if (!out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  AZCHK(dataset_check_args(which, weighing_policy));
  if (m->game == AZ_GAME_GO9_PLANES) return fail(AZ_ERR_BAD_ARG, "game id %d has no device twin", m->game);   // the one known id DISPATCH_GAME has no case for
  return dataset_create(m->game, m->device, m->gi, m->stream, out, [&](az_dataset* d) -> int {   // the data set works on the memory's stream
    int st = AZ_OK;
    DISPATCH_GAME(m->game, st = dataset_build<Gm>(m, d, which, use_symmetries != 0, use_position_averaging != 0, weighing_policy));
    return st;
  });
}
// A data set made from the (W, X, A, P, V) tensors of convert_samples (learning.jl:17-51) that a host computed itself: one thread
// per sample checks what the loss relies on and leaves the sample's terms of Wtot and of Hp = entropy_wmean(P, W) (learning.jl:63,111).
// What fails raises its SampleFault clause (engine.h); the checker's own clause is W <= 0.
__global__ void __launch_bounds__(256) k_ds_check(const float* __restrict__ W, const float* __restrict__ X, const float* __restrict__ A, const float* __restrict__ P,
                                                  const float* __restrict__ V, long long n, int xs, int nA, unsigned long long* __restrict__ bad,
                                                  double* __restrict__ t_w, double* __restrict__ t_hp) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = W[i];
  bool finite = isfinite(w) && isfinite(V[i]);
  for (int k = 0; k < xs; ++k) finite = finite && isfinite(X[(size_t)i * xs + k]);
  bool a01 = true, pneg = false, pill = false;
  int legal = 0;
  double hp = 0.0;
  for (int a = 0; a < nA; ++a) {
    const float m = A[(size_t)i * nA + a], p = P[(size_t)i * nA + a];
    finite = finite && isfinite(m) && isfinite(p);
    a01 = a01 && (m == 0.0f || m == 1.0f);
    legal += m == 1.0f;
    pneg = pneg || p < 0.0f;
    pill = pill || (p > 0.0f && m == 0.0f);
    hp += (double)(p * az_logf(p + 1.1920929e-07f) * w);             // the term k_mem_convert leaves for a memory-made data set
  }
  const int code = !finite ? SF_NONFINITE : !(w > 0.0f) ? SF_OWN : !a01 ? SF_A01 : legal == 0 ? SF_NOLEGAL : pneg ? SF_PNEG : pill ? SF_PILLEGAL : 0;
  if (code) sample_fault_raise(bad, i, code);
  t_w[i] = (double)w; t_hp[i] = code ? 0.0 : hp;
}
int dataset_tensor_stats(az_dataset* d, hipStream_t st) {
  const int64_t n = d->n;
  const size_t xs = (size_t)d->gi.C * d->gi.P, nA = (size_t)d->gi.A, N = (size_t)n;
  Scratch tmp;
  unsigned long long* d_bad; double *tw, *thp;
  AZCHK(tmp.alloc(&d_bad, 1)); AZCHK(tmp.alloc(&tw, N)); AZCHK(tmp.alloc(&thp, N));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_ds_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d->d_W, d->d_X, d->d_A, d->d_P, d->d_V, (long long)n, (int)xs, (int)nA, d_bad, tw, thp);
  unsigned long long bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  AZCHK(sample_fault_status(bad, "W <= 0"));
  DevReducer red;                                                    // the reducer of dataset_build: the same tiles and tree for the same n
  AZCHK(red.init(n));
  double sw, shp;
  AZCHK(red.sum(tw, n, st, &sw)); AZCHK(red.sum(thp, n, st, &shp));
  d->Wtot = sw;
  d->Wmean = (float)(sw / (double)n);                                // mean(W), learning.jl:110
  d->Hp = (float)(-shp / sw);                                        // entropy_wmean(P, W), learning.jl:111
  return AZ_OK;
}
extern "C" int az_dataset_create_from_tensors(int32_t game, int32_t device, int64_t n, const float* W, const float* X, const float* A,
                                              const float* P, const float* V, az_dataset** out) {
  if (!out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  GameInfo gi;
  if (!game_info(game, &gi)) return fail(AZ_ERR_BAD_ARG, "unknown game id %d", game);
  if (n < 1 || n > (1LL << 31) - 1) return fail(AZ_ERR_BAD_ARG, "n must be in 1..2^31-1");
  if (!W || !X || !A || !P || !V) return fail(AZ_ERR_BAD_ARG, "NULL tensor");
  AZCHK(use_device(device));
  return dataset_create(game, device, gi, nullptr, out, [&](az_dataset* d) -> int {
    d->n = n; d->sum_n = n;
    HIPCHK(hipStreamCreate(&d->stream));
    hipStream_t st = d->stream;
    const size_t xs = (size_t)gi.C * gi.P, nA = (size_t)gi.A, N = (size_t)n;
    AZCHK(dataset_alloc_tensors(d, n));
    HIPCHK(hipMemcpyAsync(d->d_W, W, sizeof(float) * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_V, V, sizeof(float) * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_A, A, sizeof(float) * N * nA, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_P, P, sizeof(float) * N * nA, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_X, X, sizeof(float) * N * xs, hipMemcpyHostToDevice, st));
    return dataset_tensor_stats(d, st);
  });
}
extern "C" int az_dataset_get_info(az_dataset* d, az_dataset_info* out) {
  if (!d || !out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  out->num_samples = d->n; out->sum_n = d->sum_n; out->Wtot = d->Wtot; out->Wmean = d->Wmean; out->Hp = d->Hp;
  return AZ_OK;
}
extern "C" int az_dataset_read(az_dataset* d, int64_t first, int64_t count, az_sample* samples, float* W, float* X, float* A,
                               float* P, float* V) {
  if (!d) return fail(AZ_ERR_BAD_ARG, "dataset is NULL");
  HIPCHK(hipSetDevice(d->device));
  if (first < 0 || count < 0 || first + count > d->n) return fail(AZ_ERR_BAD_ARG, "range [%lld, %lld) outside the %lld samples", (long long)first, (long long)(first + count), (long long)d->n);
  if (samples && !d->d_samples) return fail(AZ_ERR_BAD_ARG, "a data set made from tensors holds no az_sample records: read W, X, A, P, V");
  if (!count) return AZ_OK;
  const GameInfo& gi = d->gi;
  const size_t xs = (size_t)gi.C * gi.P;
  if (samples) HIPCHK(hipMemcpyAsync(samples, d->d_samples + first, sizeof(az_sample) * (size_t)count, hipMemcpyDeviceToHost, d->stream));
  if (W) HIPCHK(hipMemcpyAsync(W, d->d_W + first, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, d->stream));
  if (V) HIPCHK(hipMemcpyAsync(V, d->d_V + first, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, d->stream));
  if (A) HIPCHK(hipMemcpyAsync(A, d->d_A + (size_t)first * gi.A, sizeof(float) * (size_t)count * gi.A, hipMemcpyDeviceToHost, d->stream));
  if (P) HIPCHK(hipMemcpyAsync(P, d->d_P + (size_t)first * gi.A, sizeof(float) * (size_t)count * gi.A, hipMemcpyDeviceToHost, d->stream));
  if (X) HIPCHK(hipMemcpyAsync(X, d->d_X + (size_t)first * xs, sizeof(float) * (size_t)count * xs, hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return AZ_OK;
}

// Sum of squares of the trainable parameters (Flux.params: all but the BatchNorm running statistics), host side: one accumulator
// over the blob in ascending order
static double reg_sum_trainable(const az_engine* e) {
  const std::vector<unsigned char>& trainable = e->trainable;
  double s = 0.0;
  for (size_t i = 0; i < trainable.size(); ++i) if (trainable[i]) s += (double)e->blob[i] * (double)e->blob[i];
  return s;
}

// Reads the data set's tensors only (the network launch dispatches on the engine's geometry, net.hip), so it serves all four
// network geometries: a memory-made data set hands the tower its device-twin states, one made from tensors its planes and masks.
static int learning_status_run(az_engine* e, az_dataset* d, double l2, double cinv, double renorm, int64_t batch, az_learning_status_t* out) {
  const int64_t n = d->n;
  const int nA = d->gi.A;
  const size_t xs = (size_t)d->gi.C * d->gi.P;
  hipStream_t st = e->stream;
  Scratch tmp;
  float *Ph, *Vh, *Pinv; double *tkl, *thn, *tmse, *tinv, *tw;
  AZCHK(tmp.alloc(&Ph, (size_t)n * nA)); AZCHK(tmp.alloc(&Vh, (size_t)n)); AZCHK(tmp.alloc(&Pinv, (size_t)n));
  AZCHK(tmp.alloc(&tkl, (size_t)n)); AZCHK(tmp.alloc(&thn, (size_t)n)); AZCHK(tmp.alloc(&tmse, (size_t)n)); AZCHK(tmp.alloc(&tinv, (size_t)n));
  AZCHK(tmp.alloc(&tw, (size_t)n));
  HIPCHK(hipStreamSynchronize(d->stream));
  // Network.forward_normalized (network.jl:264-271) in test mode on the device-resident states, nn_cap at a time
  const int64_t nchunks = (n + e->nn_cap - 1) / e->nn_cap;
  std::vector<int> counts((size_t)nchunks);
  for (int64_t c = 0; c < nchunks; ++c) counts[c] = (int)std::min<int64_t>(e->nn_cap, n - c * e->nn_cap);
  int* d_counts;
  AZCHK(tmp.alloc(&d_counts, (size_t)nchunks));
  HIPCHK(hipMemcpyAsync(d_counts, counts.data(), sizeof(int) * (size_t)nchunks, hipMemcpyHostToDevice, st));
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t off = c * e->nn_cap;
    if (d->d_envs) AZCHK(net_launch(e, st, false, e->d_hfeat, d->d_envs + off, e->d_iota, d_counts + c, counts[c], nullptr, nullptr, Ph + (size_t)off * nA, Vh + off, Pinv + off, nA));
    else AZCHK(net_launch(e, st, true, e->d_hfeat, nullptr, nullptr, nullptr, counts[c], d->d_X + (size_t)off * xs, d->d_A + (size_t)off * nA, Ph + (size_t)off * nA, Vh + off, Pinv + off, nA));
  }
  HIPCHK(hipStreamSynchronize(st));                              // `counts` must outlive the copy
  hipLaunchKernelGGL(k_loss_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d->d_W, d->d_P, d->d_V, Ph, Vh, Pinv, (long long)n, nA, (float)renorm, tkl, thn, tmse, tinv);
  hipLaunchKernelGGL(k_f32_to_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d->d_W, (long long)n, tw);
  if (batch > n) batch = n;
  const int64_t nb = (n + batch - 1) / batch;                    // DataLoader(partial = true), learning.jl:171-176
  double* d_sums;
  AZCHK(tmp.alloc(&d_sums, (size_t)nb * 5));
  hipLaunchKernelGGL(k_batch_sums, dim3((unsigned)nb), dim3(256), 0, st, tw, tkl, thn, tmse, tinv, (long long)n, (long long)batch, d_sums);
  std::vector<double> sums((size_t)nb * 5);
  HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const float Lreg = l2 == 0.0 ? 0.f : (float)((double)(float)l2 * reg_sum_trainable(e));
  double aL = 0., aLp = 0., aLv = 0., aLreg = 0., aLinv = 0., aHn = 0., aw = 0.;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t m = std::min<int64_t>(batch, n - b * batch);
    const double bw = sums[b * 5], kl = sums[b * 5 + 1], hn = sums[b * 5 + 2], mse = sums[b * 5 + 3], inv = sums[b * 5 + 4];
    const float Lp = (float)(-kl / bw) - d->Hp;
    const float Lv = (float)(mse / bw);
    const float Linv = cinv == 0.0 ? 0.f : (float)cinv * (float)(inv / bw);
    const float L = ((float)(bw / (double)m) / d->Wmean) * (Lp + Lv + Lreg + Linv);
    const float Hn = (float)(-hn / bw);
    aL += (double)L * bw; aLp += (double)Lp * bw; aLv += (double)Lv * bw; aLreg += (double)Lreg * bw;
    aLinv += (double)Linv * bw; aHn += (double)Hn * bw; aw += bw;
  }
  out->L = (float)(aL / aw); out->Lp = (float)(aLp / aw); out->Lv = (float)(aLv / aw); out->Lreg = (float)(aLreg / aw);
  out->Linv = (float)(aLinv / aw); out->Hp = d->Hp; out->Hpnet = (float)(aHn / aw);
  HIPCHK(hipGetLastError());
  return AZ_OK;
}

extern "C" int az_learning_status(az_engine* e, az_dataset* d, double l2_regularization, double nonvalidity_penalty,
                                  double rewards_renormalization, int64_t loss_computation_batch_size, az_learning_status_t* out) {
  ENGINE(e);
  if (!d || !out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  if (e->ph.running) return fail(AZ_ERR_STATE, "self-play in progress");
  if (!oracle_is_net(e->cfg) || !e->net_loaded) return fail(AZ_ERR_STATE, "az_net_set_params has not been called");
  if (d->game != e->cfg.game || d->device != e->device) return fail(AZ_ERR_BAD_ARG, "data set and engine differ in game or device");
  if (d->n < 1) return fail(AZ_ERR_BAD_ARG, "empty data set");
  if (loss_computation_batch_size < 1) return fail(AZ_ERR_BAD_ARG, "loss_computation_batch_size must be >= 1");
  if (!(rewards_renormalization > 0.0)) return fail(AZ_ERR_BAD_ARG, "rewards_renormalization must be > 0");
  AZCHK(sync_all(e));
  return learning_status_run(e, d, l2_regularization, nonvalidity_penalty, rewards_renormalization, loss_computation_batch_size, out);
}
