// plane_memory.hip -- the replay memory of a host-stepped game (include/azhip.h "replay memory of plane samples").
//
//   MemoryBuffer / push_trace! / get_experience / last_batch            src/memory.jl:20-87
//   merge_by_state                                                       src/memory.jl:89-112
//   convert_samples (W, X, A, P, V)                                      src/learning.jl:17-51
//
// memory.hip stores 128-bit state keys and re-encodes them with the game's device twin.  A game whose rules live on the host has
// no twin, so this memory stores what the host can give: the planes X and the mask A the network sees, pi by full action index,
// z, t and n.  Two samples are one state when their (X, A) rows are bit-identical.  The data-set build never leaves HBM:
//   k_pm_hash    one wavefront per sample mixes the row's words into a 128-bit key (fixed shuffle tree, no atomics)
//   sort_pairs   twice (prims.h, stable): ascending (key, buffer index), so a group keeps buffer order
//   k_pm_heads   one wavefront per adjacent pair compares the FULL rows: the hash only brings equal rows together, it never
//                decides that two rows are equal.  Equal keys over different rows raise the error word
//   k_pm_groups  + scan + a third sort_pairs on each group's first buffer index: output rows in order of first occurrence
//   k_pm_merge   one wavefront per output row walks its members in buffer order (Float64, sequential, then one division, the
//                order k_mem_merge documents) and writes W, X, A, P, V; without merging the same kernel runs on groups of one
// The result is an az_dataset like az_dataset_create_from_tensors's, checked and summed by the same code (dataset_tensor_stats).
//
//   augment_with_symmetries                                              src/memory.jl:114-130
// The host declares GI.symmetries once as gather permutations (az_plane_memory_set_symmetries).  A build with use_symmetries runs the
// same pipeline over [samples ; images]; an image is never written anywhere: k_pm_hash, k_pm_heads and k_pm_merge read "word w of
// virtual row r" (pm_row / pm_word below), and their instantiation without symmetries is the build as it was.
#include "engine.h"
#include "prims.h"

#define PLANE_MEMORY(m) if (!(m)) return fail(AZ_ERR_BAD_ARG, "plane memory is NULL"); HIPCHK(hipSetDevice((m)->device))

// ---- push: check the staged samples, then store them into the ring ----------------------------------------------------------------
// One wavefront per sample, lanes over the words.  What fails raises its SampleFault clause (engine.h); the checker's own clause is n < 1.
__global__ void __launch_bounds__(64 * PM_WAVES) k_pm_check(const float* __restrict__ X, const float* __restrict__ A, const double* __restrict__ P,
                                                            const double* __restrict__ z, const double* __restrict__ t, const long long* __restrict__ nv,
                                                            long long n, int xs, int nA, unsigned long long* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  bool finite = true, a01 = true, pneg = false, pill = false, legal = false;
  for (int w = lane; w < xs; w += 64) finite = finite && isfinite(X[(size_t)i * xs + w]);
  for (int a = lane; a < nA; a += 64) {
    const float m = A[(size_t)i * nA + a];
    const double p = P[(size_t)i * nA + a];
    finite = finite && isfinite(m) && isfinite((float)p);            // the data set holds Float32(pi)
    a01 = a01 && (m == 0.0f || m == 1.0f);
    legal = legal || m == 1.0f;
    pneg = pneg || p < 0.0;
    pill = pill || (p > 0.0 && m == 0.0f);
  }
  if (lane == 0) finite = finite && isfinite(z[i]) && isfinite(t[i]);
  const bool nbad = nv && nv[i] < 1;
  const int code = __ballot(!finite) ? SF_NONFINITE : nbad ? SF_OWN : __ballot(!a01) ? SF_A01 : !__ballot(legal) ? SF_NOLEGAL
                   : __ballot(pneg) ? SF_PNEG : __ballot(pill) ? SF_PILLEGAL : 0;
  if (code && lane == 0) sample_fault_raise(bad, i, code);
}
// pushed sample j (j >= skip: the others would be overwritten within this very call) is staged sample (reverse ? n - 1 - j : j)
// and lands in slot (total + j) % cap
__global__ void __launch_bounds__(64 * PM_WAVES) k_pm_store(const float* __restrict__ X, const float* __restrict__ A, const double* __restrict__ P,
                                                            const double* __restrict__ z, const double* __restrict__ t, const long long* __restrict__ nv,
                                                            long long n, long long skip, int reverse, int xs, int nA, long long total, long long cap,
                                                            float* __restrict__ XA, double* __restrict__ D, long long* __restrict__ N) {
  const int lane = threadIdx.x & 63;
  const long long j = skip + (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (j >= n) return;
  const size_t src = (size_t)(reverse ? n - 1 - j : j), slot = (size_t)((total + j) % cap);
  const int RW = xs + nA, ND = nA + 2;
  for (int w = lane; w < xs; w += 64) XA[slot * RW + w] = X[src * xs + w];
  for (int a = lane; a < nA; a += 64) {
    XA[slot * RW + xs + a] = A[src * nA + a];
    D[slot * ND + a] = P[src * nA + a];
  }
  if (lane == 0) { D[slot * ND + nA] = z[src]; D[slot * ND + nA + 1] = t[src]; N[slot] = nv ? nv[src] : 1LL; }
}

// ---- merge_by_state over rows --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long pm_fmix(unsigned long long h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdULL; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ULL; h ^= h >> 33;
  return h;
}
// ---- virtual rows: augment_with_symmetries (memory.jl:114-130) without storing an image ---------------------------------------------
// What a build reads.  Buffer index r < n0 is sample (seq0 + r) of the ring.  With symmetries declared and asked for, r >= n0 is image
// k = (r - n0) % nsym of sample i = (r - n0) / nsym (the order of k_mem_augment): the same ring row read through perm[k], word w of the
// image being word perm[k][w] of the sample.  n0 * (1 + nsym) < 2^31, so the image's number divides in 32 bits.
struct PmView {
  const float* XA;
  long long cap, seq0, n0;
  int RW, nsym;
  const unsigned short* perm;                                        // [nsym][RW]
};
struct PmRow {
  const unsigned int* words;                                         // the ring row's RW words
  const unsigned short* perm;                                        // NULL: the sample itself
  size_t slot;
};
template <bool SYM> __device__ __forceinline__ PmRow pm_row(const PmView& v, long long r) {
  long long i = r;
  const unsigned short* perm = nullptr;
  if (SYM && r >= v.n0) {
    const unsigned int q = (unsigned int)(r - v.n0), ns = (unsigned int)v.nsym;
    i = (long long)(q / ns);
    perm = v.perm + (size_t)(q % ns) * v.RW;
  }
  const size_t slot = (size_t)((v.seq0 + i) % v.cap);
  return PmRow{(const unsigned int*)v.XA + slot * v.RW, perm, slot};
}
// word w of virtual row `row`
template <bool SYM> __device__ __forceinline__ unsigned int pm_word(const PmRow& row, int w) {
  if (SYM && row.perm) return row.words[row.perm[w]];
  return row.words[w];
}
// where double j of the virtual row's ND = nA + 2 lies in the ring's: pi'[j] = pi[aperm[j]]; z and t are the sample's
template <bool SYM> __device__ __forceinline__ int pm_dcol(const PmRow& row, int xs, int nA, int j) {
  if (SYM && row.perm && j < nA) return (int)row.perm[xs + j] - xs;
  return j;
}

// Row hash: lane l mixes words l, l + 64, ... (each with its position) into two 64-bit halves; a fixed shuffle tree folds the 64
// lanes into lane 0 (the fold is not commutative, the tree has one shape: the key depends on the row alone).  bits < 128 truncates
// the key (az_debug_plane_memory_hash_bits).  SYM = false is the build without symmetries: no table is touched.
template <bool SYM>
__global__ void __launch_bounds__(64 * PM_WAVES) k_pm_hash(PmView v, long long n, int bits,
                                                           unsigned long long* __restrict__ k0, unsigned long long* __restrict__ k1,
                                                           unsigned long long* __restrict__ k1_keep, unsigned int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (r >= n) return;
  const PmRow row = pm_row<SYM>(v, r);
  const int RW = v.RW;
  unsigned long long a = 0x9e3779b97f4a7c15ULL + (unsigned long long)lane, b = 0xc2b2ae3d27d4eb4fULL ^ (unsigned long long)lane;
  for (int w = lane; w < RW; w += 64) {
    const unsigned long long x = pm_word<SYM>(row, w), p = (unsigned long long)(w + 1);
    a = (a ^ (x | (p << 32))) * 0x9e3779b97f4a7c15ULL; a ^= a >> 29;
    b = (b ^ ((x << 32) | p)) * 0xc2b2ae3d27d4eb4fULL; b ^= b >> 31;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ta = __shfl_down(a, o), tb = __shfl_down(b, o);
    a = pm_fmix(a * 0x87c37b91114253d5ULL + ta);
    b = pm_fmix(b * 0x4cf5ad432745937fULL + tb);
  }
  if (lane == 0) {
    if (bits < 64) { a &= (1ULL << bits) - 1ULL; b = 0ULL; }
    else if (bits < 128) b &= (1ULL << (bits - 64)) - 1ULL;
    k0[r] = a; k1[r] = b; k1_keep[r] = b; idx[r] = (unsigned int)r;
  }
}
// Position i of the sorted order starts a group unless its row IS row i - 1's.  Keys that differ settle it without reading the
// rows; equal keys are never believed: the wavefront compares every word.  Equal keys over different rows are a collision -- the
// equal rows of either side may lie apart in the order, so the build is given up (a plain store of 1; every writer stores the same).
template <bool SYM>
__global__ void __launch_bounds__(64 * PM_WAVES) k_pm_heads(PmView v, long long n,
                                                            const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1,
                                                            const unsigned int* __restrict__ order, int* __restrict__ head, int* __restrict__ collision) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  if (i == 0) { if (lane == 0) head[0] = 1; return; }
  const unsigned int ra = order[i], rb = order[i - 1];
  if (k0[ra] != k0[rb] || k1[ra] != k1[rb]) { if (lane == 0) head[i] = 1; return; }
  const PmRow a = pm_row<SYM>(v, (long long)ra), b = pm_row<SYM>(v, (long long)rb);
  const int RW = v.RW;
  bool diff = false;
  for (int w = lane; w < RW; w += 64) diff = diff || pm_word<SYM>(a, w) != pm_word<SYM>(b, w);
  const bool differ = __ballot(diff) != 0ULL;
  if (lane == 0) { head[i] = differ ? 1 : 0; if (differ) *collision = 1; }
}
// group s (1-based segid of its head, in key order): its first buffer index -- the sort is stable, so that is its head's -- is the
// key of the sort that orders the output, its number the value; gpos[s] = where it starts in the key order
__global__ void k_pm_groups(const int* __restrict__ head, const int* __restrict__ seg, const unsigned int* __restrict__ order, long long n,
                            unsigned long long* __restrict__ gkey, unsigned int* __restrict__ gval, unsigned int* __restrict__ gpos) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const int s = seg[i] - 1;
  gkey[s] = order[i]; gval[s] = (unsigned int)s; gpos[s] = (unsigned int)i;
}
// One wavefront per output row g = group gord[g], members order[gpos[s] .. gpos[s + 1]) in buffer order.  Lane l owns doubles l and
// l + 64 of the ND = nA + 2 <= 128 (pi..., z, t): two named accumulators, no indexed private array.  Each sum STARTS with the first
// member (keeps -0.0) and adds the others one by one, then divides by the count; n is summed by every lane alike.  X and A are the
// first member's.  order == NULL: no merging, row g is buffer index g.  A member that is an image gives its sample's doubles through
// the action permutation (pm_dcol) and its sample's n.
template <bool SYM>
__global__ void __launch_bounds__(64 * PM_WAVES) k_pm_merge(PmView v, const double* __restrict__ D, const long long* __restrict__ N,
                                                            long long n, long long ngroups, int xs, int nA, int policy,
                                                            const unsigned int* __restrict__ order, const unsigned int* __restrict__ gord,
                                                            const unsigned int* __restrict__ gpos, float* __restrict__ W, float* __restrict__ X,
                                                            float* __restrict__ A, float* __restrict__ P, float* __restrict__ V, long long* __restrict__ t_n) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * PM_WAVES + (threadIdx.x >> 6);
  if (g >= ngroups) return;
  const int ND = nA + 2;
  long long start = g, end = g + 1;
  if (order) {
    const long long s = gord[g];
    start = gpos[s];
    end = s + 1 < ngroups ? (long long)gpos[s + 1] : n;
  }
  const int j0 = lane, j1 = lane + 64;
  const bool h0 = j0 < ND, h1 = j1 < ND;
  const PmRow first = pm_row<SYM>(v, order ? (long long)order[start] : start);
  double acc0 = h0 ? D[first.slot * ND + pm_dcol<SYM>(first, xs, nA, j0)] : 0.0, acc1 = h1 ? D[first.slot * ND + pm_dcol<SYM>(first, xs, nA, j1)] : 0.0;
  long long nsum = N[first.slot];
#pragma unroll 4
  for (long long m = start + 1; m < end; ++m) {
    const PmRow row = pm_row<SYM>(v, (long long)order[m]);
    if (h0) acc0 += D[row.slot * ND + pm_dcol<SYM>(row, xs, nA, j0)];
    if (h1) acc1 += D[row.slot * ND + pm_dcol<SYM>(row, xs, nA, j1)];
    nsum += N[row.slot];
  }
  const double cnt = (double)(end - start);
  acc0 = acc0 / cnt; acc1 = acc1 / cnt;
  if (j0 < nA) P[(size_t)g * nA + j0] = (float)acc0;
  if (j1 < nA) P[(size_t)g * nA + j1] = (float)acc1;
  if (j0 == nA) V[g] = (float)acc0;
  if (j1 == nA) V[g] = (float)acc1;
  if (lane == 0) { W[g] = sample_weight(policy, nsum); t_n[g] = nsum; }
  for (int w = lane; w < xs; w += 64) X[(size_t)g * xs + w] = __uint_as_float(pm_word<SYM>(first, w));
  for (int a = lane; a < nA; a += 64) A[(size_t)g * nA + a] = __uint_as_float(pm_word<SYM>(first, xs + a));
}

// ---- the memory ----------------------------------------------------------------------------------------------------------------------
extern "C" int az_plane_memory_create(int32_t game, int32_t device, int64_t capacity, az_plane_memory** out) {
  if (!out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  GameInfo gi;
  if (!game_info(game, &gi)) return fail(AZ_ERR_BAD_ARG, "unknown game id %d", game);
  if (capacity < 1 || capacity > (1LL << 31) - 1) return fail(AZ_ERR_BAD_ARG, "capacity must be in 1..2^31-1");
  if (gi.A + 2 > 128) return fail(AZ_ERR_BAD_ARG, "game id %d has more than 126 actions", game);   // k_pm_merge: two doubles per lane
  if (gi.C * gi.P + gi.A > 65535) return fail(AZ_ERR_BAD_ARG, "game id %d has rows of more than 65535 words", game);   // d_perm: 16-bit entries
  AZCHK(use_device(device));
  az_plane_memory* m = new (std::nothrow) az_plane_memory();
  if (!m) return fail(AZ_ERR_HIP, "out of host memory");
  m->game = game; m->device = device; m->gi = gi; m->ring.cap = capacity;
  m->xs = gi.C * gi.P; m->nA = gi.A; m->RW = m->xs + m->nA; m->ND = m->nA + 2;
  int st = [&]() -> int {
    HIPCHK(hipStreamCreate(&m->stream));
    AZCHK(mem_alloc(nullptr, &m->d_XA, (size_t)capacity * m->RW));
    AZCHK(mem_alloc(nullptr, &m->d_D, (size_t)capacity * m->ND));
    AZCHK(mem_alloc(nullptr, &m->d_n, (size_t)capacity));
    AZCHK(mem_alloc(nullptr, &m->d_perm, (size_t)AZ_PLANE_MAX_SYMMETRIES * m->RW));
    return AZ_OK;
  }();
  if (st != AZ_OK) { az_plane_memory_destroy(m); return st; }
  *out = m;
  return AZ_OK;
}
extern "C" int az_plane_memory_destroy(az_plane_memory* m) {
  if (!m) return AZ_OK;
  (void)hipSetDevice(m->device);
  if (m->d_XA) (void)hipFree(m->d_XA);
  if (m->d_D) (void)hipFree(m->d_D);
  if (m->d_n) (void)hipFree(m->d_n);
  if (m->d_perm) (void)hipFree(m->d_perm);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return AZ_OK;
}
extern "C" int az_plane_memory_length(az_plane_memory* m, int64_t* length, int64_t* cur_batch_size) {
  PLANE_MEMORY(m);
  if (length) *length = m->ring.len();
  if (cur_batch_size) *cur_batch_size = m->ring.batch();
  return AZ_OK;
}
extern "C" int az_plane_memory_new_batch(az_plane_memory* m) { PLANE_MEMORY(m); m->ring.new_batch(); return AZ_OK; }
extern "C" int az_plane_memory_empty(az_plane_memory* m) { PLANE_MEMORY(m); m->ring.empty(); return AZ_OK; }
extern "C" int az_debug_plane_memory_hash_bits(az_plane_memory* m, int32_t bits) {
  PLANE_MEMORY(m);
  if (bits < 1 || bits > 128) return fail(AZ_ERR_BAD_ARG, "hash bits must be in 1..128");
  m->hash_bits = bits;
  return AZ_OK;
}

// GI.symmetries of the host's game.  Every row is checked to be a bijection of its range here, in plain host code, before anything
// changes: a table that is not one would make the kernels read outside a sample's row.
extern "C" int az_plane_memory_set_symmetries(az_plane_memory* m, int32_t nsym, const int32_t* xperm, const int32_t* aperm) {
  PLANE_MEMORY(m);
  if (nsym < 0 || nsym > AZ_PLANE_MAX_SYMMETRIES) return fail(AZ_ERR_BAD_ARG, "nsym must be in 0..%d", AZ_PLANE_MAX_SYMMETRIES);
  if (nsym > 0 && (!xperm || !aperm)) return fail(AZ_ERR_BAD_ARG, "NULL %s table with nsym = %d", !xperm ? "xperm" : "aperm", nsym);
  const int xs = m->xs, nA = m->nA, RW = m->RW;
  std::vector<unsigned short> perm((size_t)nsym * RW);
  std::vector<int> taken;
  for (int k = 0; k < nsym; ++k)
    for (int table = 0; table < 2; ++table) {
      const int len = table ? nA : xs, base = table ? xs : 0;
      const int32_t* row = table ? aperm + (size_t)k * nA : xperm + (size_t)k * xs;
      const char* name = table ? "aperm" : "xperm";
      taken.assign((size_t)len, -1);
      for (int w = 0; w < len; ++w) {
        const int32_t src = row[w];
        if (src < 0 || src >= len) return fail(AZ_ERR_BAD_ARG, "symmetry %d: %s[%d] = %d is outside 0..%d", k, name, w, (int)src, len - 1);
        if (taken[src] >= 0) return fail(AZ_ERR_BAD_ARG, "symmetry %d: %s[%d] = %d repeats the source of %s[%d]: not a bijection", k, name, w, (int)src, name, taken[src]);
        taken[src] = w;
        perm[(size_t)k * RW + base + w] = (unsigned short)(base + src);
      }
    }
  HIPCHK(hipStreamSynchronize(m->stream));
  if (nsym > 0) HIPCHK(hipMemcpy(m->d_perm, perm.data(), sizeof(unsigned short) * perm.size(), hipMemcpyHostToDevice));
  m->nsym = nsym;
  return AZ_OK;
}
extern "C" int az_plane_memory_num_symmetries(az_plane_memory* m, int32_t* nsym) {
  PLANE_MEMORY(m);
  if (!nsym) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *nsym = m->nsym;
  return AZ_OK;
}

// stage n host samples, check them -- ALL n, those an over-capacity push then skips included -- and store them (reverse: the last
// staged sample is pushed first; advance_batch: push_trace!).  Nothing is pushed on failure.
static int plane_push(az_plane_memory* m, int64_t n, const float* X, const float* A, const double* P, const double* z, const double* t,
                      const int64_t* nvis, bool reverse, bool advance_batch) {
  const size_t N = (size_t)n, xs = (size_t)m->xs, nA = (size_t)m->nA;
  hipStream_t st = m->stream;
  Scratch tmp;
  float *sX, *sA; double *sP, *sz, *stt; long long* sn = nullptr; unsigned long long* d_bad;
  AZCHK(tmp.alloc(&sX, N * xs)); AZCHK(tmp.alloc(&sA, N * nA)); AZCHK(tmp.alloc(&sP, N * nA));
  AZCHK(tmp.alloc(&sz, N)); AZCHK(tmp.alloc(&stt, N)); AZCHK(tmp.alloc(&d_bad, 1));
  if (nvis) AZCHK(tmp.alloc(&sn, N));
  HIPCHK(hipMemcpyAsync(sX, X, sizeof(float) * N * xs, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(sA, A, sizeof(float) * N * nA, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(sP, P, sizeof(double) * N * nA, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(sz, z, sizeof(double) * N, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(stt, t, sizeof(double) * N, hipMemcpyHostToDevice, st));
  if (nvis) HIPCHK(hipMemcpyAsync(sn, nvis, sizeof(long long) * N, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_pm_check, dim3(pm_grid(n)), dim3(64 * PM_WAVES), 0, st, sX, sA, sP, sz, stt, sn, (long long)n, m->xs, m->nA, d_bad);
  unsigned long long bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  AZCHK(sample_fault_status(bad, "n < 1"));
  const long long skip = m->ring.skip(n);
  hipLaunchKernelGGL(k_pm_store, dim3(pm_grid(n - skip)), dim3(64 * PM_WAVES), 0, st, sX, sA, sP, sz, stt, sn, (long long)n, skip, reverse ? 1 : 0,
                     m->xs, m->nA, (long long)m->ring.total, (long long)m->ring.cap, m->d_XA, m->d_D, m->d_n);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  m->ring.pushed(n, advance_batch);
  return AZ_OK;
}
extern "C" int az_plane_memory_push_samples(az_plane_memory* m, int64_t n, const float* X, const float* A, const double* P, const double* z,
                                            const double* t, const int64_t* nvis) {
  PLANE_MEMORY(m);
  if (n < 0 || n > (1LL << 31) - 1) return fail(AZ_ERR_BAD_ARG, "n must be in 0..2^31-1");
  if (!n) return AZ_OK;
  if (!X || !A || !P || !z || !t) return fail(AZ_ERR_BAD_ARG, "NULL array");
  return plane_push(m, n, X, A, P, z, t, nvis, false, false);
}
extern "C" int az_plane_memory_push_trace(az_plane_memory* m, int32_t len, const float* X, const float* A, const double* P, const double* rewards,
                                          const uint8_t* white_playing, double gamma) {
  PLANE_MEMORY(m);
  if (len < 0) return fail(AZ_ERR_BAD_ARG, "len must be >= 0");
  if (!len) return AZ_OK;
  if (!X || !A || !P || !rewards || !white_playing) return fail(AZ_ERR_BAD_ARG, "NULL array");
  if (!std::isfinite(gamma)) return fail(AZ_ERR_BAD_ARG, "gamma is not finite");
  std::vector<double> z((size_t)len), t((size_t)len);
  double wr = 0.0;
  for (int i = len - 1; i >= 0; --i) {                               // memory.jl:76-84
    if (!std::isfinite(rewards[i])) return fail(AZ_ERR_BAD_ARG, "sample %d: a non-finite value", i);
    wr = gamma * wr + rewards[i];
    z[i] = white_playing[i] ? wr : -wr;
    t[i] = (double)(len - i);
  }
  return plane_push(m, len, X, A, P, z.data(), t.data(), nullptr, true, true);
}

// samples [first, first + count) of the buffer, oldest first, back to the host
extern "C" int az_plane_memory_read(az_plane_memory* m, int64_t first, int64_t count, float* X, float* A, double* P, double* z, double* t, int64_t* nvis) {
  PLANE_MEMORY(m);
  const int64_t len = m->ring.len();
  if (first < 0 || count < 0 || first + count > len) return fail(AZ_ERR_BAD_ARG, "range [%lld, %lld) outside the %lld samples", (long long)first, (long long)(first + count), (long long)len);
  if (!count) return AZ_OK;
  const size_t xs = (size_t)m->xs, nA = (size_t)m->nA, RW = (size_t)m->RW, ND = (size_t)m->ND;
  std::vector<float> xa((size_t)count * RW);
  std::vector<double> dd((size_t)count * ND);
  int64_t done = 0;
  for (const Ring::Run& r : m->ring.runs(m->ring.select(0).seq0 + first, count)) {
    const size_t pos = (size_t)r.pos, run = (size_t)r.run;
    HIPCHK(hipMemcpyAsync(xa.data() + (size_t)done * RW, m->d_XA + pos * RW, sizeof(float) * run * RW, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(dd.data() + (size_t)done * ND, m->d_D + pos * ND, sizeof(double) * run * ND, hipMemcpyDeviceToHost, m->stream));
    if (nvis) HIPCHK(hipMemcpyAsync(nvis + done, m->d_n + pos, sizeof(int64_t) * run, hipMemcpyDeviceToHost, m->stream));
    done += r.run;
  }
  HIPCHK(hipStreamSynchronize(m->stream));
  for (size_t i = 0; i < (size_t)count; ++i) {
    if (X) std::memcpy(X + i * xs, xa.data() + i * RW, sizeof(float) * xs);
    if (A) std::memcpy(A + i * nA, xa.data() + i * RW + xs, sizeof(float) * nA);
    if (P) std::memcpy(P + i * nA, dd.data() + i * ND, sizeof(double) * nA);
    if (z) z[i] = dd[i * ND + nA];
    if (t) t[i] = dd[i * ND + nA + 1];
  }
  return AZ_OK;
}

// nsym = 0: the selected samples alone; otherwise [samples ; images] over the declared symmetries (virtual rows, see PmView)
static int plane_dataset_build(az_plane_memory* m, az_dataset* d, int which, int nsym, bool merge, int policy) {
  const Ring::Selection sel = m->ring.select(which);
  const int64_t n0 = sel.n0;
  if (n0 < 1) return fail(AZ_ERR_STATE, which == 1 ? "the current batch is empty (push_trace advances it, new_batch resets it)" : "the plane memory is empty");
  const int64_t n1 = n0 * (1 + nsym);                                // rows of the build; the sort's indices are 32-bit
  if (n1 > (1LL << 31) - 1) return fail(AZ_ERR_BAD_ARG, "%lld samples with %d symmetries are %lld rows: more than 2^31-1", (long long)n0, nsym, (long long)n1);
  const bool sym = nsym > 0;
  const PmView view{m->d_XA, (long long)m->ring.cap, (long long)sel.seq0, (long long)n0, m->RW, nsym, m->d_perm};
  const int xs = m->xs, nA = m->nA;
  Scratch tmp;
  HIPCHK(hipStreamSynchronize(m->stream));                           // the memory's pushes are done; the data set works on a stream of its own
  HIPCHK(hipStreamCreate(&d->stream));
  hipStream_t st = d->stream;
  unsigned int *order = nullptr, *gord = nullptr, *gpos = nullptr;
  int64_t n2 = n1;
  if (merge) {
    unsigned long long *k1keep, *gkey, *gks; unsigned int* gval; int* coll;   // k1keep: the sort destroys its copy of the key's second half
    AZCHK(tmp.alloc(&k1keep, (size_t)n1)); AZCHK(tmp.alloc(&coll, 1));
    HIPCHK(hipMemsetAsync(coll, 0, sizeof(int), st));
    Grouping g;
    AZCHK(group_by_key(tmp, n1, st,
                       [&](unsigned long long* k0, unsigned long long* k1, unsigned int* idx) {
                         hipLaunchKernelGGL(sym ? k_pm_hash<true> : k_pm_hash<false>, dim3(pm_grid(n1)), dim3(64 * PM_WAVES), 0, st, view, (long long)n1, m->hash_bits, k0, k1, k1keep, idx);
                       },
                       [&](const unsigned long long* k0, const unsigned int* order, int* head) {
                         hipLaunchKernelGGL(sym ? k_pm_heads<true> : k_pm_heads<false>, dim3(pm_grid(n1)), dim3(64 * PM_WAVES), 0, st, view, (long long)n1, k0, k1keep, order, head, coll);
                       },
                       &g));
    int nseg = 0, collision = 0;
    HIPCHK(hipMemcpyAsync(&nseg, g.seg + (n1 - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&collision, coll, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (collision) return fail(AZ_ERR_STATE, "plane hash collision: two different (X, A) rows share their %d-bit key; no data set was built", m->hash_bits);
    n2 = nseg;
    const size_t G = (size_t)n2;
    AZCHK(tmp.alloc(&gkey, G)); AZCHK(tmp.alloc(&gks, G)); AZCHK(tmp.alloc(&gval, G)); AZCHK(tmp.alloc(&gord, G)); AZCHK(tmp.alloc(&gpos, G));
    hipLaunchKernelGGL(k_pm_groups, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, g.head, g.seg, g.order, (long long)n1, gkey, gval, gpos);
    HIPCHK(prims::sort_pairs(gkey, gks, gval, gord, n2, g.stmp, st));   // n2 <= n1: stmp is large enough
    order = g.order;
  }
  d->n = n2;
  AZCHK(dataset_alloc_tensors(d, n2));
  long long* tn;
  DevReducer red;
  AZCHK(tmp.alloc(&tn, (size_t)n2)); AZCHK(red.init(n2));
  hipLaunchKernelGGL(sym ? k_pm_merge<true> : k_pm_merge<false>, dim3(pm_grid(n2)), dim3(64 * PM_WAVES), 0, st, view, m->d_D, m->d_n, (long long)n1, (long long)n2,
                     xs, nA, policy, order, gord, gpos, d->d_W, d->d_X, d->d_A, d->d_P, d->d_V, tn);
  long long sn = 0;
  AZCHK(red.sum(tn, n2, st, &sn));
  HIPCHK(hipGetLastError());
  d->sum_n = (int64_t)sn;
  AZCHK(dataset_tensor_stats(d, st));                              // Wtot, Wmean, Hp as az_dataset_create_from_tensors computes them
  return AZ_OK;
}
extern "C" int az_dataset_create_from_plane_memory_sym(az_plane_memory* m, int32_t which, int32_t use_symmetries, int32_t use_position_averaging,
                                                       int32_t weighing_policy, az_dataset** out) {
  PLANE_MEMORY(m);
  if (!out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  AZCHK(dataset_check_args(which, weighing_policy));
  if (use_symmetries && m->nsym == 0) return fail(AZ_ERR_BAD_ARG, "use_symmetries: no symmetries were declared for this memory (game.jl:332; az_plane_memory_set_symmetries)");
  return dataset_create(m->game, m->device, m->gi, nullptr, out, [&](az_dataset* d) -> int {
    return plane_dataset_build(m, d, which, use_symmetries ? m->nsym : 0, use_position_averaging != 0, weighing_policy);
  });
}
extern "C" int az_dataset_create_from_plane_memory(az_plane_memory* m, int32_t which, int32_t use_position_averaging, int32_t weighing_policy,
                                                   az_dataset** out) {
  return az_dataset_create_from_plane_memory_sym(m, which, 0, use_position_averaging, weighing_policy, out);
}
