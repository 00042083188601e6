// simplenet.h -- NetLib.SimpleNet (src/networks/architectures/simplenet.jl:37-64) in test mode, the whole network in ONE launch:
//   common = flatten, D(indim -> h), D(h -> h) x depth_common                         (simplenet.jl:52-55)
//   vhead  = D(h -> h) x depth_vhead, Dense(h -> 1, tanh)                              (simplenet.jl:56-58)
//   phead  = D(h -> h) x depth_phead, Dense(h -> A), softmax                           (simplenet.jl:59-62)
//   D(i -> o) = Dense(i -> o) + BatchNorm(o, relu) or Dense(i -> o, relu)              (simplenet.jl:39-47)
// followed by Network.forward_normalized (network.jl:264-271), as the ResNet's heads (resnet.h heads_finish_policy: shared as it is).
//
// k_simplenet<Gm, FROM_PLANES>: a workgroup of 4 wavefronts takes SN_ROWS boards through every layer.  Activations never leave LDS:
// three buffers [SN_ROWS][rs] (the common trunk alternates between two; its result stays in one while each head alternates between the
// other two), no feature buffer in HBM.  A layer is a [SN_ROWS x K] x [K x O] product on v_mfma_f32_16x16x4_f32: wavefront w owns the
// 16-column tiles w, w + 4, ... (up to 4 of them: width <= 256) -- from width 65 on every wavefront has 2 to 4 independent accumulators,
// which covers the instruction's 40-cycle dependent latency at its 32-cycle issue interval (narrower networks have fewer tiles than
// that and are bounded by the weight fetch anyway).  K runs upwards, 16 per block: the four MFMAs of a block
// take k = 16 j + 4 q + (lane >> 4), q = 0 .. 3 -- every output is one ascending fp32 fma chain over k, no split-K, no atomics.
//   B operand: the host orders every layer into fragments [column tile][k block][64 lanes][4] (net_layout.h order_simple16); a lane's
//     load is one coalesced float4 that feeds the block's four MFMAs, fetched SN_PD blocks ahead of them.
//   A operand: one ds_read_b128 per row tile and block.  A row keeps the 16 features of a block transposed ([k slot][q]) so that the lane's
//     four values are consecutive, the k slot rotated by 2 in rows 4..7 and 12..15, and rs = 16 (mod 64) words: with these the four lane
//     groups of a ds_read_b128 each cover the 64 banks exactly once (the arrangement of k_heads16's staged features, resnet.h).
//   Padding: width is padded to 16 in columns and in k (the input to 16 in k) by the index maps' zero entries; the padded outputs are
//     relu(fma(0, 0 or 1, 0)) = 0.  No branch in the kernel knows the true width.
//   Epilogue: relu(fma(acc, scale, shift)) with the test-mode batch norm folded on the host exactly as the towers' bn_fold (scale =
//     gamma / sqrtf(var + 1e-5f), shift = fma(b - mean, scale, beta)); without batch norm scale = 1, shift = b.  The two final layers
//     are fma(acc, 1, b) = acc + b without relu, then softmax / mask / p / (sum + eps(Float32)) / 1 - sum (heads_finish_policy) and tanh.
// A board's result depends on that board alone: its row meets no other row in any MFMA, so batch size, position and source change no bit.
// width and the depths are runtime values (SimpleDev); the template is on the game only.
#pragma once
#include "resnet.h"

// Boards per workgroup: 16.  Measured with the shipped Tic-tac-toe network (profiles/simplenet/README.md): a launch costs one workgroup's
// walk through the layers whatever its size up to one workgroup per CU -- 61 us with 16 boards, 84 us with 32, at 128, 1024 and 4096
// boards alike (4096 boards are 256 workgroups of 16: one round on 256 CUs).  The 32-board form was measured and deleted.
static constexpr int SN_RT = 1;                       // row tiles of 16 boards per workgroup
static constexpr int SN_ROWS = 16 * SN_RT;            // boards per workgroup
static constexpr int SN_WAVES = 4, SN_THREADS = 64 * SN_WAVES;
static constexpr int SN_TPW = 4;                      // column tiles per wavefront at most: width <= 16 SN_WAVES SN_TPW = 256
static constexpr int SN_PD = 4;                       // k blocks of weight fragments in flight
static constexpr int SN_MAX_DEPTH = 16;               // each of depth_common, depth_phead, depth_vhead
static constexpr int SN_MAX_LAYERS = 1 + 3 * SN_MAX_DEPTH + 2;
static constexpr int SN_OUT = 32;                     // final outputs per board in LDS: logits [0, 16), the value's pre-activation at 16

enum SnMode : uint8_t { SN_HIDDEN = 0, SN_POLICY = 1, SN_VALUE = 2 };
struct SnLayer {
  uint32_t w_off, ss_off;          // float offsets of the layer's fragments in SimpleDev::w, of its [2][16 ct] scale / shift in SimpleDev::ss
  uint16_t kb, ct;                 // k blocks of 16, column tiles of 16
  uint8_t src, dst, mode, pad;     // activation buffers read and written (dst unused by the final layers), SnMode
};
struct SimpleDev {
  const float* w; const float* ss;
  int nlayers, rs, indim, kp0;     // rs: words per activation row (16 mod 64); kp0: the input padded to 16
  SnLayer layer[SN_MAX_LAYERS];
};
// words per activation row for the widest K of a network
static inline int sn_row_words(int kmax) { return (kmax + 63) / 64 * 64 + 16; }
static inline size_t sn_lds_bytes(int rs) { return ((size_t)3 * SN_ROWS * rs + (size_t)SN_ROWS * SN_OUT) * sizeof(float); }

// where feature f of row r lies in an activation buffer
__device__ __forceinline__ int sn_at(int r, int f, int rs) {
  return r * rs + (f & ~15) + 4 * (((f & 3) + 2 * ((r >> 2) & 1)) & 3) + ((f >> 2) & 3);
}

template <int NT>
__device__ __forceinline__ void sn_layer(const SnLayer& L, const f32x4v* __restrict__ wl, const float* __restrict__ ss,
                                         const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ s_out, int rs,
                                         int wave, int lane) {
  const int m = lane & 15, g = lane >> 4, kb = L.kb;
  f32x4v acc[SN_RT][NT];
#pragma unroll
  for (int r = 0; r < SN_RT; ++r)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[r][t] = f32x4v{0.f, 0.f, 0.f, 0.f};
  const float* ap = src + m * rs + 4 * ((g + 2 * ((m >> 2) & 1)) & 3);
  const f32x4v* wp = wl + (size_t)wave * kb * 64 + lane;            // tile wave + SN_WAVES t is SN_WAVES kb fragments further on
  const size_t tstep = (size_t)SN_WAVES * kb * 64;
  f32x4v b[SN_PD][NT];
  static_for<SN_PD>([&](auto pc) {
    constexpr int p = decltype(pc)::value;
    if (p < kb) {
#pragma unroll
      for (int t = 0; t < NT; ++t) b[p][t] = wp[(size_t)p * 64 + t * tstep];
    }
  });
  for (int j0 = 0; j0 < kb; j0 += SN_PD) {
    static_for<SN_PD>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      const int j = j0 + p;
      if (j < kb) {
        f32x4v a[SN_RT], bb[NT];
#pragma unroll
        for (int r = 0; r < SN_RT; ++r) a[r] = *(const f32x4v*)(ap + 16 * r * rs + 16 * j);
#pragma unroll
        for (int t = 0; t < NT; ++t) bb[t] = b[p][t];
        if (j + SN_PD < kb) {
#pragma unroll
          for (int t = 0; t < NT; ++t) b[p][t] = wp[(size_t)(j + SN_PD) * 64 + t * tstep];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int r = 0; r < SN_RT; ++r)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][q], bb[t][q], acc[r][t], 0, 0, 0);
      }
    });
  }
  const int op = 16 * L.ct;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int o = 16 * (wave + SN_WAVES * t) + m;
    const float sc = ss[o], sh = ss[op + o];
#pragma unroll
    for (int r = 0; r < SN_RT; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * r + 4 * g + i;
        const float v = az_fmaf(acc[r][t][i], sc, sh);
        if (L.mode == SN_HIDDEN) dst[sn_at(row, o, rs)] = v > 0.0f ? v : 0.0f;
        else if (o < 16) s_out[row * SN_OUT + (L.mode == SN_VALUE ? 16 : 0) + o] = v;
      }
  }
}

template <class Gm, bool FROM_PLANES>
__global__ void __launch_bounds__(SN_THREADS)
k_simplenet(SimpleDev net, const GEnv* __restrict__ envs, const int* __restrict__ eslots, const int* __restrict__ n_ptr, int n_fixed,
            const float* __restrict__ X, const float* __restrict__ Amask, float* __restrict__ Pout, float* __restrict__ Vout,
            float* __restrict__ Pinv, int pstride) {
  static_assert(Gm::A <= 16, "one policy tile");
  constexpr int P = Gm::P, IN = Gm::C * Gm::P;
  extern __shared__ __attribute__((aligned(16))) float sn_lds[];
  const int n = n_ptr ? *n_ptr : n_fixed;
  const int board0 = (int)blockIdx.x * SN_ROWS;
  if (board0 >= n) return;                                          // the grid is sized for n_max
  const int rs = net.rs, buf = SN_ROWS * rs;
  float* s_out = sn_lds + 3 * buf;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // flatten: feature f = c P + q of the W x H x C array in memory order; rows past the batch repeat its last board and are dropped
  for (int idx = threadIdx.x; idx < SN_ROWS * net.kp0; idx += SN_THREADS) {
    const int r = idx / net.kp0, f = idx % net.kp0;
    int e = board0 + r;
    if (e >= n) e = n - 1;
    float v = 0.0f;
    if (f < IN) {
      if constexpr (FROM_PLANES) v = X[(size_t)e * IN + f];
      else v = Gm::plane(envs[eslots[e]], f % P, f / P);
    }
    sn_lds[sn_at(r, f, rs)] = v;
  }
  __syncthreads();
  for (int li = 0; li < net.nlayers; ++li) {
    const SnLayer L = net.layer[li];
    const int nt = ((int)L.ct - wave + SN_WAVES - 1) / SN_WAVES;    // column tiles of this wavefront
    const f32x4v* wl = (const f32x4v*)(net.w + L.w_off);
    const float* ss = net.ss + L.ss_off;
    const float* src = sn_lds + L.src * buf;
    float* dst = sn_lds + L.dst * buf;
    switch (nt) {
      case 1: sn_layer<1>(L, wl, ss, src, dst, s_out, rs, wave, lane); break;
      case 2: sn_layer<2>(L, wl, ss, src, dst, s_out, rs, wave, lane); break;
      case 3: sn_layer<3>(L, wl, ss, src, dst, s_out, rs, wave, lane); break;
      case 4: sn_layer<4>(L, wl, ss, src, dst, s_out, rs, wave, lane); break;
      default: break;
    }
    __syncthreads();
  }
  const int b = threadIdx.x;
  if (b < SN_ROWS && board0 + b < n) {
    heads_finish_policy<Gm>(envs, eslots, Amask, Pout, Pinv, pstride, board0 + b, s_out + b * SN_OUT);
    Vout[board0 + b] = az_tanhf(s_out[b * SN_OUT + 16]);            // Dense(h -> 1, tanh), simplenet.jl:58
  }
}
