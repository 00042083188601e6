// train.hip -- the optimiser step on the device (second half; first version).
//
//   batch_updates!(tr, n)                      src/learning.jl:131-141
//   Network.train!(callback, nn, opt, ...)     src/networks/flux.jl:68-95   (Flux.withgradient + Flux.update!)
//   losses                                      src/learning.jl:67-90
//   ResNet in TRAIN mode                        src/networks/architectures/resnet.jl:53-92 (BatchNorm with batch statistics)
//
// Structure of this version: the F -> F tower convolutions run on hand-written MFMA kernels in all three passes --
// forward and data gradient on k_conv16_layer (the tower's implicit GEMM as a stand-alone layer), the weight gradient
// on k_wgrad16 (resnet16.h); the stem (K = 27), the 1x1 head convolutions and the dense layers are small plain fp32
// GEMMs on a hand-written MFMA kernel (gemm.h; im2col by a hand-written gather where needed);
// everything that is not a GEMM is hand-written here too: batch-norm statistics / apply / backward with
// deterministic two-stage column reductions, ReLU and skip wiring, the loss with its analytic gradient (softmax,
// mask normalisation, KL, invalid-mass penalty, tanh / MSE), parameter layout maps between Flux's arrays and the
// GEMM matrices, Adam / Nesterov and the running statistics.  No library call is left in the step (round 1 used a
// dlopen'ed rocBLAS for the small GEMMs).  The fused inference tower is untouched: after training the new
// parameters go back through az_net_set_params.
//
// One step for both networks: trainer_build writes a network down as a table of GEMM layers (TrLayer) -- a ResNet as stem, tower, the two
// 1x1 head convolutions and the three dense head layers, a SimpleNet as its dense chain -- and tr_forward_backward walks that table:
// gemm_layer_forward / gemm_layer_backward for every layer but the tower's F -> F convolutions, which keep their explicit MFMA block.
//
#include "engine.h"

// ------------------------------------------------------------------------------------------ small GEMMs
#include "gemm.h"
struct az_trainer;
static int tr_gemm(az_trainer* t, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                   float beta, float* C, int ldc);

// ------------------------------------------------------------------------------------------ kernels
// work[j] = blob[map[j]]  /  gblob[map[j]] = gwork[j]   (parameter layout maps, built on the host once)
__global__ void k_tr_gather(const float* __restrict__ blob, const int* __restrict__ map, long long n, float* __restrict__ work) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) work[j] = blob[map[j]];
}
// gblob[map[j]] = gwork[j] for the working entries j = list[i] that carry a gradient (one launch for every layer)
__global__ void k_tr_scatter(const float* __restrict__ gwork, const int* __restrict__ map, const int* __restrict__ list, long long n, float* __restrict__ gblob) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const int j = list[i]; gblob[map[j]] = gwork[j]; }
}
// the batch of a step: rows idx[0..B) of the data set's tensors
__global__ void k_tr_batch(const int* __restrict__ idx, int B, int xs, int A, const float* __restrict__ W, const float* __restrict__ X,
                           const float* __restrict__ Am, const float* __restrict__ P, const float* __restrict__ V,
                           float* bW, float* bX, float* bA, float* bP, float* bV) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const size_t s = (size_t)idx[b];
  for (int i = threadIdx.x; i < xs; i += blockDim.x) bX[(size_t)b * xs + i] = X[s * xs + i];
  for (int i = threadIdx.x; i < A; i += blockDim.x) { bA[(size_t)b * A + i] = Am[s * A + i]; bP[(size_t)b * A + i] = P[s * A + i]; }
  if (threadIdx.x == 0) { bW[b] = W[s]; bV[b] = V[s]; }
}
template <bool PLANES>
__global__ void __launch_bounds__(256) k_tr_im2col(const float* __restrict__ in, long long R, int C, int Wd, int Hd, float* __restrict__ col) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = R * 9 * C;
  if (t >= total) return;
  const int c = (int)(t % C);
  const int tap = (int)((t / C) % 9);
  const long long r = t / (9LL * C);
  const int P = Wd * Hd, q = (int)(r % P), x = q % Wd, y = q / Wd;
  const int dy = tap / 3 - 1, dx = tap % 3 - 1;
  float v = 0.0f;
  if (y + dy >= 0 && y + dy < Hd && x + dx >= 0 && x + dx < Wd) {
    const long long rr = r + dy * Wd + dx;
    v = PLANES ? in[((rr / P) * C + c) * P + (rr % P)] : in[rr * C + c];
  }
  col[t] = v;
}
// two-stage column sums over R rows of up to two derived quantities.  Stage 1: a block = 64 channels x 4 row lanes takes
// a chunk of 64 rows (thread: 16 rows, then the 4 lanes are added in lane order); stage 2: one block per channel adds
// the chunk partials with a fixed-shape tree.  Deterministic, double accumulators.
//   MODE 0: (x, x*x)                       batch-norm statistics of the GEMM output
//   MODE 1: (dy, dy * xhat)                batch-norm backward, dy = da * (out > 0), xhat = (g - mean) * invstd
//   MODE 2: (x, 0)                         bias gradients of the dense layers
constexpr int TR_CHUNK = 64;
template <int MODE>
__global__ void __launch_bounds__(256) k_tr_colsum(const float* __restrict__ x, const float* __restrict__ out_act, const float* __restrict__ g,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd, long long R, int C,
                                                   double* __restrict__ part /* [nchunks][2][C] */, TrFinal fin) {
  __shared__ double sh[2][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const long long r0 = (long long)blockIdx.x * TR_CHUNK, r1 = r0 + TR_CHUNK < R ? r0 + TR_CHUNK : R;
  double s0 = 0.0, s1 = 0.0;
  if (c < C) {
    float mu = 0.f, is = 0.f;
    if (MODE == 1) { mu = mean[c]; is = invstd[c]; }
    for (long long r = r0 + rl; r < r1; r += 4) {
      const size_t i = (size_t)r * C + c;
      if (MODE == 0) { const float v = x[i]; s0 += (double)v; s1 += (double)v * (double)v; }
      else if (MODE == 1) {
        const float dy = out_act[i] > 0.0f ? x[i] : 0.0f;
        const float xh = (g[i] - mu) * is;
        s0 += (double)dy; s1 += (double)dy * (double)xh;
      } else s0 += (double)x[i];
    }
  }
  sh[0][rl][cl] = s0; sh[1][rl][cl] = s1;
  __syncthreads();
  if (rl == 0 && c < C) {
    part_store(part + ((size_t)blockIdx.x * 2) * C + c, ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl]);
    part_store(part + ((size_t)blockIdx.x * 2 + 1) * C + c, ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl]);
  }
  __syncthreads();
  if (C <= 128) tr_finish(part, C, fin, &sh[0][0][0]);               // 512 doubles of scratch: 256 + 2 C (host: wider layers keep the separate launch)
}
// MODE 1 with four channels per thread (C % 4 == 0, 256 % (C/4) == 0): a block = C/4 channel quads x 256/(C/4) row lanes
// over the same 64-row chunk, 16-byte loads; the row lanes are added in lane order through 8 KB of LDS (it has to fit
// beside two workgroups of k_wgrad16, and the first form of that kernel left 10 KB).  Same partial layout as k_tr_colsum.
__global__ void __launch_bounds__(256) k_tr_colsum1v(const float* __restrict__ x, const float* __restrict__ out_act, const float* __restrict__ g,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd, long long R, int C,
                                                     double* __restrict__ part /* [nchunks][2][C] */, TrFinal fin) {
  __builtin_amdgcn_s_setprio(3);   // HBM-bound and short: its few instructions go first when it shares a SIMD with k_wgrad16's wavefronts
  __shared__ double sh[256][4];
  const int CQ = C >> 2, RL = 256 / CQ;
  const int q = threadIdx.x % CQ, rl = threadIdx.x / CQ;
  const long long r0 = (long long)blockIdx.x * TR_CHUNK, r1 = r0 + TR_CHUNK < R ? r0 + TR_CHUNK : R;
  const float4 mu = *(const float4*)(mean + 4 * q), is = *(const float4*)(invstd + 4 * q);
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  auto add = [&](const float4& vx, const float4& va, const float4& vg) {
    const float dx[4] = {vx.x, vx.y, vx.z, vx.w}, av[4] = {va.x, va.y, va.z, va.w}, gv[4] = {vg.x, vg.y, vg.z, vg.w};
    const float m[4] = {mu.x, mu.y, mu.z, mu.w}, iv[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dy = av[k] > 0.0f ? dx[k] : 0.0f;
      const float xh = (gv[k] - m[k]) * iv[k];
      s0[k] += (double)dy; s1[k] += (double)dy * (double)xh;
    }
  };
  long long r = r0 + rl;
  for (; r + 3 * RL < r1; r += 4 * RL) {                            // four rows in flight: beside k_wgrad16 this kernel gets one wavefront per SIMD
    const size_t i0 = (size_t)r * C + 4 * q, i1 = i0 + (size_t)RL * C, i2 = i1 + (size_t)RL * C, i3 = i2 + (size_t)RL * C;
    const float4 x0 = *(const float4*)(x + i0), a0 = *(const float4*)(out_act + i0), g0 = *(const float4*)(g + i0);
    const float4 x1 = *(const float4*)(x + i1), a1 = *(const float4*)(out_act + i1), g1 = *(const float4*)(g + i1);
    const float4 x2 = *(const float4*)(x + i2), a2 = *(const float4*)(out_act + i2), g2 = *(const float4*)(g + i2);
    const float4 x3 = *(const float4*)(x + i3), a3 = *(const float4*)(out_act + i3), g3 = *(const float4*)(g + i3);
    add(x0, a0, g0); add(x1, a1, g1); add(x2, a2, g2); add(x3, a3, g3);
  }
  for (; r + RL < r1; r += 2 * RL) {                                // two rows in flight
    const size_t i = (size_t)r * C + 4 * q, j = i + (size_t)RL * C;
    const float4 x0 = *(const float4*)(x + i), a0 = *(const float4*)(out_act + i), g0 = *(const float4*)(g + i);
    const float4 x1 = *(const float4*)(x + j), a1 = *(const float4*)(out_act + j), g1 = *(const float4*)(g + j);
    add(x0, a0, g0); add(x1, a1, g1);
  }
  for (; r < r1; r += RL) {
    const size_t i = (size_t)r * C + 4 * q;
    add(*(const float4*)(x + i), *(const float4*)(out_act + i), *(const float4*)(g + i));
  }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[threadIdx.x][k] = w == 0 ? s0[k] : s1[k];
    __syncthreads();
    if (rl == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double v = sh[q][k];
        for (int l = 1; l < RL; ++l) v += sh[q + l * CQ][k];
        part_store(part + ((size_t)blockIdx.x * 2 + w) * C + 4 * q + k, v);
      }
    }
    __syncthreads();
  }
  tr_finish(part, C, fin, &sh[0][0]);                                // 1024 doubles of scratch >= 256 + 2 C (C <= 256 here... the host checks)
}
// the second stage of a column sum: one workgroup per channel adds the producers' partials in a fixed order and does what the
// mode says (TrFinal, resnet16.h).  A launch of its own after every producer: riding in the producer's LAST workgroup (tr_finish)
// was built and measured in round 4 -- one workgroup reading 256 ... 672 x 2 C partials through cache-bypassing loads takes
// longer (3.4 ms per step at 5x64 instead of 1.9) than the ~6 us a dependent launch costs.
__global__ void __launch_bounds__(64) k_tr_colsum_final(const double* __restrict__ part, int nchunks, int C, double* __restrict__ sums /* [2][C] */, TrFinal f) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ double sh[2][64];
  const int c = blockIdx.x, t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int k = t; k < nchunks; k += 64) { s0 += part[((size_t)k * 2) * C + c]; s1 += part[((size_t)k * 2 + 1) * C + c]; }
  sh[0][t] = s0; sh[1][t] = s1;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (t < w) { sh[0][t] += sh[0][t + w]; sh[1][t] += sh[1][t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    const double s0 = sh[0][0], s1 = sh[1][0];
    sums[c] = s0; sums[C + c] = s1;
    if (f.mode == 1) {
      // batch statistics -> mean, 1/sqrt(var + eps) (Flux BatchNorm: biased variance, eps 1e-5) and the running statistics
      // mu <- (1-m) mu + m (mean + bias), var <- (1-m) var + m * var * R/(R-1)
      const double m = s0 / (double)f.R;
      double var = s1 / (double)f.R - m * m;
      if (var < 0.0) var = 0.0;
      f.mean[c] = (float)m;
      f.invstd[c] = (float)(1.0 / __builtin_sqrt(var + 1e-5));
      const float b = f.bias ? f.bias[c] : 0.0f;
      f.run_mean[c] = (1.0f - f.momentum) * f.run_mean[c] + f.momentum * ((float)m + b);
      f.run_var[c] = (1.0f - f.momentum) * f.run_var[c] + f.momentum * (float)(var * ((double)f.R / (double)(f.R - 1)));
    } else if (f.mode == 2) { f.dbeta[c] = (float)s0; f.dgamma[c] = (float)s1; f.mf[c] = (float)(s0 / (double)f.R); f.mf[C + c] = (float)(s1 / (double)f.R); }
    else if (f.mode == 3) f.out0[c] = (float)s0;
  }
}
// a = relu(gamma * xhat + beta (+ res))
__global__ void k_tr_bn_apply(const float* __restrict__ g, const float* __restrict__ mean, const float* __restrict__ invstd,
                              const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ res,
                              long long n, int C, float* __restrict__ a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  float v = gamma[c] * ((g[i] - mean[c]) * invstd[c]) + beta[c];
  if (res) v += res[i];
  a[i] = v > 0.0f ? v : 0.0f;
}
// batch-norm backward: dy = da * (a > 0); dg = gamma * invstd * (dy - sum(dy)/R - xhat * sum(dy*xhat)/R); dgamma = sum(dy*xhat),
// dbeta = sum(dy).  `dy_out` (optional) receives dy: the gradient that also flows into the skip connection.  mf = the two
// means as floats (k_tr_colsum_final, mode 2).  V = 4: four channels per thread (C % 4 == 0), the form that still moves
// bytes when it shares the chip with k_wgrad16 and gets one wavefront per SIMD.
template <int V>
__global__ void __launch_bounds__(256) k_tr_bn_bwd(const float* __restrict__ da, const float* __restrict__ a, const float* __restrict__ g,
                            const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                            const float* __restrict__ mf, long long n, int C, float* __restrict__ dg, float* __restrict__ dy_out) {
  __builtin_amdgcn_s_setprio(3);
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= n) return;
  const int c = (int)(i % C);
  float vda[V], va[V], vg[V], o[V], dyv[V];
  if constexpr (V == 4) {
    const float4 x = *(const float4*)(da + i), y = *(const float4*)(a + i), z = *(const float4*)(g + i);
    vda[0] = x.x; vda[1] = x.y; vda[2] = x.z; vda[3] = x.w; va[0] = y.x; va[1] = y.y; va[2] = y.z; va[3] = y.w; vg[0] = z.x; vg[1] = z.y; vg[2] = z.z; vg[3] = z.w;
  } else { vda[0] = da[i]; va[0] = a[i]; vg[0] = g[i]; }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float dy = va[k] > 0.0f ? vda[k] : 0.0f;
    const float xh = (vg[k] - mean[c + k]) * invstd[c + k];
    o[k] = gamma[c + k] * invstd[c + k] * (dy - mf[c + k] - xh * mf[C + c + k]);
    dyv[k] = dy;
  }
  if constexpr (V == 4) {
    *(float4*)(dg + i) = make_float4(o[0], o[1], o[2], o[3]);
    if (dy_out) *(float4*)(dy_out + i) = make_float4(dyv[0], dyv[1], dyv[2], dyv[3]);
  } else { dg[i] = o[0]; if (dy_out) dy_out[i] = dyv[0]; }
}
// dense epilogues: y = [relu](x + bias[c]);  backward mask: dx = dy * (y > 0)
__global__ void k_tr_bias_act(float* __restrict__ x, const float* __restrict__ bias, long long n, int C, int relu) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = x[i] + bias[(int)(i % C)];
  x[i] = relu ? (v > 0.0f ? v : 0.0f) : v;
}
__global__ void k_tr_relu_bwd(float* __restrict__ dy, const float* __restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !(y[i] > 0.0f)) dy[i] = 0.0f;
}
// `losses` (learning.jl:67-90) for one batch, forward terms and the analytic gradient w.r.t. the policy logits and the
// value pre-activation.  scale = (mean(W_batch) / Wmean) / sum(W_batch) is folded into the gradients.
//   p = softmax(logits); u = p .* A; S = sum(u); q = u / (S + eps)            (network.jl:264-271)
//   Lp_i = -sum_a P_a log(q_a + eps) w;  Linv_i = (1 - S) w;  Lv_i = ((tanh(t) - V) / rho)^2 w
__global__ void k_tr_loss(const float* __restrict__ logits, const float* __restrict__ tpre, const float* __restrict__ Am,
                          const float* __restrict__ P, const float* __restrict__ V, const float* __restrict__ W, int B, int A,
                          float cinv, float rho, float gscale, float* __restrict__ dlogits, float* __restrict__ dt,
                          double* __restrict__ t_w, double* __restrict__ t_kl, double* __restrict__ t_mse, double* __restrict__ t_inv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float eps = 1.1920929e-07f;
  float p[AZ_MAX_ACTIONS], u[AZ_MAX_ACTIONS], gq[AZ_MAX_ACTIONS];
  float mx = logits[(size_t)i * A];
  for (int a = 1; a < A; ++a) mx = logits[(size_t)i * A + a] > mx ? logits[(size_t)i * A + a] : mx;
  float se = 0.0f;
  for (int a = 0; a < A; ++a) { p[a] = az_expf(logits[(size_t)i * A + a] - mx); se += p[a]; }
  float S = 0.0f;
  for (int a = 0; a < A; ++a) { p[a] = p[a] / se; u[a] = p[a] * Am[(size_t)i * A + a]; S += u[a]; }
  const float w = W[i];
  const float den = S + eps;
  double kl = 0.0;
  float gu_sum = 0.0f;                                             // sum_b gq_b * u_b / den^2
  for (int a = 0; a < A; ++a) {
    const float q = u[a] / den;
    const float Pa = P[(size_t)i * A + a];
    kl += (double)(Pa * az_logf(q + eps) * w);
    gq[a] = -Pa / (q + eps);                                       // dLp_i/dq_a (per unit weight)
    gu_sum += gq[a] * u[a];
  }
  gu_sum = gu_sum / (den * den);
  // dL/dp_a = A_a * (gq_a / den - gu_sum - cinv) * w * gscale ;  softmax backward
  float dp[AZ_MAX_ACTIONS], dot = 0.0f;
  for (int a = 0; a < A; ++a) {
    dp[a] = Am[(size_t)i * A + a] * (gq[a] / den - gu_sum - cinv) * w * gscale;
    dot += p[a] * dp[a];
  }
  for (int a = 0; a < A; ++a) dlogits[(size_t)i * A + a] = p[a] * (dp[a] - dot);
  const float vh = az_tanhf(tpre[i]);
  const float d = vh / rho - V[i] / rho;
  dt[i] = 2.0f * d / rho * (1.0f - vh * vh) * w * gscale;
  t_w[i] = (double)w; t_kl[i] = kl; t_mse[i] = (double)(d * d * w); t_inv[i] = (double)((1.0f - S) * w);
}
// The same loss for an action set wider than AZ_MAX_ACTIONS (9x9 boards: 82): the same operations in the same order per sample, but
// the softmax p lives in the sample's row of dlogits (which the last loop overwrites with the gradient) and u, gq, dp are computed
// again where they are used instead of being kept in per-thread arrays -- 4 x 82 floats per thread would go to scratch memory.
__global__ void k_tr_loss_wide(const float* __restrict__ logits, const float* __restrict__ tpre, const float* __restrict__ Am,
                               const float* __restrict__ P, const float* __restrict__ V, const float* __restrict__ W, int B, int A,
                               float cinv, float rho, float gscale, float* __restrict__ dlogits, float* __restrict__ dt,
                               double* __restrict__ t_w, double* __restrict__ t_kl, double* __restrict__ t_mse, double* __restrict__ t_inv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float eps = 1.1920929e-07f;
  const float* lg = logits + (size_t)i * A;
  const float* am = Am + (size_t)i * A;
  const float* pt = P + (size_t)i * A;
  float* p = dlogits + (size_t)i * A;
  float mx = lg[0];
  for (int a = 1; a < A; ++a) mx = lg[a] > mx ? lg[a] : mx;
  float se = 0.0f;
  for (int a = 0; a < A; ++a) { const float v = az_expf(lg[a] - mx); p[a] = v; se += v; }
  float S = 0.0f;
  for (int a = 0; a < A; ++a) { const float v = p[a] / se; p[a] = v; S += v * am[a]; }
  const float w = W[i];
  const float den = S + eps;
  double kl = 0.0;
  float gu_sum = 0.0f;
  for (int a = 0; a < A; ++a) {
    const float u = p[a] * am[a], q = u / den, Pa = pt[a];
    kl += (double)(Pa * az_logf(q + eps) * w);
    gu_sum += (-Pa / (q + eps)) * u;
  }
  gu_sum = gu_sum / (den * den);
  auto dp_of = [&](int a) {
    const float u = p[a] * am[a], q = u / den, gq = -pt[a] / (q + eps);
    return am[a] * (gq / den - gu_sum - cinv) * w * gscale;
  };
  float dot = 0.0f;
  for (int a = 0; a < A; ++a) dot += p[a] * dp_of(a);
  for (int a = 0; a < A; ++a) p[a] = p[a] * (dp_of(a) - dot);
  const float vh = az_tanhf(tpre[i]);
  const float d = vh / rho - V[i] / rho;
  dt[i] = 2.0f * d / rho * (1.0f - vh * vh) * w * gscale;
  t_w[i] = (double)w; t_kl[i] = kl; t_mse[i] = (double)(d * d * w); t_inv[i] = (double)((1.0f - S) * w);
}
// the five sums of a step in one launch: out = (sum w, sum kl, sum mse, sum inv, sum of squares of the trainables)
__global__ void __launch_bounds__(256) k_tr_step_sums(const double* __restrict__ tw, const double* __restrict__ tkl, const double* __restrict__ tmse,
                                                      const double* __restrict__ tinv, int B, const double* __restrict__ ssq_part, int nssq,
                                                      double* __restrict__ out) {
  __shared__ double sh[5][256];
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < B; i += 256) { a[0] += tw[i]; a[1] += tkl[i]; a[2] += tmse[i]; a[3] += tinv[i]; }
  for (int i = threadIdx.x; i < nssq; i += 256) a[4] += ssq_part[i];
#pragma unroll
  for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 5) out[threadIdx.x] = sh[threadIdx.x][0];
}
// Adam (Optimisers.Adam: beta (0.9, 0.999), eps 1e-8) / Nesterov (Optimisers.Nesterov) on the trainable entries of
// the blob; the L2 term of the loss, scale * creg * sum(w^2), is added to the gradient here: + scale * 2 creg w.
__global__ void k_tr_adam(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                          const unsigned char* __restrict__ trainable, long long n, float lr, float b1t, float b2t,
                          const double* __restrict__ sums, float reg_c /* 2 creg / (B Wmean) */) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !trainable[i]) return;
  const float reg2 = (float)sums[0] * reg_c;                       // scale * 2 creg, scale = mean(W_batch) / Wmean
  const float gi = g[i] + reg2 * w[i];
  const float mt = 0.9f * m[i] + (1.0f - 0.9f) * gi;
  const float vt = 0.999f * v[i] + (1.0f - 0.999f) * gi * gi;
  m[i] = mt; v[i] = vt;
  w[i] -= mt / (1.0f - b1t) / (__builtin_sqrtf(vt / (1.0f - b2t)) + 1e-8f) * lr;
}
__global__ void k_tr_nesterov(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ vel,
                              const unsigned char* __restrict__ trainable, long long n, float lr, float rho,
                              const double* __restrict__ sums, float reg_c) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !trainable[i]) return;
  const float reg2 = (float)sums[0] * reg_c;
  const float gi = g[i] + reg2 * w[i];
  const float vo = vel[i];
  const float d = rho * rho * vo - (1.0f + rho) * lr * gi;         // Optimisers.Nesterov: newdx = -d
  vel[i] = rho * vo - lr * gi;
  w[i] += d;
}
__global__ void k_tr_sumsq(const float* __restrict__ w, const unsigned char* __restrict__ trainable, long long n, double* __restrict__ part) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) if (trainable[i]) s += (double)w[i] * (double)w[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k]; __syncthreads(); }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// ------------------------------------------------------------------------------------------ host
// One layer of a trainer's table: g = x Wm over `rows` rows (R = batch x positions for a convolution, the batch for a dense layer: the rows
// of one board are contiguous, so [R][nf] is [B][P nf] with k = p nf + f), then a = relu(bn(g) (+ skip's activation)) with batch statistics,
// or a = relu(g + b) in place (a == g), or a head's output g + b (no relu).  A convolution of the blob (net_layout.h ConvAt) or a Dense
// (+ BatchNorm) of it (the ResNet's pd / v1 / v2, DenseAt of a SimpleNet).
enum TrInput { TR_PLAIN,        // x = the activation of layer src as it lies (a 1x1 convolution, a dense layer; src = -1: the flattened planes)
               TR_IM2COL,       // x = col, the 3x3 neighbourhoods of the batch's planes (the stem: K = 9 C, im2col + GEMM)
               TR_MFMA };       // a tower F -> F convolution: forward and data gradient on k_conv16_layer, weight gradient on k_wgrad16
struct TrLayer {
  long long rows; int in, out, src;   // src: the layer whose activation is this layer's input, -1 = the batch's planes
  TrInput input;
  bool bn, relu;
  int skip;                     // the tower's second convolutions: the layer whose activation joins before the relu (the block input), else -1
  bool act_next;                // a is written by the next layer's convolution on its way in (BnIn), not by a launch of this layer
  size_t off_b, off_bn;         // blob offsets: bias, (gamma, beta, mean, var)
  size_t wk_wm;                 // offset in the working-parameter array: GEMM matrix [in][out]
  size_t wk_ffwd, wk_fdg;       // TR_MFMA: fragments of k_conv16_layer for forward / data gradient
  float *col, *g, *a, *da;      // im2col input [rows][in] (TR_IM2COL), GEMM output, activation, gradient with respect to the activation (the sum
                                // over the layer's consumers; becomes the gradient with respect to g in place)
  float *mean, *invstd;
};
struct az_trainer {               // every member starts here: az_trainer_destroy takes a half-built record apart
  az_engine* e = nullptr;
  az_dataset* d = nullptr;
  az_train_cfg cfg = {};
  int game = 0, device = 0; GameInfo gi = {};
  hipStream_t stream = nullptr;
  EnvTrainer env;                                                            // the AZHIP_TRAIN_* overrides, read when az_trainer_create constructs this record (env.h)
  hipStream_t side = nullptr;                                                // the weight gradients of the tower run here, beside the batch-norm backward passes of the next layer
  std::vector<hipEvent_t> ev_dg, ev_wg;                                     // per tower layer: output gradient ready / weight gradient done
  float* gemm_ws = nullptr; size_t gemm_ws_floats = 0;                       // split-reduction workspace of gemm_f32
  int B = 0, F = 0;
  long long R = 0;              // rows of a tower layer: batch x positions
  size_t nparams = 0;
  // ResNet: stem, 2 num_blocks tower layers, policy-head conv, value-head conv, pd, v1, v2.  SimpleNet: as SimpleLayout::dense (trunk, policy
  // head + Dense(h -> A), value head + Dense(h -> 1)).  Every layer comes after the layer it reads.
  std::vector<TrLayer> layers;
  int ntower = 0;               // the stem and the TR_MFMA layers at the front of the table; 0: a dense chain, the table has no convolution
  int ipol = 0, ival = 0;       // the layers whose g are the policy logits and the value pre-activation
  size_t nwork = 0;
  float *blob = nullptr, *gblob = nullptr, *opt_m = nullptr, *opt_v = nullptr; unsigned char* trainable = nullptr;   // [nparams]
  int* scat = nullptr; long long nscat = 0;                                  // working entries that carry a gradient (the primary ranges)
  float *work = nullptr, *gwork = nullptr; int* map = nullptr;               // working parameters and their blob map
  int* d_idx = nullptr; float *bW = nullptr, *bX = nullptr, *bA = nullptr, *bP = nullptr, *bV = nullptr;   // the batch
  float *dact = nullptr, *dact2 = nullptr, *dact3 = nullptr, *dcol = nullptr;   // [R][F] gradients (dcol / dact / dact3 take turns as the running gradient, dact2 = the skip share)
  float* wg_part = nullptr; int wg_splits = 0, wg_bpw = 0;       // k_wgrad16: partial dW per row split, boards per workgroup
  double *part = nullptr, *sums = nullptr, *terms = nullptr, *bsums = nullptr;
  size_t npart = 0; int wsum = 0, wbn = 0;                                   // what trainer_build sized them for: part [npart], sums [2][wsum], bn_mf [2][wbn]
  float* bn_mf = nullptr;                                                    // [2][C] the batch-norm backward means of the layer in flight
  int* fin_counter = nullptr;                                                // tr_finish: counter of the workgroups that have left their partial sums
  std::vector<void*> allocs;
  std::vector<int> perm; int64_t perm_pos = 0, epoch = 0; int64_t step = 0;
  float b1t = 1.0f, b2t = 1.0f;
};

template <class T> static int tr_alloc(az_trainer* t, T** p, size_t n, bool zero = false) {
  AZCHK(mem_alloc(&t->allocs, p, n));
  if (zero) HIPCHK(hipMemsetAsync(*p, 0, std::max<size_t>(n * sizeof(T), 16), t->stream));
  return AZ_OK;
}
static inline unsigned tr_grid(long long n) { return (unsigned)((n + 255) / 256); }
static int tr_gemm(az_trainer* t, bool ta, bool tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B, int ldb,
                   float beta, float* C, int ldc) {
  gemm_f32(t->stream, t->gemm_ws, t->gemm_ws_floats, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
  return AZ_OK;
}

extern "C" int az_train_cfg_init(az_train_cfg* c) {
  if (!c) return fail(AZ_ERR_BAD_ARG, "cfg is NULL");
  memset(c, 0, sizeof *c);
  c->struct_size = (int32_t)sizeof *c;
  c->optimiser = AZ_OPT_ADAM; c->lr = 2e-3f;                       // games/connect-four/params.jl:46-58
  c->lr_base = 1e-3f; c->lr_high = 1e-2f; c->lr_low = 1e-3f; c->momentum_low = 0.8f; c->momentum_high = 0.9f;
  c->l2_regularization = 1e-4; c->nonvalidity_penalty = 1.0; c->rewards_renormalization = 1.0;
  c->batch_size = 1024; c->batch_norm_momentum = 0.1f; c->seed = 1;
  return AZ_OK;
}

extern "C" int az_trainer_destroy(az_trainer* t) {
  if (!t) return AZ_OK;
  (void)hipSetDevice(t->device);
  for (void* p : t->allocs) (void)hipFree(p);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  if (t->side) { (void)hipStreamSynchronize(t->side); (void)hipStreamDestroy(t->side); }
  for (hipEvent_t ev : t->ev_dg) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : t->ev_wg) (void)hipEventDestroy(ev);
  if (t->stream) (void)hipStreamDestroy(t->stream);
  delete t;
  return AZ_OK;
}

// the parameter arrays: the blob with its gradient, the optimiser's state and the trainable mask; the working parameters with their blob map
// (net_layout.h: work[j] = blob[map[j]]) and the working entries that carry a gradient back (scat)
static int tr_upload_params(az_trainer* t, const IndexMap& map, const IndexMap& scat, const std::vector<unsigned char>& trainable) {
  const size_t wk = map.size();
  t->nwork = wk; t->nscat = (long long)scat.size();
  AZCHK(tr_alloc(t, &t->scat, scat.size()));
  AZCHK(tr_alloc(t, &t->map, wk)); AZCHK(tr_alloc(t, &t->work, wk)); AZCHK(tr_alloc(t, &t->gwork, wk, true));
  AZCHK(tr_alloc(t, &t->blob, t->nparams)); AZCHK(tr_alloc(t, &t->gblob, t->nparams, true));
  AZCHK(tr_alloc(t, &t->opt_m, t->nparams, true)); AZCHK(tr_alloc(t, &t->opt_v, t->nparams, true));
  AZCHK(tr_alloc(t, &t->trainable, t->nparams));
  HIPCHK(hipMemcpyAsync(t->scat, scat.data(), sizeof(int) * scat.size(), hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(t->map, map.data(), sizeof(int) * wk, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(t->trainable, trainable.data(), t->nparams, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(t->blob, t->e->blob.data(), sizeof(float) * t->nparams, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));                         // the host vectors go out of scope
  return AZ_OK;
}

// builds the layer table, the parameter maps and the buffers
static int trainer_build(az_trainer* t) {
  const GameInfo& gi = t->gi;
  const int B = t->B, F = t->F, A = gi.A, P = gi.P;
  const long long R = t->R;
  auto add = [&](long long rows, int in, int out, int src, TrInput input, bool bn, bool relu, size_t off_b, size_t off_bn, size_t wk_wm) -> TrLayer& {
    TrLayer c{};
    c.rows = rows; c.in = in; c.out = out; c.src = src; c.input = input; c.bn = bn; c.relu = relu; c.skip = -1;
    c.off_b = off_b; c.off_bn = off_bn; c.wk_wm = wk_wm;
    t->layers.push_back(c);
    return t->layers.back();
  };
  if (t->e->cfg.oracle == AZ_ORACLE_SIMPLENET) {                     // the dense chain and its working matrices (net_layout.h SimpleTrainMaps)
    const SimpleLayout lay = simple_layout(gi, t->e->shp);
    const SimpleTrainMaps tm(lay);
    for (size_t l = 0; l < lay.dense.size(); ++l) {
      const DenseAt& at = lay.dense[l];
      const int src = l == 0 ? -1 : ((int)l == lay.pfirst() || (int)l == lay.vfirst()) ? lay.ncommon() - 1 : (int)l - 1;   // each head starts from the trunk
      add(B, at.in, at.out, src, TR_PLAIN, at.bn, !at.last, at.b, at.bnv, tm.wm[l]);
    }
    t->ipol = lay.vfirst() - 1; t->ival = (int)lay.dense.size() - 1;
    AZCHK(tr_upload_params(t, tm.map, tm.scat, trainable_mask(lay)));
  } else {
    const NetLayout lay = net_layout(gi, t->e->cfg);
    const TrainMaps tm(lay);                                          // net_layout.h: the working parameters and where each comes from
    const int ntower = 1 + lay.ntower(), hp = ntower, hv = ntower + 1;
    t->ntower = ntower;
    // tr_forward_backward takes the input of every MFMA layer from the layer below (tr_bn_in) and the stem's from the batch's planes:
    // the stem is the one non-MFMA tower layer, whatever its plane count.
    for (int l = 0; l < (int)lay.conv.size(); ++l) {
      const ConvAt& at = lay.conv[l];
      const bool tower = l >= 1 && l < ntower;                       // the tower's F -> F convolutions (F = 64 or 128: az_engine_create): MFMA layer kernels
      TrLayer& c = add(R, at.taps() * at.cin, at.cout, l == 0 ? -1 : tower ? l - 1 : ntower - 1, l == 0 ? TR_IM2COL : tower ? TR_MFMA : TR_PLAIN, true, true,
                       at.b, at.bn, tm.conv[l].wm);
      c.wk_ffwd = tm.conv[l].ffwd; c.wk_fdg = tm.conv[l].fdg;
      if (tower && l % 2 == 0) c.skip = l - 2;                       // conv2 of a block: skip connection from the block input
      c.act_next = l + 1 < ntower;
    }
    add(B, P * lay.s.npf, A, hp, TR_PLAIN, false, false, lay.pd_b, 0, tm.pd);
    add(B, P * lay.s.nvf, F, hv, TR_PLAIN, false, true, lay.v1_b, 0, tm.v1);
    add(B, F, 1, hv + 2, TR_PLAIN, false, false, lay.v2_b, 0, tm.v2);
    t->ipol = hv + 1; t->ival = hv + 3;
    AZCHK(tr_upload_params(t, tm.map, tm.scat, trainable_mask(lay)));
    // The gradients of the convolutions share four [R][F] buffers.  The running gradient of the tower moves through a ring of three, from the
    // trunk (where both head convolutions leave their share) down: the MFMA data-gradient convolution writes out of place (see the tower
    // block of tr_forward_backward for why three).  The head convolutions' own gradients, [R][npf] and [R][nvf], lie in dact and dact2 until
    // the tower's backward pass starts; from then on dact2 is the skip share.
    AZCHK(tr_alloc(t, &t->dact, (size_t)R * F)); AZCHK(tr_alloc(t, &t->dact2, (size_t)R * F)); AZCHK(tr_alloc(t, &t->dact3, (size_t)R * F)); AZCHK(tr_alloc(t, &t->dcol, (size_t)R * F));
    float* ring[3] = {t->dcol, t->dact, t->dact3};
    for (int l = 0; l < ntower; ++l) t->layers[l].da = ring[(ntower - 1 - l) % 3];
    t->layers[hp].da = t->dact; t->layers[hv].da = t->dact2;
    for (int l = 0; l < ntower; ++l) {
      hipEvent_t a = nullptr, b = nullptr;
      HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming)); t->ev_dg.push_back(a);
      HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableTiming)); t->ev_wg.push_back(b);
    }
    // k_wgrad16: one round of workgroups over the chip
    const int tg = F == 128 ? 3 : 1, per_cu = 1;                      // 82 KB (64 filters) / 145 KB (128) of LDS: one workgroup per CU either way
    // as many workgroups per tap group as the chip holds (one round), the boards spread evenly over them: 1024 boards at
    // 128 filters = 85 workgroups x 3 tap groups with 12 or 13 boards each (whole 3-board LDS chunks per workgroup made it
    // 69 x 3 workgroups with 15 boards: a fifth of the CUs idle and a fifth chunk for everyone)
    t->wg_splits = std::max(1, std::min(B, t->e->num_cu * per_cu / tg));
    t->wg_bpw = (B + t->wg_splits - 1) / t->wg_splits;
    AZCHK(tr_alloc(t, &t->wg_part, (size_t)t->wg_splits * 9 * F * F));
  }
  // per layer: its buffers, and what it asks of the scratch the column sums share: part [partials][2][columns]; sums [2][the widest column
  // sum] (also the policy bias gradient, A columns: 82 on a 9x9 board); bn_mf [2][the widest hidden layer] (those can carry a batch norm)
  size_t npart = 0;
  int wsum = 64, wbn = 64;
  for (TrLayer& c : t->layers) {
    const size_t n = (size_t)c.rows * c.out;
    if (c.input == TR_IM2COL) AZCHK(tr_alloc(t, &c.col, (size_t)c.rows * c.in));
    AZCHK(tr_alloc(t, &c.g, n));
    if (c.bn) { AZCHK(tr_alloc(t, &c.a, n)); AZCHK(tr_alloc(t, &c.mean, c.out)); AZCHK(tr_alloc(t, &c.invstd, c.out)); }
    else c.a = c.g;                                                   // bias and relu act in place
    if (!c.da) AZCHK(tr_alloc(t, &c.da, n));                          // (a ResNet's convolutions: the shared buffers above)
    long long parts = (c.rows + TR_CHUNK - 1) / TR_CHUNK;            // chunks of k_tr_colsum ...
    if (c.input != TR_PLAIN) parts = std::max<long long>(parts, B + 1);   // ... or workgroups of k_conv16_layer (the stem alike: the scratch does not depend on the depth)
    npart = std::max(npart, (size_t)parts * 2 * std::max(c.out, 64));
    wsum = std::max(wsum, c.out);
    if (c.relu) wbn = std::max(wbn, c.out);
  }
  AZCHK(tr_alloc(t, &t->d_idx, B)); AZCHK(tr_alloc(t, &t->bW, B)); AZCHK(tr_alloc(t, &t->bV, B));
  AZCHK(tr_alloc(t, &t->bX, (size_t)B * gi.C * P)); AZCHK(tr_alloc(t, &t->bA, (size_t)B * A)); AZCHK(tr_alloc(t, &t->bP, (size_t)B * A));
  AZCHK(tr_alloc(t, &t->part, npart));
  AZCHK(tr_alloc(t, &t->sums, (size_t)2 * wsum)); AZCHK(tr_alloc(t, &t->bn_mf, (size_t)2 * wbn));
  t->npart = npart; t->wsum = wsum; t->wbn = wbn;
  AZCHK(tr_alloc(t, &t->fin_counter, 4, true));                       // tr_finish: workgroups done (every launch leaves it at zero)
  AZCHK(tr_alloc(t, &t->terms, (size_t)4 * B)); AZCHK(tr_alloc(t, &t->bsums, 8 + 1024));
  return AZ_OK;
}

template <class Gm, int F, bool STATS, int NT> static int tr_conv16_f(az_trainer* t, const float* in, const float* frag, float* out, const float* addend, const BnIn& bn, const TrFinal& fin) {
  using T = T16<Gm, F, NT>;
  static bool attr_done = false;
  if (!attr_done) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv16_layer<Gm, F, STATS, false, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, T::BYTES)); attr_done = true; }
  hipLaunchKernelGGL((k_conv16_layer<Gm, F, STATS, false, NT>), dim3((t->B + T::TB - 1) / T::TB), dim3(T::THREADS), T::BYTES, t->stream, in, (const float4*)frag, out, t->B, t->e->d_geo[T::GEO], t->part, addend, (long long*)nullptr, bn, fin);
  return AZ_OK;
}
// 3x3 F -> F convolution of [R][F] activations on the MFMA layer kernel; stats: also the first stage of the column sums
// (sum, sum of squares) of the output in t->part, *nparts workgroup partials
static int tr_conv16(az_trainer* t, const float* in, const float* frag, float* out, bool stats = false, int* nparts = nullptr, const float* addend = nullptr,
                     const BnIn& bn = BnIn{}, const TrFinal& fin = TrFinal{}) {
  DISPATCH_GEOMETRY(t->game, {
    using T = T16<Gm, 64, 11>;
    using T6 = T16<Gm, 64, 6>;
    // (r4) 64 filters and a batch that gives the 11-tile form at most one workgroup per CU: the 6-tile form (half the boards per
    // workgroup, two workgroups per CU) overlaps one workgroup's fill and epilogue with the other's products
    const bool small = t->F == 64 && t->env.conv_nt6 && (t->B + T::TB - 1) / T::TB <= cus(t->e->num_cu);
    if (nparts) *nparts = small ? (t->B + T6::TB - 1) / T6::TB : (t->B + T::TB - 1) / T::TB;
    if (t->F == 128) { if (stats) AZCHK((tr_conv16_f<Gm, 128, true, 11>(t, in, frag, out, addend, bn, fin))); else AZCHK((tr_conv16_f<Gm, 128, false, 11>(t, in, frag, out, addend, bn, fin))); }
    else if (small) { if (stats) AZCHK((tr_conv16_f<Gm, 64, true, 6>(t, in, frag, out, addend, bn, fin))); else AZCHK((tr_conv16_f<Gm, 64, false, 6>(t, in, frag, out, addend, bn, fin))); }
    else { if (stats) AZCHK((tr_conv16_f<Gm, 64, true, 11>(t, in, frag, out, addend, bn, fin))); else AZCHK((tr_conv16_f<Gm, 64, false, 11>(t, in, frag, out, addend, bn, fin))); }
  });
  return AZ_OK;
}

template <class Gm, int F> static int tr_wgrad16_f(az_trainer* t, const float* a, const float* dg, float* out, hipStream_t st) {
  // 128 filters: the 4-wavefront form (half the input channels per workgroup, one board per LDS chunk, 44 KB): the same sums in
  // the same order as the 8-wavefront form, and a workgroup of it fits on a CU beside one of k_conv16_layer
  // A board of more than 64 positions (9x9: 81) is a chunk by itself: RPC = its rows rounded up to whole tiles (96), not the 128 rows of
  // the three-board chunk, which would carry 47 padding rows through HBM loads and LDS for every board; at 128 filters with the input
  // channels split in two as well (86 KB of LDS; the 8-wavefront form would take 110 KB at 96 rows and 146 KB at 128).  DESIGN.md 4e.
  constexpr bool BIG = Gm::P > 64;
  constexpr int CS = (F == 128 && (Gm::P <= 48 || BIG)) ? 2 : 1, RPC = BIG ? (Gm::P + 15) / 16 * 16 : CS == 2 ? 48 : 128;
  using G = WG16<F, CS, RPC>;
  static bool attr_done = false;
  if (!attr_done) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wgrad16<Gm, F, 0, CS, RPC>), hipFuncAttributeMaxDynamicSharedMemorySize, G::BYTES)); attr_done = true; }
  hipLaunchKernelGGL((k_wgrad16<Gm, F, 0, CS, RPC>), dim3(t->wg_splits, G::TG * CS), dim3(G::THREADS), G::BYTES, st, a, dg, t->wg_part, t->B, t->wg_splits, (long long*)nullptr);
  const long long n = 9LL * F * F;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(tr_grid(n / 2)), dim3(256), 0, st, t->wg_part, t->wg_splits, n, out);
  return AZ_OK;
}
// weight gradient of a 3x3 F -> F convolution on the MFMA kernel: out = [9][F][F] in the Wm layout
static int tr_wgrad16(az_trainer* t, const float* a, const float* dg, float* out, hipStream_t st) {
  DISPATCH_GEOMETRY(t->game, { if (t->F == 128) AZCHK((tr_wgrad16_f<Gm, 128>(t, a, dg, out, st))); else AZCHK((tr_wgrad16_f<Gm, 64>(t, a, dg, out, st))); });
  return AZ_OK;
}

static void tr_bn_bwd(az_trainer* t, const float* da, const float* a, const float* g, const float* mean, const float* invstd, const float* gamma,
                      long long n, int C, float* dg, float* dy_out) {
  if (C % 4 == 0) hipLaunchKernelGGL((k_tr_bn_bwd<4>), dim3(tr_grid(n / 2)), dim3(256), 0, t->stream, da, a, g, mean, invstd, gamma, t->bn_mf, n, C, dg, dy_out);
  else hipLaunchKernelGGL((k_tr_bn_bwd<1>), dim3(tr_grid(n)), dim3(256), 0, t->stream, da, a, g, mean, invstd, gamma, t->bn_mf, n, C, dg, dy_out);
}
// column sums of mode MODE over R rows, result in t->sums.  ran (debug seam): what was launched -- chunks, 1 if k_tr_colsum1v, 1 if the second
// stage rides in the producer, column blocks (gridDim.y)
template <int MODE>
static int tr_colsum(az_trainer* t, const float* x, const float* out_act, const float* g, const float* mean, const float* invstd, long long R, int C,
                     TrFinal fin = TrFinal{}, int32_t* ran = nullptr) {
  const int nchunks = (int)((R + TR_CHUNK - 1) / TR_CHUNK);
  // (tr_finish -- the second stage in the producer's last workgroup -- is off: measured slower, see k_tr_colsum_final)
  const bool inside = t->env.fin_inside && C <= 128;
  fin.counter = inside ? t->fin_counter : nullptr;
  const bool vec = MODE == 1 && C % 4 == 0 && C <= 128 && 256 % (C / 4) == 0;
  const dim3 grid(nchunks, vec ? 1 : (C + 63) / 64);
  if (vec) hipLaunchKernelGGL(k_tr_colsum1v, grid, dim3(256), 0, t->stream, x, out_act, g, mean, invstd, R, C, t->part, fin);
  else hipLaunchKernelGGL((k_tr_colsum<MODE>), grid, dim3(256), 0, t->stream, x, out_act, g, mean, invstd, R, C, t->part, fin);
  if (ran) { ran[0] = nchunks; ran[1] = vec; ran[2] = inside; ran[3] = (int32_t)grid.y; }
  if (!inside) hipLaunchKernelGGL(k_tr_colsum_final, dim3(C), dim3(64), 0, t->stream, t->part, nchunks, C, t->sums, fin);
  return AZ_OK;
}

// what k_tr_colsum_final / tr_finish do with a layer's column sums.  Forward: (sum, sum of squares) of g over the layer's rows -> batch mean,
// biased variance, running statistics.  The bias before a train-mode batch norm cancels in the normalised value (the batch mean absorbs
// it); it moves the running mean only (TrFinal::bias).
static TrFinal tr_fin_stats(const az_trainer* t, const TrLayer& c) {
  TrFinal fin{}; fin.mode = 1; fin.R = c.rows; fin.momentum = t->cfg.batch_norm_momentum; fin.bias = t->blob + c.off_b; fin.mean = c.mean; fin.invstd = c.invstd;
  fin.run_mean = t->blob + c.off_bn + 2 * c.out; fin.run_var = t->blob + c.off_bn + 3 * c.out;
  return fin;
}
// backward: (sum dy, sum dy xhat) -> dbeta, dgamma in the gradient blob and the two means k_tr_bn_bwd subtracts (bn_mf)
static TrFinal tr_fin_bn_bwd(const az_trainer* t, const TrLayer& c) {
  TrFinal fin{}; fin.mode = 2; fin.R = c.rows; fin.mf = t->bn_mf; fin.dgamma = t->gblob + c.off_bn; fin.dbeta = t->gblob + c.off_bn + c.out;
  return fin;
}
// what turns g into a: for the convolution above to apply on its way in (BnIn), or for tr_layer_act
static BnIn tr_bn_in(const az_trainer* t, const TrLayer& c) {
  return BnIn{c.g, c.mean, c.invstd, t->blob + c.off_bn, t->blob + c.off_bn + c.out, c.skip >= 0 ? t->layers[c.skip].a : nullptr, c.a};
}
// a = relu(bn(g) (+ res)) over n = rows x C elements / x = [relu](x + bias) in place / the relu mask of the way back, in place
static void tr_bn_apply(az_trainer* t, const BnIn& b, long long n, int C) {
  hipLaunchKernelGGL(k_tr_bn_apply, dim3(tr_grid(n)), dim3(256), 0, t->stream, b.g, b.mean, b.invstd, b.gamma, b.beta, b.res, n, C, b.a_out);
}
static void tr_bias_act(az_trainer* t, float* x, const float* bias, long long n, int C, bool relu) {
  hipLaunchKernelGGL(k_tr_bias_act, dim3(tr_grid(n)), dim3(256), 0, t->stream, x, bias, n, C, relu ? 1 : 0);
}
static void tr_relu_bwd(az_trainer* t, float* dy, const float* y, long long n) {
  hipLaunchKernelGGL(k_tr_relu_bwd, dim3(tr_grid(n)), dim3(256), 0, t->stream, dy, y, n);
}
static void tr_layer_act(az_trainer* t, const TrLayer& c) {
  const long long n = c.rows * c.out;
  if (c.bn) tr_bn_apply(t, tr_bn_in(t, c), n, c.out);
  else tr_bias_act(t, c.g, t->blob + c.off_b, n, c.out, c.relu);
}
// the stem's gather: col[rows][9 C] = the 3x3 neighbourhoods of the planes [B][C][H][W]
static void tr_im2col(az_trainer* t, const float* planes, const TrLayer& c) {
  hipLaunchKernelGGL((k_tr_im2col<true>), dim3(tr_grid(c.rows * c.in)), dim3(256), 0, t->stream, planes, c.rows, c.in / 9, t->gi.W, t->gi.H, c.col);
}
// the loss of the batch in bA / bP / bV / bW with its gradient, per-sample terms in t->terms; force_wide: k_tr_loss_wide whatever A
// (debug seam: the two kernels on the same inputs).  Returns whether the wide kernel ran.
static bool tr_loss(az_trainer* t, const float* logits, const float* tpre, float cinv, float rho, float gscale, float* dlogits, float* dt, bool force_wide) {
  const int A = t->gi.A, B = t->B;
  hipStream_t st = t->stream;
  double *tw = t->terms, *tkl = t->terms + B, *tmse = t->terms + 2 * (size_t)B, *tinv = t->terms + 3 * (size_t)B;
  const bool wide = force_wide || A > AZ_MAX_ACTIONS;
  if (!wide)
    hipLaunchKernelGGL(k_tr_loss, dim3(tr_grid(B)), dim3(256), 0, st, logits, tpre, t->bA, t->bP, t->bV, t->bW, B, A, cinv, rho, gscale, dlogits, dt, tw, tkl, tmse, tinv);
  else                                                              // 64 threads per workgroup: the rows of a wavefront's samples are 4 A bytes apart, so more CUs share the strided reads
    hipLaunchKernelGGL(k_tr_loss_wide, dim3((B + 63) / 64), dim3(64), 0, st, logits, tpre, t->bA, t->bP, t->bV, t->bW, B, A, cinv, rho, gscale, dlogits, dt, tw, tkl, tmse, tinv);
  return wide;
}
// the five sums of a step: the per-sample terms and the sum of squares of the trainable parameters
static void tr_step_sums(az_trainer* t, double* d_sums) {
  const int B = t->B;
  hipLaunchKernelGGL(k_tr_sumsq, dim3(1024), dim3(256), 0, t->stream, t->blob, t->trainable, (long long)t->nparams, t->bsums + 8);
  hipLaunchKernelGGL(k_tr_step_sums, dim3(1), dim3(256), 0, t->stream, t->terms, t->terms + B, t->terms + 2 * (size_t)B, t->terms + 3 * (size_t)B, B, t->bsums + 8, 1024, d_sums);
}
static const float* tr_input(const az_trainer* t, const TrLayer& c) {   // TR_PLAIN on the planes: flatten = their memory order
  return c.input == TR_IM2COL ? c.col : c.src < 0 ? t->bX : t->layers[c.src].a;
}
// every layer but the tower's MFMA convolutions: the GEMM, then batch statistics + k_tr_bn_apply, or k_tr_bias_act
static int gemm_layer_forward(az_trainer* t, TrLayer& c) {
  if (c.input == TR_IM2COL) tr_im2col(t, t->bX, c);
  AZCHK(tr_gemm(t, false, false, (int)c.rows, c.out, c.in, 1.f, tr_input(t, c), c.in, t->work + c.wk_wm, c.out, 0.f, c.g, c.out));
  if (c.bn) AZCHK(tr_colsum<0>(t, c.g, nullptr, nullptr, nullptr, nullptr, c.rows, c.out, tr_fin_stats(t, c)));
  if (!c.act_next) tr_layer_act(t, c);
  return AZ_OK;
}
// ... backward: da -> dg in place (batch-norm backward with dgamma / dbeta, or the relu mask and the bias gradient), the weight gradient,
// and the data gradient into the producer's da -- written by its first consumer, added to by a second (accumulate)
static int gemm_layer_backward(az_trainer* t, TrLayer& c, bool accumulate) {
  const long long n = c.rows * c.out;
  float* dg = c.da;
  if (c.bn) {
    AZCHK(tr_colsum<1>(t, dg, c.a, c.g, c.mean, c.invstd, c.rows, c.out, tr_fin_bn_bwd(t, c)));
    tr_bn_bwd(t, dg, c.a, c.g, c.mean, c.invstd, t->blob + c.off_bn, n, c.out, dg, nullptr);
    // the bias of a layer that feeds a train-mode BatchNorm has gradient sum(dg) = gamma invstd (sum dy - R m0 - m1 sum xhat)
    // = 0 exactly (the batch mean absorbs it): its slot in gblob stays 0 and only the L2 term moves it
  } else {
    if (c.relu) tr_relu_bwd(t, dg, c.a, n);
    TrFinal fin{}; fin.mode = 3; fin.out0 = t->gblob + c.off_b;
    AZCHK(tr_colsum<2>(t, dg, nullptr, nullptr, nullptr, nullptr, c.rows, c.out, fin));
  }
  AZCHK(tr_gemm(t, true, false, c.in, c.out, (int)c.rows, 1.f, tr_input(t, c), c.in, dg, c.out, 0.f, t->gwork + c.wk_wm, c.out));
  if (c.src >= 0) AZCHK(tr_gemm(t, false, true, (int)c.rows, c.in, c.out, 1.f, dg, c.out, t->work + c.wk_wm, c.out, accumulate ? 1.f : 0.f, t->layers[c.src].da, c.in));
  return AZ_OK;
}

// forward (train mode) + loss + backward for the batch idx[0..B); the gradient of the DATA terms is left in t->gblob
// (blob layout, L2 term not included); the step's five sums (w, kl, mse, inv, sum of squares) go to d_sums (device).
// Nothing here waits for the GPU: idx_host must stay alive until the stream has consumed it.
// A ResNet in TRAIN mode (resnet.jl:53-92) and a SimpleNet (simplenet.jl:37-64) alike: the table says which layers there are.
static int tr_forward_backward(az_trainer* t, const int* idx_host, double* d_sums) {
  const GameInfo& gi = t->gi;
  const int A = gi.A, B = t->B, ntower = t->ntower, nlayers = (int)t->layers.size();
  const long long R = t->R;
  hipStream_t st = t->stream;
  az_dataset* d = t->d;
  float* blob = t->blob;
  HIPCHK(hipMemcpyAsync(t->d_idx, idx_host, sizeof(int) * B, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_tr_batch, dim3(B), dim3(64), 0, st, t->d_idx, B, gi.C * gi.P, A, d->d_W, d->d_X, d->d_A, d->d_P, d->d_V, t->bW, t->bX, t->bA, t->bP, t->bV);
  hipLaunchKernelGGL(k_tr_gather, dim3(tr_grid((long long)t->nwork)), dim3(256), 0, st, blob, t->map, (long long)t->nwork, t->work);
  HIPCHK(hipMemsetAsync(t->gblob, 0, sizeof(float) * t->nparams, st));
  // ---------------- forward ----------------
  for (TrLayer& c : t->layers) {
    if (c.input != TR_MFMA) { AZCHK(gemm_layer_forward(t, c)); continue; }
    // (r4) one launch per tower layer: the convolution of layer l computes its INPUT a(l-1) = relu(bn(g(l-1)) (+ skip)) while the rows
    // go into LDS (BnIn, and writes it for the backward pass), leaves the column sums of its output and its last workgroup turns them
    // into the layer's batch statistics (tr_finish).  Were three launches (convolution, k_tr_colsum_final, k_tr_bn_apply).
    int nparts = 0;
    TrFinal fin = tr_fin_stats(t, c);
    fin.counter = t->env.fin_inside ? t->fin_counter : nullptr;
    AZCHK(tr_conv16(t, nullptr, t->work + c.wk_ffwd, c.g, true, &nparts, nullptr, tr_bn_in(t, t->layers[c.src]), fin));
    if (!fin.counter) hipLaunchKernelGGL(k_tr_colsum_final, dim3(c.out), dim3(64), 0, st, t->part, nparts, c.out, t->sums, fin);
    if (!c.act_next) tr_layer_act(t, c);                             // the trunk: the last layer's activation has no convolution after it to ride in
  }
  TrLayer& pol = t->layers[t->ipol];
  TrLayer& val = t->layers[t->ival];
  // ---------------- loss ----------------
  // mean(W)/Wmean / sum(W) = 1 / (B Wmean): the gradient scale needs no reduction first (learning.jl:88)
  tr_loss(t, pol.g, val.g, (float)t->cfg.nonvalidity_penalty, (float)t->cfg.rewards_renormalization, 1.0f / ((float)B * d->Wmean), pol.da, val.da, false);
  tr_step_sums(t, d_sums);
  // ---------------- backward ----------------
  // The layers in reverse: every consumer of an activation comes before its producer, so da is complete when its layer's turn comes.
  // The trunk's last activation has two consumers (the heads): the first writes its da, the second adds to it.
  float* gw = t->gwork;
  std::vector<char> written(t->layers.size(), 0);
  for (int l = nlayers - 1; l >= 0; --l) {
    TrLayer& c = t->layers[l];
    if (c.input != TR_MFMA) {
      AZCHK(gemm_layer_backward(t, c, c.src >= 0 && written[c.src]));
      if (c.src >= 0) written[c.src] = 1;
      continue;
    }
    // The tower.  da = gradient w.r.t. the activation c.a; dskip (block input share) in dact2.  The MFMA data-gradient convolution
    // writes out of place, so the running gradient moves through three buffers (the front of the big scratch, where the head
    // convolutions left the trunk gradient, dact and dact3: the da of the table) instead of being copied.
    // (r3) The weight gradient of a layer is off the chain dg(l) -> da(l-1) -> dg(l-1): it runs on a second stream, so the
    // HBM-bound batch-norm backward passes of layer l-1 share the chip with the MFMA-bound k_wgrad16 of layer l.  Three
    // buffers because the data-gradient convolution of layer l-1 must not overwrite the dg that k_wgrad16 of layer l still
    // reads: it writes the buffer last read by the weight gradient of layer l+1 and waits for that one only.
    float* da = c.da;
    AZCHK(tr_colsum<1>(t, da, c.a, c.g, c.mean, c.invstd, R, c.out, tr_fin_bn_bwd(t, c)));
    // dg overwrites da; for conv2 the masked gradient dy also flows to the block input (dact2)
    tr_bn_bwd(t, da, c.a, c.g, c.mean, c.invstd, blob + c.off_bn, R * c.out, c.out, da, c.skip >= 0 ? t->dact2 : nullptr);
    if (!t->env.wg_late) HIPCHK(hipEventRecord(t->ev_dg[l], st));    // dg(l) is ready: the weight gradient may start beside the data gradient
    // data gradient da_prev = conv(dg, mirrored taps, ci <-> co): the same MFMA layer kernel with the wk_fdg fragments, out of place
    const bool first_of_block = (l % 2) == 1;                        // conv1: its input is the block input, which also gets the skip share
    if (l + 2 < ntower) HIPCHK(hipStreamWaitEvent(st, t->ev_wg[l + 2], 0));   // the weight gradient that last read the buffer about to be written
    AZCHK(tr_conv16(t, da, t->work + c.wk_fdg, t->layers[c.src].da, false, nullptr, first_of_block ? t->dact2 : nullptr));   // (r3) the add rides in the epilogue
    // the weight gradient starts when the data gradient of its layer is done: two MFMA kernels side by side only halve each
    // other's share of the chip (measured), while the HBM-bound passes of layer l-1 do fit beside k_wgrad16
    if (t->env.wg_late) HIPCHK(hipEventRecord(t->ev_dg[l], st));
    if (!t->env.one_stream) HIPCHK(hipStreamWaitEvent(t->side, t->ev_dg[l], 0));
    AZCHK(tr_wgrad16(t, t->layers[c.src].a, da, gw + c.wk_wm, t->env.one_stream ? st : t->side));
    HIPCHK(hipEventRecord(t->ev_wg[l], t->env.one_stream ? st : t->side));
  }
  for (int l = 1; l < ntower && l <= 2; ++l) HIPCHK(hipStreamWaitEvent(st, t->ev_wg[l], 0));   // the side stream is in order: its last two launches
  // working-layout weight gradients -> blob layout (the rotated copies carry no gradient of their own: their slots in
  // gwork stay zero and map to the same blob entries, so scatter only the primary ranges)
  hipLaunchKernelGGL(k_tr_scatter, dim3(tr_grid(t->nscat)), dim3(256), 0, st, gw, t->map, t->scat, t->nscat, t->gblob);
  return AZ_OK;
}

// `losses` from the five sums of a step (learning.jl:67-90): L and (Lp, Lv, Lreg, Linv, mean(W)/Wmean)
static void tr_losses(const az_trainer* t, const double* sums, float* L, float* parts) {
  const double sw = sums[0];
  const float scale = (float)(sw / (double)t->B) / t->d->Wmean;
  const float Lp = (float)(-sums[1] / sw) - t->d->Hp;
  const float Lv = (float)(sums[2] / sw);
  const float Lreg = t->cfg.l2_regularization == 0.0 ? 0.f : (float)((double)(float)t->cfg.l2_regularization * sums[4]);
  const float Linv = t->cfg.nonvalidity_penalty == 0.0 ? 0.f : (float)t->cfg.nonvalidity_penalty * (float)(sums[3] / sw);
  *L = scale * (Lp + Lv + Lreg + Linv);
  if (parts) { parts[0] = Lp; parts[1] = Lv; parts[2] = Lreg; parts[3] = Linv; parts[4] = scale; }
}

static void tr_next_batch(az_trainer* t, std::vector<int>& idx) {
  // Flux.DataLoader(shuffle = true, partial = false) cycled (learning.jl:114-119): a fresh permutation per epoch,
  // Fisher-Yates driven by the RNG contract's shuffle stream (seed; epoch)
  const int64_t n = t->d->n;
  idx.resize(t->B);
  if (t->perm.empty() || t->perm_pos + t->B > n) {
    t->perm.resize(n);
    for (int64_t i = 0; i < n; ++i) t->perm[i] = (int)i;
    az_rng r = az_rng_make(t->cfg.seed, (uint32_t)t->epoch, 0, AZ_RNG_SHUFFLE);
    for (int64_t i = n - 1; i > 0; --i) {
      int64_t j = (int64_t)(az_rng_f64(&r) * (double)(i + 1));
      if (j > i) j = i;
      std::swap(t->perm[i], t->perm[j]);
    }
    t->perm_pos = 0; t->epoch++;
  }
  for (int b = 0; b < t->B; ++b) idx[b] = t->perm[t->perm_pos + b];
  t->perm_pos += t->B;
}

extern "C" int az_trainer_create(az_engine* e, az_dataset* d, const az_train_cfg* cfg, az_trainer** out) {
  ENGINE(e);
  if (!d || !cfg || !out) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(az_train_cfg)) return fail(AZ_ERR_BAD_ARG, "az_train_cfg size mismatch: call az_train_cfg_init");
  if (!oracle_is_net(e->cfg) || !e->net_loaded) return fail(AZ_ERR_STATE, "az_net_set_params has not been called");
  if (d->game != e->cfg.game || d->device != e->device) return fail(AZ_ERR_BAD_ARG, "data set and engine differ in game or device");
  if (cfg->optimiser != AZ_OPT_ADAM && cfg->optimiser != AZ_OPT_CYCLIC_NESTEROV) return fail(AZ_ERR_BAD_ARG, "unknown optimiser %d", cfg->optimiser);
  const int64_t B = std::min<int64_t>(cfg->batch_size, d->n);     // batchsize = min(params.batch_size, length(W)), learning.jl:113
  if (cfg->batch_size < 2 || B < 2) return fail(AZ_ERR_BAD_ARG, "batch_size and the data set must have at least 2 samples (batch statistics)");
  if (!(cfg->rewards_renormalization > 0.0)) return fail(AZ_ERR_BAD_ARG, "rewards_renormalization must be > 0");
  az_trainer* t = new (std::nothrow) az_trainer();
  if (!t) return fail(AZ_ERR_HIP, "out of host memory");
  t->e = e; t->d = d; t->cfg = *cfg; t->game = e->cfg.game; t->device = e->device; t->gi = e->gi;
  t->B = (int)B; t->F = e->cfg.num_filters; t->R = (long long)B * e->gi.P; t->nparams = e->blob.size();   // (F, R: of a ResNet's tower; a dense chain has neither)
  int st = [&]() -> int {
    // the chain of the step on a high-priority stream, the weight gradients beside it on a low-priority one
    int pr_least = 0, pr_greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    HIPCHK(hipStreamCreateWithPriority(&t->stream, hipStreamDefault, pr_greatest));
    HIPCHK(hipStreamCreateWithPriority(&t->side, hipStreamNonBlocking, pr_least));
    t->gemm_ws_floats = (size_t)4 << 20;                            // 16 MB: partial tiles of the split weight-gradient reductions
    AZCHK(tr_alloc(t, &t->gemm_ws, t->gemm_ws_floats));
    AZCHK(trainer_build(t));
    return AZ_OK;
  }();
  if (st != AZ_OK) { az_trainer_destroy(t); return st; }
  *out = t;
  return AZ_OK;
}

#define TRAINER(t) if (!(t)) return fail(AZ_ERR_BAD_ARG, "trainer is NULL"); HIPCHK(hipSetDevice((t)->device))

// loss and data gradient (blob layout, WITHOUT the L2 term) of one given batch; no update.  parts = Lp, Lv, Lreg, Linv, scale.
extern "C" int az_trainer_gradients(az_trainer* t, const int32_t* sample_idx, float* loss, float* parts, float* grad, int64_t n) {
  TRAINER(t);
  if (!sample_idx || !loss) return fail(AZ_ERR_BAD_ARG, "NULL argument");
  for (int b = 0; b < t->B; ++b) if (sample_idx[b] < 0 || sample_idx[b] >= t->d->n) return fail(AZ_ERR_BAD_ARG, "sample index %d out of range", sample_idx[b]);
  if (grad && n != (int64_t)t->nparams) return fail(AZ_ERR_BAD_ARG, "gradient buffer must hold %zu floats", t->nparams);
  // the running statistics must not move in a gradient probe: save / restore them around the pass
  std::vector<float> saved(t->nparams);
  HIPCHK(hipMemcpy(saved.data(), t->blob, sizeof(float) * t->nparams, hipMemcpyDeviceToHost));
  AZCHK(tr_forward_backward(t, sample_idx, t->bsums));
  double sums[5];
  HIPCHK(hipMemcpyAsync(sums, t->bsums, sizeof sums, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  tr_losses(t, sums, loss, parts);
  if (grad) HIPCHK(hipMemcpy(grad, t->gblob, sizeof(float) * t->nparams, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(t->blob, saved.data(), sizeof(float) * t->nparams, hipMemcpyHostToDevice));
  return AZ_OK;
}

// debug aid (not part of the ABI in azhip.h): the post-ReLU activation the last forward pass left for layer `which` -- tower
// layers 0 .. 2 num_blocks ([R][F], R = batch x positions), then the policy / value head convolutions ([R][npf], [R][nvf]), then
// the value head's first dense layer ([batch][F]); of a dense chain, layer `which` of SimpleLayout::dense ([batch][out]).  tests/test_train_gpu.py reads the ReLU masks (a > 0) off them: an fp32 chain
// and an fp64 reference disagree on activations within rounding of zero, and ONE flipped unit moves single weight-gradient
// entries by more than the tolerance the rest of the gradient meets.
extern "C" int az_debug_trainer_activation(az_trainer* t, int32_t which, float* out, int64_t n) {
  TRAINER(t);
  // an index into the table, but for a ResNet's last one: the table holds the policy head's dense layer before the value head's
  const int nact = t->ntower ? t->ntower + 3 : (int)t->layers.size();
  if (which < 0 || which >= nact) return fail(AZ_ERR_BAD_ARG, "layer %d of %d", which, nact);
  const TrLayer& c = t->layers[t->ntower && which == t->ntower + 2 ? t->ival - 1 : which];
  const int64_t want = (int64_t)c.rows * c.out;
  if (!out || n != want) return fail(AZ_ERR_BAD_ARG, "buffer must hold %lld floats", (long long)want);
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipMemcpy(out, c.a, sizeof(float) * (size_t)want, hipMemcpyDeviceToHost));
  return AZ_OK;
}

// debug aids (not part of the ABI in azhip.h): the step's three MFMA kernels one at a time, on caller-supplied host arrays, through
// the trainer's own launch helpers on t->stream -- so the geometry table, wg_splits, the partial buffers, the fragment maps and the
// GEMM workspace with its split rule are the ones a step uses.  tests/test_train_kernels_gpu.py feeds them small integers, whose
// fp32 sums are exact in any order, and compares bit for bit at the batches where the kernels' inner loops iterate.
static int tr_up(Scratch& tmp, float** p, const float* host, size_t n) {   // a host array as scratch of the call
  AZCHK(tmp.alloc(p, n));
  if (host) HIPCHK(hipMemcpy(*p, host, sizeof(float) * n, hipMemcpyHostToDevice));
  return AZ_OK;
}
#define TR_TOWER(t) if (!(t)->ntower) return fail(AZ_ERR_BAD_ARG, "the trainer of a SimpleNet engine has no convolution"); if ((t)->ntower < 3) return fail(AZ_ERR_BAD_ARG, "the trainer's tower has no F -> F convolution (num_blocks = 0)")
// weight gradient of a 3x3 F -> F convolution (tr_wgrad16 = k_wgrad16 + k_wgrad_reduce): a, dg = [B P][F] with row = board P + y W + x;
// out[9][F][F] = [tap][ci][co], tap = 3 (dy + 1) + (dx + 1): sum over the rows whose neighbour (y + dy, x + dx) is on the board of a[neighbour][ci] dg[row][co]
extern "C" int az_debug_trainer_wgrad(az_trainer* t, const float* a, const float* dg, int64_t n_in, float* out, int64_t n_out) {
  TRAINER(t);
  TR_TOWER(t);
  const int64_t want_in = (int64_t)t->R * t->F, want_out = 9LL * t->F * t->F;
  if (!a || !dg || n_in != want_in) return fail(AZ_ERR_BAD_ARG, "a and dg must hold %lld floats", (long long)want_in);
  if (!out || n_out != want_out) return fail(AZ_ERR_BAD_ARG, "out must hold %lld floats", (long long)want_out);
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  HIPCHK(hipMemcpy(t->dact, a, sizeof(float) * (size_t)want_in, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->dact2, dg, sizeof(float) * (size_t)want_in, hipMemcpyHostToDevice));
  float* dw = t->gwork + t->layers[1].wk_wm;
  AZCHK(tr_wgrad16(t, t->dact, t->dact2, dw, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dw, sizeof(float) * (size_t)want_out, hipMemcpyDeviceToHost));
  return AZ_OK;
}
// tower layer `layer` >= 1 on the trainer's CURRENT parameters (k_tr_gather, then tr_conv16 = k_conv16_layer), all arrays [B P][F]:
//   dgrad = 1: out = conv(in, wk_fdg fragments) (+ addend)        -- the data gradient of the layer's input
//   dgrad = 0: a_out = relu(gamma ((in - mean) invstd) + beta (+ res)), out = conv(a_out, wk_ffwd fragments), with the column sums of
//              out finished by k_tr_colsum_final in mode 0: sums[2][F] = (sum, sum of squares); bn = [4][F]: mean, invstd, gamma, beta
// nparts: the workgroups of the launch (64 filters: which tile count ran -- ceil(B / boards of the 6- or the 11-tile form))
extern "C" int az_debug_trainer_conv(az_trainer* t, int32_t layer, int32_t dgrad, const float* in, const float* addend, const float* bn, const float* res,
                                     int64_t n, float* out, float* a_out, double* sums, int32_t* nparts) {
  TRAINER(t);
  TR_TOWER(t);
  if (layer < 1 || layer >= t->ntower) return fail(AZ_ERR_BAD_ARG, "layer %d: the F -> F convolutions are 1 .. %d", layer, t->ntower - 1);
  const int F = t->F;
  const int64_t want = (int64_t)t->R * F;
  if (!in || !out || n != want) return fail(AZ_ERR_BAD_ARG, "in and out must hold %lld floats", (long long)want);
  if (dgrad ? (bn || res || a_out || sums) : (addend || !bn || !a_out || !sums))
    return fail(AZ_ERR_BAD_ARG, dgrad ? "the data gradient takes in, addend and out only" : "the forward pass takes in, bn, res, out, a_out and sums");
  const TrLayer& c = t->layers[layer];
  const size_t bytes = sizeof(float) * (size_t)want;
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  hipLaunchKernelGGL(k_tr_gather, dim3(tr_grid((long long)t->nwork)), dim3(256), 0, t->stream, t->blob, t->map, (long long)t->nwork, t->work);
  HIPCHK(hipMemcpy(t->dact, in, bytes, hipMemcpyHostToDevice));
  const float* second = dgrad ? addend : res;
  if (second) HIPCHK(hipMemcpy(t->dact2, second, bytes, hipMemcpyHostToDevice));
  int np = 0;
  Scratch tmp;                                                      // lives until the stream has been waited for
  if (dgrad) {
    AZCHK(tr_conv16(t, t->dact, t->work + c.wk_fdg, t->dact3, false, &np, second ? t->dact2 : nullptr));
  } else {
    float* dbn = nullptr;
    AZCHK(tr_up(tmp, &dbn, bn, 4 * (size_t)F));
    TrFinal fin{};                                                  // mode 0: the sums only; no counter: the second stage is the separate launch
    AZCHK(tr_conv16(t, nullptr, t->work + c.wk_ffwd, t->dact3, true, &np, nullptr, BnIn{t->dact, dbn, dbn + F, dbn + 2 * F, dbn + 3 * F, second ? t->dact2 : nullptr, t->dcol}, fin));
    hipLaunchKernelGGL(k_tr_colsum_final, dim3(F), dim3(64), 0, t->stream, t->part, np, F, t->sums, fin);
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, t->dact3, bytes, hipMemcpyDeviceToHost));
  if (!dgrad) {
    HIPCHK(hipMemcpy(a_out, t->dcol, bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sums, t->sums, sizeof(double) * 2 * (size_t)F, hipMemcpyDeviceToHost));
  }
  if (nparts) *nparts = np;
  return AZ_OK;
}
// C[M][N] = alpha op(A) op(B) + beta C through tr_gemm: the trainer's workspace and gemm_f32's split rule.  Row-major host arrays
// with leading dimensions lda / ldb / ldc; na / nb / nc = their sizes in floats (rows x leading dimension).
extern "C" int az_debug_trainer_gemm(az_trainer* t, int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, float alpha, const float* A, int32_t lda, int64_t na,
                                     const float* B, int32_t ldb, int64_t nb, float beta, float* Cm, int32_t ldc, int64_t nc) {
  TRAINER(t);
  if (M < 1 || N < 1 || K < 1) return fail(AZ_ERR_BAD_ARG, "M, N and K must be positive");
  const int ra = ta ? K : M, ca = ta ? M : K, rb = tb ? N : K, cb = tb ? K : N;
  if (!A || lda < ca || na != (int64_t)ra * lda) return fail(AZ_ERR_BAD_ARG, "A must hold %d rows of lda >= %d floats", ra, ca);
  if (!B || ldb < cb || nb != (int64_t)rb * ldb) return fail(AZ_ERR_BAD_ARG, "B must hold %d rows of ldb >= %d floats", rb, cb);
  if (!Cm || ldc < N || nc != (int64_t)M * ldc) return fail(AZ_ERR_BAD_ARG, "C must hold %d rows of ldc >= %d floats", M, N);
  Scratch tmp;
  float *dA = nullptr, *dB = nullptr, *dC = nullptr;
  AZCHK(tr_up(tmp, &dA, A, (size_t)na)); AZCHK(tr_up(tmp, &dB, B, (size_t)nb)); AZCHK(tr_up(tmp, &dC, Cm, (size_t)nc));
  HIPCHK(hipStreamSynchronize(t->stream));
  AZCHK(tr_gemm(t, ta != 0, tb != 0, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(Cm, dC, sizeof(float) * (size_t)nc, hipMemcpyDeviceToHost));
  return AZ_OK;
}

// debug aids (not part of the ABI in azhip.h): the step's reductions and pointwise passes one at a time, as the seams above -- the
// trainer's own launch helpers (tr_colsum, tr_bn_apply, tr_bn_bwd, tr_bias_act, tr_relu_bwd, tr_im2col, tr_loss, tr_step_sums) on
// t->stream with t->part, t->sums, t->bn_mf, t->fin_counter, t->env.fin_inside and the helpers' dispatch rules; the arrays of the
// caller are scratch of the call from the allocator the trainer's own arrays come from.  tests/test_train_passes_gpu.py.
static int tr_down(float* host, const float* dev, size_t n) { HIPCHK(hipMemcpy(host, dev, sizeof(float) * n, hipMemcpyDeviceToHost)); return AZ_OK; }
// a host array [R][C] with one guard row behind it that holds `guard` in every column: a kernel that reads a row past the end reads inside the
// allocation, and what it reads shows in its sums (x = 4096 under a positive activation, g = 4096) instead of depending on what lies behind an array
static int tr_up_guarded(Scratch& tmp, float** p, const float* host, size_t n, int C, float guard) {
  AZCHK(tr_up(tmp, p, nullptr, n + (size_t)C));
  HIPCHK(hipMemcpy(*p, host, sizeof(float) * n, hipMemcpyHostToDevice));
  const std::vector<float> row((size_t)C, guard);
  HIPCHK(hipMemcpy(*p + n, row.data(), sizeof(float) * (size_t)C, hipMemcpyHostToDevice));
  return AZ_OK;
}
// column sums of `mode` (0: x, x^2; 1: dy, dy xhat with dy = x (out_act > 0), xhat = (g - mean) invstd; 2: x, 0) over x[R][C] through
// tr_colsum<mode>, finished as fin_mode says (TrFinal):
//   mode 1 reads out_act, g [R][C] and stat_in[2][C] = mean, invstd
//   fin_mode 1 reads fin_in[3][C] = bias, running mean, running variance and writes fin_out[4][C] = mean, invstd, running mean, running variance
//   fin_mode 2 writes fin_out[4][C] = dbeta, dgamma, mf[2][C] (mf = t->bn_mf);  fin_mode 3 writes fin_out[C] = out0
// sums[2][C]: t->sums (the separate second stage writes them; the second stage inside the producer does not: NaN then).
// info[4] = what tr_colsum launched: chunks, 1 if k_tr_colsum1v, 1 if the second stage ran inside the producer, gridDim.y of the producer.
// x, out_act and g lie in scratch with a guard row behind them (tr_up_guarded).  Refuses an (R, C) whose partials, sums or means the trainer's
// scratch cannot hold.
extern "C" int az_debug_trainer_colsum(az_trainer* t, int32_t mode, int64_t R, int32_t C, const float* x, const float* out_act, const float* g, int64_t n,
                                       const float* stat_in, int32_t fin_mode, float momentum, int32_t with_bias, const float* fin_in,
                                       double* sums, float* fin_out, int32_t* info) {
  TRAINER(t);
  if (mode < 0 || mode > 2 || fin_mode < 0 || fin_mode > 3) return fail(AZ_ERR_BAD_ARG, "mode %d (0 .. 2), fin_mode %d (0 .. 3)", mode, fin_mode);
  if (R < 1 || C < 1 || R > (int64_t)1 << 40 || n != R * (int64_t)C || !x || !sums) return fail(AZ_ERR_BAD_ARG, "x must hold R x C = %lld floats, R and C positive", (long long)(R * (int64_t)C));
  if ((mode == 1) != (out_act && g && stat_in)) return fail(AZ_ERR_BAD_ARG, "mode 1 and only mode 1 takes out_act, g and stat_in");
  if ((fin_mode != 0) != (fin_out != nullptr) || (fin_mode == 1) != (fin_in != nullptr)) return fail(AZ_ERR_BAD_ARG, "fin_mode %d: fin_out %s, fin_in %s", fin_mode, fin_mode ? "needed" : "not taken", fin_mode == 1 ? "needed" : "not taken");
  if (fin_mode == 1 && R < 2) return fail(AZ_ERR_BAD_ARG, "batch statistics need two rows");
  const int64_t nchunks = (R + TR_CHUNK - 1) / TR_CHUNK;
  if ((size_t)nchunks * 2 * (size_t)C > t->npart) return fail(AZ_ERR_BAD_ARG, "%lld chunks x 2 x %d columns do not fit the trainer's %zu partials", (long long)nchunks, C, t->npart);
  if (C > t->wsum) return fail(AZ_ERR_BAD_ARG, "%d columns do not fit the trainer's sums (%d)", C, t->wsum);
  if (fin_mode == 2 && C > t->wbn) return fail(AZ_ERR_BAD_ARG, "%d columns do not fit the trainer's batch-norm means (%d)", C, t->wbn);
  Scratch tmp;
  float *dx = nullptr, *da = nullptr, *dgg = nullptr, *dstat = nullptr, *dfin = nullptr, *dout = nullptr;
  AZCHK(tr_up_guarded(tmp, &dx, x, (size_t)n, C, 4096.0f));
  if (mode == 1) { AZCHK(tr_up_guarded(tmp, &da, out_act, (size_t)n, C, 1.0f)); AZCHK(tr_up_guarded(tmp, &dgg, g, (size_t)n, C, 4096.0f)); AZCHK(tr_up(tmp, &dstat, stat_in, 2 * (size_t)C)); }
  // every vector of the finisher an array of its own, as the layers' mean / invstd are
  float* o[4] = {nullptr, nullptr, nullptr, nullptr};
  TrFinal fin{};
  fin.mode = fin_mode; fin.R = R; fin.momentum = momentum;
  if (fin_mode == 1) {
    AZCHK(tr_up(tmp, &dfin, fin_in, (size_t)C));
    for (int k = 0; k < 4; ++k) AZCHK(tr_up(tmp, &o[k], k >= 2 ? fin_in + (size_t)(k - 1) * C : nullptr, (size_t)C));
    fin.bias = with_bias ? dfin : nullptr; fin.mean = o[0]; fin.invstd = o[1]; fin.run_mean = o[2]; fin.run_var = o[3];
  } else if (fin_mode == 2) {
    for (int k = 0; k < 2; ++k) AZCHK(tr_up(tmp, &o[k], nullptr, (size_t)C));
    fin.dbeta = o[0]; fin.dgamma = o[1]; fin.mf = t->bn_mf;
  } else if (fin_mode == 3) { AZCHK(tr_up(tmp, &dout, nullptr, (size_t)C)); fin.out0 = dout; }
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  HIPCHK(hipMemsetAsync(t->sums, 0xff, sizeof(double) * 2 * (size_t)C, t->stream));   // NaN where no second stage writes
  int32_t ran[4] = {0, 0, 0, 0};
  if (mode == 0) AZCHK(tr_colsum<0>(t, dx, nullptr, nullptr, nullptr, nullptr, R, C, fin, ran));
  else if (mode == 1) AZCHK(tr_colsum<1>(t, dx, da, dgg, dstat, dstat + C, R, C, fin, ran));
  else AZCHK(tr_colsum<2>(t, dx, nullptr, nullptr, nullptr, nullptr, R, C, fin, ran));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(sums, t->sums, sizeof(double) * 2 * (size_t)C, hipMemcpyDeviceToHost));
  if (fin_mode == 1) for (int k = 0; k < 4; ++k) AZCHK(tr_down(fin_out + (size_t)k * C, o[k], (size_t)C));
  if (fin_mode == 2) { for (int k = 0; k < 2; ++k) AZCHK(tr_down(fin_out + (size_t)k * C, o[k], (size_t)C)); AZCHK(tr_down(fin_out + 2 * (size_t)C, t->bn_mf, 2 * (size_t)C)); }
  if (fin_mode == 3) AZCHK(tr_down(fin_out, dout, (size_t)C));
  if (info) for (int k = 0; k < 4; ++k) info[k] = ran[k];
  return AZ_OK;
}
// the pointwise passes over [rows][C], n = rows x C:
//   op 0  out = relu(gamma ((g - mean) invstd) + beta (+ second))                 tr_bn_apply;  consts[4][C] = mean, invstd, gamma, beta
//   op 1  out = dg, written over da in place; out2 (optional) = dy                tr_bn_bwd;    first = da, second = a, consts[3][C] = mean, invstd, gamma,
//                                                                                              mf[2][C] -> t->bn_mf
//   op 2  out = [relu](g + bias) in place                                         tr_bias_act;  consts[C] = bias, flag = relu
//   op 3  out = first (second > 0) in place                                       tr_relu_bwd;  first = dy, second = y
extern "C" int az_debug_trainer_bn(az_trainer* t, int32_t op, int64_t rows, int32_t C, const float* g, const float* first, const float* second,
                                   const float* consts, const float* mf, int32_t flag, int64_t n, float* out, float* out2) {
  TRAINER(t);
  if (op < 0 || op > 3) return fail(AZ_ERR_BAD_ARG, "op %d (0 .. 3)", op);
  if (rows < 1 || C < 1 || rows > (int64_t)1 << 40 || n != rows * (int64_t)C || !out) return fail(AZ_ERR_BAD_ARG, "the arrays must hold rows x C = %lld floats, rows and C positive", (long long)(rows * (int64_t)C));
  const bool ok = op == 0 ? (g && !first && consts && !mf && !out2) : op == 1 ? (g && first && second && consts && mf)
                : op == 2 ? (g && !first && !second && consts && !mf && !out2) : (!g && first && second && !consts && !mf && !out2);
  if (!ok) return fail(AZ_ERR_BAD_ARG, "op %d does not take these arrays", op);
  if (op == 1 && C > t->wbn) return fail(AZ_ERR_BAD_ARG, "%d columns do not fit the trainer's batch-norm means (%d)", C, t->wbn);
  Scratch tmp;
  float *dg = nullptr, *d1 = nullptr, *d2 = nullptr, *dout = nullptr, *dout2 = nullptr, *dc[4] = {nullptr, nullptr, nullptr, nullptr};
  if (g) AZCHK(tr_up(tmp, &dg, g, (size_t)n));
  if (first) AZCHK(tr_up(tmp, &d1, first, (size_t)n));
  if (second) AZCHK(tr_up(tmp, &d2, second, (size_t)n));
  const int nc = op == 0 ? 4 : op == 1 ? 3 : op == 2 ? 1 : 0;
  for (int k = 0; k < nc; ++k) AZCHK(tr_up(tmp, &dc[k], consts + (size_t)k * C, (size_t)C));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  const float* res = nullptr;
  if (op == 0) {
    AZCHK(tr_up(tmp, &dout, nullptr, (size_t)n));
    tr_bn_apply(t, BnIn{dg, dc[0], dc[1], dc[2], dc[3], d2, dout}, n, C);
    res = dout;
  } else if (op == 1) {
    if (out2) AZCHK(tr_up(tmp, &dout2, nullptr, (size_t)n));
    HIPCHK(hipMemcpy(t->bn_mf, mf, sizeof(float) * 2 * (size_t)C, hipMemcpyHostToDevice));
    tr_bn_bwd(t, d1, d2, dg, dc[0], dc[1], dc[2], n, C, d1, dout2);
    res = d1;
  } else if (op == 2) { tr_bias_act(t, dg, dc[0], n, C, flag != 0); res = dg; }
  else { tr_relu_bwd(t, d1, d2, n); res = d1; }
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  AZCHK(tr_down(out, res, (size_t)n));
  if (dout2) AZCHK(tr_down(out2, dout2, (size_t)n));
  return AZ_OK;
}
// the stem's gather on the trainer's geometry and batch: planes[B][C][H][W] -> col[B H W][9 C], column = tap C + c, tap = 3 (dy + 1) + (dx + 1)
extern "C" int az_debug_trainer_im2col(az_trainer* t, const float* planes, int64_t n_in, float* col, int64_t n_out) {
  TRAINER(t);
  if (!t->ntower) return fail(AZ_ERR_BAD_ARG, "the trainer of a SimpleNet engine has no convolution");
  const TrLayer& c = t->layers[0];
  const int64_t want_in = (int64_t)t->B * t->gi.C * t->gi.P, want_out = (int64_t)c.rows * c.in;
  if (!planes || n_in != want_in) return fail(AZ_ERR_BAD_ARG, "planes must hold %lld floats", (long long)want_in);
  if (!col || n_out != want_out) return fail(AZ_ERR_BAD_ARG, "col must hold %lld floats", (long long)want_out);
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  HIPCHK(hipMemcpy(t->bX, planes, sizeof(float) * (size_t)want_in, hipMemcpyHostToDevice));
  tr_im2col(t, t->bX, c);
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  return tr_down(col, c.col, (size_t)want_out);
}
// the loss of one batch of B = the trainer's batch samples and A = the game's actions through tr_loss (force_wide: k_tr_loss_wide whatever A):
// dlogits[B][A], dt[B] and terms[4][B] = w, kl, mse, inv per sample; *wide = which kernel ran.  Then (terms_in given) k_tr_step_sums through
// tr_step_sums on terms_in[4][B]: sums5 = their four sums and the sum of squares of the trainable parameters.
extern "C" int az_debug_trainer_loss(az_trainer* t, int32_t force_wide, const float* logits, const float* tpre, const float* Am, const float* P, int64_t n_ba,
                                     const float* V, const float* W, int64_t n_b, float cinv, float rho, float gscale,
                                     float* dlogits, float* dt, double* terms, int32_t* wide, const double* terms_in, double* sums5) {
  TRAINER(t);
  const int B = t->B, A = t->gi.A;
  if (!logits || !Am || !P || !dlogits || n_ba != (int64_t)B * A) return fail(AZ_ERR_BAD_ARG, "logits, Am, P and dlogits must hold %lld floats", (long long)B * A);
  if (!tpre || !V || !W || !dt || !terms || n_b != B) return fail(AZ_ERR_BAD_ARG, "tpre, V, W and dt must hold %d floats, terms 4 x %d doubles", B, B);
  if ((terms_in != nullptr) != (sums5 != nullptr)) return fail(AZ_ERR_BAD_ARG, "terms_in and sums5 go together");
  if (!(rho > 0.0f)) return fail(AZ_ERR_BAD_ARG, "rho must be > 0");
  Scratch tmp;
  float *dl = nullptr, *dtp = nullptr, *ddl = nullptr, *ddt = nullptr;
  AZCHK(tr_up(tmp, &dl, logits, (size_t)n_ba)); AZCHK(tr_up(tmp, &dtp, tpre, (size_t)B));
  AZCHK(tr_up(tmp, &ddl, nullptr, (size_t)n_ba)); AZCHK(tr_up(tmp, &ddt, nullptr, (size_t)B));
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipStreamSynchronize(t->side));
  HIPCHK(hipMemcpy(t->bA, Am, sizeof(float) * (size_t)n_ba, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(t->bP, P, sizeof(float) * (size_t)n_ba, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->bV, V, sizeof(float) * (size_t)B, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(t->bW, W, sizeof(float) * (size_t)B, hipMemcpyHostToDevice));
  const bool w = tr_loss(t, dl, dtp, cinv, rho, gscale, ddl, ddt, force_wide != 0);
  HIPCHK(hipStreamSynchronize(t->stream));
  HIPCHK(hipGetLastError());
  AZCHK(tr_down(dlogits, ddl, (size_t)n_ba)); AZCHK(tr_down(dt, ddt, (size_t)B));
  HIPCHK(hipMemcpy(terms, t->terms, sizeof(double) * 4 * (size_t)B, hipMemcpyDeviceToHost));
  if (wide) *wide = w;
  if (terms_in) {
    HIPCHK(hipMemcpy(t->terms, terms_in, sizeof(double) * 4 * (size_t)B, hipMemcpyHostToDevice));
    tr_step_sums(t, t->bsums);
    HIPCHK(hipStreamSynchronize(t->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(sums5, t->bsums, sizeof(double) * 5, hipMemcpyDeviceToHost));
  }
  return AZ_OK;
}

// batch_updates!(tr, n) (learning.jl:131-141): n optimiser steps on successive batches; losses[i] = L before update i
extern "C" int az_trainer_batch_updates(az_trainer* t, int32_t n, float* losses) {
  TRAINER(t);
  if (n < 0) return fail(AZ_ERR_BAD_ARG, "n must be >= 0");
  if (n == 0) return AZ_OK;
  // Network.train! builds a fresh optimiser state on every call (Flux.setup inside train!, flux.jl:69,83): the Adam
  // moments / Nesterov velocities do not survive from one batch_updates! (checkpoint) to the next
  HIPCHK(hipMemsetAsync(t->opt_m, 0, sizeof(float) * t->nparams, t->stream));
  HIPCHK(hipMemsetAsync(t->opt_v, 0, sizeof(float) * t->nparams, t->stream));
  t->b1t = 1.0f; t->b2t = 1.0f;
  // the n steps are enqueued back to back: no host round trip inside the loop (the step sums of every step stay on the
  // device until the end; the batch indices of all steps stay alive in `idx`)
  std::vector<std::vector<int>> idx((size_t)n);
  double* d_sums = nullptr;
  HIPCHK(hipMalloc((void**)&d_sums, sizeof(double) * 5 * (size_t)n));
  const float reg_c = (float)(2.0 * (double)(float)t->cfg.l2_regularization / ((double)t->B * (double)t->d->Wmean));   // d/dw of scale * creg * sum(w^2) = (sum W) * reg_c * w
  int rc = AZ_OK;
  for (int i = 0; i < n && rc == AZ_OK; ++i) {
    tr_next_batch(t, idx[i]);
    double* ds = d_sums + 5 * (size_t)i;
    rc = tr_forward_backward(t, idx[i].data(), ds);
    if (rc != AZ_OK) break;
    if (t->cfg.optimiser == AZ_OPT_ADAM) {
      t->b1t *= 0.9f; t->b2t *= 0.999f;
      hipLaunchKernelGGL(k_tr_adam, dim3(tr_grid((long long)t->nparams)), dim3(256), 0, t->stream, t->blob, t->gblob, t->opt_m, t->opt_v, t->trainable,
                         (long long)t->nparams, t->cfg.lr, t->b1t, t->b2t, ds, reg_c);
    } else {
      // lr = CyclicSchedule(lr_base, lr_high, lr_low; n), momentum = CyclicSchedule(momentum_high, momentum_low,
      // momentum_high; n) (flux.jl:78-94); CyclicSchedule = PLSchedule([1, floor(.45 n), floor(.9 n), n], [base, mid, base,
      // term]) (schedule.jl:130-134).  Flux.adjust! follows update!, so step i (1-based) runs with the values of index i-1
      // and the first step with Nesterov(lr_low, momentum_high).
      auto cyc = [&](double base, double mid, double term, int k) -> float {
        const int xs[4] = {1, (int)(0.45 * n), (int)(0.90 * n), n};
        const double ys[4] = {base, mid, base, term};
        int pt = -1;
        for (int q = 0; q < 4; ++q) if (xs[q] <= k) pt = q;
        if (pt < 0) return (float)ys[0];
        if (pt == 3) return (float)ys[3];
        if (xs[pt + 1] == xs[pt]) return (float)ys[pt];
        return (float)(ys[pt] + (ys[pt + 1] - ys[pt]) / (double)(xs[pt + 1] - xs[pt]) * (double)(k - xs[pt]));
      };
      const float lr = i == 0 ? t->cfg.lr_low : cyc(t->cfg.lr_base, t->cfg.lr_high, t->cfg.lr_low, i);
      const float rho = i == 0 ? t->cfg.momentum_high : cyc(t->cfg.momentum_high, t->cfg.momentum_low, t->cfg.momentum_high, i);
      hipLaunchKernelGGL(k_tr_nesterov, dim3(tr_grid((long long)t->nparams)), dim3(256), 0, t->stream, t->blob, t->gblob, t->opt_m, t->trainable,
                         (long long)t->nparams, lr, rho, ds, reg_c);
    }
    t->step++;
  }
  std::vector<double> sums(5 * (size_t)n);
  hipError_t e1 = hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, t->stream);
  hipError_t e2 = hipStreamSynchronize(t->stream);
  hipError_t e3 = hipGetLastError();
  (void)hipFree(d_sums);
  AZCHK(rc);
  HIPCHK(e1); HIPCHK(e2); HIPCHK(e3);
  if (losses) for (int i = 0; i < n; ++i) tr_losses(t, &sums[5 * (size_t)i], &losses[i], nullptr);
  return AZ_OK;
}

// get_trained_network (learning.jl:127-129): the current parameters (Flux order, running statistics included)
extern "C" int az_trainer_get_params(az_trainer* t, float* blob, int64_t n) {
  TRAINER(t);
  if (!blob || n != (int64_t)t->nparams) return fail(AZ_ERR_BAD_ARG, "blob must hold %zu floats", t->nparams);
  HIPCHK(hipMemcpy(blob, t->blob, sizeof(float) * t->nparams, hipMemcpyDeviceToHost));
  return AZ_OK;
}
