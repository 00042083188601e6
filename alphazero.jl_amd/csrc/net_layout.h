// net_layout.h -- the parameter blob and every reordering of it, written once.  Plain C++ (no device runtime, no engine.h): a host
// compiler builds it alone (tests/net_layout_driver.cpp; tests/test_net_layout_cpu.py holds it to independent restatements).
//   NetLayout        where each piece of the flat fp32 blob (Flux array order) lies: the only place in csrc/ that knows the order and
//                    sizes of the pieces (az_net_num_params, az_net_set_params and the trainer all ask it)
//   flux_conv_index  which element of a Flux convolution weight a tap reads
//   index maps       every device weight array as a std::vector<int32_t>: dst[j] = blob[map[j]], -1 = zero padding.  One function per
//                    ORDER, named after the kernel that reads it; what is reordered is a `source`, a callable (tap, ci, co) -> blob
//                    index (or -1), so one order serves a tower layer, the concatenated head convolution and the trainer alike.
//   NetMaps          the maps of one engine's device arrays (they depend on the configuration only: built once per engine)
//   SimpleLayout     the same for NetLib.SimpleNet, the dense two-headed network (at the end of this file): SimpleMaps for k_simplenet
//                    (simplenet.h), SimpleTrainMaps for a dense optimiser chain
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct NetShape { int C, P, A, APAD, num_blocks, F, npf, nvf; };   // planes, positions, actions (padded), residual blocks, filters, head filters

// One convolution + batch norm in the blob: W (Flux (k, k, cin, cout)), bias [cout], then gamma, beta, running mean, running variance
struct ConvAt {
  int cin, cout, ksz;
  size_t w, b, bn;
  size_t bn_vec(int k) const { return bn + (size_t)k * cout; }   // k = 0 .. 3: gamma, beta, running mean, running variance
  int taps() const { return ksz * ksz; }
  size_t nw() const { return (size_t)taps() * cin * cout; }
};
// stem, 2 num_blocks tower layers, policy head (1x1 conv, dense P npf -> A), value head (1x1 conv, dense P nvf -> F, dense F -> 1)
struct NetLayout {
  NetShape s;
  std::vector<ConvAt> conv;      // [0] stem, [1 .. 2 nb] tower, then the policy-head and the value-head convolution
  size_t pd_w, pd_b, v1_w, v1_b, v2_w, v2_b, total;
  explicit NetLayout(const NetShape& sh) : s(sh) {
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += n; return o; };
    auto add_conv = [&](int cin, int cout, int ksz) {
      ConvAt c{cin, cout, ksz, 0, 0, 0};
      c.w = take(c.nw()); c.b = take(cout); c.bn = take(4 * (size_t)cout);
      conv.push_back(c);
    };
    add_conv(s.C, s.F, 3);
    for (int l = 0; l < 2 * s.num_blocks; ++l) add_conv(s.F, s.F, 3);
    add_conv(s.F, s.npf, 1);
    pd_w = take((size_t)s.A * s.P * s.npf); pd_b = take(s.A);
    add_conv(s.F, s.nvf, 1);
    v1_w = take((size_t)s.F * s.P * s.nvf); v1_b = take(s.F);
    v2_w = take(s.F); v2_b = take(1);
    total = at;
  }
  int ntower() const { return 2 * s.num_blocks; }
  const ConvAt& stem() const { return conv[0]; }
  const ConvAt& tower(int l) const { return conv[1 + l]; }
  const ConvAt& phead() const { return conv[conv.size() - 2]; }
  const ConvAt& vhead() const { return conv[conv.size() - 1]; }
};

// Offset inside a Flux convolution weight W[i + k (j + k (ci + Cin co))] of the element that tap t = (dy+1)*3 + (dx+1) reads: W[i = 1 - dx,
// j = 1 - dy] -- the true convolution, flipped kernel.  ksz = 1: the one tap 0.
inline size_t flux_conv_index(int ksz, int Cin, int tap, int ci, int co) {
  const int dy = ksz == 3 ? tap / 3 - 1 : 0, dx = ksz == 3 ? tap % 3 - 1 : 0;
  const int wi = ksz == 3 ? 1 - dx : 0, wj = ksz == 3 ? 1 - dy : 0;
  return (size_t)wi + (size_t)ksz * (wj + (size_t)ksz * (ci + (size_t)Cin * co));
}

using IndexMap = std::vector<int32_t>;
inline void append(IndexMap& to, const IndexMap& m) { to.insert(to.end(), m.begin(), m.end()); }
inline void append_zeros(IndexMap& to, size_t n) { to.insert(to.end(), n, -1); }
// the map of an array [n0][n1][n2][n3][n4] whose element (i0, .., i4) holds blob[at(i0, .., i4)]; map3: of an array [n0][n1][n2]
template <class At> IndexMap map5(int n0, int n1, int n2, int n3, int n4, At at) {
  IndexMap m;
  m.reserve((size_t)n0 * n1 * n2 * n3 * n4);
  for (int i0 = 0; i0 < n0; ++i0) for (int i1 = 0; i1 < n1; ++i1) for (int i2 = 0; i2 < n2; ++i2) for (int i3 = 0; i3 < n3; ++i3) for (int i4 = 0; i4 < n4; ++i4)
    m.push_back((int32_t)at(i0, i1, i2, i3, i4));
  return m;
}
template <class At> IndexMap map3(int n0, int n1, int n2, At at) {
  return map5(1, 1, n0, n1, n2, [&](int, int, int i0, int i1, int i2) { return at(i0, i1, i2); });
}

// ------------------------------------------------------------------------------------------------------------------- sources
// a convolution of the blob, as it is
inline auto conv_source(const ConvAt& c) {
  return [c](int tap, int ci, int co) { return (int32_t)(c.w + flux_conv_index(c.ksz, c.cin, tap, ci, co)); };
}
// ... as the data gradient reads it: input and output swapped, the taps mirrored
inline auto conv_source_transposed(const ConvAt& c) {
  return [c](int tap, int ci, int co) { return (int32_t)(c.w + flux_conv_index(c.ksz, c.cin, c.taps() - 1 - tap, co, ci)); };
}
// The two 1x1 head convolutions concatenated along the output channel -- policy filters, value filters, then zero channels up to the trunk
// width HF = F.  head_channel: where output channel co of that concatenation finds a per-channel vector (bias, a batch-norm vector).
inline auto head_source(const NetLayout& L) {
  const ConvAt p = L.phead(), v = L.vhead();
  return [p, v](int, int ci, int co) {
    return co < p.cout ? (int32_t)(p.w + flux_conv_index(1, p.cin, 0, ci, co)) : co < p.cout + v.cout ? (int32_t)(v.w + flux_conv_index(1, v.cin, 0, ci, co - p.cout)) : -1;
  };
}
inline IndexMap head_channel(const NetLayout& L, size_t in_policy, size_t in_value) {
  const int npf = L.s.npf, nvf = L.s.nvf;
  return map3(1, 1, L.s.F, [&](int, int, int co) { return co < npf ? (int32_t)(in_policy + co) : co < npf + nvf ? (int32_t)(in_value + co - npf) : -1; });
}

// --------------------------------------------------------------------------------------------------------- convolution orders
// k_tower / k_heads_mfma's head convolution (resnet.h, 32x32x2 MFMA): B fragments [tap][Cout/32][Cin/8][64 lanes][4]; lane l of float4 jq,
// component q supplies input channel (l >> 5) Cin/2 + 4 jq + q for output column 32 n + (l & 31)
template <class Src> IndexMap order_tower32(int ntap, int Cin, int Cout, Src src) {
  return map5(ntap, Cout / 32, Cin / 8, 64, 4, [&](int t, int n, int jq, int l, int q) { return src(t, (l >> 5) * (Cin / 2) + 4 * jq + q, 32 * n + (l & 31)); });
}
// k_tower16 and its kin, k_conv16_layer of the trainer (resnet16.h, 16x16x4 MFMA): B fragments [tap][F/16 column tiles][F/16][64 lanes][4];
// lane l of step s = 4 sq + q supplies input channel (g & 1) F/2 + 2 s + (g >> 1), g = l >> 4, for output column 16 ct + (l & 15)
template <class Src> IndexMap order_tower16(int ntap, int F, Src src) {
  return map5(ntap, F / 16, F / 16, 64, 4, [&](int t, int ct, int sq, int l, int q) {
    const int s = 4 * sq + q, g = l >> 4;
    return src(t, (g & 1) * (F / 2) + 2 * s + (g >> 1), 16 * ct + (l & 15));
  });
}
// k_tower16b (resnet16b.h, bf16, 16x16x32 MFMA): B fragments [tap][F/16 column tiles][F/32 k steps][64 lanes][8]; lane l of k step ks
// supplies input channels 32 ks + 8 (l >> 4) + el, el = 0 .. 7, for output column 16 ct + (l & 15)
template <class Src> IndexMap order_tower16b(int ntap, int F, Src src) {
  return map5(ntap, F / 16, F / 32, 64, 8, [&](int t, int ct, int ks, int l, int el) { return src(t, 32 * ks + 8 * (l >> 4) + el, 16 * ct + (l & 15)); });
}
// The stems run as one GEMM over k = tap C + ci, K = 9 C padded to 2 K2 (K2 = ceil(K / 2)).
// k_tower's stem (resnet.h): [F/32][K2][64 lanes]; lane l supplies k = (l >> 5) K2 + j for MFMA j, output column 32 nt + (l & 31)
template <class Src> IndexMap order_stem32(int C, int F, Src src) {
  const int K = 9 * C, K2 = (K + 1) / 2;
  return map3(F / 32, K2, 64, [&](int nt, int j, int l) {
    const int k = (l >> 5) * K2 + j;
    return k < K ? src(k / C, k % C, 32 * nt + (l & 31)) : -1;
  });
}
// k_tower16's stem (resnet16.h): [F/16][NS = ceil(2 K2 / 4)][64 lanes]; lane l of step s takes position p = 4 s + (l >> 4) of the interleaved
// halves, k = (p & 1) K2 + (p >> 1), for output column 16 ct + (l & 15)
template <class Src> IndexMap order_stem16(int C, int F, Src src) {
  const int K = 9 * C, K2 = (K + 1) / 2;
  return map3(F / 16, (2 * K2 + 3) / 4, 64, [&](int ct, int s, int l) {
    const int p = 4 * s + (l >> 4), k = (p & 1) * K2 + (p >> 1);
    return k < K && p < 2 * K2 ? src(k / C, k % C, 16 * ct + (l & 15)) : -1;
  });
}
// the trainer's GEMM matrix of a convolution (train.hip, im2col): [taps cin][cout]
template <class Src> IndexMap order_gemm(int ntap, int Cin, int Cout, Src src) { return map3(ntap, Cin, Cout, src); }

// --------------------------------------------------------------------------------------------------------------- dense orders
// n consecutive blob values, padded with zeros to `width`
inline IndexMap order_vector(size_t at, int n, int width) {
  return map3(1, 1, width, [&](int, int, int i) { return i < n ? (int32_t)(at + i) : -1; });
}
// A dense layer after Flux.flatten of (W, H, nf): Flux W[out + nout (p + P f)] -> k-major [k = p nf + f][width], columns nout .. width zero
// (k_heads and the trainer's GEMMs read it so; the inference policy matrix is APAD wide)
inline IndexMap order_dense(size_t at, int nout, int P, int nf, int width) {
  return map3(P, nf, width, [&](int p, int f, int o) { return o < nout ? (int32_t)(at + o + (size_t)nout * (p + (size_t)P * f)) : -1; });
}
// The MFMA dense heads read the value matrix (`val`, F wide) and the policy matrix (`pol`, APAD wide, A columns used), both k-major as above,
// by tiles of W columns: first the value tiles, then the policy tiles, columns past A zero; per tile [k / G^2][64 lanes][G], G = 64 / W, where
// element e of lane l in step i is W[G (G i + e) + l / W][W tile + l % W].  W = 32, k_heads_mfma (resnet.h, 32x32x2 MFMA, needs npf % 4 ==
// nvf % 4 == 0): MFMA pair i covers k = 4 i .. 4 i + 3, lane l with h = l >> 5 holds (W[4 i + h][o], W[4 i + 2 + h][o]).  W = 16, k_heads16
// (resnet16.h, 16x16x4 MFMA, 32 head filters each): per 16-k block j a float4, element s = W[16 j + 4 s + (l >> 4)][o].
inline IndexMap order_heads(const NetShape& s, const IndexMap& val, const IndexMap& pol, int W) {
  const int G = 64 / W;
  auto tiles = [&](const IndexMap& w, int K, int width, int ncol) {
    return map5(1, (ncol + W - 1) / W, K / (G * G), 64, G, [&](int, int tile, int i, int l, int e) {
      const int k = G * (G * i + e) + l / W, o = W * tile + l % W;
      return o < ncol ? w[(size_t)k * width + o] : -1;
    });
  };
  IndexMap m = tiles(val, s.P * s.nvf, s.F, s.F);
  append(m, tiles(pol, s.P * s.npf, s.APAD, s.A));
  return m;
}

// ------------------------------------------------------------------------------------------------------- an engine's arrays
// The maps behind NetDev / Net16Dev / Net16bDev (az_net_set_params gathers through them).  The tower arrays hold their layers one after
// the other and end in one zero float4 (8 bf16); an array whose kernel cannot run for this shape is that padding alone.
struct NetMaps {
  IndexMap stem_w, s16_w, conv_w, c16_w, c16b_w;            // stems; tower layers for k_tower, k_tower16, k_tower16b (bf16 engines only)
  IndexMap head_w, h16_w, h16b_w, head_b, head_bn;          // the concatenated head convolution in the three orders, its bias [F] and batch norm [4][F]
  IndexMap pol_w, pol_b, val_w, val_b, val2_w, hd_w, hd16_w;
  bool hd_ok, hd16_ok;
  NetMaps(const NetLayout& L, bool bf16) {
    const NetShape& s = L.s;
    const int F = s.F;
    stem_w = order_stem32(s.C, F, conv_source(L.stem()));
    s16_w = order_stem16(s.C, F, conv_source(L.stem()));
    for (int l = 0; l < L.ntower(); ++l) {
      append(conv_w, order_tower32(9, F, F, conv_source(L.tower(l))));
      append(c16_w, order_tower16(9, F, conv_source(L.tower(l))));
      if (bf16) append(c16b_w, order_tower16b(9, F, conv_source(L.tower(l))));
    }
    append_zeros(conv_w, 4); append_zeros(c16_w, 4); append_zeros(c16b_w, 8);
    head_w = order_tower32(1, F, F, head_source(L));
    h16_w = order_tower16(1, F, head_source(L));
    if (bf16) h16b_w = order_tower16b(1, F, head_source(L)); else append_zeros(h16b_w, 8);
    head_b = head_channel(L, L.phead().b, L.vhead().b);
    for (int k = 0; k < 4; ++k) append(head_bn, head_channel(L, L.phead().bn_vec(k), L.vhead().bn_vec(k)));
    pol_w = order_dense(L.pd_w, s.A, s.P, s.npf, s.APAD); pol_b = order_vector(L.pd_b, s.A, s.APAD);
    val_w = order_dense(L.v1_w, F, s.P, s.nvf, F); val_b = order_vector(L.v1_b, F, F);
    val2_w = order_vector(L.v2_w, F, F);
    hd_ok = s.npf % 4 == 0 && s.nvf % 4 == 0;
    hd16_ok = s.npf == 32 && s.nvf == 32;
    if (hd_ok) hd_w = order_heads(s, val_w, pol_w, 32); else append_zeros(hd_w, 4);
    if (hd16_ok) hd16_w = order_heads(s, val_w, pol_w, 16); else append_zeros(hd16_w, 4);
  }
};

// --------------------------------------------------------------------------------------------------------- the trainer's arrays
// The optimiser step's working parameters, work[j] = blob[map[j]]: per convolution its GEMM matrix and, for the tower's F -> F layers, the
// k_conv16_layer fragments for the forward pass (k_tower16's order as it is) and for the data gradient (the same order over the transposed,
// tap-mirrored weight); then the three dense matrices, k-major.  scat: the working entries that carry a gradient back to the blob -- each
// weight once (the GEMM matrices and the dense layers), not the fragment copies.
struct TrainMaps {
  struct Conv { size_t wm, ffwd, fdg; };                    // offsets in the working array; ffwd = fdg = 0 outside the tower
  std::vector<Conv> conv;                                   // as NetLayout::conv
  size_t pd, v1, v2;
  IndexMap map, scat;
  explicit TrainMaps(const NetLayout& L) {
    const NetShape& s = L.s;
    auto add = [&](const IndexMap& m, bool primary) {
      const size_t at = map.size();
      append(map, m);
      if (primary) for (size_t j = at; j < map.size(); ++j) scat.push_back((int32_t)j);
      return at;
    };
    for (size_t l = 0; l < L.conv.size(); ++l) {
      const ConvAt& c = L.conv[l];
      Conv w{add(order_gemm(c.taps(), c.cin, c.cout, conv_source(c)), true), 0, 0};
      if (l >= 1 && (int)l <= L.ntower()) {
        w.ffwd = add(order_tower16(9, s.F, conv_source(c)), false);
        w.fdg = add(order_tower16(9, s.F, conv_source_transposed(c)), false);
      }
      conv.push_back(w);
    }
    pd = add(order_dense(L.pd_w, s.A, s.P, s.npf, s.A), true);
    v1 = add(order_dense(L.v1_w, s.F, s.P, s.nvf, s.F), true);
    v2 = add(order_vector(L.v2_w, s.F, s.F), true);
  }
};
// 0 where the optimiser must not touch the blob: the running mean and variance of every batch norm
inline std::vector<unsigned char> trainable_mask(const NetLayout& L) {
  std::vector<unsigned char> t(L.total, 1);
  for (const ConvAt& c : L.conv) for (int i = 0; i < 2 * c.cout; ++i) t[c.bn_vec(2) + i] = 0;
  return t;
}

// ================================================================================================================== SimpleNet
// NetLib.SimpleNet (src/networks/architectures/simplenet.jl:37-64): with h = width, indim = prod(state_dim), A = num_actions
//   common = flatten, D(indim -> h), D(h -> h) x depth_common;  vhead = D(h -> h) x depth_vhead, Dense(h -> 1, tanh);
//   phead  = D(h -> h) x depth_phead, Dense(h -> A), softmax;   D(i -> o) = Dense(i -> o) + BatchNorm(o, relu) or Dense(i -> o, relu)
// Blob order, as the ResNet's: common, policy head, value head; per D the Flux arrays W(o, i) column-major (W[o + out i]), b(o) and --
// with batch norm only, never zero-filled otherwise -- gamma, beta, running mean, running variance; the final layers W, b.
// The shipped Tic-tac-toe network (games/tictactoe/params.jl: width 200, depth_common 6, batch norm, head depths 1) is 336 410 values,
// of which Flux.trainables counts 332 810 (the 9 x 2 x 200 running statistics are state).
struct SimpleShape { int indim, A, width, depth_common, depth_phead, depth_vhead, use_batch_norm; };
// one Dense (+ BatchNorm) in the blob
struct DenseAt {
  int in, out;
  bool bn, last;                                                  // last: Dense(h -> A) / Dense(h -> 1), no relu in the layer itself
  size_t w, b, bnv;
  size_t bn_vec(int k) const { return bnv + (size_t)k * out; }    // k = 0 .. 3: gamma, beta, running mean, running variance (bn only)
  size_t nw() const { return (size_t)in * out; }
  int32_t at(int i, int o) const { return i < in && o < out ? (int32_t)(w + o + (size_t)out * i) : -1; }   // W(o, i), -1 outside
};
struct SimpleLayout {
  SimpleShape s;
  std::vector<DenseAt> dense;    // [0 .. depth_common] common, then depth_phead D + the policy Dense, then depth_vhead D + the value Dense
  size_t total;
  explicit SimpleLayout(const SimpleShape& sh) : s(sh) {
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += n; return o; };
    auto add = [&](int in, int out, bool last) {
      DenseAt d{in, out, !last && s.use_batch_norm != 0, last, 0, 0, 0};
      d.w = take(d.nw()); d.b = take(out);
      if (d.bn) d.bnv = take(4 * (size_t)out);
      dense.push_back(d);
    };
    add(s.indim, s.width, false);
    for (int l = 0; l < s.depth_common; ++l) add(s.width, s.width, false);
    for (int l = 0; l < s.depth_phead; ++l) add(s.width, s.width, false);
    add(s.width, s.A, true);
    for (int l = 0; l < s.depth_vhead; ++l) add(s.width, s.width, false);
    add(s.width, 1, true);
    total = at;
  }
  int ncommon() const { return 1 + s.depth_common; }
  int pfirst() const { return ncommon(); }                        // first layer of the policy head; its Dense(h -> A) is pfirst() + depth_phead
  int vfirst() const { return ncommon() + s.depth_phead + 1; }    // ... of the value head; its Dense(h -> 1) is the last entry
};
inline int pad_to(int n, int m) { return (n + m - 1) / m * m; }
// k_simplenet (simplenet.h, 16x16x4 MFMA): B fragments of one layer [OP/16 column tiles][KP/16 k blocks][64 lanes][4], KP = in and OP = out
// padded to 16; component q of lane l in k block j supplies input k = 16 j + 4 q + (l >> 4) for output column 16 ct + (l & 15): the
// lane's float4 feeds four consecutive MFMAs, whose k slots (l >> 4) together run k upwards
inline IndexMap order_simple16(const DenseAt& d) {
  return map5(1, pad_to(d.out, 16) / 16, pad_to(d.in, 16) / 16, 64, 4, [&](int, int ct, int j, int l, int q) { return d.at(16 * j + 4 * q + (l >> 4), 16 * ct + (l & 15)); });
}
// the trainer's GEMM matrix of a dense layer, k-major [in][out]
inline IndexMap order_simple_gemm(const DenseAt& d) { return map3(1, d.in, d.out, [&](int, int i, int o) { return d.at(i, o); }); }
// The maps behind SimpleDev: per layer the fragments, and padded to OP its bias and (with batch norm) the four batch-norm vectors
struct SimpleMaps {
  struct Layer { IndexMap w, b, bn[4]; };
  std::vector<Layer> layer;
  explicit SimpleMaps(const SimpleLayout& L) {
    for (const DenseAt& d : L.dense) {
      Layer m;
      const int OP = pad_to(d.out, 16);
      m.w = order_simple16(d);
      m.b = order_vector(d.b, d.out, OP);
      if (d.bn) for (int k = 0; k < 4; ++k) m.bn[k] = order_vector(d.bn_vec(k), d.out, OP);
      layer.push_back(m);
    }
  }
};
// The optimiser step's working matrices of a dense chain, work[j] = blob[map[j]]: every dense matrix once, k-major; scat: all of them
// carry their gradient back to the blob
struct SimpleTrainMaps {
  std::vector<size_t> wm;                                         // offsets in the working array, as SimpleLayout::dense
  IndexMap map, scat;
  explicit SimpleTrainMaps(const SimpleLayout& L) {
    for (const DenseAt& d : L.dense) {
      wm.push_back(map.size());
      append(map, order_simple_gemm(d));
    }
    for (size_t j = 0; j < map.size(); ++j) scat.push_back((int32_t)j);
  }
};
inline std::vector<unsigned char> trainable_mask(const SimpleLayout& L) {
  std::vector<unsigned char> t(L.total, 1);
  for (const DenseAt& d : L.dense) if (d.bn) for (int i = 0; i < 2 * d.out; ++i) t[d.bn_vec(2) + i] = 0;
  return t;
}
