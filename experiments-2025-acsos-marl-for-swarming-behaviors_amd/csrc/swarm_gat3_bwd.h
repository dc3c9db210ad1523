// swarm_gat3_bwd.h — backward of the three-layer GAT (swarm_gat3.h) for a caller-supplied dL/dQ
// (swarm_gat3_q_backward): the parameter gradient torch's autograd forms for loss.backward()
// through model(batch) (train_gcn_dqn.py:122-124) when the model is the Flocking checkpoints'
// GCN with its conv2 / conv3 layers.  What swarm_qbk.h is for the one-layer network.
//
// Geometry: the forward's.  One graph per wave in the D layout's lane map (node n = 16 ct + c,
// row group p owns features 2p and 2p + 1), NS = 8 / 16 / 32 slots; at NS = 8 the lanes c >= 8
// shadow slot 7: they compute what its lanes compute and store nothing, and every sum over nodes
// reads LDS rows, so they enter none.  A block holds g3b_waves(NS) such waves.  Each wave leaves
// its 409 parameter partials in its row of the block's PART image; after one block barrier the
// block adds its waves' rows in wave order and writes gradient slab blockIdx.x: 416 columns,
// 409..415 = 0, every column of every slab written, so the workspace need not be zeroed.  A second
// launch (gat3_grad_reduce_kernel) sums the slabs per column in grad_reduce_kernel's grouped
// order.  No atomics: bitwise reproducible.
//
// Per wave (GATConv: PyG 2.5.3, heads 1, no added self loops, duplicate edges by multiplicity):
//   a keeping forward — per layer the input rows X_l, the lin output h_l (LDS), ssrc (LDS),
//   sdst / emax / 1 / den and the activated output (registers of the node's lanes) — with expf and
//   tanhf where the acting forward has __expf / tanh_fast: it is the gradient's forward, not Q's;
//   head   db2 = sum dq ; dW2 = dq^T Z ; dZ = (W2^T dq) [z > 0] ; db1 = sum dZ ; dW1 = dZ^T O3 ;
//          dO3 = W1^T dZ
//   l = 3, 2, 1:
//          dpre = dOut act'          (relu mask; 1 - t^2 for conv1)      dbias = sum dpre
//          g_uv = dpre_v . h_u ; c_uv re-formed from the kept emax, 1 / den (the forward's bits)
//          de_uv = c_uv (g_uv - sum_w c_wv g_wv) ; dp_uv = de_uv leaky'(ssrc_u + sdst_v)
//          da_dst[v] = sum_u dp_uv ; da_src[u] = sum_v dp_uv
//          dh_u = sum_v c_uv dpre_v + da_src[u] att_src + da_dst[u] att_dst
//          datt_src = sum_u da_src[u] h_u ; datt_dst = sum_v da_dst[v] h_v ; dW_l = dh^T X_l
//          l > 1: dOut_(l-1) = W_l^T dh
// Of a target's in-edges, row group p forms the terms (c, g, dp) of the sources u = 4 j + p, and the
// two sums over u are row4_sum's of the groups' partials; the target-to-source transposes (da_src,
// sum_v c_uv dpre_v) go through the wave's CM / DP images.
// A target without an in-edge has every c = 0: its softmax is formed with emax 0 and the exp
// argument 0, nothing of it is 0 / 0, and only dbias sees it.  Slots >= N have x = 0 and dq = 0 and
// no edge: zeros in every sum.  A wave whose graph is >= B writes a zero row and computes nothing.
//
// LDS per wave: G3bWave<NS> = 4.2 / 9.4 / 22.8 KiB at NS = 8 / 16 / 32 (the kept rows, the two
// NS x NS images; the kNN build's scratch overlays the backward's rows, which are written after
// it); per block, with the 416-float weight image and the waves' PART rows: 24.9 / 45.6 / 50.4 KiB
// at 4 / 4 / 2 waves, so 6 / 3 / 3 blocks fit a CU's 160 KiB.
#pragma once
#include "swarm_gat3.h"

namespace swarm {

struct G3bArgs {
  int B, N, graph, k;
  float radius;
  const float* params;   // [409]
  const float* x;        // [B*N][7]
  const uint8_t* mult;   // [B][N][N], SWARM_GRAPH_DENSE only
  const float* dq;       // [B*N][9]
  float* slabs;          // [n_slabs][kG3Cols]
  float* grad;           // [kG3Cols], the reduce launch's
  int n_slabs;
};

constexpr int kG3Cols = 416;   // SWARM_GAT3_GRAD_FLOATS: a slab's columns, and the gradient buffer's floats
static_assert(kG3Cols % 16 == 0 && kG3Cols >= G3_N_PARAMS, "whole column blocks of 16");
// graphs (= waves) of a block
__host__ __device__ constexpr int g3b_waves(int ns) { return ns <= 16 ? 4 : 2; }
inline int g3b_slabs(int ns, int batch) { return (batch + g3b_waves(ns) - 1) / g3b_waves(ns); }

template <int NS>
struct __attribute__((aligned(16))) G3bWave {
  float X[4][NS][kH3];   // input rows of conv1..3 and of lin1: X[l + 1] = the activated output of conv l + 1
  float Z[NS][kH3];      // relu(lin1)
  float DQ[NS][12];      // dq rows (9 actions)
  float ssrc[3][NS];
  float das[NS], dad[NS];
  union __attribute__((aligned(16))) {
    struct {
      float Hh[3][NS][kH3];     // lin outputs
      float D[NS][kH3];         // dZ, then the layer's dpre rows
      float DH[NS][kH3];        // the layer's dh rows
      float CM[NS][NS + 1];     // [target v][source u]: c_uv and dp_uv of the layer
      float DP[NS][NS + 1];
    };
    float ks[3 * NS * NS];      // the kNN build's distance rows (NS^2 floats) and KV scratch (NS^2 pairs)
  };
  __attribute__((aligned(16))) WSmall<NS> sm;   // px / py / knn of the graph phase
};
static_assert(sizeof(KV) == 2 * sizeof(float), "KV scratch of the kNN build");

template <int NS>
struct G3bSmem {
  G3bWave<NS> W[g3b_waves(NS)];
  __attribute__((aligned(16))) float P[kG3Cols];
  float PART[g3b_waves(NS)][kG3Cols];
};
// the header comment's figures
static_assert(sizeof(G3bWave<8>) == 4288 && sizeof(G3bWave<16>) == 9600 && sizeof(G3bWave<32>) == 23296, "LDS per wave");
static_assert(sizeof(G3bSmem<8>) == 25472 && sizeof(G3bSmem<16>) == 46720 && sizeof(G3bSmem<32>) == 51584, "LDS per block");

// out[f * KB + k] = sum_n A[n][f] B[n][k], n in slot order; one lane per output
template <int NS, int SA, int SB>
__device__ __forceinline__ void g3b_outer(float* out, int count, int KB, const float* A, const float* Bm, int lane) {
  for (int i = lane; i < count; i += 64) {
    const int f = i / KB, k = i - f * KB;
    float acc = 0.0f;
#pragma unroll
    for (int n = 0; n < NS; ++n) acc = acc + A[n * SA + f] * Bm[n * SB + k];
    out[i] = acc;
  }
}

// ---- the wave's work in phases (g3b_wave runs them in this order; the TD kernel of swarm_gat3_td.h
// runs the graph and forward phases twice, on rows it loads from the replay, before one backward)
// the graph of the wave: its kind is read at run time; mult is SWARM_GRAPH_DENSE's, of graph gid
struct G3bGraph {
  int N, graph, k;
  float radius;
  const uint8_t* mult;
  int gid;
};
// the lane's registers between the phases: its slots, its nodes' in-edge multiplicities (one graph
// for all layers, forward and backward), and what the keeping forward keeps outside LDS
template <int NS>
struct G3bKeep {
  static constexpr int CT = DGeom<NS>::CT;
  static constexpr bool kKeepM = NS <= 16;
  bool st[CT];   // the lane's slot exists (n < NS): it stores
  int nn[CT];    // the slot it reads
  int mk[kKeepM ? CT : 1][kKeepM ? NS : 1];
  float sdst[3][CT], emx[3][CT], inv[3][CT], outv[3][CT][2];
  float zv[CT][2];   // relu(lin1), the lane's features
};

template <int NS>
__device__ __forceinline__ void g3b_slots(G3bKeep<NS>& K) {
  const int c = threadIdx.x & 15;
#pragma unroll
  for (int ct = 0; ct < G3bKeep<NS>::CT; ++ct) {
    const int n = 16 * ct + c;
    K.st[ct] = n < NS;
    K.nn[ct] = min(n, NS - 1);
  }
}

// loading phase of swarm_gat3_q_backward: x and dq rows of graph gid from the caller's arrays into
// X[0], px / py and DQ; dqv = the lane's nodes' dq rows
template <int NS>
__device__ __forceinline__ void g3b_load(G3bWave<NS>& W, const G3bKeep<NS>& K, const int gid, const G3bArgs& A,
                                         float (&dqv)[DGeom<NS>::CT][kActions]) {
  constexpr int CT = DGeom<NS>::CT;
  const int lane = threadIdx.x & 63, c = lane & 15, p = lane >> 4;
  const int N = A.N;
  WSmall<NS>& sm = W.sm;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = 16 * ct + c;
    const bool nv = n < N;
    // slots that are no node alias an in-bounds one and are zeroed after the load
    const size_t node = (size_t)gid * N + min(n, N - 1);
    const float x0 = A.x[node * kFeat + p], x1 = A.x[node * kFeat + min(4 + p, kFeat - 1)];
    const float xa = nv ? x0 : 0.0f, xb = (nv && 4 + p < kFeat) ? x1 : 0.0f;
#pragma unroll
    for (int a = 0; a < kActions; ++a) {
      const float g = A.dq[node * kActions + a];
      dqv[ct][a] = nv ? g : 0.0f;
    }
    if (K.st[ct]) {
      W.X[0][n][p] = xa;
      W.X[0][n][4 + p] = xb;
      if (p == 0) sm.px[n] = xa;
      if (p == 1) sm.py[n] = xa;
      if (p == 2) {
#pragma unroll
        for (int a = 0; a < kActions; ++a) W.DQ[n][a] = dqv[ct][a];
      }
    }
  }
}

// graph phase, after a loading phase's X[0] / px / py stores: the neighbour masks and the lane's
// in-edge multiplicities
template <int NS>
__device__ __forceinline__ void g3b_graph(G3bWave<NS>& W, const G3bGraph& G, G3bKeep<NS>& K) {
  constexpr int CT = DGeom<NS>::CT;
  const int lane = threadIdx.x & 63, c = lane & 15, p = lane >> 4;
  const int N = G.N, graph = G.graph;
  WSmall<NS>& sm = W.sm;
  wave_lds_sync();
  // ---- neighbour masks: gat3_forward's graph phase, its scratch in ks (no backward row is live yet)
  if (graph == SWARM_GRAPH_KNN) {
    if constexpr (NS <= 16) {
      knn_masks_wave<NS, NS>(lane, N, G.k, sm, W.ks, reinterpret_cast<KV*>(W.ks + NS * NS));
    } else {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int n = 16 * ct + c;
        KV* q = reinterpret_cast<KV*>(W.ks + NS * NS) + K.nn[ct] * NS;
        if (n < NS && p == 0) sm.knn[n] = (n < N) ? knn_mask_node<NS, NS>(n, N, G.k, sm, q) : 0u;
      }
    }
    wave_lds_sync();
  } else if (graph == SWARM_GRAPH_RADIUS) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = 16 * ct + c;
      if (n < NS && p == 0) sm.knn[n] = radius_mask_node<NS, NS>(n, N, G.radius, sm);
    }
    wave_lds_sync();
  }
  if constexpr (G3bKeep<NS>::kKeepM) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) in_mults<NS>(K.nn[ct], N, graph, sm, G.mult, G.gid, K.mk[ct]);
  }
}
// in-edge multiplicities of the lane's node of column tile ct
template <int NS>
__device__ __forceinline__ void g3b_mults(const G3bWave<NS>& W, const G3bGraph& G, const G3bKeep<NS>& K, int ct,
                                          int (&m)[NS]) {
  if constexpr (G3bKeep<NS>::kKeepM) {
#pragma unroll
    for (int u = 0; u < NS; ++u) m[u] = K.mk[ct][u];
  } else {
    in_mults<NS>(K.nn[ct], G.N, G.graph, W.sm, G.mult, G.gid, m);
  }
}

// the keeping forward on X[0] with the weights P: conv1..3 and lin1 + relu (Z rows stored, not synced)
template <int NS>
__device__ __forceinline__ void g3b_forward(const float* __restrict__ P, G3bWave<NS>& W, const G3bGraph& G,
                                            G3bKeep<NS>& Kp) {
  constexpr int CT = DGeom<NS>::CT;
  const int c = threadIdx.x & 15, p = (threadIdx.x & 63) >> 4;
  const bool (&st)[CT] = Kp.st;
  const int (&nn)[CT] = Kp.nn;
  float (&sdst)[3][CT] = Kp.sdst, (&emx)[3][CT] = Kp.emx, (&inv)[3][CT] = Kp.inv, (&outv)[3][CT][2] = Kp.outv;
  float (&zv)[CT][2] = Kp.zv;
  auto mults = [&](int ct, int (&m)[NS]) { g3b_mults<NS>(W, G, Kp, ct, m); };

#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const float* Pc = P + g3_conv_off(l);
    const int K = l == 0 ? kFeat : kH3;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float x[kH3], h[2];
      load_row8(&W.X[l][nn[ct]][0], x);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* w = Pc + G3_W + (2 * p + i) * K;
        float acc = 0.0f;
#pragma unroll
        for (int kk = 0; kk < kH3; ++kk)
          if (kk < K) acc = acc + w[kk] * x[kk];
        h[i] = acc;
      }
      const float ps = h[0] * Pc[G3_ATT_SRC + 2 * p] + h[1] * Pc[G3_ATT_SRC + 2 * p + 1];
      const float pd = h[0] * Pc[G3_ATT_DST + 2 * p] + h[1] * Pc[G3_ATT_DST + 2 * p + 1];
      const float ss = row4_sum(ps);
      sdst[l][ct] = row4_sum(pd);
      if (st[ct]) {
        const int n = 16 * ct + c;
        *reinterpret_cast<float2*>(&W.Hh[l][n][2 * p]) = make_float2(h[0], h[1]);
        if (p == 0) W.ssrc[l][n] = ss;
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      int m[NS];
      mults(ct, m);
      float e[NS];
      float emax = -INFINITY;
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        e[u] = leaky(W.ssrc[l][u] + sdst[l][ct]);
        emax = m[u] > 0 ? fmaxf(emax, e[u]) : emax;
      }
      emax = emax > -INFINITY ? emax : 0.0f;   // no in-edge
      float den = 0.0f;
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const float ex = expf(m[u] > 0 ? e[u] - emax : 0.0f);
        e[u] = m[u] > 0 ? ex : 0.0f;
        den = den + (float)m[u] * e[u];
      }
      const float iv = 1.0f / (den + 1e-16f);
      float o0 = 0.0f, o1 = 0.0f;
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const float cf = (float)m[u] * (e[u] * iv);
        const float2 hu = *reinterpret_cast<const float2*>(&W.Hh[l][u][2 * p]);
        o0 = o0 + cf * hu.x;
        o1 = o1 + cf * hu.y;
      }
      o0 = o0 + Pc[G3_BIAS + 2 * p];
      o1 = o1 + Pc[G3_BIAS + 2 * p + 1];
      if (l == 0) { o0 = tanhf(o0); o1 = tanhf(o1); }
      else { o0 = o0 > 0.0f ? o0 : 0.0f; o1 = o1 > 0.0f ? o1 : 0.0f; }
      outv[l][ct][0] = o0;
      outv[l][ct][1] = o1;
      emx[l][ct] = emax;
      inv[l][ct] = iv;
      if (st[ct]) *reinterpret_cast<float2*>(&W.X[l + 1][16 * ct + c][2 * p]) = make_float2(o0, o1);
    }
    wave_lds_sync();
  }
  // lin1 + relu
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float x[kH3];
    load_row8(&W.X[3][nn[ct]][0], x);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float* w = P + G3_LIN1_W + (2 * p + i) * kH3;
      float acc = 0.0f;
#pragma unroll
      for (int kk = 0; kk < kH3; ++kk) acc = acc + w[kk] * x[kk];
      acc = acc + P[G3_LIN1_B + 2 * p + i];
      zv[ct][i] = acc > 0.0f ? acc : 0.0f;
    }
    if (st[ct]) *reinterpret_cast<float2*>(&W.Z[16 * ct + c][2 * p]) = make_float2(zv[ct][0], zv[ct][1]);
  }
}

// the backward for the lane's dq rows dqv (their copies in DQ): the head and conv3, conv2, conv1;
// the wave's 409 partials into part
template <int NS>
__device__ __forceinline__ void g3b_backward(const float* __restrict__ P, G3bWave<NS>& W, float* __restrict__ part,
                                             const G3bGraph& G, const G3bKeep<NS>& Kp,
                                             const float (&dqv)[DGeom<NS>::CT][kActions]) {
  constexpr int CT = DGeom<NS>::CT;
  const int lane = threadIdx.x & 63, c = lane & 15, p = lane >> 4;
  const bool pb0 = (p & 1) != 0, pb1 = (p & 2) != 0;
  const bool (&st)[CT] = Kp.st;
  const int (&nn)[CT] = Kp.nn;
  const float (&sdst)[3][CT] = Kp.sdst, (&emx)[3][CT] = Kp.emx, (&inv)[3][CT] = Kp.inv, (&outv)[3][CT][2] = Kp.outv;
  const float (&zv)[CT][2] = Kp.zv;
  auto mults = [&](int ct, int (&m)[NS]) { g3b_mults<NS>(W, G, Kp, ct, m); };

  // ---- head: dZ = (W2^T dq) [z > 0], dO3 = W1^T dZ
  float dO[CT][2];   // d(loss) / d(activated output) of the layer below, the lane's features
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float dz[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int a = 0; a < kActions; ++a) acc = acc + P[G3_LIN2_W + a * kH3 + 2 * p + i] * dqv[ct][a];
      dz[i] = zv[ct][i] > 0.0f ? acc : 0.0f;
    }
    if (st[ct]) *reinterpret_cast<float2*>(&W.D[16 * ct + c][2 * p]) = make_float2(dz[0], dz[1]);
  }
  wave_lds_sync();   // Z / D rows
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float dzr[kH3];
    load_row8(&W.D[nn[ct]][0], dzr);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < kH3; ++j) acc = acc + P[G3_LIN1_W + j * kH3 + 2 * p + i] * dzr[j];
      dO[ct][i] = acc;
    }
  }
  {
    const float one = 1.0f;   // db = sum_n rows[n][f] = the outer product with a column of ones
    g3b_outer<NS, 12, 0>(part + G3_LIN2_B, kActions, 1, &W.DQ[0][0], &one, lane);
    g3b_outer<NS, 12, kH3>(part + G3_LIN2_W, kActions * kH3, kH3, &W.DQ[0][0], &W.Z[0][0], lane);
    g3b_outer<NS, kH3, 0>(part + G3_LIN1_B, kH3, 1, &W.D[0][0], &one, lane);
    g3b_outer<NS, kH3, kH3>(part + G3_LIN1_W, kH3 * kH3, kH3, &W.D[0][0], &W.X[3][0][0], lane);
  }
  wave_lds_sync();   // D is rewritten

  // ---- conv3, conv2, conv1 (the layer as a compile-time constant: three copies of the body)
  auto layer_backward = [&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const float* Pc = P + g3_conv_off(l);
    constexpr int K = l == 0 ? kFeat : kH3;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float dpre[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float o = outv[l][ct][i];
        dpre[i] = l == 0 ? dO[ct][i] * (1.0f - o * o) : (o > 0.0f ? dO[ct][i] : 0.0f);
      }
      if (st[ct]) *reinterpret_cast<float2*>(&W.D[16 * ct + c][2 * p]) = make_float2(dpre[0], dpre[1]);
    }
    wave_lds_sync();
    // the node as a target v: c_uv, g_uv, dp_uv of its in-edges
    float dadv[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float dr[kH3];
      load_row8(&W.D[nn[ct]][0], dr);
      int m[NS];
      mults(ct, m);
      // row group p takes the sources u = 4 j + p; the two sums over u meet in row4_sum
      float cf[NS / 4], g[NS / 4];
      bool pos[NS / 4];
      float sp = 0.0f;
#pragma unroll
      for (int j = 0; j < NS / 4; ++j) {
        const int u = 4 * j + p;
        const int mu = sel4(pb0, pb1, m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]);
        const float raw = W.ssrc[l][u] + sdst[l][ct];
        const float e = leaky(raw);
        const float ex = expf(mu > 0 ? e - emx[l][ct] : 0.0f);
        pos[j] = raw > 0.0f;
        cf[j] = (float)mu * ((mu > 0 ? ex : 0.0f) * inv[l][ct]);
        float hu[kH3];
        load_row8(&W.Hh[l][u][0], hu);
        float acc = 0.0f;
#pragma unroll
        for (int f = 0; f < kH3; ++f) acc = acc + dr[f] * hu[f];
        g[j] = acc;
        sp = sp + cf[j] * acc;
      }
      const float s = row4_sum(sp);
      float ddp = 0.0f;
#pragma unroll
      for (int j = 0; j < NS / 4; ++j) {
        const float de = cf[j] * (g[j] - s);
        const float dp = pos[j] ? de : de * kLeakySlope;
        ddp = ddp + dp;
        if (st[ct]) {
          W.CM[16 * ct + c][4 * j + p] = cf[j];
          W.DP[16 * ct + c][4 * j + p] = dp;
        }
      }
      const float dd = row4_sum(ddp);
      dadv[ct] = dd;
      if (st[ct] && p == 0) W.dad[16 * ct + c] = dd;
    }
    wave_lds_sync();
    // the node as a source u: da_src, dh
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int u = nn[ct];
      float ds = 0.0f, a0 = 0.0f, a1 = 0.0f;
#pragma unroll
      for (int v = 0; v < NS; ++v) {
        ds = ds + W.DP[v][u];
        const float cv = W.CM[v][u];
        const float2 dv = *reinterpret_cast<const float2*>(&W.D[v][2 * p]);
        a0 = a0 + cv * dv.x;
        a1 = a1 + cv * dv.y;
      }
      const float h0 = a0 + ds * Pc[G3_ATT_SRC + 2 * p] + dadv[ct] * Pc[G3_ATT_DST + 2 * p];
      const float h1 = a1 + ds * Pc[G3_ATT_SRC + 2 * p + 1] + dadv[ct] * Pc[G3_ATT_DST + 2 * p + 1];
      if (st[ct]) {
        *reinterpret_cast<float2*>(&W.DH[16 * ct + c][2 * p]) = make_float2(h0, h1);
        if (p == 0) W.das[16 * ct + c] = ds;
      }
    }
    wave_lds_sync();
    if (l > 0) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        float dhr[kH3];
        load_row8(&W.DH[nn[ct]][0], dhr);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float acc = 0.0f;
#pragma unroll
          for (int f = 0; f < kH3; ++f) acc = acc + Pc[G3_W + f * kH3 + 2 * p + i] * dhr[f];
          dO[ct][i] = acc;
        }
      }
    }
    {
      const float one = 1.0f;
      float* po = part + g3_conv_off(l);
      g3b_outer<NS, kH3, kH3>(po + G3_W, kH3 * K, K, &W.DH[0][0], &W.X[l][0][0], lane);
      g3b_outer<NS, kH3, 0>(po + G3_BIAS, kH3, 1, &W.D[0][0], &one, lane);
      g3b_outer<NS, kH3, 1>(po + G3_ATT_SRC, kH3, 1, &W.Hh[l][0][0], W.das, lane);
      g3b_outer<NS, kH3, 1>(po + G3_ATT_DST, kH3, 1, &W.Hh[l][0][0], W.dad, lane);
    }
    wave_lds_sync();   // D / DH / CM / DP / das / dad are rewritten
  };
  layer_backward(std::integral_constant<int, 2>{});
  layer_backward(std::integral_constant<int, 1>{});
  layer_backward(std::integral_constant<int, 0>{});
}

template <int NS>
__device__ __forceinline__ void g3b_wave(const float* __restrict__ P, G3bWave<NS>& W, float* __restrict__ part,
                                         const int gid, const G3bArgs& A) {
  const G3bGraph G = {A.N, A.graph, A.k, A.radius, A.mult, gid};
  G3bKeep<NS> K;
  float dqv[DGeom<NS>::CT][kActions];
  g3b_slots<NS>(K);
  g3b_load<NS>(W, K, gid, A, dqv);
  g3b_graph<NS>(W, G, K);
  g3b_forward<NS>(P, W, G, K);
  g3b_backward<NS>(P, W, part, G, K, dqv);
}

template <int NS>
__global__ __launch_bounds__(64 * g3b_waves(NS)) void gat3_backward_kernel(G3bArgs A) {
  constexpr int WPB = g3b_waves(NS), NT = 64 * WPB;
  __shared__ G3bSmem<NS> L;
  for (int i = threadIdx.x; i < kG3Cols; i += NT) L.P[i] = i < G3_N_PARAMS ? A.params[i] : 0.0f;
  __syncthreads();   // weight image
  const int wi = threadIdx.x >> 6;
  const int gid = (int)blockIdx.x * WPB + wi;
  if (gid < A.B) {
    g3b_wave<NS>(L.P, L.W[wi], L.PART[wi], gid, A);
  } else {
    for (int i = threadIdx.x & 63; i < G3_N_PARAMS; i += 64) L.PART[wi][i] = 0.0f;
  }
  __syncthreads();   // every wave's partial row
  float* slab = A.slabs + (size_t)blockIdx.x * kG3Cols;
  for (int col = threadIdx.x; col < kG3Cols; col += NT) {
    float v = 0.0f;
    if (col < G3_N_PARAMS) {
      v = L.PART[0][col];
#pragma unroll
      for (int w = 1; w < WPB; ++w) v = v + L.PART[w][col];
    }
    slab[col] = v;
  }
}

// ---- the slab sum: grad_reduce_kernel's order (swarm_reduce_body.h) on 26 column blocks of 16:
// 64 groups of consecutive slabs per column, each summed in slab order, then the groups in runs of
// eight, then the runs
constexpr int kG3RedCols = 16, kG3RedGroups = 64;
constexpr int kG3RedBlocks = kG3Cols / kG3RedCols;

// LOSS = 1 (the TD path, swarm_gat3_td.h): column 409, the batch's sum of squared TD errors, is
// carried through as well; 0: grad[409..415] = 0
struct G3RedArgs {
  const float* slabs;   // [n_slabs][kG3Cols]
  int n_slabs;
  float* grad;          // [kG3Cols]
};
struct G3RedSmem {
  float part[kG3RedGroups][kG3RedCols];
  float part2[kG3RedGroups / 8][kG3RedCols];
};
// column block bx of the slab sum: gat3_grad_reduce_kernel's block, and block (bx, m) of the
// population's (swarm_pop_gat3.hip) with member m's slabs and grad in A
template <int LOSS>
__device__ __forceinline__ void g3_reduce_block(G3RedSmem& L, const int bx, const G3RedArgs& A) {
  const float* __restrict__ slabs = A.slabs;
  float* __restrict__ grad = A.grad;
  const int n_slabs = A.n_slabs;
  const int c = threadIdx.x % kG3RedCols, q = threadIdx.x / kG3RedCols;
  const int col = bx * kG3RedCols + c;
  const int per = (n_slabs + kG3RedGroups - 1) / kG3RedGroups;
  const int b0 = min(n_slabs, q * per), b1 = min(n_slabs, b0 + per);
  float s = 0.0f;
  for (int b = b0; b < b1; ++b) s = s + slabs[(size_t)b * kG3Cols + col];
  L.part[q][c] = s;
  __syncthreads();
  if (q < kG3RedGroups / 8) {
    float r = L.part[8 * q][c];
#pragma unroll
    for (int gi = 1; gi < 8; ++gi) r = r + L.part[8 * q + gi][c];
    L.part2[q][c] = r;
  }
  __syncthreads();
  if (q == 0) {
    float tot = L.part2[0][c];
#pragma unroll
    for (int gi = 1; gi < kG3RedGroups / 8; ++gi) tot = tot + L.part2[gi][c];
    grad[col] = col < G3_N_PARAMS + LOSS ? tot : 0.0f;
  }
}

template <int LOSS>
__global__ __launch_bounds__(kG3RedCols * kG3RedGroups) void gat3_grad_reduce_kernel(const float* __restrict__ slabs,
                                                                                    int n_slabs,
                                                                                    float* __restrict__ grad) {
  __shared__ G3RedSmem L;
  g3_reduce_block<LOSS>(L, blockIdx.x, G3RedArgs{slabs, n_slabs, grad});
}

// The two launches (swarm_gat3_bwd.hip).  The kernels are instantiated in a translation unit of
// their own, for swarm_qbk.h's reason: no other kernel's code may depend on them.
__attribute__((visibility("hidden"))) int gat3_bwd_launch(const G3bArgs& A, hipStream_t stream);

}  // namespace swarm
