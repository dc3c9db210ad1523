// swarm_bwd.h — the hand-written backward of GCN.forward (swarm_dl.h), each piece once: the TD
// kernel (swarm_tdk.h td_body: its pre path before y is known, and its path after B2) and
// swarm_q_backward (swarm_qbk.h qbk_body) are built from these.
//
// A block owns kTdRows = 32 node rows = 32 / NS waves of NS slots (TdLds).  Per wave, in the
// MFMA D layout (swarm_wpg.h; lane (c, p) holds features 16 t + 4 p + r of node 16 ct + c):
//   bwd_dO_tile    dT = W1^T dZ ; dO = dT * (1 - t^2)                       (one column tile)
//   bwd_attention  g_uv = dO_v.h_u ; de_uv = c_uv (g_uv - sum_w c_wv g_wv) ; dp = de * leaky'(p)
//                  da_dst[v] = sum_u dp_uv                                   (GAT only)
//   bwd_dh         da_src[u] = sum_v dp_uv ; dh_u = sum_v c_uv dO_v + da_src att_src + da_dst att_dst
// and per block, over its 32 rows once they are all in LDS:
//   bwd_dw_tile    dW = dH^T X        bwd_att_col   sum_n da[n] H[n][col]
//   col_sum32      the ordered column sum of the bias gradients
// c_uv carries the edge multiplicity; a target without an in-edge has c_uv = 0 for every u and
// adds nothing (no exp is evaluated in the backward).  What differs between the callers stays
// with them: how dZ is formed, the dW1 / dW2 tiles, every mask on a result, and every store to
// a gradient slab (the block-level pieces return their value).  The order of every sum and of
// every MFMA chain here is part of the result: the kernels are compared bit for bit.
#pragma once
#include "swarm_dl.h"

namespace swarm {

// One TD block = 32 node slots = GPB = 32 / NS sampled graphs.  Wave w < GPB runs the
// ONLINE network on graph w (forward on s with activations kept, dQ, backward of the
// per-node vectors); wave GPB + w runs the TARGET network on s' of graph w
// (y = r + gamma max_a Q_tgt), then shares the parameter products.  The parameter
// gradient of the block is a sum over its 32 node rows: MFMA 16x16x4 f32 tiles with the
// node index as K, spread over the waves, each writing its slice of the slab.
constexpr int kTdRows = 32;

template <int NS>
struct TdLds {
  static constexpr int GPB = kTdRows / NS;
  float H[kTdRows][kRow];         // online conv1.lin output
  float T[kTdRows][kRow];         // tanh(conv out)
  float R[kTdRows][kRow];         // relu(lin1)
  // written only after B1; before it, rows NS w .. NS w + NS - 1 of dZ / dO / dH are target
  // wave w's forward scratch (its H / T / R rows): 13.8 KB less LDS per block, so three
  // 256-thread blocks fit a CU (the fused tick at N = 9..16 has 3 blocks per CU)
  float dZ[kTdRows][kRow];        // dL/d lin1 pre-activation
  float dO[kTdRows][kRow];        // dL/d conv out
  float dH[kTdRows][kRow];        // dL/d h
  float X[kTdRows][9];            // node features (k < 8)
  union {
    struct {
      float cm[kTdRows][NS + 1];  // c[target row][source slot]
      float dp[kTdRows][NS + 1];  // dL/d pre-activation of edge (source -> target row)
    };
    WSmall<NS> tgsm[GPB];         // before B1: the target waves' small scratch
  };
  float yq[kTdRows], gq[kTdRows], das[kTdRows], dad[kTdRows], d2[kTdRows];   // yq: gamma max_a Q_target(s')
  int act[kTdRows];
  int tdrop[kTdRows];             // fused tick: the target wave dropped this row's graph (hand-off overrun)
  int prew[GPB];                  // online wave w is on the pre path (swarm_tdk.h td_body)
  int insl[GPB];                  // before B0: online wave w holds a graph of this tick's slot
  WSmall<NS> on[GPB];             // online waves' per-graph scratch
  __device__ WView<NS> target_view(int w) { return WView<NS>{dZ + NS * w, dO + NS * w, dH + NS * w, &tgsm[w]}; }
};

// this lane's 2 x 4 registers of a node's 32-vector to its LDS row
__device__ __forceinline__ void row_store(float* row, int p, const float (&v)[2][4]) {
  *reinterpret_cast<float4*>(row + 4 * p) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
  *reinterpret_cast<float4*>(row + 16 + 4 * p) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
}

// ---- dT^T = W1^T dZ^T on MFMA (the dz registers are the B operand), dO = dT * (1 - t^2) with the
//      forward's tanh registers, for one column tile; a tile that is not live gets zeros
__device__ __forceinline__ void bwd_dO_tile(const float* P, int c, int p, const float (&dz)[2][4],
                                            const float (&th)[2][4], bool live, float (&dO)[2][4]) {
  // W1 fragments first (16 LDS reads in flight), then the two output tiles' chains interleaved
  float w1f[2][2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) w1f[t2][t][r] = P[L_W1 + (16 * t + 4 * p + r) * kWRow + 16 * t2 + c];
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) acc[t2] = mfma16(w1f[t2][t][r], dz[t][r], acc[t2]);
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int r = 0; r < 4; ++r) dO[t2][r] = live ? acc[t2][r] * (1.0f - th[t2][r] * th[t2][r]) : 0.0f;
}

// ---- GAT backward (attention part) of one wave.  g[u][v] = H_u . dO_v on MFMA (A = the wave's H
//      rows, B = the dO registers); lane (c, p) holds g[u = 16 ut + 4 p + r][v = 16 ct + c] and
//      gets dp[ct][ut][r] of that edge; da_d[ct] = sum_u dp, the same in all four row groups
template <int NS>
__device__ __forceinline__ void bwd_attention(const float (*H)[kRow], const DFwd<NS>& F, const float* ssrc,
                                              const float (&dO)[DGeom<NS>::CT][2][4], const bool (&live)[DGeom<NS>::CT],
                                              int c, int p, float (&dp)[DGeom<NS>::CT][DGeom<NS>::CT][4],
                                              float (&da_d)[DGeom<NS>::CT]) {
  constexpr int CT = DGeom<NS>::CT;
  static_assert(NS % 16 == 0, "every MFMA column of a wave is one of its node slots");
  float ah[CT][2][4];
#pragma unroll
  for (int ut = 0; ut < CT; ++ut)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 hv = *reinterpret_cast<const float4*>(&H[16 * ut + c][16 * t + 4 * p]);
      ah[ut][t][0] = hv.x; ah[ut][t][1] = hv.y; ah[ut][t][2] = hv.z; ah[ut][t][3] = hv.w;
    }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float gv[CT][4], cu[CT][4];
    float part = 0.0f;
#pragma unroll
    for (int ut = 0; ut < CT; ++ut) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma16(ah[ut][t][r], dO[ct][t][r], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        cu[ut][r] = F.cr[ct][ut][r];   // coefficient of edge u -> v, u = 16 ut + 4 p + r (the forward's row pick)
        gv[ut][r] = acc[r];
        part = part + cu[ut][r] * gv[ut][r];
      }
    }
    const float Gs = row4_sum(part);
    float dsum = 0.0f;
#pragma unroll
    for (int ut = 0; ut < CT; ++ut)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // in-edges only (cross-graph / absent: c = 0), as selects: ssrc (a slot of this wave) is
        // read unconditionally and the value of an edge that is none is discarded
        const float de = cu[ut][r] * (gv[ut][r] - Gs);
        const float pre = ssrc[16 * ut + 4 * p + r] + F.sdst[ct];
        const float dpe = pre > 0.0f ? de : de * kLeakySlope;
        const float dpu = (cu[ut][r] != 0.0f && live[ct]) ? dpe : 0.0f;
        dsum = dsum + dpu;
        dp[ct][ut][r] = dpu;
      }
    da_d[ct] = row4_sum(dsum);
  }
}

// ---- dh_u = sum_v c[v][u] dO_v (MFMA: A = dO rows, B = C column) + da_src att_src + da_dst att_dst
//      of the wave whose rows start at row0, from its cm / dp / dO rows in LDS (wave-synced by the
//      caller) and da_d of bwd_attention; writes its dH / das / dad rows.  GS slots per graph.
template <int NS, int GS>
__device__ __forceinline__ void bwd_dh(TdLds<NS>& TB, const float* P, int row0, int N, int conv,
                                       const bool (&nv)[DGeom<NS>::CT], const float (&da_d)[DGeom<NS>::CT], int c, int p) {
  constexpr int CT = DGeom<NS>::CT;
  const float4 s0 = *reinterpret_cast<const float4*>(P + L_ATT_SRC + 4 * p);
  const float4 s1 = *reinterpret_cast<const float4*>(P + L_ATT_SRC + 16 + 4 * p);
  const float4 d0 = *reinterpret_cast<const float4*>(P + L_ATT_DST + 4 * p);
  const float4 d1 = *reinterpret_cast<const float4*>(P + L_ATT_DST + 16 + 4 * p);
  const float as[2][4] = {{s0.x, s0.y, s0.z, s0.w}, {s1.x, s1.y, s1.z, s1.w}};
  const float ad[2][4] = {{d0.x, d0.y, d0.z, d0.w}, {d1.x, d1.y, d1.z, d1.w}};
  float ao[2][NS / 4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < NS / 4; ++ks) ao[t][ks] = TB.dO[row0 + 4 * ks + p][16 * t + c];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int u = 16 * ct + c;
    float da_s = 0.0f;
    if (conv == SWARM_CONV_GAT) {   // sum over the targets v of u's own graph, in order
      const int base = (GS < NS) ? (u / GS) * GS : 0;
      float dpj[GS];   // read unconditionally (rows of this wave's graph), summed for j < N
#pragma unroll
      for (int j = 0; j < GS; ++j) dpj[j] = TB.dp[row0 + base + j][u];
#pragma unroll
      for (int j = 0; j < GS; ++j) asm volatile("" : "+v"(dpj[j]));
#pragma unroll
      for (int j = 0; j < GS; ++j) da_s = j < N ? da_s + dpj[j] : da_s;
    }
    const float das = nv[ct] ? da_s : 0.0f, dad = nv[ct] ? da_d[ct] : 0.0f;
    f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NS / 4; ++ks) {
      const float b = TB.cm[row0 + 4 * ks + p][u];
      m0 = mfma16(ao[0][ks], b, m0);
      m1 = mfma16(ao[1][ks], b, m1);
    }
    float dh[2][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dh[0][r] = nv[ct] ? (m0[r] + das * as[0][r]) + dad * ad[0][r] : 0.0f;
      dh[1][r] = nv[ct] ? (m1[r] + das * as[1][r]) + dad * ad[1][r] : 0.0f;
    }
    row_store(TB.dH[row0 + u], p, dh);
    if (p == 0) { TB.das[row0 + u] = das; TB.dad[row0 + u] = dad; }
  }
}

// ---- block-level products over the 32 rows (after the block barrier that completes them); each
//      returns its value and the caller stores it into its slab.
// dW rows 16 t .. 16 t + 15 = sum_n dH[n][f] X[n][k] (MFMA 16x16x4, K = node rows): lane (c, p)
// gets dW[16 t + 4 p + r][k = c], c < kFeat.  Operands read up front and unconditionally (column
// 8 of X is +0: the padding columns c >= kFeat read it), so no LDS round trip sits between two
// MFMAs of the chain
template <int NS>
__device__ __forceinline__ f32x4 bwd_dw_tile(const TdLds<NS>& TB, int t, int c, int p) {
  float ha[kTdRows / 4], xb[kTdRows / 4];
#pragma unroll
  for (int ks = 0; ks < kTdRows / 4; ++ks) {
    const int n = 4 * ks + p;
    ha[ks] = TB.dH[n][16 * t + c];
    xb[ks] = TB.X[n][c < kFeat ? c : 8];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < kTdRows / 4; ++ks) acc = mfma16(ha[ks], xb[ks], acc);
  return acc;
}

// sum_n src[n][col] in row order, every row read first
template <int W>
__device__ __forceinline__ float col_sum32(const float (*src)[W], int col) {
  float v[kTdRows];
#pragma unroll
  for (int n = 0; n < kTdRows; ++n) v[n] = src[n][col];
  float acc = v[0];
#pragma unroll
  for (int n = 1; n < kTdRows; ++n) acc = acc + v[n];
  return acc;
}

// datt_src (da = TB.das) / datt_dst (da = TB.dad) column col: sum_n da[n] H[n][col] in row order
template <int NS>
__device__ __forceinline__ float bwd_att_col(const TdLds<NS>& TB, const float* da, int col) {
  float v[kTdRows];
#pragma unroll
  for (int n = 0; n < kTdRows; ++n) v[n] = da[n] * TB.H[n][col];
  float acc = v[0];
#pragma unroll
  for (int n = 1; n < kTdRows; ++n) acc = acc + v[n];
  return acc;
}

}  // namespace swarm
