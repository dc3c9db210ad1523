// swarm_qbk.h — backward of GCN.forward for a caller-supplied dL/dQ (swarm_q_backward): the
// parameter gradient torch's autograd forms for loss.backward() through model(batch)
// (train_gcn_dqn.py:122-124) on an arbitrary graph, where the TD kernel (swarm_tdk.h) is wired to
// the one-hot dQ of its own loss and replay ring.
//
// Geometry of the TD kernel (swarm_launch.h): a block owns 32 node rows = 32 / NS waves of NS
// slots, a wave NS / GS graphs of GS slots; block b writes gradient slab b (swarm_common.h
// slab_index) and swarm_grad_reduce's kernel sums the slabs in its fixed order.  There is no
// target network here, so a block has only its 32 / NS forward waves.
//
// Per wave: dl_forward on x (graph built from x[:, :2] for kNN / radius, the caller's
// multiplicities for dense) with T / R kept, then
//   dR = W2^T dq ; dZ = dR * [Z > 0] ; dT = W1^T dZ ; dO = dT * (1 - t^2)
//   GAT: g_uv = dO_v.h_u ; de_uv = c_uv (g_uv - sum_w c_wv g_wv) ; dp = de * leaky'(p)
//        da_dst[v] = sum_u dp_uv ; da_src[u] = sum_v dp_uv ; dh_u = sum_v c_uv dO_v + da_src att_src + da_dst att_dst
//   GCNConv: dh_u = sum_v c_uv dO_v (the normalisation holds no parameter)
// c_uv carries the edge multiplicity; a target without an in-edge has c_uv = 0 for every u and
// adds nothing (no exp is evaluated in the backward).  After one block barrier the parameter
// products over the block's 32 rows, dW1 = dZ^T T, dW2 = dq^T R, dW = dh^T X on MFMA 16x16x4
// (node index as K), the vectors as ordered LDS column sums.  Every block writes every column
// 0..N_PARAMS of its slab (column N_PARAMS: 0), so the workspace need not be zeroed; rows of
// graphs past B and slots past N enter every sum as zeros.  No atomics: bitwise reproducible.
#pragma once
#include "swarm_tdk.h"

namespace swarm {

struct QbArgs {
  int B, N, graph, k, conv;
  float radius;
  const float* params;
  const float* x;        // [B*N][7]
  const uint8_t* mult;   // [B][N][N], SWARM_GRAPH_DENSE only
  const float* dq;       // [B*N][9]
  float* slabs;
  int n_slabs;
};

constexpr int kQbDqRow = 12;   // dq row in LDS: 9 actions, then zeros (the dW2 tile's padding columns read [9])

template <int NS>
struct QbSmem {
  TdLds<NS> TB;   // the TD block's images (no target wave uses the rows shared with them)
  __attribute__((aligned(16))) float Pon[N_LDS_PARAMS];
  __attribute__((aligned(16))) float DQ[kTdRows][kQbDqRow];
};

template <int NS, int GS, int SPEC>
__device__ __forceinline__ void qbk_body(QbSmem<NS>& L, const int vb, const QbArgs& A) {
  constexpr int GPB = kTdRows / NS, CT = DGeom<NS>::CT;
  constexpr int GPW = NS / GS;   // graphs per wave
  constexpr int NT = 64 * GPB;
  static_assert(NS % 16 == 0, "every MFMA column of a wave is one of its node slots");
  TdLds<NS>& TB = L.TB;
  const float* P = L.Pon;
  const int wi = threadIdx.x >> 6;
  const int B = A.B, N = A.N;
  DGeom<NS> d = make_dgeom<NS>(0, 1);
  const int lane = d.lane, c = d.c, p = d.p;
  // this lane's graph (dense multiplicities are indexed by it; past B: an in-bounds one, unused)
  d.gid = min(vb * (kTdRows / GS) + wi * GPW + (GS < NS ? c / GS : 0), B - 1);
  const int graph = spec_graph<SPEC>(A.graph);
  const int conv = spec_conv<SPEC>(A.conv);
  const int row0 = wi * NS;
  const WView<NS> V{TB.H + row0, TB.T + row0, TB.R + row0, &TB.on[wi]};
  static_assert(kSlabCols == 16, "slab column blocks of 16");
  float* const slab_base = A.slabs + (size_t)vb * kSlabCols;
  const uint32_t slab_stride = (uint32_t)A.n_slabs * kSlabCols;
  auto sst = [&](int q, float v) { slab_base[(uint32_t)(q >> 4) * slab_stride + (uint32_t)(q & 15)] = v; };

  ParamStage<NT> pon;
  pon.load(A.params, threadIdx.x);
  bool nv[CT];
  DFwd<NS> F;
  float dqv[CT][kActions];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = 16 * ct + c;
    const int gi = (GS < NS) ? n / GS : 0;
    const int jl = (GS < NS) ? n % GS : n;
    const int sid = vb * (kTdRows / GS) + wi * GPW + gi;
    nv[ct] = sid < B && jl < N;
    // rows that are no node alias an in-bounds one and are zeroed after the load
    const size_t node = (size_t)min(sid, B - 1) * N + min(jl, N - 1);
    const float x0 = A.x[node * kFeat + p], x1 = A.x[node * kFeat + min(4 + p, kFeat - 1)];
    F.x[ct][0] = nv[ct] ? x0 : 0.0f;
    F.x[ct][1] = (nv[ct] && 4 + p < kFeat) ? x1 : 0.0f;
#pragma unroll
    for (int a = 0; a < kActions; ++a) {
      const float g = A.dq[node * kActions + a];
      dqv[ct][a] = nv[ct] ? g : 0.0f;
    }
  }
  pon.store(L.Pon, threadIdx.x);
  __syncthreads();   // weight image

  dl_forward<NS, -1, GS>(P, d, N, graph, A.k, A.radius, conv, A.mult, V, true, F);

  // ---- dR = W2^T dq (actions in order), dZ = dR * [z > 0]; the block's images of this wave's rows
  float dz[CT][2][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float dr[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int a = 0; a < kActions; ++a)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 w = *reinterpret_cast<const float4*>(P + L_W2 + a * kWRow + 16 * t + 4 * p);
        dr[t][0] = dr[t][0] + w.x * dqv[ct][a];
        dr[t][1] = dr[t][1] + w.y * dqv[ct][a];
        dr[t][2] = dr[t][2] + w.z * dqv[ct][a];
        dr[t][3] = dr[t][3] + w.w * dqv[ct][a];
      }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dz[ct][t][r] = (nv[ct] && F.zr[ct][t][r] > 0.0f) ? dr[t][r] : 0.0f;
    const int row = row0 + 16 * ct + c;
    *reinterpret_cast<float4*>(&TB.dZ[row][4 * p]) = make_float4(dz[ct][0][0], dz[ct][0][1], dz[ct][0][2], dz[ct][0][3]);
    *reinterpret_cast<float4*>(&TB.dZ[row][16 + 4 * p]) = make_float4(dz[ct][1][0], dz[ct][1][1], dz[ct][1][2], dz[ct][1][3]);
    TB.X[row][p] = F.x[ct][0];
    TB.X[row][4 + p] = F.x[ct][1];
#pragma unroll
    for (int j = 0; j < NS / 4; ++j) TB.cm[row][4 * j + p] = pick4(F.cf[ct], j, p);
    if (p == 0) {
      TB.X[row][8] = 0.0f;
      *reinterpret_cast<float4*>(&L.DQ[row][0]) = make_float4(dqv[ct][0], dqv[ct][1], dqv[ct][2], dqv[ct][3]);
    } else if (p == 1) {
      *reinterpret_cast<float4*>(&L.DQ[row][4]) = make_float4(dqv[ct][4], dqv[ct][5], dqv[ct][6], dqv[ct][7]);
    } else if (p == 2) {
      *reinterpret_cast<float4*>(&L.DQ[row][8]) = make_float4(dqv[ct][8], 0.0f, 0.0f, 0.0f);
    }
  }

  // ---- dT^T = W1^T dZ^T on MFMA (the dz registers are the B operand), dO = dT * (1 - t^2)
  float dO[CT][2][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
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
        for (int t2 = 0; t2 < 2; ++t2) acc[t2] = mfma16(w1f[t2][t][r], dz[ct][t][r], acc[t2]);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dO[ct][t2][r] = nv[ct] ? acc[t2][r] * (1.0f - F.t[ct][t2][r] * F.t[ct][t2][r]) : 0.0f;
    const int row = row0 + 16 * ct + c;
    *reinterpret_cast<float4*>(&TB.dO[row][4 * p]) = make_float4(dO[ct][0][0], dO[ct][0][1], dO[ct][0][2], dO[ct][0][3]);
    *reinterpret_cast<float4*>(&TB.dO[row][16 + 4 * p]) = make_float4(dO[ct][1][0], dO[ct][1][1], dO[ct][1][2], dO[ct][1][3]);
  }
  // ---- GAT backward (attention part).  g[u][v] = H_u . dO_v on MFMA (A = H rows, B = the dO
  //      registers); lane (c, p) holds g[u = 16 ut + 4 p + r][v = 16 ct + c]
  float da_d[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) da_d[ct] = 0.0f;
  WSmall<NS>& sm = *V.sm;
  if (conv == SWARM_CONV_GAT) {
    float ah[CT][2][4];
#pragma unroll
    for (int ut = 0; ut < CT; ++ut) {
      const int u = 16 * ut + c;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 hv = *reinterpret_cast<const float4*>(&TB.H[row0 + u][16 * t + 4 * p]);
        ah[ut][t][0] = hv.x; ah[ut][t][1] = hv.y; ah[ut][t][2] = hv.z; ah[ut][t][3] = hv.w;
      }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int v = 16 * ct + c;
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
          // coefficient of edge u -> v, u = 16 ut + 4 p + r (registers hold every u of target v)
          float cc[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) cc[q] = F.cf[ct][16 * ut + 4 * q + r];
          cu[ut][r] = p == 0 ? cc[0] : (p == 1 ? cc[1] : (p == 2 ? cc[2] : cc[3]));
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
          const int u = 16 * ut + 4 * p + r;
          float dpu = 0.0f;
          if (cu[ut][r] != 0.0f && nv[ct]) {   // in-edges only (cross-graph / absent: c = 0)
            const float de = cu[ut][r] * (gv[ut][r] - Gs);
            const float pre = sm.ssrc[u] + F.sdst[ct];
            dpu = pre > 0.0f ? de : de * kLeakySlope;
          }
          dsum = dsum + dpu;
          TB.dp[row0 + v][u] = dpu;
        }
      da_d[ct] = row4_sum(dsum);
    }
  }
  wave_lds_sync();   // cm / dp / dO rows of this wave's graphs
  // ---- dh_u = sum_v c[v][u] dO_v (MFMA: A = dO rows, B = C column) + da_src att_src + da_dst att_dst
  {
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
        float dpj[GS];
#pragma unroll
        for (int j = 0; j < GS; ++j) dpj[j] = TB.dp[row0 + base + j][u];
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
      *reinterpret_cast<float4*>(&TB.dH[row0 + u][4 * p]) = make_float4(dh[0][0], dh[0][1], dh[0][2], dh[0][3]);
      *reinterpret_cast<float4*>(&TB.dH[row0 + u][16 + 4 * p]) = make_float4(dh[1][0], dh[1][1], dh[1][2], dh[1][3]);
      if (p == 0) { TB.das[row0 + u] = das; TB.dad[row0 + u] = dad; }
    }
  }
  __syncthreads();   // every wave's dZ / T / R / DQ / X / dO / dH / das / dad rows

  // ---- parameter products over the block's 32 rows, spread over its waves; each job writes its
  //      slice of the slab:
  //      0 / 1: dW1 = dZ^T T and dW2 = dq^T R, column half tj (16x16x4 MFMA tiles, K = node rows)
  //      2 / 3: dW rows 0-15 / 16-31 = sum_n dH[n][f] X[n][k]
  //      4: db1 (lanes 0-31) and dbias (lanes 32-63) ; 5: att_src / att_dst (lane halves)
  //      6: db2, and 0 in column N_PARAMS
  const int col = lane & 31, h = lane >> 5;
  for (int job = wi; job < 7; job += GPB) {
    if (job < 2) {
      const int tj = job;
      float a1[2][8], b1[8], a2[8], b2v[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int n = 4 * s + p;
        a1[0][s] = TB.dZ[n][c];
        a1[1][s] = TB.dZ[n][16 + c];
        b1[s] = TB.T[n][16 * tj + c];
        b2v[s] = TB.R[n][16 * tj + c];
        a2[s] = L.DQ[n][c < kActions ? c : kActions];
      }
      // lane (c, p) holds dW1[out = c (+16)][in = 16 tj + 4p .. 4p + 3] and dW2[action = c][in = ...]
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        d0 = mfma16(b1[s], a1[0][s], d0);
        d1 = mfma16(b1[s], a1[1][s], d1);
        d2 = mfma16(b2v[s], a2[s], d2);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sst(OFF_W1 + c * kHidden + 16 * tj + 4 * p + r, d0[r]);
        sst(OFF_W1 + (16 + c) * kHidden + 16 * tj + 4 * p + r, d1[r]);
        if (c < kActions) sst(OFF_W2 + c * kHidden + 16 * tj + 4 * p + r, d2[r]);
      }
    } else if (job < 4) {
      const int t = job - 2;
      float ha[kTdRows / 4], xb[kTdRows / 4];   // column 8 of X is +0: the padding columns read it
#pragma unroll
      for (int ks = 0; ks < kTdRows / 4; ++ks) {
        const int n = 4 * ks + p;
        ha[ks] = TB.dH[n][16 * t + c];
        xb[ks] = TB.X[n][c < kFeat ? c : 8];
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kTdRows / 4; ++ks) acc = mfma16(ha[ks], xb[ks], acc);
      if (c < kFeat) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sst(OFF_W + (16 * t + 4 * p + r) * kFeat + c, acc[r]);
      }
    } else if (job == 4) {
      const float(*src)[kRow] = h == 0 ? TB.dZ : TB.dO;
      float acc = src[0][col];
#pragma unroll
      for (int n = 1; n < kTdRows; ++n) acc = acc + src[n][col];
      sst((h == 0 ? OFF_B1 : OFF_BIAS) + col, acc);
    } else if (job == 5) {   // att_src (half 0) / att_dst (half 1): sum_n da[n] H[n][col]; GCNConv: none
      const float* da = h == 0 ? TB.das : TB.dad;
      float acc = da[0] * TB.H[0][col];
#pragma unroll
      for (int n = 1; n < kTdRows; ++n) acc = acc + da[n] * TB.H[n][col];
      sst((h == 0 ? OFF_ATT_SRC : OFF_ATT_DST) + col, conv == SWARM_CONV_GAT ? acc : 0.0f);
    } else {
      if (lane < kActions) {
        float acc = L.DQ[0][lane];
#pragma unroll
        for (int n = 1; n < kTdRows; ++n) acc = acc + L.DQ[n][lane];
        sst(OFF_B2 + lane, acc);
      } else if (lane == 63) {
        sst(N_PARAMS, 0.0f);
      }
    }
  }
}

template <int NS, int GS, int SPEC>
__global__ __launch_bounds__(64 * (kTdRows / NS)) void q_backward_kernel(QbArgs A) {
  __shared__ QbSmem<NS> L;
  qbk_body<NS, GS, SPEC>(L, blockIdx.x, A);
}

// Launch of q_backward_kernel for A.n_slabs blocks (swarm_qbk.hip).  The kernels are instantiated
// in a translation unit of their own: beside td_kernel they share its inline device functions, and
// the inliner's choices for td_kernel then depend on them (its code changed, same numbers).
__attribute__((visibility("hidden"))) int qbk_launch(const QbArgs& A, hipStream_t stream);

}  // namespace swarm
