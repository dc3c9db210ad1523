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
//   dR = W2^T dq ; dZ = dR * [Z > 0]            (here: the full 9-action dq row)
//   dO, the attention's dp / da_dst, dh: swarm_bwd.h, the TD kernel's own
//   GCNConv: dh_u = sum_v c_uv dO_v (the normalisation holds no parameter)
// After one block barrier the parameter products over the block's 32 rows, dW1 = dZ^T T,
// dW2 = dq^T R (here), dW = dh^T X and the vectors' ordered column sums (swarm_bwd.h).  Every
// block writes every column 0..N_PARAMS of its slab (column N_PARAMS: 0), so the workspace need
// not be zeroed; rows of graphs past B and slots past N enter every sum as zeros.  No atomics:
// bitwise reproducible.
#pragma once
#include "swarm_bwd.h"

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

  dl_forward<NS, -1, GS, spec_complete_graph(SPEC)>(P, d, N, graph, A.k, A.radius, conv, A.mult, V, true, F);

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
    row_store(TB.dZ[row], p, dz[ct]);
    TB.X[row][p] = F.x[ct][0];
    TB.X[row][4 + p] = F.x[ct][1];
#pragma unroll
    for (int j = 0; j < NS / 4; ++j) TB.cm[row][4 * j + p] = F.cc[ct][j];
    if (p == 0) {
      TB.X[row][8] = 0.0f;
      *reinterpret_cast<float4*>(&L.DQ[row][0]) = make_float4(dqv[ct][0], dqv[ct][1], dqv[ct][2], dqv[ct][3]);
    } else if (p == 1) {
      *reinterpret_cast<float4*>(&L.DQ[row][4]) = make_float4(dqv[ct][4], dqv[ct][5], dqv[ct][6], dqv[ct][7]);
    } else if (p == 2) {
      *reinterpret_cast<float4*>(&L.DQ[row][8]) = make_float4(dqv[ct][8], 0.0f, 0.0f, 0.0f);
    }
  }

  // ---- the per-node backward (swarm_bwd.h): dO, the attention's dp / da_dst, dh
  float dO[CT][2][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    bwd_dO_tile(P, c, p, dz[ct], F.t[ct], nv[ct], dO[ct]);
    row_store(TB.dO[row0 + 16 * ct + c], p, dO[ct]);
  }
  float da_d[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) da_d[ct] = 0.0f;
  if (conv == SWARM_CONV_GAT) {
    float dp[CT][CT][4];
    bwd_attention<NS>(TB.H + row0, F, V.sm->ssrc, dO, nv, c, p, dp, da_d);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int ut = 0; ut < CT; ++ut)
#pragma unroll
        for (int r = 0; r < 4; ++r) TB.dp[row0 + 16 * ct + c][16 * ut + 4 * p + r] = dp[ct][ut][r];
  }
  wave_lds_sync();   // cm / dp / dO rows of this wave's graphs
  bwd_dh<NS, GS>(TB, P, row0, N, conv, nv, da_d, c, p);
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
      const f32x4 acc = bwd_dw_tile(TB, t, c, p);
      if (c < kFeat) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sst(OFF_W + (16 * t + 4 * p + r) * kFeat + c, acc[r]);
      }
    } else if (job == 4) {
      sst((h == 0 ? OFF_B1 : OFF_BIAS) + col, col_sum32(h == 0 ? TB.dZ : TB.dO, col));
    } else if (job == 5) {   // att_src (half 0) / att_dst (half 1); GCNConv: none (the sum can be -0)
      const float acc = bwd_att_col(TB, h == 0 ? TB.das : TB.dad, col);
      sst((h == 0 ? OFF_ATT_SRC : OFF_ATT_DST) + col, conv == SWARM_CONV_GAT ? acc : 0.0f);
    } else {
      if (lane < kActions) {
        sst(OFF_B2 + lane, col_sum32(L.DQ, lane));
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
