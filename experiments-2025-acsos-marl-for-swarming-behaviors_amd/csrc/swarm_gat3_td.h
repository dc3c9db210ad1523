// swarm_gat3_td.h — the learner of the three-layer GAT (swarm_gat3.h) on the unfused device path:
// the TD-loss gradient of a replay batch (swarm_gat3_td_grad) and clip + Adam + target sync for its
// 409 parameters (swarm_gat3_adam_step).  What td_kernel + grad_reduce_kernel + adam_kernel are for
// the one-layer network.
//
// Reference: DQNTrainer.train_step_dqn (train_gcn_dqn.py:112-137) with the GCN class's conv2 / conv3
// layers (:54-55, :65-68): sample (:38-45), y = r + gamma max_a Q_target(s') (:119-121), MSELoss
// (:122-123), backward (:124), clip_grad_norm_(1) + Adam (:125-126), target sync (:131-133).
//
// gat3_td_kernel<NS>: gat3_backward_kernel's geometry (swarm_gat3_bwd.h): one sampled graph per wave
// in the forward's lane map, g3b_waves(NS) waves per block, NS = 8 / 16 / 32, the graph kind read at
// run time.  Batch position i = blockIdx.x * WPB + wave; its graph id is sample_in[i] clamped into
// the ring, or sample_index(i) under swarm_td_grad's keys.  The wave then runs, in order:
//   the skip rule (the whole grid alike): fewer than `batch` graphs in the ring -> every column of
//       every slab 0, nothing else;
//   the target pass on s': features as node_x forms them, the graph from the positions of s', the
//       keeping forward's arithmetic (expf, tanhf: y enters every gradient term) with the TARGET
//       weights, lin2, y = r + gamma max_a Q; its rows live in the wave's LDS until the online pass
//       overwrites them, and only y stays, in the registers of the node's lanes;
//   the online pass on s: g3b_graph + g3b_forward with the online weights, Q at the taken action,
//       td = Q[a] - y, dq[n][a'] = (a' == a) ? grad_scale td : 0 with grad_scale = fp32(2 / (batch N))
//       (MSELoss mean); slots >= N have dq = 0;
//   g3b_backward, unchanged.
// Column 409 of the wave's PART row is its sum of td^2 over the nodes in slot order; the block's
// slab sum and gat3_grad_reduce_kernel<1> carry it through: grad[409] = the batch's sum of squared
// TD errors, grad[410..415] = 0.  No atomics, every column of every slab written: bitwise
// reproducible, capturable.
//
// LDS per block: G3bSmem<NS> plus a second 416-float weight image (the target's): 26.5 / 47.3 /
// 52.0 KiB at NS = 8 / 16 / 32, so still 6 / 3 / 3 blocks on a CU's 160 KiB.
//
// gat3_adam_kernel: one block of 128 threads, thread t holding float4 t of the 416-float rows
// (104 float4s; floats 409..415 are no parameters: they count 0 in the norm and are never stored).
// adam_kernel's unfused semantics field for field, with adam_elem and the control block's scalars.
// The squared norm has ONE summation order: d[t] = ((g0^2 + g1^2) + g2^2) + g3^2 of float4 t;
// sq[j] = quad_sum of d[4j..4j+3] = (d[4j] + d[4j+1]) + (d[4j+2] + d[4j+3]) for the 26 groups of 16
// parameters; then wave_sum over lanes l = 0..63 of (l < 32 ? sq[l] : 0) (sq[26..31] = 0).
#pragma once
#include "swarm_adam.h"
#include "swarm_gat3_bwd.h"
#include "swarm_launch.h"

namespace swarm {

struct G3tArgs {
  int S, B, N, graph, k, env_offset;
  uint32_t k0, k1;
  float radius, gamma, grad_scale;
  const float* params;   // [409] online
  const float* target;   // [409]
  swarm_replay replay;
  const swarm_ctrl* ctrl;
  const int32_t* sample_in;   // [S] or null
  int32_t* sample_out;        // [S] or null
  float* slabs;               // [n_slabs][kG3Cols]
  float* grad;                // [kG3Cols], the reduce launch's
  int n_slabs;
};

constexpr int kG3LossCol = G3_N_PARAMS;   // column 409: the sum of squared TD errors
static_assert(kG3LossCol < kG3Cols, "the loss column lies in the slab");

template <int NS>
struct G3tSmem {
  G3bWave<NS> W[g3b_waves(NS)];
  __attribute__((aligned(16))) float P[kG3Cols];    // online weights
  __attribute__((aligned(16))) float PT[kG3Cols];   // target weights
  float PART[g3b_waves(NS)][kG3Cols];
};
// the header comment's figures: G3bSmem + one weight image
static_assert(sizeof(G3tSmem<8>) == sizeof(G3bSmem<8>) + 4 * kG3Cols && sizeof(G3tSmem<8>) == 27136, "LDS per block");
static_assert(sizeof(G3tSmem<16>) == 48384 && sizeof(G3tSmem<32>) == 53248, "LDS per block");
static_assert(6 * sizeof(G3tSmem<8>) <= 160 * 1024 && 3 * sizeof(G3tSmem<16>) <= 160 * 1024 &&
              3 * sizeof(G3tSmem<32>) <= 160 * 1024, "blocks per CU");

template <int NS>
__device__ __forceinline__ void g3t_wave(const float* __restrict__ Pon, const float* __restrict__ Ptg, G3bWave<NS>& W,
                                         float* __restrict__ part, const uint32_t gid, const G3tArgs& A) {
  constexpr int CT = DGeom<NS>::CT;
  const int lane = threadIdx.x & 63, c = lane & 15, p = lane >> 4;
  const int N = A.N;
  WSmall<NS>& sm = W.sm;
  G3bKeep<NS> K;
  g3b_slots<NS>(K);
  // ---- the graph's replay rows: node n of graph gid = slot gid / B, env gid % B
  float4 s0[CT], s1[CT];
  float rew[CT];
  int act[CT];
  bool nv[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = 16 * ct + c;
    nv[ct] = n < N;
    // slots that are no node alias an in-bounds one and are zeroed after the load
    const size_t ri = ((size_t)(gid / (uint32_t)A.B) * A.B + gid % (uint32_t)A.B) * N + min(n, N - 1);
    s0[ct] = reinterpret_cast<const float4*>(A.replay.s)[ri];
    s1[ct] = reinterpret_cast<const float4*>(A.replay.s_next)[ri];
    rew[ct] = A.replay.r[ri];
    act[ct] = min((int)A.replay.a[ri], kActions - 1);
  }
  // loading phase: the features of a state's nodes (node_x) into X[0], px / py
  auto put_x = [&](const float4 (&s)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = 16 * ct + c;
      float x[2];
      node_x(s[ct].x, s[ct].y, s[ct].z, s[ct].w, n, p, x);
      const float xa = nv[ct] ? x[0] : 0.0f, xb = nv[ct] ? x[1] : 0.0f;
      if (K.st[ct]) {
        W.X[0][n][p] = xa;
        W.X[0][n][4 + p] = xb;
        if (p == 0) sm.px[n] = xa;
        if (p == 1) sm.py[n] = xa;
      }
    }
  };
  const G3bGraph G = {N, A.graph, A.k, A.radius, nullptr, 0};

  // ---- target pass on s': y = r + gamma max_a Q_target
  put_x(s1);
  g3b_graph<NS>(W, G, K);
  g3b_forward<NS>(Ptg, W, G, K);
  wave_lds_sync();   // Z rows
  float y[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float z[kH3];
    load_row8(&W.Z[K.nn[ct]][0], z);
    float qmax = -INFINITY;
#pragma unroll
    for (int a = 0; a < kActions; ++a) {
      const float* w = Ptg + G3_LIN2_W + a * kH3;
      float acc = 0.0f;
#pragma unroll
      for (int kk = 0; kk < kH3; ++kk) acc = acc + w[kk] * z[kk];
      qmax = fmaxf(qmax, acc + Ptg[G3_LIN2_B + a]);
    }
    y[ct] = rew[ct] + A.gamma * qmax;
  }
  wave_lds_sync();   // the target pass's rows are read: the online pass overwrites them

  // ---- online pass on s: the keeping forward, Q at the taken action, dq
  put_x(s0);
  g3b_graph<NS>(W, G, K);
  g3b_forward<NS>(Pon, W, G, K);
  wave_lds_sync();   // Z rows
  float dqv[CT][kActions];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = 16 * ct + c;
    float z[kH3];
    load_row8(&W.Z[K.nn[ct]][0], z);
    const float* w = Pon + G3_LIN2_W + act[ct] * kH3;
    float acc = 0.0f;
#pragma unroll
    for (int kk = 0; kk < kH3; ++kk) acc = acc + w[kk] * z[kk];
    const float qa = acc + Pon[G3_LIN2_B + act[ct]];
    const float td = nv[ct] ? qa - y[ct] : 0.0f;
    const float gq = td * A.grad_scale;
#pragma unroll
    for (int a = 0; a < kActions; ++a) dqv[ct][a] = a == act[ct] ? gq : 0.0f;
    if (K.st[ct]) {
      if (p == 0) W.das[n] = td;   // free until conv3's backward writes it
      if (p == 2) {
#pragma unroll
        for (int a = 0; a < kActions; ++a) W.DQ[n][a] = dqv[ct][a];
      }
    }
  }
  wave_lds_sync();   // td / DQ rows
  {
    float acc = 0.0f;   // sum of td^2 in slot order (slots >= N hold 0)
#pragma unroll
    for (int n = 0; n < NS; ++n) acc = acc + W.das[n] * W.das[n];
    if (lane == 0) part[kG3LossCol] = acc;
  }
  g3b_backward<NS>(Pon, W, part, G, K, dqv);
}

// TD block bx of a batch: gat3_td_kernel's block, and block (bx, m) of the population's
// (swarm_pop_gat3.hip) with member m's keys, weights, ring, ctrl, slabs and sample_out in A
template <int NS>
__device__ __forceinline__ void g3t_block(G3tSmem<NS>& L, const int bx, const G3tArgs& A) {
  constexpr int WPB = g3b_waves(NS), NT = 64 * WPB;
  float* slab = A.slabs + (size_t)bx * kG3Cols;
  const uint32_t cap = (uint32_t)A.replay.capacity;
  const uint32_t filled = A.ctrl->filled_slots;
  const uint32_t valid_slots = filled + 1 < cap ? filled + 1 : cap;
  const uint32_t n_graphs = valid_slots * (uint32_t)A.B;
  // ---- skip while the replay holds fewer than `batch` graphs (train_gcn_dqn.py:113-115)
  if (n_graphs < (uint32_t)A.S) {
    for (int col = threadIdx.x; col < kG3Cols; col += NT) slab[col] = 0.0f;
    return;
  }
  for (int i = threadIdx.x; i < kG3Cols; i += NT) {
    L.P[i] = i < G3_N_PARAMS ? A.params[i] : 0.0f;
    L.PT[i] = i < G3_N_PARAMS ? A.target[i] : 0.0f;
  }
  __syncthreads();   // weight images
  const int wi = threadIdx.x >> 6;
  const int i = (int)bx * WPB + wi;
  if (i < A.S) {
    uint32_t gid;
    if (A.sample_in) {   // clamped into the ring: a bad index reads valid rows
      gid = min((uint32_t)A.sample_in[i], cap * (uint32_t)A.B - 1u);
    } else {             // GraphReplayBuffer.sample: random.sample -> keyed permutation
      gid = sample_index((uint32_t)i, sample_key(n_graphs, sample_salt_k0(A.k0, A.env_offset), A.k1, A.ctrl->tick));
    }
    if (A.sample_out && (threadIdx.x & 63) == 0) A.sample_out[i] = (int32_t)gid;
    g3t_wave<NS>(L.P, L.PT, L.W[wi], L.PART[wi], gid, A);
  } else {
    for (int q = threadIdx.x & 63; q < kG3Cols; q += 64) L.PART[wi][q] = 0.0f;
  }
  __syncthreads();   // every wave's partial row
  for (int col = threadIdx.x; col < kG3Cols; col += NT) {
    float v = 0.0f;
    if (col <= kG3LossCol) {
      v = L.PART[0][col];
#pragma unroll
      for (int w = 1; w < WPB; ++w) v = v + L.PART[w][col];
    }
    slab[col] = v;
  }
}

template <int NS>
__global__ __launch_bounds__(64 * g3b_waves(NS)) void gat3_td_kernel(G3tArgs A) {
  __shared__ G3tSmem<NS> L;
  g3t_block<NS>(L, blockIdx.x, A);
}

// ---------------------------------------------------------------- clip + Adam + target sync
struct G3AdamArgs {
  swarm_adam_cfg hp;
  int B, N, capacity;
  float* params;
  float* target;
  float* m;
  float* v;
  const float* grad;
  swarm_ctrl* ctrl;
};

constexpr int kG3AdamNT = 128;
constexpr int kG3NF4 = kG3Cols / 4;            // 104 float4s of a row
constexpr int kG3FullF4 = G3_N_PARAMS / 4;     // 102 of them hold four parameters; float4 102 holds one
static_assert(kG3NF4 == 104 && kG3FullF4 == 102 && 4 * kG3FullF4 + 1 == G3_N_PARAMS && kG3NF4 <= kG3AdamNT,
              "a thread's float4 t; parameter 408 alone in float4 102");
static_assert((kG3NF4 + 3) / 4 <= 32, "the norm's groups fit half a wave");

// the one block of the optimizer step: gat3_adam_kernel's, and block (0, m) of the population's
// (swarm_pop_gat3.hip) with member m's rows, ctrl, ring capacity and optimizer row in A; red: 32 floats of LDS
__device__ __forceinline__ void g3_adam_block(float* red, const G3AdamArgs& A) {
  const int tid = threadIdx.x;
  const int f4 = min(tid, kG3NF4 - 1);
  float4 g = reinterpret_cast<const float4*>(A.grad)[f4];
  float4 w = reinterpret_cast<const float4*>(A.params)[f4];
  float4 m = reinterpret_cast<const float4*>(A.m)[f4];
  float4 v = reinterpret_cast<const float4*>(A.v)[f4];
  const float loss_sum = A.grad[kG3LossCol];
  // floats that are no parameter (409..415: the loss sum, zeros) and threads past the row count 0
  if (4 * tid + 0 >= G3_N_PARAMS) g.x = 0.0f;
  if (4 * tid + 1 >= G3_N_PARAMS) g.y = 0.0f;
  if (4 * tid + 2 >= G3_N_PARAMS) g.z = 0.0f;
  if (4 * tid + 3 >= G3_N_PARAMS) g.w = 0.0f;
  swarm_ctrl* C = A.ctrl;
  const uint32_t cap = (uint32_t)A.capacity;
  const uint32_t filled = C->filled_slots;
  const uint32_t valid_slots = filled + 1 < cap ? filled + 1 : cap;
  const uint32_t tick = C->tick;
  const uint32_t step = C->adam_step + 1;
  const float step_size = C->adam_step_size, inv_bc2 = C->adam_inv_bc2;
  // a control block that skipped swarm_ctrl_init holds 0 there (adam_kernel's rule)
  const float one_m_b1 = C->one_m_beta1 != 0.0f ? C->one_m_beta1 : (float)(1.0 - adam_beta1(A.hp));
  const float one_m_b2 = C->one_m_beta2 != 0.0f ? C->one_m_beta2 : (float)(1.0 - adam_beta2(A.hp));
  const bool train = valid_slots * (uint32_t)A.B >= (uint32_t)A.hp.batch;
  const bool sync = ((tick + 1) % (uint32_t)A.hp.update_target_every) == 0u;   // after the TD step of tick `tick`
  __syncthreads();   // every thread has read ctrl before thread 0 rewrites it
  float gn = 0.0f;
  if (train) {
    // clip_grad_norm_: the squared norm in the header comment's order
    const float d = ((g.x * g.x + g.y * g.y) + g.z * g.z) + g.w * g.w;
    const float sq = quad_sum(d);
    if ((tid & 3) == 0) red[tid >> 2] = sq;
    __syncthreads();
    const int l = tid & 63;
    const float r = red[min(l, 31)];
    gn = __builtin_amdgcn_sqrtf(wave_sum(l < 32 ? r : 0.0f));
    const float coef = A.hp.max_norm * __builtin_amdgcn_rcpf(gn + 1e-6f);
    const float clamped = coef < 1.0f ? coef : 1.0f;
    adam_elem(g.x * clamped, w.x, m.x, v.x, one_m_b1, A.hp.beta2, one_m_b2, inv_bc2, A.hp.eps, step_size);
    adam_elem(g.y * clamped, w.y, m.y, v.y, one_m_b1, A.hp.beta2, one_m_b2, inv_bc2, A.hp.eps, step_size);
    adam_elem(g.z * clamped, w.z, m.z, v.z, one_m_b1, A.hp.beta2, one_m_b2, inv_bc2, A.hp.eps, step_size);
    adam_elem(g.w * clamped, w.w, m.w, v.w, one_m_b1, A.hp.beta2, one_m_b2, inv_bc2, A.hp.eps, step_size);
    if (tid < kG3FullF4) {
      reinterpret_cast<float4*>(A.params)[tid] = w;
      reinterpret_cast<float4*>(A.m)[tid] = m;
      reinterpret_cast<float4*>(A.v)[tid] = v;
      if (sync) reinterpret_cast<float4*>(A.target)[tid] = w;
    } else if (tid == kG3FullF4) {   // parameter 408; floats 409..415 stay as they are
      A.params[G3_N_PARAMS - 1] = w.x;
      A.m[G3_N_PARAMS - 1] = m.x;
      A.v[G3_N_PARAMS - 1] = v.x;
      if (sync) A.target[G3_N_PARAMS - 1] = w.x;
    }
  }
  if (tid == 0) {
    if (train) {
      C->adam_step = step;
      ctrl_set_double(C, CTRL_B1POW, ctrl_get_double(C, CTRL_B1POW) * adam_beta1(A.hp));
      ctrl_set_double(C, CTRL_B2POW, ctrl_get_double(C, CTRL_B2POW) * adam_beta2(A.hp));
      ctrl_store_next_scalars(C, A.hp);
      C->one_m_beta1 = (float)(1.0 - adam_beta1(A.hp));
      C->one_m_beta2 = (float)(1.0 - adam_beta2(A.hp));
    }
    C->grad_norm = gn;   // 0 when the update was skipped
    C->trained = 0u;     // applied now: nothing pending
    C->loss = train ? loss_sum / (float)((size_t)A.hp.batch * A.N) : 0.0f;
    C->tick = tick + 1;
    C->write_slot = (C->write_slot + 1) % cap;
    C->filled_slots = valid_slots;
  }
}

// The launches (swarm_gat3_td.hip).  The kernels are instantiated in a translation unit of their
// own, for swarm_gat3_bwd.hip's reason: no other kernel's code may depend on them.
__attribute__((visibility("hidden"))) int gat3_td_launch(const G3tArgs& A, hipStream_t stream);
__attribute__((visibility("hidden"))) int gat3_adam_launch(const G3AdamArgs& A, hipStream_t stream);

// the checks swarm_gat3_td_grad / swarm_gat3_adam_step and the population's pair (swarm_pop_gat3.hip)
// share, in swarm_hip.h's order
inline int check_gat3_td(const swarm_config* c, const swarm_adam_cfg* hp) {
  if (int e = check_config(c, kCfgGat3Td, hp)) return e;
  if (c->net != SWARM_NET_GAT3) return SWARM_E_UNSUPPORTED;   // the one-layer network: swarm_td_grad / swarm_adam_step
  if (hp->world_size != 1) return SWARM_E_UNSUPPORTED;
  if (c->graph == SWARM_GRAPH_DENSE) return SWARM_E_BADARG;
  return 0;
}

}  // namespace swarm
