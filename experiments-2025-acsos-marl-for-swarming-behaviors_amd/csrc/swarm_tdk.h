// swarm_tdk.h — body of the TD kernel: replay sample, TD loss, hand-written backward
// through GCN (PyG GATConv + MLP), per-block gradient slabs.  Shared by td_kernel
// (swarm_td.hip) and the fused training-tick kernel (swarm_tick.hip).
//
// Reference: DQNTrainer.train_step_dqn (src/training/train_gcn_dqn.py:112-137),
// GraphReplayBuffer.sample (:38-45), Adam(lr=1e-3) (:85), target sync (:131-133).
//
// Layout (swarm_wpg.h): one wave per sampled graph; a block holds 32 node slots (swarm_bwd.h TdLds).
// Backward per graph (online wave, per-node vectors in registers):
//   dQ[a] = (Q[a]-y) * 2/M                      (MSELoss mean, gather)
//   dR = W2[a]^T dQ ; dZ = dR * [Z>0]           (here: the one-hot dQ of the TD loss)
//   dO, the attention's dp / da_dst, dh: swarm_bwd.h, shared with swarm_q_backward (swarm_qbk.h)
// Parameter sums over the block's 32 node rows: dW1 = dZ^T T, dW2 = dQ^T R (here), dW = dh^T X and
// the vectors' ordered column sums (swarm_bwd.h); each block writes one slab [N_PARAMS + 1]
// (last = sum of squared TD errors) and swarm_grad_reduce sums the slabs in a fixed order
// (bitwise run-to-run reproducible).
#pragma once
#include "swarm_adam.h"
#include "swarm_bwd.h"
#include "swarm_diag.h"

namespace swarm {

struct TdArgs {
  int S, B, N, graph, k, conv, env_offset;
  uint32_t k0, k1;
  float radius;
  const float* params;
  const float* target;
  swarm_replay replay;
  const swarm_ctrl* ctrl;
  const int32_t* sample_in;
  int32_t* sample_out;
  float* slabs;
  float gamma;
  float grad_scale;   // fp32(2 / M_local)
  int n_slabs;        // TD blocks of the launch (slab layout, swarm_common.h slab_index)
};

// gradient-slab store (read once by the next launch, from another XCD).  The 4-B stores stay plain:
// as nt (td 8.4 vs 8.0 us) and as 4-B write-through sc1 (9.5 us; round 6 again: +0.1-0.2 us per
// tick) they cost more; the dW1 / dW2 tiles' 16-B pieces are write-through (sst4)
__device__ inline void slab_st(float* p, float v) { *p = v; }

// NS node slots per wave holding NS / GS graphs of GS slots (GS = 8 < NS = 16 packs two
// N <= 8 graphs into one wave: every MFMA column is a real node, one wave per SIMD).
// The dependent chain's pointers (batch indices -> replay rows) and the geometry lead the
// parameter list: preloaded into SGPRs (kernarg preload), the index loads issue at wave start.
template <int NS>
struct TdSmem {
  TdLds<NS> TB;
  __attribute__((aligned(16))) float Pon[N_LDS_PARAMS];
  __attribute__((aligned(16))) float Ptg[N_LDS_PARAMS];
  float red[64];   // fused tick: the optimizer step's norm (adam_norm2_block)
};

// the TD half of the fused training tick (swarm_tick.hip): weights from the pending
// optimizer step (recomputed in registers, as every acting block does), batch indices
// drawn in-kernel, this tick's slot read from the acting waves' hand-off records
struct TdFused {
  swarm_learner lr;
  swarm_adam_cfg hp;
  const unsigned long long* ho_rec;   // [B][ho_stride_granules(N)] tagged hand-off records
  uint32_t* ho_err;                   // bounded-wait overruns (0 in a correct run)
};
#ifndef SWARM_HO_SPIN_LIMIT
#define SWARM_HO_SPIN_LIMIT (1 << 18)
#endif
#ifndef SWARM_HO_FORCE_DROP
#define SWARM_HO_FORCE_DROP 0
#endif
#ifndef SWARM_HO_SLEEP
#define SWARM_HO_SLEEP 1  // s_sleep argument (x 64 cycles) between two hand-off sweeps
#endif
constexpr int kHoSpinLimit = SWARM_HO_SPIN_LIMIT;   // polls (with s_sleep) before a hand-off wait gives up
// test builds only (libswarm_hip_hodrop.so): every hand-off wait overruns at once
constexpr bool kHoForceDrop = SWARM_HO_FORCE_DROP == 1;
// test builds only (libswarm_hip_hodrop2.so): the target waves' s' waits overrun at once and the
// online waves never see r (their waits run to the bound): an overrun counts once per wave that
// dropped, not again in the online wave's r wait for a graph its target wave already dropped
constexpr bool kHoDropTarget = SWARM_HO_FORCE_DROP == 2;

// A hand-off wait that overruns drops the graphs it waited for: their nodes become padding
// (no TD error, no gradient, no loss), so the update is the mean over the S*N batch nodes with
// those graphs' terms zero, never one computed from a stale granule.  The overrun is counted in
// the workspace's error word (SwarmEngine.handoff_errors; DQNTrainer raises on it).  Node slot
// 16 ct + c belongs to graph (16 ct + c) / GS: with GS < 16 the lanes of its column group
// (c / GS, all four row groups) in one ct; GS = 16 one whole ct; GS = 32 both.
template <int NS, int GS>
__device__ inline void drop_overrun(const bool (&okc)[DGeom<NS>::CT], bool (&drop)[DGeom<NS>::CT],
                                    bool (&nv)[DGeom<NS>::CT], int c) {
  constexpr int CT = DGeom<NS>::CT;
  bool bad[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(!okc[ct]);
    if constexpr (GS < 16) {
      const unsigned long long cols = (((1ull << GS) - 1ull) << (GS * (c / GS))) * 0x0001000100010001ull;
      bad[ct] = (m & cols) != 0ull;
    } else {
      bad[ct] = m != 0ull;
    }
  }
  if constexpr (GS > 16) {   // one graph over every ct of the wave
    bool any = false;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) any = any || bad[ct];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) bad[ct] = any;
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
    if (bad[ct]) { drop[ct] = true; nv[ct] = false; }
}

// FRAG: both forwards' weight-image operands read in one batch right behind B0 (swarm_dl.h DFrag),
// so a wave that waits for a hand-off holds them long before its state lands
template <int NS, int GS, int SPEC, bool FUSED = false, bool FRAG = false>   // SPEC: graph + conv fixed at compile time (swarm_common.h)
__device__ __forceinline__ void td_body(TdSmem<NS>& L, const int vb, const int32_t* sample_in, const float* rs,
                                        const float* rs_next, const float* rr, const uint8_t* ra, int S, int B,
                                        int N, int capacity, const TdArgs& A, const TdFused& X,
                                        const swarm_ctrl* __restrict__ ctrl_pre = nullptr, const float* g_pre = nullptr,
                                        const float* w_pre = nullptr, const float* m_pre = nullptr,
                                        const float* v_pre = nullptr) {
  constexpr int GPB = kTdRows / NS, CT = DGeom<NS>::CT;   // GPB: online (= target) waves per block
  constexpr int GPW = NS / GS;                             // graphs per wave
  constexpr int NT = 128 * GPB;
  static_assert(!FUSED || NT == kAdamNT, "the fused TD block is one Adam workgroup");
  static_assert(GPB <= 2, "B2 jobs 2 and 3 go to the pre-path online waves by wave index (GPB <= 2)");
  static_assert(NS % 16 == 0, "every MFMA column of a wave is one of its node slots");
  TdLds<NS>& TB = L.TB;
  float* Pon = L.Pon;
  float* Ptg = L.Ptg;
  const int wave = threadIdx.x >> 6;
  const bool online = wave < GPB;
  const int wi = online ? wave : wave - GPB;
  const DGeom<NS> d = make_dgeom<NS>(vb * GPB + wi, 1 << 30);   // lane geometry; liveness is per graph
  const int graph = spec_graph<SPEC>(A.graph);
  const int conv = spec_conv<SPEC>(A.conv);
  const int row0 = wi * NS;
  const WView<NS> V = online ? WView<NS>{TB.H + row0, TB.T + row0, TB.R + row0, &TB.on[wi]} : TB.target_view(wi);
  const int lane = d.lane, c = d.c, p = d.p;
  // this block's slab column q (swarm_common.h slab_index: column-block major), addressed as a
  // wave-uniform base (the block's 16-column run in column block 0) plus a 32-bit element
  // offset: one 64-bit add per block instead of 64-bit index arithmetic per store
  static_assert(kSlabCols == 16, "slab column blocks of 16");
  float* const slab_base = A.slabs + (size_t)vb * kSlabCols;
  const uint32_t slab_stride = (uint32_t)A.n_slabs * kSlabCols;
  TD_DIAG_SLAB_STATE   // swarm_diag.h: nothing, and every block stores, in the product build
  auto sst = [&](int q, float v) {
    if (TD_DIAG_STORES_SLAB(vb)) slab_st(slab_base + ((uint32_t)(q >> 4) * slab_stride + (uint32_t)(q & 15)), v);
  };
// the dW1 / dW2 tiles' 16-B pieces: four consecutive parameters q .. q + 3 (q % 4 == 0) of one
// 16-column slab run, stored write-through (swarm_common.h st16_wt): the 1,312 of a slab's 1,674
// floats leave the XCD's L2 as they are written instead of at the launch end (round 6: C2 -0.22,
// C3 -0.43 us per tick, profiles/r06_ab_b2t_v3_*.jsonl; plain 16-B stores were neutral)
  static_assert(OFF_W1 % 16 == 0 && OFF_W2 % 16 == 0 && kHidden % 16 == 0, "16-B slab pieces");
  auto sst4 = [&](int q, f32x4 v) {
    if (!TD_DIAG_STORES_SLAB(vb)) return;
    st16_wt(slab_base + ((uint32_t)(q >> 4) * slab_stride + (uint32_t)(q & 15)), v[0], v[1], v[2], v[3]);
  };
  SWARM_RTSTAMP(8);
  SWARM_STAMP(0);

  // ---- 3-launch tick: this wave's replay indices come from the previous launch, so the
  //      dependent pair (index -> replay rows) is issued first and the weight staging and
  //      ctrl reads overlap it.  Indices are clamped into the ring: a skipped tick reads
  //      valid (unused) rows.  Fused tick: the pending Adam step's operands and ctrl first.
  AdamRegs R;
  WImageSlots wslots;
  swarm_ctrl cc = {};
  if (FUSED) {   // the fused kernel's preloaded argument SGPRs (== X.lr / A.ctrl): no kernarg round trip first
    cc = *ctrl_pre;   // issued before any kernarg-segment load, so no wait on one delays it
    __builtin_amdgcn_sched_barrier(0);
    R.load(g_pre, w_pre, m_pre, v_pre, threadIdx.x, true);
    __builtin_amdgcn_sched_barrier(0);   // every Adam operand load issued before the first scalar wait
    wslots.form(threadIdx.x);             // the thread's LDS image slots (both images), in the loads' flight time
  }
  // fused: the scalars the sampling, the hand-off test and the optimizer step read (ctrl's
  // write_slot, the batch size S, the Adam hyper-parameters) made opaque here, so they are
  // loaded with the first scalar wait instead of being re-fetched at a later first use behind a
  // second one (a kernarg / ctrl round trip on the TD chain)
  swarm_adam_cfg hp = X.hp;
  int32_t* sample_out = A.sample_out;
  const unsigned long long* ho_rec = X.ho_rec;
  if (FUSED) {
    asm volatile("" : "+s"(cc.write_slot), "+s"(cc.trained), "+s"(S), "+s"(hp.beta1), "+s"(hp.beta2), "+s"(hp.eps),
                 "+s"(hp.max_norm), "+s"(hp.update_target_every), "+s"(hp.world_size), "+s"(sample_out), "+s"(ho_rec));
  }
  // fused: the pending step's two conditions (a held rank applies no step; a target-sync tick:
  // a runtime division) from the same scalars, formed and pinned at that wait as well
  uint32_t pending = 0u, sync_target = 0u;
  if (FUSED) {
    pending = (cc.trained != 0u && cc.peer_hold == 0u) ? 1u : 0u;
    sync_target = (pending && (cc.tick % (uint32_t)hp.update_target_every) == 0u) ? 1u : 0u;
    asm volatile("" : "+v"(sync_target));   // (the division's result lives in a VGPR)
  }
  const uint32_t cap = (uint32_t)capacity;
  const uint32_t ring_graphs = cap * (uint32_t)B;
  int sid[CT];     // batch index of this lane's graph
  bool live[CT], nv[CT];
  int jl[CT];      // local node index inside the graph
  uint32_t gid[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = 16 * ct + c;
    const int gi = (GS < NS) ? n / GS : 0;
    jl[ct] = (GS < NS) ? n % GS : n;
    sid[ct] = vb * (kTdRows / GS) + wi * GPW + gi;
    live[ct] = sid[ct] < S;
    nv[ct] = live[ct] && jl[ct] < N;
    gid[ct] = 0;
    if (!FUSED && sample_in) gid[ct] = min((uint32_t)sample_in[min(sid[ct], S - 1)], ring_graphs - 1u);
  }
  ParamStage<NT> pon, ptg;
  if (!FUSED) pon.load(A.params, threadIdx.x);
  ptg.load(A.target, threadIdx.x);   // fused: overridden by the new weights on a sync tick
  const uint32_t filled = FUSED ? cc.filled_slots : A.ctrl->filled_slots;
  const uint32_t valid_slots = filled + 1 < cap ? filled + 1 : cap;
  const uint32_t n_graphs = valid_slots * (uint32_t)B;
  if (FUSED || !sample_in) {   // GraphReplayBuffer.sample: random.sample -> keyed permutation
    const uint32_t k0 = sample_salt_k0(A.k0, A.env_offset);
    const SampleKey sk = FUSED ? sample_key_cached(&cc, n_graphs, k0, A.k1, cc.tick)
                               : sample_key(n_graphs, k0, A.k1, A.ctrl->tick);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
      gid[ct] = n_graphs >= (uint32_t)S ? sample_index((uint32_t)min(sid[ct], S - 1), sk) : 0u;
  }
  // graphs of this tick's slot (fused: they come from the acting waves' hand-off records).  A
  // wave holding one takes the pre path in every kind of launch (fused, 3-launch, unfused), so
  // the three stay bit-identical to each other
  const uint32_t wslot = FUSED ? cc.write_slot : A.ctrl->write_slot;
  bool ho[CT];
  bool wait = false, inslot = false;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const bool cur = live[ct] && n_graphs >= (uint32_t)S && gid[ct] / (uint32_t)B == wslot;
    ho[ct] = FUSED && cur;
    wait = wait || ho[ct];
    inslot = inslot || cur;
  }
  // replay rows written by earlier ticks: loads issued now (fused: every lane but the hand-off ones)
  float rew[CT];
  int act[CT];
  float4 st[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const uint32_t slot = gid[ct] / (uint32_t)B, genv = gid[ct] % (uint32_t)B;
    const size_t ri = ((size_t)slot * B + genv) * N + min(jl[ct], N - 1);
    st[ct] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rew[ct] = 0.0f;
    act[ct] = 0;
    if (!ho[ct]) {
      st[ct] = reinterpret_cast<const float4*>(online ? rs : rs_next)[ri];
      rew[ct] = rr[ri];
      act[ct] = nv[ct] ? (int)ra[ri] : 0;
    }
  }
  // ---- skip while the replay holds fewer than `batch` graphs (train_gcn_dqn.py:113-115)
  if (n_graphs < (uint32_t)S) {
    for (int q = threadIdx.x; q <= N_PARAMS; q += NT) sst(q, 0.0f);
    return;
  }
  if (sample_out && online && p == 0) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
      if (live[ct] && jl[ct] == 0) sample_out[sid[ct]] = (int32_t)gid[ct];
  }
  SWARM_STAMP(1);
  const bool waited = FUSED && __builtin_amdgcn_ballot_w64(wait) != 0;
  // pre path: the online waves of a block holding one of this tick's transitions form their
  // backward for gq = 1 before y (dZ, dT, dO, the attention scores' g and dp are linear in their
  // target node's gq; the sums that mix targets, da_src and dh, stay after B2), in the time the
  // block waits for the acting wave's s' and the target forward.  Every online wave of such a
  // block takes it (round 4): the one without a hand-off graph otherwise ran its whole backward
  // after B1 and was the last to reach B3.  The rule depends only on the block's graphs, so the
  // fused, 3-launch and unfused launches still agree bit for bit
  if (online && lane == 0) TB.insl[wi] = __builtin_amdgcn_ballot_w64(inslot) != 0 ? 1 : 0;
  bool live_drop[CT];   // this wave's graph was dropped after a hand-off overrun
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) live_drop[ct] = false;
  if constexpr (FUSED) {   // the pending optimizer step (train_gcn_dqn.py:125-133), as every acting block does;
                 // done before any hand-off wait so that none of it follows the wait
    if (pending)
      adam_apply(R, hp, cc.adam_step_size, cc.adam_inv_bc2, cc.one_m_beta1, cc.one_m_beta2, threadIdx.x, L.red,
                 (hp.flags & SWARM_ADAM_F_NORM_PARTIALS) != 0);
    store_w_lds(Pon, R, threadIdx.x, wslots);
    if (__builtin_amdgcn_readfirstlane(sync_target)) store_w_lds(Ptg, R, threadIdx.x, wslots);
    else ptg.store(Ptg, threadIdx.x, wslots.b);
  } else {
    pon.store(Pon, threadIdx.x);
    ptg.store(Ptg, threadIdx.x);
  }
  if (online && p == 0 && !waited) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) TB.act[row0 + 16 * ct + c] = act[ct];
  }
  if (FUSED && !online && p == 0) {   // no graph dropped yet (set by an s' overrun, read by the r wait)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) TB.tdrop[row0 + 16 * ct + c] = 0;
  }
  __syncthreads();   // B0: weight images
  DFrag<NS> wfrag;
  if constexpr (FRAG) wfrag.load(online ? Pon : Ptg, c, p);
  SWARM_STAMP(2);
  bool pre = false;
#pragma unroll
  for (int w2 = 0; w2 < GPB; ++w2) pre = pre || TB.insl[w2] != 0;
  TD_DIAG_PRE(pre)
  pre = pre && online;
  const uint32_t tag = cc.tick + 1u;
  // granule address of this lane's node in a hand-off record: s at 0, s' at 4N, r at 8N, a at 9N
  auto ho_at = [&](int ct, int off, int per_node) -> const unsigned long long* {
    return ho_rec + (size_t)(gid[ct] % (uint32_t)B) * ho_stride_granules(N) + off + per_node * min(jl[ct], N - 1);
  };
  if (waited) {   // sweep this lane's granules until every tag is this tick's (R2 hand-off): online
                  // waves s (published at the acting prologue), target waves s' (after the integrator).
                  // Wave-local, after B0: the block's other waves are not held by it
    for (int spin = 0;; ++spin) {
      unsigned long long g[CT][4];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (ho[ct]) {
          const unsigned long long* sp = ho_at(ct, online ? 0 : 4 * N, 4);
#pragma unroll
          for (int k = 0; k < 4; ++k) g[ct][k] = ld_granule(sp + k);
        }
      bool ok = true, okc[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        okc[ct] = true;
        if (ho[ct]) {
          okc[ct] = !kHoForceDrop && !(kHoDropTarget && !online) && (uint32_t)(g[ct][0] >> 32) == tag &&
                    (uint32_t)(g[ct][1] >> 32) == tag && (uint32_t)(g[ct][2] >> 32) == tag &&
                    (uint32_t)(g[ct][3] >> 32) == tag;
          ok = ok && okc[ct];
          st[ct] = make_float4(__uint_as_float((uint32_t)g[ct][0]), __uint_as_float((uint32_t)g[ct][1]),
                               __uint_as_float((uint32_t)g[ct][2]), __uint_as_float((uint32_t)g[ct][3]));
        }
      }
      if (!__builtin_amdgcn_ballot_w64(!ok)) break;
      if (kHoForceDrop || (kHoDropTarget && !online) || spin >= kHoSpinLimit) {   // never in a correct
        drop_overrun<NS, GS>(okc, live_drop, nv, c);                              // run: drop, count
        // tell the online waves' r wait first (they then drop without counting again), count after.
        // An online wave whose own r wait overruns BEFORE this store counts the graph as well: the
        // error word counts dropping waves, and is nonzero whenever a graph was dropped
        if (FUSED && !online && p == 0) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            if (live_drop[ct]) *(volatile int*)&TB.tdrop[row0 + 16 * ct + c] = 1;
        }
        if (lane == 0) atomicAdd(X.ho_err, 1u);
        break;
      }
      __builtin_amdgcn_s_sleep(SWARM_HO_SLEEP);
    }
    SWARM_RTSTAMP(10);
    __builtin_amdgcn_s_setprio(3);   // waves of hand-off graphs are the tick's critical path
  }
  DFwd<NS> F;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    node_x(st[ct].x, st[ct].y, st[ct].z, st[ct].w, jl[ct], p, F.x[ct]);
    if (!nv[ct]) { F.x[ct][0] = 0.0f; F.x[ct][1] = 0.0f; }
  }
  // ---- forwards: online on s (activations kept), target on s' (train_gcn_dqn.py:119-121).
  //      Everything after B1 waits for the target waves' y, so they issue first.
  if (!online && !waited) __builtin_amdgcn_s_setprio(2);
  if constexpr (FRAG)
    dl_forward<NS, 16, GS, spec_complete_graph(SPEC), true>(online ? Pon : Ptg, d, N, graph, A.k, A.radius, conv, nullptr, V, online,
                                                            F, DlNoHook(), &wfrag);
  else
    dl_forward<NS, 16, GS, spec_complete_graph(SPEC)>(online ? Pon : Ptg, d, N, graph, A.k, A.radius, conv, nullptr, V, online, F);
  // fused: the rest of this tick's transitions, each as late as its first use: a for the online
  // waves' pre path here; r (published after the acting wave's reward) by the online waves after
  // it, in their wait for the target waves' y, so no poll sits between the target forward and B1
  if (FUSED && waited && online) {
    for (int spin = 0;; ++spin) {
      bool ok = true, okc[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        okc[ct] = true;
        if (ho[ct] && !live_drop[ct]) {
          const unsigned long long g = ld_granule(ho_at(ct, 9 * N, 1));
          okc[ct] = !kHoForceDrop && (uint32_t)(g >> 32) == tag;
          ok = ok && okc[ct];
          act[ct] = nv[ct] ? (int)(uint32_t)g : 0;
        }
      }
      if (!__builtin_amdgcn_ballot_w64(!ok)) break;
      if (kHoForceDrop || spin >= kHoSpinLimit) {
        if (lane == 0) atomicAdd(X.ho_err, 1u);
        drop_overrun<NS, GS>(okc, live_drop, nv, c);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (p == 0) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) TB.act[row0 + 16 * ct + c] = nv[ct] ? act[ct] : 0;
    }
  }
  // ---- pre path, before y: dZ1 = W2[a] * [z > 0], dO1 = (W1^T dZ1) (1 - t^2) (MFMA, as after B2),
  //      g1 = H_u . dO1_v, dp1 / da_dst1 of the attention (scaled by gq after B1)
  float dO1[CT][2][4], dp1[CT][CT][4], dad1[CT];
  if (pre) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int ac = min(max(act[ct], 0), kActions - 1);
      float dz1[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 w = *reinterpret_cast<const float4*>(Pon + L_W2 + ac * kWRow + 16 * t + 4 * p);
        float wv[4] = {w.x, w.y, w.z, w.w};
        asm volatile("" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]), "+v"(wv[3]));
#pragma unroll
        for (int r = 0; r < 4; ++r) dz1[t][r] = F.zr[ct][t][r] > 0.0f ? wv[r] : 0.0f;
      }
      bwd_dO_tile(Pon, c, p, dz1, F.t[ct], true, dO1[ct]);
      dad1[ct] = 0.0f;
    }
    if (conv == SWARM_CONV_GAT) {   // unmasked: nv (as known after B1) is applied there, with gq
      bool all[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) all[ct] = true;
      bwd_attention<NS>(TB.H + row0, F, V.sm->ssrc, dO1, all, c, p, dp1, dad1);
    }
  }
  if (FUSED && waited && online) {   // r of this tick's transitions (y = r + gamma max Q_tgt after B1)
    for (int spin = 0;; ++spin) {
      bool ok = true, okc[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        okc[ct] = true;
        if (ho[ct] && !live_drop[ct]) {
          const unsigned long long g = ld_granule(ho_at(ct, 8 * N, 1));
          okc[ct] = !kHoForceDrop && !kHoDropTarget && (uint32_t)(g >> 32) == tag;
          ok = ok && okc[ct];
          rew[ct] = __uint_as_float((uint32_t)g);
        }
      }
      if (!__builtin_amdgcn_ballot_w64(!ok)) break;
      if (kHoForceDrop || spin >= kHoSpinLimit) {   // the graph's rows are dropped (online side)
        // graphs the target wave has dropped already (its s' wait overran; the LDS flag is stored
        // before its count) are dropped here too but not counted a second time
        bool rest = false;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (!okc[ct] && *(volatile int*)&TB.tdrop[row0 + 16 * ct + c] != 0) {
            okc[ct] = true;
            live_drop[ct] = true;
            nv[ct] = false;
          }
          rest = rest || !okc[ct];
        }
        if (__builtin_amdgcn_ballot_w64(rest)) {
          if (lane == 0) atomicAdd(X.ho_err, 1u);
          drop_overrun<NS, GS>(okc, live_drop, nv, c);
        }
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  if (!online && p == 0) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float qmax = F.q[ct][0];
#pragma unroll
      for (int a = 1; a < kActions; ++a) qmax = fmaxf(qmax, F.q[ct][a]);
      TB.yq[row0 + 16 * ct + c] = nv[ct] ? A.gamma * qmax : 0.0f;   // y = r + this (online waves)
      if (FUSED) TB.tdrop[row0 + 16 * ct + c] = live_drop[ct] ? 1 : 0;
    }
  }
  if (!online && !waited) __builtin_amdgcn_s_setprio(0);
  if (online && lane == 0) TB.prew[wi] = pre ? 1 : 0;
  SWARM_STAMP(3);
  __syncthreads();   // B1: TD targets
  SWARM_STAMP(4);

  const float* P = Pon;
  float dz[CT][2][4];
  if (online) {
    // ---- dQ at the taken action (MSELoss mean), dR = W2[a]^T dQ, dZ = dR * [z > 0]
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int row = row0 + 16 * ct + c;
      if (FUSED && TB.tdrop[row]) nv[ct] = false;   // the target wave dropped the graph
      float qa = F.q[ct][0];
#pragma unroll
      for (int a = 1; a < kActions; ++a) qa = (act[ct] == a) ? F.q[ct][a] : qa;
      const float delta = nv[ct] ? (qa - (rew[ct] + TB.yq[row])) : 0.0f;   // y = r + gamma max Q_tgt(s')
      const float gq = delta * A.grad_scale;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float4 w = *reinterpret_cast<const float4*>(P + L_W2 + act[ct] * kWRow + 16 * t + 4 * p);
        float wv[4] = {w.x, w.y, w.z, w.w};
        asm volatile("" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]), "+v"(wv[3]));   // one vector read, not 4 masked ones
#pragma unroll
        for (int r = 0; r < 4; ++r) dz[ct][t][r] = F.zr[ct][t][r] > 0.0f ? wv[r] * gq : 0.0f;
      }
      row_store(TB.dZ[row], p, dz[ct]);
      TB.X[row][p] = F.x[ct][0];
      TB.X[row][4 + p] = F.x[ct][1];
#pragma unroll
      for (int j = 0; j < NS / 4; ++j) TB.cm[row][4 * j + p] = F.cc[ct][j];
      if (p == 0) { TB.X[row][8] = 0.0f; TB.gq[row] = gq; TB.d2[row] = delta * delta; }
      if (pre) {   // the pre path's images scaled by this node's gq (rows free since B1)
        float o[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[t][r] = nv[ct] ? dO1[ct][t][r] * gq : 0.0f;
        row_store(TB.dO[row], p, o);
        if (conv == SWARM_CONV_GAT) {
#pragma unroll
          for (int ut = 0; ut < CT; ++ut)
#pragma unroll
            for (int r = 0; r < 4; ++r) TB.dp[row][16 * ut + 4 * p + r] = nv[ct] ? dp1[ct][ut][r] * gq : 0.0f;
        }
        dad1[ct] = nv[ct] ? dad1[ct] * gq : 0.0f;
      }
    }
  }
  __syncthreads();   // B2: dZ / T / R / gq / act / d2 / X / cm of every graph (pre path: dO / dp too)
  SWARM_STAMP(5);
  int np_pre = 0;   // online waves of this block on the pre path
#pragma unroll
  for (int w2 = 0; w2 < GPB; ++w2) np_pre += TB.prew[w2];
  // the parameter products that need only B2's images (each writes its slice of the slab).
  // dW1 = dZ^T T and dW2 = onehot(a) gq R as 16x16x4 MFMA tiles, K = 4 of the block's 32 node
  // rows per step: dW1 tiles (ti, tj) = jobs 2 ti + tj, dW2's 9 action rows in one 16-row tile
  // per column half tj = jobs 4 + tj.  A wave runs three tiles of one column half tj, their
  // chains interleaved with every operand read first (as conditional reads they became a branch
  // and an LDS round trip in front of each MFMA): 24 MFMAs of 32 cycles where the 32x32x2 form
  // had 16 of 64 per product, and dW2 takes 16 rows of work instead of 32.
  auto b2_tiles = [&](int tj) {   // lane (c, p) of the D layout: column c, k-slot / row group p
    float a1[2][8], b1[8], a2[8], b2v[8];
    int an[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int n = 4 * s + p;
      a1[0][s] = TB.dZ[n][c];
      a1[1][s] = TB.dZ[n][16 + c];
      b1[s] = TB.T[n][16 * tj + c];
      b2v[s] = TB.R[n][16 * tj + c];
      an[s] = TB.act[n];
      a2[s] = TB.gq[n];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(a2[s]));   // loaded unconditionally
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f};
    // the transposed tiles (operands swapped: the same products, the same K order): lane (c, p)
    // holds dW1[out = c (+16)][in = 16 tj + 4p .. 4p + 3] and dW2[action = c][in = ...], four
    // consecutive parameters of one 16-column slab run, stored as ONE 16-B store per tile
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      d0 = mfma16(b1[s], a1[0][s], d0);
      d1 = mfma16(b1[s], a1[1][s], d1);
      d2 = mfma16(b2v[s], an[s] == c ? a2[s] : 0.0f, d2);
    }
    sst4(OFF_W1 + c * kHidden + 16 * tj + 4 * p, d0);
    sst4(OFF_W1 + (16 + c) * kHidden + 16 * tj + 4 * p, d1);
    if (c < kActions) sst4(OFF_W2 + c * kHidden + 16 * tj + 4 * p, d2);
  };
  auto b2_job = [&](int job) {   // the vector sums: job 2 = db1, job 3 = db2 and the loss
    if (job == 2) {
      if (lane < kHidden) sst(OFF_B1 + lane, col_sum32(TB.dZ, lane));
    } else if (lane < kActions || lane == 63) {   // db2 / loss: the ordered sum over the 32 rows,
      // 8 rows' reads at a time (each read unconditional: as selects around the reads they became
      // a branch and an LDS round trip per row)
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < kTdRows; k += 8) {
        int a8[8];
        float g8[8], d8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { a8[j] = TB.act[k + j]; g8[j] = TB.gq[k + j]; d8[j] = TB.d2[k + j]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(g8[j]), "+v"(d8[j]));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = lane == 63 ? d8[j] : (a8[j] == lane ? g8[j] : 0.0f);
          acc = (k == 0 && j == 0) ? v : acc + v;
        }
      }
      sst(lane == 63 ? N_PARAMS : OFF_B2 + lane, acc);
    }
  };

  const int col = lane & 31, h = lane >> 5;
  if (online) {
    // ---- the per-node backward (swarm_bwd.h).  A pre-path wave has its dO / dp rows and da_dst
    //      since B1 and joins at dh, the step that mixes targets
    float da_d[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) da_d[ct] = pre ? dad1[ct] : 0.0f;
    if (!pre) {
      float dO[CT][2][4];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        bwd_dO_tile(P, c, p, dz[ct], F.t[ct], nv[ct], dO[ct]);
        row_store(TB.dO[row0 + 16 * ct + c], p, dO[ct]);
      }
      SWARM_STAMP(24);
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
      wave_lds_sync();   // dp / dO rows of this graph
    }
    SWARM_STAMP(25);
    bwd_dh<NS, GS>(TB, P, row0, N, conv, nv, da_d, c, p);
    SWARM_STAMP(27);
  } else {
    // ---- target waves: the dW1 / dW2 tiles of column half tj = wi (GPB = 2) or both (GPB = 1);
    //      the vector sums (db1, db2 + loss) too unless the block has pre-path online waves:
    //      theirs is the short side of B2 -> B3 there, and the target waves' products the long one
    for (int tj = wi; tj < 2; tj += GPB) b2_tiles(tj);
    if (np_pre == 0)
      for (int job = 2 + wi; job < 4; job += GPB) b2_job(job);
  }
  if (online && pre) {   // (GPB = 2: one pre wave takes both sums, two split them)
    if (np_pre == 1 || wi == 0) b2_job(2);
    if (np_pre == 1 || wi == 1) b2_job(3);
  }
  SWARM_STAMP(26);   // stamps build: the B2 jobs done, before the B3 wait
  __syncthreads();   // B3: dO / dH / das / dad
  SWARM_STAMP(6);
  // ---- products over B3's images, spread over all 2 GPB waves of the block:
  //      job 0 / 1: dW rows 0-15 / 16-31 = sum_n dH[n][f] X[n][k] (MFMA 16x16x4, K = node rows)
  //      job 2: att_src / att_dst (lane halves) ; job 3: dbias
  {
    const int wall = online ? wi : GPB + wi;
    for (int job = wall; job < 4; job += 2 * GPB) {
      if (job < 2) {
        const f32x4 acc = bwd_dw_tile(TB, job, c, p);
        if (c < kFeat) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sst(OFF_W + (16 * job + 4 * p + r) * kFeat + c, acc[r]);
        }
      } else if (job == 2) {   // att_src (half 0) / att_dst (half 1)
        sst((h == 0 ? OFF_ATT_SRC : OFF_ATT_DST) + col, bwd_att_col(TB, h == 0 ? TB.das : TB.dad, col));
      } else if (lane < kHidden) {
        sst(OFF_BIAS + lane, col_sum32(TB.dO, lane));
      }
    }
  }
  SWARM_STAMP(7);
  SWARM_RTSTAMP(9);
}

}  // namespace swarm
