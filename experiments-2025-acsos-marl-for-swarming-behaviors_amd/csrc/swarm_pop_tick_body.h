// swarm_pop_tick_body.h — the statements of one block of a population tick.  NOT a header of
// declarations: it is included INSIDE a kernel's braces (as swarm_reduce_body.h is), by
// pop_tick_kernel (swarm_pop.hip) and pop_tick_hp_kernel (swarm_pop_hp.hip), so both run the
// same text, while pop_tick_kernel's code objects stay what they were when the statements stood
// in it (as an inlined function they compiled differently, like the slab reduce's).
// The including kernel is a template over NSA, NST, GS, SCEN, SPEC and provides, under these names:
//   HP (compile-time bool: one optimizer row per member), const swarm_adam_cfg* member_hp (read
//   only with HP), const swarm_pop_member* members, int B, int N, and A, T, X: the arguments of
//   tick_kernel (swarm_tick.hip) with every per-member field left empty.
  static_assert(64 * kActWPB == 256 && 128 * (kTdRows / NST) == 256, "one block shape for both halves");
  __shared__ PopSmem<NSA, NST> U;
  // the row's loads first: they need nothing of the descriptor and are in flight beside its loads
  [[maybe_unused]] swarm_adam_cfg row;
  if constexpr (HP) row = load_member_hp(member_hp, blockIdx.y);
  const swarm_pop_member M = load_member(members, blockIdx.y);
  if constexpr (HP) pin_member_hp(row);
  const swarm_ctrl* const ctrl = M.ctrl;
  const swarm_learner lr = M.lr;
  const swarm_replay replay = M.replay;
  char* const ws = static_cast<char*>(M.workspace);
  // the member's fused-tick workspace: the error word's region, then the hand-off records (swarm_launch.h)
  unsigned long long* const rec = reinterpret_cast<unsigned long long*>(ws + kTickErrBytes);
  const int n_act = (B + kActWPB - 1) / kActWPB;
  if ((int)blockIdx.x < n_act) {
    ActArgs a = A;
    if constexpr (HP) take_member_hp(a.hp, row);
    a.k0 = member_k0(M); a.k1 = member_k1(M);
    a.state = M.state; a.ctrl = ctrl; a.lr = lr; a.replay = replay; a.out = M.out;
    a.grad_norm_out = const_cast<float*>(&ctrl->grad_norm);
    a.ho_rec = rec;
    act_body<NSA, MODE_TICK, SCEN, SPEC, true, SWARM_NET_GCN>(U.a, blockIdx.x, n_act, ctrl, M.state, lr.grad, lr.w_cur,
                                                              lr.m_cur, lr.v_cur, B, N, a);
  } else {
    TdArgs t = T;
    if constexpr (HP) t.gamma = row.gamma;
    t.k0 = member_k0(M); t.k1 = member_k1(M);
    t.params = lr.w_nxt; t.target = lr.target; t.replay = replay; t.ctrl = ctrl;
    t.sample_out = M.sample_out; t.slabs = M.slabs;
    TdFused x = X;
    if constexpr (HP) take_member_hp(x.hp, row);
    x.lr = lr; x.ho_rec = rec; x.ho_err = reinterpret_cast<uint32_t*>(ws);
    td_body<NST, GS, SPEC, true>(U.t, (int)blockIdx.x - n_act, nullptr, replay.s, replay.s_next, replay.r, replay.a,
                                 t.S, B, N, replay.capacity, t, x, ctrl, lr.grad, lr.w_cur, lr.m_cur, lr.v_cur);
  }
