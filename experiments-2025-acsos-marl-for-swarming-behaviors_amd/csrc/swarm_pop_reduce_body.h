// swarm_pop_reduce_body.h — the statements of one block of a population reduce: block (x, m) is
// block x of member m's reduce (the statements of swarm_reduce_body.h).  Included INSIDE the
// braces of pop_reduce_kernel (swarm_pop.hip) and pop_reduce_hp_kernel (swarm_pop_hp.hip), as
// swarm_pop_tick_body.h is and for the same reason.  The including kernel provides:
//   HP (compile-time bool), const swarm_adam_cfg* member_hp (read only with HP),
//   const swarm_pop_member* members, int n_slabs, int env_offset, and ReduceArgs A0: the
//   arguments of grad_reduce_kernel<0> in advance mode with every per-member field left empty.
  [[maybe_unused]] swarm_adam_cfg row;
  if constexpr (HP) row = load_member_hp(member_hp, blockIdx.y);
  const swarm_pop_member M = load_member(members, blockIdx.y);
  if constexpr (HP) pin_member_hp(row);
  constexpr int PEER = 0;
  const int advance = 1;
  ReduceArgs A = A0;
  if constexpr (HP) take_member_hp(A.hp, row);
  A.slabs = M.slabs; A.grad = M.lr.grad; A.lr = M.lr; A.ctrl = M.ctrl; A.capacity = M.replay.capacity;
  A.k0 = sample_salt_k0(member_k0(M), env_offset); A.k1 = member_k1(M);
  const float* const slabs = A.slabs;
  swarm_ctrl* const ctrl = A.ctrl;
#include "swarm_reduce_body.h"
