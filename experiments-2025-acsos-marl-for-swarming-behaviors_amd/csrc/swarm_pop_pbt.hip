// swarm_pop_pbt.hip — population-based training on the device (swarm_pop_exploit): the worst
// members of a population take over the learner of the best and perturb its hyper-parameters
// (Jaderberg et al. 2017, "Population Based Training of Neural Networks", exploit = truncation
// selection, explore = perturb).  gfx950 only.
//
// Reference: src/training/train_gcn_dqn.py:262-290 trains one learner per seed under fixed
// hyper-parameters (:85,112-137) and never moves a learner; this is new ground on top of the
// population's device tables (swarm_pop_member, the swarm_adam_cfg rows of the _hp entry points).
//
// Two launches on the caller's stream, nothing allocated, nothing read back:
//   pbt_plan_kernel  one block, thread m = member m.  Scores into LDS (NaN as -inf), rank by
//                    counting (swarm_pbt.h pbt_rank, O(P) per thread, P <= 1024), by_rank[rank] =
//                    member.  A child (rank >= P - n_replace) draws one Philox block, picks its
//                    parent among ranks < n_replace, and writes parent[m] and its own row of
//                    member_hp (the parent's, explored).  Everyone else writes parent[m] = m.
//   pbt_copy_kernel  grid (8, P): block (x, m) returns at once when parent[m] == m; otherwise it
//                    copies buffer x (the seven learner rows, lr.grad) of the parent's descriptor
//                    to the child's, and block x = 0 also the optimizer's control words.
//
// No block ever writes what another reads.  Ranks are a permutation, parents are ranks
// 0..n_replace-1 and children ranks P-n_replace..P-1; n_replace <= P/2 gives n_replace <=
// P - n_replace, so the two sets are disjoint.  Only children's buffers, control words and rows
// are written, each by exactly one block (x, child) or one plan thread; only parents' are read;
// a child is never a parent.  The plan's reads of member_hp (parents' rows) and its writes
// (children's rows) are disjoint for the same reason, and parent[] is written by the plan launch
// and read by the copy launch, which the stream orders.  Members must not share buffers (the
// population's own contract).
//
// The descriptors are read as the population tick reads them (load_member: uniform loads from
// &members[blockIdx.y] and &members[parent], pointers cast to the global address space).  The ABI
// promises float alignment only for the learner pointers: a block copies float4s when both its
// pointers are 16-byte aligned (a uniform test) and dwords otherwise.
#include "swarm_pbt.h"
#include "swarm_popk.h"

namespace swarm {

__global__ __launch_bounds__(SWARM_PBT_MAX_MEMBERS) void pbt_plan_kernel(swarm_pbt_cfg C, const float* __restrict__ score,
                                                                         swarm_adam_cfg* member_hp, int P,
                                                                         int32_t* __restrict__ parent) {
  __shared__ float s[SWARM_PBT_MAX_MEMBERS];
  __shared__ int by_rank[SWARM_PBT_MAX_MEMBERS];
  const int m = threadIdx.x;
  if (m < P) s[m] = pbt_score(score[m]);
  __syncthreads();
  int rank = 0;
  if (m < P) {
    rank = pbt_rank(s, P, m);
    by_rank[rank] = m;
  }
  __syncthreads();
  if (m >= P) return;
  if (rank < P - C.n_replace) {   // a parent or a middle member: untouched (n_replace = 0: everyone)
    parent[m] = m;
    return;
  }
  const u32x4 w = philox4x32(C.round, (uint32_t)m, STREAM_PBT, 0u, (uint32_t)(C.seed & 0xFFFFFFFFu),
                             (uint32_t)(C.seed >> 32));
  const int p = by_rank[uniform_int(w.x, (uint32_t)C.n_replace)];
  parent[m] = p;
  member_hp[m] = pbt_explore(member_hp[p], C, w);
}

// n floats from src to dst by the whole block: float4s when both are 16-byte aligned
__device__ inline void pbt_copy(float* dst, const float* src, int n) {
  const int t = threadIdx.x;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0) {
    const int n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = t; i < n4; i += kPbtCopyThreads) d4[i] = s4[i];
    const int i = (n4 << 2) + t;
    if (i < n) dst[i] = src[i];
  } else {
    for (int i = t; i < n; i += kPbtCopyThreads) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(kPbtCopyThreads) void pbt_copy_kernel(const swarm_pop_member* __restrict__ members, int P,
                                                                   const int32_t* __restrict__ parent) {
  const unsigned int c = blockIdx.y;
  const int p = parent[c];
  if (p == (int)c || (unsigned int)p >= (unsigned int)P) return;   // not a child (or no member: nothing is touched)
  const swarm_pop_member D = load_member(members, c), S = load_member(members, (unsigned int)p);
  float* dst;
  const float* src;
  switch (blockIdx.x) {
    case 0: dst = D.lr.w_cur; src = S.lr.w_cur; break;
    case 1: dst = D.lr.w_nxt; src = S.lr.w_nxt; break;
    case 2: dst = D.lr.m_cur; src = S.lr.m_cur; break;
    case 3: dst = D.lr.m_nxt; src = S.lr.m_nxt; break;
    case 4: dst = D.lr.v_cur; src = S.lr.v_cur; break;
    case 5: dst = D.lr.v_nxt; src = S.lr.v_nxt; break;
    case 6: dst = D.lr.target; src = S.lr.target; break;
    default: dst = D.lr.grad; src = S.lr.grad; break;
  }
  pbt_copy(dst, src, blockIdx.x < kPbtBufs - 1 ? N_PARAMS : SWARM_GRAD_FLOATS);
  if (blockIdx.x == 0 && threadIdx.x < 32 && ((kPbtCtrlMask >> threadIdx.x) & 1u)) {
    uint32_t* dc = reinterpret_cast<uint32_t*>(D.ctrl);
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(S.ctrl);
    dc[threadIdx.x] = sc[threadIdx.x];
  }
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_pop_exploit(const swarm_pbt_cfg* pbt, const float* score, swarm_adam_cfg* member_hp,
                      const swarm_pop_member* members, int32_t n_members, int32_t* parent, void* stream) {
  if (int e = check_pbt(pbt, score, member_hp, members, n_members, parent)) return e;
  const int threads = (n_members + 63) / 64 * 64;
  hipLaunchKernelGGL(pbt_plan_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, *pbt, score, member_hp,
                     (int)n_members, parent);
  if (int e = (int)hipGetLastError()) return e;
  if (pbt->n_replace == 0) return 0;   // the plan wrote parent[m] = m; nothing to copy
  hipLaunchKernelGGL(pbt_copy_kernel, dim3(kPbtBufs, n_members), dim3(kPbtCopyThreads), 0, (hipStream_t)stream, members,
                     (int)n_members, parent);
  return (int)hipGetLastError();
}

}  // extern "C"
