// swarm_qbk.hip — the q_backward_kernel instantiations (swarm_qbk.h) and their launch; the entry
// point swarm_q_backward is in swarm_td.hip, beside the slab reduce it launches next.  gfx950 only.
//
// Reference: loss.backward() through model(batch), src/training/train_gcn_dqn.py:122-124.
#include "swarm_launch.h"
#include "swarm_qbk.h"

namespace swarm {

// q_backward_kernel<td_wave_slots(GS), GS, SPEC>: the TD kernel's slots and specs (TdSpecs: the two
// complete-graph specs, SPEC_RUNTIME for kNN / radius / dense)
int qbk_launch(const QbArgs& A, hipStream_t stream) {
  with_slots<8, 16, 32>(A.N, [&](auto gs) {
    constexpr int GS = decltype(gs)::value, NS = td_wave_slots(GS);
    with_spec<TdSpecs>(A.graph, A.conv, [&](auto sp) {
      hipLaunchKernelGGL((q_backward_kernel<NS, GS, decltype(sp)::value>), dim3(A.n_slabs), dim3(64 * (kTdRows / NS)), 0,
                         stream, A);
    });
  });
  return (int)hipGetLastError();
}

}  // namespace swarm
