// swarm_pbt.h — population-based training (swarm_pop_exploit): the PBT random stream, the entry
// point's checks and the two pure functions of the plan (a member's rank, a child's explored
// row).  The kernels are swarm_pop_pbt.hip.
#pragma once
#include <math.h>

#include "swarm_common.h"

namespace swarm {

// RNG stream id of the PBT draws (third Philox counter word), after STREAM_SAMPLE = 4 of
// swarm_common.h: child m of round r draws the one block philox4x32(r, m, STREAM_PBT, 0, k0, k1)
constexpr uint32_t STREAM_PBT = 5;

constexpr int kPbtBufs = 8;        // the seven learner rows and lr.grad: one copy block each
constexpr int kPbtCopyThreads = 256;
// the words of swarm_ctrl that belong to the optimizer and go from parent to child: adam_step (3),
// loss (5), grad_norm (6), trained (7), beta_pow (10-13), adam_step_size (14), adam_inv_bc2 (15),
// one_m_beta1 / one_m_beta2 (24, 25).  Every other word stays the child's own.
constexpr uint32_t kPbtCtrlMask = (1u << 3) | (1u << 5) | (1u << 6) | (1u << 7) | (0x3Fu << 10) | (3u << 24);
static_assert(sizeof(swarm_ctrl) == 32 * 4, "swarm_ctrl is 32 words");

// what swarm_pop_exploit checks before any launch, in this order
inline int check_pbt(const swarm_pbt_cfg* pbt, const float* score, const swarm_adam_cfg* member_hp,
                     const swarm_pop_member* members, int32_t n_members, const int32_t* parent) {
  if (!pbt || !score || !member_hp || !members || !parent) return SWARM_E_BADARG;
  if (n_members < 1) return SWARM_E_BADARG;
  if (n_members > SWARM_PBT_MAX_MEMBERS) return SWARM_E_UNSUPPORTED;
  if (pbt->n_replace < 0 || pbt->n_replace > n_members / 2) return SWARM_E_BADARG;
  if (pbt->fields & ~(SWARM_PBT_F_LR | SWARM_PBT_F_GAMMA)) return SWARM_E_BADARG;
  // the factors finite and > 0, lo <= hi; the bounds finite and in order, the lr floor > 0 (a
  // child's lr_d is then never 0, which the optimizer reads as "use the float field")
  if (!isfinite(pbt->perturb_lo) || !isfinite(pbt->perturb_hi) || !(pbt->perturb_lo > 0.0f) ||
      !(pbt->perturb_lo <= pbt->perturb_hi))
    return SWARM_E_BADARG;
  if (!isfinite(pbt->gamma_min) || !isfinite(pbt->gamma_max) || !(pbt->gamma_min <= pbt->gamma_max)) return SWARM_E_BADARG;
  if (!isfinite(pbt->lr_min) || !isfinite(pbt->lr_max) || !(pbt->lr_min > 0.0) || !(pbt->lr_min <= pbt->lr_max))
    return SWARM_E_BADARG;
  return 0;
}

// rank(m) = #{ j : s_j > s_m, or s_j == s_m and j < m } over scores in which a NaN was replaced by
// -inf (pbt_score): a total order, so the ranks of n members are a permutation of 0..n-1
__device__ inline float pbt_score(float s) { return s != s ? -INFINITY : s; }
__device__ inline int pbt_rank(const float* s, int n, int m) {
  const float sm = s[m];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const float sj = s[j];
    r += (sj > sm || (sj == sm && j < m)) ? 1 : 0;
  }
  return r;
}

// the child's row: its parent's, with lr and / or gamma perturbed and clamped.  fp32 and double
// products and differences are single roundings (-ffp-contract=off), as numpy forms them.
__device__ inline swarm_adam_cfg pbt_explore(swarm_adam_cfg row, const swarm_pbt_cfg& c, const u32x4& w) {
  if (c.fields & SWARM_PBT_F_LR) {
    const float f = u01(w.y) < 0.5f ? c.perturb_lo : c.perturb_hi;
    const double base = row.lr_d == 0.0 ? (double)row.lr : row.lr_d;
    double x = base * (double)f;
    x = x < c.lr_min ? c.lr_min : x;
    x = x > c.lr_max ? c.lr_max : x;
    row.lr_d = x;
    row.lr = (float)x;
  }
  if (c.fields & SWARM_PBT_F_GAMMA) {
    const float f = u01(w.z) < 0.5f ? c.perturb_lo : c.perturb_hi;
    float g = 1.0f - (1.0f - row.gamma) * f;
    g = g < c.gamma_min ? c.gamma_min : g;
    g = g > c.gamma_max ? c.gamma_max : g;
    row.gamma = g;
  }
  return row;
}

}  // namespace swarm
