// swarm_reduce_body.h — the statements of one slab-reduce block.  NOT a header of declarations:
// it is included INSIDE a kernel's braces, by grad_reduce_kernel (swarm_td.hip) and by the
// population's pop_reduce_kernel (swarm_pop.hip), so both run the same statements in the same
// order and their sums have the same bits, while grad_reduce_kernel's code object stays what it
// was when the statements stood in it (as an inlined function they compiled differently).
// The including kernel provides, under these names:
//   PEER (compile-time int), const float* slabs, swarm_ctrl* ctrl, int n_slabs, int advance,
//   ReduceArgs A (swarm_reduce.h)
// and blockIdx.x is the block's index within ONE learner's reduce: the kRedColBlocks column
// blocks, then in advance mode the control block and the kRedCopyBlocks copy-back blocks.
// `return` leaves the kernel.
  __shared__ float part[kRedGroups][kRedCols];
  __shared__ float part2[kRedRuns][kRedCols];
  __shared__ float peer_rv[PEER ? SWARM_PEER_MAX : 1][kRedCols];
  __shared__ float sqv[kRedCols];
  SWARM_RTSTAMP(22);
  SWARM_STAMP(28);
  swarm_ctrl* C = ctrl;
  if ((int)blockIdx.x > kRedColBlocks) {   // advance mode: a copy-back block
    const int j = (int)blockIdx.x - kRedColBlocks - 1;
    const float4* src = reinterpret_cast<const float4*>(j == 0 ? A.lr.w_nxt : (j == 1 ? A.lr.m_nxt : A.lr.v_nxt));
    float4* dst = reinterpret_cast<float4*>(j == 0 ? A.lr.w_cur : (j == 1 ? A.lr.m_cur : A.lr.v_cur));
    if ((int)threadIdx.x < N_PARAMS_PAD / 4) dst[threadIdx.x] = src[threadIdx.x];
    return;
  }
  if ((int)blockIdx.x == kRedColBlocks) {   // advance mode: the control block (red_control)
    RedCtrl rc;
    rc.capacity = A.capacity; rc.B = A.B; rc.batch = A.batch; rc.hp = A.hp; rc.k0 = A.k0; rc.k1 = A.k1;
    red_control(C, rc);
    return;
  }
  const int c = threadIdx.x % kRedCols;
  const int col = blockIdx.x * kRedCols + c;
  const int q = threadIdx.x / kRedCols;
  const int per = (n_slabs + kRedGroups - 1) / kRedGroups;
  const int b0 = q * per, b1 = min(n_slabs, b0 + per);
  // first chunk of this thread's slab column in flight before anything else.  Column col of
  // slab b is scol[16 b] (swarm_common.h slab_index): one 64-bit base per thread, 32-bit offsets
  constexpr int kChunk = kRedChunk;
  static_assert(kSlabCols == 16, "slab column blocks of 16");
  const float* const scol = slabs + ((size_t)(col >> 4) * (size_t)n_slabs * kSlabCols + (size_t)(col & 15));
  float v0[kChunk];
#pragma unroll
  for (int j = 0; j < kChunk; ++j)
    v0[j] = (col <= N_PARAMS && b0 + j < b1) ? scol[(uint32_t)(b0 + j) * kSlabCols] : 0.0f;
  float s = v0[0];
#pragma unroll
  for (int j = 1; j < kChunk; ++j) s = s + v0[j];
  if (col <= N_PARAMS) {
    for (int b = b0 + kChunk; b < b1; b += kChunk) {
      float v[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; ++j) v[j] = (b + j < b1) ? scol[(uint32_t)(b + j) * kSlabCols] : 0.0f;
#pragma unroll
      for (int j = 0; j < kChunk; ++j) s = s + v[j];
    }
  }
  SWARM_STAMP(29);
  part[q][c] = s;
  __syncthreads();
  SWARM_STAMP(30);
  if (q < kRedRuns) {
    float r = part[8 * q][c];
#pragma unroll
    for (int gi = 1; gi < 8; ++gi) r = r + part[8 * q + gi][c];
    part2[q][c] = r;
  }
  __syncthreads();
  float gcol = 0.0f;   // q == 0: this column's gradient as written to grad
  if (q == 0 && col <= N_PARAMS) {
    float tot = part2[0][c];
#pragma unroll
    for (int gi = 1; gi < kRedRuns; ++gi) tot = tot + part2[gi][c];
    if (PEER) part[0][c] = tot;   // part[0] is free again: this rank's column sums
    else A.grad[col] = tot;
    gcol = tot;
    // this rank's loss of the update (0 when skipped: the TD launch wrote zero slabs)
    if (advance && col == N_PARAMS) C->loss = tot / (float)((size_t)A.batch * A.N);
  }
  if (PEER) {
    __syncthreads();
    peer_exchange<kRedCols>(A.peer, 0, blockIdx.x, q, c, col, N_PARAMS + 1, part[0], peer_rv, &C->peer_hold);
    if (q == 0 && col <= N_PARAMS) {
      float tot = peer_rv[0][c];
      for (int w = 1; w < A.peer.world_size; ++w) tot = tot + peer_rv[w][c];
      A.grad[col] = tot;
      gcol = tot;
    }
  }
  // the clip norm's partial of these 16 columns = parameter group blockIdx.x (swarm_adam.h):
  // lanes 0-15 of wave 0 hold the columns; squares as the optimizer step forms them (scaled by
  // 1/W first when W > 1), the float4 sums ((a + b) + c) + d by lanes 0-3, then their quad sum
  if (q == 0) {
    float g = col < N_PARAMS ? gcol : 0.0f;
    if (A.hp.world_size > 1) g = g * (1.0f / (float)A.hp.world_size);
    sqv[c] = g * g;
  }
  wave_lds_sync();   // sqv is written and read by wave 0 only
  if (threadIdx.x < 4) {
    const int f = threadIdx.x;
    const float d = ((sqv[4 * f] + sqv[4 * f + 1]) + sqv[4 * f + 2]) + sqv[4 * f + 3];
    const float sq = quad_sum(d);
    if (f == 0) A.grad[kGradSqBase + blockIdx.x] = sq;
  }
  SWARM_STAMP(31);
  SWARM_RTSTAMP(23);
