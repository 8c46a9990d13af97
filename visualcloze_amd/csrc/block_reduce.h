// The ONE fixed-order block reduction of the library and the launch rule of its two-pass users (vc_rk_error_ratio, vc_fm_loss,
// vc_tensor_stats, vc_residual_change; also vc_image_compare, the monitor's first-bad search and GroupNorm's finalize).
// visualcloze_amd/reduction.py restates the same order on the host.  No atomics: a repeated run gives the same bits.
//   pass 1  nblk = min(ceil(units / N), N) blocks of N threads per sample; the units are dealt round-robin - thread t of block k takes
//           units k * N + t, + nblk * N, ... - and a thread adds the elements of its units in ascending order
//   tree    the block's N values: l[t] = op(l[t], l[t + o]) for t < o, o = N / 2, N / 4, .., 1 (neighbouring threads read neighbouring
//           entries: no bank conflict), a barrier behind every round
//   pass 2  ONE block per sample: thread t holds block t's value (the identity for t >= nblk), the same tree
#pragma once
#include "common.h"

// every thread of the block calls it with its v and gets the block's value; `l` is free for reuse when it returns.  op(x, y) combines
// an entry x with the entry y to its right: a several-field reduction is ONE tree over a small struct, combined field by field
template <int N, typename T, typename Op>
VC_DEV T block_tree(T (&l)[N], T v, Op op) {
  const int t = threadIdx.x;
  l[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = N / 2; o >= 1; o >>= 1) {
    if (t < o) l[t] = op(l[t], l[t + o]);
    __syncthreads();
  }
  const T r = l[0];
  __syncthreads();
  return r;
}
struct VcAddOp { template <typename T> VC_DEV T operator()(T x, T y) const { return x + y; } };

// the blocks of pass 1 for a pass 2 of THREADS threads; MAX_BLOCKS: the caller's public VC_*_MAX_BLOCKS (it sizes the scratch)
template <int THREADS, int MAX_BLOCKS>
inline int vc_reduce_blocks(int64_t units) {
  static_assert(THREADS == MAX_BLOCKS, "pass 2 holds one block partial per thread");
  const int64_t want = (units + THREADS - 1) / THREADS;
  return (int)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
}
