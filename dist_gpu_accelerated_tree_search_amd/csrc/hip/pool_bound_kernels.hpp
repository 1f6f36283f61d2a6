// What an unfinished PFSP search has proved: the bound of every node of the device ring
// (IEngine::pool_bound, core/engine_api.hpp PoolBound), recomputed by a kernel — front
// nodes carry their fronts and job set but not their bound, permutation nodes only the
// permutation.
//
// One kernel family per node layout, all scanning the ring slice (bot + i) & cap_mask,
// i < n, with a grid-stride loop as pool_weight_kernel does, the p table staged in LDS as
// the search kernels stage it (rows of PfspConsts<M>::MS u16, read with load_prow):
//   front nodes         one thread per node: remain = the p rows of the node's unscheduled
//                       set summed per machine, then the machine-bound chain over
//                       front + remain + minimum tail, in 32 bits (a u16 front plus a
//                       remain may pass 65535). Every machine of the bucket takes part:
//                       a padding machine has p = 0, no tail and, below the root, the
//                       last real machine's front, so its terms repeat that machine's;
//                       at the root its head is the cheapest job's whole route, which
//                       min_heads + column sum of the last real machine covers.
//   permutation, LB1    one thread per node: front and remain replayed from the prefix
//                       (pfsp_lb1_parent's replay), the root from the minimum heads.
//   permutation, LB2    one wave per node, a lane per machine pair (pairs lane, lane + 64,
//                       ...): a node costs O(pairs x jobs) Johnson steps against O(depth x
//                       machines) for its prefix, so the prefix (scheduled set by LDS
//                       atomics, front replayed by every lane alike: uniform reads, no
//                       extra issue slots) is paid once per node and shared through LDS,
//                       and the pairs, 45 or 190 from 10 machines, fill most of a wave.
//                       A thread per node would hold 64 different scheduled sets and
//                       prefixes per wave and walk them divergently; a lane per (node,
//                       pair) across nodes would gather the fronts of several nodes. With
//                       5 machines (10 pairs) most lanes idle; those pools are small.
//                       The records come from LDS where the search kernel keeps them
//                       there (P x NJ x 8 B <= 32 KB), else from global memory: a lane
//                       walks its own pair's row, 8 consecutive bytes a step.
//                       A lane stops once its partial max reaches cap (the node is stale).
// Each workgroup keeps the histogram in LDS (32-bit LDS atomics: a workgroup counts at
// most n / gridDim + 1 nodes a bin) and flushes the non-zero bins with one 64-bit global
// atomic each; bins past kBoundLdsBins go to global memory directly. The minimum is
// reduced across each wave, then one atomicMin per workgroup.
#pragma once

#include "pfsp_front_kernels.hpp"
#include "pfsp_kernels.hpp"

namespace tts {
namespace dev {

constexpr int kBoundLdsBins = 1024;
constexpr int kBoundMaxBlocks = 4096;

struct BoundSmem {
  uint32_t hist[kBoundLdsBins];
  int wmin[kBlock / kWave];
};

__device__ inline void bound_smem_init(BoundSmem& s) {
  for (int i = threadIdx.x; i < kBoundLdsBins; i += kBlock) s.hist[i] = 0u;
}

// One node of own bound `own` (>= cap: stale). cap >= b >= 0, so cap - b fits 31 bits.
__device__ inline void bound_count(BoundSmem& s, u64* __restrict__ hist, int bins, int cap, int own, int& lo) {
  const int b = min(own, cap);
  const uint32_t k = static_cast<uint32_t>(cap) - static_cast<uint32_t>(b);
  const int bin = k < static_cast<uint32_t>(bins - 1) ? static_cast<int>(k) : bins - 1;
  if (bin < kBoundLdsBins)
    atomicAdd(&s.hist[bin], 1u);
  else
    atomicAdd(&hist[bin], 1ull);
  lo = min(lo, b);
}

// After the scan (every thread of the workgroup): contains __syncthreads().
__device__ inline void bound_flush(BoundSmem& s, u64* __restrict__ hist, int bins, int* __restrict__ lower, int lo) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) s.wmin[threadIdx.x / kWave] = lo;
  __syncthreads();
  const int nb = bins < kBoundLdsBins ? bins : kBoundLdsBins;
  for (int i = threadIdx.x; i < nb; i += kBlock) {
    const uint32_t c = s.hist[i];
    if (c) atomicAdd(&hist[i], static_cast<u64>(c));
  }
  if (threadIdx.x == 0) {
    int m = s.wmin[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) m = min(m, s.wmin[w]);
    atomicMin(lower, m);
  }
}

// The p table, job-major rows of MS u16 (an even count): rows [0, jobs) from `src`, zero
// rows up to NJ, so a job id of a foreign node never reads past what was staged.
template <int NJ, int MS>
__device__ inline void bound_stage_ptab(uint16_t (&dst)[NJ][MS], const uint16_t* __restrict__ src, int jobs) {
  static_assert(MS % 2 == 0, "rows are copied as 32-bit words");
  uint32_t* d = reinterpret_cast<uint32_t*>(&dst[0][0]);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  const int have = min(jobs, NJ) * (MS / 2);
  for (int i = threadIdx.x; i < NJ * (MS / 2); i += kBlock) d[i] = i < have ? s[i] : 0u;
}

// f(job) for every job of a set, lowest first, one 64-bit word at a time.
template <class F>
__device__ inline void bound_for_each_job(uint32_t x, F f) {
  for (; x; x &= x - 1) f(__builtin_ctz(x));
}
template <class F>
__device__ inline void bound_for_each_job(uint64_t x, F f) {
  for (; x; x &= x - 1) f(__builtin_ctzll(x));
}
template <int W, class F>
__device__ inline void bound_for_each_job(const JobSet<W>& s, F f) {
  for (int k = 0; k < W; ++k)
    for (uint64_t x = s.w[k]; x; x &= x - 1) f(64 * k + __builtin_ctzll(x));
}

// ---- front nodes ---------------------------------------------------------------------------
template <int M, int NJ>
struct FrontBoundSmem {
  alignas(16) uint16_t ptab[NJ][FrontGeom<M, NJ>::MS];
  BoundSmem b;
};

template <int M, int NJ>
__global__ __launch_bounds__(kBlock) void pool_bound_front_kernel(PfspFrontArgs<M, NJ> a, u64 bot, u64 n, int cap,
                                                                  int bins, u64* __restrict__ hist,
                                                                  int* __restrict__ lower) {
  using G = FrontGeom<M, NJ>;
  using Node = typename G::Node;
  static_assert(G::MS == PfspConsts<M>::MS, "load_prow reads the front table's rows");
  __shared__ FrontBoundSmem<M, NJ> sm;
  bound_stage_ptab<NJ, G::MS>(sm.ptab, a.ptab, a.jobs);
  bound_smem_init(sm.b);
  __syncthreads();
  int lo = cap;
  for (u64 i = static_cast<u64>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kBlock) {
    const Node& nd = a.pool.ring[(bot + i) & a.pool.cap_mask];
    int r[M];
#pragma unroll
    for (int m = 0; m < M; ++m) r[m] = 0;
    const typename G::Mask rest = nd.rest;
    bound_for_each_job(rest, [&](int j) {
      if (j >= NJ) return;
      int pr[M];
      load_prow<M>(sm.ptab[j], pr);
#pragma unroll
      for (int m = 0; m < M; ++m) r[m] += pr[m];
    });
    int run = static_cast<int>(nd.front[0]) + r[0];
    int lb = run + a.min_tails[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
      run = max(run, static_cast<int>(nd.front[m]) + r[m]);
      lb = max(lb, run + a.min_tails[m]);
    }
    bound_count(sm.b, hist, bins, cap, lb, lo);
  }
  bound_flush(sm.b, hist, bins, lower, lo);
}

// ---- permutation nodes ---------------------------------------------------------------------
// The front of the prefix prmu[0..d) (the root: the minimum heads) and, with REMAIN, the
// unscheduled work per machine, as pfsp_lb1_parent replays them.
template <int NJ, int M, bool REMAIN>
__device__ inline void bound_replay_prefix(const PfspArgs<NJ, M>& a, const uint16_t (&ptab)[NJ][PfspConsts<M>::MS],
                                           const PfspNode<NJ>& nd, int d, int (&f)[M], int (&r)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    f[m] = (d == 0) ? a.min_heads[m] : 0;
    r[m] = a.sum_all[m];
  }
  for (int i = 0; i < d; ++i) {
    const int job = min(static_cast<int>(nd.prmu[i]), NJ - 1);
    int pr[M];
    load_prow<M>(ptab[job], pr);
    f[0] += pr[0];
    if (REMAIN) r[0] -= pr[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
      f[m] = max(f[m - 1], f[m]) + pr[m];
      if (REMAIN) r[m] -= pr[m];
    }
  }
}

template <int NJ, int M>
struct PermBoundSmem {
  alignas(16) uint16_t ptab[NJ][PfspConsts<M>::MS];
  BoundSmem b;
};

template <int NJ, int M>
__global__ __launch_bounds__(kBlock) void pool_bound_lb1_kernel(PfspArgs<NJ, M> a, u64 bot, u64 n, int cap, int bins,
                                                                u64* __restrict__ hist, int* __restrict__ lower) {
  __shared__ PermBoundSmem<NJ, M> sm;
  bound_stage_ptab<NJ, PfspConsts<M>::MS>(sm.ptab, a.ptab, a.jobs);
  bound_smem_init(sm.b);
  __syncthreads();
  int lo = cap;
  for (u64 i = static_cast<u64>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kBlock) {
    const PfspNode<NJ>& nd = a.pool.ring[(bot + i) & a.pool.cap_mask];
    const int d = min(static_cast<int>(nd.depth), a.jobs);
    int f[M], r[M];
    bound_replay_prefix<NJ, M, true>(a, sm.ptab, nd, d, f, r);
    int run = f[0] + r[0];
    int lb = run + a.min_tails[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
      run = max(run, f[m] + r[m]);
      lb = max(lb, run + a.min_tails[m]);
    }
    bound_count(sm.b, hist, bins, cap, lb, lo);
  }
  bound_flush(sm.b, hist, bins, lower, lo);
}

template <int NJ, int M>
struct Lb2BoundSmem {
  using C = PfspConsts<M>;
  static constexpr int WPB = kBlock / kWave;  // nodes per workgroup and trip: one per wave
  static constexpr int NW = (NJ + 63) / 64;
  static constexpr bool kRecsInLds = C::P * NJ * 8 <= 32 * 1024;  // as PfspSmem::kRecsInLds
  alignas(16) uint16_t ptab[NJ][C::MS];
  uint2 recs[kRecsInLds ? C::P * NJ : 1];
  u64 mask[WPB][NW];   // scheduled set of the wave's node
  int front[WPB][M];   // ... and its front
  BoundSmem b;
};

template <int NJ, int M>
__global__ __launch_bounds__(kBlock) void pool_bound_lb2_kernel(PfspArgs<NJ, M> a, u64 bot, u64 n, int cap, int bins,
                                                                u64* __restrict__ hist, int* __restrict__ lower) {
  using S = Lb2BoundSmem<NJ, M>;
  __shared__ S sm;
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int N = min(a.jobs, NJ);
  const int npairs = min(a.npairs, PfspConsts<M>::P);
  bound_stage_ptab<NJ, PfspConsts<M>::MS>(sm.ptab, a.ptab, a.jobs);
  if constexpr (S::kRecsInLds)
    for (int i = threadIdx.x; i < npairs * N; i += kBlock) sm.recs[i] = a.recs[i];
  bound_smem_init(sm.b);
  const uint2* recs = S::kRecsInLds ? sm.recs : a.recs;
  int lo = cap;
  // (the trip count is the same for the four waves of a workgroup: barriers inside)
  for (u64 base = static_cast<u64>(blockIdx.x) * S::WPB; base < n; base += static_cast<u64>(gridDim.x) * S::WPB) {
    const bool valid = base + wid < n;
    if (lane < S::NW) sm.mask[wid][lane] = 0ull;
    __syncthreads();
    if (valid) {
      const PfspNode<NJ>& nd = a.pool.ring[(bot + base + wid) & a.pool.cap_mask];
      const int d = min(static_cast<int>(nd.depth), N);
      for (int i = lane; i < d; i += kWave) {
        const int job = min(static_cast<int>(nd.prmu[i]), NJ - 1);
        atomicOr(&sm.mask[wid][job >> 6], 1ull << (job & 63));
      }
      int f[M], unused[M];
      bound_replay_prefix<NJ, M, false>(a, sm.ptab, nd, d, f, unused);
      if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) sm.front[wid][m] = f[m];
      }
    }
    __syncthreads();
    if (valid) {
      u64 msk[S::NW];
#pragma unroll
      for (int w = 0; w < S::NW; ++w) msk[w] = sm.mask[wid][w];
      int lb = 0;
      for (int q = lane; q < npairs; q += kWave) {
        const uint2 pi = a.pinfo[q];
        const int m0 = pi.x & 0xff, m1 = (pi.x >> 8) & 0xff;
        int t0 = sm.front[wid][m0], t1 = sm.front[wid][m1];
        const uint2* rq = recs + static_cast<size_t>(pi.x >> 16) * N;
        for (int r = 0; r < N; ++r) {
          const uint2 rc = rq[r];
          const int jb = rc.x & 0xffff;
          const int n0 = t0 + static_cast<int>(rc.x >> 16);
          const int n1 = max(t1, n0 + static_cast<int>(rc.y >> 16)) + static_cast<int>(rc.y & 0xffff);
          const bool sched = job_in<S::NW>(msk, jb);
          t0 = sched ? t0 : n0;
          t1 = sched ? t1 : n1;
        }
        lb = max(lb, max(t1 + static_cast<int>(pi.y >> 16), t0 + static_cast<int>(pi.y & 0xffff)));
        if (lb >= cap) break;
      }
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) lb = max(lb, __shfl_xor(lb, o, kWave));
      if (lane == 0) bound_count(sm.b, hist, bins, cap, lb, lo);
    }
  }
  bound_flush(sm.b, hist, bins, lower, lo);
}

// Blocks of a scan of n nodes, `per` nodes a workgroup and trip.
inline int bound_blocks(u64 n, int per) {
  const u64 b = (n + static_cast<u64>(per) - 1) / static_cast<u64>(per);
  return static_cast<int>(b < static_cast<u64>(kBoundMaxBlocks) ? (b ? b : 1) : kBoundMaxBlocks);
}

}  // namespace dev
}  // namespace tts
