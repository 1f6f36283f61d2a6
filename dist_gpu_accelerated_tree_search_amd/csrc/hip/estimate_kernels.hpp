// Device Knuth probes for PFSP (LB1, LB1_d, LB2): the kernel behind estimate_device.hpp.
//
// One wave walks one probe from the root to its dead end; the waves of the grid stride
// over the probe indices of a launch. Probe i makes the choices of the host twin's probe
// i (core/estimate.hpp knuth_estimate_indexed, core/probe_rng.hpp), so its estimate, its
// depth and its jobs are the twin's, bit for bit.
//
// The node is wave-uniform and lives in the wave's slice of LDS: per-machine front and
// remain in int32 (no 16-bit range rule here) and the unscheduled set as 64-bit words.
// A level takes one pass per set word: lane l of pass k bounds the child that appends job
// 64 k + l, the ballot of `lb < best` is that word of the survivor set, and the survivors
// are by construction in ascending job order.
//   LB1 / LB1_d  the O(M) max-plus chain from the parent's front (cpu_lb1_children; LB1 has
//                the same values, processing times being non-negative). The root's front
//                is all zero: a chain from zero passes the minimum heads on every machine,
//                so the root-child bounds and fronts equal those from min_heads.
//   LB2          the child's front (kept per lane in LDS: the pair's machines index it),
//                then machine pairs in lb2_pair_order with exit once the partial max
//                reaches `best`; each pair is a Johnson walk over the unscheduled jobs
//                (cpu_lb2). The walk's data is wave-uniform (job order, times, lags);
//                only "is this my own job" differs between lanes. `lb < best` equals the
//                host's decision, the value past the exit is not the host's.
// Tables: cum[m][j] = sum of p[i][j] over i < m, (M + 1) x N int32, from which
// p[m][j] = cum[m+1][j] - cum[m][j] and a pair's lag = cum[m1][j] - cum[m0+1][j]; the
// minimum tails; for LB2 the Johnson orders (u16 job ids) and the pairs (m0 | m1 << 8) in
// evaluation order. Every workgroup stages them in LDS; an instance whose tables and wave
// state do not fit is refused by the launcher (estimate_device.hip). No scratch: nothing
// per lane is indexed.
//
// Floating point: w = w * k and est = est + w are two round-to-nearest operations
// (__dmul_rn / __dadd_rn are never contracted), as on the host, so estimates beyond 2^53
// agree too.
//
// Not built (no measurement asked for them yet): two or three probes per wave for
// instances of at most 32 jobs, where a level leaves most lanes idle, and dealing LB2's
// (child, pair) tasks over the lanes instead of one child per lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../core/probe_rng.hpp"
#include "device_common.hpp"

namespace tts {
namespace dev {

constexpr int kEstMaxWords = 8;  // 512 jobs

struct EstParams {
  int jobs, machines, pairs, lb, best;
  int words;               // 64-bit words of the job set
  u64 seed;
  u64 first_probe;         // index of the launch's first probe (enters the hash)
  u64 count;               // probes of this launch
  const int* cum;          // [(M + 1)][N]
  const int* tails;        // [M]
  const uint16_t* johnson; // [P][N] by pair id (LB2)
  const uint16_t* pair;    // [P] m0 | m1 << 8 of evaluation step i (lb2_pair_order)
  const uint16_t* pair_id; // [P] pair id of evaluation step i (row of johnson)
  double* partial;         // [grid][3 + N]: sum est, sum est^2, sum depth, per-level sum w
  double* rec_est;         // per-probe records of this launch, or null
  int* rec_depth;
  int16_t* rec_jobs;       // [count][N], preset to -1
};

// LDS of one workgroup, in bytes, for `waves` waves (the launcher's size and the kernel's
// carve-up come from this one function).
struct EstLds {
  unsigned cum, tails, johnson, pair, pair_id, wave0, wave_bytes, total;
  unsigned w_front, w_remain, w_set, w_surv, w_lvl, w_cf, w_sum;  // offsets inside a wave's slice
};
__host__ __device__ inline unsigned est_align8(unsigned x) { return (x + 7u) & ~7u; }
__host__ __device__ inline EstLds est_lds_layout(int N, int M, int P, bool lb2, int waves) {
  EstLds L{};
  unsigned o = 0;
  L.cum = o;
  o += static_cast<unsigned>((M + 1) * N) * 4u;
  L.tails = o;
  o += static_cast<unsigned>(M) * 4u;
  L.johnson = o;
  if (lb2) o += static_cast<unsigned>(P * N) * 2u;
  L.pair = o;
  if (lb2) o += static_cast<unsigned>(P) * 2u;
  L.pair_id = o;
  if (lb2) o += static_cast<unsigned>(P) * 2u;
  o = est_align8(o);
  L.wave0 = o;
  unsigned w = 0;
  L.w_set = w;
  w += kEstMaxWords * 8u;
  L.w_surv = w;
  w += kEstMaxWords * 8u;
  L.w_sum = w;
  w += 3u * 8u;
  L.w_lvl = w;
  w += static_cast<unsigned>(N) * 8u;
  L.w_front = w;
  w += static_cast<unsigned>(M) * 4u;
  L.w_remain = w;
  w += static_cast<unsigned>(M) * 4u;
  L.w_cf = w;
  if (lb2) w += static_cast<unsigned>(M) * kWave * 4u;
  L.wave_bytes = est_align8(w);
  L.total = L.wave0 + L.wave_bytes * static_cast<unsigned>(waves);
  return L;
}

template <bool kLb2>
__global__ void __launch_bounds__(kBlock) knuth_probe_kernel(EstParams a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char est_smem[];
  const int N = a.jobs, M = a.machines, P = a.pairs, W = a.words;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  const EstLds L = est_lds_layout(N, M, P, kLb2, waves);

  int* cum = reinterpret_cast<int*>(est_smem + L.cum);
  int* tails = reinterpret_cast<int*>(est_smem + L.tails);
  uint16_t* johnson = reinterpret_cast<uint16_t*>(est_smem + L.johnson);
  uint16_t* pair = reinterpret_cast<uint16_t*>(est_smem + L.pair);
  uint16_t* pair_id = reinterpret_cast<uint16_t*>(est_smem + L.pair_id);
  for (int i = threadIdx.x; i < (M + 1) * N; i += blockDim.x) cum[i] = a.cum[i];
  for (int i = threadIdx.x; i < M; i += blockDim.x) tails[i] = a.tails[i];
  if constexpr (kLb2) {
    for (int i = threadIdx.x; i < P * N; i += blockDim.x) johnson[i] = a.johnson[i];
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      pair[i] = a.pair[i];
      pair_id[i] = a.pair_id[i];
    }
  }
  unsigned char* mine = est_smem + L.wave0 + L.wave_bytes * static_cast<unsigned>(wid);
  u64* set = reinterpret_cast<u64*>(mine + L.w_set);
  u64* surv = reinterpret_cast<u64*>(mine + L.w_surv);
  double* wsum = reinterpret_cast<double*>(mine + L.w_sum);
  double* lvl = reinterpret_cast<double*>(mine + L.w_lvl);
  int* front = reinterpret_cast<int*>(mine + L.w_front);
  int* remain = reinterpret_cast<int*>(mine + L.w_remain);
  int* cf = reinterpret_cast<int*>(mine + L.w_cf);  // [M][kWave], LB2 only
  for (int i = lane; i < N; i += kWave) lvl[i] = 0.0;
  __syncthreads();
  int total = 0;  // lane m: all the work of machine m, the root's remain
  if (lane < M)
    for (int j = 0; j < N; ++j) total += cum[(lane + 1) * N + j] - cum[lane * N + j];

  double sum = 0, sum2 = 0, sumd = 0;
  const u64 gw = static_cast<u64>(blockIdx.x) * waves + wid;
  const u64 stride = static_cast<u64>(gridDim.x) * waves;
  for (u64 i = gw; i < a.count; i += stride) {
    // ---- root: nothing scheduled, front 0, remain = machine totals ----
    // (the node's words are stored by every lane with the same wave-uniform value, so each
    // lane later reads what it wrote itself; only the root's front and remain come from
    // lane m alone, and the wave-scope fence orders them before the first level's reads)
    for (int k = 0; k < W; ++k) {
      const int b = N - 64 * k;
      set[k] = b >= 64 ? ~0ull : (b <= 0 ? 0ull : ((1ull << b) - 1ull));
    }
    if (lane < M) {  // M <= kWave
      front[lane] = 0;
      remain[lane] = total;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t h = probe_hash(a.seed, a.first_probe + i);
    double w = 1.0, est = 0.0;
    int depth = 0;
    // a parent at depth N - 1 has one leaf child, and leaves are never pushed
    while (depth < N - 1) {
      int ktotal = 0;
      for (int k = 0; k < W; ++k) {
        const u64 s = set[k];
        u64 sv = 0;
        if (s != 0) {
          const bool have = (s >> lane) & 1ull;
          const int j = have ? 64 * k + lane : 0;  // lanes without a child walk job 0's data, unused
          int lb;
          bool ok = have;
          if constexpr (!kLb2) {
            const int f0 = front[0];
            lb = f0 + remain[0] + tails[0];
            int t = f0 + (cum[N + j] - cum[j]);
            for (int m = 1; m < M; ++m) {
              const int st = max(t, front[m]);
              lb = max(lb, st + remain[m] + tails[m]);
              t = st + (cum[(m + 1) * N + j] - cum[m * N + j]);
            }
            ok = have && lb < a.best;
          } else {
            int f = front[0] + (cum[N + j] - cum[j]);
            cf[lane] = f;
            for (int m = 1; m < M; ++m) {
              f = max(f, front[m]) + (cum[(m + 1) * N + j] - cum[m * N + j]);
              cf[m * kWave + lane] = f;
            }
            lb = 0;
            bool act = have;
            for (int qi = 0; qi < P; ++qi) {
              if (__ballot(act) == 0) break;
              const int pr = pair[qi];
              const int m0 = pr & 0xff, m1 = pr >> 8;
              const uint16_t* ord = johnson + static_cast<int>(pair_id[qi]) * N;
              const int* c0 = cum + m0 * N;
              const int* c1 = cum + m1 * N;
              int t0 = cf[m0 * kWave + lane], t1 = cf[m1 * kWave + lane];
              for (int r = 0; r < N; ++r) {
                // wave-uniform: the order and the set are the wave's, so the branch is scalar
                const int jj = __builtin_amdgcn_readfirstlane(static_cast<int>(ord[r]));
                if (!__builtin_amdgcn_readfirstlane(static_cast<int>((set[jj >> 6] >> (jj & 63)) & 1ull))) continue;
                const int e0 = c0[N + jj];
                const int p0 = e0 - c0[jj];
                const int b1 = c1[jj];
                const int lag = b1 - e0;
                const int p1 = c1[N + jj] - b1;
                if (jj != j) {
                  t0 += p0;
                  t1 = max(t1, t0 + lag) + p1;
                }
              }
              if (act) {
                lb = max(lb, max(t1 + tails[m1], t0 + tails[m0]));
                if (lb >= a.best) act = false;
              }
            }
            ok = have && lb < a.best;
          }
          sv = __ballot(ok);
        }
        surv[k] = sv;
        ktotal += __popcll(sv);
      }
      if (ktotal == 0) break;
      w = __dmul_rn(w, static_cast<double>(ktotal));
      est = __dadd_rn(est, w);
      lvl[depth] = __dadd_rn(lvl[depth], w);
      // ---- the idx-th survivor in ascending job order ----
      uint32_t idx = probe_pick(probe_draw(h, static_cast<uint32_t>(depth)), static_cast<uint32_t>(ktotal));
      int word = 0;
      u64 sv = surv[0];
      for (int k = 0; k < W - 1; ++k) {
        const uint32_t c = static_cast<uint32_t>(__popcll(sv));
        if (idx < c) break;
        idx -= c;
        word = k + 1;
        sv = surv[k + 1];
      }
      const bool hit = ((sv >> lane) & 1ull) && static_cast<uint32_t>(__popcll(sv & lanemask_lt())) == idx;
      const u64 hits = __ballot(hit);  // exactly one lane: idx < popcount(sv)
      const int bit = hits ? __builtin_ctzll(hits) : 0;
      const int job = 64 * word + bit;
      if (a.rec_jobs && lane == 0) a.rec_jobs[i * static_cast<u64>(N) + depth] = static_cast<int16_t>(job);
      // ---- the child becomes the node (wave-uniform values, stored by every lane) ----
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      int f = front[0] + (cum[N + job] - cum[job]);
      front[0] = f;
      remain[0] -= cum[N + job] - cum[job];
      for (int m = 1; m < M; ++m) {
        const int pm = cum[(m + 1) * N + job] - cum[m * N + job];
        f = max(f, front[m]) + pm;
        front[m] = f;
        remain[m] -= pm;
      }
      set[word] = set[word] & ~(1ull << bit);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      ++depth;
    }
    sum = __dadd_rn(sum, est);
    sum2 = __dadd_rn(sum2, __dmul_rn(est, est));
    sumd += depth;
    if (a.rec_est && lane == 0) {
      a.rec_est[i] = est;
      a.rec_depth[i] = depth;
    }
  }
  wsum[0] = sum;
  wsum[1] = sum2;
  wsum[2] = sumd;
  __syncthreads();
  // the workgroup's partial sums: its waves in wave order
  for (int t = threadIdx.x; t < 3 + N; t += blockDim.x) {
    double x = 0;
    for (int v = 0; v < waves; ++v) {
      const unsigned char* ws = est_smem + L.wave0 + L.wave_bytes * static_cast<unsigned>(v);
      x += t < 3 ? reinterpret_cast<const double*>(ws + L.w_sum)[t] : reinterpret_cast<const double*>(ws + L.w_lvl)[t - 3];
    }
    a.partial[static_cast<u64>(blockIdx.x) * (3 + N) + t] = x;
  }
}

// ---- Lookahead probes (core/estimate.hpp lookahead_estimate_indexed) ----
// The same wave, node, tables and partial sums as above; a level is
//   1. the survivor pass over the node, as in the Knuth kernel: k, est += w k;
//   2. a wave-uniform loop over the survivor bits, ascending: child c's front, remain and set
//      go to a second node in LDS, the per-word passes over c's children give k_c under the
//      lookahead bound (the model's, or the LB1 chain for an LB2 model), and kc[c] and the
//      running sum of the weights k_c^power, pre[c], go to LDS. Everything here is
//      wave-uniform, so the prefix sums are a scalar running sum, exact in u64;
//   3. x = probe_pick_weighted(draw, T); lane l of word k asks whether survivor 64 k + l has
//      pre > x, and the first such lane of the first such word is the pick (pre does not
//      decrease along the survivors, and a survivor of weight 0 repeats its predecessor's);
//   4. w = (w T) / wt as a product and then a quotient, and the pick becomes the node.
// Floating point: every product, sum and quotient of doubles here goes through look_mul /
// look_add / look_div, whose bodies switch contraction off. __dmul_rn and __dadd_rn are an
// inline `*` and `+` that device code compiles with contraction allowed, so a product that
// feeds a sum becomes one v_fmac_f64 with one rounding; a lookahead probe adds w k at every
// level of a walk twice as deep as a Knuth probe's and would then differ from the host in
// the last bit of est.
// The two bounding blocks of the Knuth kernel are copied into est_word_lb1 / est_word_lb2
// (one node, one set word, the survivor ballot) instead of shared with it: that kernel's
// code and resource numbers stay what profiles/r15 records. Nothing per lane is indexed:
// kc and pre live in LDS.
struct LookParams {
  EstParams e;
  int power;  // 1, 2 or 3
};

struct LookLds {
  EstLds base;  // tables and the Knuth wave state; wave_bytes and total include what follows
  unsigned w_pre, w_set2, w_kc, w_front2, w_remain2;
};
__host__ __device__ inline LookLds look_lds_layout(int N, int M, int P, bool lb2, int waves) {
  LookLds L{};
  L.base = est_lds_layout(N, M, P, lb2, waves);
  unsigned w = L.base.wave_bytes;  // 8-aligned
  L.w_pre = w;
  w += static_cast<unsigned>(N) * 8u;
  L.w_set2 = w;
  w += kEstMaxWords * 8u;
  L.w_kc = w;
  w += static_cast<unsigned>(N) * 4u;
  L.w_front2 = w;
  w += static_cast<unsigned>(M) * 4u;
  L.w_remain2 = w;
  w += static_cast<unsigned>(M) * 4u;
  L.base.wave_bytes = est_align8(w);
  L.base.total = L.base.wave0 + L.base.wave_bytes * static_cast<unsigned>(waves);
  return L;
}

__device__ __forceinline__ double look_mul(double x, double y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ double look_add(double x, double y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ double look_div(double x, double y) {
#pragma clang fp contract(off)
  return x / y;
}

__device__ __forceinline__ u64 est_uniform(u64 x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
  return (static_cast<u64>(hi) << 32) | lo;
}

// Survivors among the children of node (front, remain) that append the jobs of set word k
// (s, not 0): the LB1 / LB1_d chain of the Knuth kernel.
__device__ __forceinline__ u64 est_word_lb1(int N, int M, int k, int lane, u64 s, const int* front, const int* remain,
                                            const int* cum, const int* tails, int best) {
  const bool have = (s >> lane) & 1ull;
  const int j = have ? 64 * k + lane : 0;  // lanes without a child walk job 0's data, unused
  const int f0 = front[0];
  int lb = f0 + remain[0] + tails[0];
  int t = f0 + (cum[N + j] - cum[j]);
  for (int m = 1; m < M; ++m) {
    const int st = max(t, front[m]);
    lb = max(lb, st + remain[m] + tails[m]);
    t = st + (cum[(m + 1) * N + j] - cum[m * N + j]);
  }
  return __ballot(have && lb < best);
}

// The same under LB2 (the Knuth kernel's block): `set` is the node's whole job set.
__device__ __forceinline__ u64 est_word_lb2(int N, int M, int P, int k, int lane, u64 s, const int* front,
                                            const u64* set, const int* cum, const int* tails, const uint16_t* johnson,
                                            const uint16_t* pair, const uint16_t* pair_id, int* cf, int best) {
  const bool have = (s >> lane) & 1ull;
  const int j = have ? 64 * k + lane : 0;
  int f = front[0] + (cum[N + j] - cum[j]);
  cf[lane] = f;
  for (int m = 1; m < M; ++m) {
    f = max(f, front[m]) + (cum[(m + 1) * N + j] - cum[m * N + j]);
    cf[m * kWave + lane] = f;
  }
  int lb = 0;
  bool act = have;
  for (int qi = 0; qi < P; ++qi) {
    if (__ballot(act) == 0) break;
    const int pr = pair[qi];
    const int m0 = pr & 0xff, m1 = pr >> 8;
    const uint16_t* ord = johnson + static_cast<int>(pair_id[qi]) * N;
    const int* c0 = cum + m0 * N;
    const int* c1 = cum + m1 * N;
    int t0 = cf[m0 * kWave + lane], t1 = cf[m1 * kWave + lane];
    for (int r = 0; r < N; ++r) {
      // wave-uniform: the order and the set are the wave's, so the branch is scalar
      const int jj = __builtin_amdgcn_readfirstlane(static_cast<int>(ord[r]));
      if (!__builtin_amdgcn_readfirstlane(static_cast<int>((set[jj >> 6] >> (jj & 63)) & 1ull))) continue;
      const int e0 = c0[N + jj];
      const int p0 = e0 - c0[jj];
      const int b1 = c1[jj];
      const int lag = b1 - e0;
      const int p1 = c1[N + jj] - b1;
      if (jj != j) {
        t0 += p0;
        t1 = max(t1, t0 + lag) + p1;
      }
    }
    if (act) {
      lb = max(lb, max(t1 + tails[m1], t0 + tails[m0]));
      if (lb >= best) act = false;
    }
  }
  return __ballot(have && lb < best);
}

// kLb2: the model's bound is LB2; kLookOwn: the lookahead counts with the model's bound
// (always so for LB1 / LB1_d, where <false, true> is the one instance).
template <bool kLb2, bool kLookOwn>
__global__ void __launch_bounds__(kBlock) lookahead_probe_kernel(LookParams q) {
  static_assert(kLb2 || kLookOwn, "LB1's lookahead bound is its own");
  constexpr bool kLookLb2 = kLb2 && kLookOwn;
  extern __shared__ __attribute__((aligned(16))) unsigned char est_smem[];
  const EstParams& a = q.e;
  const int N = a.jobs, M = a.machines, P = a.pairs, W = a.words;
  const int power = q.power;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int waves = blockDim.x / kWave;
  const LookLds LL = look_lds_layout(N, M, P, kLb2, waves);
  const EstLds& L = LL.base;

  int* cum = reinterpret_cast<int*>(est_smem + L.cum);
  int* tails = reinterpret_cast<int*>(est_smem + L.tails);
  uint16_t* johnson = reinterpret_cast<uint16_t*>(est_smem + L.johnson);
  uint16_t* pair = reinterpret_cast<uint16_t*>(est_smem + L.pair);
  uint16_t* pair_id = reinterpret_cast<uint16_t*>(est_smem + L.pair_id);
  for (int i = threadIdx.x; i < (M + 1) * N; i += blockDim.x) cum[i] = a.cum[i];
  for (int i = threadIdx.x; i < M; i += blockDim.x) tails[i] = a.tails[i];
  if constexpr (kLb2) {
    for (int i = threadIdx.x; i < P * N; i += blockDim.x) johnson[i] = a.johnson[i];
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      pair[i] = a.pair[i];
      pair_id[i] = a.pair_id[i];
    }
  }
  unsigned char* mine = est_smem + L.wave0 + L.wave_bytes * static_cast<unsigned>(wid);
  u64* set = reinterpret_cast<u64*>(mine + L.w_set);
  u64* surv = reinterpret_cast<u64*>(mine + L.w_surv);
  double* wsum = reinterpret_cast<double*>(mine + L.w_sum);
  double* lvl = reinterpret_cast<double*>(mine + L.w_lvl);
  int* front = reinterpret_cast<int*>(mine + L.w_front);
  int* remain = reinterpret_cast<int*>(mine + L.w_remain);
  int* cf = reinterpret_cast<int*>(mine + L.w_cf);  // [M][kWave], LB2 only
  u64* pre = reinterpret_cast<u64*>(mine + LL.w_pre);  // [N] inclusive prefix sums of the weights
  u64* set2 = reinterpret_cast<u64*>(mine + LL.w_set2);
  int* kc = reinterpret_cast<int*>(mine + LL.w_kc);  // [N] surviving children of survivor c
  int* front2 = reinterpret_cast<int*>(mine + LL.w_front2);
  int* remain2 = reinterpret_cast<int*>(mine + LL.w_remain2);
  for (int i = lane; i < N; i += kWave) lvl[i] = 0.0;
  __syncthreads();
  int total = 0;  // lane m: all the work of machine m, the root's remain
  if (lane < M)
    for (int j = 0; j < N; ++j) total += cum[(lane + 1) * N + j] - cum[lane * N + j];

  double sum = 0, sum2 = 0, sumd = 0;
  const u64 gw = static_cast<u64>(blockIdx.x) * waves + wid;
  const u64 stride = static_cast<u64>(gridDim.x) * waves;
  for (u64 i = gw; i < a.count; i += stride) {
    // ---- root, as in the Knuth kernel ----
    for (int k = 0; k < W; ++k) {
      const int b = N - 64 * k;
      set[k] = b >= 64 ? ~0ull : (b <= 0 ? 0ull : ((1ull << b) - 1ull));
    }
    if (lane < M) {  // M <= kWave
      front[lane] = 0;
      remain[lane] = total;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t h = probe_hash(a.seed, a.first_probe + i);
    double w = 1.0, est = 0.0;
    int depth = 0;
    // a parent at depth N - 1 has one leaf child, and leaves are never pushed
    while (depth < N - 1) {
      // ---- 1. survivors of the node under the model's bound ----
      int ktotal = 0;
      for (int k = 0; k < W; ++k) {
        const u64 s = est_uniform(set[k]);
        u64 sv = 0;
        if (s != 0) {
          if constexpr (kLb2)
            sv = est_word_lb2(N, M, P, k, lane, s, front, set, cum, tails, johnson, pair, pair_id, cf, a.best);
          else
            sv = est_word_lb1(N, M, k, lane, s, front, remain, cum, tails, a.best);
        }
        surv[k] = sv;
        ktotal += __popcll(sv);
      }
      if (ktotal == 0) break;
      const double wk = look_mul(w, static_cast<double>(ktotal));
      est = look_add(est, wk);
      lvl[depth] = look_add(lvl[depth], wk);
      const int level = depth;  // depth of the parent: enters the draw, indexes the record
      ++depth;
      // the survivors sit at depth N - 1: their one child is a leaf, every k_c is 0
      if (depth >= N - 1) break;
      // ---- 2. k_c of every survivor, ascending; running sum of the weights ----
      u64 T = 0;
      for (int k = 0; k < W; ++k) {
        u64 todo = est_uniform(surv[k]);
        while (todo != 0) {
          const int bit = __builtin_ctzll(todo);
          todo &= todo - 1;
          const int c = 64 * k + bit;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          int f = front[0] + (cum[N + c] - cum[c]);
          front2[0] = f;
          remain2[0] = remain[0] - (cum[N + c] - cum[c]);
          for (int m = 1; m < M; ++m) {
            const int pm = cum[(m + 1) * N + c] - cum[m * N + c];
            f = max(f, front[m]) + pm;
            front2[m] = f;
            remain2[m] = remain[m] - pm;
          }
          for (int k2 = 0; k2 < W; ++k2) set2[k2] = k2 == k ? set[k2] & ~(1ull << bit) : set[k2];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          int n = 0;
          for (int k2 = 0; k2 < W; ++k2) {
            const u64 s2 = est_uniform(set2[k2]);
            if (s2 == 0) continue;
            u64 sv2;
            if constexpr (kLookLb2)
              sv2 = est_word_lb2(N, M, P, k2, lane, s2, front2, set2, cum, tails, johnson, pair, pair_id, cf, a.best);
            else
              sv2 = est_word_lb1(N, M, k2, lane, s2, front2, remain2, cum, tails, a.best);
            n += __popcll(sv2);
          }
          u64 wt = static_cast<u64>(n);
          if (power >= 2) wt *= static_cast<u64>(n);
          if (power >= 3) wt *= static_cast<u64>(n);
          T += wt;
          kc[c] = n;
          pre[c] = T;
        }
      }
      if (T == 0) break;  // no job recorded for this level
      // ---- 3. the first survivor whose inclusive prefix exceeds x ----
      const u64 x = probe_pick_weighted(probe_draw(h, static_cast<uint32_t>(level)), T);
      int word = 0;
      u64 hits = 0;
      for (int k = 0; k < W; ++k) {
        const bool have = (surv[k] >> lane) & 1ull;
        const u64 p = pre[have ? 64 * k + lane : 0];
        hits = __ballot(have && p > x);
        if (hits != 0) {
          word = k;
          break;
        }
      }
      const int bit = hits ? __builtin_ctzll(hits) : 0;  // some lane hits: x < T
      const int job = 64 * word + bit;
      if (a.rec_jobs && lane == 0) a.rec_jobs[i * static_cast<u64>(N) + level] = static_cast<int16_t>(job);
      // ---- 4. reweight; the child becomes the node ----
      const int n = kc[job];
      u64 wt = static_cast<u64>(n);
      if (power >= 2) wt *= static_cast<u64>(n);
      if (power >= 3) wt *= static_cast<u64>(n);
      w = look_div(look_mul(w, static_cast<double>(T)), static_cast<double>(wt));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      int f = front[0] + (cum[N + job] - cum[job]);
      front[0] = f;
      remain[0] -= cum[N + job] - cum[job];
      for (int m = 1; m < M; ++m) {
        const int pm = cum[(m + 1) * N + job] - cum[m * N + job];
        f = max(f, front[m]) + pm;
        front[m] = f;
        remain[m] -= pm;
      }
      set[word] = set[word] & ~(1ull << bit);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    sum = look_add(sum, est);
    sum2 = look_add(sum2, look_mul(est, est));
    sumd += depth;
    if (a.rec_est && lane == 0) {
      a.rec_est[i] = est;
      a.rec_depth[i] = depth;
    }
  }
  wsum[0] = sum;
  wsum[1] = sum2;
  wsum[2] = sumd;
  __syncthreads();
  // the workgroup's partial sums: its waves in wave order
  for (int t = threadIdx.x; t < 3 + N; t += blockDim.x) {
    double x = 0;
    for (int v = 0; v < waves; ++v) {
      const unsigned char* ws = est_smem + L.wave0 + L.wave_bytes * static_cast<unsigned>(v);
      x += t < 3 ? reinterpret_cast<const double*>(ws + L.w_sum)[t] : reinterpret_cast<const double*>(ws + L.w_lvl)[t - 3];
    }
    a.partial[static_cast<u64>(blockIdx.x) * (3 + N) + t] = x;
  }
}

}  // namespace dev
}  // namespace tts
