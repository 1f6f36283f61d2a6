// PFSP search node, shared bit-for-bit by the host pools and the device pools.
//
// Reference node (pfsp/lib/PFSP_node.h:15-20) is {int16 depth, int16 limit1,
// int16 prmu[MAX_JOBS=20]} = 44 B with a compile-time MAX_JOBS. Here:
//   * forward branching only, so limit1 == depth-1 is implicit (not stored);
//   * job ids are uint8 up to 255 jobs, uint16 for the 500-job class;
//   * the node is 16-byte aligned: 32 B for 20 jobs (one pair of dwordx4 per lane
//     on the GPU), 64 B for 50, 112 B for 100, 208 B for 200, 1008 B for 500;
//   * the job-count bucket NJ is a template parameter chosen at run time
//     (no MAX_JOBS edit + recompile as in ref pfsp/README.md:52).
// prmu[0..depth) is the scheduled prefix in order; prmu[depth..jobs) holds the
// unscheduled jobs in arbitrary order (only the set matters to every bound).
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

#ifndef TTS_HD
#if defined(__HIPCC__)
#define TTS_HD __host__ __device__
#else
#define TTS_HD
#endif
#endif

namespace tts {

template <int NJ>
struct alignas(16) PfspNode {
  static constexpr int kMaxJobs = NJ;
  using id_t = std::conditional_t<(NJ > 255), uint16_t, uint8_t>;
  id_t depth;
  id_t prmu[NJ];
};

static_assert(sizeof(PfspNode<20>) == 32, "20-job node must be 32 B");
static_assert(sizeof(PfspNode<50>) == 64, "50-job node must be 64 B");

template <int NJ>
TTS_HD inline void pfsp_init_root(PfspNode<NJ>& root, int jobs) {
  root.depth = 0;
  for (int i = 0; i < NJ; ++i) root.prmu[i] = static_cast<typename PfspNode<NJ>::id_t>(i < jobs ? i : 0);
}

// Child obtained by moving prmu[k] (k >= depth) to position depth.
template <int NJ>
TTS_HD inline PfspNode<NJ> pfsp_child(const PfspNode<NJ>& parent, int k) {
  PfspNode<NJ> c = parent;
  const int d = parent.depth;
  const auto t = c.prmu[d];
  c.prmu[d] = c.prmu[k];
  c.prmu[k] = t;
  c.depth = static_cast<typename PfspNode<NJ>::id_t>(d + 1);
  return c;
}

// Job set wider than a machine word (front nodes above 64 jobs): W 64-bit words, low word
// first, bit j of the set in bit j % 64 of word j / 64. A plain value type with the
// handful of operations below — the hot loops never see a 128-bit integer, and never a
// shift of the whole set by a variable amount: the kernels walk a set one 64-bit word at
// a time (dev::mask_words).
template <int W>
struct JobSet {
  uint64_t w[W];
};

// The set operations of the front layout, alike for the 32-bit, the 64-bit and the
// multi-word sets: test / set / clear bit j, clear the lowest set bit, lowest set bit
// (mask_ctz, of a non-empty set), popcount, popcount below bit j, the first n bits,
// and-not, is-empty.
TTS_HD inline bool mask_test(uint32_t x, int j) { return (x >> j) & 1u; }
TTS_HD inline bool mask_test(uint64_t x, int j) { return (x >> j) & 1u; }
TTS_HD inline void mask_set(uint32_t& x, int j) { x |= uint32_t(1) << j; }
TTS_HD inline void mask_set(uint64_t& x, int j) { x |= uint64_t(1) << j; }
TTS_HD inline void mask_clear(uint32_t& x, int j) { x &= ~(uint32_t(1) << j); }
TTS_HD inline void mask_clear(uint64_t& x, int j) { x &= ~(uint64_t(1) << j); }
TTS_HD inline void mask_pop_low(uint32_t& x) { x &= x - 1; }
TTS_HD inline void mask_pop_low(uint64_t& x) { x &= x - 1; }
TTS_HD inline int mask_ctz(uint32_t x) { return __builtin_ctz(x); }
TTS_HD inline int mask_ctz(uint64_t x) { return __builtin_ctzll(x); }
TTS_HD inline int mask_count(uint32_t x) { return __builtin_popcount(x); }
TTS_HD inline int mask_count(uint64_t x) { return __builtin_popcountll(x); }
TTS_HD inline int mask_count_below(uint32_t x, int j) { return __builtin_popcount(x & ((uint32_t(1) << j) - 1u)); }
TTS_HD inline int mask_count_below(uint64_t x, int j) { return __builtin_popcountll(x & ((uint64_t(1) << j) - 1u)); }
TTS_HD inline uint32_t mask_andnot(uint32_t a, uint32_t b) { return a & ~b; }
TTS_HD inline uint64_t mask_andnot(uint64_t a, uint64_t b) { return a & ~b; }
TTS_HD inline bool mask_empty(uint32_t x) { return x == 0; }
TTS_HD inline bool mask_empty(uint64_t x) { return x == 0; }

// (the word-wise forms: a bit index picks its word by comparison, never by a variable
// index into w[], so a set held in registers stays there)
template <int W>
TTS_HD inline bool mask_test(const JobSet<W>& x, int j) {
  uint64_t v = 0;
  for (int k = 0; k < W; ++k) v = (j >> 6) == k ? x.w[k] : v;
  return (v >> (j & 63)) & 1u;
}
template <int W>
TTS_HD inline void mask_set(JobSet<W>& x, int j) {
  const uint64_t b = uint64_t(1) << (j & 63);
  for (int k = 0; k < W; ++k) x.w[k] |= (j >> 6) == k ? b : uint64_t(0);
}
template <int W>
TTS_HD inline void mask_clear(JobSet<W>& x, int j) {
  const uint64_t b = uint64_t(1) << (j & 63);
  for (int k = 0; k < W; ++k) x.w[k] &= ~((j >> 6) == k ? b : uint64_t(0));
}
template <int W>
TTS_HD inline void mask_pop_low(JobSet<W>& x) {
  bool done = false;
  for (int k = 0; k < W; ++k) {
    const bool here = !done && x.w[k] != 0;
    x.w[k] = here ? (x.w[k] & (x.w[k] - 1)) : x.w[k];
    done = done || here;
  }
}
template <int W>
TTS_HD inline int mask_ctz(const JobSet<W>& x) {
  for (int k = 0; k < W - 1; ++k)
    if (x.w[k]) return 64 * k + __builtin_ctzll(x.w[k]);
  return 64 * (W - 1) + __builtin_ctzll(x.w[W - 1]);
}
template <int W>
TTS_HD inline int mask_count(const JobSet<W>& x) {
  int c = 0;
  for (int k = 0; k < W; ++k) c += __builtin_popcountll(x.w[k]);
  return c;
}
template <int W>
TTS_HD inline int mask_count_below(const JobSet<W>& x, int j) {
  const uint64_t low = (uint64_t(1) << (j & 63)) - 1u;
  int c = 0;
  for (int k = 0; k < W; ++k) {
    const uint64_t m = k < (j >> 6) ? ~uint64_t(0) : (k == (j >> 6) ? low : uint64_t(0));
    c += __builtin_popcountll(x.w[k] & m);
  }
  return c;
}
template <int W>
TTS_HD inline JobSet<W> mask_andnot(const JobSet<W>& a, const JobSet<W>& b) {
  JobSet<W> r;
  for (int k = 0; k < W; ++k) r.w[k] = a.w[k] & ~b.w[k];
  return r;
}
template <int W>
TTS_HD inline bool mask_empty(const JobSet<W>& x) {
  uint64_t v = 0;
  for (int k = 0; k < W; ++k) v |= x.w[k];
  return v == 0;
}

// The first n bits (0 <= n <= bits of the set): the job set of an n-job root; with
// n = the set's width, every bit.
template <class Mask>
struct MaskFirst {
  TTS_HD static Mask get(int n) { return n >= static_cast<int>(8 * sizeof(Mask)) ? ~Mask(0) : ((Mask(1) << n) - Mask(1)); }
};
template <int W>
struct MaskFirst<JobSet<W>> {
  TTS_HD static JobSet<W> get(int n) {
    JobSet<W> r;
    for (int k = 0; k < W; ++k) {
      const int b = n - 64 * k;
      r.w[k] = b >= 64 ? ~uint64_t(0) : (b <= 0 ? uint64_t(0) : ((uint64_t(1) << b) - 1u));
    }
    return r;
  }
};
template <class Mask>
TTS_HD inline Mask mask_first(int n) {
  return MaskFirst<Mask>::get(n);
}

// Front-carrying node of the LB1 / LB1_d search (machine bucket MB in {5, 10, 20}). LB1
// only depends on the scheduled prefix through
// its per-machine completion times (front) and on the set of unscheduled jobs, so the
// node stores exactly that: a child costs O(M) from its parent instead of replaying
// the O(depth * M) prefix chain (ref schedule_front, c_bound_simple.c:52-69, which
// the reference repeats per child for LB1 and per parent for LB1_d). 32 B for up to
// 10 machines, 48 B for 20 (the permutation node is 32 B at 20 jobs).
//   depth       jobs scheduled
//   rest        bit j set: job j is not scheduled yet
//   front[m]    completion time of the prefix on machine m; at the root the minimum
//               heads (ref schedule_front with limit1 == -1)
// NJ (job bucket of the front layout): 20 keeps the unscheduled set in 32 bits, 50 in
// 64 (the set then starts at byte 8 and the fronts at byte 16), 100 in a JobSet of two
// 64-bit words (the set at byte 16, the fronts at byte 32: 48 / 64 / 80 B for 5 / 10 / 20
// machines, where the permutation node is 112 B). One pattern for these three: depth in
// byte 0, padding to sizeof(Mask), the set, the u16 fronts.
// 200 and 500 (TTS_FRONT_WIDE=2) keep the set in a JobSet of four / eight words. Padding
// the header to sizeof(Mask) would waste 31 / 63 bytes there, so these two have a 16-byte
// header: the depth as a u16 in bytes 0-1 (it reaches 499), the rest zero; the set at byte
// 16, low word first; the u16 fronts at byte 16 + 8 W:
//   200 jobs   64 /  80 /  96 B for 5 / 10 / 20 machines (permutation node  208 B)
//   500 jobs   96 / 112 / 128 B                          (permutation node 1008 B)
template <int NJ>
using PfspJobMask =
    std::conditional_t<(NJ <= 32), uint32_t, std::conditional_t<(NJ <= 64), uint64_t, JobSet<(NJ + 63) / 64>>>;

template <int MB, int NJ = 20>
struct alignas(16) PfspFrontNode {
  static constexpr int kMachines = MB;
  static constexpr int kJobs = NJ;
  using Mask = PfspJobMask<NJ>;
  using depth_t = std::conditional_t<(NJ > 100), uint16_t, uint8_t>;
  static constexpr int kHeader = NJ > 100 ? 16 : static_cast<int>(sizeof(Mask));  // bytes before the set
  depth_t depth;
  uint8_t pad[kHeader - sizeof(depth_t)];
  Mask rest;
  uint16_t front[MB];
};
static_assert(sizeof(PfspFrontNode<5>) == 32 && sizeof(PfspFrontNode<10>) == 32 && sizeof(PfspFrontNode<20>) == 48,
              "front node sizes");
static_assert(sizeof(PfspFrontNode<5, 50>) == 32 && sizeof(PfspFrontNode<10, 50>) == 48 &&
                  sizeof(PfspFrontNode<20, 50>) == 64,
              "50-job front node sizes");
static_assert(sizeof(JobSet<2>) == 16 && sizeof(PfspFrontNode<5, 100>) == 48 && sizeof(PfspFrontNode<10, 100>) == 64 &&
                  sizeof(PfspFrontNode<20, 100>) == 80,
              "100-job front node sizes");
using PfspFrontNodeWidest = PfspFrontNode<20, 100>;
static_assert(__builtin_offsetof(PfspFrontNodeWidest, rest) == 16 && __builtin_offsetof(PfspFrontNodeWidest, front) == 32,
              "100-job front node: the set at byte 16, the fronts at byte 32");
static_assert(sizeof(JobSet<4>) == 32 && sizeof(PfspFrontNode<5, 200>) == 64 && sizeof(PfspFrontNode<10, 200>) == 80 &&
                  sizeof(PfspFrontNode<20, 200>) == 96,
              "200-job front node sizes");
static_assert(sizeof(JobSet<8>) == 64 && sizeof(PfspFrontNode<5, 500>) == 96 && sizeof(PfspFrontNode<10, 500>) == 112 &&
                  sizeof(PfspFrontNode<20, 500>) == 128,
              "500-job front node sizes");
using PfspFrontNode200 = PfspFrontNode<20, 200>;
using PfspFrontNode500 = PfspFrontNode<20, 500>;
static_assert(sizeof(PfspFrontNode200::depth_t) == 2 && __builtin_offsetof(PfspFrontNode200, depth) == 0 &&
                  __builtin_offsetof(PfspFrontNode200, rest) == 16 && __builtin_offsetof(PfspFrontNode200, front) == 48,
              "200-job front node: u16 depth, the set at byte 16, the fronts at byte 48");
static_assert(sizeof(PfspFrontNode500::depth_t) == 2 && __builtin_offsetof(PfspFrontNode500, depth) == 0 &&
                  __builtin_offsetof(PfspFrontNode500, rest) == 16 && __builtin_offsetof(PfspFrontNode500, front) == 80,
              "500-job front node: u16 depth, the set at byte 16, the fronts at byte 80");

// Remain table of the 20-job front bucket (core/pfsp_front.hpp pfsp_front_remain_table): the
// job set cut into kRemainGroups groups of kRemainBits bits, one table row per group pattern.
// (Groups of 4 bits: 80 rows. Groups of 5 would save one row read per look-up with 128 rows,
// 2,560 B for 10 machines, and that ends the sixth resident workgroup of the 10-machine front
// kernel: 6 x 27,392 B against a CU's 163,840 B of LDS.)
constexpr int kRemainBits = 4, kRemainGroups = 5, kRemainPats = 1 << kRemainBits;
static_assert(kRemainBits * kRemainGroups == 20, "the groups cover a 20-job set");

// Job-count buckets a run-time instance is dispatched to.
inline int pfsp_bucket(int jobs) {
  if (jobs <= 20) return 20;
  if (jobs <= 50) return 50;
  if (jobs <= 100) return 100;
  if (jobs <= 200) return 200;
  return 500;
}

// Calls f(std::integral_constant<int, NJ>{}) for the bucket of `jobs`.
template <class F>
decltype(auto) with_pfsp_bucket(int jobs, F&& f) {
  switch (pfsp_bucket(jobs)) {
    case 20: return f(std::integral_constant<int, 20>{});
    case 50: return f(std::integral_constant<int, 50>{});
    case 100: return f(std::integral_constant<int, 100>{});
    case 200: return f(std::integral_constant<int, 200>{});
    default: return f(std::integral_constant<int, 500>{});
  }
}

// N-Queens node (ref nqueens/lib/NQueens_node.h:13-17 stores the full board,
// 21 B). The tree only depends on which rows are used and which diagonals are
// attacked, so the node is three 32-bit masks + depth = 16 B.
struct alignas(16) QueensNode {
  uint32_t cols;   // rows already holding a queen (bit r)
  uint32_t diag;   // attacked "r - c" diagonal, shifted so the next column reads bit r
  uint32_t anti;   // attacked "r + c" diagonal, same convention
  uint32_t depth;  // number of queens placed (== column to fill next)
};
static_assert(sizeof(QueensNode) == 16, "queens node must be 16 B");

}  // namespace tts
