// Tree-size estimation for long solves (ta056 LB2 and the like): Knuth's random-probe
// estimator on the host (D. E. Knuth, "Estimating the efficiency of backtrack
// programs", Math. Comp. 1975). A probe walks from the root, at every node expands
// all children with the problem's own decompose (same bound, same incumbent, same
// counting rules as the search), multiplies a weight by the number of pushed
// children and follows one of them uniformly at random. The sum of the weights is
// an unbiased estimate of the explored tree (the reference's "tree" count) for a
// fixed incumbent, i.e. for -u 1 runs. The reference has no estimator; this is what
// projects a time-to-solution from a measured nodes/s rate.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <random>
#include <stdexcept>
#include <thread>
#include <vector>

#include "probe_rng.hpp"
#include "problems.hpp"

namespace tts {

struct TreeEstimate {
  double tree = 0;        // mean estimate of the explored tree
  double stderr_ = 0;     // standard error of the mean
  double depth = 0;       // mean probe depth
  unsigned long long probes = 0;
  std::vector<double> per_level;  // mean estimated nodes per tree level
};

template <class Problem>
TreeEstimate knuth_estimate(const Problem& prob, int best, unsigned long long probes, unsigned long long seed,
                            int threads = 1) {
  using Node = typename Problem::Node;
  threads = std::max(1, threads);
  struct Acc {
    double s = 0, s2 = 0, depth = 0;
    std::vector<double> lvl;
  };
  std::vector<Acc> acc(threads);
  auto worker = [&](int t) {
    std::mt19937_64 rng(seed * 0x9e3779b97f4a7c15ull + static_cast<unsigned long long>(t));
    Acc& a = acc[t];
    std::vector<Node> kids;
    for (unsigned long long p = static_cast<unsigned long long>(t); p < probes; p += static_cast<unsigned long long>(threads)) {
      Node x = prob.root();
      double w = 1, est = 0;
      int lvl = 0;
      for (;;) {
        kids.clear();
        int b = best;
        u64 tree = 0, sol = 0;
        prob.decompose(x, b, tree, sol, [&](const Node& c) { kids.push_back(c); });
        if (kids.empty()) break;
        w *= static_cast<double>(kids.size());
        est += w;
        if (static_cast<int>(a.lvl.size()) <= lvl) a.lvl.resize(lvl + 1, 0.0);
        a.lvl[lvl] += w;
        ++lvl;
        x = kids[std::uniform_int_distribution<size_t>(0, kids.size() - 1)(rng)];
      }
      a.s += est;
      a.s2 += est * est;
      a.depth += lvl;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(worker, t);
  worker(0);
  for (auto& x : th) x.join();
  TreeEstimate r;
  r.probes = probes;
  double s = 0, s2 = 0, dep = 0;
  for (auto& a : acc) {
    s += a.s;
    s2 += a.s2;
    dep += a.depth;
    if (a.lvl.size() > r.per_level.size()) r.per_level.resize(a.lvl.size(), 0.0);
    for (size_t i = 0; i < a.lvl.size(); ++i) r.per_level[i] += a.lvl[i];
  }
  const double n = static_cast<double>(std::max<unsigned long long>(1, probes));
  r.tree = s / n;
  const double var = std::max(0.0, s2 / n - r.tree * r.tree);
  r.stderr_ = std::sqrt(var / n);
  r.depth = dep / n;
  for (auto& v : r.per_level) v /= n;
  return r;
}

// Mean, standard error and per-level means from the sums over `probes` probes; the
// per-level vector is cut after its last non-zero level.
inline TreeEstimate finish_estimate(double s, double s2, double depth, std::vector<double> lvl,
                                    unsigned long long probes) {
  TreeEstimate r;
  r.probes = probes;
  const double n = static_cast<double>(std::max<unsigned long long>(1, probes));
  r.tree = s / n;
  const double var = std::max(0.0, s2 / n - r.tree * r.tree);
  r.stderr_ = std::sqrt(var / n);
  r.depth = depth / n;
  while (!lvl.empty() && lvl.back() == 0.0) lvl.pop_back();
  for (auto& v : lvl) v /= n;
  r.per_level = std::move(lvl);
  return r;
}

// ---- Indexed probes: the host twin of the device estimator (hip/estimate_kernels.hpp) ----
// The rules are knuth_estimate's (decompose with a fixed `best`, the weight times the
// number of pushed children, est += w per level). Two things differ, so that a device
// probe can be checked against a host probe one by one:
//   * the survivors are ordered by the job they append, ascending (the prmu order of a
//     permutation node depends on its swap history; a device node has no such order);
//   * probe i chooses its child at every level with probe_rng.hpp from (seed, i, level).
// Probe i is therefore the same walk whichever thread, chunk or call runs it.

// Per-probe records (tests only): est, depth and the jobs chosen, -1 past the depth.
struct ProbeRecords {
  static constexpr unsigned long long kMaxProbes = 1ull << 20;
  static constexpr unsigned long long kMaxCells = 1ull << 26;  // probes x jobs: 128 MB of chosen jobs
  int jobs = 0;
  std::vector<double> est;
  std::vector<int> depth;
  std::vector<int16_t> chosen;  // [probes][jobs]
  void reset(unsigned long long probes, int jobs_) {
    if (probes > kMaxProbes || probes * static_cast<unsigned long long>(jobs_) > kMaxCells)
      throw std::invalid_argument("probe records are kept for at most 2^20 probes and 2^26 probes x jobs");
    jobs = jobs_;
    est.assign(probes, 0.0);
    depth.assign(probes, 0);
    chosen.assign(static_cast<size_t>(probes) * jobs_, static_cast<int16_t>(-1));
  }
};

// Probes of one partial sum: a chunk is reduced in probe order and the chunks in chunk
// order, whatever thread ran them, so the aggregates do not depend on `threads`.
constexpr unsigned long long kEstimateChunk = 1024;

template <int NJ>
TreeEstimate knuth_estimate_indexed(const PfspProblem<NJ>& prob, int best, unsigned long long first_probe,
                                    unsigned long long probes, unsigned long long seed, int threads = 1,
                                    ProbeRecords* records = nullptr) {
  using Node = typename PfspProblem<NJ>::Node;
  const int N = prob.inst->jobs;
  threads = std::max(1, threads);
  if (records) records->reset(probes, N);
  struct Part {
    double s = 0, s2 = 0, depth = 0;
    std::vector<double> lvl;
  };
  const unsigned long long nchunks = (probes + kEstimateChunk - 1) / kEstimateChunk;
  std::vector<Part> part(nchunks);
  std::atomic<unsigned long long> next{0};
  auto worker = [&]() {
    std::vector<Node> kids;
    std::vector<std::pair<int, int>> by_job;  // (appended job, index in kids)
    for (;;) {
      const unsigned long long c = next.fetch_add(1);
      if (c >= nchunks) break;
      Part& a = part[c];
      const unsigned long long lo = c * kEstimateChunk, hi = std::min(probes, lo + kEstimateChunk);
      for (unsigned long long i = lo; i < hi; ++i) {
        const uint64_t h = probe_hash(seed, first_probe + i);
        Node x = prob.root();
        double w = 1, est = 0;
        int lvl = 0;
        for (;;) {
          kids.clear();
          int b = best;
          u64 tree = 0, sol = 0;
          prob.decompose(x, b, tree, sol, [&](const Node& k) { kids.push_back(k); });
          if (kids.empty()) break;
          const int d = x.depth;
          by_job.clear();
          for (size_t k = 0; k < kids.size(); ++k) by_job.emplace_back(static_cast<int>(kids[k].prmu[d]), static_cast<int>(k));
          std::sort(by_job.begin(), by_job.end());
          w = w * static_cast<double>(kids.size());
          est = est + w;
          if (static_cast<int>(a.lvl.size()) <= lvl) a.lvl.resize(static_cast<size_t>(lvl) + 1, 0.0);  // levels reached only
          a.lvl[lvl] += w;
          const auto& pick = by_job[probe_pick(probe_draw(h, static_cast<uint32_t>(lvl)), static_cast<uint32_t>(kids.size()))];
          if (records) records->chosen[static_cast<size_t>(i) * N + lvl] = static_cast<int16_t>(pick.first);
          x = kids[pick.second];
          ++lvl;
        }
        a.s += est;
        a.s2 += est * est;
        a.depth += lvl;
        if (records) {
          records->est[i] = est;
          records->depth[i] = lvl;
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(worker);
  worker();
  for (auto& x : th) x.join();
  double s = 0, s2 = 0, dep = 0;
  std::vector<double> lvl(static_cast<size_t>(N), 0.0);
  for (const Part& a : part) {
    s += a.s;
    s2 += a.s2;
    dep += a.depth;
    for (size_t i = 0; i < a.lvl.size(); ++i) lvl[i] += a.lvl[i];
  }
  return finish_estimate(s, s2, dep, std::move(lvl), probes);
}

// ---- Importance-weighted probes: one level of lookahead ----
// Knuth's refinement of his own estimator: a probe no longer follows a survivor uniformly
// but with probability proportional to wt_c = k_c^power, k_c being the number of c's own
// surviving children, and divides its weight by that probability. Survivors without
// children (dead ends one level down) are never followed, so the probes reach the deep
// levels where the tree's mass is. A probe, from w = 1, est = 0 at the root:
//   1. k = survivors of the node (decompose, as above); none: stop;
//   2. est += w * k, lvl[depth] += w * k, ++depth        (multiply, then add: two roundings)
//   3. k_c for every survivor c in ascending job order, under the lookahead bound
//   4. T = sum of wt_c (u64); 0: stop, no job recorded for this level
//   5. x = probe_pick_weighted(probe_draw(h, level), T); the pick is the first survivor
//      whose inclusive prefix sum of wt exceeds x
//   6. w = (w * T) / wt_pick                              (two roundings)
// E[est] is the explored tree for any lookahead bound that is at most the problem's own: a
// survivor of weight 0 then has no surviving child to count. look = kLookBoundOwn counts with
// the problem's bound; kLookBoundLb1 with LB1 on the same instance (a relaxation of LB2, the
// same thing for LB1 and LB1_d). `depth` counts the levels that added to est, so a record
// holds depth or depth - 1 jobs.
constexpr int kLookBoundOwn = 0, kLookBoundLb1 = 1;
constexpr int kLookaheadMaxPower = 3;

// How to probe (host twin and device alike): Knuth's uniform choice, or lookahead.
struct EstimateMethod {
  bool lookahead = false;
  int power = 2;             // lookahead only
  int look = kLookBoundOwn;  // lookahead only
};

inline uint64_t lookahead_weight(uint64_t kc, int power) {
  uint64_t wt = kc;
  for (int e = 1; e < power; ++e) wt *= kc;
  return wt;
}

template <int NJ>
TreeEstimate lookahead_estimate_indexed(const PfspProblem<NJ>& prob, int best, unsigned long long first_probe,
                                        unsigned long long probes, unsigned long long seed, int power, int look,
                                        int threads = 1, ProbeRecords* records = nullptr) {
  using Node = typename PfspProblem<NJ>::Node;
  if (power < 1 || power > kLookaheadMaxPower) throw std::invalid_argument("lookahead power must be 1, 2 or 3");
  if (look != kLookBoundOwn && look != kLookBoundLb1) throw std::invalid_argument("lookahead bound must be own or lb1");
  // LB1 counts through LB1_d's O(M) chain from the parent's front: the same values (the
  // device kernel evaluates both that way), without LB1's O(N M) pass per child
  const PfspProblem<NJ> ahead(*prob.inst, (look == kLookBoundLb1 || prob.lb != 2) ? 0 : 2);
  const int N = prob.inst->jobs;
  threads = std::max(1, threads);
  if (records) records->reset(probes, N);
  struct Part {
    double s = 0, s2 = 0, depth = 0;
    std::vector<double> lvl;
  };
  const unsigned long long nchunks = (probes + kEstimateChunk - 1) / kEstimateChunk;
  std::vector<Part> part(nchunks);
  std::atomic<unsigned long long> next{0};
  auto worker = [&]() {
    std::vector<Node> kids;
    std::vector<std::pair<int, int>> by_job;  // (appended job, index in kids)
    std::vector<uint64_t> wt;                 // by survivor, ascending job
    for (;;) {
      const unsigned long long c = next.fetch_add(1);
      if (c >= nchunks) break;
      Part& a = part[c];
      const unsigned long long lo = c * kEstimateChunk, hi = std::min(probes, lo + kEstimateChunk);
      for (unsigned long long i = lo; i < hi; ++i) {
        const uint64_t h = probe_hash(seed, first_probe + i);
        Node x = prob.root();
        double w = 1, est = 0;
        int lvl = 0;
        for (;;) {
          kids.clear();
          int b = best;
          u64 tree = 0, sol = 0;
          prob.decompose(x, b, tree, sol, [&](const Node& k) { kids.push_back(k); });
          if (kids.empty()) break;
          const int d = x.depth;
          by_job.clear();
          for (size_t k = 0; k < kids.size(); ++k) by_job.emplace_back(static_cast<int>(kids[k].prmu[d]), static_cast<int>(k));
          std::sort(by_job.begin(), by_job.end());
          const double wk = w * static_cast<double>(kids.size());
          est = est + wk;
          if (static_cast<int>(a.lvl.size()) <= lvl) a.lvl.resize(static_cast<size_t>(lvl) + 1, 0.0);  // levels reached only
          a.lvl[lvl] += wk;
          ++lvl;
          // a survivor at depth N - 1 has one leaf child, never pushed: decompose counts 0
          wt.clear();
          uint64_t total = 0;
          for (const auto& jk : by_job) {
            int bb = best;
            u64 kc = 0, so = 0;
            ahead.decompose(kids[jk.second], bb, kc, so, [](const Node&) {});
            wt.push_back(lookahead_weight(kc, power));
            total += wt.back();
          }
          if (total == 0) break;
          const uint64_t at = probe_pick_weighted(probe_draw(h, static_cast<uint32_t>(d)), total);
          size_t pick = 0;
          uint64_t prefix = wt[0];
          while (prefix <= at) prefix += wt[++pick];
          if (records) records->chosen[static_cast<size_t>(i) * N + d] = static_cast<int16_t>(by_job[pick].first);
          const double wT = w * static_cast<double>(total);
          w = wT / static_cast<double>(wt[pick]);
          x = kids[by_job[pick].second];
        }
        a.s += est;
        a.s2 += est * est;
        a.depth += lvl;
        if (records) {
          records->est[i] = est;
          records->depth[i] = lvl;
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(worker);
  worker();
  for (auto& x : th) x.join();
  double s = 0, s2 = 0, dep = 0;
  std::vector<double> lvl(static_cast<size_t>(N), 0.0);
  for (const Part& a : part) {
    s += a.s;
    s2 += a.s2;
    dep += a.depth;
    for (size_t i = 0; i < a.lvl.size(); ++i) lvl[i] += a.lvl[i];
  }
  return finish_estimate(s, s2, dep, std::move(lvl), probes);
}

}  // namespace tts
