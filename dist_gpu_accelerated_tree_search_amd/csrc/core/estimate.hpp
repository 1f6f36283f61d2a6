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

}  // namespace tts
