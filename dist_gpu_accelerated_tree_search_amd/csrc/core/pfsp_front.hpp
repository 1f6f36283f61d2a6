// LB1 / LB1_d search on front-carrying nodes (core/pfsp_node.hpp PfspFrontNode):
// padded bound tables, the host problem (Step 1, Step 3, CPU workers, CPU drivers,
// oracle of the GPU kernel) and the layout dispatch every engine and driver uses.
//
// Parity: same bounds, same tree and solution counts as ref decompose_lb1 /
// decompose_lb1_d (PFSP_lib.c:7-90, c_bound_simple.c:127-244): the child appending
// job j gets
//     lb = max_m ( start_m + remain_m + tail_m ),   start_m = max(front'_{m-1}, front_m)
// where remain is the parent's unscheduled work (job j included) and tail the minimum
// tails — ref add_front_and_bound (c_bound_simple.c:219-244), i.e. LB1 == LB1_d
// (SURVEY §2.4). Only the node representation differs: the prefix's completion
// times are carried instead of recomputed from the permutation.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include "pfsp_instance.hpp"
#include "pfsp_node.hpp"
#include "problems.hpp"

namespace tts {

// Machine-count bucket of the front layout / GPU kernels: 5, 10 or 20; smaller counts
// run with zero-time padding machines (their terms never exceed a real machine's).
inline int pfsp_machine_bucket(int machines) {
  if (machines >= 1 && machines <= 5) return 5;
  if (machines > 5 && machines <= 10) return 10;
  if (machines > 10 && machines <= 20) return 20;
  return 0;
}

// Per-machine tables padded to MB machines (the layout the GPU kernels use too):
// a padding machine has zero processing times, no tail, and the whole real route of
// the cheapest job as its head, so every bound and every real front is unchanged.
struct PfspPadded {
  int heads[20], tails[20], sum_all[20];
};
inline PfspPadded pfsp_padded_tables(const PfspInstance& in, int MB) {
  if (in.machines > MB || MB > 20) throw std::invalid_argument("machine count exceeds the bucket");
  PfspPadded t{};
  int route = INT_MAX;
  for (int j = 0; j < in.jobs; ++j) {
    int s = 0;
    for (int k = 0; k < in.machines; ++k) s += in.pt(k, j);
    route = std::min(route, s);
  }
  for (int m = 0; m < MB; ++m) {
    const bool real = m < in.machines;
    t.heads[m] = real ? in.min_heads[m] : route;
    t.tails[m] = real ? in.min_tails[m] : 0;
    long s = 0;
    if (real)
      for (int j = 0; j < in.jobs; ++j) s += in.pt(m, j);
    t.sum_all[m] = static_cast<int>(s);
  }
  return t;
}

// Every prefix completion time of the instance fits 16 bits: the condition of the
// permutation-node kernels that pack a front into a u16 (the `front | remain << 16` LDS
// words of the LB2 kernels and their u16 child fronts, csrc/hip/pfsp_kernels.hpp).
// A completion time is the length of a monotone staircase path through the machine x job
// grid, not a column sum: it visits at most jobs + machines - 1 cells, so
// (jobs + machines - 1) * max p bounds it, and so does the sum of all processing times.
// Sufficient, not necessary (the longest path over all job orders is not computed).
inline bool pfsp_fronts_fit_u16(const PfspInstance& in) {
  long pmax = 0, tot = 0;
  for (int v : in.p) {
    pmax = std::max<long>(pmax, v);
    tot += v;
  }
  return std::min((in.jobs + in.machines - 1) * pmax, tot) < 65536;
}

// TTS_FRONT_WIDE=1 (CLI --front-wide): front nodes for 51-100 jobs too. Opt-in: without
// it those instances keep their permutation nodes. Read wherever TTS_FRONT is, so the
// CPU module, the HIP module and every spawned rank agree.
// TTS_FRONT_WIDE=2 (CLI --front-all): front nodes for 51-500 jobs, so it includes what 1
// does; 1 keeps meaning exactly 51-100.
inline int pfsp_front_wide_level() {
  const char* e = std::getenv("TTS_FRONT_WIDE");
  if (e == nullptr) return 0;
  return e[0] == '1' ? 1 : e[0] == '2' ? 2 : 0;
}

// The front layout applies: LB1 / LB1_d, at most 20 machines, and
//   * up to 50 jobs (job sets of 32 bits up to 20 jobs, 64 bits up to 50): the sum of all
//     processing times fits 16 bits, so every front does;
//   * 51 to 100 jobs (128-bit job sets), only with TTS_FRONT_WIDE=1: the staircase rule
//     pfsp_fronts_fit_u16, (jobs + machines - 1) * max p < 65536 (or the sum of all
//     processing times, if smaller). The sum alone would exclude every 100 x 20 instance
//     (ta081: sum 98,766, staircase 11,781). The staircase rule covers every 16-bit
//     quantity of the front kernel, each being at most (jobs + machines - 1) * max p:
//       - a front and a child's chain value are completion times: staircase paths of at
//         most jobs + machines - 1 cells (the root's minimum heads cover fewer);
//       - a remain is at most a machine's column sum (<= jobs cells), and remain + tail
//         adds at most machines - 1 - m cells of one job;
//       - a bound start_m + remain_m + tail_m covers at most (depth + m) + (jobs - depth) +
//         (machines - 1 - m) = jobs + machines - 1 cells.
//   * 101 to 500 jobs (256- and 512-bit job sets), only with TTS_FRONT_WIDE=2: the same
//     staircase rule, and the same argument cell for cell (none of its three counts depends
//     on the job range). With p <= 99: 200 x 20 gives 219 * 99 = 21,681 and 500 x 20 gives
//     519 * 99 = 51,381, so all of ta091-ta120 are accepted; a machine's column sum is at
//     most 500 * 99 = 49,500.
// TTS_FRONT=0 turns every front layout off (permutation nodes everywhere: A/B runs); the
// CPU and the HIP module read the variables alike, so every engine of a process agrees.
inline bool pfsp_front_ok(const PfspInstance& in, int lb) {
  if (lb != 0 && lb != 1) return false;
  if (const char* e = std::getenv("TTS_FRONT"))
    if (e[0] == '0') return false;
  if (in.jobs > 50)
    return in.jobs <= 500 && in.machines <= 20 && pfsp_machine_bucket(in.machines) != 0 &&
           pfsp_front_wide_level() >= (in.jobs <= 100 ? 1 : 2) && pfsp_fronts_fit_u16(in);
  if (in.jobs > 50 || in.machines > 20 || pfsp_machine_bucket(in.machines) == 0) return false;
  long tot = 0;
  for (int v : in.p) tot += v;
  return tot < 65536;
}

// job bucket of the front layout: 20 (32-bit job sets), 50 (64-bit), 100 (128-bit), 200
// (256-bit) or 500 (512-bit)
inline int pfsp_front_jobs(int jobs) { return jobs <= 20 ? 20 : jobs <= 50 ? 50 : jobs <= 100 ? 100 : jobs <= 200 ? 200 : 500; }

// Remain table of a 20-job front instance: the remain of a node (the sum of its unscheduled
// jobs' p rows, per machine) depends on its job set and the instance only, so the 20-bit set
// is cut into kRemainGroups groups of kRemainBits bits and the remain is the sum of one row
// per group. Row [g][pat] holds, as packed u16 pairs (machine 2h in the low half of word h,
// 2h + 1 in the high half, as a node's fronts), the p rows of the jobs kRemainBits g + b, b a set bit
// of pat, summed. Jobs beyond the instance's and machines beyond it are zero. A machine's
// column sum is below 65536 (pfsp_front_ok), so the 32-bit sum of the groups' rows never carries
// from a low half into a high one. Built once per instance; the GPU front kernels stage the
// same rows into LDS (csrc/hip/pfsp_front_kernels.hpp front_remain).
// [kRemainGroups][kRemainPats][(MB + 1) / 2] packed words
inline std::vector<uint32_t> pfsp_front_remain_table(const PfspInstance& in, int MB) {
  if (in.jobs > 20 || in.machines > MB || MB > 20) throw std::invalid_argument("remain table: 20-job front buckets only");
  const int HW = (MB + 1) / 2;
  std::vector<uint32_t> t(static_cast<size_t>(kRemainGroups) * kRemainPats * HW, 0u);
  for (int g = 0; g < kRemainGroups; ++g)
    for (int pat = 1; pat < kRemainPats; ++pat) {
      // the row of pat without its lowest bit, plus that bit's job
      const int b = __builtin_ctz(static_cast<unsigned>(pat)), j = kRemainBits * g + b;
      uint32_t* row = &t[(static_cast<size_t>(g) * kRemainPats + pat) * HW];
      const uint32_t* prev = &t[(static_cast<size_t>(g) * kRemainPats + (pat & (pat - 1))) * HW];
      for (int h = 0; h < HW; ++h) row[h] = prev[h];
      if (j >= in.jobs) continue;
      for (int m = 0; m < in.machines; ++m) row[m >> 1] += static_cast<uint32_t>(in.pt(m, j)) << ((m & 1) * 16);
    }
  return t;
}

template <int MB, int NJ = 20>
struct PfspFrontProblem {
  using Node = PfspFrontNode<MB, NJ>;
  using Mask = typename Node::Mask;
  static constexpr int kJobs = NJ;
  static constexpr int kMaxJ = 8 * static_cast<int>(sizeof(Mask));  // the set's width
  const PfspInstance* inst = nullptr;
  int lb = 1;
  int jobs = 0;
  PfspPadded tab{};
  int p[kMaxJ][MB];  // job-major, padded machines 0

  PfspFrontProblem(const PfspInstance& in, int lb_kind) : inst(&in), lb(lb_kind), jobs(in.jobs) {
    if (!pfsp_front_ok(in, lb_kind)) throw std::invalid_argument("front layout does not apply to this instance");
    if (pfsp_machine_bucket(in.machines) != MB) throw std::invalid_argument("wrong machine bucket");
    if (pfsp_front_jobs(in.jobs) != NJ) throw std::invalid_argument("wrong front job bucket");
    tab = pfsp_padded_tables(in, MB);
    for (int j = 0; j < kMaxJ; ++j)
      for (int m = 0; m < MB; ++m) p[j][m] = (j < in.jobs && m < in.machines) ? in.pt(m, j) : 0;
  }

  Mask all_jobs() const { return mask_first<Mask>(jobs); }

  Node root() const {
    Node r{};
    r.depth = 0;
    r.rest = all_jobs();
    for (int m = 0; m < MB; ++m) r.front[m] = static_cast<uint16_t>(tab.heads[m]);
    return r;
  }

  // remain + tail of the parent's unscheduled jobs, per machine
  void remain_tail(const Node& n, int* r) const {
    for (int m = 0; m < MB; ++m) r[m] = tab.tails[m];
    for (Mask x = n.rest; !mask_empty(x); mask_pop_low(x)) {
      const int j = mask_ctz(x);
      for (int m = 0; m < MB; ++m) r[m] += p[j][m];
    }
  }

  // Bound of the child appending job j; its front in cf (when non-null).
  int child(const Node& n, const int* r, int j, uint16_t* cf) const {
    const int* pj = p[j];
    int f0 = n.front[0];
    int lb = f0 + r[0];
    int tt = f0 + pj[0];
    // the root's front is the minimum heads (bound only); a child's front starts from 0
    int ft = (n.depth == 0 ? 0 : f0) + pj[0];
    if (cf) cf[0] = static_cast<uint16_t>(ft);
    for (int m = 1; m < MB; ++m) {
      const int fm = n.front[m];
      const int sv = std::max(tt, fm);
      lb = std::max(lb, sv + r[m]);
      tt = sv + pj[m];
      ft = std::max(ft, n.depth == 0 ? 0 : fm) + pj[m];
      if (cf) cf[m] = static_cast<uint16_t>(ft);
    }
    return lb;
  }

  // Bound of the node itself (IEngine::pool_bound): cpu_lb1 of its prefix, from what the
  // node carries — the machine-bound chain (cpu_machine_bound) over front + remain of the
  // unscheduled set + minimum tail, in 32 bits (a u16 front plus a remain may pass 65535).
  // The root's fronts are the minimum heads. Real machines only, as cpu_lb1.
  int node_bound(const Node& n, int /*cap*/) const {
    int r[MB];
    remain_tail(n, r);  // remain + tail
    int run = n.front[0] + r[0] - tab.tails[0];
    int lb = run + tab.tails[0];
    for (int m = 1; m < inst->machines; ++m) {
      run = std::max(run, n.front[m] + r[m] - tab.tails[m]);
      lb = std::max(lb, run + tab.tails[m]);
    }
    return lb;
  }

  // Bounds of every child, by job (lb_by_job[j] for j in n.rest).
  void children_bounds(const Node& n, int* lb_by_job) const {
    int r[MB];
    remain_tail(n, r);
    for (Mask x = n.rest; !mask_empty(x); mask_pop_low(x)) {
      const int j = mask_ctz(x);
      lb_by_job[j] = child(n, r, j, nullptr);
    }
  }

  template <class Push>
  void decompose(const Node& parent, int& best, unsigned long long& tree, unsigned long long& sol, Push&& push) const {
    int r[MB];
    remain_tail(parent, r);
    const bool leaf = parent.depth + 1 == jobs;
    for (Mask x = parent.rest; !mask_empty(x); mask_pop_low(x)) {
      const int j = mask_ctz(x);
      Node c{};
      const int b = child(parent, r, j, leaf ? nullptr : c.front);
      if (leaf) {
        ++sol;
        if (b < best) best = b;
      } else if (b < best) {
        c.depth = static_cast<typename Node::depth_t>(parent.depth + 1);
        c.rest = parent.rest;
        mask_clear(c.rest, j);
        push(c);
        ++tree;
      }
    }
  }
};

template <class P>
struct is_front_problem : std::false_type {};
template <int MB, int NJ>
struct is_front_problem<PfspFrontProblem<MB, NJ>> : std::true_type {};

// Front node of a permutation node (scheduled prefix prmu[0..depth)).
template <int MB, int NJ, class PermNode>
inline PfspFrontNode<MB, NJ> pfsp_front_from_perm(const PfspFrontProblem<MB, NJ>& prob, const PermNode& n) {
  PfspFrontNode<MB, NJ> f{};
  f.depth = static_cast<typename PfspFrontNode<MB, NJ>::depth_t>(n.depth);
  f.rest = prob.all_jobs();
  if (n.depth == 0) {
    for (int m = 0; m < MB; ++m) f.front[m] = static_cast<uint16_t>(prob.tab.heads[m]);
    return f;
  }
  int fr[MB] = {};
  for (int i = 0; i < n.depth; ++i) {
    const int j = n.prmu[i];
    mask_clear(f.rest, j);
    fr[0] += prob.p[j][0];
    for (int m = 1; m < MB; ++m) fr[m] = std::max(fr[m - 1], fr[m]) + prob.p[j][m];
  }
  for (int m = 0; m < MB; ++m) f.front[m] = static_cast<uint16_t>(fr[m]);
  return f;
}

// Calls f(problem) with the problem in the node layout every engine, driver and host
// step uses for (instance, lb): the front layout where it applies, else the
// permutation layout of the job-count bucket.
template <class F>
decltype(auto) with_pfsp_problem(const PfspInstance& in, int lb, F&& f) {
  if (pfsp_front_ok(in, lb)) {
    if (in.jobs <= 20) {
      switch (pfsp_machine_bucket(in.machines)) {
        case 5: return f(PfspFrontProblem<5>(in, lb));
        case 10: return f(PfspFrontProblem<10>(in, lb));
        default: return f(PfspFrontProblem<20>(in, lb));
      }
    }
    if (in.jobs <= 50) {
      switch (pfsp_machine_bucket(in.machines)) {
        case 5: return f(PfspFrontProblem<5, 50>(in, lb));
        case 10: return f(PfspFrontProblem<10, 50>(in, lb));
        default: return f(PfspFrontProblem<20, 50>(in, lb));
      }
    }
    if (in.jobs <= 100) {
      switch (pfsp_machine_bucket(in.machines)) {
        case 5: return f(PfspFrontProblem<5, 100>(in, lb));
        case 10: return f(PfspFrontProblem<10, 100>(in, lb));
        default: return f(PfspFrontProblem<20, 100>(in, lb));
      }
    }
    if (in.jobs <= 200) {
      switch (pfsp_machine_bucket(in.machines)) {
        case 5: return f(PfspFrontProblem<5, 200>(in, lb));
        case 10: return f(PfspFrontProblem<10, 200>(in, lb));
        default: return f(PfspFrontProblem<20, 200>(in, lb));
      }
    }
    switch (pfsp_machine_bucket(in.machines)) {
      case 5: return f(PfspFrontProblem<5, 500>(in, lb));
      case 10: return f(PfspFrontProblem<10, 500>(in, lb));
      default: return f(PfspFrontProblem<20, 500>(in, lb));
    }
  }
  return with_pfsp_bucket(in.jobs, [&](auto nj) -> decltype(auto) {
    return f(PfspProblem<decltype(nj)::value>(in, lb));
  });
}

}  // namespace tts
