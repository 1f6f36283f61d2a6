// Host bookkeeping of the device ring (hip/engine.hpp), host-only and header-only so the
// CPU tests reach it (tests/test_pool_ring.py through _tts_cpu): where a run of ring slots
// lies and how the host shadow of the ring moves (PoolRing), and which graph a replay may
// take given the ring's worst-case growth (ReplayPlan). One wrong term here loses or
// duplicates nodes, which a GPU run shows only as a wrong tree count, if it wraps at all.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace tts {

struct RingSpan {
  size_t offset, count;
};
// The at most two contiguous pieces of a run of slots, in order; a second piece starts at 0.
struct RingSpans {
  RingSpan piece[2];
  int pieces;
  const RingSpan* begin() const { return piece; }
  const RingSpan* end() const { return piece + pieces; }
};

// A ring of `cap` (a power of two) slots holding `stack` nodes from slot `bot` upwards. The
// two words are those of the host control block (PoolCtl bot and slot[0].stack), which is
// overwritten from the mirror after each replay: the ring refers to them and keeps no copy.
// bot is stored masked (< cap).
class PoolRing {
 public:
  using Word = unsigned long long;
  PoolRing() = default;
  PoolRing(size_t cap, Word* bot, Word* stack) : cap_(cap), bot_(bot), stack_(stack) {}
  size_t cap() const { return cap_; }
  size_t bot() const { return static_cast<size_t>(*bot_); }
  size_t stack() const { return static_cast<size_t>(*stack_); }
  size_t top() const { return bot() + stack(); }  // the slot after the newest node (spans() masks it)
  RingSpans spans(size_t start, size_t n) const {
    start &= cap_ - 1;
    const size_t first = std::min(n, cap_ - start);
    return {{{start, first}, {0, n - first}}, (first != 0) + (first < n)};
  }
  // The slot k under the bottom, and how many slots under the bottom are contiguous.
  size_t under_bottom(size_t k) const { return (bot() + cap_ - k) & (cap_ - 1); }
  size_t contiguous_under_bottom() const { return bot() ? bot() : cap_; }

  void pop_bottom(size_t n) {
    *bot_ = (bot() + n) & (cap_ - 1);
    *stack_ -= n;
  }
  void push_top(size_t n) {
    if (stack() + n > cap_) throw std::runtime_error("device ring capacity exceeded");
    *stack_ += n;
  }
  void extend_bottom(size_t k) {
    *bot_ = under_bottom(k);
    *stack_ += k;
  }
  void reset(size_t n) {  // n nodes from slot 0
    *bot_ = 0;
    *stack_ = n;
  }

 private:
  size_t cap_ = 1;
  Word *bot_ = nullptr, *stack_ = nullptr;
};

// Which graph a replay takes. The graphs hold ks() iterations: iters_small doubling up to
// iters_large, and the first replay's length when it is none of them. A replay of k
// iterations grows the ring by at most growth(k) and pops at most k x max_parents parents.
class ReplayPlan {
 public:
  ReplayPlan() = default;
  ReplayPlan(int iters_small, int iters_large, int iters_first, size_t buf_nodes, size_t cap, size_t max_parents)
      : buf_nodes_(buf_nodes), cap_(cap), max_parents_(max_parents), iters_first_(iters_first),
        iters_large_(iters_large) {
    for (int k = iters_small; k <= iters_large; k *= 2) ks_.push_back(k);
    if (iters_first % 6 == 0 && iters_first < iters_large &&
        std::find(ks_.begin(), ks_.end(), iters_first) == ks_.end()) {
      ks_.push_back(iters_first);
      std::sort(ks_.begin(), ks_.end());
    }
  }
  const std::vector<int>& ks() const { return ks_; }
  size_t growth(int k) const { return static_cast<size_t>(k + 1) * buf_nodes_; }
  // Largest graph whose worst-case ring growth (plus `extra` already in flight and the
  // `reserved` spans of copies in flight) fits, no longer than the pool size suggests: 6
  // iterations while ramping up or draining, more when the pool holds several parent
  // windows, at most kmax. Right after begin() (fresh): one long replay (iters_first) — a
  // graph boundary costs ~50 us of host sync + relaunch, an empty iteration ~4.5 us
  // (profiles/r1/r1f). Index into ks(), -1 when none fits.
  int pick(size_t total, size_t extra, size_t reserved, bool fresh, size_t kmax = SIZE_MAX) const {
    size_t want = fresh ? std::max<size_t>(6, static_cast<size_t>(iters_first_)) : 6;
    while (want < static_cast<size_t>(iters_large_) && total >= (want / 6) * 2 * max_parents_ && want * 2 <= kmax)
      want *= 2;
    for (int i = static_cast<int>(ks_.size()) - 1; i >= 0; --i) {
      if (static_cast<size_t>(ks_[i]) > want && i > 0) continue;
      if (total + extra + reserved + growth(ks_[i]) <= cap_) return i;
    }
    return -1;
  }
  // Does a replay of k iterations fit (the learned first replay, a warm-up pass)?
  bool fits(size_t total, size_t reserved, int k) const { return total + reserved + growth(k) <= cap_; }
  // The longest replay left running over a round: half of the pool stays exportable under it.
  size_t leave_kmax(size_t total) const { return std::max<size_t>(6, total / 2 / max_parents_); }
  // What no replay in flight can reach: they pop at most their iterations x window parents
  // from the top, so the oldest nodes above that (plus one window of margin) are safe.
  template <class Ks>
  size_t exportable_ahead(size_t stack, size_t export_pending, const Ks& inflight_ks) const {
    size_t k = 0;
    for (int x : inflight_ks) k += static_cast<size_t>(x);
    const size_t safe = (k + 1) * max_parents_, left = stack - export_pending;
    return left > safe ? left - safe : 0;
  }
  // How many nodes a refill may bring back with `used` on the device: the device part stays
  // within half the ring (like push_host), and the smallest graph must still fit afterwards
  // (else refills and spills would alternate).
  size_t refill_limit(size_t used) const {
    const size_t g = growth(ks_.front()), limit = std::min(cap_ / 2, cap_ > g ? cap_ - g : 0);
    return limit > used ? limit - used : 0;
  }
  // What a spill ahead leaves on the device: half the ring, and twice what the longest
  // graph can pop.
  size_t spill_ahead_keep() const {
    return std::max(cap_ / 2, 2 * static_cast<size_t>(ks_.back() + 1) * max_parents_);
  }

 private:
  std::vector<int> ks_;
  size_t buf_nodes_ = 0, cap_ = 0, max_parents_ = 1;
  int iters_first_ = 0, iters_large_ = 0;
};

}  // namespace tts
