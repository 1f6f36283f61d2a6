// Plumbing of the one-iteration probes (pfsp_probes.hpp, queens_engine.hip): device
// allocations freed on every exit path, a pool of one window with its read-back, launch
// timing and the conversion of workgroup stamps.
#pragma once

#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "pool_device.hpp"

namespace tts {

// Device allocations of a probe: freed on every exit path (a throwing HIP check included).
// Every block is registered before anything else can fail.
struct ProbeAllocs {
  std::vector<void*> owned;
  ProbeAllocs() = default;
  ProbeAllocs(const ProbeAllocs&) = delete;
  ProbeAllocs& operator=(const ProbeAllocs&) = delete;
  ~ProbeAllocs() {
    for (void* d : owned) (void)hipFree(d);
  }
  template <class T>
  T* alloc(size_t count) {
    owned.push_back(nullptr);
    TTS_HIP_CHECK(hipMalloc(&owned.back(), std::max<size_t>(count * sizeof(T), 16)));
    return static_cast<T*>(owned.back());
  }
  template <class T>
  T* zeroed(size_t count) {
    T* d = alloc<T>(count);
    TTS_HIP_CHECK(hipMemset(d, 0, std::max<size_t>(count * sizeof(T), 16)));
    return d;
  }
  // device copy of host data
  template <class T>
  T* upload(const T* h, size_t count) {
    T* d = alloc<T>(count);
    if (count) TTS_HIP_CHECK(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  template <class T>
  T* upload(const std::vector<T>& v) {
    return upload(v.data(), v.size());
  }
};

// What an iteration wrote to buffer 1: per output chunk its count and raw leaf word (the
// caller splits it), and the children's bytes chunk after chunk.
struct ProbeChunks {
  std::vector<int> counts, lwords;
  std::vector<uint8_t> children;
};

// A pool of one window in `pa`: `n` nodes in a power-of-two ring, two child buffers of
// nchunks x slot nodes with their counts, and the control block `h` with slot[0].stack = n.
template <class Node>
struct ProbePool {
  dev::PoolArgs<Node>& pa;
  const void* nodes;
  size_t n, slot;
  dev::PoolCtl h0;
  ProbePool(ProbeAllocs& mem, dev::PoolArgs<Node>& pa_, const void* nodes_, size_t n_, size_t nchunks, size_t slot_,
            int parents_per_chunk, const dev::PoolCtl& h)
      : pa(pa_), nodes(nodes_), n(n_), slot(slot_), h0(h) {
    h0.slot[0].stack = n;
    size_t cap = 1;
    while (cap < n) cap *= 2;
    pa.ring = mem.zeroed<Node>(cap);
    for (int b = 0; b < 2; ++b) {
      pa.buf[b] = mem.zeroed<Node>(nchunks * slot);
      pa.cnt[b] = mem.zeroed<int>(nchunks);
      pa.lcnt[b] = mem.zeroed<int>(nchunks);
    }
    pa.ctl = mem.zeroed<dev::PoolCtl>(1);
    pa.mirror = nullptr;
    pa.cap_mask = cap - 1;
    pa.max_parents = static_cast<int>(nchunks * parents_per_chunk);
    pa.max_chunks = static_cast<int>(nchunks);
    restore();
  }
  // the window and the initial control block again (timing loops)
  void restore() const {
    TTS_HIP_CHECK(hipMemcpy(pa.ring, nodes, n * sizeof(Node), hipMemcpyHostToDevice));
    TTS_HIP_CHECK(hipMemcpy(pa.ctl, &h0, sizeof(h0), hipMemcpyHostToDevice));
  }
  dev::PoolCtl ctl() const {
    dev::PoolCtl h{};
    TTS_HIP_CHECK(hipMemcpy(&h, pa.ctl, sizeof(h), hipMemcpyDeviceToHost));
    return h;
  }
  // the first `nout` chunks of buffer 1; `who` names the probe in the range error
  ProbeChunks read_chunks(size_t nout, const char* who) const {
    ProbeChunks r;
    r.counts.assign(nout, 0);
    r.lwords.assign(nout, 0);
    TTS_HIP_CHECK(hipMemcpy(r.counts.data(), pa.cnt[1], nout * sizeof(int), hipMemcpyDeviceToHost));
    TTS_HIP_CHECK(hipMemcpy(r.lwords.data(), pa.lcnt[1], nout * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < nout; ++c) {
      if (r.counts[c] < 0 || static_cast<size_t>(r.counts[c]) > slot)
        throw std::runtime_error(std::string(who) + ": chunk count out of range");
      const size_t at = r.children.size(), bytes = static_cast<size_t>(r.counts[c]) * sizeof(Node);
      r.children.resize(at + bytes);
      if (bytes) TTS_HIP_CHECK(hipMemcpy(r.children.data() + at, pa.buf[1] + c * slot, bytes, hipMemcpyDeviceToHost));
    }
    return r;
  }
};

struct ProbeEvent {
  hipEvent_t e = nullptr;
  ProbeEvent() { TTS_HIP_CHECK(hipEventCreate(&e)); }
  ProbeEvent(const ProbeEvent&) = delete;
  ProbeEvent& operator=(const ProbeEvent&) = delete;
  ~ProbeEvent() { (void)hipEventDestroy(e); }
};

// max(1, reps) times: restore(), then launch() between two events. Sorted milliseconds.
template <class Restore, class Launch>
std::vector<double> time_launches(int reps, Restore&& restore, Launch&& launch) {
  ProbeEvent e0, e1;
  std::vector<double> ms;
  for (int r = 0; r < std::max(1, reps); ++r) {
    restore();
    TTS_HIP_CHECK(hipEventRecord(e0.e, 0));
    launch();
    TTS_HIP_CHECK(hipEventRecord(e1.e, 0));
    TTS_HIP_CHECK(hipEventSynchronize(e1.e));
    float t = 0;
    TTS_HIP_CHECK(hipEventElapsedTime(&t, e0.e, e1.e));
    ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  return ms;
}

// Wall-clock stamps, `stride` words per workgroup with its entry stamp first, to
// microseconds from the earliest non-zero entry stamp.
struct StampClock {
  unsigned long long t0 = ~0ull;
  double us_per_tick = 0;
  StampClock(const std::vector<unsigned long long>& stamps, size_t stride, int device) {
    int rate_khz = 0;
    TTS_HIP_CHECK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, device));
    us_per_tick = 1e3 / std::max(1, rate_khz);
    for (size_t i = 0; i < stamps.size(); i += stride)
      if (stamps[i]) t0 = std::min(t0, stamps[i]);
  }
  double operator()(unsigned long long x) const { return static_cast<double>(x - t0) * us_per_tick; }
};

// Exclusive prefix of the child counts of permutation parents (children k = depth..jobs-1).
template <class Node>
std::vector<int> perm_child_offsets(const Node* parents, size_t n, int jobs) {
  std::vector<int> offsets(n + 1, 0);
  for (size_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + (jobs - parents[i].depth);
  return offsets;
}

}  // namespace tts
