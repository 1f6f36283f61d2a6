// Device allocations of a one-iteration probe (pfsp_engine.hpp, queens_engine.hip).
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "device_common.hpp"

namespace tts {

// Device allocations of a probe: freed on every exit path (a throwing HIP check included).
struct ProbeAllocs {
  std::vector<void*> owned;
  ProbeAllocs() = default;
  ProbeAllocs(const ProbeAllocs&) = delete;
  ProbeAllocs& operator=(const ProbeAllocs&) = delete;
  ~ProbeAllocs() {
    for (void* d : owned) (void)hipFree(d);
  }
  // zeroed device memory
  void* zeroed(size_t bytes) {
    void* d = nullptr;
    TTS_HIP_CHECK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
    owned.push_back(d);
    TTS_HIP_CHECK(hipMemset(d, 0, std::max<size_t>(bytes, 16)));
    return d;
  }
};

}  // namespace tts
