// Device Knuth tree-size estimate for PFSP: the launcher of hip/estimate_kernels.hpp.
// Probes [first_probe, first_probe + probes) of the host twin (core/estimate.hpp
// knuth_estimate_indexed, or lookahead_estimate_indexed for the lookahead method), run in
// bounded launches; the per-workgroup partial sums are
// reduced on the host in (launch, workgroup) order.
#pragma once

#include <string>

#include "../core/estimate.hpp"
#include "../core/pfsp_instance.hpp"

namespace tts {

// Accepted ranges (docs/KNOBS.md §6); anything else is a std::invalid_argument, never a
// silently different number.
constexpr int kEstimateMaxJobs = 512;     // eight 64-bit set words
constexpr int kEstimateMaxMachines = 64;  // one lane per machine at a probe's root
// and tables plus the state of at least one wave within 64 KB of LDS (pfsp_estimate_reject)

struct DeviceEstimate {
  TreeEstimate est;
  ProbeRecords records;            // filled when asked
  unsigned long long batch = 0;    // probes per launch after the first
  double rate = 0;                 // probes/s of the first launch, which sized `batch` (0: batch was given)
  double first_seconds = 0;        // duration of that first launch
  int grid = 0, waves = 0;         // workgroups of a full launch, waves per workgroup
  unsigned lds_bytes = 0;
  unsigned long long launches = 0;
  double seconds = 0;              // all launches, host clock
};

// Empty when the device estimator accepts (instance, lb); else the reason. A lookahead
// probe (method.lookahead, hip/estimate_kernels.hpp lookahead_probe_kernel) keeps a second
// node, k_c and the weights' prefix sums per wave, so it refuses somewhat smaller instances.
std::string pfsp_estimate_reject(const PfspInstance& in, int lb, const EstimateMethod& method = {});

// batch 0: the first launch is one pass of the resident grid (one probe per wave, at most
// kEstimateFirstBatch probes) and is timed; later launches take as many probes as that rate
// fits into kEstimateLaunchSeconds, more or fewer than the first. A first launch longer than
// kEstimateMaxLaunchSeconds is an std::invalid_argument: one probe per wave is the shortest
// launch there is, so no launch of that instance would be short. batch > 0: that many probes
// per launch. max_blocks > 0 caps the workgroups of a launch (tests: a short grid pass).
constexpr unsigned long long kEstimateFirstBatch = 4096;
constexpr double kEstimateLaunchSeconds = 0.2;
constexpr double kEstimateMaxLaunchSeconds = 1.0;
constexpr unsigned long long kEstimateMaxBatch = 1ull << 22;

DeviceEstimate pfsp_device_estimate(const PfspInstance& in, int lb, int best, unsigned long long first_probe,
                                    unsigned long long probes, unsigned long long seed, int device, bool records,
                                    unsigned long long batch, int max_blocks = 0, const EstimateMethod& method = {});

}  // namespace tts
