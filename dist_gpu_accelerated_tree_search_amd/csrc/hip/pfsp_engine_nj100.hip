// Kernel instantiations for the 100-job node bucket (one TU per bucket so the
// instantiations compile in parallel).
#include "pfsp_engine.hpp"

namespace tts {
TTS_PFSP_DEFINE_BUCKET(100)

// 51-100 jobs on front nodes with 128-bit job sets (TTS_FRONT_WIDE=1; pfsp_front_probe /
// pfsp_front_time / pfsp_front_expand_probe dispatch here from the 20-job TU)
FrontProbeResult pfsp_front_probe_nj100(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                        const EngineConfig& cfg, unsigned cap, int split_rank, int split_world,
                                        size_t split_min) {
  return with_machine_bucket(in.machines, [&](auto mm) {
    return pfsp_front_probe_t<decltype(mm)::value, 100>(in, lb, nodes, n, best, cfg, cap, split_rank, split_world,
                                                        split_min);
  });
}
std::vector<double> pfsp_front_time_nj100(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                          const EngineConfig& cfg, int reps) {
  return with_machine_bucket(in.machines, [&](auto mm) {
    return pfsp_front_time_t<decltype(mm)::value, 100>(in, lb, nodes, n, best, cfg, reps);
  });
}
FrontExpandResult pfsp_front_expand_probe_nj100(const PfspInstance& in, const void* nodes, size_t n, int best, int steps,
                                                int device, bool production) {
  return with_machine_bucket(in.machines, [&](auto mm) {
    return pfsp_front_expand_probe_t<decltype(mm)::value, 100>(in, nodes, n, best, steps, device, production);
  });
}
}  // namespace tts
