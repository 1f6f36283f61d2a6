// Run-time dispatch of PFSP engines / bound evaluation / probes over the job-count buckets.
#include "pfsp_engine.hpp"

namespace tts {

std::unique_ptr<IEngine> make_pfsp_engine(const PfspInstance& in, int lb, const EngineConfig& cfg) {
  switch (pfsp_bucket(in.jobs)) {
    case 20: return make_pfsp_engine_nj20(in, lb, cfg);
    case 50: return make_pfsp_engine_nj50(in, lb, cfg);
    case 100: return make_pfsp_engine_nj100(in, lb, cfg);
    case 200: return make_pfsp_engine_nj200(in, lb, cfg);
    default: return make_pfsp_engine_nj500(in, lb, cfg);
  }
}

std::vector<int> pfsp_gpu_bounds(const PfspInstance& in, int lb, const void* parents, size_t n, int best, int device) {
  switch (pfsp_bucket(in.jobs)) {
    case 20: return pfsp_gpu_bounds_nj20(in, lb, parents, n, best, device);
    case 50: return pfsp_gpu_bounds_nj50(in, lb, parents, n, best, device);
    case 100: return pfsp_gpu_bounds_nj100(in, lb, parents, n, best, device);
    case 200: return pfsp_gpu_bounds_nj200(in, lb, parents, n, best, device);
    default: return pfsp_gpu_bounds_nj500(in, lb, parents, n, best, device);
  }
}

std::vector<int> pfsp_expand_probe(const PfspInstance& in, int lb, const void* parents, size_t n, int best, int device,
                                   int variant, int reps, std::vector<double>* timing, ExpandProbeResult* extra) {
  switch (pfsp_bucket(in.jobs)) {
    case 20: return pfsp_expand_probe_nj20(in, lb, parents, n, best, device, variant, reps, timing, extra);
    case 50: return pfsp_expand_probe_nj50(in, lb, parents, n, best, device, variant, reps, timing, extra);
    case 100: return pfsp_expand_probe_nj100(in, lb, parents, n, best, device, variant, reps, timing, extra);
    case 200: return pfsp_expand_probe_nj200(in, lb, parents, n, best, device, variant, reps, timing, extra);
    default: return pfsp_expand_probe_nj500(in, lb, parents, n, best, device, variant, reps, timing, extra);
  }
}

ExpandProbeResult pfsp_lb1_expand_probe(const PfspInstance& in, const void* parents, size_t n, int best, int device) {
  switch (pfsp_bucket(in.jobs)) {
    case 20: return pfsp_lb1_expand_probe_nj20(in, parents, n, best, device);
    case 50: return pfsp_lb1_expand_probe_nj50(in, parents, n, best, device);
    case 100: return pfsp_lb1_expand_probe_nj100(in, parents, n, best, device);
    case 200: return pfsp_lb1_expand_probe_nj200(in, parents, n, best, device);
    default: return pfsp_lb1_expand_probe_nj500(in, parents, n, best, device);
  }
}

// The front probes: the front buckets of 20, 50, 100, 200 and 500 jobs.
FrontProbeResult pfsp_front_probe(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                  const EngineConfig& cfg, unsigned cap, int split_rank, int split_world,
                                  size_t split_min) {
  if (!pfsp_front_ok(in, lb)) throw std::invalid_argument("front probe: the front layout does not apply");
  if (in.jobs > 200) return pfsp_front_probe_nj500(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, split_min);
  if (in.jobs > 100) return pfsp_front_probe_nj200(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, split_min);
  if (in.jobs > 50) return pfsp_front_probe_nj100(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, split_min);
  if (in.jobs > 20) return pfsp_front_probe_nj50(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, split_min);
  return pfsp_front_probe_nj20(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, split_min);
}

std::vector<double> pfsp_front_time(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                    const EngineConfig& cfg, int reps) {
  if (!pfsp_front_ok(in, lb)) throw std::invalid_argument("front timing: the front layout does not apply");
  if (in.jobs > 200) return pfsp_front_time_nj500(in, lb, nodes, n, best, cfg, reps);
  if (in.jobs > 100) return pfsp_front_time_nj200(in, lb, nodes, n, best, cfg, reps);
  if (in.jobs > 50) return pfsp_front_time_nj100(in, lb, nodes, n, best, cfg, reps);
  if (in.jobs > 20) return pfsp_front_time_nj50(in, lb, nodes, n, best, cfg, reps);
  return pfsp_front_time_nj20(in, lb, nodes, n, best, cfg, reps);
}

FrontExpandResult pfsp_front_expand_probe(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, int steps,
                                          int device, bool production) {
  if (!pfsp_front_ok(in, lb)) throw std::invalid_argument("front expand probe: the front layout does not apply");
  if (in.jobs > 200) return pfsp_front_expand_probe_nj500(in, nodes, n, best, steps, device, production);
  if (in.jobs > 100) return pfsp_front_expand_probe_nj200(in, nodes, n, best, steps, device, production);
  if (in.jobs > 50) return pfsp_front_expand_probe_nj100(in, nodes, n, best, steps, device, production);
  if (in.jobs > 20) return pfsp_front_expand_probe_nj50(in, nodes, n, best, steps, device, production);
  return pfsp_front_expand_probe_nj20(in, nodes, n, best, steps, device, production);
}

}  // namespace tts
