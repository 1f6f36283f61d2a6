// Launcher of the device tree-size estimators, Knuth and lookahead (estimate_device.hpp,
// estimate_kernels.hpp).
#include "estimate_device.hpp"

#include <chrono>
#include <cstring>

#include "../core/pfsp_bounds_cpu.hpp"
#include "estimate_kernels.hpp"

namespace tts {

namespace {

struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  explicit DevBuf(size_t bytes) { TTS_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1)); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

template <class T>
DevBuf upload(const std::vector<T>& v) {
  DevBuf b(v.size() * sizeof(T));
  if (!v.empty()) TTS_HIP_CHECK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return b;
}

struct Stream {
  hipStream_t s = nullptr;
  Stream() { TTS_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

constexpr unsigned kEstLdsLimit = 64u * 1024u;  // what a workgroup gets without opting in to more

using Kernel = void (*)(dev::EstParams);
Kernel pick_kernel(bool lb2) { return lb2 ? dev::knuth_probe_kernel<true> : dev::knuth_probe_kernel<false>; }

using LookKernel = void (*)(dev::LookParams);
LookKernel pick_look_kernel(bool lb2, bool own) {
  if (!lb2) return dev::lookahead_probe_kernel<false, true>;
  return own ? dev::lookahead_probe_kernel<true, true> : dev::lookahead_probe_kernel<true, false>;
}

dev::EstLds lds_layout(int N, int M, int P, bool lb2, int waves, bool lookahead) {
  return lookahead ? dev::look_lds_layout(N, M, P, lb2, waves).base : dev::est_lds_layout(N, M, P, lb2, waves);
}

// Waves per workgroup with which tables and wave state fit the LDS limit: 4, 2 or 1; 0: none.
int fitting_waves(int N, int M, int P, bool lb2, bool lookahead) {
  for (int waves : {dev::kBlock / dev::kWave, 2, 1})
    if (lds_layout(N, M, P, lb2, waves, lookahead).total <= kEstLdsLimit) return waves;
  return 0;
}

}  // namespace

std::string pfsp_estimate_reject(const PfspInstance& in, int lb, const EstimateMethod& method) {
  if (lb < 0 || lb > 2) return "lower bound must be 0, 1 or 2";
  if (method.lookahead) {
    if (method.power < 1 || method.power > kLookaheadMaxPower) return "lookahead power must be 1, 2 or 3";
    if (method.look != kLookBoundOwn && method.look != kLookBoundLb1) return "lookahead bound must be own or lb1";
  }
  if (in.jobs < 1 || in.jobs > kEstimateMaxJobs)
    return "the device estimator takes 1 to " + std::to_string(kEstimateMaxJobs) + " jobs";
  if (in.machines < 2 || in.machines > kEstimateMaxMachines)
    return "the device estimator takes 2 to " + std::to_string(kEstimateMaxMachines) + " machines";
  long long sum = 0;
  for (int v : in.p) {
    if (v < 0) return "negative processing time";
    sum += v;
  }
  // every front, remain, tail, lag and walk value is a sum of distinct cells of p, and a
  // bound adds at most three of them
  if (3 * sum > INT_MAX)
    return "processing times too large for the device estimator: three times their sum must fit 31 bits";
  // the kernel reads its tables from LDS only
  if (fitting_waves(in.jobs, in.machines, in.npairs, lb == 2, method.lookahead) == 0)
    return "instance too large for the device estimator: its " + std::string(lb == 2 ? "LB2 " : "") +
           "tables and the " + std::string(method.lookahead ? "lookahead " : "") +
           "state of one wave pass 64 KB of LDS ("+ std::to_string(in.jobs) + " jobs x " +
           std::to_string(in.machines) + " machines)";
  return {};
}

DeviceEstimate pfsp_device_estimate(const PfspInstance& in, int lb, int best, unsigned long long first_probe,
                                    unsigned long long probes, unsigned long long seed, int device, bool records,
                                    unsigned long long batch, int max_blocks, const EstimateMethod& method) {
  const std::string why = pfsp_estimate_reject(in, lb, method);
  if (!why.empty()) throw std::invalid_argument(why);
  if (records && probes > ProbeRecords::kMaxProbes)
    throw std::invalid_argument("probe records are kept for at most 2^20 probes");
  const int N = in.jobs, M = in.machines, P = in.npairs;
  const bool lb2 = lb == 2;
  TTS_HIP_CHECK(hipSetDevice(device));

  // ---- tables ----
  std::vector<int> cum(static_cast<size_t>(M + 1) * N, 0);
  for (int m = 0; m < M; ++m)
    for (int j = 0; j < N; ++j) cum[static_cast<size_t>(m + 1) * N + j] = cum[static_cast<size_t>(m) * N + j] + in.pt(m, j);
  std::vector<uint16_t> joh, pair, pair_id;
  if (lb2) {
    joh.resize(static_cast<size_t>(P) * N);
    for (size_t i = 0; i < joh.size(); ++i) joh[i] = static_cast<uint16_t>(in.johnson[i]);
    for (int q : lb2_pair_order(in)) {
      pair.push_back(static_cast<uint16_t>(in.pair_m0[q] | (in.pair_m1[q] << 8)));
      pair_id.push_back(static_cast<uint16_t>(q));
    }
  }
  const DevBuf d_cum = upload(cum), d_tails = upload(in.min_tails), d_joh = upload(joh), d_pair = upload(pair),
               d_pid = upload(pair_id);

  // ---- shape of a launch: the most waves per workgroup with which everything fits LDS ----
  DeviceEstimate out;
  const bool look = method.lookahead;
  const int waves = fitting_waves(N, M, P, lb2, look);
  const dev::EstLds L = lds_layout(N, M, P, lb2, waves, look);
  const Kernel kernel = pick_kernel(lb2);
  // LB1's lookahead bound is its own whatever was asked: the LB1 chain
  const LookKernel look_kernel = pick_look_kernel(lb2, method.look == kLookBoundOwn);
  hipDeviceProp_t prop;
  TTS_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  int per_cu = 0;
  TTS_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, look ? reinterpret_cast<const void*>(look_kernel) : reinterpret_cast<const void*>(kernel),
      waves * dev::kWave, L.total));
  int max_grid = std::max(1, per_cu) * prop.multiProcessorCount;
  if (max_blocks >= 1) max_grid = std::min(max_grid, max_blocks);
  out.grid = max_grid;
  out.waves = waves;
  out.lds_bytes = L.total;

  // the first launch is one pass of the resident grid, the shortest a launch can be: a
  // wave walks one probe, and fewer probes only leave waves idle
  const unsigned long long pass = static_cast<unsigned long long>(max_grid) * waves;
  const unsigned long long cap = batch ? batch : kEstimateMaxBatch;
  const unsigned long long first = batch ? batch : std::min(pass, kEstimateFirstBatch);
  const size_t row = static_cast<size_t>(3 + N);
  const DevBuf d_partial(static_cast<size_t>(max_grid) * row * sizeof(double));
  std::vector<double> partial(static_cast<size_t>(max_grid) * row);
  if (records) out.records.reset(probes, N);
  const unsigned long long rec_cap = records ? std::min<unsigned long long>(probes, std::max(cap, first)) : 0;
  const DevBuf d_rest(rec_cap * sizeof(double)), d_rdep(rec_cap * sizeof(int)),
      d_rjob(rec_cap * static_cast<size_t>(N) * sizeof(int16_t));

  Stream stream;
  double s = 0, s2 = 0, dep = 0;
  std::vector<double> lvl(static_cast<size_t>(N), 0.0);
  unsigned long long done = 0, size = first;
  const auto t_all = std::chrono::steady_clock::now();
  while (done < probes) {
    const unsigned long long n = std::min(size, probes - done);
    const int grid = static_cast<int>(std::min<unsigned long long>(max_grid, (n + waves - 1) / waves));
    dev::EstParams a{};
    a.jobs = N;
    a.machines = M;
    a.pairs = lb2 ? P : 0;
    a.lb = lb;
    a.best = best;
    a.words = (N + 63) / 64;
    a.seed = seed;
    a.first_probe = first_probe + done;
    a.count = n;
    a.cum = d_cum.as<int>();
    a.tails = d_tails.as<int>();
    a.johnson = d_joh.as<uint16_t>();
    a.pair = d_pair.as<uint16_t>();
    a.pair_id = d_pid.as<uint16_t>();
    a.partial = d_partial.as<double>();
    if (records) {
      a.rec_est = d_rest.as<double>();
      a.rec_depth = d_rdep.as<int>();
      a.rec_jobs = d_rjob.as<int16_t>();
      TTS_HIP_CHECK(hipMemsetAsync(d_rjob.p, 0xff, n * static_cast<size_t>(N) * sizeof(int16_t), stream.s));
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (look)
      hipLaunchKernelGGL(look_kernel, dim3(grid), dim3(waves * dev::kWave), L.total, stream.s,
                         dev::LookParams{a, method.power});
    else
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(waves * dev::kWave), L.total, stream.s, a);
    TTS_HIP_CHECK(hipGetLastError());
    TTS_HIP_CHECK(hipMemcpyAsync(partial.data(), d_partial.p, static_cast<size_t>(grid) * row * sizeof(double),
                                 hipMemcpyDeviceToHost, stream.s));
    TTS_HIP_CHECK(hipStreamSynchronize(stream.s));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int b = 0; b < grid; ++b) {
      const double* r = &partial[static_cast<size_t>(b) * row];
      s += r[0];
      s2 += r[1];
      dep += r[2];
      for (int i = 0; i < N; ++i) lvl[i] += r[3 + i];
    }
    if (records) {
      TTS_HIP_CHECK(hipMemcpy(&out.records.est[done], d_rest.p, n * sizeof(double), hipMemcpyDeviceToHost));
      TTS_HIP_CHECK(hipMemcpy(&out.records.depth[done], d_rdep.p, n * sizeof(int), hipMemcpyDeviceToHost));
      TTS_HIP_CHECK(hipMemcpy(&out.records.chosen[static_cast<size_t>(done) * N], d_rjob.p,
                              n * static_cast<size_t>(N) * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    done += n;
    ++out.launches;
    if (!batch && out.launches == 1) {
      // size the later launches from this one's rate, up or down (its fixed costs make the
      // rate an underestimate, which errs towards shorter launches)
      out.rate = dt > 0 ? static_cast<double>(n) / dt : 0;
      out.first_seconds = dt;
      if (dt > kEstimateMaxLaunchSeconds && done < probes)
        throw std::invalid_argument("the device estimator's first launch, one probe per wave, took " +
                                    std::to_string(dt) + " s: no launch of this instance stays under " +
                                    std::to_string(kEstimateMaxLaunchSeconds) + " s; use the host twin");
      const double want = out.rate * kEstimateLaunchSeconds;
      size = want >= static_cast<double>(kEstimateMaxBatch) ? kEstimateMaxBatch
                                                            : std::max<unsigned long long>(1, static_cast<unsigned long long>(want));
    }
  }
  out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count();
  out.batch = size;
  out.est = finish_estimate(s, s2, dep, std::move(lvl), probes);
  return out;
}

}  // namespace tts
