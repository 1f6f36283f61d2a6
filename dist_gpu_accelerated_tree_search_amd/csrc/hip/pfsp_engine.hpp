// PFSP device engine: instance tables on the GPU + engine traits + factories.
//
// Parity: ref lb1_alloc_gpu / lb2_alloc_gpu (PFSP_gpu_lib.cu:154-200) deep-copy the
// bound tables once per GPU thread (and leak them). Here the tables
// are built once in the layout the kernels stage into LDS:
//   ptab  job-major u16 rows padded to 16 B        (LB1 / LB1_d / LB2 fronts)
//   recs  per machine pair, the Johnson order as {job, p0, p1, lag} u16 records,
//         so one wave-uniform 8-B read drives one Johnson step for 64 children.
// and are owned (freed) by the engine.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../core/pfsp_bounds_cpu.hpp"
#include "../core/pfsp_front.hpp"
#include "../core/pfsp_instance.hpp"
#include "engine.hpp"
#include "pfsp_front_kernels.hpp"
#include "pfsp_kernels.hpp"
#include "pool_bound_kernels.hpp"

namespace tts {

template <int NJ, int M, int LBK>
struct PfspTraits {
  using Node = PfspNode<NJ>;
  using Args = dev::PfspArgs<NJ, M>;
  using G = dev::PfspGeom<NJ, LBK, M>;
  static constexpr int kParentsPerChunk = G::BP;
  static constexpr int kChildrenPerChunk = G::SLOT;  // slot region per chunk
  static constexpr int kMaxChildren = NJ;            // children per parent (one level)
  static constexpr int kLocalSteps = G::LT;
  static constexpr int kLocalMin = 0;
  static constexpr int kMaxChunks = G::MAXCHUNKS;
  static void launch(const Args& a, int t, int grid, hipStream_t s) {
    hipLaunchKernelGGL((dev::pfsp_expand_kernel<NJ, M, LBK>), dim3(grid), dim3(dev::kBlock), 0, s, a, t);
  }
  static void flatten(const dev::PoolArgs<Node>& pa, int b, int grid, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_flatten_kernel<Node, G::SLOT, G::MAXCHUNKS>), dim3(grid), dim3(dev::kBlock), 0, s,
                       pa, b);
  }
  static void finalize(const dev::PoolArgs<Node>& pa, int b, int slot, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_finalize_kernel<Node, G::MAXCHUNKS>), dim3(1), dim3(dev::kBlock), 0, s, pa, b, slot);
  }
  // the bound of every ring node (pool_bound_kernels.hpp), for DeviceEngine::pool_bound
  static void pool_bound(const Args& a, dev::u64 bot, dev::u64 n, int cap, int bins, dev::u64* hist, int* lower,
                         hipStream_t s) {
    if constexpr (LBK >= 2)
      hipLaunchKernelGGL((dev::pool_bound_lb2_kernel<NJ, M>), dim3(dev::bound_blocks(n, dev::kBlock / dev::kWave)),
                         dim3(dev::kBlock), 0, s, a, bot, n, cap, bins, hist, lower);
    else
      hipLaunchKernelGGL((dev::pool_bound_lb1_kernel<NJ, M>), dim3(dev::bound_blocks(n, dev::kBlock)),
                         dim3(dev::kBlock), 0, s, a, bot, n, cap, bins, hist, lower);
  }
  static int blocks_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dev::pfsp_expand_kernel<NJ, M, LBK>, dev::kBlock, 0) !=
        hipSuccess)
      return 1;
    // 106 SGPRs: 6 resident per CU. The packed LB2 walks of 50+-job instances run on 3 of
    // their 4 (LDS-bound) resident workgroups: fewer walks contend for the record lines
    // (ta056 0.1748 -> 0.1773 G nodes/s, 2 per CU 0.1765; profiles/r5/grid_ab.txt)
    return dev::resident_blocks(n, (LBK == 5 && NJ >= 50) ? 3 : dev::kSgprResidentCap);
  }
};

// LB1 / LB1_d on front-carrying nodes (pfsp_front_kernels.hpp), machine bucket M.
template <int M, int NJ = 20>
struct PfspFrontTraits {
  using Node = PfspFrontNode<M, NJ>;
  using Args = dev::PfspFrontArgs<M, NJ>;
  using G = dev::FrontGeom<M, NJ>;
  static constexpr int kParentsPerChunk = G::BP;
  static constexpr int kChildrenPerChunk = G::SLOT;
  static constexpr int kMaxChildren = G::NJ;
  static constexpr int kLocalSteps = G::LT;
  // local DFS from 16K-parent windows: the wide levels of a 20-job tree take up to
  // local_steps levels per dependent kernel (ta014 -u 1, one MI355X: 0.234 -> 0.221 ms;
  // rank shares of 2/4/8-way splits 9-12 % faster; ta021 unchanged — its pool is a
  // backlog anyway; 4K-parent windows were slower again: profiles/r4/local_min.txt)
  static constexpr int kLocalMin = 16384;
  static constexpr int kMaxChunks = G::MAXCHUNKS;
  // dynamic local DFS iterations (front_dyn): not for the 100-job bucket (off by default,
  // measured slower everywhere; its donation protocol is not ported to the wider nodes)
  static constexpr bool kDyn = G::DYN;
  // Does a launch with these arguments need the instrumented instantiation (the dynamic
  // local DFS or a probe)? Everything else runs the production one.
  static bool instrumented(const Args& a) { return a.pool.dyn || a.dbg_rec || a.dbg_blk; }
  template <bool INSTR>
  static void launch_t(const Args& a, int t, int grid, hipStream_t s) {
    dev::FrontArgsT<M, NJ, INSTR> x;
    static_cast<Args&>(x) = a;
    hipLaunchKernelGGL((dev::pfsp_front_kernel<M, NJ, INSTR>), dim3(grid), dim3(dev::kBlock), 0, s, x, t);
  }
  static void launch_as(bool instr, const Args& a, int t, int grid, hipStream_t s) {
    if (instr) launch_t<true>(a, t, grid, s);
    else launch_t<false>(a, t, grid, s);
  }
  static void launch(const Args& a, int t, int grid, hipStream_t s) { launch_as(instrumented(a), a, t, grid, s); }
  static void flatten(const dev::PoolArgs<Node>& pa, int b, int grid, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_flatten_kernel<Node, G::SLOT, G::MAXCHUNKS>), dim3(grid), dim3(dev::kBlock), 0, s,
                       pa, b);
  }
  static void finalize(const dev::PoolArgs<Node>& pa, int b, int slot, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_finalize_kernel<Node, G::MAXCHUNKS>), dim3(1), dim3(dev::kBlock), 0, s, pa, b, slot);
  }
  // the bound of every ring node (pool_bound_kernels.hpp), for DeviceEngine::pool_bound
  static void pool_bound(const Args& a, dev::u64 bot, dev::u64 n, int cap, int bins, dev::u64* hist, int* lower,
                         hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_bound_front_kernel<M, NJ>), dim3(dev::bound_blocks(n, dev::kBlock)),
                       dim3(dev::kBlock), 0, s, a, bot, n, cap, bins, hist, lower);
  }
  static int blocks_per_cu() {
    // one grid serves both instantiations: what fits of either, capped as measured
    int n = 0, np = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dev::pfsp_front_kernel<M, NJ, true>, dev::kBlock, 0) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&np, dev::pfsp_front_kernel<M, NJ, false>, dev::kBlock, 0) !=
            hipSuccess)
      return 1;
    return std::min(std::min(n, np), G::GRID_WGS);  // FrontGeom::GRID_WGS (the API over-reports by one)
  }
};

// Front-layout tables: job-major u16 p rows padded to the LDS stride, padded tails.
template <int M, int NJ>
inline std::vector<uint16_t> pfsp_front_fill_args(const PfspInstance& in, dev::PfspFrontArgs<M, NJ>& a) {
  if (!pfsp_front_ok(in, 1) || pfsp_machine_bucket(in.machines) != M || pfsp_front_jobs(in.jobs) != NJ)
    throw std::invalid_argument("front layout does not apply to this instance");
  using G = dev::FrontGeom<M, NJ>;
  constexpr int MS = G::MS;
  const PfspPadded t = pfsp_padded_tables(in, M);
  // (buckets with a remain table: all NJ rows, then the table as the kernels hold it in LDS, FrontRemTab:
  // each 16-B vector of the rows as a column of its own, then the rows' remaining words)
  std::vector<uint16_t> ptab(G::RTAB ? static_cast<size_t>(NJ) * MS + static_cast<size_t>(G::TVEC) * 8
                                     : static_cast<size_t>(in.jobs) * MS,
                             0);
  for (int j = 0; j < in.jobs; ++j)
    for (int m = 0; m < in.machines; ++m) ptab[static_cast<size_t>(j) * MS + m] = static_cast<uint16_t>(in.pt(m, j));
  if constexpr (G::RTAB) {
    const std::vector<uint32_t> rows = pfsp_front_remain_table(in, M);  // [row][HW]
    std::vector<uint32_t> img(static_cast<size_t>(G::TVEC) * 4, 0u);
    for (int r = 0; r < G::TROWS; ++r)
      for (int h = 0; h < G::HW; ++h) {
        const size_t at = h < 4 * G::TQ ? (static_cast<size_t>(h / 4) * G::TROWS + r) * 4 + h % 4
                                        : static_cast<size_t>(G::TQ) * G::TROWS * 4 + static_cast<size_t>(r) * G::TR +
                                              (h - 4 * G::TQ);
        img[at] = rows[static_cast<size_t>(r) * G::HW + h];
      }
    std::memcpy(ptab.data() + static_cast<size_t>(NJ) * MS, img.data(), img.size() * sizeof(uint32_t));
  }
  a.jobs = in.jobs;
  for (int m = 0; m < M; ++m) a.min_tails[m] = t.tails[m];
  for (int h = 0; h < G::HW; ++h)
    a.tails2[h] = static_cast<uint32_t>(t.tails[2 * h]) | (2 * h + 1 < M ? static_cast<uint32_t>(t.tails[2 * h + 1]) << 16 : 0u);
  a.bpf = dev::FrontGeom<M, NJ>::BPF;
  a.cp_max = dev::FrontGeom<M, NJ>::CPMAX;
  if (const char* f = std::getenv("TTS_CP_MAX")) a.cp_max = std::max(0, std::atoi(f));  // A/B runs
  if (const char* f = std::getenv("TTS_FUSED_BPF"))  // A/B runs
    a.bpf = std::min(std::max(1, std::atoi(f)), dev::FrontGeom<M, NJ>::BPF_CP);
  return ptab;
}

// Host-side images of the device tables.
struct PfspTableImages {
  std::vector<uint16_t> ptab;  // [N][MS]
  std::vector<uint2> recs;     // [P][N]
  std::vector<uint2> pinfo;    // [P]
  std::vector<uint4> recs4;    // [P][rs4]: recs padded with zero records (lb2_walk_pipe)
  int rs4 = 0;
};

// Software-pipelined record loads in the LB2 walks (lb2_walk_pipe): on unless
// TTS_LB2_PIPE=0 (A/B).
inline int lb2_pipe_wanted() {
  const char* f = std::getenv("TTS_LB2_PIPE");
  return f ? (std::atoi(f) != 0) : 1;
}

// The LB2 kernel with two children per lane in packed u16 walks (LBK 5): every walk
// value must fit 16 bits (any job count: wide job sets read their words from LDS). A walk value (a child
// front, t0 + p0, t0 + lag, t1 + p1) is the length of a monotone staircase path
// through the machine x job grid (prefix columns, then Johnson-order columns; a lag
// is the column segment between the pair's machines), so it visits at most
// jobs + machines - 1 cells: (jobs + machines - 1) * max p bounds it (50 x 20 with
// p <= 99: 6,831). The tails are added in 32 bits after the walk. On when it applies
// unless TTS_LB2_PK=0 (A/B).
inline bool lb2_pk_ok(const PfspInstance& in) {
  long pmax = 0;
  for (int v : in.p) pmax = std::max<long>(pmax, v);
  return (in.jobs + in.machines - 1) * pmax < 65536;
}
inline bool lb2_pk_wanted(const PfspInstance& in) {
  const char* f = std::getenv("TTS_LB2_PK");
  return (f ? std::atoi(f) != 0 : true) && lb2_pk_ok(in);
}

// Strided LB2 chunks (parents ch + i * nchunks): on unless TTS_LB2_STRIDE=0 (A/B).
inline int lb2_stride_wanted() {
  const char* f = std::getenv("TTS_LB2_STRIDE");
  return f ? (std::atoi(f) != 0) : 1;
}

// Machine counts below the kernel's M are padded with trailing machines of zero
// processing time: the makespan, every LB1 machine term and the fronts of the real
// machines are unchanged (a zero machine after the last one completes with it), and
// LB2 walks only the instance's own pairs (npairs), so the bounds equal the host
// oracle's for the real instance.
//
// Accepted values: every processing time, machine column sum (the remain half of the
// LDS words), LB2 lag and tail must fit 16 bits. `u16_fronts` is set by the callers whose
// kernels also keep prefix completion times in 16 bits (the LB2 kernels: the front half
// of `front | remain << 16`, the u16 child fronts); those take only instances with
// pfsp_fronts_fit_u16. The LB1 / LB1_d kernels hold fronts in 32-bit registers
// (pfsp_lb1_parent) and need the table checks alone.
template <int NJ, int M>
inline PfspTableImages pfsp_fill_args(const PfspInstance& in, dev::PfspArgs<NJ, M>& a, bool pair_order,
                                      bool u16_fronts) {
  using C = dev::PfspConsts<M>;
  if (in.machines > M || in.machines < 1) throw std::invalid_argument("machine count exceeds kernel instantiation");
  if (in.jobs > NJ) throw std::invalid_argument("job count exceeds kernel bucket");
  for (int v : in.p)
    if (v < 0 || v > 0xffff) throw std::invalid_argument("processing time does not fit 16 bits");
  if (u16_fronts && !pfsp_fronts_fit_u16(in))
    throw std::invalid_argument("instance too large for 16-bit fronts: (jobs + machines - 1) * max p >= 65536");
  const int MR = in.machines;
  const int PR = MR * (MR - 1) / 2;
  PfspTableImages img;
  img.ptab.assign(static_cast<size_t>(in.jobs) * C::MS, 0);
  for (int j = 0; j < in.jobs; ++j)
    for (int m = 0; m < MR; ++m) img.ptab[static_cast<size_t>(j) * C::MS + m] = static_cast<uint16_t>(in.pt(m, j));
  img.recs.resize(static_cast<size_t>(PR) * in.jobs);
  for (int q = 0; q < PR; ++q) {
    const int m0 = in.pair_m0[q], m1 = in.pair_m1[q];
    for (int r = 0; r < in.jobs; ++r) {
      const int job = in.johnson[static_cast<size_t>(q) * in.jobs + r];
      const int lag = in.lags[static_cast<size_t>(q) * in.jobs + job];
      if (lag > 0xffff) throw std::invalid_argument("LB2 lag does not fit 16 bits");
      uint2 rc;
      rc.x = static_cast<uint32_t>(job) | (static_cast<uint32_t>(in.pt(m0, job)) << 16);
      rc.y = static_cast<uint32_t>(in.pt(m1, job)) | (static_cast<uint32_t>(lag) << 16);
      img.recs[static_cast<size_t>(q) * in.jobs + r] = rc;
    }
  }
  {
    const int ndouble = (in.jobs + 7) / 8;
    img.rs4 = 4 * ndouble + 4;  // walks of ndouble x 8 records + one double group of prefetch
    img.recs4.assign(static_cast<size_t>(PR) * img.rs4, make_uint4(0, 0, 0, 0));
    for (int q = 0; q < PR; ++q)
      for (int r = 0; r < in.jobs; ++r) {
        const uint2 rc = img.recs[static_cast<size_t>(q) * in.jobs + r];
        uint4& v = img.recs4[static_cast<size_t>(q) * img.rs4 + r / 2];
        if (r & 1) {
          v.z = rc.x;
          v.w = rc.y;
        } else {
          v.x = rc.x;
          v.y = rc.y;
        }
      }
  }
  // expand kernel's pair table in the learned early-exit order (lb2_pair_order);
  // recs stay in the reference order (the bounds kernel keeps its exact partial
  // values) and pinfo points each slot at its pair's records
  img.pinfo.resize(PR);
  {
    std::vector<int> ord(PR);
    for (int q = 0; q < PR; ++q) ord[q] = q;
    if (pair_order && PR > 0) ord = lb2_pair_order(in);
    for (int i = 0; i < PR; ++i) {
      const int q = ord[i];
      const int m0 = in.pair_m0[q], m1 = in.pair_m1[q];
      if (in.min_tails[m0] > 0xffff || in.min_tails[m1] > 0xffff)
        throw std::invalid_argument("LB2 tail does not fit 16 bits");
      img.pinfo[i].x = static_cast<uint32_t>(m0) | (static_cast<uint32_t>(m1) << 8) | (static_cast<uint32_t>(q) << 16);
      img.pinfo[i].y = static_cast<uint32_t>(in.min_tails[m0]) | (static_cast<uint32_t>(in.min_tails[m1]) << 16);
    }
  }
  a.jobs = in.jobs;
  a.npairs = PR;
  a.rs4 = img.rs4;
  a.lb2_pipe = lb2_pipe_wanted();
  a.lb2_stride = lb2_stride_wanted();
  for (int m = 0; m < M; ++m) {
    if (m < MR) {
      a.min_heads[m] = in.min_heads[m];
      a.min_tails[m] = in.min_tails[m];
    } else {  // padding machine: head = whole real route of the cheapest job, no tail
      int h = INT_MAX;
      for (int j = 0; j < in.jobs; ++j) {
        int t = 0;
        for (int k = 0; k < MR; ++k) t += in.pt(k, j);
        h = std::min(h, t);
      }
      a.min_heads[m] = h;
      a.min_tails[m] = 0;
    }
    long s = 0;
    if (m < MR)
      for (int j = 0; j < in.jobs; ++j) s += in.pt(m, j);
    // front and remain are packed as two u16 per machine in LDS
    if (s > 0xffff) throw std::invalid_argument("instance too large for 16-bit schedule packing");
    a.sum_all[m] = static_cast<int>(s);
  }
  for (int q = 0; q < PR; ++q) {
    a.pm0[q] = static_cast<uint8_t>(in.pair_m0[q]);
    a.pm1[q] = static_cast<uint8_t>(in.pair_m1[q]);
  }
  return img;
}

template <class T>
inline T* upload_vec(const std::vector<T>& v) {
  T* d = nullptr;
  TTS_HIP_CHECK(hipMalloc(&d, std::max<size_t>(1, v.size()) * sizeof(T)));
  if (!v.empty()) TTS_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

template <int NJ, int M, int LBK>
std::unique_ptr<IEngine> make_pfsp_engine_t(const PfspInstance& in, const EngineConfig& cfg) {
  TTS_HIP_CHECK(hipSetDevice(cfg.device));
  dev::PfspArgs<NJ, M> a{};
  const PfspTableImages img = pfsp_fill_args(in, a, LBK >= 2, LBK >= 2);
  a.ptab = upload_vec(img.ptab);
  a.recs = upload_vec(img.recs);
  a.pinfo = upload_vec(img.pinfo);
  a.recs4 = upload_vec(img.recs4);
  // B2 in rounds of pairs: ta056 (50x20) 0.060 -> 0.081 G nodes/s, ta020 (20x10)
  // 11.1 -> 8.0 ms, ta014 (20x10) even; ta010 (20x5, 10 pairs) 4.0 -> 4.6 ms
  // (profiles/r1/r1ak): on from 10 machines (45 pairs)
  a.lb2_rounds = M >= 10 ? 1 : 0;
  if (const char* f = std::getenv("TTS_LB2_ROUNDS")) a.lb2_rounds = std::atoi(f) != 0;  // A/B runs
  auto eng = std::make_unique<DeviceEngine<PfspTraits<NJ, M, LBK>>>(cfg, a);
  {  // the host twin of the node bound (spilled nodes): its own copy of the instance
    auto own = std::make_shared<const PfspInstance>(in);
    eng->set_host_node_bound([own, prob = PfspProblem<NJ>(*own, LBK >= 2 ? 2 : 1)](const PfspNode<NJ>& n, int cap) {
      return prob.node_bound(n, cap);
    });
  }
  eng->adopt(const_cast<uint16_t*>(a.ptab));
  eng->adopt(const_cast<uint2*>(a.recs));
  eng->adopt(const_cast<uint2*>(a.pinfo));
  eng->adopt(const_cast<uint4*>(a.recs4));
  return eng;
}

template <int M, int NJ = 20>
std::unique_ptr<IEngine> make_pfsp_front_engine_t(const PfspInstance& in, const EngineConfig& cfg) {
  TTS_HIP_CHECK(hipSetDevice(cfg.device));
  dev::PfspFrontArgs<M, NJ> a{};
  const std::vector<uint16_t> ptab = pfsp_front_fill_args(in, a);
  a.ptab = upload_vec(ptab);
  auto eng = std::make_unique<DeviceEngine<PfspFrontTraits<M, NJ>>>(cfg, a);
  {  // the host twin of the node bound (spilled nodes): its own copy of the instance
    auto own = std::make_shared<const PfspInstance>(in);
    auto prob = std::make_shared<const PfspFrontProblem<M, NJ>>(*own, 1);
    eng->set_host_node_bound([own, prob](const PfspFrontNode<M, NJ>& n, int cap) { return prob->node_bound(n, cap); });
  }
  eng->adopt(const_cast<uint16_t*>(a.ptab));
  return eng;
}

// Kernel machine bucket: 5, 10 or 20 (Taillard's counts); other counts up to 20 run
// in the next bucket with zero-time padding machines (pfsp_fill_args).
template <class F>
decltype(auto) with_machine_bucket(int machines, F&& f) {
  if (machines >= 1 && machines <= 5) return f(std::integral_constant<int, 5>{});
  if (machines > 5 && machines <= 10) return f(std::integral_constant<int, 10>{});
  if (machines > 10 && machines <= 20) return f(std::integral_constant<int, 20>{});
  throw std::invalid_argument("GPU kernels support 1 to 20 machines");
}

}  // namespace tts

#include "pfsp_probes.hpp"  // the probes: they use everything above

namespace tts {

// ---- run-time dispatch (pfsp_engine_dispatch.hip; per bucket in pfsp_engine_nj*.hip) ----
std::unique_ptr<IEngine> make_pfsp_engine(const PfspInstance& in, int lb, const EngineConfig& cfg);
std::vector<int> pfsp_gpu_bounds(const PfspInstance& in, int lb, const void* parents, size_t n, int best, int device);
std::vector<int> pfsp_expand_probe(const PfspInstance& in, int lb, const void* parents, size_t n, int best, int device,
                                   int variant, int reps = 0, std::vector<double>* timing = nullptr,
                                   ExpandProbeResult* extra = nullptr);
ExpandProbeResult pfsp_lb1_expand_probe(const PfspInstance& in, const void* parents, size_t n, int best, int device);
// front-layout instances only (pfsp_front_ok): the 20- to 500-job front buckets
std::vector<double> pfsp_front_time(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                    const EngineConfig& cfg, int reps);
FrontProbeResult pfsp_front_probe(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                  const EngineConfig& cfg, unsigned cap, int split_rank = 0, int split_world = 1,
                                  size_t split_min = 0);
FrontExpandResult pfsp_front_expand_probe(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, int steps,
                                          int device, bool production = false);

#define TTS_PFSP_DECLARE_BUCKET(NJ)                                                                   \
  std::unique_ptr<IEngine> make_pfsp_engine_nj##NJ(const PfspInstance& in, int lb, const EngineConfig& cfg); \
  std::vector<int> pfsp_gpu_bounds_nj##NJ(const PfspInstance& in, int lb, const void* parents, size_t n, int best, \
                                          int device);                                                \
  std::vector<int> pfsp_expand_probe_nj##NJ(const PfspInstance& in, int lb, const void* parents, size_t n, int best, \
                                            int device, int variant, int reps, std::vector<double>* timing, \
                                            ExpandProbeResult* extra); \
  ExpandProbeResult pfsp_lb1_expand_probe_nj##NJ(const PfspInstance& in, const void* parents, size_t n, int best, int device);
TTS_PFSP_DECLARE_BUCKET(20)
TTS_PFSP_DECLARE_BUCKET(50)
TTS_PFSP_DECLARE_BUCKET(100)
TTS_PFSP_DECLARE_BUCKET(200)
TTS_PFSP_DECLARE_BUCKET(500)

#define TTS_PFSP_DECLARE_FRONT_BUCKET(NJ)                                                              \
  FrontProbeResult pfsp_front_probe_nj##NJ(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, \
                                           const EngineConfig& cfg, unsigned cap, int split_rank, int split_world, \
                                           size_t split_min);                                          \
  std::vector<double> pfsp_front_time_nj##NJ(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, \
                                             const EngineConfig& cfg, int reps);                       \
  FrontExpandResult pfsp_front_expand_probe_nj##NJ(const PfspInstance& in, const void* nodes, size_t n, int best, \
                                                   int steps, int device, bool production);
TTS_PFSP_DECLARE_FRONT_BUCKET(20)
TTS_PFSP_DECLARE_FRONT_BUCKET(50)
TTS_PFSP_DECLARE_FRONT_BUCKET(100)
TTS_PFSP_DECLARE_FRONT_BUCKET(200)
TTS_PFSP_DECLARE_FRONT_BUCKET(500)

// Body of one bucket's TU: machine buckets (with_machine_bucket), LB kernels 1 (LB1
// and LB1_d) / 2.
#define TTS_PFSP_DEFINE_BUCKET(NJ)                                                                     \
  std::unique_ptr<IEngine> make_pfsp_engine_nj##NJ(const PfspInstance& in, int lb, const EngineConfig& cfg) { \
    return with_machine_bucket(in.machines, [&](auto mm) -> std::unique_ptr<IEngine> {               \
      constexpr int M = decltype(mm)::value;                                                         \
      /* (every job bucket has a front layout: 200 and 500 under TTS_FRONT_WIDE=2) */                \
        if (pfsp_front_ok(in, lb)) return make_pfsp_front_engine_t<M, NJ>(in, cfg);                  \
      if (lb != 2) return make_pfsp_engine_t<NJ, M, 1>(in, cfg);                                    \
      if (M >= 10 && lb2_pk_wanted(in)) return make_pfsp_engine_t<NJ, M, 5>(in, cfg);                 \
      return make_pfsp_engine_t<NJ, M, 2>(in, cfg);                                                  \
    });                                                                                              \
  }                                                                                                  \
  std::vector<int> pfsp_gpu_bounds_nj##NJ(const PfspInstance& in, int lb, const void* parents, size_t n, int best, \
                                          int device) {                                              \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      constexpr int M = decltype(mm)::value;                                                         \
      /* (every job bucket has a front layout: 200 and 500 under TTS_FRONT_WIDE=2) */                \
        if (pfsp_front_ok(in, lb))                                                                   \
          return pfsp_front_bounds_t<M, NJ>(in, static_cast<const PfspNode<NJ>*>(parents), n, device); \
      return lb == 2 ? pfsp_gpu_bounds_t<NJ, M, 2>(in, parents, n, best, device)                    \
                     : pfsp_gpu_bounds_t<NJ, M, 1>(in, parents, n, best, device);                   \
    });                                                                                              \
  }                                                                                                  \
  std::vector<int> pfsp_expand_probe_nj##NJ(const PfspInstance& in, int lb, const void* parents, size_t n, int best, \
                                            int device, int variant, int reps, std::vector<double>* timing, \
                                            ExpandProbeResult* extra) {                                     \
    if (lb != 2) throw std::invalid_argument("expand probe: LB2 only");                             \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      constexpr int M = decltype(mm)::value;                                                         \
      return pfsp_expand_probe_t<NJ, M, 2>(in, parents, n, best, device, variant, reps, timing, extra); \
    });                                                                                              \
  }                                                                                                  \
  ExpandProbeResult pfsp_lb1_expand_probe_nj##NJ(const PfspInstance& in, const void* parents, size_t n, int best, \
                                              int device) {                                          \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      constexpr int M = decltype(mm)::value;                                                         \
      return pfsp_lb1_expand_probe_t<NJ, M>(in, parents, n, best, device);                           \
    });                                                                                              \
  }

// The front probes of one front bucket (20 to 500 jobs), after TTS_PFSP_DEFINE_BUCKET
// in its TU.
#define TTS_PFSP_DEFINE_FRONT_BUCKET(NJ)                                                               \
  FrontProbeResult pfsp_front_probe_nj##NJ(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, \
                                           const EngineConfig& cfg, unsigned cap, int split_rank, int split_world, \
                                           size_t split_min) {                                         \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      return pfsp_front_probe_t<decltype(mm)::value, NJ>(in, lb, nodes, n, best, cfg, cap, split_rank, split_world, \
                                                         split_min);                                 \
    });                                                                                              \
  }                                                                                                  \
  std::vector<double> pfsp_front_time_nj##NJ(const PfspInstance& in, int lb, const void* nodes, size_t n, int best, \
                                             const EngineConfig& cfg, int reps) {                      \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      return pfsp_front_time_t<decltype(mm)::value, NJ>(in, lb, nodes, n, best, cfg, reps);          \
    });                                                                                              \
  }                                                                                                  \
  FrontExpandResult pfsp_front_expand_probe_nj##NJ(const PfspInstance& in, const void* nodes, size_t n, int best, \
                                                   int steps, int device, bool production) {           \
    return with_machine_bucket(in.machines, [&](auto mm) {                                           \
      return pfsp_front_expand_probe_t<decltype(mm)::value, NJ>(in, nodes, n, best, steps, device, production); \
    });                                                                                              \
  }

}  // namespace tts
