// PFSP probes (tests, scripts): batch bound evaluation and one-iteration probes of the
// production kernels, built on the probe fixture (probe_pool.hpp). Included by
// pfsp_engine.hpp after the traits and table builders it uses; instantiated in the
// per-bucket TUs (TTS_PFSP_DEFINE_BUCKET / TTS_PFSP_DEFINE_FRONT_BUCKET).
#pragma once

#include "probe_pool.hpp"

namespace tts {

// Reference-style batch evaluation on the GPU (host arrays in and out):
// bounds of every child of every parent, in parent order, children k = depth..N-1.
template <int NJ, int M, int LBK>
std::vector<int> pfsp_gpu_bounds_t(const PfspInstance& in, const void* parents, size_t n, int best, int device) {
  using Node = PfspNode<NJ>;
  TTS_HIP_CHECK(hipSetDevice(device));
  dev::PfspArgs<NJ, M> a{};
  const PfspTableImages img = pfsp_fill_args(in, a, false, LBK == 2);
  const Node* ph = static_cast<const Node*>(parents);
  const std::vector<int> offsets = perm_child_offsets(ph, n, in.jobs);
  const size_t nb = static_cast<size_t>(offsets[n]);
  std::vector<int> out(nb, 0);
  if (n == 0) return out;
  ProbeAllocs mem;
  a.ptab = mem.upload(img.ptab);
  a.recs = mem.upload(img.recs);
  a.offsets = mem.upload(offsets);
  a.parents_in = mem.upload(ph, n);
  a.bounds_out = mem.alloc<int>(nb);
  a.nparents = static_cast<int>(n);
  a.best_in = best;
  constexpr int BP = dev::PfspGeom<NJ, LBK, M>::BP;
  const int nchunks = static_cast<int>((n + BP - 1) / BP);
  hipLaunchKernelGGL((dev::pfsp_bounds_kernel<NJ, M, LBK>), dim3(std::min(nchunks, 2048)), dim3(dev::kBlock), 0, 0, a);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  TTS_HIP_CHECK(hipMemcpy(out.data(), a.bounds_out, nb * sizeof(int), hipMemcpyDeviceToHost));
  return out;
}

// Output of the expand probes beyond the bounds: the children an iteration wrote (chunk
// order), the leaves it counted and the incumbent after it.
struct ExpandProbeResult {
  std::vector<int> bounds;
  std::vector<uint8_t> children;
  long long leaves = 0;
  int best = 0;
  // from the pool after the launch (PFSP leaf words: leaves in the low half)
  template <class Node>
  void read(const ProbePool<Node>& pool, size_t nchunks, const char* who) {
    ProbeChunks ch = pool.read_chunks(nchunks, who);
    children = std::move(ch.children);
    leaves = 0;
    for (int w : ch.lwords) leaves += w & 0xffff;
    best = pool.ctl().best.v;
  }
};

// Element-wise probe of the production expand kernel (LB2 only): ONE iteration
// over `n` parents loaded as the window, with the kernel's debug output on. Returns
// every child's bound in parent order (children k = depth..N-1): the exact LB2 when
// it is below `best`, otherwise a value >= best (the kernel's prune decision).
// variant: 1 rounds of dense walks, 2 dense walks, 4 rounds of packed two-child walks
// (kernel LBK 5, the default search path where lb2_pk_ok).
// With `timing`: `reps` more launches without the debug output, each from the same
// window (ring and control block restored), on the engine's grid (resident
// workgroups), then one launch with the phase timers; timing = {min ms, median ms,
// phase A, B1, B2, B3+C shader clocks per chunk, chunks}.
template <int NJ, int M, int LBK>
std::vector<int> pfsp_expand_probe_t(const PfspInstance& in, const void* parents, size_t n, int best, int device,
                                     int variant, int reps = 0, std::vector<double>* timing = nullptr,
                                     ExpandProbeResult* extra = nullptr) {
  using Node = PfspNode<NJ>;
  using G = dev::PfspGeom<NJ, LBK, M>;
  if constexpr (LBK != 2) {
    throw std::invalid_argument("expand probe: LB2 kernels only");
  } else {
    TTS_HIP_CHECK(hipSetDevice(device));
    const std::vector<int> offsets = perm_child_offsets(static_cast<const Node*>(parents), n, in.jobs);
    const size_t nb = static_cast<size_t>(offsets[n]);
    std::vector<int> out(nb, -1);
    if (n == 0) return out;
    const size_t nchunks = (n + G::BP - 1) / G::BP;
    if (nchunks > static_cast<size_t>(G::MAXCHUNKS)) throw std::invalid_argument("expand probe: too many parents");
    dev::PfspArgs<NJ, M> a{};
    const PfspTableImages img = pfsp_fill_args(in, a, true, true);
    if (variant != 1 && variant != 2 && variant != 4) throw std::invalid_argument("expand probe: variant 1, 2 or 4");
    if (variant == 4 && !lb2_pk_ok(in)) throw std::invalid_argument("expand probe: packed walks do not apply");
    ProbeAllocs mem;
    a.ptab = mem.upload(img.ptab);
    a.recs = mem.upload(img.recs);
    a.pinfo = mem.upload(img.pinfo);
    a.recs4 = mem.upload(img.recs4);
    a.dbg_off = mem.upload(offsets);
    a.dbg_lb = mem.upload(out);
    a.lb2_rounds = variant == 1 || variant == 4;
    dev::PoolCtl h{};
    h.best.v = best;
    const ProbePool<Node> pool(mem, a.pool, parents, n, nchunks, G::SLOT, G::BP, h);
    auto launch = [&](const dim3& grid) {
      if (variant == 4)
        hipLaunchKernelGGL((dev::pfsp_expand_kernel<NJ, M, 5>), grid, dim3(dev::kBlock), 0, 0, a, 0);
      else
        hipLaunchKernelGGL((dev::pfsp_expand_kernel<NJ, M, LBK>), grid, dim3(dev::kBlock), 0, 0, a, 0);
      TTS_HIP_CHECK(hipGetLastError());
    };
    launch(dim3(static_cast<unsigned>(std::min<size_t>(nchunks, 1024))));
    TTS_HIP_CHECK(hipDeviceSynchronize());
    TTS_HIP_CHECK(hipMemcpy(out.data(), a.dbg_lb, nb * sizeof(int), hipMemcpyDeviceToHost));
    if (extra) extra->read(pool, nchunks, "expand probe");
    if (timing) {
      int bpc = 0, cus = 0;
      if (variant == 4)
        TTS_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, dev::pfsp_expand_kernel<NJ, M, 5>,
                                                                   dev::kBlock, 0));
      else
        TTS_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, dev::pfsp_expand_kernel<NJ, M, LBK>,
                                                                   dev::kBlock, 0));
      TTS_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
      const dim3 grid(static_cast<unsigned>(std::min<size_t>(nchunks, static_cast<size_t>(std::max(1, bpc * cus)))));
      a.dbg_lb = nullptr;
      const std::vector<double> ms = time_launches(reps, [&] { pool.restore(); }, [&] { launch(grid); });
      pool.restore();
      a.dbg_time = mem.zeroed<unsigned long long>(8);
      launch(grid);
      TTS_HIP_CHECK(hipDeviceSynchronize());
      unsigned long long tm[8] = {};
      TTS_HIP_CHECK(hipMemcpy(tm, a.dbg_time, sizeof(tm), hipMemcpyDeviceToHost));
      // workgroup timeline, from its own launch (no phase timers)
      pool.restore();
      a.dbg_time = nullptr;
      a.dbg_blk = mem.zeroed<unsigned long long>(3 * grid.x);
      launch(grid);
      TTS_HIP_CHECK(hipDeviceSynchronize());
      std::vector<unsigned long long> blk(3 * grid.x);
      TTS_HIP_CHECK(hipMemcpy(blk.data(), a.dbg_blk, blk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      const StampClock us(blk, 3, device);
      const double nc = static_cast<double>(std::max<unsigned long long>(1, tm[4]));
      *timing = {ms.front(), ms[ms.size() / 2], tm[0] / nc, tm[1] / nc, tm[2] / nc, tm[3] / nc, nc,
                 static_cast<double>(tm[5]), static_cast<double>(tm[6]) / std::max<unsigned long long>(1, tm[7]),
                 static_cast<double>(grid.x)};
      for (unsigned long long x : blk) timing->push_back(us(x));
    }
    return out;
  }
}

// Element-wise probe of the permutation-node LB1 / LB1_d expand kernel (instances of
// more than 50 jobs; 20 / 50 jobs under TTS_FRONT=0): ONE iteration over `n` parents
// loaded as the window. Returns every child's bound (parent order, children
// k = depth..N-1), the children the kernel wrote (chunk order; lb < best, the leaves of
// depth N-1 parents excluded), the leaves it counted and the incumbent after the launch.
template <int NJ, int M>
ExpandProbeResult pfsp_lb1_expand_probe_t(const PfspInstance& in, const void* parents, size_t n, int best, int device) {
  using Node = PfspNode<NJ>;
  using G = dev::PfspGeom<NJ, 1, M>;
  TTS_HIP_CHECK(hipSetDevice(device));
  const Node* ph = static_cast<const Node*>(parents);
  ExpandProbeResult res;
  for (size_t i = 0; i < n; ++i)
    if (ph[i].depth >= in.jobs) throw std::invalid_argument("lb1 expand probe: parents must have children");
  const std::vector<int> offsets = perm_child_offsets(ph, n, in.jobs);
  res.bounds.assign(static_cast<size_t>(offsets[n]), -1);
  res.best = best;
  if (n == 0) return res;
  const size_t nchunks = (n + G::BP - 1) / G::BP;
  if (nchunks > static_cast<size_t>(G::MAXCHUNKS)) throw std::invalid_argument("lb1 expand probe: too many parents");
  dev::PfspArgs<NJ, M> a{};
  const PfspTableImages img = pfsp_fill_args(in, a, false, false);
  ProbeAllocs mem;
  a.ptab = mem.upload(img.ptab);
  a.dbg_off = mem.upload(offsets);
  a.dbg_lb = mem.upload(res.bounds);
  dev::PoolCtl h{};
  h.best.v = best;
  const ProbePool<Node> pool(mem, a.pool, parents, n, nchunks, G::SLOT, G::BP, h);
  hipLaunchKernelGGL((dev::pfsp_expand_kernel<NJ, M, 1>), dim3(static_cast<unsigned>(std::min<size_t>(nchunks, 1024))),
                     dim3(dev::kBlock), 0, 0, a, 0);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  TTS_HIP_CHECK(hipMemcpy(res.bounds.data(), a.dbg_lb, res.bounds.size() * sizeof(int), hipMemcpyDeviceToHost));
  res.read(pool, nchunks, "lb1 expand probe");
  return res;
}

// Element-wise probe of the production LB1 / LB1_d front kernel (tests):
// a complete engine solve from `nodes` (front layout) with the kernel's probe records
// on, so every iteration shape the solve takes — one level per kernel, the split
// iteration, multi-level chunks (child-parallel and thread-per-node levels with carried
// remains), local DFS — records each child it bounds: the parent's words, the parent's
// remain as the kernel holds it, the job and the bound. Every record is checked here
// against the host oracle (PfspFrontProblem: ref add_front_and_bound,
// c_bound_simple.c:219-244). At most `cap` records are kept and checked; the count of
// all records is returned too.
struct FrontProbeResult {
  unsigned long long records = 0, checked = 0;
  unsigned long long by_kind[6] = {};
  unsigned long long bad_lb = 0, bad_remain = 0, bad_job = 0;
  EngineStats st;
  std::vector<uint32_t> first_bad;
};
template <int M, int NJ = 20>
FrontProbeResult pfsp_front_probe_t(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                    const EngineConfig& cfg, unsigned cap, int split_rank, int split_world,
                                    size_t split_min) {
  using G = dev::FrontGeom<M, NJ>;
  using Node = PfspFrontNode<M, NJ>;
  TTS_HIP_CHECK(hipSetDevice(cfg.device));
  const PfspFrontProblem<M, NJ> prob(in, lb);
  dev::PfspFrontArgs<M, NJ> a{};
  const std::vector<uint16_t> ptab = pfsp_front_fill_args(in, a);
  FrontProbeResult res;
  std::vector<uint32_t> rec;
  {
    ProbeAllocs mem;
    a.ptab = mem.upload(ptab);
    a.dbg_rec = mem.alloc<uint32_t>(std::max<size_t>(1, cap) * G::DBGW);
    a.dbg_n = mem.zeroed<unsigned>(1);
    a.dbg_cap = cap;
    {
      DeviceEngine<PfspFrontTraits<M, NJ>> eng(cfg, a);
      if (split_world > 1) eng.set_split(split_rank, split_world, split_min);
      res.st = eng.solve_from(nodes, n, best);
    }
    unsigned total = 0;
    TTS_HIP_CHECK(hipMemcpy(&total, a.dbg_n, sizeof(unsigned), hipMemcpyDeviceToHost));
    res.records = total;
    res.checked = std::min<size_t>(total, cap);
    rec.resize(res.checked * G::DBGW);
    if (res.checked)
      TTS_HIP_CHECK(hipMemcpy(rec.data(), a.dbg_rec, rec.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < res.checked; ++i) {
    const uint32_t* r = &rec[i * G::DBGW];
    // (job | kind << KS: the kind above 8 job bits up to 100 jobs, above 16 in the wider buckets)
    const int j = static_cast<int>(r[0] & ((1u << G::KS) - 1u)), kind = static_cast<int>((r[0] >> G::KS) & 0xffu);
    if (kind < 6) ++res.by_kind[kind];
    Node parent;
    std::memcpy(&parent, r + 2, sizeof(Node));
    bool bad = false;
    if (j >= NJ || !mask_test(parent.rest, j)) {
      ++res.bad_job;
      bad = true;
    } else {
      int rt[M];
      prob.remain_tail(parent, rt);
      for (int m = 0; m < M; ++m) {
        const int got = static_cast<int>((r[2 + G::NW + (m >> 1)] >> ((m & 1) * 16)) & 0xffffu);
        if (got != rt[m] - prob.tab.tails[m]) {
          ++res.bad_remain;
          bad = true;
          break;
        }
      }
      if (prob.child(parent, rt, j, nullptr) != static_cast<int>(r[1])) {
        ++res.bad_lb;
        bad = true;
      }
    }
    if (bad && res.first_bad.empty()) res.first_bad.assign(r, r + G::DBGW);
  }
  return res;
}

// What ONE front-kernel iteration wrote (tests): the children of each output chunk in the
// order the kernel laid them out, chunk after chunk. The bounds probe above checks what
// the kernel evaluates, this one what it emits.
//   steps == 0: one level per kernel — chunk c holds the survivors of parents
//               [c * 256, (c + 1) * 256) in parent order, jobs ascending;
//   steps >= 1: local DFS of up to `steps` steps — chunk c starts from parents
//               [c * bp, (c + 1) * bp) and holds the stack it left (after one step: its
//               parents' survivors, in the same order); inner[c] counts the nodes it
//               pushed and expanded itself.
// production: launch the production instantiation of the kernel (pfsp_front_kernel INSTR
// false) instead of the instrumented one.
struct FrontExpandResult {
  std::vector<uint8_t> children;  // node bytes, chunks back to back
  std::vector<int> counts;        // nodes per chunk
  std::vector<int> inner;         // per chunk: pushed - left on the stack (local DFS)
  int bp = 0;                     // window parents per chunk
  unsigned long long leaves = 0;
  int best = 0;
};
template <int M, int NJ = 20>
FrontExpandResult pfsp_front_expand_probe_t(const PfspInstance& in, const void* nodes, size_t n, int best, int steps,
                                            int device, bool production = false) {
  using G = dev::FrontGeom<M, NJ>;
  using Node = PfspFrontNode<M, NJ>;
  if (steps < 0 || steps > G::LT) throw std::invalid_argument("front expand probe: 0 (one level) to LT local steps");
  TTS_HIP_CHECK(hipSetDevice(device));
  FrontExpandResult res;
  res.best = best;
  if (n == 0) return res;
  const size_t nchunks = (n + G::BP - 1) / G::BP;
  if (nchunks > static_cast<size_t>(G::MAXCHUNKS)) throw std::invalid_argument("front expand probe: too many parents");
  dev::PfspFrontArgs<M, NJ> a{};
  const std::vector<uint16_t> ptab = pfsp_front_fill_args(in, a);
  ProbeAllocs mem;
  a.ptab = mem.upload(ptab);
  dev::PoolCtl h{};
  h.best.v = best;
  h.best0 = best;
  const ProbePool<Node> pool(mem, a.pool, nodes, n, nchunks, G::SLOT, G::BP, h);
  // the requested shape only: no fused / wide multi-level chunks, no dynamic DFS; a local
  // window whatever the pool holds (the forced form of local_steps: a single step too)
  a.pool.local_steps = -steps;
  a.pool.local_min = 1;
  const unsigned grid = static_cast<unsigned>(nchunks);
  // (the instrumented instantiation unless the production one is asked for: the launch
  // sets no probe pointer, so the two must write the same bytes)
  PfspFrontTraits<M, NJ>::launch_as(!production, a, 0, static_cast<int>(grid), 0);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  // the chunks the iteration dealt: one per 256 parents, or the window spread over the grid
  res.bp = steps == 0 ? G::BP : static_cast<int>(std::min<size_t>(G::BP, (n + grid - 1) / grid));
  const size_t nout = (n + res.bp - 1) / res.bp;
  if (nout > nchunks) throw std::runtime_error("front expand probe: more chunks than workgroups");
  ProbeChunks ch = pool.read_chunks(nout, "front expand probe");
  res.children = std::move(ch.children);
  res.counts = std::move(ch.counts);
  for (int w : ch.lwords) {  // the per-chunk leaf word: leaves in the low half, inner nodes in the high half
    res.leaves += static_cast<uint32_t>(w) & 0xffffu;
    res.inner.push_back(static_cast<int>(static_cast<uint32_t>(w) >> 16));
  }
  const dev::PoolCtl after = pool.ctl();
  if (after.overflow) throw std::runtime_error("front expand probe: the iteration reported an overflow");
  res.best = after.best.v;
  return res;
}

// Timing probe of ONE front-kernel iteration over a given window (the nodes loaded as
// the pool), on the engine's grid: `reps` launches from the same state (min / median
// ms), then one launch with the per-workgroup phase stamps (front_stamp). Returns
// {ms_min, ms_median, grid, iteration levels, then grid x 16 stamps in us from the first
// workgroup entry (0 where a stamp was not reached)}.
template <int M, int NJ = 20>
std::vector<double> pfsp_front_time_t(const PfspInstance& in, int lb, const void* nodes, size_t n, int best,
                                      const EngineConfig& cfg, int reps) {
  using G = dev::FrontGeom<M, NJ>;
  using Node = PfspFrontNode<M, NJ>;
  TTS_HIP_CHECK(hipSetDevice(cfg.device));
  (void)lb;
  dev::PfspFrontArgs<M, NJ> a{};
  const std::vector<uint16_t> ptab = pfsp_front_fill_args(in, a);
  ProbeAllocs mem;
  a.ptab = mem.upload(ptab);
  const size_t max_chunks = std::min<size_t>((cfg.max_parents + G::BP - 1) / G::BP, G::MAXCHUNKS);
  dev::PoolCtl h{};
  h.best.v = best;
  const ProbePool<Node> pool(mem, a.pool, nodes, n, max_chunks, G::SLOT, G::BP, h);
  auto& pa = a.pool;
  pa.fuse_max = cfg.fuse_max;
  pa.local_steps = std::min(cfg.local_steps, G::LT);
  pa.local_min = std::max(0, cfg.local_min);
  pa.local_stride = 0;
  pa.local_wide_steps = 0;
  if (const char* f = std::getenv("TTS_LOCAL_STRIDE")) pa.local_stride = std::atoi(f);
  pa.deep_levels = cfg.deep_levels;
  pa.deep_per[0] = cfg.deep_per3;
  pa.deep_per[1] = cfg.deep_per4;
  pa.wide_levels = cfg.wide_levels;
  if (const char* f = std::getenv("TTS_WIDE_LEVELS")) pa.wide_levels = std::atoi(f);
  int bpc = 0, cus = 0;
  bpc = PfspFrontTraits<M, NJ>::blocks_per_cu();
  if (const char* g = std::getenv("TTS_BLOCKS_PER_CU")) bpc = std::max(1, std::atoi(g));  // as DeviceEngine
  TTS_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg.device));
  const int grid = static_cast<int>(std::min<size_t>(max_chunks, static_cast<size_t>(std::max(1, bpc)) * cus));
  // dynamic local DFS (as DeviceEngine): 3 control sets, the budget in wall-clock ticks
  int dyn_us = cfg.dyn_us;
  if (const char* f = std::getenv("TTS_DYN_US")) dyn_us = std::max(0, std::atoi(f));
  const int dq = static_cast<int>(std::min<size_t>(dev::kDynQMax, max_chunks - std::min<size_t>(max_chunks, grid))) / 8 * 8;
  if (G::DYN && dyn_us > 0 && dq >= 8) {
    int rk = 0;
    TTS_HIP_CHECK(hipDeviceGetAttribute(&rk, hipDeviceAttributeWallClockRate, cfg.device));
    pa.dyn = mem.zeroed<dev::DynCtl>(3);
    pa.dyn_ticks = static_cast<int>(static_cast<long long>(dyn_us) * std::max(1, rk) / 1000);
    pa.dyn_q = dq;
  }
  auto restore = [&] {
    pool.restore();
    if (pa.dyn) TTS_HIP_CHECK(hipMemset(pa.dyn, 0, 3 * sizeof(dev::DynCtl)));
  };
  auto launch = [&] {  // as an engine launches it (production unless dynamic or stamped)
    PfspFrontTraits<M, NJ>::launch(a, 0, grid, 0);
    TTS_HIP_CHECK(hipGetLastError());
  };
  const std::vector<double> ms = time_launches(reps, restore, launch);
  restore();
  a.dbg_blk = mem.zeroed<unsigned long long>(static_cast<size_t>(grid) * 16);
  launch();  // (the stamps: the instrumented instantiation)
  TTS_HIP_CHECK(hipDeviceSynchronize());
  std::vector<unsigned long long> blk(static_cast<size_t>(grid) * 16);
  TTS_HIP_CHECK(hipMemcpy(blk.data(), a.dbg_blk, blk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const dev::PoolCtl after = pool.ctl();
  const StampClock us(blk, 16, cfg.device);
  std::vector<double> out = {ms.front(), ms[ms.size() / 2], static_cast<double>(grid),
                             static_cast<double>(after.slot[1].nch)};
  // words 9-10 and 12-14 of a workgroup are raw (dynamic DFS counters and idle ticks,
  // HW_ID, XCC_ID, local DFS counts: front_stamp / front_dyn)
  for (size_t i = 0; i < blk.size(); ++i) {
    const unsigned long long x = blk[i];
    const size_t k = i % 16;
    const bool raw = (k >= 12 && k <= 14) || k == 9 || k == 10;
    out.push_back(raw ? static_cast<double>(x) : (x ? us(x) : 0.0));
  }
  return out;
}

// Bounds of permutation-layout parents through the front kernel (tests): parents are
// converted on the host, bounds come back in the permutation's child order k = depth..N-1.
template <int M, int NJ = 20>
std::vector<int> pfsp_front_bounds_t(const PfspInstance& in, const PfspNode<NJ>* ph, size_t n, int device) {
  using FNode = PfspFrontNode<M, NJ>;
  TTS_HIP_CHECK(hipSetDevice(device));
  const PfspFrontProblem<M, NJ> prob(in, 1);
  std::vector<FNode> fn(n);
  for (size_t i = 0; i < n; ++i) fn[i] = pfsp_front_from_perm(prob, ph[i]);
  const std::vector<int> offsets = perm_child_offsets(ph, n, in.jobs);
  const size_t nb = static_cast<size_t>(offsets[n]);
  std::vector<int> by_job(nb, 0), out(nb, 0);
  if (n == 0) return out;
  dev::PfspFrontArgs<M, NJ> a{};
  const std::vector<uint16_t> ptab = pfsp_front_fill_args(in, a);
  ProbeAllocs mem;
  a.ptab = mem.upload(ptab);
  a.offsets = mem.upload(offsets);
  a.parents_in = mem.upload(fn);
  a.bounds_out = mem.alloc<int>(nb);
  a.nparents = static_cast<int>(n);
  const int blocks = static_cast<int>(std::min<size_t>((n + dev::kBlock - 1) / dev::kBlock, 2048));
  hipLaunchKernelGGL((dev::pfsp_front_bounds_kernel<M, NJ>), dim3(blocks), dim3(dev::kBlock), 0, 0, a);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  TTS_HIP_CHECK(hipMemcpy(by_job.data(), a.bounds_out, nb * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    const int d = ph[i].depth;
    for (int k = d; k < in.jobs; ++k) {
      const int job = ph[i].prmu[k];
      out[offsets[i] + (k - d)] =
          by_job[offsets[i] + mask_count_below(fn[i].rest, job)];
    }
  }
  return out;
}

}  // namespace tts
