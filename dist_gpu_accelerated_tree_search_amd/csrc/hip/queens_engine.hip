// N-Queens device engine (traits + factory) and reference-style label evaluation.
#include <algorithm>
#include <cstdlib>
#include <stdexcept>

#include "probe_pool.hpp"
#include "queens_engine.hpp"
#include "queens_kernels.hpp"

namespace tts {

struct QueensTraits {
  using Node = QueensNode;
  using Args = dev::QueensArgs;
  using S = dev::QueensSmem;
  static constexpr int kParentsPerChunk = S::BP;
  static constexpr int kChildrenPerChunk = S::MAXCH;
  static constexpr int kMaxChildren = S::MAXCH / S::BP;
  static constexpr int kLocalSteps = 1;
  static constexpr int kLocalMin = 0;
  static constexpr int kMaxChunks = S::MAXCHUNKS;
  static void launch(const Args& a, int t, int grid, hipStream_t s) {
    hipLaunchKernelGGL(dev::queens_expand_kernel, dim3(grid), dim3(dev::kBlock), 0, s, a, t);
  }
  static void flatten(const dev::PoolArgs<Node>& pa, int b, int grid, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_flatten_kernel<Node, S::MAXCH, S::MAXCHUNKS>), dim3(grid), dim3(dev::kBlock), 0, s,
                       pa, b);
  }
  static void finalize(const dev::PoolArgs<Node>& pa, int b, int slot, hipStream_t s) {
    hipLaunchKernelGGL((dev::pool_finalize_kernel<Node, S::MAXCHUNKS>), dim3(1), dim3(dev::kBlock), 0, s, pa, b, slot);
  }
  static int blocks_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, dev::queens_expand_kernel, dev::kBlock, 0) != hipSuccess)
      return 1;
    // 106 SGPRs allow 6 resident per CU; the grid takes 5 (N=17 47.1 -> 46.0 ms, 4 and 8
    // slower; profiles/r5/grid_ab.txt)
    return dev::resident_blocks(n, 5);
  }
};

static dev::QueensArgs queens_args(int N, int G) {
  if (N < 1 || N > 32) throw std::invalid_argument("N-Queens supports 1 <= N <= 32");
  if (G < 1) throw std::invalid_argument("g must be >= 1");
  dev::QueensArgs a{};
  a.N = N;
  a.G = G;
  a.full = N == 32 ? 0xffffffffu : ((1u << N) - 1u);
  // subtree finishing: parents with at most finish_k columns left (TTS_QUEENS_FINISH
  // overrides; 0 = level-by-level to the bottom). The wave-cooperative finishing is
  // fastest from 9 columns left (N=17: 6 / 7 / 8 / 9 / 10 / 11 / 12 columns 48 / 29 / 24 /
  // 21 / 25 / 37 / 138 ms; deeper subtrees overflow the LDS stacks into the register walk,
  // profiles/r6/queens/finish_depth_ab.txt)
  a.finish_k = 9;
  if (const char* f = std::getenv("TTS_QUEENS_FINISH")) a.finish_k = std::atoi(f);
  a.finish_k = std::max(0, std::min(a.finish_k, dev::kQueensFinishMax));
  return a;
}

std::unique_ptr<IEngine> make_queens_engine(int N, int G, const EngineConfig& cfg) {
  TTS_HIP_CHECK(hipSetDevice(cfg.device));
  return std::make_unique<DeviceEngine<QueensTraits>>(cfg, queens_args(N, G));
}

int queens_stack_nodes() { return dev::kQStack; }

QueensExpandResult queens_expand_probe(int N, int G, const QueensNode* nodes, size_t n, int finish_k, int split_rank,
                                       int split_world, int device) {
  using S = dev::QueensSmem;
  if (split_world > 1 && (split_rank < 0 || split_rank >= split_world))
    throw std::invalid_argument("queens expand probe: split_rank outside [0, split_world)");
  TTS_HIP_CHECK(hipSetDevice(device));
  dev::QueensArgs a = queens_args(N, G);
  a.finish_k = std::max(0, std::min(finish_k, dev::kQueensFinishMax));  // (not the environment's)
  // the finishing stacks rely on depth == queens placed (at most finish_k children per stacked node)
  for (size_t i = 0; i < n; ++i)
    if (static_cast<int>(nodes[i].depth) > N || __builtin_popcount(nodes[i].cols) != static_cast<int>(nodes[i].depth) ||
        (nodes[i].cols & ~a.full))
      throw std::invalid_argument("queens expand probe: a node's depth is not the number of its placed queens");
  QueensExpandResult res;
  if (n == 0) return res;
  const size_t nchunks = (n + S::BP - 1) / S::BP;
  if (nchunks > static_cast<size_t>(S::MAXCHUNKS)) throw std::invalid_argument("queens expand probe: too many parents");
  dev::PoolCtl h{};
  if (split_world > 1) {
    // the window holds the whole pool and at least split_min parents: this iteration splits
    h.split_world = split_world;
    h.split_rank = split_rank;
    h.split_min = 1;
  }
  ProbeAllocs mem;
  const ProbePool<QueensNode> pool(mem, a.pool, nodes, n, nchunks, S::MAXCH, S::BP, h);
  QueensTraits::launch(a, 0, static_cast<int>(nchunks), 0);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  ProbeChunks ch = pool.read_chunks(nchunks, "queens expand probe");
  res.children = std::move(ch.children);
  res.counts = std::move(ch.counts);
  for (int w : ch.lwords) res.leaves += static_cast<uint32_t>(w);  // (the whole leaf word: this kernel has no inner half)
  h = pool.ctl();
  if (h.overflow) throw std::runtime_error("queens expand probe: the iteration reported an overflow");
  for (const auto& x : h.xacc) {
    res.fin_tree += x.tree;
    res.fin_sol += x.sol;
  }
  return res;
}

std::vector<uint8_t> queens_gpu_labels(int N, int G, const QueensNode* parents, size_t n, int device) {
  TTS_HIP_CHECK(hipSetDevice(device));
  dev::QueensArgs a = queens_args(N, G);
  std::vector<uint8_t> out(n * static_cast<size_t>(N), 0);
  if (n == 0) return out;
  ProbeAllocs mem;
  a.parents_in = mem.upload(parents, n);
  a.labels_out = mem.alloc<uint8_t>(out.size());
  a.nparents = static_cast<int>(n);
  const int blocks = static_cast<int>((n + dev::kBlock - 1) / dev::kBlock);
  hipLaunchKernelGGL(dev::queens_labels_kernel, dim3(blocks), dim3(dev::kBlock), 0, 0, a);
  TTS_HIP_CHECK(hipGetLastError());
  TTS_HIP_CHECK(hipDeviceSynchronize());
  TTS_HIP_CHECK(hipMemcpy(out.data(), a.labels_out, out.size(), hipMemcpyDeviceToHost));
  return out;
}

}  // namespace tts
