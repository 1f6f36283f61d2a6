// N-Queens device engine factory (definitions in queens_engine.hip).
#pragma once

#include <memory>
#include <vector>

#include "engine.hpp"
#include "../core/pfsp_node.hpp"

namespace tts {

std::unique_ptr<IEngine> make_queens_engine(int N, int G, const EngineConfig& cfg);

// What ONE iteration of the production kernel (queens_expand_kernel) wrote (tests). The
// nodes are the whole pool, in the ring; the window is dealt in chunks of 256 parents, so
// chunk c holds the children of parents [256 c, 256 c + 256) in parent order, rows
// ascending; leaves (depth N) and finishing parents contribute none.
//   finish_k     parents with at most this many columns left are finished in the kernel
//                (clamped like the engine's; the environment is not read)
//   split_world  > 1: the iteration is the rank split of a replicated pool (split_min 1):
//                each rank keeps its share of the children, no finishing
struct QueensExpandResult {
  std::vector<uint8_t> children;  // node bytes, chunks back to back
  std::vector<int> counts;        // children per chunk
  unsigned long long leaves = 0;  // sum of the chunks' leaf words
  unsigned long long fin_tree = 0, fin_sol = 0;  // sums of the finishing accumulator lines
};
QueensExpandResult queens_expand_probe(int N, int G, const QueensNode* nodes, size_t n, int finish_k, int split_rank,
                                       int split_world, int device);
// Nodes per wave of the finishing stacks in this build (TTS_QSTACK).
int queens_stack_nodes();
std::vector<uint8_t> queens_gpu_labels(int N, int G, const QueensNode* parents, size_t n, int device);

}  // namespace tts
