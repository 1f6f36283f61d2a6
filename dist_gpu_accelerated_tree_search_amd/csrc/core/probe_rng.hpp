// Random choices of an indexed Knuth probe, shared by the host twin (core/estimate.hpp
// knuth_estimate_indexed) and the device kernel (hip/estimate_kernels.hpp). Plain C++,
// no ROCm dependency: the same text compiles in host and device code.
//
// The choice a probe makes at a level depends on (seed, probe index, level) alone, never
// on a thread, a wave, a grid size or a launch. All arithmetic is modulo 2^64:
//
//   mix(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;
//            x ^= x >> 27;  x *= 0x94d049bb133111eb;
//            x ^= x >> 31;                                  (the splitmix64 finaliser)
//   G = 0x9e3779b97f4a7c15
//   h(seed, probe)  = mix(seed + G * (probe + 1))           once per probe
//   r(h, level)     = mix(h + G * (level + 1))              level = depth of the parent, 0 at the root
//   pick(r, k)      = ((r >> 32) * k) >> 32                 index among k survivors, 0 <= pick < k
//   pick_weighted(r, T) = (r * T) >> 64                     the high half of the 64 x 64 product, 0 <= x < T
//
// The survivors are ordered by the job they append, ascending; pick is an index into
// that order. k is at most the number of jobs (< 2^32). A lookahead probe
// (lookahead_estimate_indexed) gives survivor c an integer weight wt_c, T is their sum
// (T < 2^36) and its choice is the first survivor in that order whose inclusive prefix
// sum of weights exceeds pick_weighted(r, T).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // __umul64hi, for the device side of probe_pick_weighted
#endif

#ifndef TTS_HD
#if defined(__HIPCC__)
#define TTS_HD __host__ __device__
#else
#define TTS_HD
#endif
#endif

namespace tts {

constexpr uint64_t kProbeGolden = 0x9e3779b97f4a7c15ull;

TTS_HD inline uint64_t probe_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

TTS_HD inline uint64_t probe_hash(uint64_t seed, uint64_t probe) { return probe_mix(seed + kProbeGolden * (probe + 1)); }

TTS_HD inline uint64_t probe_draw(uint64_t h, uint32_t level) {
  return probe_mix(h + kProbeGolden * (static_cast<uint64_t>(level) + 1));
}

TTS_HD inline uint32_t probe_pick(uint64_t r, uint32_t k) {
  return static_cast<uint32_t>(((r >> 32) * static_cast<uint64_t>(k)) >> 32);
}

TTS_HD inline uint64_t probe_pick_weighted(uint64_t r, uint64_t T) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, T);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(r) * T) >> 64);
#endif
}

}  // namespace tts
