// How a pool iteration deals its parent window over chunks (hip/pool_device.hpp
// pool_begin), host-callable: the kernels run the 32-bit form — every workgroup of every
// dependent kernel does this arithmetic before its first bound, and gfx950 has no 64-bit
// divide: each one expands to a long scalar sequence — and the CPU tests check it against
// the 64-bit form it replaced (tests/test_pool_window.py).
//
// A window holds B <= max_parents parents, and max_parents is an int (PoolArgs), so B, the
// spread (a grid size or a chunk count) and every quotient fit 32 bits. The ring occupancy,
// the buffered children, the ring base and the ring index stay 64-bit in pool_begin.
#pragma once

#include <cstdint>

#ifndef TTS_HD
#if defined(__HIPCC__)
#define TTS_HD __host__ __device__
#else
#define TTS_HD
#endif
#endif

namespace tts {

// Largest parent window the 32-bit form is exact for (engine.hpp checks max_parents).
constexpr uint64_t kPoolWindowMax = 0x7fffffffull;

struct PoolDeal {
  uint32_t per;  // parents per chunk when the window is spread evenly: ceil(B / spread)
  int bp;        // parents per chunk: per, at least 1 and at most cap
  int nchunks;   // ceil(B / bp)
};

// ceil(a / b) without the a + b - 1 that could wrap: b > 0.
TTS_HD inline uint32_t pool_ceil_div32(uint32_t a, uint32_t b) { return a ? (a - 1u) / b + 1u : 0u; }

// B parents spread over `spread` chunks of at most `cap` parents each (spread, cap > 0).
TTS_HD inline PoolDeal pool_deal32(uint32_t B, uint32_t spread, uint32_t cap) {
  PoolDeal d;
  d.per = pool_ceil_div32(B, spread);
  const uint32_t bp = d.per < 1u ? 1u : (d.per > cap ? cap : d.per);
  d.bp = static_cast<int>(bp);
  d.nchunks = static_cast<int>(pool_ceil_div32(B, bp));
  return d;
}

// The 64-bit form pool_begin used (the reference of the CPU check).
inline PoolDeal pool_deal64(uint64_t B, uint64_t spread, uint64_t cap) {
  PoolDeal d;
  const uint64_t per = (B + spread - 1) / spread;
  d.per = static_cast<uint32_t>(per);
  const uint64_t bp = per < 1 ? 1 : (per > cap ? cap : per);
  d.bp = static_cast<int>(bp);
  d.nchunks = static_cast<int>((B + bp - 1) / bp);
  return d;
}

}  // namespace tts
