// The byte rules of k_merge on 32-bit words: four cost bytes at a time, under a byte mask of "this cell lies in the update box".
// Each rule names the reference lines it restates; tests/test_word_rules_host.py builds tools/word_rules_check.cpp with the host
// compiler and runs every rule against its per-byte form over all byte pairs, byte positions and in-box masks.
//
// Conventions: a FLAG word has bit 7 of a byte set where a condition holds for that byte (and no other bit); a MASK word has 0xFF there.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WORD_RULE __host__ __device__ __forceinline__
#else
#define WORD_RULE inline
#endif

namespace word_rules {

constexpr uint32_t kTop = 0x80808080u, kLow7 = 0x7F7F7F7Fu;

// flag: the byte is NO_INFORMATION (255).  The low seven bits plus one carry into bit 7 only from 0x7F, never out of the byte.
WORD_RULE uint32_t isNoInformation(uint32_t w) { return ((w & kLow7) + 0x01010101u) & w & kTop; }

// flag: byte of a < byte of b, unsigned.  (a | 0x80) - (b & 0x7F) borrows nowhere; its bit 7 says low7(a) >= low7(b), which decides
// where the top bits agree.
WORD_RULE uint32_t isBelow(uint32_t a, uint32_t b) {
  const uint32_t d = (a | kTop) - (b & kLow7);
  return ((~a & b) | (~(a ^ b) & ~d)) & kTop;
}

// flag -> mask: 0x80 becomes 0xFF (0x100 - 0x01 per flagged byte; modulo 2^32 for the top byte)
WORD_RULE uint32_t maskOf(uint32_t flags) { return (flags << 1) - (flags >> 7); }

// bytes of `a` where the mask is set, of `b` elsewhere
WORD_RULE uint32_t choose(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }

// CostmapLayer::updateWithTrueOverwrite (costmap_layer.cpp:88-105): master_array[it] = costmap_[it]
WORD_RULE uint32_t updateWithTrueOverwrite(uint32_t /*master*/, uint32_t layer) { return layer; }

// CostmapLayer::updateWithOverwrite (costmap_layer.cpp:107-124): if (costmap_[it] != NO_INFORMATION) master[it] = costmap_[it]
WORD_RULE uint32_t updateWithOverwrite(uint32_t master, uint32_t layer) {
  return choose(maskOf(~isNoInformation(layer) & kTop), layer, master);
}

// CostmapLayer::updateWithMax (costmap_layer.cpp:62-86): a NO_INFORMATION layer cell is skipped;
// if (old_cost == NO_INFORMATION || old_cost < costmap_[it]) master_array[it] = costmap_[it]
WORD_RULE uint32_t updateWithMax(uint32_t master, uint32_t layer) {
  const uint32_t take = ~isNoInformation(layer) & (isNoInformation(master) | isBelow(master, layer));
  return choose(maskOf(take & kTop), layer, master);
}

// bits [lo, hi) of a 16-cell group's in-box bitmap: the group starts at column gx of its row, the box holds columns [x0, xn)
WORD_RULE uint32_t boxBits(int gx, int x0, int xn) {
  int lo = x0 - gx, hi = xn - gx;
  lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
  hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);  // (0 when hi <= lo)
}

// the byte mask of word j (cells 4j .. 4j + 3) of the group from its bitmap: bit i of the nibble -> byte i.  Times 0x00204081 a nibble's
// bit i lands on bits i, i + 7, i + 14, i + 21 - sixteen different places, so nothing carries - and bits 0, 8, 16, 24 are bits 0..3.
WORD_RULE uint32_t boxBytes(uint32_t bits, int j) {
  uint32_t m = (((bits >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u;
  m |= m << 1;  // 0x01 -> 0xFF in three doublings (a multiplication by 255 is a full 32-bit one, at a quarter of the rate)
  m |= m << 2;
  return m | (m << 4);
}

// Costmap2D::resetMap (costmap_2d.cpp:93-99) over a word: memset(..., default_value_, ...)
WORD_RULE uint32_t resetMap(uint8_t default_value) { return (uint32_t)default_value * 0x01010101u; }

// One word of LayeredCostmap::updateMap's reset -> static -> obstacle (layered_costmap.cpp:137-146) for the cells of `in_box`;
// the other bytes come back as `old`.
//   STATIC 0: no static layer, 1: StaticLayer::updateCosts without use_maximum (static_layer.cpp:295-298: updateWithTrueOverwrite), 2: with (updateWithMax)
//   OBST   0: no obstacle layer or a combination_method that does nothing, 1: combination_method 0 (obstacle_layer.cpp:437-447:
//             updateWithOverwrite), 2: combination_method 1 (updateWithMax)
//   LAYER_ONLY: ObstacleLayer::updateCosts alone on the master it is handed: no reset (and the caller passes STATIC 0)
template <int STATIC, int OBST, bool LAYER_ONLY>
WORD_RULE uint32_t mergeWord(uint32_t old, uint32_t stat, uint32_t obst, uint32_t in_box, uint8_t default_value) {
  uint32_t m = LAYER_ONLY ? old : resetMap(default_value);
  if (STATIC == 1) m = updateWithTrueOverwrite(m, stat);
  if (STATIC == 2) m = updateWithMax(m, stat);
  if (OBST == 1) m = updateWithOverwrite(m, obst);
  if (OBST == 2) m = updateWithMax(m, obst);
  return choose(in_box, m, old);
}

// floor(n / d) of a launch-uniform divisor as a multiplication: n < 2^31, d >= 1; mul = ceil(2^(31 + l) / d), shift = 31 + l with
// l = ceil(log2 d) (Granlund & Montgomery 1994, theorem 4.2 with N = 31: mul < 2^32, the product < 2^63)
struct FastDiv {
  uint32_t mul, shift;
};
inline FastDiv fastDivOf(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  const uint64_t p = 1ull << (31 + l);
  return FastDiv{(uint32_t)((p + d - 1) / d), 31 + l};
}
WORD_RULE uint32_t fastDiv(uint32_t n, FastDiv f) { return (uint32_t)(((uint64_t)n * f.mul) >> f.shift); }

}  // namespace word_rules
