// Host check of navigation_amd/csrc/costmap_word_rules.h: every word form against the plain per-byte rule.
//   c++ -std=c++17 -O1 -fsanitize=undefined,address -I navigation_amd/csrc tools/word_rules_check.cpp -o word_rules_check && ./word_rules_check
// (tests/test_word_rules_host.py does that).  Prints one line per part; the exit status is the number of parts that failed.
#include <cstdint>
#include <cstdio>

#include "costmap_word_rules.h"

using namespace word_rules;

namespace {
constexpr uint8_t kNoInfo = 255;

// the rules byte by byte, as the reference spells them
uint8_t byteWithMax(uint8_t m, uint8_t c) {  // costmap_layer.cpp:62-86
  if (c == kNoInfo) return m;
  return (m == kNoInfo || m < c) ? c : m;
}
uint8_t byteWithOverwrite(uint8_t m, uint8_t c) { return c != kNoInfo ? c : m; }  // costmap_layer.cpp:107-124
uint8_t byteMerge(int stat_rule, int obst_rule, bool layer_only, uint8_t old, uint8_t s, uint8_t o, bool in_box, uint8_t dflt) {
  if (!in_box) return old;
  uint8_t m = layer_only ? old : dflt;  // resetMap
  if (stat_rule == 1) m = s;            // updateWithTrueOverwrite
  if (stat_rule == 2) m = byteWithMax(m, s);
  if (obst_rule == 1) m = byteWithOverwrite(m, o);
  if (obst_rule == 2) m = byteWithMax(m, o);
  return m;
}

uint8_t byteAt(uint32_t w, int p) { return (uint8_t)(w >> (8 * p)); }
// a word with `b` at byte p and bytes that exercise carries and borrows around it
uint32_t around(uint8_t b, int p, uint32_t filler) { return (filler & ~(0xFFu << (8 * p))) | ((uint32_t)b << (8 * p)); }
const uint32_t kFillers[4] = {0x00000000u, 0xFFFFFFFFu, 0x7F80FE01u, 0x80FF7FFDu};

template <int STATIC, int OBST, bool LAYER_ONLY>
long mergeErrors() {
  long bad = 0;
  for (int dflt = 0; dflt < 256; dflt += 255)
    for (int p = 0; p < 4; ++p)
      for (uint32_t a = 0; a < 256; ++a)      // static byte (old master byte when LAYER_ONLY)
        for (uint32_t b = 0; b < 256; ++b) {  // obstacle byte
          const uint32_t fo = kFillers[(a + b) & 3], fs = kFillers[(a >> 2) & 3], fl = kFillers[(b >> 2) & 3];
          const uint8_t old_b = LAYER_ONLY ? (uint8_t)a : (uint8_t)(a * 7 + b * 13 + 5);
          const uint32_t old = around(old_b, p, fo), sw = around((uint8_t)a, p, fs), lw = around((uint8_t)b, p, fl);
          for (uint32_t nib = 0; nib < 16; ++nib) {
            const uint32_t in_box = boxBytes(nib << 4, 1);
            const uint32_t got = mergeWord<STATIC, OBST, LAYER_ONLY>(old, sw, lw, in_box, (uint8_t)dflt);
            for (int q = 0; q < 4; ++q) {
              const uint8_t want = byteMerge(STATIC, OBST, LAYER_ONLY, byteAt(old, q), byteAt(sw, q), byteAt(lw, q), (nib >> q) & 1u, (uint8_t)dflt);
              if (byteAt(got, q) != want) ++bad;
            }
          }
        }
  // every old master byte at every position and mask (out of the box it must come back as it was)
  for (int p = 0; p < 4; ++p)
    for (uint32_t o = 0; o < 256; ++o)
      for (uint32_t nib = 0; nib < 16; ++nib)
        for (int f = 0; f < 4; ++f) {
          const uint32_t old = around((uint8_t)o, p, kFillers[f]), sw = around((uint8_t)(o ^ 0x5A), p, kFillers[(f + 1) & 3]),
                         lw = around((uint8_t)(255 - o), p, kFillers[(f + 2) & 3]);
          const uint32_t got = mergeWord<STATIC, OBST, LAYER_ONLY>(old, sw, lw, boxBytes(nib, 0), 255);
          for (int q = 0; q < 4; ++q)
            if (byteAt(got, q) != byteMerge(STATIC, OBST, LAYER_ONLY, byteAt(old, q), byteAt(sw, q), byteAt(lw, q), (nib >> q) & 1u, 255)) ++bad;
        }
  return bad;
}

int report(const char* what, long bad) {
  std::printf("%-46s %s (%ld)\n", what, bad ? "FAILED" : "ok", bad);
  return bad ? 1 : 0;
}
}  // namespace

int main() {
  int failed = 0;
  // ---- the flag and mask helpers over every byte pair at every position
  long bad = 0;
  for (int p = 0; p < 4; ++p)
    for (uint32_t a = 0; a < 256; ++a)
      for (uint32_t b = 0; b < 256; ++b)
        for (int f = 0; f < 4; ++f) {
          const uint32_t wa = around((uint8_t)a, p, kFillers[f]), wb = around((uint8_t)b, p, kFillers[(f + b) & 3]);
          const uint32_t ni = isNoInformation(wa), lt = isBelow(wa, wb);
          if ((ni & ~kTop) || (lt & ~kTop)) ++bad;
          for (int q = 0; q < 4; ++q) {
            if (((ni >> (8 * q + 7)) & 1u) != (byteAt(wa, q) == 255)) ++bad;
            if (((lt >> (8 * q + 7)) & 1u) != (byteAt(wa, q) < byteAt(wb, q))) ++bad;
          }
          if (byteAt(updateWithMax(wa, wb), p) != byteWithMax((uint8_t)a, (uint8_t)b)) ++bad;
          if (byteAt(updateWithOverwrite(wa, wb), p) != byteWithOverwrite((uint8_t)a, (uint8_t)b)) ++bad;
          if (updateWithTrueOverwrite(wa, wb) != wb) ++bad;
        }
  for (uint32_t flags = 0; flags < 16; ++flags) {
    uint32_t f = 0, want = 0;
    for (int q = 0; q < 4; ++q)
      if ((flags >> q) & 1u) f |= 0x80u << (8 * q), want |= 0xFFu << (8 * q);
    if (maskOf(f) != want) ++bad;
    if (choose(want, 0x11223344u, 0xAABBCCDDu) != ((0x11223344u & want) | (0xAABBCCDDu & ~want))) ++bad;
  }
  failed += report("isNoInformation / isBelow / maskOf / the rules", bad);

  // ---- the box bitmap of a group and its byte masks
  bad = 0;
  for (int gx = 0; gx <= 64; gx += 16)
    for (int x0 = -3; x0 <= 84; ++x0)
      for (int xn = -3; xn <= 84; ++xn) {
        uint32_t want = 0;
        for (int k = 0; k < 16; ++k)
          if (gx + k >= x0 && gx + k < xn) want |= 1u << k;
        if (boxBits(gx, x0, xn) != want) ++bad;
      }
  if (boxBits(1 << 30, 0, 0x7FFFFFFF) != 0xFFFFu || boxBits(0, 0x7FFFFFF0, 0x7FFFFFFF) != 0u) ++bad;
  for (uint32_t bits = 0; bits < 65536; ++bits)
    for (int j = 0; j < 4; ++j) {
      uint32_t want = 0;
      for (int q = 0; q < 4; ++q)
        if ((bits >> (4 * j + q)) & 1u) want |= 0xFFu << (8 * q);
      if (boxBytes(bits, j) != want) ++bad;
    }
  if (resetMap(0) != 0u || resetMap(255) != 0xFFFFFFFFu || resetMap(0x5A) != 0x5A5A5A5Au) ++bad;
  failed += report("boxBits / boxBytes / resetMap", bad);

  // ---- the merge of a word under every setting
  failed += report("merge: no static, no obstacle", mergeErrors<0, 0, false>());
  failed += report("merge: no static, overwrite", mergeErrors<0, 1, false>());
  failed += report("merge: no static, max", mergeErrors<0, 2, false>());
  failed += report("merge: static overwrite, no obstacle", mergeErrors<1, 0, false>());
  failed += report("merge: static overwrite, overwrite", mergeErrors<1, 1, false>());
  failed += report("merge: static overwrite, max", mergeErrors<1, 2, false>());
  failed += report("merge: static max, no obstacle", mergeErrors<2, 0, false>());
  failed += report("merge: static max, overwrite", mergeErrors<2, 1, false>());
  failed += report("merge: static max, max", mergeErrors<2, 2, false>());
  failed += report("merge: layer only, nothing", mergeErrors<0, 0, true>());
  failed += report("merge: layer only, overwrite", mergeErrors<0, 1, true>());
  failed += report("merge: layer only, max", mergeErrors<0, 2, true>());

  // ---- division by multiplication: every divisor up to 4100 and some large ones, dividends around every multiple's edge
  bad = 0;
  const uint32_t big[] = {4999, 5000, 46340, 65535, 65536, 65537, 1000003, 0x3FFFFFFF, 0x40000000, 0x40000001, 0x7FFFFFFF};
  for (uint32_t i = 1; i <= 4100 + sizeof big / sizeof *big; ++i) {
    const uint32_t d = i <= 4100 ? i : big[i - 4101];
    const FastDiv f = fastDivOf(d);
    if (f.shift < 31 || f.shift > 62) ++bad;
    const uint64_t top = 0x7FFFFFFFull;
    for (uint64_t k = 0; k <= top / d; k += (top / d) / 257 + 1) {
      const uint64_t cand[3] = {k * d, k * d + d - 1, k * d + d / 2};  // a multiple, the last dividend before the next, one between
      for (uint64_t c : cand)
        if (c <= top && fastDiv((uint32_t)c, f) != (uint32_t)(c / d)) ++bad;
    }
    if (fastDiv((uint32_t)top, f) != (uint32_t)(top / d) || fastDiv(0, f) != 0) ++bad;
  }
  failed += report("fastDiv", bad);
  return failed;
}
