// Working stand-in for <boost/algorithm/string.hpp>, for tools/tp_reference_harness.cpp only, written from Boost's documentation:
// split over is_any_of with token_compress_on merging adjacent separators (a leading or trailing run still leaves an empty token).
#pragma once
#include <string>
#include <vector>
namespace boost {
struct is_any_of_t { std::string s; };
inline is_any_of_t is_any_of(const std::string& s) { is_any_of_t t; t.s = s; return t; }
enum token_compress_mode_type { token_compress_on, token_compress_off };
template <class V> void split(V& out, const std::string& in, const is_any_of_t& sep, token_compress_mode_type mode = token_compress_off) {
  out.clear();
  std::string cur;
  bool last_was_separator = false;
  for (char c : in) {
    if (sep.s.find(c) != std::string::npos) {
      if (!(mode == token_compress_on && last_was_separator)) { out.push_back(cur); cur.clear(); }
      last_was_separator = true;
    } else {
      cur += c;
      last_was_separator = false;
    }
  }
  out.push_back(cur);
}
}  // namespace boost
