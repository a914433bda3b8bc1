// orbx_covis_args.h -- the argument checks of covis.hip's entry points.  Host only: no launch, no
// device call, no HIP header, so the checks build and run on their own (tests/cpp/covis_args_main.cpp
// runs them under the address and undefined-behaviour sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace orbx {

constexpr int kCovisMaxRow = 1 << 20;         // features of one keyframe
constexpr int kCovisMaxOctave = 63;           // the octave lives in 6 bits of a row entry
constexpr int32_t kCovisMaxPoint = 1 << 26;   // point ids are below this (the per-point tables are dense)
constexpr uint8_t kCovisStereo = 1, kCovisClose = 2;  // the caller's flag bits

// one row: n features, each a point id (-1: none, else 0 <= id < kCovisMaxPoint, no id twice), an
// octave in 0..63 and the two flag bits
inline bool covis_row_ok(const int32_t* point_ids, const int32_t* octaves, const uint8_t* flags, int n) {
  if (n < 0 || n > kCovisMaxRow || (n > 0 && (!point_ids || !octaves || !flags))) return false;
  std::vector<int32_t> seen;
  seen.reserve((size_t)n);
  for (int i = 0; i < n; i++) {
    if (point_ids[i] < -1 || point_ids[i] >= kCovisMaxPoint) return false;
    if (octaves[i] < 0 || octaves[i] > kCovisMaxOctave) return false;
    if (flags[i] & ~(kCovisStereo | kCovisClose)) return false;
    if (point_ids[i] >= 0) seen.push_back(point_ids[i]);
  }
  std::sort(seen.begin(), seen.end());
  return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

// a list of keyframe ids: none negative, none twice
inline bool covis_kf_list_ok(const int64_t* ids, int n) {
  if (n < 0 || (n > 0 && !ids)) return false;
  std::vector<int64_t> seen(ids, ids + n);
  for (int64_t v : seen)
    if (v < 0) return false;
  std::sort(seen.begin(), seen.end());
  return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

// a list of point ids (repeats allowed); none_ok: -1 stands for "no point"
inline bool covis_point_list_ok(const int32_t* ids, int n, bool none_ok) {
  if (n < 0 || (n > 0 && !ids)) return false;
  for (int i = 0; i < n; i++)
    if (ids[i] < (none_ok ? -1 : 0) || ids[i] >= kCovisMaxPoint) return false;
  return true;
}

// the largest id of a list (-1 when it holds none)
inline int32_t covis_max_point(const int32_t* ids, int n) {
  int32_t m = -1;
  for (int i = 0; i < n; i++) m = std::max(m, ids[i]);
  return m;
}

}  // namespace orbx
