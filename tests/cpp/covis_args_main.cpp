// covis_args_main.cpp -- the argument checks of covis.hip's entry points (csrc/orbx_covis_args.h: host only, no
// device call) in a program of their own, to be built with the address and undefined-behaviour sanitizers and
// run on the CPU:
//   make -C orb_slam2_commit_amd/csrc asan_covis_args
// Every array is heap-allocated at its exact size, so a check that reads past n is caught.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orb_slam2_commit_amd/csrc/orbx_covis_args.h"

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #c); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

using namespace orbx;

int main() {
  {  // rows
    std::vector<int32_t> pid{3, -1, 7, -1, 0}, oct{0, 1, 7, 63, 2};
    std::vector<uint8_t> fl{0, 1, 2, 3, 0};
    REQUIRE(covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    REQUIRE(covis_row_ok(nullptr, nullptr, nullptr, 0));
    REQUIRE(!covis_row_ok(nullptr, nullptr, nullptr, 1));
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), nullptr, 5));
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), -1));
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), kCovisMaxRow + 1));  // refused before any read
    pid[4] = 3;  // a point twice
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    REQUIRE(covis_row_ok(pid.data(), oct.data(), fl.data(), 4));
    pid[4] = -2;
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    pid[4] = kCovisMaxPoint;
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    pid[4] = kCovisMaxPoint - 1;
    REQUIRE(covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    oct[0] = 64;
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    oct[0] = -1;
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    oct[0] = 0;
    fl[2] = 4;
    REQUIRE(!covis_row_ok(pid.data(), oct.data(), fl.data(), 5));
    // a long row of distinct ids, and the same with its last id repeated
    const int n = 100000;
    std::vector<int32_t> big(n), bo(n, 0);
    std::vector<uint8_t> bf(n, 3);
    for (int i = 0; i < n; i++) big[i] = (int32_t)((i * 7919LL) % 1000003);
    REQUIRE(covis_row_ok(big.data(), bo.data(), bf.data(), n));
    big[n - 1] = big[0];
    REQUIRE(!covis_row_ok(big.data(), bo.data(), bf.data(), n));
  }
  {  // keyframe lists
    std::vector<int64_t> ids{5, 0, 9, (int64_t)1 << 40};
    REQUIRE(covis_kf_list_ok(ids.data(), 4));
    REQUIRE(covis_kf_list_ok(nullptr, 0));
    REQUIRE(!covis_kf_list_ok(nullptr, 2));
    REQUIRE(!covis_kf_list_ok(ids.data(), -3));
    ids[2] = 5;
    REQUIRE(!covis_kf_list_ok(ids.data(), 4));
    REQUIRE(covis_kf_list_ok(ids.data(), 2));
    ids[2] = -1;
    REQUIRE(!covis_kf_list_ok(ids.data(), 4));
  }
  {  // point lists
    std::vector<int32_t> ids{4, 4, -1, 0};
    REQUIRE(covis_point_list_ok(ids.data(), 4, true));
    REQUIRE(!covis_point_list_ok(ids.data(), 4, false));
    REQUIRE(covis_point_list_ok(ids.data(), 2, false));
    REQUIRE(covis_point_list_ok(nullptr, 0, false) && !covis_point_list_ok(nullptr, 1, true));
    REQUIRE(!covis_point_list_ok(ids.data(), -1, true));
    REQUIRE(covis_max_point(ids.data(), 4) == 4 && covis_max_point(ids.data(), 0) == -1);
    ids[3] = kCovisMaxPoint;
    REQUIRE(!covis_point_list_ok(ids.data(), 4, true));
    ids[3] = -2;
    REQUIRE(!covis_point_list_ok(ids.data(), 4, true));
  }
  std::printf("covis args ok\n");
  return 0;
}
