// Host-only sweep of the split / scratch arithmetic of nmfmu_conv_backward (csrc/nmfmu_conv_autograd.hip,
// csrc/nmfmu_autograd.hip) over the grid of tests/test_conv_autograd_host.py, for a sanitizer build of the HOST code:
//
//   cd pytorch-nmf_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. nmfmu_conv_autograd.hip nmfmu_autograd.hip \
//       ../../tools/conv_backward_ws_sweep.cpp -o /tmp/conv_backward_ws_sweep && /tmp/conv_backward_ws_sweep
//
// Launches nothing and needs no GPU: it calls the two host functions only.  Exit status 0 and "ok" when every shape passes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nmfmu_aux.h"

namespace {

struct Shape {
  int b, c, r;
  std::vector<int32_t> lh, taps;
};

int64_t prod(const std::vector<int32_t>& v) {
  int64_t p = 1;
  for (int32_t x : v) p *= x;
  return p;
}

int check(const Shape& s) {
  const int nd = (int)s.lh.size();
  const int64_t bj = s.b * prod(s.lh), ct = s.c * prod(s.taps);
  int sp[2] = {-7, -7}, sp2[2] = {-7, -7};
  const int64_t n = nmfmu::conv_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), true, true, sp);
  const int sh = nmfmu::backward_nsplit((int)bj, (int)ct, s.r), sw = nmfmu::backward_nsplit((int)ct, (int)bj, s.r);
  int bad = 0;
  bad |= sp[0] != sh || sp[1] != sw;
  const int64_t nh = sh > 1 ? sh * bj * s.r : 0, nw = sw > 1 ? sw * ct * s.r : 0;
  bad |= n != nh + nw;
  const int64_t contraction[2] = {ct, bj};
  for (int half = 0; half < 2; ++half) {                    // no empty part, only the last one short
    const int parts = sp[half];
    const int64_t len = nmfmu::backward_part_len((int)contraction[half], parts);
    bad |= parts < 1 || len % 32 != 0 || !((parts - 1) * len < contraction[half] && contraction[half] <= parts * len);
  }
  bad |= nmfmu::conv_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), true, false, sp2) != nh || sp2[1] != 0;
  bad |= nmfmu::conv_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), false, true, sp2) != nw || sp2[0] != 0;
  bad |= nmfmu::conv_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), false, false, nullptr) != 0;
  bad |= nmfmu::conv_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), true, true, sp2) != n || sp2[0] != sp[0] ||
         sp2[1] != sp[1];                                   // nothing but the shape goes in
  if (bad) std::printf("FAILED: b %d c %d r %d ndim %d\n", s.b, s.c, s.r, nd);
  return bad;
}

}  // namespace

int main() {
  const std::vector<std::pair<std::vector<int32_t>, std::vector<int32_t>>> axes = {
      {{1}, {1}}, {{50}, {5}}, {{40}, {45}}, {{7793}, {400}}, {{9, 14}, {3, 4}}, {{300, 41}, {16, 8}}, {{4, 5, 6}, {2, 3, 2}},
      {{30, 9, 80}, {3, 1, 4}}};
  std::vector<Shape> grid;
  for (int b : {1, 3})
    for (int c : {1, 33, 1025})
      for (int r : {1, 8, 33, 130})
        for (const auto& a : axes) grid.push_back({b, c, r, a.first, a.second});
  grid.push_back({2, 55, 7, {500}, {20}});
  grid.push_back({1, 13, 130, {20, 35}, {5, 10}});
  grid.push_back({1, 257, 33, {129}, {4}});
  grid.push_back({5, 2, 300, {100000}, {1}});
  grid.push_back({1, 1, 1 << 20, {1 << 15, 1 << 15}, {1 << 15, 1 << 15}});   // the largest sizes accepted: 2^30 x 2^30, rank 2^20
  int bad = 0;
  for (const Shape& s : grid) bad += check(s);
  // rejected sizes return -1 and touch nothing
  const int32_t one[3] = {1, 1, 1}, zero[3] = {1, 0, 1}, big[1] = {1 << 11};
  int sp[2] = {-7, -7};
  bad += nmfmu::conv_backward_ws_floats(1, 1, 1, 0, one, one, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats(1, 1, 1, 4, one, one, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats(0, 1, 1, 1, one, one, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats(1, 1, 1, 3, zero, one, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats(1, 1, 1, 1, nullptr, one, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats(1, 1 << 20, 8, 1, one, big, true, true, sp) != -1;
  bad += nmfmu::conv_backward_ws_floats((1 << 30) + 1, 2, 8, 1, one, one, true, true, sp) != -1;
  bad += sp[0] != -7 || sp[1] != -7;
  std::printf("%zu shapes, %d failed: %s\n", grid.size(), bad, bad ? "FAILED" : "ok");
  return bad != 0;
}
