// Host-only sweep of the scratch / half-selection / workgroup arithmetic of nmfmu_plca_backward and nmfmu_conv_plca_backward
// (csrc/nmfmu_plca_autograd.hip) over the grid of tests/test_plca_autograd_host.py, for a sanitizer build of the HOST code:
//
//   cd pytorch-nmf_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. nmfmu_plca_autograd.hip nmfmu_conv_autograd.hip nmfmu_autograd.hip \
//       ../../tools/plca_backward_ws_sweep.cpp -o /tmp/plca_backward_ws_sweep && /tmp/plca_backward_ws_sweep
//
// Launches nothing and needs no GPU: it calls the host functions only.  Exit status 0 and "ok" when every shape passes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nmfmu_aux.h"

namespace {

int64_t prod(const std::vector<int32_t>& v) {
  int64_t p = 1;
  for (int32_t x : v) p *= x;
  return p;
}

int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

// the workgroup rule as include/nmfmu.h states it
int grid_check(int64_t outer, int rank, int64_t inner, int* blocks) {
  const nmfmu::PlcaFinishGrid g = nmfmu::plca_finish_grid(outer, rank, inner);
  const __int128 total = (__int128)outer * rank * inner;
  const int64_t want = (int64_t)std::min<__int128>(2048, (total + 8191) / 8192);
  const int64_t chunk = (outer + std::min(want, outer) - 1) / std::min(want, outer), nbo = (outer + chunk - 1) / chunk;
  int64_t nseg = 1, seg = inner;
  if (inner > 1) {
    const int64_t ns = std::max<int64_t>(1, std::min((want + nbo - 1) / nbo, inner / 1024));
    seg = ((inner + ns - 1) / ns + 3) / 4 * 4, nseg = (inner + seg - 1) / seg;
  }
  int bad = g.nbo != nbo || g.chunk != chunk || g.nseg != nseg || g.seg != seg;
  bad |= !((nbo - 1) * chunk < outer && outer <= nbo * chunk) || !((nseg - 1) * seg < inner && inner <= nseg * seg);
  bad |= nbo > 2048 || nseg > 2048 || (inner > 1 && seg % 4 != 0);
  *blocks = g.blocks();
  return bad;
}

// info and size for one combination of wanted outputs, from the two halves' (parts, output view)
int plan_check(int64_t n, const int* info, int wh, int ww, int wz, int parts_h, int parts_w, int64_t outer_h, int64_t inner_h,
               int64_t outer_w, int64_t inner_w, int rank) {
  const bool run_h = wh, z_h = wz && wh && !ww, run_w = ww || (wz && !wh);
  int bh = 0, bw = 0, bad = 0;
  int64_t want = 0;
  if (run_h) {
    bad |= grid_check(outer_h, rank, inner_h, &bh);
    if (parts_h > 1) want += round4(parts_h * outer_h * rank * inner_h);
  }
  if (run_w) {
    bad |= grid_check(outer_w, rank, inner_w, &bw);
    if (parts_w > 1 || !ww) want += round4(parts_w * outer_w * rank * inner_w);
  }
  if (wz) want += (int64_t)(z_h ? bh : bw) * rank;
  bad |= n != want;
  bad |= info[0] != (run_h ? parts_h : 0) || info[1] != (run_w ? parts_w : 0) || info[2] != bh || info[3] != bw;
  bad |= info[4] != (wz ? (z_h ? 1 : 2) : 0);
  return bad;
}

int check_dense(int m, int k, int r) {
  const int ph = nmfmu::backward_nsplit(m, k, r), pw = nmfmu::backward_nsplit(k, m, r);
  int bad = 0;
  for (int w = 0; w < 8; ++w) {
    int info[5] = {-7, -7, -7, -7, -7};
    const int64_t n = nmfmu::plca_backward_ws_floats(m, k, r, w & 4, w & 2, w & 1, info);
    bad |= plan_check(n, info, w & 4, w & 2, w & 1, ph, pw, m, 1, k, 1, r);
    bad |= nmfmu::plca_backward_ws_floats(m, k, r, w & 4, w & 2, w & 1, nullptr) != n;
  }
  if (bad) std::printf("FAILED: dense m %d k %d r %d\n", m, k, r);
  return bad;
}

struct Shape {
  int b, c, r;
  std::vector<int32_t> lh, taps;
};

int check_conv(const Shape& s) {
  const int nd = (int)s.lh.size();
  const int64_t pj = prod(s.lh), pt = prod(s.taps), bj = s.b * pj, ct = s.c * pt;
  const int ph = nmfmu::backward_nsplit((int)bj, (int)ct, s.r), pw = nmfmu::backward_nsplit((int)ct, (int)bj, s.r);
  int bad = 0;
  for (int w = 0; w < 8; ++w) {
    int info[5] = {-7, -7, -7, -7, -7};
    const int64_t n = nmfmu::conv_plca_backward_ws_floats(s.b, s.c, s.r, nd, s.lh.data(), s.taps.data(), w & 4, w & 2, w & 1, info);
    bad |= plan_check(n, info, w & 4, w & 2, w & 1, ph, pw, s.b, pj, s.c, pt, s.r);
  }
  if (bad) std::printf("FAILED: conv b %d c %d r %d ndim %d\n", s.b, s.c, s.r, nd);
  return bad;
}

}  // namespace

int main() {
  int bad = 0, count = 0;
  const int mk[][2] = {{1, 1}, {33, 130}, {300, 257}, {200, 90}, {1000, 1100}, {700, 650}, {4096, 65536}, {5, 100000},
                       {1 << 30, 1}, {1, 1 << 30}};
  for (const auto& s : mk)
    for (int r : {1, 7, 33, 128, 130, 256, 1030, 1 << 20}) bad += check_dense(s[0], s[1], r), ++count;
  const std::vector<std::pair<std::vector<int32_t>, std::vector<int32_t>>> axes = {
      {{1}, {1}}, {{50}, {5}}, {{40}, {45}}, {{7793}, {400}}, {{9, 14}, {3, 4}}, {{300, 41}, {16, 8}}, {{4, 5, 6}, {2, 3, 2}},
      {{30, 9, 80}, {3, 1, 4}}, {{4500}, {2}}, {{4501}, {3}}};
  std::vector<Shape> grid;
  for (int b : {1, 3})
    for (int c : {1, 33, 1025})
      for (int r : {1, 8, 33, 130})
        for (const auto& a : axes) grid.push_back({b, c, r, a.first, a.second});
  grid.push_back({2, 55, 7, {500}, {20}});
  grid.push_back({1, 13, 130, {20, 35}, {5, 10}});
  grid.push_back({5, 2, 300, {100000}, {1}});
  grid.push_back({1, 1, 1 << 20, {1 << 15, 1 << 15}, {1 << 15, 1 << 15}});   // the largest sizes accepted: 2^30 x 2^30, rank 2^20
  for (const Shape& s : grid) bad += check_conv(s), ++count;
  // rejected sizes return -1 and touch nothing
  const int32_t one[3] = {1, 1, 1}, zero[3] = {1, 0, 1}, big[1] = {1 << 11};
  int info[5] = {-7, -7, -7, -7, -7};
  bad += nmfmu::conv_plca_backward_ws_floats(1, 1, 1, 0, one, one, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats(1, 1, 1, 4, one, one, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats(0, 1, 1, 1, one, one, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats(1, 1, 1, 3, zero, one, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats(1, 1, 1, 1, nullptr, one, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats(1, 1 << 20, 8, 1, one, big, true, true, true, info) != -1;
  bad += nmfmu::conv_plca_backward_ws_floats((1 << 30) + 1, 2, 8, 1, one, one, true, true, true, info) != -1;
  for (int v : info) bad += v != -7;
  std::printf("%d shapes, %d failed: %s\n", count, bad, bad ? "FAILED" : "ok");
  return bad != 0;
}
