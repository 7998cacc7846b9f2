// emu_oks.cpp — TEST INFRASTRUCTURE.  Compiles what the OKS kernels of similari_amd/csrc/sa_pose.hip call — sa_pose_oks.h over
// sa_pose_gate.h's rectangle, with sa_pose.h's weight rule — with g++, so that exp, the area, the scale and the cell function can be
// compared with tests/oks_ref.py on a machine without a GPU.  The product never links this file.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/similari_assoc.h"
#include "../../similari_amd/csrc/sa_pose.h"
#include "../../similari_amd/csrc/sa_pose_oks.h"

extern "C" {

void emu_oks_exp(uint64_t n, const float* e, float* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = sa_oks_exp(e[i]);
}
void emu_oks_var2(uint32_t n, const float* sigma, float* out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = sa_oks_var2(sigma[i]);
}
// n items of P points xy [n][P][2], counts [n][P] -> area [n], the walk of k_pose_circles
void emu_oks_area(uint32_t n, uint32_t P, const float* xy, const uint8_t* counts, float* out) {
  for (size_t i = 0; i < n; ++i) {
    sa_pose_rect q;
    sa_pose_rect_clear(q);
    for (size_t p = 0; p < P; ++p)
      if (counts[i * P + p]) sa_pose_rect_add(q, xy[(i * P + p) * 2], xy[(i * P + p) * 2 + 1]);
    out[i] = sa_oks_area(q);
  }
}
// poses [M][P][2], present [M][P]; has [T][P], mean [T][P][4]; var2 [P] -> w [M][T], NaN = no pair: the extents, then per cell the tile's walk
void emu_oks_matrix(uint32_t M, uint32_t T, uint32_t P, const float* poses, const uint8_t* present, const uint8_t* has, const float* mean,
                    const float* var2, uint32_t min_common, float* w) {
  std::vector<float> pa(M), ta(T);
  emu_oks_area(M, P, poses, present, pa.data());
  for (size_t j = 0; j < T; ++j) {
    sa_pose_rect q;
    sa_pose_rect_clear(q);
    for (size_t p = 0; p < P; ++p)
      if (has[j * P + p]) sa_pose_rect_add(q, mean[(j * P + p) * 4], mean[(j * P + p) * 4 + 1]);
    ta[j] = sa_oks_area(q);
  }
  for (size_t i = 0; i < M; ++i)
    for (size_t j = 0; j < T; ++j) {
      const float s2 = sa_oks_scale(pa[i], ta[j]);
      float sum = 0.f;
      uint32_t k = 0;
      for (size_t p = 0; p < P; ++p)
        sa_oks_acc(sum, k, has[j * P + p] != 0, mean[(j * P + p) * 4], mean[(j * P + p) * 4 + 1], present[i * P + p] != 0, poses[(i * P + p) * 2],
                   poses[(i * P + p) * 2 + 1], s2, var2[p]);
      float v = sa_pose_weight(sum, k, min_common);
      if (sa_oks_refused(s2)) v = NAN;
      w[i * T + j] = v;
    }
}

}  // extern "C"
