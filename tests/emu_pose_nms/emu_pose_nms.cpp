// emu_pose_nms.cpp — TEST INFRASTRUCTURE.  Compiles what the kernels and the host path of similari_amd/csrc/sa_pose_nms.hip call —
// sa_pose_nms.h over sa_pose_oks.h — with g++, so that the filter, the rank, the pair matrix and the greedy pass can be compared with
// tests/pose_nms_ref.py on a machine without a GPU, and timed on one core by scripts/bench_pose_nms.py.  The product never links this
// file.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/similari_assoc.h"
#include "../../similari_amd/csrc/sa_pose_nms.h"

extern "C" {

// One scene: pts [m][P][comps] f32, present [m][P] or NULL, scores [m], sigmas [P].  -> out_order [m'] the caller's indices in rank
// order, *out_m = m'; out_w NULL or [m'][m'] (w for i < j, NaN elsewhere); out_keep [*out_n] the survivors in rank order.
void emu_pose_nms(uint32_t m, uint32_t P, uint32_t comps, const float* pts, const uint8_t* present, float min_score, const float* scores,
                  const float* sigmas, uint32_t min_common, float nms_threshold, float score_threshold, uint32_t* out_order, uint32_t* out_m,
                  float* out_w, uint32_t* out_keep, uint32_t* out_n) {
  std::vector<uint32_t> src;
  sa_pose_nms_rank(m, scores, score_threshold, src);
  const uint32_t n = (uint32_t)src.size();
  std::vector<float> var2(P), area(n);
  for (uint32_t p = 0; p < P; ++p) var2[p] = sa_oks_var2(sigmas[p]);
  // k_pose_nms_lay: the points point-major in rank order, the areas
  std::vector<sa_xy> z((size_t)P * n);
  for (uint32_t t = 0; t < n; ++t) {
    const float* row = pts + (size_t)src[t] * P * comps;
    for (uint32_t p = 0; p < P; ++p)
      z[(size_t)p * n + t] = sa_pose_nms_point(row[p * comps], row[p * comps + 1], comps == 3, comps == 3 ? row[p * comps + 2] : 0.f, min_score,
                                               !present || present[(size_t)src[t] * P + p] != 0);
    area[t] = sa_pose_nms_area(z.data() + t, n, P);
  }
  auto w = [&](uint32_t i, uint32_t j) {
    return sa_pose_nms_pair(P, var2.data(), min_common, z.data() + i, n, area[i], z.data() + j, n, area[j]);
  };
  for (uint32_t t = 0; t < n; ++t) out_order[t] = src[t];
  *out_m = n;
  std::vector<uint8_t> keep(n);
  if (out_w) {
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t j = 0; j < n; ++j) out_w[(size_t)i * n + j] = i < j ? w(i, j) : NAN;
    sa_pose_nms_greedy(n, nms_threshold, [&](uint32_t i, uint32_t j) { return out_w[(size_t)i * n + j]; }, keep.data());
  } else
    sa_pose_nms_greedy(n, nms_threshold, w, keep.data());
  uint32_t k = 0;
  for (uint32_t t = 0; t < n; ++t)
    if (keep[t]) out_keep[k++] = src[t];
  *out_n = k;
}

}  // extern "C"
