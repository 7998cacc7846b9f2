// emu_points.cpp — TEST INFRASTRUCTURE.  Compiles the product's point Kalman filter (similari_amd/csrc/sa_kalman_point.h, the exact
// source the HIP kernel of sa_points.hip calls) with g++, so that its arithmetic can be compared with tests/points_ref.py on a machine
// without a GPU, and so that scripts/bench_points.py has the same arithmetic on one host core as its yardstick.  The product never
// links this file.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/similari_assoc.h"
#include "../../similari_amd/csrc/sa_kalman_point.h"

namespace {
void get(const float* mean, const float* cov, size_t i, sa_pkf& s) {
  std::memcpy(s.mean, mean + i * 4, sizeof s.mean);
  std::memcpy(s.cov, cov + i * 16, sizeof s.cov);
}
void put(float* mean, float* cov, size_t i, const sa_pkf& s) {
  std::memcpy(mean + i * 4, s.mean, sizeof s.mean);
  std::memcpy(cov + i * 16, s.cov, sizeof s.cov);
}
}  // namespace

extern "C" {

// n states, mean [n][4] and cov [n][16] in place; z [n][2]
void emu_pt_initiate(float pw, float vw, uint32_t n, const float* z, float* mean, float* cov) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    sa_pkf_initiate(pw, vw, z[i * 2], z[i * 2 + 1], s);
    put(mean, cov, i, s);
  }
}
void emu_pt_predict(float pw, float vw, uint32_t n, float* mean, float* cov) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    get(mean, cov, i, s);
    sa_pkf_predict(pw, vw, s);
    put(mean, cov, i, s);
  }
}
void emu_pt_update(float pw, uint32_t n, const float* z, float* mean, float* cov) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    get(mean, cov, i, s);
    sa_pkf_update(pw, s, z[i * 2], z[i * 2 + 1]);
    put(mean, cov, i, s);
  }
}
// mode 0: d^2, 1: calculate_cost(d^2, false), 2: calculate_cost(d^2, true)
void emu_pt_distance(float pw, uint32_t n, const float* z, const float* mean, const float* cov, uint32_t mode, float* out) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    get(mean, cov, i, s);
    float d = sa_pkf_distance(pw, s, z[i * 2], z[i * 2 + 1]);
    if (mode) d = sa_pkf_cost(d, mode == 2);
    out[i] = d;
  }
}
// pts [n][comps]; min_score; mask [n] or null -> out [n] 0 / 1
void emu_pt_present(uint32_t n, uint32_t comps, const float* pts, float min_score, const uint8_t* mask, uint8_t* out) {
  for (size_t i = 0; i < n; ++i)
    out[i] = sa_point_present(pts[i * comps], pts[i * comps + 1], comps == 3, comps == 3 ? pts[i * comps + 2] : 0.0f, min_score, !mask || mask[i]);
}
// The loop a tracker runs, as one host core runs it: has [n] in place, z [n][2], present [n]; xy [n][2] or null.
void emu_pt_step(float pw, float vw, uint32_t n, const float* z, const uint8_t* present, uint8_t* has, float* mean, float* cov, float* xy) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    if (has[i]) get(mean, cov, i, s);
    const bool h = sa_pkf_step(pw, vw, has[i] != 0, s, present[i] != 0, z[i * 2], z[i * 2 + 1]);
    has[i] = h;
    if (h) put(mean, cov, i, s);
    if (xy) {
      xy[i * 2] = h ? s.mean[0] : NAN;
      xy[i * 2 + 1] = h ? s.mean[1] : NAN;
    }
  }
}

}  // extern "C"
