// emu_pose.cpp — TEST INFRASTRUCTURE.  Compiles what the kernels of similari_amd/csrc/sa_pose.hip call — sa_pose.h over
// sa_kalman_point.h, and the dense solver sa_dense.h through its host path — with g++, so that the pair weight and the whole-scene
// assignment route can be compared with tests/pose_ref.py on a machine without a GPU, and so that scripts/bench_pose.py has the same
// arithmetic on one host core as its yardstick.  The product never links this file.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/similari_assoc.h"
#include "../../similari_amd/csrc/sa_pose.h"
#include "../../similari_amd/csrc/sa_dense.h"

namespace {
void get(const float* mean, const float* cov, size_t i, sa_pkf& s) {
  std::memcpy(s.mean, mean + i * 4, sizeof s.mean);
  std::memcpy(s.cov, cov + i * 16, sizeof s.cov);
}
}  // namespace

extern "C" {

// n states -> fac [n][5] (mean x, y, l00, l10, l11) and ok [n]; what a failed pivot leaves unwritten reads 0
void emu_pose_factor(float pw, uint32_t n, const float* mean, const float* cov, float* fac, uint8_t* ok) {
  for (size_t i = 0; i < n; ++i) {
    sa_pkf s;
    get(mean, cov, i, s);
    sa_pkf_fac f{0.f, 0.f, 0.f, 0.f, 0.f};
    ok[i] = sa_pkf_factor(pw, s, f);
    const float v[5] = {f.mx, f.my, f.l00, f.l10, f.l11};
    std::memcpy(fac + i * 5, v, sizeof v);
  }
}
// factor i and z [n][2] -> d2 [n], NaN where there is no factor
void emu_pose_distance_factored(uint32_t n, const float* fac, const uint8_t* ok, const float* z, float* out) {
  for (size_t i = 0; i < n; ++i) {
    const sa_pkf_fac f{fac[i * 5], fac[i * 5 + 1], fac[i * 5 + 2], fac[i * 5 + 3], fac[i * 5 + 4]};
    out[i] = ok[i] ? sa_pkf_distance_factored(f, z[i * 2], z[i * 2 + 1]) : NAN;
  }
}

// The cells of a scene as the kernels sequence them: the factor once per (track, point), then every cell walks p ascending.
// poses [M][P][2], present [M][P]; has [T][P], mean [T][P][4], cov [T][P][16] -> w [M][T], NaN = no pair
void emu_pose_matrix(float pw, uint32_t M, uint32_t T, uint32_t P, const float* poses, const uint8_t* present, const uint8_t* has,
                     const float* mean, const float* cov, uint32_t min_common, float* w) {
  std::vector<sa_pkf_fac> fac((size_t)T * P);
  std::vector<uint8_t> ok((size_t)T * P);
  for (size_t t = 0; t < (size_t)T * P; ++t) {
    ok[t] = 0;
    if (!has[t]) continue;
    sa_pkf s;
    get(mean, cov, t, s);
    ok[t] = sa_pkf_factor(pw, s, fac[t]);
  }
  for (uint32_t i = 0; i < M; ++i)
    for (uint32_t j = 0; j < T; ++j) {
      float sum = 0.f;
      uint32_t k = 0;
      for (uint32_t p = 0; p < P; ++p) {
        const size_t zi = (size_t)i * P + p, tj = (size_t)j * P + p;
        sa_pose_acc(sum, k, ok[tj] != 0, fac[tj], present[zi] != 0, poses[zi * 2], poses[zi * 2 + 1]);
      }
      w[(size_t)i * T + j] = sa_pose_weight(sum, k, min_common);
    }
}

int64_t emu_pose_threshold_q(float threshold) { return sa_pose_threshold_q(threshold); }
int64_t emu_pose_gain(float w, int64_t threshold_q) { return sa_pose_gain(w, threshold_q); }

// The vote over w [M][T] as k_pose_tile and k_pose_assign sequence it: gains and the rows' bid words (the maximum the tile's atomics
// form), greedy start (a column goes to the lowest row that bids for it), the rows that lost their bid in ascending order, then
// sa_assign_component_dense<256, 8, false> over the whole scene as one component.  rmatch [M] = column or -1; returns 0, or a
// negative number when the matching is inconsistent.
int emu_pose_assign(uint32_t M, uint32_t T, const float* w, float threshold, int32_t* rmatch_out, int64_t* total_gain, uint32_t* n_roots) {
  if (T > 256u * 8u || M > 2048u) return -21;
  const int64_t thr = sa_pose_threshold_q(threshold);
  std::vector<int64_t> gain((size_t)M * (T ? T : 1), 0), u(M, 0);
  std::vector<unsigned long long> best(M, 0ull);
  for (uint32_t i = 0; i < M; ++i)
    for (uint32_t j = 0; j < T; ++j) {
      const int64_t g = sa_pose_gain(w[(size_t)i * T + j], thr);
      gain[(size_t)i * T + j] = g;
      const unsigned long long word = g > 0 ? sa_pose_word(g, j) : 0ull;
      best[i] = word > best[i] ? word : best[i];
    }
  std::vector<int32_t> rmatch(M, -1), cmatch(T, -1), pred(T, 0);
  std::vector<uint32_t> cwin(T, 0xffffffffu), roots;
  for (uint32_t i = 0; i < M; ++i) {
    u[i] = -sa_pose_word_gain(best[i]);
    rmatch[i] = best[i] ? (int32_t)sa_pose_word_col(best[i]) : -1;
    if (rmatch[i] >= 0 && i < cwin[rmatch[i]]) cwin[rmatch[i]] = i;
  }
  for (uint32_t i = 0; i < M; ++i) {
    if (rmatch[i] < 0) continue;
    if (cwin[rmatch[i]] == i) cmatch[rmatch[i]] = (int32_t)i;
    else {
      rmatch[i] = -1;
      roots.push_back(i);
    }
  }
  sa_dense_ws ws;
  ws.gain = gain.data(); ws.ld = T; ws.T = T;
  ws.u = u.data(); ws.rmatch = rmatch.data(); ws.cmatch = cmatch.data(); ws.pred = pred.data(); ws.part = nullptr;
  sa_assign_component_dense<256, 8, false>(ws, roots.data(), (uint32_t)roots.size());
  int64_t tot = 0;
  for (uint32_t i = 0; i < M; ++i) {
    rmatch_out[i] = rmatch[i];
    if (rmatch[i] < 0) continue;
    if ((uint32_t)rmatch[i] >= T) return -2;
    const int64_t g = gain[(size_t)i * T + rmatch[i]];
    if (g <= 0) return -9;
    if (cmatch[rmatch[i]] != (int32_t)i) return -1;
    tot += g;
  }
  if (total_gain) *total_gain = tot;
  if (n_roots) *n_roots = (uint32_t)roots.size();
  return 0;
}

}  // extern "C"
