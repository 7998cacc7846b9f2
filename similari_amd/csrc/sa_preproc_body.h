// sa_preproc_body.h — the statements of the frame-preprocessing kernels (NMS pair mask, NMS sweep, own areas and their spill path),
// included as text INSIDE the kernels that run them (sa_upkeep.hip): the single-scene kernel and its *_set twin, which runs the same
// statements on the scene a segment table names.  Text and no __device__ function for the reason sa_tail.h gives for sa_tail_body.h:
// inlined from a function of their own the statements compile to other instructions, and the single-scene kernels are to stay the
// kernels they were.  SA_PREPROC_BODY selects the body; each one lists the names the including kernel must have in scope, and its
// `return`s leave that kernel.
#define SA_BODY_NMS_MASK 1
#define SA_BODY_NMS_SWEEP 2
#define SA_BODY_OWN_AREA 3
#define SA_BODY_OWN_AREA_BIG 4
#if SA_PREPROC_BODY == SA_BODY_NMS_MASK   // in scope: raw, n, W, thr, mask of ONE scene; blockIdx.x / blockIdx.y = the word column / the 16-row band inside it
  const uint32_t i0 = blockIdx.y * 16, j0 = blockIdx.x * 64;
  if (i0 >= n || j0 >= n) return;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  __shared__ unsigned long long s_bits[16];
  if (j0 + 63 <= i0) {  // the whole word lies on or below the diagonal: no pair with i < j
    if (tid < 16 && i0 + tid < n) mask[(size_t)(i0 + tid) * W + blockIdx.x] = 0ull;
    return;
  }
  __shared__ sa_geo s_rg[16], s_cg[64];
  __shared__ double s_rv[16][8], s_cv[64][8];
  __shared__ float s_carea[64];
  __shared__ uint16_t s_list[16 * 64];
  __shared__ uint32_t s_cnt;
  __shared__ double s_poly[4 * SA_POLY_CAP * 64];
  if (tid < 16) {
    s_bits[tid] = 0ull;
    const uint32_t i = i0 + tid;
    if (i < n) {
      const BoxRaw r = raw[i];
      sa_geo g;
      g.xc = r.box.xc; g.yc = r.box.yc; g.r = sa_radius(r.box.aspect, r.box.height); g.hha = 0.f;
      s_rg[tid] = g;
      sa_vertices(r.box.xc, r.box.yc, r.box.aspect, r.box.height, r.c, r.s, s_rv[tid]);
    }
  } else if (tid >= 64 && tid < 128) {
    const uint32_t lj = tid - 64, j = j0 + lj;
    if (j < n) {
      const BoxRaw r = raw[j];
      sa_geo g;
      g.xc = r.box.xc; g.yc = r.box.yc; g.r = sa_radius(r.box.aspect, r.box.height); g.hha = 0.f;
      s_cg[lj] = g;
      sa_vertices(r.box.xc, r.box.yc, r.box.aspect, r.box.height, r.c, r.s, s_cv[lj]);
      s_carea[lj] = sa_area(r.box.aspect, r.box.height);
    }
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t li = wave * 4 + r, i = i0 + li, j = j0 + lane;
    if (i < n && j < n && i < j) {
      if (!sa_too_far(s_rg[li], s_cg[lane])) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        s_list[slot] = (uint16_t)((li << 8) | lane);
      } else if (0.0f > thr) {  // intersection() is 0.0 for far boxes: 0 / area still beats a negative threshold
        atomicOr(&s_bits[li], 1ull << lane);
      }
    }
  }
  __syncthreads();
  const uint32_t cnt = s_cnt;
  if (tid < 64) {
    double* ws = s_poly + tid;
    for (uint32_t sidx = tid; sidx < cnt; sidx += 64) {
      const uint32_t c = s_list[sidx], li = c >> 8, lj = c & 255u;
      double sv[8], cv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { sv[k] = s_rv[li][k]; cv[k] = s_cv[lj][k]; }
      const double inter = sa_clip_area_ws(sv, cv, ws, 64);
      const float metric = (float)inter / s_carea[lj];
      if (metric > thr) atomicOr(&s_bits[li], 1ull << lj);
    }
  }
  __syncthreads();
  if (tid < 16 && i0 + tid < n) mask[(size_t)(i0 + tid) * W + blockIdx.x] = s_bits[tid];
#elif SA_PREPROC_BODY == SA_BODY_NMS_SWEEP   // in scope: S (constant), mask, n, W, keep of ONE scene; one wave
  const uint32_t lane = threadIdx.x;
  uint64_t rw[S];
#pragma unroll
  for (int s = 0; s < S; ++s) rw[s] = 0ull;
  constexpr int B = 16;
  for (uint32_t i0 = 0; i0 < n; i0 += B) {
    uint64_t rows[B][S];
#pragma unroll
    for (int r = 0; r < B; ++r)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const uint32_t w = s * 64 + lane;
        rows[r][s] = (i0 + r < n && w < W) ? mask[(size_t)(i0 + r) * W + w] : 0ull;
      }
#pragma unroll
    for (int r = 0; r < B; ++r) {
      const uint32_t i = i0 + r;
      if (i >= n) break;
      const uint32_t word = i >> 6, owner = word & 63u, slot = word >> 6, bit = i & 63u;
      uint64_t mine = rw[0];
#pragma unroll
      for (int s = 1; s < S; ++s) mine = slot == (uint32_t)s ? rw[s] : mine;
      const uint64_t cur = __shfl(mine, (int)owner);
      const bool removed = (cur >> bit) & 1ull;
      if (!removed) {
#pragma unroll
        for (int s = 0; s < S; ++s) rw[s] |= rows[r][s];
      }
      if (lane == 0) keep[i] = removed ? 0 : 1;
    }
  }
#elif SA_PREPROC_BODY == SA_BODY_OWN_AREA   // in scope: raw, n, share, status of ONE scene, i = the box inside it, lane
  __shared__ double s_poly[(SA_OWN_MAXNB + 1) * 8];
  __shared__ double s_iva[SA_OWN_CAP * 64], s_ivb[SA_OWN_CAP * 64];
  __shared__ uint32_t s_cnt;
  const BoxRaw me = raw[i];
  sa_geo mg;
  mg.xc = me.box.xc; mg.yc = me.box.yc; mg.r = sa_radius(me.box.aspect, me.box.height); mg.hha = 0.f;
  double mv[8];
  sa_vertices(me.box.xc, me.box.yc, me.box.aspect, me.box.height, me.c, me.s, mv);
  const double ox = (double)me.box.xc, oy = (double)me.box.yc;
  if (lane < 8) s_poly[lane] = mv[lane] - ((lane & 1u) ? oy : ox);
  if (lane == 0) s_cnt = 1;
  __syncthreads();
  bool overflow = false;
  for (uint32_t j0 = 0; j0 < n; j0 += 64) {
    const uint32_t j = j0 + lane;
    if (j < n && j != i) {
      const BoxRaw r = raw[j];
      sa_geo g;
      g.xc = r.box.xc; g.yc = r.box.yc; g.r = sa_radius(r.box.aspect, r.box.height); g.hha = 0.f;
      if (!sa_too_far(mg, g)) {
        double v[8];
        sa_vertices(r.box.xc, r.box.yc, r.box.aspect, r.box.height, r.c, r.s, v);
        if (!sa_quads_separated(mv, v)) {
          const uint32_t slot = atomicAdd(&s_cnt, 1u);
          if (slot <= SA_OWN_MAXNB) {
#pragma unroll
            for (int k = 0; k < 8; ++k) s_poly[slot * 8 + k] = v[k] - ((k & 1) ? oy : ox);
          } else {
            overflow = true;
          }
        }
      }
    }
  }
  __syncthreads();
  if (__any(overflow)) {
    if (lane == 0) { share[i] = NAN; atomicOr(status, 1u); }
    return;
  }
  const uint32_t m1 = s_cnt;
  double acc = 0.0;
  for (uint32_t e = lane; e < m1 * 4; e += 64)
    acc += sa_own_edge(s_poly, m1, e >> 2, e & 3u, s_iva + lane, s_ivb + lane, 64, SA_OWN_CAP);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    if (acc != acc) atomicOr(status, 2u);
    const double own = fabs(acc) * 0.5;
    const float e = (float)(own / (double)(sa_area(me.box.aspect, me.box.height) + SA_EPS));
    share[i] = acc != acc ? NAN : (e >= 1.0f ? 1.0f : e);  // NaN = "not done here": the spill path takes the box
  }
#elif SA_PREPROC_BODY == SA_BODY_OWN_AREA_BIG   // in scope: raw, n, share, status of ONE scene, i, lane, s_poly / s_iva / s_ivb = the block's HBM scratch
  __shared__ uint32_t s_cnt;
  const BoxRaw me = raw[i];
  sa_geo mg;
  mg.xc = me.box.xc; mg.yc = me.box.yc; mg.r = sa_radius(me.box.aspect, me.box.height); mg.hha = 0.f;
  double mv[8];
  sa_vertices(me.box.xc, me.box.yc, me.box.aspect, me.box.height, me.c, me.s, mv);
  const double ox = (double)me.box.xc, oy = (double)me.box.yc;
  if (lane < 8) s_poly[lane] = mv[lane] - ((lane & 1u) ? oy : ox);
  if (lane == 0) s_cnt = 1;
  __syncthreads();
  for (uint32_t j0 = 0; j0 < n; j0 += 64) {
    const uint32_t j = j0 + lane;
    if (j < n && j != i) {
      const BoxRaw r = raw[j];
      sa_geo g;
      g.xc = r.box.xc; g.yc = r.box.yc; g.r = sa_radius(r.box.aspect, r.box.height); g.hha = 0.f;
      if (!sa_too_far(mg, g)) {
        double v[8];
        sa_vertices(r.box.xc, r.box.yc, r.box.aspect, r.box.height, r.c, r.s, v);
        if (!sa_quads_separated(mv, v)) {
          const uint32_t slot = atomicAdd(&s_cnt, 1u);  // at most n - 1 neighbours: always room
#pragma unroll
          for (int k = 0; k < 8; ++k) s_poly[(size_t)slot * 8 + k] = v[k] - ((k & 1) ? oy : ox);
        }
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  const uint32_t m1 = s_cnt;
  double acc = 0.0;
  for (uint32_t e = lane; e < m1 * 4; e += 64)
    acc += sa_own_edge(s_poly, m1, e >> 2, e & 3u, s_iva + lane, s_ivb + lane, 64, SA_OWN_BIGCAP);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) {
    if (acc != acc) atomicOr(status, 4u);
    const double own = fabs(acc) * 0.5;
    const float e = (float)(own / (double)(sa_area(me.box.aspect, me.box.height) + SA_EPS));
    share[i] = acc != acc ? NAN : (e >= 1.0f ? 1.0f : e);
  }
#endif
#undef SA_PREPROC_BODY
