// sa_tail_body.h — the statements of the one-workgroup assignment tail, included as text INSIDE the kernels that run them
// (k_assign_small, sa_kernels.hip; k_frame_visual<.., HELP, TAIL>, sa_gemm.hip).  Not a header of its own: sa_tail.h says why it is text
// and no __device__ function, which names the including kernel must have in scope, and that its `return`s leave that kernel.
  static_assert(!LAZY || (VISUAL && WORDS && TC == 1), "the lazy positional phase: single vote words on the one-column-per-thread form");
  static_assert(!FUSED || LAZY, "behind the tiles of its own launch: the lazy form only");
  const SceneDev S = scenes[blockIdx.z];  // by value: wave-uniform SGPRs, cannot alias the stores below
  const uint32_t N = S.N, T = S.T;
  const uint32_t q = threadIdx.x;
  constexpr uint32_t TCAP = (uint32_t)TC * SA_SMALL_N;   // columns this instantiation holds
  constexpr int DNT = SA_DENSE_NT * TC;                  // threads of the dense solver: four columns each (eight per thread cost the two-column form spilled registers)
  __shared__ uint32_t s_done;   // waves that have reported (sa_report_done)
  __shared__ uint32_t s_head[SA_SMALL_N];  // per component root: the rows that lost their greedy bid (pushed in any order)
  __shared__ uint32_t s_next[SA_SMALL_N];
  __shared__ int64_t s_u[SA_SMALL_N], s_v[TCAP], s_dist[TCAP];
  __shared__ int32_t s_rmatch[SA_SMALL_N], s_cmatch[TCAP], s_pred[TCAP];
  __shared__ uint32_t s_cstamp[TCAP], s_cscan[TCAP];
  __shared__ uint32_t s_lab[SA_SMALL_N];     // component root of a row with usable edges
  __shared__ uint32_t s_cwin[TCAP];          // per column: lowest row bidding for it
  __shared__ uint32_t s_rcount[SA_SMALL_N];  // per component root: search roots
  __shared__ uint32_t s_ccount[SA_SMALL_N];  // per component root: columns
  __shared__ uint32_t s_clist[TCAP];         // labelled columns of the running searches, one segment per component
  __shared__ uint32_t s_rlist[SA_SMALL_N];   // search roots in ascending order, one segment per component
  __shared__ uint32_t s_queue[SA_SMALL_N];   // components waiting for a group
  __shared__ uint32_t s_ctr[8];              // queue length | next queue entry | top of s_clist | top of s_rlist | dense queue length
  __shared__ unsigned long long s_part[2 * (DNT / 64)];  // the dense solver's per-wave minima (sa_wg_min_u64)
  // The edge lists the positional tiles left behind live in HBM, one strided row per candidate: every access from here on would be
  // a dependent, uncoalesced round trip (the solve is a chain of them).  They are packed ONCE into an LDS pool — an
  // exclusive scan of the row counts gives the offsets — and the row duals, the connected components of the usable graph
  // (rows without a visual verdict) and the solve itself then run out of LDS.  A scene whose lists do not fit (dense
  // Mahalanobis frames, crowds under a low threshold) keeps the HBM lists as the solver's edge storage.
  constexpr uint32_t POOL = TC == 1 ? 3072 : 0;   // (two columns per thread: the pool's 36 KB are the second half of the column arrays)
  __shared__ uint32_t s_parent[SA_SMALL_N + TCAP];
  __shared__ uint32_t s_ecnt[SA_SMALL_N], s_eoff[SA_SMALL_N], s_wsum[SA_SMALL_N / WAVE];
  __shared__ uint32_t s_ecol[POOL ? POOL : 1];
  __shared__ int64_t s_egain[POOL && !FUSED ? POOL : 1];
  int64_t* const egain = FUSED ? egain_ext : s_egain;   // (FUSED: inside the tile's buffer)
  TAIL_STAMP(0);
  uint32_t rawcnt = (!LAZY && q < N) ? S.e_cnt[q] : 0u;   // (LAZY: the phase below counts the edges it appends)
  if (q == 0) {  // what the first phase raised goes out with the results; re-armed for the next frame
    // (FUSED: a plain load beside tiles of the same launch is safe here — only euclidean tiles raise stats[0], and the form is cosine only)
    SA_OUT(S.out_stats + 0, S.stats[0]);
    SA_OUT(S.out_stats + 1, 0u);   // (k_assign_solve: a bounded wait ran out — the host refuses the frame's results)
    S.stats[0] = 0u;
    s_done = 0u;           // (barriers follow before any wave can leave)
  }
  __shared__ uint8_t s_cexcl[WORDS ? TCAP : 4];         // excluded_tracks as bytes, for the solver's HBM-list variant
  __shared__ uint32_t s_bt[WORDS ? SA_SMALL_N : 1];     // candidate -> its best column (SA_NONE: no group at all)
  __shared__ uint32_t s_cq[WORDS ? TCAP : 1];           // column -> its best candidate (SA_NONE: no group at all)
  bool has_verdict;
  int32_t vw0 = -1;
  uint32_t bt = SA_NONE;
  // SCN_WORDSK (deeper banks through the whole-track tiles of the contraction, sa_gemm.hip): K words per candidate and per track, one per count class —
  // (key of the f32 sum of the group's weights << 32 | index).  Whether a candidate has ANY group is known at once (it decides
  // whether the row takes part in the positional vote); WHICH group wins needs the frame's max_dist: W = c max_dist - sum, heaviest
  // wins, lowest index among equals — folded from the first phase's per-tile slots by this workgroup (one slot per thread, the
  // wave maxima through LDS at the barrier that is there anyway), then one more barrier for the two tables.
  __shared__ uint32_t s_wmk[WORDS ? SA_SMALL_N / WAVE : 1];
  unsigned long long rcls[WORDS ? SA_CLS_MAXK : 1], ccls[TC][WORDS ? SA_CLS_MAXK : 1];
  bool clsmode = false;
  if constexpr (WORDS && !LAZY) clsmode = (S.flags & SCN_WORDSK) != 0;
  if constexpr (WORDS) if (clsmode) {
    const uint32_t K = S.K;
    bool any = false;
    // (the first phase's max-key slots are requested FIRST, so that they travel with the class words: behind the words' processing the
    // loop below was a second trip to memory — one of the ~3 us the class-word tail took over the single-word one)
    uint32_t mk = 0, mk0 = q < S.nkeys ? S.vis_max_key[q] : 0u;
#pragma unroll
    for (uint32_t c = 0; c < SA_CLS_MAXK; ++c) {
      // all 2 x SA_CLS_MAXK loads issued together, whatever K is (the clamped index re-reads a word that is needed anyway): with the
      // load inside `c < K ? ... : ~0` every class became a scalar branch with its own load + s_waitcnt vmcnt(0) — K round trips
      // to memory one after the other, ~1 us per class
      rcls[c] = S.row_cls[(size_t)(q < N ? q : 0u) * K + (c < K ? c : K - 1u)];
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) {
        const uint32_t j = q + (uint32_t)cc * SA_SMALL_N;
        ccls[cc][c] = S.col_cls[(size_t)(j < T ? j : 0u) * K + (c < K ? c : K - 1u)];
      }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (uint32_t c = 0; c < SA_CLS_MAXK; ++c) {
      rcls[c] = (c < K && q < N) ? rcls[c] : ~0ull;
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) ccls[cc][c] = (c < K && q + (uint32_t)cc * SA_SMALL_N < T) ? ccls[cc][c] : ~0ull;
    }
#pragma unroll
    for (uint32_t c = 0; c < SA_CLS_MAXK; ++c) {
      if (rcls[c] != ~0ull) S.row_cls[(size_t)q * K + c] = ~0ull;  // re-armed (most classes of a row are empty: nothing to store)
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) {
        const uint32_t j = q + (uint32_t)cc * SA_SMALL_N;
        if (ccls[cc][c] != ~0ull) S.col_cls[(size_t)j * K + c] = ~0ull;
      }
      if (S.tap_row_best && c < K) {  // SA_FLAG_TAP: the class words as the first phase left them ([N K] then [T K])
        if (q < N) S.tap_row_best[(size_t)q * K + c] = rcls[c];
#pragma unroll
        for (int cc = 0; cc < TC; ++cc) {
          const uint32_t j = q + (uint32_t)cc * SA_SMALL_N;
          if (j < T) S.tap_col_best[(size_t)j * K + c] = ccls[cc][c];
        }
      }
      any = any || rcls[c] != ~0ull;
    }
    mk = mk0;
    for (uint32_t i = q + SA_SMALL_N; i < S.nkeys; i += SA_SMALL_N) {   // (more than 1024 tiles: frames beyond this tail's reach today)
      const uint32_t v = S.vis_max_key[i];
      mk = v > mk ? v : mk;
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const uint32_t ok = __shfl_xor(mk, o);
      mk = ok > mk ? ok : mk;
    }
    if (q % WAVE == 0) s_wmk[q / WAVE] = mk;
    has_verdict = any;  // feature_winners.contains_key(q)
    s_bt[q] = SA_NONE;  // (rows / columns beyond N / T)
#pragma unroll
    for (int cc = 0; cc < TC; ++cc) s_cq[q + (uint32_t)cc * SA_SMALL_N] = SA_NONE;
  }
  if constexpr (WORDS) {
   if (!clsmode) {
    // (weight key << 32 | index), all ones = no group at all; lowest weight wins, lowest index on ties — k_bestfit_resolve's order
    unsigned long long rb = ~0ull, cb[TC];
    if constexpr (FUSED) {
      // the words as the tiles of THIS launch left them: fetched and re-armed by one agent-scope exchange each (see FUSED above)
      if (q < N) rb = __hip_atomic_exchange(S.row_best + q, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cb[0] = q < T ? __hip_atomic_exchange(S.col_best + q, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    } else {
      rb = q < N ? S.row_best[q] : ~0ull;
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) { const uint32_t j = q + (uint32_t)cc * SA_SMALL_N; cb[cc] = j < T ? S.col_best[j] : ~0ull; }
    }
    // LAZY: the track id a winning row will report, requested with the words and parked in LDS behind the barrier that is there anyway
    // (s_dist: nothing has written it yet) — a frame that the vote decides whole (the fast exit below) then makes no dependent trip for it
    if constexpr (LAZY) s_dist[q] = q < T ? (int64_t)S.t_ids[q] : 0;
    if constexpr (!FUSED) {
      if (q < N) S.row_best[q] = ~0ull;
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) { const uint32_t j = q + (uint32_t)cc * SA_SMALL_N; if (j < T) S.col_best[j] = ~0ull; }
    }
    if (S.tap_row_best) {  // SA_FLAG_TAP: the words as the first phase left them
      if (q < N) S.tap_row_best[q] = rb;
#pragma unroll
      for (int cc = 0; cc < TC; ++cc) { const uint32_t j = q + (uint32_t)cc * SA_SMALL_N; if (j < T) S.tap_col_best[j] = cb[cc]; }
    }
    const uint32_t imask = (S.flags & SCN_WORDS10) ? 1023u : 0xffffffffu;  // deeper banks: (inverted weight key << 10) | index, k_bestfit_tile
    bt = rb != ~0ull ? ((uint32_t)rb & imask) : SA_NONE;
    has_verdict = bt != SA_NONE;  // feature_winners.contains_key(q)
    s_bt[q] = bt;
#pragma unroll
    for (int cc = 0; cc < TC; ++cc) s_cq[q + (uint32_t)cc * SA_SMALL_N] = cb[cc] != ~0ull ? ((uint32_t)cb[cc] & imask) : SA_NONE;
   }
  } else {
    has_verdict = VISUAL && q < N && S.row_has[q];
    vw0 = (VISUAL && q < N) ? S.vis_winner[q] : -1;  // with the first round trip, not after the scan
  }
  // excluded_tracks: column j was won by the candidate that is best in it iff that candidate's own best column is j
  auto excluded = [&](uint32_t j) -> bool {
    if constexpr (WORDS) {
      const uint32_t c = s_cq[j];
      return c != SA_NONE && s_bt[c] == j;
    } else return S.col_excluded[j] != 0;
  };
  // The lazy positional phase.  A positional cell counts only for a row without a visual group and a column no visual winner took
  // (visual_sort/voting.rs:72-79): this phase evaluates exactly those cells, leftover rows x non-excluded columns, with the positional
  // tiles' operations in their order (sa_box_geo / prep_box_common, sa_too_far, sa_compatible, sa_aa_quick_reject — conservative, so
  // it only drops cells that are absent anyway —, clip_area_lanes<8>, sa_iou_from_area, confidence, sa_quantise, the diagonal): the
  // same edges, bit for bit.  They go onto the row's HBM list exactly as the tiles append them (slot-major, counted here instead of
  // in e_cnt, which stays zero), so that everything below — scan, pool packing or the HBM-list solver, the taps — runs unchanged.
  // Thread q screens column q against every leftover row; the survivors (one list for the frame) are clipped by LZ_GROUPS groups of
  // eight lanes.  The LDS it uses belongs to arrays nothing has written yet: the leftover rows in s_rlist, per-row edge counts in
  // s_cscan, the survivors in the edge pool's columns, the clipping groups' vertex lists in its gains.  No leftover row (a tracking
  // frame whose every detection matched visually): one uniform branch.
  // LAZY: this thread's column's operands of the positional screen, requested behind the vote words (whose verdicts are awaited first) and
  // in flight across the leftover rows' compaction
  sa_geo lz_tg{0.f, 0.f, 0.f, 0.f};
  sa_ext lz_tx{-1.f, 0.f};
  uint64_t lz_te = 0;
  if (LAZY && q < T) { lz_tg = sa_ldg(S.t_geo + q); lz_tx = sa_ldg(S.t_ext + q); lz_te = S.t_epoch[q]; }
  if constexpr (LAZY) {
    constexpr uint32_t LZ_CAP = POOL, LZ_L = 8, LZ_WS = 4 * SA_POLY_CAP + 8, LZ_GROUPS = 48;
    static_assert(LZ_GROUPS * LZ_WS * sizeof(double) <= POOL * sizeof(int64_t) && LZ_CAP >= SA_SMALL_N, "the lazy phase's LDS");
    uint32_t* const s_lrow = s_rlist;
    uint32_t* const s_lcnt = s_cscan;
    uint32_t* const s_lsurv = s_ecol;
    double* const s_lws = (double*)egain;
    s_lcnt[q] = 0u;
    if (q == 0) { s_ctr[5] = 0u; s_ctr[6] = 0u; }
    sa_lds_barrier();   // (and every row's and column's verdict is in s_bt / s_cq)
    if (q < N && !has_verdict) s_lrow[atomicAdd(&s_ctr[6], 1u)] = q;
    sa_lds_barrier();
    const uint32_t nl = s_ctr[6];
    if (nl == 0) {
      // The fast exit: no leftover row — the visual vote has decided the whole frame (a tracking frame whose every detection matched).
      // Straight to the results: no solver state to set up, no scan, no edge; what the slow path would have written, it writes — no
      // leftover rows (out_stats[2]), no edge records (the tap), and each row its column's id out of the table parked above.
      if (q == 0) SA_OUT(S.out_stats + 2, 0u);
      if (q < N) {
        if (S.tap_ecnt) S.tap_ecnt[q] = 0u;
        const int32_t vw = (has_verdict && s_cq[bt] == q) ? (int32_t)bt : -1;   // the candidate that is best in its own best column wins it
        SA_OUT(S.out_track_id + q, vw >= 0 ? (uint64_t)s_dist[vw] : 0ull);
        SA_OUT(S.out_vote + q, vw >= 0 ? SA_VOTE_VISUAL : SA_VOTE_NONE);
        S.win_col[q] = vw;
        SA_OUT(S.out_win + q, vw);
      }
      sa_report_done(S, done_seq, &s_done);
      TAIL_STAMP(7);
      return;
    }
    if (T) {
      // the screen: thread q = column q against every leftover row of [r0, r1) (its track's operands requested above); survivors
      // onto the list while it has room — the count goes on, so that a list that overflowed is known
      const bool col_in = q < T && !excluded(q);
      const uint64_t epoch = S.epoch;
      auto screen = [&](uint32_t r0, uint32_t r1) {
        if (!col_in) return;
        for (uint32_t l0 = r0; l0 < r1; l0 += 4) {
          sa_box bx[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) bx[k] = sa_ldg(S.c_raw + s_lrow[l0 + k < r1 ? l0 + k : l0]).box;   // (four rows' loads together)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (l0 + k >= r1) continue;
            const sa_box& b = bx[k];
            const sa_geo cg = sa_box_geo(b);
            bool live = !sa_too_far(cg, lz_tg) && sa_compatible(cg, epoch, lz_tg, lz_te, p.max_idle, p.cons);
            if (live) {
              const float conf = b.confidence < p.min_confidence ? p.min_confidence : b.confidence;
              live = !sa_aa_quick_reject(cg, sa_box_ext(b.aspect, b.height, b.has_angle && b.angle != 0.0f), lz_tg, lz_tx, conf,
                                         p.positional_threshold);
            }
            if (live) {
              const uint32_t slot = atomicAdd(&s_ctr[5], 1u);
              if (slot < LZ_CAP) s_lsurv[slot] = ((l0 + k) << 16) | q;
            }
          }
        }
      };
      // the clip: groups of eight lanes, one surviving cell at a time; edges onto the row's HBM list
      auto clip = [&](uint32_t cnt) {
        const uint32_t grp = q / LZ_L, gl = q & (LZ_L - 1u), gshift = (q % WAVE) & (WAVE - LZ_L);
        double* const ws = s_lws + (grp < LZ_GROUPS ? grp : 0u) * LZ_WS;
        double* const subj = ws + 4 * SA_POLY_CAP;
        for (uint32_t sidx = grp < LZ_GROUPS ? grp : cnt; sidx < cnt; sidx += LZ_GROUPS) {
          const uint32_t c = s_lsurv[sidx];
          const uint32_t i = s_lrow[c >> 16], j = c & 0xffffu;
          const BoxRaw r = sa_ldg(S.c_raw + i);
          const double SA_G* tp = S.t_verts + (size_t)j * 8;
          double cv[8], tv[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) tv[k] = tp[k];
          const float t_hha = sa_ldg(S.t_geo + j).hha;
          sa_geo cg;
          prep_box_common(r, &cg, cv);
          if (gl == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) subj[k] = cv[k];
          }
          SA_WAVE_LDS_SYNC();
          const double inter = clip_area_lanes<(int)LZ_L>(subj, tv, ws, gl, gshift);
          float iou;
          if (gl == 0 && sa_iou_from_area(inter, cg.hha, t_hha, &iou)) {
            const float conf = r.box.confidence < p.min_confidence ? p.min_confidence : r.box.confidence;
            const float e = iou * conf;
            if (e >= p.positional_threshold) {
              const int64_t gain = sa_quantise(e) - p.threshold_q;
              if (gain > 0) sa_stg(S.e_edge + (size_t)atomicAdd(&s_lcnt[i], 1u) * N + i, SaEdge{gain, j, 0u});
            }
          }
        }
      };
      screen(0, nl);
      sa_lds_barrier();
      const uint32_t total = s_ctr[5];
      if (total <= LZ_CAP) clip(total);
      else {
        // more survivors than the list holds (frames with many leftover rows, which the host keeps eager unless told otherwise): again, in
        // batches of rows whose cells all fit
        const uint32_t rb = LZ_CAP / T;
        for (uint32_t r0 = 0; r0 < nl; r0 += rb) {
          sa_lds_barrier();   // (the last batch's list has been read)
          if (q == 0) s_ctr[5] = 0u;
          sa_lds_barrier();
          screen(r0, r0 + rb < nl ? r0 + rb : nl);
          sa_lds_barrier();
          clip(s_ctr[5]);
        }
      }
      // the appended edges are read below by other threads of the workgroup: every store acknowledged (a full barrier drains vmcnt)
      __syncthreads();
    }
    rawcnt = q < N ? s_lcnt[q] : 0u;
  }
  // Plain SORT (with a visual vote most rows arrive decided and their lists are never read): the first four edges of the row
  // are fetched before their count is known (what lies beyond the count is stale but
  // addressable), so that this round trip — the lists were written by other XCDs a moment ago, it goes to memory — overlaps the
  // count's.  What depends on them — the excluded-column flags and the track ids the results will need — is requested right after
  // the scan; the ids are not awaited before the results are written (sa_lds_barrier).  Tracking frames rarely have more than
  // four edges in a row.
  uint32_t sj[4];
  int64_t sg[4];
  {
    const SaEdge SA_G* row = S.e_edge + (q < N ? q : 0);  // slot-major: edge k of row q at [k * N + q]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = !VISUAL && q < N && (uint32_t)k < T;  // T == 0: the lists have no capacity at all
      const SaEdge ed = in ? sa_ldg(row + (size_t)k * N) : SaEdge{0, 0u, 0u};
      sj[k] = ed.col;
      sg[k] = ed.gain;
    }
  }
  if (!LAZY && q < N) S.e_cnt[q] = 0;  // left clean for the next frame's positional tiles (nothing below reads the global counter)
  if (S.tap_ecnt && q < N) S.tap_ecnt[q] = rawcnt;  // SA_FLAG_TAP: how many edge records the positional tiles appended to this row
  const uint32_t mycnt = (q < N && !has_verdict) ? rawcnt : 0u;
  s_rmatch[q] = -1;
  s_ecnt[q] = mycnt;
  s_head[q] = SA_NONE;
  s_next[q] = SA_NONE;
#pragma unroll
  for (int cc = 0; cc <= TC; ++cc) s_parent[q + (uint32_t)cc * SA_SMALL_N] = q + (uint32_t)cc * SA_SMALL_N;
#pragma unroll
  for (int cc = 0; cc < TC; ++cc) {
    const uint32_t j = q + (uint32_t)cc * SA_SMALL_N;
    s_v[j] = 0; s_cmatch[j] = -1; s_cstamp[j] = 0; s_cscan[j] = 0; s_cwin[j] = SA_NONE;
  }
  s_rcount[q] = 0; s_ccount[q] = 0; s_lab[q] = SA_NONE;
  if (q < 8) s_ctr[q] = 0;
  // leftover rows (no visual group) per wave: the scene's hint for the next frame's positional mode (out_stats[2], sa_lazy_positional)
  __shared__ uint32_t s_wleft[WORDS && TC == 1 ? SA_SMALL_N / WAVE : 1];
  if constexpr (WORDS && TC == 1) {
    const unsigned long long lm = __ballot(q < N && !has_verdict);
    if (q % WAVE == 0) s_wleft[q / WAVE] = (uint32_t)__popcll(lm);
  }
  // exclusive scan of mycnt over the 1024 threads: wave scan, then the 16 wave totals
  uint32_t incl = mycnt;
  {
    const uint32_t lane = q % WAVE;
    for (int o = 1; o < WAVE; o <<= 1) {
      uint32_t up = __shfl_up(incl, o);
      if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == WAVE - 1) s_wsum[q / WAVE] = incl;
  }
  sa_lds_barrier();
  if constexpr (WORDS) if (clsmode) {
    uint32_t mk = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < SA_SMALL_N / WAVE; ++w2) mk = s_wmk[w2] > mk ? s_wmk[w2] : mk;
    const double max_dist = mk ? (double)sa_key_f32(mk) : -1.0;
    auto best_of = [&](const unsigned long long* cls) -> uint32_t {
      double bw = 0.0;
      uint32_t bi = SA_NONE;
#pragma unroll
      for (uint32_t c = 0; c < SA_CLS_MAXK; ++c) {
        if (cls[c] == ~0ull) continue;
        const double w = (double)(c + 1u) * max_dist - (double)sa_key_f32((uint32_t)(cls[c] >> 32));
        const uint32_t i = (uint32_t)cls[c];
        if (bi == SA_NONE || w > bw || (w == bw && i < bi)) { bw = w; bi = i; }
      }
      return bi;
    };
    bt = best_of(rcls);
    s_bt[q] = bt;
#pragma unroll
    for (int cc = 0; cc < TC; ++cc) s_cq[q + (uint32_t)cc * SA_SMALL_N] = best_of(ccls[cc]);
    sa_lds_barrier();
  }
  if constexpr (WORDS) {
    if (has_verdict && s_cq[bt] == q) vw0 = (int32_t)bt;  // the candidate that is best in its own best column wins it
#pragma unroll
    for (int cc = 0; cc < TC; ++cc) { const uint32_t j = q + (uint32_t)cc * SA_SMALL_N; s_cexcl[j] = j < T && excluded(j); }
  }
  uint32_t woff = 0, total = 0;
  for (uint32_t w2 = 0; w2 < SA_SMALL_N / WAVE; ++w2) {
    const uint32_t v = s_wsum[w2];
    if (w2 < q / WAVE) woff += v;
    total += v;
  }
  if constexpr (WORDS && TC == 1) {
    if (q == 0) {
      uint32_t left = 0;
      for (uint32_t w2 = 0; w2 < SA_SMALL_N / WAVE; ++w2) left += s_wleft[w2];
      SA_OUT(S.out_stats + 2, left);
    }
  }
  if (total == 0) {  // nothing left for the positional vote (every row decided visually, or no edge at all)
    if (q < N) {
      uint64_t id = 0;
      uint8_t vt = SA_VOTE_NONE;
      const int32_t vw = vw0;
      if (vw >= 0) { id = S.t_ids[vw]; vt = SA_VOTE_VISUAL; }
      SA_OUT(S.out_track_id + q, id);
      SA_OUT(S.out_vote + q, vt);
      S.win_col[q] = vw >= 0 ? vw : -1;
      SA_OUT(S.out_win + q, vw >= 0 ? vw : -1);
    }
    sa_report_done(S, done_seq, &s_done);
    return;
  }
  TAIL_STAMP(1);
  if (VISUAL) {
    const SaEdge SA_G* row = S.e_edge + (q < N ? q : 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const SaEdge ed = (uint32_t)k < mycnt ? sa_ldg(row + (size_t)k * N) : SaEdge{0, 0u, 0u};
      sj[k] = ed.col;
      sg[k] = ed.gain;
    }
  }
  bool sx[4];
  uint64_t sid[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = (uint32_t)k < mycnt;
    sx[k] = VISUAL && in && excluded(sj[k]);
    sid[k] = in ? S.t_ids[sj[k]] : 0ull;
  }
  const bool pool = total <= POOL;
  const uint32_t myoff = woff + incl - mycnt;
  s_eoff[q] = myoff;
  int64_t maxg = 0;
  uint32_t bcol = SA_NONE;  // the column of the heaviest usable edge, lowest column on ties: this row's bid
  uint32_t usable = 0;
  if (mycnt) {
    const SaEdge SA_G* row = S.e_edge + q;
    // four edges per step: all their loads (and, with a visual vote, the dependent excluded-column flags) are in flight together
    for (uint32_t e0 = 0; e0 < mycnt; e0 += 4) {
      uint32_t jj[4];
      int64_t gg[4];
      bool skip[4];
      if (e0 == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { jj[k] = sj[k]; gg[k] = sg[k]; skip[k] = !((uint32_t)k < mycnt) || sx[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = e0 + k < mycnt;
          const SaEdge ed = in ? sa_ldg(row + (size_t)(e0 + k) * N) : SaEdge{0, 0u, 0u};
          jj[k] = ed.col;
          gg[k] = ed.gain;
          skip[k] = !in;
        }
        if (VISUAL) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (!skip[k]) skip[k] = excluded(jj[k]);  // excluded_tracks (visual_sort/voting.rs:62-71): dropped while packing
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (skip[k]) continue;
        const uint32_t j = jj[k];
        if (pool) { s_ecol[myoff + usable] = j; egain[myoff + usable] = gg[k]; }
        ++usable;
        if (gg[k] > maxg || (gg[k] == maxg && j < bcol)) { maxg = gg[k]; bcol = j; }
        sa_uf_union(s_parent, q, N + j);
      }
    }
    if (pool) s_ecnt[q] = usable;  // the packed list holds usable edges only (the HBM list keeps them all: the solver skips there)
  }
  s_u[q] = -maxg;
  if (usable) atomicMin(&s_cwin[bcol], q);  // the bid (bcol is set whenever a usable edge exists: gains are > 0)
  sa_lds_barrier();
  TAIL_STAMP(2);
  // component label = root of the union-find tree = the lowest vertex = the component's first row.  Columns count themselves
  // into their component (the room a search's list of labelled columns can need); rows learn whether their bid held.
  uint32_t lab = SA_NONE;
  if (usable) {
    lab = sa_uf_find(s_parent, q);
    s_lab[q] = lab;
    if (s_cwin[bcol] == q) { s_rmatch[q] = (int32_t)bcol; s_cmatch[bcol] = (int32_t)q; }
    else {
      s_next[q] = atomicExch(&s_head[lab], q);
      atomicAdd(&s_rcount[lab], 1u);
    }
  }
#pragma unroll
  for (int cc = 0; cc < TC; ++cc) {
    const uint32_t j = q + (uint32_t)cc * SA_SMALL_N;
    if (j < T) {
      const uint32_t r = sa_uf_find(s_parent, N + j);
      if (r < N) atomicAdd(&s_ccount[r], 1u);  // a column without usable edges is its own root (>= N)
    }
  }
  sa_lds_barrier();
  TAIL_STAMP(3);
  // A component with search roots goes onto one of two queues: the wavefronts' (bottom of s_queue) or — many roots on many columns,
  // or edge lists that did not fit the LDS pool: every relax step would walk HBM — the dense solver's (top of s_queue; the mark
  // in s_ccount tells its rows that their results come later).  sa_dense.h has the why.
  if (lab == q && s_head[q] != SA_NONE) {
    const bool dense = s_rcount[q] >= SA_DENSE_MIN_ROOTS && (s_ccount[q] >= SA_DENSE_MIN_COLS || !pool);
    if (dense) {
      s_queue[SA_SMALL_N - 1u - atomicAdd(&s_ctr[4], 1u)] = q;
      s_ccount[q] |= 0x80000000u;
    } else s_queue[atomicAdd(&s_ctr[0], 1u)] = q;
  }
  sa_lds_barrier();
  TAIL_STAMP(4);
  // groups of G lanes take components off the queue
  {
    const uint32_t lane = q % G;
    const uint32_t nq = s_ctr[0];
    sa_coop_ws w;
    w.e_cnt = s_ecnt;
    w.u = s_u; w.v = s_v; w.rmatch = s_rmatch; w.cmatch = s_cmatch; w.dist = s_dist; w.pred = s_pred; w.cstamp = s_cstamp; w.cscan = s_cscan;
    for (;;) {
      uint32_t take[1], seg[2];
      if (lane == 0) take[0] = atomicAdd(&s_ctr[1], 1u);
      const uint32_t k = sa_coop_bcast<G>(take);
      if (k >= nq) break;
      const uint32_t root = s_queue[k];
      const uint32_t R = s_rcount[root], C = s_ccount[root];
      if (lane == 0) { seg[0] = atomicAdd(&s_ctr[2], C); seg[1] = atomicAdd(&s_ctr[3], R); }
      const uint32_t cbase = sa_coop_bcast<G>(seg), rbase = sa_coop_bcast<G>(seg + 1);
      uint32_t* roots = s_rlist + rbase;
      if (R <= (uint32_t)G) {
        // a short list: every lane walks it, lane l keeps element l, ranks by comparison, one store each
        uint32_t cur = s_head[root], mine = SA_NONE;
        for (uint32_t st = 0; st < R; ++st) {
          if (st == lane) mine = cur;
          cur = s_next[cur];
        }
        uint32_t rank = 0;
        for (uint32_t st = 0; st < R; ++st) {
          const uint32_t other = __shfl(mine, st, G);
          rank += other < mine ? 1u : 0u;
        }
        if (lane < R) roots[rank] = mine;
      } else {
        // a long list: compact the scene's rows (lab == root, bid lost) in row order, G rows per step
        uint32_t cnt = 0;
        for (uint32_t r0 = 0; r0 < N; r0 += G) {
          const uint32_t row = r0 + lane;
          bool f[1];
          f[0] = row < N && s_lab[row] == root && s_rmatch[row] < 0;
          uint32_t tot;
          const uint32_t rk = sa_coop_rank<G>(f, lane, &tot);
          if (f[0]) roots[cnt + rk] = row;
          cnt += tot;
        }
      }
      sa_coop_sync<G>();
      w.clist = s_clist + cbase;
      // one call site per address space of the edge storage (LDS pool or the HBM lists), so that every pointer of the work set has
      // ONE known address space after inlining — "LDS or global, decided at run time" compiles to flat_* accesses
      if (pool) {
        w.e_col = s_ecol; w.e_gain = egain; w.ecs = 1; w.egs = 1; w.rcs = 1; w.rgs = 1; w.estride = 0; w.e_off = s_eoff; w.excluded = nullptr;
        sa_assign_component_coop<G>(w, roots, R);
      } else {
        // slot-major lists: row r starts at record r, consecutive edges are N records apart
        w.e_col = (const uint32_t*)S.e_edge + 2; w.e_gain = (const int64_t*)S.e_edge; w.ecs = 4 * N; w.egs = 2 * N; w.rcs = 4; w.rgs = 2; w.e_off = nullptr; w.estride = 1;
        if constexpr (WORDS) w.excluded = s_cexcl;
        else w.excluded = VISUAL ? (const uint8_t*)S.col_excluded : nullptr;
        sa_assign_component_coop<G>(w, roots, R);
      }
    }
  }
  TAIL_STAMP(5);
  sa_lds_barrier();  // rmatch is in LDS
  TAIL_STAMP(6);
  const uint32_t nd = s_ctr[4];  // components waiting for the dense solver (tracking frames: none)
  const bool mine_later = nd && usable && (s_ccount[lab] & 0x80000000u);
  if (q < N && !mine_later) {
    uint64_t id = 0;
    uint8_t vt = SA_VOTE_NONE;
    int32_t win = -1;
    const int32_t vw = vw0;
    if (vw >= 0) { id = S.t_ids[vw]; vt = SA_VOTE_VISUAL; win = vw; }
    else if (!has_verdict) {
      int32_t c = s_rmatch[q];
      if (c >= 0) {
        bool found = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((uint32_t)k < mycnt && sj[k] == (uint32_t)c) { id = sid[k]; found = true; }
        if (!found) id = S.t_ids[c];
        vt = SA_VOTE_POSITIONAL;
        win = c;
      }
    }
    SA_OUT(S.out_track_id + q, id);
    SA_OUT(S.out_vote + q, vt);
    S.win_col[q] = win;
    SA_OUT(S.out_win + q, win);
  }
  if (nd) {
    // The dense solver runs on SA_DENSE_NT threads (one wave per SIMD: a search step is a chain of dependent instructions, more
    // waves per SIMD only stretch it): the other waves are done — a barrier waits for the surviving waves only.
    if (q >= (uint32_t)DNT) { sa_report_done(S, done_seq, &s_done); return; }
    uint32_t rtop = s_ctr[3];
    for (uint32_t k = 0; k < nd; ++k) {
      const uint32_t root = s_queue[SA_SMALL_N - 1u - k];
      const uint32_t R = s_rcount[root];
      uint32_t* roots = s_rlist + rtop;
      rtop += R;
      // the search roots, ascending (wave 0: ballot compaction of the scene's rows), and the component's gains into the dense matrix
      if (q < WAVE) {
        uint32_t cnt = 0;
        for (uint32_t r0 = 0; r0 < N; r0 += WAVE) {
          const uint32_t row = r0 + q;
          const bool f = row < N && s_lab[row] == root && s_rmatch[row] < 0;
          const unsigned long long m = __ballot(f);
          if (f) roots[cnt + (uint32_t)__popcll(m & ((1ull << q) - 1ull))] = row;
          cnt += (uint32_t)__popcll(m);
        }
      }
      if (q == 0) s_ctr[5] = 0;  // the component's heaviest gain (32-bit variant of the solver when it is small enough)
      sa_lds_barrier();
      uint32_t mg = 0;
      for (uint32_t row = q; row < N; row += (uint32_t)DNT) {
        if (s_lab[row] != root) continue;
        const int64_t heaviest = -s_u[row];
        const uint32_t h32 = heaviest > 0x7fffffffll ? 0x7fffffffu : (uint32_t)heaviest;
        mg = h32 > mg ? h32 : mg;
        int64_t SA_G* drow = S.dense + (size_t)row * T;
        const uint32_t cnt = s_ecnt[row];
        if (pool) {
          const uint32_t off = s_eoff[row];
          for (uint32_t e = 0; e < cnt; ++e) drow[s_ecol[off + e]] = egain[off + e];
        } else {
          const SaEdge SA_G* ep = S.e_edge + row;  // slot-major lists, excluded columns still inside; four records per round trip
          for (uint32_t e0 = 0; e0 < cnt; e0 += 4) {
            SaEdge ed[4];
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) ed[k2] = e0 + k2 < cnt ? sa_ldg(ep + (size_t)(e0 + k2) * N) : SaEdge{0, 0u, 0u};
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
              if (e0 + k2 < cnt && !(VISUAL && excluded(ed[k2].col))) drow[ed[k2].col] = ed[k2].gain;
          }
        }
      }
      if (mg) atomicMax(&s_ctr[5], mg);
      __syncthreads();
      {
        sa_dense_ws w;
        w.gain = (const int64_t*)S.dense; w.ld = T; w.T = T;
        w.u = s_u; w.rmatch = s_rmatch; w.cmatch = s_cmatch; w.pred = s_pred; w.part = s_part;
        if (s_ctr[5] <= (uint32_t)SA_DENSE_K32_MAXGAIN) sa_assign_component_dense<DNT, TCAP / DNT, true>(w, roots, R);
        else sa_assign_component_dense<DNT, TCAP / DNT, false>(w, roots, R);
      }
      // results of the component's rows (none of them holds a visual verdict), and the matrix left clean for the next frame
      for (uint32_t row = q; row < N; row += (uint32_t)DNT) {
        if (s_lab[row] != root) continue;
        const int32_t c = s_rmatch[row];
        SA_OUT(S.out_track_id + row, c >= 0 ? S.t_ids[c] : 0ull);
        SA_OUT(S.out_vote + row, c >= 0 ? SA_VOTE_POSITIONAL : SA_VOTE_NONE);
        S.win_col[row] = c;
        SA_OUT(S.out_win + row, c);
        int64_t SA_G* drow = S.dense + (size_t)row * T;
        const uint32_t cnt = s_ecnt[row];
        if (pool) {
          const uint32_t off = s_eoff[row];
          for (uint32_t e = 0; e < cnt; ++e) drow[s_ecol[off + e]] = 0;
        } else {
          const SaEdge SA_G* ep = S.e_edge + row;
          for (uint32_t e0 = 0; e0 < cnt; e0 += 4) {
            uint32_t cj[4];
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) cj[k2] = e0 + k2 < cnt ? sa_ldg(ep + (size_t)(e0 + k2) * N).col : 0u;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
              if (e0 + k2 < cnt) drow[cj[k2]] = 0;
          }
        }
      }
      __syncthreads();
    }
  }
  sa_report_done(S, done_seq, &s_done);
  TAIL_STAMP(7);
