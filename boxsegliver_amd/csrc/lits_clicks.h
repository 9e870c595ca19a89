// What the two click simulators share (lits_inter.hip: one slice per sample; lits3d_clicks.hip: a [D, ch, cw]
// patch per sample): the class bits of a candidate field, the draws of a click_tab row and the column
// sweeps of the distance transform.  One copy, so the 2-D and the 3-D simulator cannot drift.
#pragma once
#include "common.h"

namespace {

constexpr int MAXK = UNETK_LITS_MAX_CLICKS;
constexpr int CTW = UNETK_LITS_CLICK_TAB_COLS;
constexpr int CLK_MAX_EXTENT = 1024;     // rows / columns of a slice the simulators take (their row buffers live in LDS)
enum { CLS_FG = 1, CLS_BG = 2, CLS_OBJ = 4, CLS_NEG = 8 };   // CLS_NEG: lits3d_clicks.hip with a `neg` plane only
constexpr int CLK_U = 8;                  // pixels a thread loads before it works on them (column sweeps, selection)

// ------------------------------------------------------------------------------------------------ the draws of one kind
// click_tab row -> how many clicks the kind asks for and by which strategy, clamped into their ranges; `bad` says that
// the row was out of range (status bit 2).  The foreground always picks by rank (strategy 1).
struct ClkDraws {
  int want, strategy;
  bool bad;
};
__device__ __forceinline__ ClkDraws clk_draws(const uint32_t* __restrict__ ct, int kind, int max_clicks) {
  ClkDraws r;
  const int n_min = kind == 0 ? 1 : 0;
  const uint32_t want_raw = ct[kind];
  r.want = (int)min(max(want_raw, (uint32_t)n_min), (uint32_t)(max_clicks - 1));
  const uint32_t strat_raw = kind == 0 ? 1u : ct[2];
  r.strategy = strat_raw == 3u ? 3 : 1;
  r.bad = (uint32_t)r.want != want_raw || (strat_raw != 1u && strat_raw != 3u);
  return r;
}

// ------------------------------------------------------------------------------------------------ column distances
// One thread, one column of `rows` pixels: gf = distance along the column to the nearest non-object pixel, the column's
// two ends counting as one (0 on non-object pixels); gb = distance along the column to the nearest object pixel; both
// capped at `cap` <= 255.  p = the column's first label (stride src_w), read only where `valid`; a column that is not
// valid holds no object.  gf / gb = the column's first byte, stride cw.
// CLK_U rows per step, their loads issued together: the sweeps are chains of dependent adds, not of dependent loads.
__device__ __forceinline__ void clk_col_sweeps(const uint8_t* __restrict__ p, bool valid, int src_w, int rows, int cw, int thr,
                                               int cap, uint8_t* __restrict__ gf, uint8_t* __restrict__ gb) {
  int df = 0, db = cap;
  for (int y0 = 0; y0 < rows; y0 += CLK_U) {
    int s[CLK_U];
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) s[u] = (valid && y0 + u < rows) ? (int)p[(int64_t)(y0 + u) * src_w] : 0;
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) {
      const int y = y0 + u;
      if (y < rows) {
        const bool o = s[u] >= thr;
        df = o ? min(df + 1, cap) : 0;
        db = o ? 0 : min(db + 1, cap);
        gf[y * cw] = (uint8_t)df;
        gb[y * cw] = (uint8_t)db;
      }
    }
  }
  df = 0;
  db = cap;
  for (int y0 = rows - 1; y0 >= 0; y0 -= CLK_U) {
    int f[CLK_U], g[CLK_U];
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) {
      const int y = max(y0 - u, 0);
      f[u] = gf[y * cw];
      g[u] = gb[y * cw];
    }
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) {
      const int y = y0 - u;
      if (y >= 0) {
        const bool o = f[u] > 0;                              // the downward distance is positive exactly on object pixels
        df = o ? min(df + 1, cap) : 0;
        db = o ? 0 : min(db + 1, cap);
        gf[y * cw] = (uint8_t)min(f[u], df);
        gb[y * cw] = (uint8_t)min(g[u], db);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ row pass
// One block, one row of cw pixels in LDS, NF fields side by side: d(x) = min_x' g(x') + |x - x'|, capped at `cap`, by
// min-plus doubling (offsets 1, 2, 4, ... compose every |x - x'| below the cap exactly).  The caller has filled buf[0] and
// synchronised; returns the half of buf that holds the result, synchronised.
template <int NF>
__device__ __forceinline__ int clk_row_minplus(int16_t (&buf)[2][NF][CLK_MAX_EXTENT], int cw, int cap) {
  int cur = 0;
  for (int o = 1; o < cap; o <<= 1) {
    for (int x = threadIdx.x; x < cw; x += blockDim.x) {
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        int v = buf[cur][k][x];
        if (x >= o) v = min(v, buf[cur][k][x - o] + o);
        if (x + o < cw) v = min(v, buf[cur][k][x + o] + o);
        buf[cur ^ 1][k][x] = (int16_t)min(v, cap);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  return cur;
}

}  // namespace
