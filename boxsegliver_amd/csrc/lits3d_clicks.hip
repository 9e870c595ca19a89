// Click guides for UNet3D from the resident LiTS slice store: the clicks of the reference's 3-D pipeline
// simulated on the label patch that unetk_lits_patch3d cuts, and rendered into sp_guide.
//
// The semantics are those of DataLoader/NF/input_pipeline_3d.py (:258-324 inter_simulation as :474-504 gen_kernel calls it,
// :364-398 data_processing) and utils/image_ops.py:437-472 create_spatial_guide_3d.  The 2-D simulator is lits_inter.hip; what
// differs here (include/unetk.h has the full statement):
//   * the erosion's element is the 3 x 3 square of one slice, so the candidate sets are thresholds of the CHESSBOARD
//     distance inside each slice.  That distance is separable: dinf(p, zeros) > t  <=>  the (2t + 1)-square around p holds
//     no zero  <=>  every column x' with |x' - x| <= t has its nearest zero farther than t from row y.  So
//       clk3_cols_kernel  thread per (slice, crop column): the column sweeps of the 2-D simulator (clk_col_sweeps)
//       clk3_rows_kernel  block per (slice, crop row), the row in LDS: the column distances are thresholded (> margin for
//                         both kinds, > margin + band for the outer edge of the background band), and the distance
//                         along the row to the nearest pixel that fails the threshold comes from the same min-plus
//                         doubling as in 2-D -> one class byte per voxel, and per row a record of 8 ints (candidates of
//                         both kinds, object pixels, sum of their x, first and last x of a background candidate)
//   * candidates are ranked over the whole patch in (z, y, x) order, but a click removes candidates from its own slice
//     only.  clk3_select_kernel (block per (sample, kind)) therefore keeps ONE count per slice in LDS, filled from the row
//     records: a rank pick finds its slice in that table and walks that slice alone, and after a click only that slice is
//     counted again.  Only the arg-max of strategy 3 reads the whole patch, 16 class bytes per load, skipping runs
//     without a candidate and runs whose farthest voxel cannot beat a distance that a live candidate is known to have
//     (the ends of the rows, from the row records) or the thread's best so far.
//   * the "small" click is the mask's mean rounded half to even, from the row records' integer sums.
// Everything is integer arithmetic: counts, sums and the arg-max key (distance, then the first in (z, y, x) order) do not
// depend on the order in which they are reduced, so two calls give identical bits.
#include "common.h"
#include "lits_clicks.h"
#include "lits_geom.h"
#include "lits_patch.h"      // TW, Box3, p3d_box, p3d_slice

namespace {

constexpr int CLK3_MAX_D = 256;           // slices of a patch: the per-slice counts live in LDS
constexpr int CLK3_REC = 8;               // int32 per row record: foreground candidates, background candidates, object pixels,
                                          // sum of the object pixels' x, first and last x of a background candidate, 0, 0

// bytes of one of the three byte fields of a sample: D slices of the store's extent, rounded up so that every field starts
// on a 16-byte boundary (clk3_select_kernel's arg-max reads 16 bytes at a time)
__host__ __device__ __forceinline__ int64_t clk3_field(const unetk_lits3d_clicks_desc& d) {
  return ((int64_t)d.D * d.src_h * d.src_w + 15) / 16 * 16;
}

// ------------------------------------------------------------------------------------------------ column distances
// Indexed (z * ch + y) * cw + x inside a field.  A slice beyond the case holds no object.
__global__ __launch_bounds__(64) void clk3_cols_kernel(unetk_lits3d_clicks_desc d, const uint8_t* __restrict__ segs,
                                                       const int32_t* __restrict__ tab, uint8_t* __restrict__ ws) {
  const int n = blockIdx.z, z = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  const Box3 b = p3d_box(tab + (int64_t)n * TW, d);
  if (x >= b.cw) return;
  const int64_t plane = (int64_t)d.src_h * d.src_w, field = clk3_field(d);
  const int64_t sl = p3d_slice(b, z, d);
  const int cap = d.margin + d.band + 1, thr = d.obj_label * d.lab_scale;
  uint8_t* gf = ws + (int64_t)n * 3 * field + (int64_t)z * b.ch * b.cw + x;
  const uint8_t* p = segs + (sl < 0 ? 0 : sl) * plane + (int64_t)b.y1 * d.src_w + b.x1 + x;
  clk_col_sweeps(p, sl >= 0, d.src_w, b.ch, b.cw, thr, cap, gf, gf + field);
}

// ------------------------------------------------------------------------------------------------ row pass, classes
// NEG (unetk_lits3d_clicks_neg): the row of the `neg` plane under the crop adds the class bit CLS_NEG and the
// row record's slot 6, the row's false-positive voxels; everything else is the plain kernel's.
template <bool NEG>
__global__ __launch_bounds__(256) void clk3_rows_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                        const uint8_t* __restrict__ negs, uint8_t* __restrict__ ws,
                                                        int32_t* __restrict__ rowrec) {
  __shared__ int16_t buf[2][3][CLK_MAX_EXTENT];
  __shared__ int red[4][7];
  const int n = blockIdx.z, z = blockIdx.y, y = blockIdx.x;
  const Box3 b = p3d_box(tab + (int64_t)n * TW, d);
  if (y >= b.ch) return;                                     // block-uniform
  const int64_t field = clk3_field(d);
  const int cap = d.margin + d.band + 1, cw = b.cw, outer = d.margin + d.band;
  const uint8_t* gf = ws + (int64_t)n * 3 * field + ((int64_t)z * b.ch + y) * cw;
  const uint8_t* gb = gf + field;
  uint8_t* cls = ws + (int64_t)n * 3 * field + 2 * field + ((int64_t)z * b.ch + y) * cw;
  // 0 where the column distance fails the threshold, else the distance to the crop's left / right border (foreground:
  // border_value = 0) or the cap (background: border_value = 1)
  for (int x = threadIdx.x; x < cw; x += 256) {
    const int f = gf[x], g = gb[x];
    buf[0][0][x] = (int16_t)(f > d.margin ? min(min(x + 1, cw - x), cap) : 0);
    buf[0][1][x] = (int16_t)(g > d.margin ? cap : 0);
    buf[0][2][x] = (int16_t)(g > outer ? cap : 0);
  }
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < cap; o <<= 1) {
    for (int x = threadIdx.x; x < cw; x += 256) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        int v = buf[cur][k][x];
        if (x >= o) v = min(v, buf[cur][k][x - o] + o);
        if (x + o < cw) v = min(v, buf[cur][k][x + o] + o);
        buf[cur ^ 1][k][x] = (int16_t)min(v, cap);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  int nf = 0, nb = 0, no = 0, so = 0, bfirst = cw, blast = -1, nn = 0;
  const int64_t nsl = NEG ? p3d_slice(b, z, d) : -1;         // a slice beyond the case holds no false positive
  const uint8_t* ng = NEG && nsl >= 0 ? negs + (nsl * d.src_h + b.y1 + y) * (int64_t)d.src_w + b.x1 : nullptr;
  for (int x = threadIdx.x; x < cw; x += 256) {
    const bool fg = buf[cur][0][x] > d.margin;
    const bool bg = buf[cur][1][x] > d.margin && !(buf[cur][2][x] > outer);
    const bool ob = gf[x] > 0;
    const bool ng1 = NEG && ng != nullptr && (int)ng[x] >= d.lab_scale;      // the plane's encoding: label 1
    cls[x] = (uint8_t)((fg ? CLS_FG : 0) | (bg ? CLS_BG : 0) | (ob ? CLS_OBJ : 0) | (ng1 ? CLS_NEG : 0));
    nn += ng1;
    nf += fg;
    nb += bg;
    no += ob;
    so += ob ? x : 0;
    bfirst = bg ? min(bfirst, x) : bfirst;
    blast = bg ? max(blast, x) : blast;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nf += __shfl_xor(nf, o);
    nb += __shfl_xor(nb, o);
    no += __shfl_xor(no, o);
    so += __shfl_xor(so, o);
    bfirst = min(bfirst, __shfl_xor(bfirst, o));
    blast = max(blast, __shfl_xor(blast, o));
    if (NEG) nn += __shfl_xor(nn, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][6] = nn;
    red[wave][0] = nf;
    red[wave][1] = nb;
    red[wave][2] = no;
    red[wave][3] = so;
    red[wave][4] = bfirst;
    red[wave][5] = blast;
  }
  __syncthreads();
  int32_t* rec = rowrec + (((int64_t)n * d.D + z) * d.src_h + y) * CLK3_REC;
  const int t = threadIdx.x;
  if (t < 4) rec[t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
  if (t == 4) rec[4] = min(min(red[0][4], red[1][4]), min(red[2][4], red[3][4]));
  if (t == 5) rec[5] = max(max(red[0][5], red[1][5]), max(red[2][5], red[3][5]));
  if (t == 6) rec[6] = NEG ? red[0][6] + red[1][6] + red[2][6] + red[3][6] : 0;
  if (t == 7) rec[7] = 0;
}

// ------------------------------------------------------------------------------------------------ selection
struct Clicks3 {
  int n, z[MAXK], y[MAXK], x[MAXK];
};
// a candidate of slice z is alive while it lies farther than `step`, in the plane, from every click so far ON ITS SLICE
// (inter_simulation :313-320: "Only operate on single slice")
__device__ __forceinline__ bool clk3_alive(int cls, int bit, int z, int y, int x, const Clicks3& c, int step2) {
  bool a = (cls & bit) != 0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {                           // unrolled: the clicks stay in registers
    const int dy = y - c.y[k], dx = x - c.x[k];
    a = a && (k >= c.n || c.z[k] != z || dy * dy + dx * dx > step2);
  }
  return a;
}
// the wave's share [lo, hi) of slice z: how many of its candidates are alive (wave-uniform)
__device__ __forceinline__ int clk3_count(const uint8_t* __restrict__ s, int lo, int hi, int lane, int cw, float rcw, int bit,
                                          int z, const Clicks3& c, int step2) {
  int a = 0;
  for (int i0 = lo; i0 < hi; i0 += 64 * CLK_U) {            // wave-uniform trip count: the ballots see whole waves
    int v[CLK_U];
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)s[i0 + u * 64 + lane] : 0;
#pragma unroll
    for (int u = 0; u < CLK_U; ++u) {
      const int i = i0 + u * 64 + lane, y = unetk_fdiv(i, cw, rcw);
      a += __popcll(__ballot(clk3_alive(v[u], bit, z, y, i - y * cw, c, step2)));
    }
  }
  return a;
}
// An upper bound of min_k d2(voxel, click k) over the voxels (z, y, xa .. xb) of one row: min_k of the distance of the
// segment's farther end (max over the voxels of a minimum <= minimum of the maxima).
__device__ __forceinline__ unsigned int clk3_far_bound(int z, int y, int xa, int xb, const Clicks3& c) {
  unsigned int ub = 0xffffffffu;
#pragma unroll
  for (int m = 0; m < MAXK; ++m) {
    const int dz = z - c.z[m], dy = y - c.y[m], da = xa - c.x[m], db = xb - c.x[m];
    ub = m < c.n ? min(ub, (unsigned int)(dz * dz + dy * dy + max(da * da, db * db))) : ub;
  }
  return ub;
}

// NEG: a background kind whose crop holds false-positive voxels (row records' slot 6) runs the reference's strategy 4: the
// candidates are the CLS_NEG voxels, every click is a rank pick, there is no "small" click; any other row runs as without NEG.
template <bool NEG>
__global__ __launch_bounds__(1024) void clk3_select_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                           const uint32_t* __restrict__ click_tab,
                                                           const uint8_t* __restrict__ ws, const int32_t* __restrict__ rowrec,
                                                           int32_t* __restrict__ pts, int32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ status) {
  __shared__ int sband[CLK3_MAX_D];                          // candidates alive per slice
  __shared__ int sneg[NEG ? CLK3_MAX_D : 1];                 // NEG: ... of the false positives
  __shared__ unsigned long long red[16][4];
  __shared__ unsigned long long wbest[16];
  __shared__ int wcnt[16];
  __shared__ unsigned int wfloor[16];
  __shared__ int pick[3];
  const int kind = blockIdx.x, n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Box3 b = p3d_box(tab + (int64_t)n * TW, d);
  const int64_t field = clk3_field(d);
  const uint8_t* cls = ws + (int64_t)n * 3 * field + 2 * field;
  const int32_t* rec = rowrec + (int64_t)n * d.D * d.src_h * CLK3_REC;
  const int D = d.D, ch = b.ch, cw = b.cw, area = b.ch * b.cw;
  const int total = D * area;                                // < 2^31: checked by the entry point
  const int chunk = ((area + 15) / 16 + 63) / 64 * 64;       // pixels of a wave in one slice: a multiple of 64, row-major across waves
  const int lo = min(wave * chunk, area), hi = min(lo + chunk, area);
  int bit = kind == 0 ? CLS_FG : CLS_BG;
  const int step2 = d.step * d.step;
  const float rcw = 1.f / (float)cw;                         // i / cw through unetk_fdiv: i < 2^20 + 512
  const uint32_t* ct = click_tab + (int64_t)n * CTW;
  const ClkDraws dr = clk_draws(ct, kind, d.max_clicks);
  const int want = dr.want;
  int strategy = dr.strategy;
  if (threadIdx.x == 0 && dr.bad) atomicOr(status, 4);

  // pass 0, from the row records: candidates per slice; the mask's voxel count and coordinate sums.  Wave w takes the
  // slices w, w + 16, ...
  unsigned long long nmask = 0, sz = 0, sy = 0, sx = 0;
  for (int z = wave; z < D; z += 16) {
    int cand = 0, cneg = 0;
    for (int y = lane; y < ch; y += 64) {
      const int4 r = *reinterpret_cast<const int4*>(rec + ((int64_t)z * d.src_h + y) * CLK3_REC);
      cand += kind == 0 ? r.x : r.y;
      if (NEG) cneg += rec[((int64_t)z * d.src_h + y) * CLK3_REC + 6];
      const unsigned long long m = (unsigned long long)(kind == 0 ? r.z : cw - r.z);
      nmask += m;
      sz += m * (unsigned long long)z;
      sy += m * (unsigned long long)y;
      sx += (unsigned long long)(kind == 0 ? r.w : cw * (cw - 1) / 2 - r.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cand += __shfl_xor(cand, o);
      if (NEG) cneg += __shfl_xor(cneg, o);
    }
    if (lane == 0) {
      sband[z] = cand;
      if (NEG) sneg[z] = cneg;
    }
  }
  nmask = wave_sum(nmask);
  sz = wave_sum(sz);
  sy = wave_sum(sy);
  sx = wave_sum(sx);
  if (lane == 0) {
    red[wave][0] = nmask;
    red[wave][1] = sz;
    red[wave][2] = sy;
    red[wave][3] = sx;
  }
  __syncthreads();
  nmask = sz = sy = sx = 0;
  for (int w = 0; w < 16; ++w) {
    nmask += red[w][0];
    sz += red[w][1];
    sy += red[w][2];
    sx += red[w][3];
  }
  bool useneg = false;                                       // block-uniform
  if (NEG && kind == 1) {
    int t = 0;
    for (int z = 0; z < D; ++z) t += sneg[z];
    useneg = t > 0;
  }
  int* scnt = useneg ? sneg : sband;
  if (useneg) {
    bit = CLS_NEG;
    strategy = 1;
  }
  int alive = 0;
  for (int z = 0; z < D; ++z) alive += scnt[z];

  Clicks3 c;
  c.n = 0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) c.z[k] = c.y[k] = c.x[k] = 0;
  if ((nmask == 0 && !useneg) || want == 0) {
    // no voxel to click on (deviation: the reference fails on an all-object patch), or no click drawn
  } else if (alive == 0) {                                   // "small": one click at the mask's mean, rounded half to even
    c.z[0] = unetk_round_div_even(sz, nmask);
    c.y[0] = unetk_round_div_even(sy, nmask);
    c.x[0] = unetk_round_div_even(sx, nmask);
    c.n = 1;
  } else {
    int zl = -1;                                             // the slice whose per-wave counts wcnt holds (the last click's)
    for (int k = 0; k < want; ++k) {
      if (k > 0) {                                           // what the last click leaves on its slice; the others keep their counts
        __syncthreads();                                     // wcnt, scnt, pick and wbest are read above / below
        const int a = clk3_count(cls + (int64_t)zl * area, lo, hi, lane, cw, rcw, bit, zl, c, step2);
        if (lane == 0) wcnt[wave] = a;
        __syncthreads();
        int s = 0;
        for (int w = 0; w < 16; ++w) s += wcnt[w];
        __syncthreads();                                     // every thread has read scnt (alive, the walk below)
        if (threadIdx.x == 0) scnt[zl] = s;
        __syncthreads();
        alive = 0;
        for (int z = 0; z < D; ++z) alive += scnt[z];
        if (alive == 0) break;                               // block-uniform
      }
      if (k == 0 || strategy == 1) {
        // rank i = (r * count) >> 32 in (z, y, x) order: the slice from the per-slice counts, then inside that slice the
        // wave that holds it walks its pixels ballot by ballot
        int rank = (int)(((unsigned long long)ct[4 + 4 * kind + k] * (unsigned long long)alive) >> 32);
        int z0 = 0;
        for (; z0 < D - 1 && rank >= scnt[z0]; ++z0) rank -= scnt[z0];     // rank < alive = sum of scnt
        if (z0 != zl) {                                      // block-uniform
          __syncthreads();
          const int a = clk3_count(cls + (int64_t)z0 * area, lo, hi, lane, cw, rcw, bit, z0, c, step2);
          if (lane == 0) wcnt[wave] = a;
          __syncthreads();
        }
        int w0 = 0;
        for (; w0 < 15 && rank >= wcnt[w0]; ++w0) rank -= wcnt[w0];        // rank < scnt[z0] = sum of wcnt
        if (wave == w0) {
          const uint8_t* s = cls + (int64_t)z0 * area;
          bool found = false;                                // wave-uniform
          for (int i0 = lo; i0 < hi && !found; i0 += 64 * CLK_U) {
            int v[CLK_U];
#pragma unroll
            for (int u = 0; u < CLK_U; ++u) v[u] = i0 + u * 64 + lane < hi ? (int)s[i0 + u * 64 + lane] : 0;
#pragma unroll
            for (int u = 0; u < CLK_U; ++u) {
              if (found) continue;
              const int i = i0 + u * 64 + lane, y = unetk_fdiv(i, cw, rcw), x = i - y * cw;
              const bool a = clk3_alive(v[u], bit, z0, y, x, c, step2);
              const unsigned long long m = __ballot(a);
              const int here = __popcll(m);
              if (rank < here) {
                if (a && __popcll(m & ((1ull << lane) - 1ull)) == rank) {
                  pick[0] = z0;
                  pick[1] = y;
                  pick[2] = x;
                }
                found = true;
              } else {
                rank -= here;
              }
            }
          }
        }
      } else {
        // strategy 3: the candidate farthest (3-D) from the clicks so far, the first in (z, y, x) order on ties
        // (np.argmax).  16 class bytes per load; the key orders by distance, then by the smaller flat index.  A run of 16
        // voxels is looked at voxel by voxel only if it could still win: its bound (clk3_far_bound over the one or two row
        // segments it covers) is at least the distance of the thread's best so far.  Equal bounds are not skipped, so ties
        // are still seen; what is skipped is strictly smaller than a key that exists -- the result is the exact arg-max.
        // First a distance that some live candidate certainly has: the first and the last background candidate of every
        // row (row records) on the slices without a click, where nothing is suppressed.  Farthest points tend to sit at
        // the ends of rows, so this floor is close to the maximum and most runs fall below it.
        unsigned int floor2 = 0;
        if (kind == 1) {
          const float rch = 1.f / (float)ch;
          for (int row = threadIdx.x; row < D * ch; row += 1024) {                  // D * ch <= 2^18
            const int z = unetk_fdiv(row, ch, rch), y = row - z * ch;
            const int32_t* rr = rec + ((int64_t)z * d.src_h + y) * CLK3_REC;
            bool clear = rr[1] > 0;
#pragma unroll
            for (int m = 0; m < MAXK; ++m) clear = clear && (m >= c.n || c.z[m] != z);
            if (clear) floor2 = max(floor2, max(clk3_far_bound(z, y, rr[4], rr[4], c), clk3_far_bound(z, y, rr[5], rr[5], c)));
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) floor2 = max(floor2, (unsigned int)__shfl_xor((int)floor2, o));
          if (lane == 0) wfloor[wave] = floor2;
          __syncthreads();
          for (int w = 0; w < 16; ++w) floor2 = max(floor2, wfloor[w]);
        }
        unsigned long long best = 0;
        const int nvec = (total + 15) >> 4;
        const uint32_t bits = (uint32_t)bit * 0x01010101u;
        const float rarea = 1.f / (float)area;
        for (int v = threadIdx.x; v < nvec; v += 1024) {
          const uint4 q = *reinterpret_cast<const uint4*>(cls + (int64_t)v * 16);
          if (((q.x | q.y | q.z | q.w) & bits) == 0) continue;
          const uint32_t w[4] = {q.x, q.y, q.z, q.w};
          int i = v * 16;
          // i / area for i < 2^31 and a quotient <= 256: the float estimate is within 1, one correction
          int z = (int)((float)i * rarea);
          int r = i - z * area;
          if (r < 0) {
            --z;
            r += area;
          } else if (r >= area) {
            ++z;
            r -= area;
          }
          int y = unetk_fdiv(r, cw, rcw), x = r - y * cw;
          const unsigned int bound = max(floor2, (unsigned int)(best >> 32));
          if (cw >= 16 && bound != 0) {                      // cw >= 16: the run covers at most two rows
            unsigned int ub = clk3_far_bound(z, y, x, min(x + 15, cw - 1), c);
            if (x + 15 >= cw) {
              const bool last = y + 1 == ch;
              ub = max(ub, clk3_far_bound(last ? z + 1 : z, last ? 0 : y + 1, 0, x + 15 - cw, c));
            }
            if (ub < bound) continue;
          }
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int byte = (int)((w[j >> 2] >> ((j & 3) * 8)) & 0xffu);
            if (i < total && clk3_alive(byte, bit, z, y, x, c, step2)) {   // bytes past the patch are not candidates
              unsigned int d2 = 0xffffffffu;
#pragma unroll
              for (int m = 0; m < MAXK; ++m) {
                const int dz = z - c.z[m], dy = y - c.y[m], dx = x - c.x[m];
                d2 = m < c.n ? min(d2, (unsigned int)(dz * dz + dy * dy + dx * dx)) : d2;
              }
              const unsigned long long key = unetk_first_key(d2, (unsigned int)i);
              best = key > best ? key : best;
            }
            ++i;
            if (++x == cw) {
              x = 0;
              if (++y == ch) {
                y = 0;
                ++z;
              }
            }
          }
        }
        best = wave_max(best);
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
          for (int w = 0; w < 16; ++w) best = wbest[w] > best ? wbest[w] : best;
          const int i = unetk_key_index(best);
          const int z = i / area, r = i - z * area;
          pick[0] = z;
          pick[1] = r / cw;
          pick[2] = r - (r / cw) * cw;
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < MAXK; ++j) {
        if (j == c.n) {
          c.z[j] = pick[0];
          c.y[j] = pick[1];
          c.x[j] = pick[2];
        }
      }
      c.n += 1;
      zl = pick[0];
    }
  }
  if (threadIdx.x == 0) {
    int32_t* o = pts + ((int64_t)n * 2 + kind) * MAXK * 3;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      o[3 * k + 0] = k < c.n ? c.z[k] : -1;
      o[3 * k + 1] = k < c.n ? c.y[k] : -1;
      o[3 * k + 2] = k < c.n ? c.x[k] : -1;
    }
    cnt[(int64_t)n * 2 + kind] = c.n;
  }
}

// ------------------------------------------------------------------------------------------------ guide
struct Guide3 {
  bool gaussian;
  float nz, ny, nx, norm;        // 2 s^2 per axis; the Euclidean divisor
};
// create_spatial_guide_3d at one crop voxel: min_k sqrt(dz^2 + dy^2 + dx^2) = sqrt(min_k ...) (the squares are exact
// integers), divided as data_processing :372 divides it; or max_k exp(-(dz^2 / (2 sz^2) + dy^2 / (2 sy^2) + dx^2 / (2 sx^2))),
// summed z, y, x as image_ops.py:471 sums them
// (oz, oy, ox): what is subtracted from the clicks, in integers, before they are used -- the crop box's origin for clicks in
// case coordinates (click_guide3d_kernel<true>), 0 for clicks relative to the box
__device__ __forceinline__ float cg3_at(int pz, int py, int px, const int32_t* __restrict__ p, int n, const Guide3& g, int oz = 0,
                                        int oy = 0, int ox = 0) {
  if (n == 0) return 0.f;
  float best = g.gaussian ? 0.f : INFINITY;
  for (int k = 0; k < n; ++k) {
    const float dz = (float)pz - (float)(p[3 * k] - oz), dy = (float)py - (float)(p[3 * k + 1] - oy),
                dx = (float)px - (float)(p[3 * k + 2] - ox);
    if (g.gaussian)
      best = fmaxf(best, expf(-(dz * dz / g.nz + dy * dy / g.ny + dx * dx / g.nx)));
    else
      best = fminf(best, dz * dz + dy * dy + dx * dx);
  }
  return g.gaussian ? best : sqrtf(best) / g.norm;
}
// LIST: ONE pair of click lists for all rows, pts [2][K][3] in case coordinates (z from the case's first slice, y and x in the
// slice) and cnt [2] (unetk_click_guide3d_list); else pts [N][2][MAXK][3] relative to each row's box and cnt [N][2]
// ROT (unetk_click_guide3d_rot): ONLY the rows whose table columns 13 / 14 are not both bit-zero; the guide is
// evaluated at the four UNCLAMPED corners of the turned coordinate (lits_rot_coord, the patch kernel's): it is a function of
// position, so a corner beyond the crop box is simply evaluated there; an invalid coordinate gives 0.  The rows that are not
// rotated are left to the plain kernel, which the entry point launches first (click_guide3d_launch says why).
template <bool LIST, bool ROT>
__global__ __launch_bounds__(256) void click_guide3d_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                            const int32_t* __restrict__ pts, const int32_t* __restrict__ cnt,
                                                            int K, float* __restrict__ guide) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int area = d.H * d.W, vol = d.D * area;              // < 2^31: checked by the entry point
  if (i >= (int64_t)d.N * vol) return;
  const int n = (int)(i / vol), r = (int)(i - (int64_t)n * vol);
  const int z = r / area, q = r - z * area;
  const int y = q / d.W, x = q - y * d.W;
  const int32_t* t = tab + (int64_t)n * TW;
  const Box3 b = p3d_box(t, d);
  LitsTaps ty, tx;
  int y0, x0;
  bool ok = true;
  if (ROT) {
    const LitsRot rot = lits_rot_of(t);
    if (!rot.on) return;                                     // the plain kernel has written this row
    const LitsRotAt at = lits_rot_coord(y, x, b.ch, b.cw, lits_ac_scale(b.ch, d.H), lits_ac_scale(b.cw, d.W), rot);
    ok = at.ok;
    const float fy0 = ok ? floorf(at.in_y) : 0.f, fx0 = ok ? floorf(at.in_x) : 0.f;
    y0 = (int)fy0;
    x0 = (int)fx0;
    ty.i0 = y0;
    ty.i1 = y0 + 1;
    ty.f = ok ? at.in_y - fy0 : 0.f;
    tx.i0 = x0;
    tx.i1 = x0 + 1;
    tx.f = ok ? at.in_x - fx0 : 0.f;
  } else {
    ty = lits_ac_taps(y * lits_ac_scale(b.ch, d.H), b.ch);
    tx = lits_ac_taps(x * lits_ac_scale(b.cw, d.W), b.cw);
    y0 = min(ty.i0, b.ch - 1);
    x0 = min(tx.i0, b.cw - 1);
  }
  Guide3 g;
  g.gaussian = d.gaussian != 0;
  g.nz = 2.f * d.stddev[0] * d.stddev[0];
  g.ny = 2.f * d.stddev[1] * d.stddev[1];
  g.nx = 2.f * d.stddev[2] * d.stddev[2];
  g.norm = d.euclid_norm;
  float v[2];
#pragma unroll
  for (int kind = 0; kind < 2; ++kind) {
    const int32_t* p = LIST ? pts + (int64_t)kind * K * 3 : pts + ((int64_t)n * 2 + kind) * MAXK * 3;
    const int k = min(max(cnt[LIST ? kind : (int64_t)n * 2 + kind], 0), LIST ? K : MAXK);
    const int oz = LIST ? b.z1 : 0, oy = LIST ? b.y1 : 0, ox = LIST ? b.x1 : 0;
    const float tl = cg3_at(z, y0, x0, p, k, g, oz, oy, ox), tr = cg3_at(z, y0, tx.i1, p, k, g, oz, oy, ox);
    const float bl = cg3_at(z, ty.i1, x0, p, k, g, oz, oy, ox), br = cg3_at(z, ty.i1, tx.i1, p, k, g, oz, oy, ox);
    v[kind] = lits_bilerp(tl, tr, bl, br, tx.f, ty.f);
    if (ROT && !ok) v[kind] = 0.f;
  }
  const int zo = t[9] != 0 ? d.D - 1 - z : z, yo = t[8] != 0 ? d.H - 1 - y : y, xo = t[7] != 0 ? d.W - 1 - x : x;
  const int64_t o = (int64_t)n * vol + ((int64_t)zo * d.H + yo) * d.W + xo;
  if (d.G == 2) {
    guide[o * 2 + 0] = v[0];
    guide[o * 2 + 1] = v[1];
  } else {
    guide[o] = v[0] - v[1];
  }
}

// WARP (unetk_click_guide3d_warp): ONLY the rows whose table column 15 is not zero, after the plain kernel
// and the rotated rows' kernel have written every row (so the rows that are not deformed keep those kernels' bits).  The
// guide is evaluated at the four unclamped corners of the coordinate p3d_warp_kernel (lits3d.hip) samples the slice at --
// lits_warp_coord, the same float32 operations -- exactly as ROT evaluates it at the turned coordinate.  One thread per
// voxel, as above: the spline is re-evaluated per slice (32 cached lattice reads beside up to 4 * 2 * MAXK expf), which keeps
// the grid and the write order of click_guide3d_kernel.
__global__ __launch_bounds__(256) void click_guide3d_warp_kernel(unetk_lits3d_clicks_desc d, const int32_t* __restrict__ tab,
                                                                 const float* __restrict__ warp, int WG,
                                                                 const int32_t* __restrict__ pts, const int32_t* __restrict__ cnt,
                                                                 float* __restrict__ guide) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int area = d.H * d.W, vol = d.D * area;              // < 2^31: checked by the entry point
  if (i >= (int64_t)d.N * vol) return;
  const int n = (int)(i / vol), r = (int)(i - (int64_t)n * vol);
  const int32_t* t = tab + (int64_t)n * TW;
  if (t[15] == 0) return;                                    // the kernels before this one have written the row
  const int z = r / area, q = r - z * area;
  const int y = q / d.W, x = q - y * d.W;
  const Box3 b = p3d_box(t, d);
  const int cells = (WG + 3) * (WG + 3);
  const float* lat = warp + (int64_t)n * 2 * cells;
  const LitsSpline sy = lits_warp_spline(y, d.H, WG), sx = lits_warp_spline(x, d.W, WG);
  const LitsRotAt at = lits_warp_coord(y, x, lits_warp_disp(lat, WG, sy, sx), lits_warp_disp(lat + cells, WG, sy, sx), b.ch, b.cw,
                                       lits_ac_scale(b.ch, d.H), lits_ac_scale(b.cw, d.W), lits_rot_of(t));
  const bool ok = at.ok;
  const float fy0 = ok ? floorf(at.in_y) : 0.f, fx0 = ok ? floorf(at.in_x) : 0.f;
  const int y0 = (int)fy0, x0 = (int)fx0;
  const float fy = ok ? at.in_y - fy0 : 0.f, fx = ok ? at.in_x - fx0 : 0.f;
  Guide3 g;
  g.gaussian = d.gaussian != 0;
  g.nz = 2.f * d.stddev[0] * d.stddev[0];
  g.ny = 2.f * d.stddev[1] * d.stddev[1];
  g.nx = 2.f * d.stddev[2] * d.stddev[2];
  g.norm = d.euclid_norm;
  float v[2];
#pragma unroll
  for (int kind = 0; kind < 2; ++kind) {
    const int32_t* p = pts + ((int64_t)n * 2 + kind) * MAXK * 3;
    const int k = min(max(cnt[(int64_t)n * 2 + kind], 0), MAXK);
    const float tl = cg3_at(z, y0, x0, p, k, g), tr = cg3_at(z, y0, x0 + 1, p, k, g);
    const float bl = cg3_at(z, y0 + 1, x0, p, k, g), br = cg3_at(z, y0 + 1, x0 + 1, p, k, g);
    v[kind] = ok ? lits_bilerp(tl, tr, bl, br, fx, fy) : 0.f;
  }
  const int zo = t[9] != 0 ? d.D - 1 - z : z, yo = t[8] != 0 ? d.H - 1 - y : y, xo = t[7] != 0 ? d.W - 1 - x : x;
  const int64_t o = (int64_t)n * vol + ((int64_t)zo * d.H + yo) * d.W + xo;
  if (d.G == 2) {
    guide[o * 2 + 0] = v[0];
    guide[o * 2 + 1] = v[1];
  } else {
    guide[o] = v[0] - v[1];
  }
}

// ------------------------------------------------------------------------------------------------ host side
bool clk3_valid(const unetk_lits3d_clicks_desc* d) {
  return d && d->N > 0 && d->N <= 65535 && d->D > 0 && d->H > 0 && d->W > 0 && d->n_slices > 0 && d->src_h > 0 && d->src_w > 0 &&
         d->lab_scale > 0 && d->obj_label > 0 && (int64_t)d->lab_scale * d->obj_label < ((int64_t)1 << 31);
}
bool clk3_supported(const unetk_lits3d_clicks_desc* d) {
  return d->margin >= 1 && d->band >= 1 && d->step >= 0 && d->step <= 16384 && (int64_t)d->margin + d->band <= 254 &&
         d->max_clicks >= 2 && d->max_clicks <= MAXK + 1 && d->src_h <= CLK_MAX_EXTENT && d->src_w <= CLK_MAX_EXTENT &&
         d->D <= CLK3_MAX_D && (int64_t)d->D * d->src_h * d->src_w < ((int64_t)1 << 31);
}

}  // namespace

extern "C" size_t unetk_lits3d_clicks_ws_bytes(const unetk_lits3d_clicks_desc* d) {
  if (!clk3_valid(d) || !clk3_supported(d)) return 0;
  return (size_t)d->N * 3 * (size_t)clk3_field(*d) + (size_t)d->N * d->D * d->src_h * CLK3_REC * sizeof(int32_t);
}

namespace {
template <bool NEG>
int clk3_launch(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const uint8_t* neg_slices, const int32_t* sample_tab,
                const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  UNETK_REQUIRE(clk3_valid(d) && seg_slices && (!NEG || neg_slices) && sample_tab && click_tab && pts && cnt && status && ws);
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)click_tab) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)status)) & 3u) == 0);
  UNETK_REQUIRE(unetk_aligned16(ws));
  if (!clk3_supported(d)) return UNETK_E_UNSUPPORTED;
  if (ws_bytes < unetk_lits3d_clicks_ws_bytes(d)) return UNETK_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = static_cast<uint8_t*>(ws);
  int32_t* rowrec = reinterpret_cast<int32_t*>(w + (size_t)d->N * 3 * (size_t)clk3_field(*d));
  UNETK_LAUNCH(clk3_cols_kernel, dim3((d->src_w + 63) / 64, d->D, d->N), dim3(64), 0, st, *d, seg_slices, sample_tab, w);
  UNETK_LAUNCH(clk3_rows_kernel<NEG>, dim3(d->src_h, d->D, d->N), dim3(256), 0, st, *d, sample_tab, neg_slices, w, rowrec);
  UNETK_LAUNCH(clk3_select_kernel<NEG>, dim3(2, d->N), dim3(1024), 0, st, *d, sample_tab, click_tab, (const uint8_t*)w,
               (const int32_t*)rowrec, pts, cnt, status);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
}  // namespace

extern "C" int unetk_lits3d_clicks(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const int32_t* sample_tab,
                                   const uint32_t* click_tab, int32_t* pts, int32_t* cnt, int32_t* status, void* ws,
                                   size_t ws_bytes, void* stream) {
  return clk3_launch<false>(d, seg_slices, nullptr, sample_tab, click_tab, pts, cnt, status, ws, ws_bytes, stream);
}

extern "C" int unetk_lits3d_clicks_neg(const unetk_lits3d_clicks_desc* d, const uint8_t* seg_slices, const uint8_t* neg_slices,
                                       const int32_t* sample_tab, const uint32_t* click_tab, int32_t* pts, int32_t* cnt,
                                       int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  return clk3_launch<true>(d, seg_slices, neg_slices, sample_tab, click_tab, pts, cnt, status, ws, ws_bytes, stream);
}

namespace {
// K == 0: unetk_click_guide3d (clicks per row, relative to its box), with rot unetk_click_guide3d_rot; else
// unetk_click_guide3d_list
// warp != nullptr (implies rot): unetk_click_guide3d_warp
int click_guide3d_launch(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts, const int32_t* cnt,
                         int K, float* guide, void* stream, bool rot = false, const float* warp = nullptr, int WG = 0) {
  UNETK_REQUIRE(d && d->N > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->src_h > 0 && d->src_w > 0 && sample_tab && pts && cnt &&
                guide && (d->G == 1 || d->G == 2));
  UNETK_REQUIRE(((((uintptr_t)sample_tab) | ((uintptr_t)pts) | ((uintptr_t)cnt) | ((uintptr_t)guide)) & 3u) == 0);
  UNETK_REQUIRE(d->gaussian != 0 ? (d->stddev[0] > 0.f && d->stddev[1] > 0.f && d->stddev[2] > 0.f) : d->euclid_norm > 0.f);
  const int64_t total = (int64_t)d->N * d->D * d->H * d->W;
  if ((int64_t)d->D * d->H * d->W >= ((int64_t)1 << 31) || (total + 255) / 256 >= ((int64_t)1 << 31)) return UNETK_E_UNSUPPORTED;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (K > 0)
    UNETK_LAUNCH((click_guide3d_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, pts, cnt, K, guide);
  else
    UNETK_LAUNCH((click_guide3d_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, pts, cnt, 0, guide);
  // Rotated rows are written again by a kernel of their own, after the plain kernel has written every row.  One kernel that
  // branched per row was tried: the compiler contracted the plain statements differently next to the rotated ones (the
  // fraction y * scale - i0 became a fused multiply-add), and the rows that are not rotated were no longer the bits of
  // unetk_click_guide3d.  Running the SAME compiled kernel on them makes that equality hold by construction, for the price
  // of evaluating the rotated rows twice (the guide is the small part of a guided batch: DESIGN.md 7.3.9).
  if (rot)
    UNETK_LAUNCH((click_guide3d_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, pts, cnt, 0, guide);
  // and the deformed rows once more, for the same reason
  if (warp)
    UNETK_LAUNCH(click_guide3d_warp_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, sample_tab, warp, WG, pts, cnt, guide);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
}  // namespace

extern "C" int unetk_click_guide3d(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts,
                                   const int32_t* cnt, float* guide, void* stream) {
  return click_guide3d_launch(d, sample_tab, pts, cnt, 0, guide, stream);
}

extern "C" int unetk_click_guide3d_rot(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts,
                                       const int32_t* cnt, float* guide, void* stream) {
  return click_guide3d_launch(d, sample_tab, pts, cnt, 0, guide, stream, true);
}

extern "C" int unetk_click_guide3d_warp(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const float* warp, int G,
                                        const int32_t* pts, const int32_t* cnt, float* guide, void* stream) {
  UNETK_REQUIRE(warp && (((uintptr_t)warp) & 3u) == 0 && G >= 1 && G <= LITS_WARP_MAX_G);
  return click_guide3d_launch(d, sample_tab, pts, cnt, 0, guide, stream, true, warp, G);
}

extern "C" int unetk_click_guide3d_list(const unetk_lits3d_clicks_desc* d, const int32_t* sample_tab, const int32_t* pts,
                                        const int32_t* cnt, int K, float* guide, void* stream) {
  UNETK_REQUIRE(K >= 1 && K <= UNETK_INTER_MAX_CLICKS);
  return click_guide3d_launch(d, sample_tab, pts, cnt, K, guide, stream);
}
