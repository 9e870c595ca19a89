// Input and output side of the offline volume evaluation (data/lits.py get_dataset_for_eval_image[_v2],
// evaluators/evaluator_liver.py _predict_case): the network's input slabs are built from a case's resident HU crop, and
// the argmax volume is zoomed back to the crop's shape, without the volume crossing to the host in between; with
// --save_predict the post-processed masks are composed into the whole case in NIfTI file order (unetk_nii_compose), so
// one copy brings the file's data to the host.  The way in of `liver_3d --mode infer` is here too: a NIfTI file's voxel block
// becomes store slices (unetk_nii_ingest, the compose's walk the other way round), and --pred_type prob composes a class's
// probabilities in file order (unetk_eval3d_prob).  Every kernel writes each output element exactly once, by plain stores, no
// atomics and no workspace.
//
// Threads walk the FLAT output (the contiguous axis fastest): a thread owns V consecutive elements = one 16-byte store,
// decomposes the index of its first element once (32-bit divisions) and steps the coordinates with carries, so 16-byte
// stores do not need rows of a suitable length; a base pointer that is not 16-byte aligned takes the one-element variant,
// and the elements past the last whole group are stored one by one.
#include "common.h"

// hipcc contracts a * b + c into an FMA by default, also through __fmul_rn / __fadd_rn (plain operators in its headers):
// the host rule rounds every product and sum on its own (numpy float32), so contraction is switched off for this file.
#pragma clang fp contract(off)

namespace {

constexpr int EIO_BLOCK = 256;
constexpr int EIO_ITERS = 4;                 // groups per thread: amortises the window table's trip into LDS
constexpr int EIO_LUT_MAX = 16384;           // window entries kept in LDS (64 KiB); the LiTS window has 451

struct SlabArgs {
  const int16_t* vol;
  const int32_t* zsrc;
  const int32_t *y0, *y1, *x0, *x1;
  const float *fy, *fx, *lut;
  float* out;
  int src_d, src_h, src_w, N, H, W, C, lo, hi;
  int total;                                 // N * H * W * C
};

__device__ __forceinline__ int eio_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one output element by the host's rule, every operation rounded on its own: rows first, then columns
__device__ __forceinline__ float slab_px(const SlabArgs& a, const float* s_lut, int n, int y, int x, int c) {
  const int z = a.zsrc[n * a.C + c];
  if (z < 0 ? z != -2 : z >= a.src_d) return 0.0f;            // -1: a plane of 0.0f (0 * w + 0 * w' is exactly 0)
  float v00, v01, v10, v11;
  if (z == -2) {
    v00 = v01 = v10 = v11 = s_lut[eio_clamp(0, a.lo, a.hi) - a.lo];
  } else {
    const int ya = eio_clamp(a.y0[y], 0, a.src_h - 1), yb = eio_clamp(a.y1[y], 0, a.src_h - 1);
    const int xa = eio_clamp(a.x0[x], 0, a.src_w - 1), xb = eio_clamp(a.x1[x], 0, a.src_w - 1);
    const int16_t* ra = a.vol + (z * a.src_h + ya) * a.src_w;
    const int16_t* rb = a.vol + (z * a.src_h + yb) * a.src_w;
    v00 = s_lut[eio_clamp(ra[xa], a.lo, a.hi) - a.lo];
    v01 = s_lut[eio_clamp(ra[xb], a.lo, a.hi) - a.lo];
    v10 = s_lut[eio_clamp(rb[xa], a.lo, a.hi) - a.lo];
    v11 = s_lut[eio_clamp(rb[xb], a.lo, a.hi) - a.lo];
  }
  const float fy = a.fy[y], fx = a.fx[x];
  const float gy = 1.0f - fy, gx = 1.0f - fx;
  const float r0 = v00 * gy + v10 * fy;
  const float r1 = v01 * gy + v11 * fy;
  return r0 * gx + r1 * fx;
}

// the coordinates of the next element of the flat [N, H, W, C] output
__device__ __forceinline__ void slab_next(const SlabArgs& a, int& n, int& y, int& x, int& c) {
  if (++c < a.C) return;
  c = 0;
  if (++x < a.W) return;
  x = 0;
  if (++y < a.H) return;
  y = 0;
  ++n;
}

template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void eval_slab_kernel(SlabArgs a) {
  extern __shared__ float s_lut[];
  for (int i = threadIdx.x; i <= a.hi - a.lo; i += EIO_BLOCK) s_lut[i] = a.lut[i];
  __syncthreads();
  const int groups = a.total / V;
#pragma unroll 1
  for (int it = 0; it < EIO_ITERS; ++it) {
    const unsigned g = (blockIdx.x * EIO_ITERS + it) * EIO_BLOCK + threadIdx.x;   // unsigned: may pass 2^31 past the end
    if (g > (unsigned)groups) return;
    const int e = (int)g * V;
    const int count = g < (unsigned)groups ? V : a.total - e;  // g == groups: the elements past the last whole group
    if (count <= 0) return;
    unsigned t = (unsigned)e;
    int c = (int)(t % (unsigned)a.C);
    t /= (unsigned)a.C;
    int x = (int)(t % (unsigned)a.W);
    t /= (unsigned)a.W;
    int y = (int)(t % (unsigned)a.H);
    int n = (int)(t / (unsigned)a.H);
    if (count == V) {
      float v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        v[k] = slab_px(a, s_lut, n, y, x, c);
        slab_next(a, n, y, x, c);
      }
      if (V == 4) {
        stg4(a.out + e, make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]));
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) a.out[e + k] = v[k];
      }
    } else {
      for (int k = 0; k < count; ++k) {
        a.out[e + k] = slab_px(a, s_lut, n, y, x, c);
        slab_next(a, n, y, x, c);
      }
    }
  }
}

struct ZoomArgs {
  const uint8_t* src;
  const int32_t *tz, *ty, *tx;
  uint8_t* dst;
  int d, h, w, D, H, W;
  int total;                                 // D * H * W
};

// first source index of output row (z, y), or -1 when either table sends the row outside
__device__ __forceinline__ int zoom_row(const ZoomArgs& a, int z, int y) {
  const int sz = a.tz[z], sy = a.ty[y];
  if ((unsigned)sz >= (unsigned)a.d || (unsigned)sy >= (unsigned)a.h) return -1;
  return (sz * a.h + sy) * a.w;
}

__device__ __forceinline__ uint32_t zoom_px(const ZoomArgs& a, int row, int x) {
  const int sx = a.tx[x];
  return row >= 0 && (unsigned)sx < (unsigned)a.w ? a.src[row + sx] : 0u;
}

// the next voxel of the flat [D, H, W] output; never called past the last voxel (the tables end there)
__device__ __forceinline__ void zoom_next(const ZoomArgs& a, int& z, int& y, int& x, int& row) {
  if (++x < a.W) return;
  x = 0;
  if (++y == a.H) {
    y = 0;
    ++z;
  }
  row = zoom_row(a, z, y);
}

template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void zoom_nearest3d_kernel(ZoomArgs a) {
  const int groups = a.total / V;
  const unsigned g = blockIdx.x * EIO_BLOCK + threadIdx.x;
  if (g > (unsigned)groups) return;
  const int e = (int)g * V;
  const int count = g < (unsigned)groups ? V : a.total - e;
  if (count <= 0) return;
  unsigned t = (unsigned)e;
  int x = (int)(t % (unsigned)a.W);
  t /= (unsigned)a.W;
  int y = (int)(t % (unsigned)a.H);
  int z = (int)(t / (unsigned)a.H);
  int row = zoom_row(a, z, y);
  if (count == V) {
    uint32_t word[(V + 3) / 4] = {};
#pragma unroll
    for (int k = 0; k < V; ++k) {
      word[k / 4] |= zoom_px(a, row, x) << (8 * (k % 4));
      if (k + 1 < V) zoom_next(a, z, y, x, row);
    }
    if (V == 16) {
      constexpr int NW = (V + 3) / 4;
      *reinterpret_cast<uint4*>(a.dst + e) = make_uint4(word[0], word[1 % NW], word[2 % NW], word[3 % NW]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) a.dst[e + k] = (uint8_t)(word[k / 4] >> (8 * (k % 4)));
    }
  } else {
    for (int k = 0; k < count; ++k) {
      a.dst[e + k] = (uint8_t)zoom_px(a, row, x);
      if (k + 1 < count) zoom_next(a, z, y, x, row);
    }
  }
}

// ---- predicted volume in NIfTI file order (evaluator_liver.py:998-1026 maybe_save_case + nii_kits.write_nii)
// Everything is expressed per FILE axis k (0 = fastest): its length n, whether the data index runs backwards along it, and
// of the data axis it runs along the box origin o, the box extent b and the masks' stride ms.  File index i_k is box
// coordinate q_k = (flip ? n - 1 - i : i) - o; a voxel is inside the box when every 0 <= q_k < b_k.
struct NiiArgs {
  const uint8_t *liver, *tumor;
  int16_t* dst;
  int n[3], flip[3], o[3], b[3], ms[3];
  int total;                                 // n[0] * n[1] * n[2]
};

__device__ __forceinline__ int nii_q(const NiiArgs& a, int k, int i) { return (a.flip[k] ? a.n[k] - 1 - i : i) - a.o[k]; }

__device__ __forceinline__ int nii_px(const NiiArgs& a, int off) {
  int v = 0;
  if (a.liver) v += a.liver[off];
  if (a.tumor) v += a.tumor[off];
  return v;
}

__device__ __forceinline__ int nii_voxel(const NiiArgs& a, int i0, int i1, int i2) {
  const int q0 = nii_q(a, 0, i0), q1 = nii_q(a, 1, i1), q2 = nii_q(a, 2, i2);
  if ((unsigned)q0 >= (unsigned)a.b[0] || (unsigned)q1 >= (unsigned)a.b[1] || (unsigned)q2 >= (unsigned)a.b[2]) return 0;
  return nii_px(a, q0 * a.ms[0] + q1 * a.ms[1] + q2 * a.ms[2]);
}

// eight consecutive mask bytes from any address (the box origin and width are arbitrary); global loads need no alignment
__device__ __forceinline__ uint64_t nii_ld8(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// File axis 0 runs along data x (ms[0] == 1): a thread owns V consecutive file elements = one 16-byte store.  A group inside
// one file row whose x run lies inside the box reads 8 bytes of each mask at once; an x flip reverses them in the registers.
template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void nii_compose_rows_kernel(NiiArgs a) {
  const int groups = a.total / V;
  const unsigned g = blockIdx.x * EIO_BLOCK + threadIdx.x;
  if (g > (unsigned)groups) return;
  const int e = (int)g * V;
  const int count = g < (unsigned)groups ? V : a.total - e;
  if (count <= 0) return;
  unsigned t = (unsigned)e;
  int i0 = (int)(t % (unsigned)a.n[0]);
  t /= (unsigned)a.n[0];
  int i1 = (int)(t % (unsigned)a.n[1]);
  int i2 = (int)(t / (unsigned)a.n[1]);
  if (V == 8 && count == V && i0 + V <= a.n[0]) {
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    const int q1 = nii_q(a, 1, i1), q2 = nii_q(a, 2, i2);
    const int qlo = (a.flip[0] ? a.n[0] - V - i0 : i0) - a.o[0];          // lowest box x of the group
    if ((unsigned)q1 < (unsigned)a.b[1] && (unsigned)q2 < (unsigned)a.b[2] && qlo + V > 0 && qlo < a.b[0]) {
      const int row = q1 * a.ms[1] + q2 * a.ms[2];
      int v[8];
      if (qlo >= 0 && qlo + V <= a.b[0]) {
        const uint64_t l = a.liver ? nii_ld8(a.liver + row + qlo) : 0ull;
        const uint64_t m = a.tumor ? nii_ld8(a.tumor + row + qlo) : 0ull;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (int)((l >> (8 * j)) & 0xffu) + (int)((m >> (8 * j)) & 0xffu);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (unsigned)(qlo + j) < (unsigned)a.b[0] ? nii_px(a, row + qlo + j) : 0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) word[k / 2] |= (uint32_t)(a.flip[0] ? v[7 - k] : v[k]) << (16 * (k % 2));
    }
    *reinterpret_cast<uint4*>(a.dst + e) = make_uint4(word[0], word[1], word[2], word[3]);
  } else {
    for (int k = 0; k < count; ++k) {
      a.dst[e + k] = (int16_t)nii_voxel(a, i0, i1, i2);
      if (++i0 == a.n[0]) {
        i0 = 0;
        if (++i1 == a.n[1]) {
          i1 = 0;
          ++i2;
        }
      }
    }
  }
}

// File axis 0 runs along data y or z, data x along file axis KX (1 or 2): per index of the third axis, a transpose of
// NII_TILE x NII_TILE tiles through LDS.  Lanes walk data x while reading the masks and file axis 0 while storing, so both
// sides touch consecutive addresses; a row stride of 33 words keeps the column reads out of each other's LDS banks.
constexpr int NII_TILE = 64;

template <int KX>
__global__ __launch_bounds__(EIO_BLOCK) void nii_compose_tr_kernel(NiiArgs a) {
  __shared__ int16_t tile[NII_TILE][NII_TILE + 2];
  constexpr int KR = 3 - KX;
  const int base0 = blockIdx.x * NII_TILE;
  for (int ir = blockIdx.z; ir < a.n[KR]; ir += gridDim.z) {
    for (int basex = blockIdx.y * NII_TILE; basex < a.n[KX]; basex += gridDim.y * NII_TILE) {
      for (int t = threadIdx.x; t < NII_TILE * NII_TILE; t += EIO_BLOCK) {
        const int xi = t % NII_TILE, ai = t / NII_TILE;
        const int i0 = base0 + ai, ix = basex + xi;
        if (i0 < a.n[0] && ix < a.n[KX]) tile[ai][xi] = (int16_t)nii_voxel(a, i0, KX == 1 ? ix : ir, KX == 1 ? ir : ix);
      }
      __syncthreads();
      for (int t = threadIdx.x; t < NII_TILE * NII_TILE; t += EIO_BLOCK) {
        const int ai = t % NII_TILE, xi = t / NII_TILE;
        const int i0 = base0 + ai, ix = basex + xi;
        if (i0 < a.n[0] && ix < a.n[KX]) {
          const int i1 = KX == 1 ? ix : ir, i2 = KX == 1 ? ir : ix;
          a.dst[i0 + a.n[0] * (i1 + a.n[1] * i2)] = tile[ai][xi];
        }
      }
      __syncthreads();
    }
  }
}

// ---- a NIfTI file's voxel block to store slices (unetk_nii_ingest: nii_kits.read_nii + the store's encoding, extract.py:72)
// The inverse walk of the compose above, per FILE axis k (0 = fastest): its length n, whether the data index runs backwards
// along it, and the stride ds of the data axis it runs along in dst [d,h,w].  File voxel (i0, i1, i2) lands at
// sum_k (flip_k ? n_k - 1 - i_k : i_k) * ds_k; the map is a bijection, so every element of dst is written exactly once.
struct IngestArgs {
  const void* src;
  uint16_t* dst;
  double slope, inter;
  int n[3], flip[3], ds[3];
  int code, scaled, lo, hi, scale;
  int total;                                 // n[0] * n[1] * n[2]
};

// float64 -> int16 as the host casts it where numpy defines the cast (truncation toward zero); this project's rule where it
// does not: NaN gives 0, values beyond the int16 range saturate
__device__ __forceinline__ int ingest_cast(double v) {
  if (v != v) return 0;
  if (v >= 32767.0) return 32767;
  if (v <= -32768.0) return -32768;
  return (int)v;
}

__device__ __forceinline__ int ingest_int(const IngestArgs& a, long long r) {
  if (a.scaled) return ingest_cast((double)r * a.slope + a.inter);          // two roundings, as numpy's (no FMA in this file)
  return (int)(r > 32767 ? 32767 : r < -32768 ? -32768 : r);
}

__device__ __forceinline__ int ingest_real(const IngestArgs& a, double v) {
  return ingest_cast(a.scaled ? v * a.slope + a.inter : v);
}

__device__ __forceinline__ uint16_t ingest_encode(const IngestArgs& a, int v16) {
  return (uint16_t)((min(max(v16, a.lo), a.hi) - a.lo) * a.scale);
}

// file element e (NIfTI datatype codes) by the value rule
__device__ __forceinline__ uint16_t ingest_px(const IngestArgs& a, int e) {
  int v16;
  switch (a.code) {
    case 2: v16 = ingest_int(a, static_cast<const uint8_t*>(a.src)[e]); break;
    case 4: v16 = ingest_int(a, static_cast<const int16_t*>(a.src)[e]); break;
    case 8: v16 = ingest_int(a, static_cast<const int32_t*>(a.src)[e]); break;
    case 16: v16 = ingest_real(a, (double)static_cast<const float*>(a.src)[e]); break;
    case 64: v16 = ingest_real(a, static_cast<const double*>(a.src)[e]); break;
    case 256: v16 = ingest_int(a, static_cast<const int8_t*>(a.src)[e]); break;
    case 512: v16 = ingest_int(a, static_cast<const uint16_t*>(a.src)[e]); break;
    default: v16 = ingest_int(a, static_cast<const uint32_t*>(a.src)[e]); break;      // 768
  }
  return ingest_encode(a, v16);
}

__device__ __forceinline__ int ingest_c(const IngestArgs& a, int k, int i) { return a.flip[k] ? a.n[k] - 1 - i : i; }

// File axis 0 runs along data x (ds[0] == 1).  V == 1: one file element per thread, any datatype.  V == 8 (int16 without
// scaling, src 16-byte aligned): a thread owns eight consecutive file elements = one 16-byte load; a group inside one file row
// is reversed in the registers when x is flipped and leaves in one 16-byte store where its place in dst is 16-byte aligned
// (every group of a row whose length is a multiple of 8, as LiTS's 512), else in eight 2-byte stores.
template <int V>
__global__ __launch_bounds__(EIO_BLOCK) void nii_ingest_rows_kernel(IngestArgs a) {
  const int groups = a.total / V;
  const unsigned g = blockIdx.x * EIO_BLOCK + threadIdx.x;
  if (g > (unsigned)groups) return;
  const int e = (int)g * V;
  const int count = g < (unsigned)groups ? V : a.total - e;
  if (count <= 0) return;
  unsigned t = (unsigned)e;
  int i0 = (int)(t % (unsigned)a.n[0]);
  t /= (unsigned)a.n[0];
  int i1 = (int)(t % (unsigned)a.n[1]);
  int i2 = (int)(t / (unsigned)a.n[1]);
  if (V == 8 && count == V && i0 + V <= a.n[0]) {
    const uint4 raw = *reinterpret_cast<const uint4*>(static_cast<const int16_t*>(a.src) + e);
    const uint32_t in[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t enc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) enc[j] = ingest_encode(a, (int)(int16_t)(in[j / 2] >> (16 * (j % 2))));
    uint16_t* out = a.dst + ingest_c(a, 1, i1) * a.ds[1] + ingest_c(a, 2, i2) * a.ds[2] + (a.flip[0] ? a.n[0] - V - i0 : i0);
    if ((((uintptr_t)out) & 15u) == 0) {
      uint32_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) word[k / 2] |= (a.flip[0] ? enc[7 - k] : enc[k]) << (16 * (k % 2));
      *reinterpret_cast<uint4*>(out) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) out[k] = (uint16_t)(a.flip[0] ? enc[7 - k] : enc[k]);
    }
  } else {
    for (int k = 0; k < count; ++k) {
      a.dst[ingest_c(a, 0, i0) + ingest_c(a, 1, i1) * a.ds[1] + ingest_c(a, 2, i2) * a.ds[2]] = ingest_px(a, e + k);
      if (++i0 == a.n[0]) {
        i0 = 0;
        if (++i1 == a.n[1]) {
          i1 = 0;
          ++i2;
        }
      }
    }
  }
}

// File axis 0 runs along data y or z, data x along file axis KX (1 or 2): per index of the third axis, the transpose of
// nii_compose_tr_kernel the other way round.  Lanes walk file axis 0 while reading the file and data x while storing, so both
// sides touch consecutive addresses (backwards under a flip); the same row stride of 33 words keeps the column reads of the
// second phase out of each other's LDS banks.
template <int KX>
__global__ __launch_bounds__(EIO_BLOCK) void nii_ingest_tr_kernel(IngestArgs a) {
  __shared__ uint16_t tile[NII_TILE][NII_TILE + 2];
  constexpr int KR = 3 - KX;
  const int base0 = blockIdx.x * NII_TILE;
  for (int ir = blockIdx.z; ir < a.n[KR]; ir += gridDim.z) {
    for (int basex = blockIdx.y * NII_TILE; basex < a.n[KX]; basex += gridDim.y * NII_TILE) {
      for (int t = threadIdx.x; t < NII_TILE * NII_TILE; t += EIO_BLOCK) {
        const int ai = t % NII_TILE, xi = t / NII_TILE;
        const int i0 = base0 + ai, ix = basex + xi;
        if (i0 < a.n[0] && ix < a.n[KX]) {
          const int i1 = KX == 1 ? ix : ir, i2 = KX == 1 ? ir : ix;
          tile[xi][ai] = ingest_px(a, i0 + a.n[0] * (i1 + a.n[1] * i2));
        }
      }
      __syncthreads();
      for (int t = threadIdx.x; t < NII_TILE * NII_TILE; t += EIO_BLOCK) {
        const int xi = t % NII_TILE, ai = t / NII_TILE;
        const int i0 = base0 + ai, ix = basex + xi;
        if (i0 < a.n[0] && ix < a.n[KX])
          a.dst[ingest_c(a, 0, i0) * a.ds[0] + ingest_c(a, KX, ix) + ingest_c(a, KR, ir) * a.ds[KR]] = tile[xi][ai];
      }
      __syncthreads();
    }
  }
}

// ---- class probabilities of a sliding-window case in NIfTI file order (unetk_eval3d_prob).  One thread per FILE element, the
// flat file index fastest along the lanes: the stores are consecutive bytes for every orientation; the reads are consecutive
// voxels of acc (stride C floats) and of the weight when file axis 0 is data x, and strided gathers otherwise.
struct ProbArgs {
  const float *acc, *wsum;
  const int32_t* cnt;
  uint8_t* dst;
  int n[3], flip[3], ds[3], o[3], b[3];      // per file axis; ds: the voxel stride of its data axis, o / b: the box
  int C, c;
  int total;
};

__global__ __launch_bounds__(EIO_BLOCK) void eval3d_prob_kernel(ProbArgs a) {
  const unsigned e = blockIdx.x * EIO_BLOCK + threadIdx.x;
  if (e >= (unsigned)a.total) return;
  unsigned t = e;
  const int i0 = (int)(t % (unsigned)a.n[0]);
  t /= (unsigned)a.n[0];
  const int i1 = (int)(t % (unsigned)a.n[1]);
  const int i2 = (int)(t / (unsigned)a.n[1]);
  const int c0 = a.flip[0] ? a.n[0] - 1 - i0 : i0, c1 = a.flip[1] ? a.n[1] - 1 - i1 : i1, c2 = a.flip[2] ? a.n[2] - 1 - i2 : i2;
  uint8_t q = 0;
  if ((unsigned)(c0 - a.o[0]) < (unsigned)a.b[0] && (unsigned)(c1 - a.o[1]) < (unsigned)a.b[1] &&
      (unsigned)(c2 - a.o[2]) < (unsigned)a.b[2]) {
    const int vox = c0 * a.ds[0] + c1 * a.ds[1] + c2 * a.ds[2];
    const float w = a.wsum ? a.wsum[vox] : (float)a.cnt[vox];
    if (w > 0.f) {
      const float p = __fdiv_rn(a.acc[(size_t)vox * a.C + a.c], w);
      q = (uint8_t)fminf(fmaxf(rintf(255.0f * p), 0.0f), 255.0f);
    }
  }
  a.dst[e] = q;
}

static inline bool eio_fits(int a, int b, int c, int d = 1) {
  return a > 0 && b > 0 && c > 0 && d > 0 && (int64_t)a * b * c < ((int64_t)1 << 31) &&
         (int64_t)a * b * c * d < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int unetk_eval_slab(const int16_t* vol, int src_d, int src_h, int src_w, const int32_t* zsrc, int N, int C,
                               const int32_t* y0, const int32_t* y1, const float* fy, int H, const int32_t* x0,
                               const int32_t* x1, const float* fx, int W, const float* lut, int lut_n, int lo, int hi,
                               float* images, void* stream) {
  UNETK_REQUIRE(eio_fits(src_d, src_h, src_w) && eio_fits(H, W, C, N));
  UNETK_REQUIRE(hi >= lo && (int64_t)hi - lo + 1 <= (int64_t)lut_n && lo >= -32768 && hi <= 32767);
  UNETK_REQUIRE(vol && zsrc && y0 && y1 && fy && x0 && x1 && fx && lut && images && (((uintptr_t)images) & 3u) == 0);
  if (hi - lo + 1 > EIO_LUT_MAX) return UNETK_E_UNSUPPORTED;
  SlabArgs a;
  a.vol = vol; a.zsrc = zsrc; a.y0 = y0; a.y1 = y1; a.x0 = x0; a.x1 = x1; a.fy = fy; a.fx = fx; a.lut = lut; a.out = images;
  a.src_d = src_d; a.src_h = src_h; a.src_w = src_w; a.N = N; a.H = H; a.W = W; a.C = C; a.lo = lo; a.hi = hi;
  a.total = N * H * W * C;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(hi - lo + 1) * sizeof(float);
  const int per_block = EIO_BLOCK * EIO_ITERS;
  if (unetk_aligned16(images)) {
    const int groups = a.total / 4 + 1;                        // + 1: the thread that stores the elements past the last group
    UNETK_LAUNCH(eval_slab_kernel<4>, dim3((groups + per_block - 1) / per_block), dim3(EIO_BLOCK), lds, st, a);
  } else {
    UNETK_LAUNCH(eval_slab_kernel<1>, dim3((a.total + per_block - 1) / per_block), dim3(EIO_BLOCK), lds, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_zoom_nearest3d(const uint8_t* src, int d, int h, int w, const int32_t* tz, const int32_t* ty,
                                    const int32_t* tx, int D, int H, int W, uint8_t* dst, void* stream) {
  UNETK_REQUIRE(eio_fits(d, h, w) && eio_fits(D, H, W));
  UNETK_REQUIRE(src && tz && ty && tx && dst);
  ZoomArgs a;
  a.src = src; a.tz = tz; a.ty = ty; a.tx = tx; a.dst = dst;
  a.d = d; a.h = h; a.w = w; a.D = D; a.H = H; a.W = W;
  a.total = D * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (unetk_aligned16(dst)) {
    const int groups = a.total / 16 + 1;
    UNETK_LAUNCH(zoom_nearest3d_kernel<16>, dim3((groups + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  } else {
    UNETK_LAUNCH(zoom_nearest3d_kernel<1>, dim3((a.total + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_nii_compose(const uint8_t* liver, const uint8_t* tumor, int bd, int bh, int bw, int z1, int y1, int x1,
                                 int d, int h, int w, int t0, int t1, int t2, int flips, int16_t* dst, void* stream) {
  UNETK_REQUIRE((liver || tumor) && dst && (((uintptr_t)dst) & 1u) == 0);
  UNETK_REQUIRE(d > 0 && h > 0 && w > 0 && bd > 0 && bh > 0 && bw > 0);
  UNETK_REQUIRE(z1 >= 0 && y1 >= 0 && x1 >= 0 && (int64_t)z1 + bd <= d && (int64_t)y1 + bh <= h && (int64_t)x1 + bw <= w);
  const int tb[3] = {t0, t1, t2};
  unsigned seen = 0;
  for (int k = 0; k < 3; ++k) {
    UNETK_REQUIRE(tb[k] >= 0 && tb[k] <= 2);
    seen |= 1u << tb[k];
  }
  UNETK_REQUIRE(seen == 7u && (flips & ~7) == 0);
  if (!eio_fits(d, h, w)) return UNETK_E_UNSUPPORTED;
  // per data axis (z, y, x): length, box origin, box extent, mask stride, flip bit
  const int len[3] = {d, h, w}, org[3] = {z1, y1, x1}, ext[3] = {bd, bh, bw}, mst[3] = {bh * bw, bw, 1};
  const int fbit[3] = {(flips >> 2) & 1, (flips >> 1) & 1, flips & 1};
  NiiArgs a;
  a.liver = liver; a.tumor = tumor; a.dst = dst;
  for (int k = 0; k < 3; ++k) {
    a.n[k] = len[tb[k]]; a.flip[k] = fbit[tb[k]]; a.o[k] = org[tb[k]]; a.b[k] = ext[tb[k]]; a.ms[k] = mst[tb[k]];
  }
  a.total = d * h * w;
  hipStream_t st = (hipStream_t)stream;
  if (tb[0] != 2) {
    const int kx = tb[1] == 2 ? 1 : 2;
    const int tiles_x = (a.n[kx] + NII_TILE - 1) / NII_TILE;
    const dim3 grid((a.n[0] + NII_TILE - 1) / NII_TILE, tiles_x < 65535 ? tiles_x : 65535, a.n[3 - kx] < 65535 ? a.n[3 - kx] : 65535);
    if (kx == 1) {
      UNETK_LAUNCH(nii_compose_tr_kernel<1>, grid, dim3(EIO_BLOCK), 0, st, a);
    } else {
      UNETK_LAUNCH(nii_compose_tr_kernel<2>, grid, dim3(EIO_BLOCK), 0, st, a);
    }
  } else if (unetk_aligned16(dst)) {
    const int groups = a.total / 8 + 1;                        // + 1: the thread that stores the elements past the last group
    UNETK_LAUNCH(nii_compose_rows_kernel<8>, dim3((groups + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  } else {
    UNETK_LAUNCH(nii_compose_rows_kernel<1>, dim3(a.total / EIO_BLOCK + 1), dim3(EIO_BLOCK), 0, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

static inline bool eio_perm(const int tb[3]) {
  unsigned seen = 0;
  for (int k = 0; k < 3; ++k) {
    if (tb[k] < 0 || tb[k] > 2) return false;
    seen |= 1u << tb[k];
  }
  return seen == 7u;
}

extern "C" int unetk_nii_ingest(const void* src, int datatype, int n0, int n1, int n2, double scl_slope, double scl_inter, int t0,
                                int t1, int t2, int flips, int lo, int hi, int scale, uint16_t* dst, void* stream) {
  UNETK_REQUIRE(src && dst && (((uintptr_t)dst) & 1u) == 0);
  UNETK_REQUIRE(n0 > 0 && n1 > 0 && n2 > 0 && scale > 0 && lo <= hi && ((int64_t)hi - lo) * scale <= 65535);
  const int tb[3] = {t0, t1, t2};
  UNETK_REQUIRE(eio_perm(tb) && (flips & ~7) == 0);
  int item;                                                  // bytes per source element
  switch (datatype) {
    case 2: case 256: item = 1; break;
    case 4: case 512: item = 2; break;
    case 8: case 16: case 768: item = 4; break;
    case 64: item = 8; break;
    default: return UNETK_E_BADARG;
  }
  UNETK_REQUIRE((((uintptr_t)src) & (uintptr_t)(item - 1)) == 0);
  if (!eio_fits(n0, n1, n2)) return UNETK_E_UNSUPPORTED;
  const int nf[3] = {n0, n1, n2};
  int len[3] = {0, 0, 0};                                    // data axes (z, y, x)
  for (int k = 0; k < 3; ++k) len[tb[k]] = nf[k];
  const int dstr[3] = {len[1] * len[2], len[2], 1};
  const int fbit[3] = {(flips >> 2) & 1, (flips >> 1) & 1, flips & 1};
  IngestArgs a;
  a.src = src; a.dst = dst; a.slope = scl_slope; a.inter = scl_inter;
  for (int k = 0; k < 3; ++k) {
    a.n[k] = nf[k]; a.flip[k] = fbit[tb[k]]; a.ds[k] = dstr[tb[k]];
  }
  a.code = datatype; a.scaled = (scl_slope != 0.0 && scl_slope == scl_slope) ? 1 : 0;
  a.lo = lo; a.hi = hi; a.scale = scale;
  a.total = n0 * n1 * n2;
  hipStream_t st = (hipStream_t)stream;
  if (tb[0] != 2) {
    const int kx = tb[1] == 2 ? 1 : 2;
    const int tiles_x = (a.n[kx] + NII_TILE - 1) / NII_TILE;
    const dim3 grid((a.n[0] + NII_TILE - 1) / NII_TILE, tiles_x < 65535 ? tiles_x : 65535, a.n[3 - kx] < 65535 ? a.n[3 - kx] : 65535);
    if (kx == 1) {
      UNETK_LAUNCH(nii_ingest_tr_kernel<1>, grid, dim3(EIO_BLOCK), 0, st, a);
    } else {
      UNETK_LAUNCH(nii_ingest_tr_kernel<2>, grid, dim3(EIO_BLOCK), 0, st, a);
    }
  } else if (datatype == 4 && !a.scaled && unetk_aligned16(src)) {
    const int groups = a.total / 8 + 1;                        // + 1: the thread that stores the elements past the last group
    UNETK_LAUNCH(nii_ingest_rows_kernel<8>, dim3((groups + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, st, a);
  } else {
    UNETK_LAUNCH(nii_ingest_rows_kernel<1>, dim3(a.total / EIO_BLOCK + 1), dim3(EIO_BLOCK), 0, st, a);
  }
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}

extern "C" int unetk_eval3d_prob(const float* acc, int C, int c, int depth, int src_h, int src_w, const float* wsum,
                                 const int32_t* cnt, const int32_t box[6], int t0, int t1, int t2, int flips, uint8_t* dst,
                                 void* stream) {
  UNETK_REQUIRE(acc && box && dst && C >= 1 && C <= 8 && c >= 0 && c < C && depth > 0 && src_h > 0 && src_w > 0);
  UNETK_REQUIRE((wsum != nullptr) != (cnt != nullptr));                   // exactly one kind of weight
  UNETK_REQUIRE(((((uintptr_t)acc) | ((uintptr_t)wsum) | ((uintptr_t)cnt)) & 3u) == 0);
  UNETK_REQUIRE(0 <= box[0] && box[0] < box[1] && box[1] <= depth && 0 <= box[2] && box[2] < box[3] && box[3] <= src_h &&
                0 <= box[4] && box[4] < box[5] && box[5] <= src_w);
  const int tb[3] = {t0, t1, t2};
  UNETK_REQUIRE(eio_perm(tb) && (flips & ~7) == 0);
  if (!eio_fits(depth, src_h, src_w)) return UNETK_E_UNSUPPORTED;
  const int len[3] = {depth, src_h, src_w}, dstr[3] = {src_h * src_w, src_w, 1};
  const int org[3] = {box[0], box[2], box[4]}, ext[3] = {box[1] - box[0], box[3] - box[2], box[5] - box[4]};
  const int fbit[3] = {(flips >> 2) & 1, (flips >> 1) & 1, flips & 1};
  ProbArgs a;
  a.acc = acc; a.wsum = wsum; a.cnt = cnt; a.dst = dst; a.C = C; a.c = c;
  for (int k = 0; k < 3; ++k) {
    a.n[k] = len[tb[k]]; a.flip[k] = fbit[tb[k]]; a.ds[k] = dstr[tb[k]]; a.o[k] = org[tb[k]]; a.b[k] = ext[tb[k]];
  }
  a.total = depth * src_h * src_w;
  UNETK_LAUNCH(eval3d_prob_kernel, dim3((a.total + EIO_BLOCK - 1) / EIO_BLOCK), dim3(EIO_BLOCK), 0, (hipStream_t)stream, a);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
