// conv3x3 filter gradient with bf16 STORAGE (UNETK_BF16S): x and dy are bf16 in HBM, dW accumulates in fp32.
//   dW[tap][ci][co] = sum_pixels x[pixel + tap][ci] * dy[pixel][co]        (Conv2DBackpropFilter of
//   slim.conv2d(x, C, 3), NetworksV2/UNet.py:79,85,94, in the mixed-precision mode of BASELINE.json configs[2])
//
// GEMM view: M = ci, N = co, K = pixels, on v_mfma_f32_32x32x16_bf16.  Both operands are K-STRIDED in memory (NHWC:
// the 8 pixels a lane needs for its channel are 8 different rows), which the fp32-storage kernel paid for with 38
// ds_read_b32 + 19 conversions per 9 MFMAs (LDS-read bound at ~520 TFLOP/s).  Here the tiles stay bf16 in LDS exactly
// as they lie in HBM ([pixel][64 channels], 128-byte rows) and are read through the LDS TRANSPOSE path:
// ds_read_b64_tr_b16 hands each lane four consecutive pixels of ONE channel.
//   * per 16-pixel k-step a wave issues 2 transposed reads for its dy fragment and 3 per filter row for x (12 consecutive
//     halo pixels of its channel); the three kw taps of a filter row are the windows [kw, kw + 8) of those 12 values --
//     kw = 0 and kw = 2 are register sub-ranges, kw = 1 costs four v_alignbit.  11 reads per 9 MFMAs.
//   * tiles arrive by async direct-to-LDS loads (global_load_lds_dwordx4, 1 KiB per wave instruction) into a FOUR-stage
//     ring (160 KiB): a tile is ~1 us of MFMA work at the bf16 rate, less than one HBM round trip, so three tiles are
//     kept in flight (the fp32 kernel's two stages left this kernel latency-bound at 3.6 us per tile).  Every wave
//     issues exactly five pieces per tile (the 40th is a dummy), so "tile t has landed" is the constant s_waitcnt
//     vmcnt(10); past the end of its range a block re-fetches its last tile to keep that count.  The image is
//     lane-linear, so the bank swizzle is applied on the GLOBAL side: lane L of a piece fetches 16-byte chunk
//     (L & 7) ^ 4 * bit1(row) of its row.  With it any four consecutive rows x 32 channels (one transposed read of a
//     32-lane half) cover four distinct 64-byte bank groups: conflict-free for every tap shift.
//   * 512 threads = 2 (ci) x 2 (co) x 2 (pixel-row halves) waves own a 64 x 64 x 9-tap panel; split-K over pixel tiles
//     into slabs + the fixed-order slab reduction of conv_wgrad.hip => bit-reproducible, no atomics.
#include "common.h"

#include <stdlib.h>

namespace {

constexpr int TW = 16, TH = 8, HWD = TW + 2;
constexpr int HALO_PIX = (TH + 2) * HWD;          // 180
constexpr int CT = 64;                            // channels per panel side = one 128-byte LDS row
constexpr int NP_X = (HALO_PIX + 7) / 8;          // 23 one-KiB pieces (8 rows each) of the x halo
constexpr int NP_Y = TH * TW / 8;                 // 16 pieces of the dy tile
constexpr int NP = NP_X + NP_Y;                   // 39 (+ 1 dummy so that every wave issues IPW loads per tile)
constexpr int IPW = (NP + 7) / 8;                 // 5 pieces per wave
constexpr int NSTAGE = 4;
constexpr int XH_B = NP_X * 1024, STAGE_B = IPW * 8 * 1024;      // 40 KiB
constexpr int RED_B = 4 * 144 * 64 * 4;           // pixel-row-half reduction scratch: [4 waves][9 x 16][64 lanes] floats
constexpr int LDS_B = NSTAGE * STAGE_B > RED_B ? NSTAGE * STAGE_B : RED_B;
static_assert(LDS_B <= 160 * 1024, "LDS budget");

// 128 bytes of zeros in global memory: the source of out-of-image halo pixels for the direct-to-LDS loads (constant data;
// the fp32 kernel memsets a page of its workspace per call instead -- one more launch)
__device__ const uint32_t kZeroPage[32] = {};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// four consecutive rows (pixels) of one channel column: lane 4q + p of a 16-lane group addresses row q, channels 4p..4p+3
// of the group's 16; lane i receives channel i, row q in element q.
__device__ __forceinline__ uint2 tr_read(const char* base, int byte_off) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + byte_off));
  return __builtin_bit_cast(uint2, v);
}
__device__ __forceinline__ bf16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(bf16x8, make_uint4(a, b, c, d));
}

// PF: the first fragments of tile t + 1 are requested during tile t (two tiles of load flight); !PF: behind the barrier (three)
template <bool PF>
__global__ __launch_bounds__(512) void conv3x3_wgrad_bf16s_kernel(WgParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][STAGE_B]; reused as the reduction scratch
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave & 1, wci = (wave >> 1) & 1, ks = wave >> 2;
  const int l31 = lane & 31, h = lane >> 5;

  int bid = xcd_remap(blockIdx.x, gridDim.x);      // the panels of one pixel split run together on one XCD: its L2 serves
  const int co_t = bid % p.n_co_tiles; bid /= p.n_co_tiles;   // the x / dy tiles they share
  const int ci_t = bid % p.n_ci_tiles; bid /= p.n_ci_tiles;
  const int split = bid;
  const int ci0 = ci_t * CT, co0 = co_t * CT;
  const bf16_t* xb = reinterpret_cast<const bf16_t*>(p.x);
  const bf16_t* dyb = reinterpret_cast<const bf16_t*>(p.dy);

  // ---- staging: wave w issues pieces j = w + 8 i; lane = (row of the piece, 16-byte slot); the chunk it fetches is
  // the slot XOR-swizzled by bit 1 of the row (row = 8 j + (lane >> 3): bit 1 = lane bit 4)
  const int lrow = lane >> 3;
  const int lchunk = (lane & 7) ^ (((lane >> 4) & 1) << 2);
  int rel_h[IPW], rel_w[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int j = wave + 8 * i;
    if (j < NP_X) {
      const int pix = 8 * j + lrow;
      rel_h[i] = pix < HALO_PIX ? pix / HWD - 1 : (1 << 20);      // relative to the tile origin; 1 << 20 = dummy row
      rel_w[i] = pix % HWD - 1;
    } else if (j >= NP) {
      rel_h[i] = 1 << 20;                                          // the dummy 40th piece: zeros into the stage's spare KiB
      rel_w[i] = 0;
    } else {
      const int pix = 8 * (j - NP_X) + lrow;
      rel_h[i] = pix / TW;
      rel_w[i] = pix % TW;
    }
  }
  // Per lane and piece, the byte offset of its 16-byte chunk from the tile's origin pixel (h0, w0) -- constant over the tiles
  // (pieces that are not part of the tile -- rows past the halo, the 40th piece -- read the origin itself: their LDS
  // bytes are never used).  An INTERIOR tile (halo inside the image: all but the border tiles) then needs no per-lane
  // work at all: one scalar base per operand and the offset register.  Round 2 recomputed row / column / validity / a
  // 64-bit product per lane and piece for every tile: 3.5 vector instructions per MFMA (rocprofv3 SQ_INSTS_VALU), issued
  // by both waves of a SIMD at the same time, next to a matrix pipe that leaves the vector unit 24 of every 32 cycles.
  uint32_t poff[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int j = wave + 8 * i;
    const bool real = rel_h[i] < (1 << 19);
    const bool is_x = j < NP_X;
    const int64_t o = real ? ((int64_t)rel_h[i] * p.W + rel_w[i]) * (is_x ? p.xs : p.ys) + lchunk * 8 : 0;
    poff[i] = (uint32_t)(o * 2);        // wraps for the negative offsets of the halo's first row / column: added mod 2^32 to a
  }                                     // 32-bit origin offset below
  struct TileSrc {          // where a tile's pieces come from: wave-uniform, computed once per tile
    int h0, w0;
    int64_t ximg, yimg;
    bool interior;
    const char *xo, *yo;    // interior tiles: image bases + 32-bit origin offsets (fit 32 bits: checked on the host)
    uint32_t xorg, yorg;
  };
  auto locate = [&](int tile) {
    TileSrc ts;
    const int tw_i = tile % p.tiles_w;
    const int th_i = (tile / p.tiles_w) % p.tiles_h;
    const int n_tile = tile / (p.tiles_w * p.tiles_h);
    ts.h0 = th_i * TH; ts.w0 = tw_i * TW;
    ts.ximg = p.xa.off(n_tile); ts.yimg = p.ya.off(n_tile);
    ts.interior = ts.h0 >= 1 && ts.w0 >= 1 && ts.h0 + TH + 1 <= p.H && ts.w0 + TW + 1 <= p.W;
    ts.xo = reinterpret_cast<const char*>(xb + ts.ximg + ci0);
    ts.yo = reinterpret_cast<const char*>(dyb + ts.yimg + co0);
    ts.xorg = (uint32_t)((ts.h0 * p.W + ts.w0) * p.xs) * 2u;
    ts.yorg = (uint32_t)((ts.h0 * p.W + ts.w0) * p.ys) * 2u;
    return ts;
  };
  auto issue_pieces = [&](const TileSrc& ts, int stage, int mask) {
    if (ts.interior) {
#pragma unroll
      for (int i = 0; i < IPW; ++i) {
        if (!(mask & (1 << i))) continue;
        const int j = wave + 8 * i;
        const bool is_x = j < NP_X;
        const char* src = (is_x ? ts.xo : ts.yo) + (uint32_t)((is_x ? ts.xorg : ts.yorg) + poff[i]);
        char* dst = smem + stage * STAGE_B + j * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int j = wave + 8 * i;
      if (mask & (1 << i)) {
        const bool is_x = j < NP_X;
        const int gh = ts.h0 + rel_h[i], gw = ts.w0 + rel_w[i];
        const bool ok = gh >= 0 && gh < p.H && gw >= 0 && gw < p.W;
        const int64_t pixoff = (int64_t)gh * p.W + gw;
        const bf16_t* src = is_x ? xb + ts.ximg + pixoff * p.xs + ci0 + lchunk * 8 : dyb + ts.yimg + pixoff * p.ys + co0 + lchunk * 8;
        if (!ok) src = reinterpret_cast<const bf16_t*>(kZeroPage) + (lane & 7) * 8;
        char* dst = smem + stage * STAGE_B + j * 1024;   // wave-uniform; lanes land at dst + lane * 16 B
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    }
  };
  auto issue_tile = [&](int tile, int stage) { issue_pieces(locate(tile), stage, (1 << IPW) - 1); };

  // ---- fragment addressing.  16-lane group g = lane >> 4: channel 16-block (g & 1) of the wave's 32, pixel half h = g >> 1.
  const int i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3, g16 = (lane >> 4) & 1;
  const int chunk_a = 2 * (wci * 2 + g16) + (p4 >> 1), chunk_b = 2 * (wco * 2 + g16) + (p4 >> 1);
  // byte offset of this lane's 8 bytes inside its row, for rows with bit 1 == (q4 >> 1) ^ par
  const int a_off0 = q4 * 128 + ((chunk_a ^ (((q4 >> 1) ^ 0) << 2)) << 4) + 8 * (p4 & 1) + 8 * h * 128;
  const int a_off1 = q4 * 128 + ((chunk_a ^ (((q4 >> 1) ^ 1) << 2)) << 4) + 8 * (p4 & 1) + 8 * h * 128;
  const int b_off = q4 * 128 + ((chunk_b ^ ((q4 >> 1) << 2)) << 4) + 8 * (p4 & 1) + 8 * h * 128;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int t_begin = split * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.total_tiles);

  // prologue: three tiles in flight (indices clamped to the block's last tile: the ring then always holds IPW loads per
  // stage and "tile t + 1 has landed" is vmcnt(IPW))
  if (t_begin < t_end) {
#pragma unroll
    for (int k = 0; k < NSTAGE - 1; ++k) issue_tile(min(t_begin + k, t_end - 1), k);
  }
  // The main loop is hand-synchronised.  __syncthreads() carries a fence that waits for ALL outstanding memory operations
  // (vmcnt(0): the tiles in flight!), and the compiler guards every LDS read that follows a direct-to-LDS load with
  // another vmcnt(0) (it cannot tell the ring's stages apart) -- together they serialised loads and MFMAs (measured:
  // time = loads + compute).  So: a bare s_barrier after a counted vmcnt, and the transposed reads are inline asm with
  // counted lgkmcnt waits whose "+v" operands tie the consuming MFMAs behind them.
  //
  // Round 3 (what tools/mfma_mix_bf16.hip and the conv kernel's probe build showed about loops of this shape):
  //   * the barrier at the top of tile t now guarantees tile t + 1 (vmcnt(IPW): two tiles of flight instead of three, still
  //     4-5 us), so the FIRST fragments of tile t + 1 are requested during the last MFMAs of tile t: no wave sits behind the
  //     barrier waiting for LDS;
  //   * waves 0..3 request tile t + 3 behind the barrier, waves 4..7 (their SIMD partners: waves are dealt to the SIMDs
  //     cyclically) in the middle of the tile: five direct-to-LDS loads hold a wave at issue for several hundred cycles,
  //     and this way one partner requests while the other feeds the matrix pipe.
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
#define TR_READ(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define LGKM_WAIT3(n, r0, r1, r2) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(r0), "+v"(r1), "+v"(r2))
#define LGKM_WAIT5(n, r0, r1, r2, r3, r4) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4))
#define LO(v) ((uint32_t)(v))
#define HI(v) ((uint32_t)((v) >> 32))
  // MFMAs of one halo row hr (12 pixels of this lane's channel in a0 a1 a2) against the dy row rr_: filter row kh = hr - rr_
#ifdef UNETK_WG16_PROBE
  // timing probe (WRONG results): every 32x32x16 MFMA replaced by TWO 16x16x32 MFMAs on the same operand registers -- the same
  // matrix-pipe cycles, LDS traffic and register count -- to see what the MFMA shape alone does to this kernel's clock
  f32x4 accp[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) accp[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#define MF2(t_, A_, B_)                                                                                                    \
  accp[t_][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A_, B_, accp[t_][0], 0, 0, 0);                                     \
  accp[t_][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A_, B_, accp[t_][1], 0, 0, 0);
#define ROW_MFMA(kh_, a0, a1, a2, b0, b1)                                                                                  \
  {                                                                                                                        \
    const bf16x8 bb = frag(LO(b0), HI(b0), LO(b1), HI(b1));                                                                \
    MF2((kh_) * 3 + 0, frag(LO(a0), HI(a0), LO(a1), HI(a1)), bb)                                                           \
    MF2((kh_) * 3 + 1, frag(__builtin_amdgcn_alignbit(HI(a0), LO(a0), 16), __builtin_amdgcn_alignbit(LO(a1), HI(a0), 16),  \
                            __builtin_amdgcn_alignbit(HI(a1), LO(a1), 16), __builtin_amdgcn_alignbit(LO(a2), HI(a1), 16)), bb) \
    MF2((kh_) * 3 + 2, frag(HI(a0), LO(a1), HI(a1), LO(a2)), bb)                                                           \
  }
#else
#define ROW_MFMA(kh_, a0, a1, a2, b0, b1)                                                                                  \
  {                                                                                                                        \
    const bf16x8 bb = frag(LO(b0), HI(b0), LO(b1), HI(b1));                                                                \
    acc[(kh_) * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(LO(a0), HI(a0), LO(a1), HI(a1)), bb, acc[(kh_) * 3 + 0], 0, 0, 0); \
    acc[(kh_) * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                                                          \
        frag(__builtin_amdgcn_alignbit(HI(a0), LO(a0), 16), __builtin_amdgcn_alignbit(LO(a1), HI(a0), 16),                  \
             __builtin_amdgcn_alignbit(HI(a1), LO(a1), 16), __builtin_amdgcn_alignbit(LO(a2), HI(a1), 16)),                 \
        bb, acc[(kh_) * 3 + 1], 0, 0, 0);                                                                                  \
    acc[(kh_) * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(HI(a0), LO(a1), HI(a1), LO(a2)), bb, acc[(kh_) * 3 + 2], 0, 0, 0); \
  }
#endif
  constexpr int AROW = HWD * 128, BROW = TW * 128;     // bytes between consecutive halo rows / dy tile rows
  static_assert(IPW == 5 && NSTAGE == 4, "the wait counts below: vmcnt(IPW) = one younger tile in flight");
  uint64_t B00, B01, B10, B11, B20, B21, B30, B31;
  uint64_t P0, P1, P2, Q0, Q1, Q2;                     // halo rows, double-buffered: even rows in P, odd rows in Q
  const uint32_t a0_rel = ks * (TH / 2) * AROW + a_off0, a1_rel = ks * (TH / 2) * AROW + a_off1;
  const uint32_t b_rel = XH_B + ks * (TH / 2) * BROW + b_off;
  if (PF && t_begin < t_end) {
    asm volatile("s_waitcnt vmcnt(5)" ::: "memory");   // this wave's pieces of tiles 0 and 1 have landed ...
    __builtin_amdgcn_s_barrier();                      // ... everybody's
    // the first requests of tile 0: dy rows 0, 1 and halo row 0 -- the order the steady state leaves them in
    const uint32_t yb = lds0 + b_rel, xa0 = lds0 + a0_rel;
    TR_READ(B00, yb, 0 * BROW);            TR_READ(B01, yb, 0 * BROW + 512);
    TR_READ(B10, yb, 1 * BROW);            TR_READ(B11, yb, 1 * BROW + 512);
    TR_READ(P0, xa0, 0 * AROW);            TR_READ(P1, xa0, 0 * AROW + 512);   TR_READ(P2, xa0, 0 * AROW + 1024);
  }
  int stage = 0;
  for (int tile = t_begin; tile < t_end; ++tile, stage = (stage + 1) & (NSTAGE - 1)) {
    if constexpr (PF) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");  // this wave's pieces of tile + 1 have landed (tile + 2 may fly) ...
    else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");              // ... of this tile (two younger tiles may fly)
#ifdef UNETK_V3_PROBE
    if (!(p.dbg & 16))
#endif
    __builtin_amdgcn_s_barrier();                      // ... everybody's have, and every wave is done reading the stage of tile - 1
#ifdef UNETK_V3_PROBE
    const bool spread = p.dbg & 2048;      // one piece behind each of the first five MFMA groups instead of five in a row
    TileSrc ts_next;
    if (spread) ts_next = locate(min(tile + NSTAGE - 1, t_end - 1));
#define SPREAD_PIECE(i) if (spread) issue_pieces(ts_next, (stage + NSTAGE - 1) & (NSTAGE - 1), 1 << (i));
    if (!(p.dbg & (4 | 2048)))
#else
#define SPREAD_PIECE(i)
#endif
    if (wave < 4) issue_tile(min(tile + NSTAGE - 1, t_end - 1), (stage + NSTAGE - 1) & (NSTAGE - 1));

    // this wave's four tile rows r = 4 ks + rr read halo rows 4 ks + 0 .. 5 (parity of the swizzle = parity of the local
    // index, 4 ks being even) and dy rows 4 ks + 0 .. 3.  Halo row hr serves the pairs (rr, kh = hr - rr).
    const uint32_t xa0 = lds0 + stage * STAGE_B + a0_rel;   // even local halo rows
    const uint32_t xa1 = lds0 + stage * STAGE_B + a1_rel;   // odd
    const uint32_t yb = lds0 + stage * STAGE_B + b_rel;
    const int nstage = (stage + 1) & (NSTAGE - 1);
    const uint32_t nxa0 = lds0 + nstage * STAGE_B + a0_rel, nyb = lds0 + nstage * STAGE_B + b_rel;
    // outstanding (oldest first): B00 B01 B10 B11 P0 P1 P2 of this tile, requested during the previous one (PF) or here
    if constexpr (!PF) {
      TR_READ(B00, yb, 0 * BROW);            TR_READ(B01, yb, 0 * BROW + 512);
      TR_READ(B10, yb, 1 * BROW);            TR_READ(B11, yb, 1 * BROW + 512);
      TR_READ(P0, xa0, 0 * AROW);            TR_READ(P1, xa0, 0 * AROW + 512);   TR_READ(P2, xa0, 0 * AROW + 1024);
    }
    // hr = 0: prefetch row 1 and dy row 2
    TR_READ(Q0, xa1, 1 * AROW);            TR_READ(Q1, xa1, 1 * AROW + 512);   TR_READ(Q2, xa1, 1 * AROW + 1024);
    TR_READ(B20, yb, 2 * BROW);            TR_READ(B21, yb, 2 * BROW + 512);
    LGKM_WAIT5(5, P0, P1, P2, B00, B01);
    asm volatile("" : "+v"(B10), "+v"(B11));
    ROW_MFMA(0, P0, P1, P2, B00, B01);
    SPREAD_PIECE(0)
    // hr = 1 (in Q): prefetch row 2 -> P is free once the MFMAs above have read it (program order), dy row 3
    {
      uint64_t R0, R1, R2;
      TR_READ(R0, xa0, 2 * AROW);          TR_READ(R1, xa0, 2 * AROW + 512);   TR_READ(R2, xa0, 2 * AROW + 1024);
      TR_READ(B30, yb, 3 * BROW);          TR_READ(B31, yb, 3 * BROW + 512);
      LGKM_WAIT5(7, Q0, Q1, Q2, B10, B11);
      ROW_MFMA(0, Q0, Q1, Q2, B10, B11);
      ROW_MFMA(1, Q0, Q1, Q2, B00, B01);
      SPREAD_PIECE(1)
      // hr = 2 (in R): prefetch row 3 into Q
      TR_READ(Q0, xa1, 3 * AROW);          TR_READ(Q1, xa1, 3 * AROW + 512);   TR_READ(Q2, xa1, 3 * AROW + 1024);
      LGKM_WAIT5(5, R0, R1, R2, B20, B21);
      ROW_MFMA(0, R0, R1, R2, B20, B21);
      ROW_MFMA(1, R0, R1, R2, B10, B11);
      ROW_MFMA(2, R0, R1, R2, B00, B01);
    }
    SPREAD_PIECE(2)
#ifdef UNETK_V3_PROBE
    if (!(p.dbg & (4 | 2048)))
#endif
    if (wave >= 4) issue_tile(min(tile + NSTAGE - 1, t_end - 1), (stage + NSTAGE - 1) & (NSTAGE - 1));
    // hr = 3 (in Q): prefetch row 4 into P
    TR_READ(P0, xa0, 4 * AROW);            TR_READ(P1, xa0, 4 * AROW + 512);   TR_READ(P2, xa0, 4 * AROW + 1024);
    LGKM_WAIT5(3, Q0, Q1, Q2, B30, B31);
    ROW_MFMA(0, Q0, Q1, Q2, B30, B31);
    ROW_MFMA(1, Q0, Q1, Q2, B20, B21);
    ROW_MFMA(2, Q0, Q1, Q2, B10, B11);
    SPREAD_PIECE(3)
    // dy rows 0, 1 are done: request them for the NEXT tile (its stage became visible at this tile's barrier)
    if constexpr (PF) {
      asm volatile("s_nop 0" : "+v"(B00), "+v"(B01), "+v"(B10), "+v"(B11));      // orders the requests behind the MFMAs above
      TR_READ(B00, nyb, 0 * BROW);           TR_READ(B01, nyb, 0 * BROW + 512);
      TR_READ(B10, nyb, 1 * BROW);           TR_READ(B11, nyb, 1 * BROW + 512);
    }
    // hr = 4 (in P): prefetch row 5 into Q
    TR_READ(Q0, xa1, 5 * AROW);            TR_READ(Q1, xa1, 5 * AROW + 512);   TR_READ(Q2, xa1, 5 * AROW + 1024);
    if constexpr (PF) LGKM_WAIT3(7, P0, P1, P2);
    else LGKM_WAIT3(3, P0, P1, P2);
    ROW_MFMA(1, P0, P1, P2, B30, B31);
    ROW_MFMA(2, P0, P1, P2, B20, B21);
    SPREAD_PIECE(4)
    if constexpr (PF) {      // halo row 0 of the next tile
      asm volatile("s_nop 0" : "+v"(P0), "+v"(P1), "+v"(P2));
      TR_READ(P0, nxa0, 0 * AROW);           TR_READ(P1, nxa0, 0 * AROW + 512);  TR_READ(P2, nxa0, 0 * AROW + 1024);
      LGKM_WAIT3(3, Q0, Q1, Q2);
    } else {
      LGKM_WAIT3(0, Q0, Q1, Q2);
    }
    // hr = 5 (in Q)
    ROW_MFMA(2, Q0, Q1, Q2, B30, B31);
  }
#undef SPREAD_PIECE
#undef TR_READ
#undef LGKM_WAIT3
#undef LGKM_WAIT5
#undef ROW_MFMA
#undef LO
#undef HI

#ifdef UNETK_WG16_PROBE
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][4 * j + r] += accp[t][j][r];
#undef MF2
#endif
  // ---- sum the two pixel-row halves through LDS (fixed order), then the ks == 0 waves write the split's slab
  float* red = reinterpret_cast<float*>(smem);  // [4 waves][144][64 lanes]
  const int pidx = wci * 2 + wco;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the clamped re-fetches and the fragment requests behind the last tile
  __syncthreads();
#ifdef UNETK_V3_PROBE
  if (p.dbg & 32) { if (acc[0][0] == 12345.f) p.slab[0] = 1.f; return; }
#endif
  if (ks == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(pidx * 144 + t * 16 + r) * 64 + lane] = acc[t][r];
  }
  __syncthreads();
  if (ks == 0) {
    float* out = p.slab + (int64_t)split * 9 * p.Cin * p.Cout;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + wci * 32 + mfma32_row(r, h);
        out[((int64_t)t * p.Cin + ci) * p.Cout + co0 + wco * 32 + l31] = acc[t][r] + red[(pidx * 144 + t * 16 + r) * 64 + lane];
      }
  }
}

// First layer (9 * Cin <= 32 rows, Cout = 64; Encode1/conv1): x is the fp32 image, dy is bf16.  HBM-bound on reading dy
// once; same MFMA contraction as conv3x3_wgrad_c3_kernel (conv_wgrad.hip) with dy widened to fp32 on its way into LDS.
__global__ __launch_bounds__(256) void conv3x3_wgrad_c3_bf16s_kernel(WgParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dyt = reinterpret_cast<float*>(smem);          // [128 pixels][64]
  float* xh = dyt + TH * TW * CT;                        // [180 pixels][4]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int khalf = wave >> 1, wco = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;
  const int cin = p.Cin, m_rows = 9 * cin;
  const int split = blockIdx.x;
  const bool a_on = l31 < m_rows;
  const int a_tap = a_on ? l31 / cin : 0, a_ci = a_on ? l31 % cin : 0;
  const int a_off = ((a_tap / 3) * HWD + (a_tap % 3)) * 4 + a_ci;
  const bf16_t* dyb = reinterpret_cast<const bf16_t*>(p.dy);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int t_begin = split * p.tiles_per_split;
  const int t_end = min(t_begin + p.tiles_per_split, p.total_tiles);
  // The next tile waits in registers while this one is contracted (round 3: the loop was load -> barrier -> MFMAs -> barrier
  // with nothing in flight during the MFMAs, 1.3 TB/s of dy): 8 x (pixel, channel quad) of dy and 3 halo values per thread
  constexpr int NDY = TH * TW * (CT / 4) / 256, NXH = (HALO_PIX * 4 + 255) / 256;
  uint2 dyr[NDY];
  float xr[NXH];
  auto fetch = [&](int tile) {
    const int tw_i = tile % p.tiles_w;
    const int th_i = (tile / p.tiles_w) % p.tiles_h;
    const int n_img = tile / (p.tiles_w * p.tiles_h);
    const int h0 = th_i * TH, w0 = tw_i * TW;
    const int64_t ximg = p.xa.off(n_img), yimg = p.ya.off(n_img);
#pragma unroll
    for (int i = 0; i < NDY; ++i) {
      const int idx = tid + i * 256;
      const int pix = idx >> 4, cq = idx & 15;
      const int gh = h0 + (pix >> 4), gw = w0 + (pix & 15);
      dyr[i] = make_uint2(0u, 0u);
      if (gh < p.H && gw < p.W) dyr[i] = *reinterpret_cast<const uint2*>(dyb + yimg + ((int64_t)gh * p.W + gw) * p.ys + cq * 4);
    }
#pragma unroll
    for (int i = 0; i < NXH; ++i) {
      const int idx = tid + i * 256;
      const int pix = idx >> 2, c = idx & 3;
      const int gh = h0 - 1 + pix / HWD, gw = w0 - 1 + pix % HWD;
      xr[i] = 0.f;
      if (idx < HALO_PIX * 4 && c < cin && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W)
        xr[i] = p.x[ximg + ((int64_t)gh * p.W + gw) * p.xs + c];
    }
  };
  if (t_begin < t_end) fetch(t_begin);
  for (int tile = t_begin; tile < t_end; ++tile) {
    __syncthreads();   // previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < NDY; ++i) {
      const int idx = tid + i * 256;
      const float4 v = make_float4(unetk_bf16_lo(dyr[i].x), unetk_bf16_hi(dyr[i].x), unetk_bf16_lo(dyr[i].y), unetk_bf16_hi(dyr[i].y));
      *reinterpret_cast<float4*>(&dyt[(idx >> 4) * CT + (idx & 15) * 4]) = v;
    }
#pragma unroll
    for (int i = 0; i < NXH; ++i) {
      const int idx = tid + i * 256;
      if (idx < HALO_PIX * 4) xh[idx] = xr[i];
    }
    __syncthreads();
    if (tile + 1 < t_end) fetch(tile + 1);
#pragma unroll
    for (int rr = 0; rr < TH / 2; ++rr) {
      const int r = khalf * (TH / 2) + rr;
#pragma unroll
      for (int c2 = 0; c2 < TW / 2; ++c2) {
        const int col = 2 * c2 + h;
        const float b = dyt[(r * TW + col) * CT + wco * 32 + l31];
        float a = xh[(r * HWD + col) * 4 + a_off];
        a = a_on ? a : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);   // [2][16][64]
  if (khalf == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wco * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (khalf == 0) {
    float* out = p.slab + (int64_t)split * m_rows * p.Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = mfma32_row(r, h);
      if (i < m_rows) out[(int64_t)i * p.Cout + wco * 32 + l31] = acc[r] + red[(wco * 16 + r) * 64 + lane];
    }
  }
}

}  // namespace

bool unetk_wgrad_plan_bf16s(const WgShape& s, WgPlan& pl, int* want) {
  if (s.Cin % CT == 0 && s.Cout % CT == 0) {
    pl.family = WG_BF16S;
    pl.n_ci_tiles = s.Cin / CT;
    pl.n_co_tiles = s.Cout / CT;
    const int panels = pl.n_ci_tiles * pl.n_co_tiles;
    // ONE round of blocks: 256 CUs x one 512-thread block (160 KB of LDS) -- all blocks do equal work, and every extra
    // split costs a 9 x Cin x Cout slab written and read again (with >= 256 panels there is no split and no reduction)
    *want = panels >= 256 ? 1 : (256 + panels - 1) / panels;
  } else if (9 * s.Cin <= 32 && s.Cout == CT) {
    pl.family = WG_BF16S_C3;
    pl.n_ci_tiles = pl.n_co_tiles = 1;
    *want = 1024;     // = the resident blocks (four per CU): measured 2048 / 1024 / 512 splits -> 0.163 / 0.146 / 0.155 ms
  } else {
    return false;
  }
  return true;
}

int unetk_wgrad_launch_bf16s(const WgPlan& pl, const WgParams& p, hipStream_t st) {
  if (pl.family == WG_BF16S_C3) {
    const size_t lds3 = (size_t)(TH * TW * CT + HALO_PIX * 4) * sizeof(float);
    UNETK_LAUNCH(conv3x3_wgrad_c3_bf16s_kernel, dim3(pl.grid), dim3(256), lds3, st, p);
    UNETK_LAUNCH_CHECK();
    return UNETK_OK;
  }
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)conv3x3_wgrad_bf16s_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_B);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)conv3x3_wgrad_bf16s_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_B);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  // UNETK_WGRAD_DEEP=1 (measurement): three tiles of load flight, first fragments behind the barrier
  static const int deep = unetk_env_int("UNETK_WGRAD_DEEP", 0);
  if (deep) UNETK_LAUNCH(conv3x3_wgrad_bf16s_kernel<false>, dim3(pl.grid), dim3(512), LDS_B, st, p);
  else UNETK_LAUNCH(conv3x3_wgrad_bf16s_kernel<true>, dim3(pl.grid), dim3(512), LDS_B, st, p);
  UNETK_LAUNCH_CHECK();
  return UNETK_OK;
}
