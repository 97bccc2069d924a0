// frame_tile.h — what the kernels that write into video frames share (draw.hip, heat.hip, redact.hip): the 2 x 2 pixel blocks, the
// blend, the walk of a tile's primitives through LDS, the coverage test of the drawing rule (include/deepcut_hip.h, dc_draw_people).
// THE OWNERSHIP: a workgroup of 256 threads has one kDrawTileW x kDrawTileH pixel tile of one frame, a thread one 2 x 2 pixel block of
// it — the pixels q = 2 * row + column and, for NV12, the chroma sample they share.  So the owner of a chroma sample owns its luma
// pixels, nothing needs an atomic, and no two threads write one byte.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dc {

constexpr int kFmtBgr = 0, kFmtNv12 = 1;  // DC_PIX_BGR24, DC_PIX_NV12
constexpr int kBlocksX = kDrawTileW / 2, kBlocksY = kDrawTileH / 2;
static_assert(kBlocksX * kBlocksY == 256, "one thread per 2 x 2 block of the tile");
static_assert(kDrawChunk <= 256, "a chunk is staged by one pass of the workgroup");

__device__ __forceinline__ int frame_blend(int c, int dst, int a) { return (c * a + dst * (256 - a) + 128) >> 8; }

// The thread's block of the tile whose first pixel is (X0, Y0), in a frame of H x W pixels: (x0, y0) is pixel 0, in[q] whether pixel q
// lies in the frame.  -> n_in, how many do: a thread with none holds nothing
__device__ __forceinline__ int tile_block(int X0, int Y0, int H, int W, int& x0, int& y0, bool (&in)[4]) {
  x0 = X0 + 2 * ((int)threadIdx.x % kBlocksX), y0 = Y0 + 2 * ((int)threadIdx.x / kBlocksX);
  int n_in = 0;
  for (int q = 0; q < 4; ++q) in[q] = x0 + (q & 1) < W && y0 + (q >> 1) < H, n_in += in[q];
  return n_in;
}

// The block and its bytes in registers: NC per pixel (BGR24: B, G, R; NV12: Y) and the chroma sample.  colour: bytes as DrawPrim::colour
template <int FMT>
struct BlockPixels {
  static constexpr int NC = FMT == kFmtBgr ? 3 : 1;
  int x0, y0, n_in;
  bool in[4];
  int v[4][NC], cb = 0, cr = 0;
  unsigned touched = 0;  // bit q: pixel q, bit 4: the chroma sample
  unsigned char* chroma = nullptr;
  __device__ __forceinline__ BlockPixels(int X0, int Y0, int H, int W) { n_in = tile_block(X0, Y0, H, W, x0, y0, in); }
  __device__ __forceinline__ unsigned char* pixel(const DrawPlanes& f, int q) const {
    return f.plane0 + (long)(y0 + (q >> 1)) * f.pitch0 + (long)(x0 + (q & 1)) * NC;
  }
  __device__ __forceinline__ void load(const DrawPlanes& f) {
    for (int q = 0; q < 4; ++q) {
      const unsigned char* s = pixel(f, q);
      for (int c = 0; c < NC; ++c) v[q][c] = in[q] ? (int)s[c] : 0;
    }
    if (FMT == kFmtNv12 && n_in) {
      chroma = f.plane1 + (long)(y0 >> 1) * f.pitch1 + (long)(x0 >> 1) * 2;
      cb = chroma[0], cr = chroma[1];
    }
  }
  __device__ __forceinline__ void blend_pixel(int q, unsigned colour, int a) {
    v[q][0] = frame_blend(colour & 255, v[q][0], a);
    if (FMT == kFmtBgr) v[q][1] = frame_blend((colour >> 8) & 255, v[q][1], a), v[q][NC - 1] = frame_blend((colour >> 16) & 255, v[q][NC - 1], a);
    touched |= 1u << q;
  }
  __device__ __forceinline__ void blend_chroma(unsigned colour, int a) {
    cb = frame_blend((colour >> 8) & 255, cb, a), cr = frame_blend((colour >> 16) & 255, cr, a);
    touched |= 16u;
  }
  __device__ __forceinline__ void store(const DrawPlanes& f) const {  // bytes nothing was blended into are never stored
    for (int q = 0; q < 4; ++q)
      if (touched >> q & 1) {
        unsigned char* d = pixel(f, q);
        for (int c = 0; c < NC; ++c) d[c] = (unsigned char)v[q][c];
      }
    if (FMT == kFmtNv12 && (touched & 16u)) chroma[0] = (unsigned char)cb, chroma[1] = (unsigned char)cr;
  }
};

// One step of the walk of tile t's primitives: the chunk that starts at `base` goes into sp[kDrawChunk] (LDS) between two barriers, so
// every thread of the workgroup takes part, and every lane then reads the same address (a broadcast, no bank conflict).  -> its length
__device__ __forceinline__ int stage_chunk(DrawPrim* sp, const DrawTile& t, int base, const int* __restrict__ index,
                                           const DrawPrim* __restrict__ prims) {
  const int m = min(kDrawChunk, t.count - base);
  __syncthreads();  // everybody is through with the chunk before
  if ((int)threadIdx.x < m) sp[threadIdx.x] = prims[index[t.first + base + (int)threadIdx.x]];
  __syncthreads();
  return m;
}

// The coverage rule, in int64.  Coordinates are at most 2^19 units and a pixel centre at most 2^18, so w, v are below 2^20 and d below
// 2^20 + 1 per component: w.w, w.d and L = d.d stay below 2^42, |cross| below 2^42, and r16^2 L <= 2^20 * 2^41 = 2^61 for a capsule
// (r16 <= 1024).  |cross| >= 2^31 means cross^2 >= 2^62 > r16^2 L — outside —, so the square is formed only below 2^62: every product
// fits int64.  A disc may be larger (the redaction's head disc, r16 <= 2^14): its test forms r16^2 <= 2^28 alone.
__device__ __forceinline__ bool draw_covers(const DrawPrim& p, int px, int py) {
  const long long wx = px - p.ax, wy = py - p.ay, r2 = (long long)p.r16 * p.r16;
  if (wx * wx + wy * wy <= r2) return true;
  if (!p.capsule) return false;
  const long long vx = px - p.bx, vy = py - p.by;
  if (vx * vx + vy * vy <= r2) return true;
  const long long dx = p.bx - p.ax, dy = p.by - p.ay, L = dx * dx + dy * dy, dot = wx * dx + wy * dy;
  if (!(dot > 0 && dot < L)) return false;
  const long long cross = wx * dy - wy * dx;
  if (cross <= -(1LL << 31) || cross >= (1LL << 31)) return false;
  return cross * cross <= r2 * L;
}

// outside the box of the ends grown by the radius: outside the primitive (every covered point is within r16 of the segment).  (cx, cy) is
// the centre of the upper left pixel of a 2 x 2 block; false when any of the block's four centres may be covered
__device__ __forceinline__ bool draw_block_outside(const DrawPrim& p, int cx, int cy) {
  return cx + 16 < min(p.ax, p.bx) - p.r16 || cx > max(p.ax, p.bx) + p.r16 || cy + 16 < min(p.ay, p.by) - p.r16 ||
         cy > max(p.ay, p.by) + p.r16;
}

// ---- what a tile does with a chunk of primitives in LDS, shared by the kernels that are handed bins (draw.hip, redact.hip) and the
// ones that bin for themselves (overlay.hip) ---------------------------------------------------------------------------------------------

// The drawing rule on sp[0 .. m), in order, for the thread's block; (cx, cy) is the centre of pixel 0
template <int FMT>
__device__ __forceinline__ void draw_chunk(BlockPixels<FMT>& px, const DrawPrim* sp, int m, int cx, int cy) {
  for (int i = 0; i < m; ++i) {
    const DrawPrim p = sp[i];
    if (draw_block_outside(p, cx, cy)) continue;
    int k = 0;
    for (int q = 0; q < 4; ++q) {
      if (!px.in[q] || !draw_covers(p, cx + 16 * (q & 1), cy + 16 * (q >> 1))) continue;
      ++k;
      px.blend_pixel(q, p.colour, p.alpha);
    }
    // the chroma sample once per primitive, by the share of the block's in-frame pixels it covers
    if (FMT == kFmtNv12 && k) px.blend_chroma(p.colour, (p.alpha * k + px.n_in / 2) / px.n_in);
  }
}

// The redaction's phase 1 on sp[0 .. m): is the centre of one of the thread's in-frame pixels covered?  A set: `hit` only ever rises
__device__ __forceinline__ void redact_cover_chunk(bool& hit, const bool (&in)[4], const DrawPrim* sp, int m, int cx, int cy) {
  for (int i = 0; i < m && !hit; ++i) {
    const DrawPrim p = sp[i];
    if (draw_block_outside(p, cx, cy)) continue;
    for (int q = 0; q < 4; ++q) hit = hit || (in[q] && draw_covers(p, cx + 16 * (q & 1), cy + 16 * (q >> 1)));
  }
}

constexpr int kMaxRedactBlocks = kBlocksX * kBlocksY;  // B = 2: every thread a block of its own
static_assert(kMaxRedactBlocks == 256, "the flags and sums are cleared by one pass of the workgroup");
static_assert(kDrawTileW == 32 && kDrawTileH == 32, "the block sizes 2 .. 32 divide the tile");

// the thread's B x B block within the tile, B = 1 << bshift
__device__ __forceinline__ int redact_block_of(int x0, int y0, int bshift) {
  return ((y0 & (kDrawTileH - 1)) >> bshift) * (kDrawTileW >> bshift) + ((x0 & (kDrawTileW - 1)) >> bshift);
}

// The redaction's phases 2 and 3 behind phase 1: flag[kMaxRedactBlocks] and acc[3][kMaxRedactBlocks] (LDS) were cleared before a barrier
// that every thread has passed; EVERY thread of the workgroup calls this (it holds barriers).  (2) sums — the threads of flagged blocks
// add their in-frame bytes into the block's accumulators (integer adds: any order gives the same sum); (3) stores — the same threads
// write the rounded means (or the fill colour) to their own pixels and chroma sample.  fill: bytes as DrawPrim::colour
template <int FMT, int EFFECT>
__device__ __forceinline__ void redact_finish(const DrawPlanes& f, int H, int W, int x0, int y0, const bool (&in)[4], int n_in, int blk, bool hit,
                                              int bshift, unsigned fill, int* flag, int (*acc)[kMaxRedactBlocks]) {
  constexpr int NC = FMT == kFmtBgr ? 3 : 1;  // bytes per pixel of plane 0
  if (hit) flag[blk] = 1;  // every writer writes the same value
  __syncthreads();
  const bool mine = n_in && flag[blk];  // the thread has pixels in a selected block

  unsigned char* const d0 = f.plane0 + (long)y0 * f.pitch0 + (long)x0 * NC;  // pixel 0; dereferenced for in-frame pixels only
  unsigned char* const chroma = FMT == kFmtNv12 ? f.plane1 + (long)(y0 >> 1) * f.pitch1 + (long)(x0 >> 1) * 2 : nullptr;
  int out[3] = {(int)(fill & 255), (int)(fill >> 8 & 255), (int)(fill >> 16 & 255)};
  if (EFFECT == kRedactMosaic) {
    // ---- 2. sums: the thread's in-frame bytes, and its chroma sample, into the block's accumulators ----------------------------------
    if (mine) {
      int s[3] = {0, 0, 0};
      for (int q = 0; q < 4; ++q) {
        if (!in[q]) continue;
        const unsigned char* src = d0 + (long)(q >> 1) * f.pitch0 + (q & 1) * NC;
        for (int c = 0; c < NC; ++c) s[c] += (int)src[c];
      }
      if (FMT == kFmtNv12) s[1] = chroma[0], s[2] = chroma[1];
      for (int c = 0; c < 3; ++c) atomicAdd(&acc[c][blk], s[c]);
    }
    __syncthreads();
    if (mine) {
      // the block's in-frame pixels n and chroma samples m: it starts at an even pixel, so a partial row or column of samples counts
      const int B = 1 << bshift, bw = min(B, W - ((x0 >> bshift) << bshift)), bh = min(B, H - ((y0 >> bshift) << bshift));
      const int n = bw * bh, mc = ((bw + 1) >> 1) * ((bh + 1) >> 1);
      for (int c = 0; c < 3; ++c) {
        const int k = (FMT == kFmtNv12 && c > 0) ? mc : n;
        out[c] = (int)((unsigned)(acc[c][blk] + k / 2) / (unsigned)k);
      }
    }
  }
  // ---- 3. stores: the thread's own in-frame pixels and its own chroma sample ---------------------------------------------------------
  if (!mine) return;
  for (int q = 0; q < 4; ++q) {
    if (!in[q]) continue;
    unsigned char* d = d0 + (long)(q >> 1) * f.pitch0 + (q & 1) * NC;
    for (int c = 0; c < NC; ++c) d[c] = (unsigned char)out[c];
  }
  if (FMT == kFmtNv12) chroma[0] = (unsigned char)out[1], chroma[1] = (unsigned char)out[2];
}

}  // namespace dc
