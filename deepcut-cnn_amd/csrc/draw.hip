// draw.hip — skeletons blended into video frames on the device (dc_draw_people; the rule: include/deepcut_hip.h).  The host side
// (the primitive list, the tile bins) is draw.cpp.
//
// PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.
//
// Integer work on a few bytes per pixel.  One workgroup per non-empty tile, one thread per 2 x 2 pixel block: a thread holds its four
// pixels (and, for NV12, the one chroma sample they share) in registers from the first primitive to the last, so the drawing order
// is kept without atomics and no two threads write one byte.  The tile's primitives are workgroup-uniform: a chunk of them is staged
// into LDS and every lane reads the same address (a broadcast, no bank conflict).  Bytes no primitive covers are never stored.
#include <hip/hip_runtime.h>

#include "draw_cover.h"
#include "kernels.h"

namespace dc {

namespace {
constexpr int kFmtBgr = 0, kFmtNv12 = 1;  // DC_PIX_BGR24, DC_PIX_NV12
constexpr int kBlocksX = kDrawTileW / 2, kBlocksY = kDrawTileH / 2;
static_assert(kBlocksX * kBlocksY == 256, "one thread per 2 x 2 block of the tile");
static_assert(kDrawChunk <= 256, "a chunk is staged by one pass of the workgroup");

__device__ __forceinline__ int draw_blend(int c, int dst, int a) { return (c * a + dst * (256 - a) + 128) >> 8; }

template <int FMT>
__global__ __launch_bounds__(256) void draw_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                   const int* __restrict__ index, const DrawPrim* __restrict__ prims) {
  constexpr int NC = FMT == kFmtBgr ? 3 : 1;  // bytes held per pixel
  __shared__ DrawPrim sp[kDrawChunk];
  const DrawTile t = tiles[blockIdx.x];
  const DrawPlanes f = frames[t.frame];
  const int x0 = t.tx * kDrawTileW + 2 * ((int)threadIdx.x % kBlocksX), y0 = t.ty * kDrawTileH + 2 * ((int)threadIdx.x / kBlocksX);
  // the block's pixels q = 2 * row + column; a thread whose block lies outside the frame holds nothing and only helps staging
  bool in[4];
  int n_in = 0;
  for (int q = 0; q < 4; ++q) in[q] = x0 + (q & 1) < W && y0 + (q >> 1) < H, n_in += in[q];
  int v[4][NC], cb = 0, cr = 0;
  unsigned touched = 0;  // bit q: pixel q, bit 4: the chroma sample
  for (int q = 0; q < 4; ++q) {
    const unsigned char* s = f.plane0 + (long)(y0 + (q >> 1)) * f.pitch0 + (long)(x0 + (q & 1)) * NC;
    for (int c = 0; c < NC; ++c) v[q][c] = in[q] ? (int)s[c] : 0;
  }
  unsigned char* chroma = nullptr;
  if (FMT == kFmtNv12 && n_in) {
    chroma = f.plane1 + (long)(y0 >> 1) * f.pitch1 + (long)(x0 >> 1) * 2;
    cb = chroma[0], cr = chroma[1];
  }
  const int cx = 16 * x0 + 8, cy = 16 * y0 + 8;  // the centre of pixel 0
  for (int base = 0; base < t.count; base += kDrawChunk) {
    const int m = min(kDrawChunk, t.count - base);
    __syncthreads();  // everybody is through with the chunk before
    if ((int)threadIdx.x < m) sp[threadIdx.x] = prims[index[t.first + base + (int)threadIdx.x]];
    __syncthreads();
    if (!n_in) continue;
    for (int i = 0; i < m; ++i) {
      const DrawPrim p = sp[i];
      if (draw_block_outside(p, cx, cy)) continue;
      const int c0 = p.colour & 255, c1 = (p.colour >> 8) & 255, c2 = (p.colour >> 16) & 255;
      int k = 0;
      for (int q = 0; q < 4; ++q) {
        if (!in[q] || !draw_covers(p, cx + 16 * (q & 1), cy + 16 * (q >> 1))) continue;
        ++k;
        touched |= 1u << q;
        v[q][0] = draw_blend(c0, v[q][0], p.alpha);
        if (FMT == kFmtBgr) v[q][1] = draw_blend(c1, v[q][1], p.alpha), v[q][NC - 1] = draw_blend(c2, v[q][NC - 1], p.alpha);
      }
      if (FMT == kFmtNv12 && k) {  // the chroma sample once per primitive, by the share of the block's in-frame pixels it covers
        const int ac = (p.alpha * k + n_in / 2) / n_in;
        cb = draw_blend(c1, cb, ac), cr = draw_blend(c2, cr, ac);
        touched |= 16u;
      }
    }
  }
  for (int q = 0; q < 4; ++q)
    if (touched >> q & 1) {
      unsigned char* d = f.plane0 + (long)(y0 + (q >> 1)) * f.pitch0 + (long)(x0 + (q & 1)) * NC;
      for (int c = 0; c < NC; ++c) d[c] = (unsigned char)v[q][c];
    }
  if (FMT == kFmtNv12 && (touched & 16u)) chroma[0] = (unsigned char)cb, chroma[1] = (unsigned char)cr;
}
}  // namespace

int launch_draw(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                const DrawPrim* prims, void* stream) {
  if (n_tiles <= 0) return 0;
  if (format != kFmtBgr && format != kFmtNv12) return (int)hipErrorInvalidValue;
  if (format == kFmtBgr)
    hipLaunchKernelGGL(draw_kernel<kFmtBgr>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims);
  else
    hipLaunchKernelGGL(draw_kernel<kFmtNv12>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims);
  return (int)hipGetLastError();
}

}  // namespace dc
