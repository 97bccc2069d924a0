// draw.hip — skeletons blended into video frames on the device (dc_draw_people; the rule: include/deepcut_hip.h).  The host side
// (the primitive list, the tile bins) is draw.cpp.
//
// PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.
//
// Integer work on a few bytes per pixel.  One workgroup per non-empty tile, one thread per 2 x 2 pixel block (frame_tile.h: the
// ownership): a thread holds its bytes in registers from the first primitive to the last, so the drawing order is kept without atomics.
// The tile's primitives are workgroup-uniform: they go through LDS a chunk at a time.  Bytes no primitive covers are never stored.
#include <hip/hip_runtime.h>

#include "frame_tile.h"
#include "kernels.h"

namespace dc {

namespace {
template <int FMT>
__global__ __launch_bounds__(256) void draw_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                   const int* __restrict__ index, const DrawPrim* __restrict__ prims) {
  __shared__ DrawPrim sp[kDrawChunk];
  const DrawTile t = tiles[blockIdx.x];
  const DrawPlanes f = frames[t.frame];
  // a thread whose block lies outside the frame holds nothing and only helps staging
  BlockPixels<FMT> px(t.tx * kDrawTileW, t.ty * kDrawTileH, H, W);
  px.load(f);
  const int cx = 16 * px.x0 + 8, cy = 16 * px.y0 + 8;  // the centre of pixel 0
  for (int base = 0; base < t.count; base += kDrawChunk) {
    const int m = stage_chunk(sp, t, base, index, prims);
    if (!px.n_in) continue;
    draw_chunk(px, sp, m, cx, cy);
  }
  px.store(f);
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
