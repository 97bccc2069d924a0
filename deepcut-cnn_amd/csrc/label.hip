// label.hip — people's ids written into video frames on the device (dc_label_people; the rule: include/deepcut_hip.h).  The host side
// (the texts, the placement, the tile bins) is label.cpp; the form that bins for itself is in overlay.hip.
//
// PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing; the rule is this project's own.
//
// Integer work on a few bytes per pixel, held to bytes and not to a rate: labelled tiles are few.  One workgroup per non-empty tile, one
// thread per 2 x 2 pixel block (frame_tile.h: the ownership): a thread holds its bytes in registers from the first label to the last, so
// the order is kept without atomics.  The font (322 bytes) goes into LDS once per workgroup, the tile's labels a chunk at a time.  The
// divisions by the scale and by the advance are plain 32-bit ones.  Bytes no layer covers are never stored.
#include <hip/hip_runtime.h>

#include "label_tile.h"

namespace dc {

namespace {
template <int FMT>
__global__ __launch_bounds__(256) void label_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                    const int* __restrict__ index, const LabelPrim* __restrict__ prims) {
  __shared__ LabelPrim sp[kLabelChunk];
  __shared__ unsigned char font[kLabelFontBytes];
  const DrawTile t = tiles[blockIdx.x];
  const DrawPlanes f = frames[t.frame];
  label_stage_font(font);  // the first chunk's barriers follow
  BlockPixels<FMT> px(t.tx * kDrawTileW, t.ty * kDrawTileH, H, W);
  px.load(f);
  for (int base = 0; base < t.count; base += kLabelChunk) {
    const int m = min(kLabelChunk, t.count - base);
    __syncthreads();  // everybody is through with the chunk before
    if ((int)threadIdx.x < m) sp[threadIdx.x] = prims[index[t.first + base + (int)threadIdx.x]];
    __syncthreads();
    if (px.n_in) label_chunk(px, sp, m, font);  // a thread whose block lies outside the frame only helps staging
  }
  px.store(f);
}
}  // namespace

int launch_label(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                 const LabelPrim* prims, void* stream) {
  if (n_tiles <= 0) return 0;
  if (format != kFmtBgr && format != kFmtNv12) return (int)hipErrorInvalidValue;
  if (format == kFmtBgr)
    hipLaunchKernelGGL(label_kernel<kFmtBgr>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims);
  else
    hipLaunchKernelGGL(label_kernel<kFmtNv12>, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims);
  return (int)hipGetLastError();
}

}  // namespace dc
