// redact.hip — people redacted in video frames on the device: a mosaic or a solid colour over the B x B pixel blocks that regions derived
// from people's joints reach (dc_redact_people; the rule: include/deepcut_hip.h).  The host side (the primitives, the tile bins) is
// redact.cpp.
//
// PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own.
//
// One workgroup per non-empty tile, one thread per 2 x 2 pixel block (frame_tile.h: the ownership), so the owner of a chroma sample owns
// its luma pixels.  B is even and divides the tile: a thread's four pixels lie in ONE block, a block in ONE tile.  Three phases between
// barriers: (1) coverage — the tile's primitives go through LDS a chunk at a time, a thread that finds one of its pixel centres covered
// raises its block's flag; (2) sums — the threads of flagged blocks add their in-frame bytes into the block's LDS accumulators (integer
// adds: any order gives the same sum); (3) stores — the same threads write the rounded means (or the fill colour) to their own pixels
// and chroma sample.  Nobody else stores anything, and every byte is read before the barrier that precedes its store.
#include <hip/hip_runtime.h>

#include "frame_tile.h"
#include "kernels.h"

namespace dc {

namespace {
// bshift = log2(B), 1 .. 5; fill: bytes as DrawPrim::colour (EFFECT == kRedactFill)
template <int FMT, int EFFECT>
__global__ __launch_bounds__(256) void redact_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                     const int* __restrict__ index, const DrawPrim* __restrict__ prims, int bshift,
                                                     unsigned fill) {
  __shared__ DrawPrim sp[kDrawChunk];
  __shared__ int flag[kMaxRedactBlocks];
  __shared__ int acc[3][kMaxRedactBlocks];  // BGR24: B, G, R; NV12: Y, Cb, Cr
  const DrawTile t = tiles[blockIdx.x];
  const DrawPlanes f = frames[t.frame];
  // the thread's pixels; a thread whose pixels lie outside the frame only helps staging
  int x0, y0;
  bool in[4];
  const int n_in = tile_block(t.tx * kDrawTileW, t.ty * kDrawTileH, H, W, x0, y0, in);
  // the thread's B x B block within the tile
  const int blk = redact_block_of(x0, y0, bshift);
  flag[threadIdx.x] = 0;
  for (int c = 0; c < 3; ++c) acc[c][threadIdx.x] = 0;

  // ---- 1. coverage: is the centre of one of the thread's in-frame pixels covered by a primitive of the tile? ---------------------------
  const int cx = 16 * x0 + 8, cy = 16 * y0 + 8;  // the centre of pixel 0
  bool hit = false;
  for (int base = 0; base < t.count; base += kDrawChunk) {
    const int m = stage_chunk(sp, t, base, index, prims);  // its barriers: on the first trip the flags and sums are cleared
    if (!n_in || hit) continue;  // nothing left to find out, but the staging still needs this thread
    redact_cover_chunk(hit, in, sp, m, cx, cy);
  }
  // ---- 2. sums, 3. stores (frame_tile.h) ---------------------------------------------------------------------------------------------
  redact_finish<FMT, EFFECT>(f, H, W, x0, y0, in, n_in, blk, hit, bshift, fill, flag, acc);
}

template <int FMT>
int launch_effect(int effect, int bshift, unsigned fill, const DrawPlanes* frames, int H, int W, const DrawTile* tiles, int n_tiles,
                  const int* index, const DrawPrim* prims, hipStream_t s) {
  if (effect == kRedactMosaic)
    hipLaunchKernelGGL((redact_kernel<FMT, kRedactMosaic>), dim3(n_tiles), dim3(256), 0, s, frames, H, W, tiles, index, prims, bshift, fill);
  else
    hipLaunchKernelGGL((redact_kernel<FMT, kRedactFill>), dim3(n_tiles), dim3(256), 0, s, frames, H, W, tiles, index, prims, bshift, fill);
  return (int)hipGetLastError();
}
}  // namespace

int launch_redact(int format, int effect, int block, unsigned fill, const DrawPlanes* frames, int height, int width, const DrawTile* tiles,
                  int n_tiles, const int* index, const DrawPrim* prims, void* stream) {
  if (n_tiles <= 0) return 0;
  int bshift = 0;
  while (bshift < 6 && (1 << bshift) != block) ++bshift;
  if ((format != kFmtBgr && format != kFmtNv12) || (effect != kRedactMosaic && effect != kRedactFill) || bshift < 1 || bshift > 5)
    return (int)hipErrorInvalidValue;
  return format == kFmtBgr ? launch_effect<kFmtBgr>(effect, bshift, fill, frames, height, width, tiles, n_tiles, index, prims, (hipStream_t)stream)
                           : launch_effect<kFmtNv12>(effect, bshift, fill, frames, height, width, tiles, n_tiles, index, prims, (hipStream_t)stream);
}

}  // namespace dc
