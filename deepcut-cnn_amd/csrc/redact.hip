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
constexpr int kMaxRedactBlocks = kBlocksX * kBlocksY;  // B = 2: every thread a block of its own
static_assert(kMaxRedactBlocks == 256, "the flags and sums are cleared by one pass of the workgroup");
static_assert(kDrawTileW == 32 && kDrawTileH == 32, "the block sizes 2 .. 32 divide the tile");

// bshift = log2(B), 1 .. 5; fill: bytes as DrawPrim::colour (EFFECT == kRedactFill)
template <int FMT, int EFFECT>
__global__ __launch_bounds__(256) void redact_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                     const int* __restrict__ index, const DrawPrim* __restrict__ prims, int bshift,
                                                     unsigned fill) {
  constexpr int NC = FMT == kFmtBgr ? 3 : 1;  // bytes per pixel of plane 0
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
  const int blk = ((y0 & (kDrawTileH - 1)) >> bshift) * (kDrawTileW >> bshift) + ((x0 & (kDrawTileW - 1)) >> bshift);
  flag[threadIdx.x] = 0;
  for (int c = 0; c < 3; ++c) acc[c][threadIdx.x] = 0;

  // ---- 1. coverage: is the centre of one of the thread's in-frame pixels covered by a primitive of the tile? ---------------------------
  const int cx = 16 * x0 + 8, cy = 16 * y0 + 8;  // the centre of pixel 0
  bool hit = false;
  for (int base = 0; base < t.count; base += kDrawChunk) {
    const int m = stage_chunk(sp, t, base, index, prims);  // its barriers: on the first trip the flags and sums are cleared
    if (!n_in || hit) continue;  // nothing left to find out, but the staging still needs this thread
    for (int i = 0; i < m && !hit; ++i) {
      const DrawPrim p = sp[i];
      if (draw_block_outside(p, cx, cy)) continue;
      for (int q = 0; q < 4; ++q) hit = hit || (in[q] && draw_covers(p, cx + 16 * (q & 1), cy + 16 * (q >> 1)));
    }
  }
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
