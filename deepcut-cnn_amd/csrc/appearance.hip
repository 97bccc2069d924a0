// appearance.hip — appearance descriptors of people, counted from video frames on the device: per person and channel, a 16-bin histogram
// of the bytes of the pixels under the capsules of the person's sampled limbs (dc_describe_people; the rule: include/deepcut_hip.h).  The
// host side (the primitives, the tile bins) is appearance.cpp.
//
// PARITY UNPINNED BY THE REFERENCE, which stops at the maps; the rule is this project's own.
//
// One workgroup per non-empty tile, one thread per 2 x 2 pixel block (frame_tile.h: the ownership), so the thread that holds a chroma
// sample holds its luma pixels.  A thread loads its bytes once and walks the tile's primitives a chunk at a time through LDS, keeping a
// 4-bit hit mask for the person at hand.  The host bins the primitives in person order, so a tile's run of one person is contiguous and
// every thread meets the change of person at the same primitive: the branch is uniform and may hold barriers.  There, and at the end,
// the threads add their hit pixels into a 48-bin LDS histogram, and 48 threads add its non-zero bins to desc with integer atomics that
// return nothing.  Integer sums commute: the result does not depend on the order of tiles, threads or primitives.  No frame byte is stored.
#include <hip/hip_runtime.h>

#include "frame_tile.h"
#include "kernels.h"

namespace dc {

namespace {
static_assert(kAppearDesc <= 256, "one pass of the workgroup clears and flushes the histogram");

// `hits` pixels of bin `bin` of channel c; the caller merges equal neighbours, so a block of one colour costs one LDS atomic per channel
__device__ __forceinline__ void appear_count(int* hist, int c, int bin, int hits) { atomicAdd(&hist[c * kAppearBins + bin], hits); }

// The person at hand is complete within this tile: the threads' hit pixels go into hist[kAppearDesc] (LDS, all zeros on entry), then its
// non-zero bins into the person's descriptor, and hist is zeros again.  EVERY thread of the workgroup calls this (it holds barriers).
// v[q][c]: the three bytes of pixel q; mask: bit q = the person's region holds pixel q
__device__ __forceinline__ void appear_flush(int* hist, int* __restrict__ person_desc, const int (&v)[4][3], unsigned mask) {
  if (mask) {
    for (int c = 0; c < 3; ++c) {
      int bin = -1, hits = 0;  // a run of equal bins
      for (int q = 0; q < 4; ++q) {
        if (!(mask >> q & 1)) continue;
        const int b = v[q][c] >> 4;
        if (b != bin && hits) appear_count(hist, c, bin, hits), hits = 0;
        bin = b, ++hits;
      }
      appear_count(hist, c, bin, hits);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < kAppearDesc) {
    const int n = hist[threadIdx.x];
    if (n) atomicAdd(&person_desc[threadIdx.x], n), hist[threadIdx.x] = 0;
  }
  __syncthreads();
}

template <int FMT>
__global__ __launch_bounds__(256) void describe_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawTile* __restrict__ tiles,
                                                       const int* __restrict__ index, const DrawPrim* __restrict__ prims, int P,
                                                       int* __restrict__ desc) {
  __shared__ DrawPrim sp[kDrawChunk];
  __shared__ int hist[kAppearDesc];
  const DrawTile t = tiles[blockIdx.x];
  const DrawPlanes f = frames[t.frame];
  // the thread's pixels; a thread whose pixels lie outside the frame only helps staging and flushing
  int x0, y0;
  bool in[4];
  const int n_in = tile_block(t.tx * kDrawTileW, t.ty * kDrawTileH, H, W, x0, y0, in);
  if ((int)threadIdx.x < kAppearDesc) hist[threadIdx.x] = 0;  // the first stage_chunk's barriers stand between this and the first add

  // ---- the thread's bytes, loaded once: BGR24 B, G, R; NV12 Y of the pixel, Cb and Cr of the block's sample ------------------------------
  constexpr int NC = FMT == kFmtBgr ? 3 : 1;
  int v[4][3] = {};
  if (n_in) {
    int cb = 0, cr = 0;
    if (FMT == kFmtNv12) {
      const unsigned char* chroma = f.plane1 + (long)(y0 >> 1) * f.pitch1 + (long)(x0 >> 1) * 2;
      cb = chroma[0], cr = chroma[1];
    }
    for (int q = 0; q < 4; ++q) {
      if (!in[q]) continue;
      const unsigned char* s = f.plane0 + (long)(y0 + (q >> 1)) * f.pitch0 + (long)(x0 + (q & 1)) * NC;
      v[q][0] = s[0];
      v[q][1] = FMT == kFmtBgr ? (int)s[NC - 2] : cb;
      v[q][2] = FMT == kFmtBgr ? (int)s[NC - 1] : cr;
    }
  }
  unsigned all = 0;  // the thread's in-frame pixels
  for (int q = 0; q < 4; ++q) all |= (unsigned)in[q] << q;

  // ---- the walk: runs of one person's primitives, a flush where the person changes; the person at hand persists across chunks --------------
  const int cx = 16 * x0 + 8, cy = 16 * y0 + 8;  // the centre of pixel 0
  int* const frame_desc = desc + (long)t.frame * P * kAppearDesc;
  int person = -1;
  unsigned mask = 0;
  for (int base = 0; base < t.count; base += kDrawChunk) {
    const int m = stage_chunk(sp, t, base, index, prims);
    for (int i = 0; i < m; ++i) {
      const DrawPrim p = sp[i];  // every lane reads the same address
      if ((int)p.colour != person) {  // the same primitive for every thread: uniform
        if (person >= 0) appear_flush(hist, frame_desc + (long)person * kAppearDesc, v, mask);
        person = (int)p.colour, mask = 0;
      }
      if (mask == all || draw_block_outside(p, cx, cy)) continue;  // nothing left to find out (a thread without pixels: all == 0)
      for (int q = 0; q < 4; ++q)
        if (((all & ~mask) >> q & 1) && draw_covers(p, cx + 16 * (q & 1), cy + 16 * (q >> 1))) mask |= 1u << q;
    }
  }
  if (person >= 0) appear_flush(hist, frame_desc + (long)person * kAppearDesc, v, mask);
}
}  // namespace

int launch_describe(int format, const DrawPlanes* frames, int height, int width, const DrawTile* tiles, int n_tiles, const int* index,
                    const DrawPrim* prims, int P, int* desc, void* stream) {
  if (n_tiles <= 0) return 0;
  if (format != kFmtBgr && format != kFmtNv12) return (int)hipErrorInvalidValue;
  if (format == kFmtBgr)
    hipLaunchKernelGGL((describe_kernel<kFmtBgr>), dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims, P, desc);
  else
    hipLaunchKernelGGL((describe_kernel<kFmtNv12>), dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, frames, height, width, tiles, index, prims, P, desc);
  return (int)hipGetLastError();
}

}  // namespace dc
