// draw_cover.h — the coverage test of the drawing rule (include/deepcut_hip.h, dc_draw_people), shared by the kernels that decide
// which pixel centres a disc or a capsule covers: draw.hip (the overlay) and redact.hip (the redaction).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dc {

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

}  // namespace dc
