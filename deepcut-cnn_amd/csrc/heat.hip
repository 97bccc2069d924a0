// heat.hip — score maps blended into video frames on the device (dc_draw_heatmap; the rule: include/deepcut_hip.h).  The host side
// (the checks, the sample tables, the colours) is heat.cpp.
//
// PARITY UNPINNED BY THE REFERENCE: its demo draws 14 circles with numpy and never shows a map; the rule is this project's own.
//
// One workgroup per 32 x 32 pixel tile of one frame, one thread per 2 x 2 pixel block (frame_tile.h: the ownership — the thread that owns
// a chroma sample owns its four luma pixels, so there are no atomics and no two threads write one byte).  The per-axis tables say which
// map cells a tile reaches: a patch of at most kHeatMaxPatch cells per side.  The workgroup stages it into LDS once, the drawn channels
// only, quantised to 16 bits (the rule's only floating-point step), and every interpolation tap then comes from LDS.
//
// LDS: the whole patch is held, channel-major [place in the joint list][patch row][patch column] — the launch asks for
// n_joints * max_cells * 2 bytes, max_cells being the largest patch of any tile of THIS call.  A wave's lanes read one channel at
// neighbouring cells (2-byte elements in a row: lanes on one dword are a broadcast, a 32-lane half spans two block rows, i.e. a few
// patch rows), so the taps meet few bank conflicts; the staging writes of the NHWC readers stride by a channel plane and do conflict,
// once per cell.  At scale <= 1 a patch is at most 6 x 6 cells: 1 KB for 14 joints, and LDS bounds nothing.  The extreme, scale 8 with
// 32 joints, is 34 * 34 * 32 * 2 B = 74 KB: two workgroups (8 waves) per CU of 160 KB.
#include <hip/hip_runtime.h>

#include "by_kind.h"
#include "frame_tile.h"
#include "kernels.h"

namespace dc {

namespace {
// one sample point: the four taps' places in a channel's patch, and the two fractions (0..255)
struct HeatTap {
  int o00, o01, o10, o11, fx, fy;
};
__device__ __forceinline__ HeatTap heat_tap(int tx, int ty, int lo_x, int lo_y, int Wm, int Hm, int pw) {
  const int i0 = tx >> 8, j0 = ty >> 8, i1 = min(i0 + 1, Wm - 1), j1 = min(j0 + 1, Hm - 1);
  const int r0 = (j0 - lo_y) * pw, r1 = (j1 - lo_y) * pw;
  return HeatTap{r0 + i0 - lo_x, r0 + i1 - lo_x, r1 + i0 - lo_x, r1 + i1 - lo_x, tx & 255, ty & 255};
}
// int32 throughout: q <= 4096, top and bot <= 2^20, the sum <= 2^28
__device__ __forceinline__ int heat_interp(const unsigned short* q, const HeatTap& t) {
  const int top = (int)q[t.o00] * (256 - t.fx) + (int)q[t.o01] * t.fx, bot = (int)q[t.o10] * (256 - t.fx) + (int)q[t.o11] * t.fx;
  return (top * (256 - t.fy) + bot * t.fy + 32768) >> 16;
}

template <int FMT, typename T, bool NCHW>
__global__ __launch_bounds__(256) void heat_kernel(const HeatParams p) {
  constexpr int NS = FMT == kFmtBgr ? 4 : 5;  // sample points of a thread: its pixels q = 2 * row + column, then the chroma sample
  extern __shared__ unsigned short heat_lds[];  // [n_joints][cells]
  const int X0 = (int)blockIdx.x * kDrawTileW, Y0 = (int)blockIdx.y * kDrawTileH, b = (int)blockIdx.z;
  const int X1 = min(X0 + kDrawTileW, p.W) - 1, Y1 = min(Y0 + kDrawTileH, p.H) - 1;
  // the patch: the tables ascend, a block centre lies right of / below its first pixel's centre, and past its last one's at an odd edge
  const int lo_x = p.tx[X0] >> 8, lo_y = p.ty[Y0] >> 8;
  int hi_x = p.tx[X1] >> 8, hi_y = p.ty[Y1] >> 8;
  if (FMT == kFmtNv12) hi_x = max(hi_x, p.cx[X1 >> 1] >> 8), hi_y = max(hi_y, p.cy[Y1 >> 1] >> 8);
  hi_x = min(hi_x + 1, p.Wm - 1), hi_y = min(hi_y + 1, p.Hm - 1);
  const int pw = hi_x - lo_x + 1, ph = hi_y - lo_y + 1, cells = pw * ph, nj = p.n_joints;
  if (cells > p.max_cells) return;  // never: the host sized the launch's LDS by the same tables
  const T* map = static_cast<const T*>(p.map);
  int qmax = 0;
  for (int i = (int)threadIdx.x; i < cells * nj; i += 256) {
    // NHWC: the lanes of a wave take a cell's channels, which are contiguous; NCHW: a channel's cells along a row
    const int k = NCHW ? i / cells : i % nj, cell = NCHW ? i % cells : i / nj;
    const int y = lo_y + cell / pw, x = lo_x + cell % pw, c = p.joints[k];
    const long at = NCHW ? (((long)b * p.C + c) * p.Hm + y) * p.Wm + x : (((long)b * p.Hm + y) * p.Wm + x) * p.cp + p.c0 + c;
    // the one floating-point step: NaN counts as 0 (fmaxf returns its other operand)
    const int q = (int)rintf(fminf(fmaxf((float)map[at], 0.f), 1.f) * 4096.0f);
    heat_lds[k * cells + cell] = (unsigned short)q;
    qmax = max(qmax, q);
  }
  // an interpolated v is at most the largest staged q: below the gate nothing of this tile is blended, and no pixel is loaded
  if (!__syncthreads_or(qmax >= p.vgate)) return;

  const DrawPlanes f = p.frames[b];
  BlockPixels<FMT> px(X0, Y0, p.H, p.W);
  if (!px.n_in) return;  // no barrier follows
  const int x0 = px.x0, y0 = px.y0;
  HeatTap tap[NS];
  {
    const int txa = p.tx[x0], txb = p.tx[min(x0 + 1, p.W - 1)], tya = p.ty[y0], tyb = p.ty[min(y0 + 1, p.H - 1)];
    for (int q = 0; q < 4; ++q) tap[q] = heat_tap(q & 1 ? txb : txa, q >> 1 ? tyb : tya, lo_x, lo_y, p.Wm, p.Hm, pw);
    if (FMT == kFmtNv12) tap[NS - 1] = heat_tap(p.cx[x0 >> 1], p.cy[y0 >> 1], lo_x, lo_y, p.Wm, p.Hm, pw);
  }
  px.load(f);
  auto alpha_of = [&](int s) { return p.alpha_score ? (p.alpha * s + 2048) >> 12 : p.alpha; };
  auto blend = [&](int pt, unsigned colour, int a) { pt < 4 ? px.blend_pixel(pt, colour, a) : px.blend_chroma(colour, a); };
  if (p.by_joint) {  // the list in order, later channels over earlier ones
    for (int k = 0; k < nj; ++k) {
      const unsigned short* qk = heat_lds + k * cells;
      const unsigned colour = p.colour[k];
#pragma unroll
      for (int pt = 0; pt < NS; ++pt) {
        if (pt < 4 && !px.in[pt]) continue;
        const int s = heat_interp(qk, tap[pt]), a = alpha_of(s);
        if (s >= p.vmin && a > 0) blend(pt, colour, a);
      }
    }
  } else {  // interpolate first, then the maximum; one blend
    int vm[NS];
#pragma unroll
    for (int pt = 0; pt < NS; ++pt) vm[pt] = 0;
    for (int k = 0; k < nj; ++k) {
      const unsigned short* qk = heat_lds + k * cells;
#pragma unroll
      for (int pt = 0; pt < NS; ++pt) vm[pt] = max(vm[pt], heat_interp(qk, tap[pt]));
    }
#pragma unroll
    for (int pt = 0; pt < NS; ++pt) {
      if (pt < 4 && !px.in[pt]) continue;
      const int s = vm[pt], a = alpha_of(s);
      if (s >= p.vmin && a > 0) blend(pt, p.colour[min(255, s >> 4)], a);
    }
  }
  px.store(f);
}

template <int FMT, typename T, bool NCHW>
int heat_launch(const HeatParams& p, int nb, size_t lds, void* stream) {
  auto* kernel = heat_kernel<FMT, T, NCHW>;
  if (lds > 32 * 1024) {  // beyond what a launch gets unasked
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid((unsigned)((p.W + kDrawTileW - 1) / kDrawTileW), (unsigned)((p.H + kDrawTileH - 1) / kDrawTileH), (unsigned)nb);
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}
}  // namespace

int launch_heat(int format, int ekind, int nchw, const HeatParams& p, int nb, void* stream) {
  if (nb <= 0) return 0;
  if (format != kFmtBgr && format != kFmtNv12) return (int)hipErrorInvalidValue;
  if (p.n_joints < 1 || p.n_joints > kHeatMaxJoints || p.max_cells < 1 || p.max_cells > (kHeatMaxPatch + 1) * (kHeatMaxPatch + 1) || p.H < 1 ||
      p.W < 1 || p.Hm < 1 || p.Wm < 1 || (nchw && ekind != kElemF32))
    return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)p.n_joints * p.max_cells * sizeof(unsigned short);
  if (nchw) return format == kFmtBgr ? heat_launch<kFmtBgr, float, true>(p, nb, lds, stream) : heat_launch<kFmtNv12, float, true>(p, nb, lds, stream);
  return dc_by_kind(ekind, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return format == kFmtBgr ? heat_launch<kFmtBgr, T, false>(p, nb, lds, stream) : heat_launch<kFmtNv12, T, false>(p, nb, lds, stream);
  });
}

}  // namespace dc
