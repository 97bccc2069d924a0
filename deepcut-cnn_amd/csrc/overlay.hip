// overlay.hip — the overlays made from people that are in device memory (dc_overlay_people_device, dc_net_track_frames_async_overlay;
// the rules and the bytes are dc_draw_people's and dc_redact_people's, include/deepcut_hip.h).  The host side is overlay.cpp.
//
// PARITY UNPINNED BY THE REFERENCE, which draws with matplotlib on the host and redacts nothing; the rules are this project's own.
//
// Two steps.  THE BUILDER: one workgroup per frame, one thread per person.  A thread makes its person's primitives exactly as draw.cpp /
// redact.cpp make them — held_joints / snap16, the order, the radii in double with one multiply and one rint, the colour key in int64,
// what TileBins::add drops — once to count them and, behind a workgroup scan that gives every person its stretch, once to write them.
// THE TILE KERNELS: one workgroup per tile of every frame.  The frame's primitives are walked in passes of 256, a thread testing one
// against the tile by TileBins::add's rule; the hits are compacted IN ORDER into LDS (ballot and popcount inside a wave, wave totals
// through LDS) and go through the tile code of frame_tile.h that draw_kernel and redact_kernel run.  A tile nothing hits touches no pixel.
#include <hip/hip_runtime.h>

#include "frame_tile.h"
#include "kernels.h"
#include "label_tile.h"

namespace dc {

namespace {
constexpr int kPass = 256;  // primitives tested at a time: one per thread
static_assert(kPass == kBlocksX * kBlocksY, "a pass is one primitive per thread of the tile's workgroup");

// ---- TileBins::add's rule ---------------------------------------------------------------------------------------------------------------
// the pixels whose CENTRES 16 px + 8 lie in the primitive's bounding box grown by its radius, clipped to the frame (the shifts are
// arithmetic: floor((lo + 7) / 16) is the first pixel whose centre is >= lo, floor((hi - 8) / 16) the last whose centre is <= hi).
// -> whether there is one: a primitive wholly outside is dropped
__device__ __forceinline__ bool prim_pixels(const DrawPrim& p, int H, int W, int& x0, int& y0, int& x1, int& y1) {
  x0 = max(0, (min(p.ax, p.bx) - p.r16 + 7) >> 4), x1 = min(W - 1, (max(p.ax, p.bx) + p.r16 - 8) >> 4);
  y0 = max(0, (min(p.ay, p.by) - p.r16 + 7) >> 4), y1 = min(H - 1, (max(p.ay, p.by) + p.r16 - 8) >> 4);
  return x0 <= x1 && y0 <= y1;
}

// ---- the builder ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double d_max(double a, double b) { return a < b ? b : a; }  // std::max
__device__ __forceinline__ double d_min(double a, double b) { return b < a ? b : a; }  // std::min
__device__ __forceinline__ int snap16_dev(double v) { return (int)rint(16.0 * d_min(32768.0, d_max(-32768.0, v))); }
__device__ __forceinline__ int clamp_int_dev(double v, double lo, double hi) { return (int)d_min(d_max(v, lo), hi); }

// One person's primitives in their order, into out[0 ..) when `out` is not null.  -> how many reach the frame; made: a region primitive
// was made (the redaction's `redacted`), be it wholly outside the frame.  key: what chooses the person's colour
__device__ int person_prims(const OverlayBuild& q, const double* __restrict__ pose, const int* __restrict__ cd, long long key, DrawPrim* out,
                            bool& made) {
  int qx[32], qy[32];
  unsigned held = 0;
  for (int j = 0; j < q.J; ++j) {
    const double x = pose[3 * j], y = pose[3 * j + 1], s = pose[3 * j + 2];
    const bool h = isfinite(x) && isfinite(y) && isfinite(s) && s > q.min_score;
    qx[j] = h ? snap16_dev(x) : 0, qy[j] = h ? snap16_dev(y) : 0;
    held |= (unsigned)h << j;
  }
  auto is_held = [&](int j) { return (held >> j & 1u) != 0; };
  int n = 0;
  auto put = [&](const DrawPrim& p) {
    int x0, y0, x1, y1;
    if (!prim_pixels(p, q.H, q.W, x0, y0, x1, y1)) return;
    if (out) out[n] = p;
    ++n;
  };
  made = false;
  if (!q.redact) {
    // people by index; of a person the limbs in edge order, then the joints in joint order
    unsigned person = 0;
    if (q.by_person) person = key < 0 ? q.untracked : q.palette[(int)(key % q.n_palette)];
    auto filled = [&](int j) { return cd && cd[j] <= -2; };
    for (int e = 0; q.rl > 0 && e < q.n_edges; ++e) {
      const int a = q.edges[2 * e], c = q.edges[2 * e + 1];
      if (!is_held(a) || !is_held(c)) continue;
      const unsigned col = q.by_person ? person : q.palette[c % q.n_palette];
      put(DrawPrim{qx[a], qy[a], qx[c], qy[c], q.rl, 1, filled(a) || filled(c) ? q.alpha_filled : q.alpha, col});
    }
    for (int j = 0; q.rj > 0 && j < q.J; ++j) {
      if (!is_held(j)) continue;
      const unsigned col = q.by_person ? person : q.palette[j % q.n_palette];
      put(DrawPrim{qx[j], qy[j], qx[j], qy[j], q.rj, 0, filled(j) ? q.alpha_filled : q.alpha, col});
    }
    return n;
  }
  // the redaction: a set, kept in the order head disc, limbs, joints
  auto add = [&](const DrawPrim& p) {
    if (p.r16 < 1) return;
    made = true;
    put(p);
  };
  int lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0, n_held = 0;
  for (int j = 0; j < q.J; ++j) {
    if (!is_held(j)) continue;
    lo_x = n_held ? min(lo_x, qx[j]) : qx[j], hi_x = n_held ? max(hi_x, qx[j]) : qx[j];
    lo_y = n_held ? min(lo_y, qy[j]) : qy[j], hi_y = n_held ? max(hi_y, qy[j]) : qy[j];
    ++n_held;
  }
  const int a = q.head_a, c = q.head_b;
  const bool head = is_held(a) && is_held(c);
  if (head) {
    const long long dx = (long long)qx[c] - qx[a], dy = (long long)qy[c] - qy[a], L = dx * dx + dy * dy;
    const double len = sqrt((double)L);
    const double scaled = q.head_scale * len;  // one multiply, one rint
    const int r16 = clamp_int_dev(rint(scaled), q.r_lo, q.r_hi);
    const int mx = (qx[a] + qx[c]) >> 1, my = (qy[a] + qy[c]) >> 1;
    add(DrawPrim{mx, my, mx, my, r16, 0, 0, 0u});
  }
  if (q.region == 1 || (q.region == 2 && !head)) {  // DC_REDACT_BODY, DC_REDACT_HEAD_OR_BODY
    const int s16 = max(hi_x - lo_x, hi_y - lo_y);
    const double scaled = q.body_scale * (double)s16;
    const int rb16 = clamp_int_dev(rint(scaled), q.r_lo, 1024.0);  // the drawing rule's largest capsule radius
    for (int e = 0; e < q.n_edges; ++e) {
      const int ea = q.edges[2 * e], ec = q.edges[2 * e + 1];
      if (is_held(ea) && is_held(ec)) add(DrawPrim{qx[ea], qy[ea], qx[ec], qy[ec], rb16, 1, 0, 0u});
    }
    for (int j = 0; j < q.J; ++j)
      if (is_held(j)) add(DrawPrim{qx[j], qy[j], qx[j], qy[j], rb16, 0, 0, 0u});
  }
  return n;
}

__global__ __launch_bounds__(256) void overlay_build_kernel(const OverlayBuild q, const int* __restrict__ n_people,
                                                            const double* __restrict__ people, const int* __restrict__ cand,
                                                            const long long* __restrict__ ids, const long long* __restrict__ only_ids,
                                                            const long long* __restrict__ keep_ids, DrawPrim* __restrict__ prims,
                                                            int* __restrict__ n_prims, int* __restrict__ redacted) {
  __shared__ int wave_tot[4];
  const int b = blockIdx.x, p = threadIdx.x, lane = p & 63, wave = p >> 6;
  const int n = min(max(n_people[b], 0), q.P);  // whatever the count says, nothing beyond P is read
  const size_t at = (size_t)b * q.P + p;
  bool take = p < n;
  long long key = p;
  if (take && ids) key = ids[at];
  if (take && q.redact) {  // only_ids: only the people with one of these ids; keep_ids: everybody but them
    if (q.n_only >= 0) {
      bool found = false;
      for (int k = 0; k < q.n_only; ++k) found = found || only_ids[k] == key;
      take = found;
    }
    for (int k = 0; take && k < q.n_keep; ++k) take = keep_ids[k] != key;
  }
  const double* pose = people + at * q.J * 3;
  const int* cd = cand ? cand + at * q.J : nullptr;
  bool made = false;
  const int count = take ? person_prims(q, pose, cd, key, nullptr, made) : 0;
  // the workgroup scan: inside a wave by shuffles, the four wave totals through LDS
  int upto = count;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(upto, d);
    if (lane >= d) upto += v;
  }
  if (lane == 63) wave_tot[wave] = upto;
  __syncthreads();
  int first = upto - count, total = 0;
  for (int k = 0; k < 4; ++k) {
    if (k < wave) first += wave_tot[k];
    total += wave_tot[k];
  }
  // the person's stretch: first + count <= the sum over at most P people of at most 1 + n_edges + J each, the frame's stride
  const size_t stride = (size_t)q.P * overlay_prims_per_person(q.J, q.n_edges);
  if (count) person_prims(q, pose, cd, key, prims + (size_t)b * stride + first, made);
  if (p == 0) n_prims[b] = total;
  if (q.redact && redacted && p < q.P) redacted[at] = made ? 1 : 0;
}

// ---- a pass of the tile kernels: which of prims[base .. base + 256) reach tile (tx, ty), compacted in order into sp ------------------------
// Every thread of the workgroup calls it (three barriers).  -> how many there are, the same in every thread
__device__ __forceinline__ int compact_pass(DrawPrim* sp, int* wave_tot, const DrawPrim* __restrict__ prims, int base, int n, int tx, int ty,
                                            int H, int W) {
  const int i = base + (int)threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  DrawPrim p{};
  bool hit = false;
  if (i < n) {
    p = prims[i];
    int x0, y0, x1, y1;
    hit = prim_pixels(p, H, W, x0, y0, x1, y1) && x0 / kDrawTileW <= tx && tx <= x1 / kDrawTileW && y0 / kDrawTileH <= ty &&
          ty <= y1 / kDrawTileH;
  }
  const unsigned long long hits = __ballot(hit);
  const int before = __popcll(hits & ((1ull << lane) - 1ull));
  __syncthreads();  // everybody is through with the chunk before, and with its totals
  if (lane == 0) wave_tot[wave] = __popcll(hits);
  __syncthreads();
  int first = before, total = 0;
  for (int k = 0; k < 4; ++k) {
    if (k < wave) first += wave_tot[k];
    total += wave_tot[k];
  }
  if (hit) sp[first] = p;
  __syncthreads();
  return total;
}

template <int FMT>
__global__ __launch_bounds__(256) void draw_all_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const DrawPrim* __restrict__ prims,
                                                       const int* __restrict__ n_prims, int stride) {
  __shared__ DrawPrim sp[kPass];
  __shared__ int wave_tot[4];
  const int b = blockIdx.z, n = min(n_prims[b], stride);
  if (n <= 0) return;
  const DrawPrim* mine = prims + (size_t)b * stride;
  BlockPixels<FMT> px(blockIdx.x * kDrawTileW, blockIdx.y * kDrawTileH, H, W);
  const int cx = 16 * px.x0 + 8, cy = 16 * px.y0 + 8;  // the centre of pixel 0
  DrawPlanes f{};
  bool loaded = false;
  for (int base = 0; base < n; base += kPass) {
    const int m = compact_pass(sp, wave_tot, mine, base, n, blockIdx.x, blockIdx.y, H, W);
    if (!m) continue;
    if (!loaded) f = frames[b], px.load(f), loaded = true;  // the first hit: a tile nothing reaches loads no pixel
    if (px.n_in) draw_chunk(px, sp, m, cx, cy);
  }
  if (loaded) px.store(f);
}

template <int FMT, int EFFECT>
__global__ __launch_bounds__(256) void redact_all_kernel(const DrawPlanes* __restrict__ frames, int H, int W,
                                                         const DrawPrim* __restrict__ prims, const int* __restrict__ n_prims, int stride,
                                                         int bshift, unsigned fill) {
  __shared__ DrawPrim sp[kPass];
  __shared__ int wave_tot[4];
  __shared__ int flag[kMaxRedactBlocks];
  __shared__ int acc[3][kMaxRedactBlocks];
  const int b = blockIdx.z, n = min(n_prims[b], stride);
  if (n <= 0) return;
  const DrawPrim* mine = prims + (size_t)b * stride;
  int x0, y0;
  bool in[4];
  const int n_in = tile_block(blockIdx.x * kDrawTileW, blockIdx.y * kDrawTileH, H, W, x0, y0, in);
  const int blk = redact_block_of(x0, y0, bshift);
  flag[threadIdx.x] = 0;  // the first pass's barriers follow
  for (int c = 0; c < 3; ++c) acc[c][threadIdx.x] = 0;
  // ---- 1. coverage, fed by the compaction ---------------------------------------------------------------------------------------------
  const int cx = 16 * x0 + 8, cy = 16 * y0 + 8;
  bool hit = false;
  int reached = 0;
  for (int base = 0; base < n; base += kPass) {
    const int m = compact_pass(sp, wave_tot, mine, base, n, blockIdx.x, blockIdx.y, H, W);
    reached += m;
    if (n_in && !hit) redact_cover_chunk(hit, in, sp, m, cx, cy);
  }
  if (!reached) return;  // the same in every thread: nothing reaches the tile, no pixel is loaded
  // ---- 2. sums, 3. stores ---------------------------------------------------------------------------------------------------------------
  const DrawPlanes f = frames[b];
  redact_finish<FMT, EFFECT>(f, H, W, x0, y0, in, n_in, blk, hit, bshift, fill, flag, acc);
}

// ---- the labels (the rule: dc_label_people) ----------------------------------------------------------------------------------------------
// The builder of the labels, in the pattern of overlay_build_kernel: one workgroup per frame, one thread per person, who makes at most
// one label exactly as label.cpp makes it — held joints by snap16, the key's digits by int64 division behind the prefix, the anchor and
// the clamp by label_place —; the workgroup scan puts the labels in person order.  Device labels take no `texts`.
__global__ __launch_bounds__(256) void label_build_kernel(const LabelBuild q, const int* __restrict__ n_people, const double* __restrict__ people,
                                                          const long long* __restrict__ ids, LabelPrim* __restrict__ prims,
                                                          int* __restrict__ n_labels) {
  __shared__ int wave_tot[4];
  const int b = blockIdx.x, p = threadIdx.x, lane = p & 63, wave = p >> 6;
  const int n = min(max(n_people[b], 0), q.P);  // whatever the count says, nothing beyond P is read
  const size_t at = (size_t)b * q.P + p;
  LabelPrim lp{};
  bool made = false;
  if (p < n && (q.alpha_text > 0 || q.alpha_plate > 0)) {
    const long long key = ids ? ids[at] : (long long)p;
    if (key >= 0) {
      const double* pose = people + at * q.J * 3;
      int qx[32], qy[32];
      unsigned held = 0;
      for (int j = 0; j < q.J; ++j) {
        const double x = pose[3 * j], y = pose[3 * j + 1], s = pose[3 * j + 2];
        const bool h = isfinite(x) && isfinite(y) && isfinite(s) && s > q.min_score;
        qx[j] = h ? snap16_dev(x) : 0, qy[j] = h ? snap16_dev(y) : 0;
        held |= (unsigned)h << j;
      }
      for (int k = 0; k < q.n_prefix; ++k) lp.text[k] = q.prefix[k];
      lp.n = label_put_key(key, lp.text, q.n_prefix), lp.s = q.scale;
      made = label_place(qx, qy, held, q.J, q.anchor, lp.n, lp.s, q.gap, q.H, q.W, lp.x, lp.y);
      const unsigned person = q.palette[(int)(key % q.n_palette)];
      lp.text_colour = q.plate_by_person ? q.text_colour : person, lp.plate_colour = q.plate_by_person ? person : q.plate_colour;
      lp.alpha_text = q.alpha_text, lp.alpha_plate = q.alpha_plate;
    }
  }
  const int count = made ? 1 : 0;
  int upto = count;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(upto, d);
    if (lane >= d) upto += v;
  }
  if (lane == 63) wave_tot[wave] = upto;
  __syncthreads();
  int first = upto - count, total = 0;
  for (int k = 0; k < 4; ++k) {
    if (k < wave) first += wave_tot[k];
    total += wave_tot[k];
  }
  if (made) prims[(size_t)b * q.P + first] = lp;  // first < the number of people who made a label <= P, the frame's stride
  if (p == 0) n_labels[b] = total;
}

// Over every tile of every frame, behind draw_all_kernel: the frame's labels are walked in passes of kLabelPass, the first kLabelPass
// threads testing one each against the tile; the hits are compacted in order into LDS and go through label_chunk.  A tile that
// nothing reaches loads no pixel
template <int FMT>
__global__ __launch_bounds__(256) void label_all_kernel(const DrawPlanes* __restrict__ frames, int H, int W, const LabelPrim* __restrict__ prims,
                                                        const int* __restrict__ n_labels, int stride) {
  __shared__ LabelPrim sp[kLabelPass];
  __shared__ unsigned char font[kLabelFontBytes];
  __shared__ int wave_tot[4];
  const int b = blockIdx.z, n = min(n_labels[b], stride);
  if (n <= 0) return;
  const LabelPrim* mine = prims + (size_t)b * stride;
  label_stage_font(font);  // the first pass's barriers follow
  BlockPixels<FMT> px(blockIdx.x * kDrawTileW, blockIdx.y * kDrawTileH, H, W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  DrawPlanes f{};
  bool loaded = false;
  for (int base = 0; base < n; base += kLabelPass) {
    const int i = base + (int)threadIdx.x;
    LabelPrim p{};
    bool hit = false;
    if ((int)threadIdx.x < kLabelPass && i < n) {
      p = mine[i];
      hit = label_reaches(p, blockIdx.x, blockIdx.y, H, W);
    }
    const unsigned long long hits = __ballot(hit);
    const int before = __popcll(hits & ((1ull << lane) - 1ull));
    __syncthreads();  // everybody is through with the pass before, and with its totals
    if (lane == 0) wave_tot[wave] = __popcll(hits);
    __syncthreads();
    int first = before, m = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) first += wave_tot[k];
      m += wave_tot[k];
    }
    if (hit) sp[first] = p;  // first < m <= kLabelPass
    __syncthreads();
    if (!m) continue;  // the same in every thread
    if (!loaded) f = frames[b], px.load(f), loaded = true;
    if (px.n_in) label_chunk(px, sp, m, font);
  }
  if (loaded) px.store(f);
}

// small tables that travel as kernel arguments: no host buffer has to outlive an upload, and nothing waits
struct IdList {
  long long v[kOverlayMaxIds];
};
struct FrameList {
  DrawPlanes f[kOverlayMaxFrames];
};
__global__ void put_ids_kernel(const IdList list, int n, long long* __restrict__ to) {
  if ((int)threadIdx.x < n) to[threadIdx.x] = list.v[threadIdx.x];
}
__global__ void put_frames_kernel(const FrameList list, int n, DrawPlanes* __restrict__ to) {
  if ((int)threadIdx.x < n) to[threadIdx.x] = list.f[threadIdx.x];
}

dim3 tile_grid(int nb, int H, int W) { return dim3((W + kDrawTileW - 1) / kDrawTileW, (H + kDrawTileH - 1) / kDrawTileH, nb); }
}  // namespace

int launch_overlay_put_ids(const long long* host, int n, long long* to, void* stream) {
  if (n <= 0) return 0;
  if (n > kOverlayMaxIds) return (int)hipErrorInvalidValue;
  IdList list{};
  for (int k = 0; k < n; ++k) list.v[k] = host[k];
  hipLaunchKernelGGL(put_ids_kernel, dim3(1), dim3(kOverlayMaxIds), 0, (hipStream_t)stream, list, n, to);
  return (int)hipGetLastError();
}

int launch_overlay_put_frames(const DrawPlanes* host, int nb, DrawPlanes* to, void* stream) {
  if (nb < 1 || nb > kOverlayMaxFrames) return (int)hipErrorInvalidValue;
  FrameList list{};
  for (int b = 0; b < nb; ++b) list.f[b] = host[b];
  hipLaunchKernelGGL(put_frames_kernel, dim3(1), dim3(kOverlayMaxFrames), 0, (hipStream_t)stream, list, nb, to);
  return (int)hipGetLastError();
}

int launch_overlay_build(const OverlayBuild& q, int nb, const int* n_people, const double* people, const int* cand, const long long* ids,
                         const long long* only_ids, const long long* keep_ids, DrawPrim* prims, int* n_prims, int* redacted, void* stream) {
  if (nb < 1 || q.P < 1 || q.P > 256 || q.J < 1 || q.J > 32 || q.n_edges < 0 || q.n_edges > 128 || q.n_only > kOverlayMaxIds ||
      q.n_keep > kOverlayMaxIds || (!q.redact && (q.n_palette < 1 || q.n_palette > 256)) || (q.redact && (q.n_only >= 0 || q.n_keep >= 0) && !ids))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_build_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, q, n_people, people, cand, ids, only_ids, keep_ids, prims,
                     n_prims, redacted);
  return (int)hipGetLastError();
}

int launch_draw_all(int format, const DrawPlanes* frames, int nb, int height, int width, const DrawPrim* prims, const int* n_prims, int stride,
                    void* stream) {
  if ((format != kFmtBgr && format != kFmtNv12) || nb < 1 || nb > kOverlayMaxFrames || height < 1 || width < 1 || stride < 1)
    return (int)hipErrorInvalidValue;
  const dim3 grid = tile_grid(nb, height, width);
  if (format == kFmtBgr)
    hipLaunchKernelGGL(draw_all_kernel<kFmtBgr>, grid, dim3(256), 0, (hipStream_t)stream, frames, height, width, prims, n_prims, stride);
  else
    hipLaunchKernelGGL(draw_all_kernel<kFmtNv12>, grid, dim3(256), 0, (hipStream_t)stream, frames, height, width, prims, n_prims, stride);
  return (int)hipGetLastError();
}

int launch_label_build(const LabelBuild& q, int nb, const int* n_people, const double* people, const long long* ids, LabelPrim* prims,
                       int* n_labels, void* stream) {
  if (nb < 1 || q.P < 1 || q.P > 256 || q.J < 1 || q.J > 32 || q.scale < 1 || q.scale > 8 || q.n_palette < 1 || q.n_palette > 256 ||
      q.n_prefix < 0 || q.n_prefix > 4)
    return (int)hipErrorInvalidValue;
  for (int k = 0; k < q.n_prefix; ++k)
    if (q.prefix[k] >= kLabelGlyphs) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(label_build_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, q, n_people, people, ids, prims, n_labels);
  return (int)hipGetLastError();
}

int launch_label_all(int format, const DrawPlanes* frames, int nb, int height, int width, const LabelPrim* prims, const int* n_labels, int stride,
                     void* stream) {
  if ((format != kFmtBgr && format != kFmtNv12) || nb < 1 || nb > kOverlayMaxFrames || height < 1 || width < 1 || stride < 1)
    return (int)hipErrorInvalidValue;
  const dim3 grid = tile_grid(nb, height, width);
  if (format == kFmtBgr)
    hipLaunchKernelGGL(label_all_kernel<kFmtBgr>, grid, dim3(256), 0, (hipStream_t)stream, frames, height, width, prims, n_labels, stride);
  else
    hipLaunchKernelGGL(label_all_kernel<kFmtNv12>, grid, dim3(256), 0, (hipStream_t)stream, frames, height, width, prims, n_labels, stride);
  return (int)hipGetLastError();
}

namespace {
template <int FMT>
int launch_effect_all(int effect, int bshift, unsigned fill, const DrawPlanes* frames, dim3 grid, int H, int W, const DrawPrim* prims,
                      const int* n_prims, int stride, hipStream_t s) {
  if (effect == kRedactMosaic)
    hipLaunchKernelGGL((redact_all_kernel<FMT, kRedactMosaic>), grid, dim3(256), 0, s, frames, H, W, prims, n_prims, stride, bshift, fill);
  else
    hipLaunchKernelGGL((redact_all_kernel<FMT, kRedactFill>), grid, dim3(256), 0, s, frames, H, W, prims, n_prims, stride, bshift, fill);
  return (int)hipGetLastError();
}
}  // namespace

int launch_redact_all(int format, int effect, int block, unsigned fill, const DrawPlanes* frames, int nb, int height, int width,
                      const DrawPrim* prims, const int* n_prims, int stride, void* stream) {
  int bshift = 0;
  while (bshift < 6 && (1 << bshift) != block) ++bshift;
  if ((format != kFmtBgr && format != kFmtNv12) || (effect != kRedactMosaic && effect != kRedactFill) || bshift < 1 || bshift > 5 || nb < 1 ||
      nb > kOverlayMaxFrames || height < 1 || width < 1 || stride < 1)
    return (int)hipErrorInvalidValue;
  const dim3 grid = tile_grid(nb, height, width);
  return format == kFmtBgr ? launch_effect_all<kFmtBgr>(effect, bshift, fill, frames, grid, height, width, prims, n_prims, stride, (hipStream_t)stream)
                           : launch_effect_all<kFmtNv12>(effect, bshift, fill, frames, grid, height, width, prims, n_prims, stride, (hipStream_t)stream);
}

}  // namespace dc
