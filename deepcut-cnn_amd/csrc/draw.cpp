// draw.cpp — dc_draw_people: the host half of the skeleton overlay.  People become an ordered list of primitives (limbs as capsules,
// joints as discs) in 1/16-pixel fixed point with their colours converted once, the primitives are binned into the tiles their grown
// bounding boxes touch, and one launch draws the non-empty tiles (draw.hip).  The rule is stated in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.
#include <map>

#include "net_internal.h"

namespace dc {

namespace {
constexpr int kDrawMaxEdges = 128, kDrawMaxFrames = 64, kDrawMaxSide = 16384;

// pixels -> 1/16 pixel, ties to even
int snap16(double v) { return (int)std::rint(16.0 * std::min(32768.0, std::max(-32768.0, v))); }

}  // namespace

// the calls' device buffer, per device: grow-only and never freed, like the utility stream; the caller holds the runtime lock, and
// every call waits for its work, so the next call finds it free
DevBuf& draw_buffer(int device) {
  static std::map<int, DevBuf*> bufs;
  DevBuf*& b = bufs[device];
  if (!b) b = new DevBuf();
  return *b;
}

void draw_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                 const int* cand, const long long* ids, const dc_draw_style* st, void* stream) {
  const char* who = "draw_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  auto in_range = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
  if (nb < 1 || nb > kDrawMaxFrames) bad("nb must be in [1, " + std::to_string(kDrawMaxFrames) + "]");
  if (h < 1 || h > kDrawMaxSide || w < 1 || w > kDrawMaxSide) bad("height and width must be in [1, " + std::to_string(kDrawMaxSide) + "]");
  check_frames(who, frames, nb, h, w);
  if (P < 1 || P > kPeopleMaxPeople) bad("max_people (P) must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (J < 1 || J > kPeopleMaxJoints) bad("n_joints (J) must be in [1, " + std::to_string(kPeopleMaxJoints) + "]");
  if (!st) bad("null argument: style");
  if (st->n_edges < 0 || st->n_edges > kDrawMaxEdges) bad("n_edges must be in [0, " + std::to_string(kDrawMaxEdges) + "]");
  if (st->n_edges && !st->edges) bad("edges must be [n_edges][2] joints, or n_edges = 0");
  for (int e = 0; e < 2 * st->n_edges; ++e)
    if (st->edges[e] < 0 || st->edges[e] >= J)
      bad("edges[" + std::to_string(e / 2) + "] names joint " + std::to_string(st->edges[e]) + " outside [0, " + std::to_string(J) + ")");
  if (!in_range(st->joint_radius, 0.0, 64.0)) bad("joint_radius must be in [0, 64]");
  if (!in_range(st->limb_radius, 0.0, 64.0)) bad("limb_radius must be in [0, 64]");
  if (st->alpha < 0 || st->alpha > 256) bad("alpha must be in [0, 256]");
  if (st->alpha_filled < 0 || st->alpha_filled > 256) bad("alpha_filled must be in [0, 256]");
  if (!(std::isfinite(st->min_score) && st->min_score >= 0.0)) bad("min_score must be finite and >= 0");
  if (st->color_mode != DC_DRAW_BY_PERSON && st->color_mode != DC_DRAW_BY_JOINT) bad("color_mode must be DC_DRAW_BY_PERSON or DC_DRAW_BY_JOINT");
  if (!st->palette) bad("null argument: palette");
  if (st->n_palette < 1 || st->n_palette > 256) bad("n_palette must be in [1, 256]");
  for (int b = 0; b < nb; ++b)
    if (n_people[b] < 0 || n_people[b] > P)
      bad("n_people[" + std::to_string(b) + "] = " + std::to_string(n_people[b]) + " is outside [0, P = " + std::to_string(P) + "]");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "draw_people() in CPU mode");

  // ---- the primitives, in drawing order: people by index; of a person the limbs in edge order, then the joints in joint order -------
  const int format = frames[0].format;
  const bool nv12 = format == DC_PIX_NV12;
  const ForwardCsc csc(frames[0].matrix, frames[0].range);
  auto colour = [&](const unsigned char* rgb) {
    return nv12 ? csc(rgb[0], rgb[1], rgb[2]) : (unsigned)rgb[2] | (unsigned)rgb[1] << 8 | (unsigned)rgb[0] << 16;
  };
  const int rj = (int)std::rint(16.0 * st->joint_radius), rl = (int)std::rint(16.0 * st->limb_radius);
  const int tiles_x = (w + kDrawTileW - 1) / kDrawTileW, tiles_y = (h + kDrawTileH - 1) / kDrawTileH;
  std::vector<DrawPrim> prims;
  std::vector<DrawTile> tiles;
  std::vector<int> index;
  std::vector<int> count((size_t)tiles_x * tiles_y), slot;  // per tile of the frame at hand: its primitives, then its place in `tiles`
  struct Box {
    int tx0, ty0, tx1, ty1;  // the tiles a primitive is binned into, inclusive
  };
  std::vector<Box> boxes;
  std::vector<char> touched((size_t)nb, 0);
  for (int b = 0; b < nb; ++b) {
    const size_t first_prim = prims.size();
    boxes.clear();
    // a primitive goes into every tile that holds a pixel CENTRE of its bounding box grown by the radius: conservative, and the kernel's
    // result does not depend on it (a tile's extra primitives cover none of its pixels)
    auto add = [&](const DrawPrim& p) {
      auto lo_px = [](int lo) { return (int)std::floor((lo - 8 + 15) / 16.0); };  // the first pixel whose centre 16 px + 8 is >= lo
      auto hi_px = [](int hi) { return (int)std::floor((hi - 8) / 16.0); };       // the last one whose centre is <= hi
      const int x0 = std::max(0, lo_px(std::min(p.ax, p.bx) - p.r16)), x1 = std::min(w - 1, hi_px(std::max(p.ax, p.bx) + p.r16));
      const int y0 = std::max(0, lo_px(std::min(p.ay, p.by) - p.r16)), y1 = std::min(h - 1, hi_px(std::max(p.ay, p.by) + p.r16));
      if (x0 > x1 || y0 > y1) return;  // wholly outside the frame
      prims.push_back(p);
      const Box bx{x0 / kDrawTileW, y0 / kDrawTileH, x1 / kDrawTileW, y1 / kDrawTileH};
      boxes.push_back(bx);
      for (int ty = bx.ty0; ty <= bx.ty1; ++ty)
        for (int tx = bx.tx0; tx <= bx.tx1; ++tx) ++count[(size_t)ty * tiles_x + tx];
    };
    for (int p = 0; p < n_people[b]; ++p) {
      const double* pose = people + ((size_t)b * P + p) * J * 3;
      const int* cd = cand ? cand + ((size_t)b * P + p) * J : nullptr;
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool drawn[kPeopleMaxJoints];
      for (int j = 0; j < J; ++j) {
        const double x = pose[3 * j], y = pose[3 * j + 1], s = pose[3 * j + 2];
        drawn[j] = std::isfinite(x) && std::isfinite(y) && std::isfinite(s) && s > st->min_score;
        if (drawn[j]) qx[j] = snap16(x), qy[j] = snap16(y);
      }
      unsigned person = 0;
      if (st->color_mode == DC_DRAW_BY_PERSON) {
        const long long key = ids ? ids[(size_t)b * P + p] : (long long)p;
        person = colour(key < 0 ? st->untracked : st->palette + 3 * (size_t)(key % st->n_palette));
      }
      auto alpha_of = [&](bool filled) { return filled ? st->alpha_filled : st->alpha; };
      for (int e = 0; rl > 0 && e < st->n_edges; ++e) {
        const int a = st->edges[2 * e], c = st->edges[2 * e + 1];
        if (!drawn[a] || !drawn[c]) continue;
        const unsigned col = st->color_mode == DC_DRAW_BY_PERSON ? person : colour(st->palette + 3 * (size_t)(c % st->n_palette));
        add(DrawPrim{qx[a], qy[a], qx[c], qy[c], rl, 1, alpha_of(cd && (cd[a] <= -2 || cd[c] <= -2)), col});
      }
      for (int j = 0; rj > 0 && j < J; ++j) {
        if (!drawn[j]) continue;
        const unsigned col = st->color_mode == DC_DRAW_BY_PERSON ? person : colour(st->palette + 3 * (size_t)(j % st->n_palette));
        add(DrawPrim{qx[j], qy[j], qx[j], qy[j], rj, 0, alpha_of(cd && cd[j] <= -2), col});
      }
    }
    if (prims.size() == first_prim) continue;
    touched[(size_t)b] = 1;
    // the non-empty tiles of this frame, row by row, each with its stretch of `index`; then the primitives in order fill the stretches
    slot.assign(count.size(), -1);
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        int& c = count[(size_t)ty * tiles_x + tx];
        if (!c) continue;
        slot[(size_t)ty * tiles_x + tx] = (int)tiles.size();
        tiles.push_back(DrawTile{b, tx, ty, (int)index.size(), 0});
        index.resize(index.size() + (size_t)c);
        if (index.size() > ((size_t)1 << 30)) bad("more than 2^30 primitive-tile pairs to draw");
        c = 0;  // ready for the next frame
      }
    for (size_t i = 0; i < boxes.size(); ++i)
      for (int ty = boxes[i].ty0; ty <= boxes[i].ty1; ++ty)
        for (int tx = boxes[i].tx0; tx <= boxes[i].tx1; ++tx) {
          DrawTile& t = tiles[(size_t)slot[(size_t)ty * tiles_x + tx]];
          index[(size_t)t.first + t.count++] = (int)(first_prim + i);
        }
  }
  if (tiles.empty()) return;  // nothing to draw: no launch, no copy, nothing written

  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  HIPCHECK(hipSetDevice(Context::get().device));
  // ---- one upload (frame table | tiles | index | primitives), the staged planes of host frames behind it, one launch -----------------
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const int planes = nv12 ? 2 : 1;
  const int rows[2] = {h, (h + 1) / 2}, rb[2] = {nv12 ? w : 3 * w, 2 * ((w + 1) / 2)};
  const size_t per = up((size_t)rb[0] * rows[0]) + (nv12 ? up((size_t)rb[1] * rows[1]) : 0);
  const size_t fr_b = up((size_t)nb * sizeof(DrawPlanes)), tl_b = up(tiles.size() * sizeof(DrawTile)), ix_b = up(index.size() * sizeof(int)),
               pr_b = up(prims.size() * sizeof(DrawPrim)), head_b = fr_b + tl_b + ix_b + pr_b;
  RuntimeLock rl_;
  hipStream_t s = stream ? (hipStream_t)stream : util_stream();
  unsigned char* dev = (unsigned char*)draw_buffer(Context::get().device).get(head_b + (is_device ? 0 : per * nb));
  std::vector<unsigned char> head(head_b, 0);
  DrawPlanes* table = reinterpret_cast<DrawPlanes*>(head.data());
  for (int b = 0; b < nb; ++b) {
    if (is_device) {
      table[b] = DrawPlanes{(unsigned char*)frames[b].plane[0], nv12 ? (unsigned char*)frames[b].plane[1] : nullptr, frames[b].pitch[0],
                            nv12 ? frames[b].pitch[1] : 0};
    } else {
      // host frames: the planes without their padding, staged behind the head; a frame nothing is drawn into does not travel
      unsigned char* d0 = dev + head_b + per * b;
      table[b] = DrawPlanes{d0, nv12 ? d0 + up((size_t)rb[0] * rows[0]) : nullptr, rb[0], nv12 ? rb[1] : 0};
    }
  }
  std::memcpy(head.data() + fr_b, tiles.data(), tiles.size() * sizeof(DrawTile));
  std::memcpy(head.data() + fr_b + tl_b, index.data(), index.size() * sizeof(int));
  std::memcpy(head.data() + fr_b + tl_b + ix_b, prims.data(), prims.size() * sizeof(DrawPrim));
  HIPCHECK(hipMemcpyAsync(dev, head.data(), head_b, hipMemcpyHostToDevice, s));
  if (!is_device)
    for (int b = 0; b < nb; ++b) {
      if (!touched[(size_t)b]) continue;
      unsigned char* d[2] = {table[b].plane0, table[b].plane1};
      for (int k = 0; k < planes; ++k)
        HIPCHECK(hipMemcpy2DAsync(d[k], (size_t)rb[k], frames[b].plane[k], (size_t)frames[b].pitch[k], (size_t)rb[k], (size_t)rows[k],
                                  hipMemcpyHostToDevice, s));
    }
  // the grid is the number of non-empty tiles
  KCHECK(launch_draw(format, reinterpret_cast<const DrawPlanes*>(dev), h, w, reinterpret_cast<const DrawTile*>(dev + fr_b), (int)tiles.size(),
                     reinterpret_cast<const int*>(dev + fr_b + tl_b), reinterpret_cast<const DrawPrim*>(dev + fr_b + tl_b + ix_b), s));
  if (!is_device)
    for (int b = 0; b < nb; ++b) {
      if (!touched[(size_t)b]) continue;
      unsigned char* d[2] = {table[b].plane0, table[b].plane1};
      for (int k = 0; k < planes; ++k)  // rows of rb[k] bytes into the caller's pitch: the padding is never written
        HIPCHECK(hipMemcpy2DAsync(const_cast<void*>(frames[b].plane[k]), (size_t)frames[b].pitch[k], d[k], (size_t)rb[k], (size_t)rb[k],
                                  (size_t)rows[k], hipMemcpyDeviceToHost, s));
    }
  HIPCHECK(hipStreamSynchronize(s));
}

void draw_limits(int* tile_w, int* tile_h, int* chunk) {
  if (tile_w) *tile_w = kDrawTileW;
  if (tile_h) *tile_h = kDrawTileH;
  if (chunk) *chunk = kDrawChunk;
}

}  // namespace dc
