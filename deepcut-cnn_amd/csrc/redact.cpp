// redact.cpp — dc_redact_people: the host half of the redaction.  People become region primitives (a head disc; limbs as capsules and
// joints as discs of a radius taken from the person's size) in 1/16-pixel fixed point, the primitives are binned into the tiles their
// grown bounding boxes touch, and one launch redacts the non-empty tiles (redact.hip).  The structure is draw.cpp's; the rule is stated
// in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own.
#include "net_internal.h"

namespace dc {

namespace {
constexpr int kRedactMaxEdges = 128, kRedactMaxFrames = 64, kRedactMaxSide = 16384;  // dc_draw_people's limits
constexpr double kRedactMaxRadius = 1024.0;                                          // pixels: the head disc
constexpr int kRedactBodyCap = 1024;                                                 // 1/16 pixel: the drawing rule's largest capsule radius

// pixels -> 1/16 pixel, ties to even: the drawing rule's snapping
int snap16(double v) { return (int)std::rint(16.0 * std::min(32768.0, std::max(-32768.0, v))); }
// min(max(v, lo), hi) in double, then the conversion: hi wins where lo > hi
int clamp_int(double v, double lo, double hi) { return (int)std::min(std::max(v, lo), hi); }

}  // namespace

void redact_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                   const unsigned char* select, const dc_redact_style* st, int* redacted, void* stream) {
  const char* who = "redact_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  auto scale_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (nb < 1 || nb > kRedactMaxFrames) bad("nb must be in [1, " + std::to_string(kRedactMaxFrames) + "]");
  if (h < 1 || h > kRedactMaxSide || w < 1 || w > kRedactMaxSide) bad("height and width must be in [1, " + std::to_string(kRedactMaxSide) + "]");
  check_frames(who, frames, nb, h, w);
  if (P < 1 || P > kPeopleMaxPeople) bad("max_people (P) must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (J < 1 || J > kPeopleMaxJoints) bad("n_joints (J) must be in [1, " + std::to_string(kPeopleMaxJoints) + "]");
  if (!st) bad("null argument: style");
  if (st->region != DC_REDACT_HEAD && st->region != DC_REDACT_BODY && st->region != DC_REDACT_HEAD_OR_BODY)
    bad("region must be DC_REDACT_HEAD, DC_REDACT_BODY or DC_REDACT_HEAD_OR_BODY");
  if (st->effect != DC_REDACT_MOSAIC && st->effect != DC_REDACT_FILL) bad("effect must be DC_REDACT_MOSAIC or DC_REDACT_FILL");
  if (st->block != 2 && st->block != 4 && st->block != 8 && st->block != 16 && st->block != 32) bad("block must be 2, 4, 8, 16 or 32");
  if (st->head_a < 0 || st->head_a >= J) bad("head_a names joint " + std::to_string(st->head_a) + " outside [0, " + std::to_string(J) + ")");
  if (st->head_b < 0 || st->head_b >= J) bad("head_b names joint " + std::to_string(st->head_b) + " outside [0, " + std::to_string(J) + ")");
  if (st->head_a == st->head_b) bad("head_a and head_b must be two different joints");
  if (!scale_ok(st->head_scale)) bad("head_scale must be finite and >= 0");
  if (!scale_ok(st->body_scale)) bad("body_scale must be finite and >= 0");
  if (!(scale_ok(st->min_radius) && st->min_radius <= kRedactMaxRadius)) bad("min_radius must be in [0, 1024]");
  if (!(scale_ok(st->max_radius) && st->max_radius <= kRedactMaxRadius)) bad("max_radius must be in [0, 1024]");
  if (st->min_radius > st->max_radius) bad("min_radius must not be above max_radius");
  if (!scale_ok(st->min_score)) bad("min_score must be finite and >= 0");
  if (st->n_edges < 0 || st->n_edges > kRedactMaxEdges) bad("n_edges must be in [0, " + std::to_string(kRedactMaxEdges) + "]");
  if (st->n_edges && !st->edges) bad("edges must be [n_edges][2] joints, or n_edges = 0");
  for (int e = 0; e < 2 * st->n_edges; ++e)
    if (st->edges[e] < 0 || st->edges[e] >= J)
      bad("edges[" + std::to_string(e / 2) + "] names joint " + std::to_string(st->edges[e]) + " outside [0, " + std::to_string(J) + ")");
  for (int b = 0; b < nb; ++b)
    if (n_people[b] < 0 || n_people[b] > P)
      bad("n_people[" + std::to_string(b) + "] = " + std::to_string(n_people[b]) + " is outside [0, P = " + std::to_string(P) + "]");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "redact_people() in CPU mode");

  // ---- the primitives: a set, kept in the order people, head disc, limbs, joints -----------------------------------------------------
  const int format = frames[0].format;
  const bool nv12 = format == DC_PIX_NV12;
  unsigned fill = (unsigned)st->fill[2] | (unsigned)st->fill[1] << 8 | (unsigned)st->fill[0] << 16;
  if (nv12) fill = ForwardCsc(frames[0].matrix, frames[0].range)(st->fill[0], st->fill[1], st->fill[2]);
  const double r_lo = std::rint(16.0 * st->min_radius), r_hi = std::rint(16.0 * st->max_radius);
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
  if (redacted) std::fill(redacted, redacted + (size_t)nb * P, 0);
  for (int b = 0; b < nb; ++b) {
    const size_t first_prim = prims.size();
    boxes.clear();
    // a primitive goes into every tile that holds a pixel CENTRE of its bounding box grown by the radius: conservative, and a selected
    // block lies in the tile of the covered pixel that selects it.  -> whether the primitive was made (its radius is not 0)
    auto add = [&](const DrawPrim& p) {
      if (p.r16 < 1) return false;
      auto lo_px = [](int lo) { return (int)std::floor((lo - 8 + 15) / 16.0); };  // the first pixel whose centre 16 px + 8 is >= lo
      auto hi_px = [](int hi) { return (int)std::floor((hi - 8) / 16.0); };       // the last one whose centre is <= hi
      const int x0 = std::max(0, lo_px(std::min(p.ax, p.bx) - p.r16)), x1 = std::min(w - 1, hi_px(std::max(p.ax, p.bx) + p.r16));
      const int y0 = std::max(0, lo_px(std::min(p.ay, p.by) - p.r16)), y1 = std::min(h - 1, hi_px(std::max(p.ay, p.by) + p.r16));
      if (x0 > x1 || y0 > y1) return true;  // made, and wholly outside the frame
      prims.push_back(p);
      const Box bx{x0 / kDrawTileW, y0 / kDrawTileH, x1 / kDrawTileW, y1 / kDrawTileH};
      boxes.push_back(bx);
      for (int ty = bx.ty0; ty <= bx.ty1; ++ty)
        for (int tx = bx.tx0; tx <= bx.tx1; ++tx) ++count[(size_t)ty * tiles_x + tx];
      return true;
    };
    for (int p = 0; p < n_people[b]; ++p) {
      if (select && !select[(size_t)b * P + p]) continue;
      const double* pose = people + ((size_t)b * P + p) * J * 3;
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool held[kPeopleMaxJoints];
      int lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0, n_held = 0;
      for (int j = 0; j < J; ++j) {
        const double x = pose[3 * j], y = pose[3 * j + 1], s = pose[3 * j + 2];
        held[j] = std::isfinite(x) && std::isfinite(y) && std::isfinite(s) && s > st->min_score;
        if (!held[j]) continue;
        qx[j] = snap16(x), qy[j] = snap16(y);
        lo_x = n_held ? std::min(lo_x, qx[j]) : qx[j], hi_x = n_held ? std::max(hi_x, qx[j]) : qx[j];
        lo_y = n_held ? std::min(lo_y, qy[j]) : qy[j], hi_y = n_held ? std::max(hi_y, qy[j]) : qy[j];
        ++n_held;
      }
      bool made = false;
      const int a = st->head_a, c = st->head_b;
      const bool head = held[a] && held[c];
      if (head) {
        const long long dx = (long long)qx[c] - qx[a], dy = (long long)qy[c] - qy[a], L = dx * dx + dy * dy;
        const double len = std::sqrt((double)L);
        const double scaled = st->head_scale * len;  // one multiply, one rint
        const int r16 = clamp_int(std::rint(scaled), r_lo, r_hi);
        const int mx = (qx[a] + qx[c]) >> 1, my = (qy[a] + qy[c]) >> 1;
        made |= add(DrawPrim{mx, my, mx, my, r16, 0, 0, 0u});
      }
      if (st->region == DC_REDACT_BODY || (st->region == DC_REDACT_HEAD_OR_BODY && !head)) {
        const int s16 = std::max(hi_x - lo_x, hi_y - lo_y);
        const double scaled = st->body_scale * (double)s16;
        const int rb16 = clamp_int(std::rint(scaled), r_lo, (double)kRedactBodyCap);
        for (int e = 0; e < st->n_edges; ++e) {
          const int ea = st->edges[2 * e], ec = st->edges[2 * e + 1];
          if (held[ea] && held[ec]) made |= add(DrawPrim{qx[ea], qy[ea], qx[ec], qy[ec], rb16, 1, 0, 0u});
        }
        for (int j = 0; j < J; ++j)
          if (held[j]) made |= add(DrawPrim{qx[j], qy[j], qx[j], qy[j], rb16, 0, 0, 0u});
      }
      if (redacted && made) redacted[(size_t)b * P + p] = 1;
    }
    if (prims.size() == first_prim) continue;
    touched[(size_t)b] = 1;
    // the non-empty tiles of this frame, row by row, each with its stretch of `index`; then the primitives fill the stretches
    slot.assign(count.size(), -1);
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        int& c = count[(size_t)ty * tiles_x + tx];
        if (!c) continue;
        slot[(size_t)ty * tiles_x + tx] = (int)tiles.size();
        tiles.push_back(DrawTile{b, tx, ty, (int)index.size(), 0});
        index.resize(index.size() + (size_t)c);
        if (index.size() > ((size_t)1 << 30)) bad("more than 2^30 primitive-tile pairs to redact");
        c = 0;  // ready for the next frame
      }
    for (size_t i = 0; i < boxes.size(); ++i)
      for (int ty = boxes[i].ty0; ty <= boxes[i].ty1; ++ty)
        for (int tx = boxes[i].tx0; tx <= boxes[i].tx1; ++tx) {
          DrawTile& t = tiles[(size_t)slot[(size_t)ty * tiles_x + tx]];
          index[(size_t)t.first + t.count++] = (int)(first_prim + i);
        }
  }
  if (tiles.empty()) return;  // nothing reaches a frame: no launch, no copy, nothing written

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
      // host frames: the planes without their padding, staged behind the head; a frame nothing is redacted in does not travel
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
  KCHECK(launch_redact(format, st->effect == DC_REDACT_FILL ? kRedactFill : kRedactMosaic, st->block, fill, reinterpret_cast<const DrawPlanes*>(dev),
                       h, w, reinterpret_cast<const DrawTile*>(dev + fr_b), (int)tiles.size(), reinterpret_cast<const int*>(dev + fr_b + tl_b),
                       reinterpret_cast<const DrawPrim*>(dev + fr_b + tl_b + ix_b), s));
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

}  // namespace dc
