// draw.cpp — dc_draw_people: the host half of the skeleton overlay.  People become an ordered list of primitives (limbs as capsules,
// joints as discs) in 1/16-pixel fixed point with their colours converted once, the primitives are binned into the tiles their grown
// bounding boxes touch (tile_bins.h), and one launch draws the non-empty tiles (draw.hip).  The rule is stated in include/deepcut_hip.h.
// Below it: what the three passes over frames share on the host — the refusals they word alike, their device buffer, and FrameStage.
//
// PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.
#include <map>

#include "net_internal.h"
#include "tile_bins.h"

namespace dc {

void check_draw_style(const char* who, const dc_draw_style* st, int J) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  auto in_range = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
  if (!st) bad("null argument: style");
  check_edges(who, st->n_edges, st->edges, J);
  if (!in_range(st->joint_radius, 0.0, 64.0)) bad("joint_radius must be in [0, 64]");
  if (!in_range(st->limb_radius, 0.0, 64.0)) bad("limb_radius must be in [0, 64]");
  if (st->alpha < 0 || st->alpha > 256) bad("alpha must be in [0, 256]");
  if (st->alpha_filled < 0 || st->alpha_filled > 256) bad("alpha_filled must be in [0, 256]");
  if (!(std::isfinite(st->min_score) && st->min_score >= 0.0)) bad("min_score must be finite and >= 0");
  if (st->color_mode != DC_DRAW_BY_PERSON && st->color_mode != DC_DRAW_BY_JOINT) bad("color_mode must be DC_DRAW_BY_PERSON or DC_DRAW_BY_JOINT");
  if (!st->palette) bad("null argument: palette");
  if (st->n_palette < 1 || st->n_palette > 256) bad("n_palette must be in [1, 256]");
}

void draw_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                 const int* cand, const long long* ids, const dc_draw_style* st, void* stream) {
  const char* who = "draw_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  check_frame_dims(who, nb, h, w);
  check_frames(who, frames, nb, h, w);
  check_people_dims(who, P, J);
  check_draw_style(who, st, J);
  check_n_people(who, n_people, nb, P);
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "draw_people() in CPU mode");

  // ---- the primitives, in drawing order: people by index; of a person the limbs in edge order, then the joints in joint order -------
  const FrameColour colour(frames[0]);
  const int rj = (int)std::rint(16.0 * st->joint_radius), rl = (int)std::rint(16.0 * st->limb_radius);
  TileBins bins(nb, h, w);
  for (int b = 0; b < nb; ++b) {
    for (int p = 0; p < n_people[b]; ++p) {
      const double* pose = people + ((size_t)b * P + p) * J * 3;
      const int* cd = cand ? cand + ((size_t)b * P + p) * J : nullptr;
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool drawn[kPeopleMaxJoints];
      held_joints(pose, J, st->min_score, qx, qy, drawn);
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
        bins.add(DrawPrim{qx[a], qy[a], qx[c], qy[c], rl, 1, alpha_of(cd && (cd[a] <= -2 || cd[c] <= -2)), col});
      }
      for (int j = 0; rj > 0 && j < J; ++j) {
        if (!drawn[j]) continue;
        const unsigned col = st->color_mode == DC_DRAW_BY_PERSON ? person : colour(st->palette + 3 * (size_t)(j % st->n_palette));
        bins.add(DrawPrim{qx[j], qy[j], qx[j], qy[j], rj, 0, alpha_of(cd && cd[j] <= -2), col});
      }
    }
    if (!bins.close_frame(b)) bad("more than 2^30 primitive-tile pairs to draw");
  }
  if (bins.tiles.empty()) return;  // nothing to draw: no launch, no copy, nothing written

  // ---- one upload (frame table | tiles | index | primitives), the staged planes of host frames behind it, one launch -----------------
  FrameStage stage(frames, nb, h, w, is_device, Context::get().device, stream, bins.bytes());
  bins.pack(stage.head);
  stage.copy_in(bins.touched.data());  // a frame nothing is drawn into does not travel
  // the grid is the number of non-empty tiles
  KCHECK(launch_draw(frames[0].format, stage.dev_frames, h, w, reinterpret_cast<const DrawTile*>(stage.dev_head), (int)bins.tiles.size(),
                     reinterpret_cast<const int*>(stage.dev_head + bins.index_at()),
                     reinterpret_cast<const DrawPrim*>(stage.dev_head + bins.prims_at()), stage.s));
  stage.copy_out(bins.touched.data());
}

void draw_limits(int* tile_w, int* tile_h, int* chunk) {
  if (tile_w) *tile_w = kDrawTileW;
  if (tile_h) *tile_h = kDrawTileH;
  if (chunk) *chunk = kDrawChunk;
}

// ---- what the passes over video frames share (net_internal.h): their refusals, their device buffer, the stager ------------------------
namespace {
[[noreturn]] void bad(const char* who, const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); }
}  // namespace

void check_frame_dims(const char* who, int nb, int h, int w) {
  if (nb < 1 || nb > kFrameMaxFrames) bad(who, "nb must be in [1, " + std::to_string(kFrameMaxFrames) + "]");
  if (h < 1 || h > kFrameMaxSide || w < 1 || w > kFrameMaxSide) bad(who, "height and width must be in [1, " + std::to_string(kFrameMaxSide) + "]");
}

void check_people_dims(const char* who, int P, int J) {
  if (P < 1 || P > kPeopleMaxPeople) bad(who, "max_people (P) must be in [1, " + std::to_string(kPeopleMaxPeople) + "]");
  if (J < 1 || J > kPeopleMaxJoints) bad(who, "n_joints (J) must be in [1, " + std::to_string(kPeopleMaxJoints) + "]");
}

void check_edges(const char* who, int n_edges, const int* edges, int J) {
  if (n_edges < 0 || n_edges > kFrameMaxEdges) bad(who, "n_edges must be in [0, " + std::to_string(kFrameMaxEdges) + "]");
  if (n_edges && !edges) bad(who, "edges must be [n_edges][2] joints, or n_edges = 0");
  for (int e = 0; e < 2 * n_edges; ++e)
    if (edges[e] < 0 || edges[e] >= J)
      bad(who, "edges[" + std::to_string(e / 2) + "] names joint " + std::to_string(edges[e]) + " outside [0, " + std::to_string(J) + ")");
}

void check_n_people(const char* who, const int* n_people, int nb, int P) {
  for (int b = 0; b < nb; ++b)
    if (n_people[b] < 0 || n_people[b] > P)
      bad(who, "n_people[" + std::to_string(b) + "] = " + std::to_string(n_people[b]) + " is outside [0, P = " + std::to_string(P) + "]");
}

// grow-only and never freed, like the utility stream; the caller holds the runtime lock, and every call waits for its work, so the
// next call finds it free
DevBuf& draw_buffer(int device) {
  static std::map<int, DevBuf*> bufs;
  DevBuf*& b = bufs[device];
  if (!b) b = new DevBuf();
  return *b;
}

FrameStage::FrameStage(const dc_frame* frames, int nb, int h, int w, bool is_device, int device, void* stream, size_t head_bytes, size_t extra_bytes)
    : frames_(frames), nb_(nb), is_device_(is_device), extra_bytes_(extra_bytes) {
  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  HIPCHECK(hipSetDevice(device));
  lock_ = std::unique_lock<std::recursive_mutex>(runtime_mu());
  s = stream ? (hipStream_t)stream : util_stream();
  const bool nv12 = frames[0].format == DC_PIX_NV12;
  planes_ = nv12 ? 2 : 1;
  rows_[0] = h, rows_[1] = (h + 1) / 2, rb_[0] = nv12 ? w : 3 * w, rb_[1] = 2 * ((w + 1) / 2);
  const size_t p0 = frame_up((size_t)rb_[0] * rows_[0]), per = p0 + (nv12 ? frame_up((size_t)rb_[1] * rows_[1]) : 0);
  const size_t fr_b = frame_up((size_t)nb * sizeof(DrawPlanes)), head_b = frame_up(head_bytes), extra_b = frame_up(extra_bytes);
  unsigned char* dev = (unsigned char*)draw_buffer(device).get(fr_b + head_b + extra_b + (is_device ? 0 : per * nb));
  host_.assign(fr_b + head_b, 0);
  head = host_.data() + fr_b;
  dev_frames = reinterpret_cast<const DrawPlanes*>(dev), dev_head = dev + fr_b, dev_extra = dev_head + head_b;
  DrawPlanes* table = reinterpret_cast<DrawPlanes*>(host_.data());
  for (int b = 0; b < nb; ++b) {
    if (is_device) {
      table[b] = DrawPlanes{(unsigned char*)frames[b].plane[0], nv12 ? (unsigned char*)frames[b].plane[1] : nullptr, frames[b].pitch[0],
                            nv12 ? frames[b].pitch[1] : 0};
    } else {
      unsigned char* d0 = dev_extra + extra_b + per * b;
      table[b] = DrawPlanes{d0, nv12 ? d0 + p0 : nullptr, rb_[0], nv12 ? rb_[1] : 0};
    }
  }
}

void FrameStage::move_planes(const char* mask, bool to_host) {
  if (is_device_) return;
  const DrawPlanes* table = reinterpret_cast<const DrawPlanes*>(host_.data());
  for (int b = 0; b < nb_; ++b) {
    if (mask && !mask[b]) continue;  // a frame nothing reaches does not travel
    unsigned char* d[2] = {table[b].plane0, table[b].plane1};
    for (int k = 0; k < planes_; ++k) {
      void* host = const_cast<void*>(frames_[b].plane[k]);
      const size_t pitch = (size_t)frames_[b].pitch[k], row = (size_t)rb_[k], rows = (size_t)rows_[k];
      if (to_host)  // rows of `row` bytes into the caller's pitch: the padding is never written
        HIPCHECK(hipMemcpy2DAsync(host, pitch, d[k], row, row, rows, hipMemcpyDeviceToHost, s));
      else
        HIPCHECK(hipMemcpy2DAsync(d[k], row, host, pitch, row, rows, hipMemcpyHostToDevice, s));
    }
  }
}

void FrameStage::copy_in(const char* mask, const void* extra) {
  HIPCHECK(hipMemcpyAsync(const_cast<DrawPlanes*>(dev_frames), host_.data(), host_.size(), hipMemcpyHostToDevice, s));
  if (extra) HIPCHECK(hipMemcpyAsync(dev_extra, extra, extra_bytes_, hipMemcpyHostToDevice, s));
  move_planes(mask, false);
}

void FrameStage::copy_out(const char* mask) {
  move_planes(mask, true);
  HIPCHECK(hipStreamSynchronize(s));
}

}  // namespace dc
