// redact.cpp — dc_redact_people: the host half of the redaction.  People become region primitives (a head disc; limbs as capsules and
// joints as discs of a radius taken from the person's size) in 1/16-pixel fixed point, the primitives are binned into the tiles their
// grown bounding boxes touch (tile_bins.h), and one launch redacts the non-empty tiles (redact.hip).  The rule is stated in
// include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own.
#include "net_internal.h"
#include "tile_bins.h"

namespace dc {

namespace {
constexpr double kRedactMaxRadius = 1024.0;  // pixels: the head disc
}  // namespace

void check_redact_style(const char* who, const dc_redact_style* st, int J) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  auto scale_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
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
  check_edges(who, st->n_edges, st->edges, J);
}

void redact_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                   const unsigned char* select, const dc_redact_style* st, int* redacted, void* stream) {
  const char* who = "redact_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  check_frame_dims(who, nb, h, w);
  check_frames(who, frames, nb, h, w);
  check_people_dims(who, P, J);
  check_redact_style(who, st, J);
  check_n_people(who, n_people, nb, P);
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "redact_people() in CPU mode");

  // ---- the primitives: a set, kept in the order people, head disc, limbs, joints -----------------------------------------------------
  const unsigned fill = FrameColour(frames[0])(st->fill);
  const double r_lo = std::rint(16.0 * st->min_radius), r_hi = std::rint(16.0 * st->max_radius);
  TileBins bins(nb, h, w);
  if (redacted) std::fill(redacted, redacted + (size_t)nb * P, 0);
  // -> whether the primitive was made (its radius is not 0), be it wholly outside the frame
  auto add = [&](const DrawPrim& p) {
    if (p.r16 >= 1) bins.add(p);
    return p.r16 >= 1;
  };
  for (int b = 0; b < nb; ++b) {
    for (int p = 0; p < n_people[b]; ++p) {
      if (select && !select[(size_t)b * P + p]) continue;
      const double* pose = people + ((size_t)b * P + p) * J * 3;
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool held[kPeopleMaxJoints];
      held_joints(pose, J, st->min_score, qx, qy, held);
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
        const int rb16 = body_radius16(st->body_scale, held_extent(J, qx, qy, held), r_lo);
        made |= body_capsules(st->n_edges, st->edges, qx, qy, held, rb16, 0u, add);
        for (int j = 0; j < J; ++j)
          if (held[j]) made |= add(DrawPrim{qx[j], qy[j], qx[j], qy[j], rb16, 0, 0, 0u});
      }
      if (redacted && made) redacted[(size_t)b * P + p] = 1;
    }
    if (!bins.close_frame(b)) bad("more than 2^30 primitive-tile pairs to redact");
  }
  if (bins.tiles.empty()) return;  // nothing reaches a frame: no launch, no copy, nothing written

  // ---- one upload (frame table | tiles | index | primitives), the staged planes of host frames behind it, one launch -----------------
  FrameStage stage(frames, nb, h, w, is_device, Context::get().device, stream, bins.bytes());
  bins.pack(stage.head);
  stage.copy_in(bins.touched.data());  // a frame nothing is redacted in does not travel
  // the grid is the number of non-empty tiles
  KCHECK(launch_redact(frames[0].format, st->effect == DC_REDACT_FILL ? kRedactFill : kRedactMosaic, st->block, fill, stage.dev_frames, h, w,
                       reinterpret_cast<const DrawTile*>(stage.dev_head), (int)bins.tiles.size(),
                       reinterpret_cast<const int*>(stage.dev_head + bins.index_at()),
                       reinterpret_cast<const DrawPrim*>(stage.dev_head + bins.prims_at()), stage.s));
  stage.copy_out(bins.touched.data());
}

}  // namespace dc
