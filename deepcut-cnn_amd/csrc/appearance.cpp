// appearance.cpp — dc_describe_people: the host half of the appearance descriptor.  Every person's sampled limbs (the torso) become
// capsules of the redaction's body radius in 1/16-pixel fixed point, each carrying its person's index; they are binned, in person order,
// into the tiles their grown bounding boxes touch (tile_bins.h), and one launch counts the bytes under them per person (appearance.hip).
// The rule is stated in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE, which stops at the maps; the rule is this project's own.
#include <cstddef>

#include "net_internal.h"
#include "tile_bins.h"

namespace dc {

namespace {
constexpr double kAppearMaxMinRadius = 64.0;  // pixels: the body radius never exceeds it
static_assert(kAppearBins == DC_APPEARANCE_BINS, "the kernel's bins are the header's");

void check_appearance_style(const char* who, const dc_appearance_style* st, int J) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  if (!st) bad("null argument: style");
  // the struct's first version ends with min_score; fields a later version adds would read as defaults for an older caller
  constexpr size_t first = offsetof(dc_appearance_style, min_score) + sizeof(st->min_score);
  if (st->size < first) bad("style.size = " + std::to_string(st->size) + " is smaller than dc_appearance_style's first version (" + std::to_string(first) + ")");
  check_edges(who, st->n_edges, st->edges, J);
  if (!(std::isfinite(st->scale) && st->scale >= 0.0)) bad("scale must be finite and >= 0");
  if (!(std::isfinite(st->min_radius) && st->min_radius >= 0.0 && st->min_radius <= kAppearMaxMinRadius)) bad("min_radius must be in [0, 64]");
  if (!(std::isfinite(st->min_score) && st->min_score >= 0.0)) bad("min_score must be finite and >= 0");
}
}  // namespace

void describe_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                     const dc_appearance_style* st, int* desc, void* stream) {
  const char* who = "describe_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  check_frame_dims(who, nb, h, w);
  check_frames(who, frames, nb, h, w);
  check_people_dims(who, P, J);
  check_appearance_style(who, st, J);
  check_n_people(who, n_people, nb, P);
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "describe_people() in CPU mode");

  // ---- the primitives: of every person, in person order, the capsules of the held limbs; the person's index travels as the colour ------
  const double r_lo = std::rint(16.0 * st->min_radius);
  const size_t n_desc = (size_t)nb * P * kAppearDesc;
  TileBins bins(nb, h, w);
  for (int b = 0; b < nb; ++b) {
    for (int p = 0; p < n_people[b]; ++p) {
      const double* pose = people + ((size_t)b * P + p) * J * 3;
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool held[kPeopleMaxJoints];
      held_joints(pose, J, st->min_score, qx, qy, held);
      const int r16 = body_radius16(st->scale, held_extent(J, qx, qy, held), r_lo);
      if (r16 < 1) continue;  // a radius of 0 makes no primitive
      body_capsules(st->n_edges, st->edges, qx, qy, held, r16, (unsigned)p, [&](const DrawPrim& c) { return bins.add(c); });
    }
    if (!bins.close_frame(b)) bad("more than 2^30 primitive-tile pairs to describe");
  }
  std::fill(desc, desc + n_desc, 0);
  if (bins.tiles.empty()) return;  // no region reaches a frame: all zeros, no launch, no copy

  // ---- one upload (frame table | tiles | index | primitives), desc behind it, the staged planes of host frames, one launch -------------
  FrameStage stage(frames, nb, h, w, is_device, Context::get().device, stream, bins.bytes(), n_desc * sizeof(int));
  bins.pack(stage.head);
  stage.copy_in(bins.touched.data());  // a frame no region reaches does not travel; nothing travels back but desc
  int* d_desc = reinterpret_cast<int*>(stage.dev_extra);
  HIPCHECK(hipMemsetAsync(d_desc, 0, n_desc * sizeof(int), stage.s));
  // the grid is the number of non-empty tiles
  KCHECK(launch_describe(frames[0].format, stage.dev_frames, h, w, reinterpret_cast<const DrawTile*>(stage.dev_head), (int)bins.tiles.size(),
                         reinterpret_cast<const int*>(stage.dev_head + bins.index_at()),
                         reinterpret_cast<const DrawPrim*>(stage.dev_head + bins.prims_at()), P, d_desc, stage.s));
  HIPCHECK(hipMemcpyAsync(desc, d_desc, n_desc * sizeof(int), hipMemcpyDeviceToHost, stage.s));
  HIPCHECK(hipStreamSynchronize(stage.s));
}

}  // namespace dc
