// label.cpp — dc_label_people / dc_label_font: the host half of the label overlay.  People become an ordered list of labels — the text
// (a `texts` row, or the prefix and the key in decimal), the plate's place from the held joints, clamped into the frame, the two
// colours converted once —, the labels' plate rectangles are binned into the tiles they touch (tile_bins.h, by pixel box), and one launch
// writes the non-empty tiles (label.hip).  The rule is stated in include/deepcut_hip.h.  The device routes check the style with
// check_label_style and make the builder's arguments with label_build_args (overlay.cpp).
//
// PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing; the rule is this project's own.
#include "label_tile.h"
#include "net_internal.h"
#include "tile_bins.h"

namespace dc {

static_assert(kLabelMaxChars == DC_LABEL_MAX_CHARS, "a text row of the C ABI is a LabelPrim's text");
static_assert(sizeof(LabelPrim) == 56, "LabelPrim is packed as the kernels read it");

namespace {
std::string byte_name(unsigned char c) {
  char buf[16];
  std::snprintf(buf, sizeof buf, "0x%02X", (unsigned)c);
  return buf;
}
// the prefix as places in the font table -> its length; refuses a prefix of more than 4 characters or with a byte outside the set
int prefix_glyphs(const char* who, const dc_label_style* st, unsigned char* out) {
  int n = 0;
  while (n < 5 && st->prefix[n]) ++n;
  if (n > 4) throw DcError(DC_EINVAL, std::string(who) + ": prefix must be NUL-terminated and hold at most 4 characters");
  for (int i = 0; i < n; ++i) {
    const int g = label_glyph((unsigned char)st->prefix[i]);
    if (g < 0)
      throw DcError(DC_EINVAL, std::string(who) + ": prefix[" + std::to_string(i) + "] = byte " + byte_name((unsigned char)st->prefix[i]) +
                                   " is outside the label character set");
    out[i] = (unsigned char)g;
  }
  return n;
}
}  // namespace

void check_label_style(const char* who, const dc_label_style* st, int J) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  if (!st) bad("null argument: label style");
  if (st->scale < 1 || st->scale > 8) bad("scale must be in [1, 8]");
  if (st->gap < 0 || st->gap > 64) bad("gap must be in [0, 64]");
  if (st->anchor_joint < -1 || st->anchor_joint >= J) bad("anchor_joint must be -1 or in [0, J = " + std::to_string(J) + ")");
  if (st->alpha_text < 0 || st->alpha_text > 256) bad("alpha_text must be in [0, 256]");
  if (st->alpha_plate < 0 || st->alpha_plate > 256) bad("alpha_plate must be in [0, 256]");
  if (!(std::isfinite(st->min_score) && st->min_score >= 0.0)) bad("min_score must be finite and >= 0");
  if (st->color_mode != DC_LABEL_PLATE_BY_PERSON && st->color_mode != DC_LABEL_TEXT_BY_PERSON)
    bad("color_mode must be DC_LABEL_PLATE_BY_PERSON or DC_LABEL_TEXT_BY_PERSON");
  if (!st->palette) bad("null argument: palette");
  if (st->n_palette < 1 || st->n_palette > 256) bad("n_palette must be in [1, 256]");
  unsigned char glyphs[4];
  prefix_glyphs(who, st, glyphs);
}

LabelBuild label_build_args(const dc_label_style* st, const dc_frame& like, int P, int J, int h, int w) {
  const FrameColour colour(like);
  LabelBuild q{};
  q.P = P, q.J = J, q.H = h, q.W = w;
  q.scale = st->scale, q.gap = st->gap, q.anchor = st->anchor_joint, q.alpha_text = st->alpha_text, q.alpha_plate = st->alpha_plate;
  q.plate_by_person = st->color_mode == DC_LABEL_PLATE_BY_PERSON, q.n_palette = st->n_palette, q.min_score = st->min_score;
  q.text_colour = colour(st->text_color), q.plate_colour = colour(st->plate_color);
  for (int k = 0; k < st->n_palette; ++k) q.palette[k] = colour(st->palette + 3 * (size_t)k);
  q.n_prefix = prefix_glyphs("label style", st, q.prefix);
  return q;
}

void label_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                  const long long* ids, const char* texts, const dc_label_style* st, void* stream) {
  const char* who = "label_people";
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  check_frame_dims(who, nb, h, w);
  check_frames(who, frames, nb, h, w);
  check_people_dims(who, P, J);
  check_label_style(who, st, J);
  check_n_people(who, n_people, nb, P);
  for (int b = 0; texts && b < nb; ++b)
    for (int p = 0; p < n_people[b]; ++p) {
      const char* row = texts + ((size_t)b * P + p) * kLabelMaxChars;
      const std::string at = "texts[" + std::to_string(b) + "][" + std::to_string(p) + "]";
      int n = 0;
      while (n < kLabelMaxChars && row[n]) ++n;
      if (n == kLabelMaxChars) bad(at + " has no NUL in its " + std::to_string(kLabelMaxChars) + " bytes");
      for (int i = 0; i < n; ++i)
        if (label_glyph((unsigned char)row[i]) < 0)
          bad(at + "[" + std::to_string(i) + "] = byte " + byte_name((unsigned char)row[i]) + " is outside the label character set");
    }
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "label_people() in CPU mode");

  // ---- the labels, in order: frames, then people by index ------------------------------------------------------------------------------
  const LabelBuild q = label_build_args(st, frames[0], P, J, h, w);
  std::vector<LabelPrim> prims;
  TileBins bins(nb, h, w);
  for (int b = 0; b < nb; ++b) {
    for (int p = 0; (q.alpha_text > 0 || q.alpha_plate > 0) && p < n_people[b]; ++p) {
      const long long key = ids ? ids[(size_t)b * P + p] : (long long)p;
      const char* row = texts ? texts + ((size_t)b * P + p) * kLabelMaxChars : nullptr;
      LabelPrim lp{};
      if (row && row[0]) {
        for (; row[lp.n]; ++lp.n) lp.text[lp.n] = (unsigned char)label_glyph((unsigned char)row[lp.n]);
      } else if (key >= 0) {
        for (int k = 0; k < q.n_prefix; ++k) lp.text[k] = q.prefix[k];
        lp.n = label_put_key(key, lp.text, q.n_prefix);
      } else {
        continue;  // untracked and no text of its own
      }
      int qx[kPeopleMaxJoints], qy[kPeopleMaxJoints];
      bool is_held[kPeopleMaxJoints];
      held_joints(people + ((size_t)b * P + p) * J * 3, J, q.min_score, qx, qy, is_held);
      unsigned held = 0;
      for (int j = 0; j < J; ++j) held |= (unsigned)is_held[j] << j;
      lp.s = q.scale;
      if (!label_place(qx, qy, held, J, q.anchor, lp.n, lp.s, q.gap, h, w, lp.x, lp.y)) continue;
      const unsigned person = q.palette[key < 0 ? 0 : (int)(key % q.n_palette)];
      lp.text_colour = q.plate_by_person ? q.text_colour : person, lp.plate_colour = q.plate_by_person ? person : q.plate_colour;
      lp.alpha_text = q.alpha_text, lp.alpha_plate = q.alpha_plate;
      // the pixel box is the plate rectangle, also when the plate is not made
      if (bins.add_box(lp.x, lp.y, lp.x + label_plate_w(lp.n, lp.s) - 1, lp.y + label_plate_h(lp.s) - 1)) prims.push_back(lp);
    }
    if (!bins.close_frame(b)) bad("more than 2^30 label-tile pairs");
  }
  if (bins.tiles.empty()) return;  // no label: no launch, no copy, nothing written

  // ---- one upload (frame table | tiles | index | labels), the staged planes of host frames behind it, one launch ----------------------
  const size_t labels_at = bins.prims_at();  // the binner holds no DrawPrim: the labels take their place
  FrameStage stage(frames, nb, h, w, is_device, Context::get().device, stream, labels_at + frame_up(prims.size() * sizeof(LabelPrim)));
  bins.pack(stage.head);
  std::memcpy(stage.head + labels_at, prims.data(), prims.size() * sizeof(LabelPrim));
  stage.copy_in(bins.touched.data());  // a frame nothing is labelled in does not travel
  KCHECK(launch_label(frames[0].format, stage.dev_frames, h, w, reinterpret_cast<const DrawTile*>(stage.dev_head), (int)bins.tiles.size(),
                      reinterpret_cast<const int*>(stage.dev_head + bins.index_at()),
                      reinterpret_cast<const LabelPrim*>(stage.dev_head + labels_at), stage.s));
  stage.copy_out(bins.touched.data());
}

void label_font(int ch, unsigned char* rows) {
  const int g = ch >= 0 && ch < 256 ? label_glyph(ch) : -1;
  if (g < 0) throw DcError(DC_EINVAL, "label_font: byte " + std::to_string(ch) + " is outside the label character set");
  if (!rows) throw DcError(DC_EINVAL, "label_font: null argument: rows");
  for (int r = 0; r < kLabelGlyphRows; ++r) rows[r] = kLabelFont[g][r];
}

}  // namespace dc
