// heat.cpp — dc_draw_heatmap / dc_net_draw_heatmap / dc_group_draw_heatmap: the host half of the score-map overlay.  Every check, the
// per-axis sample tables in double, the colours converted once, one upload through the frame passes' stager (FrameStage, net_internal.h),
// one launch (heat.hip).  The rule is stated in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE: its demo draws 14 circles with numpy and never shows a map; the rule is this project's own.
#include "net_internal.h"

// the sample positions are evaluated operation by operation: a fused multiply-add would round (x + 0.5 - origin) * scale - 4.0 once
// instead of twice and move a tie
#pragma STDC FP_CONTRACT OFF

namespace dc {

namespace {
constexpr int kHeatMaxMapSide = 65536;

// the map as the kernel reads it
struct HeatMap {
  const void* ptr;  // device memory; for a host map: null, `host` is uploaded behind the head
  const float* host;
  int cp, c0, ek, nchw;
};

void heat_check(const char* who, const dc_frame* frames, int nb, int h, int w, int C, int Hm, int Wm, double scale, double ox, double oy,
                const dc_heat_style* st) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  auto in_range = [](double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; };
  check_frame_dims(who, nb, h, w);
  if (!frames) bad("null argument: frames");
  check_frames(who, frames, nb, h, w);
  if (C < 1 || C > kHeatMaxJoints) bad("the map's channels (C) must be in [1, " + std::to_string(kHeatMaxJoints) + "]");
  if (Hm < 1 || Hm > kHeatMaxMapSide || Wm < 1 || Wm > kHeatMaxMapSide) bad("the map's Hm and Wm must be in [1, " + std::to_string(kHeatMaxMapSide) + "]");
  if (!in_range(scale, 1.0 / 64.0, 8.0)) bad("scale must be finite and in [1/64, 8]");
  if (!in_range(ox, -32768.0, 32768.0)) bad("origin_x must be finite and in [-32768, 32768]");
  if (!in_range(oy, -32768.0, 32768.0)) bad("origin_y must be finite and in [-32768, 32768]");
  if (!st) bad("null argument: style");
  if (st->n_joints < 1 || st->n_joints > kHeatMaxJoints) bad("n_joints must be in [1, " + std::to_string(kHeatMaxJoints) + "]");
  if (!st->joints) bad("null argument: joints");
  for (int k = 0; k < st->n_joints; ++k)
    if (st->joints[k] < 0 || st->joints[k] >= C)
      bad("joints[" + std::to_string(k) + "] names channel " + std::to_string(st->joints[k]) + " outside [0, " + std::to_string(C) + ")");
  if (st->mode != DC_HEAT_MAX && st->mode != DC_HEAT_BY_JOINT) bad("mode must be DC_HEAT_MAX or DC_HEAT_BY_JOINT");
  if (st->alpha < 0 || st->alpha > 256) bad("alpha must be in [0, 256]");
  if (st->alpha_mode != DC_HEAT_ALPHA_CONST && st->alpha_mode != DC_HEAT_ALPHA_SCORE) bad("alpha_mode must be DC_HEAT_ALPHA_CONST or DC_HEAT_ALPHA_SCORE");
  if (!in_range(st->min_score, 0.0, 1.0)) bad("min_score must be finite and in [0, 1]");
  if (st->mode == DC_HEAT_MAX && !st->lut) bad("null argument: lut (DC_HEAT_MAX)");
  if (st->mode == DC_HEAT_BY_JOINT && !st->palette) bad("null argument: palette (DC_HEAT_BY_JOINT)");
  if (st->mode == DC_HEAT_BY_JOINT && (st->n_palette < 1 || st->n_palette > 256)) bad("n_palette must be in [1, 256]");
}

// t of `count` sample points along one axis: point i at pixel coordinate first + step * i, against a map of `cells` cells
void heat_table(int* t, int count, double first, double step, double origin, double scale, int cells) {
  const long hi = 256L * (cells - 1);
  for (int i = 0; i < count; ++i) {
    const double c = first + step * (double)i;  // exact: small integers and halves
    const double d = c - origin;
    const double m = d * scale;
    const double n = m - 4.0;
    const double u = n / 8.0;
    const long v = (long)std::rint(256.0 * u);
    t[i] = (int)std::min(hi, std::max(0L, v));
  }
}

// the device half (every argument checked; GPU mode): tables, colours, upload, launch on s, copies back, wait.  `device`: whose buffer
void heat_blend_frames(const dc_frame* frames, int nb, int h, int w, bool is_device, const HeatMap& map, int C, int Hm, int Wm, double scale,
                       double ox, double oy, const dc_heat_style* st, int device, void* stream) {
  if (st->alpha == 0) return;  // A(v) = 0 everywhere: no launch, no copy, nothing written
  const int format = frames[0].format;
  const bool nv12 = format == DC_PIX_NV12;
  const int cw = (w + 1) / 2, ch = (h + 1) / 2;
  const int n_col = st->mode == DC_HEAT_MAX ? 256 : st->n_joints;
  const size_t tab_n = (size_t)w + h + (nv12 ? cw + ch : 0), tab_b = frame_up(tab_n * sizeof(int)), col_b = frame_up((size_t)n_col * sizeof(unsigned));
  // the tables | the colours, made here and copied into the stager's head below: the refusal of a too large patch needs the tables and
  // comes before the stager's refusal without a device, so they cannot be written straight into stage.head
  std::vector<unsigned char> head(tab_b + col_b, 0);
  int* tx = reinterpret_cast<int*>(head.data());
  int *ty = tx + w, *cx = ty + h, *cy = cx + cw;
  heat_table(tx, w, 0.5, 1.0, ox, scale, Wm);
  heat_table(ty, h, 0.5, 1.0, oy, scale, Hm);
  if (nv12) heat_table(cx, cw, 1.0, 2.0, ox, scale, Wm), heat_table(cy, ch, 1.0, 2.0, oy, scale, Hm);
  // the largest patch of any tile, per axis, exactly as the kernel derives a tile's patch from the tables
  auto span = [&](const int* t, const int* c, int n, int cells) {
    int most = 1;
    for (int a = 0; a < n; a += kDrawTileW) {
      const int b = std::min(a + kDrawTileW, n) - 1;
      int hi = t[b] >> 8;
      if (nv12) hi = std::max(hi, c[b >> 1] >> 8);
      most = std::max(most, std::min(hi + 1, cells - 1) - (t[a] >> 8) + 1);
    }
    return most;
  };
  static_assert(kDrawTileW == kDrawTileH, "one span rule for both axes");
  const int max_pw = span(tx, cx, w, Wm), max_ph = span(ty, cy, h, Hm);
  if (max_pw > kHeatMaxPatch + 1 || max_ph > kHeatMaxPatch + 1) throw DcError(DC_EINVAL, "draw_heatmap: a tile reaches more map cells than the kernel stages");
  // colours: R, G, B -> the frame's bytes, once
  const FrameColour colour(frames[0]);
  unsigned* col = reinterpret_cast<unsigned*>(head.data() + tab_b);
  for (int i = 0; i < n_col; ++i) col[i] = colour(st->mode == DC_HEAT_MAX ? st->lut + 3 * (size_t)i : st->palette + 3 * (size_t)(i % st->n_palette));

  // every frame travels; a host map goes between the head and the planes
  FrameStage stage(frames, nb, h, w, is_device, device, stream, head.size(), map.host ? (size_t)nb * C * Hm * Wm * sizeof(float) : 0);
  std::memcpy(stage.head, head.data(), head.size());
  stage.copy_in(nullptr, map.host);
  HeatParams p{};
  p.frames = stage.dev_frames;
  p.map = map.host ? (const void*)stage.dev_extra : map.ptr;
  const int* dtab = reinterpret_cast<const int*>(stage.dev_head);
  p.tx = dtab, p.ty = dtab + w, p.cx = nv12 ? dtab + w + h : nullptr, p.cy = nv12 ? dtab + w + h + cw : nullptr;
  p.colour = reinterpret_cast<const unsigned*>(stage.dev_head + tab_b);
  p.H = h, p.W = w, p.Hm = Hm, p.Wm = Wm, p.C = C, p.cp = map.cp, p.c0 = map.c0;
  p.n_joints = st->n_joints, p.by_joint = st->mode == DC_HEAT_BY_JOINT, p.alpha = st->alpha, p.alpha_score = st->alpha_mode == DC_HEAT_ALPHA_SCORE;
  p.vmin = (int)std::rint(4096.0 * st->min_score);
  // the least v that is blended: v >= vmin, and A(v) > 0 — for DC_HEAT_ALPHA_SCORE alpha v + 2048 >= 4096
  p.vgate = p.alpha_score ? std::max(p.vmin, (2048 + st->alpha - 1) / st->alpha) : p.vmin;
  p.max_cells = max_pw * max_ph;
  for (int k = 0; k < st->n_joints; ++k) p.joints[k] = (unsigned char)st->joints[k];
  KCHECK(launch_heat(format, map.ek, map.nchw, p, nb, stage.s));
  stage.copy_out();
}
}  // namespace

void draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const float* map, bool map_is_device, int C, int Hm, int Wm,
                  const dc_heat_geometry* g, const dc_heat_style* st, void* stream) {
  const char* who = "draw_heatmap";
  if (!g) throw DcError(DC_EINVAL, std::string(who) + ": null argument: geometry");
  heat_check(who, frames, nb, h, w, C, Hm, Wm, g->scale, g->origin_x, g->origin_y, st);
  if (!map) throw DcError(DC_EINVAL, std::string(who) + ": null argument: map");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "draw_heatmap() in CPU mode");
  const HeatMap m{map_is_device ? map : nullptr, map_is_device ? nullptr : map, 0, 0, kElemF32, 1};
  heat_blend_frames(frames, nb, h, w, is_device, m, C, Hm, Wm, g->scale, g->origin_x, g->origin_y, st, Context::get().device, stream);
}

void Net::draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const dc_heat_geometry* g, const dc_heat_style* st) {
  const char* who = "draw_heatmap";
  if (!g) throw DcError(DC_EINVAL, std::string(who) + ": null argument: geometry");
  const std::vector<int>& shape = prob_shape();
  heat_check(who, frames, nb, h, w, shape[1], shape[2], shape[3], g->scale, g->origin_x, g->origin_y, st);
  if (shape[0] != nb)
    throw DcError(DC_EINVAL, std::string(who) + ": nb = " + std::to_string(nb) + " frames, the last forward held " + std::to_string(shape[0]) + " images");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "draw_heatmap() in CPU mode");
  ensure_device();
  const MapRef P = map_ref("prob");  // its own refusals: before a forward, `prob` left out of the plan
  const HeatMap m{P.ptr, nullptr, P.cp, P.c0, P.ek, 0};
  heat_blend_frames(frames, nb, h, w, is_device, m, P.C, P.H, P.W, g->scale, g->origin_x, g->origin_y, st, device, stream);
}

void NetGroup::draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const double* scales, int base, double origin_x,
                            double origin_y, const dc_heat_style* st, const FuseMirror* fm_in) {
  const char* who = "draw_heatmap";
  const bool use[3] = {true, false, false};
  int C[3], NB;
  check_fuse(who, scales, base, use, 0, nullptr, nullptr, C, NB);
  const MirrorPlan mp = check_mirror(who, fm_in, base, use, 0, C);
  const std::vector<int>& shape = nets[(size_t)base]->prob_shape();
  heat_check(who, frames, nb, h, w, shape[1], shape[2], shape[3], scales[base], origin_x, origin_y, st);
  if (NB != nb)
    throw DcError(DC_EINVAL, std::string(who) + ": nb = " + std::to_string(nb) + " frames, the last forwards held " + std::to_string(NB) + " images");
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "draw_heatmap() in CPU mode");
  nets[0]->ensure_device();
  void* s = stream();
  const FusedMaps fm = fuse(scales, base, use, nullptr, nullptr, s, mp);
  const Net::MapRef& P = fm.map[0];
  const HeatMap m{P.ptr, nullptr, P.cp, P.c0, P.ek, 0};
  heat_blend_frames(frames, nb, h, w, is_device, m, P.C, P.H, P.W, scales[base], origin_x, origin_y, st, nets[0]->device, s);
  fuse_done(s);
}

}  // namespace dc
