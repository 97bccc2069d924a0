// overlay.cpp — the host side of the overlays made from people in device memory: dc_overlay_people_device, and what
// Net::track_frames_async enqueues behind the tracker for dc_net_track_frames_async_overlay (people.cpp).  The styles are checked with
// the synchronous entries' functions and words and converted once (OverlayPlan); the primitives and the per-tile selection are made on
// the device (overlay.hip), so the host reads no pose and waits for nothing.  The rules are stated in include/deepcut_hip.h.
//
// PARITY UNPINNED BY THE REFERENCE, which draws with matplotlib on the host and redacts nothing; the rules are this project's own.
#include <map>

#include "net_internal.h"

namespace dc {

static_assert(kOverlayMaxFrames == kFrameMaxFrames, "the frame table travels as one kernel argument");
static_assert(sizeof(DrawPlanes) == sizeof(FramePlanes), "a staged frame table is read as the planes that are written");

OverlayPlan::OverlayPlan(const char* who, const dc_frame& like, int nb, int h_, int w_, int P_, int J_, const OverlayArgs& a, bool have_ids)
    : format(like.format), P(P_), J(J_), h(h_), w(w_) {
  auto bad = [&](const std::string& m) { throw DcError(DC_EINVAL, std::string(who) + ": " + m); };
  if (!a.draw && !a.redact && !a.labels)  // the older entries keep their words
    bad(a.styles_entry ? "null argument: style (styles must hold a draw style, a redact style, a label style or several of them)"
                       : "null argument: style (a draw style, a redact style or both)");
  if (a.redact) check_redact_style(who, a.redact, J);
  if (a.draw) check_draw_style(who, a.draw, J);
  if (a.labels) check_label_style(who, a.labels, J);
  auto check_list = [&](const char* name, const long long* v, int n) {
    if (n < 0) return;
    if (!a.redact) bad(std::string(name) + " chooses who is redacted: a redact style is needed");
    if (n > kOverlayMaxIds) bad(std::string(name) + " holds " + std::to_string(n) + " ids, at most " + std::to_string(kOverlayMaxIds) + " are taken");
    if (n && !v) bad(std::string("null argument: ") + name);
    if (!have_ids) bad("only_ids / keep_ids choose people by id: ids is needed");
  };
  check_list("only_ids", a.only_ids, a.n_only);
  check_list("keep_ids", a.keep_ids, a.n_keep);

  const FrameColour colour(like);
  auto common = [&](OverlayBuild& q, int n_edges, const int* edges, double min_score) {
    q.P = P, q.J = J, q.H = h, q.W = w, q.n_edges = n_edges, q.min_score = min_score;
    for (int e = 0; e < 2 * n_edges; ++e) q.edges[e] = (unsigned char)edges[e];
    q.n_only = q.n_keep = -1;
  };
  if (a.redact) {
    const dc_redact_style* st = a.redact;
    redact = true;
    common(rb, st->n_edges, st->edges, st->min_score);
    rb.redact = 1;
    rb.region = st->region, rb.head_a = st->head_a, rb.head_b = st->head_b;
    rb.head_scale = st->head_scale, rb.body_scale = st->body_scale;
    rb.r_lo = std::rint(16.0 * st->min_radius), rb.r_hi = std::rint(16.0 * st->max_radius);
    rb.n_only = a.n_only < 0 ? -1 : a.n_only, rb.n_keep = a.n_keep < 0 ? -1 : a.n_keep;
    for (int k = 0; k < rb.n_only; ++k) only[k] = a.only_ids[k];
    for (int k = 0; k < rb.n_keep; ++k) keep[k] = a.keep_ids[k];
    effect = st->effect == DC_REDACT_FILL ? kRedactFill : kRedactMosaic, block = st->block, fill = colour(st->fill);
    stride_redact = P * overlay_prims_per_person(J, st->n_edges);
  }
  if (a.draw) {
    const dc_draw_style* st = a.draw;
    draw = true;
    common(db, st->n_edges, st->edges, st->min_score);
    db.rj = (int)std::rint(16.0 * st->joint_radius), db.rl = (int)std::rint(16.0 * st->limb_radius);
    db.alpha = st->alpha, db.alpha_filled = st->alpha_filled;
    db.by_person = st->color_mode == DC_DRAW_BY_PERSON, db.n_palette = st->n_palette;
    db.untracked = colour(st->untracked);
    for (int k = 0; k < st->n_palette; ++k) db.palette[k] = colour(st->palette + 3 * (size_t)k);
    stride_draw = P * overlay_prims_per_person(J, st->n_edges);
  }
  if (a.labels) labels = true, lb = label_build_args(a.labels, like, P, J, h, w);
  size_t at = 0;
  auto take = [&](size_t b) {
    const size_t r = at;
    at += frame_up(b);
    return r;
  };
  at_table = take((size_t)nb * sizeof(DrawPlanes));
  at_lists = take(2 * (size_t)kOverlayMaxIds * sizeof(long long));
  at_count = take(3 * (size_t)nb * sizeof(int));
  at_redacted = take((size_t)nb * P * sizeof(int));
  at_prims_r = take((size_t)nb * stride_redact * sizeof(DrawPrim));
  at_prims_d = take((size_t)nb * stride_draw * sizeof(DrawPrim));
  at_prims_l = take(labels ? (size_t)nb * P * sizeof(LabelPrim) : 0);
  bytes = at;
}

void OverlayPlan::build(unsigned char* dev, int nb, const int* d_np, const double* d_ppl, const int* d_cand, const long long* d_ids,
                        int* d_redacted, void* s) const {
  long long* lists = reinterpret_cast<long long*>(dev + at_lists);
  int* count = reinterpret_cast<int*>(dev + at_count);
  if (redact) {
    KCHECK(launch_overlay_put_ids(only, rb.n_only, lists, s));
    KCHECK(launch_overlay_put_ids(keep, rb.n_keep, lists + kOverlayMaxIds, s));
    KCHECK(launch_overlay_build(rb, nb, d_np, d_ppl, nullptr, d_ids, lists, lists + kOverlayMaxIds, reinterpret_cast<DrawPrim*>(dev + at_prims_r),
                                count, d_redacted ? d_redacted : reinterpret_cast<int*>(dev + at_redacted), s));
  }
  if (draw)
    KCHECK(launch_overlay_build(db, nb, d_np, d_ppl, d_cand, d_ids, nullptr, nullptr, reinterpret_cast<DrawPrim*>(dev + at_prims_d), count + nb,
                                nullptr, s));
  if (labels) KCHECK(launch_label_build(lb, nb, d_np, d_ppl, d_ids, reinterpret_cast<LabelPrim*>(dev + at_prims_l), count + 2 * nb, s));
}

void OverlayPlan::tiles(unsigned char* dev, const DrawPlanes* table, int nb, void* s) const {
  DrawPlanes* d_table = reinterpret_cast<DrawPlanes*>(dev + at_table);
  const int* count = reinterpret_cast<const int*>(dev + at_count);
  KCHECK(launch_overlay_put_frames(table, nb, d_table, s));
  if (redact)  // redaction first: the skeletons go over the mosaic
    KCHECK(launch_redact_all(format, effect, block, fill, d_table, nb, h, w, reinterpret_cast<const DrawPrim*>(dev + at_prims_r), count,
                             stride_redact, s));
  if (draw) KCHECK(launch_draw_all(format, d_table, nb, h, w, reinterpret_cast<const DrawPrim*>(dev + at_prims_d), count + nb, stride_draw, s));
  if (labels)  // last: the labels go over everything else
    KCHECK(launch_label_all(format, d_table, nb, h, w, reinterpret_cast<const LabelPrim*>(dev + at_prims_l), count + 2 * nb, P, s));
}

namespace {
// grow-only and never freed, one per device AND stream: work on one stream is ordered, so the next call on it finds the buffer free
// without anybody waiting; a growth frees the old block, which waits for the device
DevBuf& overlay_buffer(int device, void* stream) {
  static std::map<std::pair<int, void*>, DevBuf*> bufs;
  DevBuf*& b = bufs[std::make_pair(device, stream)];
  if (!b) b = new DevBuf();
  return *b;
}
}  // namespace

void overlay_people_device(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* d_np, const double* d_ppl,
                           const int* d_cand, const long long* d_ids, const OverlayArgs& a, void* stream) {
  const char* who = "overlay_people_device";
  check_frame_dims(who, nb, h, w);
  check_frames(who, frames, nb, h, w);
  check_people_dims(who, P, J);
  const OverlayPlan plan(who, frames[0], nb, h, w, P, J, a, d_ids != nullptr);
  if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "overlay_people_device() in CPU mode");
  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  const int device = Context::get().device;
  HIPCHECK(hipSetDevice(device));
  RuntimeLock rl;
  hipStream_t s = stream ? (hipStream_t)stream : util_stream();
  const bool nv12 = frames[0].format == DC_PIX_NV12;
  const int planes = nv12 ? 2 : 1, rows[2] = {h, (h + 1) / 2}, rb[2] = {nv12 ? w : 3 * w, 2 * ((w + 1) / 2)};
  const size_t p0 = frame_up((size_t)rb[0] * rows[0]), per = p0 + (nv12 ? frame_up((size_t)rb[1] * rows[1]) : 0);
  unsigned char* dev = (unsigned char*)overlay_buffer(device, stream).get(plan.bytes + (is_device ? 0 : per * nb));
  std::vector<DrawPlanes> table((size_t)nb);
  for (int b = 0; b < nb; ++b) {
    unsigned char* d0 = is_device ? (unsigned char*)frames[b].plane[0] : dev + plan.bytes + per * b;
    unsigned char* d1 = !nv12 ? nullptr : is_device ? (unsigned char*)frames[b].plane[1] : d0 + p0;
    table[(size_t)b] = DrawPlanes{d0, d1, is_device ? frames[b].pitch[0] : rb[0], !nv12 ? 0 : is_device ? frames[b].pitch[1] : rb[1]};
  }
  // host frames: every one travels up and back (which of them is touched is known on the device only), never its padding
  auto move = [&](bool to_host) {
    for (int b = 0; b < nb; ++b) {
      unsigned char* d[2] = {table[(size_t)b].plane0, table[(size_t)b].plane1};
      for (int k = 0; k < planes; ++k) {
        void* host = const_cast<void*>(frames[b].plane[k]);
        const size_t pitch = (size_t)frames[b].pitch[k], row = (size_t)rb[k], n_rows = (size_t)rows[k];
        if (to_host) HIPCHECK(hipMemcpy2DAsync(host, pitch, d[k], row, row, n_rows, hipMemcpyDeviceToHost, s));
        else HIPCHECK(hipMemcpy2DAsync(d[k], row, host, pitch, row, n_rows, hipMemcpyHostToDevice, s));
      }
    }
  };
  if (!is_device) move(false);
  plan.build(dev, nb, d_np, d_ppl, d_cand, d_ids, a.redacted, s);
  plan.tiles(dev, table.data(), nb, s);
  if (!is_device) move(true);
  if (!is_device || !stream) HIPCHECK(hipStreamSynchronize(s));  // a caller's stream with device frames: the caller's to wait for
}

}  // namespace dc
