// net_internal.h — what the translation units of the graph runtime share and nobody else sees (net.h is the interface).
// Round 5: csrc/net.cpp (3 700 lines) was split by concern, no behaviour change:
//   runtime.cpp   Caffe context, the process-wide runtime lock, device allocation / fills / uploads, DevBuf (the grow-only device
//                 buffer, net.h), Storage (SyncedMemory + Blob)
//   net_init.cpp  Net::Init semantics: InsertSplits, layer set-up and shape inference, weight files
//   net_lower.cpp the lowering to a launch plan and the per-shape plan cache
//   net_tune.cpp  tile selection by measurement, the tune-cache file, set_tile / reports
//   net_run.cpp   execution: uploads, SyncedMemory moves, launches, hipGraph capture, the batch / request entries, map output
//   net_image.cpp image entry (pre-processing on the device), pose decode, multi-person consumers, plan / profile / debug text;
//                 the map readers on MapRefs that Net and NetGroup share (select_parts; people.cpp: assemble_maps)
//   net_group.cpp NetGroup: pyramid-grouped execution
//   streams.cpp   the process-wide pool of executor streams chosen by measurement (round 5)
//   multi_gpu.cpp in-process multi-GPU forward of the C ABI (round 5)
// This header: CallStream (the one stream rule of the entries), decode_to and the box table's layout (shared by the readers), and what
// the passes over video frames share: their limits and refusals, snap16 / held_joints / FrameColour, FrameStage.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <sstream>
#include <string>

#include "../../include/deepcut_hip.h"
#include "net.h"

namespace dc {

#define HIPCHECK(expr)                                                                               \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      throw DcError(DC_EDEVICE, std::string(#expr) + " failed: " + hipGetErrorString(e_));           \
  } while (0)
#define KCHECK(expr)                                                                                 \
  do {                                                                                               \
    int e_ = (expr);                                                                                 \
    if (e_ != 0)                                                                                     \
      throw DcError(DC_EDEVICE, std::string(#expr) + " failed: " + hipGetErrorString((hipError_t)e_)); \
  } while (0)

// ---- runtime.cpp ----------------------------------------------------------------------------------
std::recursive_mutex& runtime_mu();
struct RuntimeLock {
  std::lock_guard<std::recursive_mutex> lk;
  RuntimeLock() : lk(runtime_mu()) {}
};
hipStream_t util_stream();  // utility stream of the current device (non-blocking, never destroyed); caller holds the runtime lock
void dev_zero(void* p, size_t bytes, void* s);
void dev_upload(void* dst, const void* src, size_t bytes, void* s);
void dev_free(void* p);
void dev_alloc(void** p, size_t bytes);
void storage_to_device_impl(Storage& s, void* stream, bool wait);

// ---- the stream rule of the entries that take a `stream` (include/deepcut_hip.h, dc_net_forward_batch) ----------------------------
// NULL: the executor's own stream, synchronous.  A caller's stream, or DC_STREAM_OWN (the executor's own): asynchronous when the buffers
// are device memory, nothing is waited for; host destinations are always waited for.
struct CallStream {
  void* user;  // the caller's stream, else null
  bool own;    // DC_STREAM_OWN
  explicit CallStream(void* user_stream) : user(user_stream == DC_STREAM_OWN ? nullptr : user_stream), own(user_stream == DC_STREAM_OWN) {}
  void* on(void* own_stream) const { return user ? user : own_stream; }  // the caller's stream, or the executor's own
  bool async() const { return user || own; }
  void finish(bool is_device, void* s) const {
    if (!(is_device && async())) HIPCHECK(hipStreamSynchronize((hipStream_t)s));
  }
};

// ---- shared by the map readers of Net and NetGroup (net_image.cpp, net_group.cpp) -------------------------------------------------
// the pose doubles of a decode on `s`: straight into a device destination, or through `scratch` to the host (enqueued, not waited for)
template <typename Launch>
void decode_to(DevBuf& scratch, size_t cnt, double* out, bool is_device, void* s, const Launch& launch) {
  if (is_device) {
    KCHECK(launch(out));
    return;
  }
  double* dev = (double*)scratch.get(cnt * sizeof(double));
  KCHECK(launch(dev));
  HIPCHECK(hipMemcpyAsync(out, dev, cnt * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)s));
}
// the box table of n boxes (Net::box_dev_ / box_host_): BoxPrepItem[n], padded to 16 bytes, then PoseDecodeItem[n]
inline size_t box_decode_offset(int n) { return ((size_t)n * sizeof(BoxPrepItem) + 15) / 16 * 16; }
inline size_t box_table_bytes(int n) { return box_decode_offset(n) + (size_t)n * sizeof(PoseDecodeItem); }
// library's own and only kernel launches are recorded — nothing another thread does can belong to the capture.
template <class F>
hipGraphExec_t capture_graph(void* cs, F&& enqueue) {
  RuntimeLock rl;
  hipGraph_t graph;
  HIPCHECK(hipStreamBeginCapture((hipStream_t)cs, hipStreamCaptureModeRelaxed));
  try {
    enqueue(cs);
  } catch (...) {
    hipGraph_t g2;
    (void)hipStreamEndCapture((hipStream_t)cs, &g2);
    throw;
  }
  HIPCHECK(hipStreamEndCapture((hipStream_t)cs, &graph));
  hipGraphExec_t ge;
  const hipError_t e = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) throw DcError(DC_EDEVICE, std::string("hipGraphInstantiate failed: ") + hipGetErrorString(e));
  return ge;
}

// ---- shared by the passes over video frames (draw.cpp, heat.cpp, redact.cpp; defined in draw.cpp) --------------------------------------
#define DC_INTERNAL __attribute__((visibility("hidden")))  // shared by the translation units, no part of what the library exports
constexpr int kFrameMaxFrames = 64, kFrameMaxSide = 16384, kFrameMaxEdges = 128;
// the refusals the passes word alike (DC_EINVAL, "<who>: ..."), each called where the entry's order of checks has it
DC_INTERNAL void check_frame_dims(const char* who, int nb, int h, int w);
DC_INTERNAL void check_people_dims(const char* who, int P, int J);
DC_INTERNAL void check_edges(const char* who, int n_edges, const int* edges, int J);
DC_INTERNAL void check_n_people(const char* who, const int* n_people, int nb, int P);
// the styles as dc_draw_people / dc_redact_people refuse them, a null one included (draw.cpp, redact.cpp)
DC_INTERNAL void check_draw_style(const char* who, const dc_draw_style* st, int J);
DC_INTERNAL void check_redact_style(const char* who, const dc_redact_style* st, int J);
// the label style as dc_label_people refuses it (label.cpp), and the builder's arguments made from a checked one
DC_INTERNAL void check_label_style(const char* who, const dc_label_style* st, int J);
DC_INTERNAL LabelBuild label_build_args(const dc_label_style* st, const dc_frame& like, int P, int J, int h, int w);
// pixels -> 1/16 pixel, ties to even
DC_INTERNAL inline int snap16(double v) { return (int)std::rint(16.0 * std::min(32768.0, std::max(-32768.0, v))); }
// a pose [J][3] (x, y, score) -> held[j]: the joint is finite and its score above min_score; then (qx, qy)[j] is its snapped place
DC_INTERNAL inline void held_joints(const double* pose, int J, double min_score, int* qx, int* qy, bool* held) {
  for (int j = 0; j < J; ++j) {
    const double x = pose[3 * j], y = pose[3 * j + 1], s = pose[3 * j + 2];
    held[j] = std::isfinite(x) && std::isfinite(y) && std::isfinite(s) && s > min_score;
    if (held[j]) qx[j] = snap16(x), qy[j] = snap16(y);
  }
}
// ---- the body primitives of the redaction rule, shared by dc_redact_people (redact.cpp) and dc_describe_people (appearance.cpp) ---------
constexpr int kBodyRadiusCap = 1024;  // 1/16 pixel: the drawing rule's largest capsule radius
// min(max(v, lo), hi) in double, then the conversion: hi wins where lo > hi
DC_INTERNAL inline int clamp_int(double v, double lo, double hi) { return (int)std::min(std::max(v, lo), hi); }
// s16: the larger side of the bounding box of the held joints in snapped units (0 for one joint or none)
DC_INTERNAL inline int held_extent(int J, const int* qx, const int* qy, const bool* held) {
  int lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0, n_held = 0;
  for (int j = 0; j < J; ++j) {
    if (!held[j]) continue;
    lo_x = n_held ? std::min(lo_x, qx[j]) : qx[j], hi_x = n_held ? std::max(hi_x, qx[j]) : qx[j];
    lo_y = n_held ? std::min(lo_y, qy[j]) : qy[j], hi_y = n_held ? std::max(hi_y, qy[j]) : qy[j];
    ++n_held;
  }
  return std::max(hi_x - lo_x, hi_y - lo_y);
}
// the body radius clamp(rint(scale * s16), r_lo, 1024), r_lo = rint(16 min_radius): one double multiply, one rint
DC_INTERNAL inline int body_radius16(double scale, int s16, double r_lo) {
  const double scaled = scale * (double)s16;
  return clamp_int(std::rint(scaled), r_lo, (double)kBodyRadiusCap);
}
// every limb of `edges` whose two joints are held, as a capsule of radius r16 carrying `colour`, handed to add(DrawPrim) -> whether the
// primitive was made; -> whether any was
template <class Add>
inline bool body_capsules(int n_edges, const int* edges, const int* qx, const int* qy, const bool* held, int r16, unsigned colour, Add&& add) {
  bool made = false;
  for (int e = 0; e < n_edges; ++e) {
    const int ea = edges[2 * e], ec = edges[2 * e + 1];
    if (held[ea] && held[ec]) made |= add(DrawPrim{qx[ea], qy[ea], qx[ec], qy[ec], r16, 1, 0, colour});
  }
  return made;
}
inline int clip8(long v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }
// the forward colour rule: the counterpart of frame_csc's inverse (net_image.cpp), coefficients in double, rounded to nearest
struct ForwardCsc {
  int y0, y[3], cb[3], cr[3];
  ForwardCsc(int matrix, int range) {
    const double Kr = matrix == DC_CSC_BT709 ? 0.2126 : 0.299, Kb = matrix == DC_CSC_BT709 ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
    const double sy = range == DC_RANGE_FULL ? 1.0 : 255.0 / 219.0, sc = range == DC_RANGE_FULL ? 1.0 : 255.0 / 224.0;
    y0 = range == DC_RANGE_FULL ? 0 : 16;
    const double ky[3] = {Kr, Kg, Kb}, kb[3] = {-Kr, -Kg, 1.0 - Kb}, kr[3] = {1.0 - Kr, -Kg, -Kb};
    for (int i = 0; i < 3; ++i) {
      y[i] = (int)std::rint(65536.0 * ky[i] / sy);
      cb[i] = (int)std::rint(65536.0 * kb[i] / (2.0 * (1.0 - Kb)) / sc);
      cr[i] = (int)std::rint(65536.0 * kr[i] / (2.0 * (1.0 - Kr)) / sc);
    }
  }
  // R, G, B -> Y | Cb << 8 | Cr << 16; the shift is arithmetic
  unsigned operator()(int r, int g, int b) const {
    const int Y = clip8(y0 + ((y[0] * r + y[1] * g + y[2] * b + 32768) >> 16));
    const int Cb = clip8(128 + ((cb[0] * r + cb[1] * g + cb[2] * b + 32768) >> 16));
    const int Cr = clip8(128 + ((cr[0] * r + cr[1] * g + cr[2] * b + 32768) >> 16));
    return (unsigned)Y | (unsigned)Cb << 8 | (unsigned)Cr << 16;
  }
};
// R, G, B -> a frame's bytes as DrawPrim::colour: Y | Cb << 8 | Cr << 16 by the forward rule, or B | G << 8 | R << 16; the
// coefficients are made once
struct DC_INTERNAL FrameColour {
  bool nv12;
  ForwardCsc csc;
  explicit FrameColour(const dc_frame& f) : nv12(f.format == DC_PIX_NV12), csc(f.matrix, f.range) {}
  unsigned operator()(const unsigned char* rgb) const {
    return nv12 ? csc(rgb[0], rgb[1], rgb[2]) : (unsigned)rgb[2] | (unsigned)rgb[1] << 8 | (unsigned)rgb[0] << 16;
  }
};
// the passes' device buffer, per device (draw.cpp): the caller holds the runtime lock, and every call waits for its work
DevBuf& draw_buffer(int device);
// One call's device memory in that buffer and the way of host frames through it.  The layout, every part rounded up to 256 bytes:
//   DrawPlanes[nb] | the caller's head | extra (heat's host map) | host frames only: every frame's planes without their padding
// The constructor refuses without a device, makes `device` current, takes the runtime lock (held until destruction), chooses the stream
// (the caller's, else the utility stream) and fills the table: the caller's planes for device frames, the staged ones for host frames.
// The caller then fills `head`, calls copy_in, launches on `s`, and calls copy_out.  mask: [nb], the frames that travel; null = all.
struct DC_INTERNAL FrameStage {
  FrameStage(const dc_frame* frames, int nb, int h, int w, bool is_device, int device, void* stream, size_t head_bytes, size_t extra_bytes = 0);
  void copy_in(const char* mask = nullptr, const void* extra = nullptr);  // the table and the head, `extra`, the planes of host frames
  void copy_out(const char* mask = nullptr);                              // the planes of host frames back (never their padding); the wait
  hipStream_t s;
  unsigned char* head;           // host: head_bytes zeros
  const DrawPlanes* dev_frames;  // device: the table, the head, the extra block
  unsigned char *dev_head, *dev_extra;

 private:
  void move_planes(const char* mask, bool to_host);
  std::unique_lock<std::recursive_mutex> lock_;
  const dc_frame* frames_;
  int nb_, planes_, rows_[2], rb_[2];  // per plane: rows, and the bytes of a row
  bool is_device_;
  size_t extra_bytes_;
  std::vector<unsigned char> host_;  // the table | the head
};

// The overlays from people in device memory (overlay.cpp), checked with the synchronous entries' words (DC_EINVAL, before a device is
// needed) and converted once: the builders' arguments, the id lists, and the layout of the device block the launches work in —
//   DrawPlanes[nb] | only_ids, keep_ids | n_prims of the redaction, of the drawing, of the labels | redacted [nb][P] | the redaction's
//   primitives | the drawing's | the labels' (LabelPrim [nb][P]) — every part rounded up to 256 bytes.  like: a frame of the call (format, matrix, range).
// build: the builders, which read the people — for the chain IN FRONT OF the tracker's event, since they read its scratch.  tiles: the
// frame table (host copy `table`, travelling as a kernel argument) and the tile kernels, redaction first; they read the block only.
struct DC_INTERNAL OverlayPlan {
  OverlayPlan(const char* who, const dc_frame& like, int nb, int h, int w, int P, int J, const OverlayArgs& a, bool have_ids);
  void build(unsigned char* dev, int nb, const int* d_np, const double* d_ppl, const int* d_cand, const long long* d_ids, int* d_redacted,
             void* s) const;  // d_redacted null: the block's own
  void tiles(unsigned char* dev, const DrawPlanes* table, int nb, void* s) const;
  bool draw = false, redact = false, labels = false;
  int format, effect = 0, block = 0, P, J, h, w, stride_draw = 0, stride_redact = 0;
  unsigned fill = 0;
  OverlayBuild db{}, rb{};
  LabelBuild lb{};
  long long only[kOverlayMaxIds] = {}, keep[kOverlayMaxIds] = {};
  size_t at_table = 0, at_lists = 0, at_count = 0, at_redacted = 0, at_prims_r = 0, at_prims_d = 0, at_prims_l = 0, bytes = 0;
};

// ---- streams.cpp ------------------------------------------------------------------------------------
std::vector<void*> executor_stream_pool(int device, size_t want);  // a COPY of the first `want` process-wide candidates
void pool_stream_acquire(void* s);
void pool_stream_release(void* s);
int pool_stream_users(void* s);

// ---- small helpers -----------------------------------------------------------------------------------
inline int env_int(const char* k, int def) {
  const char* v = std::getenv(k);
  return v ? std::atoi(v) : def;
}
inline int form_mode(const ConvForm& f) { return env_int(f.env, f.env_default); }  // a form's switch: -1 / 0 / >= 1 (kernels.h ConvForm::env)
uint64_t content_hash(const float* p, size_t n);               // net_lower.cpp
void load_tune_cache_locked(ModelShared& shared);        // net_tune.cpp: DC_TUNE_CACHE file -> table (once per model)
void write_tune_cache_locked(ModelShared& shared);       // net_tune.cpp: table (united with the file) -> file, atomically

}  // namespace dc
