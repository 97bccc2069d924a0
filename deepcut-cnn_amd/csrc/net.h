// net.h — graph runtime of the DeeperCut forward path: the MI355X-native counterpart of
// caffe::Net / caffe::Layer / caffe::Blob / caffe::SyncedMemory / caffe::Caffe for the TEST-phase
// forward of models/deepercut/*.prototxt (reference: src/caffe/net.cpp, include/caffe/layer.hpp,
// src/caffe/blob.cpp, src/caffe/syncedmem.cpp, src/caffe/common.cpp).
//
// It is not a layer-by-layer interpreter.  Net::Init semantics (InsertSplits, in-place tops, output
// discovery, name-matched weight loading) are reproduced so that the pycaffe-visible surface is the
// reference's, but execution goes through a *lowered plan*: BatchNorm+Scale(+bias)+ReLU are folded
// into the producing convolution's epilogue, residual Eltwise adds and the Deconvolution+Crop+Eltwise
// heads are fused, activations live channels-last (NHWC) in HBM, and every convolution /
// deconvolution is one launch (4 for a stride-2 deconvolution: one per output parity class) of the
// gather-GEMM MFMA kernel in conv_gemm.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "formats.h"
#include "kernels.h"

struct dc_frame;  // include/deepcut_hip.h: one video frame (planes, pitches, format, matrix, range)
struct dc_complete_params;  // include/deepcut_hip.h: stage D of the people assembly
struct dc_dedupe_params;    // include/deepcut_hip.h: stage E of the people assembly
struct dc_draw_style;       // include/deepcut_hip.h: the skeleton overlay
struct dc_label_style;      // include/deepcut_hip.h: the label overlay
struct dc_redact_style;     // include/deepcut_hip.h: the redaction
struct dc_appearance_style; // include/deepcut_hip.h: the appearance descriptor
struct dc_track_appearance_params;  // include/deepcut_hip.h: the tracker's appearance steps
struct dc_heat_geometry;    // include/deepcut_hip.h: the score-map overlay
struct dc_heat_style;
struct dc_track_smooth_params;  // include/deepcut_hip.h: step 8 of the tracker's rule

namespace dc {

// ---- Caffe context (common.cpp:13-20: thread-local mode + device) ---------------------------------
struct Context {
  int mode = 0;     // DC_MODE_CPU (reference default, common.cpp:55,100)
  int device = 0;
  static Context& get();
};
int device_count();  // 0 without a GPU; never throws

// ---- SyncedMemory + Blob ----------------------------------------------------------------------------
enum Head { UNINITIALIZED = 0, HEAD_AT_CPU = 1, HEAD_AT_GPU = 2, SYNCED = 3 };

struct Net;
struct Tracker;
struct ModelShared;
struct Storage {
  std::vector<int> shape;  // logical Caffe shape (N,C,H,W for activations)
  float* host = nullptr;
  size_t host_cap = 0;
  bool host_pinned = false;
  unsigned char* dev = nullptr;  // NHWC image (float, _Float16 or __bf16 elements, `esize` bytes each), channel pitch cp()
  size_t dev_cap = 0;            // capacity in bytes
  int esize = 4;                 // bytes per device element (2 in fp16 and bf16 nets)
  int ekind = kElemF32;          // ElemKind of the device image
  float* stage = nullptr;  // device NCHW staging for up/download
  size_t stage_cap = 0;
  int head = UNINITIALIZED;
  bool pad4 = false;   // channel pitch rounded up to one 16-byte vector (tensors read by the gather-GEMM)
  bool is_param = false;
  bool elided = false;  // absorbed by fusion in the current plan: never materialised
  // net outputs the caller reads through host pointers after forward() (pycaffe: blobs['prob'].data): once an output was
  // downloaded on demand, the following forwards send it to the (pinned) host copy right behind the head launch, inside the
  // forward's own synchronisation — `.data` then finds it there (SYNCED) instead of paying a kernel, a copy and a stream
  // round trip per map.  An output that was NOT touched between two forwards stops being sent (next_pred is 9.1 of the
  // 10.2 MB and the demo never reads it, estimate_pose.py:104-112).
  bool host_wanted = false, host_touched = false;
  int view_of = -1;     // >= 0: this blob is channels [view_c0, view_c0+C) of storage `view_of` (merged heads)
  int view_c0 = 0, view_cp = 0;
  Net* owner = nullptr;  // activations: the net whose stream moves this blob between host and device (null: stand-alone blob)
  std::shared_ptr<ModelShared> shared;  // params: the model state a net and its clones own jointly (outlives any one of them)
  uint64_t packed_hash = 0;  // params: content hash when the filter images were last packed (see ModelShared::touched)
  bool touch_listed = false; // params: already on ModelShared::touched (an access loop must not grow the list)
  int id = -1;

  ~Storage();
  size_t count() const;
  int dim(int i) const { return i < (int)shape.size() ? shape[i] : 1; }
  int cp() const;                 // channel pitch of the device image
  size_t dev_count() const;       // elements of the device image
  void reshape(const std::vector<int>& s);  // Blob::Reshape: capacity only grows (blob.cpp:23-43)
  float* host_ptr();              // allocates + zero-fills on first touch (syncedmem.cpp:25-31)
  void ensure_dev(size_t n);  // n elements
  void* dev_at(long elem) const { return dev + elem * esize; }
  void ensure_stage(size_t n);
};

struct NetBlob {
  std::string name;
  std::shared_ptr<Storage> st;
  bool standalone = false;  // dc_blob_create: owned by the caller, moved on the default stream of the thread's device
};

// SyncedMemory::to_gpu / to_cpu (syncedmem.cpp:25-101) for a blob that may or may not belong to a net: `stream` is the
// owner's stream (null: the default stream), `base` the concatenated tensor a channel view lives in (else null)
void storage_to_device(Storage& s, void* stream);
void storage_to_host(Storage& s, void* stream, Storage* base);
void storage_download_enqueue(Storage& s, void* stream, Storage* base);  // the device -> host part of it, no wait, head untouched
void storage_mutable_device(Storage& s, void* stream);  // SyncedMemory::mutable_gpu_data: device image authoritative
// Blob::CopyFrom (blob.cpp:435-474): wherever the source is authoritative; device copies re-pitch through an NCHW stage
void storage_copy(Storage& dst, Storage& src, Storage* src_base, void* stream);

struct ConvSpec {
  int num_output = 0, kh = 1, kw = 1, sh = 1, sw = 1, ph = 0, pw = 0, dh = 1, dw = 1, group = 1;
  bool bias = true;
};

struct LayerRec {
  std::string name, type;
  std::vector<int> bottoms, tops;  // indices into Net::blobs
  TextMsg def;                     // the layer { } message
  std::vector<std::shared_ptr<NetBlob>> params;
  bool is_split = false;
  // parsed parameters
  ConvSpec conv;
  int pool_k = 1, pool_s = 1, pool_p = 0;
  float bn_eps = 1e-5f;
  bool scale_bias = false;
  float relu_slope = 0.f;
  int crop_oh = 0, crop_ow = 0;
};

// ---- lowered plan -----------------------------------------------------------------------------------
struct DevVec {  // a packed filter / affine vector; shared between a Net and its clones
  std::vector<float> host;
  bool as_half = false;  // filter image of an fp16 net: converted to _Float16 on upload
  bool as_bf16 = false;  // ... of a bf16 net: converted to __bf16 (round to nearest even) on upload
  // fp16 filter images: output channel c of the image was multiplied by an exact power of two 2^k(c) that brings its largest
  // weight into [2^13, 2^14) — filters of 1e-5 (a head on a trunk with large activations) would otherwise sit in float16's
  // subnormal range with a handful of significant bits —; row_scale[c] = 2^-k(c) goes into the launch's fp32 epilogue scale
  std::vector<float> row_scale;
  float* dev = nullptr;
  size_t uploaded = 0;
  DevVec() = default;
  DevVec(const DevVec&) = delete;
  DevVec& operator=(const DevVec&) = delete;
  ~DevVec();
};

// What a Net and its clones own JOINTLY (shared_ptr): the packed filter / affine images in HBM, the tile choices measured
// on the device, and the generation counter of the parameters.  Parameter blobs point here (not at a Net), so a blob
// obtained through one executor stays safe to touch after that executor is gone, and a parameter write reaches every
// executor: each compares `weights_gen` with the generation its plans were lowered from before it runs.
struct ModelShared {
  std::mutex mu;
  std::map<std::string, std::shared_ptr<DevVec>> vec_by_key;  // packed-weight cache (plans hold the images they use alive)
  uint64_t weights_gen = 1;   // bumped when parameter CONTENT changed (copy_from, a write through params that changed bytes)
  uint64_t packed_gen = 0;    // generation vec_by_key was packed from
  std::vector<std::weak_ptr<Storage>> touched;  // params handed out writable since the last check (Blob.data is always mutable
                                                // in pycaffe, _caffe.cpp:273: a read must not cost a 263 MB re-pack)
  std::map<std::string, int> tune_cache;        // GEMM signature -> fastest variant, one timing per process and model
  bool tune_file_loaded = false;
  std::map<std::string, std::vector<std::pair<float, int>>> tune_timings;  // signature -> (ms of a 5-launch burst, variant), sorted: pass 1 of autotune
};

struct ResampleTable {  // Pillow-style 8-bit bilinear resample of one axis: taps and 22-bit weights, on the device
  int ksize = 0;
  std::vector<int> bounds;  // host copy of [out][2] (first tap, tap count)
  int* dev_bounds = nullptr;
  int* dev_coeffs = nullptr;
  ResampleTable() = default;
  ResampleTable(const ResampleTable&) = delete;
  ResampleTable& operator=(const ResampleTable&) = delete;
  ~ResampleTable();
};
// host side of Pillow's precompute_coeffs + normalize_coeffs_8bpc (bilinear, whole-image box)
void resample_coeffs(int in_size, int out_size, int& ksize, std::vector<int>& bounds, std::vector<int>& coeffs);
// estimate_pose.py:85-88,96: canvas (stride-8) and resized-image sizes for an h x w image at `scale`
void image_canvas_size(int h, int w, double scale, int& out_h, int& out_w, int& new_h, int& new_w);
// the box entry's argument checks (Net::forward_boxes), host only: every box (x0, y0, x1, y1) non-empty and inside the h x w image,
// every scale positive, the canvas a positive multiple of 8 that holds every box's own canvas (image_canvas_size of the crop at its
// scale).  Throws DC_EINVAL naming the first box at fault.
void check_boxes(int h, int w, const int* boxes, const double* scales, int n, int canvas_h, int canvas_w);
// the frame entries' argument checks, host only: n frames of h x w (include/deepcut_hip.h, dc_frame).  Throws DC_EINVAL naming the
// field and the frame index: a NULL plane the format needs, a pitch below the minimum, an unknown format / matrix / range, a frame that
// differs from frame 0 in one of those three.
void check_frames(const char* who, const dc_frame* frames, int n, int h, int w);
// a group member's canvas in the box entry: the base canvas side times the member's pyramid scale, rounded up to the stride 8
inline int box_member_canvas(int side, double pyramid_scale) { return (int)(std::ceil((double)side * pyramid_scale / 8) * 8); }

// A tile takes K segments of `klen` elements: klen is a multiple of its K tile, and for a row-tap launch exactly one K tile.  (A row
// tap spans several adjacent pixels of a narrow input; the kernel checks a lane's tap validity at its column of the tap's FIRST K tile,
// so a later K tile of the same tap would read the pixels past the row end — the next row's, or past the tensor — as if they were inside.)
inline bool tile_takes_k(int v, int klen, bool row_tap) {
  const int bk = conv_variant_bk(v);
  return klen % bk == 0 && (!row_tap || bk == klen);
}

struct Launch {
  enum Kind { CONV, POOL, ELT, CROP } kind = CONV;
  std::string label;    // e.g. "res4b3_branch2b+bn+scale+relu"
  std::string kernel;   // variant / kernel name
  int first_layer = 0, last_layer = 0;
  int in = -1, in2 = -1, out = -1;  // storage ids (in2: residual / second operand)
  // CONV
  ConvGemmParams cg{};  // pointers filled at launch time
  int variant = 0;
  bool row_tap = false;  // one tap per kernel row over several adjacent pixels (inputs narrower than a K tile): see tile_takes_k
  std::shared_ptr<DevVec> w, scale, shift;  // packed filters / folded affine (kept alive by the plan)
  std::shared_ptr<DevVec> form_w;           // the filter image of the forms this launch can run on (kernels.h ConvForm): Winograd-transformed
                                            // filters of a 3x3 layer, the image of a streaming 1x1 layer or of the stem; else null
  std::shared_ptr<DevVec> form_w43;         // the filter image of wino_f43 (36 points, wino43_pack_filters), beside form_w on a 3x3 layer that takes both
  std::shared_ptr<DevVec> form_scale;       // the epilogue scale of a form with its own (ConvForm::own_scale: folded affine x the image's row scale x 4)
  // a form this launch can run on: the image exists, and the form serves the net's element type and takes the layer
  bool takes_form(int v) const {
    const ConvForm* f = conv_form(v);
    return f && form_w && (v != kWinoF43 || form_w43) && f->ekind == cg.ekind && cg.ncls <= 1 && (f->geometry == kForm1x1) == (cg.nty == 1 && cg.ntx == 1) &&
           (f->geometry == kFormStem) == (cg.nty == 7 && cg.ntx == 1) && f->eligible(cg);
  }
  // a tile (or form) this launch can run on: the net's element kind, the launch's K segments and deconvolution classes
  bool takes_tile(int v) const {
    if (conv_form(v)) return takes_form(v);
    return conv_variant_exists(v) && conv_variant_ekind(v) == cg.ekind && tile_takes_k(v, cg.klen, row_tap) && (cg.ncls <= 1 || conv_variant_multiclass(v));
  }
  void set_variant(int v) { variant = v, kernel = variant_kernel_label(v), grid = variant_grid(cg, v); }  // a tile or form, its label and grid
  long y_off = 0;                      // element offset of this launch's first output (deconvolution classes, channel splits)
  long w_off = 0;                      // element offset of this launch's first filter row inside `w` (channel splits)
  int c_off = 0;                       // first output channel of this launch inside scale / shift (channel splits)
  double flops = 0;                    // algorithmic 2*MAC
  long grid = 0;
  // POOL
  int pk = 0, ps = 0, pp = 0;
  // ELT
  int relu = 0, sigmoid = 0;
  // CROP
  int oh = 0, ow = 0;
};

// Everything that depends on the INPUT SHAPE: the lowered launches, which storages are views / elided, the captured
// hipGraph.  A Net keeps one per shape it has met (LRU): Layer::Forward re-derives shapes on every call
// (layer.hpp:451-456) and the demo's scale loop changes the shape on every iteration (estimate_pose.py:81-128), so a
// 4-scale pyramid must not re-lower 734 layers and re-instantiate a 160-node graph four times per image.
struct PlanState {
  std::vector<int> input_shape;
  std::vector<Launch> plan;
  double flops = 0;
  std::vector<int> views;  // storages that are channel views in this plan
  struct StorageState {
    int id, view_of, view_c0;
    bool elided;
  };
  std::vector<StorageState> sstate;                       // per-storage fusion state to restore on activation
  std::vector<std::pair<int, std::vector<int>>> aux_shapes;  // tensors created by the lowering (merged heads)
  void* graph_exec = nullptr;
  uint64_t graph_buf_gen = 0;  // Net::buf_gen_ when the graph was captured (a reallocated buffer makes it stale)
  bool tuned = false;
  uint64_t last_use = 0;
};

struct NetStats {  // dc_net_stats
  long long lowerings = 0, graph_instantiations = 0, plan_hits = 0, autotune_runs = 0, buffer_growths = 0, repacks = 0, sparse_packs = 0;
};

// The grow-only device buffer of the host code (runtime.cpp): every scratch, staging and table buffer of a Net and a NetGroup is one.
// Not one, on purpose: Storage (the head state of a SyncedMemory, zero fill, buffer_growths), the Tracker's per-image scratch (sized in
// images; allocates before it frees, after waiting for its event) and Comm::grow_dev (switches devices, shares Buf with pinned memory).
struct DevBuf {
  unsigned char* dev = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf();
  // at least `bytes`; the contents do not survive a growth.  -> whether it reallocated.  A failed allocation throws and leaves the
  // buffer empty (dev null, cap 0): the next call allocates again, never works on a null pointer
  bool reserve(size_t bytes);
  void* get(size_t bytes) { return reserve(bytes), dev; }
};

// Stage D of the people assembly (dc_complete_params, include/deepcut_hip.h): state of a net or a group, not an argument of the entries
struct CompleteParams {
  int enabled = 0;
  float fill_threshold = 0.f;
  int fill_radius = 0, min_support = 0;
  // DC_EINVAL naming the field; host only.  A null pointer is "off"
  static CompleteParams checked(const dc_complete_params* p);
};

// Stage E of the people assembly (dc_dedupe_params, include/deepcut_hip.h): state of a net or a group like CompleteParams
struct DedupeParams {
  int enabled = 0;
  double max_dist = 0.0, min_size = 0.0;
  int min_common = 0, n_sigma = 0, absorb = 0;
  double sigma[kPeopleMaxJoints] = {};  // the first n_sigma are the caller's; n_sigma == 0: all 1.0
  // DC_EINVAL naming the field; host only.  A null pointer is "off", and so is enabled == 0 unless `always` (dc_dedupe_people, which
  // has no use for a switch)
  static DedupeParams checked(const dc_dedupe_params* p, const char* who, bool always = false);
  // DC_ESHAPE for an n_sigma that is neither 0 nor J and for min_common > J: what only a call that knows the joints can refuse
  void check_joints(const char* who, int J) const;
  const double* sigma_or_null() const { return n_sigma ? sigma : nullptr; }
};
// dc_dedupe_people (people.cpp): stage E alone on host arrays, synchronous
void dedupe_people(const dc_dedupe_params* params, int nb, int P, int J, const int* n_people, const double* people, const int* cand,
                   int* n_out, double* people_out, int* cand_out, int* kept_from, int* suppressed_by);
// dc_draw_people / dc_draw_limits (draw.cpp): skeletons blended into frames in place on the device, synchronous
void draw_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                 const int* cand, const long long* ids, const dc_draw_style* style, void* stream);
void draw_limits(int* tile_w, int* tile_h, int* chunk);
// dc_label_people / dc_label_font (label.cpp): people's ids as text on a plate, in place on the device, synchronous
void label_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                  const long long* ids, const char* texts, const dc_label_style* style, void* stream);
void label_font(int ch, unsigned char* rows);
// The overlays of dc_overlay_people_device / dc_net_track_frames_async_overlay: either style or both (redaction first), the id lists
// of the redaction (n < 0: no such list) and where `redacted` [nb][P] goes (may be null) — device memory for the stand-alone entry,
// the caller's host array for the chain
struct OverlayArgs {
  const dc_draw_style* draw = nullptr;
  const dc_redact_style* redact = nullptr;
  const long long* only_ids = nullptr;
  int n_only = -1;
  const long long* keep_ids = nullptr;
  int n_keep = -1;
  int* redacted = nullptr;
  const dc_label_style* labels = nullptr;  // the labels, written last (dc_overlay_styles)
  bool styles_entry = false;               // the call came through a `_styles` entry, which takes a label style too: the refusal says so
  bool any() const { return draw || redact || labels; }
};
// dc_overlay_people_device (overlay.cpp): the bytes of redact_people then draw_people from people, cand and ids in DEVICE memory, the
// primitives and the tile selection made on the device.  Asynchronous on a caller's stream with device frames, else it waits
void overlay_people_device(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* d_n_people,
                           const double* d_people, const int* d_cand, const long long* d_ids, const OverlayArgs& overlay, void* stream);

// dc_redact_people (redact.cpp): regions derived from people's joints replaced by a mosaic or a colour, in place on the device, synchronous
void redact_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                   const unsigned char* select, const dc_redact_style* style, int* redacted, void* stream);
// dc_describe_people (appearance.cpp): per person, 3 x 16-bin histograms of the frame bytes under the capsules of `style->edges`, counted
// on the device; frames are only read.  desc: host [nb][P][3][16], all of it written.  Synchronous
void describe_people(const dc_frame* frames, int nb, int h, int w, bool is_device, int P, int J, const int* n_people, const double* people,
                     const dc_appearance_style* style, int* desc, void* stream);
// dc_draw_heatmap (heat.cpp): a float32 NCHW score map, host or device, blended into frames in place on the device, synchronous
void draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const float* map, bool map_is_device, int C, int Hm, int Wm,
                  const dc_heat_geometry* geometry, const dc_heat_style* style, void* stream);

// What the assembly calls behind its last stage with the device arrays it left (n_people, people, cand): the tracker's launch.  True:
// the hook has delivered `people` and `cand` to the host arrays itself (a tracker with smoothing on), and the assembly downloads neither.
using AfterPeople = std::function<bool(const int* d_np, const double* d_ppl, const int* d_cand)>;

struct Net {
  std::string name;
  int phase = 1;
  std::vector<LayerRec> layers;  // after InsertSplits
  std::vector<std::shared_ptr<NetBlob>> blobs;
  std::map<std::string, int> blob_index;
  std::vector<std::shared_ptr<Storage>> storages;
  std::vector<int> inputs, outputs;  // blob indices

  int fuse = 2;
  int dtype = 0;  // ElemKind of activations / filters: 0 float; 1 _Float16, 2 __bf16 (fp32 accumulate + epilogue in both)
  int use_graph = 0;
  int outputs_mask = -1;  // DC_OPT_OUTPUTS: bit i = output i (order of `outputs`) is wanted
  int sparse_pairwise = 0;  // DC_OPT_SPARSE_PAIRWISE: a plan without next_pred has the pairwise head evaluated at the cells its consumers read
  CompleteParams completion;  // dc_net_set_completion: stage D behind every assembly of this net (off by default; a clone copies it)
  DedupeParams dedupe;        // dc_net_set_dedupe: stage E behind stage D (or C), likewise
  std::shared_ptr<ModelShared> shared;   // joint with every clone
  uint64_t seen_weights_gen = 0;         // generation the cached plans were lowered from
  // the ACTIVE plan (the fields below are swapped with a parked PlanState when the input shape changes)
  bool plan_valid = false;
  std::vector<int> plan_input_shape;
  std::vector<Launch> plan;
  std::vector<int> plan_views_;          // storages that are channel views in the current plan
  double plan_flops = 0;
  void* graph_exec = nullptr;
  uint64_t graph_buf_gen = 0;
  bool tuned = false;                    // tile variants of the current plan were timed on the device
  std::vector<std::unique_ptr<PlanState>> parked_;  // plans of the other shapes met so far (LRU, DC_PLAN_CACHE entries)
  uint64_t use_clock_ = 0, cur_last_use_ = 0;
  uint64_t buf_gen_ = 1;                 // bumped whenever a device buffer of this net is reallocated
  uint64_t tile_gen_ = 1;                // bumped whenever a launch of the active plan changes its tile (autotune, set_tile): a
                                         // NetGroup that captured this member's launches in ITS graph re-merges
  NetStats stats;
  std::map<std::string, int> aux_index_; // concatenated-head tensors created by the lowering
  void* stream = nullptr;
  bool stream_borrowed_ = false;  // `stream` belongs to the process-wide executor pool (streams.cpp): never destroyed with the net
  int device = -1;
  DevBuf pose_dev;  // the poses of a decode on their way to a host destination (decode_to)
  std::string text_buf;
  std::string proto_text;  // kept for clone()

  ~Net();
  static Net* create(const std::string& prototxt_text, int phase, const Net* clone_of = nullptr);
  Net* clone();           // same graph and input shape, SHARED parameters and packed device weights
  void synchronize();     // wait for everything enqueued on the net's own stream
  // streams.cpp: the executors' own streams chosen by timing their forwards on candidate assignments (hardware-queue sharing decides
  // what "in flight" is worth and the API does not say which queue a stream got)
  static void choose_streams(const std::vector<Net*>& nets, int ncand, int reps, double* rate_chosen, double* rate_first);
  void adopt_stream(void* s);  // a pool stream becomes the net's own
  void* own_stream();          // the net's own stream, created on first use
  void set_dtype(int d);  // 0 float32 / 1 float16 / 2 bfloat16 device images (DC_OPT_DTYPE)
  void set_outputs_mask(int mask);  // DC_OPT_OUTPUTS
  void set_sparse_pairwise(int v);  // DC_OPT_SPARSE_PAIRWISE (sparse_pairwise.cpp): DC_EUNSUP on a net without a recognisable pairwise head
  void copy_from(const std::string& path);
  void save(const std::string& path);
  void reshape();         // propagate input shapes through every layer (Net::Reshape)
  void build_plan();      // lower to launches for the current shapes (host only; no device needed)
  void ensure_plan();     // make the plan of the current input shape the active one: cache hit, or build_plan()
  void invalidate_plans();  // drop every cached plan and graph (option / weight change)
  void mark_weights_changed();  // parameter content changed: every executor re-packs and re-lowers before its next run
  void reserve(int n, int h, int w);  // lower + allocate + tune for a shape without running it
  void prepare_to_run();              // the same for the current input shape (no reshape)
  // one reference layer stand-alone (Layer<Dtype>::SetUp on given bottoms): a net whose inputs are the layer's bottoms
  static Net* create_for_layer(const std::string& layer_text, int phase, const std::vector<std::vector<int>>& bottom_shapes);
  void forward(int start, int end);
  // host_async (host buffers only): nothing is waited for — the upload, the forward and the downloads are enqueued on the net's own
  // stream and the caller collects with synchronize(); truly asynchronous for pinned buffers (dc_host_alloc), staged by the runtime otherwise
  void forward_batch(const float* input, int n, int h, int w, bool is_device, float* prob, float* loc,
                     float* next, void* user_stream, bool host_async = false);
  // the same from n separate HOST images (one pointer each; pinned memory: the DMA engines read them in place), asynchronous on the
  // net's own stream — what dc_forward_batch uses when the caller's arrays are pinned: no staging copy on the host
  void forward_host_images(const float* const* inputs, int n, int h, int w);
  // cross-request batching: n independent single-image requests (device buffers, one pointer set per request) as ONE batch-n forward
  void forward_requests(int n, const float* const* inputs, int h, int w, float* const* prob, float* const* loc, float* const* next,
                        void* user_stream);
  // image entry: pre-processing (estimate_pose.py:83-103) + forward + optional decode, all on the device
  // frames (dc_net_forward_frames): n video frames instead of `bgr`, which is then not read; the same call in every other respect
  void forward_images(const unsigned char* bgr, int n, int h, int w, double scale, bool is_device, float* prob, float* loc,
                      float* next, double* pose, void* user_stream, const dc_frame* frames = nullptr);
  // box entry: n person boxes of ONE h x w image (boxes: n x 4 int32 (x0, y0, x1, y1), half-open; scales: n doubles; both host
  // arrays), box i pre-processed at scales[i] as an image of its own onto a common canvas_h x canvas_w canvas, ONE batch-n forward,
  // pose i decoded on its own canvas's cells at scales[i] and shifted by (x0, y0) into image coordinates.  n = 0 does nothing.
  // frame (dc_net_forward_boxes_frame): ONE video frame instead of `bgr`
  void forward_boxes(const unsigned char* bgr, int h, int w, bool is_device, const int* boxes, const double* scales, int n, int canvas_h,
                     int canvas_w, float* prob, float* loc, float* next, double* pose, void* user_stream, const dc_frame* frame = nullptr);
  void sync_to_host(Storage& s);       // SyncedMemory::to_cpu
  void sync_to_device(Storage& s);     // SyncedMemory::to_gpu
  void decode_pose(double scale, double* out, bool is_device, void* user_stream);  // after a forward
  // the maps of the last forward as NCHW float32 (elem 0) or float16 (elem 1, fp16 nets), host or device destination
  void emit_last_maps(void* prob, void* loc, void* next, int elem, bool is_device, void* user_stream);
  // multi-person consumers of the maps of the last forward (encoding: pose_data_layer.cpp:686-802)
  void detect_parts(double scale, float thr, int radius, int max_det, int* counts, double* dets);
  // `prob` of the last forward blended into nb frames in place (dc_net_draw_heatmap; heat.cpp), on the net's stream, waited for
  void draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const dc_heat_geometry* geometry, const dc_heat_style* style);
  void decode_pairwise(double scale, int ndet, const int* det, const double* mean, const double* stdev, double* out);
  // the raw next_pred values at ndet (image, row, col) cells -> out [ndet][C] float32 (dc_net_pairwise_at): from the dense map when the plan
  // has it, by the sparse head otherwise
  void pairwise_at(int ndet, const int* det, float* out);
  // the people of every image of the last forward: candidates (part_select), pair costs and greedy assembly (people.cpp / people.hip)
  // back to back on the device, only the results travel (dc_net_assemble_people; the grouping rule is this project's own)
  struct AssembleParams {
    double scale;
    float threshold;
    int radius, max_det;
    double max_cost;
    float seed_threshold;
    int max_people, min_joints;
    CompleteParams complete{};  // what assemble_maps runs behind stage C: the net's or the group's setting, put there by assemble_last /
                                // NetGroup::assemble_people (the entries leave it off)
    DedupeParams dedupe{};      // likewise stage E, behind stage D (or stage C when completion is off)
  };
  // tracker (may be null; dc_net_track_people): its launch runs behind the assembly's on the people left on the device -> ids, place
  // [NB][max_people]; everything else is computed and returned exactly as without it.  slot_of (may be null: image b updates slot b):
  // [NB], the slot every image updates (dc_net_track_people_slots)
  void assemble_people(const AssembleParams& p, int n_edges, const int* edges, const double* mean, const double* stdev, const int* joint_order,
                       int* n_people, double* people, int* cand, double* cost, Tracker* tracker = nullptr, long long* ids = nullptr,
                       int* place = nullptr, const int* slot_of = nullptr);
  // The whole video chain on the net's own stream with no host wait (dc_net_track_frames_async): upload of host planes, pre-processing,
  // the plan, candidates, (sparse head,) pair costs, assembly, the tracker's launch (tracker may be null: people without ids) and the
  // downloads.  Every argument check runs before any device work, in the order forward_images / assemble_people / Tracker::check_call
  // make them; everything small is copied before the return; frame planes and output arrays stay the caller's until synchronize().
  void track_frames_async(Tracker* tracker, const dc_frame* frames, const unsigned char* bgr, int n, int h, int w, double scale, bool is_device,
                          const int* slot_of, const AssembleParams& p, int n_edges, const int* edges, const double* mean, const double* stdev,
                          const int* joint_order, int* n_people, double* people, int* cand, long long* ids, int* place,
                          const OverlayArgs* overlay = nullptr);
  // ... with `overlay` (dc_net_track_frames_async_overlay) the frames are redacted and drawn into behind the tracker, from the people,
  // cand and ids where the chain left them on the device: the builders in front of the tracker's event (they read its scratch), the tile
  // kernels behind it, on the planes frame_source staged for host frames, which then travel back; overlay->redacted is a host array
  // front half of forward_images: the uint8 pixels -> the network's NHWC input image, enqueued on s (the plan of the canvas
  // shape is active afterwards); returns the canvas height / width
  // mirror: the images are read flipped left to right (ImagePrepParams::mirror; NetGroup::forward_images hands it down)
  // frames (already checked): n video frames instead of `bgr`, read by the kernels' frame reader through the per-image plane table;
  // host frames are staged first (stage_frames), device frames read where they are
  void prep_images(const unsigned char* bgr, int n, int h, int w, double scale, bool is_device, void* s, bool mirror = false,
                   const dc_frame* frames = nullptr);
  // front half of forward_boxes (arguments already checked): the boxes' canvases in ONE launch, and the per-box decode table;
  // returns the device copy of the image the launch reads (a host image is uploaded once)
  // mirror: every crop is read flipped left to right (BoxPrepParams::mirror; NetGroup::forward_boxes hands it down), and the member
  // remembers that its last box batch was (box_mirror_)
  // frame (already checked): ONE video frame instead of `bgr`; a host frame is staged (staged_planes() is its device copy); returns null
  const unsigned char* prep_boxes(const unsigned char* bgr, int h, int w, bool is_device, const int* boxes, const double* scales, int n,
                                  int canvas_h, int canvas_w, void* s, bool mirror = false, const dc_frame* frame = nullptr);
  // the device copies of the host frames of the last prep_images / prep_boxes (planes in the net's image buffer, pitch padding dropped):
  // what a group hands to the other members that share those frames, so that they travel once
  const std::vector<FramePlanes>& staged_planes() const { return frame_host_; }
  // back half: the poses of the boxes of the last prep_boxes, in image coordinates (host or device `out`, n x 5 x J doubles)
  void decode_boxes(double* out, bool is_device, void* s);
  std::string plan_text();
  std::string profile_text(int iters);
  std::string tune_report_text();  // per GEMM signature of the current plan: tile in use, launches, the isolated timings of autotune
  void set_tile(const std::string& key, const std::string& tile);  // override the tile of one signature (tuning under the caller's own load)
  std::string debug_info_text();  // Net::ForwardDebugInfo (net.cpp:648-681): mean |x| of every top / parameter blob
  int layer_index(const std::string& name) const;

 private:
  friend struct NetGroup;
  void init_from(const TextMsg& root);
  void setup_layer(LayerRec& L);
  void reshape_layer(LayerRec& L);
  void ensure_device();
  void upload_vecs();
  friend void prepare_wino43(Net& n, bool& grew);
  void run_launch(const Launch& l, void* s);
  void run_plan(int start, int end, void* s);
  const Net* clone_src_ = nullptr;  // during create() of a clone only
  void release_graph();
  void check_weights();   // compare the shared weight generation / touched parameters with what the plans were built from
  void park_current();
  void autotune();
  std::string tune_key(const Launch& l) const;
  Storage& begin_batch(int n, int h, int w);
  void enqueue_plan(void* s);
  void emit_maps(void* prob, void* loc, void* next, bool is_device, void* s, int dst_esize = 4);
  std::shared_ptr<ResampleTable> resample_table(int in_size, int out_size);
  std::map<std::pair<int, int>, std::shared_ptr<ResampleTable>> resample_;
  struct MapRef {
    const void* ptr;
    int cp, c0, es, ek, NB, C, H, W;
  };
  MapRef map_ref(const char* blob_name);  // device image of an output map (channel views of the merged heads included)
  const std::vector<int>& prob_shape() const;  // (NB, J, H, W) of `prob`, host only: DC_EINVAL without the blob, DC_ESHAPE unless 4-D
  // the device half of detect_parts, shared with NetGroup::detect_parts (net_image.cpp): the scratch carved, launch_part_select on the
  // maps given by reference, the two downloads, and the wait for `stream`
  static void select_parts(const MapRef& P, const MapRef& L, float thr, int radius, double scale, int max_det,
                           const std::function<void*(size_t)>& scratch, void* stream, int* counts, double* dets);
  // assemble_people in three parts, shared with NetGroup::assemble_people (people.cpp): the checks of the parameters, the checks of the
  // edges / statistics / joint order against J joints (-> the lookup table lut[a*J + c] followed by the joint order), both host only,
  // and the device half: the three launches on maps given by reference, scratch memory from `scratch(bytes)`, everything on `stream`
  static void check_assemble_params(const AssembleParams& q);
  static std::vector<int> check_assemble_graph(const AssembleParams& q, int J, int n_edges, const int* edges, const double* mean,
                                               const double* stdev, const int* joint_order);
  // between (may be empty): called with stage A's device outputs (counts, dets) after its launch and before stage B's — the sparse
  // pairwise head fills N's cells there.  after (may be empty): called with stage C's device outputs (n_people, people) behind its
  // launch — and behind stage D's when q.complete is enabled, on the completed people, and stage E's when q.dedupe is, on the people it
  // kept — and before the downloads — the tracker's launch goes there
  // keep (may be null: the table and the statistics go into the scratch with every call): where they stay on the device from call to call,
  // uploaded only when their content differs from what is there, from a host copy that outlives the upload.  wait = false: nothing is
  // waited for — the results are in the host arrays once `stream` has been, and nothing of the caller's small arguments is read after
  // the return (keep is needed then)
  struct AssembleTables {
    DevBuf buf;
    std::vector<unsigned char> host;  // lookup table and joint order (ints), then mean and standard deviation (doubles)
    void* stream = nullptr;           // the stream the upload ran on
  };
  static void assemble_maps(const MapRef& P, const MapRef& L, const MapRef& N, const AssembleParams& q, const std::vector<int>& table,
                            int n_edges, const double* mean, const double* stdev, const std::function<void*(size_t)>& scratch, void* stream,
                            int* n_people, double* people, int* cand, double* cost,
                            const std::function<void(const int*, const double*)>& between = nullptr,
                            const AfterPeople& after = nullptr, AssembleTables* keep = nullptr,
                            bool wait = true);
  AssembleTables asm_tables_;
  void assemble_last(const AssembleParams& q_in, const std::vector<int>& table, int n_edges, const double* mean, const double* stdev,
                     int* n_people, double* people, int* cand, double* cost, const AfterPeople& after,
                     bool wait);
  // DC_OPT_SPARSE_PAIRWISE (sparse_pairwise.cpp)
  struct PairHead {
    int elt = -1, conv = -1, crop = -1, deconv = -1;  // layer indices: the Eltwise SUM, its 1x1 Convolution, its Crop and the Crop's Deconvolution
  };
  PairHead find_pair_head() const;
  bool next_in_plan() const;  // the current plan computes next_pred (as a tensor of its own or a view of the merged heads)
  struct SparseNext {
    MapRef N;          // the float32 scratch map [NB][H][W][C]: defined at the cells the head was run at
    SparseHeadArgs a;
    int ekind;         // element type of the head's inputs
    int* work;         // class lists (launch_sparse_head)
    int* cells;        // room for the (image, row, col) triples
  };
  SparseNext sparse_next(int nslots, int ntriples);   // inputs, packed filters and scratch; nothing launched
  SparseNext sparse_next_at(int ndet, const int* det);  // ... and the head run at ndet host triples
  void refresh_pack_cache();  // caller holds shared->mu: the packed-image cache emptied when the parameters changed since it was filled
  std::shared_ptr<DevVec> sparse_w_, sparse_b_;  // the head's filter image and bias (kept alive here as a plan keeps its launches')
  DevBuf sparse_dev_;
  // V and M of the wino_f43 launches (kernels.h wino43_workspace_bytes): sized for the largest such launch of the plan when the buffers of a
  // plan are prepared, before any forward or capture; grown (buf_gen_ bumped) but never shrunk or freed while the net lives; a clone has its own
  DevBuf wino43_dev_;
  DevBuf scratch_dev_;  // candidates / detections / pairwise scratch
  void* scratch(size_t bytes) { return scratch_dev_.get(bytes); }
  DevBuf img_dev_;  // uint8 source images uploaded from the host
  DevBuf overlay_dev_;  // the overlays of track_frames_async: OverlayPlan's block (net_internal.h)
  const unsigned char* upload_image(const unsigned char* host, size_t bytes, void* s);  // -> the device copy in img_dev_, enqueued on s
  DevBuf frame_dev_;   // frame entries: FramePlanes[n], the frame readers' plane table
  std::vector<FramePlanes> frame_host_;  // the host side of that table (device addresses): uploaded only when it differs from what is there
  void* frame_stream_ = nullptr;         // ... and the stream that upload ran on
  // n checked frames of h x w -> the frame readers' source: host planes staged into img_dev_ (one 2-D copy per plane on s), the plane
  // table uploaded when it differs from the one on the device, the conversion's coefficients
  FrameSource frame_source(const dc_frame* frames, int n, int h, int w, bool is_device, void* s);
  DevBuf tmp_dev_;  // horizontally resampled rows
  DevBuf box_dev_;  // box entry: BoxPrepItem[n] then PoseDecodeItem[n] (net_internal.h box_decode_offset / box_table_bytes)
  std::vector<unsigned char> box_host_;  // the host side of that table (outlives its upload)
  int box_n_ = 0;                     // boxes of the last prep_boxes
  bool box_mirror_ = false;           // ... and whether it read them flipped left to right
};

// ---- tracking people from frame to frame (track.cpp / track.hip; the rule: include/deepcut_hip.h, dc_tracker_update) ---------------
// The tracks of `slots` independent sequences in one device allocation, made, zeroed and bound to a device at the first update:
//   slot blocks (kernels.h TrackSlot) | sigma^2 [J]
// and the per-image scratch in a second one, sized for the largest image count of a call so far (at least `slots`):
//   distances [cap][T][256] | staging of host poses: n_people [cap], people [cap][256][J][3] | outputs: ids [cap][256], place [cap][256]
//   and, once smoothing has been on: step 8's outputs smooth [cap][256][J][3], src [cap][256][J], cand [cap][256][J]
// It grows on demand; the contents do not survive that and need not: every call fills what it reads.  The filters of step 8 are a third
// allocation, [slots][T][J] TrackFilter, made at the first update with smoothing on.
// Order: the tracker holds an event.  Every enqueue of an update — under the runtime lock, which is held for the enqueue only — makes its
// stream wait for the event of the update enqueued before it (hipStreamWaitEvent: no host wait) and records the event again behind its
// own launch and the copies out of the shared scratch.  Updates therefore apply in the order of the host calls that enqueued them,
// whichever net, clone or stream carried them, and an asynchronous entry (Net::track_frames_async) need not wait for anything.  The
// synchronous calls (update, state, reset, the destructor, the synchronous track_people entries) wait for the event on the host first.
struct Tracker {
  TrackParams tp{};
  int slots = 0;
  std::vector<double> sig2;
  int device = -1;  // bound at the first update
  unsigned char* dev = nullptr;
  size_t slot_stride = 0, off_sig = 0, total = 0;
  void* done = nullptr;              // hipEvent_t: behind the last update enqueued (made with the device buffer)
  unsigned char* img_dev = nullptr;  // the per-image scratch ...
  int img_cap = 0;                   // ... and how many images it holds
  size_t off_dist = 0, off_np = 0, off_ppl = 0, off_ids = 0, off_place = 0;
  // step 8 (dc_tracker_set_smoothing).  The filters [slots][T][J] (kernels.h TrackFilter) are an allocation of their own, made at the
  // first update with smoothing on and zeroed there and at the first update after smoothing went from off to on (filt_clear).  The
  // scratch then also holds the outputs smooth [cap][256][J][3], src and cand [cap][256][J] (img_smooth), which the enqueue downloads
  // BEFORE it records the event: the next update's launch waits for that event, so it cannot overwrite what has not been copied out.
  struct SmoothParams {
    int enabled = 0;
    double min_cutoff = 0.0, beta = 0.0, d_cutoff = 0.0;
    int max_hold = 0;
  } smooth;
  unsigned char* filt_dev = nullptr;
  bool filt_clear = false, img_smooth = false;
  size_t off_smooth = 0, off_src = 0, off_cand = 0;
  struct SmoothOut {  // where an enqueue delivers step 8 (host arrays, any may be null); d_cand: the assembly's, on the device, or null
    double* people = nullptr;
    int* src = nullptr;
    const int* d_cand = nullptr;
    int* cand = nullptr;
  };
  // the appearance steps (dc_tracker_set_appearance).  The models and galleries [slots] (kernels.h TrackAppearSlot) are an allocation of
  // their own, made at the first update with appearance on and zeroed there and at the first update after it went from off to on
  // (app_clear).  The scratch then also holds desc and qdesc [cap][256][48] and reid [cap][256] (img_appear); reid is downloaded in front
  // of the event like step 8's outputs.
  struct AppearParams {
    int enabled = 0, min_pixels = 0, alpha256 = 0, reid_max = 0, max_age = 0, min_hits = 0;
  } appear;
  unsigned char* app_dev = nullptr;
  size_t app_stride = 0;
  bool app_clear = false, img_appear = false;
  size_t off_desc = 0, off_qdesc = 0, off_reid = 0;
  // every argument error is DC_EINVAL naming the parameter; no device is needed
  static Tracker* create(int slots, int max_tracks, int n_joints, const double* sigma, int max_misses, int min_common, double max_dist,
                         double min_size, int motion);
  ~Tracker();
  Tracker() = default;
  Tracker(const Tracker&) = delete;
  Tracker& operator=(const Tracker&) = delete;
  // host only: nb images of at most P people with J joints fit this tracker (DC_EINVAL / DC_ESHAPE naming what does not).  slot_of
  // null: image b updates slot b, nb <= slots; else nb <= 64 images, image b updates slot slot_of[b], each in [0, slots)
  void check_call(const char* who, int nb, int P, int J, const int* slot_of = nullptr) const;
  // host wait for the last update enqueued (nothing enqueued yet: returns at once); the caller is on the tracker's device
  void wait_done();
  // the caller holds the runtime lock; `on_device` is the current device.  Binds / checks the device, allocates at the first use and
  // makes room for nb images, waiting for the tracker's work in flight before the scratch is replaced
  void prepare(int on_device, int nb, void* stream);
  // ... and, after prepare, still under the lock: `stream` waits for the update before, then the launch on d_np / d_ppl (slot_of checked,
  // or null) and the downloads of ids / place / dist (any null), then the event is recorded.  No host wait.
  // With smoothing on step 8 runs in the same launch, and `so` (may be null) says where its results go.
  // before_done (may be null): called behind the launch and IN FRONT OF the event's record with what the update left in the shared
  // scratch — the people (step 8's with smoothing on, else d_ppl), cand (step 8's cand_out with smoothing on, null when it made none;
  // else `d_cand`) and the ids.  Whatever it enqueues on `stream` reads the scratch before the next update may overwrite it.
  using BeforeDone = std::function<void(const double* d_people, const int* d_cand, const long long* d_ids)>;
  // With appearance on its steps run in the same launch: d_desc (device [nb][P][48], null: nobody has a valid descriptor) and where
  // reid goes (host, may be null).
  void enqueue(int nb, int P, const int* slot_of, const int* d_np, const double* d_ppl, long long* ids, int* place, double* dist, void* stream,
               const SmoothOut* so = nullptr, const BeforeDone* before_done = nullptr, const int* d_cand = nullptr, const int* d_desc = nullptr,
               int* reid = nullptr);
  // with_appearance: dc_tracker_update_appearance (DC_EINVAL when appearance is off); desc: host [nb][P][48] or null
  void update(int nb, int P, const int* slot_of, const int* n_people, const double* people, long long* ids, int* place, double* dist,
              double* smooth_out = nullptr, int* src = nullptr, bool smoothed = false, bool with_appearance = false, const int* desc = nullptr,
              int* reid = nullptr);
  // host only, ordered like set_smoothing; null: off.  Off -> on starts with empty models and gallery, a change while on keeps them
  void set_appearance(const dc_track_appearance_params* p);
  void appearance_state(int slot, int* track_model, int* track_valid, long long* gallery_ids, int* gallery_age, int* gallery_model);
  // host only, ordered like set_option; null: off.  Off -> on starts with empty filters, a change while on keeps them
  void set_smoothing(const dc_track_smooth_params* p);
  void smooth_state(int slot, double* poses, int* gap);
  // for the chained entries' `after` hook: enqueue, and with smoothing on deliver people / cand from step 8 -> true (the caller then
  // downloads neither itself)
  bool enqueue_chained(int nb, int P, const int* slot_of, const int* d_np, const double* d_ppl, const int* d_cand, long long* ids, int* place,
                       double* people, int* cand, void* stream, const BeforeDone* before_done = nullptr);
  void reset(int slot);  // -1: all
  // DC_TRACK_OPT_*: host only (no device needed); set waits for the last update enqueued, then stores: later updates use the value
  void set_option(int key, int value);
  int get_option(int key) const;
  void state(int slot, long long* ids, int* misses, int* hits, double* poses);
};

// ---- pyramid-grouped execution (round 4) ---------------------------------------------------------------------------------
// The demo runs the scales of an image pyramid one forward after the other (python/pose/estimate_pose.py:81-128), the
// reference one SGEMM per image and layer (base_conv_layer.cpp:326-341): four launches per layer over the SAME filters, each
// starting on L2s that hold neither its filters nor its input, each with its own dispatch ramp and tail.  A NetGroup runs
// several executors of ONE model (a net and its clones, each at its own input shape) as ONE launch sequence: launch i of
// the group is launch i of every member's plan merged into a multi-problem gather-GEMM (kernels.h ConvProblem) — the
// residue classes of the deconvolution heads become problems too —, so a 4-scale pyramid is 161 launches (one lane) or 318 (the default two
// concurrent lanes of two scales, GroupPlan::lane_members) instead of 632.
// Members keep their blobs, plans and tile choices: a member can still be run alone.  Launches that cannot merge (a member on a
// form that does not merge, max-pool, stand-alone element-wise layers) run member by member inside the same sequence.
struct GroupLaunch {
  bool multi = false;
  int lane = 0;               // which lane of the plan runs it (GroupPlan::lane_members)
  int index = 0;              // index into every member's plan
  int member = -1;            // !multi: the member whose launch `index` this is
  ConvGemmParams p{};         // multi: the layer's common block (not yet prepared for a variant)
  bool row_tap = false;       // ... a row-tap layer (Launch::row_tap)
  int form = -1;              // ... the multi-problem form every member can run on (ConvForm::launch_multi), else -1,
  const void* form_w = nullptr; // ... and the members' shared image of it (read instead of p.w on that form)
  ConvMultiTable table{};     // ... and the problems (pointers filled, not yet prepared)
  ConvMultiArgs args{};       // both, prepared for `variant`: the kernel arguments
  int nprob = 0;
  int variant = -1;
  long grid = 0;
  std::string key, label;
  double flops = 0;
  std::vector<int> prob_member;  // per problem: the member it belongs to (diagnostics)
};
struct GroupPlan {
  std::vector<std::vector<int>> shapes;   // per member: its input shape
  std::vector<uint64_t> lowerings, buf_gens, weight_gens, tile_gens;  // per member, when the plan was merged
  std::vector<GroupLaunch> launches;
  int nlanes = 1;
  std::vector<std::vector<int>> lane_members;  // per lane: member indices (ascending)
  std::vector<void*> lane_graphs;              // per lane: the captured hipGraphExec, or null
  bool tuned = false;
  uint64_t last_use = 0;
  double flops = 0;
  void drop_graphs();
};
struct GroupStats {
  long long merges = 0, graph_instantiations = 0, autotune_runs = 0, plan_hits = 0;
};
struct NetGroup {
  std::vector<Net*> nets;  // borrowed: executors of one model (a net and its clones), alive as long as the group
  CompleteParams completion;  // dc_group_set_completion: stage D behind the assembly of the fused maps (the members' settings are not read)
  DedupeParams dedupe;        // dc_group_set_dedupe: stage E likewise
  GroupStats stats;
  std::string text_buf;
  ~NetGroup();
  static NetGroup* create(const std::vector<Net*>& members);
  // one batch per member (member c gets inputs[c] of n[c] x 3 x h[c] x w[c]); pointers as Net::forward_batch
  void forward_batch(const float* const* inputs, const int* n, const int* h, const int* w, bool is_device, float* const* prob,
                     float* const* loc, float* const* next, void* user_stream);
  // image entry: member c pre-processes n[c] images of h[c] x w[c] at scale[c] (Net::forward_images), then ONE grouped
  // forward, then per member the maps / the decoded pose.  mirror (dc_group_forward_images_mirrored): [M] 0/1, null = none; a mirrored
  // member pre-processes its images flipped left to right and returns its raw maps, in the flipped image's frame
  // frames (dc_group_forward_frames): frames[c] = member c's n[c] video frames instead of bgr[c]; host frames that several members share
  // are staged once
  void forward_images(const unsigned char* const* bgr, const int* n, const int* h, const int* w, const double* scale, bool is_device,
                      float* const* prob, float* const* loc, float* const* next, double* const* pose, void* user_stream,
                      const int* mirror = nullptr, const dc_frame* const* frames = nullptr);
  // box entry (Net::forward_boxes): member c takes every box at scales[i] * pyramid[c] on a canvas of box_member_canvas(canvas_h / w,
  // pyramid[c]); the image is uploaded once, each member pre-processes its boxes in one launch, then ONE grouped forward.
  // mirror (dc_group_forward_boxes_mirrored): [M] 0/1, null = none; a marked member pre-processes every crop flipped left to right
  // frame (dc_group_forward_boxes_frame): ONE video frame instead of `bgr`, staged once when it is host memory
  void forward_boxes(const unsigned char* bgr, int h, int w, bool is_device, const int* boxes, const double* scales, int n,
                     const double* pyramid, int canvas_h, int canvas_w, float* const* prob, float* const* loc, float* const* next,
                     double* const* pose, void* user_stream, const int* mirror = nullptr, const dc_frame* frame = nullptr);
  // Multi-scale fusion (dc_group_fuse_maps; the rule: include/deepcut_hip.h): the maps of the members' LAST forwards — member c holds the
  // same images at scales[c] — resampled onto member `base`'s grid, brought into its units and averaged, in ONE launch (launch_fuse_maps)
  // into a float32 buffer the group owns.  Everything runs on the group's stream (the first member's own; fuse_maps: or the caller's), so
  // a grouped forward issued there before is complete; a caller who forwarded the members individually synchronises them first.
  // The fused buffer, the table and the scratch are the group's only copies: every call first makes its stream wait for the previous
  // call's work (an event, no host wait), so a call may follow an asynchronous fuse_maps on another stream.  What an asynchronous
  // fuse_maps wrote to the caller's device buffers is the caller's to wait for, as with forward_images.
  // fuse_maps: the fused maps as NCHW float32 (any of them null: not fused), host or device, stream as forward_images
  // Mirrored members (dc_group_*_mirrored; the rule: include/deepcut_hip.h): `fm` names the members that saw the image flipped left to
  // right, the image's width, the joint permutation and the regression edges.  Null, or no member marked: nobody is mirrored, and the
  // launch reads no mirror table.  Otherwise the same launch_fuse_maps, with the two tables of the mirrored members.
  struct FuseMirror {
    const int* mirror;        // [M] 0/1, null = none
    int image_width;
    const int* joint_mirror;  // [J]
    int n_edges;
    const int* edges;         // [n_edges][2]
  };
  void fuse_maps(const double* scales, int base, int n_edges, const double* mean, const double* stdev, float* prob, float* loc, float* next,
                 bool is_device, void* user_stream, const FuseMirror* fm = nullptr);
  // Net::detect_parts on the fused prob / loc_pred at scales[base]
  void detect_parts(const double* scales, int base, float thr, int radius, int max_det, int* counts, double* dets, const FuseMirror* fm = nullptr);
  // Net::draw_heatmap on the fused prob (fused alone, as detect_parts fuses it) at scales[base] (dc_group_draw_heatmap; heat.cpp)
  void draw_heatmap(const dc_frame* frames, int nb, int h, int w, bool is_device, const double* scales, int base, double origin_x,
                    double origin_y, const dc_heat_style* style, const FuseMirror* fm = nullptr);
  // fusion of all three maps, then Net::assemble_people's three launches on them at scales[base] (p.scale is not read)
  void assemble_people(const double* scales, int base, const Net::AssembleParams& p, int n_edges, const int* edges, const double* mean,
                       const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, double* cost,
                       const FuseMirror* fm = nullptr, Tracker* tracker = nullptr, long long* ids = nullptr, int* place = nullptr,
                       const int* slot_of = nullptr);
  // Single-person pose from the fused maps (dc_group_decode_pose): prob and loc_pred fused as detect_parts fuses them, then
  // launch_pose_decode on the fused float32 views at scales[base] -> pose [NB][5][J], host or device, stream as fuse_maps
  void decode_pose(const double* scales, int base, double* pose, bool is_device, void* user_stream, const FuseMirror* fm = nullptr);
  // The box entry's fused decode (dc_group_decode_boxes) on the boxes of the members' last forward_boxes: prob and loc_pred fused with the
  // pyramid scales as member scales and, for a mirrored member, one reflected column per box (its crop width and the scale the member ran
  // it at, from the member's own box table); then launch_pose_decode_items on the fused views with the base member's decode items.
  // fm->image_width is not read.  Any of prob / loc / pose null: not returned.
  void decode_boxes(const double* pyramid, int base, float* prob, float* loc, double* pose, bool is_device, void* user_stream,
                    const FuseMirror* fm = nullptr);
  // lanes: 0 = automatic (2 members: two lanes; 3: one; 4 and more: two), else that many (at most one per member); every merged plan is dropped
  void set_lanes(int n);
  int lanes() const { return cur_ ? cur_->nlanes : lanes_opt_; }
  std::string plan_text();
  std::string profile_text(int iters);
  // as Net::tune_report_text / Net::set_tile, for the merged launches of the last forward's plan (signature = "G<problems>:" + the
  // members' signatures): what deepcut_tools.tune_in_flight walks when the load is groups in flight
  std::string tune_report_text();
  void set_tile(const std::string& key, const std::string& tile);
  int num_launches();
  int num_multi_launches();
  double flops();

 private:
  std::vector<std::unique_ptr<GroupPlan>> plans_;
  GroupPlan* cur_ = nullptr;
  uint64_t use_clock_ = 0;
  int lanes_opt_ = 0;
  std::vector<void*> lane_events_;  // per lane: its join event
  std::map<void*, std::vector<void*>> lane_choice_;  // caller's stream -> per lane the side stream measured best (index 0 unused; borrowed)
  void* fork_event_ = nullptr;
  GroupPlan& ensure_plan();   // after every member's begin_batch: the merged plan of the members' current shapes
  void merge(GroupPlan& gp);
  bool plan_current(const GroupPlan& gp) const;
  GroupPlan& current_plan();
  void forget_plan(GroupPlan* gp);  // out of the cache (a merge that threw, an eviction); cur_ never dangles
  void autotune(GroupPlan& gp);
  void apply_variant(GroupPlan& gp, GroupLaunch& gl, int variant);
  void run(GroupPlan& gp, int lane, void* s);  // lane < 0: every launch
  void enqueue(void* s);
  void launch_lanes(GroupPlan& gp, void* s, const std::vector<void*>& side, bool use_graph);
  void choose_lane_streams(GroupPlan& gp, void* s, bool use_graph);
  void drop_plan(GroupPlan& gp);
  void* stream();
  // fusion: the host checks (-> channels per map, 0 where use[k] is false, and the batch size), and the launch (-> the fused maps as
  // channel views of fused_)
  struct FusedMaps {
    Net::MapRef map[3];
  };
  void check_scales(const char* who, const double* scales, int base) const;  // the scales and the base index alone
  void check_fuse(const char* who, const double* scales, int base, const bool use[3], int n_edges, const double* mean, const double* stdev,
                  int C[3], int& NB) const;
  // what check_mirror makes of a FuseMirror (host only): empty `on` = no mirrored member
  struct MirrorPlan {
    std::vector<int> on;      // [M] 0/1
    std::vector<int> pi;      // [J]
    std::vector<int> edge;    // [E]: the lowest-index edge equal to (pi[a], pi[c]) of edge (a, c); empty when next_pred takes no part
    int image_width = 0;
  };
  MirrorPlan check_mirror(const char* who, const FuseMirror* fm, int base, const bool use[3], int n_edges, const int C[3]) const;
  // ws: null = every image of a mirrored member m reflects at (mp.image_width - 1) * scales[m]; else [M][NB], the box entry's own
  FusedMaps fuse(const double* scales, int base, const bool use[3], const double* mean, const double* stdev, void* s, const MirrorPlan& mp,
                 const std::vector<double>* ws = nullptr);
  // the fused maps k with dst[k] != null as NCHW float32 to host or device destinations, enqueued on s (fuse_maps, decode_boxes)
  void emit_fused(const FusedMaps& fm, float* const dst[3], bool is_device, void* s);
  DevBuf fused_, fuse_table_, fuse_stage_, people_scratch_;
  void* fuse_event_ = nullptr;    // recorded behind the last fusion call's work ...
  void* fuse_stream_ = nullptr;   // ... on this stream
  void fuse_done(void* s);        // record it
  std::vector<unsigned char> fuse_table_host_;  // what fuse_table_ holds: the members' descriptors, then gain and bias [M][channels] (a member mirrored: then the FuseFlip records [M][NB] and the source channels)
};

// ---- runtime.cpp: pinned host memory (dc_host_alloc / dc_host_free) ---------------------------------------------------------
void* host_alloc_pinned(size_t bytes);
void host_free_pinned(void* p);

// ---- multi_gpu.cpp: in-process multi-GPU forward (dc_comm_*, dc_forward_batch) ----------------------------------------------
struct Comm;
Comm* comm_create(int nexec, const int* devices, int transport);
void comm_destroy(Comm* c);
int comm_transport(const Comm* c);
int comm_nexec(const Comm* c);
void comm_forward(Comm* c, Net* const* nets, int nexec, const float* const* inputs, const int (*hw)[2], int n, float* const* prob, float* const* loc,
                  float* const* next);
int comm_item_executor(const Comm* c, int i);
void comm_root_maps(const Comm* c, int i, const void** prob, const void** loc, const void** next, int dims[5]);
std::vector<std::vector<int>> lpt_schedule(const std::vector<double>& cost, int nexec);

}  // namespace dc
