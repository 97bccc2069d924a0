// c_api.cpp — the extern "C" boundary declared in include/deepcut_hip.h.  No C++ exception and no
// C++ type crosses it.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/deepcut_hip.h"
#include "net.h"

using namespace dc;

// dc_net* / dc_blob* are dc::Net* / dc::NetBlob* behind opaque C names

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
template <typename F>
int guard(F&& f) {
  try {
    f();
    return DC_OK;
  } catch (const DcError& e) {
    return fail(e.code, e.what());
  } catch (const std::bad_alloc&) {
    return fail(DC_EDEVICE, "out of host memory");
  } catch (const std::exception& e) {
    return fail(DC_EINVAL, e.what());
  }
}
// stand-alone blobs (dc_blob_create) move on the default stream of the calling thread's device (Caffe::SetDevice)
void standalone_device() {
  if (device_count() <= 0) throw DcError(DC_EDEVICE, "no HIP device visible");
  if (hipSetDevice(Context::get().device) != hipSuccess) throw DcError(DC_EDEVICE, "hipSetDevice failed");
}
inline Net* N(dc_net* n) { return reinterpret_cast<Net*>(n); }
inline NetBlob* B(dc_blob* b) { return reinterpret_cast<NetBlob*>(b); }
#define REQUIRE(p)                                                   \
  if (!(p)) return fail(DC_EINVAL, "null argument: " #p)
}  // namespace

extern "C" {

const char* dc_last_error(void) { return g_err.c_str(); }
const char* dc_version(void) { return "deepcut_hip 0.1 (gfx950)"; }

int dc_set_mode(int mode) {
  if (mode != DC_MODE_CPU && mode != DC_MODE_GPU) return fail(DC_EINVAL, "mode must be DC_MODE_CPU or DC_MODE_GPU");
  Context::get().mode = mode;
  return DC_OK;
}
int dc_get_mode(void) { return Context::get().mode; }
int dc_set_device(int id) {
  int n = device_count();
  if (id < 0 || (n > 0 && id >= n))
    return fail(DC_EDEVICE, "device " + std::to_string(id) + " out of range (" + std::to_string(n) + " visible)");
  Context::get().device = id;
  if (n > 0 && hipSetDevice(id) != hipSuccess) return fail(DC_EDEVICE, "hipSetDevice failed");
  return DC_OK;
}
int dc_get_device(void) { return Context::get().device; }
int dc_device_count(void) { return device_count(); }

int dc_net_create_from_text(const char* text, const char* model, int phase, dc_net** out) {
  REQUIRE(text);
  REQUIRE(out);
  *out = nullptr;
  return guard([&] {
    std::unique_ptr<Net> n(Net::create(text, phase));
    if (model && *model) n->copy_from(model);
    *out = reinterpret_cast<dc_net*>(n.release());
  });
}
int dc_net_create(const char* proto, const char* model, int phase, dc_net** out) {
  REQUIRE(proto);
  REQUIRE(out);
  *out = nullptr;
  return guard([&] {
    std::string text = read_file(proto);
    if (model && *model) {  // CheckFile (_caffe.cpp:45-52): fail before building the net
      FILE* f = std::fopen(model, "rb");
      if (!f) throw DcError(DC_EIO, std::string("Could not open file ") + model);
      std::fclose(f);
    }
    std::unique_ptr<Net> n(Net::create(text, phase));
    if (model && *model) n->copy_from(model);
    *out = reinterpret_cast<dc_net*>(n.release());
  });
}
int dc_net_clone(dc_net* net, dc_net** out) {
  REQUIRE(net);
  REQUIRE(out);
  *out = nullptr;
  return guard([&] { *out = reinterpret_cast<dc_net*>(N(net)->clone()); });
}
int dc_net_forward_host_async(dc_net* net, const float* input, int n, int h, int w, float* prob, float* loc, float* next) {
  REQUIRE(net);
  REQUIRE(input);
  if (n <= 0 || h <= 0 || w <= 0) return fail(DC_EINVAL, "forward_host_async: n, h, w must be positive");
  return guard([&] { N(net)->forward_batch(input, n, h, w, false, prob, loc, next, nullptr, true); });
}
int dc_host_alloc(size_t bytes, void** out) {
  REQUIRE(out);
  *out = nullptr;
  if (bytes == 0) return fail(DC_EINVAL, "dc_host_alloc: zero bytes");
  return guard([&] {
    standalone_device();
    *out = host_alloc_pinned(bytes);
  });
}
int dc_host_free(void* p) {
  if (!p) return DC_OK;
  return guard([&] { host_free_pinned(p); });
}
int dc_nets_choose_streams(dc_net* const* nets, int n, int candidates, int reps, double* rate_chosen, double* rate_first) {
  REQUIRE(nets);
  if (n < 1 || n > 64) return fail(DC_EINVAL, "dc_nets_choose_streams: 1..64 executors");
  std::vector<Net*> v;
  for (int i = 0; i < n; ++i) {
    if (!nets[i]) return fail(DC_EINVAL, "dc_nets_choose_streams: null net");
    for (Net* o : v)
      if (o == N(nets[i])) return fail(DC_EINVAL, "dc_nets_choose_streams: the same net twice");
    v.push_back(N(nets[i]));
  }
  return guard([&] { Net::choose_streams(v, candidates, reps <= 0 ? 3 : reps, rate_chosen, rate_first); });
}
int dc_net_stream(dc_net* net, void** out) {
  REQUIRE(net);
  REQUIRE(out);
  *out = nullptr;
  return guard([&] {
    if (Context::get().mode != DC_MODE_GPU) throw DcError(DC_ENOCPU, "dc_net_stream in CPU mode: libdeepcut_hip provides the MI355X path only");
    *out = N(net)->own_stream();
  });
}
int dc_net_busy(dc_net* net, int* busy) {
  REQUIRE(net);
  REQUIRE(busy);
  *busy = 0;
  if (!N(net)->stream) return DC_OK;
  hipError_t e = hipStreamQuery((hipStream_t)N(net)->stream);
  if (e == hipErrorNotReady) {
    *busy = 1;
    return DC_OK;
  }
  if (e != hipSuccess) return fail(DC_EDEVICE, std::string("hipStreamQuery failed: ") + hipGetErrorString(e));
  return DC_OK;
}
int dc_net_synchronize(dc_net* net) {
  REQUIRE(net);
  return guard([&] { N(net)->synchronize(); });
}
int dc_net_destroy(dc_net* net) {
  if (net) delete N(net);
  return DC_OK;
}
int dc_net_set_option(dc_net* net, int key, int value) {
  REQUIRE(net);
  return guard([&] {
    Net* n = N(net);
    if (key == DC_OPT_FUSE) {
      if (n->fuse != value) n->invalidate_plans();
      n->fuse = value;
    } else if (key == DC_OPT_HIPGRAPH) {
      n->use_graph = value;
    } else if (key == DC_OPT_DTYPE) {
      n->set_dtype(value);
    } else if (key == DC_OPT_OUTPUTS) {
      n->set_outputs_mask(value);
    } else if (key == DC_OPT_SPARSE_PAIRWISE) {
      n->set_sparse_pairwise(value);
    } else {
      throw DcError(DC_EINVAL, "unknown option " + std::to_string(key));
    }
  });
}
int dc_net_get_option(dc_net* net, int key, int* value) {
  REQUIRE(net);
  REQUIRE(value);
  Net* n = N(net);
  if (key == DC_OPT_FUSE) *value = n->fuse;
  else if (key == DC_OPT_HIPGRAPH) *value = n->use_graph;
  else if (key == DC_OPT_DTYPE) *value = n->dtype;
  else if (key == DC_OPT_OUTPUTS) *value = n->outputs_mask;
  else if (key == DC_OPT_SPARSE_PAIRWISE) *value = n->sparse_pairwise;
  else return fail(DC_EINVAL, "unknown option " + std::to_string(key));
  return DC_OK;
}
int dc_net_copy_from(dc_net* net, const char* path) {
  REQUIRE(net);
  REQUIRE(path);
  return guard([&] { N(net)->copy_from(path); });
}
int dc_net_save(dc_net* net, const char* path) {
  REQUIRE(net);
  REQUIRE(path);
  return guard([&] { N(net)->save(path); });
}
const char* dc_net_name(dc_net* net) { return net ? N(net)->name.c_str() : ""; }

int dc_net_num_layers(dc_net* net) { return net ? (int)N(net)->layers.size() : 0; }
const char* dc_net_layer_name(dc_net* net, int i) {
  if (!net || i < 0 || i >= (int)N(net)->layers.size()) return nullptr;
  return N(net)->layers[i].name.c_str();
}
const char* dc_net_layer_type(dc_net* net, int i) {
  if (!net || i < 0 || i >= (int)N(net)->layers.size()) return nullptr;
  return N(net)->layers[i].type.c_str();
}
int dc_net_num_blobs(dc_net* net) { return net ? (int)N(net)->blobs.size() : 0; }
const char* dc_net_blob_name(dc_net* net, int i) {
  if (!net || i < 0 || i >= (int)N(net)->blobs.size()) return nullptr;
  return N(net)->blobs[i]->name.c_str();
}
int dc_net_blob(dc_net* net, const char* name, dc_blob** out) {
  REQUIRE(net);
  REQUIRE(name);
  REQUIRE(out);
  auto it = N(net)->blob_index.find(name);
  if (it == N(net)->blob_index.end()) return fail(DC_EINVAL, std::string("Unknown blob name ") + name);
  *out = reinterpret_cast<dc_blob*>(N(net)->blobs[it->second].get());
  return DC_OK;
}
int dc_net_num_inputs(dc_net* net) { return net ? (int)N(net)->inputs.size() : 0; }
const char* dc_net_input_name(dc_net* net, int i) {
  if (!net || i < 0 || i >= (int)N(net)->inputs.size()) return nullptr;
  return N(net)->blobs[N(net)->inputs[i]]->name.c_str();
}
int dc_net_num_outputs(dc_net* net) { return net ? (int)N(net)->outputs.size() : 0; }
const char* dc_net_output_name(dc_net* net, int i) {
  if (!net || i < 0 || i >= (int)N(net)->outputs.size()) return nullptr;
  return N(net)->blobs[N(net)->outputs[i]]->name.c_str();
}
int dc_net_layer_num_params(dc_net* net, const char* layer) {
  if (!net || !layer) return 0;
  int li = N(net)->layer_index(layer);
  return li < 0 ? 0 : (int)N(net)->layers[li].params.size();
}
int dc_net_param(dc_net* net, const char* layer, int idx, dc_blob** out) {
  REQUIRE(net);
  REQUIRE(layer);
  REQUIRE(out);
  int li = N(net)->layer_index(layer);
  if (li < 0) return fail(DC_EINVAL, std::string("Unknown layer name ") + layer);
  auto& ps = N(net)->layers[li].params;
  if (idx < 0 || idx >= (int)ps.size()) return fail(DC_EINVAL, "param index out of range");
  *out = reinterpret_cast<dc_blob*>(ps[idx].get());
  return DC_OK;
}

int dc_net_reshape(dc_net* net) {
  REQUIRE(net);
  return guard([&] { N(net)->reshape(); });
}
int dc_net_forward(dc_net* net, int start, int end, float* loss) {
  REQUIRE(net);
  if (loss) *loss = 0.f;
  int nl = (int)N(net)->layers.size();
  if (start < 0 || end >= nl || start > end + 1)
    return fail(DC_EINVAL, "forward range out of bounds (net.cpp:566-567)");
  return guard([&] { N(net)->forward(start, end); });
}
int dc_net_forward_all(dc_net* net) {
  REQUIRE(net);
  return guard([&] { N(net)->forward(0, (int)N(net)->layers.size() - 1); });
}

int dc_blob_num_axes(dc_blob* b) { return b ? (int)B(b)->st->shape.size() : 0; }
int dc_blob_shape(dc_blob* b, int* ndim, int* dims) {
  REQUIRE(b);
  REQUIRE(ndim);
  REQUIRE(dims);
  auto& s = B(b)->st->shape;
  if (s.size() > 8) return fail(DC_EINVAL, "too many axes");
  *ndim = (int)s.size();
  for (size_t i = 0; i < s.size(); ++i) dims[i] = s[i];
  return DC_OK;
}
int dc_blob_count(dc_blob* b) { return b ? (int)B(b)->st->count() : 0; }
int dc_blob_reshape(dc_blob* b, int ndim, const int* dims) {
  REQUIRE(b);
  if (ndim < 0 || ndim > 8) return fail(DC_EINVAL, "bad number of axes");
  if (ndim > 0) REQUIRE(dims);  // a 0-axis (scalar) shape has no dimension list, as in dc_blob_create
  return guard([&] {
    Storage& s = *B(b)->st;
    if (s.is_param) throw DcError(DC_EINVAL, "parameter blobs cannot be reshaped");
    s.reshape(ndim > 0 ? std::vector<int>(dims, dims + ndim) : std::vector<int>());
  });
}
static int blob_host(dc_blob* b, float** out, bool mut) {
  return guard([&] {
    Storage& s = *B(b)->st;
    if (s.elided && !s.is_param)
      throw DcError(DC_EUNSUP, "blob '" + B(b)->name + "' is folded into a fused kernel in the current plan (or feeds only outputs that "
                                "DC_OPT_OUTPUTS leaves out) and never materialised; create the net with DC_OPT_FUSE 0 / all outputs to observe it");
    if (s.head == HEAD_AT_GPU) {
      if (s.owner) s.owner->sync_to_host(s);
      else standalone_device(), storage_to_host(s, nullptr, nullptr);
    }
    *out = s.host_ptr();
    s.host_touched = true;
    if (s.head == UNINITIALIZED) s.head = HEAD_AT_CPU;
    if (mut) {
      s.head = HEAD_AT_CPU;
      if (s.is_param && s.shared) {  // a writable view was handed out: its content is re-checked before the next run
        std::lock_guard<std::mutex> lk(s.shared->mu);
        if (!s.touch_listed) s.shared->touched.push_back(B(b)->st), s.touch_listed = true;
      }
    }
  });
}
int dc_blob_cpu_data(dc_blob* b, const float** out) {
  REQUIRE(b);
  REQUIRE(out);
  float* p = nullptr;
  int r = blob_host(b, &p, false);
  *out = p;
  return r;
}
int dc_blob_mutable_cpu_data(dc_blob* b, float** out) {
  REQUIRE(b);
  REQUIRE(out);
  return blob_host(b, out, true);
}
int dc_blob_head(dc_blob* b) { return b ? B(b)->st->head : 0; }
int dc_blob_gpu_data(dc_blob* b, const void** dev, int* pitch) {
  REQUIRE(b);
  REQUIRE(dev);
  return guard([&] {
    Storage& s = *B(b)->st;
    if (s.is_param) throw DcError(DC_EUNSUP, "parameters are packed per kernel on the device; no NHWC image exists");
    if (s.view_of < 0 && (s.head == HEAD_AT_CPU || s.head == UNINITIALIZED)) {
      if (s.owner) s.owner->sync_to_device(s);
      else standalone_device(), storage_to_device(s, nullptr);
    }
    if (s.view_of >= 0) {  // channel slice of a concatenated head tensor
      Storage& base = *s.owner->storages[s.view_of];
      *dev = base.dev_at(s.view_c0);
      if (pitch) *pitch = base.cp();
    } else {
      *dev = s.dev;
      if (pitch) *pitch = s.cp();
    }
  });
}

int dc_blob_create(int ndim, const int* dims, dc_blob** out) {
  REQUIRE(out);
  *out = nullptr;
  if (ndim < 0 || ndim > 8 || (ndim > 0 && !dims)) return fail(DC_EINVAL, "bad number of axes");
  return guard([&] {
    std::unique_ptr<NetBlob> b(new NetBlob());
    b->standalone = true;
    b->st = std::make_shared<Storage>();
    b->st->reshape(std::vector<int>(dims, dims + ndim));
    *out = reinterpret_cast<dc_blob*>(b.release());
  });
}
int dc_blob_destroy(dc_blob* b) {
  if (!b) return DC_OK;
  if (!B(b)->standalone) return fail(DC_EINVAL, "this blob belongs to a net");
  delete B(b);
  return DC_OK;
}
int dc_blob_mutable_gpu_data(dc_blob* b, void** dev, int* pitch) {
  REQUIRE(b);
  REQUIRE(dev);
  return guard([&] {
    Storage& s = *B(b)->st;
    if (s.is_param) throw DcError(DC_EUNSUP, "parameters are packed per kernel on the device; no NHWC image exists");
    if (s.view_of >= 0 || s.elided)
      throw DcError(DC_EUNSUP, "blob '" + B(b)->name + "' is fused into another tensor in the current plan; use DC_OPT_FUSE 0");
    if (s.owner) {
      s.owner->sync_to_device(s);
      s.head = HEAD_AT_GPU;
    } else {
      standalone_device();
      storage_mutable_device(s, nullptr);
    }
    *dev = s.dev;
    if (pitch) *pitch = s.cp();
  });
}
int dc_blob_copy_from(dc_blob* dst, dc_blob* src, int reshape) {
  REQUIRE(dst);
  REQUIRE(src);
  return guard([&] {
    Storage &d = *B(dst)->st, &s = *B(src)->st;
    if (s.elided && !s.is_param) throw DcError(DC_EUNSUP, "source blob '" + B(src)->name + "' is never materialised in the current plan");
    if (d.shape != s.shape) {  // Blob::CopyFrom (blob.cpp:435-443)
      if (!reshape) throw DcError(DC_ESHAPE, "Trying to copy blobs of different sizes.");
      if (d.is_param) throw DcError(DC_EINVAL, "parameter blobs cannot be reshaped");
      d.reshape(s.shape);
    }
    Net* own = d.owner ? d.owner : s.owner;
    void* stream = nullptr;
    if (s.head == HEAD_AT_GPU) {
      if (s.owner && s.owner != own) s.owner->synchronize();  // the source may still be being written on its own net's stream
      if (own) {
        own->synchronize();
        stream = own->stream;
        if (hipSetDevice(own->device >= 0 ? own->device : Context::get().device) != hipSuccess) throw DcError(DC_EDEVICE, "hipSetDevice failed");
      } else {
        standalone_device();
      }
    }
    storage_copy(d, s, s.view_of >= 0 && s.owner ? s.owner->storages[s.view_of].get() : nullptr, stream);
    if (d.is_param && d.shared) {
      std::lock_guard<std::mutex> lk(d.shared->mu);
      if (!d.touch_listed) d.shared->touched.push_back(B(dst)->st), d.touch_listed = true;
    }
  });
}
int dc_net_create_for_layer(const char* layer_text, int phase, int nbottom, dc_blob* const* bottoms, dc_net** out) {
  REQUIRE(layer_text);
  REQUIRE(out);
  *out = nullptr;
  if (nbottom < 0 || (nbottom > 0 && !bottoms)) return fail(DC_EINVAL, "bad bottom list");
  return guard([&] {
    std::vector<std::vector<int>> shapes;
    for (int i = 0; i < nbottom; ++i) {
      if (!bottoms[i]) throw DcError(DC_EINVAL, "null bottom blob");
      shapes.push_back(B(bottoms[i])->st->shape);
    }
    *out = reinterpret_cast<dc_net*>(Net::create_for_layer(layer_text, phase, shapes));
  });
}

int dc_net_forward_batch(dc_net* net, const float* input, int n, int h, int w, int is_device, float* prob,
                         float* loc_pred, float* next_pred, void* stream) {
  REQUIRE(net);
  REQUIRE(input);
  if (n <= 0 || h <= 0 || w <= 0) return fail(DC_EINVAL, "bad batch shape");
  return guard([&] { N(net)->forward_batch(input, n, h, w, is_device != 0, prob, loc_pred, next_pred, stream); });
}

int dc_net_forward_requests(dc_net* net, int n, const float* const* inputs, int h, int w, float* const* prob,
                            float* const* loc_pred, float* const* next_pred, void* stream) {
  REQUIRE(net);
  REQUIRE(inputs);
  if (n <= 0 || h <= 0 || w <= 0) return fail(DC_EINVAL, "bad batch shape");
  for (int i = 0; i < n; ++i)
    if (!inputs[i]) return fail(DC_EINVAL, "null request input");
  return guard([&] { N(net)->forward_requests(n, inputs, h, w, prob, loc_pred, next_pred, stream); });
}

int dc_net_decode_pose(dc_net* net, double scale, double* pose, int is_device, void* stream) {
  REQUIRE(net);
  REQUIRE(pose);
  if (!(scale > 0)) return fail(DC_EINVAL, "scale must be positive");
  return guard([&] { N(net)->decode_pose(scale, pose, is_device != 0, stream); });
}

int dc_net_emit_maps(dc_net* net, void* prob, void* loc_pred, void* next_pred, int elem, int is_device, void* stream) {
  REQUIRE(net);
  return guard([&] { N(net)->emit_last_maps(prob, loc_pred, next_pred, elem, is_device != 0, stream); });
}

int dc_net_forward_images(dc_net* net, const unsigned char* images, int n, int height, int width, double scale,
                          int is_device, float* prob, float* loc_pred, float* next_pred, double* pose, void* stream) {
  REQUIRE(net);
  REQUIRE(images);
  if (n <= 0 || height <= 0 || width <= 0) return fail(DC_EINVAL, "n, height and width must be positive");
  if (!(scale > 0)) return fail(DC_EINVAL, "scale must be positive");
  return guard([&] {
    N(net)->forward_images(images, n, height, width, scale, is_device != 0, prob, loc_pred, next_pred, pose, stream);
  });
}

int dc_net_forward_boxes(dc_net* net, const unsigned char* image, int height, int width, int is_device, const int* boxes, const double* scales,
                         int n, int canvas_h, int canvas_w, float* prob, float* loc_pred, float* next_pred, double* pose, void* stream) {
  REQUIRE(net);
  if (n == 0) return DC_OK;
  REQUIRE(image);
  return guard([&] {
    N(net)->forward_boxes(image, height, width, is_device != 0, boxes, scales, n, canvas_h, canvas_w, prob, loc_pred, next_pred, pose, stream);
  });
}

int dc_net_forward_frames(dc_net* net, const dc_frame* frames, int n, int height, int width, double scale, int is_device, float* prob,
                          float* loc_pred, float* next_pred, double* pose, void* stream) {
  REQUIRE(net);
  REQUIRE(frames);
  if (n <= 0 || height <= 0 || width <= 0) return fail(DC_EINVAL, "n, height and width must be positive");
  if (!(scale > 0)) return fail(DC_EINVAL, "scale must be positive");
  return guard([&] {
    N(net)->forward_images(nullptr, n, height, width, scale, is_device != 0, prob, loc_pred, next_pred, pose, stream, frames);
  });
}

int dc_net_forward_boxes_frame(dc_net* net, const dc_frame* frame, int height, int width, int is_device, const int* boxes,
                               const double* scales, int n, int canvas_h, int canvas_w, float* prob, float* loc_pred, float* next_pred,
                               double* pose, void* stream) {
  REQUIRE(net);
  if (n == 0) return DC_OK;
  REQUIRE(frame);
  return guard([&] {
    N(net)->forward_boxes(nullptr, height, width, is_device != 0, boxes, scales, n, canvas_h, canvas_w, prob, loc_pred, next_pred, pose, stream,
                          frame);
  });
}

int dc_image_canvas_size(int height, int width, double scale, int* canvas_h, int* canvas_w) {
  REQUIRE(canvas_h);
  REQUIRE(canvas_w);
  if (height <= 0 || width <= 0 || !(scale > 0)) return fail(DC_EINVAL, "height, width and scale must be positive");
  int nh, nw;
  dc::image_canvas_size(height, width, scale, *canvas_h, *canvas_w, nh, nw);
  return DC_OK;
}

int dc_net_detect_parts(dc_net* net, double scale, float threshold, int radius, int max_det, int* counts, double* dets) {
  REQUIRE(net);
  REQUIRE(counts);
  REQUIRE(dets);
  return guard([&] { N(net)->detect_parts(scale, threshold, radius, max_det, counts, dets); });
}

int dc_net_decode_pairwise(dc_net* net, double scale, int ndet, const int* detections, const double* mean,
                           const double* stdev, double* out) {
  REQUIRE(net);
  if (ndet > 0) {
    REQUIRE(detections);
    REQUIRE(out);
  }
  return guard([&] { N(net)->decode_pairwise(scale, ndet, detections, mean, stdev, out); });
}

int dc_net_pairwise_at(dc_net* net, int ndet, const int* detections, float* out) {
  REQUIRE(net);
  if (ndet > 0) {
    REQUIRE(detections);
    REQUIRE(out);
  }
  return guard([&] { N(net)->pairwise_at(ndet, detections, out); });
}

int dc_pair_stats_read(const char* path, int max_edges, int* n_edges, int* edges, double* mean, double* stdev) {
  REQUIRE(path);
  REQUIRE(n_edges);
  REQUIRE(edges);
  REQUIRE(mean);
  REQUIRE(stdev);
  *n_edges = 0;
  if (max_edges < 0) return fail(DC_EINVAL, "max_edges must be >= 0");
  return guard([&] {
    const PairStats st = read_pair_stats(path);
    *n_edges = st.n_edges();
    if (st.n_edges() > max_edges)
      throw DcError(DC_EINVAL, std::string("pair statistics ") + path + ": " + std::to_string(st.n_edges()) + " edges, the caller's arrays hold max_edges = " +
                                   std::to_string(max_edges));
    std::copy(st.edges.begin(), st.edges.end(), edges);
    std::copy(st.mean.begin(), st.mean.end(), mean);
    std::copy(st.stdev.begin(), st.stdev.end(), stdev);
  });
}

int dc_net_assemble_people(dc_net* net, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean, const double* stdev,
                           const int* joint_order, int* n_people, double* people, int* cand, double* cost) {
  REQUIRE(net);
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    N(net)->assemble_people(q, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost);
  });
}

int dc_net_flops(dc_net* net, double* flops) {
  REQUIRE(net);
  REQUIRE(flops);
  return guard([&] {
    Net* n = N(net);
    n->ensure_plan();
    *flops = n->plan_flops;
  });
}
int dc_net_num_launches(dc_net* net) {
  if (!net) return 0;
  int r = 0;
  guard([&] {
    N(net)->plan_text();
    r = (int)N(net)->plan.size();
  });
  return r;
}
const char* dc_net_plan_text(dc_net* net) {
  if (!net) return nullptr;
  Net* n = N(net);
  int rc = guard([&] { n->text_buf = n->plan_text(); });
  return rc == DC_OK ? n->text_buf.c_str() : nullptr;
}
int dc_net_stats(dc_net* net, long long* out, int n) {
  REQUIRE(net);
  REQUIRE(out);
  const NetStats& st = N(net)->stats;
  const long long v[DC_NUM_STATS] = {st.lowerings,      st.graph_instantiations, st.plan_hits, st.autotune_runs,
                                     st.buffer_growths, st.repacks,              (long long)N(net)->parked_.size() + (N(net)->plan_valid ? 1 : 0),
                                     st.sparse_packs};
  for (int i = 0; i < n && i < DC_NUM_STATS; ++i) out[i] = v[i];
  return DC_OK;
}
int dc_net_reserve(dc_net* net, int n, int h, int w) {
  REQUIRE(net);
  if (n <= 0 || h <= 0 || w <= 0) return fail(DC_EINVAL, "bad batch shape");
  return guard([&] { N(net)->reserve(n, h, w); });
}
int dc_net_device(dc_net* net) { return net ? N(net)->device : -1; }

const char* dc_net_profile_text(dc_net* net, int iters) {
  if (!net) return nullptr;
  Net* n = N(net);
  int rc = guard([&] { n->text_buf = n->profile_text(iters > 0 ? iters : 10); });
  return rc == DC_OK ? n->text_buf.c_str() : nullptr;
}

const char* dc_net_debug_info(dc_net* net) {
  if (!net) return nullptr;
  Net* n = N(net);
  int rc = guard([&] { n->text_buf = n->debug_info_text(); });
  return rc == DC_OK ? n->text_buf.c_str() : nullptr;
}

const char* dc_net_tune_report(dc_net* net) {
  if (!net) return nullptr;
  Net* n = N(net);
  int rc = guard([&] { n->text_buf = n->tune_report_text(); });
  return rc == DC_OK ? n->text_buf.c_str() : nullptr;
}
int dc_net_set_tile(dc_net* net, const char* signature, const char* tile) {
  REQUIRE(net);
  REQUIRE(signature);
  REQUIRE(tile);
  return guard([&] { N(net)->set_tile(signature, tile); });
}

// tile variants of the gather-GEMM (diagnostics / tests: DC_CONV_VARIANT takes an index into this table)
int dc_conv_variant_count(void) { return dc::conv_num_variants(); }
const char* dc_conv_variant_name(int i) { return i >= 0 && i < dc::conv_num_variants() ? dc::conv_variant(i).name : nullptr; }
int dc_conv_variant_esize(int i) { return i >= 0 && i < dc::conv_num_variants() ? dc::conv_variant_esize(i) : 0; }
int dc_conv_bf16_variant_count(void) { return dc::conv_num_bf16_variants(); }
const char* dc_conv_bf16_variant_name(int i) {
  return i >= 0 && i < dc::conv_num_bf16_variants() ? dc::conv_variant(dc::kBf16Variant0 + i).name : nullptr;
}
int dc_wino_half_pack(const float* g, int cout, int cin, int rowscale, float* out, float* row_scale) {
  REQUIRE(g);
  REQUIRE(out);
  REQUIRE(row_scale);
  if (cout <= 0 || cin <= 0 || cout % 32 || cin % 16) return fail(DC_EINVAL, "dc_wino_half_pack: cout must be a multiple of 32, cin of 16");
  return guard([&] { dc::wino_half_pack_filters(g, cout, cin, rowscale != 0, out, row_scale); });
}

int dc_wino_blocks(const char* tile, int tiles_y, int tiles_x) {
  if (!tile || tiles_y < 1 || tiles_x < 1) return -1;
  try {
    return (int)dc::wino_form_blocks(dc::variant_by_name(tile), tiles_y, tiles_x);
  } catch (...) {
    return -1;
  }
}

int dc_wino_cover(int tiles_y, int tiles_x, int* out) {
  if (!out || tiles_y < 1 || tiles_x < 1) return -1;
  const dc::WinoCover c = dc::wino_plan_cover(tiles_y, tiles_x);
  const int v[12] = {c.vertical, c.cut, c.blocks, c.na, c.nb, c.a_nby, c.a_nbx, c.b_nby, c.b_nbx, c.b_ty0, c.b_tx0, dc::wino_mix_offered(tiles_y, tiles_x) ? 1 : 0};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
  return c.blocks;
}

int dc_wino_mix_offered(int tiles_y, int tiles_x, int images, int cout) {
  if (tiles_y < 1 || tiles_x < 1 || images < 1 || cout < 1) return -1;
  return dc::wino_mix_offered_launch(tiles_y, tiles_x, images, cout) ? 1 : 0;
}

int dc_stream1x1_pack(const float* g, int cout, int k, float* out) {
  if (!g || !out) return fail(DC_EINVAL, "dc_stream1x1_pack: null pointer");
  if (cout <= 0 || k <= 0 || cout % 32 || k % 16) return fail(DC_EINVAL, "dc_stream1x1_pack: cout must be a multiple of 32, k of 16");
  return guard([&] { dc::stream1x1_pack_filters(g, cout, k, out); });
}

int dc_sparse_head_pack_size(int cout, int k3, int k5) {
  if (cout <= 0 || k3 <= 0 || k5 <= 0) return -1;
  const size_t n = dc::sparse_head_image_floats(cout, k3, k5);
  return n > 0x7fffffffu ? -1 : (int)n;
}

int dc_sparse_head_pack(const float* ws, const float* wd, int cout, int k3, int k5, float* out) {
  if (!ws || !wd || !out) return fail(DC_EINVAL, "dc_sparse_head_pack: null pointer");
  if (dc_sparse_head_pack_size(cout, k3, k5) < 0) return fail(DC_EINVAL, "dc_sparse_head_pack: cout, k3 and k5 must be positive (and the image below 2^31 floats)");
  return guard([&] { dc::sparse_head_pack_filters(ws, wd, cout, k3, k5, out); });
}

int dc_stream1x1f_pack(const float* g, int cout, int k, float* out) {
  if (!g || !out) return fail(DC_EINVAL, "dc_stream1x1f_pack: null pointer");
  if (cout <= 0 || k <= 0 || cout % 16 || k % 16) return fail(DC_EINVAL, "dc_stream1x1f_pack: cout and k must be multiples of 16");
  return guard([&] { dc::stream1x1f_pack_filters(g, cout, k, out); });
}

int dc_stream1x1f_rows(const float* x, int m, int k, int x_stride, const float* g, int cout, const float* scale, const float* shift, float* y,
                       int y_rows, int y_stride, int y_c0, const float* resid, int relu) {
  if (!x || !g || !y) return fail(DC_EINVAL, "dc_stream1x1f_rows: null pointer");
  if (m <= 0 || y_rows < m || k <= 0 || k % 16 || cout <= 0 || cout % 64 || x_stride < k || x_stride % 4 || y_stride % 4 || y_c0 < 0 || y_c0 % 4 ||
      y_c0 + cout > y_stride || (long)y_rows * y_stride * 4 >= 0x7fffffffL || (long)m * x_stride * 4 >= 0x7fffffffL)
    return fail(DC_EINVAL, "dc_stream1x1f_rows: m <= y_rows, k % 16 == 0, cout % 64 == 0, k <= x_stride, y_c0 + cout <= y_stride, strides and y_c0 multiples of 4");
  return guard([&] {
    ConvGemmParams p{};
    p.esize = 4, p.ekind = kElemF32;
    p.NB = 1, p.OH = 1, p.OW = m, p.M = m, p.Cout = cout;
    p.x_img_stride = (long)m * x_stride, p.x_row_stride = m * x_stride, p.x_rows = 1, p.x_rowlen = (m - 1) * x_stride + k;
    p.sy = 1, p.sx = x_stride, p.nty = 1, p.ntx = 1, p.klen = k, p.Ktot = k;
    p.y_img_stride = (long)m * y_stride, p.y_row_stride = m * y_stride, p.y_pix_stride = y_stride;
    p.relu = relu ? 1 : 0;
    if (!stream1x1f_eligible(p)) throw DcError(DC_EINVAL, "dc_stream1x1f_rows: the form does not take this shape");
    standalone_device();
    struct Dev {  // the launch's device buffers, freed whatever happens
      std::vector<void*> p;
      ~Dev() {
        for (void* q : p) (void)hipFree(q);
      }
      float* up(const float* h, size_t n) {
        void* d = nullptr;
        if (hipMalloc(&d, n * 4) != hipSuccess) throw DcError(DC_EDEVICE, "dc_stream1x1f_rows: hipMalloc failed");
        p.push_back(d);
        if (hipMemcpy(d, h, n * 4, hipMemcpyHostToDevice) != hipSuccess) throw DcError(DC_EDEVICE, "dc_stream1x1f_rows: copy to the device failed");
        return (float*)d;
      }
    } dev;
    std::vector<float> packed((size_t)cout * k);
    stream1x1f_pack_filters(g, cout, k, packed.data());
    const size_t ny = (size_t)y_rows * y_stride;
    float* const dy = dev.up(y, ny);
    p.x = dev.up(x, (size_t)m * x_stride);
    p.w = dev.up(packed.data(), packed.size());
    p.scale = scale ? dev.up(scale, cout) : nullptr;
    p.shift = shift ? dev.up(shift, cout) : nullptr;
    p.y = dy + y_c0;
    p.resid = resid ? dev.up(resid, ny) + y_c0 : nullptr;
    const int e = launch_stream1x1f(p, nullptr);
    if (e != 0 || hipDeviceSynchronize() != hipSuccess) throw DcError(DC_EDEVICE, "dc_stream1x1f_rows: the launch failed");
    if (hipMemcpy(y, dy, ny * 4, hipMemcpyDeviceToHost) != hipSuccess) throw DcError(DC_EDEVICE, "dc_stream1x1f_rows: copy from the device failed");
  });
}

int dc_wino43_pack(const float* g, int cout, int cin, float* out) {
  if (!g || !out) return fail(DC_EINVAL, "dc_wino43_pack: null pointer");
  if (cout <= 0 || cin <= 0 || cout % 16 || cin % 16) return fail(DC_EINVAL, "dc_wino43_pack: cout and cin must be multiples of 16");
  return guard([&] { dc::wino43_pack_filters(g, cout, cin, out); });
}

int dc_stem7x7_pack(const float* g, int c, float* out) {
  if (!g || !out) return fail(DC_EINVAL, "dc_stem7x7_pack: null pointer");
  if (c < 1 || c > 4) return fail(DC_EINVAL, "dc_stem7x7_pack: 1 to 4 input channels");
  return guard([&] { dc::stem7x7_pack_filters(g, c, out); });
}

// ---- pyramid-grouped execution ---------------------------------------------------------------------------------------
namespace {
inline NetGroup* G(dc_group* g) { return reinterpret_cast<NetGroup*>(g); }
}
int dc_group_create(dc_net* const* nets, int n, dc_group** out) {
  REQUIRE(nets);
  REQUIRE(out);
  *out = nullptr;
  if (n <= 0) return fail(DC_EINVAL, "a group needs at least one net");
  return guard([&] {
    std::vector<Net*> m;
    for (int i = 0; i < n; ++i) m.push_back(N(nets[i]));
    *out = reinterpret_cast<dc_group*>(NetGroup::create(m));
  });
}
int dc_group_destroy(dc_group* group) {
  delete G(group);
  return DC_OK;
}
int dc_group_size(dc_group* group) { return group ? (int)G(group)->nets.size() : 0; }
int dc_group_set_lanes(dc_group* group, int lanes) {
  REQUIRE(group);
  return guard([&] { G(group)->set_lanes(lanes); });
}
int dc_group_forward_batch(dc_group* group, const float* const* inputs, const int* n, const int* h, const int* w, int is_device,
                           float* const* prob, float* const* loc_pred, float* const* next_pred, void* stream) {
  REQUIRE(group);
  REQUIRE(inputs);
  REQUIRE(n);
  REQUIRE(h);
  REQUIRE(w);
  for (size_t c = 0; c < G(group)->nets.size(); ++c) {
    if (!inputs[c]) return fail(DC_EINVAL, "null input for group member " + std::to_string(c));
    if (n[c] <= 0 || h[c] <= 0 || w[c] <= 0) return fail(DC_EINVAL, "bad batch shape for group member " + std::to_string(c));
  }
  return guard([&] { G(group)->forward_batch(inputs, n, h, w, is_device != 0, prob, loc_pred, next_pred, stream); });
}
// the argument checks and the call of both image entries of a group (mirror null: nobody is mirrored)
static int group_forward_images(dc_group* group, const unsigned char* const* images, const int* n, const int* height, const int* width,
                                const double* scale, const int* mirror, int is_device, float* const* prob, float* const* loc_pred,
                                float* const* next_pred, double* const* pose, void* stream) {
  REQUIRE(group);
  REQUIRE(images);
  REQUIRE(n);
  REQUIRE(height);
  REQUIRE(width);
  REQUIRE(scale);
  for (size_t c = 0; c < G(group)->nets.size(); ++c) {
    if (!images[c]) return fail(DC_EINVAL, "null images for group member " + std::to_string(c));
    if (n[c] <= 0 || height[c] <= 0 || width[c] <= 0 || !(scale[c] > 0)) return fail(DC_EINVAL, "bad image shape / scale for group member " + std::to_string(c));
  }
  return guard([&] { G(group)->forward_images(images, n, height, width, scale, is_device != 0, prob, loc_pred, next_pred, pose, stream, mirror); });
}
int dc_group_forward_images(dc_group* group, const unsigned char* const* images, const int* n, const int* height, const int* width,
                            const double* scale, int is_device, float* const* prob, float* const* loc_pred, float* const* next_pred,
                            double* const* pose, void* stream) {
  return group_forward_images(group, images, n, height, width, scale, nullptr, is_device, prob, loc_pred, next_pred, pose, stream);
}
// the argument checks and the call of both box entries of a group (mirror null: nobody is mirrored)
static int group_forward_boxes(dc_group* group, const unsigned char* image, int height, int width, int is_device, const int* boxes,
                               const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w, const int* mirror,
                               float* const* prob, float* const* loc_pred, float* const* next_pred, double* const* pose, void* stream) {
  REQUIRE(group);
  if (n == 0) return DC_OK;
  REQUIRE(image);
  REQUIRE(pyramid_scales);
  return guard([&] {
    G(group)->forward_boxes(image, height, width, is_device != 0, boxes, scales, n, pyramid_scales, canvas_h, canvas_w, prob, loc_pred,
                            next_pred, pose, stream, mirror);
  });
}
int dc_group_forward_boxes(dc_group* group, const unsigned char* image, int height, int width, int is_device, const int* boxes,
                           const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w, float* const* prob,
                           float* const* loc_pred, float* const* next_pred, double* const* pose, void* stream) {
  return group_forward_boxes(group, image, height, width, is_device, boxes, scales, n, pyramid_scales, canvas_h, canvas_w, nullptr, prob,
                             loc_pred, next_pred, pose, stream);
}
// the same two on video frames (dc_frame)
int dc_group_forward_frames(dc_group* group, const dc_frame* const* frames, const int* n, const int* height, const int* width,
                            const double* scale, const int* mirror, int is_device, float* const* prob, float* const* loc_pred,
                            float* const* next_pred, double* const* pose, void* stream) {
  REQUIRE(group);
  REQUIRE(frames);
  REQUIRE(n);
  REQUIRE(height);
  REQUIRE(width);
  REQUIRE(scale);
  for (size_t c = 0; c < G(group)->nets.size(); ++c) {
    if (!frames[c]) return fail(DC_EINVAL, "null frames for group member " + std::to_string(c));
    if (n[c] <= 0 || height[c] <= 0 || width[c] <= 0 || !(scale[c] > 0)) return fail(DC_EINVAL, "bad image shape / scale for group member " + std::to_string(c));
  }
  return guard([&] {
    G(group)->forward_images(nullptr, n, height, width, scale, is_device != 0, prob, loc_pred, next_pred, pose, stream, mirror, frames);
  });
}
int dc_group_forward_boxes_frame(dc_group* group, const dc_frame* frame, int height, int width, int is_device, const int* boxes,
                                 const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w, const int* mirror,
                                 float* const* prob, float* const* loc_pred, float* const* next_pred, double* const* pose, void* stream) {
  REQUIRE(group);
  if (n == 0) return DC_OK;
  REQUIRE(frame);
  REQUIRE(pyramid_scales);
  return guard([&] {
    G(group)->forward_boxes(nullptr, height, width, is_device != 0, boxes, scales, n, pyramid_scales, canvas_h, canvas_w, prob, loc_pred,
                            next_pred, pose, stream, mirror, frame);
  });
}
// multi-scale fusion: a null `scales` is the library's to refuse (DC_EINVAL naming it), like every other argument of the rule.  The plain
// entries are the mirrored ones with no mirror table.
int dc_group_fuse_maps(dc_group* group, const double* scales, int base, int n_edges, const double* mean, const double* stdev, float* prob,
                       float* loc_pred, float* next_pred, int is_device, void* stream) {
  return dc_group_fuse_maps_mirrored(group, scales, base, nullptr, n_edges, mean, stdev, prob, loc_pred, next_pred, is_device, stream);
}
int dc_group_detect_parts(dc_group* group, const double* scales, int base, float threshold, int radius, int max_det, int* counts,
                          double* dets) {
  return dc_group_detect_parts_mirrored(group, scales, base, nullptr, threshold, radius, max_det, counts, dets);
}
int dc_group_assemble_people(dc_group* group, const double* scales, int base, const dc_assemble_params* p, int n_edges, const int* edges,
                             const double* mean, const double* stdev, const int* joint_order, int* n_people, double* people, int* cand,
                             double* cost) {
  return dc_group_assemble_people_mirrored(group, scales, base, nullptr, p, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost);
}
// mirrored members: a dc_fuse_mirror; null, or no member marked: nobody is mirrored (net_group.cpp check_mirror)
static const NetGroup::FuseMirror* mirror_args(const dc_fuse_mirror* fm, NetGroup::FuseMirror& to) {
  if (!fm) return nullptr;
  to = NetGroup::FuseMirror{fm->mirror, fm->image_width, fm->joint_mirror, fm->n_edges, fm->edges};
  return &to;
}
int dc_group_forward_images_mirrored(dc_group* group, const unsigned char* const* images, const int* n, const int* height, const int* width,
                                     const double* scale, const int* mirror, int is_device, float* const* prob, float* const* loc_pred,
                                     float* const* next_pred, void* stream) {
  return group_forward_images(group, images, n, height, width, scale, mirror, is_device, prob, loc_pred, next_pred, nullptr, stream);
}
int dc_group_fuse_maps_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, int n_edges, const double* mean,
                                const double* stdev, float* prob, float* loc_pred, float* next_pred, int is_device, void* stream) {
  REQUIRE(group);
  return guard([&] {
    NetGroup::FuseMirror m;
    G(group)->fuse_maps(scales, base, n_edges, mean, stdev, prob, loc_pred, next_pred, is_device != 0, stream, mirror_args(fm, m));
  });
}
int dc_group_detect_parts_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, float threshold, int radius,
                                   int max_det, int* counts, double* dets) {
  REQUIRE(group);
  REQUIRE(counts);
  REQUIRE(dets);
  return guard([&] {
    NetGroup::FuseMirror m;
    G(group)->detect_parts(scales, base, threshold, radius, max_det, counts, dets, mirror_args(fm, m));
  });
}
int dc_group_assemble_people_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, const dc_assemble_params* p,
                                      int n_edges, const int* edges, const double* mean, const double* stdev, const int* joint_order,
                                      int* n_people, double* people, int* cand, double* cost) {
  REQUIRE(group);
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    NetGroup::FuseMirror m;
    G(group)->assemble_people(scales, base, q, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost, mirror_args(fm, m));
  });
}
// tracking people from frame to frame (track.cpp): a dc_tracker* is a dc::Tracker*
static inline Tracker* TR(dc_tracker* t) { return reinterpret_cast<Tracker*>(t); }
int dc_tracker_create(const dc_tracker_params* p, dc_tracker** out) {
  REQUIRE(p);
  REQUIRE(out);
  *out = nullptr;
  return guard([&] {
    *out = reinterpret_cast<dc_tracker*>(
        Tracker::create(p->slots, p->max_tracks, p->n_joints, p->sigma, p->max_misses, p->min_common, p->max_dist, p->min_size, p->motion));
  });
}
int dc_tracker_destroy(dc_tracker* tracker) {
  if (!tracker) return DC_OK;
  return guard([&] { delete TR(tracker); });
}
int dc_tracker_reset(dc_tracker* tracker, int slot) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->reset(slot); });
}
int dc_tracker_update(dc_tracker* tracker, int nb, int P, const int* n_people, const double* people, long long* ids, int* place,
                      double* dist) {
  return dc_tracker_update_slots(tracker, nb, P, nullptr, n_people, people, ids, place, dist);
}
int dc_tracker_update_slots(dc_tracker* tracker, int nb, int P, const int* slot_of, const int* n_people, const double* people,
                            long long* ids, int* place, double* dist) {
  REQUIRE(tracker);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(ids);
  return guard([&] { TR(tracker)->update(nb, P, slot_of, n_people, people, ids, place, dist); });
}
int dc_tracker_state(dc_tracker* tracker, int slot, long long* ids, int* misses, int* hits, double* poses) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->state(slot, ids, misses, hits, poses); });
}
int dc_tracker_set_option(dc_tracker* tracker, int key, int value) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->set_option(key, value); });
}
int dc_tracker_get_option(dc_tracker* tracker, int key, int* value) {
  REQUIRE(tracker);
  REQUIRE(value);
  return guard([&] { *value = TR(tracker)->get_option(key); });
}
int dc_tracker_set_smoothing(dc_tracker* tracker, const dc_track_smooth_params* p) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->set_smoothing(p); });
}
int dc_tracker_get_smoothing(dc_tracker* tracker, dc_track_smooth_params* out) {
  REQUIRE(tracker);
  REQUIRE(out);
  return guard([&] {
    const Tracker::SmoothParams& q = TR(tracker)->smooth;
    *out = dc_track_smooth_params{q.enabled, q.min_cutoff, q.beta, q.d_cutoff, q.max_hold};
  });
}
int dc_tracker_update_smoothed(dc_tracker* tracker, int nb, int P, const int* slot_of, const int* n_people, const double* people,
                               long long* ids, int* place, double* dist, double* smooth, int* src) {
  REQUIRE(tracker);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(ids);
  return guard([&] { TR(tracker)->update(nb, P, slot_of, n_people, people, ids, place, dist, smooth, src, true); });
}
int dc_tracker_smooth_state(dc_tracker* tracker, int slot, double* poses, int* gap) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->smooth_state(slot, poses, gap); });
}
// the tracker's appearance steps (track.cpp)
int dc_tracker_set_appearance(dc_tracker* tracker, const dc_track_appearance_params* p) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->set_appearance(p); });
}
int dc_tracker_get_appearance(dc_tracker* tracker, dc_track_appearance_params* out) {
  REQUIRE(tracker);
  REQUIRE(out);
  return guard([&] {
    const Tracker::AppearParams& q = TR(tracker)->appear;
    *out = dc_track_appearance_params{q.enabled, q.min_pixels, q.alpha256, q.reid_max, q.max_age, q.min_hits};
  });
}
int dc_tracker_update_appearance(dc_tracker* tracker, int nb, int P, const int* slot_of, const int* n_people, const double* people,
                                 const int* desc, long long* ids, int* place, double* dist, int* reid, double* smooth, int* src) {
  REQUIRE(tracker);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(ids);
  return guard([&] { TR(tracker)->update(nb, P, slot_of, n_people, people, ids, place, dist, smooth, src, false, true, desc, reid); });
}
int dc_tracker_appearance_state(dc_tracker* tracker, int slot, int* track_model, int* track_valid, long long* gallery_ids, int* gallery_age,
                                int* gallery_model) {
  REQUIRE(tracker);
  return guard([&] { TR(tracker)->appearance_state(slot, track_model, track_valid, gallery_ids, gallery_age, gallery_model); });
}
int dc_net_track_people(dc_net* net, dc_tracker* tracker, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean,
                        const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, double* cost,
                        long long* ids, int* place) {
  return dc_net_track_people_slots(net, tracker, nullptr, p, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost, ids, place);
}
int dc_net_track_people_slots(dc_net* net, dc_tracker* tracker, const int* slot_of, const dc_assemble_params* p, int n_edges,
                              const int* edges, const double* mean, const double* stdev, const int* joint_order, int* n_people,
                              double* people, int* cand, double* cost, long long* ids, int* place) {
  REQUIRE(net);
  REQUIRE(tracker);
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(ids);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    N(net)->assemble_people(q, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost, TR(tracker), ids, place, slot_of);
  });
}
int dc_group_track_people(dc_group* group, dc_tracker* tracker, const double* scales, int base, const dc_fuse_mirror* fm,
                          const dc_assemble_params* p, int n_edges, const int* edges, const double* mean, const double* stdev,
                          const int* joint_order, int* n_people, double* people, int* cand, double* cost, long long* ids, int* place) {
  return dc_group_track_people_slots(group, tracker, nullptr, scales, base, fm, p, n_edges, edges, mean, stdev, joint_order, n_people, people,
                                     cand, cost, ids, place);
}
int dc_group_track_people_slots(dc_group* group, dc_tracker* tracker, const int* slot_of, const double* scales, int base,
                                const dc_fuse_mirror* fm, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean,
                                const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, double* cost,
                                long long* ids, int* place) {
  REQUIRE(group);
  REQUIRE(tracker);
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(ids);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    NetGroup::FuseMirror m;
    G(group)->assemble_people(scales, base, q, n_edges, edges, mean, stdev, joint_order, n_people, people, cand, cost, mirror_args(fm, m),
                              TR(tracker), ids, place, slot_of);
  });
}
int dc_net_track_frames_async(dc_net* net, dc_tracker* tracker, const dc_frame* frames, const unsigned char* images, int n, int height,
                              int width, double scale, int is_device, const int* slot_of, const dc_assemble_params* p, int n_edges,
                              const int* edges, const double* mean, const double* stdev, const int* joint_order, int* n_people,
                              double* people, int* cand, long long* ids, int* place) {
  REQUIRE(net);
  if (!frames) REQUIRE(images);
  if (n <= 0 || height <= 0 || width <= 0) return fail(DC_EINVAL, "n, height and width must be positive");
  if (!(scale > 0)) return fail(DC_EINVAL, "scale must be positive");
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    N(net)->track_frames_async(tracker ? TR(tracker) : nullptr, frames, images, n, height, width, scale, is_device != 0, slot_of, q, n_edges,
                               edges, mean, stdev, joint_order, n_people, people, cand, ids, place);
  });
}
// stage D of the people assembly: state of the net / the group, checked here with no device (CompleteParams::checked, people.cpp)
static void completion_out(const CompleteParams& c, dc_complete_params* out) {
  out->enabled = c.enabled;
  out->fill_threshold = c.fill_threshold;
  out->fill_radius = c.fill_radius;
  out->min_support = c.min_support;
}
int dc_net_set_completion(dc_net* net, const dc_complete_params* p) {
  REQUIRE(net);
  return guard([&] { N(net)->completion = CompleteParams::checked(p); });
}
int dc_net_get_completion(dc_net* net, dc_complete_params* out) {
  REQUIRE(net);
  REQUIRE(out);
  completion_out(N(net)->completion, out);
  return DC_OK;
}
int dc_group_set_completion(dc_group* group, const dc_complete_params* p) {
  REQUIRE(group);
  return guard([&] { G(group)->completion = CompleteParams::checked(p); });
}
int dc_group_get_completion(dc_group* group, dc_complete_params* out) {
  REQUIRE(group);
  REQUIRE(out);
  completion_out(G(group)->completion, out);
  return DC_OK;
}
// stage E of the people assembly: state of the net / the group like stage D's (DedupeParams::checked, people.cpp)
static void dedupe_out(const DedupeParams& d, dc_dedupe_params* out, double* sigma_out) {
  out->enabled = d.enabled;
  out->max_dist = d.max_dist;
  out->min_common = d.min_common;
  out->min_size = d.min_size;
  out->n_sigma = d.n_sigma;
  out->absorb = d.absorb;
  for (int j = 0; sigma_out && j < kPeopleMaxJoints; ++j) sigma_out[j] = d.sigma[j];
}
int dc_net_set_dedupe(dc_net* net, const dc_dedupe_params* p) {
  REQUIRE(net);
  return guard([&] { N(net)->dedupe = DedupeParams::checked(p, "set_dedupe"); });
}
int dc_net_get_dedupe(dc_net* net, dc_dedupe_params* out, double* sigma_out) {
  REQUIRE(net);
  REQUIRE(out);
  dedupe_out(N(net)->dedupe, out, sigma_out);
  return DC_OK;
}
int dc_group_set_dedupe(dc_group* group, const dc_dedupe_params* p) {
  REQUIRE(group);
  return guard([&] { G(group)->dedupe = DedupeParams::checked(p, "set_dedupe"); });
}
int dc_group_get_dedupe(dc_group* group, dc_dedupe_params* out, double* sigma_out) {
  REQUIRE(group);
  REQUIRE(out);
  dedupe_out(G(group)->dedupe, out, sigma_out);
  return DC_OK;
}
int dc_dedupe_people(const dc_dedupe_params* p, int nb, int P, int J, const int* n_people, const double* people, const int* cand, int* n_out,
                     double* people_out, int* cand_out, int* kept_from, int* suppressed_by) {
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(n_out);
  REQUIRE(people_out);
  return guard([&] { dedupe_people(p, nb, P, J, n_people, people, cand, n_out, people_out, cand_out, kept_from, suppressed_by); });
}
// the skeleton overlay (draw.cpp)
int dc_draw_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                   const double* people, const int* cand, const long long* ids, const dc_draw_style* style, void* stream) {
  REQUIRE(frames);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(style);
  return guard([&] { draw_people(frames, nb, height, width, is_device != 0, P, J, n_people, people, cand, ids, style, stream); });
}
int dc_draw_limits(int* tile_w, int* tile_h, int* chunk) {
  draw_limits(tile_w, tile_h, chunk);
  return DC_OK;
}
// the redaction (redact.cpp); a null style is refused there, after the frames' own checks, naming the field
int dc_redact_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                     const double* people, const unsigned char* select, const dc_redact_style* style, int* redacted, void* stream) {
  REQUIRE(frames);
  REQUIRE(n_people);
  REQUIRE(people);
  return guard([&] { redact_people(frames, nb, height, width, is_device != 0, P, J, n_people, people, select, style, redacted, stream); });
}
// the appearance descriptor (appearance.cpp); a null style is refused there, after the frames' own checks, naming the field
int dc_describe_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                       const double* people, const dc_appearance_style* style, int* desc, void* stream) {
  REQUIRE(frames);
  REQUIRE(n_people);
  REQUIRE(people);
  REQUIRE(desc);
  return guard([&] { describe_people(frames, nb, height, width, is_device != 0, P, J, n_people, people, style, desc, stream); });
}
// the overlays from people in device memory (overlay.cpp, people.cpp); a call without a style is refused there, naming the field
// dc_overlay_styles as the caller compiled it -> OverlayArgs: fields beyond the caller's `size` read as NULL / no list
static OverlayArgs overlay_args(const char* who, const dc_overlay_styles* st, int* redacted, bool styles_entry = true) {
  OverlayArgs a;
  a.redacted = redacted, a.styles_entry = styles_entry;
  if (!st) return a;  // no style at all: refused, or the plain chain, where the entry decides
  if (st->size < offsetof(dc_overlay_styles, redact) + sizeof(st->redact) || st->size > sizeof(dc_overlay_styles))
    throw DcError(DC_EINVAL, std::string(who) + ": styles.size = " + std::to_string(st->size) + " must be sizeof(dc_overlay_styles) of the caller, in [" +
                                 std::to_string(offsetof(dc_overlay_styles, redact) + sizeof(st->redact)) + ", " +
                                 std::to_string(sizeof(dc_overlay_styles)) + "]");
  auto has = [&](size_t end) { return st->size >= end; };
  a.draw = st->draw, a.redact = st->redact;
  if (has(offsetof(dc_overlay_styles, labels) + sizeof(st->labels))) a.labels = st->labels;
  if (has(offsetof(dc_overlay_styles, n_only) + sizeof(st->n_only))) a.only_ids = st->only_ids, a.n_only = st->n_only;
  if (has(offsetof(dc_overlay_styles, n_keep) + sizeof(st->n_keep))) a.keep_ids = st->keep_ids, a.n_keep = st->n_keep;
  return a;
}
// the older entries' arguments as a styles block, and their refusals' words
static dc_overlay_styles overlay_styles(const dc_draw_style* draw, const dc_redact_style* redact, const long long* only_ids, int n_only,
                                        const long long* keep_ids, int n_keep) {
  dc_overlay_styles st{};
  st.size = sizeof st, st.draw = draw, st.redact = redact, st.labels = nullptr;
  st.only_ids = only_ids, st.n_only = n_only, st.keep_ids = keep_ids, st.n_keep = n_keep;
  return st;
}
// both device entries; styles_entry: the refusal of a call without any style names the label style too
static int overlay_device_entry(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                                const double* people, const int* cand, const long long* ids, const dc_overlay_styles* styles, int* redacted,
                                void* stream, bool styles_entry) {
  REQUIRE(frames);
  REQUIRE(n_people);
  REQUIRE(people);
  return guard([&] {
    overlay_people_device(frames, nb, height, width, is_device != 0, P, J, n_people, people, cand, ids,
                          overlay_args("overlay_people_device", styles, redacted, styles_entry), stream);
  });
}
int dc_overlay_people_device_styles(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                                    const double* people, const int* cand, const long long* ids, const dc_overlay_styles* styles,
                                    int* redacted, void* stream) {
  return overlay_device_entry(frames, nb, height, width, is_device, P, J, n_people, people, cand, ids, styles, redacted, stream, true);
}
int dc_overlay_people_device(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                             const double* people, const int* cand, const long long* ids, const dc_draw_style* draw,
                             const dc_redact_style* redact, const long long* only_ids, int n_only, const long long* keep_ids, int n_keep,
                             int* redacted, void* stream) {
  const dc_overlay_styles st = overlay_styles(draw, redact, only_ids, n_only, keep_ids, n_keep);
  return overlay_device_entry(frames, nb, height, width, is_device, P, J, n_people, people, cand, ids, &st, redacted, stream, false);
}
// the label overlay (label.cpp); a null style is refused there, after the frames' own checks, naming the field
int dc_label_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                    const double* people, const long long* ids, const char* texts, const dc_label_style* style, void* stream) {
  REQUIRE(frames);
  REQUIRE(n_people);
  REQUIRE(people);
  return guard([&] { label_people(frames, nb, height, width, is_device != 0, P, J, n_people, people, ids, texts, style, stream); });
}
int dc_label_font(int ch, unsigned char rows[7]) {
  return guard([&] { label_font(ch, rows); });
}
int dc_net_track_frames_async_overlay(dc_net* net, dc_tracker* tracker, const dc_frame* frames, const unsigned char* images, int n, int height,
                                      int width, double scale, int is_device, const int* slot_of, const dc_assemble_params* p, int n_edges,
                                      const int* edges, const double* mean, const double* stdev, const int* joint_order, int* n_people,
                                      double* people, int* cand, long long* ids, int* place, const dc_draw_style* draw,
                                      const dc_redact_style* redact, const long long* only_ids, int n_only, const long long* keep_ids,
                                      int n_keep, int* redacted) {
  const dc_overlay_styles st = overlay_styles(draw, redact, only_ids, n_only, keep_ids, n_keep);
  return dc_net_track_frames_async_styles(net, tracker, frames, images, n, height, width, scale, is_device, slot_of, p, n_edges, edges, mean, stdev,
                                          joint_order, n_people, people, cand, ids, place, &st, redacted);
}
int dc_net_track_frames_async_styles(dc_net* net, dc_tracker* tracker, const dc_frame* frames, const unsigned char* images, int n, int height,
                                     int width, double scale, int is_device, const int* slot_of, const dc_assemble_params* p, int n_edges,
                                     const int* edges, const double* mean, const double* stdev, const int* joint_order, int* n_people,
                                     double* people, int* cand, long long* ids, int* place, const dc_overlay_styles* styles, int* redacted) {
  REQUIRE(net);
  if (!frames) REQUIRE(images);
  if (n <= 0 || height <= 0 || width <= 0) return fail(DC_EINVAL, "n, height and width must be positive");
  if (!(scale > 0)) return fail(DC_EINVAL, "scale must be positive");
  REQUIRE(p);
  REQUIRE(n_people);
  REQUIRE(people);
  if (n_edges > 0) REQUIRE(edges);
  return guard([&] {
    Net::AssembleParams q{p->scale, p->threshold, p->radius, p->max_det, p->max_cost, p->seed_threshold, p->max_people, p->min_joints};
    const OverlayArgs a = overlay_args("track_frames_async", styles, redacted);
    N(net)->track_frames_async(tracker ? TR(tracker) : nullptr, frames, images, n, height, width, scale, is_device != 0, slot_of, q, n_edges,
                               edges, mean, stdev, joint_order, n_people, people, cand, ids, place, &a);
  });
}
// the score-map overlay (heat.cpp); null geometry / style / map are refused there, after the frames' own checks, naming the field
int dc_draw_heatmap(const dc_frame* frames, int nb, int height, int width, int is_device, const float* map, int map_is_device, int C, int Hm,
                    int Wm, const dc_heat_geometry* geometry, const dc_heat_style* style, void* stream) {
  REQUIRE(frames);
  return guard([&] { draw_heatmap(frames, nb, height, width, is_device != 0, map, map_is_device != 0, C, Hm, Wm, geometry, style, stream); });
}
int dc_net_draw_heatmap(dc_net* net, const dc_frame* frames, int nb, int height, int width, int is_device, const dc_heat_geometry* geometry,
                        const dc_heat_style* style) {
  REQUIRE(net);
  REQUIRE(frames);
  return guard([&] { N(net)->draw_heatmap(frames, nb, height, width, is_device != 0, geometry, style); });
}
int dc_group_draw_heatmap(dc_group* group, const dc_frame* frames, int nb, int height, int width, int is_device, const double* scales, int base,
                          double origin_x, double origin_y, const dc_heat_style* style) {
  return dc_group_draw_heatmap_mirrored(group, frames, nb, height, width, is_device, scales, base, nullptr, origin_x, origin_y, style);
}
int dc_group_draw_heatmap_mirrored(dc_group* group, const dc_frame* frames, int nb, int height, int width, int is_device, const double* scales,
                                   int base, const dc_fuse_mirror* fm, double origin_x, double origin_y, const dc_heat_style* style) {
  REQUIRE(group);
  REQUIRE(frames);
  return guard([&] {
    NetGroup::FuseMirror m;
    G(group)->draw_heatmap(frames, nb, height, width, is_device != 0, scales, base, origin_x, origin_y, style, mirror_args(fm, m));
  });
}
// single-person and box poses from the fused maps (net_group.cpp decode_pose / decode_boxes)
int dc_group_decode_pose(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, double* pose, int is_device, void* stream) {
  REQUIRE(group);
  REQUIRE(pose);
  return guard([&] {
    NetGroup::FuseMirror m;
    G(group)->decode_pose(scales, base, pose, is_device != 0, stream, mirror_args(fm, m));
  });
}
int dc_group_forward_boxes_mirrored(dc_group* group, const unsigned char* image, int height, int width, int is_device, const int* boxes,
                                    const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w, const int* mirror,
                                    float* const* prob, float* const* loc_pred, float* const* next_pred, void* stream) {
  return group_forward_boxes(group, image, height, width, is_device, boxes, scales, n, pyramid_scales, canvas_h, canvas_w, mirror, prob,
                             loc_pred, next_pred, nullptr, stream);
}
int dc_group_decode_boxes(dc_group* group, const double* pyramid_scales, int base, const dc_fuse_mirror* fm, float* prob, float* loc_pred,
                          double* pose, int is_device, void* stream) {
  REQUIRE(group);
  return guard([&] {
    NetGroup::FuseMirror m;
    G(group)->decode_boxes(pyramid_scales, base, prob, loc_pred, pose, is_device != 0, stream, mirror_args(fm, m));
  });
}
int dc_comm_create(int nexec, const int* devices, int transport, dc_comm** out) {
  REQUIRE(out);
  *out = nullptr;
  return guard([&] { *out = reinterpret_cast<dc_comm*>(comm_create(nexec, devices, transport)); });
}
int dc_comm_destroy(dc_comm* comm) {
  if (!comm) return DC_OK;
  return guard([&] { comm_destroy(reinterpret_cast<Comm*>(comm)); });
}
int dc_comm_transport(dc_comm* comm) {
  if (!comm) return fail(DC_EINVAL, "null argument: comm");
  return comm_transport(reinterpret_cast<Comm*>(comm));
}
int dc_forward_batch(dc_comm* comm, dc_net* const* nets, int nexec, const float* const* inputs, const int (*hw)[2], int n,
                     float* const* prob, float* const* loc, float* const* next) {
  REQUIRE(comm);
  REQUIRE(nets);
  if (nexec < 1) return fail(DC_EINVAL, "dc_forward_batch: no executors");
  return guard([&] {
    std::vector<Net*> v;
    for (int k = 0; k < nexec; ++k) v.push_back(N(nets[k]));
    comm_forward(reinterpret_cast<Comm*>(comm), v.data(), nexec, inputs, hw, n, prob, loc, next);
  });
}
int dc_comm_item_executor(dc_comm* comm, int i) {
  if (!comm) return fail(DC_EINVAL, "null argument: comm");
  int r = -1;
  int rc = guard([&] { r = comm_item_executor(reinterpret_cast<Comm*>(comm), i); });
  return rc == DC_OK ? r : rc;
}
int dc_comm_root_maps(dc_comm* comm, int i, const void** prob, const void** loc, const void** next, int dims[5]) {
  REQUIRE(comm);
  return guard([&] { comm_root_maps(reinterpret_cast<Comm*>(comm), i, prob, loc, next, dims); });
}
int dc_lpt_schedule(const double* cost, int n, int nexec, int* exec_of_item) {
  if (n < 0 || nexec < 1) return fail(DC_EINVAL, "dc_lpt_schedule: n >= 0 items on nexec >= 1 executors");
  if (n == 0) return DC_OK;
  REQUIRE(cost);
  REQUIRE(exec_of_item);
  return guard([&] {
    const auto share = lpt_schedule(std::vector<double>(cost, cost + n), nexec);
    for (int k = 0; k < nexec; ++k)
      for (int i : share[(size_t)k]) exec_of_item[i] = k;
  });
}

const char* dc_group_plan_text(dc_group* group) {
  if (!group) return nullptr;
  NetGroup* g = G(group);
  int rc = guard([&] { g->text_buf = g->plan_text(); });
  return rc == DC_OK ? g->text_buf.c_str() : nullptr;
}
const char* dc_group_profile_text(dc_group* group, int iters) {
  if (!group) return nullptr;
  NetGroup* g = G(group);
  int rc = guard([&] { g->text_buf = g->profile_text(iters > 0 ? iters : 10); });
  return rc == DC_OK ? g->text_buf.c_str() : nullptr;
}
const char* dc_group_tune_report(dc_group* group) {
  if (!group) return nullptr;
  NetGroup* g = G(group);
  int rc = guard([&] { g->text_buf = g->tune_report_text(); });
  return rc == DC_OK ? g->text_buf.c_str() : nullptr;
}
int dc_group_set_tile(dc_group* group, const char* signature, const char* tile) {
  REQUIRE(group);
  REQUIRE(signature);
  REQUIRE(tile);
  return guard([&] { G(group)->set_tile(signature, tile); });
}
int dc_group_stats(dc_group* group, long long* out, int n) {
  REQUIRE(group);
  REQUIRE(out);
  NetGroup* g = G(group);
  const long long v[DC_NUM_GSTATS] = {g->stats.merges, g->stats.graph_instantiations, g->stats.autotune_runs, g->stats.plan_hits,
                                      (long long)g->num_launches(), (long long)g->num_multi_launches(), (long long)g->lanes()};
  for (int i = 0; i < n && i < DC_NUM_GSTATS; ++i) out[i] = v[i];
  return DC_OK;
}
int dc_group_flops(dc_group* group, double* out) {
  REQUIRE(group);
  REQUIRE(out);
  *out = G(group)->flops();
  return DC_OK;
}

}  // extern "C"
