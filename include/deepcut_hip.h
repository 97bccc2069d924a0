/*
 * deepcut_hip.h — C ABI of libdeepcut_hip.so, the MI355X (gfx950) forward path of the
 * DeeperCut part detector.
 *
 * This is the drop-in boundary for the ONE hot path of eldar/deepcut-cnn: the TEST-phase
 * forward of models/deepercut/ResNet-152.prototxt behind caffe::Net::ForwardFromTo /
 * pycaffe net.forward().  The reference has no C ABI (it binds C++ to Python through
 * Boost.Python, python/caffe/_caffe.cpp); every entry point below names the reference
 * interface it stands in for (file:line relative to the reference tree).  A maintainer
 * binds these with ctypes / pybind / Boost.Python exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DC_E* code on failure; the message is
 *     available from dc_last_error() (thread local).  Nothing aborts the process (the
 *     reference LOG(FATAL)s; we never continue silently either).
 *   - handles are opaque; a dc_blob* is owned by its net (or, for dc_blob_create, by the
 *     caller) and stays valid until that owner is destroyed.
 *   - host tensors are float32, C-contiguous NCHW exactly as caffe::Blob (blob.hpp:153-164).
 *     Device tensors are channels-last (NHWC) float32; see DESIGN.md "Data layout in HBM".
 *   - mode/device are per thread, like caffe::Caffe (common.cpp:13-20).
 *   - there is NO CPU compute path in this library: dc_net_forward in CPU mode fails with
 *     DC_ENOCPU.  The CPU restatement of the reference lives in oracle/ and is test-only.
 */
#ifndef DEEPCUT_HIP_H_
#define DEEPCUT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_OK 0
#define DC_EINVAL (-1)   /* bad argument / malformed model                         */
#define DC_EIO (-2)      /* "Could not open file ..." (_caffe.cpp:45-52)            */
#define DC_ESHAPE (-3)   /* shape / blob-count mismatch (net.cpp:822-834)           */
#define DC_EUNSUP (-4)   /* layer type or parameter outside the supported path      */
#define DC_EDEVICE (-5)  /* HIP runtime error / no gfx950 device                    */
#define DC_ENOCPU (-6)   /* forward requested in CPU mode: not provided             */

#define DC_MODE_CPU 0 /* caffe::Caffe::CPU (common.hpp:107) */
#define DC_MODE_GPU 1 /* caffe::Caffe::GPU                  */
#define DC_PHASE_TRAIN 0 /* caffe.proto:253-256 */
#define DC_PHASE_TEST 1

/* dc_net_set_option keys */
#define DC_OPT_FUSE 1       /* 0: every named blob materialised (Caffe-visible semantics);
                               1: + residual-add and Deconvolution+Crop+Eltwise head fusion;
                               2 (default): + the sibling heads run as one concatenated GEMM     */
#define DC_OPT_HIPGRAPH 2   /* 1: replay the per-shape launch sequence as a hipGraph        */
#define DC_OPT_DTYPE 3      /* 0 (default): float32 activations and filters in HBM, v_mfma_f32_32x32x2_f32;
                               1: float16 activations and filters, v_mfma_f32_32x32x16_f16 with float32
                               accumulation and epilogue (BASELINE configs[2]);
                               2: bfloat16 activations and filters (float32's exponent range: no overflow where
                               float32 has none), v_mfma_f32_32x32x16_bf16 with float32 accumulation and epilogue,
                               the direct gather-GEMM tiles only (no Winograd / streaming / stem forms);
                               host blobs stay float32 */

#define DC_OPT_OUTPUTS 4    /* bit i set = the i-th output blob of the net (dc_net_num_outputs order: alphabetical, net.cpp:268-273) is wanted;
                               default -1 = all.  The lowering drops every launch that only feeds unwanted outputs (the demo reads `prob`
                               and `loc_pred` only, python/pose/estimate_pose.py:231-241, and the 364-channel `next_pred` head is 23.3 of the
                               241 GFLOP of a 544x736 forward); an unwanted output blob is elided: reading it is DC_EUNSUP.  The wanted
                               maps equal the full forward's up to the summation order of the tile chosen for the narrower head GEMM
                               (bit for bit under the same tile, tests/test_gpu_outputs.py) */

#define DC_OPT_SPARSE_PAIRWISE 5 /* 0 (default): nothing changes anywhere.  1: on a net whose DC_OPT_OUTPUTS leaves `next_pred` out,
                               dc_net_assemble_people, dc_net_decode_pairwise and dc_net_pairwise_at evaluate the pairwise head at the
                               cells they read instead of answering DC_EUNSUP (the rule: dc_net_pairwise_at); a net whose plan computes
                               `next_pred` reads the dense map, same bits as with 0.  Inherited by clones.  Setting 1 on a net without
                               a recognisable pairwise head is DC_EUNSUP naming the layer.  dc_group_* entries do not look at it. */

typedef struct dc_net dc_net;
typedef struct dc_blob dc_blob;

/* ---- error / context ---------------------------------------------------------------- */
const char* dc_last_error(void);
const char* dc_version(void);

/* Caffe::set_mode / Caffe::mode  (common.hpp:148-150; _caffe.cpp:38-39)                  */
int dc_set_mode(int mode);
int dc_get_mode(void);
/* Caffe::SetDevice (common.cpp:140-158; _caffe.cpp:221)                                  */
int dc_set_device(int device_id);
int dc_get_device(void);
/* number of visible HIP devices (0 when there is no GPU; never fails)                    */
int dc_device_count(void);

/* ---- Net ------------------------------------------------------------------------------ */
/* Net<float>::Net(param_file, phase) + CopyTrainedLayersFrom(weights)
 * (net.cpp:31-37,843-858; _caffe.cpp:76-96).  caffemodel may be NULL.                    */
int dc_net_create(const char* prototxt_path, const char* caffemodel_path, int phase, dc_net** out);
/* same, from an in-memory prototxt string                                                */
int dc_net_create_from_text(const char* prototxt_text, const char* caffemodel_path, int phase,
                            dc_net** out);
int dc_net_destroy(dc_net* net);
/* A second executor of the same model on the same device: own activations / stream / hipGraph, SHARED
 * parameter blobs and packed filter images (no reference counterpart; Net::ShareTrainedLayersWith,
 * net.cpp:751-769, is the nearest idea).  Used to keep several independent forwards in flight.           */
int dc_net_clone(dc_net* net, dc_net** out);
/* wait for everything enqueued on the net's own stream (see DC_STREAM_OWN)                                */
int dc_net_synchronize(dc_net* net);
/* non-blocking: *busy = 1 while work enqueued on the net's own stream (DC_STREAM_OWN) has not finished, else 0 — what a
 * dispatcher polls to hand queued requests to whichever executor is free (deepcut_tools.Pipeline); no reference counterpart  */
int dc_net_busy(dc_net* net, int* busy);
int dc_net_set_option(dc_net* net, int key, int value);
int dc_net_get_option(dc_net* net, int key, int* value);
/* Net::CopyTrainedLayersFrom(file) (net.cpp:805-858): match by layer name, check blob
 * count and shape, ignore unmatched source layers.  Formats: binary NetParameter in the current
 * `layer` form or the deprecated V1 / V0 `layers` form (upgraded as upgrade_proto.cpp:19-78 does),
 * and — for names ending in ".h5", the reference's rule (net.cpp:843-850) — HDF5 weights
 * /data/<layer>/<param index> (CopyTrainedLayersFromHDF5, net.cpp:861-909).                     */
int dc_net_copy_from(dc_net* net, const char* caffemodel_path);
/* Net::ToProto + WriteProtoToBinaryFile (net.cpp:910-925; _caffe.cpp:98-102)             */
int dc_net_save(dc_net* net, const char* caffemodel_path);
const char* dc_net_name(dc_net* net);

/* Net::layer_names / layers()[i]->type() (net.hpp:126-133), AFTER InsertSplits           */
int dc_net_num_layers(dc_net* net);
const char* dc_net_layer_name(dc_net* net, int i);
const char* dc_net_layer_type(dc_net* net, int i);
/* Net::blob_names / blobs (net.hpp:122-125,135), creation order, split blobs included    */
int dc_net_num_blobs(dc_net* net);
const char* dc_net_blob_name(dc_net* net, int i);
/* Net::blob_by_name (net.cpp:947-957); unknown name -> DC_EINVAL                         */
int dc_net_blob(dc_net* net, const char* name, dc_blob** out);
/* Net::input_blob_indices / output_blob_indices (net.hpp:182-189): outputs are the
 * unconsumed blobs in alphabetical order (net.cpp:268-273)                               */
int dc_net_num_inputs(dc_net* net);
const char* dc_net_input_name(dc_net* net, int i);
int dc_net_num_outputs(dc_net* net);
const char* dc_net_output_name(dc_net* net, int i);
/* Net::layers()[i]->blobs()[j]  (pycaffe net.params, pycaffe.py:40-51)                   */
int dc_net_layer_num_params(dc_net* net, const char* layer_name);
int dc_net_param(dc_net* net, const char* layer_name, int idx, dc_blob** out);

/* Net::Reshape (net.cpp:744-749): propagate the current input shapes                     */
int dc_net_reshape(dc_net* net);
/* Net::ForwardFromTo(start, end) (net.cpp:565-581; _caffe.cpp:231 "_forward").  Layer
 * indices are those of dc_net_layer_name.  Re-derives every shape from the current input
 * shape (Layer::Forward calls Reshape, layer.hpp:451-456).  Synchronous: on return all
 * outputs are computed.  *loss (may be NULL) receives 0 (no loss layers on this path).   */
int dc_net_forward(dc_net* net, int start, int end, float* loss);
/* Net::ForwardPrefilled convenience: whole net                                           */
int dc_net_forward_all(dc_net* net);

/* ---- Blob (caffe::Blob<float> + SyncedMemory) ----------------------------------------- */
/* Blob::shape (blob.hpp:52-71).  dims must hold 4 ints (params may have 1 axis)          */
int dc_blob_num_axes(dc_blob* b);
int dc_blob_shape(dc_blob* b, int* ndim, int* dims /*[8]*/);
int dc_blob_count(dc_blob* b);
/* Blob::Reshape (blob.cpp:23-43; _caffe.cpp:181-193): capacity only grows                */
int dc_blob_reshape(dc_blob* b, int ndim, const int* dims);
/* Blob::cpu_data / mutable_cpu_data (blob.cpp:82-86,105-109 -> syncedmem.cpp:25-77,
 * 103-128).  The pointer is host memory owned by the blob, NCHW, valid until a reshape
 * grows the blob or the owner is destroyed.  mutable_: host becomes authoritative
 * (HEAD_AT_CPU) so the next forward re-uploads; a pending device result is downloaded first. */
int dc_blob_cpu_data(dc_blob* b, const float** out);
int dc_blob_mutable_cpu_data(dc_blob* b, float** out);
/* SyncedMemory::head() (syncedmem.hpp:59): 0 UNINITIALIZED 1 HEAD_AT_CPU 2 HEAD_AT_GPU 3 SYNCED */
int dc_blob_head(dc_blob* b);
/* Blob::gpu_data (blob.cpp:88-92): device pointer of the channels-last (NHWC) image of the
 * blob, plus its channel pitch (>= channels; the 3-channel input is stored with pitch 4).
 * Its elements are the net's DC_OPT_DTYPE: float32, float16, or on a bf16 net (2) the bfloat16
 * values as they are in HBM (pitch rounded to 8 elements like float16's).  Same for the mutable form. */
int dc_blob_gpu_data(dc_blob* b, const void** dev_ptr, int* channel_pitch);

/* Blob<float>() / Blob<float>(shape) (blob.hpp:26-33): a blob of its own, owned by the caller — the bottoms and tops a
 * stand-alone Layer is driven with, or the backing store of a caffe::SyncedMemory.  It moves between host and device on
 * the default stream of the calling thread's device (Caffe::SetDevice).  dc_blob_destroy refuses a net's blob.       */
int dc_blob_create(int ndim, const int* dims, dc_blob** out);
int dc_blob_destroy(dc_blob* b);
/* Blob::mutable_gpu_data (blob.cpp:111-115 -> SyncedMemory::mutable_gpu_data, syncedmem.cpp:130-139): the device image
 * (channels-last for 4-D blobs, plain otherwise) becomes authoritative (HEAD_AT_GPU); an UNINITIALIZED blob gets a
 * zeroed image, a host-side one is uploaded first.  Refused for blobs a fused plan never materialises.            */
int dc_blob_mutable_gpu_data(dc_blob* b, void** dev_ptr, int* channel_pitch);
/* Blob::CopyFrom(source, copy_diff=false, reshape) (blob.cpp:435-474): copies wherever the source is authoritative —
 * host to host, or device image to device image (re-pitched) leaving dst HEAD_AT_GPU.  Shapes must agree unless
 * `reshape`.                                                                                                      */
int dc_blob_copy_from(dc_blob* dst, dc_blob* src, int reshape);

/* ---- one reference layer stand-alone: Layer<Dtype>::SetUp(bottom, top) (layer.hpp:67-74) ---------------------------
 * layer_param_text: the text-format LayerParameter (the body of a `layer { }` message, or the message itself).  The
 * result is a net whose inputs are the layer's bottoms (named as in the text, shaped like `bottoms`), with DC_OPT_FUSE 0:
 * Layer::Reshape = dc_blob_reshape on its inputs + dc_net_reshape, Layer::Forward_gpu = dc_net_forward_all, the layer's
 * blobs() = dc_net_param(net, <layer name>, i).  include/caffe_facade.hpp wraps this as caffe::Layer<float>.        */
int dc_net_create_for_layer(const char* layer_param_text, int phase, int nbottom, dc_blob* const* bottoms, dc_net** out);

/* ---- batched / sharded extension (no reference counterpart: the reference forwards one
 * image at a time, conv_layer.cpp:31).  Runs `n` same-shape images as one batch:
 * inputs  : host or device NCHW float32 [n,3,H,W] (is_device selects)
 * outputs : prob [n,14,h,w], loc_pred [n,28,h,w], next_pred [n,364,h,w] NCHW float32, host or
 *           device like the input; any of them may be NULL to skip the copy-out.
 * stream  : hipStream_t to enqueue on.  NULL = the net's own stream, synchronous.  DC_STREAM_OWN = the
 *           net's own stream, asynchronous for device buffers (pair with dc_net_synchronize).  With a
 *           caller stream and device buffers the call is asynchronous on that stream.              */
#define DC_STREAM_OWN ((void*)-1)
int dc_net_forward_batch(dc_net* net, const float* input, int n, int h, int w, int is_device,
                         float* prob, float* loc_pred, float* next_pred, void* stream);

/* The same with HOST buffers and NO wait: the upload of the batch, the forward and the downloads of the maps are enqueued on the
 * net's own stream; dc_net_synchronize (or dc_net_busy) tells when the outputs are there, and input and outputs must stay valid
 * until then.  With buffers from dc_host_alloc (pinned) the copies run on the DMA engines beside other executors' kernels, which is
 * what lets several executors keep host-in / host-out requests in flight (deepcut_tools.Pipeline.submit_host); pageable buffers
 * work too, staged by the runtime.  Replaces the blocking copies of SyncedMemory::to_gpu / to_cpu (src/caffe/syncedmem.cpp:25-77) for
 * callers that do not need the reference's synchronous contract.                                                          */
int dc_net_forward_host_async(dc_net* net, const float* input, int n, int h, int w, float* prob, float* loc_pred, float* next_pred);
/* pinned (page-locked) host memory for the entry above; the reference pins its blobs the same way in GPU mode
 * (CaffeMallocHost, include/caffe/syncedmem.hpp:15-44)                                                                 */
int dc_host_alloc(size_t bytes, void** out);
int dc_host_free(void* p);

/* ---- executor streams chosen by measurement -----------------------------------------------------------------------------
 * A HIP process has four hardware queues; a stream is bound to one of them at creation and streams that share a queue run one
 * after the other — with four executors "in flight" the throughput is 380 to 490 images/s depending on which streams they got
 * (profiles/r04_stream_subsets.txt), and the API does not say.  dc_nets_choose_streams times the executors' REAL forwards (each must
 * have run or reserved its shape) on assignments of a process-wide pool of `candidates` (0 = 8) streams, `reps` (0 = 3) forwards
 * per executor and burst, and makes the best assignment the executors' own streams (DC_STREAM_OWN, dc_net_stream).  rate_chosen /
 * rate_first (may be NULL): forwards per second with the chosen streams / with the first n streams of the pool.  No reference
 * counterpart (one legacy stream per thread, src/caffe/common.cpp:99-158).                                                */
int dc_nets_choose_streams(dc_net* const* nets, int n, int candidates, int reps, double* rate_chosen, double* rate_first);
/* the net's own stream (a hipStream_t), created on first use: what DC_STREAM_OWN enqueues on                              */
int dc_net_stream(dc_net* net, void** out);

/* Cross-request batching: `n` independent single-image requests — one DEVICE input pointer ([3,H,W] float32) and one
 * set of DEVICE output pointers per request (the arrays, or single entries, may be NULL) — run as ONE batch-n forward;
 * request i's maps land in its own buffers.  What a server does with concurrent batch-1 requests (the reference forwards
 * one image at a time, conv_layer.cpp:31).  stream as dc_net_forward_batch.                                       */
int dc_net_forward_requests(dc_net* net, int n, const float* const* inputs, int h, int w, float* const* prob,
                            float* const* loc_pred, float* const* next_pred, void* stream);

/* The maps of the LAST forward copied out as NCHW, host or device destination, any pointer NULL to skip: elem 0 =
 * float32; elem 1 = the net's 16-bit element type, offered by fp16 and bf16 nets (DC_OPT_DTYPE 1 / 2) only, refused on a
 * float32 net — float16 or bfloat16 values as they are in HBM, i.e. half the
 * bytes for the gather of the maps to rank 0 (no reference counterpart; Blob::cpu_data of the three outputs).
 * stream as dc_net_forward_batch.                                                                             */
int dc_net_emit_maps(dc_net* net, void* prob, void* loc_pred, void* next_pred, int elem, int is_device, void* stream);

/* ---- pose decoding on the device (python/pose/estimate_pose.py:131-143 `_pose_from_mats`): after a
 * forward, writes pose[n][5][J] doubles (x, y, confidence, and the refinement vector in the reference's
 * (row, column) order, all divided by `scale`) to a host buffer (is_device=0) or a device buffer.
 * A NaN in `prob` is outside the rule: numpy's argmax picks the first NaN, the device skips NaN cells.   */
int dc_net_decode_pose(dc_net* net, double scale, double* pose, int is_device, void* stream);

/* ---- image entry: the demo's pre-processing on the device + forward + optional decode -------------------
 * python/pose/estimate_pose.py:83-128 for `n` same-size images at one scale, without the float canvas ever
 * existing on the host: replicate the last row / column 64 px (:89-95), scipy.misc.imresize(img, scale,
 * 'bilinear') = Pillow's 8-bit two-pass bilinear resample to (int((W+64)*scale), int((H+64)*scale)) (:96;
 * bit-exact: 22-bit fixed-point weights computed as Pillow does; the identity at scale 1), subtract the BGR
 * mean [104,117,123] (:97), paste on a zero canvas of ceil(H*scale/8)*8 x ceil(W*scale/8)*8 (:85-88,
 * :99-103), written straight into the `data` blob's image in HBM; then the forward; then, if `pose` is not
 * NULL, `_pose_from_mats` (:131-143) as dc_net_decode_pose does.
 * images  : n * height * width * 3 bytes, BGR, HWC, packed; host (is_device=0) or device memory.
 * outputs : as dc_net_forward_batch (any may be NULL); pose = n*5*J doubles or NULL, host/device like the rest.
 * stream  : as dc_net_forward_batch.  The net input is reshaped to the canvas size.                       */
int dc_net_forward_images(dc_net* net, const unsigned char* images, int n, int height, int width, double scale,
                          int is_device, float* prob, float* loc_pred, float* next_pred, double* pose, void* stream);
/* the canvas (= network input) height and width dc_net_forward_images uses for an image at `scale` */
int dc_image_canvas_size(int height, int width, double scale, int* canvas_h, int* canvas_w);

/* ---- box entry: top-down poses for the person boxes of ONE image ------------------------------------------------------
 * Box i = boxes[4i..4i+3] = (x0, y0, x1, y1), half-open, inside the height x width image, at scale scales[i], is treated as the
 * image of its own that a caller would cut on the host: crop = image[y0:y1, x0:x1]; its canvas is dc_net_forward_images' pre-
 * processing of that crop at scales[i] (the 64-px replicate padding repeats the CROP's last row / column, not the image's),
 * pasted at the top-left of a zero canvas of canvas_h x canvas_w.  All n canvases are made by ONE launch straight into the `data`
 * blob's image (float32, float16 or bfloat16 nets alike), then ONE batch-n forward.  pose (n*5*J doubles, or NULL) is
 * `_pose_from_mats` of box i's maps restricted to the cells of the crop's own canvas (dc_image_canvas_size(y1-y0, x1-x0,
 * scales[i]) / 8), divided by scales[i], with x and y (rows 0 and 1) shifted by (x0, y0) into image coordinates; the other
 * rows as dc_net_decode_pose.  The result equals dc_net_forward_images on each host-cut crop placed on the common canvas.
 * Finding the boxes (a person detector) and choosing their scales are the caller's.
 * image   : height * width * 3 bytes, BGR, HWC; host (is_device=0) or device memory.  boxes (int32 n x 4) and scales (n doubles)
 *           are host arrays.
 * canvas  : canvas_h and canvas_w multiples of 8, at least every box's own canvas (dc_image_canvas_size of the crop).
 * outputs : as dc_net_forward_images (any may be NULL); maps are n x the whole canvas's map.  stream as dc_net_forward_batch.
 * Errors  : DC_EINVAL naming the box, before any device work, for an empty box, a box outside the image, a non-positive scale,
 *           a canvas that is not a multiple of 8 or smaller than a box's own canvas.  n = 0 does nothing.                      */
int dc_net_forward_boxes(dc_net* net, const unsigned char* image, int height, int width, int is_device, const int* boxes, const double* scales,
                         int n, int canvas_h, int canvas_w, float* prob, float* loc_pred, float* next_pred, double* pose, void* stream);

/* ---- video frames: the image and box entries on NV12 and pitched surfaces ------------------------------------------------
 * NO REFERENCE COUNTERPART: the reference's demo reads packed BGR from cv2.imread.  A dc_frame describes one image where a decoder
 * left it: up to two planes with a row pitch in BYTES each, host (is_device=0) or device memory like the other entries' pixels.
 * Odd widths and heights are allowed; the chroma plane then has the extra half row / column, as the sizes below say.            */
#define DC_PIX_BGR24 0   /* plane[0]: B,G,R bytes, pitch[0] >= 3*width; plane[1] unused                                  */
#define DC_PIX_NV12  1   /* plane[0]: Y, height rows, pitch[0] >= width; plane[1]: Cb,Cr byte pairs,
                            (height+1)/2 rows of (width+1)/2 pairs, pitch[1] >= 2*((width+1)/2)                         */
#define DC_CSC_BT601 0   /* Kr = 0.299,  Kb = 0.114  */
#define DC_CSC_BT709 1   /* Kr = 0.2126, Kb = 0.0722 */
#define DC_RANGE_LIMITED 0   /* Y 16..235, C 16..240 */
#define DC_RANGE_FULL    1
typedef struct dc_frame { const void* plane[2]; int pitch[2]; int format, matrix, range; } dc_frame;
/* THE RULE (this project's statement of the two standards; integer arithmetic, the same on every path).
 * Chroma siting: the pixel at image position (x, y) uses chroma sample (x >> 1, y >> 1); there is no interpolation.  For the box
 *   entries x and y are ABSOLUTE image coordinates (x0 + crop column, y0 + crop row), not crop-relative: a box with an odd origin
 *   pairs chroma differently from a host-cut crop of the planes.
 * Conversion: c = Y - y0, d = Cb - 128, e = Cr - 128.  Limited range: y0 = 16, sy = 255/219, sc = 255/224; full range: y0 = 0,
 *   sy = sc = 1.  Kg = 1 - Kr - Kb.  Five coefficients, computed on the host in double and rounded to nearest:
 *     ky = rint(65536 sy)                     rv = rint(65536 * 2(1-Kr) sc)          bu = rint(65536 * 2(1-Kb) sc)
 *     gu = rint(65536 * (-2 Kb (1-Kb) / Kg) sc)                 gv = rint(65536 * (-2 Kr (1-Kr) / Kg) sc)
 *   then on int32 with an arithmetic shift (the magnitude stays below 2^26), clip8 = clamp to 0..255:
 *     R = clip8((ky c + rv e + 32768) >> 16)    G = clip8((ky c + gu d + gv e + 32768) >> 16)    B = clip8((ky c + bu d + 32768) >> 16)
 *   (ky, rv, bu, gu, gv): BT.601 limited (76309, 104597, 132201, -25675, -53279), BT.709 limited (76309, 117489, 138438, -13975,
 *   -34925), BT.601 full (65536, 91881, 116130, -22553, -46802).  Each coefficient is within 2^-17 of the real one and multiplies a
 *   value of at most 255, so the result is within one level of the real-valued matrix rounded to nearest (tests/test_nv12_rule.py:
 *   all 2^24 triples, every matrix and range; full-range BT.601 is also within one level of Pillow's YCbCr -> RGB, whose tables
 *   are no closed form, so equality with Pillow is not claimed).
 * Where it runs: where a source pixel is fetched by the pre-processing kernels, after the replicate clamp and the mirror
 *   reflection.  Pillow's resample works on 8-bit channels, so every frame entry gives BIT FOR BIT what the entry it is named after
 *   gives on the image converted by the rule on the host.  DC_PIX_BGR24 applies no conversion: it only adds the pitch.
 * The entries: each is the entry it is named after with a dc_frame where that one takes a pixel pointer, and behaves like it in
 *   every other respect (outputs, pose, stream, is_device, errors, n = 0).  dc_net_forward_frames takes n frames (n separate
 *   surfaces of one height x width, format, matrix and range); the box entries one.  dc_group_forward_frames takes one array of
 *   n[c] frames per member (the usual case: the same array for every member); the two group entries take `mirror` ([members] 0/1,
 *   NULL = none) as the _mirrored entries do, and a mirrored member records that its last batch was mirrored exactly as they do, so
 *   dc_group_fuse_maps_mirrored, dc_group_decode_pose, dc_group_decode_boxes and dc_group_assemble_people_mirrored work unchanged.
 * Host frames (is_device = 0) are NOT converted on the host: their planes are staged into the net's image buffer, one 2-D copy per
 *   plane on the call's stream, without the pitch padding — 1.5 bytes per pixel travel for NV12 —, and a frame that several
 *   members of a group share travels once.
 * Errors: DC_EINVAL naming the field and the frame index, before any device work, for a NULL plane the format needs, a pitch below
 *   the minimum, an unknown format / matrix / range, and frames of one call that differ in format, matrix or range.             */
int dc_net_forward_frames(dc_net* net, const dc_frame* frames, int n, int height, int width, double scale, int is_device, float* prob,
                          float* loc_pred, float* next_pred, double* pose, void* stream);
int dc_net_forward_boxes_frame(dc_net* net, const dc_frame* frame, int height, int width, int is_device, const int* boxes,
                               const double* scales, int n, int canvas_h, int canvas_w, float* prob, float* loc_pred, float* next_pred,
                               double* pose, void* stream);

/* ---- multi-person consumers of the maps (no reference code: the reference repository stops at the maps) --------
 * What they invert is the label encoding of the reference's training layer (src/caffe/layers/pose_data_layer.cpp:
 * 686-802): a map cell (row, col) stands for the image point pt = (col*8+4, row*8+4)/scale; loc_pred holds
 * (joint - pt)*scale/sqrt(53); next_pred channel pair l holds ((next joint - pt)*scale - mean[l]) / std[l] for
 * regression edge l (edges, means and stds come from the model's `joint_pairs_stats` file, caffe.proto:1184).
 *
 * dc_net_detect_parts: non-maximum suppression of every score map of the last forward, on the device: a cell is a
 * candidate if prob >= threshold and it is the maximum of its (2*radius+1)^2 window (ties: the lower row-major cell
 * index).  Per image and joint the candidates are ordered by (score descending, cell ascending) and the first
 * max_det are returned: counts[n*J + j] and dets[((n*J + j)*max_det + k)*5 + {0..4}] = x, y (refined with loc_pred,
 * divided by scale), score, cell row, cell column.  Host buffers; synchronous.
 * dc_net_decode_pairwise: for ndet detections given as (image, cell row, cell column) triples and every edge l,
 * out[(d*E + l)*2 + {0,1}] = pt + (next_pred[2l + k] at the cell * std[l][k] + mean[l][k]) / scale, E = channels/2;
 * mean / std may be NULL (0 / 1).  Host buffers; synchronous.                                               */
int dc_net_detect_parts(dc_net* net, double scale, float threshold, int radius, int max_det, int* counts, double* dets);
int dc_net_decode_pairwise(dc_net* net, double scale, int ndet, const int* detections, const double* mean,
                           const double* stdev, double* out);

/* ---- people: bottom-up assembly from the part candidates and the pairwise maps, on the device ------------------------
 * NO REFERENCE COUNTERPART: the reference repository stops at the maps and has no consumer of `next_pred`.  Only the label encoding of
 * its training layer (src/caffe/layers/pose_data_layer.cpp:686-802) is restated, as above; the grouping rule below is this project's
 * own and its parity is unpinned by the reference.
 *
 * dc_pair_stats_read: the `joint_pairs_stats` file of a model (caffe.proto:1184; the reference reads it with readMatricesFromFile,
 * src/caffe/util/SimpleMatrix.cpp:9-37).  Text, everything whitespace-separated: repeated blocks of `# <name>`, `<rows> <cols>`, rows x
 * cols numbers.  The first three matrices are used (pose_data_layer.cpp:453-455): edges [E][2] of 1-based class ids (cls, next_cls),
 * returned as 0-based joints = class - 1 (:85-88), means [E][2], standard deviations [E][2].  Host only, no GPU.  *n_edges = E.
 * Errors: DC_EIO for an unreadable file; DC_EINVAL naming what is wrong for fewer than three matrices, a matrix that is not E x 2,
 *         differing row counts, a truncated block, a class id < 1, a non-positive or non-finite standard deviation, E > max_edges
 *         (*n_edges then says how many the file holds).
 *
 * dc_net_assemble_people: the people of every image of the last forward, in three stages on the device with no host round trip
 * in between; host output buffers, synchronous on the net's stream like dc_net_detect_parts; float32, float16 and bfloat16 nets alike.
 *  A. candidates: dc_net_detect_parts(scale, threshold, radius, max_det); candidate (j, i) is entry i of joint j's list.
 *  B. pair costs: for joints a != c, candidate i of a and k of c, with F = the lowest-index edge l with edges[l] == (a, c) and R = the
 *     lowest-index edge with edges[l] == (c, a) (edges: n_edges x 2 0-based joints; n_edges = next_pred channels / 2, else DC_ESHAPE):
 *       pred(cell, l) = pt(cell) + (next_pred[2l..2l+1] at cell * std[l] + mean[l]) / scale        (as dc_net_decode_pairwise)
 *       d_f = |pred(cell of (a,i), F) - position of (c,k)|,  d_r = |pred(cell of (c,k), R) - position of (a,i)|   (image pixels)
 *       cost[b][a][c][i][k] = scale * mean of those of d_f, d_r whose edge exists (network pixels); +infinity when neither exists, for
 *       a == c and for slots beyond a list's count.  cost[b][c][a][k][i] is the same number.  All arithmetic in double.
 *  C. greedy assembly, deterministic (same inputs, same people): the joints are processed in joint_order ([J], a permutation; NULL =
 *     0..J-1).  For joint j: (1) for every person p (creation order) and free candidate i of j, the link cost L(p, i) = the arithmetic
 *     mean of cost[b][a][j][candidate p holds of a][i] over the joints a (ascending) that p holds and whose cost is finite; infinite if
 *     there is none.  (2) Until no link with L <= max_cost remains: among the links of people without joint j and free candidates
 *     take the smallest L (ties: the lower p, then the lower i), assign it.  (3) Every candidate of j still free, in list order, with
 *     score >= seed_threshold starts a new person holding only this joint, until max_people exist.  After the last joint people
 *     with fewer than min_joints joints are dropped, the others keep their order.
 *  D. (only with dc_net_set_completion enabled; off by default) completion: joints a person lacks are looked for in the score map
 *     around the position its held joints predict; a joint filled so has cand = -2.  The rule is stated at dc_complete_params below.
 *  E. (only with dc_net_set_dedupe enabled; off by default) dedupe: a person that a better-scored kept person is "the same" as, by the
 *     tracker's distance, is suppressed, and n_people shrinks.  The rule is stated at dc_dedupe_params below.
 * Outputs: n_people[b]; people[((b*P + q)*J + j)*3 + {0,1,2}] = x, y, score of person q's candidate of joint j, (0, 0, 0) where it has
 *          none and for q >= n_people[b]; cand[(b*P + q)*J + j] = that candidate's index in joint j's list or -1 (may be NULL); cost (may
 *          be NULL: diagnostics and tests) = the whole tensor [n][J][J][max_det][max_det].  P = max_people.
 * Errors : DC_EINVAL naming the parameter for scale <= 0, threshold < 0, radius outside [0, 64], max_det outside [1, 64], max_cost
 *          negative or not finite, max_people outside [1, 256], min_joints outside [1, J]; DC_EINVAL before any device work for a joint
 *          index outside [0, J), an edge with a == b, a joint_order that is not a permutation; DC_EUNSUP when `next_pred` is left out by
 *          DC_OPT_OUTPUTS (unless DC_OPT_SPARSE_PAIRWISE is 1: stage B then reads the head evaluated at stage A's cells, see
 *          dc_net_pairwise_at); DC_ESHAPE for a wrong n_edges or more than 32 joints.                                                 */
typedef struct dc_assemble_params {
  double scale;          /* as dc_net_detect_parts */
  float  threshold;      /* candidate score threshold */
  int    radius, max_det;/* NMS window, candidates kept per joint: 1 <= max_det <= 64 here */
  double max_cost;       /* a link is allowed when its cost (network pixels) <= max_cost */
  float  seed_threshold; /* a candidate that joins nobody starts a person when its score >= this */
  int    max_people;     /* P, 1..256 */
  int    min_joints;     /* people with fewer assigned joints are dropped from the result */
} dc_assemble_params;
int dc_pair_stats_read(const char* path, int max_edges, int* n_edges, int* edges, double* mean, double* stdev);
int dc_net_assemble_people(dc_net* net, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean, const double* stdev,
                           const int* joint_order, int* n_people, double* people, int* cand, double* cost);

/* ---- the pairwise head at candidate cells only (DC_OPT_SPARSE_PAIRWISE) -------------------------------------------------------
 * Bottom-up people is the only consumer of `next_pred` and reads it at the part candidates' cells only: at most J x max_det cells
 * per image of the 68 x 92 of a 544x736 forward, while the dense 364-channel head is 23.3 of that forward's 241 GFLOP.  With
 * DC_OPT_SPARSE_PAIRWISE 1 a net whose output selection leaves `next_pred` out (DC_OPT_OUTPUTS) evaluates the head at those cells:
 * dc_net_assemble_people between its stages A and B (no host round trip: the candidates stay on the device), dc_net_decode_pairwise
 * and dc_net_pairwise_at at the cells they are given.  Everything downstream runs unchanged on a float32 scratch map.
 *
 * The pairwise head is recognised from the layer list (it does not depend on the lowering): `next_pred` must be the top of an Eltwise
 * SUM whose bottoms are
 *   - a Convolution 1x1, stride 1, pad 0, group 1 (filters Ws[n][k], input X3), and
 *   - the fork's Crop (offsets oh, ow) of a Deconvolution with kernel 3, stride 2, pad 0, dilation 1, group 1 (filters
 *     Wd[k][n][ky][kx], input X5 of h5 x w5 cells),
 * each with or without a bias.  Anything else is DC_EUNSUP naming the layer.  For image b, channel n and cell (r, c):
 *
 *   next[b,n,r,c] = bias_s[n] + bias_d[n]
 *                 + sum_k Ws[n,k] * X3[b,k,r,c]
 *                 + sum over ky, kx in {0,1,2} with (r+oh-ky) even, (c+ow-kx) even, 0 <= (r+oh-ky)/2 < h5, 0 <= (c+ow-kx)/2 < w5 of
 *                       sum_k Wd[k,n,ky,kx] * X5[b,k,(r+oh-ky)/2,(c+ow-kx)/2]
 *
 * A cell uses 1, 2, 2 or 4 of the nine taps, by the parity of (r+oh, c+ow); row 0 and column 0 lose the ky = 2 / kx = 2 taps.
 * Operands are what the dense head sees: activations in the net's element type, filters rounded to it on float16 / bfloat16 nets, the
 * bias in float32.  Products are accumulated in float32 on v_mfma_f32_32x32x2_f32 and the result is float32 for every net type: it is
 * NOT rounded to 16 bits as the dense map of a 16-bit net is.  Deterministic, no float atomics: the value at a cell depends on that cell
 * only — not on its place in the list, the other cells, or which entry asked; a cell listed twice is computed twice.
 * X3 and X5 must be materialised in the current plan (they are in every plan that computes `loc_pred`), else DC_EUNSUP; a host-
 * authoritative one is uploaded first, as an output map is.  The filters are packed once per model and element type, shared with
 * clones and dropped when the parameters change, like every other filter image (DC_STAT_SPARSE_PACKS counts the packs a net made).
 * OUT OF SCOPE: dc_group_* (pyramids, mirrored members).  The fused bottom-up path needs every member's head at the four neighbours of
 * each base cell; dc_group_assemble_people on members without `next_pred` keeps answering DC_EUNSUP whatever this option says.
 *
 * dc_net_pairwise_at: the raw `next_pred` values of the last forward at ndet cells, detections = (image, cell row, cell column)
 * triples, out[d*C + n] float32: read from the dense map when the plan has it (widened from a 16-bit net's map), by the rule above
 * otherwise.  Host buffers; synchronous.  DC_EINVAL before any device work for a cell outside the map; DC_EUNSUP for a net whose plan
 * has no `next_pred` while the option is 0.
 * dc_sparse_head_pack (tests / diagnostics; host only): the head's filter image as the library packs it for float32 nets, from
 * ws [cout][k3] and wd [k5][cout][3][3]: float32 [segment 0..9][ceil(cout/32)][K block of 8][64 lanes][4], segment t < 9 the tap
 * ky*3 + kx = t over k5 channels, segment 9 the skip over k3; lane l of K block j of chunk q holds W[k = 8j + 4(l/32) + m][n = 32q + l%32],
 * m = 0..3, zeros beyond k and cout.  Segments 0..8 take ceil(cout/32) * ceil(k5/8) * 256 floats each, segment 9
 * ceil(cout/32) * ceil(k3/8) * 256; dc_sparse_head_pack_size is their sum (-1 on bad arguments).                                   */
int dc_net_pairwise_at(dc_net* net, int ndet, const int* detections /* image,row,col */, float* out /* [ndet][C] */);
int dc_sparse_head_pack_size(int cout, int k3, int k5);
int dc_sparse_head_pack(const float* ws, const float* wd, int cout, int k3, int k5, float* out);


/* ---- introspection used by bench.py / DESIGN.md ----------------------------------------- */
/* algorithmic FLOPs (2*MAC of conv+deconv) of the current shape               */
int dc_net_flops(dc_net* net, double* flops);
/* number of kernel launches in the current plan                                           */
int dc_net_num_launches(dc_net* net);
/* counters of the per-shape plan cache: Layer::Forward re-derives every shape on every call (layer.hpp:451-456) and the
 * demo changes the input shape once per scale (estimate_pose.py:81-128); a shape met before must cost neither a
 * re-lowering nor a graph instantiation.  out[i] for i < n:                                                     */
#define DC_STAT_LOWERINGS 0        /* times the layer graph was lowered to a launch plan                  */
#define DC_STAT_GRAPH_INSTANTIATIONS 1 /* hipGraph captures + instantiations                              */
#define DC_STAT_PLAN_HITS 2        /* shape changes served from the cache                                 */
#define DC_STAT_AUTOTUNE_RUNS 3    /* plans for which at least one GEMM signature had to be timed         */
#define DC_STAT_BUFFER_GROWTHS 4   /* device buffers (re)allocated                                        */
#define DC_STAT_REPACKS 5          /* times the filter images were re-packed from the parameter blobs     */
#define DC_STAT_CACHED_PLANS 6     /* shapes currently cached (LRU of DC_PLAN_CACHE, default 16)          */
#define DC_STAT_SPARSE_PACKS 7     /* times this net packed the pairwise head's filter image (DC_OPT_SPARSE_PAIRWISE) */
#define DC_NUM_STATS 8
int dc_net_stats(dc_net* net, long long* out, int n);
/* lower, allocate and tune the plan of an [n,3,h,w] input without running it: reserving the LARGEST shape of a
 * pyramid first means no buffer grows (and no captured graph goes stale) while the smaller ones are met        */
int dc_net_reserve(dc_net* net, int n, int h, int w);
/* the HIP device this net executes on (-1 until its first device use: then Caffe::SetDevice's value, common.cpp:140) */
int dc_net_device(dc_net* net);
/* human-readable launch plan of the current shape (kernel variant, tile, grid per op);
 * pointer valid until the next call on this net                                           */
const char* dc_net_plan_text(dc_net* net);
/* time each op of the current plan with hipEvents on the net's stream (iters runs each);
 * returns a text table (op, kernel, us, GFLOP, TFLOP/s); pointer valid until next call    */
const char* dc_net_profile_text(dc_net* net, int iters);
/* Net::ForwardDebugInfo / InputDebugInfo (src/caffe/net.cpp:648-681, `debug_info: true` in the NetParameter,
 * caffe.proto:88): one line per input, top blob and parameter blob with its mean absolute value after the LAST
 * forward, in the reference's log format ("    [Forward] Layer conv1, top blob conv1 data: 0.0645").  In-place chains
 * run as one kernel here: the value is reported at the chain's last layer; with DC_OPT_FUSE 0 every Caffe-visible
 * blob is materialised (fused blobs are reported as elided otherwise).  NULL + dc_last_error() on failure;
 * pointer valid until the next call on this net.                                                                   */
const char* dc_net_debug_info(dc_net* net);
/* Tile choices of the current shape, for a tuner that works under the caller's own load (deepcut_tools.tune_in_flight): one line
 * per GEMM signature of the plan, "<signature>\t<tile in use>\t<launches>\t<tile>:<us timed alone> ..." (fastest first; the
 * signature is the key DC_TUNE_CACHE files use).  dc_net_set_tile overrides the tile of one signature in this executor's
 * current plan and in the choice table it shares with its clones; the captured graph is dropped (re-captured by the next
 * forward): call it while the executor is idle (nothing of it in flight on any stream).  DC_EUNSUP if the tile cannot take a
 * launch of the signature.  No reference counterpart: the reference has one
 * SGEMM per layer (math_functions.cu:13-27).                                                                            */
const char* dc_net_tune_report(dc_net* net);
int dc_net_set_tile(dc_net* net, const char* signature, const char* tile);
/* the gather-GEMM's tile-variant table (csrc/conv_gemm.cpp): number of entries, name and element size (4 float / 2 half) of
 * entry i — what the environment switch DC_CONV_VARIANT=<i> forces and the names dc_net_plan_text / DC_TUNE_CACHE use.
 * No reference counterpart: the reference has one SGEMM (math_functions.cu:13-27); diagnostics only.                  */
int dc_conv_variant_count(void);
const char* dc_conv_variant_name(int i);
int dc_conv_variant_esize(int i);
/* the bfloat16 tiles (DC_OPT_DTYPE 2), a table of their own: names for dc_net_set_tile / tune caches, index i = what
 * DC_CONV_VARIANT_BF16=i forces on bf16 nets                                                                            */
int dc_conv_bf16_variant_count(void);
const char* dc_conv_bf16_variant_name(int i);
/* the float16 Winograd form's filter image (csrc/wino_f16.hip, tile `wino_h23`), made on the host exactly as the lowering makes it:
 * g = [cout][cin][3][3] (Caffe order, convolution_param of a stride-1 3x3 layer; cin % 16 == 0, cout % 32 == 0) -> out[16 * cout * cin]
 * = U = G g G^T per (co, ci) in double, channel co multiplied by row_scale[co]^-1 — an exact power of two bringing its largest |U|
 * into [2^13, 2^14) when `rowscale` is non-zero, else 1 —, in MFMA fragment order [cout/32][4 i][cin/16][4 j][64 lanes][8]:
 * lane = 32 * ((ci % 16) / 8) + co % 32, element = ci % 8.  Diagnostics / tests (the host half of the kernel's parity:
 * tests/test_wino_half_pack.py); the reference has no counterpart (its 3x3 layers are im2col + SGEMM, base_conv_layer.cpp:257-280). */
int dc_wino_half_pack(const float* g, int cout, int cin, int rowscale, float* out, float* row_scale);
/* the tile blocks (= workgroups per image phase and 16 output channels) that the float32 Winograd form `tile` (`wino_f23`, `wino_f23_w16`:
 * 4 x 8 tiles; `wino_f23_5x6`, `wino_f23_5x6_w16`: 5 x 6) needs for a grid of tiles_y x tiles_x 2x2-output tiles; -1 for any other name.
 * The 5 x 6 forms are candidates of the per-shape timing where they need strictly fewer blocks.  Diagnostics / tests.               */
int dc_wino_blocks(const char* tile, int tiles_y, int tiles_x);
/* the cover of a tiles_y x tiles_x tile grid that `wino_f23_mix` / `wino_f23_mix_w16` run (`dc_wino_blocks` answers for these names too): one
 * straight cut, region A in front of it on 4 x 8-tile blocks from the grid's origin, region B behind it on 5 x 6-tile blocks; fewest blocks,
 * on a tie a pure cover before a cut one, then fewest 5 x 6 blocks; either region may be empty.  out[12] = {vertical cut (else horizontal), cut (tile row / column), blocks,
 * blocks of A, of B, A's block rows, block columns, B's block rows, block columns, B's first tile row, first tile column, offered};
 * offered: the cover needs strictly fewer blocks than both pure ones — one of the two conditions under which the per-shape timing tries the mixed
 * forms; the other is the size of the launch (`dc_wino_mix_offered`).
 * Returns the block count, -1 on bad arguments.  A pure function: no device.  Diagnostics / tests.                                   */
int dc_wino_cover(int tiles_y, int tiles_x, int* out);
/* 1 where the per-shape timing tries the mixed forms for a 3x3 layer of `images` images (batch x dilation^2 phase images) of tiles_y x tiles_x
 * tiles and cout output channels: the cover is `offered` (above) and the launch on 4 x 8 blocks has at least 128 workgroups, half the CUs — a
 * smaller launch leaves most workgroup slots of the chip free with either cover (a bound from that argument, not from a measurement).  0 elsewhere (`set_tile` and tune caches still take the forms
 * wherever the kernel is eligible), -1 on bad arguments.                                                                              */
int dc_wino_mix_offered(int tiles_y, int tiles_x, int images, int cout);

/* the filter images of the two float16 kernels added in round 6, made on the host exactly as the lowering makes them (diagnostics / tests:
 * tests/test_stream_pack.py emulates the matrix instruction's operand layout on them; the reference has no counterpart — its 1x1 layers
 * are one SGEMM per image, base_conv_layer.cpp:326-341, its stem im2col + SGEMM, base_conv_layer.cpp:257-280):
 *  dc_stream1x1_pack: g = [cout][k] (a 1x1 filter bank; cout % 32 == 0, k % 16 == 0) -> out[cout * k] in the ROW-operand order of
 *    v_mfma_f32_32x32x16_f16, [cout/32][k/16][64 lanes][8]: lane = 32 * ((kk % 16) / 8) + co % 32, element = kk % 8 (csrc/stream1x1.hip);
 *  dc_stem7x7_pack:   g = [64][c][7][7] (c <= 4) -> out[14336] = [fragment 2][kernel row 7][K step 2][64 lanes][8], element e = kx * 4 + ci
 *    of a kernel row at lane 32 * ((e % 16) / 8) + co % 32, position e % 8 of K step e / 16, zeros elsewhere (csrc/stem_f16.hip).        */
int dc_stream1x1_pack(const float* g, int cout, int k, float* out);
int dc_stem7x7_pack(const float* g, int c, float* out);
/*  dc_stream1x1f_pack: the float32 form of the streaming 1x1 kernel (csrc/stream1x1_f32.hip, tile `ws1x1f`): g = [cout][k] (cout % 16 == 0,
 *    k % 16 == 0) -> out[cout * k] in the ROW-operand order of v_mfma_f32_16x16x4_f32 with the K range cut into four runs,
 *    [cout/16][k/16 vectors][64 lanes][4]: lane = 16 q + co % 16 holds run q, element e of vector j = g[co][q k/4 + 4 j + e] — matrix step
 *    4 j + e of a 16-pixel step multiplies column (q k/4 + 4 j + e) of the filters with the same element of the pixel rows (one 16-byte LDS
 *    read of a pixel's row feeds four matrix steps).  tests/test_stream_pack.py.                                                        */
int dc_stream1x1f_pack(const float* g, int cout, int k, float* out);
/*  dc_stream1x1f_rows: ONE launch of that kernel on host arrays, with the strides a lowered net does not produce (tests / diagnostics):
 *    x = [m][x_stride], the first k floats of a row are the pixel's channels; g = [cout][k] (packed here); scale / shift = [cout] or NULL;
 *    y = [y_rows][y_stride], in and out: the launch writes channels [y_c0, y_c0 + cout) of rows [0, m) — a channel view of a wider tensor —
 *    and every other element comes back as it went in; resid = NULL or the shortcut in y's layout, read at the same channels; relu != 0
 *    applies the ReLU.  m <= y_rows, k in 64 / 128 / 256 / 512, cout % 64 == 0, strides and y_c0 multiples of 4.  Copies to the calling
 *    thread's device, launches on its default stream, waits, copies y back.  tests/test_gpu_ws1x1f_addressing.py.                       */
int dc_stream1x1f_rows(const float* x, int m, int k, int x_stride, const float* g, int cout, const float* scale, const float* shift, float* y,
                       int y_rows, int y_stride, int y_c0, const float* resid, int relu);
/*  dc_wino43_pack: the filter image of the unfused Winograd F(4x4,3x3) form (csrc/wino43_f32.hip, tile `wino_f43`): g = [cout][cin][3][3]
 *    (cout % 16 == 0, cin % 16 == 0) -> out[36 * cout * cin]: U = G g G^T per (co, ci) in double, rounded once to float; point p = 6 i + j
 *    (U[i][j]) is the [cout][cin] matrix at out + p * cout * cin, each in dc_stream1x1f_pack's order.  tests/test_wino43_host.py.          */
int dc_wino43_pack(const float* g, int cout, int cin, float* out);

/* ---- pyramid-grouped execution: several executors of ONE model, each at its own input shape, as ONE launch sequence ----
 * Replaces the scale loop of the demo (python/pose/estimate_pose.py:81-128: one net.forward() per scale, every shape change a
 * full Reshape) and, per layer, the reference's one-SGEMM-per-image loop (src/caffe/layers/base_conv_layer.cpp:326-341,
 * conv_layer.cpp:31): launch i of the group is launch i of EVERY member merged into one multi-problem gather-GEMM, so a layer's
 * filters are pulled through the L2s once for all scales and the chip sees one dispatch ramp and one tail per layer
 * (a 4-scale pyramid: 161 launches as one lane, 318 as the default two concurrent lanes, instead of 632).  Members are a net and its clones (dc_net_clone: shared parameters, own
 * activations); they stay usable on their own, and their blobs hold the results of a grouped forward exactly as after their own
 * (dc_net_blob / dc_net_decode_pose / dc_net_emit_maps / dc_net_detect_parts on a member see them).  Results equal the members'
 * own forwards up to the fp32 summation order of the tile chosen (bit-identical for the same tile).  The group borrows the nets: it
 * must not RUN after one of them is gone (destroying it afterwards is harmless).  Arrays below have one entry per member, in the order given at creation.                          */
typedef struct dc_group dc_group;
int dc_group_create(dc_net* const* nets, int n, dc_group** out);
int dc_group_destroy(dc_group* group);
int dc_group_size(dc_group* group);
/* LANES: the members are dealt to `lanes` lanes (largest with smallest), every lane is merged on its own and runs on a stream of
 * its own, concurrently with the others — the launches of one lane fill the dispatch ramps and tails of the other's (one grouped
 * 4-scale float16 pyramid batch: 12.1 ms as one lane, 10.6 ms as two), at the price of one filter fetch per lane and layer.
 * 0 (default) = automatic: two members run as two lanes (plain concurrency: faster than merging two tensors), three as one lane,
 * four or more as two lanes of merged members.  Drops the merged plans.                                                      */
int dc_group_set_lanes(dc_group* group, int lanes);
/* dc_net_forward_batch for every member at once: member c forwards inputs[c] = n[c] x 3 x h[c] x w[c]; output pointer arrays
 * (or single entries) may be NULL.  stream as dc_net_forward_batch (NULL = the first member's own stream, synchronous).      */
int dc_group_forward_batch(dc_group* group, const float* const* inputs, const int* n, const int* h, const int* w, int is_device,
                           float* const* prob, float* const* loc_pred, float* const* next_pred, void* stream);
/* dc_net_forward_images for every member at once (member c: n[c] images of height[c] x width[c] at scale[c]; the usual case is
 * the SAME images at the scales of a pyramid): pre-processing per member, ONE grouped forward, then per member the maps and —
 * pose[c] not NULL — the decoded pose.                                                                                       */
int dc_group_forward_images(dc_group* group, const unsigned char* const* images, const int* n, const int* height, const int* width,
                            const double* scale, int is_device, float* const* prob, float* const* loc_pred, float* const* next_pred,
                            double* const* pose, void* stream);
/* dc_net_forward_boxes over an image pyramid: member c takes every box i at scales[i] * pyramid_scales[c] on a canvas of
 * ceil(canvas_h * pyramid_scales[c] / 8) * 8 x ceil(canvas_w * pyramid_scales[c] / 8) * 8; the image is uploaded once, each member
 * pre-processes all its boxes in one launch, then ONE grouped forward; per member c the maps (n x its canvas's map) and pose[c]
 * (n*5*J doubles, image coordinates).  Arrays of outputs have one entry per member, as dc_group_forward_images.  The same errors
 * as dc_net_forward_boxes, checked for every member before any device work; n = 0 does nothing.                             */
int dc_group_forward_boxes(dc_group* group, const unsigned char* image, int height, int width, int is_device, const int* boxes,
                           const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w, float* const* prob,
                           float* const* loc_pred, float* const* next_pred, double* const* pose, void* stream);
/* ---- multi-scale bottom-up people: the maps of a pyramid fused on the device ------------------------------------------------------
 * NO REFERENCE COUNTERPART, as for dc_net_assemble_people: the reference repository stops at the maps.  The fusion rule below is this
 * project's own and its parity is unpinned by the reference; only the label encoding (pose_data_layer.cpp:686-802) is restated.
 *
 * The group has M members; member m holds, from its LAST forward, the maps of the same NB images at scale scales[m] (the usual case: one
 * dc_group_forward_images over a pyramid).  s_b = scales[base].  The fused maps live on the base member's grid H_b x W_b and are
 * float32 whatever the members' element type.  For member m: q = scales[m] / s_b and rho = s_b / scales[m], one division each in
 * double (both exactly 1 for the base member).
 *  Sample position of base cell (r, c) in member m: u = ((8c + 4) q - 4) / 8, v = ((8r + 4) q - 4) / 8 in double (the cell's image
 *     point, in member m's cells); u clamped to [0, W_m - 1], v to [0, H_m - 1]; x0 = floor(u), x1 = min(x0 + 1, W_m - 1), fx = u - x0,
 *     the same for y; fx, fy converted to float.
 *  Sample, in float32, the four corners read in the member's element type and widened to float:
 *     val = (1 - fy) ((1 - fx) a00 + fx a01) + fy ((1 - fx) a10 + fx a11)
 *  Conversion into the base member's units: out_m = val * gain + bias, with (gain, bias) = (1, 0) for prob; (rho, 0) for loc_pred, which
 *     holds (joint - pt) s / sqrt(53); (rho, (rho - 1) mean[l][k] / std[l][k]) for next_pred channel 2l + k, which turns ((next - pt) s_m -
 *     mean) / std into ((next - pt) s_b - mean) / std.  The table [M][channels] is computed on the host in double and uploaded as float;
 *     mean / stdev NULL = 0 / 1.
 *  Fusion: fused = (sum over m ascending of out_m) * (1 / M), in float32.
 * A group of one member fuses to that member's maps widened to float32; the base member always contributes its own cells unchanged; a
 * field that is linear in the cell position is interpolated without error wherever nothing is clamped.  Nothing is atomic or
 * order-dependent: same inputs, same bits.  One launch fuses every map, member and image.
 *
 * Everything runs on the group's stream (the first member's own; dc_group_fuse_maps: or `stream`), so a grouped forward issued there
 * before is complete when the fusion reads its maps.  A caller who forwarded the members individually (dc_net_forward_* with streams
 * of their own) synchronises them first.  The fused buffer is the group's only one: each of the three calls makes its stream wait
 * (an event, no host wait) for what the previous of them left running, so they may follow an asynchronous dc_group_fuse_maps on another
 * stream; the caller's own device destinations of that call are the caller's to wait for.  Calls on one group come from one thread at a time.
 *
 * dc_group_fuse_maps: the fused maps as NCHW float32 [NB][C][H_b][W_b], any of prob / loc_pred / next_pred NULL to leave that map out
 *     (n_edges, mean and stdev are read only when next_pred is asked for).  Host or device destinations and `stream` as in
 *     dc_group_forward_images.
 * dc_group_detect_parts: dc_net_detect_parts on the fused prob and loc_pred (only these two are fused) at scale s_b.
 * dc_group_assemble_people: fuses all three maps, then stages A, B and C of dc_net_assemble_people on the fused maps at scale s_b with no
 *     host round trip in between; p->scale is not read, everything else is as there (outputs, limits, errors).
 * Errors, raised before any device work and naming what is wrong: DC_EINVAL for null scales, a scale that is not positive and finite,
 *     base outside [0, M), a non-finite mean, a std that is not positive and finite; DC_ESHAPE for members whose maps differ in batch size
 *     or channel counts, and for n_edges different from next_pred channels / 2 when next_pred takes part.  Then DC_ENOCPU in CPU mode.
 *     DC_EUNSUP when next_pred is asked for or needed but left out by DC_OPT_OUTPUTS on a member.                                      */
int dc_group_fuse_maps(dc_group* group, const double* scales, int base, int n_edges, const double* mean, const double* stdev, float* prob,
                       float* loc_pred, float* next_pred, int is_device, void* stream);
int dc_group_detect_parts(dc_group* group, const double* scales, int base, float threshold, int radius, int max_det, int* counts,
                          double* dets);
int dc_group_assemble_people(dc_group* group, const double* scales, int base, const dc_assemble_params* p, int n_edges, const int* edges,
                             const double* mean, const double* stdev, const int* joint_order, int* n_people, double* people, int* cand,
                             double* cost);
/* ---- mirror test-time augmentation for the bottom-up entry: mirrored members fused on the device --------------------------------------
 * NO REFERENCE COUNTERPART: the reference stops at the maps and mirrors nothing on the pose path.  The rule below extends the
 * fusion rule above, is this project's own, and its parity is unpinned by the reference.
 *
 * dc_group_forward_images_mirrored: dc_group_forward_images with mirror[c] != 0 marking the members that see their images flipped left
 *     to right.  Such a member's pre-processing reads source column w - 1 - x wherever it would read column x of the unpadded image (the
 *     replicate padding therefore repeats the flipped image's last column, which is original column 0); the resample, the mean and the
 *     canvas are unchanged, so its network input is, bit for bit, what dc_group_forward_images makes of the host-flipped image, for
 *     float32, float16 and bfloat16 nets, with and without a horizontal resample pass.  The maps returned for a mirrored member are that
 *     member's RAW maps, in the flipped image's frame: columns run right to left, left and right joints are swapped and the x components
 *     of loc_pred and next_pred have the other sign — dc_group_fuse_maps_mirrored undoes all of it.  There is no `pose` argument: a
 *     mirrored member's own decoded pose would be in flipped coordinates.  mirror NULL or all zeros enqueues exactly what
 *     dc_group_forward_images enqueues.
 *
 * dc_fuse_mirror: mirror[m] != 0 marks the members that saw the image flipped; image_width = w, the pixels of the unscaled image every
 *     member saw; joint_mirror = pi, the joint that joint j becomes in the mirror (an involution: pi[pi[j]] == j; the table is the
 *     model's: the caller supplies it); edges [n_edges][2] = the 0-based (joint, next joint) of every regression edge, as
 *     dc_net_assemble_people, needed whenever next_pred takes part and a member is mirrored.
 * For a member with mirror[m] == 0 everything is as in dc_group_fuse_maps.  The base member must be unmirrored.  For a mirrored member
 * m, with q = scales[m] / s_b and rho = s_b / scales[m] as there:
 *  Sample position of base cell (r, c): v as there; u = (((w - 1) scales[m] - (8c + 4) q) - 4) / 8 in double, in this order (a cell
 *     stands for image point (8c + 4) / s, and image column x of the flipped image is column w - 1 - x of the original).  Clamp, floor,
 *     corners and the float weights as there.
 *  Source channel and conversion, out_m = val(source channel) * gain + bias:
 *     prob j          reads channel pi[j],         gain 1
 *     loc_pred 2j     reads channel 2 pi[j],       gain -rho
 *     loc_pred 2j + 1 reads channel 2 pi[j] + 1,   gain rho
 *     next_pred of edge l = (a, c) reads edge l', the lowest-index edge equal to (pi[a], pi[c]):
 *       channel 2l     reads 2l',     gain -rho std[l'][0] / std[l][0], bias -(rho mean[l'][0] + mean[l][0]) / std[l][0]
 *       channel 2l + 1 reads 2l' + 1, gain  rho std[l'][1] / std[l][1], bias  (rho mean[l'][1] - mean[l][1]) / std[l][1]
 *     (with l' = l and no sign change these are dc_group_fuse_maps' (rho, (rho - 1) mean / std)).  Gain and bias are computed on the host in
 *     double and uploaded as float; a third table of the same size holds the source channel, as int.
 *  Fusion: unchanged — the ascending sum over the members, times 1 / M, in float32; nothing is atomic, same inputs give the same bits.
 * One launch fuses every map, member and image, as before.  A group without a mirrored member (fm NULL, fm->mirror NULL or all zeros)
 * takes dc_group_fuse_maps' own path and kernel: the results are bit-identical to the unmirrored calls and nothing else of fm is read.
 * dc_group_detect_parts_mirrored / dc_group_assemble_people_mirrored: dc_group_detect_parts / dc_group_assemble_people on maps fused so.
 * Errors, raised before any device work and naming what is wrong: everything the unmirrored calls refuse, in the same way; then, with a
 *     mirrored member, DC_EINVAL for image_width <= 0, a mirrored base member, joint_mirror NULL, out of range or not an involution, and
 *     — only when next_pred takes part — fm->n_edges different from n_edges, NULL edges, or an edge whose mirrored edge is not among
 *     the edges.                                                                                                                        */
typedef struct dc_fuse_mirror {
  const int* mirror;       /* [M] 0/1 per member */
  int        image_width;  /* pixels of the unscaled image every member saw */
  const int* joint_mirror; /* [J], an involution: pi[pi[j]] == j */
  int        n_edges;      /* with edges: needed whenever next_pred takes part and a member is mirrored */
  const int* edges;        /* [n_edges][2] 0-based (joint, next joint), as dc_net_assemble_people */
} dc_fuse_mirror;
int dc_group_forward_images_mirrored(dc_group* group, const unsigned char* const* images, const int* n, const int* height, const int* width,
                                     const double* scale, const int* mirror /* [M], 0/1; NULL = none */, int is_device, float* const* prob,
                                     float* const* loc_pred, float* const* next_pred, void* stream);
int dc_group_fuse_maps_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, int n_edges, const double* mean,
                                const double* stdev, float* prob, float* loc_pred, float* next_pred, int is_device, void* stream);
int dc_group_detect_parts_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, float threshold, int radius,
                                   int max_det, int* counts, double* dets);
int dc_group_assemble_people_mirrored(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, const dc_assemble_params* p,
                                      int n_edges, const int* edges, const double* mean, const double* stdev, const int* joint_order,
                                      int* n_people, double* people, int* cand, double* cost);
/* ---- fused multi-scale and mirrored poses for the single-person entry and the box entry ----------------------------------------------
 * NO REFERENCE COUNTERPART, PARITY UNPINNED BY THE REFERENCE: the reference decodes every scale of its pyramid on its own and keeps the
 * "best" one (estimate_pose.py:119-126), combines no maps and mirrors nothing.  Decoding the FUSED maps is this project's own rule; the
 * fusion is dc_group_fuse_maps[_mirrored]'s, the decode is `_pose_from_mats` (:131-143) as dc_net_decode_pose / dc_net_forward_boxes run it.
 *
 * dc_group_decode_pose: the members hold, from their last forward, the same NB images at scales[m]; fm is NULL or as in
 *     dc_group_fuse_maps_mirrored.  `prob` and `loc_pred` alone are fused, by that rule, in the same launch and with the same tables as
 *     dc_group_detect_parts_mirrored — so it also works on members whose outputs are narrowed to these two (DC_OPT_OUTPUTS) —, then every
 *     joint's first maximum of the fused float32 `prob` in row-major order is refined by the fused `loc_pred` at s_b = scales[base]:
 *     pose[NB][5][J] doubles, as dc_net_decode_pose.  Host or device destination and `stream` as in dc_group_fuse_maps.  Refuses what
 *     dc_group_detect_parts_mirrored refuses of its scales, base and fm, in the same order and before any device work.
 *
 * dc_group_forward_boxes_mirrored: dc_group_forward_boxes with mirror[c] != 0 marking the members that pre-process every crop flipped
 *     left to right: crop column w - 1 - sx wherever column sx of the unpadded crop would be read, applied after the clamp that makes the
 *     replicate padding (which therefore repeats the flipped crop's last column, the crop's original column 0); resample tables, mean and
 *     canvas are untouched, so a mirrored member's input and maps are, bit for bit, those of dc_group_forward_boxes on the host-flipped
 *     image with every box reflected as (W - x1, y0, W - x0, y1), for float32, float16 and bfloat16 nets.  The member remembers that its
 *     last box batch was mirrored.  The maps returned for it are its RAW maps, in the flipped crop's frame, and there is no `pose`
 *     argument, for the reason dc_group_forward_images_mirrored has none.  mirror NULL or all zeros enqueues exactly what
 *     dc_group_forward_boxes enqueues.
 *
 * dc_group_decode_boxes: on the n boxes of the members' last (dc_net_ / dc_group_)forward_boxes[_mirrored] — every member keeps its own
 *     table of them, nothing is passed again.  The fusion rule is dc_group_fuse_maps[_mirrored]'s with the pyramid scales as the member
 *     scales: q = pyramid_scales[m] / pyramid_scales[base], rho = pyramid_scales[base] / pyramid_scales[m], the same for every box, so
 *     gain, bias and source channels are unchanged.  The one difference is the reflected column of a mirrored member, which every box has
 *     of its own: for box i of width cw_i = x1 - x0, ws[m][i] = (double)(cw_i - 1) * (scales[i] * pyramid_scales[m]) — the inner product
 *     being the scale the member ran that box at — and u = ((ws[m][i] - (8c + 4) q) - 4) / 8, in this order; clamp, floor, corners and
 *     float weights as there.  THE CLAMP STAYS AT THE MEMBER'S WHOLE MAP, the common canvas, not at the crop's own cells: cells past a
 *     crop's own canvas hold the net's answer to the zero canvas, and the decode never looks at them.
 *     The decode is dc_net_forward_boxes' on the fused float32 maps with the base member's own items: scale scales[i] *
 *     pyramid_scales[base], offset (x0, y0), arg-max (first maximum in row-major order) restricted to the crop's own canvas on the base
 *     grid.  prob / loc_pred: the fused maps as NCHW float32 [n][C][H_b][W_b] on the base member's canvas; pose: [n][5][J] doubles in image
 *     coordinates; any of the three NULL.  Host or device destinations and `stream` as in dc_group_fuse_maps.
 *     Errors, before any device work: DC_EINVAL naming the member that holds another number of boxes than member 0; what
 *     dc_group_detect_parts_mirrored refuses of the scales, base and fm (a mirrored base member included) except that fm->image_width is
 *     not read; DC_EINVAL naming the member whose fm->mirror flag disagrees with what its last box batch was; DC_EINVAL when no boxes
 *     are held or the maps are not those of the boxes.  Then DC_ENOCPU in CPU mode.                                                     */
int dc_group_decode_pose(dc_group* group, const double* scales, int base, const dc_fuse_mirror* fm, double* pose, int is_device, void* stream);
int dc_group_forward_boxes_mirrored(dc_group* group, const unsigned char* image, int height, int width, int is_device, const int* boxes,
                                    const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w,
                                    const int* mirror /* [M], 0/1; NULL = none */, float* const* prob, float* const* loc_pred,
                                    float* const* next_pred, void* stream);
int dc_group_decode_boxes(dc_group* group, const double* pyramid_scales, int base, const dc_fuse_mirror* fm, float* prob, float* loc_pred,
                          double* pose, int is_device, void* stream);
/* dc_group_forward_images[_mirrored] / dc_group_forward_boxes[_mirrored] on video frames (dc_frame, above: the rule, the staging, the
 * errors).  frames[c] is member c's array of n[c] frames; pose entries of a mirrored member are the caller's to leave NULL.     */
int dc_group_forward_frames(dc_group* group, const dc_frame* const* frames, const int* n, const int* height, const int* width,
                            const double* scale, const int* mirror /* [M], 0/1; NULL = none */, int is_device, float* const* prob,
                            float* const* loc_pred, float* const* next_pred, double* const* pose, void* stream);
int dc_group_forward_boxes_frame(dc_group* group, const dc_frame* frame, int height, int width, int is_device, const int* boxes,
                                 const double* scales, int n, const double* pyramid_scales, int canvas_h, int canvas_w,
                                 const int* mirror /* [M], 0/1; NULL = none */, float* const* prob, float* const* loc_pred,
                                 float* const* next_pred, double* const* pose, void* stream);
/* the merged plan of the last forward: one line per launch ("conv_gemm_mp<tile> problems=.. grid=.." or "member c: <kernel>");
 * NULL + dc_last_error() before the first forward; pointer valid until the next call on this group                            */
const char* dc_group_plan_text(dc_group* group);
/* every launch of that plan timed with hipEvents (iters runs each), same table as dc_net_profile_text                        */
const char* dc_group_profile_text(dc_group* group, int iters);
/* dc_net_tune_report / dc_net_set_tile for the merged launches of the last forward's plan: signature = "G<problems>:" + the members'
 * signatures joined by '|' (the key DC_TUNE_CACHE files carry for them); set_tile wants the group idle (it synchronises the members'
 * own streams; work enqueued on a caller's stream is the caller's to wait for)                                              */
const char* dc_group_tune_report(dc_group* group);
int dc_group_set_tile(dc_group* group, const char* signature, const char* tile);
#define DC_GSTAT_MERGES 0               /* times the members' plans were merged into a group plan                  */
#define DC_GSTAT_GRAPH_INSTANTIATIONS 1 /* hipGraph captures + instantiations of group plans                       */
#define DC_GSTAT_AUTOTUNE_RUNS 2        /* group plans for which at least one merged signature had to be timed     */
#define DC_GSTAT_PLAN_HITS 3            /* forwards served by a cached group plan                                  */
#define DC_GSTAT_LAUNCHES 4             /* launches of the last forward's plan                                     */
#define DC_GSTAT_MULTI_LAUNCHES 5       /* ... of which multi-problem                                              */
#define DC_GSTAT_LANES 6                /* lanes of the last forward's plan                                        */
#define DC_NUM_GSTATS 7
int dc_group_stats(dc_group* group, long long* out, int n);
/* algorithmic FLOPs of the last grouped forward (the members' dc_net_flops summed)                                          */
int dc_group_flops(dc_group* group, double* out);

/* ---- tracking: the same person across the frames of a video, identities kept on the device --------------------------------------
 * PARITY UNPINNED BY THE REFERENCE: the reference repository stops at the maps and has no tracker.  As with the assembly rule of
 * dc_net_assemble_people, the rule below is this project's own; tests/track_ref.py restates it in float64 NumPy.
 *
 * A tracker has S slots.  A slot is one independent sequence: image b of a call updates slot b, or the slot a slot map names (below).
 * Each slot has T track places and a counter next_id that starts at 0.  A live track holds: id; pose[J][3] = x, y, score in image pixels (a joint is HELD when its score
 * > 0); vel[J][2]; misses; hits.  An update of a slot with the people[n][J][3] of a frame (n <= P <= 256) does the following, all
 * arithmetic in double, sums over joints ascending:
 *  1. Track size.  s_i = max(min_size, max(x extent, y extent) over the held joints of pose_i); one held joint has extent 0.
 *  2. Predicted joints.  pred_i[j] = pose_i[j] + (motion == 1 ? vel_i[j] * (misses_i + 1) : 0).
 *  3. Distance.  Over the n_c joints held by both track i and person q:
 *         D[i][q] = (sum_j ((pred_x - q_x)^2 + (pred_y - q_y)^2) / (s_i^2 * sigma_j^2)) / n_c,
 *     +inf when n_c < min_common, when place i is free, or when q >= n.
 *  4. Greedy matching.  While an unmatched live track and an unmatched person with D <= max_dist remain, the pair with the smallest D
 *     is matched; ties go to the lower place i, then the lower q.
 *  4'. Optimal assignment, INSTEAD of step 4 in a tracker whose option DC_TRACK_OPT_ASSIGN is DC_TRACK_ASSIGN_OPTIMAL (below; the
 *     default is step 4).  Greedy matching swaps identities when two people pass each other: the closest pair is taken first and the
 *     leftover pair forced together even when the other pairing is far better overall.  Step 4' solves the linear assignment problem.
 *     Rows are the places live at the start of the update in ascending place order, r = 1..R (place i_r); real columns are the frame's
 *     people, c = 1..n for person q = c - 1; dummy columns are c = n+1..n+R; m = n + R <= 512.  C[r][c] of a real column is
 *     D[i_r][q] when `D <= max_dist` is true and +inf otherwise (a NaN distance is forbidden, as in step 4); C[r][c] of a dummy column
 *     is max_dist for every row: an unmatched track costs max_dist.  The matching is what this procedure returns — the shortest
 *     augmenting path Hungarian method with row duals u and column duals v, all in double, nothing but subtract, add and compare:
 *         u[0..R] = 0, v[0..m] = 0, p[0..m] = 0, way[0..m] = 0
 *         for r = 1..R:
 *             p[0] = r; j0 = 0; minv[1..m] = +inf; used[0..m] = false
 *             repeat:
 *                 used[j0] = true; i0 = p[j0]; delta = +inf
 *                 for j = 1..m ascending, not used[j]:
 *                     cur = (C[i0][j] - u[i0]) - v[j]
 *                     if cur < minv[j]: minv[j] = cur; way[j] = j0
 *                     if minv[j] < delta: delta = minv[j]; j1 = j        (strict: the lowest j among equal minima)
 *                 for j = 0..m: if used[j]: u[p[j]] += delta; v[j] -= delta
 *                               else:       minv[j] -= delta
 *                 j0 = j1
 *             until p[j0] == 0
 *             repeat: j1 = way[j0]; p[j0] = p[j1]; j0 = j1  until j0 == 0
 *     Person q is matched to place i_{p[q+1]} when p[q+1] != 0; a row that sits on a dummy column is unmatched.  The total — the sum of
 *     D over the matched pairs + max_dist * (the unmatched live tracks) — is minimal, and no matched pair has D > max_dist.  An allowed
 *     pair with D == max_dist ties with a dummy column; the scan order above decides that tie and every other one, which is why the rule
 *     is the procedure itself and not merely "an optimum".  Deterministic.  A dummy column with finite cost is always unused, so delta is
 *     always finite, the inner loop marks one new column per trip and ends within m + 1 trips; the kernel holds both loops to these
 *     bounds as hard trip limits, so that no input can make it spin.  PARITY UNPINNED BY THE REFERENCE, like the rest of the tracker:
 *     there is no reference counterpart; tests/assign_ref.py restates the procedure in float64 loops.  Steps 1-3 and 5-7 are shared.
 *  5. Matched track.  vel[j] = (person - old pose) / (misses + 1) for the joints held by both the old pose and the person, 0 elsewhere;
 *     pose = the person's, whole (a joint the person lacks becomes not held); misses = 0; hits += 1.
 *  6. Unmatched live track.  misses += 1; pose and velocity stay; the track is freed when misses > max_misses.
 *  7. Births.  The unmatched people, q ascending, take the free places, place index ascending (places freed in step 6 of this update
 *     count as free): id = next_id++, hits = 1, misses = 0, vel = 0.  A person for whom no place is free gets id -1 and is not
 *     tracked.  Ids are never reused within a slot (the opt-in appearance steps below give a RETURNING person their old id back: step 7').
 *  8. Smoothed poses, OPT-IN (dc_tracker_set_smoothing; off by default, and nothing above changes by a bit when it is off or on).
 *     PARITY UNPINNED BY THE REFERENCE, like the rest of the tracker: the reference stops at the maps; tests/smooth_ref.py restates this
 *     step in float64 loops.  The raw assembly result jitters from frame to frame, and a joint that falls below the threshold for one
 *     frame comes back as (0, 0, 0); step 5 forgets it too.  Step 8 keeps a filter per track place and joint and returns, beside ids and
 *     place, a smoothed pose per person in which short gaps are bridged.  All arithmetic is in double, in the order written.  Smoothing
 *     influences no decision: ids, place, dist and everything dc_tracker_state returns are bit for bit what they are without it.
 *     Parameters (dc_track_smooth_params): min_cutoff (finite, > 0; cycles per update), beta (finite, >= 0: how much a surprise opens
 *     the filter), d_cutoff (finite, > 0; cycles per update, for the rate estimate), max_hold (0..1000: updates a joint may be
 *     bridged).  Time is counted in updates — one image of a slot is one update —, so a 1 Hz cutoff on 30 fps video is
 *     min_cutoff = 1/30.  THE DEFAULTS THE PYTHON LAYER CHOOSES (0.1, 4.0, 0.03, 3) ARE PLACEHOLDERS, NOT TUNED ON REAL VIDEO.
 *     Helper: A(fc, dt) = r / (r + 1) with r = (TWO_PI * fc) * dt and TWO_PI = 6.283185307179586.
 *     Filter state per track place i and joint j: fx, fy (position), dx, dy (rate per update), fs (last observed score), gap (updates
 *     since the last observation), n (0: holds nothing, 1: one observation, 2: running).  After steps 5-7 of an image:
 *     8a. A place matched in step 5 to person q, or born in step 7 from q.  On birth the place's filter is cleared first (n = 0 for
 *         every joint).  s is the step-1 size of the person's pose, which is the track's new pose.  For every joint, with (px, py, ps)
 *         the person's values:
 *           held (ps > 0), n == 0:  fx = px; fy = py; dx = dy = 0; fs = ps; gap = 0; n = 1.  Out (px, py, ps), src 1.
 *           held, n == 1:  dt = gap + 1; dx = (px - fx) / dt; dy = (py - fy) / dt; fx = px; fy = py; fs = ps; gap = 0; n = 2.
 *                          Out (px, py, ps), src 1.  (The rate starts from the first difference: started from zero it takes tens of
 *                          frames to catch up with a walking person.)
 *           held, n == 2:  dt = gap + 1; qx = fx + dx * dt; qy = fy + dy * dt; ex = px - qx; ey = py - qy;
 *                          a = A(min_cutoff + beta * ((|ex| + |ey|) / s), dt); b = A(d_cutoff, dt);
 *                          fx = qx + a * ex; fy = qy + a * ey; dx = dx + b * (ex / dt); dy = dy + b * (ey / dt); fs = ps; gap = 0.
 *                          Out (fx, fy, ps), src 1.  (Predict, then correct: unlike a plain low-pass this has no lag behind a constant
 *                          velocity; the surprise, normalised by the person's size, opens the filter, so a real change of direction
 *                          is followed quickly.)
 *           not held, n > 0:  gap += 1.  If gap > max_hold: n = 0, out (0, 0, 0), src 0.  Otherwise out (fx + dx * gap, fy + dy * gap,
 *                          fs), src 2: a BRIDGED joint.
 *           not held, n == 0:  out (0, 0, 0), src 0.
 *     8b. A live track that step 6 left unmatched and did not free.  For every joint with n > 0: gap += 1, and n = 0 when
 *         gap > max_hold.  A freed place has n = 0 everywhere.
 *     8c. A person with id -1 (no free place): out is the person as given, src 1 for held joints.  Entries q >= n_people: zeros.
 *     Scores are not smoothed, real timestamps (variable frame intervals) are not taken, and bridged joints take no part in the matching.
 * Deterministic: the same calls give the same ids.  dc_tracker_reset(slot) frees the slot's tracks and sets next_id back to 0; it
 *     clears the slot's filters of step 8 as well.
 *
 * dc_tracker_create: slots 1..64; max_tracks (T) 1..256; n_joints (J) 1..32; sigma[J] NULL (all 1.0) or each finite and > 0;
 *     max_misses >= 0; min_common 1..J; max_dist finite and >= 0; min_size finite and > 0; motion 0 or 1.  Anything else is DC_EINVAL
 *     naming the parameter.  Creation needs no device: the device buffer is allocated, zeroed and bound to the calling thread's device
 *     (the net's, in the chained entries) at the first update.  THE DEFAULTS THE PYTHON LAYER CHOOSES FOR max_misses, min_common,
 *     max_dist, min_size AND sigma ARE PLACEHOLDERS, NOT TUNED ON REAL VIDEO: override them.
 * dc_tracker_set_option / dc_tracker_get_option: key DC_TRACK_OPT_ASSIGN, value DC_TRACK_ASSIGN_GREEDY (step 4, the default) or
 *     DC_TRACK_ASSIGN_OPTIMAL (step 4').  Setting needs no device and works before the first update, like creation.  It orders itself
 *     like the other synchronous calls: it waits for the last enqueued update, then stores the value, and every update enqueued
 *     afterwards uses it.  The slots' state is untouched, so a sequence may switch rule between frames.  An unknown key or value is
 *     DC_EINVAL naming it.  dc_tracker_params carries no option: it has no size field and compiled callers exist.
 * dc_tracker_set_smoothing / dc_tracker_get_smoothing: step 8's switch and parameters; NULL (or enabled == 0) is off, the default.  They
 *     need no device and order themselves like dc_tracker_set_option: set waits for the last enqueued update, after which every update
 *     enqueued later uses the new value.  Going from off to on starts with empty filters; changing parameters while on keeps the
 *     filters.  A bad value is DC_EINVAL naming the field.  The filters are a device allocation of their own, 48 bytes per place and
 *     joint, made at the first update with smoothing on; a tracker that leaves smoothing off runs the kernels it ran without step 8.
 * dc_tracker_update_smoothed: dc_tracker_update_slots plus smooth[nb][P][J][3] and src[nb][P][J] (int: 0 nothing, 1 observed,
 *     2 bridged; either may be NULL).  DC_EINVAL when smoothing is off.  The other update entries advance the filters too when
 *     smoothing is on; they merely do not return step 8's outputs.
 * dc_tracker_smooth_state: where the filters of a slot expect every joint now: poses[T][J][3] = (fx + dx * gap, fy + dy * gap, fs) and
 *     gap[T][J] where n > 0, zeros and -1 elsewhere (either may be NULL).  Synchronous like dc_tracker_state.
 * Chained entries with smoothing on (dc_net_track_people[_slots], dc_group_track_people[_slots], dc_net_track_frames_async; no
 *     signature changes): `people` is downloaded from the smoothed poses and `cand` carries -3 at bridged joints, next to -2 for filled
 *     ones; n_people, cost, ids and place are what they were, and the net's own device copies of the people stay raw.  The sparse
 *     pairwise head, fused pyramids, mirrored groups, completion and dedupe are covered: the tracker receives what those stages leave.
 *     Step 8's outputs leave the tracker's scratch in front of the tracker's event, so a later update cannot overwrite what an earlier
 *     asynchronous call has not downloaded yet.
 * dc_tracker_update: host poses — n_people[nb], people[nb][P][J][3] (entries of q >= n_people[b] are not read) — are uploaded and
 *     image b updates slot b in one launch (one workgroup per slot).  This is how top-down poses of dc_net_forward_boxes get tracked.
 *     Outputs: ids[nb][P] (long long; -1 for q >= n and for an untracked person), place[nb][P] (int, the track place; -1 likewise; may
 *     be NULL), dist[nb][T][P] (the D of step 3; may be NULL: diagnostics and tests).
 * Slot map (dc_tracker_update_slots, dc_net_track_people_slots, dc_group_track_people_slots): slot_of[nb], each in [0, S), says which slot
 *     image b updates, so that several consecutive frames of ONE video travel in one call (a batch forward of k frames, slot_of = k times
 *     the sequence's slot).  Images with the same slot are applied in ascending b, each on the state the one before left; images with
 *     different slots are independent.  The result — ids, place and dist per image, the slots' state — is by definition that of applying
 *     the images one at a time.  A slot no image names is not touched.  With a map nb may be 1..64 whatever S is; the tracker's per-image
 *     scratch grows to the largest nb seen.  slot_of == NULL is the identity map of the entries without it (nb <= S), which are these
 *     entries called with NULL.  One launch either way: one workgroup per slot walks the images of its slot.
 * dc_net_track_people / dc_group_track_people: dc_net_assemble_people / dc_group_assemble_people[_mirrored] (fm may be NULL) with the
 *     tracker's launch behind the assembly's on the same stream, reading the people where the assembly left them on the device: one more
 *     launch, no more transfer than the ids.  They return what the assembly entries return, unchanged, plus ids / place
 *     [n][max_people].  The sparse pairwise path (DC_OPT_SPARSE_PAIRWISE) is covered.
 * dc_tracker_state: a slot's tracks, e.g. to see where occluded people were last seen: ids[T], misses[T], hits[T], poses[T][J][3]
 *     (any may be NULL); free places give -1 / 0 / 0 / zeros.  Before the first update every place is free.
 * dc_net_track_frames_async: the whole video chain on the net's own stream with NO host wait — it enqueues the upload of host planes,
 *     the pre-processing launch, the forward, candidates, the sparse pairwise head when DC_OPT_SPARSE_PAIRWISE applies, pair costs,
 *     assembly, the tracker's launch and the downloads — and returns when all of this is enqueued.  The input is n video frames
 *     (frames, as dc_net_forward_frames) or, with frames == NULL, n packed BGR images (images, as dc_net_forward_images); scale and
 *     p->scale are the pre-processing's and the assembly's as in the synchronous entries.  tracker may be NULL: people without ids, and
 *     ids must then be NULL too.  slot_of as above (NULL: image b -> slot b).  Outputs: n_people[n], people[n][max_people][J][3],
 *     cand[n][max_people][J] (may be NULL), ids / place [n][max_people] (place may be NULL).  dc_net_busy / dc_net_synchronize tell when
 *     the outputs are there, as for dc_net_forward_host_async.  Lifetimes: frame planes (host or device) and the output arrays must
 *     stay valid and untouched until then; everything small — params, edges, statistics, joint order, slot map, frame descriptors — is
 *     copied before the return.  Output arrays and host planes from dc_host_alloc are moved by the DMA engines in place; pageable ones
 *     work too and are staged by the runtime (the call may then wait for earlier copies).  A second call on a net that is still busy
 *     queues behind the first in stream order; to overlap calls, issue them on a net and its clones — the tracker keeps their updates in
 *     the order of the calls.  The results equal those of dc_net_forward_frames / dc_net_forward_images followed by
 *     dc_net_track_people[_slots] (or dc_net_assemble_people), bit for bit.  There is no asynchronous group (pyramid / mirror) entry.
 * Order: updates of a tracker apply in the order of the host calls that enqueued them, whichever net, clone, group or stream carried
 *     them.  The tracker holds an event: every enqueue of an update makes its stream wait for the event of the update before it (on
 *     the device, no host wait) and records the event again behind its own launch and copies; the library's runtime lock is held for the
 *     enqueue only.  The synchronous calls — dc_tracker_update[_slots], dc_tracker_state, dc_tracker_reset, dc_tracker_destroy and the
 *     synchronous dc_*_track_people[_slots] — wait on the host for the last enqueued update first and return with their own work done,
 *     so dc_tracker_state called with asynchronous requests in flight returns the state after all of them.
 * Errors, before any device work: DC_EINVAL naming the parameter for nb outside [1, slots] (with a slot map: outside [1, 64]), a
 *     slot_of[b] outside [0, slots), ids without a tracker (dc_net_track_frames_async, which refuses what dc_net_forward_frames,
 *     dc_net_assemble_people and dc_tracker_update refuse, in that order), P (max_people) outside [1, 256], a
 *     n_people[b] outside [0, P], a slot outside [0, slots) (dc_tracker_reset: -1 = all); DC_ESHAPE for a tracker whose n_joints is not
 *     the net's; whatever the assembly entry refuses.  Then DC_ENOCPU for an update in CPU mode (there is no CPU path), DC_EDEVICE for
 *     a tracker bound to another device than the calling thread's (the net's).                                                        */
typedef struct dc_tracker dc_tracker;
typedef struct dc_tracker_params {
  int    slots;          /* S, 1..64 */
  int    max_tracks;     /* T, 1..256 */
  int    n_joints;       /* J, 1..32 */
  const double* sigma;   /* [J] per-joint tolerance, NULL = all 1.0 */
  int    max_misses;     /* a track is freed after more than this many updates in a row without a match */
  int    min_common;     /* joints a track and a person must both hold to be compared */
  double max_dist;       /* a match needs D <= max_dist */
  double min_size;       /* lower bound of the track size s_i, image pixels */
  int    motion;         /* 0: compare with the last pose; 1: with the pose moved on by its velocity */
} dc_tracker_params;
int dc_tracker_create(const dc_tracker_params* p, dc_tracker** out);
int dc_tracker_destroy(dc_tracker* tracker);
int dc_tracker_reset(dc_tracker* tracker, int slot /* -1: all */);
int dc_tracker_update(dc_tracker* tracker, int nb, int P, const int* n_people, const double* people, long long* ids, int* place,
                      double* dist);
int dc_tracker_update_slots(dc_tracker* tracker, int nb, int P, const int* slot_of /* [nb], NULL: image b -> slot b */,
                            const int* n_people, const double* people, long long* ids, int* place, double* dist);
int dc_tracker_state(dc_tracker* tracker, int slot, long long* ids, int* misses, int* hits, double* poses);
#define DC_TRACK_OPT_ASSIGN     1
#define DC_TRACK_ASSIGN_GREEDY  0   /* step 4, the default */
#define DC_TRACK_ASSIGN_OPTIMAL 1   /* step 4' */
int dc_tracker_set_option(dc_tracker* tracker, int key, int value);
int dc_tracker_get_option(dc_tracker* tracker, int key, int* value);
typedef struct dc_track_smooth_params {
  int    enabled;     /* 0 / 1: the switch */
  double min_cutoff;  /* finite, > 0; cycles per update */
  double beta;        /* finite, >= 0; how much a surprise opens the filter */
  double d_cutoff;    /* finite, > 0; cycles per update, for the rate estimate */
  int    max_hold;    /* 0..1000: updates a joint may be bridged */
} dc_track_smooth_params;
int dc_tracker_set_smoothing(dc_tracker* tracker, const dc_track_smooth_params* p /* NULL: off */);
int dc_tracker_get_smoothing(dc_tracker* tracker, dc_track_smooth_params* out);
int dc_tracker_update_smoothed(dc_tracker* tracker, int nb, int P, const int* slot_of /* [nb], NULL: image b -> slot b */,
                               const int* n_people, const double* people, long long* ids, int* place, double* dist,
                               double* smooth /* [nb][P][J][3] */, int* src /* [nb][P][J] */);
int dc_tracker_smooth_state(dc_tracker* tracker, int slot, double* poses /* [T][J][3] */, int* gap /* [T][J] */);
int dc_net_track_people(dc_net* net, dc_tracker* tracker, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean,
                        const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, double* cost,
                        long long* ids, int* place);
/* ---- the tracker's appearance steps: a returning person takes their old id, OPT-IN (off by default) ----------------------------------
 * PARITY UNPINNED BY THE REFERENCE, like the rest of the tracker; the rule is this project's own, and tests/appear_ref.py restates it.
 * Steps 6 and 7 above free a track after max_misses updates and never reuse an id, so a person who walks behind a pillar for two
 * seconds comes back as a new person.  With appearance on, a freed track's appearance model waits in a gallery for a while, and a
 * person who is born with a descriptor (dc_describe_people, below) close enough to an entry takes that entry's id.  The rule is ALL
 * INTEGER.  Steps 1-7 and 8 are untouched: place, dist, the tracks' poses and everything step 8 returns are bit for bit what they are
 * without it; only ids and next_id differ, and only from the first re-identification on.  With appearance off nothing changes by a bit,
 * and the kernels are the ones a tracker without it ran.
 *   Quantised descriptor.  A descriptor h[3][16] with n = sum_k h[0][k] >= min_pixels is VALID; then q[c][k] = (4096 * h[c][k] + n / 2) / n
 *     in int64, integer division.  Rounding lets a channel of q sum to 4096 +- 8.
 *   Dissimilarity.  A(m, q) = 12288 - sum_c sum_k min(m[c][k], q[c][k]), an int; it may be as low as -24, and nothing depends on its sign.
 *   Model update.  m += ((q - m) * alpha256 + 128) >> 8 per element, the shift arithmetic; the first valid observation sets m = q.
 *   State per slot, beside the tracks: model[T][48] and valid[T]; a gallery of DC_TRACK_GALLERY = 64 entries, each (id, age, model[48]).
 *   0'. At the start of an image's update every occupied gallery entry gets age += 1 and is freed when age > max_age.
 *   5'. A track matched in step 5 whose person has a valid descriptor updates its model.
 *   6'. The tracks freed by step 6 in this update, place ascending, that have hits >= min_hits and a valid model enter the gallery with
 *       age 0, one after the other: each into the lowest free entry; with none free it replaces the entry of largest age, the lower
 *       index among equals.
 *   7'. INSTEAD of step 7's ids.  The places are step 7's.  Among the unmatched people who receive a place and have a valid descriptor:
 *       while such a person and an occupied entry with A(entry.model, q) <= reid_max remain, the pair with the smallest A is taken — ties
 *       go to the lower entry index, then to the lower person, step 4's idiom.  The person's new track takes the entry's id, its model is
 *       the entry's updated with q, the entry is freed, reid = 1.  Every other born person takes next_id + (their rank among the born
 *       people not re-identified, q ascending), and next_id advances by that count; their model is q when valid, else not valid.
 *       hits = 1, misses = 0, vel = 0 as in step 7, and step 8's filters are cleared as on any birth.  Entries pushed by step 6' of the
 *       same update take part.
 *   Invariants: an id is live at most once, and is never in the gallery while live.
 *   An update without descriptors — the older update entries, the chained entries, or desc == NULL — counts everyone's descriptor as not
 *   valid: steps 0' and 6' still run, nobody is re-identified, and the ids are the plain rule's.
 * dc_tracker_set_appearance / dc_tracker_get_appearance: the switch and parameters; NULL (or enabled == 0) is off.  They need no device
 *     and order themselves like dc_tracker_set_smoothing.  Off -> on starts with no model and an empty gallery; a parameter change
 *     while on keeps them; dc_tracker_reset clears the slot's.  A bad value is DC_EINVAL naming the field.  The state is a device
 *     allocation of its own, made at the first update with appearance on, as the filters of step 8 are.  THE DEFAULTS THE PYTHON LAYER
 *     CHOOSES ARE PLACEHOLDERS, NOT TUNED ON REAL VIDEO.
 * dc_tracker_update_appearance: dc_tracker_update_slots plus desc[nb][P][3][16] (host, as dc_describe_people returns it; may be NULL)
 *     and reid[nb][P] (1: the person took an id from the gallery; may be NULL); smooth and src as dc_tracker_update_smoothed, NULL when
 *     smoothing is off.  DC_EINVAL when appearance is off, or when smooth / src are given with smoothing off.
 * dc_tracker_appearance_state: track_model[T][48] and track_valid[T] (zeros for a place that is free or has no valid model),
 *     gallery_ids[64], gallery_age[64] (-1 for a free entry) and gallery_model[64][48] (zeros likewise); any may be NULL.  Synchronous
 *     like dc_tracker_state.
 * Not built, on purpose: descriptors inside the chained and asynchronous entries, an appearance term inside the distance of step 3,
 *     learned embeddings.                                                                                                          */
typedef struct dc_track_appearance_params {
  int enabled;      /* 0 / 1: the switch */
  int min_pixels;   /* >= 1: a descriptor with fewer region pixels is not valid */
  int alpha256;     /* 0..256: weight of a new observation in the model */
  int reid_max;     /* 0..12288: largest dissimilarity that re-identifies */
  int max_age;      /* 0..100000: updates a freed track stays in the gallery */
  int min_hits;     /* >= 1: hits a freed track needs to enter the gallery */
} dc_track_appearance_params;
#define DC_TRACK_GALLERY 64
int dc_tracker_set_appearance(dc_tracker* tracker, const dc_track_appearance_params* p /* NULL: off */);
int dc_tracker_get_appearance(dc_tracker* tracker, dc_track_appearance_params* out);
int dc_tracker_update_appearance(dc_tracker* tracker, int nb, int P, const int* slot_of /* [nb], NULL: image b -> slot b */,
                                 const int* n_people, const double* people,
                                 const int* desc /* host [nb][P][3][16], may be NULL: nobody has a valid descriptor */, long long* ids,
                                 int* place, double* dist, int* reid /* [nb][P], may be NULL */, double* smooth /* [nb][P][J][3] */,
                                 int* src /* [nb][P][J] */);
int dc_tracker_appearance_state(dc_tracker* tracker, int slot, int* track_model /* [T][48] */, int* track_valid /* [T] */,
                                long long* gallery_ids /* [64] */, int* gallery_age /* [64] */, int* gallery_model /* [64][48] */);
int dc_group_track_people(dc_group* group, dc_tracker* tracker, const double* scales, int base, const dc_fuse_mirror* fm /* may be NULL */,
                          const dc_assemble_params* p, int n_edges, const int* edges, const double* mean, const double* stdev,
                          const int* joint_order, int* n_people, double* people, int* cand, double* cost, long long* ids, int* place);
int dc_net_track_people_slots(dc_net* net, dc_tracker* tracker, const int* slot_of /* [batch], NULL: image b -> slot b */,
                              const dc_assemble_params* p, int n_edges, const int* edges, const double* mean, const double* stdev,
                              const int* joint_order, int* n_people, double* people, int* cand, double* cost, long long* ids, int* place);
int dc_group_track_people_slots(dc_group* group, dc_tracker* tracker, const int* slot_of /* [batch], NULL: image b -> slot b */,
                                const double* scales, int base, const dc_fuse_mirror* fm /* may be NULL */, const dc_assemble_params* p,
                                int n_edges, const int* edges, const double* mean, const double* stdev, const int* joint_order,
                                int* n_people, double* people, int* cand, double* cost, long long* ids, int* place);
int dc_net_track_frames_async(dc_net* net, dc_tracker* tracker /* NULL: people without ids */, const dc_frame* frames /* or NULL */,
                              const unsigned char* images /* packed BGR when frames is NULL */, int n, int height, int width, double scale,
                              int is_device, const int* slot_of /* NULL: identity */, const dc_assemble_params* p, int n_edges,
                              const int* edges, const double* mean, const double* stdev, const int* joint_order, int* n_people,
                              double* people, int* cand /* may be NULL */, long long* ids, int* place /* both may be NULL; ids must be
                              NULL when tracker is NULL */);

/* ---- people, stage D: joints the assembly missed, filled from the pairwise predictions (opt-in) ------------------------------------
 * NO REFERENCE COUNTERPART, PARITY UNPINNED BY THE REFERENCE: like stages B and C of dc_net_assemble_people this rule is this project's
 * own (the reference repository stops at the maps); tests/complete_ref.py restates it in float64.
 *
 * A person can only hold a joint that survived stage A (score >= threshold, the maximum of its window, among the first max_det).  With
 * completion enabled every entry that assembles people runs one more launch behind stage C, on the device, and looks for each missing
 * joint where the person's held joints say it should be.  The setting is state of the net or the group (dc_assemble_params is
 * unchanged): it covers dc_net_assemble_people, dc_net_track_people[_slots], dc_net_track_frames_async and — set on the group — the
 * dc_group_assemble_people[_mirrored] and dc_group_track_people[_slots] entries; the sparse pairwise path (DC_OPT_SPARSE_PAIRWISE) is
 * covered, because the head was evaluated at exactly the cells of the held candidates.  The tracker's launch receives the completed
 * people.  Not enabled (the default): no launch is added and every result keeps its bits.
 *
 * Inputs: stage A's candidate lists; stage C's people and `cand` AFTER the min_joints drop; the three maps the assembly read (prob,
 * loc_pred, and next_pred or the sparse float32 map); the lookup of the edges, mean, std, scale and the NMS radius of the assembly; the
 * three parameters below.  All arithmetic in double; map values are read as their element type holds them.  For every image b, every
 * surviving person q and every joint j that q does not hold — the items are independent of each other: a joint filled here is NOT a
 * predictor of another fill, so neither order nor thread timing matters:
 *  1. predictors: the joints a, ascending, that q holds from stage C and for which an edge F = the lowest-index edge (a, j) exists; each
 *     gives pred_a = pred(cell of q's candidate of a, F), image pixels, as in stage B.  Fewer than min_support predictors: j stays missing.
 *  2. expected position: e = (the sum of pred_a over a ascending) / their count.  e not finite: j stays missing.
 *  3. window: col0 = floor(e_x * scale / 8), row0 = floor(e_y * scale / 8); rows row0 - fill_radius .. row0 + fill_radius and the same
 *     for columns, clipped to the map.  Empty after clipping: j stays missing.
 *  4. exclusion: a window cell is skipped when it lies within Chebyshev distance `radius` (the assembly's NMS radius) of the cell of a
 *     candidate of joint j that ANY person of image b holds after stage C: such a cell belongs to somebody's peak.  Cells of fills
 *     exclude nothing, so two people may fill the same joint from the same cell.
 *  5. choice: among the remaining cells the one with the largest prob[j], ties to the lower row-major cell index; a NaN score is never
 *     chosen.  If that score is >= fill_threshold the joint becomes x, y = the cell refined with loc_pred exactly as stage A computes a
 *     candidate's x, y, score = prob, and cand = -2.  Otherwise j stays (0, 0, 0) with cand -1.
 * Unchanged by stage D: n_people, the order of people, every joint stage C assigned; min_joints keeps counting stage C's joints only,
 * so completion never changes who survives.
 *
 * dc_net_set_completion / dc_group_set_completion: p == NULL or p->enabled == 0 turns completion off (the other fields are then not
 * read and read back as 0).  Host only, no device needed.  DC_EINVAL naming the field for fill_threshold not finite or <= 0,
 * fill_radius outside [0, 16], min_support < 1.  dc_*_get_completion: what was stored.  dc_net_clone copies the net's setting at clone
 * time; a group has a setting of its own and does not read its members'.  The values are the caller's to choose: nothing here has
 * been tuned on real images.                                                                                                      */
typedef struct dc_complete_params {
  int   enabled;         /* 0: off */
  float fill_threshold;  /* a fill needs prob >= this; > 0 */
  int   fill_radius;     /* half width of the search window, map cells: 0..16 */
  int   min_support;     /* predictors needed, >= 1 */
} dc_complete_params;
int dc_net_set_completion(dc_net* net, const dc_complete_params* p /* NULL: off */);
int dc_net_get_completion(dc_net* net, dc_complete_params* out);
int dc_group_set_completion(dc_group* group, const dc_complete_params* p /* NULL: off */);
int dc_group_get_completion(dc_group* group, dc_complete_params* out);

/* ---- people, stage E: a person who is there twice is suppressed on the device (opt-in) -----------------------------------------------
 * NO REFERENCE COUNTERPART, PARITY UNPINNED BY THE REFERENCE: like stages B to D and the tracker this rule is this project's own (the
 * reference repository stops at the maps); tests/dedupe_ref.py restates it in float64 loops.
 *
 * The assembly produces the same human twice in three ways: a link that costs more than max_cost lets the rest of a body seed a second
 * person (A holds joints 0..6, B holds 7..13); stage D then fills what each fragment lacks — "two people may fill the same joint from
 * the same cell" — so both come back as full skeletons on top of each other; and a small NMS radius or a fused pyramid gives two
 * candidates a cell apart, each of which becomes a person.  Every duplicate is a track of its own in a tracker and a box of its own for
 * a top-down forward.  With dedupe enabled every entry that assembles people runs one more launch behind stage D (behind stage C when
 * completion is off), before the tracker's launch and before the downloads: the tracker and the caller receive the people it kept.
 * The setting is state of the net or the group exactly as completion is, and covers the same entries.  Not enabled (the default): no
 * launch is added and every result keeps its bits.
 *
 * Inputs, per image b: n = n_people[b]; people[q][j] = (x, y, score) and cand[q][j] as the previous stage left them; the parameters
 * below.  All arithmetic in double; sums run over the joints ascending.
 *  1. Held, score, size.  Joint j of q is HELD when its score > 0 (the tracker's definition: a NaN or negative score is not held; a
 *     joint stage D filled, cand == -2, is).  S_q = the sum of the scores of q's held joints.  s_q = max(min_size, max(x extent, y
 *     extent) over q's held joints): step 1 of the tracker rule with this stage's own min_size, computed as the tracker computes it —
 *     the extents are max - min with fmin / fmax, which pass over a NaN, and count only when the x extent is >= 0, i.e. when some held
 *     joint has an x that is not a NaN.
 *  2. Rank.  q ranks before q' when S_q > S_q', or when the two are equal and q < q'.  (S is never a NaN; an infinite score ranks first.)
 *  3. Distance.  For A ranked before B, over the n_c joints both hold:
 *         D(A, B) = (sum_j ((A_x - B_x)^2 + (A_y - B_y)^2) / (s_A^2 * sigma_j^2)) / n_c
 *     — the tracker's step 3 with pred = pose.  A and B are SIMILAR when n_c >= min_common and `D <= max_dist` is true: a NaN distance is
 *     never similar, D == max_dist is.
 *  4. Sweep, in rank order.  A person is SUPPRESSED by the first kept person ranked before it that it is similar to; otherwise it is
 *     KEPT.  A suppressed person suppresses nobody.
 *  5. Absorb (only with absorb = 1).  For a kept A and a joint j with cand_A[j] < 0 (missing or filled), the donors are the people
 *     suppressed by A whose cand[j] >= 0, i.e. assigned by stage C.  If there are any, A's joint j becomes the first-ranked donor's
 *     (x, y, score) and cand.  Steps 1 to 4 read the input only: absorbed joints influence no decision.  Every candidate still belongs
 *     to at most one person, because a donor does not survive.  This turns the two fragments above back into one person made of
 *     stage C's joints only.
 *  6. Compaction.  The kept people stay in ascending input order (stage C's "the others keep their order"); n_people[b] is their count;
 *     entries beyond it are (0, 0, 0) with cand = -1.  The stage writes to buffers of its own and reads its input while it runs.
 * Stage E leaves min_joints and stage D's results for the survivors as they are.  Deterministic: no step depends on thread timing.
 *
 * dc_net_set_dedupe / dc_group_set_dedupe: p == NULL or p->enabled == 0 turns the stage off (the other fields are then not read and
 * read back as 0, sigma as n_sigma = 0).  Host only, no device needed.  DC_EINVAL naming the field for max_dist not finite or < 0,
 * min_common < 1, min_size not finite or <= 0, n_sigma outside [0, 32], sigma NULL with n_sigma != 0, a sigma value not
 * finite or <= 0, absorb other than 0 or 1.  sigma is copied (at most 32 entries); it need not outlive the call.  What only a call
 * that knows the joints can refuse is DC_ESHAPE at the first assembling call: an n_sigma that is neither 0 nor the net's J, and
 * min_common > J.  dc_*_get_dedupe: what was stored; out->sigma is not written — pass sigma_out [32] (may be NULL) for the values.
 * dc_net_clone copies the net's setting at clone time; a group has a setting of its own and does not read its members'.
 * THE DEFAULTS THE PYTHON LAYER CHOOSES ARE PLACEHOLDERS, NOT TUNED ON REAL IMAGES: override them.
 *
 * dc_dedupe_people: the stage alone, on host arrays, synchronous — this is how top-down poses of dc_net_forward_boxes (overlapping
 * detector boxes give the same person twice) are cleaned before dc_tracker_update.  people[nb][P][J][3] and cand[nb][P][J] (entries of
 * q >= n_people[b] are not read).  cand == NULL: a joint counts as assigned exactly when it is held (candidate 0 where held, -1
 * elsewhere, which is also what cand_out then holds), so only missing joints are absorbed.  Outputs: n_out[nb], people_out[nb][P][J][3],
 * cand_out[nb][P][J] (may be NULL), kept_from[nb][P] = the input index of output person o, -1 for o >= n_out[b] (may be NULL),
 * suppressed_by[nb][P] = the input index of the kept person that suppressed q, -1 for a kept q and for q >= n_people[b] (may be NULL).
 * p->enabled is not read.  Errors, before any device work: DC_EINVAL for a NULL p, n_people, people, n_out or people_out, whatever
 * the setters refuse, nb < 1, P outside [1, 256], J outside [1, 32], an n_people[b] outside [0, P]; DC_ESHAPE for n_sigma neither 0
 * nor J and for min_common > J.  Then DC_ENOCPU in CPU mode (there is no CPU path).                                                 */
typedef struct dc_dedupe_params {
  int    enabled;        /* 0: off */
  double max_dist;       /* A and B are the same person when D(A, B) <= max_dist; finite, >= 0 */
  int    min_common;     /* joints both must hold to be compared, >= 1 */
  double min_size;       /* lower bound of the size s_A, image pixels; finite, > 0 */
  const double* sigma;   /* [n_sigma] per-joint tolerance, each finite and > 0; NULL with n_sigma = 0 = all 1.0 */
  int    n_sigma;        /* 0 or the number of joints */
  int    absorb;         /* 1: a kept person takes the assigned joints it lacks from the people it suppressed */
} dc_dedupe_params;
int dc_net_set_dedupe(dc_net* net, const dc_dedupe_params* p /* NULL: off */);
int dc_net_get_dedupe(dc_net* net, dc_dedupe_params* out, double* sigma_out /* [32], may be NULL */);
int dc_group_set_dedupe(dc_group* group, const dc_dedupe_params* p /* NULL: off */);
int dc_group_get_dedupe(dc_group* group, dc_dedupe_params* out, double* sigma_out /* [32], may be NULL */);
int dc_dedupe_people(const dc_dedupe_params* p, int nb, int P, int J, const int* n_people, const double* people,
                     const int* cand /* may be NULL: assigned == held */, int* n_out, double* people_out, int* cand_out /* may be NULL */,
                     int* kept_from /* [nb][P], may be NULL */, int* suppressed_by /* [nb][P] input index or -1, may be NULL */);

/* ---- drawing people into video frames: skeletons blended into BGR24 or NV12 frames in place, on the device ---------------
 * PARITY UNPINNED BY THE REFERENCE: the reference's demo draws with matplotlib / scipy.misc on the host and states no rule.  THE RULE
 * below is this project's own, like the assembly and tracking rules.  It is integer only, so every path gives the same bytes
 * (tests/draw_ref.py restates it in numpy; the device is held to that byte for byte).  No anti-aliasing: it would end byte equality.
 *
 * Input per image b: n_people[b] people of J joints (x, y, score) in image pixels, people[nb][P][J][3], as every people entry returns
 *   them; cand[nb][P][J] (may be NULL): -2 = filled (stage D), -3 = bridged (the tracker's step 8); ids[nb][P] (may be NULL).
 * Which joints are drawn: x, y and score all finite and score > min_score (min_score >= 0, so (0, 0, 0) is never drawn).  A limb — edge
 *   e = (a, c) of the style's skeleton table — is drawn when both its joints are.
 * Snapping: a coordinate is clamped to [-32768, 32768] pixels, then q = (int)rint(16 v): 1/16-pixel fixed point, ties to even.
 *   Radii: r16 = rint(16 radius), radius in [0, 64] pixels; r16 = 0 means that kind of primitive is not drawn.  The centre of pixel
 *   (px, py) is (16 px + 8, 16 py + 8).
 * Coverage, in int64, of the pixel centre p.  w = p - a, v = p - b, d = b - a, L = d.d:
 *   disc at a:            w.w <= r16^2
 *   capsule from a to b:  w.w <= r16^2, or v.v <= r16^2, or (0 < w.d < L and |cross| < 2^31 and cross^2 <= r16^2 L), cross = w.x d.y - w.y d.x
 *   The guard is exact: coordinates are at most 2^19 units, so |d| components are at most 2^20, L <= 2^41 and r16^2 L <= 2^61;
 *   |cross| >= 2^31 implies cross^2 >= 2^62 > r16^2 L — outside —, so the square is never formed and every product that is fits int64.
 * Order: people in index order; of a person the limbs in edge order, then the joints in joint order.  Later primitives go over earlier
 *   ones: with alpha < 256 the order is visible, and it is kept exactly.
 * Blend, per covered pixel and 8-bit channel: out = (c A + dst (256 - A) + 128) >> 8, A = alpha, or alpha_filled for a joint with
 *   cand <= -2 and for a limb with such an end (cand NULL: alpha everywhere).
 * Colour: DC_DRAW_BY_PERSON: palette[key % n_palette] with key = p without ids, key = ids[b][p] when that is >= 0, and the style's
 *   `untracked` colour when it is < 0.  DC_DRAW_BY_JOINT: joint j gets palette[j % n_palette], limb e palette[edges[e][1] % n_palette].
 *   palette is [n_palette][3] R, G, B.
 * BGR24: the pixel's three channels are blended.
 * NV12: luma is blended per pixel with the colour's Y.  A chroma sample (x >> 1, y >> 1) — the siting of dc_frame's rule — is blended
 *   once per primitive, in the same order: with k of the block's n in-frame pixels covered (n = 4, or 2 or 1 at an odd right / bottom
 *   edge) and k > 0, Ac = (A k + n / 2) / n, and Cb and Cr are blended with Ac.  The colour goes R, G, B -> Y, Cb, Cr once per
 *   primitive by the forward counterpart of dc_frame's rule (Kr, Kb, Kg, y0, sy, sc as there; coefficients in double, rounded to
 *   nearest; int32 with an arithmetic shift):
 *     Y  = clip8(y0  + ((yr R + yg G + yb B + 32768) >> 16)),  (yr, yg, yb) = rint(65536 (Kr, Kg, Kb) / sy)
 *     Cb = clip8(128 + ((...) >> 16)),  coefficients rint(65536 (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) / sc)
 *     Cr = clip8(128 + ((...) >> 16)),  coefficients rint(65536 (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) / sc)
 *   BT.601 limited: Y (16829, 33039, 6416), Cb (-9714, -19071, 28784), Cr (28784, -24103, -4681); BT.601 full: (19595, 38470, 7471),
 *   (-11058, -21710, 32768), (32768, -27439, -5329); BT.709 limited: (11966, 40254, 4064), (-6596, -22189, 28784), (28784, -26145,
 *   -2639); BT.709 full: (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005).  Forward and then dc_frame's inverse
 *   comes back within 2 levels (limited) / 1 level (full) on all 2^24 triples (tests/test_draw_host.py).
 * Untouched bytes: bytes of a frame that no primitive covers are not written — pitch padding and, for NV12, chroma samples whose
 *   block no primitive covers included.
 *
 * dc_draw_people: nb frames (1..64) of one height x width (1..16384 each), format, matrix and range, written through their plane
 *   pointers; P in [1, 256], J in [1, 32].  Stand-alone like dc_dedupe_people: no net, people as host arrays.  The call returns when the
 *   drawing is complete: device frames (is_device = 1) are drawn on `stream`, or on the library's utility stream when it is NULL, and the
 *   stream is waited for; host frames are staged up without their padding, drawn, and copied back with 2-D copies (the padding is never
 *   written; a frame nothing is drawn into does not travel).  Only tiles that hold a primitive are launched (one workgroup each); a call
 *   with nothing to draw launches nothing and writes nothing.
 * Errors, before any device work: DC_EINVAL naming the field and the index for what the frame entries refuse (a NULL plane, a pitch
 *   below the minimum, an unknown format / matrix / range, frames that differ in these), nb, height, width, P or J out of range, a NULL
 *   style or palette, n_edges outside [0, 128], an edge joint outside [0, J), a radius outside [0, 64], alpha or alpha_filled outside
 *   [0, 256], min_score not finite or < 0, an unknown color_mode, n_palette outside [1, 256], an n_people[b] outside [0, P].  Then
 *   DC_ENOCPU in CPU mode (there is no CPU path).
 * dc_draw_limits: the tile size and the primitives staged at a time that the kernel was built with (any pointer may be NULL).    */
#define DC_DRAW_BY_PERSON 0
#define DC_DRAW_BY_JOINT  1
typedef struct dc_draw_style {
  int n_edges; const int* edges;            /* [n_edges][2] 0-based joints, 0..128; 0 = joints only */
  double joint_radius, limb_radius;         /* pixels, 0..64 */
  int alpha, alpha_filled;                  /* 0..256 */
  double min_score;                         /* finite, >= 0 */
  int color_mode; const unsigned char* palette; int n_palette; unsigned char untracked[3];
} dc_draw_style;
int dc_draw_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                   const double* people, const int* cand /* may be NULL */, const long long* ids /* may be NULL */,
                   const dc_draw_style* style, void* stream);
int dc_draw_limits(int* tile_w, int* tile_h, int* chunk);

/* ---- blending score maps into video frames: a stride-8 map brought onto the pixel grid of BGR24 or NV12 frames, on the device ------
 * PARITY UNPINNED BY THE REFERENCE: the reference's demo (python/pose/pose_demo.py) draws 14 numpy circles and never shows a map.  THE
 * RULE below is this project's own, like the drawing rule above.  It is integer from the first quantisation on, so every path gives the
 * same bytes (tests/heat_ref.py restates it in numpy; the device is held to that byte for byte, pitch padding included).
 *
 * Input: nb frames as dc_draw_people takes them, a score map S[nb][C][Hm][Wm] (C in [1, 32]; cell (row, col) stands at network pixel
 *   (8 col + 4, 8 row + 4): the stride is 8, as everywhere on the pose path), a geometry — scale: frame pixels x scale = network pixels,
 *   finite, in [1/64, 8]; origin_x, origin_y: the frame pixel coordinates the map's pixel 0 lies at, finite, |.| <= 32768 — and a style.
 * Quantisation, the only floating-point step: a cell's value is widened to float32 (exact for float16 and bfloat16), then
 *   q = (int)rintf(fminf(fmaxf(s, 0), 1) * 4096.0f), NaN counting as 0: q in [0, 4096].  Every operation is exact or correctly rounded.
 * Sample positions, on the host, in double, operation by operation with no fused multiply-add.  Luma column x:
 *   u = ((x + 0.5 - origin_x) * scale - 4.0) / 8.0   (the inverse of x = (8 col + 4) / scale, the pixel's centre at x + 0.5 — the
 *   drawing rule's 16 px + 8), t = (long)rint(256.0 * u) clamped to [0, 256 (Wm - 1)], i0 = t >> 8, f = t & 255, i1 = min(i0 + 1, Wm - 1).
 *   Rows likewise with origin_y and Hm.  NV12: the chroma sample of block (bx, by) has tables of its own, evaluated at the block's centre
 *   — x + 0.5 replaced by 2 bx + 1, y + 0.5 by 2 by + 1 —, at an odd right or bottom edge too.
 * Interpolation, int32, per drawn channel: top = q00 (256 - fx) + q01 fx, bot = q10 (256 - fx) + q11 fx,
 *   v = (top (256 - fy) + bot fy + 32768) >> 16: v in [0, 4096], the largest intermediate is 2^28.
 * What is blended: vmin = (int)rint(4096 min_score); A(v) = alpha (DC_HEAT_ALPHA_CONST) or (alpha v + 2048) >> 12 (DC_HEAT_ALPHA_SCORE);
 *   the blend is the drawing rule's, out = (c A + dst (256 - A) + 128) >> 8.
 *   DC_HEAT_MAX: v = the maximum over the drawn channels of their v (interpolate first, then the maximum); if v >= vmin and A(v) > 0, ONE
 *     blend with colour lut[min(255, v >> 4)].  lut is [256][3] R, G, B and the caller's: the library has none of its own (the Python
 *     binding's caffe.HEAT_LUT is a PLACEHOLDER ramp, not tested for legibility).
 *   DC_HEAT_BY_JOINT: the drawn channels in list order; each one with v_k >= vmin and A(v_k) > 0 is blended with palette[k % n_palette],
 *     k its place in the list (not its channel).  Later channels go over earlier ones: the order is visible, and it is kept.
 * BGR24: the pixel's three channels are blended.  NV12: luma is blended per pixel with the colour's Y; the chroma sample is blended by
 *   the same procedure run once at the block centre, with the colour's Cb and Cr.  Colours go R, G, B -> Y, Cb, Cr once, on the host,
 *   by the forward colour rule stated under dc_draw_people.
 * Untouched bytes: a byte is written only if a blend was executed for it; pitch padding is never written; a call whose style cannot
 *   blend anything (alpha = 0) launches nothing and writes nothing.
 *
 * dc_draw_heatmap: stand-alone like dc_dedupe_people — `map` is float32 NCHW [nb][C][Hm][Wm] in host (map_is_device = 0) or device
 *   memory.  The call returns when the blending is complete: on `stream`, or on the library's utility stream when it is NULL; host
 *   frames are staged up without their padding and copied back with 2-D copies.
 * dc_net_draw_heatmap: `prob` of the net's last forward, read where it is in the net's element type (float32, float16, bfloat16; the
 *   channel views of merged heads included), on the net's stream behind the forward.  DC_EINVAL when the forward's batch is not nb;
 *   what reading `prob` itself refuses (no forward yet: DC_EINVAL; `prob` left out of the plan: DC_EUNSUP) is passed on.
 * dc_group_draw_heatmap(_mirrored): `prob` alone fused exactly as dc_group_detect_parts(_mirrored) fuses it, drawn at scales[base]
 *   (which must lie in the geometry's range); geometry->scale is not read.  The mirrored form costs no kernel of its own: the fused map
 *   is already un-mirrored.
 * Errors, before any device work: DC_EINVAL naming the field for what dc_draw_people refuses of nb, height, width and the frames; C
 *   outside [1, 32], Hm or Wm outside [1, 65536]; a NULL map, geometry or style; scale, origin_x, origin_y outside the ranges above or
 *   not finite; n_joints outside [1, 32], NULL joints, joints[k] outside [0, C); an unknown mode or alpha_mode; alpha outside [0, 256];
 *   min_score not finite or outside [0, 1]; DC_HEAT_MAX with a NULL lut; DC_HEAT_BY_JOINT with a NULL palette or n_palette outside
 *   [1, 256].  Then DC_ENOCPU in CPU mode (there is no CPU path).
 * Not built, on purpose: the box entry's per-box geometry (one geometry per call); an entry on VideoPipeline / dc_net_track_frames_async
 *   (the net's maps belong to a later frame by the time a result is handed back); the loc_pred / next_pred vector fields; anti-aliasing
 *   or float blending (either would end byte equality).                                                                          */
#define DC_HEAT_MAX         0
#define DC_HEAT_BY_JOINT    1
#define DC_HEAT_ALPHA_CONST 0
#define DC_HEAT_ALPHA_SCORE 1
typedef struct dc_heat_geometry {
  double scale;                 /* frame pixels x scale = network pixels; [1/64, 8] */
  double origin_x, origin_y;    /* frame pixels, |.| <= 32768; 0 = the map's image is the frame */
} dc_heat_geometry;
typedef struct dc_heat_style {
  int n_joints; const int* joints;          /* the channels drawn, in order; 1..32 entries in [0, C), repeats allowed */
  int mode;                                 /* DC_HEAT_MAX, DC_HEAT_BY_JOINT */
  int alpha, alpha_mode;                    /* 0..256; DC_HEAT_ALPHA_CONST, DC_HEAT_ALPHA_SCORE */
  double min_score;                         /* finite, 0..1 */
  const unsigned char* lut;                 /* [256][3] R, G, B: DC_HEAT_MAX */
  const unsigned char* palette; int n_palette;  /* [n_palette][3] R, G, B, 1..256: DC_HEAT_BY_JOINT */
} dc_heat_style;
int dc_draw_heatmap(const dc_frame* frames, int nb, int height, int width, int is_device, const float* map, int map_is_device, int C,
                    int Hm, int Wm, const dc_heat_geometry* geometry, const dc_heat_style* style, void* stream);
int dc_net_draw_heatmap(dc_net* net, const dc_frame* frames, int nb, int height, int width, int is_device,
                        const dc_heat_geometry* geometry, const dc_heat_style* style);
int dc_group_draw_heatmap(dc_group* group, const dc_frame* frames, int nb, int height, int width, int is_device, const double* scales,
                          int base, double origin_x, double origin_y, const dc_heat_style* style);
int dc_group_draw_heatmap_mirrored(dc_group* group, const dc_frame* frames, int nb, int height, int width, int is_device,
                                   const double* scales, int base, const dc_fuse_mirror* fm, double origin_x, double origin_y,
                                   const dc_heat_style* style);

/* ---- redacting people in video frames: a mosaic or a solid colour over heads or bodies of BGR24 or NV12 frames, on the device ------
 * PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind.  THE RULE below is this project's own, like the drawing rule above.
 * It is integer only, so every path gives the same bytes (tests/redact_ref.py restates it in numpy; the device is held to that byte for
 * byte, pitch padding included).
 *
 * Input: frames, people[nb][P][J][3] and n_people[nb] as dc_draw_people takes them; select[nb][P] (may be NULL: everyone): person p of
 *   frame b takes part when p < n_people[b] and select[b][p] is non-zero; a style.  Output: redacted[nb][P] (may be NULL), all of it
 *   written: 1 where at least one region primitive was made for the person, 0 otherwise (not selected, beyond n_people[b], or no
 *   primitive: a person whose neck is below the threshold gets no head region, and the caller must be able to see that).  A primitive
 *   is made from the joints alone, whether or not it reaches into the frame; one whose radius comes out 0 is not made.
 * Which joints are held: as in drawing — x, y and score all finite and score > min_score.  Held coordinates are snapped exactly as
 *   dc_draw_people snaps them: clamped to [-32768, 32768] pixels, then q = (int)rint(16 v).  clamp(v, lo, hi) below is min(max(v, lo), hi),
 *   taken in double before the conversion to int.
 * Regions, by style->region.  The head pair (head_a, head_b) names two joints (the neck, the head top) and is checked for every region.
 *   The head disc, when both joints of the pair are held: with d = b - a in snapped units and L = d.d in int64 (at most 2^41, exact in
 *     double), the disc centred at ((ax + bx) >> 1, (ay + by) >> 1) (arithmetic shift) of radius
 *     r16 = clamp(rint(head_scale * sqrt((double)L)), rint(16 min_radius), rint(16 max_radius)), 0 <= min_radius <= max_radius <= 1024
 *     pixels: one correctly rounded square root, one double multiply and one rint, ties to even.  The disc test w.w <= r16^2 of the
 *     drawing rule stays below 2^43 in int64 for such radii (|w| components below 2^21, r16 <= 2^14, so r16^2 <= 2^28).
 *   The body primitives: every limb of style->edges whose two joints are held, as a capsule; every held joint, as a disc; coverage by
 *     the drawing rule's capsule and disc tests.  Their radius is rb16 = clamp(rint(body_scale * s16), rint(16 min_radius), 1024), s16
 *     (an int) the larger side of the bounding box of the person's held joints in snapped units (0 for a single joint: the radius is
 *     then min_radius).  The cap of 1024 units = 64 pixels — the drawing rule's largest radius, and it wins over min_radius — keeps the
 *     capsule test's int64 proof as it stands there (r16^2 L <= 2^61).
 *   DC_REDACT_HEAD: the head disc.  DC_REDACT_BODY: the head disc and the body primitives.  DC_REDACT_HEAD_OR_BODY: the head disc when
 *     the pair is held, else the body primitives.
 * Blocks: block B in {2, 4, 8, 16, 32} — even, so an NV12 chroma sample lies in exactly one block; a divisor of the kernel's 32 x 32
 *   tile, so a block lies in exactly one tile.  The grid is anchored at pixel (0, 0) of the frame; blocks at the right and bottom edge
 *   may be partial.  A block is selected when the centre (16 px + 8, 16 py + 8) of any of its in-frame pixels is covered by any
 *   primitive of that frame.  Selection is a set: the result does not depend on the order of people or primitives.
 * Effect on a selected block, n the number of its in-frame pixels, sums over the bytes the call found:
 *   DC_REDACT_MOSAIC, BGR24: each channel of every in-frame pixel becomes (sum + n / 2) / n of that channel over the block (integer
 *     division).  NV12: the same on luma; every chroma sample (cx, cy) with pixel (2 cx, 2 cy) in the block becomes the block's mean Cb
 *     and Cr, (sum + m / 2) / m over those m samples.  The largest sum is 1024 * 255.
 *   DC_REDACT_FILL: every in-frame pixel, and every such chroma sample, becomes `fill` (R, G, B), converted once by the forward colour
 *     rule stated under dc_draw_people.
 * Untouched bytes: bytes outside selected blocks, pitch padding included, are never stored.  A call that makes no primitive that
 *   reaches the frame launches nothing and writes nothing; a host frame nothing is redacted in does not travel.  A MOSAIC call
 *   repeated on its own output changes no byte (a block of equal bytes v has the mean (n v + n / 2) / n = v).
 *
 * dc_redact_people: stand-alone like dc_draw_people — no net, people as host arrays, frames in host (is_device = 0) or device memory,
 *   the work on the device either way; the limits of nb, height, width, P, J and n_edges are dc_draw_people's.  The call returns when
 *   the redaction is complete: on `stream`, or on the library's utility stream when it is NULL; host frames are staged up without their
 *   padding and copied back with 2-D copies.  One launch: only tiles some primitive's bounding box touches (one workgroup each).
 * Errors, before any device work: DC_EINVAL naming the field for everything dc_draw_people refuses of frames, nb, height, width, P, J,
 *   n_people and edges; a NULL style; an unknown region or effect; block not in the list; head_a or head_b outside [0, J), or equal;
 *   head_scale or body_scale not finite or < 0; min_radius or max_radius not finite, min_radius < 0, max_radius > 1024 or
 *   min_radius > max_radius; min_score not finite or < 0.  Then DC_ENOCPU in CPU mode (there is no CPU path).
 * Not built, on purpose: blur; per-box geometry (the asynchronous entry is dc_net_track_frames_async_overlay, below).  A mosaic with
 *   small blocks is NOT a privacy guarantee (the means still carry the face), and DC_REDACT_HEAD does not redact a person without a
 *   held head pair: that is what `redacted` is for.                                                                              */
#define DC_REDACT_HEAD         0
#define DC_REDACT_BODY         1
#define DC_REDACT_HEAD_OR_BODY 2
#define DC_REDACT_MOSAIC       0
#define DC_REDACT_FILL         1
typedef struct dc_redact_style {
  int region, head_a, head_b;               /* DC_REDACT_HEAD, _BODY, _HEAD_OR_BODY; the head pair: two different joints in [0, J) */
  double head_scale, body_scale, min_radius, max_radius, min_score; /* scales finite, >= 0; radii in pixels, 0 <= min <= max <= 1024 */
  int n_edges; const int* edges;            /* [n_edges][2] 0-based joints, 0..128: the limbs of the body region */
  int effect, block;                        /* DC_REDACT_MOSAIC, DC_REDACT_FILL; 2, 4, 8, 16 or 32 */
  unsigned char fill[3];                    /* R, G, B: DC_REDACT_FILL */
} dc_redact_style;
int dc_redact_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                     const double* people, const unsigned char* select /* [nb][P], may be NULL: everyone */,
                     const dc_redact_style* style, int* redacted /* [nb][P], may be NULL */, void* stream);

/* ---- overlays from people in device memory: redaction and skeletons without a round trip through the host ------------------
 * PARITY UNPINNED BY THE REFERENCE.  There is NO rule of its own here.  THE RULE'S PLACE: both entries below write the bytes of
 * dc_redact_people then dc_draw_people on the people this call returns (dc_net_track_frames_async_overlay) or is given
 * (dc_overlay_people_device) — redaction first, the skeletons over the mosaic —, byte for byte, with `redacted` as dc_redact_people
 * reports it.  What differs is where the work is done: the primitives (snapping, order, radii, colour keys) and the per-tile selection
 * are made on the device from n_people, people, cand and ids in device memory, so the host reads no pose, takes no second upload of the
 * pixels and waits for nothing.  Every tile of every frame is a workgroup; one that no primitive reaches loads and stores no pixel.
 *
 * Styles: `draw` and `redact` may each be NULL (not both).  The redaction chooses people by id instead of by mask — a mask cannot exist
 *   before the people do —: only_ids[n_only] (n_only < 0: no list; 0: nobody) keeps only the people with one of these ids, keep_ids
 *   [n_keep] (n_keep < 0: no list) leaves the people with one of these ids visible; both are combined by AND, as the Python binding's
 *   redact_select combines them; at most 256 ids each; they need ids (and a redact style).  The drawing takes cand and ids as
 *   dc_draw_people does.
 *
 * dc_overlay_people_device: the device half alone.  frames as dc_draw_people takes them (device frames are written in place; host frames
 *   are staged up without their padding, written, and ALL copied back with 2-D copies, padding never written: which frames are touched
 *   is known on the device only).  n_people [nb], people [nb][P][J][3], cand [nb][P][J] (may be NULL), ids [nb][P] (may be NULL) and
 *   redacted [nb][P] (may be NULL; written by the redaction only) are DEVICE pointers; an n_people[b] outside [0, P] is read as clamped.
 *   With device frames and a `stream` the call is asynchronous on that stream: it returns once everything is enqueued, and the next call
 *   on the same stream may follow at once.  Otherwise (host frames, or stream NULL: the library's utility stream) it waits.
 * dc_net_track_frames_async_overlay: dc_net_track_frames_async with the overlays enqueued on the net's stream behind the tracker's
 *   launch, from the people it hands back — the kept people after completion and dedupe, or with smoothing on the tracker's smoothed
 *   poses and their cand (bridged joints at alpha_filled; cand NULL: alpha everywhere) — and the tracker's ids (no tracker: the person's
 *   index chooses the colour, and id lists are refused).  Device frames and device `images` are written in place.  Host frames and host
 *   `images` are written in the device copy the pre-processing staged — no second upload — and then EVERY one of them is copied back
 *   into the caller's planes (2-D copies into the caller's pitch, padding never written): nobody knows at enqueue time which frames are
 *   touched.  They must be writable, and stay the caller's only after the net was synchronised; pinned host planes keep the call free
 *   of host waits.  redacted [n][max_people] (host, may be NULL) comes back with the other results.  With both styles NULL the call
 *   enqueues exactly what dc_net_track_frames_async enqueues.
 * Errors, before any device work and worded like the synchronous entries': everything dc_draw_people / dc_redact_people refuse of nb,
 *   height, width, the frames, P, J and the styles; both styles NULL; an id list of more than 256 ids, one without ids or without a
 *   redact style; for the chain what dc_net_track_frames_async refuses.  Then DC_ENOCPU in CPU mode.
 * Not built, on purpose: heat-map overlays in the chain (the net's maps belong to a later frame by the time a result is handed back);
 *   a `select` mask.                                                                                                              */
int dc_overlay_people_device(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J,
                             const int* n_people /* device */, const double* people /* device */, const int* cand /* device, may be NULL */,
                             const long long* ids /* device, may be NULL */, const dc_draw_style* draw /* may be NULL */,
                             const dc_redact_style* redact /* may be NULL */, const long long* only_ids, int n_only /* < 0: no list */,
                             const long long* keep_ids, int n_keep /* < 0: no list */, int* redacted /* device [nb][P], may be NULL */,
                             void* stream);
int dc_net_track_frames_async_overlay(dc_net* net, dc_tracker* tracker /* NULL: people without ids */, const dc_frame* frames /* or NULL */,
                                      const unsigned char* images /* or NULL */, int n, int height, int width, double scale, int is_device,
                                      const int* slot_of, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean,
                                      const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, long long* ids,
                                      int* place, const dc_draw_style* draw /* may be NULL */, const dc_redact_style* redact /* may be NULL */,
                                      const long long* only_ids, int n_only /* < 0: no list */, const long long* keep_ids,
                                      int n_keep /* < 0: no list */, int* redacted /* host [n][max_people], may be NULL */);

/* ---- labelling people in video frames: a person's id as text on a plate, in BGR24 or NV12 frames in place, on the device ----
 * PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing.  THE RULE below is this project's own and
 * integer only, so every path gives the same bytes (tests/label_ref.py restates it in numpy; the device is held to that byte for byte).
 * No anti-aliasing: it would end byte equality.  All values below are C ints unless said otherwise; / and % act on non-negative
 * values; >> is arithmetic.
 *
 * Font: built in, the project's own data (csrc/label_font.h), a PLACEHOLDER like the palettes.  A glyph is 5 columns x 7 rows, one
 *   byte per row, bit 4 the leftmost column; the advance is 6 columns.  The set is 0-9, A-Z, space and # - . : / % + _ ? — 46 glyphs.
 *   Lower-case letters fold to upper-case; every other byte is refused, never substituted.  dc_label_font hands out a glyph's rows.
 * Text: the key of person p of frame b is ids[b][p], or p when ids is NULL (the drawing rule's key).  The made text is `prefix` (0 to 4
 *   characters of the set) followed by the key in decimal: at most 4 + 19 = 23 characters (DC_LABEL_MAX_CHARS is 24, the NUL
 *   included).  A key < 0 — an untracked person — makes no text.  texts[nb][P][24] (synchronous entry only, may be NULL): a row is
 *   NUL-padded; a non-empty row (first byte not NUL) replaces the made text of that person, whatever the key; an empty row falls back
 *   to the made text.  A person without a text gets no label.  Rows of people p >= n_people[b] are not read.
 * Held joints, as in drawing: x, y and score all finite and score > min_score; snapped by the drawing rule's clamp and q = rint(16 v).
 *   A person with no held joint gets no label.
 * Geometry, with n the number of characters (1..23) and s = scale (1..8):
 *   tw = s (6 n - 1), th = 7 s; the plate: pw = tw + 2 s, ph = th + 2 s.
 *   anchor_joint in [0, J) and that joint held:  X = (qx >> 4) - (pw >> 1), Yb = qy >> 4.
 *   otherwise (anchor_joint = -1, or the joint not held): the upper left of the bounding box of the held joints,
 *     X = lo_x >> 4, Yb = lo_y >> 4 (lo_x, lo_y: the least snapped qx, qy over the held joints).
 *   Y = Yb - gap - ph, gap in [0, 64] pixels.
 *   X = min(max(X, 0), max(0, W - pw)), Y = min(max(Y, 0), max(0, H - ph)): a label is pulled into the frame where it fits, and cut
 *   at the right / bottom edge where it does not (then X = 0 / Y = 0).
 * Layers, per label, in this order:
 *   plate: the pixels X <= px < X + pw, Y <= py < Y + ph, blended with alpha_plate.  Not made when alpha_plate = 0.
 *   text:  u = px - X - s, v = py - Y - s; a pixel can be covered when 0 <= u < tw and 0 <= v < th; with k = u / s, i = k / 6, c = k % 6,
 *     r = v / s it IS covered when c < 5 and bit (4 - c) of row r of the glyph of text[i] is set.  Blended with alpha_text.  Not made
 *     when alpha_text = 0.
 *   With both alphas 0 no label is made at all.  Only pixels inside the frame are covered.
 * Order: frames in order; people in index order; later labels go over earlier ones.  Labels go over everything else: where entries
 *   combine overlays the order is redaction, then skeletons, then labels.
 * Blend: the drawing rule's out = (c A + dst (256 - A) + 128) >> 8 per covered pixel and channel.  BGR24: three channels.  NV12: luma
 *   per pixel; a chroma sample is blended ONCE PER LAYER with Ac = (A k + n / 2) / n for k > 0 of the block's n in-frame pixels
 *   covered by that layer — what the drawing rule does per primitive, a layer standing for a primitive.
 * Colour: DC_LABEL_PLATE_BY_PERSON: the plate is palette[key % n_palette], the text text_color.  DC_LABEL_TEXT_BY_PERSON: the text is
 *   palette[key % n_palette], the plate plate_color.  key is the person's key also when a `texts` row replaces the made text; for a
 *   key < 0 (possible only with such a row) the palette entry is palette[0].  Colours go R, G, B -> frame bytes once per label by the
 *   drawing rule's forward conversion.
 * Untouched bytes: bytes no made layer covers are never stored, pitch padding included.  A call that makes no label launches nothing
 *   and writes nothing; a host frame nothing is labelled in does not travel.
 *
 * dc_label_people: stand-alone like dc_draw_people — no net, people as host arrays, frames in host or device memory with the same
 *   limits on nb, height, width, P and J; one launch over the non-empty tiles; the call returns when the frames are written.
 * Errors, before any device work: DC_EINVAL naming the field and the index for everything dc_draw_people refuses of the frames, nb,
 *   height, width, P, J and n_people; a NULL style or palette; scale outside [1, 8], gap outside [0, 64], anchor_joint outside
 *   [-1, J), alpha_text or alpha_plate outside [0, 256], min_score not finite or < 0, an unknown color_mode, n_palette outside
 *   [1, 256]; a prefix without a NUL in its first 5 bytes; a byte outside the set in prefix or in a texts row, naming b, p and the byte;
 *   a texts row without a NUL in its 24 bytes.  Then DC_ENOCPU in CPU mode.
 * dc_label_font: rows[0 .. 7) of the glyph of byte ch (lower case folded), or DC_EINVAL for a byte outside the set.
 *
 * On the device routes (dc_overlay_styles.labels, below) the labels are made from the people, and the ids, in device memory, exactly
 *   as above, and written behind the skeletons.
 * Not built, on purpose: `texts` on the device routes (a text for a person cannot exist before the person does); anti-aliasing; fonts
 *   of other sizes; per-box geometry.                                                                                               */
#define DC_LABEL_MAX_CHARS 24
#define DC_LABEL_PLATE_BY_PERSON 0
#define DC_LABEL_TEXT_BY_PERSON  1
typedef struct dc_label_style {
  int scale, gap, anchor_joint;             /* 1..8; 0..64 px; -1 or [0, J) */
  int alpha_text, alpha_plate;              /* 0..256 */
  double min_score;                         /* finite, >= 0 */
  int color_mode; const unsigned char* palette; int n_palette;   /* [n_palette][3] R, G, B; 1..256 */
  unsigned char text_color[3], plate_color[3];
  char prefix[8];                           /* NUL-terminated, at most 4 characters of the set */
} dc_label_style;
int dc_label_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                    const double* people, const long long* ids /* may be NULL */, const char* texts /* [nb][P][24], may be NULL */,
                    const dc_label_style* style, void* stream);
int dc_label_font(int ch, unsigned char rows[7]);   /* 0, or DC_EINVAL for a byte outside the set */

/* ---- one styles block for the two device entries, so that a further overlay needs no further pair of entries -----------------
 * dc_overlay_people_device_styles / dc_net_track_frames_async_styles are dc_overlay_people_device / dc_net_track_frames_async_overlay
 * with the styles and the id lists in one struct; the older two are wrappers over them and keep every behaviour and refusal.  `size`
 * is sizeof(dc_overlay_styles) as the CALLER compiled it: fields beyond it read as NULL / no list, so an older caller keeps working
 * with a newer library.  A size below that of the first field group (size, draw, redact) or above the library's struct is DC_EINVAL.
 * labels: the label overlay (dc_label_people's rule, without `texts`), written behind the redaction and the skeletons; the key is
 * the tracker's id (the person's index without ids).  dc_overlay_people_device_styles refuses a call with all three styles NULL (a
 * NULL `styles` included); the chain entry then enqueues what dc_net_track_frames_async enqueues.  With `labels` NULL the two
 * entries enqueue exactly what the older ones enqueue.                                                                              */
typedef struct dc_overlay_styles {
  size_t size;                              /* sizeof(dc_overlay_styles) of the caller: fields beyond it read as NULL / no list */
  const dc_draw_style* draw; const dc_redact_style* redact; const dc_label_style* labels;   /* each may be NULL */
  const long long* only_ids; int n_only; const long long* keep_ids; int n_keep;             /* < 0: no list */
} dc_overlay_styles;
int dc_overlay_people_device_styles(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J,
                                    const int* n_people /* device */, const double* people /* device */,
                                    const int* cand /* device, may be NULL */, const long long* ids /* device, may be NULL */,
                                    const dc_overlay_styles* styles, int* redacted /* device [nb][P], may be NULL */, void* stream);
int dc_net_track_frames_async_styles(dc_net* net, dc_tracker* tracker /* NULL: people without ids */, const dc_frame* frames /* or NULL */,
                                     const unsigned char* images /* or NULL */, int n, int height, int width, double scale, int is_device,
                                     const int* slot_of, const dc_assemble_params* p, int n_edges, const int* edges, const double* mean,
                                     const double* stdev, const int* joint_order, int* n_people, double* people, int* cand, long long* ids,
                                     int* place, const dc_overlay_styles* styles, int* redacted /* host [n][max_people], may be NULL */);

/* ---- appearance descriptors: what a person looks like, counted from a BGR24 or NV12 frame on the device ------------------------------
 * PARITY UNPINNED BY THE REFERENCE, which stops at the maps.  THE RULE below is this project's own, like the redaction rule it borrows
 * from.  It is integer only, so every path gives the same counts (tests/appear_ref.py restates it in numpy; the device is held to that
 * exactly, and to leaving every frame byte, pitch padding included, as it was).
 *
 * Input: frames, people[nb][P][J][3] and n_people[nb] as dc_redact_people takes them; a style.  Output: desc[nb][P][3][16] (host ints),
 *   ALL of it written: zeros for p >= n_people[b], for a person with no primitive, and for a region that lies outside the frame.
 * Which joints are held, and how they are snapped: exactly as in dc_redact_people — x, y and score finite and score > min_score; clamped
 *   to [-32768, 32768] pixels, then q = (int)rint(16 v).
 * The region of person p: a capsule for every limb of style->edges whose two joints are held (the torso's sides, say); there are no
 *   joint discs.  The radius is the redaction's body radius, r16 = clamp(rint(scale * s16), rint(16 min_radius), 1024), s16 (an int) the
 *   larger side of the bounding box of the person's held joints in snapped units; a radius of 0 makes no primitive.  0 <= min_radius <= 64
 *   pixels, so the cap of 1024 units never meets a larger lower bound.
 * Region pixels: an in-frame pixel (x, y) belongs to the region when its centre (16 x + 8, 16 y + 8) is covered, by the drawing rule's
 *   capsule test in int64, by ANY of that person's capsules.  A pixel counts once per person however many of the person's capsules cover
 *   it, and once for each of several people whose regions overlap.
 * Per region pixel, three bytes c0, c1, c2 — BGR24: B, G, R; NV12: Y(x, y), and Cb, Cr of the sample (x >> 1, y >> 1) — and
 *   desc[b][p][c][v >> 4] += 1 for each.  So each channel's 16 counts sum to the region's pixel count n (at most 2^28: the frame's).
 *   The result is a sum of integers: it does not depend on the order of people, primitives or tiles.
 * Frames are read-only here: no frame byte is stored, host frames are staged up (only those a primitive reaches) and nothing is copied
 *   back but desc.  A call whose regions reach no frame launches nothing.
 *
 * dc_describe_people: stand-alone like dc_redact_people — no net, people as host arrays, frames in host (is_device = 0) or device
 *   memory, the counting on the device either way; the limits of nb, height, width, P, J and n_edges are dc_draw_people's.  The call
 *   returns when desc is complete: on `stream`, or on the library's utility stream when it is NULL.  One launch: only tiles some
 *   capsule's bounding box touches (one workgroup each), desc zeroed on the same stream in front of it.  style->size is
 *   sizeof(dc_appearance_style) as the CALLER compiled it, as dc_overlay_styles.size.
 * Errors, before any device work: DC_EINVAL naming the field for everything dc_redact_people refuses of frames, nb, height, width, P, J,
 *   n_people and edges; a NULL style, or a size smaller than the struct's first version (through min_score); scale not finite or < 0;
 *   min_radius outside [0, 64]; min_score not finite or < 0.  Then DC_ENOCPU in CPU mode (there is no CPU path).
 * Not built, on purpose: descriptors inside the asynchronous video chain, learned embeddings, per-box geometry.  The tracker's use of
 *   the descriptor is dc_tracker_update_appearance, above.  The descriptor is a coarse colour histogram: it tells a red coat from a blue one, not two people in grey.            */
#define DC_APPEARANCE_BINS 16
typedef struct dc_appearance_style {
  size_t size;                              /* sizeof(dc_appearance_style) of the caller */
  int n_edges; const int* edges;            /* [n_edges][2] 0-based joints, 0..128: the limbs sampled (the torso) */
  double scale, min_radius, min_score;      /* scale finite, >= 0; min_radius in pixels, 0..64; min_score finite, >= 0 */
} dc_appearance_style;
int dc_describe_people(const dc_frame* frames, int nb, int height, int width, int is_device, int P, int J, const int* n_people,
                       const double* people, const dc_appearance_style* style, int* desc /* host [nb][P][3][16] */, void* stream);

/* ---- in-process multi-GPU forward (SURVEY 8(b)'s dc_forward_batch) -------------------------------------------------------
 * A communicator over `nexec` executors: executor k runs on devices[k] (NULL: k modulo the visible devices) on a host thread of its
 * own (mode and device are per thread, src/caffe/common.cpp:13-20).  transport: how the maps travel to the root executor's device —
 * DC_COMM_RCCL: one grouped ncclRecv x (n-1) / ncclSend exchange (librccl.so is opened with dlopen at the first use; needs one
 * executor per device); DC_COMM_PEER: hipMemcpyPeerAsync (device-to-device copies when executors share a device: the loop-back
 * transport of the 1-GPU tests); DC_COMM_AUTO: RCCL when it loads, the devices are distinct AND the communicators it makes move a
 * byte from every peer to the root at creation (dc_comm_create probes them), else PEER; an explicit DC_COMM_RCCL reports the failure
 * instead.  ENVIRONMENT: on hosts whose driver offers dmabuf IPC only (the MI355X boxes this was built on), RCCL's peer buffers need
 * HSA_ENABLE_IPC_MODE_LEGACY=0 in the process environment BEFORE the HIP runtime is loaded — without it ncclCommInitAll / the first
 * exchange fail with `hipIpcGetMemHandle: invalid argument`.  The library does not change the environment of its host process.
 * The calling thread's current HIP device is the same after dc_comm_create / dc_forward_batch as before.
 * dc_forward_batch: `n` host images (inputs[i]: 3 x hw[i][0] x hw[i][1] float32 NCHW, shapes may differ) are dealt to the executors
 * longest-processing-time-first over H*W, every executor forwards the same-shape images of its share on nets[k], a group of 8 (float16:
 * 16) or more images as two sub-batches, so that staging, forward and the way back of consecutive (sub-)batches overlap (round 6) —
 * nets[k] must live on devices[k]: replicas created under dc_set_device(k), or clones where executors share a device —, the maps are
 * gathered on the root's device (dc_comm_root_maps: NCHW float32 device pointers of image i, dims = {prob, loc_pred, next_pred
 * channels, map height, map width}, valid until the next call) and copied to prob[i] / loc_pred[i] / next_pred[i] (host; arrays or
 * entries may be NULL).  Synchronous.  The reference has no inference-time multi-GPU path (its P2PSync, src/caffe/parallel.cpp:287-322,
 * sums gradients along a tree); the consumer this serves is a tools/caffe.cpp-style C++ program (tools/caffe.cpp:302-388).   */
#define DC_COMM_AUTO 0
#define DC_COMM_RCCL 1
#define DC_COMM_PEER 2
typedef struct dc_comm dc_comm;
int dc_comm_create(int nexec, const int* devices, int transport, dc_comm** out);
int dc_comm_destroy(dc_comm* comm);
int dc_comm_transport(dc_comm* comm); /* DC_COMM_RCCL or DC_COMM_PEER (negative: error) */
int dc_forward_batch(dc_comm* comm, dc_net* const* nets, int nexec, const float* const* inputs, const int (*hw)[2], int n,
                     float* const* prob, float* const* loc_pred, float* const* next_pred);
int dc_comm_item_executor(dc_comm* comm, int i); /* which executor forwarded image i of the last call (negative: error) */
int dc_comm_root_maps(dc_comm* comm, int i, const void** prob, const void** loc_pred, const void** next_pred, int dims[5]);
/* the schedule alone (host only): exec_of_item[i] = executor of item i for `n` items of the given costs on `nexec` executors */
int dc_lpt_schedule(const double* cost, int n, int nexec, int* exec_of_item);

#ifdef __cplusplus
}
#endif
#endif /* DEEPCUT_HIP_H_ */
