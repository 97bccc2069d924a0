"""ctypes binding of libdeepcut_hip.so with the reference's pycaffe names and semantics
(python/caffe/pycaffe.py:22-108, python/caffe/_caffe.cpp:76-96,159-193,219-277)."""
import contextlib
import ctypes as C
import os
import sys
from collections import OrderedDict

import numpy as np

TRAIN = 0  # caffe.proto:253-256
TEST = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_CANDIDATES = [
    os.environ.get("DEEPCUT_HIP_LIB", ""),
    os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libdeepcut_hip.so")),
]


class DeepcutError(RuntimeError):
    """Raised for every failure the reference would LOG(FATAL)/CHECK-abort on, and for I/O errors
    (the reference raises RuntimeError('Could not open file ...'), _caffe.cpp:45-52)."""

    def __init__(self, code, msg):
        RuntimeError.__init__(self, msg)
        self.code = code


def lib_path():
    for p in _LIB_CANDIDATES:
        if p and os.path.exists(p):
            return p
    raise ImportError(
        "libdeepcut_hip.so not found (looked in %s). Build it with `python deepcut-cnn_amd/build.py`; "
        "there is no Python/CPU fallback for the forward path." % [p for p in _LIB_CANDIDATES if p])


class AssembleParams(C.Structure):
    """dc_assemble_params (include/deepcut_hip.h)."""
    _fields_ = [("scale", C.c_double), ("threshold", C.c_float), ("radius", C.c_int), ("max_det", C.c_int), ("max_cost", C.c_double),
                ("seed_threshold", C.c_float), ("max_people", C.c_int), ("min_joints", C.c_int)]


class CompleteParams(C.Structure):
    """dc_complete_params (include/deepcut_hip.h)."""
    _fields_ = [("enabled", C.c_int), ("fill_threshold", C.c_float), ("fill_radius", C.c_int), ("min_support", C.c_int)]


class DedupeParams(C.Structure):
    """dc_dedupe_params (include/deepcut_hip.h)."""
    _fields_ = [("enabled", C.c_int), ("max_dist", C.c_double), ("min_common", C.c_int), ("min_size", C.c_double), ("sigma", C.c_void_p),
                ("n_sigma", C.c_int), ("absorb", C.c_int)]


class FuseMirror(C.Structure):
    """dc_fuse_mirror (include/deepcut_hip.h)."""
    _fields_ = [("mirror", C.c_void_p), ("image_width", C.c_int), ("joint_mirror", C.c_void_p), ("n_edges", C.c_int), ("edges", C.c_void_p)]


class TrackerParams(C.Structure):
    """dc_tracker_params (include/deepcut_hip.h)."""
    _fields_ = [("slots", C.c_int), ("max_tracks", C.c_int), ("n_joints", C.c_int), ("sigma", C.c_void_p), ("max_misses", C.c_int),
                ("min_common", C.c_int), ("max_dist", C.c_double), ("min_size", C.c_double), ("motion", C.c_int)]


class TrackSmoothParams(C.Structure):
    """dc_track_smooth_params (include/deepcut_hip.h)."""
    _fields_ = [("enabled", C.c_int), ("min_cutoff", C.c_double), ("beta", C.c_double), ("d_cutoff", C.c_double), ("max_hold", C.c_int)]


class TrackAppearanceParams(C.Structure):
    """dc_track_appearance_params (include/deepcut_hip.h)."""
    _fields_ = [("enabled", C.c_int), ("min_pixels", C.c_int), ("alpha256", C.c_int), ("reid_max", C.c_int), ("max_age", C.c_int),
                ("min_hits", C.c_int)]


# Step 8 of the tracker's rule (`Tracker.smoothing`).  PLACEHOLDERS, NOT TUNED ON REAL VIDEO: override them.  Time counts in updates: a
# 1 Hz cutoff on 30 fps video is min_cutoff = 1 / 30.
SMOOTH_DEFAULTS = {"min_cutoff": 0.1, "beta": 4.0, "d_cutoff": 0.03, "max_hold": 3}


class DcFrame(C.Structure):
    """dc_frame (include/deepcut_hip.h)."""
    _fields_ = [("plane", C.c_void_p * 2), ("pitch", C.c_int * 2), ("format", C.c_int), ("matrix", C.c_int), ("range", C.c_int)]


class DrawStyle(C.Structure):
    """dc_draw_style (include/deepcut_hip.h)."""
    _fields_ = [("n_edges", C.c_int), ("edges", C.c_void_p), ("joint_radius", C.c_double), ("limb_radius", C.c_double), ("alpha", C.c_int),
                ("alpha_filled", C.c_int), ("min_score", C.c_double), ("color_mode", C.c_int), ("palette", C.c_void_p), ("n_palette", C.c_int),
                ("untracked", C.c_ubyte * 3)]


class RedactStyle(C.Structure):
    """dc_redact_style (include/deepcut_hip.h)."""
    _fields_ = [("region", C.c_int), ("head_a", C.c_int), ("head_b", C.c_int), ("head_scale", C.c_double), ("body_scale", C.c_double),
                ("min_radius", C.c_double), ("max_radius", C.c_double), ("min_score", C.c_double), ("n_edges", C.c_int), ("edges", C.c_void_p),
                ("effect", C.c_int), ("block", C.c_int), ("fill", C.c_ubyte * 3)]


class AppearanceStyle(C.Structure):
    """dc_appearance_style (include/deepcut_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("n_edges", C.c_int), ("edges", C.c_void_p), ("scale", C.c_double), ("min_radius", C.c_double),
                ("min_score", C.c_double)]


class LabelStyle(C.Structure):
    """dc_label_style (include/deepcut_hip.h)."""
    _fields_ = [("scale", C.c_int), ("gap", C.c_int), ("anchor_joint", C.c_int), ("alpha_text", C.c_int), ("alpha_plate", C.c_int),
                ("min_score", C.c_double), ("color_mode", C.c_int), ("palette", C.c_void_p), ("n_palette", C.c_int),
                ("text_color", C.c_ubyte * 3), ("plate_color", C.c_ubyte * 3), ("prefix", C.c_char * 8)]


class OverlayStyles(C.Structure):
    """dc_overlay_styles (include/deepcut_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("draw", C.POINTER(DrawStyle)), ("redact", C.POINTER(RedactStyle)), ("labels", C.POINTER(LabelStyle)),
                ("only_ids", C.c_void_p), ("n_only", C.c_int), ("keep_ids", C.c_void_p), ("n_keep", C.c_int)]


class HeatGeometry(C.Structure):
    """dc_heat_geometry (include/deepcut_hip.h)."""
    _fields_ = [("scale", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double)]


class HeatStyle(C.Structure):
    """dc_heat_style (include/deepcut_hip.h)."""
    _fields_ = [("n_joints", C.c_int), ("joints", C.c_void_p), ("mode", C.c_int), ("alpha", C.c_int), ("alpha_mode", C.c_int),
                ("min_score", C.c_double), ("lut", C.c_void_p), ("palette", C.c_void_p), ("n_palette", C.c_int)]


MAX_ASSEMBLE_DET, MAX_ASSEMBLE_PEOPLE = 64, 256  # dc_net_assemble_people's limits
# Stage D of the people assembly (`Net.completion`, the `complete=` arguments).  PLACEHOLDERS, not tuned on real images: override them.
COMPLETE_DEFAULTS = {"fill_threshold": 0.25, "fill_radius": 2, "min_support": 2}
# Stage E of the people assembly (`Net.dedupe`, the `dedupe=` arguments, `dedupe_people`).  PLACEHOLDERS, not tuned on real images:
# override them.  sigma None = 1.0 for every joint.
DEDUPE_DEFAULTS = {"max_dist": 0.05, "min_common": 3, "min_size": 32.0, "sigma": None, "absorb": True}
PIX_BGR24, PIX_NV12 = 0, 1  # DC_PIX_*
_CSC_MATRIX = {"bt601": 0, "bt709": 1}  # DC_CSC_*
_CSC_RANGE = {"limited": 0, "full": 1}  # DC_RANGE_*


def csc_coefficients(matrix="bt601", range="limited"):
    """(ky, rv, bu, gu, gv, y0) of the NV12 conversion rule (include/deepcut_hip.h, dc_frame): computed in double, rounded to nearest."""
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[_CSC_MATRIX[matrix]]
    kg = 1.0 - kr - kb
    full = bool(_CSC_RANGE[range])
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    r = lambda v: int(np.rint(v))  # noqa: E731
    return (r(65536.0 * sy), r(65536.0 * 2.0 * (1.0 - kr) * sc), r(65536.0 * 2.0 * (1.0 - kb) * sc),
            r(65536.0 * (-2.0 * kb * (1.0 - kb) / kg) * sc), r(65536.0 * (-2.0 * kr * (1.0 - kr) / kg) * sc), 0 if full else 16)


class Frame(object):
    """One video frame where a decoder left it (dc_frame): NV12 or BGR planes with a row pitch, host arrays or device addresses.
    Accepted by Net / NetGroup.forward_images and forward_boxes and by pose.estimate_pose / estimate_poses / estimate_people wherever
    they take a uint8 image; the conversion runs on the device where the pre-processing fetches a pixel (the rule: deepcut_hip.h)."""

    def __init__(self, fmt, planes, pitches, height, width, matrix="bt601", range="limited", device=False, keep=()):
        if matrix not in _CSC_MATRIX:
            raise ValueError("matrix must be one of %s, got %r" % (sorted(_CSC_MATRIX), matrix))
        if range not in _CSC_RANGE:
            raise ValueError("range must be one of %s, got %r" % (sorted(_CSC_RANGE), range))
        self.format, self.matrix, self.range = int(fmt), matrix, range
        self.height, self.width = int(height), int(width)
        if self.height <= 0 or self.width <= 0:
            raise ValueError("a frame's height and width must be positive, got %d x %d" % (self.height, self.width))
        self.planes = [int(p or 0) for p in planes]
        self.pitches = [int(p) for p in pitches]
        self.is_device = bool(device)
        self._keep = tuple(keep)  # the host arrays the plane addresses point into

    @property
    def shape(self):
        return (self.height, self.width, 3)

    @staticmethod
    def _plane(a, name, shape):
        """A host plane as it is (no copy: the pitch is the array's own row stride); -> its row pitch in bytes."""
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
            raise ValueError("%s must be a uint8 numpy array" % name)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(a.shape)))
        inner = [int(np.prod(shape[k + 1:])) for k in range(1, len(shape))]
        if [int(v) for v in a.strides[1:]] != inner:
            raise ValueError("%s: the samples of a row must be contiguous (strides %s, expected %s after the row stride)" %
                             (name, tuple(a.strides), tuple(inner)))
        if a.strides[0] < int(np.prod(shape[1:])):
            raise ValueError("%s: row stride %d is below the %d bytes of a row" % (name, a.strides[0], int(np.prod(shape[1:]))))
        return int(a.strides[0])

    @classmethod
    def nv12(cls, y, uv, matrix="bt601", range="limited"):
        """y: uint8 [H, W]; uv: uint8 [(H+1)//2, (W+1)//2, 2] (Cb, Cr).  Row pitches are the arrays' strides[0]."""
        if not isinstance(y, np.ndarray) or y.ndim != 2:
            raise ValueError("y must be a uint8 [H, W] numpy array")
        h, w = y.shape
        py = cls._plane(y, "y", (h, w))
        puv = cls._plane(uv, "uv", ((h + 1) // 2, (w + 1) // 2, 2))
        return cls(PIX_NV12, [y.ctypes.data, uv.ctypes.data], [py, puv], h, w, matrix, range, False, (y, uv))

    @classmethod
    def bgr(cls, array):
        """array: uint8 [H, W, 3] B, G, R with any row stride (a view of a wider surface)."""
        if not isinstance(array, np.ndarray) or array.ndim != 3:
            raise ValueError("array must be a uint8 [H, W, 3] numpy array")
        h, w = array.shape[:2]
        p = cls._plane(array, "array", (h, w, 3))
        return cls(PIX_BGR24, [array.ctypes.data, 0], [p, 0], h, w, keep=(array,))

    @classmethod
    def nv12_device(cls, y_ptr, uv_ptr, height, width, pitch_y, pitch_uv, matrix="bt601", range="limited"):
        """Device planes by address (e.g. tensor.data_ptr()); the memory stays the caller's to keep alive."""
        return cls(PIX_NV12, [y_ptr, uv_ptr], [pitch_y, pitch_uv], height, width, matrix, range, True)

    @classmethod
    def bgr_device(cls, ptr, height, width, pitch):
        return cls(PIX_BGR24, [ptr, 0], [pitch, 0], height, width, device=True)

    def c_frame(self):
        f = DcFrame()
        f.plane[0], f.plane[1] = self.planes[0] or None, self.planes[1] or None
        f.pitch[0], f.pitch[1] = self.pitches
        f.format, f.matrix, f.range = self.format, _CSC_MATRIX[self.matrix], _CSC_RANGE[self.range]
        return f

    def to_bgr(self):
        """-> uint8 [H, W, 3] B, G, R: the conversion rule in numpy (host frames only), for callers who draw the result."""
        if self.is_device:
            raise ValueError("to_bgr() works on host frames only")
        if self.format == PIX_BGR24:
            return np.ascontiguousarray(self._keep[0])
        y, uv = self._keep
        ky, rv, bu, gu, gv, y0 = csc_coefficients(self.matrix, self.range)
        rows, cols = np.arange(self.height) >> 1, np.arange(self.width) >> 1
        c = y.astype(np.int32) - y0
        d = uv[rows][:, cols, 0].astype(np.int32) - 128
        e = uv[rows][:, cols, 1].astype(np.int32) - 128
        lum = ky * c + 32768
        out = np.stack([(lum + bu * d) >> 16, (lum + gu * d + gv * e) >> 16, (lum + rv * e) >> 16], axis=2)
        return np.clip(out, 0, 255).astype(np.uint8)


def _frame_list(images):
    """images -> a list of Frames when it is a Frame or a non-empty list / tuple of Frames, else None (the array paths)."""
    if isinstance(images, Frame):
        return [images]
    if isinstance(images, (list, tuple)) and images and all(isinstance(f, Frame) for f in images):
        return list(images)
    return None


def _frame_array(frames):
    """-> (dc_frame[n], height, width, is_device) of frames of one size that are all host or all device memory."""
    f0 = frames[0]
    for i, f in enumerate(frames):
        if (f.height, f.width) != (f0.height, f0.width):
            raise ValueError("frame %d is %d x %d, frame 0 is %d x %d (one batch takes frames of one size)" %
                             (i, f.height, f.width, f0.height, f0.width))
        if f.is_device != f0.is_device:
            raise ValueError("frame %d and frame 0 are not both host or both device frames" % i)
    return (DcFrame * len(frames))(*[f.c_frame() for f in frames]), f0.height, f0.width, f0.is_device


def _load():
    # PyTorch-ROCm wheels bundle their own HIP runtime under the same SONAME as /opt/rocm's.  Whichever is
    # loaded first serves the whole process; if ours comes first torch later reports "No HIP GPUs".  When
    # torch is installed, let it load first so both sides share one runtime (and torch streams / tensors can
    # be handed to dc_net_forward_batch).  DEEPCUT_NO_TORCH_PRELOAD=1 skips this.
    if not os.environ.get("DEEPCUT_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:  # torch absent: plain ROCm runtime
            pass
    lib = C.CDLL(lib_path())
    vp, ci, cp = C.c_void_p, C.c_int, C.c_char_p
    sig = {
        "dc_last_error": (cp, []),
        "dc_version": (cp, []),
        "dc_set_mode": (ci, [ci]),
        "dc_get_mode": (ci, []),
        "dc_set_device": (ci, [ci]),
        "dc_get_device": (ci, []),
        "dc_device_count": (ci, []),
        "dc_net_create": (ci, [cp, cp, ci, C.POINTER(vp)]),
        "dc_net_create_from_text": (ci, [cp, cp, ci, C.POINTER(vp)]),
        "dc_net_destroy": (ci, [vp]),
        "dc_net_clone": (ci, [vp, C.POINTER(vp)]),
        "dc_net_synchronize": (ci, [vp]),
        "dc_net_busy": (ci, [vp, C.POINTER(ci)]),
        "dc_net_set_option": (ci, [vp, ci, ci]),
        "dc_net_get_option": (ci, [vp, ci, C.POINTER(ci)]),
        "dc_net_copy_from": (ci, [vp, cp]),
        "dc_net_save": (ci, [vp, cp]),
        "dc_net_name": (cp, [vp]),
        "dc_net_num_layers": (ci, [vp]),
        "dc_net_layer_name": (cp, [vp, ci]),
        "dc_net_layer_type": (cp, [vp, ci]),
        "dc_net_num_blobs": (ci, [vp]),
        "dc_net_blob_name": (cp, [vp, ci]),
        "dc_net_blob": (ci, [vp, cp, C.POINTER(vp)]),
        "dc_net_num_inputs": (ci, [vp]),
        "dc_net_input_name": (cp, [vp, ci]),
        "dc_net_num_outputs": (ci, [vp]),
        "dc_net_output_name": (cp, [vp, ci]),
        "dc_net_layer_num_params": (ci, [vp, cp]),
        "dc_net_param": (ci, [vp, cp, ci, C.POINTER(vp)]),
        "dc_net_reshape": (ci, [vp]),
        "dc_net_forward": (ci, [vp, ci, ci, C.POINTER(C.c_float)]),
        "dc_net_forward_all": (ci, [vp]),
        "dc_blob_num_axes": (ci, [vp]),
        "dc_blob_shape": (ci, [vp, C.POINTER(ci), C.POINTER(ci)]),
        "dc_blob_count": (ci, [vp]),
        "dc_blob_reshape": (ci, [vp, ci, C.POINTER(ci)]),
        "dc_blob_cpu_data": (ci, [vp, C.POINTER(C.POINTER(C.c_float))]),
        "dc_blob_mutable_cpu_data": (ci, [vp, C.POINTER(C.POINTER(C.c_float))]),
        "dc_blob_head": (ci, [vp]),
        "dc_blob_gpu_data": (ci, [vp, C.POINTER(vp), C.POINTER(ci)]),
        "dc_blob_create": (ci, [ci, C.POINTER(ci), C.POINTER(vp)]),
        "dc_blob_destroy": (ci, [vp]),
        "dc_blob_mutable_gpu_data": (ci, [vp, C.POINTER(vp), C.POINTER(ci)]),
        "dc_blob_copy_from": (ci, [vp, vp, ci]),
        "dc_net_create_for_layer": (ci, [cp, ci, ci, C.POINTER(vp), C.POINTER(vp)]),
        "dc_net_forward_batch": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]),
        "dc_net_forward_requests": (ci, [vp, ci, C.POINTER(vp), ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_net_decode_pose": (ci, [vp, C.c_double, vp, ci, vp]),
        "dc_net_emit_maps": (ci, [vp, vp, vp, vp, ci, ci, vp]),
        "dc_net_forward_images": (ci, [vp, vp, ci, ci, ci, C.c_double, ci, vp, vp, vp, vp, vp]),
        "dc_image_canvas_size": (ci, [ci, ci, C.c_double, C.POINTER(ci), C.POINTER(ci)]),
        "dc_net_forward_boxes": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
        "dc_net_forward_frames": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, C.c_double, ci, vp, vp, vp, vp, vp]),
        "dc_net_forward_boxes_frame": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
        "dc_group_forward_frames": (ci, [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_double), vp, ci,
                                         C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_group_forward_boxes_frame": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, vp, vp, ci, C.POINTER(C.c_double), ci, ci, vp, C.POINTER(vp),
                                              C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_net_detect_parts": (ci, [vp, C.c_double, C.c_float, ci, ci, vp, vp]),
        "dc_net_decode_pairwise": (ci, [vp, C.c_double, ci, vp, vp, vp, vp]),
        "dc_pair_stats_read": (ci, [cp, ci, C.POINTER(ci), vp, vp, vp]),
        "dc_net_assemble_people": (ci, [vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dc_tracker_create": (ci, [C.POINTER(TrackerParams), C.POINTER(vp)]),
        "dc_tracker_destroy": (ci, [vp]),
        "dc_tracker_reset": (ci, [vp, ci]),
        "dc_tracker_update": (ci, [vp, ci, ci, vp, vp, vp, vp, vp]),
        "dc_tracker_update_slots": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp]),
        "dc_tracker_state": (ci, [vp, ci, vp, vp, vp, vp]),
        "dc_tracker_set_option": (ci, [vp, ci, ci]),
        "dc_tracker_get_option": (ci, [vp, ci, C.POINTER(ci)]),
        "dc_tracker_set_smoothing": (ci, [vp, C.POINTER(TrackSmoothParams)]),
        "dc_tracker_get_smoothing": (ci, [vp, C.POINTER(TrackSmoothParams)]),
        "dc_tracker_update_smoothed": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dc_tracker_smooth_state": (ci, [vp, ci, vp, vp]),
        "dc_net_track_people_slots": (ci, [vp, vp, vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dc_net_track_people": (ci, [vp, vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dc_group_track_people": (ci, [vp, vp, vp, ci, C.POINTER(FuseMirror), C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                       vp, vp]),
        "dc_group_track_people_slots": (ci, [vp, vp, vp, vp, ci, C.POINTER(FuseMirror), C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp,
                                             vp, vp, vp, vp]),
        "dc_net_track_frames_async": (ci, [vp, vp, vp, vp, ci, ci, ci, C.c_double, ci, vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp]),
        "dc_net_flops": (ci, [vp, C.POINTER(C.c_double)]),
        "dc_net_num_launches": (ci, [vp]),
        "dc_net_plan_text": (cp, [vp]),
        "dc_net_profile_text": (cp, [vp, ci]),
        "dc_net_stats": (ci, [vp, C.POINTER(C.c_longlong), ci]),
        "dc_net_reserve": (ci, [vp, ci, ci, ci]),
        "dc_net_device": (ci, [vp]),
        "dc_net_debug_info": (cp, [vp]),
        "dc_net_tune_report": (cp, [vp]),
        "dc_net_set_tile": (ci, [vp, cp, cp]),
        "dc_group_create": (ci, [C.POINTER(vp), ci, C.POINTER(vp)]),
        "dc_group_destroy": (ci, [vp]),
        "dc_group_size": (ci, [vp]),
        "dc_group_set_lanes": (ci, [vp, ci]),
        "dc_group_forward_batch": (ci, [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(vp), vp]),
        "dc_group_forward_images": (ci, [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_double), ci,
                                         C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_group_forward_boxes": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, C.POINTER(C.c_double), ci, ci, C.POINTER(vp), C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_group_fuse_maps": (ci, [vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]),
        "dc_group_detect_parts": (ci, [vp, vp, ci, C.c_float, ci, ci, vp, vp]),
        "dc_group_assemble_people": (ci, [vp, vp, ci, C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp, vp]),
        "dc_group_forward_images_mirrored": (ci, [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_double), vp, ci,
                                                  C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]),
        "dc_group_fuse_maps_mirrored": (ci, [vp, vp, ci, C.POINTER(FuseMirror), ci, vp, vp, vp, vp, vp, ci, vp]),
        "dc_group_detect_parts_mirrored": (ci, [vp, vp, ci, C.POINTER(FuseMirror), C.c_float, ci, ci, vp, vp]),
        "dc_group_assemble_people_mirrored": (ci, [vp, vp, ci, C.POINTER(FuseMirror), C.POINTER(AssembleParams), ci, vp, vp, vp, vp, vp, vp, vp,
                                                   vp]),
        "dc_group_decode_pose": (ci, [vp, vp, ci, C.POINTER(FuseMirror), vp, ci, vp]),
        "dc_group_forward_boxes_mirrored": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, C.POINTER(C.c_double), ci, ci, vp, C.POINTER(vp), C.POINTER(vp),
                                                 C.POINTER(vp), vp]),
        "dc_group_decode_boxes": (ci, [vp, vp, ci, C.POINTER(FuseMirror), vp, vp, vp, ci, vp]),
        "dc_group_plan_text": (cp, [vp]),
        "dc_group_profile_text": (cp, [vp, ci]),
        "dc_group_tune_report": (cp, [vp]),
        "dc_group_set_tile": (ci, [vp, cp, cp]),
        "dc_group_stats": (ci, [vp, C.POINTER(C.c_longlong), ci]),
        "dc_group_flops": (ci, [vp, C.POINTER(C.c_double)]),
        "dc_net_forward_host_async": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
        "dc_host_alloc": (ci, [C.c_size_t, C.POINTER(vp)]),
        "dc_host_free": (ci, [vp]),
        "dc_nets_choose_streams": (ci, [C.POINTER(vp), ci, ci, ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dc_net_stream": (ci, [vp, C.POINTER(vp)]),
        "dc_comm_create": (ci, [ci, C.POINTER(ci), ci, C.POINTER(vp)]),
        "dc_comm_destroy": (ci, [vp]),
        "dc_comm_transport": (ci, [vp]),
        "dc_forward_batch": (ci, [vp, C.POINTER(vp), ci, C.POINTER(vp), C.POINTER(ci * 2), ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "dc_comm_item_executor": (ci, [vp, ci]),
        "dc_comm_root_maps": (ci, [vp, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ci)]),
        "dc_lpt_schedule": (ci, [C.POINTER(C.c_double), ci, ci, C.POINTER(ci)]),
        "dc_conv_variant_count": (ci, []),
        "dc_conv_variant_name": (cp, [ci]),
        "dc_conv_variant_esize": (ci, [ci]),
        "dc_conv_bf16_variant_count": (ci, []),
        "dc_conv_bf16_variant_name": (cp, [ci]),
        "dc_wino_half_pack": (ci, [C.c_void_p, ci, ci, ci, C.c_void_p, C.c_void_p]),
        "dc_wino_blocks": (ci, [cp, ci, ci]),
        "dc_wino_cover": (ci, [ci, ci, C.c_void_p]),
        "dc_wino_mix_offered": (ci, [ci, ci, ci, ci]),
        "dc_stream1x1_pack": (ci, [C.c_void_p, ci, ci, C.c_void_p]),
        "dc_stem7x7_pack": (ci, [C.c_void_p, ci, C.c_void_p]),
        "dc_stream1x1f_pack": (ci, [C.c_void_p, ci, ci, C.c_void_p]),
        "dc_stream1x1f_rows": (ci, [C.c_void_p, ci, ci, ci, C.c_void_p, ci, C.c_void_p, C.c_void_p, C.c_void_p, ci, ci, ci, C.c_void_p, ci]),
        "dc_wino43_pack": (ci, [C.c_void_p, ci, ci, C.c_void_p]),
        "dc_net_pairwise_at": (ci, [vp, ci, C.c_void_p, C.c_void_p]),
        "dc_sparse_head_pack_size": (ci, [ci, ci, ci]),
        "dc_sparse_head_pack": (ci, [C.c_void_p, C.c_void_p, ci, ci, ci, C.c_void_p]),
        "dc_net_set_completion": (ci, [vp, C.POINTER(CompleteParams)]),
        "dc_net_get_completion": (ci, [vp, C.POINTER(CompleteParams)]),
        "dc_group_set_completion": (ci, [vp, C.POINTER(CompleteParams)]),
        "dc_group_get_completion": (ci, [vp, C.POINTER(CompleteParams)]),
        "dc_net_set_dedupe": (ci, [vp, C.POINTER(DedupeParams)]),
        "dc_net_get_dedupe": (ci, [vp, C.POINTER(DedupeParams), C.c_void_p]),
        "dc_group_set_dedupe": (ci, [vp, C.POINTER(DedupeParams)]),
        "dc_group_get_dedupe": (ci, [vp, C.POINTER(DedupeParams), C.c_void_p]),
        "dc_dedupe_people": (ci, [C.POINTER(DedupeParams), ci, ci, ci] + [C.c_void_p] * 8),
        "dc_draw_people": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(DrawStyle), vp]),
        "dc_draw_limits": (ci, [C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
        "dc_redact_people": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, vp, C.POINTER(RedactStyle), vp, vp]),
        "dc_tracker_set_appearance": (ci, [vp, C.POINTER(TrackAppearanceParams)]),
        "dc_tracker_get_appearance": (ci, [vp, C.POINTER(TrackAppearanceParams)]),
        "dc_tracker_update_appearance": (ci, [vp, ci, ci] + [vp] * 10),
        "dc_tracker_appearance_state": (ci, [vp, ci, vp, vp, vp, vp, vp]),
        "dc_describe_people": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, C.POINTER(AppearanceStyle), vp, vp]),
        "dc_overlay_people_device": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(DrawStyle), C.POINTER(RedactStyle),
                                          vp, ci, vp, ci, vp, vp]),
        "dc_net_track_frames_async_overlay": (ci, [vp, vp, vp, vp, ci, ci, ci, C.c_double, ci, vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp,
                                                   vp, vp, vp, vp, vp, C.POINTER(DrawStyle), C.POINTER(RedactStyle), vp, ci, vp, ci, vp]),
        "dc_label_people": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(LabelStyle), vp]),
        "dc_label_font": (ci, [ci, C.POINTER(C.c_ubyte * 7)]),
        "dc_overlay_people_device_styles": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(OverlayStyles), vp, vp]),
        "dc_net_track_frames_async_styles": (ci, [vp, vp, vp, vp, ci, ci, ci, C.c_double, ci, vp, C.POINTER(AssembleParams), ci, vp, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, C.POINTER(OverlayStyles), vp]),
        "dc_draw_heatmap": (ci, [C.POINTER(DcFrame), ci, ci, ci, ci, vp, ci, ci, ci, ci, C.POINTER(HeatGeometry), C.POINTER(HeatStyle), vp]),
        "dc_net_draw_heatmap": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, ci, C.POINTER(HeatGeometry), C.POINTER(HeatStyle)]),
        "dc_group_draw_heatmap": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, ci, vp, ci, C.c_double, C.c_double, C.POINTER(HeatStyle)]),
        "dc_group_draw_heatmap_mirrored": (ci, [vp, C.POINTER(DcFrame), ci, ci, ci, ci, vp, ci, C.POINTER(FuseMirror), C.c_double, C.c_double,
                                                C.POINTER(HeatStyle)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib, sorted(sig)


_lib, EXPORTED_SYMBOLS = _load()


def _check(rc):
    if rc != 0:
        raise DeepcutError(rc, (_lib.dc_last_error() or b"").decode())


def set_mode_cpu():
    _check(_lib.dc_set_mode(0))


def set_mode_gpu():
    _check(_lib.dc_set_mode(1))


def set_device(device_id):
    _check(_lib.dc_set_device(int(device_id)))


def device_count():
    return _lib.dc_device_count()


# Net(..., dtype=...) -> DC_OPT_DTYPE
_DTYPES = {"f32": 0, "float32": 0, "f16": 1, "float16": 1, "bf16": 2, "bfloat16": 2}


def conv_variants():
    """[(name, element size)] of the gather-GEMM tile variants, in DC_CONV_VARIANT index order (diagnostics)."""
    return [((_lib.dc_conv_variant_name(i) or b"").decode(), _lib.dc_conv_variant_esize(i)) for i in range(_lib.dc_conv_variant_count())]


def conv_variants_bf16():
    """[name] of the bfloat16 tile variants (their own table), in DC_CONV_VARIANT_BF16 index order."""
    return [(_lib.dc_conv_bf16_variant_name(i) or b"").decode() for i in range(_lib.dc_conv_bf16_variant_count())]


def wino_blocks(tile, tiles_y, tiles_x):
    """dc_wino_blocks: the tile blocks the float32 Winograd form `tile` needs for a tiles_y x tiles_x tile grid (-1: not such a form)."""
    return _lib.dc_wino_blocks(tile.encode(), int(tiles_y), int(tiles_x))


def wino_cover(tiles_y, tiles_x):
    """dc_wino_cover: the cover of a tiles_y x tiles_x tile grid by 4 x 8- and 5 x 6-tile blocks that the forms wino_f23_mix / wino_f23_mix_w16
    run, as a dict: vertical, cut, blocks, na, nb, a_nby, a_nbx, b_nby, b_nbx, b_ty0, b_tx0, offered (None on bad arguments)."""
    out = (C.c_int * 12)()
    if _lib.dc_wino_cover(int(tiles_y), int(tiles_x), C.cast(out, C.c_void_p)) < 0:
        return None
    keys = ("vertical", "cut", "blocks", "na", "nb", "a_nby", "a_nbx", "b_nby", "b_nbx", "b_ty0", "b_tx0", "offered")
    return dict(zip(keys, (int(v) for v in out)))


def wino_mix_offered(tiles_y, tiles_x, images, cout):
    """dc_wino_mix_offered: whether the per-shape timing tries wino_f23_mix / wino_f23_mix_w16 for a 3x3 layer of `images` (phase) images of
    tiles_y x tiles_x tiles and cout output channels (-1 on bad arguments)."""
    return _lib.dc_wino_mix_offered(int(tiles_y), int(tiles_x), int(images), int(cout))


def stream1x1_pack(g):
    """dc_stream1x1_pack: the filter image of the streaming 1x1 form (csrc/stream1x1.hip) of g [cout, k] (or [cout, k, 1, 1]) as the lowering
    packs it: float32 values in the order [cout/32][k/16][64 lanes][8] (tests / diagnostics)."""
    g = np.ascontiguousarray(g, np.float32)
    cout, k = g.shape[0], int(np.prod(g.shape[1:]))
    out = np.empty((cout // 32, k // 16, 64, 8), np.float32)
    _check(_lib.dc_stream1x1_pack(g.ctypes.data_as(C.c_void_p), cout, k, out.ctypes.data_as(C.c_void_p)))
    return out


def stream1x1f_pack(g):
    """dc_stream1x1f_pack: the filter image of the float32 streaming 1x1 form (csrc/stream1x1_f32.hip) of g [cout, k] (or [cout, k, 1, 1]) as
    the lowering packs it: [cout/16][k/16][64 lanes][4] (tests / diagnostics)."""
    g = np.ascontiguousarray(g, np.float32)
    cout, k = g.shape[0], int(np.prod(g.shape[1:]))
    out = np.empty((cout // 16, k // 16, 64, 4), np.float32)
    _check(_lib.dc_stream1x1f_pack(g.ctypes.data_as(C.c_void_p), cout, k, out.ctypes.data_as(C.c_void_p)))
    return out


def stream1x1f_rows(x, g, y, y_c0=0, m=None, scale=None, shift=None, resid=None, relu=False):
    """dc_stream1x1f_rows: one launch of the float32 streaming 1x1 form on x [rows, x_stride] (a pixel's channels: the first k floats of its row),
    filters g [cout, k]; writes channels [y_c0, y_c0 + cout) of the first m rows (default: all rows of x) of y [y_rows, y_stride] IN PLACE;
    resid: the shortcut, an array like y (tests / diagnostics)."""
    x, g = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(g, np.float32)
    assert y.dtype == np.float32 and y.flags["C_CONTIGUOUS"] and y.ndim == 2 and x.ndim == 2 and g.ndim == 2
    m = x.shape[0] if m is None else m
    assert m <= x.shape[0]
    opt = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (scale, shift, resid)]
    assert opt[2] is None or opt[2].shape == y.shape
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    _check(_lib.dc_stream1x1f_rows(ptr(x), m, g.shape[1], x.shape[1], ptr(g), g.shape[0], ptr(opt[0]), ptr(opt[1]), ptr(y), y.shape[0], y.shape[1],
                                   y_c0, ptr(opt[2]), 1 if relu else 0))
    return y


def wino43_pack(g):
    """dc_wino43_pack: the filter image of the unfused Winograd F(4x4,3x3) form (csrc/wino43_f32.hip) of g [cout, cin, 3, 3] as the lowering
    packs it: [36 points][cout/16][cin/16][64 lanes][4], point 6 i + j = (G g G^T)[i][j] in stream1x1f_pack's order (tests / diagnostics)."""
    g = np.ascontiguousarray(g, np.float32)
    cout, cin = g.shape[0], g.shape[1]
    out = np.empty((36, cout // 16, cin // 16, 64, 4), np.float32)
    _check(_lib.dc_wino43_pack(g.ctypes.data_as(C.c_void_p), cout, cin, out.ctypes.data_as(C.c_void_p)))
    return out


def sparse_head_pack(ws, wd):
    """dc_sparse_head_pack: the filter image of the sparse pairwise head (csrc/sparse_head.hip) of the skip filters ws [cout, k3] (or
    [cout, k3, 1, 1]) and the deconvolution filters wd [k5, cout, 3, 3] as the library packs it for float32 nets -> (taps float32
    [9, ceil(cout/32), ceil(k5/8), 64, 4], skip float32 [ceil(cout/32), ceil(k3/8), 64, 4]): lane l of K block j of chunk q holds
    W[k = 8j + 4(l // 32) + m][n = 32q + l % 32], zeros beyond k and cout (tests / diagnostics)."""
    ws = np.ascontiguousarray(ws, np.float32)
    wd = np.ascontiguousarray(wd, np.float32)
    cout, k3 = ws.shape[0], int(np.prod(ws.shape[1:]))
    if wd.ndim != 4 or wd.shape[1:] != (cout, 3, 3):
        raise ValueError("wd must be [k5, %d, 3, 3], got %s" % (cout, wd.shape))
    k5 = wd.shape[0]
    n = _lib.dc_sparse_head_pack_size(cout, k3, k5)
    if n < 0:
        raise ValueError("bad sizes cout=%d k3=%d k5=%d" % (cout, k3, k5))
    out = np.empty(n, np.float32)
    _check(_lib.dc_sparse_head_pack(ws.ctypes.data_as(C.c_void_p), wd.ctypes.data_as(C.c_void_p), cout, k3, k5, out.ctypes.data_as(C.c_void_p)))
    nq, n5, n3 = (cout + 31) // 32, (k5 + 7) // 8, (k3 + 7) // 8
    cut = 9 * nq * n5 * 256
    return out[:cut].reshape(9, nq, n5, 64, 4), out[cut:].reshape(nq, n3, 64, 4)


def stem7x7_pack(g):
    """dc_stem7x7_pack: the filter image of the float16 stem kernel (csrc/stem_f16.hip) of g [64, c, 7, 7], c <= 4: float32 values in the
    order [fragment 2][kernel row 7][K step 2][64 lanes][8] (tests / diagnostics)."""
    g = np.ascontiguousarray(g, np.float32)
    if g.ndim != 4 or g.shape[0] != 64 or g.shape[2:] != (7, 7):
        raise ValueError("stem7x7_pack: g must be [64, c, 7, 7]")
    out = np.empty((2, 7, 2, 64, 8), np.float32)
    _check(_lib.dc_stem7x7_pack(g.ctypes.data_as(C.c_void_p), g.shape[1], out.ctypes.data_as(C.c_void_p)))
    return out


def wino_half_pack(g, rowscale=True):
    """dc_wino_half_pack: the float16 Winograd form's filter image of g [cout, cin, 3, 3] as the lowering packs it (float32 values,
    before the conversion to half) -> (image [cout/32, 4, cin/16, 4, 64, 8], row_scale [cout]).  Host only (tests)."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    cout, cin = g.shape[:2]
    out = np.empty((cout // 32, 4, cin // 16, 4, 64, 8), np.float32)
    rs = np.empty(cout, np.float32)
    _check(_lib.dc_wino_half_pack(g.ctypes.data_as(C.c_void_p), cout, cin, 1 if rowscale else 0, out.ctypes.data_as(C.c_void_p), rs.ctypes.data_as(C.c_void_p)))
    return out, rs


def canvas_size(height, width, scale):
    """(H, W) of the network input the demo builds for an image at `scale` (estimate_pose.py:85-88)."""
    h, w = C.c_int(), C.c_int()
    _check(_lib.dc_image_canvas_size(int(height), int(width), float(scale), C.byref(h), C.byref(w)))
    return h.value, w.value


def member_canvas(side, pyramid_scale):
    """A NetGroup member's canvas side in the box entry: `side` * pyramid_scale rounded up to the stride 8."""
    return int(np.ceil(float(side) * float(pyramid_scale) / 8) * 8)


def check_boxes(image_shape, boxes, scales=1.0, canvas=None):
    """The box entry's arguments, checked on the host before anything reaches the device.  image_shape: (H, W[, 3]); boxes: n x 4
    integers (x0, y0, x1, y1), half-open, inside the image; scales: one number or one per box.  -> (boxes int32 [n, 4], scales
    float64 [n], (canvas_h, canvas_w)); canvas None = the smallest canvas that holds every box's own canvas (canvas_size of the
    crop at its scale).  Raises ValueError naming the box at fault."""
    h, w = int(image_shape[0]), int(image_shape[1])
    b = np.asarray(boxes)
    if b.size == 0:
        b = b.reshape(0, 4)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError("boxes must be an n x 4 array of (x0, y0, x1, y1), got shape %s" % (b.shape,))
    if not np.issubdtype(b.dtype, np.integer):
        if not (np.isfinite(b).all() and (b == np.round(b)).all()):
            raise ValueError("box corners must be whole pixels")
    b = np.ascontiguousarray(b, dtype=np.int32)
    n = b.shape[0]
    sc = np.asarray(scales, np.float64)
    sc = np.ascontiguousarray(np.full(n, float(sc)) if sc.ndim == 0 else sc.reshape(-1))
    if sc.shape[0] != n:
        raise ValueError("%d scales for %d boxes" % (sc.shape[0], n))
    need_h = need_w = 8
    for i in range(n):
        x0, y0, x1, y1 = (int(v) for v in b[i])
        if x1 <= x0 or y1 <= y0:
            raise ValueError("box %d (%d, %d, %d, %d) is empty" % (i, x0, y0, x1, y1))
        if x0 < 0 or y0 < 0 or x1 > w or y1 > h:
            raise ValueError("box %d (%d, %d, %d, %d) lies outside the %dx%d image" % (i, x0, y0, x1, y1, h, w))
        if not (np.isfinite(sc[i]) and sc[i] > 0):
            raise ValueError("box %d (%d, %d, %d, %d): scale %r is not positive" % (i, x0, y0, x1, y1, sc[i]))
        if int((x1 - x0 + 64) * sc[i]) < 1 or int((y1 - y0 + 64) * sc[i]) < 1:
            raise ValueError("box %d (%d, %d, %d, %d): scale %r leaves no pixels" % (i, x0, y0, x1, y1, sc[i]))
        ch, cw = canvas_size(y1 - y0, x1 - x0, sc[i])
        if canvas is not None and (ch > canvas[0] or cw > canvas[1]):
            raise ValueError("box %d (%d, %d, %d, %d) at scale %r needs a %dx%d canvas, larger than %dx%d"
                             % (i, x0, y0, x1, y1, sc[i], ch, cw, canvas[0], canvas[1]))
        need_h, need_w = max(need_h, ch), max(need_w, cw)
    if canvas is None:
        canvas = (need_h, need_w)
    canvas = (int(canvas[0]), int(canvas[1]))
    if min(canvas) < 8 or canvas[0] % 8 or canvas[1] % 8:
        raise ValueError("canvas %dx%d is not a positive multiple of 8 on both sides" % canvas)
    return b, sc, canvas


def pair_stats_read(path, max_edges=4096):
    """dc_pair_stats_read: the `joint_pairs_stats` text file of a model -> (edges int32 [E, 2] of 0-based joints, mean float64 [E, 2],
    std float64 [E, 2]).  Host only."""
    n = C.c_int()
    edges = np.zeros((max_edges, 2), np.int32)
    mean, std = np.zeros((max_edges, 2), np.float64), np.zeros((max_edges, 2), np.float64)
    _check(_lib.dc_pair_stats_read(os.fsencode(path), int(max_edges), C.byref(n), edges.ctypes.data_as(C.c_void_p),
                                   mean.ctypes.data_as(C.c_void_p), std.ctypes.data_as(C.c_void_p)))
    return edges[:n.value].copy(), mean[:n.value].copy(), std[:n.value].copy()


def check_assembly(num_joints, n_edges_wanted, edges, mean=None, std=None, joint_order=None, scale=1.0, threshold=0.1, radius=1, max_det=16,
                   max_cost=32.0, seed_threshold=0.5, max_people=32, min_joints=1):
    """The arguments of Net.assemble_people, checked on the host before raw pointers cross the boundary (the library reads
    2 * n_edges numbers through each of them).  n_edges_wanted: next_pred channels / 2, or None when unknown.
    -> (AssembleParams, edges int32 [E, 2], mean or None, std or None, joint_order int32 [J] or None).  Raises ValueError naming the argument."""
    j = int(num_joints)
    e = np.asarray(edges)
    if e.size == 0:
        e = e.reshape(0, 2)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError("edges must be an E x 2 array of 0-based (joint, next joint), got shape %s" % (e.shape,))
    if not np.issubdtype(e.dtype, np.integer):
        if not (np.isfinite(e).all() and (e == np.round(e)).all()):
            raise ValueError("edges must hold whole joint indices")
    e = np.ascontiguousarray(e, dtype=np.int32)
    for l in range(e.shape[0]):
        a, b = int(e[l, 0]), int(e[l, 1])
        if not (0 <= a < j and 0 <= b < j):
            raise ValueError("edges: edge %d (%d, %d) names a joint outside [0, %d)" % (l, a, b, j))
        if a == b:
            raise ValueError("edges: edge %d joins joint %d to itself" % (l, a))
    if n_edges_wanted is not None and e.shape[0] != int(n_edges_wanted):
        raise ValueError("edges: %d edges for a next_pred of %d channels (2 per regression edge)" % (e.shape[0], 2 * int(n_edges_wanted)))

    def stat(name, v, positive):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.size != 2 * e.shape[0]:
            raise ValueError("%s must be [E, 2] = [%d, 2], got shape %s" % (name, e.shape[0], v.shape))
        if not np.isfinite(v).all() or (positive and not (v > 0).all()):
            raise ValueError("%s must be finite%s" % (name, " and positive" if positive else ""))
        return v.reshape(e.shape[0], 2)

    m, s = stat("mean", mean, False), stat("std", std, True)
    order = None
    if joint_order is not None:
        order = np.asarray(joint_order)
        if order.ndim != 1 or order.shape[0] != j or sorted(int(v) for v in order) != list(range(j)) or not (order == np.round(order)).all():
            raise ValueError("joint_order must be a permutation of 0..%d, got %r" % (j - 1, list(np.asarray(joint_order).tolist())))
        order = np.ascontiguousarray(order, dtype=np.int32)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("scale must be positive, got %r" % (scale,))
    if not threshold >= 0:
        raise ValueError("threshold must be >= 0, got %r" % (threshold,))
    if not 0 <= int(radius) <= 64:
        raise ValueError("radius must be in [0, 64], got %r" % (radius,))
    if not 1 <= int(max_det) <= MAX_ASSEMBLE_DET:
        raise ValueError("max_det must be in [1, %d], got %r" % (MAX_ASSEMBLE_DET, max_det))
    if not (np.isfinite(max_cost) and max_cost >= 0):
        raise ValueError("max_cost must be finite and >= 0, got %r" % (max_cost,))
    if not np.isfinite(seed_threshold):
        raise ValueError("seed_threshold must be finite, got %r" % (seed_threshold,))
    if not 1 <= int(max_people) <= MAX_ASSEMBLE_PEOPLE:
        raise ValueError("max_people must be in [1, %d], got %r" % (MAX_ASSEMBLE_PEOPLE, max_people))
    if not 1 <= int(min_joints) <= j:
        raise ValueError("min_joints must be in [1, %d], got %r" % (j, min_joints))
    q = AssembleParams(float(scale), float(threshold), int(radius), int(max_det), float(max_cost), float(seed_threshold), int(max_people),
                       int(min_joints))
    return q, e, m, s, order


def lpt_schedule(costs, nexec):
    """Longest-processing-time-first shares (dc_lpt_schedule: the schedule dc_forward_batch deals images by; the same lists as
    deepcut_tools.lpt_shards): per executor the item indices, ascending."""
    n = len(costs)
    out = (C.c_int * max(n, 1))()
    _check(_lib.dc_lpt_schedule((C.c_double * max(n, 1))(*[float(c) for c in costs]), n, int(nexec), out))
    shares = [[] for _ in range(int(nexec))]
    for i in range(n):
        shares[out[i]].append(i)
    return shares


def pinned_empty(shape, dtype=np.float32):
    """A NumPy array over pinned (page-locked) host memory from dc_host_alloc, freed when the array and every view of it are gone:
    what Net.forward_host_async / Pipeline.submit_host copy from and to without a staging pass."""
    import weakref

    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if len(tuple(shape)) else 1
    p = C.c_void_p()
    _check(_lib.dc_host_alloc(max(1, n * dt.itemsize), C.byref(p)))
    buf = (C.c_char * max(1, n * dt.itemsize)).from_address(p.value)
    a = np.frombuffer(buf, dt, count=n).reshape(shape)
    weakref.finalize(a.base if a.base is not None else a, _lib.dc_host_free, C.c_void_p(p.value))
    return a


def choose_streams(nets, candidates=8, reps=3):
    """dc_nets_choose_streams: the executors' own streams (stream="own") chosen by timing their real forwards on assignments of a
    process-wide pool of candidate streams — which hardware queue a stream landed on decides what forwards "in flight" are worth
    (380 to 490 images/s for four batch-1 executors) and the API does not say.  Every net must have run or reserved its shape.
    -> {"forwards_per_s_chosen": ..., "forwards_per_s_first_created": ...}."""
    k = len(nets)
    a, b = C.c_double(), C.c_double()
    _check(_lib.dc_nets_choose_streams((C.c_void_p * k)(*[n._h for n in nets]), k, int(candidates), int(reps), C.byref(a), C.byref(b)))
    return {"forwards_per_s_chosen": a.value, "forwards_per_s_first_created": b.value}


class _OutPool(object):
    """Result arrays handed out again once NOBODY holds the previous hand-out or a view of it.  The memory belongs to a ctypes
    buffer the pool keeps; every hand-out is a NEW ndarray over it and the pool keeps only a weak reference to that ndarray:
    views hold their base array alive, so the weak reference dies exactly when the last of them is gone.  (Round 4 asked
    sys.getrefcount, an implementation detail that changes with borrowed-reference loads and free-threaded builds.)"""

    def __init__(self, keep=4):
        self.keep, self.entries = keep, []

    def take(self, shape):
        import weakref

        n = int(np.prod(shape))
        for e in self.entries:
            if e[1] == n and (e[2] is None or e[2]() is None):
                a = np.frombuffer(e[0], np.float32, count=n)
                e[2] = weakref.ref(a)
                return a.reshape(shape)
        buf = (C.c_float * max(n, 1))()  # zero-filled: the pages exist before the first device-to-host copy lands in them
        a = np.frombuffer(buf, np.float32, count=n)
        if len(self.entries) < self.keep:
            import weakref as _w

            self.entries.append([buf, n, _w.ref(a)])
        return a.reshape(shape)


class Tracker(object):
    """The same person across the frames of a video (dc_tracker_*): `slots` independent sequences of at most `max_tracks` live tracks
    each, kept on the device.  An update associates the people of a frame with the slot's tracks greedily by a size-normalised mean
    squared joint distance and gives every person an id that stays with them; the rule is stated in include/deepcut_hip.h
    (dc_tracker_update).  PARITY UNPINNED BY THE REFERENCE, which stops at the maps: the rule is this project's own.
    sigma: [J] per-joint tolerance (None = 1.0); a track and a person are compared over the joints both hold (at least min_common), a
    match needs a distance <= max_dist, a track without a match for more than max_misses updates in a row is dropped; min_size: lower
    bound in pixels of the track size the distance is normalised by; motion: 1 compares with the pose moved on by its velocity, 0 with
    the last pose.  THE DEFAULTS OF max_misses, min_common, max_dist, min_size AND sigma ARE PLACEHOLDERS, NOT TUNED ON REAL VIDEO:
    override them.  assign: "greedy" (the default: the closest pair first, step 4 of the rule) or "optimal" (step 4': the assignment
    with the smallest total distance, an unmatched track costing max_dist — two people who pass each other keep their ids where greedy
    matching swaps them); also a property, which may change between updates: the tracks stay.
    smooth: None / False (off, the default), True (SMOOTH_DEFAULTS: PLACEHOLDERS, NOT TUNED ON REAL VIDEO) or a dict of some of
    min_cutoff, beta, d_cutoff, max_hold — step 8 of the rule: a filter per track and joint on the device smooths the poses and
    bridges joints that vanish for at most max_hold updates; no id, place or distance changes by a bit.  Also the property `smoothing`.
    appearance: None / False (off, the default), True (APPEARANCE_DEFAULTS: PLACEHOLDERS, NOT TUNED ON REAL VIDEO) or a dict of some of
    min_pixels, alpha256, reid_max, max_age, min_hits — the appearance steps of the rule (dc_tracker_update_appearance): a freed track's
    appearance model waits in a gallery, and a person born with a descriptor (`describe_people`, handed to `update(desc=...)`) close
    enough to it takes the old id back.  Also the property `appearance`.
    Creation needs no device; updates need GPU mode.  The calls of this class are synchronous; updates apply in call order, those
    enqueued by `Net.track_frames_async` included (the synchronous calls wait for them first)."""

    ASSIGN = {"greedy": 0, "optimal": 1}  # DC_TRACK_ASSIGN_*
    _OPT_ASSIGN = 1  # DC_TRACK_OPT_ASSIGN

    def __init__(self, n_joints=14, slots=1, max_tracks=64, sigma=None, max_misses=5, min_common=3, max_dist=0.25, min_size=32.0, motion=1,
                 assign="greedy", smooth=None, appearance=None):
        self._h = None
        self._assign_value(assign)
        smooth = smooth_params(smooth)
        appearance = appearance_params(appearance)
        sig = None
        if sigma is not None:
            sig = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
            if sig.shape[0] != int(n_joints):
                raise ValueError("sigma must hold one value per joint: %d values for %d joints" % (sig.shape[0], int(n_joints)))
        q = TrackerParams(int(slots), int(max_tracks), int(n_joints), None if sig is None else sig.ctypes.data, int(max_misses),
                          int(min_common), float(max_dist), float(min_size), int(motion))
        h = C.c_void_p()
        _check(_lib.dc_tracker_create(C.byref(q), C.byref(h)))
        self._h = h
        self.n_joints, self.slots, self.max_tracks = int(n_joints), int(slots), int(max_tracks)
        if assign != "greedy":
            self.assign = assign
        if smooth is not None:
            self.smoothing = smooth
        if appearance is not None:
            self.appearance = appearance

    @classmethod
    def _assign_value(cls, assign):
        if not isinstance(assign, str) or assign not in cls.ASSIGN:
            raise ValueError("assign must be one of %s, got %r" % (", ".join(repr(k) for k in sorted(cls.ASSIGN)), assign))
        return cls.ASSIGN[assign]

    @property
    def assign(self):
        """The matching rule of the updates to come: "greedy" or "optimal" (DC_TRACK_OPT_ASSIGN)."""
        v = C.c_int(-1)
        _check(_lib.dc_tracker_get_option(self._h, self._OPT_ASSIGN, C.byref(v)))
        return [k for k, x in self.ASSIGN.items() if x == v.value][0]

    @assign.setter
    def assign(self, assign):
        _check(_lib.dc_tracker_set_option(self._h, self._OPT_ASSIGN, self._assign_value(assign)))

    @property
    def smoothing(self):
        """None (off, the default) or {"min_cutoff", "beta", "d_cutoff", "max_hold"}: step 8 of the rule (dc_tracker_set_smoothing).
        Assign None / False, True (SMOOTH_DEFAULTS: PLACEHOLDERS, NOT TUNED ON REAL VIDEO) or a dict of some of the four; cutoffs are in
        cycles per update.  May change between updates: off -> on starts with empty filters, a change while on keeps them.  A bad value
        raises DeepcutError naming the field, with or without a device."""
        q = TrackSmoothParams()
        _check(_lib.dc_tracker_get_smoothing(self._h, C.byref(q)))
        if not q.enabled:
            return None
        return {"min_cutoff": float(q.min_cutoff), "beta": float(q.beta), "d_cutoff": float(q.d_cutoff), "max_hold": int(q.max_hold)}

    @smoothing.setter
    def smoothing(self, smooth):
        d = smooth_params(smooth)
        if d is None:
            _check(_lib.dc_tracker_set_smoothing(self._h, None))
            return
        try:
            q = TrackSmoothParams(1, float(d["min_cutoff"]), float(d["beta"]), float(d["d_cutoff"]), int(d["max_hold"]))
        except (TypeError, ValueError) as e:
            raise ValueError("smooth: min_cutoff, beta and d_cutoff must be numbers, max_hold a whole number (%s)" % (e,))
        _check(_lib.dc_tracker_set_smoothing(self._h, C.byref(q)))

    @property
    def appearance(self):
        """None (off, the default) or {"min_pixels", "alpha256", "reid_max", "max_age", "min_hits"}: the appearance steps of the rule
        (dc_tracker_set_appearance).  Assign None / False, True (APPEARANCE_DEFAULTS: PLACEHOLDERS, NOT TUNED ON REAL VIDEO) or a dict of
        some of the five.  May change between updates: off -> on starts with no model and an empty gallery, a change while on keeps them.
        A bad value raises DeepcutError naming the field, with or without a device."""
        q = TrackAppearanceParams()
        _check(_lib.dc_tracker_get_appearance(self._h, C.byref(q)))
        if not q.enabled:
            return None
        return {k: int(getattr(q, k)) for k in _APPEARANCE_TRACK_KEYS}

    @appearance.setter
    def appearance(self, appearance):
        d = appearance_params(appearance)
        if d is None:
            _check(_lib.dc_tracker_set_appearance(self._h, None))
            return
        try:
            q = TrackAppearanceParams(1, *[int(d[k]) for k in _APPEARANCE_TRACK_KEYS])
        except (TypeError, ValueError) as e:
            raise ValueError("appearance: min_pixels, alpha256, reid_max, max_age and min_hits must be whole numbers (%s)" % (e,))
        _check(_lib.dc_tracker_set_appearance(self._h, C.byref(q)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.dc_tracker_destroy(self._h)
            self._h = None

    def update(self, people, n_people=None, return_dist=False, slot_of=None, return_smooth=False, desc=None, return_reid=False):
        """people: [nb, P, J, 3] float64 (x, y, score; a joint counts when its score > 0) with n_people [nb] of them valid per image, or
        a list of nb arrays [m_b, J, 3] (n_people is then their lengths) — image b updates slot b.  This is how poses that did not come
        from `track_people` (top-down poses of `forward_boxes`, say) get tracked.
        slot_of: [nb] ints in [0, slots), the slot every image updates (dc_tracker_update_slots): images of one slot apply in ascending b,
        each on the state the one before left — several frames of one video in one call; nb may then be 1..64 whatever `slots` is.
        -> (ids int64 [nb, P], place int32 [nb, P]): -1 beyond n_people[b] and for a person no track place was free for; with
        return_dist also the distances float64 [nb, max_tracks, P].  return_smooth (needs `smoothing` on, dc_tracker_update_smoothed):
        -> (ids, place[, dist], smooth, src) with smooth float64 [nb, P, J, 3], the smoothed poses, and src int32 [nb, P, J]: 0 nothing,
        1 observed, 2 bridged.
        desc (needs `appearance` on, dc_tracker_update_appearance): int32 [nb, P, 3, 16] as `describe_people` returns it for these people
        — a person born with a valid descriptor may take an id back from the gallery; return_reid: reid int32 [nb, P] comes last in the
        tuple, 1 where that happened.  Without desc an update of a tracker with appearance on re-identifies nobody."""
        j = self.n_joints
        if n_people is None and not (isinstance(people, np.ndarray) and people.ndim == 4):
            arrs = [np.asarray(a, np.float64).reshape(-1, j, 3) for a in people]
            n = np.array([a.shape[0] for a in arrs], np.int32)
            ppl = np.zeros((len(arrs), max(1, int(n.max()) if len(arrs) else 1), j, 3), np.float64)
            for b, a in enumerate(arrs):
                ppl[b, :a.shape[0]] = a
        else:
            ppl = np.ascontiguousarray(people, dtype=np.float64)
            if ppl.ndim != 4 or ppl.shape[2:] != (j, 3):
                raise ValueError("people must be [nb, P, %d, 3] (x, y, score), got shape %s" % (j, ppl.shape))
            n = np.full(ppl.shape[0], ppl.shape[1], np.int32) if n_people is None else np.ascontiguousarray(n_people, dtype=np.int32).reshape(-1)
            if n.shape[0] != ppl.shape[0]:
                raise ValueError("n_people must hold one count per image: %d counts for %d images" % (n.shape[0], ppl.shape[0]))
        nb, p = ppl.shape[:2]
        ids = np.full((nb, p), -1, np.int64)
        place = np.full((nb, p), -1, np.int32)
        dist = np.zeros((nb, self.max_tracks, p), np.float64) if return_dist else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        if desc is not None or return_reid:
            dsc = None if desc is None else np.ascontiguousarray(desc, dtype=np.int32)
            if dsc is not None and dsc.shape != (nb, p, 3, APPEARANCE_BINS):
                raise ValueError("desc must be [%d, %d, 3, %d] like people, got shape %s" % (nb, p, APPEARANCE_BINS, dsc.shape))
            reid = np.zeros((nb, p), np.int32)
            smooth, src = (np.zeros((nb, p, j, 3), np.float64), np.zeros((nb, p, j), np.int32)) if return_smooth else (None, None)
            _check(_lib.dc_tracker_update_appearance(self._h, nb, p, None if slot_of is None else ptr(_slot_map(slot_of, nb)), ptr(n), ptr(ppl),
                                                     ptr(dsc), ptr(ids), ptr(place), ptr(dist), ptr(reid), ptr(smooth), ptr(src)))
            out = (ids, place) + ((dist,) if return_dist else ()) + ((smooth, src) if return_smooth else ())
            return out + ((reid,) if return_reid else ())
        if return_smooth:
            smooth, src = np.zeros((nb, p, j, 3), np.float64), np.zeros((nb, p, j), np.int32)
            _check(_lib.dc_tracker_update_smoothed(self._h, nb, p, None if slot_of is None else ptr(_slot_map(slot_of, nb)), ptr(n), ptr(ppl),
                                                   ptr(ids), ptr(place), ptr(dist), ptr(smooth), ptr(src)))
            return (ids, place, dist, smooth, src) if return_dist else (ids, place, smooth, src)
        if slot_of is None:
            _check(_lib.dc_tracker_update(self._h, nb, p, ptr(n), ptr(ppl), ptr(ids), ptr(place), ptr(dist)))
        else:
            _check(_lib.dc_tracker_update_slots(self._h, nb, p, ptr(_slot_map(slot_of, nb)), ptr(n), ptr(ppl), ptr(ids), ptr(place), ptr(dist)))
        return (ids, place, dist) if return_dist else (ids, place)

    def reset(self, slot=None):
        """Forget the tracks of `slot` (None: of every slot); its ids start again at 0."""
        _check(_lib.dc_tracker_reset(self._h, -1 if slot is None else int(slot)))

    def state(self, slot=0):
        """The tracks of a slot, e.g. to see where occluded people were last seen -> dict: "ids" int64 [T] (-1 = free place), "misses"
        int32 [T] (updates since the last match), "hits" int32 [T] (matches so far, the birth included), "poses" float64 [T, J, 3]."""
        t, j = self.max_tracks, self.n_joints
        out = {"ids": np.full(t, -1, np.int64), "misses": np.zeros(t, np.int32), "hits": np.zeros(t, np.int32),
               "poses": np.zeros((t, j, 3), np.float64)}
        _check(_lib.dc_tracker_state(self._h, int(slot), *[out[k].ctypes.data_as(C.c_void_p) for k in ("ids", "misses", "hits", "poses")]))
        return out

    def appearance_state(self, slot=0):
        """The appearance models of a slot (dc_tracker_appearance_state) -> dict: "track_model" int32 [T, 3, 16] and "track_valid" int32
        [T] (zeros for a place that is free or has no valid model); "gallery_ids" int64 [64] and "gallery_age" int32 [64] (-1 = free
        entry), "gallery_model" int32 [64, 3, 16].  All empty with appearance off."""
        t = self.max_tracks
        out = {"track_model": np.zeros((t, 3, APPEARANCE_BINS), np.int32), "track_valid": np.zeros(t, np.int32),
               "gallery_ids": np.full(TRACK_GALLERY, -1, np.int64), "gallery_age": np.full(TRACK_GALLERY, -1, np.int32),
               "gallery_model": np.zeros((TRACK_GALLERY, 3, APPEARANCE_BINS), np.int32)}
        _check(_lib.dc_tracker_appearance_state(self._h, int(slot), *[out[k].ctypes.data_as(C.c_void_p) for k in
                                                                      ("track_model", "track_valid", "gallery_ids", "gallery_age", "gallery_model")]))
        return out

    def smooth_state(self, slot=0):
        """Where the filters of a slot expect every joint now (dc_tracker_smooth_state) -> dict: "poses" float64 [T, J, 3], the filter's
        position moved on by its rate over the updates since the joint was last observed, with the last observed score, and "gap" int32
        [T, J], those updates; zeros and -1 where the filter holds nothing (always, with smoothing off)."""
        t, j = self.max_tracks, self.n_joints
        out = {"poses": np.zeros((t, j, 3), np.float64), "gap": np.full((t, j), -1, np.int32)}
        _check(_lib.dc_tracker_smooth_state(self._h, int(slot), out["poses"].ctypes.data_as(C.c_void_p), out["gap"].ctypes.data_as(C.c_void_p)))
        return out


def smooth_params(smooth):
    """A `smooth=` argument / a `smoothing` value -> the dict of the four parameters, or None for off.  None and False are off, True is
    SMOOTH_DEFAULTS (PLACEHOLDERS, not tuned on real video), a dict overrides some of them.  The values themselves are checked by the
    library (dc_tracker_set_smoothing)."""
    if smooth is None or smooth is False:
        return None
    if smooth is True:
        return dict(SMOOTH_DEFAULTS)
    if not isinstance(smooth, dict):
        raise TypeError("smooth must be None, True or a dict of %s, got %r" % (sorted(SMOOTH_DEFAULTS), smooth))
    unknown = sorted(set(smooth) - set(SMOOTH_DEFAULTS))
    if unknown:
        raise ValueError("smooth: unknown keys %r (known: %s)" % (unknown, sorted(SMOOTH_DEFAULTS)))
    return dict(SMOOTH_DEFAULTS, **smooth)


def _slot_map(slot_of, nb):
    """slot_of of a tracked call -> int32 [nb] (the library checks the values)."""
    m = np.ascontiguousarray(slot_of, dtype=np.int32).reshape(-1)
    if m.shape[0] != nb:
        raise ValueError("slot_of must hold one slot per image: %d slots for %d images" % (m.shape[0], nb))
    return m


def completion_params(complete):
    """A `complete=` argument / a `completion` value -> the dict of the three parameters, or None for off.  None and False are off, True
    is COMPLETE_DEFAULTS, a dict overrides some of them.  The values themselves are checked by the library (dc_net_set_completion)."""
    if complete is None or complete is False:
        return None
    if complete is True:
        return dict(COMPLETE_DEFAULTS)
    if not isinstance(complete, dict):
        raise TypeError("complete must be None, True or a dict of %s, got %r" % (sorted(COMPLETE_DEFAULTS), complete))
    unknown = sorted(set(complete) - set(COMPLETE_DEFAULTS))
    if unknown:
        raise ValueError("complete: unknown keys %r (known: %s)" % (unknown, sorted(COMPLETE_DEFAULTS)))
    return dict(COMPLETE_DEFAULTS, **complete)


def dedupe_params(dedupe):
    """A `dedupe=` argument / a `dedupe` value -> the dict of the five parameters, or None for off.  None and False are off, True is
    DEDUPE_DEFAULTS (PLACEHOLDERS, not tuned on real images), a dict overrides some of them.  The values themselves are checked by the
    library (dc_net_set_dedupe)."""
    if dedupe is None or dedupe is False:
        return None
    if dedupe is True:
        return dict(DEDUPE_DEFAULTS)
    if not isinstance(dedupe, dict):
        raise TypeError("dedupe must be None, True or a dict of %s, got %r" % (sorted(DEDUPE_DEFAULTS), dedupe))
    unknown = sorted(set(dedupe) - set(DEDUPE_DEFAULTS))
    if unknown:
        raise ValueError("dedupe: unknown keys %r (known: %s)" % (unknown, sorted(DEDUPE_DEFAULTS)))
    return dict(DEDUPE_DEFAULTS, **dedupe)


def _dedupe_struct(d):
    """The dict of `dedupe_params` -> (DedupeParams, what must stay alive beside it)."""
    try:
        sig = None if d["sigma"] is None else np.ascontiguousarray(d["sigma"], dtype=np.float64).reshape(-1)
        q = DedupeParams(1, float(d["max_dist"]), int(d["min_common"]), float(d["min_size"]), None if sig is None else sig.ctypes.data,
                         0 if sig is None else int(sig.shape[0]), int(bool(d["absorb"])))
    except (TypeError, ValueError) as e:
        raise ValueError("dedupe: max_dist and min_size must be numbers, min_common a whole number, sigma numbers or None (%s)" % (e,))
    return q, sig


def dedupe_people(people, n_people=None, cand=None, dedupe=True, return_maps=False):
    """Stage E of the people assembly alone, on poses from anywhere (dc_dedupe_people; the rule: include/deepcut_hip.h): the people a
    better-scored kept person is the same as, by the tracker's distance, are suppressed.  This is how top-down poses of `forward_boxes`
    (overlapping boxes give the same person twice) are cleaned before `Tracker.update`.
    people: [nb, P, J, 3] float64 (x, y, score; a joint is held when its score > 0) with n_people [nb] of them valid per image, or a
    list of nb arrays [m_b, J, 3], as `Tracker.update` takes them.  cand: int32 [nb, P, J] (or a list of [m_b, J]) as `assemble_people`
    returns it, or None: a joint then counts as assigned exactly when it is held.  dedupe: True (DEDUPE_DEFAULTS: PLACEHOLDERS, not
    tuned on real images) or a dict of some of max_dist, min_common, min_size, sigma, absorb.
    -> one dict per image: {"people": [m, J, 3], "cand": int32 [m, J]}, the kept people in input order; with return_maps also
    "kept_from": int32 [m] (the input index of every kept person) and "suppressed_by": int32 [n_b] (per input person the input index of
    the kept person that suppressed it, -1 = kept).  Needs GPU mode."""
    d = dedupe_params(dedupe)
    if d is None:
        raise ValueError("dedupe_people needs parameters: dedupe=True or a dict, not %r" % (dedupe,))
    q, _sig = _dedupe_struct(d)
    if n_people is None and not (isinstance(people, np.ndarray) and people.ndim == 4):
        arrs = [np.asarray(a, np.float64) for a in people]
        if not arrs:
            return []
        j = max([a.shape[1] for a in arrs if a.ndim == 3] or [0])
        if j < 1 or any(a.ndim != 3 or a.shape[1:] != (j, 3) for a in arrs):
            raise ValueError("people must be arrays [m, J, 3] of one J, got shapes %s" % ([a.shape for a in arrs],))
        n = np.array([a.shape[0] for a in arrs], np.int32)
        ppl = np.zeros((len(arrs), max(1, int(n.max())), j, 3), np.float64)
        cnd = None if cand is None else np.full(ppl.shape[:3], -1, np.int32)
        for b, a in enumerate(arrs):
            ppl[b, :a.shape[0]] = a
            if cnd is not None:
                cnd[b, :a.shape[0]] = np.asarray(cand[b], np.int32).reshape(a.shape[0], j)
    else:
        ppl = np.ascontiguousarray(people, dtype=np.float64)
        if ppl.ndim != 4 or ppl.shape[3] != 3:
            raise ValueError("people must be [nb, P, J, 3] (x, y, score), got shape %s" % (ppl.shape,))
        n = np.full(ppl.shape[0], ppl.shape[1], np.int32) if n_people is None else np.ascontiguousarray(n_people, dtype=np.int32).reshape(-1)
        if n.shape[0] != ppl.shape[0]:
            raise ValueError("n_people must hold one count per image: %d counts for %d images" % (n.shape[0], ppl.shape[0]))
        cnd = None if cand is None else np.ascontiguousarray(cand, dtype=np.int32)
        if cnd is not None and cnd.shape != ppl.shape[:3]:
            raise ValueError("cand must be %s like people, got shape %s" % (ppl.shape[:3], cnd.shape))
    nb, p, j = ppl.shape[:3]
    n_out = np.zeros(nb, np.int32)
    ppl_out, cand_out = np.zeros((nb, p, j, 3), np.float64), np.full((nb, p, j), -1, np.int32)
    kept_from, by = np.full((nb, p), -1, np.int32), np.full((nb, p), -1, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(_lib.dc_dedupe_people(C.byref(q), nb, p, j, ptr(n), ptr(ppl), ptr(cnd), ptr(n_out), ptr(ppl_out), ptr(cand_out), ptr(kept_from),
                                 ptr(by)))
    out = []
    for b in range(nb):
        m = int(n_out[b])
        e = {"people": ppl_out[b, :m].copy(), "cand": cand_out[b, :m].copy()}
        if return_maps:
            e["kept_from"], e["suppressed_by"] = kept_from[b, :m].copy(), by[b, :int(n[b])].copy()
        out.append(e)
    return out


# ---- drawing people into frames (dc_draw_people; the rule: include/deepcut_hip.h — this project's own, the reference has none) -------
# By-joint colours: the reference demo's 14-colour table (R, G, B), one per MPII joint.
DRAW_JOINT_COLORS = tuple([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 245, 255), (255, 131, 250), (255, 255, 0)] * 2 + [(0, 0, 0), (255, 255, 255)])
# By-person colours (R, G, B), indexed by id.  A PLACEHOLDER: twelve hues chosen by eye to stay apart from their neighbours, not tested
# for legibility on real video; pass palette= for another.
DRAW_ID_COLORS = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
                  (210, 245, 60), (250, 190, 190), (0, 128, 128), (170, 110, 40))
_DRAW_MODES = {"id": 0, "joint": 1}  # DC_DRAW_BY_PERSON, DC_DRAW_BY_JOINT


def draw_limits():
    """-> (tile_w, tile_h, chunk): the tile a workgroup of the drawing kernel covers, and the primitives it stages at a time."""
    v = [C.c_int() for _ in range(3)]
    _check(_lib.dc_draw_limits(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def draw_coefficients(matrix="bt601", range="limited"):
    """((yr, yg, yb), (cb_r, cb_g, cb_b), (cr_r, cr_g, cr_b), y0) of the forward colour rule the NV12 overlay converts its colours by
    (include/deepcut_hip.h, dc_draw_people): the counterpart of `csc_coefficients`, computed in double, rounded to nearest."""
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[_CSC_MATRIX[matrix]]
    kg = 1.0 - kr - kb
    full = bool(_CSC_RANGE[range])
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    r = lambda v: int(np.rint(v))  # noqa: E731
    return (tuple(r(65536.0 * k / sy) for k in (kr, kg, kb)),
            tuple(r(65536.0 * k / (2.0 * (1.0 - kb)) / sc) for k in (-kr, -kg, 1.0 - kb)),
            tuple(r(65536.0 * k / (2.0 * (1.0 - kr)) / sc) for k in (1.0 - kr, -kg, -kb)), 0 if full else 16)


def _per_image(v, dtype, tail):
    """v -> [nb, P] + tail, from the [nb, P, ...] array, the single image's [m, ...] array or a list of nb arrays [m_b, ...]."""
    if not isinstance(v, np.ndarray):
        try:  # a list of numbers or of equal arrays is the array itself; a ragged one stays a list of per-image arrays
            a = np.asarray(v, dtype)
            v = a if a.ndim in (1 + len(tail), 2 + len(tail)) else v
        except ValueError:
            pass
    if isinstance(v, np.ndarray) and v.ndim == 2 + len(tail):
        return np.ascontiguousarray(v, dtype=dtype)
    if isinstance(v, np.ndarray) and v.ndim == 1 + len(tail):
        v = [v]
    rows = [np.asarray(a, dtype).reshape((-1,) + tail) for a in v]
    out = np.zeros((len(rows), max([1] + [a.shape[0] for a in rows])) + tail, dtype)
    for b, a in enumerate(rows):
        out[b, :a.shape[0]] = a
    return out


def _frames_and_people(frames, people, n_people, writable=True):
    """What `draw_people` and `redact_people` take as frames and people -> (dc_frame[nb], nb, h, w, is_device, what to keep alive,
    people float64 [nb, P, J, 3], n_people int32 [nb], P, J).  writable=False (`describe_people`): the frames are only read."""
    arr, nb, h, w, is_device, keep = _writable_frames(frames, writable)
    if isinstance(people, np.ndarray) and people.ndim in (3, 4):
        if people.shape[-1] != 3:
            raise ValueError("people must be [m, J, 3] or [nb, P, J, 3] (x, y, score), got shape %s" % (people.shape,))
        j = int(people.shape[-2])
        if n_people is None:
            n_people = [people.shape[0]] if people.ndim == 3 else [people.shape[1]] * people.shape[0]
    else:
        rows = [np.asarray(a, np.float64) for a in people]
        if not rows or any(a.ndim != 3 or a.shape[1:] != rows[0].shape[1:] or a.shape[2] != 3 for a in rows):
            raise ValueError("people must be arrays [m, J, 3] of one J, got shapes %s" % ([a.shape for a in rows],))
        j = int(rows[0].shape[1])
        if n_people is None:
            n_people = [a.shape[0] for a in rows]
        people = rows
    ppl = _per_image(people, np.float64, (j, 3))
    n = np.ascontiguousarray(n_people, dtype=np.int32).reshape(-1)
    if ppl.shape[0] != nb or n.shape[0] != nb:
        raise ValueError("people and n_people must hold one entry per frame: %d and %d for %d frames" % (ppl.shape[0], n.shape[0], nb))
    p = int(ppl.shape[1])
    if p < 1:
        ppl, p = np.zeros((nb, 1, j, 3), np.float64), 1
    return arr, nb, h, w, is_device, keep, ppl, n, p, j


def _edges_array(edges):
    """edges of `draw_people` and `redact_people` -> int32 [E, 2] (None: no limbs)."""
    e = np.zeros((0, 2), np.int32) if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError("edges must be [E, 2] joints, got shape %s" % (e.shape,))
    return e


def _palette_array(palette):
    """A palette of `draw_people` and `draw_heatmap` -> uint8 [n, 3]."""
    pal = np.ascontiguousarray(palette, dtype=np.uint8)
    if pal.ndim != 2 or pal.shape[1] != 3:
        raise ValueError("palette must be [n, 3] R, G, B, got shape %s" % (pal.shape,))
    return pal


def _stream_arg(stream):
    """The `stream` of the calls that write into frames, as the library takes it."""
    return None if stream is None else C.c_void_p(int(stream))


def _draw_style_struct(edges=None, joint_radius=4.0, limb_radius=2.0, alpha=256, alpha_filled=128, min_score=0.0, color="id", palette=None,
                       untracked=(128, 128, 128)):
    """The style arguments of `draw_people` -> (DrawStyle, the arrays it points into).  Names and shapes are checked here; the values are
    the library's to refuse."""
    if color not in _DRAW_MODES:
        raise ValueError("color must be one of %s, got %r" % (sorted(_DRAW_MODES), color))
    if palette is None:
        palette = DRAW_ID_COLORS if color == "id" else DRAW_JOINT_COLORS
    pal = _palette_array(palette)
    e = _edges_array(edges)
    st = DrawStyle()
    st.n_edges, st.edges = int(e.shape[0]), e.ctypes.data if e.shape[0] else None
    st.joint_radius, st.limb_radius = float(joint_radius), float(limb_radius)
    st.alpha, st.alpha_filled, st.min_score = int(alpha), int(alpha_filled), float(min_score)
    st.color_mode, st.palette, st.n_palette = _DRAW_MODES[color], pal.ctypes.data if pal.shape[0] else None, int(pal.shape[0])
    st.untracked[:] = [int(v) for v in untracked]
    return st, (pal, e)


def draw_people(frames, people, n_people=None, ids=None, cand=None, edges=None, joint_radius=4.0, limb_radius=2.0, alpha=256, alpha_filled=128,
                min_score=0.0, color="id", palette=None, untracked=(128, 128, 128), stream=None):
    """Skeletons blended into frames IN PLACE on the device (dc_draw_people; the rule — integer only, this project's own: the reference
    draws with matplotlib and states none — is in include/deepcut_hip.h): joints as discs of joint_radius pixels, the limbs `edges`
    ([E, 2] joints, None = joints only) as capsules of limb_radius, people in index order, of a person the limbs and then the joints.
    frames: a `Frame` (NV12 or BGR24, host or device), a list of them (one size, format, matrix and range), or a uint8 [H, W, 3] BGR
    array, wrapped like `Frame.bgr`.  Host arrays are drawn in place and must be writable (ValueError otherwise).
    people: float64 [m, J, 3] (one frame) or [nb, P, J, 3] with n_people [nb], or a list of nb arrays [m_b, J, 3], as `dedupe_people`
    takes them; cand: int32 of the same leading shape or None — joints it marks filled (-2) or bridged (-3), and limbs that end in one,
    are blended with alpha_filled instead of alpha (both 0..256, 256 = opaque); ids: int64 [nb, P] / [m] or None.
    color: "id" — palette[id % len] (the person's index without ids; `untracked` for id < 0), palette None = DRAW_ID_COLORS (a
    PLACEHOLDER) — or "joint" — palette[j % len] for joint j and for a limb ending in j, None = DRAW_JOINT_COLORS.  Colours are R, G, B.
    stream: a HIP stream for device frames (None: the library's own).  The call returns when the drawing is complete.  Needs GPU mode."""
    arr, nb, h, w, is_device, _keep, ppl, n, p, j = _frames_and_people(frames, people, n_people)
    cnd = None if cand is None else _per_image(cand, np.int32, (j,))
    if cnd is not None and cnd.shape != ppl.shape[:3]:
        raise ValueError("cand must be %s like people, got shape %s" % (ppl.shape[:3], cnd.shape))
    idv = None if ids is None else _per_image(ids, np.int64, ())
    if idv is not None and idv.shape != ppl.shape[:2]:
        raise ValueError("ids must be %s like people, got shape %s" % (ppl.shape[:2], idv.shape))
    st, _alive = _draw_style_struct(edges, joint_radius, limb_radius, alpha, alpha_filled, min_score, color, palette, untracked)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(_lib.dc_draw_people(arr, nb, h, w, int(is_device), p, j, ptr(n), ptr(ppl), ptr(cnd), ptr(idv), C.byref(st), _stream_arg(stream)))


# ---- redacting people in frames (dc_redact_people; the rule: include/deepcut_hip.h — this project's own, the reference has none) -------
# PLACEHOLDERS, NOT TUNED ON REAL VIDEO: override them.  The head disc's radius is head_scale times the distance neck - head top, a body
# primitive's body_scale times the larger side of the person's bounding box; both are kept within [min_radius, max_radius] pixels (the
# body's within 64 pixels as well).
REDACT_DEFAULTS = {"head_scale": 0.75, "body_scale": 0.06, "min_radius": 4.0, "max_radius": 256.0}
_REDACT_REGIONS = {"head": 0, "body": 1, "head_or_body": 2}  # DC_REDACT_HEAD, DC_REDACT_BODY, DC_REDACT_HEAD_OR_BODY
_REDACT_EFFECTS = {"mosaic": 0, "fill": 1}  # DC_REDACT_MOSAIC, DC_REDACT_FILL


def redact_select(ids, only_ids=None, keep_ids=None, select=None):
    """-> uint8 array shaped like `ids` (or None: everyone): who `redact_people` redacts.  only_ids: only the people with one of these
    ids; keep_ids: everybody but the people with one of these ids (they stay visible); select: a mask of the caller's, combined with
    the two by AND.  only_ids / keep_ids need `ids`."""
    if only_ids is None and keep_ids is None:
        return None if select is None else (np.asarray(select) != 0).astype(np.uint8)
    if ids is None:
        raise ValueError("only_ids / keep_ids choose people by id: ids is needed")
    ids = np.asarray(ids, np.int64)
    sel = np.ones(ids.shape, bool) if select is None else np.asarray(select) != 0
    if sel.shape != ids.shape:
        raise ValueError("select must be %s like ids, got shape %s" % (ids.shape, sel.shape))
    if only_ids is not None:
        sel = sel & np.isin(ids, np.asarray(list(only_ids), np.int64))
    if keep_ids is not None:
        sel = sel & ~np.isin(ids, np.asarray(list(keep_ids), np.int64))
    return sel.astype(np.uint8)


def _redact_style_struct(region="head", head=None, edges=None, head_scale=REDACT_DEFAULTS["head_scale"], body_scale=REDACT_DEFAULTS["body_scale"],
                         min_radius=REDACT_DEFAULTS["min_radius"], max_radius=REDACT_DEFAULTS["max_radius"], min_score=0.0, effect="mosaic",
                         block=8, fill=(0, 0, 0)):
    """The style arguments of `redact_people` -> (RedactStyle, the arrays it points into).  Names and shapes are checked here; the values
    are the library's to refuse."""
    if region not in _REDACT_REGIONS:
        raise ValueError("region must be one of %s, got %r" % (sorted(_REDACT_REGIONS), region))
    if effect not in _REDACT_EFFECTS:
        raise ValueError("effect must be one of %s, got %r" % (sorted(_REDACT_EFFECTS), effect))
    if head is None or len(head) != 2:
        raise ValueError("head must name the joint pair (neck, head top), got %r (pose.redact_people has the MPII one)" % (head,))
    e = _edges_array(edges)
    st = RedactStyle()
    st.region, st.head_a, st.head_b = _REDACT_REGIONS[region], int(head[0]), int(head[1])
    st.head_scale, st.body_scale, st.min_radius, st.max_radius = float(head_scale), float(body_scale), float(min_radius), float(max_radius)
    st.min_score, st.n_edges, st.edges = float(min_score), int(e.shape[0]), e.ctypes.data if e.shape[0] else None
    st.effect, st.block = _REDACT_EFFECTS[effect], int(block)
    st.fill[:] = [int(v) for v in fill]
    return st, (e,)


def redact_people(frames, people, n_people=None, select=None, ids=None, only_ids=None, keep_ids=None, region="head", head=None, edges=None,
                  head_scale=REDACT_DEFAULTS["head_scale"], body_scale=REDACT_DEFAULTS["body_scale"], min_radius=REDACT_DEFAULTS["min_radius"],
                  max_radius=REDACT_DEFAULTS["max_radius"], min_score=0.0, effect="mosaic", block=8, fill=(0, 0, 0), stream=None):
    """Regions derived from people's joints replaced by a mosaic or a solid colour, IN PLACE on the device (dc_redact_people; the rule —
    integer only, this project's own: the reference has nothing of the kind — is in include/deepcut_hip.h).  frames and people /
    n_people: as `draw_people` takes them.
    region: "head" — a disc around the middle of the joint pair head = (neck, head top), of radius head_scale times their distance;
    "body" — that disc, the limbs `edges` ([E, 2] joints, None = none) as capsules and every joint as a disc, of radius body_scale times
    the larger side of the person's bounding box (64 pixels at the most); "head_or_body" — the head disc where the pair is there, else
    the body.  Radii are kept within [min_radius, max_radius] pixels.  The scale and radius defaults (REDACT_DEFAULTS) are PLACEHOLDERS,
    not tuned on real video.  Only joints with score > min_score count.
    effect: "mosaic" — every block x block pixel block (2, 4, 8, 16 or 32; the grid starts at pixel (0, 0)) that holds a covered pixel
    becomes its mean — or "fill" — it becomes `fill` (R, G, B).  A mosaic with small blocks is NOT a privacy guarantee.
    Who: everyone, or the people `select` (like ids, non-zero = redact) marks; only_ids / keep_ids (with ids: int64 [nb, P] / [m]) choose
    by id — only these, or everybody but these (`redact_select`).
    -> `redacted`, int32 shaped like ids ([m] for one frame's [m, J, 3], else [nb, P]): 1 where a region was made for the person.  A
    person whose head pair is not there is NOT redacted by region "head": look at what comes back.
    stream: a HIP stream for device frames (None: the library's own).  The call returns when the redaction is complete.  Needs GPU mode."""
    single = isinstance(people, np.ndarray) and people.ndim == 3
    arr, nb, h, w, is_device, _keep, ppl, n, p, j = _frames_and_people(frames, people, n_people)
    idv = None if ids is None else _per_image(ids, np.int64, ())
    if idv is not None and idv.shape != ppl.shape[:2]:
        raise ValueError("ids must be %s like people, got shape %s" % (ppl.shape[:2], idv.shape))
    sel = None if select is None else _per_image(select, np.uint8, ())
    if sel is not None and sel.shape != ppl.shape[:2]:
        raise ValueError("select must be %s like people, got shape %s" % (ppl.shape[:2], sel.shape))
    sel = redact_select(idv, only_ids, keep_ids, sel)
    st, _alive = _redact_style_struct(region, head, edges, head_scale, body_scale, min_radius, max_radius, min_score, effect, block, fill)
    out = np.zeros((nb, p), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(_lib.dc_redact_people(arr, nb, h, w, int(is_device), p, j, ptr(n), ptr(ppl), ptr(sel), C.byref(st), ptr(out), _stream_arg(stream)))
    return out[0, :people.shape[0]] if single else out


# ---- appearance descriptors of people (dc_describe_people; the rule: include/deepcut_hip.h — this project's own, the reference has none) --
# PLACEHOLDERS, NOT TUNED ON REAL VIDEO: override them.  A capsule's radius is `scale` times the larger side of the person's bounding
# box, at least min_radius pixels (and 64 pixels at the most).
# Of the tracker's appearance steps (`Tracker.appearance`): a descriptor needs min_pixels region pixels, a new observation weighs
# alpha256 / 256 in a track's model, a dissimilarity of at most reid_max (of 12288) re-identifies, a freed track with at least min_hits hits
# waits max_age updates in the gallery.  PLACEHOLDERS, NOT TUNED ON REAL VIDEO, like the rest.
APPEARANCE_DEFAULTS = {"scale": 0.04, "min_radius": 2.0, "min_score": 0.0, "min_pixels": 64, "alpha256": 64, "reid_max": 4096, "max_age": 300,
                       "min_hits": 5}
APPEARANCE_BINS = 16  # DC_APPEARANCE_BINS
TRACK_GALLERY = 64  # DC_TRACK_GALLERY
_APPEARANCE_TRACK_KEYS = ("min_pixels", "alpha256", "reid_max", "max_age", "min_hits")  # dc_track_appearance_params, in its order


def appearance_params(appearance, keys=_APPEARANCE_TRACK_KEYS):
    """An `appearance=` argument / an `appearance` value -> the dict of the parameters `keys` (the tracker's five by default), or None
    for off.  None and False are off, True is APPEARANCE_DEFAULTS (PLACEHOLDERS, not tuned on real video), a dict overrides some of them.
    The values themselves are checked by the library (dc_tracker_set_appearance, dc_describe_people)."""
    if appearance is None or appearance is False:
        return None
    if appearance is True:
        appearance = {}
    if not isinstance(appearance, dict):
        raise TypeError("appearance must be None, True or a dict of %s, got %r" % (sorted(keys), appearance))
    unknown = sorted(set(appearance) - set(keys))
    if unknown:
        raise ValueError("appearance: unknown keys %r (known: %s)" % (unknown, sorted(keys)))
    return dict({k: APPEARANCE_DEFAULTS[k] for k in keys if k in APPEARANCE_DEFAULTS}, **appearance)


def describe_people(frames, people, n_people=None, edges=None, scale=APPEARANCE_DEFAULTS["scale"], min_radius=APPEARANCE_DEFAULTS["min_radius"],
                    min_score=APPEARANCE_DEFAULTS["min_score"], stream=None):
    """What people look like, counted from frames on the device (dc_describe_people; the rule — integer only, this project's own: the
    reference stops at the maps — is in include/deepcut_hip.h): per person, the pixels under the capsules of the limbs `edges` ([E, 2]
    joints: the torso's — `pose.describe_people` has the MPII ones; None = none, so all zeros), of radius `scale` times the larger side
    of the person's bounding box and at least min_radius pixels, and per channel (BGR24: B, G, R; NV12: Y, Cb, Cr) a histogram of their
    bytes in 16 bins of 16 values.  The defaults (APPEARANCE_DEFAULTS) are PLACEHOLDERS, not tuned on real video.  Only joints with
    score > min_score count.
    frames and people / n_people: as `redact_people` takes them, but the frames are ONLY READ and need not be writable.
    -> int32 [m, 3, 16] for one frame's [m, J, 3], else [nb, P, 3, 16]: each channel's counts sum to the pixels of the person's region,
    0 for a person without a held limb or wholly outside the frame.
    stream: a HIP stream for device frames (None: the library's own).  The call returns when the counts are complete.  Needs GPU mode."""
    single = isinstance(people, np.ndarray) and people.ndim == 3
    arr, nb, h, w, is_device, _keep, ppl, n, p, j = _frames_and_people(frames, people, n_people, writable=False)
    e = _edges_array(edges)
    st = AppearanceStyle()
    st.size, st.n_edges, st.edges = C.sizeof(AppearanceStyle), int(e.shape[0]), e.ctypes.data if e.shape[0] else None
    st.scale, st.min_radius, st.min_score = float(scale), float(min_radius), float(min_score)
    out = np.zeros((nb, p, 3, APPEARANCE_BINS), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(_lib.dc_describe_people(arr, nb, h, w, int(is_device), p, j, ptr(n), ptr(ppl), C.byref(st), ptr(out), _stream_arg(stream)))
    return out[0, :people.shape[0]] if single else out


# ---- labelling people in frames (dc_label_people; the rule: include/deepcut_hip.h — this project's own, the reference has none) --------
LABEL_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:/%+_?"  # the font's set, in the table's order; lower case folds to upper case
LABEL_MAX_CHARS = 24  # DC_LABEL_MAX_CHARS: a text holds at most 23 characters


def _label_font():
    font = {}
    for ch in LABEL_CHARS:
        rows = (C.c_ubyte * 7)()
        _check(_lib.dc_label_font(ord(ch), C.byref(rows)))
        font[ch] = tuple(int(v) for v in rows)
    return font


# The built-in 5 x 7 font as the kernels read it (dc_label_font): {character: 7 rows, bit 4 the leftmost column}.  A PLACEHOLDER.
LABEL_FONT = _label_font()
# PLACEHOLDERS, not tested for legibility on real video: override them.  palette None = DRAW_ID_COLORS.
LABEL_DEFAULTS = {"scale": 2, "gap": 2, "anchor": None, "prefix": "", "alpha_text": 256, "alpha_plate": 160, "min_score": 0.0, "color": "plate",
                  "palette": None, "text_color": (255, 255, 255), "plate_color": (0, 0, 0)}
_LABEL_MODES = {"plate": 0, "text": 1}  # DC_LABEL_PLATE_BY_PERSON, DC_LABEL_TEXT_BY_PERSON


def _label_text(text, what, limit):
    """A text of `label_people` -> its bytes, upper-cased; ValueError naming a character outside the set or a text that is too long."""
    if not isinstance(text, str):
        raise ValueError("%s must be a str, got %r" % (what, text))
    up = text.upper()
    for i, ch in enumerate(up):
        if ch not in LABEL_CHARS:
            raise ValueError("%s: character %r at %d is outside the label set %r" % (what, text[i], i, LABEL_CHARS))
    if len(up) > limit:
        raise ValueError("%s: %r holds %d characters, at most %d are taken" % (what, text, len(up), limit))
    return up.encode("ascii")


def _label_style_struct(scale=LABEL_DEFAULTS["scale"], gap=LABEL_DEFAULTS["gap"], anchor=LABEL_DEFAULTS["anchor"], prefix=LABEL_DEFAULTS["prefix"],
                        alpha_text=LABEL_DEFAULTS["alpha_text"], alpha_plate=LABEL_DEFAULTS["alpha_plate"], min_score=LABEL_DEFAULTS["min_score"],
                        color=LABEL_DEFAULTS["color"], palette=LABEL_DEFAULTS["palette"], text_color=LABEL_DEFAULTS["text_color"],
                        plate_color=LABEL_DEFAULTS["plate_color"]):
    """The style arguments of `label_people` -> (LabelStyle, the arrays it points into).  Names, shapes and the prefix's characters are
    checked here; the values are the library's to refuse."""
    if color not in _LABEL_MODES:
        raise ValueError("color must be one of %s, got %r" % (sorted(_LABEL_MODES), color))
    pal = _palette_array(DRAW_ID_COLORS if palette is None else palette)
    st = LabelStyle()
    st.scale, st.gap, st.anchor_joint = int(scale), int(gap), -1 if anchor is None else int(anchor)
    st.alpha_text, st.alpha_plate, st.min_score = int(alpha_text), int(alpha_plate), float(min_score)
    st.color_mode, st.palette, st.n_palette = _LABEL_MODES[color], pal.ctypes.data if pal.shape[0] else None, int(pal.shape[0])
    st.text_color[:] = [int(v) for v in text_color]
    st.plate_color[:] = [int(v) for v in plate_color]
    st.prefix = _label_text(prefix, "prefix", 4)
    return st, (pal,)


def _label_texts(texts, nb, p):
    """texts of `label_people` — a list of str (one frame) or a list of nb such lists; None or "" = the made text — -> bytes [nb, P, 24]."""
    if texts is None:
        return None
    rows = list(texts)
    if nb == 1 and (not rows or isinstance(rows[0], str) or rows[0] is None):
        rows = [rows]
    if len(rows) != nb:
        raise ValueError("texts must hold one list per frame: %d for %d frames" % (len(rows), nb))
    out = np.zeros((nb, p, LABEL_MAX_CHARS), np.uint8)
    for b, row in enumerate(rows):
        row = list(row)
        if len(row) > p:
            raise ValueError("texts[%d] holds %d texts for %d people" % (b, len(row), p))
        for k, t in enumerate(row):
            v = _label_text("" if t is None else t, "texts[%d][%d]" % (b, k), LABEL_MAX_CHARS - 1)
            out[b, k, :len(v)] = np.frombuffer(v, np.uint8)
    return out


def label_people(frames, people, n_people=None, ids=None, texts=None, scale=LABEL_DEFAULTS["scale"], gap=LABEL_DEFAULTS["gap"],
                 anchor=LABEL_DEFAULTS["anchor"], prefix=LABEL_DEFAULTS["prefix"], alpha_text=LABEL_DEFAULTS["alpha_text"],
                 alpha_plate=LABEL_DEFAULTS["alpha_plate"], min_score=LABEL_DEFAULTS["min_score"], color=LABEL_DEFAULTS["color"],
                 palette=LABEL_DEFAULTS["palette"], text_color=LABEL_DEFAULTS["text_color"], plate_color=LABEL_DEFAULTS["plate_color"],
                 stream=None):
    """People's ids written into frames IN PLACE on the device (dc_label_people; the rule — integer only, this project's own: the
    reference labels nothing — is in include/deepcut_hip.h): per person `prefix` (at most 4 characters) and the id in decimal, in the
    built-in 5 x 7 font (LABEL_FONT) at `scale` (1..8), on a plate, `gap` pixels above the joint `anchor` (centred on it) or, with
    anchor None or that joint not held, above the upper left corner of the person's bounding box; pulled into the frame where it fits.
    frames, people, n_people, ids: as `draw_people` takes them (without ids the person's index is written; an id < 0 gets no label).
    texts: a list of str per frame (a plain list for one frame), upper-cased here; a non-empty one replaces the person's made text.
    A character outside LABEL_CHARS, or a text of more than 23 characters, is a ValueError here, before any call into the library.
    color: "plate" — the plate is palette[id % len] and the text text_color — or "text" — the text takes the palette colour and the
    plate plate_color; palette None = DRAW_ID_COLORS.  alpha_text / alpha_plate: 0..256 (0: that layer is not made).  The defaults
    (LABEL_DEFAULTS) are PLACEHOLDERS.  stream: as `draw_people`.  The call returns when the frames are written.  Needs GPU mode."""
    arr, nb, h, w, is_device, _keep, ppl, n, p, j = _frames_and_people(frames, people, n_people)
    idv = None if ids is None else _per_image(ids, np.int64, ())
    if idv is not None and idv.shape != ppl.shape[:2]:
        raise ValueError("ids must be %s like people, got shape %s" % (ppl.shape[:2], idv.shape))
    txt = _label_texts(texts, nb, p)
    st, _alive = _label_style_struct(scale, gap, anchor, prefix, alpha_text, alpha_plate, min_score, color, palette, text_color, plate_color)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _check(_lib.dc_label_people(arr, nb, h, w, int(is_device), p, j, ptr(n), ptr(ppl), ptr(idv), ptr(txt), C.byref(st), _stream_arg(stream)))


def _label_overlay_struct(labels):
    """labels= of the device routes: True or a dict of the STYLE arguments of `label_people` -> (LabelStyle, what to keep alive).  `texts`
    and `stream` are refused: a text for a person cannot exist before the person does, and the route has its own stream."""
    style = {} if labels is True else dict(labels)
    for k in ("texts", "stream"):
        if style.pop(k, None) is not None:
            raise ValueError("%s cannot go with labels on this route: the labels are made on the device from the people it finds" % k)
    return _label_style_struct(**style)


def _overlay_styles_struct(dst, rst, lst, only, keep):
    """The styles of the two `_styles` entries -> (OverlayStyles, nothing more to keep alive than its parts)."""
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    st = OverlayStyles()
    st.size = C.sizeof(OverlayStyles)
    if dst is not None:
        st.draw = C.pointer(dst)
    if rst is not None:
        st.redact = C.pointer(rst)
    if lst is not None:
        st.labels = C.pointer(lst)
    st.only_ids, st.n_only = ptr(only), -1 if only is None else int(only.size)
    st.keep_ids, st.n_keep = ptr(keep), -1 if keep is None else int(keep.size)
    return st


# ---- overlays from people in device memory (dc_overlay_people_device, dc_net_track_frames_async_overlay) --------------------------------
def _overlay_args(draw, redact, have_ids, labels=None):
    """draw / redact: None or dicts of the STYLE arguments of `draw_people` / `redact_people` (a redact dict may carry only_ids /
    keep_ids) -> (DrawStyle or None, RedactStyle or None, only_ids int64 array or None, keep_ids likewise, what to keep alive).
    labels (checked by the caller, `_label_overlay_struct`) only makes a call without the two a good one."""
    if draw is None and redact is None and labels is None:
        raise ValueError("an overlay needs draw=, redact= or both — or labels=, alone or beside them")
    dst = rst = only = keep = None
    alive = []
    if redact is not None:
        r = dict(redact)
        if r.pop("select", None) is not None:
            raise ValueError("select is a mask over people, who do not exist before the call: choose them by only_ids / keep_ids")
        only, keep = r.pop("only_ids", None), r.pop("keep_ids", None)
        if (only is not None or keep is not None) and not have_ids:
            raise ValueError("only_ids / keep_ids choose people by id: ids is needed")
        only = None if only is None else np.ascontiguousarray(list(only), dtype=np.int64).reshape(-1)
        keep = None if keep is None else np.ascontiguousarray(list(keep), dtype=np.int64).reshape(-1)
        rst, a = _redact_style_struct(**r)
        alive.append(a)
    if draw is not None:
        dst, a = _draw_style_struct(**dict(draw))
        alive.append(a)
    return dst, rst, only, keep, alive


def _overlay_c_args(dst, rst, only, keep):
    """... as the two entries take them: draw, redact, only_ids, n_only, keep_ids, n_keep."""
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return (None if dst is None else C.byref(dst), None if rst is None else C.byref(rst), ptr(only), -1 if only is None else int(only.size),
            ptr(keep), -1 if keep is None else int(keep.size))


def _device_pointer(a, name, dtype, shape):
    """A device array of the caller's (anything with data_ptr(), dtype and shape, a torch tensor for one; or None) -> its address."""
    if a is None:
        return None
    if not hasattr(a, "data_ptr"):
        raise ValueError("%s must be a device tensor (data_ptr(), shape), got %r" % (name, type(a).__name__))
    if tuple(a.shape) != tuple(shape) or dtype not in str(a.dtype) or (hasattr(a, "is_contiguous") and not a.is_contiguous()):
        raise ValueError("%s must be a contiguous %s device tensor of shape %s, got %s %s" % (name, dtype, tuple(shape), a.dtype, tuple(a.shape)))
    return C.c_void_p(int(a.data_ptr()))


def overlay_people_device(frames, people, n_people, cand=None, ids=None, draw=None, redact=None, redacted=None, stream=None, labels=None):
    """The bytes of `redact_people` then `draw_people` from people that are in DEVICE memory (dc_overlay_people_device): the primitives
    and the per-tile selection are made on the device, nothing of the poses travels.  frames: as `draw_people` takes them (host frames
    travel up and ALL travel back).  people: a float64 device tensor [nb, P, J, 3] (a torch tensor: anything with data_ptr(), dtype and
    shape); n_people: int32 [nb]; cand: int32 [nb, P, J] or None; ids: int64 [nb, P] or None; redacted: int32 [nb, P] or None, written by
    the redaction.  draw / redact: dicts of the style arguments of `draw_people` / `redact_people` (either may be None); a redact dict
    may carry only_ids / keep_ids (at most 256 each; they need ids) and no `select`.  stream: a HIP stream — with device frames the call
    then returns once everything is enqueued on it, and the tensors must stay alive until that stream has run; otherwise it waits.
    labels: None, True (LABEL_DEFAULTS) or a dict of the style arguments of `label_people` without `texts` and `stream`
    (dc_overlay_people_device_styles): the bytes of `label_people` behind the other two, the ids (or the people's indices) as text."""
    arr, nb, h, w, is_device, _keep = _writable_frames(frames)
    shape = tuple(getattr(people, "shape", ()))
    if len(shape) != 4 or shape[0] != nb or shape[3] != 3:
        raise ValueError("people must be a device tensor [nb = %d, P, J, 3], got shape %s" % (nb, shape))
    p, j = int(shape[1]), int(shape[2])
    lst, _lalive = (None, None) if labels is None else _label_overlay_struct(labels)
    dst, rst, only, keep, _alive = _overlay_args(draw, redact, ids is not None, lst)
    if lst is not None:
        styles = _overlay_styles_struct(dst, rst, lst, only, keep)
        _check(_lib.dc_overlay_people_device_styles(arr, nb, h, w, int(is_device), p, j, _device_pointer(n_people, "n_people", "int32", (nb,)),
                                                    _device_pointer(people, "people", "float64", shape),
                                                    _device_pointer(cand, "cand", "int32", (nb, p, j)), _device_pointer(ids, "ids", "int64", (nb, p)),
                                                    C.byref(styles), _device_pointer(redacted, "redacted", "int32", (nb, p)), _stream_arg(stream)))
        return
    _check(_lib.dc_overlay_people_device(arr, nb, h, w, int(is_device), p, j, _device_pointer(n_people, "n_people", "int32", (nb,)),
                                         _device_pointer(people, "people", "float64", shape), _device_pointer(cand, "cand", "int32", (nb, p, j)),
                                         _device_pointer(ids, "ids", "int64", (nb, p)), *_overlay_c_args(dst, rst, only, keep),
                                         _device_pointer(redacted, "redacted", "int32", (nb, p)), _stream_arg(stream)))


# ---- blending score maps into frames (dc_draw_heatmap; the rule: include/deepcut_hip.h — this project's own, the reference has none) ----
# The colour ramp of mode "max" (R, G, B by v >> 4).  A PLACEHOLDER: a plain black - blue - cyan - green - yellow - red - white ramp in
# six linear pieces, not tested for legibility on real video or for colour-blind readers; pass lut= for another.
def _heat_ramp():
    stops = ((0, 0, 0), (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0), (255, 255, 255))
    out = []
    for i in range(256):
        k, f = divmod(i * (len(stops) - 1), 255)
        a, b = stops[min(k, len(stops) - 1)], stops[min(k + 1, len(stops) - 1)]
        out.append(tuple((a[c] * (255 - f) + b[c] * f + 127) // 255 for c in range(3)))
    return tuple(out)


HEAT_LUT = _heat_ramp()
_HEAT_MODES = {"max": 0, "joints": 1}  # DC_HEAT_MAX, DC_HEAT_BY_JOINT
_HEAT_ALPHA_MODES = {"const": 0, "score": 1}  # DC_HEAT_ALPHA_CONST, DC_HEAT_ALPHA_SCORE


def _writable_frames(frames, writable=True):
    """frames of the calls that write into them (`draw_people`, `redact_people`, `draw_heatmap`) -> (dc_frame[nb], nb, h, w, is_device,
    what to keep alive).  writable=False: of a call that only reads them (`describe_people`), so a read-only host array will do."""
    fl = _frame_list(frames)
    if fl is None:
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            fl = [Frame.bgr(frames)]
        else:
            raise ValueError("frames must be a caffe.Frame, a non-empty list of them, or a uint8 [H, W, 3] BGR array")
    for i, f in enumerate(fl):
        for a in f._keep:
            if writable and isinstance(a, np.ndarray) and not a.flags.writeable:
                raise ValueError("frame %d: a host array that is drawn into must be writable" % i)
    arr, h, w, is_device = _frame_array(fl)
    return arr, len(fl), h, w, is_device, fl


def _heat_style(channels, joints, mode, alpha, alpha_mode, min_score, lut, palette):
    """-> (HeatStyle, the arrays it points into).  Only names and shapes are checked here; the values are the library's to refuse."""
    if mode not in _HEAT_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(_HEAT_MODES), mode))
    if alpha_mode not in _HEAT_ALPHA_MODES:
        raise ValueError("alpha_mode must be one of %s, got %r" % (sorted(_HEAT_ALPHA_MODES), alpha_mode))
    j = np.ascontiguousarray(np.arange(channels) if joints is None else joints, dtype=np.int32).reshape(-1)
    lt = np.ascontiguousarray(HEAT_LUT if lut is None else lut, dtype=np.uint8)
    if lt.shape != (256, 3):
        raise ValueError("lut must be [256, 3] R, G, B, got shape %s" % (lt.shape,))
    pal = _palette_array(DRAW_JOINT_COLORS if palette is None else palette)
    st = HeatStyle()
    st.n_joints, st.joints = int(j.shape[0]), j.ctypes.data if j.shape[0] else None
    st.mode, st.alpha, st.alpha_mode, st.min_score = _HEAT_MODES[mode], int(alpha), _HEAT_ALPHA_MODES[alpha_mode], float(min_score)
    st.lut, st.palette, st.n_palette = lt.ctypes.data, pal.ctypes.data if pal.shape[0] else None, int(pal.shape[0])
    return st, (j, lt, pal)


def draw_heatmap(frames, scores, scale, origin=(0.0, 0.0), joints=None, mode="max", alpha=128, alpha_mode="score", min_score=0.0, lut=None,
                 palette=None, stream=None):
    """A score map blended into frames IN PLACE on the device (dc_draw_heatmap; the rule — integer from the first quantisation on, this
    project's own: the reference's demo never shows a map — is in include/deepcut_hip.h).  The stride-8 map is brought onto the pixel grid
    bilinearly in 1/256 steps of 1/4096 scores.
    frames: as `draw_people` takes them.  scores: float32 [C, Hm, Wm] (one frame) or [nb, C, Hm, Wm], a host array — `net.blobs["prob"].data`,
    `NetGroup.fuse_maps(...)["prob"]` —, C <= 32.  scale: frame pixels x scale = network pixels (what the forward ran at), 1/64 .. 8;
    origin: (x, y) in frame pixels of the map's pixel 0 (a crop's corner).
    joints: the channels drawn, in order (None: all).  mode "max": the maximum over them, coloured by lut[v >> 4] ([256, 3] R, G, B; None =
    HEAT_LUT, a PLACEHOLDER ramp); "joints": every channel in list order over the ones before it, the k-th with palette[k % len] (None =
    DRAW_JOINT_COLORS).  alpha 0 .. 256 (256 = opaque), alpha_mode "const" or "score" (alpha times the score); only scores >= min_score
    (0 .. 1) are blended.  stream: a HIP stream for device frames (None: the library's own).  The call returns when the blending is
    complete.  Needs GPU mode."""
    arr, nb, h, w, is_device, _keep = _writable_frames(frames)
    s = np.ascontiguousarray(scores, dtype=np.float32)
    if s.ndim == 3:
        s = s[None]
    if s.ndim != 4 or s.shape[0] != nb:
        raise ValueError("scores must be [C, Hm, Wm] or [nb, C, Hm, Wm] with one map per frame: shape %s for %d frame(s)" % (s.shape, nb))
    st, _arrays = _heat_style(s.shape[1], joints, mode, alpha, alpha_mode, min_score, lut, palette)
    g = HeatGeometry(float(scale), float(origin[0]), float(origin[1]))
    _check(_lib.dc_draw_heatmap(arr, nb, h, w, int(is_device), s.ctypes.data_as(C.c_void_p), 0, s.shape[1], s.shape[2], s.shape[3], C.byref(g),
                                C.byref(st), _stream_arg(stream)))


class _Completing(object):
    """`completion` and `dedupe` of Net and NetGroup (stages D and E of the people assembly, include/deepcut_hip.h): state of the object,
    read by every entry that assembles people.  `_set_completion` / `_get_completion` / `_set_dedupe` / `_get_dedupe` name the library
    entries."""

    @property
    def dedupe(self):
        """None (off, the default) or {"max_dist", "min_common", "min_size", "sigma", "absorb"}: with it every assembling entry removes
        the people who are there twice, on the device behind the assembly and the completion and before the tracker (stage E): people
        are ranked by the sum of their joint scores, and a person that a better kept person is the same as — the tracker's distance,
        normalised by the better one's size, <= max_dist over at least min_common joints both hold — is suppressed; with absorb the kept
        person takes the assigned joints it lacks from the people it suppressed, which puts two fragments of one human back together.
        Assign None / False, True (DEDUPE_DEFAULTS: PLACEHOLDERS, not tuned on real images) or a dict of some of the five.  A bad value
        raises DeepcutError naming the field, with or without a device; a sigma whose length is not the net's joints, or min_common above
        them, is refused by the first assembling call.  `Net.clone()` copies the setting; a NetGroup has one of its own.  The rule is
        this project's own: the reference stops at the maps."""
        q, sig = DedupeParams(), np.zeros(32, np.float64)
        _check(getattr(_lib, self._get_dedupe)(self._h, C.byref(q), sig.ctypes.data_as(C.c_void_p)))
        if not q.enabled:
            return None
        return {"max_dist": float(q.max_dist), "min_common": int(q.min_common), "min_size": float(q.min_size),
                "sigma": sig[:q.n_sigma].copy() if q.n_sigma else None, "absorb": bool(q.absorb)}

    @dedupe.setter
    def dedupe(self, dedupe):
        d = dedupe_params(dedupe)
        if d is None:
            _check(getattr(_lib, self._set_dedupe)(self._h, None))
            return
        q, _sig = _dedupe_struct(d)
        _check(getattr(_lib, self._set_dedupe)(self._h, C.byref(q)))

    @property
    def completion(self):
        """None (off, the default) or {"fill_threshold", "fill_radius", "min_support"}: with it every assembling entry fills the joints
        a person lacks from the score map around the position the person's held joints predict, on the device behind the assembly
        (a joint filled so has cand == -2, and the result a "filled" array).  Assign None / False, True (COMPLETE_DEFAULTS: PLACEHOLDERS,
        not tuned on real images) or a dict of some of the three.  A bad value raises DeepcutError naming the field, with or without a
        device.  `Net.clone()` copies the setting; a NetGroup has one of its own.  The rule is this project's own: the reference stops
        at the maps."""
        q = CompleteParams()
        _check(getattr(_lib, self._get_completion)(self._h, C.byref(q)))
        if not q.enabled:
            return None
        return {"fill_threshold": float(q.fill_threshold), "fill_radius": int(q.fill_radius), "min_support": int(q.min_support)}

    @completion.setter
    def completion(self, complete):
        d = completion_params(complete)
        if d is None:
            _check(getattr(_lib, self._set_completion)(self._h, None))
            return
        try:
            q = CompleteParams(1, float(d["fill_threshold"]), int(d["fill_radius"]), int(d["min_support"]))
        except (TypeError, ValueError) as e:
            raise ValueError("completion: fill_threshold must be a number, fill_radius and min_support whole numbers (%s)" % (e,))
        _check(getattr(_lib, self._set_completion)(self._h, C.byref(q)))

    @contextlib.contextmanager
    def _completing(self, complete, dedupe=None):
        """For the calls that take `complete=` and `dedupe=`: None leaves the object's `completion` / `dedupe` as it is; anything else
        holds for this call only."""
        if dedupe is not None:
            before = self.dedupe
            self.dedupe = dedupe
            try:
                with self._completing(complete) as completed:
                    yield completed
            finally:
                self.dedupe = before
            return
        if complete is None:
            yield self.completion is not None
            return
        before = self.completion
        self.completion = complete
        try:
            yield self.completion is not None
        finally:
            self.completion = before


class TrackedFrames(object):
    """What `Net.track_frames_async` returns: the request in flight.  It owns the pinned output arrays and keeps the frames alive;
    `result()` waits for the net and returns what `Net.track_people` returns."""

    def __init__(self, net, tracked, count, people, cand, ids, place, keep, pool=None, completed=False, bridging=False, redacted=None):
        self._net, self._tracked, self._keep, self._pool, self._completed = net, tracked, keep, pool, completed
        self._bridging, self._redacted = bridging, redacted
        self._count, self._people, self._cand, self._ids, self._place = count, people, cand, ids, place
        self._out, self._ready = None, False

    def done(self):
        """True when the results are there: the net's stream was seen with nothing left to do since this request went out (remembered,
        so that a later request on the same net does not make this one look unfinished)."""
        if not self._ready and not self._net.busy():
            self._ready = True
        return self._ready

    def result(self):
        """-> one dict per image: "people", "cand" and, with a tracker, "ids" and "place" (`Net.track_people`); with redact= also
        "redacted" (int32 [m], as `redact_people` returns it).  Waits for the net."""
        if self._out is None:
            if not self._ready:
                self._net.synchronize()
                self._ready = True
            out = []
            for b in range(self._count.shape[0]):
                m = int(self._count[b])
                d = {"people": self._people[b, :m].copy(), "cand": self._cand[b, :m].copy()}
                if self._completed:
                    d["filled"] = d["cand"] == -2
                if self._bridging:
                    d["bridged"] = d["cand"] == -3
                if self._tracked:
                    d["ids"], d["place"] = self._ids[b, :m].copy(), self._place[b, :m].copy()
                if self._redacted is not None:
                    d["redacted"] = self._redacted[b, :m].copy()
                out.append(d)
            self._out, self._keep = out, None
            if self._pool is not None:  # everything is copied out: the pinned arrays serve the net's next request of this shape
                self._pool.append((self._count, self._people, self._cand, self._ids, self._place))
                self._count = self._people = self._cand = self._ids = self._place = self._pool = None
                if self._redacted is not None:
                    self._net.__dict__.setdefault("_async_redacted", {}).setdefault(self._redacted.shape, []).append(self._redacted)
            self._redacted = None
        return self._out


def _tracker_smoothing(tracker):
    """Whether the results of a chained entry carry "bridged": the tracker has smoothing on (`Tracker.smoothing`)."""
    _tracker_handle(tracker)
    return tracker.smoothing is not None


def _tracker_handle(tracker):
    if not isinstance(tracker, Tracker):
        raise TypeError("track_people needs a caffe.Tracker, got %r" % (type(tracker).__name__,))
    return tracker._h


class Layer(object):
    """caffe.Layer as pycaffe shows it: the type string and the parameter blobs."""

    def __init__(self, type_, blobs):
        self.type = type_
        self.blobs = list(blobs)


class Blob(object):
    """caffe.Blob (_caffe.cpp:259-277).  `.data` is a writable float32 NCHW view of the blob's host
    memory whose base object keeps the owning Net alive (python/caffe/test/test_net.py:48-60)."""

    def __init__(self, handle, owner):
        self._h = handle
        self._owner = owner  # keeps the Net (and thus the memory) alive

    @property
    def shape(self):
        n = C.c_int()
        dims = (C.c_int * 8)()
        _check(_lib.dc_blob_shape(self._h, C.byref(n), dims))
        return tuple(dims[i] for i in range(n.value))

    def _legacy(self, i):
        s = self.shape
        s = (1,) * (4 - len(s)) + s  # Blob::LegacyShape (blob.hpp:118-134)
        return s[i]

    num = property(lambda self: self._legacy(0))
    channels = property(lambda self: self._legacy(1))
    height = property(lambda self: self._legacy(2))
    width = property(lambda self: self._legacy(3))
    count = property(lambda self: _lib.dc_blob_count(self._h))

    def reshape(self, *dims):
        if len(dims) == 1 and hasattr(dims[0], "__len__"):
            dims = tuple(dims[0])
        arr = (C.c_int * len(dims))(*[int(d) for d in dims])
        _check(_lib.dc_blob_reshape(self._h, len(dims), arr))

    @property
    def data(self):
        p = C.POINTER(C.c_float)()
        _check(_lib.dc_blob_mutable_cpu_data(self._h, C.byref(p)))  # Blob::mutable_cpu_data (_caffe.cpp:273)
        shape = self.shape
        n = int(np.prod(shape)) if shape else 1
        buf = (C.c_float * n).from_address(C.addressof(p.contents))
        buf._owner = self  # ndarray.base chain -> ctypes array -> Blob -> Net
        return np.frombuffer(buf, dtype=np.float32).reshape(shape)

    @property
    def head(self):
        return _lib.dc_blob_head(self._h)

    def gpu_data(self):
        """(device pointer of the NHWC image, channel pitch) — Blob::gpu_data."""
        p = C.c_void_p()
        pitch = C.c_int()
        _check(_lib.dc_blob_gpu_data(self._h, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value


class _NetHandle(object):
    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h:
            _lib.dc_net_destroy(self.h)
            self.h = None


class Net(_Completing):
    """caffe.Net(model_def, model_bin, phase) / caffe.Net(model_def, phase)  (_caffe.cpp:76-96,227-228)."""

    _set_completion, _get_completion = "dc_net_set_completion", "dc_net_get_completion"
    _set_dedupe, _get_dedupe = "dc_net_set_dedupe", "dc_net_get_dedupe"

    def __init__(self, model_def, *args, **kw):
        if "_handle" in kw:  # clone()
            self._h = kw["_handle"]
            self._handle = _NetHandle(self._h)
            self._blobs = None
            self._params = None
            return
        if len(args) == 2:
            weights, phase = args
        elif len(args) == 1:
            weights, phase = None, args[0]
        else:
            raise TypeError("Net(model_def, [weights,] phase)")
        h = C.c_void_p()
        if kw.get("from_text"):
            rc = _lib.dc_net_create_from_text(model_def.encode(), weights.encode() if weights else None, int(phase), C.byref(h))
        else:
            rc = _lib.dc_net_create(model_def.encode(), weights.encode() if weights else None, int(phase), C.byref(h))
        _check(rc)
        self._handle = _NetHandle(h)
        self._h = h
        if "fuse" in kw:
            self.set_option(1, int(kw["fuse"]))
        if "hipgraph" in kw:
            self.set_option(2, int(kw["hipgraph"]))
        if "dtype" in kw:
            self.set_option(3, _DTYPES[kw["dtype"]])
        self._blobs = None
        self._params = None
        if kw.get("want") is not None:
            self.set_outputs(kw["want"])
        if kw.get("sparse_pairwise"):
            self.sparse_pairwise = True

    def set_option(self, key, value):
        _check(_lib.dc_net_set_option(self._h, int(key), int(value)))

    def get_option(self, key):
        v = C.c_int()
        _check(_lib.dc_net_get_option(self._h, int(key), C.byref(v)))
        return v.value

    def set_outputs(self, names=None):
        """DC_OPT_OUTPUTS: the output blobs the forward has to produce (None = all).  The lowering drops every launch that only feeds
        the others — the demo reads `prob` and `loc_pred` only (python/pose/estimate_pose.py:231-241), and without `next_pred` the
        merged heads shrink from 406 to 42 channels.  The wanted maps equal the full forward's (bit for bit under the same tile); `forward()` returns
        the wanted outputs only, and `.data` on a left-out blob raises."""
        outs = self.outputs
        if names is None:
            mask = -1
        else:
            unknown = [n for n in names if n not in outs]
            if unknown:
                raise ValueError("not output blobs of this net: %r (outputs: %r)" % (unknown, outs))
            mask = 0
            for n in names:
                mask |= 1 << outs.index(n)
        self.set_option(4, mask)

    @property
    def wanted_outputs(self):
        mask = self.get_option(4)
        return [n for i, n in enumerate(self.outputs) if mask == -1 or (mask >> i) & 1]

    @property
    def sparse_pairwise(self):
        """DC_OPT_SPARSE_PAIRWISE: a net whose outputs leave `next_pred` out evaluates the pairwise head at the cells `assemble_people`,
        `decode_pairwise` and `pairwise_at` read (include/deepcut_hip.h, dc_net_pairwise_at) instead of refusing.  Off by default; a
        net that computes `next_pred` reads the dense map either way.  Setting it on a net without such a head raises (DC_EUNSUP)."""
        return bool(self.get_option(5))

    @sparse_pairwise.setter
    def sparse_pairwise(self, on):
        self.set_option(5, 1 if on else 0)

    @property
    def dtype(self):
        """'f32', 'f16' or 'bf16': the element type of activations and filters in HBM (DC_OPT_DTYPE)."""
        return {1: "f16", 2: "bf16"}.get(self.get_option(3), "f32")

    # --- pycaffe.py:22-59 -----------------------------------------------------------------
    @property
    def blobs(self):
        if self._blobs is None:
            d = OrderedDict()
            for i in range(_lib.dc_net_num_blobs(self._h)):
                name = _lib.dc_net_blob_name(self._h, i)
                bh = C.c_void_p()
                _check(_lib.dc_net_blob(self._h, name, C.byref(bh)))
                d[name.decode()] = Blob(bh, self._handle)
            self._blobs = d
        return self._blobs

    @property
    def _layer_names(self):
        # fixed at construction (Net::Init); forward() looks names up on every call: 734 ctypes round trips otherwise
        names = self.__dict__.get("_names_cache")
        if names is None:
            names = self.__dict__["_names_cache"] = [_lib.dc_net_layer_name(self._h, i).decode() for i in range(_lib.dc_net_num_layers(self._h))]
        return list(names)

    @property
    def layer_types(self):
        return [_lib.dc_net_layer_type(self._h, i).decode() for i in range(_lib.dc_net_num_layers(self._h))]

    @property
    def layers(self):
        """caffe.Net.layers (_caffe.cpp:243-244, Layer :279-284): one object per layer (auto-inserted Split layers
        included) with `.type` and `.blobs` (the layer's parameter blobs, shared with `net.params`)."""
        names, types, params = self._layer_names, self.layer_types, self.params
        return [Layer(t, params.get(n, [])) for n, t in zip(names, types)]

    @property
    def params(self):
        if self._params is None:
            d = OrderedDict()
            for name in self._layer_names:
                n = _lib.dc_net_layer_num_params(self._h, name.encode())
                if n > 0:
                    lst = []
                    for j in range(n):
                        bh = C.c_void_p()
                        _check(_lib.dc_net_param(self._h, name.encode(), j, C.byref(bh)))
                        lst.append(Blob(bh, self._handle))
                    d[name] = lst
            self._params = d
        return self._params

    @property
    def inputs(self):
        v = self.__dict__.get("_inputs_cache")
        if v is None:
            v = self.__dict__["_inputs_cache"] = [_lib.dc_net_input_name(self._h, i).decode() for i in range(_lib.dc_net_num_inputs(self._h))]
        return list(v)

    @property
    def outputs(self):
        v = self.__dict__.get("_outputs_cache")
        if v is None:
            v = self.__dict__["_outputs_cache"] = [_lib.dc_net_output_name(self._h, i).decode() for i in range(_lib.dc_net_num_outputs(self._h))]
        return list(v)

    @property
    def name(self):
        return _lib.dc_net_name(self._h).decode()

    # --- pycaffe.py:62-108 ----------------------------------------------------------------
    def _forward(self, start, end):
        loss = C.c_float()
        _check(_lib.dc_net_forward(self._h, int(start), int(end), C.byref(loss)))
        return loss.value

    def forward(self, blobs=None, start=None, end=None, **kwargs):
        if blobs is None:
            blobs = []
        if start is None and end is None:
            start_ind, end_ind = 0, _lib.dc_net_num_layers(self._h) - 1
            outputs = set(self.wanted_outputs + blobs)
        else:
            names = self._layer_names
            start_ind = names.index(start) if start is not None else 0
            if end is not None:
                end_ind = names.index(end)
                outputs = set([end] + blobs)
            else:
                end_ind = len(names) - 1
                outputs = set(self.wanted_outputs + blobs)
        if kwargs:
            if set(kwargs.keys()) != set(self.inputs):
                raise Exception("Input blob arguments do not match net inputs.")
            for in_, blob in kwargs.items():
                if blob.shape[0] != self.blobs[in_].num:
                    raise Exception("Input is not batch sized")
                self.blobs[in_].data[...] = blob
        self._forward(start_ind, end_ind)
        return {out: self.blobs[out].data for out in outputs}

    def reshape(self):
        _check(_lib.dc_net_reshape(self._h))

    def copy_from(self, path):
        _check(_lib.dc_net_copy_from(self._h, path.encode()))

    def save(self, path):
        _check(_lib.dc_net_save(self._h, path.encode()))

    # --- extensions (no pycaffe counterpart) ---------------------------------------------------
    def _out_array(self, key, shape, out=None):
        """Destination array of one output map.  `out` (a dict of C-contiguous float32 arrays of the right shape) wins.
        Otherwise memory from a small per-net pool is handed out again once NOBODY references the previous hand-out any more
        (views included: `_OutPool`), else new memory is taken.
        Why: a fresh 73 MB `np.empty` is untouched virtual memory; the device-to-host copy then faults every page of it
        inside the driver's pin-on-the-fly path, which cost the float16 batch-8 host entry 7-35 ms per call (review r3,
        weak 2) against 2.4 ms for the same copy into pages that exist."""
        if out is not None and key in out:
            a = out[key]
            if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and tuple(a.shape) == tuple(shape)):
                raise ValueError("out[%r] must be a C-contiguous float32 array of shape %s" % (key, tuple(shape)))
            return a
        pools = self.__dict__.setdefault("_out_pool", OrderedDict())
        pk = (key, tuple(shape))
        pool = pools.get(pk)
        if pool is None:
            pool = pools[pk] = _OutPool()
            while len(pools) > 24:  # shapes of long ago go first
                pools.popitem(last=False)
        else:
            pools.move_to_end(pk)
        return pool.take(tuple(shape))

    def forward_batch(self, images, want=("prob", "loc_pred", "next_pred"), out=None):
        """images: float32 [n,3,H,W] host array -> dict of NCHW host arrays (one batched launch plan).  The arrays of a
        result that the caller no longer references are recycled by a later call (see _out_array); `out` = {name: array}
        writes into the caller's own buffers."""
        x = np.ascontiguousarray(images, dtype=np.float32)
        n, c, h, w = x.shape
        self.blobs["data"].reshape(n, c, h, w)
        self.reshape()
        outs = {}
        ptrs = {}
        for k in ("prob", "loc_pred", "next_pred"):
            if k in want:
                outs[k] = self._out_array(k, self.blobs[k].shape, out)
                ptrs[k] = outs[k].ctypes.data_as(C.c_void_p)
            else:
                ptrs[k] = None
        _check(_lib.dc_net_forward_batch(self._h, x.ctypes.data_as(C.c_void_p), n, h, w, 0, ptrs["prob"],
                                         ptrs["loc_pred"], ptrs["next_pred"], None))
        return outs

    def forward_device(self, in_ptr, n, h, w, prob_ptr=None, loc_ptr=None, next_ptr=None, stream=None):
        """Device-resident batch: raw device pointers (e.g. torch tensor .data_ptr()), asynchronous on
        `stream` when given."""
        if stream == "own":  # DC_STREAM_OWN: the net's own stream, asynchronous
            stream = C.c_void_p(-1).value
        _check(_lib.dc_net_forward_batch(self._h, C.c_void_p(in_ptr), n, h, w, 1, C.c_void_p(prob_ptr or 0),
                                         C.c_void_p(loc_ptr or 0), C.c_void_p(next_ptr or 0), C.c_void_p(stream or 0)))

    def forward_host_async(self, x, prob=None, loc_pred=None, next_pred=None):
        """dc_net_forward_host_async: x float32 [n,3,H,W] and the output arrays (C-contiguous float32 of the maps' shapes, or
        None) are HOST arrays; nothing is waited for — the upload, the forward and the downloads are enqueued on the net's own
        stream.  Collect with synchronize() (or poll busy()); every array must stay alive and untouched until then.  Arrays from
        caffe.pinned_empty() are copied by the DMA engines beside other executors' kernels."""
        for a in (x, prob, loc_pred, next_pred):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]):
                raise ValueError("forward_host_async wants C-contiguous float32 arrays")
        if x.ndim != 4:
            raise ValueError("forward_host_async takes a [n, C, H, W] batch, got shape %s" % (x.shape,))
        n, c, h, w = x.shape
        # the library reads n*C*h*w floats and writes whole maps through these raw pointers, asynchronously (DMA): a wrongly shaped
        # array would be silent out-of-bounds host memory access, so every size is checked against the net's own shape inference
        want_c = self.blobs["data"].channels
        if c != want_c:
            raise ValueError("forward_host_async: input has %d channels, the net's 'data' blob %d" % (c, want_c))
        dims = self.__dict__.setdefault("_host_map_counts", {})
        key = (n, h, w)
        if key not in dims:
            self.blobs["data"].reshape(n, c, h, w)
            self.reshape()  # shape inference only (host)
            dims[key] = {k: int(np.prod(self.blobs[k].shape)) for k in ("prob", "loc_pred", "next_pred") if k in self.blobs}
            while len(dims) > 64:
                dims.pop(next(iter(dims)))
        for name, a in (("prob", prob), ("loc_pred", loc_pred), ("next_pred", next_pred)):
            if a is not None and a.size != dims[key].get(name, -1):
                raise ValueError("forward_host_async: %s has %d elements, the map of a %s batch %d" % (name, a.size, (n, c, h, w), dims[key].get(name, -1)))
        ptr = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)  # noqa: E731
        _check(_lib.dc_net_forward_host_async(self._h, ptr(x), n, h, w, ptr(prob), ptr(loc_pred), ptr(next_pred)))

    def stream_handle(self):
        """The net's own HIP stream (an integer hipStream_t, e.g. for torch.cuda.ExternalStream): what stream="own" enqueues on."""
        p = C.c_void_p()
        _check(_lib.dc_net_stream(self._h, C.byref(p)))
        return p.value or 0

    def forward_requests(self, in_ptrs, h, w, prob_ptrs=None, loc_ptrs=None, next_ptrs=None, stream=None):
        """Cross-request batching: len(in_ptrs) independent single-image requests (raw device pointers, one output pointer
        per request or None) run as ONE batch forward; asynchronous on `stream` ("own" = the net's)."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        n = len(in_ptrs)

        def arr(ps):
            if ps is None:
                return None
            return (C.c_void_p * n)(*[C.c_void_p(p or 0) for p in ps])

        _check(_lib.dc_net_forward_requests(self._h, n, arr(in_ptrs), int(h), int(w), arr(prob_ptrs), arr(loc_ptrs), arr(next_ptrs),
                                            C.c_void_p(stream or 0)))

    def decode_pose(self, scale=1.0):
        """-> float64 [n, 5, J]: `_pose_from_mats` of the last forward, computed on the device."""
        n, j = self.blobs["prob"].shape[:2]
        out = np.empty((n, 5, j), np.float64)
        _check(_lib.dc_net_decode_pose(self._h, float(scale), out.ctypes.data_as(C.c_void_p), 0, None))
        return out

    def forward_images(self, images, scale=1.0, want=("prob", "loc_pred"), pose=True):
        """images: uint8 [n,H,W,3] (or [H,W,3]) BGR host array.  The demo's pre-processing (replicate pad, PIL-exact
        bilinear rescale, mean subtraction, stride-8 canvas; estimate_pose.py:83-103) runs on the device, then the
        forward and — pose=True — `_pose_from_mats`.  -> dict with the requested NCHW maps and "pose" [n,5,J].
        A `Frame` or a list of `Frame`s (video frames of one size: dc_net_forward_frames) is taken in place of the array."""
        frames = _frame_list(images)
        if frames is not None:
            return self._forward_frames(frames, scale, want, pose)
        x = np.ascontiguousarray(images, dtype=np.uint8)
        if x.ndim == 3:
            x = x[None]
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("images must be uint8 [n,H,W,3] (BGR)")
        n, h, w, _ = x.shape
        ch, cw = canvas_size(h, w, scale)
        self.blobs["data"].reshape(n, 3, ch, cw)
        self.reshape()
        outs, ptrs = {}, {}
        for k in ("prob", "loc_pred", "next_pred"):
            if k in want:
                outs[k] = self._out_array(k, self.blobs[k].shape)
                ptrs[k] = outs[k].ctypes.data_as(C.c_void_p)
            else:
                ptrs[k] = None
        pp = None
        if pose:
            outs["pose"] = np.empty((n, 5, self.blobs["prob"].shape[1]), np.float64)
            pp = outs["pose"].ctypes.data_as(C.c_void_p)
        _check(_lib.dc_net_forward_images(self._h, x.ctypes.data_as(C.c_void_p), n, h, w, float(scale), 0, ptrs["prob"],
                                          ptrs["loc_pred"], ptrs["next_pred"], pp, None))
        return outs

    def _host_maps(self, want):
        """-> the requested maps of the last forward as NCHW float32 host arrays (dc_net_emit_maps)."""
        outs = {k: self._out_array(k, self.blobs[k].shape) for k in ("prob", "loc_pred", "next_pred") if k in want}
        if outs:
            p = {k: outs[k].ctypes.data_as(C.c_void_p) if k in outs else None for k in ("prob", "loc_pred", "next_pred")}
            _check(_lib.dc_net_emit_maps(self._h, p["prob"], p["loc_pred"], p["next_pred"], 0, 0, None))
        return outs

    def _forward_frames(self, frames, scale, want, pose):
        arr, h, w, dev = _frame_array(frames)
        n = len(frames)
        ch, cw = canvas_size(h, w, scale)
        self.blobs["data"].reshape(n, 3, ch, cw)
        self.reshape()
        if dev:  # device frames: the forward with no output (it is complete on return), then the maps and the pose to the host
            _check(_lib.dc_net_forward_frames(self._h, arr, n, h, w, float(scale), 1, None, None, None, None, None))
            outs = self._host_maps(want)
            if pose:
                outs["pose"] = self.decode_pose(scale)
            return outs
        outs = {k: self._out_array(k, self.blobs[k].shape) for k in ("prob", "loc_pred", "next_pred") if k in want}
        ptrs = {k: outs[k].ctypes.data_as(C.c_void_p) if k in outs else None for k in ("prob", "loc_pred", "next_pred")}
        pp = None
        if pose:
            outs["pose"] = np.empty((n, 5, self.blobs["prob"].shape[1]), np.float64)
            pp = outs["pose"].ctypes.data_as(C.c_void_p)
        _check(_lib.dc_net_forward_frames(self._h, arr, n, h, w, float(scale), 0, ptrs["prob"], ptrs["loc_pred"], ptrs["next_pred"], pp, None))
        return outs

    def forward_boxes(self, image, boxes, scales=1.0, canvas=None, want=("prob", "loc_pred"), pose=True):
        """Top-down poses of person boxes: image uint8 [H,W,3] BGR host array, boxes n x 4 (x0, y0, x1, y1) half-open pixel
        corners, scales one number or one per box, canvas (h, w) multiples of 8 or None (the smallest that fits every box:
        check_boxes).  Box i is pre-processed as forward_images would pre-process image[y0:y1, x0:x1] at scales[i], pasted at the
        top-left of the common canvas; all boxes in one launch and one batch forward.  -> dict with the requested NCHW maps
        (n x the whole canvas's map) and "pose" [n,5,J] decoded on each box's own canvas, in image coordinates.
        A `Frame` (dc_net_forward_boxes_frame) is taken in place of the array; a box pairs chroma by its place in the IMAGE.  A device
        frame's poses are not copied to the host by this method: pass pose=False."""
        frame = image if isinstance(image, Frame) else None
        if frame is not None and frame.is_device and pose:
            raise ValueError("forward_boxes of a device frame returns maps only: pass pose=False")
        x = None if frame is not None else np.ascontiguousarray(image, dtype=np.uint8)
        if x is not None and (x.ndim != 3 or x.shape[2] != 3):
            raise ValueError("image must be uint8 [H,W,3] (BGR)")
        shape = frame.shape if frame is not None else x.shape
        b, sc, (ch, cw) = check_boxes(shape, boxes, scales, canvas)
        n, j = b.shape[0], self.blobs["prob"].shape[1]
        if n == 0:
            outs = {k: np.empty((0,), np.float32) for k in ("prob", "loc_pred", "next_pred") if k in want}
            if pose:
                outs["pose"] = np.empty((0, 5, j), np.float64)
            return outs
        self.blobs["data"].reshape(n, 3, ch, cw)
        self.reshape()
        if frame is not None and frame.is_device:
            _check(_lib.dc_net_forward_boxes_frame(self._h, C.byref(frame.c_frame()), shape[0], shape[1], 1, b.ctypes.data_as(C.c_void_p),
                                                   sc.ctypes.data_as(C.c_void_p), n, ch, cw, None, None, None, None, None))
            return self._host_maps(want)
        outs, ptrs = {}, {}
        for k in ("prob", "loc_pred", "next_pred"):
            if k in want:
                outs[k] = self._out_array(k, self.blobs[k].shape)
                ptrs[k] = outs[k].ctypes.data_as(C.c_void_p)
            else:
                ptrs[k] = None
        pp = None
        if pose:
            outs["pose"] = np.empty((n, 5, j), np.float64)
            pp = outs["pose"].ctypes.data_as(C.c_void_p)
        if frame is not None:
            _check(_lib.dc_net_forward_boxes_frame(self._h, C.byref(frame.c_frame()), shape[0], shape[1], 0, b.ctypes.data_as(C.c_void_p),
                                                   sc.ctypes.data_as(C.c_void_p), n, ch, cw, ptrs["prob"], ptrs["loc_pred"], ptrs["next_pred"],
                                                   pp, None))
            return outs
        _check(_lib.dc_net_forward_boxes(self._h, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], 0, b.ctypes.data_as(C.c_void_p),
                                         sc.ctypes.data_as(C.c_void_p), n, ch, cw, ptrs["prob"], ptrs["loc_pred"], ptrs["next_pred"], pp, None))
        return outs

    def forward_boxes_device(self, img_ptr, h, w, boxes, scales, canvas, prob_ptr=None, loc_ptr=None, next_ptr=None, pose_ptr=None,
                             stream=None):
        """Device-resident form of forward_boxes: the image (uint8 [h,w,3]) and the outputs are raw device pointers, boxes and scales
        host arrays, canvas (h, w) given; asynchronous on `stream` ("own" = the net's)."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        b, sc, (ch, cw) = check_boxes((h, w), boxes, scales, canvas)
        _check(_lib.dc_net_forward_boxes(self._h, C.c_void_p(img_ptr), int(h), int(w), 1, b.ctypes.data_as(C.c_void_p),
                                         sc.ctypes.data_as(C.c_void_p), b.shape[0], ch, cw, C.c_void_p(prob_ptr or 0), C.c_void_p(loc_ptr or 0),
                                         C.c_void_p(next_ptr or 0), C.c_void_p(pose_ptr or 0), C.c_void_p(stream or 0)))

    def forward_images_device(self, img_ptr, n, h, w, scale=1.0, prob_ptr=None, loc_ptr=None, next_ptr=None,
                              pose_ptr=None, stream=None):
        """Device-resident form of forward_images: raw device pointers, asynchronous on `stream` ("own" = the net's)."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        _check(_lib.dc_net_forward_images(self._h, C.c_void_p(img_ptr), n, h, w, float(scale), 1, C.c_void_p(prob_ptr or 0),
                                          C.c_void_p(loc_ptr or 0), C.c_void_p(next_ptr or 0), C.c_void_p(pose_ptr or 0),
                                          C.c_void_p(stream or 0)))

    def emit_maps_device(self, prob_ptr=None, loc_ptr=None, next_ptr=None, half=False, stream=None):
        """Copy the maps of the last forward into device buffers as NCHW float32, or (half=True, fp16 / bf16 nets) the net's
        16-bit values as they are (float16 / bfloat16) — the gather payload in the net's own element type.  Asynchronous on `stream` ("own" = the net's)."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        _check(_lib.dc_net_emit_maps(self._h, C.c_void_p(prob_ptr or 0), C.c_void_p(loc_ptr or 0), C.c_void_p(next_ptr or 0),
                                     1 if half else 0, 1, C.c_void_p(stream or 0)))

    def detect_parts(self, scale=1.0, threshold=0.1, radius=1, max_det=32):
        """Part candidates of the last forward (NMS of every score map + location refinement, on the device).
        -> (counts int32 [n, J], dets float64 [n, J, max_det, 5] = x, y, score, cell row, cell column)."""
        n, j = self.blobs["prob"].shape[:2]
        counts = np.zeros((n, j), np.int32)
        dets = np.zeros((n, j, max_det, 5), np.float64)
        _check(_lib.dc_net_detect_parts(self._h, float(scale), float(threshold), int(radius), int(max_det),
                                        counts.ctypes.data_as(C.c_void_p), dets.ctypes.data_as(C.c_void_p)))
        return counts, dets

    def draw_heatmap(self, frames, scale=1.0, origin=(0.0, 0.0), joints=None, mode="max", alpha=128, alpha_mode="score", min_score=0.0,
                     lut=None, palette=None):
        """`prob` of the last forward blended into frames IN PLACE (dc_net_draw_heatmap): `caffe.draw_heatmap` on the map where it is on
        the device, in the net's element type — no download, no layout pass.  One frame per image of the forward; scale: what the forward
        ran at.  The other arguments as `caffe.draw_heatmap`.  Runs on the net's stream behind the forward and returns when complete."""
        arr, nb, h, w, is_device, _keep = _writable_frames(frames)
        st, _arrays = _heat_style(self.blobs["prob"].shape[1], joints, mode, alpha, alpha_mode, min_score, lut, palette)
        g = HeatGeometry(float(scale), float(origin[0]), float(origin[1]))
        _check(_lib.dc_net_draw_heatmap(self._h, arr, nb, h, w, int(is_device), C.byref(g), C.byref(st)))

    def decode_pairwise(self, detections, scale=1.0, mean=None, std=None):
        """detections: int [D, 3] (image, cell row, cell column) -> float64 [D, E, 2]: where every regression edge of
        next_pred puts the next joint, seen from each detection's cell (mean / std: [E, 2] de-normalisation)."""
        det = np.ascontiguousarray(detections, np.int32).reshape(-1, 3)
        e = self.blobs["next_pred"].shape[1] // 2
        out = np.zeros((det.shape[0], e, 2), np.float64)
        m = None if mean is None else np.ascontiguousarray(mean, np.float64).reshape(e, 2)
        s = None if std is None else np.ascontiguousarray(std, np.float64).reshape(e, 2)
        _check(_lib.dc_net_decode_pairwise(self._h, float(scale), det.shape[0], det.ctypes.data_as(C.c_void_p),
                                           None if m is None else m.ctypes.data_as(C.c_void_p),
                                           None if s is None else s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def pairwise_at(self, detections):
        """detections: int [D, 3] (image, cell row, cell column) -> float32 [D, C]: the raw `next_pred` values of the last forward at those
        cells (dc_net_pairwise_at): from the dense map when the plan computes it, else — `sparse_pairwise` set — the pairwise head
        evaluated at those cells alone.  A cell outside the map raises before any device work."""
        det = np.ascontiguousarray(detections, np.int32).reshape(-1, 3)
        out = np.zeros((det.shape[0], self.blobs["next_pred"].shape[1]), np.float32)
        _check(_lib.dc_net_pairwise_at(self._h, det.shape[0], det.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def assemble_people(self, scale=1.0, threshold=0.1, radius=1, max_det=16, edges=None, mean=None, std=None, max_cost=32.0,
                        seed_threshold=0.5, max_people=32, min_joints=1, joint_order=None, return_cost=False, complete=None, dedupe=None):
        """The people of every image of the last forward (dc_net_assemble_people): part candidates, pair costs from `next_pred` and a
        greedy assembly, all on the device; only the results come back.  edges: [E, 2] 0-based (joint, next joint) of the regression
        edges (E = next_pred channels / 2), mean / std: their [E, 2] de-normalisation (deepcut_tools.read_pair_stats), None = 0 / 1.
        A link is allowed when its cost (network pixels) is <= max_cost; a candidate that joins nobody starts a person when its score
        is >= seed_threshold.  The defaults of max_cost and seed_threshold are PLACEHOLDERS, not tuned on real images: override them.
        The grouping rule (include/deepcut_hip.h) is this project's own; the reference stops at the maps.
        -> one dict per image: {"people": float64 [m, J, 3] = x, y, score ((0, 0, 0) for a missing joint), "cand": int32 [m, J] =
        index in the joint's candidate list or -1}, plus "cost": float64 [J, J, max_det, max_det] with return_cost.
        complete: None = the net's `completion` as it stands; True, a dict or False = that setting for this call only.  When completion
        runs, missing joints are filled on the device (stage D, include/deepcut_hip.h): such a joint has cand == -2 and the dict gains
        "filled": bool [m, J].
        dedupe: likewise for the net's `dedupe` (stage E): None = as it stands; True, a dict or False = for this call only.  When it runs,
        people who are there twice are suppressed on the device behind the completion: m shrinks, the kept people keep their order."""
        return self._assemble_people(None, scale, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people, min_joints,
                                     joint_order, return_cost, complete=complete, dedupe=dedupe)

    def track_people(self, tracker, scale=1.0, threshold=0.1, radius=1, max_det=16, edges=None, mean=None, std=None, max_cost=32.0,
                     seed_threshold=0.5, max_people=32, min_joints=1, joint_order=None, return_cost=False, slot_of=None, complete=None,
                     dedupe=None):
        """`assemble_people` with the identities of a `caffe.Tracker` (dc_net_track_people): the tracker's update runs on the device
        behind the assembly, on the people where the assembly left them — image b updates slot b.  The arguments and the result are
        `assemble_people`'s, unchanged, with two more entries per image: "ids": int64 [m] (the same person keeps their id from frame
        to frame; -1 = no track place was free) and "place": int32 [m] (the track place, an index into `tracker.state()`).
        slot_of: [batch] ints, the slot every image updates (dc_net_track_people_slots; `Tracker.update`): a batch forward of k
        consecutive frames of one video is tracked with slot_of = [slot] * k.
        complete, dedupe: as `assemble_people`; the tracker then receives the completed people / only the people that were kept."""
        _tracker_handle(tracker)
        return self._assemble_people(tracker, scale, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people,
                                     min_joints, joint_order, return_cost, slot_of, complete, dedupe)

    def track_frames_async(self, frames_or_images, tracker=None, scale=1.0, slot_of=None, assemble_scale=None, threshold=0.1, radius=1,
                           max_det=16, edges=None, mean=None, std=None, max_cost=32.0, seed_threshold=0.5, max_people=32, min_joints=1,
                           joint_order=None, complete=None, dedupe=None, draw=None, redact=None, labels=None):
        """The whole video chain without a host wait (dc_net_track_frames_async): upload, pre-processing, forward, assembly, the
        tracker's update and the downloads are enqueued on the net's own stream and the call returns.  frames_or_images: a `Frame`, a
        list of `Frame`s of one size, or uint8 [n,H,W,3] / [H,W,3] BGR; they must stay untouched until the result is collected.
        tracker: a `caffe.Tracker`, or None for people without ids; slot_of as `track_people`.  scale: the pre-processing's;
        assemble_scale: the assembly's (None: the same).  The other arguments are `assemble_people`'s, `complete` and `dedupe` included
        (what holds when the call is made is what the request runs with).
        -> a `TrackedFrames`: `result()` synchronises the net and returns what `forward_images` + `track_people` return, bit for bit.
        A second call on a busy net queues behind the first; to overlap calls use clones (`deepcut_tools.VideoPipeline`): the tracker
        keeps the updates in call order.
        draw / redact (dc_net_track_frames_async_overlay): None, or dicts of the style arguments of `draw_people` / `redact_people` — the
        frames are then redacted and drawn into IN PLACE inside the chain, behind the tracker, from the people, cand and ids being handed
        back (the bytes of `redact_people` then `draw_people` on them), with no host wait: they must be writable, host frames ALL travel
        back, and they are the caller's again after `result()`.  A redact dict may carry only_ids / keep_ids (they need a tracker) and
        no `select`; `result()` then adds "redacted".
        labels (dc_net_track_frames_async_styles): None, True (LABEL_DEFAULTS) or a dict of the style arguments of `label_people`
        without `texts` and `stream` — the tracker's ids (without a tracker the people's indices) are written over the other two, the
        bytes of `label_people` on the people and ids handed back."""
        if edges is None:
            raise ValueError("track_frames_async needs the regression edges (deepcut_tools.read_pair_stats)")
        if tracker is not None:
            _tracker_handle(tracker)
        overlay = lst = None
        if draw is not None or redact is not None or labels is not None:
            lst, lalive = (None, None) if labels is None else _label_overlay_struct(labels)
            overlay = _overlay_args(draw, redact, tracker is not None, lst)
            overlay[4].append(lalive)
            if isinstance(frames_or_images, np.ndarray) and not (frames_or_images.dtype == np.uint8 and frames_or_images.flags.c_contiguous and
                                                                 frames_or_images.flags.writeable):
                raise ValueError("images that are drawn into must be a writable contiguous uint8 array")
        frames = _frame_list(frames_or_images)
        if frames is not None:
            arr, h, w, dev = _frame_array(frames)
            n, x, keep = len(frames), None, (arr, frames)
            if overlay is not None:
                _writable_frames(frames)  # ValueError for a host array that cannot be written
        else:
            x = np.ascontiguousarray(frames_or_images, dtype=np.uint8)
            if x.ndim == 3:
                x = x[None]
            if x.ndim != 4 or x.shape[3] != 3:
                raise ValueError("images must be uint8 [n,H,W,3] (BGR)")
            n, h, w, _ = x.shape
            arr, dev, keep = None, False, (x,)
        ch, cw = canvas_size(h, w, scale)
        self.blobs["data"].reshape(n, 3, ch, cw)
        self.reshape()
        j = self.blobs["prob"].shape[1]
        want_e = self.blobs["next_pred"].shape[1] // 2 if "next_pred" in self.blobs else None
        q, e, m, s, order = check_assembly(j, want_e, edges, mean, std, joint_order, scale if assemble_scale is None else assemble_scale,
                                           threshold, radius, max_det, max_cost, seed_threshold, max_people, min_joints)
        p = q.max_people
        # pinned outputs: the DMA engines move them.  In CPU mode there is no device to pin against, and the call below says so
        # (DC_ENOCPU) after the library's own argument checks
        # (pinning and unpinning cost more than the call and wait for the device: a collected request hands its arrays back)
        out = pinned_empty if _lib.dc_get_mode() == 1 else np.empty
        pools = self.__dict__.setdefault("_async_outputs", {})
        if len(pools) > 8:
            pools.clear()
        pool = pools.setdefault((n, p, j, tracker is not None), [])
        if pool:
            count, people, cand, ids, place = pool.pop()
        else:
            count, people, cand = out((n,), np.int32), out((n, p, j, 3), np.float64), out((n, p, j), np.int32)
            ids = place = None
            if tracker is not None:
                ids, place = out((n, p), np.int64), out((n, p), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        bridging = tracker is not None and _tracker_smoothing(tracker)
        args = (self._h, None if tracker is None else tracker._h, arr, ptr(x), n, h, w, float(scale), 1 if dev else 0,
                None if slot_of is None else ptr(_slot_map(slot_of, n)), C.byref(q), e.shape[0], ptr(e), ptr(m), ptr(s), ptr(order), ptr(count),
                ptr(people), ptr(cand), ptr(ids), ptr(place))
        redacted = None
        with self._completing(complete, dedupe) as completed:
            if overlay is None:
                _check(_lib.dc_net_track_frames_async(*args))
            else:
                dst, rst, only, keep_ids, alive = overlay
                spare = self.__dict__.setdefault("_async_redacted", {}).setdefault((n, p), [])  # pinned once, like the other outputs
                redacted = None if rst is None else (spare.pop() if spare else out((n, p), np.int32))
                keep = keep + (alive, redacted)
                if lst is None:
                    _check(_lib.dc_net_track_frames_async_overlay(*(args + _overlay_c_args(dst, rst, only, keep_ids) + (ptr(redacted),))))
                else:
                    styles = _overlay_styles_struct(dst, rst, lst, only, keep_ids)
                    keep = keep + (lst, styles)
                    _check(_lib.dc_net_track_frames_async_styles(*(args + (C.byref(styles), ptr(redacted)))))
        return TrackedFrames(self, tracker is not None, count, people, cand, ids, place, keep + (tracker,), pool, completed, bridging, redacted)

    def _assemble_people(self, tracker, scale, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people, min_joints,
                         joint_order, return_cost, slot_of=None, complete=None, dedupe=None):
        if edges is None:
            raise ValueError("assemble_people needs the regression edges (deepcut_tools.read_pair_stats)")
        n, j = self.blobs["prob"].shape[:2]
        want_e = self.blobs["next_pred"].shape[1] // 2 if "next_pred" in self.blobs else None
        q, e, m, s, order = check_assembly(j, want_e, edges, mean, std, joint_order, scale, threshold, radius, max_det, max_cost, seed_threshold,
                                           max_people, min_joints)
        p, md = q.max_people, q.max_det
        count = np.zeros(n, np.int32)
        people = np.zeros((n, p, j, 3), np.float64)
        cand = np.zeros((n, p, j), np.int32)
        cost = np.zeros((n, j, j, md, md), np.float64) if return_cost else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        bridging = tracker is not None and _tracker_smoothing(tracker)
        with self._completing(complete, dedupe) as completed:
            if tracker is None:
                _check(_lib.dc_net_assemble_people(self._h, C.byref(q), e.shape[0], ptr(e), ptr(m), ptr(s), ptr(order), ptr(count), ptr(people),
                                                   ptr(cand), ptr(cost)))
            else:
                ids, place = np.full((n, p), -1, np.int64), np.full((n, p), -1, np.int32)
                if slot_of is None:
                    _check(_lib.dc_net_track_people(self._h, _tracker_handle(tracker), C.byref(q), e.shape[0], ptr(e), ptr(m), ptr(s),
                                                    ptr(order), ptr(count), ptr(people), ptr(cand), ptr(cost), ptr(ids), ptr(place)))
                else:
                    _check(_lib.dc_net_track_people_slots(self._h, _tracker_handle(tracker), ptr(_slot_map(slot_of, n)), C.byref(q),
                                                          e.shape[0], ptr(e), ptr(m), ptr(s), ptr(order), ptr(count), ptr(people), ptr(cand),
                                                          ptr(cost), ptr(ids), ptr(place)))
        out = []
        for b in range(n):
            d = {"people": people[b, :count[b]].copy(), "cand": cand[b, :count[b]].copy()}
            if completed:
                d["filled"] = d["cand"] == -2
            if bridging:
                d["bridged"] = d["cand"] == -3
            if return_cost:
                d["cost"] = cost[b]
            if tracker is not None:
                d["ids"], d["place"] = ids[b, :count[b]].copy(), place[b, :count[b]].copy()
            out.append(d)
        return out

    def clone(self):
        """A second executor of the same model (own activations / stream / graph) sharing the parameters and
        the packed weights in HBM with this net."""
        h = C.c_void_p()
        _check(_lib.dc_net_clone(self._h, C.byref(h)))
        return Net(None, _handle=h)

    def synchronize(self):
        _check(_lib.dc_net_synchronize(self._h))

    def busy(self):
        """True while work enqueued on the net's own stream (stream="own") has not finished (non-blocking)."""
        b = C.c_int()
        _check(_lib.dc_net_busy(self._h, C.byref(b)))
        return bool(b.value)

    STAT_NAMES = ("lowerings", "graph_instantiations", "plan_hits", "autotune_runs", "buffer_growths", "repacks",
                  "cached_plans", "sparse_packs")

    def stats(self):
        """Counters of the per-shape plan cache (dc_net_stats): dict name -> int."""
        v = (C.c_longlong * len(self.STAT_NAMES))()
        _check(_lib.dc_net_stats(self._h, v, len(self.STAT_NAMES)))
        return dict(zip(self.STAT_NAMES, [int(x) for x in v]))

    def reserve(self, n, h, w):
        """Lower, allocate and tune the plan of an [n,3,h,w] input without running it (largest shape of a pyramid first:
        nothing grows afterwards, so no captured graph goes stale)."""
        _check(_lib.dc_net_reserve(self._h, int(n), int(h), int(w)))

    @property
    def device(self):
        """HIP device this net executes on (-1 before its first device use)."""
        return _lib.dc_net_device(self._h)

    def flops(self):
        v = C.c_double()
        _check(_lib.dc_net_flops(self._h, C.byref(v)))
        return v.value

    def num_launches(self):
        return _lib.dc_net_num_launches(self._h)

    def debug_info(self):
        """The reference's `debug_info` log of the last forward (net.cpp:648-681): mean |x| per top / parameter blob."""
        t = _lib.dc_net_debug_info(self._h)
        if t is None:
            raise DeepcutError(-1, (_lib.dc_last_error() or b"").decode())
        return t.decode()

    def tune_report(self):
        """Tile choices of the current shape: [{signature, tile, launches, timed: [(tile, us alone), ...]}] in plan order."""
        t = _lib.dc_net_tune_report(self._h)
        if t is None:
            raise DeepcutError(-1, (_lib.dc_last_error() or b"").decode())
        out = []
        for ln in t.decode().splitlines():
            f = ln.split("\t")
            if len(f) < 3:
                continue
            timed = [(c.rsplit(":", 1)[0], float(c.rsplit(":", 1)[1])) for c in (f[3].split() if len(f) > 3 else [])]
            out.append({"signature": f[0], "tile": f[1], "launches": int(f[2]), "timed": timed})
        return out

    def set_tile(self, signature, tile):
        """Override the tile of one GEMM signature in this executor's current plan (and the table shared with its clones)."""
        _check(_lib.dc_net_set_tile(self._h, signature.encode(), tile.encode()))

    def plan_text(self):
        t = _lib.dc_net_plan_text(self._h)
        if t is None:
            _check(-1)
        return t.decode()

    def profile_text(self, iters=10):
        t = _lib.dc_net_profile_text(self._h, iters)
        if t is None:
            raise DeepcutError(-1, (_lib.dc_last_error() or b"").decode())
        return t.decode()


class NetGroup(_Completing):
    """Several executors of ONE model (a net and its clones), each at its own input shape, run as ONE launch sequence
    (dc_group_*): launch i of the group is launch i of every member merged into a multi-problem gather-GEMM.  The scale
    loop of the demo (python/pose/estimate_pose.py:81-128) as one forward: `NetGroup.for_shapes(net, [(8, 272, 368), ...])`.
    Members stay usable on their own; after a grouped forward their blobs hold the results (decode_pose, detect_parts,
    emit_maps_device on a member see them)."""

    STAT_NAMES = ("merges", "graph_instantiations", "autotune_runs", "plan_hits", "launches", "multi_launches", "lanes")
    _set_completion, _get_completion = "dc_group_set_completion", "dc_group_get_completion"
    _set_dedupe, _get_dedupe = "dc_group_set_dedupe", "dc_group_get_dedupe"

    def __init__(self, nets, lanes=None):
        """lanes: None / 0 = automatic (the members are dealt largest-with-smallest to lanes that run concurrently on their own
        streams: two members -> two lanes, i.e. plain concurrency; three -> one lane; four and more -> two lanes of merged members),
        n = that many."""
        self.nets = list(nets)
        arr = (C.c_void_p * len(self.nets))(*[n._h for n in self.nets])
        h = C.c_void_p()
        _check(_lib.dc_group_create(arr, len(self.nets), C.byref(h)))
        self._h = h
        if lanes:
            self.set_lanes(lanes)

    def set_lanes(self, lanes):
        _check(_lib.dc_group_set_lanes(self._h, int(lanes or 0)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.dc_group_destroy(h)  # (the members are kept alive by self.nets until here)

    @classmethod
    def for_shapes(cls, net, shapes, lanes=None):
        """`net` and len(shapes) - 1 clones, member c reserved at shapes[c] = (n, h, w)."""
        nets = [net] + [net.clone() for _ in shapes[1:]]
        for m, (n, h, w) in zip(nets, shapes):
            m.reserve(n, h, w)
        return cls(nets, lanes=lanes)

    def __len__(self):
        return len(self.nets)

    @staticmethod
    def _ptrs(ps, k):
        if ps is None:
            return None
        return (C.c_void_p * k)(*[C.c_void_p(p or 0) for p in ps])

    @staticmethod
    def _ints(v):
        return (C.c_int * len(v))(*[int(x) for x in v])

    def forward_device(self, in_ptrs, shapes, prob_ptrs=None, loc_ptrs=None, next_ptrs=None, stream=None):
        """Device-resident: member c forwards the NCHW float32 batch at in_ptrs[c] of shapes[c] = (n, h, w); output
        pointer lists (or entries) may be None.  Asynchronous on `stream` when given ("own" = the first member's)."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        k = len(self.nets)
        if len(in_ptrs) != k or len(shapes) != k:
            raise ValueError("one input and one shape per group member")
        _check(_lib.dc_group_forward_batch(self._h, self._ptrs(in_ptrs, k), self._ints([s[0] for s in shapes]), self._ints([s[1] for s in shapes]),
                                           self._ints([s[2] for s in shapes]), 1, self._ptrs(prob_ptrs, k), self._ptrs(loc_ptrs, k),
                                           self._ptrs(next_ptrs, k), C.c_void_p(stream or 0)))

    def forward_batch(self, images, want=("prob", "loc_pred", "next_pred")):
        """images: one float32 [n,3,H,W] host array per member -> one dict of NCHW host arrays per member."""
        k = len(self.nets)
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in images]
        if len(xs) != k:
            raise ValueError("one batch per group member")
        outs = []
        for m, x in zip(self.nets, xs):
            n, c, h, w = x.shape
            m.blobs["data"].reshape(n, c, h, w)
            m.reshape()
            outs.append({key: m._out_array(key, m.blobs[key].shape) for key in ("prob", "loc_pred", "next_pred") if key in want})

        def col(key):
            return self._ptrs([o[key].ctypes.data if key in o else None for o in outs], k)

        _check(_lib.dc_group_forward_batch(self._h, self._ptrs([x.ctypes.data for x in xs], k), self._ints([x.shape[0] for x in xs]),
                                           self._ints([x.shape[2] for x in xs]), self._ints([x.shape[3] for x in xs]), 0, col("prob"),
                                           col("loc_pred"), col("next_pred"), None))
        return outs

    def forward_images(self, images, scales, want=("prob", "loc_pred"), pose=True, mirror=None):
        """images: ONE uint8 [n,H,W,3] BGR host array (every member sees it, member c at scales[c] — the demo's pyramid), or a
        list of one array per member.  -> one dict per member with the requested maps and "pose" [n,5,J].
        mirror: one 0/1 per member; a marked member sees its images flipped left to right, flipped by the pre-processing on the device
        (dc_group_forward_images_mirrored), and returns its RAW maps, in the flipped image's frame (`fuse_maps(mirror=...)` undoes the
        flip).  No pose is decoded then: a mirrored member's own pose would be in flipped coordinates, so pose=True is refused.
        A `Frame` or a list of `Frame`s is ONE batch of video frames that every member sees (dc_group_forward_frames); host frames
        are uploaded once for the whole group."""
        k = len(self.nets)
        if mirror is not None:
            mirror = [int(bool(v)) for v in mirror]
            if len(mirror) != k:
                raise ValueError("one mirror flag per group member: %d flags for %d members" % (len(mirror), k))
            if pose:
                raise ValueError("forward_images(mirror=...) decodes no pose (a mirrored member's would be in flipped coordinates): pass pose=False")
        frames = _frame_list(images)
        if frames is not None:  # one batch of video frames that every member sees (dc_group_forward_frames)
            return self._forward_frames(frames, scales, want, pose, mirror)
        if isinstance(images, np.ndarray):
            images = [images] * k
        xs = [np.ascontiguousarray(x, dtype=np.uint8) for x in images]
        xs = [x[None] if x.ndim == 3 else x for x in xs]
        if len(xs) != k or len(scales) != k:
            raise ValueError("one image batch and one scale per group member")
        outs = []
        for m, x, sc in zip(self.nets, xs, scales):
            n, h, w, _ = x.shape
            ch, cw = canvas_size(h, w, sc)
            m.blobs["data"].reshape(n, 3, ch, cw)
            m.reshape()
            o = {key: m._out_array(key, m.blobs[key].shape) for key in ("prob", "loc_pred", "next_pred") if key in want}
            if pose:
                o["pose"] = np.empty((n, 5, m.blobs["prob"].shape[1]), np.float64)
            outs.append(o)

        def col(key):
            return self._ptrs([o[key].ctypes.data if key in o else None for o in outs], k)

        if mirror is not None:
            _check(_lib.dc_group_forward_images_mirrored(self._h, self._ptrs([x.ctypes.data for x in xs], k), self._ints([x.shape[0] for x in xs]),
                                                         self._ints([x.shape[1] for x in xs]), self._ints([x.shape[2] for x in xs]),
                                                         (C.c_double * k)(*[float(s) for s in scales]), self._ints(mirror), 0, col("prob"),
                                                         col("loc_pred"), col("next_pred"), None))
            return outs
        _check(_lib.dc_group_forward_images(self._h, self._ptrs([x.ctypes.data for x in xs], k), self._ints([x.shape[0] for x in xs]),
                                            self._ints([x.shape[1] for x in xs]), self._ints([x.shape[2] for x in xs]),
                                            (C.c_double * k)(*[float(s) for s in scales]), 0, col("prob"), col("loc_pred"), col("next_pred"),
                                            col("pose"), None))
        return outs

    def _forward_frames(self, frames, scales, want, pose, mirror):
        k = len(self.nets)
        if len(scales) != k:
            raise ValueError("one scale per group member")
        arr, h, w, dev = _frame_array(frames)
        n = len(frames)
        outs = []
        for m, sc in zip(self.nets, scales):
            ch, cw = canvas_size(h, w, sc)
            m.blobs["data"].reshape(n, 3, ch, cw)
            m.reshape()
            o = {}
            if not dev:
                o = {key: m._out_array(key, m.blobs[key].shape) for key in ("prob", "loc_pred", "next_pred") if key in want}
                if pose:
                    o["pose"] = np.empty((n, 5, m.blobs["prob"].shape[1]), np.float64)
            outs.append(o)

        def col(key):
            return None if dev else self._ptrs([o[key].ctypes.data if key in o else None for o in outs], k)

        _check(_lib.dc_group_forward_frames(self._h, self._ptrs([C.addressof(arr)] * k, k), self._ints([n] * k), self._ints([h] * k),
                                            self._ints([w] * k), (C.c_double * k)(*[float(s) for s in scales]),
                                            None if mirror is None else self._ints(mirror), 1 if dev else 0, col("prob"), col("loc_pred"),
                                            col("next_pred"), col("pose"), None))
        if dev:  # the forward is complete: every member's maps and pose to the host
            for m, sc, o in zip(self.nets, scales, outs):
                o.update(m._host_maps(want))
                if pose:
                    o["pose"] = m.decode_pose(sc)
        return outs

    def forward_boxes(self, image, boxes, pyramid, scales=1.0, canvas=None, want=("prob", "loc_pred"), pose=True, mirror=None):
        """Net.forward_boxes over an image pyramid, as ONE grouped forward: member c takes box i at scales[i] * pyramid[c] on a
        canvas of member_canvas(canvas, pyramid[c]); canvas None = the smallest base canvas that fits every box at scales[i].
        -> one dict per member with the requested maps and "pose" [n,5,J] in image coordinates.
        mirror: one 0/1 per member; a marked member pre-processes every crop flipped left to right on the device
        (dc_group_forward_boxes_mirrored) and returns its RAW maps, in the flipped crop's frame (`decode_boxes(mirror=...)` undoes the
        flip).  When it names a member, "pose" is absent from the result: a mirrored member's own pose would be in flipped coordinates.
        None or all zeros: exactly the unmirrored call."""
        k = len(self.nets)
        if mirror is not None:
            mirror = [int(bool(v)) for v in mirror]
            if len(mirror) != k:
                raise ValueError("one mirror flag per group member: %d flags for %d members" % (len(mirror), k))
            if not any(mirror):
                mirror = None
            else:
                pose = False
        frame = image if isinstance(image, Frame) else None  # a video frame (dc_group_forward_boxes_frame) in place of the array
        if frame is not None and frame.is_device and pose:
            raise ValueError("forward_boxes of a device frame returns maps only: pass pose=False")
        x = None if frame is not None else np.ascontiguousarray(image, dtype=np.uint8)
        if x is not None and (x.ndim != 3 or x.shape[2] != 3):
            raise ValueError("image must be uint8 [H,W,3] (BGR)")
        shape = frame.shape if frame is not None else x.shape
        pyr = [float(p) for p in pyramid]
        if len(pyr) != k:
            raise ValueError("one pyramid scale per group member")
        b, sc, (ch, cw) = check_boxes(shape, boxes, scales, canvas)
        n = b.shape[0]
        canv = [(member_canvas(ch, p), member_canvas(cw, p)) for p in pyr]
        for p, cv in zip(pyr, canv):
            check_boxes(shape, b, sc * p, cv)
        outs = []
        for m, (mh, mw) in zip(self.nets, canv):
            j = m.blobs["prob"].shape[1]
            if n == 0:
                o = {key: np.empty((0,), np.float32) for key in ("prob", "loc_pred", "next_pred") if key in want}
                if pose:
                    o["pose"] = np.empty((0, 5, j), np.float64)
                outs.append(o)
                continue
            m.blobs["data"].reshape(n, 3, mh, mw)
            m.reshape()
            o = {key: m._out_array(key, m.blobs[key].shape) for key in ("prob", "loc_pred", "next_pred") if key in want}
            if pose:
                o["pose"] = np.empty((n, 5, j), np.float64)
            outs.append(o)
        if n == 0:
            return outs

        def col(key):
            return self._ptrs([o[key].ctypes.data if key in o else None for o in outs], k)

        if frame is not None:
            dev = frame.is_device
            _check(_lib.dc_group_forward_boxes_frame(self._h, C.byref(frame.c_frame()), shape[0], shape[1], 1 if dev else 0,
                                                     b.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), n, (C.c_double * k)(*pyr), ch, cw,
                                                     None if mirror is None else self._ints(mirror), None if dev else col("prob"),
                                                     None if dev else col("loc_pred"), None if dev else col("next_pred"),
                                                     None if dev else col("pose"), None))
            if dev:  # the forward is complete: the arrays made above are filled from the members' maps
                outs = [m._host_maps(want) for m in self.nets]
            return outs
        if mirror is not None:
            _check(_lib.dc_group_forward_boxes_mirrored(self._h, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], 0,
                                                        b.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), n, (C.c_double * k)(*pyr), ch,
                                                        cw, self._ints(mirror), col("prob"), col("loc_pred"), col("next_pred"), None))
            return outs
        _check(_lib.dc_group_forward_boxes(self._h, x.ctypes.data_as(C.c_void_p), x.shape[0], x.shape[1], 0, b.ctypes.data_as(C.c_void_p),
                                           sc.ctypes.data_as(C.c_void_p), n, (C.c_double * k)(*pyr), ch, cw, col("prob"), col("loc_pred"),
                                           col("next_pred"), col("pose"), None))
        return outs

    def forward_images_device(self, img_ptrs, shapes, scales, prob_ptrs=None, loc_ptrs=None, next_ptrs=None, pose_ptrs=None, stream=None):
        """Device-resident form: img_ptrs[c] -> uint8 [n,H,W,3] of shapes[c] = (n, H, W) at scales[c]."""
        if stream == "own":
            stream = C.c_void_p(-1).value
        k = len(self.nets)
        _check(_lib.dc_group_forward_images(self._h, self._ptrs(img_ptrs, k), self._ints([s[0] for s in shapes]), self._ints([s[1] for s in shapes]),
                                            self._ints([s[2] for s in shapes]), (C.c_double * k)(*[float(s) for s in scales]), 1,
                                            self._ptrs(prob_ptrs, k), self._ptrs(loc_ptrs, k), self._ptrs(next_ptrs, k), self._ptrs(pose_ptrs, k),
                                            C.c_void_p(stream or 0)))

    def _scales(self, scales, base):
        """-> (float64 [M] array, base index): one scale per member; what the values must be is the library's to say."""
        sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
        if sc.shape[0] != len(self.nets):
            raise ValueError("one scale per group member: %d scales for %d members" % (sc.shape[0], len(self.nets)))
        return sc, int(base)

    def _mirror(self, mirror, image_width, joint_mirror, edges):
        """-> (pointer to a FuseMirror, the arrays it points into) for the dc_group_*_mirrored entries; mirror None: a null pointer,
        nobody is mirrored.  Only the lengths are checked here; what the values must be (a positive width, an involution, an unmirrored
        base, mirrored edges present) is the library's to say."""
        if mirror is None:
            return None, ()
        flags = np.ascontiguousarray([int(bool(v)) for v in mirror], dtype=np.int32)
        if flags.shape[0] != len(self.nets):
            raise ValueError("one mirror flag per group member: %d flags for %d members" % (flags.shape[0], len(self.nets)))
        pi = None if joint_mirror is None else np.ascontiguousarray(joint_mirror, dtype=np.int32).reshape(-1)
        j = self.nets[0].blobs["prob"].shape[1]
        if pi is not None and pi.shape[0] != j:
            raise ValueError("joint_mirror must name one joint per joint: %d entries for %d joints" % (pi.shape[0], j))
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        fm = FuseMirror(ptr(flags), int(image_width or 0), ptr(pi), 0 if e is None else e.shape[0], ptr(e))
        return C.pointer(fm), (flags, pi, e)

    def fuse_maps(self, scales, base=0, mean=None, std=None, want=("prob", "loc_pred", "next_pred"), mirror=None, image_width=None,
                  joint_mirror=None, edges=None):
        """The maps of the members' last forwards (member c holds the same images at scales[c]) fused on member `base`'s grid, on the
        device in one launch (dc_group_fuse_maps; the rule is in include/deepcut_hip.h and is this project's own: the reference stops at
        the maps).  Every member's map is sampled bilinearly at the base cells' image points, loc_pred and next_pred are converted
        into the base member's units (mean / std: the [E, 2] statistics of next_pred, None = 0 / 1), and the members are averaged.
        -> dict of float32 NCHW arrays on the base grid, whatever the members' element type.
        mirror: one 0/1 per member, marking the members that saw the image flipped left to right (`forward_images(mirror=...)`); then
        image_width (the pixels of the unscaled image), joint_mirror (the joint every joint becomes in the mirror, e.g.
        pose.MIRROR_MPII14) and — when next_pred is fused — edges ([E, 2], as assemble_people) are needed: the mirrored members are
        sampled at the reflected position, their channels permuted and the x components negated, still in the one launch
        (dc_group_fuse_maps_mirrored).  None: no member is mirrored, and the other three are not read."""
        sc, base = self._scales(scales, base)
        want = [k for k in ("prob", "loc_pred", "next_pred") if k in want]
        ref = self.nets[base if 0 <= base < len(self.nets) else 0]
        e = ref.blobs["next_pred"].shape[1] // 2 if "next_pred" in want else 0
        stats = []
        for name, v in (("mean", mean), ("std", std)):
            if v is None or "next_pred" not in want:
                stats.append(None)
                continue
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.size != 2 * e:
                raise ValueError("%s must be [E, 2] = [%d, 2], got shape %s" % (name, e, v.shape))
            stats.append(v)
        hw = ref.blobs["prob"].shape[2:]
        out = {k: np.empty(tuple(ref.blobs[k].shape[:2]) + tuple(hw), np.float32) for k in want}
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        fm, _keep = self._mirror(mirror, image_width, joint_mirror, edges if "next_pred" in want else None)
        _check(_lib.dc_group_fuse_maps_mirrored(self._h, ptr(sc), base, fm, e, ptr(stats[0]), ptr(stats[1]), ptr(out.get("prob")),
                                                ptr(out.get("loc_pred")), ptr(out.get("next_pred")), 0, None))
        return out

    def detect_parts(self, scales, base=0, threshold=0.1, radius=1, max_det=32, mirror=None, image_width=None, joint_mirror=None):
        """Net.detect_parts on the fused `prob` and `loc_pred` of the members' last forwards, at scales[base] (dc_group_detect_parts).
        -> (counts int32 [n, J], dets float64 [n, J, max_det, 5] = x, y, score, cell row, cell column on the base member's grid).
        mirror / image_width / joint_mirror: as `fuse_maps` (dc_group_detect_parts_mirrored)."""
        sc, base = self._scales(scales, base)
        n, j = self.nets[0].blobs["prob"].shape[:2]
        counts = np.zeros((n, j), np.int32)
        dets = np.zeros((n, j, max(int(max_det), 0), 5), np.float64)
        fm, _keep = self._mirror(mirror, image_width, joint_mirror, None)
        _check(_lib.dc_group_detect_parts_mirrored(self._h, sc.ctypes.data_as(C.c_void_p), base, fm, float(threshold), int(radius), int(max_det),
                                                   counts.ctypes.data_as(C.c_void_p), dets.ctypes.data_as(C.c_void_p)))
        return counts, dets

    def draw_heatmap(self, frames, scales, base=None, origin=(0.0, 0.0), joints=None, mode="max", alpha=128, alpha_mode="score",
                     min_score=0.0, lut=None, palette=None, mirror=None, image_width=None, joint_mirror=None):
        """`Net.draw_heatmap` on the FUSED `prob` of the members' last forwards (dc_group_draw_heatmap): `prob` alone is fused on member
        `base`'s grid as `detect_parts` fuses it (base None: member 0) and blended at scales[base].  mirror / image_width / joint_mirror:
        as `fuse_maps` (dc_group_draw_heatmap_mirrored; the fused map is already un-mirrored).  The other arguments as `caffe.draw_heatmap`."""
        sc, base = self._scales(scales, 0 if base is None else base)
        arr, nb, h, w, is_device, _keep = _writable_frames(frames)
        st, _arrays = _heat_style(self.nets[0].blobs["prob"].shape[1], joints, mode, alpha, alpha_mode, min_score, lut, palette)
        fm, _keep2 = self._mirror(mirror, image_width, joint_mirror, None)
        _check(_lib.dc_group_draw_heatmap_mirrored(self._h, arr, nb, h, w, int(is_device), sc.ctypes.data_as(C.c_void_p), base, fm,
                                                   float(origin[0]), float(origin[1]), C.byref(st)))

    def decode_pose(self, scales, base=0, mirror=None, image_width=None, joint_mirror=None):
        """The single-person pose of every image of the members' last forwards from the FUSED maps (dc_group_decode_pose): `prob` and
        `loc_pred` are fused on member `base`'s grid as `detect_parts` fuses them, then decoded there at scales[base] as
        `Net.decode_pose` decodes a net's own maps.  -> float64 [n, 5, J].  Works on members narrowed to `prob` and `loc_pred`.
        mirror / image_width / joint_mirror: as `fuse_maps`.  The rule is this project's own (the reference keeps the best single scale)."""
        sc, base = self._scales(scales, base)
        n, j = self.nets[0].blobs["prob"].shape[:2]
        pose = np.empty((n, 5, j), np.float64)
        fm, _keep = self._mirror(mirror, image_width, joint_mirror, None)
        _check(_lib.dc_group_decode_pose(self._h, sc.ctypes.data_as(C.c_void_p), base, fm, pose.ctypes.data_as(C.c_void_p), 0, None))
        return pose

    def decode_boxes(self, pyramid, base=0, mirror=None, joint_mirror=None, want=()):
        """The poses of the boxes of the members' last `forward_boxes` from the FUSED maps (dc_group_decode_boxes): `prob` and `loc_pred`
        of every member are fused on member `base`'s canvas — `pyramid` as the member scales; a mirrored member (`forward_boxes(mirror=...)`,
        the same flags here) is sampled at every box's own reflected column — and decoded there as `forward_boxes` decodes a member's own
        maps: at scales[i] * pyramid[base], restricted to the crop's own cells, shifted by the box corner.
        -> dict: "pose" [n, 5, J] float64 in image coordinates, and the fused float32 maps named in `want` ("prob", "loc_pred")."""
        sc, base = self._scales(pyramid, base)
        ref = self.nets[base if 0 <= base < len(self.nets) else 0]
        n, j = ref.blobs["prob"].shape[:2]
        hw = tuple(ref.blobs["prob"].shape[2:])
        out = {k: np.empty((n, ref.blobs[k].shape[1]) + hw, np.float32) for k in ("prob", "loc_pred") if k in want}
        out["pose"] = np.empty((n, 5, j), np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        fm, _keep = self._mirror(mirror, 0, joint_mirror, None)
        _check(_lib.dc_group_decode_boxes(self._h, ptr(sc), base, fm, ptr(out.get("prob")), ptr(out.get("loc_pred")), ptr(out["pose"]), 0, None))
        return out

    def assemble_people(self, scales, base=0, threshold=0.1, radius=1, max_det=16, edges=None, mean=None, std=None, max_cost=32.0,
                        seed_threshold=0.5, max_people=32, min_joints=1, joint_order=None, return_cost=False, mirror=None, image_width=None,
                        joint_mirror=None, complete=None, dedupe=None):
        """Net.assemble_people on the fused maps of a pyramid (dc_group_assemble_people): the three maps of the members' last forwards
        are fused on member `base`'s grid (`fuse_maps`), then the candidates, the pair costs and the greedy assembly run on them at
        scales[base], all on the device with no host round trip in between.  The other arguments and the result are Net.assemble_people's.
        mirror / image_width / joint_mirror: as `fuse_maps`, with `edges` as the regression edges (dc_group_assemble_people_mirrored).
        complete, dedupe: as `Net.assemble_people`, on the group's own `completion` / `dedupe` (the members' settings are not read)."""
        return self._assemble_people(None, scales, base, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people,
                                     min_joints, joint_order, return_cost, mirror, image_width, joint_mirror, complete=complete, dedupe=dedupe)

    def track_people(self, tracker, scales, base=0, threshold=0.1, radius=1, max_det=16, edges=None, mean=None, std=None, max_cost=32.0,
                     seed_threshold=0.5, max_people=32, min_joints=1, joint_order=None, return_cost=False, mirror=None, image_width=None,
                     joint_mirror=None, slot_of=None, complete=None, dedupe=None):
        """`assemble_people` with the identities of a `caffe.Tracker` (dc_group_track_people), plain or mirrored: the tracker's update
        runs on the device behind the assembly of the fused maps.  The arguments and the result are `assemble_people`'s, unchanged,
        plus "ids" and "place" per image as `Net.track_people` gives them.  slot_of: as `Net.track_people` (dc_group_track_people_slots)."""
        _tracker_handle(tracker)
        return self._assemble_people(tracker, scales, base, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people,
                                     min_joints, joint_order, return_cost, mirror, image_width, joint_mirror, slot_of, complete, dedupe)

    def _assemble_people(self, tracker, scales, base, threshold, radius, max_det, edges, mean, std, max_cost, seed_threshold, max_people,
                         min_joints, joint_order, return_cost, mirror, image_width, joint_mirror, slot_of=None, complete=None, dedupe=None):
        if edges is None:
            raise ValueError("assemble_people needs the regression edges (deepcut_tools.read_pair_stats)")
        sc, base = self._scales(scales, base)
        ref = self.nets[0]
        n, j = ref.blobs["prob"].shape[:2]
        want_e = ref.blobs["next_pred"].shape[1] // 2 if "next_pred" in ref.blobs else None
        q, e, m, s, order = check_assembly(j, want_e, edges, mean, std, joint_order, 1.0, threshold, radius, max_det, max_cost, seed_threshold,
                                           max_people, min_joints)
        p, md = q.max_people, q.max_det
        count = np.zeros(n, np.int32)
        people = np.zeros((n, p, j, 3), np.float64)
        cand = np.zeros((n, p, j), np.int32)
        cost = np.zeros((n, j, j, md, md), np.float64) if return_cost else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        fm, _keep = self._mirror(mirror, image_width, joint_mirror, e)
        bridging = tracker is not None and _tracker_smoothing(tracker)
        with self._completing(complete, dedupe) as completed:
            if tracker is None:
                _check(_lib.dc_group_assemble_people_mirrored(self._h, ptr(sc), base, fm, C.byref(q), e.shape[0], ptr(e), ptr(m), ptr(s),
                                                              ptr(order), ptr(count), ptr(people), ptr(cand), ptr(cost)))
            else:
                ids, place = np.full((n, p), -1, np.int64), np.full((n, p), -1, np.int32)
                if slot_of is None:
                    _check(_lib.dc_group_track_people(self._h, _tracker_handle(tracker), ptr(sc), base, fm, C.byref(q), e.shape[0], ptr(e),
                                                      ptr(m), ptr(s), ptr(order), ptr(count), ptr(people), ptr(cand), ptr(cost), ptr(ids),
                                                      ptr(place)))
                else:
                    _check(_lib.dc_group_track_people_slots(self._h, _tracker_handle(tracker), ptr(_slot_map(slot_of, n)), ptr(sc), base, fm,
                                                            C.byref(q), e.shape[0], ptr(e), ptr(m), ptr(s), ptr(order), ptr(count),
                                                            ptr(people), ptr(cand), ptr(cost), ptr(ids), ptr(place)))
        out = []
        for b in range(n):
            d = {"people": people[b, :count[b]].copy(), "cand": cand[b, :count[b]].copy()}
            if completed:
                d["filled"] = d["cand"] == -2
            if bridging:
                d["bridged"] = d["cand"] == -3
            if return_cost:
                d["cost"] = cost[b]
            if tracker is not None:
                d["ids"], d["place"] = ids[b, :count[b]].copy(), place[b, :count[b]].copy()
            out.append(d)
        return out

    def synchronize(self):
        self.nets[0].synchronize()

    def plan_text(self):
        t = _lib.dc_group_plan_text(self._h)
        if t is None:
            _check(-1)
        return t.decode()

    def tune_report(self):
        """As Net.tune_report, for the merged launches of the last forward's plan."""
        t = _lib.dc_group_tune_report(self._h)
        if t is None:
            _check(-1)
        out = []
        for ln in t.decode().splitlines():
            f = ln.split("\t")
            if len(f) < 3:
                continue
            timed = [(c.rsplit(":", 1)[0], float(c.rsplit(":", 1)[1])) for c in (f[3].split() if len(f) > 3 else [])]
            out.append({"signature": f[0], "tile": f[1], "launches": int(f[2]), "timed": timed})
        return out

    def set_tile(self, signature, tile):
        _check(_lib.dc_group_set_tile(self._h, signature.encode(), tile.encode()))

    def profile_text(self, iters=10):
        t = _lib.dc_group_profile_text(self._h, int(iters))
        if t is None:
            _check(-1)
        return t.decode()

    def stats(self):
        v = (C.c_longlong * len(self.STAT_NAMES))()
        _check(_lib.dc_group_stats(self._h, v, len(self.STAT_NAMES)))
        return dict(zip(self.STAT_NAMES, [int(x) for x in v]))

    def flops(self):
        f = C.c_double()
        _check(_lib.dc_group_flops(self._h, C.byref(f)))
        return f.value


class Comm(object):
    """In-process multi-GPU forward (dc_comm_create / dc_forward_batch): `nets[k]` runs on `devices[k]` on a host thread of its own
    inside the library; images are dealt longest-processing-time-first over H*W, the maps gathered on the root executor's device
    (RCCL ncclSend / ncclRecv opened with dlopen, or peer copies — `transport`: "auto", "rccl", "peer") and returned as host arrays."""

    TRANSPORTS = {"auto": 0, "rccl": 1, "peer": 2}

    def __init__(self, nets, devices=None, transport="auto"):
        self.nets = list(nets)
        k = len(self.nets)
        dev = None if devices is None else (C.c_int * k)(*[int(d) for d in devices])
        h = C.c_void_p()
        _check(_lib.dc_comm_create(k, dev, self.TRANSPORTS[transport], C.byref(h)))
        self._h = h
        self._fin = __import__("weakref").finalize(self, _lib.dc_comm_destroy, C.c_void_p(h.value))

    @property
    def transport(self):
        t = _lib.dc_comm_transport(self._h)
        return {1: "rccl", 2: "peer"}.get(t, t)

    def forward(self, images, want=("prob", "loc_pred", "next_pred"), pinned=False, out=None):
        """images: a list of float32 [3,H,W] host arrays (shapes may differ) -> a list of dicts of [C,h,w] host arrays.
        pinned=True: the result arrays are pinned host memory (caffe.pinned_empty) — the library then downloads every map straight
        into them on the DMA engines, no scatter copy; images that are pinned arrays themselves are uploaded in place likewise.
        out: the list a previous call returned (same images' shapes, same `want`): its arrays are written again instead of new ones
        being made — page-locking 10 MB per image on every call costs more than the copies it saves."""
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in images]
        n, k = len(xs), len(self.nets)
        if any(x.ndim != 3 or x.shape[0] != 3 for x in xs):
            raise ValueError("dc_forward_batch takes [3,H,W] images")
        hw = (C.c_int * 2 * max(n, 1))()
        for i, x in enumerate(xs):
            hw[i][0], hw[i][1] = x.shape[1], x.shape[2]
        # the maps' shapes come from the net's own shape inference (host only), once per distinct image shape: the library
        # writes C x h x w floats per map, so the arrays must be exactly that
        dims = self.__dict__.setdefault("_map_dims", {})
        for x in xs:
            hw_ = (x.shape[1], x.shape[2])
            if hw_ not in dims:
                m0 = self.nets[0]
                m0.blobs["data"].reshape(1, 3, *hw_)
                m0.reshape()
                dims[hw_] = {key: tuple(m0.blobs[key].shape[1:]) for key in ("prob", "loc_pred", "next_pred")}
        mk = pinned_empty if pinned else (lambda shape: np.empty(shape, np.float32))
        if out is not None:
            if len(out) != n or any(set(o) != set(want) or any(tuple(o[key].shape) != tuple(dims[(x.shape[1], x.shape[2])][key]) or o[key].dtype != np.float32
                                                                 or not o[key].flags["C_CONTIGUOUS"] for key in want) for o, x in zip(out, xs)):
                raise ValueError("out= must be the result list of a call with the same image shapes and `want`")
            outs = out
        else:
            outs = [{key: mk(dims[(x.shape[1], x.shape[2])][key]) for key in want} for x in xs]

        def col(key):
            if key not in want:
                return None
            return (C.c_void_p * max(n, 1))(*[C.c_void_p(o[key].ctypes.data) for o in outs])

        _check(_lib.dc_forward_batch(self._h, (C.c_void_p * k)(*[m._h for m in self.nets]), k,
                                     (C.c_void_p * max(n, 1))(*[C.c_void_p(x.ctypes.data) for x in xs]), hw, n, col("prob"), col("loc_pred"), col("next_pred")))
        return outs

    def executor_of(self, i):
        r = _lib.dc_comm_item_executor(self._h, int(i))
        if r < 0:
            _check(r)
        return r

    def root_maps(self, i):
        """Device pointers (on the root executor's device) and dims of image i's gathered maps: (prob, loc_pred, next_pred, dims)."""
        p, l, x = C.c_void_p(), C.c_void_p(), C.c_void_p()
        dims = (C.c_int * 5)()
        _check(_lib.dc_comm_root_maps(self._h, int(i), C.byref(p), C.byref(l), C.byref(x), dims))
        return p.value, l.value, x.value, list(dims)
