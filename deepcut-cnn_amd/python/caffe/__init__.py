"""`caffe` — drop-in pycaffe surface for the DeeperCut forward path on MI355X.

Mirrors what python/pose/estimate_pose.py and pose_demo.py use of the reference's pycaffe
(python/caffe/__init__.py:1-4, python/caffe/pycaffe.py, python/caffe/_caffe.cpp): `Net`, `Blob`,
`TEST`/`TRAIN`, `set_mode_cpu`, `set_mode_gpu`, `set_device`.  It is a ctypes binding of
libdeepcut_hip.so (include/deepcut_hip.h); there is no compute in Python and no CPU fallback:
`forward()` in CPU mode raises.
"""
from .pycaffe import Net, NetGroup, Tracker, TrackedFrames, Comm, Blob, Frame, csc_coefficients, Layer, choose_streams, pinned_empty, lpt_schedule, set_mode_cpu, set_mode_gpu, set_device, device_count, canvas_size, check_boxes, member_canvas, check_assembly, pair_stats_read, conv_variants, conv_variants_bf16, wino_half_pack, wino_blocks, wino_cover, wino_mix_offered, stream1x1_pack, stream1x1f_pack, stream1x1f_rows, wino43_pack, stem7x7_pack, sparse_head_pack, lib_path  # noqa: F401
from .pycaffe import TRAIN, TEST, DeepcutError  # noqa: F401
from .pycaffe import dedupe_people, dedupe_params, DEDUPE_DEFAULTS  # noqa: F401
from .pycaffe import smooth_params, SMOOTH_DEFAULTS  # noqa: F401
from .pycaffe import draw_people, draw_limits, draw_coefficients, DRAW_JOINT_COLORS, DRAW_ID_COLORS  # noqa: F401
from .pycaffe import draw_heatmap, HEAT_LUT  # noqa: F401
from .pycaffe import redact_people, redact_select, REDACT_DEFAULTS  # noqa: F401
from .pycaffe import overlay_people_device  # noqa: F401
from .pycaffe import describe_people, appearance_params, APPEARANCE_DEFAULTS, APPEARANCE_BINS, TRACK_GALLERY  # noqa: F401
from .pycaffe import label_people, LABEL_FONT, LABEL_CHARS, LABEL_DEFAULTS, LABEL_MAX_CHARS  # noqa: F401

__version__ = "1.0.0-rc3+deepcut_hip"
