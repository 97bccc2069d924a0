"""Several people in one image, bottom-up: one forward, then the part candidates, the pair costs from `next_pred` and a greedy
assembly on the device (`caffe.Net.assemble_people`).

NO REFERENCE COUNTERPART: the reference's python/pose stops at `estimate_pose` (one person) and its repository has no consumer of
`next_pred`.  The grouping rule is this project's own (include/deepcut_hip.h, dc_net_assemble_people)."""
import numpy as _np

_MODEL = {}


def _get_model(model_def, model_bin):
    # a cache of its own: `estimate_pose` narrows the outputs of ITS cached net to `prob` and `loc_pred`, this entry needs all three
    import caffe as _caffe

    key = (model_def, model_bin)
    if key not in _MODEL:
        _MODEL[key] = _caffe.Net(model_def, model_bin, _caffe.TEST)
    return _MODEL[key]


def estimate_people(image, model_def, model_bin, stats, scale=1.0, net=None, **assembly):
    """image: HxWx3 BGR uint8.  stats: the path of the model's pair-statistics file (deepcut_tools.read_pair_stats) or the
    (edges, mean, std) triple itself.  Runs the image entry (`Net.forward_images`: pre-processing on the device) with all three
    outputs computed, then `Net.assemble_people(scale=scale, edges=..., mean=..., std=..., **assembly)`; `assembly` takes its other
    arguments (threshold, radius, max_det, max_cost, seed_threshold, max_people, min_joints, joint_order: the defaults of max_cost
    and seed_threshold are placeholders, not tuned on real images).
    -> float64 [m, J, 3]: x, y, score per person and joint in image coordinates, (0, 0, 0) where a person has no such joint.
    A caller-supplied `net` keeps its output selection: one that leaves `next_pred` out is refused, not changed."""
    if isinstance(stats, (str, bytes)) or hasattr(stats, "__fspath__"):
        from deepcut_tools import read_pair_stats

        stats = read_pair_stats(stats)
    edges, mean, std = stats
    if net is None:
        net = _get_model(model_def, model_bin)
    missing = [k for k in ("prob", "loc_pred", "next_pred") if k not in net.wanted_outputs]
    if missing:
        raise ValueError("estimate_people needs all three maps, the net leaves out %r (net.set_outputs(None) brings them back)" % (missing,))
    image = _np.asarray(image)
    if image.dtype != _np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image must be uint8 [H,W,3] (BGR)")
    net.forward_images(image, scale, want=(), pose=False)
    return net.assemble_people(scale=scale, edges=edges, mean=mean, std=std, **assembly)[0]["people"]


def people_boxes(people, image_shape, margin):
    """people: [m, J, 3] as `estimate_people` returns them; image_shape: (H, W[, 3]); margin: pixels added on every side.
    -> int32 [m, 4] boxes (x0, y0, x1, y1), half-open, around each person's assigned joints (score > 0), clipped to the image and
    at least one pixel wide and high: what `estimate_poses` / `Net.forward_boxes` accept, so the bottom-up result can seed the
    top-down entry without an external person detector.  A person without an assigned joint gets the whole image."""
    h, w = int(image_shape[0]), int(image_shape[1])
    p = _np.asarray(people, _np.float64)
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("people must be [m, J, 3] (x, y, score), got shape %s" % (p.shape,))
    out = _np.zeros((p.shape[0], 4), _np.int32)
    for i in range(p.shape[0]):
        have = p[i, :, 2] > 0
        if not have.any():
            out[i] = (0, 0, w, h)
            continue
        x, y = p[i, have, 0], p[i, have, 1]
        x0 = int(_np.clip(_np.floor(x.min() - margin), 0, w - 1))
        y0 = int(_np.clip(_np.floor(y.min() - margin), 0, h - 1))
        x1 = int(_np.clip(_np.ceil(x.max() + margin) + 1, x0 + 1, w))
        y1 = int(_np.clip(_np.ceil(y.max() + margin) + 1, y0 + 1, h))
        out[i] = (x0, y0, x1, y1)
    return out
