"""Several people in one image, bottom-up: one forward, then the part candidates, the pair costs from `next_pred` and a greedy
assembly on the device (`caffe.Net.assemble_people`); over an image pyramid, one grouped forward, then the maps of all scales
fused on the device and assembled there (`caffe.NetGroup.assemble_people`).

NO REFERENCE COUNTERPART: the reference's python/pose stops at `estimate_pose` (one person) and its repository has no consumer of
`next_pred`.  The grouping rule, the multi-scale fusion rule and its mirrored form (flip=True) are this project's own
(include/deepcut_hip.h, dc_net_assemble_people, dc_group_fuse_maps and dc_group_fuse_maps_mirrored); the reference mirrors nothing on
the pose path, so their parity is unpinned by the reference."""
import numpy as _np

_MODEL = {}

# The joint every joint becomes when the image is flipped left to right, in the MPII 14-joint order the DeeperCut models are trained on
# (right ankle, knee, hip; left hip, knee, ankle; right wrist, elbow, shoulder; left shoulder, elbow, wrist; upper neck; head top).  The
# reference's Python names no joints, so this table is the caller's to override (`joint_mirror=`) for a model with another joint order.
MIRROR_MPII14 = (5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13)
# The limbs `draw_people` draws between the joints of that order: the legs through the hips, the arms through the shoulders to the upper
# neck, neck to head top, and the trunk's two sides.  Like the mirror table it is the caller's to override (`edges=`).
SKELETON_MPII14 = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 12), (12, 9), (9, 10), (10, 11), (12, 13), (2, 8), (3, 9))
# The joint pair `redact_people` places the head disc on: (upper neck, head top).  The caller's to override (`head=`) likewise.
HEAD_MPII14 = (12, 13)
# The limbs `describe_people` samples a person's appearance under: shoulder to hip on either side, the shoulder line and the hip line.
# The caller's to override (`edges=`) likewise.
TORSO_MPII14 = ((8, 2), (9, 3), (8, 9), (2, 3))


def _get_model(model_def, model_bin):
    # a cache of its own: `estimate_pose` narrows the outputs of ITS cached net to `prob` and `loc_pred`, this entry needs all three
    import caffe as _caffe

    key = (model_def, model_bin)
    if key not in _MODEL:
        _MODEL[key] = _caffe.Net(model_def, model_bin, _caffe.TEST)
    return _MODEL[key]


_SPARSE_MODEL = {}


def _get_sparse_model(model_def, model_bin):
    # the sparse entry's own cache: a net narrowed to `prob` and `loc_pred` with the pairwise head evaluated at the candidates' cells
    import caffe as _caffe

    key = (model_def, model_bin)
    if key not in _SPARSE_MODEL:
        _SPARSE_MODEL[key] = _caffe.Net(model_def, model_bin, _caffe.TEST, want=["loc_pred", "prob"], sparse_pairwise=True)
    return _SPARSE_MODEL[key]


def _base_scale(scales):
    """The member a pyramid is fused on when the caller names none: the scale nearest 1.0, the first of equals."""
    return min(range(len(scales)), key=lambda i: (abs(float(scales[i]) - 1.0), i))


def _check_joint_mirror(joint_mirror):
    """-> the table as a list of ints; ValueError unless it is an involution of 0..J-1 (needs no net and no device)."""
    if joint_mirror is None:
        raise ValueError("flip=True needs joint_mirror (pose.MIRROR_MPII14 for the DeeperCut models)")
    pi = [int(v) for v in joint_mirror]
    for j, v in enumerate(pi):
        if not 0 <= v < len(pi):
            raise ValueError("joint_mirror[%d] = %d is outside [0, %d)" % (j, v, len(pi)))
        if pi[v] != j:
            raise ValueError("joint_mirror is not an involution: joint %d -> %d -> %d" % (j, v, pi[v]))
    return pi


def estimate_people(image, model_def, model_bin, stats, scale=1.0, net=None, scales=None, base=None, flip=False, joint_mirror=MIRROR_MPII14,
                    sparse=False, **assembly):
    """image: HxWx3 BGR uint8, or a `caffe.Frame` (NV12 / pitched BGR planes, converted by the device pre-processing).  stats: the path of the model's pair-statistics file (deepcut_tools.read_pair_stats) or the
    (edges, mean, std) triple itself.  Runs the image entry (`Net.forward_images`: pre-processing on the device) with all three
    outputs computed, then `Net.assemble_people(scale=scale, edges=..., mean=..., std=..., **assembly)`; `assembly` takes its other
    arguments (threshold, radius, max_det, max_cost, seed_threshold, max_people, min_joints, joint_order: the defaults of max_cost
    and seed_threshold are placeholders, not tuned on real images) and `complete` (None, True or a dict: joints the assembly missed are
    filled on the device from the pairwise predictions, `Net.completion`; its defaults are placeholders too) and `dedupe` (None, True or
    a dict: people who are there twice are suppressed on the device behind the completion, `Net.dedupe`; placeholders likewise).
    -> float64 [m, J, 3]: x, y, score per person and joint in image coordinates, (0, 0, 0) where a person has no such joint.
    A caller-supplied `net` keeps its output selection: one that leaves `next_pred` out is refused, not changed.
    scales: a list of scales runs the image pyramid instead — the net and clones of it kept with it, as `estimate_pose` uses them, in
    ONE grouped forward (`NetGroup.forward_images`), then `NetGroup.assemble_people`: the maps of all scales are fused on the grid of
    member `base` (None = the scale nearest 1.0, the first of equals) on the device and assembled there at scales[base].  `scale`
    must then be left at 1.0.
    sparse: True runs on a cached net of its own that computes `prob` and `loc_pred` only and evaluates the 364-channel pairwise head at
    the part candidates' cells (`Net.sparse_pairwise`; the rule: include/deepcut_hip.h, dc_net_pairwise_at) instead of over the whole map.
    A caller's `net` is used as given and never changed: it must either compute `next_pred` or have `sparse_pairwise` set.  Pyramids and
    mirrored members are out of scope for the sparse head: sparse=True with scales= or flip=True raises ValueError.
    The clones are the ones `estimate_pose` keeps with the net for its own pyramids; they are set to compute
    all three outputs here (after the net itself has been accepted: a net that leaves `next_pred` out is refused before anything is
    touched), and `estimate_pose` on its own cached net narrows its clones again — alternating the two entries on ONE net re-lowers the
    clones' plans at every switch, so give each entry a net of its own where both are in use.
    flip: mirror test-time augmentation — every scale is run on the image and on its left-right mirror and all the maps are fused: a single
    `scale` becomes a group of two, a pyramid of k scales a group of 2k (the k plain members, then their mirrors), still ONE grouped
    forward (the flip is part of the device pre-processing) and ONE `NetGroup.assemble_people`.  joint_mirror: the joint every joint
    becomes in the mirror (MIRROR_MPII14 by default: the caller's to override for another joint order); `stats` must hold, for every edge
    (a, c), the edge (joint_mirror[a], joint_mirror[c]).  The base stays a plain member: None = the plain scale nearest 1.0."""
    return _people_of_image(None, image, model_def, model_bin, stats, scale, net, scales, base, flip, joint_mirror, sparse, assembly)["people"]


def draw_people(frame, people, ids=None, **style):
    """Draw people into a frame IN PLACE on the device: `caffe.draw_people` with the MPII skeleton (`SKELETON_MPII14`) for `edges` unless
    the caller names another.  frame: a writable uint8 [H, W, 3] BGR array or a `caffe.Frame` (NV12 / BGR24, host or device); people:
    [m, J, 3] as `estimate_people` / `track_people` return them; ids: int64 [m] or None; style: what `caffe.draw_people` takes (cand,
    edges, joint_radius, limb_radius, alpha, alpha_filled, min_score, color, palette, untracked, stream).  PARITY UNPINNED BY THE
    REFERENCE: the drawing rule is this project's own (include/deepcut_hip.h, dc_draw_people)."""
    import caffe as _caffe

    style.setdefault("edges", SKELETON_MPII14)
    _caffe.draw_people(frame, _np.asarray(people, _np.float64), ids=ids, **style)


def draw_heatmap(frame, scores, scale, **style):
    """Blend a score map into a frame IN PLACE on the device: `caffe.draw_heatmap` with the demo's joint colours
    (`caffe.DRAW_JOINT_COLORS`) for `palette` unless the caller names another.  frame: a writable uint8 [H, W, 3] BGR array or a
    `caffe.Frame`; scores: float32 [J, Hm, Wm] (`net.blobs["prob"].data[0]`); scale: what the forward ran at; style: what
    `caffe.draw_heatmap` takes (origin, joints, mode, alpha, alpha_mode, min_score, lut, palette, stream).  PARITY UNPINNED BY THE
    REFERENCE: the blending rule is this project's own (include/deepcut_hip.h, dc_draw_heatmap)."""
    import caffe as _caffe

    style.setdefault("palette", _caffe.DRAW_JOINT_COLORS)
    _caffe.draw_heatmap(frame, _np.asarray(scores, _np.float32), scale, **style)


def redact_people(frame, people, ids=None, **style):
    """Redact people in a frame IN PLACE on the device: `caffe.redact_people` with the MPII head pair (`HEAD_MPII14`: upper neck, head
    top) for `head` and the MPII skeleton (`SKELETON_MPII14`) for `edges` unless the caller names others.  frame, people, ids: as
    `draw_people` takes them; style: what `caffe.redact_people` takes (select, only_ids, keep_ids, region, head_scale, body_scale,
    min_radius, max_radius, min_score, effect, block, fill, stream; the scale and radius defaults are PLACEHOLDERS, not tuned on real
    video).  -> int32 [m]: 1 where a region was made for the person — with region "head" a person whose neck or head top is missing is
    NOT redacted.  PARITY UNPINNED BY THE REFERENCE: the rule is this project's own (include/deepcut_hip.h, dc_redact_people)."""
    import caffe as _caffe

    style.setdefault("head", HEAD_MPII14)
    style.setdefault("edges", SKELETON_MPII14)
    return _caffe.redact_people(frame, _np.asarray(people, _np.float64), ids=ids, **style)


def describe_people(frame, people, **style):
    """What people look like, counted from a frame on the device: `caffe.describe_people` with the MPII torso (`TORSO_MPII14`) for
    `edges` unless the caller names another.  frame: a uint8 [H, W, 3] BGR array or a `caffe.Frame` (NV12 / BGR24, host or device), only
    read; people: [m, J, 3] as `estimate_people` / `track_people` return them; style: what `caffe.describe_people` takes (edges, scale,
    min_radius, min_score, stream; the defaults, `caffe.APPEARANCE_DEFAULTS`, are PLACEHOLDERS, not tuned on real video).
    -> int32 [m, 3, 16].  PARITY UNPINNED BY THE REFERENCE: the rule is this project's own (include/deepcut_hip.h, dc_describe_people)."""
    import caffe as _caffe

    style.setdefault("edges", TORSO_MPII14)
    return _caffe.describe_people(frame, _np.asarray(people, _np.float64), **style)


def label_people(frame, people, ids=None, **style):
    """Write people's ids into a frame IN PLACE on the device: `caffe.label_people`.  frame, people: as `draw_people` takes them; ids:
    int64 [m] as `track_people` returns them, or None (the people's indices are written); an id < 0 gets no label.  style: what
    `caffe.label_people` takes (texts, scale, gap, anchor, prefix, alpha_text, alpha_plate, min_score, color, palette, text_color,
    plate_color, stream; the defaults, `caffe.LABEL_DEFAULTS`, are PLACEHOLDERS).  PARITY UNPINNED BY THE REFERENCE: the rule is this
    project's own (include/deepcut_hip.h, dc_label_people)."""
    import caffe as _caffe

    _caffe.label_people(frame, _np.asarray(people, _np.float64), ids=ids, **style)


def _label_style(labels):
    """labels= of `track_people` / `VideoPipeline` -> None (off) or the style dict."""
    if labels is None or labels is False:
        return None
    if labels is True:
        return {}
    if not isinstance(labels, dict):
        raise ValueError("labels must be None, True or a dict of what label_people takes, got %r" % (labels,))
    return dict(labels)


def _redact_style(redact):
    """redact= of `track_people` / `VideoPipeline` -> None (off) or the style dict."""
    if redact is None or redact is False:
        return None
    if redact is True:
        return {}
    if not isinstance(redact, dict):
        raise ValueError("redact must be None, True or a dict of what redact_people takes, got %r" % (redact,))
    return dict(redact)


def _draw_style(draw):
    """draw= of `track_people` / `VideoPipeline` -> None (off) or the style dict."""
    if draw is None or draw is False:
        return None
    if draw is True:
        return {}
    if not isinstance(draw, dict):
        raise ValueError("draw must be None, True or a dict of what draw_people takes, got %r" % (draw,))
    return dict(draw)


def track_people(frames, model_def, model_bin, stats, tracker=None, depth=1, batch=1, assign="greedy", smooth=None, draw=None, redact=None,
                 in_chain=False, labels=None, appearance=None, **kw):
    """`estimate_people` over the frames of a video, with identities: a generator over an iterable of images (HxWx3 BGR uint8) or
    `caffe.Frame`s that yields, per frame, (people float64 [m, J, 3], ids int64 [m]) — the same person keeps their id from frame to
    frame, -1 marks a person no track place was free for.  kw: what `estimate_people` takes (scale / scales / base / flip / joint_mirror /
    sparse / net / the assembly arguments, `complete` and `dedupe` among them: the tracker then receives the completed people, and only those that were kept); every frame runs as `estimate_people` runs it, except that the last call is
    `Net.track_people` / `NetGroup.track_people`: the association runs on the device behind the assembly, the people it returns are
    `estimate_people`'s.  tracker: a `caffe.Tracker` of one slot or more (slot 0 is used); None makes one with the defaults, which are
    PLACEHOLDERS, not tuned on real video, and with the matching rule `assign` ("greedy" or "optimal", as `caffe.Tracker` takes it; a
    tracker of the caller's keeps its own setting) and with `smooth` (None, True or a dict, as `caffe.Tracker` takes it: the people
    yielded are then the smoothed poses of step 8 of the rule, short gaps bridged; its defaults are PLACEHOLDERS, not tuned on real
    video, and a tracker of the caller's keeps its own setting here too).  PARITY UNPINNED BY THE REFERENCE: the tracking rule is this project's own
    (include/deepcut_hip.h, dc_tracker_update).
    depth / batch: the defaults (1, 1) run one synchronous call per frame.  depth > 1 keeps that many frames in flight on the net and
    its clones, batch > 1 sends that many consecutive frames as one batch forward (`deepcut_tools.VideoPipeline`); the results are the
    same (people, ids) in frame order, up to `depth * batch` frames behind the input.  One forward per frame only: a pyramid
    (scales= / flip=True) has no asynchronous entry and raises ValueError.
    draw: None (off: nothing is added to the run), True or a dict of what `draw_people` takes — every frame is drawn into IN PLACE on the
    device, with the people and ids being yielded (the smoothed, de-duplicated ones; filled and bridged joints at alpha_filled), before
    they are yielded.  The frames must then be writable arrays or `caffe.Frame`s; (people, ids) are what they are without `draw`.
    redact: None (off: nothing is added to the run), True or a dict of what `redact_people` takes — every frame is redacted IN PLACE on the
    device with the people and ids being yielded, BEFORE the drawing (the skeletons go over the mosaic) and before they are yielded;
    (people, ids) are what they are without `redact`.  Who was not redacted (region "head": no neck or head top) is not reported here:
    call `redact_people` on the yielded people where that matters.
    in_chain: False (the default) redacts and draws with the synchronous entries on the people that came back; True sends the styles with
    the request (`deepcut_tools.VideoPipeline(in_chain=True)`, whatever depth and batch are): the frames are written inside the
    asynchronous chain on the device — the same bytes, the same (people, ids).  A redact dict with `select` raises ValueError then.
    labels: None (off: nothing is added to the run), True or a dict of what `label_people` takes — every frame gets the ids being yielded
    written over the redaction and the skeletons; with in_chain=True a dict with `texts` or `stream` raises ValueError.
    appearance: None (off: exactly the calls of today), True or a dict of some of edges, scale, min_radius, min_score (what
    `describe_people` takes; edges None = `TORSO_MPII14`) and min_pixels, alpha256, reid_max, max_age, min_hits (what `caffe.Tracker`'s
    `appearance` takes) — a person who left for longer than max_misses frames and comes back looking the same takes their old id back.
    THE DEFAULTS (`caffe.APPEARANCE_DEFAULTS`) ARE PLACEHOLDERS, NOT TUNED ON REAL VIDEO.  Per frame: the forward, `assemble_people`
    (completion and dedupe as today), `describe_people` on the frame as it came (before any overlay), then `Tracker.update(people,
    desc=...)`; with smoothing on the smoothed poses are yielded.  A tracker of the caller's has its `appearance` set from the dict's
    tracker keys.  The synchronous route only: with depth > 1, batch > 1 or in_chain=True it raises ValueError."""
    style = _draw_style(draw)
    app = _appearance_args(appearance)
    rstyle = None if redact is None or redact is False else _redact_style(redact)
    lstyle = _label_style(labels)
    args = dict(scale=1.0, net=None, scales=None, base=None, flip=False, joint_mirror=MIRROR_MPII14, sparse=False)
    for k in list(kw):
        if k in args:
            args[k] = kw.pop(k)
    in_chain = bool(in_chain) and (style is not None or rstyle is not None or lstyle is not None)
    if app is not None and (int(depth) != 1 or int(batch) != 1 or in_chain):
        raise ValueError("track_people: appearance= runs on the synchronous route only (depth=1, batch=1, not in_chain): got depth=%r, batch=%r, "
                         "in_chain=%r" % (depth, batch, in_chain))
    if int(depth) != 1 or int(batch) != 1 or in_chain:
        if args["scales"] is not None or args["flip"]:
            raise ValueError("track_people: depth > 1 / batch > 1 / in_chain run one forward per frame; a pyramid (scales= / flip=True) has no "
                             "asynchronous entry: use depth=1, batch=1")
        if in_chain:
            kw = dict(kw, in_chain=True)
        if lstyle is not None:
            kw = dict(kw, labels=lstyle)
        for item in _track_in_flight(frames, model_def, model_bin, stats, tracker, int(depth), int(batch), args, kw, assign, smooth, style, rstyle):
            yield item
        return
    for image in frames:
        if tracker is None:
            import caffe as _caffe

            tracker = _caffe.Tracker(n_joints=len(MIRROR_MPII14), assign=assign, smooth=smooth)
        if app is not None:
            d = _people_by_appearance(tracker, app, image, model_def, model_bin, stats, args, kw)
        else:
            d = _people_of_image(tracker, image, model_def, model_bin, stats, args["scale"], args["net"], args["scales"], args["base"], args["flip"],
                                 args["joint_mirror"], args["sparse"], kw)
        if rstyle is not None:
            redact_people(image, d["people"], d["ids"], **rstyle)
        if style is not None:
            draw_people(image, d["people"], d["ids"], **dict(style, cand=d["cand"]))
        if lstyle is not None:
            label_people(image, d["people"], d["ids"], **lstyle)
        yield d["people"], d["ids"]


_APPEARANCE_STYLE_KEYS = ("edges", "scale", "min_radius", "min_score")


def _appearance_args(appearance):
    """appearance= of `track_people` -> None (off) or (the style dict of `describe_people`, the dict `caffe.Tracker.appearance` takes)."""
    if appearance is None or appearance is False:
        return None
    import caffe as _caffe

    track_keys = ("min_pixels", "alpha256", "reid_max", "max_age", "min_hits")
    both = _caffe.appearance_params(appearance, _APPEARANCE_STYLE_KEYS + track_keys)  # the refusal of an unknown key
    style = {k: both[k] for k in _APPEARANCE_STYLE_KEYS if k in both}
    if style.get("edges") is None:
        style["edges"] = TORSO_MPII14
    return style, {k: both[k] for k in track_keys}


def _people_by_appearance(tracker, app, image, model_def, model_bin, stats, args, assembly):
    """One frame of `track_people(appearance=...)` -> the dict `Net.track_people` would give: the people without a tracker, their
    descriptors from the frame, then the tracker's update with them."""
    import caffe as _caffe

    style, params = app
    if tracker.appearance != params:
        tracker.appearance = params
    d = _people_of_image(None, image, model_def, model_bin, stats, args["scale"], args["net"], args["scales"], args["base"], args["flip"],
                         args["joint_mirror"], args["sparse"], assembly)
    people, cand = _np.ascontiguousarray(d["people"], dtype=_np.float64), _np.array(d["cand"], _np.int32)
    m = people.shape[0]
    ppl, desc = _np.zeros((1, max(m, 1)) + people.shape[1:], _np.float64), _np.zeros((1, max(m, 1), 3, _caffe.APPEARANCE_BINS), _np.int32)
    if m:  # a frame without people still updates the tracker: its tracks miss, the gallery ages
        ppl[0], desc[0] = people, _caffe.describe_people(image, people, **style)
    smoothed = tracker.smoothing is not None
    out = tracker.update(ppl, n_people=[m], desc=desc, return_smooth=smoothed)
    ids, place = out[0][0, :m], out[1][0, :m]
    if smoothed:
        people, src = out[2][0, :m], out[3][0, :m]
        cand[src == 2] = -3
    return dict(d, people=people, cand=cand, ids=ids, place=place)


def _track_in_flight(frames, model_def, model_bin, stats, tracker, depth, batch, args, assembly, assign="greedy", smooth=None, style=None, rstyle=None):
    """`track_people` through `deepcut_tools.VideoPipeline` -> (people, ids) per frame, in frame order."""
    import caffe as _caffe
    from deepcut_tools import VideoPipeline

    net = args["net"]
    if net is None:
        net = _get_sparse_model(model_def, model_bin) if args["sparse"] else _get_model(model_def, model_bin)
    if tracker is None:
        tracker = _caffe.Tracker(n_joints=len(MIRROR_MPII14), assign=assign, smooth=smooth)
    if style is not None:
        assembly = dict(assembly, draw=style)
    if rstyle is not None:
        assembly = dict(assembly, redact=rstyle)
    pipe = VideoPipeline(net, tracker, depth=depth, batch=batch, stats=stats, scale=args["scale"], **assembly)
    ahead = 0
    for image in frames:
        pipe.submit(image if hasattr(image, "c_frame") else _np.ascontiguousarray(image, dtype=_np.uint8))
        ahead += 1
        if ahead > depth * batch:
            _, people, ids = pipe.wait_one()
            ahead -= 1
            yield people, ids
    for _, people, ids in pipe.drain():
        yield people, ids


def _people_of_image(tracker, image, model_def, model_bin, stats, scale, net, scales, base, flip, joint_mirror, sparse, assembly):
    """The body `estimate_people` and `track_people` share -> the dict of the one image: the forward, then `assemble_people` (tracker
    None) or `track_people` of the net or of the group."""
    if scales is not None and float(scale) != 1.0:
        raise ValueError("estimate_people takes scale (one forward) or scales (a pyramid), not both: scale=%r, scales=%r" % (scale, scales))
    if sparse and (scales is not None or flip):
        raise ValueError("estimate_people: sparse=True evaluates the pairwise head of ONE forward at its candidates' cells; the fused path of "
                         "scales= / flip=True needs every member's dense next_pred")
    if flip:
        joint_mirror = _check_joint_mirror(joint_mirror)
        plain = len(scales) if scales is not None else 1
        if base is not None and not 0 <= int(base) < plain:
            raise ValueError("base %r must name one of the %d plain members: the mirrored members come after them and cannot be the base" % (base, plain))
    if isinstance(stats, (str, bytes)) or hasattr(stats, "__fspath__"):
        from deepcut_tools import read_pair_stats

        stats = read_pair_stats(stats)
    edges, mean, std = stats
    if net is None:
        net = _get_sparse_model(model_def, model_bin) if sparse else _get_model(model_def, model_bin)
    need = ("prob", "loc_pred") if getattr(net, "sparse_pairwise", False) else ("prob", "loc_pred", "next_pred")
    missing = [k for k in need if k not in net.wanted_outputs]
    if missing:
        raise ValueError("estimate_people needs all three maps, the net leaves out %r (net.set_outputs(None) brings them back)" % (missing,))
    from .estimate_pose import _is_frame

    frame = _is_frame(image)
    if not frame:
        image = _np.asarray(image)
        if image.dtype != _np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image must be uint8 [H,W,3] (BGR)")
    if scales is not None or flip:
        from .estimate_pose import _scale_group

        scales = [float(v) for v in scales] if scales is not None else [float(scale)]
        if not scales:
            raise ValueError("scales must name at least one scale")
        mirrored = {}
        if flip:
            if base is None:
                base = _base_scale(scales)
            mirrored = dict(mirror=[0] * len(scales) + [1] * len(scales), image_width=image.width if frame else image.shape[1], joint_mirror=joint_mirror)
            scales = scales + scales
        grp = _scale_group(net, len(scales))
        for m in grp.nets[1:]:  # the clones kept with the net are this module's to set: all three outputs, like the net itself
            if sorted(m.wanted_outputs) != sorted(net.wanted_outputs):
                m.set_outputs(None)
        grp.forward_images(image, scales, want=(), pose=False, mirror=mirrored.get("mirror"))
        last = grp.assemble_people if tracker is None else (lambda *a, **k: grp.track_people(tracker, *a, **k))
        return last(scales, _base_scale(scales) if base is None else int(base), edges=edges, mean=mean, std=std, **dict(assembly, **mirrored))[0]
    net.forward_images(image, scale, want=(), pose=False)
    last = net.assemble_people if tracker is None else (lambda **k: net.track_people(tracker, **k))
    return last(scale=scale, edges=edges, mean=mean, std=std, **assembly)[0]


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
