"""Video frames in flight: tracked people of a stream of frames with several requests on the GPU at a time.

`Net.track_frames_async` (dc_net_track_frames_async) enqueues the whole chain of a frame — upload, pre-processing, forward, assembly,
the tracker's update, downloads — on its net's stream and returns.  `VideoPipeline` keeps `depth` executors busy with it (the net and
`depth - 1` clones: own activations, own stream, own graph, SHARED parameters) and can send `batch` consecutive frames as ONE batch
forward whose images the tracker applies in order (the slot map of dc_tracker_update_slots).  The tracker keeps the updates of all
executors in the order of the calls (an event on the device, no host wait), and results come back in submission order.
PARITY UNPINNED BY THE REFERENCE, which stops at the maps: assembly and tracking rules are this project's own (include/deepcut_hip.h).
"""
import collections


class VideoPipeline(object):
    MAX_DEPTH = 4  # a HIP process has four hardware queues: a fifth executor only shares one

    def __init__(self, net, tracker=None, depth=3, batch=1, stats=None, scale=1.0, choose_streams=True, complete=None, dedupe=None, draw=None,
                 redact=None, in_chain=False, labels=None, **assembly):
        """net: a `caffe.Net` with all three maps (or a sparse-pairwise net); tracker: a `caffe.Tracker` or None (people without ids,
        ids come back as None); depth: executors, 1..4; batch: frames per call, 1..64; stats: (edges, mean, std) as
        `deepcut_tools.read_pair_stats` returns them, or a path; scale: the pre-processing's and the assembly's; assembly: what
        `Net.assemble_people` takes (threshold, max_det, max_cost, ...).  complete: as `Net.assemble_people` takes it — None leaves
        every executor with the net's `completion` (the clones made here copy it), True or a dict is passed with every request.  dedupe: likewise for the net's `dedupe`
        (stage E: people who are there twice are suppressed before the tracker sees them).  draw: None (off: nothing is added), True or a
        dict of what `pose.draw_people` takes — every frame is kept with its request and drawn into IN PLACE on the device with the people
        and ids being handed back (filled and bridged joints at alpha_filled), before they are handed back; the frames must then be
        writable arrays or `caffe.Frame`s.  redact: None (off: nothing is added), True or a dict of what `pose.redact_people` takes —
        every frame is kept likewise and redacted IN PLACE on the device with the people and ids being handed back, before the drawing
        (the skeletons go over the mosaic); (people, ids) are what they are without it.  in_chain: False (the default) applies draw /
        redact when a request is collected, with the synchronous `pose.redact_people` / `pose.draw_people` on the people copied to the
        host; True sends the styles WITH the request (`Net.track_frames_async(draw=, redact=)`): the frames are written inside the chain
        on the device, from the people where the tracker left them, and collecting a request calls nothing — the same bytes, the same
        (people, ids).  A redact dict with `select` is refused then (ValueError: a mask cannot exist before the people do; use
        only_ids / keep_ids, which need a tracker), as is `stream` in either dict.  labels: None (off: nothing is added), True or a
        dict of what `pose.label_people` takes — every frame gets the ids (without a tracker the people's indices) written over the
        redaction and the skeletons, on either route with the same bytes; with in_chain=True `texts` and `stream` in it are refused
        (ValueError: a text for a person cannot exist before the person does)."""
        depth, batch = int(depth), int(batch)
        if not 1 <= depth <= self.MAX_DEPTH:
            raise ValueError("depth must be in [1, %d], got %d" % (self.MAX_DEPTH, depth))
        if not 1 <= batch <= 64:
            raise ValueError("batch must be in [1, 64], got %d" % batch)
        if stats is None:
            raise ValueError("VideoPipeline needs the pair statistics (stats=(edges, mean, std) or a path)")
        if isinstance(stats, (str, bytes)) or hasattr(stats, "__fspath__"):
            from .pair_stats import read_pair_stats

            stats = read_pair_stats(stats)
        self.edges, self.mean, self.std = stats
        self.nets = [net] + [net.clone() for _ in range(depth - 1)]
        self.tracker, self.batch, self.scale, self.assembly = tracker, batch, float(scale), dict(assembly)
        if complete is not None:
            self.assembly["complete"] = complete
        if dedupe is not None:
            self.assembly["dedupe"] = dedupe
        self._draw = None  # the style dict when frames are drawn into
        if draw is not None and draw is not False:
            from pose.people import _draw_style

            self._draw = _draw_style(draw)
        self._redact = None  # the style dict when frames are redacted
        if redact is not None and redact is not False:
            from pose.people import _redact_style

            self._redact = _redact_style(redact)
        self._labels = None  # the style dict when frames are labelled
        if labels is not None and labels is not False:
            from pose.people import _label_style

            self._labels = _label_style(labels)
        self._in_chain = bool(in_chain) and (self._draw is not None or self._redact is not None or self._labels is not None)
        if self._in_chain:
            from pose.people import HEAD_MPII14, SKELETON_MPII14

            for style in (self._draw, self._redact, self._labels):
                if style is not None and "stream" in style:
                    raise ValueError("in_chain=True runs on the executor's own stream: the style must not name one")
            if self._labels is not None and self._labels.get("texts") is not None:
                raise ValueError("in_chain=True: texts are per person, and the people do not exist before the request")
            if self._draw is not None:
                self._draw.setdefault("edges", SKELETON_MPII14)  # what pose.draw_people / pose.redact_people fill in on the host route
            if self._redact is not None:
                if self._redact.get("select") is not None:
                    raise ValueError("in_chain=True: select is a mask over people, who do not exist before the request: choose them by "
                                     "only_ids / keep_ids")
                if (self._redact.get("only_ids") is not None or self._redact.get("keep_ids") is not None) and tracker is None:
                    raise ValueError("only_ids / keep_ids choose people by id: ids is needed")
                self._redact.setdefault("head", HEAD_MPII14)
                self._redact.setdefault("edges", SKELETON_MPII14)
        self._choose_streams = bool(choose_streams)
        self.stream_choice = None            # what caffe.choose_streams measured, once it ran
        self._held = []                      # frames of the batch being gathered: (frame, tag, slot, shape key)
        self._pending = collections.deque()  # requests in flight, in submission order: (executor, handle, tags)
        self._done = collections.deque()     # results not yet handed back, in submission order
        self._next = 0
        self.calls = 0

    @property
    def depth(self):
        return len(self.nets)

    # ---- launching ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _shape_key(frame):
        if hasattr(frame, "is_device") and hasattr(frame, "c_frame"):  # a caffe.Frame
            return ("frame", frame.format, frame.height, frame.width, frame.is_device, frame.matrix, frame.range)
        shape = tuple(getattr(frame, "shape", ()))
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError("submit takes a caffe.Frame or an HxWx3 uint8 image")
        return ("bgr",) + shape

    def _free_executor(self):
        # an executor is busy while a request of it has not been SEEN finished (done() remembers: the net may get the next one at once)
        busy = set(k for k, handle, _, _ in self._pending if not handle.done())
        for i in range(len(self.nets)):
            k = (self._next + i) % len(self.nets)
            if k not in busy:
                return k
        return None

    def _collect_oldest(self):
        """Wait for the oldest request (the tracker ran them in submission order, so it finishes first or nearly) and queue its results."""
        k, handle, tags, frames = self._pending.popleft()
        results = handle.result()
        if self._in_chain and frames is not None and isinstance(frames, tuple):  # images sent as one stacked batch: back into the caller's
            for image, written in zip(*frames):
                image[...] = written
        host_route = frames is not None and not self._in_chain  # in_chain: the chain has written the frames
        for i, (tag, d) in enumerate(zip(tags, results)):
            if host_route and self._redact is not None:
                from pose.people import redact_people

                redact_people(frames[i], d["people"], d.get("ids"), **self._redact)
            if host_route and self._draw is not None:
                from pose.people import draw_people

                draw_people(frames[i], d["people"], d.get("ids"), **dict(self._draw, cand=d.get("cand")))
            if host_route and self._labels is not None:
                from pose.people import label_people

                label_people(frames[i], d["people"], d.get("ids"), **self._labels)
            self._done.append((tag, d["people"], d.get("ids")))

    def _send(self):
        held, self._held = self._held, []
        if not held:
            return
        k = self._free_executor()
        while k is None:  # every executor is busy: the only place a submit blocks
            self._collect_oldest()
            k = self._free_executor()
        self._next = (k + 1) % len(self.nets)
        frames = [h[0] for h in held]
        kept = frames if self._draw is not None or self._redact is not None or self._labels is not None else None  # the frames themselves, to be redacted / drawn into when their results are there
        if held[0][3][0] == "bgr":
            import numpy as np

            if self._in_chain and len(frames) > 1:  # the chain writes into the stacked copy
                stacked = np.stack(frames)
                kept, frames = (frames, stacked), stacked
            else:
                frames = np.stack(frames) if len(frames) > 1 else frames[0]
        if self._choose_streams and len(self.nets) > 1 and not self._pending and self.calls == 0:
            # first call: every executor lowers / allocates / tunes the shape, then the library picks their streams by timing them
            # together — untimed set-up, as in Pipeline
            import caffe

            self._choose_streams = False
            key = held[0][3]
            ch, cw = caffe.canvas_size(*(key[2:4] if key[0] == "frame" else key[1:3]), self.scale)
            for e in self.nets:
                e.reserve(len(held), ch, cw)
            self.stream_choice = caffe.choose_streams(self.nets)
        slot_of = None if self.tracker is None else [h[2] for h in held]
        styles = dict(draw=self._draw, redact=self._redact) if self._in_chain else {}
        if self._in_chain and self._labels is not None:
            styles["labels"] = self._labels
        handle = self.nets[k].track_frames_async(frames, self.tracker, self.scale, slot_of=slot_of, edges=self.edges, mean=self.mean,
                                                 std=self.std, **dict(self.assembly, **styles))
        self.calls += 1
        self._pending.append((k, handle, [h[1] for h in held], kept))

    def submit(self, frame, tag=None, slot=0):
        """Enqueue one frame (a `caffe.Frame` or an HxWx3 uint8 BGR image) of the sequence in tracker slot `slot`.  With batch > 1 the
        frame is held until `batch` frames of one shape are there (or flush() / drain()); a frame of another shape sends what is held
        first.  The frame must stay untouched until its result comes back.  Blocks only when every executor is busy."""
        key = self._shape_key(frame)
        if self._held and self._held[0][3] != key:
            self._send()
        self._held.append((frame, tag, int(slot), key))
        if len(self._held) >= self.batch:
            self._send()

    def flush(self):
        """Send the frames held for a batch as they are (a partial batch)."""
        self._send()

    def wait_one(self):
        """-> (tag, people float64 [m, J, 3], ids int64 [m] or None) of the oldest frame not yet handed back: results come in
        submission order."""
        if not (self._done or self._pending or self._held):
            raise RuntimeError("wait_one() with nothing submitted")
        if not self._done:
            if not self._pending:
                self._send()
            self._collect_oldest()
        return self._done.popleft()

    def drain(self):
        """Send what is held, wait for everything -> the list of (tag, people, ids) in submission order."""
        self._send()
        while self._pending:
            self._collect_oldest()
        out = list(self._done)
        self._done.clear()
        return out
