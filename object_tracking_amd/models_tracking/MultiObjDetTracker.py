"""MultiObjDetTracker -- the reference's simultaneous detect-and-track model
(models_tracking/MultiObjDetTracker.py) with the same public surface, running
on the MI355X through libmi355_dt.so.

Kept from the reference (file:line into the reference):
  class attributes / defaults             MultiObjDetTracker.py:70-120
  __init__(argv={})                       :122-133  (builds KerasYOLO with the 6-key argv)
  load_model()                            :160-189  TimeDistributed(YOLO) -> concat([x_bbox, x_vis])
                                                    -> ConvLSTM2D(512,(3,3)) -> 1x1 conv -> reshape
  load_weights()                          :291-293
  predict(input_paths, output_paths)      :295-315  (broken as written; the
                                                    INTENDED behaviour is implemented)
  train()                                 :221-288  (out of scope: raises)

Track identity is an ADDITION with no reference semantics (`trackid` is written
by the dataset converters and never read): ids come from
the deterministic greedy IoU association specified in DESIGN.md "Track identity".
"""
import os

import numpy as np

import mi355_dt
from models_detection.KerasYOLO import KerasYOLO
from utility.frames import imwrite_bgr, load_frame
from utility.utils import BoundBox, draw_boxes

mot17_class_map = {
    '1': 'Pedestrian', '2': 'Person on vehicle', '3': 'Car', '4': 'Bicycle', '5': 'Motorbike',
    '6': 'Non motorized vehicle', '7': 'Static person', '8': 'Distractor', '9': 'Occluder',
    '10': 'Occluder on the ground', '11': 'Occluder full', '12': 'Reflection'}


class NativeTrackerModel(object):
    """Replaces the Keras `Model([images, true_boxes], [tracking, detection])`
    (MultiObjDetTracker.py:185-188)."""

    def __init__(self, owner):
        self.owner = owner
        self.ctx = owner.detector.model.ctx      # one dt_ctx holds detector + recurrent head
        self.loaded = False

    def set_weights(self, w):
        """w: dict(kernel [3,3,Cb+1024,4U], recurrent [3,3,U,4U], bias [4U],
        out_kernel [1,1,U,Cb], out_bias [Cb]) in Keras layouts
        ('tconv_lstm' and 'timedist_tconv2', MultiObjDetTracker.py:176,182)."""
        units = int(w["recurrent"].shape[2])
        self.ctx.tracker_load(units, w["kernel"], w["recurrent"], w["bias"], w["out_kernel"], w["out_bias"])
        self.loaded = True

    def load_weights(self, path):
        """Keras-style load_weights (MultiObjDetTracker.py:291-293).  Accepts
          * a Keras HDF5 checkpoint (.hdf5 / .h5: whole-model file as ModelCheckpoint writes it, :253-259, or a
            weights-only file): layers 'tconv_lstm' and 'timedist_tconv2' (:176,182); if the file also carries the
            detector (the TimeDistributed copies 'timedist_bbox'), its conv_N / norm_N weights replace the
            detector's.  Read with utility/keras_h5.py (pure Python; h5py is used when importable);
          * an .npz with arrays kernel / recurrent / bias / out_kernel / out_bias (+ optional `darknet` stream)."""
        if path.endswith(".npz"):
            d = np.load(path)
            if "darknet" in d:
                self.owner.detector.model.set_darknet_blob(d["darknet"])
            self.set_weights({k: d[k] for k in ("kernel", "recurrent", "bias", "out_kernel", "out_bias")})
            return
        from utility import keras_h5
        layers = keras_h5.read_keras_weights(path)
        blob = keras_h5.darknet_blob_from_keras(layers)
        if blob is not None:
            self.owner.detector.model.set_darknet_blob(blob)
        self.set_weights(keras_h5.tracker_weights_from_keras(layers))

    def forward(self, frames, want_det=True):
        return self.ctx.track_forward(self.owner.detector.model.to_device(frames), want_det=want_det)

    def forward_stream(self, frames, slots, want_det=False):
        return self.ctx.track_stream_forward(self.owner.detector.model.to_device(frames), slots, want_det=want_det)

    def predict(self, inputs, batch_size=None):
        """Keras-style: [x (B,T,H,W,3), b] -> [tracking, detection] numpy grids
        (B,T,G,G,BOX,5+CLASS)  (MultiObjDetTracker.py:307)."""
        x = inputs[0] if isinstance(inputs, (list, tuple)) else inputs
        trk, det = self.forward(x, want_det=True)
        return [trk.cpu().numpy(), det.cpu().numpy()]

    def summary(self):
        o = self.owner
        print("NativeTrackerModel: TimeDistributed(YOLOv2) -> ConvLSTM2D(512,3x3) -> Conv2D(%d,1x1); T=%d on %s" % (
            o.BOX * (5 + o.CLASS), o.SEQUENCE_LENGTH, self.ctx.device))


class MultiObjDetTracker(object):
    LABELS_IMAGENET_VIDEO = [
        'n02691156', 'n02419796', 'n02131653', 'n02834778', 'n01503061', 'n02924116', 'n02958343', 'n02402425',
        'n02084071', 'n02121808', 'n02503517', 'n02118333', 'n02510455', 'n02342885', 'n02374451', 'n02129165',
        'n01674464', 'n02484322', 'n03790512', 'n02324045', 'n02509815', 'n02411705', 'n01726692', 'n02355227',
        'n02129604', 'n04468005', 'n01662784', 'n04530566', 'n02062744', 'n02391049']

    LABELS_MOT17 = ['1', '2', '3', '4', '5', '6', '7', '8', '9', '10', '11', '12']

    LABELS = LABELS_MOT17
    IMAGE_H, IMAGE_W = 416, 416
    GRID_H, GRID_W = 13, 13
    BOX = 5
    CLASS = len(LABELS)
    CLASS_WEIGHTS = np.ones(CLASS, dtype='float32')
    OBJ_THRESHOLD = 0.5
    NMS_THRESHOLD = 0.45
    ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]

    NO_OBJECT_SCALE = 1.0
    OBJECT_SCALE = 5.0
    COORD_SCALE = 1.0
    CLASS_SCALE = 1.0

    BATCH_SIZE = 1
    WARM_UP_BATCHES = 0
    TRUE_BOX_BUFFER = 50

    SEQUENCE_LENGTH = 4
    MAX_BOX_PER_IMAGE = 50

    LOAD_MODEL = True
    INITIAL_EPOCH = 0
    SAVED_MODEL_PATH = 'models/MultiObjDetTracker-CHKPNT-03-0.55.hdf5'

    # build-defined (no reference counterpart): IoU a frame-t box needs with a
    # frame-(t-1) box of the same label to inherit its track id
    ASSOC_THRESHOLD = 0.3
    # build-defined track memory: frames a track may go without a box and still keep its id (0: a box can
    # inherit an id from the previous frame only), and the entries of the table of tracks (None: the box capacity `cap`;
    # a table of at most 64 entries, which needs cap <= 64 too, runs in registers)
    MAX_AGE = 0
    TRACK_CAP = None
    # build-defined track motion: None = none; a number in [0, 1] = a track is matched where its velocity predicts
    # it, the velocity following the observed one with this gain (whatever MAX_AGE is; the result then always carries `gaps`)
    MOTION_GAIN = None
    # build-defined track read-out: None = none; an int >= 1 = the result also carries `hits` and, per frame, the
    # tracks that have had a box in at least MIN_HITS frames -- the lost ones (up to MAX_AGE frames) at their predicted place.  The
    # match is the track-motion rule with MOTION_GAIN (None: gain 0, the track-memory rule)
    MIN_HITS = None
    # build-defined track match policy: how a frame's boxes are matched to the table of tracks.  Both False: boxes
    # in decode order, each against the tracks of its own label.  MATCH_BEST_FIRST: the (box, track) pairs are taken best IoU first, so
    # the result does not depend on the order of the frame's boxes.  MATCH_ANY_LABEL: labels are not compared, so a track survives a
    # flipped label.  With either set the result carries `gaps` and `hits` (the match runs in the track read-out's kernel; the read-out
    # itself still appears only with MIN_HITS)
    MATCH_BEST_FIRST = False
    MATCH_ANY_LABEL = False
    # build-defined track assignment: the match of a frame is the optimal one-to-one assignment (the largest summed
    # IoU, the Hungarian step of the SORT family) instead of a greedy pass; MATCH_ANY_LABEL still applies, MATCH_BEST_FIRST beside it is
    # refused by the library.  The result carries `gaps` and `hits` as with a MATCH_* policy
    MATCH_OPTIMAL = False
    # build-defined track scores: None = off.  A number = the two-pass match of BYTE on the decoded boxes' scores
    # (mi355_dt.Context.associate_tracks_scored; the optimal assignment is implied, MATCH_BEST_FIRST is refused): boxes with float SCORE_AT
    # (6: the class score, 4: the objectness) >= SCORE_HIGH are matched first, the weaker ones only continue a track still unmatched and no
    # older than MAX_AGE_LOW frames (at ASSOC_THRESHOLD_LOW; None: ASSOC_THRESHOLD), and a box that matches nothing opens a track only
    # with a score >= SCORE_NEW (None: SCORE_HIGH) -- otherwise it is dropped: ids -1, hits 0.  Meant to go with a low OBJ_THRESHOLD.
    # MATCH_ANY_LABEL, MIN_HITS, MOTION_GAIN, TRACK_CAP and INGEST_FIT apply as they do without it; the result carries `gaps` and `hits`
    SCORE_HIGH = None
    SCORE_NEW = None
    ASSOC_THRESHOLD_LOW = None
    MAX_AGE_LOW = 0
    SCORE_AT = 6
    # build-defined frame ingest: track_stream on lists of device frames exchanges channels 0 and 2 while ingesting
    INGEST_SWAP_RB = False
    # build-defined frame views: None = lists of frames are stretched (dt_ingest_frames).  "letterbox" / "stretch" = they
    # go through dt_ingest_views (items may be utility.frames.FrameView; a plain frame is fitted whole by this rule) and the decoded boxes
    # are mapped to the source frames' normalised coordinates BEFORE association: ids, the track table, velocities and the read-out rows
    # live in source space, and the result carries `affine` [n, T, 4]
    INGEST_FIT = None

    train_image_folder = 'data/MOT17/MOT17Det/train/'
    train_annot_folder = 'data/MOT17Ann/train/'
    valid_image_folder = 'data/MOT17/MOT17Det/train/'
    valid_annot_folder = 'data/MOT17Ann/val/'

    model = None
    detector = None
    model_detector = None

    def __init__(self, argv={}, detector_weights=None, tracker_weights=None):
        """`argv` as in the reference (its 6 keys are overwritten from the class
        attributes, MultiObjDetTracker.py:123-128).  `detector_weights` /
        `tracker_weights` (additions) supply a darknet stream and a Keras-layout
        weight dict instead of files."""
        argv = dict(argv)
        argv['LABELS'] = self.LABELS
        argv['BATCH_SIZE'] = self.BATCH_SIZE * self.SEQUENCE_LENGTH
        argv['IMAGE_H'] = self.IMAGE_H
        argv['IMAGE_W'] = self.IMAGE_W
        argv['GRID_H'] = self.GRID_H
        argv['GRID_W'] = self.GRID_W
        self.CLASS = len(self.LABELS)

        self.detector = KerasYOLO(argv, weights=detector_weights)
        self._tracker_weights = tracker_weights
        self.load_model()
        if tracker_weights is not None:
            self.model.set_weights(tracker_weights)
        elif self.LOAD_MODEL:
            self.load_weights()

    def load_model(self):
        # the reference's two-output detector sub-model (:162-164) is the same
        # native detector, tapped at conv_23 and conv_feat inside dt_track_forward
        self.model_detector = self.detector.model
        self.model_detector.get_layer('conv_23')
        self.model_detector.get_layer('conv_feat')
        self.model = NativeTrackerModel(self)
        self.model.summary()

    def load_weights(self):
        path = self.SAVED_MODEL_PATH
        if not os.path.isfile(path):
            alt = os.path.splitext(path)[0] + ".npz"
            if os.path.isfile(alt):
                path = alt
            else:
                raise IOError("checkpoint %r not found (the reference loads it in __init__ when LOAD_MODEL, "
                              "MultiObjDetTracker.py:131-133)" % self.SAVED_MODEL_PATH)
        self.model.load_weights(path)
        try:
            self.INITIAL_EPOCH = int(self.SAVED_MODEL_PATH.split('-')[2])
        except (IndexError, ValueError):
            pass

    def _match_policy(self):
        return (mi355_dt.DT_MATCH_BEST_FIRST if self.MATCH_BEST_FIRST else 0) | (mi355_dt.DT_MATCH_ANY_LABEL if self.MATCH_ANY_LABEL else 0)

    def _score_args(self):
        """the keyword arguments of the scored association entries (SCORE_HIGH set)"""
        return dict(score_high=self.SCORE_HIGH, score_new=self.SCORE_NEW, assoc_threshold_low=self.ASSOC_THRESHOLD_LOW,
                    max_age_low=self.MAX_AGE_LOW, score_at=self.SCORE_AT, match=self._match_policy(), readout=self.MIN_HITS is not None)

    def train(self):
        raise NotImplementedError("training (custom_loss_*, fit_generator) is outside the MI355X hot path this "
                                  "build covers (SURVEY.md C7/C8); only inference entry points are implemented")

    # ------------------------------------------------------------------
    def track_clips(self, frames, cap=None):
        """Batched device path (addition).  frames [n_clips,T,H,W,3] uint8/float32
        (numpy or device tensor).  Returns device tensors:
          boxes  [n_clips,T,cap,8]  x,y,w,h,conf,label,score,cell (decode order)
          counts [n_clips,T]        boxes per frame
          ids    [n_clips,T,cap]    track ids (-1 in unused slots), per clip from 0
          nids   [n_clips]          ids opened per clip
          gaps   [n_clips,T,cap]    only with MAX_AGE > 0, a MOTION_GAIN, MIN_HITS or a MATCH_* policy (MATCH_OPTIMAL and SCORE_HIGH included): frames the box's track had missed (0 unbroken, -1 new id / unused)
        and only with MIN_HITS (the track read-out, mi355_dt.Context.associate_tracks):
          hits   [n_clips,T,cap]    frames in which the box's track has had a box (also with a MATCH_* policy alone)
          tracks [n_clips,T,tcap,8], track_info [n_clips,T,tcap,4], track_counts [n_clips,T]   the confirmed tracks of every frame
        One dt_track_forward (YOLOv2 x T, ConvLSTM recurrence, 1x1), one dt_decode
        over all frames, one dt_associate."""
        return self.decode_and_associate(self.model.forward(frames, want_det=False), cap=cap)

    # ---- streaming (addition): ConvLSTM state and track ids carried across calls ----
    def open_streams(self, n_slots, cap=None, track_cap=None):
        """Allocate n_slots stream slots on the device (every one fresh).  cap: box capacity per frame, as in track_clips;
        track_cap: entries of a slot's track table (None: TRACK_CAP, and with that None too: cap)."""
        if cap is None:
            cap = self.GRID_H * self.GRID_W * self.BOX
        if track_cap is None:
            track_cap = self.TRACK_CAP
        self.model.ctx.stream_open(n_slots, cap, track_cap=track_cap)
        self._stream_cap = cap

    def reset_streams(self, slots=None):
        """The listed slots (None: all) start over: zero recurrent state, track ids from 0."""
        self.model.ctx.stream_reset(slots)

    def track_stream(self, frames, slots, cap=None):
        """track_clips for live streams.  frames [n,T,H,W,3]: the next T frames of n streams, stream i living in slot slots[i]
        (distinct numbers below open_streams' n_slots; see models_tracking/streams.py:StreamTable for a key -> slot map).
        Returns the track_clips dict; a stream fed in chunks of any sizes gives what track_clips gives on the concatenation:
        `ids` continue across calls and `nids` counts the ids a stream has opened since its reset.
        frames may also be a LIST of n streams, each a list of its next T device frames as decoders and crops hand them out -- uint8
        [H,W,3] tensors (row-pitched views allowed) and NV12 pairs (y, uv), every frame at its own size, equal T
        (mi355_dt.Context.ingest_frames): one ingest call converts and resizes them to IMAGE_H x IMAGE_W on the device."""
        ctx, affine = self.model.ctx, None
        if isinstance(frames, (list, tuple)):
            frames, affine = self._ingest_streams(frames)
        if cap is None:
            cap = getattr(self, "_stream_cap", None) or self.GRID_H * self.GRID_W * self.BOX
        trk = self.model.forward_stream(frames, slots, want_det=False)
        n, T = trk.shape[:2]
        flat = trk.reshape((n * T,) + tuple(trk.shape[2:]))
        r = ctx.decode(flat, self.OBJ_THRESHOLD, self.NMS_THRESHOLD, self.ANCHORS, len(self.LABELS), cap=cap)
        boxes = r["boxes"].reshape(n, T, cap, mi355_dt.DT_BOX_FLOATS)
        counts = r["counts"].reshape(n, T)
        if affine is not None:
            # to source coordinates before anything is matched; without views nothing is mapped (an identity map is not free of effect:
            # -0.0 * 1 + 0 is +0.0)
            ctx.boxes_map(boxes, counts, affine)
            return dict(self._associate_stream(boxes, counts, slots), netout=trk, affine=affine.reshape(n, T, 4))
        return dict(self._associate_stream(boxes, counts, slots), netout=trk)

    def _associate_stream(self, boxes, counts, slots):
        """the association entry the class attributes select, on a call's boxes: the result dict without `netout`"""
        ctx = self.model.ctx
        match = self._match_policy()
        if self.SCORE_HIGH is not None:
            a = ctx.associate_stream_tracks_scored(boxes, counts, self.ASSOC_THRESHOLD, slots, self.MAX_AGE,
                                                   0.0 if self.MOTION_GAIN is None else self.MOTION_GAIN, self.MIN_HITS or 1, **self._score_args())
            return dict(a, boxes=boxes, counts=counts)
        if self.MIN_HITS is not None or match or self.MATCH_OPTIMAL:
            a = ctx.associate_stream_tracks(boxes, counts, self.ASSOC_THRESHOLD, slots, self.MAX_AGE,
                                            0.0 if self.MOTION_GAIN is None else self.MOTION_GAIN, self.MIN_HITS or 1, match=match,
                                            readout=self.MIN_HITS is not None, assign=bool(self.MATCH_OPTIMAL))
            return dict(a, boxes=boxes, counts=counts)
        if self.MOTION_GAIN is not None:
            ids, nids, gaps = ctx.associate_stream(boxes, counts, self.ASSOC_THRESHOLD, slots, max_age=self.MAX_AGE, want_gaps=True,
                                                   motion_gain=self.MOTION_GAIN)
            return dict(boxes=boxes, counts=counts, ids=ids, nids=nids, gaps=gaps)
        if self.MAX_AGE > 0:
            ids, nids, gaps = ctx.associate_stream(boxes, counts, self.ASSOC_THRESHOLD, slots, max_age=self.MAX_AGE, want_gaps=True)
            return dict(boxes=boxes, counts=counts, ids=ids, nids=nids, gaps=gaps)
        ids, nids = ctx.associate_stream(boxes, counts, self.ASSOC_THRESHOLD, slots)
        return dict(boxes=boxes, counts=counts, ids=ids, nids=nids)

    def _ingest_streams(self, streams):
        """a list (streams) of lists (T frames each) -> (uint8 [n, T, IMAGE_H, IMAGE_W, 3] on the device, affine): one dt_ingest_frames call
        and None, or with INGEST_FIT one dt_ingest_views call and the box map [n * T, 4] of its views"""
        n = len(streams)
        if n == 0 or any(not isinstance(s, (list, tuple)) for s in streams):
            raise mi355_dt.NativeError("track_stream: frames must be a tensor or a list (streams) of lists (the frames of each)")
        T = len(streams[0])
        for i, s in enumerate(streams):
            if len(s) != T or T == 0:
                raise mi355_dt.NativeError("track_stream: stream %d has %d frames, stream 0 has %d (equal, and at least one)" % (i, len(s), T))
        flat = [f for s in streams for f in s]
        if self.INGEST_FIT is None:
            out, affine = self.model.ctx.ingest_frames(flat, self.IMAGE_H, self.IMAGE_W, swap_rb=self.INGEST_SWAP_RB), None
        else:
            out, affine = self.model.ctx.ingest_views(flat, self.IMAGE_H, self.IMAGE_W, swap_rb=self.INGEST_SWAP_RB, fit=self.INGEST_FIT)
        return out.reshape(n, T, self.IMAGE_H, self.IMAGE_W, 3), affine

    def decode_and_associate(self, trk, cap=None):
        """tracking grid [n_clips,T,G,G,BOX,5+C] (device) -> the track_clips result dict: one dt_decode over all frames
        (OBJ_THRESHOLD / NMS_THRESHOLD may be arrays of one value per frame, clip-major), one dt_associate."""
        ctx = self.model.ctx
        n_clips, T = trk.shape[:2]
        flat = trk.reshape((n_clips * T,) + tuple(trk.shape[2:]))
        if cap is None:
            cap = self.GRID_H * self.GRID_W * self.BOX
        r = ctx.decode(flat, self.OBJ_THRESHOLD, self.NMS_THRESHOLD, self.ANCHORS, len(self.LABELS), cap=cap)
        boxes = r["boxes"].reshape(n_clips, T, cap, mi355_dt.DT_BOX_FLOATS)
        counts = r["counts"].reshape(n_clips, T)
        match = self._match_policy()
        if self.SCORE_HIGH is not None:
            a = ctx.associate_tracks_scored(boxes, counts, self.ASSOC_THRESHOLD, self.MAX_AGE, 0.0 if self.MOTION_GAIN is None else self.MOTION_GAIN,
                                            self.MIN_HITS or 1, track_cap=self.TRACK_CAP, **self._score_args())
            return dict(a, boxes=boxes, counts=counts, netout=trk)
        if self.MIN_HITS is not None or match or self.MATCH_OPTIMAL:
            a = ctx.associate_tracks(boxes, counts, self.ASSOC_THRESHOLD, self.MAX_AGE, 0.0 if self.MOTION_GAIN is None else self.MOTION_GAIN,
                                     self.MIN_HITS or 1, track_cap=self.TRACK_CAP, match=match, readout=self.MIN_HITS is not None,
                                     assign=bool(self.MATCH_OPTIMAL))
            return dict(a, boxes=boxes, counts=counts, netout=trk)
        if self.MOTION_GAIN is not None:
            ids, nids, gaps = ctx.associate(boxes, counts, self.ASSOC_THRESHOLD, max_age=self.MAX_AGE, track_cap=self.TRACK_CAP,
                                            want_gaps=True, motion_gain=self.MOTION_GAIN)
            return dict(boxes=boxes, counts=counts, ids=ids, nids=nids, gaps=gaps, netout=trk)
        if self.MAX_AGE > 0:
            ids, nids, gaps = ctx.associate(boxes, counts, self.ASSOC_THRESHOLD, max_age=self.MAX_AGE, track_cap=self.TRACK_CAP,
                                            want_gaps=True)
            return dict(boxes=boxes, counts=counts, ids=ids, nids=nids, gaps=gaps, netout=trk)
        ids, nids = ctx.associate(boxes, counts, self.ASSOC_THRESHOLD)
        return dict(boxes=boxes, counts=counts, ids=ids, nids=nids, netout=trk)

    def empty_result(self, T, cap=None):
        """result dict for zero clips (a rank that owns no clip in a frame-sharded run)"""
        import torch
        ctx = self.model.ctx
        if cap is None:
            cap = self.GRID_H * self.GRID_W * self.BOX
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=ctx.device)
        res = dict(boxes=z((0, T, cap, mi355_dt.DT_BOX_FLOATS), torch.float32), counts=z((0, T), torch.int32),
                   ids=z((0, T, cap), torch.int32), nids=z((0,), torch.int32), netout=None)
        if self.MIN_HITS is None and (self._match_policy() or self.MATCH_OPTIMAL or self.SCORE_HIGH is not None):
            res.update(gaps=z((0, T, cap), torch.int32), hits=z((0, T, cap), torch.int32))
        if self.MIN_HITS is not None:
            tcap = cap if self.TRACK_CAP is None else self.TRACK_CAP
            res.update(gaps=z((0, T, cap), torch.int32), hits=z((0, T, cap), torch.int32),
                       tracks=z((0, T, tcap, mi355_dt.DT_TRACK_FLOATS), torch.float32),
                       track_info=z((0, T, tcap, mi355_dt.DT_TRACK_INTS), torch.int32), track_counts=z((0, T), torch.int32))
        return res

    def score(self, result, gt, confirmed=False, iou_threshold=0.5, any_label=False, obj_cap=None, state=None, per_box=True):
        """Score a track_clips / track_stream result against ground-truth tracks on the device (mi355_dt.Context.track_score; the
        rule: DESIGN.md "Track scoring").  gt = (gt_boxes [n,T,gcap,8], gt_counts [n,T], gt_ids [n,T,gcap]), numpy or device tensors
        (utility.evaluate.gt_from_mot builds one sequence of them from MOT gt.txt).  The hypotheses are the result's boxes / counts /
        ids, or with confirmed=True its read-out tracks / track_counts / track_info (MIN_HITS set; coasting tracks included).
        state: the previous chunk's score, for results of track_stream.  utility.evaluate.summarize gives MOTA etc. of the return."""
        import torch
        ctx = self.model.ctx
        dev = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=ctx.device, dtype=dt).contiguous()
        gb, gc, gi = dev(gt[0], torch.float32), dev(gt[1], torch.int32), dev(gt[2], torch.int32)
        if confirmed:
            if result.get("tracks") is None:
                raise mi355_dt.NativeError("score(confirmed=True) needs the track read-out in the result (MIN_HITS)")
            hyp = (result["tracks"], result["track_counts"], result["track_info"])
        else:
            hyp = (result["boxes"], result["counts"], result["ids"])
        return ctx.track_score(gb, gc, gi, hyp[0], hyp[1], hyp[2], iou_threshold=iou_threshold, any_label=any_label, obj_cap=obj_cap,
                               state=state, per_box=per_box)

    def identity(self, result, gt, confirmed=False, iou_threshold=0.5, any_label=False, state=None):
        """Identity scoring of a track_clips / track_stream result against ground-truth tracks on the device
        (mi355_dt.Context.identity_score; the rule: DESIGN.md "Identity scoring"): gt and the choice of hypotheses are score()'s.
        state: the previous chunk's result, for results of track_stream.  utility.evaluate.identity gives IDF1 etc. of the return."""
        import torch
        ctx = self.model.ctx
        dev = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=ctx.device, dtype=dt).contiguous()
        gb, gc, gi = dev(gt[0], torch.float32), dev(gt[1], torch.int32), dev(gt[2], torch.int32)
        if confirmed:
            if result.get("tracks") is None:
                raise mi355_dt.NativeError("identity(confirmed=True) needs the track read-out in the result (MIN_HITS)")
            hyp = (result["tracks"], result["track_counts"], result["track_info"])
        else:
            hyp = (result["boxes"], result["counts"], result["ids"])
        return ctx.identity_score(gb, gc, gi, hyp[0], hyp[1], hyp[2], iou_threshold=iou_threshold, any_label=any_label, state=state)

    def hota(self, result, gt, confirmed=False, any_label=False, thresholds=None, align=None, state=None):
        """HOTA scoring of a track_clips / track_stream result against ground-truth tracks on the device
        (mi355_dt.Context.hota_score; the rule: DESIGN.md "HOTA scoring"): gt and the choice of hypotheses are score()'s; thresholds:
        None = utility.evaluate.HOTA_THRESHOLDS.  align / state: for results of track_stream -- a finished Context.hota_align result of
        the whole run, and the previous chunk's return.  utility.evaluate.hota gives HOTA, DetA, AssA, LocA etc. of the return."""
        import torch
        ctx = self.model.ctx
        dev = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=ctx.device, dtype=dt).contiguous()
        gb, gc, gi = dev(gt[0], torch.float32), dev(gt[1], torch.int32), dev(gt[2], torch.int32)
        if confirmed:
            if result.get("tracks") is None:
                raise mi355_dt.NativeError("hota(confirmed=True) needs the track read-out in the result (MIN_HITS)")
            hyp = (result["tracks"], result["track_counts"], result["track_info"])
        else:
            hyp = (result["boxes"], result["counts"], result["ids"])
        return ctx.hota_score(gb, gc, gi, hyp[0], hyp[1], hyp[2], thresholds=thresholds, any_label=any_label, align=align, state=state)

    @staticmethod
    def boxes_from_result(res, clip=0):
        """Host view of track_clips output for one clip: list over t of BoundBox lists."""
        boxes = res["boxes"][clip].cpu().numpy()
        counts = res["counts"][clip].cpu().numpy()
        ids = res["ids"][clip].cpu().numpy()
        gaps = res["gaps"][clip].cpu().numpy() if res.get("gaps") is not None else None
        hits = res["hits"][clip].cpu().numpy() if res.get("hits") is not None else None
        out = []
        for t in range(boxes.shape[0]):
            n = min(int(counts[t]), boxes.shape[1])
            lst = []
            for i in range(n):
                x, y, w, h, c, lab, sc, _ = boxes[t, i]
                bb = BoundBox(x, y, w, h, c, None)
                bb.label = int(lab)
                bb.score = sc
                bb.track_id = int(ids[t, i])
                # frames the track had gone without a box (0: unbroken, -1: a new id); None when the result carries no gaps (MAX_AGE = 0)
                bb.track_gap = int(gaps[t, i]) if gaps is not None else None
                # frames in which the track has had a box, this one included; None when the result carries no hits (MIN_HITS = None)
                bb.track_hits = int(hits[t, i]) if hits is not None else None
                lst.append(bb)
            out.append(lst)
        return out

    @staticmethod
    def tracks_from_result(res, clip=0):
        """Host view of the track read-out (MIN_HITS set) for one clip: list over t of BoundBox lists, one box per confirmed track
        in table order -- the frame's confirmed boxes, then the lost tracks where their velocity predicts them.  Each carries
        .label, .track_id, .track_age (0: seen in this frame), .track_hits; a track seen in this frame has the conf and score of its
        box, a coasting one 0."""
        boxes = res["boxes"][clip].cpu().numpy()
        tracks = res["tracks"][clip].cpu().numpy()
        info = res["track_info"][clip].cpu().numpy()
        tcounts = res["track_counts"][clip].cpu().numpy()
        out = []
        for t in range(tracks.shape[0]):
            lst = []
            for k in range(int(tcounts[t])):
                x, y, w, h, lab = tracks[t, k, :5]
                tid, age, nhits, box = (int(v) for v in info[t, k])
                c, sc = (boxes[t, box, 4], boxes[t, box, 6]) if box >= 0 else (0.0, 0.0)
                bb = BoundBox(x, y, w, h, c, None)
                bb.label = int(lab)
                bb.score = sc
                bb.track_id, bb.track_age, bb.track_hits = tid, age, nhits
                lst.append(bb)
            out.append(lst)
        return out

    def predict(self, input_paths, output_paths):
        """Intended behaviour of MultiObjDetTracker.py:295-315: read SEQUENCE_LENGTH
        frames, one forward of the tracker, decode the TRACKING grid of every
        time step, draw and save each frame.  Returns the per-frame box lists
        (each box carries .track_id).  With MIN_HITS set the confirmed tracks are drawn and returned instead
        (tracks_from_result): an unconfirmed box is left out, a lost track is drawn where it is expected."""
        assert len(input_paths) == self.SEQUENCE_LENGTH
        x = np.zeros((1, self.SEQUENCE_LENGTH, self.IMAGE_H, self.IMAGE_W, 3), dtype=np.uint8)
        images = []
        for i, input_path in enumerate(input_paths):
            image, resized = load_frame(input_path, self.IMAGE_H, self.IMAGE_W)
            images.append(image)
            x[0, i] = resized
        res = self.track_clips(x)
        per_frame = self.tracks_from_result(res, 0) if self.MIN_HITS is not None else self.boxes_from_result(res, 0)
        for i, boxes in enumerate(per_frame):
            image = draw_boxes(images[i], boxes, self.LABELS)
            print(len(boxes), 'Bounding Boxes Found')
            print("File Saved to", output_paths[i])
            imwrite_bgr(output_paths[i], image)
        return per_frame
