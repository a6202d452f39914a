"""ctypes binding of libmi355_dt.so (include/mi355_dt.h) for the Python host.

PyTorch-ROCm is used only as plumbing: device buffers (`tensor.data_ptr()`),
the current HIP stream and `torch.distributed`.  All compute goes through the
C ABI.  There is NO CPU fallback: if the shared library is missing, or no gfx950
device is visible, this module raises -- it never routes around the HIP path.

The binding style follows the reference's own ctypes precedent,
models_detection/YOLO.py:6-37,58-119 (libdarknet.so), with status codes added.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355_dt.so")

DT_FRAMES_U8 = 0
DT_FRAMES_F32 = 1
DT_BOX_FLOATS = 8
DT_TRACK_FLOATS = 8      # a track read-out row: x, y, w, h, label, vx, vy, 0
DT_TRACK_INTS = 4        # ... and its integers: id, age, hits, box
DT_MATCH_BEST_FIRST = 1  # track match policy bits (dt_associate_tracks_match): candidate pairs taken best IoU first
DT_MATCH_ANY_LABEL = 2   # ... labels not compared
DT_ASSIGN_IOU_SCALE = 1048576  # track assignment (dt_associate_tracks_assign): a candidate weighs 1 + trunc(IoU * this)
DT_SCORE_INTS = 8        # track scoring totals (dt_track_score): frames, gt boxes, hyp boxes, matches, switches, fragments, overflow, 0
DT_SCORE_OBJ_INTS = 8    # ... an object row: gt id, last track id, present, matched, switches, fragments, last appearance matched, 0
DT_SCORE_ANY_LABEL = 1   # ... flag bits: labels not compared
DT_SCORE_RESUME = 2      # ... totals / objs / nobjs are in-out, the call continues from them
DT_IDENT_INTS = 8        # identity scoring sizes (dt_identity_overlap): frames, gt boxes, hyp boxes, gt / hyp trajectories, gt / hyp overflow, valid pairs
DT_HOTA_MAX_THR = 32     # HOTA scoring (dt_hota_count): the most IoU thresholds of a call
DT_PIX_RGB24 = 0         # pixel formats of dt_frame_desc (dt_ingest_frames): 3 interleaved bytes per pixel, as they lie
DT_PIX_NV12 = 1          # ... plane0 = Y, plane1 = U,V interleaved, one pair per 2x2 pixels
DT_PIX_SWAP_RB = 16      # ... flag: output channels 0 and 2 exchanged
DT_FIT_STRETCH = 0       # fit modes of dt_view_fit: the whole output
DT_FIT_LETTERBOX = 1     # ... the largest centred rectangle of the source's aspect ratio
FIT_MODES = {"stretch": DT_FIT_STRETCH, "letterbox": DT_FIT_LETTERBOX}

SYMBOLS = [
    "dt_create", "dt_destroy", "dt_last_error", "dt_set_stream", "dt_abi_version",
    "dt_detector_config", "dt_load_darknet_weights", "dt_detect_forward", "dt_detector_tap", "dt_ingest_resize",
    "dt_decode", "dt_bbox_iou", "dt_tracker_load", "dt_track_forward", "dt_associate",
    "dt_tiny_load", "dt_tiny_forward", "dt_tiny_features", "dt_tiny_sequence", "dt_top_box", "dt_heatmap_from_boxes", "dt_heatmap_from_xywh64", "dt_rect_from_heatmap", "dt_encode_targets", "dt_graph_enable", "dt_conv2d", "dt_convlstm_step",
    "dt_profile_enable", "dt_profile_reset", "dt_profile_read", "dt_profile_names", "dt_policy_reload", "dt_detector_extract", "dt_decode_per_frame",
    "dt_track_row_width", "dt_track_detect", "dt_track_recurrent",
    "dt_packed_row_ints", "dt_pack_detections", "dt_unpack_detections",
    "dt_track_xproj_width", "dt_track_detect_xproj", "dt_track_recurrent_xproj",
    "dt_gemm_split_bf16", "dt_gemm_split", "dt_policy_set", "dt_amax_read",
    "dt_stream_open", "dt_stream_reset", "dt_track_stream_forward", "dt_associate_stream",
    "dt_associate_mem", "dt_stream_open_tracks", "dt_associate_stream_mem",
    "dt_associate_motion", "dt_associate_stream_motion",
    "dt_associate_tracks", "dt_associate_stream_tracks",
    "dt_associate_tracks_match", "dt_associate_stream_tracks_match",
    "dt_tiny_stream_open", "dt_tiny_stream_reset", "dt_tiny_stream_sequence", "dt_tiny_stream_forward",
    "dt_ingest_frames",
    "dt_view_fit", "dt_view_affine", "dt_ingest_views", "dt_boxes_map",
    "dt_track_score",
    "dt_detect_match", "dt_detect_rank",
    "dt_identity_overlap", "dt_assign_max",
    "dt_hota_align", "dt_hota_weights", "dt_hota_count",
    "dt_associate_tracks_assign", "dt_associate_stream_tracks_assign",
    "dt_wino_geometry", "dt_wino_input", "dt_wino_output",
    "dt_conv_igemm",
    "dt_associate_tracks_scored", "dt_associate_stream_tracks_scored",
    "dt_conv1",
]
# dt_wino_input / dt_wino_output (include/mi355_dt.h): what h_geom holds, and the codes of the kernel forms the launchers report
DT_WINO_GEOM_INTS = 10
WINO_GEOM_KEYS = ("g", "ph", "pw", "th", "tw", "Mt", "Mp", "form", "grid", "threads")
WIN_FORMS = {"tpi2": 1, "tpi4": 2, "tpi6": 3, "tpi4_s3": 4, "coop6": 5, "s3_6": 6, "s3_4": 7, "h2_6": 8, "h2_4": 9}
WOUT_FORMS = {"tpi6": 1, "tpi4": 2, "tpi2": 3, "coop6": 4, "gates6": 5, "gates4": 6, "gates2": 7}
# dt_conv_igemm (include/mi355_dt.h): the kinds it takes, the tile configurations it takes and reports, and what h_info holds
DT_CONV_INFO_INTS = 8
CONV_INFO_KEYS = ("cfg", "BM", "BN", "threads", "persistent", "grid_x", "grid_y", "total")
CONV_KINDS = {"plain": 0, "pool": 1, "pool_both": 2, "s2d": 3, "gates": 4, "partial": 5}
CONV_CFGS = {"128x128": 0, "128x64": 1, "256x128": 2, "256x256": 3, "64x128": 4}
# dt_conv1 (include/mi355_dt.h): what h_info holds and the kernel instances it reports
DT_CONV1_INFO_INTS = 6
CONV1_INFO_KEYS = ("instance", "tpw", "grid_x", "grid_y", "grid_z", "fills_amax")
CONV1_INSTANCES = {"mfma_f32": 0, "s3_u8_full": 1, "s3_u8": 2, "s3_f32": 3}

_lib = None


class NativeError(RuntimeError):
    pass


class FrameDesc(ctypes.Structure):
    """dt_frame_desc (include/mi355_dt.h): one frame of dt_ingest_frames"""
    _fields_ = [("d_plane0", ctypes.c_void_p), ("d_plane1", ctypes.c_void_p),
                ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("pitch0", ctypes.c_int32), ("pitch1", ctypes.c_int32),
                ("format", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ConvIgemmDesc(ctypes.Structure):
    """dt_conv_igemm_desc (include/mi355_dt.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("ks", "B", "H", "W", "Cin", "N", "P", "in_ld")] + [("in_bs", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("npad", "kind", "cfg", "ksplit", "act", "publish", "wg_cap")] + [("slope", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("out_ld", "out2_ld", "xp_ld", "c_ld")]


class FrameView(ctypes.Structure):
    """dt_frame_view (include/mi355_dt.h): one view of dt_ingest_views -- a frame, a source and a destination rectangle, a fill"""
    _fields_ = [("frame", FrameDesc),
                ("src_x", ctypes.c_int32), ("src_y", ctypes.c_int32), ("src_w", ctypes.c_int32), ("src_h", ctypes.c_int32),
                ("dst_x", ctypes.c_int32), ("dst_y", ctypes.c_int32), ("dst_w", ctypes.c_int32), ("dst_h", ctypes.c_int32),
                ("fill", ctypes.c_uint8 * 3), ("reserved0", ctypes.c_uint8), ("reserved", ctypes.c_int32)]


def load_library():
    """dlopen libmi355_dt.so and declare the prototypes.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "libmi355_dt.so not found at %s -- build it with `python -m object_tracking_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cf, csz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.dt_create.argtypes = [ctypes.POINTER(vp)]
    L.dt_destroy.argtypes = [vp]
    L.dt_destroy.restype = None
    L.dt_last_error.argtypes = [vp]
    L.dt_last_error.restype = ctypes.c_char_p
    L.dt_set_stream.argtypes = [vp, vp]
    L.dt_abi_version.argtypes = []
    L.dt_detector_config.argtypes = [vp, ci, ci, ci, ci, vp]
    L.dt_load_darknet_weights.argtypes = [vp, vp, csz, ctypes.POINTER(csz)]
    L.dt_detect_forward.argtypes = [vp, vp, ci, ci, vp, vp]
    L.dt_detector_tap.argtypes = [vp, ctypes.c_char_p, ci, vp]
    L.dt_detector_extract.argtypes = [vp, vp, ci, ci, ctypes.c_char_p, vp, csz, ctypes.POINTER(ci)]
    L.dt_ingest_resize.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci]
    L.dt_ingest_frames.argtypes = [vp, ctypes.POINTER(FrameDesc), ci, vp, ci, ci]
    L.dt_view_fit.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_int32)]
    L.dt_view_affine.argtypes = [ctypes.POINTER(FrameView), ci, ci, ctypes.POINTER(cf)]
    L.dt_ingest_views.argtypes = [vp, ctypes.POINTER(FrameView), ci, vp, ci, ci]
    L.dt_boxes_map.argtypes = [vp, vp, vp, ci, ci, vp]
    L.dt_decode.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, vp, ci, vp, vp, vp, vp]
    L.dt_bbox_iou.argtypes = [vp, vp, ci, vp]
    L.dt_decode_per_frame.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp]
    L.dt_tracker_load.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.dt_track_forward.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.dt_associate.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp, vp]
    L.dt_stream_open.argtypes = [vp, ci, ci]
    L.dt_stream_reset.argtypes = [vp, ctypes.POINTER(ci), ci]
    L.dt_track_stream_forward.argtypes = [vp, vp, ci, ci, ci, ctypes.POINTER(ci), vp, vp]
    L.dt_associate_stream.argtypes = [vp, vp, vp, ci, ci, ci, cf, ctypes.POINTER(ci), vp, vp]
    L.dt_associate_mem.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, vp, vp, vp]
    L.dt_stream_open_tracks.argtypes = [vp, ci, ci, ci]
    L.dt_associate_stream_mem.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ctypes.POINTER(ci), vp, vp, vp]
    L.dt_associate_motion.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, vp, vp, vp]
    L.dt_associate_stream_motion.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, cf, ctypes.POINTER(ci), vp, vp, vp]
    L.dt_associate_tracks.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, vp, vp, vp, vp, vp, vp, vp]
    L.dt_associate_stream_tracks.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, cf, ci, ctypes.POINTER(ci), vp, vp, vp, vp, vp, vp, vp]
    L.dt_associate_tracks_match.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.dt_associate_stream_tracks_match.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, cf, ci, ci, ctypes.POINTER(ci), vp, vp, vp, vp, vp, vp, vp]
    L.dt_associate_tracks_assign.argtypes = L.dt_associate_tracks_match.argtypes
    L.dt_associate_stream_tracks_assign.argtypes = L.dt_associate_stream_tracks_match.argtypes
    L.dt_associate_tracks_scored.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, ci, cf, ci, ci, ci, cf, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp]
    L.dt_associate_stream_tracks_scored.argtypes = [vp, vp, vp, ci, ci, ci, cf, ci, cf, ci, ci, ci, cf, cf, cf, ci, ctypes.POINTER(ci), vp, vp, vp, vp, vp,
                                                    vp, vp]
    L.dt_track_score.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, cf, ci, ci, vp, vp, vp, vp, vp, vp]
    L.dt_identity_overlap.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, cf, ci, ci, ci, vp, vp, vp, vp]
    L.dt_assign_max.argtypes = [vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp, vp]
    L.dt_hota_align.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    L.dt_hota_weights.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dt_hota_count.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.dt_detect_match.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, ci, ci, ci, vp, ci, vp, vp, vp]
    L.dt_detect_rank.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    L.dt_track_row_width.argtypes = [vp]
    L.dt_track_detect.argtypes = [vp, vp, ci, ci, vp]
    L.dt_track_recurrent.argtypes = [vp, vp, ci, ci, vp, vp]
    L.dt_track_xproj_width.argtypes = [vp]
    L.dt_track_detect_xproj.argtypes = [vp, vp, ci, ci, vp, vp]
    L.dt_track_recurrent_xproj.argtypes = [vp, vp, ci, ci, vp]
    L.dt_packed_row_ints.argtypes = [ci, ci]
    L.dt_pack_detections.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.dt_unpack_detections.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.dt_tiny_load.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.dt_heatmap_from_boxes.argtypes = [vp, vp, ci, ci, vp]
    L.dt_heatmap_from_xywh64.argtypes = [vp, vp, ci, ci, vp]
    L.dt_rect_from_heatmap.argtypes = [vp, vp, ci, ci, cf, vp]
    L.dt_encode_targets.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]
    L.dt_tiny_forward.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    L.dt_tiny_features.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.dt_tiny_sequence.argtypes = [vp, vp, ci, ci, vp]
    L.dt_tiny_stream_open.argtypes = [vp, ci]
    L.dt_tiny_stream_reset.argtypes = [vp, ctypes.POINTER(ci), ci]
    L.dt_tiny_stream_sequence.argtypes = [vp, vp, ci, ci, ctypes.POINTER(ci), vp]
    L.dt_tiny_stream_forward.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ci), vp]
    L.dt_top_box.argtypes = [vp, vp, vp, ci, ci, vp]
    L.dt_conv2d.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, ci, vp, cf, ci, vp, vp]
    L.dt_convlstm_step.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp]
    L.dt_gemm_split_bf16.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.dt_gemm_split.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    cll, geom = ctypes.c_longlong, ctypes.POINTER(ci)
    L.dt_wino_geometry.argtypes = [vp, ci, ci, ci, ci, ci, geom]
    L.dt_wino_input.argtypes = [vp, vp, ci, ci, ci, ci, ci, cll, ci, ci, ci, ci, ci, vp, cll, geom]
    L.dt_wino_output.argtypes = [vp, vp, cll, ci, ci, ci, ci, ci, ci, vp, vp, cf, vp, ci, vp, ci, ci, vp, ci, vp, ci, ci, ci, geom]
    L.dt_conv_igemm.argtypes = [vp, ctypes.POINTER(ConvIgemmDesc), vp, vp, vp, vp, vp, vp, vp, vp, geom]
    L.dt_conv1.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, cf, ci, ci, ci, vp, geom]
    L.dt_profile_enable.argtypes = [vp, ci]
    L.dt_graph_enable.argtypes = [vp, ci]
    L.dt_profile_reset.argtypes = [vp]
    L.dt_policy_reload.argtypes = [vp]
    L.dt_policy_set.argtypes = [vp, ctypes.c_char_p, ci]
    L.dt_amax_read.argtypes = [vp, ci, ctypes.POINTER(cf)]
    L.dt_profile_names.argtypes = [vp, ctypes.c_char_p, csz]
    L.dt_profile_read.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double)]
    for s in SYMBOLS:
        if s not in ("dt_destroy", "dt_last_error", "dt_packed_row_ints"):
            getattr(L, s).restype = ctypes.c_int
    L.dt_packed_row_ints.restype = ctypes.c_size_t
    _lib = L
    return L


def view_fit(src_w, src_h, out_w, out_h, mode="letterbox"):
    """dt_view_fit: the destination rectangle (x, y, w, h) of a src_w x src_h source in an out_w x out_h output; mode "letterbox" /
    "stretch" (or DT_FIT_*).  A host function: no context, no device."""
    rect = (ctypes.c_int32 * 4)()
    m = FIT_MODES.get(mode, mode)
    if not isinstance(m, int) or load_library().dt_view_fit(int(src_w), int(src_h), int(out_w), int(out_h), m, rect) != 0:
        raise NativeError("dt_view_fit failed (1): sizes %dx%d -> %dx%d must be >= 1 and the mode \"letterbox\" or \"stretch\", got %r"
                          % (src_w, src_h, out_w, out_h, mode))
    return tuple(int(v) for v in rect)


def view_affine(view, out_w, out_h):
    """dt_view_affine: (ax, bx, ay, by) of a mi355_dt.FrameView as a float32 numpy array [4] -- x' = x*ax + bx, y' = y*ay + by,
    w' = w*ax, h' = h*ay take a box normalised to the out_h x out_w network input to the view's whole source frame."""
    a = (ctypes.c_float * 4)()
    if load_library().dt_view_affine(ctypes.byref(view), int(out_w), int(out_h), a) != 0:
        raise NativeError("dt_view_affine failed (1): the output, the destination rectangle and the frame must be at least 1x1")
    return np.array(a[:], dtype=np.float32)


def _hptr(a):
    """host float32 array -> (keepalive, void*)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Context(object):
    """One dt_ctx (one GPU, one process)."""

    def __init__(self, device=None):
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise NativeError("no HIP device visible to PyTorch-ROCm; the MI355X path has no CPU fallback")
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        h = ctypes.c_void_p()
        rc = self.lib.dt_create(ctypes.byref(h))
        if rc != 0:
            raise NativeError("dt_create failed (%d): %s" % (rc, self.lib.dt_last_error(None).decode()))
        self.h = h
        self.pin = -1                   # the pin override last handed to dt_policy_set (-1: DT_PIN decides)
        self.cb = None
        self.grid = None
        self.nb_box = None
        self.nb_class = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.dt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise NativeError("%s failed (%d): %s" % (what, rc, self.lib.dt_last_error(self.h).decode()))

    def _sync_stream(self):
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        self.lib.dt_set_stream(self.h, ctypes.c_void_p(st))

    def _f32(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float32, device=self.device)

    # ---- detector -----------------------------------------------------
    def detector_config(self, image_h, image_w, nb_box, nb_class, anchors):
        keep, p = _hptr(anchors)
        self._check(self.lib.dt_detector_config(self.h, image_h, image_w, nb_box, nb_class, p), "dt_detector_config")
        self.image_h, self.image_w = image_h, image_w
        self.nb_box, self.nb_class = nb_box, nb_class
        self.cb = nb_box * (5 + nb_class)
        self.grid = (image_h // 32, image_w // 32)

    def load_darknet_weights(self, blob):
        keep, p = _hptr(blob)
        used = ctypes.c_size_t(0)
        self._check(self.lib.dt_load_darknet_weights(self.h, p, keep.size, ctypes.byref(used)), "dt_load_darknet_weights")
        return used.value

    def _frames_dtype(self, frames):
        t = self.torch
        if frames.dtype == t.uint8:
            return DT_FRAMES_U8
        if frames.dtype == t.float32:
            return DT_FRAMES_F32
        raise NativeError("frames must be uint8 or float32, got %s" % frames.dtype)

    def detect_forward(self, frames, want_feat=False):
        """frames [B,H,W,3] device tensor -> netout [B,G,G,nb_box,5+C] (+ feat [B,G,G,1024])."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        B = frames.shape[0]
        gh, gw = self.grid
        netout = self._f32(B, gh, gw, self.nb_box, 5 + self.nb_class)
        feat = self._f32(B, gh, gw, 1024) if want_feat else None
        self._sync_stream()
        self._check(self.lib.dt_detect_forward(self.h, _dptr(frames), self._frames_dtype(frames), B,
                                               _dptr(netout), _dptr(feat)), "dt_detect_forward")
        return (netout, feat) if want_feat else netout

    def detect_forward_internal(self, frames):
        """Forward into the context's own workspaces (for dt_detector_tap)."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        self._sync_stream()
        self._check(self.lib.dt_detect_forward(self.h, _dptr(frames), self._frames_dtype(frames), frames.shape[0],
                                               None, None), "dt_detect_forward")

    def detector_tap(self, name, batch):
        H, W = self.image_h, self.image_w
        shape = {"act_13": (batch, H // 16, W // 16, 512), "conv_feat": (batch, H // 32, W // 32, 1024),
                 "conv_23": (batch, H // 32, W // 32, self.cb)}[name]
        out = self._f32(*shape)
        self._sync_stream()
        self._check(self.lib.dt_detector_tap(self.h, name.encode(), batch, _dptr(out)), "dt_detector_tap")
        return out

    def layer_shape(self, layer, batch=1):
        """(batch, h, w, channels) of a named detector layer; raises NativeError for an unknown name."""
        shape = (ctypes.c_int * 4)()
        self._check(self.lib.dt_detector_extract(self.h, None, 0, batch, layer.encode(), None, 0, shape), "dt_detector_extract")
        return tuple(int(v) for v in shape)

    def detector_extract(self, frames, layer):
        """frames [B,H,W,3] device tensor -> the named layer's output [B,h,w,C] (KerasYOLO.extract, any layer)."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        B = frames.shape[0]
        shape = (ctypes.c_int * 4)()
        self._check(self.lib.dt_detector_extract(self.h, None, 0, B, layer.encode(), None, 0, shape), "dt_detector_extract")
        out = self._f32(*[int(v) for v in shape])
        self._sync_stream()
        self._check(self.lib.dt_detector_extract(self.h, _dptr(frames), self._frames_dtype(frames), B, layer.encode(),
                                                 _dptr(out), out.numel(), shape), "dt_detector_extract")
        return out

    # ---- frame ingest -------------------------------------------------
    def ingest_resize(self, frames, out_h, out_w):
        """frames uint8 [n,Hs,Ws,3] device tensor -> uint8 [n,out_h,out_w,3] (cv2.resize INTER_LINEAR)."""
        t = self.torch
        assert frames.is_cuda and frames.dtype == t.uint8 and frames.is_contiguous() and frames.dim() == 4
        n, Hs, Ws, _ = frames.shape
        out = t.empty((n, out_h, out_w, 3), dtype=t.uint8, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_ingest_resize(self.h, _dptr(frames), n, Hs, Ws, _dptr(out), out_h, out_w),
                    "dt_ingest_resize")
        return out

    def _frame_desc(self, i, item, flags, entry="dt_ingest_frames"):
        """item i of ingest_frames / ingest_views -> FrameDesc; the tensors are read as they lie (no copy)"""
        t = self.torch
        head = "%s failed (1): frame %d: " % (entry, i)

        def plane(x, what, dims):
            if not t.is_tensor(x):
                raise NativeError(head + "%s is not a tensor" % what)
            if not x.is_cuda or x.dtype != t.uint8:
                raise NativeError(head + "%s must be a uint8 device tensor, got %s on %s"
                                  % (what, x.dtype, x.device))
            if x.dim() != dims:
                raise NativeError(head + "%s has %d axes, not %d" % (what, x.dim(), dims))
            return x

        def pitch(x, what, inner):
            """rows at any pitch, the bytes of a row dense: strides (pitch, *inner); the stride of an axis of one element says nothing"""
            st, row = tuple(x.stride()), int(np.prod(x.shape[1:]))
            if any(x.shape[1 + k] > 1 and st[1 + k] != v for k, v in enumerate(inner)) or (x.shape[0] > 1 and st[0] < row):
                raise NativeError(head + "%s has strides %s; a row must be dense and the rows apart, strides (pitch, %s)"
                                  % (what, st, ", ".join(str(v) for v in inner)))
            return int(st[0]) if x.shape[0] > 1 else row

        if isinstance(item, (tuple, list)):
            if len(item) != 2:
                raise NativeError(head + "an NV12 item is a pair (y, uv), got %d items" % len(item))
            y, uv = plane(item[0], "y", 2), plane(item[1], "uv", 3)
            H, W = int(y.shape[0]), int(y.shape[1])
            if tuple(uv.shape) != (H // 2, W // 2, 2) or H % 2 or W % 2:
                raise NativeError(head + "y is %dx%d (both must be even) and uv must be [%d, %d, 2], got %s"
                                  % (H, W, H // 2, W // 2, tuple(uv.shape)))
            return FrameDesc(y.data_ptr(), uv.data_ptr(), H, W, pitch(y, "y", (1,)), pitch(uv, "uv", (2, 1)), DT_PIX_NV12 | flags, 0)
        x = plane(item, "the frame", 3)
        if x.shape[2] != 3:
            raise NativeError(head + "an RGB24 frame is [H, W, 3], got %s" % (tuple(x.shape),))
        return FrameDesc(x.data_ptr(), None, int(x.shape[0]), int(x.shape[1]), pitch(x, "the frame", (3, 1)), 0, DT_PIX_RGB24 | flags, 0)

    def ingest_frames(self, frames, out_h, out_w, swap_rb=False, out=None):
        """frames: a sequence whose items are uint8 device tensors [H,W,3] with strides (pitch, 3, 1) (a row-pitched view is taken as it
        lies) or NV12 pairs (y [H,W] at strides (pitch, 1), uv [H/2,W/2,2] at strides (pitch, 2, 1)), every item at its own size
        -> uint8 [n,out_h,out_w,3] (dt_ingest_frames: NV12 -> RGB where needed, then dt_ingest_resize's resize).  swap_rb: channels 0 and
        2 of the result exchanged.  out: a preallocated contiguous [n,out_h,out_w,3] uint8 device tensor to fill instead."""
        t = self.torch
        if t.is_tensor(frames) or not isinstance(frames, (list, tuple)):
            raise NativeError("dt_ingest_frames failed (1): frames must be a list or tuple of frames, got %s" % type(frames).__name__)
        n = len(frames)
        flags = DT_PIX_SWAP_RB if swap_rb else 0
        desc = (FrameDesc * max(1, n))(*[self._frame_desc(i, item, flags) for i, item in enumerate(frames)])
        if out is None:
            out = t.empty((n, out_h, out_w, 3), dtype=t.uint8, device=self.device)
        elif not (t.is_tensor(out) and out.is_cuda and out.dtype == t.uint8 and out.is_contiguous() and tuple(out.shape) == (n, out_h, out_w, 3)):
            raise NativeError("dt_ingest_frames failed (1): out must be a contiguous uint8 device tensor [%d, %d, %d, 3]" % (n, out_h, out_w))
        self._sync_stream()
        self._check(self.lib.dt_ingest_frames(self.h, desc, n, _dptr(out), int(out_h), int(out_w)), "dt_ingest_frames")
        return out

    def _frame_view(self, i, item, flags, out_h, out_w, fit, fill):
        """item i of ingest_views -> FrameView.  An item with a `.frame` attribute is a view description (utility.frames.FrameView:
        frame, crop, fit, fill, dst); anything else is a frame of ingest_frames, taken whole with the call's fit and fill."""
        head = "dt_ingest_views failed (1): frame %d: " % i
        crop = dst = None
        if hasattr(item, "frame"):
            crop, dst = getattr(item, "crop", None), getattr(item, "dst", None)
            fit = getattr(item, "fit", None) or fit
            fill = getattr(item, "fill", None) or fill
            item = item.frame

        def rect(r, what):
            try:
                r = tuple(r)
                ok = len(r) == 4 and all(int(v) == v and -2 ** 31 <= v < 2 ** 31 for v in r)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise NativeError(head + "%s must be four integers (x, y, w, h), got %r" % (what, r))
            return tuple(int(v) for v in r)

        d = self._frame_desc(i, item, flags, entry="dt_ingest_views")
        sx, sy, sw, sh = (0, 0, d.width, d.height) if crop is None else rect(crop, "crop")
        if dst is not None:
            dx, dy, dw, dh = rect(dst, "dst")
        else:
            if fit not in FIT_MODES:
                raise NativeError(head + "fit must be \"letterbox\" or \"stretch\", got %r" % (fit,))
            if sw < 1 or sh < 1:
                raise NativeError(head + "crop (%d, %d, %d, %d) is empty" % (sx, sy, sw, sh))
            dx, dy, dw, dh = view_fit(sw, sh, out_w, out_h, fit)
        try:
            fill = tuple(fill)
            ok = len(fill) == 3 and all(int(v) == v and 0 <= v <= 255 for v in fill)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise NativeError(head + "fill must be three bytes, got %r" % (fill,))
        return FrameView(d, sx, sy, sw, sh, dx, dy, dw, dh, (ctypes.c_uint8 * 3)(*[int(v) for v in fill]), 0, 0)

    def ingest_views(self, views, out_h, out_w, swap_rb=False, out=None, fit="letterbox", fill=(128, 128, 128)):
        """views: a sequence whose items are view descriptions (utility.frames.FrameView: a frame, a crop, a fit or an explicit
        destination rectangle, a fill) or plain frames of ingest_frames, which are taken whole with this call's `fit` and `fill`
        -> (frames uint8 [n,out_h,out_w,3], affine float32 numpy [n,4]) (dt_ingest_views: every crop converted, resized into its
        destination rectangle, the fill around it; dt_view_affine: the (ax, bx, ay, by) that boxes_map takes).  swap_rb and out as for
        ingest_frames; the fill is written as it is, whatever swap_rb says."""
        t = self.torch
        if t.is_tensor(views) or not isinstance(views, (list, tuple)):
            raise NativeError("dt_ingest_views failed (1): views must be a list or tuple of views, got %s" % type(views).__name__)
        n = len(views)
        flags = DT_PIX_SWAP_RB if swap_rb else 0
        arr = (FrameView * max(1, n))(*[self._frame_view(i, item, flags, int(out_h), int(out_w), fit, fill) for i, item in enumerate(views)])
        if out is None:
            out = t.empty((n, out_h, out_w, 3), dtype=t.uint8, device=self.device)
        elif not (t.is_tensor(out) and out.is_cuda and out.dtype == t.uint8 and out.is_contiguous() and tuple(out.shape) == (n, out_h, out_w, 3)):
            raise NativeError("dt_ingest_views failed (1): out must be a contiguous uint8 device tensor [%d, %d, %d, 3]" % (n, out_h, out_w))
        self._sync_stream()
        self._check(self.lib.dt_ingest_views(self.h, arr, n, _dptr(out), int(out_h), int(out_w)), "dt_ingest_views")
        affine = np.empty((n, 4), dtype=np.float32)
        for i in range(n):
            affine[i] = view_affine(arr[i], out_w, out_h)
        return out, affine

    def boxes_map(self, boxes, counts, affine):
        """boxes [..., cap, 8] device float32, counts int32 of the leading shape, affine float32 [frames, 4] on the host (ingest_views'):
        x, y, w, h of rows < min(count, cap) of every frame mapped IN PLACE (dt_boxes_map); [R, T, cap, 8] counts as R*T frames.
        Returns boxes."""
        t = self.torch
        assert boxes.is_cuda and boxes.dtype == t.float32 and boxes.is_contiguous() and boxes.dim() >= 2 and boxes.shape[-1] == DT_BOX_FLOATS
        assert counts.is_cuda and counts.dtype == t.int32 and counts.is_contiguous()
        cap = int(boxes.shape[-2])
        n = boxes.numel() // max(1, cap * DT_BOX_FLOATS)
        a = np.ascontiguousarray(affine, dtype=np.float32).reshape(-1, 4)
        if counts.numel() != n or a.shape[0] != n:
            raise NativeError("dt_boxes_map failed (1): %d frames of boxes, %d counts, %d affines" % (n, counts.numel(), a.shape[0]))
        self._sync_stream()
        self._check(self.lib.dt_boxes_map(self.h, _dptr(boxes), _dptr(counts), n, cap, a.ctypes.data_as(ctypes.c_void_p)), "dt_boxes_map")
        return boxes

    # ---- decode -------------------------------------------------------
    def decode(self, netout, obj_threshold, nms_threshold, anchors, nb_class, cap=None,
               want_classes=False, want_post=False):
        """netout [B,GH,GW,NB,5+C] device float32 (not modified).  Returns dict of
        device tensors: boxes [B,cap,8], counts [B] (+ classes, post).  obj_threshold / nms_threshold are
        scalars, or arrays / tensors of one value per frame (dt_decode_per_frame)."""
        t = self.torch
        assert netout.is_cuda and netout.dtype == t.float32 and netout.is_contiguous() and netout.dim() == 5
        B, GH, GW, NB, S = netout.shape
        assert S == 5 + nb_class
        if cap is None:
            cap = GH * GW * NB
        boxes = t.empty((B, cap, DT_BOX_FLOATS), dtype=t.float32, device=self.device)   # the kernel zero-fills rows >= count
        counts = t.empty((B,), dtype=t.int32, device=self.device)
        classes = t.zeros((B, cap, nb_class), dtype=t.float32, device=self.device) if want_classes else None
        post = t.empty_like(netout) if want_post else None
        keep, ap = _hptr(anchors)
        self._sync_stream()
        if np.ndim(obj_threshold) or np.ndim(nms_threshold) or t.is_tensor(obj_threshold) or t.is_tensor(nms_threshold):
            def per_frame(v):
                v = v.detach().cpu().numpy() if t.is_tensor(v) else np.asarray(v)
                return np.broadcast_to(v.astype(np.float32).reshape(-1), (B,))
            thr = t.from_numpy(np.ascontiguousarray(np.stack([per_frame(obj_threshold), per_frame(nms_threshold)], 1))).to(self.device)
            self._check(self.lib.dt_decode_per_frame(self.h, _dptr(netout), B, GH, GW, NB, nb_class, _dptr(thr), ap, cap,
                                                     _dptr(boxes), _dptr(counts), _dptr(classes), _dptr(post)),
                        "dt_decode_per_frame")
        else:
            self._check(self.lib.dt_decode(self.h, _dptr(netout), B, GH, GW, NB, nb_class, float(obj_threshold),
                                           float(nms_threshold), ap, cap, _dptr(boxes), _dptr(counts),
                                           _dptr(classes), _dptr(post)), "dt_decode")
        return dict(boxes=boxes, counts=counts, classes=classes, post=post)

    def bbox_iou(self, pairs):
        t = self.torch
        assert pairs.is_cuda and pairs.dtype == t.float32 and pairs.is_contiguous()
        n = pairs.shape[0]
        out = self._f32(n)
        self._sync_stream()
        self._check(self.lib.dt_bbox_iou(self.h, _dptr(pairs), n, _dptr(out)), "dt_bbox_iou")
        return out

    def associate(self, boxes, counts, assoc_threshold, max_age=0, track_cap=None, want_gaps=False, motion_gain=None):
        """boxes [n_clips,T,cap,8], counts [n_clips,T] int32 -> ids [n_clips,T,cap], nids [n_clips].
        max_age > 0, a track_cap or want_gaps: the track-memory rule (dt_associate_mem) -- a track that misses up to max_age frames keeps
        its id, the table of tracks holds track_cap (None: cap) entries; with want_gaps the result is (ids, nids, gaps [n_clips,T,cap]).
        motion_gain (a number in [0, 1]; None: none of it): the track-motion rule (dt_associate_motion) -- the memory rule with every
        track matched where its velocity predicts it, whatever max_age is."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n_clips, T, cap, _ = boxes.shape
        ids = t.empty((n_clips, T, cap), dtype=t.int32, device=self.device)
        nids = t.empty((n_clips,), dtype=t.int32, device=self.device)
        self._sync_stream()
        if motion_gain is not None:
            gaps = t.empty((n_clips, T, cap), dtype=t.int32, device=self.device) if want_gaps else None
            self._check(self.lib.dt_associate_motion(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold), int(max_age),
                                                     cap if track_cap is None else int(track_cap), float(motion_gain), _dptr(ids), _dptr(nids),
                                                     _dptr(gaps)), "dt_associate_motion")
            return (ids, nids, gaps) if want_gaps else (ids, nids)
        if max_age != 0 or track_cap is not None or want_gaps:
            gaps = t.empty((n_clips, T, cap), dtype=t.int32, device=self.device) if want_gaps else None
            self._check(self.lib.dt_associate_mem(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold), int(max_age),
                                                  cap if track_cap is None else int(track_cap), _dptr(ids), _dptr(nids), _dptr(gaps)),
                        "dt_associate_mem")
            return (ids, nids, gaps) if want_gaps else (ids, nids)
        self._check(self.lib.dt_associate(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap,
                                          float(assoc_threshold), _dptr(ids), _dptr(nids)), "dt_associate")
        return ids, nids

    # ---- cross-stream exchange ------------------------------------------
    def _tracks_outputs(self, n, T, cap, tcap, readout=True):
        t = self.torch
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        if not readout:
            return dict(ids=i32(n, T, cap), nids=i32(n), gaps=i32(n, T, cap), hits=i32(n, T, cap))
        return dict(ids=i32(n, T, cap), nids=i32(n), gaps=i32(n, T, cap), hits=i32(n, T, cap),
                    tracks=t.empty((n, T, tcap, DT_TRACK_FLOATS), dtype=t.float32, device=self.device),
                    track_info=i32(n, T, tcap, DT_TRACK_INTS), track_counts=i32(n, T))

    def associate_tracks(self, boxes, counts, assoc_threshold, max_age, gain, min_hits, track_cap=None, match=0, readout=True, assign=False):
        """The track-motion rule with a hit count per track and the read-out of the confirmed tracks (dt_associate_tracks).
        boxes [n_clips,T,cap,8], counts [n_clips,T] int32 -> dict: ids, gaps, hits [n_clips,T,cap], nids [n_clips] (ids, nids, gaps are
        associate(..., motion_gain=gain)'s; hits = frames in which the box's track has had a box), and per frame the tracks with
        hits >= min_hits in table order -- the frame's boxes, then the lost tracks at their predicted place:
        tracks [n_clips,T,tcap,8] (x, y, w, h, label, vx, vy, 0), track_info [n_clips,T,tcap,4] (id, age, hits, box; box = -1 for a
        coasting track), track_counts [n_clips,T]; rows from the count on are 0 / -1.  tcap = track_cap (None: cap).
        match: the track match policy, DT_MATCH_BEST_FIRST | DT_MATCH_ANY_LABEL bits (dt_associate_tracks_match); 0 = boxes in decode
        order, entries of the box's label (dt_associate_tracks).  readout=False: no tracks / track_info / track_counts (the NULL triple).
        assign=True: the match of a frame is the optimal (maximum summed IoU) one-to-one assignment (dt_associate_tracks_assign); match
        may then be 0 or DT_MATCH_ANY_LABEL, and the library refuses DT_MATCH_BEST_FIRST."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n_clips, T, cap, _ = boxes.shape
        tcap = cap if track_cap is None else int(track_cap)
        r = self._tracks_outputs(n_clips, T, cap, max(tcap, 0), readout)
        self._sync_stream()
        if assign:
            self._check(self.lib.dt_associate_tracks_assign(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold),
                                                            int(max_age), tcap, float(gain), int(min_hits), int(match), _dptr(r["ids"]),
                                                            _dptr(r["nids"]), _dptr(r["gaps"]), _dptr(r["hits"]), _dptr(r.get("tracks")),
                                                            _dptr(r.get("track_info")), _dptr(r.get("track_counts"))), "dt_associate_tracks_assign")
            return r
        if match != 0:
            self._check(self.lib.dt_associate_tracks_match(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold),
                                                           int(max_age), tcap, float(gain), int(min_hits), int(match), _dptr(r["ids"]),
                                                           _dptr(r["nids"]), _dptr(r["gaps"]), _dptr(r["hits"]), _dptr(r.get("tracks")),
                                                           _dptr(r.get("track_info")), _dptr(r.get("track_counts"))), "dt_associate_tracks_match")
            return r
        self._check(self.lib.dt_associate_tracks(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold), int(max_age),
                                                 tcap, float(gain), int(min_hits), _dptr(r["ids"]), _dptr(r["nids"]), _dptr(r["gaps"]),
                                                 _dptr(r["hits"]), _dptr(r.get("tracks")), _dptr(r.get("track_info")), _dptr(r.get("track_counts"))),
                    "dt_associate_tracks")
        return r

    def associate_tracks_scored(self, boxes, counts, assoc_threshold, max_age, gain, min_hits, score_high, score_new=None,
                                assoc_threshold_low=None, max_age_low=0, score_at=6, track_cap=None, match=0, readout=True):
        """associate_tracks(..., assign=True) in two passes by detection score (dt_associate_tracks_scored; DESIGN.md "Track scores"): the
        boxes whose float score_at is >= score_high are assigned first; the others are offered to the tracks still unmatched, no older
        than min(max_age, max_age_low), at assoc_threshold_low (max_age_low = -1: not at all); an unmatched box opens an id only with a
        score >= score_new and is dropped otherwise: ids -1, gaps -1, hits 0.  score_new None: score_high; assoc_threshold_low None:
        assoc_threshold.  match: 0 or DT_MATCH_ANY_LABEL.  The dict of associate_tracks."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n_clips, T, cap, _ = boxes.shape
        tcap = cap if track_cap is None else int(track_cap)
        r = self._tracks_outputs(n_clips, T, cap, max(tcap, 0), readout)
        self._sync_stream()
        self._check(self.lib.dt_associate_tracks_scored(self.h, _dptr(boxes), _dptr(counts), n_clips, T, cap, float(assoc_threshold), int(max_age),
                                                        tcap, float(gain), int(min_hits), int(match), int(score_at), float(score_high),
                                                        float(score_high if score_new is None else score_new),
                                                        float(assoc_threshold if assoc_threshold_low is None else assoc_threshold_low),
                                                        int(max_age_low), _dptr(r["ids"]), _dptr(r["nids"]), _dptr(r["gaps"]), _dptr(r["hits"]),
                                                        _dptr(r.get("tracks")), _dptr(r.get("track_info")), _dptr(r.get("track_counts"))),
                    "dt_associate_tracks_scored")
        return r

    def track_score(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, iou_threshold=0.5, any_label=False, obj_cap=None,
                    state=None, per_box=True):
        """CLEAR-MOT counts of a tracker's output against ground-truth tracks (dt_track_score; the rule: DESIGN.md "Track scoring").
        gt_boxes [n,T,gcap,8] (x, y, w, h in floats 0..3, the label in float 5), gt_counts [n,T] int32, gt_ids [n,T,gcap] int32;
        hyp_boxes [n,T,hcap,8] with hyp_counts [n,T] and hyp_ids either [n,T,hcap] int32 -- `boxes` / `counts` / `ids` of an association
        result, the label in float 5 -- or a [n,T,hcap,4] `track_info` beside `tracks` / `track_counts`, the label in float 4.
        -> dict: totals [n,8] (frames, gt, hyp, matches, switches, fragments, overflow, 0), objs [n,obj_cap,8] (gt id, last track id,
        present, matched, switches, fragments, last appearance matched, 0), nobjs [n], frame_counts [n,T,4] (gt, hyp, matches, switches)
        and, with per_box, match [n,T,gcap] (hypothesis row or -1) and miou [n,T,gcap] (else both None).
        obj_cap: rows of the object table (None: the state's, or max(64, 2 * gcap)); ids beyond it are scored without memory and counted
        in `overflow`.  state: a previous result whose totals / objs / nobjs this call continues (they are copied, not written): chunks
        of any sizes along T give the result of one call on the concatenation.  utility.evaluate.summarize turns it into MOTA etc."""
        t = self.torch
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        n, T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[2]
        assert hyp_boxes.shape[:2] == (n, T) and hyp_boxes.shape[3] == 8 and gt_boxes.shape[3] == DT_BOX_FLOATS
        if hyp_ids.dim() == 4:
            stride, label_at = int(hyp_ids.shape[3]), 4
        else:
            stride, label_at = 1, 5
        assert tuple(hyp_ids.shape[:3]) == (n, T, hcap) and tuple(gt_ids.shape) == (n, T, gcap)
        assert tuple(gt_counts.shape) == (n, T) and tuple(hyp_counts.shape) == (n, T)
        for x, dt in ((gt_boxes, t.float32), (hyp_boxes, t.float32), (gt_counts, t.int32), (gt_ids, t.int32), (hyp_counts, t.int32),
                      (hyp_ids, t.int32)):
            assert x.is_cuda and x.is_contiguous() and x.dtype == dt
        flags = DT_SCORE_ANY_LABEL if any_label else 0
        if state is not None:
            ocap = int(state["objs"].shape[1])
            assert obj_cap is None or int(obj_cap) == ocap, "obj_cap differs from the state's"
            assert int(state["objs"].shape[0]) == n
            totals, objs, nobjs = state["totals"].clone(), state["objs"].clone(), state["nobjs"].clone()
            flags |= DT_SCORE_RESUME
        else:
            ocap = max(64, 2 * gcap) if obj_cap is None else int(obj_cap)
            totals, objs, nobjs = i32(n, DT_SCORE_INTS), i32(n, max(ocap, 0), DT_SCORE_OBJ_INTS), i32(n)
        r = dict(totals=totals, objs=objs, nobjs=nobjs, frame_counts=i32(n, T, 4),
                 match=i32(n, T, gcap) if per_box else None,
                 miou=t.empty((n, T, gcap), dtype=t.float32, device=self.device) if per_box else None)
        self._sync_stream()
        self._check(self.lib.dt_track_score(self.h, _dptr(gt_boxes), _dptr(gt_counts), _dptr(gt_ids), gcap, _dptr(hyp_boxes), _dptr(hyp_counts),
                                            _dptr(hyp_ids), hcap, stride, label_at, n, T, float(iou_threshold), flags, ocap, _dptr(totals),
                                            _dptr(objs), _dptr(nobjs), _dptr(r["frame_counts"]), _dptr(r["match"]), _dptr(r["miou"])),
                    "dt_track_score")
        return r

    def identity_overlap(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, iou_threshold=0.5, any_label=False, gt_cap=None,
                         hyp_cap=None, state=None):
        """The overlap of ground-truth trajectories with hypothesis trajectories (dt_identity_overlap; the rule: DESIGN.md "Identity
        scoring").  The six inputs, iou_threshold and any_label are track_score's.
        -> dict: sizes [n,8] (frames, gt boxes, hyp boxes, gt trajectories, hyp trajectories, gt overflow boxes, hyp overflow boxes,
        valid pairs), gt_tab [n,gt_cap,2] and hyp_tab [n,hyp_cap,2] (id, boxes; unused rows -1, 0), overlap [n,gt_cap,hyp_cap] int32.
        gt_cap / hyp_cap: rows of the two tables (None: the state's, or max(64, 2 * gcap) / max(64, 2 * hcap)); boxes of ids beyond
        them are counted as overflow and take no part.  state: a previous result this call continues (copied, not written): chunks of
        any sizes along T give the result of one call on the concatenation."""
        t = self.torch
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        n, T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[2]
        assert hyp_boxes.shape[:2] == (n, T) and hyp_boxes.shape[3] == 8 and gt_boxes.shape[3] == DT_BOX_FLOATS
        if hyp_ids.dim() == 4:
            stride, label_at = int(hyp_ids.shape[3]), 4
        else:
            stride, label_at = 1, 5
        assert tuple(hyp_ids.shape[:3]) == (n, T, hcap) and tuple(gt_ids.shape) == (n, T, gcap)
        assert tuple(gt_counts.shape) == (n, T) and tuple(hyp_counts.shape) == (n, T)
        for x, dt in ((gt_boxes, t.float32), (hyp_boxes, t.float32), (gt_counts, t.int32), (gt_ids, t.int32), (hyp_counts, t.int32),
                      (hyp_ids, t.int32)):
            assert x.is_cuda and x.is_contiguous() and x.dtype == dt
        flags = DT_SCORE_ANY_LABEL if any_label else 0
        if state is not None:
            acap, bcap = int(state["gt_tab"].shape[1]), int(state["hyp_tab"].shape[1])
            assert gt_cap is None or int(gt_cap) == acap, "gt_cap differs from the state's"
            assert hyp_cap is None or int(hyp_cap) == bcap, "hyp_cap differs from the state's"
            assert int(state["sizes"].shape[0]) == n and tuple(state["overlap"].shape) == (n, acap, bcap)
            r = {k: state[k].clone() for k in ("sizes", "gt_tab", "hyp_tab", "overlap")}
            flags |= DT_SCORE_RESUME
        else:
            acap = max(64, 2 * gcap) if gt_cap is None else int(gt_cap)
            bcap = max(64, 2 * hcap) if hyp_cap is None else int(hyp_cap)
            r = dict(sizes=i32(n, DT_IDENT_INTS), gt_tab=i32(n, max(acap, 0), 2), hyp_tab=i32(n, max(bcap, 0), 2),
                     overlap=i32(n, max(acap, 0), max(bcap, 0)))
        self._sync_stream()
        self._check(self.lib.dt_identity_overlap(self.h, _dptr(gt_boxes), _dptr(gt_counts), _dptr(gt_ids), gcap, _dptr(hyp_boxes),
                                                 _dptr(hyp_counts), _dptr(hyp_ids), hcap, stride, label_at, n, T, float(iou_threshold), flags,
                                                 acap, bcap, _dptr(r["sizes"]), _dptr(r["gt_tab"]), _dptr(r["hyp_tab"]), _dptr(r["overlap"])),
                    "dt_identity_overlap")
        return r

    def assign_max(self, weights, dims=None, rows_at=0, cols_at=1):
        """An exact one-to-one assignment of maximum total weight per problem (dt_assign_max; DESIGN.md "Identity scoring").
        weights [n,rcap,ccap] int32 on the device, each in [0, 2^24]; dims [n,k] int32 with the rows and columns in use of problem i
        in words rows_at and cols_at (None: every problem is rcap x ccap).
        -> (row_to_col [n,rcap] int32, col_to_row [n,ccap] int32, total [n] int64): the partner or -1 -- a pair of weight 0 is
        reported as unassigned -- and the sum of the chosen weights."""
        t = self.torch
        n, rcap, ccap = weights.shape
        assert weights.is_cuda and weights.is_contiguous() and weights.dtype == t.int32
        if dims is None:
            dims = t.tensor([[rcap, ccap]], dtype=t.int32, device=self.device).repeat(n, 1).contiguous()
            rows_at, cols_at = 0, 1
        assert dims.dim() == 2 and int(dims.shape[0]) == n and dims.is_cuda and dims.is_contiguous() and dims.dtype == t.int32
        r2c = t.empty((n, rcap), dtype=t.int32, device=self.device)
        c2r = t.empty((n, ccap), dtype=t.int32, device=self.device)
        total = t.empty((n,), dtype=t.int64, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_assign_max(self.h, _dptr(weights), rcap, ccap, _dptr(dims), int(dims.shape[1]), int(rows_at), int(cols_at), n,
                                           _dptr(r2c), _dptr(c2r), _dptr(total)), "dt_assign_max")
        return r2c, c2r, total

    def identity_score(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, iou_threshold=0.5, any_label=False, gt_cap=None,
                       hyp_cap=None, state=None):
        """identity_overlap, then assign_max on its overlap with the trajectory counts of `sizes`: the overlap's dict plus gt_to_hyp
        [n,gt_cap], hyp_to_gt [n,hyp_cap] (rows of the other table, or -1) and idtp [n] int64.  utility.evaluate.identity turns it
        into IDF1 etc.  `state` is a previous result (of either method); the assignment is solved anew on the accumulated overlap."""
        r = self.identity_overlap(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, iou_threshold, any_label, gt_cap, hyp_cap, state)
        r["gt_to_hyp"], r["hyp_to_gt"], r["idtp"] = self.assign_max(r["overlap"], r["sizes"], 3, 4)
        return r

    def _hota_inputs(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids):
        """the checks of identity_overlap's six inputs -> (n, T, gcap, hcap, id_stride, label_at)"""
        t = self.torch
        n, T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[2]
        assert hyp_boxes.shape[:2] == (n, T) and hyp_boxes.shape[3] == 8 and gt_boxes.shape[3] == DT_BOX_FLOATS
        if hyp_ids.dim() == 4:
            stride, label_at = int(hyp_ids.shape[3]), 4
        else:
            stride, label_at = 1, 5
        assert tuple(hyp_ids.shape[:3]) == (n, T, hcap) and tuple(gt_ids.shape) == (n, T, gcap)
        assert tuple(gt_counts.shape) == (n, T) and tuple(hyp_counts.shape) == (n, T)
        for x, dt in ((gt_boxes, t.float32), (hyp_boxes, t.float32), (gt_counts, t.int32), (gt_ids, t.int32), (hyp_counts, t.int32),
                      (hyp_ids, t.int32)):
            assert x.is_cuda and x.is_contiguous() and x.dtype == dt
        return n, T, gcap, hcap, stride, label_at

    def hota_align(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, any_label=False, gt_cap=None, hyp_cap=None, state=None):
        """Pass 1 of HOTA scoring (dt_hota_align; the rule: DESIGN.md "HOTA scoring"): the alignment of ground-truth trajectories with
        hypothesis trajectories over a clip.  The six inputs, any_label, gt_cap / hyp_cap and state are identity_overlap's.
        -> dict: sizes [n,8], gt_tab [n,gt_cap,2], hyp_tab [n,hyp_cap,2] as identity_overlap gives them (sizes word 7: the pairs of
        similarity > 0), align [n,gt_cap,hyp_cap] int64, and any_label.  state: a previous result this call continues (copied, not
        written): chunks of any sizes along T give the result of one call on the concatenation."""
        t = self.torch
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        n, T, gcap, hcap, stride, label_at = self._hota_inputs(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids)
        flags = DT_SCORE_ANY_LABEL if any_label else 0
        if state is not None:
            acap, bcap = int(state["gt_tab"].shape[1]), int(state["hyp_tab"].shape[1])
            assert gt_cap is None or int(gt_cap) == acap, "gt_cap differs from the state's"
            assert hyp_cap is None or int(hyp_cap) == bcap, "hyp_cap differs from the state's"
            assert int(state["sizes"].shape[0]) == n and tuple(state["align"].shape) == (n, acap, bcap)
            assert bool(state["any_label"]) == bool(any_label), "any_label differs from the state's"
            r = {k: state[k].clone() for k in ("sizes", "gt_tab", "hyp_tab", "align")}
            flags |= DT_SCORE_RESUME
        else:
            acap = max(64, 2 * gcap) if gt_cap is None else int(gt_cap)
            bcap = max(64, 2 * hcap) if hyp_cap is None else int(hyp_cap)
            r = dict(sizes=i32(n, DT_IDENT_INTS), gt_tab=i32(n, max(acap, 0), 2), hyp_tab=i32(n, max(bcap, 0), 2),
                     align=t.empty((n, max(acap, 0), max(bcap, 0)), dtype=t.int64, device=self.device))
        r["any_label"] = bool(any_label)
        self._sync_stream()
        self._check(self.lib.dt_hota_align(self.h, _dptr(gt_boxes), _dptr(gt_counts), _dptr(gt_ids), gcap, _dptr(hyp_boxes), _dptr(hyp_counts),
                                           _dptr(hyp_ids), hcap, stride, label_at, n, T, flags, acap, bcap, _dptr(r["sizes"]),
                                           _dptr(r["gt_tab"]), _dptr(r["hyp_tab"]), _dptr(r["align"])), "dt_hota_align")
        return r

    def hota_weights(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, align):
        """Pass 2 of HOTA scoring (dt_hota_weights): the weights of every frame's match from a FINISHED hota_align result of the whole
        clip (labels are compared as that result's any_label says).
        -> dict: w [n,T,gcap,hcap] int32 (0 outside the frame's counts), dims [n,T,2] (the clamped row counts), gt_ent [n,T,gcap] and
        hyp_ent [n,T,hcap] (the row's trajectory, or -1).  assign_max on w viewed as [n*T,gcap,hcap] with dims gives the match."""
        t = self.torch
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        n, T, gcap, hcap, stride, label_at = self._hota_inputs(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids)
        acap, bcap = int(align["gt_tab"].shape[1]), int(align["hyp_tab"].shape[1])
        assert tuple(align["sizes"].shape) == (n, DT_IDENT_INTS) and tuple(align["align"].shape) == (n, acap, bcap)
        for k, dt in (("sizes", t.int32), ("gt_tab", t.int32), ("hyp_tab", t.int32), ("align", t.int64)):
            assert align[k].is_cuda and align[k].is_contiguous() and align[k].dtype == dt
        flags = DT_SCORE_ANY_LABEL if align["any_label"] else 0
        r = dict(w=i32(n, T, gcap, hcap), dims=i32(n, T, 2), gt_ent=i32(n, T, gcap), hyp_ent=i32(n, T, hcap))
        self._sync_stream()
        self._check(self.lib.dt_hota_weights(self.h, _dptr(gt_boxes), _dptr(gt_counts), _dptr(gt_ids), gcap, _dptr(hyp_boxes), _dptr(hyp_counts),
                                             _dptr(hyp_ids), hcap, stride, label_at, n, T, flags, acap, bcap, _dptr(align["sizes"]),
                                             _dptr(align["gt_tab"]), _dptr(align["hyp_tab"]), _dptr(align["align"]), _dptr(r["w"]),
                                             _dptr(r["dims"]), _dptr(r["gt_ent"]), _dptr(r["hyp_ent"])), "dt_hota_weights")
        return r

    def hota_count(self, gt_boxes, hyp_boxes, weights, row_to_col, thresholds, gt_cap, hyp_cap, state=None):
        """The matched pairs of every frame counted per IoU level (dt_hota_count): weights is a hota_weights result on these boxes,
        row_to_col [n*T,gcap] assign_max's match on it, thresholds 1..32 values in (0, 1], strictly ascending, gt_cap / hyp_cap the
        rows of the two trajectory tables.
        -> dict: tp [n,n_thr] int32, loc [n,n_thr] int64, pairs [n,n_thr,gt_cap,hyp_cap] int32 -- per BUCKET: a pair whose IoU reaches
        L >= 1 thresholds is counted in bucket L - 1 only (utility.evaluate.hota takes the suffix sums) -- and thresholds.
        state: a previous result (of the earlier chunks of these clips) that this call adds to (copied, not written)."""
        t = self.torch
        n, T, gcap, _ = gt_boxes.shape
        hcap = hyp_boxes.shape[2]
        acap, bcap = int(gt_cap), int(hyp_cap)
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        k = len(thr)
        assert tuple(hyp_boxes.shape) == (n, T, hcap, 8) and gt_boxes.shape[3] == DT_BOX_FLOATS
        assert tuple(weights["dims"].shape) == (n, T, 2) and tuple(weights["gt_ent"].shape) == (n, T, gcap)
        assert tuple(weights["hyp_ent"].shape) == (n, T, hcap) and tuple(row_to_col.shape) == (n * T, gcap)
        for x, dt in ((gt_boxes, t.float32), (hyp_boxes, t.float32), (weights["dims"], t.int32), (weights["gt_ent"], t.int32),
                      (weights["hyp_ent"], t.int32), (row_to_col, t.int32)):
            assert x.is_cuda and x.is_contiguous() and x.dtype == dt
        flags = 0
        if state is not None:
            assert np.array_equal(np.asarray(state["thresholds"], dtype=np.float32), thr), "thresholds differ from the state's"
            assert tuple(state["pairs"].shape) == (n, k, acap, bcap)
            r = {key: state[key].clone() for key in ("tp", "loc", "pairs")}
            flags = DT_SCORE_RESUME
        else:
            r = dict(tp=t.empty((n, k), dtype=t.int32, device=self.device), loc=t.empty((n, k), dtype=t.int64, device=self.device),
                     pairs=t.empty((n, k, max(acap, 0), max(bcap, 0)), dtype=t.int32, device=self.device))
        r["thresholds"] = thr.copy()
        self._sync_stream()
        self._check(self.lib.dt_hota_count(self.h, _dptr(gt_boxes), gcap, _dptr(hyp_boxes), hcap, n, T, _dptr(weights["dims"]),
                                           _dptr(weights["gt_ent"]), _dptr(weights["hyp_ent"]), _dptr(row_to_col),
                                           thr.ctypes.data_as(ctypes.c_void_p), k, acap, bcap, flags, _dptr(r["tp"]), _dptr(r["loc"]),
                                           _dptr(r["pairs"])), "dt_hota_count")
        return r

    def hota_score(self, gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, thresholds=None, any_label=False, gt_cap=None,
                   hyp_cap=None, align=None, state=None):
        """HOTA scoring (DESIGN.md "HOTA scoring"): hota_align on these inputs (align=None), or a finished hota_align result of the whole
        clip passed as `align` (any_label, gt_cap and hyp_cap are then that result's); then hota_weights, assign_max on every frame and
        hota_count.  thresholds: None = utility.evaluate.HOTA_THRESHOLDS (0.05 .. 0.95).
        -> dict: the alignment's sizes, gt_tab, hyp_tab and align; the count's tp, loc, pairs and thresholds; and the frames' w, dims,
        gt_ent, hyp_ent and row_to_col [n*T,gcap].  utility.evaluate.hota turns it into HOTA, DetA, AssA, LocA etc.
        state: the previous chunk's result, whose counts this call adds to.  A clip fed in chunks takes two loops over them: first
        hota_align(..., state=previous) over all chunks, then hota_score(..., align=the last alignment, state=previous) per chunk."""
        if thresholds is None:
            from utility.evaluate import HOTA_THRESHOLDS as thresholds
        if align is None:
            align = self.hota_align(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, any_label, gt_cap, hyp_cap)
        w = self.hota_weights(gt_boxes, gt_counts, gt_ids, hyp_boxes, hyp_counts, hyp_ids, align)
        n, T, gcap, hcap = w["w"].shape
        r2c, _, _ = self.assign_max(w["w"].view(n * T, gcap, hcap), w["dims"].view(n * T, 2))
        r = self.hota_count(gt_boxes, hyp_boxes, w, r2c, thresholds, align["gt_tab"].shape[1], align["hyp_tab"].shape[1], state)
        r.update(w, row_to_col=r2c, **{k: align[k] for k in ("sizes", "gt_tab", "hyp_tab", "align", "any_label")})
        return r

    def _detect_score_inputs(self, det_boxes, det_counts, gt_boxes, gt_counts, gt_flags):
        t = self.torch
        B, cap, _ = det_boxes.shape
        gcap = gt_boxes.shape[1]
        assert det_boxes.shape[2] == DT_BOX_FLOATS and tuple(gt_boxes.shape) == (B, gcap, DT_BOX_FLOATS)
        assert tuple(det_counts.shape) == (B,) and tuple(gt_counts.shape) == (B,)
        assert gt_flags is None or tuple(gt_flags.shape) == (B, gcap)
        for x, dt in ((det_boxes, t.float32), (gt_boxes, t.float32), (det_counts, t.int32), (gt_counts, t.int32), (gt_flags, t.int32)):
            assert x is None or (x.is_cuda and x.is_contiguous() and x.dtype == dt)
        return B, cap, gcap

    def detect_match(self, det_boxes, det_counts, gt_boxes, gt_counts, nb_class, thresholds=(0.5,), gt_flags=None, score_at=6):
        """The VOC match of detections against ground truth, per frame (dt_detect_match; the rule: DESIGN.md "Detection scoring").
        det_boxes [B,cap,8] / det_counts [B] as KerasYOLO.detect leaves them (the label in float 5, the ranking score in float
        score_at: 6 = score, 4 = conf); gt_boxes [B,gcap,8] (x, y, w, h, the label in float 5), gt_counts [B], gt_flags [B,gcap] int32
        with bit 0 = ignore, or None; thresholds: 1..16 IoU thresholds in (0, 1].
        -> dict of device tensors: state [n_thr,B,cap] int32 (1 TP, 0 FP, 2 ignored, -1 unused), best [B,cap] int32 (the ground-truth
        row of the largest IoU among those of the detection's label, -1 without one), iou [B,cap] float32; and thresholds, nb_class.
        Frames are matched independently: results of chunks of frames concatenate along B."""
        t = self.torch
        B, cap, gcap = self._detect_score_inputs(det_boxes, det_counts, gt_boxes, gt_counts, gt_flags)
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        r = dict(state=t.empty((len(thr), B, cap), dtype=t.int32, device=self.device),
                 best=t.empty((B, cap), dtype=t.int32, device=self.device), iou=self._f32(B, cap),
                 thresholds=thr.copy(), nb_class=int(nb_class))
        self._sync_stream()
        self._check(self.lib.dt_detect_match(self.h, _dptr(det_boxes), _dptr(det_counts), cap, int(score_at), _dptr(gt_boxes),
                                             _dptr(gt_counts), _dptr(gt_flags), gcap, B, int(nb_class),
                                             thr.ctypes.data_as(ctypes.c_void_p), len(thr), _dptr(r["state"]), _dptr(r["best"]),
                                             _dptr(r["iou"])), "dt_detect_match")
        return r

    def detect_rank(self, det_boxes, det_counts, state, gt_boxes, gt_counts, nb_class, gt_flags=None, score_at=6):
        """Every detection's position in its class's score order over all B frames (dt_detect_rank), from the `state` [n_thr,B,cap]
        of detect_match on the same inputs (chunks concatenated along B).
        -> dict of device tensors: rank, ctp [n_thr,B,cap] int32 (the position among the class's detections of state 0 / 1 by
        descending score, ties to the lower flat index, and the TPs up to it; -1 for ignored and unused rows), ngt [nb_class],
        ndet, ntp [n_thr,nb_class] int32.  utility.evaluate.average_precision turns them into AP."""
        t = self.torch
        B, cap, gcap = self._detect_score_inputs(det_boxes, det_counts, gt_boxes, gt_counts, gt_flags)
        n_thr, C = int(state.shape[0]), int(nb_class)
        assert tuple(state.shape) == (n_thr, B, cap) and state.is_cuda and state.is_contiguous() and state.dtype == t.int32
        i32 = lambda *shape: t.empty(shape, dtype=t.int32, device=self.device)
        r = dict(rank=i32(n_thr, B, cap), ctp=i32(n_thr, B, cap), ngt=i32(max(C, 0)), ndet=i32(n_thr, max(C, 0)), ntp=i32(n_thr, max(C, 0)))
        self._sync_stream()
        self._check(self.lib.dt_detect_rank(self.h, _dptr(det_boxes), _dptr(det_counts), cap, int(score_at), _dptr(state), _dptr(gt_boxes),
                                            _dptr(gt_counts), _dptr(gt_flags), gcap, B, C, n_thr, _dptr(r["rank"]), _dptr(r["ctp"]),
                                            _dptr(r["ngt"]), _dptr(r["ndet"]), _dptr(r["ntp"])), "dt_detect_rank")
        return r

    def detect_score(self, det_boxes, det_counts, gt_boxes, gt_counts, nb_class, thresholds=(0.5,), gt_flags=None, score_at=6):
        """detect_match, then detect_rank on its states: the union of both dicts, plus `scores` and `labels` [B,cap] (floats score_at
        and 5 of det_boxes, as views) -- what utility.evaluate.average_precision / precision_recall take."""
        r = self.detect_match(det_boxes, det_counts, gt_boxes, gt_counts, nb_class, thresholds, gt_flags, score_at)
        r.update(self.detect_rank(det_boxes, det_counts, r["state"], gt_boxes, gt_counts, nb_class, gt_flags, score_at))
        r["scores"], r["labels"] = det_boxes[:, :, int(score_at)], det_boxes[:, :, 5]
        return r

    def pack_detections(self, boxes, counts, ids, nids, n_rows):
        """this rank's detection table -> int32 rows [n_rows, dt_packed_row_ints(T, cap)] (rows past the local clips
        are empty): the buffer of the ONE all-gather of a step."""
        t = self.torch
        n, T, cap = ids.shape
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and ids.is_contiguous() and nids.is_contiguous()
        assert counts.dtype == t.int32 and ids.dtype == t.int32 and nids.dtype == t.int32 and boxes.dtype == t.float32
        assert n <= n_rows, "this rank holds %d clips but the exchange was sized for at most %d per rank (n_clips_max)" % (n, n_rows)
        rows = t.empty((n_rows, int(self.lib.dt_packed_row_ints(T, cap))), dtype=t.int32, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_pack_detections(self.h, _dptr(boxes), _dptr(counts), _dptr(ids), _dptr(nids), n, T, cap,
                                                n_rows, _dptr(rows)), "dt_pack_detections")
        return rows

    def unpack_detections(self, rows, T, cap):
        """gathered rows of all ranks [R, row] -> (boxes, counts, ids, nids, gids) of the valid clips in global order"""
        t = self.torch
        assert rows.is_cuda and rows.is_contiguous() and rows.dtype == t.int32
        R = rows.shape[0]
        assert rows.shape[1] == int(self.lib.dt_packed_row_ints(T, cap))
        boxes = t.empty((R, T, cap, DT_BOX_FLOATS), dtype=t.float32, device=self.device)
        counts = t.empty((R, T), dtype=t.int32, device=self.device)
        ids = t.empty((R, T, cap), dtype=t.int32, device=self.device)
        nids = t.empty((R,), dtype=t.int32, device=self.device)
        gids = t.empty((R, T, cap), dtype=t.int64, device=self.device)
        nv = t.zeros((1,), dtype=t.int32, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_unpack_detections(self.h, _dptr(rows), R, T, cap, _dptr(boxes), _dptr(counts), _dptr(ids),
                                                  _dptr(nids), _dptr(gids), _dptr(nv)), "dt_unpack_detections")
        n = int(nv.item())
        return boxes[:n], counts[:n], ids[:n], nids[:n], gids[:n]

    # ---- tracker ------------------------------------------------------
    def tracker_load(self, units, kernel, recurrent, bias, out_kernel, out_bias):
        ks = [_hptr(a) for a in (kernel, recurrent, bias, out_kernel, out_bias)]
        self._check(self.lib.dt_tracker_load(self.h, units, *[k[1] for k in ks]), "dt_tracker_load")
        self.trk_units = units

    def track_forward(self, frames, want_det=True):
        """frames [n_clips,T,H,W,3] -> tracking grid [n_clips,T,G,G,NB,5+C] (+ detection grid)."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 5
        n_clips, T = frames.shape[:2]
        gh, gw = self.grid
        trk = self._f32(n_clips, T, gh, gw, self.nb_box, 5 + self.nb_class)
        det = self._f32(n_clips, T, gh, gw, self.nb_box, 5 + self.nb_class) if want_det else None
        self._sync_stream()
        self._check(self.lib.dt_track_forward(self.h, _dptr(frames), self._frames_dtype(frames), n_clips, T,
                                              _dptr(trk), _dptr(det)), "dt_track_forward")
        return (trk, det) if want_det else trk

    # ---- streaming: state carried across calls ---------------------------
    @staticmethod
    def _slot_array(slots):
        """host list of slot numbers -> (n, ctypes int array)"""
        slots = [int(v) for v in slots]
        return len(slots), (ctypes.c_int * max(1, len(slots)))(*slots)

    def stream_open(self, n_slots, cap, track_cap=None):
        """(re)allocate the stream slots, every one fresh; cap = box capacity of the association state, track_cap (None: cap) = entries
        of a slot's track table (associate_stream with max_age > 0)"""
        self._sync_stream()
        if track_cap is None:
            self._check(self.lib.dt_stream_open(self.h, int(n_slots), int(cap)), "dt_stream_open")
        else:
            self._check(self.lib.dt_stream_open_tracks(self.h, int(n_slots), int(cap), int(track_cap)), "dt_stream_open_tracks")
        self._stream_tcap = int(cap if track_cap is None else track_cap)      # rows per frame of associate_stream_tracks' read-out

    def stream_reset(self, slots=None):
        """the listed slots (None: all) fresh again: zero ConvLSTM state, track ids from 0"""
        self._sync_stream()
        if slots is None:
            self._check(self.lib.dt_stream_reset(self.h, None, 0), "dt_stream_reset")
        else:
            n, arr = self._slot_array(slots)
            self._check(self.lib.dt_stream_reset(self.h, arr, n), "dt_stream_reset")

    def track_stream_forward(self, frames, slots, want_det=False):
        """track_forward on frames [n,T,H,W,3] whose stream i continues from -- and leaves its ConvLSTM state in -- slot slots[i]."""
        if frames is None:
            raise NativeError("dt_track_stream_forward failed (1): null frames")
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 5
        n, T = frames.shape[:2]
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_track_stream_forward failed (1): %d slots for %d streams" % (ns, n))
        gh, gw = self.grid
        trk = self._f32(n, T, gh, gw, self.nb_box, 5 + self.nb_class)
        det = self._f32(n, T, gh, gw, self.nb_box, 5 + self.nb_class) if want_det else None
        self._sync_stream()
        self._check(self.lib.dt_track_stream_forward(self.h, _dptr(frames), self._frames_dtype(frames), n, T, arr,
                                                     _dptr(trk), _dptr(det)), "dt_track_stream_forward")
        return (trk, det) if want_det else trk

    def associate_stream(self, boxes, counts, assoc_threshold, slots, max_age=0, want_gaps=False, motion_gain=None):
        """associate on boxes [n,T,cap,8], counts [n,T]: frame 0 of stream i is matched against the last frame slot slots[i] saw,
        ids continue across calls, nids [n] = ids opened by the stream since its reset.
        max_age > 0 or want_gaps: the track-memory rule (dt_associate_stream_mem) against the slot's track table; with want_gaps the
        result is (ids, nids, gaps [n,T,cap]).
        motion_gain (a number in [0, 1]; None: none of it): the track-motion rule (dt_associate_stream_motion); a call without it makes
        the slot's tracks forget their velocities."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n, T, cap, _ = boxes.shape
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_associate_stream failed (1): %d slots for %d streams" % (ns, n))
        ids = t.empty((n, T, cap), dtype=t.int32, device=self.device)
        nids = t.empty((n,), dtype=t.int32, device=self.device)
        self._sync_stream()
        if motion_gain is not None:
            gaps = t.empty((n, T, cap), dtype=t.int32, device=self.device) if want_gaps else None
            self._check(self.lib.dt_associate_stream_motion(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold),
                                                            int(max_age), float(motion_gain), arr, _dptr(ids), _dptr(nids), _dptr(gaps)),
                        "dt_associate_stream_motion")
            return (ids, nids, gaps) if want_gaps else (ids, nids)
        if max_age != 0 or want_gaps:
            gaps = t.empty((n, T, cap), dtype=t.int32, device=self.device) if want_gaps else None
            self._check(self.lib.dt_associate_stream_mem(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold),
                                                         int(max_age), arr, _dptr(ids), _dptr(nids), _dptr(gaps)), "dt_associate_stream_mem")
            return (ids, nids, gaps) if want_gaps else (ids, nids)
        self._check(self.lib.dt_associate_stream(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold),
                                                 arr, _dptr(ids), _dptr(nids)), "dt_associate_stream")
        return ids, nids

    def associate_stream_tracks(self, boxes, counts, assoc_threshold, slots, max_age, gain, min_hits, match=0, readout=True, assign=False):
        """associate_tracks for streams (dt_associate_stream_tracks): the slot's track table carries velocities and hit counts across
        calls; the read-out has the table's track_cap rows per frame.  The dict of associate_tracks.  After a call of associate_stream
        with a motion_gain the slot's tracks read as hits = 1; after one without, their velocities are forgotten too.
        match: the track match policy of this call (dt_associate_stream_tracks_match); it leaves nothing in the slot.
        readout=False: no tracks / track_info / track_counts.
        assign=True: the optimal assignment as the match of this call (dt_associate_stream_tracks_assign); match 0 or DT_MATCH_ANY_LABEL."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n, T, cap, _ = boxes.shape
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_associate_stream_tracks failed (1): %d slots for %d streams" % (ns, n))
        r = self._tracks_outputs(n, T, cap, getattr(self, "_stream_tcap", None) or cap, readout)
        self._sync_stream()
        if assign:
            self._check(self.lib.dt_associate_stream_tracks_assign(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold),
                                                                   int(max_age), float(gain), int(min_hits), int(match), arr, _dptr(r["ids"]),
                                                                   _dptr(r["nids"]), _dptr(r["gaps"]), _dptr(r["hits"]), _dptr(r.get("tracks")),
                                                                   _dptr(r.get("track_info")), _dptr(r.get("track_counts"))),
                        "dt_associate_stream_tracks_assign")
            return r
        if match != 0:
            self._check(self.lib.dt_associate_stream_tracks_match(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold),
                                                                  int(max_age), float(gain), int(min_hits), int(match), arr, _dptr(r["ids"]),
                                                                  _dptr(r["nids"]), _dptr(r["gaps"]), _dptr(r["hits"]), _dptr(r.get("tracks")),
                                                                  _dptr(r.get("track_info")), _dptr(r.get("track_counts"))),
                        "dt_associate_stream_tracks_match")
            return r
        self._check(self.lib.dt_associate_stream_tracks(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold), int(max_age),
                                                        float(gain), int(min_hits), arr, _dptr(r["ids"]), _dptr(r["nids"]), _dptr(r["gaps"]),
                                                        _dptr(r["hits"]), _dptr(r.get("tracks")), _dptr(r.get("track_info")),
                                                        _dptr(r.get("track_counts"))), "dt_associate_stream_tracks")
        return r

    def associate_stream_tracks_scored(self, boxes, counts, assoc_threshold, slots, max_age, gain, min_hits, score_high, score_new=None,
                                       assoc_threshold_low=None, max_age_low=0, score_at=6, match=0, readout=True):
        """associate_tracks_scored for streams (dt_associate_stream_tracks_scored): associate_stream_tracks(..., assign=True) with the two
        passes by score.  The slot may be shared with every other association entry: the rows a call leaves for its last frame's dropped
        boxes are matched by none of them."""
        t = self.torch
        assert boxes.is_cuda and boxes.is_contiguous() and counts.is_contiguous() and counts.dtype == t.int32
        n, T, cap, _ = boxes.shape
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_associate_stream_tracks_scored failed (1): %d slots for %d streams" % (ns, n))
        r = self._tracks_outputs(n, T, cap, getattr(self, "_stream_tcap", None) or cap, readout)
        self._sync_stream()
        self._check(self.lib.dt_associate_stream_tracks_scored(self.h, _dptr(boxes), _dptr(counts), n, T, cap, float(assoc_threshold), int(max_age),
                                                               float(gain), int(min_hits), int(match), int(score_at), float(score_high),
                                                               float(score_high if score_new is None else score_new),
                                                               float(assoc_threshold if assoc_threshold_low is None else assoc_threshold_low),
                                                               int(max_age_low), arr, _dptr(r["ids"]), _dptr(r["nids"]), _dptr(r["gaps"]),
                                                               _dptr(r["hits"]), _dptr(r.get("tracks")),
                                                               _dptr(r.get("track_info")), _dptr(r.get("track_counts"))),
                    "dt_associate_stream_tracks_scored")
        return r

    def track_row_width(self):
        return int(self.lib.dt_track_row_width(self.h))

    def track_detect(self, frames):
        """frames [F,H,W,3] -> z rows [F,G,G,row_width] = [conv_feat | x_bbox | pad] (frame-shard half 1)."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        F = frames.shape[0]
        gh, gw = self.grid
        z = self._f32(F, gh, gw, self.lib.dt_track_row_width(self.h))
        self._sync_stream()
        self._check(self.lib.dt_track_detect(self.h, _dptr(frames), self._frames_dtype(frames), F, _dptr(z)), "dt_track_detect")
        return z

    def track_recurrent(self, z, want_det=False):
        """z [n_clips,T,G,G,row_width] -> tracking grid [n_clips,T,G,G,NB,5+C] (frame-shard half 2)."""
        assert z.is_cuda and z.is_contiguous() and z.dim() == 5 and z.dtype == self.torch.float32
        n_clips, T = z.shape[:2]
        gh, gw = self.grid
        trk = self._f32(n_clips, T, gh, gw, self.nb_box, 5 + self.nb_class)
        det = self._f32(n_clips, T, gh, gw, self.nb_box, 5 + self.nb_class) if want_det else None
        self._sync_stream()
        self._check(self.lib.dt_track_recurrent(self.h, _dptr(z), n_clips, T, _dptr(trk), _dptr(det)), "dt_track_recurrent")
        return (trk, det) if want_det else trk

    def track_xproj_width(self):
        return int(self.lib.dt_track_xproj_width(self.h))

    def track_detect_xproj(self, frames):
        """frames [F,H,W,3] -> ConvLSTM input-projection rows [F,G,G,4U] (frame-shard half 1, projection included)."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        F = frames.shape[0]
        gh, gw = self.grid
        xp = self._f32(F, gh, gw, self.track_xproj_width())
        self._sync_stream()
        self._check(self.lib.dt_track_detect_xproj(self.h, _dptr(frames), self._frames_dtype(frames), F, _dptr(xp), None),
                    "dt_track_detect_xproj")
        return xp

    def track_recurrent_xproj(self, xp):
        """xp [n_clips,T,G,G,4U] -> tracking grid [n_clips,T,G,G,NB,5+C] (frame-shard half 2: the recurrence alone)."""
        assert xp.is_cuda and xp.is_contiguous() and xp.dim() == 5 and xp.dtype == self.torch.float32
        n_clips, T = xp.shape[:2]
        gh, gw = self.grid
        trk = self._f32(n_clips, T, gh, gw, self.nb_box, 5 + self.nb_class)
        self._sync_stream()
        self._check(self.lib.dt_track_recurrent_xproj(self.h, _dptr(xp), n_clips, T, _dptr(trk)), "dt_track_recurrent_xproj")
        return trk

    # ---- tiny tracker ---------------------------------------------------
    def tiny_load(self, D, units, kernel, recurrent, bias, dense_kernel, dense_bias):
        ks = [_hptr(a) for a in (kernel, recurrent, bias, dense_kernel, dense_bias)]
        self.tiny_out = int(np.asarray(dense_kernel).shape[1])
        self.tiny_D = int(D)
        self._check(self.lib.dt_tiny_load(self.h, D, units, self.tiny_out, *[k[1] for k in ks]), "dt_tiny_load")

    def heatmap_from_boxes(self, box4, hmap_size):
        """box4 [n,4] centre-format -> [n, hs*hs] 0/1 heatmaps (utils.generate_heatmap_feat)."""
        n = box4.shape[0]
        out = self._f32(n, hmap_size * hmap_size)
        self._sync_stream()
        self._check(self.lib.dt_heatmap_from_boxes(self.h, _dptr(box4), n, hmap_size, _dptr(out)), "dt_heatmap_from_boxes")
        return out

    def heatmap_from_xywh64(self, xywh, hmap_size):
        """xywh [n,4] float64 (det_x, det_y, det_w, det_h) exactly as utils.generate_heatmap_feat takes them."""
        assert xywh.dtype == self.torch.float64 and xywh.is_cuda and xywh.is_contiguous()
        n = xywh.shape[0]
        out = self._f32(n, hmap_size * hmap_size)
        self._sync_stream()
        self._check(self.lib.dt_heatmap_from_xywh64(self.h, _dptr(xywh), n, hmap_size, _dptr(out)), "dt_heatmap_from_xywh64")
        return out

    def encode_targets(self, objs, counts, dims, aug, grid_h, grid_w, nb_box, nb_class, image_h, image_w,
                       true_box_buffer, anchors):
        """objs int32 [n,cap,5], counts int32 [n], dims int32 [n,2], aug float64 [n,4] or None ->
        (y float64 [n,GH,GW,NB,5+C], b float64 [n,TBB,4])  (preprocessing.py:171-188, 214-293)."""
        t = self.torch
        assert objs.dtype == t.int32 and counts.dtype == t.int32 and dims.dtype == t.int32
        assert objs.is_cuda and objs.is_contiguous() and counts.is_contiguous() and dims.is_contiguous()
        n, cap = objs.shape[0], objs.shape[1]
        if aug is not None:
            assert aug.dtype == t.float64 and aug.is_cuda and aug.is_contiguous() and aug.shape == (n, 4)
        an = np.ascontiguousarray(anchors, dtype=np.float64)
        assert an.size == 2 * nb_box
        y = t.empty((n, grid_h, grid_w, nb_box, 5 + nb_class), dtype=t.float64, device=self.device)
        b = t.empty((n, true_box_buffer, 4), dtype=t.float64, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_encode_targets(self.h, _dptr(objs), _dptr(counts), _dptr(dims),
                                               _dptr(aug) if aug is not None else None, n, cap, grid_h, grid_w,
                                               nb_box, nb_class, image_h, image_w, true_box_buffer,
                                               an.ctypes.data_as(ctypes.c_void_p), _dptr(y), _dptr(b)),
                    "dt_encode_targets")
        return y, b

    def rect_from_heatmap(self, heat, hmap_size, thresh=0.75):
        """heat [n, hs*hs] -> int32 [n,4] (x1,y1,x2,y2) (utils.generate_rectangle_from_heatmap)."""
        t = self.torch
        n = heat.shape[0]
        out = t.empty((n, 4), dtype=t.int32, device=self.device)
        self._sync_stream()
        self._check(self.lib.dt_rect_from_heatmap(self.h, _dptr(heat), n, hmap_size, float(thresh), _dptr(out)),
                    "dt_rect_from_heatmap")
        return out

    def tiny_forward(self, feat, det, pool="Global"):
        """feat [n_seq,T,fh,fw,fc], det [n_seq,T,4] -> [n_seq,T,4]."""
        t = self.torch
        assert feat.is_cuda and feat.is_contiguous() and feat.dtype == t.float32
        assert det.is_cuda and det.is_contiguous() and det.dtype == t.float32
        n_seq, T, fh, fw, fc = feat.shape
        out = self._f32(n_seq, T, self.tiny_out)
        self._sync_stream()
        self._check(self.lib.dt_tiny_forward(self.h, _dptr(feat), _dptr(det), n_seq, T, fh, fw, fc,
                                             0 if pool == "Global" else 1, _dptr(out)), "dt_tiny_forward")
        return out

    def tiny_features(self, feat, det, D, pool="Global"):
        """feat [n,fh,fw,fc], det [n,4] -> rows [n,D] (pooled feature (+) det box)."""
        n, fh, fw, fc = feat.shape
        x = self._f32(n, D)
        self._sync_stream()
        self._check(self.lib.dt_tiny_features(self.h, _dptr(feat), _dptr(det), n, fh, fw, fc,
                                              0 if pool == "Global" else 1, _dptr(x)), "dt_tiny_features")
        return x

    def tiny_sequence(self, x):
        """x [n_seq,T,D] -> [n_seq,T,4]."""
        assert x.is_cuda and x.is_contiguous()
        n_seq, T, _ = x.shape
        out = self._f32(n_seq, T, self.tiny_out)
        self._sync_stream()
        self._check(self.lib.dt_tiny_sequence(self.h, _dptr(x), n_seq, T, _dptr(out)), "dt_tiny_sequence")
        return out

    # ---- tiny tracker streams: the LSTM state carried across calls -------
    def tiny_stream_open(self, n_slots):
        """(re)allocate the tiny trackers' stream slots (h, c [units] per slot), every one fresh; apart from stream_open's table"""
        self._sync_stream()
        self._check(self.lib.dt_tiny_stream_open(self.h, int(n_slots)), "dt_tiny_stream_open")

    def tiny_stream_reset(self, slots=None):
        """the listed slots (None: all) fresh again: the next call on them starts from h = c = 0"""
        self._sync_stream()
        if slots is None:
            self._check(self.lib.dt_tiny_stream_reset(self.h, None, 0), "dt_tiny_stream_reset")
        else:
            n, arr = self._slot_array(slots)
            self._check(self.lib.dt_tiny_stream_reset(self.h, arr, n), "dt_tiny_stream_reset")

    def tiny_stream_sequence(self, x, slots):
        """tiny_sequence on x [n,T,D] whose sequence i continues from -- and leaves its LSTM state in -- slot slots[i]."""
        assert x.is_cuda and x.is_contiguous()
        n, T, _ = x.shape
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_tiny_stream_sequence failed (1): %d slots for %d streams" % (ns, n))
        out = self._f32(n, T, self.tiny_out)
        self._sync_stream()
        self._check(self.lib.dt_tiny_stream_sequence(self.h, _dptr(x), n, T, arr, _dptr(out)), "dt_tiny_stream_sequence")
        return out

    def tiny_stream_forward(self, feat, det, slots, pool="Global"):
        """tiny_forward on feat [n,T,fh,fw,fc], det [n,T,4 or hs*hs] whose sequence i continues in slot slots[i]."""
        t = self.torch
        assert feat.is_cuda and feat.is_contiguous() and feat.dtype == t.float32
        assert det.is_cuda and det.is_contiguous() and det.dtype == t.float32
        n, T, fh, fw, fc = feat.shape
        ns, arr = self._slot_array(slots)
        if ns != n:
            raise NativeError("dt_tiny_stream_forward failed (1): %d slots for %d streams" % (ns, n))
        out = self._f32(n, T, self.tiny_out)
        self._sync_stream()
        self._check(self.lib.dt_tiny_stream_forward(self.h, _dptr(feat), _dptr(det), n, T, fh, fw, fc,
                                                    0 if pool == "Global" else 1, arr, _dptr(out)), "dt_tiny_stream_forward")
        return out

    def top_box(self, boxes, counts):
        """boxes [F,cap,8], counts [F] -> [F,4] highest-score box per frame (zeros if none)."""
        F, cap, _ = boxes.shape
        out = self._f32(F, 4)
        self._sync_stream()
        self._check(self.lib.dt_top_box(self.h, _dptr(boxes), _dptr(counts), F, cap, _dptr(out)), "dt_top_box")
        return out

    # ---- layer-level (parity tests) -----------------------------------
    def conv2d(self, x, kernel_hwio, bias=None, leaky_slope=1.0, pool=0):
        t = self.torch
        assert x.is_cuda and x.is_contiguous() and x.dtype == t.float32
        B, H, W, Cin = x.shape
        k, _, ci, Cout = kernel_hwio.shape
        assert ci == Cin
        kk, kp = _hptr(kernel_hwio)
        bb, bp = _hptr(bias) if bias is not None else (None, None)
        if pool == 0:
            out, out2 = self._f32(B, H, W, Cout), None
        elif pool == 1:
            out, out2 = self._f32(B, H // 2, W // 2, Cout), None
        elif pool == 2:
            out, out2 = self._f32(B, H, W, Cout), self._f32(B, H // 2, W // 2, Cout)
        else:
            out, out2 = self._f32(B, H // 2, W // 2, 4 * Cout), None
        self._sync_stream()
        self._check(self.lib.dt_conv2d(self.h, _dptr(x), B, H, W, Cin, kp, k, Cout, bp, float(leaky_slope), pool,
                                       _dptr(out), _dptr(out2)), "dt_conv2d")
        return (out, out2) if pool == 2 else out

    def convlstm_step(self, x, h, c, kernel, recurrent, bias):
        t = self.torch
        B, H, W, Cx = x.shape
        U = h.shape[-1]
        ho, co = t.empty_like(h), t.empty_like(c)
        ks = [_hptr(a) for a in (kernel, recurrent, bias)]
        self._sync_stream()
        self._check(self.lib.dt_convlstm_step(self.h, _dptr(x), B, H, W, Cx, _dptr(h), _dptr(c), U,
                                              ks[0][1], ks[1][1], ks[2][1], _dptr(ho), _dptr(co)), "dt_convlstm_step")
        return ho, co

    def gemm_split_bf16(self, v, u, half=0, nt=3):
        """v [P,Mt,K], u [P,N,K] float32 -> [P,Mt,N] through wino_gemm_s3.hip: the Winograd-domain contraction at a caller-chosen
        shape.  nt=3: three-term bf16 split of both operands on the device, six MFMA partial products per multiply; nt=2: the
        fp16 form (two terms of the scaled operands, three products)."""
        t = self.torch
        assert v.is_cuda and u.is_cuda and v.is_contiguous() and u.is_contiguous() and v.dtype == t.float32 and u.dtype == t.float32
        P, Mt, K = v.shape
        assert u.shape[0] == P and u.shape[2] == K
        N = u.shape[1]
        out = self._f32(P, Mt, N)
        self._sync_stream()
        self._check(self.lib.dt_gemm_split(self.h, _dptr(v), _dptr(u), P, Mt, K, N, int(half), int(nt), _dptr(out)), "dt_gemm_split")
        return out

    def gemm_split(self, v, u, half=0, nt=2):
        return self.gemm_split_bf16(v, u, half=half, nt=nt)

    # ---- the Winograd transforms alone (csrc/winograd.hip) -------------
    @staticmethod
    def _wino_geom(g):
        return dict(zip(WINO_GEOM_KEYS, [int(v) for v in g]))

    def _nhwc_view(self, t, what):
        """[B,H,W,C] float32 device view with dense channels, rows and frames of pixels `ld` floats apart -> (ld, frame stride)"""
        assert t.is_cuda and t.dtype == self.torch.float32 and t.dim() == 4 and t.stride(3) == 1 and t.stride(1) == t.shape[2] * t.stride(2), what
        return t.stride(2), t.stride(0)

    def wino_geometry(self, ts, B, H, W, pooled=False):
        """the tile geometry the library gives a Winograd launch (dt_wino_geometry): g, ph, pw, th, tw, Mt, Mp"""
        g = (ctypes.c_int * DT_WINO_GEOM_INTS)()
        self._check(self.lib.dt_wino_geometry(self.h, int(ts), int(B), int(H), int(W), int(bool(pooled)), g), "dt_wino_geometry")
        return {k: v for k, v in self._wino_geom(g).items() if k not in ("form", "grid", "threads")}

    def wino_input(self, x, v, ts, nt=0, pooled=False, force_form=0, wg_cap=0):
        """Bt d B of the view x [B,H,W,C] (pixel stride >= C, any frame stride) into the caller's buffer v (dt_wino_input): nt=0 float32
        [P,Mt,C], nt=3 / 2 the split layouts in 16-bit words.  Returns the geometry with the kernel form, grid and workgroup size taken."""
        ld, bs = self._nhwc_view(x, "x")
        assert v.is_cuda and v.is_contiguous()
        B, H, W, C = x.shape
        g = (ctypes.c_int * DT_WINO_GEOM_INTS)()
        self._sync_stream()
        self._check(self.lib.dt_wino_input(self.h, _dptr(x), B, H, W, C, ld, bs, int(ts), int(bool(pooled)), int(nt), int(force_form), int(wg_cap),
                                           _dptr(v), v.numel() * v.element_size(), g), "dt_wino_input")
        return self._wino_geom(g)

    def wino_output(self, m, N, B, H, W, ts, bias=None, bias16=None, slope=1.0, out=None, out2=None, publish=False, xproj=None, cstate=None,
                    force_form=0, wg_cap=0):
        """At m A of m [P,Mt,m_ld] (dt_wino_output) into the caller's views out [B,H,W,N] and / or out2 [B,H//2,W//2,N] (pixel stride >= N), or,
        with cstate, the ConvLSTM gate update: xproj [B,H,W,N] read, cstate [B,H,W,N//4] updated in place, h to out [B,H,W,N//4].  publish:
        max |x| of what was stored goes to max-|x| slot 57 (amax_read).  Returns the geometry with the kernel form, grid and workgroup size."""
        t = self.torch
        assert m.is_cuda and m.is_contiguous() and m.dtype == t.float32 and m.dim() == 3
        lds = {}
        for name, a, shape in (("out", out, (B, H, W)), ("out2", out2, (B, H // 2, W // 2)), ("xproj", xproj, (B, H, W)), ("cstate", cstate, (B, H, W))):
            lds[name] = 0
            if a is not None:
                assert tuple(a.shape[:3]) == shape, name
                lds[name], bs = self._nhwc_view(a, name)
                assert bs == shape[1] * shape[2] * lds[name], name + ": frames follow each other"
        for a in (bias, bias16):
            assert a is None or (a.is_cuda and a.is_contiguous() and a.dtype == t.float32)
        g = (ctypes.c_int * DT_WINO_GEOM_INTS)()
        self._sync_stream()
        self._check(self.lib.dt_wino_output(self.h, _dptr(m), m.numel(), m.shape[2], int(N), int(B), int(H), int(W), int(ts), _dptr(bias), _dptr(bias16),
                                            float(slope), _dptr(out), lds["out"], _dptr(out2), lds["out2"], int(bool(publish)), _dptr(xproj), lds["xproj"],
                                            _dptr(cstate), lds["cstate"], int(force_form), int(wg_cap), g), "dt_wino_output")
        return self._wino_geom(g)

    # ---- the fp32 implicit-GEMM kernel alone (csrc/conv_igemm.hip) -----
    def conv_igemm(self, x, out, ks, kernel=None, bias=None, wt=None, kind="plain", cfg="128x128", slope=1.0, act=0, ksplit=0, npad=0, out2=None,
                   xproj=None, cstate=None, publish=False, wg_cap=0):
        """conv_igemm.hip through its production launcher on caller views (dt_conv_igemm).  Layer mode: x [B,H,W,Cin] (pixel stride >= Cin,
        any frame stride), kernel numpy HWIO [ks,ks,Cin,N], bias numpy [N] or None.  Batched GEMM: x [P,Mt,K] and wt [P,N,K] dense device
        tensors.  out / out2 / xproj / cstate are 2-D row views [rows, columns] with unit column stride; their row stride is the ld ([P,Mt,N]
        with dense problems for the batched GEMM).  Returns what ran: cfg, BM, BN, threads, persistent, grid_x, grid_y, total."""
        t = self.torch
        d = ConvIgemmDesc()
        if wt is not None:
            assert x.is_cuda and x.is_contiguous() and wt.is_cuda and wt.is_contiguous() and x.dim() == 3 and wt.dim() == 3 and x.dtype == wt.dtype == t.float32
            assert out.dim() == 3 and out.stride(2) == 1 and out.stride(0) == out.shape[1] * out.stride(1)
            d.P, (d.B, d.H, d.W), d.Cin, d.N = x.shape[0], (1, 1, x.shape[1]), x.shape[2], wt.shape[1]
            d.in_ld, d.in_bs, d.out_ld = d.Cin, d.W * d.Cin, out.stride(1)
        else:
            d.in_ld, d.in_bs = self._nhwc_view(x, "x")
            d.P, (d.B, d.H, d.W, d.Cin), d.N = 1, x.shape, kernel.shape[3]
            assert out.dim() == 2 and out.stride(1) == 1
            d.out_ld = out.stride(0)
        for name, a in (("out2_ld", out2), ("xp_ld", xproj), ("c_ld", cstate)):
            if a is not None:
                assert a.is_cuda and a.dtype == t.float32 and a.dim() == 2 and a.stride(1) == 1, name
                setattr(d, name, a.stride(0))
        d.ks, d.npad, d.kind, d.cfg = int(ks), int(npad), CONV_KINDS.get(kind, kind), CONV_CFGS.get(cfg, cfg)
        d.ksplit, d.act, d.publish, d.wg_cap, d.slope = int(ksplit), int(act), int(bool(publish)), int(wg_cap), float(slope)
        kk, kp = _hptr(kernel) if kernel is not None else (None, None)
        bb, bp = _hptr(bias) if bias is not None else (None, None)
        info = (ctypes.c_int * DT_CONV_INFO_INTS)()
        self._sync_stream()
        self._check(self.lib.dt_conv_igemm(self.h, ctypes.byref(d), _dptr(x), kp, bp, _dptr(wt), _dptr(out), _dptr(out2), _dptr(xproj), _dptr(cstate), info),
                    "dt_conv_igemm")
        return dict(zip(CONV_INFO_KEYS, [int(v) for v in info]))

    # ---- conv_1's direct kernels alone (csrc/conv1.hip) ------------------
    def conv1(self, frames, w, bias, out, slope=0.1, split=True, tpw=0, publish=False, batch=None):
        """conv1.hip through its production launcher (dt_conv1), no detector configured.  frames [B,H,W,3] uint8 (a contiguous view at ANY byte
        offset of its buffer) or float32; w numpy [27,32] (row 9 ky + 3 kx + ci, scale folded), bias numpy [32]; out a contiguous float32
        [B,H/2,W/2,32] view.  split: pass the three-term tables (False: the fp32 MFMA kernel); tpw: 0 = the launcher's rule;
        batch: the B to pass instead of frames.shape[0] (a refusal test's 0).  Returns the launcher's plan: instance (CONV1_INSTANCES), tpw, grid_x,
        grid_y, grid_z, fills_amax."""
        t = self.torch
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 4 and frames.shape[3] == 3
        B, H, W, _ = frames.shape
        assert out.is_cuda and out.is_contiguous() and out.dtype == t.float32 and out.numel() == B * (H // 2) * (W // 2) * 32
        if batch is not None:
            B = batch
        w = np.ascontiguousarray(w, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        assert w.shape == (27, 32) and bias.shape == (32,)
        info = (ctypes.c_int * DT_CONV1_INFO_INTS)()
        self._sync_stream()
        self._check(self.lib.dt_conv1(self.h, _dptr(frames), self._frames_dtype(frames), int(B), int(H), int(W), w.ctypes.data_as(ctypes.c_void_p),
                                      bias.ctypes.data_as(ctypes.c_void_p), float(slope), int(bool(split)), int(tpw), int(bool(publish)), _dptr(out), info),
                    "dt_conv1")
        return dict(zip(CONV1_INFO_KEYS, [int(v) for v in info]))

    # ---- profiling ------------------------------------------------------
    def profile_enable(self, on=True):
        self._sync_stream()
        self._check(self.lib.dt_profile_enable(self.h, 1 if on else 0), "dt_profile_enable")

    def profile_reset(self):
        self._check(self.lib.dt_profile_reset(self.h), "dt_profile_reset")

    def profile_names(self):
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.dt_profile_names(self.h, buf, len(buf)), "dt_profile_names")
        return [n for n in buf.value.decode().split("\n") if n]

    def reload_policy(self):
        """re-read the DT_* tuning / test knobs from the environment (read in dt_create; a pin override stays)"""
        self._check(self.lib.dt_policy_reload(self.h), "dt_policy_reload")

    def policy_set(self, name, value):
        """one knob of THIS context without the process environment (dt_policy_set): "pin" 1 / 0, or -1 to follow DT_PIN"""
        self._check(self.lib.dt_policy_set(self.h, name.encode(), int(value)), "dt_policy_set")
        if name == "pin":
            self.pin = int(value)

    def graph_enable(self, on=True):
        """hipGraph replay of the detector trunk and the ConvLSTM recurrence (low-latency serving)."""
        self._check(self.lib.dt_graph_enable(self.h, 1 if on else 0), "dt_graph_enable")

    def profile_read(self, name):
        n = ctypes.c_int64(0)
        ms, fl, by = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self.lib.dt_profile_read(self.h, name.encode(), ctypes.byref(n), ctypes.byref(ms),
                                             ctypes.byref(fl), ctypes.byref(by)), "dt_profile_read")
        return dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)

    def amax_read(self, slot):
        """max |x| held in max-|x| slot `slot` (include/mi355_dt.h: dt_amax_read has the slot map), as a numpy float32"""
        v = ctypes.c_float(0.0)
        self._sync_stream()
        self._check(self.lib.dt_amax_read(self.h, int(slot), ctypes.byref(v)), "dt_amax_read")
        return np.float32(v.value)


_default_ctx = None


def default_context():
    """Process-wide context on the current device (created on first use)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx
