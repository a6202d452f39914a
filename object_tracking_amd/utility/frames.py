"""Frame ingest for the predict entry points (host bookkeeping, not the hot path).

The reference does  cv2.imread -> cv2.resize(image,(IMAGE_H,IMAGE_W)) -> /255.
(models_detection/KerasYOLO.py:525-528).  OpenCV is not part of this image, so
decoding uses PIL; the resize runs on the device (csrc/ingest.hip: OpenCV's 8-bit
INTER_LINEAR scheme -- half-pixel centres, no anti-aliasing, 11-bit fixed-point
coefficients).  Parity with OpenCV itself is unpinned (cv2 absent).  Frames stay
uint8 BGR (cv2.imread's channel order; the reference's predict path never flips
to RGB); the /255. happens on the device, fused into conv_1.
"""
import numpy as np


def imread_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def imwrite_bgr(path, image):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image[..., ::-1])).save(path)


def resize_bilinear_u8(image, out_h, out_w, ctx=None):
    """HxWx3 uint8 -> out_h x out_w x3 uint8 on the device (dt_ingest_resize: OpenCV's 8-bit
    INTER_LINEAR scheme, half-pixel centres, no anti-aliasing)."""
    import torch
    import mi355_dt
    ctx = ctx if ctx is not None else mi355_dt.default_context()
    d = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)[None]).to(ctx.device)
    return ctx.ingest_resize(d, out_h, out_w)[0].cpu().numpy()


def nv12_planes(surface, height, width, pitch=None):
    """One NV12 surface as a video decoder returns it -- a uint8 tensor of at least (height + height/2) * pitch bytes: `height` rows of Y,
    then height/2 rows of interleaved U,V, every row `pitch` bytes apart (default: width) -- -> the pair (y [height, width],
    uv [height/2, width/2, 2]) that ingest_frames takes.  Both are VIEWS of the surface: nothing is copied."""
    pitch = width if pitch is None else int(pitch)
    if height < 2 or width < 2 or height % 2 or width % 2:
        raise ValueError("an NV12 surface has an even height and width, got %dx%d" % (height, width))
    if pitch < width:
        raise ValueError("pitch %d is below the width %d" % (pitch, width))
    rows = height + height // 2
    flat = surface.reshape(-1)
    if flat.numel() < rows * pitch:
        raise ValueError("a %dx%d NV12 surface at pitch %d holds %d bytes, got %d" % (height, width, pitch, rows * pitch, flat.numel()))
    y = flat.as_strided((height, width), (pitch, 1))
    uv = flat.as_strided((height // 2, width // 2, 2), (pitch, 2, 1), height * pitch)
    return y, uv


def ingest_frames(frames, image_h, image_w, ctx=None, swap_rb=False):
    """A list of device frames -- uint8 [H,W,3] tensors (row-pitched views allowed) and NV12 pairs (y, uv), each at its own size -- ->
    uint8 [n, image_h, image_w, 3] on the device, the network input (dt_ingest_frames: one fused launch per 64 frames, no host wait)."""
    import mi355_dt
    ctx = ctx if ctx is not None else mi355_dt.default_context()
    return ctx.ingest_frames(frames, image_h, image_w, swap_rb=swap_rb)


class FrameView(object):
    """A host-side description of one VIEW of a frame (dt_ingest_views): which part of the frame goes where in the
    network input, and what surrounds it.
      frame  what ingest_frames takes as an item: a uint8 [H,W,3] device tensor (row-pitched views allowed) or an NV12 pair (y, uv)
      crop   (x, y, w, h) in pixels of the frame, any parity; None: the whole frame
      fit    "letterbox" (the largest centred rectangle of the crop's aspect ratio, mi355_dt.view_fit) or "stretch" (the whole input)
      fill   three bytes for channels 0, 1, 2 of the pixels around the destination rectangle (written as they are, swap_rb or not)
      dst    (x, y, w, h) in pixels of the network input: an explicit destination rectangle, instead of the fit"""
    __slots__ = ("frame", "crop", "fit", "fill", "dst")

    def __init__(self, frame, crop=None, fit="letterbox", fill=(128, 128, 128), dst=None):
        self.frame, self.crop, self.fit, self.fill, self.dst = frame, crop, fit, fill, dst


def ingest_views(views, image_h, image_w, ctx=None, swap_rb=False, fit="letterbox", fill=(128, 128, 128)):
    """A list of FrameViews -- and plain frames of ingest_frames, taken whole with `fit` and `fill` -- -> (uint8 [n, image_h, image_w, 3]
    on the device, affine float32 numpy [n, 4]): every crop converted, resized into its destination rectangle and surrounded by its fill
    in one fused launch per 32 views (dt_ingest_views); Context.boxes_map(boxes, counts, affine) takes the decoded boxes back to the
    source frames' normalised coordinates.  Boxes that lie in the fill are neither clipped nor dropped."""
    import mi355_dt
    ctx = ctx if ctx is not None else mi355_dt.default_context()
    return ctx.ingest_views(views, image_h, image_w, swap_rb=swap_rb, fit=fit, fill=fill)


def load_frame(path, image_h, image_w, ctx=None):
    """Returns (original BGR image, resized uint8 BGR frame)."""
    image = imread_bgr(path)
    return image, resize_bilinear_u8(image, image_h, image_w, ctx)
