"""Plain restatement of dt_ingest_frames (include/mi355_dt.h) in numpy: test infrastructure only.

An item is what the entry takes, on the host: a uint8 array [H, W, 3] (RGB24, the bytes as they lie) or a pair (y [H, W], uv [H/2, W/2, 2])
(NV12).  Output frame = resize(convert(item)): the conversion is written out here from the definition; the resize is the oracle's
(oracle.resize_bilinear_u8), which stays the yardstick for it.
"""
import numpy as np


def nv12_to_rgb_unclamped(y, uv):
    """y uint8 [H, W], uv uint8 [H/2, W/2, 2] -> int32 [H, W, 3]: (R, G, B) after the >> 20 and BEFORE the clamp to [0, 255]"""
    y = np.asarray(y)
    uv = np.asarray(uv)
    H, W = y.shape
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and H % 2 == 0 and W % 2 == 0 and uv.shape == (H // 2, W // 2, 2), (y.shape, uv.shape)
    r, c = np.arange(H)[:, None] // 2, np.arange(W)[None, :] // 2      # chroma is NOT interpolated: one pair per 2x2 pixels
    Y = y.astype(np.int32)
    U = uv[r, c, 0].astype(np.int32)
    V = uv[r, c, 1].astype(np.int32)
    yy = np.maximum(Y - 16, 0) * np.int32(1220542)
    u = U - 128
    v = V - 128
    R = (yy + 1673527 * v + 524288) >> 20
    G = (yy - 852492 * v - 409993 * u + 524288) >> 20
    B = (yy + 2116026 * u + 524288) >> 20
    out = np.stack([R, G, B], axis=-1)
    assert out.dtype == np.int32
    return out


def nv12_to_rgb(y, uv):
    """y uint8 [H, W], uv uint8 [H/2, W/2, 2] -> uint8 [H, W, 3] in (R, G, B) order"""
    return np.clip(nv12_to_rgb_unclamped(y, uv), 0, 255).astype(np.uint8)


def convert(item, swap_rb=False):
    """one item -> uint8 [H, W, 3], the frame the resize reads"""
    if isinstance(item, (tuple, list)):
        rgb = nv12_to_rgb(*item)
    else:
        rgb = np.asarray(item)
        assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3, rgb.shape
    return np.ascontiguousarray(rgb[..., ::-1] if swap_rb else rgb)


def ingest_frames_ref(items, out_h, out_w, swap_rb=False):
    """items -> uint8 [n, out_h, out_w, 3]: every item converted, optionally channel-swapped, then resized on its own"""
    from oracle import oracle as orc
    out = np.empty((len(items), out_h, out_w, 3), dtype=np.uint8)
    for i, item in enumerate(items):
        out[i] = orc.resize_bilinear_u8(convert(item, swap_rb)[None], out_h, out_w)[0]
    return out
