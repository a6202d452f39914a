/*
 * mi355_dt.h -- C ABI of libmi355_dt.so: the MI355X (gfx950) detect-and-track
 * hot path of ktzsh/object-tracking.
 *
 * The reference has no FFI on this path: its hot path is Keras calls made from
 * two Python classes.  The in-tree precedent for
 * "Python host <-> C-ABI .so" is models_detection/YOLO.py:6-37,58-119 (ctypes
 * over libdarknet.so).  Each entry point below names the reference call it
 * replaces.  Conventions:
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from dt_last_error(ctx);
 *   - pointers named d_* are DEVICE pointers (e.g. torch tensor.data_ptr());
 *     pointers named h_* are HOST pointers; the caller owns all of them;
 *   - all tensors are dense float32 NHWC unless stated; frames may be uint8;
 *   - every launch goes to the stream set with dt_set_stream (default: the
 *     null stream); calls are asynchronous with respect to the host unless
 *     stated; one dt_ctx per GPU per process, not re-entrant across threads;
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point fails with DT_ERR_DEVICE.
 */
#ifndef MI355_DT_H
#define MI355_DT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported from a library built with -fvisibility=hidden */
#define DT_API __attribute__((visibility("default")))

#define DT_OK 0
#define DT_ERR_ARG 1      /* bad argument / shape */
#define DT_ERR_DEVICE 2   /* HIP error (no device, launch failure, OOM) */
#define DT_ERR_STATE 3    /* weights not loaded / wrong call order */

#define DT_FRAMES_U8 0    /* uint8 HWC frames; x/255. fused into conv_1 (utils.py:150-153) */
#define DT_FRAMES_F32 1   /* float32 frames, already normalised */

#define DT_BOX_FLOATS 8   /* x, y, w, h, conf, label, score, cell */
#define DT_TRACK_FLOATS 8 /* a track read-out row: x, y, w, h, label, vx, vy, 0 (dt_associate_tracks) */
#define DT_TRACK_INTS 4   /* ... and its integers: id, age, hits, box */

#define DT_MATCH_DECODE_ORDER 0 /* track match policy (dt_associate_tracks_match): boxes in decode order, entries of the box's label */
#define DT_MATCH_BEST_FIRST 1   /* ... bit: the candidate pairs are taken best IoU first */
#define DT_MATCH_ANY_LABEL 2    /* ... bit: labels are not compared */
#define DT_ASSIGN_IOU_SCALE 1048576 /* track assignment (dt_associate_tracks_assign): a candidate weighs 1 + trunc(IoU * this), 2^20 */

#define DT_SCORE_INTS 8       /* track scoring totals of a clip (dt_track_score): frames, gt boxes, hyp boxes, matches, switches, fragments, overflow, 0 */
#define DT_SCORE_OBJ_INTS 8   /* ... a row of its object table: gt id, last track id (-1: never matched), present, matched, switches, fragments,
                               *     last appearance matched (0/1), 0 */
#define DT_SCORE_ANY_LABEL 1  /* ... flag bit: labels are not compared */
#define DT_SCORE_RESUME 2     /* ... flag bit: d_totals, d_objs, d_nobjs are in-out and the call continues from them */
#define DT_IDENT_INTS 8       /* identity scoring sizes of a clip (dt_identity_overlap): frames, gt boxes, hyp boxes, gt trajectories, hyp trajectories,
                               *     gt overflow boxes, hyp overflow boxes, valid pairs */
#define DT_HOTA_MAX_THR 32    /* HOTA scoring (dt_hota_count): the most IoU thresholds of a call */

typedef struct dt_ctx dt_ctx;

/* ---- context ---------------------------------------------------------- */
DT_API int dt_create(dt_ctx **out);
DT_API void dt_destroy(dt_ctx *ctx);
DT_API const char *dt_last_error(dt_ctx *ctx);
DT_API int dt_set_stream(dt_ctx *ctx, void *hip_stream);
/* ABI version of this header: major*100+minor (1.08: 1.07 + dt_amax_read, and later the four stream entries dt_stream_open, dt_stream_reset,
 * dt_track_stream_forward, dt_associate_stream, and the three track-memory entries dt_associate_mem, dt_stream_open_tracks, dt_associate_stream_mem
 * and the four tiny-tracker stream entries dt_tiny_stream_open, dt_tiny_stream_reset, dt_tiny_stream_sequence, dt_tiny_stream_forward
 * and the two track-motion entries dt_associate_motion, dt_associate_stream_motion
 * and the two track read-out entries dt_associate_tracks, dt_associate_stream_tracks
 * and the two track match policy entries dt_associate_tracks_match, dt_associate_stream_tracks_match
 * and the one frame-ingest entry dt_ingest_frames
 * and the four frame-view entries dt_view_fit, dt_view_affine, dt_ingest_views, dt_boxes_map
 * and the one track scoring entry dt_track_score
 * and the two detection scoring entries dt_detect_match, dt_detect_rank
 * and the two identity scoring entries dt_identity_overlap, dt_assign_max
 * and the three HOTA scoring entries dt_hota_align, dt_hota_weights, dt_hota_count
 * and the two track assignment entries dt_associate_tracks_assign, dt_associate_stream_tracks_assign
 * and the three Winograd transform test entries dt_wino_geometry, dt_wino_input, dt_wino_output
 * and the one implicit-GEMM kernel test entry dt_conv_igemm
 * and the two track score entries dt_associate_tracks_scored, dt_associate_stream_tracks_scored
 * and the one conv_1 kernel test entry dt_conv1
 * -- additions only, the number stayed; 1.07: 1.06 + dt_gemm_split, dt_policy_set) */
DT_API int dt_abi_version(void);

/* ---- detector: KerasYOLO ---------------------------------------------- */
/* Replaces KerasYOLO.load_model graph construction (KerasYOLO.py:277-405) for
 * image_h x image_w inputs (multiples of 32), nb_box anchors per cell and
 * nb_class classes; anchors[2*nb_box] as KerasYOLO.ANCHORS (KerasYOLO.py:45). */
DT_API int dt_detector_config(dt_ctx *ctx, int image_h, int image_w, int nb_box,
                       int nb_class, const float *h_anchors);

/* Replaces init_weights + WeightReader (KerasYOLO.py:244-274,
 * utility/utils.py:138-148).  h_blob = float32 contents of a darknet .weights
 * file INCLUDING its 4-float header (the reader's offset starts at 4).  Folds
 * inference BatchNorm (eps 1e-3) into each kernel and uploads.  *consumed
 * receives the reader offset after conv_23 (may be NULL). */
DT_API int dt_load_darknet_weights(dt_ctx *ctx, const float *h_blob, size_t n_floats,
                            size_t *consumed);

/* Replaces model.predict([input_image, dummy])  (KerasYOLO.py:531) and the
 * two-output detector Model of MultiObjDetTracker.py:162-164.
 *   d_frames  [batch, H, W, 3] uint8 or float32 (frames_dtype)
 *   d_netout  [batch, G, G, nb_box*(5+C)]  raw conv_23 output     (may be NULL)
 *   d_feat    [batch, G, G, 1024]          'conv_feat' activation (may be NULL) */
DT_API int dt_detect_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype,
                      int batch, float *d_netout, float *d_feat);

/* Replaces KerasYOLO.extract's intermediate_layer_model for the named taps the
 * reference reaches for: "conv_23", "conv_feat", "act_13" (26x26x512 skip
 * tensor, the TinyTracker feature layer, config.json:9).  Valid after a
 * dt_detect_forward of the same batch; copies into d_out. */
DT_API int dt_detector_tap(dt_ctx *ctx, const char *name, int batch, float *d_out);

/* Replaces KerasYOLO.extract's intermediate_layer_model for ANY layer of the detector graph
 * (KerasYOLO.py:509-520: Model(inputs, self.model.get_layer(layer).output).predict(...)).  Layer names as the
 * reference / Keras give them: conv_1..conv_23 (Conv2D output; conv_23 incl. its bias), norm_1..norm_22
 * (BatchNormalization output), leaky_re_lu_1..21 (alias act_N) and conv_feat (after LeakyReLU),
 * max_pooling2d_1..5, lambda_1 (space_to_depth), concatenate_1, reshape_1 / lambda_2 (= conv_23 values).
 * The fused production path never materialises most of these: the call re-runs the graph up to the layer and
 * executes that layer un-fused (a one-image debugging call, not a hot path).  The layers before it run in the
 * kernel forms dt_detect_forward takes at this batch; leaky_re_lu_4 is written by the fused conv_3 + conv_4
 * launch itself wherever the forward takes that launch.
 *   shape4 [4] receives (batch, h, w, channels) of the layer (may be NULL); with d_out == NULL only the shape
 *   is returned; d_out holds out_floats floats and receives the dense NHWC tensor. */
DT_API int dt_detector_extract(dt_ctx *ctx, const void *d_frames, int frames_dtype, int batch,
                               const char *layer, float *d_out, size_t out_floats, int *shape4);

/* ---- frame ingest ----------------------------------------------------- */
/* Replaces cv2.resize(image, (IMAGE_H, IMAGE_W)) on decoded uint8 frames
 * (KerasYOLO.py:526, MultiObjDetTracker.py:302); the /255. of normalize() is fused into
 * conv_1.  OpenCV's 8-bit INTER_LINEAR scheme (half-pixel centres, 11-bit coefficients).
 *   d_src [n, src_h, src_w, 3] uint8  ->  d_dst [n, dst_h, dst_w, 3] uint8 */
DT_API int dt_ingest_resize(dt_ctx *ctx, const uint8_t *d_src, int n, int src_h, int src_w,
                     uint8_t *d_dst, int dst_h, int dst_w);

/* Frames as a video decoder or a cropped view hands them out (addition; BUILD-DEFINED): NV12 or 3-byte interleaved
 * frames, each with its own size and row pitches, converted and resized to the uint8 network input in one call.
 * Output frame i = resize(convert(h_desc[i])):
 *   convert, RGB24: the three bytes of a pixel as they lie.
 *   convert, NV12:  Y = plane0[r*pitch0 + c], (U, V) = plane1[(r/2)*pitch1 + (c/2)*2 + {0, 1}] -- chroma is NOT interpolated -- and, in
 *                   int32 with an arithmetic >>:  y = max(Y - 16, 0) * 1220542, u = U - 128, v = V - 128,
 *                     R = clamp((y + 1673527*v             + 524288) >> 20, 0, 255)
 *                     G = clamp((y -  852492*v - 409993*u  + 524288) >> 20, 0, 255)
 *                     B = clamp((y + 2116026*u             + 524288) >> 20, 0, 255)
 *                   (BT.601 limited range, the fixed-point constants OpenCV publishes for its 8-bit YUV420 conversions; parity with cv2
 *                   itself is unpinned, as for the resize); output channel order (R, G, B).
 *   DT_PIX_SWAP_RB: channels 0 and 2 of the converted pixel exchanged, for either format.
 *   resize:         dt_ingest_resize's scheme on the converted 8-bit values, bit for bit.
 * h_desc is a HOST array of n descriptors, consumed before the call returns (like h_slots); the call is asynchronous on the context's
 * stream.  The descriptors travel as kernel arguments, 64 frames per launch: a call makes ceil(n / 64) launches and no device upload,
 * keeps nothing per size in the context and never waits for the device, whatever sizes it mixes.  (dt_ingest_resize keeps its
 * per-size table and remains the entry for tight same-size batches.)
 * DT_ERR_ARG, with the frame index in the message where a descriptor is at fault: a null ctx, h_desc, d_dst or needed plane; n <= 0;
 * dst_h / dst_w outside dt_ingest_resize's bounds; height or width < 1 or > 16384; NV12 with an odd height or width; a pitch below its
 * minimum; an unknown format value or flag bit; reserved != 0.  The whole array is validated before anything is launched: an error
 * leaves d_dst untouched.
 * Not done here, on purpose: full-range and BT.709 matrices, chroma interpolation, planar I420, 10-bit surfaces.  Crop rectangles and
 * letterboxing are not this entry's either: they are dt_ingest_views', further down. */
#define DT_PIX_RGB24   0   /* 3 interleaved bytes per pixel, taken in the order they lie (what dt_ingest_resize reads) */
#define DT_PIX_NV12    1   /* plane0 = Y [height][pitch0]; plane1 = U,V interleaved [height/2][pitch1], one pair per 2x2 pixels */
#define DT_PIX_SWAP_RB 16  /* flag, or-ed in: output channels 0 and 2 exchanged */

typedef struct dt_frame_desc {
    const void *d_plane0, *d_plane1;   /* device pointers; plane1 ignored (may be NULL) for RGB24 */
    int32_t height, width;             /* pixels; NV12: both even */
    int32_t pitch0, pitch1;            /* bytes per row; RGB24: pitch0 >= 3*width; NV12: pitch0 >= width, pitch1 >= width */
    int32_t format;                    /* DT_PIX_* [| DT_PIX_SWAP_RB] */
    int32_t reserved;                  /* 0 */
} dt_frame_desc;

DT_API int dt_ingest_frames(dt_ctx *ctx, const dt_frame_desc *h_desc, int n,
                            uint8_t *d_dst, int dst_h, int dst_w);

/* Frame VIEWS (addition; BUILD-DEFINED): a frame of dt_ingest_frames plus a source rectangle (a crop), a destination
 * rectangle inside the network input (a placement, e.g. a letterbox) and a fill colour around it -- converted, cropped, resized and placed
 * in one launch -- and the map that takes the decoded boxes back to the SOURCE frame's normalised coordinates.  Integer arithmetic only.
 *   source rectangle       (src_x, src_y, src_w, src_h) in pixels of the frame: src_w, src_h >= 1, inside the frame.  Any parity is
 *                          allowed for NV12: chroma is addressed by the ABSOLUTE pixel position, plane1[((src_y+r)/2)*pitch1 +
 *                          ((src_x+c)/2)*2 + {0, 1}] -- the conversion is pointwise, so cropping commutes with it.
 *   destination rectangle  (dst_x, dst_y, dst_w, dst_h) in pixels of the output frame [out_h, out_w]: dst_w, dst_h >= 1, inside it.
 *   fill                   three bytes, written as they are to channels 0, 1, 2 of every output pixel outside the destination rectangle;
 *                          DT_PIX_SWAP_RB does not touch them.
 * Inside the destination rectangle, output pixel (dst_y + r, dst_x + c) is pixel (r, c) of dt_ingest_frames' resize of
 * crop(convert(frame)) from src_h x src_w to dst_h x dst_w: the coefficients are those of (src_w, dst_w, c) and (src_h, dst_h, r),
 * operation for operation, and the source indices are offset by (src_y, src_x).  A view whose source rectangle is the whole frame and
 * whose destination rectangle is the whole output is dt_ingest_frames, bit for bit.
 *
 * dt_view_fit: the destination rectangle rect = (x, y, w, h) that fits a src_w x src_h source into an out_w x out_h output.  A host
 * function without a context or a device.
 *   DT_FIT_STRETCH    (0, 0, out_w, out_h)
 *   DT_FIT_LETTERBOX  in 64-bit integers with truncating divisions (round half up, centred, the odd pixel below and to the right):
 *                       if src_w*out_h >= src_h*out_w:  w = out_w, h = max(1, (src_h*out_w + src_w/2) / src_w)
 *                       otherwise:                      h = out_h, w = max(1, (src_w*out_h + src_h/2) / src_h)
 *                       x = (out_w - w)/2, y = (out_h - h)/2
 *                     1920x1080 -> 416x416 gives (0, 91, 416, 234); 1080x1920 gives (91, 0, 234, 416).
 *   DT_ERR_ARG: a size < 1, an unknown mode, a null rect.
 *
 * dt_view_affine: affine = (ax, bx, ay, by), the map from decode's boxes -- normalised to the network input -- to the view's source
 * frame, normalised to the WHOLE frame (width, height), not to the crop.  A host function without a context or a device.
 *   ax = (float)((double)(out_w*src_w) / (double)(dst_w*width)),  bx = (float)((double)(src_x*dst_w - dst_x*src_w) / (double)(dst_w*width))
 *   ay, by likewise with out_h, src_h, dst_h, height, src_y, dst_y.  The integer products are exact in int64; one double division, then
 *   one rounding to float.  DT_ERR_ARG: a null pointer or one of those sizes < 1.
 * A box maps as x' = x*ax + bx, y' = y*ay + by, w' = w*ax, h' = h*ay in float32, the product rounded and then the sum rounded (no FMA).
 * Boxes whose centre lies in the fill are NOT clipped or dropped: they map to coordinates outside the crop (or outside [0, 1]).
 *
 * dt_ingest_views keeps dt_ingest_frames' contract: h_views is a HOST array consumed before the call returns; the views travel as
 * kernel arguments, 32 views per launch (32 x 80 bytes and the other arguments stay within HIP's 4096 bytes of kernel arguments): a
 * call makes ceil(n / 32) launches, no upload, uses no workspace, never waits for the device and keeps nothing per size.  The whole
 * array is validated before the first launch -- everything dt_ingest_frames checks on the embedded descriptor, both rectangles as
 * defined above, both reserved fields 0 -- and an error (DT_ERR_ARG) names the frame and leaves d_dst untouched.
 *
 * dt_boxes_map applies per-frame affines in place to floats 0..3 of rows < min(d_counts[i], cap) of frame i of d_boxes
 * [n][cap][DT_BOX_FLOATS]; every other float and every other row keeps its bits.  h_affine is a HOST array [n][4], consumed before the
 * call returns; the affines travel as kernel arguments, 128 frames per launch.  DT_ERR_ARG: a null pointer, n <= 0, cap <= 0, a
 * non-finite affine (nothing is launched then). */
#define DT_FIT_STRETCH   0
#define DT_FIT_LETTERBOX 1

typedef struct dt_frame_view {
    dt_frame_desc frame;                     /* as for dt_ingest_frames, reserved == 0 */
    int32_t src_x, src_y, src_w, src_h;      /* the crop, pixels of the frame */
    int32_t dst_x, dst_y, dst_w, dst_h;      /* the placement, pixels of the output frame */
    uint8_t fill[3]; uint8_t reserved0;      /* channels 0, 1, 2 outside the placement; 0 */
    int32_t reserved;                        /* 0 */
} dt_frame_view;                             /* 80 bytes */

DT_API int dt_view_fit(int src_w, int src_h, int out_w, int out_h, int mode, int32_t rect[4]);
DT_API int dt_view_affine(const dt_frame_view *v, int out_w, int out_h, float affine[4]);
DT_API int dt_ingest_views(dt_ctx *ctx, const dt_frame_view *h_views, int n,
                           uint8_t *d_dst, int out_h, int out_w);
DT_API int dt_boxes_map(dt_ctx *ctx, float *d_boxes, const int *d_counts, int n, int cap,
                        const float *h_affine);

/* ---- decode_netout + NMS (utility/utils.py:208-257) -------------------- */
/*   d_netout  [batch, GH, GW, NB, 5+NC]  raw logits (NOT modified)
 *   d_boxes   [batch, cap, DT_BOX_FLOATS] surviving boxes in (row,col,b) order; rows from
 *             min(count, cap) on are zero-filled (the buffer may be uninitialised)
 *   d_counts  [batch] int32: number of survivors (may exceed cap; extra dropped)
 *   d_classes [batch, cap, NC] post-NMS class scores per box (may be NULL)
 *   d_post    [batch, GH, GW, NB, 5+NC] the reference's in-place-mutated netout
 *             (conf / thresholded class scores after NMS) (may be NULL)        */
DT_API int dt_decode(dt_ctx *ctx, const float *d_netout, int batch, int GH, int GW,
              int NB, int NC, float obj_threshold, float nms_threshold,
              const float *h_anchors, int cap, float *d_boxes, int *d_counts,
              float *d_classes, float *d_post);

/* The same with one (obj_threshold, nms_threshold) pair PER FRAME -- d_thresholds [batch, 2] float32 on the
 * device: streams of a batch may run different operating points (addition; the reference decodes one frame per
 * call with one pair, utils.py:208). */
DT_API int dt_decode_per_frame(dt_ctx *ctx, const float *d_netout, int batch, int GH, int GW,
                        int NB, int NC, const float *d_thresholds, const float *h_anchors, int cap,
                        float *d_boxes, int *d_counts, float *d_classes, float *d_post);

/* bbox_iou (utility/utils.py:155-173) on n pairs: d_pairs [n,8] -> d_iou [n] */
DT_API int dt_bbox_iou(dt_ctx *ctx, const float *d_pairs, int n, float *d_iou);

/* ---- tracker: MultiObjDetTracker --------------------------------------- */
/* Replaces MultiObjDetTracker.load_model's recurrent head
 * (MultiObjDetTracker.py:175-183) + load_weights (:291-293).  Keras layouts:
 *   h_kernel     [3,3,Cb+1024,4U]  ConvLSTM2D input kernel, x_bbox channels first
 *   h_recurrent  [3,3,U,4U]        recurrent kernel
 *   h_bias       [4U]              gate order i,f,c,o
 *   h_out_kernel [1,1,U,Cb]        'tconv_2' 1x1 conv,  h_out_bias [Cb]
 * with Cb = nb_box*(5+C), U = units (512). */
DT_API int dt_tracker_load(dt_ctx *ctx, int units, const float *h_kernel,
                    const float *h_recurrent, const float *h_bias,
                    const float *h_out_kernel, const float *h_out_bias);

/* Replaces model.predict([x, b]) of the tracker model (MultiObjDetTracker.py:307).
 *   d_frames [n_clips, T, H, W, 3]
 *   d_trk    [n_clips, T, G, G, Cb]  'tracking' output grid   (may be NULL)
 *   d_det    [n_clips, T, G, G, Cb]  'detection' output grid  (may be NULL)
 * ConvLSTM state is zero at t=0 of every call (stateless Keras RNN). */
DT_API int dt_track_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype,
                     int n_clips, int T, float *d_trk, float *d_det);

/* The two halves of dt_track_forward, exposed so that ONE stream can use several GPUs (frame-shard, SURVEY.md 8e row 3,
 * BASELINE.json configs[4]): each rank runs the TimeDistributed detector (MultiObjDetTracker.py:166-171) on its share
 * of the frames, the per-frame rows z = [conv_feat 1024 | x_bbox Cb | zero pad] are exchanged (RCCL all-gather), and
 * the owner of a clip runs ConvLSTM2D + tconv_2 (:175-183) on the stitched rows.  dt_track_row_width = floats per grid
 * cell of a row (1024 + Cb rounded up to 32).
 *   dt_track_detect:    d_frames [n_frames,H,W,3]      -> d_z [n_frames, G, G, row_width]
 *   dt_track_recurrent: d_z [n_clips, T, G, G, row_width] -> d_trk [n_clips,T,G,G,Cb] (+ d_det, may be NULL)
 * dt_track_forward == dt_track_detect on all frames followed by dt_track_recurrent. */
DT_API int dt_track_row_width(dt_ctx *ctx);
DT_API int dt_track_detect(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n_frames, float *d_z);
DT_API int dt_track_recurrent(dt_ctx *ctx, const float *d_z, int n_clips, int T, float *d_trk, float *d_det);

/* The same split ONE STEP LATER in the graph (the default of parallel.track_clips_frame_sharded): ConvLSTM2D's input
 * projection W * x_t + b (MultiObjDetTracker.py:176) does not depend on the recurrence, so the rank that ran the detector on a
 * frame runs it as well -- 55 % of the recurrent head's FLOPs move from the clip's owner (sequential in T) to the part that is
 * spread over all GPUs -- and the rows that travel are the projection rows, dt_track_xproj_width = 4 * units floats per grid cell.
 *   dt_track_detect_xproj:    d_frames [n_frames,H,W,3] -> d_xp [n_frames, G, G, 4U]  (+ d_det [n_frames,G,G,Cb], may be NULL)
 *   dt_track_recurrent_xproj: d_xp [n_clips, T, G, G, 4U] -> d_trk [n_clips,T,G,G,Cb]
 * dt_track_forward == dt_track_detect_xproj on all frames followed by dt_track_recurrent_xproj. */
DT_API int dt_track_xproj_width(dt_ctx *ctx);
DT_API int dt_track_detect_xproj(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n_frames, float *d_xp, float *d_det);
DT_API int dt_track_recurrent_xproj(dt_ctx *ctx, const float *d_xp, int n_clips, int T, float *d_trk);

/* Track identity (BUILD-DEFINED, DESIGN.md "Track identity"; the reference has
 * none).  d_boxes [n_clips,T,cap,8], d_counts [n_clips,T]
 * -> d_ids [n_clips,T,cap] int32 (-1 unused), d_nids [n_clips] ids opened. */
DT_API int dt_associate(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold,
                 int *d_ids, int *d_nids);
/* Track memory (BUILD-DEFINED, DESIGN.md "Track identity"): a track that misses up to max_age frames keeps its id.  The kernel keeps a
 * track table of at most tcap entries (box, label, id, age = frames since the track last had a box) per clip; a box takes the id of the
 * unclaimed entry of its label with age <= max_age and the largest IoU >= assoc_threshold (ties: lowest table index), else a new id.
 * After a frame the table is the frame's boxes in decode order followed by the unclaimed entries with age + 1 <= max_age in their old
 * order, cut at tcap.  d_gaps [n_clips,T,cap] (may be NULL): the claimed entry's age -- 0 unbroken, k after k missed frames, -1 for a
 * new id and in unused entries.  max_age = 0 is dt_associate bit for bit.  No motion model, no cross-label match, no optimal assignment.
 * DT_ERR_ARG: max_age < 0, tcap < cap, or a table that does not fit the LDS (tcap <= 64 and T <= 64 run in registers and need none). */
DT_API int dt_associate_mem(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap,
                 int *d_ids, int *d_nids, int *d_gaps);
/* Track motion (BUILD-DEFINED, DESIGN.md "Track identity"): dt_associate_mem with every table entry matched where a constant velocity
 * predicts it.  An entry carries a velocity (vx, vy) of its box's x, y per frame.  With k = (float)(age + 1) its predicted box is
 * (x + k*vx, y + k*vy, w, h) and the IoU of the match is taken against that box; everything else of the match is dt_associate_mem's.
 * When a box claims an entry: o = (x_box - x_entry) / k on the entry's STORED x (y likewise), v_box = v + gain * (o - v); a box that
 * opens a new id starts at rest.  Survivors keep box and velocity.  All float32, every operation rounded on its own, no FMA.
 * gain in [0, 1]; gain = 0 is dt_associate_mem bit for bit.  max_age = 0 still uses the velocity: an age-0 entry is matched one step
 * ahead, and in dense scenes that can open a few more ids than dt_associate does.  w / h are not predicted; boxes must be finite.
 * No Kalman filter, no cross-label match, no optimal assignment; a minimum hit count and the read-out of predicted boxes: dt_associate_tracks.
 * DT_ERR_ARG: as dt_associate_mem (the LDS tables hold 9 words per entry here, so the largest tcap is smaller), and gain outside
 * [0, 1] or NaN. */
DT_API int dt_associate_motion(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap, float gain,
                 int *d_ids, int *d_nids, int *d_gaps);
/* Track read-out (BUILD-DEFINED, DESIGN.md "Track identity"): dt_associate_motion with a hit count per table entry, and the table written
 * out once per frame.  Match, velocity update, rebuild and capacity cut are dt_associate_motion's bit for bit: d_ids, d_nids, d_gaps are
 * its outputs for any min_hits.  hits = frames in which the track had a box: 1 for a box that opens an id, the claimed entry's + 1 for a
 * box that claims one, unchanged for an unclaimed survivor.
 *   d_hits    [n_clips, T, cap] int32     hits of box i's track after frame t, -1 in unused entries; may be NULL (so may d_gaps)
 *   d_tracks  [n_clips, T, tcap, DT_TRACK_FLOATS]   x, y, w, h, label, vx, vy, 0 of every CONFIRMED entry (hits >= min_hits) of the table
 *             after frame t's rebuild and cut, compacted in table order: the frame's boxes in decode order, then the lost tracks.  An
 *             entry of age 0 reports its stored x, y bits; one of age a >= 1 reports x + (float)a * vx, y + (float)a * vy (one multiply,
 *             then one add): where the track is expected in frame t.  w, h, vx, vy are the stored values.
 *   d_tinfo   [n_clips, T, tcap, DT_TRACK_INTS] int32   id, age, hits, box: the index of the entry's box in frame t, -1 for a coasting entry
 *   d_tcounts [n_clips, T] int32          rows written; rows from there on are zero in d_tracks and -1 in d_tinfo (the buffers may
 *             arrive uninitialised)
 * d_tracks, d_tinfo, d_tcounts: all three, or all three NULL (no read-out).  min_hits = 1, max_age = 0: the read-out is the frame's boxes.
 * Not done here: dropping an unconfirmed track at its first miss, a Kalman filter, a w / h model, an optimal assignment; cross-label
 * matching and a best-IoU-first order: dt_associate_tracks_match.
 * DT_ERR_ARG: as dt_associate_motion (the LDS tables hold 10 words per entry here, so the largest tcap is smaller again), min_hits < 1,
 * a partial read-out triple. */
DT_API int dt_associate_tracks(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap, float gain, int min_hits,
                 int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* Track match policy (BUILD-DEFINED, DESIGN.md "Track match policy"): dt_associate_tracks with the MATCH of a frame's boxes to the table
 * chosen by the call; prediction, velocity update, hits, gaps, rebuild, capacity cut and read-out are dt_associate_tracks' bit for bit.
 * match is a set of DT_MATCH_* bits, 0 to 3; match = 0 is dt_associate_tracks bit for bit.
 * Candidates of a frame: pairs (box i, table entry j with age <= max_age) whose IoU -- box i against entry j's predicted box -- is at
 * least assoc_threshold; the labels must be equal unless DT_MATCH_ANY_LABEL is set, which leaves them uncompared.
 * Without DT_MATCH_BEST_FIRST the boxes are visited in decode order and each takes its unclaimed candidate entry of the largest IoU,
 * ties to the lowest j.  With it the candidate pair of the largest IoU (compared as float32; ties to the lowest i, then the lowest j) is
 * taken repeatedly: box i claims entry j, every candidate of box i and of entry j leaves the set, until the set is empty -- a result
 * that does not depend on the order in which the frame's boxes arrive, ties apart.  Then the boxes that claimed nothing open new ids
 * in decode order; whenever both orders find the same pairs every output is the same bit for bit.  A box that claims an entry of another
 * label carries on its id, hits and velocity; the rebuilt entry has the box's label.
 * Not done here: an optimal (Hungarian) assignment -- that is dt_associate_tracks_assign below, an entry of its own --, a cost other
 * than IoU.
 * DT_ERR_ARG: as dt_associate_tracks, and match outside 0..3.  With DT_MATCH_BEST_FIRST the LDS also holds three words per box (best
 * candidate key, its entry, claimed), 20 * tcap + 4 * cap words in all: tcap = cap fits up to 1706 (1950 without the bit); a table
 * with tcap <= 64 and T <= 64 runs in registers and keeps only the frame's keys, 256 * cap bytes, in the LDS. */
DT_API int dt_associate_tracks_match(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match,
                 int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* Track assignment (BUILD-DEFINED, DESIGN.md "Track assignment"): dt_associate_tracks_match with the match of a frame replaced by an
 * optimal one-to-one assignment, the step every association tracker of the SORT family takes (Hungarian method on the IoU matrix).
 * Arguments and outputs are dt_associate_tracks_match's.  match is 0 or DT_MATCH_ANY_LABEL; DT_MATCH_BEST_FIRST is refused, for an
 * order means nothing to an assignment.
 * Candidates of a frame are exactly dt_associate_tracks_match's: pairs (box i in decode order, table entry j with age <= max_age), labels
 * equal as floats unless DT_MATCH_ANY_LABEL is set, iou = bbox_iou(box i, predicted box of entry j) >= assoc_threshold as float32; a NaN
 * is never a candidate.
 * Weights: a matrix W[n][nt] of int32 over all n boxes and all nt table entries.  A candidate has W[i][j] = 1 + (int)(iou *
 * 1048576.0f) (DT_ASSIGN_IOU_SCALE; the product is exact, the factor being a power of two, and the conversion truncates); every other
 * pair has weight 0.  IoU differences below 2^-20 are therefore ties.
 * Match: the claimed pairs are the row_to_col of dt_assign_max on W with rows = n and cols = nt -- the same method, the same
 * orientation rule (solved on the side with fewer rows), the same tie rule (the lowest column), pairs of weight 0 reported as
 * unassigned.  The result is an exact maximum of the summed quantised IoU over the one-to-one sets of candidates, and which optimum
 * is chosen is fixed.  The set of the largest weight is not always the largest set: one pair of IoU 0.9 beats two of 0.3 each, and the
 * box left over opens an id.
 * Everything after the match is dt_associate_tracks_match's bit for bit: a claiming box inherits id, gap, hits + 1 and the velocity
 * update on the entry's stored x, y; the other boxes open ids in decode order, at rest, with hits 1; rebuild, capacity cut and read-out
 * are unchanged.  Boxes must be finite; non-finite boxes give unspecified ids, but the call still terminates and stays in bounds.
 * Cost: up to min(n, nt)^2 solver steps per frame, each a pass over max(n, nt) entries 64 at a time; meant for frames of tens to a few
 * hundred boxes.
 * Not done here: a cost other than IoU, Kalman or w / h models, the optimal assignment inside dt_track_score's frame step.
 * DT_ERR_ARG: as dt_associate_tracks_match, match other than 0 or DT_MATCH_ANY_LABEL, and a table that does not fit the 160 KB of LDS:
 * beside the two tables and four words per box the LDS holds the solver's six work arrays of tcap + 1 words, so 26 * tcap + 4 * cap + 6
 * words must not exceed 40960 (tcap = cap fits up to 1365).  A table with tcap <= 64 and T <= 64 runs in registers and keeps only the
 * frame's weights and pairs, 260 * cap + 512 bytes, in the LDS. */
DT_API int dt_associate_tracks_assign(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match,
                 int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* Track scores (BUILD-DEFINED, DESIGN.md "Track scores"): dt_associate_tracks_assign in two passes that use the detection score beside
 * each box -- the BYTE rule (Zhang et al., ECCV 2022): confident boxes are matched first, the weak ones are offered only to the tracks
 * still unmatched, and a weak box no track wants is thrown away instead of opening a track.  Everything not named here is
 * dt_associate_tracks_assign's, bit for bit: arguments, outputs, prediction, velocity update, hits, gaps, rebuild order, capacity cut
 * and read-out.  match is 0 or DT_MATCH_ANY_LABEL.
 * A frame has n boxes, the table nt entries, and s_i = float score_at of box i (0..7; dt_decode writes conf at 4 and score at 6).
 * Classes: box i is HIGH when s_i >= score_high as float32, else LOW; a NaN score is LOW.
 * Pass 1: the candidates are dt_associate_tracks_assign's, restricted to HIGH boxes: W1[n][nt] is its weight matrix with every LOW row
 * zero, and the pairs are the row_to_col of dt_assign_max on W1 with rows = n and cols = nt -- the full shape, so that the solver's
 * orientation and tie rules do not depend on how many boxes are HIGH.
 * Pass 2 (skipped when max_age_low = -1): the candidates are the pairs of a LOW box i and an entry j that was not claimed in pass 1, with
 * age_j <= min(max_age, max_age_low), labels equal unless DT_MATCH_ANY_LABEL is set, and bbox_iou(box i, predicted box of j) >=
 * assoc_threshold_low as float32.  A candidate weighs 1 + (int)(iou * 1048576.0f), everything else 0, on the full [n][nt] shape; the
 * pairs are dt_assign_max's as in pass 1.  max_age_low = 0 is BYTE's own rule: a weak box only continues a track that had a box in the
 * previous frame.
 * After the passes a box that claimed an entry in either pass inherits exactly as in dt_associate_tracks_assign: id, gap, hits + 1 and
 * the velocity update.  An unclaimed box with s_i >= score_new opens an id, in decode order, at rest, with hits 1.  Every other unclaimed
 * box is DROPPED: d_ids = -1, d_gaps = -1, d_hits = 0 (in unused entries d_hits stays -1).
 * The table: a dropped box still takes its row among the frame's leading rows -- a DEAD row with id -1, hits 0, age 0 and velocity 0; its
 * box and label are stored.  So the table keeps its order: the leading rows are the frame's boxes in decode order, and an age-0 row's
 * `box` index is its table index.  A dead row is never a candidate of any association entry, is never confirmed or read out, and never
 * survives the next rebuild.  It DOES count in the capacity cut of the one frame that made it: with tcap close to the number of boxes
 * plus lost tracks, dropped boxes can push the last lost tracks out of the table.
 * Equivalences: if every box's score is >= both score_high and score_new, every output and the slot are dt_associate_tracks_assign's, bit
 * for bit.  With max_age_low = -1 and score_new = score_high the HIGH boxes get the ids, gaps and hits that dt_associate_tracks_assign
 * gives on the same frames with the LOW boxes removed and the rest moved up, as long as no capacity cut drops an entry in either run.
 * Boxes and scores must be finite otherwise: non-finite ones give unspecified ids, but the call still terminates and stays in bounds.
 * Not done here: a Kalman filter, a cost that weighs the score into the IoU, a separate rule for unconfirmed tracks (BYTE's third
 * step), scored variants of the decode-order and best-first policies.
 * DT_ERR_ARG, with nothing launched and nothing written: everything dt_associate_tracks_assign refuses, score_at outside 0..7, a NaN
 * score_high, score_new or assoc_threshold_low, max_age_low < -1, and a table that does not fit the 160 KB of LDS: the general form
 * holds one more word per box (its score), so 26 * tcap + 5 * cap + 6 words must not exceed 40960.  A table with tcap <= 64 and T <= 64
 * runs in registers, fetches the score as one more scalar per box and refills the one weight tile for pass 2: 260 * cap + 512 bytes, as
 * dt_associate_tracks_assign. */
DT_API int dt_associate_tracks_scored(dt_ctx *ctx, const float *d_boxes, const int *d_counts,
                 int n_clips, int T, int cap, float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match,
                 int score_at, float score_high, float score_new, float assoc_threshold_low, int max_age_low,
                 int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);

/* Track scoring (BUILD-DEFINED, DESIGN.md "Track scoring"): the CLEAR-MOT frame step (Bernardin & Stiefelhagen 2008) of a tracker's output
 * against ground-truth tracks, with the optimal assignment replaced by this library's best-IoU-first order.  Clips are scored
 * independently, one wavefront each, frames in sequence.
 *   d_gt_boxes  [n_clips, T, gcap, DT_BOX_FLOATS]  floats 0..3 = x, y, w, h as dt_decode normalises them, float 5 = label, the rest ignored
 *   d_gt_counts [n_clips, T] int32, d_gt_ids [n_clips, T, gcap] int32      rows g < min(count, gcap) take part
 *   d_hyp_boxes [n_clips, T, hcap, 8]   x, y, w, h in floats 0..3, the label in float hyp_label_at: 5 for dt_decode's boxes, 4 for read-out
 *               rows (DT_TRACK_FLOATS); d_hyp_counts [n_clips, T]; rows i < min(count, hcap) take part
 *   d_hyp_ids   the id of row i of frame t is word (t * hcap + i) * id_stride of the clip: id_stride = 1 with d_ids of dt_associate*,
 *               id_stride = DT_TRACK_INTS with d_tinfo -- so the confirmed-track read-out is scored by the same entry, its coasting rows
 *               as ordinary hypotheses
 * The OBJECT TABLE of a clip has at most ocap rows of DT_SCORE_OBJ_INTS int32, one per distinct ground-truth id in order of first appearance.
 * The step of a frame (every read of the table sees it as the previous frame left it; it is written behind the match):
 *   valid pair (g, i): bbox_iou(gt box g, hyp box i) >= iou_threshold as float32 (dt_bbox_iou's bits), and equal labels as floats unless
 *       DT_SCORE_ANY_LABEL is set;
 *   carry-over: g ascending; if g's id has a row with last track id tau >= 0, the lowest unclaimed i whose id is tau is looked up, and if
 *       (g, i) is valid g is matched to i (a correspondence is kept while it is valid, even where a closer hypothesis exists);
 *   the rest: among the unmatched g and unclaimed i the valid pair of the largest IoU is taken repeatedly, compared as float32, ties to the
 *       lowest g, then the lowest i (the order of DT_MATCH_BEST_FIRST);
 *   counts: matches; switches = matched g whose row had tau >= 0 and tau != the matched hypothesis' id; fragments = matched g whose row
 *       had matched > 0 and last appearance matched == 0;
 *   update, in g order: an id without a row gets one appended; when the table is full the box has no memory (no carry-over, never a
 *       switch or fragment, nothing recorded) and overflow is incremented per such box; an id < 0 has no memory either and is not counted
 *       as overflow.  Otherwise present += 1; matched: matched += 1, switches / fragments as counted, last track id = the hypothesis' id,
 *       last appearance matched = 1; unmatched: last appearance matched = 0 and the last track id is kept.  An id that occurs twice or more in
 *       a frame is updated as this walk in g order leaves it: the counters add, its highest g decides last appearance matched, and the
 *       last track id is that of its highest MATCHED g (an unmatched row keeps the id, also one a lower row of the frame has just set).
 *   d_totals  [n_clips, DT_SCORE_INTS] int32      frames, gt boxes, hyp boxes, matches, switches, fragments, overflow, 0
 *             (misses = gt - matches, false positives = hyp - matches)
 *   d_objs    [n_clips, ocap, DT_SCORE_OBJ_INTS] int32, d_nobjs [n_clips] int32 the rows in use
 *   d_fcounts [n_clips, T, 4] int32               gt, hyp, matches, switches of every frame; may be NULL
 *   d_match   [n_clips, T, gcap] int32            the hypothesis row matched to g, -1 for unmatched and unused rows
 *   d_miou    [n_clips, T, gcap] float32          the IoU of that match, 0 elsewhere; d_match and d_miou: both, or both NULL
 * Without DT_SCORE_RESUME d_totals, d_objs, d_nobjs may arrive uninitialised and every word of them is written: the rows of d_objs from
 * d_nobjs on are zero with -1 in the gt id and last track id fields.  With it the three are in-out and the call continues from them:
 * chunks of any sizes along T give every output of the one call on the concatenation, bit for bit -- the contract of the stream entries,
 * with the state owned by the caller (no slot table).  Asynchronous on the context's stream; n_clips = 0 is a no-op.
 * Not done here: an optimal (Hungarian) assignment in the frame step (dt_assign_max is one; IDF1: dt_identity_overlap below; HOTA:
 * dt_hota_align below), ignore regions and visibility weighting, dropping coasting rows.  (Detector AP: dt_detect_match / dt_detect_rank below.)
 * DT_ERR_ARG (nothing launched): a NULL required pointer, n_clips < 0, T, gcap, hcap or ocap <= 0, id_stride < 1, hyp_label_at outside
 * 0..7, unknown flag bits, one of d_match / d_miou without the other, a threshold that is NaN or outside (0, 1], or a table and frame
 * that do not fit the 160 KB of LDS: 8 * ocap + 11 * gcap + 7 * hcap words must not exceed 40960 (gcap = hcap = 128: ocap up to 4832). */
DT_API int dt_track_score(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                 const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                 int n_clips, int T, float iou_threshold, int flags, int ocap,
                 int *d_totals, int *d_objs, int *d_nobjs, int *d_fcounts, int *d_match, float *d_miou);

/* Identity scoring (BUILD-DEFINED, DESIGN.md "Identity scoring"): IDF1 (Ristani et al. 2016) of a tracker's output against ground-truth
 * tracks.  Two entries: the overlap of ground-truth trajectories with hypothesis trajectories over a clip, then an exact one-to-one
 * assignment of maximum weight on it, whose total is IDTP.  IDFN = gt boxes - IDTP, IDFP = hyp boxes - IDTP (the paper's minimum-cost
 * formulation with its dummy nodes removed); IDP = IDTP / hyp, IDR = IDTP / gt, IDF1 = 2 IDTP / (gt + hyp) are taken on the host in float64
 * (Python: utility.evaluate.identity).  No float is summed on the device.
 *
 * dt_identity_overlap: the input arguments, d_gt_boxes .. iou_threshold and flags, are dt_track_score's, bit for bit, DT_SCORE_ANY_LABEL and
 * DT_SCORE_RESUME included -- so an association result and the confirmed-track read-out are scored by the same entry.  Clips are scored
 * independently, one wavefront each, frames in sequence.
 * TRAJECTORIES: a clip has a ground-truth table of at most acap rows, one per distinct ground-truth id >= 0 in order of first appearance
 * (within a frame: row order), and a hypothesis table of at most bcap rows built the same way from the hypothesis ids >= 0; a row holds the
 * id and its number of boxes.  A box whose id is < 0, or whose id finds its table full, has no trajectory: it counts in the box totals and,
 * in the full-table case, in that side's overflow count, and takes no part in the overlap.
 * OVERLAP: n[a][b] = the valid row pairs (g, i) over all frames with g of ground-truth trajectory a and i of hypothesis trajectory b; valid
 * is dt_track_score's definition: bbox_iou(gt box g, hyp box i) >= iou_threshold as float32, and equal labels as floats unless
 * DT_SCORE_ANY_LABEL.  Nothing is claimed and nothing is carried over: every valid pair of a frame counts (with distinct ids inside a
 * frame at most one per frame and trajectory pair; repeated ids add).
 *   d_sizes   [n_clips, DT_IDENT_INTS] int32   frames, gt boxes, hyp boxes, gt trajectories, hyp trajectories, gt overflow boxes, hyp overflow
 *             boxes, valid pairs (those counted into d_overlap: its sum)
 *   d_gt_tab  [n_clips, acap, 2] int32, d_hyp_tab [n_clips, bcap, 2] int32   id, boxes; unused rows are (-1, 0)
 *   d_overlap [n_clips, acap, bcap] int32
 * Without DT_SCORE_RESUME every word of the four is written and the buffers may arrive uninitialised.  With it they are in-out: chunks of
 * any sizes along T give the outputs of one call on the concatenation, bit for bit.  Asynchronous on the context's stream; n_clips = 0 is
 * a no-op.
 * DT_ERR_ARG (nothing launched, nothing written): a NULL pointer, n_clips < 0, T, gcap, hcap, acap or bcap <= 0, id_stride < 1, hyp_label_at
 * outside 0..7, unknown flag bits, a threshold that is NaN or outside (0, 1], n_clips * acap * bcap >= 2^31, or a frame and tables that
 * do not fit the 160 KB of LDS: 2 * acap + 2 * bcap + 7 * gcap + 7 * hcap words must not exceed 40960 (gcap = hcap = 128: acap + bcap up
 * to 19584).
 *
 * dt_assign_max: n independent problems, one wavefront each.  Problem k has rows = d_dims[k * stride + rows_at] and cols = d_dims[k * stride
 * + cols_at], clamped to [0, rcap] and [0, ccap] (d_sizes of dt_identity_overlap is passed as it is, with stride DT_IDENT_INTS, rows_at 3,
 * cols_at 4), and the weights d_w[k][r][c], r < rows, c < cols, of d_w [n, rcap, ccap] int32.  It finds a one-to-one assignment of rows to
 * columns that maximises the sum of the chosen weights, by the shortest-augmenting-path Hungarian method with integer potentials (exact;
 * no float), solved on the orientation whose row count is the smaller.
 *   d_row_to_col [n, rcap] int32, d_col_to_row [n, ccap] int32   the partner, or -1: a pair whose weight is 0 is reported as unassigned, and
 *             so are rows and columns beyond the counts
 *   d_total      [n] int64                                        the sum of the chosen weights (IDTP on an overlap matrix)
 * Every word of the three is written.  Weights must lie in [0, 2^24]; outside that the result is unspecified, but the call still
 * terminates and stays in bounds.  Which of several optimal assignments is reported is fixed by the method as DESIGN.md states it step
 * by step (ties to the lowest column); two runs give identical bits.  Asynchronous on the context's stream; n = 0 is a no-op.
 * DT_ERR_ARG (nothing launched, nothing written): a NULL pointer, n < 0, rcap or ccap <= 0, rows_at or cols_at outside 0..stride-1,
 * n * rcap * ccap >= 2^31, or work arrays that do not fit the 160 KB of LDS: 6 * (max(rcap, ccap) + 1) words must not exceed 40960
 * (caps up to 6825).
 * Not done here: ignore regions.  (HOTA: dt_hota_align, dt_hota_weights, dt_hota_count below, which call this solver per frame; its method is
 * also the tracker's own match in dt_associate_tracks_assign.) */
DT_API int dt_identity_overlap(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                 const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                 int n_clips, int T, float iou_threshold, int flags, int acap, int bcap,
                 int *d_sizes, int *d_gt_tab, int *d_hyp_tab, int *d_overlap);
DT_API int dt_assign_max(dt_ctx *ctx, const int *d_w, int rcap, int ccap, const int *d_dims, int stride, int rows_at, int cols_at, int n,
                 int *d_row_to_col, int *d_col_to_row, int64_t *d_total);

/* HOTA scoring (BUILD-DEFINED, DESIGN.md "HOTA scoring"): HOTA (Luiten et al., IJCV 2021) of a tracker's output against ground-truth
 * tracks, restated on the quantised similarity q = (int)(IoU * 2^20) so that the device sums integers only and every output is
 * independent of the order of any sum.  Three entries, with dt_assign_max between the second and the third; DetA, AssA, HOTA, LocA
 * and their siblings are ratios taken on the host in float64 (Python: utility.evaluate.hota).  S = DT_ASSIGN_IOU_SCALE = 2^20.
 *
 * The input arguments d_gt_boxes .. T of dt_hota_align and dt_hota_weights are dt_track_score's, name for name (there is no IoU threshold
 * here); flags: DT_SCORE_ANY_LABEL, and for dt_hota_align DT_SCORE_RESUME.  Rows, trajectories, the two tables and the overflow counts are
 * dt_identity_overlap's.
 * SIMILARITY of a frame's row pair (g, i): q[g][i] = (int)(bbox_iou(gt box g, hyp box i) * 1048576.0f) (dt_bbox_iou's float32 bits; the
 * product is exact, the conversion truncates), and q = 0 when the labels differ as floats (unless DT_SCORE_ANY_LABEL), when the IoU is
 * NaN or <= 0, or when either row has no trajectory.  Boxes must have w, h >= 0 and be finite (then IoU <= 1, q <= S); a trajectory must
 * have fewer than 2^22 boxes.  Outside that the results are unspecified, but every call terminates and stays in bounds.
 *
 * dt_hota_align (pass 1, one wavefront per clip, frames in sequence): per frame R[g] = sum_i q[g][i] and C[i] = sum_g q[g][i] in int64,
 * and every pair with q > 0 adds c = (q << 20) / (R[g] + C[i] - q) (int64, integer division) to P[a][b] of its trajectories (a, b).  The
 * c of a row, and of a column, add up to S at most, so P[a][b] <= S * min(n_a, n_b) with n the trajectories' box counts, repeated ids
 * included.
 *   d_sizes   [n_clips, DT_IDENT_INTS] int32   dt_identity_overlap's words, word 7 = the pairs with q > 0
 *   d_gt_tab  [n_clips, acap, 2] int32, d_hyp_tab [n_clips, bcap, 2] int32   id, boxes; unused rows are (-1, 0)
 *   d_align   [n_clips, acap, bcap] int64      P
 * Without DT_SCORE_RESUME every word of the four is written.  With it they are in-out: chunks of any sizes along T give the outputs of
 * one call on the concatenation, bit for bit.
 *
 * dt_hota_weights (pass 2, one wavefront per (clip, frame); frames are independent): from the FINISHED d_sizes, d_gt_tab, d_hyp_tab and
 * d_align of the whole clip, W[g][i] = 1 + (P[a][b] * q) / (S * (n_a + n_b) - P[a][b]) (int64, integer division) where q > 0, else 0.
 * The divisor is >= S * max(n_a, n_b) > 0 and W <= S + 1, inside dt_assign_max's [0, 2^24].
 *   d_w       [n_clips, T, gcap, hcap] int32   every word written, 0 outside the frame's counts
 *   d_dims    [n_clips, T, 2] int32            the frame's clamped row counts ng, nh
 *   d_gt_ent  [n_clips, T, gcap] int32, d_hyp_ent [n_clips, T, hcap] int32   the row's trajectory (table row), or -1
 * The frame's match is dt_assign_max's d_row_to_col on d_w as n_clips * T problems [gcap, hcap] with d_dims (stride 2, rows_at 0,
 * cols_at 1): the solver is called unchanged, so its orientation and tie rules apply, and pairs of weight 0 are unassigned.
 *
 * dt_hota_count (one wavefront per (clip, frame)): h_thresholds [n_thr] on the HOST, 1 <= n_thr <= DT_HOTA_MAX_THR, each in (0, 1],
 * strictly ascending.  A matched pair's level L is the number of k with IoU >= h_thresholds[k], compared as float32 (the IoU is the call
 * whose product gave q).  A pair of level L >= 1 adds, in bucket L - 1: 1 to tp, q to loc, 1 to pairs[a][b].  A pair that passes
 * threshold k passes every lower one: the figures at threshold k are the sums over the buckets k .. n_thr - 1, taken on the host.
 *   d_tp      [n_clips, n_thr] int32, d_loc [n_clips, n_thr] int64, d_pairs [n_clips, n_thr, acap, bcap] int32
 * flags: 0, or DT_SCORE_RESUME: the three are in-out and the call adds to them (the chunks of a clip, each with its own d_dims ..
 * d_row_to_col); without it every word is written.  Rows whose d_row_to_col, d_gt_ent or d_hyp_ent lies outside its range are skipped.
 *
 * All three are asynchronous on the context's stream; n_clips = 0 is a no-op.  A clip fed in chunks takes two loops over the chunks:
 * dt_hota_align with DT_SCORE_RESUME over all of them first, then dt_hota_weights, dt_assign_max and dt_hota_count (DT_SCORE_RESUME) per chunk.
 * Not done here: ignore regions, visibility weighting, per-class breakdowns (the caller filters by label).
 * DT_ERR_ARG (nothing launched, nothing written): a NULL pointer, n_clips < 0, T, gcap, hcap, acap or bcap <= 0, id_stride < 1, hyp_label_at
 * outside 0..7, unknown flag bits, n_thr outside 1..32, a threshold that is NaN, outside (0, 1] or not above its predecessor,
 * n_clips * acap * bcap (align, weights), n_clips * T * gcap * hcap (weights), n_clips * n_thr * acap * bcap, n_clips * T * gcap or
 * n_clips * T * hcap (count) >= 2^31, or a frame and tables that do not fit the 160 KB of LDS: 2 * acap + 2 * bcap + 9 * gcap + 9 * hcap
 * words (align; the int64 R and C beside dt_identity_overlap's rows) or 2 * acap + 2 * bcap + 7 * gcap + 7 * hcap words (weights) must not
 * exceed 40960. */
DT_API int dt_hota_align(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                 const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                 int n_clips, int T, int flags, int acap, int bcap,
                 int *d_sizes, int *d_gt_tab, int *d_hyp_tab, int64_t *d_align);
DT_API int dt_hota_weights(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                 const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                 int n_clips, int T, int flags, int acap, int bcap,
                 const int *d_sizes, const int *d_gt_tab, const int *d_hyp_tab, const int64_t *d_align,
                 int *d_w, int *d_dims, int *d_gt_ent, int *d_hyp_ent);
DT_API int dt_hota_count(dt_ctx *ctx, const float *d_gt_boxes, int gcap, const float *d_hyp_boxes, int hcap, int n_clips, int T,
                 const int *d_dims, const int *d_gt_ent, const int *d_hyp_ent, const int *d_row_to_col,
                 const float *h_thresholds, int n_thr, int acap, int bcap, int flags,
                 int *d_tp, int64_t *d_loc, int *d_pairs);

/* Detection scoring (BUILD-DEFINED, DESIGN.md "Detection scoring"): per-class average precision of a detector's boxes against ground truth,
 * by the VOC devkit's match.  Two entries: the match of every frame, then the position of every detection in its class's score order over
 * the whole set.  Both give integers (and the IoU of the match); precision, recall and AP are taken from them on the host, in float64
 * (Python: utility.evaluate.average_precision).  No float is summed on the device.
 *   d_det_boxes [B, cap, DT_BOX_FLOATS]   x, y, w, h in floats 0..3, the label in float 5, the ranking score in float score_at (6: dt_decode's
 *               score, 4: its conf); d_det_counts [B] int32; rows i < min(count, cap) take part (a negative count reads as 0)
 *   d_gt_boxes  [B, gcap, DT_BOX_FLOATS]  x, y, w, h, the label in float 5; d_gt_counts [B]; rows g < min(count, gcap) take part
 *   d_gt_flags  [B, gcap] int32, bit 0 = ignore (VOC "difficult", MOT distractors); NULL: no row is ignored
 *   h_thresholds[n_thr] on the HOST, 1 <= n_thr <= 16, each in (0, 1]: one call gives COCO's .50:.05:.95
 * A row takes part only if its label l is an integer value with 0 <= l < NC.  Boxes and scores must be finite (and so must the areas
 * w * h).  Two boxes without area have the IoU 0 / 0 = NaN: the tests below are written as the kernel makes them, so a NaN is never the
 * larger IoU and is below no threshold.
 * MATCH, per frame, independent of other frames:
 *   1. the candidates of detection i are all ground-truth rows of equal label (as floats), claimed and ignored rows too; best[i] is the
 *      candidate of the largest bbox_iou(gt g, det i) as float32 (dt_bbox_iou's bits), ties to the lowest g, and iou[i] that IoU; without a
 *      candidate best = -1 and iou = 0.  Neither depends on the threshold.
 *   2. per threshold k the frame's detections are walked by descending score (float32, ties to the lower row):
 *      best < 0 or iou < thr[k]: FP (state 0); else best is an ignore row: ignored (state 2), nothing is claimed; else best is unclaimed at
 *      k: TP (state 1), and it is claimed; else FP (a duplicate -- no second-best row is looked for).
 *   d_state [n_thr, B, cap] int32   1 TP, 0 FP, 2 ignored, -1 in rows that take no part (beyond the count, or a label outside 0..NC-1)
 *   d_best  [B, cap] int32, d_iou [B, cap] float32   -1 and 0 in rows that take no part
 * RANK, over all B frames, per threshold k and label c: the detections of label c with state 0 or 1 at k, by descending score, ties to
 * the lower flat index b * cap + i.
 *   d_rank  [n_thr, B, cap] int32   the detection's position in that order, from 0; -1 for ignored and unused rows
 *   d_ctp   [n_thr, B, cap] int32   the TPs at positions <= its own; -1 likewise
 *   d_ngt   [NC] int32              ground-truth rows of label c without the ignore bit
 *   d_ndet, d_ntp [n_thr, NC] int32 the ranked detections, and the TPs among them
 * Every word of every output is written; the buffers may arrive uninitialised.  Asynchronous on the context's stream.  B = 0 launches no
 * match and the rank writes the totals as zeros; the per-frame arrays, which are empty then, are not looked at and may be NULL.
 * CHUNK CONTRACT: the match is per frame, so the match outputs of chunks of frames, concatenated along B (d_state along its second axis),
 * are the outputs of one call on the concatenation; the rank runs once over the concatenation (it needs every score of a class).
 * The match runs one 64-lane workgroup per frame with the frame in LDS: 3 * cap + 6 * gcap words must not exceed 40960 (160 KB;
 * cap = gcap = 1024 uses 9216).  The rank compacts the rows in use first (a prefix sum over min(count, cap)) and compares each with
 * every other such row: its work grows with (rows in use)^2, not (B * cap)^2; it keeps 16 bytes per row of [B, cap] in a workspace.
 * Not done here, on purpose: COCO's match (best UNCLAIMED row, crowd regions), area ranges and max-detections cuts, per-class score
 * thresholds, label-free AP.
 * DT_ERR_ARG (nothing launched, no output written): a NULL required pointer, B < 0, cap, gcap or NC <= 0, n_thr outside 1..16, a
 * threshold that is NaN or outside (0, 1], score_at outside 0..7, B * cap or B * gcap >= 2^31, or (match) the LDS bound above. */
DT_API int dt_detect_match(dt_ctx *ctx, const float *d_det_boxes, const int *d_det_counts, int cap, int score_at,
                 const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_flags, int gcap,
                 int B, int NC, const float *h_thresholds, int n_thr,
                 int *d_state, int *d_best, float *d_iou);
DT_API int dt_detect_rank(dt_ctx *ctx, const float *d_det_boxes, const int *d_det_counts, int cap, int score_at, const int *d_state,
                 const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_flags, int gcap,
                 int B, int NC, int n_thr,
                 int *d_rank, int *d_ctp, int *d_ngt, int *d_ndet, int *d_ntp);

/* ---- streaming: ConvLSTM state and track ids carried across calls (addition; the reference's predict() sees one window) ---- *
 * A live stream delivers a frame, or a few, at a time.  The context holds a table of STREAM SLOTS in device memory; per slot the ConvLSTM
 * state h, c [G*G][U], the track table (the last frame's boxes first, then lost tracks: boxes [tcap][8], ids and ages [tcap]; tcap = cap unless
 * dt_stream_open_tracks says otherwise), the next free track id, and counters of frames seen.
 * Contract: a stream fed in chunks of any sizes gives what the stateless calls give on the concatenation of those chunks as one clip.
 * A FRESH slot (after dt_stream_open / dt_stream_reset, and after dt_tracker_load, dt_load_darknet_weights or dt_detector_config, which make
 * every slot fresh -- a load that changes the state's shape closes the table) is indistinguishable from a stateless call.
 * h_slots is a HOST array of n DISTINCT slot numbers in [0, n_slots) (else DT_ERR_ARG; DT_ERR_STATE before dt_stream_open): stream i of the
 * call lives in slot h_slots[i].  The array is consumed before the call returns; the streams of a call need not be in step.
 *
 * dt_stream_open: (re)allocates the table, every slot fresh; needs a loaded tracker.  cap = box capacity of the association state.
 * dt_stream_reset: the listed slots fresh again (zero state, ids from 0); h_slots == NULL: all of them.  Stream-ordered, no host wait. */
DT_API int dt_stream_open(dt_ctx *ctx, int n_slots, int cap);
/* dt_stream_open with a track table of tcap >= cap entries per slot (boxes [tcap][8], ids [tcap], ages [tcap]) for dt_associate_stream_mem;
 * dt_stream_open(ctx, n, cap) is dt_stream_open_tracks(ctx, n, cap, cap).  DT_ERR_ARG: tcap < cap or tcap > 65535. */
DT_API int dt_stream_open_tracks(dt_ctx *ctx, int n_slots, int cap, int tcap);
DT_API int dt_stream_reset(dt_ctx *ctx, const int *h_slots, int n);
/* dt_track_forward on d_frames [n, T, H, W, 3]: stream i starts from the state in slot h_slots[i] and leaves its state after frame T-1
 * there.  d_trk / d_det as dt_track_forward.  When any slot of the call is warm, t = 0 is a full recurrent step (the form steps t >= 1 take). */
DT_API int dt_track_stream_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n, int T, const int *h_slots,
                            float *d_trk, float *d_det);
/* dt_associate on d_boxes [n,T,cap,8], d_counts [n,T]: frame 0 of stream i is matched against the slot's stored last frame, new ids
 * continue from the slot's counter, d_nids[i] = ids the stream has opened since its reset; the slot then holds frame T-1.  cap must be
 * the table's (DT_ERR_ARG). */
DT_API int dt_associate_stream(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, const int *h_slots, int *d_ids, int *d_nids);
/* dt_associate_mem for streams: the slot's track table is the table frame 0 is matched against, and the table after frame T-1 goes back
 * to the slot.  Chunks of any sizes with one max_age give what dt_associate_mem gives on the concatenation with tcap = the table's.
 * max_age belongs to the call: a call with a smaller one ignores older entries, and they leave the table at the end of its first frame.
 * dt_associate_stream on any table is this entry with max_age = 0; the two may be mixed on one slot.  Errors as dt_associate_stream, and
 * DT_ERR_ARG for max_age < 0; an error leaves the slots as they were. */
DT_API int dt_associate_stream_mem(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, const int *h_slots, int *d_ids, int *d_nids, int *d_gaps);
/* dt_associate_motion for streams: the slot's track table, with a velocity per entry (a further [tcap][2] floats per slot), is the table
 * frame 0 is matched against, and table and velocities after frame T-1 go back to the slot.  Chunks of any sizes with one max_age and
 * one gain give what dt_associate_motion gives on the concatenation with tcap = the table's, bit for bit.  The three stream association
 * entries may be mixed on one slot: a call of dt_associate_stream or dt_associate_stream_mem makes the slot's tracks forget their
 * velocities (the next motion call finds every track at rest); ids, boxes and ages carry over as between those two.  A fresh or reset
 * slot has an empty table.  Errors as dt_associate_stream_mem, and DT_ERR_ARG for gain outside [0, 1] or NaN or a table whose 9-word
 * entries do not fit the LDS; an error leaves the slots as they were. */
DT_API int dt_associate_stream_motion(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, float gain, const int *h_slots, int *d_ids, int *d_nids, int *d_gaps);
/* dt_associate_tracks for streams: the slot's table carries velocities and hit counts (a further [tcap] int32 per slot).  Chunks of any
 * sizes with one max_age, one gain and one min_hits give every output of dt_associate_tracks on the concatenation with tcap = the
 * table's, bit for bit (d_tracks / d_tinfo rows have the table's tcap).  Mixed with the other stream association entries on one slot:
 * after dt_associate_stream_motion the velocities carry over and every track reads as hits = 1; after dt_associate_stream or
 * dt_associate_stream_mem the velocities are forgotten too.  Errors as dt_associate_stream_motion, and DT_ERR_ARG for min_hits < 1, a
 * partial read-out triple or a table whose 10-word entries do not fit the LDS; an error leaves the slots as they were. */
DT_API int dt_associate_stream_tracks(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, float gain, int min_hits, const int *h_slots, int *d_ids, int *d_nids, int *d_gaps,
                        int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* dt_associate_tracks_match for streams: dt_associate_stream_tracks with the match policy of the call; match = 0 is that entry bit for
 * bit.  The policy leaves nothing in the slot and the slot layout is dt_associate_stream_tracks': calls with different match values may
 * follow each other on one slot, and chunks of any sizes give what dt_associate_tracks_match gives on the concatenation when every
 * chunk uses the same match.  Errors as dt_associate_stream_tracks, and DT_ERR_ARG for match outside 0..3 or, with DT_MATCH_BEST_FIRST,
 * a table that does not fit the LDS beside the order's three words per box; an error leaves the slots as they were. */
DT_API int dt_associate_stream_tracks_match(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, float gain, int min_hits, int match, const int *h_slots, int *d_ids, int *d_nids,
                        int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* dt_associate_tracks_assign for streams: dt_associate_stream_tracks with the optimal assignment as the match of every frame; match is
 * 0 or DT_MATCH_ANY_LABEL.  The policy leaves nothing in the slot and the slot layout is dt_associate_stream_tracks': calls of any
 * association entry may follow each other on one slot, exactly as dt_associate_stream_tracks_match documents, and chunks of any sizes
 * give what dt_associate_tracks_assign gives on the concatenation with tcap = the table's.  Errors as dt_associate_stream_tracks, and
 * DT_ERR_ARG for any other match or a table beyond 26 * tcap + 4 * cap + 6 <= 40960 words (refused before the slot list is written);
 * an error leaves the slots as they were. */
DT_API int dt_associate_stream_tracks_assign(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, float gain, int min_hits, int match, const int *h_slots, int *d_ids, int *d_nids,
                        int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);
/* dt_associate_tracks_scored for streams: dt_associate_stream_tracks_assign with the two passes by score as the match of every frame.
 * The slot layout is dt_associate_stream_tracks'; chunks of any sizes give what dt_associate_tracks_scored gives on the concatenation
 * with tcap = the table's.  After a call the slot's leading rows may hold DEAD rows (id -1, hits 0: the last frame's dropped boxes).
 * Calls of any association entry may still follow each other on one slot: every entry's candidate test asks for an id >= 0, so a dead
 * row is matched by none of them and leaves the table at the end of the next call's first frame.  Errors as
 * dt_associate_stream_tracks_assign, and DT_ERR_ARG for score_at outside 0..7, a NaN score_high, score_new or thr_low, max_age_low < -1
 * or a table beyond 26 * tcap + 5 * cap + 6 <= 40960 words (refused before the slot list is written); an error leaves the slots as
 * they were. */
DT_API int dt_associate_stream_tracks_scored(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                        float thr, int max_age, float gain, int min_hits, int match,
                        int score_at, float score_high, float score_new, float thr_low, int max_age_low,
                        const int *h_slots, int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts);

/* ---- cross-stream detection exchange (multi-GPU; the reference has no counterpart) ---- *
 * north_star: "RCCL all-gather of detections over xGMI only for cross-stream association".  Each rank packs its
 * detection table (the outputs of dt_decode + dt_associate for its clips) into ONE int32 row per clip,
 *     row = [ boxes T*cap*8 (float bits) | ids T*cap | counts T | nids | valid ],   dt_packed_row_ints(T, cap) ints,
 * padded with empty rows (valid = 0) to n_rows = the largest clip count of any rank, so that the exchange is ONE
 * fixed-size all-gather per step (the caller's collective: ncclAllGather / torch.distributed on d_rows, n_rows *
 * row ints per rank).  dt_unpack_detections compacts the gathered rows of all ranks (rank-major = global clip order)
 * back into tables and makes the per-clip track ids globally unique: gid = id + sum of nids of all earlier clips.
 *   dt_pack_detections:   d_boxes [n_clips,T,cap,8], d_counts [n_clips,T], d_ids [n_clips,T,cap], d_nids [n_clips]
 *                         -> d_rows [n_rows, row] int32          (n_rows >= n_clips; n_clips may be 0)
 *   dt_unpack_detections: d_rows [n_rows, row] -> d_boxes/d_counts/d_ids/d_nids sized for n_rows clips (the first
 *                         *d_n_valid are filled), d_gids [n_rows,T,cap] int64 (may be NULL), d_n_valid [1] int32 */
DT_API size_t dt_packed_row_ints(int T, int cap);
DT_API int dt_pack_detections(dt_ctx *ctx, const float *d_boxes, const int *d_counts, const int *d_ids,
                       const int *d_nids, int n_clips, int T, int cap, int n_rows, int32_t *d_rows);
DT_API int dt_unpack_detections(dt_ctx *ctx, const int32_t *d_rows, int n_rows, int T, int cap, float *d_boxes,
                         int *d_counts, int *d_ids, int *d_nids, int64_t *d_gids, int *d_n_valid);

/* ---- TinyTracker (models_tracking/TinyTracker.py:25-41) ---------------- */
/* Also serves TinyHeatmapTracker (models_tracking/TinyHeatmapTracker.py:26-48): same
 * graph with a heatmap_size^2-wide detection input and Dense(heatmap_size^2, sigmoid).
 *   h_kernel [D,4U], h_recurrent [U,4U], h_bias [4U], h_dense_kernel [U,out_dim],
 *   h_dense_bias [out_dim]; D = pooled feature width + detection input width
 *   (4 or heatmap_size^2); out_dim = 4 or heatmap_size^2.  pool: 0 = 'Global', 1 = 'Max'. */
DT_API int dt_tiny_load(dt_ctx *ctx, int D, int units, int out_dim, const float *h_kernel,
                 const float *h_recurrent, const float *h_bias,
                 const float *h_dense_kernel, const float *h_dense_bias);

/* Replaces model_tracker.predict([img_fv, det]).
 *   d_feat [n_seq, T, fh, fw, fc], d_det [n_seq, T, D - feature width] -> d_out [n_seq, T, out_dim] */
DT_API int dt_tiny_forward(dt_ctx *ctx, const float *d_feat, const float *d_det,
                    int n_seq, int T, int fh, int fw, int fc, int pool,
                    float *d_out);

/* The two halves of dt_tiny_forward, exposed so that a frame-sharded deployment
 * (BASELINE.json configs[3]) can all-gather the small per-frame rows between them:
 *   dt_tiny_features: pool + concatenate([feat, det]) -> d_x [n_rows, D]   (TinyTracker.py:29-34)
 *   dt_tiny_sequence: d_x [n_seq, T, D] -> LSTM over T -> Dense -> d_out [n_seq, T, 4]  (:36-37) */
DT_API int dt_tiny_features(dt_ctx *ctx, const float *d_feat, const float *d_det, int n_rows,
                     int fh, int fw, int fc, int pool, float *d_x);
DT_API int dt_tiny_sequence(dt_ctx *ctx, const float *d_x, int n_seq, int T, float *d_out);

/* ---- streaming single-object trackers: the LSTM state h, c [U] carried across calls (addition; the contract of the stream block above) ---- *
 * A table of TINY STREAM SLOTS, apart from dt_stream_open's (a context may hold both; neither touches the other): per slot h (two copies,
 * used alternately), c and a counter of frames seen.  A tiny stream fed in chunks of any sizes gives what dt_tiny_sequence / dt_tiny_forward
 * give on the concatenation of those chunks as one sequence, bit for bit; a FRESH slot (after dt_tiny_stream_open / dt_tiny_stream_reset, and
 * after dt_tiny_load, which makes every slot fresh before it replaces a weight) is indistinguishable from a stateless call.
 * h_slots: a HOST array of n DISTINCT numbers in [0, n_slots), consumed before the call returns; sequence i of the call lives in slot
 * h_slots[i].  The streams of a call need not be in step; fresh and warm slots may be mixed in one call.
 * DT_ERR_STATE: before dt_tiny_load or before dt_tiny_stream_open (a load for other units would close the table; units is 512 today, so
 * no load does).  DT_ERR_ARG: a duplicate or out-of-range
 * slot, n <= 0, T <= 0, n_slots <= 0.  An error leaves every slot as it was.
 *   dt_tiny_stream_open:     (re)allocates the table, every slot fresh; needs loaded weights
 *   dt_tiny_stream_reset:    the listed slots fresh again; h_slots == NULL: all of them.  Stream-ordered, no host wait
 *   dt_tiny_stream_sequence: dt_tiny_sequence on d_x [n, T, D], sequence i continuing from -- and leaving its state in -- slot h_slots[i]
 *   dt_tiny_stream_forward:  dt_tiny_features followed by dt_tiny_stream_sequence (arguments as dt_tiny_forward) */
DT_API int dt_tiny_stream_open(dt_ctx *ctx, int n_slots);
DT_API int dt_tiny_stream_reset(dt_ctx *ctx, const int *h_slots, int n);          /* h_slots == NULL: all */
DT_API int dt_tiny_stream_sequence(dt_ctx *ctx, const float *d_x, int n, int T, const int *h_slots, float *d_out);
DT_API int dt_tiny_stream_forward(dt_ctx *ctx, const float *d_feat, const float *d_det, int n, int T,
                                  int fh, int fw, int fc, int pool, const int *h_slots, float *d_out);

/* generate_heatmap_feat (utility/utils.py:53-58) applied as the data generator does
 * (preprocessing.py:455): d_box4 [n,4] centre-format (cx,cy,w,h) -> d_heat [n, hs*hs] of 0/1.
 * generate_rectangle_from_heatmap (utility/utils.py:61-79): d_heat [n, hs*hs] ->
 * d_rect [n,4] int32 (x1,y1,x2,y2), (hs,hs,-1,-1) when no cell reaches thresh. */
DT_API int dt_heatmap_from_boxes(dt_ctx *ctx, const float *d_box4, int n, int hmap_size, float *d_heat);
/* same with the function's own argument list: d_xywh [n,4] float64 (det_x, det_y, det_w, det_h) */
DT_API int dt_heatmap_from_xywh64(dt_ctx *ctx, const double *d_xywh, int n, int hmap_size, float *d_heat);
DT_API int dt_rect_from_heatmap(dt_ctx *ctx, const float *d_heat, int n, int hmap_size, float thresh,
                         int *d_rect);

/* Detection box handed to the single-object tracker at inference (build-defined:
 * the reference only has the training-time choice, preprocessing.py:421-456):
 * highest-score survivor per frame as (cx,cy,w,h), zeros when a frame has none.
 *   d_boxes [n_frames, cap, 8], d_counts [n_frames] -> d_out4 [n_frames, 4] */
DT_API int dt_top_box(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_frames,
               int cap, float *d_out4);

/* ---- training-target encoding (the step before the path when fine-tuning) ----
 * Replaces the object-coordinate fix at the end of BaseBatchGenerator.aug_image
 * (utility/preprocessing.py:171-188) + BatchGenerator.output_from_instance's y / b construction
 * (:214-293).  float64 like the reference's Python floats; bit-exact.
 *   d_objs   [n_frames, cap, 5] int32   xmin, ymin, xmax, ymax, LABELS index (-1: name not in LABELS)
 *   d_counts [n_frames] int32           objects per frame
 *   d_dims   [n_frames, 2] int32        original image (width, height)
 *   d_aug    [n_frames, 4] float64      the augmentation draw (scale, offx, offy, flip) of
 *                                       aug_image :150-166, or NULL for augment=False
 *   h_anchors [2*nb_box] float64 (host) ANCHORS
 *   d_y [n_frames, grid_h, grid_w, nb_box, 5+nb_class] float64, d_b [n_frames, true_box_buffer, 4] float64
 *   (b is the reference's (1,1,1,TRUE_BOX_BUFFER,4) block without the unit axes) */
DT_API int dt_encode_targets(dt_ctx *ctx, const int *d_objs, const int *d_counts, const int *d_dims,
                      const double *d_aug, int n_frames, int cap, int grid_h, int grid_w, int nb_box,
                      int nb_class, int image_h, int image_w, int true_box_buffer,
                      const double *h_anchors, double *d_y, double *d_b);

/* ---- hipGraph replay (low-latency serving; default off) ---------------- *
 * With graphs on, the launch-bound inner sequences that only touch library-owned buffers -- the detector
 * trunk conv_2..conv_21 and the ConvLSTM recurrence -- are captured once per shape (on the second call
 * with that shape) and replayed with hipGraphLaunch on an internal stream that is ordered after and
 * before the caller's stream with events.  Results are identical.  Graphs are dropped when weights are
 * reloaded or a workspace grows; profiling (dt_profile_enable) bypasses them. */
DT_API int dt_graph_enable(dt_ctx *ctx, int on);

/* ---- layer-level entry points (used by the parity tests) --------------- */
/* Conv2D 'same' stride 1 (+ optional folded bias, LeakyReLU slope, fused 2x2
 * maxpool) through the MFMA implicit-GEMM kernel.  h_kernel is Keras HWIO
 * [k,k,Cin,Cout]; Cin must be a multiple of 32 (use dt_conv1 for RGB input).
 *   pool: 0 none, 1 pooled output only, 2 both (d_out unpooled, d_out2 pooled) */
DT_API int dt_conv2d(dt_ctx *ctx, const float *d_in, int B, int H, int W, int Cin,
              const float *h_kernel, int k, int Cout, const float *h_bias,
              float leaky_slope, int pool, float *d_out, float *d_out2);

/* One ConvLSTM2D step (MultiObjDetTracker.py:176): d_x [B,H,W,Cx] with Cx a
 * multiple of 32, d_h/d_c [B,H,W,U] -> d_h_out/d_c_out. */
DT_API int dt_convlstm_step(dt_ctx *ctx, const float *d_x, int B, int H, int W, int Cx,
                     const float *d_h, const float *d_c, int U,
                     const float *h_kernel, const float *h_recurrent,
                     const float *h_bias, float *d_h_out, float *d_c_out);

/* The split-bf16 batched GEMM of the F(6x6,3x3) / F(4x4,3x3) layers (wino_gemm_s3.hip) on the caller's fp32 operands --
 * the contraction over input channels that models_detection/KerasYOLO.py:351-396 (conv_14 .. conv_22) and
 * models_tracking/MultiObjDetTracker.py:176 (both ConvLSTM2D convolutions) become in Winograd form -- so that the parity
 * tests can check the kernel against float64 AT THE SHAPES bench.py runs (P = 64, Mt = 7840, K = 1024 / 1280, ...):
 *   d_v [P][Mt][K], d_u [P][N][K] float32  ->  d_m [P][Mt][N] = sum_k v * u     (K % 32 == 0, N % 128 == 0)
 * Both operands are split into three bf16 terms on the device by the production pack kernel, then the production
 * launcher runs.  half: 0 = the launcher's own choice of row tile, 1 = 128-row tiles (two workgroups per CU), -1 = 256;
 * 2 = the 1x1 layers' form (P = 1): d_v is read as fp32 rows by the kernel itself, which splits its A fragments in registers. */
DT_API int dt_gemm_split_bf16(dt_ctx *ctx, const float *d_v, const float *d_u, int P, int Mt, int K, int N, int half,
                              float *d_m);
/* The same with the operand form chosen: nt = 3 -- three bf16 terms, six partial products per multiply (dt_gemm_split_bf16);
 * nt = 2 -- the fp16 form the library runs by default since round 6: each operand scaled by a power of two from its measured
 * max |x| (d_v as ONE tensor, like an activation; d_u per plane p, like the Winograd-domain weights) and carried as two fp16
 * terms hi + lo, three partial products lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_f16, the fp32 accumulator scaled back
 * in the epilogue (P <= 64). */
DT_API int dt_gemm_split(dt_ctx *ctx, const float *d_v, const float *d_u, int P, int Mt, int K, int N, int half, int nt,
                         float *d_m);

/* The Winograd transforms ALONE (csrc/winograd.hip), without the GEMM between them: the production tile geometry (frame mosaics under
 * the context's DT_WINO_MOSAIC policy included) and the production launchers on caller data.  ts = 2, 4 or 6.
 * h_geom[DT_WINO_GEOM_INTS] receives g, ph, pw, th, tw, Mt, Mp (g x g frames per virtual image at pitch ph / pw, th x tw tiles of ts x ts
 * outputs on it, Mt tiles in all, Mp = Mt rounded up to 256) and then WHICH KERNEL the launcher chose, with what grid: form (input:
 * DT_WIN_*, output: DT_WOUT_*), workgroups, threads per workgroup.  dt_wino_geometry fills the first seven alone (pooled != 0: the
 * geometry of a launch that pools -- an even pitch). */
#define DT_WINO_GEOM_INTS 10
enum { DT_WIN_TPI2 = 1, DT_WIN_TPI4, DT_WIN_TPI6, DT_WIN_TPI4_S3, DT_WIN_COOP6, DT_WIN_S3_6, DT_WIN_S3_4, DT_WIN_H2_6, DT_WIN_H2_4 };
enum { DT_WOUT_TPI6 = 1, DT_WOUT_TPI4, DT_WOUT_TPI2, DT_WOUT_COOP6, DT_WOUT_GATES6, DT_WOUT_GATES4, DT_WOUT_GATES2 };
DT_API int dt_wino_geometry(dt_ctx *ctx, int ts, int B, int H, int W, int pooled, int *h_geom);
/* Input transform Bt d B of d_in [B][H][W][in_ld >= C] (frame stride in_bs floats) into d_v (v_bytes bytes), in the form nt:
 *   0: float32 V [P][Mt][C], P = (ts+2)^2, position p = (ts+2) xi + nu;
 *   3: three bf16 terms [P][3][C/16][Mp][16] (16-bit words; ts = 6: C % 32 == 0, ts = 4: C % 16 == 0);
 *   2: two fp16 terms [P][2][C/16][Mp][16] of V[p] * 2^(14 - floor(log2 max|d_in|)) * rowfac[xi] * rowfac[nu] as the split GEMM reads them
 *      (ts = 4 / 6, C % 32 == 0, dense frames); max |d_in| is measured into max-|x| slot 57.
 * Rows Mt .. Mp-1 of the split layouts are not written.  force_form (fp32, ts = 6: 1 = one thread per item, 2 = lane-cooperative) and wg_cap
 * (> 0: at most so many workgroups) are WinoArgs' test-only fields; 0 = what production launches.  DT_ERR_ARG for what the launcher refuses. */
DT_API int dt_wino_input(dt_ctx *ctx, const float *d_in, int B, int H, int W, int C, int in_ld, long long in_bs, int ts, int pooled, int nt,
                         int force_form, int wg_cap, void *d_v, long long v_bytes, int *h_geom);
/* Output transform At m A of d_m [P][Mt][m_ld >= N] (m_floats floats) for the geometry of (B, H, W, ts, d_out2 != null):
 *   plain form: + d_bias [N] (or null), + d_bias16 [16][N] border corrections (or null; slope 1, d_out only), LeakyReLU(slope), to
 *     d_out [B][H][W][out_ld >= N] and / or its 2x2 max-pooled d_out2 [B][H/2][W/2][out2_ld >= N] (either may be null); publish != 0: max |x| of
 *     the stored values (the pooled ones where d_out2 is set) into max-|x| slot 57, zeroed first (dt_amax_read);
 *   gate form (d_cstate != null; N = 4 U, columns [j/32][gate][j%32], N % 128 == 0): z = transform + d_xproj [B][H][W][xp_ld >= N], the ConvLSTM2D
 *     update of d_cstate [B][H][W][c_ld >= U] in place, h to d_out [B][H][W][out_ld >= U].
 * force_form (ts = 6, plain form), wg_cap, h_geom and errors as for dt_wino_input. */
DT_API int dt_wino_output(dt_ctx *ctx, const float *d_m, long long m_floats, int m_ld, int N, int B, int H, int W, int ts, const float *d_bias,
                          const float *d_bias16, float slope, float *d_out, int out_ld, float *d_out2, int out2_ld, int publish,
                          const float *d_xproj, int xp_ld, float *d_cstate, int c_ld, int force_form, int wg_cap, int *h_geom);

/* The fp32 implicit-GEMM kernel ALONE (csrc/conv_igemm.hip) on caller views with strides: no policy, no kernel-form choice, the tile
 * configuration `cfg` handed straight to the production launcher (tests/test_gpu_conv_igemm_edges.py).
 *   layer mode (P <= 1): d_in [B][H][W][in_ld >= Cin] with frames in_bs >= H*W*in_ld floats apart (1x1 plain / gates / split-K: dense frames,
 *     as the launcher demands), h_kernel Keras HWIO [ks][ks][Cin][N] and h_bias [N] or null, packed and padded as a loaded layer's are
 *     (npad = 0: N rounded up to 256; else the weight rows to allocate, a multiple of 128 >= N -- what the 256x256 fallback looks at);
 *   batched-GEMM mode (P > 1, ks = 1, kind plain, H = 1, W = Mt): d_in [P][Mt][Cin] and d_wt [P][N][Cin] device operands, d_out [P][Mt][out_ld],
 *     no bias -- the Winograd GEMMs' launch.
 *   kind: DT_CONV_PLAIN  d_out [B*H*W][out_ld >= N];  DT_CONV_POOL  d_out [B*H/2*W/2][out_ld >= N] 2x2 max;  DT_CONV_POOL_BOTH (ks 3)  d_out
 *     unpooled and d_out2 [..][out2_ld >= N] pooled;  DT_CONV_S2D (ks 1)  d_out [B*H/2*W/2][out_ld >= 4 N] tf.space_to_depth(2);
 *     DT_CONV_GATES  N = 4 U Keras gate columns (i, f, c, o), no bias: z = conv + d_xproj [B*H*W][xp_ld >= N] in PACKED column order
 *     [j/32][gate][j%32], d_cstate [B*H*W][c_ld >= U] updated in place, h to d_out [B*H*W][out_ld >= U];
 *     DT_CONV_PARTIAL or ksplit > 1 (plain only): split-K partial sums over ksplit <= ks*ks*Cin/32 ranges into a slab, then the reduce kernel
 *     (bias, LeakyReLU) into d_out.
 *   slope: LeakyReLU slope (1 = linear); act: 1 = sigmoid instead; publish != 0: max |x| of the stored values (the pooled ones where the kind
 *     pools) into max-|x| slot 57, zeroed first; wg_cap > 0: a persistent launch uses at most so many workgroups (ConvArgs' test-only field).
 * h_info[DT_CONV_INFO_INTS] receives what ran: the resolved tile configuration (DT_CFG_*), BM, BN, threads per workgroup, 1 if the instance is
 * the persistent one, grid x, grid y, tiles in all.  DT_ERR_ARG, and no launch, for what the launcher refuses. */
#define DT_CONV_INFO_INTS 8
enum { DT_CONV_PLAIN = 0, DT_CONV_POOL, DT_CONV_POOL_BOTH, DT_CONV_S2D, DT_CONV_GATES, DT_CONV_PARTIAL };
enum { DT_CFG_128x128 = 0, DT_CFG_128x64, DT_CFG_256x128, DT_CFG_256x256, DT_CFG_64x128 };
typedef struct dt_conv_igemm_desc {
    int32_t ks, B, H, W, Cin, N, P, in_ld;
    int64_t in_bs;
    int32_t npad, kind, cfg, ksplit, act, publish, wg_cap;
    float slope;
    int32_t out_ld, out2_ld, xp_ld, c_ld;
} dt_conv_igemm_desc;
DT_API int dt_conv_igemm(dt_ctx *ctx, const dt_conv_igemm_desc *desc, const float *d_in, const float *h_kernel, const float *h_bias, const float *d_wt,
                         float *d_out, float *d_out2, const float *d_xproj, float *d_cstate, int *h_info);

/* conv_1's direct kernels ALONE (csrc/conv1.hip: x/255, Conv2D(32,(3,3),'same') on RGB, bias, LeakyReLU, 2x2 max) through the production
 * launcher, with no detector configured (tests/test_gpu_conv1_edges.py).
 *   d_frames [B][H][W][3], DT_FRAMES_U8 (ANY byte address) or DT_FRAMES_F32 (already normalised; 4-byte aligned); H and W even, B in 1..65535;
 *   h_w [27][32], row k = 9 ky + 3 kx + ci, the BatchNorm scale already folded in; h_bias [32]; slope >= 0: LeakyReLU slope (1 = linear);
 *   split: 1 = the two three-term bf16 tables are built from h_w exactly as dt_load_darknet_weights builds them and passed (the split kernels;
 *     uint8 frames with W % 4 != 0 or at an unaligned address fall back to the fp32 MFMA kernel), 0 = null tables (the fp32 MFMA kernel);
 *   tpw: the launcher's test-only force_tpw -- 0 = its own rule for the tiles a workgroup walks along x, 1..26 = walk that many;
 *   publish != 0: max |x| of the stored values into max-|x| slot 57, zeroed first (dt_amax_read; the fp32 MFMA kernel publishes nothing: 0);
 *   d_out [B][H/2][W/2][32].
 * h_info[DT_CONV1_INFO_INTS] receives the launcher's plan: the instance (DT_C1_*), tpw, grid x, y, z, and 1 if the instance fills the slot.
 * DT_ERR_ARG with a message, and no launch, for what the launcher refuses: odd H or W, B <= 0 or > 65535, slope < 0, tpw outside 0..26. */
#define DT_CONV1_INFO_INTS 6
enum { DT_C1_MFMA_F32 = 0, DT_C1_S3_U8_FULL, DT_C1_S3_U8, DT_C1_S3_F32 };
DT_API int dt_conv1(dt_ctx *ctx, const void *d_frames, int frames_dtype, int B, int H, int W, const float *h_w, const float *h_bias, float slope,
                    int split, int tpw, int publish, float *d_out, int *h_info);

/* ---- tuning / test knobs ------------------------------------------------- *
 * The DT_* environment variables of DESIGN.md's appendix are read in dt_create (no launch path calls getenv);
 * this re-reads them into a live context.  dt_conv2d / dt_convlstm_step do the same on entry. */
DT_API int dt_policy_reload(dt_ctx *ctx);
/* One knob of ONE context without touching the process environment: name "pin", value 1 / 0 = DT_PIN on / off for this
 * context only (kernel selection independent of the batch a call carries; object_tracking_amd/parallel.py: deterministic=True),
 * -1 = follow DT_PIN again.  The override persists through dt_policy_reload and the test entry points' re-reads.  Any other
 * name or value fails with DT_ERR_ARG. */
DT_API int dt_policy_set(dt_ctx *ctx, const char *name, int value);
/* The max |x| the fp16 form scales a tensor by, as the kernels read it: synchronises the context's stream and returns in *h_out the
 * maximum over the sub-words of max-|x| slot `slot` (0..127).  Slot map: 0 = 1.0 (the recurrent step's bound |h| <= 1); i in 1..23 =
 * the output of conv_i as its consumer reads it (pooled where the layer pools, the space_to_depth tensor for conv_21; slot 20 becomes
 * the whole concat read by conv_22), published by the producing kernel's epilogue and zeroed at the start of every detector forward;
 * 32 + i = the input of conv_i where conv_i measured it itself; 56 = the tracker's z rows (ConvLSTM input projection); 57, 58 = the
 * layer-level test entry points' inputs (dt_conv2d / dt_convlstm_step: x, h); 64.. = scratch of the weight packs.  DT_AMAX_MEASURE=1
 * makes every consumer measure its input (32 + i / 56 / 57) while the producers still publish (tests compare the two). */
DT_API int dt_amax_read(dt_ctx *ctx, int slot, float *h_out);

/* ---- profiling --------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on the ctx
 * stream.  dt_profile_read synchronises the stream and returns, per kernel
 * family, launches / total ms / algorithmic flops / algorithmic bytes since the
 * last reset.  names: "conv_igemm", "conv1_direct", "convlstm_gates",
 * "decode_nms", "associate", "lstm_step", "pool", "stream_state", "misc"; per-layer tags such as
 * "conv_igemm:conv_19", "conv_igemm:convlstm_step" are listed by dt_profile_names. */
DT_API int dt_profile_enable(dt_ctx *ctx, int on);
DT_API int dt_profile_reset(dt_ctx *ctx);
/* newline-separated list of every name with data (families and "family:layer" tags) */
DT_API int dt_profile_names(dt_ctx *ctx, char *buf, size_t buflen);
DT_API int dt_profile_read(dt_ctx *ctx, const char *name, int64_t *launches,
                    double *total_ms, double *flops, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* MI355_DT_H */
