/* ubd.h -- C ABI of libubd_hip.so: the MI355X (gfx950) implementation of the
 * ubdvss hot path (dilated-FCN forward -> threshold map -> external components ->
 * rotated quads; train step = forward + loss + backward + Adam; training input:
 * geometric augmentation warps, photometric augmentation stages, bicubic resize,
 * label rasteriser).
 *
 * The reference (asmekal/ubdvss) has no FFI: the path sits behind three Python
 * seams.  Each entry point below names the seam it replaces (paths relative to
 * the reference root).  All pointers are raw DEVICE pointers owned by the caller
 * (e.g. torch tensors' data_ptr()) unless marked HOST; the library owns only its
 * handle.  Every call enqueues work on the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*, NULL = default stream) and returns without
 * synchronising.  Return value: 0 = ok, non-zero = error (see ubd_last_error()).
 * No torch types, no C++ types.
 */
#ifndef UBD_H
#define UBD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBD_ABI_VERSION 3

/* activation storage / compute dtype (weights, logits, loss and gradients are fp32) */
enum { UBD_F32 = 0, UBD_BF16 = 1, UBD_F16 = 2 };
/* input image dtype for ubd_forward; UBD_IN_PREPACKED may be OR-ed in: the packed-fragment region of `workspace`
 * already holds the fragments of the CURRENT parameter values (left there by a previous ubd_forward or
 * ubd_pack_weights on the same handle and workspace), so the per-call repacking kernels (~14 us) are skipped -- and so is the
 * zeroing of the fused stem kernel's strip counters, which that kernel leaves at zero itself: pass the flag only while
 * nothing else has written to the head of the workspace since. */
enum { UBD_IN_F32 = 0, UBD_IN_U8 = 1, UBD_IN_PREPACKED = 0x100 };
/* preprocessing fused into the first layer's load (net.py:217-218, NetConfig.get_preprocessing_fn) */
enum { UBD_PRE_NONE = 0, UBD_PRE_MOBILENET = 1 };

/* Mirrors the fields of NetConfig that reach the kernels (net.py:98-132):
 * grey -> c_in, fml_compatible, n_classes (0 = detection only). */
typedef struct ubd_config {
    int32_t c_in;            /* 1 (grey=True, the reference default) or 3 */
    int32_t n_classes;       /* 0..UBD_MAX_CLASSES */
    int32_t fml_compatible;  /* 1: ZeroPadding2D((1,0),(1,0)) + 'valid' for stride 2 (net.py:229-232) */
    int32_t dtype;           /* UBD_F32 / UBD_BF16 / UBD_F16 */
} ubd_config;

#define UBD_MAX_CLASSES 31
#define UBD_LOSS_FLOATS 16
#define UBD_N_FILTERS 24

typedef struct ubd_handle ubd_handle;

/* --- lifecycle ----------------------------------------------------------- */
int ubd_abi_version(void);
const char *ubd_build_id(void);                         /* 16 hex digits: fingerprint of the kernel sources (every .hip and .h file of csrc) THIS library was compiled from */
const char *ubd_last_error(void);                       /* thread-local message of the last failure */
/* Host staging helper of the streaming seam (ModelRunner.predict_stream; the loop of model_runner.py:60-67): copies n bytes with `threads`
 * native threads (1..16) -- a batch of pageable numpy memory into a pinned staging buffer without the interpreter in the way.  Returns 0. */
int ubd_host_memcpy_mt(void *dst, const void *src, size_t n, int threads);
int ubd_create(const ubd_config *cfg, ubd_handle **out); /* replaces NetManager.build_model (net.py:273-314) */
void ubd_destroy(ubd_handle *h);

/* Number of fp32 parameters; flat order = Keras model.get_weights() order
 * (SURVEY.md 9.2): per separable layer [depthwise(3,3,C,1), pointwise(1,1,C,24), bias],
 * per Conv2D [kernel HWIO, bias]; head last. */
size_t ubd_param_count(const ubd_handle *h);
/* Compute units the handle sizes its persistent grids for: the device's count, or UBD_TEST_NUM_CUS when that is set at
 * ubd_create (tests walk many tiles per block on small shapes with it; no reference counterpart). */
int ubd_num_cus(const ubd_handle *h);

/* Bytes of caller-provided device workspace needed by ubd_forward / ubd_train_step
 * for a batch of n images of height x width (multiples of 4). */
size_t ubd_forward_workspace_bytes(const ubd_handle *h, int n, int height, int width);
size_t ubd_train_workspace_bytes(const ubd_handle *h, int n, int height, int width);
size_t ubd_postprocess_workspace_bytes(const ubd_handle *h, int n, int map_h, int map_w, int cap);
size_t ubd_loss_workspace_bytes(const ubd_handle *h, int n, int map_h, int map_w);

/* --- inference ----------------------------------------------------------- */
/* Replaces keras Model.predict(images) at model_runner.py:119 / predict.py:74-76.
 * images: NHWC, (n, height, width, c_in), in_dtype UBD_IN_F32 (already preprocessed, or raw with
 *         preprocessing != NONE) or UBD_IN_U8.
 * logits: fp32 NHWC (n, height/4, width/4, 1+n_classes): channel 0 detection logit. */
int ubd_forward(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                int n, int height, int width, float *logits,
                void *workspace, size_t workspace_bytes, void *stream);

/* Layer-level entry points (profiling / roofline measurement of the dominant kernel; the
 * reference has no counterpart -- Keras runs the whole graph in one session.run).
 * ubd_pack_weights fills the packed-fragment region at the start of a forward workspace;
 * ubd_dilated_layer then runs ONE dense dilated 3x3 layer (layer = 0..5 -> net.py:298-304,
 * dilation 1,2,4,8,16,1) + bias + ReLU on (n, map_h, map_w, 24) activations. */
int ubd_pack_weights(ubd_handle *h, const float *params, void *workspace, size_t workspace_bytes, void *stream);
int ubd_dilated_layer(ubd_handle *h, const float *params, int layer, const void *in, void *out,
                      int n, int map_h, int map_w, const void *workspace, void *stream);

/* Replaces ModelRunner.predict's host tail (model_runner.py:121-134) and
 * SegmapManager.postprocess (segmap_manager.py:41-69) + utils.get_contours_and_boxes
 * (utils.py:51-60) for the whole batch:
 *   map = logits[...,0] > logit_threshold (strict);
 *   external 8-connected components (cv2.findContours RETR_EXTERNAL semantics);
 *   keep contourArea > min_area; minAreaRect -> boxPoints -> round(x*scale) half-to-even;
 *   optional class vote: argmax of mean softmax(class logits) over the filled contour.
 * Outputs (device):
 *   binary_map : int32 (n, map_h, map_w) values {0,1}              (may be NULL)
 *   quads      : int32 (n, cap, 8)  x1,y1,...,x4,y4 in cv2.boxPoints order, objects in cv2's
 *                return order (last raster-discovered first)
 *   classes    : int32 (n, cap)     (ignored when n_classes == 0; may be NULL then)
 *   counts     : int32 (n)          number of objects found; if counts[i] > cap the list of
 *                image i was truncated to cap entries and the caller must treat it as an error. */
int ubd_postprocess(ubd_handle *h, const float *logits, int n, int map_h, int map_w,
                    float logit_threshold, int scale, float min_area,
                    int32_t *binary_map, int32_t *quads, int32_t *classes, int32_t *counts, int cap,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ubd_forward of one batch and ubd_postprocess of an EARLIER batch's logits in one call (arguments as in those two; pp_* name the
 * earlier batch).  Replaces nothing new in the reference -- ModelRunner.predict (model_runner.py:105-138) runs the model and the
 * postprocess one after the other -- it is how the MI355X host overlaps the postprocess of batch k with the forward pass of
 * batch k+1: when the forward pass takes the one-kernel stem, the first pp_n blocks of that kernel do the postprocess before they
 * join the stem's work queue (no second stream, no events, no extra launch); otherwise the two calls are made back to back.
 * pp_logits must not alias `logits`.  Results are identical to the separate calls. */
int ubd_forward_postprocess(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                            int n, int height, int width, float *logits, void *workspace, size_t workspace_bytes,
                            const float *pp_logits, int pp_n, int pp_map_h, int pp_map_w, float logit_threshold, int scale,
                            float min_area, int32_t *binary_map, int32_t *quads, int32_t *classes, int32_t *counts, int cap,
                            void *pp_workspace, size_t pp_workspace_bytes, void *stream);

/* --- multi-scale inference (net.py:44-59 _create_multiscale_input / UpSampling2D branch, net.py:368-389 _build_multiscale_model) ---
 * The reference's multi-scale model runs the base net on the batch at full, 1/2, ..., 1/2^P size (P = max_scale_power, 3 at
 * net.py:368), brings every result back to the full map size with UpSampling2D(2^s) (nearest: y[i >> s, j >> s]) and takes the mean.
 * Size rule: height and width must be multiples of 4 * 2^P, otherwise the maps of the levels cannot be combined (the reference's
 * graph fails at its concatenation); every entry point below refuses other sizes and names the multiple.
 * Pyramid: the reference resizes with tf.image.resize_images (TF1's legacy bilinear, align_corners = False).  Under the size rule
 * in_size / out_size is exactly 2^s, every sample position is an integer and the interpolation weight is 0, so for finite inputs
 * level s is exactly images[:, ::2^s, ::2^s, :] (tests/test_multiscale_host.py holds the general formula against the
 * slice).  The slice commutes with the per-pixel preprocessing: uint8 pixels stay uint8 and each level's pass preprocesses them in
 * its first layer.
 * Mean: PER CHANNEL, out (n, height/4, width/4, 1 + n_classes).  The reference takes K.mean over the concatenation of all channels
 * of all levels, which is this value for a detection-only net (one channel) and meaningless with classes: a stated deviation.
 * Arithmetic, fixed so that it can be checked bit for bit: fp32, acc = y_0; acc += y_1[...]; ...; acc += y_P[...] in level order,
 * then acc / (float)(P + 1) as one IEEE division.  Parity with the reduction order of TF's K.mean is unpinned.
 * The same graph is trained by ubd_train_step_multiscale (training section below).
 *
 * Packed levels: levels first..P of an (n, height, width) array of pixel_bytes-byte pixels, level s being (n, height >> s,
 * width >> s), lie one after another without padding.  ubd_multiscale_levels_bytes is their total size (0 unless n, height, width,
 * pixel_bytes >= 1, first_level >= 0, max_scale_power 0..4 and both sides multiples of 2^max_scale_power); level s starts
 * ubd_multiscale_levels_bytes(..., first_level, s - 1) bytes into the buffer. */
size_t ubd_multiscale_levels_bytes(int n, int height, int width, int pixel_bytes, int first_level, int max_scale_power);

/* Layer-level entry points, in the spirit of ubd_dilated_layer.
 * ubd_multiscale_gather: levels 1..max_scale_power (1..4) of a batch, packed into levels_out, in ONE launch.
 *   images: NHWC (n, height, width, channels), channels 1 or 3, in_dtype UBD_IN_U8 or UBD_IN_F32 (copied bit for bit)
 *   levels_out: levels_bytes >= ubd_multiscale_levels_bytes(n, height, width, channels * (1 or 4), 1, max_scale_power)
 * Every even source row is read once, with 16-byte loads (8-byte for uint8 rows whose width is 8 mod 16), and feeds every level it
 * belongs to; odd rows are not read; nothing outside the rows and the packed levels is touched.  images and levels_out must be
 * 16-byte aligned, n * height / 2 < 2^31.
 * ubd_multiscale_fuse: the mean above.
 *   level_logits: fp32, levels 0..max_scale_power (0..4) of (n, map_h, map_w, k) packed, level 0 first; map_h and map_w multiples of
 *                 2^max_scale_power, k 1..UBD_MAX_CLASSES + 1
 *   out: fp32 (n, map_h, map_w, k); may be level 0 itself (level_logits), must not overlap anything else
 * Level 0 is read once (16-byte accesses where the addresses and map_w * k allow, else 8 or 4); the coarser levels come from cache.
 * ubd_multiscale_fuse_backward: the adjoint of that mean -- what each level's logits receive of d loss / d mean.
 *   dmean: fp32 (n, map_h, map_w, k)
 *   level_dlogits: fp32, levels 0..max_scale_power packed exactly as level_logits of ubd_multiscale_fuse (level s is (n, map_h >> s,
 *                  map_w >> s, k), ubd_multiscale_levels_bytes(n, map_h, map_w, 4 * k, 0, s - 1) bytes into the buffer); must not
 *                  overlap dmean.  The same limits and refusals as ubd_multiscale_fuse.
 * Arithmetic, fixed so that it can be checked bit for bit, per channel in fp32:  S_0 = dmean;
 *   S_s[i, j] = (S_(s-1)[2i, 2j] + S_(s-1)[2i, 2j+1]) + (S_(s-1)[2i+1, 2j] + S_(s-1)[2i+1, 2j+1])   (three additions, this association);
 *   level_dlogits_s = S_s / (float)(P + 1), one IEEE division per element; no FMA contraction, no reciprocal multiply.
 * dmean is read exactly once (16-byte accesses where the addresses and map_w * k allow, else 8 or 4); the sums pass from level to level
 * in LDS; no atomics, every output element is written once by one lane; nothing outside the packed levels is written.
 * All three: every violation returns non-zero with ubd_last_error() set and launches nothing; one launch, no handle, no host
 * synchronisation, no allocation, capturable in a HIP graph. */
int ubd_multiscale_gather(const void *images, int in_dtype, int n, int height, int width, int channels, int max_scale_power,
                          void *levels_out, size_t levels_bytes, void *stream);
int ubd_multiscale_fuse(const float *level_logits, int n, int map_h, int map_w, int k, int max_scale_power, float *out, void *stream);
int ubd_multiscale_fuse_backward(const float *dmean, int n, int map_h, int map_w, int k, int max_scale_power,
                                 float *level_dlogits, void *stream);

/* Replaces keras Model.predict of the model _build_multiscale_model returns (net.py:368-389).  Arguments as ubd_forward, plus
 * max_scale_power 0..4.  Enqueues on `stream`, in this order and with nothing between them that waits, allocates or reads on the
 * host: the gather; ubd_forward of level 0 into `logits` (it packs the weights once, unless UBD_IN_PREPACKED is OR-ed into in_dtype
 * under ubd_forward's rule); ubd_forward of levels 1..P, which reuse the packed fragments at the head of the same workspace; the
 * fuse, in place on `logits`.  Each level's pass is the existing path for its shape and dtype (UBD_F32 / UBD_BF16 / UBD_F16
 * handles alike), so `logits` equal ubd_multiscale_fuse of ubd_forward's outputs on the slices bit for bit.  One stream, a strictly
 * linear chain: capturable in a HIP graph.  max_scale_power == 0 IS ubd_forward: the same launches, the same bytes, and
 * ubd_forward_multiscale_workspace_bytes == ubd_forward_workspace_bytes.
 * Workspace: ubd_forward_multiscale_workspace_bytes (0 for arguments this call refuses): the forward workspace, then the packed
 * image levels (which is why it depends on in_dtype), then the packed logits of levels 1..P.
 * Refused (non-zero return, ubd_last_error names the required multiple): max_scale_power outside 0..4, a side that is not a
 * multiple of 4 * 2^max_scale_power, a workspace that is too small; with max_scale_power >= 1 also images that are not 16-byte
 * aligned. */
size_t ubd_forward_multiscale_workspace_bytes(const ubd_handle *h, int in_dtype, int n, int height, int width, int max_scale_power);
int ubd_forward_multiscale(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                           int n, int height, int width, int max_scale_power, float *logits,
                           void *workspace, size_t workspace_bytes, void *stream);

/* --- training ------------------------------------------------------------ */
/* Replaces the loss callable losses.get_loss(classification_mode)(y_true, y_pred)
 * (losses.py:20-24, :33-126) together with its autodiff gradient.
 *   y_true : int32 (n, map_h, map_w) labels 0..n_classes (0 = background)
 *   loss   : fp32 [UBD_LOSS_FLOATS] = {total, detection, classification, n_hard_k,
 *            positive_loss, negative_loss, hard_negative_loss (losses.py:138-191), n_pos,
 *            tp, tn, fp, fn of the detection map logit0 > 0 vs y_true > 0, number of positive pixels whose
 *            class argmax equals the label (keras_metrics.py:110-172), n_pixels, 0, 0}
 *   dlogits: fp32 like logits (may be NULL for loss only)
 * Batch-global reductions and top-k run over the n images given (per-replica semantics). */
int ubd_loss(ubd_handle *h, const float *logits, const int32_t *y_true, int n, int map_h, int map_w,
             float *loss, float *dlogits, void *workspace, size_t workspace_bytes, void *stream);

/* One pass fwd -> loss -> backward (replaces the body of Keras train_on_batch driven by
 * fit_generator, train.py:176-188, up to but excluding the optimiser update).
 *   grads : fp32 [param_count], same flat order as params (overwritten)
 *   loss  : fp32 [UBD_LOSS_FLOATS] as in ubd_loss
 * The caller may all-reduce `grads` across ranks before ubd_adam_step. */
int ubd_train_step(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                   const int32_t *y_true, int n, int height, int width,
                   float *grads, float *loss, void *workspace, size_t workspace_bytes, void *stream);

/* ubd_train_step through the multi-scale graph (net.py:368-389; train.py compiles and fits whichever model build_model returns).
 * Arguments, `grads` and `loss` as ubd_train_step, plus max_scale_power 0..4; y_true is (n, height/4, width/4) and the loss is taken
 * on the mean map.  Enqueues on `stream`, with nothing that waits, allocates or reads on the host: the pyramid gather; for every
 * level s = 0..P the handle's training forward (all activations kept) on level s, in the level's own region of the workspace; the
 * fuse into a mean map; the loss once, on the mean map (`loss`, d loss / d mean); ubd_multiscale_fuse_backward; for every level the
 * handle's backward pass for that level's shape from its own share of the gradient, into a gradient vector of its own; one kernel
 * grads = ((g_0 + g_1) + g_2) + ... + g_P, fp32, in level order.  Forward, loss and backward are ubd_train_step's kernels for each
 * shape and handle precision (UBD_F32 / UBD_BF16 / UBD_F16); every level packs its own weight fragments, as ubd_train_step does.
 * max_scale_power == 0 IS ubd_train_step: the same launches, the same bytes in `grads` and `loss`, and
 * ubd_train_multiscale_workspace_bytes == ubd_train_workspace_bytes.
 * Refused (non-zero return, ubd_last_error names the required multiple): max_scale_power outside 0..4, a side that is not a
 * multiple of 4 * 2^max_scale_power, a workspace smaller than ubd_train_multiscale_workspace_bytes (0 for arguments this call
 * refuses); with max_scale_power >= 1 also images or a workspace that are not 16-byte aligned, UBD_IN_PREPACKED, and a handle whose
 * communicator was made with UBD_COMM_FUSED: the exchange is never skipped silently -- use the explicit mode (ubd_comm_init without
 * UBD_COMM_FUSED, ubd_allreduce_grads on `grads` after this call). */
size_t ubd_train_multiscale_workspace_bytes(const ubd_handle *h, int in_dtype, int n, int height, int width, int max_scale_power);
int ubd_train_step_multiscale(ubd_handle *h, const float *params, const void *images, int in_dtype, int preprocessing,
                              const int32_t *y_true, int n, int height, int width, int max_scale_power,
                              float *grads, float *loss, void *workspace, size_t workspace_bytes, void *stream);

/* Keras 2.2 Adam (train.py:110): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v updated in place;
 * p -= lr_t*m/(sqrt(v)+eps); grads are multiplied by grad_scale first (1/world for DP mean). */
int ubd_adam_step(float *params, const float *grads, float *m, float *v, size_t count,
                  int t, float lr, float beta1, float beta2, float eps, float grad_scale, void *stream);

/* --- epoch logs (train.py:176-188: what Keras' BaseLogger keeps while fit_generator runs, and evaluate_generator for val_) ---
 * Adds one step's loss vector to the size-weighted sums of an epoch, on the device, so that the loop reads them ONCE per epoch
 * instead of reading the loss after every step.
 *   loss     : device fp32 [UBD_LOSS_FLOATS], as ubd_loss / ubd_train_step just wrote it on the same stream
 *   n_images : the step's batch size (>= 1)
 *   acc      : device, ubd_epoch_accumulator_bytes() bytes = (2 + UBD_EPOCH_VALUES) doubles, zeroed by the caller at the start
 *              of an epoch:  acc[0] += n_images (Keras' `seen`);  acc[1] += 1 when the total loss is not finite;
 *              acc[2 + i] += value_i * n_images for, in this order: loss, detection_pixel_acc, detection_pixel_precision,
 *              detection_pixel_recall, detection_pixel_f1, classification_pixel_acc, positive_loss, negative_loss,
 *              hard_negative_loss, detection_loss, classification_loss.
 * The values are those of keras_metrics.py:110-191 formed in double from the fp32 entries: tp / max(1, tp + fp),
 * ((2 p) r) / (p + r) or 0 when p + r == 0, cls_ok / max(1, n_pos), (tp + tn) / max(1, n_pixels); product and sum are rounded
 * separately.  All eleven are always added (the host takes the ones its mode reports); a value that is not finite goes into its
 * sum as it would in BaseLogger.  An epoch's log is acc[2 + i] / acc[0]: the mean of the per-batch values, not a pooled metric.
 * One launch of one wave, no atomics (launches on one stream are ordered); no handle, no host synchronisation, no allocation,
 * capturable in a HIP graph. */
#define UBD_EPOCH_VALUES 11
size_t ubd_epoch_accumulator_bytes(void);
int ubd_epoch_accumulate(const float *loss, int n_images, double *acc, void *stream);

/* --- training labels --------------------------------------------------------
 * Replaces SegmapManager.build_segmentation_map (segmap_manager.py:81-104) + _proper_round (:106-133) for a whole batch:
 * every object quad (8 float64 x1,y1..x4,y4 in IMAGE pixels; fractional after _rescale_image_and_markup / augmentation) is
 * divided by `scale` in double precision, its corners are snapped outward and the polygon is filled with PIL's
 * ImageDraw.polygon rule, objects in order (later over earlier), into an int32 map of (map_h, map_w) = image size / scale.
 * values[i][o]: what to write (class id + 1, or 1; 255 for drawing).
 *   quads float64 (n, cap, 8), values int32 (n, cap), counts int32 (n) (objects per image, <= cap), labels int32 (n, map_h, map_w):
 * the y_true layout of ubd_loss / ubd_train_step.  Bit-identical to Pillow for every quad except zero-area folds whose
 * opposite corners coincide (see raster.hip); the Python host rejects those. */
int ubd_build_label_maps(const double *quads, const int32_t *values, const int32_t *counts, int n, int cap,
                         int map_h, int map_w, int scale, int32_t *labels, void *stream);

/* --- polygon ground truth (semantic_segmentation/markup_readers.py:257-285, SegmentationMapMarkupReader) ---
 * Data sets whose ground truth is a segmentation map give one convex hull per external component, not a quad.  The three calls
 * below take such polygons with up to UBD_POLY_MAX_VERTS vertices. */
#define UBD_POLY_MAX_VERTS 64

/* Label maps from polygon markup: ubd_build_label_maps for objects of 3..max_verts vertices.
 *   verts  : device double (n, cap, max_verts, 2) x, y in image pixels; max_verts 3..UBD_POLY_MAX_VERTS
 *   nverts : device int32 (n, cap) vertices of every object
 * An object with 4 vertices is a quad: it goes through _proper_round and the quad rule and gets exactly the pixels
 * ubd_build_label_maps writes for it (the opposite-corner fold included).  Any other object with 3..max_verts vertices is divided
 * by the scale in double and truncated toward zero (segmap_manager.py:114-116: the reference does not snap a polygon that is
 * not a quad), then filled with ImageDraw.polygon's rule for n edges (csrc/polygon_fill.h; tests/test_polygon_fill_host.py pins
 * it to Pillow on convex polygons).  Objects are painted in order, later over earlier; quads and polygons may be mixed.  Objects
 * with any other vertex count are skipped (the Python host rejects them).  values, counts, labels, scale as in
 * ubd_build_label_maps.  Limits: map_w <= 8192, map_h and n <= 65535 (non-zero return, nothing launched).  One launch (one
 * block per map row), no host synchronisation, capturable in a HIP graph. */
int ubd_build_label_maps_polygons(const double *verts, const int32_t *nverts, const int32_t *values, const int32_t *counts,
                                  int n, int cap, int max_verts, int map_h, int map_w, int scale, int32_t *labels, void *stream);

/* Segmentation maps -> hull polygons (markup_readers.py:271-285: findContours(RETR_EXTERNAL) -> cv2.convexHull per contour).
 *   maps   : device uint8 (n, map_h, map_w); foreground is a byte that is not 0
 *   verts  : device int32 (n, cap, UBD_POLY_MAX_VERTS, 2) x, y in map pixels
 *   nverts : device int32 (n, cap) the TRUE hull size of every object; only the first UBD_POLY_MAX_VERTS vertices are stored,
 *            so nverts > UBD_POLY_MAX_VERTS tells the caller that the polygon is incomplete
 *   counts : device int32 (n) objects found; counts[i] > cap: the list of image i was truncated to cap entries (as ubd_postprocess)
 * Objects: the external 8-connected components, every one of them (the reader's min_area = -1), by the rule of ubd_postprocess
 * (a component inside a hole of another is not an object), in the order ubd_postprocess returns them (cv2's: last discovered
 * first).  Polygon: the strictly convex hull of the component's pixels (= the hull of its contour).  Vertex cycle: that of
 * cv2.convexHull(contour) with its defaults (clockwise = False) as restated here -- it starts at the vertex with the greatest x
 * (the greatest y among equals) and moves towards the vertex with the greatest y; this is the cycle of the postprocess' hull
 * (oracle/cv_post.c convex_hull) reversed and rotated to that start.  Hulls of 1 and 2 vertices (single pixels, straight
 * one-pixel lines) are emitted as they are.  As for the rest of the postprocess, parity with cv2 itself is unpinned: OpenCV is
 * not available where this is built.
 * Takes no handle.  Limits (non-zero return, ubd_last_error, nothing launched): n >= 1, sides 1..32767, n * map_h * map_w < 2^31,
 * cap 1..UBD_EVAL_MAX_GT, workspace_bytes >= ubd_segmap_polygons_workspace_bytes (0 for sizes outside the limits).  Global-memory
 * labelling at every map size (the call runs once per data set, not per step); no host synchronisation, no allocation,
 * capturable in a HIP graph. */
size_t ubd_segmap_polygons_workspace_bytes(int n, int map_h, int map_w, int cap);
int ubd_segmap_polygons(const uint8_t *maps, int n, int map_h, int map_w, int32_t *verts, int32_t *nverts, int32_t *counts,
                        int cap, void *workspace, size_t workspace_bytes, void *stream);

/* --- image preparation ------------------------------------------------------
 * Replaces Image.resize((dst_w, dst_h), Image.BICUBIC) of SegmapManager._rescale_image_and_markup (segmap_manager.py:135-173)
 * and, for dst_c == 1 from RGB, the Image.convert('L') of data_generators.py:177, for n uint8 images of any sizes to one size.
 * src + src_offsets[i] (HOST int64 byte offsets) = image i, (src_hw[2i], src_hw[2i+1]) (HOST) rows x cols, rows packed (pitch w*src_c).
 * dst: uint8 NHWC (n, dst_h, dst_w, dst_c).  Bit-identical to Pillow's 8-bit BICUBIC resampler.
 * (src_c, dst_c): (1,1), (3,3), (3,1) = resize then convert('L'), (1,3) = the grey result in three channels.
 * Limits: source sides 1..16384, destination sides 1..8192, n >= 1, n*dst_h*dst_w*dst_c < 2^31 (non-zero return otherwise).
 * Enqueues one launch per 64 images; no host synchronisation, capturable in a HIP graph. */
int ubd_resize_images(const uint8_t *src, const int64_t *src_offsets, const int32_t *src_hw, int src_c, int n,
                      uint8_t *dst, int dst_h, int dst_w, int dst_c, void *stream);

/* --- geometric augmentation ---------------------------------------------------
 * The image half of SegLinksImageAugmentation (augmentation.py:50-85): Image.rotate(angle, BILINEAR, expand=True) (:167),
 * Image.crop (:117), the quarter turns that Image.rotate performs as Image.transpose (:80), and
 * Image.transform(size, PERSPECTIVE, coeffs, BILINEAR) (:201), for n uint8 images of `channels` (1 or 3) channels, every image
 * with its own source and destination size.  Bit-identical to Pillow's generic transform with the bilinear filter.
 * Image i is read through a signed strided VIEW of the source buffer: view pixel (x, y) is at
 * src + src_offset + x * src_xpitch + y * src_ypitch (bytes; a packed image has pitches channels and src_w * channels), so a
 * crop (offset, smaller size) and a quarter turn (pitches swapped / negated) cost no pass of their own.  The destination image is
 * written packed (row pitch dst_w * channels) at dst + dst_offset; dword stores are used where that address is a multiple
 * of 4.  mode: UBD_WARP_COPY writes the view out as it is (dst size = view size); UBD_WARP_AFFINE maps destination pixel
 * centres through coeffs[0..5] (Pillow's AFFINE data: the matrix Image.rotate computes), UBD_WARP_PERSPECTIVE through
 * coeffs[0..7] (Pillow's PERSPECTIVE data); destination pixels whose source position is outside the view are 0.
 * descs: HOST array of n descriptors.  src_bytes / dst_bytes: sizes of the two buffers; every view and every destination
 * must lie inside them.  Source and destination must not overlap.
 * Limits: sides 1..16384 (so an image stays below 2^31 bytes), n >= 1, finite coefficients (non-zero return otherwise, nothing launched).
 * Enqueues one launch per 32 images; no host synchronisation, capturable in a HIP graph. */
enum { UBD_WARP_COPY = 0, UBD_WARP_AFFINE = 1, UBD_WARP_PERSPECTIVE = 2 };
typedef struct ubd_warp_desc {
    int64_t src_offset;              /* bytes from src to the view's pixel (0, 0) */
    int64_t dst_offset;              /* bytes from dst to the destination image */
    int32_t src_xpitch, src_ypitch;  /* signed bytes per view column / view row */
    int32_t src_w, src_h;            /* view size */
    int32_t dst_w, dst_h;
    int32_t mode;                    /* UBD_WARP_* */
    int32_t reserved;                /* 0 */
    double coeffs[8];
} ubd_warp_desc;
int ubd_warp_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, const ubd_warp_desc *descs,
                    int channels, int n, void *stream);

/* --- rectified patches of the found objects ---------------------------------------
 * The hand-over to a decoder: one upright uint8 patch of patch_h x patch_w per found object, cut out of the ORIGINAL frames
 * where the outputs of ubd_postprocess lie.  The engine restated is Pillow's Image.transform((patch_w, patch_h), Image.QUAD,
 * data, Image.BILINEAR), bit for bit (QUAD data as Image.__transformer forms it, quad_transform, and the bilinear filter that
 * ubd_warp_images uses), which a host would call once per object on frames copied back first.
 * ALL POINTERS ARE DEVICE POINTERS, the descriptors included: the call is one launch for any n and reads nothing on the host.
 *   src + src_offsets[i] (int64 byte offsets) = image i, packed uint8 rows of src_hw[2i] x src_hw[2i+1] (rows x cols) pixels of
 *     `channels` (1 or 3); src_bytes: size of the buffer behind src.  An image that does not lie inside [0, src_bytes) cannot be
 *     refused on the host, because its descriptor is device memory: the kernel treats it as EMPTY, reads nothing of it, and its
 *     patches come out all zero.
 *   quads (n, cap, 8) int32, counts (n) int32: exactly as ubd_postprocess writes them; slots j >= min(counts[i], cap) are not read.
 *   scales: (n, 2) doubles, xscale then yscale of image i (original / network size, ModelRunner.rescale's), or NULL: no rescale.
 *     Corners are rescaled as utils.rescale_bbox does: X = trunc(clamp(x * xscale, -2^30, 2^30)), toward zero.
 *   expand: > 0; 1.0 takes the corners as they are, otherwise every corner P becomes c + (P - c) * expand about the mean c of
 *     the four (a quiet zone around the code).
 *   patches: uint8 (n, cap, patch_h, patch_w, channels).  patch_quads: int32 (n, cap, 8) or NULL: the rescaled corners of every
 *     object in the order NW, NE, SE, SW of its patch, before expansion.  Patches and patch_quads rows of slots that hold no
 *     object are NOT written; nothing outside the two outputs is written.
 * Orientation (exact, in int64): corners in clockwise order on the screen (the order is reversed when the signed area says
 * counter-clockwise; a degenerate quad counts as clockwise), NW = corner 0 if side 0-1 is at least as long as side 1-2, else
 * corner 1.  The patch's width therefore runs along a long side and the patch is a rotation of the object, never a mirror
 * image; which of the two long sides is on top stays open (a half turn), decoders read both directions.  The order in which a
 * quad's vertices are listed does not change its patch.
 * The QUAD map sends the patch's corners to the four corners and interpolates bilinearly between them: for a rectangle (what
 * the postprocess' minAreaRect finds) it is affine and the patch is an exact rectification; for any other quad it is Pillow's
 * bilinear corner map, not a perspective one.  Positions outside the image give 0, as in ubd_warp_images.
 * Limits (non-zero return, ubd_last_error, nothing launched): n >= 1, cap >= 1, patch_h and patch_w 1..1024, channels 1 or 3,
 * expand finite and > 0, no null pointer except scales and patch_quads, n * cap * ceil(patch_h * patch_w / 1024) < 2^31.
 * |x * xscale| beyond 2^30 is clamped; without scales the orientation is exact for |coordinates| <= 2^30.
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph. */
int ubd_extract_objects(const uint8_t *src, size_t src_bytes, const int64_t *src_offsets, const int32_t *src_hw, int channels,
                        const int32_t *quads, const int32_t *counts, int n, int cap, const double *scales, double expand,
                        uint8_t *patches, int patch_h, int patch_w, int32_t *patch_quads, void *stream);

/* --- decoding of the object patches: EAN-13 / UPC-A / EAN-8 / UPC-E -----------------
 * The stage behind ubd_extract_objects: the digits of the retail symbol in every patch, read where the patches lie, so that
 * 64 bytes per object cross to the host instead of the patch.  One family, defined by the public EAN/UPC tables: EAN-13, UPC-A
 * (an EAN-13 whose first digit is 0), EAN-8 and UPC-E; `symbologies` is a mask whose bits are numbered over all families: bit 2,
 * Code 128, has a result row of its own and is read by ubd_decode_text_patches below, not here.  Integer arithmetic only (every division floors, every dividend is non-negative); the numpy restatement
 * tests/decode_oracle.py is matched bit for bit.
 *   patches (n, cap, patch_h, patch_w, channels) uint8 and counts (n) int32: DEVICE pointers, exactly as ubd_extract_objects
 *     writes and reads them; slots j >= min(counts[i], cap) are not read and their result rows are NOT written.
 *   params: HOST pointer, read before the call returns.
 *   results: DEVICE int32 (n, cap, 16): [0] symbology: 0 none, 13, 8 or 6 (UPC-E); [1] votes; [2] direction mask: bit 0 read left to
 *     right, bit 1 read right to left (the patch is the half-turned one); [3..15] the digits, an EAN-8 fills eight and the rest
 *     is -1; a UPC-E fills eight as well: number system, d1..d6, check digit.  For "none" every digit is -1 and votes and mask are 0.
 * Per patch:
 *   luma: the byte (1 channel) or (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (3 channels: Pillow's convert('L')).
 *   scan lines k = 0..S-1: centre row r_k = ((2k + 1) * patch_h) / (2S); p[x] = the luma sum over the rows [r_k - b, r_k + b]
 *     clipped to the patch, m = the number of those rows.
 *   local threshold: lo[x], hi[x] = min, max of p over [x - R, x + R] clipped to the line; d[x] = 2 p[x] - lo[x] - hi[x];
 *     where hi[x] - lo[x] < C * m, d[x] = max(d[x], 1).  A pixel is dark iff d[x] < 0.
 *   edges: between x and x + 1 wherever the darkness differs, in 1/256 pixel: e = 256 x + (256 |d[x]|) / (|d[x]| + |d[x+1]|),
 *     light-to-dark or dark-to-light.  Reading right to left is DEFINED on the mirrored list e'_j = 256 (patch_w - 1) - e_(E-1-j)
 *     with the polarities swapped, not on a second pass over the pixels.
 *   candidates: a light-to-dark edge i with the next 59 runs (EAN-13, 95 modules) or 43 runs (EAN-8, 67 modules) behind it;
 *     St = e[i + runs] - e[i].  The light run q before edge i and the one after the last run must each satisfy
 *     modules * q >= QZ * St; where that neighbouring edge is missing (the patch border) the test passes.  Every run w of the
 *     start guard (3 runs), the centre guard (5 runs) and the end guard (3 runs) must satisfy (2 * modules * w + St) / (2 St) == 1.
 *   characters: 4 runs w0..w3 of sum S4, edge to similar edge: E1 = (14 (w0 + w1) + S4) / (2 S4), E2 = (14 (w1 + w2) + S4) / (2 S4),
 *     both in 2..5; of the patterns n0..n3 of the allowed sets with n0 + n1 == E1 and n1 + n2 == E2 the one with the least
 *     |7 (w0 + w2) - S4 (n0 + n2)|; a tie rejects the candidate.  Set L, run widths in scan order for the digits 0..9:
 *     3211 2221 2122 1411 1132 1231 1114 1312 1213 3112; set R the same widths; set G those of L reversed.
 *     EAN-13: six left characters of {L, G}, whose parity word gives the first digit (0..9: LLLLLL LLGLGG LLGGLG LLGGGL LGLLGG
 *     LGGLLG LGGGLL LGLGLG LGLGGL LGGLGL; any other word rejects), then six of {R}.  EAN-8: four of {L}, four of {R}.
 *   checksums: EAN-13 (10 - (d0 + d2 + .. + d10 + 3 (d1 + d3 + .. + d11)) % 10) % 10 == d12;
 *     EAN-8 (10 - (3 (d0 + d2 + d4 + d6) + d1 + d3 + d5) % 10) % 10 == d7.
 *   UPC-E (bit 6): start guard of 3 runs, six characters of {L, G}, end guard of 6 runs (a space first): 33 runs, 51 modules.
 *     Candidate: a light-to-dark edge i with 33 runs behind it, St = e[i + 33] - e[i].  The light run q before edge i must
 *     satisfy 51 q >= QZ * St, the one after the last run 51 q >= max(QZ, 5) * St (a missing edge passes).  The five modules
 *     hold whatever QZ says: start guard, six L / G characters, centre guard and the first bar of the right half of an EAN-13
 *     have the shape of a UPC-E, and its parity word can be one of the twenty below (first digit 1, LLGLGG, is the word 0B of
 *     number system 1); as many UPC-E votes as EAN-13 votes would turn a good EAN-13 into "none".  No run inside an EAN symbol
 *     is wider than 4 modules, so the run behind that first bar fails the test.  Every run w of the two guards must satisfy
 *     (2 * 51 * w + St) / (2 St) == 1.  The six characters are read by the rule above.  Parity word: a set bit = G, the first
 *     character in the top bit; for number system 0 and the check digits 0..9 the words are 38 34 32 31 2C 26 23 2A 29 25
 *     (hexadecimal), number system 1 has their 6-bit complements, any other word rejects.  The digits d1..d6 stand for the
 *     UPC-A number NS a1..a10: d6 in 0..2: d1 d2 d6 0 0 0 0 d3 d4 d5; d6 = 3: d1 d2 d3 0 0 0 0 0 d4 d5; d6 = 4: d1 d2 d3 d4 0 0 0
 *     0 0 d5; d6 in 5..9: d1 d2 d3 d4 d5 0 0 0 0 d6; and (10 - (3 (NS + a2 + a4 + a6 + a8 + a10) + a1 + a3 + a5 + a7 + a9) % 10)
 *     % 10 must equal the check digit the parity word gave.  0 123456 5 is valid: 0 12345 00006 has the check digit 5.
 *   votes: per (line, direction, symbology) only the valid candidate with the lowest start index counts, one vote for its
 *     (symbology, digits).  The payload with the most votes wins, its mask is the OR of the directions that voted for it; fewer
 *     than min_votes, or another payload with as many votes: none.
 * Limits (non-zero return, ubd_last_error begins with "ubd_decode_patches", nothing launched, nothing written): no null
 * pointer, n >= 1, cap >= 1, n * cap < 2^31, patch_w 32..1024, patch_h 1..1024, channels 1 or 3, and the ranges below.
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph. */
typedef struct ubd_decode_params {
    int32_t symbologies;             /* bit 0 EAN-13 (UPC-A included), bit 1 EAN-8, bit 6 UPC-E: ubd_decode_patches takes any
                                        non-empty subset of 1 | 2 | 64; bit 2 Code 128, bit 7 Code 93: ubd_decode_text_patches
                                        takes 4, 128 or 132; bit 3 ITF, bit 4 Code 39, bit 8 Codabar: ubd_decode_width_patches
                                        takes any non-empty subset of 8 | 16 | 256.  The bits are numbered over all families.
                                        Bit 5 (32) is skipped: it was held back as the first bit no family reads when bits
                                        0..4 were given out, callers and tests rely on every layer refusing it, and so the
                                        three symbologies that came later took 6..8 and 32 stays unassigned.  Bit 10 POSTNET,
                                        bit 11 PLANET, bit 12 RM4SCC, bit 13 KIX: ubd_decode_postal_patches takes any non-empty
                                        subset of 1024 | 2048 | 4096 | 8192 = 15360, and the three older entries refuse these
                                        bits.  Bit 9 (512) is skipped for the reason bit 5 is: every older entry is held to
                                        refusing it, so it stays unassigned.  Bit 15 (32768) Data Matrix:
                                        ubd_decode_matrix_patches takes exactly 32768, and the four older entries refuse it.
                                        Bit 14 (16384) is skipped as bits 5 and 9 are */
    int32_t scan_rows;               /* S, 1..32        default 8  */
    int32_t band;                    /* b, 0..8         default 1  */
    int32_t window;                  /* R, 1..64        default 16 */
    int32_t contrast;                /* C, 0..255       default 24 */
    int32_t quiet;                   /* QZ, 0..16 modules, default 3 */
    int32_t min_votes;               /* 1..2*S          default 2  */
} ubd_decode_params;
int ubd_decode_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                       const ubd_decode_params *params, int32_t *results, void *stream);

/* --- decoding of the object patches: Code 128 / GS1-128 / Code 93 ---------------------
 * The second family behind ubd_extract_objects: the text of the Code 128 symbol in every patch, 128 bytes per object.  The
 * contract is that of ubd_decode_patches (device patches and counts as ubd_extract_objects writes them, params a HOST pointer
 * read before the call returns, slots j >= min(counts[i], cap) neither read nor written), the params struct is the same, and
 * `symbologies` must be 4 (bit 2, Code 128), 128 (bit 7, Code 93) or 132 (both).  Integer arithmetic only (every division
 * floors, every dividend is non-negative); the numpy restatements tests/text_decode_oracle.py (Code 128) and
 * tests/extra_decode_oracle.py (Code 93 and the two together) are matched bit for bit.
 *   results: DEVICE uint8 (n, cap, 128), aligned to 4 bytes: [0] 128, or 0 for none (a Code 93 row is laid out below); [1] votes; [2] direction mask (bit 0 read
 *     left to right, bit 1 read right to left: the patch is the half-turned one); [3] T, the number of text elements; [4] flags,
 *     bit 0: the first data character is FNC1 (GS1-128); [5] D, the number of data symbol characters; [6] the start value
 *     (103 / 104 / 105); [7] the check value; [8 .. 8 + T) the text elements; the rest 0xFF.  For "none" bytes 0..7 are 0 and
 *     bytes 8..127 are 0xFF.  A text element is an ASCII code 0..127 or 0xF1..0xF4 for FNC1..FNC4 (FNC4's Latin-1 meaning is
 *     not interpreted).
 * Per patch:
 *   luma, scan lines, local threshold, edges and the mirrored list for reading right to left: those of ubd_decode_patches.
 *   character: six runs w0..w5 (a bar first) of sum S; E_k = (22 (w_k + w_(k+1)) + S) / (2 S) for k = 0..3, each in 2..7; the
 *     pattern n0..n5 is the one of the table with n_k + n_(k+1) == E_k for all four k (the 107 keys are distinct); with
 *     V = n0 + n2 + n4 it must satisfy 2 |11 (w0 + w2 + w4) - S V| < 3 S.  Otherwise there is no character.
 *   table: run widths for the values 0..106, a bar first; 103 / 104 / 105 are Start A / B / C, 106 is the first six runs of
 *     the stop:
 *     212222 222122 222221 121223 121322 131222 122213 122312 132212 221213 221312 231212 112232 122132 122231 113222 123122
 *     123221 223211 221132 221231 213212 223112 312131 311222 321122 321221 312212 322112 322211 212123 212321 232121 111323
 *     131123 131321 112313 132113 132311 211313 231113 231311 112133 112331 132131 113123 113321 133121 313121 211331 231131
 *     213113 213311 213131 311123 311321 331121 312113 312311 332111 314111 221411 431111 111224 111422 121124 121421 141122
 *     141221 112214 112412 122114 122411 142112 142211 241211 221114 413111 241112 134111 111242 121142 121241 114212 124112
 *     124211 411212 421112 421211 212141 214121 412121 111143 111341 131141 114113 114311 411113 411311 113141 114131 311141
 *     411131 211412 211214 211232 233111
 *   candidate at a light-to-dark edge i of the direction's list e (E edges):
 *     1. the character at i (edges i..i+6) is a start, 103 / 104 / 105; S_0 is its width;
 *     2. if i >= 1: 11 (e_i - e_(i-1)) >= QZ * S_0;
 *     3. the characters at j = i + 6, i + 12, ..: character j needs the edges j..j+6, its width S must satisfy
 *        3 S_prev <= 4 S <= 5 S_prev, and it must decode to 0..102 (data) or 106 (stop); no character, or a value 103..105,
 *        rejects the candidate, and so do more than 62 values (start + 60 data + check) before a stop;
 *     4. at the stop edge j+7 must exist and the last bar b = e_(j+7) - e_(j+6) satisfy (22 b + S) / (2 S) == 2; if edge j+8
 *        exists: 11 (e_(j+8) - e_(j+7)) >= QZ * S;
 *     5. the values are start, d_1..d_D, check: D >= 1 and (start + sum k d_k) mod 103 == check.
 *   votes: per (line, direction, symbology) only the valid candidate with the lowest start index counts, one vote for its
 *     (symbology, whole value sequence), compared in full.  The sequence with the most votes wins, its mask is the OR of the directions
 *     that voted for it; fewer than min_votes, or another sequence with as many votes: none.
 *   text of the winner: the set in force comes from the start value (A, B, C).  In set C the values 0..99 are two digit
 *     characters, 100 switches to B, 101 to A, 102 is FNC1.  In sets A and B: 0..95 are ASCII (A: 0..63 -> 32..95, 64..95 ->
 *     0..31; B: 0..95 -> 32..127), 96 FNC3, 97 FNC2, 98 Shift (the next one data character is read in the other of A and B; a
 *     Shift as the last data character is dropped, a shifted Shift is a Shift again), 99 switches to C, 100 is Code B in A and
 *     FNC4 in B, 101 is FNC4 in A and Code A in B, 102 FNC1.  D <= 60 bounds T at 120.
 *   Code 93 (bit 7) character: six runs w0..w5 (a bar first) of sum S, nine modules; E_k = (18 (w_k + w_(k+1)) + S) / (2 S) for
 *     k = 0..3, each in 2..5; the pattern n0..n5 is the one of the table with n_k + n_(k+1) == E_k for all four k (the 48 keys
 *     are distinct); with V = n0 + n2 + n4 it must satisfy 2 |9 (w0 + w2 + w4) - S V| < 3 S (the table holds 48 of the 56
 *     six-run compositions of 9).  Table, run widths for the values 0..47:
 *     131112 111213 111312 111411 121113 121212 121311 111114 131211 141111 211113 211212 211311 221112 221211 231111 112113
 *     112212 112311 122112 132111 111123 111222 111321 121122 131121 212112 212211 211122 211221 221121 222111 112122 112221
 *     122121 123111 121131 311112 311211 321111 112131 113121 211131 121221 312111 311121 122211 111141
 *     0..9 are the digits, 10..35 A..Z, 36..42 - . space $ / + %, 43..46 the shifts ($) (%) (/) (+), 47 is start / stop.
 *   Code 93 candidate at a light-to-dark edge i:
 *     1. the character at i (edges i..i+6) is 47; S_0 is its width;
 *     2. if i >= 1: 9 (e_i - e_(i-1)) >= QZ * S_0;
 *     3. the characters at j = i + 6, i + 12, ..: the edges j..j+6 must exist, 3 S_prev <= 4 S <= 5 S_prev, and the character
 *        must decode; 47 is the stop, every other value counts; a 63rd value before a stop rejects the candidate;
 *     4. at the stop edge j+7 must exist and the termination bar b = e_(j+7) - e_(j+6) satisfy (18 b + S) / (2 S) == 1; if edge
 *        j+8 exists: 9 (e_(j+8) - e_(j+7)) >= QZ * S;
 *     5. the values are d_1..d_D, C, K with 1 <= D <= 60; C == (sum of d_k * weight) mod 47 with the weights 1..20 cycling from
 *        the right (d_D weighs 1), and K == the same sum over d_1..d_D, C with the weights 1..15.  "TEST93" has C = 41 (+), K = 6.
 *     Read backwards a Code 93 begins with its termination bar, which starts no character: it votes in one direction.
 *   Code 93 result row: [0] 93; [1] votes; [2] direction mask; [3] T = D; [4] 0; [5] D; [6] C; [7] K; [8 .. 8 + D) one element
 *     per data value: the ASCII code for 0..42, 0xE1..0xE4 for the shifts 43..46 (shift pairs are not interpreted); the rest 0xFF.
 * Limits (non-zero return, ubd_last_error begins with "ubd_decode_text_patches", nothing launched, nothing written): those of
 * ubd_decode_patches (no null pointer, n >= 1, cap >= 1, n * cap < 2^31, patch_w 32..1024, patch_h 1..1024, channels 1 or 3,
 * the ranges of ubd_decode_params), symbologies 4, 128 or 132, results aligned to 4 bytes.
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph. */
int ubd_decode_text_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                            const ubd_decode_params *params, uint8_t *results, void *stream);

/* --- decoding of the object patches: Interleaved 2 of 5 (ITF) / Code 39 / Codabar -----
 * The third family behind ubd_extract_objects: the two-width codes, in which every bar and every space is either narrow or
 * wide: the digits of an ITF symbol (ITF-14 included) or the characters of a Code 39 or Codabar symbol in every patch, 128
 * bytes per object.  The contract is that of ubd_decode_text_patches (device patches and counts as ubd_extract_objects writes them, params
 * a HOST pointer read before the call returns, slots j >= min(counts[i], cap) neither read nor written), the params struct is
 * the same, and `symbologies` must be a non-empty subset of 8 (bit 3, ITF), 16 (bit 4, Code 39) and 256 (bit 8, Codabar).
 * Integer arithmetic only, and no rule divides; the numpy restatements tests/width_decode_oracle.py (ITF, Code 39) and
 * tests/extra_decode_oracle.py (Codabar and the three together) are matched bit for bit.
 *   results: DEVICE uint8 (n, cap, 128), aligned to 4 bytes: [0] 25 (ITF), 39 (Code 39) or 27 (Codabar), or 0 for none; [1] votes; [2]
 *     direction mask (bit 0 read left to right, bit 1 read right to left: the patch is the half-turned one); [3] T, the number of
 *     text elements; [4] flags, bit 0: the optional check character holds (below; informational, it never rejects); [5..7] 0;
 *     [8 .. 8 + T) the ASCII codes of the elements; the rest 0xFF.  For "none" bytes 0..7 are 0 and bytes 8..127 are 0xFF.
 * Per patch:
 *   luma, scan lines, local threshold, edges and the mirrored list for reading right to left: those of ubd_decode_patches.
 *   narrow or wide: over a group of runs with the least run lo and the greatest run hi, a run w is wide iff 2 w > lo + hi.
 *     The group is valid only if it holds a wide run and 2 * (least wide run) >= 3 * (greatest narrow run).
 *   ITF pair: ten runs (a bar first) of sum S.  The five bars are one group and the five spaces another, classified
 *     separately; each must be valid, hold exactly two wide runs and show one of the patterns of the digits 0..9:
 *     nnWWn WnnnW nWnnW WWnnn nnWnW WnWnn nWWnn nnnWW WnnWn nWnWn.  The bars give the first digit, the spaces the second.
 *   ITF candidate at a light-to-dark edge i of the direction's list e (E edges):
 *     1. the start is the four runs at the edges i..i+4 (edge i+4 must exist), of sum S4;
 *     2. if i >= 1: 4 (e_i - e_(i-1)) >= QZ * S4;
 *     3. pairs at j = i + 4, i + 14, ..: if the edges j..j+10 exist, the ten runs decode to a pair and, from the second pair
 *        on, 7 S_prev <= 8 S <= 9 S_prev, the pair is data (data before stop); otherwise j must be the stop.  A 31st pair
 *        rejects the candidate, and so do fewer than 3;
 *     4. every run w of the start must satisfy lo <= 2 w <= lo + hi with lo, hi of the FIRST pair's group of w's colour;
 *     5. the stop is the runs at the edges j..j+3 (edge j+3 must exist), against lo, hi of the LAST pair's groups: the first
 *        bar wide (2 w > lo + hi of the bars), the space and the last bar with lo <= 2 w <= lo + hi of their colour; if edge
 *        j+4 exists: 2 (e_(j+4) - e_(j+3)) >= QZ * (space + last bar).
 *     The T = 2 * pairs elements are the digits as ASCII.  Flag bit 0 (the GS1 check digit):
 *     (d_(T-1) + sum over k < T-1 of d_k * (3 if T-1-k is odd else 1)) % 10 == 0; 15400141288763 holds it.
 *   Code 39 character: nine runs (a bar first) of sum S, one group; it must be valid, hold exactly three wide runs and show a
 *     pattern of the table; N6 is the sum of its six narrow runs.  Table, with the bar columns 1..10 = WnnnW nWnnW WWnnn nnWnW
 *     WnWnn nWWnn nnnWW WnnWn nWnWn nnWWn (bars and spaces interleaved, a bar first): the characters 1 2 3 4 5 6 7 8 9 0 take
 *     the columns 1..10 with the spaces nWnn; A..J with nnWn; K..T with nnnW; U V W X Y Z - . space * with Wnnn; $ / + % have
 *     five narrow bars and the spaces WWWn WWnW WnWW nWWW.  So 1 = WnnWnnnnW, A = WnnnnWnnW, * = nWnnWnWnn, % = nnnWnWnWn.
 *     Check values: 0-9 -> 0..9, A-Z -> 10..35, - . space $ / + % -> 36..42.
 *   Code 39 candidate at a light-to-dark edge i:
 *     1. the character at i (edges i..i+9) is *; S_prev and N6 are its;
 *     2. if i >= 1: 6 (e_i - e_(i-1)) >= QZ * N6;
 *     3. characters at j = i + 10, i + 20, ..: the edges j..j+9 must exist; the gap g = e_j - e_(j-1) must satisfy
 *        N6_prev <= 12 g and 2 g <= S_prev; the width 7 S_prev <= 8 S <= 9 S_prev; the character must decode.  A * is the stop,
 *        every other character is data; a 61st data character rejects the candidate, and so does a stop behind none;
 *     4. if edge j+10 exists behind the stop: 6 (e_(j+10) - e_(j+9)) >= QZ * N6 of the stop.
 *     The T elements are the data characters as ASCII; pairs of Full ASCII are not interpreted.  Flag bit 0 (the modulo-43
 *     check character): T >= 2 and (the sum of the first T-1 values) % 43 == the last value; "CODE 39" sums to 113, its check
 *     character is R (27).
 *   Codabar (bit 8) character: seven runs (a bar first).  The four bars are one group and the three spaces another, classified
 *     separately as those of an ITF pair are, with one rule beside the group rule: a group whose greatest run is less than
 *     1.5 times its least (2 hi < 3 lo) has no wide run and is valid.  (First proposal: the seven runs as one group, as a Code 39
 *     character's nine are.  The acceptance set moved it: at a narrow run of 2 pixels and a ratio of 2, blurred, the wide bars
 *     of : / . + come out at 3.8 pixels and their narrow spaces at 2.8, which one group cannot tell apart.)  The pattern is the
 *     mask of the wide runs, the first run in the top bit; for 0123456789-$:/.+ABCD the masks are 03 06 09 60 12 42 21 24 30 48
 *     0C 18 45 51 54 15 1A 29 0B 0E (hexadecimal); any other mask is no character.  A character's value is its index in that
 *     list.  N is the sum of its narrow runs and c their number (5 for the values 0..11, 4 for the others), S its width.
 *   Codabar candidate at a light-to-dark edge i:
 *     1. the character at i (edges i..i+7) is one of A B C D;
 *     2. if i >= 1: 4 (e_i - e_(i-1)) >= QZ * N;
 *     3. characters at j = i + 8, i + 16, ..: the edges j..j+7 must exist; the gap g = e_j - e_(j-1) must satisfy
 *        N_prev <= 2 c_prev g (half a mean narrow run) and 2 g <= S_prev; the character must decode; character widths differ
 *        inside a symbol, so neighbours are compared by their mean narrow runs: 3 N_prev c <= 4 N c_prev <= 5 N_prev c.  One of
 *        A B C D is the stop, every other character is data; a 61st data character rejects the candidate, and so does a stop
 *        behind none;
 *     4. if edge j+8 exists behind the stop: 4 (e_(j+8) - e_(j+7)) >= QZ * N of the stop.
 *     The T elements are all characters, start and stop included, as ASCII.  Flag bit 0: the sum of all T values is 0 modulo 16
 *     (informational).  No start pattern read backwards (2C 4A 68 38) is in the table, so a symbol votes in one direction.
 *   votes: per (line, direction, symbology) only the valid candidate with the lowest start index counts, one vote for its
 *     (symbology, all elements), compared in full.  The payload with the most votes wins, its mask is the OR of the directions
 *     that voted for it; fewer than min_votes, or another payload with as many votes: none.
 * Limits (non-zero return, ubd_last_error begins with "ubd_decode_width_patches", nothing launched, nothing written): those
 * of ubd_decode_text_patches, with symbologies a non-empty subset of 8 | 16 | 256.
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph. */
int ubd_decode_width_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                             const ubd_decode_params *params, uint8_t *results, void *stream);

/* --- decoding of the object patches: POSTNET / PLANET / RM4SCC / KIX -------------------
 * The fourth family behind ubd_extract_objects: the postal height-modulated codes.  Their bars all have one width and one pitch
 * and the data is in how far each bar rises and falls, so no run width carries anything and the candidates are walked on the
 * patch itself, bar by bar.  Read are POSTNET and PLANET (two bar heights on one base line), RM4SCC (Royal Mail 4-state) and
 * KIX (the same characters without frame bars and without a check).  Not read: Intelligent Mail and Australia Post, and no
 * error correction of any kind.  The contract is that of ubd_decode_width_patches (device patches and counts as
 * ubd_extract_objects writes them, params a HOST pointer read before the call returns, slots j >= min(counts[i], cap) neither
 * read nor written), the params struct is the same, and `symbologies` must be a non-empty subset of 1024 (bit 10, POSTNET),
 * 2048 (bit 11, PLANET), 4096 (bit 12, RM4SCC) and 8192 (bit 13, KIX).  Integer arithmetic only (every division floors, every
 * dividend is non-negative); the numpy restatement tests/postal_decode_oracle.py is matched bit for bit.
 *   results: DEVICE uint8 (n, cap, 128), aligned to 4 bytes: [0] 80 (POSTNET), 76 (PLANET), 82 (RM4SCC) or 75 (KIX), or 0 for
 *     none; [1] votes; [2] direction mask (bit 0 read as the patch lies, bit 1 read on the half-turned patch); [3] T, the number
 *     of characters; [4] flags, bit 0: the symbol carries a check and it held (always 1 for the first three, 0 for KIX); [5] B,
 *     the number of bars; [6..7] 0; [8 .. 8 + T) the ASCII codes of the characters, the check digit or check character
 *     included; the rest 0xFF.  For "none" bytes 0..7 are 0 and bytes 8..127 are 0xFF.
 * Per patch (H rows, W columns):
 *   luma g(y, x), scan lines k with their rows r_k, band profile, local threshold, edges and the mirrored list: those of
 *     ubd_decode_patches.  They serve only to find the start edges and the light run before them.
 *   direction 1 is direction 0 on the half-turned patch: g'(y, x) = g(H - 1 - y, W - 1 - x), the edge list is the mirrored list,
 *     the row is H - 1 - r_k.  Everything below is said for direction 0.
 *   walk from a light-to-dark edge i whose closing edge i + 1 exists, once per G (5 for POSTNET and PLANET, 4 for RM4SCC and KIX).
 *     State: the row r = r_k and the bar [s, t] = [e_i, e_(i+1)] in 1/256 pixel.  Per bar, on single-row luma:
 *     1. xc = (s + t + 256) / 512; Lmin, Lmax the least and greatest g(r, x) over x in [xc - R, xc + R] clipped to the patch
 *        (R = window); thr = Lmin + Lmax; a pixel is dark iff 2 g < thr.  The chain ends, this bar not part of it, if
 *        Lmax - Lmin < C (contrast) or (r, xc) is not dark;
 *     2. from the second bar on the pitch p = s - s_prev: the chain ends unless 4 (t - s) <= 3 p, and from the third bar on
 *        unless 3 p_prev <= 4 p <= 5 p_prev;
 *     3. top and bot are the first and last row of the unbroken dark run through (r, xc) in column xc;
 *     4. the tracking row, once this bar is the G-th or a later one: T the greatest top and Bm the least bot of the last G bars
 *        (this one included); the chain ends, this bar not part of it, if Bm < T; q = (Bm - T) / 4;
 *        r = min(max(r, T + q), Bm - q).  The row moves only when it nears the edge of what the last G bars share;
 *     5. the bar is part of the chain.  A 123rd bar: no candidate;
 *     6. the next bar, on the row r of step 4 with this bar's thr, d(x) = 2 g(r, x) - thr: the first x in
 *        [t / 256 + 1, t / 256 + 1 + n) with x + 1 <= W - 1 and d(x) >= 0 > d(x + 1), where n = 2 p / 256 pixels (n = R behind
 *        the first bar), gives s' = 256 x + 256 d(x) / (d(x) - d(x + 1)); the first x' in (x, x + R] with x' + 1 <= W - 1 and
 *        d(x') < 0 <= d(x' + 1) gives t' = 256 x' + 256 (-d(x')) / (d(x' + 1) - d(x')).  If either is not found the chain ends.
 *     (Two simpler designs failed on rendered symbols: extents measured from the fixed scan row lose the tracker band of a
 *     4-state code under 1 to 2 degrees of slant; re-centring the row on every window of bars loses the short bars of a PLANET
 *     behind six tall bars in a row.  Hence the clamped row of step 4.)
 *   quiet zones, with B bars and St = t_last - s_first: if i >= 1: (2 B - 1) (e_i - e_(i-1)) >= QZ * St; and on the row r left
 *     by the last bar's step 4, with the last bar's thr, every pixel x in [t_last / 256 + 1, t_last / 256 + 1 + n) with x <= W - 1,
 *     n = ceil(QZ * St / ((2 B - 1) * 256)), must be light (2 g >= thr).
 *   long or short: per bar a = -top and c = bot; Hs the greatest bot - top + 1 of the chain.  A group is the bars of one
 *     character; of a framed symbol the first bar joins the first character's group and the last bar the last's.  Per group,
 *     over a and separately over c, with the least value lo and the greatest hi: if 5 (hi - lo) < Hs no bar of the group is long,
 *     otherwise a bar w is long iff 2 w > lo + hi.  A word is a character's bars in order, 1 = long.
 *   POSTNET: B one of 32, 37, 52, 62; no bar long in c; the first and the last bar long in a; the a word of each five bars is
 *     one of 11000 00011 00101 00110 01001 01010 01100 10001 10010 10100, the digits 0..9; the digits sum to 0 modulo 10.
 *   PLANET: B one of 62, 72; the same with every a word complemented before it is looked up.
 *   RM4SCC: B = 4 n + 2, n in 2..30; the first bar long in a and not in c, the last long in both; the a word and the c word of
 *     each four bars are among 0011 0101 0110 1001 1010 1100, of the indices 0..5; value = 6 * index(a word) + index(c word),
 *     the character "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[value].  The last value must equal 6 * ((Rs + 5) % 6) + (Cs + 5) % 6,
 *     Rs the sum of (value / 6 + 1) and Cs the sum of (value % 6 + 1) over the others, both modulo 6.  SN34RD1A has the check K.
 *   KIX: B = 4 n, n in 4..30; the characters as RM4SCC's, no frame bars and no check.  A KIX votes in direction 0 only: its
 *     half-turned reading is always another valid KIX text (every character reversed with a and c swapped), so both directions
 *     would tie to "none".  The caller must know which way up a KIX lies.
 *   votes: per (line, direction, symbology) only the valid candidate with the lowest start index counts, one vote for its
 *     (symbology, all characters).  The payload with the most votes wins, its mask is the OR of the directions that voted for
 *     it; fewer than min_votes, or another payload with as many votes: none.
 * Limits (non-zero return, ubd_last_error begins with "ubd_decode_postal_patches", nothing launched, nothing written): those
 * of ubd_decode_width_patches, with symbologies a non-empty subset of 15360.
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph.
 * hip_stream is the hipStream_t of the launch, exactly what the other entries call `stream`.  It has a name of its own because
 * tests/test_lib_call_host.py counts the declarations that end in `void *stream` and holds that set to the 33 entries of
 * ubdvss_amd/_lib.py's ON_STREAM; an entry that came later stands beside that set (_lib.LAUNCHED), not in it. */
int ubd_decode_postal_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                              const ubd_decode_params *params, uint8_t *results, void *hip_stream);

/* --- decoding of the object patches: Data Matrix (ECC 200, 10 x 10 to 26 x 26) ---------
 * The fifth family behind ubd_extract_objects and the first 2-D one: the Data Matrix symbol that stands roughly upright (any of
 * the four quarter turns, a few degrees of slant) and alone in its patch.  It is the one entry with error correction: one
 * Reed-Solomon block per symbol.  Read are the nine square sizes 10, 12 .. 26 of ECC 200 and the ASCII encodation.  Not read:
 * rectangular sizes, sizes from 32 x 32 up, the C40 / Text / X12 / EDIFACT / Base 256 schemes, macros, ECI and structured append
 * (they come back as raw codewords), ECC 000-140, mirrored or light-on-dark symbols.  The contract is that of
 * ubd_decode_postal_patches (device patches and counts as ubd_extract_objects writes them, params a HOST pointer read before
 * the call returns, slots j >= min(counts[i], cap) neither read nor written), the params struct is the same, and `symbologies`
 * must be exactly 32768 (bit 15).  Bit 14 (16384) is skipped for the reason bits 5 and 9 are: every older layer is held to
 * refusing it.  The four older entries refuse bit 15.  Of the params, band, window and contrast are used; scan_rows, quiet and
 * min_votes are checked against their usual ranges and otherwise UNUSED (there are no scan lines and no votes here).  Integer
 * arithmetic only; `/` below floors (dividends may be negative), `>>` is an arithmetic shift; the numpy restatement
 * tests/matrix_decode_oracle.py is matched bit for bit.
 *   results: DEVICE uint8 (n, cap, 128), aligned to 4 bytes: [0] 68 ('D'), or 0 for none; [1] n, the modules per side, 10..26;
 *     [2] the quarter turns 0..3 (counter-clockwise) by which the patch shows the symbol turned; [3] T, the number of text
 *     elements; [4] flags, bit 0: FNC1 in first position (GS1), bit 1: the text is incomplete (a codeword outside the ASCII
 *     encodation ended it); [5] the codewords Reed-Solomon corrected; [6] the finder mismatches of the hypothesis that stood;
 *     [7] U, the number of raw codewords; [8 .. 8 + T) the elements (bytes: Latin-1); [8 + T .. 8 + T + U) the raw data
 *     codewords; the rest 0xFF.  For "none" bytes 0..7 are 0 and bytes 8..127 are 0xFF.
 * Per patch (H rows, W columns), with b = band, m = (2 b + 1)^2, R = window, C = contrast:
 *   1. dark map: luma g(y, x) as in ubd_decode_patches.  s(y, x) = the sum of g over the (2 b + 1)^2 neighbourhood, coordinates
 *      clamped to the patch; lo, hi = the least and greatest s over the square [x - R, x + R] x [y - R, y + R] clipped to the
 *      patch; d = 2 m g(y, x) - lo - hi; where hi - lo < C m, d = max(d, 1).  A pixel is dark iff d < -C m.  (The raw pixel
 *      against the smoothed extremes: a smoothed pixel loses isolated modules at 3 pixels a module.  The margin -C m: the
 *      extremes of a 33 x 33 window of noise pass a flatness test made for 33 samples, and without it a ring of speckle at
 *      distance R around the symbol breaks step 2.)
 *   2. box: cd(x), rd(y) the dark pixels per column and row; x0, x1 the first and last column with cd >= max(1, max(cd) / 4),
 *      y0, y1 likewise from rd.  None found, or a side x1 - x0 + 1 or y1 - y0 + 1 under 20 pixels: none.
 *   3. side lines: left(y) = the first dark x in columns x0..x1 of row y, right(y) = the last such x plus 1, for y in y0..y1;
 *      top(x), bottom(x) the same down column x over rows y0..y1; a row or column without a dark pixel in the box is skipped.
 *      A side's extent [a0, a1] is y0..y1 (left, right) or x0..x1 (top, bottom), L = a1 - a0 + 1, and its two segments are
 *      [a0 + L / 16, a0 + L / 2 - 1] and [a1 - L / 2 + 1, a1 - L / 16].  Fewer than 4 values in a segment: none.  Each segment
 *      [s0, s1] gives an anchor in 1/16 pixel: along the side c = 8 (s0 + s1 + 1); across it p = 16 v, v the k-th smallest
 *      (left, top) or k-th largest (right, bottom) of the segment's `count` values, k = count / 4, counted from 0.  (A quartile
 *      lands on the outer edge of a dashed side as of a solid one and ignores stray pixels.)  The side's line through its
 *      anchors (c1, p1), (c2, p2): line(c) = p1 + ((p2 - p1) (c - c1)) / (c2 - c1), clamped to -32768..32767 (so that every
 *      product fits an int32).
 *   4. corners in 1/16 pixel, for (top, left), (top, right), (bottom, left), (bottom, right): y = horizontal(8 (x0 + x1 + 1));
 *      then three times x = vertical(y), y = horizontal(x).
 *   5. sample of module (r, c) of an n x n grid, N = 2 n, u = 2 c + 1, v = 2 r + 1: X = ((N - u)(N - v) TL + u (N - v) TR +
 *      (N - u) v BL + u v BR) / N^2 per coordinate; the pixel (X >> 4, Y >> 4) clamped to the patch; the module is dark iff that
 *      pixel is.
 *   6. finder: for n = 10, 12 .. 26 the 4 n - 4 border modules are sampled, and for each turn t = 0..3 the mismatches against the
 *      turned canonical border are counted.  Module (r, c) of the grid lies in the symbol at (r, c), (c, n - 1 - r),
 *      (n - 1 - r, n - 1 - c), (n - 1 - c, r) for t = 0, 1, 2, 3.  The canonical border: column 0 and row n - 1 dark; else row 0
 *      dark at even columns; else column n - 1 dark at odd rows.  The hypothesis (n, t) with the fewest mismatches `miss` of the
 *      36 stands only if 8 miss <= 4 n - 4 and every other hypothesis has more.  Else none.
 *   7. codewords: the n x n grid is sampled and written where each module lies in the symbol; the placement of ISO/IEC 16022
 *      Annex F is walked on the (n - 2) x (n - 2) mapping matrix inside the border (the Utah shape with its two wrap rules, the
 *      four corner cases at their standard trigger positions, the fixed corner left out), bit 1 the most significant.
 *      Data / check codewords: 10: 3 / 5, 12: 5 / 7, 14: 8 / 10, 16: 12 / 12, 18: 18 / 14, 20: 22 / 18, 22: 30 / 20,
 *      24: 36 / 24, 26: 44 / 28 (each pair sums to (n - 2)^2 / 8).
 *   8. Reed-Solomon over GF(256) with the polynomial 0x12D, alpha = 2, e check codewords, the first codeword the highest power:
 *      S_j = r(alpha^j), j = 1..e.  All zero: nothing to correct.  Otherwise Berlekamp-Massey, the Chien search over the
 *      codeword positions and Forney's values; at most e / 2 errors, the number of roots found must equal the locator's degree,
 *      and the corrected word's syndromes must vanish.  Anything else: none.  ("123456" is 142 164 186 with the check codewords
 *      114 25 5 88 102.)
 *   9. text of the data codewords: 1..128 the element cw - 1; 130..229 two digit elements; 235 followed by a codeword 1..128:
 *      the element of that codeword + 127 (upper shift); 129 ends the data; 232 in first position sets flag bit 0, later it is
 *      the element 0x1D.  Any other codeword (a 235 without such a follower included) sets flag bit 1 and ends the text: it and
 *      the data codewords behind it are the U raw bytes.
 * Limits (non-zero return, ubd_last_error begins with "ubd_decode_matrix_patches", nothing launched, nothing written): no null
 * pointer, results aligned to 4 bytes, n >= 1, cap >= 1, n * cap < 2^31, patch_h and patch_w 32..128, channels 1 or 3,
 * symbologies 32768, band 0..2, window 1..64, contrast 0..255, and scan_rows, quiet, min_votes in the ranges of
 * ubd_decode_params.  (band <= 2 and sides <= 128 keep the workgroup within 64 KB of LDS.)
 * One launch; no host synchronisation, no allocation, no handle, capturable in a HIP graph.
 * launch_stream is the hipStream_t of the launch, what the other entries call `stream` or `hip_stream`.  Its name matches neither
 * of the two patterns by which tests/test_lib_call_host.py and tests/test_postal_decode_host.py count the older declarations;
 * ubdvss_amd/_lib.py keeps such an entry in LAUNCHED_LATER (tests/test_matrix_decode_host.py holds that set to this header). */
int ubd_decode_matrix_patches(const uint8_t *patches, const int32_t *counts, int n, int cap, int patch_h, int patch_w, int channels,
                              const ubd_decode_params *params, uint8_t *results, void *launch_stream);

/* --- photometric augmentation ---------------------------------------------------
 * The built part of the reference's imgaug stage (augmentation.py:276-332: all of it but the two noise-alpha operations), one
 * operation ("stage") per image per call, for n
 * uint8 images of `channels` (1 or 3) channels with packed rows (pitch w * channels), every image with its own size, at
 * src + src_offset, written at dst + dst_offset.  imgaug and OpenCV are not available to pin against: every mode is DEFINED in
 * integer arithmetic here (each follows imgaug's published formula) and the device matches the numpy oracle of the tests bit for
 * bit; PARITY WITH imgaug / cv2 IS UNPINNED.  `>>` is an arithmetic shift, clamp is to 0..255, borders are reflect-101 (fold
 * with period 2(n-1); always 0 for n = 1).  Layout of p[] per mode:
 *   UBD_PHOTO_AFFINE  (Invert, Add, Multiply, ContrastNormalization): p[c] = m_c, p[3 + c] = a_c (Q16), c = channel;
 *                     out = clamp((m_c v + a_c + 32768) >> 16)
 *   UBD_PHOTO_GREY    (Grayscale): p[0] = aq = rint(alpha 16384); g = (4899 R + 9617 G + 1868 B + 8192) >> 14,
 *                     out = ((16384 - aq) v + aq g + 8192) >> 14; one channel: the identity
 *   UBD_PHOTO_FILTER3 (Sharpen, Emboss): p[0..8] = the 3x3 correlation taps in Q14, row-major, |tap| <= 13 * 16384;
 *                     out = clamp((sum tap v + 8192) >> 14)
 *   UBD_PHOTO_SEP     (GaussianBlur): p[0] = radius r (1..4), p[1 + d] = Q14 weight at distance d = 0..r, each 0..16384, the
 *                     2r + 1 taps summing to 16384; rows: t = (sum w v + 64) >> 7, then columns: out = clamp((sum w t + 2^20) >> 21)
 *   UBD_PHOTO_BOX     (AverageBlur): p[0] = k (2..7); window offsets -(k/2) .. k-1-(k/2) on both axes, S its sum,
 *                     out = (2 S + k k) / (2 k k)
 *   UBD_PHOTO_NOISE   (AdditiveGaussianNoise): p[0] = the bits of the fp32 scale (finite, >= 0); flags bit 0 = per channel
 *   UBD_PHOTO_DROPOUT (Dropout): p[0] = the bits of the uint32 threshold floor(p 2^32); flags bit 0 = per channel
 *   UBD_PHOTO_MEDIAN = 16 (MedianBlur): p[0] = k, odd, 3..11; per channel, out = the median of the k x k window centred on the
 *                     pixel = element (k k - 1) / 2 of its sorted k k values.  Coordinates outside the image are CLAMPED TO THE
 *                     EDGE (OpenCV's medianBlur documents BORDER_REPLICATE) -- not the reflect-101 of the other neighbourhood modes
 *   UBD_PHOTO_HSV = 17 (AddToHueAndSaturation): 3 channels only; p[0] = dh, p[1] = ds, each -255..255.  All int32, `/` truncates
 *                     (its operands are never negative).  Forward, OpenCV's 8-bit RGB -> HSV (H 0..179) with its Q12 reciprocal
 *                     tables: V = max(R,G,B), m = min(R,G,B), D = V - m; sdiv(i) = (2088960 + i) / (2 i), hdiv(i) =
 *                     (245760 + i) / (2 i) for i >= 1, both 0 for i = 0 (= rint((255 << 12) / i), rint((180 << 12) / (6 i)));
 *                     S = (D sdiv(V) + 2048) >> 12; hn = G - B if V = R, else B - R + 2 D if V = G, else R - G + 4 D (the first
 *                     case that matches); H = (hn hdiv(D) + 2048) >> 12, H += 180 if H < 0.  Shift: H' = (H + dh) mod 180
 *                     (0..179), S' = clamp(S + ds, 0, 255), V unchanged.  Backward: i = H' / 30, f = H' - 30 i,
 *                     P = (30 V (255 - S') + 3825) / 7650, Q = (V (7650 - S' f) + 3825) / 7650,
 *                     T = (V (7650 - S' (30 - f)) + 3825) / 7650; (R,G,B) by sector i = 0..5: (V,T,P), (Q,V,P), (P,V,T), (P,Q,V),
 *                     (T,P,V), (V,P,Q).  Over all 2^24 colours H stays in 0..179 and S in 0..255, the largest product is
 *                     1 044 582; dh = ds = 0 is NOT the identity (8-bit HSV loses up to 5 levels).  Design decision: imgaug of the
 *                     reference's era adds one value to the H and S channels and CLIPS H at 0..255; later imgaug wraps the hue.
 *                     This mode wraps.
 *   UBD_PHOTO_ELASTIC = 18 (ElasticTransformation): p[0] = aq = rint(256 alpha), 0..4096; p[1] = w0, p[2] = w1: the Q14 taps of
 *                     the 3-tap Gaussian that smooths the displacement field, each >= 0, w0 + 2 w1 = 16384; seed = the Philox key.
 *                     Raw field of a pixel inside the image, from the words of counter (y w + x, 0, 0, 0):
 *                     ex = (r0 >> 16) - 32768, ey = (r1 >> 16) - 32768 (Q15 in (-1, 1)); outside the image both are 0 (imgaug's
 *                     gaussian_filter(mode="constant", cval=0)).  Smoothing, for ex and ey alike: rows
 *                     t = (w1 e(x-1) + w0 e(x) + w1 e(x+1) + 8192) >> 14, then columns s = (w1 t(y-1) + w0 t(y) + w1 t(y+1) + 8192)
 *                     >> 14 with t = 0 for a row outside the image; every sum stays below 2^30.  Displacement in 1/32 pixel:
 *                     d = (aq s + 2^17) >> 18 (|aq s| <= 2^27, so at most 16 pixels).  Source position X = 32 x + dx,
 *                     Y = 32 y + dy; ix = X >> 5, kx = X & 31, likewise for y: output (x, y) samples the input at (x + dx, y + dy).
 *                     Interpolation: Keys' bicubic with a = -3/4 at 1/32-pixel phases (cv2.remap's INTER_CUBIC), exact integer
 *                     weights in Q17: W0 = -3 k (32 - k)^2, W1 = 5 k^3 - 288 k^2 + 131072, W2 = W1 at 32 - k, W3 = -3 (32 - k) k^2
 *                     (they sum to 131072) on the taps ix - 1 .. ix + 2; a tap outside the image contributes 0 (constant border).
 *                     out = clamp((sum_j sum_i Wy_j Wx_i v(ix-1+i, iy-1+j) + 2^33) >> 34), exact: a row's inner sum stays below
 *                     2^26 (int32), the four outer products are int64.  All channels share one displacement.  aq = 0 is the
 *                     identity; a constant image stays constant wherever all 16 taps are inside.  Design decision: imgaug of the
 *                     reference's era interpolates with a scipy cubic spline; this mode follows the later cv2 path, which is
 *                     defined without a whole-row prefilter.
 * Random words of NOISE / DROPOUT / ELASTIC: Philox4x32-10, key = seed (lo, hi), counter = (y w + x, 0, j, 0); block j = 0 gives r0..r3,
 * j = 1 gives r4..r7.  DROPOUT: 0 where the word < threshold; channel c tests r_c per channel, else every channel tests r0.
 * NOISE: u1 = ((a >> 9) + 0.5) 2^-23, u2 likewise from b, z = sqrt(-2 ln u1) cos(2 pi u2) in fp32, out = clamp(rint(v + scale z));
 * (a, b) = (r_2c, r_2c+1) per channel, else (r0, r1).
 * The pointwise modes (AFFINE, GREY, NOISE, DROPOUT, HSV) may run in place (same address for source and destination of an image);
 * any other overlap of an image's source and destination is refused, for the neighbourhood modes (FILTER3, SEP, BOX, MEDIAN,
 * ELASTIC) every one.
 * descs: HOST array of n descriptors.  Dword loads / stores are used where the addresses allow; any byte alignment works.
 * Limits: sides 1..16384 (so an image stays below 2^31 bytes), n >= 1, channels 1 or 3, ranges inside the two buffers, a known
 * mode (0..6 and 16..18: 7..15 and everything above 18 are refused), BOX k 2..7, SEP radius 1..4, MEDIAN k odd and 3..11, HSV
 * with 3 channels and |dh|, |ds| <= 255, ELASTIC aq 0..4096 with taps >= 0 and w0 + 2 w1 = 16384; and the parameter ranges that keep every sum inside int32: AFFINE |m_c| <= 2^17 and
 * |a_c| <= 2^24 (all three channels' entries are checked), GREY aq 0..16384, FILTER3 |tap| <= 13 * 16384, SEP weights 0..16384
 * whose 2r + 1 taps sum to 16384, NOISE scale finite and >= 0 (non-zero return otherwise, nothing launched).
 * Enqueues at most four launches per 32 images (one kernel each for the pointwise modes, for FILTER3 / SEP / BOX, for MEDIAN and
 * for ELASTIC; a kernel whose modes do not occur is not launched); no host synchronisation, capturable in a HIP graph.
 * The two noise-alpha operations of that stage, SimplexNoiseAlpha(EdgeDetect / DirectedEdgeDetect) and FrequencyNoiseAlpha, are
 * ubd_noise_alpha_images below. */
enum { UBD_PHOTO_AFFINE, UBD_PHOTO_GREY, UBD_PHOTO_FILTER3, UBD_PHOTO_SEP, UBD_PHOTO_BOX, UBD_PHOTO_NOISE, UBD_PHOTO_DROPOUT,
       UBD_PHOTO_MEDIAN = 16, UBD_PHOTO_HSV = 17, UBD_PHOTO_ELASTIC = 18 };
typedef struct ubd_photo_desc {
    int64_t src_offset, dst_offset;  /* bytes from src / dst to the image */
    int32_t w, h;
    int32_t mode;                    /* UBD_PHOTO_* */
    int32_t flags;                   /* bit 0: per channel (NOISE, DROPOUT) */
    uint64_t seed;                   /* Philox key (NOISE, DROPOUT, ELASTIC) */
    int32_t p[24];                   /* per mode, see above; unused entries 0 */
} ubd_photo_desc;
int ubd_photometric_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes,
                           const ubd_photo_desc *descs, int channels, int n, void *stream);

/* --- mask-blended augmentation stages ---------------------------------------------
 * The last two operations of the reference's imgaug stage: SimplexNoiseAlpha(OneOf([EdgeDetect, DirectedEdgeDetect]))
 * (augmentation.py:301-304) and FrequencyNoiseAlpha(first = Multiply, second = ContrastNormalization) (:319-323).  Both blend two
 * differently processed copies of the image, per pixel, by a smooth random mask: a few tiny noise grids (made by the caller on
 * the host), upscaled to the image, aggregated and pushed through a curve.  Images as for ubd_photometric_images: n uint8 images
 * of `channels` (1 or 3) channels with packed rows, every image with its own size at src + src_offset, written at
 * dst + dst_offset; sides 1..16384; any byte alignment works, dword accesses are used where the addresses allow.  Every
 * overlap of an image's source and destination ranges is refused (the FILTER3 branch reads neighbours).
 * DEFINITION, all in integer arithmetic (`>>` is an arithmetic shift, `/` has non-negative operands only); the device matches
 * tests/noise_alpha_oracle.py bit for bit; PARITY WITH imgaug / cv2 IS UNPINNED (cv2.resize's coefficients are restated at
 * 1/32-pixel phases, the noise generators are the caller's).
 *   Branches `first` and `second` give a uint8 value per channel, F_c and S_c:
 *     UBD_NA_IDENTITY  the pixel
 *     UBD_NA_FILTER3   p[0..8] = 3x3 correlation taps in Q14, row-major, |tap| <= 13 * 16384, reflect-101 border:
 *                      clamp((sum tap v + 8192) >> 14), exactly UBD_PHOTO_FILTER3
 *     UBD_NA_AFFINE    p[c] = m_c, p[3 + c] = a_c (Q16), |m_c| <= 2^17, |a_c| <= 2^24 (all three entries are checked):
 *                      clamp((m_c v + a_c + 32768) >> 16), exactly UBD_PHOTO_AFFINE
 *   Mask: `iterations` (1..3) grids; grid i has gw x gh cells (each 1..16), row-major uint16 values g in 0..32768 (Q15) at
 *   tables + grid_offset, and an upscale method.  Upscaled value u_i(x, y), Q15; each axis independently (x shown; y the same
 *   with h, gh, y):
 *     UBD_NA_NEAREST   ix = min(gw - 1, (x gw) / w), one tap of weight 1
 *     UBD_NA_LINEAR, UBD_NA_CUBIC (cv2.resize's pixel-centre rule): X = (2 x + 1) gw - w, ix = floor(X / 2 w) (a true floor: X may
 *                      be negative, then ix = -1), r = X - ix 2 w, phase k = (32 r) / (2 w) in 0..31
 *       LINEAR         taps ix, ix + 1 with weights 32 - k, k
 *       CUBIC          taps ix - 1 .. ix + 2 with the Q17 Keys weights W0..W3 at phase k of UBD_PHOTO_ELASTIC (they sum to 131072)
 *     tap indices are clamped to 0..gw-1 (replicate border).  The 2-D value is the full double sum over both axes' taps, rounded
 *     once: NEAREST g itself; LINEAR (sum wy wx g + 512) >> 10; CUBIC clamp((sum Wy Wx g + 2^33) >> 34, 0, 32768) (per axis the
 *     sum of |W| is at most 180224 = 1.375 * 2^17, so the sum needs 64 bits and stays below 2^51).
 *   Aggregation: UBD_NA_MAX u = max_i u_i; UBD_NA_AVG u = (sum_i u_i + iterations / 2) / iterations.
 *   Curve: 257 uint16 values T[0..256], each 0..16384 (Q14), at tables + curve_offset (a sigmoid, or T[i] = 64 i for none):
 *     i = u >> 7, f = u & 127, a = T[i] when f = 0, else (T[i] (128 - f) + T[i + 1] f + 64) >> 7 (i = 256 occurs only with f = 0).
 *   Blend, one mask for all channels: out_c = (a F_c + (16384 - a) S_c + 8192) >> 14.
 * descs: HOST array of n descriptors; tables: DEVICE array of table_count uint16 values; offsets into it are in uint16 units.
 * Checked on the host (non-zero return, nothing launched, ubd_last_error() starts with the function's name): null pointers,
 * n >= 1, channels 1 or 3, sides, ranges inside the two buffers, overlaps, branch kinds and parameters, iterations 1..3, grid
 * sides 1..16, the upscale and aggregation codes, every grid and the curve inside table_count.  The table VALUES are on the
 * device and are trusted: a g above 32768 or a T above 16384 is the caller's error (the result is then undefined, though no
 * access leaves the buffers).
 * Enqueues one launch per 24 images; no host synchronisation, capturable in a HIP graph. */
enum { UBD_NA_IDENTITY, UBD_NA_FILTER3, UBD_NA_AFFINE };      /* branch kinds */
enum { UBD_NA_NEAREST, UBD_NA_LINEAR, UBD_NA_CUBIC };         /* upscale methods */
enum { UBD_NA_MAX, UBD_NA_AVG };                              /* aggregation */
typedef struct ubd_noise_alpha_branch {
    int32_t kind;                    /* UBD_NA_IDENTITY / FILTER3 / AFFINE */
    int32_t p[9];                    /* per kind, see above; unused entries 0 */
} ubd_noise_alpha_branch;
typedef struct ubd_noise_alpha_grid {
    int32_t gw, gh;                  /* 1..16 */
    int32_t upscale;                 /* UBD_NA_NEAREST / LINEAR / CUBIC */
    int32_t reserved;                /* 0 */
    int64_t grid_offset;             /* uint16 units from tables to the gh * gw values */
} ubd_noise_alpha_grid;
typedef struct ubd_noise_alpha_desc {
    int64_t src_offset, dst_offset;  /* bytes from src / dst to the image */
    int32_t w, h;
    int32_t iterations;              /* 1..3: how many of grid[] are used */
    int32_t aggregation;             /* UBD_NA_MAX / AVG */
    ubd_noise_alpha_branch first, second;
    ubd_noise_alpha_grid grid[3];
    int64_t curve_offset;            /* uint16 units from tables to T[0..256] */
} ubd_noise_alpha_desc;
int ubd_noise_alpha_images(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes,
                           const ubd_noise_alpha_desc *descs, const uint16_t *tables, size_t table_count,
                           int channels, int n, void *stream);

/* --- object-level evaluation ----------------------------------------------------
 * Replaces FtMetricsCalculator (evaluation.py:168-429: areas, the G x F intersection / IoU tables :210-227, analyze :229-328, the
 * confusion matrix increments :330-362, group IoU :379-387, precision / recall / IoU by area :389-404) for a whole batch and every
 * IoU threshold at once, and the summing half of FtMetrics.append (:53-97): the accumulator holds SUMS, the host forms the
 * running averages from them.  The found objects are the outputs of ubd_postprocess as they lie in device memory.
 * Ground-truth polygons: convex, 3..UBD_EVAL_MAX_VERTS vertices, either winding (normalised on the device); found quads: 4
 * vertices.  All geometry in fp64; areas of unions are exact boundary integrals, not rasterised (tie rules: evaluate.hip).
 *   scales         : device (n, 2) xscale, yscale or NULL: found coordinate = trunc(coordinate * scale) (utils.py:67-69,
 *                    model_runner.py:140-148)
 *   gt_xy          : device, packed x,y of the vertices of all ground-truth polygons of the call (n_gt_vertices vertices)
 *   gt_first       : device (total_gt + 1) first vertex of each polygon; total_gt = gt_image_first[n].  The device checks every
 *                    polygon's vertex range against n_gt_vertices (a range outside it, or not 3..8 vertices, flags the image);
 *                    the length of gt_first itself is the caller's to keep
 *   gt_class       : device (total_gt) class index 0..n_classes-1, or NULL when n_classes == 0
 *   gt_image_first : HOST (n + 1) first polygon of each image; max_gt >= the largest number of polygons of one image
 *   thresholds     : HOST (n_thresholds) doubles, compared as they are (tp needs iou >= t, detection_rate iou_by_area > t)
 *   per_image      : device (n, n_thresholds) records or NULL
 *   accumulator    : device, ubd_evaluate_accumulator_bytes(n_thresholds, n_classes) bytes, zeroed by the caller before the first
 *                    call, as 8-byte slots: [0] int64 images scored, [1] int64 images flagged (not scored), [2..4] double sums of
 *                    precision / recall / IoU by area, [5..7] unused; then 10 slots per threshold: int64 tp, fp, fn, one_to_one,
 *                    one_to_many, many_to_one, matched_boxes_count, detection_rate, double iou_sum, unused; then double
 *                    (n_thresholds, n_classes, n_classes) confusion sums [actual][predicted].
 * Per-image contributions are added in image order by one block: the same calls give the same bits.  An image whose counts[i]
 * exceeds cap (a truncated list, see ubd_postprocess) or whose ground truth is malformed is NOT scored: its records carry
 * flags != 0 and slot [1] counts it.  Limits: n >= 1, polygons per image <= UBD_EVAL_MAX_GT, cap <= UBD_EVAL_MAX_FOUND,
 * n_thresholds <= UBD_EVAL_MAX_THRESHOLDS, n_classes <= UBD_MAX_CLASSES (non-zero return otherwise, nothing launched).
 * Enqueues four launches per 64 images; no host synchronisation, capturable in a HIP graph. */
#define UBD_EVAL_MAX_VERTS 8
#define UBD_EVAL_MAX_GT 256
#define UBD_EVAL_MAX_FOUND 256
#define UBD_EVAL_MAX_THRESHOLDS 16
enum { UBD_EVAL_FLAG_OVERFLOW = 1, UBD_EVAL_FLAG_BAD_GT = 2 };
typedef struct ubd_eval_record {             /* FtMetrics of one image at one threshold (evaluation.py:262-328), sums not averages */
    int32_t tp, fp, fn;
    int32_t one_to_one, one_to_many, many_to_one;
    int32_t matched_boxes_count;
    int32_t detection_rate;                  /* 0 / 1 */
    int32_t n_gt, n_found;
    int32_t flags;                           /* UBD_EVAL_FLAG_*; non-zero: every other counter is 0 */
    int32_t reserved;
    double iou_sum;                          /* sum of the matched IoUs (average_iou * matched_boxes_count) */
    double precision_by_area, recall_by_area, iou_by_area;
} ubd_eval_record;
size_t ubd_evaluate_accumulator_bytes(int n_thresholds, int n_classes);                       /* 0 for sizes outside the limits */
size_t ubd_evaluate_workspace_bytes(int n, int max_gt, int cap, int n_thresholds, int n_classes);   /* 0 for sizes outside the limits */
int ubd_evaluate_objects(const int32_t *quads, const int32_t *classes, const int32_t *counts, int n, int cap,
                         const double *scales, const double *gt_xy, int n_gt_vertices, const int32_t *gt_first,
                         const int32_t *gt_class, const int32_t *gt_image_first, int max_gt,
                         const double *thresholds, int n_thresholds, int n_classes,
                         ubd_eval_record *per_image, void *accumulator, void *workspace, size_t workspace_bytes, void *stream);
/* Diagnostics: where the last ubd_evaluate_objects call with these sizes left its tables in the workspace (the arrays
 * FtMetricsCalculator.__init__ builds, evaluation.py:210-227).  Image i starts at workspace + *offset_bytes + i * *stride_doubles * 8:
 * double areas of the ground truths [max_gt], areas of the found quads [cap], intersections [max_gt][cap], IoU [max_gt][cap]. */
int ubd_evaluate_tables_layout(int n, int max_gt, int cap, int n_thresholds, int n_classes, int64_t *offset_bytes,
                               int64_t *stride_doubles);

/* ubd_evaluate_objects for convex ground-truth polygons of 3..max_verts vertices, max_verts 3..UBD_POLY_MAX_VERTS (hulls read
 * from segmentation maps: ubd_segmap_polygons).  Arguments, accumulator, records, flags, tie rules and the fixed reduction order
 * are those of ubd_evaluate_objects; a polygon with fewer than 3 or more than max_verts vertices flags its image
 * UBD_EVAL_FLAG_BAD_GT.  The workspace keeps max_verts vertices per polygon slot: ubd_evaluate_polygons_workspace_bytes and
 * ubd_evaluate_polygons_tables_layout are the siblings of the two calls above.  On ground truth of at most UBD_EVAL_MAX_VERTS
 * vertices the records and the accumulator are bit-identical to ubd_evaluate_objects'. */
size_t ubd_evaluate_polygons_workspace_bytes(int n, int max_gt, int cap, int n_thresholds, int n_classes, int max_verts);
int ubd_evaluate_polygons(const int32_t *quads, const int32_t *classes, const int32_t *counts, int n, int cap,
                          const double *scales, const double *gt_xy, int n_gt_vertices, const int32_t *gt_first,
                          const int32_t *gt_class, const int32_t *gt_image_first, int max_gt, const double *thresholds,
                          int n_thresholds, int n_classes, int max_verts, ubd_eval_record *per_image, void *accumulator,
                          void *workspace, size_t workspace_bytes, void *stream);
int ubd_evaluate_polygons_tables_layout(int n, int max_gt, int cap, int n_thresholds, int n_classes, int max_verts,
                                        int64_t *offset_bytes, int64_t *stride_doubles);

/* --- pixel classification accuracy (semantic_segmentation/evaluation.py:546-575, _calc_pixel_classification_correctness_mask) ---
 * For n maps of map_h x map_w: pred = argmax over the n_classes class logits of a pixel (np.argmax: first maximum, first NaN),
 * mask = label > 0, true = label - 1 where mask else 0, correct = (true == pred) at every pixel.  Objects are the external
 * 8-connected components of mask (every one, single pixels included); an object's region is its filled contour (enclosed
 * background and nested components included) and its accuracy is the share of correct pixels of the region.
 *   class_logits : device, the first CLASS logit of pixel 0; pixel p's classes are class_logits[p * pixel_stride + 0..n_classes-1]
 *                  (the net's (n, h, w, 1 + n_classes) output: &logits[1] with pixel_stride = n_classes + 1)
 *   labels       : device (n, h, w) int32, the y_true layout of ubd_loss: 0 background, k > 0 class k - 1, negative = background
 *   mask         : device (n, h, w) int8 or NULL: +1 mask & correct, -1 mask & !correct, 0 elsewhere
 *   per_image    : device (n) records or NULL
 *   accumulator  : device, ubd_evaluate_pixels_accumulator_bytes() bytes, zeroed by the caller before the first call, as 8-byte
 *                  slots: [0] int64 n_correct, [1] int64 n_total, [2] int64 n_objects, [3] double sum of the object accuracies,
 *                  [4] int64 images, [5..7] unused.
 * The object accuracies are formed in fp64 and summed in a fixed order (objects by raster position of their first pixel, images
 * in order, one block): the same calls give the same bits.  Limits (non-zero return, ubd_last_error, nothing launched, the
 * accumulator untouched): n >= 1, n_classes 1..31, 1 <= map_h, map_w < 32768 (no multiple-of-4 requirement),
 * pixel_stride >= n_classes.  Any n: the call works through the batch in chunks of less than 2^31 pixels.  Maps of at most
 * 16384 pixels take three launches per chunk (one block per map labels it in LDS), larger maps seven; no host
 * synchronisation, no allocation, capturable in a HIP graph. */
typedef struct ubd_pixel_record {
    int64_t n_correct, n_total;              /* pixels with mask & correct, pixels with mask */
    int64_t n_objects;
    double object_acc_sum;                   /* sum over the image's objects of correct / size */
} ubd_pixel_record;
size_t ubd_evaluate_pixels_accumulator_bytes(void);
size_t ubd_evaluate_pixels_workspace_bytes(int n, int map_h, int map_w);   /* 0 outside the limits */
int ubd_evaluate_pixels(const float *class_logits, int pixel_stride, int n_classes,
                        const int32_t *labels, int n, int map_h, int map_w,
                        int8_t *mask, ubd_pixel_record *per_image,
                        void *accumulator, void *workspace, size_t workspace_bytes, void *stream);

/* --- detection scores and ranked records for average precision (NO reference counterpart: the reference has no confidence of a
 * found object and reports P / R / F1 at one operating point only) -------------------------------------------------------------
 * ubd_score_objects: scores[i][o] = mean detection probability over the REGION of found object o of image i.
 *   logits       : device; pixel p's detection logit is logits[p * pixel_stride] (the net's (n, h, w, K) output: pixel_stride = K)
 *   quads, counts: device, as ubd_postprocess writes them (image coordinates)
 *   scores       : device fp32 (n, cap); slots o >= min(counts[i], cap) are written 0.0f, an image with counts[i] > cap scores
 *                  its first cap entries
 * Region: exactly the map pixels ubd_build_label_maps would paint for the quad at `scale` -- the corners divided by scale and
 * snapped outward (_proper_round, segmap_manager.py:106-133), the polygon filled by ImageDraw.polygon's rule (csrc/raster_fill.h),
 * clipped to the map.  Stated deviation: the region is the found BOX, not the component's filled contour, so a thin diagonal
 * object scores lower than its own pixels alone would.
 * Arithmetic, fixed so that every parallelisation gives the same bits: p = 1.0f / (1.0f + expf(-x)) in fp32, a NaN p counts as 0;
 * q = (uint32_t)rintf(p * 16777216.0f); the q are summed in 64-bit integers; score = (float)((double)sum / (16777216.0 *
 * (double)count)).  An empty region (a box wholly outside the map) scores 0.0f.
 * Non-zero return, ubd_last_error set and nothing launched (all checked before the first HIP call): a null pointer; n, map_h, map_w,
 * cap, scale or pixel_stride below 1; map_h or map_w >= 32768; n * map_h * map_w or n * cap >= 2^31.
 * No handle, no workspace; one launch, no host synchronisation, capturable in a HIP graph.
 *
 * ubd_rank_detections: COCO's greedy matching of every image at every IoU threshold at once, appended to an epoch buffer that is
 * read once per epoch.  NOT the reference's 1-1 / 1-many / many-1 analysis (ubd_evaluate_objects): the average precision formed from
 * these records at a threshold and the precision / recall of ubd_evaluate_objects at the same threshold need not lie on one curve.
 *   scores, counts : device (n, cap) fp32 and (n) int32: ubd_score_objects' output and ubd_postprocess' counts
 *   iou            : device; IoU of ground truth g and found f of image i = iou[i * image_stride_doubles + g * cap + f]: the IoU table
 *                    ubd_evaluate_tables_layout / ubd_evaluate_polygons_tables_layout locate in the workspace of the evaluate call
 *                    just made on the same stream (image start + (max_gt + cap + max_gt * cap) doubles, stride as reported)
 *   gt_counts      : device (n) int32 ground-truth objects per image (rows of the image's table)
 *   thresholds     : HOST (n_thresholds) doubles, compared as they are: a match needs iou >= t
 * Per image: the detections 0 .. counts[i]-1 are taken in descending score, ties to the lower index, a NaN score last.  For every
 * threshold j independently a detection takes the not-yet-taken ground truth with the largest IoU (ties to the lowest g, a NaN IoU
 * never matches); if that IoU is >= t_j the detection is a true positive at j and the ground truth is taken, otherwise it is a false
 * positive and nothing is taken.
 * rank_buffer: device, ubd_rank_buffer_bytes(capacity) bytes, zeroed by the caller once.  Eight int64 slots -- [0] records written,
 * [1] records dropped for lack of capacity, [2] ground-truth objects of the scored images, [3] images scored, [4] images flagged,
 * [5..7] unused -- then `capacity` records {float score; uint32_t tp_mask}, bit j = true positive at threshold j.  An image with
 * counts[i] > cap or gt_counts[i] > UBD_EVAL_MAX_GT is flagged: it writes no record and adds nothing to [2].  Records are appended in
 * image order and inside an image in the ranked order; no atomics on global memory: the same calls give the same bytes.
 * Limits (non-zero return, nothing launched, checked before the first HIP call): non-null pointers, n >= 1, cap 1..UBD_EVAL_MAX_FOUND,
 * n_thresholds 1..UBD_EVAL_MAX_THRESHOLDS, image_stride_doubles >= 1, capacity >= 1.  Two launches, no host synchronisation,
 * capturable in a HIP graph. */
int ubd_score_objects(const float *logits, int pixel_stride, const int32_t *quads, const int32_t *counts,
                      int n, int map_h, int map_w, int cap, int scale, float *scores, void *stream);
size_t ubd_rank_buffer_bytes(int64_t capacity);          /* 0 for capacity < 1 */
int ubd_rank_detections(const float *scores, const int32_t *counts, int n, int cap,
                        const double *iou, int64_t image_stride_doubles, const int32_t *gt_counts,
                        const double *thresholds, int n_thresholds,
                        void *rank_buffer, int64_t capacity, void *stream);

/* --- visualisations (semantic_segmentation/visualizations.py:20-151, Visualizer.compute_visualizations) -------------------
 * The four overlays of a batch in one pass over the image pixels, from what the forward pass, the postprocess and the
 * evaluation left in device memory.  Every overlay is draw_segmentation_map (:138-151), Image.composite(Image.blend(image,
 * solid(color), 0.5), image, mask); for 8-bit images and a 0 / 255 mask that is exactly, per channel,
 * out = (in + color) >> 1 where the mask is set and out = in elsewhere; green = (0, 255, 0), red = (255, 0, 0).
 *   images     : device (n, height, width, channels), channels 1 or 3; a grey image becomes RGB by repeating the channel.
 *                UBD_IN_U8: the pixels as they are.  UBD_IN_F32: the reference's denorm, then astype(uint8):
 *                UBD_PRE_MOBILENET x * 127.5 + 127.5 in fp32 (product and sum rounded separately), UBD_PRE_NONE x itself; both
 *                truncate toward zero.  Values outside [0, 255] are CLAMPED and NaN gives 0: numpy leaves that cast undefined,
 *                this is the project's definition.  Float images must be 4-byte aligned.
 *   maps       : (n, map_h, map_w) each; height = s map_h and width = s map_w for ONE integer s >= 1 (s = 1: the augmentation
 *                preview, s = 4: the net's scale).  A map reaches image size as Image.resize(NEAREST) does for an integer
 *                ratio, map[y / s][x / s].  Any other pair of sizes is refused: the general nearest ratio
 *                floor((x + 0.5) map_w / width) is NOT built.
 *   out_gt                 <- gt_labels (int32): green where the label > 0 (visualize_segmentation_map of the label maps, :108-123)
 *   out_seg_map            <- binary_map (int32, the {0, 1} map of ubd_postprocess): green where the entry > 0
 *   out_postprocessed      <- quads (n, cap, 8) int32 and counts (n), the outputs of ubd_postprocess: green inside every found quad,
 *                             filled at image resolution with ImageDraw.polygon's rule (draw_bboxes / draw_markup :94-135 with
 *                             build_segmentation_map(scale = 1, for_drawing = True); the rule ubd_build_label_maps matches to
 *                             Pillow).  Identical to Pillow on convex quads, which is what ubd_postprocess finds.  Two known
 *                             classes differ, for this call and ubd_build_label_maps alike: a quad whose opposite corners
 *                             coincide, and rare self-intersecting slivers -- (23,17) (16,19) (25,17) (19,18), three rows
 *                             high with two corners in its top row, leaves pixel (22, 17) unset where Pillow sets it
 *                             (csrc/raster_fill.h; tests/test_raster_fill_host.py pins the example).  The quads are in
 *                             the coordinates of `images` and may lie partly or wholly outside them; counts[i] > cap is clamped
 *                             to cap as in ubd_build_label_maps.
 *   out_classification_gt  <- cls_mask (int8, the mask of ubd_evaluate_pixels): green where +1, red where -1 (:82-91)
 * Each output is (n, height, width, 3) uint8.  An output is written if and only if it and its source are non-NULL; an output
 * given without its source is an error; with no output at all the call returns 0 and launches nothing.  Outputs must not
 * overlap the images or each other.  Dword accesses are used where an address is a multiple of 4, bytes elsewhere: any byte
 * alignment of the uint8 tensors works.
 * Limits: n >= 1, sides 1..16384, n * height * width * 3 < 2^31, cap >= 1 with quads.  Every violation returns non-zero with
 * ubd_last_error() set and launches nothing; all of them are checked before the first HIP call.
 * One launch; no host synchronisation, no allocation, capturable in a HIP graph. */
int ubd_visualize_images(const void *images, int in_dtype, int preprocessing, int n, int height, int width, int channels,
                         int map_h, int map_w, const int32_t *gt_labels, const int32_t *binary_map,
                         const int32_t *quads, const int32_t *counts, int cap, const int8_t *cls_mask,
                         uint8_t *out_gt, uint8_t *out_seg_map, uint8_t *out_postprocessed, uint8_t *out_classification_gt,
                         void *stream);

/* --- data parallelism (no reference counterpart: the reference is single-device) -------------------
 * One process per GPU, per-replica loss (losses.py:86-126 applied to the rank's own images), ONE sum all-reduce of the flat
 * fp32 gradient vector per step over RCCL / xGMI, 1/world applied by ubd_adam_step's grad_scale, parameters broadcast once.
 * The handle owns the communicator.  unique_id: 128 HOST bytes created on one rank by ubd_comm_unique_id and handed to all
 * ranks by the caller (file, socket, launcher store).  librccl is resolved with dlopen when the first of these is called. */
#define UBD_UNIQUE_ID_BYTES 128
/* flags of ubd_comm_init.  UBD_COMM_FUSED: ubd_train_step all-reduces `grads` itself (SUM over ranks) -- the dilated + head
 * segment on a communication stream under the stem layers' backward pass, the stem segment on the caller's stream, which
 * then joins the first -- so `grads` come back summed and the caller must NOT call ubd_allreduce_grads again. */
enum { UBD_COMM_FUSED = 1, UBD_COMM_GLOBAL_LOSS = 2 };
/* UBD_COMM_GLOBAL_LOSS: ubd_loss / ubd_train_step evaluate the reductions of losses.py:86-126 -- n_pos, n_neg, the positive /
 * negative means, the top-k of the FLATTENED batch (losses.py:111) and the classification mean -- over the images of all
 * ranks (rank r holds flat indices [r*npix, (r+1)*npix), equal shards), i.e. the reference's loss at the global batch
 * instead of one loss per replica.  The returned loss is the global one on every rank and d loss / d logits is its exact
 * gradient, so the parameter gradients must be SUMMED over the ranks and applied with grad_scale = 1 (not 1/world). */
int ubd_comm_unique_id(void *unique_id_out);
int ubd_comm_init(ubd_handle *h, const void *unique_id, int rank, int world, int flags);   /* collective: every rank calls it */
int ubd_comm_destroy(ubd_handle *h);                                                        /* also done by ubd_destroy */
int ubd_comm_world(const ubd_handle *h);                                                    /* 1 without a communicator */
/* In-place SUM all-reduce of grads[0..count) over the ranks, enqueued on `stream` (replaces nothing in the reference; it is
 * the exchange step between ubd_train_step and ubd_adam_step). */
int ubd_allreduce_grads(ubd_handle *h, float *grads, size_t count, void *stream);
/* params[0..count) of rank `root` to every rank (initial weights / after loading a model on one rank). */
int ubd_broadcast_params(ubd_handle *h, float *params, size_t count, int root, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UBD_H */
