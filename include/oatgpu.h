/*
 * oatgpu.h -- C ABI of liboatgpu.so: the MI355X (gfx950) implementation of Oat's
 * per-frame image hot path
 *
 *      framefilt mog  ->  framefilt col (BGR2HSV)  ->  posidet hsv | thresh
 *
 * Plain pointers and sizes only; no C++ or torch types, no exceptions.  Every
 * entry point names the reference interface it replaces (paths relative to
 * jonnew/Oat).  INTEGRATION.md shows the binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - return 0 on success, a negative OATGPU_E_* code on failure;
 *     oatgpu_last_error() gives the text.
 *   - a pipelined call (oatgpu_track_enqueue*, _sequence_dev, _batch*) whose kernel launches fail half-way is FATAL
 *     for its context: the frame counts, learning-rate schedule and possibly the model have moved ahead of the
 *     results, so every later pipelined call returns OATGPU_E_HIP ("context unusable ...") instead of silently
 *     losing parity with the reference; results already outstanding can be collected, then destroy the context
 *     (the reference's component would have thrown out of process() and exited, framefilter/main.cpp:278-295).
 *   - the caller owns every host buffer; the context owns all device state
 *     (MOG2 model planes, bit masks, label tables, result ring).
 *   - one context per host thread (not re-entrant).  The HIP streams the work is
 *     issued on belong to the device and are shared by all contexts of a process
 *     (DESIGN.md section 4); oatgpu_set_stream makes a context issue its per-pixel
 *     kernel and copies on an external HIP stream instead.
 *   - pixel buffers are packed, rows*cols*channels bytes, no row padding
 *     (lib/datatypes/Frame.h:92-103, lib/shmemdf/Sink.h:289-290).
 *   - "stream" below = one camera stream (an independent Oat pipeline), not a
 *     HIP stream, unless it says HIP.
 */
#ifndef OATGPU_H
#define OATGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OATGPU_ABI_VERSION 9     /* 2: oatgpu_position grew (filter outputs), new entry points; 3: oatgpu_config.mog_restore_nmodes; 4: oatgpu_cvt_color, oatgpu_set_fusion, oatgpu_set_homography, oatgpu_profile.mog_frames; 5: oatgpu_track_sequence_dev_timed, oatgpu_track_enqueue_dev pairs frames only after oatgpu_set_fusion(2); 6: oatgpu_track_input_consumed_stream, oatgpu_track_stage, oatgpu_track_enqueue_staged; 7: oatgpu_track_stage_abort, oatgpu_set_early_blob, oatgpu_set_stage_copy, oatgpu_set_deferred / _fetch_frame / _fetch_position, a failed pipelined launch is fatal for its context; 8: oatgpu_track_sequence_dev_latency, oatgpu_device_open_retries, oatgpu_set_k1_workgroup, oatgpu_last_step_shape, oatgpu_early_blob_timeouts, a parked blob workgroup that times out switches early dispatch off for its context; 9: oatgpu_profile.dropped, every scratch set is allocated by oatgpu_create (an out-of-memory is reported there, never in the middle of a step); additive entries of 9 (detect them by symbol): oatgpu_undistort_map, oatgpu_set_undistort, oatgpu_undistort_filter, oatgpu_undistort_dev, oatgpu_set_track_undistort */
/* Further additive entries of ABI 9 (detect them by symbol; no existing struct or entry changes): the marker sets --
 * oatgpu_set_markers, oatgpu_set_marker_window, oatgpu_track_markers_dev, oatgpu_track_markers, oatgpu_read_marker_mask,
 * with the structs oatgpu_marker and oatgpu_combined; marker sets on the pipelined path -- oatgpu_set_marker_pipeline,
 * oatgpu_track_collect_markers, oatgpu_track_markers_sequence_dev; the filter chain behind the combined record --
 * oatgpu_set_marker_filters, oatgpu_marker_filtered, with the structs oatgpu_region, oatgpu_marker_filters, oatgpu_filtered;
 * the motion tracker -- oatgpu_set_diff_tracker, oatgpu_diff_reset, oatgpu_diff_batch_dev, oatgpu_diff_batch,
 * oatgpu_diff_sequence_dev, oatgpu_read_diff_mask; the subtraction tracker -- oatgpu_set_bsub_tracker, oatgpu_bsub_reset,
 * oatgpu_bsub_track_batch_dev, oatgpu_bsub_track_batch, oatgpu_bsub_track_sequence_dev, oatgpu_bsub_get_state,
 * oatgpu_read_bsub_mask; Bayer RAW8 ingest -- oatgpu_debayer_filter, oatgpu_debayer_dev, oatgpu_set_track_bayer, with the
 * OATGPU_BAYER_* pattern values; RAW8 frames for the motion and the subtraction tracker -- oatgpu_set_tracker_bayer; the filter
 * chain behind the motion and the subtraction tracker -- oatgpu_set_tracker_filters, oatgpu_tracker_filtered; target tracks --
 * oatgpu_set_tracks, oatgpu_tracks, oatgpu_tracks_update, with the struct oatgpu_track; target shapes --
 * oatgpu_set_target_shapes, oatgpu_target_shapes, with the struct oatgpu_shape; target crops -- oatgpu_set_target_crops,
 * oatgpu_target_crops, oatgpu_crop_windows_dev, with the struct oatgpu_crop_window and the OATGPU_CROP_* modes; crop tensors --
 * oatgpu_set_target_crop_tensor, oatgpu_target_crop_tensor_sets, oatgpu_crop_tensor_windows_dev, with the struct
 * oatgpu_crop_tensor_fmt and the OATGPU_TENSOR_* dtypes; target masks -- oatgpu_set_target_mask_tensor,
 * oatgpu_target_mask_tensor_sets. */

enum {
    OATGPU_OK = 0,
    OATGPU_E_INVALID = -1,    /* bad argument / configuration               */
    OATGPU_E_HIP = -2,        /* HIP runtime error (text in last_error)     */
    OATGPU_E_NOMEM = -3,
    OATGPU_E_RING_FULL = -4,  /* track_enqueue without a free result slot   */
    OATGPU_E_RING_EMPTY = -5, /* track_collect with nothing outstanding     */
    OATGPU_E_NODEVICE = -6    /* no usable HIP device                       */
};

/* Context configuration.  Fill with oatgpu_default_config() first; it sets the
 * reference's defaults:
 *   MOG2   cv::createBackgroundSubtractorMOG2() with all defaults
 *          (src/framefilter/BackgroundSubtractorMOG.cpp:82-83)
 *   hsv    HSVDetector.h:77-94 / HSVDetector.cpp:34-47 (all-pass thresholds,
 *          erode off, dilate 10, area [0, DBL_MAX))
 */
typedef struct oatgpu_config {
    int32_t device;            /* HIP device ordinal                          */
    int32_t n_streams;         /* camera streams batched in this context      */
    int32_t rows, cols;        /* frame geometry, identical for all streams   */
    int32_t ring_depth;        /* outstanding track_enqueue results (>=1)     */
    int32_t channels;          /* 3: BGR frames (mog -> col HSV -> posidet hsv)
                                  1: GREY frames (mog -> posidet thresh; -T = h_lo/h_hi) */

    /* --- MOG2 (BackgroundSubtractorMOG.cpp:82-83) --- */
    int32_t history;           /* 500 */
    int32_t nmixtures;         /* 5 (1..5 supported)                          */
    float var_threshold;       /* Tb 16   */
    float background_ratio;    /* TB 0.9  */
    float var_threshold_gen;   /* Tg 9    */
    float var_init;            /* 15      */
    float var_min;             /* 4       */
    float var_max;             /* 75      */
    float ct;                  /* 0.05; must lie in [0, 0.5): OpenCV accepts any value, the kernel relies on a matched
                                  mode (weight >= alpha (1 - ct)) never being prunable (weight < alpha ct) */
    float tau;                 /* 0.5     */
    int32_t detect_shadows;    /* 1       */
    int32_t shadow_value;      /* 127     */

    /* --- detector (HSVDetector.cpp:77-140, SimpleThreshold.cpp:71-112) --- */
    int32_t h_lo, h_hi;        /* -H [min,max] in [0,256]; also -T for thresh */
    int32_t s_lo, s_hi;        /* -S */
    int32_t v_lo, v_hi;        /* -V */
    int32_t erode;             /* -e, 0 = off                                 */
    int32_t dilate;            /* -d, 0 = off                                 */
    double min_area, max_area; /* -a [min,max)                                */

    /* --- posidet diff (DifferenceDetector.h:63-76) --- */
    int32_t diff_threshold;    /* -d, default 10                              */
    int32_t blur;              /* -b, default 2; 0 = off; <= 22 supported     */

    /* --- MOG2 mode count (MOG2Invoker's `nmodes = nNewModes;`) --- */
    int32_t mog_restore_nmodes; /* 1 (default): the per-pixel mode count is set back to its value at
                                  entry after the weight renormalisation, as cv::BackgroundSubtractorMOG2
                                  does -- a pruned mode keeps its slot with weight 0 and modesUsed never
                                  shrinks; 0: a pruned mode leaves the count (round 1's reading).
                                  oracle/mog2.c "Mode count" has the derivation; no OpenCV is available
                                  here to settle it, hence a switch rather than a constant. */
    int32_t reserved_;
} oatgpu_config;

/* What posidet writes into oat::Position2D (src/positiondetector/DetectorFunc.cpp:46,58-60)
 * plus the raw integer Green sums the centroid is derived from. */
typedef struct oatgpu_position {
    int32_t valid;             /* Position2D::position_valid                  */
    int32_t first_pixel;       /* raster index of the blob's first pixel, -1  */
    double x, y;               /* Position2D::position (pixels)               */
    double area;               /* siftContours' area out-parameter            */
    int64_t a00, a10, a01;     /* exact contour sums (cv::moments internals)  */
    /* With oatgpu_set_kalman on (fused track calls only), valid/x/y above are what
     * `posifilt kalman` would hand downstream (Position2D::position_valid/position) and: */
    int32_t velocity_valid;    /* Position2D::velocity_valid (0 when the filter is off) */
    int32_t raw_valid;         /* the detector's own position_valid              */
    double vx, vy;             /* Position2D::velocity (position units / s)      */
    double raw_x, raw_y;       /* the detector's own centroid                    */
} oatgpu_position;

/* Per-stage device time accumulated while profiling is enabled (HIP events on
 * the context's HIP stream). */
typedef struct oatgpu_profile {
    int64_t steps;             /* track steps measured                        */
    double mog_ms;             /* fused MOG2+mask+HSV+inRange kernel          */
    double morph_ms;           /* erode + dilate                              */
    double blob_ms;            /* labelling + contour sums + selection        */
    double total_ms;           /* first event to last event of each step      */
    double event_pair_ms;      /* calibration: elapsed time of an event pair around an EMPTY
                                  kernel on the same HIP stream (what mog_ms contains per step
                                  besides kernel execution); measured at profile_enable */
    int64_t mog_frames;        /* frames the `steps` measured launches of the fused kernel covered
                                  (steps .. 2 * steps, see oatgpu_set_fusion)              */
    int64_t dropped;           /* samples left out: their per-pixel launch read more than 8 x the running average and 1 ms above it -- a host
                                  thread descheduled between the event record and the launch call puts its absence into the
                                  pair; at most 4 in a row (a 5th is a change of regime and is taken)  */
} oatgpu_profile;

typedef struct oatgpu_ctx oatgpu_ctx;

int oatgpu_abi_version(void);
int oatgpu_default_config(oatgpu_config *cfg);

/* Object lifetime == the reference component's (MOG model and scratch are
 * members: BackgroundSubtractorMOG.h:72-73, HSVDetector.h:83).
 * Device memory, all of it allocated HERE (an out-of-memory is OATGPU_E_NOMEM from oatgpu_create, never a failure in the middle of a
 * pipelined step): per camera stream and pixel 101 B of model + 150 B of back-half scratch (five sets of 30 B: three launch orders'
 * worth plus the repair set) + ring_depth / 8 B of threshold words + the staging frame; 1080p: 0.52 GB a stream, 4K: 2.1 GB.  The
 * host-frame path (oatgpu_track_enqueue / _stage) adds ring_depth staging frames on first use.
 * Marker sets add theirs in oatgpu_set_markers (30 B + n_markers / 2 B a pixel and stream) and, for the pipelined marker path, in
 * oatgpu_set_marker_pipeline: per pixel, stream and MARKER 60 B of back-half scratch (TWO sets for M x n planes, one for each
 * frame of a two-frame step; all marker work runs in order on one stream, so no more are needed) + ring_depth / 2 B of per-slot
 * bit planes and taps -- 1.5 GB at 4K and 6.3 GB for 16 x 1080p with three markers and a ring of 4. */
oatgpu_ctx *oatgpu_create(const oatgpu_config *cfg);   /* NULL on failure; oatgpu_last_error(NULL) */
void oatgpu_destroy(oatgpu_ctx *ctx);
const char *oatgpu_last_error(const oatgpu_ctx *ctx);

/* Host-memory helpers for callers that do not link HIP themselves.  Frames handed to the
 * stage-by-stage calls may live anywhere; when they live in page-locked memory (a shared-memory
 * segment registered with oatgpu_host_register, or a buffer from oatgpu_host_alloc) the copies
 * are direct DMA instead of bounce-buffered. */
/* Devices and where they hang: oatgpu_device_count() HIP devices are visible; oatgpu_device_numa_node(i) is the NUMA node
 * of device i's PCIe slot (from its bus id through sysfs), -1 if unknown.  A multi-device component keeps the thread that
 * drives device i on that node's CPUs (host/oat_track_hip.cpp --gpu-index D0,D1,..): its launches, its shared-memory reads
 * and the staging copies then stay on the socket the GPU is attached to.  No reference counterpart. */
int oatgpu_device_count(void);
/* oatgpu_create opens its device with a bounded retry (several processes opening one freshly booted device at the same
 * instant can see the first runtime calls fail transiently); this is how many retries this process has needed so far. */
int oatgpu_device_open_retries(void);
int oatgpu_device_numa_node(int32_t device);
int oatgpu_host_register(void *ptr, size_t bytes);
int oatgpu_host_unregister(void *ptr);
void *oatgpu_host_alloc(size_t bytes);
void oatgpu_host_free(void *ptr);

/* HIP stream plumbing (hipStream_t passed as void*). */
int oatgpu_set_stream(oatgpu_ctx *ctx, void *hip_stream);
void *oatgpu_get_stream(oatgpu_ctx *ctx);
int oatgpu_synchronize(oatgpu_ctx *ctx);

/* Frames per launch of the fused per-pixel kernel on the pipelined path, 1 or 2.  The MOG2 update is a recurrence
 * per pixel, so two consecutive frames of a stream can be taken on ONE pass over its model (kept in registers
 * between them).  With 2, an enqueue only REGISTERS its frame; the kernels are launched when the next frame is
 * enqueued -- or as soon as the frame's result is asked for (oatgpu_track_collect / oatgpu_track_ready reaching
 * that frame, oatgpu_track_input_consumed) or any synchronous entry point runs, then for the one frame alone; a
 * caller that collects every frame before it enqueues the next (oatgpu_track_batch*, a camera-bound component
 * loop) never waits for a second frame.  Results, their order, the threshold images and the model are
 * bit-identical either way (FrameFilter.cpp:59-98 / PositionDetector.cpp:58-99: one token out per token in, in
 * order).
 * DEFAULT (no call): two frames a launch wherever the LIBRARY owns the frame's lifetime -- oatgpu_track_enqueue
 * (host frames: copied to a staging slot inside the call) and oatgpu_track_sequence_dev (all frames handed over at
 * once) -- and ONE frame a launch for oatgpu_track_enqueue_dev, whose kernel is then queued inside the call as it
 * always was, so a caller that reuses its device buffer in stream order stays correct.  oatgpu_set_fusion(2) opts
 * oatgpu_track_enqueue_dev in: from then on a frame handed to it must stay valid and UNTOUCHED until its result
 * was collected or oatgpu_track_input_consumed returned.  oatgpu_set_fusion(1) switches pairing off everywhere.
 * While a traffic audit is on (oatgpu_traffic_audit) GREY contexts launch one frame at a time. */
int oatgpu_set_fusion(oatgpu_ctx *ctx, int32_t frames_per_launch);

/* Early dispatch of the blob-analysis workgroup.  On the pipelined device-frame path of steps of 4 MP and more, the big
 * workgroups that label a step's masks (findContours + moments, DetectorFunc.cpp:41-63) are submitted on a HIP stream of
 * their own together with the step's other kernels and WAIT ON THE DEVICE for their frames' row scans: they take their
 * wave slots while the per-pixel kernel of an earlier frame drains instead of queueing for them on the frame's critical path.
 * on = -1 (the default): by shape -- contexts of at most three streams, whose per-pixel kernel then runs with one wave a
 * workgroup (4K: 18.5 k -> 19.2 k fps; 2 x 1080p: 64.8 k -> 70.3 k; 3 x: 69.3 k -> 72-74 k; four and more lose); 0: never; 1: every eligible step (several streams: row scan + blob analysis beside the
 * per-pixel kernel 16 x 1080p 427 -> 69 us for 1-3 % of the frame rate).  Results are identical either way.
 * Switch it off (0) under tools that serialise kernel dispatches -- a counter-collecting profiler (rocprofv3 --pmc) would
 * let the waiting workgroup run before the row scan it waits for; the kernel then gives up after 100 ms and the frame is
 * redone by the global kernels: correct, but slow. */
int oatgpu_set_early_blob(oatgpu_ctx *ctx, int32_t on);
/* 1 once a parked blob workgroup of this context has given up after 100 ms because its row scan was not dispatched beside it
 * (a tool that serialises kernel dispatches), else 0.  It switches early dispatch off for the context (oatgpu_last_error
 * says so) and raises a flag on the device at which the workgroups parked behind it decline without waiting; all those
 * frames are redone by the global kernels: results are unaffected, and the episode costs its caller 100 ms once. */
int64_t oatgpu_early_blob_timeouts(const oatgpu_ctx *ctx);
/* Threads of a workgroup of the fused per-pixel kernel on the pipelined path: 0 (default) by path -- 64 (one wave a
 * workgroup) where the step's blob workgroup is dispatched early, where a LONE frame (nothing else outstanding) of a
 * context that would use the early order is launched, or the model is dense; 256 otherwise -- or 64 / 256
 * whatever the path.  Results are identical.  For profiling the shipped instantiation under a tool that needs
 * oatgpu_set_early_blob(0) (bench.py's counter passes). */
int oatgpu_set_k1_workgroup(oatgpu_ctx *ctx, int32_t threads);
/* How the latest pipelined step was launched: threads of a per-pixel workgroup (0 before the first step) and whether its
 * blob workgroup was dispatched early.  Either pointer may be NULL. */
int oatgpu_last_step_shape(const oatgpu_ctx *ctx, int32_t *k1_workgroup, int32_t *early_blob);
/* Image rows a workgroup of the row scan takes on the pipelined path.  4 rows deliver a frame's result soonest; 16 rows are
 * fewer, longer workgroups beside the per-pixel kernel, which then runs ~3 % faster at 4K, and a result that comes up to
 * ~85 us later (4K; ~28 us at 1080p).  rows = 0 (the default): by pipeline depth -- 16 on a step launched while at least four
 * earlier frames are still uncollected (results are collected in order: nobody can be waiting for that step's), 4 otherwise;
 * a caller that keeps a ring of 2 or 4, or one frame at a time, always gets 4.  rows = 4 / 16: that height on every eligible
 * step whatever the depth.  Eligible: a step of the early or the paired order whose fused erosion fits the row scan's LDS at
 * 16 rows ((16 + max(dilate, 1) - 1) x 8-byte words of a row <= 64 KiB); every other step takes 4.  Other values are refused.
 * Results are identical either way. */
int oatgpu_set_rowscan_rows(oatgpu_ctx *ctx, int32_t rows);
/* Rows a row-scan workgroup of the latest pipelined step took (0 before the first step). */
int oatgpu_last_step_rowscan_rows(const oatgpu_ctx *ctx);

/* Re-configure the detector between frames (what the reference's tuning GUI
 * mutates: HSVDetector.cpp:175-251). */
int oatgpu_set_detector(oatgpu_ctx *ctx, int32_t h_lo, int32_t h_hi, int32_t s_lo, int32_t s_hi,
                        int32_t v_lo, int32_t v_hi, int32_t erode, int32_t dilate,
                        double min_area, double max_area);

/* `posifilt kalman` (src/positionfilter/KalmanFilter2D.cpp:63-141) applied to every stream's
 * detections inside the fused track calls (oatgpu_track_batch/_dev/_enqueue_dev), on the device,
 * in frame order.  dt: --dt (s, default 0.02); timeout: --timeout (s, default 0 -- with which the
 * reference's filter never tracks); sigma_accel: --sigma-accel (default 5); sigma_noise:
 * --sigma-noise (default 0).  All must be >= 0 and dt > 0 (TOMLSanitize lower bound 0).  Calling it
 * (re)starts every stream's filter from the reference's initial state; enable = 0 turns it off.
 * The single-stage oatgpu_detect_* calls are never filtered.  OATGPU_E_INVALID -- nothing has changed -- while results are
 * outstanding (oatgpu_track_enqueue*): a filter restarted between a frame's enqueue and its collect would have no frame order. */
int oatgpu_set_kalman(oatgpu_ctx *ctx, int32_t enable, double dt, double timeout, double sigma_accel,
                      double sigma_noise);

/* `posifilt homography` on the batch (src/positionfilter/HomographyTransform2D.cpp:62-107) behind the detector and,
 * when it is on, the position filter: every result of the fused track calls goes through cv::perspectiveTransform with
 * the row-major 3x3 matrix h9 (--homography [h11,h12,...,h33], :44-58) -- position where valid, velocity where valid
 * with the matrix' offsets zeroed (:79-89).  raw_x / raw_y keep the detector's pixels.  The caller marks the
 * Position2D it publishes as WORLD units with this matrix (Position2D::setCoordSystem, :102).  enable = 0: off.
 * OATGPU_E_INVALID -- nothing has changed -- while results are outstanding (it is applied when a result is collected). */
int oatgpu_set_homography(oatgpu_ctx *ctx, int32_t enable, const double *h9);

/* `framefilt mask` fused in front of mog (src/framefilter/FrameMasker.cpp:71-75:
 * frame.setTo(0, roi_mask == 0)): roi_mask is rows*cols bytes, nonzero = keep; NULL removes the
 * mask of that stream.  Applies to oatgpu_mog_apply / _filter and the fused track calls. */
int oatgpu_set_roi_mask(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *roi_mask);

/* BackgroundSubtractor::filter (`framefilt bsub`, src/framefilter/BackgroundSubtractor.cpp:87-100):
 * the first frame of a camera stream becomes its background; alpha > 0 adapts it
 * (cv::accumulateWeighted); out = in - background, saturating.  rows*cols*channels bytes; out may
 * equal in. */
int oatgpu_bsub_filter(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *frame_in, uint8_t *frame_out,
                       double alpha);

/* `framefilt bsub -f FILE` (BackgroundSubtractor.cpp:63-71): the background image of stream s comes from
 * the caller (rows*cols*channels bytes) instead of the first frame.  As in the reference it cannot adapt
 * afterwards (its fp32 accumulator is never made): oatgpu_bsub_filter with alpha > 0 then fails. */
int oatgpu_bsub_set_background(oatgpu_ctx *ctx, int32_t stream, const uint8_t *image);

/* FrameMasker::filter (FrameMasker.cpp:71-75) as a stage of its own: out = in where the ROI of stream s
 * (oatgpu_set_roi_mask) is non-zero, 0 elsewhere; without a ROI the frame passes unchanged.  In place allowed. */
int oatgpu_mask_filter(oatgpu_ctx *ctx, int32_t stream, const uint8_t *in, uint8_t *out);

/* Threshold::filter (`framefilt thresh`, src/framefilter/Threshold.cpp:67-81): grey conversion for BGR
 * contexts, inRange [i_min, i_max] (0..256), pixels outside are zeroed.  out may equal in. */
int oatgpu_thresh_filter(oatgpu_ctx *ctx, const uint8_t *frame_in, uint8_t *frame_out, int32_t i_min,
                         int32_t i_max);

/* Undistorter::filter (`framefilt undistort`, src/framefilter/Undistorter.cpp:83-88): cv::undistort(frame, K, D) of OpenCV 3.1
 * with no new camera matrix -- the map of initUndistortRectifyMap (CV_16SC2, built in cv::undistort's stripes of
 * max(1, 4096 / cols) rows) and remap(INTER_LINEAR, BORDER_CONSTANT 0) in its fixed point, on 8-bit GREY or BGR frames.
 * K: the camera matrix, row-major [K11, K12, ..., K33] (--camera-matrix); dist: k1, k2, p1, p2, k3[, k4, k5, k6]
 * (--distortion-coeffs).  n_dist must be 5 or 8: fewer than 5 or more than 8 fail with the reference's text
 * (Undistorter.cpp:61-62); 6 and 7 pass the reference's check but OpenCV 3.1 asserts on them at the first frame, so they are
 * refused here.
 *
 * oatgpu_undistort_map: the map alone, on the host, without a device or a context -- exactly OpenCV's two planes:
 * map1 rows*cols*2 shorts (sx, sy), map2 rows*cols fractions (fy*32 + fx, in 1/32 px). */
int oatgpu_undistort_map(int32_t rows, int32_t cols, const double K[9], const double *dist, int32_t n_dist,
                         int16_t *map1, uint16_t *map2);
/* The map of camera stream s, built on the host once (cv::undistort rebuilds the same map every frame) and kept on the
 * device; the first call allocates the context's map planes (6 B a pixel and stream).  n_dist = 0 removes the stream's map.
 * Each stream may have its own calibration. */
int oatgpu_set_undistort(oatgpu_ctx *ctx, int32_t stream, const double K[9], const double *dist, int32_t n_dist);
/* One frame of stream s (rows*cols*channels bytes); out may equal in (the reference clones first).  OATGPU_E_INVALID when
 * the stream has no map. */
int oatgpu_undistort_filter(oatgpu_ctx *ctx, int32_t stream, const uint8_t *in, uint8_t *out);
/* Throughput form: one frame for EVERY stream, device memory, stream-major (as oatgpu_track_batch_dev), in ONE kernel launch
 * on the context's stream; returns once it is queued (oatgpu_synchronize / the stream from oatgpu_get_stream order the
 * caller's work behind it).  Every stream needs a map; out_dev must not overlap frames_dev. */
int oatgpu_undistort_dev(oatgpu_ctx *ctx, const void *frames_dev, void *out_dev);
/* framefilt undistort INSIDE the fused tracker (default off).  With on = 1 every fused track call (oatgpu_track_batch,
 * _batch_dev, _enqueue, _enqueue_dev, _stage / _enqueue_staged, _sequence_dev and its _timed / _latency forms) remaps each
 * stream's frame with that stream's map (oatgpu_set_undistort) before anything else: the chain is undistort -> ROI mask
 * (so the mask is defined on the UNDISTORTED image) -> MOG2 -> colour -> detector -> position filter -> homography.  One
 * remap launch a step covers every stream and both frames of a two-frame step; the per-pixel kernel then reads the
 * context's undistorted copy.  on = 1 fails (OATGPU_E_INVALID, naming the stream) if any stream has no map; while it is on,
 * oatgpu_set_undistort(s, ..., n_dist = 0) is refused, a recalibration is allowed (it drains outstanding work and takes
 * effect from the next frame).  The call drains outstanding work; on = 1 allocates two undistorted-frame buffers of
 * n_streams*rows*cols*channels bytes each the first time (an out-of-memory is reported here, never in the middle of a
 * step).  With it off nothing changes, maps or none; the stage-by-stage calls never look at it.  oatgpu_track_input_consumed
 * keeps its rule for device frames: it returns once the step's per-pixel kernel has finished, which runs behind the remap
 * that read the caller's frame. */
int oatgpu_set_track_undistort(oatgpu_ctx *ctx, int32_t on);

/* ---- Bayer RAW8 -> BGR: the frame server's pixel-format conversion (src/frameserver/PointGreyCam.cpp:48-50, :729) ----
 *
 * Input rows x cols bytes, one sample a pixel; output rows x cols x 3 bytes BGR.  A pattern is named by the 2 x 2 tile at
 * image rows 0-1, columns 0-1 read row by row (the camera vendors' convention); OpenCV names the tile at rows 1-2, columns
 * 1-2, so RGGB is COLOR_BayerBG2BGR, BGGR COLOR_BayerRG2BGR, GRBG COLOR_BayerGB2BGR and GBRG COLOR_BayerGR2BGR.
 * Interior pixels (1 <= y <= rows - 2, 1 <= x <= cols - 2), 32-bit integer sums: at an R or B site the own colour is the
 * sample, G = (N + S + W + E + 2) >> 2, the opposite colour = (NW + NE + SW + SE + 2) >> 2; at a G site G is the sample, the
 * colour of the horizontal neighbours = (W + E + 1) >> 1, of the vertical ones = (N + S + 1) >> 1.  Output (y, x) is the
 * interior triple of (clamp(y, 1, rows - 2), clamp(x, 1, cols - 2)) with that pixel's own site colours.  rows < 3 or
 * cols < 3 is refused. */
#define OATGPU_BAYER_RGGB 1      /* R G / G B */
#define OATGPU_BAYER_BGGR 2      /* B G / G R */
#define OATGPU_BAYER_GRBG 3      /* G R / B G */
#define OATGPU_BAYER_GBRG 4      /* G B / R G */
/* One host frame, synchronous (deferrable like the other frame filters). */
int oatgpu_debayer_filter(oatgpu_ctx *ctx, int32_t pattern, const uint8_t *raw_in, uint8_t *bgr_out);
/* One frame for EVERY stream in device memory, stream-major: n_streams*rows*cols bytes in, n_streams*rows*cols*3 out; one
 * launch (one per 64 streams) on the context's stream, returns once queued, as oatgpu_undistort_dev.  n_patterns is 1 (one
 * pattern for all) or n_streams.  bgr_dev must not overlap raw_dev. */
int oatgpu_debayer_dev(oatgpu_ctx *ctx, const int32_t *patterns, int32_t n_patterns, const void *raw_dev, void *bgr_dev);
/* Bayer frames INSIDE the fused tracker (default off; NULL / 0 turns it off).  While on, every fused track call
 * (oatgpu_track_batch, _batch_dev, _enqueue, _enqueue_dev, _stage / _enqueue_staged, _sequence_dev and its _timed / _latency
 * forms, oatgpu_track_markers[_dev], _markers_sequence_dev and the marker pipeline) takes RAW8 frames -- rows*cols bytes a
 * stream for host frames, n_streams*rows*cols stream-major for device frames -- and host -> device copies move that many
 * bytes.  The chain is demosaic -> [undistort] -> ROI mask -> MOG2 -> colour -> detector -> filters: one demosaic launch a
 * step covers every stream and both frames of a two-frame step, into two BGR buffers of the context that the remap or the
 * per-pixel kernel then reads.  The call drains outstanding work and allocates those buffers (2 x n_streams*rows*cols*3
 * bytes) the first time: an out-of-memory is reported here, never in the middle of a step.  Refused (OATGPU_E_INVALID)
 * before anything has moved: channels != 3, a pattern outside 1..4, n_patterns neither 1 nor n_streams, frames smaller than
 * 3 x 3, a partly staged frame set.  While it is on the diff and bsub tracker calls are refused; the stage-by-stage calls
 * never look at it; with it off nothing changes.  oatgpu_track_input_consumed[_stream] keep their rules.  RAW8 frames for
 * the diff and bsub trackers are a switch of their own: oatgpu_set_tracker_bayer below. */
int oatgpu_set_track_bayer(oatgpu_ctx *ctx, const int32_t *patterns, int32_t n_patterns);
/* Bayer RAW8 frames for the motion and the subtraction tracker of the context (default off; NULL / 0 turns it off).  While
 * on, oatgpu_diff_batch, _batch_dev, oatgpu_diff_sequence_dev, oatgpu_bsub_track_batch, _batch_dev and
 * oatgpu_bsub_track_sequence_dev take RAW8 frames -- rows*cols bytes a stream for host frames (that many bytes are
 * uploaded), n_streams*rows*cols stream-major for device frames.  n_patterns is 1 (one pattern for all) or n_streams.  The
 * chain is demosaic -> ROI mask -> (col GREY -> diff) or (bsub -> col HSV -> window): the front kernel demosaics its pixels
 * in registers with exactly the arithmetic above, no BGR frame is written, and the ROI falls on the demosaiced pixel.
 * Results, taps and state are bit-identical to oatgpu_debayer_dev followed by the BGR call.  The state -- the last grey
 * image, the BGR background and its fp32 accumulator -- stays in the demosaiced domain and shared with oatgpu_detect_diff,
 * oatgpu_bsub_filter, oatgpu_bsub_set_background (a BGR image) and oatgpu_bsub_get_state, which never look at the switch;
 * turning it on or off between steps keeps the state: a stream fed RAW8 on one step and BGR on the next continues as one
 * stream.  Refused (OATGPU_E_INVALID) with nothing changed: channels != 3, a pattern outside 1..4, n_patterns neither 1
 * nor n_streams, frames smaller than 3 x 3, results outstanding, a partly staged frame set, oatgpu_set_tracker_undistort
 * on.  Independent of oatgpu_set_track_bayer: while THAT is on the diff and bsub calls stay refused.  With it off nothing
 * changes. */
int oatgpu_set_tracker_bayer(oatgpu_ctx *ctx, const int32_t *patterns, int32_t n_patterns);
/* framefilt undistort for the motion and the subtraction tracker of the context (default off).  While on, oatgpu_diff_batch,
 * _batch_dev, oatgpu_diff_sequence_dev, oatgpu_bsub_track_batch, _batch_dev and oatgpu_bsub_track_sequence_dev remap every
 * stream's frame with that stream's map (oatgpu_set_undistort) INSIDE the front kernel: the lane loads the map entries of its
 * own pixels -- once for both frames of a paired launch -- and gathers them from the caller's frame; no undistorted frame is
 * written and nothing is allocated.  The chain is undistort -> ROI mask (the mask is defined on the UNDISTORTED image) ->
 * (col GREY -> diff) or (bsub -> col HSV -> window): B, G and R are remapped each on its own (INTER_LINEAR, border constant
 * 0: a pixel whose source lies off the frame is (0, 0, 0)) and the grey, the difference and the window are taken of the
 * remapped triple.  Results, taps and state are bit-identical to oatgpu_undistort_dev followed by the same call.  The
 * sequence calls keep their pairing rules and four frames in flight.  The state -- the last grey image, the background and
 * its fp32 accumulator, the first-frame flags -- stays in the undistorted domain and shared with oatgpu_detect_diff,
 * oatgpu_bsub_filter, oatgpu_bsub_set_background (an image in undistorted coordinates) and oatgpu_bsub_get_state, which never
 * look at the switch; turning it on or off between steps keeps the state: steps with the switch on and off continue one
 * another.  Refused (OATGPU_E_INVALID) with nothing changed: on outside 0 / 1, on = 1 while any stream has no map (naming
 * the stream) or while oatgpu_set_tracker_bayer is on (RAW8 and undistortion together are not supported: the gather would
 * demosaic four corners a pixel), results outstanding, a partly staged frame set.  While it is on,
 * oatgpu_set_undistort(s, ..., n_dist = 0) is refused; a recalibration is allowed, drains outstanding work and takes effect
 * from the next frame.  Independent of oatgpu_set_track_undistort: while THAT is on the diff and bsub calls stay refused,
 * as they do with the position filter or a homography on.  With it off nothing changes. */
int oatgpu_set_tracker_undistort(oatgpu_ctx *ctx, int32_t on);

/* ---- marker sets: several colour windows per camera behind ONE MOG2 pass, `posicom mean` behind them ----
 *
 * The canonical rig: an animal wearing two or three coloured LEDs, one `framefilt mog`, one `framefilt col`, ONE `posidet hsv`
 * PER COLOUR (HSVDetector.cpp:142-173) and `posicom mean --heading-anchor i` behind them
 * (src/positioncombiner/MeanPosition.cpp:60-118): position = mean of the markers, heading = direction from the anchor marker
 * to the others.  MOG2 does not depend on the detector, so one model pass serves every marker.
 *
 * How: the context's OWN window must be the NON-ZERO window -- H [0,256], S [0,256], V [1,256] (channels == 1: intensity
 * h_lo/h_hi = [1,256]; erode / dilate / area are free).  Its threshold plane (OATGPU_TAP_THRESHOLD) is then Z = "the pixel
 * of the frame `framefilt mog` published is non-zero"; a foreground pixel that is pure black is a zero in that frame like any
 * background pixel, so Z ? px : 0 IS that frame and marker m's mask is inRange_m(hsv(Z ? px : 0)), hsv(0) = (0,0,0) -- a
 * window that contains (0,0,0) selects the background, as in the reference.  One small kernel makes all M masks from the
 * frame the per-pixel kernel read and Z; each mask then goes through the ordinary morphology + blob analysis with its
 * marker's erode / dilate / area; a last kernel combines each camera's M positions.
 *
 * oatgpu_marker: one marker's detector.  Windows as oatgpu_set_detector's (0..256, lo > hi = empty; channels == 1: h_lo/h_hi
 * are the intensity window, s_* / v_* ignored). */
typedef struct oatgpu_marker {
    int32_t h_lo, h_hi, s_lo, s_hi, v_lo, v_hi;
    int32_t erode, dilate;         /* -e / -d of this marker's posidet, 0 = off */
    double min_area, max_area;     /* -a [min,max)                              */
} oatgpu_marker;
/* What `posicom mean` publishes for one camera (oat::Position2D).  MeanPosition::combine is kept as it is: x, y add
 * (1.0 / M) * position of every VALID marker in marker order, position_valid is 0 as soon as one marker is invalid (x, y are
 * then the partial sum); with a heading anchor (hx, hy) adds position_m - position_anchor while the running position_valid is
 * still set (an invalid position is (0, 0)) and heading_valid goes 0 otherwise; the sum is then divided by its length --
 * NaN for M = 1 or coincident markers, with heading_valid 1, as the reference.  Without an anchor heading_valid = 0
 * (detectors set no heading); velocity_valid = 0: this record is what `posicom mean` publishes, BEFORE any position filter --
 * the chain of oatgpu_set_marker_filters leaves it as it is and publishes a record of its own (oatgpu_filtered).
 * n_valid: markers found. */
typedef struct oatgpu_combined {
    int32_t position_valid, heading_valid, velocity_valid, n_valid;
    double x, y, hx, hy;
} oatgpu_combined;
/* Switches marker sets on with n_markers (1..8) markers, the same defaults[m] for every camera, and allocates everything a
 * marker step needs (one more back-half scratch set of 30 B a pixel and stream + n_markers / 2 B of bit planes; an
 * out-of-memory is OATGPU_E_NOMEM from THIS call, never from a step).  heading_anchor: -1 none, else a marker index < n_markers
 * (`posicom mean --heading-anchor`).  n_markers = 0 frees it all and switches markers off (defaults may be NULL).  Drains
 * outstanding work.  The ordinary track calls do not look at any of it. */
int oatgpu_set_markers(oatgpu_ctx *ctx, int32_t n_markers, const oatgpu_marker *defaults, int32_t heading_anchor);
/* The COLOUR window of one marker for one camera (16 cameras do not have 16 identical lighting conditions): takes m's six
 * threshold values; erode / dilate / area stay per marker (m's are ignored). */
int oatgpu_set_marker_window(oatgpu_ctx *ctx, int32_t stream, int32_t marker, const oatgpu_marker *m);
/* One synchronous step: one frame for EVERY stream (device memory, stream-major, as oatgpu_track_batch_dev), the model
 * advances by one frame with oatgpu_track_batch_dev's learning_rate rule.  fg[n_streams] (or NULL): what oatgpu_track_batch_dev
 * returns under the non-zero window -- the largest foreground blob of each camera; markers[s * n_markers + m]: marker m of
 * camera s (`posidet hsv` number m); mean[n_streams] (or NULL): the combined positions.  With oatgpu_set_track_undistort(1)
 * and / or a ROI mask the markers see the undistorted, masked frame, as the model does.
 * OATGPU_E_INVALID -- before anything has moved -- when results are outstanding (oatgpu_track_enqueue*), markers are not
 * configured, the context's own window is not the non-zero window, or oatgpu_set_kalman / oatgpu_set_homography is on (those
 * two act on the foreground result of the plain track calls; the filters of a marker rig are oatgpu_set_marker_filters, which
 * runs behind the combined record of this step and of every pipelined form).
 * Two-frame launches, the result ring and the early blob dispatch do not extend to markers. */
int oatgpu_track_markers_dev(oatgpu_ctx *ctx, const void *frames_dev, double learning_rate, oatgpu_position *fg,
                             oatgpu_position *markers, oatgpu_combined *mean);
/* Same with the frames in host memory: frames_host[i] -> rows*cols*channels bytes of stream i, n == n_streams. */
int oatgpu_track_markers(oatgpu_ctx *ctx, const uint8_t *const *frames_host, int32_t n, double learning_rate,
                         oatgpu_position *fg, oatgpu_position *markers, oatgpu_combined *mean);
/* oatgpu_read_mask for marker m's masks of the latest marker step: which = OATGPU_TAP_THRESHOLD (its inRange output),
 * _MORPH, _FINAL; rows*cols bytes {0,255}. */
int oatgpu_read_marker_mask(oatgpu_ctx *ctx, int32_t stream, int32_t marker, int32_t which, uint8_t *out);
/* Marker sets on the PIPELINED path (default off).  on = 1 is refused -- before anything has moved, with the synchronous step's
 * messages -- when results are outstanding, markers are not configured, the context's own window is not the non-zero window, or
 * oatgpu_set_kalman / oatgpu_set_homography is on (the filters of a marker rig are oatgpu_set_marker_filters: allowed with
 * this switch on or off, in either order).  It allocates everything the path needs (sizes: oatgpu_create's note): per
 * ring slot the M bit planes and every marker's tmp / morph / fin planes, ring_depth host-mapped record sets (M x n_streams result
 * records + n_streams combined records + n_streams filtered records), events, and two back-half scratch sets for M x n_streams planes; an out-of-memory is
 * OATGPU_E_NOMEM from THIS call and leaves an ordinary, working context.  on = 0 frees it all (refused while results are
 * outstanding).
 * While it is on, EVERY pipelined entry point (oatgpu_track_enqueue_dev, _enqueue, _stage + _enqueue_staged, the
 * oatgpu_track_sequence_dev family) also queues the marker work of its frames -- the marker masks from the frames the per-pixel
 * kernel read, ONE back half for all markers, the combiner -- with no host synchronisation and no copy back added;
 * oatgpu_track_ready reports a frame set ready when its marker results are, too; oatgpu_track_collect returns the foreground
 * result alone and retires the marker results with the slot; oatgpu_track_input_consumed[_stream] covers the marker kernel's
 * reads of the frames.  Marker steps take the paired or the plain launch order, never the early one.  The
 * synchronous oatgpu_track_markers[_dev] keep working between drained runs.  REFUSED while it is on (switch it off first):
 * oatgpu_set_markers, enabling oatgpu_set_kalman / oatgpu_set_homography, an oatgpu_set_detector that moves the own window
 * away from the non-zero window.  oatgpu_set_marker_window stays allowed (it drains first).
 * oatgpu_read_marker_mask reads the planes of the frame set COLLECTED last -- pipelined or synchronous, whichever was later. */
int oatgpu_set_marker_pipeline(oatgpu_ctx *ctx, int32_t on);
/* oatgpu_track_collect for such a context: the oldest outstanding frame set, in enqueue order.  fg[n_streams] (or NULL),
 * markers[s * n_markers + m], mean[n_streams] (or NULL) as in oatgpu_track_markers_dev.  OATGPU_E_INVALID when the switch is off,
 * OATGPU_E_RING_EMPTY with nothing outstanding. */
int oatgpu_track_collect_markers(oatgpu_ctx *ctx, oatgpu_position *fg, oatgpu_position *markers, oatgpu_combined *mean);
/* The marker counterpart of oatgpu_track_sequence_dev (the library owns the frames' lifetime: two frames a launch by default):
 * fg[t * n_streams + s] (or NULL), markers[(t * n_streams + s) * n_markers + m], mean[t * n_streams + s] (or NULL). */
int oatgpu_track_markers_sequence_dev(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames, double learning_rate,
                                      oatgpu_position *fg, oatgpu_position *markers, oatgpu_combined *mean);

/* ---- the filter chain behind the combined record: `posifilt kalman` -> `posifilt homography` -> `posifilt region` ----
 *
 * What a marker rig's user records: the token `posicom mean` publishes goes through `posifilt kalman` (bridges frames where an
 * LED is occluded, adds a velocity), `posifilt homography` (metres) and `posifilt region` (which arm of the maze).  The chain
 * runs on the device, in frame order, in ONE launch behind the combiner -- on the synchronous marker step and on every
 * pipelined form -- in this fixed order; each member is switched on its own.  Input per camera and frame is the oatgpu_combined
 * record, which stays as it is; with no chain configured nothing is launched.  oatgpu_set_kalman / oatgpu_set_homography are a
 * different thing (the foreground result of plain track calls) and stay refused on marker contexts.
 *
 * kalman      KalmanFilter2D::filter as oatgpu_set_kalman has it, fed (position_valid, x, y) of the combined record: a
 *             partial-sum x, y under position_valid == 0 is not a measurement.  position_valid = velocity_valid = found,
 *             position / velocity = the reported state (6.0 before the first track, the every-sample timeout test, the stale
 *             measurement, the predicted state: all kept).  The heading passes through.  One filter state per camera stream,
 *             separate from oatgpu_set_kalman's.
 * homography  HomographyTransform2D::filter (HomographyTransform2D.cpp:63-106): the position where valid; the velocity and
 *             the heading where valid through the matrix with its offsets zeroed; the heading is then normalised as
 *             cv::normalize does a one-element vector -- multiplied by the reciprocal of its length (by 0 where the length is
 *             not above DBL_EPSILON).  A NaN heading (one marker, coincident markers) becomes (0, 0), heading_valid still 1.
 * region      RegionFilter2D::filter (RegionFilter2D.cpp:130-152) where position_valid: the position converted as
 *             (cv::Point) does (cvRound per coordinate, ties to even), every configured vertex converted the same way, then
 *             cv::pointPolygonTest(contour, pt, false) >= 0 (the boundary counts as inside) in 64-bit integers.  The regions
 *             are tested IN THE ORDER GIVEN and the first hit wins -- the reference iterates a cpptoml table, an unordered map,
 *             so its order for overlapping regions is unspecified.  A coordinate that is not finite or beyond int32 after
 *             rounding matches no region.  At most 16 regions of at most 64 points; a name takes at most 9 bytes (the
 *             reference's strcpy overruns its 10-byte field with more); a vertex beyond +-32767 after rounding is refused. */
typedef struct oatgpu_region {
    char name[10];
    int32_t n_points;
    const double *xy;              /* n_points pairs x, y */
} oatgpu_region;
typedef struct oatgpu_marker_filters {
    int32_t kalman;                /* 0: off */
    double dt, timeout, sigma_accel, sigma_noise;      /* as oatgpu_set_kalman's, same checks */
    int32_t homography;            /* 0: off */
    double h[9];                   /* row-major */
    int32_t n_regions;             /* 0: off */
    const oatgpu_region *regions;
} oatgpu_marker_filters;
typedef struct oatgpu_filtered {
    int32_t position_valid, velocity_valid, heading_valid, region_valid;
    int32_t region /* -1: none */, reserved_;
    double x, y, vx, vy, hx, hy;
} oatgpu_filtered;
/* Configures the chain.  f = NULL, or all three members off, switches it off.  A successful call (re)starts every stream's
 * Kalman state from the reference's initial state.  OATGPU_E_INVALID, with nothing changed, when results are outstanding,
 * markers are not configured, a limit above is exceeded, a name is too long or a Kalman parameter is out of range.  Allowed
 * with the marker pipeline on or off, in either order.  Every successful oatgpu_set_markers drops the chain. */
int oatgpu_set_marker_filters(oatgpu_ctx *ctx, const oatgpu_marker_filters *f);
/* The filtered records of the frame sets the LATEST marker-result call delivered: one set for oatgpu_track_markers[_dev] and
 * oatgpu_track_collect_markers, n_frames sets for oatgpu_track_markers_sequence_dev; out[t * n_streams + s].  Returns the
 * number of sets written; OATGPU_E_INVALID when no chain is configured, no marker result has been delivered since it was, or
 * max_sets is too small.  Nothing is consumed: the call may be repeated.  The chain advances for every frame whether or not
 * this is called; oatgpu_track_collect on a marker-pipeline context retires the slot's filtered record with the slot. */
int oatgpu_marker_filtered(oatgpu_ctx *ctx, oatgpu_filtered *out, int32_t max_sets);

/* ---- the same chain behind the motion and the subtraction tracker ----
 *
 * What a marker-less rig's user records: `posidet diff` (or `framefilt bsub` -> `posidet hsv`) -> `posifilt kalman` (a velocity,
 * and the frames bridged where the animal stood still or was hidden) -> `posifilt homography` -> `posifilt region`.  While a
 * chain is configured, every frame of oatgpu_diff_batch, _batch_dev, oatgpu_diff_sequence_dev, oatgpu_bsub_track_batch,
 * _batch_dev and oatgpu_bsub_track_sequence_dev advances it by one sample per camera stream, in frame order: one launch a frame
 * on the device, behind that frame's blob analysis; inside the sequence calls, with four frames in flight on three HIP streams,
 * the launches of consecutive frames are ordered by events -- nothing waits on the device.  Batch calls and sequence calls,
 * and the two trackers, continue one another: the chain and its one filter state per camera stream are the CONTEXT's -- not
 * oatgpu_set_kalman's and not the marker chain's.
 *
 * The members, their order, their switches and the limits are those of oatgpu_set_marker_filters above; the input per camera
 * and frame is the detector's result (valid, and the centroid of the integer sums exactly as oatgpu_position.x / .y).  An
 * invalid detection is no measurement.  A detector publishes no heading: heading_valid = 0, hx = hy = 0.  With kalman off an
 * invalid detection gives position_valid = 0, x = y = vx = vy = 0 and no region.
 *
 * The oatgpu_position results of those calls, their taps and their state are bit for bit what they are without a chain.
 * oatgpu_detect_diff, oatgpu_bsub_filter, the MOG2 track calls and the marker calls never look at the chain;
 * oatgpu_set_tracker_bayer, oatgpu_set_tracker_undistort, oatgpu_diff_reset, oatgpu_bsub_reset and oatgpu_bsub_set_background
 * do not touch the filter state.  oatgpu_set_kalman / oatgpu_set_homography keep their meaning (the foreground result of plain
 * track calls), and the tracker calls stay refused while they are on.
 *
 * Configures the chain.  f = NULL, or all three members off, switches it off and frees it.  A successful call (re)starts every
 * stream's Kalman state from the reference's initial state; it drains outstanding work.  Everything the chain needs -- state,
 * a filtered set for each of the four slots, the ordering events -- is made here, never inside a step: an out-of-memory is
 * OATGPU_E_NOMEM from this call and leaves a working context.  OATGPU_E_INVALID, with nothing changed, when results are
 * outstanding, a frame set is partly staged, a limit is exceeded, a name is too long or a Kalman parameter is out of range.
 * Allowed with either tracker on or off, in either order. */
int oatgpu_set_tracker_filters(oatgpu_ctx *ctx, const oatgpu_marker_filters *f);
/* The filtered records of the frame sets the LATEST call of the six above delivered: one set for a batch call, n_frames sets
 * for a sequence call; out[t * n_streams + s].  Returns the number of sets written; OATGPU_E_INVALID when no chain is
 * configured, no tracker call has run since it was configured, or max_sets is too small.  Nothing is consumed: the call may
 * be repeated.  The chain advances for every frame whether or not this is called. */
int oatgpu_tracker_filtered(oatgpu_ctx *ctx, oatgpu_filtered *out, int32_t max_sets);

/* ---- multi-target detection: the K largest blobs of every camera, ranked ----
 * Every detector publishes one object a camera: the largest contour inside the area window.  With targets on, every call that
 * delivers a foreground result -- oatgpu_track_batch[_dev], oatgpu_track_enqueue* / _collect, oatgpu_track_stage /
 * _enqueue_staged, the three oatgpu_track_sequence_dev calls, oatgpu_detect_hsv / _thresh / _diff, and the batch and sequence
 * calls of the motion and the subtraction tracker -- also ranks the K best candidates of every camera and frame.
 *
 * For one camera and one frame, on the mask after erode / dilate and the one-pixel frame zeroing:
 *   candidates  its external contours with m00 > 0 and min_area <= m00 < max_area -- the contours the ordinary selection
 *               considers; a blob inside another blob's hole is not one;
 *   ranking     area descending; among equal areas the LATER first pixel in raster order comes first (the rule by which the
 *               ordinary selection picks its winner);
 *   rank 0      is therefore bit for bit the ordinary result (before oatgpu_set_kalman / oatgpu_set_homography);
 *   rank j      is invalid (valid = 0, first_pixel = -1) when fewer than j + 1 candidates exist;
 *   n_found     is the number of candidates and may exceed K.
 * Ranks carry no identity from frame to frame.  Targets are raw detections: oatgpu_set_kalman, oatgpu_set_homography and both
 * filter chains keep acting on the ordinary result only.  The ordinary results, the taps, the models and every state are bit
 * for bit what they are with targets off.
 *
 * Cost: a step with targets on takes the global blob kernels -- not the single-workgroup LDS kernel -- with one small ranking
 * kernel (k_blob_rank) behind them, and the fused tracker launches it in the plain order: no early dispatch, no paired back
 * half (oatgpu_last_step_shape reports early_blob 0).  With targets off every call does exactly what it did before.
 *
 * oatgpu_set_targets(k): 0 switches targets off (the default), 1..OATGPU_MAX_TARGETS on.  Drains outstanding work.  Everything
 * is allocated here, never in a step -- a target set for every ring slot and the synchronous detectors' extra slot, and for the
 * four slots of each batched tracker that is on (one switched on later allocates its own): an out-of-memory is OATGPU_E_NOMEM
 * from this call and leaves a working context.  OATGPU_E_INVALID, with nothing changed, when k is out of range, results are
 * outstanding or a frame set is partly staged, oatgpu_set_deferred is on, or marker sets are configured;
 * oatgpu_set_markers(n > 0) and oatgpu_set_deferred(1) are refused while targets are on.  oatgpu_set_targets itself is refused
 * while tracks (oatgpu_set_tracks) or target shapes (oatgpu_set_target_shapes) are on: switch them off first. */
#define OATGPU_MAX_TARGETS 8
int oatgpu_set_targets(oatgpu_ctx *ctx, int32_t k);          /* 0: off (default) */
/* The target sets of the frame sets the LATEST result-delivering call handed out: one set for a batch call, a collect or a
 * single-stage detector, n_frames sets for a sequence call.  out[(t * n_streams + s) * K + j] is rank j of camera s of set t,
 * n_found[t * n_streams + s] its candidate count.  A single-stage detector analyses one stream: the other streams of its set
 * come back invalid with n_found 0.  Returns the number of sets written; nothing is consumed.  OATGPU_E_INVALID when targets
 * are off, no such call has run since oatgpu_set_targets, or max_sets is too small. */
int oatgpu_targets(oatgpu_ctx *ctx, oatgpu_position *out, int32_t *n_found, int32_t max_sets);

/* ---- target tracks: identity across frames for the K ranked blobs ----
 * Rank is not identity: two animals of similar size swap ranks from frame to frame.  With tracks on, every frame of the motion
 * and the subtraction tracker (oatgpu_diff_batch[_dev], oatgpu_diff_sequence_dev, oatgpu_bsub_track_batch[_dev],
 * oatgpu_bsub_track_sequence_dev) also assigns its ranked detections to K persistent track slots per camera, runs one Kalman
 * filter per slot and publishes each slot's filtered record with an identity: one launch a frame on the device
 * (k_target_tracks) behind the frame's ranking, in frame order; inside the sequence calls the launches of consecutive frames are
 * ordered by events on the host -- nothing waits on the device.  Batch calls, sequence calls, oatgpu_tracks_update and the two
 * trackers continue one another.  The reference has nothing like this (every posidet publishes one object): the semantics are
 * this project's own.
 *
 * Per camera stream the context owns K track slots (K = the K of oatgpu_set_targets).  Each slot holds
 *   - one Kalman filter: a KalmanState, started from the reference's initial state by oatgpu_set_tracks and never re-created
 *     afterwards;
 *   - id (int64, 0 = empty), age and missed.
 * Per camera there is next_id, starting at 1.  A reborn slot therefore carries the covariance filter_step leaves behind: that
 * is exactly what `posifilt kalman` does after its own timeout, and it is kept.
 *
 * Parameters: the chain parameters of oatgpu_marker_filters, with kalman required on and homography and regions optional;
 * gate, in pixels: gate >= 0, or +inf for no gate; NaN or a negative value is refused.
 *
 * One frame of one camera takes the frame's target set.  Rank j is valid for j < D, with centroid (cx_j, cy_j) exactly as
 * oatgpu_position.x / .y give it.  All arithmetic is fp64, one rounding per operation, no contraction.
 *   1. Live slots.  Slot i is live if its Kalman output of the previous frame had position_valid = 1 (found).
 *   2. Prediction.  The predicted position of slot i is px = x + dt * vx, py = y + dt * vy, from that previous Kalman output in
 *      pixels, before any homography.
 *   3. Cost.  c(i, j) = dx * dx + dy * dy with dx = cx_j - px_i, dy = cy_j - py_i.  A pair is admissible iff slot i is live,
 *      rank j is valid and c <= gate * gate.  A NaN cost is inadmissible.
 *   4. Assignment.  Greedy global nearest neighbour.  Repeat until no pair is left: among admissible pairs whose slot and rank
 *      are both unassigned, take the smallest c; break equal costs by the smaller slot index, then by the smaller rank; assign
 *      the pair.
 *   5. Births.  Valid ranks still unassigned take, in rank order, the slots that were NOT LIVE AT THE START OF THIS FRAME, in
 *      ascending slot index.  A slot taken this way gets id = next_id++ and age = 0.  A rank with no such slot left is dropped.
 *   6. One sample per slot.  Every slot takes exactly one sample this frame: assigned or born slots take
 *      filter_step(valid, cx, cy); every other slot takes an invalid sample.  The slot then runs homography -> region, as the
 *      trackers' chain does, with no heading.
 *   7. The slot's output: the nine-word filtered record, i.e. oatgpu_filtered, bit for bit what the chain gives for that sample
 *      stream; id, which is 0 if the slot is not live AFTER the step (the slot's id is then cleared); rank, the rank it took
 *      this frame, or -1; age, the number of frames since birth; missed, the number of consecutive frames without a
 *      measurement, 0 on a measured frame.  A slot that is not live reports id 0, rank -1, age 0, missed 0.
 * Ids are never reused until the next oatgpu_set_tracks.  The assignment is greedy on purpose: exactly specifiable, K <= 8.
 *
 * Tracks act on the raw ranked detections.  The ordinary result, oatgpu_targets, the trackers' own filter chain
 * (oatgpu_set_tracker_filters, a separate state), taps, models and tracker state stay bit for bit what they are without tracks.
 * oatgpu_diff_reset, oatgpu_bsub_reset, RAW8 and undistortion switches never touch track state.  The fused tracker's own calls
 * (oatgpu_track_*) and the single-stage detectors do NOT advance tracks: with tracks on they behave as with tracks off; their
 * users, and any outside detector, go through oatgpu_tracks_update.
 *
 * Left out: tracks advanced inside the fused tracker's own batch, ring and sequence calls; an optimal (Hungarian) assignment;
 * tracks on marker planes; merging and splitting of blobs; several GPUs. */
typedef struct oatgpu_track {
    oatgpu_filtered filtered;      /* the slot's record behind kalman -> homography -> region; no heading */
    int64_t id;                    /* 0: the slot is not live */
    int32_t rank;                  /* the rank the slot took this frame, -1: none */
    int32_t age;                   /* frames since birth */
    int32_t missed;                /* consecutive frames without a measurement */
    int32_t reserved_;
} oatgpu_track;                    /* 96 bytes */
/* f = NULL switches tracks off and frees everything.  Otherwise: requires targets on, checks its parameters as
 * oatgpu_set_tracker_filters does and drains outstanding work; (re)starts every slot and every camera's next_id.  Everything is
 * allocated here, never in a step -- state, a track set for the four slots of each batched tracker that is on (one switched on
 * later allocates its own), an extra set for oatgpu_tracks_update, one ordering event per slot: an out-of-memory is
 * OATGPU_E_NOMEM and leaves a working context.  OATGPU_E_INVALID, with nothing changed, when targets are off, f->kalman == 0,
 * the gate is NaN or negative, a limit is exceeded or results are outstanding.  While tracks are on, oatgpu_set_targets is
 * refused (switch tracks off first). */
int oatgpu_set_tracks(oatgpu_ctx *ctx, const oatgpu_marker_filters *f, double gate);
/* The track sets of the frame sets the LATEST delivering call handed out (the six tracker calls above: one set for a batch
 * call, n_frames for a sequence call; oatgpu_tracks_update: its one set), in the convention of oatgpu_targets:
 * out[(t * n_streams + s) * K + i] is slot i of camera s of set t.  Returns the number of sets written; nothing is consumed.
 * OATGPU_E_INVALID when tracks are off, no such call has run since oatgpu_set_tracks, or max_sets is too small. */
int oatgpu_tracks(oatgpu_ctx *ctx, oatgpu_track *out, int32_t max_sets);
/* One synchronous association step, on the device, for one frame set of n_streams x K positions: exactly what oatgpu_targets
 * returns for one set; valid, x and y are used.  Advances the same track state; out[s * K + i] receives slot i of camera s.
 * This is how the fused tracker, the single-stage detectors and any outside detector reach tracks.  Refused while results are
 * outstanding. */
int oatgpu_tracks_update(oatgpu_ctx *ctx, const oatgpu_position *targets, oatgpu_track *out);

/* ---- target shapes: second moments, extents and body axis of the K ranked blobs ----
 * A target is a centroid and an area.  With shapes on, every call that delivers target sets (the list at oatgpu_set_targets)
 * also delivers, for every rank, the blob's order-2 moments, its bounding box and its orientation axis: one more kernel
 * (k_blob_shape) behind the frame's ranking, launched only while shapes are on.  The reference keeps m00, m10 and m01 of a
 * contour only (siftContours); what follows is cv::moments' next three fields and cv::boundingRect of the same contour.
 *
 * For every valid rank j of a target set, over the directed edges (x0, y0) -> (x1, y1) of the blob's EXTERNAL contour -- exactly
 * the edges whose order-0 and order-1 sums are a00, a10 and a01: the unit steps between neighbouring border pixels, one per side
 * of a pixel that faces the outside background; an edge facing a hole is not one -- with d = x0 * y1 - x1 * y0, in int64:
 *   a20 += d * (x0 * (x0 + x1) + x1 * x1)
 *   a11 += d * (x0 * ((y0 + y1) + y0) + x1 * ((y0 + y1) + y1))
 *   a02 += d * (y0 * (y0 + y1) + y1 * y1)
 * This is contourMoments of OpenCV 3.1 (imgproc/moments.cpp) over the contour's CHAIN_APPROX_SIMPLE points (the sums over a
 * straight piece equal the sums over its unit steps), exact in integers; it equals the double sums there wherever those stay
 * below 2^53.
 * x_min, y_min, x_max, y_max are the extremes of the contour's pixels; cv::boundingRect is (x_min, y_min, x_max - x_min + 1,
 * y_max - y_min + 1).
 *
 * The derived fields are fp64, use + - * / and sqrt only, one rounding per operation, no contraction.  With sg the sign of a00:
 *   m00 = a00 * sg 0.5,  m10 = a10 * sg 0.16666666666666666666666666666667,  m01 likewise from a01 (as oatgpu_position forms them)
 *   m20 = a20 * sg 0.083333333333333333333333333333333
 *   m11 = a11 * sg 0.041666666666666666666666666666667
 *   m02 = a02 * sg 0.083333333333333333333333333333333        (multiplications by these constants, as the source has them)
 *   inv = 1.0 / m00,  cx = m10 * inv,  cy = m01 * inv
 *   mu20 = m20 - m10 * cx,  mu11 = m11 - m10 * cy,  mu02 = m02 - m01 * cy            (completeMomentState)
 *   a = mu20 * inv,  b = mu11 * inv,  c = mu02 * inv                                 (the covariance of the blob's area)
 *   h = (a - c) * 0.5,  r = sqrt(h * h + b * b)
 *   l1 = (a + c) * 0.5 + r,  l2 = (a + c) * 0.5 - r                                  (its eigenvalues)
 *   major = 2 * sqrt(max(l1, 0)),  minor = 2 * sqrt(max(l2, 0))                      (max(l, 0): l where l > 0, else +0)
 * The body axis, the eigenvector of l1:
 *   v = (h + r, b) if h >= 0, else (b, r - h);  n = sqrt(vx * vx + vy * vy);  axis_valid = n > 0
 *   axis = (vx / n, vy / n), both components negated if vx < 0, or if vx == 0 and vy < 0.
 * An axis has no front: the sign rule only makes it unique (axis_x >= 0), it says nothing about where the head is.  A blob
 * whose covariance is isotropic (a square, a disc) has no axis: axis_valid = 0 and axis = (0, 0).  An invalid rank is all zeros.
 *
 * Shapes are read-only passengers: the ordinary results, oatgpu_targets, oatgpu_tracks, both filter chains, taps, models and
 * every state are bit for bit what they are with shapes off; integer sums make two runs bit-alike.  oatgpu_tracks_update
 * delivers no shapes.  With tracks on, oatgpu_track.rank indexes the frame's shape set: shapes[(t * n_streams + s) * K +
 * track.rank] is the shape of the identified animal -- the way to an identity's body axis.
 *
 * Left out: a heading inside oatgpu_track with the sign taken from the velocity; shapes on marker planes; third-order and Hu
 * moments; several GPUs. */
typedef struct oatgpu_shape {
    int32_t valid;                 /* the rank's position_valid */
    int32_t axis_valid;
    int64_t a20, a11, a02;         /* the exact order-2 sums */
    int32_t x_min, y_min, x_max, y_max;
    double mu20, mu11, mu02;       /* central moments */
    double axis_x, axis_y;         /* unit vector along the body, axis_x >= 0 */
    double major, minor;           /* 2 * sqrt(eigenvalue): the semi-axes' doubles of the equivalent ellipse, in pixels */
} oatgpu_shape;                    /* 104 bytes */
/* on = 1: requires targets on; drains outstanding work; allocates everything here, never in a step -- a shape set and a device
 * accumulator for every slot that has a target set (the ring's slots and the synchronous detectors' extra one, the four slots of
 * each batched tracker that is on; one switched on later allocates its own): an out-of-memory is OATGPU_E_NOMEM and leaves a
 * working context.  A successful call starts the delivered lists over (oatgpu_targets included).  on = 0 frees everything.
 * OATGPU_E_INVALID, with nothing changed, while results are outstanding or a frame set is partly staged, or targets are off.
 * While shapes are on, oatgpu_set_targets is refused (switch shapes off first). */
int oatgpu_set_target_shapes(oatgpu_ctx *ctx, int32_t on);
/* The shape sets of the frame sets the LATEST result-delivering call handed out, in oatgpu_targets' convention:
 * out[(t * n_streams + s) * K + j] is rank j of camera s of set t (a single-stage detector: the other streams are invalid).
 * Returns the number of sets written; nothing is consumed.  OATGPU_E_INVALID when shapes are off, no such call has run since
 * oatgpu_set_target_shapes, or max_sets is too small. */
int oatgpu_target_shapes(oatgpu_ctx *ctx, oatgpu_shape *out, int32_t max_sets);

/* ---- target crops: a frame window around every ranked blob, upright or turned to the body axis ----
 * Targets, tracks and shapes deliver numbers.  With crops on, the batch and sequence calls of the motion and the subtraction
 * tracker (the six calls that advance tracks) also deliver an h x w window of the INPUT frame for every rank of every camera
 * and frame: one more kernel (k_target_crops) behind the frame's ranking (and k_blob_shape), launched only while crops are on.
 * A 64 x 64 window per animal can follow its result to the host at rates a whole frame cannot.  oatgpu_crop_windows_dev cuts
 * windows at caller-given centres and axes; it is how the fused tracker, the single-stage detectors and any outside detector
 * reach crops.  The reference has nothing like this: the semantics are this project's own.
 *
 * Window geometry.  A window is (valid, cx, cy, ax, ay, upright) over an H x W frame of C interleaved channels (C = 1 or 3, the
 * context's channels).  Output pixel (i, j) -- row i of h, column j of w -- uses u = (double)(j - w / 2) and
 * v = (double)(i - h / 2), with integer division.
 *   Upright:  X0 = (int)rint(cx) - w / 2,  Y0 = (int)rint(cy) - h / 2   (rint rounds half to even, as cvRound does)
 *             out(i, j) = frame(Y0 + i, X0 + j); every pixel outside the frame is 0.
 *   Axis:     all fp64, one rounding per operation, no contraction:
 *             X = (cx + u * ax) - v * ay,   Y = (cy + u * ay) + v * ax
 *             qx = (int)rint(X * 32.0),  sx = qx >> 5 (arithmetic shift),  fx = qx & 31;  qy, sy, fy likewise from Y
 *             out(i, j) = (sum S * p + 512) >> 10 over the four corners (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1)
 *             with the weights (32 - fx)(32 - fy), fx (32 - fy), (32 - fx) fy, fx fy -- `framefilt undistort`'s pixel rule
 *             (INTER_LINEAR in OpenCV's fixed point); corners outside the frame are 0 (BORDER_CONSTANT 0); each channel on its
 *             own.  A position that is not finite, or whose |rint(X * 32.0)| or |rint(Y * 32.0)| reaches 2^30, lies outside
 *             every frame: the pixel is 0.
 *   Invalid:  h * w * C zeros.  Every byte of every window is written by every launch: a stale crop never survives in a slot.
 * A window whose centre or axis is NaN or infinite, or whose |cx| or |cy| exceeds 1e6, is invalid (qx cannot overflow).
 *
 * In the trackers the window of rank j has valid = the rank's valid; (cx, cy) exactly what oatgpu_position.x / .y carry for the
 * rank; in axis mode (ax, ay) = oatgpu_shape.axis_x / .axis_y where the rank's shape has axis_valid = 1 -- the body axis lies
 * along the window's +x; axis_x >= 0, so a window is never turned by more than 90 degrees either way, and the axis still has no
 * front.  A rank without an axis (a square) takes the upright rule as it stands.  Crops are cut from the frame as the caller gave
 * it, before the ROI mask and before anything the front kernel does to it.  With tracks on, oatgpu_track.rank indexes the
 * frame's crop set exactly as it indexes the shape set: the way to one small video per identified animal.
 *
 * Crops are read-only passengers: the ordinary results, oatgpu_targets, oatgpu_target_shapes, oatgpu_tracks, both filter chains,
 * taps, models and every state are bit for bit what they are with crops off.  The fused tracker's own calls and the single-stage
 * detectors deliver no crops: with crops on they behave as with crops off, exactly as they do for tracks.
 *
 * Left out: crops inside the fused tracker's own batch, ring and sequence calls and in oat-track-hip (ring frames may be
 * overwritten after oatgpu_track_input_consumed); crops from RAW8 or undistorted front ends; crops on marker planes; a window
 * turned by the velocity's sign; several GPUs.  (Crops in device memory, and scaling: crop tensors, below.) */
#define OATGPU_CROP_OFF 0
#define OATGPU_CROP_UPRIGHT 1
#define OATGPU_CROP_AXIS 2
#define OATGPU_CROP_MAX_SIDE 256
#define OATGPU_CROP_MAX_WINDOWS 8      /* per_stream of oatgpu_crop_windows_dev */
/* mode OATGPU_CROP_OFF switches crops off (the default) and frees everything; h and w are not looked at.  Otherwise:
 * 1 <= h <= 256, 4 <= w <= 256, w % 4 == 0; requires targets on, OATGPU_CROP_AXIS requires target shapes on; drains outstanding
 * work; allocates everything here, never in a step -- a crop set beside every target set of each batched tracker that is on
 * (one switched on later allocates its own), in page-locked host-mapped memory: an out-of-memory is OATGPU_E_NOMEM and leaves a
 * working context.  A successful call starts the delivered lists over, as oatgpu_set_target_shapes does.  OATGPU_E_INVALID, with
 * nothing changed, when a parameter is out of range, results are outstanding or a frame set is partly staged, targets (or, for
 * OATGPU_CROP_AXIS, shapes) are off, or oatgpu_set_tracker_bayer or oatgpu_set_tracker_undistort is on.  While crops are on,
 * those two switches and oatgpu_set_targets are refused, and oatgpu_set_target_shapes(0) is refused in axis mode. */
int oatgpu_set_target_crops(oatgpu_ctx *ctx, int32_t mode, int32_t h, int32_t w);
/* The crop sets of the frame sets the LATEST delivering call handed out (one set for a batch call, n_frames for a sequence
 * call), in oatgpu_targets' convention: out[(((t * n_streams + s) * K + j) * h + i) * w * C + x * C + c] is channel c of pixel
 * (i, x) of rank j of camera s of set t.  Returns the number of sets written; nothing is consumed.  OATGPU_E_INVALID when crops
 * are off, no such call has run since oatgpu_set_target_crops (or the latest delivering call was not one of the six), or
 * max_sets is too small. */
int oatgpu_target_crops(oatgpu_ctx *ctx, uint8_t *out, int32_t max_sets);
typedef struct oatgpu_crop_window {
    int32_t valid;                 /* 0: the window is h * w * C zeros */
    int32_t upright;               /* != 0: the upright rule, (ax, ay) is not used (but must be finite) */
    double cx, cy;                 /* the centre, in frame pixels */
    double ax, ay;                 /* the direction of the window's +x; used as given, not normalised */
} oatgpu_crop_window;              /* 40 bytes */
/* One synchronous step: per_stream (1..OATGPU_CROP_MAX_WINDOWS) windows for each of the context's n_streams frames.  frames_dev:
 * n_streams * rows * cols * channels bytes in device memory, stream-major, any alignment; win[s * per_stream + q] and
 * out[((s * per_stream + q) * h + i) * w * C + ...] are on the host.  The size limits of oatgpu_set_target_crops; needs no
 * switch and touches nothing a switch owns (its buffers are made, and grown, by the call: OATGPU_E_NOMEM).  Refused while
 * results are outstanding. */
int oatgpu_crop_windows_dev(oatgpu_ctx *ctx, const void *frames_dev, const oatgpu_crop_window *win, int32_t per_stream,
                            int32_t h, int32_t w, uint8_t *out);

/* ---- crop tensors: target windows in device memory, zoomed and converted for a network ----
 * Target crops end in page-locked host memory.  A pose network or a closed-loop classifier runs on the GPU that cut them, and
 * wants them there, in its number format, at its scale.  With crop tensors on, the same six calls -- the batch and sequence calls
 * of the motion and the subtraction tracker -- also write, for every frame set, rank and camera, a window into DEVICE memory the
 * caller owns: one more kernel (k_crop_tensor) behind the frame's ranking (k_blob_shape, k_target_crops), launched only while the
 * switch is on; no byte crosses the host link.  oatgpu_crop_tensor_windows_dev is the explicit form.  The reference has nothing
 * like this: the semantics are this project's own.
 *
 * A crop tensor element is a window of "target crops" above, followed by a conversion.
 *
 * Window.  With zoom == 1.0 the window of rank j is exactly the window of target crops for the mode: OATGPU_CROP_UPRIGHT the copy
 * around the rounded centroid; OATGPU_CROP_AXIS the axis rule where the rank's shape has axis_valid, else the upright rule.  With
 * any other zoom it is ALWAYS the axis (gather) rule above, along (ax, ay) = (zoom * axis_x, zoom * axis_y) in axis mode where the
 * rank has an axis, and along (zoom, 0.0) otherwise -- each product one fp64 multiply; the direction is then used as given, not
 * normalised, exactly as oatgpu_crop_window's.  zoom is in source pixels per output pixel: zoom = 2 shows a 128 x 128 region of the
 * frame in a 64 x 64 window, zoom = 0.5 a 32 x 32 region.  This is point-sampled bilinear, not an area filter: every output pixel
 * is the fixed-point interpolation of the four frame pixels around ONE position, so a zoom above 1 skips pixels and aliases as any
 * point sampling does.  1/16 <= zoom <= 16, and zoom must be finite.  An invalid window and every pixel outside the frame give the
 * uint8 value 0 before the conversion, as in target crops.
 *
 * Conversion, by oatgpu_crop_tensor_fmt.dtype; p is the window's uint8 value, C the context's channels, in the frame's order (BGR;
 * GREY contexts have C = 1):
 *   OATGPU_TENSOR_U8:   p itself, interleaved [h][w][C]: at zoom == 1 byte for byte the layout and content of oatgpu_target_crops.
 *                       scale and bias are not used (but must be finite).
 *   OATGPU_TENSOR_F32:  planar [C][h][w]; the value is fl32(fl32((float)p * scale[c]) + bias[c]) -- two fp32 roundings, no fused
 *                       multiply-add.
 *   OATGPU_TENSOR_F16:  planar [C][h][w]; that fp32 value rounded to nearest even to IEEE half.
 * An invalid window therefore holds bias[c] (as fp32 or half), not 0.
 *
 * Crop tensors are read-only passengers: the ordinary results, oatgpu_targets, oatgpu_target_shapes, oatgpu_target_crops,
 * oatgpu_tracks, both filter chains, taps, models and every state are bit for bit what they are with the switch off.  The fused
 * tracker's own calls and the single-stage detectors deliver none: with the switch on they behave as with it off, as with crops.
 * The switch is independent of oatgpu_set_target_crops: either, both or neither may be on, and they may differ in size and mode; a
 * context with only tensors on has no host-mapped crop sets and pays for no store into them.
 *
 * Left out: tensors inside the fused tracker's own calls and in the host binaries; RAW8 or undistorted front ends; an
 * area-filtered downscale; RGB channel order; marker planes; several GPUs. */
#define OATGPU_TENSOR_U8 0
#define OATGPU_TENSOR_F16 1
#define OATGPU_TENSOR_F32 2
typedef struct oatgpu_crop_tensor_fmt {
    int32_t dtype;                 /* OATGPU_TENSOR_U8 | _F16 | _F32 */
    int32_t reserved;              /* 0 */
    float scale[3], bias[3];       /* per channel, in the frame's order; a GREY context uses [0] */
} oatgpu_crop_tensor_fmt;          /* 32 bytes */
/* mode OATGPU_CROP_OFF switches crop tensors off (the default); nothing else is looked at.  Otherwise h, w within the limits of
 * oatgpu_set_target_crops, zoom and fmt as above, and out_dev: CALLER-OWNED DEVICE memory of capacity_sets (>= 1) entries of
 * n_streams * K * C * h * w elements of the dtype, 16-byte aligned.  The library never allocates, frees or copies it; the caller
 * keeps it alive and unchanged in place until the switch is off.  Frame set t of a delivering call is written into entry t -- one
 * entry for a batch call, n_frames for a sequence call -- in oatgpu_targets' order: element
 * (((t * n_streams + s) * K + j) * C + c) * h * w + i * w + x for F16 / F32, ((((t * n_streams + s) * K + j) * h + i) * w + x) * C + c
 * for U8.  Every element of such an entry is written on every launch (a stale window never survives); entries past the delivered
 * count are not touched.  The entry is complete when the call returns.  A sequence call of more frames than capacity_sets is
 * refused with OATGPU_E_INVALID before anything is launched and with nothing changed.
 * Requires targets on, OATGPU_CROP_AXIS target shapes on; drains outstanding work; allocates nothing.  OATGPU_E_INVALID, with
 * nothing changed, when a parameter is out of range (mode, h, w; a dtype that is none of the three; reserved != 0; a zoom outside
 * 1/16 .. 16 or not finite; a scale or bias that is not finite; out_dev null or not 16-byte aligned; capacity_sets < 1), results
 * are outstanding or a frame set is partly staged, targets (or, for OATGPU_CROP_AXIS, shapes) are off, or
 * oatgpu_set_tracker_bayer or oatgpu_set_tracker_undistort is on.  While the switch is on, those two switches and
 * oatgpu_set_targets are refused, and oatgpu_set_target_shapes(0) is refused in axis mode. */
int oatgpu_set_target_crop_tensor(oatgpu_ctx *ctx, int32_t mode, int32_t h, int32_t w, double zoom,
                                  const oatgpu_crop_tensor_fmt *fmt, void *out_dev, int32_t capacity_sets);
/* The number of entries the LATEST delivering call wrote (1 for a batch call, n_frames for a sequence call).  OATGPU_E_INVALID when
 * crop tensors are off, or no such call has run since oatgpu_set_target_crop_tensor (or the latest delivering call was not one of
 * the six). */
int oatgpu_target_crop_tensor_sets(oatgpu_ctx *ctx);
/* The explicit form, one synchronous step like oatgpu_crop_windows_dev: per_stream (1..OATGPU_CROP_MAX_WINDOWS) windows for each
 * of the context's n_streams frames.  The table win[s * per_stream + q] is on the host; there is no zoom argument -- the caller
 * puts the zoom into (ax, ay) of a window that is not upright.  out_dev: n_streams * per_stream entries of C * h * w elements in
 * device memory, 16-byte aligned, complete when the call returns.  Needs no switch and touches nothing a switch owns (its table is
 * made by the first call: OATGPU_E_NOMEM).  It is how the fused tracker, the single-stage detectors and any outside detector
 * reach tensors.  Refused while results are outstanding. */
int oatgpu_crop_tensor_windows_dev(oatgpu_ctx *ctx, const void *frames_dev, const oatgpu_crop_window *win, int32_t per_stream,
                                   int32_t h, int32_t w, const oatgpu_crop_tensor_fmt *fmt, void *out_dev);

/* ---- target masks: each ranked blob's own pixels as a device tensor ----
 * A crop or a crop tensor shows an h x w window of the frame around every ranked blob.  With two animals near each other the window
 * of rank 0 also holds rank 1, a reflection, or a blob too small to be ranked.  With target masks on, the same six calls -- the batch
 * and sequence calls of the motion and the subtraction tracker -- also write, for every frame set, rank and camera, which elements
 * of that window are THIS blob, into DEVICE memory the caller owns: one more kernel (k_target_mask) behind the frame's ranking,
 * launched only while the switch is on; nothing is downloaded and nothing is labelled on the host.  The reference has nothing like
 * this: the semantics are this project's own.
 *
 * Window.  The window of (stream, rank) is exactly the window of "crop tensors" above for the same mode, h, w and zoom: valid,
 * upright, centre and direction as derived there (the rank's centroid; the body axis in OATGPU_CROP_AXIS where the shape has
 * axis_valid; any zoom but 1.0 makes it a gather along (zoom * axis_x, zoom * axis_y), or (zoom, 0.0) otherwise), with the same
 * check: a centre or a direction that is not finite, or a centre beyond +-1e6, is no window.
 *
 * Source pixel of element (i, j), 0 <= i < h, 0 <= j < w.  Upright (the copy): (rint(cx) - w/2 + j, rint(cy) - h/2 + i).
 * Otherwise (the gather): the crop's X = (cx + u * ax) - v * ay, Y = (cy + u * ay) + v * ax in fp64 with u = j - w/2, v = i - h/2,
 * then qx = rint(32 * X), qy = rint(32 * Y) under the same range check (|qx|, |qy| < 2^30, else outside every frame); the source
 * pixel is ((qx + 16) >> 5, (qy + 16) >> 5) with arithmetic shifts.  This is the nearest pixel to the position the crop's bilinear
 * gather samples (a tie goes up), so a mask and a crop tensor of the same setting are aligned.
 *
 * Value.  The element is ON when all three hold: the source pixel is inside the frame; its bit in the final mask is set -- the
 * mask findContours sees, after erode / dilate, with the one-pixel frame zeroed --; and it belongs to the 8-connected component
 * whose first pixel in raster order is this rank's first_pixel.  Otherwise it is OFF: background, another component, a blob inside
 * this blob's hole, the hole itself, a pixel outside the frame, an invalid rank or window.  ON / OFF are 255 / 0 for
 * OATGPU_TENSOR_U8 and 1.0 / 0.0 for OATGPU_TENSOR_F16 and OATGPU_TENSOR_F32.
 *
 * mode OATGPU_CROP_OFF switches target masks off (the default); nothing else is looked at.  Otherwise mode, h, w and zoom have the
 * meaning and the limits of oatgpu_set_target_crop_tensor, dtype is one of the three OATGPU_TENSOR_* values, and out_dev is
 * CALLER-OWNED DEVICE memory, 16-byte aligned, of capacity_sets (>= 1) entries of n_streams * K * h * w elements of the dtype, laid
 * out [sets][n][K][h][w]: element (((t * n_streams + s) * K + j) * h + i) * w + x.  There is no channel axis.  The library never
 * allocates, frees or copies it.  Frame set t of a delivering call goes into entry t, not into the tracker's slot; every element of
 * a delivered entry is written on every launch; entries past the delivered count are not touched; the entry is complete when the
 * call returns.  A sequence call of more frames than capacity_sets is refused with OATGPU_E_INVALID before anything is launched
 * and with nothing changed.  The fused tracker's own calls and the single-stage detectors deliver none and reset the count, as for
 * crop tensors.
 *
 * Target masks are read-only passengers and the switch allocates nothing: the ordinary results, oatgpu_targets,
 * oatgpu_target_shapes, oatgpu_target_crops, the crop tensor, oatgpu_tracks, both filter chains, the taps and every state are bit
 * for bit what they are with the switch off.  The switch is independent of oatgpu_set_target_crops and
 * oatgpu_set_target_crop_tensor.  The mask lives in the tracker's own pixel domain -- behind oatgpu_set_tracker_bayer the
 * demosaiced frame's, behind oatgpu_set_tracker_undistort the undistorted frame's --, so unlike those two it is NOT refused with
 * either front end, in either order of switching.
 *
 * OATGPU_E_INVALID, with nothing changed and a working context, when: targets are off; shapes are off for OATGPU_CROP_AXIS;
 * results are outstanding or a frame set is partly staged; mode, h, w or zoom is out of range as for crop tensors; the dtype is
 * none of the three; out_dev is null or not 16-byte aligned; capacity_sets < 1.  While the switch is on oatgpu_set_targets is
 * refused, and in axis mode oatgpu_set_target_shapes(0).
 *
 * Left out: an explicit-window form; masks in the fused tracker's own calls and in the host binaries; a plane of rank labels;
 * masked crops (tensor * mask is one line for the caller); marker planes; several GPUs. */
int oatgpu_set_target_mask_tensor(oatgpu_ctx *ctx, int32_t mode, int32_t h, int32_t w, double zoom, int32_t dtype, void *out_dev,
                                  int32_t capacity_sets);
/* The number of entries the LATEST delivering call wrote (1 for a batch call, n_frames for a sequence call).  OATGPU_E_INVALID when
 * target masks are off, or no such call has run since oatgpu_set_target_mask_tensor (or the latest delivering call was not one of
 * the six). */
int oatgpu_target_mask_tensor_sets(oatgpu_ctx *ctx);

/* Deferred completion of the stage-by-stage operators below (default off).  With on = 1 a frame filter (oatgpu_mog_filter,
 * _bsub_filter, _mask_filter, _thresh_filter, _undistort_filter, _bgr2hsv, _cvt_color) or a detector (oatgpu_detect_hsv / _thresh / _diff)
 * returns as soon as its INPUT frame has been read -- the point where the reference posts its SOURCE, right after its
 * memcpy (FrameFilter.cpp:73-80, PositionDetector.cpp:78-86) -- leaves its output argument untouched (it may be NULL for the
 * detectors) and keeps the result on the device; oatgpu_fetch_frame / oatgpu_fetch_position then deliver it: a component
 * posts its SOURCE, waits for its SINK and has the filtered frame copied STRAIGHT into the sink's (page-locked) shared-memory
 * frame, without the staging copy in between (host/component.hpp).  One result may be waiting at a time: the next
 * stage-by-stage call before the fetch fails with OATGPU_E_INVALID.  Results are those of the plain calls. */
int oatgpu_set_deferred(oatgpu_ctx *ctx, int32_t on);
int oatgpu_fetch_frame(oatgpu_ctx *ctx, uint8_t *frame_out);
int oatgpu_fetch_position(oatgpu_ctx *ctx, oatgpu_position *out);

/* ---- stage-by-stage operators (host buffers), one call == one reference call ---- */

/* cv::BackgroundSubtractorMOG2::apply(frame, mask, learning_rate)
 * (BackgroundSubtractorMOG.cpp:124).  fgmask_out: rows*cols, values {0,127,255}. */
int oatgpu_mog_apply(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *bgr_in,
                     uint8_t *fgmask_out, double learning_rate);

/* BackgroundSubtractorMOG::filter(cv::Mat&) CPU-branch semantics
 * (BackgroundSubtractorMOG.cpp:114-127): apply + frame.setTo(0, mask == 0).
 * bgr_out may equal bgr_in. */
int oatgpu_mog_filter(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *bgr_in,
                      uint8_t *bgr_out, double learning_rate);

/* ColorConvert::filter with COLOR_BGR2HSV (ColorConvert.cpp:101-107). */
int oatgpu_bgr2hsv(oatgpu_ctx *ctx, const uint8_t *bgr_in, uint8_t *hsv_out);

/* ColorConvert::filter for any pair of colours (ColorConvert.cpp:101-107): from_color / to_color are
 * oat::PixelColor values (BINARY 0, GREY 1, BGR 2, HSV 3; Color.h:29-34), the cvtColor code comes from
 * oat::color_conv_table (Color.h:45-51): BGR -> GREY|BINARY (COLOR_BGR2GRAY -- the bridge `posidet thresh`
 * and `posidet diff` need, SimpleThreshold.cpp:46, DifferenceDetector.cpp:44), GREY|BINARY -> BGR, BGR -> HSV,
 * HSV -> BGR.  in: rows*cols*(1|3) bytes, out: rows*cols*(1|3) bytes, must not overlap unless equal in size.
 * OATGPU_E_INVALID with the reference's texts for pairs with nothing to do (ColorConvert.cpp:79-85) or
 * not possible (Color.h:88-95). */
int oatgpu_cvt_color(oatgpu_ctx *ctx, int32_t from_color, int32_t to_color, const uint8_t *in, uint8_t *out);

/* HSVDetector::detectPosition (HSVDetector.cpp:142-173): hsv_in rows*cols*3. */
int oatgpu_detect_hsv(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *hsv_in,
                      oatgpu_position *out);

/* SimpleThreshold::detectPosition (SimpleThreshold.cpp:114-134): grey_in rows*cols;
 * uses h_lo/h_hi as -T [min,max]. */
int oatgpu_detect_thresh(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *grey_in,
                         oatgpu_position *out);

/* DifferenceDetector::detectPosition (DifferenceDetector.cpp:98-173): grey_in rows*cols.  Stateful
 * per camera stream (the previous frame); the first frame of a stream is analysed as is, like the
 * reference.  For blur <= 22 a box blur of a {0,255} image is non-zero exactly where the k x k
 * dilation is (away from the outermost ring, which findContours zeroes), so the blur runs as a
 * bit-mask dilation. */
int oatgpu_detect_diff(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *grey_in, oatgpu_position *out);

/* ---- motion tracker: framefilt col -C GREY -> posidet diff for EVERY stream of the context, one front launch a step ----
 *
 * Frames are cfg.channels wide: 3 = the chain `framefilt col -C GREY -> posidet diff` (DifferenceDetector.cpp:98-173 behind
 * ColorConvert), 1 = `posidet diff` alone.  Where a stream has a ROI (oatgpu_set_roi_mask) the frame is masked first
 * (`framefilt mask` in front of col).  Parameters are the config's diff_threshold, blur and min_area / max_area; erode never.
 * A stream's first frame is analysed as it is (pixel != 0, no blur), afterwards blur is a dilation -- oatgpu_detect_diff's rules,
 * and oatgpu_detect_diff's STATE: the last image and the first-frame flag of a stream are shared, a stream advanced by one form
 * continues in the other.
 *
 * oatgpu_set_diff_tracker(1) drains outstanding work and allocates everything a step needs (an out-of-memory is reported here,
 * as OATGPU_E_NOMEM, never in the middle of a step): the last-image planes if oatgpu_detect_diff has not made them (1 byte a
 * pixel and stream), four sets of threshold words and of the tracker's own MORPH / FINAL planes (3 bits a pixel and stream a
 * set: 1.5 bytes in all), four host-mapped result sets and eight events.  The rest of a back half's scratch is the context's own
 * sets 0..3, used only while nothing else of the context is in flight.  0 frees it all but the last images.
 *
 * Every diff call is synchronous: it returns with none of its work in flight and leaves the result ring, the pipelined path's
 * counters and what oatgpu_read_mask shows untouched.  OATGPU_E_INVALID, with a message naming the cause and before anything is
 * read or has moved: the tracker is off; results are outstanding (oatgpu_track_enqueue*) or a set is partly staged;
 * oatgpu_set_kalman, oatgpu_set_homography or oatgpu_set_track_undistort is on; a null argument; n != n_streams;
 * n_frames < 0.  n_frames == 0 succeeds and does nothing. */
int oatgpu_set_diff_tracker(oatgpu_ctx *ctx, int32_t on);
/* Forget the last image of one stream (-1: of every stream): its next frame is a first frame again.  Also for oatgpu_detect_diff. */
int oatgpu_diff_reset(oatgpu_ctx *ctx, int32_t stream_ix);
/* One step: frames_dev = n_streams*rows*cols*channels bytes, stream-major (as oatgpu_track_batch_dev); out[n_streams].
 * Frames and rows of any alignment are taken; 4-byte aligned frames of a width divisible by 4 take the 4-pixels-a-lane kernel. */
int oatgpu_diff_batch_dev(oatgpu_ctx *ctx, const void *frames_dev, oatgpu_position *out);
/* The same on host frames: frames_host[i] -> rows*cols*channels bytes of stream i. */
int oatgpu_diff_batch(oatgpu_ctx *ctx, const uint8_t *const *frames_host, int32_t n, oatgpu_position *out);
/* A recorded sequence in one call: frames_dev[t] = frame set t, out[n_frames][n_streams].  Up to four frames are in flight, two
 * consecutive frames share a front launch wherever every stream has a last image; results, masks and the last images are those
 * of n_frames calls of oatgpu_diff_batch_dev. */
int oatgpu_diff_sequence_dev(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames, oatgpu_position *out);
/* oatgpu_read_mask for the latest diff frame (of a sequence: its last): which = OATGPU_TAP_THRESHOLD (|g - last| > thr),
 * _MORPH (after the blur-as-dilation), _FINAL; out rows*cols bytes {0, 255}.  OATGPU_E_INVALID before the first diff step. */
int oatgpu_read_diff_mask(oatgpu_ctx *ctx, int32_t stream_ix, int32_t which, uint8_t *out);

/* ---- subtraction tracker: framefilt bsub -> col -C HSV -> posidet hsv for EVERY stream of the context, one front launch a step ----
 *
 * Frames are cfg.channels wide: 3 = the chain `framefilt bsub -> framefilt col -C HSV -> posidet hsv` (BackgroundSubtractor.cpp:
 * 79-100, ColorConvert.cpp, HSVDetector.cpp:142-173), 1 = `framefilt bsub -> posidet thresh` (SimpleThreshold.cpp:114-134).  Where
 * a stream has a ROI (oatgpu_set_roi_mask) the frame is masked first (`framefilt mask` in front of bsub, FrameMasker.cpp:71-75):
 * on a first frame the masked pixels of the background are 0.  alpha is bsub's adaptation coefficient (-a): 0 = the background
 * stays what the stream's first frame (or oatgpu_bsub_set_background) made it; > 0 = cv::accumulateWeighted in fp32 on every frame,
 * the first included.  The window is the config's h/s/v (GREY: h_lo / h_hi) on the DIFFERENCE image, then the config's erode,
 * dilate and min_area / max_area.
 *
 * The background is oatgpu_bsub_filter's STATE: the u8 image, the fp32 accumulator and the first-frame flag of a stream are
 * shared, a stream advanced by one form continues in the other, oatgpu_bsub_set_background serves both.
 *
 * oatgpu_set_bsub_tracker(1) drains outstanding work and allocates everything a step needs (an out-of-memory is reported here,
 * as OATGPU_E_NOMEM, never in the middle of a step): the background planes if oatgpu_bsub_filter has not made them (5 bytes a
 * pixel, channel and stream), four sets of threshold words and of the tracker's own TMP / MORPH / FINAL planes (4 bits a pixel and
 * stream a set), four host-mapped result sets and eight events.  The rest of a back half's scratch is the context's own sets 0..3,
 * used only while nothing else of the context is in flight.  0 frees it all but the background.
 *
 * Every call is synchronous: it returns with none of its work in flight and leaves the result ring, the pipelined path's
 * counters and what oatgpu_read_mask shows untouched.  OATGPU_E_INVALID, with a message naming the cause and before anything is
 * read or has moved: the tracker is off; results are outstanding (oatgpu_track_enqueue*) or a set is partly staged;
 * oatgpu_set_kalman, oatgpu_set_homography or oatgpu_set_track_undistort is on; alpha outside [0, 1]; alpha > 0 while a stream's
 * background came from a file (the message names the stream; BackgroundSubtractor.cpp:63-71 makes no accumulator for it); a null
 * argument; n != n_streams; n_frames < 0.  n_frames == 0 succeeds and does nothing. */
int oatgpu_set_bsub_tracker(oatgpu_ctx *ctx, int32_t on);
/* Forget the background of one stream (-1: of every stream): its next frame is a first frame again (setBackgroundImage,
 * BackgroundSubtractor.cpp:79-85).  Also for oatgpu_bsub_filter. */
int oatgpu_bsub_reset(oatgpu_ctx *ctx, int32_t stream_ix);
/* One step (BackgroundSubtractor.cpp:87-100 -> HSVDetector.cpp:142-173 / SimpleThreshold.cpp:114-134): frames_dev =
 * n_streams*rows*cols*channels bytes, stream-major (as oatgpu_track_batch_dev); out[n_streams].  Frames and rows of any alignment
 * are taken; 4-byte aligned frames of a width divisible by 4 take the 4-pixels-a-lane kernel. */
int oatgpu_bsub_track_batch_dev(oatgpu_ctx *ctx, const void *frames_dev, double alpha, oatgpu_position *out);
/* The same on host frames (BackgroundSubtractor.cpp:87-100 and the detectors as above): frames_host[i] -> rows*cols*channels bytes
 * of stream i. */
int oatgpu_bsub_track_batch(oatgpu_ctx *ctx, const uint8_t *const *frames_host, int32_t n, double alpha, oatgpu_position *out);
/* A recorded sequence in one call (n_frames runs of BackgroundSubtractor.cpp:87-100 and the detector): frames_dev[t] = frame set
 * t, out[n_frames][n_streams].  Up to four frames are in flight, two consecutive frames share a front launch wherever a next
 * frame exists; results, masks and the background are those of n_frames calls of oatgpu_bsub_track_batch_dev. */
int oatgpu_bsub_track_sequence_dev(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames, double alpha,
                                   oatgpu_position *out);
/* The background of one stream as it stands (background_img_ and its fp32 twin, BackgroundSubtractor.cpp:79-100): bg
 * rows*cols*channels bytes, acc as many floats; either may be NULL.  OATGPU_E_INVALID while the stream has no background, and for
 * acc when the background came from a file.  Synchronises.  Also for oatgpu_bsub_filter. */
int oatgpu_bsub_get_state(oatgpu_ctx *ctx, int32_t stream_ix, uint8_t *bg, float *acc);
/* oatgpu_read_mask for the latest subtraction-tracker frame (of a sequence: its last; HSVDetector.cpp:146-158's threshold_frame_):
 * which = OATGPU_TAP_THRESHOLD (the window on the difference), _MORPH (after erode / dilate), _FINAL; out rows*cols bytes {0, 255}.
 * OATGPU_E_INVALID before the first step. */
int oatgpu_read_bsub_mask(oatgpu_ctx *ctx, int32_t stream_ix, int32_t which, uint8_t *out);

/* ---- fused hot path: mog + setTo + BGR2HSV + inRange + erode + dilate + blob ---- */

/* One frame for EVERY stream of the context (the whole chain
 * FrameFilter::process -> ColorConvert -> PositionDetector::process,
 * FrameFilter.cpp:59-98, PositionDetector.cpp:58-99, minus the shm hand-offs).
 * frames_host[i] -> rows*cols*channels bytes of stream i.  out[n_streams].
 * With channels == 1 the chain is framefilt mog (GREY) -> posidet thresh.
 * OATGPU_E_INVALID -- before anything is read or has moved -- while results are outstanding (oatgpu_track_enqueue*) or a
 * frame set is partly staged (oatgpu_track_stage); the same holds for oatgpu_track_batch_dev. */
int oatgpu_track_batch(oatgpu_ctx *ctx, const uint8_t *const *frames_host, int32_t n,
                       double learning_rate, oatgpu_position *out);

/* Same with the frames already resident in device memory:
 * frames_dev = n_streams*rows*cols*channels bytes, stream-major. */
int oatgpu_track_batch_dev(oatgpu_ctx *ctx, const void *frames_dev, double learning_rate,
                           oatgpu_position *out);

/* Pipelined form: enqueue returns at once; collect returns results in enqueue
 * order (exactly one result set per enqueued frame set, SURVEY.md 8b token
 * discipline).  Up to ring_depth enqueues may be outstanding.  By default the per-pixel
 * kernel that reads frames_dev is queued on the context's stream inside this call; after
 * oatgpu_set_fusion(2) it may go out with the NEXT frame's instead, and frames_dev must stay
 * valid and untouched until the frame's result was collected or oatgpu_track_input_consumed
 * returned (see oatgpu_set_fusion). */
int oatgpu_track_enqueue_dev(oatgpu_ctx *ctx, const void *frames_dev, double learning_rate);
/* Pipelined form for frames in HOST memory (what a camera or a shared-memory SOURCE hands over):
 * the frames are copied to a per-slot device buffer on a copy stream of their own, so the copy of
 * frame t+1 overlaps the kernels of frame t.  With page-locked frames (oatgpu_host_alloc /
 * oatgpu_host_register) the copies are direct DMA; the caller must leave frames_host[i] untouched
 * until the matching oatgpu_track_collect returns. */
int oatgpu_track_enqueue(oatgpu_ctx *ctx, const uint8_t *const *frames_host, int32_t n, double learning_rate);
int oatgpu_track_collect(oatgpu_ctx *ctx, oatgpu_position *out);
/* oatgpu_track_enqueue camera by camera, for components whose cameras do not deliver at the same instant:
 * oatgpu_track_stage starts the H2D copy of ONE camera's frame of the NEXT frame set as soon as that camera has
 * one (PositionDetector.cpp:63-75 waits for its one source; an N-camera component need not hold the link idle
 * until the slowest of N has delivered); once every stream 0..n_streams-1 has been staged,
 * oatgpu_track_enqueue_staged registers the set exactly as oatgpu_track_enqueue would have.  While a set is being
 * staged oatgpu_track_input_consumed_stream(i) waits for stream i's own copy (any staged stream, any order).
 * OATGPU_E_RING_FULL from the first oatgpu_track_stage of a set when ring_depth sets are outstanding.
 * OATGPU_E_INVALID, the open set staying as it is: a stream index outside 0..n_streams-1; a stream staged twice;
 * oatgpu_track_enqueue_staged before every stream is staged (also with none); oatgpu_track_enqueue / _enqueue_dev and the
 * synchronous track calls while a set is open (it owns the next ring slot: finish it or give it up with
 * oatgpu_track_stage_abort); oatgpu_track_input_consumed_stream(i) for a stream the open set has not staged yet.
 * oatgpu_track_collect, oatgpu_track_ready, the settings and the single-stage calls stay allowed while a set is open. */
int oatgpu_track_stage(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *frame_host);
int oatgpu_track_enqueue_staged(oatgpu_ctx *ctx, double learning_rate);
/* How oatgpu_track_stage moves a camera's frame: 0 (default) a DMA copy (hipMemcpyAsync); 1 a small copy KERNEL that reads
 * the frame in place over PCIe -- for frames in page-locked, mapped host memory (oatgpu_host_register'ed shared-memory
 * segments, oatgpu_host_alloc) that are 16-byte aligned; anything else takes the DMA path.  A launch costs the host a
 * quarter of a DMA copy's set-up, which is what an N-camera round is short of. */
int oatgpu_set_stage_copy(oatgpu_ctx *ctx, int32_t mode);
/* Gives up a partly staged frame set: a camera ended in the middle of a round (its SINK went END, lib/shmemdf/Source.h:187-215)
 * or a call failed after the first oatgpu_track_stage.  Waits for the copies already started (their SOURCEs may be posted
 * afterwards), registers nothing, owes no result; the next oatgpu_track_stage starts a new set.  No-op without one. */
int oatgpu_track_stage_abort(oatgpu_ctx *ctx);

/* oatgpu_track_input_consumed blocks until every frame handed over so far has been read out of the caller's
 * buffers -- host frames (oatgpu_track_enqueue): their H2D copies are done; device frames
 * (oatgpu_track_enqueue_dev): the per-pixel kernel that reads them has finished (a frame that was only
 * registered, oatgpu_set_fusion(2), is launched first; with oatgpu_set_track_undistort(1) the same point: the remap that
 * reads the caller's frame runs before that kernel on the same stream, so "consumed" is never earlier than without it).  From then on the caller may release or overwrite
 * them, i.e. post() the shared-memory SOURCEs while the device is still computing (the reference releases
 * its source right after its memcpy, FrameFilter.cpp:73-80 / PositionDetector.cpp:78-86).
 * oatgpu_track_ready: 1 if oatgpu_track_collect would return without blocking, 0 if the oldest outstanding
 * result is still being computed (or nothing is outstanding), < 0 on error.  (If that oldest frame is still only
 * registered -- oatgpu_set_fusion -- the call launches it; if its speculative back half declined the frame, the
 * call launches the global kernels on it and reports 0 until they are done.) */
int oatgpu_track_input_consumed(oatgpu_ctx *ctx);
/* The same for ONE camera stream of the latest oatgpu_track_enqueue: returns when frames_host[stream_ix] has been
 * read (its H2D copy is done), so an N-camera component posts every SOURCE as its own frame leaves shared memory
 * instead of after all N copies -- the frames travel one after the other over one PCIe link, and the upstream
 * writers of the first cameras refill their segments while the later copies are still running (PositionDetector.cpp:78-86
 * releases its one source right after its one memcpy; this is that rule per camera).  Call it for the streams in
 * ascending order.  Per-stream events are recorded from the first call on (that first call waits for the whole
 * set); for device frames it is oatgpu_track_input_consumed. */
int oatgpu_track_input_consumed_stream(oatgpu_ctx *ctx, int32_t stream_ix);
int oatgpu_track_ready(oatgpu_ctx *ctx);

/* A whole recorded sequence through the pipelined path in one call (what `oat frameserve file`
 * feeding the chain amounts to, without a host round trip per frame): frames_dev[t] = frame set t
 * in device memory (n_streams*rows*cols*channels bytes, stream-major), out[t*n_streams + s] = the
 * result of stream s for frame t.  Equivalent to the enqueue/collect loop with the ring kept full;
 * nothing may be outstanding when it is called. */
int oatgpu_track_sequence_dev(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames,
                              double learning_rate, oatgpu_position *out);
/* The same, also reporting WHEN each frame's result was collected: done_s[t] = seconds since the call was
 * entered (steady clock) at which frame t's result set had been handed out.  With the ring kept full the
 * difference done_s[t+K] - done_s[t] is the steady-state time of K steps, free of the pipeline's fill and drain
 * (bench.py's block timing).  done_s may be NULL. */
int oatgpu_track_sequence_dev_timed(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames,
                                    double learning_rate, oatgpu_position *out, double *done_s);
/* ... and WHEN each frame was handed to oatgpu_track_enqueue_dev inside the call: enq_s[t], same clock; done_s[t] -
 * enq_s[t] is the time a frame spends in the pipeline with the ring kept full (bench.py latency_us).  Either may be NULL. */
int oatgpu_track_sequence_dev_latency(oatgpu_ctx *ctx, const void *const *frames_dev, int32_t n_frames,
                                      double learning_rate, oatgpu_position *out, double *done_s, double *enq_s);
int oatgpu_track_outstanding(const oatgpu_ctx *ctx);

/* ---- parity taps / model checkpoint (not in the reference; for tests and resume) ---- */

enum {
    OATGPU_TAP_THRESHOLD = 0,  /* inRange output (after the fused kernel)        */
    OATGPU_TAP_MORPH = 1,      /* after erode/dilate == reference threshold_frame_ */
    OATGPU_TAP_FINAL = 2       /* after the 1-px frame zeroing findContours does */
};
/* Unpacks the device bit mask of the last processed frame of a stream to
 * rows*cols bytes {0,255}. */
int oatgpu_read_mask(oatgpu_ctx *ctx, int32_t stream_ix, int32_t which, uint8_t *out);

/* MOG2 model of one stream in the oracle's (OpenCV's) logical layout:
 * modes_used[rows*cols], weight/variance[rows*cols*nmix], mean[rows*cols*nmix*channels].
 * Entries of unused modes (>= modes_used) are unspecified on get.
 * set_state / load take ANY model.  One that is not what a run of this library leaves -- a weight that is neither 0 nor in
 * [2^-62, 4], a mean that is not finite, at least 2^20 in size or -0.f, a variance outside [var_min, var_max] -- is advanced
 * by the kernel instantiations that keep the compiler's IEEE division and compute every update (exact for any input,
 * several times slower) until the stream is re-initialised or a plain model is imported; every other model by the product
 * instantiations. */
int oatgpu_mog_get_state(oatgpu_ctx *ctx, int32_t stream_ix, uint8_t *modes_used, float *weight,
                         float *variance, float *mean, int32_t *nframes);
int oatgpu_mog_set_state(oatgpu_ctx *ctx, int32_t stream_ix, const uint8_t *modes_used,
                         const float *weight, const float *variance, const float *mean,
                         int32_t nframes);

/* MOG2 model checkpoint of one stream (the reference has none: a restarted `framefilt mog`
 * relearns its background for ~history frames).  save writes PATH atomically (PATH.tmp + rename);
 * load refuses a file whose geometry, channel count or mixture count differ from the context's.
 * Resuming from a checkpoint continues bit-identically to an uninterrupted run. */
int oatgpu_mog_save(oatgpu_ctx *ctx, int32_t stream_ix, const char *path);
int oatgpu_mog_load(oatgpu_ctx *ctx, int32_t stream_ix, const char *path);

/* ---- measurement ---- */
/* on = 0: off; on = 1: time every step; on = N > 1: time every Nth step (each timed step costs
 * five hipEventRecord calls, ~20 us of host time -- sample when the host is the bottleneck). */
int oatgpu_profile_enable(oatgpu_ctx *ctx, int32_t on);
int oatgpu_profile_read(oatgpu_ctx *ctx, oatgpu_profile *out);   /* synchronises */
int oatgpu_profile_reset(oatgpu_ctx *ctx);

/* Traffic audit of the fused per-pixel kernel (measurement; bench.py's `useful_bytes_per_px`).  While on,
 * the kernel runs in an instantiation that also counts, for every load and store it executes, the bytes its
 * lanes ask for and the 32-byte sectors / 64-byte half lines those requests touch.  Results are unchanged
 * (same predicates, same arithmetic); the audited launches are slower and must not be timed. */
typedef struct oatgpu_traffic {
    int64_t launches;                 /* audited kernel launches                          */
    int64_t pixels;                   /* pixels processed by them                         */
    int64_t lane_bytes_read;          /* bytes requested by the lanes: what the arithmetic */
    int64_t lane_bytes_written;       /*   can depend on / has changed ("useful" bytes)    */
    int64_t sector32_bytes_read;      /* the same requests in whole 32-byte sectors        */
    int64_t sector32_bytes_written;
    int64_t sector64_bytes_read;      /* ... and in whole 64-byte half lines               */
    int64_t sector64_bytes_written;
} oatgpu_traffic;
int oatgpu_traffic_audit(oatgpu_ctx *ctx, int32_t on);             /* on != 0: zero the counters and start */
int oatgpu_traffic_read(oatgpu_ctx *ctx, oatgpu_traffic *out);     /* synchronises */

/* Achievable HBM rates of THIS device, measured with plain streaming kernels (16 B/lane, `bytes`
 * per buffer, best of `reps`): *read_gbps for a read-only sum, *copy_gbps for read+write of a copy
 * (bytes moved = 2*bytes).  The spec peak (8 TB/s on MI355X) is never reached by any kernel; these
 * are the ceilings the hot path is compared against besides the spec. */
int oatgpu_measure_hbm(oatgpu_ctx *ctx, size_t bytes, int32_t reps, double *read_gbps, double *copy_gbps);

#ifdef __cplusplus
}
#endif
#endif /* OATGPU_H */
