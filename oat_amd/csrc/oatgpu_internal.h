// oatgpu_internal.h -- device-side layout contract shared by the kernel TUs and
// the C-ABI TU.  Not installed; the public surface is include/oatgpu.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace oatgpu {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// Geometry.  Every per-pixel device array of one camera stream lives in a
// PADDED index space: row pitch Wp = 64*ceil(W/64) pixels, so a 64-bit mask
// word never straddles two image rows.  p = y*Wp + x.  (For 640/1920/3840
// wide frames Wp == W and p is the plain raster index.)
// Arrays are allocated for Palloc = 1024*ceil(H*Wp/1024) entries so that the
// MOG kernel's 1024-pixel blocks need no tail handling on state planes.
// ---------------------------------------------------------------------------
struct Geom {
    int H, W, Wp;        // rows, cols, padded pitch
    int words;           // Wp / 64 mask words per row
    int P;               // H * Wp
    int Palloc;          // P rounded up to 1024
    int n_streams;
    unsigned words_magic; // ceil(2^32 / words): row of mask word i = (i * words_magic) >> 32, exact for every word of a frame
};

// MOG2 model in HBM (per stream): 25 fp32 planes + one u8 plane (mode counters), 101 B/px.
// One lane of K1 owns one pixel (p = y*Wp + x), a wavefront 64 consecutive pixels = one mask word:
// every plane access of a wave is one coalesced 256-byte line pair and __ballot(thr) IS the word.
// (Round 1 measured 2 and 4 pixels per lane with 8/16-byte accesses: 108/165 VGPRs, 4/3 waves per
// SIMD, slower; tools/k1_lab.hip shows the bare access pattern gains <= 3 % from wider accesses.)
//
// The counter byte of a pixel:  bits 0-2  modesUsed (what the reference keeps, 0..5)
//                               bits 3-6  LIVE hints: bit 2+k set <=> slot k (k = 1..4) holds a
//                                         weight that is not exactly 0
// The hints are this kernel's own bookkeeping (exported state has bits 0-2 only).  With the
// reference's `nmodes = nNewModes;` a pruned mode keeps its slot for ever with weight 0, so after a
// while most pixels count 5 modes of which 1-2 are alive; a slot whose weight is 0 can only matter
// to a pixel that has not matched an earlier mode (it may be re-matched and revived).  K1 therefore
// loads, of slots >= 1, the weights of LIVE slots only, and variance/mean only for pixels that did
// not match mode 0 as background ("needy" lanes) -- see k_mog_fused.
constexpr int kMogPlanes = 25;
constexpr int kMaxMix = 5;
constexpr int kWavePx = 64;               // pixels one wavefront owns
constexpr int kCountMask = 7;
constexpr int kLiveShift = 2;             // live bit of slot k is bit kLiveShift + k (k >= 1)

// Where the model lives.  Per mode k: a WEIGHT plane (fp32[Palloc]) and a plane of {variance, mean[channels]}
// RECORDS (fp32[Palloc][1 + channels]: 16 bytes per pixel for BGR, 8 for GREY), mode after mode; the counter bytes
// in an array of their own.  Weights stand alone because they are what changes every frame on every live mode;
// variance and mean travel together (a mode's fit test, update and swap always touch all of them): one 16-byte
// access per lane -- 1 KiB per wave instruction for mode 0, which every pixel reads and rewrites every frame --
// and a lane that needs a later mode touches ONE half-sector of it instead of a sector in each of four planes.
// (Round 1 and the first half of round 2 kept 25 scalar planes; profiles/r02_k1_layout_ab.txt also has the
// measurements of 256-pixel tile records and of the nontemporal cache policy, both rejected.)
constexpr size_t kPlanePad = 0;     // floats between consecutive planes (DRAM channel alignment of the ten streams was an A/B knob: no gain)
__host__ __device__ inline size_t mog_stream_floats(int Palloc) { return (size_t)kMogPlanes * Palloc + 10 * kPlanePad; }
__host__ __device__ inline size_t mog_w_off(int Palloc, int ch, int k) { return (size_t)k * ((2 + ch) * (size_t)Palloc + 2 * kPlanePad); }
__host__ __device__ inline size_t mog_vm_off(int Palloc, int ch, int k) { return mog_w_off(Palloc, ch, k) + Palloc + kPlanePad; }

struct MogParams {
    float Tb, TB, Tg, varInit, varMin, varMax, tau;
    int nmix;
    int detectShadows;
    int shadowVal;
    int restoreCount;        // MOG2Invoker's `nmodes = nNewModes;` (oatgpu_config.mog_restore_nmodes)
};

// inRange bounds after cv::inRange's normalisation: lo > hi encodes "empty".
struct RangeParams {
    int lo[3], hi[3];
};

struct MogLaunch {
    const uint8_t *frames;   // [n][H*W*channels] packed BGR (3) or GREY (1)
    int channels;
    float *state;            // [n][mog_stream_floats(Palloc)]
    uint8_t *nmodes;         // planar layout only: [n][Palloc] counters (same lane-interleaved slots)
    u64 *thr_bits;           // [n][Palloc/64] or nullptr
    uint8_t *out_bgr;        // [n][H*W*3] masked frame or nullptr
    uint8_t *out_mask;       // [n][H*W] {0,127,255} or nullptr
    int out_base;            // out_bgr / out_mask are indexed by (stream - out_base)
    const u64 *roi_bits;     // [n][Palloc/64] region-of-interest bits (framefilt mask fused in) or nullptr
    float alphaT, alpha1, prune;
    int fresh;               // 1: model is (re)initialised this frame -> no modes
    // Temporal fusion (kernels_mog.hip "Two frames a launch"): frames2 != nullptr -> the launch advances every
    // stream by TWO frames -- `frames` then `frames2` -- on ONE pass over the model; thr_bits2 takes the second
    // frame's threshold words, the *2 rates are the second frame's.  Never with fresh or out_bgr / out_mask; with audit
    // for BGR only.
    const uint8_t *frames2;
    u64 *thr_bits2;
    float alphaT2, alpha12, prune2;
    int nt_loads;            // 1: slots 1..4 are LOADED with the streaming cache policy too (dense models; kernels_mog.hip)
    unsigned long long *audit;   // nullptr, or 8 device counters: the traffic-audit instantiation runs (oatgpu_traffic_audit)
    MogParams mp;
    RangeParams rp;
    int audit_frozen;            // (last: the product instantiations never read it, and their argument offsets stay as measured)
                                 // audited launches: 1 when the PRODUCT launcher would have picked a frozen-model instantiation
                                 // for this launch (launch_mog_fused: every rate 0, default-policy loads, not fresh) -- the audit
                                 // then counts a fitted record's store only where its bits changed, as that kernel stores
#ifdef OATGPU_RS_TIMING
    unsigned long long *rs_end;  // measurement builds: the launch's last workgroups stamp the wall clock here (tools/rowscan_probe.py)
#endif
};

// --- kernels_mog.hip ---
// stop: an event that becomes the launch's own completion (nullptr: none)
// wg: threads a workgroup, 256 or 64 (one wave a workgroup: kernels_mog.hip, k_mog_fused); wild_model: a stream of the launch
// holds an imported model that is not PLAIN -- weights the kernel's in-range division does not cover, means or variances on
// which a rate-0 update is not the identity; wild_sink: 8 device counters the
// launches that keep the compiler's division count into (the audit instantiations; never nullptr in a context's launches)
struct MogLaunchOpts {
    int wg = 256;
    bool wild_model = false;
    bool frozen_ok = true;       // varMin <= varInit <= varMax: the frozen-model instantiations may skip the identity update of a fit site
    unsigned long long *wild_sink = nullptr;
};
void launch_mog_fused(const Geom &g, const MogLaunch &a, int first_stream, int n_streams, hipStream_t st, hipEvent_t stop,
                      const MogLaunchOpts &o);
void launch_density_probe(const uint8_t *nmodes, size_t total, unsigned *out, hipStream_t st);   // out = {live modes, samples}
// model checkpoint: logical (OpenCV AoS) <-> device planes
// state / nmodes point at ONE stream's model
void launch_state_export(const Geom &g, float *state, uint8_t *nmodes, int nmix, int channels,
                         uint8_t *modes_used, float *weight, float *variance, float *mean, hipStream_t st);
void launch_state_import(const Geom &g, float *state, uint8_t *nmodes, int nmix, int channels,
                         const uint8_t *modes_used, const float *weight, const float *variance,
                         const float *mean, hipStream_t st);

// --- kernels_measure.hip ---
// plain streaming kernels for the achievable-bandwidth measurement (n16 = number of 16-byte elements)
void launch_stream_read(const void *src, size_t n16, unsigned *sink, hipStream_t st);
void launch_stream_copy(const void *src, void *dst, size_t n16, hipStream_t st);
void launch_nop(hipStream_t st);   // one empty wave: calibrates what an event pair adds around a launch

// --- kernels_stages.hip --- (one component on one frame a launch)
// workgroups of 256 threads for a grid-stride loop over n elements: one thread an element up to a cap
inline unsigned grid_stride_blocks(size_t n) { const size_t blocks = (n + 255) / 256; return blocks > 8192 ? 8192u : (unsigned)blocks; }
// bytes from device-visible (page-locked, mapped) host memory to device memory by a kernel; both 16-byte aligned
void launch_stage_copy(const void *src_dev_visible, void *dst, size_t bytes, hipStream_t st);
void launch_bgr2hsv(const uint8_t *bgr, uint8_t *hsv, size_t npx, hipStream_t st);
// code 0: BGR -> GREY, 1: GREY -> BGR, 2: HSV -> BGR (Color.h:45-51); in/out 4-byte aligned
void launch_cvt_color(int code, const uint8_t *in, uint8_t *out, size_t npx, hipStream_t st);
// 3-channel (HSV) or 1-channel (grey) inRange of ONE frame into a bit mask.
void launch_inrange_bits(const Geom &g, const uint8_t *frame, int channels, const RangeParams &rp,
                         u64 *bits, hipStream_t st);
// framefilt bsub (BackgroundSubtractor.cpp:87-100) on n = rows*cols*channels bytes of one stream
void launch_bsub(const uint8_t *in, uint8_t *out, uint8_t *bg, float *bg_f, size_t n, float a, float b, int first,
                 int learn, hipStream_t st);
// framefilt mask (FrameMasker.cpp:71-75) with ONE stream's ROI bit plane
void launch_apply_roi(const Geom &g, const uint8_t *in, uint8_t *out, int channels, const u64 *roi, hipStream_t st);
// framefilt thresh (Threshold.cpp:67-81): BGR->grey (channels 3) -> inRange -> setTo(0)
void launch_thresh_filter(const uint8_t *in, uint8_t *out, size_t npx, int channels, int lo, int hi, hipStream_t st);
// posidet diff front end of ONE frame: bits = |frame - last| > thr (or frame != 0 when !have_last); last = frame
void launch_absdiff_bits(const Geom &g, const uint8_t *frame, uint8_t *last, int thr, int have_last, u64 *bits,
                         hipStream_t st);
void launch_unpack_bits(const Geom &g, const u64 *bits, uint8_t *out, hipStream_t st);
// rows*cols bytes (nonzero = keep) -> bit mask of one stream
void launch_pack_bits(const Geom &g, const uint8_t *in, u64 *bits, hipStream_t st);

// --- kernels_diff.hip, kernels_bsubtrack.hip --- (the front ends of the two batched trackers)
// what both front launches take: the frames, where the threshold words go, and the frames' form
struct FrontLaunch {
    const uint8_t *frames;   // [n][H*W*channels] packed BGR (3) or GREY (1), stream-major
    const uint8_t *frames2;  // nullptr, or the NEXT frame of every stream: the launch advances two frames
    int channels;
    u64 *bits, *bits2;       // [n][Palloc/64] threshold words of the frame(s); every word is written
    const u64 *roi;          // [n][Palloc/64] region-of-interest bits (framefilt mask in front of everything else) or nullptr
    const int *bayer;        // HOST: nullptr, or [n] OATGPU_BAYER_* 1..4 (checked by the caller; channels == 3, H, W >= 3): frames / frames2
                             // are Bayer RAW8, [n][H*W], demosaiced in registers; the tracker's own images stay BGR
    const uint32_t *ud_map1; // nullptr, or the undistortion maps of the n streams (plane 0; stream s at + s * ud_stride entries,
    const uint16_t *ud_map2; //   ud_stride = undistort_map_stride(H, W)): frames / frames2 are remapped in registers, every stream
    size_t ud_stride;        //   with its own map, the tracker's own images are in undistorted coordinates; not together with bayer
};
// Run-time switches as template arguments: f(std::bool_constant<b>{}...) for the bools given, in their order.  The front
// launches pick their kernel instantiation with it.
template <class F> void lift_bools(F &&f) { f(); }
template <class F, class... Rest> void lift_bools(F &&f, bool b, Rest... rest)
{
    if (b) lift_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else lift_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// the motion tracker's front end: col GREY -> posidet diff's absdiff + threshold, DESIGN.md 9c
struct DiffLaunch : FrontLaunch {   // (frames2: every stream has a last image)
    uint8_t *last;           // [n][H*W] previous GREY frame of every stream, refreshed by the launch
    const char *have_last;   // HOST: [n] 0: the stream's first frame (bit = g != 0)
    int thr;
};
// 4 pixels a lane with dword accesses: W % 4 == 0 and frames / frames2 / last 4-byte aligned (with ud_map1: `last` alone, the
// frames are gathered with unaligned loads); otherwise one pixel a lane
bool diff_front_is_wide(const Geom &g, const DiffLaunch &a);
void launch_diff_front(const Geom &g, const DiffLaunch &a, int n_streams, hipStream_t st);

// the subtraction tracker's front end: bsub -> col HSV -> inRange, or bsub -> inRange for GREY, DESIGN.md 9d
struct BsubLaunch : FrontLaunch {
    uint8_t *bg;             // [n][H*W*channels] framefilt bsub's background of every stream
    float *acc;              // [n][H*W*channels] ... and its fp32 accumulator
    const char *have;        // HOST: [n] 0: the stream's first frame (acc = bg = the masked frame)
    RangeParams rp;          // the window on hsv(difference); GREY: lo[0] <= difference <= hi[0]
    bool learn;              // alpha > 0: cv::accumulateWeighted with a = (float)alpha, b = 1 - a
    float a, b;
};
// 4 pixels a lane: W % 4 == 0, frames / frames2 / bg 4-byte and acc 16-byte aligned (with ud_map1: bg and acc alone); otherwise
// one pixel a lane
bool bsubtrack_front_is_wide(const Geom &g, const BsubLaunch &a);
void launch_bsubtrack_front(const Geom &g, const BsubLaunch &a, int n_streams, hipStream_t st);

// --- kernels_undistort.hip --- (framefilt undistort, Undistorter.cpp:83-88)
// 0, or -1 with the reason in *why: 5 to 8 coefficients (the reference's check) and not 6 or 7 (OpenCV 3.1 asserts on those)
int undistort_check_coeffs(int n_dist, const char **why);
// cv::undistort's map of a rows x cols frame (stripes of initUndistortRectifyMap, CV_16SC2): map1 rows*cols*2, map2 rows*cols
void undistort_build_map(int rows, int cols, const double K[9], const double *dist, int n_dist, int16_t *map1, uint16_t *map2);
// device map planes of one stream are padded to a multiple of kMapAlign entries: map1 as one u32 (sx | sy << 16) a pixel
constexpr int kMapAlign = 64;
size_t undistort_map_stride(int H, int W);
// remap of n_streams consecutive frames (stream-major, H*W*channels bytes each) with map planes map1 / map2 + s * map_stride
void launch_undistort(const uint8_t *in, uint8_t *out, const uint32_t *map1, const uint16_t *map2, size_t map_stride, int H,
                      int W, int channels, int n_streams, hipStream_t st);
// the fused tracker's remap of a whole step: n_frames (1 or 2) sets of n_streams frames, set i from in[i] into out[i], stream s
// of every set with map planes map1 / map2 + s * map_stride -- one launch (grid z = frame)
void launch_undistort_frames(const uint8_t *const *in, uint8_t *const *out, int n_frames, const uint32_t *map1,
                             const uint16_t *map2, size_t map_stride, int H, int W, int channels, int n_streams, hipStream_t st);

// --- kernels_debayer.hip --- (Bayer RAW8 -> BGR)
// n_frames (1 or 2) sets of n_streams raw frames (stream-major, H*W bytes each), set i from in[i] into out[i] (H*W*3 bytes a
// stream), stream s with patterns[s] (OATGPU_BAYER_* 1..4, checked by the caller); H, W >= 3.  One launch per 64 streams.
bool debayer_is_wide(int W, const uint8_t *const *in, uint8_t *const *out, int n_frames);
void launch_debayer_frames(const uint8_t *const *in, uint8_t *const *out, int n_frames, const int *patterns, int H, int W,
                           int n_streams, hipStream_t st);

// --- the blob stage: kernels_rowscan.hip (morphology, row scan), kernels_bloblds.hip (k_blob_lds), kernels_blob.hip (the global
// kernels, the riders and the orchestration of all three) ---
struct BlobBuffers {
    u64 *thr;        // [2][n][Palloc/64] inRange output, double-buffered across frames
    u64 *tmp;        // [n][Palloc/64] morphology ping
    u64 *morph;      // [n][Palloc/64] after erode/dilate
    u64 *fin;        // [n][Palloc/64] after 1-px frame zeroing
    u64 *trans;      // [n][Palloc/64] run-start (transition) bits
    int *carry;      // [n][H*words]   start x of the run entering each word
    int *parent;     // [n][Palloc]    union-find over run heads (sparse)
    long long *acc;  // [n][Palloc][3] Green sums per root (sparse)
    unsigned *done;  // [n]            workgroup arrival counter of k_green_select
    int *roots;      // [n][Palloc/2]  foreground roots of the current frame
    unsigned *nroots;// [n]
    // the single-workgroup LDS path (k_blob_lds): written by k_rowscan
    unsigned short *wpre;  // [n][H*words] run starts of the row in the words before this one
    int *rowinfo;          // [n][H]       0: no foreground in the row; else its number of runs
    unsigned *lds_ok;      // [n]          1: k_blob_lds wrote this frame's result, k_merge / k_green_select stand down
    // the early blob workgroup (kernels_bloblds.hip "Early dispatch"): a one-lane kernel behind the row scan publishes the frame's
    // ticket, the k_blob_lds workgroup that was dispatched ahead of it waits for exactly that ticket
    unsigned *ready;       // [n]          ticket of the latest frame whose row scan is complete (k_publish_ticket)
    unsigned *nopark;      // [1], one per CONTEXT (every scratch set points at it): set by the first parked workgroup that gave up
                           //              waiting -- the parked workgroups already in flight behind it decline at once instead of
                           //              waiting their own 100 ms each (kPathNoPark)
};
struct ResultRec {   // device-side result, one per stream per step
    long long a00, a10, a01;
    int first_pixel;
    int valid;
    // written by k_kalman when the position filter is on
    int kal_valid;
    int path;            // who wrote the record: 1 = k_blob_lds, 0 = k_green_select (host: when to speculate, below);
                         // kPathTimeout beside valid == kNeedsGlobal: the parked k_blob_lds workgroup gave up waiting for its ticket
    double kx, ky, kvx, kvy;
};

// `posifilt kalman` state of one camera stream (KalmanFilter2D.h:53-82 + cv::KalmanFilter members)
struct KalmanState {
    double statePre[4], statePost[4], Ppre[16], Ppost[16];
    double meas[2];          // kf_meas_ (keeps the stale measurement across missed detections)
    double reported[4];      // kf_predicted_state_ before it starts sharing statePre's buffer
    int found, missing, aliased;
    unsigned ticket;         // index of the next frame allowed to update this filter
};
struct KalmanLaunch {
    KalmanState *state;      // [n_streams]
    double dt, sig_accel, sig_noise;
    int threshold;           // not_found_count_threshold_ = (int)(timeout / dt)
    unsigned ticket;         // this frame's index
};
#ifdef OATGPU_RS_TIMING
void oatgpu_debug_rs_set_k1_end(const unsigned long long *p);     // measurement builds (kernels_rowscan.hip)
#endif
void launch_kalman(const KalmanLaunch &k, ResultRec *results, int n_streams, hipStream_t st);
void launch_kalman_reset(KalmanState *state, int n_streams, unsigned ticket, hipStream_t st);

void launch_morph(const Geom &g, const u64 *src, u64 *dst, int k, bool is_erode, int first_stream,
                  int n_streams, hipStream_t st);
// src_bits: mask before morphology; ero_k > 1 / dil_k > 1 fuse the erosion / dilation into the row
// scan (the erosion through LDS: rowscan_lds_bytes() must stay under kRowscanLdsMax, otherwise the
// caller erodes with launch_morph first and passes ero_k = 0).
// results: device-visible (host-mapped) array indexed by stream.
constexpr size_t kRowscanLdsMax = 64 * 1024;
size_t rowscan_lds_bytes(const Geom &g, int dil_k);
// Rows a row-scan workgroup takes where a step is launched deep in the pipeline (kernels_rowscan.hip "Rows a workgroup"; the default
// height, kRsRows, stays with the kernel).  A step takes it only if rowscan_lds_bytes_rows(g, dil_k, kRsRowsDeep) <= kRowscanLdsMax.
constexpr int kRsRowsNarrow = 4, kRsRowsDeep = 16;
constexpr int kRsRowsDeepAlt = 32;      // (measurement builds: the other height of profiles/rowscan_deep_rows.txt)
size_t rowscan_lds_bytes_rows(const Geom &g, int dil_k, int rows);
// The row scan alone (the launchers below are made of it): src / b are nf (1 or 2) frames' source masks and scratch sets, one launch
// for both; clear: reset lds_ok too (nobody else will); tag: measurement builds' row-group stamp.
void launch_rowscan(const Geom &g, const u64 *const *src, int ero_k, int dil_k, const BlobBuffers *b, int nf, int first_stream,
                    int n_streams, int clear, hipStream_t st, unsigned tag = 0u, int rows = kRsRowsNarrow);
// The global kernels' grid (k_green_select, k_blob_shape; blobedges_inline.h: chunk_bits, border_chunk).
// kGreenChunks threads per mask word, each owning 64 / kGreenChunks of its bits: the per-bit loops are
// serial, and a word on a horizontal edge of a blob has up to 64 border pixels -- with one thread per word
// that thread alone ran 10+ us at 1080p while a frame without a blob took 5 (profiles/r02_backhalf_latency_*.md).
constexpr int kGreenChunks = 4;
constexpr int kGreenBlock = 1024;          // big workgroups: every workgroup costs one same-address arrival atomic (~12 ns each, serialised)
// mode: kBlobFull  = row scan + k_blob_lds + k_merge + k_green_select (the last two stand down when the LDS
//                     kernel took the frame);
//       kBlobSpec  = row scan + k_blob_lds only: a frame too busy for it comes back with valid == kNeedsGlobal and
//                     the caller runs kBlobGlobal on the same threshold bits before it hands the result out;
//       kBlobGlobal = row scan + k_merge + k_green_select.
enum { kBlobFull = 0, kBlobSpec = 1, kBlobGlobal = 2 };
constexpr int kNeedsGlobal = -2;
constexpr int kPathTimeout = 2;
constexpr int kPathNoPark = 3;     // beside valid == kNeedsGlobal: declined without waiting, an earlier workgroup of the context had timed out
void launch_blob(const Geom &g, const BlobBuffers &b, const u64 *src_bits, int ero_k, int dil_k, double min_area,
                 double max_area, ResultRec *results, int first_stream, int n_streams, hipStream_t st, int mode = kBlobFull);
// The same in two halves on two HIP streams (kernels_bloblds.hip "Early dispatch"): the row scan with a one-lane kernel behind
// it that publishes `ticket`, and everything behind the row scan, whose k_blob_lds workgroup may be dispatched long before
// the row scan has run and waits for `ticket` on the device.  ticket != 0.
void launch_rowscan_signal(const Geom &g, const BlobBuffers &b, const u64 *src_bits, int ero_k, int dil_k, int first_stream,
                           int n_streams, unsigned ticket, hipStream_t st, int rows = kRsRowsNarrow);
// both frames of a two-frame step: ONE row-scan launch and ONE k_blob_lds launch (speculative mode), lds-able geometries only
void launch_blob_pair(const Geom &g, const BlobBuffers *b, const u64 *const *src, int ero_k, int dil_k, double min_area,
                      double max_area, ResultRec *const *results, int n_streams, hipStream_t st, int rows = kRsRowsNarrow);
// the blob workgroups of the nf (1 or 2) frames of a step in ONE launch (speculative mode): arrays of nf scratch sets,
// result records and tickets
void launch_blob_tail2(const Geom &g, const BlobBuffers *b, double min_area, double max_area, ResultRec *const *results,
                       int n_streams, const unsigned *ticket, int nf, hipStream_t st_tail);

// The marker sets' table-driven back half (kernels_blob.hip, launch_blob_table): what plane s of the launch -- marker s / n of
// camera s % n -- takes from its marker, one entry a PLANE ([M][n], the layout of the planes themselves), in device memory
struct BlobTab {
    int ero, dil;                // erode size (1: none) and dilate size (0: none) in effect
    double min_area, max_area;
};
void launch_blob_table(const Geom &g, const BlobBuffers *b, const u64 *const *src, const BlobTab *tab, int max_dil,
                       ResultRec *const *results, int n_planes, int nf, hipStream_t st);
// its row scan: plane s of the launch with the erode / dilate sizes of tab[s], the LDS sized by max_dil
void launch_rowscan_table(const Geom &g, const u64 *const *src, const BlobTab *tab, int max_dil, const BlobBuffers *b, int nf,
                          int n_planes, hipStream_t st);
// k_blob_lds, one workgroup a stream and frame: grid (1, ny, nz), frame z (0 or 1) on scratch set bz into resultsz, waiting for
// ticketz if that is not 0; spec: a declined frame comes back marked kNeedsGlobal; tab != nullptr: the area window of plane s is
// tab[s]'s (the TAB form)
void launch_blob_lds(const Geom &g, int ny, int nz, const BlobBuffers &b0, const BlobBuffers &b1, double min_area, double max_area,
                     ResultRec *results0, ResultRec *results1, int first_stream, int spec, unsigned ticket0, unsigned ticket1,
                     const BlobTab *tab, hipStream_t st);

// Multi-target detection (oatgpu_set_targets; kernels_blob.hip, k_blob_rank): the k largest candidates of every
// stream, ranked, out of what a kBlobGlobal back half has left in its scratch set b -- launched on the same HIP stream directly
// behind launch_blob(..., kBlobGlobal) or k_green_select's other launchers, before the set's next row scan.  recs[n][k]
// (stream first_stream + i at recs + (first_stream + i) * k) and found[n] may be host-mapped memory: 64-bit stores.  1 <= k <= kMaxTargets.
constexpr int kMaxTargets = 8;
struct TargetRec {   // one ranked blob: ResultRec's first four fields
    long long a00, a10, a01;
    int first_pixel;
    int valid;
};
void launch_blob_rank(const Geom &g, const BlobBuffers &b, double min_area, double max_area, int k, TargetRec *recs,
                      long long *found, int first_stream, int n_streams, hipStream_t st);

// Target shapes (oatgpu_set_target_shapes; kernels_blob.hip, k_blob_shape): the order-2 Green sums and the extents of
// the k ranked blobs of every stream -- launched on the same HIP stream directly behind launch_blob_rank, on the same scratch set b
// and the target set recs it has just written.  out[n][k] may be host-mapped memory (64-bit stores).  accum[n][k][kShapeAccWords]
// and arrived[n] are device memory that is all zero before the first launch and left all zero by every launch; launches that may
// run at the same time (frames in flight on several HIP streams) take an accumulator and a counter each.
constexpr int kShapeAccWords = 5;       // a20, a11, a02, {INT_MAX - x_min, INT_MAX - y_min}, {x_max, y_max}
struct ShapeRec {    // one ranked blob's raw shape, six 64-bit words
    long long a20, a11, a02;
    int x_min, y_min, x_max, y_max;
    int valid, reserved_;
};
void launch_blob_shape(const Geom &g, const BlobBuffers &b, int k, const TargetRec *recs, u64 *accum, unsigned *arrived,
                       ShapeRec *out, int first_stream, int n_streams, hipStream_t st);

// --- kernels_crops.hip --- (target crops: a frame window around every ranked blob, oatgpu_set_target_crops)
constexpr int kCropMaxSide = 256;      // 1 <= h <= 256, 4 <= w <= 256, w % 4 == 0
constexpr int kCropMaxWindows = 8;     // windows a stream of oatgpu_crop_windows_dev
struct CropWin { int valid, upright; double cx, cy, ax, ay; };      // one explicit window, five 64-bit words: oatgpu_crop_window's layout
struct CropLaunch {
    const uint8_t *frames;   // [n_streams][H*W*channels] packed BGR (3) or GREY (1), stream-major; any alignment
    int channels;
    int h, w;                // the window
    int k;                   // windows a stream
    int axis;                // records: 1 turns the window of a rank that has a body axis (shp is not null)
    const TargetRec *recs;   // [n_streams][k] a target set (may be host-mapped memory) ...
    const ShapeRec *shp;     // ... with the shape set beside it, or nullptr
    const CropWin *win;      // recs == nullptr: [n_streams][k] explicit windows (may be host-mapped memory)
    uint8_t *out;            // [n_streams][k][h][w][channels], 4-byte aligned (may be host-mapped memory: 32-bit stores)
};
// One launch for every window of every stream: workgroups over (row block, window, stream), a lane 4 output pixels of one row.
// A window's record is fetched once a workgroup; every byte of every window is written, zeros where the window is invalid.
void launch_target_crops(const Geom &g, const CropLaunch &a, int n_streams, hipStream_t st);

// --- kernels_croptensor.hip --- (crop tensors: those windows, zoomed and converted, in the caller's device memory;
// oatgpu_set_target_crop_tensor, oatgpu_crop_tensor_windows_dev)
// what the crop kernel (crops_inline.h) writes: k_target_crops' bytes, or a tensor's elements by oatgpu_crop_tensor_fmt's dtype
constexpr int kCropOutBytes = -1, kCropOutU8 = 0, kCropOutF16 = 1, kCropOutF32 = 2;
struct CropTensorLaunch : CropLaunch {   // out: [n_streams][k] windows of h * w * channels elements in DEVICE memory, 16-byte aligned
    double zoom;             // records: source pixels an output pixel; 1.0: the window of target crops as it stands
    float scale[3], bias[3]; // kCropOutF16 / kCropOutF32: per channel, in the frame's order
};
// The grid and the rules of launch_target_crops; every element of every window is written (an invalid window: bias[c], 0 for bytes).
void launch_crop_tensor(const Geom &g, const CropTensorLaunch &a, int dtype, int n_streams, hipStream_t st);

// --- kernels_targetmask.hip --- (target masks: each ranked blob's own pixels in the window of its crop tensor, in the caller's
// device memory; oatgpu_set_target_mask_tensor)
// The crop kernel's further outputs: kCropOutMask + a tensor dtype.  The window is the crop tensor's; instead of a frame pixel an
// element is ON where its source pixel is set in the final mask and belongs to the rank's 8-connected component.
constexpr int kCropOutMask = 8;
struct MaskTensorLaunch : CropTensorLaunch {   // frames, channels, win, scale and bias are not used; recs is never null
    Geom g;                  // the tracker's pixel domain: the window's source pixels are pixels of the final mask
    BlobBuffers b;           // the scratch set of the slot's global back half: fin, trans, carry, parent are read, nothing is written
};
// Behind launch_blob_rank (and launch_blob_shape for windows along the axis) on the HIP stream of a kBlobGlobal back half, before
// the set's next row scan; out: [n_streams][k][h][w] elements of the dtype (kCropOutU8: 255 / 0, the floats 1.0 / 0.0) in DEVICE
// memory, every element written.
void launch_target_mask(const MaskTensorLaunch &a, int dtype, int n_streams, hipStream_t st);

// --- kernels_markers.hip --- (marker sets: M colour windows per camera behind one MOG2 pass, `posicom mean`)
constexpr int kMaxMarkers = 8;
struct MarkerCombined {   // device-side record of k_marker_combine, one per stream per step: oatgpu_combined's layout
    int position_valid, heading_valid, velocity_valid, n_valid;
    double x, y, hx, hy;
};
// bit planes [M][n_streams][Palloc/64] of inRange_m(hsv(Z ? px : 0)) for every stream in one launch: frames = what the
// per-pixel kernel read (stream-major), zbits = the threshold plane it wrote under the non-zero window, win = [n_streams][M]
// windows in DEVICE memory
void launch_marker_bits(const Geom &g, const uint8_t *frames, int channels, const u64 *zbits, const RangeParams *win, int M,
                        u64 *planes, int n_streams, hipStream_t st);
// ... for the nf (1 or 2) frames of a step in one launch (grid z = frame): frame i reads frames[i] and zbits[i], writes planes[i]
void launch_marker_bits_frames(const Geom &g, const uint8_t *const *frames, int channels, const u64 *const *zbits,
                               const RangeParams *win, int M, u64 *const *planes, int n_streams, int nf, hipStream_t st);
// MeanPosition::combine over results[M][n_streams] (anchor -1: no heading) into out[n_streams]
void launch_marker_combine(const ResultRec *results, int M, int anchor, int n_streams, MarkerCombined *out, hipStream_t st);
// ... for the nf frames of a step in one launch; copy[i] (nullptr: none) also receives frame i's M x n_streams result records
// (out and copy may be host-mapped memory: 64-bit stores)
void launch_marker_combine_frames(const ResultRec *const *results, int M, int anchor, int n_streams, MarkerCombined *const *out,
                                  ResultRec *const *copy, int nf, hipStream_t st);

// The filter chain behind the combined record (oatgpu_set_marker_filters): kalman -> homography -> region, every member
// switched on its own.  MarkerFiltered is oatgpu_filtered's layout.
constexpr int kMaxRegions = 16, kMaxRegionPoints = 64;
struct MarkerFiltered {
    int position_valid, velocity_valid, heading_valid, region_valid;
    int region, reserved_;       // index of the first region hit, -1: none
    double x, y, vx, vy, hx, hy;
};
struct MarkerFilterParams {      // in DEVICE memory, read uniformly by every lane
    int kalman, threshold;       // threshold: not_found_count_threshold_ = (int)(timeout / dt)
    double dt, sig_accel, sig_noise;
    int homography, n_regions;
    double h[9];
    int region[kMaxRegions][2];  // first vertex and number of vertices of each region, in configured order
    int verts[kMaxRegions * kMaxRegionPoints][2];    // (x, y) after (cv::Point) of the configured point
};
// The chain (both launches: kernels_trackfilt.hip) on the nf (1 or 2) frames of a step, IN ORDER in one lane per stream: frame i reads in[i] (k_marker_combine's
// records, written by an earlier launch on the same HIP stream), writes out[i] (may be host-mapped memory: 64-bit stores) and
// advances state[s] (the ticket of KalmanState is not used: every launch of a context runs behind the one before)
void launch_marker_filters(const MarkerFilterParams *params, KalmanState *state, const MarkerCombined *const *in,
                           MarkerFiltered *const *out, int n_streams, int nf, hipStream_t st);
// The same chain behind the motion and the subtraction tracker (oatgpu_set_tracker_filters): ONE frame a
// launch, one lane per stream.  in[n_streams]: the tracker's result records of the frame's slot, written by the blob kernels
// earlier on the same HIP stream; out[n_streams] may be host-mapped memory (64-bit stores).  A detector has no heading.  The
// caller orders the launches of consecutive frames (events): nothing waits on the device.
void launch_tracker_filters(const MarkerFilterParams *params, KalmanState *state, const ResultRec *in, MarkerFiltered *out,
                            int n_streams, hipStream_t st);

// --- kernels_tracks.hip --- (target tracks: identity across frames for the k ranked blobs, oatgpu_set_tracks)
struct TrackRec {                // one slot's output, twelve 64-bit words: oatgpu_track's layout
    MarkerFiltered f;
    long long id;                // 0: the slot is not live
    int rank, age;               // rank taken this frame (-1: none), frames since birth
    int missed, reserved_;       // consecutive frames without a measurement
};
struct TrackMeta { long long id; int age, missed; };     // a slot's identity between launches, beside its KalmanState
struct TrackTriple { long long valid; double x, y; };    // one detection as oatgpu_tracks_update hands it over
struct TrackLaunch {
    const MarkerFilterParams *params;    // the chain's parameters (kalman on), in DEVICE memory
    KalmanState *state;                  // [n_streams][k] one filter a slot
    TrackMeta *meta;                     // [n_streams][k]
    long long *next_id;                  // [n_streams]
    double gate2;                        // gate * gate (+inf: no gate)
    int k;                               // slots a camera = ranks a camera, 1..kMaxTargets
};
// One association step for every camera stream: one wave a stream.  The frame's detections are recs[n_streams][k] (a target set,
// written by k_blob_rank earlier on the same HIP stream) or, where recs is null, tri[n_streams][k]; out[n_streams][k] may be
// host-mapped memory (64-bit stores).  The caller orders the launches of consecutive frames (events): nothing waits on the device.
void launch_target_tracks(const TrackLaunch &a, const TargetRec *recs, const TrackTriple *tri, TrackRec *out, int n_streams,
                          hipStream_t st);

}  // namespace oatgpu
