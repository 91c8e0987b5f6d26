// oatgpu_ctx.h -- the context of the C ABI (include/oatgpu.h) and what more than one of its units needs.  Not installed.
//
// No CPU fallback for any pixel work: every entry point either runs
// the HIP kernels or fails with an error code.
#pragma once
#include "../../include/oatgpu.h"
#include "oatgpu_internal.h"
#include "hip_owned.h"
#include "posfilt_inline.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <unistd.h>

using namespace oatgpu;

// Measurement switches (OATGPU_A_RESERVE / EARLY_BLOB / EARLY_MIN_PX / LONE_PLAIN / PAIR_BACK / K1_WG /
// K1_STOP_EVENT / RS_DEEP_ROWS, and OATGPU_K1_LDS in kernels_mog.hip) exist only in A/B builds made with -DOATGPU_MEASURE
// (`make variant`); each overrides one value of a path the product takes.  The product library never reads
// them, so nothing in the environment can change what it computes or skip work (tests/test_gpu_parity.py::
// test_measurement_env_is_inert_in_the_product_library).
static inline const char *measure_env(const char *name)
{
#ifdef OATGPU_MEASURE
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

struct ProfStep { Event e[5]; int frames = 1; };   // frames: what the K1 launch between e[0] and e[1] covered
struct Rate { float alphaT, alpha1, prune; int fresh; };   // A: K1 begin/end; B: back-half begin, after erode, end

__attribute__((visibility("hidden"))) void release_streams(int device);       // (api_context.hip)
// the context's share of its device's streams (-1: none); declared FIRST in the context, so given back LAST, after every buffer and event
struct StreamLease { int device = -1; ~StreamLease() { if (device >= 0) release_streams(device); } };

// One scratch set of the back half: owns the 14 arrays tmp .. ready of its BlobBuffers (thr and nopark are the context's, every
// set points at them).  Kernels take the plain BlobBuffers by value (b).
struct Scratch {
    BlobBuffers b{};
    Scratch() = default;
    Scratch(Scratch &&o) noexcept : b(std::exchange(o.b, BlobBuffers{})) {}
    Scratch &operator=(Scratch &&o) noexcept { if (this != &o) { reset(); b = std::exchange(o.b, BlobBuffers{}); } return *this; }
    ~Scratch() { reset(); }
    bool alloc(const oatgpu_ctx *c, size_t planes = 0);      // planes: how many (0: one a camera stream)
    void reset()
    {
        void *const own[] = {b.tmp, b.morph, b.fin, b.trans, b.carry, b.parent, b.acc, b.done, b.roots, b.nroots, b.wpre, b.rowinfo, b.lds_ok, b.ready};
        for (void *p : own) if (p) hipFree(p);
        b = BlobBuffers{};
    }
};

// marker sets (oatgpu_set_markers; kernels_markers.hip): M colour windows per camera behind the one model pass.  Everything
// below is made by oatgpu_set_markers and used by the synchronous marker step alone, on stream A.
struct MarkerSet {
    int n = 0;                                 // M; 0: markers off
    int anchor = -1;                           // `posicom mean --heading-anchor`, -1: none
    std::vector<oatgpu_marker> def;            // [M] erode / dilate / area of each marker (and its default window)
    std::vector<RangeParams> win_host;         // [n][M] normalised colour windows, per camera and marker
    DevMem<RangeParams> win;                   // ... on the device
    DevMem<u64> planes;                        // [M][n][Palloc/64] k_marker_bits' output = launch_blob's src_bits
    DevMem<u64> masks;                         // [M][3][n][Palloc/64] each marker's own tmp / morph / fin planes (the taps)
    Scratch bb;                                // the rest of one back-half scratch set, shared by the markers (they run one after the other)
    DevMem<ResultRec> res;                     // device: [M][n] result records, then [n] MarkerCombined
    HostMem<ResultRec> res_host;               // page-locked mirror: one copy back a step
    std::vector<const u64 *> tap_morph;        // [M] where marker m's mask after erode / dilate is
};
// the pipelined marker path (oatgpu_set_marker_pipeline): everything below is made by the switch, never inside a step.
// A step's marker work: k_marker_bits on stream A right behind its per-pixel kernel (launch_marker_work), the back half of
// all M x n planes and the combiner on B2 (a lone frame: on A), results into the slot's host-mapped record set.
struct MarkerPipeline {
    bool on = false;
    bool table = false;                        // the one-launch back half takes this geometry and these markers (else: marker by marker)
    int max_dil = 0;                           // largest dilation of the set: the row scan's LDS
    DevMem<u64> planes;                        // [ring][M][n][Palloc/64] k_marker_bits' output, per ring slot
    DevMem<u64> masks;                         // [ring][3][M][n][Palloc/64] the slot's tmp / morph / fin planes of every marker (the taps)
    Scratch bb[2];                             // the rest of a back-half scratch set for M x n planes, one for each frame of a step
    DevMem<BlobTab> tab;                       // [M][n] device table of the one-launch back half
    DevMem<ResultRec> res;                     // device: [2][M][n] the step's result records, read by k_marker_combine
    HostMem<ResultRec> rec;                    // host-mapped: [ring] sets of M x n ResultRec + n MarkerCombined, written by k_marker_combine through dev()
    std::vector<Event> ev;                     // [ring] the marker work whose last frame sits in this slot is done
    std::vector<int> ev_of;                    // [ring] slot -> the slot whose event covers its marker results
    std::vector<const u64 *> tap_morph;        // [ring][M] where the MORPH tap of marker m of that slot is
    Event bits_ev;                             // stream A: the step's k_marker_bits has finished
    int last_slot = -1;                        // ring slot of the frame set collected last on the pipelined path; -1: the synchronous step was later
    // a record set: M x n result records, n combined records, n filtered records (written only while a chain is configured)
    size_t set_bytes = 0;                      // = M n sizeof(ResultRec) + n (sizeof(MarkerCombined) + sizeof(MarkerFiltered))
};
// The list a delivering call keeps: the sets it handed out, for the reader that hands them out again (oatgpu_targets,
// oatgpu_tracks, oatgpu_*_filtered, ...).  ONE convention for every such list: the call starts it over where it begins to deliver
// (begin), every set it delivers joins it (keep: room for one more set of `per` items, filled by the caller), and delivered_to
// (below) is the reader, with its three refusals.  Every list has its own count.
template <class T> struct Delivered {
    std::vector<T> items;                      // [sets][per]
    size_t per = 0;                            // items a set, as the latest keep had it
    int sets = 0;
    void begin() { sets = 0; }
    T *keep(size_t per_)
    {
        per = per_;
        items.resize((size_t)(sets + 1) * per);
        return items.data() + (size_t)sets++ * per;
    }
    void keep(size_t per_, const void *set) { memcpy(keep(per_), set, per_ * sizeof(T)); }
};
// A filter chain kalman -> homography -> region (chain_step, posfilt_inline.h) as the host keeps it: what the marker chain and the
// trackers' chain have in common.  api_trackfilt.hip configures it (configure_chain) and hands out what a call delivered
// (chain_hand_out); the owners below add the buffers their kernels write.
struct PosfiltChain {
    bool on = false;
    DevMem<MarkerFilterParams> params;         // device: the chain's parameters and the region table
    DevMem<KalmanState> state;                 // device: [n] the chain's own filter state, one per camera stream (not c->kal's)
    Delivered<oatgpu_filtered> last;           // [sets][n] what the latest delivering call delivered (oatgpu_*_filtered)
};
// the filter chain behind the combined record (oatgpu_set_marker_filters): ONE launch behind k_marker_combine on the same HIP
// stream.  Made by the setter, dropped with the marker set.
struct MarkerFilters : PosfiltChain {
    DevMem<MarkerFiltered> out;                // device: [n] the synchronous step's filtered records
    HostMem<MarkerFiltered> out_host;          // ... their page-locked mirror
    bool append = false;                       // inside oatgpu_track_markers_sequence_dev: every collected set is kept
};

// The target family: what rides on the slot of a ranked result.  Target sets live in three homes -- the result ring
// and the slots of the two batched trackers (for_each_target_home) --, and every home owns, slot for slot, what the context's
// switches ask for: TargetSets::alloc makes all of it, for the setters (rebuild_target_sets, api_targets.hip) and for a batched
// tracker switched on later (BatchedTrackerState::alloc); nothing is made inside a step.
//
// Target shapes (oatgpu_set_target_shapes; api_targets.hip).  A shape set is what k_blob_shape writes for one frame
// set: [n][k] ShapeRec, host-mapped.  ShapeSets owns one for each slot of the TargetSets it stands beside, and the slot's device
// accumulator and arrival counter (frames in flight sit in different slots, so no two launches share them).  Empty while shapes are off.
struct ShapeSets {
    HostMem<ShapeRec> mem;                     // [slots][n][k]
    DevMem<u64> accum;                         // [slots][n][k][kShapeAccWords], all zero between launches
    DevMem<unsigned> arrived;                  // [slots][n], likewise
    size_t n = 0, k = 0;
    bool alloc(size_t slots, size_t n_streams, int k_);        // false: hipGetLastError() has the reason
    ShapeRec *rec_dev(int slot) const { return mem.dev() + (size_t)slot * n * k; }
    const ShapeRec *rec_host(int slot) const { return mem.host() + (size_t)slot * n * k; }
    u64 *accum_of(int slot) const { return accum + (size_t)slot * n * k * kShapeAccWords; }
    unsigned *arrived_of(int slot) const { return arrived + (size_t)slot * n; }
};
// Target crops (oatgpu_set_target_crops; api_crops.hip).  A crop set is what k_target_crops writes for one frame set:
// [n][k][h][w][channels] bytes, host-mapped.  CropSets owns one for each slot of the TargetSets it stands beside -- a batched
// tracker's: the fused tracker and the single-stage detectors deliver no crops, their target sets have none.  Empty while crops are off.
struct CropSets {
    HostMem<uint8_t> mem;                      // [slots][n][k][h][w][channels]
    size_t set_bytes = 0;
    bool alloc(size_t slots, size_t n_streams, int k, int h, int w, int channels);     // false: hipGetLastError() has the reason
    uint8_t *set_dev(int slot) const { return mem.dev() + (size_t)slot * set_bytes; }
    const uint8_t *set_host(int slot) const { return mem.host() + (size_t)slot * set_bytes; }
};
// the switches of the family that decide what stands beside a slot
struct TargetWants { int k; bool shapes; int crop_mode, crop_h, crop_w; bool tracks; };
// Multi-target detection (oatgpu_set_targets; api_targets.hip).  A target set is what k_blob_rank writes for one
// frame set: [n][k] TargetRec, then [n] candidate counts.  TargetSets owns one for each slot of one home, host-mapped, and the
// riders' sets beside them.
struct TargetSets {
    HostMem<char> mem;
    ShapeSets shp;                             // the shape sets beside the target sets, slot for slot, while shapes are on
    CropSets crp;                              // the crop sets beside them, while crops are on (a batched tracker's sets only)
    HostMem<TrackRec> trk;                     // [slots][n][k] the track sets beside them, while tracks are on (likewise)
    size_t n = 0, k = 0, set_bytes = 0;
    // everything `w` asks for (nothing with w.k == 0), zeroed; of_tracker: the slots of a batched tracker.  false: hipGetLastError() has the reason
    bool alloc(const TargetWants &w, size_t slots, size_t n_streams, int channels, bool of_tracker);
    TargetRec *rec_dev(int slot) const { return (TargetRec *)(mem.dev() + (size_t)slot * set_bytes); }
    long long *found_dev(int slot) const { return (long long *)(rec_dev(slot) + n * k); }
    const TargetRec *rec_host(int slot) const { return (const TargetRec *)(mem.host() + (size_t)slot * set_bytes); }
    const long long *found_host(int slot) const { return (const long long *)(rec_host(slot) + n * k); }
    TrackRec *trk_dev(int slot) const { return trk.dev() + (size_t)slot * n * k; }
    const TrackRec *trk_host(int slot) const { return trk.host() + (size_t)slot * n * k; }
};
// Crop tensors (oatgpu_set_target_crop_tensor; api_croptensor.hip): the switch's parameters and the CALLER's device
// memory -- never allocated, freed or copied here.  k_crop_tensor writes entry t of it for frame set t of a delivering call.
struct CropTensor {
    int mode = 0, h = 0, w = 0;                // OATGPU_CROP_*, the window
    double zoom = 1.0;
    oatgpu_crop_tensor_fmt fmt{};
    uint8_t *out = nullptr;                    // device: [capacity][n][k][...] elements of fmt.dtype
    int capacity = 0;
    size_t entry_bytes = 0;
    int last_sets = 0;                         // entries the latest delivering call wrote (oatgpu_target_crop_tensor_sets)
};
// Target masks (oatgpu_set_target_mask_tensor; api_targetmask.hip): the switch's parameters and the CALLER's device
// memory, as for crop tensors.  k_target_mask writes entry t of it for frame set t of a delivering call.
struct MaskTensor {
    int mode = 0, h = 0, w = 0;                // OATGPU_CROP_*, the window
    double zoom = 1.0;
    int dtype = 0;                             // OATGPU_TENSOR_*
    uint8_t *out = nullptr;                    // device: [capacity][n][k][h][w] elements of the dtype
    int capacity = 0;
    size_t entry_bytes = 0;
    int last_sets = 0;                         // entries the latest delivering call wrote (oatgpu_target_mask_tensor_sets)
};
struct Targets {
    int k = 0;                                 // K; 0: targets off
    TargetSets ring;                           // [ring_slots + 1] beside oatgpu_ctx::res: the ring's slots and the synchronous detectors' extra one
    bool append = false;                       // inside oatgpu_track_sequence_dev: every collected set is kept
    bool shapes = false;                       // oatgpu_set_target_shapes: every TargetSets of the context has its ShapeSets
    int crop_mode = 0, crop_h = 0, crop_w = 0; // oatgpu_set_target_crops: OATGPU_CROP_*, the window
    CropTensor ct;                             // oatgpu_set_target_crop_tensor; independent of crop_mode
    MaskTensor mt;                             // oatgpu_set_target_mask_tensor; independent of both
    // what the latest delivering call delivered (targets_begin starts all of them over, and ct.last_sets and mt.last_sets)
    Delivered<oatgpu_position> last;           // [sets][n][k] oatgpu_targets ...
    Delivered<int32_t> last_found;             // [sets][n] ... and its candidate counts
    Delivered<oatgpu_shape> last_shapes;       // [sets][n][k] while shapes are on (oatgpu_target_shapes)
    Delivered<uint8_t> last_crops;             // [sets][n][k][h][w][channels] while crops are on (oatgpu_target_crops); a call of the
                                               // fused tracker or a single-stage detector delivers none
    // the explicit window calls (oatgpu_crop_windows_dev, oatgpu_crop_tensor_windows_dev): made and grown by them; they outlive
    // both crop switches
    HostMem<CropWin> win;                      // host-mapped: [n][kCropMaxWindows] the table of windows of either call
    HostMem<uint8_t> cw_out;                   // host-mapped: [cw_bytes] the windows oatgpu_crop_windows_dev copies out
    size_t cw_bytes = 0;
};

// frames a batched tracker has in flight inside its sequence call (run_sequence_in_flight); each sits in a slot of its own
constexpr int kSeqSlots = 4;

// What a batched tracker keeps for every camera of the context.  Everything below is made by the tracker's switch (alloc), never
// inside a step.  A frame's back half runs in the context's scratch set `slot` (0..3) under open_sync's drain, the way detect_tail
// uses set 0 -- with the planes behind the taps replaced by the tracker's own, so that oatgpu_read_diff_mask / oatgpu_read_bsub_mask
// hold whatever the context's other calls do in between.
// (Not `BatchedTracker`: oat-track-hip has a class of that name, and the structs of this header are global -- the program's
// destructor would stand in for the library's: tests/test_abi_exports.py::test_no_cxx_symbol_is_shared_with_a_host_program.)
struct BatchedTrackerState {
    int planes;                                // mask planes a slot
    bool on = false;
    size_t n = 0, words = 0;                   // camera streams, and the words of one plane of all of them: n * Palloc / 64
    DevMem<u64> bits;                          // [kSeqSlots][n][Palloc/64] the front kernel's threshold words
    DevMem<u64> masks;                         // [kSeqSlots][planes][n][Palloc/64] the slot's planes (the taps)
    HostMem<ResultRec> rec;                    // host-mapped: [kSeqSlots][n] result records, written by the blob kernels through dev()
    TargetSets tgt;                            // [kSeqSlots] target sets beside rec and what rides on them, as the family's switches stand
    const uint8_t *frame[kSeqSlots] = {};      // the frame set the slot's front launch read, as the caller gave it (tracker_front) ...
    int entry[kSeqSlots] = {};                 // ... and its place in the call: 0 for a batch call, the frame's index in a sequence call
    Event ev_front[kSeqSlots];                 // stream A: the front launch that wrote this slot's bits has finished
    Event ev_done[kSeqSlots];                  // the slot's back half has finished
    int last = -1;                             // slot of the tracker's latest frame (oatgpu_read_*_mask); -1: none yet
    explicit BatchedTrackerState(int planes) : planes(planes) {}
    bool alloc(const oatgpu_ctx *c);           // all of the above, planes zeroed, `on` set; false: hipGetLastError() has the reason
    u64 *bits_of(int slot) const { return bits + (size_t)slot * words; }
    u64 *mask(int slot, int which) const { return masks + ((size_t)slot * planes + which) * words; }
    ResultRec *rec_dev(int slot) const { return rec.dev() + (size_t)slot * n; }
};
// the motion tracker (oatgpu_set_diff_tracker; kernels_diff.hip): `framefilt col -C GREY` -> `posidet diff`.
// Planes: morph, fin.
struct DiffTracker : BatchedTrackerState {
    DiffTracker() : BatchedTrackerState(2) {}
    std::vector<char> last_dilated;            // [n] of the latest frame: the stream's back half dilated (its MORPH tap is the morph plane)
};
// the subtraction tracker (oatgpu_set_bsub_tracker; kernels_bsubtrack.hip): `framefilt bsub` -> `col -C HSV` ->
// `posidet hsv` (GREY: bsub -> `posidet thresh`).  Planes: tmp, morph, fin.  The background itself -- bsub_bg, bsub_f, bsub_have --
// is the context's: oatgpu_bsub_filter's.
struct BsubTracker : BatchedTrackerState {
    BsubTracker() : BatchedTrackerState(3) {}
    const u64 *last_tap = nullptr;             // of the latest frame: where the mask after erode / dilate is (the MORPH tap)
};

// the filter chain behind the two batched trackers (oatgpu_set_tracker_filters; kernels_trackfilt.hip): kalman ->
// homography -> region on the result records of a slot, one launch a frame behind the slot's back half.  One chain and one filter
// state per camera stream for the context -- both trackers advance it; not c->kal's and not the marker chain's.  Everything below
// is made by the setter, never inside a step.
struct TrackerFilters : PosfiltChain {
    HostMem<MarkerFiltered> out;               // host-mapped: [kSeqSlots][n] the slot's filtered set, written by k_tracker_filters through dev()
    Event ev[kSeqSlots];                       // the slot's filter launch has finished: frame t's launch waits for frame t - 1's
};

// Target tracks (oatgpu_set_tracks; api_tracks.hip, kernels_tracks.hip): K persistent track slots per camera
// stream behind the ranked detections of the motion and the subtraction tracker, one k_target_tracks launch a frame behind the
// slot's k_blob_rank, in frame order.  One state for the context -- both trackers and oatgpu_tracks_update advance it.  Everything
// below is made by the setter, never inside a step; the trackers' track sets are TargetSets::trk.
struct Tracks {
    bool on = false;
    int k = 0;                                 // K of oatgpu_set_targets when tracks were switched on
    double gate2 = 0.0;                        // gate * gate
    DevMem<MarkerFilterParams> params;         // device: the chain's parameters and the region table
    DevMem<KalmanState> state;                 // device: [n][K] one filter a slot
    DevMem<TrackMeta> meta;                    // device: [n][K] id, age, missed of every slot
    DevMem<long long> next_id;                 // device: [n]
    HostMem<TrackTriple> upd_in;               // host-mapped: [n][K] the detections of oatgpu_tracks_update
    HostMem<TrackRec> upd_out;                 // host-mapped: [n][K] ... and its track set
    Event ev[kSeqSlots];                       // the slot's track launch has finished: frame t's launch waits for frame t - 1's
    Delivered<oatgpu_track> last;              // [sets][n][K] what the latest delivering call delivered (oatgpu_tracks)
    TrackLaunch launch() const { return {params, state, meta, next_id, gate2, k}; }
};

struct oatgpu_ctx {
    StreamLease lease;
    oatgpu_config cfg;
    Geom g;
    hipStream_t stream = nullptr;   // stream A: uploads + the fused per-pixel kernel
    static constexpr int kNB = 3;                // back-half streams B0..B2
    static constexpr int kSets = 5;              // scratch sets of the back half: up to four for frames in flight + one for repairs
    bool b_used[kNB] = {};          // B streams this context has launched on (the only ones it ever has to drain)
    hipStream_t stream_b[kNB] = {}; // streams B0..B2: morphology + blob analysis, on the plain path frame t on B[t % 3]
                                    // (B[t % 2] for host frames), overlapped with later frames' per-pixel kernels and each other
    Event ev_k1[kNB];            // the K1 whose back half runs on B[q] has finished (its threshold bits are ready)
    unsigned long long enq_total = 0, col_total = 0;  // pipelined frames enqueued / collected so far
    // cache policy of K1's slot-1..4 loads (kernels_mog.hip): streaming on dense models.  Two host-mapped
    // {live modes, samples} pairs filled alternately by k_density_probe; read one probe late, never waited for.
    HostMem<unsigned> dens;
    unsigned long long dens_probes = 0;
    bool nt_loads = false;
    // back half: frames go through row scan + k_blob_lds ONLY (kBlobSpec) while that keeps working; a frame too busy
    // for the LDS kernel comes back marked, oatgpu_track_collect then runs the global kernels on its threshold bits
    // (still in its ring slot) before handing the result out, and the full launch sequence is used until
    // kSpecAfter frames in a row were taken by the LDS kernel again.
    bool lds_spec = true;
    int lds_streak = 0;
    struct Slot {                   // per ring slot
        bool spec = false;          // launched speculatively (row scan + LDS kernel alone): redone in the repair set if declined
        bool filtered = false;      // was the position filter applied to this slot?
        bool repair = false;        // the global kernels are redoing this frame (ready/quiesce)
        int ev = 0;                 // the slot whose ring event covers this slot's result (itself, or the second frame of its
                                    // launch when both back halves share a B stream)
    };
    std::vector<Slot> slots;        // [ring_slots]
    int ring_slots = 0;                               // internal ring size (= ring_depth); one threshold-bit buffer per slot
    hipStream_t stream_c = nullptr;  // H2D copies of oatgpu_track_enqueue (created on first use)
    DevMem<uint8_t> frames_ring;     // [ring_slots][n_streams*rows*cols*channels] staging for host frames
    std::vector<Event> copy_ev;      // [ring_slots] frames of this slot have arrived
    std::vector<Event> copy_ev_s;        // [ring_slots][n_streams] ... and every single one of them (oatgpu_track_input_consumed_stream)
    hipStream_t stream_c2 = nullptr;     // second copy stream of the camera-by-camera path (shared per device)
    Event ev_c2;                         // ... and its "all my copies of this set are done"
    std::vector<char> staged;            // [n_streams] oatgpu_track_stage: frame of the NEXT set already on its way
    int staged_count = 0, stage_slot = -1;
    bool per_stream_copy_ev = false;     // recorded from the first per-stream call on
    bool last_copy_per_stream = false;   // the latest enqueue recorded them
    int last_copy_slot = -1;         // slot of the most recent oatgpu_track_enqueue (host frames)
    KalmanLaunch kal{};              // kal.state == nullptr: position filter off
    DevMem<KalmanState> kal_state;   // ... the owner of kal.state
    bool kal_on = false;
    unsigned kal_ticket = 0;         // ticket of the next enqueued frame
    // Early dispatch of the blob workgroup (kernels_bloblds.hip): the row scans of a device-frame step go down B0 / B1 by frame
    // parity, as on the plain path; the k_blob_lds workgroups of the step's frames are submitted with them as ONE launch on
    // B2 and wait on the device for their row scans' tickets.  Scratch sets 0 .. 3 by frame index mod 4; repairs of declined
    // frames use set 4 on B2.
    int early_blob = -1;             // -1: by shape -- at most THREE streams, 4 MP a step and more, where the per-pixel kernel then runs with one wave
                                     // a workgroup (k_mog_fused, WG): 4K 18.5 k -> 19.2 k fps, result 245 -> 250 us behind its frame
                                     // (profiles/r05g_wg64_early_blob_ab.txt).  With 256-thread workgroups the parked workgroup costs
                                     // the per-pixel kernel 4 % (one at 4K) to 20 % (32 of them, 16 x 1080p) and several streams gain
                                     // nothing either way (r05h): off there.  0 / 1: oatgpu_set_early_blob
    bool stage_kernel = false;       // oatgpu_set_stage_copy(1): oatgpu_track_stage copies with a kernel reading the host frame in place
    int k1_stop_event = -1;          // the step's "K1 done" event rides on the last K1 launch's own completion signal (no marker
                                     // packet behind it on stream A): -1 by step size (>= 4 MP: +1..2.5 % at 4K; small steps are
                                     // bound by the host's calls, and hipExtLaunchKernel costs more of those: one 1080p stream -3 %),
                                     // 0 / 1 forced (measurement builds: OATGPU_K1_STOP_EVENT)
    size_t early_min_px = 4000000;   // pixels a step from which the early order is considered (measurement builds: OATGPU_EARLY_MIN_PX)
    int k1_wg_force = 0;             // oatgpu_set_k1_workgroup (64 | 256): the per-pixel kernel's workgroup size whatever the path
    DevMem<unsigned> nopark;         // device word: a parked blob workgroup of this context has timed out (BlobBuffers::nopark)
    unsigned long long early_timeouts = 0;   // frames whose parked blob workgroup gave up waiting for its row scan (kWaitTicks):
                                     // something serialises kernel dispatches -- the context then stops parking (early_off)
    bool early_off = false;
    int last_k1_wg = 0;              // what the latest pipelined step used (oatgpu_last_step_shape)
    bool last_step_early = false;
    int rs_rows_force = 0;           // oatgpu_set_rowscan_rows: 0 by pipeline depth (plan_step), kRsRowsNarrow / kRsRowsDeep on every eligible step
    int rs_rows_deep = kRsRowsDeep;  // the wide height (measurement builds: OATGPU_RS_DEEP_ROWS = 16 | 32)
    int last_rs_rows = 0;            // rows a row-scan workgroup of the latest pipelined step (oatgpu_last_step_rowscan_rows)
    int last_early = -1;             // path of the previous step (-1: none yet; 0 plain, 1 early, 2 paired): a switch drains the B streams first
    int lone_plain = 1;              // a frame launched with NOTHING else outstanding (a camera-paced caller) takes the plain order even where the early
                                     // order is the default: no ticket kernel, no parked workgroup to release -- one frame at a time 133.5 -> 129.3 us at
                                     // 4K, 89.6 -> 85.9 us for two 1080p streams, frame rate unchanged (profiles/r07t_lone_frame_plain_order_ab.txt) --
                                     // and its back half goes to stream A itself (inline_back in launch_jobs: 4K 131 -> 122 us, one 1080p stream
                                     // 66 -> 58.5 us, profiles/r07in_lone_frame_inline_ab.txt; measurement builds: OATGPU_LONE_PLAIN=0)
    int pair_back = 1;               // two-frame steps outside the early order: ONE row-scan launch and ONE blob launch for both frames
                                     // (measurement builds: OATGPU_PAIR_BACK=0)
    unsigned pair_steps = 0;         // paired steps so far (their parity picks the B stream and the two scratch sets)
    unsigned bh_ticket[kSets] = {};
    unsigned early_frames = 0;       // frames that took the early path (their parity picks scratch set and row-scan stream)
    Event ev_blob[kSets];            // scratch set q: its latest reader is done
    bool ev_blob_valid[kSets] = {};
    int last_slot = 0;               // ring slot whose threshold bits the latest back half read (oatgpu_read_mask)
    std::string err;
    // Deferred completion of the single-stage calls (oatgpu_set_deferred): the call returns when its INPUT has been read
    // (the H2D copy is done), the result stays on the device until oatgpu_fetch_frame / oatgpu_fetch_position
    bool deferred = false;
    Event ev_h2d;
    int defer_kind = 0;              // 0 nothing waiting, 1 a frame (defer_dev, defer_bytes), 2 a position (defer_s)
    const uint8_t *defer_dev = nullptr;
    size_t defer_bytes = 0;
    int defer_s = 0;
    bool broken = false;             // a launch of the pipelined path failed half-way: the model and its rate schedule are ahead
                                     // of the results -- every later pipelined call is refused (oatgpu.h "Errors")
    // Temporal fusion (kernels_mog.hip "Two frames a launch"): with fuse == 2 a pipelined enqueue only REGISTERS its
    // frame (ring slot, counters); the kernels go out when the next frame is enqueued -- K1 once for both -- or when
    // somebody needs the frame's result or the model (collect / ready of that very frame, every synchronous entry
    // point, destroy), then for the one frame alone.  Results, their order and the model are those of one launch a frame.
    struct FrameJob { const void *frames = nullptr; double lr = 0.0; hipEvent_t ready = nullptr; int slot = 0; };
    // `posifilt homography` behind the detector / the position filter (oatgpu_set_homography): applied where the
    // centroid is finished, on the host, in the reference's double arithmetic
    bool homo_on = false;
    double homo[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int fuse = 0;                                     // 0: default -- pair where the library owns the frame's lifetime
                                                      // (host frames, track_sequence_dev), not for oatgpu_track_enqueue_dev
    bool in_sequence = false;                         // inside oatgpu_track_sequence_dev: its frames are all in hand
    Event ev_in;                                      // stream A has read every frame handed over so far (input_consumed)
    bool dev_unconsumed = false;                      // device frames were enqueued since the last input_consumed
    bool pend_valid = false;
    FrameJob pend;
    unsigned long long launched_total = 0;            // frames whose kernels are out (<= enq_total)

    // device memory
    DevMem<float> state;
    DevMem<uint8_t> nmodes;
    DevMem<uint8_t> frames;        // staging [n][H*W*3]
    DevMem<uint8_t> aux_a;         // [H*W*3]
    DevMem<uint8_t> aux_b;         // [H*W*3]
    DevMem<uint8_t> bsub_bg;       // [n][H*W*ch] framefilt bsub background (u8) and its fp32 accumulator
    DevMem<float> bsub_f;
    std::vector<char> bsub_have;
    DevMem<uint8_t> diff_last;     // [n][H*W] previous GREY frame of posidet diff, allocated on first use
    std::vector<char> diff_have;   // per camera stream
    DevMem<u64> roi;               // [n][Palloc/64] ROI bits, allocated on first oatgpu_set_roi_mask
    DevMem<uint32_t> ud_map1;      // [n][ud_stride] framefilt undistort maps (sx | sy << 16) and [n][ud_stride] fractions,
    DevMem<uint16_t> ud_map2;      //   allocated on first oatgpu_set_undistort (kernels_undistort.hip)
    size_t ud_stride = 0;
    std::vector<char> ud_have;     // per camera stream: has a map
    bool ud_track = false;         // oatgpu_set_track_undistort: the fused track calls remap every frame first (launch_front)
    DevMem<uint8_t> ud_frames[2];  // [2][n][H*W*ch] the remapped frames of a step (frame i of a two-frame step in buffer i): K1
                                   //   reads them in place of the caller's; allocated by oatgpu_set_track_undistort(1)
    bool by_track = false;         // oatgpu_set_track_bayer: the fused track calls take Bayer RAW8 frames and demosaic them first (launch_front)
    std::vector<int> by_pat;       // [n] OATGPU_BAYER_* of every camera stream while by_track
    DevMem<uint8_t> by_frames[2];  // [2][n][H*W*3] the demosaiced frames of a step (ud_frames' lifetime rule): the remap, or K1, reads
                                   //   them in place of the caller's; allocated by oatgpu_set_track_bayer
    bool tb_on = false;            // oatgpu_set_tracker_bayer: the motion and the subtraction tracker take Bayer RAW8 frames and demosaic
    std::vector<int> tb_pat;       //   them inside their front kernels; [n] OATGPU_BAYER_* of every camera stream while tb_on
    bool tu_on = false;            // oatgpu_set_tracker_undistort: the motion and the subtraction tracker remap every stream's frame with
                                   //   its map (ud_map1 / ud_map2, every ud_have set while on) inside their front kernels
    DevMem<u64> thr;               // [ring_slots][n][Palloc/64] the ring's threshold buffers (BlobBuffers::thr of every scratch set)
    Scratch bb[kSets];             // scratch sets, all made with the context
    const u64 *last_morph = nullptr;
    const u64 *last_fin = nullptr;
    HostMem<ResultRec> res;        // [ring_depth+1][n] pinned + mapped (last slot: single-stage calls); kernels store results straight to the host through dev()
    std::vector<Event> ring_ev;
    int ring_count = 0;

    std::vector<int> nframes;      // per camera stream
    std::vector<Rate> rates_scratch;

    // profiling
    bool prof = false;
    int prof_every = 1;            // sample every Nth step (event records cost ~4 us of host time each)
    unsigned long long prof_tick = 0;
    std::vector<ProfStep> prof_steps;
    size_t prof_used = 0;
    oatgpu_profile prof_sum{};
    int prof_drop_streak = 0;      // consecutive samples prof_fold took for host stalls
    double event_pair_ms = 0.0;

    // traffic audit (oatgpu_traffic_audit)
    DevMem<unsigned long long> audit_dev;      // 8 counters
#ifdef OATGPU_RS_TIMING
    unsigned long long *rs_k1_end = nullptr;   // (leaked at destroy: measurement builds only)
#endif
    DevMem<unsigned long long> wild_sink;      // 8 counters nobody reads: launches outside div_inrange's operands (kernels_mog.hip)
    std::vector<char> wild_model;              // [n_streams] 1: an imported model with weights no run of the kernel produces
    bool audit_on = false;
    long long audit_launches = 0;

    MarkerSet mk; MarkerPipeline mkp; MarkerFilters mf;      // the optional features: dropping one is assignment (c->mkp = {})
    DiffTracker df;
    BsubTracker bs;
    TrackerFilters tf;
    Targets tg;
    Tracks tk;
};

// a back half's erosion and dilation, planned and issued (plan_morph, issue_morph: api_track.hip)
struct MorphPlan {
    int ero, dil;               // erode / dilate sizes in effect (0: none)
    bool ero_apart;             // the erosion is a launch of its own, not fused into the row scan
};
struct MorphIssued { const u64 *src; int ero; const u64 *tap; };

// What a pipelined step does, decided before anything of it is launched (plan_step)
struct StepPlan : MorphPlan {  // (the context's erode / dilate: plan_morph)
    bool share_b, early, inline_back, paired, spec_plain;
    int k1_wg;                  // threads a K1 workgroup
    int rs_rows;                // rows a row-scan workgroup (kRsRowsNarrow, or the wide height on a step deep in the pipeline)
    hipEvent_t k1_done;         // the step's "K1 done" event (nullptr: inline_back, nobody waits for it)
};

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), OATGPU_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

// What the pipelined entry points refuse, always in this order; `checks` names the ones that apply to the caller.
enum : unsigned { kRefStaging = 1, kRefState = 2, kRefRingFull = 4 };
static constexpr int kRepairSet = oatgpu_ctx::kSets - 1, kRepairStream = oatgpu_ctx::kNB - 1;

// Helpers that cross unit boundaries, by the unit that defines them.  Hidden: none of them joins the library's dynamic symbols.
#pragma GCC visibility push(hidden)
// api_context.hip
extern thread_local std::string g_last_error;
int fail(oatgpu_ctx *c, int code, const char *fmt, ...);
hipError_t drain_b(oatgpu_ctx *c);
int check_detector(oatgpu_ctx *c, const oatgpu_marker &k, int blur = 0);
hipStream_t acquire_copy_stream(int device);
hipStream_t acquire_copy_stream2(int device);
hipError_t make_events(std::vector<Event> &table, size_t count, unsigned flags);
int quiesce(oatgpu_ctx *c);
int open_sync(oatgpu_ctx *c);
int check_stream_ix(oatgpu_ctx *c, int s);
// api_stages.hip
int read_plane(oatgpu_ctx *c, const u64 *plane, uint8_t *out);
int ensure_bsub(oatgpu_ctx *c, size_t nb);
// api_track.hip
Rate mog_begin(oatgpu_ctx *c, int s, double learningRate);
MogLaunch mog_launch_base(oatgpu_ctx *c, const uint8_t *frames, const Rate &r);
MogLaunchOpts mog_launch_opts(oatgpu_ctx *c, int s0, int s1, int wg);
void to_position(const ResultRec &r, oatgpu_position *o);
MorphPlan plan_morph(const Geom &g, int erode, int dilate);
MorphIssued issue_morph(const Geom &g, const MorphPlan &m, const BlobBuffers &bb, const u64 *thr, int s0, int n, hipStream_t st);
int back_half(oatgpu_ctx *c, BlobBuffers &bb, const u64 *thr, int s0, int n, int slot, hipStream_t st,
              hipEvent_t ev_mid, int erode_k = -1, int dilate_k = -1, int mode = kBlobFull);
int flush_pending(oatgpu_ctx *c);
int repair_outstanding(oatgpu_ctx *c);
int upload_frames(oatgpu_ctx *c, const uint8_t *const *frames_host, size_t frame_bytes);
// api_markers.hip
bool own_window_is_nonzero(const oatgpu_config &k);
int launch_marker_work(oatgpu_ctx *c, const oatgpu_ctx::FrameJob *j, int nj, const StepPlan &plan);
// api_trackfilt.hip: the chain as both of its owners use it (who: "marker" or "tracker", in the messages) -- the checked parameters
// for configure_chain below, and the list of the latest delivering call to the caller
int chain_params(oatgpu_ctx *c, const oatgpu_marker_filters *f, MarkerFilterParams &p);
int chain_hand_out(oatgpu_ctx *c, const PosfiltChain &ch, const char *who, const char *none_yet, oatgpu_filtered *out, int max_sets);
// ... what every reader of a Delivered list refuses (delivered_to, below): off and none_yet are the texts of the first two
int delivered_refusals(oatgpu_ctx *c, bool on, const char *off, const char *none_yet, int sets, int max_sets);
// ... and what the two batched trackers share; `name` is "diff" or "bsub", `what` the call's name in a refusal
int tracker_refusals(oatgpu_ctx *c, const BatchedTrackerState &bt, const char *name, const char *what);
int check_batch_dev(oatgpu_ctx *c, const void *frames_dev, const oatgpu_position *out);
int check_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int n, const oatgpu_position *out);
int check_sequence_dev(oatgpu_ctx *c, const void *const *frames_dev, int n_frames, const oatgpu_position *out);
int open_tap(oatgpu_ctx *c, const BatchedTrackerState &bt, const char *name, const char *none_yet, int s, int which, const uint8_t *out);
int reset_have(oatgpu_ctx *c, std::vector<char> &have, int s);
// A step of a batched tracker around its front and blob launches: tracker_begin where the call begins to deliver --
// every list a tracker's call delivers starts over --; tracker_tail behind the blob launch of the frame in `slot` on st: rank,
// shape, crops, crop tensor, target mask, tracks, filters (bb: the slot's scratch set, rd: its result records; prev_slot: the slot of the frame
// before inside a sequence call, whose track and filter launches this frame's wait for, -1: none); tracker_hand_out: the finished
// frame in `slot` to the caller, and every set of it into its list -- the only place a tracker's call keeps.
void tracker_begin(oatgpu_ctx *c);
int tracker_tail(oatgpu_ctx *c, const BatchedTrackerState &bt, const BlobBuffers &bb, const ResultRec *rd, int slot, int prev_slot, hipStream_t st);
void tracker_hand_out(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, oatgpu_position *out);
// api_targets.hip: k_blob_rank behind a kBlobGlobal back half of scratch set bb on st, for streams [s0, s0 + n), into `slot` of ts,
// and k_blob_shape behind it while shapes are on; the lists a delivering call keeps (targets_begin where it starts to deliver: the
// whole family's lists start over; targets_keep for every set, its shape set with it; only: the one stream a single-stage detector
// analysed, -1: all) -- all do nothing while targets are off.  rebuild_target_sets: every home's sets made anew for the switches
// `w`, built aside -- a failed allocation ("<what>: allocation failed") leaves the context as it was.
int targets_launch(oatgpu_ctx *c, const BlobBuffers &bb, const TargetSets &ts, int slot, int s0, int n, hipStream_t st);
void targets_begin(oatgpu_ctx *c);
void targets_keep(oatgpu_ctx *c, const TargetSets &ts, int slot, int only = -1);
int rebuild_target_sets(oatgpu_ctx *c, const TargetWants &w, const char *what);
// api_crops.hip: k_target_crops on the ranked frame in the tracker's slot, from the frame set the slot remembers into the slot's crop
// set, and the crop set tracker_hand_out keeps -- both do nothing while crops are off.  And what target crops and crop tensors
// share (what: the call's name in a refusal): the CropLaunch base from a tracker's slot and from the context's table of explicit
// windows; the checks of a mode, of a window's size, and of what the context must be for a crop switch to go on; an explicit call's
// own checks (check_windows: per_stream and the window) and the rest up to its launch (load_windows: results outstanding, the
// context drained, the caller's windows in the context's table -- made on first use, built aside).
int crops_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, hipStream_t st);
void crops_keep(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot);
void crop_launch_from_slot(CropLaunch &a, const oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, int mode, int h, int w);
void crop_launch_from_table(CropLaunch &a, const oatgpu_ctx *c, const void *frames_dev, int per_stream, int h, int w);
int check_crop_mode(oatgpu_ctx *c, const char *what, int mode);
int check_crop_size(oatgpu_ctx *c, const char *what, int h, int w);
int check_crop_zoom(oatgpu_ctx *c, const char *what, double zoom);
int check_window_riders(oatgpu_ctx *c, const char *what, int mode);
int check_crop_switch(oatgpu_ctx *c, const char *what, int mode);
int check_windows(oatgpu_ctx *c, const char *what, int per_stream, int h, int w);
int load_windows(oatgpu_ctx *c, const char *what, const oatgpu_crop_window *win, int per_stream);
// api_croptensor.hip: crops_launch's neighbour -- k_crop_tensor behind it on the same stream, from the slot's frame set into the
// entry the slot remembers of the caller's memory --, the count tracker_hand_out keeps, and the refusal of a sequence call of more
// frames than the caller's memory has entries.  All do nothing while crop tensors are off.
int crop_tensor_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, hipStream_t st);
void crop_tensor_keep(oatgpu_ctx *c);
int crop_tensor_room(oatgpu_ctx *c, int n_frames, const char *what);
// api_targetmask.hip: crop_tensor_launch's neighbour -- k_target_mask behind it on the same stream, from the scratch set bb of the
// slot's back half into the entry the slot remembers of the caller's memory --, the count tracker_hand_out keeps, and the refusal
// of a sequence call of more frames than the caller's memory has entries.  All do nothing while target masks are off.
int mask_tensor_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, const BlobBuffers &bb, int slot, hipStream_t st);
void mask_tensor_keep(oatgpu_ctx *c);
int mask_tensor_room(oatgpu_ctx *c, int n_frames, const char *what);
// api_tracks.hip: k_target_tracks on the target set of the tracker's slot `slot`, on st behind its ranking, into the slot's track set;
// the filter chain on the slot's result records behind that.  Inside a sequence call (st is a B stream) consecutive frames sit on
// different HIP streams: each launch waits for its own event of the frame before it (prev_slot) and records its own; the
// synchronous step runs on stream A alone and needs neither.  Each does nothing while its switch is off.
int tracks_launch(oatgpu_ctx *c, const TargetSets &ts, int slot, int prev_slot, hipStream_t st);
int tracker_filters_launch(oatgpu_ctx *c, const ResultRec *rec_dev, int slot, int prev_slot, hipStream_t st);      // (api_trackfilt.hip)
// api_measure.hip
void prof_fold(oatgpu_ctx *c);
#pragma GCC visibility pop

// A Delivered list to its reader, behind the reader's null checks -> the number of sets
template <class T>
static int delivered_to(oatgpu_ctx *c, const Delivered<T> &d, bool on, const char *off, const char *none_yet, void *out, int max_sets)
{
    const int rc = delivered_refusals(c, on, off, none_yet, d.sets, max_sets);
    if (rc) return rc;
    memcpy(out, d.items.data(), (size_t)d.sets * d.per * sizeof(T));
    return d.sets;
}

// The homes of target sets: f(sets, slots, of_tracker, on) for the result ring and the two batched trackers' slots; on: the home
// exists at the moment (a tracker that is off has no sets)
template <class F> static void for_each_target_home(oatgpu_ctx *c, F f)
{
    f(c->tg.ring, (size_t)c->ring_slots + 1, false, true);
    f(c->df.tgt, (size_t)kSeqSlots, true, c->df.on);
    f(c->bs.tgt, (size_t)kSeqSlots, true, c->bs.on);
}
// ... and the family's switches as they stand
static inline TargetWants wants_of(const oatgpu_ctx *c)
{
    return {c->tg.k, c->tg.shapes, c->tg.crop_mode, c->tg.crop_h, c->tg.crop_w, c->tk.on};
}

// the ten values of a detector: an oatgpu_marker holds a marker's, the context's own come out of its config
static inline oatgpu_marker detector_of(const oatgpu_config &k)
{
    return {k.h_lo, k.h_hi, k.s_lo, k.s_hi, k.v_lo, k.v_hi, k.erode, k.dilate, k.min_area, k.max_area};
}

// cv::inRange's scalar-bound normalisation for 8U sources
static inline void norm_range(int lo, int hi, int &l, int &h)
{
    if (lo > hi || lo > 255 || hi < 0) { l = 1; h = 0; return; }
    l = lo < 0 ? 0 : lo;
    h = hi > 255 ? 255 : hi;
}
static inline RangeParams range_of(const oatgpu_marker &k)
{
    RangeParams r;
    norm_range(k.h_lo, k.h_hi, r.lo[0], r.hi[0]);
    norm_range(k.s_lo, k.s_hi, r.lo[1], r.hi[1]);
    norm_range(k.v_lo, k.v_hi, r.lo[2], r.hi[2]);
    return r;
}

// bytes of one camera's frame as the fused track calls take it: RAW8 with oatgpu_set_track_bayer on
static inline size_t track_in_bytes(const oatgpu_ctx *c) { return (size_t)c->g.H * c->g.W * (c->by_track ? 1 : c->cfg.channels); }
// ... and as the motion and the subtraction tracker take it: RAW8 with oatgpu_set_tracker_bayer on
static inline size_t tracker_in_bytes(const oatgpu_ctx *c) { return (size_t)c->g.H * c->g.W * (c->tb_on ? 1 : c->cfg.channels); }
// ... and what the front launch of either takes from the context: frame set f1 (f2: and the next) into the bits of `slot` (and
// slot2), the ROI, the Bayer patterns with oatgpu_set_tracker_bayer on, the streams' maps with oatgpu_set_tracker_undistort on
// (the slots remember their frame set here, and its place `entry` in the call -- f2's is entry + 1: k_target_crops and k_crop_tensor
// cut from it behind the slot's ranking, the latter into that entry of the caller's memory)
static inline void tracker_front(const oatgpu_ctx *c, BatchedTrackerState &bt, const void *f1, const void *f2, int slot, int slot2, int entry,
                                 FrontLaunch &a)
{
    a.frames = (const uint8_t *)f1; a.frames2 = (const uint8_t *)f2; a.channels = c->cfg.channels;
    bt.frame[slot] = a.frames; bt.entry[slot] = entry;
    if (f2) { bt.frame[slot2] = a.frames2; bt.entry[slot2] = entry + 1; }
    a.bits = bt.bits_of(slot); a.bits2 = f2 ? bt.bits_of(slot2) : nullptr;
    a.roi = c->roi;
    a.bayer = c->tb_on ? c->tb_pat.data() : nullptr;
    if (c->tu_on) { a.ud_map1 = c->ud_map1; a.ud_map2 = c->ud_map2; a.ud_stride = c->ud_stride; }
}
// frame i of the step as K1 and the marker kernels see it: remapped, demosaiced, or the caller's own
static inline const uint8_t *step_frame(const oatgpu_ctx *c, int i, const void *given)
{
    return c->ud_track ? (const uint8_t *)c->ud_frames[i] : c->by_track ? (const uint8_t *)c->by_frames[i] : (const uint8_t *)given;
}

// ring slot of the next frame to be enqueued / collected
static inline int enq_slot(const oatgpu_ctx *c) { return (int)(c->enq_total % (unsigned long long)c->ring_slots); }
static inline int col_slot(const oatgpu_ctx *c) { return (int)(c->col_total % (unsigned long long)c->ring_slots); }

static inline u64 *thr_buf(oatgpu_ctx *c, int parity)
{
    return c->thr + (size_t)parity * c->cfg.n_streams * (c->g.Palloc >> 6);
}

// B streams of the plain order for a frame.  Host frames arrive over the copy stream: use one B stream fewer then: the copy
// stream sits on the last B stream's hardware queue (see acquire_streams)
static inline int plain_b_streams(const oatgpu_ctx::FrameJob &f) { return f.ready ? 2 : oatgpu_ctx::kNB; }

// The switch of a batched tracker (oatgpu_set_diff_tracker, oatgpu_set_bsub_tracker; c is not null).  Off: the tracker is dropped.
// On: a new one is built aside -- extra(made, ok) first: what this tracker needs besides, an error code or ok = false for a failed
// allocation -- and the context takes it when everything worked.
template <class Tracker, class Extra> static int set_batched_tracker(oatgpu_ctx *c, Tracker &cur, int on, const char *name, Extra extra)
{
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_%s_tracker while enqueued results are outstanding", name);
    if (!on == !cur.on) return OATGPU_OK;
    int rc = open_sync(c);
    if (rc) return rc;
    if (!on) { cur = Tracker{}; return OATGPU_OK; }
    Tracker made;
    bool ok = true;
    rc = extra(made, ok);
    if (rc) return rc;
    if (!ok || !made.alloc(c)) return fail(c, OATGPU_E_NOMEM, "%s tracker: allocation failed: %s", name, hipGetErrorString(hipGetLastError()));
    cur = std::move(made);
    return OATGPU_OK;
}

// The body of oatgpu_set_marker_filters and oatgpu_set_tracker_filters (c is not null).  Everything is checked before anything
// changes: results outstanding; `refused`, the text of the owner's own precondition where it does not hold (nullptr: it holds);
// the parameters (chain_params).  Nothing asked for: the chain is dropped.  First use: a chain is built aside -- extra(made, n):
// the owner's own buffers, false for a failed allocation -- and the context takes it when everything worked.  Then the parameters
// go up and every stream's filter starts from the reference's initial state.
template <class Chain, class Extra>
static int configure_chain(oatgpu_ctx *c, Chain &cur, const oatgpu_marker_filters *f, const char *who, const char *refused, Extra extra)
{
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_%s_filters while enqueued results are outstanding", who);
    if (refused) return fail(c, OATGPU_E_INVALID, "%s", refused);
    const bool on = f && (f->kalman || f->homography || f->n_regions > 0);
    std::vector<MarkerFilterParams> hp(on ? 1 : 0);      // (8 KiB: not on the stack)
    if (on) {
        const int prc = chain_params(c, f, hp[0]);
        if (prc) return prc;
    }
    int rc = open_sync(c);
    if (rc) return rc;
    if (!on) { cur = {}; return OATGPU_OK; }
    const size_t n = (size_t)c->cfg.n_streams;
    Chain made;
    const bool first = !cur.params;
    Chain &ch = first ? made : cur;
    if (first) {
        bool ok = ch.params.alloc(sizeof(MarkerFilterParams)) == hipSuccess;
        ok = ok && ch.state.alloc(n * sizeof(KalmanState)) == hipSuccess;
        ok = ok && extra(ch, n);
        if (!ok) return fail(c, OATGPU_E_NOMEM, "%s filters: allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        ch.last.items.reserve(n);
    }
    HIPCHK(c, hipMemcpy(ch.params, hp.data(), sizeof(MarkerFilterParams), hipMemcpyHostToDevice));
    launch_kalman_reset(ch.state, (int)n, 0u, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (first) cur = std::move(made);
    cur.on = true;
    cur.last.begin();
    return OATGPU_OK;
}

// A recorded sequence of a batched tracker (api_diff.hip, api_bsubtrack.hip) with up to kSeqSlots frames in flight.  Front launches
// go to stream A, frames_of(t) (1 or 2) frames a launch; front(t, nf, q, q2) issues the one for frames t (.. t + 1) into slots q
// (and q2); frame t's back half -- back(slot, i, B), i = its place in the front launch -- runs on B[t % 3] behind the front launch's
// event in slot t % kSeqSlots, and a slot is reused only after hand_out(slot, frame) has collected it.  Everything is collected
// before the call returns; on an error nothing of the call stays in flight.
template <class FramesOf, class Front, class Back, class HandOut>
static int run_sequence_in_flight(oatgpu_ctx *c, int n_frames, Event *ev_front, Event *ev_done, FramesOf frames_of, Front front,
                                  Back back, HandOut hand_out)
{
    constexpr int K = kSeqSlots;
    int got = 0, rc = OATGPU_OK;
    auto collect_one = [&]() -> int {
        const int q = got % K;
        HIPCHK(c, hipEventSynchronize(ev_done[q]));
        hand_out(q, got);
        ++got;
        return OATGPU_OK;
    };
    auto back_on_b = [&](int t, int i, hipEvent_t front_done) -> int {
        const int q = t % K, b = t % oatgpu_ctx::kNB;
        hipStream_t B = c->stream_b[b];
        c->b_used[b] = true;
        HIPCHK(c, hipStreamWaitEvent(B, front_done, 0));
        const int r = back(q, i, B);
        if (r) return r;
        HIPCHK(c, hipEventRecord(ev_done[q], B));
        return OATGPU_OK;
    };
    int t = 0;
    while (t < n_frames && !rc) {
        const int nf = frames_of(t);
        while (!rc && t + nf - got > K) rc = collect_one();
        if (rc) break;
        const int q = t % K;
        rc = front(t, nf, q, (t + 1) % K);
        if (rc) break;
        hipError_t e = hipEventRecord(ev_front[q], c->stream);
        if (e != hipSuccess) { rc = fail(c, OATGPU_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e)); break; }
        rc = back_on_b(t, 0, ev_front[q]);
        if (!rc && nf == 2) rc = back_on_b(t + 1, 1, ev_front[q]);
        if (rc) break;
        t += nf;
    }
    while (!rc && got < n_frames) rc = collect_one();
    if (rc) { (void)hipStreamSynchronize(c->stream); (void)drain_b(c); }       // nothing of this call stays in flight
    return rc;
}

static inline void mark_speculative(oatgpu_ctx *c, int slot)
{
    c->slots[slot].spec = true;
    c->slots[slot].filtered = false;
}
