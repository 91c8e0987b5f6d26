// oat-posidet-hip TYPE SOURCE SINK [CONFIGURATION]
//   TYPE  hsv     replacement of `oat posidet hsv`    (src/positiondetector/HSVDetector.cpp)
//         thresh  replacement of `oat posidet thresh` (src/positiondetector/SimpleThreshold.cpp)
//         diff    replacement of `oat posidet diff`   (src/positiondetector/DifferenceDetector.cpp)
//                 diff --bgr: of the chain `oat framefilt col -C GREY` -> `oat posidet diff` on a BGR source (the motion tracker)
//                 hsv --bsub: of the chain `oat framefilt bsub` -> `oat framefilt col -C HSV` -> `oat posidet hsv` on a BGR source,
//                 thresh --bsub: of `oat framefilt bsub` -> `oat posidet thresh` on a GREY source (the subtraction tracker)
//                 diff --bayer P, hsv --bsub --bayer P: the two BGR chains on a GREY-tagged Bayer RAW8 source (a colour camera's
//                 own pixel format, PointGreyCam.cpp:48-50): the demosaic is done in the same kernel (oatgpu_set_tracker_bayer)
//                 diff [--bgr], hsv --bsub, thresh --bsub with --camera-matrix K --distortion-coeffs D: `oat framefilt undistort`
//                 (Undistorter.cpp:83-88) in front of the chain, done in the same kernel (oatgpu_set_tracker_undistort); a plain
//                 `diff` then runs the motion tracker on its GREY source
//                 diff [--bgr|--bayer P], hsv --bsub, thresh --bsub with --kalman / --homography H / --region R: `oat posifilt
//                 kalman` -> `oat posifilt homography` -> `oat posifilt region` behind the detector, on the device in the same step
//                 (oatgpu_set_tracker_filters): the SINK carries the filtered Position2D; a plain `diff` then runs the motion
//                 tracker on its GREY source
//                 every TYPE and form with --target-sinks T0,T1,..: the K largest blobs of the frame, ranked (oatgpu_set_targets):
//                 sink j receives rank j as a Position2D with the frame's Sample on every frame, invalid where the rank is empty;
//                 the SINK carries what it carries without the option
//                 diff [--bgr|--bayer P], hsv --bsub, thresh --bsub with --track-sinks T0,T1,.. --kalman ..: target tracks
//                 (oatgpu_set_tracks): K = the list's length persistent track slots behind the K ranked blobs; sink i carries slot
//                 i's filtered Position2D on every frame, invalid while the slot is empty -- the slot is the identity on the wire
//                 diff [--bgr], hsv --bsub, thresh --bsub with --crop-sinks C0,C1,.. --crop-size HxW [--crop-axis] beside
//                 --target-sinks or --track-sinks: target crops (oatgpu_set_target_crops): frame sink j carries rank j's H x W window
//                 of the SOURCE frame (with --track-sinks: the window of the rank track slot j took) in the source's colour with
//                 the frame's Sample on every frame, zeros where there is none
// Same positional arguments and option names as src/positiondetector/main.cpp:85-271.
#include "component.hpp"
#include "filter_chain.hpp"
#include "target_sinks.hpp"

#include <algorithm>
#include <cfloat>

using namespace oat;

enum class Kind { HSV, THRESH, DIFF };

class GpuDetector : public PositionDetector {
public:
    // bayer: 0, or the OATGPU_BAYER_* pattern of a RAW8 source (GREY-tagged) in front of a BGR chain
    // undistort: the calibration of `framefilt undistort` in front of a batched tracker's chain, or nullptr
    // filters: a filter chain behind the detector (kalman_ / homography_on_ / regions_ below): the batched trackers have one
    GpuDetector(const std::string &src, const std::string &snk, Kind kind, bool bgr = false, bool bsub = false, int bayer = 0,
                const UndistortCalibration *undistort = nullptr, bool filters = false)
        : PositionDetector(src, snk), kind_(kind), bgr_(bgr && kind == Kind::DIFF), bsub_(bsub && kind != Kind::DIFF), bayer_(bayer)
    {
        oatgpu_default_config(&cfg_);
        if (undistort) { undistort_ = *undistort; undistort_on_ = true; }
        // the motion tracker: a BGR source, a remap in front, or a filter chain behind
        difftrk_ = bgr_ || (kind == Kind::DIFF && (undistort_on_ || filters));
        if (bgr_) { required_color_ = PIX_BGR; cfg_.channels = 3; cfg_.erode = 0; cfg_.dilate = 0; }
        else if (difftrk_) { required_color_ = PIX_GREY; cfg_.channels = 1; cfg_.erode = 0; cfg_.dilate = 0; }
        else if (bsub_ && kind == Kind::HSV) { required_color_ = PIX_BGR; cfg_.channels = 3; cfg_.erode = 0; cfg_.dilate = 10; }
        else if (bsub_) { required_color_ = PIX_GREY; cfg_.channels = 1; cfg_.erode = 0; cfg_.dilate = 0; }
        else if (kind == Kind::HSV) { required_color_ = PIX_HSV; cfg_.erode = 0; cfg_.dilate = 10; }   // HSVDetector.cpp:42-46
        else { required_color_ = PIX_GREY; cfg_.erode = 0; cfg_.dilate = 0; }   // SimpleThreshold.cpp:42-46, DifferenceDetector.cpp:41-44
        if (bayer_) required_color_ = PIX_GREY;          // one sample a pixel, as `oat-frameserve-raw -C GREY` serves RAW8
    }
    oatgpu_config cfg_;
    double bsub_alpha_{0.0};            // --bsub-alpha: framefilt bsub's -a (BackgroundSubtractor.h)
    std::string bsub_background_;       // --bsub-background: framefilt bsub's -f, PGM/PPM instead of cv::imread's formats
    // the filter chain behind a batched tracker (--kalman / --homography / --region): the SINK then carries the filtered Position2D
    bool kalman_{false}, homography_on_{false};
    double dt_{0.02}, timeout_{0.0}, sig_accel_{5.0}, sig_noise_{0.0};      // KalmanFilter2D.cpp:69-85
    double homography_[9]{1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<RegionDef> regions_;
    bool chain_on() const { return kalman_ || homography_on_ || !regions_.empty(); }
    std::vector<std::string> target_sink_addresses_;     // --target-sinks: rank j of every frame on the j-th address
    bool target_shape_{false};                           // --target-shape: rank j's token carries the blob's body axis as its heading
    std::vector<std::string> track_sink_addresses_;      // --track-sinks: track slot i of every frame on the i-th address
    double track_gate_{HUGE_VAL};                        // --track-gate: pixels (default: no gate)
    std::vector<std::string> crop_sink_addresses_;       // --crop-sinks: rank j's (track slot j's) window of every frame on the j-th address
    int crop_h_{0}, crop_w_{0};                          // --crop-size HxW
    bool crop_axis_{false};                              // --crop-axis: the window is turned to the blob's body axis
    // the sinks beside the SINK: the target sinks, then the track sinks
    std::vector<std::string> extra_sink_addresses() const
    {
        std::vector<std::string> v = target_sink_addresses_;
        v.insert(v.end(), track_sink_addresses_.begin(), track_sink_addresses_.end());
        return v;
    }

protected:
    // (a detector that fails while connecting still binds its target sinks, so that its destructor sets them END)
    bool connectToNode() override
    {
        try {
            return PositionDetector::connectToNode();
        } catch (...) {
            bind_target_sinks(false);
            bind_crop_sinks(false);
            throw;
        }
    }
    // the crop sinks: frame sinks of crop_h_ x crop_w_ pixels in the source's colour
    void bind_crop_sinks(bool loud)
    {
        const size_t bytes = (size_t)crop_h_ * crop_w_ * color_bytes(required_color_);
        if (crop_sinks_.empty()) crop_sinks_ = std::vector<Sink<Frame>>(crop_sink_addresses_.size());
        for (size_t j = crop_shared_.size(); j < crop_sinks_.size(); ++j) {
            try {
                crop_sinks_[j].bind(crop_sink_addresses_[j], bytes);
                crop_shared_.push_back(crop_sinks_[j].retrieve((size_t)crop_h_, (size_t)crop_w_, color_cvtype(required_color_), required_color_));
            } catch (...) {
                if (loud) throw;
                return;
            }
        }
    }
    // the frame's windows to their sinks, every one with the frame's Sample: rank j's on sink j, or, with track sinks, the window
    // of the rank slot j took this frame; zeros where there is none
    void publish_crops(const Position2D &position)
    {
        const size_t C = crop_sink_addresses_.size();
        if (!C) return;
        const size_t K = std::max(target_sink_addresses_.size(), track_sink_addresses_.size());
        const size_t bytes = (size_t)crop_h_ * crop_w_ * color_bytes(required_color_);
        crop_set_.resize(K * bytes);
        if (oatgpu_target_crops(gpu_.ctx, crop_set_.data(), 1) != 1) gpu_.check(OATGPU_E_INVALID);
        oatgpu_track slots[OATGPU_MAX_TARGETS];
        const bool by_track = !track_sink_addresses_.empty();
        if (by_track && oatgpu_tracks(gpu_.ctx, slots, 1) != 1) gpu_.check(OATGPU_E_INVALID);
        for (size_t j = 0; j < C; ++j) {
            const int rank = by_track ? (slots[j].id ? slots[j].rank : -1) : (int)j;
            crop_sinks_[j].wait();
            if (rank >= 0) memcpy(crop_shared_[j].data(), crop_set_.data() + (size_t)rank * bytes, bytes);
            else memset(crop_shared_[j].data(), 0, bytes);
            crop_shared_[j].sample() = position.sample();
            crop_sinks_[j].post();
        }
    }
    void bind_target_sinks(bool loud)
    {
        const std::vector<std::string> names = extra_sink_addresses();
        if (target_sinks_.empty()) target_sinks_ = std::vector<Sink<Position2D>>(names.size());
        for (size_t j = target_shared_.size(); j < target_sinks_.size(); ++j) {
            try {
                target_sinks_[j].bind(names[j], names[j]);
                target_shared_.push_back(target_sinks_[j].retrieve());
            } catch (...) {
                if (loud) throw;
                return;
            }
        }
    }
    // the frame's ranks to their sinks, every one with the frame's Sample
    void publish_targets(const Position2D &position)
    {
        const size_t K = target_sink_addresses_.size();
        if (!K) return;
        oatgpu_position ranks[OATGPU_MAX_TARGETS];
        int32_t found = 0;
        if (oatgpu_targets(gpu_.ctx, ranks, &found, 1) != 1) gpu_.check(OATGPU_E_INVALID);
        oatgpu_shape shapes[OATGPU_MAX_TARGETS];
        if (target_shape_ && oatgpu_target_shapes(gpu_.ctx, shapes, 1) != 1) gpu_.check(OATGPU_E_INVALID);
        for (size_t j = 0; j < K; ++j) {
            target_sinks_[j].wait();
            *target_shared_[j] = target_position(ranks[j], position.sample(), target_shape_ ? &shapes[j] : nullptr);
            target_sinks_[j].post();
        }
    }
    // the frame's track slots to their sinks (behind the target sinks in target_sinks_), every one with the frame's Sample
    void publish_tracks(const Position2D &position)
    {
        const size_t K = track_sink_addresses_.size(), first = target_sink_addresses_.size();
        if (!K) return;
        oatgpu_track slots[OATGPU_MAX_TARGETS];
        if (oatgpu_tracks(gpu_.ctx, slots, 1) != 1) gpu_.check(OATGPU_E_INVALID);
        for (size_t i = 0; i < K; ++i) {
            Position2D pos("");
            pos.set_sample(position.sample());
            publish_filtered(pos, slots[i].filtered, regions_, homography_on_ ? homography_ : nullptr);
            target_sinks_[first + i].wait();
            *target_shared_[first + i] = pos;
            target_sinks_[first + i].post();
        }
    }
    oatgpu_marker_filters chain_of(std::vector<oatgpu_region> &rs) const
    {
        oatgpu_marker_filters f = chain_filters(regions_, rs);
        f.kalman = kalman_; f.dt = dt_; f.timeout = timeout_; f.sigma_accel = sig_accel_; f.sigma_noise = sig_noise_;
        f.homography = homography_on_;
        std::copy(homography_, homography_ + 9, f.h);
        return f;
    }
    void configure_for(const FrameParams &p) override
    {
        cfg_.rows = (int)p.rows; cfg_.cols = (int)p.cols; cfg_.n_streams = 1;
        gpu_.create(cfg_);
        if (difftrk_) gpu_.check(oatgpu_set_diff_tracker(gpu_.ctx, 1));
        if (bayer_) { const int32_t pat = bayer_; gpu_.check(oatgpu_set_tracker_bayer(gpu_.ctx, &pat, 1)); }
        if (bsub_) {
            gpu_.check(oatgpu_set_bsub_tracker(gpu_.ctx, 1));
            if (!bsub_background_.empty()) {                 // BackgroundSubtractor.cpp:63-71: imread(.., COLOR)
                const PnmImage im = read_background_image(bsub_background_, p.rows, p.cols, cfg_.channels);
                gpu_.check(oatgpu_bsub_set_background(gpu_.ctx, 0, im.px.data()));
            }
        }
        if (undistort_on_) {                                 // (a background image is one in undistorted coordinates)
            gpu_.check(oatgpu_set_undistort(gpu_.ctx, 0, undistort_.K, undistort_.dist.data(), (int32_t)undistort_.dist.size()));
            gpu_.check(oatgpu_set_tracker_undistort(gpu_.ctx, 1));
        }
        if (chain_on()) {
            std::vector<oatgpu_region> rs;
            const oatgpu_marker_filters f = chain_of(rs);
            gpu_.check(oatgpu_set_tracker_filters(gpu_.ctx, &f));
        }
        const size_t n_targets = std::max(target_sink_addresses_.size(), track_sink_addresses_.size());      // (equal where both are given)
        if (n_targets) gpu_.check(oatgpu_set_targets(gpu_.ctx, (int32_t)n_targets));
        if (target_shape_) gpu_.check(oatgpu_set_target_shapes(gpu_.ctx, 1));
        if (!track_sink_addresses_.empty()) {                // the chain options describe the tracks too
            std::vector<oatgpu_region> rs;
            const oatgpu_marker_filters f = chain_of(rs);
            gpu_.check(oatgpu_set_tracks(gpu_.ctx, &f, track_gate_));
        }
        if (!crop_sink_addresses_.empty())
            gpu_.check(oatgpu_set_target_crops(gpu_.ctx, crop_axis_ ? OATGPU_CROP_AXIS : OATGPU_CROP_UPRIGHT, crop_h_, crop_w_));
        if (n_targets) bind_target_sinks(true);
        bind_crop_sinks(true);
    }
    // HSVDetector.cpp:142-173 / SimpleThreshold.cpp:114-134
    // Deferred (oatgpu_set_deferred): the call returns when the frame has left shared memory, PositionDetector::process posts
    // the source, and detect_finish() waits for the kernels and takes the position (PositionDetector.cpp:78-96).
    bool detect_from_shm(const Frame &frame, Position2D &) override
    {
        if (difftrk_ || bsub_) return false;  // the batched trackers' step is synchronous: the frame is copied and the source posted first
        if (!extra_sink_addresses().empty()) return false;       // (targets do not go with deferred completion: the synchronous call)
        if (!deferred_on_) { gpu_.check(oatgpu_set_deferred(gpu_.ctx, 1)); deferred_on_ = true; }
        gpu_.check(kind_ == Kind::HSV ? oatgpu_detect_hsv(gpu_.ctx, 0, frame.data(), nullptr)
                   : kind_ == Kind::THRESH ? oatgpu_detect_thresh(gpu_.ctx, 0, frame.data(), nullptr)
                                           : oatgpu_detect_diff(gpu_.ctx, 0, frame.data(), nullptr));
        return true;
    }
    void detect_finish(Position2D &position) override
    {
        oatgpu_position r;
        gpu_.check(oatgpu_fetch_position(gpu_.ctx, &r));
        position.position_valid = r.valid != 0;                   // DetectorFunc.cpp:46,58-60
        if (r.valid) { position.position.x = r.x; position.position.y = r.y; }
    }
    void detectPosition(Frame &frame, Position2D &position) override
    {
        oatgpu_position r;
        const uint8_t *one[1] = {frame.data()};
        gpu_.check(difftrk_ ? oatgpu_diff_batch(gpu_.ctx, one, 1, &r)
                   : bsub_ ? oatgpu_bsub_track_batch(gpu_.ctx, one, 1, bsub_alpha_, &r)
                   : kind_ == Kind::HSV ? oatgpu_detect_hsv(gpu_.ctx, 0, frame.data(), &r)
                   : kind_ == Kind::THRESH ? oatgpu_detect_thresh(gpu_.ctx, 0, frame.data(), &r)
                                           : oatgpu_detect_diff(gpu_.ctx, 0, frame.data(), &r));
        position.position_valid = r.valid != 0;                   // DetectorFunc.cpp:46,58-60
        if (r.valid) { position.position.x = r.x; position.position.y = r.y; }
        if (chain_on()) {                                         // ... behind posifilt kalman / homography / region
            oatgpu_filtered f;
            if (oatgpu_tracker_filtered(gpu_.ctx, &f, 1) != 1) gpu_.check(OATGPU_E_INVALID);
            publish_filtered(position, f, regions_, homography_on_ ? homography_ : nullptr);
        }
        publish_targets(position);
        publish_tracks(position);
        publish_crops(position);
    }
    Kind kind_;
    bool bgr_, bsub_;
    int bayer_;
    bool difftrk_{false}, undistort_on_{false};
    UndistortCalibration undistort_{};
    bool deferred_on_{false};
    GpuCtx gpu_;
    std::vector<Sink<Position2D>> target_sinks_;         // [K] (after gpu_: the sinks go END before the context is destroyed)
    std::vector<Position2D *> target_shared_;
    std::vector<Sink<Frame>> crop_sinks_;                // [C] frame sinks behind them
    std::vector<Frame> crop_shared_;
    std::vector<uint8_t> crop_set_;                      // the frame's crop set, [K][h][w][channels]
};

static void usage()
{
    std::cout << "Usage: oat-posidet-hip TYPE SOURCE SINK [CONFIGURATION]\nTYPE\n  hsv | thresh | diff\n"
                 "diff:   -d diff-threshold (default 10)  -b blur (default 2, <= 22)  -a [min,max] area\n"
                 "        --bgr  the SOURCE is BGR: framefilt col -C GREY is done in front of the detector, in the same kernel\n"
                 "        --bayer RGGB|BGGR|GRBG|GBRG  the SOURCE is Bayer RAW8 (GREY-tagged, the 2 x 2 tile at rows 0-1, columns 0-1):\n"
                 "        demosaic and framefilt col -C GREY are done in front of the detector, in the same kernel (selects the BGR chain)\n"
                 "hsv:    -H/-S/-V [min,max] in [0,256]  -e erode  -d dilate (default 10)  -a [min,max] area\n"
                 "thresh: -T [min,max]  -e erode  -d dilate  -a [min,max] area\n"
                 "hsv, thresh: --bsub  framefilt bsub (and, for hsv, col -C HSV) is done in front of the detector, in the same kernel:\n"
                 "        the SOURCE is then BGR for hsv, GREY for thresh\n"
                 "        --bsub-alpha A  bsub's adaptation coefficient, 0..1 (default 0: the first frame stays the background)\n"
                 "        --bsub-background FILE.ppm|.pgm  the background image instead of the first frame (it cannot adapt)\n"
                 "        --bayer P  with hsv --bsub: the SOURCE is Bayer RAW8 (GREY-tagged), demosaiced in the same kernel; a background\n"
                 "        image stays BGR\n"
                 "diff, hsv --bsub, thresh --bsub:\n"
                 "        --camera-matrix [K11,K12,...,K33] --distortion-coeffs [k1,k2,p1,p2,k3] or [k1,k2,p1,p2,k3,k4,k5,k6]\n"
                 "        framefilt undistort is done in front of the chain, in the same kernel (both are needed; not with --bayer)\n"
                 "        --kalman [--dt s] [--timeout s] [--sigma-accel a] [--sigma-noise n]  --homography [h11,h12,...,h33]\n"
                 "        --region 'NAME=[[x0,y0],[x1,y1],...]' (repeatable; at most 16 regions of 64 points, a name of at most 9 bytes)\n"
                 "        posifilt kalman, posifilt homography and posifilt region behind the detector, in this order, each on its own, on\n"
                 "        the device in the same step: the SINK carries the filtered position -- position and velocity of the Kalman\n"
                 "        filter (defaults dt 0.02, timeout 0, sigma-accel 5, sigma-noise 0), WORLD units with the matrix, the name of\n"
                 "        the first region (command-line order) that holds the position.  In a -c file: kalman = true, dt = .., homography\n"
                 "        = [..] and one [[KEY.region]] table per region with name and points.  Long names only (-T is thresh's window).\n"
                 "        hsv and thresh need --bsub for them; a plain diff runs the motion tracker on its GREY source.\n"
                 "all:    --gpu-index N  HIP device ordinal (default 0)\n"
                 "        --target-sinks T0,T1,..  (at most 8 names; target-sinks = \"T0,T1\" in a -c file) multi-target detection: the K\n"
                 "        largest blobs inside the area window, ranked by area (ties: the later first pixel first); rank j of every frame\n"
                 "        goes to sink Tj as a Position2D with the frame's sample, invalid where fewer than j + 1 blobs exist.  Rank 0 is\n"
                 "        the detector's own result; the SINK carries what it carries without the option.  Targets are raw detections:\n"
                 "        a filter chain acts on the SINK only.\n"
                 "        --target-shape  (with --target-sinks; target-shape = true in a -c file) target shapes: rank j's Position2D also\n"
                 "        carries the blob's body axis -- the major axis of its second moments, a unit vector with x >= 0: an axis has no\n"
                 "        front -- as its heading; no heading where the blob has no axis (a square, a disc).\n"
                 "diff, hsv --bsub, thresh --bsub:\n"
                 "        --track-sinks T0,T1,.. [--track-gate PX] --kalman [..] [--homography ..] [--region ..]  (at most 8 names) target\n"
                 "        tracks: K = the number of names persistent track slots behind the K ranked blobs -- each frame's blobs are\n"
                 "        assigned to the slots by greedy nearest neighbour inside PX pixels (default: no gate) of where the slot's\n"
                 "        Kalman filter expects its object, new objects take free slots.  Sink Ti carries slot i's filtered Position2D\n"
                 "        with the frame's sample on every frame (position, velocity, region, WORLD units under a homography), invalid\n"
                 "        while the slot is empty: the slot is the identity.  Switches targets on itself; the chain options describe\n"
                 "        both the SINK's chain and the tracks.  With --target-sinks too, both lists have the same length.\n"
                 "diff [--bgr], hsv --bsub, thresh --bsub:\n"
                 "        --crop-sinks C0,C1,.. --crop-size HxW [--crop-axis]  (beside --target-sinks or --track-sinks; at most K names;\n"
                 "        crop-sinks = \"C0,C1\", crop-size = \"64x64\", crop-axis = true in a -c file) target crops: frame sink Cj carries\n"
                 "        the H x W window of the SOURCE frame around rank j's centroid, in the source's colour with the frame's sample,\n"
                 "        on every frame; zeros where the rank is empty.  1 <= H <= 256, 4 <= W <= 256, W a multiple of 4.  --crop-axis\n"
                 "        (needs --target-shape) turns each window so that the blob's body axis lies along its +x; a blob without an\n"
                 "        axis keeps the upright window.  With --track-sinks, sink Ci carries the window of the rank track slot i took,\n"
                 "        zeros while the slot has none: the sink is the identity.  Not with --bayer or --camera-matrix.\n";
}

int main(int argc, char **argv)
{
    try {
        // -d is "dilate" for hsv/thresh and "diff-threshold" for diff (DifferenceDetector.cpp:49-50)
        const bool is_diff = argc > 1 && std::string(argv[1]) == "diff";
        Options o = Options::parse(argc, argv,
            {{"H", "h-thresh"}, {"S", "s-thresh"}, {"V", "v-thresh"}, {"T", "thresh"}, {"e", "erode"},
             {"d", is_diff ? "diff-threshold" : "dilate"}, {"b", "blur"}, {"a", "area"}, {"t", "tune"}, {"h", "help"}, {"v", "version"}},
            {"help", "version", "tune", "bgr", "bsub", "kalman", "target-shape", "crop-axis"});
        if (o.has("version")) { std::cout << "oat-posidet-hip (MI355X drop-in, liboatgpu ABI " << oatgpu_abi_version() << ")\n"; return 0; }
        if (o.has("help") || o.positional.size() != 3) { usage(); return o.has("help") ? 0 : -1; }
        const std::string type = o.positional[0];
        if (type != "hsv" && type != "thresh" && type != "diff") throw std::runtime_error("Selected TYPE is invalid.");
        // option names per TYPE: HSVDetector.cpp:49-75, SimpleThreshold.cpp:49-69, DifferenceDetector.cpp:41-62
        if (type == "hsv")
            o.apply_config({"h-thresh", "s-thresh", "v-thresh", "erode", "dilate", "area", "tune", "gpu-index", "bsub", "bsub-alpha", "bsub-background", "bayer",
                            "camera-matrix", "distortion-coeffs", "kalman", "dt", "timeout", "sigma-accel", "sigma-noise", "homography", "target-sinks", "target-shape", "track-sinks", "track-gate", "crop-sinks", "crop-size", "crop-axis"},
                           {"tune", "bsub", "kalman", "target-shape", "crop-axis"});
        else if (type == "thresh")
            o.apply_config({"thresh", "erode", "dilate", "area", "tune", "gpu-index", "bsub", "bsub-alpha", "bsub-background", "bayer",
                            "camera-matrix", "distortion-coeffs", "kalman", "dt", "timeout", "sigma-accel", "sigma-noise", "homography", "target-sinks", "target-shape", "track-sinks", "track-gate", "crop-sinks", "crop-size", "crop-axis"},
                           {"tune", "bsub", "kalman", "target-shape", "crop-axis"});
        else o.apply_config({"diff-threshold", "blur", "area", "tune", "gpu-index", "bgr", "bayer", "camera-matrix", "distortion-coeffs",
                             "kalman", "dt", "timeout", "sigma-accel", "sigma-noise", "homography", "target-sinks", "target-shape", "track-sinks", "track-gate", "crop-sinks", "crop-size", "crop-axis"},
                            {"tune", "bgr", "kalman", "target-shape", "crop-axis"});
        if (o.has("bgr") && type != "diff") throw std::runtime_error("--bgr goes with TYPE diff only");
        if (type == "diff" && (o.has("bsub") || o.has("bsub-alpha") || o.has("bsub-background")))
            throw std::runtime_error("--bsub goes with TYPE hsv or thresh only");
        if (!o.has("bsub") && (o.has("bsub-alpha") || o.has("bsub-background")))
            throw std::runtime_error("--bsub-alpha and --bsub-background need --bsub");
        if (o.has("bsub-background") && o.num("bsub-alpha", 0, 0, 1) > 0)
            throw std::runtime_error("a background image from a file cannot adapt (--bsub-alpha must be 0)");
        // --bayer: the SOURCE's pixel format; it selects the BGR chain by itself, and is checked before any device is opened
        int bayer = 0;
        if (o.has("bayer")) {
            if (o.has("bgr")) throw std::runtime_error("--bayer and --bgr exclude each other: --bayer selects the BGR chain on a RAW8 source");
            if (type == "thresh") throw std::runtime_error("--bayer goes with TYPE diff, or with hsv --bsub: thresh is a GREY chain");
            if (type == "hsv" && !o.has("bsub")) throw std::runtime_error("--bayer with TYPE hsv needs --bsub");
            bayer = bayer_pattern(o.kv["bayer"]);
        }
        // --camera-matrix / --distortion-coeffs: framefilt undistort in front of a batched tracker's chain (Undistorter.cpp:57-81),
        // checked before any device is opened: distortion-coeffs first, then camera-matrix
        UndistortCalibration cal{};
        const bool undistort = o.has("camera-matrix") || o.has("distortion-coeffs");
        if (undistort) {
            if (bayer) throw std::runtime_error("--camera-matrix / --distortion-coeffs and --bayer exclude each other: a RAW8 source cannot be undistorted in the detector's kernel");
            if (type != "diff" && !o.has("bsub"))
                throw std::runtime_error("--camera-matrix / --distortion-coeffs with TYPE hsv or thresh need --bsub");
            cal = read_undistort_calibration(o);
        }
        // --kalman / --homography / --region (or the [[KEY.region]] tables of the -c file): the filter chain behind a batched tracker,
        // checked before any device is opened
        std::vector<RegionDef> regions;
        if (o.all.count("region")) for (const std::string &r : o.all["region"]) regions.push_back(parse_region(r));
        else if (!o.config_file.empty()) regions = read_region_tables(o.config_file, o.config_key);
        double homography[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const bool filters = o.has("kalman") || o.has("homography") || !regions.empty();
        for (const char *k : {"dt", "timeout", "sigma-accel", "sigma-noise"})
            if (o.has(k) && !o.has("kalman")) throw std::runtime_error(std::string("--") + k + " is a parameter of --kalman");
        if (filters) {
            if (type != "diff" && !o.has("bsub"))
                throw std::runtime_error("--kalman / --homography / --region with TYPE " + type + " need --bsub: the filter chain runs behind "
                                         "the batched trackers (diff, hsv --bsub, thresh --bsub), not behind the single-stage detector");
            if (regions.size() > 16) throw std::runtime_error("--region: " + std::to_string(regions.size()) + " regions, at most 16");
            if (o.has("kalman") && !(o.num("dt", 0.02, 0, 1e9) > 0)) throw std::runtime_error("--kalman: --dt must be > 0");
        }
        const bool homography_on = o.arr9("homography", homography);
        // --target-sinks: the K ranked blobs of every frame, checked before any device is opened
        std::vector<std::string> target_sinks;
        if (o.has("target-sinks")) {
            if (o.has("marker")) throw std::runtime_error("--target-sinks does not go with --marker");
            const std::vector<std::string> lists = o.all.count("target-sinks") ? o.all["target-sinks"] : target_sink_lists_of_config(o.kv["target-sinks"]);
            target_sinks = check_target_sinks(lists, {o.positional[2]}, false)[0];
        }
        check_target_shape(o.has("target-shape"), !target_sinks.empty());
        // --track-sinks: the K track slots of every frame, checked before any device is opened
        std::vector<std::string> track_sinks;
        if (o.has("track-gate") && !o.has("track-sinks")) throw std::runtime_error("--track-gate is a parameter of --track-sinks");
        if (o.has("track-sinks")) {
            if (o.has("marker")) throw std::runtime_error("--track-sinks does not go with --marker");
            if (type != "diff" && !o.has("bsub"))
                throw std::runtime_error("--track-sinks with TYPE " + type + " needs --bsub: tracks run behind the batched trackers (diff, hsv "
                                         "--bsub, thresh --bsub), not behind the single-stage detector");
            if (!o.has("kalman")) throw std::runtime_error("--track-sinks needs --kalman: every track slot runs a Kalman filter");
            const std::vector<std::string> lists = o.all.count("track-sinks") ? o.all["track-sinks"] : target_sink_lists_of_config(o.kv["track-sinks"]);
            track_sinks = check_target_sinks(lists, {o.positional[2]}, false, "--track-sinks", target_sinks)[0];
            if (!target_sinks.empty() && target_sinks.size() != track_sinks.size())
                throw std::runtime_error("--track-sinks names " + std::to_string(track_sinks.size()) + " sinks, --target-sinks " +
                                         std::to_string(target_sinks.size()) + ": K is one number");
        }
        // --crop-sinks: the ranks' (the track slots') windows of every frame, checked before any device is opened
        std::vector<std::string> crop_sinks;
        int crop_h = 0, crop_w = 0;
        if ((o.has("crop-size") || o.has("crop-axis")) && !o.has("crop-sinks"))
            throw std::runtime_error("--crop-size and --crop-axis are parameters of --crop-sinks");
        if (o.has("crop-sinks")) {
            if (type != "diff" && !o.has("bsub"))
                throw std::runtime_error("--crop-sinks with TYPE " + type + " needs --bsub: crops are cut behind the batched trackers (diff, hsv "
                                         "--bsub, thresh --bsub), not behind the single-stage detector");
            if (bayer || undistort)
                throw std::runtime_error("--crop-sinks does not go with --bayer or --camera-matrix / --distortion-coeffs: crops are cut from "
                                         "the frame as the SOURCE serves it");
            if (target_sinks.empty() && track_sinks.empty())
                throw std::runtime_error("--crop-sinks needs --target-sinks or --track-sinks: a window is cut around a ranked blob");
            const std::vector<std::string> lists = o.all.count("crop-sinks") ? o.all["crop-sinks"] : target_sink_lists_of_config(o.kv["crop-sinks"]);
            std::vector<std::string> taken = target_sinks;
            taken.insert(taken.end(), track_sinks.begin(), track_sinks.end());
            crop_sinks = check_target_sinks(lists, {o.positional[2]}, false, "--crop-sinks", taken)[0];
            const size_t k = std::max(target_sinks.size(), track_sinks.size());
            if (crop_sinks.size() > k)
                throw std::runtime_error("--crop-sinks names " + std::to_string(crop_sinks.size()) + " sinks for " + std::to_string(k) +
                                         " ranked blobs: at most K");
            if (o.has("crop-axis") && !o.has("target-shape"))
                throw std::runtime_error("--crop-axis needs --target-shape: the window is turned to the body axis of the blob's shape");
            if (!o.has("crop-size")) throw std::runtime_error("--crop-sinks needs --crop-size HxW");
            std::string size = o.kv.at("crop-size");
            size.erase(std::remove_if(size.begin(), size.end(), [](char ch) { return ch == '"' || ch == '\''; }), size.end());
            char x = 0, rest = 0;
            if (sscanf(size.c_str(), "%d%c%d%c", &crop_h, &x, &crop_w, &rest) != 3 || (x != 'x' && x != 'X'))
                throw std::runtime_error("--crop-size: expected HxW, got '" + size + "'");
            if (crop_h < 1 || crop_h > OATGPU_CROP_MAX_SIDE || crop_w < 4 || crop_w > OATGPU_CROP_MAX_SIDE || crop_w % 4 != 0)
                throw std::runtime_error("--crop-size: a window is 1..256 rows by 4..256 columns, the columns a multiple of 4 (got '" + size + "')");
        }
        if (o.has("tune")) throw std::runtime_error("--tune needs a GUI and is not available in the hip detector");
        auto d = std::make_unique<GpuDetector>(o.positional[1], o.positional[2],
                                               type == "hsv" ? Kind::HSV : type == "thresh" ? Kind::THRESH : Kind::DIFF,
                                               o.has("bgr") || (bayer && type == "diff"), o.has("bsub"), bayer,
                                               undistort ? &cal : nullptr, filters || !track_sinks.empty() || !crop_sinks.empty());
        d->kalman_ = o.has("kalman");
        d->dt_ = o.num("dt", 0.02, 0, 1e9);                         // KalmanFilter2D.cpp:69-85 (lower bound 0)
        d->timeout_ = o.num("timeout", 0.0, 0, 1e18);
        d->sig_accel_ = o.num("sigma-accel", 5.0, 0, 1e18);
        d->sig_noise_ = o.num("sigma-noise", 0.0, 0, 1e18);
        d->homography_on_ = homography_on;
        std::copy(homography, homography + 9, d->homography_);
        d->regions_ = regions;
        d->target_sink_addresses_ = target_sinks;
        d->target_shape_ = o.has("target-shape");
        d->track_sink_addresses_ = track_sinks;
        d->crop_sink_addresses_ = crop_sinks;
        d->crop_h_ = crop_h; d->crop_w_ = crop_w;
        d->crop_axis_ = o.has("crop-axis");
        if (o.has("track-gate")) {
            char *end = nullptr;
            const std::string g = o.kv.at("track-gate");
            const double v = strtod(g.c_str(), &end);
            if (end == g.c_str() || *end || !(v >= 0)) throw std::runtime_error("--track-gate: expected pixels >= 0 (or inf), got '" + g + "'");
            d->track_gate_ = v;
        }
        d->bsub_alpha_ = o.num("bsub-alpha", 0, 0, 1);
        if (o.has("bsub-background")) d->bsub_background_ = o.kv.at("bsub-background");
        d->cfg_.device = (int)o.num("gpu-index", 0, 0, 64);
        double a, b;
        auto range = [](double x, double y, const char *what) {
            if (x < 0 || x > 256 || y < 0 || y > 256) throw std::runtime_error(std::string("Values of ") + what + " should be between 0 and 256.");
        };
        if (type == "hsv") {
            if (o.arr2("h-thresh", a, b)) { range(a, b, "h-thresh"); d->cfg_.h_lo = (int)a; d->cfg_.h_hi = (int)b; }
            if (o.arr2("s-thresh", a, b)) { range(a, b, "s-thresh"); d->cfg_.s_lo = (int)a; d->cfg_.s_hi = (int)b; }
            if (o.arr2("v-thresh", a, b)) { range(a, b, "v-thresh"); d->cfg_.v_lo = (int)a; d->cfg_.v_hi = (int)b; }
        } else if (o.arr2("thresh", a, b)) { range(a, b, "thresh"); d->cfg_.h_lo = (int)a; d->cfg_.h_hi = (int)b; }
        if (o.has("diff-threshold")) d->cfg_.diff_threshold = (int)o.num("diff-threshold", 10, 0, 1e6);
        if (o.has("blur")) d->cfg_.blur = (int)o.num("blur", 2, 0, 1e6);
        if (o.has("erode")) d->cfg_.erode = (int)o.num("erode", 0, 0, 1e6);
        if (o.has("dilate")) d->cfg_.dilate = (int)o.num("dilate", 0, 0, 1e6);
        if (o.arr2("area", a, b)) {
            if (a >= b) throw std::runtime_error("Max area should be larger than min area.");   // HSVDetector.cpp:135
            d->cfg_.min_area = a; d->cfg_.max_area = b;
        }
        return d->run();
    } catch (const std::exception &e) {
        std::cerr << "oat-posidet-hip: " << e.what() << std::endl;
        return -1;
    }
}
