// oat-track-hip SOURCE[,SOURCE...] SINK[,SINK...] [CONFIGURATION]
//
// The whole chain  framefilt mog -> framefilt col -C HSV -> posidet hsv  (optionally -> posifilt kalman)
// for N camera streams in ONE process, ONE device context and ONE fused launch per stage and step:
// N BGR oat::Frame SOURCEs in, N oat::Position2D SINKs out -- SOURCE i feeds SINK i, one token out per
// token in, in order, carrying its frame's Sample (PositionDetector.cpp:80).  N = 1 is the drop-in for a
// single pipeline; N > 1 is the reference's multi-camera shape (examples/two-gige/two-gige.sh:7-8: one
// component instance per camera) batched into one launch, which is what BASELINE configs 3 and 4 ask for.
//
// The loop is the reference's (FrameFilter.cpp:59-98, PositionDetector.cpp:58-99) with its three phases
// pipelined through the library's result ring instead of run back to back:
//
//   wait on every SOURCE                              PositionDetector.cpp:63-75
//   oatgpu_track_enqueue(frames in shared memory)     the H2D copies read the (page-locked) shm frames
//   oatgpu_track_input_consumed_stream(i), post SOURCE i   the reference posts right after its memcpy (:78-86);
//                                                     here, camera by camera, right after the DMA out of its segment
//   collect + publish finished results                :88-96, SINK i: wait, *shared = position, post
//
// A result is published as soon as it is ready whenever the camera the loop is waiting for has no frame yet (minimum
// latency, camera-bound pipelines); with frames waiting the loop goes on staging and finished results leave SINK by
// SINK between the copies (the link never idles for a consumer's hand-shake), at the latest when the ring is full.  Options are the union of the three stock components'
// (-a is mog's adaptation coefficient; the detector's area is --area).
//
// --gpu-index D0,D1,...  shards the cameras over several devices from THIS process (BASELINE configs 3/4 at the
// drop-in boundary: 64 x 1080p as 8 per GPU, 8 x 4K as one per GPU): the SOURCE list is cut into
// contiguous blocks -- camera s goes to shard s / ceil(S/N), as oat_amd/dist.py partitions streams over ranks --
// and every shard is a batched tracker of its own (own device context, own thread, own loop): streams are
// independent, so nothing crosses between shards.  The same device may be named twice (two contexts on one GPU).
//
// --ingest-root D0 (with --gpu-index D0,D1,...): every camera's frame is ingested on device D0 and travels to the device that
// owns its stream over RCCL send/recv (scatter_tracker.hpp; north_star's "RCCL over xGMI only for the trivial stream-to-rank
// scatter") -- one process, one thread, the same partition.  Without it every shard ingests its own cameras (the realistic
// camera topology).
//
// --camera-matrix / --distortion-coeffs (one calibration for every camera) or --undistort-key T0[,T1,...] (tables of the -c
// file, one for every camera or one per camera) put `framefilt undistort` in front of the chain, inside the same context
// (oatgpu_set_track_undistort): undistort -> mask -> mog -> col -> detector, the ROI mask on the undistorted image.
//
// --thresh [lo,hi] selects the GREY chain instead:  framefilt mog -> posidet thresh  on SOURCEs that carry GREY
// frames (a mono camera or `framefilt col -C GREY`; SimpleThreshold.cpp:46 requires them), the one-channel model
// and the intensity window of SimpleThreshold.cpp:171-174 in the same fused launches.
#include "component.hpp"
#include "filter_chain.hpp"
#include "target_sinks.hpp"
#include "scatter_tracker.hpp"
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <fstream>
#include <sched.h>
#include <sstream>
#include <thread>
#include <unistd.h>

using namespace oat;

static std::vector<std::string> split_list(const std::string &s)
{
    std::vector<std::string> out;
    size_t a = 0;
    while (a <= s.size()) {
        const size_t b = s.find(',', a);
        const std::string t = s.substr(a, b == std::string::npos ? std::string::npos : b - a);
        if (t.empty()) throw std::runtime_error("empty address in list '" + s + "'");
        out.push_back(t);
        if (b == std::string::npos) break;
        a = b + 1;
    }
    return out;
}

// Keep the calling thread on the CPUs of the NUMA node device `dev` hangs off (oatgpu_device_numa_node): its launch calls,
// its reads of the shared-memory frames and the staging copies stay on that socket.  Best effort; false if nothing was done.
static bool pin_thread_to_device_node(int dev)
{
    const int node = oatgpu_device_numa_node(dev);
    if (node < 0) return false;
    std::ifstream f("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
    std::string list;
    if (!f || !std::getline(f, list)) return false;
    cpu_set_t set;
    CPU_ZERO(&set);
    size_t a = 0;
    int n = 0;
    while (a < list.size()) {
        size_t b = list.find(',', a);
        if (b == std::string::npos) b = list.size();
        const std::string part = list.substr(a, b - a);
        const size_t dash = part.find('-');
        const int lo = atoi(part.c_str()), hi = dash == std::string::npos ? lo : atoi(part.c_str() + dash + 1);
        for (int c = lo; c <= hi && c < CPU_SETSIZE; ++c) { CPU_SET(c, &set); ++n; }
        a = b + 1;
    }
    return n > 0 && sched_setaffinity(0, sizeof set, &set) == 0;
}

// ---- marker sets: one `posidet hsv` per colour and `posicom mean` behind them, in ONE tracker (oatgpu_set_markers) ----
// --marker "H=[lo,hi] S=[lo,hi] V=[lo,hi] e=K d=K area=[a,b]": every item optional, HSVDetector's defaults otherwise
// (HSVDetector.h:77-94: all-pass window, erode off, dilate 10, area [0, DBL_MAX)).
static oatgpu_marker default_marker()
{
    oatgpu_config c;
    oatgpu_default_config(&c);
    oatgpu_marker m{};
    m.h_lo = c.h_lo; m.h_hi = c.h_hi; m.s_lo = c.s_lo; m.s_hi = c.s_hi; m.v_lo = c.v_lo; m.v_hi = c.v_hi;
    m.erode = c.erode; m.dilate = c.dilate; m.min_area = c.min_area; m.max_area = c.max_area;
    return m;
}
static void marker_item(oatgpu_marker &m, const std::string &key, const std::string &val, const std::string &where)
{
    double a = 0, b = 0;
    char tail = 0;
    const bool pair = sscanf(val.c_str(), " [ %lf , %lf %c", &a, &b, &tail) == 3 && tail == ']';
    char *end = nullptr;
    const double v = strtod(val.c_str(), &end);
    const bool scalar = end != val.c_str() && *end == 0;
    auto need = [&](bool ok, const char *what) {
        if (!ok) throw std::runtime_error(where + ": '" + key + "' must be " + what + ", got '" + val + "'");
    };
    if (key == "H" || key == "h-thresh") { need(pair, "a 2-element array, e.g. [0,256]"); m.h_lo = (int)a; m.h_hi = (int)b; }
    else if (key == "S" || key == "s-thresh") { need(pair, "a 2-element array, e.g. [0,256]"); m.s_lo = (int)a; m.s_hi = (int)b; }
    else if (key == "V" || key == "v-thresh") { need(pair, "a 2-element array, e.g. [0,256]"); m.v_lo = (int)a; m.v_hi = (int)b; }
    else if (key == "area") { need(pair, "a 2-element array [min,max]"); m.min_area = a; m.max_area = b; }
    else if (key == "e" || key == "erode") { need(scalar && v >= 0 && v <= 1e6, "a number >= 0"); m.erode = (int)v; }
    else if (key == "d" || key == "dilate") { need(scalar && v >= 0 && v <= 1e6, "a number >= 0"); m.dilate = (int)v; }
    else throw std::runtime_error(where + ": unknown item '" + key + "' (H, S, V, e, d, area)");
}
static oatgpu_marker parse_marker(const std::string &text)
{
    oatgpu_marker m = default_marker();
    std::istringstream in(text);
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos || eq == 0) throw std::runtime_error("--marker: expected KEY=VALUE items, got '" + tok + "'");
        marker_item(m, tok.substr(0, eq), tok.substr(eq + 1), "--marker");
    }
    return m;
}
// The TOML form: every [[KEY.marker]] table of the -c file is one marker, in file order, with posidet hsv's option names
// (h-thresh, s-thresh, v-thresh, erode, dilate, area).
static std::vector<oatgpu_marker> read_marker_tables(const std::string &file, const std::string &key)
{
    std::vector<oatgpu_marker> out;
    std::ifstream in(file);
    if (!in) return out;
    auto trim = [](std::string t) {
        const size_t a = t.find_first_not_of(" \t\r\n"), b = t.find_last_not_of(" \t\r\n");
        return a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
    };
    const std::string header = "[[" + key + ".marker]]", where = "[[" + key + ".marker]]";
    std::string line;
    bool inside = false;
    while (std::getline(in, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        line = trim(line);
        if (line.empty()) continue;
        if (line.front() == '[' && line.find('=') == std::string::npos) {
            std::string h;
            for (char ch : line) if (ch != ' ' && ch != '\t') h += ch;
            inside = h == header;
            if (inside) out.push_back(default_marker());
            continue;
        }
        if (!inside) continue;
        const size_t eq = line.find('=');
        if (eq == std::string::npos) throw std::runtime_error(where + ": expected key = value");
        std::string val;
        for (char ch : trim(line.substr(eq + 1))) if (ch != ' ' && ch != '\t') val += ch;
        marker_item(out.back(), trim(line.substr(0, eq)), val, where);
    }
    return out;
}

// ---- the filter chain behind the combined record (oatgpu_set_marker_filters): --mean-kalman, --mean-homography, --region ----
// (--region and the [[KEY.region]] tables: parse_region, check_region, read_region_tables of filter_chain.hpp)

class BatchedTracker : public Component {
public:
    // stream_base / n_total: where this shard's cameras sit in the command line's SOURCE list (model file names)
    BatchedTracker(const std::vector<std::string> &sources, const std::vector<std::string> &sinks, int stream_base = 0,
                   int n_total = -1)
        : source_addresses_(sources), sink_addresses_(sinks), n_((int)sources.size()), stream_base_(stream_base),
          n_total_(n_total < 0 ? (int)sources.size() : n_total)
    {
        if (sources.size() != sinks.size()) throw std::runtime_error("need as many SINKs as SOURCEs");
        oatgpu_default_config(&cfg_);
        name_ = "track[" + sources[0] + (n_ > 1 ? ",..(" + std::to_string(n_) + ")" : "") + "->" + sinks[0] + (n_ > 1 ? ",.." : "") + "]";
        frame_sources_ = std::vector<Source<Frame>>(n_);
        position_sinks_ = std::vector<Sink<Position2D>>(n_);
        src_pins_ = std::vector<ShmRegistration>(n_);
    }
    std::string name() const override { return name_; }
    // marker mode: the context's own window becomes the non-zero window (its threshold plane is then "the masked frame's
    // pixel is non-zero", what every marker's mask is made from); sinks[s][m] = address of camera s' marker m
    void set_markers(const std::vector<oatgpu_marker> &markers, int heading_anchor, const std::vector<std::vector<std::string>> &sinks)
    {
        markers_ = markers;
        heading_anchor_ = heading_anchor;
        marker_sink_addresses_ = sinks;
        marker_sinks_ = std::vector<Sink<Position2D>>((size_t)n_ * markers.size());
        cfg_.h_lo = 0; cfg_.h_hi = 256; cfg_.s_lo = 0; cfg_.s_hi = 256; cfg_.v_lo = 1; cfg_.v_hi = 256;
    }
    // --target-sinks: multi-target detection (oatgpu_set_targets); sinks[s][j] = address of rank j of camera s
    // shape: --target-shape, rank j's token carries the blob's body axis as its heading (oatgpu_set_target_shapes)
    void set_targets(const std::vector<std::vector<std::string>> &sinks, bool shape = false)
    {
        target_shape_ = shape;
        target_sink_addresses_ = sinks;
        targets_k_ = sinks.empty() ? 0 : (int)sinks[0].size();
        target_sinks_ = std::vector<Sink<Position2D>>((size_t)n_ * targets_k_);
    }
    oatgpu_config cfg_;
    double learning_coeff_{0.0};
    bool kalman_{false};            // --kalman: `posifilt kalman` fused behind the detector
    double dt_{0.02}, timeout_{0.0}, sig_accel_{5.0}, sig_noise_{0.0};   // KalmanFilter2D.h:56-60
    std::string model_file_;        // --model-file: resume the MOG2 model(s) from / checkpoint to this file
    std::string mask_file_;         // --mask: `framefilt mask` fused in front of mog (FrameMasker.cpp:45-75)
    bool grey_{false};              // --thresh: GREY frames, mog -> posidet thresh
    int stage_copy_{0};             // --stage-copy kernel: oatgpu_set_stage_copy(1)
    bool timing_{false};            // --timing: where the loop's wall clock goes, printed at exit (stderr)
    bool homography_on_{false};     // --homography: `posifilt homography` behind the detector / the position filter
    double homography_[9]{1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<UndistortCalibration> undistort_;   // one per camera of this shard: `framefilt undistort` fused in front (empty: off)
    std::vector<int32_t> bayer_;    // --bayer: one OATGPU_BAYER_* per camera of this shard; the SOURCEs carry RAW8 (GREY-tagged) frames
    // marker sets (--marker, repeatable): M `posidet hsv` detectors per camera behind the one model pass and `posicom mean`
    // behind them; marker m of camera s is published on marker_sink_addresses_[s][m], the combined position on SINK s
    std::vector<oatgpu_marker> markers_;
    int heading_anchor_{-1};        // --heading-anchor (`posicom mean`), -1: no heading
    int marker_ring_{0};            // --marker-ring D: marker mode through the staged loop and a result ring of D (0: the synchronous step)
    std::vector<std::vector<std::string>> marker_sink_addresses_;
    std::vector<std::vector<std::string>> target_sink_addresses_;
    int targets_k_{0};              // K of --target-sinks (0: off)
    bool target_shape_{false};      // --target-shape
    // the filter chain behind the combined record (--mean-kalman / --mean-homography / --region): the camera's SINK then carries
    // the FILTERED Position2D; Kalman parameters are dt_ .. sig_noise_ above
    bool mean_kalman_{false}, mean_homography_on_{false};
    double mean_homography_[9]{1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<RegionDef> regions_;
    bool chain_on() const { return mean_kalman_ || mean_homography_on_ || !regions_.empty(); }
    ~BatchedTracker() override
    {
        if (!model_file_.empty() && gpu_.ctx)
            for (int s = 0; s < n_; ++s)
                if (oatgpu_mog_save(gpu_.ctx, s, model_path(s).c_str()) != OATGPU_OK)
                    std::cerr << name() << ": " << oatgpu_last_error(gpu_.ctx) << std::endl;
    }

    // --timing: seconds spent waiting for SOURCEs, in oatgpu_track_stage, waiting for a camera's copy, posting SOURCEs,
    // registering the set, and collecting + publishing results; rounds counted
    double t_wait_{0}, t_stage_{0}, t_consumed_{0}, t_post_{0}, t_enqueue_{0}, t_publish_{0}, t_r16_{0}, t_last_{0};
    unsigned long long rounds_{0};
    void print_timing() const
    {
        if (!timing_ || !rounds_) return;
        const double r = 1e6 / (double)rounds_;
        // (the rate between the end of round 16 and the end of the last round: process start-up, the first frames' page
        // registration and the models' initialisation are the harness's, not the loop's)
        const double steady = rounds_ > 16 && t_last_ > t_r16_ ? (double)(rounds_ - 16) * n_ / (t_last_ - t_r16_) : 0.0;
        std::fprintf(stderr, "%s: %llu rounds x %d cameras; per round (us): source wait %.1f, stage calls %.1f, copy wait %.1f, "
                             "source post %.1f, enqueue %.1f, collect+publish %.1f; steady %.1f fps aggregate\n", name().c_str(),
                     rounds_, n_, t_wait_ * r, t_stage_ * r, t_consumed_ * r, t_post_ * r, t_enqueue_ * r, t_publish_ * r, steady);
    }

protected:
    static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    std::string model_path(int s) const { return n_total_ == 1 ? model_file_ : model_file_ + "." + std::to_string(stream_base_ + s); }

    // PositionDetector.cpp:40-56, for every stream
    bool connectToNode() override
    {
        // A tracker that fails while connecting (a camera with another geometry, no device memory, an unreadable mask
        // or model file) still BINDS its SINKs on the way out, so that its destructor sets them END (Sink.h:73-91) and
        // the consumers of this shard's cameras end instead of waiting for a sink that will never appear -- with
        // several shards in one process the others keep running, where the reference's one-camera process would
        // simply have exited (framefilter/main.cpp:278-295).
        try {
            return connect_all();
        } catch (...) {
            for (int s = 0; s < n_; ++s) {
                if ((size_t)s < shared_positions_.size()) continue;        // bound before the failure
                try { position_sinks_[s].bind(sink_addresses_[s], sink_addresses_[s]); } catch (...) {}
            }
            for (size_t i = marker_shared_.size(); i < marker_sinks_.size(); ++i) {
                const std::string &a = marker_sink_addresses_[i / markers_.size()][i % markers_.size()];
                try { marker_sinks_[i].bind(a, a); } catch (...) {}
            }
            for (size_t i = target_shared_.size(); i < target_sinks_.size(); ++i) {
                const std::string &a = target_sink_addresses_[i / targets_k_][i % targets_k_];
                try { target_sinks_[i].bind(a, a); } catch (...) {}
            }
            throw;
        }
    }

    bool connect_all()
    {
        for (int s = 0; s < n_; ++s) frame_sources_[s].touch(source_addresses_[s]);
        FrameParams p0{};
        for (int s = 0; s < n_; ++s) {
            if (frame_sources_[s].connect(grey_ || !bayer_.empty() ? PIX_GREY : PIX_BGR) != SourceState::CONNECTED) return false;
            const FrameParams p = frame_sources_[s].parameters();
            if (s == 0) p0 = p;
            else if (p.rows != p0.rows || p.cols != p0.cols)
                throw std::runtime_error("all SOURCEs of one batched tracker must have the same frame geometry");
        }
        cfg_.rows = (int)p0.rows; cfg_.cols = (int)p0.cols; cfg_.n_streams = n_;
        cfg_.channels = grey_ ? 1 : 3;
        if (cfg_.ring_depth < 2) cfg_.ring_depth = 2;
        gpu_.create(cfg_);
        if (!bayer_.empty()) gpu_.check(oatgpu_set_track_bayer(gpu_.ctx, bayer_.data(), n_));
        if (!undistort_.empty()) {
            for (int s = 0; s < n_; ++s)
                gpu_.check(oatgpu_set_undistort(gpu_.ctx, s, undistort_[s].K, undistort_[s].dist.data(), (int32_t)undistort_[s].dist.size()));
            gpu_.check(oatgpu_set_track_undistort(gpu_.ctx, 1));
        }
        if (!model_file_.empty())
            for (int s = 0; s < n_; ++s)
                if (access(model_path(s).c_str(), R_OK) == 0) gpu_.check(oatgpu_mog_load(gpu_.ctx, s, model_path(s).c_str()));
        if (!mask_file_.empty()) {
            const GreyImage m = read_pnm_grey(mask_file_);               // FrameMasker.cpp:45-62: imread(.., GRAYSCALE)
            if (m.rows != p0.rows || m.cols != p0.cols) throw std::runtime_error("Mask image and frame source image do not have equal sizes");   // FrameMasker.cpp:77-81
            for (int s = 0; s < n_; ++s) gpu_.check(oatgpu_set_roi_mask(gpu_.ctx, s, m.px.data()));
        }
        if (kalman_) gpu_.check(oatgpu_set_kalman(gpu_.ctx, 1, dt_, timeout_, sig_accel_, sig_noise_));
        if (stage_copy_) gpu_.check(oatgpu_set_stage_copy(gpu_.ctx, stage_copy_));
        if (homography_on_) gpu_.check(oatgpu_set_homography(gpu_.ctx, 1, homography_));
        for (int s = 0; s < n_; ++s) {
            position_sinks_[s].bind(sink_addresses_[s], sink_addresses_[s]);
            shared_positions_.push_back(position_sinks_[s].retrieve());
        }
        frame_ptrs_.resize(n_);
        results_.resize(n_);
        if (targets_k_) {
            gpu_.check(oatgpu_set_targets(gpu_.ctx, targets_k_));
            for (size_t i = 0; i < target_sinks_.size(); ++i) {
                const std::string &a = target_sink_addresses_[i / targets_k_][i % targets_k_];
                target_sinks_[i].bind(a, a);
                target_shared_.push_back(target_sinks_[i].retrieve());
            }
            target_results_.resize((size_t)n_ * targets_k_);
            target_found_.resize(n_);
            if (target_shape_) {
                gpu_.check(oatgpu_set_target_shapes(gpu_.ctx, 1));
                target_shapes_.resize((size_t)n_ * targets_k_);
            }
        }
        if (!markers_.empty()) {
            const int M = (int)markers_.size();
            gpu_.check(oatgpu_set_markers(gpu_.ctx, M, markers_.data(), heading_anchor_));
            for (size_t i = 0; i < marker_sinks_.size(); ++i) {
                const std::string &a = marker_sink_addresses_[i / M][i % M];
                marker_sinks_[i].bind(a, a);
                marker_shared_.push_back(marker_sinks_[i].retrieve());
            }
            marker_results_.resize((size_t)n_ * M);
            combined_.resize(n_);
            if (marker_ring_) gpu_.check(oatgpu_set_marker_pipeline(gpu_.ctx, 1));
            if (chain_on()) {
                std::vector<oatgpu_region> rs;
                oatgpu_marker_filters f = chain_filters(regions_, rs);
                f.kalman = mean_kalman_; f.dt = dt_; f.timeout = timeout_; f.sigma_accel = sig_accel_; f.sigma_noise = sig_noise_;
                f.homography = mean_homography_on_;
                std::copy(mean_homography_, mean_homography_ + 9, f.h);
                gpu_.check(oatgpu_set_marker_filters(gpu_.ctx, &f));
                filtered_.resize(n_);
            }
        }
        return true;
    }

    // Results leave set by set, SINK by SINK (PositionDetector.cpp:88-96 per camera): publish_some() hands out up to
    // max_sinks tokens of the oldest outstanding result set -- with only_if_ready it never waits for the device -- so that
    // the staging loop below can publish BETWEEN its copies: a SINK's wait() is a round trip to the consumer process
    // (~30 us each; 8 cameras: 275 us a round), and done behind the round it was time the PCIe link sat idle
    // (r04, `--timing`: 8 x 1080p 6.2 k -> see DESIGN.md section 6).  Order per SINK is the frames' order.
    void publish_sink(int s)
    {
        if (marker_ring_) return publish_markers(s, pub_samples_[s]);
        const oatgpu_position &r = results_[s];
        Position2D pos("");
        pos.set_sample(pub_samples_[s]);                             // PositionDetector.cpp:80
        pos.position_valid = r.valid != 0;
        if (kalman_) {                                               // KalmanFilter2D.cpp:123-137
            pos.position.x = r.x; pos.position.y = r.y;
            pos.velocity.x = r.vx; pos.velocity.y = r.vy;
            pos.velocity_valid = r.velocity_valid != 0;
        } else if (r.valid) {                                        // DetectorFunc.cpp:46,58-60: x/y only when found
            pos.position.x = r.x; pos.position.y = r.y;
        }
        if (homography_on_) pos.setCoordSystem(DistanceUnit::WORLD, homography_);   // HomographyTransform2D.cpp:102
        position_sinks_[s].wait();
        *shared_positions_[s] = pos;
        position_sinks_[s].post();
        for (int j = 0; j < targets_k_; ++j)                         // rank j of camera s, raw, with the frame's Sample
            put(target_sinks_[(size_t)s * targets_k_ + j], target_shared_[(size_t)s * targets_k_ + j],
                target_position(target_results_[(size_t)s * targets_k_ + j], pub_samples_[s],
                                target_shape_ ? &target_shapes_[(size_t)s * targets_k_ + j] : nullptr));
    }
    void publish_some(int max_sinks, bool only_if_ready)
    {
        if (!collected_) {
            if (pending_.empty()) return;
            if (only_if_ready && oatgpu_track_ready(gpu_.ctx) != 1) return;
            if (marker_ring_)
            {
                gpu_.check(oatgpu_track_collect_markers(gpu_.ctx, results_.data(), marker_results_.data(), combined_.data()));
                fetch_filtered();
            }
            else
                gpu_.check(oatgpu_track_collect(gpu_.ctx, results_.data()));
            if (targets_k_ && oatgpu_targets(gpu_.ctx, target_results_.data(), target_found_.data(), 1) != 1)    // the set just collected
                gpu_.check(OATGPU_E_INVALID);
            if (target_shape_ && oatgpu_target_shapes(gpu_.ctx, target_shapes_.data(), 1) != 1) gpu_.check(OATGPU_E_INVALID);
            pub_samples_ = std::move(pending_.front());
            pending_.pop_front();
            collected_ = true;
            pub_cursor_ = 0;
        }
        for (; pub_cursor_ < n_ && max_sinks > 0; ++pub_cursor_, --max_sinks) publish_sink(pub_cursor_);
        if (pub_cursor_ == n_) collected_ = false;
    }
    // the set in progress to its end, or else the whole next set (waits for the device if it must)
    void publish() { publish_some(n_, false); }
    bool results_owed() const { return collected_ || !pending_.empty(); }

    // Marker mode.  Without --marker-ring: the synchronous marker step once per round of frames (oatgpu_track_markers).  Every
    // camera's frame is waited for, the step runs, the SOURCEs are posted, then every marker's Position2D leaves on its sink
    // and the combined one (`posicom mean`: position, heading) on the camera's ordinary SINK.  With --marker-ring D the
    // ordinary staged loop below runs (oatgpu_set_marker_pipeline): the cameras are staged one by one, results leave up to
    // D - 1 rounds behind through oatgpu_track_collect_markers, camera by camera as publish_markers writes them.
    static void put(Sink<Position2D> &sink, Position2D *shared, const Position2D &pos)
    {
        sink.wait();
        *shared = pos;
        sink.post();
    }
    // the filtered records of the frame set the marker call before this has just delivered
    void fetch_filtered()
    {
        if (!chain_on()) return;
        const int got = oatgpu_marker_filtered(gpu_.ctx, filtered_.data(), 1);
        if (got != 1) gpu_.check(got < 0 ? got : OATGPU_E_INVALID);
    }
    int process_markers()
    {
        std::vector<Sample> samples(n_);
        for (int s = 0; s < n_; ++s) {
            if (frame_sources_[s].wait() == NodeState::END) {
                for (int q = 0; q < s; ++q) frame_sources_[q].post();      // the round is dropped: nothing is owed for it
                return 1;
            }
            const Frame &shm = *frame_sources_[s].retrieve();
            src_pins_[s].pin(shm);
            samples[s] = shm.sample();
            frame_ptrs_[s] = shm.data();
        }
        gpu_.check(oatgpu_track_markers(gpu_.ctx, frame_ptrs_.data(), n_, learning_coeff_, results_.data(), marker_results_.data(),
                                        combined_.data()));
        fetch_filtered();
        for (int s = 0; s < n_; ++s) frame_sources_[s].post();
        for (int s = 0; s < n_; ++s) publish_markers(s, samples[s]);
        ++rounds_;
        return 0;
    }
    // camera s of the marker results in hand: every marker's Position2D on its sink, the combined one on the camera's SINK
    void publish_markers(int s, const Sample &sample)
    {
        const int M = (int)markers_.size();
        for (int m = 0; m < M; ++m) {                                   // `posidet hsv` number m of camera s
            const oatgpu_position &r = marker_results_[(size_t)s * M + m];
            Position2D pos("");
            pos.set_sample(sample);
            pos.position_valid = r.valid != 0;
            if (r.valid) { pos.position.x = r.x; pos.position.y = r.y; }   // DetectorFunc.cpp:46,58-60
            put(marker_sinks_[(size_t)s * M + m], marker_shared_[(size_t)s * M + m], pos);
        }
        const oatgpu_combined &c = combined_[s];                        // MeanPosition.cpp:60-118
        Position2D pos("");
        pos.set_sample(sample);
        pos.position_valid = c.position_valid != 0;
        pos.position.x = c.x; pos.position.y = c.y;
        pos.heading_valid = c.heading_valid != 0;
        pos.heading.x = c.hx; pos.heading.y = c.hy;
        if (chain_on()) {                                               // ... behind posifilt kalman / homography / region
            publish_filtered(pos, filtered_[s], regions_, mean_homography_on_ ? mean_homography_ : nullptr);
        }
        put(position_sinks_[s], shared_positions_[s], pos);
    }

    int process() override
    {
        if (!markers_.empty() && !marker_ring_) return process_markers();
        // ---- a frame from every camera (PositionDetector.cpp:63-75), camera by camera: as soon as camera s has delivered,
        // its H2D copy starts (oatgpu_track_stage), and camera s - 1, whose copy has meanwhile left its segment, is
        // posted (PositionDetector.cpp:78-86 per camera) -- the n frames cross one PCIe link one after the other, and
        // the upstream writers refill their segments while the later cameras are still being waited for and copied
        // (8 x 1080p: a round is the link's time, not the slowest writer's memcpy + the link's time) ----
        std::vector<Sample> samples(n_);
        double t0 = timing_ ? now_s() : 0.0, t1;
#define OAT_LAP(acc) do { if (timing_) { t1 = now_s(); acc += t1 - t0; t0 = t1; } } while (0)
        for (int s = 0; s < n_; ++s) {
            // Nothing to stage yet (this camera has not delivered): results that are owed leave NOW -- the reference publishes
            // a position as soon as it has one (PositionDetector.cpp:88-96); a frame that was only registered for a
            // two-frame launch goes out alone (oatgpu_track_collect), which is right when the cameras are slower than
            // the device.  With a frame waiting the loop goes on staging and the results leave between the copies.
            while (!quit && results_owed() && !frame_sources_[s].token_waiting()) publish_some(1, collected_);
            OAT_LAP(t_publish_);
            const NodeState st = frame_sources_[s].wait();
            OAT_LAP(t_wait_);
            if (st == NodeState::END) {
                // (frames of this round already staged are dropped with the round: their sources get their post, the
                // set is never registered; frames of earlier rounds still get their tokens)
                for (int q = (s > 0 ? s - 1 : 0); q < s; ++q) {
                    gpu_.check(oatgpu_track_input_consumed_stream(gpu_.ctx, q));
                    frame_sources_[q].post();
                }
                gpu_.check(oatgpu_track_stage_abort(gpu_.ctx));        // the partly staged set is given up, nothing is owed for it
                while (results_owed() && !quit) publish();
                print_timing();
                return 1;
            }
            const Frame &shm = *frame_sources_[s].retrieve();
            src_pins_[s].pin(shm);
            samples[s] = shm.sample();
            gpu_.check(oatgpu_track_stage(gpu_.ctx, s, shm.data()));
            OAT_LAP(t_stage_);
            // while this camera's copy runs: one token of a FINISHED result set to its SINK (never the newest set: asking for
            // a frame that is only registered would launch it alone and end the two-frames-a-launch pairing)
            if (collected_ || pending_.size() >= 2) { publish_some(1, true); OAT_LAP(t_publish_); }
            if (s > 0) {
                gpu_.check(oatgpu_track_input_consumed_stream(gpu_.ctx, s - 1));
                OAT_LAP(t_consumed_);
                frame_sources_[s - 1].post();
                OAT_LAP(t_post_);
            }
        }
        gpu_.check(oatgpu_track_input_consumed_stream(gpu_.ctx, n_ - 1));
        OAT_LAP(t_consumed_);
        frame_sources_[n_ - 1].post();
        OAT_LAP(t_post_);
        gpu_.check(oatgpu_track_enqueue_staged(gpu_.ctx, learning_coeff_));
        OAT_LAP(t_enqueue_);
        pending_.push_back(std::move(samples));
        ++rounds_;
        if (timing_) { t_last_ = now_s(); if (rounds_ == 16) t_r16_ = t_last_; }

        // ---- a free ring slot for the next round; everything else leaves while the loop waits for a camera (top of the
        // loop: at once when no frame is waiting -- minimum latency) or between the next round's copies (frames waiting) ----
        while ((int)pending_.size() == cfg_.ring_depth && !quit) publish();
        OAT_LAP(t_publish_);
#undef OAT_LAP
        return 0;
    }

    std::string name_;
    std::vector<std::string> source_addresses_, sink_addresses_;
    int n_, stream_base_, n_total_;
    std::vector<Source<Frame>> frame_sources_;
    std::vector<Sink<Position2D>> position_sinks_;
    std::vector<Position2D *> shared_positions_;
    std::vector<ShmRegistration> src_pins_;    // declared after the sources: unregistered before the segments are unmapped
    std::vector<const uint8_t *> frame_ptrs_;
    std::vector<oatgpu_position> results_;
    std::vector<Sink<Position2D>> marker_sinks_;       // [n][M]
    std::vector<Position2D *> marker_shared_;
    std::vector<oatgpu_position> marker_results_;      // [n][M]
    std::vector<oatgpu_combined> combined_;            // [n]
    std::vector<oatgpu_filtered> filtered_;            // [n] the combined records behind the filter chain
    std::vector<Sink<Position2D>> target_sinks_;       // [n][K]
    std::vector<Position2D *> target_shared_;
    std::vector<oatgpu_position> target_results_;      // [n][K] of the result set that is being handed out
    std::vector<int32_t> target_found_;                // [n]
    std::vector<oatgpu_shape> target_shapes_;          // [n][K] beside target_results_ with --target-shape
    std::deque<std::vector<Sample>> pending_;  // Samples of the frames whose results are still on the device
    std::vector<Sample> pub_samples_;          // ... and of the result set that is being handed out (publish_some)
    bool collected_{false};
    int pub_cursor_{0};
    GpuCtx gpu_;
};

int main(int argc, char **argv)
{
    try {
        Options o = Options::parse(argc, argv,
            {{"a", "adaptation-coeff"}, {"H", "h-thresh"}, {"S", "s-thresh"}, {"V", "v-thresh"}, {"e", "erode"},
             {"d", "dilate"}, {"T", "timeout"}, {"n", "sigma-noise"}, {"f", "mask"}, {"h", "help"}, {"v", "version"}},
            {"help", "version", "kalman", "timing", "print-partition", "mean-kalman", "target-shape"});
        if (o.has("version")) { std::cout << "oat-track-hip (MI355X drop-in, liboatgpu ABI " << oatgpu_abi_version() << ")\n"; return 0; }
        if (o.has("help") || o.positional.size() != 2) {
            std::cout << "Usage: oat-track-hip SOURCE[,SOURCE..] SINK[,SINK..] [-a coeff] [-H [lo,hi]] [-S ..] [-V ..] [-e n] [-d n] [--area [min,max]]\n"
                         "       [--gpu-index N | N0,N1,..] [--ring D] [--model-file FILE] [-f|--mask FILE.pgm] [--stage-copy dma|kernel]\n"
                         "       [--thresh [lo,hi]]   GREY SOURCEs: framefilt mog -> posidet thresh instead of the HSV chain\n"
                         "       [--bayer P | P0,P1,..]  the SOURCEs carry Bayer RAW8 frames (GREY-tagged, as `oat-frameserve-raw -C GREY` serves): they\n"
                         "                            are demosaiced on the device in front of the chain; P = RGGB | BGGR | GRBG | GBRG, the 2 x 2 tile\n"
                         "                            at image rows 0-1, columns 0-1 -- one for all cameras or one per SOURCE.  Not with --thresh.\n"
                         "       [--homography [h11,h12,...,h33]]   posifilt homography fused in (positions in world units)\n"
                         "       [--kalman [--dt s] [-T|--timeout s] [--sigma-accel a] [-n|--sigma-noise n]]   (posifilt kalman fused in)\n"
                         "       [--camera-matrix [K11,...,K33] --distortion-coeffs [k1,k2,p1,p2,k3(,k4,k5,k6)] | --undistort-key T0[,T1,..]]\n"
                         "                            framefilt undistort fused in front of the chain (the mask applies to the undistorted image):\n"
                         "                            one calibration for every camera, or tables of the -c file holding camera-matrix /\n"
                         "                            distortion-coeffs, one for every camera or one per SOURCE\n"
                         "       [--marker \"H=[lo,hi] S=[lo,hi] V=[lo,hi] e=K d=K area=[a,b]\"]... --marker-sinks M0,M1,..  [--heading-anchor I]\n"
                         "                            marker sets: one posidet hsv per --marker (repeatable, up to 8) behind ONE mog pass, and\n"
                         "                            posicom mean behind them: marker m of a camera is published on the m-th address of that\n"
                         "                            camera's --marker-sinks list (one list per camera, repeat the option), the mean position and --\n"
                         "                            with --heading-anchor I -- the heading from marker I to the others on the camera's SINK.\n"
                         "                            In a -c file: one [[track.marker]] table per marker (h-thresh, s-thresh, v-thresh, erode, dilate,\n"
                         "                            area) under the tracker's table name, marker-sinks = [\"a,b\", ..], heading-anchor = I.\n"
                         "                            Not with --kalman, --homography, --ring > 1, --ingest-root, -H/-S/-V, --thresh.\n"
                         "       [--marker-ring D]    (D >= 2; marker-ring in a -c file) marker mode through the pipelined loop: the cameras are\n"
                         "                            staged one by one, two frames a launch, results are published up to D - 1 rounds behind.\n"
                         "                            Without it a marker round is one synchronous step.\n"
                         "       [--mean-kalman [--dt s] [-T|--timeout s] [--sigma-accel a] [-n|--sigma-noise n]]  [--mean-homography [h11,...,h33]]\n"
                         "       [--region 'NAME=[[x0,y0],[x1,y1],...]']...\n"
                         "                            (all three need --marker) the filters of a marker rig, behind posicom mean: posifilt kalman,\n"
                         "                            posifilt homography and posifilt region on the mean position, in this order, each on its own\n"
                         "                            switch; the camera's SINK then carries the filtered position: position and velocity from the\n"
                         "                            Kalman filter, the heading through the homography, the name of the first --region (command-line\n"
                         "                            order; at most 16 of at most 64 points, names of at most 9 bytes) that holds the position.  With\n"
                         "                            or without --marker-ring; the per-marker sinks are unchanged.  In a -c file: mean-kalman = true,\n"
                         "                            mean-homography = [..], and one [[track.region]] table per region with name and points.\n"
                         "       [--target-sinks T0,T1,..]...   multi-target detection: the K largest blobs of every camera's mask inside the area\n"
                         "                            window, ranked by area (ties: the later first pixel first).  One comma list per camera (repeat\n"
                         "                            the option), every list of the same length K <= 8; rank j of a camera's frame goes to the j-th\n"
                         "                            address of its list as a Position2D with the frame's sample, invalid where fewer than j + 1 blobs\n"
                         "                            exist.  Rank 0 is the detector's own result; the SINK carries what it carries without the option\n"
                         "                            (--kalman / --homography act on the SINK only).  With or without --ring.  In a -c file:\n"
                         "                            target-sinks = [\"a,b\", \"c,d\"].  Not with --marker or --ingest-root.\n"
                         "       [--target-shape]     (with --target-sinks; target-shape = true in a -c file) target shapes: rank j's Position2D also\n"
                         "                            carries the blob's body axis -- the major axis of its second moments, a unit vector with x >= 0:\n"
                         "                            an axis has no front -- as its heading; no heading where the blob has no axis.\n"
                         "N SOURCEs / N SINKs: N cameras batched into one device pass per frame; SOURCE i feeds SINK i.\n"
                         "--gpu-index N0,N1,..: the cameras are split into contiguous blocks, one per listed device (own context and thread).\n"
                         "--ingest-root D0 (with --gpu-index D0,D1,..): all frames are ingested on device D0 and scattered to their devices\n"
                         "       over RCCL send/recv (one process, one thread); --timing prints bytes per peer and ms per step.\n"
                         "--print-partition: print which cameras go to which device (both forms) and exit; no device is touched.\n";
            return o.has("help") ? 0 : -1;
        }
        const char *ud_exclusive = "--camera-matrix / --distortion-coeffs and --undistort-key are mutually exclusive";
        if ((o.has("camera-matrix") || o.has("distortion-coeffs")) && o.has("undistort-key")) throw std::runtime_error(ud_exclusive);
        o.apply_config({"adaptation-coeff", "h-thresh", "s-thresh", "v-thresh", "erode", "dilate", "area", "model-file",
                        "kalman", "dt", "timeout", "sigma-accel", "sigma-noise", "gpu-index", "ring", "mask", "thresh", "homography", "stage-copy", "timing",
                        "ingest-root", "print-partition", "camera-matrix", "distortion-coeffs", "undistort-key", "marker-sinks", "heading-anchor", "marker-ring",
                        "mean-kalman", "mean-homography", "bayer", "target-sinks", "target-shape"},
                       {"kalman", "timing", "print-partition", "mean-kalman", "target-shape"});
        const std::vector<std::string> sources = split_list(o.positional[0]), sinks = split_list(o.positional[1]);
        if (sources.size() != sinks.size()) throw std::runtime_error("need as many SINKs as SOURCEs");
        // marker sets: --marker (repeatable) or the [[KEY.marker]] tables of the -c file; refused with what the synchronous
        // marker step does not extend to
        std::vector<oatgpu_marker> markers;
        if (o.all.count("marker")) for (const std::string &m : o.all["marker"]) markers.push_back(parse_marker(m));
        else if (!o.config_file.empty()) markers = read_marker_tables(o.config_file, o.config_key);
        std::vector<std::vector<std::string>> marker_sinks;
        int heading_anchor = -1, marker_ring = 0;
        // the filter chain behind the combined record: --region (repeatable) or the [[KEY.region]] tables of the -c file
        std::vector<RegionDef> regions;
        double mean_h[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        bool mean_homography = false;
        if (markers.empty()) {
            for (const char *k : {"mean-kalman", "mean-homography", "region"})
                if (o.has(k)) throw std::runtime_error(std::string("--") + k + " filters the mean position of a marker set: it needs at least one --marker");
            if (!o.config_file.empty() && !read_region_tables(o.config_file, o.config_key).empty())
                throw std::runtime_error("[[" + o.config_key + ".region]] (--region) filters the mean position of a marker set: it needs at least one --marker");
            if (o.has("marker-sinks") || o.has("heading-anchor")) throw std::runtime_error("--marker-sinks / --heading-anchor need at least one --marker");
            if (o.has("marker-ring")) throw std::runtime_error("--marker-ring needs at least one --marker");
        } else {
            if (o.has("marker-ring")) {
                char *end = nullptr;
                const long v = strtol(o.kv["marker-ring"].c_str(), &end, 10);
                if (end == o.kv["marker-ring"].c_str() || *end || v < 2 || v > 64)
                    throw std::runtime_error("--marker-ring: expected a ring depth in 2..64, got '" + o.kv["marker-ring"] + "'");
                marker_ring = (int)v;
            }
            for (const char *k : {"kalman", "homography", "ingest-root", "thresh"})
                if (o.has(k)) throw std::runtime_error(std::string("--marker does not go with --") + k +
                                                       (k[0] == 'k' ? " (the filter of a marker rig's mean position is --mean-kalman)"
                                                        : k[0] == 'h' ? " (the homography of a marker rig's mean position is --mean-homography)" : ""));
            for (const char *k : {"h-thresh", "s-thresh", "v-thresh"})
                if (o.has(k)) throw std::runtime_error(std::string("--marker does not go with --") + k + ": each marker has its own window (H= S= V= inside --marker)");
            if (o.num("ring", 1, 1, 64) > 1) throw std::runtime_error("--marker does not go with --ring > 1: the ring of marker mode is --marker-ring D (without it the marker step is synchronous, one round of frames at a time)");
            if (markers.size() > 8) throw std::runtime_error("--marker: at most 8 markers");
            if (o.all.count("region")) for (const std::string &r : o.all["region"]) regions.push_back(parse_region(r));
            else if (!o.config_file.empty()) regions = read_region_tables(o.config_file, o.config_key);
            if (regions.size() > 16) throw std::runtime_error("--region: " + std::to_string(regions.size()) + " regions, at most 16");
            if (o.has("mean-homography")) {
                Options h;
                h.kv["--mean-homography"] = o.kv["mean-homography"];
                mean_homography = h.arr9("--mean-homography", mean_h);
            }
            if (o.has("mean-kalman") && !(o.num("dt", 0.02, 0, 1e9) > 0)) throw std::runtime_error("--mean-kalman: --dt must be > 0");
            std::vector<std::string> lists;
            if (o.all.count("marker-sinks")) lists = o.all["marker-sinks"];
            else if (o.has("marker-sinks")) {                              // the -c file: "a,b" or ["a,b", "c,d"]
                const std::string &v = o.kv["marker-sinks"];
                size_t a = 0;
                while ((a = v.find_first_of("\"'", a)) != std::string::npos) {
                    const size_t b = v.find(v[a], a + 1);
                    if (b == std::string::npos) break;
                    lists.push_back(v.substr(a + 1, b - a - 1));
                    a = b + 1;
                }
                if (lists.empty()) lists.push_back(v);
            }
            if (lists.size() != sources.size())
                throw std::runtime_error("--marker-sinks: " + std::to_string(lists.size()) + " lists for " + std::to_string(sources.size()) +
                                         " SOURCEs (one comma list per camera: repeat the option)");
            for (const std::string &l : lists) {
                marker_sinks.push_back(split_list(l));
                if (marker_sinks.back().size() != markers.size())
                    throw std::runtime_error("--marker-sinks: '" + l + "' names " + std::to_string(marker_sinks.back().size()) + " sinks for " +
                                             std::to_string(markers.size()) + " markers");
            }
            if (o.has("heading-anchor")) {
                char *end = nullptr;
                const long v = strtol(o.kv["heading-anchor"].c_str(), &end, 10);
                if (end == o.kv["heading-anchor"].c_str() || *end || v < 0 || v >= (long)markers.size())   // MeanPosition.cpp:55-57
                    throw std::runtime_error("--heading-anchor: expected a marker index in 0.." + std::to_string(markers.size() - 1));
                heading_anchor = (int)v;
            }
        }
        // --target-sinks: one list per camera, all of one length; checked before any device is opened
        std::vector<std::vector<std::string>> target_sinks;
        if (o.has("target-sinks")) {
            if (o.has("ingest-root")) throw std::runtime_error("--ingest-root does not take --target-sinks");
            target_sinks = check_target_sinks(o.all.count("target-sinks") ? o.all["target-sinks"] : target_sink_lists_of_config(o.kv["target-sinks"]),
                                              sinks, !markers.empty());
        }
        check_target_shape(o.has("target-shape"), !target_sinks.empty());
        // --gpu-index N | N0,N1,...: one shard of the SOURCE list per listed device (contiguous blocks)
        std::vector<int> devices;
        for (const std::string &d : split_list(o.has("gpu-index") ? o.kv["gpu-index"] : std::string("0"))) {
            char *end = nullptr;
            const long v = strtol(d.c_str(), &end, 10);
            if (!end || *end || v < 0 || v > 1023) throw std::runtime_error("--gpu-index: expected N or N0,N1,... (device ordinals)");
            devices.push_back((int)v);
        }
        if (o.has("print-partition")) {
            // which cameras go to which device (camera s -> shard s / ceil(S / N), contiguous blocks, for life) --
            // printed without touching a device, for both launch forms; tests/test_host_pipeline.py holds it to oat_amd/dist.py
            const int S = (int)sources.size(), N = (int)devices.size(), per = (S + N - 1) / N;
            for (int k = 0; k < N && k * per < S; ++k)
                std::cout << "shard " << k << " device " << devices[k] << " cameras " << k * per << " " << std::min(S, (k + 1) * per)
                          << (o.has("ingest-root") ? (devices[k] == (int)o.num("ingest-root", 0, 0, 1023) ? " root" : " peer") : "") << "\n";
            return 0;
        }
        // `framefilt undistort` in front of the chain: one calibration per SOURCE, every one checked here, before any device is
        // opened (Undistorter.cpp:57-81).  --undistort-key names tables of the -c file (the reference's [undistort] table as it
        // is); the tracker's own table may be one of them, otherwise it may not hold a calibration of its own as well.
        std::vector<UndistortCalibration> cals;
        if (o.has("undistort-key")) {
            const std::vector<std::string> keys = split_list(o.kv["undistort-key"]);
            if (o.config_file.empty()) throw std::runtime_error("--undistort-key names tables of the configuration file: give -c FILE KEY");
            if ((o.has("camera-matrix") || o.has("distortion-coeffs")) && std::find(keys.begin(), keys.end(), o.config_key) == keys.end())
                throw std::runtime_error(ud_exclusive);
            if (keys.size() != 1 && keys.size() != sources.size())
                throw std::runtime_error("--undistort-key: " + std::to_string(keys.size()) + " tables for " + std::to_string(sources.size()) +
                                         " SOURCEs (give one for every camera or one per SOURCE)");
            for (const std::string &k : keys) {
                Options t;
                t.config_file = o.config_file;
                t.config_key = k;
                t.apply_config({"camera-matrix", "distortion-coeffs"});     // Undistorter.cpp:43-53
                cals.push_back(read_undistort_calibration(t));
            }
            if (cals.size() == 1) cals.assign(sources.size(), cals[0]);
        } else if (o.has("camera-matrix") || o.has("distortion-coeffs")) {
            cals.assign(sources.size(), read_undistort_calibration(o));
        }
        // --bayer: the SOURCEs' pixel format, one pattern for all cameras or one per SOURCE; checked before any device is opened
        std::vector<int32_t> bayer;
        if (o.has("bayer")) {
            if (o.has("thresh")) throw std::runtime_error("--bayer does not go with --thresh: demosaiced frames are BGR, --thresh selects the GREY chain");
            for (const std::string &p : split_list(o.kv["bayer"])) bayer.push_back(bayer_pattern(p));
            if (bayer.size() != 1 && bayer.size() != sources.size())
                throw std::runtime_error("--bayer: " + std::to_string(bayer.size()) + " patterns for " + std::to_string(sources.size()) +
                                         " SOURCEs (give one for every camera or one per SOURCE)");
            if (bayer.size() == 1) bayer.assign(sources.size(), bayer[0]);
        }
        if (o.has("ingest-root")) {                                       // the stream-to-rank scatter over RCCL (scatter_tracker.hpp)
            for (const char *k : {"kalman", "thresh", "mask", "model-file", "homography", "stage-copy"})
                if (o.has(k)) throw std::runtime_error(std::string("--ingest-root does not take --") + k);
            ScatterTracker t(sources, sinks, devices, (int)o.num("ingest-root", 0, 0, 1023));
            t.learning_coeff_ = o.num("adaptation-coeff", 0.0, 0.0, 1.0);
            double a, b;
            if (o.arr2("h-thresh", a, b)) { t.cfg_.h_lo = (int)a; t.cfg_.h_hi = (int)b; }
            if (o.arr2("s-thresh", a, b)) { t.cfg_.s_lo = (int)a; t.cfg_.s_hi = (int)b; }
            if (o.arr2("v-thresh", a, b)) { t.cfg_.v_lo = (int)a; t.cfg_.v_hi = (int)b; }
            if (o.has("erode")) t.cfg_.erode = (int)o.num("erode", 0, 0, 1e6);
            if (o.has("dilate")) t.cfg_.dilate = (int)o.num("dilate", 0, 0, 1e6);
            if (o.arr2("area", a, b)) { t.cfg_.min_area = a; t.cfg_.max_area = b; }
            t.cfg_.ring_depth = (int)o.num("ring", 2, 2, 64);
            t.timing_ = o.has("timing");
            t.undistort_ = cals;
            t.bayer_ = bayer;
            return t.run();
        }
        const int S = (int)sources.size(), N = (int)devices.size(), per = (S + N - 1) / N;
        std::vector<std::unique_ptr<BatchedTracker>> shards;
        for (int k = 0; k < N && k * per < S; ++k) {
            const int s0 = k * per, s1 = std::min(S, s0 + per);
            auto t = std::make_unique<BatchedTracker>(std::vector<std::string>(sources.begin() + s0, sources.begin() + s1),
                                                      std::vector<std::string>(sinks.begin() + s0, sinks.begin() + s1), s0, S);
            t->learning_coeff_ = o.num("adaptation-coeff", 0.0, 0.0, 1.0);
            double a, b;
            if (o.arr2("h-thresh", a, b)) { t->cfg_.h_lo = (int)a; t->cfg_.h_hi = (int)b; }
            if (o.arr2("s-thresh", a, b)) { t->cfg_.s_lo = (int)a; t->cfg_.s_hi = (int)b; }
            if (o.arr2("v-thresh", a, b)) { t->cfg_.v_lo = (int)a; t->cfg_.v_hi = (int)b; }
            if (o.arr2("thresh", a, b)) {                                 // SimpleThreshold.cpp:86-97
                if (a < 0 || a > 256 || b < 0 || b > 256) throw std::runtime_error("Values of thresh should be between 0 and 256.");
                t->grey_ = true;
                t->cfg_.h_lo = (int)a; t->cfg_.h_hi = (int)b;              // the one-channel window lives in the h slot
            }
            if (o.has("erode")) t->cfg_.erode = (int)o.num("erode", 0, 0, 1e6);
            if (o.has("dilate")) t->cfg_.dilate = (int)o.num("dilate", 0, 0, 1e6);
            if (o.arr2("area", a, b)) { t->cfg_.min_area = a; t->cfg_.max_area = b; }
            t->cfg_.device = devices[k];
            t->cfg_.ring_depth = marker_ring ? marker_ring : (int)o.num("ring", 2, 1, 64);
            t->marker_ring_ = marker_ring;
            if (o.has("model-file")) t->model_file_ = o.kv["model-file"];
            if (o.has("mask")) t->mask_file_ = o.kv["mask"];
            if (o.has("stage-copy")) {
                if (o.kv["stage-copy"] == "kernel") t->stage_copy_ = 1;
                else if (o.kv["stage-copy"] != "dma") throw std::runtime_error("--stage-copy: expected dma or kernel");
            }
            t->timing_ = o.has("timing");
            t->kalman_ = o.has("kalman");
            t->homography_on_ = o.arr9("homography", t->homography_);
            if (!cals.empty()) t->undistort_.assign(cals.begin() + s0, cals.begin() + s1);
            if (!bayer.empty()) t->bayer_.assign(bayer.begin() + s0, bayer.begin() + s1);
            if (!target_sinks.empty())
                t->set_targets(std::vector<std::vector<std::string>>(target_sinks.begin() + s0, target_sinks.begin() + s1), o.has("target-shape"));
            if (!markers.empty())
                t->set_markers(markers, heading_anchor, std::vector<std::vector<std::string>>(marker_sinks.begin() + s0, marker_sinks.begin() + s1));
            t->dt_ = o.num("dt", 0.02, 0, 1e9);                        // KalmanFilter2D.cpp:69-85 (lower bound 0)
            t->timeout_ = o.num("timeout", 0.0, 0, 1e18);
            t->sig_accel_ = o.num("sigma-accel", 5.0, 0, 1e18);
            t->sig_noise_ = o.num("sigma-noise", 0.0, 0, 1e18);
            t->mean_kalman_ = o.has("mean-kalman");
            t->mean_homography_on_ = mean_homography;
            std::copy(mean_h, mean_h + 9, t->mean_homography_);
            t->regions_ = regions;
            shards.push_back(std::move(t));
        }
        if (shards.size() == 1) return shards[0]->run();
        // one thread per shard: a device context belongs to the thread that drives it; SIGINT reaches every loop
        // through `quit` (the waits are 10 ms slices), END of a shard's SOURCEs ends that shard only
        // A shard that ends -- END of its SOURCEs, or a failure -- is DESTROYED at once, by its own thread: its SINKs go
        // END and its SOURCE slots are released while the other shards keep running, exactly what the exit of the
        // reference's one-camera process does for its consumers and producers (lib/shmemdf/Sink.h:73-91,
        // Source.h:90-112); the process exit code still reports the failure.
        std::vector<int> rc(shards.size(), 0);
        std::vector<std::thread> th;
        for (size_t k = 0; k < shards.size(); ++k)
            th.emplace_back([&, k] {
                pin_thread_to_device_node(shards[k]->cfg_.device);      // the shard's thread next to its GPU
                rc[k] = shards[k]->run();
                shards[k].reset();
            });
        for (auto &t : th) t.join();
        for (int r : rc) if (r) return r;
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "oat-track-hip: " << e.what() << std::endl;
        return -1;
    }
}
