// oat-frame-dump SOURCE FILE [-n N]
// The counterpart of oat-frameserve-raw at the other end of a frame pipeline: every frame token of SOURCE is appended to
// FILE as a headerless packed dump (rows*cols*channels bytes each), and one line per token -- "rows cols COLOR tick" -- goes to
// stdout.  For tests and for looking at what a frame filter publishes; no device, no OpenCV.
#include "component.hpp"

#include <fstream>

using namespace oat;

int main(int argc, char **argv)
{
    try {
        Options o = Options::parse(argc, argv, {{"n", "num"}, {"h", "help"}}, {"help"});
        if (o.has("help") || o.positional.size() != 2) { std::cout << "Usage: oat-frame-dump SOURCE FILE [-n N]\n"; return o.has("help") ? 0 : -1; }
        std::signal(SIGINT, sigHandler);
        const uint64_t n = (uint64_t)o.num("num", 1e18, 1, 1e18);
        std::ofstream out(o.positional[1], std::ios::binary);
        if (!out) throw std::runtime_error("cannot open " + o.positional[1]);
        Source<Frame> src;
        src.touch(o.positional[0]);
        if (src.connect() != SourceState::CONNECTED) return 0;
        const FrameParams p = src.parameters();
        const size_t fb = p.rows * p.cols * color_bytes(p.color);
        for (uint64_t i = 0; i < n && !quit; ++i) {
            if (src.wait() == NodeState::END) break;
            const Frame &f = *src.retrieve();
            out.write((const char *)f.data(), (std::streamsize)fb);
            const uint64_t tick = f.sample().count();
            src.post();
            std::cout << p.rows << " " << p.cols << " " << color_str(p.color) << " " << tick << std::endl;
        }
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "oat-frame-dump: " << e.what() << std::endl;
        return -1;
    }
}
