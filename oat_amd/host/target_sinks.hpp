// target_sinks.hpp -- `--target-sinks T0,T1,..` of oat-posidet-hip and oat-track-hip (multi-target detection, oatgpu_set_targets):
// one comma list per camera, K = the list's length, the same for every camera; sink j receives rank j of its camera on every
// frame.  With `--target-shape` (target shapes, oatgpu_set_target_shapes) rank j's Position2D also carries the blob's body axis as
// its heading.  Everything is checked at start-up, before a device is opened.
#pragma once
#include "component.hpp"

#include <set>

namespace oat {

inline std::vector<std::string> target_sink_names(const std::string &s)
{
    std::vector<std::string> out;
    size_t a = 0;
    while (a <= s.size()) {
        const size_t b = s.find(',', a);
        out.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    return out;
}

// the lists of a -c file's `target-sinks = "a,b"` or `= ["a,b", "c,d"]`
inline std::vector<std::string> target_sink_lists_of_config(const std::string &v)
{
    std::vector<std::string> lists;
    size_t a = 0;
    while ((a = v.find_first_of("\"'", a)) != std::string::npos) {
        const size_t b = v.find(v[a], a + 1);
        if (b == std::string::npos) break;
        lists.push_back(v.substr(a + 1, b - a - 1));
        a = b + 1;
    }
    if (lists.empty()) lists.push_back(v);
    return lists;
}

// lists: one per camera; sinks: the cameras' ordinary SINKs (a target sink may not repeat one of them either); taken: names that
// are in use besides (--track-sinks: the target sinks); option: the option the lists came from, for the messages
inline std::vector<std::vector<std::string>> check_target_sinks(const std::vector<std::string> &lists, const std::vector<std::string> &sinks,
                                                                bool markers, const std::string &option = "--target-sinks",
                                                                const std::vector<std::string> &taken = {})
{
    if (markers)
        throw std::runtime_error(option + " does not go with --marker: targets rank the blobs of one mask, a marker set has one mask a marker");
    if (lists.size() != sinks.size())
        throw std::runtime_error(option + ": " + std::to_string(lists.size()) + " lists for " + std::to_string(sinks.size()) +
                                 " SOURCEs (one comma list per camera: repeat the option)");
    std::vector<std::vector<std::string>> out;
    std::set<std::string> seen(sinks.begin(), sinks.end());
    seen.insert(taken.begin(), taken.end());
    for (const std::string &l : lists) {
        out.push_back(target_sink_names(l));
        if (out.back().size() > OATGPU_MAX_TARGETS)
            throw std::runtime_error(option + ": '" + l + "' names " + std::to_string(out.back().size()) + " sinks, at most " +
                                     std::to_string(OATGPU_MAX_TARGETS));
        if (out.back().size() != out.front().size())
            throw std::runtime_error(option + ": lists of different lengths (" + std::to_string(out.front().size()) + " and " +
                                     std::to_string(out.back().size()) + "): K is the same for every camera");
        for (const std::string &name : out.back()) {
            if (name.empty()) throw std::runtime_error(option + ": an empty sink name in '" + l + "'");
            if (!seen.insert(name).second) throw std::runtime_error(option + ": sink '" + name + "' is named twice");
        }
    }
    return out;
}

// --target-shape without --target-sinks is refused at start-up
inline void check_target_shape(bool shape, bool have_target_sinks)
{
    if (shape && !have_target_sinks)
        throw std::runtime_error("--target-shape needs --target-sinks: the body axis travels as the heading of the ranked blobs' tokens");
}

// rank j of a camera as the Position2D its sink receives: a detector's token (DetectorFunc.cpp:46,58-60), invalid where the rank is
// empty; shape (--target-shape): the rank's oatgpu_shape, whose body axis becomes the token's heading -- an axis has no front, its
// sign is oatgpu_shape's rule
inline Position2D target_position(const oatgpu_position &r, const Sample &sample, const oatgpu_shape *shape = nullptr)
{
    Position2D pos("");
    pos.set_sample(sample);
    pos.position_valid = r.valid != 0;
    if (r.valid) { pos.position.x = r.x; pos.position.y = r.y; }
    if (shape && shape->valid && shape->axis_valid) {
        pos.heading_valid = true;
        pos.heading.x = shape->axis_x; pos.heading.y = shape->axis_y;
    }
    return pos;
}

}  // namespace oat
