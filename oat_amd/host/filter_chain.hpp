// filter_chain.hpp -- what the binaries with a filter chain `posifilt kalman` -> `posifilt homography` -> `posifilt region` on the
// device share: oat-track-hip (the mean position of a marker rig, oatgpu_set_marker_filters) and oat-posidet-hip (the motion and the
// subtraction tracker, oatgpu_set_tracker_filters).  The --region option and the [[KEY.region]] tables of the -c file, the regions
// as the library takes them, and the Position2D a filtered record is published as.
#pragma once
#include "component.hpp"

#include <cmath>
#include <cstring>
#include <fstream>

// One `posifilt region` polygon: --region 'NAME=[[x0,y0],[x1,y1],...]' (repeatable, command-line order is region order), or a
// [[KEY.region]] table of the -c file with name = "NAME" and points = [[x0,y0],...].  The library's limits are checked here,
// before a device is opened: at most 16 regions of at most 64 points, a name of 1 to 9 bytes (the reference's strcpy overruns its
// 10-byte field with more), every coordinate within +-32767 once rounded.
struct RegionDef {
    std::string name;
    std::vector<double> xy;
};
inline std::vector<double> parse_region_points(const std::string &text, const std::string &where)
{
    auto bad = [&](const char *what) { return std::runtime_error(where + ": " + what + " in '" + text + "' (expected [[x0,y0],[x1,y1],...])"); };
    const char *p = text.c_str();
    auto skip = [&] { while (*p == ' ' || *p == '\t') ++p; };
    auto number = [&](double &v) {
        skip();
        char *end = nullptr;
        v = strtod(p, &end);
        if (end == p) throw bad("expected a number");
        p = end;
        skip();
    };
    std::vector<double> xy;
    skip();
    if (*p++ != '[') throw bad("expected '['");
    skip();
    while (*p != ']') {
        if (*p++ != '[') throw bad("a point is a pair [x,y]");
        double x, y;
        number(x);
        if (*p++ != ',') throw bad("a point is a pair [x,y]");
        number(y);
        if (*p++ != ']') throw bad("a point is a pair [x,y]");
        xy.push_back(x); xy.push_back(y);
        skip();
        if (*p == ',') { ++p; skip(); if (*p == ']') throw bad("expected a point"); }
        else if (*p != ']') throw bad("expected ',' or ']'");
    }
    ++p;
    skip();
    if (*p) throw bad("text behind the closing ']'");
    return xy;
}
inline void check_region(const RegionDef &r, const std::string &where)
{
    if (r.name.empty()) throw std::runtime_error(where + ": a region needs a name");
    if (r.name.size() > 9) throw std::runtime_error(where + ": the name '" + r.name + "' is longer than 9 bytes");
    if (r.xy.size() / 2 > 64) throw std::runtime_error(where + ": region '" + r.name + "' has " + std::to_string(r.xy.size() / 2) + " points, at most 64");
    for (double v : r.xy)
        if (!(std::fabs(std::nearbyint(v)) <= 32767.0)) throw std::runtime_error(where + ": region '" + r.name + "' has a coordinate beyond +-32767");
}
inline RegionDef parse_region(const std::string &text)
{
    const size_t eq = text.find('=');
    if (eq == std::string::npos) throw std::runtime_error("--region: expected NAME=[[x0,y0],[x1,y1],...], got '" + text + "'");
    RegionDef r;
    r.name = text.substr(0, eq);
    r.xy = parse_region_points(text.substr(eq + 1), "--region");
    check_region(r, "--region");
    return r;
}
// every [[KEY.region]] table of the -c file, in file order; points may span lines
inline std::vector<RegionDef> read_region_tables(const std::string &file, const std::string &key)
{
    std::vector<RegionDef> out;
    std::ifstream in(file);
    if (!in) return out;
    auto trim = [](std::string t) {
        const size_t a = t.find_first_not_of(" \t\r\n"), b = t.find_last_not_of(" \t\r\n");
        return a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
    };
    auto next = [&](std::string &line) {
        if (!std::getline(in, line)) return false;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        line = trim(line);
        return true;
    };
    auto depth = [](const std::string &v) { int d = 0; for (char ch : v) d += ch == '[' ? 1 : ch == ']' ? -1 : 0; return d; };
    const std::string header = "[[" + key + ".region]]", where = header;
    std::vector<bool> named, pointed;
    std::string line;
    bool inside = false;
    while (next(line)) {
        if (line.empty()) continue;
        if (line.front() == '[' && line.find('=') == std::string::npos) {
            std::string h;
            for (char ch : line) if (ch != ' ' && ch != '\t') h += ch;
            inside = h == header;
            if (inside) { out.emplace_back(); named.push_back(false); pointed.push_back(false); }
            continue;
        }
        if (!inside) continue;
        const size_t eq = line.find('=');
        if (eq == std::string::npos) throw std::runtime_error(where + ": expected key = value");
        const std::string k = trim(line.substr(0, eq));
        std::string val = trim(line.substr(eq + 1)), more;
        while (depth(val) > 0 && next(more)) val += " " + more;
        if (k == "name") {
            if (val.size() < 2 || (val.front() != '"' && val.front() != '\'') || val.back() != val.front())
                throw std::runtime_error(where + ": name must be a string, got " + val);
            out.back().name = val.substr(1, val.size() - 2);
            named.back() = true;
        } else if (k == "points") {
            out.back().xy = parse_region_points(val, where);
            pointed.back() = true;
        } else {
            throw std::runtime_error(where + ": unknown key '" + k + "' (name, points)");
        }
    }
    for (size_t i = 0; i < out.size(); ++i) {
        if (!named[i] || !pointed[i]) throw std::runtime_error(where + ": a region table holds name and points");
        check_region(out[i], where);
    }
    return out;
}

// the regions as oatgpu_marker_filters takes them (rs keeps them; `regions` must outlive the setter's call); the caller fills
// the Kalman and homography members
inline oatgpu_marker_filters chain_filters(const std::vector<RegionDef> &regions, std::vector<oatgpu_region> &rs)
{
    rs.assign(regions.size(), oatgpu_region{});
    for (size_t i = 0; i < rs.size(); ++i) {
        std::strncpy(rs[i].name, regions[i].name.c_str(), sizeof rs[i].name);
        rs[i].n_points = (int32_t)(regions[i].xy.size() / 2);
        rs[i].xy = regions[i].xy.data();
    }
    oatgpu_marker_filters f{};
    f.n_regions = (int32_t)rs.size();
    f.regions = rs.data();
    return f;
}

// A filtered record as the token behind posifilt kalman / homography / region: position, velocity, heading, the name of the
// region (RegionFilter2D.cpp:140-146) and, with a homography h, WORLD units and the matrix (HomographyTransform2D.cpp:102)
inline void publish_filtered(oat::Position2D &pos, const oatgpu_filtered &f, const std::vector<RegionDef> &regions, const double *h)
{
    pos.position_valid = f.position_valid != 0;
    pos.position.x = f.x; pos.position.y = f.y;
    pos.velocity_valid = f.velocity_valid != 0;
    pos.velocity.x = f.vx; pos.velocity.y = f.vy;
    pos.heading_valid = f.heading_valid != 0;
    pos.heading.x = f.hx; pos.heading.y = f.hy;
    if (f.region_valid) {
        pos.region_valid = true;
        std::strncpy(pos.region, regions[(size_t)f.region].name.c_str(), sizeof pos.region - 1);
    }
    if (h) pos.setCoordSystem(oat::DistanceUnit::WORLD, h);
}
