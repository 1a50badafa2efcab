// The finder's silhouette gate through the C++ mirror (include/dbot_amd/object_finder.hpp, ObjectFinder::Gate,
// ObjectFinder::evidence, SceneFinder::set_gate): one find with the gate at the two rules' defaults and require_confirmed on
// one frame, after a setting the library refuses.  Compiled and run by tests/test_find_gate_cpp.py, against Python.
//
//   find_gate_check <in.bin> <out.bin>
//
// in.bin: as tests/cpp/find_refinement_check.cpp's.  out.bin: int32 found, n; double poses [n][12], scores [n],
// states [n][12]; int32 the result's records [n][10] and classes [n].  Exit status 0; "NO_DEVICE" on stdout (and status 0)
// where no device can be opened.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "dbot_amd/object_finder.hpp"

using namespace dbot_amd;

template <typename T> static bool get(std::FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: find_gate_check in.bin out.bin\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t h[11];
    double K[9];
    if (!get(f, h, 11) || !get(f, K, 9)) { std::fprintf(stderr, "short input\n"); return 2; }
    const int cols = h[0], rows = h[1];
    std::vector<std::vector<Real>> vs(1, std::vector<Real>(3 * static_cast<size_t>(h[2])));
    std::vector<std::vector<int32_t>> ts(1, std::vector<int32_t>(3 * static_cast<size_t>(h[3])));
    ObjectFinder::Obsrv frame(static_cast<size_t>(cols) * rows);
    const bool ok = get(f, vs[0].data(), vs[0].size()) && get(f, ts[0].data(), ts[0].size()) && get(f, frame.data(), frame.size());
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }

    auto om = std::make_shared<ObjectModel>(vs, ts, false);
    auto cam = std::make_shared<CameraData>();
    for (int i = 0; i < 9; ++i) cam->camera_matrix[i] = K[i];
    cam->resolution.width = cols;
    cam->resolution.height = rows;
    RbSensorBuilder<>::Parameters sp;
    sp.sample_count = 1;
    ObjectFinder::Parameters p;
    p.max_seeds = h[4];
    p.n_rotations = h[5];
    p.n_candidates = h[6];
    p.n_survivors = h[7];
    p.rounds = h[8];
    p.children = h[9];
    p.batch = h[10];
    std::shared_ptr<RbSensor<>> sensor;
    try {
        sensor = RbSensorBuilder<>(om, cam, sp).build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    ObjectFinder::Result r;
    ObjectFinder::Evidence ev;
    try {
        ObjectFinder finder(sensor, om, p);
        ObjectFinder::Gate g;
        if (g.enabled != 1 || g.require_confirmed != 0 || g.radius != 2 || g.min_rim_pixels != 16 || g.min_pixels != 16 || g.sigmas != 3.0 ||
            g.min_support_fraction != 0.5 || g.min_visible_fraction != 0.25 || g.min_valid_fraction != 0.5 || g.min_contour_fraction != 0.3 ||
            g.min_flush_fraction != 0.5) {
            std::fprintf(stderr, "ObjectFinder::Gate: not the two rules' defaults\n");
            return 1;
        }
        g.require_confirmed = 1;
        finder.set_gate(&g);
        ObjectFinder::Gate bad;
        bad.radius = 9;
        bool refused = false;
        try {
            finder.set_gate(&bad);
        } catch (const std::runtime_error&) {
            refused = true;                 // ... and the setting of before stays
        }
        if (!refused) {
            std::fprintf(stderr, "radius 9 was accepted\n");
            return 1;
        }
        r = finder.find(frame);
        ev = finder.evidence(RBS_FIND_RESULT);
        SceneFinder scene(sensor, om, p);   // a scene finder of one body takes the setting too, and refuses the bad one
        scene.set_gate(&g);
        refused = false;
        try {
            scene.set_gate(&bad);
        } catch (const std::runtime_error&) {
            refused = true;
        }
        if (!refused) {
            std::fprintf(stderr, "SceneFinder: radius 9 was accepted\n");
            return 1;
        }
        scene.set_gate(nullptr);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    const int32_t head[2] = {r.found ? 1 : 0, static_cast<int32_t>(r.scores.size())};
    std::vector<double> states;
    for (const auto& s : r.states) states.insert(states.end(), s.data().begin(), s.data().end());
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(head, sizeof(int32_t), 2, o) != 2 ||
        std::fwrite(r.poses.data(), sizeof(double), r.poses.size(), o) != r.poses.size() ||
        std::fwrite(r.scores.data(), sizeof(double), r.scores.size(), o) != r.scores.size() ||
        std::fwrite(states.data(), sizeof(double), states.size(), o) != states.size() ||
        std::fwrite(ev.records.data(), sizeof(int32_t), ev.records.size(), o) != ev.records.size() ||
        std::fwrite(ev.classes.data(), sizeof(int32_t), ev.classes.size(), o) != ev.classes.size()) {
        std::perror(argv[2]);
        return 2;
    }
    std::fclose(o);
    std::printf("OK %d poses\n", head[1]);
    return 0;
}
