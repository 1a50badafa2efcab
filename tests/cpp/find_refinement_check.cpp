// The object finder's step 6b through the C++ mirror (include/dbot_amd/object_finder.hpp, ObjectFinder::Refinement): one find
// with the library's default refinement on one frame, after a setting the library refuses.  Compiled and run by
// tests/test_gpu_find_refinement.py, against Python.
//
//   find_refinement_check <in.bin> <out.bin>
//
// in.bin (native endianness): int32 cols, rows, vertex count, triangle count, max_seeds, n_rotations, n_candidates,
// n_survivors, rounds, children, batch; double K[9]; the vertices (double xyz, used as they are: the caller centres
// them) and triangles (int32); float frame [rows * cols].  out.bin: int32 found, n; double poses [n][12], scores [n],
// states [n][12], the final covariances [n][36] (by survivor, not by rank).  Exit status 0; "NO_DEVICE" on stdout (and status 0)
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
        std::fprintf(stderr, "usage: find_refinement_check in.bin out.bin\n");
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
    std::vector<Real> cov;
    try {
        ObjectFinder finder(sensor, om, p);
        ObjectFinder::Refinement g;
        if (g.enabled != 1 || g.elite != 8 || g.mix != 0.5 || g.shrink != 1.0 || g.jitter != 1e-10) {
            std::fprintf(stderr, "ObjectFinder::Refinement: not the library's defaults\n");
            return 1;
        }
        finder.set_refinement(&g);
        ObjectFinder::Refinement bad;
        bad.elite = p.children + 1;
        bool refused = false;
        try {
            finder.set_refinement(&bad);
        } catch (const std::runtime_error&) {
            refused = true;                 // ... and the setting of before stays
        }
        if (!refused) {
            std::fprintf(stderr, "elite > children was accepted\n");
            return 1;
        }
        r = finder.find(frame);
        cov = finder.covariance(p.rounds);
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
        std::fwrite(cov.data(), sizeof(double), cov.size(), o) != cov.size()) {
        std::perror(argv[2]);
        return 2;
    }
    std::fclose(o);
    std::printf("OK %d poses\n", head[1]);
    return 0;
}
