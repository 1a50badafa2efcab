// The Gaussian tracker through the C++ mirror (include/dbot_amd/gaussian_tracker_builder.hpp), frame by frame
// (track) or with one frame of look-ahead (submit k+1 before result k).  Driven by tests/test_gaussian_pipeline_cpu.py
// (compiled there) and tests/test_gpu_gaussian_pipeline.py (run there).
//
//   gauss_pipeline_check --track|--submit <in.bin> <out.bin>
//
// in.bin (native endianness): int32 parts, cols, rows, frames; double K[9]; per part int32 vertex count, triangle count;
// the vertices (double xyz) and triangles (int32) of every part in turn; double initial state [12 parts] (original mesh
// frame); double frames [frames][rows * cols].  out.bin: double states [frames][12 parts], then the last covariance.
// Exit status 0; "NO_DEVICE" on stdout (and status 0) where no device can be opened.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "dbot_amd/gaussian_tracker_builder.hpp"

using namespace dbot_amd;

template <typename T> static bool get(std::FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 4 || (std::strcmp(argv[1], "--track") && std::strcmp(argv[1], "--submit"))) {
        std::fprintf(stderr, "usage: gauss_pipeline_check --track|--submit in.bin out.bin\n");
        return 2;
    }
    const bool lookahead = !std::strcmp(argv[1], "--submit");
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 2; }
    int32_t hdr[4];
    double K[9];
    if (!get(f, hdr, 4) || !get(f, K, 9)) { std::fprintf(stderr, "short input\n"); return 2; }
    const int parts = hdr[0], cols = hdr[1], rows = hdr[2], nf = hdr[3];
    const size_t npx = static_cast<size_t>(cols) * rows;
    std::vector<int32_t> counts(2 * static_cast<size_t>(parts));
    if (!get(f, counts.data(), counts.size())) { std::fprintf(stderr, "short input\n"); return 2; }
    std::vector<std::vector<Real>> vs(parts);
    std::vector<std::vector<int32_t>> ts(parts);
    for (int b = 0; b < parts; ++b) {
        vs[b].resize(3 * static_cast<size_t>(counts[2 * b]));
        ts[b].resize(3 * static_cast<size_t>(counts[2 * b + 1]));
        if (!get(f, vs[b].data(), vs[b].size()) || !get(f, ts[b].data(), ts[b].size())) { std::fprintf(stderr, "short input\n"); return 2; }
    }
    GaussianTracker::State init(parts);
    std::vector<GaussianTracker::Obsrv> frames(nf, GaussianTracker::Obsrv(npx));
    bool ok = get(f, init.data().data(), init.data().size());
    for (int k = 0; ok && k < nf; ++k) ok = get(f, frames[k].data(), npx);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }

    auto om = std::make_shared<ObjectModel>(vs, ts, true);
    auto cam = std::make_shared<CameraData>();
    for (int i = 0; i < 9; ++i) cam->camera_matrix[i] = K[i];
    cam->resolution.width = cols;
    cam->resolution.height = rows;
    GaussianTrackerBuilder<>::Parameters p;
    p.object_transition.part_count = parts;
    std::shared_ptr<GaussianTracker> tracker;
    try {
        tracker = GaussianTrackerBuilder<>(om, cam, p).build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    std::vector<double> out;
    try {
        tracker->initialize({init});
        auto keep = [&](const GaussianTracker::State& s) { out.insert(out.end(), s.data().begin(), s.data().end()); };
        if (lookahead) {
            if (nf > 0) tracker->submit(frames[0]);
            for (int k = 0; k < nf; ++k) {
                if (k + 1 < nf) tracker->submit(frames[k + 1]);
                keep(tracker->result());
            }
        } else {
            for (int k = 0; k < nf; ++k) keep(tracker->track(frames[k]));
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    const std::vector<Real>& cov = tracker->covariance();
    out.insert(out.end(), cov.begin(), cov.end());
    std::FILE* o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) { std::perror(argv[3]); return 2; }
    std::fclose(o);
    std::printf("OK %d frames\n", nf);
    return 0;
}
