// scene_find_check.cpp -- exercises the scene finder's mirror of include/dbot_amd/object_finder.hpp: two tetrahedra side by
// side 0.7 m in front of an 80 x 60 camera, found from their own depth image in front of a wall
// (tests/test_scene_find_cpu.py).
//   scene_find_check  -> "OK <order...> | <found mask> <|dt| of body 0, mm> <|dt| of body 1, mm> <joint score> <given back bit for bit>",
//                        or "NO_DEVICE <message>"
#include <dbot_amd/object_finder.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

typedef dbot_amd::FreeFloatingRigidBodiesState State;
typedef dbot_amd::RbSensorBuilder<State> SensorBuilder;

int main()
{
    const int rows = 60, cols = 80;
    double K[9] = {71.2875, 0, 39.5, 0, 71.2875, 29.5, 0, 0, 1};
    std::vector<std::vector<double>> verts(2);
    std::vector<std::vector<int32_t>> tris(2);
    verts[0] = {0, 0, 0, 0.2, 0, 0, 0, 0.2, 0, 0, 0, 0.2};
    verts[1] = {0, 0, 0, 0.3, 0, 0, 0, 0.3, 0, 0, 0, 0.3};
    tris[0] = tris[1] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
    auto object_model = std::make_shared<dbot_amd::ObjectModel>(verts, tris, /*center_object_frame=*/true);
    auto camera_data = std::make_shared<dbot_amd::CameraData>(dbot_amd::CameraData::from_native(K, cols, rows, 1));
    SensorBuilder::Parameters params_obsrv;
    params_obsrv.use_gpu = true;
    params_obsrv.sample_count = 1;
    params_obsrv.occlusion.p_occluded_visible = 0.1;
    params_obsrv.occlusion.p_occluded_occluded = 0.7;
    params_obsrv.occlusion.initial_occlusion_prob = 0.1;
    params_obsrv.kinect.tail_weight = 0.01;
    params_obsrv.kinect.model_sigma = 0.003;
    params_obsrv.kinect.sigma_factor = 0.0014247;
    params_obsrv.delta_time = 1. / 30.;
    params_obsrv.use_custom_shaders = false;
    params_obsrv.geometry_shader_file = "none";
    auto sensor_builder = std::shared_ptr<SensorBuilder>(new SensorBuilder(object_model, camera_data, params_obsrv));

    // the defaults and the refusals need no device
    dbot_amd::SceneFinder::Parameters sp;
    if (sp.explain_sigmas != 3.0 || sp.explain_radius != 2 || sp.polish_sweeps != 2 || sp.polish_children != 64 ||
        sp.polish_sigma_translation != 0.005 || std::fabs(sp.polish_sigma_angle - 5.0 * 3.14159265358979323846 / 180.0) > 1e-15 ||
        sp.polish_decay != 0.6) {
        std::printf("BAD_DEFAULTS\n");
        return 1;
    }
    dbot_amd::ObjectFinder::Parameters fp;
    rbs_find_scene* none = nullptr;
    dbot_amd::SceneFinder::Parameters bad;
    bad.explain_radius = 9;
    if (rbs_find_scene_create(nullptr, &fp, &bad, &none) != RBS_ERR_INVALID_ARGUMENT || none ||
        std::strcmp(rbs_last_error(nullptr), "find_scene: explain_radius outside 0..8") != 0) {
        std::printf("BAD_REFUSAL %s\n", rbs_last_error(nullptr));
        return 1;
    }
    if (rbs_find_scene_create(nullptr, &fp, nullptr, &none) != RBS_ERR_INVALID_ARGUMENT || none) return 1;   // (no sensor)

    std::shared_ptr<dbot_amd::RbSensor<State>> sensor;
    try {
        sensor = sensor_builder->build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    fp.max_seeds = 48;
    fp.n_rotations = 128;
    fp.n_candidates = 256;
    fp.n_survivors = 8;
    fp.rounds = 3;
    fp.children = 16;
    fp.batch = 4096;
    dbot_amd::SceneFinder finder(sensor, object_model, fp, sp);
    if (finder.parts() != 2) return 1;
    std::vector<dbot_amd::Real> truth = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.2, 0, 0.7, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.2, 0, 0.8};
    std::vector<float> depth(static_cast<size_t>(rows) * cols, 0.f);
    if (rbs_render_depth(sensor->handle(), truth.data(), depth.data()) != RBS_OK) return 1;
    for (float& d : depth)
        if (!(d < std::numeric_limits<float>::infinity())) d = 1.5f;
    dbot_amd::SceneFinder::Result r = finder.find(depth);
    std::printf("OK");
    for (int b : finder.order()) std::printf(" %d", b);
    double dt[2];
    for (int b = 0; b < 2; ++b) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (r.poses[12 * b + 9 + k] - truth[12 * b + 9 + k]) * (r.poses[12 * b + 9 + k] - truth[12 * b + 9 + k]);
        dt[b] = 1e3 * std::sqrt(s);
    }
    // body 1 alone, body 0 given: its pose comes back bit for bit
    dbot_amd::SceneFinder::Result g = finder.find(depth, 2u, truth);
    const bool same = std::memcmp(g.poses.data(), truth.data(), sizeof(dbot_amd::Real) * 12) == 0 && g.searched == 2u &&
                      finder.residual(1, rows, cols).size() == depth.size();
    bool threw = false;
    try {
        finder.find(depth, 2u);   // a body not searched and no poses given
    } catch (const std::exception&) {
        threw = true;
    }
    std::printf(" | %u %.3f %.3f %.3f %d\n", r.found, dt[0], dt[1], r.joint_score, same && threw ? 1 : 0);
    return 0;
}
