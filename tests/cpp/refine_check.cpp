// refine_check.cpp -- exercises include/dbot_amd/pose_refiner.hpp: a tetrahedron 0.7 m in front of a 160 x 120 camera, its
// pose moved 3 mm along x and refined against its own depth image (tests/test_refine_cpp.py).
//   refine_check  -> "OK <status> <iterations> <count first> <count last> <|t - truth| before, m> <after, m> <first iteration's status>",
//                    or "NO_DEVICE <message>"
#include <dbot_amd/pose_refiner.hpp>

#include <cmath>
#include <cstdio>
#include <limits>

typedef dbot_amd::FreeFloatingRigidBodiesState State;
typedef dbot_amd::RbSensorBuilder<State> SensorBuilder;

int main()
{
    const int rows = 120, cols = 160;
    double K[9] = {142.575, 0, 79.5, 0, 142.575, 59.5, 0, 0, 1};
    std::vector<std::vector<double>> verts(1);
    std::vector<std::vector<int32_t>> tris(1);
    verts[0] = {0, 0, 0, 0.2, 0, 0, 0, 0.2, 0, 0, 0, 0.2};
    tris[0] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
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

    // the parameter check needs no device
    dbot_amd::PoseRefiner::Parameters p;
    if (p.iters != 10 || p.min_pixels != 16 || rbs_refine_check_params(&p) != RBS_OK) {
        std::printf("BAD_DEFAULTS\n");
        return 1;
    }
    dbot_amd::PoseRefiner::Parameters bad;
    bad.iters = 33;
    if (rbs_refine_check_params(&bad) != RBS_ERR_INVALID_ARGUMENT) {
        std::printf("BAD_CHECK\n");
        return 1;
    }

    std::shared_ptr<dbot_amd::RbSensor<State>> sensor;
    try {
        sensor = sensor_builder->build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    bool threw = false;
    try {
        dbot_amd::PoseRefiner refused(sensor, object_model, bad);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) return 1;
    dbot_amd::PoseRefiner refiner(sensor, object_model, p);
    // the right-angled corner towards the camera, so that three faces show: a single face leaves the pose free to slide in
    // its plane (RBS_REFINE_DEGENERATE)
    const double a = 1.0 / std::sqrt(2.0), b6 = 1.0 / std::sqrt(6.0), g = 1.0 / std::sqrt(3.0);
    std::vector<dbot_amd::Real> truth = {a, -a, 0, b6, b6, -2 * b6, g, g, g, 0, 0, 0.7};
    std::vector<float> frame(static_cast<size_t>(rows) * cols, 0.f);
    if (rbs_render_depth(sensor->handle(), truth.data(), frame.data()) != RBS_OK) return 1;   // the frame IS the truth's depth image ...
    for (float& f : frame)
        if (!(f < std::numeric_limits<float>::infinity())) f = 1.5f;                         // ... in front of a wall
    std::vector<dbot_amd::Real> start = truth;
    start[9] += 0.003;
    dbot_amd::PoseRefiner::Result r = refiner.refine(start, frame);
    const rbs_refine_body& b = r.at(0, 0);
    const double after = std::sqrt((r.poses[9] - truth[9]) * (r.poses[9] - truth[9]) + (r.poses[10] - truth[10]) * (r.poses[10] - truth[10]) +
                                   (r.poses[11] - truth[11]) * (r.poses[11] - truth[11]));
    const rbs_refine_history h0 = refiner.history(0, 0, 0);
    float ms[3];
    refiner.kernel_ms(ms);
    std::printf("OK %d %d %d %d %.6f %.6f %d\n", b.status, b.iterations, b.count_first, b.count_last, 0.003, after, h0.status);
    threw = false;
    try {
        refiner.refine(std::vector<dbot_amd::Real>(12, std::numeric_limits<double>::quiet_NaN()), frame);
    } catch (const std::exception&) {
        threw = true;
    }
    return threw && h0.pose[9] == start[9] && ms[0] > 0.f ? 0 : 1;
}
