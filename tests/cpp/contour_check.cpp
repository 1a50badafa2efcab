// contour_check.cpp -- exercises the contour rule of include/dbot_amd/pose_assessor.hpp: a tetrahedron 0.7 m in front of
// an 80 x 60 camera, one pose judged against its own depth image in front of a wall, and against the wall alone with the
// body's depth image pressed into it (tests/test_contour_cpp.py).
//   contour_check  -> "OK <rim> <valid> <flush> <in_front> <beyond> <verdict> <first confirmed pose>
//                         <rim> <valid> <flush> <in_front> <beyond> <verdict> <first supported pose> <first confirmed pose>",
//                     or "NO_DEVICE <message>"
#include <dbot_amd/pose_assessor.hpp>

#include <cstdio>
#include <limits>

typedef dbot_amd::FreeFloatingRigidBodiesState State;
typedef dbot_amd::RbSensorBuilder<State> SensorBuilder;

int main()
{
    const int rows = 60, cols = 80;
    double K[9] = {71.2875, 0, 39.5, 0, 71.2875, 29.5, 0, 0, 1};
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

    // the verdict and the refusals need no device
    dbot_amd::PoseAssessor::Parameters p;
    dbot_amd::PoseAssessor::ContourParameters c;
    if (c.radius != 2 || c.min_rim_pixels != 16 || c.min_valid_fraction != 0.5 || c.min_contour_fraction != 0.3 || c.min_flush_fraction != 0.5) {
        std::printf("BAD_DEFAULTS\n");
        return 1;
    }
    rbs_contour_body body = rbs_contour_body();
    body.rim = body.valid = 100;
    body.flush = 50;
    body.in_front = 50;
    int32_t v = -1;
    if (rbs_contour_verdict(&c, &body, &v) != RBS_OK || v != RBS_CONTOUR_ABSENT) {
        std::printf("BAD_VERDICT %d\n", v);
        return 1;
    }
    dbot_amd::PoseAssessor::ContourParameters bad;
    bad.radius = 9;
    if (rbs_contour_verdict(&bad, &body, &v) != RBS_ERR_INVALID_ARGUMENT) return 1;

    std::shared_ptr<dbot_amd::RbSensor<State>> sensor;
    try {
        sensor = sensor_builder->build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    dbot_amd::PoseAssessor plain(sensor, object_model, p);
    dbot_amd::PoseAssessor assessor(sensor, object_model, p, c);
    if (plain.contour() || !assessor.contour() || assessor.contour_verdict(body) != RBS_CONTOUR_ABSENT) return 1;
    bool threw = false;
    try {
        plain.set_contour(bad);
    } catch (const std::exception&) {
        threw = true;
    }
    if (!threw || plain.contour()) return 1;
    std::vector<dbot_amd::Real> pose = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.7};
    std::vector<float> depth(static_cast<size_t>(rows) * cols, 0.f);
    if (rbs_render_depth(sensor->handle(), pose.data(), depth.data()) != RBS_OK) return 1;
    std::vector<float> object(depth), wall(depth);
    const float inf = std::numeric_limits<float>::infinity();
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const size_t i = static_cast<size_t>(y) * cols + x;
            if (depth[i] < inf) continue;
            object[i] = 1.5f;                // the frame IS the pose's depth image in front of a wall: the scene falls away at the rim
            float a = -inf;                  // a surface that goes on past the silhouette: the body's farthest depth within 2 pixels
            for (int v2 = (y < 2 ? 0 : y - 2); v2 <= y + 2 && v2 < rows; ++v2)
                for (int u2 = (x < 2 ? 0 : x - 2); u2 <= x + 2 && u2 < cols; ++u2) {
                    const float d = depth[static_cast<size_t>(v2) * cols + u2];
                    if (d < inf && d > a) a = d;
                }
            wall[i] = a > -inf ? a : 1.5f;
        }
    dbot_amd::PoseAssessor::Result r = assessor.assess(pose, object);
    dbot_amd::PoseAssessor::Result w = assessor.assess(pose, wall);
    dbot_amd::PoseAssessor::Result off = plain.assess(pose, object);
    if (!off.contour.empty() || !off.confirmed(0) || r.contour.size() != 1 || r.at(0, 0).rendered != off.at(0, 0).rendered) return 1;
    float ms[3] = {-1.f, -1.f, -1.f};
    threw = false;
    try {
        assessor.contour_kernel_ms(ms);      // the last call was a plain one
    } catch (const std::exception&) {
        threw = true;
    }
    if (!threw) return 1;
    const rbs_contour_body& a = r.contour_at(0, 0);
    const rbs_contour_body& b = w.contour_at(0, 0);
    std::printf("OK %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", a.rim, a.valid, a.flush, a.in_front, a.beyond, a.verdict, r.first_confirmed(),
                b.rim, b.valid, b.flush, b.in_front, b.beyond, b.verdict, w.first_supported(), w.first_confirmed());
    threw = false;
    try {
        assessor.assess(std::vector<dbot_amd::Real>(12, std::numeric_limits<double>::quiet_NaN()), object);
    } catch (const std::exception&) {
        threw = true;
    }
    return threw ? 0 : 1;
}
