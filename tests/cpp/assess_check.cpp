// assess_check.cpp -- exercises include/dbot_amd/pose_assessor.hpp: a tetrahedron 0.7 m in front of an 80 x 60 camera,
// one pose judged against its own depth image (tests/test_assess_cpp.py).
//   assess_check  -> "OK <rendered> <valid> <support> <in_front> <behind> <verdict> <first supported pose>", or "NO_DEVICE <message>"
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

    // the verdict needs no device
    dbot_amd::PoseAssessor::Parameters p;
    rbs_assess_body body = rbs_assess_body();
    body.rendered = body.valid = 100;
    body.support = 20;
    body.in_front = 59;
    body.behind = 21;
    int32_t v = -1;
    if (rbs_assess_verdict(&p, &body, &v) != RBS_OK || v != RBS_ASSESS_LOST) {
        std::printf("BAD_VERDICT %d\n", v);
        return 1;
    }

    std::shared_ptr<dbot_amd::RbSensor<State>> sensor;
    try {
        sensor = sensor_builder->build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    dbot_amd::PoseAssessor assessor(sensor, object_model, p);
    if (assessor.verdict(body) != RBS_ASSESS_LOST) return 1;
    std::vector<dbot_amd::Real> pose = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.7};
    std::vector<float> frame(static_cast<size_t>(rows) * cols, 0.f);
    if (rbs_render_depth(sensor->handle(), pose.data(), frame.data()) != RBS_OK) return 1;   // the frame IS the pose's depth image ...
    for (float& f : frame)
        if (!(f < std::numeric_limits<float>::infinity())) f = 1.5f;                        // ... in front of a wall
    dbot_amd::PoseAssessor::Result r = assessor.assess(pose, frame);
    const rbs_assess_body& b = r.at(0, 0);
    std::printf("OK %d %d %d %d %d %d %d\n", b.rendered, b.valid, b.support, b.in_front, b.behind, b.verdict, r.first_supported());
    bool threw = false;
    try {
        assessor.assess(std::vector<dbot_amd::Real>(12, std::numeric_limits<double>::quiet_NaN()), frame);
    } catch (const std::exception&) {
        threw = true;
    }
    return threw ? 0 : 1;
}
