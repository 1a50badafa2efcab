// modes_check.cpp -- exercises dbot_amd::ParticleTracker::enable_modes / modes (include/dbot_amd/rb_sensor_builder.hpp): a
// tetrahedron in front of an 80 x 60 camera tracked over the frames of a file (tests/test_gpu_tracker_modes.py writes it and
// runs the Python mirror over the same frames).
//   modes_check FRAMES.bin   FRAMES.bin: int32 count, then count x 4800 doubles
//   -> per frame "FRAME k frame n_modes" and per mode "MODE seed" followed by density, mass, core_mass and the six delta
//      components as hex floats; "NO_DEVICE <message>" where there is no GPU.
#include <dbot_amd/rb_sensor_builder.hpp>

#include <cstdio>

typedef dbot_amd::FreeFloatingRigidBodiesState State;
typedef dbot_amd::RbSensorBuilder<State> SensorBuilder;
typedef dbot_amd::ObjectTransitionBuilder<State> TransitionBuilder;
typedef dbot_amd::ParticleTrackerBuilder<dbot_amd::ParticleTracker> TrackerBuilder;

int main(int argc, char** argv)
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
    params_obsrv.sample_count = 300;
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
    auto transition_builder = std::shared_ptr<TransitionBuilder>(new TransitionBuilder(TransitionBuilder::Parameters()));
    TrackerBuilder::Parameters params_tracker;
    params_tracker.evaluation_count = 300;
    params_tracker.seed = 11;
    std::shared_ptr<dbot_amd::ParticleTracker> tracker;
    try {
        tracker = TrackerBuilder(transition_builder, sensor_builder, object_model, params_tracker).build();
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
        return 0;
    }
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (std::fread(&count, sizeof(count), 1, f) != 1 || count < 1 || count > 64) return 2;
    State init(1);
    init.position(0)[2] = 0.7;
    tracker->initialize(std::vector<State>(1, init));
    bool refused = false;
    try {
        tracker->modes();                // the report is off
    } catch (const std::exception&) {
        refused = true;
    }
    if (!refused) return 3;
    tracker->enable_modes();
    std::vector<double> frame(static_cast<size_t>(rows) * cols);
    for (int k = 0; k < count; ++k) {
        if (std::fread(frame.data(), sizeof(double), frame.size(), f) != frame.size()) return 2;
        tracker->track(frame);
        const dbot_amd::ParticleTracker::Modes m = tracker->modes();
        std::printf("FRAME %d %d %d\n", k, m.frame, static_cast<int>(m.bodies[0].size()));
        for (const dbot_amd::ParticleTracker::Mode& mode : m.bodies[0]) {
            std::printf("MODE %d %a %a %a", mode.seed, mode.density, mode.mass, mode.core_mass);
            for (double v : mode.delta) std::printf(" %a", v);
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}
