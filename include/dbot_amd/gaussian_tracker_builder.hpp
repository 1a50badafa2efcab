// gaussian_tracker_builder.hpp -- C++ host-side mirror of the reference's second tracker, the robust
// Gaussian tracker, over the C-ABI of librbsensor_mi355x.so (rbs_gauss_*), in the style of
// rb_sensor_builder.hpp.
//
// It keeps the names of what R:source/dbot_ros/tracker/gaussian_tracker_node.cpp constructs:
//     dbot::GaussianTrackerBuilder<Tracker>::Parameters (field names)   :71-133
//     tracker->initialize(initial_poses) / tracker->track(image) -> State
// The filter is this project's restatement: sigma poses rendered and reduced on
// the sensor's device, the small algebra on the host inside the library.  The object model is loaded by
// the caller (params.ori names the meshes, as in the node) and handed to the builder with the camera data.
//
// Header-only; link with -lrbsensor_mi355x.  No CPU fallback: without a device build() throws.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rb_sensor_builder.hpp"

namespace dbot_amd
{
/// dbot::ObjectResourceIdentifier as the node fills it (package path, directory, mesh file names).
struct ObjectResourceIdentifier {
    std::string package_path, directory;
    std::vector<std::string> meshes;
    int count_meshes() const { return static_cast<int>(meshes.size()); }
};

/// The tracker the builder returns: initialize(initial_states), track(image) -> State.
class GaussianTracker
{
public:
    typedef FreeFloatingRigidBodiesState State;
    typedef std::vector<Real> Obsrv;  // rows*cols depth image, metres, NaN = no reading

    GaussianTracker(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om,
                    const rbs_gauss_params& gp, bool center_object_frame, Real moving_average_update_rate)
        : sensor_(sensor), om_(om), center_(center_object_frame), rate_(moving_average_update_rate), parts_(om->count_parts())
    {
        if (rbs_gauss_create(sensor_->handle(), &gp, &g_) != RBS_OK)
            throw std::runtime_error(std::string("GaussianTracker: ") + rbs_last_error(sensor_->handle()));
    }
    ~GaussianTracker() { rbs_gauss_destroy(g_); }
    GaussianTracker(const GaussianTracker&) = delete;
    GaussianTracker& operator=(const GaussianTracker&) = delete;

    /// The first initial state is the default pose (velocities zeroed); mean delta 0, the library's
    /// initial covariance (per body diag(lin^2, ang^2, lin^2, ang^2)).
    void initialize(const std::vector<State>& initial_states)
    {
        if (initial_states.empty()) throw std::runtime_error("GaussianTracker::initialize: no initial state");
        State m = shift(initial_states[0], +1.0);
        for (int b = 0; b < parts_; ++b)
            for (int k = 6; k < 12; ++k) m.component(b)[k] = 0.0;
        check(rbs_gauss_initialize(g_, m.data().data(), nullptr));
        have_average_ = false;
    }

    State track(const Obsrv& image)
    {
        State model(parts_);
        covariance_.resize(static_cast<size_t>(12 * parts_) * static_cast<size_t>(12 * parts_));
        check(rbs_gauss_track_f64(g_, image.data(), model.data().data(), covariance_.data()));
        return averaged(model);
    }
    /// The same frame in two halves (rbs_gauss_submit_f64 / rbs_gauss_result), the whole filter step on the
    /// device: a caller that has the next image before it needs this estimate keeps up to two frames in flight.
    void submit(const Obsrv& image)
    {
        check(rbs_gauss_submit_f64(g_, image.data()));
    }
    State result()
    {
        State model(parts_);
        covariance_.resize(static_cast<size_t>(12 * parts_) * static_cast<size_t>(12 * parts_));
        check(rbs_gauss_result(g_, model.data().data(), covariance_.data()));
        return averaged(model);
    }
    /// The belief's covariance after the last frame: (12 parts)^2 reals, row-major, model coordinates.
    const std::vector<Real>& covariance() const { return covariance_; }

private:
    State averaged(const State& model)
    {
        State est = shift(model, -1.0);
        if (!have_average_) { average_ = est; have_average_ = true; }
        else
            for (size_t k = 0; k < est.data().size(); ++k)
                average_.data()[k] = rate_ * est.data()[k] + (1.0 - rate_) * average_.data()[k];
        return average_;
    }
    void check(int32_t rc) const
    {
        if (rc != RBS_OK) throw std::runtime_error(std::string("GaussianTracker: ") + rbs_last_error(sensor_->handle()));
    }
    // camera-frame pose of the ORIGINAL mesh frame <-> pose of the centred mesh frame
    State shift(const State& s, Real sign) const
    {
        State o = s;
        if (!center_) return o;
        Real R[9];
        for (int b = 0; b < parts_; ++b) {
            State::rotation_matrix(o.euler_vector(b), R);
            const Real* c = om_->centers().data() + 3 * b;
            for (int r = 0; r < 3; ++r) o.position(b)[r] += sign * (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
        }
        return o;
    }
    std::shared_ptr<RbSensor<State>> sensor_;
    std::shared_ptr<ObjectModel> om_;
    bool center_;
    Real rate_;
    int parts_;
    rbs_gauss* g_ = nullptr;
    State average_{1};
    bool have_average_ = false;
    std::vector<Real> covariance_;
};

/// dbot::GaussianTrackerBuilder<Tracker>(params, camera_data).build() (R:...gaussian_tracker_node.cpp:135-140).
template <typename Tracker = GaussianTracker>
class GaussianTrackerBuilder
{
public:
    typedef typename Tracker::State State;
    struct Parameters {
        ObjectResourceIdentifier ori;
        Real ut_alpha = 1.0;
        Real moving_average_update_rate = 1.0;
        bool center_object_frame = true;
        struct Observation {
            Real tail_weight = 0.1;
            Real bg_depth = -3.0;
            Real fg_noise_std = 0.001;
            Real bg_noise_std = 100.0;
            Real uniform_tail_min = -5000.0;
            Real uniform_tail_max = 5000.0;
            int sensors = 0;   // pixels (camera_data->pixels())
        } observation;
        struct ObjectTransition {
            Real linear_sigma_x = 0.002, linear_sigma_y = 0.002, linear_sigma_z = 0.002;
            Real angular_sigma_x = 0.01, angular_sigma_y = 0.01, angular_sigma_z = 0.01;
            Real velocity_factor = 0.8;
            int part_count = 1;
        } object_transition;
        int device_id = 0;     // HIP ordinal of the device the sigma poses are rendered on
    };

    GaussianTrackerBuilder(const std::shared_ptr<ObjectModel>& object_model, const std::shared_ptr<CameraData>& camera_data,
                           const Parameters& params)
        : om_(object_model), cam_(camera_data), params_(params)
    {
    }

    std::shared_ptr<Tracker> build() const
    {
        // the device handle the tracker renders with: one slot, the sensor's likelihood parameters unused
        typename RbSensorBuilder<State>::Parameters sp;
        sp.sample_count = 1;
        auto sensor = std::make_shared<RbSensor<State>>(*om_, *cam_, sp, params_.device_id);
        const auto& t = params_.object_transition;
        const auto& o = params_.observation;
        rbs_gauss_params p{};
        p.linear_sigma[0] = t.linear_sigma_x; p.linear_sigma[1] = t.linear_sigma_y; p.linear_sigma[2] = t.linear_sigma_z;
        p.angular_sigma[0] = t.angular_sigma_x; p.angular_sigma[1] = t.angular_sigma_y; p.angular_sigma[2] = t.angular_sigma_z;
        p.velocity_factor = t.velocity_factor;
        p.ut_alpha = params_.ut_alpha;
        p.fg_noise_std = o.fg_noise_std;
        p.bg_depth = o.bg_depth;
        p.bg_noise_std = o.bg_noise_std;
        p.tail_weight = o.tail_weight;
        p.uniform_tail_min = o.uniform_tail_min;
        p.uniform_tail_max = o.uniform_tail_max;
        return std::make_shared<Tracker>(sensor, om_, p, params_.center_object_frame, params_.moving_average_update_rate);
    }

private:
    std::shared_ptr<ObjectModel> om_;
    std::shared_ptr<CameraData> cam_;
    Parameters params_;
};

}  // namespace dbot_amd
