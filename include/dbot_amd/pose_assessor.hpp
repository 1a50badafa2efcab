// pose_assessor.hpp -- C++ host-side mirror of the pose assessor (rbs_assess_*, include/rbsensor_mi355x.h), in the style
// of object_finder.hpp.
//
// It stands in for the person the reference's controller puts between FindObject and RunObjectTracker
// (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:180-195):
//     PoseAssessor assessor(sensor, object_model);
//     PoseAssessor::Result a = assessor.assess(r.poses, image);   // r: ObjectFinder::Result
//     if (a.first_supported() >= 0) tracker->initialize({r.states[a.first_supported()]});
// Poses are R|t of the sensor's (centred) mesh frame, [n][parts][12], as the C-ABI takes them.
//
// Header-only; link with -lrbsensor_mi355x.  No CPU fallback: without a device the sensor cannot be built.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rb_sensor_builder.hpp"

namespace dbot_amd
{
class PoseAssessor
{
public:
    typedef FreeFloatingRigidBodiesState State;
    typedef std::vector<float> Obsrv;  // rows*cols depth image, metres, NaN = no reading

    /// rbs_assess_params with the library's defaults.
    struct Parameters : rbs_assess_params {
        Parameters() { rbs_assess_default_params(this); }
    };

    struct Result {
        int n = 0, parts = 0;
        std::vector<rbs_assess_body> bodies;   // [n][parts]
        const rbs_assess_body& at(int k, int b) const { return bodies[static_cast<size_t>(k) * parts + b]; }
        /// Every body of pose k reads RBS_ASSESS_SUPPORTED.
        bool supported(int k) const
        {
            for (int b = 0; b < parts; ++b)
                if (at(k, b).verdict != RBS_ASSESS_SUPPORTED) return false;
            return true;
        }
        /// The first such pose, -1: none.
        int first_supported() const
        {
            for (int k = 0; k < n; ++k)
                if (supported(k)) return k;
            return -1;
        }
    };

    PoseAssessor(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om, const Parameters& p = Parameters())
        : sensor_(sensor), parts_(om->count_parts()), p_(p)
    {
        rbs_assess_body probe = rbs_assess_body();
        int32_t v = 0;
        if (rbs_assess_verdict(&p_, &probe, &v) != RBS_OK) throw std::invalid_argument("PoseAssessor: bad parameters");
    }

    /// n = poses.size() / (12 parts) poses judged against `image` (the sensor's resolution); an empty image: the
    /// sensor's current observation.
    Result assess(const std::vector<Real>& poses, const Obsrv& image = Obsrv())
    {
        Result r;
        r.parts = parts_;
        r.n = static_cast<int>(poses.size() / (12 * static_cast<size_t>(parts_)));
        r.bodies.assign(static_cast<size_t>(r.n > 0 ? r.n : 1) * parts_, rbs_assess_body());
        if (rbs_assess_poses(sensor_->handle(), &p_, image.empty() ? nullptr : image.data(), poses.data(), r.n, r.bodies.data()) != RBS_OK)
            throw std::runtime_error(std::string("PoseAssessor::assess: ") + rbs_last_error(sensor_->handle()));
        r.bodies.resize(static_cast<size_t>(r.n) * parts_);
        return r;
    }

    /// The rule's verdict of one record's counts (host only).
    int verdict(const rbs_assess_body& body) const
    {
        int32_t v = 0;
        if (rbs_assess_verdict(&p_, &body, &v) != RBS_OK) throw std::invalid_argument("PoseAssessor::verdict: bad parameters");
        return v;
    }

    /// Depth image of body b of the last call's pose k, rendered alone (+inf where it covers nothing); for the tests.
    std::vector<float> plane(int k, int b, size_t pixels)
    {
        std::vector<float> out(pixels);
        if (rbs_assess_get_plane(sensor_->handle(), k, b, out.data()) != RBS_OK)
            throw std::runtime_error(std::string("PoseAssessor::plane: ") + rbs_last_error(sensor_->handle()));
        return out;
    }

    /// Device ms of the last call: render, count.
    void kernel_ms(float out[2])
    {
        if (rbs_assess_kernel_ms(sensor_->handle(), out) != RBS_OK)
            throw std::runtime_error(std::string("PoseAssessor::kernel_ms: ") + rbs_last_error(sensor_->handle()));
    }

    const Parameters& params() const { return p_; }

private:
    std::shared_ptr<RbSensor<State>> sensor_;
    int parts_;
    Parameters p_;
};

}  // namespace dbot_amd
