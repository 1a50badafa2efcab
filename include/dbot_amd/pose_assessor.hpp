// pose_assessor.hpp -- C++ host-side mirror of the pose assessor (rbs_assess_*, include/rbsensor_mi355x.h), in the style
// of object_finder.hpp.
//
// It stands in for the person the reference's controller puts between FindObject and RunObjectTracker
// (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:180-195):
//     PoseAssessor assessor(sensor, object_model);
//     PoseAssessor::Result a = assessor.assess(r.poses, image);   // r: ObjectFinder::Result
//     if (a.first_supported() >= 0) tracker->initialize({r.states[a.first_supported()]});
// Poses are R|t of the sensor's (centred) mesh frame, [n][parts][12], as the C-ABI takes them.
// The contour rule (rbs_contour_*) is opt-in: construct with ContourParameters, or set_contour(), and assess() judges the
// silhouette in the same call; Result::confirmed(k) then asks for SUPPORTED and RBS_CONTOUR_PRESENT.
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

    /// rbs_contour_params with the library's defaults.
    struct ContourParameters : rbs_contour_params {
        ContourParameters() { rbs_contour_default_params(this); }
    };

    struct Result {
        int n = 0, parts = 0;
        std::vector<rbs_assess_body> bodies;   // [n][parts]
        std::vector<rbs_contour_body> contour;  // [n][parts]; empty: the contour rule is off
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
        const rbs_contour_body& contour_at(int k, int b) const { return contour[static_cast<size_t>(k) * parts + b]; }
        /// supported(k), and with the contour rule on every body's silhouette reads RBS_CONTOUR_PRESENT.
        bool confirmed(int k) const
        {
            if (!supported(k)) return false;
            if (contour.empty()) return true;
            for (int b = 0; b < parts; ++b)
                if (contour_at(k, b).verdict != RBS_CONTOUR_PRESENT) return false;
            return true;
        }
        /// The first such pose, -1: none.
        int first_confirmed() const
        {
            for (int k = 0; k < n; ++k)
                if (confirmed(k)) return k;
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

    /// The same with the contour rule on.
    PoseAssessor(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om, const Parameters& p,
                 const ContourParameters& c)
        : PoseAssessor(sensor, om, p)
    {
        set_contour(c);
    }

    /// Switches the contour rule on (rbs_contour_poses from now on) ...
    void set_contour(const ContourParameters& c)
    {
        rbs_contour_body probe = rbs_contour_body();
        int32_t v = 0;
        if (rbs_contour_verdict(&c, &probe, &v) != RBS_OK) throw std::invalid_argument("PoseAssessor: bad contour parameters");
        c_ = c;
        contour_ = true;
    }
    /// ... and off again.
    void clear_contour() { contour_ = false; }
    bool contour() const { return contour_; }

    /// n = poses.size() / (12 parts) poses judged against `image` (the sensor's resolution); an empty image: the
    /// sensor's current observation.
    Result assess(const std::vector<Real>& poses, const Obsrv& image = Obsrv())
    {
        Result r;
        r.parts = parts_;
        r.n = static_cast<int>(poses.size() / (12 * static_cast<size_t>(parts_)));
        r.bodies.assign(static_cast<size_t>(r.n > 0 ? r.n : 1) * parts_, rbs_assess_body());
        const float* frame = image.empty() ? nullptr : image.data();
        int32_t rc;
        if (contour_) {
            r.contour.assign(r.bodies.size(), rbs_contour_body());
            rc = rbs_contour_poses(sensor_->handle(), &p_, &c_, frame, poses.data(), r.n, r.bodies.data(), r.contour.data());
        } else {
            rc = rbs_assess_poses(sensor_->handle(), &p_, frame, poses.data(), r.n, r.bodies.data());
        }
        if (rc != RBS_OK) throw std::runtime_error(std::string("PoseAssessor::assess: ") + rbs_last_error(sensor_->handle()));
        r.bodies.resize(static_cast<size_t>(r.n) * parts_);
        if (contour_) r.contour.resize(r.bodies.size());
        return r;
    }

    /// The rule's verdict of one record's counts (host only).
    int verdict(const rbs_assess_body& body) const
    {
        int32_t v = 0;
        if (rbs_assess_verdict(&p_, &body, &v) != RBS_OK) throw std::invalid_argument("PoseAssessor::verdict: bad parameters");
        return v;
    }

    /// The contour rule's verdict of one record's counts (host only); the library's defaults while the rule is off.
    int contour_verdict(const rbs_contour_body& body) const
    {
        int32_t v = 0;
        if (rbs_contour_verdict(contour_ ? &c_ : nullptr, &body, &v) != RBS_OK)
            throw std::invalid_argument("PoseAssessor::contour_verdict: bad parameters");
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

    /// Device ms of the last call with the contour rule on: render, count, contour.
    void contour_kernel_ms(float out[3])
    {
        if (rbs_contour_kernel_ms(sensor_->handle(), out) != RBS_OK)
            throw std::runtime_error(std::string("PoseAssessor::contour_kernel_ms: ") + rbs_last_error(sensor_->handle()));
    }

    const Parameters& params() const { return p_; }
    const ContourParameters& contour_params() const { return c_; }

private:
    std::shared_ptr<RbSensor<State>> sensor_;
    int parts_;
    Parameters p_;
    ContourParameters c_;
    bool contour_ = false;
};

}  // namespace dbot_amd
