// pose_refiner.hpp -- C++ host-side mirror of the pose refiner (rbs_refine_*, include/rbsensor_mi355x.h), in the style of
// pose_assessor.hpp.
//
// Between a pose that is roughly right and the tracker (or the assessor) that starts from it:
//     PoseRefiner refiner(sensor, object_model);
//     PoseRefiner::Result f = refiner.refine(r.poses, image);     // r: ObjectFinder::Result
//     PoseAssessor::Result a = assessor.assess(f.poses, image);
// Poses are R|t of the sensor's (centred) mesh frame, [n][parts][12], as the C-ABI takes them.  Every default of
// Parameters is an unmeasured starting value (the C header says so field by field).
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
class PoseRefiner
{
public:
    typedef FreeFloatingRigidBodiesState State;
    typedef std::vector<float> Obsrv;  // rows*cols depth image, metres, NaN = no reading

    /// rbs_refine_params with the library's defaults.
    struct Parameters : rbs_refine_params {
        Parameters() { rbs_refine_default_params(this); }
    };

    struct Result {
        int n = 0, parts = 0;
        std::vector<Real> poses;               // [n][parts][12], refined
        std::vector<rbs_refine_body> bodies;   // [n][parts]
        const rbs_refine_body& at(int k, int b) const { return bodies[static_cast<size_t>(k) * parts + b]; }
        /// Every body of pose k reads RBS_REFINE_CONVERGED.
        bool converged(int k) const
        {
            for (int b = 0; b < parts; ++b)
                if (at(k, b).status != RBS_REFINE_CONVERGED) return false;
            return true;
        }
    };

    PoseRefiner(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om, const Parameters& p = Parameters())
        : sensor_(sensor), parts_(om->count_parts()), p_(p)
    {
        if (rbs_refine_check_params(&p_) != RBS_OK) throw std::invalid_argument("PoseRefiner: bad parameters");
    }

    /// n = poses.size() / (12 parts) poses refined against `image` (the sensor's resolution); an empty image: the
    /// sensor's current observation.
    Result refine(const std::vector<Real>& poses, const Obsrv& image = Obsrv())
    {
        Result r;
        r.parts = parts_;
        r.n = static_cast<int>(poses.size() / (12 * static_cast<size_t>(parts_)));
        r.poses.assign(poses.size() ? poses.size() : 12, Real(0));
        r.bodies.assign(static_cast<size_t>(r.n > 0 ? r.n : 1) * parts_, rbs_refine_body());
        const int32_t rc = rbs_refine_poses(sensor_->handle(), &p_, image.empty() ? nullptr : image.data(), poses.data(), r.n,
                                            r.poses.data(), r.bodies.data());
        if (rc != RBS_OK) throw std::runtime_error(std::string("PoseRefiner::refine: ") + rbs_last_error(sensor_->handle()));
        r.poses.resize(poses.size());
        r.bodies.resize(static_cast<size_t>(r.n) * parts_);
        return r;
    }

    /// Iteration `it` of body b of the last call's pose k; for the tests.
    rbs_refine_history history(int k, int b, int it)
    {
        rbs_refine_history out = rbs_refine_history();
        if (rbs_refine_get_history(sensor_->handle(), k, b, it, &out) != RBS_OK)
            throw std::runtime_error(std::string("PoseRefiner::history: ") + rbs_last_error(sensor_->handle()));
        return out;
    }

    /// Device ms of the last call, summed over its iterations: render, accumulate, solve.
    void kernel_ms(float out[3])
    {
        if (rbs_refine_kernel_ms(sensor_->handle(), out) != RBS_OK)
            throw std::runtime_error(std::string("PoseRefiner::kernel_ms: ") + rbs_last_error(sensor_->handle()));
    }

    const Parameters& params() const { return p_; }

private:
    std::shared_ptr<RbSensor<State>> sensor_;
    int parts_;
    Parameters p_;
};

}  // namespace dbot_amd
