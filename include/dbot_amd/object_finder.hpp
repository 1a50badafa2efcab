// object_finder.hpp -- C++ host-side mirror of the object finder (rbs_find_*, include/rbsensor_mi355x.h), in the style
// of rb_sensor_builder.hpp.
//
// It stands in for the FindObject service the reference's controller calls when a request has auto_detect set, and
// whose pose starts the tracker (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:143-167):
//     ObjectFinder finder(sensor, object_model, params);
//     ObjectFinder::Result r = finder.find(image);        // r.states[0] -> tracker->initialize({r.states[0]})
// States are in the caller's mesh frame (center_object_frame undone) with zero velocities; poses are R|t of the
// sensor's (centred) mesh frame, as the C-ABI returns them.
//
// SceneFinder below mirrors the scene finder (rbs_find_scene_*) the same way, for models of several objects.
//
// Header-only; link with -lrbsensor_mi355x.  No CPU fallback: without a device the sensor cannot be built.
#pragma once

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rb_sensor_builder.hpp"

namespace dbot_amd
{
class ObjectFinder
{
public:
    typedef FreeFloatingRigidBodiesState State;
    typedef std::vector<float> Obsrv;  // rows*cols depth image, metres, NaN = no reading

    /// rbs_find_params with the library's defaults (the optional object_finder: rosparam mapping overrides fields).
    struct Parameters : rbs_find_params {
        Parameters() { rbs_find_default_params(this); }
    };

    /// rbs_find_foreground with the library's defaults, enabled (step 1b: seeds from what stands in front of the dominant plane).
    struct Foreground : rbs_find_foreground {
        Foreground() { rbs_find_default_foreground(this); }
    };

    /// rbs_find_refinement with the library's defaults, enabled (step 6b: every survivor's search covariance adapts to its best children).
    struct Refinement : rbs_find_refinement {
        Refinement() { rbs_find_default_refinement(this); }
    };

    /// rbs_find_gate with the two rules' defaults, enabled (steps 4b, 5 and 7: the confirmed poses first).
    struct Gate : rbs_find_gate {
        Gate() { rbs_find_default_gate(this); }
    };

    /// The last find's evidence of one stage (rbs_find_get_evidence): records [n][10], classes [n] (0: confirmed).
    struct Evidence {
        std::vector<int32_t> records, classes;
    };

    /// The last find's dominant plane, 1 / z = a u + b v + c over the coarse pixels (rbs_find_get_plane).
    struct Plane {
        bool accepted = false;
        Real a = 0, b = 0, c = 0;
        long count = 0, n_valid = 0, trial = 0, masked = 0;
    };

    struct Result {
        bool found = false;
        std::vector<State> states;       // best first
        std::vector<Real> poses;         // [K][12]
        std::vector<Real> scores;        // [K]
    };

    ObjectFinder(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om, const Parameters& p = Parameters())
        : sensor_(sensor), om_(om), k_(p.n_survivors)
    {
        if (rbs_find_create(sensor_->handle(), &p, &f_) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder: ") + rbs_last_error(sensor_->handle()));
    }
    ~ObjectFinder() { rbs_find_destroy(f_); }
    ObjectFinder(const ObjectFinder&) = delete;
    ObjectFinder& operator=(const ObjectFinder&) = delete;

    /// One find on `image` (the sensor's resolution); an empty image: the sensor's current observation.
    Result find(const Obsrv& image = Obsrv())
    {
        Result r;
        r.poses.assign(12 * static_cast<size_t>(k_), 0.0);
        r.scores.assign(static_cast<size_t>(k_), 0.0);
        int32_t n = 0, found = 0;
        if (rbs_find_run(f_, image.empty() ? nullptr : image.data(), k_, r.poses.data(), r.scores.data(), &n, &found) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::find: ") + rbs_find_last_error(f_));
        r.found = found != 0;
        r.poses.resize(12 * static_cast<size_t>(n));
        r.scores.resize(static_cast<size_t>(n));
        const Real* c = om_->centers().data();
        for (int i = 0; i < n; ++i) {
            const Real* P = r.poses.data() + 12 * static_cast<size_t>(i);
            State s(1);
            for (int k = 0; k < 3; ++k) s.position(0)[k] = P[9 + k] - (P[3 * k] * c[0] + P[3 * k + 1] * c[1] + P[3 * k + 2] * c[2]);
            rotation_vector(P, s.euler_vector(0));
            r.states.push_back(s);
        }
        return r;
    }

    /// Step 1b for the finds from the next one on; nullptr (or enabled == 0): off.  Bad values throw, the previous setting stays.
    void set_foreground(const rbs_find_foreground* g)
    {
        if (rbs_find_set_foreground(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::set_foreground: ") + rbs_find_last_error(f_));
    }

    /// Step 6b for the finds from the next one on; nullptr (or enabled == 0): off, step 6's fixed schedule.  Bad values throw,
    /// the previous setting stays.
    void set_refinement(const rbs_find_refinement* g)
    {
        if (rbs_find_set_refinement(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::set_refinement: ") + rbs_find_last_error(f_));
    }

    /// The gate for the finds from the next one on; nullptr (or enabled == 0): off.  Bad values throw, the previous setting stays.
    void set_gate(const rbs_find_gate* g)
    {
        if (rbs_find_set_gate(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::set_gate: ") + rbs_find_last_error(f_));
    }

    /// The last find's evidence of RBS_FIND_COARSE, _CANDIDATES, _SURVIVORS or _RESULT, in that stage's order; the gate only.
    Evidence evidence(int stage)
    {
        int64_t n = 0;
        if (rbs_find_get_evidence(f_, stage, nullptr, nullptr, &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::evidence: ") + rbs_find_last_error(f_));
        Evidence e;
        e.records.assign(10 * static_cast<size_t>(n), 0);
        e.classes.assign(static_cast<size_t>(n), 0);
        if (rbs_find_get_evidence(f_, stage, e.records.data(), e.classes.data(), &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::evidence: ") + rbs_find_last_error(f_));
        return e;
    }

    /// The last find's covariances entering `round` (round == rounds: the final ones), [survivors][36] row-major; step 6b only.
    std::vector<Real> covariance(int round)
    {
        int64_t n = 0;
        if (rbs_find_get_covariance(f_, round, nullptr, &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::covariance: ") + rbs_find_last_error(f_));
        std::vector<Real> out(36 * static_cast<size_t>(n));
        if (rbs_find_get_covariance(f_, round, out.data(), &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::covariance: ") + rbs_find_last_error(f_));
        return out;
    }

    Plane plane()
    {
        double o[8];
        if (rbs_find_get_plane(f_, o) != RBS_OK) throw std::runtime_error(std::string("ObjectFinder::plane: ") + rbs_find_last_error(f_));
        Plane p;
        p.accepted = o[0] != 0.0;
        p.a = o[1]; p.b = o[2]; p.c = o[3];
        p.count = static_cast<long>(o[4]); p.n_valid = static_cast<long>(o[5]);
        p.trial = static_cast<long>(o[6]); p.masked = static_cast<long>(o[7]);
        return p;
    }

    /// The last find's seeding frame at the coarse resolution (the stage off: the coarse frame).
    std::vector<float> seed_frame()
    {
        int64_t n = 0;
        if (rbs_find_get_seed_frame(f_, nullptr, &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::seed_frame: ") + rbs_find_last_error(f_));
        std::vector<float> out(static_cast<size_t>(n));
        if (rbs_find_get_seed_frame(f_, out.data(), &n) != RBS_OK)
            throw std::runtime_error(std::string("ObjectFinder::seed_frame: ") + rbs_find_last_error(f_));
        return out;
    }

    rbs_find* handle() { return f_; }

private:
    friend class SceneFinder;   // (rotation_vector)
    /// row-major rotation matrix -> rotation vector (atan2 form, as dbot_ros_amd.pose.matrix_to_rotvec)
    static void rotation_vector(const Real* R, Real* rv)
    {
        const Real s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
        const Real sn = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
        const Real cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
        const Real angle = std::atan2(sn, cs);
        if (sn > 1e-8) {
            for (int k = 0; k < 3; ++k) rv[k] = s[k] * (angle / sn);
            return;
        }
        if (cs > 0.0) {
            for (int k = 0; k < 3; ++k) rv[k] = s[k];
            return;
        }
        Real d[3];
        for (int k = 0; k < 3; ++k) d[k] = std::sqrt(std::fmax((R[4 * k] + 1.0) * 0.5, 0.0));
        const int i = d[0] >= d[1] ? (d[0] >= d[2] ? 0 : 2) : (d[1] >= d[2] ? 1 : 2);
        Real a[3];
        for (int k = 0; k < 3; ++k) a[k] = (R[3 * k + i] + (k == i ? 1.0 : 0.0)) / (2.0 * d[i]);
        const Real an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 3; ++k) rv[k] = a[k] / an * angle;
    }

    std::shared_ptr<RbSensor<State>> sensor_;
    std::shared_ptr<ObjectModel> om_;
    int k_;
    rbs_find* f_ = nullptr;
};

/// The scene finder (rbs_find_scene_*): every body of a model of several from one depth frame.
///     SceneFinder finder(sensor, object_model, find_params, scene_params);
///     SceneFinder::Result r = finder.find(image);          // r.all_found() -> tracker->initialize({r.state})
/// `search` names the bodies to place (bit b = body b; 0: all); the poses of the others are given, [B][12] in the sensor's
/// mesh frames, and come back bit for bit.
class SceneFinder
{
public:
    typedef ObjectFinder::State State;
    typedef ObjectFinder::Obsrv Obsrv;

    /// rbs_find_scene_params with the library's defaults (the optional object_finder/scene: rosparam mapping overrides fields).
    struct Parameters : rbs_find_scene_params {
        Parameters() { rbs_find_scene_default_params(this); }
    };

    struct Result {
        uint32_t searched = 0, found = 0;   // bit b: body b was searched / has a pose that passed min_score
        State state = State(0);             // all bodies, the caller's mesh frames (valid when every body has a pose)
        std::vector<Real> poses;            // [B][12]; NaN: a searched body without a pose
        std::vector<Real> scores;           // [B] on each body's residual frame; NaN: given, or no pose
        Real joint_score = 0;               // NaN: a body has no pose
        bool all_found() const { return searched != 0 && (found & searched) == searched; }
    };

    SceneFinder(const std::shared_ptr<RbSensor<State>>& sensor, const std::shared_ptr<ObjectModel>& om,
                const ObjectFinder::Parameters& p = ObjectFinder::Parameters(), const Parameters& sp = Parameters())
        : sensor_(sensor), om_(om), parts_(om->count_parts())
    {
        if (rbs_find_scene_create(sensor_->handle(), &p, &sp, &f_) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder: ") + rbs_last_error(sensor_->handle()));
    }
    ~SceneFinder() { rbs_find_scene_destroy(f_); }
    SceneFinder(const SceneFinder&) = delete;
    SceneFinder& operator=(const SceneFinder&) = delete;

    int parts() const { return parts_; }

    /// One scene find on `image` (the sensor's resolution; empty: the sensor's current observation).
    Result find(const Obsrv& image = Obsrv(), uint32_t search = 0, const std::vector<Real>& given_poses = std::vector<Real>())
    {
        const size_t B = static_cast<size_t>(parts_);
        Result r;
        r.searched = search ? search : (parts_ >= 32 ? 0xFFFFFFFFu : (1u << parts_) - 1u);
        if (!given_poses.empty() && given_poses.size() != 12 * B) throw std::invalid_argument("SceneFinder::find: given_poses is not [B][12]");
        r.poses.assign(12 * B, 0.0);
        r.scores.assign(B, 0.0);
        if (rbs_find_scene_run(f_, image.empty() ? nullptr : image.data(), r.searched, given_poses.empty() ? nullptr : given_poses.data(),
                               r.poses.data(), r.scores.data(), &r.found, &r.joint_score) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::find: ") + rbs_find_scene_last_error(f_));
        const Real* c = om_->centers().data();
        r.state = State(parts_);
        for (size_t b = 0; b < B; ++b) {
            const Real* P = r.poses.data() + 12 * b;
            for (int k = 0; k < 3; ++k)
                r.state.position(b)[k] = P[9 + k] - (P[3 * k] * c[3 * b] + P[3 * k + 1] * c[3 * b + 1] + P[3 * k + 2] * c[3 * b + 2]);
            ObjectFinder::rotation_vector(P, r.state.euler_vector(b));
        }
        return r;
    }

    /// Steps 1b / 6b of every body's find; nullptr (or enabled == 0): off.  Bad values throw, the previous setting stays.
    void set_foreground(const rbs_find_foreground* g)
    {
        if (rbs_find_scene_set_foreground(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::set_foreground: ") + rbs_find_scene_last_error(f_));
    }
    void set_refinement(const rbs_find_refinement* g)
    {
        if (rbs_find_scene_set_refinement(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::set_refinement: ") + rbs_find_scene_last_error(f_));
    }
    /// The gate of every body's find (ObjectFinder::Gate); with require_confirmed a body without a confirmed pose is not placed.
    void set_gate(const rbs_find_gate* g)
    {
        if (rbs_find_scene_set_gate(f_, g) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::set_gate: ") + rbs_find_scene_last_error(f_));
    }

    /// The last scene find's S1: the searched bodies in the order they were taken.
    std::vector<int> order()
    {
        int32_t o[32], n = 0;
        if (rbs_find_scene_get_order(f_, o, &n, nullptr) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::order: ") + rbs_find_scene_last_error(f_));
        return std::vector<int>(o, o + n);
    }

    /// The residual frame searched body `body` was found on (rows x cols: the sensor's resolution).
    std::vector<float> residual(int body, int rows, int cols)
    {
        std::vector<float> out(static_cast<size_t>(rows) * static_cast<size_t>(cols));
        if (rbs_find_scene_get_residual(f_, body, out.data()) != RBS_OK)
            throw std::runtime_error(std::string("SceneFinder::residual: ") + rbs_find_scene_last_error(f_));
        return out;
    }

    rbs_find_scene* handle() { return f_; }

private:
    std::shared_ptr<RbSensor<State>> sensor_;
    std::shared_ptr<ObjectModel> om_;
    int parts_;
    rbs_find_scene* f_ = nullptr;
};

}  // namespace dbot_amd
