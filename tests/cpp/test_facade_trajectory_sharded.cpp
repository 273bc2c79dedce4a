// C++ façade (include/eslam_gpu.hpp) on the GPU: the trajectory log of a sharded estimator.  An
// EmbodiedSlamFilter whose estimator is shard 0 of 1 over the library's own RCCL communicator
// (PoseEstimator::setCommRccl) enables the log through eslam_gpu_trajectory_enable_sharded.
// Through updates, a resample to another count and more updates, its trajectoryInfo(),
// bestTrajectory() and smoothedTrajectory() must equal those of an unsharded filter given the
// same calls, byte for byte.  Run by tests/test_gpu_trajectory_sharded_facade.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "eslam_gpu.hpp"

static int fails = 0;
#define EXPECT(c, msg)                                         \
    do {                                                       \
        if (!(c)) { std::printf("FAIL: %s\n", msg); ++fails; } \
    } while (0)

namespace eslam_ns = eslam::gpu;

static eslam_ns::MlsGrid flat_grid(uint32_t W)
{
    eslam_ns::MlsGrid g;
    g.width = g.height = W;
    g.scaleX = g.scaleY = 0.1;
    g.offsetX = g.offsetY = -0.05 * W;
    g.cellStart.resize(W * W + 1);
    for (uint32_t i = 0; i <= W * W; ++i) g.cellStart[i] = i;
    g.mean.assign(W * W, 0.0f);
    g.stdev.assign(W * W, 0.05f);
    return g;
}

// four feet fixed in the world, seen from the body at (x, y, 0.18) with heading yaw
static eslam_ns::BodyContactState body_state(double x, double y, double yaw)
{
    static const double feet_w[4][2] = {{0.25, 0.0}, {-0.25, 0.0}, {0.25, -0.5}, {-0.25, -0.5}};
    eslam_ns::BodyContactState bs;
    bs.points.resize(4);
    const double c = std::cos(yaw), s = std::sin(yaw);
    for (int i = 0; i < 4; ++i) {
        const double dx = feet_w[i][0] - x, dy = feet_w[i][1] - y;
        bs.points[i].position = eslam_ns::Vector3d(c * dx + s * dy, -s * dx + c * dy, -0.18);
        bs.points[i].contact = 1.0f;
        bs.points[i].groupId = -1;
    }
    bs.time = x;
    return bs;
}

static eslam_ns::Affine3d body_pose(double x, double y, double yaw)
{
    eslam_ns::Affine3d T = eslam_ns::Affine3d::Identity();
    T.linear() = eslam_ns::Quaterniond(std::cos(yaw / 2), 0, 0, std::sin(yaw / 2)).toRotationMatrix();
    T.translation() = eslam_ns::Vector3d(x, y, 0.18);
    return T;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static bool same_log(eslam_ns::EmbodiedSlamFilter& s, eslam_ns::EmbodiedSlamFilter& u, size_t entries, const char* what)
{
    const eslam_trajectory_info is = s.trajectoryInfo(), iu = u.trajectoryInfo();
    bool ok = is.enabled == 1 && is.entries == entries && is.entries == iu.entries && is.first_step == iu.first_step &&
              is.last_step == iu.last_step && is.particles == iu.particles && is.capacity_steps == iu.capacity_steps;
    ok = ok && s.getBestParticleIndex() == u.getBestParticleIndex();
    const std::vector<eslam_trajectory_pose> ps = s.bestTrajectory(), pu = u.bestTrajectory();
    ok = ok && ps.size() == entries && same_bytes(ps, pu);
    ok = ok && same_bytes(s.trajectory(0), u.trajectory(0));
    const std::vector<eslam_trajectory_estimate> es = s.smoothedTrajectory(), eu = u.smoothedTrajectory();
    ok = ok && es.size() == entries && same_bytes(es, eu);
    if (!ok) std::printf("  (%s: entries %llu / %llu)\n", what, (unsigned long long)is.entries, (unsigned long long)iu.entries);
    return ok;
}

int main()
{
    const size_t N = 3000;
    const eslam_ns::MlsGrid env = flat_grid(120);
    eslam_ns::Configuration ec;
    ec.particleCount = N;
    ec.minEffective = N + 1;                       // every update resamples
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;
    try {
        // making the estimator a shard drops its particles, which are then initialised again; the
        // unsharded filter is given the same calls (a second initialisation draws other samples)
        eslam_ns::EmbodiedSlamFilter es(oc, ec), eu(oc, ec);
        es.init(env, startPose, true);
        es.estimator().setCommRccl(1, 0, eslam_ns::PoseEstimator::rcclUniqueId(), N, std::vector<uint64_t>{0, N});
        EXPECT(es.estimator().sharded(), "the estimator is sharded");
        const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};
        EXPECT(eslam_gpu_init_pose(es.estimator().handle(), p0, q0) == ESLAM_OK, "shard init");
        es.estimator().invalidate();
        eu.init(env, startPose, true);
        EXPECT(eslam_gpu_init_pose(eu.estimator().handle(), p0, q0) == ESLAM_OK, "second init");
        eu.estimator().invalidate();
        EXPECT(eslam_gpu_trajectory_enable(es.estimator().handle(), 4, 0) == ESLAM_ERR_UNSUPPORTED,
               "the plain C call still refuses a sharded filter");
        es.enableTrajectory(4, 4096);
        eu.enableTrajectory(4, 4096);
        EXPECT(es.trajectoryInfo().enabled == 1 && es.trajectoryInfo().max_particles == 4096, "enableTrajectory on the sharded estimator");
        double x = 0, yaw = 0;
        auto advance = [&]() {
            yaw += 0.002;
            x += 0.02;
            const bool a = es.update(body_pose(x, 0, yaw), body_state(x, 0, yaw), ltc);
            const bool b = eu.update(body_pose(x, 0, yaw), body_state(x, 0, yaw), ltc);
            return a && b;
        };
        for (int s = 0; s < 3; ++s) EXPECT(advance(), "updates");
        EXPECT(same_log(es, eu, 3, "three updates"), "after three updates: the sharded estimator's log == the plain one's");
        const std::vector<eslam_trajectory_estimate> sm = es.smoothedTrajectory();
        EXPECT(sm.size() == 3 && sm[0].distinct_ancestors < sm[1].distinct_ancestors && sm[1].distinct_ancestors < N &&
                   sm[2].distinct_ancestors == N,
               "the lineages coalesce going back: not identity maps");
        es.estimator().resample_multinomial(2500);
        eu.estimator().resample_multinomial(2500);
        EXPECT(same_log(es, eu, 3, "a composition"), "after a resample to another count (a composed link)");
        for (int s = 0; s < 2; ++s) EXPECT(advance(), "updates after the resample");
        EXPECT(same_log(es, eu, 4, "the ring wrapped"), "after the ring wrapped");
        bool threw = false;
        try {
            es.estimator().resample_stratified(4097);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        EXPECT(threw, "a resample beyond the log's max_particles is an exception");
        EXPECT(same_log(es, eu, 4, "after the refusal"), "... and changes nothing");
        es.clearTrajectory();
        eu.clearTrajectory();
        EXPECT(advance(), "an update after the clear");
        EXPECT(same_log(es, eu, 1, "cleared"), "after clearTrajectory and one update");
        es.disableTrajectory();
        EXPECT(es.trajectoryInfo().enabled == 0, "disableTrajectory");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    std::printf(fails ? "facade trajectory sharded: %d FAILED\n" : "facade trajectory sharded OK\n", fails);
    return fails ? 1 : 0;
}
