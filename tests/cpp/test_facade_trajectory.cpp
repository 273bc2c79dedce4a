// C++ façade (include/eslam_gpu.hpp) on the GPU: the trajectory log through EmbodiedSlamFilter.
// enableTrajectory, then every update() leaves one entry; bestTrajectory() is
// trajectory(getBestParticleIndex()), its newest node the best particle's pose as getParticles()
// has it, its step ids increasing; smoothedTrajectory() has one estimate per entry with the same
// step ids, all particles counted and at most as many distinct ancestors as particles, fewer
// further back; clear and disable do what they say.  Run by tests/test_gpu_trajectory_facade.py.
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

// four feet under a body 0.18 m up
static eslam_ns::BodyContactState body_state()
{
    static const double feet[4][2] = {{0.25, 0.25}, {-0.25, 0.25}, {0.25, -0.25}, {-0.25, -0.25}};
    eslam_ns::BodyContactState bs;
    bs.points.resize(4);
    for (int i = 0; i < 4; ++i) {
        bs.points[i].position = eslam_ns::Vector3d(feet[i][0], feet[i][1], -0.18);
        bs.points[i].contact = 1.0f;
        bs.points[i].groupId = -1;
    }
    return bs;
}

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main()
{
    const eslam_ns::MlsGrid env = flat_grid(120);
    eslam_ns::Configuration ec;
    ec.particleCount = 1500;
    ec.minEffective = 1600;                       // above the count: every update resamples, lineages coalesce
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    try {
        ef.init(env, startPose, true);
        EXPECT(ef.trajectoryInfo().enabled == 0, "no log before it is enabled");
        ef.enableTrajectory(8);
        const int kSteps = 6;
        for (int k = 0; k < kSteps; ++k) {
            eslam_ns::Affine3d T = eslam_ns::Affine3d::Identity();
            T.translation() = eslam_ns::Vector3d(0.15 * (k + 1), 0.02 * k, 0.18);
            ef.update(T, body_state(), std::vector<eslam_ns::TerrainClassification>());
        }
        const eslam_trajectory_info info = ef.trajectoryInfo();
        EXPECT(info.enabled == 1 && info.capacity_steps == 8 && info.max_particles >= 1500, "the log's shape");
        EXPECT(info.entries == (uint64_t)kSteps && info.first_step == 0 && info.last_step == (uint64_t)kSteps - 1 && info.particles == 1500,
               "one entry per update");
        EXPECT(info.bytes >= 8ull * 1500 * 44, "44 bytes per particle and entry");

        const size_t best = ef.getBestParticleIndex();
        const std::vector<eslam_trajectory_pose> path = ef.bestTrajectory();
        EXPECT(path.size() == (size_t)kSteps, "a node per entry");
        const std::vector<eslam_trajectory_pose> again = ef.trajectory(best);
        EXPECT(path.size() == again.size() && std::memcmp(path.data(), again.data(), path.size() * sizeof(path[0])) == 0,
               "bestTrajectory() is trajectory(getBestParticleIndex())");
        bool rising = true, inside = true;
        for (size_t k = 0; k < path.size(); ++k) {
            if (path[k].step != (uint64_t)k) rising = false;
            if (path[k].slot >= path[k].particles || path[k].particles != 1500) inside = false;
        }
        EXPECT(rising, "step ids increase from the oldest entry");
        EXPECT(inside, "every node names a slot of its entry");
        if (!path.empty()) {
            const eslam_ns::PoseParticle& p = ef.getParticles()[best];
            const eslam_trajectory_pose& last = path.back();
            EXPECT(last.slot == best, "the newest node is the particle itself");
            EXPECT(same(last.x, p.position.x()) && same(last.y, p.position.y()) && same(last.yaw, p.orientation) && same(last.z, p.zPos) &&
                       same(last.zsigma, p.zSigma),
                   "... with the best particle's pose");
        }

        const std::vector<eslam_trajectory_estimate> est = ef.smoothedTrajectory();
        EXPECT(est.size() == (size_t)kSteps, "an estimate per entry");
        bool ok = true;
        for (size_t k = 0; k < est.size(); ++k) {
            if (est[k].step != (uint64_t)k || est[k].moments.particles_counted != 1500) ok = false;
            if (est[k].distinct_ancestors < 1 || est[k].distinct_ancestors > 1500) ok = false;
            if (k && est[k].distinct_ancestors < est[k - 1].distinct_ancestors) ok = false;
        }
        EXPECT(ok, "the estimates' step ids, counts and distinct ancestors");
        if (!est.empty()) {
            const eslam_pose_moments now = ef.poseMoments().m;
            EXPECT(std::memcmp(&est.back().moments, &now, sizeof(now)) == 0, "the newest entry's estimate is poseMoments()");
            EXPECT(est.front().distinct_ancestors < 1500, "resampling thinned the oldest entry's ancestors");
        }

        ef.clearTrajectory();
        EXPECT(ef.trajectoryInfo().enabled == 1 && ef.trajectoryInfo().entries == 0 && ef.bestTrajectory().empty(), "clear keeps it enabled");
        ef.disableTrajectory();
        EXPECT(ef.trajectoryInfo().enabled == 0, "disable");
        bool threw = false;
        try {
            ef.bestTrajectory();
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "not enabled") != nullptr;
        }
        EXPECT(threw, "a query without the log is an exception that says so");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("trajectory facade OK\n");
    return 0;
}
