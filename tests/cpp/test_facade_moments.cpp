// C++ façade (include/eslam_gpu.hpp) on the GPU: PoseEstimator::poseMoments and
// EmbodiedSlamFilter::poseMoments return what eslam_gpu_pose_moments returns, gated and ungated;
// PoseMoments::pose() composes the mean as getCentroid composes its pose (the yaw about Z, then
// zCompensatedOrientation); PoseGate's constructor from a mixture component fills eslam_pose_gate
// as documented (mean, covariance, chi2 = sigmas^2).  Run by tests/test_gpu_pose_moments_facade.py.
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

// four feet under a body at the origin, 0.18 m up
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

static bool same(const eslam_pose_moments& a, const eslam_pose_moments& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main()
{
    const eslam_ns::MlsGrid env = flat_grid(120);
    eslam_ns::Configuration ec;
    ec.particleCount = 1500;
    ec.minEffective = 50;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    try {
        ef.init(env, startPose, true);
        eslam_ns::PoseEstimator& pe = ef.estimator();
        // one step with the body rolled and yawed: zCompensatedOrientation is the roll
        const eslam_ns::Quaterniond roll(std::cos(0.05), std::sin(0.05), 0, 0), yaw(std::cos(0.2), 0, 0, std::sin(0.2));
        eslam_ns::Affine3d T = eslam_ns::Affine3d::Identity();
        T.linear() = (yaw * roll).toRotationMatrix();
        T.translation() = eslam_ns::Vector3d(0, 0, 0.18);
        ef.update(T, body_state(), std::vector<eslam_ns::TerrainClassification>());
        // three groups through getParticles(), one yaw for all: the edit is what gets summed
        std::vector<eslam_ns::PoseParticle>& v = pe.getParticles();
        for (size_t i = 0; i < v.size(); ++i) {
            const int grp = (int)(i % 3);
            v[i].position = eslam_ns::Vector2d(0.05 * std::sin((double)i) + 4.0 * grp, 0.05 * std::cos((double)i) - 1.0 * grp);
            v[i].orientation = 0.7;
            v[i].zPos = 0.18 + 0.001 * (double)(i % 5);
            v[i].zSigma = 0.01;
            v[i].weight = 1e-3 * (1.0 + (double)(i % 7)) * (grp == 1 ? 3.0 : 1.0);
        }
        // ungated: the façade, both classes, against the C ABI
        const eslam_ns::PoseMoments all = pe.poseMoments();
        eslam_pose_moments c;
        EXPECT(eslam_gpu_pose_moments(pe.handle(), nullptr, &c) == ESLAM_OK, "the C ABI's call");
        EXPECT(same(all.m, c), "poseMoments() equals eslam_gpu_pose_moments");
        EXPECT(same(ef.poseMoments().m, c), "EmbodiedSlamFilter::poseMoments() too");
        EXPECT(all.particlesCounted() == 1500 && all.particlesGatedOut() == 0 && all.particlesSkipped() == 0, "the counts");
        EXPECT(same(all.position().x(), c.mean[0]) && same(all.yaw(), c.mean[3]) && same(all.cov(0, 3), c.cov[3]) &&
                   same(all.cov(3, 0), c.cov[12]) && same(all.zWithin(), c.z_within) && same(all.yawResultant(), c.yaw_resultant) &&
                   same(all.effective(), c.effective) && same(all.weightShare(), c.weight_share),
               "the accessors read the struct");
        EXPECT(all.weightShare() == 1.0 && std::fabs(all.yaw() - 0.7) < 1e-12 && std::fabs(all.zWithin() - 1e-4) < 1e-15, "the values");
        // the cluster recipe: the mixture, its heaviest component, the gate around it
        const eslam_ns::GaussianMixture2D g3 = pe.fitGmm();
        EXPECT(g3.params.size() == 3, "three components");
        size_t heavy = 0;
        for (size_t k = 1; k < g3.params.size(); ++k)
            if (g3.params[k].weight > g3.params[heavy].weight) heavy = k;
        EXPECT(heavy == 1, "the middle group is the heaviest");
        const eslam_ns::PoseGate gate(g3.params[heavy], 3.0);
        const eslam_pose_gate cg = gate.c();
        const eslam_ns::Gaussian2D& d = g3.params[heavy].dist;
        EXPECT(same(cg.centre[0], d.mean.x()) && same(cg.centre[1], d.mean.y()) && same(cg.cov[0], d.cov(0, 0)) &&
                   same(cg.cov[1], d.cov(0, 1)) && same(cg.cov[2], d.cov(1, 1)) && cg.chi2 == 9.0,
               "PoseGate(component, sigmas): the component's mean and covariance, chi2 = sigmas^2");
        const eslam_ns::PoseMoments one = ef.poseMoments(&gate);
        EXPECT(eslam_gpu_pose_moments(pe.handle(), &cg, &c) == ESLAM_OK, "the C ABI's gated call");
        EXPECT(same(one.m, c), "poseMoments(gate) equals eslam_gpu_pose_moments");
        EXPECT(one.particlesCounted() == 500 && one.particlesGatedOut() == 1000, "the gate holds the middle group");
        EXPECT(std::fabs(one.position().x() - 4.0) < 0.01 && std::fabs(one.position().y() + 1.0) < 0.01, "... at its place");
        EXPECT(one.weightShare() > 0.55 && one.weightShare() < 0.65, "... with 3/5 of the weight");
        // pose(): the yaw about Z, then zCompensatedOrientation
        double zc[4];
        EXPECT(eslam_gpu_get_z_compensated_orientation(pe.handle(), zc) == ESLAM_OK, "the C ABI's zCompensatedOrientation");
        EXPECT(std::fabs(zc[1] - std::sin(0.05)) < 1e-12 && std::fabs(zc[3]) < 1e-12, "... is the step's roll, yaw removed");
        const eslam_ns::Quaterniond& q = all.zCompensatedOrientation;
        EXPECT(same(q.w(), zc[0]) && same(q.x(), zc[1]) && same(q.y(), zc[2]) && same(q.z(), zc[3]), "... carried by PoseMoments");
        const eslam_ns::Pose p = all.pose();
        const eslam_ns::Quaterniond want = eslam_ns::Quaterniond(std::cos(0.5 * all.yaw()), 0, 0, std::sin(0.5 * all.yaw())) * q;
        EXPECT(same(p.orientation.w(), want.w()) && same(p.orientation.x(), want.x()) && same(p.orientation.y(), want.y()) &&
                   same(p.orientation.z(), want.z()) && same(p.position.z(), all.m.mean[2]),
               "pose(): yaw about Z, then zCompensatedOrientation");
        // ... as getCentroid composes its pose: with one yaw for all its linear mean is the circular one
        const eslam_ns::Pose cen = pe.getCentroid();          // normalises the weights: last
        EXPECT(std::fabs(p.position.x() - cen.position.x()) < 1e-12 && std::fabs(p.position.y() - cen.position.y()) < 1e-12 &&
                   std::fabs(p.position.z() - cen.position.z()) < 1e-12,
               "pose() is at getCentroid's position");
        EXPECT(std::fabs(p.orientation.w() - cen.orientation.w()) < 1e-12 && std::fabs(p.orientation.x() - cen.orientation.x()) < 1e-12 &&
                   std::fabs(p.orientation.y() - cen.orientation.y()) < 1e-12 && std::fabs(p.orientation.z() - cen.orientation.z()) < 1e-12,
               "pose() has getCentroid's orientation");
        // a refused gate is an exception that says so, and the filter stays usable
        bool threw = false;
        try {
            eslam_ns::PoseGate bad;
            bad.cov(0, 1) = 2.0;
            pe.poseMoments(&bad);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "gate") != nullptr;
        }
        EXPECT(threw, "a gate that is not positive definite is an exception that says so");
        EXPECT(pe.poseMoments().particlesCounted() == 1500, "... and the filter is still usable");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("moments facade OK\n");
    return 0;
}
