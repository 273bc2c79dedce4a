// C++ façade (include/eslam_gpu.hpp) on the GPU: PoseEstimator::resample_stratified(n) and
// resample_multinomial(n) with the reference's signatures (src/ParticleFilter.hpp:85-148):
// getParticles() has the new size afterwards, the multinomial weights are 1 / the old size, an
// edit made through getParticles() before the call is resampled, and update() still runs at
// the new count.  Run by tests/test_gpu_resample_facade.py.
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

int main()
{
    const eslam_ns::MlsGrid env = flat_grid(120);
    eslam_ns::Configuration ec;
    ec.particleCount = 1500;
    ec.minEffective = 50;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;

    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    ef.init(env, startPose, true);
    eslam_ns::PoseEstimator& pe = ef.estimator();
    double x = 0, yaw = 0;
    auto advance = [&]() {
        yaw += 0.002;
        x += 0.02;
        return ef.update(body_pose(x, 0, yaw), body_state(x, 0, yaw), ltc);
    };
    try {
        for (int s = 0; s < 3; ++s) EXPECT(advance(), "update before the resamples");
        EXPECT(pe.getParticles().size() == 1500, "the initial size");

        // shrink, stratified: the weights are carried (they were normalised by the update)
        pe.resample_stratified(400);
        EXPECT(pe.size() == 400 && pe.getParticles().size() == 400, "resample_stratified(400): 400 particles");
        EXPECT(pe.lastResample().n_before == 1500 && pe.lastResample().n_after == 400, "the stratified call's info");
        double sum = 0;
        for (const auto& p : pe.getParticles()) sum += p.weight;
        EXPECT(sum > 0.0 && sum < 1.0, "carried weights: 400 of 1500 normalised ones");
        EXPECT(advance(), "update at 400 particles");
        EXPECT(pe.getParticles().size() == 400, "still 400 after an update");

        // grow, multinomial: every weight is 1 / the old size; an edit made through getParticles()
        // just before is what gets resampled (all the mass on particle 7)
        std::vector<eslam_ns::PoseParticle>& v = pe.getParticles();
        for (auto& p : v) p.weight = 0.0;
        v[7].weight = 1.0;
        const eslam_ns::PoseParticle seven = v[7];
        const size_t old_size = v.size();
        pe.resample_multinomial(2500);
        const std::vector<eslam_ns::PoseParticle>& g = pe.getParticles();
        EXPECT(g.size() == 2500 && pe.size() == 2500, "resample_multinomial(2500): 2500 particles (the weights sum to 1)");
        EXPECT(pe.lastResample().n_before == old_size && pe.lastResample().dropped == 0, "the multinomial call's info");
        size_t bad_w = 0, bad_p = 0;
        for (const auto& p : g) {
            if (p.weight != 1.0 / (double)old_size) ++bad_w;
            if (std::memcmp(&p.position, &seven.position, sizeof(p.position)) || p.orientation != seven.orientation ||
                p.zPos != seven.zPos)
                ++bad_p;
        }
        EXPECT(bad_w == 0, "multinomial weights are 1.0 / old_size");
        EXPECT(bad_p == 0, "every copy is the particle that held the mass");
        EXPECT(advance(), "update at 2500 particles");
        EXPECT(pe.getParticles().size() == 2500, "still 2500 after an update");
        const eslam_ns::Affine3d c = ef.getCentroid();
        EXPECT(std::isfinite(c.translation().x()), "a centroid at the new count");

        // samples == n, and the limits
        pe.resample_stratified(2500);
        EXPECT(pe.getParticles().size() == 2500, "resample_stratified(n) keeps the size");
        bool threw = false;
        try {
            pe.resample_stratified(0);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        EXPECT(threw && pe.size() == 2500, "samples == 0 is an exception and changes nothing");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("resample facade OK\n");
    return 0;
}
