// C++ façade (include/eslam_gpu.hpp) on the GPU: resample_stratified(n) / resample_multinomial(n)
// on a sharded estimator.  An EmbodiedSlamFilter whose estimator is shard 0 of 1 over the
// library's own RCCL communicator (PoseEstimator::setCommRccl) takes the collectives
// eslam_gpu_resample_stratified_sharded / _multinomial_sharded there.  After resample_stratified(7001)
// (beyond the capacity) and resample_multinomial(129) it must hold the particles of an unsharded
// filter given the same calls, byte for byte, shardBounds() must be the canonical table of the
// new count, and updates must go on alike.  Run by tests/test_gpu_resample_sharded_facade.py.
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

static bool same_particles(eslam_ns::EmbodiedSlamFilter& a, eslam_ns::EmbodiedSlamFilter& b, size_t want)
{
    const std::vector<eslam_ns::PoseParticle>& pa = a.getParticles();
    const std::vector<eslam_ns::PoseParticle>& pb = b.getParticles();
    size_t diff = pa.size() != pb.size() || pa.size() != want;
    for (size_t i = 0; i < pa.size() && i < pb.size(); ++i)
        diff += std::memcmp(&pa[i].position.v[0], &pb[i].position.v[0], 8) || std::memcmp(&pa[i].position.v[1], &pb[i].position.v[1], 8) ||
                std::memcmp(&pa[i].orientation, &pb[i].orientation, 8) || std::memcmp(&pa[i].zPos, &pb[i].zPos, 8) ||
                std::memcmp(&pa[i].zSigma, &pb[i].zSigma, 8) || std::memcmp(&pa[i].weight, &pb[i].weight, 8) ||
                std::memcmp(&pa[i].mprob, &pb[i].mprob, 8) || pa[i].floating != pb[i].floating;
    return diff == 0;
}

int main()
{
    const size_t N = 3000;
    const eslam_ns::MlsGrid env = flat_grid(120);
    eslam_ns::Configuration ec;
    ec.particleCount = N;
    ec.minEffective = 50;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;
    const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};
    try {
        // making the estimator a shard drops its particles, which are then initialised again; the
        // unsharded filter is given the same calls (a second initialisation draws other samples)
        eslam_ns::EmbodiedSlamFilter es(oc, ec), eu(oc, ec);
        es.init(env, startPose, true);
        es.estimator().setCommRccl(1, 0, eslam_ns::PoseEstimator::rcclUniqueId(), N, std::vector<uint64_t>{0, N});
        EXPECT(es.estimator().sharded(), "the estimator is sharded");
        EXPECT(eslam_gpu_init_pose(es.estimator().handle(), p0, q0) == ESLAM_OK, "shard init");
        es.estimator().invalidate();
        eu.init(env, startPose, true);
        EXPECT(eslam_gpu_init_pose(eu.estimator().handle(), p0, q0) == ESLAM_OK, "second init");
        eu.estimator().invalidate();
        EXPECT(es.estimator().shardBounds() == (std::vector<uint64_t>{0, N}), "the table set_comm was given");
        double x = 0, yaw = 0;
        auto advance = [&]() {
            yaw += 0.002;
            x += 0.02;
            const bool a = es.update(body_pose(x, 0, yaw), body_state(x, 0, yaw), ltc);
            const bool b = eu.update(body_pose(x, 0, yaw), body_state(x, 0, yaw), ltc);
            return a && b;
        };
        for (int s = 0; s < 2; ++s) EXPECT(advance(), "updates before the resamples");
        EXPECT(same_particles(es, eu, N), "the shard starts as the unsharded filter does");

        es.estimator().resample_stratified(7001);
        eu.estimator().resample_stratified(7001);
        EXPECT(same_particles(es, eu, 7001), "resample_stratified(7001): the sharded filter == the unsharded one, byte for byte");
        EXPECT(es.estimator().shardBounds() == (std::vector<uint64_t>{0, 7001}), "the table of 7001 particles");
        EXPECT(es.estimator().shardBounds() == eslam_ns::PoseEstimator::canonicalShardBounds(7001, 1), "... the canonical one");
        EXPECT(!std::memcmp(&es.estimator().lastResample(), &eu.estimator().lastResample(), sizeof(eslam_resample_info)) &&
                   eu.estimator().lastResample().n_before == N && eu.estimator().lastResample().n_after == 7001,
               "the stratified call's info");
        EXPECT(advance(), "update at 7001 particles");
        EXPECT(same_particles(es, eu, 7001), "an update at 7001 particles");

        es.estimator().resample_multinomial(129);
        eu.estimator().resample_multinomial(129);
        const size_t kept = (size_t)eu.estimator().lastResample().n_after;
        EXPECT(kept > 64 && kept <= 129, "the multinomial call keeps most draws (normalised weights)");
        EXPECT(same_particles(es, eu, kept), "resample_multinomial(129): the sharded filter == the unsharded one, byte for byte");
        EXPECT(es.estimator().shardBounds() == (std::vector<uint64_t>{0, (uint64_t)kept}), "the table of the kept draws");
        EXPECT(!std::memcmp(&es.estimator().lastResample(), &eu.estimator().lastResample(), sizeof(eslam_resample_info)),
               "the multinomial call's info");
        EXPECT(advance(), "update after the multinomial call");
        EXPECT(same_particles(es, eu, kept), "an update after the multinomial call");

        bool threw = false;
        try {
            es.estimator().resample_stratified(0);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        EXPECT(threw && es.estimator().getParticles().size() == kept, "samples == 0 is an exception and changes nothing");
        threw = false;
        try {
            (void)eu.estimator().shardBounds();
        } catch (const std::runtime_error&) {
            threw = true;
        }
        EXPECT(threw, "an unsharded estimator has no shard table");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    std::printf(fails ? "facade resample sharded: %d FAILED\n" : "facade resample sharded OK\n", fails);
    return fails ? 1 : 0;
}
