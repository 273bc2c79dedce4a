// C++ façade (include/eslam_gpu.hpp) on the GPU: the shared map's merge on a sharded filter.
// An EmbodiedSlamFilter whose estimator is shard 0 of 1 over the library's own RCCL communicator
// (PoseEstimator::setCommRccl) goes through processMap(scan, true, true) and the camera overload
// of update (src/EmbodiedSlamFilter.cpp:184-227, 239-309): PoseEstimator::updateSharedMap takes
// the collective eslam_gpu_shared_map_update_sharded there.  It must end with the same particles
// and the same eslam_gpu_get_map bytes as an unsharded filter given the same calls.  Run by
// tests/test_gpu_shared_map_sharded.py.
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

static eslam_ns::Matrix3d rot_y(double a)
{
    eslam_ns::Matrix3d R = eslam_ns::Matrix3d::Identity();
    R(0, 0) = std::cos(a); R(0, 2) = std::sin(a);
    R(2, 0) = -std::sin(a); R(2, 2) = std::cos(a);
    return R;
}

// a camera 0.4 m up looking ahead and down: image x to the right (body -y), image y down (body -z)
static eslam_ns::Affine3d camera_pose()
{
    eslam_ns::Matrix3d C;
    C(0, 0) = 0; C(0, 1) = 0; C(0, 2) = 1;
    C(1, 0) = -1; C(1, 1) = 0; C(1, 2) = 0;
    C(2, 0) = 0; C(2, 1) = -1; C(2, 2) = 0;
    eslam_ns::Affine3d T = eslam_ns::Affine3d::Identity();
    T.linear() = rot_y(0.6) * C;
    T.translation() = eslam_ns::Vector3d(0.15, 0.0, 0.4);
    return T;
}

// the floor 0.18 m below the body as the camera sees it, with a few invalid pixels
static eslam_ns::DistanceImage depth_image()
{
    eslam_ns::DistanceImage im;
    im.width = 37;
    im.height = 23;
    const double f = 30.0;
    im.scale_x = im.scale_y = 1.0 / f;
    im.center_x = -((double)im.width - 1.0) / 2.0 / f;
    im.center_y = -((double)im.height - 1.0) / 2.0 / f;
    const eslam_ns::Affine3d T = camera_pose();
    for (uint32_t v = 0; v < im.height; ++v)
        for (uint32_t u = 0; u < im.width; ++u) {
            const eslam_ns::Vector3d ray(u * im.scale_x + im.center_x, v * im.scale_y + im.center_y, 1.0);
            const double dz = (T.linear() * ray)[2];
            double d = dz < -1e-3 ? (-0.18 - 0.4) / dz : 9.0;
            if ((u * 7 + v) % 41 == 0) d = (u & 1) ? 0.0 : NAN;
            im.data.push_back((float)d);
        }
    return im;
}

struct HostMap {
    uint64_t np = 0;
    std::vector<uint32_t> cells;
    std::vector<float> mean, stdev;
};

static bool get_map(eslam_ctx* ctx, HostMap* m)
{
    uint32_t w = 0, h = 0;
    int hh = 0;
    if (eslam_gpu_map_size(ctx, &w, &h, &m->np, &hh) != ESLAM_OK) return false;
    m->cells.assign((size_t)w * h + 1, 0);
    m->mean.assign(m->np, 0.0f);
    m->stdev.assign(m->np, 0.0f);
    return eslam_gpu_get_map(ctx, m->cells.data(), m->mean.data(), m->stdev.data(), nullptr, m->np) == ESLAM_OK;
}

static bool same_map(const HostMap& a, const HostMap& b)
{
    return a.np == b.np && a.cells == b.cells && !std::memcmp(a.mean.data(), b.mean.data(), a.np * 4) &&
           !std::memcmp(a.stdev.data(), b.stdev.data(), a.np * 4);
}

static bool same_particles(eslam_ns::EmbodiedSlamFilter& a, eslam_ns::EmbodiedSlamFilter& b)
{
    const std::vector<eslam_ns::PoseParticle>& pa = a.getParticles();
    const std::vector<eslam_ns::PoseParticle>& pb = b.getParticles();
    size_t diff = pa.size() != pb.size() || pa.empty();
    for (size_t i = 0; i < pa.size() && i < pb.size(); ++i)
        diff += std::memcmp(&pa[i].position.v[0], &pb[i].position.v[0], 8) || std::memcmp(&pa[i].position.v[1], &pb[i].position.v[1], 8) ||
                std::memcmp(&pa[i].orientation, &pb[i].orientation, 8) || std::memcmp(&pa[i].zPos, &pb[i].zPos, 8) ||
                std::memcmp(&pa[i].zSigma, &pb[i].zSigma, 8) || std::memcmp(&pa[i].weight, &pb[i].weight, 8) ||
                std::memcmp(&pa[i].mprob, &pb[i].mprob, 8) || pa[i].floating != pb[i].floating;
    return diff == 0;
}

int main()
{
    const uint32_t W = 120;
    const size_t N = 2000;
    const eslam_ns::MlsGrid env = flat_grid(W);
    eslam_ns::Configuration ec;
    ec.particleCount = N;
    ec.minEffective = 1500;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;
    const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};

    // the sharded filter: init() builds the estimator and attaches the grid; making it a shard
    // drops the particles, which are then initialised again.  The unsharded filter is given the
    // same calls (a filter's second initialisation draws other samples than its first).
    eslam_ns::EmbodiedSlamFilter es(oc, ec), eu(oc, ec);
    es.init(env, startPose, true);
    es.estimator().setCommRccl(1, 0, eslam_ns::PoseEstimator::rcclUniqueId(), N, std::vector<uint64_t>{0, N});
    EXPECT(es.estimator().sharded(), "the estimator is sharded");
    EXPECT(eslam_gpu_init_pose(es.estimator().handle(), p0, q0) == ESLAM_OK, "shard init");
    es.estimator().invalidate();
    eu.init(env, startPose, true);
    EXPECT(!eu.estimator().sharded(), "the other estimator is not");
    EXPECT(eslam_gpu_init_pose(eu.estimator().handle(), p0, q0) == ESLAM_OK, "second init");
    eu.estimator().invalidate();
    EXPECT(same_particles(es, eu), "the shard starts as the unsharded filter does");

    // the ground ahead 5 cm above the grid (fuses) and a ledge 0.6 m up (a second level)
    std::vector<eslam_ns::ScanPatch> scan;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 4; ++j) {
            eslam_ns::ScanPatch sp;
            sp.position = eslam_ns::Vector3d(0.35 + 0.1 * i, -0.6 + 0.2 * j, (i & 1) ? 0.42 : -0.13);
            sp.stdev = 0.03;
            scan.push_back(sp);
        }

    HostMap m0, ms, mu;
    EXPECT(get_map(eu.estimator().handle(), &m0), "get_map after init");
    double x = 0, yaw = 0;
    auto contact_step = [&](double dx) {
        x += dx;
        yaw += 0.002;
        const eslam_ns::Affine3d T = body_pose(x, 0, yaw);
        const eslam_ns::BodyContactState bs = body_state(x, 0, yaw);
        const bool a = es.update(T, bs, ltc), b = eu.update(T, bs, ltc);
        EXPECT(a && b, "both filters update");
        return T;
    };
    auto compare = [&](const char* what) {
        EXPECT(same_particles(es, eu), what);
        EXPECT(get_map(es.estimator().handle(), &ms) && get_map(eu.estimator().handle(), &mu) && same_map(ms, mu), what);
    };

    contact_step(0.02);
    eslam_ns::Affine3d T = contact_step(0.02);
    es.processMap(scan, true, true);
    eu.processMap(scan, true, true);
    compare("processMap(scan, true, true): the sharded filter == the unsharded one, bit for bit");
    EXPECT(mu.np > m0.np, "the scan inserted a second level");
    const uint64_t np1 = mu.np;
    HostMap m1 = mu;

    const eslam_ns::DistanceImage im = depth_image();
    const eslam_ns::Affine3d c2b = camera_pose();
    const bool a = es.update(T, im, c2b), b = eu.update(T, im, c2b);
    EXPECT(a && b, "the first image after init maps on both filters");
    EXPECT(!std::memcmp(&es.lastScanInfo(), &eu.lastScanInfo(), sizeof(eslam_scan_info)) && eu.lastScanInfo().patches > 1,
           "the image's scan");
    compare("update(body2odometry, DistanceImage, camera2body): the sharded filter == the unsharded one, bit for bit");
    EXPECT(mu.np >= np1 && !same_map(mu, m1), "the camera path merged into the shared map");

    contact_step(0.02);                                      // a step on the merged grid
    compare("a step after the merges");

    // the counters, and runs that split the one shard
    const eslam_shared_merge_info is = es.estimator().updateSharedMap(scan, 7 * scan.size());
    const eslam_shared_merge_info iu = eu.estimator().updateSharedMap(scan, 7 * scan.size());
    EXPECT(!std::memcmp(&is, &iu, sizeof(is)) && is.particles_done == N && is.runs == (N + 6) / 7, "updateSharedMap's counters");
    compare("updateSharedMap(scan, maxRecords)");

    std::printf(fails ? "facade shared map sharded: %d FAILED\n" : "facade shared map sharded OK\n", fails);
    return fails ? 1 : 0;
}
