// C++ façade (include/eslam_gpu.hpp) on the GPU: EmbodiedSlamFilter::processMap with the shared
// map (useSharedMap = true) and update = true merges the scan into the shared grid
// (src/EmbodiedSlamFilter.cpp:184-227; the camera path's processMap(scanMap, false, true) at
// :301).  processMap(scan, false, true) and processMap(scan, true, true) must equal the raw ABI
// sequence (eslam_gpu_map_match, eslam_gpu_shared_map_update) bit for bit: the same particles
// and the same eslam_gpu_get_map bytes.  Run by tests/test_gpu_shared_map.py.
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

int main()
{
    const uint32_t W = 120;
    const eslam_ns::MlsGrid env = flat_grid(W);
    eslam_ns::Configuration ec;
    ec.particleCount = 2000;
    ec.minEffective = 1500;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);   // zSigma well below the ledge's 0.6 m
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;

    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    ef.init(env, startPose, true);
    eslam_ns::FootContact odo(oc);
    eslam_ns::PoseEstimator raw(odo, ec);
    const eslam_mls_grid g = env.toC();
    EXPECT(eslam_gpu_set_map(raw.handle(), &g) == ESLAM_OK, "raw set_map");
    const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};
    EXPECT(eslam_gpu_init_pose(raw.handle(), p0, q0) == ESLAM_OK, "raw init");

    // the ground ahead 5 cm above the grid (fuses) and a ledge 0.6 m up (a second level)
    std::vector<eslam_ns::ScanPatch> scan;
    std::vector<eslam_scan_patch> rs;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 4; ++j) {
            eslam_ns::ScanPatch sp;
            sp.position = eslam_ns::Vector3d(0.35 + 0.1 * i, -0.6 + 0.2 * j, (i & 1) ? 0.42 : -0.13);
            sp.stdev = 0.03;
            scan.push_back(sp);
            eslam_scan_patch r;
            for (int k = 0; k < 3; ++k) r.position[k] = sp.position[k];
            r.stdev = sp.stdev;
            rs.push_back(r);
        }

    HostMap m0, mf, mr;
    EXPECT(get_map(ef.estimator().handle(), &m0), "get_map after init");
    EXPECT(m0.np == (uint64_t)W * W && m0.cells == env.cellStart && !std::memcmp(m0.mean.data(), env.mean.data(), m0.np * 4) &&
               !std::memcmp(m0.stdev.data(), env.stdev.data(), m0.np * 4),
           "get_map after set_map returns the uploaded grid");

    const size_t n = 2000;
    std::vector<double> X(n), Y(n), TH(n), Z(n), ZS(n), Wt(n), M(n);
    std::vector<uint8_t> FL(n), NC(n);
    eslam_particles p = {X.data(), Y.data(), TH.data(), Z.data(), ZS.data(), Wt.data(), M.data(), FL.data(), NC.data()};
    double x = 0, yaw = 0;
    uint64_t inserted = 0, fused = 0;
    for (int s = 0; s < 6; ++s) {
        yaw += 0.002;
        x += 0.02;
        const eslam_ns::Affine3d T = body_pose(x, 0, yaw);
        const eslam_ns::BodyContactState bs = body_state(x, 0, yaw);
        ef.update(T, bs, ltc);
        const eslam_ns::Quaterniond q(T.linear());
        odo.update(bs, q);
        const eslam_step_input in = raw.makeInput(bs, q, T.translation(), 0);
        int u = 0;
        EXPECT(eslam_gpu_step(raw.handle(), &in, &u) == ESLAM_OK && u == 1, "raw step");
        if (s < 2) continue;
        const bool match = (s & 1) != 0;                        // (false, true) and (true, true) in turn
        ef.processMap(scan, match, true);
        if (match) EXPECT(eslam_gpu_map_match(raw.handle(), rs.data(), (uint32_t)rs.size()) == ESLAM_OK, "raw match");
        eslam_shared_merge_info info;
        EXPECT(eslam_gpu_shared_map_update(raw.handle(), rs.data(), (uint32_t)rs.size(), 0, &info) == ESLAM_OK, "raw merge");
        EXPECT(info.particles_done == n && info.patches_placed + info.patches_off_grid == n * rs.size(), "merge counters");
        inserted += info.inserted;
        fused += info.fused;
        EXPECT(get_map(ef.estimator().handle(), &mf) && get_map(raw.handle(), &mr), "get_map");
        EXPECT(same_map(mf, mr), "processMap(update = true) on the shared map: the same grid as the raw ABI, bit for bit");
        EXPECT(mr.np == info.n_patches, "n_patches");
        std::vector<eslam_ns::PoseParticle>& a = ef.getParticles();
        EXPECT(eslam_gpu_download_particles(raw.handle(), &p) == ESLAM_OK, "raw download");
        size_t diff = a.size() != n;
        for (size_t i = 0; i < a.size() && i < n; ++i)
            diff += std::memcmp(&a[i].position.v[0], &X[i], 8) || std::memcmp(&a[i].position.v[1], &Y[i], 8) ||
                    std::memcmp(&a[i].orientation, &TH[i], 8) || std::memcmp(&a[i].zPos, &Z[i], 8) ||
                    std::memcmp(&a[i].zSigma, &ZS[i], 8) || std::memcmp(&a[i].weight, &Wt[i], 8) ||
                    std::memcmp(&a[i].mprob, &M[i], 8) || a[i].floating != (FL[i] != 0);
        EXPECT(diff == 0, "processMap(update = true) on the shared map: the same particles as the raw ABI, bit for bit");
    }
    EXPECT(inserted > 0 && fused > 0, "the scans fused with the ground and inserted a second level");
    EXPECT(mf.np > m0.np, "the patch count grew");

    // PoseEstimator::updateSharedMap hands the counters out
    const eslam_shared_merge_info last = ef.estimator().updateSharedMap(scan, 7 * scan.size());
    EXPECT(last.particles_done == n && last.runs > 1 && last.n_patches >= mf.np, "updateSharedMap(scan, maxRecords)");

    std::printf(fails ? "facade shared map: %d FAILED\n" : "facade shared map OK\n", fails);
    return fails ? 1 : 0;
}
