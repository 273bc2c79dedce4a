// C++ façade (include/eslam_gpu.hpp) on the GPU: PoseEstimator::particleGrid(i) -- the
// reference's particles[i].grid.getMap() (src/PoseEstimator.hpp:79-87) -- equals the raw ABI's
// eslam_gpu_get_particle_grid byte for byte and is an MlsGrid setEnvironment takes, and
// EmbodiedSlamFilter::adoptParticleMap(i) equals eslam_gpu_adopt_particle_map: the same grid
// and, after further steps and map updates, the same particles.  Run by
// tests/test_gpu_particle_grid_facade.py.
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

// a flat grid whose cells at x >= 0.3 hold nothing yet (the terrain ahead is not mapped)
static eslam_ns::MlsGrid half_grid(uint32_t W)
{
    eslam_ns::MlsGrid g;
    g.width = g.height = W;
    g.scaleX = g.scaleY = 0.1;
    g.offsetX = g.offsetY = -0.05 * W;
    g.cellStart.assign((size_t)W * W + 1, 0);
    uint32_t k = 0;
    for (uint32_t c = 0; c < W * W; ++c) {
        g.cellStart[c] = k;
        if (g.offsetX + ((c % W) + 0.5) * g.scaleX < 0.3) ++k;
    }
    g.cellStart[(size_t)W * W] = k;
    g.mean.assign(k, 0.0f);
    g.stdev.assign(k, 0.05f);
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

static bool get_particle_grid(eslam_ctx* ctx, uint64_t i, uint32_t W, HostMap* m)
{
    if (eslam_gpu_particle_grid_size(ctx, i, &m->np) != ESLAM_OK) return false;
    m->cells.assign((size_t)W * W + 1, 0);
    m->mean.assign(m->np, 0.0f);
    m->stdev.assign(m->np, 0.0f);
    return eslam_gpu_get_particle_grid(ctx, i, m->cells.data(), m->mean.data(), m->stdev.data(), nullptr, m->np) == ESLAM_OK;
}

static bool same_map(const HostMap& a, const HostMap& b)
{
    return a.np == b.np && a.cells == b.cells && !std::memcmp(a.mean.data(), b.mean.data(), a.np * 4) &&
           !std::memcmp(a.stdev.data(), b.stdev.data(), a.np * 4);
}

int main()
{
    const uint32_t W = 83;
    const size_t n = 600;
    const eslam_ns::MlsGrid env = half_grid(W);
    eslam_ns::Configuration ec;
    ec.particleCount = n;
    ec.minEffective = 400;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;

    try {
        eslam_ns::EmbodiedSlamFilter ef(oc, ec);
        ef.init(env, startPose, false);
        eslam_ns::FootContact odo(oc);
        eslam_ns::PoseEstimator raw(odo, ec);
        const eslam_mls_grid g = env.toC();
        EXPECT(eslam_gpu_set_map(raw.handle(), &g) == ESLAM_OK, "raw set_map");
        EXPECT(eslam_gpu_set_particle_maps(raw.handle(), 1) == ESLAM_OK, "raw per-particle maps");
        const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};
        EXPECT(eslam_gpu_init_pose(raw.handle(), p0, q0) == ESLAM_OK, "raw init");

        std::vector<eslam_ns::ScanPatch> scan;
        std::vector<eslam_scan_patch> rs;
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 5; ++j) {
                eslam_ns::ScanPatch sp;
                sp.position = eslam_ns::Vector3d(0.35 + 0.1 * i, -0.7 + 0.2 * j, -0.18 + 0.01 * std::sin(3.0 * i + j));
                sp.stdev = 0.03;
                scan.push_back(sp);
                eslam_scan_patch r;
                for (int k = 0; k < 3; ++k) r.position[k] = sp.position[k];
                r.stdev = sp.stdev;
                rs.push_back(r);
            }

        std::vector<double> X(n), Y(n), TH(n), Z(n), ZS(n), Wt(n), M(n);
        std::vector<uint8_t> FL(n), NC(n);
        eslam_particles p = {X.data(), Y.data(), TH.data(), Z.data(), ZS.data(), Wt.data(), M.data(), FL.data(), NC.data()};
        double x = 0, yaw = 0;
        auto advance = [&]() {
            yaw += 0.002;
            x += 0.02;
            const eslam_ns::Affine3d T = body_pose(x, 0, yaw);
            const eslam_ns::BodyContactState bs = body_state(x, 0, yaw);
            ef.update(T, bs, ltc);
            ef.processMap(scan, false, true);
            const eslam_ns::Quaterniond q(T.linear());
            odo.update(bs, q);
            const eslam_step_input in = raw.makeInput(bs, q, T.translation(), 0);
            int u = 0;
            EXPECT(eslam_gpu_step(raw.handle(), &in, &u) == ESLAM_OK && u == 1, "raw step");
            EXPECT(eslam_gpu_map_update(raw.handle(), rs.data(), (uint32_t)rs.size()) == ESLAM_OK, "raw map update");
        };
        auto same_particles = [&]() {
            std::vector<eslam_ns::PoseParticle>& a = ef.getParticles();
            if (eslam_gpu_download_particles(raw.handle(), &p) != ESLAM_OK) return false;
            size_t diff = a.size() != n;
            for (size_t i = 0; i < a.size() && i < n; ++i)
                diff += std::memcmp(&a[i].position.v[0], &X[i], 8) || std::memcmp(&a[i].position.v[1], &Y[i], 8) ||
                        std::memcmp(&a[i].orientation, &TH[i], 8) || std::memcmp(&a[i].zPos, &Z[i], 8) ||
                        std::memcmp(&a[i].zSigma, &ZS[i], 8) || std::memcmp(&a[i].weight, &Wt[i], 8) ||
                        std::memcmp(&a[i].mprob, &M[i], 8) || a[i].floating != (FL[i] != 0);
            return diff == 0;
        };
        for (int s = 0; s < 8; ++s) advance();
        EXPECT(same_particles(), "the mapping run: façade and raw ABI hold the same particles");

        // particleGrid(i) == eslam_gpu_get_particle_grid, byte for byte, with the environment's geometry
        const size_t best = ef.getBestParticleIndex();
        const size_t probes[3] = {0, best, n - 1};
        eslam_ns::MlsGrid bestGrid;
        for (size_t i : probes) {
            const eslam_ns::MlsGrid pg = ef.estimator().particleGrid(i);
            HostMap r;
            EXPECT(get_particle_grid(raw.handle(), i, W, &r), "raw get_particle_grid");
            EXPECT(pg.width == W && pg.height == W && pg.mean.size() == r.np && pg.stdev.size() == r.np && pg.cellStart == r.cells &&
                       !std::memcmp(pg.mean.data(), r.mean.data(), r.np * 4) && !std::memcmp(pg.stdev.data(), r.stdev.data(), r.np * 4),
                   "particleGrid(i): the raw ABI's arrays, byte for byte");
            EXPECT(pg.patchHeight.empty() && pg.scaleX == env.scaleX && pg.offsetX == env.offsetX && pg.offsetY == env.offsetY,
                   "particleGrid(i): the environment's geometry, no heights");
            EXPECT(r.np > env.mean.size(), "the particle's own patches are in its grid");
            if (i == best) bestGrid = pg;
        }
        bool threw = false;
        try {
            ef.estimator().particleGrid(n);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        EXPECT(threw, "particleGrid(n) is an exception");

        // adoptParticleMap(i) == eslam_gpu_adopt_particle_map: the exported grid is the shared one
        ef.adoptParticleMap(best);
        EXPECT(eslam_gpu_adopt_particle_map(raw.handle(), best) == ESLAM_OK, "raw adopt");
        HostMap mf, mr;
        EXPECT(get_map(ef.estimator().handle(), &mf) && get_map(raw.handle(), &mr), "get_map");
        EXPECT(same_map(mf, mr), "adoptParticleMap: the same grid as the raw ABI");
        EXPECT(mf.np == bestGrid.mean.size() && mf.cells == bestGrid.cellStart &&
                   !std::memcmp(mf.mean.data(), bestGrid.mean.data(), mf.np * 4) &&
                   !std::memcmp(mf.stdev.data(), bestGrid.stdev.data(), mf.np * 4),
               "adoptParticleMap: the shared grid is particleGrid(i)");
        uint32_t cnt = 1;
        EXPECT(eslam_gpu_get_particle_map(ef.estimator().handle(), 0, nullptr, nullptr, nullptr, 0, &cnt) == ESLAM_OK && cnt == 0,
               "adoptParticleMap: every particle's own map starts over");
        for (int s = 0; s < 3; ++s) advance();
        EXPECT(same_particles(), "after the adoption: façade and raw ABI continue alike");
        const eslam_ns::MlsGrid again = ef.estimator().particleGrid(1);
        EXPECT(again.mean.size() > mf.np, "new own patches on top of the adopted grid");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    std::printf(fails ? "facade particle grid: %d FAILED\n" : "facade particle grid OK\n", fails);
    return fails ? 1 : 0;
}
