// C++ façade (include/eslam_gpu.hpp) on the GPU: PoseEstimator::fitGmm and
// EmbodiedSlamFilter::getPoseDistribution(stride, GmmParams) return what eslam_gpu_fit_pose_gmm
// returns, live components only, read as the reference's viewer reads PoseDistribution::gmm
// (viz/ParticleVisualization.cpp:98-107); getPoseDistribution(stride) leaves gmm empty.
// Run by tests/test_gpu_gmm_facade.py.
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

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// the façade's mixture against the C ABI's components: the live ones, in order, bit for bit
static bool equal(const eslam_ns::GaussianMixture2D& g, const eslam_gmm_component* c, unsigned K, const eslam_gmm_info& info)
{
    size_t j = 0;
    for (unsigned k = 0; k < K; ++k) {
        if (!(info.live_mask >> k & 1u)) continue;
        if (!(c[k].weight > 0.0) || j >= g.params.size()) return false;
        const eslam_ns::GaussianMixture2D::Parameter& p = g.params[j++];
        if (!same(p.weight, c[k].weight) || !same(p.dist.mean.x(), c[k].mean[0]) || !same(p.dist.mean.y(), c[k].mean[1]) ||
            !same(p.dist.cov(0, 0), c[k].cov[0]) || !same(p.dist.cov(0, 1), c[k].cov[1]) || !same(p.dist.cov(1, 0), c[k].cov[1]) ||
            !same(p.dist.cov(1, 1), c[k].cov[2]))
            return false;
    }
    return j == g.params.size() && j == info.components_live && g.info.iterations == info.iterations &&
           g.info.converged == info.converged && same(g.info.log_likelihood, info.log_likelihood) &&
           g.info.particles_used == info.particles_used;
}

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
        // three groups through getParticles(): the edit is what gets fitted
        std::vector<eslam_ns::PoseParticle>& v = pe.getParticles();
        for (size_t i = 0; i < v.size(); ++i) {
            const int grp = (int)(i % 3);
            v[i].position = eslam_ns::Vector2d(v[i].position.x() + 4.0 * grp, v[i].position.y() - 1.0 * grp);
            v[i].weight = 1e-3 * (1.0 + (double)(i % 7));
        }
        for (unsigned K : {1u, 3u, 5u}) {
            eslam_ns::GmmParams gp;
            gp.components = K;
            const eslam_ns::GaussianMixture2D g = pe.fitGmm(gp);
            eslam_gmm_params p;
            eslam_gmm_params_default(&p);
            p.components = K;
            eslam_gmm_component c[ESLAM_GMM_MAX_COMPONENTS];
            eslam_gmm_info info;
            EXPECT(eslam_gpu_fit_pose_gmm(pe.handle(), &p, c, &info) == ESLAM_OK, "the C ABI's fit");
            EXPECT(equal(g, c, K, info), "fitGmm equals eslam_gpu_fit_pose_gmm, live components only");
            EXPECT(!g.params.empty() && g.params.size() <= K, "live components");
            const eslam_ns::PoseDistribution d = ef.getPoseDistribution(4, gp);
            EXPECT(equal(d.gmm, c, K, info), "getPoseDistribution(stride, GmmParams) fills gmm with the same fit");
            EXPECT(d.particles.size() == (1500 - 1) / 4 + 1, "... and the strided particles");
        }
        const eslam_ns::GaussianMixture2D g3 = ef.fitGmm();
        EXPECT(g3.params.size() == 3 && g3.info.converged == 1, "the default parameters find the three groups");
        for (size_t k = 0; k < g3.params.size(); ++k) {
            EXPECT(std::fabs(g3.params[k].dist.mean.x() - 4.0 * (double)k) < 0.1, "a group's mean x");
            EXPECT(std::fabs(g3.params[k].dist.mean.y() + 1.0 * (double)k) < 0.1, "a group's mean y");
            EXPECT(std::fabs(g3.params[k].weight - 1.0 / 3.0) < 0.02, "a group's weight");
        }
        // a dead component is left out: every particle on one spot, three components asked for
        for (auto& p : pe.getParticles()) p.position = eslam_ns::Vector2d(1.25, -0.5);
        const eslam_ns::GaussianMixture2D one = pe.fitGmm();
        EXPECT(one.params.size() == 1 && one.info.components_live == 1, "identical particles: one live component");
        EXPECT(one.params[0].weight == 1.0 && one.params[0].dist.mean.x() == 1.25 && one.params[0].dist.cov(0, 0) == 0.0,
               "... at the spot, covariance 0");
        EXPECT(ef.getPoseDistribution(1).gmm.params.empty() && ef.getPoseDistribution().gmm.info.iterations == 0,
               "getPoseDistribution(stride) leaves gmm empty");
        bool threw = false;
        try {
            eslam_ns::GmmParams bad;
            bad.components = 9;
            pe.fitGmm(bad);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "components") != nullptr;
        }
        EXPECT(threw, "nine components is an exception that says so");
        EXPECT(pe.fitGmm().params.size() == 1, "... and the filter is still usable");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("gmm facade OK\n");
    return 0;
}
