// C++ façade (include/eslam_gpu.hpp) on the GPU: PoseEstimator::kldCount returns what
// eslam_gpu_kld_count returns, bit for bit; resampleKld leaves the particles that a twin estimator
// has after resample_stratified / resample_multinomial(info.samples), getParticles() at the new
// size, lastKld() and lastResample() the two infos; an edit made through getParticles() before
// the call is what gets counted and resampled.  Run by tests/test_gpu_kld_facade.py.
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

static bool same_particles(const std::vector<eslam_ns::PoseParticle>& a, const std::vector<eslam_ns::PoseParticle>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (std::memcmp(&a[i].position, &b[i].position, sizeof(a[i].position)) || std::memcmp(&a[i].orientation, &b[i].orientation, 8) ||
            std::memcmp(&a[i].zPos, &b[i].zPos, 8) || std::memcmp(&a[i].weight, &b[i].weight, 8))
            return false;
    }
    return true;
}

// a cloud through getParticles(): the same values on both estimators
static void spread(eslam_ns::PoseEstimator& pe, double step)
{
    std::vector<eslam_ns::PoseParticle>& v = pe.getParticles();
    for (size_t i = 0; i < v.size(); ++i) {
        v[i].position = eslam_ns::Vector2d(step * (double)(i % 37) - 0.3, step * (double)(i % 23) - 0.2);
        v[i].orientation = 0.05 * (double)(i % 11) - 0.2;
        v[i].weight = (1.0 + (double)(i % 7)) / 6000.0;
    }
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
    eslam_ns::EmbodiedSlamFilter ef(oc, ec), twin(oc, ec);
    try {
        ef.init(env, startPose, true);
        twin.init(env, startPose, true);
        eslam_ns::PoseEstimator &pe = ef.estimator(), &pt = twin.estimator();
        spread(pe, 0.03);
        spread(pt, 0.03);

        // kldCount against the C ABI, the edit written back first
        eslam_ns::KldParams kp;
        kp.nMin = 1;
        const eslam_kld_info got = pe.kldCount(kp);
        eslam_kld_params p;
        eslam_kld_params_default(nullptr, &p);
        eslam_kld_info want;
        EXPECT(eslam_gpu_kld_count(pe.handle(), &p, &want) == ESLAM_OK, "the C ABI's count");
        EXPECT(std::memcmp(&got, &want, sizeof(got)) == 0, "kldCount equals eslam_gpu_kld_count");
        EXPECT(got.particles_counted == 1500 && got.bins_occupied > 100 && got.samples > 1500, "a spread cloud asks for more particles");
        const eslam_kld_info viaFilter = ef.kldCount(kp);
        EXPECT(std::memcmp(&viaFilter, &want, sizeof(want)) == 0, "EmbodiedSlamFilter::kldCount forwards");
        const eslam_kld_info dflt = pe.kldCount();
        EXPECT(dflt.bins_occupied == want.bins_occupied && dflt.samples == want.samples, "the default n_min is the configured count");
        spread(pe, 0.0005);
        spread(pt, 0.0005);
        const eslam_kld_info tight = pe.kldCount();
        EXPECT(tight.samples == 1500 && (tight.clamped & 1u), "... which a converged cloud is raised to");
        EXPECT(pe.size() == 1500 && pe.getParticles().size() == 1500, "a count changes no size");

        // resampleKld: grow (the spread cloud, stratified), then shrink (multinomial, coarse bins)
        spread(pe, 0.03);
        spread(pt, 0.03);
        pe.resampleKld(kp);
        const size_t n1 = pe.size();
        EXPECT(std::memcmp(&pe.lastKld(), &want, sizeof(want)) == 0, "lastKld() is the count's info");
        EXPECT(n1 == want.samples && pe.getParticles().size() == n1, "getParticles() has the new size");
        EXPECT(pe.lastResample().n_before == 1500 && pe.lastResample().n_after == n1, "lastResample()");
        pt.resample_stratified(n1);
        EXPECT(same_particles(pe.getParticles(), pt.getParticles()), "the particles of resample_stratified(info.samples)");
        kp.binXY = 0.5;
        kp.thetaBins = 4;
        kp.multinomial = true;
        ef.resampleKld(kp);
        const size_t n2 = pe.lastKld().samples;
        EXPECT(n2 > 1 && n2 < n1 && pe.lastResample().n_before == n1, "coarse bins shrink the filter");
        pt.resample_multinomial(n2);
        EXPECT(pe.size() == pt.size() && pe.lastResample().n_after == pe.size() && pe.lastResample().dropped == pt.lastResample().dropped,
               "the multinomial call's info");
        EXPECT(same_particles(pe.getParticles(), pt.getParticles()), "the particles of resample_multinomial(info.samples)");

        // an edit through getParticles() is what gets counted: all the mass on particle 7
        std::vector<eslam_ns::PoseParticle>& v = pe.getParticles();
        for (auto& q : v) q.weight = 0.0;
        v[7].weight = 1.0;
        const eslam_ns::PoseParticle seven = v[7];
        eslam_ns::KldParams one;
        one.nMin = 300;
        pe.resampleKld(one);
        EXPECT(pe.lastKld().particles_counted == 1 && pe.lastKld().bins_occupied == 1 && pe.lastKld().samples == 300,
               "one counted particle: n_min");
        size_t bad = 0;
        for (const auto& q : pe.getParticles())
            if (std::memcmp(&q.position, &seven.position, sizeof(q.position)) || q.orientation != seven.orientation) ++bad;
        EXPECT(pe.getParticles().size() == 300 && bad == 0, "300 copies of the particle that held the mass");

        // refusals are exceptions that say why; lastKld() holds the box of a cloud too spread
        bool threw = false;
        try {
            eslam_ns::KldParams badp;
            badp.thetaBins = 0;
            pe.kldCount(badp);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "theta_bins") != nullptr;
        }
        EXPECT(threw, "no yaw bins is an exception that says so");
        spread(pe, 0.03);
        threw = false;
        try {
            eslam_ns::KldParams tiny;
            tiny.maxBins = 8;
            pe.resampleKld(tiny);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "too spread") != nullptr;
        }
        EXPECT(threw && pe.lastKld().bins[0] > 1 && pe.lastKld().samples == 0 && pe.size() == 300, "too spread: the box, nothing changed");
        EXPECT(pe.kldCount(kp).particles_counted == 300, "... and the filter is still usable");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("kld facade OK\n");
    return 0;
}
