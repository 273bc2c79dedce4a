// C++ façade (include/eslam_gpu.hpp) on the GPU: EmbodiedSlamFilter::saveState(path) writes the
// filter's own part into a 4096-byte prefix and the device's snapshot behind it by offset
// (eslam_gpu_save_at); loadState(path) on a second filter that was only constructed reads it back
// (eslam_gpu_load_at), and three update + processMap calls on both then give identical
// getParticles(), bit for bit.  The blob behind the prefix is the one inside saveState(ostream).
// Run by tests/test_gpu_snapshot_facade_file.py (argument: the file to write).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
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

static bool same_bits(double a, double b) { return !std::memcmp(&a, &b, sizeof(a)); }

static size_t differing(const std::vector<eslam_ns::PoseParticle>& a, const std::vector<eslam_ns::PoseParticle>& b)
{
    if (a.size() != b.size()) return a.size() + b.size() + 1;
    size_t d = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const eslam_ns::PoseParticle &p = a[i], &q = b[i];
        if (!same_bits(p.position.x(), q.position.x()) || !same_bits(p.position.y(), q.position.y()) ||
            !same_bits(p.orientation, q.orientation) || !same_bits(p.zPos, q.zPos) || !same_bits(p.zSigma, q.zSigma) ||
            !same_bits(p.weight, q.weight) || !same_bits(p.mprob, q.mprob) || p.floating != q.floating ||
            p.cpoints.size() != q.cpoints.size())
            ++d;
    }
    return d;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::printf("usage: test_snapshot_facade_file FILE\n");
        return 2;
    }
    const std::string path = argv[1];
    const uint32_t W = 120;
    const eslam_ns::MlsGrid env = flat_grid(W);
    eslam_ns::Configuration ec;
    ec.particleCount = 2000;
    ec.minEffective = 2001;                                   // a resample at every update: shared tables
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.contactModel.minContacts = 3;
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;

    std::vector<eslam_ns::ScanPatch> scan;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 4; ++j) {
            eslam_ns::ScanPatch sp;
            sp.position = eslam_ns::Vector3d(0.35 + 0.1 * i, -0.6 + 0.2 * j, -0.13 + 0.01 * j);
            sp.stdev = 0.03;
            scan.push_back(sp);
        }

    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    ef.init(env, startPose, false);                           // every particle its own map
    double x = 0, yaw = 0;
    auto advance = [&](eslam_ns::EmbodiedSlamFilter& f, double fx, double fyaw) {
        const bool u = f.update(body_pose(fx, 0, fyaw), body_state(fx, 0, fyaw), ltc);
        f.processMap(scan, false, true);
        return u;
    };
    for (int s = 0; s < 4; ++s) {
        yaw += 0.002;
        x += 0.02;
        EXPECT(advance(ef, x, yaw), "update before the save");
    }
    std::stringstream ss(std::ios::in | std::ios::out | std::ios::binary);
    try {
        ef.saveState(path, 65536);
        ef.saveState(ss);
    } catch (const std::exception& e) {
        std::printf("FAIL: saveState threw: %s\n", e.what());
        return 1;
    }
    std::ifstream in(path, std::ios::binary);
    const std::string file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::string stream = ss.str();
    const size_t prefix = eslam_ns::EmbodiedSlamFilter::kStatePrefix;
    EXPECT(prefix == 4096 && file.size() > prefix + 100000, "the file holds the prefix, the particles and their maps");
    if (file.size() > prefix && stream.size() > file.size() - prefix) {
        const size_t blob = file.size() - prefix, own = stream.size() - blob;
        EXPECT(file.compare(prefix, blob, stream, own, blob) == 0, "the blob behind the prefix is the one inside saveState(ostream)");
        EXPECT(own <= prefix && file.compare(0, own, stream, 0, own) == 0, "the prefix starts with the filter's own part");
        EXPECT(file.find_first_not_of('\0', own) >= prefix, "zeros up to the blob");
    } else {
        EXPECT(false, "the stream form is the file's blob behind the filter's own part");
    }

    eslam_ns::EmbodiedSlamFilter rest(oc, ec);                // only constructed: no init()
    try {
        rest.loadState(path, 4096);
    } catch (const std::exception& e) {
        std::printf("FAIL: loadState threw: %s\n", e.what());
        return 1;
    }
    EXPECT(differing(ef.getParticles(), rest.getParticles()) == 0, "the loaded particles equal the saved ones");
    for (int s = 0; s < 3; ++s) {
        yaw += 0.002;
        x += 0.02;
        const bool a = advance(ef, x, yaw), b = advance(rest, x, yaw);
        EXPECT(a && b, "update after the load");
        EXPECT(differing(ef.getParticles(), rest.getParticles()) == 0,
               "update + processMap after loadState(path): the same particles as the filter that saved, bit for bit");
    }
    // both filters save the same file again, over the old one (no truncation needed: the size is set)
    ef.saveState(path);
    std::ifstream in1(path, std::ios::binary);
    const std::string f1((std::istreambuf_iterator<char>(in1)), std::istreambuf_iterator<char>());
    rest.saveState(path, 4096);
    std::ifstream in2(path, std::ios::binary);
    const std::string f2((std::istreambuf_iterator<char>(in2)), std::istreambuf_iterator<char>());
    EXPECT(f1 == f2 && f1 != file, "both filters save the same bytes");
    bool threw = false;
    try {
        rest.loadState(path + ".missing");
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT(threw, "a missing file is an exception");

    if (fails) return 1;
    std::printf("snapshot facade file OK\n");
    return 0;
}
