// C++ façade (include/eslam_gpu.hpp) on the GPU: EmbodiedSlamFilter::update(body2odometry,
// LaserScan, laser2body) and update(body2odometry, DistanceImage, camera2body)
// (src/EmbodiedSlamFilter.cpp:311-351, 239-309).  On both map modes each overload must equal the raw
// ABI sequence -- eslam_gpu_scan_from_laser / _depth, then eslam_gpu_map_match /
// eslam_gpu_map_update / eslam_gpu_shared_map_update as processMap would call them -- bit for bit
// (particles, the shared grid, sampled particle maps), and follow the reference's gates: true on
// the first call after init, false for an unmoved pose, true again past the threshold; on the
// shared map the laser path does not merge and the camera path does.  Run by
// tests/test_gpu_scan_facade.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "eslam_gpu.hpp"

static int fails = 0;
#define EXPECT(c, msg)                                                      \
    do {                                                                    \
        if (!(c)) { std::printf("FAIL (%s): %s\n", g_mode, msg); ++fails; } \
    } while (0)

namespace eslam_ns = eslam::gpu;
static const char* g_mode = "";

// a flat grid; with `hole` the cells ahead of x = 0.3 are left empty (the particles' own cells)
static eslam_ns::MlsGrid flat_grid(uint32_t W, bool hole)
{
    eslam_ns::MlsGrid g;
    g.width = g.height = W;
    g.scaleX = g.scaleY = 0.1;
    g.offsetX = g.offsetY = -0.05 * W;
    g.cellStart.resize(W * W + 1);
    uint32_t np = 0;
    for (uint32_t n = 0; n < W; ++n)
        for (uint32_t m = 0; m < W; ++m) {
            g.cellStart[n * W + m] = np;
            const double x = g.offsetX + (m + 0.5) * g.scaleX;
            if (!hole || x < 0.3) ++np;
        }
    g.cellStart[W * W] = np;
    g.mean.assign(np, 0.0f);
    g.stdev.assign(np, 0.05f);
    return g;
}

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

// a laser 0.2 m above the body's origin, pitched down, sweeping the floor 0.18 m below the body
static eslam_ns::Affine3d laser_pose()
{
    eslam_ns::Affine3d T = eslam_ns::Affine3d::Identity();
    T.linear() = rot_y(0.4);
    T.translation() = eslam_ns::Vector3d(0.2, 0.0, 0.2);
    return T;
}

static eslam_ns::LaserScan laser_scan(double lift)
{
    eslam_ns::LaserScan s;
    s.start_angle = -0.6;
    s.angular_resolution = 0.01;
    s.minRange = 20;
    s.maxRange = 30000;
    for (int i = 0; i < 121; ++i) {
        const double a = s.start_angle + i * s.angular_resolution;
        const double r = (0.38 - lift) / (std::sin(0.4) * std::cos(a));
        s.ranges.push_back(i % 17 == 3 ? (uint32_t)(i % 6) : (uint32_t)std::lround(r * 1000.0));
    }
    s.ranges[7] = 25000;                                    // past maxSensorRange
    return s;
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

static eslam_ns::DistanceImage depth_image(double lift)
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
            double d = dz < -1e-3 ? (-0.18 + lift - 0.4) / dz : 9.0;
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

static const size_t N = 1500;

// the façade's particles against the raw context's, bit for bit
static bool same_particles(eslam_ns::EmbodiedSlamFilter& ef, eslam_ctx* raw)
{
    std::vector<double> X(N), Y(N), TH(N), Z(N), ZS(N), Wt(N), M(N);
    std::vector<uint8_t> FL(N), NC(N);
    eslam_particles p = {X.data(), Y.data(), TH.data(), Z.data(), ZS.data(), Wt.data(), M.data(), FL.data(), NC.data()};
    if (eslam_gpu_download_particles(raw, &p) != ESLAM_OK) return false;
    std::vector<eslam_ns::PoseParticle>& a = ef.getParticles();
    size_t diff = a.size() != N;
    for (size_t i = 0; i < a.size() && i < N; ++i)
        diff += std::memcmp(&a[i].position.v[0], &X[i], 8) || std::memcmp(&a[i].position.v[1], &Y[i], 8) ||
                std::memcmp(&a[i].orientation, &TH[i], 8) || std::memcmp(&a[i].zPos, &Z[i], 8) ||
                std::memcmp(&a[i].zSigma, &ZS[i], 8) || std::memcmp(&a[i].weight, &Wt[i], 8) ||
                std::memcmp(&a[i].mprob, &M[i], 8) || a[i].floating != (FL[i] != 0);
    return diff == 0;
}

// sampled particles' own maps, bit for bit; *cells receives how many cells they hold in all
static bool same_particle_maps(eslam_ctx* a, eslam_ctx* b, uint64_t* cells)
{
    const uint32_t cap = 8192;
    std::vector<uint32_t> ca(cap), cb(cap);
    std::vector<float> ma(cap), mb(cap), sa(cap), sb(cap);
    *cells = 0;
    for (uint64_t i = 0; i < N; i += 97) {
        uint32_t na = 0, nb = 0;
        if (eslam_gpu_get_particle_map(a, i, ca.data(), ma.data(), sa.data(), cap, &na) != ESLAM_OK) return false;
        if (eslam_gpu_get_particle_map(b, i, cb.data(), mb.data(), sb.data(), cap, &nb) != ESLAM_OK) return false;
        if (na != nb || na > cap) return false;
        if (std::memcmp(ca.data(), cb.data(), na * 4) || std::memcmp(ma.data(), mb.data(), na * 4) ||
            std::memcmp(sa.data(), sb.data(), na * 4))
            return false;
        *cells += na;
    }
    return true;
}

// the raw ABI sequence of one sensor update: the scan, then processMap(scan, match, update)
static void raw_sensor(eslam_ns::PoseEstimator& raw, const eslam_ns::Configuration& ec, bool shared, bool camera,
                       const eslam_ns::Affine3d& body, const eslam_ns::Affine3d& sensor2body, const eslam_ns::LaserScan& ls,
                       const eslam_ns::DistanceImage& im, eslam_scan_info* info)
{
    eslam_ctx* h = raw.handle();
    eslam_scan_params p;
    const eslam_config c = ec.toC();
    EXPECT(eslam_scan_params_default(&c, &p) == ESLAM_OK, "raw params");
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) p.sensor2body[4 * r + k] = sensor2body.linear()(r, k);
        p.sensor2body[4 * r + 3] = sensor2body.translation()[r];
    }
    const eslam_ns::Quaterniond q(body.linear());
    p.orientation[0] = q.w(); p.orientation[1] = q.x(); p.orientation[2] = q.y(); p.orientation[3] = q.z();
    p.resolution = ec.gridResolution;
    p.patch_thickness = ec.gridPatchThickness;
    p.max_sensor_range = ec.maxSensorRange;
    if (camera) {
        eslam_depth_image d;
        std::memset(&d, 0, sizeof(d));
        d.width = im.width; d.height = im.height;
        d.scale_x = im.scale_x; d.scale_y = im.scale_y; d.center_x = im.center_x; d.center_y = im.center_y;
        d.data = im.data.data();
        EXPECT(eslam_gpu_scan_from_depth(h, &d, &p, info) == ESLAM_OK, "raw scan_from_depth");
    } else {
        eslam_laser_scan s;
        std::memset(&s, 0, sizeof(s));
        s.start_angle = ls.start_angle; s.angular_resolution = ls.angular_resolution;
        s.min_range = ls.minRange; s.max_range = ls.maxRange;
        s.n = (uint32_t)ls.ranges.size();
        s.ranges = ls.ranges.data();
        EXPECT(eslam_gpu_scan_from_laser(h, &s, &p, info) == ESLAM_OK, "raw scan_from_laser");
    }
    uint64_t n = 0;
    EXPECT(eslam_gpu_scan_patches(h, nullptr, 0, &n) == ESLAM_OK && n == info->patches && n > 0, "raw scan_patches (count)");
    std::vector<eslam_scan_patch> sp(n);
    EXPECT(eslam_gpu_scan_patches(h, sp.data(), n, &n) == ESLAM_OK, "raw scan_patches");
    const bool match = camera ? false : ec.useVisualUpdate;
    const bool update = camera ? true : !shared;
    if (match) EXPECT(eslam_gpu_map_match(h, sp.data(), (uint32_t)n) == ESLAM_OK, "raw map_match");
    if (update && !shared) EXPECT(eslam_gpu_map_update(h, sp.data(), (uint32_t)n) == ESLAM_OK, "raw map_update");
    if (update && shared) EXPECT(eslam_gpu_shared_map_update(h, sp.data(), (uint32_t)n, 0, nullptr) == ESLAM_OK, "raw shared_map_update");
}

static void run(bool shared)
{
    g_mode = shared ? "shared map" : "particle maps";
    const eslam_ns::MlsGrid env = flat_grid(120, !shared);
    eslam_ns::Configuration ec;
    ec.particleCount = N;
    ec.minEffective = 1000;
    ec.measurementThreshold = eslam_ns::UpdateThreshold(-1, -1);
    ec.initialTranslationError = eslam_ns::Vector3d(0.1, 0.1, 0.05);
    ec.useVisualUpdate = true;                               // the laser path matches
    ec.localMapPages = 64;                                   // an image reaches more tiles than the default pool's 16
    eslam_ns::OdometryConfiguration oc;
    eslam_ns::Pose startPose(eslam_ns::Vector3d(0, 0, 0.18), eslam_ns::Quaterniond::Identity());
    std::vector<eslam_ns::TerrainClassification> ltc;

    eslam_ns::EmbodiedSlamFilter ef(oc, ec);
    ef.init(env, startPose, shared);
    eslam_ns::FootContact odo(oc);
    eslam_ns::PoseEstimator raw(odo, ec);
    const eslam_mls_grid g = env.toC();
    EXPECT(eslam_gpu_set_map(raw.handle(), &g) == ESLAM_OK, "raw set_map");
    EXPECT(eslam_gpu_set_particle_maps(raw.handle(), shared ? 0 : 1) == ESLAM_OK, "raw set_particle_maps");
    const double p0[3] = {0, 0, 0.18}, q0[4] = {1, 0, 0, 0};
    EXPECT(eslam_gpu_init_pose(raw.handle(), p0, q0) == ESLAM_OK, "raw init");

    const eslam_ns::Affine3d l2b = laser_pose(), c2b = camera_pose();
    double x = 0, yaw = 0;
    auto contact_step = [&](double dx) {
        x += dx;
        yaw += 0.002;
        const eslam_ns::Affine3d T = body_pose(x, 0, yaw);
        const eslam_ns::BodyContactState bs = body_state(x, 0, yaw);
        ef.update(T, bs, ltc);
        const eslam_ns::Quaterniond q(T.linear());
        odo.update(bs, q);
        const eslam_step_input in = raw.makeInput(bs, q, T.translation(), 0);
        int u = 0;
        EXPECT(eslam_gpu_step(raw.handle(), &in, &u) == ESLAM_OK && u == 1, "raw step");
        return T;
    };
    HostMap before, mf, mr;
    uint64_t cells = 0, cells_before = 0;
    auto compare = [&](const char* what) {
        EXPECT(same_particles(ef, raw.handle()), what);
        if (shared) {
            EXPECT(get_map(ef.estimator().handle(), &mf) && get_map(raw.handle(), &mr) && same_map(mf, mr), what);
        } else {
            EXPECT(same_particle_maps(ef.estimator().handle(), raw.handle(), &cells), what);
        }
    };
    int k = 0;
    auto sensor = [&](bool camera, const eslam_ns::Affine3d& T, bool expect) {
        const eslam_ns::LaserScan ls = laser_scan(0.01 * k);
        const eslam_ns::DistanceImage im = depth_image(0.01 * k);
        ++k;
        const bool got = camera ? ef.update(T, im, c2b) : ef.update(T, ls, l2b);
        EXPECT(got == expect, camera ? "camera update: the gate's answer" : "laser update: the gate's answer");
        if (got) {
            eslam_scan_info info;
            raw_sensor(raw, ec, shared, camera, T, camera ? c2b : l2b, ls, im, &info);
            EXPECT(!std::memcmp(&info, &ef.lastScanInfo(), sizeof(info)) && info.patches > 1 && info.points_invalid > 0,
                   "the scan's counters");
        }
        compare(camera ? "camera update == the raw ABI sequence, bit for bit" : "laser update == the raw ABI sequence, bit for bit");
    };

    eslam_ns::Affine3d T = contact_step(0.02);
    EXPECT(get_map(ef.estimator().handle(), &before), "get_map");
    sensor(false, T, true);                                  // the first scan after init maps
    if (shared) EXPECT(same_map(mf, before), "the laser path does not merge on the shared map");
    else EXPECT(cells > 0, "the laser path merged into the particles' maps");
    cells_before = cells;
    sensor(false, T, false);                                 // unmoved: no
    sensor(true, T, true);                                   // the first image after init maps
    if (shared) EXPECT(!same_map(mf, before), "the camera path merges on the shared map (its patches fuse with the floor's)");
    else EXPECT(cells > cells_before, "the camera path merged into the particles' maps");
    sensor(true, T, false);                                  // unmoved: no
    T = contact_step(0.1);                                   // past mappingThreshold (5 deg read as 0.087 m, Q6)
    sensor(false, T, true);
    sensor(true, T, false);                                  // not past mappingCameraThreshold (0.52 m)
    sensor(false, T, false);
    T = contact_step(0.6);
    sensor(true, T, true);
    sensor(false, T, true);
    contact_step(0.02);                                      // a step on what the updates left
    compare("a step after the sensor updates");
}

// reference-shaped stand-ins (base::samples::LaserScan / DistanceImage: same member names, other classes)
struct RefLaserScan {
    double start_angle, angular_resolution, speed;
    std::vector<uint32_t> ranges;
    uint32_t minRange, maxRange;
    std::vector<float> remission;
};
struct RefDistanceImage {
    uint16_t width, height;
    float scale_x, scale_y, center_x, center_y;
    std::vector<float> data;
};

static void adapters()
{
    g_mode = "adapters";
    const RefLaserScan rl = {-1.5, 0.25, 0.0, {7u, 1200u, 3u}, 20u, 30000u, {}};
    const eslam_ns::LaserScan l = eslam_ns::toLaserScan(rl);
    EXPECT(l.start_angle == -1.5 && l.angular_resolution == 0.25 && l.ranges == rl.ranges && l.minRange == 20 && l.maxRange == 30000,
           "toLaserScan");
    const RefDistanceImage ri = {3, 2, 0.5f, 0.25f, -0.5f, -0.125f, {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}};
    const eslam_ns::DistanceImage d = eslam_ns::toDistanceImage(ri);
    EXPECT(d.width == 3 && d.height == 2 && d.scale_x == 0.5 && d.scale_y == 0.25 && d.center_x == -0.5 && d.center_y == -0.125 &&
               d.data == ri.data,
           "toDistanceImage");
}

int main()
{
    adapters();
    run(true);
    run(false);
    std::printf(fails ? "facade scan: %d FAILED\n" : "facade scan OK\n", fails);
    return fails ? 1 : 0;
}
