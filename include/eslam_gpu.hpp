// eslam_gpu.hpp -- C++ façade over the C ABI (eslam_gpu.h) with the reference's class API.
//
// The reference's callers (the Rock orogen task, viz/) use these classes directly; this
// header gives them the same names, constructors, method signatures, configuration fields
// and exception texts, over the MI355X library:
//   eslam::Configuration, ContactModelConfiguration, SurfaceHashConfig, UpdateThreshold
//                               src/Configuration.hpp:12-213
//   eslam::EmbodiedSlamFilter   src/EmbodiedSlamFilter.hpp:58-74 (contact path)
//   eslam::PoseEstimator        src/PoseEstimator.hpp:120-134
//   ParticleFilter<T>           src/ParticleFilter.hpp:34-173 (members of PoseEstimator)
//   eslam::PoseParticle / ContactPoint / PoseDistribution   src/PoseParticle.hpp:20-114
// A call site ports by switching the namespace to eslam::gpu.  The Eigen, base-types,
// odometry and envire types the reference signatures take are not in this image; the
// header carries small stand-ins with the same member names (Vector3d::x(), Affine3d::
// linear() / translation(), Quaterniond(w, x, y, z), base::Pose, BodyContactState::points,
// ...) and templated adapters (toGpu, toAffine, toContactState) that accept the real
// types by those member names.  The map handed to init() is an MlsGrid (the envire
// MLSGrid that EmbodiedSlamFilter::init finds in the environment); odometry::FootContact
// is the contact-odometry front end below.  Header-only; link libeslam_gpu.so.
#ifndef ESLAM_GPU_HPP
#define ESLAM_GPU_HPP

#include <cmath>
#include <cstdint>
#include <cstring>
#include <istream>
#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "eslam_gpu.h"

namespace eslam {
namespace gpu {

// ---------------------------------------------------------------------------------------
// Eigen-shaped stand-ins (the members the reference's call sites use)
// ---------------------------------------------------------------------------------------
struct Vector2d {
    double v[2] = {0, 0};
    Vector2d() = default;
    Vector2d(double x, double y) : v{x, y} {}
    double& x() { return v[0]; }
    double& y() { return v[1]; }
    double x() const { return v[0]; }
    double y() const { return v[1]; }
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    double operator()(int i) const { return v[i]; }
};

struct Vector3d {
    double v[3] = {0, 0, 0};
    Vector3d() = default;
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    static Vector3d Zero() { return Vector3d(); }
    static Vector3d UnitZ() { return Vector3d(0, 0, 1); }
    double& x() { return v[0]; }
    double& y() { return v[1]; }
    double& z() { return v[2]; }
    double x() const { return v[0]; }
    double y() const { return v[1]; }
    double z() const { return v[2]; }
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    double operator()(int i) const { return v[i]; }
    double norm() const { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
    Vector3d operator+(const Vector3d& o) const { return Vector3d(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
    Vector3d operator-(const Vector3d& o) const { return Vector3d(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
    Vector3d operator*(double s) const { return Vector3d(v[0] * s, v[1] * s, v[2] * s); }
};

struct Matrix3d {
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // row-major
    static Matrix3d Identity()
    {
        Matrix3d r;
        r.m[0] = r.m[4] = r.m[8] = 1.0;
        return r;
    }
    double& operator()(int r, int c) { return m[r * 3 + c]; }
    double operator()(int r, int c) const { return m[r * 3 + c]; }
    Vector3d operator*(const Vector3d& p) const
    {
        Vector3d o;
        for (int r = 0; r < 3; ++r) o.v[r] = (m[r * 3] * p.v[0] + m[r * 3 + 1] * p.v[1]) + m[r * 3 + 2] * p.v[2];
        return o;
    }
    Matrix3d operator*(const Matrix3d& b) const
    {
        Matrix3d o;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) o.m[r * 3 + c] = m[r * 3] * b.m[c] + m[r * 3 + 1] * b.m[3 + c] + m[r * 3 + 2] * b.m[6 + c];
        return o;
    }
    Matrix3d transpose() const
    {
        Matrix3d o;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) o.m[c * 3 + r] = m[r * 3 + c];
        return o;
    }
};

struct Quaterniond {
    double w_ = 1, x_ = 0, y_ = 0, z_ = 0;
    Quaterniond() = default;
    Quaterniond(double w, double x, double y, double z) : w_(w), x_(x), y_(y), z_(z) {}
    explicit Quaterniond(const Matrix3d& R)        // Eigen's rotation-matrix constructor
    {
        const double t = R(0, 0) + R(1, 1) + R(2, 2);
        if (t > 0) {
            const double s = std::sqrt(t + 1.0) * 2;
            w_ = 0.25 * s; x_ = (R(2, 1) - R(1, 2)) / s; y_ = (R(0, 2) - R(2, 0)) / s; z_ = (R(1, 0) - R(0, 1)) / s;
        } else if (R(0, 0) > R(1, 1) && R(0, 0) > R(2, 2)) {
            const double s = std::sqrt(1.0 + R(0, 0) - R(1, 1) - R(2, 2)) * 2;
            w_ = (R(2, 1) - R(1, 2)) / s; x_ = 0.25 * s; y_ = (R(0, 1) + R(1, 0)) / s; z_ = (R(0, 2) + R(2, 0)) / s;
        } else if (R(1, 1) > R(2, 2)) {
            const double s = std::sqrt(1.0 + R(1, 1) - R(0, 0) - R(2, 2)) * 2;
            w_ = (R(0, 2) - R(2, 0)) / s; x_ = (R(0, 1) + R(1, 0)) / s; y_ = 0.25 * s; z_ = (R(1, 2) + R(2, 1)) / s;
        } else {
            const double s = std::sqrt(1.0 + R(2, 2) - R(0, 0) - R(1, 1)) * 2;
            w_ = (R(1, 0) - R(0, 1)) / s; x_ = (R(0, 2) + R(2, 0)) / s; y_ = (R(1, 2) + R(2, 1)) / s; z_ = 0.25 * s;
        }
    }
    static Quaterniond Identity() { return Quaterniond(); }
    double w() const { return w_; }
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    Quaterniond conjugate() const { return Quaterniond(w_, -x_, -y_, -z_); }
    Quaterniond inverse() const { return conjugate(); }   // unit quaternions
    Quaterniond operator*(const Quaterniond& b) const
    {
        return Quaterniond(w_ * b.w_ - x_ * b.x_ - y_ * b.y_ - z_ * b.z_, w_ * b.x_ + x_ * b.w_ + y_ * b.z_ - z_ * b.y_,
                           w_ * b.y_ - x_ * b.z_ + y_ * b.w_ + z_ * b.x_, w_ * b.z_ + x_ * b.y_ - y_ * b.x_ + z_ * b.w_);
    }
    Matrix3d toRotationMatrix() const
    {
        Matrix3d R;
        const double w = w_, x = x_, y = y_, z = z_;
        R.m[0] = 1 - 2 * (y * y + z * z); R.m[1] = 2 * (x * y - w * z); R.m[2] = 2 * (x * z + w * y);
        R.m[3] = 2 * (x * y + w * z); R.m[4] = 1 - 2 * (x * x + z * z); R.m[5] = 2 * (y * z - w * x);
        R.m[6] = 2 * (x * z - w * y); R.m[7] = 2 * (y * z + w * x); R.m[8] = 1 - 2 * (x * x + y * y);
        return R;
    }
    Vector3d operator*(const Vector3d& p) const { return toRotationMatrix() * p; }
};

struct Affine3d {
    Matrix3d R = Matrix3d::Identity();
    Vector3d t;
    static Affine3d Identity() { return Affine3d(); }
    Matrix3d& linear() { return R; }
    const Matrix3d& linear() const { return R; }
    Vector3d& translation() { return t; }
    const Vector3d& translation() const { return t; }
    Affine3d operator*(const Affine3d& b) const
    {
        Affine3d o;
        o.R = R * b.R;
        o.t = R * b.t + t;
        return o;
    }
    Vector3d operator*(const Vector3d& p) const { return R * p + t; }
    Affine3d inverse() const
    {
        Affine3d o;
        o.R = R.transpose();
        o.t = (o.R * t) * -1.0;
        return o;
    }
};

// base::Pose2D / base::Pose
struct Pose2D {
    Vector2d position;
    double orientation = 0;
    Pose2D() = default;
    Pose2D(const Vector2d& p, double o) : position(p), orientation(o) {}
};

struct Pose {
    Vector3d position;
    Quaterniond orientation;
    Pose() = default;
    Pose(const Vector3d& p, const Quaterniond& q) : position(p), orientation(q) {}
    explicit Pose(const Affine3d& T) : position(T.translation()), orientation(T.linear()) {}
    Affine3d toTransform() const
    {
        Affine3d T;
        T.R = orientation.toRotationMatrix();
        T.t = position;
        return T;
    }
};

// odometry::BodyContactPoint / BodyContactState; terrain_estimator::TerrainClassification
struct BodyContactPoint {
    Vector3d position;
    float contact = 1.0f;                 // NaN (unknown) passes the contact gate (Q13)
    int groupId = -1;
    float slip = 0.0f;
};

struct BodyContactState {
    std::vector<BodyContactPoint> points;
    double time = 0;
};

struct TerrainClassification {};          // only counted (ltc.size() > 0 forces an update)

// ---------------------------------------------------------------------------------------
// Configuration  src/Configuration.hpp:12-213 (same fields and defaults)
// ---------------------------------------------------------------------------------------
struct UpdateThreshold {
    UpdateThreshold() {}
    UpdateThreshold(double distance, double angle) : distance(distance), angle(angle) {}
    bool test(double distance, double angle) const { return distance > this->distance || angle > this->angle; }
    // test(const Eigen::Affine3d&)  src/Configuration.hpp:23-26: the rotation angle
    // (Eigen::AngleAxisd(linear()).angle() = 2 atan2(|q.vec|, |q.w|)) goes in as the distance and
    // the translation's norm as the angle (Q6, kept)
    bool test(const Affine3d& pdelta) const
    {
        const Quaterniond q(pdelta.linear());
        const double n = std::sqrt(q.x() * q.x() + q.y() * q.y() + q.z() * q.z());
        const double a = n != 0.0 ? 2.0 * std::atan2(n, std::fabs(q.w())) : 0.0;
        const Vector3d& t = pdelta.translation();
        return test(a, std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
    }
    double distance = 0;
    double angle = 0;
};

struct SurfaceHashConfig {
    bool useHash = false;
    size_t period = 10;
    double percentage = 0.05;
    double avgFactor = 0.1;
    size_t slopeBins = 20;
    size_t angularSteps = 16;
};

struct ContactModelConfiguration {
    bool useSlipUpdate = false;
    bool useShapeUpdate = true;
    size_t minContacts = 3;
    double contactLikelihoodCorrection = 0.33;
    double contactPointRadius = 0.01;
};

struct Configuration {
    unsigned long seed = 42u;
    size_t particleCount = 250;
    size_t minEffective = 50;
    Vector3d initialRotationError = Vector3d(0, 0, 0.1);
    Vector3d initialTranslationError = Vector3d(0.1, 0.1, 1.0);
    double measurementError = 0.1;
    double discountFactor = 0.9;
    double spreadThreshold = 0.9;
    double spreadTranslationFactor = 0.1;
    double spreadRotationFactor = 0.05;
    double slipFactor = 0.05;
    double maxYawDeviation = 15 * M_PI / 180.0;
    UpdateThreshold measurementThreshold = UpdateThreshold(0.1, 10 * M_PI / 180.0);
    UpdateThreshold mappingThreshold = UpdateThreshold(0.02, 5 * M_PI / 180.0);
    UpdateThreshold mappingCameraThreshold = UpdateThreshold(1.0, 30 * M_PI / 180.0);
    double gridSize = 20.0;
    double gridResolution = 0.05;
    double gridThreshold = 0.5;
    double gridPatchThickness = 0.1;
    double gridGapSize = 1.5;
    bool gridUseNegativeInformation = false;
    double maxSensorRange = 3.0;
    bool useVisualUpdate = false;
    ContactModelConfiguration contactModel;
    bool logDebug = false;
    unsigned int logParticlePeriod = 100;
    uint32_t flags = 0;                   // build-specific ESLAM_FLAG_* (not in the reference)
    uint32_t localMapPages = 0;           // build-specific: per-particle map page pool per particle (0: 16)
    uint32_t localMapTrail = 16;          // build-specific: tiles a particle's map keeps behind its window
    uint32_t sumChunkRows = 0;            // build-specific: eslam_config::sum_chunk_rows (0: by particle count)

    // the fields the MI355X path consumes, as the C ABI's POD (hash: the init() argument)
    eslam_config toC(const SurfaceHashConfig& hash = SurfaceHashConfig()) const
    {
        eslam_config c;
        eslam_config_default(&c);
        c.seed = seed;
        c.particle_count = particleCount;
        c.min_effective = minEffective;
        for (int i = 0; i < 3; ++i) {
            c.initial_rotation_error[i] = initialRotationError[i];
            c.initial_translation_error[i] = initialTranslationError[i];
        }
        c.measurement_error = measurementError;
        c.discount_factor = discountFactor;
        c.spread_threshold = spreadThreshold;
        c.spread_translation_factor = spreadTranslationFactor;
        c.spread_rotation_factor = spreadRotationFactor;
        c.slip_factor = slipFactor;
        c.max_yaw_deviation = maxYawDeviation;
        c.measurement_threshold_distance = measurementThreshold.distance;
        c.measurement_threshold_angle = measurementThreshold.angle;
        c.use_slip_update = contactModel.useSlipUpdate;
        c.use_shape_update = contactModel.useShapeUpdate;
        c.min_contacts = contactModel.minContacts;
        c.contact_likelihood_correction = contactModel.contactLikelihoodCorrection;
        c.contact_point_radius = contactModel.contactPointRadius;
        c.hash_use = hash.useHash;
        c.hash_period = hash.period;
        c.hash_percentage = hash.percentage;
        c.hash_avg_factor = hash.avgFactor;
        c.hash_slope_bins = hash.slopeBins;
        c.hash_angular_steps = hash.angularSteps;
        c.log_debug = logDebug;
        c.flags = flags;
        c.max_sensor_range = maxSensorRange;       // the reach of a particle's own map
        c.local_map_pages = localMapPages;
        c.local_map_trail = localMapTrail;
        c.sum_chunk_rows = sumChunkRows;
        return c;
    }
};

// ---------------------------------------------------------------------------------------
// adapters from the reference's own types (templated on their member names, so they take
// eslam::Configuration, Eigen::Affine3d, odometry::BodyContactState, ... as they are)
// ---------------------------------------------------------------------------------------
template <class V> inline Vector3d toVector3(const V& v) { return Vector3d(v[0], v[1], v[2]); }

// eslam::Configuration -> eslam::gpu::Configuration (src/Configuration.hpp:76-211)
template <class RefConfig> Configuration toGpu(const RefConfig& r)
{
    Configuration c;
    c.seed = r.seed;
    c.particleCount = r.particleCount;
    c.minEffective = r.minEffective;
    c.initialRotationError = toVector3(r.initialRotationError);
    c.initialTranslationError = toVector3(r.initialTranslationError);
    c.measurementError = r.measurementError;
    c.discountFactor = r.discountFactor;
    c.spreadThreshold = r.spreadThreshold;
    c.spreadTranslationFactor = r.spreadTranslationFactor;
    c.spreadRotationFactor = r.spreadRotationFactor;
    c.slipFactor = r.slipFactor;
    c.maxYawDeviation = r.maxYawDeviation;
    c.measurementThreshold = UpdateThreshold(r.measurementThreshold.distance, r.measurementThreshold.angle);
    c.mappingThreshold = UpdateThreshold(r.mappingThreshold.distance, r.mappingThreshold.angle);
    c.mappingCameraThreshold = UpdateThreshold(r.mappingCameraThreshold.distance, r.mappingCameraThreshold.angle);
    c.gridSize = r.gridSize;
    c.gridResolution = r.gridResolution;
    c.gridThreshold = r.gridThreshold;
    c.gridPatchThickness = r.gridPatchThickness;
    c.gridGapSize = r.gridGapSize;
    c.gridUseNegativeInformation = r.gridUseNegativeInformation;
    c.maxSensorRange = r.maxSensorRange;
    c.useVisualUpdate = r.useVisualUpdate;
    c.contactModel.useSlipUpdate = r.contactModel.useSlipUpdate;
    c.contactModel.useShapeUpdate = r.contactModel.useShapeUpdate;
    c.contactModel.minContacts = r.contactModel.minContacts;
    c.contactModel.contactLikelihoodCorrection = r.contactModel.contactLikelihoodCorrection;
    c.contactModel.contactPointRadius = r.contactModel.contactPointRadius;
    c.logDebug = r.logDebug;
    c.logParticlePeriod = r.logParticlePeriod;
    return c;
}

template <class RefHash> SurfaceHashConfig toGpuHash(const RefHash& r)
{
    SurfaceHashConfig h;
    h.useHash = r.useHash;
    h.period = r.period;
    h.percentage = r.percentage;
    h.avgFactor = r.avgFactor;
    h.slopeBins = r.slopeBins;
    h.angularSteps = r.angularSteps;
    return h;
}

// Eigen::Affine3d (or anything with linear()(r, c) and translation()[i])
template <class A> Affine3d toAffine(const A& T)
{
    Affine3d o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.R(r, c) = T.linear()(r, c);
        o.t[r] = T.translation()[r];
    }
    return o;
}

// odometry::BodyContactState (points[i].position / contact / groupId)
template <class BS> BodyContactState toContactState(const BS& bs)
{
    BodyContactState o;
    o.points.resize(bs.points.size());
    for (size_t i = 0; i < bs.points.size(); ++i) {
        o.points[i].position = toVector3(bs.points[i].position);
        o.points[i].contact = bs.points[i].contact;
        o.points[i].groupId = bs.points[i].groupId;
    }
    return o;
}

// ---------------------------------------------------------------------------------------
// MLS grid (the envire::MLSGrid EmbodiedSlamFilter::init takes from the environment) and
// ContactPoint / PoseParticle / PoseDistribution
// ---------------------------------------------------------------------------------------
struct MlsGrid {
    uint32_t width = 0, height = 0;
    double scaleX = 0.1, scaleY = 0.1, offsetX = 0, offsetY = 0;
    Affine3d global2local;                // GridAccess::C_global2local (src/PoseEstimator.hpp:65-71)
    std::vector<uint32_t> cellStart;      // width * height + 1 (CSR; cell = n * width + m)
    std::vector<float> mean, stdev, patchHeight;   // per patch; patchHeight empty = horizontal

    eslam_mls_grid toC() const
    {
        eslam_mls_grid g;
        std::memset(&g, 0, sizeof(g));
        g.width = width;
        g.height = height;
        g.scale_x = scaleX;
        g.scale_y = scaleY;
        g.offset_x = offsetX;
        g.offset_y = offsetY;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) g.global2local[r * 4 + c] = global2local.R(r, c);
            g.global2local[r * 4 + 3] = global2local.t[r];
        }
        g.cell_start = cellStart.data();
        g.patch_mean = mean.data();
        g.patch_stdev = stdev.data();
        g.patch_height = patchHeight.empty() ? nullptr : patchHeight.data();
        g.n_patches = mean.size();
        return g;
    }
};

struct ContactPoint {                     // src/PoseParticle.hpp:20-43
    Vector3d point;
    double zdiff = INFINITY, zvar = INFINITY, prob = 1.0;
};

struct PoseParticle {                     // src/PoseParticle.hpp:52-86
    Vector2d position;
    double orientation = 0;
    double zPos = 0, zSigma = 0;
    double mprob = 0;
    bool floating = true;
    std::vector<ContactPoint> cpoints;    // filled with Configuration::logDebug (or ESLAM_FLAG_RECORD_CONTACTS)
    std::vector<ContactPoint> spoints;    // slip points: empty (useSlipUpdate's color matching is not on this path)
    Vector3d meas_pos;
    double meas_theta = 0;
    double weight = 0;
};

// The 2-D Gaussian mixture over the particles' (x, y) (PoseDistribution::GMM, src/PoseParticle.hpp:
// 88-114: envire's GaussianMixture<double, 2>), read as the viewer reads it
// (viz/ParticleVisualization.cpp:98-107): params[i].weight, params[i].dist.mean, params[i].dist.cov.
// Fitted on the device by eslam_gpu_fit_pose_gmm (the rule is this build's own).
struct Matrix2d {
    double m[4] = {0, 0, 0, 0};           // row-major
    double& operator()(int r, int c) { return m[r * 2 + c]; }
    double operator()(int r, int c) const { return m[r * 2 + c]; }
};
struct Gaussian2D {
    Vector2d mean;
    Matrix2d cov;
};
struct GaussianMixture2D {
    struct Parameter {
        double weight = 0;
        Gaussian2D dist;
    };
    std::vector<Parameter> params;        // the live components only, in slab order
    // of the fit that filled it (eslam_gmm_info): log_likelihood is that of the parameters before
    // the last M-step
    eslam_gmm_info info = {};
};
struct GmmParams {                        // eslam_gmm_params_default
    unsigned components = 3, maxIterations = 10;
    double tolerance = 1e-5, minVariance = 1e-6;
};

// The gate of poseMoments(): the ellipse (p - centre)^T cov^-1 (p - centre) <= chi2 over p = (x, y)
// (eslam_pose_gate).  From a mixture's component and a sigma count: its mean, its covariance and
// chi2 = sigmas^2, so 3 is the component's 3-sigma ellipse.
struct PoseGate {
    Vector2d centre;
    Matrix2d cov;                         // symmetric: (0, 1) is read
    double chi2 = 9.0;
    PoseGate() { cov(0, 0) = cov(1, 1) = 1.0; }
    PoseGate(const Vector2d& c, const Matrix2d& a, double chi2_) : centre(c), cov(a), chi2(chi2_) {}
    PoseGate(const GaussianMixture2D::Parameter& component, double sigmas)
        : centre(component.dist.mean), cov(component.dist.cov), chi2(sigmas * sigmas) {}
    eslam_pose_gate c() const
    {
        eslam_pose_gate g;
        g.centre[0] = centre[0];
        g.centre[1] = centre[1];
        g.cov[0] = cov(0, 0);
        g.cov[1] = cov(0, 1);
        g.cov[2] = cov(1, 1);
        g.chi2 = chi2;
        return g;
    }
};

// The pose estimate with its covariance (eslam_gpu_pose_moments; the rule is this build's own,
// DESIGN.md 5i): the fields of eslam_pose_moments, and the yaw-free body orientation of the last
// step that pose() composes the orientation with.
struct PoseMoments {
    eslam_pose_moments m = {};
    Quaterniond zCompensatedOrientation;
    uint64_t particlesCounted() const { return m.particles_counted; }
    uint64_t particlesGatedOut() const { return m.particles_gated_out; }
    uint64_t particlesSkipped() const { return m.particles_skipped; }
    Vector3d position() const { return Vector3d(m.mean[0], m.mean[1], m.mean[2]); }
    double yaw() const { return m.mean[3]; }                  // the circular mean, in (-pi, pi]
    double cov(int r, int c) const { return m.cov[4 * r + c]; }   // over (x, y, z, yaw deviation)
    double zWithin() const { return m.z_within; }             // add to cov(2, 2) for the total z variance
    double yawResultant() const { return m.yaw_resultant; }
    double effective() const { return m.effective; }
    double weightShare() const { return m.weight_share; }
    // the mean as getCentroid composes its pose (src/PoseEstimator.cpp:378-382): the yaw about Z,
    // then zCompensatedOrientation
    Pose pose() const
    {
        const double ha = 0.5 * m.mean[3];
        return Pose(position(), Quaterniond(std::cos(ha), 0.0, 0.0, std::sin(ha)) * zCompensatedOrientation);
    }
};

// KLD-sampling's parameters (eslam_kld_params_default).  nMin 0: the configured
// particle count.
struct KldParams {
    double binXY = 0.1;                   // metres
    unsigned thetaBins = 36;              // yaw bins per turn
    bool multinomial = false;             // resampleKld: resample_multinomial instead of _stratified
    double epsilon = 0.05, zQuantile = 2.3263478740408408;      // the KL bound; delta = 0.01
    uint64_t nMin = 0, nMax = 0;          // nMax 0: only the call's own limits
    double minChange = 0;                 // hysteresis, a fraction of the current count
    uint64_t maxBins = 0;                 // bitmap bits; 0 = 2^27
};

struct PoseDistribution {                 // src/PoseParticle.hpp:88-114
    typedef GaussianMixture2D GMM;
    double time = 0;
    std::vector<PoseParticle> particles;
    GMM gmm;                              // empty unless asked for (getPoseDistribution(stride, GmmParams))
    Quaterniond orientation;
    BodyContactState bodyState;
};

inline void check(eslam_ctx* ctx, int rc)
{
    if (rc != ESLAM_OK) throw std::runtime_error(eslam_gpu_last_error(ctx));
}

// ---------------------------------------------------------------------------------------
// FootContact: contact-odometry front end (stands in for odometry::FootContact, which the
// reference links from the external odometry package; its algorithm is not in the
// reference, so this one is the build's own and parity-unpinned).  Between two body
// states, every contact point in stance in both (contact >= stanceThreshold, same index)
// is taken to be fixed in the world: the body moved by the mean of R_prev p_prev - R_cur p_cur
// over those points.  The error grows with the travelled distance (constError +
// distError * |delta|, per axis).  It answers what PoseEstimator::project asks
// (src/PoseEstimator.cpp:188-198): getPoseDelta(), getPositionError() and the Gaussian
// getPoseDeltaSample2D() draws from (mean dx, dy, dyaw in the heading frame; diagonal cov).
// ---------------------------------------------------------------------------------------
struct OdometryConfiguration {
    float stanceThreshold = 0.5f;
    Vector3d constError = Vector3d(0.001, 0.001, 0.001);   // position sigma per step (m)
    Vector3d distError = Vector3d(0.05, 0.05, 0.05);       // position sigma per metre travelled
    double constYawError = 1e-3;                            // rad per step
    double distYawError = 0.01;                             // rad per metre
};

// plain values to and from a stream (EmbodiedSlamFilter::saveState / loadState)
namespace detail {
template <class T> inline void put(std::ostream& os, const T& v) { os.write(reinterpret_cast<const char*>(&v), sizeof(T)); }
template <class T> inline void get(std::istream& is, T& v)
{
    is.read(reinterpret_cast<char*>(&v), sizeof(T));
    if (!is) throw std::runtime_error("loadState: the stream ended early");
}
inline void putQ(std::ostream& os, const Quaterniond& q)
{
    const double v[4] = {q.w(), q.x(), q.y(), q.z()};
    put(os, v);
}
inline void getQ(std::istream& is, Quaterniond& q)
{
    double v[4];
    get(is, v);
    q = Quaterniond(v[0], v[1], v[2], v[3]);
}
inline void putV(std::ostream& os, const Vector3d& p)
{
    const double v[3] = {p[0], p[1], p[2]};
    put(os, v);
}
inline void getV(std::istream& is, Vector3d& p)
{
    double v[3];
    get(is, v);
    p = Vector3d(v[0], v[1], v[2]);
}
inline void putState(std::ostream& os, const BodyContactState& s)
{
    put(os, (uint64_t)s.points.size());
    put(os, s.time);
    for (const BodyContactPoint& p : s.points) {
        putV(os, p.position);
        put(os, p.contact);
        put(os, (int32_t)p.groupId);
        put(os, p.slip);
    }
}
inline void getState(std::istream& is, BodyContactState& s)
{
    uint64_t n = 0;
    get(is, n);
    if (n > 4096) throw std::runtime_error("loadState: bad body contact state");
    get(is, s.time);
    s.points.resize((size_t)n);
    for (BodyContactPoint& p : s.points) {
        int32_t g = 0;
        getV(is, p.position);
        get(is, p.contact);
        get(is, g);
        get(is, p.slip);
        p.groupId = g;
    }
}
}  // namespace detail

class FootContact {
public:
    explicit FootContact(const OdometryConfiguration& config = OdometryConfiguration()) : config_(config) {}

    // what the odometry carries from one update to the next (the configuration is the caller's)
    void saveState(std::ostream& os) const
    {
        detail::put(os, (uint32_t)(has_prev_ ? 1 : 0));
        detail::put(os, (int32_t)stance_);
        detail::putState(os, prev_);
        detail::putQ(os, prev_q_);
        detail::putV(os, delta_.position);
        detail::putQ(os, delta_.orientation);
        detail::put(os, mean2d_);
        detail::put(os, sigma_);
        detail::put(os, yawVar_);
    }
    void loadState(std::istream& is)
    {
        uint32_t hp = 0;
        int32_t st = 0;
        detail::get(is, hp);
        detail::get(is, st);
        detail::getState(is, prev_);
        detail::getQ(is, prev_q_);
        detail::getV(is, delta_.position);
        detail::getQ(is, delta_.orientation);
        detail::get(is, mean2d_);
        detail::get(is, sigma_);
        detail::get(is, yawVar_);
        has_prev_ = hp != 0;
        stance_ = st;
    }

    void update(const BodyContactState& state, const Quaterniond& orientation)
    {
        delta_ = Pose();
        Vector3d d;
        int n = 0;
        if (has_prev_) {
            const Matrix3d Rp = prev_q_.toRotationMatrix(), Rc = orientation.toRotationMatrix();
            for (size_t i = 0; i < state.points.size() && i < prev_.points.size(); ++i) {
                const BodyContactPoint &a = prev_.points[i], &b = state.points[i];
                if (!(a.contact >= config_.stanceThreshold) || !(b.contact >= config_.stanceThreshold)) continue;
                d = d + (Rp * a.position - Rc * b.position);
                ++n;
            }
            if (n) d = d * (1.0 / n);
            // body frame of the previous state
            delta_.position = Rp.transpose() * d;
            delta_.orientation = prev_q_.inverse() * orientation;
            const double yaw_p = yawOf(Rp), yaw_c = yawOf(Rc);
            const double c = std::cos(-yaw_p), s = std::sin(-yaw_p);
            mean2d_[0] = c * d[0] - s * d[1];
            mean2d_[1] = s * d[0] + c * d[1];
            mean2d_[2] = wrap(yaw_c - yaw_p);
        }
        const double dist = std::sqrt(mean2d_[0] * mean2d_[0] + mean2d_[1] * mean2d_[1]);
        for (int i = 0; i < 3; ++i) {
            const double s = config_.constError[i] + config_.distError[i] * dist;
            sigma_[i] = s * s;
        }
        const double sy = config_.constYawError + config_.distYawError * dist;
        yawVar_ = sy * sy;
        prev_ = state;
        prev_q_ = orientation;
        has_prev_ = true;
        stance_ = n;
    }
    const Pose& getPoseDelta() const { return delta_; }
    Matrix3d getPositionError() const
    {
        Matrix3d P;
        P(0, 0) = sigma_[0]; P(1, 1) = sigma_[1]; P(2, 2) = sigma_[2];
        return P;
    }
    // the Gaussian of getPoseDeltaSample2D(): mean (dx, dy, dyaw), covariance row-major
    void getSampleDistribution2D(double mean[3], double cov[9]) const
    {
        std::memcpy(mean, mean2d_, sizeof(mean2d_));
        std::memset(cov, 0, 9 * sizeof(double));
        cov[0] = sigma_[0]; cov[4] = sigma_[1]; cov[8] = yawVar_;
    }
    int stancePoints() const { return stance_; }

private:
    static double yawOf(const Matrix3d& R) { return std::atan2(R(1, 0), R(0, 0)); }
    static double wrap(double a) { return std::atan2(std::sin(a), std::cos(a)); }
    OdometryConfiguration config_;
    BodyContactState prev_;
    Quaterniond prev_q_;
    bool has_prev_ = false;
    Pose delta_;
    double mean2d_[3] = {0, 0, 0};
    double sigma_[3] = {0, 0, 0};
    double yawVar_ = 0;
    int stance_ = 0;
};

// ---------------------------------------------------------------------------------------
// PoseEstimator  src/PoseEstimator.hpp:120-134 (+ the ParticleFilter<T> members it inherits)
// ---------------------------------------------------------------------------------------
// one cell of the scan's MLS (the scanMap of processMap): position in the yaw-free body
// frame, sensor sigma
struct ScanPatch {
    Vector3d position;
    double stdev = 0.0;
};

// base::samples::LaserScan / base::samples::DistanceImage: the fields the scan MLS is built from
// (DESIGN.md 5f), under their own names
struct LaserScan {
    double start_angle = 0;               // radians, the first beam
    double angular_resolution = 0;        // radians between beams
    std::vector<uint32_t> ranges;         // millimetres; 1..5 are error codes
    uint32_t minRange = 0, maxRange = 0;  // millimetres
};

struct DistanceImage {
    uint32_t width = 0, height = 0;
    double scale_x = 1, scale_y = 1, center_x = 0, center_y = 0;   // x = (u scale_x + center_x) d
    std::vector<float> data;              // width * height, row-major, metres
};

template <class LS> LaserScan toLaserScan(const LS& s)
{
    LaserScan o;
    o.start_angle = s.start_angle;
    o.angular_resolution = s.angular_resolution;
    o.ranges.assign(s.ranges.begin(), s.ranges.end());
    o.minRange = s.minRange;
    o.maxRange = s.maxRange;
    return o;
}

template <class DI> DistanceImage toDistanceImage(const DI& d)
{
    DistanceImage o;
    o.width = d.width;
    o.height = d.height;
    o.scale_x = d.scale_x;
    o.scale_y = d.scale_y;
    o.center_x = d.center_x;
    o.center_y = d.center_y;
    o.data.assign(d.data.begin(), d.data.end());
    return o;
}

struct SurfaceHash {                      // src/SurfaceHash.hpp:155-231: built on the device
    SurfaceHashConfig config;
    void setConfiguration(const SurfaceHashConfig& c) { config = c; }
};

class PoseEstimator {
public:
    typedef PoseParticle Particle;

    // src/PoseEstimator.cpp:13-25; device: the MI355X (one per process; multi-GPU: setCommRccl)
    PoseEstimator(FootContact& odometry, const Configuration& config, int device = 0,
                  const SurfaceHashConfig& hash = SurfaceHashConfig())
        : odometry_(odometry), config_(config)
    {
        const eslam_config c = config.toC(hash);
        if (eslam_gpu_create(&c, device, &ctx_) != ESLAM_OK) throw std::runtime_error("eslam_gpu_create failed (no MI355X visible?)");
    }
    ~PoseEstimator() { eslam_gpu_destroy(ctx_); }   // never collective (include/eslam_gpu.h)
    // multi-GPU: the collective end of a sharded filter's life -- every rank calls it before
    // the filter is destroyed, completing an exchange the rank may still owe
    void finish() { check(ctx_, eslam_gpu_finish(ctx_)); }
    PoseEstimator(const PoseEstimator&) = delete;
    PoseEstimator& operator=(const PoseEstimator&) = delete;

    // setEnvironment(env, map, useShared)  src/PoseEstimator.cpp:49-62: useShared = false gives
    // every particle its own map (the shared grid plus its own patches; before init)
    void setEnvironment(const MlsGrid& env, bool useShared = true)
    {
        const eslam_mls_grid g = env.toC();
        check(ctx_, eslam_gpu_set_map(ctx_, &g));
        check(ctx_, eslam_gpu_set_particle_maps(ctx_, useShared ? 0 : 1));
        setGridGeometry(env);
    }
    // the geometry particleGrid() gives its grids (setEnvironment records it; an estimator that
    // took its map from a loaded state is told here): scale, offset and global2local of env
    void setGridGeometry(const MlsGrid& env)
    {
        geometry_ = MlsGrid();
        geometry_.scaleX = env.scaleX; geometry_.scaleY = env.scaleY;
        geometry_.offsetX = env.offsetX; geometry_.offsetY = env.offsetY;
        geometry_.global2local = env.global2local;
        has_geometry_ = true;
    }
    // particles[i].grid.getMap()  src/PoseEstimator.hpp:79-87 (GridAccess::getMap; the viewer's
    // viewMap(particle_idx) reads it, viz/EslamWidget.cpp:108-116): particle i's whole map -- its
    // own patch per cell, then the shared grid's -- composed on the device
    // (eslam_gpu_get_particle_grid), as an MlsGrid setEnvironment takes.  getPatch on it answers
    // as particle i's own lookups do.  useShared = false only; i is the local index on a sharded
    // estimator.
    MlsGrid particleGrid(size_t i)
    {
        if (!has_geometry_) throw std::runtime_error("particleGrid: no grid geometry (setEnvironment or setGridGeometry)");
        flush();
        uint32_t w = 0, h = 0;
        int heights = 0;
        uint64_t np = 0;
        check(ctx_, eslam_gpu_map_size(ctx_, &w, &h, nullptr, &heights));
        check(ctx_, eslam_gpu_particle_grid_size(ctx_, (uint64_t)i, &np));
        MlsGrid g = geometry_;
        g.width = w;
        g.height = h;
        g.cellStart.assign((size_t)w * h + 1, 0u);
        g.mean.assign(np, 0.0f);
        g.stdev.assign(np, 0.0f);
        if (heights) g.patchHeight.assign(np, 0.0f);
        // (non-null patch pointers for an empty grid too)
        float none = 0.0f;
        check(ctx_, eslam_gpu_get_particle_grid(ctx_, (uint64_t)i, g.cellStart.data(), np ? g.mean.data() : &none,
                                                np ? g.stdev.data() : &none, heights && np ? g.patchHeight.data() : nullptr, np));
        return g;
    }
    // continue in particle i's map (eslam_gpu_adopt_particle_map): as setEnvironment(particleGrid(i))
    // with the map mode kept and no host round trip -- the composed grid becomes the shared one and
    // every particle's own map starts over, empty.  One GPU only.
    void adoptParticleMap(size_t i)
    {
        flush();
        check(ctx_, eslam_gpu_adopt_particle_map(ctx_, (uint64_t)i));
    }
    // cloneMaps  src/PoseEstimator.cpp:31-47: the copies a resample made share their ancestor's
    // patches until the next map update gives each a private copy (copy on write), so there is
    // nothing to do here
    void cloneMaps() {}
    // the match half of EmbodiedSlamFilter::processMap(scanMap, match, update)
    // (src/EmbodiedSlamFilter.cpp:214-221): every particle's weight *= pow(weight, 0.1f)
    void matchMaps(const std::vector<ScanPatch>& scan)
    {
        flush();
        invalidate();
        std::vector<eslam_scan_patch> p(scan.size());
        for (size_t k = 0; k < scan.size(); ++k) {
            for (int i = 0; i < 3; ++i) p[k].position[i] = scan[k].position[i];
            p[k].stdev = scan[k].stdev;
        }
        check(ctx_, eslam_gpu_map_match(ctx_, p.data(), (uint32_t)p.size()));
    }
    // the merge half of EmbodiedSlamFilter::processMap(scanMap, match, update)
    // (src/EmbodiedSlamFilter.cpp:179-232) for per-particle maps: the scan's patches in the
    // yaw-free body frame, placed at every particle's pose
    void updateMaps(const std::vector<ScanPatch>& scan)
    {
        flush();
        std::vector<eslam_scan_patch> p(scan.size());
        for (size_t k = 0; k < scan.size(); ++k) {
            for (int i = 0; i < 3; ++i) p[k].position[i] = scan[k].position[i];
            p[k].stdev = scan[k].stdev;
        }
        check(ctx_, eslam_gpu_map_update(ctx_, p.data(), (uint32_t)p.size()));
    }
    // the same merge with the shared map (useShared = true: every particle's pgrid is the one
    // grid, src/EmbodiedSlamFilter.cpp:184-227): the scan goes into the shared grid once per
    // particle, at that particle's pose, in particle order (eslam_gpu_shared_map_update; the
    // particles do not change).  Returns the merge's counters.  On a sharded estimator this is
    // the collective eslam_gpu_shared_map_update_sharded: every rank must pass the same scan, and
    // every rank's copy of the grid ends as one GPU's would (global particle order).
    eslam_shared_merge_info updateSharedMap(const std::vector<ScanPatch>& scan, uint64_t maxRecords = 0)
    {
        flush();
        std::vector<eslam_scan_patch> p(scan.size());
        for (size_t k = 0; k < scan.size(); ++k) {
            for (int i = 0; i < 3; ++i) p[k].position[i] = scan[k].position[i];
            p[k].stdev = scan[k].stdev;
        }
        eslam_shared_merge_info info;
        if (sharded())
            check(ctx_, eslam_gpu_shared_map_update_sharded(ctx_, p.data(), (uint32_t)p.size(), maxRecords, &info));
        else
            check(ctx_, eslam_gpu_shared_map_update(ctx_, p.data(), (uint32_t)p.size(), maxRecords, &info));
        return info;
    }

    // The scan's MLS from a sensor reading, built on the device (eslam_gpu_scan_from_laser /
    // eslam_gpu_scan_from_depth): what the reference's ScanMeshing /
    // DistanceGridToPointcloud and MLSProjection hand to processMap.  sensor2body is laser2body
    // or camera2body, orientation the body's (body2odometry's rotation); the grid's resolution,
    // the patch thickness and the range come from the Configuration, the sigmas are the
    // reference's (src/EmbodiedSlamFilter.cpp:280-296, 322-336).
    eslam_scan_params scanParams(const Affine3d& sensor2body, const Quaterniond& orientation) const
    {
        eslam_scan_params p;
        const eslam_config c = config_.toC();
        eslam_scan_params_default(&c, &p);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) p.sensor2body[4 * r + k] = sensor2body.linear()(r, k);
            p.sensor2body[4 * r + 3] = sensor2body.translation()[r];
        }
        p.orientation[0] = orientation.w(); p.orientation[1] = orientation.x();
        p.orientation[2] = orientation.y(); p.orientation[3] = orientation.z();
        p.resolution = config_.gridResolution;
        p.patch_thickness = config_.gridPatchThickness;
        p.max_sensor_range = config_.maxSensorRange;
        return p;
    }
    std::vector<ScanPatch> scanFromLaser(const LaserScan& scan, const Affine3d& laser2body, const Quaterniond& orientation,
                                         eslam_scan_info* info = nullptr)
    {
        const eslam_scan_params p = scanParams(laser2body, orientation);
        eslam_laser_scan s;
        std::memset(&s, 0, sizeof(s));
        s.start_angle = scan.start_angle;
        s.angular_resolution = scan.angular_resolution;
        s.min_range = scan.minRange;
        s.max_range = scan.maxRange;
        s.n = (uint32_t)scan.ranges.size();
        s.ranges = scan.ranges.data();
        check(ctx_, eslam_gpu_scan_from_laser(ctx_, &s, &p, info));
        return lastScan();
    }
    std::vector<ScanPatch> scanFromDistanceImage(const DistanceImage& image, const Affine3d& camera2body,
                                                 const Quaterniond& orientation, eslam_scan_info* info = nullptr)
    {
        if (image.data.size() != (size_t)image.width * image.height)
            throw std::runtime_error("DistanceImage: data does not hold width * height pixels");
        const eslam_scan_params p = scanParams(camera2body, orientation);
        eslam_depth_image d;
        std::memset(&d, 0, sizeof(d));
        d.width = image.width;
        d.height = image.height;
        d.scale_x = image.scale_x; d.scale_y = image.scale_y;
        d.center_x = image.center_x; d.center_y = image.center_y;
        d.data = image.data.data();
        check(ctx_, eslam_gpu_scan_from_depth(ctx_, &d, &p, info));
        return lastScan();
    }
    // the last built scan's patches (eslam_gpu_scan_patches)
    std::vector<ScanPatch> lastScan()
    {
        uint64_t n = 0;
        check(ctx_, eslam_gpu_scan_patches(ctx_, nullptr, 0, &n));
        std::vector<eslam_scan_patch> raw(n);
        if (n) check(ctx_, eslam_gpu_scan_patches(ctx_, raw.data(), n, &n));
        std::vector<ScanPatch> out(raw.size());
        for (size_t k = 0; k < raw.size(); ++k) {
            out[k].position = Vector3d(raw[k].position[0], raw[k].position[1], raw[k].position[2]);
            out[k].stdev = raw[k].stdev;
        }
        return out;
    }

    // init(numParticles, hash)  src/PoseEstimator.cpp:75-86 (the hash is built on the device
    // from the environment's grid; the SurfaceHashConfig was given at construction)
    void init(int numParticles, SurfaceHash* hash)
    {
        if (!hash) throw std::runtime_error("could not sample from pose hash.");
        discardView();
        check(ctx_, eslam_gpu_hash_create(ctx_));
        check(ctx_, eslam_gpu_init_hash(ctx_, (uint64_t)numParticles));
    }
    // init(numParticles, mu, sigma, zpos, zsigma)  src/PoseEstimator.cpp:88-102
    void init(int numParticles, const Pose2D& mu, const Pose2D& sigma, double zpos = 0, double zsigma = 0)
    {
        const double m[3] = {mu.position.x(), mu.position.y(), mu.orientation};
        const double s[3] = {sigma.position.x(), sigma.position.y(), sigma.orientation};
        discardView();
        check(ctx_, eslam_gpu_init_gaussian(ctx_, (uint64_t)numParticles, m, s, zpos, zsigma));
    }

    // project(state, orientation)  src/PoseEstimator.cpp:184-242 (the odometry has been updated)
    void project(const BodyContactState& state, const Quaterniond& orientation)
    {
        const eslam_step_input in = makeInput(state, orientation, Vector3d(), 0);
        flush();
        invalidate();
        check(ctx_, eslam_gpu_project(ctx_, &in));
    }
    // update(state, orientation, ltc)  src/PoseEstimator.cpp:244-255
    void update(const BodyContactState& state, const Quaterniond& orientation, const std::vector<TerrainClassification>& ltc)
    {
        const eslam_step_input in = makeInput(state, orientation, Vector3d(), ltc.size());
        flush();
        invalidate();
        check(ctx_, eslam_gpu_update(ctx_, &in));
        check(ctx_, eslam_gpu_sync(ctx_, &last_));
    }

    // ParticleFilter<T>  src/ParticleFilter.hpp:34-173
    double getWeightsSum()
    {
        flush();
        double s = 0;
        check(ctx_, eslam_gpu_get_weights_sum(ctx_, &s));
        return s;
    }
    double getWeightAvg() { return getWeightsSum() / (double)size(); }
    double normalizeWeights()
    {
        flush();
        invalidate();
        double e = 0;
        check(ctx_, eslam_gpu_normalize_weights(ctx_, &e));
        return e;
    }
    void resample()
    {
        flush();
        invalidate();
        check(ctx_, eslam_gpu_resample(ctx_));
    }
    // resample_stratified(samples) / resample_multinomial(samples)  src/ParticleFilter.hpp:85-148:
    // to any count; getParticles() has the new size afterwards (eslam_gpu_resample_stratified /
    // _multinomial: the limits with per-particle maps and sharded filters, and samples == 0, are
    // errors there and exceptions here).  On a sharded estimator these are the collectives
    // eslam_gpu_resample_stratified_sharded / _multinomial_sharded: every rank calls with the
    // same count, the filter is laid out by the canonical table of the new count afterwards
    // (shardBounds()), and getParticles() has the rank's new local size.
    void resample_stratified(size_t samples)
    {
        flush();
        invalidate();
        if (sharded())
            check(ctx_, eslam_gpu_resample_stratified_sharded(ctx_, samples, &last_resample_));
        else
            check(ctx_, eslam_gpu_resample_stratified(ctx_, samples, &last_resample_));
    }
    void resample_multinomial(size_t samples)
    {
        flush();
        invalidate();
        if (sharded())
            check(ctx_, eslam_gpu_resample_multinomial_sharded(ctx_, samples, &last_resample_));
        else
            check(ctx_, eslam_gpu_resample_multinomial(ctx_, samples, &last_resample_));
    }
    const eslam_resample_info& lastResample() const { return last_resample_; }
    // KLD-sampling (eslam_gpu_kld_count): the occupied bins of the pose lattice over
    // the particles as they stand, counted on the device, and the count they ask for
    // (info.samples).  The filter is unchanged.  A collective on a sharded estimator.
    eslam_kld_info kldCount(const KldParams& kp = KldParams()) const
    {
        flush();
        const eslam_kld_params p = kldParams(kp);
        eslam_kld_info info = {};
        check(ctx_, eslam_gpu_kld_count(ctx_, &p, &info));
        return info;
    }
    // ... then the resample to that count (eslam_gpu_resample_kld): stratified, or multinomial
    // with kp.multinomial; getParticles() has the new size afterwards and, on a sharded estimator,
    // shardBounds() the new table.  lastKld() and lastResample() give the two infos; lastKld() is
    // filled as far as the call got when it throws.
    void resampleKld(const KldParams& kp = KldParams())
    {
        flush();
        invalidate();
        const eslam_kld_params p = kldParams(kp);
        check(ctx_, eslam_gpu_resample_kld(ctx_, &p, &last_kld_, &last_resample_));
    }
    const eslam_kld_info& lastKld() const { return last_kld_; }
    size_t getBestParticleIndex() const
    {
        flush();
        uint64_t i = 0;
        check(ctx_, eslam_gpu_get_best_particle_index(ctx_, &i));
        return (size_t)i;
    }
    // getCentroid  src/PoseEstimator.cpp:354-383 (normalises in place, Q15)
    Pose getCentroid()
    {
        flush();
        invalidate();                     // normalises the weights
        double p[3], q[4];
        check(ctx_, eslam_gpu_get_centroid(ctx_, p, q));
        return Pose(Vector3d(p[0], p[1], p[2]), Quaterniond(q[0], q[1], q[2], q[3]));
    }
    // the pose with its uncertainty: the Gaussian mixture over (x, y) of the particles as they
    // stand, fitted on the device (eslam_gpu_fit_pose_gmm); the filter is unchanged (no
    // normalisation, unlike getCentroid).  Live components only.
    GaussianMixture2D fitGmm(const GmmParams& gp = GmmParams()) const
    {
        flush();
        eslam_gmm_params p;
        p.components = gp.components;
        p.max_iterations = gp.maxIterations;
        p.tolerance = gp.tolerance;
        p.min_variance = gp.minVariance;
        eslam_gmm_component c[ESLAM_GMM_MAX_COMPONENTS] = {};
        GaussianMixture2D g;
        // components outside [1, 8] are refused before `c` is written
        check(ctx_, eslam_gpu_fit_pose_gmm(ctx_, &p, c, &g.info));
        for (unsigned k = 0; k < gp.components; ++k) {
            if (!(g.info.live_mask >> k & 1u)) continue;      // the library's own liveness decision
            GaussianMixture2D::Parameter q;
            q.weight = c[k].weight;
            q.dist.mean = Vector2d(c[k].mean[0], c[k].mean[1]);
            q.dist.cov(0, 0) = c[k].cov[0];
            q.dist.cov(0, 1) = q.dist.cov(1, 0) = c[k].cov[1];
            q.dist.cov(1, 1) = c[k].cov[2];
            g.params.push_back(q);
        }
        return g;
    }
    // the pose estimate with its 4 x 4 covariance over (x, y, z, yaw), summed on the device over
    // the particles as they stand, or over those inside `gate` (eslam_gpu_pose_moments); the filter
    // is unchanged.  The dominant cluster's estimate: fitGmm(), its heaviest component c, then
    // PoseGate g(c, 3) and poseMoments(&g).
    PoseMoments poseMoments(const PoseGate* gate = nullptr) const
    {
        flush();
        PoseMoments r;
        eslam_pose_gate g;
        if (gate) g = gate->c();
        check(ctx_, eslam_gpu_pose_moments(ctx_, gate ? &g : nullptr, &r.m));
        double q[4];
        check(ctx_, eslam_gpu_get_z_compensated_orientation(ctx_, q));
        r.zCompensatedOrientation = Quaterniond(q[0], q[1], q[2], q[3]);
        return r;
    }

    // The trajectory log (eslam_gpu_trajectory_*): what the reference keeps inside
    // each particle's map and in the logged PoseDistribution stream.  Once enabled, every update()
    // and every step of EmbodiedSlamFilter::update ends with a record on the device of the
    // particles' poses and ancestry, in a ring of `steps` entries of up to maxParticles particles
    // (0: the filter's capacity), 44 bytes per particle and entry.
    // A sharded estimator keeps the log too (eslam_gpu_trajectory_enable_sharded): the call is
    // then a collective, maxParticles is this rank's, and clearTrajectory(), trajectory() and
    // smoothedTrajectory() are collectives that give every rank the one-GPU answer.  The index
    // trajectory(i) takes is global there, which is what getBestParticleIndex() returns.
    void enableTrajectory(uint32_t steps, uint64_t maxParticles = 0)
    {
        flush();
        if (sharded())
            check(ctx_, eslam_gpu_trajectory_enable_sharded(ctx_, steps, maxParticles));
        else
            check(ctx_, eslam_gpu_trajectory_enable(ctx_, steps, maxParticles));
    }
    void disableTrajectory() { check(ctx_, eslam_gpu_trajectory_disable(ctx_)); }
    void clearTrajectory() { check(ctx_, eslam_gpu_trajectory_clear(ctx_)); }
    eslam_trajectory_info trajectoryInfo() const
    {
        eslam_trajectory_info info;
        check(ctx_, eslam_gpu_trajectory_info(ctx_, &info));
        return info;
    }
    // the lineage of the current particle i through the held entries, oldest first
    std::vector<eslam_trajectory_pose> trajectory(size_t i) const
    {
        flush();
        std::vector<eslam_trajectory_pose> path(trajectoryInfo().entries);
        const uint64_t index = i;
        uint64_t steps = 0;
        check(ctx_, eslam_gpu_get_trajectories(ctx_, &index, 1, path.data(), path.size(), &steps));
        path.resize(steps);
        return path;
    }
    // per held entry, oldest first: the pose moments of the current particles' ancestors in it
    // under the current weights (the fixed-lag smoothed estimate) and their distinct count
    std::vector<eslam_trajectory_estimate> smoothedTrajectory() const
    {
        flush();
        std::vector<eslam_trajectory_estimate> est(trajectoryInfo().entries);
        uint64_t entries = 0;
        check(ctx_, eslam_gpu_trajectory_smoothed(ctx_, est.data(), est.size(), &entries));
        est.resize(entries);
        return est;
    }

    // getParticles(): the particles as a vector the caller may edit, like the reference's
    // std::vector<Particle>& (src/ParticleFilter.hpp:150-153; processMap edits weights through
    // it, src/EmbodiedSlamFilter.cpp:183-220).  The particles live in HBM: the vector is
    // downloaded on first use after the device changed them, and edits -- pose, zPos, zSigma,
    // weight, mprob, floating, the number of cpoints, or the vector's size -- are written back
    // (eslam_gpu_write_particles, or a whole new set when the size changed) before the next
    // call that uses the particles on the device.  With logDebug it carries cpoints / meas_pos /
    // meas_theta of the last update.  The reference stays valid; its contents are those of the
    // last download.
    std::vector<Particle>& getParticles()
    {
        if (!view_valid_) {
            view_ = getParticles(0, 1, size());
            shadow_.resize(view_.size());
            for (size_t i = 0; i < view_.size(); ++i) shadow_[i] = hot(view_[i]);
            view_valid_ = true;
        }
        return view_;
    }
    // particles first, first + stride, ... (count): a device-side gather, for logging; a copy
    // (edits to it are not written back)
    std::vector<Particle> getParticles(size_t first, size_t stride, size_t count)
    {
        flush();
        std::vector<eslam_particle_record> rec(count);
        // contact points per particle: at most the contacts of the last step
        const uint32_t maxc = config_.logDebug || (config_.flags & ESLAM_FLAG_RECORD_CONTACTS) ? (last_m_ ? last_m_ : 1) : 0;
        std::vector<eslam_cpoint> cp(maxc ? count * maxc : 0);
        check(ctx_, eslam_gpu_download_records(ctx_, first, stride, count, rec.data(), maxc ? cp.data() : nullptr, maxc));
        std::vector<Particle> particles(count);
        for (size_t k = 0; k < count; ++k) {
            const eslam_particle_record& r = rec[k];
            Particle& p = particles[k];
            p.position = Vector2d(r.position[0], r.position[1]);
            p.orientation = r.orientation;
            p.zPos = r.zpos;
            p.zSigma = r.zsigma;
            p.mprob = r.mprob;
            p.weight = r.weight;
            p.floating = r.floating != 0;
            p.meas_pos = Vector3d(r.meas_pos[0], r.meas_pos[1], r.meas_pos[2]);
            p.meas_theta = r.meas_theta;
            p.cpoints.clear();
            p.spoints.clear();
            if (maxc) {
                const uint32_t nc = r.n_cpoints < maxc ? r.n_cpoints : maxc;
                for (uint32_t q = 0; q < nc; ++q) {
                    const eslam_cpoint& c = cp[k * maxc + q];
                    ContactPoint o;
                    o.point = Vector3d(c.point[0], c.point[1], c.point[2]);
                    o.zdiff = c.zdiff;
                    o.zvar = c.zvar;
                    o.prob = c.prob;
                    p.cpoints.push_back(o);
                }
            } else {
                p.cpoints.resize(r.n_cpoints);        // the count (cpoints.size()) without the capture
            }
        }
        return particles;
    }
    void setParticles(const std::vector<Particle>& in)
    {
        discardView();
        replaceSet(in);
    }
    size_t size() const
    {
        uint64_t n = 0;
        check(ctx_, eslam_gpu_particle_count(ctx_, &n));
        return (size_t)n;
    }

private:
    eslam_kld_params kldParams(const KldParams& kp) const
    {
        eslam_kld_params p;
        const eslam_config c = config_.toC();
        eslam_kld_params_default(&c, &p);             // n_min: the configured particle count
        p.bin_xy = kp.binXY;
        p.theta_bins = kp.thetaBins;
        p.multinomial = kp.multinomial ? 1u : 0u;
        p.epsilon = kp.epsilon;
        p.z_quantile = kp.zQuantile;
        if (kp.nMin) p.n_min = kp.nMin;
        p.n_max = kp.nMax;
        p.min_change = kp.minChange;
        p.max_bins = kp.maxBins;
        return p;
    }
    void replaceSet(const std::vector<Particle>& in) const
    {
        const size_t n = in.size();
        std::vector<double> x(n), y(n), th(n), z(n), zs(n), w(n), mp(n);
        std::vector<uint8_t> fl(n), nc(n);
        for (size_t i = 0; i < n; ++i) {
            x[i] = in[i].position.x(); y[i] = in[i].position.y(); th[i] = in[i].orientation; z[i] = in[i].zPos;
            zs[i] = in[i].zSigma; w[i] = in[i].weight; mp[i] = in[i].mprob; fl[i] = in[i].floating;
            nc[i] = (uint8_t)in[i].cpoints.size();
        }
        eslam_particles p = {x.data(), y.data(), th.data(), z.data(), zs.data(), w.data(), mp.data(), fl.data(), nc.data()};
        check(ctx_, eslam_gpu_upload_particles(ctx_, n, &p));
    }

public:

    // multi-GPU (the reference has one CPU filter): this estimator becomes shard `rank` of
    // an nGlobal-particle filter over an RCCL communicator the library drives.  Rank 0 calls
    // rcclUniqueId(), the caller broadcasts the id, every rank calls setCommRccl
    // (collective) before init; shardGbase: the first global index of every rank + nGlobal.
    static std::vector<uint8_t> rcclUniqueId()
    {
        std::vector<uint8_t> id(ESLAM_RCCL_ID_BYTES);
        if (eslam_gpu_rccl_unique_id(id.data()) != ESLAM_OK) throw std::runtime_error("eslam_gpu_rccl_unique_id failed");
        return id;
    }
    void setCommRccl(int nranks, int rank, const std::vector<uint8_t>& id, uint64_t nGlobal,
                     const std::vector<uint64_t>& shardGbase)
    {
        if (id.size() != ESLAM_RCCL_ID_BYTES || shardGbase.size() != (size_t)nranks + 1)
            throw std::runtime_error("setCommRccl: bad id or shard table");
        check(ctx_, eslam_gpu_set_comm_rccl(ctx_, nranks, rank, id.data(), nGlobal, shardGbase.data()));
        sharded_ = nranks > 0;
        rank_ = rank;
    }
    // the same with caller-supplied collectives (eslam_gpu_set_comm); comm == nullptr: one GPU
    void setComm(const eslam_comm* comm, uint64_t nGlobal, const std::vector<uint64_t>& shardGbase)
    {
        check(ctx_, eslam_gpu_set_comm(ctx_, comm, nGlobal, comm ? shardGbase.data() : nullptr));
        sharded_ = comm != nullptr;
        rank_ = comm ? comm->rank : 0;
    }
    bool sharded() const { return sharded_; }
    int rank() const { return rank_; }
    // the sharded estimator's current shard table: the first global index of every rank + the
    // global count (eslam_gpu_get_shard_bounds); a resample to another count changes it
    std::vector<uint64_t> shardBounds() const
    {
        uint64_t b[17] = {};
        check(ctx_, eslam_gpu_get_shard_bounds(ctx_, b, 17));
        size_t ranks = 1;
        while (ranks < 16 && b[ranks + 1] > b[ranks]) ++ranks;
        return std::vector<uint64_t>(b, b + ranks + 1);
    }
    // the canonical table of an nGlobal-particle filter over nranks ranks (eslam_gpu_shard_bounds)
    static std::vector<uint64_t> canonicalShardBounds(uint64_t nGlobal, int nranks, uint32_t sumChunkRows = 0)
    {
        std::vector<uint64_t> b((size_t)(nranks > 0 ? nranks : 0) + 1);
        if (eslam_gpu_shard_bounds(nGlobal, nranks, sumChunkRows, b.data()) != ESLAM_OK)
            throw std::runtime_error("eslam_gpu_shard_bounds: the count cannot be split over the ranks");
        return b;
    }

    // the device's snapshot as one file written and read by offset (eslam_gpu_save_at /
    // eslam_gpu_load_at): on a sharded estimator collectives, every rank writing and reading its
    // part of the one blob; returns what the call reports (bytes: the blob's size)
    eslam_snapshot_info saveAt(eslam_pwrite_fn pwrite, void* user, uint64_t chunkBytes = 0)
    {
        flush();
        eslam_snapshot_info info;
        check(ctx_, eslam_gpu_save_at(ctx_, pwrite, user, chunkBytes, &info));
        return info;
    }
    eslam_snapshot_info loadAt(eslam_pread_fn pread, void* user, uint64_t knownBytes = 0, uint64_t chunkBytes = 0)
    {
        eslam_snapshot_info info;
        const int rc = eslam_gpu_load_at(ctx_, pread, user, knownBytes, chunkBytes, &info);
        invalidate();
        check(ctx_, rc);
        return info;
    }

    // write the edits made to the getParticles() vector back to the device (a no-op without
    // any); every call above that uses the particles on the device runs it first.  On a
    // sharded filter the write-back is collective (eslam_gpu_write_particles): a rank holding
    // a view writes back even without edits, so the ranks stay matched as long as they call
    // getParticles() at the same points (SPMD order, include/eslam_gpu.h).  The contract is on
    // the caller: a rank that never took a view (view_valid_ false) skips the write-back, so
    // either every rank calls getParticles() at a point or none does
    void flush() const
    {
        if (!view_valid_) return;
        if (view_.size() != shadow_.size()) {          // the caller resized the set: replace it
            view_valid_ = false;
            replaceSet(view_);
            return;
        }
        size_t lo = view_.size(), hi = 0;
        for (size_t i = 0; i < view_.size(); ++i) {
            const Hot h = hot(view_[i]);
            if (std::memcmp(&h, &shadow_[i], sizeof(Hot)) != 0) {
                if (i < lo) lo = i;
                hi = i + 1;
                shadow_[i] = h;
            }
        }
        if (lo >= hi) {
            if (!sharded()) return;
            lo = hi = 0;
        }
        const size_t n = hi - lo;
        std::vector<double> x(n), y(n), th(n), z(n), zs(n), w(n), mp(n);
        std::vector<uint8_t> fl(n), nc(n);
        for (size_t k = 0; k < n; ++k) {
            const Hot& h = shadow_[lo + k];
            x[k] = h.v[0]; y[k] = h.v[1]; th[k] = h.v[2]; z[k] = h.v[3]; zs[k] = h.v[4]; w[k] = h.v[5]; mp[k] = h.v[6];
            fl[k] = h.floating; nc[k] = h.ncp;
        }
        eslam_particles p = {x.data(), y.data(), th.data(), z.data(), zs.data(), w.data(), mp.data(), fl.data(), nc.data()};
        check(ctx_, eslam_gpu_write_particles(ctx_, lo, n, &p));
    }
    // the device is about to change the particles: the next getParticles() downloads again
    void invalidate() { view_valid_ = false; }

    const eslam_update_info& lastUpdate() const { return last_; }
    eslam_ctx* handle() const { return ctx_; }
    FootContact& odometry() { return odometry_; }

    // the C ABI's per-step input: the body state, orientation and this estimator's odometry
    eslam_step_input makeInput(const BodyContactState& state, const Quaterniond& orientation, const Vector3d& translation,
                               size_t ltcCount) const
    {
        eslam_step_input in;
        std::memset(&in, 0, sizeof(in));
        in.body2odometry_rot[0] = orientation.w();
        in.body2odometry_rot[1] = orientation.x();
        in.body2odometry_rot[2] = orientation.y();
        in.body2odometry_rot[3] = orientation.z();
        for (int i = 0; i < 3; ++i) in.body2odometry_trans[i] = translation[i];
        const Pose& d = odometry_.getPoseDelta();
        for (int i = 0; i < 3; ++i) in.pose_delta_trans[i] = d.position[i];
        in.position_error_zz = odometry_.getPositionError()(2, 2);
        odometry_.getSampleDistribution2D(in.sample_mean, in.sample_cov);
        if (state.points.size() > ESLAM_MAX_CONTACTS) throw std::runtime_error("too many contact points");
        in.n_contacts = (uint32_t)state.points.size();
        last_m_ = in.n_contacts;
        in.ltc_count = (uint32_t)ltcCount;
        for (size_t i = 0; i < state.points.size(); ++i) {
            for (int k = 0; k < 3; ++k) in.contacts[i].position[k] = state.points[i].position[k];
            in.contacts[i].contact = state.points[i].contact;
            in.contacts[i].group_id = state.points[i].groupId;
        }
        return in;
    }

private:
    // the fields of a particle the device holds, as last downloaded or written back
    struct Hot {
        double v[7];                      // x, y, orientation, zPos, zSigma, weight, mprob
        uint8_t floating, ncp, pad[6];
    };
    static Hot hot(const Particle& p)
    {
        Hot h;
        std::memset(&h, 0, sizeof(h));
        h.v[0] = p.position.x(); h.v[1] = p.position.y(); h.v[2] = p.orientation; h.v[3] = p.zPos;
        h.v[4] = p.zSigma; h.v[5] = p.weight; h.v[6] = p.mprob;
        h.floating = p.floating ? 1 : 0;
        h.ncp = (uint8_t)(p.cpoints.size() & 0x7f);
        return h;
    }
    // a new particle set replaces the view without writing it back
    void discardView() const { view_valid_ = false; }

    FootContact& odometry_;
    Configuration config_;
    eslam_ctx* ctx_ = nullptr;
    eslam_update_info last_ = {};
    eslam_resample_info last_resample_ = {};
    eslam_kld_info last_kld_ = {};
    mutable std::vector<Particle> view_;           // getParticles()
    mutable std::vector<Hot> shadow_;              // view_ as the device holds it
    mutable bool view_valid_ = false;
    mutable uint32_t last_m_ = 0;
    bool sharded_ = false;
    int rank_ = 0;
    MlsGrid geometry_;                             // particleGrid(): scale, offset, global2local
    bool has_geometry_ = false;
};

// ---------------------------------------------------------------------------------------
// EmbodiedSlamFilter  src/EmbodiedSlamFilter.hpp:58-74 (the contact path)
// ---------------------------------------------------------------------------------------
class EmbodiedSlamFilter {
public:
    // src/EmbodiedSlamFilter.cpp:13-23 (device: the MI355X this filter runs on)
    EmbodiedSlamFilter(const OdometryConfiguration& odometryConfig, const Configuration& eslamConfig, int device = 0)
        : eslamConfig_(eslamConfig), odometry_(odometryConfig), device_(device)
    {
    }

    // init(env, pose, useSharedMap, hashConfig)  src/EmbodiedSlamFilter.cpp:70-128: the grid
    // is the environment's MLS grid; with hashConfig.useHash the particles are drawn from the
    // surface hash built on the device, else around the pose
    void init(const MlsGrid& env, const Pose& pose, bool useSharedMap = true,
              const SurfaceHashConfig& hashConfig = SurfaceHashConfig())
    {
        hashConfig_ = hashConfig;
        filter_.reset(new PoseEstimator(odometry_, eslamConfig_, device_, hashConfig));
        filter_->setEnvironment(env, useSharedMap);
        filter_->invalidate();
        sharedMap_ = useSharedMap;
        const double p[3] = {pose.position.x(), pose.position.y(), pose.position.z()};
        const double q[4] = {pose.orientation.w(), pose.orientation.x(), pose.orientation.y(), pose.orientation.z()};
        check(filter_->handle(), eslam_gpu_init_pose(filter_->handle(), p, q));
        update_idx_ = 0;
        resetMappingPoses();
    }

    // update(body2odometry, bs, ltc)  src/EmbodiedSlamFilter.cpp:353-369: odometry.update,
    // project, and the measurement update when UpdateThreshold::test passes (Q6) or ltc is
    // non-empty
    bool update(const Affine3d& body2odometry, const BodyContactState& bs, const std::vector<TerrainClassification>& ltc)
    {
        PoseEstimator& f = estimator();
        const Quaterniond orientation(body2odometry.linear());
        odometry_.update(bs, orientation);
        const eslam_step_input in = f.makeInput(bs, orientation, body2odometry.translation(), ltc.size());
        int updated = 0;
        f.flush();                        // edits made through getParticles()
        f.invalidate();
        check(f.handle(), eslam_gpu_step(f.handle(), &in, &updated));
        if (updated) ++update_idx_;
        last_state_ = bs;
        last_orientation_ = orientation;
        return updated != 0;
    }

    // update(body2odometry, scan, laser2body)  src/EmbodiedSlamFilter.cpp:311-351: when the laser
    // has moved past mappingThreshold since the last mapped scan (mapPose), the scan's MLS is
    // built on the device (PoseEstimator::scanFromLaser) and goes through
    // processMap(scan, useVisualUpdate, !sharedMap) -- with the shared map the laser only matches,
    // it does not merge
    bool update(const Affine3d& body2odometry, const LaserScan& scan, const Affine3d& laser2body)
    {
        if (!eslamConfig_.mappingThreshold.test(mapPose_.inverse() * body2odometry * laser2body)) return false;
        const Quaterniond orientation(body2odometry.linear());
        const std::vector<ScanPatch> scanMap = estimator().scanFromLaser(scan, laser2body, orientation, &lastScanInfo_);
        processMap(scanMap, eslamConfig_.useVisualUpdate, !sharedMap_);
        mapPose_ = body2odometry * laser2body;
        return true;
    }

    // update(body2odometry, dimage, camera2body)  src/EmbodiedSlamFilter.cpp:239-309: gated by
    // mappingCameraThreshold on stereoPose; the image's MLS always merges
    // (processMap(scan, false, true)), into the shared grid or into every particle's map.  The
    // texture image of the reference's signature is not taken.  On a sharded
    // estimator with the shared map the merge is a collective: every rank passes the same image.
    bool update(const Affine3d& body2odometry, const DistanceImage& dimage, const Affine3d& camera2body)
    {
        if (!eslamConfig_.mappingCameraThreshold.test(stereoPose_.inverse() * body2odometry * camera2body)) return false;
        const Quaterniond orientation(body2odometry.linear());
        const std::vector<ScanPatch> scanMap = estimator().scanFromDistanceImage(dimage, camera2body, orientation, &lastScanInfo_);
        processMap(scanMap, false, true);
        stereoPose_ = body2odometry * camera2body;
        return true;
    }
    // the counters of the last scan one of the two overloads above built
    const eslam_scan_info& lastScanInfo() const { return lastScanInfo_; }

    // processMap(scanMap, match, update)  src/EmbodiedSlamFilter.cpp:179-232 with the scan's
    // MLS as patches: match weights every particle against its map first -- the shared grid
    // (useSharedMap = true: the laser path's match-only call, :342-344) or its own map (the
    // build's match rule, eslam_gpu_map_match); update then merges the patches into every
    // particle's own map (useSharedMap = false; the reference's update-only call, :340-342) or,
    // with the shared map, into the one grid once per particle in particle order (the camera
    // path's processMap(scanMap, false, true), :301).  On a sharded estimator the shared map's
    // merge is a collective (PoseEstimator::updateSharedMap): every rank passes the same scan.
    void processMap(const std::vector<ScanPatch>& scanMap, bool match, bool update)
    {
        if (match) estimator().matchMaps(scanMap);
        if (update && !sharedMap_) estimator().updateMaps(scanMap);
        if (update && sharedMap_) estimator().updateSharedMap(scanMap);
    }

    // After a mapping run (useSharedMap = false), localise in the map particle i built, e.g. the
    // best one's (getBestParticleIndex()): PoseEstimator::adoptParticleMap.  The filter keeps
    // its map mode, so later scans merge into fresh per-particle maps on top of the adopted grid.
    void adoptParticleMap(size_t i) { estimator().adoptParticleMap(i); }

    // saveState / loadState: everything the filter needs to continue bit for bit -- this object's
    // own state (the map mode, the update count, the contact odometry between two updates), then
    // the device's snapshot through eslam_gpu_save_stream / eslam_gpu_load_stream (include/
    // eslam_gpu.h: particles, RNG, grid, pose hash, per-particle maps).  loadState works on a
    // filter that was only constructed (init() not called; hashConfig as init() would get it) and
    // replaces what an initialised one holds; the two configurations are this filter's own.
    // mapPose and stereoPose (the gates of the laser and camera updates) are not carried: after
    // loadState they read as after init, so the next scan and the next image map.
    // Failures are exceptions (std::runtime_error with the library's message).
    void saveState(std::ostream& os, uint64_t chunkBytes = 0)
    {
        PoseEstimator& f = estimator();
        f.flush();                        // edits made through getParticles()
        detail::put(os, kStateMagic);
        detail::put(os, (uint32_t)(sharedMap_ ? 1 : 0));
        detail::put(os, (uint32_t)0);
        detail::put(os, update_idx_);
        odometry_.saveState(os);
        detail::putState(os, last_state_);
        detail::putQ(os, last_orientation_);
        check(f.handle(), eslam_gpu_save_stream(f.handle(), &EmbodiedSlamFilter::writeStream, &os, chunkBytes, nullptr));
        if (!os) throw std::runtime_error("saveState: the stream failed");
    }
    void loadState(std::istream& is, uint64_t chunkBytes = 0) { loadState(is, hashConfig_, chunkBytes); }
    void loadState(std::istream& is, const SurfaceHashConfig& hashConfig, uint64_t chunkBytes = 0)
    {
        uint64_t magic = 0, idx = 0;
        uint32_t shared = 0, pad = 0;
        detail::get(is, magic);
        if (magic != kStateMagic) throw std::runtime_error("loadState: not a filter state");
        detail::get(is, shared);
        detail::get(is, pad);
        detail::get(is, idx);
        FootContact odo = odometry_;
        BodyContactState ls;
        Quaterniond lo;
        odo.loadState(is);
        detail::getState(is, ls);
        detail::getQ(is, lo);
        hashConfig_ = hashConfig;
        filter_.reset(new PoseEstimator(odometry_, eslamConfig_, device_, hashConfig));
        check(filter_->handle(), eslam_gpu_set_particle_maps(filter_->handle(), shared ? 0 : 1));
        check(filter_->handle(), eslam_gpu_load_stream(filter_->handle(), &EmbodiedSlamFilter::readStream, &is, chunkBytes, nullptr));
        filter_->invalidate();
        odometry_ = odo;
        sharedMap_ = shared != 0;
        update_idx_ = idx;
        last_state_ = ls;
        last_orientation_ = lo;
        resetMappingPoses();              // not in the state: the next scan and image map, as after init
    }

    // The same state as one file: this object's own part in a fixed prefix of kStatePrefix bytes
    // (zeros behind it), the device's snapshot behind the prefix, written and read by offset.
    // Works on a sharded filter too (collectives: every rank calls them with the same path):
    // rank 0 writes the prefix -- the odometry state is the same on every rank -- and every rank
    // its part of the blob; loadState then loads into the estimator as it is sharded, each rank
    // its slice, whatever layout wrote the file.  An unsharded filter may be only constructed.
    void saveState(const std::string& path, uint64_t chunkBytes = 0)
    {
        PoseEstimator& f = estimator();
        std::ostringstream head(std::ios::out | std::ios::binary);
        detail::put(head, kStateMagic);
        detail::put(head, (uint32_t)(sharedMap_ ? 1 : 0));
        detail::put(head, (uint32_t)0);
        detail::put(head, update_idx_);
        odometry_.saveState(head);
        detail::putState(head, last_state_);
        detail::putQ(head, last_orientation_);
        std::string prefix = head.str();
        if (prefix.size() > kStatePrefix) throw std::runtime_error("saveState: the filter's own state exceeds its prefix");
        prefix.resize(kStatePrefix, '\0');
        StateFile file(path, O_WRONLY | O_CREAT);
        if (!f.sharded() || f.rank() == 0)
            if (pwriteFile(&file, 0, prefix.data(), kStatePrefix) != 0) throw std::runtime_error("saveState: cannot write " + path);
        file.base = kStatePrefix;
        const eslam_snapshot_info info = f.saveAt(&EmbodiedSlamFilter::pwriteFile, &file, chunkBytes);
        // the file is the prefix and the blob (every rank may do this once all have written)
        if (::ftruncate(file.fd, (off_t)(kStatePrefix + info.bytes)) != 0) throw std::runtime_error("saveState: cannot size " + path);
    }
    void loadState(const std::string& path, uint64_t chunkBytes = 0) { loadState(path, hashConfig_, chunkBytes); }
    void loadState(const std::string& path, const SurfaceHashConfig& hashConfig, uint64_t chunkBytes = 0)
    {
        StateFile file(path, O_RDONLY);
        std::string prefix(kStatePrefix, '\0');
        if (preadFile(&file, 0, &prefix[0], kStatePrefix) != 0) throw std::runtime_error("loadState: cannot read " + path);
        const off_t size = ::lseek(file.fd, 0, SEEK_END);
        std::istringstream is(prefix, std::ios::in | std::ios::binary);
        uint64_t magic = 0, idx = 0;
        uint32_t shared = 0, pad = 0;
        detail::get(is, magic);
        if (magic != kStateMagic) throw std::runtime_error("loadState: not a filter state");
        detail::get(is, shared);
        detail::get(is, pad);
        detail::get(is, idx);
        FootContact odo = odometry_;
        BodyContactState ls;
        Quaterniond lo;
        odo.loadState(is);
        detail::getState(is, ls);
        detail::getQ(is, lo);
        if (!(filter_ && filter_->sharded())) {          // a sharded estimator keeps its communicator and layout
            hashConfig_ = hashConfig;
            filter_.reset(new PoseEstimator(odometry_, eslamConfig_, device_, hashConfig));
            check(filter_->handle(), eslam_gpu_set_particle_maps(filter_->handle(), shared ? 0 : 1));
        }
        file.base = kStatePrefix;
        filter_->loadAt(&EmbodiedSlamFilter::preadFile, &file, size > (off_t)kStatePrefix ? (uint64_t)size - kStatePrefix : 1, chunkBytes);
        odometry_ = odo;
        sharedMap_ = shared != 0;
        update_idx_ = idx;
        last_state_ = ls;
        last_orientation_ = lo;
        resetMappingPoses();
    }
    static constexpr uint64_t kStatePrefix = 4096;

    std::vector<PoseParticle>& getParticles() { return estimator().getParticles(); }
    size_t getBestParticleIndex() const { return estimator().getBestParticleIndex(); }
    Affine3d getCentroid() { return estimator().getCentroid().toTransform(); }

    // the particle distribution a Rock task logs every logParticlePeriod-th update
    // (src/Configuration.hpp:203-212; PoseDistribution src/PoseParticle.hpp:88-114): true when
    // the last update is one to log (period 0: never, 1: every update)
    bool logDue() const
    {
        const unsigned p = eslamConfig_.logParticlePeriod;
        return p != 0 && update_idx_ != 0 && (update_idx_ - 1) % p == 0;
    }
    // stride: every stride-th particle (a device-side subsample for large filters)
    PoseDistribution getPoseDistribution(size_t stride = 1)
    {
        PoseDistribution d;
        PoseEstimator& f = estimator();
        const size_t n = f.size();
        if (stride == 0) stride = 1;
        d.particles = f.getParticles(0, stride, n ? (n - 1) / stride + 1 : 0);
        d.orientation = last_orientation_;
        d.bodyState = last_state_;
        d.time = last_state_.time;
        return d;
    }
    // ... with d.gmm fitted on the device over all particles, whatever the stride
    PoseDistribution getPoseDistribution(size_t stride, const GmmParams& gp)
    {
        PoseDistribution d = getPoseDistribution(stride);
        d.gmm = estimator().fitGmm(gp);
        return d;
    }
    GaussianMixture2D fitGmm(const GmmParams& gp = GmmParams()) { return estimator().fitGmm(gp); }
    PoseMoments poseMoments(const PoseGate* gate = nullptr) const { return estimator().poseMoments(gate); }
    // KLD-sampling: the particle count the posterior asks for, and the resample to it
    eslam_kld_info kldCount(const KldParams& kp = KldParams()) { return estimator().kldCount(kp); }
    void resampleKld(const KldParams& kp = KldParams()) { estimator().resampleKld(kp); }
    // the trajectory log (PoseEstimator::enableTrajectory); bestTrajectory(): the path the best
    // particle's map was built along
    void enableTrajectory(uint32_t steps, uint64_t maxParticles = 0) { estimator().enableTrajectory(steps, maxParticles); }
    void disableTrajectory() { estimator().disableTrajectory(); }
    void clearTrajectory() { estimator().clearTrajectory(); }
    eslam_trajectory_info trajectoryInfo() { return estimator().trajectoryInfo(); }
    std::vector<eslam_trajectory_pose> trajectory(size_t i) { return estimator().trajectory(i); }
    std::vector<eslam_trajectory_pose> bestTrajectory() { return trajectory(getBestParticleIndex()); }
    std::vector<eslam_trajectory_estimate> smoothedTrajectory() { return estimator().smoothedTrajectory(); }

    PoseEstimator& estimator()
    {
        if (!filter_) throw std::runtime_error("EmbodiedSlamFilter: init() has not been called");
        return *filter_;
    }
    const PoseEstimator& estimator() const
    {
        if (!filter_) throw std::runtime_error("EmbodiedSlamFilter: init() has not been called");
        return *filter_;
    }
    FootContact& odometry() { return odometry_; }

private:
    struct Holder {                       // unique_ptr without <memory> in the public surface
        PoseEstimator* p = nullptr;
        ~Holder() { delete p; }
        void reset(PoseEstimator* q) { delete p; p = q; }
        explicit operator bool() const { return p != nullptr; }
        PoseEstimator& operator*() const { return *p; }
        PoseEstimator* operator->() const { return p; }
    };
    static constexpr uint64_t kStateMagic = 0x3154534641465345ull;   // "ESFAFST1"
    static int writeStream(void* user, const void* data, uint64_t bytes)
    {
        std::ostream& os = *static_cast<std::ostream*>(user);
        os.write(static_cast<const char*>(data), (std::streamsize)bytes);
        return os ? 0 : 1;
    }
    // a state file: its descriptor, and where the device's blob starts in it
    struct StateFile {
        int fd;
        uint64_t base = 0;
        StateFile(const std::string& path, int flags) : fd(::open(path.c_str(), flags, 0644))
        {
            if (fd < 0) throw std::runtime_error("cannot open " + path);
        }
        ~StateFile() { ::close(fd); }
        StateFile(const StateFile&) = delete;
        StateFile& operator=(const StateFile&) = delete;
    };
    static int pwriteFile(void* user, uint64_t offset, const void* data, uint64_t bytes)
    {
        const StateFile& f = *static_cast<const StateFile*>(user);
        const char* p = static_cast<const char*>(data);
        while (bytes) {
            const ssize_t w = ::pwrite(f.fd, p, bytes, (off_t)(f.base + offset));
            if (w <= 0) return 1;
            p += w;
            offset += (uint64_t)w;
            bytes -= (uint64_t)w;
        }
        return 0;
    }
    static int preadFile(void* user, uint64_t offset, void* data, uint64_t bytes)
    {
        const StateFile& f = *static_cast<const StateFile*>(user);
        char* p = static_cast<char*>(data);
        while (bytes) {
            const ssize_t r = ::pread(f.fd, p, bytes, (off_t)(f.base + offset));
            if (r <= 0) return 1;
            p += r;
            offset += (uint64_t)r;
            bytes -= (uint64_t)r;
        }
        return 0;
    }
    static int readStream(void* user, void* data, uint64_t bytes)
    {
        std::istream& is = *static_cast<std::istream*>(user);
        is.read(static_cast<char*>(data), (std::streamsize)bytes);
        return is ? 0 : 1;
    }
    // udPose = mapPose = stereoPose = Translation(1000, 0, 0)  src/EmbodiedSlamFilter.cpp:128 (udPose
    // lives in the library): the first scan and the first image always map
    void resetMappingPoses()
    {
        mapPose_ = stereoPose_ = Affine3d::Identity();
        mapPose_.translation() = stereoPose_.translation() = Vector3d(1000, 0, 0);
        std::memset(&lastScanInfo_, 0, sizeof(lastScanInfo_));
    }
    Configuration eslamConfig_;
    SurfaceHashConfig hashConfig_;
    Affine3d mapPose_, stereoPose_;
    eslam_scan_info lastScanInfo_ = {};
    FootContact odometry_;
    int device_;
    Holder filter_;
    bool sharedMap_ = true;
    uint64_t update_idx_ = 0;
    BodyContactState last_state_;
    Quaterniond last_orientation_;
};

}  // namespace gpu
}  // namespace eslam

#endif
