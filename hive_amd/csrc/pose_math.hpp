// Float64 vector and unit-quaternion arithmetic shared by the pose optimisers (fts.hip, poseopt.hip).  Every expression states its operation order: the
// translation units that include this are built without contraction, and their results are functions of that order.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HIVE_HD __host__ __device__ __forceinline__
#else
#define HIVE_HD inline
#endif

namespace hive_pose {

struct Vec3 {
    double x, y, z;
};
HIVE_HD Vec3 operator+(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
HIVE_HD Vec3 operator-(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
HIVE_HD Vec3 operator*(double s, Vec3 a) { return {s * a.x, s * a.y, s * a.z}; }
HIVE_HD double dot(Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
HIVE_HD Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
HIVE_HD Vec3 load3(const double *p) { return {p[0], p[1], p[2]}; }
HIVE_HD void store3(double *p, Vec3 a) {
    p[0] = a.x;
    p[1] = a.y;
    p[2] = a.z;
}

struct Pose {
    Vec3 a;      // vector part of the unit quaternion
    double s;    // its scalar part
    double norm; // |q|
    Vec3 t;
};

// p = (scalar-last quaternion, translation, ..)
HIVE_HD Pose load_pose(const double *p) {
    Pose o;
    const double n = sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3]);
    o.a = {p[0] / n, p[1] / n, p[2] / n};
    o.s = p[3] / n;
    o.norm = n;
    o.t = load3(p + 4);
    return o;
}

// conj(u) (v, 0) u
HIVE_HD Vec3 rotate_inverse(const Pose &u, Vec3 v) {
    return ((u.s * u.s - dot(u.a, u.a)) * v + (2.0 * dot(u.a, v)) * u.a) - (2.0 * u.s) * cross(u.a, v);
}

// u (g, 0) conj(u)
HIVE_HD Vec3 rotate_forward(const Pose &u, Vec3 g) {
    return ((u.s * u.s - dot(u.a, u.a)) * g + (2.0 * dot(u.a, g)) * u.a) + (2.0 * u.s) * cross(u.a, g);
}

}  // namespace hive_pose
