// The arithmetic of hive_pose_optimise (poseopt.hip), as host/device functions: one correspondence's residual and hand-derived gradient, a frame's
// regularisers, the Adam update, the scheduler / early-stopping state machine.  The rule is stated above hive_pose_optimise in include/hive_mi355x.h; this
// file is its only statement in code (the kernels add the summation order).
#pragma once
#include "pose_math.hpp"

namespace hive_pose {

constexpr int PO_STRIDE = 9;  // doubles per frame: quaternion (scalar last), translation, scale, shift
constexpr int PO_ACC = 10;    // a frame's sums: d/dq (4), d/dt (3), d/dscale, d/dshift, its share of the loss

struct PoConst {
    int n;          // frames
    long long m;    // correspondences
    int smooth, position_only;
    double fx, fy, cx, cy;
    double pose_t_reg, pose_r_reg, l2;
    double beta1, beta2, eps;
};

// what launch 1 leaves for launch 2 and for the host
struct PoState {
    double lr;           // the learning rate the next step uses
    double b1k, b2k;     // beta^k of the next step
    double sched_best;   // ReduceLROnPlateau
    double stop_best;    // EarlyStopping
    double final_loss;   // the evaluation launch's loss
    int sched_bad, stop_calls;
    int stop;            // 1: every later launch is a no-op
    int epochs_run;
    int nonfinite_epoch; // first epoch whose loss was not finite, -1 = none
    int bad_depth;       // set by the widening pass
};

struct PoSchedule {
    double threshold;  // min_loss_delta
    int lr_patience, stop_patience;
};

// ReduceLROnPlateau(mode='min', threshold_mode='abs', factor=0.1, cooldown=0, min_lr=0, eps=1e-8).step(loss), then EarlyStopping.step(loss)
HIVE_HD void po_schedule(PoState &s, const PoSchedule &o, double loss) {
    if (loss < s.sched_best - o.threshold) {
        s.sched_best = loss;
        s.sched_bad = 0;
    } else {
        s.sched_bad += 1;
    }
    if (s.sched_bad > o.lr_patience) {
        const double lower = s.lr * 0.1;
        if (s.lr - lower > 1e-8) s.lr = lower;
        s.sched_bad = 0;
    }
    if (loss < s.stop_best && fabs(loss - s.stop_best) > o.threshold) {
        s.stop_best = loss;
        s.stop_calls = 0;
    } else {
        s.stop_calls += 1;
    }
    if (s.stop_calls > o.stop_patience) s.stop = 1;
}

HIVE_HD Vec3 po_unproject(const PoConst &k, double u, double v, double d) { return {((u - k.cx) * d) / k.fx, ((v - k.cy) * d) / k.fy, d}; }

// d/d(a, s) of g . (conj(u) (v, 0) u) for the unit quaternion u = (a, s)
HIVE_HD void po_quat_grad(Vec3 a, double s, Vec3 v, Vec3 g, Vec3 &ga, double &gs) {
    gs = dot(g, (2.0 * s) * v - 2.0 * cross(a, v));
    ga = (((-2.0 * dot(g, v)) * a + (2.0 * dot(a, v)) * g) + (2.0 * dot(g, a)) * v) - (2.0 * s) * cross(v, g);
}

// d/dq of the raw quaternion from d/du of the unit one: (d/du - u (u . d/du)) / |q|, added to acc[0..3]
HIVE_HD void po_add_raw_quat(const Pose &u, Vec3 ga, double gs, double *acc) {
    const double radial = dot(u.a, ga) + u.s * gs;
    acc[0] += (ga.x - u.a.x * radial) / u.norm;
    acc[1] += (ga.y - u.a.y * radial) / u.norm;
    acc[2] += (ga.z - u.a.z * radial) / u.norm;
    acc[3] += (gs - u.s * radial) / u.norm;
}

// One side of the residual: w = conj(u) (c - t) u with c the camera-space point of (pu, pv, depth) -- Affine: depth' = 1 / (scale (1 / depth) + shift).
struct PoSide {
    Pose u;
    Vec3 c, v, w;
    double rx, ry, dp, inv_d;  // Affine: the ray ((pu - cx) / fx, (pv - cy) / fy), depth', 1 / depth
};

template <bool AFFINE>
HIVE_HD void po_side(const PoConst &k, const double *par, int f, const double *raw, const double *cam, PoSide &o) {
    const double *p = par + (size_t)f * PO_STRIDE;
    o.u = load_pose(p);
    if (AFFINE) {
        o.inv_d = 1.0 / raw[2];
        o.dp = 1.0 / (p[7] * o.inv_d + p[8]);
        o.c = po_unproject(k, raw[0], raw[1], o.dp);
        o.rx = (raw[0] - k.cx) / k.fx;
        o.ry = (raw[1] - k.cy) / k.fy;
    } else {
        o.c = load3(cam);
    }
    o.v = o.c - o.u.t;
    o.w = rotate_inverse(o.u, o.v);
}

// back through w = conj(u) (c - t) u of this frame: g = dL/dw, added to acc
template <bool AFFINE>
HIVE_HD void po_back_side(const PoSide &o, Vec3 g, double *acc) {
    const Vec3 gc = rotate_forward(o.u, g);  // dL/dc = -dL/dt
    Vec3 ga;
    double gs;
    po_quat_grad(o.u.a, o.u.s, o.v, g, ga, gs);
    po_add_raw_quat(o.u, ga, gs, acc);
    acc[4] -= gc.x;
    acc[5] -= gc.y;
    acc[6] -= gc.z;
    if (AFFINE) {
        const double gd = (gc.x * o.rx + gc.y * o.ry) + gc.z;  // dL/ddepth'
        const double dd = -(o.dp * o.dp);                       // ddepth'/dshift
        acc[7] += gd * (dd * o.inv_d);
        acc[8] += gd * dd;
    }
}

// Correspondence k seen from its frame on `side` (0 = index_i, 1 = index_j): that frame's share of the gradient and, on side 0, the residual's norm.
// raw [m][6] = (u_i, v_i, depth_i, u_j, v_j, depth_j) widened; cam [m][6] = the two camera-space points (Rigid only).
template <bool IMAGE2D, bool AFFINE>
HIVE_HD void po_entry(const PoConst &k, const double *par, const double *raw, const double *cam, const int *index_i, const int *index_j, long long e, int side,
                      double *acc) {
    const double *rw = raw + (size_t)e * 6, *cm = AFFINE ? nullptr : cam + (size_t)e * 6;
    const int fi = index_i[e], fj = index_j[e];
    const double inv_m = 1.0 / (double)k.m;
    PoSide I;
    po_side<AFFINE>(k, par, fi, rw, cm, I);
    if (!IMAGE2D) {
        PoSide J;
        po_side<AFFINE>(k, par, fj, rw + 3, AFFINE ? nullptr : cm + 3, J);
        const Vec3 r = I.w - J.w;
        const double rn = sqrt(dot(r, r));
        if (side == 0) acc[9] += rn;
        if (!(rn > 0.0)) return;
        const Vec3 g = (inv_m / rn) * r;  // dL/dp; dL/dq = -g
        if (side == 0)
            po_back_side<AFFINE>(I, g, acc);
        else
            po_back_side<AFFINE>(J, -1.0 * g, acc);
    } else {
        const Pose uj = load_pose(par + (size_t)fj * PO_STRIDE);
        const Vec3 x = rotate_forward(uj, I.w) + uj.t;
        const double z = x.z;
        const double ru = rw[3] - (k.fx * x.x + k.cx * z) / z, rv = rw[4] - (k.fy * x.y + k.cy * z) / z;
        const double rn = sqrt(ru * ru + rv * rv);
        if (side == 0) acc[9] += rn;
        if (!(rn > 0.0)) return;
        const double gu = -((inv_m / rn) * ru), gv = -((inv_m / rn) * rv);  // dL/d(projection)
        const Vec3 gx = {(gu * k.fx) / z, (gv * k.fy) / z, -(((gu * k.fx) * x.x + (gv * k.fy) * x.y) / (z * z))};
        if (side == 0) {
            po_back_side<AFFINE>(I, rotate_inverse(uj, gx), acc);
        } else {  // u p conj(u) is conj(u') p u' with u' = conj(u): the same derivative, the vector part negated
            Vec3 ga;
            double gs;
            po_quat_grad(-1.0 * uj.a, uj.s, I.w, gx, ga, gs);
            po_add_raw_quat(uj, -1.0 * ga, gs, acc);
            acc[4] += gx.x;
            acc[5] += gx.y;
            acc[6] += gx.z;
        }
    }
}

HIVE_HD Vec3 po_t(const double *par, int f) { return load3(par + (size_t)f * PO_STRIDE + 4); }
HIVE_HD Vec3 po_d1(const double *par, int a) { return po_t(par, a) - po_t(par, a + 1); }
HIVE_HD Vec3 po_d2(const double *par, int a) { return (po_t(par, a) - 2.0 * po_t(par, a + 1)) + po_t(par, a + 2); }
HIVE_HD Vec3 po_d3(const double *par, int a) { return po_d2(par, a) - po_d2(par, a + 1); }
HIVE_HD double po_qdot(const double *par, int a) {
    const double *p = par + (size_t)a * PO_STRIDE, *q = p + PO_STRIDE;
    return ((p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]) + p[3] * q[3];
}

// acc holds frame f's sums over its incidence list.  Turns acc[9] into the frame's share of the loss, adds the regularisers (a difference belongs to its
// FIRST frame; a mean over no rows -- n < 4 -- is 0) and zeroes what is pinned.
template <bool AFFINE>
HIVE_HD void po_frame_tail(const PoConst &k, const double *par, int f, double *acc) {
    const int n = k.n;
    double loss = acc[9] / (double)k.m;
    if (k.smooth) {
        Vec3 gt = {0.0, 0.0, 0.0};
        if (n >= 2) {
            const double w = k.pose_t_reg / (double)(n - 1);
            Vec3 s = {0.0, 0.0, 0.0};
            if (f <= n - 2) {
                const Vec3 d = po_d1(par, f);
                loss += w * dot(d, d);
                s = s + d;
            }
            if (f >= 1) s = s - po_d1(par, f - 1);
            gt = gt + (2.0 * w) * s;
        }
        if (n >= 3) {
            const double w = k.pose_t_reg / (double)(n - 2);
            Vec3 s = {0.0, 0.0, 0.0};
            if (f <= n - 3) {
                const Vec3 d = po_d2(par, f);
                loss += w * dot(d, d);
                s = s + d;
            }
            if (f >= 1 && f <= n - 2) s = s - 2.0 * po_d2(par, f - 1);
            if (f >= 2) s = s + po_d2(par, f - 2);
            gt = gt + (2.0 * w) * s;
        }
        if (n >= 4) {
            const double w = k.pose_t_reg / (double)(n - 3);
            Vec3 s = {0.0, 0.0, 0.0};
            if (f <= n - 4) {
                const Vec3 d = po_d3(par, f);
                loss += w * dot(d, d);
                s = s + d;
            }
            if (f >= 1 && f <= n - 3) s = s - 3.0 * po_d3(par, f - 1);
            if (f >= 2 && f <= n - 2) s = s + 3.0 * po_d3(par, f - 2);
            if (f >= 3) s = s - po_d3(par, f - 3);
            gt = gt + (2.0 * w) * s;
        }
        acc[4] += gt.x;
        acc[5] += gt.y;
        acc[6] += gt.z;
        if (n >= 2) {  // 1 - (r_a . r_{a + 1})^2 on the raw quaternions
            const double w = k.pose_r_reg / (double)(n - 1);
            const double *q = par + (size_t)f * PO_STRIDE;
            if (f <= n - 2) {
                const double c = po_qdot(par, f);
                loss += w * (1.0 - c * c);
                for (int j = 0; j < 4; ++j) acc[j] -= ((2.0 * w) * c) * q[PO_STRIDE + j];
            }
            if (f >= 1) {
                const double c = po_qdot(par, f - 1);
                for (int j = 0; j < 4; ++j) acc[j] -= ((2.0 * w) * c) * q[j - PO_STRIDE];
            }
        }
    }
    if (AFFINE) {
        const double *p = par + (size_t)f * PO_STRIDE;
        const double w = k.l2 / (double)n, e = 1.0 / p[7] - 1.0;
        loss += w * (e * e) + (2.0 * w) * (p[8] * p[8]);
        acc[7] += ((2.0 * w) * e) * (-1.0 / (p[7] * p[7]));
        acc[8] += (4.0 * w) * p[8];
    }
    acc[9] = loss;
    if (f == 0 || k.position_only)
        for (int j = 0; j < 4; ++j) acc[j] = 0.0;
    if (f == 0)
        for (int j = 4; j < 7; ++j) acc[j] = 0.0;
}

// torch.optim.Adam on the `count` leading parameters of a frame: mom [2][PO_STRIDE] first and second moments, b1k / b2k = beta^step
HIVE_HD void po_adam(const PoConst &k, const double *p, const double *g, double *mom, double lr, double b1k, double b2k, int count, double *out) {
    const double step = lr / (1.0 - b1k), root2 = sqrt(1.0 - b2k);
    for (int j = 0; j < PO_STRIDE; ++j) {
        if (j >= count) {
            out[j] = p[j];
            continue;
        }
        const double m1 = mom[j] + (1.0 - k.beta1) * (g[j] - mom[j]);
        const double m2 = k.beta2 * mom[PO_STRIDE + j] + (1.0 - k.beta2) * (g[j] * g[j]);
        mom[j] = m1;
        mom[PO_STRIDE + j] = m2;
        out[j] = p[j] - step * (m1 / (sqrt(m2) / root2 + k.eps));
    }
}

}  // namespace hive_pose
