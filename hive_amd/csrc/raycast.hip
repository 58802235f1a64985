// Ray casts the TSDF volume from a camera pose: depth, surface point, normal and colour per pixel, straight from the planes (no marching cubes).  What a
// KinectFusion-style tracker aligns the live frame against (track.hip), and a preview of the volume on its own.  gfx950 only.
// The rules are stated in include/hive_mi355x.h above hive_tsdf_raycast; in short (float32, every operation rounded once, no fused multiply-add):
//
//   ray        d = ((u - cx) / fx, (v - cy) / fy, 1); w_r = (R[r][0] d_0 + R[r][1] d_1) + R[r][2]; the parameter is camera z
//   voxel      p_r(z) = ((z w_r + t_r) - origin_r) / voxel_size
//   range      slab test against the box of voxel centres [0, dim - 1]^3 in voxel coordinates, cut to [z_near, z_far]; k = 0 .. floor((z_out - z_in) / step)
//   sample     trilinear in the order z, y, x as a + f (b - a); valid iff the eight corners are inside the grid and have weight > 0
//   march      z_k = z_in + k step; (+, <= 0) is the hit at z_prev + (step S_prev) / (S_prev - S_k); (<0, >0) ends the ray; invalid samples never pair
//   normal     central differences of the sample one voxel either side of the hit along each grid axis, normalised
//   colour     the packed colour of voxel floor(p + 0.5), clamped to the grid
//
// One lane per ray; a wave covers an 8 x 8 pixel tile (neighbouring rays touch neighbouring voxels), a workgroup 16 x 16 pixels.  A sample gathers 16 floats:
// eight corners of the weight plane and of the tsdf plane, 64 bytes.
#include "hive_internal.hpp"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_TILE = 16;          // pixels per workgroup side: 2 x 2 waves of 8 x 8
constexpr int RC_MAX_STEPS = 1 << 20;

struct RaycastParams {
    const float *tsdf, *weight, *color;
    int X, Y, Z;
    float ox, oy, oz, vs;
    float R[9], t[3];
    float fx, fy, cx, cy;
    float z_near, z_far, step;
    int H, W;
};

// S at voxel coordinate (px, py, pz); false: a corner is outside the grid or was never observed
__device__ __forceinline__ bool rc_sample(const RaycastParams &p, float px, float py, float pz, float &S) {
    if (!(px >= 0.f && py >= 0.f && pz >= 0.f && px < (float)(p.X - 1) && py < (float)(p.Y - 1) && pz < (float)(p.Z - 1))) return false;  // (NaN: false)
    const float bx = floorf(px), by = floorf(py), bz = floorf(pz);
    const float fx = px - bx, fy = py - by, fz = pz - bz;
    const size_t sy = (size_t)p.Z, sx = (size_t)p.Y * p.Z;
    const size_t at = (size_t)(int)bx * sx + (size_t)(int)by * sy + (size_t)(int)bz;
    const float *w = p.weight + at;
    if (!(w[0] > 0.f && w[1] > 0.f && w[sy] > 0.f && w[sy + 1] > 0.f && w[sx] > 0.f && w[sx + 1] > 0.f && w[sx + sy] > 0.f && w[sx + sy + 1] > 0.f)) return false;
    const float *t = p.tsdf + at;
    const float c00 = t[0] + fz * (t[1] - t[0]);
    const float c01 = t[sy] + fz * (t[sy + 1] - t[sy]);
    const float c10 = t[sx] + fz * (t[sx + 1] - t[sx]);
    const float c11 = t[sx + sy] + fz * (t[sx + sy + 1] - t[sx + sy]);
    const float c0 = c00 + fy * (c01 - c00);
    const float c1 = c10 + fy * (c11 - c10);
    S = c0 + fx * (c1 - c0);
    return true;
}

__device__ __forceinline__ float rc_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float rc_max(float a, float b) { return a > b ? a : b; }

// one axis of the slab test in voxel coordinates; false: the ray never enters
__device__ __forceinline__ bool rc_slab(float g0, float gd, float hi, float &z_in, float &z_out) {
    if (gd != 0.f) {
        const float a = (0.f - g0) / gd, b = (hi - g0) / gd;
        z_in = rc_max(z_in, rc_min(a, b));
        z_out = rc_min(z_out, rc_max(a, b));
        return true;
    }
    return g0 >= 0.f && g0 <= hi;  // parallel to the slab: inside or never
}

__global__ __launch_bounds__(RC_THREADS) void tsdf_raycast_kernel(RaycastParams p, float *__restrict__ depth, float *__restrict__ vertex, float *__restrict__ normal,
                                                                  uint8_t *__restrict__ color) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int v = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3), u = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
    if (v >= p.H || u >= p.W) return;
    const float d0 = ((float)u - p.cx) / p.fx, d1 = ((float)v - p.cy) / p.fy;
    float w[3], g0[3], gd[3];
    const float o[3] = {p.ox, p.oy, p.oz};
    const int dim[3] = {p.X, p.Y, p.Z};
    float z_in = p.z_near, z_out = p.z_far > 0.f ? p.z_far : __builtin_inff();
    bool live = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        w[r] = (p.R[3 * r + 0] * d0 + p.R[3 * r + 1] * d1) + p.R[3 * r + 2];
        g0[r] = (p.t[r] - o[r]) / p.vs;
        gd[r] = w[r] / p.vs;
        live = rc_slab(g0[r], gd[r], (float)(dim[r] - 1), z_in, z_out) && live;
    }
    live = live && z_in <= z_out;
    float z_hit = 0.f;
    bool hit = false;
    if (live) {
        const float span = floorf((z_out - z_in) / p.step);
        const int last = span < (float)RC_MAX_STEPS ? (int)span : RC_MAX_STEPS;
        bool prev_ok = false;
        float S_prev = 0.f, z_prev = 0.f;
        for (int k = 0; k <= last; ++k) {
            const float z = z_in + (float)k * p.step;
            float S = 0.f;
            const bool ok = rc_sample(p, ((z * w[0] + p.t[0]) - o[0]) / p.vs, ((z * w[1] + p.t[1]) - o[1]) / p.vs, ((z * w[2] + p.t[2]) - o[2]) / p.vs, S);
            if (ok && prev_ok) {
                if (S_prev > 0.f && S <= 0.f) {
                    z_hit = z_prev + (p.step * S_prev) / (S_prev - S);
                    hit = true;
                    break;
                }
                if (S_prev < 0.f && S > 0.f) break;  // leaving a surface from behind
            }
            prev_ok = ok, S_prev = S, z_prev = z;
        }
    }
    const size_t px = (size_t)v * p.W + u;
    float P[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    unsigned rgb = 0;
    if (hit) {
        float q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) P[r] = z_hit * w[r] + p.t[r], q[r] = (P[r] - o[r]) / p.vs;
        if (normal) {
            float a[3], b[3];
            bool ok = rc_sample(p, q[0] + 1.f, q[1], q[2], a[0]) && rc_sample(p, q[0] - 1.f, q[1], q[2], b[0]);
            ok = ok && rc_sample(p, q[0], q[1] + 1.f, q[2], a[1]) && rc_sample(p, q[0], q[1] - 1.f, q[2], b[1]);
            ok = ok && rc_sample(p, q[0], q[1], q[2] + 1.f, a[2]) && rc_sample(p, q[0], q[1], q[2] - 1.f, b[2]);
            if (ok) {
                const float gx = a[0] - b[0], gy = a[1] - b[1], gz = a[2] - b[2];
                const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                if (len > 0.f) n[0] = gx / len, n[1] = gy / len, n[2] = gz / len;
            }
        }
        if (color) {
            int c[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float f = floorf(q[r] + 0.5f);
                c[r] = f < 0.f ? 0 : (f > (float)(dim[r] - 1) ? dim[r] - 1 : (int)f);
            }
            rgb = (unsigned)p.color[((size_t)c[0] * p.Y + c[1]) * p.Z + c[2]];
        }
    }
    if (depth) depth[px] = z_hit;
    if (vertex) vertex[3 * px + 0] = P[0], vertex[3 * px + 1] = P[1], vertex[3 * px + 2] = P[2];
    if (normal) normal[3 * px + 0] = n[0], normal[3 * px + 1] = n[1], normal[3 * px + 2] = n[2];
    if (color) color[3 * px + 0] = (uint8_t)(rgb & 255u), color[3 * px + 1] = (uint8_t)((rgb >> 8) & 255u), color[3 * px + 2] = (uint8_t)((rgb >> 16) & 255u);
}

}  // namespace

extern "C" {

int hive_tsdf_raycast(hive_tsdf *vol, int H, int W, const float K[9], const double cam_pose[16], float z_near, float z_far, float step_in_trunc, float *d_depth,
                      float *d_vertex, float *d_normal, uint8_t *d_color) {
    HIVE_ENTER(vol ? vol->ctx : nullptr);
    if (!vol) return hive_fail(nullptr, HIVE_ERR_INVALID, "vol is NULL");
    hive_ctx *ctx = vol->ctx;
    HIVE_REQUIRE(ctx, vol->x_off == 0 && vol->dim[0] == vol->grid_dim0, "raycast: this volume is an x-slab [%lld, %lld) of a %lld-wide grid; gather the slabs into a "
                 "whole volume first", (long long)vol->x_off, (long long)(vol->x_off + vol->dim[0]), (long long)vol->grid_dim0);
    HIVE_REQUIRE(ctx, K && cam_pose, "raycast: NULL camera");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "raycast: bad image size %d x %d", H, W);
    HIVE_REQUIRE(ctx, K[0] != 0.f && K[4] != 0.f, "raycast: fx and fy must not be 0");
    HIVE_REQUIRE(ctx, z_near >= 0.f, "raycast: z_near must be >= 0");
    HIVE_REQUIRE(ctx, step_in_trunc > 0.f, "raycast: step_in_trunc must be > 0");
    HIVE_REQUIRE(ctx, vol->dim[0] < (1ll << 24) && vol->dim[1] < (1ll << 24) && vol->dim[2] < (1ll << 24), "raycast: a volume side of 2^24 voxels or more");
    RaycastParams p;
    p.tsdf = vol->d_tsdf, p.weight = vol->d_weight, p.color = vol->d_color;
    p.X = (int)vol->dim[0], p.Y = (int)vol->dim[1], p.Z = (int)vol->dim[2];
    p.ox = vol->origin[0], p.oy = vol->origin[1], p.oz = vol->origin[2], p.vs = vol->voxel_size;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[3 * r + c] = (float)cam_pose[4 * r + c];
        p.t[r] = (float)cam_pose[4 * r + 3];
    }
    p.fx = K[0], p.fy = K[4], p.cx = K[2], p.cy = K[5];
    p.z_near = z_near, p.z_far = z_far, p.step = step_in_trunc * vol->trunc;
    p.H = H, p.W = W;
    const dim3 grid((unsigned)((W + RC_TILE - 1) / RC_TILE), (unsigned)((H + RC_TILE - 1) / RC_TILE));
    HIVE_REQUIRE(ctx, grid.y <= 65535, "raycast: H = %d has too many tile rows", H);
    hipLaunchKernelGGL(tsdf_raycast_kernel, grid, dim3(RC_THREADS), 0, ctx->stream, p, d_depth, d_vertex, d_normal, d_color);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
