// Camera pose optimisation (PoseOptimiser._optimisation_loop, hive/pose_optimisation.py:1256-1519) as PROJECTED Adam.  gfx950 only.
//
//   hive_pose_optimise -> the Adam loop over poses (and, Affine, a depth scale and shift per frame) against the correspondences of a FeatureSet
//   hive_pose_project  -> one epoch's projection alone: quaternions normalised, positions clipped
//
// Deliberate deviation, not pinned against the reference's run: the reference assigns NEW Parameter objects for the normalised quaternions (and the clipped
// positions) every epoch while its optimiser keeps the old ones, whose .grad stays None, so step() moves nothing.  Here the normalisation and the clip are
// projections of the LIVE parameters, in place, and Adam steps those same parameters with its moments and step count carried through.
//
// Float64 throughout (the reference keeps float32 parameters), compiled without contraction, every sum in an order that depends on the problem alone: results are
// bit-identical from run to run and do not depend on check_every.  The rule -- loss, clip, scheduler -- stands above hive_pose_optimise in
// include/hive_mi355x.h; its arithmetic is poseopt_core.hpp.  Gradients, by hand, with u = q / |q| = (a, s), v = c - t, w = conj(u) (v, 0) u and g = dL/dw:
//   dL/dc = u (g, 0) conj(u) = -dL/dt,   dL/ds = g . (2 s v - 2 (a x v)),   dL/da = -2 (g.v) a + 2 (a.v) g + 2 (g.a) v - 2 s (v x g),
//   dL/dq = (dL/du - u (u . dL/du)) / |q|;   Affine: c = depth' ray, dL/ddepth' = dL/dc . ray, ddepth'/dshift = -depth'^2, ddepth'/dscale = -depth'^2 / depth.
//   World3D: r = p - q, g_p = r / (M |r|) = -g_q.   Image2D: x = u_j (p, 0) conj(u_j) + t_j, r = pixel_j - pi(x), G = dL/dpi = -r / (M |r|),
//   dL/dx = (G_u f_x / z, G_v f_y / z, -(G_u f_x x + G_v f_y y) / z^2) = dL/dt_j, g_p = conj(u_j) (dL/dx, 0) u_j, and dL/du_j is the formula above at conj(u_j).
//   A residual of norm 0 contributes 0 (torch.norm's subgradient).
//
// Launches.  Per epoch two bounded launches; none waits for another workgroup:
//   prepare (ONE workgroup of 256): sums the previous epoch's per-frame loss shares (thread k takes frames k, k + 256, .. in order, lane butterfly xor 32 .. 1,
//     the four waves in order), runs the scheduler and early-stopping state machine on that loss, then projects the parameters in place: q / |q| per frame;
//     the clip of the positions (differences in parallel, the running sum from the first clipped step on by ONE thread, frame after frame).
//   step (one workgroup of 256 per frame): walks the frame's incidence list -- (correspondence k, side) ascending, built on the host by a counting sort --
//     thread j taking entries j, j + 256, .. in order; every entry recomputes its residual from the epoch's read-only parameter buffer; lane butterfly, waves
//     in order; thread 0 adds the regularisers, zeroes the pinned components, does the Adam update into the OTHER parameter buffer and writes the frame's share
//     of the loss (the residual norms of its side-0 entries / M, the regulariser terms whose first frame it is).
// Once the device-side stop flag is set (early stop, or a non-finite loss), every later launch returns at once; the host enqueues check_every epochs at a time
// and reads the state once per batch.
#include "hive_internal.hpp"
#include "poseopt_core.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>

namespace {

using namespace hive_pose;

constexpr int PO_THREADS = 256;
constexpr int PO_WAVES = PO_THREADS / 64;

struct PoArgs {
    PoConst k;
    PoSchedule sched;
    PoState *state;
    double *par[2];        // [n][PO_STRIDE] each: an epoch reads par[epoch & 1] and writes the other
    double *mom;           // [n][2][PO_STRIDE]
    double *partial;       // [n] loss shares
    double *losses, *rates;  // [epochs]
    double *grad;          // [n][PO_STRIDE] (evaluation)
    double *clip;          // [n][3] clipped differences
    const double *raw, *cam;  // [m][6]
    const int *index_i, *index_j;  // [m]
    const int *offsets;    // [n + 1]
    const int *entries;    // [2 m]: 2 k + side
    double max_distance;   // < 0: no clip
};

__device__ __forceinline__ double po_loss_sum(const double *partial, int n, double (*lds)[PO_ACC]) {
    double s[1] = {0.0};
    for (int f = threadIdx.x; f < n; f += PO_THREADS) s[0] += partial[f];
    block_butterfly_sum<1>(s, lds);
    return s[0];
}

// the projection of one epoch, in place on par: every thread of the one workgroup
__device__ __forceinline__ void po_project(double *par, int n, double max_distance, double *clip, double (*stage)[3], int *first_shared) {
    for (int f = threadIdx.x; f < n; f += PO_THREADS) {
        double *q = par + (size_t)f * PO_STRIDE;
        const double norm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        for (int j = 0; j < 4; ++j) q[j] = q[j] / norm;
    }
    if (max_distance < 0.0) return;
    if (threadIdx.x == 0) *first_shared = n;
    __syncthreads();
    int first = n;
    for (int f = threadIdx.x + 1; f < n; f += PO_THREADS) {
        Vec3 d = po_t(par, f) - po_t(par, f - 1);
        const double dist = sqrt(dot(d, d));
        if (dist > max_distance) {
            d = (max_distance / dist) * d;
            first = min(first, f);
        }
        store3(clip + (size_t)f * 3, d);
    }
    if (first < n) atomicMin(first_shared, first);  // an integer minimum: the same whatever the order
    __syncthreads();
    first = *first_shared;
    if (first >= n) return;
    // t'_f = t'_{f - 1} + d_f from the first clipped step on: chunks of 256 differences through LDS, summed by thread 0
    Vec3 run = po_t(par, first - 1);
    for (int base = first; base < n; base += PO_THREADS) {
        const int f = base + threadIdx.x;
        if (f < n) store3(stage[threadIdx.x], load3(clip + (size_t)f * 3));
        __syncthreads();
        if (threadIdx.x == 0) {
            const int count = min(PO_THREADS, n - base);
            for (int j = 0; j < count; ++j) {
                run = run + load3(stage[j]);
                store3(stage[j], run);
            }
        }
        __syncthreads();
        if (f < n) store3(par + (size_t)f * PO_STRIDE + 4, load3(stage[threadIdx.x]));
        __syncthreads();
    }
}

// epoch: the epoch about to run (its predecessor's loss is summed and judged); final: nothing follows, only the judging
__global__ __launch_bounds__(PO_THREADS) void po_prepare_kernel(PoArgs a, int epoch, int final) {
    __shared__ double lds[PO_WAVES][PO_ACC];
    __shared__ double stage[PO_THREADS][3];
    __shared__ int flag, first_shared;
    if (threadIdx.x == 0) flag = a.state->stop;
    __syncthreads();
    if (flag) return;
    if (epoch > 0) {
        const double loss = po_loss_sum(a.partial, a.k.n, lds);
        if (threadIdx.x == 0) {
            PoState s = *a.state;
            a.losses[epoch - 1] = loss;
            if (!(fabs(loss) <= DBL_MAX)) {
                s.nonfinite_epoch = epoch - 1;
                s.stop = 1;
            } else {
                po_schedule(s, a.sched, loss);
            }
            a.rates[epoch - 1] = s.lr;
            if (s.stop || final) s.epochs_run = epoch;
            flag = s.stop;
            *a.state = s;
        }
        __syncthreads();
        if (flag) return;
    }
    if (final) return;
    if (threadIdx.x == 0) {
        a.state->b1k *= a.k.beta1;
        a.state->b2k *= a.k.beta2;
    }
    po_project(a.par[epoch & 1], a.k.n, a.max_distance, a.clip, stage, &first_shared);
}

__global__ __launch_bounds__(PO_THREADS) void po_project_kernel(double *par, int n, double max_distance, double *clip) {
    __shared__ double stage[PO_THREADS][3];
    __shared__ int first_shared;
    po_project(par, n, max_distance, clip, stage, &first_shared);
}

// grid (n).  evaluate = 0: one Adam step from par[epoch & 1] into the other buffer; 1: gradient and loss shares at par[epoch & 1], nothing stepped
template <bool IMAGE2D, bool AFFINE>
__global__ __launch_bounds__(PO_THREADS) void po_step_kernel(PoArgs a, int epoch, int evaluate) {
    __shared__ double lds[PO_WAVES][PO_ACC];
    if (!evaluate && a.state->stop) return;
    const int f = blockIdx.x;
    const double *par = a.par[epoch & 1];
    double acc[PO_ACC];
    for (int j = 0; j < PO_ACC; ++j) acc[j] = 0.0;
    const int end = a.offsets[f + 1];
    for (int e = a.offsets[f] + threadIdx.x; e < end; e += PO_THREADS) {
        const int entry = a.entries[e];
        po_entry<IMAGE2D, AFFINE>(a.k, par, a.raw, a.cam, a.index_i, a.index_j, entry >> 1, entry & 1, acc);
    }
    block_butterfly_sum<PO_ACC>(acc, lds);
    if (threadIdx.x != 0) return;
    po_frame_tail<AFFINE>(a.k, par, f, acc);
    a.partial[f] = acc[9];
    if (evaluate) {
        for (int j = 0; j < PO_STRIDE; ++j) a.grad[(size_t)f * PO_STRIDE + j] = acc[j];
        return;
    }
    po_adam(a.k, par + (size_t)f * PO_STRIDE, acc, a.mom + (size_t)f * 2 * PO_STRIDE, a.state->lr, a.state->b1k, a.state->b2k, AFFINE ? 9 : 7,
            a.par[(epoch + 1) & 1] + (size_t)f * PO_STRIDE);
}

__global__ __launch_bounds__(PO_THREADS) void po_final_loss_kernel(PoArgs a) {
    __shared__ double lds[PO_WAVES][PO_ACC];
    const double loss = po_loss_sum(a.partial, a.k.n, lds);
    if (threadIdx.x == 0) a.state->final_loss = loss;
}

// widens the correspondences; Rigid: the camera-space points ((u - c_x) * depth) / f_x, ((v - c_y) * depth) / f_y, depth, once
__global__ __launch_bounds__(PO_THREADS) void po_widen_kernel(PoConst k, const float *__restrict__ pi, const float *__restrict__ di, const float *__restrict__ pj,
                                                              const float *__restrict__ dj, double *__restrict__ raw, double *__restrict__ cam, PoState *state) {
    const long long e = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (e >= k.m) return;
    double r[6] = {(double)pi[2 * e], (double)pi[2 * e + 1], (double)di[e], (double)pj[2 * e], (double)pj[2 * e + 1], (double)dj[e]};
    for (int j = 0; j < 6; ++j) raw[e * 6 + j] = r[j];
    if (!(r[2] > 0.0 && r[5] > 0.0 && r[2] <= DBL_MAX && r[5] <= DBL_MAX)) atomicOr(&state->bad_depth, 1);
    if (cam) {
        store3(cam + e * 6, po_unproject(k, r[0], r[1], r[2]));
        store3(cam + e * 6 + 3, po_unproject(k, r[3], r[4], r[5]));
    }
}

void po_launch_step(hive_ctx *ctx, const PoArgs &a, bool image2d, bool affine, int epoch, int evaluate) {
    const dim3 grid(a.k.n), block(PO_THREADS);
    if (image2d && affine)
        hipLaunchKernelGGL((po_step_kernel<true, true>), grid, block, 0, ctx->stream, a, epoch, evaluate);
    else if (image2d)
        hipLaunchKernelGGL((po_step_kernel<true, false>), grid, block, 0, ctx->stream, a, epoch, evaluate);
    else if (affine)
        hipLaunchKernelGGL((po_step_kernel<false, true>), grid, block, 0, ctx->stream, a, epoch, evaluate);
    else
        hipLaunchKernelGGL((po_step_kernel<false, false>), grid, block, 0, ctx->stream, a, epoch, evaluate);
}

}  // namespace

extern "C" {

int hive_pose_project(hive_ctx *ctx, double *params, int n_frames, double max_frame_distance) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, params, "pose_project: NULL argument");
    HIVE_REQUIRE(ctx, n_frames >= 1 && n_frames <= (1 << 20), "pose_project: bad frame count %d", n_frames);
    const size_t n = (size_t)n_frames;
    hive_scratch_layout lay;
    double *d_par = nullptr, *d_clip = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        lay.off = 0;
        d_par = lay.take<double>(n * PO_STRIDE);
        d_clip = lay.take<double>(n * 3);
        if (pass == 0) {
            int rc;
            if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay.bytes()))) return rc;
            lay.base = (char *)ctx->d_scratch;
        }
    }
    std::vector<double> rows(n * PO_STRIDE, 0.0);
    for (size_t f = 0; f < n; ++f) memcpy(&rows[f * PO_STRIDE], params + f * 7, 56);
    int rc;
    if ((rc = hive_upload(ctx, d_par, rows.data(), rows.size() * 8))) return rc;
    hipLaunchKernelGGL(po_project_kernel, dim3(1), dim3(PO_THREADS), 0, ctx->stream, d_par, n_frames, max_frame_distance, d_clip);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(rows.data(), d_par, rows.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t f = 0; f < n; ++f) memcpy(params + f * 7, &rows[f * PO_STRIDE], 56);
    return HIVE_OK;
}

int hive_pose_optimise(hive_ctx *ctx, double *params, double *scale, double *shift, int n_frames, double fx, double fy, double cx, double cy,
                       const int64_t *d_index_i, const float *d_points_i, const float *d_depth_i, const int64_t *d_index_j, const float *d_points_j,
                       const float *d_depth_j, int64_t n_matches, const hive_pose_options *options, double max_frame_distance, int check_every, double *losses,
                       double *learning_rates, int *epochs_run, double *final_loss, double *gradient) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, params && options && epochs_run, "pose_optimise: NULL argument");
    const hive_pose_options &o = *options;
    HIVE_REQUIRE(ctx, o.alignment_type != HIVE_POSE_DEFORMABLE, "pose_optimise: Deformable alignment is not implemented (Rigid and Affine are)");
    HIVE_REQUIRE(ctx, o.alignment_type == HIVE_POSE_RIGID || o.alignment_type == HIVE_POSE_AFFINE, "pose_optimise: bad alignment type %d", o.alignment_type);
    HIVE_REQUIRE(ctx, o.residual_type == HIVE_POSE_WORLD3D || o.residual_type == HIVE_POSE_IMAGE2D, "pose_optimise: bad residual type %d", o.residual_type);
    const bool affine = o.alignment_type == HIVE_POSE_AFFINE, image2d = o.residual_type == HIVE_POSE_IMAGE2D;
    HIVE_REQUIRE(ctx, !affine || (scale && shift), "pose_optimise: Affine alignment needs scale and shift");
    HIVE_REQUIRE(ctx, n_frames >= 2 && n_frames <= (1 << 20), "pose_optimise: %d frames (at least 2, at most 2^20)", n_frames);
    HIVE_REQUIRE(ctx, n_matches >= 1 && n_matches < (1ll << 30), "pose_optimise: %lld correspondences (at least 1, fewer than 2^30)", (long long)n_matches);
    HIVE_REQUIRE(ctx, d_index_i && d_points_i && d_depth_i && d_index_j && d_points_j && d_depth_j, "pose_optimise: NULL correspondence array");
    HIVE_REQUIRE(ctx, fx > 0.0 && fy > 0.0 && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy),
                 "pose_optimise: focal lengths must be positive (f_x = %g, f_y = %g)", fx, fy);
    HIVE_REQUIRE(ctx, o.num_epochs >= 0 && o.num_epochs <= (1 << 24), "pose_optimise: bad epoch count %d", o.num_epochs);
    HIVE_REQUIRE(ctx, o.num_epochs == 0 || (losses && learning_rates), "pose_optimise: losses and learning_rates are needed");
    HIVE_REQUIRE(ctx, o.learning_rate > 0.0 && o.min_loss_delta >= 0.0 && o.lr_scheduler_patience >= 0 && o.early_stopping_patience >= 0,
                 "pose_optimise: bad learning rate, loss delta or patience");
    HIVE_REQUIRE(ctx, check_every >= 1, "pose_optimise: check_every = %d", check_every);
    const int n = n_frames, epochs = o.num_epochs;
    const size_t m = (size_t)n_matches;

    // the incidence lists, on the host: frame -> (k, side) ascending, a counting sort over k = 0 .. m - 1, side 0 then 1
    std::vector<int64_t> host_index(2 * m);
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(host_index.data(), d_index_i, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(host_index.data() + m, d_index_j, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> index32(2 * m), offsets((size_t)n + 1, 0), entries(2 * m);
    for (size_t e = 0; e < 2 * m; ++e) {
        const int64_t f = host_index[e];
        HIVE_REQUIRE(ctx, f >= 0 && f < n, "pose_optimise: correspondence %lld names frame %lld on side %s; there are %d frames", (long long)(e % m), (long long)f,
                     e < m ? "i" : "j", n);
        index32[e] = (int32_t)f;
        offsets[(size_t)f + 1] += 1;
    }
    for (int f = 0; f < n; ++f) offsets[(size_t)f + 1] += offsets[(size_t)f];
    {
        std::vector<int32_t> cursor(offsets.begin(), offsets.end() - 1);
        for (size_t k = 0; k < m; ++k) {
            entries[(size_t)cursor[(size_t)index32[k]]++] = (int32_t)(2 * k);
            entries[(size_t)cursor[(size_t)index32[m + k]]++] = (int32_t)(2 * k + 1);
        }
    }

    hive_scratch_layout lay;
    PoArgs a;
    for (int pass = 0; pass < 2; ++pass) {
        lay.off = 0;
        a.state = lay.take<PoState>(1);
        a.par[0] = lay.take<double>((size_t)n * PO_STRIDE);
        a.par[1] = lay.take<double>((size_t)n * PO_STRIDE);
        a.mom = lay.take<double>((size_t)n * 2 * PO_STRIDE);
        a.partial = lay.take<double>((size_t)n);
        a.losses = lay.take<double>((size_t)std::max(epochs, 1));
        a.rates = lay.take<double>((size_t)std::max(epochs, 1));
        a.grad = lay.take<double>((size_t)n * PO_STRIDE);
        a.clip = lay.take<double>((size_t)n * 3);
        a.raw = lay.take<double>(m * 6);
        a.cam = affine ? nullptr : lay.take<double>(m * 6);
        a.index_i = lay.take<int>(m);
        a.index_j = lay.take<int>(m);
        a.offsets = lay.take<int>((size_t)n + 1);
        a.entries = lay.take<int>(2 * m);
        if (pass == 0) {
            int rc;
            if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay.bytes()))) return rc;
            lay.base = (char *)ctx->d_scratch;
        }
    }
    a.k.n = n;
    a.k.m = (long long)m;
    a.k.smooth = o.smooth_trajectory ? 1 : 0;
    a.k.position_only = o.position_only ? 1 : 0;
    a.k.fx = fx;
    a.k.fy = fy;
    a.k.cx = cx;
    a.k.cy = cy;
    a.k.pose_t_reg = o.pose_t_reg;
    a.k.pose_r_reg = o.pose_r_reg;
    a.k.l2 = o.l2_regularisation;
    a.k.beta1 = 0.9;
    a.k.beta2 = 0.999;
    a.k.eps = 1e-8;
    a.sched.threshold = o.min_loss_delta;
    a.sched.lr_patience = o.lr_scheduler_patience;
    a.sched.stop_patience = o.early_stopping_patience;
    a.max_distance = max_frame_distance;

    PoState first = {};
    first.lr = o.learning_rate;
    first.b1k = first.b2k = 1.0;
    first.sched_best = first.stop_best = std::numeric_limits<double>::infinity();
    first.nonfinite_epoch = -1;
    std::vector<double> rows((size_t)n * PO_STRIDE);
    for (int f = 0; f < n; ++f) {
        memcpy(&rows[(size_t)f * PO_STRIDE], params + (size_t)f * 7, 56);
        rows[(size_t)f * PO_STRIDE + 7] = affine ? scale[f] : 1.0;
        rows[(size_t)f * PO_STRIDE + 8] = affine ? shift[f] : 0.0;
    }
    int rc;
    if ((rc = hive_upload(ctx, a.state, &first, sizeof(first)))) return rc;
    if ((rc = hive_upload(ctx, a.par[0], rows.data(), rows.size() * 8))) return rc;
    if ((rc = hive_upload(ctx, (void *)a.index_i, index32.data(), m * 4))) return rc;
    if ((rc = hive_upload(ctx, (void *)a.index_j, index32.data() + m, m * 4))) return rc;
    if ((rc = hive_upload(ctx, (void *)a.offsets, offsets.data(), offsets.size() * 4))) return rc;
    if ((rc = hive_upload(ctx, (void *)a.entries, entries.data(), entries.size() * 4))) return rc;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(a.mom, 0, (size_t)n * 2 * PO_STRIDE * 8, ctx->stream));
    hipLaunchKernelGGL(po_widen_kernel, dim3((unsigned)((m + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, ctx->stream, a.k, d_points_i, d_depth_i, d_points_j,
                       d_depth_j, (double *)a.raw, (double *)a.cam, a.state);
    HIVE_CHECK_HIP(ctx, hipGetLastError());

    PoState now = first;
    auto read_state = [&]() -> int {
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(&now, a.state, sizeof(now), hipMemcpyDeviceToHost, ctx->stream));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return HIVE_OK;
    };
    if ((rc = read_state())) return rc;
    HIVE_REQUIRE(ctx, !now.bad_depth, "pose_optimise: every depth must be positive and finite");
    for (int epoch = 0; epoch < epochs && !now.stop;) {
        const int batch_end = (int)std::min<long long>((long long)epoch + check_every, epochs);
        for (; epoch < batch_end; ++epoch) {
            hipLaunchKernelGGL(po_prepare_kernel, dim3(1), dim3(PO_THREADS), 0, ctx->stream, a, epoch, 0);
            po_launch_step(ctx, a, image2d, affine, epoch, 0);
        }
        if (epoch == epochs) hipLaunchKernelGGL(po_prepare_kernel, dim3(1), dim3(PO_THREADS), 0, ctx->stream, a, epochs, 1);
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        if ((rc = read_state())) return rc;
        if (now.nonfinite_epoch >= 0) return hive_fail(ctx, HIVE_ERR_INVALID, "pose_optimise: the loss of epoch %d is not finite", now.nonfinite_epoch);
    }
    const int ran = now.epochs_run;
    *epochs_run = ran;
    if (final_loss || gradient) {
        po_launch_step(ctx, a, image2d, affine, ran, 1);
        hipLaunchKernelGGL(po_final_loss_kernel, dim3(1), dim3(PO_THREADS), 0, ctx->stream, a);
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        if ((rc = read_state())) return rc;
        if (final_loss) *final_loss = now.final_loss;
    }
    std::vector<double> grad_rows(gradient ? (size_t)n * PO_STRIDE : 0);
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(rows.data(), a.par[ran & 1], rows.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (ran) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(losses, a.losses, (size_t)ran * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (ran) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(learning_rates, a.rates, (size_t)ran * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (gradient) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(gradient, a.grad, (size_t)n * PO_STRIDE * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < n; ++f) {
        memcpy(params + (size_t)f * 7, &rows[(size_t)f * PO_STRIDE], 56);
        if (affine) {
            scale[f] = rows[(size_t)f * PO_STRIDE + 7];
            shift[f] = rows[(size_t)f * PO_STRIDE + 8];
        }
    }
    return HIVE_OK;
}

}  // extern "C"
