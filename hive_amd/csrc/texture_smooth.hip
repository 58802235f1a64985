// Smooths the view labels of texture.hip across the edges of the mesh: one view's areas kept in a table instead of reduced (vote), the edge adjacency of
// any triangle list (face_neighbours), and an iterated-conditional-modes labelling in integers (smooth).  No counterpart in the reference.  gfx950 only.  The
// rules are stated in include/hive_mi355x.h above hive_texture_vote and restated in numpy in tests/texture_smoothing_restatement.py; in short:
//
//   vote        hive_texture_select's candidate test with a sign filter on the snapped area A; area[view][f] = |A| of a candidate, else 0.
//   neighbours  g is listed by f once per unordered vertex pair that is an edge of both; a face with a bad or repeated id lists nothing and is listed nowhere.
//               vertex -> faces lists (count with integer atomics, scan, fill: the order inside a list depends on the run, the SET does not), then per face edge
//               (a, b) a walk of a's list for faces holding b, inserted in ascending order.  Quadratic in a face's degree: fine for surfaces, not for a soup
//               of thousands of faces on one edge.
//   smooth      L[f] = argmax area (lower view on a tie); rounds of propose / apply read from the labels at the round's start, ping-pong; a face applies iff
//               its gain beats every proposing neighbour entry's, ties by mix32 of the face id.  Two launches a round; a device flag makes the launches queued
//               behind convergence no-ops; the host polls once per batch of rounds.  Every sum is an integer: the result depends on the inputs alone.
//
// Kernels: one thread per face (or per vertex / per item of a scan), 256 threads (four wave64) a workgroup; no float arithmetic.
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_TILE = HIVE_SCAN_TILE;  // items per workgroup of the two scans
constexpr int TS_MAX_VIEWS = 65535, TS_MAX_ROUNDS = 4096, TS_BATCH = 8, TS_MAX_DEGREE = 65535;
constexpr long long TS_MAX_AREA = 1ll << 47, TS_MAX_SEAM_COST = 1ll << 40;
constexpr unsigned long long TS_ERR_ADJACENCY = 1, TS_ERR_DEGREE = 2, TS_ERR_AREA = 4, TS_ERR_ROUNDS = 8;
// the u64 words of hive_texture_smooth at hive_ctx::d_scalars + TXS_SCALARS; hive_mesh_face_neighbours keeps its total behind them
enum { TS_DONE = 0, TS_ERR, TS_ROUNDS, TS_CHANGES, TS_SEAMS_BEFORE, TS_SEAMS_AFTER, TS_GIVEN_UP, TS_PROPOSALS /* two, by round parity */, TS_WORDS = TS_PROPOSALS + 2 };
constexpr int NB_TOTAL = TS_WORDS;
static_assert(2 * (NB_TOTAL + 2) <= TXS_SCALARS_WORDS && TXS_SCALARS % 2 == 0, "the block holds the u64 words, 8-byte aligned");

dim3 ts_grid(long long n) { return dim3((unsigned)std::max<long long>(1, (n + TS_THREADS - 1) / TS_THREADS)); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long s) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
// adds the workgroup's values to *at: one integer atomic per wave (the total does not depend on the order)
__device__ __forceinline__ void add_to(unsigned long long *at, unsigned long long mine) {
    const unsigned long long s = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(at, s);
}

// ------------------------------------------------------------------------------------------------------------------------ vote
// (the candidate test is texture_select_kernel's, statement by statement: tests/test_texture_smoothing_gpu.py holds the table's argmax to hive_texture_select's keys)
__global__ __launch_bounds__(TS_THREADS) void texture_vote_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, const int32_t *__restrict__ xy,
                                                                  const double *__restrict__ z, const float *__restrict__ depth, const uint8_t *__restrict__ mask, int H,
                                                                  int W, int facing, double tolerance, long long *__restrict__ row) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    if (f >= nf) return;
    const int id[3] = {faces[3 * f + 0], faces[3 * f + 1], faces[3 * f + 2]};
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && (unsigned long long)id[k] < (unsigned long long)nv;
    long long X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
    for (int k = 0; k < 3 && ok; ++k) {
        const double zk = z[id[k]];
        if (!(zk > 0.0)) {  // a rejected vertex has z = 0
            ok = false;
            break;
        }
        X[k] = xy[2 * (long long)id[k]], Y[k] = xy[2 * (long long)id[k] + 1];
        const long long i = (Y[k] + 128) >> 8, j = (X[k] + 128) >> 8;
        if (i < 0 || i >= H || j < 0 || j >= W) {
            ok = false;
            break;
        }
        const long long px = i * W + j;
        const float d = depth[px];
        ok = !(mask && mask[px]) && (d == 0.f || zk <= (double)d + tolerance);
    }
    const long long A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
    ok = ok && A != 0 && (facing == 0 || (facing > 0 ? A < 0 : A > 0));
    row[f] = ok ? (A < 0 ? -A : A) : 0;
}

// ------------------------------------------------------------------------------------------------------------------------ neighbours
struct NbParams {
    const int32_t *faces;  // [nf][3]
    long long nf, nv;
    unsigned *vcount;   // [nv] faces of a vertex
    unsigned *cursor;   // [nv]
    unsigned *vstart;   // [nv + 1]
    int32_t *vfaces;    // [3 nf]
    unsigned *degree;   // [nf]
    unsigned *blocks;   // block sums of the scan in flight
    __device__ bool load(long long f, int id[3]) const {
        id[0] = faces[3 * f], id[1] = faces[3 * f + 1], id[2] = faces[3 * f + 2];
        return (unsigned long long)id[0] < (unsigned long long)nv && (unsigned long long)id[1] < (unsigned long long)nv &&
               (unsigned long long)id[2] < (unsigned long long)nv && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    }
};

__global__ __launch_bounds__(TS_THREADS) void nb_count_kernel(NbParams p) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    int id[3];
    if (f >= p.nf || !p.load(f, id)) return;
    for (int k = 0; k < 3; ++k) atomicAdd(p.vcount + id[k], 1u);
}

// (the two scans: tile_sums_kernel and tile_offsets_kernel of hive_internal.hpp, shared with texture_level.hip)
__global__ __launch_bounds__(TS_THREADS) void nb_fill_kernel(NbParams p) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    int id[3];
    if (f >= p.nf || !p.load(f, id)) return;
    for (int k = 0; k < 3; ++k) p.vfaces[p.vstart[id[k]] + atomicAdd(p.cursor + id[k], 1u)] = (int32_t)f;
}

// the neighbour entries of face f in the order of the walk: edge (id[k], id[k + 1]), the list of id[k]
template <class Visit>
__device__ __forceinline__ void nb_walk(const NbParams &p, long long f, const int id[3], Visit visit) {
    for (int k = 0; k < 3; ++k) {
        const int a = id[k], b = id[k == 2 ? 0 : k + 1];
        for (unsigned e = p.vstart[a]; e < p.vstart[a + 1]; ++e) {
            const int g = p.vfaces[e];
            if (g == f) continue;
            if (p.faces[3 * (long long)g] == b || p.faces[3 * (long long)g + 1] == b || p.faces[3 * (long long)g + 2] == b) visit(g);
        }
    }
}

__global__ __launch_bounds__(TS_THREADS) void nb_degree_kernel(NbParams p) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    if (f >= p.nf) return;
    int id[3];
    unsigned n = 0;
    if (p.load(f, id)) nb_walk(p, f, id, [&](int) { ++n; });
    p.degree[f] = n;
}

// (offsets: what nb_offsets_kernel made of the degrees; every segment lies inside the capacity the host checked against their total)
__global__ __launch_bounds__(TS_THREADS) void nb_entries_kernel(NbParams p, const long long *__restrict__ offsets, int32_t *__restrict__ out) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    int id[3];
    if (f >= p.nf || !p.load(f, id)) return;
    int32_t *mine = out + offsets[f];
    long long n = 0;
    const long long room = offsets[f + 1] - offsets[f];
    nb_walk(p, f, id, [&](int g) {
        if (n >= room) return;  // (the walk of nb_degree_kernel again: it finds the same entries)
        long long at = n++;
        for (; at > 0 && mine[at - 1] > g; --at) mine[at] = mine[at - 1];  // insertion into the ascending run
        mine[at] = g;
    });
}

// ------------------------------------------------------------------------------------------------------------------------ smooth
struct SmParams {
    const long long *area;  // [n_views][nf]
    int n_views;
    long long nf;
    const long long *offsets;  // [nf + 1]
    const int32_t *nbr;
    long long n_entries;
    long long seam_cost;
    int32_t *label[2];  // [nf] each: round r reads label[r & 1] and writes the other
    int32_t *proposal;  // [nf] the label a face proposes, -1 = none
    long long *gain;    // [nf]
    unsigned long long *sc;
    __device__ bool stopped() const { return sc[TS_DONE] || sc[TS_ERR]; }
};

// checks the adjacency and the table (nothing later reads out of bounds through them) and sets the start labels
__global__ __launch_bounds__(TS_THREADS) void sm_init_kernel(SmParams p) {
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    if (f >= p.nf) return;
    const long long lo = p.offsets[f], hi = p.offsets[f + 1];
    unsigned long long err = 0;
    if (lo < 0 || hi < lo || hi > p.n_entries || (f == 0 && lo != 0))
        err |= TS_ERR_ADJACENCY;
    else if (hi - lo > TS_MAX_DEGREE)
        err |= TS_ERR_DEGREE;
    else
        for (long long e = lo; e < hi; ++e)
            if ((unsigned long long)p.nbr[e] >= (unsigned long long)p.nf || p.nbr[e] == f) err |= TS_ERR_ADJACENCY;
    int best = -1;
    long long most = 0;
    for (int v = 0; v < p.n_views; ++v) {
        const long long a = p.area[(long long)v * p.nf + f];
        if (a < 0 || a >= TS_MAX_AREA) err |= TS_ERR_AREA;
        if (a > most) most = a, best = v;
    }
    p.label[0][f] = best;
    if (err) atomicOr(p.sc + TS_ERR, err);
}

// neighbour entries (f, g) with f < g whose labels are both >= 0 and differ
__device__ __forceinline__ unsigned long long sm_seams(const SmParams &p, long long f, const int32_t *__restrict__ L) {
    const int cur = L[f];
    unsigned long long n = 0;
    if (cur >= 0)
        for (long long e = p.offsets[f]; e < p.offsets[f + 1]; ++e) {
            const int g = p.nbr[e];
            n += g > f && L[g] >= 0 && L[g] != cur;
        }
    return n;
}

__global__ __launch_bounds__(TS_THREADS) void sm_seams_before_kernel(SmParams p) {
    if (p.sc[TS_ERR]) return;
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    add_to(p.sc + TS_SEAMS_BEFORE, f < p.nf ? sm_seams(p, f, p.label[0]) : 0ull);
}

__global__ __launch_bounds__(TS_THREADS) void sm_propose_kernel(SmParams p, int round) {
    if (p.stopped()) return;
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    const int32_t *__restrict__ L = p.label[round & 1];
    int best = -1;
    long long best_gain = 0;
    const int cur = f < p.nf ? L[f] : -1;
    if (cur >= 0) {
        const long long lo = p.offsets[f], hi = p.offsets[f + 1];
        const long long a_cur = p.area[(long long)cur * p.nf + f];
        long long c_cur = 0;
        for (long long e = lo; e < hi; ++e) c_cur += L[p.nbr[e]] == cur;
        for (long long e = lo; e < hi; ++e) {
            const int l = L[p.nbr[e]];
            if (l < 0 || l == cur) continue;
            bool seen = false;  // each label once, at its first entry
            for (long long d = lo; d < e && !seen; ++d) seen = L[p.nbr[d]] == l;
            if (seen) continue;
            const long long a_l = p.area[(long long)l * p.nf + f];
            if (a_l == 0) continue;
            long long c_l = 0;
            for (long long d = e; d < hi; ++d) c_l += L[p.nbr[d]] == l;
            const long long g = (a_l - a_cur) + p.seam_cost * (c_l - c_cur);
            if (g > best_gain || (g == best_gain && best >= 0 && l < best)) best_gain = g, best = l;
        }
    }
    if (f < p.nf) {
        p.proposal[f] = best;
        p.gain[f] = best_gain;
    }
    add_to(p.sc + TS_PROPOSALS + (round & 1), best >= 0 ? 1ull : 0ull);
}

// (only a round without proposals sets TS_DONE, and in such a round no thread has anything to do: a workgroup that starts late and sees the flag loses nothing)
__global__ __launch_bounds__(TS_THREADS) void sm_apply_kernel(SmParams p, int round) {
    if (p.stopped()) return;
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    if (p.sc[TS_PROPOSALS + (round & 1)] == 0) {
        if (f == 0) p.sc[TS_DONE] = 1;
        return;
    }
    if (f == 0) {
        if (round >= TS_MAX_ROUNDS) atomicOr(p.sc + TS_ERR, TS_ERR_ROUNDS);
        p.sc[TS_ROUNDS] = (unsigned long long)round + 1;
        p.sc[TS_PROPOSALS + ((round + 1) & 1)] = 0;  // the next round's count: nobody reads or adds to it during this launch
    }
    unsigned long long changed = 0;
    if (f < p.nf) {
        int l = p.label[round & 1][f];
        const int mine = p.proposal[f];
        if (mine >= 0) {
            const long long g_f = p.gain[f];
            const unsigned h_f = mix32((unsigned)f);
            bool wins = true;
            for (long long e = p.offsets[f]; e < p.offsets[f + 1] && wins; ++e) {
                const int g = p.nbr[e];
                if (p.proposal[g] < 0) continue;
                const long long g_g = p.gain[g];
                wins = g_f > g_g || (g_f == g_g && h_f < mix32((unsigned)g));
            }
            if (wins) l = mine, changed = 1;
        }
        p.label[(round + 1) & 1][f] = l;
    }
    add_to(p.sc + TS_CHANGES, changed);
}

__global__ __launch_bounds__(TS_THREADS) void sm_finish_kernel(SmParams p, unsigned long long *__restrict__ best) {
    if (p.sc[TS_ERR]) return;
    const long long f = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
    const int32_t *__restrict__ L = p.label[p.sc[TS_ROUNDS] & 1];
    unsigned long long seams = 0, given_up = 0;
    if (f < p.nf) {
        const int l = L[f];
        long long most = 0;
        for (int v = 0; v < p.n_views; ++v) most = max(most, p.area[(long long)v * p.nf + f]);
        const long long a = l >= 0 ? p.area[(long long)l * p.nf + f] : 0;
        best[f] = l >= 0 ? ((unsigned long long)a << 16) | (unsigned long long)(65535 - l) : 0ull;
        given_up = (unsigned long long)(most - a);
        seams = sm_seams(p, f, L);
    }
    add_to(p.sc + TS_SEAMS_AFTER, seams);
    add_to(p.sc + TS_GIVEN_UP, given_up);
}

}  // namespace

extern "C" {

int hive_texture_vote(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const double *d_z, const float *d_depth,
                      const uint8_t *d_mask, int H, int W, int view_index, double depth_tolerance, int facing, int64_t *d_area) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && ((long long)H + 1) * ((long long)W + 1) <= (1ll << 31), "texture_vote: bad screen size %d x %d", H, W);
    HIVE_REQUIRE(ctx, nf >= 0 && nf < (1ll << 31) && nv >= 0 && nv < (1ll << 31), "texture_vote: bad counts %lld faces, %lld vertices", (long long)nf, (long long)nv);
    HIVE_REQUIRE(ctx, view_index >= 0 && view_index < TS_MAX_VIEWS, "texture_vote: view_index %d outside [0, 65535)", view_index);
    // (the row of the last view is refused when n_views * nf >= 2^31: a table of that size has no complete set of rows)
    HIVE_REQUIRE(ctx, ((long long)view_index + 1) * nf < (1ll << 31), "texture_vote: row %d of %lld faces ends at or past entry 2^31 of the table", view_index, (long long)nf);
    HIVE_REQUIRE(ctx, depth_tolerance >= 0.0, "texture_vote: depth_tolerance must be >= 0");  // (false for a NaN)
    HIVE_REQUIRE(ctx, facing >= -1 && facing <= 1, "texture_vote: facing %d is none of -1, 0, 1", facing);
    if (nf == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_faces && d_area && (nv == 0 || (d_xy && d_z && d_depth)), "texture_vote: NULL argument");
    hipLaunchKernelGGL(texture_vote_kernel, ts_grid(nf), dim3(TS_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, d_xy, d_z, d_depth, d_mask, H, W, facing,
                       depth_tolerance, (long long *)d_area + (long long)view_index * nf);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_mesh_face_neighbours(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, int64_t *d_offsets, int32_t *d_neighbours, int64_t capacity,
                              int64_t *total) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, total && d_offsets, "mesh_face_neighbours: NULL argument");
    *total = 0;
    HIVE_REQUIRE(ctx, nf >= 0 && 3 * nf < (1ll << 31) && nv >= 0 && nv < (1ll << 31), "mesh_face_neighbours: bad counts %lld faces, %lld vertices", (long long)nf,
                 (long long)nv);
    HIVE_REQUIRE(ctx, capacity >= 0 && (capacity == 0 || d_neighbours) && (nf == 0 || d_faces), "mesh_face_neighbours: NULL argument or a negative capacity");
    hipStream_t s = ctx->stream;
    if (nf == 0 || nv == 0) {  // no face, or none with an id in range: nf + 1 zeros
        HIVE_CHECK_HIP(ctx, hipMemsetAsync(d_offsets, 0, (size_t)(nf + 1) * sizeof(int64_t), s));
        return HIVE_OK;
    }
    NbParams p{};
    p.faces = d_faces, p.nf = nf, p.nv = nv;
    const int nb_v = hive_div_up(nv + 1, TS_TILE), nb_f = hive_div_up(nf + 1, TS_TILE);
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        p.vcount = L.take<unsigned>(2 * (size_t)nv);  // the counts and, behind them, the cursors: one memset
        p.cursor = p.vcount ? p.vcount + nv : nullptr;
        p.vstart = L.take<unsigned>((size_t)nv + 1);
        p.vfaces = L.take<int32_t>(3 * (size_t)nf);
        p.degree = L.take<unsigned>((size_t)nf);
        p.blocks = L.take<unsigned>((size_t)std::max(nb_v, nb_f));
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    unsigned long long *d_total = (unsigned long long *)(ctx->d_scalars + TXS_SCALARS) + NB_TOTAL;
    const dim3 blk(TS_THREADS);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(p.vcount, 0, 2 * (size_t)nv * sizeof(unsigned), s));
    hipLaunchKernelGGL(nb_count_kernel, ts_grid(nf), blk, 0, s, p);
    hipLaunchKernelGGL(tile_sums_kernel<TS_TILE>, dim3(nb_v), blk, 0, s, (const unsigned *)p.vcount, (long long)nv, p.blocks);
    hive_scan_counts(ctx, nb_v, d_total + 1, p.blocks);
    hipLaunchKernelGGL((tile_offsets_kernel<TS_TILE, unsigned>), dim3(nb_v), blk, 0, s, (const unsigned *)p.vcount, (long long)nv, (const unsigned *)p.blocks, p.vstart);
    hipLaunchKernelGGL(nb_fill_kernel, ts_grid(nf), blk, 0, s, p);
    hipLaunchKernelGGL(nb_degree_kernel, ts_grid(nf), blk, 0, s, p);
    hipLaunchKernelGGL(tile_sums_kernel<TS_TILE>, dim3(nb_f), blk, 0, s, (const unsigned *)p.degree, (long long)nf, p.blocks);
    hive_scan_counts(ctx, nb_f, d_total, p.blocks);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    void *pinned;
    if ((rc = hive_pinned_small(ctx, &pinned))) return rc;
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(pinned, d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
    const unsigned long long n = *(volatile unsigned long long *)pinned;
    *total = (int64_t)n;
    // (the scanned block sums are 32-bit words: a larger total would have wrapped in them)
    HIVE_REQUIRE(ctx, n < (1ull << 31), "mesh_face_neighbours: %llu entries: the adjacency holds fewer than 2^31", n);
    HIVE_REQUIRE(ctx, (unsigned long long)capacity >= n, "mesh_face_neighbours: capacity %lld is too small: the adjacency has %llu entries", (long long)capacity, n);
    hipLaunchKernelGGL((tile_offsets_kernel<TS_TILE, long long>), dim3(nb_f), blk, 0, s, (const unsigned *)p.degree, (long long)nf, (const unsigned *)p.blocks, (long long *)d_offsets);
    if (n) hipLaunchKernelGGL(nb_entries_kernel, ts_grid(nf), blk, 0, s, p, (const long long *)d_offsets, d_neighbours);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_texture_smooth(hive_ctx *ctx, const int64_t *d_area, int n_views, int64_t nf, const int64_t *d_offsets, const int32_t *d_neighbours, int64_t n_entries,
                        int64_t seam_cost, int rounds_per_poll, uint64_t *d_best, int64_t stats[5]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n_views > 0 && n_views <= TS_MAX_VIEWS, "texture_smooth: %d views outside [1, 65535]", n_views);
    HIVE_REQUIRE(ctx, nf >= 0 && (long long)n_views * nf < (1ll << 31), "texture_smooth: %d views x %lld faces: the table holds fewer than 2^31 entries", n_views,
                 (long long)nf);
    HIVE_REQUIRE(ctx, seam_cost >= 0 && seam_cost < TS_MAX_SEAM_COST, "texture_smooth: seam_cost %lld outside [0, 2^40)", (long long)seam_cost);
    HIVE_REQUIRE(ctx, n_entries >= 0 && n_entries < (1ll << 31), "texture_smooth: %lld neighbour entries outside [0, 2^31)", (long long)n_entries);
    HIVE_REQUIRE(ctx, rounds_per_poll >= 0 && rounds_per_poll <= TS_MAX_ROUNDS, "texture_smooth: rounds_per_poll %d outside [0, 4096]", rounds_per_poll);
    if (stats) memset(stats, 0, 5 * sizeof(int64_t));
    if (nf == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_area && d_offsets && d_best && (n_entries == 0 || d_neighbours), "texture_smooth: NULL argument");
    SmParams p{};
    p.area = (const long long *)d_area, p.n_views = n_views, p.nf = nf;
    p.offsets = (const long long *)d_offsets, p.nbr = d_neighbours, p.n_entries = n_entries, p.seam_cost = seam_cost;
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        p.label[0] = L.take<int32_t>((size_t)nf);
        p.label[1] = L.take<int32_t>((size_t)nf);
        p.proposal = L.take<int32_t>((size_t)nf);
        p.gain = L.take<long long>((size_t)nf);
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    p.sc = (unsigned long long *)(ctx->d_scalars + TXS_SCALARS);
    hipStream_t s = ctx->stream;
    const dim3 grid = ts_grid(nf), blk(TS_THREADS);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(p.sc, 0, TS_WORDS * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(sm_init_kernel, grid, blk, 0, s, p);
    hipLaunchKernelGGL(sm_seams_before_kernel, grid, blk, 0, s, p);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    void *pinned;
    if ((rc = hive_pinned_small(ctx, &pinned))) return rc;
    volatile unsigned long long *back = (volatile unsigned long long *)pinned;
    // rounds in batches; between batches one small read-back says whether to go on.  A round is the same whichever batch it falls in.
    const int batch = rounds_per_poll ? rounds_per_poll : TS_BATCH;
    for (int round = 0;;) {
        for (int r = 0; r < batch && round <= TS_MAX_ROUNDS; ++r, ++round) {
            hipLaunchKernelGGL(sm_propose_kernel, grid, blk, 0, s, p, round);
            hipLaunchKernelGGL(sm_apply_kernel, grid, blk, 0, s, p, round);
        }
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(pinned, p.sc, TS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
        if (back[TS_DONE] || back[TS_ERR]) break;
        if (round > TS_MAX_ROUNDS) return hive_fail(ctx, HIVE_ERR_STATE, "texture_smooth: the round loop did not end");
    }
    const unsigned long long err = back[TS_ERR];
    if (err & TS_ERR_ADJACENCY)
        return hive_fail(ctx, HIVE_ERR_INVALID, "texture_smooth: the adjacency is not one of %lld faces and %lld entries (offsets ascending from 0, ids in range, no face its own neighbour)",
                         (long long)nf, (long long)n_entries);
    if (err & TS_ERR_DEGREE) return hive_fail(ctx, HIVE_ERR_INVALID, "texture_smooth: a face has 65536 or more neighbour entries");
    if (err & TS_ERR_AREA) return hive_fail(ctx, HIVE_ERR_INVALID, "texture_smooth: an area outside [0, 2^47)");
    if (err & TS_ERR_ROUNDS) return hive_fail(ctx, HIVE_ERR_STATE, "texture_smooth: %d rounds and faces still propose", TS_MAX_ROUNDS);
    hipLaunchKernelGGL(sm_finish_kernel, grid, blk, 0, s, p, (unsigned long long *)d_best);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    if (stats) {
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(pinned, p.sc, TS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
        stats[0] = (int64_t)back[TS_ROUNDS], stats[1] = (int64_t)back[TS_CHANGES], stats[2] = (int64_t)back[TS_SEAMS_BEFORE];
        stats[3] = (int64_t)back[TS_SEAMS_AFTER], stats[4] = (int64_t)back[TS_GIVEN_UP];
    }
    return HIVE_OK;
}

}  // extern "C"
