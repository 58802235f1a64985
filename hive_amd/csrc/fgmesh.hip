// Foreground per-frame meshing: the inner loops of Pipeline._create_scene (/root/reference/hive/pipeline.py:340-483) that sit
// behind point_cloud_from_depth (csrc/geometry.hip), for gfx950.
//
//   hive_grid_mesh     _triangulate_faces (:651-667) + _filter_faces (:670-694).  The reference runs a Delaunay triangulation
//                      (Qhull) over the valid pixels' integer (u, v) coordinates and then drops every face that has an edge
//                      longer than max_pixel_distance pixels or spanning more than max_depth_distance metres.  The points
//                      ARE a pixel lattice, so the triangulation is implicit: every 2 x 2 pixel block whose corners are valid
//                      gives the two halves of its unit square (fixed diagonal top-right / bottom-left), a block with exactly
//                      three valid corners gives their triangle; no point set, no Qhull.  Faces index the rows of
//                      point_cloud_from_depth's output (valid pixels in row-major order) and are wound like the reference's
//                      reversed simplices (negative cross product in (u, v)).  Delaunay of a lattice also BRIDGES an invalid pixel whose
//                      4-neighbours are valid: the triangle through three of them has the hole as its circumcentre (radius 1, no valid
//                      point inside) and sides (sqrt 2, sqrt 2, 2), which pass the default 2-pixel limit; with all four neighbours valid
//                      the diamond is split along one of its diagonals (they are co-circular: Qhull's arbitrary choice, here west - east).
//                      These are the only triangles of a lattice Delaunay whose sides are all <= 2: with them the face SET after the
//                      filter equals the reference's up to the diagonal inside each co-circular unit square / diamond
//                      (tests/test_fgmesh_gpu.py against scipy's Delaunay).
//   hive_texture_window _get_mesh_texture_and_uv (:782-808): project the vertices (world2image, its default int32 pixels), their
//                      bounding box (the crop of the frame that becomes the texture), uv relative to the box's corner.
//
// All integer work (vertex ids, face lists, the crop window) is exact; the filter compares in the reference's types
// (float32 depth differences, float64 pixel distances).
#include "mesh_compact.hpp"

namespace {

// a workgroup takes TILE (mesh_compact.hpp) pixels, and the 2 x 2 blocks by their top-left pixel

__device__ __forceinline__ bool px_valid(const float *depth, const uint8_t *mask, int i) { return (!mask || mask[i]) && depth[i] > 0.0f; }

struct GridParams {
    int H, W;
    double max_px;    // max_pixel_distance, compared in float64 (points2d is an integer array: np.linalg.norm gives float64)
    float max_depth;  // max_depth_distance, compared in float32 (depth is a float32 array)
};

__device__ __forceinline__ bool edge_ok(const GridParams &p, const float *depth, int a, int b, int du, int dv) {
    const double dist = sqrt((double)(du * du + dv * dv));
    return dist <= p.max_px && fabsf(depth[a] - depth[b]) <= p.max_depth;
}

// triangles that belong to pixel i = (v, u), in order: those of the 2 x 2 block whose top-left pixel it is (corners a b / c d), then, where
// pixel i itself is invalid, the triangles that bridge it (4-neighbours n / w e / s).  Returns the count and the corners (pixel indices).
constexpr int MAX_PIXEL_FACES = 4;
__device__ __forceinline__ int pixel_faces(const GridParams &p, const float *depth, const uint8_t *mask, int i, int (&tri)[MAX_PIXEL_FACES][3]) {
    const int v = i / p.W, u = i - v * p.W;
    int n = 0;
    // every triangle is listed clockwise-on-screen-with-v-down reversed, i.e. with a negative (u, v) cross product
    auto push = [&](int p0, int p1, int p2, bool ok) {
        if (ok) {
            tri[n][0] = p0;
            tri[n][1] = p1;
            tri[n][2] = p2;
            ++n;
        }
    };
    if (v + 1 < p.H && u + 1 < p.W) {
        const int a = i, b = i + 1, c = i + p.W, d = i + p.W + 1;
        const bool va = px_valid(depth, mask, a), vb = px_valid(depth, mask, b), vc = px_valid(depth, mask, c), vd = px_valid(depth, mask, d);
        const int nv = va + vb + vc + vd;
        if (nv >= 3) {
            const bool e_ab = va && vb && edge_ok(p, depth, a, b, 1, 0), e_ac = va && vc && edge_ok(p, depth, a, c, 0, 1);
            const bool e_bd = vb && vd && edge_ok(p, depth, b, d, 0, 1), e_cd = vc && vd && edge_ok(p, depth, c, d, 1, 0);
            const bool e_bc = vb && vc && edge_ok(p, depth, b, c, 1, 1), e_ad = va && vd && edge_ok(p, depth, a, d, 1, 1);
            if (nv == 4) {            // diagonal b - c
                push(a, c, b, e_ab && e_ac && e_bc);
                push(b, c, d, e_bd && e_cd && e_bc);
            } else if (!vd) {
                push(a, c, b, e_ab && e_ac && e_bc);
            } else if (!va) {
                push(b, c, d, e_bd && e_cd && e_bc);
            } else if (!vb) {
                push(a, c, d, e_ac && e_cd && e_ad);
            } else {  // !vc
                push(a, d, b, e_ab && e_bd && e_ad);
            }
        }
    }
    if (!px_valid(depth, mask, i)) {  // a hole: bridged where at least three of its 4-neighbours are valid -- a neighbour outside the image counts as invalid, so a
        // one-pixel hole ON the border with its three in-image neighbours valid gets its (sqrt 2, sqrt 2, 2) triangle too, as Delaunay gives it
        const int nn = i - p.W, ss = i + p.W, ww = i - 1, ee = i + 1;
        const bool vn = v > 0 && px_valid(depth, mask, nn), vs = v + 1 < p.H && px_valid(depth, mask, ss);
        const bool vw = u > 0 && px_valid(depth, mask, ww), ve = u + 1 < p.W && px_valid(depth, mask, ee);
        if (vn + vs + vw + ve >= 3) {
            const bool e_we = vw && ve && edge_ok(p, depth, ww, ee, 2, 0), e_ns = vn && vs && edge_ok(p, depth, nn, ss, 0, 2);
            const bool e_wn = vw && vn && edge_ok(p, depth, ww, nn, 1, 1), e_ne = vn && ve && edge_ok(p, depth, nn, ee, 1, 1);
            const bool e_ws = vw && vs && edge_ok(p, depth, ww, ss, 1, 1), e_se = vs && ve && edge_ok(p, depth, ss, ee, 1, 1);
            if (vw && ve) {           // (all four valid: the west - east diagonal)
                push(ww, ee, nn, vn && e_we && e_wn && e_ne);
                push(ww, ss, ee, vs && e_we && e_ws && e_se);
            } else if (!vw) {
                push(nn, ss, ee, e_ns && e_ne && e_se);
            } else {  // !ve
                push(nn, ww, ss, e_ns && e_wn && e_ws);
            }
        }
    }
    return n;
}

__global__ __launch_bounds__(256) void grid_count_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, GridParams p,
                                                         unsigned *__restrict__ blk_valid, unsigned *__restrict__ blk_faces) {
    __shared__ unsigned lds[8];
    const int n = p.H * p.W;
    unsigned c[2] = {0, 0};  // valid pixels, faces
    for (int j = 0; j < TILE / 256; ++j) {
        const int i = blockIdx.x * TILE + threadIdx.x * (TILE / 256) + j;
        if (i < n) {
            c[0] += px_valid(depth, mask, i);
            int tri[MAX_PIXEL_FACES][3];
            c[1] += (unsigned)pixel_faces(p, depth, mask, i, tri);
        }
    }
    block_sum(c, lds);
    if (threadIdx.x == 0) {
        blk_valid[blockIdx.x] = c[0];
        blk_faces[blockIdx.x] = c[1];
    }
}

// point_cloud_from_depth's rows (csrc/geometry.hip unproject_write_kernel's arithmetic, verbatim): vertex vid[i] of valid pixel i
struct FrameMeshCam {
    double Kinv[9], R[9], t[3];
};
__global__ __launch_bounds__(256) void grid_vertices_kernel(const float *__restrict__ depth, const int *__restrict__ vid, int n, int W, FrameMeshCam p,
                                                            double *__restrict__ out_xyz, long long capacity) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long id = vid[i];
    if (id < 0 || id >= capacity) return;
    const double d = (double)depth[i];
    const double pu = (double)(i % W), pv = (double)(i / W);
    double cam[3];
    for (int r = 0; r < 3; ++r) cam[r] = d * (p.Kinv[3 * r + 0] * pu + p.Kinv[3 * r + 1] * pv + p.Kinv[3 * r + 2]) - p.t[r];
    for (int r = 0; r < 3; ++r) out_xyz[3 * id + r] = p.R[0 * 3 + r] * cam[0] + p.R[1 * 3 + r] * cam[1] + p.R[2 * 3 + r] * cam[2];
}

// vid[i] = row of pixel i in point_cloud_from_depth's output, or -1
__global__ __launch_bounds__(256) void grid_vid_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, int n,
                                                       const unsigned *__restrict__ blk_valid, int *__restrict__ vid) {
    __shared__ unsigned lds[4];
    const int base = blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    bool ok[TILE / 256];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        ok[j] = base + j < n && px_valid(depth, mask, base + j);
        c += ok[j];
    }
    unsigned id = blk_valid[blockIdx.x] + block_exclusive(c, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j)
        if (base + j < n) vid[base + j] = ok[j] ? (int)id++ : -1;
}

__global__ __launch_bounds__(256) void grid_faces_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, GridParams p,
                                                         const unsigned *__restrict__ blk_faces, const int *__restrict__ vid,
                                                         int32_t *__restrict__ faces, long long capacity) {
    __shared__ unsigned lds[4];
    const int n = p.H * p.W;
    const int base = blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    int tri[TILE / 256][MAX_PIXEL_FACES][3];
    int cnt[TILE / 256];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        cnt[j] = base + j < n ? pixel_faces(p, depth, mask, base + j, tri[j]) : 0;
        c += (unsigned)cnt[j];
    }
    long long f = (long long)blk_faces[blockIdx.x] + block_exclusive(c, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j)
        for (int k = 0; k < cnt[j]; ++k, ++f)
            if (f < capacity) {
                faces[3 * f + 0] = vid[tri[j][k][0]];
                faces[3 * f + 1] = vid[tri[j][k][1]];
                faces[3 * f + 2] = vid[tri[j][k][2]];
            }
}

// _filter_faces on an explicit face list (any triangulation): keep face f iff all three edges pass both limits; order kept.
struct FilterParams {
    const int32_t *points2d;  // [n][2] (u, v)
    const float *depth;       // [n]
    const int32_t *faces;     // [F][3]
    long long F;
    double max_px;
    float max_depth;
};

__device__ __forceinline__ bool face_ok(const FilterParams &p, long long f) {
    const int i0 = p.faces[3 * f], i1 = p.faces[3 * f + 1], i2 = p.faces[3 * f + 2];
    const int e[3][2] = {{i0, i1}, {i2, i1}, {i0, i2}};  // faces[:, [0, 2, 0]] against faces[:, [1, 1, 2]]
    for (int k = 0; k < 3; ++k) {
        const int a = e[k][0], b = e[k][1];
        const long long du = (long long)p.points2d[2 * a] - p.points2d[2 * b], dv = (long long)p.points2d[2 * a + 1] - p.points2d[2 * b + 1];
        if (!(sqrt((double)(du * du + dv * dv)) <= p.max_px)) return false;
        if (!(fabsf(p.depth[a] - p.depth[b]) <= p.max_depth)) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void filter_count_kernel(FilterParams p, unsigned *__restrict__ blk) {
    __shared__ unsigned lds[4];
    unsigned c[1] = {0};
    for (int j = 0; j < TILE / 256; ++j) {
        const long long f = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256) + j;
        if (f < p.F) c[0] += face_ok(p, f);
    }
    block_sum(c, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = c[0];
}

__global__ __launch_bounds__(256) void filter_write_kernel(FilterParams p, const unsigned *__restrict__ blk, int32_t *__restrict__ out) {
    __shared__ unsigned lds[4];
    const long long base = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    bool ok[TILE / 256];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        ok[j] = base + j < p.F && face_ok(p, base + j);
        c += ok[j];
    }
    long long o = (long long)blk[blockIdx.x] + block_exclusive(c, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j)
        if (ok[j]) {
            out[3 * o + 0] = p.faces[3 * (base + j) + 0];
            out[3 * o + 1] = p.faces[3 * (base + j) + 1];
            out[3 * o + 2] = p.faces[3 * (base + j) + 2];
            ++o;
        }
}

struct WindowParams {
    double K[9], R[9], t[3];
    double scale;
};

// uv = world2image(points) in its default int32 form (np.round, half to even -- geometric.py:175-178); bbox = {min, max} per axis
// (int atomics) over an initial INT_MAX, INT_MAX, INT_MIN, INT_MIN.  The point count is the host's (n_ptr null, n_or_capacity = n) or lives in device
// memory (the frame path: the vertex count is known to the device only), bounded by n_or_capacity.
__global__ __launch_bounds__(256) void window_project_kernel(const double *__restrict__ pts, const unsigned *__restrict__ n_ptr, long long n_or_capacity, WindowParams p,
                                                             int32_t *__restrict__ uv, int *__restrict__ out) {
    const long long n = n_ptr ? min((long long)*n_ptr, n_or_capacity) : n_or_capacity;
    int mn_u = 0x7fffffff, mn_v = 0x7fffffff, mx_u = (int)0x80000000, mx_v = (int)0x80000000;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        double cam[3], c[3];
        for (int r = 0; r < 3; ++r) cam[r] = p.R[3 * r + 0] * X[0] + p.R[3 * r + 1] * X[1] + p.R[3 * r + 2] * X[2] + p.t[r];
        for (int r = 0; r < 3; ++r) c[r] = p.K[3 * r + 0] * cam[0] + p.K[3 * r + 1] * cam[1] + p.K[3 * r + 2] * cam[2];
        const double u = c[0] / c[2] / p.scale, v = c[1] / c[2] / p.scale;
        const int ru = (int)rint(u), rv = (int)rint(v);  // np.round: half to even
        uv[2 * i + 0] = ru;
        uv[2 * i + 1] = rv;
        mn_u = min(mn_u, ru);
        mx_u = max(mx_u, ru);
        mn_v = min(mn_v, rv);
        mx_v = max(mx_v, rv);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn_u = min(mn_u, __shfl_xor(mn_u, off));
        mx_u = max(mx_u, __shfl_xor(mx_u, off));
        mn_v = min(mn_v, __shfl_xor(mn_v, off));
        mx_v = max(mx_v, __shfl_xor(mx_v, off));
    }
    if ((threadIdx.x & 63) == 0 && mn_u != 0x7fffffff) {  // (a wave without points: its atomics would change nothing)
        atomicMin(out + 0, mn_u);
        atomicMin(out + 1, mn_v);
        atomicMax(out + 2, mx_u);
        atomicMax(out + 3, mx_v);
    }
}

__global__ __launch_bounds__(256) void window_shift_kernel(int32_t *__restrict__ uv, const unsigned *__restrict__ n_ptr, long long n_or_capacity, const int *__restrict__ bbox) {
    const long long n = n_ptr ? min((long long)*n_ptr, n_or_capacity) : n_or_capacity;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        uv[2 * i + 0] -= bbox[0];
        uv[2 * i + 1] -= bbox[1];
    }
}


// ---- _cleanup_with_connected_components (/root/reference/hive/pipeline.py:741-779): floater removal by edge-connected components --------------------
// trimesh.graph.face_adjacency pairs two faces when they share an edge (unordered vertex pair) that exactly two faces use; the components of that graph --
// over the faces that have at least one such neighbour -- with at least min_len faces survive: all of them, or (objects) the largest, the one with the
// smallest face index on a tie.  Six steps, every count and index exact:
//   edge table   open-addressing hash of the face-edges keyed (min << 32) | max (vertex ids < 2^30, so ~0 is free as the empty key); slot of every face-edge
//   edge users   per slot: the number of face-edges on it and the smallest face among them (a separate launch: every insert has landed)
//   union-find   per face-edge on a slot with exactly two users whose smallest face is another face: union the two; roots hook the larger under the smaller
//                with agent-scope CAS, parents are read through agent-scope atomics (workgroups on other XCDs see the hooks, not their stale L2 lines)
//   labels       every face's root = the smallest face of its component; per root the faces that have a neighbour (wave-aggregated atomics)
//   selection    one 64-bit atomicMax of (size << 32) | ~root over the roots whose size passes min_len (the largest; on a tie the smallest root)
//   compaction   the surviving faces in order, the vertices an input face references in order (trimesh's process=True), faces remapped: mesh_compact.hpp
// Every bounded loop that runs out (table full, a CAS that keeps losing) and every out-of-range vertex id sets a bit of the error word instead of spinning.
constexpr unsigned long long CC_EMPTY = ~0ull;
constexpr int CC_ERR_TABLE = 1, CC_ERR_VERTEX = 2, CC_ERR_UNION = 4;
constexpr int CC_CAS_CAP = 1 << 16;

// scalar block of a clean-up (hive_ctx::d_scalars + CC_SCALARS): [0] vertices in, [1] faces in, [2] error word, [4..5] selection (u64),
// [6] vertices out, [7] faces out, [8..11] the texture window's box (hive_fg_frame_mesh_cc): [0..11] is the frame path's one read-back.  CC_SCALARS and its
// extent: the map in hive_internal.hpp

struct CCParams {
    const unsigned *counts;       // [0] V, [1] F (device)
    unsigned *err;
    unsigned long long *best;
    long long face_cap, vert_cap;  // the sizes the scratch was laid out for (bounds on the device counts)
    long long table_cap;           // slots allocated (a power of two)
    const int32_t *faces;          // [F][3]
    unsigned long long *keys;      // [table]
    unsigned *users;               // [table] face-edges on the slot
    int *first;                    // [table] smallest face on the slot
    int *slot;                     // [3 F]
    int *parent;                   // [F] union-find forest
    int *label;                    // [F] root of every face (a separate array: path halving may still rewrite parent entries behind a finished find)
    uint8_t *has_nbr;              // [F]
    unsigned *size;                // [F] faces with a neighbour per root
    uint8_t *referenced;           // [V]
    int *vmap;                     // [V] compacted index or -1
    double min_len;
    int is_object;

    __device__ long long nf() const { return min((long long)counts[1], face_cap); }
    __device__ long long nv() const { return min((long long)counts[0], vert_cap); }
    __device__ bool passes(unsigned component_size) const { return component_size > 0 && (double)component_size >= min_len; }
    // the compaction (mesh_compact.hpp): the vertices an input face references, the faces of the surviving components
    __device__ bool keep_vertex(long long i) const { return referenced[i]; }
    __device__ bool keep_face(long long f) const {
        if (!has_nbr[f]) return false;
        const int r = label[f];
        if (!passes(size[r])) return false;
        if (!is_object) return true;
        const unsigned long long b = *best;  // cc_select_kernel: (size << 32) | ~root of the largest component
        return b && (unsigned)~(unsigned)r == (unsigned)b;
    }
    __device__ int face_vertex(long long f, int k) const {  // (an id out of range has set the error word already: the call fails, the read stays in bounds)
        const int v = faces[3 * f + k];
        return v >= 0 && v < nv() ? vmap[v] : -1;
    }
};
// slots in use for F faces: the power of two >= 4 F (at most 3 F distinct edges: load <= 3 / 4), at least 64, within what was allocated
__device__ __forceinline__ unsigned long long cc_table(const CCParams &p) {
    unsigned long long c = 64;
    while (c < 4ull * (unsigned long long)p.nf() && (long long)c < p.table_cap) c <<= 1;
    return c;
}
__device__ __forceinline__ unsigned long long cc_hash(unsigned long long k) {  // splitmix64 finaliser
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
__device__ __forceinline__ int cc_load(const int *a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int *a, int v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving (every parent is an ancestor: parent[x] <= x, a non-root never becomes a root again)
__device__ __forceinline__ int cc_find(int *parent, int x) {
    int p = cc_load(parent + x);
    while (p != x) {
        const int gp = cc_load(parent + p);
        if (gp != p) cc_store(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__global__ __launch_bounds__(256) void cc_init_kernel(CCParams p) {
    const unsigned long long table = cc_table(p);
    const long long nf = p.nf(), nv = p.nv();
    const long long n = max((long long)table, max(nf, nv));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *p.err = 0;
        *p.best = 0;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (i < (long long)table) {
            p.keys[i] = CC_EMPTY;
            p.users[i] = 0;
            p.first[i] = 0x7fffffff;
        }
        if (i < nf) {
            p.parent[i] = (int)i;
            p.has_nbr[i] = 0;
            p.size[i] = 0;
        }
        if (i < nv) p.referenced[i] = nf == 0;  // trimesh keeps every vertex of a mesh without faces
    }
}

__global__ __launch_bounds__(256) void cc_insert_kernel(CCParams p) {
    const unsigned long long mask = cc_table(p) - 1;
    const long long nf = p.nf(), nv = p.nv();
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < 3 * nf; e += (long long)gridDim.x * 256) {
        const long long f = e / 3;
        const int k = (int)(e - 3 * f);
        const int a = p.faces[3 * f + k], b = p.faces[3 * f + (k == 2 ? 0 : k + 1)];
        p.slot[e] = -1;
        if (a < 0 || a >= nv || b < 0 || b >= nv) {
            atomicOr(p.err, (unsigned)CC_ERR_VERTEX);
            continue;
        }
        p.referenced[a] = 1;
        const unsigned long long key = ((unsigned long long)min(a, b) << 32) | (unsigned)max(a, b);
        unsigned long long s = cc_hash(key) & mask;
        int found = -1;
        for (unsigned long long probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
            const unsigned long long old = atomicCAS(p.keys + s, CC_EMPTY, key);
            if (old == CC_EMPTY || old == key) {
                found = (int)s;
                break;
            }
        }
        if (found < 0) atomicOr(p.err, (unsigned)CC_ERR_TABLE);
        p.slot[e] = found;
    }
}

__global__ __launch_bounds__(256) void cc_users_kernel(CCParams p) {
    const long long nf = p.nf();
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < 3 * nf; e += (long long)gridDim.x * 256) {
        const int s = p.slot[e];
        if (s < 0) continue;
        atomicAdd(p.users + s, 1u);
        atomicMin(p.first + s, (int)(e / 3));
    }
}

__global__ __launch_bounds__(256) void cc_union_kernel(CCParams p) {
    const long long nf = p.nf();
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < 3 * nf; e += (long long)gridDim.x * 256) {
        const int s = p.slot[e];
        if (s < 0 || p.users[s] != 2) continue;
        const int f = (int)(e / 3), g = p.first[s];
        if (g == f) continue;  // the smaller face of the pair (or a face using the edge twice: trimesh drops such self-pairs) does nothing
        p.has_nbr[f] = 1;
        p.has_nbr[g] = 1;
        int a = f, b = g, it = 0;
        for (; it < CC_CAS_CAP; ++it) {
            a = cc_find(p.parent, a);
            b = cc_find(p.parent, b);
            if (a == b) break;
            const int hi = max(a, b), lo = min(a, b);
            int expected = hi;
            if (__hip_atomic_compare_exchange_strong(p.parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        }
        if (it == CC_CAS_CAP) atomicOr(p.err, (unsigned)CC_ERR_UNION);
    }
}

// labels and per-root sizes of the faces with a neighbour: one atomic per distinct root in a wave
__global__ __launch_bounds__(256) void cc_label_kernel(CCParams p) {
    const long long nf = p.nf();
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256; base < nf; base += (long long)gridDim.x * 256) {
        const long long f = base + threadIdx.x;
        int root = -1;
        if (f < nf) {
            root = cc_find(p.parent, (int)f);
            p.label[f] = root;
            if (!p.has_nbr[f]) root = -1;
        }
        unsigned long long todo = __ballot(root >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader);
            const unsigned long long same = __ballot(root == r);
            if (lane == leader) atomicAdd(p.size + r, (unsigned)__popcll(same));
            todo &= ~same;
        }
    }
}

__global__ __launch_bounds__(256) void cc_select_kernel(CCParams p) {
    const long long nf = p.nf();
    unsigned long long best = 0;
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nf; f += (long long)gridDim.x * 256)
        if (p.label[f] == (int)f && p.passes(p.size[f])) best = max(best, ((unsigned long long)p.size[f] << 32) | (unsigned)~(unsigned)f);
    for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(p.best, best);
}

// frame_mesh_run: the pixels' vertex rows through a stage's vertex map (vid[i] = vmap[vid[i]], -1 = not written)
__global__ __launch_bounds__(256) void remap_vid_kernel(int *__restrict__ vid, int n, const int *__restrict__ vmap, const unsigned *__restrict__ n_verts, long long vert_cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = vid[i];
    vid[i] = v >= 0 && v < min((long long)*n_verts, vert_cap) ? vmap[v] : -1;
}

// scratch of a clean-up of at most face_cap faces over at most vert_cap vertices, taken from L
void cc_layout(hive_scratch_layout &L, long long face_cap, long long vert_cap, CCParams &p, unsigned **bv, unsigned **bf, int *nb) {
    long long table = 64;
    while (table < 4 * face_cap) table <<= 1;
    *nb = (int)std::max<long long>(1, (std::max(face_cap, vert_cap) + TILE - 1) / TILE);
    const size_t T = (size_t)table, F = (size_t)face_cap, V = (size_t)vert_cap;
    p.face_cap = face_cap;
    p.vert_cap = vert_cap;
    p.table_cap = table;
    p.keys = L.take<unsigned long long>(T);
    p.users = L.take<unsigned>(T);
    p.first = L.take<int>(T);
    p.slot = L.take<int>(3 * F);
    p.parent = L.take<int>(F);
    p.label = L.take<int>(F);
    p.size = L.take<unsigned>(F);
    p.has_nbr = L.take<uint8_t>(F);
    p.vmap = L.take<int>(V);
    p.referenced = L.take<uint8_t>(V);
    *bv = L.take<unsigned>((size_t)*nb);
    *bf = L.take<unsigned>((size_t)*nb);
}

// the clean-up's launches on faces already in device memory (counts in p.counts): scans into scalars[6] (vertices) / [7] (faces), box init at scalars + 8
void cc_launch(hive_ctx *ctx, const CCParams &p, unsigned *bv, unsigned *bf, int nb, unsigned *scalars, int32_t *out_faces, long long out_face_cap,
               int32_t *out_vertex_index) {
    const long long work = std::max<long long>(3 * p.face_cap, std::max<long long>(p.table_cap, p.vert_cap));
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, (long long)ctx->num_cus * 8)));
    hipLaunchKernelGGL(cc_init_kernel, grid, dim3(256), 0, ctx->stream, p);
    hipLaunchKernelGGL(cc_insert_kernel, grid, dim3(256), 0, ctx->stream, p);
    hipLaunchKernelGGL(cc_users_kernel, grid, dim3(256), 0, ctx->stream, p);
    hipLaunchKernelGGL(cc_union_kernel, grid, dim3(256), 0, ctx->stream, p);
    hipLaunchKernelGGL(cc_label_kernel, grid, dim3(256), 0, ctx->stream, p);
    if (p.is_object) hipLaunchKernelGGL(cc_select_kernel, grid, dim3(256), 0, ctx->stream, p);
    launch_compaction(ctx, p, bv, bf, nb, scalars + 6, (int *)(scalars + 8), out_faces, out_face_cap, out_vertex_index);
}

int cc_error(hive_ctx *ctx, unsigned err) {
    if (err & CC_ERR_VERTEX) return hive_fail(ctx, HIVE_ERR_INVALID, "mesh_cleanup_cc: a face references a vertex id outside [0, n_vertices)");
    if (err & CC_ERR_TABLE) return hive_fail(ctx, HIVE_ERR_STATE, "mesh_cleanup_cc: the edge table ran full");
    if (err & CC_ERR_UNION) return hive_fail(ctx, HIVE_ERR_STATE, "mesh_cleanup_cc: a union kept losing its compare-and-swap (%d tries)", CC_CAS_CAP);
    return HIVE_OK;
}

// ---- the frame path: one object of one frame from the mask to the texture window, behind hive_fg_frame_mesh / _cc / _dec -----------------------------
struct FrameMeshJob {
    const char *name;      // the entry point, for messages
    long long max_pixels;  // H W stays below it
    const float *depth;    // the inputs
    const uint8_t *mask;
    int H, W;
    const double *Kinv, *K, *R, *t;
    double max_px, max_depth;
    double *vertices;  // the caller's buffers and their capacities
    int64_t vertex_capacity;
    int32_t *faces;
    int64_t face_capacity;
    int32_t *uv;
    int64_t *n_vertices, *n_faces;  // the results
    int32_t *bbox;
    // the optional stages, in the order they run, and what only they report
    bool decimate = false;
    int64_t budget = 0;
    double max_error = 0.0;
    bool cleanup = false;
    int is_object = 0;
    double min_len = 0.0;
    int64_t *before = nullptr, *decimated = nullptr, *stats = nullptr;  // counts after the grid / after the decimation; the decimation's statistics
};

struct FrameMeshScratch {
    unsigned *bv, *bf;  // the grid's block counts
    int *vid;
    int32_t *grid_faces, *dec_faces;  // with a later stage: every pixel's faces fit
    double *pos;                      // the grid's vertices, for the decimation
    char *dec;
    CCParams cc;
    unsigned *cbv, *cbf;
    int cnb;
};

// device scratch: grid block counts x 2 | vid | the grid's faces | [the grid's vertices | the decimated faces | the decimation's state] | the clean-up's tables
size_t frame_mesh_layout(char *base, const FrameMeshJob &j, FrameMeshScratch &s) {
    const size_t n = (size_t)j.H * j.W, nb = (n + TILE - 1) / TILE, fcap = MAX_PIXEL_FACES * n;
    hive_scratch_layout L{base};
    s.bv = L.take<unsigned>(nb);
    s.bf = L.take<unsigned>(nb);
    s.vid = L.take<int>(n);
    if (!j.decimate && !j.cleanup) return L.bytes();  // the plain path: its faces go straight to the caller
    s.grid_faces = L.take<int32_t>(3 * fcap);
    if (j.decimate) {
        s.pos = L.take<double>(3 * n);
        s.dec_faces = L.take<int32_t>(3 * fcap);
        s.dec = L.take<char>(hive_decimate_scratch_bytes((long long)n, (long long)fcap));
    }
    cc_layout(L, (long long)fcap, (long long)n, s.cc, &s.cbv, &s.cbf, &s.cnb);  // (also reserved by a decimation without the clean-up)
    return L.bytes();
}

// Scalar block (hive_ctx::d_scalars + CC_SCALARS, the clean-up's): [0] / [1] vertices / faces of the grid, [2] the clean-up's error word, [4..5] its
// selection, [6] / [7] vertices / faces of the result, [8..11] the texture window's box, [12] / [13] vertices / faces after the decimation.
int frame_mesh_run(hive_ctx *ctx, const FrameMeshJob &j) {
    HIVE_REQUIRE(ctx, j.depth && j.Kinv && j.K && j.R && j.t && j.vertices && j.faces && j.uv && j.n_vertices && j.n_faces && j.bbox, "%s: NULL argument", j.name);
    HIVE_REQUIRE(ctx, j.H > 0 && j.W > 0 && (long long)j.H * j.W < j.max_pixels, "%s: bad image size %dx%d", j.name, j.H, j.W);
    HIVE_REQUIRE(ctx, j.vertex_capacity > 0 && j.face_capacity > 0, "%s: empty output buffers", j.name);
    HIVE_REQUIRE(ctx, !j.decimate || j.budget >= 0, "%s: budget %lld < 0", j.name, (long long)j.budget);
    const int n = j.H * j.W, nb = (n + TILE - 1) / TILE;
    const long long fcap = (long long)MAX_PIXEL_FACES * n;
    FrameMeshScratch s{};
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, frame_mesh_layout(nullptr, j, s));
    if (rc) return rc;
    frame_mesh_layout((char *)ctx->d_scratch, j, s);
    const bool staged = j.decimate || j.cleanup;
    unsigned *sc = ctx->d_scalars + CC_SCALARS, *final_counts = sc + 6;
    int *d_box = (int *)(sc + 8);
    // where the grid's faces go: the caller's buffer when no later stage follows, scratch otherwise
    int32_t *grid_faces = staged ? s.grid_faces : j.faces;
    const long long grid_face_cap = staged ? fcap : (long long)j.face_capacity;
    // which stage writes the final counts: the last one that runs; the earlier ones write the words their successor reads
    unsigned *grid_counts = staged ? sc : final_counts;
    unsigned *dec_counts = j.cleanup ? sc + 12 : final_counts;
    const GridParams gp{j.H, j.W, j.max_px, (float)j.max_depth};
    FrameMeshCam cam;
    memcpy(cam.Kinv, j.Kinv, sizeof(cam.Kinv));
    memcpy(cam.R, j.R, sizeof(cam.R));
    memcpy(cam.t, j.t, sizeof(cam.t));
    WindowParams wp;
    memcpy(wp.K, j.K, sizeof(wp.K));
    memcpy(wp.R, j.R, sizeof(wp.R));
    memcpy(wp.t, j.t, sizeof(wp.t));
    wp.scale = 1.0;
    const dim3 tiles(nb), pixels((n + 255) / 256), blk(256);
    hipStream_t st = ctx->stream;
    // 1. the triangulation + face filter of the valid pixels (hive_grid_mesh's kernels; the scan also empties the texture window's box)
    hipLaunchKernelGGL(grid_count_kernel, tiles, blk, 0, st, j.depth, j.mask, gp, s.bv, s.bf);
    scan_counts_box(ctx, s.bv, s.bf, nb, grid_counts, d_box);
    hipLaunchKernelGGL(grid_vid_kernel, tiles, blk, 0, st, j.depth, j.mask, n, (const unsigned *)s.bv, s.vid);
    hipLaunchKernelGGL(grid_faces_kernel, tiles, blk, 0, st, j.depth, j.mask, gp, (const unsigned *)s.bf, (const int *)s.vid, grid_faces, grid_face_cap);
    // 2. the decimation (hive_mesh_decimate) of the grid's mesh in scratch; without the clean-up its faces are the result
    if (j.decimate) {
        HIVE_CHECK_HIP(ctx, hipMemsetAsync(sc + 2, 0, sizeof(unsigned), st));
        hipLaunchKernelGGL(grid_vertices_kernel, pixels, blk, 0, st, j.depth, (const int *)s.vid, n, j.W, cam, s.pos, (long long)n);
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        hive_dec_job dj;
        dj.pos = s.pos;
        dj.faces = grid_faces;
        dj.counts = grid_counts;
        dj.vert_cap = n;
        dj.face_cap = fcap;
        dj.budget = j.budget;
        dj.max_error = j.max_error;
        dj.out_faces = j.cleanup ? s.dec_faces : j.faces;
        dj.out_face_cap = j.cleanup ? fcap : (long long)j.face_capacity;
        dj.out_counts = dec_counts;
        if ((rc = hive_decimate_run(ctx, dj, s.dec, j.stats))) return rc;
        hipLaunchKernelGGL(remap_vid_kernel, pixels, blk, 0, st, s.vid, n, (const int *)hive_decimate_vmap(s.dec, n, fcap), (const unsigned *)grid_counts, (long long)n);
    }
    // 3. the clean-up (hive_mesh_cleanup_cc) of the mesh so far: survivors into the caller's faces, remapped to the vertices they reference
    if (j.cleanup) {
        CCParams &p = s.cc;
        p.counts = j.decimate ? dec_counts : grid_counts;
        p.err = sc + 2;
        p.best = (unsigned long long *)(sc + 4);
        p.faces = j.decimate ? s.dec_faces : grid_faces;
        p.min_len = j.min_len;
        p.is_object = j.is_object ? 1 : 0;
        cc_launch(ctx, p, s.cbv, s.cbf, s.cnb, sc, j.faces, (long long)j.face_capacity, nullptr);
        hipLaunchKernelGGL(remap_vid_kernel, pixels, blk, 0, st, s.vid, n, (const int *)p.vmap, p.counts, (long long)n);
    }
    // 4. the vertices of the pixels that are left, 5. their texture window
    hipLaunchKernelGGL(grid_vertices_kernel, pixels, blk, 0, st, j.depth, (const int *)s.vid, n, j.W, cam, j.vertices, (long long)j.vertex_capacity);
    const dim3 wgrid((unsigned)std::min<long long>((std::min<long long>(n, j.vertex_capacity) + 255) / 256, (long long)ctx->num_cus * 4));
    hipLaunchKernelGGL(window_project_kernel, wgrid, blk, 0, st, (const double *)j.vertices, (const unsigned *)final_counts, (long long)j.vertex_capacity, wp, j.uv, d_box);
    hipLaunchKernelGGL(window_shift_kernel, wgrid, blk, 0, st, j.uv, (const unsigned *)final_counts, (long long)j.vertex_capacity, (const int *)d_box);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    // 6. ONE read-back through pinned memory, of the words in use: [6..11] on the plain path, [0..11] with the clean-up, [0..13] with the decimation
    const int first = staged ? 0 : 6, last = j.decimate ? 14 : 12;
    static_assert(CC_SCALARS_WORDS >= 14, "the frame mesh runner uses words [0..13] of the clean-up's block");
    unsigned *back;
    if ((rc = hive_pinned_small(ctx, (void **)&back))) return rc;
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back + first, sc + first, (size_t)(last - first) * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(st));
    // when the clean-up's error word is checked: whenever the clean-up ran, before any result is handed out
    if (j.cleanup && (rc = cc_error(ctx, back[2]))) return rc;
    const unsigned nv = back[6], nf = back[7];
    const int *box = (const int *)(back + 8);
    *j.n_vertices = nv;
    *j.n_faces = nf;
    j.bbox[0] = box[0];
    j.bbox[1] = box[1];
    j.bbox[2] = nv ? box[2] + 1 : box[2];
    j.bbox[3] = nv ? box[3] + 1 : box[3];
    if (staged && j.before) {
        j.before[0] = back[0];
        j.before[1] = back[1];
    }
    if (j.decimate && j.decimated) {
        j.decimated[0] = back[dec_counts - sc];
        j.decimated[1] = back[dec_counts - sc + 1];
    }
    HIVE_REQUIRE(ctx, (int64_t)nv <= j.vertex_capacity && (int64_t)nf <= j.face_capacity, "%s: %u vertices / %u faces do not fit the buffers (%lld / %lld)", j.name, nv, nf,
                 (long long)j.vertex_capacity, (long long)j.face_capacity);
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_grid_mesh(hive_ctx *ctx, const float *depth, const uint8_t *mask, int H, int W, double max_pixel_distance,
                   double max_depth_distance, int mem, int32_t *out_faces, int64_t capacity, int64_t *n_faces, int64_t *n_vertices) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, depth && n_faces, "grid_mesh: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 30), "grid_mesh: bad image size %dx%d", H, W);
    HIVE_REQUIRE(ctx, capacity >= 0 && (capacity == 0 || out_faces), "grid_mesh: bad output buffer");
    HIVE_REQUIRE(ctx, mem == HIVE_MEM_HOST || mem == HIVE_MEM_DEVICE, "grid_mesh: bad mem kind %d", mem);
    const int n = H * W, nb = (n + TILE - 1) / TILE;
    // device scratch: [depth | mask] (host inputs) | block counts x 2 | vid | faces (host outputs)
    float *s_depth;
    uint8_t *s_mask;
    unsigned *bv, *bf;
    int *vid;
    int32_t *s_faces = nullptr;
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        s_depth = L.take<float>((size_t)n);
        s_mask = L.take<uint8_t>((size_t)n);
        bv = L.take<unsigned>((size_t)nb);
        bf = L.take<unsigned>((size_t)nb);
        vid = L.take<int>((size_t)n);
        if (mem == HIVE_MEM_HOST) s_faces = L.take<int32_t>(3 * (size_t)capacity);
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    const float *d_depth = depth;
    const uint8_t *d_mask = mask;
    int32_t *d_faces = out_faces;
    if (mem == HIVE_MEM_HOST) {
        if ((rc = hive_upload(ctx, s_depth, depth, (size_t)n * 4))) return rc;
        d_depth = s_depth;
        if (mask) {
            if ((rc = hive_upload(ctx, s_mask, mask, (size_t)n))) return rc;
            d_mask = s_mask;
        }
        d_faces = s_faces;
    }
    unsigned *d_tot = ctx->d_scalars + SC_GRID_TOTALS;  // [0] = vertices, [1] = faces
    GridParams p{H, W, max_pixel_distance, (float)max_depth_distance};
    hipLaunchKernelGGL(grid_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_depth, d_mask, p, bv, bf);
    hive_scan_counts(ctx, nb, d_tot, bv, bf);
    hipLaunchKernelGGL(grid_vid_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_depth, d_mask, n, (const unsigned *)bv, vid);
    if (capacity > 0)
        hipLaunchKernelGGL(grid_faces_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_depth, d_mask, p, (const unsigned *)bf, (const int *)vid, d_faces,
                           (long long)capacity);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    unsigned tot[2] = {0, 0};
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_faces = tot[1];
    if (n_vertices) *n_vertices = tot[0];
    if (mem == HIVE_MEM_HOST && capacity > 0) {
        const size_t nf = (size_t)std::min<int64_t>(capacity, (int64_t)tot[1]);
        if (nf) HIVE_CHECK_HIP(ctx, hipMemcpy(out_faces, d_faces, nf * 12, hipMemcpyDeviceToHost));
    }
    return HIVE_OK;
}

int hive_fg_frame_mesh(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                       const double t[3], double max_pixel_distance, double max_depth_distance, double *d_vertices, int64_t vertex_capacity, int32_t *d_faces,
                       int64_t face_capacity, int32_t *d_uv, int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    FrameMeshJob j{"fg_frame_mesh", 1ll << 30, d_depth, d_mask, H, W, Kinv, K, R, t, max_pixel_distance, max_depth_distance,
                   d_vertices, vertex_capacity, d_faces, face_capacity, d_uv, n_vertices, n_faces, bbox};
    return frame_mesh_run(ctx, j);
}

int hive_mesh_cleanup_cc(hive_ctx *ctx, const int32_t *faces, int64_t n_faces, int64_t n_vertices, int is_object, double min_len, int mem, int32_t *out_faces,
                         int32_t *out_vertex_index, int64_t *n_faces_out, int64_t *n_vertices_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n_faces_out && n_vertices_out, "mesh_cleanup_cc: NULL argument");
    HIVE_REQUIRE(ctx, n_faces >= 0 && n_faces < (1ll << 29) && n_vertices >= 0 && n_vertices < (1ll << 30), "mesh_cleanup_cc: bad sizes (%lld faces, %lld vertices)",
                 (long long)n_faces, (long long)n_vertices);
    HIVE_REQUIRE(ctx, (n_faces == 0 || (faces && out_faces)) && (n_vertices == 0 || out_vertex_index), "mesh_cleanup_cc: NULL argument");
    HIVE_REQUIRE(ctx, mem == HIVE_MEM_HOST || mem == HIVE_MEM_DEVICE, "mesh_cleanup_cc: bad mem kind %d", mem);
    *n_faces_out = 0;
    *n_vertices_out = 0;
    if (n_vertices == 0) {  // no vertex: a face can only reference ids out of range
        HIVE_REQUIRE(ctx, n_faces == 0, "mesh_cleanup_cc: a face references a vertex id outside [0, n_vertices)");
        return HIVE_OK;
    }
    const long long fcap = std::max<long long>(n_faces, 1);
    // device scratch: [faces | out faces | out vertex ids] (host memory) | the clean-up's tables
    CCParams p{};
    unsigned *bv, *bf;
    int nb;
    int32_t *s_faces = nullptr, *s_out_faces = nullptr, *s_out_vi = nullptr;
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        if (mem == HIVE_MEM_HOST) {
            s_faces = L.take<int32_t>(3 * (size_t)fcap);
            s_out_faces = L.take<int32_t>(3 * (size_t)fcap);
            s_out_vi = L.take<int32_t>((size_t)n_vertices);
        }
        cc_layout(L, fcap, n_vertices, p, &bv, &bf, &nb);
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    const int32_t *d_faces = faces;
    int32_t *d_out_faces = out_faces, *d_out_vi = out_vertex_index;
    if (mem == HIVE_MEM_HOST) {
        if (n_faces && (rc = hive_upload(ctx, s_faces, faces, (size_t)n_faces * 12))) return rc;
        d_faces = s_faces;
        d_out_faces = s_out_faces;
        d_out_vi = s_out_vi;
    }
    unsigned *sc = ctx->d_scalars + CC_SCALARS;
    const unsigned counts[2] = {(unsigned)n_vertices, (unsigned)n_faces};
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(sc, counts, sizeof(counts), hipMemcpyHostToDevice, ctx->stream));
    p.counts = sc;
    p.err = sc + 2;
    p.best = (unsigned long long *)(sc + 4);
    p.faces = d_faces;
    p.min_len = min_len;
    p.is_object = is_object ? 1 : 0;
    cc_launch(ctx, p, bv, bf, nb, sc, d_out_faces, fcap, d_out_vi);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    unsigned back[8];
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back, sc, sizeof(back), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = cc_error(ctx, back[2]))) return rc;
    *n_vertices_out = back[6];
    *n_faces_out = back[7];
    if (mem == HIVE_MEM_HOST) {
        if (back[7]) HIVE_CHECK_HIP(ctx, hipMemcpy(out_faces, d_out_faces, (size_t)back[7] * 12, hipMemcpyDeviceToHost));
        if (back[6]) HIVE_CHECK_HIP(ctx, hipMemcpy(out_vertex_index, d_out_vi, (size_t)back[6] * 4, hipMemcpyDeviceToHost));
    }
    return HIVE_OK;
}

int hive_fg_frame_mesh_cc(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                          const double t[3], double max_pixel_distance, double max_depth_distance, int is_object, double min_len, double *d_vertices,
                          int64_t vertex_capacity, int32_t *d_faces, int64_t face_capacity, int32_t *d_uv, int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4], int64_t before[2]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    FrameMeshJob j{"fg_frame_mesh_cc", 1ll << 27, d_depth, d_mask, H, W, Kinv, K, R, t, max_pixel_distance, max_depth_distance,
                   d_vertices, vertex_capacity, d_faces, face_capacity, d_uv, n_vertices, n_faces, bbox};
    j.cleanup = true;
    j.is_object = is_object;
    j.min_len = min_len;
    j.before = before;
    return frame_mesh_run(ctx, j);
}

int hive_fg_frame_mesh_dec(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                           const double t[3], double max_pixel_distance, double max_depth_distance, int64_t budget, double max_error, int enable_cc,
                           int is_object, double min_len, double *d_vertices, int64_t vertex_capacity, int32_t *d_faces, int64_t face_capacity, int32_t *d_uv,
                           int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4], int64_t before[2], int64_t decimated[2], int64_t stats[3]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    FrameMeshJob j{"fg_frame_mesh_dec", 1ll << 27, d_depth, d_mask, H, W, Kinv, K, R, t, max_pixel_distance, max_depth_distance,
                   d_vertices, vertex_capacity, d_faces, face_capacity, d_uv, n_vertices, n_faces, bbox};
    j.decimate = true;
    j.budget = budget;
    j.max_error = max_error;
    j.cleanup = enable_cc != 0;
    j.is_object = is_object;
    j.min_len = min_len;
    j.before = before;
    j.decimated = decimated;
    j.stats = stats;
    return frame_mesh_run(ctx, j);
}

int hive_filter_faces(hive_ctx *ctx, const int32_t *points2d, const float *depth, int64_t n_points, const int32_t *faces, int64_t n_faces_in,
                      double max_pixel_distance, double max_depth_distance, int mem, int32_t *out_faces, int64_t *n_faces_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n_faces_out && n_points >= 0 && n_faces_in >= 0, "filter_faces: bad arguments");
    *n_faces_out = 0;
    if (n_faces_in == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, points2d && depth && faces && out_faces && n_points > 0, "filter_faces: NULL argument");
    HIVE_REQUIRE(ctx, mem == HIVE_MEM_HOST || mem == HIVE_MEM_DEVICE, "filter_faces: bad mem kind %d", mem);
    const int nb = (int)((n_faces_in + TILE - 1) / TILE);
    // device scratch: [points | depth | faces | out faces] (host memory) | block counts
    int32_t *s_points2d, *s_faces, *s_out;
    float *s_depth;
    unsigned *blk;
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        s_points2d = L.take<int32_t>(2 * (size_t)n_points);
        s_depth = L.take<float>((size_t)n_points);
        s_faces = L.take<int32_t>(3 * (size_t)n_faces_in);
        s_out = L.take<int32_t>(3 * (size_t)n_faces_in);
        blk = L.take<unsigned>((size_t)nb);
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    FilterParams p{points2d, depth, faces, (long long)n_faces_in, max_pixel_distance, (float)max_depth_distance};
    int32_t *d_out = out_faces;
    if (mem == HIVE_MEM_HOST) {
        if ((rc = hive_upload(ctx, s_points2d, points2d, (size_t)n_points * 8))) return rc;
        if ((rc = hive_upload(ctx, s_depth, depth, (size_t)n_points * 4))) return rc;
        if ((rc = hive_upload(ctx, s_faces, faces, (size_t)n_faces_in * 12))) return rc;
        p.points2d = s_points2d;
        p.depth = s_depth;
        p.faces = s_faces;
        d_out = s_out;
    }
    unsigned *d_tot = ctx->d_scalars + SC_FILTER_TOTAL;
    hipLaunchKernelGGL(filter_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, p, blk);
    hive_scan_counts(ctx, nb, d_tot, blk);
    hipLaunchKernelGGL(filter_write_kernel, dim3(nb), dim3(256), 0, ctx->stream, p, (const unsigned *)blk, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    unsigned tot = 0;
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_faces_out = tot;
    if (mem == HIVE_MEM_HOST && tot) HIVE_CHECK_HIP(ctx, hipMemcpy(out_faces, d_out, (size_t)tot * 12, hipMemcpyDeviceToHost));
    return HIVE_OK;
}

int hive_texture_window(hive_ctx *ctx, const double *points, int64_t n, const double K[9], const double R[9], const double t[3],
                        double scale_factor, int mem, int32_t *out_uv, int32_t bbox[4]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, points && K && R && t && out_uv && bbox && n > 0, "texture_window: bad arguments");
    HIVE_REQUIRE(ctx, scale_factor != 0.0, "texture_window: scale_factor must not be 0");
    int rc;
    const double *d_pts = points;
    int32_t *d_uv = out_uv;
    if (mem == HIVE_MEM_HOST) {
        const size_t off_uv = ((size_t)n * 24 + 255) & ~(size_t)255;
        if ((rc = hive_reserve_device(ctx, &ctx->d_in, &ctx->in_bytes, off_uv + (size_t)n * 8))) return rc;
        if ((rc = hive_upload(ctx, ctx->d_in, points, (size_t)n * 24))) return rc;
        d_pts = (const double *)ctx->d_in;
        d_uv = (int32_t *)((char *)ctx->d_in + off_uv);
    }
    int *d_box = (int *)(ctx->d_scalars + SC_WINDOW_BOX);
    const int32_t init[4] = {0x7fffffff, 0x7fffffff, (int32_t)0x80000000, (int32_t)0x80000000};
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_box, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    WindowParams p;
    memcpy(p.K, K, sizeof(p.K));
    memcpy(p.R, R, sizeof(p.R));
    memcpy(p.t, t, sizeof(p.t));
    p.scale = scale_factor;
    const dim3 grid((unsigned)std::min<long long>((n + 255) / 256, (long long)ctx->num_cus * 4));
    hipLaunchKernelGGL(window_project_kernel, grid, dim3(256), 0, ctx->stream, d_pts, (const unsigned *)nullptr, (long long)n, p, d_uv, d_box);
    hipLaunchKernelGGL(window_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_uv, (const unsigned *)nullptr, (long long)n, (const int *)d_box);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    int32_t box[4];
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // min_u, min_v, max_u + 1, max_v + 1: `texture = image[min_v:max_v, min_u:max_u]` (pipeline.py:802-805)
    bbox[0] = box[0];
    bbox[1] = box[1];
    bbox[2] = box[2] + 1;
    bbox[3] = box[3] + 1;
    if (mem == HIVE_MEM_HOST) HIVE_CHECK_HIP(ctx, hipMemcpy(out_uv, d_uv, (size_t)n * 8, hipMemcpyDeviceToHost));
    return HIVE_OK;
}

}  // extern "C"
