// Mesh decimation of the foreground objects: Pipeline._decimate_mesh (/root/reference/hive/pipeline.py:697-738 -- OpenMesh's ModQuadric in binary mode
// + decimate_to_faces) as a parallel quadric-error halfedge collapse, for gfx950.  The rules are restated in include/hive_mi355x.h (hive_mesh_decimate)
// and DESIGN.md §5.8; tests/decimate_restatement.py restates the same rounds in numpy, and the kernels match it bit for bit (-ffp-contract=off).
//
// State of a call: the working faces fw (a dead face has fw[3 f] = -1), one float64 quadric of 10 terms per vertex, the vertex flags (locked, removed), and
// per round the incidence of the faces alive: one linked list of face corners per vertex (head / next, built with atomicExch; every use of it is
// order-independent, so the lists' order does not matter).  One round, ten launches:
//   key       every unlocked vertex v0 with >= 2 faces: its best legal collapse v0 -> v1 (smallest float32 cost, then smallest v1), judged on the mesh at the
//             start of the round; key = the cost's band (top 5 bits of its order-preserving float32 bits: 16 octaves) << 32 | mix32(v0) (a bijection
//             of v0: keys are unique, and collapses of one band are not ordered by the vertex numbering or by small cost differences, either of which
//             leaves few local minima and a handful of collapses per round), ~0 = none
//   fmin/vmin twice: m2[v] = the smallest key within two edges of v (vertex -> face -> vertex, two passes)
//   select    v0 is applied iff key(v0) == m2[v0] == m2[v1]: no two applied collapses share a face, nor read what another one writes
//   thresh    one workgroup: stop when nothing is selected; otherwise, when the selected collapses would remove at least F - budget faces, keep the
//             cheapest prefix by key that reaches F <= budget (a bit-by-bit search of the threshold key over the selected set)
//   apply     faces: v0 -> v1, degenerate faces die; vertices: Q(v1) += Q(v0), v0 removed, lists reset; build: the new lists
// Integer atomics only (list heads, appends and counts whose final values do not depend on order): results are identical from run to run.
#include "mesh_compact.hpp"

namespace {

constexpr int DEC_MAX_ROUNDS = 4096;
constexpr int DEC_BATCH = 16;  // rounds issued between two polls of the device state
constexpr unsigned long long KEY_NONE = ~0ull;
constexpr uint8_t F_LOCKED = 1, F_REMOVED = 2;
constexpr unsigned ERR_VERTEX = 1, ERR_DEGENERATE = 2, ERR_ROUNDS = 4;
// scalar block (hive_ctx::d_scalars + DEC_SCALARS): [0] faces now, [1] done, [2] error word, [3] selected, [4] faces the selected remove, [5] rounds,
// [6] collapses, [7] locked vertices, [8..9] threshold key (u64), [12..15] a scratch box for the output scan, [DEC_ENTRY ..] hive_mesh_decimate's own
// counts.  DEC_SCALARS and its extent: the map in hive_internal.hpp
constexpr int DEC_ENTRY = 16;
static_assert(DEC_ENTRY + 4 <= DEC_SCALARS_WORDS, "hive_mesh_decimate keeps V, F in and vertices / faces out in four words behind the runner's sixteen");
constexpr float DEC_FLT_MIN = 1.17549435e-38f;
// a vertex's key keeps the top 5 bits of the mapped float32 cost (bands of 16 octaves): with all 32, a smooth cost field has few local minima and a
// round applies ~2 collapses (426 rounds for a 2.5 k-face object against 200 with bands; tests/decimate_restatement.py)
constexpr int KEY_BAND_SHIFT = 27;

struct DecParams {
    const unsigned *counts;
    long long vert_cap, face_cap;
    const double *pos;
    const int32_t *faces_in;
    long long budget;
    double max_error;
    int32_t *fw;               // [F][3]
    double *Q;                 // [V][10]
    int *head;                 // [V]
    int *next;                 // [3 F]
    uint8_t *flags;            // [V]
    uint8_t *sel;              // [V]
    uint8_t *rem;              // [V] faces the best collapse removes
    int *tgt;                  // [V]
    unsigned long long *key;   // [V]
    unsigned long long *m1;    // [V]
    unsigned long long *m2;    // [V]
    unsigned long long *fk;    // [F]
    int *list;                 // [V] selected vertices
    int *vmap;                 // [V]
    unsigned *sc;
    // the output compaction (mesh_compact.hpp): the vertices not removed, isolated ones included, and the faces alive
    __device__ long long nv() const { return min((long long)counts[0], vert_cap); }
    __device__ long long nf() const { return min((long long)counts[1], face_cap); }
    __device__ bool keep_vertex(long long i) const { return !(flags[i] & F_REMOVED); }
    __device__ bool keep_face(long long f) const { return fw[3 * f] >= 0; }
    __device__ int face_vertex(long long f, int k) const { return vmap[fw[3 * f + k]]; }
};

// the round kernels run while nothing has stopped the decimation and the face count is above the budget
__device__ __forceinline__ bool dec_active(const DecParams &p) {
    const volatile unsigned *sc = p.sc;
    return !sc[1] && !sc[2] && (long long)sc[0] > p.budget;
}
__device__ __forceinline__ bool dec_applying(const DecParams &p) {
    const volatile unsigned *sc = p.sc;
    return !sc[1] && !sc[2];
}

__device__ __forceinline__ unsigned cost_bits(double cost) {
    const unsigned b = __float_as_uint((float)cost);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the plane quadric of face (i0, i1, i2), OpenMesh ModQuadricT::initialize's arithmetic in float64 (tests/decimate_restatement.py face_quadrics)
__device__ void face_quadric(const double *pos, int i0, int i1, int i2, double q[10]) {
    const double p0x = pos[3 * i0], p0y = pos[3 * i0 + 1], p0z = pos[3 * i0 + 2];
    const double ax = pos[3 * i1] - p0x, ay = pos[3 * i1 + 1] - p0y, az = pos[3 * i1 + 2] - p0z;
    const double bx = pos[3 * i2] - p0x, by = pos[3 * i2 + 1] - p0y, bz = pos[3 * i2 + 2] - p0z;
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    double area = sqrt(nx * nx + ny * ny + nz * nz);
    if (area > (double)DEC_FLT_MIN) {
        nx = nx / area;
        ny = ny / area;
        nz = nz / area;
        area = area * 0.5;
    }
    const double d = -(p0x * nx + p0y * ny + p0z * nz);
    q[0] = nx * nx * area;
    q[1] = nx * ny * area;
    q[2] = nx * nz * area;
    q[3] = nx * d * area;
    q[4] = ny * ny * area;
    q[5] = ny * nz * area;
    q[6] = ny * d * area;
    q[7] = nz * nz * area;
    q[8] = nz * d * area;
    q[9] = d * d * area;
}

// OpenMesh QuadricT::evaluate, left to right
__device__ __forceinline__ double qeval(const double q[10], double x, double y, double z) {
    return q[0] * x * x + 2.0 * q[1] * x * y + 2.0 * q[2] * x * z + 2.0 * q[3] * x + q[4] * y * y + 2.0 * q[5] * y * z + 2.0 * q[6] * y + q[7] * z * z +
           2.0 * q[8] * z + q[9];
}

// ---- incidence queries on the lists of the current round ----
__device__ __forceinline__ bool ecount_face(const DecParams &p, int f, int w) { return p.fw[3 * f] == w || p.fw[3 * f + 1] == w || p.fw[3 * f + 2] == w; }
// faces of v that contain w
__device__ int ecount(const DecParams &p, int v, int w) {
    int n = 0;
    for (int c = p.head[v]; c >= 0; c = p.next[c]) {
        const int f = c / 3;
        n += p.fw[3 * f] == w || p.fw[3 * f + 1] == w || p.fw[3 * f + 2] == w;
    }
    return n;
}
__device__ int nfaces(const DecParams &p, int v) {
    int n = 0;
    for (int c = p.head[v]; c >= 0; c = p.next[c]) ++n;
    return n;
}
// the other two corners of the face of corner c
__device__ __forceinline__ void others(const DecParams &p, int c, int &a, int &b) {
    const int f = c / 3, k = c - 3 * f;
    a = p.fw[3 * f + (k == 2 ? 0 : k + 1)];
    b = p.fw[3 * f + (k == 0 ? 2 : k - 1)];
}
// distinct neighbours of v
__device__ int valence(const DecParams &p, int v) {
    int n = 0;
    for (int c = p.head[v]; c >= 0; c = p.next[c]) {
        int ab[2];
        others(p, c, ab[0], ab[1]);
        for (int j = 0; j < 2; ++j) {
            bool seen = j == 1 && ab[0] == ab[1];
            for (int e = p.head[v]; e != c && !seen; e = p.next[e]) {
                const int f = e / 3;
                seen = p.fw[3 * f] == ab[j] || p.fw[3 * f + 1] == ab[j] || p.fw[3 * f + 2] == ab[j];
            }
            n += !seen;
        }
    }
    return n;
}

// the neighbour occurrences of a vertex (two per face, in list order) held by the thread: the legality checks of its candidates read them instead of
// walking the lists again.  A vertex with more than MAX_FACES faces takes part in no collapse (faces(v0) + faces(v1) - removed > MAX_FACES), so
// every ring the checks need fits.
constexpr int MAX_FACES = 24;
constexpr int RING = 2 * MAX_FACES;
struct Ring {
    int n;
    int w[RING];
};
__device__ bool gather(const DecParams &p, int v, Ring &r) {
    r.n = 0;
    for (int c = p.head[v]; c >= 0; c = p.next[c]) {
        if (r.n + 2 > RING) return false;
        others(p, c, r.w[r.n], r.w[r.n + 1]);
        r.n += 2;
    }
    return true;
}
__device__ __forceinline__ int rcount(const Ring &r, int w) {
    int n = 0;
    for (int i = 0; i < r.n; ++i) n += r.w[i] == w;
    return n;
}
__device__ bool rboundary(const Ring &r) {
    for (int i = 0; i < r.n; ++i)
        if (rcount(r, r.w[i]) == 1) return true;
    return false;
}
// legality of v0 -> v1 on their gathered rings (tests/decimate_restatement.py collapse_cost); *removes = faces the collapse removes
__device__ bool collapse_ok(const DecParams &p, int v1, const Ring &r0, const Ring &r1, bool b0, int *removes) {
    if (p.flags[v1] & F_LOCKED) return false;
    int opp[2], cnt = 0;
    for (int i = 0; i < r0.n; i += 2) {
        const int a = r0.w[i], b = r0.w[i + 1];
        if (a == v1 || b == v1) {
            if (cnt == 2) return false;
            opp[cnt++] = a == v1 ? b : a;
        }
    }
    if (cnt == 2 && opp[0] == opp[1]) return false;
    if (r0.n / 2 + r1.n / 2 - cnt > MAX_FACES) return false;
    const bool b1 = rboundary(r1);
    if (b0 && !(cnt == 1 && b1)) return false;
    if (cnt == 2 && b0 && b1) return false;
    for (int i = 0; i < r0.n; ++i) {
        const int w = r0.w[i];
        if (w == v1 || w == opp[0] || (cnt == 2 && w == opp[1])) continue;
        if (rcount(r1, w) > 0) return false;
    }
    for (int j = 0; j < cnt; ++j)
        if (rcount(r0, opp[j]) == 1 && rcount(r1, opp[j]) == 1) return false;
    if (cnt == 2 && ecount(p, opp[0], opp[1]) > 0 && valence(p, opp[0]) == 3 && valence(p, opp[1]) == 3) return false;
    *removes = cnt;
    return true;
}

__global__ __launch_bounds__(256) void dec_init_kernel(DecParams p) {
    const long long nv = p.nv(), nf = p.nf();
    // the scalar block is cleared on the stream before this launch: the error word below is only ever OR-ed into, never reset by a thread of this launch
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.sc[0] = (unsigned)nf;
        p.sc[1] = nf <= p.budget;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < max(nv, nf); i += (long long)gridDim.x * 256) {
        if (i < nv) {
            p.head[i] = -1;
            p.flags[i] = 0;
            p.sel[i] = 0;
        }
        if (i < nf) {
            const int a = p.faces_in[3 * i], b = p.faces_in[3 * i + 1], c = p.faces_in[3 * i + 2];
            p.fw[3 * i] = a;
            p.fw[3 * i + 1] = b;
            p.fw[3 * i + 2] = c;
            if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) atomicOr(p.sc + 2, ERR_VERTEX);
            else if (a == b || b == c || a == c) atomicOr(p.sc + 2, ERR_DEGENERATE);
        }
    }
}

__global__ __launch_bounds__(256) void dec_build_kernel(DecParams p) {
    if (!dec_active(p)) return;
    const long long nf = p.nf(), nv = p.nv();
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nf; f += (long long)gridDim.x * 256) {
        if (p.fw[3 * f] < 0) continue;
        for (int k = 0; k < 3; ++k) {
            const int c = (int)(3 * f + k), v = p.fw[c];
            if (v >= 0 && v < nv) p.next[c] = atomicExch(p.head + v, c);  // (validated by dec_init_kernel; a bad face has stopped the call)
        }
    }
}

// the vertex quadrics (faces in ascending index) and the locked vertices, once
__global__ __launch_bounds__(256) void dec_quadric_kernel(DecParams p) {
    if (!dec_active(p)) return;
    const long long nv = p.nv();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const int v = (int)i;
        double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int prev = -1;;) {
            int f = 0x7fffffff;
            for (int c = p.head[v]; c >= 0; c = p.next[c])
                if (c / 3 > prev) f = min(f, c / 3);
            if (f == 0x7fffffff) break;
            double fq[10];
            face_quadric(p.pos, p.fw[3 * f], p.fw[3 * f + 1], p.fw[3 * f + 2], fq);
            for (int j = 0; j < 10; ++j) q[j] = q[j] + fq[j];
            prev = f;
        }
        for (int j = 0; j < 10; ++j) p.Q[10 * i + j] = q[j];
        // locked: boundary edges neither 0 nor 2, or an edge with more than two faces (each boundary edge is seen once, as a neighbour of count 1)
        int nb = 0;
        bool multi = false;
        for (int c = p.head[v]; c >= 0; c = p.next[c]) {
            int ab[2];
            others(p, c, ab[0], ab[1]);
            for (int j = 0; j < 2; ++j) {
                const int n = ecount(p, v, ab[j]);
                nb += n == 1;
                multi |= n > 2;
            }
        }
        if (p.head[v] >= 0 && (multi || (nb != 0 && nb != 2))) {
            p.flags[v] = F_LOCKED;
            atomicAdd(p.sc + 7, 1u);
        }
    }
}

__global__ __launch_bounds__(256) void dec_key_kernel(DecParams p) {
    if (!dec_active(p)) return;
    const long long nv = p.nv();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const int v0 = (int)i;
        unsigned long long best = KEY_NONE;
        int best_v1 = -1, best_rem = 0;
        Ring r0, r1;
        if (!p.flags[v0] && nfaces(p, v0) >= 2 && gather(p, v0, r0)) {
            const bool b0 = rboundary(r0);
            double q0[10];
            for (int j = 0; j < 10; ++j) q0[j] = p.Q[10 * i + j];
            for (int c = p.head[v0]; c >= 0; c = p.next[c]) {
                int ab[2];
                others(p, c, ab[0], ab[1]);
                for (int j = 0; j < 2; ++j) {
                    const int v1 = ab[j];
                    bool seen = false;  // each neighbour once: its other occurrences give the same answer
                    for (int e = p.head[v0]; e != c && !seen; e = p.next[e]) seen = ecount_face(p, e / 3, v1);
                    if (seen) continue;
                    int removes = 0;
                    if ((p.flags[v1] & F_LOCKED) || !gather(p, v1, r1) || !collapse_ok(p, v1, r0, r1, b0, &removes)) continue;
                    double q[10];
                    for (int k = 0; k < 10; ++k) q[k] = q0[k] + p.Q[10 * (long long)v1 + k];
                    const double cost = qeval(q, p.pos[3 * (long long)v1], p.pos[3 * (long long)v1 + 1], p.pos[3 * (long long)v1 + 2]);
                    if (!(cost < p.max_error)) continue;
                    const unsigned long long cand = ((unsigned long long)cost_bits(cost) << 32) | (unsigned)v1;
                    if (cand < best) {
                        best = cand;
                        best_v1 = v1;
                        best_rem = removes;
                    }
                }
            }
        }
        p.key[i] = best == KEY_NONE ? KEY_NONE : ((best >> (32 + KEY_BAND_SHIFT)) << 32) | mix32((unsigned)v0);
        p.tgt[i] = best_v1;
        p.rem[i] = (uint8_t)best_rem;
    }
}

// fk[f] = smallest src over the corners of live face f
__global__ __launch_bounds__(256) void dec_fmin_kernel(DecParams p, const unsigned long long *__restrict__ src) {
    if (!dec_active(p)) return;
    const long long nf = p.nf();
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nf; f += (long long)gridDim.x * 256) {
        if (p.fw[3 * f] < 0) continue;
        p.fk[f] = min(src[p.fw[3 * f]], min(src[p.fw[3 * f + 1]], src[p.fw[3 * f + 2]]));
    }
}

// dst[v] = min(src[v], fk over the faces of v)
__global__ __launch_bounds__(256) void dec_vmin_kernel(DecParams p, const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst) {
    if (!dec_active(p)) return;
    const long long nv = p.nv();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        unsigned long long m = src[i];
        for (int c = p.head[i]; c >= 0; c = p.next[c]) m = min(m, p.fk[c / 3]);
        dst[i] = m;
    }
}

__global__ __launch_bounds__(256) void dec_select_kernel(DecParams p) {
    if (!dec_active(p)) return;
    const long long nv = p.nv();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const unsigned long long k = p.key[i];
        const bool s = k != KEY_NONE && k == p.m2[i] && k == p.m2[p.tgt[i]];
        p.sel[i] = s;
        if (s) {
            p.list[atomicAdd(p.sc + 3, 1u)] = (int)i;
            atomicAdd(p.sc + 4, (unsigned)p.rem[i]);
        }
    }
}

// one workgroup of 1024: the end of the decimation, or the threshold key of the collapses this round applies
__global__ __launch_bounds__(1024) void dec_thresh_kernel(DecParams p) {
    __shared__ unsigned long long part[16];
    __shared__ int stop;
    unsigned *sc = p.sc;
    if (!dec_applying(p)) return;
    const unsigned n_sel = sc[3], total = sc[4];
    const long long f_now = sc[0];
    if (threadIdx.x == 0) {
        stop = 0;
        if (f_now <= p.budget || n_sel == 0) {
            sc[1] = 1;
            stop = 1;
        } else if (sc[5] == (unsigned)DEC_MAX_ROUNDS) {
            atomicOr(sc + 2, ERR_ROUNDS);
            sc[1] = 1;
            stop = 1;
        }
    }
    __syncthreads();
    if (stop) return;
    const long long need = f_now - p.budget;
    unsigned long long thr = KEY_NONE;
    if ((long long)total >= need) {
        // the largest x whose prefix (keys <= x) removes fewer than `need` faces, bit by bit; the threshold is x + 1 (a selected key)
        unsigned long long x = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const unsigned long long t = x | (1ull << bit);
            unsigned long long s = 0;
            for (unsigned j = threadIdx.x; j < n_sel; j += 1024) {
                const int v = p.list[j];
                if (p.key[v] <= t) s += p.rem[v];
            }
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
            __syncthreads();
            unsigned long long sum = 0;
            for (int w = 0; w < 16; ++w) sum += part[w];
            __syncthreads();
            if ((long long)sum < need) x = t;
        }
        thr = x + 1;
    }
    unsigned applied = 0;
    for (unsigned j = threadIdx.x; j < n_sel; j += 1024) applied += p.key[p.list[j]] <= thr;
    for (int off = 32; off > 0; off >>= 1) applied += (unsigned)__shfl_xor((int)applied, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = applied;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
        for (int w = 0; w < 16; ++w) sum += (unsigned)part[w];
        *(unsigned long long *)(sc + 8) = thr;
        sc[3] = 0;
        sc[4] = 0;
        sc[5] += 1;
        sc[6] += sum;
    }
}

__device__ __forceinline__ bool applied(const DecParams &p, int v, unsigned long long thr) { return p.sel[v] && p.key[v] <= thr; }

__global__ __launch_bounds__(256) void dec_apply_faces_kernel(DecParams p) {
    if (!dec_applying(p)) return;
    const unsigned long long thr = *(const unsigned long long *)(p.sc + 8);
    const long long nf = p.nf();
    unsigned killed = 0;
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nf; f += (long long)gridDim.x * 256) {
        if (p.fw[3 * f] < 0) continue;
        int c[3];
        bool moved = false;
        for (int k = 0; k < 3; ++k) {
            c[k] = p.fw[3 * f + k];
            if (applied(p, c[k], thr)) {
                c[k] = p.tgt[c[k]];
                moved = true;
            }
        }
        if (!moved) continue;
        if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) {
            p.fw[3 * f] = -1;
            ++killed;
        } else {
            for (int k = 0; k < 3; ++k) p.fw[3 * f + k] = c[k];
        }
    }
    for (int off = 32; off > 0; off >>= 1) killed += (unsigned)__shfl_xor((int)killed, off);
    if ((threadIdx.x & 63) == 0 && killed) atomicSub(p.sc, killed);
}

__global__ __launch_bounds__(256) void dec_apply_vertices_kernel(DecParams p) {
    if (!dec_applying(p)) return;
    const unsigned long long thr = *(const unsigned long long *)(p.sc + 8);
    const long long nv = p.nv();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        p.head[i] = -1;
        if (applied(p, (int)i, thr)) {
            const long long t = p.tgt[i];
            for (int j = 0; j < 10; ++j) p.Q[10 * t + j] = p.Q[10 * t + j] + p.Q[10 * i + j];
            p.flags[i] |= F_REMOVED;
        }
        p.sel[i] = 0;
    }
}

struct DecLayout {
    size_t bytes;
    int nb;
    unsigned *bv, *bf;
};

DecLayout dec_layout(hive_scratch_layout L, long long vert_cap, long long face_cap, DecParams &p) {
    DecLayout l{};
    l.nb = (int)std::max<long long>(1, (std::max(face_cap, vert_cap) + TILE - 1) / TILE);
    const size_t V = (size_t)vert_cap, F = (size_t)face_cap;
    p.vert_cap = vert_cap;
    p.face_cap = face_cap;
    p.vmap = L.take<int>(V);  // first: hive_decimate_vmap
    p.fw = L.take<int32_t>(3 * F);
    p.Q = L.take<double>(10 * V);
    p.head = L.take<int>(V);
    p.next = L.take<int>(3 * F);
    p.flags = L.take<uint8_t>(V);
    p.sel = L.take<uint8_t>(V);
    p.rem = L.take<uint8_t>(V);
    p.tgt = L.take<int>(V);
    p.key = L.take<unsigned long long>(V);
    p.m1 = L.take<unsigned long long>(V);
    p.m2 = L.take<unsigned long long>(V);
    p.fk = L.take<unsigned long long>(F);
    p.list = L.take<int>(V);
    l.bv = L.take<unsigned>((size_t)l.nb);
    l.bf = L.take<unsigned>((size_t)l.nb);
    l.bytes = L.bytes();
    return l;
}

int dec_error(hive_ctx *ctx, unsigned err) {
    if (err & ERR_VERTEX) return hive_fail(ctx, HIVE_ERR_INVALID, "mesh_decimate: a face references a vertex id outside [0, n_vertices)");
    if (err & ERR_DEGENERATE) return hive_fail(ctx, HIVE_ERR_INVALID, "mesh_decimate: a face repeats a vertex");
    if (err & ERR_ROUNDS) return hive_fail(ctx, HIVE_ERR_STATE, "mesh_decimate: %d rounds and legal collapses remain", DEC_MAX_ROUNDS);
    return HIVE_OK;
}

}  // namespace

size_t hive_decimate_scratch_bytes(long long vert_cap, long long face_cap) {
    DecParams p{};
    return dec_layout({}, std::max<long long>(vert_cap, 1), std::max<long long>(face_cap, 1), p).bytes;
}

int32_t *hive_decimate_vmap(void *scratch, long long, long long) { return (int32_t *)scratch; }

int hive_decimate_run(hive_ctx *ctx, const hive_dec_job &job, void *scratch, int64_t stats[3]) {
    DecParams p{};
    const DecLayout l = dec_layout({(char *)scratch}, std::max<long long>(job.vert_cap, 1), std::max<long long>(job.face_cap, 1), p);
    p.counts = job.counts;
    p.pos = job.pos;
    p.faces_in = job.faces;
    p.budget = job.budget;
    p.max_error = job.max_error;
    p.sc = ctx->d_scalars + DEC_SCALARS;
    const long long work = std::max(p.vert_cap, p.face_cap);
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, (long long)ctx->num_cus * 8))), blk(256);
    hipStream_t s = ctx->stream;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(p.sc, 0, 12 * sizeof(unsigned), s));  // [0..11]: counters, error word, threshold
    hipLaunchKernelGGL(dec_init_kernel, grid, blk, 0, s, p);
    hipLaunchKernelGGL(dec_build_kernel, grid, blk, 0, s, p);
    hipLaunchKernelGGL(dec_quadric_kernel, grid, blk, 0, s, p);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    void *pinned;
    int rc = hive_pinned_small(ctx, &pinned);
    if (rc) return rc;
    volatile unsigned *back = (volatile unsigned *)pinned;
    // rounds in batches; between batches one small read-back says whether to go on (no kernel waits on the device for progress)
    for (int issued = 0;;) {
        for (int r = 0; r < DEC_BATCH; ++r, ++issued) {
            hipLaunchKernelGGL(dec_key_kernel, grid, blk, 0, s, p);
            hipLaunchKernelGGL(dec_fmin_kernel, grid, blk, 0, s, p, (const unsigned long long *)p.key);
            hipLaunchKernelGGL(dec_vmin_kernel, grid, blk, 0, s, p, (const unsigned long long *)p.key, p.m1);
            hipLaunchKernelGGL(dec_fmin_kernel, grid, blk, 0, s, p, (const unsigned long long *)p.m1);
            hipLaunchKernelGGL(dec_vmin_kernel, grid, blk, 0, s, p, (const unsigned long long *)p.m1, p.m2);
            hipLaunchKernelGGL(dec_select_kernel, grid, blk, 0, s, p);
            hipLaunchKernelGGL(dec_thresh_kernel, dim3(1), dim3(1024), 0, s, p);
            hipLaunchKernelGGL(dec_apply_faces_kernel, grid, blk, 0, s, p);
            hipLaunchKernelGGL(dec_apply_vertices_kernel, grid, blk, 0, s, p);
            hipLaunchKernelGGL(dec_build_kernel, grid, blk, 0, s, p);
        }
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(pinned, p.sc, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
        if (back[1] || back[2] || (long long)back[0] <= job.budget) break;
        if (issued > DEC_MAX_ROUNDS + DEC_BATCH) return hive_fail(ctx, HIVE_ERR_STATE, "mesh_decimate: the round loop did not end");
    }
    const unsigned err = back[2];
    if (stats) {
        stats[0] = back[5];
        stats[1] = back[6];
        stats[2] = back[7];
    }
    if ((rc = dec_error(ctx, err))) return rc;
    launch_compaction(ctx, p, l.bv, l.bf, l.nb, job.out_counts, (int *)(p.sc + 12), job.out_faces, job.out_face_cap, job.out_vertex_index);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

extern "C" {

int hive_mesh_decimate(hive_ctx *ctx, const double *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int64_t budget, double max_error, int mem,
                       int32_t *out_faces, int32_t *out_vertex_index, int64_t *n_faces_out, int64_t *n_vertices_out, int64_t stats[3]) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n_faces_out && n_vertices_out, "mesh_decimate: NULL argument");
    HIVE_REQUIRE(ctx, n_faces >= 0 && n_faces < (1ll << 29) && n_vertices >= 0 && n_vertices < (1ll << 30), "mesh_decimate: bad sizes (%lld faces, %lld vertices)",
                 (long long)n_faces, (long long)n_vertices);
    HIVE_REQUIRE(ctx, budget >= 0, "mesh_decimate: budget %lld < 0", (long long)budget);
    HIVE_REQUIRE(ctx, (n_faces == 0 || (faces && out_faces)) && (n_vertices == 0 || (vertices && out_vertex_index)), "mesh_decimate: NULL argument");
    HIVE_REQUIRE(ctx, mem == HIVE_MEM_HOST || mem == HIVE_MEM_DEVICE, "mesh_decimate: bad mem kind %d", mem);
    *n_faces_out = 0;
    *n_vertices_out = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (n_vertices == 0) {
        HIVE_REQUIRE(ctx, n_faces == 0, "mesh_decimate: a face references a vertex id outside [0, n_vertices)");
        return HIVE_OK;
    }
    const long long fcap = std::max<long long>(n_faces, 1);
    // device scratch: [vertices | faces | out faces | out vertex ids] (host memory) | the decimation's state
    double *s_pos = nullptr;
    int32_t *s_faces = nullptr, *s_out_faces = nullptr, *s_out_vi = nullptr;
    char *s_dec;
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        if (mem == HIVE_MEM_HOST) {
            s_pos = L.take<double>(3 * (size_t)n_vertices);
            s_faces = L.take<int32_t>(3 * (size_t)fcap);
            s_out_faces = L.take<int32_t>(3 * (size_t)fcap);
            s_out_vi = L.take<int32_t>((size_t)n_vertices);
        }
        s_dec = L.take<char>(hive_decimate_scratch_bytes(n_vertices, fcap));
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    hive_dec_job job;
    job.pos = vertices;
    job.faces = faces;
    job.out_faces = out_faces;
    job.out_vertex_index = out_vertex_index;
    if (mem == HIVE_MEM_HOST) {
        if ((rc = hive_upload(ctx, s_pos, vertices, (size_t)n_vertices * 24))) return rc;
        if (n_faces && (rc = hive_upload(ctx, s_faces, faces, (size_t)n_faces * 12))) return rc;
        job.pos = s_pos;
        job.faces = s_faces;
        job.out_faces = s_out_faces;
        job.out_vertex_index = s_out_vi;
    }
    unsigned *sc = ctx->d_scalars + DEC_SCALARS + DEC_ENTRY;  // [0] = V, [1] = F in, [2] / [3] = vertices / faces out
    const unsigned counts[2] = {(unsigned)n_vertices, (unsigned)n_faces};
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(sc, counts, sizeof(counts), hipMemcpyHostToDevice, ctx->stream));
    job.counts = sc;
    job.vert_cap = n_vertices;
    job.face_cap = fcap;
    job.budget = budget;
    job.max_error = max_error;
    job.out_face_cap = fcap;
    job.out_counts = sc + 2;
    if ((rc = hive_decimate_run(ctx, job, s_dec, stats))) return rc;
    unsigned out[2];
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(out, sc + 2, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_vertices_out = out[0];
    *n_faces_out = out[1];
    if (mem == HIVE_MEM_HOST) {
        if (out[1]) HIVE_CHECK_HIP(ctx, hipMemcpy(out_faces, job.out_faces, (size_t)out[1] * 12, hipMemcpyDeviceToHost));
        if (out[0]) HIVE_CHECK_HIP(ctx, hipMemcpy(out_vertex_index, job.out_vertex_index, (size_t)out[0] * 4, hipMemcpyDeviceToHost));
    }
    return HIVE_OK;
}

}  // extern "C"
