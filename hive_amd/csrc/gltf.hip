// glTF 2.0 export: the meshes of a scene packed on the device into the binary buffer of a .glb, in the file's final byte layout.  gfx950 only.
//
//   hive_gltf_layout -> offset and length of every buffer view of every mesh (host only)
//   hive_gltf_pack   -> the bytes of those views in d_out and the float64 bounds of every mesh, THREE launches for any number of meshes
//
// The rules (what is stored, how it is rounded, what fails) are stated in include/hive_mi355x.h and restated in numpy in tests/gltf_restatement.py.  Float64
// arithmetic, compiled without contraction, every result independent of the launch geometry: min and max do not depend on order (and no floating-point atomic is
// used anyway), everything else is element-wise.  The same bytes on every run, alone or inside a batch.
//
// One upload carries the whole descriptor table: the segments (one per buffer view: source, destination, the elements before it), the meshes of the bounds pass
// (the chunks before each), the colour table and the two error words.
//   bounds        one workgroup per CHUNK of 1024 vertices of one mesh (found in the chunk prefix by hive_internal.hpp's last_not_after): a thread takes vertices chunk * 1024 + j * 256
//                 + thread, j = 0 .. 3, the 64 lanes combine in a butterfly, the four waves through LDS -> partial[chunk] = {min xyz, max xyz}.  A vertex that is
//                 not finite lowers error word 0 to its mesh (integer atomic minimum).
//   bounds, final one workgroup per MESH over its chunks' partials (thread k takes chunks k, k + 256, ..) -> bounds[mesh] = {lo xyz, hi xyz, s xyz}, s the
//                 quantisation step (hi - lo) / 65535.0, 1.0 on a flat axis.
//   pack          one thread per output ELEMENT (a vertex of POSITION / TEXCOORD_0 / COLOR_0, a face of the indices) over the concatenated element ranges of all
//                 segments, its segment found in the element prefix the same way.  An index outside [0, V) lowers error word 1 to its mesh.
// The kernels are memory-bound: a vertex is read once per attribute and written once; stores are plain 16- and 32-bit C++ stores (views are 4-byte aligned,
// uint16 indices 2-byte aligned).
#include "hive_internal.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_CHUNK_PER_THREAD = 4;
constexpr int GL_CHUNK = GL_THREADS * GL_CHUNK_PER_THREAD;  // vertices per workgroup of the bounds pass
constexpr unsigned GL_NO_MESH = 0xFFFFFFFFu;

struct GltfSeg {         // one buffer view of one mesh
    const void *src;     // vertices / uv / colours / faces
    uint8_t *dst;        // d_out + the view's offset
    long long first;     // elements of the segments before this one
    long long count;     // V, or F for the indices
    long long V;
    int mesh, kind;      // kind: HIVE_GLTF_POSITION ..
    int wide;            // float64 vertices / int64 faces
    int channels;        // of the colours
    int idx16;           // indices stored as uint16
    int pad;
};
static_assert(sizeof(GltfSeg) == 64, "GltfSeg is uploaded as a table of 64-byte rows");

struct GltfBoundsMesh {  // one mesh of the bounds pass
    const void *vertices;
    long long V;
    long long first_chunk;  // chunks of the meshes before this one
    int wide, pad;
};
static_assert(sizeof(GltfBoundsMesh) == 32, "GltfBoundsMesh is uploaded as a table of 32-byte rows");

__device__ __forceinline__ double load_coord(const void *vertices, int wide, long long at) {
    return wide ? ((const double *)vertices)[at] : (double)((const float *)vertices)[at];
}

// min over m[0..2], max over m[3..5]: butterfly over the 64 lanes, then the four waves in order; valid in thread 0
__device__ __forceinline__ void bounds_block_reduce(double m[6], double (*lds)[6]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 6; ++k) {
            const double o = __shfl_xor(m[k], off);
            m[k] = k < 3 ? fmin(m[k], o) : fmax(m[k], o);
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; ++k) lds[threadIdx.x >> 6][k] = m[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < GL_THREADS / 64; ++w)
            for (int k = 0; k < 6; ++k) m[k] = k < 3 ? fmin(m[k], lds[w][k]) : fmax(m[k], lds[w][k]);
}

// grid (chunks of all meshes): partial[chunk] = {min x, y, z, max x, y, z} of the chunk's vertices
__global__ __launch_bounds__(GL_THREADS) void gltf_bounds_kernel(const GltfBoundsMesh *__restrict__ meshes, int n_meshes, double *__restrict__ partial,
                                                                 unsigned *__restrict__ flags) {
    __shared__ double lds[GL_THREADS / 64][6];
    const long long chunk = blockIdx.x;
    const int lo = last_not_after(n_meshes, chunk, [meshes](int i) { return meshes[i].first_chunk; });  // the mesh that holds this chunk
    const GltfBoundsMesh mesh = meshes[lo];
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int j = 0; j < GL_CHUNK_PER_THREAD; ++j) {
        const long long v = (chunk - mesh.first_chunk) * GL_CHUNK + j * GL_THREADS + threadIdx.x;
        if (v < mesh.V)
            for (int k = 0; k < 3; ++k) {
                const double x = load_coord(mesh.vertices, mesh.wide, 3 * v + k);
                bad |= !(fabs(x) <= DBL_MAX);
                m[k] = fmin(m[k], x);
                m[3 + k] = fmax(m[3 + k], x);
            }
    }
    if (bad) atomicMin(&flags[0], (unsigned)lo);
    bounds_block_reduce(m, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) partial[chunk * 6 + k] = m[k];
}

// grid (meshes): bounds[mesh] = {lo x, y, z, hi x, y, z, s x, y, z}
__global__ __launch_bounds__(GL_THREADS) void gltf_bounds_final_kernel(const GltfBoundsMesh *__restrict__ meshes, const double *__restrict__ partial,
                                                                       double *__restrict__ bounds) {
    __shared__ double lds[GL_THREADS / 64][6];
    const GltfBoundsMesh mesh = meshes[blockIdx.x];
    const long long chunks = (mesh.V + GL_CHUNK - 1) / GL_CHUNK;
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (long long c = threadIdx.x; c < chunks; c += GL_THREADS)
        for (int k = 0; k < 6; ++k) {
            const double o = partial[(mesh.first_chunk + c) * 6 + k];
            m[k] = k < 3 ? fmin(m[k], o) : fmax(m[k], o);
        }
    bounds_block_reduce(m, lds);
    if (threadIdx.x == 0) {
        double *out = bounds + (size_t)blockIdx.x * 9;
        for (int k = 0; k < 3; ++k) {
            out[k] = m[k];
            out[3 + k] = m[3 + k];
            out[6 + k] = m[3 + k] == m[k] ? 1.0 : (m[3 + k] - m[k]) / 65535.0;
        }
    }
}

__device__ __forceinline__ unsigned quantise_unit(double c) { return (unsigned)rint(fmin(fmax(c, 0.0), 1.0) * 65535.0); }

// grid (elements of all segments / 256)
__global__ __launch_bounds__(GL_THREADS) void gltf_pack_kernel(const GltfSeg *__restrict__ segs, int n_segs, long long total, int quantize,
                                                               const uint8_t *__restrict__ lut, const double *__restrict__ bounds, unsigned *__restrict__ flags) {
    const long long e = (long long)blockIdx.x * GL_THREADS + threadIdx.x;
    if (e >= total) return;
    const GltfSeg s = segs[last_not_after(n_segs, e, [segs](int i) { return segs[i].first; })];  // the segment that holds this element
    const long long i = e - s.first;
    if (s.kind == HIVE_GLTF_POSITION) {
        if (!quantize) {
            float *out = (float *)s.dst + 3 * i;
            if (s.wide) {
                const double *in = (const double *)s.src + 3 * i;
                for (int k = 0; k < 3; ++k) out[k] = (float)in[k];  // round to nearest even
            } else {
                const float *in = (const float *)s.src + 3 * i;
                for (int k = 0; k < 3; ++k) out[k] = in[k];
            }
        } else {
            const double *b = bounds + (size_t)s.mesh * 9;
            unsigned q[3];
            for (int k = 0; k < 3; ++k) q[k] = (unsigned)fmin(65535.0, rint((load_coord(s.src, s.wide, 3 * i + k) - b[k]) / b[6 + k]));
            unsigned *out = (unsigned *)s.dst + 2 * i;  // x | y << 16, z | 0 << 16: an 8-byte stride
            out[0] = q[0] | q[1] << 16;
            out[1] = q[2];
        }
    } else if (s.kind == HIVE_GLTF_TEXCOORD) {
        const double *in = (const double *)s.src + 2 * i;
        const double u = in[0], v = 1.0 - in[1];  // the atlas has its origin bottom-left, glTF top-left
        if (!quantize) {
            float *out = (float *)s.dst + 2 * i;
            out[0] = (float)u;
            out[1] = (float)v;
        } else {
            ((unsigned *)s.dst)[i] = quantise_unit(u) | quantise_unit(v) << 16;
        }
    } else if (s.kind == HIVE_GLTF_COLOR) {
        const uint8_t *in = (const uint8_t *)s.src + (size_t)s.channels * i;
        unsigned c[4] = {in[0], in[1], in[2], s.channels == 4 ? (unsigned)in[3] : 255u};
        if (lut)
            for (int k = 0; k < 3; ++k) c[k] = lut[c[k]];
        ((unsigned *)s.dst)[i] = c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24;
    } else {
        long long f[3];
        for (int k = 0; k < 3; ++k) f[k] = s.wide ? (long long)((const int64_t *)s.src)[3 * i + k] : (long long)((const int32_t *)s.src)[3 * i + k];
        if (f[0] < 0 || f[0] >= s.V || f[1] < 0 || f[1] >= s.V || f[2] < 0 || f[2] >= s.V) atomicMin(&flags[1], (unsigned)s.mesh);
        if (s.idx16) {
            unsigned short *out = (unsigned short *)s.dst + 3 * i;
            for (int k = 0; k < 3; ++k) out[k] = (unsigned short)f[k];
            if (i == s.count - 1 && (s.count & 1)) out[3] = 0;  // 3 F uint16 with F odd: the two bytes up to the 4-byte boundary
        } else {
            unsigned *out = (unsigned *)s.dst + 3 * i;
            for (int k = 0; k < 3; ++k) out[k] = (unsigned)f[k];
        }
    }
}

constexpr long long GL_MAX_VERTICES = (1ll << 31) - 1, GL_MAX_FACES = (1ll << 31) - 1;
constexpr int GL_MAX_MESHES = 1 << 20;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool index16(const hive_gltf_mesh &m, int quantize) { return quantize && m.n_vertices <= 65535; }

// validates the descriptors and fills views[n][4] (NULL: validate only)
int gltf_layout(hive_ctx *ctx, const hive_gltf_mesh *meshes, int n, int quantize, hive_gltf_view *views, int64_t *total_bytes) {
    HIVE_REQUIRE(ctx, meshes && n >= 1 && n <= GL_MAX_MESHES, "gltf: %d meshes (1 .. %d, and a descriptor table)", n, GL_MAX_MESHES);
    HIVE_REQUIRE(ctx, quantize == 0 || quantize == 1, "gltf: quantize must be 0 or 1, got %d", quantize);
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const hive_gltf_mesh &m = meshes[i];
        HIVE_REQUIRE(ctx, m.n_vertices >= 1 && m.n_vertices <= GL_MAX_VERTICES, "gltf: mesh %d has %lld vertices (1 .. 2^31 - 1)", i, (long long)m.n_vertices);
        HIVE_REQUIRE(ctx, m.n_faces != 0, "gltf: mesh %d has n_faces == 0 (leave the node out)", i);
        HIVE_REQUIRE(ctx, m.n_faces >= 1 && m.n_faces <= GL_MAX_FACES, "gltf: mesh %d has %lld faces (1 .. 2^31 - 1)", i, (long long)m.n_faces);
        HIVE_REQUIRE(ctx, m.vertex_dtype == HIVE_GLTF_F32 || m.vertex_dtype == HIVE_GLTF_F64, "gltf: mesh %d: vertex dtype %d (0 float32, 1 float64)", i, m.vertex_dtype);
        HIVE_REQUIRE(ctx, m.face_dtype == HIVE_GLTF_I32 || m.face_dtype == HIVE_GLTF_I64, "gltf: mesh %d: face dtype %d (0 int32, 1 int64)", i, m.face_dtype);
        HIVE_REQUIRE(ctx, !m.colors || m.color_channels == 3 || m.color_channels == 4, "gltf: mesh %d: %d colour channels (3 or 4)", i, m.color_channels);
        const int64_t V = m.n_vertices, F = m.n_faces;
        const int64_t bytes[4] = {V * (quantize ? 8 : 12), m.uv ? V * (quantize ? 4 : 8) : 0, m.colors ? V * 4 : 0, F * 3 * (index16(m, quantize) ? 2 : 4)};
        for (int k = 0; k < 4; ++k) {
            hive_gltf_view view = {0, 0};
            if (bytes[k]) {
                at = (at + 3) & ~(int64_t)3;
                view.offset = at;
                view.length = bytes[k];
                at += bytes[k];
            }
            if (views) views[(size_t)i * 4 + k] = view;
        }
    }
    if (total_bytes) *total_bytes = (at + 3) & ~(int64_t)3;
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_gltf_layout(const hive_gltf_mesh *meshes, int n, int quantize, hive_gltf_view *views, int64_t *total_bytes) {
    if (!views || !total_bytes) return hive_fail(nullptr, HIVE_ERR_INVALID, "gltf_layout: NULL argument");
    return gltf_layout(nullptr, meshes, n, quantize, views, total_bytes);
}

int hive_gltf_pack(hive_ctx *ctx, const hive_gltf_mesh *meshes, int n, int quantize, const uint8_t *lut, uint8_t *d_out, int64_t out_bytes, double *bounds) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_out && bounds, "gltf_pack: NULL argument");
    HIVE_REQUIRE(ctx, ((uintptr_t)d_out & 3) == 0, "gltf_pack: d_out must be 4-byte aligned");
    std::vector<hive_gltf_view> views((size_t)std::max(n, 0) * 4);
    int64_t total_bytes = 0;
    int rc;
    if ((rc = gltf_layout(ctx, meshes, n, quantize, views.data(), &total_bytes))) return rc;
    std::vector<GltfSeg> segs;
    std::vector<GltfBoundsMesh> bmeshes((size_t)n);
    long long elements = 0, chunks = 0;
    for (int i = 0; i < n; ++i) {
        const hive_gltf_mesh &m = meshes[i];
        HIVE_REQUIRE(ctx, m.vertices && m.faces, "gltf_pack: mesh %d: NULL vertices or faces", i);
        int64_t end = 0;
        for (int k = 0; k < 4; ++k) end = std::max(end, views[(size_t)i * 4 + k].offset + views[(size_t)i * 4 + k].length);
        HIVE_REQUIRE(ctx, ((end + 3) & ~(int64_t)3) <= out_bytes, "gltf_pack: out_bytes = %lld is too small for mesh %d, whose views end at byte %lld (%lld in all)",
                     (long long)out_bytes, i, (long long)((end + 3) & ~(int64_t)3), (long long)total_bytes);
        const void *src[4] = {m.vertices, m.uv, m.colors, m.faces};
        for (int k = 0; k < 4; ++k) {
            const hive_gltf_view &view = views[(size_t)i * 4 + k];
            if (!view.length) continue;
            GltfSeg s;
            s.src = src[k];
            s.dst = d_out + view.offset;
            s.first = elements;
            s.count = k == HIVE_GLTF_INDICES ? m.n_faces : m.n_vertices;
            s.V = m.n_vertices;
            s.mesh = i;
            s.kind = k;
            s.wide = k == HIVE_GLTF_INDICES ? m.face_dtype == HIVE_GLTF_I64 : m.vertex_dtype == HIVE_GLTF_F64;
            s.channels = m.color_channels;
            s.idx16 = index16(m, quantize);
            s.pad = 0;
            elements += s.count;
            segs.push_back(s);
        }
        bmeshes[(size_t)i] = {m.vertices, (long long)m.n_vertices, chunks, m.vertex_dtype == HIVE_GLTF_F64, 0};
        chunks += (m.n_vertices + GL_CHUNK - 1) / GL_CHUNK;
    }
    const long long blocks = (elements + GL_THREADS - 1) / GL_THREADS;
    HIVE_REQUIRE(ctx, blocks < (1ll << 31) && chunks < (1ll << 31), "gltf_pack: %lld elements in one call (fewer than 2^39)", elements);
    // one block of scratch: segments | meshes | colour table | error words  (one upload)  | partial bounds | bounds
    const size_t o_segs = 0, o_meshes = o_segs + align256(segs.size() * sizeof(GltfSeg)), o_lut = o_meshes + align256(bmeshes.size() * sizeof(GltfBoundsMesh));
    const size_t o_flags = o_lut + 256, o_partial = o_flags + 256, o_bounds = o_partial + align256((size_t)chunks * 48);
    const size_t bytes = o_bounds + align256((size_t)n * 72);
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, bytes))) return rc;
    char *base = (char *)ctx->d_scratch;
    std::vector<uint8_t> table(o_partial, 0);
    memcpy(table.data() + o_segs, segs.data(), segs.size() * sizeof(GltfSeg));
    memcpy(table.data() + o_meshes, bmeshes.data(), bmeshes.size() * sizeof(GltfBoundsMesh));
    if (lut) memcpy(table.data() + o_lut, lut, 256);
    const unsigned no_mesh[2] = {GL_NO_MESH, GL_NO_MESH};
    memcpy(table.data() + o_flags, no_mesh, sizeof(no_mesh));
    if ((rc = hive_upload(ctx, base, table.data(), table.size()))) return rc;
    const GltfBoundsMesh *d_meshes = (const GltfBoundsMesh *)(base + o_meshes);
    unsigned *d_flags = (unsigned *)(base + o_flags);
    double *d_partial = (double *)(base + o_partial), *d_bounds = (double *)(base + o_bounds);
    hipLaunchKernelGGL(gltf_bounds_kernel, dim3((unsigned)chunks), dim3(GL_THREADS), 0, ctx->stream, d_meshes, n, d_partial, d_flags);
    hipLaunchKernelGGL(gltf_bounds_final_kernel, dim3((unsigned)n), dim3(GL_THREADS), 0, ctx->stream, d_meshes, (const double *)d_partial, d_bounds);
    hipLaunchKernelGGL(gltf_pack_kernel, dim3((unsigned)blocks), dim3(GL_THREADS), 0, ctx->stream, (const GltfSeg *)(base + o_segs), (int)segs.size(), elements, quantize,
                       lut ? (const uint8_t *)(base + o_lut) : nullptr, (const double *)d_bounds, d_flags);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    std::vector<double> back((size_t)n * 9);
    unsigned flags[2] = {GL_NO_MESH, GL_NO_MESH};
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back.data(), d_bounds, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    HIVE_REQUIRE(ctx, flags[0] == GL_NO_MESH, "gltf_pack: mesh %u has a vertex that is not finite", flags[0]);
    HIVE_REQUIRE(ctx, flags[1] == GL_NO_MESH, "gltf_pack: mesh %u has a face index outside [0, %lld)", flags[1],
                 (long long)(flags[1] < (unsigned)n ? meshes[flags[1]].n_vertices : 0));
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) bounds[(size_t)i * 6 + k] = back[(size_t)i * 9 + k];
    return HIVE_OK;
}

}  // extern "C"
