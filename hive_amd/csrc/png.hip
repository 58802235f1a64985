// PNG encoder: a batch of gray (8 or 16 bit) and RGB pictures of different sizes -> one PNG file each, packed into the caller's device buffer.  gfx950 only.
//
//   hive_png_layout -> the all-stored byte bound and offset of every picture (host only)
//   hive_png_encode -> the files in d_out and their sizes, FOURTEEN launches for any number of pictures
//
// The rules (the filter choice, the deflate parse and the code builder) are stated in include/hive_mi355x.h above hive_png_encode and restated in numpy in
// tests/png_restatement.py.  Integer arithmetic only; the atomics are integer adds, ORs of disjoint bits, XORs and maxima in LDS, so the bytes do not depend
// on the launch geometry, the run, the batch or the position in it.
//
// One upload carries the picture table and the powers x^(2^k) of the CRC polynomial.  "Stream" is the filtered bytes of all pictures back to back (a filter
// byte in front of every row); a "position" is an index into it; a "segment" is PG_SEGMENT bytes of ONE picture's stream (the last one shorter).
//   filter         one wave per row: the five filters' sums of |signed byte| (against the raw row above), the choice, the filtered row.
//   sort x 3       a stable radix sort of the positions by their next three bytes, a byte per pass: tile histograms (LDS integer adds), one workgroup per
//                  digit scans its tiles, and the scatter ranks a tile with thread d walking the tile for digit d -- no rank depends on timing.
//   previous       neighbours in the sorted order with equal bytes: the nearest earlier position with the same three bytes.
//   segment        one workgroup per segment: a thread per position measures the three candidates (one pixel left, one row up, the sorted neighbour); one
//                  lane walks the greedy parse; histograms (LDS integer adds); the three code builders (rank sort by all threads, the two-queue merge by one
//                  lane, depths by all); the block's bits against the stored block; the bits ORed into an LDS image at scanned offsets; the segment's bytes,
//                  its CRC remainder and its Adler sums to scratch.
//   picture        one workgroup per picture: exclusive scan of the segment sizes, the Adler-32 and the IDAT CRC combined from the segments' parts by
//                  their distance to the end, and every byte of the file outside the segments.
//   place          one workgroup per segment: its bytes behind the segments before it.
// The kernels move bytes and small integers; none is compute-bound.  The scans and the search are hive_internal.hpp's: block_scan_chunks (sort scan,
// picture), block_exclusive_total (the segment's token loop: a chunk's bits are carried in a register) and last_not_after (the picture of a row or a
// segment); the host frame -- the one upload, the sizes' read-back, the checks of the sides and of out_bytes -- is shared with jpeg.hip through the same header.
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_SEGMENT = 8192;                 // bytes of filtered stream per deflate block
constexpr int PG_SLOT = PG_SEGMENT + 8;          // scratch bytes per coded segment (at most PG_SEGMENT + 5 are used)
constexpr int PG_OUT_WORDS = PG_SLOT / 4 + 2;    // LDS image of a dynamic block
constexpr int PG_WINDOW = 32768, PG_MAX_MATCH = 258, PG_MIN_MATCH = 3, PG_FAR = 4096;
constexpr int PG_TILE = 2048;                    // positions per workgroup of a sort pass
constexpr int PG_LIT = 286, PG_DIST = 30, PG_CL = 19;
constexpr int PG_FIXED = 8 + 25 + 12 + 2 + 4 + 12;  // signature, IHDR, the IDAT frame, the zlib header, the Adler-32, IEND
constexpr int PG_DATA_AT = 8 + 25 + 8 + 2;       // where the first segment goes in the file
constexpr long long PG_MAX_STREAM = 1ll << 27;   // positions per call
constexpr int PG_MAX_PICTURES = 1 << 16;
constexpr unsigned PG_POLY = 0xEDB88320u;
constexpr unsigned PG_NONE = 0xFFFFFFFFu;
constexpr unsigned PG_TOKEN = 1u << 31;          // match word: length (9 bits) | distance - 1 (15 bits) << 9 | PG_TOKEN where the parse stops

struct PngPic {
    const uint8_t *src;
    long long pitch;
    long long out_off;     // of the file in d_out
    long long stream_off;  // of the picture's first position in the stream
    int H, W;
    int kind;
    int rowbytes;
    int stream_len;        // H * (rowbytes + 1)
    int first_seg, nseg;
    int first_row;         // rows of the pictures before this one
};
static_assert(sizeof(PngPic) == 64, "PngPic is uploaded as a table of 64-byte rows");

struct PngTables {
    unsigned x2n[32];  // x^(2^k) mod the CRC polynomial, reflected
};

__constant__ unsigned short PG_LENGTH_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char PG_LENGTH_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short PG_DIST_BASE[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                                193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char PG_DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ unsigned char PG_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// the picture that holds row / segment `at` of the call
__device__ __forceinline__ int pg_picture_of_row(const PngPic *__restrict__ pics, int n, int at) {
    return last_not_after(n, at, [pics](int i) { return pics[i].first_row; });
}
__device__ __forceinline__ int pg_picture_of_segment(const PngPic *__restrict__ pics, int n, int at) {
    return last_not_after(n, at, [pics](int i) { return pics[i].first_seg; });
}

// byte x of row y as PNG orders the samples (16-bit samples most significant byte first; the pictures hold them in host order, the least significant first)
__device__ __forceinline__ int pg_raw(const PngPic &P, int y, int x) { return P.src[(size_t)y * P.pitch + (P.kind == HIVE_PNG_GRAY16 ? x ^ 1 : x)]; }

__device__ __forceinline__ int pg_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int pg_filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : pg_paeth(a, b, c);
    return (x - pred) & 255;
}

// grid (rows of all pictures / 4): one wave per row -> the row's filter byte and filtered bytes in the stream
__global__ __launch_bounds__(PG_THREADS) void png_filter_kernel(const PngPic *__restrict__ pics, int n_pics, int total_rows, uint8_t *__restrict__ stream) {
    const int row = blockIdx.x * (PG_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= total_rows) return;  // the whole wave
    const PngPic P = pics[pg_picture_of_row(pics, n_pics, row)];
    const int y = row - P.first_row, bpp = P.kind == HIVE_PNG_GRAY8 ? 1 : P.kind == HIVE_PNG_GRAY16 ? 2 : 3;
    unsigned sum[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < P.rowbytes; x += 64) {
        const int v = pg_raw(P, y, x), a = x >= bpp ? pg_raw(P, y, x - bpp) : 0, b = y ? pg_raw(P, y - 1, x) : 0, c = (y && x >= bpp) ? pg_raw(P, y - 1, x - bpp) : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int f = pg_filtered(t, v, a, b, c);
            sum[t] += (unsigned)(f < 128 ? f : 256 - f);
        }
    }
    int type = 0;
    unsigned best = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        unsigned s = sum[t];
        for (int off = 32; off > 0; off >>= 1) s += (unsigned)__shfl_xor((int)s, off);
        if (t == 0 || s < best) {  // ties keep the lower type
            best = s;
            type = t;
        }
    }
    uint8_t *dst = stream + P.stream_off + (long long)y * (P.rowbytes + 1);
    if (lane == 0) dst[0] = (uint8_t)type;
    for (int x = lane; x < P.rowbytes; x += 64) {
        const int v = pg_raw(P, y, x), a = x >= bpp ? pg_raw(P, y, x - bpp) : 0, b = y ? pg_raw(P, y - 1, x) : 0, c = (y && x >= bpp) ? pg_raw(P, y - 1, x - bpp) : 0;
        dst[1 + x] = (uint8_t)pg_filtered(type, v, a, b, c);
    }
}

// ---- the sort: positions by (byte at +0, +1, +2), equal keys in position order -------------------------------------------------------------------------------
// the digit of pass `pass` (the LAST pass sorts by the first byte) of the position at index i of the pass's input; zero past the stream's end
__device__ __forceinline__ unsigned pg_position(const unsigned *__restrict__ in, unsigned i) { return in ? in[i] : i; }
__device__ __forceinline__ unsigned pg_digit(const uint8_t *__restrict__ stream, unsigned n, unsigned pos, int pass) {
    const unsigned at = pos + (unsigned)(2 - pass);
    return at < n ? stream[at] : 0u;
}

// grid (tiles): hist[digit * tiles + tile]
__global__ __launch_bounds__(PG_THREADS) void png_sort_count_kernel(const uint8_t *__restrict__ stream, unsigned n, const unsigned *__restrict__ in, int pass,
                                                                    unsigned *__restrict__ hist) {
    __shared__ unsigned count[256];
    count[threadIdx.x] = 0;
    __syncthreads();
    const unsigned first = blockIdx.x * (unsigned)PG_TILE;
    for (unsigned k = threadIdx.x; k < (unsigned)PG_TILE; k += PG_THREADS)
        if (first + k < n) atomicAdd(&count[pg_digit(stream, n, pg_position(in, first + k), pass)], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = count[threadIdx.x];
}

// grid (256 digits): the digit's tile counts -> exclusive offsets in place, and its total
__global__ __launch_bounds__(PG_THREADS) void png_sort_scan_kernel(unsigned *__restrict__ hist, unsigned tiles, unsigned *__restrict__ totals) {
    __shared__ unsigned lds[PG_THREADS / 64];
    unsigned *row = hist + (size_t)blockIdx.x * tiles;
    const unsigned total = block_scan_chunks(tiles, lds, [&](unsigned i) { return row[i]; }, [&](unsigned i, unsigned at) { row[i] = at; });
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// grid (tiles): every position of the tile to its place in `out`.  Thread d walks the tile's digits in order and numbers those equal to d.
__global__ __launch_bounds__(PG_THREADS) void png_sort_scatter_kernel(const uint8_t *__restrict__ stream, unsigned n, const unsigned *__restrict__ in, int pass,
                                                                      const unsigned *__restrict__ hist, const unsigned *__restrict__ totals,
                                                                      unsigned *__restrict__ out) {
    __shared__ unsigned lds[PG_THREADS / 64];
    __shared__ unsigned base[256];
    __shared__ unsigned position[PG_TILE];
    __shared__ unsigned short rank[PG_TILE];
    __shared__ __align__(4) unsigned char digit[PG_TILE];
    const unsigned first = blockIdx.x * (unsigned)PG_TILE, count = min((unsigned)PG_TILE, n - first), d = threadIdx.x;
    for (unsigned k = threadIdx.x; k < (unsigned)PG_TILE; k += PG_THREADS) {
        const unsigned pos = k < count ? pg_position(in, first + k) : 0u;
        position[k] = pos;
        digit[k] = (unsigned char)(k < count ? pg_digit(stream, n, pos, pass) : 0u);
    }
    const unsigned before = block_exclusive(totals[d], lds);  // positions of smaller digits; its barriers also publish the tile
    base[d] = before + hist[(size_t)d * gridDim.x + blockIdx.x];
    unsigned seen = 0;
    const unsigned *words = (const unsigned *)digit;
    for (unsigned w = 0; w < (count + 3u) / 4u; ++w) {
        const unsigned four = words[w];
#pragma unroll
        for (unsigned j = 0; j < 4; ++j)
            if (4 * w + j < count && ((four >> (8 * j)) & 255u) == d) rank[4 * w + j] = (unsigned short)seen++;
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < count; k += PG_THREADS) {
        const unsigned at = base[digit[k]] + rank[k];
        if (at < n) out[at] = position[k];  // always: a permutation of 0 .. n - 1
    }
}

// a thread per sorted index: previous[p] = the position sorted just before p if its three bytes equal p's, else PG_NONE
__global__ __launch_bounds__(PG_THREADS) void png_previous_kernel(const uint8_t *__restrict__ stream, unsigned n, const unsigned *__restrict__ order,
                                                                  unsigned *__restrict__ previous) {
    const unsigned i = blockIdx.x * (unsigned)PG_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned p = order[i];
    if (p >= n) return;
    unsigned q = PG_NONE;
    if (i > 0 && p + 2 < n) {
        const unsigned c = order[i - 1];
        if (c < p && stream[c] == stream[p] && stream[c + 1] == stream[p + 1] && stream[c + 2] == stream[p + 2]) q = c;
    }
    previous[p] = q;
}

// ---- a segment ---------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pg_length_symbol(int length) {
    int s = 28;
    while (PG_LENGTH_BASE[s] > length) --s;
    return s;
}
__device__ __forceinline__ int pg_dist_symbol(int distance) {
    int s = 29;
    while (PG_DIST_BASE[s] > distance) --s;
    return s;
}

// the reflected CRC register after byte b
__device__ __host__ __forceinline__ unsigned pg_crc_byte(unsigned c, unsigned b) {
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PG_POLY : c >> 1;
    return c;
}
// a * b mod the CRC polynomial, both reflected (bit 31 is x^0)
__device__ __host__ __forceinline__ unsigned pg_multmodp(unsigned a, unsigned b) {
    unsigned p = 0;
    for (unsigned m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PG_POLY : b >> 1;
    }
    return p;
}
// x^(8 * bytes) mod the polynomial: what moves a CRC remainder `bytes` bytes towards the front
__device__ __forceinline__ unsigned pg_shift(const unsigned *__restrict__ x2n, unsigned long long bytes) {
    unsigned p = 1u << 31;
    for (int k = 3; bytes; bytes >>= 1, ++k)
        if (bytes & 1ull) p = pg_multmodp(x2n[k & 31], p);
    return p;
}

struct PgBuilder {          // LDS of the code builder
    unsigned work[PG_LIT];  // the counts the tree is built of
    unsigned weight[2 * PG_LIT];
    unsigned short parent[2 * PG_LIT];
    unsigned short leaf_symbol[PG_LIT];
    unsigned next_code[16];
    unsigned leaves, deepest;
};

// counts[n] -> lengths[n] of at most `limit` bits and codes[n] = the code's bits in stream order | length << 16.  The whole workgroup calls it.
__device__ void pg_build_codes(const unsigned *counts, int n, unsigned limit, unsigned char *lengths, unsigned *codes, PgBuilder &B) {
    const int tid = threadIdx.x;
    for (int s = tid; s < n; s += PG_THREADS) B.work[s] = counts[s];
    __syncthreads();
    if (tid == 0) {  // fewer than two used symbols: the lowest unused ones get a count of 1
        int used = 0;
        for (int s = 0; s < n; ++s) used += B.work[s] != 0;
        for (int s = 0; used < 2 && s < n; ++s)
            if (!B.work[s]) {
                B.work[s] = 1;
                ++used;
            }
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) B.leaves = B.deepest = 0;
        __syncthreads();
        for (int s = tid; s < n; s += PG_THREADS) {
            const unsigned c = B.work[s];
            lengths[s] = 0;
            if (!c) continue;
            int r = 0;  // leaves in order of (count, symbol)
            for (int j = 0; j < n; ++j) {
                const unsigned o = B.work[j];
                r += o && (o < c || (o == c && j < s));
            }
            B.leaf_symbol[r] = (unsigned short)s;
            B.weight[r] = c;
            atomicAdd(&B.leaves, 1u);
        }
        __syncthreads();
        const int m = (int)B.leaves;
        if (tid == 0) {  // always join the two smallest of (next leaf, next joined node), a leaf before a node of the same weight
            int li = 0, ni = m;
            for (int fresh = m; fresh < 2 * m - 1; ++fresh) {
                unsigned total = 0;
                for (int k = 0; k < 2; ++k) {
                    int pick;
                    if (li < m && (ni >= fresh || B.weight[li] <= B.weight[ni]))
                        pick = li++;
                    else
                        pick = ni++;
                    B.parent[pick] = (unsigned short)fresh;
                    total += B.weight[pick];
                }
                B.weight[fresh] = total;
            }
        }
        __syncthreads();
        for (int leaf = tid; leaf < m; leaf += PG_THREADS) {
            unsigned depth = 0;
            for (int node = leaf; node != 2 * m - 2; node = B.parent[node]) ++depth;
            lengths[B.leaf_symbol[leaf]] = (unsigned char)min(depth, 255u);
            atomicMax(&B.deepest, depth);
        }
        __syncthreads();
        if (B.deepest <= limit) break;  // the same for every thread
        for (int s = tid; s < n; s += PG_THREADS)
            if (B.work[s]) B.work[s] = (B.work[s] + 1u) >> 1;
        __syncthreads();
    }
    if (tid == 0) {  // RFC 1951 3.2.2
        unsigned per_length[16] = {0};
        for (int s = 0; s < n; ++s) per_length[lengths[s] & 15]++;
        per_length[0] = 0;
        unsigned code = 0;
        B.next_code[0] = 0;
        for (int bits = 1; bits < 16; ++bits) {
            code = (code + per_length[bits - 1]) << 1;
            B.next_code[bits] = code;
        }
    }
    __syncthreads();
    for (int s = tid; s < n; s += PG_THREADS) {
        const unsigned len = lengths[s];
        unsigned entry = 0;
        if (len) {
            unsigned code = B.next_code[len];
            for (int j = 0; j < s; ++j) code += lengths[j] == len;
            entry = (__brev(code) >> (32u - len)) | len << 16;
        }
        codes[s] = entry;
    }
    __syncthreads();
}

// n <= 32 bits of v (v < 2^n) at bit `pos` of an image whose bytes fill from their least significant bit
__device__ __forceinline__ void pg_put(unsigned *image, unsigned pos, unsigned v, unsigned n) {
    if (!n || (pos >> 5) + 1u >= (unsigned)PG_OUT_WORDS) return;  // never: a dynamic block is only written where it is shorter than the stored one
    const unsigned long long x = (unsigned long long)v << (pos & 31u);
    if ((unsigned)x) atomicOr(image + (pos >> 5), (unsigned)x);
    if ((unsigned)(x >> 32)) atomicOr(image + (pos >> 5) + 1, (unsigned)(x >> 32));
}

// grid (segments of all pictures)
__global__ __launch_bounds__(PG_THREADS) void png_segment_kernel(const PngPic *__restrict__ pics, int n_pics, const PngTables *__restrict__ tab,
                                                                 const uint8_t *__restrict__ stream, const unsigned *__restrict__ previous,
                                                                 uint8_t *__restrict__ slots, unsigned *__restrict__ seg_bytes, unsigned *__restrict__ seg_crc,
                                                                 unsigned *__restrict__ seg_adler) {
    __shared__ unsigned match[PG_SEGMENT];
    __shared__ unsigned image[PG_OUT_WORDS];
    __shared__ unsigned lit_count[PG_LIT], dist_count[PG_DIST], cl_count[PG_CL];
    __shared__ unsigned lit_code[PG_LIT], dist_code[PG_DIST], cl_code[PG_CL];
    __shared__ unsigned char lit_len[PG_LIT], dist_len[PG_DIST], cl_len[PG_CL];
    __shared__ PgBuilder builder;
    __shared__ unsigned scan_lds[PG_THREADS / 64];
    __shared__ unsigned header_bits, block_bits, crc_acc;  // header_bits: of a dynamic block in front of its first token, from lane 0 to all
    __shared__ unsigned long long adler_a, adler_b;
    __shared__ int hlit, hdist, hclen;
    const int tid = threadIdx.x;
    const PngPic P = pics[pg_picture_of_segment(pics, n_pics, blockIdx.x)];
    const int seg = blockIdx.x - P.first_seg, s0 = seg * PG_SEGMENT, L = min(PG_SEGMENT, P.stream_len - s0), final = seg == P.nseg - 1;
    const int bpp = P.kind == HIVE_PNG_GRAY8 ? 1 : P.kind == HIVE_PNG_GRAY16 ? 2 : 3;
    const uint8_t *st = stream + P.stream_off;  // the picture's stream
    for (int i = tid; i < PG_OUT_WORDS; i += PG_THREADS) image[i] = 0;
    for (int i = tid; i < PG_LIT; i += PG_THREADS) lit_count[i] = i == 256;
    if (tid < PG_DIST) dist_count[tid] = 0;
    if (tid < PG_CL) cl_count[tid] = 0;
    if (tid == 0) {
        block_bits = crc_acc = 0;
        adler_a = adler_b = 0;
    }
    // the three candidates of every position
    for (int i = tid; i < L; i += PG_THREADS) {
        const int p = s0 + i, room = min(PG_MAX_MATCH, L - i);
        int best = 0, best_d = 0;
        if (room >= PG_MIN_MATCH) {
            int cand[3] = {bpp, P.rowbytes + 1, 0};
            const unsigned g = previous[P.stream_off + p];
            if (g != PG_NONE && (long long)g >= P.stream_off && p + 3 <= P.stream_len) cand[2] = (int)(P.stream_off + p - (long long)g);
            for (int k = 0; k < 3; ++k) {
                const int d = cand[k];
                if (d < 1 || d > p || d > PG_WINDOW || (k == 1 && d == cand[0]) || (k == 2 && (d == cand[0] || d == cand[1]))) continue;
                int len = 0;
                while (len < room && st[p + len] == st[p - d + len]) ++len;
                if (len < PG_MIN_MATCH || (len == PG_MIN_MATCH && d > PG_FAR)) continue;
                if (len > best || (len == best && d < best_d)) {
                    best = len;
                    best_d = d;
                }
            }
        }
        match[i] = best ? (unsigned)best | (unsigned)(best_d - 1) << 9 : 0u;
    }
    __syncthreads();
    if (tid == 0)  // the greedy parse from the segment's start
        for (int i = 0; i < L;) {
            const unsigned m = match[i];
            match[i] = m | PG_TOKEN;
            i += (m & 511u) ? (int)(m & 511u) : 1;
        }
    __syncthreads();
    for (int i = tid; i < L; i += PG_THREADS) {
        const unsigned m = match[i];
        if (!(m & PG_TOKEN)) continue;
        if (m & 511u) {
            atomicAdd(&lit_count[257 + pg_length_symbol((int)(m & 511u))], 1u);
            atomicAdd(&dist_count[pg_dist_symbol((int)((m >> 9) & 32767u) + 1)], 1u);
        } else {
            atomicAdd(&lit_count[st[s0 + i]], 1u);
        }
    }
    __syncthreads();
    pg_build_codes(lit_count, PG_LIT, 15, lit_len, lit_code, builder);
    pg_build_codes(dist_count, PG_DIST, 15, dist_len, dist_code, builder);
    if (tid == 0) {
        int top = PG_LIT - 1;
        while (top > 256 && !lit_len[top]) --top;
        hlit = top + 1;
        top = PG_DIST - 1;
        while (top > 0 && !dist_len[top]) --top;
        hdist = top + 1;
    }
    __syncthreads();
    for (int k = tid; k < hlit + hdist; k += PG_THREADS) atomicAdd(&cl_count[k < hlit ? lit_len[k] : dist_len[k - hlit]], 1u);
    __syncthreads();
    pg_build_codes(cl_count, PG_CL, 7, cl_len, cl_code, builder);
    if (tid == 0) {
        int top = 18;
        while (top > 3 && !cl_len[PG_CL_ORDER[top]]) --top;
        hclen = top + 1;
    }
    // the block's bits: 3 + 5 + 5 + 4, the code-length code, the code lengths, the tokens, the end of block
    {
        unsigned bits = 0;
        for (int s = tid; s < PG_LIT; s += PG_THREADS) bits += lit_count[s] * (lit_len[s] + (s > 256 ? PG_LENGTH_EXTRA[s - 257] : 0u));
        if (tid < PG_DIST) bits += dist_count[tid] * (dist_len[tid] + PG_DIST_EXTRA[tid]);
        if (tid < PG_CL) bits += cl_count[tid] * cl_len[tid];
        if (bits) atomicAdd(&block_bits, bits);
    }
    __syncthreads();
    const unsigned total_bits = 17u + 3u * (unsigned)hclen + block_bits;
    const unsigned coded_bytes = final ? (total_bits + 7u) / 8u : (total_bits + 3u + 7u) / 8u + 4u;
    const bool dynamic = coded_bytes < (unsigned)L + 5u;
    const unsigned nbytes = dynamic ? coded_bytes : (unsigned)L + 5u;
    if (dynamic) {
        if (tid == 0) {
            unsigned pos = 0;
            pg_put(image, pos, (unsigned)final | 2u << 1, 3), pos += 3;
            pg_put(image, pos, (unsigned)(hlit - 257), 5), pos += 5;
            pg_put(image, pos, (unsigned)(hdist - 1), 5), pos += 5;
            pg_put(image, pos, (unsigned)(hclen - 4), 4), pos += 4;
            for (int k = 0; k < hclen; ++k, pos += 3) pg_put(image, pos, cl_len[PG_CL_ORDER[k]], 3);
            for (int k = 0; k < hlit + hdist; ++k) {
                const unsigned e = cl_code[k < hlit ? lit_len[k] : dist_len[k - hlit]];
                pg_put(image, pos, e & 0xFFFFu, e >> 16), pos += e >> 16;
            }
            header_bits = pos;
        }
        __syncthreads();
        unsigned carry = header_bits;  // bits in front of this chunk of positions (header_bits is not written again)
        for (int base = 0; base < L; base += PG_THREADS) {
            const int i = base + tid;
            unsigned first = 0, first_bits = 0, second = 0, second_bits = 0;
            const unsigned m = i < L ? match[i] : 0u;
            if (m & PG_TOKEN) {
                if (m & 511u) {
                    const int length = (int)(m & 511u), distance = (int)((m >> 9) & 32767u) + 1, ls = pg_length_symbol(length), ds = pg_dist_symbol(distance);
                    const unsigned le = lit_code[257 + ls], de = dist_code[ds];
                    first = (le & 0xFFFFu) | (unsigned)(length - PG_LENGTH_BASE[ls]) << (le >> 16);
                    first_bits = (le >> 16) + PG_LENGTH_EXTRA[ls];
                    second = (de & 0xFFFFu) | (unsigned)(distance - PG_DIST_BASE[ds]) << (de >> 16);
                    second_bits = (de >> 16) + PG_DIST_EXTRA[ds];
                } else {
                    const unsigned le = lit_code[st[s0 + i]];
                    first = le & 0xFFFFu;
                    first_bits = le >> 16;
                }
            }
            unsigned chunk_bits;
            const unsigned at = block_exclusive_total(first_bits + second_bits, scan_lds, &chunk_bits);
            pg_put(image, carry + at, first, first_bits);
            pg_put(image, carry + at + first_bits, second, second_bits);
            carry += chunk_bits;
        }
        if (tid == 0) {
            pg_put(image, carry, lit_code[256] & 0xFFFFu, lit_code[256] >> 16);
            // behind a block that is not the last: 000 (an empty stored block), zeros up to the byte, LEN 0000, NLEN FFFF
            if (!final) pg_put(image, (nbytes - 2u) * 8u, 0xFFFFu, 16);
        }
        __syncthreads();
    }
    // the segment's bytes: to its slot, into the CRC remainder (every thread a run of bytes, moved to the segment's end) and, of its INPUT bytes, the Adler sums
    auto byte_at = [&](unsigned i) -> unsigned {
        if (dynamic) return (image[i >> 2] >> (8u * (i & 3u))) & 255u;
        if (i >= 5u) return st[s0 + (int)i - 5];
        const unsigned len = (unsigned)L;
        return i == 0 ? (unsigned)final : i == 1 ? (len & 255u) : i == 2 ? (len >> 8) : i == 3 ? (~len & 255u) : ((~len >> 8) & 255u);
    };
    uint8_t *slot = slots + (size_t)blockIdx.x * PG_SLOT;
    for (unsigned i = tid; i < nbytes; i += PG_THREADS) slot[i] = (uint8_t)byte_at(i);
    {
        const unsigned run = (nbytes + PG_THREADS - 1u) / PG_THREADS, from = min(nbytes, (unsigned)tid * run), to = min(nbytes, from + run);
        if (to > from) {
            unsigned c = 0;
            for (unsigned i = from; i < to; ++i) c = pg_crc_byte(c, byte_at(i));
            atomicXor(&crc_acc, pg_multmodp(pg_shift(tab->x2n, nbytes - to), c));
        }
        unsigned a = 0, b = 0;  // b: byte k of the segment counts L - k times
        for (int i = tid; i < L; i += PG_THREADS) {
            const unsigned v = st[s0 + i];
            a += v;
            b += v * (unsigned)(L - i);
        }
        atomicAdd(&adler_a, (unsigned long long)a);
        atomicAdd(&adler_b, (unsigned long long)b);
    }
    __syncthreads();
    if (tid == 0) {
        seg_bytes[blockIdx.x] = nbytes;
        seg_crc[blockIdx.x] = crc_acc;
        seg_adler[2 * (size_t)blockIdx.x] = (unsigned)(adler_a % 65521ull);
        seg_adler[2 * (size_t)blockIdx.x + 1] = (unsigned)(adler_b % 65521ull);
    }
}

__device__ __forceinline__ void pg_store_be32(uint8_t *dst, unsigned v) {
    dst[0] = (uint8_t)(v >> 24);
    dst[1] = (uint8_t)(v >> 16);
    dst[2] = (uint8_t)(v >> 8);
    dst[3] = (uint8_t)v;
}

// grid (pictures): seg_off (behind the zlib header), sizes[picture], and every byte of the file that is not a segment's
__global__ __launch_bounds__(PG_THREADS) void png_picture_kernel(const PngPic *__restrict__ pics, const PngTables *__restrict__ tab, const unsigned *__restrict__ seg_bytes,
                                                                 const unsigned *__restrict__ seg_crc, const unsigned *__restrict__ seg_adler,
                                                                 unsigned *__restrict__ seg_off, uint8_t *__restrict__ out, long long *__restrict__ sizes) {
    __shared__ unsigned lds[PG_THREADS / 64];
    __shared__ unsigned crc_acc;
    __shared__ unsigned long long s1, s2;
    const PngPic P = pics[blockIdx.x];
    if (threadIdx.x == 0) {
        crc_acc = 0;
        s1 = s2 = 0;
    }
    const unsigned deflate_bytes = block_scan_chunks((unsigned)P.nseg, lds, [&](unsigned i) { return seg_bytes[P.first_seg + i]; },
                                                     [&](unsigned i, unsigned at) { seg_off[P.first_seg + i] = at; });
    // Adler-32 of the stream: s1 = 1 + every byte; s2 = every running s1 = the length + every segment's own sum + its byte sum times the bytes behind it.
    // CRC of "IDAT" + data: every segment's remainder moved by the bytes behind it (the Adler-32's four among them)
    unsigned long long a_sum = 0, b_sum = 0;
    unsigned crc = 0;
    for (int i = threadIdx.x; i < P.nseg; i += PG_THREADS) {
        const int g = P.first_seg + i;
        const unsigned long long a = seg_adler[2 * (size_t)g], b = seg_adler[2 * (size_t)g + 1];
        const long long behind = (long long)P.stream_len - min((long long)(i + 1) * PG_SEGMENT, (long long)P.stream_len);
        a_sum += a;
        b_sum += (b + a * (unsigned long long)(behind % 65521)) % 65521ull;
        crc ^= pg_multmodp(pg_shift(tab->x2n, (unsigned long long)(deflate_bytes - seg_off[g] - seg_bytes[g]) + 4ull), seg_crc[g]);
    }
    atomicAdd(&s1, a_sum);
    atomicAdd(&s2, b_sum);
    if (crc) atomicXor(&crc_acc, crc);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint8_t *dst = out + P.out_off;
        const unsigned char signature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
        for (int k = 0; k < 8; ++k) dst[k] = signature[k];
        pg_store_be32(dst + 8, 13u);
        const unsigned char ihdr[17] = {'I', 'H', 'D', 'R', (unsigned char)(P.W >> 24), (unsigned char)(P.W >> 16), (unsigned char)(P.W >> 8), (unsigned char)P.W,
                                        (unsigned char)(P.H >> 24), (unsigned char)(P.H >> 16), (unsigned char)(P.H >> 8), (unsigned char)P.H,
                                        (unsigned char)(P.kind == HIVE_PNG_GRAY16 ? 16 : 8), (unsigned char)(P.kind == HIVE_PNG_RGB8 ? 2 : 0), 0, 0, 0};
        unsigned c = 0xFFFFFFFFu;
        for (int k = 0; k < 17; ++k) {
            dst[12 + k] = ihdr[k];
            c = pg_crc_byte(c, ihdr[k]);
        }
        pg_store_be32(dst + 29, ~c);
        pg_store_be32(dst + 33, deflate_bytes + 6u);
        const unsigned char front[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
        c = 0xFFFFFFFFu;
        for (int k = 0; k < 6; ++k) {
            dst[37 + k] = front[k];
            c = pg_crc_byte(c, front[k]);
        }
        const unsigned adler = (unsigned)(((unsigned long long)P.stream_len + s2) % 65521ull) << 16 | (unsigned)((1ull + s1) % 65521ull);
        uint8_t *tail = dst + PG_DATA_AT + deflate_bytes;
        pg_store_be32(tail, adler);
        unsigned last = 0;
        for (int k = 0; k < 4; ++k) last = pg_crc_byte(last, (adler >> (24 - 8 * k)) & 255u);
        c = pg_multmodp(pg_shift(tab->x2n, (unsigned long long)deflate_bytes + 4ull), c) ^ crc_acc ^ last;
        pg_store_be32(tail + 4, ~c);
        const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int k = 0; k < 12; ++k) tail[8 + k] = iend[k];
        sizes[blockIdx.x] = (long long)PG_FIXED + deflate_bytes;
    }
}

// grid (segments): the slot's bytes to their place in the file
__global__ __launch_bounds__(PG_THREADS) void png_place_kernel(const PngPic *__restrict__ pics, int n_pics, const uint8_t *__restrict__ slots,
                                                               const unsigned *__restrict__ seg_bytes, const unsigned *__restrict__ seg_off, uint8_t *__restrict__ out) {
    const PngPic P = pics[pg_picture_of_segment(pics, n_pics, blockIdx.x)];
    const uint8_t *slot = slots + (size_t)blockIdx.x * PG_SLOT;
    const unsigned nbytes = min(seg_bytes[blockIdx.x], (unsigned)PG_SLOT);
    uint8_t *dst = out + P.out_off + PG_DATA_AT + seg_off[blockIdx.x];
    for (unsigned i = threadIdx.x; i < nbytes; i += PG_THREADS) dst[i] = slot[i];
}

int png_bpp(int kind) { return kind == HIVE_PNG_GRAY8 ? 1 : kind == HIVE_PNG_GRAY16 ? 2 : 3; }

// validates the call and fills offsets[n] (may be NULL) and *total_bytes
int png_layout(hive_ctx *ctx, const hive_png_image *images, int n, int64_t *offsets, int64_t *total_bytes) {
    HIVE_REQUIRE(ctx, images && n >= 1 && n <= PG_MAX_PICTURES, "png: %d pictures (1 .. %d, and a descriptor table)", n, PG_MAX_PICTURES);
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const hive_png_image &im = images[i];
        HIVE_REQUIRE(ctx, im.kind == HIVE_PNG_GRAY8 || im.kind == HIVE_PNG_GRAY16 || im.kind == HIVE_PNG_RGB8, "png: picture %d: unknown kind %d (%d gray 8, %d gray 16, %d RGB 8)",
                     i, im.kind, HIVE_PNG_GRAY8, HIVE_PNG_GRAY16, HIVE_PNG_RGB8);
        if (int rc = hive_picture_sides(ctx, "png", i, im.height, im.width)) return rc;
        const int64_t stream = (int64_t)im.height * (1 + (int64_t)im.width * png_bpp(im.kind));
        HIVE_REQUIRE(ctx, stream <= PG_MAX_STREAM, "png: picture %d has %lld bytes of rows (at most %lld per call)", i, (long long)stream, PG_MAX_STREAM);
        if (offsets) offsets[i] = at;
        at += (PG_FIXED + stream + 5 * ((stream + PG_SEGMENT - 1) / PG_SEGMENT) + 3) & ~(int64_t)3;
    }
    if (total_bytes) *total_bytes = at;
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_png_layout(const hive_png_image *images, int n, int64_t *offsets, int64_t *total_bytes) {
    if (!offsets || !total_bytes) return hive_fail(nullptr, HIVE_ERR_INVALID, "png_layout: NULL argument");
    return png_layout(nullptr, images, n, offsets, total_bytes);
}

int hive_png_encode(hive_ctx *ctx, const hive_png_image *images, int n, uint8_t *d_out, int64_t out_bytes, int64_t *sizes) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_out && sizes, "png_encode: NULL argument");
    std::vector<int64_t> offsets((size_t)std::max(n, 1));
    int64_t total_bytes = 0;
    int rc;
    if ((rc = png_layout(ctx, images, n, offsets.data(), &total_bytes))) return rc;
    if ((rc = hive_picture_room(ctx, "png", out_bytes, total_bytes))) return rc;
    std::vector<PngPic> pics((size_t)n);
    long long positions = 0, segments = 0, rows = 0;
    for (int i = 0; i < n; ++i) {
        const hive_png_image &im = images[i];
        const int rowbytes = im.width * png_bpp(im.kind);
        HIVE_REQUIRE(ctx, im.pixels, "png_encode: picture %d: NULL pixels", i);
        HIVE_REQUIRE(ctx, im.pitch >= rowbytes, "png_encode: picture %d: a row pitch of %lld bytes under its %d bytes of pixels", i, (long long)im.pitch, rowbytes);
        PngPic &P = pics[(size_t)i];
        memset(&P, 0, sizeof(P));
        P.src = (const uint8_t *)im.pixels;
        P.pitch = im.pitch;
        P.out_off = offsets[(size_t)i];
        P.stream_off = positions;
        P.H = im.height;
        P.W = im.width;
        P.kind = im.kind;
        P.rowbytes = rowbytes;
        P.stream_len = im.height * (rowbytes + 1);
        P.first_seg = (int)segments;
        P.nseg = (P.stream_len + PG_SEGMENT - 1) / PG_SEGMENT;
        P.first_row = (int)rows;
        positions += P.stream_len;
        segments += P.nseg;
        rows += im.height;
        HIVE_REQUIRE(ctx, positions <= PG_MAX_STREAM, "png_encode: more than %lld bytes of rows in one call (reached at picture %d)", PG_MAX_STREAM, i);
    }
    PngTables tables;
    tables.x2n[0] = 1u << 30;  // x^1
    for (int k = 1; k < 32; ++k) tables.x2n[k] = pg_multmodp(tables.x2n[k - 1], tables.x2n[k - 1]);
    const unsigned N = (unsigned)positions, tiles = (N + PG_TILE - 1) / PG_TILE;
    hive_scratch_layout L;
    for (int pass = 0; pass < 2; ++pass) {
        L.off = 0;
        PngPic *d_pics = L.take<PngPic>((size_t)n);
        PngTables *d_tab = L.take<PngTables>(1);
        uint8_t *d_stream = L.take<uint8_t>((size_t)N + 4);
        unsigned *d_order_a = L.take<unsigned>((size_t)N), *d_order_b = L.take<unsigned>((size_t)N);
        unsigned *d_hist = L.take<unsigned>((size_t)tiles * 256), *d_totals = L.take<unsigned>(256);
        uint8_t *d_slots = L.take<uint8_t>((size_t)segments * PG_SLOT);
        unsigned *d_seg_bytes = L.take<unsigned>((size_t)segments), *d_seg_crc = L.take<unsigned>((size_t)segments), *d_seg_off = L.take<unsigned>((size_t)segments);
        unsigned *d_seg_adler = L.take<unsigned>((size_t)segments * 2);
        long long *d_sizes = L.take<long long>((size_t)n);
        if (pass == 0) {
            if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, L.bytes()))) return rc;
            L.base = (char *)ctx->d_scratch;
            continue;
        }
        if ((rc = hive_upload_tables(ctx, d_pics, pics, d_tab, tables))) return rc;
        const dim3 threads(PG_THREADS);
        hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), threads, 0, ctx->stream, d_pics, n, (int)rows, d_stream);
        // three stable passes, the last by the first byte: identity -> a -> b -> a
        const unsigned *in = nullptr;
        unsigned *out = d_order_a;
        for (int p = 0; p < 3; ++p) {
            hipLaunchKernelGGL(png_sort_count_kernel, dim3(tiles), threads, 0, ctx->stream, (const uint8_t *)d_stream, N, in, p, d_hist);
            hipLaunchKernelGGL(png_sort_scan_kernel, dim3(256), threads, 0, ctx->stream, d_hist, tiles, d_totals);
            hipLaunchKernelGGL(png_sort_scatter_kernel, dim3(tiles), threads, 0, ctx->stream, (const uint8_t *)d_stream, N, in, p, (const unsigned *)d_hist,
                               (const unsigned *)d_totals, out);
            in = out;
            out = out == d_order_a ? d_order_b : d_order_a;
        }
        unsigned *d_previous = out;  // the buffer the last pass did not write
        hipLaunchKernelGGL(png_previous_kernel, dim3((N + PG_THREADS - 1) / PG_THREADS), threads, 0, ctx->stream, (const uint8_t *)d_stream, N, in, d_previous);
        hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)segments), threads, 0, ctx->stream, d_pics, n, d_tab, (const uint8_t *)d_stream,
                           (const unsigned *)d_previous, d_slots, d_seg_bytes, d_seg_crc, d_seg_adler);
        hipLaunchKernelGGL(png_picture_kernel, dim3((unsigned)n), threads, 0, ctx->stream, d_pics, d_tab, (const unsigned *)d_seg_bytes, (const unsigned *)d_seg_crc,
                           (const unsigned *)d_seg_adler, d_seg_off, d_out, d_sizes);
        hipLaunchKernelGGL(png_place_kernel, dim3((unsigned)segments), threads, 0, ctx->stream, d_pics, n, (const uint8_t *)d_slots, (const unsigned *)d_seg_bytes,
                           (const unsigned *)d_seg_off, d_out);
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        return hive_read_sizes(ctx, d_sizes, n, sizes);
    }
    return HIVE_OK;
}

}  // extern "C"
