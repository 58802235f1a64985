// Baseline JPEG encoder: a batch of RGB pictures of different sizes -> one JFIF file each, packed into the caller's device buffer.  gfx950 only.
//
//   hive_jpeg_layout -> worst-case byte bound and offset of every picture (host only)
//   hive_jpeg_encode -> the files in d_out and their sizes, SEVEN launches and one clear for any number of pictures
//
// The rules (libjpeg's integer arithmetic, Pillow's header) are stated in include/hive_mi355x.h and restated in numpy in tests/jpeg_restatement.py.  Integer
// arithmetic only; the only atomics are integer ORs of disjoint bits and one integer add per byte counted, so the bytes do not depend on the launch geometry,
// the run, the batch or the position in it.
//
// One upload carries the picture table (source, size, the MCUs and intervals before it, where its file goes), the quantisation divisors, the four Huffman
// tables as code | length << 16 per symbol, and the header template.  "Block" is an 8 x 8 block of one component, numbered in scan order over all pictures:
// block = MCU * blocks-per-MCU + position in the MCU (4:4:4: Y Cb Cr; 4:2:0: Y00 Y01 Y10 Y11 Cb Cr); "interval" is one MCU row (the restart interval).
//   transform      one workgroup per 30 blocks (whole MCUs: 10 or 5).  A thread per sample: colour conversion with the edge rules as clamped reads (and the
//                  2 x 2 mean of 4:2:0 chroma) into LDS; a thread per block row, then per block column: the 8-point butterfly in place (rows 9 words apart,
//                  blocks 72: both passes free of bank conflicts); a thread per coefficient: quantise into zigzag order (int16, LDS); dummy blocks take their
//                  DC; one coalesced copy to the coefficient scratch.
//   lengths        one wave per block, lane k = zigzag coefficient k: the ballot of the non-zero lanes gives each lane its zero run (the distance to the
//                  previous set bit), hence its ZRL count, size category and code length; lane 0 codes the DC difference against the previous block of its
//                  component (a plain read, no chain), lane 63 the EOB.  The wave's sum is the block's bit length.
//   block scan     one workgroup per interval: exclusive scan of the lengths -> each block's bit offset in its interval, and the interval's bits.
//   bits           the lengths' wave again; a wave prefix sum places each lane's code, ORed into the interval's unstuffed stream (cleared before; 32-bit
//                  words holding four bytes most significant first).
//   count          one workgroup per interval: bytes of the stream (the last padded with 1-bits) and how many are 0xFF -> the interval's length with its marker.
//   picture scan   one workgroup per picture: exclusive scan of its intervals' lengths -> where each goes, the file's size, and the header.
//   stuff          one workgroup per interval: every byte to its place behind the 0xFF bytes before it (a block scan per 256 bytes), a 0x00 behind each 0xFF,
//                  then RSTn or EOI.
// The kernels move bytes and small integers; none is compute-bound.  The scans and the search are hive_internal.hpp's: block_scan_chunks (block scan, picture
// scan), block_exclusive_total (stuff: the 0xFF count of a chunk is carried in a register) and last_not_after (the picture of an MCU or an interval); the
// host frame -- the one upload, the sizes' read-back, the checks of the sides and of out_bytes -- is shared with png.hip through the same header.
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_GROUP_BLOCKS = 30;     // blocks per workgroup of the transform: a multiple of 3 and of 6
constexpr int JP_ROW = 9, JP_BLOCK = 72;  // LDS strides of a block's row and of a block, in words
constexpr int JP_BLOCK_BITS = 22 + 63 * 26;  // the longest block: see hive_jpeg_layout in hive_mi355x.h
constexpr int JP_BLOCK_WORDS = (JP_BLOCK_BITS + 31) / 32;  // 52 words = 208 bytes of unstuffed stream per block
constexpr int JP_HEADER = 629;
constexpr long long JP_MAX_BLOCKS = 1ll << 22;
constexpr int JP_MAX_PICTURES = 1 << 16;

struct JpegPic {
    const uint8_t *src;
    long long pitch;
    long long out_off;   // of the file in d_out
    long long bound;     // the layout's bound of the file
    int H, W;
    int mcus_x, mcus_y;
    int first_mcu;       // MCUs of the pictures before this one
    int first_interval;  // MCU rows of the pictures before this one
    int pad[2];
};
static_assert(sizeof(JpegPic) == 64, "JpegPic is uploaded as a table of 64-byte rows");

struct JpegTables {
    unsigned short divisor[2][64];  // quantisation table << 3, natural order; [0] luminance, [1] chrominance
    unsigned dc[2][16];             // code | length << 16 per size category
    unsigned ac[2][256];            // code | length << 16 per run << 4 | size
    int size_at, dri_at;            // where the header holds height, width (2 + 2 bytes) and the restart interval (2 bytes)
    unsigned char header[JP_HEADER + 3];
};

const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// the zigzag position of the coefficient at natural index p
__constant__ unsigned char JP_ZIGZAG_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// the picture that holds MCU / interval `at` of the call
__device__ __forceinline__ int jp_picture_of_mcu(const JpegPic *__restrict__ pics, int n, int at) {
    return last_not_after(n, at, [pics](int i) { return pics[i].first_mcu; });
}
__device__ __forceinline__ int jp_picture_of_interval(const JpegPic *__restrict__ pics, int n, int at) {
    return last_not_after(n, at, [pics](int i) { return pics[i].first_interval; });
}

// JFIF colour conversion in 16-bit fixed point: component 0 Y, 1 Cb, 2 Cr
__device__ __forceinline__ int jp_convert(const uint8_t *__restrict__ px, int comp) {
    const int r = px[0], g = px[1], b = px[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the 8-point butterfly of the slow integer DCT (Loeffler, Ligtenberg, Moschytz; CONST_BITS 13, PASS1_BITS 2) over d[0], d[stride], ..
template <bool FIRST>
__device__ __forceinline__ void jp_dct8(int *d, int stride) {
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride], d7 = d[7 * stride];
    int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int N = FIRST ? 11 : 15;
    d[0] = FIRST ? (tmp10 + tmp11) * 4 : jp_descale(tmp10 + tmp11, 2);
    d[4 * stride] = FIRST ? (tmp10 - tmp11) * 4 : jp_descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2 * stride] = jp_descale(z1 + tmp13 * 6270, N);
    d[6 * stride] = jp_descale(z1 - tmp12 * 15137, N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446;
    tmp5 *= 16819;
    tmp6 *= 25172;
    tmp7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * stride] = jp_descale(tmp4 + z1 + z3, N);
    d[5 * stride] = jp_descale(tmp5 + z2 + z4, N);
    d[3 * stride] = jp_descale(tmp6 + z2 + z3, N);
    d[stride] = jp_descale(tmp7 + z1 + z4, N);
}

enum { JP_DUMMY = 4, JP_VALID = 8 };  // flags of a block beside its component (bits 0 .. 1)

// grid (MCUs of all pictures / MCUs per workgroup): coef[block][64] int16 in zigzag order
template <int SUB>  // 0: 4:4:4, 1: 4:2:0
__global__ __launch_bounds__(JP_THREADS) void jpeg_transform_kernel(const JpegPic *__restrict__ pics, int n_pics, int total_mcus, const JpegTables *__restrict__ tab,
                                                                    short *__restrict__ coef) {
    constexpr int BPM = SUB ? 6 : 3, MPG = JP_GROUP_BLOCKS / BPM;
    __shared__ int samples[JP_GROUP_BLOCKS * JP_BLOCK];
    __shared__ __align__(16) short quantised[JP_GROUP_BLOCKS * 64];
    __shared__ int desc[JP_GROUP_BLOCKS][4];  // picture, first sample column and row of the block in its component, component | flags
    const int tid = threadIdx.x;
    if (tid < JP_GROUP_BLOCKS) {
        const int mcu = blockIdx.x * MPG + tid / BPM, k = tid % BPM;
        int pic = 0, bx = 0, by = 0, flags = 0;
        if (mcu < total_mcus) {
            pic = jp_picture_of_mcu(pics, n_pics, mcu);
            const JpegPic P = pics[pic];
            const int local = mcu - P.first_mcu, mx = local % P.mcus_x, my = local / P.mcus_x;
            flags = JP_VALID;
            if (SUB && k < 4) {
                bx = 2 * mx + (k & 1);
                by = 2 * my + (k >> 1);
                if (bx >= (P.W + 7) / 8 || by >= (P.H + 7) / 8) flags |= JP_DUMMY;
            } else {
                bx = mx;
                by = my;
                flags |= SUB ? k - 3 : k;
            }
        }
        desc[tid][0] = pic;
        desc[tid][1] = bx * 8;
        desc[tid][2] = by * 8;
        desc[tid][3] = flags;
    }
    __syncthreads();
    for (int idx = tid; idx < JP_GROUP_BLOCKS * 64; idx += JP_THREADS) {
        const int b = idx >> 6, r = (idx >> 3) & 7, c = idx & 7, flags = desc[b][3], comp = flags & 3;
        int v = 0;
        if ((flags & JP_VALID) && !(flags & JP_DUMMY)) {
            const JpegPic P = pics[desc[b][0]];
            const int x = desc[b][1] + c, y = desc[b][2] + r;
            if (SUB && comp) {
                // a chroma sample of 4:2:0: rows replicated up to an even height only, then the last down-sampled row replicated; columns replicated at
                // full resolution; bias 1, 2, 1, 2 .. along the output row
                const int yc = min(y, (P.H + 1) / 2 - 1);
                const int y0 = min(2 * yc, P.H - 1), y1 = min(2 * yc + 1, P.H - 1), x0 = min(2 * x, P.W - 1), x1 = min(2 * x + 1, P.W - 1);
                const uint8_t *row0 = P.src + (size_t)y0 * P.pitch, *row1 = P.src + (size_t)y1 * P.pitch;
                v = (jp_convert(row0 + 3 * (size_t)x0, comp) + jp_convert(row0 + 3 * (size_t)x1, comp) + jp_convert(row1 + 3 * (size_t)x0, comp) +
                     jp_convert(row1 + 3 * (size_t)x1, comp) + 1 + (x & 1)) >> 2;
            } else {
                v = jp_convert(P.src + (size_t)min(y, P.H - 1) * P.pitch + 3 * (size_t)min(x, P.W - 1), comp);
            }
            v -= 128;
        }
        samples[b * JP_BLOCK + r * JP_ROW + c] = v;
    }
    __syncthreads();
    if (tid < JP_GROUP_BLOCKS * 8) jp_dct8<true>(samples + (tid >> 3) * JP_BLOCK + (tid & 7) * JP_ROW, 1);
    __syncthreads();
    if (tid < JP_GROUP_BLOCKS * 8) jp_dct8<false>(samples + (tid >> 3) * JP_BLOCK + (tid & 7), JP_ROW);
    __syncthreads();
    for (int idx = tid; idx < JP_GROUP_BLOCKS * 64; idx += JP_THREADS) {
        const int b = idx >> 6, p = idx & 63, flags = desc[b][3];
        const int v = samples[b * JP_BLOCK + (p >> 3) * JP_ROW + (p & 7)], d = tab->divisor[(flags & 3) ? 1 : 0][p];
        const int m = (abs(v) + (d >> 1)) / d;
        quantised[b * 64 + JP_ZIGZAG_OF[p]] = (flags & JP_DUMMY) ? (short)0 : (short)(v < 0 ? -m : m);
    }
    __syncthreads();
    if (SUB) {
        // dummy blocks: past the right edge the DC of the block to the left; a dummy row takes the DC of Y01 (itself possibly a dummy) in both blocks
        if (tid < MPG) {
            short *q = quantised + tid * 6 * 64;
            const bool right = desc[tid * 6 + 1][3] & JP_DUMMY, bottom = desc[tid * 6 + 2][3] & JP_DUMMY;
            if (right) q[64] = q[0];
            if (bottom)
                q[128] = q[192] = q[64];
            else if (right)
                q[192] = q[128];
        }
        __syncthreads();
    }
    const int first = blockIdx.x * MPG, mcus = min(MPG, total_mcus - first), words = mcus * BPM * 32;
    unsigned *dst = (unsigned *)(coef + (size_t)first * BPM * 64);
    for (int i = tid; i < words; i += JP_THREADS) dst[i] = ((const unsigned *)quantised)[i];
}

struct JpLane {
    unsigned zrl;    // ZRL codes in front
    unsigned bits;   // the Huffman code, then the value bits
    unsigned nbits;
};

// what lane `lane` of a block's wave emits: v its coefficient (lane 0: the DC difference), acmask the non-zero AC lanes
__device__ __forceinline__ JpLane jp_lane_code(int lane, int v, unsigned long long acmask, const unsigned *__restrict__ dc, const unsigned *__restrict__ ac) {
    JpLane o = {0u, 0u, 0u};
    const unsigned a = (unsigned)abs(v), size = a ? 32u - (unsigned)__clz((int)a) : 0u;
    const unsigned value = (unsigned)(v + (v >> 31)) & ((1u << size) - 1u);
    if (lane == 0) {
        const unsigned e = dc[size];
        o.bits = (e & 0xFFFFu) << size | value;
        o.nbits = (e >> 16) + size;
    } else if (v != 0) {
        const unsigned long long before = acmask & ((1ull << lane) - 1ull);
        const int previous = before ? 63 - __clzll((long long)before) : 0;
        const unsigned run = (unsigned)(lane - previous - 1);
        const unsigned e = ac[(run & 15u) << 4 | size];
        o.zrl = run >> 4;
        o.bits = (e & 0xFFFFu) << size | value;
        o.nbits = (e >> 16) + size;
    } else if (lane == 63) {  // the last coefficient is zero: EOB
        o.bits = ac[0] & 0xFFFFu;
        o.nbits = ac[0] >> 16;
    }
    return o;
}

// the block a wave codes: its coefficient for this lane, its tables, and the first block of its interval
struct JpBlock {
    int v;
    int chroma;
    long long interval_first;
};

template <int SUB>
__device__ __forceinline__ JpBlock jp_block(const JpegPic *__restrict__ pics, int n_pics, const short *__restrict__ coef, long long g, int lane) {
    constexpr int BPM = SUB ? 6 : 3;
    const int mcu = (int)(g / BPM), k = (int)(g % BPM);
    const JpegPic P = pics[jp_picture_of_mcu(pics, n_pics, mcu)];
    const int local = mcu - P.first_mcu, mx = local % P.mcus_x;
    long long pred = -1;  // the previous block of the same component in the interval
    if (SUB && k >= 1 && k <= 3)
        pred = g - 1;
    else if (mx > 0)
        pred = SUB && k == 0 ? g - 3 : g - BPM;
    JpBlock o;
    o.v = coef[g * 64 + lane];
    if (lane == 0 && pred >= 0) o.v -= coef[pred * 64];
    o.chroma = SUB ? k >= 4 : k >= 1;
    o.interval_first = (long long)(mcu - mx) * BPM;
    return o;
}

__device__ __forceinline__ unsigned jp_lane_length(const JpLane &c, const unsigned *__restrict__ ac) { return c.zrl * (ac[0xF0] >> 16) + c.nbits; }

// grid (blocks of all pictures / 4): one wave per block -> its bit length
template <int SUB>
__global__ __launch_bounds__(JP_THREADS) void jpeg_length_kernel(const JpegPic *__restrict__ pics, int n_pics, long long total_blocks, const JpegTables *__restrict__ tab,
                                                                 const short *__restrict__ coef, unsigned *__restrict__ block_bits) {
    const long long g = (long long)blockIdx.x * (JP_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= total_blocks) return;  // the whole wave
    const JpBlock B = jp_block<SUB>(pics, n_pics, coef, g, lane);
    const unsigned long long acmask = __ballot(lane > 0 && B.v != 0);
    unsigned len = jp_lane_length(jp_lane_code(lane, B.v, acmask, tab->dc[B.chroma], tab->ac[B.chroma]), tab->ac[B.chroma]);
    for (int off = 32; off > 0; off >>= 1) len += (unsigned)__shfl_xor((int)len, off);
    if (lane == 0) block_bits[g] = len;
}

// grid (intervals): exclusive scan of the interval's block lengths -> block_off, and interval_bits
template <int SUB>
__global__ __launch_bounds__(JP_THREADS) void jpeg_block_scan_kernel(const JpegPic *__restrict__ pics, int n_pics, const unsigned *__restrict__ block_bits,
                                                                     unsigned *__restrict__ block_off, unsigned *__restrict__ interval_bits) {
    constexpr int BPM = SUB ? 6 : 3;
    __shared__ unsigned lds[JP_THREADS / 64];
    const JpegPic P = pics[jp_picture_of_interval(pics, n_pics, blockIdx.x)];
    const long long first = ((long long)P.first_mcu + (long long)(blockIdx.x - P.first_interval) * P.mcus_x) * BPM;
    const unsigned bits = block_scan_chunks((unsigned)(P.mcus_x * BPM), lds, [&](unsigned i) { return block_bits[first + i]; },
                                            [&](unsigned i, unsigned at) { block_off[first + i] = at; });
    if (threadIdx.x == 0) interval_bits[blockIdx.x] = bits;
}

// n <= 27 bits of v at bit `pos` of a stream whose 32-bit words hold their bits most significant first
__device__ __forceinline__ void jp_put(unsigned *__restrict__ stream, unsigned pos, unsigned v, unsigned n) {
    if (!n) return;
    const unsigned long long x = (unsigned long long)v << (64u - (pos & 31u) - n);
    unsigned *w = stream + (pos >> 5);
    if ((unsigned)(x >> 32)) atomicOr(w, (unsigned)(x >> 32));
    if ((unsigned)x) atomicOr(w + 1, (unsigned)x);  // non-zero only where the code reaches into the next word
}

// grid (blocks of all pictures / 4): one wave per block ORs its codes into the interval's stream (JP_BLOCK_WORDS words per block of the interval, zero before)
template <int SUB>
__global__ __launch_bounds__(JP_THREADS) void jpeg_bits_kernel(const JpegPic *__restrict__ pics, int n_pics, long long total_blocks, const JpegTables *__restrict__ tab,
                                                               const short *__restrict__ coef, const unsigned *__restrict__ block_off, unsigned *__restrict__ stream) {
    const long long g = (long long)blockIdx.x * (JP_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= total_blocks) return;
    const JpBlock B = jp_block<SUB>(pics, n_pics, coef, g, lane);
    const unsigned long long acmask = __ballot(lane > 0 && B.v != 0);
    const unsigned *ac = tab->ac[B.chroma];
    const JpLane c = jp_lane_code(lane, B.v, acmask, tab->dc[B.chroma], ac);
    const unsigned len = jp_lane_length(c, ac);
    unsigned inc = len;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    unsigned pos = block_off[g] + inc - len;
    unsigned *s = stream + B.interval_first * JP_BLOCK_WORDS;
    const unsigned zrl = ac[0xF0] & 0xFFFFu, zrl_bits = ac[0xF0] >> 16;
    for (unsigned z = 0; z < c.zrl; ++z, pos += zrl_bits) jp_put(s, pos, zrl, zrl_bits);
    jp_put(s, pos, c.bits, c.nbits);
}

// byte j of an interval's stream of `bits` bits in `nbytes` bytes: the last one padded with 1-bits
__device__ __forceinline__ unsigned jp_byte(const unsigned *__restrict__ s, unsigned j, unsigned nbytes, unsigned bits) {
    unsigned b = (s[j >> 2] >> (24u - 8u * (j & 3u))) & 255u;
    if (j == nbytes - 1u) b |= (1u << (8u * nbytes - bits)) - 1u;
    return b;
}

struct JpInterval {
    const unsigned *stream;
    int local;  // the interval's index in its picture
    int last;
    JpegPic P;
};

template <int SUB>
__device__ __forceinline__ JpInterval jp_interval(const JpegPic *__restrict__ pics, int n_pics, const unsigned *__restrict__ stream, int interval) {
    constexpr int BPM = SUB ? 6 : 3;
    JpInterval o;
    o.P = pics[jp_picture_of_interval(pics, n_pics, interval)];
    o.local = interval - o.P.first_interval;
    o.last = o.local == o.P.mcus_y - 1;
    o.stream = stream + ((long long)o.P.first_mcu + (long long)o.local * o.P.mcus_x) * BPM * JP_BLOCK_WORDS;
    return o;
}

// grid (intervals): interval_bytes = stream bytes + stuffed zeros + the two bytes of RSTn / EOI
template <int SUB>
__global__ __launch_bounds__(JP_THREADS) void jpeg_count_kernel(const JpegPic *__restrict__ pics, int n_pics, const unsigned *__restrict__ stream,
                                                                const unsigned *__restrict__ interval_bits, unsigned *__restrict__ interval_bytes) {
    __shared__ unsigned stuffed;
    if (threadIdx.x == 0) stuffed = 0;
    __syncthreads();
    const JpInterval I = jp_interval<SUB>(pics, n_pics, stream, blockIdx.x);
    const unsigned bits = interval_bits[blockIdx.x], nbytes = (bits + 7u) >> 3;
    unsigned mine = 0;
    for (unsigned j = threadIdx.x; j < nbytes; j += JP_THREADS) mine += jp_byte(I.stream, j, nbytes, bits) == 255u;
    if (mine) atomicAdd(&stuffed, mine);
    __syncthreads();
    if (threadIdx.x == 0) interval_bytes[blockIdx.x] = nbytes + stuffed + 2u;
}

// grid (pictures): exclusive scan of the picture's interval lengths -> interval_off (behind the header), sizes[picture], and the header in place
__global__ __launch_bounds__(JP_THREADS) void jpeg_picture_scan_kernel(const JpegPic *__restrict__ pics, const JpegTables *__restrict__ tab,
                                                                       const unsigned *__restrict__ interval_bytes, unsigned *__restrict__ interval_off,
                                                                       uint8_t *__restrict__ out, long long *__restrict__ sizes) {
    __shared__ unsigned lds[JP_THREADS / 64];
    const JpegPic P = pics[blockIdx.x];
    const unsigned scan_bytes = block_scan_chunks((unsigned)P.mcus_y, lds, [&](unsigned i) { return interval_bytes[P.first_interval + i]; },
                                                  [&](unsigned i, unsigned at) { interval_off[P.first_interval + i] = at; });
    if (threadIdx.x == 0) sizes[blockIdx.x] = (long long)JP_HEADER + scan_bytes;
    uint8_t *dst = out + P.out_off;
    for (int i = threadIdx.x; i < JP_HEADER; i += JP_THREADS) {
        unsigned b = tab->header[i];
        const int s = i - tab->size_at, d = i - tab->dri_at;
        if (s >= 0 && s < 4) b = ((s < 2 ? P.H : P.W) >> (s & 1 ? 0 : 8)) & 255;
        if (d >= 0 && d < 2) b = (P.mcus_x >> (d ? 0 : 8)) & 255;
        dst[i] = (uint8_t)b;
    }
}

// grid (intervals): the interval's bytes with a 0x00 behind every 0xFF, then RST(n mod 8) or, behind the last, EOI
template <int SUB>
__global__ __launch_bounds__(JP_THREADS) void jpeg_stuff_kernel(const JpegPic *__restrict__ pics, int n_pics, const unsigned *__restrict__ stream,
                                                                const unsigned *__restrict__ interval_bits, const unsigned *__restrict__ interval_off,
                                                                uint8_t *__restrict__ out) {
    __shared__ unsigned lds[JP_THREADS / 64];
    const JpInterval I = jp_interval<SUB>(pics, n_pics, stream, blockIdx.x);
    const unsigned bits = interval_bits[blockIdx.x], nbytes = (bits + 7u) >> 3;
    const long long at = (long long)JP_HEADER + interval_off[blockIdx.x];
    uint8_t *dst = out + I.P.out_off + at;
    const long long room = I.P.bound - at;  // never reached: the bound is the worst case
    unsigned carry = 0;                      // 0xFF bytes before this chunk
    for (unsigned base = 0; base < nbytes; base += JP_THREADS) {
        const unsigned j = base + threadIdx.x;
        const unsigned b = j < nbytes ? jp_byte(I.stream, j, nbytes, bits) : 0u, ff = b == 255u;
        unsigned chunk_ff;
        const unsigned before = block_exclusive_total(ff, lds, &chunk_ff);
        const long long pos = (long long)j + carry + before;
        if (j < nbytes && pos + ff < room) {
            dst[pos] = (uint8_t)b;
            if (ff) dst[pos + 1] = 0;
        }
        carry += chunk_ff;
    }
    if (threadIdx.x == 0 && (long long)nbytes + carry + 1 < room) {
        dst[nbytes + carry] = 0xFF;
        dst[nbytes + carry + 1] = (uint8_t)(I.last ? 0xD9 : 0xD0 + (I.local & 7));
    }
}

// ---- host: the Annex K tables ----------------------------------------------------------------------------------------------------------------------------
const unsigned char LUMINANCE_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61, 12, 12, 14, 19, 26,  58,  60,  55, 14, 13, 16, 24, 40,  57,  69,  56, 14, 17, 22, 29, 51,  87,  80,  62,
                                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char CHROMINANCE_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const unsigned char DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
const unsigned char AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
    0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
    0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
const unsigned char AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
    0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
    0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
    0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

struct HuffmanSpec {
    int ident;
    const unsigned char *bits, *vals;
    int n_vals;
};
const HuffmanSpec HUFFMAN[4] = {{0x00, DC_LUM_BITS, DC_VALS, 12}, {0x10, AC_LUM_BITS, AC_LUM_VALS, 162}, {0x01, DC_CHR_BITS, DC_VALS, 12}, {0x11, AC_CHR_BITS, AC_CHR_VALS, 162}};

// code | length << 16 per symbol (Annex C: codes of one length count up, one more bit doubles)
void huffman_codes(const HuffmanSpec &h, unsigned *table, int table_size) {
    std::fill(table, table + table_size, 0u);
    unsigned code = 0;
    int at = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int i = 0; i < h.bits[length - 1]; ++i, ++at, ++code)
            if (h.vals[at] < table_size) table[h.vals[at]] = code | (unsigned)length << 16;
        code <<= 1;
    }
}

void jpeg_tables(int quality, int sub, JpegTables &t) {
    memset(&t, 0, sizeof(t));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    unsigned char q[2][64];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 64; ++i) {
            q[k][i] = (unsigned char)std::min(255, std::max(1, ((k ? CHROMINANCE_Q : LUMINANCE_Q)[i] * scale + 50) / 100));
            t.divisor[k][i] = (unsigned short)(q[k][i] << 3);
        }
    huffman_codes(HUFFMAN[0], t.dc[0], 16);
    huffman_codes(HUFFMAN[1], t.ac[0], 256);
    huffman_codes(HUFFMAN[2], t.dc[1], 16);
    huffman_codes(HUFFMAN[3], t.ac[1], 256);
    // the header as Pillow writes it; height, width and the restart interval are filled in per picture
    std::vector<unsigned char> h;
    auto put = [&h](std::initializer_list<int> bytes) {
        for (int b : bytes) h.push_back((unsigned char)b);
    };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int k = 0; k < 2; ++k) {
        put({0xFF, 0xDB, 0, 67, k});
        for (int i = 0; i < 64; ++i) h.push_back(q[k][ZIGZAG[i]]);
    }
    put({0xFF, 0xC0, 0, 17, 8});
    t.size_at = (int)h.size();
    put({0, 0, 0, 0, 3, 1, sub ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (const HuffmanSpec &s : HUFFMAN) {
        put({0xFF, 0xC4, 0, 19 + s.n_vals, s.ident});
        h.insert(h.end(), s.bits, s.bits + 16);
        h.insert(h.end(), s.vals, s.vals + s.n_vals);
    }
    put({0xFF, 0xDD, 0, 4});
    t.dri_at = (int)h.size();
    put({0, 0, 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    memcpy(t.header, h.data(), std::min(h.size(), sizeof(t.header)));
}

struct JpegGrid {
    long long mcus_x, mcus_y, blocks;
};

JpegGrid jpeg_grid(const hive_jpeg_image &im, int sub) {
    const int mcu = sub ? 16 : 8;
    JpegGrid g;
    g.mcus_x = (im.width + mcu - 1) / mcu;
    g.mcus_y = (im.height + mcu - 1) / mcu;
    g.blocks = g.mcus_x * g.mcus_y * (sub ? 6 : 3);
    return g;
}

// validates the call and fills offsets[n] (may be NULL) and *total_bytes
int jpeg_layout(hive_ctx *ctx, const hive_jpeg_image *images, int n, int subsampling, int64_t *offsets, int64_t *total_bytes) {
    HIVE_REQUIRE(ctx, images && n >= 1 && n <= JP_MAX_PICTURES, "jpeg: %d pictures (1 .. %d, and a descriptor table)", n, JP_MAX_PICTURES);
    HIVE_REQUIRE(ctx, subsampling == HIVE_JPEG_444 || subsampling == HIVE_JPEG_420, "jpeg: unknown subsampling %d (%d for 4:4:4, %d for 4:2:0)", subsampling,
                 HIVE_JPEG_444, HIVE_JPEG_420);
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const hive_jpeg_image &im = images[i];
        if (int rc = hive_picture_sides(ctx, "jpeg", i, im.height, im.width)) return rc;
        const JpegGrid g = jpeg_grid(im, subsampling == HIVE_JPEG_420);
        if (offsets) offsets[i] = at;
        at += (JP_HEADER + g.blocks * (2 * JP_BLOCK_WORDS * 4) + g.mcus_y * 2 + 3) & ~(int64_t)3;
    }
    if (total_bytes) *total_bytes = at;
    return HIVE_OK;
}

template <int SUB>
int jpeg_launch(hive_ctx *ctx, const JpegPic *d_pics, int n, long long mcus, long long blocks, long long intervals, const JpegTables *d_tab, short *d_coef,
                unsigned *d_block_bits, unsigned *d_block_off, unsigned *d_interval_bits, unsigned *d_interval_bytes, unsigned *d_interval_off, unsigned *d_stream,
                uint8_t *d_out, long long *d_sizes) {
    constexpr int MPG = JP_GROUP_BLOCKS / (SUB ? 6 : 3), WAVES = JP_THREADS / 64;
    const dim3 threads(JP_THREADS), per_block((unsigned)((blocks + WAVES - 1) / WAVES)), per_interval((unsigned)intervals);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(d_stream, 0, (size_t)blocks * JP_BLOCK_WORDS * 4, ctx->stream));
    hipLaunchKernelGGL(jpeg_transform_kernel<SUB>, dim3((unsigned)((mcus + MPG - 1) / MPG)), threads, 0, ctx->stream, d_pics, n, (int)mcus, d_tab, d_coef);
    hipLaunchKernelGGL(jpeg_length_kernel<SUB>, per_block, threads, 0, ctx->stream, d_pics, n, blocks, d_tab, (const short *)d_coef, d_block_bits);
    hipLaunchKernelGGL(jpeg_block_scan_kernel<SUB>, per_interval, threads, 0, ctx->stream, d_pics, n, (const unsigned *)d_block_bits, d_block_off, d_interval_bits);
    hipLaunchKernelGGL(jpeg_bits_kernel<SUB>, per_block, threads, 0, ctx->stream, d_pics, n, blocks, d_tab, (const short *)d_coef, (const unsigned *)d_block_off, d_stream);
    hipLaunchKernelGGL(jpeg_count_kernel<SUB>, per_interval, threads, 0, ctx->stream, d_pics, n, (const unsigned *)d_stream, (const unsigned *)d_interval_bits,
                       d_interval_bytes);
    hipLaunchKernelGGL(jpeg_picture_scan_kernel, dim3((unsigned)n), threads, 0, ctx->stream, d_pics, d_tab, (const unsigned *)d_interval_bytes, d_interval_off, d_out,
                       d_sizes);
    hipLaunchKernelGGL(jpeg_stuff_kernel<SUB>, per_interval, threads, 0, ctx->stream, d_pics, n, (const unsigned *)d_stream, (const unsigned *)d_interval_bits,
                       (const unsigned *)d_interval_off, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_jpeg_layout(const hive_jpeg_image *images, int n, int subsampling, int64_t *offsets, int64_t *total_bytes) {
    if (!offsets || !total_bytes) return hive_fail(nullptr, HIVE_ERR_INVALID, "jpeg_layout: NULL argument");
    return jpeg_layout(nullptr, images, n, subsampling, offsets, total_bytes);
}

int hive_jpeg_encode(hive_ctx *ctx, const hive_jpeg_image *images, int n, int quality, int subsampling, uint8_t *d_out, int64_t out_bytes, int64_t *sizes) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_out && sizes, "jpeg_encode: NULL argument");
    HIVE_REQUIRE(ctx, quality >= 1 && quality <= 100, "jpeg_encode: quality %d outside 1 .. 100", quality);
    std::vector<int64_t> offsets((size_t)std::max(n, 1));
    int64_t total_bytes = 0;
    int rc;
    if ((rc = jpeg_layout(ctx, images, n, subsampling, offsets.data(), &total_bytes))) return rc;
    if ((rc = hive_picture_room(ctx, "jpeg", out_bytes, total_bytes))) return rc;
    const int sub = subsampling == HIVE_JPEG_420;
    std::vector<JpegPic> pics((size_t)n);
    long long mcus = 0, intervals = 0;
    for (int i = 0; i < n; ++i) {
        const hive_jpeg_image &im = images[i];
        HIVE_REQUIRE(ctx, im.data, "jpeg_encode: picture %d: NULL data", i);
        HIVE_REQUIRE(ctx, im.pitch >= 3ll * im.width, "jpeg_encode: picture %d: a row pitch of %lld bytes under its %d pixels of 3 bytes", i, (long long)im.pitch, im.width);
        const JpegGrid g = jpeg_grid(im, sub);
        JpegPic &P = pics[(size_t)i];
        memset(&P, 0, sizeof(P));
        P.src = im.data;
        P.pitch = im.pitch;
        P.out_off = offsets[(size_t)i];
        P.bound = (i + 1 < n ? offsets[(size_t)i + 1] : total_bytes) - offsets[(size_t)i];
        P.H = im.height;
        P.W = im.width;
        P.mcus_x = (int)g.mcus_x;
        P.mcus_y = (int)g.mcus_y;
        P.first_mcu = (int)mcus;
        P.first_interval = (int)intervals;
        mcus += g.mcus_x * g.mcus_y;
        intervals += g.mcus_y;
        HIVE_REQUIRE(ctx, mcus * (sub ? 6 : 3) <= JP_MAX_BLOCKS, "jpeg_encode: more than %lld 8 x 8 blocks in one call (reached at picture %d)", JP_MAX_BLOCKS, i);
    }
    const long long blocks = mcus * (sub ? 6 : 3);
    JpegTables tables;
    jpeg_tables(quality, sub, tables);
    hive_scratch_layout L;
    for (int pass = 0; pass < 2; ++pass) {
        L.off = 0;
        JpegPic *d_pics = L.take<JpegPic>((size_t)n);
        JpegTables *d_tab = L.take<JpegTables>(1);
        short *d_coef = L.take<short>((size_t)blocks * 64);
        unsigned *d_block_bits = L.take<unsigned>((size_t)blocks), *d_block_off = L.take<unsigned>((size_t)blocks);
        unsigned *d_interval_bits = L.take<unsigned>((size_t)intervals), *d_interval_bytes = L.take<unsigned>((size_t)intervals);
        unsigned *d_interval_off = L.take<unsigned>((size_t)intervals);
        unsigned *d_stream = L.take<unsigned>((size_t)blocks * JP_BLOCK_WORDS);
        long long *d_sizes = L.take<long long>((size_t)n);
        if (pass == 0) {
            if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, L.bytes()))) return rc;
            L.base = (char *)ctx->d_scratch;
            continue;
        }
        if ((rc = hive_upload_tables(ctx, d_pics, pics, d_tab, tables))) return rc;
        rc = sub ? jpeg_launch<1>(ctx, d_pics, n, mcus, blocks, intervals, d_tab, d_coef, d_block_bits, d_block_off, d_interval_bits, d_interval_bytes, d_interval_off,
                                  d_stream, d_out, d_sizes)
                 : jpeg_launch<0>(ctx, d_pics, n, mcus, blocks, intervals, d_tab, d_coef, d_block_bits, d_block_off, d_interval_bits, d_interval_bytes, d_interval_off,
                                  d_stream, d_out, d_sizes);
        if (rc) return rc;
        return hive_read_sizes(ctx, d_sizes, n, sizes);
    }
    return HIVE_OK;
}

}  // extern "C"
