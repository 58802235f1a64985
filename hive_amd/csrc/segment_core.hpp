// The arithmetic of the motion segmentation that has a sequential meaning (rules `motion`, `open`, `label` of include/hive_mi355x.h), as functions for the host
// and the device alike: the motion predicate, the extraction of a row's runs from its bit mask, which of a pixel's upper neighbours a labelling unions it
// with, and the union step.  segment.hip's kernels call these; so does any plain C++ program that includes this file (no HIP needed: HIVE_HD is `inline`
// there), which is how they are run under the host sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef HIVE_HD
#if defined(__HIPCC__)
#define HIVE_HD __host__ __device__ __forceinline__
#else
#define HIVE_HD inline
#endif
#endif

// the tile one workgroup labels in LDS: a row is one wave's ballot (64 lanes), SEG_TILE_H rows over the four waves.  tests/segmentation_cases.py reads these two
constexpr int SEG_TILE_H = 32;
constexpr int SEG_TILE_W = 64;
static_assert(SEG_TILE_W == 64, "a tile row is the ballot of one 64-lane wave");
constexpr int SEG_MAX_OPEN = 16;  // hive_mask_open: most iterations (the halo of a box pass in LDS)

// rule `motion`: float32, each operation rounded once.  The threshold is the larger of the two terms, written as a comparison so that a threshold that is
// not a number sets nothing
HIVE_HD bool seg_moving(float live, float model, float min_difference, float relative_difference) {
    const float rel = relative_difference * model;
    const float thr = min_difference > rel ? min_difference : rel;
    const float diff = model - live;
    return live > 0.0f && model > 0.0f && diff > thr;
}

// The run of set bits of `row` that holds bit c (which is set) starts at the returned column: one above the highest clear bit below c, or 0
HIVE_HD int seg_run_start(uint64_t row, int c) {
    const uint64_t clear_below = ~row & ((uint64_t(1) << c) - 1);  // c <= 63
    int top = -1;
#if defined(__HIP_DEVICE_COMPILE__)
    top = 63 - __clzll((long long)clear_below);  // __clzll(0) = 64
#else
    for (uint64_t m = clear_below; m; m >>= 1) ++top;  // (at most 64 steps: m loses a bit each)
#endif
    return top + 1;
}

// Which upper neighbours the set pixel at column c of `row` is unioned with, `up` being the row above (bits outside 0 .. 63 do not exist: the neighbouring
// tile's pixels are the border launch's).  Every pair of touching runs (own run [s, e], upper run [s', e']) gets at least one link and most get exactly
// one: where the runs share columns, at column max(s, s') -- the pixel is its own run's start or stands under the upper run's start; where they touch only
// diagonally (connectivity 8), at that one pixel pair.
constexpr int SEG_LINK_UP = 1, SEG_LINK_UP_LEFT = 2, SEG_LINK_UP_RIGHT = 4;
HIVE_HD int seg_links(uint64_t row, uint64_t up, int c, int connectivity) {
    const auto bit = [](uint64_t m, int i) { return i >= 0 && i < 64 && ((m >> i) & 1); };
    int links = 0;
    if (bit(up, c)) {
        if (!bit(row, c - 1) || !bit(up, c - 1)) links |= SEG_LINK_UP;
    } else if (connectivity == 8) {
        if (bit(up, c - 1) && !bit(row, c - 1)) links |= SEG_LINK_UP_LEFT;
        if (bit(up, c + 1) && !bit(row, c + 1)) links |= SEG_LINK_UP_RIGHT;
    }
    return links;
}

// One relaxed read of a label another thread may be lowering
HIVE_HD int seg_load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The root of x's tree.  Invariant of every label plane: L[x] <= x, and labels only ever decrease.  Termination: every step either stops (L[x] == x) or moves to a
// strictly smaller index, whatever other threads write meanwhile (they write values that are smaller still), so at most x + 1 steps.
HIVE_HD int seg_find(const int *L, int x) {
    for (;;) {
        const int p = seg_load(L + x);
        if (p == x) return x;
        x = p;
    }
}

// Joins the trees of a and b, always hanging the larger root under the smaller.  amin(p, v) lowers *p to min(*p, v) as ONE indivisible step and returns the
// value before (atomicMin on the device, plain code in a sequential program).  Termination: with roots a > b, either L[a] was still a and now is b (done), or
// another thread had lowered L[a] to old < a first; the next round starts from (old, b), both below a, so the larger root of the pair decreases strictly from
// round to round and is never negative.
template <class AtomicMin>
HIVE_HD void seg_union(int *L, int a, int b, AtomicMin amin) {
    for (;;) {
        a = seg_find(L, a), b = seg_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = amin(L + a, b);
        if (old == a) return;
        a = old;
    }
}
