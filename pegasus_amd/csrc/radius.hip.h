// radius.hip.h -- how many points lie within `radius` of every point (open3d's remove_radius_outlier: the reference's
// load_ply(clean_pcd=True) and denoise_point_cloud, /root/reference/src/gs/gaussian_model.py:238-247,633-651).  Not on the
// render path.  DESIGN.md section 15 holds the rule and what was measured.
//
// The rule.  count_i = #{ j (j = i included) : ((dx*dx) + dy*dy) + dz*dz < r2 }, all in float64: dx, dy, dz are the float64
// differences of the float32 coordinates widened exactly, r2 = radius * radius rounded once (on the host), every product and
// sum rounded on its own (radius_within() switches contraction off for itself, whatever the build's flags say) and the
// comparison strict.  Counts are exact integers, so they do not depend on the order in which any atomic below lands.
//
// The grid.  knn.hip.h's dense grid is sized from the bounding box, so one floater far away makes every cell huge; this one is
// sparse.  The cell edge is h = radius * RADIUS_CELL_MARGIN and only occupied cells exist: they sit in an open-addressing hash
// table (linear probing, at most half full) keyed by the FULL cell coordinate (three int32, stored biased so that no stored
// word is 0 = empty).  A slot's key is two write-once words, claimed by compare-and-swap one after the other: a 64-bit word
// (x, y) and a 32-bit word z.  A thread that finds (x, y) its own (or claims it) and z its own (or claims it) has its slot;
// any other outcome sends it to the next slot.  A slot whose (x, y) was claimed by one cell and whose z by another of the same
// column simply ends up as the second cell's, and the first goes on probing: no thread ever waits for another, and since both
// words are write-once a key can never sit in two slots (a thread only passes a slot whose key differs from its own for good).
// A lookup compares both words and stops at the first empty (x, y).
//   insert      one lane per point: find / claim the cell's slot, count the point there, remember the slot
//   ranges      one lane per slot: a wave scan of the counts, one atomic add per wave on the running total for the wave's
//               base.  (A scan whose order across waves is whatever order they arrive in: cells already lie in hash order,
//               which is as arbitrary, and nothing downstream depends on where a cell's range starts.)
//   scatter     one lane per point: sorted[begin[slot]++] = (x, y, z, original index), as knn_scatter_kernel does; afterwards
//               begin[slot] is the END of the cell's range and end - count its start
//   count       one lane per point IN CELL ORDER, so the lanes of a wave mostly share a cell, probe the same 27 slots
//               (one address per wave: a broadcast) and walk the same candidates; stops at `cap` hits and writes
//               min(count, cap) at the point's original index.
// One lane per point is the baseline layout and is kept: with the filter's cap of nb_points + 1 a lane in a dense region is
// done after a few dozen candidates and a floater's 27 cells are empty, so there is little for a wave-per-cell layout with
// candidates staged in LDS to win; the exact mode (cap = n) is O(points x neighbours) in any layout.  The float64 test is used
// as it is, without an fp32 prefilter: none was measured, so none was added.
//
// No pair with d2 < r2 lies more than one cell apart on any axis.  Let m = RADIUS_CELL_MARGIN - 1 = 1e-4 and u = 2^-53.
//  (a) The pair passes the test, so fl(dx*dx) <= fl(sum) < r2 = radius^2 (1 + e0) with |e0| <= u (all terms are >= 0 and
//      rounding is monotone), and fl(dx*dx) >= dx^2 (1 - u) unless it underflows, in which case |dx| < 2^-511 and the two
//      coordinates, being float32, are equal.  dx itself is the difference of two float32 values rounded to float64 (exact
//      unless their exponents lie more than 29 apart), so the true |x1 - x2| <= |dx| (1 + u).  Together |x1 - x2| < radius (1 +
//      2^-51).
//  (b) The cell index is c(x) = floor(t(x)), t(x) = fl(x * inv_h), inv_h = fl(1 / fl(radius * RADIUS_CELL_MARGIN)): three
//      roundings, so t(x) = x / (radius (1 + m)) * (1 + e) with |e| < 2^-51.  In the domain (below) |t| < 2^30, so the absolute
//      error of t is below 2^30 * 2^-51 = 2^-21.
//  (c) Hence |t(x1) - t(x2)| < (1 + 2^-51) / (1 + m) + 2 * 2^-21 < 1 - 9.9e-5 + 9.6e-7 < 1, and two reals less than 1 apart
//      have floors at most 1 apart.
// A cell edge of exactly the radius (m = 0) leaves no room for (a) and (b): the bound of (c) becomes 1 + 2^-51 + 2^-20, and
// a pair a hair less than r apart whose quotients round to either side of two cell walls lies two cells apart.  The margin
// absorbs every rounding above 100 times over (as knn.hip.h's 0.99999 does there) and costs (1 + m)^3 - 1 = 0.03 % more
// candidates.
//
// Domain (the caller's contract: the entry cannot see device data; pegasus_amd/outliers.py checks it with one reduction):
// every coordinate finite with |x| / radius < 2^30.  Then |c| < 2^30 and c +- 1 fit an int32.  Outside it radius_cell() clamps
// the index to +-2^30, so the table and every index stay in bounds and only the counts are wrong.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr double RADIUS_CELL_MARGIN = 1.0001;      // cell edge / radius
constexpr double RADIUS_CELL_LIMIT = 1073741824.0; // 2^30: |cell index| of a point in the domain stays below it
constexpr uint32_t RADIUS_KEY_BIAS = 0x40000001u;  // stored word = index + bias in 1 .. 2^31 + 1: never 0 (= empty)
constexpr int RADIUS_BLOCK = 256;

struct alignas(16) RadiusSlot {
    unsigned long long xy;                         // (biased y << 32) | biased x; 0: empty
    uint32_t z;                                    // biased z; 0: not claimed yet
    uint32_t count;                                // points in the cell
};
static_assert(sizeof(RadiusSlot) == 16, "RadiusSlot must be 16 B");

struct RadiusKey { unsigned long long xy; uint32_t z; uint32_t hash; };

__device__ __forceinline__ int radius_cell(float x, double inv_h) {
    const double t = floor((double)x * inv_h);
    return (int)fmin(fmax(t, -RADIUS_CELL_LIMIT), RADIUS_CELL_LIMIT);      // (fmax drops a NaN)
}

__device__ __forceinline__ RadiusKey radius_key(int cx, int cy, int cz) {
    const uint32_t ux = (uint32_t)cx + RADIUS_KEY_BIAS, uy = (uint32_t)cy + RADIUS_KEY_BIAS, uz = (uint32_t)cz + RADIUS_KEY_BIAS;
    uint32_t h = ux * 0x9E3779B1u ^ uy * 0x85EBCA77u ^ uz * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return RadiusKey{((unsigned long long)uy << 32) | ux, uz, h};
}

// the rule's test, with every product and sum rounded on its own
__device__ __forceinline__ bool radius_within(float4 p, float4 q, double r2) {
#pragma clang fp contract(off)
    const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y, dz = (double)q.z - (double)p.z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz < r2;
}

// slots: `mask + 1` of them (a power of two, at least 2 n), zeroed.  point_slot[i]: the slot of point i's cell.
__global__ __launch_bounds__(RADIUS_BLOCK) void radius_insert_kernel(int n, const float* __restrict__ xyz, double inv_h,
                                                                     RadiusSlot* __restrict__ slots, uint32_t mask,
                                                                     uint32_t* __restrict__ point_slot) {
    const int64_t i = (int64_t)blockIdx.x * RADIUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const RadiusKey k = radius_key(radius_cell(xyz[3 * i], inv_h), radius_cell(xyz[3 * i + 1], inv_h),
                                   radius_cell(xyz[3 * i + 2], inv_h));
    uint32_t s = k.hash & mask;
    // at most half the slots are ever claimed, so an empty one turns up; the bound only keeps the loop finite regardless
    for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {
        const unsigned long long was_xy = atomicCAS(&slots[s].xy, 0ull, k.xy);
        if (was_xy != 0ull && was_xy != k.xy) continue;
        const uint32_t was_z = atomicCAS(&slots[s].z, 0u, k.z);
        if (was_z == 0u || was_z == k.z) break;
    }
    atomicAdd(&slots[s].count, 1u);
    point_slot[i] = s;
}

// begin[s] = where cell s's range starts in `sorted`; the grid covers the slots exactly (their number is a multiple of the block)
__global__ __launch_bounds__(RADIUS_BLOCK) void radius_ranges_kernel(const RadiusSlot* __restrict__ slots,
                                                                     uint32_t* __restrict__ begin, uint32_t* __restrict__ total) {
    const size_t s = (size_t)blockIdx.x * RADIUS_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t v = slots[s].count;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += t;
    }
    uint32_t base = 0;
    if (lane == WAVE - 1 && incl) base = atomicAdd(total, incl);
    base = __shfl(base, WAVE - 1, WAVE);
    begin[s] = base + incl - v;
}

__global__ __launch_bounds__(RADIUS_BLOCK) void radius_scatter_kernel(int n, const float* __restrict__ xyz,
                                                                      const uint32_t* __restrict__ point_slot,
                                                                      uint32_t* __restrict__ begin, float4* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * RADIUS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = atomicAdd(&begin[point_slot[i]], 1u);
    if (at < (uint32_t)n)                                        // (always: the counts sum to n)
        sorted[at] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
}

// one lane per point, in cell order.  `end`: the scatter's cursors, each now one past its cell's last point.
__global__ __launch_bounds__(RADIUS_BLOCK) void radius_count_kernel(int n, const float4* __restrict__ sorted,
                                                                    const RadiusSlot* __restrict__ slots,
                                                                    const uint32_t* __restrict__ end, uint32_t mask, double inv_h,
                                                                    double r2, int cap, int32_t* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * RADIUS_BLOCK + threadIdx.x;
    if (s >= n) return;
    const float4 p = sorted[s];
    const int cx = radius_cell(p.x, inv_h), cy = radius_cell(p.y, inv_h), cz = radius_cell(p.z, inv_h);
    int count = 0;
    for (int turn = 0; turn < 27 && count < cap; ++turn) {
        const int c = (turn + 13) % 27;                          // the point's own cell first: most hits, soonest at the cap
        const RadiusKey k = radius_key(cx + c % 3 - 1, cy + c / 3 % 3 - 1, cz + c / 9 - 1);
        uint32_t at = k.hash & mask;
        uint32_t cell_count = 0;                                 // 0: no such cell
        for (uint32_t probes = 0; probes <= mask; ++probes, at = (at + 1) & mask) {
            const RadiusSlot slot = slots[at];
            if (slot.xy == 0ull) break;
            if (slot.xy == k.xy && slot.z == k.z) { cell_count = slot.count; break; }
        }
        if (cell_count == 0) continue;
        const uint32_t last = min(end[at], (uint32_t)n);         // (never more than n: the counts sum to n)
        for (uint32_t j = last - min(cell_count, last); j < last && count < cap; ++j)
            count += radius_within(p, sorted[j], r2) ? 1 : 0;
    }
    const int orig = __float_as_int(p.w);
    if ((uint32_t)orig < (uint32_t)n) counts[orig] = count;
}

}  // namespace pgr
