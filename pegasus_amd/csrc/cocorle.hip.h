// cocorle.hip.h -- COCO annotations of binary masks: run-length encoding, decoding and overlap counts (the BOP toolkit's
// bop_toolkit_lib/pycoco_utils.py: binary_mask_to_rle, rle_to_binary_mask, bbox_from_binary_mask, and the integer parts
// of compute_ious).  Everything here is an integer: tests/coco_reference.py restates it in NumPy and the results are equal.
//
// The rule (pycoco_utils.binary_mask_to_rle).  A mask is uint8 [H,W] row-major, a pixel is set when its byte is non-zero.
// Pixels are taken in COLUMN-major order, p = x H + y.  Runs alternate and start with a run of zeros: counts[0] is the
// number of zeros in front of the first set pixel (0 when pixel 0 is set).  With a virtual unset pixel in front of pixel 0,
// a TRANSITION is a pixel that differs from its predecessor, at positions t_0 < t_1 < ... < t_{T-1}, and
//     counts = [t_0, t_1 - t_0, ..., t_{T-1} - t_{T-2}, H W - t_{T-1}]           ([H W] when T = 0),  n_counts = T + 1.
// The predecessor of the top pixel of column x is the bottom pixel of column x - 1: a run goes through column ends.
//
// Encode, count pass (pgr_mask_rle_count), three launches:
//   rle_planes_kernel   reads the row-major bytes and writes BIT PLANES: word (k, s, x) holds rows 32 s .. 32 s + 31 of column
//                       x of mask k, bit r = pixel (x, 32 s + r) set, rows >= H clear.  A wave takes RLE_TILE_COLS = 256
//                       columns of RLE_WORD_ROWS = 32 rows: a lane owns 4 neighbouring columns, reads them as ONE dword per
//                       row (256 B per wave and instruction) and ORs each byte's verdict into its column's word -- no lane
//                       talks to another.  The 4 waves of a workgroup take 4 row segments (RLE_BLOCK_ROWS = 128).  Mask k
//                       starts at byte k H W and row y at y W, so a lane's dword is in general NOT 4-byte aligned: it is
//                       assembled from the two aligned dwords around it (rle_load4).  The 4 words of a lane are one 16-byte
//                       store (the plane's row pitch is W rounded up to 4 words).
//   rle_columns_kernel  one lane per column (lanes along x: every plane read is coalesced) walks its S = ceil(H / 32) words:
//                       transitions = (w ^ (w << 1 | carry)), the carry coming from the segment above or, for the top word,
//                       from the bottom pixel of column x - 1; per column the number of transitions, the set pixels, the
//                       first and last set row and the position of the last transition -- 16 bytes.
//   rle_scan_kernel     one workgroup per mask: exclusive sum of the columns' transition counts (where a column's counts
//                       start in the mask's slot) and exclusive max of the last transition (the position a column's first
//                       count is measured from), both written back over the column records; area, extents, n_counts to stats.
// Encode, emit pass (pgr_mask_rle_emit), one launch over the same workspace:
//   rle_emit_kernel     one lane per column again: every transition of the column becomes position - previous position at
//                       its index; the lane of the last column adds H W - last.  Every store is checked against the mask's
//                       slot [offsets[k], offsets[k+1]) and the capacity.
// No atomics anywhere in the encoder: two runs give equal bytes.
//
// Decode (pgr_mask_rle_decode).  A mask is cut into slices of whole pixel ranges in column-major order, one workgroup each.
// A workgroup walks the mask's counts 256 at a time, keeping the running sum; a chunk that reaches into its slice is
// scanned (run ends into LDS) and every pixel of the overlap finds its run by bisection: the value is the run's index & 1.
// Every pixel is written exactly once; pixels behind the last run (counts that sum to less than H W) are 0, runs beyond
// H W are cut (the host wrapper refuses both).  Zero-length runs are skipped by the bisection (first end > p).
//
// Overlap (pgr_mask_overlap).  inter[i,j] = number of pixels set in both a_i and b_j; one workgroup per (pair, pixel chunk),
// 4 pixels per lane and step through rle_load4, a wave reduction and one integer atomic add per wave.  The pairs of column
// j = 0 add area_a, those of row i = 0 area_b.
#pragma once
#include "pgr_common.h"

namespace pgr {

constexpr int RLE_WORD_ROWS = PGR_RLE_WORD_ROWS;      // rows per plane word
constexpr int RLE_TILE_COLS = PGR_RLE_TILE_COLS;      // columns per wave of the plane kernel: 64 lanes x 4 bytes
constexpr int RLE_BLOCK_ROWS = PGR_RLE_BLOCK_ROWS;    // rows per workgroup of the plane kernel: 4 waves x 32
constexpr int RLE_THREADS = 256;
constexpr int RLE_DECODE_CHUNK = PGR_RLE_DECODE_CHUNK;            // runs scanned at a time
constexpr int RLE_DECODE_MIN_SLICE = PGR_RLE_DECODE_MIN_SLICE;    // pixels per decode workgroup, at least
constexpr int RLE_DECODE_MAX_SLICES = PGR_RLE_DECODE_MAX_SLICES;  // workgroups per mask, at most
constexpr int OVERLAP_CHUNK = PGR_MASK_OVERLAP_CHUNK;             // pixels per overlap workgroup
static_assert(RLE_TILE_COLS == 4 * WAVE && RLE_BLOCK_ROWS == RLE_WORD_ROWS * (RLE_THREADS / WAVE) && RLE_WORD_ROWS == 32 &&
              RLE_DECODE_CHUNK == RLE_THREADS, "the kernels are written for these shapes");

struct RleColumn {           // 16 bytes per column: rle_columns_kernel writes, rle_scan_kernel rewrites `first` and `prev`
    int32_t first;           // transitions in the column -> index of the column's first count in the mask's slot
    int32_t area;            // set pixels in the column
    int32_t prev;            // position of the column's last transition (0: none) -> of the last transition before the column
    uint32_t rows;           // first set row | (last set row + 1) << 16;  0xFFFF | 0 << 16 when the column is empty
};

// 0x80 in every byte of v that is non-zero
__device__ __forceinline__ uint32_t rle_nonzero_bytes(uint32_t v) {
    return (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
}

// Bytes p[0 .. n) (1 <= n <= 4) as the low bytes of a dword, the rest unspecified, for ANY alignment of p: only aligned
// dwords that hold at least one of the n bytes are read, so no read leaves the pages the n bytes lie in.
__device__ __forceinline__ uint32_t rle_load4(const uint8_t* p, int n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t shift = (uint32_t)(a & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - shift);
    const uint32_t lo = gload(q);
    if (shift == 0) return lo;
    uint32_t hi = 0;
    if (shift + (uint32_t)n > 4u) hi = gload(q + 1);
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
}

__global__ __launch_bounds__(RLE_THREADS) void rle_planes_kernel(const uint8_t* __restrict__ masks, int W, int H, int S, int Wp,
                                                                int col_tiles, int row_groups, uint32_t* __restrict__ planes) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint32_t per_mask = (uint32_t)col_tiles * (uint32_t)row_groups;
    const uint32_t k = blockIdx.x / per_mask, rem = blockIdx.x % per_mask;
    const int s = (int)(rem / (uint32_t)col_tiles) * (RLE_THREADS / WAVE) + wave;
    const int x = (int)(rem % (uint32_t)col_tiles) * RLE_TILE_COLS + 4 * lane;
    if (s >= S || x >= Wp) return;
    const int n = min(4, W - x);                                         // >= 1: Wp - W < 4 and x is a multiple of 4
    const uint32_t keep = n == 4 ? 0x80808080u : (0x80808080u >> (8 * (4 - n)));
    const int y0 = s * RLE_WORD_ROWS, rows = min(RLE_WORD_ROWS, H - y0);
    const uint8_t* p = masks + (size_t)k * (size_t)W * (size_t)H + (size_t)y0 * (size_t)W + (size_t)x;
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
        const uint32_t t = rle_nonzero_bytes(rle_load4(p, n)) & keep;
        w0 |= ((t >> 7) & 1u) << r;
        w1 |= ((t >> 15) & 1u) << r;
        w2 |= ((t >> 23) & 1u) << r;
        w3 |= (t >> 31) << r;
        p += W;
    }
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(planes + ((size_t)k * (size_t)S + (size_t)s) * (size_t)Wp + (size_t)x);
    *(PGR_GLOBAL u32x4_t*)dst = u32x4_t{w0, w1, w2, w3};
}

// the transitions of word s of a column: bit r = pixel 32 s + r differs from its predecessor (`carry`: the predecessor of row 0)
__device__ __forceinline__ uint32_t rle_transitions(uint32_t w, uint32_t carry, int s, int S, int H) {
    const int tail = H & (RLE_WORD_ROWS - 1);
    const uint32_t valid = (s == S - 1 && tail) ? ((1u << tail) - 1u) : 0xFFFFFFFFu;
    return (w ^ ((w << 1) | carry)) & valid;
}

// the pixel above the top of column x: the bottom pixel of column x - 1, unset for column 0
__device__ __forceinline__ uint32_t rle_column_carry(const uint32_t* __restrict__ plane, int x, int S, int Wp, int H) {
    if (x == 0) return 0u;
    return (gload(plane + (size_t)(S - 1) * (size_t)Wp + (size_t)(x - 1)) >> ((H - 1) & (RLE_WORD_ROWS - 1))) & 1u;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_columns_kernel(const uint32_t* __restrict__ planes, int W, int H, int S, int Wp,
                                                                 int col_blocks, RleColumn* __restrict__ columns) {
    const uint32_t k = blockIdx.x / (uint32_t)col_blocks;
    const int x = (int)(blockIdx.x % (uint32_t)col_blocks) * RLE_THREADS + threadIdx.x;
    if (x >= W) return;
    const uint32_t* plane = planes + (size_t)k * (size_t)S * (size_t)Wp;
    uint32_t carry = rle_column_carry(plane, x, S, Wp, H);
    int32_t count = 0, area = 0, last = 0;
    uint32_t y_min = 0xFFFFu, y_end = 0u;
    for (int s = 0; s < S; ++s) {
        const uint32_t w = gload(plane + (size_t)s * (size_t)Wp + (size_t)x);
        const uint32_t t = rle_transitions(w, carry, s, S, H);
        carry = w >> 31;
        count += __popc(t);
        area += __popc(w);
        if (w) {
            y_min = min(y_min, (uint32_t)(s * RLE_WORD_ROWS + __ffs((int)w) - 1));
            y_end = (uint32_t)(s * RLE_WORD_ROWS + 32 - __clz((int)w));
        }
        if (t) last = x * H + s * RLE_WORD_ROWS + 31 - __clz((int)t);
    }
    columns[(size_t)k * (size_t)W + (size_t)x] = RleColumn{count, area, last, y_min | (y_end << 16)};
}

// inclusive scans over the RLE_THREADS values of a workgroup (every thread calls): shuffles in the wave, LDS across waves
template <typename T, typename Op>
__device__ __forceinline__ T rle_block_scan(T v, T identity, Op op, T* wave_totals) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T up = __shfl_up(v, d, WAVE);
        if (lane >= d) v = op(up, v);
    }
    __syncthreads();                                   // the totals of an earlier scan have been read
    if (lane == WAVE - 1) wave_totals[wave] = v;
    __syncthreads();
    T before = identity;
    for (int q = 0; q < wave; ++q) before = op(before, wave_totals[q]);
    return op(before, v);
}

__global__ __launch_bounds__(RLE_THREADS) void rle_scan_kernel(RleColumn* __restrict__ columns, int W, int H,
                                                              int32_t* __restrict__ stats) {
    __shared__ int32_t totals[RLE_THREADS / WAVE];
    __shared__ int32_t red[5][RLE_THREADS / WAVE];
    const size_t k = blockIdx.x;
    RleColumn* col = columns + k * (size_t)W;
    const int per = (W + RLE_THREADS - 1) / RLE_THREADS;
    const int x0 = min(W, (int)threadIdx.x * per), x1 = min(W, x0 + per);
    int32_t count = 0, area = 0, last = 0, x_min = INT32_MAX, x_max = INT32_MIN, y_min = INT32_MAX, y_max = INT32_MIN;
    for (int x = x0; x < x1; ++x) {
        const RleColumn c = col[x];
        count += c.first;
        last = max(last, c.prev);
        if (c.area) {
            area += c.area;
            x_min = min(x_min, x);
            x_max = x;
            y_min = min(y_min, (int32_t)(c.rows & 0xFFFFu));
            y_max = max(y_max, (int32_t)(c.rows >> 16) - 1);
        }
    }
    const auto add = [](int32_t a, int32_t b) { return a + b; };
    const auto mx = [](int32_t a, int32_t b) { return max(a, b); };
    const int32_t count_incl = rle_block_scan<int32_t>(count, 0, add, totals);
    const int32_t last_incl = rle_block_scan<int32_t>(last, 0, mx, totals);
    // a thread's first column starts behind everything of the threads in front of it
    int32_t first = count_incl - count;
    int32_t prev = __shfl_up(last_incl, 1, WAVE);
    {
        const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
        __syncthreads();
        if (lane == WAVE - 1) totals[wave] = last_incl;
        __syncthreads();
        if (lane == 0) prev = wave ? totals[wave - 1] : 0;
    }
    for (int x = x0; x < x1; ++x) {
        const RleColumn c = col[x];
        col[x].first = first;
        col[x].prev = prev;
        first += c.first;
        prev = max(prev, c.prev);
    }
    // area and extents: wave reductions, then the four waves through LDS
    int32_t v[5] = {area, x_min, y_min, x_max, y_max};
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int32_t o = __shfl_xor(v[q], d, WAVE);
            v[q] = q == 0 ? v[q] + o : (q < 3 ? min(v[q], o) : max(v[q], o));
        }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0)
        for (int q = 0; q < 5; ++q) red[q][threadIdx.x / WAVE] = v[q];
    __syncthreads();
    if (threadIdx.x == RLE_THREADS - 1) {
        int32_t r[5] = {red[0][0], red[1][0], red[2][0], red[3][0], red[4][0]};
        for (int w = 1; w < RLE_THREADS / WAVE; ++w) {
            r[0] += red[0][w];
            r[1] = min(r[1], red[1][w]); r[2] = min(r[2], red[2][w]);
            r[3] = max(r[3], red[3][w]); r[4] = max(r[4], red[4][w]);
        }
        int32_t* row = stats + k * 6;
        row[0] = count_incl + 1;                       // the last thread's inclusive sum: every transition of the mask
        row[1] = r[0]; row[2] = r[1]; row[3] = r[2]; row[4] = r[3]; row[5] = r[4];
    }
}

__global__ __launch_bounds__(RLE_THREADS) void rle_emit_kernel(const uint32_t* __restrict__ planes,
                                                              const RleColumn* __restrict__ columns, int W, int H, int S, int Wp,
                                                              int col_blocks, const long long* __restrict__ offsets,
                                                              int32_t* __restrict__ counts, long long capacity) {
    const uint32_t k = blockIdx.x / (uint32_t)col_blocks;
    const int x = (int)(blockIdx.x % (uint32_t)col_blocks) * RLE_THREADS + threadIdx.x;
    if (x >= W) return;
    const uint32_t* plane = planes + (size_t)k * (size_t)S * (size_t)Wp;
    const RleColumn c = columns[(size_t)k * (size_t)W + (size_t)x];
    const long long slot0 = offsets[k], slot1 = min(offsets[k + 1], capacity);
    if (slot0 < 0) return;
    long long at = slot0 + c.first;
    int32_t prev = c.prev;
    uint32_t carry = rle_column_carry(plane, x, S, Wp, H);
    for (int s = 0; s < S; ++s) {
        const uint32_t w = gload(plane + (size_t)s * (size_t)Wp + (size_t)x);
        uint32_t t = rle_transitions(w, carry, s, S, H);
        carry = w >> 31;
        while (t) {
            const int32_t p = x * H + s * RLE_WORD_ROWS + __ffs((int)t) - 1;
            t &= t - 1u;
            if (at >= slot0 && at < slot1) counts[at] = p - prev;
            ++at;
            prev = p;
        }
    }
    if (x == W - 1 && at >= slot0 && at < slot1) counts[at] = W * H - prev;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_decode_kernel(const int32_t* __restrict__ counts,
                                                                const long long* __restrict__ offsets, int W, int H,
                                                                int slices, int slice, uint8_t* __restrict__ masks) {
    __shared__ long long totals[RLE_THREADS / WAVE];
    __shared__ int32_t ends[RLE_DECODE_CHUNK];
    const size_t k = blockIdx.x / (uint32_t)slices;
    const int HW = W * H;
    const int lo = (int)(blockIdx.x % (uint32_t)slices) * slice, hi = min(HW, lo + slice);      // slices * slice < 2^31 (host)
    if (lo >= hi) return;
    uint8_t* out = masks + k * (size_t)HW;
    const long long o0 = offsets[k];
    const long long n = max(0ll, offsets[k + 1] - o0);
    long long base = 0;                                 // pixels in front of the chunk
    for (long long c0 = 0; c0 < n && base < hi; c0 += RLE_DECODE_CHUNK) {
        const long long j = c0 + threadIdx.x;
        const long long mine = j < n ? (long long)min(max(counts[o0 + j], 0), HW) : 0ll;
        const long long incl = rle_block_scan<long long>(mine, 0ll, [](long long a, long long b) { return a + b; }, totals);
        __syncthreads();                                // the pixels of the chunk before have been looked up
        ends[threadIdx.x] = (int32_t)min(base + incl, (long long)HW);
        __syncthreads();
        const int chunk_end = ends[RLE_DECODE_CHUNK - 1];
        const int p0 = max(lo, (int)min(base, (long long)HW)), p1 = min(hi, chunk_end);
        for (int p = p0 + (int)threadIdx.x; p < p1; p += RLE_THREADS) {
            int a = 0, b = RLE_DECODE_CHUNK - 1;        // the first run of the chunk that ends behind p
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (ends[mid] > p) b = mid; else a = mid + 1;
            }
            const int x = p / H, y = p - x * H;
            gstore(out + (size_t)y * (size_t)W + (size_t)x, (uint8_t)((c0 + a) & 1));
        }
        long long total = 0;                            // of all four waves, unclamped (the next scan syncs before it writes)
        for (int q = 0; q < RLE_THREADS / WAVE; ++q) total += totals[q];
        base += total;
    }
    const int tail = max(lo, (int)min(base, (long long)HW));
    for (int p = tail + (int)threadIdx.x; p < hi; p += RLE_THREADS) {
        const int x = p / H, y = p - x * H;
        gstore(out + (size_t)y * (size_t)W + (size_t)x, (uint8_t)0);
    }
}

__global__ __launch_bounds__(RLE_THREADS) void mask_overlap_kernel(const uint8_t* __restrict__ a, int n_a,
                                                                  const uint8_t* __restrict__ b, int n_b, size_t HW, int chunks,
                                                                  int32_t* __restrict__ inter, int32_t* __restrict__ area_a,
                                                                  int32_t* __restrict__ area_b) {
    const uint32_t pair = blockIdx.x / (uint32_t)chunks;
    const size_t q0 = (size_t)(blockIdx.x % (uint32_t)chunks) * OVERLAP_CHUNK, q1 = min(HW, q0 + OVERLAP_CHUNK);
    const int i = (int)(pair / (uint32_t)n_b), j = (int)(pair % (uint32_t)n_b);
    const uint8_t* pa = a + (size_t)i * HW;
    const uint8_t* pb = b + (size_t)j * HW;
    int32_t both = 0, in_a = 0, in_b = 0;
    for (size_t q = q0 + 4 * (size_t)threadIdx.x; q < q1; q += 4 * RLE_THREADS) {
        const int n = (int)min((size_t)4, q1 - q);
        const uint32_t keep = n == 4 ? 0x80808080u : (0x80808080u >> (8 * (4 - n)));
        const uint32_t ta = rle_nonzero_bytes(rle_load4(pa + q, n)) & keep;
        const uint32_t tb = rle_nonzero_bytes(rle_load4(pb + q, n)) & keep;
        both += __popc(ta & tb);
        in_a += __popc(ta);
        in_b += __popc(tb);
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        both += __shfl_xor(both, d, WAVE);
        in_a += __shfl_xor(in_a, d, WAVE);
        in_b += __shfl_xor(in_b, d, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (both) atomicAdd(inter + (size_t)i * (size_t)n_b + (size_t)j, both);
        if (j == 0 && in_a) atomicAdd(area_a + i, in_a);
        if (i == 0 && in_b) atomicAdd(area_b + j, in_b);
    }
}

}  // namespace pgr
