// tilebin.hip.h -- sync-free tile binning for gfx950: (Gaussian, tile) instances -> per-tile lists, unsorted.
// Replaces SURVEY.md section 8a rows a6-a7 (scan, emission) of the reference design with a layout that never leaves the
// chip's fast paths; the lists are sorted by tilesort.hip.h (rows a8-a9).  Only instances that can reach alpha >= 1/255
// somewhere in their tile are listed (tile_may_contribute below): the images are unchanged, the lists are ~1.7x shorter.
//
//   bin_count    one workgroup per CHUNK of Gaussians: tile histogram in LDS (LDS atomics), then ONE
//                coalesced global atomicAdd per (chunk, touched tile) that both accumulates the tile
//                total and RESERVES the chunk's slice of the tile's list (returned offset -> rel[][]).
//                Scattered per-instance global atomics measured 9 G/s on MI355X (700 us per view);
//                this form measured 16 us (scripts/microbench/atomics_bin.hip).
//   tile_scan    exclusive scan of the tile totals -> ranges[tile] = [start,end), instance total,
//                overflow flag -- all on the device, no host round trip.
//   bin_scatter  same chunks: LDS cursors = range start + rel; every instance takes its slot with an
//                LDS atomic and stores (depth bits, index) = 8 B.
//
// Everything is integer/bit work: bit-exact against the oracle's lists.
#pragma once
#include <type_traits>

#include "composite.hip.h"       // work-order constants only: tile_scan_kernel counts the compositor's work-order bins
                                 // (ORDER_BINS, xcd_of_tile, coarse_class); the sort's tier table is pgr_common.h's
#include "cull.hip.h"
#include "pgr_common.h"

namespace pgr {

constexpr int BIN_CHUNK = 4096;        // Gaussians per binning workgroup
#ifndef PGR_BIN_THREADS
#define PGR_BIN_THREADS 512     // 8 waves share a chunk's 64 groups by ticket; 37 KiB of LDS at 2500 tiles = four per CU
#endif                           // (measured: 1024 threads +5 % in the count walk, 768 and 256 +8..10 %)
constexpr int BIN_THREADS = PGR_BIN_THREADS;
constexpr int BIN_LDS_TILES = 16384;   // tiles histogrammed per LDS pass (64 KiB)

// rect packed as 4 x uint16: minx, miny, maxx, maxy (exclusive); all zero = culled
__device__ __forceinline__ uint2 pack_rect(int minx, int miny, int maxx, int maxy) {
    return make_uint2((uint32_t)minx | ((uint32_t)miny << 16), (uint32_t)maxx | ((uint32_t)maxy << 16));
}

struct BinView {                 // per-view pointers used by the binning kernels (device table)
    const uint2* rects;          // [n] packed CANDIDATE tile rectangles (preprocess.hip.h candidate_rect)
    const float4* splats;        // [n, 3] records (preprocess.hip.h): q0 = (x,y,A,B), q1 = (C,op,B/C,B/A), q2 = (r,g,b,depth)
    uint32_t* tile_count;        // [tiles] zero-filled before bin_count
    uint32_t* rel;               // [chunks, tiles]
    uint2* ranges;               // [tiles]
    uint32_t* counters;          // [0] total instances, [1] overflow flag
    uint2* bucket;               // [max_instances] (depth bits, index), unsorted per tile
    uint32_t* gauss_sorted;      // [max_instances]
    uint64_t* alt;               // [max_instances] second key buffer for lists beyond the LDS tiers
    uint32_t* obj_last;          // [tiles] zero-filled; 1 + position of the last object entry of the sorted list
    int32_t n_env;               // Gaussians < n_env are environment; < 0: no semantic pass wanted
    // Exact depth ties are broken by tie_index[i] instead of the position i (PgrScene::tie_index: a scene stored in
    // another order than the caller's keeps the caller's tie order).  Lists are sorted by (depth, position) as always;
    // the bucket sort then looks the tie index up for the few keys that share their depth with another key of the
    // list and corrects their ranks; the merge-sort fallback (piled-up depths) sorts (depth, tie index) keys and maps
    // them back to positions through tie_inv.  NULL = the position is the tie index.
    const int32_t* tie_index;
    const uint32_t* tie_inv;
    // What the count walk found, kept for the scatter walk (see bin_kernel): a fixed region per 64-Gaussian group (its 64
    // depths + one ballot per window of candidates), in the space the sort only needs AFTER the scatter walk (alt +
    // gauss_sorted).
    uint2* records;
};


// one DPP step on a 32-bit word: CTRL = the control word (an immediate), lanes that read from outside get 0
template <int CTRL, int ROW_MASK = 0xF, bool BOUND_CTRL = true>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, BOUND_CTRL);
}

// inclusive prefix sum over the 64 lanes of a wave (row shifts, then the two row broadcasts of gfx9)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += dpp_u32<0x111>(v);               // row_shr:1
    v += dpp_u32<0x112>(v);               // row_shr:2
    v += dpp_u32<0x114>(v);               // row_shr:4
    v += dpp_u32<0x118>(v);               // row_shr:8
    v += dpp_u32<0x142, 0xA, false>(v);   // row_bcast:15 -> rows 1, 3
    v += dpp_u32<0x143, 0xC, false>(v);   // row_bcast:31 -> rows 2, 3
    return v;
}

// inclusive prefix MAX over the 64 lanes (0 is the identity: out-of-row DPP reads return 0)
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v) {
    v = max(v, dpp_u32<0x111>(v));
    v = max(v, dpp_u32<0x112>(v));
    v = max(v, dpp_u32<0x114>(v));
    v = max(v, dpp_u32<0x118>(v));
    v = max(v, dpp_u32<0x142, 0xA, false>(v));
    v = max(v, dpp_u32<0x143, 0xC, false>(v));
    return v;
}

// Both binning passes walk the same candidate space: every tile of every Gaussian's rectangle.  Rectangle
// areas vary from 1 to hundreds of tiles, so a loop per Gaussian leaves most lanes idle (measured 6x on
// MI355X).  Instead each wave takes 64 Gaussians, prefix-sums their areas (DPP scan), and its lanes sweep the
// FLATTENED candidate index space 64 at a time; every lane evaluates exactly one candidate per iteration.
//   candidate c -> owning Gaussian: every owner whose segment starts inside the 64-candidate window drops a head
//     flag (position << 6 | lane) at its start; a DPP prefix-max hands every candidate the last head at or before
//     it (candidates before the first head continue the previous window's owner).  ~14 VALU per iteration where a
//     binary search over the prefix with ds_bpermute took 6 LDS round trips.
//   owner's data (cull record, rectangle, depth bits): parked once per 64 Gaussians in a per-wave LDS table of
//     three float4 and fetched with three ds_read_b128 -- not 12 ds_bpermute per iteration.
//   tile inside the rectangle: k / w by a reciprocal multiply with an exact +-1 correction, no integer division.
// The binning kernels were VALU-bound (SQ_ACTIVE_INST_VALU ~ duration): these three cut the instruction count per
// iteration from ~180 to ~85.
//   SCATTER = false: lds[] = tile histogram; flushed with one coalesced reserving atomic per touched tile.
//   SCATTER = true : lds[] = write cursors (range start + this chunk's reserved offset).
// The count walk leaves what it found behind, ONE BIT PER CANDIDATE: per window of a group's walk the ballot of the
// predicate (8 bytes per 64 candidates, ~1 MB per view), in front of them the group's 64 depths (256 contiguous bytes
// instead of 64 words at a 48-byte stride).  Every 64-Gaussian group owns a fixed 768-byte region (64 depths + 62 ballots:
// up to 3 968 candidates; a group with more is simply evaluated twice as before), so there is nothing to reserve and
// nothing to look up: region = group index x 768 B, in the space the sort only needs after the scatter walk (alt +
// gauss_sorted).  The scatter walk then repeats the candidate enumeration -- same groups, same windows -- but takes the
// verdict from the bit instead of evaluating the predicate again, skips windows without a set bit, and reads neither the
// splat records nor their strided depths.
constexpr int BIN_STAGE_WORDS = WAVE * 12 + WAVE;         // per wave: 64 x 3 float4 + 64 head words
// One- and two-view calls launch 488 workgroups (C3) on 256 CUs and last as long as their heaviest chunk (7x the mean number
// of candidates in a C3 view): 16 waves per chunk instead of 8 -- count walk 44.7 -> 33.1 us, scatter walk 58.4 -> 51.1 us
// for a single view.  (Several workgroups per chunk, each with its own `rel` row: the scatter walk gains what the count
// walk loses to the extra zero-fills and flushes of 2 500 tile counters -- 2 parts 43 / 45 us, 4 parts 55 / 38: dropped.)
constexpr int BIN_THREADS_SMALL = 1024;
// tiles: tiles histogrammed per LDS pass (all of them up to BIN_LDS_TILES; a LAYERED call: the tiles of ONE layer)
__host__ __device__ inline size_t bin_lds_bytes(int tiles, int threads) {
    return ((size_t)(tiles < BIN_LDS_TILES ? tiles : BIN_LDS_TILES) + 3) / 4 * 16 + (size_t)(threads / WAVE) * BIN_STAGE_WORDS * 4 + 16;
}

// LAYERED binning (PgrForwardCall::layers): the view is one tall image of n_layers x layer_rows tile rows, `tiles` =
// n_layers x layer_tiles.  Gaussians are ordered by layer, so a chunk of 4096 holds one layer (two at a boundary): the
// chunk histograms ONE layer per LDS pass -- lo = (layer - 1) x layer_tiles, span = layer_tiles -- over the layers its
// first and last Gaussian name; a 64-Gaussian group takes part in the passes of the layers it holds, and a group that
// straddles a boundary keeps no verdict bits (its region would be written once per pass).
struct BinLayers {
    const int32_t* layer_id;     // [n] non-decreasing; NULL = not layered
    int32_t layer_tiles;         // grid_x * grid_y of one layer
    int32_t layer_rows;          // grid_y of one layer
    int32_t n_layers;
};
constexpr uint32_t VERDICT_WINDOWS = 62;                               // ballots per group region
constexpr uint32_t VERDICT_REGION_WORDS = 192;                         // 4-byte words: 64 depths + 2 x 62 (+ 4 unused)

// vis: blockcull.hip.h's visibility words (NULL = all visible); a 64-Gaussian group whose bit is clear has no rectangle
// to read (the preprocess did not write one).
//
// The 64 groups of a chunk are handed out to the waves one at a time (an LDS ticket): walks last from nothing to dozens
// of iterations, and a static split left most waves of a workgroup waiting for its slowest one.  A group's rectangles and
// records are fetched with all loads in flight at once (a visible group's Gaussians are nearly all visible, so the
// records do not wait for the rectangle).
//
// verdict_groups: how many groups have a region (0: none -- more tiles than one LDS pass holds, or PGR_BIN_RECORDS=0).
template <bool SCATTER, int THREADS>
__global__ __launch_bounds__(THREADS) void bin_kernel(const BinView* __restrict__ views, int n, int grid_x,
                                                          int tiles, int W, int H, const uint32_t* __restrict__ vis,
                                                          int vis_words, int verdict_groups,
                                                          BinLayers layers = BinLayers{nullptr, 0, 0, 0}) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr int BIN_WAVES = THREADS / WAVE;
    const BinView& bv = views[blockIdx.y];
    if (SCATTER && gload(bv.counters + 1)) return;   // overflow: reported by the host, nothing may be written past the buffers
    const int chunk = blockIdx.x;
    const int begin = chunk * BIN_CHUNK, end = min(n, begin + BIN_CHUNK);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const bool layered = layers.layer_id != nullptr;
    const int hist_words = (min(layered ? layers.layer_tiles : tiles, BIN_LDS_TILES) + 3) / 4 * 4;
    float4* const stage = reinterpret_cast<float4*>(lds + hist_words + wave * BIN_STAGE_WORDS);   // [64][3]
    // lanes talk to each other through this array inside one wave: DS operations of a wave execute in order, and a
    // compiler memory barrier keeps the load behind the stores.  (NOT volatile: a volatile generic pointer turns the
    // three accesses into flat_store/flat_load ... sc0 sc1 with a vmcnt(0) wait each.)
    uint32_t* const heads = reinterpret_cast<uint32_t*>(stage + WAVE * 3);                           // [64]
    // ctrl[0] = next ticket, ctrl[1..2] = visibility bits of the chunk's groups (fetched once, ahead of the walk)
    uint32_t* const ctrl = lds + hist_words + BIN_WAVES * BIN_STAGE_WORDS;
    constexpr int GROUPS = BIN_CHUNK / WAVE;
    static_assert(GROUPS == WAVE, "one visibility bit per lane of a wave");
    // LDS passes: windows of BIN_LDS_TILES tiles, or (layered) the layers this chunk's Gaussians belong to
    int pass_first = 0, pass_last = (tiles - 1) / BIN_LDS_TILES;
    if (layered) {
        if (begin >= end) return;
        pass_first = max(1, min(layers.n_layers + 1, (int)gload(layers.layer_id + begin)));
        pass_last = min(layers.n_layers, (int)gload(layers.layer_id + end - 1));
    }
    for (int lp = pass_first; lp <= pass_last; ++lp) {
        const int lo = layered ? (lp - 1) * layers.layer_tiles : lp * BIN_LDS_TILES;
        const int span = layered ? layers.layer_tiles : min(BIN_LDS_TILES, tiles - lo);
        const int row_off = layered ? (lp - 1) * layers.layer_rows : 0;     // tile row of the layer's first row
        for (int t = threadIdx.x; t < span; t += THREADS)
            lds[t] = SCATTER ? gload(bv.ranges + lo + t).x + gload(bv.rel + (size_t)chunk * tiles + lo + t) : 0u;
        if (wave == 0) {
            const int b = begin + lane * WAVE;
            bool visible = b < end;
            if (visible && vis) visible = (vis[(size_t)(b / WAVE) * vis_words + (blockIdx.y >> 5)] >> (blockIdx.y & 31)) & 1u;
            const uint64_t m = __ballot(visible);
            if (lane == 0) { ctrl[0] = 0u; ctrl[1] = (uint32_t)m; ctrl[2] = (uint32_t)(m >> 32); }
        }
        __syncthreads();
        const uint64_t vis_bits = ((uint64_t)ctrl[2] << 32) | ctrl[1];
        // next visible group of the chunk, or GROUPS
        auto take_ticket = [&]() {
            for (;;) {
                uint32_t ticket = 0;
                if (lane == 0) ticket = atomicAdd(&ctrl[0], 1u);
                ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket);
                if (ticket >= (uint32_t)GROUPS || ((vis_bits >> ticket) & 1ull)) return ticket;
            }
        };
        for (uint32_t ticket = take_ticket(); ticket < (uint32_t)GROUPS; ticket = take_ticket()) {
            const int base = begin + (int)ticket * WAVE;
            bool has_region = base / WAVE < verdict_groups;
            if (layered) {                   // (scalar: the group's first and last layer)
                const int l0 = gload(layers.layer_id + base), l1 = gload(layers.layer_id + min(base + WAVE, end) - 1);
                if (lp < l0 || lp > l1) continue;
                has_region = has_region && l0 == l1;
            }
            uint32_t* const region = reinterpret_cast<uint32_t*>(bv.records) + (size_t)(base / WAVE) * VERDICT_REGION_WORDS;
            uint64_t* const ballots = reinterpret_cast<uint64_t*>(region + WAVE);
            const int i = base + lane;
            const int ic = i < end ? i : end - 1;
            uint2 r = gload(bv.rects + ic);
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            float depth = 0.0f;
            uint64_t my_ballot = 0;                  // scatter walk: lane l = the verdicts of window l
            if (SCATTER && has_region) {             // (requested before the candidate count says whether they were written)
                depth = __uint_as_float(gload(region + lane));
                if (lane < (int)VERDICT_WINDOWS) my_ballot = gload(ballots + lane);
            } else {
                q0 = gload(bv.splats + (size_t)ic * 3);
                q1 = gload(bv.splats + (size_t)ic * 3 + 1);
                if (SCATTER || has_region) depth = gload(reinterpret_cast<const float*>(bv.splats + (size_t)ic * 3 + 2) + 3);
            }
            if (i >= end) r = make_uint2(0u, 0u);
            const int w = (int)(r.y & 0xffff) - (int)(r.x & 0xffff), h = (int)(r.y >> 16) - (int)(r.x >> 16);
            const uint32_t area = (w > 0 && h > 0) ? (uint32_t)(w * h) : 0u;
            const uint32_t incl = wave_inclusive_scan(area);
            const uint32_t excl = incl - area;
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
            const bool bits = has_region && total <= VERDICT_WINDOWS * (uint32_t)WAVE;   // same verdict in both walks
            if (SCATTER && has_region && !bits) {
                q0 = gload(bv.splats + (size_t)ic * 3);
                q1 = gload(bv.splats + (size_t)ic * 3 + 1);
                depth = gload(reinterpret_cast<const float*>(bv.splats + (size_t)ic * 3 + 2) + 3);
            }
            // one group's walk, compiled per combination of FROM_BITS (scatter walk: verdicts are read) and WRITE_BITS
            // (count walk: verdicts are kept): the loop bodies are free of mode branches (one body with run-time flags:
            // scatter walk 22.5 -> 27 us)
            auto walk = [&](auto from_bits_c, auto write_bits_c) {
                constexpr bool FROM_BITS = decltype(from_bits_c)::value, WRITE_BITS = decltype(write_bits_c)::value;
                float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0;
                if (area) {
                    uint32_t flags = 0;
                    if (!FROM_BITS) {
                        const CullSplat cs = make_cull_splat(make_float2(q0.x, q0.y), make_float4(q0.z, q0.w, q1.x, q1.y), q1.z, q1.w);
                        s0 = make_float4(cs.mx, cs.my, cs.A, cs.B);
                        s1 = make_float4(cs.C, cs.rBC, cs.rBA, cs.tau);
                        flags = cs.flags;
                    }
                    s2 = make_float4(__uint_as_float(flags | ((uint32_t)w << 2)), __uint_as_float(r.x), 1.0f / (float)w, depth);
                }
                if (!FROM_BITS) { stage[lane * 3 + 0] = s0; stage[lane * 3 + 1] = s1; }
                stage[lane * 3 + 2] = s2;
                __builtin_amdgcn_wave_barrier();
                if (WRITE_BITS && total) gstore(region + lane, __float_as_uint(depth));
                uint32_t carry_key = 0;        // owner of the candidate just before the window: (start + 1) << 6 | lane
                uint32_t it = 0;
                for (uint32_t c0 = 0; c0 < total; c0 += WAVE, ++it) {
                    uint64_t verdicts = ~0ull;
                    if (FROM_BITS) {
                        const uint32_t vlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)my_ballot, (int)it);
                        const uint32_t vhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(my_ballot >> 32), (int)it);
                        verdicts = ((uint64_t)vhi << 32) | vlo;
                    }
                    heads[lane] = 0u;
                    asm volatile("" ::: "memory");
                    if (area && excl - c0 < (uint32_t)WAVE) heads[excl - c0] = ((excl + 1u) << 6) | (uint32_t)lane;
                    asm volatile("" ::: "memory");
                    uint32_t key = wave_inclusive_max(heads[lane]);     // same wave: LDS ops are ordered
                    asm volatile("" ::: "memory");
                    key = key ? key : carry_key;
                    carry_key = (uint32_t)__builtin_amdgcn_readlane((int)key, WAVE - 1);
                    if (FROM_BITS && verdicts == 0ull) continue;          // nothing of this window is listed
                    const uint32_t c = c0 + (uint32_t)lane;
                    const int g = (int)(key & 63u);
                    const uint32_t k = c - ((key >> 6) - 1u);
                    const float4 o2 = stage[g * 3 + 2];
                    const uint32_t fw = __float_as_uint(o2.x), rlo = __float_as_uint(o2.y);
                    const int ow = (int)(fw >> 2);
                    // ty = k / w: reciprocal estimate, then an exact +-1 correction
                    int ty = (int)(((float)k + 0.5f) * o2.z);
                    int tx = (int)k - ty * ow;
                    if (tx < 0) { --ty; tx += ow; } else if (tx >= ow) { ++ty; tx -= ow; }
                    const int x = (int)(rlo & 0xffff) + tx, y = (int)(rlo >> 16) + ty;
                    const int t = y * grid_x + x - lo;
                    bool pass = c < total && (unsigned)t < (unsigned)span;
                    if (FROM_BITS) {
                        pass = pass && ((verdicts >> lane) & 1ull);
                    } else if (pass) {
                        const float4 o0 = stage[g * 3 + 0], o1 = stage[g * 3 + 1];
                        CullSplat cs;
                        cs.mx = o0.x; cs.my = o0.y; cs.A = o0.z; cs.B = o0.w;
                        cs.C = o1.x; cs.rBC = o1.y; cs.rBA = o1.z; cs.tau = o1.w; cs.flags = fw & 3u;
                        pass = tile_may_contribute(cs, x, y - row_off, W, H);
                    }
                    if (WRITE_BITS) {
                        const uint64_t m = __ballot(pass);
                        if (lane == 0) gstore(ballots + it, m);
                    }
                    if (pass) {
                        const uint32_t slot = atomicAdd(&lds[t], 1u);
                        if (SCATTER) gstore(bv.bucket + slot, make_uint2(__float_as_uint(o2.w), (uint32_t)(base + g)));
                    }
                }
            };
            if (SCATTER) {
                if (bits) walk(std::true_type{}, std::false_type{}); else walk(std::false_type{}, std::false_type{});
            } else {
                if (bits) walk(std::false_type{}, std::true_type{}); else walk(std::false_type{}, std::false_type{});
            }
        }
        __syncthreads();
        if (!SCATTER) {
            for (int t = threadIdx.x; t < span; t += THREADS) {
                const uint32_t cnt = lds[t];
                gstore(bv.rel + (size_t)chunk * tiles + lo + t, cnt ? gatomic_add(bv.tile_count + lo + t, cnt) : 0u);
            }
            __syncthreads();
        }
    }
}

// tie_inv[tie_index[i]] = i  (tie_index is a permutation; entries out of range are ignored)
__global__ void invert_tie_index_kernel(int n, const int32_t* __restrict__ tie_index, uint32_t* __restrict__ tie_inv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = tie_index[i];
    if ((unsigned)k < (unsigned)n) tie_inv[k] = (uint32_t)i;
}

// one workgroup per view.  The running total is kept in 64 bits: a view's instance count can pass 2^32 (millions of
// screen-filling splats x thousands of tiles), and a wrapped 32-bit sum could land below max_instances and let the
// scatter pass write through wrapped ranges.  Ranges are clamped to max_instances (no cursor can pass the buffers
// even if a later stage ignored the flag); counters[0] saturates at 0xffffffff.
//
// The same pass knows every list's length, so it also does what two small launches did until round 3 (order_count,
// order_scan): it counts the compositor's work items per (XCD stream, length class) into order_state, and the LAST
// workgroup to finish (agent-scope ticket behind a fence) turns the counts into the streams' write cursors.
__global__ __launch_bounds__(1024) void tile_scan_kernel(const BinView* __restrict__ views, int tiles,
                                                         uint32_t max_instances, int grid_x,
                                                         uint32_t* __restrict__ order_state, int skip_empty,
                                                         uint32_t* __restrict__ host_status) {
    __shared__ unsigned long long wave_tot[1024 / WAVE];
    __shared__ unsigned long long carry_s;
    __shared__ uint32_t hist[ORDER_BINS];
    __shared__ uint32_t last_s;
    const BinView& bv = views[blockIdx.x];
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    if (threadIdx.x == 0) carry_s = 0;
    if (threadIdx.x < ORDER_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int base = 0; base < tiles; base += 1024) {
        const int idx = base + threadIdx.x;
        const unsigned long long v = idx < tiles ? (unsigned long long)bv.tile_count[idx] : 0ull;
        unsigned long long s = v;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned long long t = __shfl_up(s, d, WAVE);
            if (lane >= d) s += t;
        }
        if (lane == WAVE - 1) wave_tot[wid] = s;
        __syncthreads();
        unsigned long long wave_prefix = 0;
        for (int w = 0; w < wid; ++w) wave_prefix += wave_tot[w];
        const unsigned long long carry = carry_s;
        const unsigned long long excl = carry + wave_prefix + s - v;
        const unsigned long long cap = max_instances;
        if (idx < tiles) {
            const uint2 r = make_uint2((uint32_t)min(excl, cap), (uint32_t)min(excl + v, cap));
            bv.ranges[idx] = r;
            // (a layered call gives empty lists no work item: their pixels are pre-filled, layer_mask_fill_kernel)
            if (order_state && !(skip_empty && r.y == r.x))
                atomicAdd(&hist[xcd_of_tile(idx, grid_x) * ORDER_CLASSES_USED + coarse_class(r.y - r.x)], ITEMS_PER_TILE);
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + wave_prefix + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t total = (uint32_t)min(carry_s, 0xffffffffull);
        const uint32_t over = carry_s > (unsigned long long)max_instances ? 1u : 0u;
        bv.counters[0] = total;
        bv.counters[1] = over;
        // early status (PgrForwardCall::status_event): the two words are FINAL here -- nothing after the scan changes them --
        // so they go straight to the caller's pinned host memory, and the event recorded behind this kernel lets the host
        // decide about an overflow while scatter, sort and compositor still run
        if (host_status) {
            host_status[2 * blockIdx.x] = total;
            host_status[2 * blockIdx.x + 1] = over;
            __threadfence_system();
        }
    }
    if (!order_state) return;
    if (gridDim.x == 1) {
        // one view, one workgroup: the counts are this workgroup's own LDS words -- no agent-scope atomics, ticket or fences
        // (two __threadfence() are ~7 us of the ~14 us this kernel takes in a single-view call, where every launch is latency)
        __syncthreads();
        if (threadIdx.x < NUM_XCD) {
            uint32_t acc = 0;
            for (int c = 0; c < ORDER_CLASSES_USED; ++c) {
                gstore(order_state + threadIdx.x * ORDER_CLASSES_USED + c, acc);
                acc += hist[threadIdx.x * ORDER_CLASSES_USED + c];
            }
        }
        return;
    }
    if (threadIdx.x < ORDER_BINS && hist[threadIdx.x]) gatomic_add(order_state + threadIdx.x, hist[threadIdx.x]);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last_s = gatomic_add(order_state + ORDER_DONE_WORD, 1u) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    if (threadIdx.x < NUM_XCD) {             // one thread per stream: exclusive prefix over the classes = write cursors
        uint32_t acc = 0;
        for (int c = 0; c < ORDER_CLASSES_USED; ++c) {
            const uint32_t v = gatomic_load(order_state + threadIdx.x * ORDER_CLASSES_USED + c);
            gstore(order_state + threadIdx.x * ORDER_CLASSES_USED + c, acc);
            acc += v;
        }
    }
}

}  // namespace pgr
