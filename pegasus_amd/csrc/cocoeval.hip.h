// cocoeval.hip.h -- COCO detection / segmentation scores (the BOP toolkit's scripts/eval_bop22_coco.py over
// pycocotools.COCOeval): IoU inside (image, category) groups straight from run lists or boxes, the greedy matching of
// evaluateImg, and the precision / recall tables of accumulate.
//
// pycocotools is not a requirement of this project and cannot be run where it is developed: parity with it is PINNED BY THE
// WRITTEN RULE BELOW AND BY HAND-WORKED KNOWN ANSWERS, NOT BY RECORDED OUTPUTS (DESIGN.md section 14;
// tests/coco_eval_reference.py restates the rule in NumPy and every result here is equal to it, floats bit for bit).
//
// The rule (COCOeval's, quirks included).
//   Groups.    One group per (image, category): its detections sorted by -score (stable) and cut to maxDets[-1], its GT in
//              file order.  The IoU matrix of a group is iou[iou_offset + d * gt_count + g], float64.
//   segm IoU.  inter = pixels set in both; union = area_d + area_g - inter, area_d alone when the GT is a crowd;
//              iou = inter / union as ONE float64 division of exact integers, and 0 when inter == 0 (the empty union too).
//   bbox IoU.  [x,y,w,h] float64: iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise; inter = iw*ih if both > 0, else 0;
//              union = dw*dh + gw*gh - inter, dw*dh for a crowd; iou = 0 when inter == 0, else inter / union.  Every operation
//              is one IEEE operation in that order: no contraction into FMAs (the pragma below).  pycocotools divides 0/0
//              for two zero-area boxes; here that is 0.
//   Matching.  Per area range [lo, hi] and threshold t: GT _ignore = flag or area < lo or area > hi; the GT are walked in the
//              stable order "not ignored first".  Detections in score order: best = min(t, 1 - 1e-10), m = -1; for each GT:
//              skip one already matched at t unless it is a crowd; break if m > -1, GT m is not ignored and this one is; skip
//              if iou < best; else best = iou, m = this GT.  A matched detection takes the ignore flag of its GT; an
//              unmatched one is ignored when its area is outside [lo, hi].
//   Accumulate. Per (category k, area range a, maxDet m): the detections of k with in-image rank < m in the global stable
//              order by -score; npig = GT of k not ignored for a.  tp = cumsum(matched & ~ignored), fp = cumsum(~matched &
//              ~ignored); rc = tp / npig; pr = tp / (fp + tp + 2^-52); recall = rc[-1] (0 without detections); pr made
//              non-increasing from the right; for each recall threshold r, i = the first index with rc[i] >= r:
//              precision = pr[i], scores = score[i], both 0 when there is none.  Everything is -1 where npig == 0.
//
// Kernels.
//   coco_rle_prefix_kernel   one workgroup per mask: its counts, 256 at a time with a carry, become run END positions (cut at
//                            H W, negative counts read as 0, as pgr_mask_rle_decode) and the number of set pixels in front
//                            of each end (`cover`); the last cover is the mask's area.
//   coco_rle_iou_kernel      one workgroup per group, one wave per (detection, GT) pair in turn, one lane per set run [s, e)
//                            of the detection: inter = sum of cover_g(e) - cover_g(s), cover_g(p) by bisection in the GT's
//                            run ends (the first run that ends behind p: zero-length runs are skipped, as the decode kernel
//                            does).  A group's GT ends and covers are staged in LDS when they fit (COCO_LDS_RUNS) and read
//                            from the workspace when they do not.  Integers, a wave reduction by shuffles, one division.
//   coco_box_iou_kernel      one workgroup per group, one thread per pair in turn.
//   coco_match_kernel        one wave per group, one lane per (area range, threshold).  The ignore-sorted GT orders (one per
//                            area range) are built once per group by ballots into the workspace.  A lane's "GT matched" state
//                            IS its row of the gt_match output, cleared to -1 first: any gt_count works and nothing is
//                            staged.  The IoU element is the same address for the lanes of one area range.
//   coco_accumulate_kernel   one workgroup per (k, a, m), looping over t: a chunked scan with carry selects the ranks < m and
//                            sums tp | fp (one 64-bit scan), compacting tp, pr and the detection index into the workgroup's
//                            workspace slice; a second chunked scan from the right takes the running maximum of pr; then one
//                            bisection per recall threshold.  Every output cell is written once.
// No atomics anywhere: two runs give equal bytes.
#pragma once
#include "cocorle.hip.h"
#include "pgr_common.h"

#pragma clang fp contract(off)

namespace pgr {

constexpr int COCO_THREADS = 256;
constexpr int COCO_CHUNK = PGR_COCO_CHUNK;          // elements a workgroup scans at a time
constexpr int COCO_LDS_RUNS = PGR_COCO_LDS_RUNS;    // GT runs of a group staged in LDS, at most
constexpr int COCO_MAX_LANES = PGR_COCO_MAX_LANES;  // area ranges x thresholds of one matching call
static_assert(COCO_CHUNK == COCO_THREADS && COCO_CHUNK == RLE_THREADS && COCO_MAX_LANES == WAVE, "written for these shapes");

struct CocoMatchParams {
    double thr[COCO_MAX_LANES];          // per lane: min(t, 1 - 1e-10)
    double lo[COCO_MAX_LANES], hi[COCO_MAX_LANES];
    int32_t n_thr, n_area;
};

// [o0, o1) of mask k, cut to [0, total]
__device__ __forceinline__ void coco_slot(const long long* __restrict__ offsets, long long k, long long total, long long* o0,
                                          long long* o1) {
    const long long a = min(max(offsets[k], 0ll), total);
    *o0 = a;
    *o1 = min(max(offsets[k + 1], a), total);
}

__global__ __launch_bounds__(COCO_THREADS) void coco_rle_prefix_kernel(const int32_t* __restrict__ counts,
                                                                      const long long* __restrict__ offsets, long long total,
                                                                      int HW, int32_t* __restrict__ ends,
                                                                      int32_t* __restrict__ cover, long long* __restrict__ area) {
    __shared__ long long totals[COCO_THREADS / WAVE];
    const long long k = blockIdx.x;
    long long o0, o1;
    coco_slot(offsets, k, total, &o0, &o1);
    const long long n = o1 - o0;
    const auto add = [](long long a, long long b) { return a + b; };
    long long base = 0, set = 0;                        // pixels / set pixels in front of the chunk (unclamped / clamped)
    for (long long c0 = 0; c0 < n; c0 += COCO_CHUNK) {
        const long long j = c0 + threadIdx.x;
        const long long mine = j < n ? (long long)min(max(counts[o0 + j], 0), HW) : 0ll;
        const long long incl = base + rle_block_scan<long long>(mine, 0ll, add, totals);
        const long long e1 = min(incl, (long long)HW), e0 = min(incl - mine, (long long)HW);
        long long chunk = 0;
        for (int q = 0; q < COCO_THREADS / WAVE; ++q) chunk += totals[q];
        const long long len = (j & 1) ? e1 - e0 : 0ll;     // runs alternate and start with zeros: the odd ones are set
        const long long cov = set + rle_block_scan<long long>(len, 0ll, add, totals);
        if (j < n) {
            ends[o0 + j] = (int32_t)e1;
            cover[o0 + j] = (int32_t)cov;
        }
        long long chunk_set = 0;
        for (int q = 0; q < COCO_THREADS / WAVE; ++q) chunk_set += totals[q];
        base += chunk;
        set += chunk_set;
    }
    if (threadIdx.x == 0) area[k] = set;
}

// set pixels of a mask in front of pixel p; `ends` / `cover` are the mask's n runs (LDS or global)
__device__ __forceinline__ int32_t coco_cover(const int32_t* ends, const int32_t* cover, int n, int32_t p) {
    if (n <= 0) return 0;
    if (ends[n - 1] <= p) return cover[n - 1];
    int a = 0, b = n - 1;                                  // the first run that ends behind p
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (ends[mid] > p) b = mid; else a = mid + 1;
    }
    const int32_t before = a ? cover[a - 1] : 0, start = a ? ends[a - 1] : 0;
    return before + ((a & 1) ? p - start : 0);
}

__global__ __launch_bounds__(COCO_THREADS) void coco_rle_iou_kernel(
    const PgrCocoGroup* __restrict__ groups, const long long* __restrict__ dt_offsets, long long dt_total,
    const long long* __restrict__ gt_offsets, long long gt_total, const uint8_t* __restrict__ gt_crowd,
    const int32_t* __restrict__ dt_ends, const int32_t* __restrict__ gt_ends, const int32_t* __restrict__ gt_cover,
    const long long* __restrict__ dt_area, const long long* __restrict__ gt_area, long long* __restrict__ inter,
    double* __restrict__ iou) {
    __shared__ int32_t s_ends[COCO_LDS_RUNS], s_cover[COCO_LDS_RUNS];
    const PgrCocoGroup G = groups[blockIdx.x];
    if (G.dt_count <= 0 || G.gt_count <= 0) return;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    long long g0, g1, unused;
    coco_slot(gt_offsets, G.gt_begin, gt_total, &g0, &unused);
    coco_slot(gt_offsets, (long long)G.gt_begin + G.gt_count - 1, gt_total, &unused, &g1);
    g1 = max(g1, g0);
    const bool staged = g1 - g0 <= COCO_LDS_RUNS;
    if (staged) {
        for (long long i = threadIdx.x; i < g1 - g0; i += COCO_THREADS) {
            s_ends[i] = gt_ends[g0 + i];
            s_cover[i] = gt_cover[g0 + i];
        }
    }
    __syncthreads();
    const long long pairs = (long long)G.dt_count * G.gt_count;
    for (long long pair = wave; pair < pairs; pair += COCO_THREADS / WAVE) {
        const int d = (int)(pair / G.gt_count), g = (int)(pair % G.gt_count);
        long long d0, d1, q0, q1;
        coco_slot(dt_offsets, (long long)G.dt_begin + d, dt_total, &d0, &d1);
        coco_slot(gt_offsets, (long long)G.gt_begin + g, gt_total, &q0, &q1);
        q0 = min(max(q0, g0), g1);                         // inside the group's range whatever the offsets hold
        q1 = min(max(q1, q0), g1);
        const int n_g = (int)min(q1 - q0, (long long)INT32_MAX);
        const int32_t* ge = staged ? s_ends + (q0 - g0) : gt_ends + q0;
        const int32_t* gc = staged ? s_cover + (q0 - g0) : gt_cover + q0;
        long long acc = 0;
        for (long long j = 1 + 2 * (long long)lane; j < d1 - d0; j += 2 * WAVE) {
            const int32_t s = dt_ends[d0 + j - 1], e = dt_ends[d0 + j];
            if (e > s) acc += coco_cover(ge, gc, n_g, e) - coco_cover(ge, gc, n_g, s);
        }
#pragma unroll
        for (int w = 1; w < WAVE; w <<= 1) acc += __shfl_xor(acc, w, WAVE);
        if (lane == 0) {
            const long long a_d = dt_area[G.dt_begin + d], a_g = gt_area[G.gt_begin + g];
            const long long uni = gt_crowd[G.gt_begin + g] ? a_d : a_d + a_g - acc;
            const long long at = G.iou_offset + (long long)d * G.gt_count + g;
            inter[at] = acc;
            iou[at] = acc == 0 ? 0.0 : __ddiv_rn((double)acc, (double)uni);
        }
    }
}

__global__ __launch_bounds__(COCO_THREADS) void coco_box_iou_kernel(const PgrCocoGroup* __restrict__ groups,
                                                                   const double* __restrict__ dt_boxes,
                                                                   const double* __restrict__ gt_boxes,
                                                                   const uint8_t* __restrict__ gt_crowd,
                                                                   double* __restrict__ iou) {
    const PgrCocoGroup G = groups[blockIdx.x];
    if (G.dt_count <= 0 || G.gt_count <= 0) return;
    const long long pairs = (long long)G.dt_count * G.gt_count;
    for (long long pair = threadIdx.x; pair < pairs; pair += COCO_THREADS) {
        const int d = (int)(pair / G.gt_count), g = (int)(pair % G.gt_count);
        const double* D = dt_boxes + 4 * ((long long)G.dt_begin + d);
        const double* B = gt_boxes + 4 * ((long long)G.gt_begin + g);
        const double dx = D[0], dy = D[1], dw = D[2], dh = D[3], gx = B[0], gy = B[1], gw = B[2], gh = B[3];
        const double iw = __dsub_rn(fmin(__dadd_rn(dx, dw), __dadd_rn(gx, gw)), fmax(dx, gx));
        const double ih = __dsub_rn(fmin(__dadd_rn(dy, dh), __dadd_rn(gy, gh)), fmax(dy, gy));
        const double in = (iw > 0.0 && ih > 0.0) ? __dmul_rn(iw, ih) : 0.0;
        const double a_d = __dmul_rn(dw, dh);
        const double uni = gt_crowd[G.gt_begin + g] ? a_d : __dsub_rn(__dadd_rn(a_d, __dmul_rn(gw, gh)), in);
        iou[G.iou_offset + pair] = in == 0.0 ? 0.0 : __ddiv_rn(in, uni);
    }
}

__global__ __launch_bounds__(WAVE) void coco_match_kernel(const PgrCocoGroup* __restrict__ groups, CocoMatchParams P,
                                                         const double* __restrict__ iou, const double* __restrict__ dt_area,
                                                         const double* __restrict__ gt_area,
                                                         const uint8_t* __restrict__ gt_flag,
                                                         const uint8_t* __restrict__ gt_crowd, long long n_dt, long long n_gt,
                                                         int32_t* __restrict__ order, int32_t* __restrict__ dt_match,
                                                         uint8_t* __restrict__ dt_ignore, int32_t* __restrict__ gt_match,
                                                         uint8_t* __restrict__ gt_ignore) {
    const PgrCocoGroup G = groups[blockIdx.x];
    const int lane = threadIdx.x;
    const int T = P.n_thr, A = P.n_area;
    // the GT's ignore flags and the order "not ignored first", once per area range; the matched state of every lane
    for (int a = 0; a < A; ++a) {
        uint8_t* ig = gt_ignore + (long long)a * n_gt + G.gt_begin;
        int32_t* ord = order + (long long)a * n_gt + G.gt_begin;
        int kept = 0;
        for (int g0 = 0; g0 < G.gt_count; g0 += WAVE) {
            const int g = g0 + lane;
            bool out = true;
            if (g < G.gt_count) {
                const double ar = gt_area[G.gt_begin + g];
                out = gt_flag[G.gt_begin + g] != 0 || ar < P.lo[a * T] || ar > P.hi[a * T];
                ig[g] = out ? 1 : 0;
            }
            kept += __popcll(__ballot(!out));
        }
        int at_kept = 0, at_out = kept;
        for (int g0 = 0; g0 < G.gt_count; g0 += WAVE) {
            const int g = g0 + lane;
            const bool valid = g < G.gt_count;
            const bool out = valid ? ig[g] != 0 : true;
            const unsigned long long m_kept = __ballot(valid && !out), m_out = __ballot(valid && out);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (valid) ord[out ? at_out + __popcll(m_out & below) : at_kept + __popcll(m_kept & below)] = g;
            at_kept += __popcll(m_kept);
            at_out += __popcll(m_out);
        }
        for (int t = 0; t < T; ++t) {
            int32_t* row = gt_match + ((long long)a * T + t) * n_gt + G.gt_begin;
            for (int g = lane; g < G.gt_count; g += WAVE) row[g] = -1;
        }
    }
    __syncthreads();                                       // one wave: orders the stores above before the reads below
    if (lane >= A * T) return;
    const int a = lane / T;
    const double thr = P.thr[lane], lo = P.lo[lane], hi = P.hi[lane];
    const uint8_t* ig = gt_ignore + (long long)a * n_gt + G.gt_begin;
    const int32_t* ord = order + (long long)a * n_gt + G.gt_begin;
    int32_t* gm = gt_match + (long long)lane * n_gt + G.gt_begin;          // lane = a * T + t
    int32_t* dm = dt_match + (long long)lane * n_dt + G.dt_begin;
    uint8_t* di = dt_ignore + (long long)lane * n_dt + G.dt_begin;
    for (int d = 0; d < G.dt_count; ++d) {
        const double* row = iou + G.iou_offset + (long long)d * G.gt_count;
        double best = thr;
        int m = -1;
        bool m_ig = false;
        for (int p = 0; p < G.gt_count; ++p) {
            const int g = ord[p];
            const bool g_ig = ig[g] != 0;
            if (gm[g] >= 0 && !gt_crowd[G.gt_begin + g]) continue;
            if (m > -1 && !m_ig && g_ig) break;
            const double v = row[g];
            if (v < best) continue;
            best = v;
            m = g;
            m_ig = g_ig;
        }
        if (m > -1) {
            dm[d] = G.gt_begin + m;
            di[d] = m_ig ? 1 : 0;
            gm[m] = G.dt_begin + d;
        } else {
            const double ar = dt_area[G.dt_begin + d];
            dm[d] = -1;
            di[d] = (ar < lo || ar > hi) ? 1 : 0;
        }
    }
}

struct CocoAccumulateParams {
    int32_t max_dets[PGR_COCO_MAX_MAXDETS];
    int32_t K, A, M, T, R;
};

__global__ __launch_bounds__(COCO_THREADS) void coco_accumulate_kernel(
    CocoAccumulateParams P, const long long* __restrict__ perm, const long long* __restrict__ seg_start, long long n_dt,
    const int32_t* __restrict__ rank, const int32_t* __restrict__ dt_match, const uint8_t* __restrict__ dt_ignore,
    const int32_t* __restrict__ npig, const double* __restrict__ rec_thrs, const double* __restrict__ dt_scores,
    int32_t* __restrict__ ws_tp, int32_t* __restrict__ ws_idx, double* __restrict__ ws_pr, double* __restrict__ precision,
    double* __restrict__ scores, double* __restrict__ recall) {
    __shared__ long long totals64[COCO_THREADS / WAVE];
    __shared__ int32_t totals32[COCO_THREADS / WAVE];
    __shared__ double totals_f[COCO_THREADS / WAVE];
    const int K = P.K, A = P.A, M = P.M, T = P.T, R = P.R;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, k = blockIdx.x / (M * A);
    const int32_t max_det = P.max_dets[m];
    const int32_t np = npig[k * A + a];
    const auto cell = [&](int t, int r) { return ((((long long)t * R + r) * K + k) * A + a) * M + m; };
    if (np <= 0) {
        for (int i = threadIdx.x; i < T * R; i += COCO_THREADS) {
            precision[cell(i / R, i % R)] = -1.0;
            scores[cell(i / R, i % R)] = -1.0;
        }
        for (int t = threadIdx.x; t < T; t += COCO_THREADS) recall[(((long long)t * K + k) * A + a) * M + m] = -1.0;
        return;
    }
    const long long s0 = min(max(seg_start[k], 0ll), n_dt), s1 = min(max(seg_start[k + 1], s0), n_dt);
    // this workgroup's slice of the workspace: as long as its segment
    const long long slice = ((long long)a * M + m) * n_dt + s0;
    int32_t* tpc = ws_tp + slice;
    int32_t* idx = ws_idx + slice;
    double* prc = ws_pr + slice;
    const auto add64 = [](long long x, long long y) { return x + y; };
    const auto add32 = [](int32_t x, int32_t y) { return x + y; };
    const auto fmx = [](double x, double y) { return fmax(x, y); };
    const double npd = (double)np;
    for (int t = 0; t < T; ++t) {
        const int32_t* match = dt_match + ((long long)a * T + t) * n_dt;
        const uint8_t* ign = dt_ignore + ((long long)a * T + t) * n_dt;
        long long carry = 0;                               // tp | fp << 32 in front of the chunk
        int32_t kept = 0;                                  // selected detections in front of the chunk
        for (long long c0 = s0; c0 < s1; c0 += COCO_CHUNK) {
            const long long i = c0 + threadIdx.x;
            long long det = -1;
            if (i < s1) {
                det = perm[i];
                if (det < 0 || det >= n_dt || rank[det] >= max_det) det = -1;
            }
            long long v = 0;
            if (det >= 0 && !ign[det]) v = match[det] >= 0 ? 1ll : (1ll << 32);
            const long long both = carry + rle_block_scan<long long>(v, 0ll, add64, totals64);
            long long chunk = 0;
            for (int q = 0; q < COCO_THREADS / WAVE; ++q) chunk += totals64[q];
            const int32_t sel = det >= 0 ? 1 : 0;
            const int32_t c = kept + rle_block_scan<int32_t>(sel, 0, add32, totals32) - 1;
            int32_t chunk_kept = 0;
            for (int q = 0; q < COCO_THREADS / WAVE; ++q) chunk_kept += totals32[q];
            if (sel) {
                const double tp = (double)(both & 0xffffffffll), fp = (double)(both >> 32);
                tpc[c] = (int32_t)(both & 0xffffffffll);
                idx[c] = (int32_t)det;
                prc[c] = __ddiv_rn(tp, __dadd_rn(__dadd_rn(fp, tp), 2.220446049250313e-16));
            }
            carry += chunk;
            kept += chunk_kept;
        }
        __syncthreads();                                   // the compacted arrays are written
        const int32_t n = kept;
        double behind = -1.0;                              // the largest pr behind the chunk
        for (long long c0 = 0; c0 < n; c0 += COCO_CHUNK) {
            const long long j = (long long)n - 1 - (c0 + threadIdx.x);
            const double mine = j >= 0 ? prc[j] : -1.0;
            const double incl = fmax(behind, rle_block_scan<double>(mine, -1.0, fmx, totals_f));
            if (j >= 0) prc[j] = incl;
            double chunk = -1.0;
            for (int q = 0; q < COCO_THREADS / WAVE; ++q) chunk = fmax(chunk, totals_f[q]);
            behind = fmax(behind, chunk);
        }
        __syncthreads();                                   // the running maxima are written
        for (int r = threadIdx.x; r < R; r += COCO_THREADS) {
            const double want = rec_thrs[r];
            int32_t lo = 0, hi = n;                        // the first detection whose recall reaches `want`
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                if (__ddiv_rn((double)tpc[mid], npd) >= want) hi = mid; else lo = mid + 1;
            }
            precision[cell(t, r)] = lo < n ? prc[lo] : 0.0;
            scores[cell(t, r)] = lo < n ? dt_scores[idx[lo]] : 0.0;
        }
        if (threadIdx.x == 0)
            recall[(((long long)t * K + k) * A + a) * M + m] = n ? __ddiv_rn((double)tpc[n - 1], npd) : 0.0;
        __syncthreads();                                   // the slice is read before the next threshold rewrites it
    }
}

}  // namespace pgr
