// png.hip.h -- PNG files of device images: parallel deflate, CRC-32, Adler-32 and chunk framing (pgr_png_encode,
// pgr_png_emit).  Owned by io.hip.
//
// THE FILE: signature, IHDR, ONE IDAT, IEND.  Colour type / depth 0/8, 2/8, 0/16 (big-endian samples), no interlace, every row
// filter type 0.  The IDAT payload is one zlib stream: 78 01, deflate data, the big-endian Adler-32 of the filtered raw stream
// (H rows of 1 + row_bytes).  The raw stream is cut into segments of PNG_S = PGR_PNG_SEGMENT_BYTES; one workgroup encodes one
// segment, independently of all others, and no match reaches in front of its segment.  A segment becomes one deflate block of
// the cheapest of stored / fixed Huffman / dynamic Huffman by the bytes it takes, ties to the earlier.  A Huffman-coded segment
// but the last is followed by an empty stored block (000, pad, 00 00 FF FF); a stored block ends on a byte boundary by itself.
// The last block carries BFINAL and is padded to a byte.  So: segment <= raw length + 5 bytes, file <= 63 + raw + 5 segments.
//
// png_encode_kernel, one workgroup of PNG_THREADS per segment, everything in LDS (72 KiB: two workgroups per CU):
//   1 load      the segment's raw bytes from the job's strided image (filter bytes, big-endian swap, mask scale); Adler sums
//   2 candidates (level 1) hash of the 3 bytes at p -> the highest earlier position of the bucket, one sub-block of PNG_THREADS
//               positions after the other: look up, barrier, atomicMax, barrier -- a position sees the sub-blocks in front of it
//   3 matches   per position: distances 1, 2, 3, 6, 1 + row_bytes and the hash candidate, each extended four bytes a step to
//               at most 258 inside the segment; longest wins, ties to the smaller distance.  A thread takes 16 consecutive
//               positions and starts a candidate's extension where the match of the position before it leaves off
//   4 parse     greedy from byte 0 by pointer jumping: jump[p] = p + max(1, len); each round marks the successors of marked
//               positions and squares the jump, ceil(log2 n) rounds
//   5 codes     LDS histograms of the marked tokens, the builder of png_codes.h on one lane per alphabet, the code-length
//               alphabet over the length sequence with its zero runs as symbols 17 / 18, the three costs, canonical codes
//               (counts per length, first codes, rank among equal lengths)
//   6 bits      per-thread bit counts over 16 consecutive positions, workgroup prefix sum, atomicOr into the dword image
//   7 out       CRC-32 of the bytes (a chunk per thread, combined with x^(8 * bytes behind it)), the image and the segment's
//               record to the workspace
// png_finish_kernel, one workgroup per file: offsets of the segments inside the IDAT, the file's size, Adler-32 and IDAT CRC.
// png_emit_kernel, one workgroup per segment: copies it behind its predecessors; the first also writes the 43 bytes in front
// and the 20 bytes behind.  Every global store is a plain C++ store.
#pragma once
#include "pgr_common.h"
#include "png_codes.h"

namespace pgr {

constexpr int PNG_S = PGR_PNG_SEGMENT_BYTES;
constexpr int PNG_THREADS = PGR_PNG_SUBBLOCK;
constexpr int PNG_PER_THREAD = PNG_S / PNG_THREADS;
constexpr int PNG_WAVES = PNG_THREADS / WAVE;
constexpr int PNG_HASH_BITS = 11;
constexpr int PNG_OUT_WORDS = PNG_S / 4 + 4;                 // a segment takes at most PNG_S + 5 bytes
constexpr int PNG_SLOT_BYTES = PNG_OUT_WORDS * 4;            // its place in the workspace
constexpr int PNG_CRC_CHUNK = ((PNG_S + 8 + PNG_THREADS - 1) / PNG_THREADS + 3) / 4 * 4;
constexpr int PNG_FINISH_THREADS = 256;
constexpr int PNG_EMIT_THREADS = 256;
constexpr int PNG_HEAD_BYTES = 43, PNG_TAIL_BYTES = 20;      // in front of the deflate data and behind it
constexpr uint32_t PNG_MARK = 0x80000000u;                   // in match[]: the greedy parse has a token here
constexpr int PNG_DIST_AT = 288, PNG_CL_AT = 320, PNG_ALL_CODES = PNG_CL_AT + PNG_CL_SYMBOLS;
static_assert(PNG_S % PNG_THREADS == 0 && PNG_S >= 8192 && PNG_S <= 32768 && (PNG_S & (PNG_S - 1)) == 0, "segment size");
static_assert(PNG_THREADS >= PNG_ALL_CODES && PNG_THREADS % WAVE == 0, "one thread per code");

__constant__ PngX8Table c_png_x8 = png_make_x8_table();
__constant__ uint8_t c_png_cl_order[PNG_CL_SYMBOLS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngJobDev {
    const uint8_t* pixels;
    int64_t row_stride;
    uint64_t raw_bytes;
    int32_t pixel_stride, width, height, kind, scale;
    uint32_t row_len;            // 1 + row_bytes
    uint32_t seg_first, n_segs;
};
struct PngSegInfo { uint32_t nbytes, crc, adler_a, adler_b; uint64_t prefix, pad; };
struct PngFileInfo { uint64_t data_bytes; uint32_t idat_crc, adler, ihdr_crc, pad; };

// the job of a segment: jobs[k].seg_first ascends
__device__ __forceinline__ int png_job_of_segment(const PngJobDev* jobs, int n_jobs, uint32_t seg) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].seg_first <= seg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// byte g of a job's filtered raw stream
__device__ __forceinline__ uint32_t png_raw_byte(const PngJobDev& J, uint32_t g) {
    const uint32_t row = g / J.row_len, c = g - row * J.row_len;
    if (c == 0) return 0;                                                        // filter type 0
    const uint8_t* line = J.pixels + (int64_t)row * J.row_stride;
    const uint32_t b = c - 1;
    if (J.kind == PGR_PNG_GRAY8) return (gload(line + (int64_t)b * J.pixel_stride) * (uint32_t)J.scale) & 255u;
    if (J.kind == PGR_PNG_RGB8) return gload(line + (int64_t)(b / 3) * J.pixel_stride + b % 3);
    return gload(line + (int64_t)(b >> 1) * J.pixel_stride + ((b & 1u) ^ 1u));   // big-endian from little-endian storage
}

struct PngLds {
    uint32_t raw[PNG_S / 4 + 2];
    uint32_t match[PNG_S];                       // len | dist << 9 | PNG_MARK   (while the candidates are found: position + 1)
    uint16_t jump[PNG_S + 2];
    union { uint32_t hash[1 << PNG_HASH_BITS]; uint32_t out[PNG_OUT_WORDS]; };
    uint32_t hist[PNG_CL_AT];                    // literal/length counts, distance counts at PNG_DIST_AT
    uint32_t cl_hist[PNG_CL_SYMBOLS];
    uint32_t codes[PNG_ALL_CODES];               // bit-reversed code | length << 16
    uint32_t count[3][16], first[3][16];
    uint32_t scratch_a[2 * 288 + 16], scratch_b[2 * 32 + 16];
    uint32_t wave_sum[PNG_WAVES];
    uint64_t zero_mask[PNG_WAVES];               // the code-length sequence: entry i is a zero
    uint32_t job, n, form, hlit, hdist, hclen, extra_bits, cost_dyn, cost_fix, adler_a, adler_b, crc, nbytes;
    uint8_t lens[PNG_ALL_CODES + 1];             // code lengths: literal/length, distance at PNG_DIST_AT, code-length at PNG_CL_AT
};
static_assert(sizeof(PngLds) <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ uint32_t png_load4(const uint32_t* raw, uint32_t p) {          // bytes p .. p + 3
    const uint32_t i = p >> 2;
    return __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], p & 3u);
}
// bytes that agree at p and q, at most max_len; the first `known` of them are known to agree
__device__ __forceinline__ uint32_t png_match_len(const uint32_t* raw, uint32_t p, uint32_t q, uint32_t max_len, uint32_t known) {
    uint32_t k = known;
    while (k < max_len) {
        const uint32_t x = png_load4(raw, p + k) ^ png_load4(raw, q + k);
        if (x) { k += (uint32_t)(__ffs((int)x) - 1) >> 3; break; }
        k += 4;
    }
    return min(k, max_len);
}
// value's low `bits` (<= 32) bits into the image at bit `pos`
__device__ __forceinline__ void png_put_bits(uint32_t* out, uint32_t pos, uint32_t value, uint32_t bits) {
    if (bits == 0 || (pos >> 5) + 1 >= (uint32_t)PNG_OUT_WORDS) return;       // (the costs keep every block inside the image)
    const uint64_t x = (uint64_t)value << (pos & 31u);
    atomicOr(&out[pos >> 5], (uint32_t)x);
    if ((uint32_t)(x >> 32)) atomicOr(&out[(pos >> 5) + 1], (uint32_t)(x >> 32));
}
// exclusive prefix sum over the workgroup; `total` is the sum of all.  Two barriers.
__device__ __forceinline__ uint32_t png_block_scan(uint32_t v, uint32_t* wave_sum, uint32_t& total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += o;
    }
    if (lane == WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int k = 0; k < (int)(blockDim.x / WAVE); ++k) {
        const uint32_t s = wave_sum[k];
        if (k < wave) before += s;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}
// the token at a marked position: its codes and extra bits, (bits, value) for the literal/length part and the distance part
__device__ __forceinline__ void png_token_bits(const PngLds& L, uint32_t p, uint32_t m, uint32_t& bits1, uint32_t& val1,
                                               uint32_t& bits2, uint32_t& val2) {
    const uint32_t len = m & 511u;
    bits2 = 0; val2 = 0;
    if (len == 0) {
        const uint32_t c = L.codes[(L.raw[p >> 2] >> ((p & 3u) * 8)) & 255u];
        bits1 = c >> 16; val1 = c & 0xFFFFu;
        return;
    }
    uint32_t s, eb, ev;
    png_length_symbol(len, s, eb, ev);
    uint32_t c = L.codes[s];
    bits1 = (c >> 16) + eb; val1 = (c & 0xFFFFu) | (ev << (c >> 16));
    png_dist_symbol((m >> 9) & 0xFFFFu, s, eb, ev);
    c = L.codes[PNG_DIST_AT + s];
    bits2 = (c >> 16) + eb; val2 = (c & 0xFFFFu) | (ev << (c >> 16));
}

__global__ void __launch_bounds__(PNG_THREADS) png_encode_kernel(const PngJobDev* __restrict__ jobs, int n_jobs, int level,
                                                                 PngSegInfo* __restrict__ info, uint8_t* __restrict__ slots) {
    __shared__ PngLds L;
    const uint32_t tid = threadIdx.x, seg = blockIdx.x;
    if (tid == 0) L.job = (uint32_t)png_job_of_segment(jobs, n_jobs, seg);
    for (uint32_t i = tid; i < PNG_CL_AT; i += PNG_THREADS) L.hist[i] = 0;
    for (uint32_t i = tid; i < PNG_ALL_CODES + 1; i += PNG_THREADS) L.lens[i] = 0;
    if (tid < PNG_CL_SYMBOLS) L.cl_hist[tid] = 0;
    if (tid < 48) (&L.count[0][0])[tid] = 0;
    if (tid == 0) { L.extra_bits = L.cost_dyn = L.cost_fix = L.adler_a = L.adler_b = L.crc = 0; }
    __syncthreads();
    const PngJobDev J = jobs[L.job];
    const uint32_t s_in_job = seg - J.seg_first;
    const uint64_t g0 = (uint64_t)s_in_job * PNG_S;
    const uint32_t n = (uint32_t)min((uint64_t)PNG_S, J.raw_bytes - g0);
    const bool last = s_in_job + 1 == J.n_segs;
    uint8_t* raw8 = reinterpret_cast<uint8_t*>(L.raw);

    // 1 load
    {
        uint32_t a = 0, b = 0;
        for (uint32_t i = tid; i < PNG_S + 8; i += PNG_THREADS) {
            const uint32_t v = i < n ? png_raw_byte(J, (uint32_t)g0 + i) : 0;
            raw8[i] = (uint8_t)v;
            a += v;
            b += (n - min(i, n)) * v;
        }
        atomicAdd(&L.adler_a, a % PNG_ADLER_MOD);
        atomicAdd(&L.adler_b, b % PNG_ADLER_MOD);
    }
    if (level > 0)
        for (uint32_t i = tid; i < (1u << PNG_HASH_BITS); i += PNG_THREADS) L.hash[i] = 0;
    __syncthreads();

    if (level > 0) {
        // 2 candidates
        for (uint32_t p0 = 0; p0 < n; p0 += PNG_THREADS) {
            const uint32_t p = p0 + tid;
            const bool hashed = p + PNG_MIN_MATCH <= n;
            uint32_t h = 0;
            if (hashed) {
                h = ((png_load4(L.raw, p) & 0xFFFFFFu) * 0x9E3779B1u) >> (32 - PNG_HASH_BITS);
                L.match[p] = L.hash[h];
            }
            __syncthreads();
            if (hashed) atomicMax(&L.hash[h], p + 1);
            __syncthreads();
        }
        // 3 matches
        const uint32_t row_dist = J.row_len;
        // a thread takes 16 consecutive positions: a match of L bytes at p - 1 is one of L - 1 bytes at p for the same distance,
        // which is where that candidate's extension starts.  Kept per fixed distance (0: not extended at p - 1), so a run costs
        // each of them one step a position and not its whole length again
        uint32_t carried[5] = {0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
            const uint32_t p = tid * PNG_PER_THREAD + i;
            if (p >= n) break;
            const uint32_t max_len = min((uint32_t)PNG_MAX_MATCH, n - p);
            uint32_t best_len = 0, best_dist = 0;
            if (max_len >= PNG_MIN_MATCH) {
                const uint32_t cand = L.match[p];
                // (max_len >= 3 for every position but the segment's last two, which no carried length outlives)
                const uint32_t dists[6] = {1, 2, 3, 6, row_dist, cand ? p + 1 - cand : 0};
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const uint32_t d = dists[c];
                    if (d == 0 || d > p || (best_len == max_len && d > best_dist)) {
                        if (c < 5) carried[c] = 0;
                        continue;
                    }
                    const uint32_t known = c < 5 && carried[c] ? carried[c] - 1 : 0;
                    const uint32_t len = png_match_len(L.raw, p, p - d, max_len, known);
                    if (c < 5) carried[c] = len;
                    if (len >= PNG_MIN_MATCH && (len > best_len || (len == best_len && d < best_dist))) { best_len = len; best_dist = d; }
                }
            }
            L.match[p] = best_len | (best_dist << 9);
            L.jump[p] = (uint16_t)(p + max(best_len, 1u));
        }
        if (tid == 0) { L.jump[n] = (uint16_t)n; }
        __syncthreads();
        // 4 parse
        if (tid == 0) L.match[0] |= PNG_MARK;
        __syncthreads();
        const int rounds = 32 - __clz((int)n);
        for (int r = 0; r < rounds; ++r) {
            uint16_t next[PNG_PER_THREAD];
#pragma unroll
            for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
                const uint32_t p = i * PNG_THREADS + tid;
                next[i] = 0;
                if (p < n) {
                    const uint32_t j = L.jump[p];
                    if ((L.match[p] & PNG_MARK) && j < n) atomicOr(&L.match[j], PNG_MARK);
                    next[i] = L.jump[j];
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
                const uint32_t p = i * PNG_THREADS + tid;
                if (p < n) L.jump[p] = next[i];
            }
            __syncthreads();
        }
    } else {
        for (uint32_t p = tid; p < n; p += PNG_THREADS) L.match[p] = PNG_MARK;
        __syncthreads();
    }

    // 5 codes: histograms of the tokens at this thread's 16 consecutive positions
    const uint32_t p_first = tid * PNG_PER_THREAD;
    {
        uint32_t extra = 0;
        for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
            const uint32_t p = p_first + i;
            if (p >= n) break;
            const uint32_t m = L.match[p];
            if (!(m & PNG_MARK)) continue;
            const uint32_t len = m & 511u;
            if (len == 0) { atomicAdd(&L.hist[raw8[p]], 1u); continue; }
            uint32_t s, eb, ev;
            png_length_symbol(len, s, eb, ev);
            atomicAdd(&L.hist[s], 1u);
            extra += eb;
            png_dist_symbol((m >> 9) & 0xFFFFu, s, eb, ev);
            atomicAdd(&L.hist[PNG_DIST_AT + s], 1u);
            extra += eb;
        }
        if (extra) atomicAdd(&L.extra_bits, extra);
        if (tid == 0) L.hist[256] = 1;                                         // end of block: always coded
    }
    __syncthreads();
    if (tid == 0) {
        png_code_lengths(L.hist, PNG_LITLEN_SYMBOLS, 15, L.lens, L.scratch_a);
        uint32_t s = PNG_LITLEN_SYMBOLS;
        while (s > 257 && L.lens[s - 1] == 0) --s;
        L.hlit = s;
    }
    if (tid == WAVE) {
        png_code_lengths(L.hist + PNG_DIST_AT, PNG_DIST_SYMBOLS, 15, L.lens + PNG_DIST_AT, L.scratch_b);
        uint32_t s = PNG_DIST_SYMBOLS;
        while (s > 1 && L.lens[PNG_DIST_AT + s - 1] == 0) --s;
        L.hdist = s;                                                           // no distance used: one zero length
    }
    __syncthreads();
    // the code lengths as ONE sequence of hlit + hdist entries, one thread each.  A run of zeros goes as symbols 18 (11..138
    // zeros) and 17 (3..10), found from the waves' ballots by the thread at its start; one or two left over and every other
    // length go as themselves (symbol 16 is not used)
    const uint32_t hlit = L.hlit, hdist = L.hdist;
    const bool in_seq = tid < hlit + hdist;
    const uint32_t my_cl = in_seq ? L.lens[tid < hlit ? tid : PNG_DIST_AT + tid - hlit] : 1;
    const bool is_zero = in_seq && my_cl == 0;
    {
        const uint64_t zeros = __ballot(is_zero);
        if ((tid & (WAVE - 1)) == 0) L.zero_mask[tid / WAVE] = zeros;
    }
    __syncthreads();
    uint32_t run = 0;
    if (is_zero && !(tid > 0 && ((L.zero_mask[(tid - 1) / WAVE] >> ((tid - 1) & 63u)) & 1u))) {
        for (uint32_t i = tid; i < PNG_THREADS;) {
            const uint32_t room = 64 - (i & 63u);
            const uint64_t stop = ~(L.zero_mask[i / WAVE] >> (i & 63u));           // the shifted-in zeros stop it at the word's end
            const uint32_t c = min(stop ? (uint32_t)__builtin_ctzll(stop) : 64u, room);
            run += c;
            i += c;
            if (c < room) break;
        }
    }
    const uint32_t rest = run % 138;
    const uint32_t n18 = run / 138 + (rest >= 11), n17 = rest >= 3 && rest < 11, n0 = rest < 3 ? rest : 0;
    if (run) {
        if (n18) atomicAdd(&L.cl_hist[18], n18);
        if (n17) atomicAdd(&L.cl_hist[17], n17);
        if (n0) atomicAdd(&L.cl_hist[0], n0);
    } else if (in_seq && !is_zero) {
        atomicAdd(&L.cl_hist[my_cl], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        png_code_lengths(L.cl_hist, PNG_CL_SYMBOLS, 7, L.lens + PNG_CL_AT, L.scratch_a);
        uint32_t k = PNG_CL_SYMBOLS;
        while (k > 4 && L.lens[PNG_CL_AT + c_png_cl_order[k - 1]] == 0) --k;
        L.hclen = k;
    }
    __syncthreads();
    if (tid < PNG_CL_AT) {
        const uint32_t f = L.hist[tid];
        if (f) { atomicAdd(&L.cost_dyn, f * L.lens[tid]); atomicAdd(&L.cost_fix, f * png_fixed_length((int)tid)); }
    }
    // where this thread's part of the coded lengths starts, and how long they are together (two barriers)
    uint32_t header_bits;
    const uint32_t header_at = png_block_scan(
        run ? n18 * (L.lens[PNG_CL_AT + 18] + 7u) + n17 * (L.lens[PNG_CL_AT + 17] + 3u) + n0 * L.lens[PNG_CL_AT]
            : (in_seq && !is_zero) ? L.lens[PNG_CL_AT + my_cl] : 0u,
        L.wave_sum, header_bits);
    if (tid == 0) {
        // the three forms by the bytes the segment takes, ties to the earlier: 0 stored, 1 fixed, 2 dynamic
        const uint32_t bits_fix = 3 + L.cost_fix + L.extra_bits;
        const uint32_t bits_dyn = 3 + 14 + 3 * L.hclen + header_bits + L.cost_dyn + L.extra_bits;
        const uint32_t bytes_fix = last ? (bits_fix + 7) / 8 : (bits_fix + 3 + 7) / 8 + 4;
        const uint32_t bytes_dyn = last ? (bits_dyn + 7) / 8 : (bits_dyn + 3 + 7) / 8 + 4;
        uint32_t form = 0, best = n + 5;
        if (bytes_fix < best) { form = 1; best = bytes_fix; }
        if (bytes_dyn < best) { form = 2; best = bytes_dyn; }
        L.form = form;
        L.nbytes = best;
    }
    __syncthreads();
    const uint32_t form = L.form, nbytes = L.nbytes;
    for (uint32_t i = tid; i < PNG_OUT_WORDS; i += PNG_THREADS) L.out[i] = 0;
    if (form == 1 && tid < PNG_CL_AT) L.lens[tid] = (uint8_t)png_fixed_length((int)tid);
    __syncthreads();
    if (form == 0) {
        uint8_t* out8 = reinterpret_cast<uint8_t*>(L.out);
        if (tid == 0) {
            out8[0] = last ? 1 : 0;
            out8[1] = (uint8_t)(n & 255u); out8[2] = (uint8_t)(n >> 8);
            out8[3] = (uint8_t)(~n & 255u); out8[4] = (uint8_t)((~n >> 8) & 255u);
        }
        for (uint32_t i = tid; i < n; i += PNG_THREADS) out8[5 + i] = raw8[i];
    } else {
        // canonical codes of the three alphabets: counts per length, first code per length, rank among equal lengths
        const int alphabet = tid < PNG_DIST_AT ? 0 : tid < PNG_CL_AT ? 1 : 2;
        const uint32_t base = alphabet == 0 ? 0 : alphabet == 1 ? PNG_DIST_AT : PNG_CL_AT;
        const uint32_t my_len = tid < PNG_ALL_CODES ? L.lens[tid] : 0;
        if (my_len) atomicAdd(&L.count[alphabet][my_len], 1u);
        __syncthreads();
        if (tid < 3) {
            uint32_t code = 0;
            L.first[tid][0] = 0;
            for (int l = 1; l < 16; ++l) {
                code = (code + (l > 1 ? L.count[tid][l - 1] : 0)) << 1;
                L.first[tid][l] = code;
            }
        }
        __syncthreads();
        if (tid < PNG_ALL_CODES) {
            uint32_t rank = 0;
            for (uint32_t j = base; j < tid; ++j) rank += L.lens[j] == my_len;
            const uint32_t code = L.first[alphabet][my_len] + rank;
            L.codes[tid] = my_len ? ((__brev(code) >> (32 - my_len)) | (my_len << 16)) : 0;
        }
        __syncthreads();
        // 6 bits
        uint32_t token_base = 3;
        if (tid == 0) png_put_bits(L.out, 0, (last ? 1u : 0u) | ((uint32_t)form << 1), 3);
        if (form == 2) {
            const uint32_t hclen = L.hclen;
            if (tid == 0) png_put_bits(L.out, 3, (hlit - 257) | ((hdist - 1) << 5) | ((hclen - 4) << 10), 14);
            if (tid < hclen) png_put_bits(L.out, 17 + 3 * tid, L.lens[PNG_CL_AT + c_png_cl_order[tid]], 3);
            uint32_t at = 17 + 3 * hclen + header_at;
            if (run) {
                const uint32_t c18 = L.codes[PNG_CL_AT + 18], c17 = L.codes[PNG_CL_AT + 17], c0 = L.codes[PNG_CL_AT];
                for (uint32_t k = 0; k < n18; ++k) {
                    const uint32_t zeros = k < run / 138 ? 138 : rest;
                    png_put_bits(L.out, at, (c18 & 0xFFFFu) | ((zeros - 11) << (c18 >> 16)), (c18 >> 16) + 7);
                    at += (c18 >> 16) + 7;
                }
                if (n17) png_put_bits(L.out, at, (c17 & 0xFFFFu) | ((rest - 3) << (c17 >> 16)), (c17 >> 16) + 3);
                for (uint32_t k = 0; k < n0; ++k) png_put_bits(L.out, at + k * (c0 >> 16), c0 & 0xFFFFu, c0 >> 16);
            } else if (in_seq && !is_zero) {
                const uint32_t c = L.codes[PNG_CL_AT + my_cl];
                png_put_bits(L.out, at, c & 0xFFFFu, c >> 16);
            }
            token_base = 17 + 3 * hclen + header_bits;
        }
        uint32_t my_bits = 0;
        for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
            const uint32_t p = p_first + i;
            if (p >= n) break;
            const uint32_t m = L.match[p];
            if (!(m & PNG_MARK)) continue;
            uint32_t b1, v1, b2, v2;
            png_token_bits(L, p, m, b1, v1, b2, v2);
            my_bits += b1 + b2;
        }
        uint32_t token_bits;
        uint32_t pos = token_base + png_block_scan(my_bits, L.wave_sum, token_bits);
        for (uint32_t i = 0; i < PNG_PER_THREAD; ++i) {
            const uint32_t p = p_first + i;
            if (p >= n) break;
            const uint32_t m = L.match[p];
            if (!(m & PNG_MARK)) continue;
            uint32_t b1, v1, b2, v2;
            png_token_bits(L, p, m, b1, v1, b2, v2);
            png_put_bits(L.out, pos, v1, b1);
            png_put_bits(L.out, pos + b1, v2, b2);
            pos += b1 + b2;
        }
        if (tid == 0) {
            const uint32_t eob = L.codes[256];
            uint32_t end = token_base + token_bits;
            png_put_bits(L.out, end, eob & 0xFFFFu, eob >> 16);
            end += eob >> 16;
            if (!last) png_put_bits(L.out, ((end + 3 + 7) / 8) * 8 + 16, 0xFFFFu, 16);      // 000, pad, 00 00 FF FF
        }
    }
    __syncthreads();

    // 7 out
    {
        const uint8_t* out8 = reinterpret_cast<const uint8_t*>(L.out);
        const uint32_t start = tid * PNG_CRC_CHUNK;
        if (start < nbytes) {
            const uint32_t end = min(start + (uint32_t)PNG_CRC_CHUNK, nbytes);
            uint32_t reg = 0xFFFFFFFFu;
            for (uint32_t i = start; i < end; ++i) reg = png_crc_byte(reg, out8[i]);
            atomicXor(&L.crc, png_gf_mul(~reg, png_x8_pow(c_png_x8.pow, nbytes - end)));
        }
        uint32_t* slot = reinterpret_cast<uint32_t*>(slots + (size_t)seg * PNG_SLOT_BYTES);
        for (uint32_t i = tid; i < (nbytes + 3) / 4; i += PNG_THREADS) slot[i] = L.out[i];
    }
    __syncthreads();
    if (tid == 0) {
        PngSegInfo r;
        r.nbytes = nbytes;
        r.crc = L.crc;
        r.adler_a = (1 + L.adler_a) % PNG_ADLER_MOD;
        r.adler_b = (n + L.adler_b) % PNG_ADLER_MOD;
        r.prefix = 0;
        r.pad = 0;
        info[seg] = r;
    }
}

// One workgroup per file: the segments' offsets inside the deflate data, the file's size and checksums.
__global__ void __launch_bounds__(PNG_FINISH_THREADS) png_finish_kernel(const PngJobDev* __restrict__ jobs, PngSegInfo* __restrict__ info,
                                                                        PngFileInfo* __restrict__ files, long long* __restrict__ sizes) {
    __shared__ uint32_t wave_sum[PNG_FINISH_THREADS / WAVE];
    __shared__ uint32_t s_crc, s_a, s_b;
    const uint32_t tid = threadIdx.x;
    const PngJobDev J = jobs[blockIdx.x];
    PngSegInfo* segs = info + J.seg_first;
    if (tid == 0) { s_crc = 0; s_a = 0; s_b = 0; }
    uint64_t data = 0;
    for (uint32_t base = 0; base < J.n_segs; base += PNG_FINISH_THREADS) {
        const uint32_t i = base + tid;
        const uint32_t v = i < J.n_segs ? min(segs[i].nbytes, (uint32_t)PNG_SLOT_BYTES) : 0;
        uint32_t total;
        const uint32_t at = png_block_scan(v, wave_sum, total);
        if (i < J.n_segs) segs[i].prefix = data + at;
        data += total;
    }
    uint32_t crc = 0, a = 0, b = 0;
    for (uint32_t i = tid; i < J.n_segs; i += PNG_FINISH_THREADS) {              // the same thread wrote segs[i].prefix
        const PngSegInfo r = segs[i];
        const uint32_t nb = min(r.nbytes, (uint32_t)PNG_SLOT_BYTES);
        const uint64_t raw_behind = J.raw_bytes - min(J.raw_bytes, (uint64_t)(i + 1) * PNG_S);
        crc ^= png_gf_mul(r.crc, png_x8_pow(c_png_x8.pow, data - r.prefix - nb + 4));       // the Adler-32 follows the data
        const uint32_t a1 = (r.adler_a + PNG_ADLER_MOD - 1) % PNG_ADLER_MOD;
        a = (a + a1) % PNG_ADLER_MOD;
        b = (uint32_t)((b + r.adler_b + (raw_behind % PNG_ADLER_MOD) * a1) % PNG_ADLER_MOD);
    }
    __syncthreads();
    atomicXor(&s_crc, crc);
    atomicAdd(&s_a, a);
    atomicAdd(&s_b, b);
    __syncthreads();
    if (tid == 0) {
        PngFileInfo F;
        F.data_bytes = data;
        F.adler = ((s_b % PNG_ADLER_MOD) << 16) | ((1 + s_a) % PNG_ADLER_MOD);
        const uint32_t depth = J.kind == PGR_PNG_GRAY16 ? 16 : 8, ctype = J.kind == PGR_PNG_RGB8 ? 2 : 0;
        const uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(J.width >> 24), (uint8_t)(J.width >> 16), (uint8_t)(J.width >> 8),
                                  (uint8_t)J.width, (uint8_t)(J.height >> 24), (uint8_t)(J.height >> 16), (uint8_t)(J.height >> 8),
                                  (uint8_t)J.height, (uint8_t)depth, (uint8_t)ctype, 0, 0, 0};
        uint32_t reg = 0xFFFFFFFFu;
        for (int i = 0; i < 17; ++i) reg = png_crc_byte(reg, ihdr[i]);
        F.ihdr_crc = ~reg;
        const uint8_t head[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
        reg = 0xFFFFFFFFu;
        for (int i = 0; i < 6; ++i) reg = png_crc_byte(reg, head[i]);
        uint32_t tail = 0xFFFFFFFFu;
        for (int i = 0; i < 4; ++i) tail = png_crc_byte(tail, (F.adler >> (24 - 8 * i)) & 255u);
        F.idat_crc = png_gf_mul(~reg, png_x8_pow(c_png_x8.pow, data + 4)) ^ s_crc ^ ~tail;
        F.pad = 0;
        files[blockIdx.x] = F;
        sizes[blockIdx.x] = (long long)(PNG_HEAD_BYTES + PNG_TAIL_BYTES + data);
    }
}

// byte t of the 43 in front of the deflate data / of the 20 behind it
__device__ __forceinline__ uint32_t png_head_byte(const PngJobDev& J, const PngFileInfo& F, uint32_t t) {
    const uint8_t fixed[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    if (t < 16) return fixed[t];
    if (t < 20) return ((uint32_t)J.width >> (8 * (19 - t))) & 255u;
    if (t < 24) return ((uint32_t)J.height >> (8 * (23 - t))) & 255u;
    if (t == 24) return J.kind == PGR_PNG_GRAY16 ? 16 : 8;
    if (t == 25) return J.kind == PGR_PNG_RGB8 ? 2 : 0;
    if (t < 29) return 0;
    if (t < 33) return (F.ihdr_crc >> (8 * (32 - t))) & 255u;
    if (t < 37) return (uint32_t)((F.data_bytes + 6) >> (8 * (36 - t))) & 255u;
    const uint8_t idat[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    return idat[t - 37];
}
__device__ __forceinline__ uint32_t png_tail_byte(const PngFileInfo& F, uint32_t t) {
    if (t < 4) return (F.adler >> (8 * (3 - t))) & 255u;
    if (t < 8) return (F.idat_crc >> (8 * (7 - t))) & 255u;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    return iend[t - 8];
}

// One workgroup per segment.  A byte of file k is stored at files[offsets[k] + rel] only for 0 <= rel < min(offsets[k+1], total)
// - offsets[k] and offsets[k] >= 0: no store leaves the file's range whatever the device-side offsets or the workspace hold.
__global__ void __launch_bounds__(PNG_EMIT_THREADS) png_emit_kernel(const PngJobDev* __restrict__ jobs, int n_jobs, uint32_t n_segs,
                                                                    const PngSegInfo* __restrict__ info, const PngFileInfo* __restrict__ finfo,
                                                                    const uint8_t* __restrict__ slots, const long long* __restrict__ offsets,
                                                                    long long total, uint8_t* __restrict__ files) {
    const uint32_t tid = threadIdx.x, seg = blockIdx.x;
    const int job = png_job_of_segment(jobs, n_jobs, seg);
    const PngJobDev J = jobs[job];
    const long long lo = offsets[job], hi = min(offsets[job + 1], total);
    if (lo < 0 || hi <= lo) return;
    const uint64_t room = (uint64_t)(hi - lo);
    uint8_t* file = files + lo;
    const PngSegInfo r = info[seg];
    const uint32_t nb = min(r.nbytes, (uint32_t)PNG_SLOT_BYTES);
    const uint8_t* slot = slots + (size_t)seg * PNG_SLOT_BYTES;
    const uint64_t at = (uint64_t)PNG_HEAD_BYTES + r.prefix;
    for (uint32_t i = tid; i < nb; i += PNG_EMIT_THREADS) {
        const uint64_t rel = at + i;
        if (rel >= at && rel < room) file[rel] = slot[i];
    }
    if (seg == J.seg_first && seg < n_segs) {
        const PngFileInfo F = finfo[job];
        if (tid < PNG_HEAD_BYTES) {
            if (tid < room) file[tid] = (uint8_t)png_head_byte(J, F, tid);
        } else if (tid >= WAVE && tid < WAVE + PNG_TAIL_BYTES) {
            const uint64_t rel = (uint64_t)PNG_HEAD_BYTES + F.data_bytes + (tid - WAVE);
            if (rel >= PNG_HEAD_BYTES && rel < room) file[rel] = (uint8_t)png_tail_byte(F, tid - WAVE);
        }
    }
}

}  // namespace pgr
