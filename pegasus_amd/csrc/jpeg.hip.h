// jpeg.hip.h -- baseline JPEG files of device images: colour transform, 8x8 DCT, quantisation, per-file Huffman tables and
// the entropy-coded scan (pgr_jpeg_encode, pgr_jpeg_emit).  Owned by io.hip, behind png.hip.h.
//
// THE FILE: SOI, APP0 JFIF 1.01 (units 0, density 1:1, no thumbnail), ONE DQT (table 0, for colour also table 1; 8-bit, zigzag
// order), SOF0 (8-bit; gray: component 1; colour: components 1, 2, 3 = Y, Cb, Cr, Y sampled 1x1 or 2x2, chroma 1x1, chroma on
// tables 1), ONE DHT (DC0, AC0, for colour also DC1, AC1), DRI (JPEG_R), SOS (one interleaved scan, Ss 0, Se 63, Ah/Al 0),
// entropy data, EOI.
//
// SAMPLES.  The image is extended to whole MCUs (8x8; 16x16 at 4:2:0) by repeating its last column and row.  Colour is JFIF
// full-range YCbCr in libjpeg's 16-bit fixed point:
//   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
// At 4:2:0 a chroma sample is (a + b + c + d + 2) >> 2 of the 2x2 chroma values under it.  Every sample s loses 128.
//
// DCT.  C[u][x] = round(2^19 c_u cos((2x + 1) u pi / 16)), c_0 = 1 / sqrt 2, c_u = 1: the integers of JPEG_K below, by the
// symmetries of the cosine.  Two passes, no rounding between them:
//   T[y][u] = sum_x C[u][x] s[y][x]            (int32, |T| < 2^29, scale 2^20 of the orthonormal row transform)
//   F[v][u] = sum_y C[v][y] T[y][u]            (int64, scale 2^40)
//   f       = (F + 2^27) >> 28                 (floor; scale 2^12, |f| < 2^24)
// Each sum runs x (y) = 0 .. 7 in order -- integers: the order does not matter.
// QUANTISATION.  q = sign(f) * ((|f| + Q * 2^11) / (Q * 2^12)), integer division: f / (Q 2^12) rounded half away from zero.  Q is
// the IJG table (pgr_jpeg_quant_tables).  AC is clamped to +-1023; the DC difference to +-2047.
// (|f / 2^12 - exact coefficient| <= 0.003: 2^-11 * 2.83 from the rounding of C in the first pass, 8 * 0.5 * 362.04 / 2^20 from the
// second, 2^-13 from the shift.)
//
// SCAN.  MCUs in raster order; in an MCU Y (four blocks at 4:2:0: top left, top right, bottom left, bottom right), Cb, Cr.  An
// interval is JPEG_R MCUs whatever the width.  DC: difference to the previous block of the component, predictor 0 at the start
// of an interval; symbol = size.  AC in zigzag order: (run << 4) | size, ZRL F0 per 16 zeros, EOB 00 when the block's last
// coefficient is 0.  Extra bits: v, or v - 1 for v < 0, in `size` bits.  Bits are packed MSB first, an interval is padded with
// 1-bits to a byte, every FF byte (the padded one included) is followed by 00, interval i is followed by RST(i mod 8), the last
// by EOI.
//
// CODES.  Per file and table from the file's own symbol counts: counts c become (c + 2^k - 1) >> k for the smallest k that
// brings the table's largest count to 2^22 or below (k = 0 below 4 million blocks); a pseudo-symbol 256 with count 1 is added;
// png_code_lengths with limit 16; the pseudo-symbol swaps lengths with the LARGEST symbol of the longest length if its own is
// shorter; canonical codes by (length, symbol), so the pseudo-symbol takes the code of all ones and is left out of the DHT.
//
// jpeg_blocks_kernel  one workgroup per interval, a wave per block: samples, DCT by wave shuffles, quantised coefficients
//                     in zigzag order (DC as its difference) to the workspace, symbol counts through LDS to the file's histograms
// jpeg_tables_kernel  one workgroup per file, a wave per table: lengths (one lane), codes and DHT order (all lanes), the header
// jpeg_scan_kernel    one workgroup per interval, a wave per block: the nonzero mask of a block is one __ballot, runs are bit
//                     operations on it; bits per block, prefix, atomicOr into an LDS dword image, stuffing count.  <false> stores
//                     the interval's byte count, <true> stores its bytes into the file (and the first interval the header)
// jpeg_finish_kernel  one workgroup per file: the intervals' offsets and the file's size
// Every global store is a plain C++ store; the histogram flush is an integer atomic add whose result does not depend on order.
#pragma once
#include "pgr_common.h"
#include "png_codes.h"

namespace pgr {

constexpr int JPEG_R = PGR_JPEG_RESTART_MCUS;
constexpr int JPEG_THREADS = 256;
constexpr int JPEG_WAVES = JPEG_THREADS / WAVE;
constexpr int JPEG_MAX_BLOCKS = JPEG_R * 6;                      // of an interval, at 4:2:0
constexpr int JPEG_BLOCK_BITS = (16 + 11) + 63 * (16 + 10);      // the most a block takes: 1665
constexpr int JPEG_CHUNK = (((JPEG_MAX_BLOCKS * JPEG_BLOCK_BITS + 7) / 8 + JPEG_THREADS - 1) / JPEG_THREADS + 3) / 4 * 4;
constexpr int JPEG_IMG_WORDS = JPEG_THREADS * JPEG_CHUNK / 4 + 1;
constexpr int JPEG_HEAD_MAX = 640;                               // 613 is the longest header (12 DC and 162 AC symbols a table)
constexpr int JPEG_SYMBOLS = 257;                                // 256 and the pseudo-symbol
static_assert(JPEG_R >= 1 && JPEG_R <= 64, "an interval's bits fit LDS twice over");
static_assert(JPEG_THREADS * JPEG_CHUNK * 8 >= JPEG_MAX_BLOCKS * JPEG_BLOCK_BITS + 7, "the image holds an interval");

// round(2^19 cos(k pi / 16)), k = 0 .. 8
__constant__ int32_t c_jpeg_k[9] = {524288, 514214, 484379, 435930, 370728, 291279, 200636, 102284, 0};

struct JpegZigzag { uint8_t nat_of_zz[64], zz_of_nat[64]; };
constexpr JpegZigzag jpeg_make_zigzag() {
    JpegZigzag z{};
    int x = 0, y = 0;
    for (int k = 0; k < 64; ++k) {
        z.nat_of_zz[k] = (uint8_t)(y * 8 + x);
        z.zz_of_nat[y * 8 + x] = (uint8_t)k;
        if ((x + y) % 2 == 0) {                  // moving up and to the right
            if (x == 7) ++y; else if (y == 0) ++x; else { ++x; --y; }
        } else {
            if (y == 7) ++x; else if (x == 0) ++y; else { --x; ++y; }
        }
    }
    return z;
}
constexpr JpegZigzag JPEG_ZIGZAG = jpeg_make_zigzag();
static_assert(JPEG_ZIGZAG.nat_of_zz[2] == 8 && JPEG_ZIGZAG.nat_of_zz[9] == 24 && JPEG_ZIGZAG.nat_of_zz[35] == 56 &&
              JPEG_ZIGZAG.nat_of_zz[62] == 62 && JPEG_ZIGZAG.zz_of_nat[63] == 63, "the zigzag of ITU-T T.81 figure 5");
__constant__ JpegZigzag c_jpeg_zigzag = jpeg_make_zigzag();

struct JpegJobDev {
    const uint8_t* pixels;
    int64_t row_stride;
    uint64_t coef_first;                         // the file's first block in the coefficient array
    int32_t pixel_stride, width, height, kind, sub;
    uint32_t mcu_w, n_mcu, iv_first, n_iv, bpm, n_y;      // MCUs a row, MCUs, intervals, blocks an MCU, Y blocks an MCU
    uint16_t q[2][64];                           // natural order
};
struct JpegFileInfo {
    uint32_t hist[4][256];                       // DC0, AC0, DC1, AC1
    uint32_t code[4][256];                       // code | length << 16
    uint64_t data_bytes;
    uint32_t head_bytes, pad;
    uint8_t head[JPEG_HEAD_MAX];
};
struct JpegIvInfo { uint32_t nbytes, pad; uint64_t prefix; };

__device__ __forceinline__ int jpeg_job_of_interval(const JpegJobDev* jobs, int n_jobs, uint32_t iv) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].iv_first <= iv) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int32_t jpeg_dct_coef(int u, int x) {
    if (u == 0) return c_jpeg_k[4];
    const int a = ((2 * x + 1) * u) & 31;
    return a <= 8 ? c_jpeg_k[a] : a <= 16 ? -c_jpeg_k[16 - a] : a <= 24 ? -c_jpeg_k[a - 16] : c_jpeg_k[32 - a];
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of the pixel at (px, py), which lies inside the image
__device__ __forceinline__ int jpeg_component(const JpegJobDev& J, int px, int py, int comp) {
    const uint8_t* p = J.pixels + (int64_t)py * J.row_stride + (int64_t)px * J.pixel_stride;
    if (J.kind == PGR_JPEG_GRAY8) return gload(p);
    const int r = gload(p), g = gload(p + 1), b = gload(p + 2);
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// sample (x, y) of block j of an MCU, level-shifted
__device__ __forceinline__ int jpeg_sample(const JpegJobDev& J, uint32_t mcu, uint32_t j, int y, int x) {
    const int my = (int)(mcu / J.mcu_w), mx = (int)(mcu - (uint32_t)my * J.mcu_w);
    const int w1 = J.width - 1, h1 = J.height - 1;
    if (J.sub == PGR_JPEG_444) return jpeg_component(J, min(mx * 8 + x, w1), min(my * 8 + y, h1), (int)j) - 128;
    if (j < 4) return jpeg_component(J, min(mx * 16 + (int)(j & 1u) * 8 + x, w1), min(my * 16 + (int)(j >> 1) * 8 + y, h1), 0) - 128;
    const int comp = (int)j - 3, x0 = mx * 16 + 2 * x, y0 = my * 16 + 2 * y;
    const int sum = jpeg_component(J, min(x0, w1), min(y0, h1), comp) + jpeg_component(J, min(x0 + 1, w1), min(y0, h1), comp) +
                    jpeg_component(J, min(x0, w1), min(y0 + 1, h1), comp) + jpeg_component(J, min(x0 + 1, w1), min(y0 + 1, h1), comp);
    return ((sum + 2) >> 2) - 128;
}

// What lane `lane` of a wave that holds a block's 64 zigzag coefficients (position 0: the DC difference) sends: `zrl` ZRL
// symbols, then `symbol` with `extra` in `size` bits, if `coded`.  Lane 0 codes with the DC table.  All 64 lanes call it.
struct JpegToken { uint32_t zrl, symbol, size, extra; bool coded; };
__device__ __forceinline__ JpegToken jpeg_token(int v, int lane) {
    const uint64_t ac = __ballot(v != 0) & ~1ull;
    JpegToken t;
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    t.size = 32u - (uint32_t)__clz(a);
    t.extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << t.size) - 1u);
    t.zrl = 0;
    if (lane == 0) { t.symbol = t.size; t.coded = true; return t; }
    if (v != 0) {
        const uint64_t below = ac & ((1ull << lane) - 1ull);
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const uint32_t run = (uint32_t)(lane - prev - 1);
        t.zrl = run >> 4;
        t.symbol = ((run & 15u) << 4) | t.size;
        t.coded = true;
        return t;
    }
    t.symbol = 0;                                // EOB: the block's last coefficient is zero
    t.coded = lane == 63;
    return t;
}

__device__ __forceinline__ uint32_t jpeg_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

struct JpegBlocksLds {
    int16_t coef[JPEG_MAX_BLOCKS][64];           // zigzag order, DC as quantised
    uint32_t hist[4][256];
    uint16_t q[2][64];
    uint32_t job;
};

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_blocks_kernel(const JpegJobDev* __restrict__ jobs, int n_jobs,
                                                                    JpegFileInfo* __restrict__ finfo, int16_t* __restrict__ coefs) {
    __shared__ JpegBlocksLds L;
    const uint32_t tid = threadIdx.x, iv = blockIdx.x;
    const int lane = (int)(tid & (WAVE - 1)), wave = (int)(tid / WAVE);
    if (tid == 0) L.job = (uint32_t)jpeg_job_of_interval(jobs, n_jobs, iv);
    for (uint32_t i = tid; i < 4 * 256; i += JPEG_THREADS) (&L.hist[0][0])[i] = 0;
    __syncthreads();
    const JpegJobDev& J = jobs[L.job];
    if (tid < 128) (&L.q[0][0])[tid] = (&J.q[0][0])[tid];
    __syncthreads();
    const uint32_t bpm = J.bpm, n_y = J.n_y;
    const uint32_t mcu0 = (iv - J.iv_first) * JPEG_R;
    const uint32_t n_blocks = min((uint32_t)JPEG_R, J.n_mcu - mcu0) * bpm;
    int32_t cu[8], cv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { cu[i] = jpeg_dct_coef(lane & 7, i); cv[i] = jpeg_dct_coef(lane >> 3, i); }
    const uint32_t my_zz = c_jpeg_zigzag.zz_of_nat[lane];

    for (uint32_t b = (uint32_t)wave; b < n_blocks; b += JPEG_WAVES) {
        const uint32_t m = b / bpm, j = b - m * bpm;
        const int s = jpeg_sample(J, mcu0 + m, j, lane >> 3, lane & 7);
        int32_t t = 0;                           // lane (y, u)
#pragma unroll
        for (int x = 0; x < 8; ++x) t += cu[x] * __shfl(s, (lane & 56) | x, WAVE);
        int64_t F = 0;                           // lane (v, u)
#pragma unroll
        for (int y = 0; y < 8; ++y) F += (int64_t)cv[y] * (int64_t)__shfl(t, (y << 3) | (lane & 7), WAVE);
        const int32_t f = (int32_t)((F + (1ll << 27)) >> 28);
        const int32_t Q = L.q[j < n_y ? 0 : 1][lane];
        int32_t q = ((f < 0 ? -f : f) + (Q << 11)) / (Q << 12);
        if (lane != 0) q = min(q, 1023);
        L.coef[b][my_zz] = (int16_t)(f < 0 ? -q : q);
    }
    __syncthreads();

    int16_t* out = coefs + (J.coef_first + (uint64_t)mcu0 * bpm) * 64;
    for (uint32_t b = (uint32_t)wave; b < n_blocks; b += JPEG_WAVES) {
        const uint32_t m = b / bpm, j = b - m * bpm;
        int v = L.coef[b][lane];
        if (lane == 0) {
            // the previous block of the component inside the interval
            int prev = -1;
            if (j >= n_y) prev = (int)b - (int)bpm;
            else if (j > 0) prev = (int)b - 1;
            else if (m > 0) prev = (int)b - (int)bpm + (int)n_y - 1;
            v -= prev >= 0 ? (int)L.coef[prev][0] : 0;
            v = max(-2047, min(2047, v));
        }
        const JpegToken t = jpeg_token(v, lane);
        const uint32_t table = (j < n_y ? 0u : 2u) + (lane == 0 ? 0u : 1u);
        if (t.coded) atomicAdd(&L.hist[table][t.symbol], 1u);
        if (t.zrl) atomicAdd(&L.hist[table][0xF0], t.zrl);
        out[(uint64_t)b * 64 + lane] = (int16_t)v;
    }
    __syncthreads();
    uint32_t* hist = &finfo[L.job].hist[0][0];
    for (uint32_t i = tid; i < 4 * 256; i += JPEG_THREADS) {
        const uint32_t h = (&L.hist[0][0])[i];
        if (h) atomicAdd(&hist[i], h);
    }
}

// the bytes of a file's header into F.head; returns their count
__device__ inline uint32_t jpeg_write_head(const JpegJobDev& J, JpegFileInfo& F, const uint32_t* n_syms, const uint8_t (*counts)[17],
                                           const uint8_t (*syms)[256]) {
    uint8_t* h = F.head;
    uint32_t n = 0;
    const bool colour = J.kind == PGR_JPEG_RGB8;
    const uint32_t nc = colour ? 3 : 1, n_tab = colour ? 4 : 2;
    auto put = [&](uint32_t b) { if (n < (uint32_t)JPEG_HEAD_MAX) h[n] = (uint8_t)b; ++n; };
    auto put16 = [&](uint32_t v) { put(v >> 8); put(v & 255u); };
    put16(0xFFD8);
    put16(0xFFE0); put16(16); put('J'); put('F'); put('I'); put('F'); put(0); put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
    put16(0xFFDB); put16(2 + 65 * (colour ? 2 : 1));
    for (uint32_t t = 0; t < (colour ? 2u : 1u); ++t) {
        put(t);
        for (int k = 0; k < 64; ++k) put(J.q[t][c_jpeg_zigzag.nat_of_zz[k]]);
    }
    put16(0xFFC0); put16(8 + 3 * nc); put(8); put16((uint32_t)J.height); put16((uint32_t)J.width); put(nc);
    put(1); put(J.sub == PGR_JPEG_420 ? 0x22 : 0x11); put(0);
    if (colour) { put(2); put(0x11); put(1); put(3); put(0x11); put(1); }
    uint32_t dht = 2;
    for (uint32_t t = 0; t < n_tab; ++t) dht += 17 + n_syms[t];
    put16(0xFFC4); put16(dht);
    for (uint32_t t = 0; t < n_tab; ++t) {
        put(((t & 1u) << 4) | (t >> 1));         // class (0 DC, 1 AC) and identifier
        for (int l = 1; l <= 16; ++l) put(counts[t][l]);
        for (uint32_t i = 0; i < n_syms[t]; ++i) put(syms[t][i]);
    }
    put16(0xFFDD); put16(4); put16(JPEG_R);
    put16(0xFFDA); put16(6 + 2 * nc); put(nc); put(1); put(0x00);
    if (colour) { put(2); put(0x11); put(3); put(0x11); }
    put(0); put(63); put(0);
    return min(n, (uint32_t)JPEG_HEAD_MAX);
}

struct JpegTablesLds {
    uint32_t freq[4][JPEG_SYMBOLS + 3];
    uint32_t scratch[4][png_code_scratch_words(JPEG_SYMBOLS) + 1];
    uint32_t first[4][17], start[4][17], n_syms[4];
    uint8_t lens[4][JPEG_SYMBOLS + 3];
    uint8_t counts[4][17];                       // codes per length, without the pseudo-symbol (<= 255)
    uint8_t syms[4][256];                        // the DHT's symbols, by (length, symbol)
};

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_tables_kernel(const JpegJobDev* __restrict__ jobs, JpegFileInfo* __restrict__ finfo) {
    __shared__ JpegTablesLds L;
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & (WAVE - 1)), t = (int)(tid / WAVE);
    const JpegJobDev& J = jobs[blockIdx.x];
    JpegFileInfo& F = finfo[blockIdx.x];
    const bool live = t < (J.kind == PGR_JPEG_RGB8 ? 4 : 2);
    if (live) {
        uint32_t most = 0;
        for (int s = lane; s < 256; s += WAVE) most = max(most, F.hist[t][s]);
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) most = max(most, (uint32_t)__shfl_xor(most, d, WAVE));
        uint32_t k = 0;
        while ((((uint64_t)most + (1ull << k) - 1) >> k) > PNG_CODE_MAX_FREQ) ++k;
        for (int s = lane; s < 256; s += WAVE) L.freq[t][s] = (uint32_t)(((uint64_t)F.hist[t][s] + (1ull << k) - 1) >> k);
        if (lane == 0) L.freq[t][256] = 1;
    }
    __syncthreads();
    if (live && lane == 0) {
        uint8_t* lens = L.lens[t];
        png_code_lengths(L.freq[t], JPEG_SYMBOLS, 16, lens, L.scratch[t]);
        uint32_t longest = 0;
        for (int s = 0; s < JPEG_SYMBOLS; ++s) longest = max(longest, (uint32_t)lens[s]);
        if (lens[256] < longest) {
            int s = 255;
            while (lens[s] != longest) --s;      // (one exists: the pseudo-symbol does not hold that length)
            lens[s] = lens[256];
            lens[256] = (uint8_t)longest;
        }
        uint32_t count[17];
        for (int l = 0; l <= 16; ++l) count[l] = 0;
        for (int s = 0; s < 256; ++s) count[lens[s]]++;
        uint32_t code = 0, at = 0;
        for (int l = 1; l <= 16; ++l) {
            L.first[t][l] = code;
            L.start[t][l] = at;
            L.counts[t][l] = (uint8_t)count[l];
            code = (code + count[l]) << 1;
            at += count[l];
        }
        L.n_syms[t] = at;
    }
    __syncthreads();
    if (live) {
        for (int s = lane; s < 256; s += WAVE) {
            const uint32_t l = L.lens[t][s];
            uint32_t rank = 0;
            for (int i = 0; i < s; ++i) rank += L.lens[t][i] == l;
            F.code[t][s] = l ? ((L.first[t][l] + rank) | (l << 16)) : 0u;
            if (l) L.syms[t][L.start[t][l] + rank] = (uint8_t)s;
        }
    }
    __syncthreads();
    if (tid == 0) {
        F.head_bytes = jpeg_write_head(J, F, L.n_syms, L.counts, L.syms);
        F.pad = 0;
    }
}

// value's low `bits` (1 .. 32) bits into the image at bit `pos`, first bit in a word's bit 31
__device__ __forceinline__ void jpeg_put_bits(uint32_t* img, uint32_t pos, uint32_t value, uint32_t bits) {
    if (bits == 0 || (pos >> 5) + 1 >= (uint32_t)JPEG_IMG_WORDS) return;        // (JPEG_BLOCK_BITS keeps every interval inside)
    const uint64_t x = (uint64_t)value << (64u - (pos & 31u) - bits);
    atomicOr(&img[pos >> 5], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&img[(pos >> 5) + 1], (uint32_t)x);
}
__device__ __forceinline__ uint32_t jpeg_img_byte(const uint32_t* img, uint32_t i) { return (img[i >> 2] >> (24u - 8u * (i & 3u))) & 255u; }

struct JpegScanLds {
    uint32_t img[JPEG_IMG_WORDS];
    uint32_t code[4][256];
    uint32_t block_at[JPEG_MAX_BLOCKS + 1];
    uint32_t wave_sum[JPEG_WAVES];
    uint32_t job;
};
static_assert(sizeof(JpegScanLds) <= 40 * 1024 && sizeof(JpegBlocksLds) <= 40 * 1024, "at least two workgroups per CU, with room");

// One workgroup per interval.  EMIT: a byte of file k is stored at files[offsets[k] + rel] only for 0 <= rel < min(offsets[k+1],
// total) - offsets[k] and offsets[k] >= 0: no store leaves the file's range whatever the device-side offsets or the workspace hold.
template <bool EMIT>
__global__ void __launch_bounds__(JPEG_THREADS) jpeg_scan_kernel(const JpegJobDev* __restrict__ jobs, int n_jobs,
                                                                  const JpegFileInfo* __restrict__ finfo, JpegIvInfo* __restrict__ info,
                                                                  const int16_t* __restrict__ coefs, const long long* __restrict__ offsets,
                                                                  long long total, uint8_t* __restrict__ files) {
    __shared__ JpegScanLds L;
    const uint32_t tid = threadIdx.x, iv = blockIdx.x;
    const int lane = (int)(tid & (WAVE - 1)), wave = (int)(tid / WAVE);
    if (tid == 0) L.job = (uint32_t)jpeg_job_of_interval(jobs, n_jobs, iv);
    for (uint32_t i = tid; i < JPEG_IMG_WORDS; i += JPEG_THREADS) L.img[i] = 0;
    __syncthreads();
    const uint32_t job = L.job;
    const JpegJobDev& J = jobs[job];
    const JpegFileInfo& F = finfo[job];
    for (uint32_t i = tid; i < 4 * 256; i += JPEG_THREADS) (&L.code[0][0])[i] = (&F.code[0][0])[i];
    const uint32_t bpm = J.bpm, n_y = J.n_y, iv_in = iv - J.iv_first;
    const uint32_t mcu0 = iv_in * JPEG_R;
    const uint32_t n_blocks = min((uint32_t)JPEG_R, J.n_mcu - mcu0) * bpm;
    const int16_t* in = coefs + (J.coef_first + (uint64_t)mcu0 * bpm) * 64;
    __syncthreads();

    // the bits of each block
    for (uint32_t b = (uint32_t)wave; b < n_blocks; b += JPEG_WAVES) {
        const uint32_t j = b % bpm;
        const JpegToken t = jpeg_token(in[(uint64_t)b * 64 + lane], lane);
        const uint32_t* code = L.code[(j < n_y ? 0u : 2u) + (lane == 0 ? 0u : 1u)];
        const uint32_t bits = t.coded ? t.zrl * (code[0xF0] >> 16) + (code[t.symbol] >> 16) + t.size : 0u;
        const uint32_t sum = jpeg_wave_sum(bits);
        if (lane == 0) L.block_at[b + 1] = min(sum, (uint32_t)JPEG_BLOCK_BITS);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t at = 0;
        L.block_at[0] = 0;
        for (uint32_t b = 1; b <= n_blocks; ++b) { at += L.block_at[b]; L.block_at[b] = at; }
        if (at & 7u) jpeg_put_bits(L.img, at, (1u << (8u - (at & 7u))) - 1u, 8u - (at & 7u));       // 1-bits to the byte
    }
    __syncthreads();
    for (uint32_t b = (uint32_t)wave; b < n_blocks; b += JPEG_WAVES) {
        const uint32_t j = b % bpm;
        const JpegToken t = jpeg_token(in[(uint64_t)b * 64 + lane], lane);
        const uint32_t* code = L.code[(j < n_y ? 0u : 2u) + (lane == 0 ? 0u : 1u)];
        const uint32_t zrl = code[0xF0], c = code[t.symbol];
        const uint32_t bits = t.coded ? t.zrl * (zrl >> 16) + (c >> 16) + t.size : 0u;
        uint32_t incl = bits;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += o;
        }
        uint32_t pos = L.block_at[b] + incl - bits;
        if (t.coded) {
            for (uint32_t z = 0; z < t.zrl; ++z) { jpeg_put_bits(L.img, pos, zrl & 0xFFFFu, zrl >> 16); pos += zrl >> 16; }
            jpeg_put_bits(L.img, pos, ((c & 0xFFFFu) << t.size) | t.extra, (c >> 16) + t.size);
        }
    }
    __syncthreads();

    // stuffing: a chunk of the image's bytes per thread
    const uint32_t n_plain = (L.block_at[n_blocks] + 7u) >> 3;
    const uint32_t c0 = min(tid * JPEG_CHUNK, n_plain), c1 = min(c0 + JPEG_CHUNK, n_plain);
    uint32_t ff = 0;
    for (uint32_t i = c0; i < c1; ++i) ff += jpeg_img_byte(L.img, i) == 255u;
    uint32_t n_ff;
    const uint32_t ff_before = png_block_scan(ff, L.wave_sum, n_ff);
    if (!EMIT) {
        if (tid == 0) {
            JpegIvInfo r;
            r.nbytes = n_plain + n_ff + 2;       // and RSTm or EOI
            r.pad = 0;
            r.prefix = 0;
            info[iv] = r;
        }
        return;
    }
    const long long lo = offsets[job], hi = min(offsets[job + 1], total);
    if (lo < 0 || hi <= lo) return;
    const uint64_t room = (uint64_t)(hi - lo);
    uint8_t* file = files + lo;
    const uint32_t head_bytes = min(F.head_bytes, (uint32_t)JPEG_HEAD_MAX);
    const uint64_t at = (uint64_t)head_bytes + info[iv].prefix;
    uint64_t rel = at + c0 + ff_before;
    for (uint32_t i = c0; i < c1; ++i) {
        const uint32_t v = jpeg_img_byte(L.img, i);
        if (rel >= at && rel < room) file[rel] = (uint8_t)v;
        ++rel;
        if (v == 255u) {
            if (rel >= at && rel < room) file[rel] = 0;
            ++rel;
        }
    }
    if (tid == 0) {
        const uint64_t m = at + n_plain + n_ff;
        if (m >= at && m < room) file[m] = 0xFF;
        if (m + 1 >= at && m + 1 < room) file[m + 1] = (uint8_t)(iv_in + 1 == J.n_iv ? 0xD9u : 0xD0u + (iv_in & 7u));
    }
    if (iv_in == 0)
        for (uint32_t i = tid; i < head_bytes; i += JPEG_THREADS)
            if (i < room) file[i] = F.head[i];
}

// One workgroup per file: where each interval starts behind the header, and the file's size.
__global__ void __launch_bounds__(JPEG_THREADS) jpeg_finish_kernel(const JpegJobDev* __restrict__ jobs, JpegIvInfo* __restrict__ info,
                                                                    JpegFileInfo* __restrict__ finfo, long long* __restrict__ sizes) {
    __shared__ uint32_t wave_sum[JPEG_WAVES];
    const uint32_t tid = threadIdx.x;
    const JpegJobDev& J = jobs[blockIdx.x];
    JpegIvInfo* ivs = info + J.iv_first;
    const uint32_t n_iv = J.n_iv;
    uint64_t data = 0;
    for (uint32_t base = 0; base < n_iv; base += JPEG_THREADS) {
        const uint32_t i = base + tid;
        const uint32_t v = i < n_iv ? ivs[i].nbytes : 0;
        uint32_t sum;
        const uint32_t at = png_block_scan(v, wave_sum, sum);
        if (i < n_iv) ivs[i].prefix = data + at;
        data += sum;
    }
    if (tid == 0) {
        finfo[blockIdx.x].data_bytes = data;
        sizes[blockIdx.x] = (long long)(finfo[blockIdx.x].head_bytes + data);
    }
}

}  // namespace pgr
