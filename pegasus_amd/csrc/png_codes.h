// png_codes.h -- the integer rules of the PNG encoder that host and device share: the length-limited code builder, the
// deflate symbol tables and the CRC-32 / Adler-32 algebra.  No kernel and no __constant__ table: any translation unit may
// include it (DESIGN.md "Source layout"); the kernels are in png.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgr {

constexpr int PNG_CODE_MAX_SYMBOLS = 288;            // the largest alphabet the builder takes
constexpr uint32_t PNG_CODE_MAX_FREQ = 1u << 22;     // and the largest count: 288 of them still sum below 2^31
// uint32 words of scratch the builder needs for an alphabet of n symbols
constexpr int png_code_scratch_words(int n) { return 2 * n + 17; }

// Code lengths of a prefix code for the symbols with freq != 0, none longer than `limit`; 0 for unused symbols.
//   no used symbol   -> all 0 (the caller sends one zero length: HDIST = 0)
//   one used symbol  -> length 1 (the one incomplete code inflate accepts, for a lone distance symbol)
//   two or more      -> a COMPLETE code: sum of 2^-length is exactly 1, which inflate demands of every other code
// The code is Huffman's (Moffat and Katajainen's in-place construction on the sorted counts) when that fits `limit`.  When it
// does not, lengths beyond the limit are cut to it and the Kraft sum is brought back to 1 one unit of 2^-limit at a time: a
// code of the limit leaves, the deepest code above the limit moves one level down and takes the leaver as its sibling.  Then
// the lengths are handed out again in order of the counts, the rarest symbol the longest.  If that costs more than the flat
// complete code (2^L - used symbols at L - 1 bits, the rest at L = ceil(log2(used)) bits), the flat code is taken: the result
// never costs more than ceil(log2(used)) bits for every used symbol.  Ties between equal counts go by symbol index, so host
// and device build the same code.  Preconditions (the callers check them): 1 <= n <= 288, 1 <= limit <= 16 (deflate's callers
// pass 15 and 7, the JPEG encoder 16), n <= 2^limit,
// freq[s] <= 2^22.  `scratch`: png_code_scratch_words(n) words (LDS on the device: the function keeps no array of its own).
__host__ __device__ inline void png_code_lengths(const uint32_t* freq, int n, int limit, uint8_t* lengths, uint32_t* scratch) {
    uint32_t* w = scratch;             // sorted keys, then weights / parents, then depths
    uint32_t* sym = scratch + n;       // the symbols in that order
    uint32_t* num = scratch + 2 * n;   // codes per length
    int m = 0;
    for (int s = 0; s < n; ++s) {
        lengths[s] = 0;
        if (freq[s]) w[m++] = (freq[s] << 9) | (uint32_t)s;
    }
    if (m == 0) return;
    if (m == 1) { lengths[w[0] & 511u] = 1; return; }
    // heapsort, ascending by (count, symbol): the keys are distinct
    for (int start = m / 2 - 1, end = m; end > 1;) {
        int root;
        if (start >= 0) root = start--;
        else { --end; const uint32_t t = w[0]; w[0] = w[end]; w[end] = t; root = 0; }
        const uint32_t v = w[root];
        for (;;) {
            int child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && w[child + 1] > w[child]) ++child;
            if (w[child] <= v) break;
            w[root] = w[child];
            root = child;
        }
        w[root] = v;
    }
    for (int i = 0; i < m; ++i) { sym[i] = w[i] & 511u; w[i] >>= 9; }
    // Huffman depths in place: internal node weights, then parent indices, then depths (w[0] ends as the rarest symbol's)
    w[0] += w[1];
    for (int root = 0, leaf = 2, next = 1; next < m - 1; ++next) {
        if (leaf >= m || w[root] < w[leaf]) { w[next] = w[root]; w[root++] = (uint32_t)next; }
        else w[next] = w[leaf++];
        if (leaf >= m || (root < next && w[root] < w[leaf])) { w[next] += w[root]; w[root++] = (uint32_t)next; }
        else w[next] += w[leaf++];
    }
    w[m - 2] = 0;
    for (int next = m - 3; next >= 0; --next) w[next] = w[w[next]] + 1;
    for (int avail = 1, used = 0, depth = 0, root = m - 2, next = m - 1; avail > 0;) {
        while (root >= 0 && (int)w[root] == depth) { ++used; --root; }
        while (avail > used) { w[next--] = (uint32_t)depth; --avail; }
        avail = 2 * used;
        ++depth;
        used = 0;
    }
    // the limit
    for (int l = 0; l <= 16; ++l) num[l] = 0;
    for (int i = 0; i < m; ++i) num[w[i] < (uint32_t)limit ? w[i] : (uint32_t)limit]++;
    uint32_t kraft = 0;                                        // in units of 2^-limit
    for (int l = 1; l <= limit; ++l) kraft += num[l] << (limit - l);
    while (kraft > (1u << limit) && num[limit] > 0) {
        num[limit]--;
        for (int l = limit - 1; l > 0; --l)
            if (num[l]) { num[l]--; num[l + 1] += 2; break; }
        --kraft;
    }
    uint64_t cost = 0;
    for (int l = limit, i = 0; l > 0; --l)
        for (uint32_t c = 0; c < num[l]; ++c, ++i) { lengths[sym[i]] = (uint8_t)l; cost += (uint64_t)freq[sym[i]] * (uint32_t)l; }
    // the flat complete code
    int L = 1;
    while ((1 << L) < m) ++L;
    const int n_short = (1 << L) - m;                          // the most frequent symbols: one bit less
    uint64_t flat = 0;
    for (int i = 0; i < m; ++i) flat += (uint64_t)freq[sym[i]] * (uint32_t)(i >= m - n_short ? L - 1 : L);
    if (flat < cost)
        for (int i = 0; i < m; ++i) lengths[sym[i]] = (uint8_t)(i >= m - n_short ? L - 1 : L);
}

// ---- deflate's symbol tables (RFC 1951 3.2.5, 3.2.6) as arithmetic ---------------------------------------------------------
constexpr int PNG_LITLEN_SYMBOLS = 286, PNG_DIST_SYMBOLS = 30, PNG_CL_SYMBOLS = 19;
constexpr int PNG_MIN_MATCH = 3, PNG_MAX_MATCH = 258;

// length 3..258 -> symbol 257..285, its extra bits and their value
__host__ __device__ inline void png_length_symbol(uint32_t len, uint32_t& symbol, uint32_t& extra_bits, uint32_t& extra) {
    const uint32_t l = len - 3;
    if (l < 8 || l == 255) { symbol = l == 255 ? 285 : 257 + l; extra_bits = 0; extra = 0; return; }
    uint32_t msb = 3;
    while ((l >> (msb + 1)) != 0) ++msb;
    extra_bits = msb - 2;
    symbol = 261 + 4 * extra_bits + ((l >> extra_bits) & 3u);
    extra = l & ((1u << extra_bits) - 1);
}
// distance 1..32768 -> symbol 0..29, its extra bits and their value
__host__ __device__ inline void png_dist_symbol(uint32_t dist, uint32_t& symbol, uint32_t& extra_bits, uint32_t& extra) {
    const uint32_t d = dist - 1;
    if (d < 4) { symbol = d; extra_bits = 0; extra = 0; return; }
    uint32_t msb = 2;
    while ((d >> (msb + 1)) != 0) ++msb;
    extra_bits = msb - 1;
    symbol = 2 * msb + ((d >> extra_bits) & 1u);
    extra = d & ((1u << extra_bits) - 1);
}
// the fixed code's lengths (3.2.6): index < 288 literal/length, 288 + s distance symbol s
__host__ __device__ inline uint32_t png_fixed_length(int index) {
    return index < 144 ? 8 : index < 256 ? 9 : index < 280 ? 7 : index < 288 ? 8 : 5;
}

// ---- checksums -------------------------------------------------------------------------------------------------------------
// CRC-32 (reflected, polynomial EDB88320): a register holds a polynomial over GF(2) with x^0 in bit 31.
//   crc(AB) = crc(A) * x^(8 len B) mod P  xor  crc(B)            (zlib's crc32_combine; the pre- and post-inversion cancel)
// Adler-32 of a concatenation, both halves started at (1, 0):   A = A1 + A2 - 1,  B = B1 + B2 + len2 * (A1 - 1)   (mod 65521)
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;
constexpr uint32_t PNG_ADLER_MOD = 65521u;
constexpr uint32_t PNG_GF_ONE = 0x80000000u;

__host__ __device__ constexpr uint32_t png_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (PNG_GF_ONE >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);          // times x
    }
    return p;
}
struct PngX8Table { uint32_t pow[32]; };                       // x^(8 * 2^k) mod P
constexpr PngX8Table png_make_x8_table() {
    PngX8Table t{};
    uint32_t p = PNG_GF_ONE >> 8;
    for (int k = 0; k < 32; ++k) { t.pow[k] = p; p = png_gf_mul(p, p); }
    return t;
}
// x^(8 * bytes) mod P
__host__ __device__ inline uint32_t png_x8_pow(const uint32_t* table, uint64_t bytes) {
    uint32_t r = PNG_GF_ONE;
    for (int k = 0; k < 32 && (bytes >> k) != 0; ++k)
        if ((bytes >> k) & 1u) r = png_gf_mul(r, table[k]);
    return r;
}
// one byte into an (inverted) CRC register
__host__ __device__ constexpr uint32_t png_crc_byte(uint32_t reg, uint32_t byte) {
    reg ^= byte;
    for (int i = 0; i < 8; ++i) reg = (reg >> 1) ^ ((reg & 1u) ? PNG_CRC_POLY : 0u);
    return reg;
}

}  // namespace pgr
