// io.hip -- host side of the image-file entries of libpegasus_raster.so: PNG and JPEG files of device images, undistortion
// of a COLMAP project's images and points.
// Owns its kernel headers: no other translation unit includes them (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_common.h"
#include "png.hip.h"
#include "jpeg.hip.h"
#include "undistort.hip.h"

using namespace pgr;

// ---- PNG encoding (png.hip.h, png_codes.h) ------------------------------------------------------------------------------------
namespace {
constexpr int32_t PNG_MAX_SIDE = 16384;
int png_bytes_per_pixel(int32_t kind) { return kind == PGR_PNG_GRAY8 ? 1 : kind == PGR_PNG_RGB8 ? 3 : kind == PGR_PNG_GRAY16 ? 2 : 0; }
bool png_shape_ok(int32_t width, int32_t height, int32_t kind) {
    return width >= 1 && width <= PNG_MAX_SIDE && height >= 1 && height <= PNG_MAX_SIDE && png_bytes_per_pixel(kind) != 0;
}
// what the sizing needs of a job; pgr_png_encode also asks for its pixels
bool png_job_ok(const PgrPngJob& j) {
    if (!png_shape_ok(j.width, j.height, j.kind)) return false;
    const int bpp = png_bytes_per_pixel(j.kind);
    if (j.scale != 1 && !(j.scale == 255 && j.kind == PGR_PNG_GRAY8)) return false;
    return j.pixel_stride >= bpp && j.row_stride >= (int64_t)(j.width - 1) * j.pixel_stride + bpp;
}
int64_t png_raw_bytes(int32_t width, int32_t height, int32_t kind) {
    return (int64_t)height * (1 + (int64_t)width * png_bytes_per_pixel(kind));
}
int64_t png_segments(int64_t raw_bytes) { return (raw_bytes + PNG_S - 1) / PNG_S; }

// the encoder's workspace: the job table, one record per file, one per segment, one slot per segment
struct PngLayout { size_t jobs, files, info, slots, total; int64_t n_segs; };
PngLayout png_layout(int32_t n_jobs, const PgrPngJob* jobs) {
    PngLayout L{};
    if (n_jobs <= 0 || !jobs) return L;
    int64_t segs = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (!png_job_ok(jobs[k])) return L;
        segs += png_segments(png_raw_bytes(jobs[k].width, jobs[k].height, jobs[k].kind));
    }
    if (segs > MAX_GRID_BLOCKS) return L;
    Carver c;
    L.jobs = c.take((size_t)n_jobs * sizeof(PngJobDev));
    L.files = c.take((size_t)n_jobs * sizeof(PngFileInfo));
    L.info = c.take((size_t)segs * sizeof(PngSegInfo));
    L.slots = c.take((size_t)segs * PNG_SLOT_BYTES);
    L.total = c.off;
    L.n_segs = segs;
    return L;
}
}  // namespace

size_t pgr_png_workspace_bytes(int32_t n_jobs, const PgrPngJob* jobs) { return png_layout(n_jobs, jobs).total; }

int64_t pgr_png_max_bytes(int32_t width, int32_t height, int32_t kind) {
    if (!png_shape_ok(width, height, kind)) return 0;
    const int64_t raw = png_raw_bytes(width, height, kind);
    return PNG_HEAD_BYTES + PNG_TAIL_BYTES + raw + 5 * png_segments(raw);
}

int32_t pgr_png_code_lengths(const uint32_t* freq, int32_t n, int32_t limit, uint8_t* lengths) {
    if (!freq || !lengths || n < 1 || n > PNG_CODE_MAX_SYMBOLS || limit < 1 || limit > 15 || n > (1 << limit)) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t s = 0; s < n; ++s)
        if (freq[s] > PNG_CODE_MAX_FREQ) return PGR_ERR_INVALID_ARGUMENT;
    uint32_t scratch[png_code_scratch_words(PNG_CODE_MAX_SYMBOLS)];
    png_code_lengths(freq, n, limit, lengths, scratch);
    return PGR_OK;
}

int32_t pgr_png_encode(const PgrPngJob* jobs, int32_t n_jobs, int32_t level, int64_t* sizes, void* workspace, size_t workspace_bytes,
                       void* stream_v) {
    if (n_jobs < 0 || (level != 0 && level != 1)) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const PngLayout L = png_layout(n_jobs, jobs);
    if (!L.total || !sizes || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_jobs; ++k)
        if (!jobs[k].pixels) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    std::vector<PngJobDev> table((size_t)n_jobs);
    uint32_t seg = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrPngJob& j = jobs[k];
        PngJobDev& d = table[(size_t)k];
        d.pixels = static_cast<const uint8_t*>(j.pixels);
        d.row_stride = j.row_stride;
        d.raw_bytes = (uint64_t)png_raw_bytes(j.width, j.height, j.kind);
        d.pixel_stride = j.pixel_stride; d.width = j.width; d.height = j.height; d.kind = j.kind; d.scale = j.scale;
        d.row_len = (uint32_t)(1 + j.width * png_bytes_per_pixel(j.kind));
        d.seg_first = seg;
        d.n_segs = (uint32_t)png_segments((int64_t)d.raw_bytes);
        seg += d.n_segs;
    }
    hipStream_t stream = as_stream(stream_v);
    auto* jobs_dev = ws_at<PngJobDev>(workspace, L.jobs);
    // in stream order, and read when this returns: the caller may free its table after the call
    if (!hip_ok(hipMemcpyWithStream(jobs_dev, table.data(), table.size() * sizeof(PngJobDev), hipMemcpyHostToDevice, stream),
                "memcpy png jobs"))
        return PGR_ERR_LAUNCH_FAILURE;
    auto* info = ws_at<PngSegInfo>(workspace, L.info);
    png_encode_kernel<<<(unsigned)L.n_segs, PNG_THREADS, 0, stream>>>(jobs_dev, n_jobs, level, info, ws_at<uint8_t>(workspace, L.slots));
    png_finish_kernel<<<(unsigned)n_jobs, PNG_FINISH_THREADS, 0, stream>>>(jobs_dev, info, ws_at<PngFileInfo>(workspace, L.files),
                                                                          reinterpret_cast<long long*>(sizes));
    return launch_status("png_encode launch");
}

int32_t pgr_png_emit(const PgrPngJob* jobs, int32_t n_jobs, const int64_t* offsets, int64_t total, uint8_t* files, int64_t capacity,
                     const void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const PngLayout L = png_layout(n_jobs, jobs);
    if (!L.total || !offsets || !files || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    // every file has its 63 framing bytes and a segment, and none exceeds its bound
    int64_t most = 0;
    for (int32_t k = 0; k < n_jobs; ++k) most += pgr_png_max_bytes(jobs[k].width, jobs[k].height, jobs[k].kind);
    if (total <= (int64_t)(PNG_HEAD_BYTES + PNG_TAIL_BYTES) * n_jobs || total > most || capacity < total) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    png_emit_kernel<<<(unsigned)L.n_segs, PNG_EMIT_THREADS, 0, as_stream(stream_v)>>>(
        ws_at<const PngJobDev>(workspace, L.jobs), n_jobs, (uint32_t)L.n_segs, ws_at<const PngSegInfo>(workspace, L.info),
        ws_at<const PngFileInfo>(workspace, L.files), ws_at<const uint8_t>(workspace, L.slots),
        reinterpret_cast<const long long*>(offsets), (long long)total, files);
    return launch_status("png_emit launch");
}

// ---- JPEG encoding (jpeg.hip.h) -----------------------------------------------------------------------------------------------
namespace {
constexpr int32_t JPEG_MAX_SIDE = 16384;
constexpr int64_t JPEG_BLOCK_BYTES = 2 * ((JPEG_BLOCK_BITS + 7) / 8);      // every byte of a block's bits stuffed
constexpr int64_t JPEG_MIN_BYTES = 120;                                     // less than any header and its EOI

// ITU-T T.81 Annex K, tables K.1 and K.2, in natural order: what PIL writes at quality 50 --
//   python -c "from PIL import Image; Image.new('RGB', (8, 8)).save('q50.jpg', quality=50); print(Image.open('q50.jpg').quantization)"
constexpr uint8_t JPEG_BASE_LUM[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                       14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                       18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t JPEG_BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                          99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
int jpeg_quant(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    return std::min(255, std::max(1, (base * s + 50) / 100));
}

bool jpeg_shape_ok(int32_t width, int32_t height, int32_t kind, int32_t sub) {
    return width >= 1 && width <= JPEG_MAX_SIDE && height >= 1 && height <= JPEG_MAX_SIDE &&
           ((kind == PGR_JPEG_GRAY8 && sub == PGR_JPEG_444) || (kind == PGR_JPEG_RGB8 && (sub == PGR_JPEG_444 || sub == PGR_JPEG_420)));
}
bool jpeg_job_ok(const PgrJpegJob& j) {
    if (!jpeg_shape_ok(j.width, j.height, j.kind, j.subsampling) || j.quality < 1 || j.quality > 100) return false;
    const int bpp = j.kind == PGR_JPEG_GRAY8 ? 1 : 3;
    return j.pixel_stride >= bpp && j.row_stride >= (int64_t)(j.width - 1) * j.pixel_stride + bpp;
}
// MCUs a row, MCUs, restart intervals and blocks of a shape inside the domain
struct JpegShape { int64_t mcu_w, n_mcu, n_iv, bpm, n_y; };
JpegShape jpeg_shape(int32_t width, int32_t height, int32_t kind, int32_t sub) {
    const int side = sub == PGR_JPEG_420 ? 16 : 8;
    JpegShape s;
    s.mcu_w = (width + side - 1) / side;
    s.n_mcu = s.mcu_w * ((height + side - 1) / side);
    s.n_iv = (s.n_mcu + JPEG_R - 1) / JPEG_R;
    s.n_y = sub == PGR_JPEG_420 ? 4 : 1;
    s.bpm = kind == PGR_JPEG_GRAY8 ? 1 : s.n_y + 2;
    return s;
}

// the encoder's workspace: the job table, one record per file and per interval, the coefficients
struct JpegLayout { size_t jobs, files, info, coefs, total; int64_t n_iv; };
JpegLayout jpeg_layout(int32_t n_jobs, const PgrJpegJob* jobs) {
    JpegLayout L{};
    if (n_jobs <= 0 || !jobs) return L;
    int64_t ivs = 0, blocks = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        if (!jpeg_job_ok(jobs[k])) return L;
        const JpegShape s = jpeg_shape(jobs[k].width, jobs[k].height, jobs[k].kind, jobs[k].subsampling);
        ivs += s.n_iv;
        blocks += s.n_mcu * s.bpm;
    }
    if (ivs > MAX_GRID_BLOCKS) return L;
    Carver c;
    L.jobs = c.take((size_t)n_jobs * sizeof(JpegJobDev));
    L.files = c.take((size_t)n_jobs * sizeof(JpegFileInfo));
    L.info = c.take((size_t)ivs * sizeof(JpegIvInfo));
    L.coefs = c.take((size_t)blocks * 64 * sizeof(int16_t));
    L.total = c.off;
    L.n_iv = ivs;
    return L;
}
}  // namespace

size_t pgr_jpeg_workspace_bytes(int32_t n_jobs, const PgrJpegJob* jobs) { return jpeg_layout(n_jobs, jobs).total; }

int64_t pgr_jpeg_max_bytes(int32_t width, int32_t height, int32_t kind, int32_t subsampling) {
    if (!jpeg_shape_ok(width, height, kind, subsampling)) return 0;
    const JpegShape s = jpeg_shape(width, height, kind, subsampling);
    return (kind == PGR_JPEG_GRAY8 ? 330 : 613) + JPEG_BLOCK_BYTES * s.n_mcu * s.bpm + 2 * s.n_iv;
}

int32_t pgr_jpeg_quant_tables(int32_t quality, uint8_t* lum, uint8_t* chroma) {
    if (quality < 1 || quality > 100 || !lum || !chroma) return PGR_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 64; ++i) {
        lum[i] = (uint8_t)jpeg_quant(JPEG_BASE_LUM[i], quality);
        chroma[i] = (uint8_t)jpeg_quant(JPEG_BASE_CHROMA[i], quality);
    }
    return PGR_OK;
}

int32_t pgr_jpeg_encode(const PgrJpegJob* jobs, int32_t n_jobs, int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const JpegLayout L = jpeg_layout(n_jobs, jobs);
    if (!L.total || !sizes || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < n_jobs; ++k)
        if (!jobs[k].pixels) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    std::vector<JpegJobDev> table((size_t)n_jobs);
    uint32_t iv = 0;
    uint64_t block = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrJpegJob& j = jobs[k];
        const JpegShape s = jpeg_shape(j.width, j.height, j.kind, j.subsampling);
        JpegJobDev& d = table[(size_t)k];
        d.pixels = static_cast<const uint8_t*>(j.pixels);
        d.row_stride = j.row_stride;
        d.coef_first = block;
        d.pixel_stride = j.pixel_stride; d.width = j.width; d.height = j.height; d.kind = j.kind; d.sub = j.subsampling;
        d.mcu_w = (uint32_t)s.mcu_w; d.n_mcu = (uint32_t)s.n_mcu; d.iv_first = iv; d.n_iv = (uint32_t)s.n_iv;
        d.bpm = (uint32_t)s.bpm; d.n_y = (uint32_t)s.n_y;
        for (int i = 0; i < 64; ++i) {
            d.q[0][i] = (uint16_t)jpeg_quant(JPEG_BASE_LUM[i], j.quality);
            d.q[1][i] = (uint16_t)jpeg_quant(JPEG_BASE_CHROMA[i], j.quality);
        }
        iv += d.n_iv;
        block += (uint64_t)(s.n_mcu * s.bpm);
    }
    hipStream_t stream = as_stream(stream_v);
    auto* jobs_dev = ws_at<JpegJobDev>(workspace, L.jobs);
    auto* files = ws_at<JpegFileInfo>(workspace, L.files);
    auto* info = ws_at<JpegIvInfo>(workspace, L.info);
    auto* coefs = ws_at<int16_t>(workspace, L.coefs);
    // in stream order, and read when this returns: the caller may free its table after the call
    if (!hip_ok(hipMemcpyWithStream(jobs_dev, table.data(), table.size() * sizeof(JpegJobDev), hipMemcpyHostToDevice, stream),
                "memcpy jpeg jobs") ||
        !hip_ok(hipMemsetAsync(files, 0, (size_t)n_jobs * sizeof(JpegFileInfo), stream), "memset jpeg histograms"))
        return PGR_ERR_LAUNCH_FAILURE;
    jpeg_blocks_kernel<<<(unsigned)L.n_iv, JPEG_THREADS, 0, stream>>>(jobs_dev, n_jobs, files, coefs);
    jpeg_tables_kernel<<<(unsigned)n_jobs, JPEG_THREADS, 0, stream>>>(jobs_dev, files);
    jpeg_scan_kernel<false><<<(unsigned)L.n_iv, JPEG_THREADS, 0, stream>>>(jobs_dev, n_jobs, files, info, coefs, nullptr, 0, nullptr);
    jpeg_finish_kernel<<<(unsigned)n_jobs, JPEG_THREADS, 0, stream>>>(jobs_dev, info, files, reinterpret_cast<long long*>(sizes));
    return launch_status("jpeg_encode launch");
}

int32_t pgr_jpeg_emit(const PgrJpegJob* jobs, int32_t n_jobs, const int64_t* offsets, int64_t total, uint8_t* files, int64_t capacity,
                      const void* workspace, size_t workspace_bytes, void* stream_v) {
    if (n_jobs < 0) return PGR_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return PGR_OK;
    const JpegLayout L = jpeg_layout(n_jobs, jobs);
    if (!L.total || !offsets || !files || !workspace || !workspace_aligned_16(workspace)) return PGR_ERR_INVALID_ARGUMENT;
    int64_t most = 0;
    for (int32_t k = 0; k < n_jobs; ++k) most += pgr_jpeg_max_bytes(jobs[k].width, jobs[k].height, jobs[k].kind, jobs[k].subsampling);
    if (total <= JPEG_MIN_BYTES * n_jobs || total > most || capacity < total) return PGR_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < L.total) return PGR_ERR_WORKSPACE_TOO_SMALL;
    // the scan kernel only reads the workspace when it emits
    jpeg_scan_kernel<true><<<(unsigned)L.n_iv, JPEG_THREADS, 0, as_stream(stream_v)>>>(
        ws_at<const JpegJobDev>(workspace, L.jobs), n_jobs, ws_at<const JpegFileInfo>(workspace, L.files),
        const_cast<JpegIvInfo*>(ws_at<const JpegIvInfo>(workspace, L.info)), ws_at<const int16_t>(workspace, L.coefs),
        reinterpret_cast<const long long*>(offsets), (long long)total, files);
    return launch_status("jpeg_emit launch");
}

// ---- undistortion (undistort.hip.h) ---------------------------------------------------------------------------------------------
namespace {
constexpr int32_t UND_MAX_SIDE = 32768;

// a COLMAP model id and its parameters in COLMAP's order as the kernels' camera; false for a model outside the rule or
// focal lengths that do not divide
bool und_camera(int32_t model, const double* p, UndCam& c, int& kind) {
    if (!p) return false;
    c = UndCam{};
    int n_k = 0, first_k = 0;
    switch (model) {
        case 0: kind = UND_PINHOLE; c.fx = c.fy = p[0]; c.cx = p[1]; c.cy = p[2]; break;
        case 1: kind = UND_PINHOLE; c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3]; break;
        case 2: kind = UND_SIMPLE_RADIAL; c.fx = c.fy = p[0]; c.cx = p[1]; c.cy = p[2]; first_k = 3; n_k = 1; break;
        case 3: kind = UND_RADIAL; c.fx = c.fy = p[0]; c.cx = p[1]; c.cy = p[2]; first_k = 3; n_k = 2; break;
        case 4: kind = UND_OPENCV; c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3]; first_k = 4; n_k = 4; break;
        case 5: kind = UND_FISHEYE; c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3]; first_k = 4; n_k = 4; break;
        case 6: kind = UND_FULL_OPENCV; c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3]; first_k = 4; n_k = 8; break;
        default: return false;
    }
    for (int i = 0; i < n_k; ++i) c.k[i] = p[first_k + i];
    for (int i = 0; i < n_k; ++i)
        if (!std::isfinite(c.k[i])) return false;
    return std::isfinite(c.fx) && std::isfinite(c.fy) && c.fx != 0.0 && c.fy != 0.0 && std::isfinite(c.cx) && std::isfinite(c.cy);
}

int und_channel_slot(int32_t channels) { return channels == 1 ? 0 : channels == 3 ? 1 : channels == 4 ? 2 : -1; }

// what both image entries ask of a job: two images that lie inside their strides
bool und_images_ok(const PgrUndistortJob& j) {
    const int32_t c = j.channels;
    return j.src && j.dst && und_channel_slot(c) >= 0 && j.src_width >= 1 && j.src_width <= UND_MAX_SIDE && j.src_height >= 1 &&
           j.src_height <= UND_MAX_SIDE && j.dst_width >= 1 && j.dst_width <= UND_MAX_SIDE && j.dst_height >= 1 &&
           j.dst_height <= UND_MAX_SIDE && j.src_stride >= (int64_t)j.src_width * c && j.dst_stride >= (int64_t)j.dst_width * c;
}

void und_job_images(const PgrUndistortJob& j, UndJobDev& d, uint32_t& blocks) {
    d.src = static_cast<const uint8_t*>(j.src); d.dst = static_cast<uint8_t*>(j.dst);
    d.src_stride = j.src_stride; d.dst_stride = j.dst_stride;
    d.sw = j.src_width; d.sh = j.src_height; d.dw = j.dst_width; d.dh = j.dst_height;
    d.block0 = blocks;
    d.blocks_x = (uint32_t)((j.dst_width + UND_BLOCK_W - 1) / UND_BLOCK_W);
    blocks += d.blocks_x * (uint32_t)((j.dst_height + UND_ROWS - 1) / UND_ROWS);
}

using UndImageKernel = void (*)(const UndJobTable);
template <int M> constexpr UndImageKernel und_remap_row(int slot) {
    return slot == 0 ? und_remap_kernel<M, 1> : slot == 1 ? und_remap_kernel<M, 3> : und_remap_kernel<M, 4>;
}
UndImageKernel und_remap_fn(int kind, int slot) {
    switch (kind) {
        case UND_PINHOLE: return und_remap_row<UND_PINHOLE>(slot);
        case UND_SIMPLE_RADIAL: return und_remap_row<UND_SIMPLE_RADIAL>(slot);
        case UND_RADIAL: return und_remap_row<UND_RADIAL>(slot);
        case UND_OPENCV: return und_remap_row<UND_OPENCV>(slot);
        case UND_FULL_OPENCV: return und_remap_row<UND_FULL_OPENCV>(slot);
        default: return und_remap_row<UND_FISHEYE>(slot);
    }
}

// the launches of one group of jobs (those of `pick`): a table of at most UND_JOBS_PER_LAUNCH jobs per launch
template <typename Pick, typename Fill>
void und_launch_group(UndImageKernel fn, int32_t n_jobs, const PgrUndistortJob* jobs, int32_t factor, Pick pick, Fill fill,
                      hipStream_t stream) {
    UndJobTable T{};
    T.factor = factor;
    uint32_t blocks = 0;
    for (int32_t k = 0; k <= n_jobs; ++k) {
        if (k < n_jobs && pick(k)) {
            UndJobDev& d = T.job[T.count++];
            und_job_images(jobs[k], d, blocks);
            fill(k, d);
        }
        if (T.count == UND_JOBS_PER_LAUNCH || (k == n_jobs && T.count > 0)) {
            fn<<<blocks, UND_THREADS, 0, stream>>>(T);
            T.count = 0;
            blocks = 0;
        }
    }
}
}  // namespace

int32_t pgr_undistort_points(int32_t model, const double* params, int64_t n, const double* xy, double* uv, uint8_t* ok,
                             void* stream_v) {
    UndCam c;
    int kind = 0;
    if (n < 0 || !und_camera(model, params, c, kind) || (n > 0 && (!xy || !uv)) || (n + UND_THREADS - 1) / UND_THREADS > MAX_GRID_BLOCKS)
        return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    const unsigned blocks = (unsigned)((n + UND_THREADS - 1) / UND_THREADS);
    hipStream_t stream = as_stream(stream_v);
    switch (kind) {
        case UND_PINHOLE: und_points_kernel<UND_PINHOLE><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
        case UND_SIMPLE_RADIAL: und_points_kernel<UND_SIMPLE_RADIAL><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
        case UND_RADIAL: und_points_kernel<UND_RADIAL><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
        case UND_OPENCV: und_points_kernel<UND_OPENCV><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
        case UND_FULL_OPENCV: und_points_kernel<UND_FULL_OPENCV><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
        default: und_points_kernel<UND_FISHEYE><<<blocks, UND_THREADS, 0, stream>>>(c, n, xy, uv, ok); break;
    }
    return launch_status("undistort_points launch");
}

int32_t pgr_distort_points(int32_t model, const double* params, int64_t n, const double* uv, double* xy, void* stream_v) {
    UndCam c;
    int kind = 0;
    if (n < 0 || !und_camera(model, params, c, kind) || (n > 0 && (!uv || !xy)) || (n + UND_THREADS - 1) / UND_THREADS > MAX_GRID_BLOCKS)
        return PGR_ERR_INVALID_ARGUMENT;
    if (n == 0) return PGR_OK;
    const unsigned blocks = (unsigned)((n + UND_THREADS - 1) / UND_THREADS);
    hipStream_t stream = as_stream(stream_v);
    switch (kind) {
        case UND_PINHOLE: und_distort_kernel<UND_PINHOLE><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
        case UND_SIMPLE_RADIAL: und_distort_kernel<UND_SIMPLE_RADIAL><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
        case UND_RADIAL: und_distort_kernel<UND_RADIAL><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
        case UND_OPENCV: und_distort_kernel<UND_OPENCV><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
        case UND_FULL_OPENCV: und_distort_kernel<UND_FULL_OPENCV><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
        default: und_distort_kernel<UND_FISHEYE><<<blocks, UND_THREADS, 0, stream>>>(c, n, uv, xy); break;
    }
    return launch_status("distort_points launch");
}

int32_t pgr_undistort_images(const PgrUndistortJob* jobs, int32_t n_jobs, void* stream_v) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return PGR_ERR_INVALID_ARGUMENT;
    std::vector<UndCam> cams((size_t)n_jobs);
    std::vector<int> group((size_t)n_jobs);                   // model kind * 3 + channel slot
    bool present[UND_MODELS * 3] = {};
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrUndistortJob& j = jobs[k];
        int kind = 0;
        if (!und_images_ok(j) || !und_camera(j.model, j.params, cams[(size_t)k], kind)) return PGR_ERR_INVALID_ARGUMENT;
        for (int i = 0; i < 4; ++i)
            if (!std::isfinite(j.pinhole[i])) return PGR_ERR_INVALID_ARGUMENT;
        if (j.pinhole[0] == 0.0 || j.pinhole[1] == 0.0) return PGR_ERR_INVALID_ARGUMENT;
        group[(size_t)k] = kind * 3 + und_channel_slot(j.channels);
        present[group[(size_t)k]] = true;
    }
    hipStream_t stream = as_stream(stream_v);
    for (int g = 0; g < UND_MODELS * 3; ++g) {
        if (!present[g]) continue;
        und_launch_group(und_remap_fn(g / 3, g % 3), n_jobs, jobs, 0, [&](int32_t k) { return group[(size_t)k] == g; },
                         [&](int32_t k, UndJobDev& d) {
                             d.cam = cams[(size_t)k];
                             d.pfx = jobs[k].pinhole[0]; d.pfy = jobs[k].pinhole[1]; d.pcx = jobs[k].pinhole[2]; d.pcy = jobs[k].pinhole[3];
                         }, stream);
    }
    return n_jobs == 0 ? PGR_OK : launch_status("undistort_images launch");
}

int32_t pgr_image_box_downscale(const PgrUndistortJob* jobs, int32_t n_jobs, int32_t factor, void* stream_v) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs) || (factor != 2 && factor != 4 && factor != 8)) return PGR_ERR_INVALID_ARGUMENT;
    bool present[3] = {};
    for (int32_t k = 0; k < n_jobs; ++k) {
        const PgrUndistortJob& j = jobs[k];
        if (!und_images_ok(j) || (int64_t)j.dst_width * factor > j.src_width || (int64_t)j.dst_height * factor > j.src_height)
            return PGR_ERR_INVALID_ARGUMENT;
        present[und_channel_slot(j.channels)] = true;
    }
    hipStream_t stream = as_stream(stream_v);
    const UndImageKernel fns[3] = {und_box_kernel<1>, und_box_kernel<3>, und_box_kernel<4>};
    for (int s = 0; s < 3; ++s) {
        if (!present[s]) continue;
        und_launch_group(fns[s], n_jobs, jobs, factor, [&](int32_t k) { return und_channel_slot(jobs[k].channels) == s; },
                         [](int32_t, UndJobDev&) {}, stream);
    }
    return n_jobs == 0 ? PGR_OK : launch_status("image_box_downscale launch");
}
