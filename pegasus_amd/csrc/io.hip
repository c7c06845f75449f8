// io.hip -- host side of the file-format entries of libpegasus_raster.so: PNG files of device images.
// Owns its kernel header: no other translation unit includes it (DESIGN.md "Source layout").
#include <hip/hip_runtime.h>

#include <vector>

#include "host_common.h"
#include "png.hip.h"

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
