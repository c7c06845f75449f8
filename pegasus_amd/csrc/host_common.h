// host_common.h -- what the host side of every translation unit of libpegasus_raster.so shares: the HIP error string
// behind pgr_last_hip_error, the workspace carver and the small casts every entry repeats.  Host code only: no kernel,
// no device function (DESIGN.md "Source layout").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/pegasus_raster.h"

namespace pgr {

inline thread_local char g_hip_error[256] = "";      // one object for the whole library (pgr_last_hip_error reads it)

inline bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    snprintf(g_hip_error, sizeof(g_hip_error), "%s: %s", what, hipGetErrorString(e));
    return false;
}

// How an entry ends behind its launches: `what` names them in pgr_last_hip_error.
inline int32_t launch_status(const char* what) { return hip_ok(hipGetLastError(), what) ? PGR_OK : PGR_ERR_LAUNCH_FAILURE; }

// The C ABI passes a stream as void*.
inline hipStream_t as_stream(void* stream_v) { return static_cast<hipStream_t>(stream_v); }

// The T* at a byte offset of a workspace.
template <typename T> T* ws_at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
template <typename T> const T* ws_at(const void* base, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }

constexpr size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Hands out consecutive slices of a buffer, each aligned to 256 B; a slice of zero bytes still takes one unit.  So no layout
// is empty, and the layout functions that check their sizing arguments themselves return one whose total is 0 for "refused".
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align_up(bytes ? bytes : 1); return o; }
};

// What the evaluation entries (masks, COCO scores) ask of a workspace pointer: their kernels read and write it in 16-byte and
// 8-byte elements at the carved offsets.  And the most workgroups one launch of theirs may have: grid.x is 31 bits.
inline bool workspace_aligned_16(const void* workspace) { return reinterpret_cast<uintptr_t>(workspace) % 16 == 0; }
constexpr int64_t MAX_GRID_BLOCKS = 0x7fffffff;

}  // namespace pgr
