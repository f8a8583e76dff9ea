// The argument checks the file decoders' C entries share (png_decode.hip egs_png_decode_ex, jpeg_decode.hip egs_jpeg_decode_phases).
// Host code only, plain C++17: tests/decode_args_host.cpp compiles it with the host compiler under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/egs_raster.h"

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// The opening check of an entry, after the checks of its own arguments: the counts (n_second is the entry's second count: IDAT chunks,
// restart intervals), the NULL pointers, the alignments -- scratch 16, status 4, the device copy of the descriptors 8, the device copy of
// the second table second_align (a power of two).  -> 0, EGS_ERR_ARG or EGS_ERR_RANGE, in the order the entries document.
inline int decode_open(int n_files, int n_second, const void* files, const void* desc_host, const void* desc_device, const void* second_host,
                       const void* second_device, uintptr_t second_align, const void* out, const void* status, const void* scratch) {
    if (n_files < 1 || n_second < 1) return EGS_ERR_ARG;
    if (n_files > 65535) return EGS_ERR_RANGE;
    if (!files || !desc_host || !desc_device || !second_host || !second_device || !out || !status || !scratch) return EGS_ERR_ARG;
    if (((uintptr_t)scratch & 15) || ((uintptr_t)status & 3) || ((uintptr_t)desc_device & 7) || ((uintptr_t)second_device & (second_align - 1)))
        return EGS_ERR_ARG;
    return 0;
}

// One region of a packed buffer: `room` bytes at `offset` must start at or behind *end (ascending, no overlap with the region before),
// at a multiple of `align` (a power of two), and lie inside the buffer's `limit` bytes.  Sizes first, then offset > limit - room: no sum
// that could wrap.  Accepted: *end moves behind the region.  -> whether the region is accepted.
inline bool decode_region(uint64_t offset, uint64_t room, uint64_t align, uint64_t limit, size_t* end) {
    if ((offset & (align - 1)) || offset < *end || room > limit || offset > limit - room) return false;
    *end = (size_t)(offset + room);
    return true;
}
