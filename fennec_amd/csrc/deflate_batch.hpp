// What deflate.hip's batched kernels read, and the stream's bound -- plain C++ (no HIP word), so that the planner of the PNG
// compress batch (png_compress_plan.cpp) and the CPU build of deflate.hip (tools/deflate_hostsim) take it as it is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fennec_hip.h"

namespace fnx {

inline size_t deflate_chunks(size_t n) { return n ? (n + FNX_DEFLATE_CHUNK - 1) / FNX_DEFLATE_CHUNK : 1; }

// every chunk stored (5 bytes of block header) and closed by the empty stored block (5), the zlib header and the Adler-32
inline size_t deflate_bound(size_t n) { return n + 10 * deflate_chunks(n) + 6; }

// a chunk's output slot: the stored bound (chunk + 10), dword reads one past the end
constexpr int DEFLATE_SLOT_BYTES = FNX_DEFLATE_CHUNK + 32;

// the match-distance hint as the chunk kernel takes it: a row length inside a chunk, else none
inline int deflate_row_hint(long long row) { return row > 0 && row < FNX_DEFLATE_CHUNK ? static_cast<int>(row) : 0; }

// deflate_chunk_batch_kernel: one workgroup per unit -- a chunk of up to FNX_DEFLATE_CHUNK bytes of one stream of the batch
struct DeflateBatchUnit {
    const uint8_t *src;                  // DEVICE: the chunk's first byte
    uint32_t len;                        // 1 .. FNX_DEFLATE_CHUNK
    int32_t row;                         // deflate_row_hint of its stream
    uint32_t last;                       // the stream's last chunk: it carries BFINAL
    uint32_t image;                      // whose stream
};
// deflate_gather_batch_kernel: a stream's units lie back to back, [chunk0, chunk0 + nchunks)
struct DeflateBatchImage {
    unsigned long long n;                // the stream's input bytes
    uint32_t chunk0, nchunks;
};

}  // namespace fnx
