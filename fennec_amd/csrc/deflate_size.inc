// deflate.hip's SIZE-ONLY kernels, included into it behind the emitting ones (it needs their DeflateArgs, df_block_sum and the
// chunk bodies): the two chunk kernels' size-only forms and the one-workgroup sum that stands where the gather stood
// (fnx_png_encoded_size, the PNG target-size legs' "how many bytes?"; DESIGN.md section 5.15).

// The same parse and the same choice of form as deflate_chunk_kernel, then the chunk's byte count into meta[0] and nothing else --
// no codes, no bits, no slot (a.slots is not read).
__global__ __launch_bounds__(DF_T) void deflate_chunk_size_kernel(DeflateArgs a)
{
#define DF_CHUNK_INDEX blockIdx.x
#define DF_SIZE_ONLY 1
#include "deflate_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_CHUNK_INDEX
}

__global__ __launch_bounds__(DF_T) void deflate_dense_chunk_size_kernel(DeflateArgs a)   // the dense level's size-only form
{
#define DF_CHUNK_INDEX blockIdx.x
#define DF_STREAM_POS base
#define DF_SIZE_ONLY 1
#include "deflate_dense_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_STREAM_POS
#undef DF_CHUNK_INDEX
}

// The size-only form's gather: ONE workgroup adds the chunks' byte counts (meta word 0 of each) and the six bytes of header and
// Adler-32 into the result word -- a sum of integers: any order gives the same value.
__global__ __launch_bounds__(DF_T) void deflate_size_kernel(const uint32_t *meta, uint32_t nchunks, unsigned long long *result)
{
    __shared__ unsigned long long s_red[4];
    unsigned long long all = 0;
    for (uint32_t j = threadIdx.x; j < nchunks; j += DF_T) all += meta[4 * static_cast<size_t>(j)];
    all = df_block_sum(all, s_red);
    if (threadIdx.x == 0) *result = 2 + all + 4;
}
