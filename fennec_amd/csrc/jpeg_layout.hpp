// The layout of the JPEG files this library writes, stated once for host and device code: what a chroma subsampling mode
// (fnx_ctx_set_jpeg_subsampling) means for the planes' padding, the MCU, the scan order and the per-component DC prediction.
// Plain functions of the mode; the kernels that need them are templated on the mode, so every call folds to the constants the
// 4:2:0 code always had.  (tools/jpeg_layout_hostsim holds them against a plain walk of writer.go's loops on the CPU.)
//   4:2:0 (mode 0): MCU = 16 x 16 px = Y00 Y01 Y10 Y11 Cb Cr; Y padded to 16, Cb / Cr half size
//   4:4:4 (mode 1): MCU =  8 x  8 px = Y Cb Cr;               every plane padded to 8
#pragma once

#if defined(__HIPCC__)
#define FNX_LAYOUT_FN __host__ __device__ inline
#else
#define FNX_LAYOUT_FN inline
#endif

namespace fnx {

constexpr int JPEG_420 = 0, JPEG_444 = 1;      // FNX_JPEG_SUBSAMPLING_420 / _444

// pixels an MCU covers each way; blocks it holds
FNX_LAYOUT_FN int jpeg_mcu_px(int mode) { return mode == JPEG_444 ? 8 : 16; }
FNX_LAYOUT_FN int jpeg_mcu_blocks(int mode) { return mode == JPEG_444 ? 3 : 6; }
// the image.YCbCrSubsampleRatio the file decodes to (convert.hip's `ratio`): 4:2:0 is 2, 4:4:4 is 0
FNX_LAYOUT_FN int jpeg_ycbcr_ratio(int mode) { return mode == JPEG_444 ? 0 : 2; }
// the Y component's sampling byte in SOF0 (Cb and Cr are 0x11 in both modes)
FNX_LAYOUT_FN int jpeg_y_sampling(int mode) { return mode == JPEG_444 ? 0x11 : 0x22; }

// the planes of a w x h image: Y ys x yh, Cb / Cr cs x ch; *mx x *my MCUs
FNX_LAYOUT_FN void jpeg_layout_dims(int mode, int w, int h, int *ys, int *yh, int *cs, int *ch, int *mx, int *my)
{
    const int m = jpeg_mcu_px(mode);
    *mx = (w + m - 1) / m; *my = (h + m - 1) / m;
    *ys = m * *mx; *yh = m * *my; *cs = 8 * *mx; *ch = 8 * *my;
}

// blocks of the whole scan
FNX_LAYOUT_FN int jpeg_scan_blocks(int mode, int mx, int my) { return mx * my * jpeg_mcu_blocks(mode); }

// the scan position of block (bx, by) of `plane` (0 Y, 1 Cb, 2 Cr), MCUs in raster order (writer.go writeSOS)
FNX_LAYOUT_FN int jpeg_scan_index(int mode, int mx, int plane, int bx, int by)
{
    if (mode == JPEG_444) return (by * mx + bx) * 3 + plane;
    return plane == 0 ? ((by >> 1) * mx + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1) : (by * mx + bx) * 6 + 3 + plane;
}

// For the block at scan position i of its image, j = i % jpeg_mcu_blocks(mode) its place inside the MCU:
// the Huffman class (0 luminance, 1 chrominance) ...
FNX_LAYOUT_FN int jpeg_slot_class(int mode, int j) { return mode == JPEG_444 ? (j != 0) : (j >= 4); }
// ... and how many scan positions back its component's previous block lies (behind the image's first block: prediction 0)
FNX_LAYOUT_FN int jpeg_slot_prev(int mode, int j)
{
    if (mode == JPEG_444) return 3;
    return j == 0 ? 3 : (j < 4 ? 1 : 6);
}

}  // namespace fnx
