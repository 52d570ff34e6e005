// fennec_amd/csrc/jpeg_layout.hpp on the CPU, against a plain walk of writer.go's loops: for every mode and every w x h of a
// list, the MCUs in raster order, each MCU's blocks in writeSOS's order (4:2:0: Y at (0,0) (1,0) (0,1) (1,1), Cb, Cr; 4:4:4: Y, Cb,
// Cr), a running scan position and a per-component "previous block".  The header's functions must give, for every block, the
// position the walk gives it (jpeg_scan_index: a bijection onto 0 .. blocks - 1), the component's class (jpeg_slot_class) and the
// distance to the component's previous block (jpeg_slot_prev; the first block of a component has none: the distance then
// points in front of the image).  Prints one line per case, "w h mode mx my blocks"; exit 1 and a message on a mismatch.
//   jpeg_layout_hostsim [w h ...]      (default: a sweep of 1..40 x 1..40 and a few large sizes)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_layout.hpp"

using namespace fnx;

static int check(int mode, int w, int h)
{
    int ys, yh, cs, ch, mx, my;
    jpeg_layout_dims(mode, w, h, &ys, &yh, &cs, &ch, &mx, &my);
    const int m = jpeg_mcu_px(mode), per = jpeg_mcu_blocks(mode), hy = m / 8;
    if (mx != (w + m - 1) / m || my != (h + m - 1) / m || ys != m * mx || yh != m * my || cs != 8 * mx || ch != 8 * my) {
        std::printf("dims of %d x %d in mode %d\n", w, h, mode);
        return 1;
    }
    const int n = jpeg_scan_blocks(mode, mx, my);
    if (n != mx * my * (hy * hy + 2)) {
        std::printf("blocks of %d x %d in mode %d: %d\n", w, h, mode, n);
        return 1;
    }
    std::vector<char> seen(static_cast<size_t>(n), 0);
    int pos = 0, last[3] = {-1, -1, -1};
    for (int my0 = 0; my0 < my; my0++)
        for (int mx0 = 0; mx0 < mx; mx0++)
            for (int j = 0; j < per; j++, pos++) {
                const int comp = j < hy * hy ? 0 : j - hy * hy + 1;
                const int bx = comp == 0 ? hy * mx0 + (j % hy) : mx0, by = comp == 0 ? hy * my0 + (j / hy) : my0;
                const int at = jpeg_scan_index(mode, mx, comp, bx, by);
                if (at != pos || at < 0 || at >= n || seen[static_cast<size_t>(at)]) {
                    std::printf("%d x %d mode %d: block (%d, %d) of component %d is at %d, the walk is at %d\n", w, h, mode, bx, by, comp, at, pos);
                    return 1;
                }
                seen[static_cast<size_t>(at)] = 1;
                if (pos % per != j || jpeg_slot_class(mode, j) != (comp != 0)) {
                    std::printf("%d x %d mode %d: slot %d of component %d has class %d\n", w, h, mode, j, comp, jpeg_slot_class(mode, j));
                    return 1;
                }
                const int prev = pos - jpeg_slot_prev(mode, j);
                if (last[comp] < 0 ? prev >= 0 : prev != last[comp]) {
                    std::printf("%d x %d mode %d: position %d (component %d) predicts from %d, the walk from %d\n", w, h, mode, pos, comp, prev, last[comp]);
                    return 1;
                }
                last[comp] = pos;
            }
    if (jpeg_ycbcr_ratio(mode) != (mode == JPEG_444 ? 0 : 2) || jpeg_y_sampling(mode) != ((hy << 4) | hy)) {
        std::printf("ratio or sampling byte of mode %d\n", mode);
        return 1;
    }
    std::printf("%d %d %d %d %d %d\n", w, h, mode, mx, my, n);
    return 0;
}

int main(int argc, char **argv)
{
    std::vector<int> dims;
    for (int i = 1; i + 1 < argc; i += 2) {
        dims.push_back(std::atoi(argv[i]));
        dims.push_back(std::atoi(argv[i + 1]));
    }
    if (dims.empty()) {
        for (int h = 1; h <= 40; h++)
            for (int w = 1; w <= 40; w++) {
                dims.push_back(w);
                dims.push_back(h);
            }
        const int large[] = {264, 24, 24, 520, 528, 40, 3840, 2160, 65535, 1, 1, 65535, 4097, 4095};
        dims.insert(dims.end(), large, large + sizeof(large) / sizeof(large[0]));
    }
    for (size_t i = 0; i + 1 < dims.size(); i += 2) {
        if (dims[i] < 1 || dims[i] > 65535 || dims[i + 1] < 1 || dims[i + 1] > 65535) {
            std::printf("not a JPEG size: %d x %d\n", dims[i], dims[i + 1]);
            return 1;
        }
        for (int mode : {JPEG_420, JPEG_444})
            if (check(mode, dims[i], dims[i + 1])) return 1;
    }
    return 0;
}
