#!/bin/bash
# tools/fuzz_png_host.cpp under ASan + UBSan over files of every colour type and bit depth, written by the tests' own PNG
# writer (CPU only, ~1 min):
#   bash tools/fuzz_png_host.sh [iters-per-file] > profiles/rNN_fuzz_png_host.txt
set -eu
cd "$(dirname "$0")/.."
T=$(mktemp -d)
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
    -Ifennec_amd/csrc tools/fuzz_png_host.cpp fennec_amd/csrc/png_parse.cpp -o "$T/fuzz"
python - "$T" <<'P'
import sys
sys.path.insert(0, "tests")
import png_decode_ref as ref
k = 0
for ct, depth in ref.PAIRS:
    s = ref.random_samples(23, 70, ct, depth, k)
    pal = ref.random_palette(1 << min(depth, 8), k) if ct == 3 else None
    trns = bytes(range(1 << min(depth, 8))) if ct == 3 else bytes(2) if ct == 0 else bytes(6) if ct == 2 else None
    filters = [(y * 7 + k) % 5 for y in range(70)]
    open(f"{sys.argv[1]}/f{k:02d}.png", "wb").write(ref.write_png(s, ct, depth, filters=filters, palette=pal, trns=trns,
                                                                  idat_sizes=[1, 50] if k % 2 else None, level=(0, 1, 6, 9)[k % 4]))
    k += 1
P
ASAN_OPTIONS=detect_leaks=1 "$T/fuzz" "${1:-20000}" "$T"/f*.png
rm -rf "$T"
