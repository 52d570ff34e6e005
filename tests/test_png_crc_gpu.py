"""fnx_ctx_set_png_crc on the GPU: every route that makes a PNG file from a device deflate writes, with the IDAT chunk's CRC
taken from crc32.hip's kernels ("device"), the bytes it writes with the host's CRC ("host") -- same ctx, both deflate levels --
and every chunk's CRC is zlib.crc32's (png_filter_ref.chunks checks each one)."""
from __future__ import annotations

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as pf
from fennec_amd import FNX_CRC_PIECE, FNX_FORMAT_PNG, FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED

pytestmark = pytest.mark.gpu

SIZES = ((5, 3), (67, 7), (1031, 37))
KINDS = ("rgb", "rgba", "gray", "pal8", "pal1")
LEVELS = ("fast", "dense")


@pytest.fixture(scope="module")
def ctx():
    c = fennec_amd.Context(0)
    yield c
    c.set_png_crc("host")
    c.set_deflate_level("fast")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def source(kind, w, h, content, seed):
    """(src, FNX_PNG_* kind, ncolors, palette) for png_encode: noise, or gradients with no noise at all"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind in ("rgb", "rgba"):
        if content == "noise":
            img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        else:
            img = (np.stack([x * 3 + y, x + y * 2, x + 40, 255 - x // 2], axis=-1) & 255).astype(np.uint8)
        if kind == "rgb":
            img[..., 3] = 255
        else:
            img[0, 0, 3] = 7
        return np.ascontiguousarray(img), FNX_PNG_NRGBA, 0, None
    n = {"gray": 256, "pal8": 200, "pal1": 2}[kind]
    plane = rng.integers(0, n, (h, w)).astype(np.uint8) if content == "noise" else ((x // 3 + y) % n).astype(np.uint8)
    if kind == "gray":
        return plane, FNX_PNG_GRAY, 0, None
    pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pal[n // 2:, 3] = 255
    return plane, FNX_PNG_PALETTED, n, pal


def encode(ctx, src, kind, ncolors, pal):
    return ctx.png_encode(dev(src), kind, ncolors, -1, pal)


def both_modes(ctx, make):
    """make() under "host", then under "device": (host's value, device's value, the kernel list after each)"""
    ctx.set_png_crc("host")
    a = make()
    ka = ctx.last_kernel()
    ctx.set_png_crc("device")
    b = make()
    kb = ctx.last_kernel()
    ctx.set_png_crc("host")
    return a, b, ka, kb


@pytest.mark.parametrize("level", LEVELS)
def test_png_encode_every_kind_size_and_content(ctx, level):
    ctx.set_deflate_level(level)
    idat = {}
    for kind in KINDS:
        for w, h in SIZES:
            for content in ("noise", "smooth"):
                src = source(kind, w, h, content, 3)
                host, device, kh, kd = both_modes(ctx, lambda: encode(ctx, *src))
                assert device == host, (kind, w, h, content, len(host), len(device))
                chunks = pf.chunks(device)                              # every chunk's CRC against zlib.crc32
                assert [t for t, _ in chunks][0] == b"IHDR" and [t for t, _ in chunks][-2:] == [b"IDAT", b"IEND"]
                assert "crc32_pieces_kernel" in kd and "crc32" not in kh
                assert kd.split(", ")[0] == kh
                idat[kind, w, h, content] = len(dict(chunks)[b"IDAT"])
    # the noise RGBA stream is stored and crosses two piece boundaries; the smooth one stays inside a piece
    assert idat["rgba", 1031, 37, "noise"] > 37 * (1 + 4 * 1031) > 2 * FNX_CRC_PIECE
    assert idat["rgba", 1031, 37, "smooth"] < FNX_CRC_PIECE
    ctx.set_deflate_level("fast")


def batch_images(n):
    """n images of mixed kinds and sizes, a 1 x 1 one among them: the streams start at every byte alignment"""
    rng = np.random.default_rng(n)
    out = []
    for i in range(n):
        w, h = ((1, 1), (5, 3), (67, 7), (9, 5), (130, 41), (3, 11), (1031, 37))[i % 7]
        which = i % 4
        if which == 0:
            img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)                       # RGBA noise
        elif which == 1:
            img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)                       # RGB noise
            img[..., 3] = 255
        elif which == 2:
            v = rng.integers(0, 2 + i, (h, w)).astype(np.uint8)                       # a few colours: paletted (or grey)
            img = np.stack([v, v * 3 & 255, v, np.full_like(v, 255)], axis=-1)
        else:
            y, x = np.mgrid[0:h, 0:w]
            v = ((x + y) & 255).astype(np.uint8)                                       # grey gradient
            img = np.stack([v, v, v, np.full_like(v, 255)], axis=-1)
        out.append(np.ascontiguousarray(img))
    return out


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", (1, 3, 33))
def test_compress_batch(ctx, level, n):
    ctx.set_deflate_level(level)
    imgs = [dev(a) for a in batch_images(n)]
    (fh, kh_), (fd, kd_), kh, kd = both_modes(ctx, lambda: ctx.png_compress_batch(imgs))
    assert fd == fh and kd_ == kh_
    assert "crc32_pieces_batch_kernel" in kd and "crc32" not in kh and kd.startswith(kh)
    ctx.set_png_crc("device")
    for i, t in enumerate(imgs):
        assert fd[i] == ctx.compress_png(t, device_deflate=True), i       # the single route's file, under "device" too
        pf.chunks(fd[i])
    ctx.set_png_crc("host")
    starts = np.cumsum([0] + [len(dict(pf.chunks(f))[b"IDAT"]) for f in fd[:-1]])
    if n == 33:
        assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    ctx.set_deflate_level("fast")


def test_recompress_batch_on_two_small_files(ctx):
    files = [ctx.compress_png(dev(a), device_deflate=True) for a in (batch_images(3)[2], pf.smooth_rgba(19, 6, 1, opaque=False))]
    (fh, kh_, sh), (fd, kd_, sd), kh, kd = both_modes(ctx, lambda: ctx.png_recompress_batch(files))
    assert sh == sd == [fennec_amd.FNX_OK] * 2 and kd_ == kh_
    assert fd == fh and all(f is not None for f in fd)
    for f in fd:
        pf.chunks(f)
    assert "crc32_pieces_batch_kernel" in kd and "crc32" not in kh


def test_hit_target_size_png(ctx):
    img = pf.smooth_rgba(64, 64, 4)
    gh, gd, kh, kd = both_modes(ctx, lambda: ctx.hit_target_size(img, 1 << 20, FNX_FORMAT_PNG))
    assert gh["status"] == gd["status"] == fennec_amd.FNX_OK and gh["winner"] == gd["winner"]
    assert gd["data"] == gh["data"] and gd["data"][:8] == b"\x89PNG\r\n\x1a\n"
    pf.chunks(gd["data"])
    assert "crc32_pieces_kernel" in kd and "crc32" not in kh


def test_back_to_host_the_files_are_still_equal(ctx):
    src = source("rgba", 67, 7, "noise", 9)
    ctx.set_png_crc("device")
    device = encode(ctx, *src)
    assert "crc32_pieces_kernel" in ctx.last_kernel()
    ctx.set_png_crc("host")
    host = encode(ctx, *src)
    assert "crc32" not in ctx.last_kernel() and host == device
    with pytest.raises(fennec_amd.FennecError):
        ctx.set_png_crc("both")
    with pytest.raises(fennec_amd.FennecError):
        ctx.set_png_crc(2)
