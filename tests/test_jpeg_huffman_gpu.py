"""FNX_JPEG_HUFFMAN_OPTIMIZED on the GPU (-m gpu): jpeg_hufftab_kernel's tables and jpeg_symhist_kernel's counts against the
plain-Python statement of the rule (tests/jpeg_hufftab_ref.py), the files byte for byte against jpeg_craft's writer with those
tables, both size-query routes, the searches, the batch -- and the standard mode's bytes again after switching back."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import fennec_amd
import jpeg_hufftab_ref as ref
from oracle import oracle as orc

PROF_JPEG = 16
ONE_WAIT, TWO_STEP = "jpeg_ffcount_strips_kernel", "jpeg_pack_kernel"
QUALITIES = (1, 50, 75, 100)


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture()
def opt(ctx):
    ctx.set_jpeg_huffman("optimized")
    yield ctx
    ctx.set_jpeg_huffman("standard")


def _images():
    """name -> (image, qualities): the plain images at four qualities, the crafted sheets at the quality they were made for"""
    out = {name: (np.ascontiguousarray(img), QUALITIES) for name, img in ref.plain_images().items()}
    out.update({name: (np.ascontiguousarray(img), (q,)) for name, (img, q) in ref.crafted_images().items()})
    return out


@functools.lru_cache(None)
def _expected(name, quality):
    """(standard file, coefficients, optimised file, crafted scan) of one image at one quality: computed once, never changed"""
    img = _all_images()[name]
    std, coef = orc.jpeg_encode(img, quality, with_coefficients=True)
    data, crafted, _ = ref.optimized_file(std, coef, img.shape[1], img.shape[0])
    return std, coef, data, crafted


@functools.lru_cache(None)
def _all_images():
    out = {name: img for name, (img, _) in _images().items()}
    out["sizes_48x40"] = ref._photo_like(48, 40, 21)
    out["photo_64x48"] = ref._photo_like(64, 48, 9)
    flat = np.full((32, 32, 4), 255, np.uint8)
    flat[..., :3] = (40, 90, 200)
    grad = np.full((32, 32, 4), 255, np.uint8)
    grad[..., 0] = np.arange(32)[None, :] * 8
    grad[..., 1] = np.arange(32)[:, None] * 8
    grad[..., 2] = 128
    out.update({"batch_flat": flat, "batch_noise": ref._noise(32, 32, 13), "batch_gradient": grad})
    return out


def _same_file(got, name, quality):
    _, _, want, crafted = _expected(name, quality)
    assert got == want, (name, quality, ref.first_difference(got, want, crafted))


# ------------------------------------------------------------------------------------------------ the two kernels on their own
@pytest.mark.gpu
def test_huffman_tables_are_the_helpers(ctx):
    hists = ref.all_histograms()
    std_tabs = ref.standard_tables()
    pad = (-len(hists)) % 4
    todo = hists + hists[:pad]
    for k in range(0, len(todo), 4):                     # four independent tables a call
        group = todo[k:k + 4]
        got = ctx.jpeg_huffman_tables(np.array([h for _, _, h in group], dtype=np.uint32))
        assert ctx.last_kernel(PROF_JPEG) == "jpeg_hufftab_kernel"
        for t, (name, _, h) in enumerate(group):
            try:
                bits, vals = ref.build_table(h)
                std = False
            except ref.TooLong:
                bits, vals = std_tabs[t]                 # the standard table of the slot the histogram was handed in
                std = True
            g = got[t]
            assert g["standard"] == std, name
            assert (g["bits"], g["vals"]) == (list(bits), list(vals)), name
            assert g["lut"].tolist() == ref.lut_words(bits, vals), name
    assert any(n == "geometric_33" for n, _, _ in hists)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_images()))
def test_symbol_histogram_is_the_helpers(ctx, name):
    img, qualities = _images()[name]
    for q in qualities:
        want = ref.symbol_histogram(_expected(name, q)[1])
        got = ctx.jpeg_symbol_histogram(img, q).astype(np.int64)
        assert ctx.last_kernel(PROF_JPEG) == "jpeg_symhist_kernel"
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, q, [(f"table {t}", f"symbol {s:#04x}", int(got[t, s]), int(want[t, s])) for t, s in bad[:8]])


def test_the_noise_image_spans_workgroups_of_the_histogram_kernel():
    img = _images()["noise_128x96"][0]
    assert (img.shape[1] // 16) * (img.shape[0] // 16) * 6 == 288 > 256


# ------------------------------------------------------------------------------------------------------------------ files
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_images()))
def test_files_are_the_helpers_byte_for_byte(opt, name):
    img, qualities = _images()[name]
    for q in qualities:
        data = opt.jpeg_encode(img, q)
        _same_file(data, name, q)
        assert np.array_equal(opt.jpeg_decode(data), opt.jpeg_roundtrip(img, q)), (name, q)
    opt.set_jpeg_huffman("standard")
    for q in qualities:
        assert opt.jpeg_encode(img, q) == _expected(name, q)[0], (name, q)


@pytest.mark.gpu
def test_both_size_routes_return_the_files_length(opt):
    img = _all_images()["sizes_48x40"]
    for q in (1, 10, 25, 50, 75, 90, 100):
        n = len(_expected("sizes_48x40", q)[2])
        assert len(opt.jpeg_encode(img, q)) == n
        for form, kernel in (("1", ONE_WAIT), ("0", TWO_STEP)):
            with opt.forms(jpeg_size=form):
                assert opt.jpeg_encoded_size(img, q) == n, (q, form)
                assert opt.last_kernel(PROF_JPEG) == kernel, (q, form)


# --------------------------------------------------------------------------------------------------------------- searches
@pytest.mark.gpu
def test_size_search_follows_the_optimised_sizes(ctx):
    name = "photo_64x48"
    img = _all_images()[name]
    h, w = img.shape[:2]
    for tq in (30, 75):
        target = len(_expected(name, tq)[0])                             # the standard file's size at that quality
        ctx.set_jpeg_huffman("standard")
        std = ctx.jpeg_size_search(img, target, skip_ssim=True)
        ctx.set_jpeg_huffman("optimized")
        try:
            got = ctx.jpeg_size_search(img, target, skip_ssim=True)
        finally:
            ctx.set_jpeg_huffman("standard")
        q, sz, steps = ref.size_bisect(lambda quality: len(_expected(name, quality)[2]), w, h, target)
        assert got is not None and std is not None
        assert (got[1], len(got[0]), got[3]) == (q, sz, steps), tq
        _same_file(got[0], name, q)
        assert got[1] >= std[1], (tq, got[1], std[1])


@pytest.mark.gpu
def test_compress_keeps_quality_and_ssim(ctx):
    name = "photo_64x48"
    img = _all_images()[name]
    ctx.set_jpeg_huffman("standard")
    s_data, s_q, s_ssim, s_steps = ctx.jpeg_compress(img, 0.95)
    ctx.set_jpeg_huffman("optimized")
    try:
        data, q, ssim, steps = ctx.jpeg_compress(img, 0.95)
    finally:
        ctx.set_jpeg_huffman("standard")
    assert (q, ssim, steps) == (s_q, s_ssim, s_steps)
    assert s_data == _expected(name, q)[0]
    _same_file(data, name, q)


@pytest.mark.gpu
def test_encode_scaled_is_the_file_of_the_box_image(opt):
    img = _all_images()["photo_64x48"]
    small = np.ascontiguousarray(orc.box_downsample(img, 23, 17))
    std, coef = orc.jpeg_encode(small, 75, with_coefficients=True)
    want, crafted, _ = ref.optimized_file(std, coef, 23, 17)
    got = opt.jpeg_encode_scaled(img, 23, 17, 75)
    assert got == want, ref.first_difference(got, want, crafted)
    assert opt.jpeg_encode_scaled(img, 23, 17, 75, size_only=True) == len(want)


# ------------------------------------------------------------------------------------------------------------------ batch
@pytest.mark.gpu
def test_batches_are_the_single_calls_files(opt):
    import torch
    names = ("batch_flat", "batch_noise", "batch_gradient")
    host = [_all_images()[n] for n in names]
    single = [opt.jpeg_compress(img, 0.95) for img in host]
    tabs = [ref.dht_tables(s[0]) for s in single]
    assert tabs[0] != tabs[1] != tabs[2] != tabs[0]                       # three different sets of tables
    for n, s in zip(names, single):
        _same_file(s[0], n, s[1])
    dev = [torch.from_numpy(img).cuda() for img in host]
    torch.cuda.synchronize()
    got = opt.jpeg_compress_batch(dev, 0.95)
    for k, (g, s) in enumerate(zip(got, single)):
        assert tuple(g) == tuple(s), names[k]
    opt.set_jpeg_huffman("standard")
    files = [opt.jpeg_encode(img, 90) for img in host]                    # the three standard files as sources
    opt.set_jpeg_huffman("optimized")
    one = [opt.jpeg_recompress(f, 0.95) for f in files]
    many = opt.jpeg_recompress_batch(files, 0.95)
    for k, (g, s) in enumerate(zip(many, one)):
        assert not isinstance(g, Exception), g
        assert tuple(g) == tuple(s), names[k]
        assert ref.dht_tables(g[0]) != ref.standard_tables()
