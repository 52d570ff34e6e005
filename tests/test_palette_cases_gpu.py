"""GPU tests (-m gpu) of applyPalette on the crafted cases of tests/palette_cases.py, on BOTH routes of palette.hip: the grid of
candidate lists (pal_grid_kernel + apply_palette_grid_kernel; what images of 256 k pixels and more take) and the walk over the
whole palette (apply_palette_kernel), selected with fnx_ctx_set_form(ctx, "palette_grid", "1" / "0") or left to the library,
and asserted from fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) for every call.

Every index plane and quantized image is compared byte for byte with the plane the case planted (tests/test_palette_cases.py
shows on the CPU what each case reaches), with the oracle and with palette[idx].  Host arrays; device tensors, views on a
4-byte-aligned base and with row tails inside a poisoned parent, indices alone; every w x h of 1..9 x 1..5 at every pixel
offset; the library's own choice on either side of 262144 pixels; and fnx_quantize, whose palette never leaves the device,
on images whose median cut is full of duplicated entries."""
import numpy as np
import pytest

import fennec_amd
import median_cut_ref
import palette_cases as pc

pytestmark = pytest.mark.gpu

GRID, WALK = "apply_palette_grid_kernel", "apply_palette_kernel"
ROUTES = {"1": GRID, "0": WALK, None: WALK}                    # palette_grid -> the kernel; None: every case here is below 256 k pixels
FORM = pytest.mark.parametrize("form", list(ROUTES), ids=lambda f: {"1": "grid", "0": "walk", None: "default"}[f])


@pytest.fixture(scope="module")
def _module_ctx():
    return fennec_amd.Context(0)


@pytest.fixture()
def ctx(_module_ctx):
    yield _module_ctx
    _module_ctx.set_form("palette_grid", None)


_ORACLE = {}


def oracle_of(orc, case):
    """the oracle's plane and image of a case, computed once and left alone"""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = orc.apply_palette(case.img, case.palette)
    return _ORACLE[case.name]


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def check_call(ctx, orc, case, x, form, what, want_quantized=True):
    ctx.set_form("palette_grid", form)
    idx, q = ctx.applyPalette(x, case.palette, want_quantized=want_quantized)
    ctx.sync()
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[form], (what, ctx.last_kernel(fennec_amd.PROF_MAIN))
    idx = _np(idx)
    wi, wq = oracle_of(orc, case)
    assert idx.shape == case.want.shape and idx.dtype == np.uint8
    assert np.array_equal(idx, case.want), (what, np.argwhere(idx != case.want)[:6].tolist(), idx[idx != case.want][:6].tolist(), case.want[idx != case.want][:6].tolist())
    assert np.array_equal(idx, wi), what
    if want_quantized:
        q = _np(q)
        assert np.array_equal(q, case.palette[case.want]) and np.array_equal(q, wq), what
    else:
        assert q is None


# ------------------------------------------------------------------ every case, every form
@FORM
@pytest.mark.parametrize("case", pc.CASES, ids=repr)
def test_cases(ctx, orc, case, form):
    check_call(ctx, orc, case, case.img, form, f"{case.name}, host")


# ------------------------------------------------------------------ presentations
def poison(h, w, palette, seed=5):
    """pixels that would change an index: the palette's own entries, each the nearest entry of itself"""
    rng = np.random.default_rng(seed)
    p = palette[rng.integers(0, len(palette), (h, w))].copy()
    p[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return p


def device_views(img, palette):
    """(name, view): a base that is 4-byte aligned only with a stride that is no multiple of 16, and a 16-byte-aligned base
    and stride with row tails"""
    import torch
    h, w = img.shape[:2]
    pw = w + 2 + (1 if (w + 2) % 4 == 0 else 0)
    parent = poison(h + 1, pw, palette)
    parent[:h, 1:1 + w] = img
    v4 = torch.from_numpy(parent).cuda()[:h, 1:1 + w]
    assert v4.data_ptr() % 16 == 4 and v4.stride(0) % 16 != 0 and v4.stride(0) != 4 * w
    yield "view4", v4
    pw = 4 + w + (-w) % 4 + 4
    parent = poison(h + 1, pw, palette)
    parent[:h, 4:4 + w] = img
    v16 = torch.from_numpy(parent).cuda()[:h, 4:4 + w]
    assert v16.data_ptr() % 16 == 0 and v16.stride(0) % 16 == 0 and v16.stride(0) != 4 * w
    yield "view16", v16


@FORM
@pytest.mark.parametrize("name", pc.PRESENTED)
def test_presentations(ctx, orc, name, form):
    """on the device the index tensor is tight: an odd width drives the word store and the byte store in one image"""
    import torch
    case = pc.BY_NAME[name]
    tight = torch.from_numpy(case.img.copy()).cuda()
    check_call(ctx, orc, case, tight, form, f"{name}, device")
    check_call(ctx, orc, case, tight, form, f"{name}, device, indices alone", want_quantized=False)
    check_call(ctx, orc, case, case.img, form, f"{name}, host, indices alone", want_quantized=False)
    for vname, view in device_views(case.img, case.palette):
        check_call(ctx, orc, case, view, form, f"{name}, {vname}")
        check_call(ctx, orc, case, view, form, f"{name}, {vname}, indices alone", want_quantized=False)


# ------------------------------------------------------------------ every small shape at every pixel offset
@FORM
def test_small_shapes(ctx, form):
    """w in 1..9, h in 1..5 at pixel offsets 0..3 of a wider device buffer whose padding is poisoned; the pixels are the
    neighbourhood of midpoint_tie's pixel across a cell border, under its eight tied entries"""
    import torch
    where, m = "at8", 8
    pal, pos = pc.midpoint_palette(m, where, 5, 29, 77)
    colours = np.array(pc.midpoint_neighbourhood(where), dtype=np.uint8)
    ctx.set_form("palette_grid", form)
    parent_w = 13
    for h in range(1, 6):
        base = poison(h + 1, parent_w, pal, 9)
        for w in range(1, 10):
            k = (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 11 + w) % len(colours)
            inner = np.concatenate([colours[k], np.full((h, w, 1), 255, np.uint8)], axis=2)
            inner[(k == 13)] = (8, 8, 8, 3)                                          # the tied pixel itself, translucent
            want = pc.nearest_first(pal, inner)
            assert (want[(k == 13)] == min(pos)).all()
            for off in range(4):
                buf = base.copy()
                buf[:h, off:off + w] = inner
                view = torch.from_numpy(buf).cuda()[:h, off:off + w]
                assert view.data_ptr() % 16 == 4 * off
                for want_q in (True, False):
                    idx, q = ctx.applyPalette(view, pal, want_quantized=want_q)
                    ctx.sync()
                    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[form]
                    what = f"{w} x {h} at pixel offset {off}, quantized {want_q}"
                    assert np.array_equal(_np(idx), want), what
                    assert q is None or np.array_equal(_np(q), pal[want]), what


# ------------------------------------------------------------------ the library's own choice
@pytest.mark.parametrize("shape,route", [((512, 512), GRID), ((511, 513), WALK)], ids=["512x512_grid", "511x513_walk"])
@pytest.mark.parametrize("kind", ["random", "clustered"])
def test_the_automatic_choice(ctx, orc, kind, shape, route):
    """exactly 262144 pixels take the grid, 262143 the walk; both tiled from every_cell"""
    import torch
    case = pc.BY_NAME[f"every_cell_{kind}"]
    w, h = shape
    img = np.ascontiguousarray(np.tile(case.img, (5, 2, 1))[:h, :w])
    assert img.shape == (h, w, 4) and (w * h >= 262144) == (route == GRID)
    wi, wq = orc.apply_palette(img, case.palette)
    assert np.array_equal(wi, np.tile(case.want, (5, 2))[:h, :w])
    for x in (img, torch.from_numpy(img).cuda()):
        idx, q = ctx.applyPalette(x, case.palette)
        ctx.sync()
        assert ctx.last_kernel(fennec_amd.PROF_MAIN) == route
        assert np.array_equal(_np(idx), wi) and np.array_equal(_np(q), wq)


# ------------------------------------------------------------------ the palette made on the device (fnx_quantize)
QUANTIZED = {"two_colours_64x64": 256, "flat_16x16": 256, "5x2_random": 256, "tie_free_16x16": 256}


@pytest.mark.parametrize("form", ["1", "0"], ids=["grid", "walk"])
@pytest.mark.parametrize("name", list(QUANTIZED))
def test_device_made_palette(ctx, name, form):
    """median cut of a few-colour image returns duplicated entries (boxes of identical samples keep splitting): crowded cells
    and lowest-index ties with the entry count read on the device (n_dev, pal_tables_kernel)"""
    import torch
    img = np.ascontiguousarray(median_cut_ref.CASES[name][0])
    max_colors = QUANTIZED[name]
    ctx.set_form("palette_grid", form)
    seen = []
    for space, src in (("host", img), ("device", torch.from_numpy(img).cuda())):
        pal, idx, q, s = ctx.quantize(src, max_colors, want_ssim=False)
        ctx.sync()
        assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[form] and s is None
        idx, q = _np(idx), _np(q)
        distinct = len({tuple(p) for p in pal.tolist()})
        print(name, space, "ncolors", len(pal), "distinct", distinct)
        want = pc.nearest_first(pal, img)                                            # the first minimum over the RETURNED palette
        assert np.array_equal(idx, want), (name, space, np.argwhere(idx != want)[:6].tolist())
        assert np.array_equal(q, pal[idx]) and (q[..., 3] == 255).all()
        p2, i2, q2, _ = ctx.quantize(src, max_colors, want_indices=False, want_ssim=False)       # the launch without an index plane
        ctx.sync()
        assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[form]
        assert i2 is None and np.array_equal(p2, pal) and np.array_equal(_np(q2), q)
        p3, i3, q3, _ = ctx.quantize(src, max_colors, want_quantized=False, want_ssim=False)
        ctx.sync()
        assert q3 is None and np.array_equal(p3, pal) and np.array_equal(_np(i3), idx)
        seen.append((pal, idx, q))
    assert all(np.array_equal(a, b) for a, b in zip(*seen))                          # the same bytes in both spaces
    pal = seen[0][0]
    if name == "two_colours_64x64":
        assert len(pal) == 256 and len({tuple(p) for p in pal.tolist()}) == 2
    if name == "flat_16x16":
        assert len({tuple(p) for p in pal.tolist()}) == 1 and (seen[0][1] == 0).all()
    if name == "5x2_random":
        assert len(pal) < 256
    if name == "tie_free_16x16":
        assert len(pal) == 256
