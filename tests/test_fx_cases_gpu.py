"""GPU tests (-m gpu) of Sharpen / AdaptiveSharpen on the crafted cases of tests/fx_cases.py: exact ties by the thousand, both
fix lists at their cap, one past it and far past it, the saturation decision on and around |Sobel| = 400, Sharpen amounts one
ulp from a tie -- in every kernel form, from host arrays, device tensors and strided device views, through the batch entry,
each call twice, and with the route the dispatch took asserted (fnx_ctx_last_kernel(ctx, FNX_PROF_FX)) for every call.

What each case reaches is proved on the CPU (tests/test_fx_cases.py).  Every device destination is filled with 0xA5 first
(the staging slot of a host call through a call on a flat 0xA5 image): a sample that no kernel wrote cannot pass for right.

Mutants of effects.hip with one wrong decision each (CHANGELOG.md has the table): the overflow branches recomputing the listed
entries only, the saturation bound lowered to 1.59e11f and build_rtab without its near-tie refusal each fail tests of this file."""
import numpy as np
import pytest

import fennec_amd
import fx_cases as fc
import np_restatement as npr

pytestmark = pytest.mark.gpu

POISON = 0xA5
# form -> (fx_stream, fx_pairs, the marching kernel it asks for)
FORMS = {"stream": ("1", "1", "fx_stream_kernel"), "tile_pairs": ("0", "1", "fx_march_kernel"), "tile_rows": ("0", "0", "fx_march_kernel")}
FLAT = " + fx_flat_kernel"


@pytest.fixture(scope="module")
def _module_ctx():
    return fennec_amd.Context(0)


@pytest.fixture()
def ctx(_module_ctx):
    yield _module_ctx
    for name in ("fx_stream", "fx_pairs", "fx_ref"):
        _module_ctx.set_form(name, None)


def set_form(ctx, form):
    stream, pairs, kernel = FORMS[form]
    ctx.set_form("fx_stream", stream)
    ctx.set_form("fx_pairs", pairs)
    return kernel


_WANT = {}


def want_adaptive(orc, case):
    """the oracle's image of a case, computed once and left alone"""
    if case.name not in _WANT:
        w = orc.adaptive_sharpen(np.ascontiguousarray(case.img), case.strength)
        w.setflags(write=False)
        _WANT[case.name] = w
    return _WANT[case.name]


def layouts(img):
    """(name, image, whole image compared): a host array, a tight device tensor, a strided device view with 16-byte-aligned rows
    and one with 4-byte alignment only (of a SubImage the interior is compared: its frame follows the reference's flat copy)"""
    import torch
    h, w = img.shape[:2]
    tight = np.ascontiguousarray(img)
    yield "host", tight, True
    yield "device", torch.from_numpy(tight.copy()).cuda(), True
    right = 4 + (-w) % 4                                        # parent rows a multiple of 16 bytes
    p16 = torch.from_numpy(np.pad(tight, ((0, 0), (4, right), (0, 0)), constant_values=7)).cuda()
    v16 = p16[:, 4:4 + w]
    assert v16.data_ptr() % 16 == 0 and v16.stride(0) % 16 == 0 and v16.stride(0) != 4 * w
    yield "view16", v16, False
    p4 = torch.from_numpy(np.pad(tight, ((0, 0), (3, 2), (0, 0)), constant_values=7)).cuda()
    v4 = p4[:, 3:3 + w]
    assert v4.data_ptr() % 16 == 12 and v4.stride(0) != 4 * w
    yield "view4", v4, False


def call(ctx, src, amount, adaptive):
    """fnx_sharpen / fnx_adaptive_sharpen into a destination that holds 0xA5 everywhere -> the image as a numpy array"""
    s = fennec_amd._Img(src)
    if s.space == fennec_amd.FNX_DEVICE:
        import torch
        dst = torch.full((s.h, s.w, 4), POISON, dtype=torch.uint8, device=src.device)
        torch.cuda.synchronize()
    else:
        ctx.sharpen_amount(np.full((s.h, s.w, 4), POISON, np.uint8), 1.0, False)      # a flat image sharpens to itself: the staging slot holds 0xA5
        dst = np.full((s.h, s.w, 4), POISON, np.uint8)
    d = fennec_amd._Img(dst)
    fn = ctx._lib.fnx_adaptive_sharpen if adaptive else ctx._lib.fnx_sharpen
    with ctx._ordered(src, dst):
        ctx._chk(fn(ctx._h, s.space, s.ptr, s.stride, s.w, s.h, float(amount), d.ptr, d.stride), "sharpen")
    ctx.sync()
    return dst if isinstance(dst, np.ndarray) else dst.cpu().numpy()


def first_difference(got, want, cl, whole, what):
    """None, or the message of the first differing byte: the case, form, pixel, channel, exact distance and saturation class"""
    g, w = (got, want) if whole else (got[1:-1, 1:-1], want[1:-1, 1:-1])
    if np.array_equal(g, w):
        return None
    y, x, ch = (int(v[0]) for v in np.nonzero(g != w))
    if not whole:
        y, x = y + 1, x + 1
    msg = f"{what}: got {int(got[y, x, ch])}, want {int(want[y, x, ch])} at "
    h, wd = want.shape[:2]
    if ch < 3 and 1 <= x < wd - 1 and 1 <= y < h - 1 and cl is not None:
        return msg + cl.describe(y, x, ch) + f"; {int((g != w).sum())} bytes differ"
    return msg + f"pixel ({x}, {y}) channel {ch} (frame or alpha); {int((g != w).sum())} bytes differ"


def check(ctx, src, amount, adaptive, want, cl, whole, route, what):
    for rep in (1, 2):                                           # each call twice on one ctx
        got = call(ctx, src, amount, adaptive)
        took = ctx.last_kernel(fennec_amd.PROF_FX)
        msg = first_difference(got, want, cl, whole, f"{what}, call {rep}, by {took}")
        assert msg is None, msg
        assert took == route, (what, rep, took)


# ------------------------------------------------------------------ AdaptiveSharpen: every case, every form, every layout
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_adaptive_cases(ctx, orc, case, form):
    kernel = set_form(ctx, form)
    want = want_adaptive(orc, case)
    amount = 1.0 + case.strength * 2.0                           # effects.go:63
    for lname, src, whole in layouts(case.img):
        route = kernel + ("" if whole else FLAT)
        check(ctx, src, amount, True, want, case.cl, whole, route, f"{case.name}, {form}, {lname}")
    # the public entry, strength in
    for rep in (1, 2):
        got = ctx.AdaptiveSharpen(np.ascontiguousarray(case.img), case.strength)
        assert ctx.last_kernel(fennec_amd.PROF_FX) == kernel
        msg = first_difference(got, want, case.cl, True, f"{case.name}, {form}, AdaptiveSharpen, call {rep}")
        assert msg is None, msg


@pytest.mark.parametrize("form", list(FORMS))
def test_adaptive_amounts_past_the_guard_take_the_fp64_kernel(ctx, form):
    """fx_guard() holds for amounts in (0, 8]: 8 marches, above it the reference-order kernel runs whatever form is selected"""
    kernel = set_form(ctx, form)
    for name in ("steps_2.5_rgb", "ramp10_amp2_rgb", "soft_64x48"):
        img = np.ascontiguousarray(fc.BY_NAME[name].img)
        for amount, route in ((8.0, kernel), (8.5, "fx_ref_kernel"), (40.0, "fx_ref_kernel")):
            want = npr.adaptive_sharpen_amount(img, amount)
            cl = fc.classify(img, int(2 * amount), 2)
            for lname, src, whole in layouts(img):
                check(ctx, src, amount, True, want, cl, whole, route + ("" if whole else FLAT), f"{name}, amount {amount}, {form}, {lname}")


# ------------------------------------------------------------------ Sharpen: exact ties by table, near-ties by the fp64 kernel
SHARPEN_IMAGES = ("ramp10_amp2_rgb", "steps_2.5_rgb", "soft_64x48", "half_left")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(fc.sharpen_amounts()))
def test_sharpen_amounts(ctx, name, form):
    from fractions import Fraction
    kernel = set_form(ctx, form)
    amount = fc.sharpen_amounts()[name]
    route = "fx_ref_kernel" if name in fc.NEAR_TIE else kernel
    for iname in SHARPEN_IMAGES:
        img = np.ascontiguousarray(fc.BY_NAME[iname].img)
        want = npr.sharpen_amount(img, amount)
        cl = fc.classify(img, Fraction(amount), adaptive=False)
        for lname, src, whole in layouts(img):
            check(ctx, src, amount, False, want, cl, whole, route + ("" if whole else FLAT), f"{iname}, Sharpen amount {name}, {form}, {lname}")


@pytest.mark.parametrize("target", ["1.5+ulp", "1.5-ulp", "2.5-ulp"])
def test_public_strength_next_to_a_tie_amount(ctx, orc, target):
    """Sharpen(img, s) with 1 + 1.5 s one ulp from 1.5 or 2.5: the table's rule is wrong on a third of these bytes, the library takes the fp64 kernel"""
    amount = fc.sharpen_amounts()[target]
    s = fc.strength_for_amount(amount)
    assert s is not None
    for iname in SHARPEN_IMAGES:
        img = np.ascontiguousarray(fc.BY_NAME[iname].img)
        want = orc.sharpen(img, s)
        for rep in (1, 2):
            got = ctx.Sharpen(img, s)
            assert ctx.last_kernel(fennec_amd.PROF_FX) == "fx_ref_kernel"
            msg = first_difference(got, want, None, True, f"{iname}, Sharpen strength {s!r}, call {rep}")
            assert msg is None, msg


# ------------------------------------------------------------------ batches
BATCHES = {
    (64, 24): ("flat", "ramp10_amp2_rgb", "soft", "steps_2.5_rgb", "flat"),
    (130, 50): ("flat", "cap_tile_inner_513", "soft", "pyth_rgb", "cap_segment_65", "flat", "cap_segment_64", "cap_tile_edge_512"),
    (200, 150): ("flat", "half_left", "soft", "steps_2.5_big", "half_bottom"),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("geom", list(BATCHES), ids=lambda g: f"{g[0]}x{g[1]}")
def test_batches(ctx, orc, geom, form):
    """sharpen_batch, adaptive both ways: an overflowing image between a flat and a soft one (a wave of the batch launch owns one
    image's strip and segment: its list must not leak into a neighbour's)"""
    import torch
    kernel = set_form(ctx, form)
    w, h = geom
    imgs = [fc.flat(w, h) if n == "flat" else fc.soft(w, h, 77) if n == "soft" else np.ascontiguousarray(fc.BY_NAME[n].img) for n in BATCHES[geom]]
    dev = [torch.from_numpy(i.copy()).cuda() for i in imgs]
    for adaptive in (True, False):
        want = [orc.adaptive_sharpen(i, 0.75) if adaptive else orc.sharpen(i, 0.75) for i in imgs]
        cls = [fc.classify(i, 5, 2) if adaptive else fc.classify(i, 17, 8, adaptive=False) for i in imgs]
        for rep in (1, 2):
            outs = [torch.full((h, w, 4), POISON, dtype=torch.uint8, device="cuda") for _ in imgs]
            torch.cuda.synchronize()
            ctx.sharpen_batch(dev, 0.75, adaptive=adaptive, outs=outs)
            ctx.sync()
            assert ctx.last_kernel(fennec_amd.PROF_FX) == kernel
            for k, name in enumerate(BATCHES[geom]):
                msg = first_difference(outs[k].cpu().numpy(), want[k], cls[k], True, f"batch image {k} ({name}), adaptive {adaptive}, {form}, call {rep}")
                assert msg is None, msg


def test_routes_of_the_other_entries(ctx):
    """gaussianBlur3x3 reports the same routes; the fp64 form on request"""
    img = np.ascontiguousarray(fc.BY_NAME["pyth_rgb"].img)
    ctx.blur3x3(img)
    assert ctx.last_kernel(fennec_amd.PROF_FX) == "fx_stream_kernel"
    ctx.set_form("fx_stream", "0")
    ctx.blur3x3(img)
    assert ctx.last_kernel(fennec_amd.PROF_FX) == "fx_march_kernel"
    ctx.set_form("fx_ref", "1")
    ctx.AdaptiveSharpen(img, 0.75)
    assert ctx.last_kernel(fennec_amd.PROF_FX) == "fx_ref_kernel"
