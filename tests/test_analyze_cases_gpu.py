"""GPU tests (-m gpu) of Analyze on the crafted cases of tests/analyze_cases.py, on BOTH routes of analyze.hip: the one-launch
route (analyze_one_kernel + analyze_tail_kernel, the default) and the staged route (analyze_pass_kernel and the four launches
after it -- what a batch of more than 4096 images takes), selected with fnx_ctx_set_form(ctx, "analyze_staged", "1") and
asserted from fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) for every call.

Every result is held to the oracle with the suite's usual bars (_check_analysis) AND to the value the case planted, which
tests/analyze_cases.py states from the definitions alone (tests/test_analyze_cases.py shows on the CPU what each case reaches
and that the reference meets it).  Host arrays, device views on the scalar path (base 4-byte aligned, stride no multiple of 16)
and on the vector path with row tails, batches of 3 and 5 with one tensor twice; every w x h of 1..9 x 1..5 at every byte
offset inside a poisoned buffer; the colour tables' hand-over under inputs that load the table; the suite's Analyze images on
the staged route."""
from fractions import Fraction

import numpy as np
import pytest

import analyze_cases as ac
import fennec_amd
from analyze_cases import _check_analysis
from test_gpu_parity import ANALYZE_IMAGES

pytestmark = pytest.mark.gpu

ROUTES = {None: "analyze_one_kernel", "1": "analyze_pass_kernel"}       # analyze_staged -> the route's first kernel
STAGED = pytest.mark.parametrize("staged", list(ROUTES), ids=lambda s: "staged" if s else "one_launch")


@pytest.fixture(scope="module")
def _module_ctx():
    return fennec_amd.Context(0)


@pytest.fixture()
def ctx(_module_ctx):
    yield _module_ctx
    _module_ctx.set_form("analyze_staged", None)


_WANT = {}


def want_of(orc, case):
    """the oracle's analysis of a case, computed once and left alone"""
    if case.name not in _WANT:
        _WANT[case.name] = orc.analyze(case.img)
    return _WANT[case.name]


def check_planted(raw, case, what):
    for key, want in case.expect.items():
        if key == "histogram":
            assert np.array_equal(raw[key], want), (what, key, np.nonzero(raw[key] != want)[0][:8].tolist())
        else:
            assert raw[key] == want, (what, key, raw[key], want)
    if case.kind == "contrast_grid":
        var = case.info["variance"]                              # exact; the fp64 chains are ten orders closer than the suite's 1e-9
        assert abs(Fraction(raw["variance_sum"]) - var) <= Fraction(1, 10 ** 9) * var, what


def check_call(ctx, orc, case, x, staged, what):
    ctx.set_form("analyze_staged", staged)
    raw = ctx.analyze_raw(x)
    took = ctx.last_kernel(fennec_amd.PROF_MAIN)
    st = ctx.Analyze(x)
    assert took == ROUTES[staged] == ctx.last_kernel(fennec_amd.PROF_MAIN), (what, took)
    check_planted(raw, case, what)
    _check_analysis(raw, st, want_of(orc, case))


# ------------------------------------------------------------------ every case, both routes
@STAGED
@pytest.mark.parametrize("case", ac.CASES, ids=repr)
def test_cases(ctx, orc, case, staged):
    check_call(ctx, orc, case, case.img, staged, f"{case.name}, host")


# ------------------------------------------------------------------ presentations
def poison(h, w, seed=5):
    """pixels that would change every statistic: coloured, translucent, thousands of distinct ones, black and white among them"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    p[..., 3] = rng.integers(0, 255, (h, w), dtype=np.uint8)
    p[::2, ::3, :3] = 255
    p[1::2, 1::3, :3] = 0
    return p


def device_views(img):
    """(name, view): the scalar path -- the base 4-byte aligned only, the stride no multiple of 16 -- and the vector path with
    row tails -- base and stride multiples of 16, w % 4 in {1, 2, 3}"""
    import torch
    h, w = img.shape[:2]
    assert w % 4
    pw = w + 2 + (1 if (w + 2) % 4 == 0 else 0)
    parent = poison(h + 1, pw)
    parent[:h, 1:1 + w] = img
    v4 = torch.from_numpy(parent).cuda()[:h, 1:1 + w]
    assert v4.data_ptr() % 16 == 4 and v4.stride(0) % 16 != 0 and v4.stride(0) != 4 * w
    yield "view4", v4
    pw = 4 + w + (-w) % 4 + 4
    parent = poison(h + 1, pw)
    parent[:h, 4:4 + w] = img
    v16 = torch.from_numpy(parent).cuda()[:h, 4:4 + w]
    assert v16.data_ptr() % 16 == 0 and v16.stride(0) % 16 == 0 and v16.stride(0) != 4 * w
    yield "view16", v16


@STAGED
@pytest.mark.parametrize("name", ac.PRESENTED)
def test_presentations(ctx, orc, name, staged):
    import torch
    case = ac.BY_NAME[name]
    check_call(ctx, orc, case, case.img, staged, f"{name}, host")
    tight = torch.from_numpy(case.img.copy()).cuda()
    check_call(ctx, orc, case, tight, staged, f"{name}, device")
    for vname, view in device_views(case.img):
        check_call(ctx, orc, case, view, staged, f"{name}, {vname}")


@STAGED
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("group", list(ac.BATCHES))
def test_batches(ctx, orc, group, n, staged):
    """plan_analyze_batch: the workgroups per image change with n; one tensor is in the batch twice"""
    import torch
    names = ac.batch_names(group, n)
    dev = {nm: torch.from_numpy(ac.BY_NAME[nm].img.copy()).cuda() for nm in set(names)}
    torch.cuda.synchronize()
    ctx.set_form("analyze_staged", staged)
    plan = ctx.plan_analyze_batch([dev[nm] for nm in names])
    for rep in (1, 2):
        raw = plan.run()
        assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[staged]
        stats = plan.stats()
        for k, nm in enumerate(names):
            case = ac.BY_NAME[nm]
            r = ctx._analysis_dict(raw[k])
            check_planted(r, case, f"batch {group} of {n}, image {k} ({nm}), call {rep}")
            _check_analysis(r, stats[k], want_of(orc, case))


# ------------------------------------------------------------------ the strided pass, every small shape at every offset
def _inner(w, h):
    """grey, opaque, a handful of values: any poisoned pixel that leaks in flips both flags and a histogram bin"""
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    v = ((7 * x + 13 * y + 5) % 6 * 30 + 20).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], axis=2)


@STAGED
@pytest.mark.parametrize("parent_w", [16, 13], ids=lambda p: f"stride{4 * p}")
def test_strided_pass_shapes(ctx, orc, parent_w, staged):
    """w in 1..9, h in 1..5 at byte offsets 0, 4, 8 and 12 of a wider device buffer (rows of 64 bytes: 16-byte loads with row
    tails at offset 0; rows of 52 bytes: the scalar path throughout) whose padding is poisoned"""
    import torch
    ctx.set_form("analyze_staged", staged)
    shapes = [(w, h) for h in range(1, 6) for w in range(1, 10)] + [(1, 300), (4, 257), (5, 131), (3, 1000)]   # ... and narrow, tall ones
    bases = {}
    for w, h in shapes:
        inner = _inner(w, h)
        want = orc.analyze(inner)
        assert want["has_alpha"] == 0 and want["is_grayscale"] == 1
        base = bases.setdefault(h, poison(h + 1, parent_w, 9))
        for off in range(4):
            parent = base.copy()
            parent[:h, off:off + w] = inner
            view = torch.from_numpy(parent).cuda()[:h, off:off + w]
            assert view.data_ptr() % 16 == 4 * off
            raw = ctx.analyze_raw(view)
            assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[staged]
            try:
                _check_analysis(raw, ctx.Analyze(view), want)
            except AssertionError as e:
                raise AssertionError(f"{w} x {h} at byte offset {4 * off}, row stride {4 * parent_w}: {e}") from e


# ------------------------------------------------------------------ the colour tables between calls
@STAGED
def test_colour_tables_hand_over_under_load(orc, staged):
    """the one-launch route keeps two colour tables per ctx and each launch clears the other; the staged route clears its
    table per call.  2100 colours in one probe chain through slot 0, then five of the SAME colours: a table that was not
    cleared answers 0 for the second image.  Five rounds on one ctx, single calls and a batch between them."""
    import torch
    big, few = ac.BY_NAME["colliding_2100"], ac.BY_NAME["colliding_5"]
    assert set(few.info) <= set(big.info) and len(few.info) == 5
    c = fennec_amd.Context(0)
    c.set_form("analyze_staged", staged)
    d = [torch.from_numpy(k.img.copy()).cuda() for k in (big, few, few)]
    torch.cuda.synchronize()
    plan = c.plan_analyze_batch(d)
    for rnd in range(5):
        for case in (big, few):
            raw = c.analyze_raw(case.img)
            assert c.last_kernel(fennec_amd.PROF_MAIN) == ROUTES[staged]
            check_planted(raw, case, f"round {rnd}, {case.name}")
            _check_analysis(raw, c.Analyze(case.img), want_of(orc, case))
        res = plan.run()
        for k, case in enumerate((big, few, few)):
            check_planted(c._analysis_dict(res[k]), case, f"round {rnd}, batch image {k}")
    c.close()


# ------------------------------------------------------------------ the suite's own images on the staged route
@pytest.mark.parametrize("name", list(ANALYZE_IMAGES))
def test_analyze_images_on_the_staged_route(ctx, orc, name):
    """late_noise_1000x800 was written for the staged route's second colour launch; here it meets it"""
    img = np.ascontiguousarray(ANALYZE_IMAGES[name]())
    ctx.set_form("analyze_staged", "1")
    raw = ctx.analyze_raw(img)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == "analyze_pass_kernel"
    _check_analysis(raw, ctx.Analyze(img), orc.analyze(img))
    ctx.set_form("analyze_staged", "0")                          # "0" is the default's route
    ctx.analyze_raw(img)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == "analyze_one_kernel"
