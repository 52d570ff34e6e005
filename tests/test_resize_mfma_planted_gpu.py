"""resize_mfma_kernel's rounding guard on planted samples (csrc/resize_mfma.hip; the model: tests/resize_mfma_model.py).

tests/test_resize_mfma_gpu.py meets the kernel's fp64 fix-up only where noise happens to flag a sample, and cannot tell
whether a tile was handed back to resize_fused_sparse_kernel, which repairs whatever the matrix kernel got wrong.  Here
windows that the guard flags AND whose fixed-point byte is not the reference's -- only the fix-up gives the right byte -- are
found on the host and planted at chosen places of opaque noise: an H sample (x, y) by writing the window into source row y
at x's taps, a V sample (x, dy) by making the source rows of dy's taps flat at the window's values across x's H window (a flat
run resamples to itself, so the intermediate column is the window).  Before every GPU call the model counts the flagged lanes
of every set of the kernel (chance flags of the noise included): at least one where a sample was planted, at most 16
anywhere, so no workgroup may give up -- and fnx_ctx_resize_mfma_report must say so (gave_up == 0), or the equality with the
oracle would prove nothing about the path.  One lane more in a set (17) and the workgroup must give up."""
import numpy as np
import pytest

import fennec_amd
from fennec_amd import synth
import resize_mfma_model as M

pytestmark = pytest.mark.gpu

ROUTE = "resize_mfma_kernel"


def _noise(w, h, seed):
    img = synth.noise_image(w, h, seed, alpha=True)
    img[..., 3] = 255
    return img


class Planted:
    """an opaque image with planted samples, the plans of its two tables, and what the model makes of it"""

    def __init__(self, w, h, dw, dh, seed, tables=None):
        self.w, self.h, self.dw, self.dh = w, h, dw, dh
        self.ph = M.lanczos_plan(dw, w) if tables is None else M.plan(tables[0], w)
        self.pv = M.lanczos_plan(dh, h) if tables is None else M.plan(tables[1], h)
        assert self.ph is not None and self.pv is not None
        self.img = _noise(w, h, seed)
        self.rng = np.random.default_rng(seed)
        self.hs, self.vs = [], []                      # planted (x, y, plane) / (x, dy, plane)
        self._model = None

    def cols(self, x):
        return slice(int(self.ph.first[x]), int(self.ph.first[x] + self.ph.count[x]))

    def rows(self, dy):
        return slice(int(self.pv.first[dy]), int(self.pv.first[dy] + self.pv.count[dy]))

    def plant_h(self, x, y, c, wrong=True):
        self.img[y, self.cols(x), c] = M.find_window(self.ph, x, self.rng, wrong)
        self.hs.append((x, y, c, wrong))
        self._model = None

    def plant_v(self, x, dy, c, wrong=True, x_end=None):
        """flat rows across the H windows of outputs x .. x_end"""
        win = M.find_window(self.pv, dy, self.rng, wrong)
        span = slice(self.cols(x).start, self.cols(x if x_end is None else x_end).stop)
        self.img[self.rows(dy), span, c] = win[:, None]
        self.vs.append((x, dy, c, wrong))
        self._model = None

    @property
    def model(self):
        if self._model is None:
            self._model = M.run_image(self.ph, self.pv, self.img)
        return self._model

    def h_set(self, x, y, c):
        return int(self.model.sets_h[x // 16, y // 16 - self.model.slot0, c])

    def v_set(self, x, dy, c):
        return int(self.model.sets_v[dy // 16, x // 16, c])

    def check_model(self, dense_ok=False):
        """every planted sample is flagged in the model's maps (and its unfixed byte wrong, where asked); its set counts it;
        no set holds more than 16 flagged lanes"""
        m = self.model
        for x, y, c, wrong in self.hs:
            assert m.flag_h[y, x, c] and (m.wrong_h[y, x, c] or not wrong), ("H", x, y, c)
            assert self.h_set(x, y, c) >= 1
        for x, dy, c, wrong in self.vs:
            assert m.flag_v[dy, x, c] and (m.wrong_v[dy, x, c] or not wrong), ("V", x, dy, c)
            assert self.v_set(x, dy, c) >= 1
        if not dense_ok:
            assert m.sets_h.max() <= M.DENSE and m.sets_v.max() <= M.DENSE, (m.sets_h.max(), m.sets_v.max())


def _run(ctx, orc, case, gave_up=0, tables=None):
    """the GPU call: the image is the oracle's byte for byte (and the model's), the route is the matrix kernel's, and the
    report says how many workgroups gave up"""
    if tables is None:
        got = ctx.lanczosResize(case.img, case.dw, case.dh)
        want = orc.lanczos_resize(case.img, case.dw, case.dh, procs=8)
    else:
        got = ctx.lanczos_resize_tables(case.img, case.dw, case.dh, *tables)
        want = orc.resize_v(orc.resize_h(case.img, case.dw, tables[0], procs=8), case.dh, tables[1], procs=8)
    ctx.sync()
    assert np.array_equal(case.model.out, want), "the model itself"
    back, wgs = ctx.resize_mfma_report()
    assert ctx.last_kernel(fennec_amd.PROF_RESIZE).startswith(ROUTE)
    assert wgs > 0
    assert back == gave_up if isinstance(gave_up, int) else gave_up(back), (back, wgs)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:4])
    return back, wgs


@pytest.fixture()
def mctx():
    c = fennec_amd.Context(0)
    c.set_form("resize_mfma", 2)
    return c


# -- 2:1 --------------------------------------------------------------------------------------------------------------------
def build_2to1(w, h, seed=11):
    """640 x 480 or 641 x 479 -> 320 x 240: strip 0 and the last strip (whose staged row starts before its first window when
    the row ends early), each wave's 16 columns, each 4-row group, the first and the last V group, clamped edge outputs,
    each plane alone and all three of one pixel, the bottom row (repeated in the last slot when srcH is no multiple of 16)"""
    k = Planted(w, h, 320, 240, seed)
    last_slot = (h - 1) // 16
    for wave in range(4):                                        # H: strip 0 in slot 3, the last strip in the last slot
        k.plant_h(16 * wave + 5, 16 * 3 + 4 * wave + 1, wave % 3)
        k.plant_h(256 + 16 * wave + 9, 16 * last_slot + 4 * (3 - wave) + 2, (wave + 1) % 3)
    for x, y, c in ((0, 100, 0), (1, 102, 2), (319, 101, 1), (318, 104, 0)):      # clamped tap lists
        k.plant_h(x, y, c)
    for c in range(3):                                           # one pixel, three planes, three windows
        k.plant_h(150, 200, c)
    for x in (10, 80, 200, 300):                                 # the bottom row: at most 4 outputs
        k.plant_h(x, h - 1, 1)
    for x, dy, c in ((40, 0, 0), (120, 7, 1), (200, 15, 2), (40, 230, 2), (120, 239, 0), (280, 224, 1),     # first / last V group
                     (0, 60, 1), (319, 64, 2), (77, 100, 0), (163, 141, 1), (251, 170, 2)):
        k.plant_v(x, dy, c)
    for c in range(3):
        k.plant_v(100, 120, c)
    return k


@pytest.mark.parametrize("w,h", [(640, 480), (641, 479)])
def test_two_to_one(mctx, orc, w, h):
    k = build_2to1(w, h)
    k.check_model()
    _run(mctx, orc, k)


def test_two_to_one_on_the_default_ctx(orc):
    """the product's own route (mode 1: downscales)"""
    k = build_2to1(640, 480)
    k.check_model()
    _run(fennec_amd.Context(0), orc, k)


# -- a generic downscale, an upscale (S = 22) ---------------------------------------------------------------------------------
def build_generic(kind, w=1000, h=700, dw=460, dh=322, seed=23):
    k = Planted(w, h, dw, dh, seed)
    sx, sy = dw / 460.0, dh / 322.0
    if kind in ("h", "both"):
        for i, (x, y) in enumerate(((3, 5), (70, 130), (200, 333), (333, 470), (459, 650), (130, 699), (401, 17), (258, 555))):
            k.plant_h(min(int(x * sx), dw - 1), min(int(y * h / 700.0), h - 1), i % 3)
    if kind in ("v", "both"):
        for i, (x, dy) in enumerate(((30, 2), (100, 40), (171, 90), (290, 160), (370, 230), (440, 300), (220, 321), (459, 120))):
            k.plant_v(min(int(x * sx), dw - 1), min(int(dy * sy), dh - 1), (i + 1) % 3)
    return k


@pytest.mark.parametrize("kind", ["h", "v", "both"])
def test_generic_downscale(mctx, orc, kind):
    k = build_generic(kind)
    k.check_model()
    _run(mctx, orc, k)


def test_upscale_table_of_s22(mctx, orc):
    k = build_generic("both", 640, 480, 1280, 960, seed=29)
    assert k.ph.S == 22 and k.pv.S == 22
    k.check_model()
    _run(mctx, orc, k)


# -- exact ties inside the kernel ---------------------------------------------------------------------------------------------
def build_stripes(seed=31):
    """two-level stripes (a, a + 1) at 2:1 put every output whose window they fill on an exact tie.  A patch of them, small
    enough for its sets: vertical stripes for H ties, horizontal ones for V ties; (a, parity) from the model, such that the
    unfixed byte is wrong"""
    k = Planted(640, 480, 320, 240, seed)

    def pick(p, d):
        for a in range(40, 250):
            for par in (0, 1):
                win = np.zeros(16, np.int64)
                n = int(p.count[d])
                win[:n] = a + ((int(p.first[d]) + np.arange(n) + par) & 1)
                fl, raw, ref, _ = M.kernel_bytes(p, d, win)
                if fl and raw != ref:
                    return a, par
        raise AssertionError("no stripe pair with a wrong unfixed byte")

    # H: outputs 100 .. 103, rows 160 .. 167 (8 lanes of one set), plane 1
    a, par = pick(k.ph, 101)
    span = np.arange(k.cols(100).start, k.cols(103).stop)
    k.img[160:168, span, 1] = (a + ((span + par) & 1))[None, :]
    k.hs += [(x, y, 1, x == 101) for x in (100, 101, 102, 103) for y in (160, 167)]
    # V: outputs 200 .. 203 (one 4-px group), output rows 40 .. 47, plane 2
    a, par = pick(k.pv, 44)
    rows = np.arange(k.rows(40).start, k.rows(47).stop)
    k.img[rows[:, None], np.arange(k.cols(200).start, k.cols(203).stop)[None, :], 2] = (a + ((rows + par) & 1))[:, None]
    k.vs += [(x, dy, 2, dy == 44) for x in (200, 203) for dy in (40, 44, 47)]
    return k


def test_stripe_patch(mctx, orc):
    k = build_stripes()
    k.check_model()
    assert k.h_set(100, 160, 1) >= 8 and k.v_set(200, 40, 2) >= 8
    _run(mctx, orc, k)


# -- the density limit --------------------------------------------------------------------------------------------------------
H_SET = (7, 9, 1)          # H group (outputs 112 .. 127), slot (rows 144 .. 159), plane
V_SET = (5, 6, 2)          # V group (output rows 80 .. 95), outputs 96 .. 111, plane


def build_dense_h(extra, seed=37):
    """16 flagged lanes in one H set: 16 rows, output xb + (row % 4) -- and with `extra` a 17th, eight outputs further in row 0"""
    k = Planted(640, 480, 320, 240, seed)
    hg, slot, c = H_SET
    for j in range(16):
        k.plant_h(16 * hg + 2 + (j % 4), 16 * slot + j, c)
    if extra:
        k.plant_h(16 * hg + 10, 16 * slot, c)
    return k


def build_dense_v(extra, seed=41, dims=(640, 480, 320, 240), where=V_SET, offs=(3, 4, 5, 6, 7), narrow_to=3):
    """16 flagged lanes in one V set: a column profile, flat across the 16 outputs' H windows, that flags four output rows
    of the group (offs[:4]; each row's four 4-px lanes) -- and with `extra` a fifth row (offs[4]) over outputs x0 .. x0 + narrow_to only,
    which lie in the first 4-px group: the 17th.  Each row of `offs` must bring two source rows the rows before it do not read: the profile is searched
    in those."""
    k = Planted(*dims, seed)
    vg, xg, c = where
    dys, x0 = [16 * vg + o for o in offs], 16 * xg
    prof = None
    while prof is None:
        prof = {}
        for dy in dys:
            prof = M.extend_profile(k.pv, prof, dy, k.rng)
            if prof is None:
                break
    wide = slice(k.cols(x0).start, k.cols(x0 + 15).stop)
    narrow = slice(k.cols(x0).start, k.cols(x0 + narrow_to).stop)
    for s, v in prof.items():
        if s < k.rows(dys[3]).stop:
            k.img[s, wide, c] = v
        elif extra:
            k.img[s, narrow, c] = v
    k.vs += [(x, dy, c, False) for dy in dys[:4] for x in (x0, x0 + 7, x0 + 15)]
    if extra:
        k.vs += [(x, dys[4], c, False) for x in (x0, x0 + narrow_to)]
    return k


@pytest.mark.parametrize("build,where", [(build_dense_h, H_SET), (build_dense_v, V_SET)])
def test_density_limit(mctx, orc, build, where):
    """exactly 16 flagged lanes in a set: the kernel fixes them all itself; 17: the workgroup gives up and
    resize_fused_sparse_kernel redoes its tiles.  Both exact.  (At 2:1 a V group's last slot is its own -- need = 2 j + 2 --, so
    every V set here runs from the `if (vready())` behind the H set; test_density_limit_inside_the_v_loop has the other place.)"""
    for extra, lanes in ((False, 16), (True, 17)):
        k = build(extra)
        k.check_model(dense_ok=True)
        m = k.model
        sets = m.sets_h if build is build_dense_h else m.sets_v
        if build is build_dense_h:
            assert sets[where[0], where[1] - m.slot0, where[2]] == lanes
        else:
            assert sets[where] == lanes
        assert (sets > M.DENSE).sum() == (1 if extra else 0)
        other = m.sets_v if build is build_dense_h else m.sets_h
        assert other.max() <= M.DENSE
        _run(mctx, orc, k, gave_up=(lambda n: n >= 1) if extra else 0)


def test_density_limit_inside_the_v_loop(mctx, orc):
    """The V pair again where a slot completes TWO V groups: the 2x upscale 640 x 480 -> 1280 x 960 (need = (8 j + 10) >> 4: an
    even group shares its last slot with the group before it).  The first of the two runs from `if (vready())`, the second
    inside `while (vready())`, behind that loop's own barrier and post() -- provided both belong to one workgroup, i.e. the
    even group does not start a run of segj groups.  segj is the launch's choice; the report gives it away (workgroups = 20
    strips x ceil(60 / segj) per image), so a batch of plain noise is launched first and the group chosen from its answer.  A
    batch of three, because a single 1280 x 960 call takes segj = 2 on 256 CUs and then every even group starts its run.
    16 lanes: fixed inside the loop's vset; 17: s_bad[(it + 1) & 1] raised there, and exactly one workgroup of the batch
    gives up."""
    import torch
    dims = (640, 480, 1280, 960)
    pv = M.lanczos_plan(960, 480)
    nvg, strips = 60, 20
    need = [int((pv.first[16 * g:16 * g + 16] + pv.count[16 * g:16 * g + 16] - 1).max()) >> 4 for g in range(nvg)]
    plain = [Planted(*dims, seed) for seed in (61, 67, 71)]
    for k in plain:
        k.check_model()
    probe = mctx.lanczosResizeBatch([torch.from_numpy(k.img).cuda() for k in plain], 1280, 960)
    mctx.sync()
    back, wgs = mctx.resize_mfma_report()
    assert mctx.last_kernel(fennec_amd.PROF_RESIZE).startswith(ROUTE) and back == 0 and wgs % 3 == 0, (back, wgs)
    for o, k in zip(probe, plain):
        assert np.array_equal(o.cpu().numpy(), k.model.out)
    segj = [q for q in range(1, 9) if strips * -(-nvg // q) == wgs // 3]
    assert len(segj) == 1, wgs
    groups = [j for j in range(2, nvg - 1, 2) if need[j] == need[j - 1] and j % segj[0]]
    assert groups, f"with {segj[0]} groups per workgroup no even group runs inside the loop"
    j = groups[len(groups) // 2]
    where = (j, 37, 1)
    # (the 17th over outputs x0 .. x0 + 2: x0 + 3 and x0 + 4 share a window, and x0 + 4 is the next lane's)
    cases = [build_dense_v(extra, 73, dims, where, (0, 3, 7, 11, 15), 2) for extra in (False, True)]
    for k, lanes in zip(cases, (16, 17)):
        k.check_model(dense_ok=True)
        assert k.model.sets_v[where] == lanes and (k.model.sets_v > M.DENSE).sum() == lanes - 16
        assert k.model.sets_h.max() <= M.DENSE
        assert np.array_equal(k.model.out, orc.lanczos_resize(k.img, 1280, 960, procs=8)), "the model itself"
    cases.append(plain[0])
    outs = mctx.lanczosResizeBatch([torch.from_numpy(k.img).cuda() for k in cases], 1280, 960)
    mctx.sync()
    back2, wgs2 = mctx.resize_mfma_report()
    assert mctx.last_kernel(fennec_amd.PROF_RESIZE).startswith(ROUTE)
    assert (back2, wgs2) == (1, wgs), (back2, wgs2, wgs)
    for o, k in zip(outs, cases):
        bad = np.argwhere(o.cpu().numpy() != k.model.out)
        assert len(bad) == 0, (len(bad), bad[:4])


def test_report_refuses_null_outputs_of_a_live_ctx(mctx):
    import ctypes as C
    lib, n = fennec_amd.load_library(), C.c_uint(7)
    assert lib.fnx_ctx_resize_mfma_report(mctx._h, None, C.byref(n)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_ctx_resize_mfma_report(mctx._h, C.byref(n), None) == fennec_amd.FNX_ERR_INVALID
    assert n.value == 7 and mctx.resize_mfma_report() == (0, 0)


# -- a batch ------------------------------------------------------------------------------------------------------------------
def test_batch_counts_only_the_dense_image(mctx, orc):
    """three same-geometry images in one launch: sparse in a V set, 17 lanes in the same V set, plain noise.  Each equals its
    single call; one workgroup owns a V set, so the batch's gave_up is exactly the dense image's 1"""
    import torch
    vg, xg, c = V_SET
    sparse = Planted(640, 480, 320, 240, 43)
    sparse.plant_v(16 * xg + 5, 16 * vg + 6, c)
    sparse.plant_h(16 * xg + 9, 200, 0)
    plain = Planted(640, 480, 320, 240, 47)
    cases = [sparse, build_dense_v(True), plain]
    singles = []
    for k, back in zip(cases, (0, 1, 0)):
        k.check_model(dense_ok=back > 0)
        _run(mctx, orc, k, gave_up=back)
        singles.append(k.model.out)
    dev = [torch.from_numpy(k.img).cuda() for k in cases]
    outs = mctx.lanczosResizeBatch(dev, 320, 240)
    mctx.sync()
    back, wgs = mctx.resize_mfma_report()
    assert mctx.last_kernel(fennec_amd.PROF_RESIZE).startswith(ROUTE)
    assert back == 1 and wgs > 0 and wgs % 3 == 0, (back, wgs)
    for o, want in zip(outs, singles):
        assert np.array_equal(o.cpu().numpy(), want)


# -- caller tables ------------------------------------------------------------------------------------------------------------
def _checker(w, h):
    """0/255 checkerboards of three block sizes per plane, single-px lines and hard edges, a band of noise at the bottom"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 4), 255, np.uint8)
    for c, b in enumerate((1, 2, 5)):
        img[..., c] = 255 * (((x // b) + (y // b)) & 1)
    img[h // 3: h // 3 + 20, :, :3] = 255 * (x[h // 3: h // 3 + 20, :, None] > w // 2)
    img[:, w // 4, :3] = 255
    img[h // 5, :, :3] = 0
    img[-24:, :, :3] = _noise(w, 24, 53)[..., :3]
    return img


def test_caller_tables_with_heavy_lobes(mctx, orc):
    """the heaviest negative lobes the kernel accepts (sums from -63 to 318: the offset of 64 and the saturation at both
    ends) on 0/255 content, through fnx_lanczos_resize; and a table just past the limit, which must take another route"""
    w, h, dw, dh = 258, 194, 256, 192                           # (equal dims would be lanczosResize's flat copy)
    tables = (M.lobe_table(dw, M.LOBE_X), M.lobe_table(dh, M.LOBE_X))
    k = Planted(w, h, dw, dh, 59, tables)
    k.img = _checker(w, h)
    k.check_model()
    assert (k.model.out[..., :3] == 0).any() and (k.model.out[..., :3] == 255).any()
    _run(mctx, orc, k, tables=tables)
    past = (63.0 + 1e-6) / 255.0
    refused = (M.lobe_table(dw, past), M.lobe_table(dh, past))
    assert fennec_amd.resize_fixed_point(refused[0], w) is None
    ctx = fennec_amd.Context(0)
    ctx.set_form("resize_mfma", 2)
    got = ctx.lanczos_resize_tables(k.img, dw, dh, *refused)
    ctx.sync()
    assert ctx.resize_mfma_report() == (0, 0)
    assert not ctx.last_kernel(fennec_amd.PROF_RESIZE).startswith(ROUTE)
    assert np.array_equal(got, orc.resize_v(orc.resize_h(k.img, dw, refused[0], procs=8), dh, refused[1], procs=8))
