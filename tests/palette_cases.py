"""Crafted applyPalette cases (targetsize.go:488-546: nearest palette entry by squared RGB distance, the lowest index wins a
tie) and a host model of the candidate grid of fennec_amd/csrc/palette.hip.  Plain numpy; nothing here touches the GPU.

The grid route asks, per pixel, only the candidate list of the pixel's cell (32 x 32 x 32 cells of 8 x 8 x 8 colours): every
entry i with mind_i <= U, U = min_j maxd_j.  grid_lists() restates pg_chan and the two loops of pal_grid_kernel and says, per
cell, U, the candidate SET and the entries with mind == U -- nothing about the slot an entry lands in (atomicAdd order).

Each case plants a palette and an image so that one decision of that route is the only thing between the right index plane
and a wrong one, and states the index plane from the construction wherever the construction fixes it:

  list_len_k      one cell with exactly k candidates, each the strict unique nearest entry of some pixel of the image; every
                  row of the image is one wave (256 pixels) whose longest list is exactly k (the wave's `most > 3 / 7 / 15`,
                  the record's second 16 bytes, the 31-candidate cap and its 0xff mark)
  rim_tie         the one colour of a cell that is as far from the cell's best entry as it is close to an outside entry whose
                  mind equals U (the pruning rule's `<=`)
  midpoint_tie    2, 4 and 8 entries at the same distance from a pixel, inside a cell and across a cell border
  duplicates      one colour at two indices far apart; palettes of one and of two colours (what medianCut returns for such images)
  mixed_wave      one wave holding pixels of a marked cell, a 1-candidate cell and a 17-candidate cell; widths around 256
  every_cell      one colour of each of the 32768 cells
  alpha_ignored   arbitrary source alpha

tests/test_palette_cases.py shows on the CPU that the cases reach what they claim; tests/test_palette_cases_gpu.py runs them."""
import numpy as np

CELL = 8                   # colours per cell and axis
CELLS = 32 * 32 * 32
CAP = 31                   # candidates a 32-byte record holds; more: the cell is marked and its pixels walk the palette
MARKED = "marked"


# ------------------------------------------------------------------ cells
def cell_no(cr, cg, cb):
    return int(cr) | (int(cg) << 5) | (int(cb) << 10)


def cell_of(rgb):
    """cell number(s) of colour(s) (..., >= 3)"""
    c = np.asarray(rgb).astype(np.int64)
    return (c[..., 0] >> 3) | ((c[..., 1] >> 3) << 5) | ((c[..., 2] >> 3) << 10)


def cell_colours(cell):
    """the cell's 512 colours, (512, 3), red fastest"""
    lo = np.array([(cell & 31) << 3, ((cell >> 5) & 31) << 3, ((cell >> 10) & 31) << 3])
    t = np.arange(512)
    return np.stack([t & 7, (t >> 3) & 7, t >> 6], axis=1) + lo[None, :]


# ------------------------------------------------------------------ the model of pal_grid_kernel
def pg_chan(p, lo):
    """smallest and largest squared distance from entry value p to the interval [lo, lo + 7] of one channel"""
    hi = lo + 7
    d0 = max(lo - p, p - hi, 0)
    d1 = max(p - lo, hi - p)
    return d0 * d0, d1 * d1


def mind_maxd(rgb, cell):
    lo = ((cell & 31) << 3, ((cell >> 5) & 31) << 3, ((cell >> 10) & 31) << 3)
    mn = mx = 0
    for c in range(3):
        a, b = pg_chan(int(rgb[c]), lo[c])
        mn, mx = mn + a, mx + b
    return mn, mx


def grid_arrays(palette, cells):
    """(U (m,), candidate (m, n) bool, mind == U (m, n) bool) for the m cells: both loops of pal_grid_kernel, vectorised"""
    pal = np.asarray(palette)[:, :3].astype(np.int32)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    us, cands, ties = [], [], []
    for at in range(0, len(cells), 2048):
        c = cells[at:at + 2048]
        lo = np.stack([(c & 31) << 3, ((c >> 5) & 31) << 3, ((c >> 10) & 31) << 3], axis=1).astype(np.int32)[:, None, :]
        hi = lo + 7
        p = pal[None, :, :]
        d0 = np.maximum(np.maximum(lo - p, p - hi), 0)
        d1 = np.maximum(p - lo, hi - p)
        mind, maxd = (d0 * d0).sum(axis=2), (d1 * d1).sum(axis=2)
        u = maxd.min(axis=1)                                    # first loop: U = min over the entries of maxd
        us.append(u)
        cands.append(mind <= u[:, None])                        # second loop: `mn <= u`
        ties.append(mind == u[:, None])
    return np.concatenate(us), np.concatenate(cands), np.concatenate(ties)


def grid_lists(palette, cells):
    """per cell: (U, the candidate set, the entries with mind == U)"""
    u, cand, tie = grid_arrays(palette, cells)
    return [(int(u[k]), frozenset(np.nonzero(cand[k])[0].tolist()), frozenset(np.nonzero(tie[k])[0].tolist())) for k in range(len(u))]


def claimed(length):
    """the count byte of a record whose cell has `length` candidates"""
    return MARKED if length > CAP else length


# ------------------------------------------------------------------ the definition, for planes no construction fixes
def nearest_first(palette, px, among=None):
    """index of the nearest entry, the lowest index among equals: the minimum of dist * 256 + index.  among: only these indices"""
    pal = np.asarray(palette)[:, :3].astype(np.int64)
    idx = np.arange(len(pal), dtype=np.int64) if among is None else np.asarray(among, dtype=np.int64)
    flat = np.asarray(px)[..., :3].reshape(-1, 3).astype(np.int64)
    out = np.empty(len(flat), dtype=np.uint8)
    for at in range(0, len(flat), 8192):
        f = flat[at:at + 8192]
        dist = np.zeros((len(f), len(idx)), dtype=np.int64)
        for c in range(3):
            d = f[:, c:c + 1] - pal[idx, c][None, :]
            dist += d * d
        out[at:at + 8192] = ((dist * 256 + idx[None, :]).min(axis=1) & 255).astype(np.uint8)
    return out.reshape(np.asarray(px).shape[:-1])


# ------------------------------------------------------------------ palettes: planted entries spread over 0..n-1, far fillers
def assemble(planted, n, seed, far_ok, pin=None):
    """-> (palette (n, 4), pos: the index of each planted entry).  The planted entries take shuffled indices (pin: {planted
    number: index} fixes some), every other index a random colour that far_ok accepts."""
    rng = np.random.default_rng(seed)
    assert len(planted) <= n <= 256
    pos = rng.permutation(n)[:len(planted)].tolist()
    for j, at in (pin or {}).items():
        if at in pos:
            k = pos.index(at)
            pos[k], pos[j] = pos[j], pos[k]
        else:
            pos[j] = at
    assert len(set(pos)) == len(planted)
    pal = np.zeros((n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    for j, c in enumerate(planted):
        pal[pos[j], :3] = c
    for i in sorted(set(range(n)) - set(pos)):
        while True:
            c = rng.integers(0, 256, 3)
            if far_ok(c):
                break
        pal[i, :3] = c
    return pal, pos


def opaque(rgb, shape):
    """(h, w, 4) image of the colours, alpha 255"""
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(shape + (3,))
    return np.concatenate([rgb, np.full(shape + (1,), 255, np.uint8)], axis=2)


def padded(colours, pad, count):
    c = [tuple(int(v) for v in x) for x in colours]
    assert len(c) <= count
    return c + [tuple(pad)] * (count - len(c))


# ------------------------------------------------------------------ list_len_k
LIST_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
MIRRORED_LENS = (4, 8, 16, 32)
_NS = (256, 61, 131, 100)                 # 61 and 131: no multiple of 8


def _place(t):
    """cell (0,0,0)'s construction moved to cell (t,t,t): t = 31 mirrors it, so that the outside entries lie on the inner faces"""
    return (lambda v: 255 - np.asarray(v)) if t == 31 else (lambda v: np.asarray(v) + 8 * t)


def list_entries(k, t):
    """the k planted entries of cell (t,t,t): one at lo + 3 (maxd 48 = U), k - 1 one step outside a face (mind 1, maxd >= 64)"""
    assert 1 <= k <= 49 and t in (0, 2, 20, 31)
    base = [(3, 3, 3)]
    for u in (0, 2, 4, 6):
        for v in (0, 2, 4, 6):
            for axis in range(3):
                e = [u, v]
                e.insert(axis, 8)
                base.append(tuple(e))
    return [tuple(int(x) for x in _place(t)(e)) for e in base[:k]]


def list_len(k, t, n, seed):
    cell = cell_no(t, t, t)
    planted = list_entries(k, t)
    pin = {}
    if k >= 2:
        pin[1] = n - 1                    # a candidate at the palette's last index
    if k >= 3:
        pin[k - 1] = 0                    # ... and one at its first
    pal, pos = assemble(planted, n, seed, lambda c: mind_maxd(c, cell)[0] > 48, pin)
    img = opaque(cell_colours(cell), (2, 256))                   # each row: one wave, every pixel of it in the cell
    # the far entries are farther than the entry at lo + 3 from every colour of the cell: the plane is decided among the planted
    want = nearest_first(pal, img, among=sorted(pos))
    return pal, img, want, dict(cells={cell: k}, planted=pos, u=48)


# ------------------------------------------------------------------ rim_tie
def rim_tie(kind, order, mirror, wide):
    """corner: best (0,0,0) (maxd 147 = U), tied (14,14,14) (mind 147), pixel (7,7,7) at 147 from both.  axisA: best 0 on axis A
    and 3 on the others (maxd 49 + 16 + 16 = 81 = U), tied 16 on axis A and 7 on the others (mind 81): off one face only; the
    pixel (7,7,7) is at 81 from both.  Every other colour of the cell is strictly nearer the best entry.  order 'tied_first':
    the tied entry has index 0 and must win that pixel; 'best_first': the best entry has."""
    if kind == "corner":
        best, tied, u = (0, 0, 0), (14, 14, 14), 147
    else:
        axis = int(kind[-1])
        best, tied = [3, 3, 3], [7, 7, 7]
        best[axis], tied[axis], u = 0, 16, 81
    far, pixel = (200, 200, 200), (7, 7, 7)
    rim = [tuple(int(v) for v in c) for c in cell_colours(0) if 7 in c]                  # the cell's three faces towards the tied entry
    assert len(rim) == 169 and pixel in rim
    flip = (lambda c: tuple(255 - v for v in c)) if mirror else (lambda c: tuple(c))
    best, tied, far, pixel = flip(best), flip(tied), flip(far), flip(pixel)
    rim = [flip(c) for c in rim]
    entries = [tied, best, far] if order == "tied_first" else [best, tied, far]
    pal = opaque(entries, (1, 3))[0]
    i_best, i_tied = entries.index(best), entries.index(tied)
    colours = padded(rim, pixel, 256 if wide else 172)
    img = opaque(colours, (1, 256) if wide else (43, 4))
    is_pixel = (img[..., :3] == np.array(pixel, dtype=np.uint8)).all(axis=2)
    want = np.where(is_pixel, min(i_best, i_tied), i_best).astype(np.uint8)
    cell = int(cell_of(np.array(pixel)))
    return pal, img, want, dict(cells={cell: 2}, u=u, tied=i_tied, best=i_best, pixel=pixel)


# ------------------------------------------------------------------ midpoint_tie
MIDPOINTS = {"inside": ((20, 20, 20), 3), "at7": ((7, 7, 7), 2), "at8": ((8, 8, 8), 2)}


def midpoint_entries(m, where):
    p, d = MIDPOINTS[where]
    if m == 8:
        offs = [(a, b, c) for a in (-d, d) for b in (-d, d) for c in (-d, d)]
    else:
        offs = [tuple(s if k == axis else 0 for k in range(3)) for axis in range(m // 2) for s in (-d, d)]
    return [tuple(p[k] + o[k] for k in range(3)) for o in offs]


def midpoint_neighbourhood(where):
    p, _ = MIDPOINTS[where]
    return [(p[0] + a, p[1] + b, p[2] + c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1)]


def midpoint_palette(m, where, lowest, n, seed):
    """m entries at the same distance from the pixel; entry number `lowest` takes the lowest of their indices"""
    p, _ = MIDPOINTS[where]
    planted = midpoint_entries(m, where)
    far_ok = lambda c: max(abs(int(c[k]) - p[k]) for k in range(3)) >= 40            # >= 1600 away; the planted are within 48
    pal, pos = assemble(planted, n, seed, far_ok)
    ranks = sorted(pos)
    order = [lowest] + [j for j in range(m) if j != lowest]
    new = [0] * m
    for r, j in enumerate(order):
        new[j] = ranks[r]
    for j, c in enumerate(planted):
        pal[new[j], :3] = c
    return pal, new


def midpoint_tie(m, where, lowest, n, seed):
    p, _ = MIDPOINTS[where]
    pal, pos = midpoint_palette(m, where, lowest, n, seed)
    img = opaque(padded(midpoint_neighbourhood(where), p, 28), (7, 4))
    want = nearest_first(pal, img, among=sorted(pos))
    at_p = (img[..., :3] == np.array(p, dtype=np.uint8)).all(axis=2)
    assert (want[at_p] == pos[lowest]).all() and pos[lowest] == min(pos)
    return pal, img, want, dict(cells={}, planted=pos, pixel=p, lowest=pos[lowest])


# ------------------------------------------------------------------ duplicates
CROWD_CELL = cell_no(10, 10, 10)
LONE_CELL = cell_no(20, 20, 20)
LIST_CELL = cell_no(2, 2, 2)


def crowd(count, seed):
    """count distinct colours of CROWD_CELL"""
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in c) for c in cell_colours(CROWD_CELL)[rng.permutation(512)[:count]]]


def duplicate_pairs():
    """cell (2,2,2): three planted entries and a twin of the one at lo + 3 -- a list of 4; cell (10,10,10): 40 entries inside it
    and a twin of one of them -- marked.  The twins sit far behind their originals."""
    listed = list_entries(3, 2)
    crowded = crowd(40, 11)
    planted = listed + [listed[0]] + crowded + [crowded[0]]
    j_twin_l, j_crowd0, j_twin_c = 3, 4, 4 + 40
    pin = {0: 5, j_twin_l: 250, j_crowd0: 9, j_twin_c: 251, j_crowd0 + 1: 255}
    pal, pos = assemble(planted, 256, 21, lambda c: mind_maxd(c, LIST_CELL)[0] > 48, pin)
    img = opaque(np.concatenate([cell_colours(LIST_CELL), cell_colours(CROWD_CELL)]), (4, 256))
    want = nearest_first(pal, img)
    for colour, first in ((listed[0], 5), (crowded[0], 9), (crowded[1], 255)):
        hit = (img[..., :3] == np.array(colour, dtype=np.uint8)).all(axis=2)
        assert hit.sum() == 1 and (want[hit] == first).all()             # the pixel of a twinned colour takes the original
    return pal, img, want, dict(cells={LIST_CELL: 4, CROWD_CELL: MARKED}, planted=pos)


def one_colour():
    colour = (37, 99, 200)
    pal = opaque([colour] * 256, (1, 256))[0]
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    img[2, 3, :3] = colour
    img[..., 3] = 255
    return pal, img, np.zeros((5, 7), dtype=np.uint8), dict(cells={int(cell_of(np.array(colour))): MARKED, 0: MARKED, CELLS - 1: MARKED})


TWO_A, TWO_B = (200, 30, 40), (10, 220, 90)


def two_colours(pattern):
    """256 entries of two colours.  a_first: B at 100, 103, ...; b_first: B at 0, 1, 2 and from 200 on."""
    is_b = np.zeros(256, dtype=bool)
    if pattern == "a_first":
        is_b[100::3] = True
    else:
        is_b[:3] = True
        is_b[200:] = True
    pal = opaque(np.where(is_b[:, None], np.array(TWO_B), np.array(TWO_A)), (1, 256))[0]
    ia, ib = int(np.argmin(is_b)), int(np.argmax(is_b))
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (6, 8, 4), dtype=np.uint8)
    img[0, 0, :3], img[0, 1, :3], img[5, 7, :3] = TWO_A, TWO_B, (105, 125, 65)       # ... and the midpoint of the two: a tie
    img[..., 3] = 255
    c = img[..., :3].astype(np.int64)
    da, db = ((c - np.array(TWO_A)) ** 2).sum(axis=2), ((c - np.array(TWO_B)) ** 2).sum(axis=2)
    assert da[5, 7] == db[5, 7]
    want = np.where(da < db, ia, np.where(db < da, ib, min(ia, ib))).astype(np.uint8)
    cells = {int(cell_of(np.array(TWO_A))): MARKED, int(cell_of(np.array(TWO_B))): MARKED}
    return pal, img, want, dict(cells=cells, first=(ia, ib))


# ------------------------------------------------------------------ mixed_wave
MIXED_WIDTHS = (253, 255, 257, 259)
_MIXED = {}


def mixed_palette():
    """17 candidates in cell (2,2,2), one in cell (20,20,20), 40 entries inside cell (10,10,10) (marked)"""
    if not _MIXED:
        listed, lone, crowded = list_entries(17, 2), [(163, 163, 163)], crowd(40, 12)
        planted = listed + lone + crowded
        far_ok = lambda c: mind_maxd(c, LIST_CELL)[0] > 48 and mind_maxd(c, LONE_CELL)[0] > 48
        pal, pos = assemble(planted, 256, 22, far_ok, {17 + 1: 255, 1: 254, 17: 128})
        _MIXED.update(pal=pal, pos=pos, crowded=crowded)
    return _MIXED["pal"], _MIXED["pos"], _MIXED["crowded"]


def mixed_wave(w):
    pal, pos, crowded = mixed_palette()
    in_crowd = crowded + [tuple(int(v) for v in c) for c in cell_colours(CROWD_CELL)]
    sources = (in_crowd, cell_colours(LONE_CELL).tolist(), cell_colours(LIST_CELL).tolist())
    h = 2
    rows = [[sources[x % 3][(x // 3 + 171 * y) % len(sources[x % 3])] for x in range(w)] for y in range(h)]
    img = opaque(rows, (h, w))
    want = nearest_first(pal, img)
    x = np.arange(w)
    assert (want[:, x % 3 == 1] == 128).all()                                    # the lone cell's pixels: its one entry
    assert set(want[:, x % 3 == 2].reshape(-1).tolist()) <= set(pos[:17])
    assert want[0, 0] == 255 and tuple(img[0, 0, :3]) == crowded[0]              # the palette's last entry, from the marked cell
    return pal, img, want, dict(cells={LIST_CELL: 17, LONE_CELL: 1, CROWD_CELL: MARKED}, planted=pos)


# ------------------------------------------------------------------ every_cell
def every_cell_image():
    """256 x 128: pixel number c holds a colour of cell c, the offset inside the cell varying with c"""
    c = np.arange(CELLS, dtype=np.int64)
    hsh = (c * 2654435761) >> 7
    rgb = np.stack([((c & 31) << 3) + (hsh & 7), (((c >> 5) & 31) << 3) + ((hsh >> 3) & 7), (((c >> 10) & 31) << 3) + ((hsh >> 6) & 7)], axis=1)
    return opaque(rgb, (128, 256))


def random_palette(n, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    return pal


def clustered_palette(n, seed):
    """entries crowded around a few centres (what medianCut makes of a photograph): long lists, marked cells, near ties"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, size=(max(1, n // 24), 3))
    rgb = np.clip(centres[rng.integers(0, len(centres), size=n)] + rng.integers(-6, 7, size=(n, 3)), 0, 255)
    return opaque(rgb, (1, n))[0]


def every_cell(kind):
    pal = random_palette(256, 41) if kind == "random" else clustered_palette(256, 42)
    img = every_cell_image()
    return pal, img, nearest_first(pal, img), dict(cells={})


# ------------------------------------------------------------------ alpha_ignored
def alpha_ignored(base):
    pal, img, want, info = base._get()[:4]
    rng = np.random.default_rng(8)
    out = img.copy()
    out[..., 3] = rng.integers(0, 256, img.shape[:2], dtype=np.uint8)
    out[0, 0, 3], out[-1, -1, 3] = 0, 254
    return pal, out, want, info


# ------------------------------------------------------------------ the cases
class Case:
    """name, kind, palette (n, 4), img, want (the index plane), info (cells: {cell: planted list length or MARKED}); made once, read-only"""

    def __init__(self, name, kind, make):
        self.name, self.kind, self._make, self._made = name, kind, make, None

    def _get(self):
        if self._made is None:
            pal, img, want, info = self._make()
            pal, img, want = np.ascontiguousarray(pal, dtype=np.uint8), np.ascontiguousarray(img, dtype=np.uint8), np.ascontiguousarray(want, dtype=np.uint8)
            assert pal.ndim == 2 and pal.shape[1] == 4 and (pal[:, 3] == 255).all() and img.shape[:2] == want.shape
            for a in (pal, img, want):
                a.setflags(write=False)
            self._made = (pal, img, want, info)
        return self._made

    palette = property(lambda self: self._get()[0])
    img = property(lambda self: self._get()[1])
    want = property(lambda self: self._get()[2])
    info = property(lambda self: self._get()[3])

    def __repr__(self):
        return self.name


def _cases():
    c = []
    add = lambda name, kind, make: c.append(Case(name, kind, make))
    for i, k in enumerate(LIST_LENS):
        n = max(_NS[i % 4], 35 + (k > 30) * 26)
        add(f"list_len_{k}", "list_len", lambda k=k, n=n, i=i: list_len(k, 2, n, 100 + i))
    for i, k in enumerate(MIRRORED_LENS):
        for t in (0, 31):
            n = _NS[(i + (t == 31)) % 4]
            add(f"list_len_{k}_cell{t}", "list_len", lambda k=k, t=t, n=n, i=i: list_len(k, t, n, 200 + 2 * i + (t == 31)))
    for wide in (False, True):
        tail = "_256w" if wide else "_4w"
        for kind in ("corner", "axis0", "axis1", "axis2"):
            for order in ("tied_first", "best_first"):
                add(f"rim_tie_{kind}_{order}{tail}", "rim_tie", lambda kind=kind, order=order, wide=wide: rim_tie(kind, order, False, wide))
        add(f"rim_tie_corner_mirror{tail}", "rim_tie", lambda wide=wide: rim_tie("corner", "tied_first", True, wide))
        add(f"rim_tie_axis1_mirror{tail}", "rim_tie", lambda wide=wide: rim_tie("axis1", "tied_first", True, wide))
    s = 0
    for m in (2, 4, 8):
        for where in MIDPOINTS:
            for lowest in range(m):
                n = (m + 1, 256, 29)[s % 3]
                add(f"midpoint_tie_{m}_{where}_low{lowest}", "midpoint_tie", lambda m=m, where=where, lowest=lowest, n=n, s=s: midpoint_tie(m, where, lowest, n, 300 + s))
                s += 1
    add("duplicates_pairs", "duplicates", duplicate_pairs)
    add("duplicates_one_colour", "duplicates", one_colour)
    add("duplicates_two_colours_a_first", "duplicates", lambda: two_colours("a_first"))
    add("duplicates_two_colours_b_first", "duplicates", lambda: two_colours("b_first"))
    for w in MIXED_WIDTHS:
        add(f"mixed_wave_{w}", "mixed_wave", lambda w=w: mixed_wave(w))
    add("every_cell_random", "every_cell", lambda: every_cell("random"))
    add("every_cell_clustered", "every_cell", lambda: every_cell("clustered"))
    by = {x.name: x for x in c}
    add("alpha_ignored_list_len_5", "alpha_ignored", lambda: alpha_ignored(by["list_len_5"]))
    add("alpha_ignored_mixed_wave_255", "alpha_ignored", lambda: alpha_ignored(by["mixed_wave_255"]))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

# the presentations of tests/test_palette_cases_gpu.py (device tensors and views, want_quantized=False)
PRESENTED = ("list_len_16", "rim_tie_corner_tied_first_4w", "mixed_wave_255")
