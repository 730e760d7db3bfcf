"""Scenes of the host-frame delivery suite (csrc/vrt_host_frame.hip behind csrc/vrt_hip_host_frame.cpp: vrt_hip_host_register,
vrt_hip_frame_host, vrt_hip_host_unregister): the geometries, crafted scenes whose lit cells are known, a model that predicts for
every delivery its mode and the exact set of words it writes, and the cases both tests run.  numpy only, no GPU; the one import is the
assembly suite's map from a cell key to its raster rectangle.

tests/test_gpu_host_frame_cells.py poisons the whole registered buffer before every delivery and asserts afterwards that the buffer
equals where(written, fresh render, poison) on every word -- `written` is this model's.  tests/test_host_frame_scenes.py checks on the
CPU that the scenes light the cells they name (by the list suite's cull model) and that each wrong variant of the model (WRONG) is seen
by at least one case.

  geometry(name, bg, pixels)        tile grid, cell grid and background of a delivery, from w, h, tw, th alone
  cell_pixels(geo, key)             the raster words of a cell (the key -> rectangle map is assembly_scenes.cell_pixels)
  spots / flood / dark / scene_of   Gaussians under the pinhole camera of scene.cli_camera(w, h) with a known lit set
  DeliveryModel                     per-buffer histories, the two tally words and the published count of one context
  CASES                             name -> Case(buffers, steps, retain); run(case, wrong) -> what every delivery must do

The rules of the model are the ones include/vrt_hip.h ("host frames") and the head of csrc/vrt_hip_host_frame.cpp state.
  full    the first delivery after registration; a frame that kept no stamps; an image size, tile grid or background other than that of
          the buffer's recorded history; a published count c with 4 c > 3 n_cells.  Writes words 0 .. w*h - 1, nothing beyond.  A
          full delivery without stamps records nothing: the delivery after it is a full one too.
  delta   every other delivery: the pixels of the cells lit now (frame) and of the cells of the history that are dark now (background).
  count   every launch (one per delivery with stamps) adds its count -- |lit| after a full copy, |lit u held| in a delta -- to
          tally[launches & 1] and publishes, then clears, the other word: with a sync between deliveries a delivery reads the count of
          the launch before the previous launch on that buffer.  A delivery without stamps launches nothing.  Registration clears the
          slot's words; a slot is the lowest free number.
  stamps  a frame keeps its stamps iff the fused list kernel ran (at most MAX_FUSED_CELLS cells per tile) on a context that retains its
          frame (VRT_HIP_RETAIN_FRAME unset).  vrt_hip_frame_host builds the lists of every frame anew, so a repeated pose keeps them.
"""
from types import SimpleNamespace

import numpy as np

import assembly_scenes as A

CELL = 32
MAX_FUSED_CELLS = 64                            # csrc/vrt_kernels.h
MAX_HOST_BUFFERS = 16                           # vrt_hip_ctx::MAX_HOST_BUFFERS
BG = A.BG                                       # "mode8": 0 (computed alpha), "opaque": 0xFF000000
POISON = 0x5EEDF00D                             # no frame of a case may hold it: the GPU test asserts that of every expected frame
DEPTH = 5.0                                     # plane distances between the eye and every crafted Gaussian
EYE = np.array([0.0, 0.0, -4.0])                # scene.cli_camera: looks along +z, plane point of pixel (x, y) = (-1 + 2x/w, -1 + 2y/h, -3)
SPOT_SIGMA_PX, SPOT_MAGNITUDE = 0.4, 4.0        # a spot: 0.4 pixels wide where the pixels are smallest, bright enough to show
GAUSSIAN = np.dtype([("albedo", np.float32, 4), ("mu", np.float32, 4), ("sigma", np.float32), ("magnitude", np.float32)])

# name: (w, h, tw, th) and what tile_geometry must make of it: (tiles_w, tiles_h, tile_w, tile_h, stride, cells_x, cells_y)
GEOMETRIES = {
    "128x128": ((128, 128, 1.0, 1.0), (2, 2, 64, 64, 128, 2, 2)),          # the base: 16 exact cells, 4 workgroups
    "96x40": ((96, 40, 2.0 / 3.0, 2.0), (3, 1, 32, 40, 96, 1, 2)),         # 6 cells: the second workgroup has two waves; cells of 8 rows
    "32x32": ((32, 32, 2.0, 2.0), (1, 1, 32, 32, 32, 1, 1)),               # one cell
    "64x32": ((64, 32, 1.0, 2.0), (2, 1, 32, 32, 64, 1, 1)),               # two cells
    "70x44": ((70, 44, 1.0, 1.0), (2, 2, 35, 22, 70, 2, 1)),               # tile_w % 4 = 3: dwords, quads that straddle the tile's edge, cells of 3 columns
    "80x54": ((80, 54, 1.0, 1.0), (2, 2, 40, 27, 80, 2, 1)),               # quads; a partial cell of 8 columns, clipped rows
    "65x33": ((65, 33, 1.0, 1.0), (2, 2, 32, 16, 64, 1, 1)),               # w*h % 4 = 1: dwords; stride below the width, sheared rows, a tail of 97 words
    "288x288": ((288, 288, 2.0, 2.0), (1, 1, 288, 288, 288, 9, 9)),        # 81 cells in one tile: no fused list kernel, no stamps
    "96x96": ((96, 96, 1.0, 1.0), (2, 2, 48, 48, 96, 2, 2)),               # the other image size of the fall-back cases; cells of 16 columns and rows
    "128x128/4": ((128, 128, 0.5, 0.5), (4, 4, 32, 32, 128, 1, 1)),        # the other tile grid over the base image, 16 cells too
    "64x32/3": ((64, 32, 1.0, 0.75), (2, 3, 32, 12, 64, 1, 1)),            # three tile rows of 12 over 32 rows: the last overhangs the image
}
# wrong variants of the model, one changed line each (tests/test_host_frame_scenes.py)
WRONG = ("one-history", "held-not-reset", "lit-skipped-when-held", "dense-at-3/4", "lag-one", "count-lit-only", "history-only-no-record",
         "nostamps-shifts-parity", "columns-beyond-tile", "beyond-image", "register-keeps-count", "full-writes-buffer")


# ---- geometry ----
def geometry(name, bg="mode8", pixels=None):
    """The delivery geometry `name` with background `bg` into a registered buffer of `pixels` words (default: w * h).  float32
    arithmetic as the header and DESIGN.md give it: tiles ceil(2 / tw) by ceil(2 / th), a tile floor(w tw / 2) by floor(h th / 2)."""
    w, h, tw, th = GEOMETRIES[name][0]
    f, two = np.float32, np.float32(2.0)
    g = SimpleNamespace(name=name, w=w, h=h, tw=float(f(tw)), th=float(f(th)), bg=bg, background=BG[bg])
    g.tiles_w, g.tiles_h = int(np.ceil(two / f(tw))), int(np.ceil(two / f(th)))
    g.tile_w, g.tile_h = int(f(w) * f(tw) / two), int(f(h) * f(th) / two)
    g.stride = g.tile_w * g.tiles_w
    g.cells_x, g.cells_y = -(-g.tile_w // CELL), -(-g.tile_h // CELL)
    g.cpt = g.cells_x * g.cells_y
    g.tiles = g.tiles_w * g.tiles_h
    g.n_cells = g.tiles * g.cpt
    g.npix = w * h
    g.pixels = g.npix if pixels is None else pixels
    g.refine = g.stride == w                     # tiles are rectangles of the image: the list kernels cull by tile and cell cones
    g.fused = g.cpt <= MAX_FUSED_CELLS           # the fused list kernel runs: the frame keeps its stamps
    g.sig = (w, h, g.tiles_w, g.tiles_h, g.tile_w, g.tile_h, g.background)
    assert g.pixels >= g.npix
    return g


def cell_pixels(geo, key, wrong=None):
    """The raster word indices of cell `key` = tile * cells per tile + cell, sorted: tx tile_w + x + stride (ty tile_h + y) without
    the columns at or beyond tile_w, the rows at or beyond tile_h and the indices at or beyond w * h."""
    if wrong == "beyond-image":                  # ... or only those beyond the registered buffer
        geo = SimpleNamespace(**dict(vars(geo), npix=geo.pixels))
    pix, inside = A.cell_pixels(geo, key, "no-quad-guard" if wrong == "columns-beyond-tile" else None)
    return np.sort(pix[inside])


def cell_of_word(geo):
    """Per word of the registered buffer the key of the cell that owns it, -1 for a word no tile covers, -2 beyond the image."""
    owner = np.full(geo.pixels, -1, np.int64)
    owner[geo.npix:] = -2
    for key in range(geo.n_cells):
        owner[cell_pixels(geo, key)] = key
    return owner


# ---- scenes ----
def cell_centre(geo, key):
    """The image position (x, y), in pixels, that a spot of cell `key` is seen at: the centre of the cell's rectangle, clipped to its
    tile and to the image.  Where the tiles are no rectangles of the image (65x33) nothing culls by cell: a cell -- the whole tile --
    is lit iff the reference's tile test keeps the Gaussian, |x_tile - p| <= |x_tile| + tw / 2 + 3.3 sigma_p on both axes with p =
    the centre seen from the PLANE (not the eye).  For two tiles per axis that is p beyond -+(0.5 + 3.3 sigma_p): the spot goes to
    p = -+0.75."""
    t, ci = divmod(key, geo.cpt)
    ty, tx = divmod(t, geo.tiles_w)
    if not geo.refine:
        assert geo.cpt == 1 and geo.tiles_w == geo.tiles_h == 2
        p = np.array([(-0.75, 0.75)[tx], (-0.75, 0.75)[ty]]) * (DEPTH - 1.0) / DEPTH          # seen from the plane -> seen from the eye
        return (p[0] + 1.0) * geo.w / 2.0, (p[1] + 1.0) * geo.h / 2.0
    x0, y0 = (ci % geo.cells_x) * CELL, (ci // geo.cells_x) * CELL
    x1, y1 = min(x0 + CELL, geo.tile_w) - 1, min(y0 + CELL, geo.tile_h) - 1
    y1 = min(ty * geo.tile_h + y1, geo.h - 1) - ty * geo.tile_h
    return tx * geo.tile_w + (x0 + x1) / 2.0, ty * geo.tile_h + (y0 + y1) / 2.0


def _gaussians(mu, sigma, magnitude, colour):
    g = np.zeros(len(mu), GAUSSIAN)
    g["mu"][:, :3] = mu
    g["albedo"][:, :3] = colour
    g["albedo"][:, 3] = 1.0
    g["sigma"], g["magnitude"] = sigma, magnitude
    return g


def at_pixel(geo, x, y, depth=DEPTH):
    """The world point that the camera of scene.cli_camera(w, h) sees at image position (x, y), `depth` plane distances away."""
    return EYE + depth * np.array([-1.0 + 2.0 * x / geo.w, -1.0 + 2.0 * y / geo.h, 1.0])


def spots(geo, cells, fatten=1.0):
    """One narrow Gaussian per named cell, at cell_centre: the lit set is exactly `cells` (tests/test_host_frame_scenes.py asserts it
    with the list suite's cull model, at 1.5 times this sigma as well: room to spare).  sigma is SPOT_SIGMA_PX of the smaller pixel
    pitch at that depth (2 depth / w by 2 depth / h)."""
    cells = sorted(cells)
    assert cells and all(0 <= k < geo.n_cells for k in cells)
    sigma = fatten * SPOT_SIGMA_PX * 2.0 * DEPTH / max(geo.w, geo.h)
    mu = np.array([at_pixel(geo, *cell_centre(geo, k)) for k in cells])
    colour = np.array([[0.3 + 0.7 * ((k * 0.37) % 1.0), 0.3 + 0.7 * ((k * 0.61) % 1.0), 0.9] for k in cells])
    return _gaussians(mu, sigma, SPOT_MAGNITUDE, colour)


def flood(geo):
    """One wide Gaussian in the middle of the view: every cell is lit."""
    return _gaussians(at_pixel(geo, geo.w / 2.0, geo.h / 2.0)[None, :], 3.0, 1.0, np.array([[0.9, 0.5, 0.2]]))


def dark(geo):
    """One Gaussian behind the camera: the reference's tile test files it in no tile, no cell is lit."""
    return _gaussians(np.array([[0.0, 0.0, -10.0]]), 0.5, 1.0, np.array([[1.0, 1.0, 1.0]]))


_scenes = {}


def scene_of(geo, what):
    """what: "flood", "dark" or a collection of cell keys.  Returns Scene(g, lit) -- built once per geometry, background aside."""
    what = what if isinstance(what, str) else tuple(sorted(what))
    key = (geo.name, what)
    if key not in _scenes:
        if what == "flood":
            g, lit = flood(geo), frozenset(range(geo.n_cells))
        elif what == "dark":
            g, lit = dark(geo), frozenset()
        else:
            g, lit = spots(geo, what), frozenset(what)
        _scenes[key] = SimpleNamespace(what=what, g=g, lit=lit)
    return _scenes[key]


def first_cells(k):
    """The cells of a scene with exactly k lit cells: the first k."""
    return tuple(range(k))


# ---- the model ----
class Refused(Exception):
    pass


class DeliveryModel:
    """The host buffers of one context.  deliver() returns (mode, written): "full" or "delta" and the sorted word indices that the
    delivery writes.  wrong: one of WRONG."""

    def __init__(self, wrong=None):
        assert wrong is None or wrong in WRONG
        self.wrong, self.bufs = wrong, {}
        self.slots = [SimpleNamespace(tally=[0, 0], published=0) for _ in range(MAX_HOST_BUFFERS)]
        self.shared = self._history()

    @staticmethod
    def _history():
        return SimpleNamespace(valid=False, sig=None, lit=frozenset())

    def register(self, buf, pixels):
        if len(self.bufs) >= MAX_HOST_BUFFERS:
            raise Refused(buf)
        assert buf not in self.bufs
        slot = min(set(range(MAX_HOST_BUFFERS)) - {b.slot for b in self.bufs.values()})
        if self.wrong != "register-keeps-count":
            self.slots[slot].tally, self.slots[slot].published = [0, 0], 0
        self.bufs[buf] = SimpleNamespace(pixels=pixels, slot=slot, launches=0, history=self._history())

    def unregister(self, buf):
        del self.bufs[buf]

    def published(self, buf):
        return self.slots[self.bufs[buf].slot].published

    def deliver(self, buf, geo, lit, stamps):
        b, wrong = self.bufs[buf], self.wrong
        assert b.pixels == geo.pixels >= geo.npix
        s = self.slots[b.slot]
        h = self.shared if wrong == "one-history" else b.history
        lit = frozenset(lit)
        dense = 4 * s.published >= 3 * geo.n_cells if wrong == "dense-at-3/4" else 4 * s.published > 3 * geo.n_cells
        if stamps and h.valid and h.sig == geo.sig and not dense:
            mode, held = "delta", h.lit
            frame = lit - held if wrong == "lit-skipped-when-held" else lit
            reset = frozenset() if wrong == "held-not-reset" else held - lit
            cells = [cell_pixels(geo, k, wrong) for k in sorted(frame | reset)]
            written = np.unique(np.concatenate(cells)) if cells else np.zeros(0, np.int64)
            count = len(lit) if wrong == "count-lit-only" else len(lit | held)
        else:
            mode, count = "full", len(lit)
            written = np.arange(geo.pixels if wrong == "full-writes-buffer" else geo.npix)
            h.valid = False
            if not stamps:                       # nothing to record, nothing launched
                if wrong == "nostamps-shifts-parity":
                    b.launches += 1
                return mode, written
        if not (mode == "full" and wrong == "history-only-no-record"):
            h.lit = lit
        h.sig, h.valid = geo.sig, True
        parity = b.launches & 1
        b.launches += 1
        s.tally[parity] += count
        other = parity if wrong == "lag-one" else parity ^ 1
        s.published, s.tally[other] = s.tally[other], 0
        return mode, written


# ---- cases ----
def D(buf, geo, what, bg="mode8", set_view=True):
    """A delivery of scene `what` at geometry `geo` into buffer `buf`.  set_view: the caller sets the camera before the frame."""
    return SimpleNamespace(op="deliver", buf=buf, geo=geo, what=what, bg=bg, set_view=set_view)


def F(geo, what, bg="mode8"):
    """A frame into the context's own buffer, not delivered."""
    return SimpleNamespace(op="frame", geo=geo, what=what, bg=bg)


def R(geo, what, bg="mode8"):
    """A vrt_hip_render into the context's own buffer."""
    return SimpleNamespace(op="render", geo=geo, what=what, bg=bg)


def Reg(buf, refused=False):
    return SimpleNamespace(op="register", buf=buf, refused=refused)


def Unreg(buf):
    return SimpleNamespace(op="unregister", buf=buf)


def _case(steps, buffers=None, retain=True, registered=True):
    """buffers: name -> words (default: one buffer "A" as large as the largest image delivered into it).  registered: every buffer is
    registered, in order, before the first step."""
    if buffers is None:
        buffers = {}
        for s in steps:
            if s.op == "deliver":
                buffers[s.buf] = max(buffers.get(s.buf, 0), geometry(s.geo).npix)
    steps = ([Reg(b) for b in buffers] if registered else []) + list(steps)
    return SimpleNamespace(buffers=buffers, steps=steps, retain=retain)


def _seq(geo, whats, buf="A", **kw):
    return [D(buf, geo, w, **kw) for w in whats]


BASE = "128x128"
K12, K13 = first_cells(12), first_cells(13)                # of 16: 4 * 12 = 3 * 16 stays a delta, 13 switches
EVEN8, ODD8 = tuple(range(0, 16, 2)), tuple(range(1, 16, 2))
BIG = 288 * 288
# 70x44 and 80x54: the pixels are taller than wide, and the cone of a cell is round: a spot in a narrow cell lights the cells beside
# it, one in a wide cell the narrow cell of its tile.  The named sets are closed under that; the narrow cells 1, 3, 5, 7 still light
# up, stay and go dark on their own turns.
NARROW = [(0, 1, 2, 3), (2, 3), (6, 7), (4, 5, 6, 7), (2, 3, 6, 7), "dark", "flood", (2, 3)]


def _sixteen():
    names = [f"B{i:02d}" for i in range(MAX_HOST_BUFFERS)]
    what = lambda i, rnd: "flood" if i % 2 == 0 else ((i + rnd) % 16,)       # noqa: E731  even buffers go dense, odd ones move a spot
    steps = [Reg(b) for b in names] + [Reg("B16", refused=True)]
    for rnd in range(4):
        steps += [D(b, BASE, what(i, rnd)) for i, b in enumerate(names)]
    steps += [Unreg("B08"), Reg("B08")]                                          # the middle slot, with a dense history behind it
    for rnd in range(4, 8):
        steps += [D(b, BASE, what(i, rnd)) for i, b in enumerate(names[6:11], 6)]
    return _case(steps, buffers={b: 128 * 128 for b in names + ["B16"]}, registered=False)


CASES = {
    # the base geometry
    "base-light-move-dark": _case(_seq(BASE, [(1, 6), (1, 6, 11), (6, 12), (12, 13), "dark", (3,), "dark", "dark"])),
    "base-same-twice": _case(_seq(BASE, [(2, 5, 9), (2, 5, 9), (2, 5, 9)])),
    "base-all-dark": _case(_seq(BASE, ["dark", "dark", "dark"])),
    "base-all-lit": _case(_seq(BASE, ["flood", "flood"])),
    "base-one-cell": _case(_seq(BASE, [(7,), (7,), (8,), (7,)])),
    # cell counts that are no multiple of the four cells of a workgroup
    "6-cells": _case(_seq("96x40", [(0,), (0, 1), (3,), (3, 4, 5), "dark", "flood", (0, 2, 4), (4, 5), (3,)])),
    "1-cell": _case(_seq("32x32", [(0,), "dark", "dark", (0,), (0,)])),
    "2-cells": _case(_seq("64x32", [(0,), (1,), (0, 1), "dark", (1,)])),
    # dwords because of the tile width; the narrow cells' neighbours are lit with them (their cones hold the whole narrow cell)
    "3-columns": _case(_seq("70x44", NARROW)),
    "8-columns": _case(_seq("80x54", NARROW)),
    # dwords because of the pixel count
    "sheared": _case(_seq("65x33", [(0,), (0, 3), (1, 2), "dark", "flood", (2,), (3,)])),
    # tile rows beyond the image's end: `pix < npix` is live; the buffer is as large as the tile grid
    "overhang": _case(_seq("64x32/3", [(4,), (4, 5), (0, 5), "dark", "flood", (5,), (1, 4)]), buffers={"A": 64 * 36}),
    # no stamps: every delivery is a full one
    "81-cells": _case(_seq("288x288", ["flood", "flood", "dark", (40,), (40,)])),
    "no-retain": _case(_seq(BASE, [(1, 6), (1, 6), (6, 7), "dark"]), retain=False),
    # the same pose again with nothing set in between: the lists are rebuilt, the stamps kept, the delivery a delta
    "repeated-pose": _case([D("A", BASE, (1, 6))] + _seq(BASE, [(1, 6), (1, 6), (1, 6)], set_view=False) + [D("A", BASE, (1, 7)), D("A", BASE, (1, 7), set_view=False)]),
    # changes that fall back to a full copy, each followed by a delta
    "fall-backs": _case([D("A", BASE, (1, 6)), D("A", BASE, (1, 7)), D("A", BASE, (1, 7), "opaque"), D("A", BASE, (2, 7), "opaque"),
                         D("A", BASE, (2, 7)), D("A", BASE, (2,)), D("A", "96x96", (0, 3)), D("A", "96x96", (3, 12, 13)), D("A", BASE, (5, 6)),
                         D("A", BASE, (6,)), D("A", "128x128/4", (6, 9)), D("A", "128x128/4", (9, 10)), D("A", BASE, (9, 10)), D("A", BASE, (10,))]),
    "larger-buffer": _case([D("A", "96x96", (0, 3)), D("A", "96x96", (3, 12)), D("A", "96x96", (3, 12), "opaque"), D("A", "96x96", (12, 13), "opaque"),
                            D("A", "96x96", "flood", "opaque"), D("A", "96x96", "flood", "opaque"), D("A", "96x96", "flood", "opaque")],
                           buffers={"A": 128 * 128 + 64}),
    # the dense switch: 16 cells, 4 c > 48 <=> c >= 13
    "dense-12": _case(_seq(BASE, [K12] * 6)),
    "dense-13": _case(_seq(BASE, [K13] * 6)),
    "dense-lag": _case(_seq(BASE, [(1, 6), (1, 7), (2, 7)] + ["flood"] * 4 + [(2, 7), (2, 8), (3, 8), (3, 9)])),
    "dense-union": _case(_seq(BASE, [EVEN8, ODD8, EVEN8, ODD8, EVEN8, ODD8, EVEN8])),
    "dense-no-stamps": _case(_seq(BASE, ["flood"] * 3) + [D("A", "288x288", "flood")] + _seq(BASE, [(1,), (1, 2), (2,), (3,)]), buffers={"A": BIG}),
    # buffers
    "two-buffers": _case([D("A", BASE, (1, 6)), D("B", BASE, (9, 10)), D("A", BASE, (1, 7)), D("B", BASE, "flood"), D("A", BASE, (7,)),
                          D("B", BASE, "flood"), D("A", BASE, "dark"), D("B", BASE, "flood"), D("A", BASE, (3,)), D("B", BASE, (10,)),
                          D("A", BASE, (3, 4)), D("B", BASE, (10, 11))]),
    "sixteen-buffers": _sixteen(),
    "frames-between": _case([D("A", BASE, (1, 6)), F(BASE, (9,)), F(BASE, "dark"), R(BASE, (3,)), D("A", BASE, (1, 7)), F(BASE, "flood"),
                             D("A", BASE, (7,)), R(BASE, "flood"), D("A", BASE, (7, 8))]),
}
UNSYNCED = "two-buffers"                         # the case that the GPU test also enqueues without a sync between deliveries


def keeps_stamps(geo, retain=True):
    """plan_frame's rule: the stamps of a frame are kept by the fused list kernel, on a context that retains its frame."""
    return bool(retain and geo.fused)


def run(case, wrong=None):
    """What every step of the case must do, by the model: a list parallel to case.steps of None (nothing to compare) or
    Expect(geo, scene, mode, written)."""
    m, out = DeliveryModel(wrong), []
    for s in case.steps:
        e = None
        if s.op == "register":
            try:
                m.register(s.buf, case.buffers[s.buf])
                assert not s.refused, s.buf
            except Refused:
                assert s.refused, s.buf
        elif s.op == "unregister":
            m.unregister(s.buf)
        elif s.op == "deliver":
            geo = geometry(s.geo, s.bg, case.buffers[s.buf])
            sc = scene_of(geo, s.what)
            mode, written = m.deliver(s.buf, geo, sc.lit, keeps_stamps(geo, case.retain))
            e = SimpleNamespace(geo=geo, scene=sc, mode=mode, written=written)
        out.append(e)
    return out


def final_frames(case):
    """Per buffer the last delivery into it: (geo, scene) -- what the buffer holds when everything has landed."""
    last = {}
    for s, e in zip(case.steps, run(case)):
        if e is not None:
            last[s.buf] = (e.geo, e.scene)
    return last
