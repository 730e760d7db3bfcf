"""Scenes of the frame assembly suite (csrc/vrt_assembly_kernel.hip behind csrc/vrt_hip_assembly.cpp): the tile geometry of an
assembling context, crafted sparse shards and compact gathers, and a numpy model of what the kernels must leave in the frame buffer.

Everything here is integer data movement, so the model is exact and the GPU test (tests/test_gpu_assembly.py) asserts equalities.  The
CPU test (tests/test_assembly_scenes.py) checks the scenes themselves: the geometries, the model against sharding.py where both apply,
and that each of the wrong variants of the model (WRONG) changes an image that the GPU test holds.

  geometry(w, h, tw, th, world)          what tile_geometry / prepare_tile_grid / rebuild_shard / sparse_capacity make of a job
  block / cells_of / build_shard         a shard from an explicit list of (key, 32x32 pixels); free slots and the part of a stored cell
                                         outside its tile hold sentinels that must never reach an image
  full(shards, geo, bg, slots)           the frame a full assembly leaves
  Histories                              the retained assembly with its stamps and sequence numbers, per frame buffer
  compact(gathered, stride, table, ..)   the frame the compact kernel leaves
  frame_shards / sequence / history_ops  the crafted frames, retained sequences and buffer rotations both tests run
"""
from types import SimpleNamespace

import numpy as np

from conftest import load_pkg

load_pkg()
from sgrt_amd import sharding  # noqa: E402

CELL, HDR = sharding.CELL, sharding.SPARSE_HDR_WORDS
MAX_SHARDS = MAX_FRAMES = 64                    # csrc/vrt_kernels.h: MAX_SHARDS, MAX_ASSEMBLY_FRAMES
SENT_FREE = 0xDEADBEEF                          # key and pixel slots at and beyond n; padded slots of a compact gather
SENT_OUT = 0xBADC0DE5                           # pixels of a stored cell outside its tile
PREFILL = 0x5A5A5A5A                            # frame buffers before the first assembly
BG = {"mode8": 0, "opaque": 0xFF000000}         # VRT_ALPHA_COMPUTED / VRT_ALPHA_OPAQUE: what an assembly writes where nothing is lit
PIXEL_TAG = 0x40000000                          # stored pixels are PIXEL_TAG | 24 random bits (not 0): no sentinel, background or prefill

# name: (w, h, tw, th) and what the context must make of it: (tiles_w, tiles_h, tile_w, tile_h, stride)
GEOMETRIES = {
    "128x128": ((128, 128, 1.0, 1.0), (2, 2, 64, 64, 128)),       # exact cells; 16 frame cells, less than one wave
    "71x45": ((71, 45, 1.0, 1.0), (2, 2, 35, 22, 70)),            # tile_w % 4 = 3, partial cells on both axes, sheared rows, 115-pixel tail
    "200x136": ((200, 136, 0.4, 0.4), (5, 5, 40, 27, 200)),       # what the renderer tests use; 200-pixel tail
    "100x64": ((100, 64, 0.3, 0.5), (7, 4, 15, 16, 105)),         # stride > width: span 6720 > 6400 pixels, `pix < npix` is live
    "96x40": ((96, 40, 2.0 / 3.0, 2.0), (3, 1, 32, 40, 96)),      # grid and tiles not square; a cell row of 8 pixels
    "396x396": ((396, 396, 1.0 / 3.0, 1.0 / 3.0), (6, 6, 66, 66, 396)),   # 324 frame cells: a second block whose second wave has 4 live lanes
    "512x512": ((512, 512, 1.0, 1.0), (2, 2, 256, 256, 512)),     # 65536-pixel tiles: four passes of the compact kernel's loop
    "32x32": ((32, 32, 2.0, 2.0), (1, 1, 32, 32, 32)),            # one cell: the cheap image of the 64-buffer tests
    "64x32": ((64, 32, 1.0, 2.0), (2, 1, 32, 32, 64)),            # two cells: the 64-buffer tests with a lit cell that moves
}
WORLDS = (1, 2, 3, 8)
WRONG = ("no-quad-guard", "no-row-guard", "stride-is-width", "no-npix-guard", "no-header-check", "slots-beyond-n", "n-not-clamped",
         "tail-is-bg", "clear-not-clipped", "stale-is-seq", "no-stamp", "background-survives", "grid-survives", "padded-is-tile0")


def geometry(w, h, tw, th, world):
    """The job of an assembling context: float32 arithmetic as tile_geometry and prepare_tile_grid do it."""
    tw, th, two = np.float32(tw), np.float32(th), np.float32(2.0)
    g = SimpleNamespace(w=w, h=h, tw=float(tw), th=float(th), world=world)
    g.tiles_w, g.tiles_h = int(np.ceil(two / tw)), int(np.ceil(two / th))
    g.tile_w, g.tile_h = int(np.float32(w) * tw / two), int(np.float32(h) * th / two)
    g.tiles = g.tiles_w * g.tiles_h
    g.stride = g.tile_w * g.tiles_w
    g.npix = w * h
    g.span = g.stride * g.tile_h * g.tiles_h
    g.covered = min(g.npix, g.span)
    g.cells_x, g.cells_y = -(-g.tile_w // CELL), -(-g.tile_h // CELL)
    g.cpt = g.cells_x * g.cells_y
    g.table = sharding.shard_table(g.tiles_w, g.tiles_h, world)
    g.slots = g.table.shape[1]
    g.max_cells = g.slots * g.cpt
    g.frame_cells = g.tiles * g.cpt
    g.P = sharding.sparse_pixel_offset(g.max_cells)
    g.words = g.P + g.max_cells * CELL * CELL
    g.shard_pixels = g.slots * g.tile_w * g.tile_h
    g.sig = (g.tiles_w, g.tiles_h, g.tile_w, g.tile_h, w, h)        # what a retained history is bound to, beside the background
    return g


def geo_of(name, world):
    return geometry(*GEOMETRIES[name][0], world)


def owned(geo, rank):
    """Keys of the cells of rank's tiles."""
    return [int(t) * geo.cpt + ci for t in geo.table[rank] if t >= 0 for ci in range(geo.cpt)]


def cell_pixels(geo, key, wrong=None):
    """(pix [32, 32], inside [32, 32]): the linear pixel index of every pixel of cell `key` and whether the scatter kernel writes it."""
    t, ci = divmod(key, geo.cpt)
    ty, tx = divmod(t, geo.tiles_w)
    pxt = (ci % geo.cells_x) * CELL + np.arange(CELL)
    pyt = (ci // geo.cells_x) * CELL + np.arange(CELL)
    stride = geo.w if wrong == "stride-is-width" else geo.stride
    pix = (tx * geo.tile_w + pxt)[None, :] + stride * (ty * geo.tile_h + pyt)[:, None]
    cols = (pxt - pxt % 4 if wrong == "no-quad-guard" else pxt) < geo.tile_w
    rows = np.ones(CELL, bool) if wrong == "no-row-guard" else pyt < geo.tile_h
    inside = rows[:, None] & cols[None, :]
    if wrong == "no-npix-guard":
        pix = pix % geo.npix
    return pix, inside & (pix < geo.npix)


# ---- shards ----
def block(geo, key, seed):
    """The 32 x 32 pixels a shard stores for cell `key`: seeded by (seed, key) alone, so that two shards that store the same cell of
    the same frame store the same pixels; SENT_OUT outside the tile."""
    rng = np.random.default_rng([seed, key])
    b = rng.integers(1, 1 << 24, (CELL, CELL)).astype(np.uint32) | np.uint32(PIXEL_TAG)
    t, ci = divmod(key, geo.cpt)
    if t < geo.tiles:
        x = (ci % geo.cells_x) * CELL + np.arange(CELL)
        y = (ci // geo.cells_x) * CELL + np.arange(CELL)
        b[~((y < geo.tile_h)[:, None] & (x < geo.tile_w)[None, :])] = SENT_OUT
    return b


def cells_of(geo, keys, seed):
    return [(int(k), block(geo, int(k), seed)) for k in keys]


def build_shard(cap, cpt, cells, seed, n=None, header=None):
    """A shard buffer of capacity `cap`.  The first n cells (default: all) are stored, in a seeded shuffle of the slots; cells beyond n
    stay behind them as a reused buffer keeps them -- stale keys and pixels that the header does not cover.  Every other key and pixel
    slot holds SENT_FREE.  header: {word: value} written over the header last."""
    n = len(cells) if n is None else n
    assert n <= len(cells) <= cap
    P = sharding.sparse_pixel_offset(cap)
    sh = np.full(P + cap * CELL * CELL, SENT_FREE, np.uint32)
    sh[:HDR] = (n, cap, cpt, 0)
    order = list(np.random.default_rng(seed).permutation(n)) + list(range(n, len(cells)))
    for slot, k in enumerate(order):
        key, px = cells[k]
        sh[HDR + slot] = key
        sh[P + slot * CELL * CELL: P + (slot + 1) * CELL * CELL] = np.asarray(px, np.uint32).ravel()
    for k, v in (header or {}).items():
        sh[k] = v
    return sh


def prefix(sh, geo, k):
    """The first P + k cells of a shard: what travels when the fullest shard of a batch holds k cells."""
    return sh[:geo.P + k * CELL * CELL]


# ---- the models ----
def full(shards, geo, bg, slots=None, wrong=None, img=None, stamp=None, seq=0):
    """The frame of a full assembly, as a linear pixel array: background over what the tiles cover, 0 behind it, then every stored cell
    of every shard of this job in the order given.  With img: only the cells, into img (the retained assembly's scatter)."""
    if img is None:
        img = np.empty(geo.npix, np.uint32)
        img[:geo.covered] = bg
        img[geo.covered:] = bg if wrong == "tail-is-bg" else 0
    for sh in shards:
        if wrong != "no-header-check" and (int(sh[1]) != geo.max_cells or int(sh[2]) != geo.cpt):
            continue
        n = geo.max_cells if wrong == "slots-beyond-n" else min(int(sh[0]), geo.max_cells)
        if slots is not None and wrong != "n-not-clamped":
            n = min(n, slots)
        for slot in range(n):
            key = int(sh[HDR + slot])
            if key // geo.cpt >= geo.tiles:
                continue
            if stamp is not None and wrong != "no-stamp":
                stamp[key] = seq
            px = sh[geo.P + slot * CELL * CELL: geo.P + (slot + 1) * CELL * CELL].reshape(CELL, CELL)
            pix, inside = cell_pixels(geo, key, wrong)
            img[pix[inside]] = px[inside]
    return img


class Histories:
    """The retained assembly of one context: per frame buffer a stamp per cell of the frame and a sequence number, as
    assembly_background, the scatter kernel and clear_stale_cells keep them.  The caller owns the images; an entry of `images` is what
    the buffer holds.  `evicted` lists the buffers whose history was dropped to make room, in order."""

    def __init__(self, wrong=None):
        self.wrong, self.h, self.images, self.evicted = wrong, {}, {}, []

    def _background(self, buf, geo, bg, retained, batch):
        img = self.images.setdefault(buf, np.full(geo.npix, PREFILL, np.uint32))
        h, incremental = None, False
        if not retained:
            self.h.pop(buf, None)
        else:
            h = self.h.get(buf)
            if h is None:
                if len(self.h) >= MAX_FRAMES:
                    victim = next(b for b in self.h if b not in batch)         # the oldest that is not one of this call's own
                    del self.h[victim]
                    self.evicted.append(victim)
                h = self.h[buf] = SimpleNamespace(sig=None, bg=None, seq=0, stamp=None)
            same_grid = h.sig == geo.sig or (self.wrong == "grid-survives" and h.seq != 0 and len(h.stamp) >= geo.frame_cells)
            incremental = h.seq != 0 and same_grid and (h.bg == bg or self.wrong == "background-survives")
            if not incremental:
                h.stamp, h.sig, h.bg, h.seq = np.zeros(geo.frame_cells, np.uint32), geo.sig, bg, 0
            h.seq += 1
        if not incremental:
            img[:geo.covered] = bg
            img[geo.covered:] = bg if self.wrong == "tail-is-bg" else 0
        return img, h, incremental

    def _clear(self, img, h, geo, bg):
        stale = h.seq if self.wrong == "stale-is-seq" else h.seq - 1
        for key in np.flatnonzero(h.stamp[:geo.frame_cells] == stale):
            pix, inside = cell_pixels(geo, int(key))
            if self.wrong == "clear-not-clipped":
                inside = pix < geo.npix
            img[pix[inside]] = bg

    def assemble(self, buf, shards, geo, bg, retained=True, slots=None, batch=()):
        img, h, incremental = self._background(buf, geo, bg, retained, batch or (buf,))
        full(shards, geo, bg, slots, self.wrong, img, h.stamp if h else None, h.seq if h else 0)
        if incremental:
            self._clear(img, h, geo, bg)
        return img

    def assemble_batch(self, bufs, frames, geo, bg, retained=True, slots=None):
        """One batch call: frames[f] (a list of shards) into bufs[f]."""
        return [self.assemble(b, sh, geo, bg, retained, slots, tuple(bufs)) for b, sh in zip(bufs, frames)]


def compact(gathered, rank_stride, table, geo, prefill=PREFILL, wrong=None):
    """The frame assemble_kernel leaves in a buffer of `prefill`: slot s of rank r, at gathered[r * rank_stride + s * tile pixels], is
    tile table[r, s]; padded slots (-1) are skipped and pixels that no tile covers are left alone."""
    img = np.full(geo.npix, prefill, np.uint32)
    per = geo.tile_w * geo.tile_h
    x, y = np.arange(geo.tile_w), np.arange(geo.tile_h)
    for r in range(table.shape[0]):
        for s in range(table.shape[1]):
            t = int(table[r, s])
            if t < 0:
                if wrong != "padded-is-tile0":
                    continue
                t = 0
            ty, tx = divmod(t, geo.tiles_w)
            stride = geo.w if wrong == "stride-is-width" else geo.stride
            pix = (tx * geo.tile_w + x)[None, :] + stride * (ty * geo.tile_h + y)[:, None]
            src = gathered[r * rank_stride + s * per: r * rank_stride + (s + 1) * per].reshape(geo.tile_h, geo.tile_w)
            if wrong == "no-npix-guard":
                pix = pix % geo.npix
            ok = pix < geo.npix
            img[pix[ok]] = src[ok]
    return img


def has_sentinel(img):
    return bool(np.isin(img, np.array([SENT_FREE, SENT_OUT], np.uint32)).any())


# ---- crafted frames ----
KINDS = ("half", "empty-shard", "whole-tile", "twice", "full", "overfull", "beyond-grid", "cap-off", "cpt-off", "stale-slots")


def half(geo, rank, seed):
    """A seeded half of the cells of rank's tiles, at least one where it owns a tile."""
    own = owned(geo, rank)
    if not own:
        return []
    rng = np.random.default_rng([seed, rank, 77])
    return sorted(int(k) for k in rng.choice(own, max(1, len(own) // 2), replace=False))


def frame_shards(geo, kind, seed):
    """The shards of one crafted frame: every rank stores a seeded half of its cells, and `kind` says what else happens.  Two shards
    that store the same cell store the same pixels (block() depends on the key and the seed alone): different pixels would be a race
    by design.  "twice", "cap-off" and "cpt-off" append one shard to the world's."""
    keys = [half(geo, r, seed) for r in range(geo.world)]
    stored = set(k for ks in keys for k in ks)
    spare = [k for k in range(geo.frame_cells) if k not in stored]          # cells nobody stores: what a bad shard may claim
    cap, cpt = geo.max_cells, geo.cpt
    mk = lambda ks, r, **kw: build_shard(cap, cpt, cells_of(geo, ks, seed), [seed, r], **kw)   # noqa: E731
    first = next(r for r in range(geo.world) if keys[r])                   # a shard that owns a tile
    shards = [mk(ks, r) for r, ks in enumerate(keys)]
    if kind == "half":
        pass
    elif kind == "empty-shard":
        shards[first] = mk([], first)
    elif kind == "whole-tile":
        shards[first] = mk(owned(geo, first)[:cpt], first)
    elif kind == "twice":                                                   # one more shard with cells that others store too
        shards.append(mk(sorted(stored)[:min(3, cap)], geo.world))
    elif kind in ("full", "overfull"):                                      # n = capacity, and a header that claims 5 more
        shards[first] = mk(list(range(cap)), first, header={0: cap + 5} if kind == "overfull" else None)
    elif kind == "beyond-grid":                                             # the first key past the grid and a large one, in stored slots
        ks = keys[first][:max(0, cap - 2)]
        cells = cells_of(geo, ks, seed) + [(geo.frame_cells, block(geo, geo.frame_cells, seed)), (0x7FFFFFF0, block(geo, 0x7FFFFFF0, seed))]
        shards[first] = build_shard(cap, cpt, cells[-cap:], [seed, first])
    elif kind in ("cap-off", "cpt-off"):                                    # not a shard of this job: its cells must not appear
        claim = (spare or sorted(stored))[:cap]
        shards.append(mk(claim, geo.world, header={1: cap + 1} if kind == "cap-off" else {2: cpt + 1}))
    elif kind == "stale-slots":                                             # a reused buffer: valid keys and pixels behind n
        ks = keys[first]
        stale = [k for k in spare if k not in ks][:cap - len(ks)]
        shards[first] = build_shard(cap, cpt, cells_of(geo, ks + stale, seed), [seed, first], n=len(ks))
    else:
        raise KeyError(kind)
    return shards


def fullest(shards):
    return max(int(s[0]) for s in shards)


BATCH_CASES = (("71x45", 3, 1), ("100x64", 2, 3), ("396x396", 3, 3), ("200x136", 8, 3), ("32x32", 1, 64))     # (geometry, world, frames)


def batch_frames(geo, nframes, seed, empty=False):
    """The frames of a batch: "half" frames of different seeds, or frames whose shards are all empty."""
    if empty:
        return [[build_shard(geo.max_cells, geo.cpt, [], [seed, f, r]) for r in range(geo.world)] for f in range(nframes)]
    return [frame_shards(geo, "half", seed + 31 * f) for f in range(nframes)]


def batch_strides(geo, frames):
    """(name, stride in words, slots the model keeps, frames) for a batch: the whole shard, the prefix of the fullest shard, one cell
    less than that (only where a cell is left: a prefix of the header alone keeps all slots), the header alone with empty shards."""
    k = max(fullest(f) for f in frames)
    out = [("whole", geo.words, None, frames), ("fullest", geo.P + k * CELL * CELL, None, frames)]
    if k >= 2:
        out.append(("one-short", geo.P + (k - 1) * CELL * CELL, k - 1, frames))
    out.append(("header", geo.P, None, batch_frames(geo, len(frames), 5, empty=True)))
    return out


def compact_gather(geo, seed, frames=1, frame=0):
    """(gathered, rank stride, offset of the frame): a gather of [rank][frames][shard] of seeded values -- SENT_FREE in padded slots and
    in the other frames --, the frame to assemble being the `frame`-th."""
    sp, per = geo.shard_pixels, geo.tile_w * geo.tile_h
    g = np.full(geo.world * frames * sp, SENT_FREE, np.uint32)
    rng = np.random.default_rng([seed, geo.world])
    for r in range(geo.world):
        for s in range(geo.slots):
            if geo.table[r, s] >= 0:
                o = (r * frames + frame) * sp + s * per
                g[o:o + per] = rng.integers(1, 1 << 24, per).astype(np.uint32) | np.uint32(PIXEL_TAG)
    return g, frames * sp, frame * sp


# ---- retained sequences ----
SEQUENCES = (("128x128", 2), ("71x45", 3), ("396x396", 3), ("100x64", 8))     # (geometry, world)


def sequence(name, world, seed=1):
    """The steps of a retained sequence into one buffer: Step(label, geo, shards, bg, retained).  Every cell is stored by the rank that
    owns its tile; pixels are new in every step."""
    geo = geo_of(name, world)
    owner = {k: r for r in range(world) for k in owned(geo, r)}
    fc = geo.frame_cells
    rng = np.random.default_rng([seed, 5])
    A = sorted(int(k) for k in rng.choice(fc, fc // 2, replace=False))
    B = [k for k in range(fc) if k not in A]
    steps = []

    def step(label, keys, bg="mode8", retained=True, g=geo, own=owner, bad=None):
        s = seed * 1000 + len(steps)
        shards = [build_shard(g.max_cells, g.cpt, cells_of(g, [k for k in keys if own[k] == r], s), [s, r],
                              header={1: g.max_cells - 1} if bad == r else None) for r in range(g.world)]
        steps.append(SimpleNamespace(label=label, geo=g, shards=shards, bg=bg, retained=retained))

    step("all", range(fc))
    step("none", [])                                                        # all go dark
    step("half", A)
    step("same half", A)                                                    # none goes dark
    step("other half", B)
    busiest = max(range(world), key=lambda r: sum(owner[k] == r for k in B))
    step("a header stops matching", B, bad=busiest)                         # that shard's cells go back to background
    step("all again", range(fc))
    if fc > 256:                                                            # the whole last block of the clear kernel, lit and dark
        step("last block", range(256, fc))
        step("last block dark", [])
    wave = list(range(64, 128)) if fc >= 128 else list(range(fc))           # the cells of one wave, then every second one dark
    step("one wave", wave)
    step("every second cell of the wave", wave[::2])
    step("background changes", A, bg="opaque")
    step("other half, new background", B, bg="opaque")
    step("plain assembly", A, bg="opaque", retained=False)                  # ends the history
    step("retained after plain", B, bg="opaque")                            # starts one
    step("dark", [], bg="opaque")
    if name == "128x128":                                                   # another tile grid over the same pixels and cell count
        g2 = geometry(128, 128, 0.5, 0.5, world)
        own2 = {k: r for r in range(world) for k in owned(g2, r)}
        step("first background again", A)
        step("lit before the grid changes", [2, 7])                         # cell 2 lies where cell 4 of the other grid does
        step("another grid", [0, 5, 10], g=g2, own=own2)
        step("half in the other grid", A, g=g2, own=own2)
        step("first grid again", B)
    return steps


def expected(step, slots=None):
    return full(step.shards, step.geo, BG[step.bg], slots)


def lit_keys(step):
    """Keys that the step's assembly stores."""
    g = step.geo
    return {int(k) for sh in step.shards if int(sh[1]) == g.max_cells and int(sh[2]) == g.cpt for k in sh[HDR:HDR + int(sh[0])]}


def alternating(name, world):
    """The same steps through the batch call, two frames a call into two buffers that swap places from call to call: call i assembles
    step i of two sequences of different seeds, [(buffer, step), (buffer, step)]."""
    a, b = sequence(name, world, seed=2), sequence(name, world, seed=3)
    return [((i % 2, sa), (1 - i % 2, sb)) for i, (sa, sb) in enumerate(zip(a, b))]


# ---- more frame buffers than histories ----
def history_frame(geo, buf, rnd):
    """The shard (world 1) of buffer number `buf` in round `rnd`: the lit cell moves from round to round, and in an image of one
    cell it is lit every second round."""
    n = buf + rnd
    keys = [n % geo.frame_cells] if geo.frame_cells > 1 else ([0] if n % 2 == 0 else [])
    return [build_shard(geo.max_cells, geo.cpt, cells_of(geo, keys, 100 * rnd + buf), [buf, rnd])]


def history_ops():
    """The rotation of frame buffers of the histories test: (batch?, [buffer names], round).  A0 .. A63 twice; a 65th buffer; A0
    again; a batch of 64 new buffers; a batch of 32 A and 32 B; the same batch again."""
    A, B = [f"A{i}" for i in range(64)], [f"B{i}" for i in range(64)]
    mix = [x for pair in zip(A[:32], B[:32]) for x in pair]
    return ([(False, [a], 0) for a in A] + [(False, [a], 1) for a in A] + [(False, ["C"], 2), (False, ["A0"], 3), (True, B, 4), (True, mix, 5),
            (True, mix, 6)])


def buffer_number(name):
    return {"A": 0, "B": 64, "C": 128}[name[0]] + int(name[1:] or 0)
