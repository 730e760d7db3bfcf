"""The exact dense body (csrc/vrt_dense_block.hpp: dense_shade_block) on its own: the saturation skips, the deal of the emitters
in chunks of six over 4, 8 and 16 waves, the rank sort's tie-break, blocks with lanes that write nothing, every instantiated Exp /
Erf pair, and the same body as the table kernel's fallback.  Scenes, the float64 model of the body's decisions and the derived
bounds: tests/dense_scenes.py; that the scenes can see what they are for: tests/test_dense_scenes.py.

Every frame is rendered with the exact kernels (table step 0), the prune off, cull_eps = 0 and statistics on.  The shape of the
exact launch (VRT_HIP_DENSE_WAVES = 4 | 8 | 16, 17 = 16 waves without the saturation tests) is read when a context is created:
every test makes contexts of its own.  The table kernel's shape is read once per process: its 8-wave fallback runs in ONE child,
    VRT_HIP_TABLE_WAVES=8 VRT_HIP_DENSE_WAVES=8 python tests/test_gpu_dense.py fallback
which prints the frames it rendered; the parent holds them against its own 8-wave context bit for bit.

The counters (vrt_hip_stats.dense_visits_full / _zero / _common) hold one count per (chunk of six emitters, absorber) visit of a
wave: their sum is ceil(cnt / 6) cnt per block whatever the shape -- an identity -- and which class a visit falls in is a property
of the scene that the model brackets.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.join(HERE, "..", "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import dense_scenes as D      # noqa: E402
from dense_scenes import ERF_AS, EXP_VCL   # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120            # python start, the library, two scenes, four frames
NO_TABLE_STEP = 1e-5           # a step no table can meet (test_table_mode_stays_inside_the_tolerance): every block is declined
FALLBACK_LENGTHS = (97, 193)


def channels(img):
    img = np.asarray(img).reshape(-1)
    return ((img[:, None] >> np.array([0, 8, 16, 24], np.uint32)) & 255).astype(np.int32)


def context(pkg, waves, setenv):
    setenv("VRT_HIP_DENSE_WAVES", str(waves))
    return pkg.Renderer(0)


def frame(r, sc, pair=(EXP_VCL, ERF_AS), step=0.0):
    """One frame of the scene: (packed pixels, radiance in float64 -- the same bits --, statistics)."""
    r.set_gaussians(sc.g)
    r.set_plane(sc.w, sc.h, *sc.plane)
    r.tile_gaussians(sc.tw, sc.th, sc.view)
    r.set_options(pair[0], pair[1], 0.0)
    r.set_table_step(step)
    r.set_cull_prune(0.0)
    r.enable_stats(True)
    img, rad = r.render(sc.origin)
    return img.reshape(-1).copy(), rad.reshape(-1, 4).astype(np.float64), r.stats()


def visits(st):
    return st["dense_visits_full"], st["dense_visits_zero"], st["dense_visits_common"]


def against_oracle(sc, img, rad, what, orad=None, extra=0.0, pixels=True):
    """Radiance within the boundary suite's tolerance (plus `extra` per pixel) of the oracle on every pixel, packed pixels within 1."""
    orad = sc.orad if orad is None else orad
    tol = D.tolerance(sc.n, orad.max())
    err = np.abs(rad - orad).max(1)
    print(f"{what}: largest error against the oracle {err.max():.3g} (tolerance {tol:.3g}{'' if np.ndim(extra) == 0 and extra == 0.0 else ' + jump'})", flush=True)
    assert (err <= tol + extra).all(), (what, float(err.max()))
    if pixels:
        assert np.abs(channels(img) - channels(sc.oimg)).max() <= 1, what
    return float(err.max())


def one_whole_block(sc, st, what):
    """The frame is one dense block that starts from the whole scene and keeps it; one count per visit."""
    assert st["dense_blocks"] == 1 and st["overflow_blocks"] == 0, (what, st["dense_blocks"], st["overflow_blocks"])
    assert st["list_entries"] == st["tile_entries"] == sc.n, (what, st["list_entries"], st["tile_entries"])
    assert sum(visits(st)) == D.visit_total([sc.n]), (what, visits(st))


def in_brackets(sc, st, erf, what):
    p = D.plan(sc, D.SAT[erf])
    full, zero, common = visits(st)
    print(f"{what}: visits {p.total} zero {zero} in {p.zero} common {common} in {p.common} full {full}", flush=True)
    assert p.zero[0] <= zero <= p.zero[1], (what, zero, p.zero)
    assert p.common[0] <= common <= p.common[1], (what, common, p.common)


@pytest.mark.parametrize("waves", D.SHAPES)
def test_deal_and_skips_per_shape(pkg, oracle, monkeypatch, waves):
    """Every list length of the deal (all residues mod 6; fewer chunks than waves; the first chunk of a second round of 8 and of 16
    waves; both routes into the kernel, the block kernel's hand-over up to 96 and the dense queue from 97) as one 8x8 block, against
    the oracle with markers on the ranks where the deal could lose or double an emitter.  The statistics: one dense block that holds
    the whole scene, one count per visit; without the saturation tests (17) every visit is `full`, with them `zero` and `common`
    sit in the model's brackets (25 .. 45 % of the visits each: a skip that never fires, or fires where it must not, shows here
    before it shows in the image)."""
    r = context(pkg, waves, monkeypatch.setenv)
    try:
        for n in D.LENGTHS:
            sc = D.scene(oracle, ("stack", n))
            what = f"waves={waves} n={n}"
            img, rad, st = frame(r, sc)
            one_whole_block(sc, st, what)
            if waves == 17:
                assert visits(st)[1:] == (0, 0), (what, visits(st))
            else:
                in_brackets(sc, st, ERF_AS, what)
            against_oracle(sc, img, rad, what)
    finally:
        r.close()


def skip_ratio(sc, rad16, rad17, orad):
    return float((np.abs(rad16 - rad17).max(1) / D.skip_bound(sc, orad)).max())


def test_skipping_changes_nothing_but_the_association(pkg, oracle, monkeypatch):
    """16 waves with the saturation tests against 16 without: a skipped `zero` visit drops fma(A, 0, acc), a skipped `common` one
    moves -2 A_j from each running sum into one of its own.  The bound is derived per pixel from the scene (dense_scenes.skip_bound)."""
    r16, r17 = context(pkg, 16, monkeypatch.setenv), context(pkg, 17, monkeypatch.setenv)
    try:
        worst = 0.0
        for n in D.LENGTHS:
            sc = D.scene(oracle, ("stack", n))
            _, rad16, st16 = frame(r16, sc)
            _, rad17, st17 = frame(r17, sc)
            assert visits(st17)[1:] == (0, 0) and visits(st16)[1] > 0 and visits(st16)[2] > 0
            ratio = skip_ratio(sc, rad16, rad17, sc.orad)
            worst = max(worst, ratio)
            print(f"n={n}: skipping moves a pixel by {np.abs(rad16 - rad17).max():.3g}, {ratio:.3g} of its bound", flush=True)
            assert ratio <= 1.0, (n, ratio)
        print(f"largest ratio to the skip bound: {worst:.3g}", flush=True)
    finally:
        r16.close()
        r17.close()


def test_the_shapes_agree(pkg, oracle, monkeypatch):
    """4, 8 and 16 waves: chunks are aligned multiples of six whatever the shape, so every emitter's term is the same bits and only
    the order in which a ray's non-negative terms are added differs (dense_scenes.shape_bound)."""
    rs = {w: context(pkg, w, monkeypatch.setenv) for w in D.WAVES}
    try:
        worst = 0.0
        for n in D.LENGTHS:
            sc = D.scene(oracle, ("stack", n))
            rads = {w: frame(r, sc)[1] for w, r in rs.items()}
            bound = D.shape_bound(sc, sc.orad)
            for a, b in ((4, 8), (4, 16), (8, 16)):
                ratio = float((np.abs(rads[a] - rads[b]).max(1) / bound).max())
                worst = max(worst, ratio)
                print(f"n={n}: {a} against {b} waves {np.abs(rads[a] - rads[b]).max():.3g}, {ratio:.3g} of its bound", flush=True)
                assert ratio <= 1.0, (n, a, b, ratio)
        print(f"largest ratio to the shape bound: {worst:.3g}", flush=True)
    finally:
        for r in rs.values():
            r.close()


@pytest.mark.parametrize("pair", D.PAIRS, ids=[f"{D.EXP_NAMES[e]}-{D.ERF_NAMES[f]}" for e, f in D.PAIRS])
def test_every_exp_erf_pair(pkg, oracle, monkeypatch, pair):
    """The nine instantiated pairs, SAT = 5.5 / 4.2 / 3.1 / 2.9 / 2.0 by the Erf: with against without the saturation tests inside
    the skip bound (the terms that are not skipped are the same bits on both sides, so the jumps of spline_erf_mirror at 0 and of
    taylor_erf at +-2 cancel), `zero` and `common` in the brackets of that SAT, and the frame against the oracle rendered with the
    same pair -- the two discontinuous Erfs with one jump on top, jump x max_j A_j x L per pixel: a sample within float noise of the
    jump (an emitter's own centre sample sits on the mirror's) may fall on either side."""
    r16, r17 = context(pkg, 16, monkeypatch.setenv), context(pkg, 17, monkeypatch.setenv)
    name = f"{D.EXP_NAMES[pair[0]]}-{D.ERF_NAMES[pair[1]]}"
    try:
        for n in D.PAIR_LENGTHS:
            sc = D.scene(oracle, ("stack", n))
            what = f"{name} n={n}"
            orad = D.oracle_pair(oracle, sc, *pair)
            img16, rad16, st16 = frame(r16, sc, pair)
            _, rad17, st17 = frame(r17, sc, pair)
            one_whole_block(sc, st16, what)
            one_whole_block(sc, st17, what)
            assert visits(st17)[1:] == (0, 0)
            in_brackets(sc, st16, pair[1], what)
            ratio = skip_ratio(sc, rad16, rad17, orad)
            print(f"{what}: skipping moves a pixel by {np.abs(rad16 - rad17).max():.3g}, {ratio:.3g} of its bound", flush=True)
            assert ratio <= 1.0, (what, ratio)
            extra = D.ERF_JUMP.get(pair[1], 0.0) * D.geometry(sc).A.max(1)[sc.pixels] * orad.max(1)
            for rad, tag in ((rad16, "16"), (rad17, "17")):
                against_oracle(sc, img16, rad, f"{what} waves={tag}", orad=orad, extra=extra, pixels=False)
    finally:
        r16.close()
        r17.close()


@pytest.mark.parametrize("waves", D.WAVES)
def test_tied_keys(pkg, oracle, monkeypatch, waves):
    """Bit-equal keys: groups of 2, 3 and 7 copies of a centre, and 30 Gaussians at one centre.  A tie-break that gave two
    candidates one rank would leave a row of LDS unwritten -- it then holds a Gaussian of the stack of 193 rendered just before --
    and lose a Gaussian: every pixel against the oracle, and the counters (the model ranks ties by list position, as the kernel)."""
    r = context(pkg, waves, monkeypatch.setenv)
    try:
        for same_depth in (False, True):
            frame(r, D.scene(oracle, ("stack", 193)))
            sc = D.scene(oracle, ("ties", same_depth))
            what = f"waves={waves} ties{' at one centre' if same_depth else ''} n={sc.n}"
            img, rad, st = frame(r, sc)
            one_whole_block(sc, st, what)
            in_brackets(sc, st, ERF_AS, what)
            against_oracle(sc, img, rad, what)
    finally:
        r.close()


@pytest.mark.parametrize("waves", (16, 8))
@pytest.mark.parametrize("name", list(D.RAGGED))
def test_ragged_blocks(pkg, oracle, monkeypatch, name, waves):
    """Blocks with lanes that write nothing (beyond the tile's right and bottom edge: they shade the clamped pixel and take part in
    every wave-wide decision), down to a block of 2x2 pixels: every pixel against the oracle.  Every block that holds a pixel is
    shaded, by the dense body; its candidates are at least what one of its rays keeps and at most the scene."""
    sc = D.scene(oracle, ("ragged", name))
    blocks = D.blocks_of(sc)
    seen = D.seen(sc)
    r = context(pkg, waves, monkeypatch.setenv)
    try:
        what = f"waves={waves} {name}"
        img, rad, st = frame(r, sc)
        print(what, {k: st[k] for k in ("shaded_blocks", "dense_blocks", "overflow_blocks", "tile_entries", "list_entries")}, visits(st), flush=True)
        assert st["shaded_blocks"] == st["dense_blocks"] == len(blocks) and st["overflow_blocks"] == 0
        assert st["tile_entries"] == sc.n * len(blocks)
        assert sum(int(seen[pix].any(0).sum()) for pix, _ in blocks) <= st["list_entries"] <= sc.n * len(blocks)
        if st["list_entries"] == sc.n * len(blocks):
            assert sum(visits(st)) == D.visit_total([sc.n] * len(blocks))
        against_oracle(sc, img, rad, what)
    finally:
        r.close()


# ---- the fallback inside the table kernel ----
def fallback_frames(r, oracle, out=print):
    """On the context `r`: the exact launch and, at a step no table can meet, the table kernel's fallback -- the same body over the
    table kernel's waves.  One declined block, one count per visit, radiance and pixels bit for bit.  {n: the exact radiance}."""
    rads = {}
    for n in FALLBACK_LENGTHS:
        sc = D.scene(oracle, ("stack", n))
        img0, rad0, st0 = frame(r, sc)
        img1, rad1, st1 = frame(r, sc, step=NO_TABLE_STEP)
        assert st0["table_declined"] == 0 and st0["table_blocks"] == 0 and st0["dense_blocks"] == 1
        assert st1["table_declined"] == st1["dense_blocks"] == 1 and st1["table_blocks"] == 0, (n, st1["table_declined"], st1["dense_blocks"])
        one_whole_block(sc, st0, f"exact n={n}")
        one_whole_block(sc, st1, f"fallback n={n}")
        assert visits(st1) == visits(st0), (n, visits(st1), visits(st0))
        equal = bool((rad1 == rad0).all() and (img1 == img0).all())
        out(f"n={n}: fallback against the exact launch {np.abs(rad1 - rad0).max():.3g}, bit-equal {equal}")
        assert equal, n
        rads[n] = rad0
    return rads


def test_the_table_kernels_fallback_is_the_same_arithmetic(pkg, oracle, monkeypatch):
    """Frames of this size take the table kernel's 16-wave shape: its fallback and the exact launch of a 16-wave context give the
    same bits.  The 8-wave shape of both, in one child process: the same there, and the child's frames are the bits of this
    process's own 8-wave exact launch (so the child did run 8 waves: the 16-wave frames differ from them)."""
    assert "VRT_HIP_TABLE_WAVES" not in os.environ      # read once per process
    r16, r8 = context(pkg, 16, monkeypatch.setenv), context(pkg, 8, monkeypatch.setenv)
    try:
        rads16 = fallback_frames(r16, oracle, out=lambda s: print("16 waves", s, flush=True))
        rads8 = {n: frame(r8, D.scene(oracle, ("stack", n)))[1] for n in FALLBACK_LENGTHS}
    finally:
        r16.close()
        r8.close()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "fallback"], timeout=CHILD_TIMEOUT, capture_output=True, text=True,
                           env={**os.environ, "VRT_HIP_TABLE_WAVES": "8", "VRT_HIP_DENSE_WAVES": "8"})
    lines = child.stdout.splitlines()
    print("\n".join(ln for ln in lines if not ln.startswith("rad ")), child.stderr, sep="\n", flush=True)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    sent = {int(ln.split()[1]): ln.split()[2] for ln in lines if ln.startswith("rad ")}
    assert sorted(sent) == sorted(FALLBACK_LENGTHS)
    for n in FALLBACK_LENGTHS:
        assert sent[n] == rads8[n].astype(np.float32).tobytes().hex(), n
        print(f"n={n}: 8 against 16 waves {np.abs(rads8[n] - rads16[n]).max():.3g}", flush=True)
    assert any((rads8[n] != rads16[n]).any() for n in FALLBACK_LENGTHS)


if __name__ == "__main__":
    import oracle as O
    from table_cases import load_pkg
    assert sys.argv[1:] == ["fallback"] and os.environ.get("VRT_HIP_TABLE_WAVES") == os.environ.get("VRT_HIP_DENSE_WAVES") == "8"
    O.build()
    ctx = load_pkg().Renderer(0)
    try:
        for length, radiance in fallback_frames(ctx, O, out=lambda s: print("8 waves", s, flush=True)).items():
            print("rad", length, radiance.astype(np.float32).tobytes().hex(), flush=True)
    finally:
        ctx.close()
