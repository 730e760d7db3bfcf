"""Host-frame delivery, word by word (csrc/vrt_host_frame.hip: host_frame_kernel, deliver_cell; csrc/vrt_hip_host_frame.cpp:
vrt_hip_host_register, vrt_hip_frame_host, vrt_hip_host_unregister) against the model of tests/host_frame_scenes.py, on its crafted
cases: small geometries, scenes whose lit cells are known, sequences that walk through every rule of "full or delta".

One harness runs every delivery of every case.  Before a delivery the WHOLE registered buffer is overwritten with a poison word that no
frame holds; after the delivery and a sync the buffer must equal where(written, fresh render, poison) on every word, exactly.  That
pins the mode (a full copy leaves no poison in the image), that nothing is written that the rules leave alone (poison survives there,
beyond w * h too) and that nothing is left out.  `written` is the model's; the fresh render is vrt_hip_render of the same scene and
pose on the session's context.  The lit set that the model is given is the scene's own; once per scene it is held against the cell
keys that vrt_hip_frame_sparse_device stores on another context, and against the pixels of the fresh render.
"""
import numpy as np
import pytest

import host_frame_scenes as H
from assembly_scenes import HDR

pytestmark = pytest.mark.gpu

_cams, _wants, _keys = {}, {}, {}


def camera(geo):
    """(view, position) of scene.cli_camera(w, h): the pose of every frame here."""
    if (geo.w, geo.h) not in _cams:
        from sgrt_amd import scene
        cam = scene.cli_camera(geo.w, geo.h)[0]
        _cams[(geo.w, geo.h)] = (cam.view.copy(), cam.position.copy())
    return _cams[(geo.w, geo.h)]


def pack_of(pkg, geo):
    return pkg.PACK_ROUND | (pkg.ALPHA_COMPUTED if geo.bg == "mode8" else pkg.ALPHA_OPAQUE)


def want_of(pkg, renderer, geo, sc):
    """A fresh vrt_hip_render of the scene at the geometry, w * h words: made once, never changed."""
    key = (geo.name, geo.bg, sc.what)
    if key not in _wants:
        view, pos = camera(geo)
        renderer.set_gaussians(sc.g)
        renderer.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        renderer.set_camera_view(geo.w, geo.h, view)
        renderer.tile_gaussians(geo.tw, geo.th, view)
        img = renderer.render(pos, pack_of(pkg, geo), want_radiance=False)[0].reshape(-1).copy()
        assert not (img == H.POISON).any(), f"{key}: the frame holds the poison word"
        img.setflags(write=False)
        _wants[key] = img
    return _wants[key]


@pytest.fixture(scope="module")
def keys_context(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def check_lit_set(pkg, keys_context, geo, sc, want):
    """Once per (geometry, scene): the scene's lit set is the set of cell keys a sparse frame of it stores, and no cell outside it holds
    a pixel that is not background."""
    key = (geo.name, sc.what)
    if key not in _keys:
        import torch
        r, st = keys_context, torch.cuda.current_stream().cuda_stream
        view, pos = camera(geo)
        r.set_gaussians(sc.g)
        r.set_camera_view(geo.w, geo.h, view)
        r.set_shard(0, 1)
        r.tile_gaussians_device(geo.tw, geo.th, view, st)
        words = r.sparse_shard_words()
        buf = torch.full((words,), -1, dtype=torch.int32, device="cuda")
        r.frame_sparse_call(geo.tw, geo.th, view, pos, pack_of(pkg, geo))(buf.data_ptr(), st)
        torch.cuda.synchronize()
        sh = buf.cpu().numpy().view(np.uint32)
        assert int(sh[2]) == geo.cpt and int(sh[0]) <= int(sh[1]), (key, sh[:4])
        _keys[key] = frozenset(int(k) for k in sh[HDR:HDR + int(sh[0])])
    assert _keys[key] == sc.lit, f"{key}: the scene names {sorted(sc.lit)}, the list kernel lit {sorted(_keys[key])}"
    owner = H.cell_of_word(geo)[:geo.npix]
    shows = set(np.unique(owner[(want != geo.background) & (owner >= 0)]).tolist())
    assert shows <= set(sc.lit), f"{key}: cells {sorted(shows - set(sc.lit))} hold pixels and are not lit"


def describe(geo, got, expect, written):
    """The first few cells with a wrong word, and what is wrong there."""
    bad = np.flatnonzero(got != expect)
    owner = H.cell_of_word(geo)
    mask = np.zeros(geo.pixels, bool)
    mask[written] = True
    out = []
    for k in list(dict.fromkeys(owner[bad].tolist()))[:4]:
        i = int(bad[owner[bad] == k][0])
        where = {-1: "words no tile covers", -2: "words beyond w*h"}.get(k, f"cell {k}")
        what = ("left alone, must be written" if got[i] == H.POISON else "wrong pixel") if mask[i] else "written, must be left alone"
        out.append(f"{where}: word {i} = {int(got[i]):#010x}, want {int(expect[i]):#010x} ({what}; {int((owner[bad] == k).sum())} words)")
    return f"{len(bad)} wrong words; " + "; ".join(out)


def set_scene(r, state, sc):
    if state.get("scene") is not sc:
        r.set_gaussians(sc.g)
        state["scene"] = sc


def play(pkg, renderer, keys_context, name, synced=True):
    """Every step of the case on a context of its own.  synced: poison, deliver, sync, compare, step by step; otherwise everything is
    enqueued and only the final frames are compared."""
    case = H.CASES[name]
    r = pkg.Renderer(0)
    bufs = {b: pkg.host_frame(n, 1).reshape(-1) for b, n in case.buffers.items()}
    for b in bufs.values():
        b[:] = H.POISON
    state = {}
    try:
        for i, (s, e) in enumerate(zip(case.steps, H.run(case))):
            if s.op == "register":
                if s.refused:
                    with pytest.raises(pkg.VrtHipError, match="at most 16 host buffers"):
                        r.register_host(bufs[s.buf])
                else:
                    r.register_host(bufs[s.buf])
                continue
            if s.op == "unregister":
                r.unregister_host(bufs[s.buf])
                continue
            geo = e.geo if e else H.geometry(s.geo, s.bg)
            sc = e.scene if e else H.scene_of(geo, s.what)
            view, pos = camera(geo)
            set_scene(r, state, sc)
            if s.op == "frame":
                r.set_camera_view(geo.w, geo.h, view)
                r.frame(geo.tw, geo.th, view, pos, pack_of(pkg, geo), want_image=False, wait=False)
                continue
            if s.op == "render":
                r.set_camera_view(geo.w, geo.h, view)
                r.tile_gaussians(geo.tw, geo.th, view)
                r.render(pos, pack_of(pkg, geo), want_radiance=False)
                continue
            buf = bufs[s.buf]
            if s.set_view:
                r.set_camera_view(geo.w, geo.h, view)
            if not synced:
                r.frame_host(geo.tw, geo.th, view, pos, pack_of(pkg, geo), buf)
                continue
            want = want_of(pkg, renderer, geo, sc)
            check_lit_set(pkg, keys_context, geo, sc, want)
            buf[:] = H.POISON
            r.frame_host(geo.tw, geo.th, view, pos, pack_of(pkg, geo), buf)
            r.sync()
            got = buf.copy()
            expect = np.full(geo.pixels, H.POISON, np.uint32)
            expect[e.written] = want[e.written]
            if not np.array_equal(got, expect):
                seen = "delta" if (got[:geo.npix] == H.POISON).any() else "full"
                pytest.fail(f"case {name}, step {i} (buffer {s.buf}, {geo.name} {geo.bg}, scene {sc.what}): expected a {e.mode} delivery of "
                            f"{len(e.written)} words, saw a {seen} one of {int((got != H.POISON).sum())}: {describe(geo, got, expect, e.written)}")
        if not synced:
            r.sync()
            for b, (geo, sc) in H.final_frames(case).items():
                np.testing.assert_array_equal(bufs[b][:geo.npix], want_of(pkg, renderer, geo, sc), err_msg=f"case {name}, buffer {b}: final frame")
    finally:
        r.close()


@pytest.mark.parametrize("name", [n for n in H.CASES if n != "no-retain"])
def test_every_delivery_writes_the_words_of_the_model(pkg, renderer, keys_context, name):
    play(pkg, renderer, keys_context, name)


def test_without_retained_stamps_every_delivery_is_full(pkg, renderer, keys_context, monkeypatch):
    """VRT_HIP_RETAIN_FRAME=0 is read when the context is created."""
    real = pkg.Renderer

    def made_without_retention(*a, **kw):
        monkeypatch.setenv("VRT_HIP_RETAIN_FRAME", "0")
        try:
            return real(*a, **kw)
        finally:
            monkeypatch.delenv("VRT_HIP_RETAIN_FRAME")

    assert not H.CASES["no-retain"].retain
    monkeypatch.setattr(pkg, "Renderer", made_without_retention)
    play(pkg, renderer, keys_context, "no-retain")


def test_two_buffers_enqueued_without_a_sync(pkg, renderer, keys_context):
    """The two-buffer case with nothing waited for between deliveries: which deliveries are full is then a matter of timing (the count
    a delivery reads lags by what is in flight), the pixels are not.  Only the final frames are compared."""
    play(pkg, renderer, keys_context, H.UNSYNCED, synced=False)
