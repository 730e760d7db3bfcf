"""GPU tests of the tile-shard exchange on CUDA tensors: one process and one GPU play every rank.

sharding.SparseFrameGatherer -- what bench.py --gpus N runs for N > 1 -- is built with device="cuda" and the loopback collective of
tests/exchange_scenes.py, which has the stream semantics of the NCCL backend: a call never blocks the host, the output holds poison until
a private comm stream has delivered the data a few milliseconds late, and wait() only makes the caller's current stream wait.  That is the
code the gloo tests (CPU tensors) and the two-rank rehearsal (stage=True) never reach: all_gather_into_tensor and the sent[b] event, the
side stream of start() with work.wait(), the pinned header maximum and record_stream, the pinned read-back of the "gather" exchange's
all-reduce, finish()'s late check on CUDA tensors with its re-gather, and the CUDA-event phase timers.

`world` contexts with set_shard(q, world) render grid_scene(16) at 512 x 512 in 8 x 8 tiles of 64 px (4 cells a tile) with the sparse-frame
entry points bench.py uses (frame_sparse_call; frame_batch_call(..., out_kind=2) on a render stream per buffer that waits for fg.sent[b]):
the shard of the rank under test into fg.shard_frame(b, f), the others' into buffers the loopback reads.  The camera moves every frame.
Every frame rank 0 assembles (scatter_sparse[_batch]_device, retained) must equal the unsharded context's raster frame of the same camera
on all w * h words; regathered, bytes_moved, cells_sent per batch, the hint and the collective log must EQUAL protocol_model(), fed with
the fullest-shard counts read from a reference rendering of the shards.  There are no tolerances in this file.

The last test runs the same sequences through the real torch.distributed module ("nccl", world size 1) in a child process.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exchange_scenes as X

pytestmark = pytest.mark.gpu
W = H = 512
TILES_N = 8
TW = 2.0 / TILES_N
PREFILL = 0x11111111
# (camera offset, focal length) of the growing sequence, one per batch: the lit cells of the fullest shard go 2 -> 48 -> 96 -> 127 of 128
# at world 2, 2 -> 32 -> 64 -> 87 of 88 at world 3 and 1 -> 12 -> 24 -> 32 of 32 at world 8 -- each step outgrows h + h // 4 + 8
LEVELS = ((-12.0, 1.0), (-8.0, 9.0 / 2.2), (-8.0, 9.0 / 1.45), (-8.0, 7.5))


def sequence(name, n, F):
    """(offset, orbit angle, focal length, turned away by) of every frame: no two consecutive frames share a camera."""
    if name == "growing":
        return [LEVELS[min(k // F, len(LEVELS) - 1)][:1] + (0.5 * (k % F) + 0.1 * (k // F),) + LEVELS[min(k // F, len(LEVELS) - 1)][1:] + (0.0,)
                for k in range(n)]
    if name == "full":                       # every cell of the frame lit (world 8: every cell of a shard)
        return [(-8.0, 0.4 * (k % 4) + 0.05 * k, 7.5, 0.0) for k in range(n)]
    return [(-4.0, 3.0 * k, 1.0, 180.0 if name == "dark_first" and k < F else 0.0) for k in range(n)]


def camera(off, rot, focal, away):
    from sgrt_amd import scene
    cam = scene.Camera((0.0, 0.0, off), W, H, -90.0, 0.0, focal)
    cam.orbit(rot)
    cam.turn(np.float32(-90.0) - np.float32(rot) + np.float32(away), 0.0)
    return cam


def pack_of(pkg, bg):
    return pkg.PACK_ROUND | (pkg.ALPHA_COMPUTED if bg == "mode8" else pkg.ALPHA_OPAQUE)


def new_context(pkg, g, cam, rank, world, stream):
    r = pkg.Renderer(0)
    r.set_gaussians(g)
    r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
    r.set_table_step(pkg.TABLE_STEP_DEFAULT)
    r.set_camera_view(W, H, cam.view)
    r.set_shard(rank, world)
    r.tile_gaussians_device(TW, TW, cam.view, stream)
    return r


_reference = {}


def reference_frames(pkg, r, name, n, F, bg):
    """The unsharded context's raster frames [n, w * h] of a sequence, rendered once and left unchanged."""
    key = (name, n, F, bg)
    if key not in _reference:
        from sgrt_amd import scene
        r.set_gaussians(scene.grid_scene(16))
        r.set_options(pkg.EXP_VCL, pkg.ERF_AS, 1e-9)
        r.set_table_step(pkg.TABLE_STEP_DEFAULT)
        r.set_shard(0, 1)
        out = np.zeros((n, W * H), np.uint32)
        for k, c in enumerate(sequence(name, n, F)):
            cam = camera(*c)
            r.set_camera_view(W, H, cam.view)
            r.tile_gaussians(TW, TW, cam.view)
            out[k] = r.render(cam.position, pack_of(pkg, bg), want_radiance=False)[0].reshape(-1)
        assert not (out == X.POISON_PIXEL).any() and not (out == PREFILL).any()
        if name != "dark_first":
            assert all((fr != fr[0]).any() for fr in out), "a frame with nothing in it"
        out.setflags(write=False)
        _reference[key] = out
    return _reference[key]


class Play:
    """One rank's gatherer on CUDA tensors, and the contexts of every rank behind it.

    batch=False: the frame-by-frame callbacks (render / assemble with scatter_sparse_device(..., retained=True)), everything on the current
    stream.  batch=True: the batch callbacks as bench.py writes them -- F contexts a rank, one frame_batch_call per rank and batch on a
    render stream per buffer that waits for fg.sent[b] (and for the peers' send copies, which the loopback takes where a real peer takes
    its own); the buffers share the contexts here, so a render also waits for the one before it; scatter_sparse_batch_device(...,
    retained=True) into one image per frame of the batch.  dist: the real torch.distributed (world 1) instead of a loopback."""

    def __init__(self, pkg, name, nsteps, F, world, NB, bg="mode8", rank=0, exchange="all_gather", stage=False, batch=False, cls=None, dist=None):
        import torch
        from sgrt_amd import scene, sharding
        self.pkg, self.name, self.nsteps, self.F, self.world, self.NB, self.rank, self.batch = pkg, name, nsteps, F, world, NB, rank, batch
        self.exchange, self.stage, self.bg, self.pack = exchange, stage, bg, pack_of(pkg, bg)
        self.cams = [camera(*c) for c in sequence(name, nsteps, F)]
        self.st = torch.cuda.current_stream().cuda_stream
        g = scene.grid_scene(16)
        self.ctx = []
        try:
            for q in range(world):
                self.ctx.append([new_context(pkg, g, self.cams[0], q, world, self.st) for _ in range(F if batch else 1)])
            self.words = self.ctx[0][0].sparse_shard_words()
            self.cap = sharding.sparse_capacity(sharding.shard_table(TILES_N, TILES_N, world), W // TILES_N, H // TILES_N)
            assert sharding.sparse_words(self.cap) == self.words and all(c.sparse_shard_words() == self.words for row in self.ctx for c in row)
            self.counts = self._reference_counts()
            self.nf = X.batches(nsteps, F)
            self.m = X.fullest(self.counts, self.nf)
            self.peer = {q: [torch.zeros(F * self.words, dtype=torch.int32, device="cuda") for _ in range(NB)] for q in range(world) if q != rank}
            self.lb = X.Loopback(rank, world, self._peers) if dist is None else None
            self.fg = (cls or sharding.SparseFrameGatherer)(self.lb if dist is None else dist, rank, world, self.words, self.cap, F, "cuda",
                                                            stage=stage, nbuf=NB, exchange=exchange)
            self.flight = X.Flight(self.fg)
            if self.lb is not None:
                self.lb.buffers = self.fg.shard
            self.images = [torch.full((W * H,), PREFILL, dtype=torch.int32, device="cuda") for _ in range(F if batch else 1)]
            self.rstreams = [torch.cuda.Stream() for _ in range(NB)] if batch else None
            self.peer_sent, self.last_render, self.keep = [None] * NB, None, []
            self.handed, self.final, self.got, self.error = [], [], [], None
            torch.cuda.synchronize()
        except Exception:
            self.close()
            raise

    def close(self):
        import torch
        torch.cuda.synchronize()
        if getattr(self, "lb", None) is not None:
            self.lb.drain()
        for row in self.ctx:
            for c in row:
                c.close()
        self.ctx = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _reference_counts(self):
        """counts[k][q]: the cells rank q's shard of frame k stores, from a rendering of its own (one frame at a time, waited for)."""
        import torch
        buf = torch.zeros(self.words, dtype=torch.int32, device="cuda")
        out = []
        for cam in self.cams:
            row = []
            for q in range(self.world):
                r = self.ctx[q][0]
                r.set_camera_view(W, H, cam.view)
                r.frame_sparse_call(TW, TW, cam.view, cam.position, self.pack)(buf.data_ptr(), self.st)
                hdr = buf[:4].cpu().tolist()
                assert hdr[1:] == [self.cap, 4, 0] and 0 <= hdr[0] <= self.cap, hdr
                row.append(hdr[0])
            out.append(row)
        return out

    def model(self, hint=None):
        return X.protocol_model(self.m, self.nf, self.world, self.cap, self.NB, self.exchange, stage=self.stage, into_tensor=True, hint=hint)

    # -- what the other ranks send: a copy of their prefixes taken now, on the current stream, as their own send copies would be
    def _peers(self, nf, prefix):
        import torch
        b = self.flight.b
        ks = self.flight.frames(b)
        most = max([self.counts[k][q] for k in ks for q in self.peer], default=0)
        if not nf:
            return None, most
        blocks = [self.peer[q][b].view(self.F, self.words)[:nf, :prefix].clone() if q in self.peer else None for q in range(self.world)]
        self.peer_sent[b] = torch.cuda.Event()
        self.peer_sent[b].record()
        return blocks, most

    def _buffer(self, q, b):
        return self.fg.shard[b] if q == self.rank else self.peer[q][b]

    def render(self, b, f):
        cam = self.cams[self.flight.rendering(b, f)]
        for q in range(self.world):
            r = self.ctx[q][0]
            r.set_camera_view(W, H, cam.view)
            call = r.frame_sparse_call(TW, TW, cam.view, cam.position, self.pack)
            self.keep.append(call)
            call(self._buffer(q, b).data_ptr() + 4 * f * self.words, self.st)

    def render_batch(self, b, nf):
        import torch
        fg, rs = self.fg, self.rstreams[b]
        cams = [self.cams[k] for k in self.flight.rendering_batch(b, nf)]
        cams += [cams[-1]] * (self.F - nf)
        for ev in (fg.sent[b], self.peer_sent[b], self.last_render):
            if ev is not None:
                rs.wait_event(ev)
        r0 = fg.mark(rs)
        for q in range(self.world):
            for r, cam in zip(self.ctx[q], cams):
                r.set_camera_view(W, H, cam.view)
            call = self.ctx[q][0].frame_batch_call(self.ctx[q][1:], TW, TW, [c.view for c in cams], [c.position for c in cams], self.pack, out_kind=2)
            self.keep.append(call)
            base = self._buffer(q, b).data_ptr()
            call([base + 4 * f * self.words for f in range(self.F)], rs.cuda_stream, nf)
        fg.note("render", r0, fg.mark(rs))
        done = torch.cuda.Event()
        done.record(rs)
        torch.cuda.current_stream().wait_event(done)
        self.last_render = done

    def assemble(self, b, f):
        fg = self.fg
        self.handed.append(self.flight.frames(b)[f])
        if f == 0:
            self.final.append(fg.cells_sent[b])
        self.ctx[0][0].scatter_sparse_device([t.data_ptr() for t in fg.gathered_shards(b, f)], self.pack, self.images[0].data_ptr(), self.st,
                                             retained=True)
        self.got.append(self.images[0].clone())

    def assemble_batch(self, b, nf):
        fg = self.fg
        self.handed += self.flight.frames(b)[:nf]
        self.final.append(fg.cells_sent[b])
        self.ctx[0][0].scatter_sparse_batch_device([fg.recv[b][q].data_ptr() for q in range(self.world)], fg.prefix[b], nf, self.pack,
                                                   [im.data_ptr() for im in self.images], self.st, retained=True)
        self.got += [self.images[f].clone() for f in range(nf)]

    def run(self):
        """One run of the sequence, waited for; differences() then says what separates it from the model and the reference frames."""
        import torch
        self.flight.count, self.handed, self.final, self.got, self.error = 0, [], [], [], None
        self.hint0, self.moved0, self.again0 = self.fg.cells_hint, self.fg.bytes_moved, self.fg.regathered
        if self.lb is not None:
            self.lb.log = []
        try:
            if self.batch:
                self.fg.run(self.nsteps, None, None, self.render_batch, self.assemble_batch)
            else:
                self.fg.run(self.nsteps, self.render, self.assemble)
        except Exception as e:                  # (a wrong variant may ask for a prefix of 2^31 cells; nothing is launched with it)
            self.error = repr(e)
        torch.cuda.synchronize()
        if self.lb is not None:
            self.lb.drain()
        return self

    def differences(self, want):
        """Nothing, for the gatherer as it should be.  want: the reference frames [nsteps, w * h]."""
        fg, mo, out = self.fg, self.model(self.hint0), []
        if self.error is not None:
            return [("error", self.error)]
        if self.lb is not None and self.lb.log != mo.log:
            out.append(("log", self.lb.log, mo.log))
        if fg.regathered - self.again0 != len(mo.regathered):
            out.append(("regathered", fg.regathered - self.again0, mo.regathered))
        if fg.cells_hint != mo.hint:
            out.append(("hint", fg.cells_hint, mo.hint))
        if not all(fg.sent[b] is not None and fg.sent[b].query() for b in range(min(self.NB, len(self.nf)))):
            out.append(("sent", fg.sent))
        if self.rank != 0:
            if self.handed or fg.bytes_moved:
                out.append(("a rank that assembles nothing", self.handed, fg.bytes_moved))
            return out
        if self.handed != list(range(self.nsteps)):
            out.append(("order", self.handed))
        if self.final != mo.cells_final:
            out.append(("cells_sent", self.final, mo.cells_final))
        if fg.bytes_moved - self.moved0 != mo.bytes_moved:
            out.append(("bytes_moved", fg.bytes_moved - self.moved0, mo.bytes_moved))
        bad = [k for k, im in zip(self.handed, self.got) if not np.array_equal(im.cpu().numpy().view(np.uint32), want[k])]
        if bad:
            out.append(("frames", bad))
        return out


def growing_precondition(p):
    """At least two batches outgrow the margin on what travels -- from the reference shards' headers, before anything is run."""
    late = []
    for i in range(1, len(p.m)):
        h = max(p.m[:max(1, i - p.NB + 1)])
        if p.m[i] > min(p.cap, h + h // 4 + 8):
            late.append(i)
    assert len(late) >= 2 and late == p.model().regathered, (p.m, p.cap, late)


def play_and_check(pkg, renderer, name, nsteps, F, world, NB, **kw):
    want = reference_frames(pkg, renderer, name, nsteps, F, kw.get("bg", "mode8"))
    with Play(pkg, name, nsteps, F, world, NB, **kw) as p:
        if name == "growing" and not p.stage:
            growing_precondition(p)
        if name == "steady":
            assert p.model().regathered == [], p.m
        assert p.run().differences(want) == [], (name, world, NB, kw, p.m)
        return p.model(), p.m, p.cap, list(p.lb.log)


def test_loopback_on_cuda_tensors(pkg):
    """The loopback itself: neither the call nor wait() blocks the host (the comm stream is still busy when both have returned), the
    output holds poison until somebody waits, the data is there for whatever the caller enqueues behind wait(), the filler is bounded."""
    import torch
    send = torch.arange(3 * 40, dtype=torch.int32, device="cuda").reshape(3, 40)
    other = send + 1000
    lb = X.Loopback(0, 2, lambda nf, prefix: ([None, other[:nf, :prefix].clone()], 0))
    for _ in range(2):                                            # (the first call measures the filler's unit)
        out = torch.zeros((2, 3, 40), dtype=torch.int32, device="cuda")
        t0 = time.perf_counter()
        work = lb.all_gather_into_tensor(out, send, async_op=True)
        torch.cuda.current_stream().synchronize()
        early = out.cpu()
        work.wait()
        behind = out.clone()
        busy = not work.done.query()
        lb.comm.synchronize()
        late_ms = (time.perf_counter() - t0) * 1e3
    assert busy and (early[:, :, 0] == X.POISON_COUNT).all() and (early[:, :, 1:] == X.POISON_PIXEL).all()
    assert behind[0].equal(send) and behind[1].equal(other)
    assert late_ms < 100.0, late_ms
    print(f"loopback: data {late_ms:.2f} ms after the call")
    with pytest.raises(RuntimeError):
        work._get_duration()
    most = torch.tensor([7], dtype=torch.int64, device="cuda")
    lb2 = X.Loopback(1, 2, lambda nf, prefix: (None, 41))
    lb2.all_reduce(most, op=lb2.ReduceOp.MAX)
    assert int(most.item()) == 41 and lb2.gather(send, None, dst=0, async_op=True).wait()
    assert lb.log == [("all_gather_into_tensor", (3, 40))] * 2 and lb2.log == [("all_reduce", (1,)), ("gather", (3, 40))]
    lb.drain(), lb2.drain()


@pytest.mark.parametrize("bg", ["mode8", "opaque"])
@pytest.mark.parametrize("NB", [2, 3])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_steady_and_growing_sequences(pkg, renderer, world, NB, bg):
    """Every world with 2 and 3 buffers under both backgrounds: the steady sequence frame by frame, the growing one in batches (and the
    other way round at the other background), 11 and 8 frames in batches of 3 with a ragged last one."""
    by_frame = bg == "mode8"
    mo, m, cap, _ = play_and_check(pkg, renderer, "steady", 8, 3, world, NB, bg=bg, batch=not by_frame)
    assert mo.regathered == []
    mo, m, cap, log = play_and_check(pkg, renderer, "growing", 11, 3, world, NB, bg=bg, batch=by_frame)
    assert len(mo.regathered) >= 2 and [kind for kind, _ in log].count("all_reduce") == 1


@pytest.mark.parametrize("world,NB,name,batch", [(2, 2, "growing", False), (3, 3, "steady", True), (8, 2, "growing", True), (8, 3, "steady", False)])
def test_gather_exchange(pkg, renderer, world, NB, name, batch):
    """exchange="gather": gather to rank 0 and an all-reduce per batch whose result is read back through pinned memory, one batch late."""
    mo, m, cap, log = play_and_check(pkg, renderer, name, 11 if name == "growing" else 8, 3, world, NB, exchange="gather", batch=batch)
    assert [kind for kind, _ in log].count("all_reduce") == len(m)


@pytest.mark.parametrize("world,name", [(2, "growing"), (3, "steady"), (8, "growing")])
def test_the_last_rank_issues_the_same_collectives(pkg, renderer, world, name):
    """The gatherer plays the last rank: its log is the model's, which is rank 0's (a difference is a deadlock), and it assembles nothing.
    Under "gather" as well, where it receives nothing at all."""
    n = 11 if name == "growing" else 8
    for exchange in ("all_gather", "gather"):
        mo0, _, _, log0 = play_and_check(pkg, renderer, name, n, 3, world, 2, exchange=exchange, batch=True)
        mo1, _, _, log1 = play_and_check(pkg, renderer, name, n, 3, world, 2, exchange=exchange, batch=True, rank=world - 1)
        assert log0 == log1 == mo0.log == mo1.log


def test_staged_exchange_on_cuda_tensors(pkg, renderer):
    """stage=True, the rehearsal's path: all-reduce, host read and a host-staged all_gather per batch; nothing is gathered twice."""
    mo, m, cap, log = play_and_check(pkg, renderer, "growing", 11, 3, 2, 2, stage=True)
    assert mo.regathered == [] and mo.cells == [max(m[:i + 1]) for i in range(len(m))]
    assert [kind for kind, _ in log] == ["all_reduce", "all_gather"] * len(m)


def test_first_batch_without_a_lit_cell(pkg, renderer):
    """The camera looks away during the first batch: the hint starts at 0 and the prefix is the header area alone."""
    from sgrt_amd import sharding
    for world, batch in ((3, True), (2, False)):
        mo, m, cap, log = play_and_check(pkg, renderer, "dark_first", 8, 3, world, 2, batch=batch)
        assert m[0] == 0 and min(m[1:]) > 0 and mo.cells[0] == 0 and log[1] == ("all_gather_into_tensor", (3, sharding.sparse_pixel_offset(cap)))


def test_every_cell_of_a_shard_lit(pkg, renderer):
    """World 8, the grid filling the frame: the fullest shard stores every cell it has, the prefix is the whole buffer (cells = cap)."""
    from sgrt_amd import sharding
    for NB, batch in ((3, False), (2, True)):
        mo, m, cap, log = play_and_check(pkg, renderer, "full", 7, 2, 8, NB, batch=batch)
        assert set(m) == {cap} == set(mo.cells) and mo.regathered == []
        assert all(shape[1] == sharding.sparse_words(cap) for kind, shape in log if kind != "all_reduce")


def test_phase_timers(pkg, renderer):
    """fg.timing = True: CUDA events around every phase; the sums are finite and not negative, the frames are the same."""
    for batch in (True, False):
        want = reference_frames(pkg, renderer, "growing", 11, 3, "mode8")
        with Play(pkg, "growing", 11, 3, 3, 3, batch=batch) as p:
            p.fg.timing = True
            assert p.run().differences(want) == []
            ph = p.fg.phase_ms()
            assert ph["frames"] == 11 and ph["batches_gathered_twice"] == len(p.model().regathered) >= 2
            for key in ("render", "gather", "assemble", "host_in_run"):
                assert math.isfinite(ph[key]) and ph[key] >= 0.0, (key, ph)
            assert "gather_nccl" not in ph                           # the loopback's works keep no duration, as the backend's by default
            assert p.fg.phase_ms()["frames"] == 0                    # ... and everything noted is forgotten


def test_two_runs_with_one_gatherer(pkg, renderer):
    """After the first run the hint is known: the second run issues no all-reduce under "all_gather", and its log, counters and frames
    are the model's with that hint."""
    want = reference_frames(pkg, renderer, "steady", 8, 3, "mode8")
    for batch in (False, True):
        with Play(pkg, "steady", 8, 3, 2, 2, batch=batch) as p:
            assert p.run().differences(want) == []
            assert p.lb.log[0] == ("all_reduce", (1,))
            hint = p.fg.cells_hint
            assert p.run().differences(want) == [] and p.hint0 == hint == max(p.m)
            assert p.lb.log == p.model(hint).log and all(kind == "all_gather_into_tensor" for kind, _ in p.lb.log)


@pytest.mark.parametrize("name,exchange", [("finish_without_wait", "all_gather"), ("finish_without_wait", "gather"), ("side_stream_without_wait", "all_gather")])
def test_missing_waits_are_caught(pkg, renderer, monkeypatch, name, exchange):
    """The two variants CUDA tensors alone can show, on the steady sequence (what an assembly may read is there in any case): without
    the wait in finish() the assembly meets the poison -- shards of another geometry, which it does not touch -- and the frames are wrong
    (the first batch under "all_gather", where later batches are saved by the host's wait for the side stream; every batch under
    "gather").  Without work.wait() the side stream is ordered behind nothing, not even behind the loopback's poison on the caller's
    stream: it reads whatever the allocator handed out.  So, for this variant alone, memory is handed out poisoned (torch.empty of a
    receive buffer fills it and waits); the header maximum is then the poison count, and the late check asks for 2^31 cells."""
    import torch
    want = reference_frames(pkg, renderer, "steady", 8, 3, "mode8")
    if name == "side_stream_without_wait":
        empty = torch.empty

        def poisoned_empty(*args, **kw):
            t = empty(*args, **kw)
            if t.is_cuda and t.dtype == torch.int32 and t.dim() == 3:
                X.Loopback._poison(t)
                torch.cuda.current_stream().synchronize()
            return t
        monkeypatch.setattr(torch, "empty", poisoned_empty)
    with Play(pkg, "steady", 8, 3, 2, 2, exchange=exchange, cls=X.variant(name)) as p:
        diff = p.run().differences(want)
        monkeypatch.undo()
        assert diff, name
        print(name, exchange, [d[:2] for d in diff])


# ---- the real backend, world size 1 --------------------------------------------------------------------------------------------------
def child(store_path):
    """Runs in a process of its own: torch.distributed over "nccl" with one rank.  The steady and the growing sequence through the real
    module (Work.wait(), all_gather_into_tensor, _get_duration), both exchanges, batch and frame-by-frame callbacks, the timers once."""
    import torch
    import torch.distributed as dist
    from conftest import load_pkg
    pkg = load_pkg()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", store=dist.FileStore(store_path, 1), rank=0, world_size=1)
    report = []
    try:
        ref = pkg.Renderer(0)
        for name, n, exchange, batch, timing in (("steady", 8, "all_gather", False, False), ("growing", 11, "all_gather", True, True),
                                                 ("growing", 11, "gather", False, False), ("steady", 8, "gather", True, False)):
            want = reference_frames(pkg, ref, name, n, 3, "mode8")
            with Play(pkg, name, n, 3, 1, 2, exchange=exchange, batch=batch, dist=dist) as p:
                if name == "growing":
                    growing_precondition(p)
                p.fg.timing = timing
                diff = p.run().differences(want)
                assert diff == [], (name, exchange, diff)
                ph = p.fg.phase_ms() if timing else {}
                assert all(math.isfinite(v) and v >= 0 for v in ph.values()), ph
                report.append({"sequence": name, "exchange": exchange, "batch": batch, "m": p.m, "gathered_twice": p.model().regathered, "phases": ph})
        ref.close()
    finally:
        dist.destroy_process_group()
    print(json.dumps({"cases": report}))


def test_real_backend_at_world_size_one(tmp_path):
    """torch.distributed itself, as far as one GPU reaches: rendezvous through a file under tmp_path, traffic on the loopback interface."""
    import torch.distributed as dist
    if not dist.is_nccl_available():
        pytest.skip("torch.distributed has no NCCL/RCCL backend")
    env = dict(os.environ, NCCL_SOCKET_IFNAME="lo", TORCH_NCCL_ENABLE_TIMING="1")
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(tmp_path / "rendezvous")], capture_output=True, text=True,
                       timeout=120, env=env, cwd=tmp_path)
    took = time.perf_counter() - t0
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert len(res["cases"]) == 4 and all(len(c["gathered_twice"]) >= 2 for c in res["cases"] if c["sequence"] == "growing")
    print(f"world-size-1 child: {took:.1f} s", res)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child(sys.argv[2])
