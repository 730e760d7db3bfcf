"""The tile-shard exchange (sharding.SparseFrameGatherer, what bench.py --gpus N runs for N > 1) played by ONE process: a loopback
collective with the stream semantics of ProcessGroupNCCL, a model of the protocol, and wrong variants of the gatherer.

  Loopback        stands where torch.distributed stands in the gatherer.  The other ranks' contributions come from a callable; the data
                  arrives LATE (CUDA: on a private stream behind a filler of a few milliseconds, once it is waited for; CPU: inside
                  wait()), and until then the output holds poison -- a header count of 0x7FFFFFFF and a pixel no frame holds -- so that
                  a consumer that did not wait, or looked at the headers too early, reads something that cannot be mistaken for a frame.
  protocol_model  what travels with every batch, which batches travel twice, the bytes and the sequence of collectives, from the
                  fullest-shard counts m[i] alone.  It walks run()'s order of start() and finish(); it does not run the class.
  variant(name)   the gatherer with ONE line of one method replaced (the method's source is taken from the class, the line must be
                  there exactly as often as expected: a variant cannot quietly stop being one when sharding.py changes).
  Flight          book-keeping for whoever plays the ranks: which frames are in which buffer, and which buffer the gatherer is talking
                  about when a collective is issued (a re-gather belongs to an older batch than the one just rendered).
  CPU scenes      the moving-blob frames of tests/test_dist_gloo.py on a larger tile grid, and play(): one rank's whole run on CPU
                  tensors.  tests/test_exchange_scenes.py holds them against the model; tests/test_gpu_exchange.py does the same with
                  shards the HIP kernels render, on CUDA tensors.

Two variants change code that only CUDA tensors reach and cannot show on the CPU: "side_stream_without_wait" (CPU tensors have no side
stream: their headers are read in finish(), behind the wait -- the CPU counterpart of that mistake IS "finish_without_wait") and
"sent_never_recorded" (the event exists only for CUDA tensors).  The first is run on the GPU (test_gpu_exchange.py).  The second cannot be
shown from outside the class on the GPU either: before a buffer is rendered into again, finish() has made the host wait for an event that
sits directly in front of the send copy (the all-reduce's read-back) or behind it (the side stream's), so the window is one small copy
wide; the event is what keeps that correct by construction rather than by timing.
"""
import functools
import inspect
import textwrap
from collections import namedtuple

import numpy as np

POISON_COUNT = 0x7FFFFFFF      # header word 0 of everything a collective has not delivered yet
POISON_PIXEL = 0x5EA7DEAD      # every other word of it (the frames of both test files are checked not to hold it)
FILLER_MS = 3.0                # how late the loopback's data is on a GPU


# ---- the loopback collective -------------------------------------------------------------------------------------------------------
class _Work:
    """What an asynchronous collective returns.  CUDA: wait() makes the CALLER'S CURRENT STREAM wait for the comm stream's done-event
    and returns at once; the comm stream's share -- filler, copies, done-event -- is enqueued when wait() is first called (see Loopback).
    CPU: the data is written inside wait().  The tensors stay alive as long as the work does (the loopback keeps every work of a run, as
    the backend's watchdog does until a collective has completed)."""

    def __init__(self, enqueue=None, deliver=None, keep=()):
        self.enqueue, self.deliver, self.keep, self.done, self.waits = enqueue, deliver, keep, None, 0

    def start(self):
        if self.enqueue is not None:
            self.done = self.enqueue()
            self.enqueue = None

    def wait(self):
        self.waits += 1
        if self.enqueue is not None or self.done is not None:
            import torch
            self.start()
            torch.cuda.current_stream().wait_event(self.done)
        elif self.deliver is not None:
            self.deliver()
            self.deliver = None
        return True

    def _get_duration(self):
        raise RuntimeError("getDuration only works if timing was enabled")


class Loopback:
    """The surface SparseFrameGatherer uses of torch.distributed, for rank `rank` of `world`, in one process.

    CUDA tensors: at call time the output is poisoned on the caller's current stream and an event is recorded there; a private comm
    stream waits for that event, runs a bounded filler (FILLER_MS), does the copies and records the done-event.  The comm stream's share
    is enqueued when somebody first calls wait() on the work (or at drain()), not at call time: the HIP runtime runs all streams of a
    process on a handful of hardware queues, and a comm stream that happens to share its queue with the consumer's stream delivers data
    that is late by the clock but never late for that consumer -- a missing wait then shows in one process and not in the next (it did).
    Data that nobody has waited for is a schedule the backend allows, and here it is the only one: what is read without a wait is poison
    whatever the queues do, and the filler keeps the data late for the host even after wait() has returned.

    peers(nf, prefix) -> (blocks, most): blocks[q] is what rank q sends for the batch in flight, an int32 tensor [nf, prefix] that is
    valid on the caller's current stream at call time (a snapshot, as a rank's own send copy is; it is brought to the device of what this
    rank sends -- the host, in a staged exchange; the entry of this rank is ignored); most is the fullest header count among the other
    ranks for that batch.  all_reduce asks peers(0, 0) and uses `most` alone.  log: every collective as (kind, shape of what one rank
    sends).  buffers: tensors the caller writes again while collectives are in flight; what is sent must be a copy of its own."""

    class ReduceOp:
        MAX = "max"

    _unit = None               # (callable that enqueues one filler unit, units per millisecond), measured once per process

    def __init__(self, rank, world, peers, filler_ms=FILLER_MS):
        self.rank, self.world, self.peers, self.filler_ms = rank, world, peers, filler_ms
        self.log, self.works, self.comm = [], [], None
        self.buffers = []          # tensors the caller writes again while a collective is in flight: none of them may be what is sent

    # -- the filler: a bounded amount of GPU work in front of the copies, so that the data is late
    @classmethod
    def _filler_unit(cls):
        if cls._unit is None:
            import torch
            junk = torch.empty(1 << 24, dtype=torch.int32, device="cuda")         # 64 MB: the throw-away copy
            spin = getattr(torch.cuda, "_sleep", None)
            one = (lambda: spin(100000)) if spin is not None else (lambda: junk.copy_(junk.flip(0)))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            one()
            torch.cuda.synchronize()
            a.record()
            for _ in range(4):
                one()
            b.record()
            b.synchronize()
            cls._unit = (one, 4.0 / max(a.elapsed_time(b), 1e-3))
        return cls._unit

    @classmethod
    def fill(cls, ms):
        """Enqueue about `ms` milliseconds of nothing on the current stream."""
        one, per_ms = cls._filler_unit()
        for _ in range(max(1, min(4096, int(round(ms * per_ms))))):
            one()

    def _fill(self):
        self.fill(self.filler_ms)

    @staticmethod
    def _poison(t):
        t.fill_(POISON_PIXEL)
        t[..., 0] = POISON_COUNT

    def _collective(self, kind, send, outs, async_op):
        """outs: {q: tensor that receives rank q's block} -- what THIS rank receives (nothing on a rank that only sends)."""
        import torch
        self.log.append((kind, tuple(send.shape)))
        assert all(send.untyped_storage().data_ptr() != t.untyped_storage().data_ptr() for t in self.buffers), \
            "the rank sends its shard buffer itself, not a copy: the next batch is rendered into what the collective still reads"
        nf, prefix = send.shape
        blocks = self.peers(nf, prefix)[0] if any(q != self.rank for q in outs) else None
        pairs = [(o, send if q == self.rank else blocks[q].to(send.device)) for q, o in sorted(outs.items())]
        for o, s in pairs:
            assert tuple(o.shape) == tuple(s.shape) and o.dtype == s.dtype and o.device == s.device, (kind, o.shape, s.shape)
        if send.is_cuda:
            if self.comm is None:
                self.comm = torch.cuda.Stream()
            for o, _ in pairs:
                self._poison(o)                                   # on the caller's stream, at call time
            ready = torch.cuda.Event()
            ready.record()

            def enqueue():
                with torch.cuda.stream(self.comm):
                    self.comm.wait_event(ready)
                    self._fill()
                    for o, s in pairs:
                        o.copy_(s)
                    done = torch.cuda.Event()
                    done.record()
                return done
            work = _Work(enqueue=enqueue, keep=pairs)
        else:
            for o, _ in pairs:
                self._poison(o)

            def deliver():
                for o, s in pairs:
                    o.copy_(s)
            work = _Work(deliver=deliver, keep=pairs)
        self.works.append(work)
        if async_op:
            return work
        work.wait()
        return None

    def all_gather_into_tensor(self, out, send, async_op=False):
        assert out.shape[0] == self.world
        return self._collective("all_gather_into_tensor", send, {q: out[q] for q in range(self.world)}, async_op)

    def all_gather(self, outs, send, async_op=False):
        assert len(outs) == self.world
        return self._collective("all_gather", send, dict(enumerate(outs)), async_op)

    def gather(self, send, outs, dst=0, async_op=False):
        assert (outs is not None and len(outs) == self.world) if self.rank == dst else outs is None
        return self._collective("gather", send, dict(enumerate(outs)) if self.rank == dst else {}, async_op)

    def all_reduce(self, t, op=None):
        """In place, and synchronous with respect to the calling stream."""
        assert op == self.ReduceOp.MAX and t.numel() == 1
        self.log.append(("all_reduce", tuple(t.shape)))
        t.clamp_(min=int(self.peers(0, 0)[1]))

    def drain(self):
        """Everything the comm stream still holds has run; the works (and the tensors they keep) may go."""
        for work in self.works:
            work.start()
        if self.comm is not None:
            self.comm.synchronize()
        self.works = []


# ---- the protocol, from the counts alone -------------------------------------------------------------------------------------------
Model = namedtuple("Model", "cells regathered cells_final bytes_moved log hint")


def protocol_model(m, nf, world, cap, NB, exchange, stage=False, into_tensor=False, hint=None):
    """m[i]: cells of the fullest shard (any rank, any frame) of batch i; nf[i]: its frames.  run() starts batch i and then finishes
    batch i - (NB - 1), the oldest one in flight; the rest is finished oldest first when the steps are over.

      - without a hint (a new gatherer) batch 0 learns m[0] by all-reduce and travels with exactly that; so does EVERY batch of a staged
        exchange (all-reduce + host read: the hint is the running maximum, nothing is checked late);
      - otherwise a batch travels with min(cap, h + h // 4 + 8), h being the hint when start(i) runs: the largest count of the batches
        finished by then; "gather" still all-reduces every batch (its result is read late), "all_gather" reads the received headers;
      - a checked batch whose m[i] exceeds what travelled is gathered again with exactly m[i], when it is finished.

    hint: the gatherer's cells_hint before the run (a second run with the same gatherer).  into_tensor: CUDA tensors (all_gather is then
    all_gather_into_tensor).  Returns cells (first journey), the batches gathered twice, the cells rank 0 finally holds, rank 0's
    bytes_moved, the collective log and the hint afterwards."""
    from sgrt_amd.sharding import CELL, sparse_pixel_offset
    P = sparse_pixel_offset(cap)
    kind = "gather" if exchange == "gather" else ("all_gather_into_tensor" if into_tensor and not stage else "all_gather")
    log, cells, checked, again, moved, known = [], [], [], [], [0], [hint]

    def travel(i, c):
        prefix = P + c * CELL * CELL
        log.append((kind, (nf[i], prefix)))
        moved[0] += (world - 1) * nf[i] * prefix * 4

    def finish(i):
        if checked[i]:
            known[0] = max(known[0], m[i])
            if m[i] > cells[i]:
                again.append(i)
                travel(i, m[i])

    for i in range(len(m)):
        first = known[0] is None
        if exchange == "gather" or stage or first:
            log.append(("all_reduce", (1,)))
        if first or stage:
            known[0] = max(known[0] or 0, m[i])
            cells.append(known[0])
        else:
            cells.append(min(cap, known[0] + known[0] // 4 + 8))
        checked.append(not (first or stage))
        travel(i, cells[i])
        if i >= NB - 1:
            finish(i - (NB - 1))
    for i in range(max(0, len(m) - (NB - 1)), len(m)):
        finish(i)
    final = [m[i] if i in again else cells[i] for i in range(len(m))]
    return Model(cells, again, final, moved[0], log, known[0])


# ---- wrong variants ------------------------------------------------------------------------------------------------------------------
# name: (method, the text to replace, its replacement, how often the text stands in the method).  The last one is what this suite found in
# the class: .contiguous() of a prefix that is contiguous as it lies (the whole buffer, or any prefix of a single frame) is no copy.
MUTATIONS = {
    "finish_without_wait": ("run", "pending[b].wait()", "pass", 1),
    "side_stream_without_wait": ("start", "work.wait()", "pass", 1),
    "never_gathers_again": ("run", "if most > self.cells_sent[b]:", "if False:", 1),
    "late_check_greater_or_equal": ("run", "if most > self.cells_sent[b]:", "if most >= self.cells_sent[b]:", 1),
    "hint_not_raised": ("run", "self.cells_hint = max(self.cells_hint, most)", "pass", 1),
    "margin_without_8": ("start", "self.cells_hint // 4 + 8", "self.cells_hint // 4", 2),
    "prefix_one_cell_short": ("_gather", "self.P + int(cells) * CELL * CELL", "self.P + max(0, int(cells) - 1) * CELL * CELL", 1),
    "sent_never_recorded": ("_gather", "self.sent[b].record()", "pass", 1),
    "sends_the_buffer_itself": ("_gather", ".clone(memory_format=torch.contiguous_format)", ".contiguous()", 1),
}
CUDA_ONLY = ("side_stream_without_wait", "sent_never_recorded")     # see the module docstring


@functools.lru_cache(maxsize=None)
def variant(name):
    """SparseFrameGatherer with the one replacement MUTATIONS[name] names."""
    from sgrt_amd import sharding
    method, old, new, count = MUTATIONS[name]
    src = textwrap.dedent(inspect.getsource(getattr(sharding.SparseFrameGatherer, method)))
    assert src.count(old) == count, f"{name}: {old!r} stands {src.count(old)} times in {method}(), expected {count}"
    ns = dict(vars(sharding))
    exec(compile(src.replace(old, new), f"<{name}>", "exec"), ns)
    return type("Gatherer_" + name, (sharding.SparseFrameGatherer,), {method: ns[method]})


# ---- who is in which buffer ----------------------------------------------------------------------------------------------------------
class Flight:
    """Counts the frames as they are rendered and remembers which of them each buffer holds; start() and _gather() of the gatherer are
    wrapped (on the instance, calling through to the class's or the variant's method) only to note the buffer they are called for."""

    def __init__(self, fg):
        self.fg, self.count, self.held, self.b = fg, 0, {}, None
        for name in ("start", "_gather"):
            setattr(fg, name, self._noting(getattr(fg, name)))

    def _noting(self, inner):
        def outer(b, *args):
            self.b = b
            return inner(b, *args)
        return outer

    def rendering(self, b, f):
        """render(b, f) is being called: the number of the frame it renders."""
        k = self.count
        self.count += 1
        self.held[b] = [k] if f == 0 else self.held[b] + [k]
        assert len(self.held[b]) == f + 1
        return k

    def rendering_batch(self, b, nf):
        return [self.rendering(b, f) for f in range(nf)]

    def frames(self, b=None):
        """The frames in buffer b (default: the buffer the gatherer is talking about)."""
        return self.held[self.b if b is None else b]


def batches(nsteps, F):
    return [min(F, nsteps - i) for i in range(0, nsteps, F)]


def fullest(counts, nf):
    """m[i] of the model from counts[k][q] (cells stored in rank q's shard of frame k) and the frames per batch."""
    out, k = [], 0
    for n in nf:
        out.append(max(int(c) for row in counts[k:k + n] for c in row))
        k += n
    return out


# ---- CPU scenes: the gloo test's moving blob, 8 x 8 tiles of 80 x 40 pixels (3 x 2 cells a tile, the last column and row partial) ------
TILES_N, TILE_W, TILE_H = 8, 80, 40
H, W = TILES_N * TILE_H, TILES_N * TILE_W
KINDS = ("steady", "growing", "full", "dark_first")
GROWING_RADIUS = (6, 110, 200, 1000)           # per batch: each step outgrows the margin on the prefix until everything is lit


@functools.lru_cache(maxsize=None)
def frame_image(kind, k, F):
    """Frame k of a sequence (F frames a batch): a blob over a zero background; every pixel value carries its place and k.  Read-only."""
    yy, xx = np.mgrid[0:H, 0:W]
    value = np.uint32(0x01000000) + (yy * W + xx + k).astype(np.uint32)
    if kind == "full":
        value.setflags(write=False)
        return value
    if kind == "growing":
        radius = GROWING_RADIUS[min(k // F, len(GROWING_RADIUS) - 1)]
        blob = (yy - (150 + 5 * (k % 3))) ** 2 + (xx - (330 + 7 * (k % 4))) ** 2 < radius ** 2
    else:
        radius = 18 + 3 * (k % 4)
        blob = (yy - (20 + 9 * k) % H) ** 2 + (xx - (30 + 31 * k) % W) ** 2 < radius ** 2
        if kind == "dark_first" and k < F:
            blob = np.zeros_like(blob)
    img = np.where(blob, value, np.uint32(0)).astype(np.uint32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def geometry(world):
    from sgrt_amd import sharding
    tab = sharding.shard_table(TILES_N, TILES_N, world)
    cap = sharding.sparse_capacity(tab, TILE_W, TILE_H)
    return tab, cap, sharding.sparse_words(cap)


@functools.lru_cache(maxsize=None)
def cpu_shards(kind, world, nsteps, F):
    """shards[k][q] (u32 arrays) of every frame and rank, made once and never written."""
    from sgrt_amd import sharding
    tab = geometry(world)[0]
    out = []
    for k in range(nsteps):
        img = frame_image(kind, k, F)
        assert not (img == POISON_PIXEL).any()
        row = [sharding.extract_sparse(img, tab, q, TILES_N, TILE_W, TILE_H) for q in range(world)]
        for sh in row:
            sh.setflags(write=False)
        out.append(row)
    return out


Case = namedtuple("Case", "world F NB exchange stage kind nsteps")
Played = namedtuple("Played", "bad_frames regathered bytes_moved cells_final log hint error")


def model_of(case, hint=None, into_tensor=False):
    nf = batches(case.nsteps, case.F)
    counts = [[int(sh[0]) for sh in row] for row in cpu_shards(case.kind, case.world, case.nsteps, case.F)]
    return protocol_model(fullest(counts, nf), nf, case.world, geometry(case.world)[1], case.NB, case.exchange, stage=case.stage,
                          into_tensor=into_tensor, hint=hint)


def play(case, rank, cls=None):
    """Rank `rank`'s whole run of `case` on CPU tensors through a Loopback.  Rank 0 assembles every frame it is handed with the host
    mirror of the assembly and compares it with the frame that was rendered; an exception ends the run and is part of the result."""
    import torch
    from sgrt_amd import sharding
    world, F = case.world, case.F
    tab, cap, words = geometry(world)
    shards = cpu_shards(case.kind, world, case.nsteps, F)
    others = [q for q in range(world) if q != rank]
    flight = [None]

    def peers(nf, prefix):
        ks = flight[0].frames()
        most = max([int(shards[k][q][0]) for k in ks for q in others], default=0)
        blocks = [None if q == rank or not nf else torch.from_numpy(np.stack([shards[k][q][:prefix] for k in ks[:nf]]).view(np.int32))
                  for q in range(world)]
        return blocks, most

    lb = Loopback(rank, world, peers)
    fg = (cls or sharding.SparseFrameGatherer)(lb, rank, world, words, cap, F, "cpu", stage=case.stage, nbuf=case.NB, exchange=case.exchange)
    fl = flight[0] = Flight(fg)
    lb.buffers = fg.shard
    handed, bad, final = [], [], []

    def render(b, f):
        k = fl.rendering(b, f)
        fg.shard_frame(b, f).copy_(torch.from_numpy(shards[k][rank].view(np.int32).copy()))

    def assemble(b, f):
        k = fl.frames(b)[f]
        handed.append(k)
        if f == 0:
            final.append(fg.cells_sent[b])
        parts = [t.numpy().view(np.uint32) for t in fg.gathered_shards(b, f)]
        # what the assembly may read must be there: a shard that claims more cells than travelled, or poison, is a wrong frame
        sane = all(int(p[1]) == cap and int(p[0]) <= cap and len(p) >= fg.P + int(p[0]) * 1024 for p in parts)
        if not sane or not np.array_equal(sharding.scatter_sparse(parts, TILES_N, TILE_W, TILE_H, H, W), frame_image(case.kind, k, F)):
            bad.append(k)

    error = None
    try:
        fg.run(case.nsteps, render, assemble)
    except Exception as e:                     # (a variant may ask for a prefix of 2^31 cells)
        error = repr(e)
    if rank == 0 and error is None and handed != list(range(case.nsteps)):
        bad.append(("order", tuple(handed)))
    return Played(bad, fg.regathered, fg.bytes_moved, final, lb.log, fg.cells_hint, error)


def differences(played, model, rank):
    """What separates a rank's run from the model: nothing, for the gatherer as it should be."""
    out = []
    if played.error is not None:
        out.append(("error", played.error))
    if played.log != model.log:
        out.append(("log", played.log, model.log))
    if played.regathered != len(model.regathered):
        out.append(("regathered", played.regathered, model.regathered))
    if played.hint != model.hint:
        out.append(("hint", played.hint, model.hint))
    if rank == 0:
        if played.bad_frames:
            out.append(("frames", played.bad_frames))
        if played.bytes_moved != model.bytes_moved:
            out.append(("bytes_moved", played.bytes_moved, model.bytes_moved))
        if played.cells_final != model.cells_final:
            out.append(("cells_sent", played.cells_final, model.cells_final))
    elif played.bytes_moved != 0:
        out.append(("bytes_moved on a rank that assembles nothing", played.bytes_moved))
    return out
