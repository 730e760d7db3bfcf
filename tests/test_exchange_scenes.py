"""CPU tests of the tile-shard exchange (sharding.SparseFrameGatherer) through the loopback collective of tests/exchange_scenes.py:
every rank of worlds 1, 2, 3 and 8 is played in turn over the same moving-blob sequences.  Rank 0 must assemble every frame bit for bit,
its counters and every rank's collective log must EQUAL protocol_model(), all ranks' logs must be the same (a difference is a deadlock on
a real backend), and every wrong variant of the gatherer that CPU tensors can show must differ from the model somewhere.

The loopback delivers inside wait() and leaves poison until then, so "forgot to wait" is as deterministic here as a stream race is not.
tests/test_gpu_exchange.py runs the same model against CUDA tensors and shards the kernels render.
"""
import numpy as np
import pytest

import exchange_scenes as X
from exchange_scenes import Case

WORLDS, FS, NBS = (1, 2, 3, 8), (1, 2, 3, 4), (2, 3)


def steps_of(kind, F):
    """Enough batches for the sequence to do what it is named for, the last one ragged wherever a batch has more than one frame."""
    return (5 if kind == "growing" else 4) * F + (F > 1) * (F - 1 if kind == "growing" else 1)


def cases(kinds=X.KINDS, worlds=WORLDS):
    return [Case(world, F, NB, exchange, stage, kind, steps_of(kind, F))
            for kind in kinds for world in worlds for F in FS for NB in NBS for exchange in ("all_gather", "gather") for stage in (False, True)]


def test_the_sequences_are_what_their_names_say(pkg):
    """Before anything is run, on the model alone: "growing" gathers at least two batches twice, "steady" none, "full" travels with the
    whole buffer, "dark_first" starts with the header area alone; a staged exchange never gathers twice."""
    from sgrt_amd import sharding
    for c in cases():
        mo, cap = X.model_of(c), X.geometry(c.world)[1]
        nf = X.batches(c.nsteps, c.F)
        assert nf[-1] < c.F or c.F == 1
        if c.stage:
            assert mo.regathered == []
            continue
        if c.kind == "growing":
            assert len(mo.regathered) >= 2, c
        if c.kind == "steady":
            assert mo.regathered == [], c
        if c.kind == "full":
            assert set(mo.cells) == {cap} and mo.log[1][1][1] == sharding.sparse_words(cap), c
        if c.kind == "dark_first":
            assert mo.cells[0] == 0 and mo.log[1][1][1] == sharding.sparse_pixel_offset(cap), c


def test_model_equals_the_closed_form(pkg):
    """Batch i >= 1 of a new gatherer travels with min(cap, h + h // 4 + 8), h = max(m[:max(1, i - NB + 1)]): the model, which walks
    run()'s order, says the same for any counts."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, NB, cap = int(rng.integers(1, 9)), int(rng.integers(2, 5)), int(rng.integers(1, 200))
        m = [int(x) for x in rng.integers(0, cap + 1, n)]
        for exchange in ("all_gather", "gather"):
            mo = X.protocol_model(m, [2] * n, 3, cap, NB, exchange)
            want = [m[0]] + [min(cap, h + h // 4 + 8) for h in (max(m[:max(1, i - NB + 1)]) for i in range(1, n))]
            assert mo.cells == want and mo.regathered == [i for i in range(1, n) if m[i] > want[i]]
            assert mo.hint == max(m) and len(mo.log) == (n if exchange == "gather" else 1) + n + len(mo.regathered)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_against_the_model(pkg, kind, world):
    """frames_per_gather 1 .. 4 with a ragged last batch, 2 and 3 buffers, both exchanges, staged or not: every rank's log is the
    model's (so all ranks agree), rank 0's frames, regathered, bytes_moved and cells_sent are right, the others assemble nothing."""
    for c in cases((kind,), (world,)):
        mo = X.model_of(c)
        for rank in range(world):
            assert X.differences(X.play(c, rank), mo, rank) == [], (c, rank)


def test_a_second_run_needs_no_all_reduce(pkg):
    """The hint outlives run(): under "all_gather" a second run with the same gatherer starts with a prefix from the hint and issues no
    all-reduce at all.  (play() makes a new gatherer per run, so this one is played by hand.)"""
    import torch
    from sgrt_amd import sharding
    c = Case(3, 2, 2, "all_gather", False, "steady", 7)
    tab, cap, words = X.geometry(c.world)
    shards = X.cpu_shards(c.kind, c.world, c.nsteps, c.F)
    flight = [None]

    def peers(nf, prefix):
        ks = flight[0].frames()
        return ([torch.from_numpy(np.stack([shards[k][q][:prefix] for k in ks[:nf]]).view(np.int32)) if nf else None for q in range(c.world)],
                max(int(shards[k][q][0]) for k in ks for q in (1, 2)))

    lb = X.Loopback(0, c.world, peers)
    fg = sharding.SparseFrameGatherer(lb, 0, c.world, words, cap, c.F, "cpu", nbuf=c.NB)
    fl = flight[0] = X.Flight(fg)
    frames = []
    for rnd in range(2):
        fl.count, lb.log, hint = 0, [], fg.cells_hint

        def render(b, f):
            fg.shard_frame(b, f).copy_(torch.from_numpy(shards[fl.rendering(b, f)][0].view(np.int32).copy()))

        def assemble(b, f):
            parts = [t.numpy().view(np.uint32) for t in fg.gathered_shards(b, f)]
            frames.append(sharding.scatter_sparse(parts, X.TILES_N, X.TILE_W, X.TILE_H, X.H, X.W))
        fg.run(c.nsteps, render, assemble)
        mo = X.model_of(c, hint=hint)
        assert lb.log == mo.log and fg.cells_hint == mo.hint
        assert ("all_reduce", (1,)) in lb.log if rnd == 0 else all(kind == "all_gather" for kind, _ in lb.log)
    assert len(frames) == 2 * c.nsteps
    for k, fr in enumerate(frames):
        np.testing.assert_array_equal(fr, X.frame_image(c.kind, k % c.nsteps, c.F))


@pytest.mark.parametrize("name", [n for n in X.MUTATIONS if n not in X.CUDA_ONLY])
def test_wrong_variants_are_caught(pkg, name):
    """One line of the gatherer replaced: some rank of some case must differ from the model -- a wrong frame, a wrong counter, a log that
    diverges, or an exception.  (The two variants of CUDA-only code are named in exchange_scenes.py; they can be built all the same.)"""
    cls = X.variant(name)
    caught = []
    for c in cases(worlds=(2, 8)):
        if c.F in (1, 3) and c.NB == 2 and not c.stage:
            mo = X.model_of(c)
            caught += [(c, rank) for rank in (0, c.world - 1) if X.differences(X.play(c, rank, cls), mo, rank)]
    assert caught, name
    print(name, "caught in", len(caught), "runs, first", caught[0])


def test_cuda_only_variants_can_be_built(pkg):
    from sgrt_amd import sharding
    for name in X.CUDA_ONLY:
        assert issubclass(X.variant(name), sharding.SparseFrameGatherer)


def test_loopback_poisons_until_waited_for(pkg):
    """The loopback itself: poison at call time, the data inside wait(), the log, a rank that only sends, all_reduce in place."""
    import torch
    send = torch.arange(12, dtype=torch.int32).reshape(2, 6)
    other = send + 100
    lb = X.Loopback(0, 2, lambda nf, prefix: ([None, other[:nf, :prefix]], 41))
    out = torch.zeros((2, 2, 6), dtype=torch.int32)
    work = lb.all_gather(list(out.unbind(0)), send, async_op=True)
    assert (out[:, :, 0] == X.POISON_COUNT).all() and (out[:, :, 1:] == X.POISON_PIXEL).all()
    work.wait()
    assert out[0].equal(send) and out[1].equal(other)
    with pytest.raises(RuntimeError):
        work._get_duration()
    most = torch.tensor([7], dtype=torch.int64)
    lb.all_reduce(most, op=lb.ReduceOp.MAX)
    assert int(most) == 41
    last = X.Loopback(1, 2, lambda nf, prefix: 1 / 0)            # the last rank of a gather receives nothing and asks nobody
    assert last.gather(send, None, dst=0, async_op=True).wait()
    lb.gather(send, list(out.unbind(0)), dst=0)
    assert lb.log == [("all_gather", (2, 6)), ("all_reduce", (1,)), ("gather", (2, 6))] and last.log == [("gather", (2, 6))]
