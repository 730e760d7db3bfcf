"""tests/bundle_state_scenes.py on the CPU: the step generator is deterministic and its committed sequences reach every op, entry
point, way of calling, list source x kernel and stream hand-over that tests/test_gpu_bundle_state.py claims to exercise; the run cannot
hide behind refusals, darkness or steps without a float64 reference; and `run`, driven with a stub that answers every call with a digest
of the state it believes it has, passes the faithful stub and reports every WRONG one.
"""
import zlib

import numpy as np
import pytest

import bundle_state_scenes as BS
from bundle_state_scenes import N_OF


def all_steps():
    for seed, n in BS.CASES:
        yield from BS.walk(seed, n)


# ---- 1. the generator ----
def test_the_generator_is_deterministic():
    for seed, n in BS.CASES:
        assert list(BS.steps(seed, n)) == list(BS.steps(seed, n))
        assert [s for _, s, _, _ in BS.walk(seed, n)] == [s for _, s, _, _ in BS.walk(seed, n)]
    assert list(BS.steps(1, 30)) != list(BS.steps(2, 30))
    assert list(BS.steps(1, 20)) == list(BS.steps(1, 30))[:20]        # a shorter run is the longer one's beginning


def test_every_op_entry_point_and_way_of_calling_occurs():
    ops, calls, hows, setters, why = (set() for _ in range(5))
    for (op, call, how), st, w, _ in all_steps():
        ops.add(op); calls.add(call); hows.add(how); why.add(w)
        if op == "scene":
            setters.add(st.setter)
    assert ops == set(BS.OPS) and calls == set(BS.CALLS) and hows == set(BS.HOWS)
    assert setters == {"host", "device", "side"}
    assert why == {None, "count", "size", "stale", "pair"}                  # every refusal, and calls that are not refused
    assert {c for (_, c, _), _, w, _ in all_steps() if w is None} == set(BS.CALLS)       # ... every entry point also when it is NOT refused
    assert {h for (_, _, h), _, w, _ in all_steps() if w is None} == set(BS.HOWS)
    assert {st.opt[2] for _, st, _, _ in all_steps()} == {1e-9, 0.0, 1e-6}
    for sw in ("index", "sort", "ordered", "stats"):
        assert {getattr(st, sw) for _, st, w, _ in all_steps() if w is None} == {False, True}, sw


def test_every_list_source_meets_every_kernel(oracle):
    seen = set()
    for _, st, why, _ in all_steps():
        if why is None:
            seen |= {(BS.list_source(st), k) for k in BS.kernels_reached(oracle, st)}
    assert seen == {(s, k) for s in ("chunks", "index", "plan") for k in ("short", "long", "scratch")}, sorted(seen)


def test_a_replayed_plan_and_an_atomic_table_with_a_bound_occur():
    run = [(step, st) for step, st, why, _ in all_steps() if why is None]
    assert sum(BS.replayed(st) and st.plan.keep and st.plan.scene != st.scene for _, st in run) >= 3     # frozen lists on a moved scene
    assert sum(BS.replayed(st) and not st.plan.keep for _, st in run) >= 1                               # other rays under a strict plan
    for call in ("grad", "tgrad"):
        assert sum(c == call and not st.ordered and BS.qualifies64(st) for (_, c, _), st in run) >= 2, call
        assert sum(c == call and st.ordered for (_, c, _), st in run) >= 2, call
    assert sum(c == "gn_diag" and st.ordered for (_, c, _), st in run) >= 1
    assert sum(st.sort and st.plan is None and st.bundle.count > 64 for _, st in run) >= 5               # ray_order is compared


def test_the_scene_grows_shrinks_and_grows_again_across_4097():
    for seed, n in BS.CASES:
        sizes = [N_OF[st.scene] for (op, _, _), st, _, _ in BS.walk(seed, n) if op == "scene"]
        big = [i for i, s in enumerate(sizes) if s == 4097]
        if len(big) >= 2 and any(s < 4097 for s in sizes[:big[0]]) and any(s < 4097 for s in sizes[big[0]:big[-1]]):
            return
    pytest.fail("no committed seed grows to 4097, shrinks and grows to 4097 again")


def test_every_stream_takes_over_from_a_bundle_in_flight_on_another():
    """A hand-over that needs the library: a nosync bundle, then -- behind a state change in which the harness waits for nothing (run
    enqueues the next device form BEFORE it waits for the one in flight) -- a device form on another stream.  Refused steps and host
    forms in between do not count: they wait."""
    seen, quiet = set(), 0
    for seed, n in BS.CASES:
        prev = None                                                              # the stream of a nosync bundle still in flight
        for (op, _, how), st, why, turn in BS.walk(seed, n):
            stream = None if (how == "host" or why) else turn % BS.NSTREAMS
            if stream is not None and prev is not None:
                assert stream != prev                                            # the turn moved on: another stream
                seen.add(stream)
                quiet += op in ("none", "bundle") or (op == "scene" and st.setter != "host")     # ... and the library's setter does not wait either
            prev = stream if (how == "nosync" and not why) else None
    print(f"{quiet} hand-overs with no waiting state change in between")
    assert seen == set(range(BS.NSTREAMS)) and quiet >= 3


def test_a_bundle_is_left_in_flight_across_every_kind_of_state_change():
    across = set()
    for seed, n in BS.CASES:
        flying = False
        for (op, _, how), st, why, _ in BS.walk(seed, n):
            if flying:
                across.add(op + (" by " + st.setter if op == "scene" else ""))
            flying = how == "nosync" and not why
    assert across >= {"scene by host", "scene by device", "scene by side", "options", "index", "sort", "ordered", "plan", "plan-keep", "unplan",
                      "frame", "bundle", "none"}, sorted(across)


# ---- 2. the run cannot hide failures ----
def test_refusals_darkness_and_steps_without_a_reference_are_capped(oracle):
    steps = list(all_steps())
    refused = sum(why is not None for _, _, why, _ in steps)
    compared = [st for _, st, why, _ in steps if why is None]
    lit = sum(BS.lit(oracle, st) for st in compared)
    checked = sum(why is None and BS.qualifies64(st) for _, st, why, _ in steps)
    print(f"{len(steps)} steps: {refused} refused, {lit} of {len(compared)} compared calls lit, {checked} with a float64 reference")
    assert 4 * refused <= len(steps)
    assert 4 * lit >= 3 * len(compared)
    assert 3 * checked >= len(steps)


def test_the_twins_are_other_scenes_of_the_same_size(oracle):
    for n in BS.TWINS:
        a, b = BS.scene(oracle, f"cloud-{n}"), BS.scene(oracle, f"cloud-{n}~")
        assert len(a) == len(b) == n and not np.array_equal(a["mu"], b["mu"])
        assert np.abs(a["mu"] - b["mu"]).max() < 0.2 and (b["sigma"] > 0).all()


# ---- 3. run against a stub ----
WRONG = ("options_under_plan", "index_after_device", "order_kept", "counters_kept", "nosync_late", "bitmap_after_shrink", "refusal_writes",
         "refusal_code")


def digest(*what):
    return np.array([zlib.crc32(repr(what).encode())], np.uint64)


class Stub:
    """Answers every call with a digest of the state it BELIEVES it has.  Faithful, the digest of a call is a function of (call, the
    lists' scene, options and rays, the scene, the options, the rays) -- what include/vrt_hip.h says a bundle's bits are a function of.
    wrong (one line each): "options_under_plan" an options change is ignored while a plan is bound; "index_after_device" the index is not
    rebuilt after a device-side scene update; "order_kept" the sorted order of the previous bundle is kept when the ray count did not
    change; "counters_kept" the counters are not cleared before the second of two back-to-back calls; "nosync_late" a bundle in flight
    sees the state at the time it is waited for; "bitmap_after_shrink" a bitmap word stays set when the scene shrinks; "refusal_writes" a
    refused device form has written an output; "refusal_code" it reports another status than VRT_HIP_ERR_INVALID."""

    def __init__(self, wrong=None):
        self.wrong, self.scene, self.opt, self.gen, self.plan = wrong, None, (1, 1, 1e-9), 0, None
        self.sw = {"index": False, "sort": False, "ordered": False, "stats": False}
        self.index_of = self.order_of = self.last = None
        self.bitmap = 0

    def close(self):
        pass

    def set_scene(self, name, how, turn):
        if self.wrong == "bitmap_after_shrink" and self.scene is not None and N_OF[name] < N_OF[self.scene]:
            self.bitmap = max(self.bitmap, N_OF[self.scene])
        if N_OF[name] > self.bitmap:
            self.bitmap = 0                                                        # the bitmap grows: cleared
        if not (self.wrong == "index_after_device" and how != "host" and self.sw["index"]):
            self.index_of = name
        self.scene, self.gen = name, self.gen + 1

    def set_options(self, opt):
        if self.wrong == "options_under_plan" and self.plan is not None:
            return
        self.gen += opt != self.opt
        self.opt = opt

    def set_switch(self, name, on):
        self.sw[name] = bool(on)
        if name == "index" and on:
            self.index_of = self.scene

    def make_plan(self, b, keep):
        self.plan = BS.Plan(keep, self.scene, self.opt, b, self.gen)

    def unplan(self):
        self.plan = None

    def plan_lists(self):
        p = self.plan
        return digest("lists", p.scene, p.opt[0], p.opt[2], p.bundle)

    def frame(self):
        return digest("frame", self.scene, self.opt)

    def _state(self, b):
        return dict(scene=self.scene, opt=self.opt, plan=self.plan, bundle=b, gen=self.gen)

    def _digest(self, call, b, extra=0):
        p = self.plan
        lists = (p.scene, p.opt[0], p.opt[2], p.bundle) if p is not None else (self.index_of if self.sw["index"] else self.scene, self.opt[0], self.opt[2], b)
        stale_order = False
        if p is None and self.sw["sort"] and b.count > 64:
            key = (b, self.scene, self.opt, self.sw["index"])
            if not (self.wrong == "order_kept" and self.order_of is not None and self.order_of[0].count == b.count):
                self.order_of = key
            stale_order = self.order_of != key
        self.last = (call, b)
        return {"digest": digest(call, lists, self.scene, self.opt, b, stale_order, self.bitmap if (self.sw["index"] and p is None) else 0, extra)}

    def _code(self, call, b):
        return BS.INVALID if BS.verdict(BS.State(scene=self.scene, opt=self.opt, plan=self.plan, bundle=b, gen=self.gen), call) else 0

    def host(self, call, b):
        if self._code(call, b):
            raise BS.Refused(call)
        return self._digest(call, b)

    def host_code(self, call, b):
        return self._code(call, b)

    def refused(self, call, b, turn):
        code = self._code(call, b)
        return (-2 if code and self.wrong == "refusal_code" else code), not (code and self.wrong == "refusal_writes")

    def enqueue(self, call, b, turn, reps):
        if self._code(call, b):
            raise BS.Refused(call)
        for rep in range(reps):
            got = self._digest(call, b, rep if self.wrong == "counters_kept" else 0)
        return (call, b) if self.wrong == "nosync_late" else got

    def collect(self, ticket):
        return self._digest(*ticket) if isinstance(ticket, tuple) else ticket

    def stats(self):
        return digest("stats", self.last)

    def records(self):
        return {"records": digest("records", self.last), "mismatches": np.zeros(2, np.uint64)}

    def order(self):
        return digest("order", self.order_of)


def test_the_faithful_stub_passes_every_seed():
    for seed, n in BS.CASES:
        assert BS.run(Stub(), Stub, seed, n) == [], (seed, n)


@pytest.mark.parametrize("wrong", WRONG)
def test_run_reports_every_wrong_stub(wrong):
    found = {seed: BS.run(Stub(wrong), Stub, seed, n) for seed, n in BS.CASES}
    print(wrong, {seed: len(bad) for seed, bad in found.items()})
    assert any(found.values()), wrong


def test_run_prints_one_line_per_step():
    lines = []
    seed, n = BS.CASES[0]
    BS.run(Stub(), Stub, seed, n, out=lines.append)
    assert sum(line.startswith("step ") for line in lines) == n
