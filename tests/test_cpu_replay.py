"""CPU suite: harness._Replay, the one holder of the capture-and-replay rule, driven with recording stand-ins for
torch.cuda.CUDAGraph, torch.cuda.synchronize and harness.capture (no GPU, no HIP call)."""
import contextlib
import weakref

import pytest
import torch


@pytest.fixture
def rec(monkeypatch):
    """`rec.seen` lists, in order, every launch of `rec.launch`, every call of the three stand-ins and every replay;
    `rec.graphs` holds a weak reference to every fake graph made; `rec.dead_at_enter` says, per capture, whether all
    the graphs made BEFORE the one being captured were already gone when the capture was entered."""
    from gdn_amd import harness

    class Rec:
        seen, graphs, dead_at_enter, value = [], [], [], 0

        def launch(self, *args):
            self.seen.append(("launch",) + args if args else "launch")
            self.value += 1
            return self.value

    rec = Rec()

    class FakeGraph:
        def __init__(self):
            rec.graphs.append(weakref.ref(self))

        def replay(self):
            rec.seen.append("replay")

    @contextlib.contextmanager
    def fake_capture(graph, pool=None):
        rec.dead_at_enter.append(all(ref() is None for ref in rec.graphs if ref() is not graph))
        rec.seen.append("capture-enter")
        yield
        rec.seen.append("capture-exit")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: rec.seen.append("synchronize"))
    monkeypatch.setattr(harness, "capture", fake_capture)
    rec.Replay = harness._Replay
    return rec


FIRST = ["launch", "synchronize", "capture-enter", "launch", "capture-exit"]


def test_without_use_graph_every_call_launches_and_nothing_touches_torch_cuda(rec):
    stale = []
    eager = rec.Replay(rec.launch, False, key=lambda: stale.append("key") or 1, on_stale=lambda: stale.append("stale"))
    assert [eager(), eager(), eager()] == [1, 2, 3]
    assert rec.seen == ["launch"] * 3 and eager.graph is None and rec.graphs == [] and stale == []


def test_the_first_graphed_call_is_the_run_and_later_calls_replay_its_recorded_value(rec):
    held = rec.Replay(rec.launch, True)
    assert held.graph is None
    assert held() == 1                                   # the eager launch's value: that launch is the run
    assert rec.seen == FIRST and held.graph is not None
    del rec.seen[:]
    assert held() == 2 and rec.seen == ["replay"]        # the value the captured call returned
    assert held() == 2 and rec.seen == ["replay"] * 2 and len(rec.graphs) == 1


def test_a_changed_key_releases_the_old_graph_before_the_capture_and_calls_on_stale_once(rec):
    key, stale = [7], []
    held = rec.Replay(rec.launch, True, key=lambda: key[0], on_stale=lambda: stale.append(list(rec.seen)))
    held(), held()
    assert stale == [] and rec.seen == FIRST + ["replay"]            # never at the very first capture
    old = rec.graphs[0]
    assert old() is held.graph
    key[0] = 8
    del rec.seen[:]
    held()
    assert stale == [[]]                                 # once, before anything was launched
    assert rec.seen == FIRST and rec.dead_at_enter == [True, True] and old() is None
    assert held.graph is rec.graphs[1]()
    held()
    assert rec.seen == FIRST + ["replay"] and len(stale) == 1
    # drop(): the key did not change, so the next call captures again without on_stale
    held.drop()
    assert held.graph is None and rec.graphs[1]() is None
    del rec.seen[:]
    held()
    assert rec.seen == FIRST and len(stale) == 1 and rec.dead_at_enter == [True] * 3


def test_args_are_asked_once_per_capture_and_given_to_both_launches(rec):
    asked = []
    held = rec.Replay(rec.launch, True, args=lambda: asked.append(1) or (5, True))
    held(), held(), held()
    assert asked == [1]
    assert rec.seen == [("launch", 5, True), "synchronize", "capture-enter", ("launch", 5, True), "capture-exit",
                        "replay", "replay"]


def test_capture_now_records_no_eager_launch_and_replays_even_without_use_graph(rec):
    held = rec.Replay(rec.launch, False)
    assert held() == 1                                   # eager
    del rec.seen[:]
    held.capture()
    assert rec.seen == ["capture-enter", "launch", "capture-exit"] and held.graph is not None
    assert held() == 2 and rec.seen[3:] == ["replay"]
    held.drop()
    assert held() == 3 and rec.seen[4:] == ["launch"] and held.graph is None


def test_two_holders_with_one_key_callable_go_stale_independently(rec):
    key = [1]
    a, b = (rec.Replay(rec.launch, True, key=lambda: key[0]) for _ in range(2))
    a(), b()
    graph_a, graph_b = a.graph, b.graph
    a.drop()
    assert a.graph is None and b.graph is graph_b
    a()
    assert a.graph is not None and a.graph is not graph_a and b.graph is graph_b
    key[0] = 2
    graph_a = a.graph
    a()                                                  # a has seen the new key; b still holds the old one
    assert a.graph is not graph_a and b.graph is graph_b
    del rec.seen[:]
    a(), b()
    assert rec.seen == ["replay"] + FIRST and b.graph is not graph_b
