"""CPU suite: the host logic of training in gdn_amd.harness — the order in which the captured-step scaffold issues
its halves and hooks, the operand-range pin, and the checkpoint / early-stop rule (no compute calls: no GPU here)."""
import pytest
import torch


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("hooks", [False, True])
def test_captured_step_issues_its_halves_and_hooks_in_order(split, hooks):
    """Eager `_CapturedStep.step()`: pre, forward+backward, [all-reduce, only when split], update, post; then ONE
    invalidate_constants, last; returns `loss`.  `prepare()` of an eager step captures nothing."""
    from gdn_amd import harness
    seen = []

    class Step(harness._CapturedStep):
        def __init__(self):
            super().__init__(False, split, *([lambda: seen.append("pre"), lambda: seen.append("post")] if hooks
                                             else [None, None]))
            self.model = type("M", (), {"invalidate_constants": staticmethod(lambda: seen.append("invalidate"))})()
            self.loss = object()

        def _forward_backward(self):
            seen.append("fb")

        def _all_reduce(self):
            seen.append("all_reduce")

        def _update(self):
            seen.append("update")

    step = Step()
    step.prepare()
    assert step._graphs is None and seen == []
    want = ["pre"] * hooks + ["fb"] + ["all_reduce"] * split + ["update"] + ["post"] * hooks + ["invalidate"]
    for done in (1, 2):
        assert step.step() is step.loss
        assert seen == want * done
    assert step._graphs is None


@pytest.mark.parametrize("before", ["auto", "narrow", "wide"])
@pytest.mark.parametrize("wide", [False, True])
def test_pinned_range_sets_and_restores(before, wide):
    from gdn_amd import GDN, harness
    model = GDN([torch.zeros((2, 1), dtype=torch.long)], 8, dim=16, input_dim=4, topk=3)
    model.operand_range = before
    with harness.pinned_range(model, wide):
        assert model.operand_range == ("wide" if wide else "narrow")
    assert model.operand_range == before
    with pytest.raises(KeyError):
        with harness.pinned_range(model, wide):
            assert model.operand_range == ("wide" if wide else "narrow")
            raise KeyError("inside")
    assert model.operand_range == before


@pytest.mark.parametrize("save_path", ["best.pt", ""])
def test_checkpoint_and_early_stop_rule(save_path, monkeypatch):
    """Validation: save on a STRICTLY better loss, stop at the 15th epoch in a row without one.  No validation: save
    on a better summed training loss, never stop.  An empty save_path saves nothing and decides the same."""
    from gdn_amd import harness
    saved = []
    monkeypatch.setattr(torch, "save", lambda state, path: saved.append((epoch, state, path)))
    model = type("M", (), {"state_dict": staticmethod(lambda: "state")})()

    best, stops = harness._BestSoFar(), []
    for epoch, val in enumerate([3, 2, 2, 1] + [1] * 15):
        stops.append(best.update(val, 100.0 - epoch, model, save_path))     # (the summed loss must not matter)
    assert [e for e, _s, _p in saved] == ([0, 1, 3] if save_path else [])
    assert all(s == "state" and p == save_path for _e, s, p in saved)
    assert stops == [False] * 18 + [True]                # epoch 3 + 15 stale ones
    assert best.min_loss == 1 and best.stale == 15

    saved.clear()
    best, stops = harness._BestSoFar(), []
    for epoch, acc in enumerate([5, 6, 4] + [7] * 20):
        stops.append(best.update(None, acc, model, save_path))
    assert [e for e, _s, _p in saved] == ([0, 2] if save_path else [])
    assert not any(stops) and best.min_loss == 4
