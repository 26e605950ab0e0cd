"""tests/_head_train_ref.py pinned: head_f64 against a float64 nn.BatchNorm1d chain under autograd and against
_grad_check.staged_f64, the kink condition of every case, the dropout draw, and the case tables held to the library's
own byte counts and to the chunk arithmetic of gdn_head_train.hip.  Host only: no GPU, no launch."""
import pytest
import torch

import _head_train_ref as ref
from _grad_check import f64_leaves, staged_f64
from conftest import load_golden, meta
from gdn_amd import _lib

TOL = 1e-12


def close(got, want, what):
    top = float(want.abs().max())
    assert float((got.reshape(want.shape) - want).abs().max()) <= TOL * max(top, 1e-300), (what, top)


def _args(t, form, mask):
    lin = (t["lin_w"], t["lin_b"]) if form == "lin" else (None, None)
    return (t["z"], t["emb"], t["bn1"], t["bn2"], mask, *lin, t["d_out"] if form == "lin" else t["d_act"], t["batch"])


@pytest.mark.parametrize("name,form,masked", [("d16-ragged", "lin", True), ("any-d50", "act", False),
                                              ("edge-columns", "lin", True), ("edge-columns", "act", True)])
def test_head_f64_equals_a_float64_module_chain(name, form, masked):
    """out / act, every gradient, and both BatchNorms' running mean, running variance and counter after the call."""
    t = ref.inputs(ref.BY_ID[name])
    args = _args(t, form, t["mask"] if masked else None)
    got, want = ref.head_f64(*args), ref.torch_chain(*args)
    names = ("out",) + ref.GRADS_LIN if form == "lin" else ("act",) + ref.GRADS_ACT
    for key in names + ref.RUNNING:
        assert bool(torch.isfinite(got[key]).all()), key
        close(got[key], want[key], (name, key))
    assert got["nbt1"] == want["nbt1"] == ref.COUNTER0 + 1 and got["nbt2"] == want["nbt2"] == ref.COUNTER0 + 1
    # the unbiased estimate, at each BatchNorm's own momentum
    rows = t["batch"] * t["n"]
    var1 = t["z"].double().var(0, unbiased=False)
    close(got["rv1"], (1 - ref.BN1_MOM) * t["bn1"]["running_var"].double() + ref.BN1_MOM * var1 * rows / (rows - 1), "rv1")
    if name == "edge-columns":
        # variance 0 behind a live ReLU: gradients flow through inv = 1 / sqrt(eps); xhat = 0, so d_bn1_w is exactly 0;
        # the dead channel and the emb = 0 column give exact zeros where they must
        assert float(t["z"][:, 0].var()) == 0.0 and float(got["y1"][:, 0].min()) > 0.5
        assert float(got["d_z"][:, 0].abs().max()) > 1.0 and float(got["d_emb"][:, 0].abs().max()) > 0.01
        assert float(got["d_bn1_w"][0]) == 0.0 and float(got["rv1"][0]) == (1 - ref.BN1_MOM) * float(t["bn1"]["running_var"][0])
        assert not bool(got["d_z"][:, 1].any()) and not bool(got["d_emb"][:, 1].any()) and not bool(got["d_z"][:, 3].any())
    # the uncancelled scales bound what they stand in for
    for key, s in got["scale"].items():
        assert s.shape == got[key].shape and bool((s >= got[key].abs() * (1 - 1e-12)).all()), key


def test_head_f64_without_running_statistics():
    t = ref.inputs(ref.BY_ID["any-d3"])
    for bn in (t["bn1"], t["bn2"]):
        bn["running_mean"] = bn["running_var"] = None
    args = _args(t, "lin", None)
    got, want = ref.head_f64(*args), ref.torch_chain(*args)
    for key in ("out",) + ref.GRADS_LIN:
        close(got[key], want[key], key)
    assert all(got[key] is None and want[key] is None for key in ref.RUNNING + ("nbt1", "nbt2"))


@pytest.mark.parametrize("case", ["msl_demo_w5_k5", "mlp2_n20_w8_k6"])
def test_head_f64_equals_the_staged_float64_oracle(case):
    """staged_f64's z, mask and the gradient at its `out` (Linear head) / `act` (MLP head) stage, pushed through
    head_f64, give its out / act and its gradient at z, the BatchNorm and Linear parameter gradients."""
    data, p = load_golden(case)
    m = meta(data)
    x, y = torch.from_numpy(data["x"]).double(), torch.from_numpy(data["y"]).double()
    mask, graph = torch.from_numpy(data["dropout_mask"]).double(), torch.from_numpy(data["learned_graph"])
    leaf = f64_leaves(p)
    _loss, st, sg, grads = staged_f64(leaf, x, y, graph, m["out_layer_num"], mask)
    b, n, d = m["b"], m["n"], m["d"]
    from oracle import gdn_oracle
    bns = [dict(weight=leaf[pre + "weight"].detach(), bias=leaf[pre + "bias"].detach(), eps=gdn_oracle.BN_EPS,
                momentum=gdn_oracle.BN_MOMENTUM, running_mean=None) for pre in ("gnn_layers.0.bn.", "bn_outlayer_in.")]
    z, mk = st["z"].reshape(b * n, d), mask.reshape(b * n, d)
    if m["out_layer_num"] == 1:
        d_out = 2.0 * (st["out"] - y).reshape(-1) / (b * n)
        got = ref.head_f64(z, leaf["embedding.weight"], *bns, mk, leaf["out_layer.mlp.0.weight"].detach().view(d),
                           leaf["out_layer.mlp.0.bias"].detach(), d_out, b)
        close(got["out"], st["out"].reshape(-1), "out")
        close(got["d_lin_w"], grads["out_layer.mlp.0.weight"], "d_lin_w")
        close(got["d_lin_b"], grads["out_layer.mlp.0.bias"], "d_lin_b")
    else:
        got = ref.head_f64(z, leaf["embedding.weight"], *bns, mk, None, None, sg["act"].reshape(b * n, d), b)
        close(got["act"], st["act"].reshape(b * n, d), "act")
    close(got["d_z"], sg["z"].reshape(b * n, d), "d_z")
    for tag, pre in (("1", "gnn_layers.0.bn."), ("2", "bn_outlayer_in.")):
        close(got[f"d_bn{tag}_w"], grads[pre + "weight"], pre + "weight")
        close(got[f"d_bn{tag}_b"], grads[pre + "bias"], pre + "bias")


def test_no_case_sits_on_a_kink():
    """A condition on the seeds, not a measurement: at most 1e-4 of a case's elements have a pre-activation inside
    KINK_BAND (every element counted, whether a gradient arrives there or not); cases below 100 000 elements: none."""
    for case in ref.CASES:
        t = ref.inputs(case)
        res = ref.head_f64(*_args(t, "lin", None))
        kinks = int(ref.kink_elements(res["y1"], res["y2"]).sum())
        count = t["z"].numel()
        assert kinks <= 1e-4 * count and (count >= 100000 or kinks == 0), (case["id"], kinks, count)
        assert all(bool(torch.isfinite(v).all()) for v in res.values() if torch.is_tensor(v)), case["id"]
    # `live` narrows the set: a dropped-out element is no kink
    y = torch.tensor([[1e-8, 1.0]], dtype=torch.float64)
    assert ref.kink_elements(y, y + 1).tolist() == [[True, False]]
    assert not bool(ref.kink_elements(y, y + 1, (torch.tensor([[False, True]]), torch.tensor([[True, True]]))).any())


def test_the_draw():
    count = 1 << 20
    for p in (0.2, 0.9):
        keep = ref.mix32_keep(12345, 3, count, p)
        assert keep.dtype == torch.bool and abs(float(keep.double().mean()) - (1.0 - p)) < 3e-3, p
        assert not torch.equal(keep, ref.mix32_keep(12345, 4, count, p))
        assert torch.equal(keep, ref.mix32_keep(12345, 3, count, p))
    assert bool(ref.mix32_keep(7 << 33 | 5, 11, count, 0.0).all())
    # the threshold comes from p as a float32: 0.2f = 0.200000003 (858993472), not 0.2 (858993459)
    assert ref.drop_threshold(0.2) == 858993472 and ref.drop_threshold(0.0) == 0 and ref.drop_threshold(0.5) == 1 << 31
    assert ref.keep_scale(0.2) == 1.25 and ref.keep_scale(0.0) == 1.0


def test_the_case_tables():
    lib = _lib.load()
    ids = [c["id"] for c in ref.CASES]
    assert len(set(ids)) == len(ids) == 17 and set(ref.CORE) <= set(ids)
    for c in ref.CASES:
        b, n, d = c["shape"]
        assert lib.gdn_head_train_stats_bytes(d) > 0 and lib.gdn_head_train_workspace_bytes(n, d) > 0, c["id"]
        assert b * n >= 2 and 1 <= d <= 256
        assert c["family"] == (ref.TILE if d in (16, 32, 64, 128) else ref.ANY), c["id"]
        padded = d if c["family"] == ref.TILE else next(p for p in (16, 32, 64, 128, 256) if d <= p)
        slots = 1024 // padded
        assert c["padded"] == padded and c["chunks"] == (n + slots - 1) // slots, c["id"]
        # the byte count of the workspace is affine in n: what the GPU tests size the sums block by
        per_n = lib.gdn_head_train_workspace_bytes(2, d) - lib.gdn_head_train_workspace_bytes(1, d)
        assert lib.gdn_head_train_workspace_bytes(n, d) - n * per_n == lib.gdn_head_train_workspace_bytes(1, d) - per_n > 0
    by = ref.BY_ID
    assert by["d16-ragged"]["shape"][1] - 64 == 6 and by["d32-one-extra"]["shape"][1] - 32 == 1
    assert by["d32-many-parts"]["shape"][0] > 4 * 64                     # more rounds of 4 windows than 64 parts
    assert by["d64-n700"]["shape"][1] * 64 * 4 > 160 * 1024             # n * d fp32 beyond the LDS
    assert by["any-d3"]["shape"][2] % 4 != 0 and by["any-d129"]["shape"][2] % 4 != 0
    assert by["any-d200-ragged"]["chunks"] == 33 and by["any-d200-ragged"]["shape"][1] - 32 * 4 == 2
    assert {c["padded"] for c in ref.CASES if c["family"] == ref.ANY} == {16, 32, 64, 128, 256}
    assert lib.gdn_head_train_stats_bytes(0) == 0 and lib.gdn_head_train_workspace_bytes(5, 0) == 0
