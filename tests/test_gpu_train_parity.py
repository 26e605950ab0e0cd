"""GPU suite: one training step (train.py:68-72 usage) — HIP forward + HIP backward of the graph
layer and of the train-mode head (torch only for the dropout draw and the out_layer_num > 1 MLP) — against
the gradients the reference produced, the reference's loss curves, and the float64 oracle."""
import numpy as np
import pytest
import torch

from _head_train_ref import mix32_keep as _mix32_mask   # the in-kernel dropout draw: (seed, step, count, p, device)
from conftest import MODEL_CASES, load_golden, meta
from test_gpu_forward_parity import build_model

pytestmark = pytest.mark.gpu


class FixedMaskDropout(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = list(masks), 0

    def forward(self, x):
        if not self.training:
            return x
        m = self.masks[self.calls]
        self.calls += 1
        return x * m


@pytest.mark.parametrize("case", MODEL_CASES)
def test_train_step_matches_reference_grads(case, gpu_device):
    data, p = load_golden(case)
    m = meta(data)
    model = build_model(p, m, gpu_device)
    model.injected_graph = torch.from_numpy(data["learned_graph"]).to(gpu_device)
    model.dp = FixedMaskDropout([torch.from_numpy(data["dropout_mask"]).to(gpu_device)])
    model.train()
    model.zero_grad()
    x = torch.from_numpy(data["x"]).to(gpu_device)
    y = torch.from_numpy(data["y"]).to(gpu_device)
    out = model(x, None)
    loss = torch.nn.functional.mse_loss(out, y, reduction="mean")       # train.py:20-23
    loss.backward()
    # train-mode BatchNorm normalises by the statistics of as few as B*N = 50..254 rows, which
    # amplifies fp32 association differences ~1/sigma: 5e-5 here (north_star bar: 1e-4)
    np.testing.assert_allclose(out.detach().cpu().numpy(), data["train_out"], atol=5e-5, rtol=0)
    np.testing.assert_allclose(loss.item(), float(data["train_loss"]), atol=5e-5, rtol=0)
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        np.testing.assert_allclose(prm.grad.cpu().numpy(), data["g/" + name], atol=5e-5, rtol=1e-3,
                                   err_msg=name)
    for key, val in model.state_dict().items():
        if "running" in key or "num_batches" in key:
            np.testing.assert_allclose(val.cpu().numpy(), data["p_after_train_fwd/" + key], atol=2e-5,
                                       rtol=0, err_msg=key)


def test_two_adam_steps_match_reference_train_loop(gpu_device):
    """the reference's train() for 1 epoch x 2 batches (Adam lr 1e-3)."""
    data, p = load_golden("train_loop_2step")
    m = meta(data)
    model = build_model(p, m, gpu_device)
    masks = [torch.from_numpy(mk).to(gpu_device) for mk in data["masks"]]
    model.dp = FixedMaskDropout(masks)
    opt = torch.optim.Adam(model.parameters(), lr=0.001, weight_decay=0.0)   # train.py:31
    model.train()
    losses = []
    x = torch.from_numpy(data["x"]).to(gpu_device)
    y = torch.from_numpy(data["y"]).to(gpu_device)
    for s in range(0, x.shape[0], m["b"]):
        opt.zero_grad()
        out = model(x[s:s + m["b"]], None)
        loss = torch.nn.functional.mse_loss(out, y[s:s + m["b"]], reduction="mean")
        loss.backward()
        opt.step()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, data["losses"], atol=2e-5, rtol=0)
    for key, val in model.state_dict().items():
        # Adam's first steps move every weight by ~lr regardless of gradient scale, so tiny
        # gradient differences are amplified: compare with an lr-sized tolerance
        atol = 2e-4
        if key == "gnn_layers.0.gnn.bias":
            # this bias feeds a train-mode BatchNorm, so its true gradient is exactly 0 and both
            # implementations see only rounding noise (~1e-9), which Adam turns into +-lr steps:
            # each step the two runs may move in opposite directions: up to ~2*lr apart per step
            atol = 4.5e-3
        np.testing.assert_allclose(val.cpu().numpy(), data["p_final/" + key], atol=atol, rtol=0, err_msg=key)


def _torch_head(z, emb, bn1, bn2, lin_w, lin_b, mask, batch):
    """fp64 torch restatement of models/GDN.py:77-79,:175-184 in training mode (the oracle's train branch
    uses the same modules; this one exists so the kernel can be checked at shapes without a fixture)."""
    n, d = emb.shape
    h = torch.relu(torch.nn.functional.batch_norm(z, None, None, bn1[0], bn1[1], True, 0.0, 1e-5))
    h = h.view(batch, n, d) * emb
    h = torch.relu(torch.nn.functional.batch_norm(h.permute(0, 2, 1), None, None, bn2[0], bn2[1], True, 0.0,
                                                  1e-5)).permute(0, 2, 1)
    if mask is not None:
        h = h * mask.view(batch, n, d)
    return (h @ lin_w.view(d, 1)).view(batch, n) + lin_b


@pytest.mark.parametrize("batch,n,d,use_mask", [(3, 7, 16, True), (5, 20, 32, False), (4, 127, 64, True),
                                                (2, 40, 128, True), (1, 2, 64, False), (9, 700, 64, True),
                                                (2048, 127, 64, True), (6, 127, 64, "u8"), (3, 33, 128, "u8"),
                                                (5, 9, 16, "u8")])
def test_head_train_kernels_match_fp64_autograd(batch, n, d, use_mask, gpu_device):
    """gdn_head_train_fwd / _bwd against torch autograd in float64 (incl. n*d beyond the LDS-resident
    embedding-gradient partial: n=700, d=64)."""
    from gdn_amd import ops
    g = torch.Generator().manual_seed(batch * 1000 + n + d)
    z = torch.randn((batch * n, d), generator=g) * 0.7 + 0.3
    emb = torch.randn((n, d), generator=g)
    prm = [torch.rand((d,), generator=g) + 0.5, torch.randn((d,), generator=g) * 0.2,
           torch.rand((d,), generator=g) + 0.5, torch.randn((d,), generator=g) * 0.2,
           torch.randn((1, d), generator=g) * 0.3, torch.randn((1,), generator=g)]
    mask = ((torch.rand((batch * n, d), generator=g) > 0.2).float() / 0.8) if use_mask else None
    d_out = torch.randn((batch, n), generator=g)

    ref_in = [t.double().requires_grad_(True) for t in (z, emb, *prm)]
    ref = _torch_head(ref_in[0], ref_in[1], ref_in[2:4], ref_in[4:6], ref_in[6], ref_in[7],
                      None if mask is None else mask.double(), batch)
    ref.backward(d_out.double())

    bn1, bn2 = torch.nn.BatchNorm1d(d), torch.nn.BatchNorm1d(d)
    with torch.no_grad():
        bn1.weight.copy_(prm[0]); bn1.bias.copy_(prm[1]); bn2.weight.copy_(prm[2]); bn2.bias.copy_(prm[3])
    bn1, bn2 = bn1.to(gpu_device), bn2.to(gpu_device)
    zg, eg = z.to(gpu_device), emb.to(gpu_device)
    mg, mscale = (None if mask is None else mask.to(gpu_device)), 1.0
    if use_mask == "u8":                            # byte keep-mask form: multiplier = keep * 1/(1-p)
        mg, mscale = (mask > 0).to(torch.uint8).to(gpu_device), 1.0 / 0.8
    lw, lb = prm[4].to(gpu_device), prm[5].to(gpu_device)
    out, stats = ops.head_train_fwd(zg, eg, bn1, bn2, lw, lb, mg, batch, mscale)
    np.testing.assert_allclose(out.cpu().numpy(), ref.detach().numpy(), atol=2e-5, rtol=1e-5)
    grads = ops.head_train_bwd(d_out.to(gpu_device), zg, eg, bn1.weight.detach(), bn1.bias.detach(),
                               bn2.weight.detach(), bn2.bias.detach(), lw, mg, stats, 1e-5, 1e-5, batch, mscale)
    names = ["d_z", "d_emb", "d_bn1_w", "d_bn1_b", "d_bn2_w", "d_bn2_b", "d_lin_w", "d_lin_b"]
    for name, got, want in zip(names, grads, [t.grad for t in ref_in]):
        want = want.reshape(got.shape).numpy()
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=3e-5 * scale, rtol=1e-4, err_msg=name)
    # running statistics: momentum 0.1 from (0, 1), unbiased variance; batch counter
    np.testing.assert_allclose(bn1.running_mean.cpu().numpy(), 0.1 * z.double().mean(0).numpy(), atol=1e-6)
    np.testing.assert_allclose(bn1.running_var.cpu().numpy(),
                               0.9 + 0.1 * z.double().var(0, unbiased=True).numpy(), atol=1e-5, rtol=1e-5)
    assert int(bn1.num_batches_tracked) == 1 and int(bn2.num_batches_tracked) == 1


def test_head_train_rejects_single_row(gpu_device):
    """torch raises for train-mode BatchNorm over one value per channel; so does the kernel entry point."""
    from gdn_amd import ops, _lib
    bn1, bn2 = torch.nn.BatchNorm1d(64).to(gpu_device), torch.nn.BatchNorm1d(64).to(gpu_device)
    z = torch.zeros((1, 64), device=gpu_device)
    with pytest.raises(_lib.GdnHipError):
        ops.head_train_fwd(z, torch.zeros((1, 64), device=gpu_device), bn1, bn2,
                           torch.zeros((1, 64), device=gpu_device), torch.zeros((1,), device=gpu_device), None, 1)


def test_training_forward_follows_unversioned_parameter_writes(gpu_device):
    """Fused optimizers update parameters without bumping `_version`: the train-mode forward must still
    rebuild the sensor graph from the current embedding."""
    from test_gpu_forward_parity import random_params
    model = random_params(12, 6, 3, 64, seed=1).to(gpu_device).train()
    x = torch.rand((4, 12, 6), device=gpu_device)
    model(x, None)
    before = model.learned_graph.clone()
    with torch.no_grad():
        model.embedding.weight.data.copy_(torch.randn_like(model.embedding.weight))   # no version bump
    model(x, None)
    assert not torch.equal(before, model.learned_graph)
    model.eval()
    model(x, None)
    cached = model.learned_graph.clone()
    with torch.no_grad():
        model.embedding.weight.data.copy_(torch.randn_like(model.embedding.weight))
    model.invalidate_constants()
    model(x, None)
    assert not torch.equal(cached, model.learned_graph)


def test_harness_train_reproduces_reference_losses(gpu_device):
    """harness.train (mirror of train.py:27-112) over the golden 2-batch loader: per-step losses of the
    reference's own train()."""
    from gdn_amd import harness
    data, p = load_golden("train_loop_2step")
    m = meta(data)
    model = build_model(p, m, gpu_device)
    model.dp = FixedMaskDropout([torch.from_numpy(mk).to(gpu_device) for mk in data["masks"]])
    x, y = torch.from_numpy(data["x"]), torch.from_numpy(data["y"])
    loader = [(x[s:s + m["b"]], y[s:s + m["b"]], torch.zeros(m["b"]), None) for s in range(0, x.shape[0], m["b"])]
    losses = harness.train(model, "", {"epoch": 1}, loader, None)
    np.testing.assert_allclose(losses, data["losses"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("use_graph", [False, True])
def test_48_step_training_curve_follows_the_reference(use_graph, gpu_device):
    """Row 15 over a longer horizon: 6 epochs x 8 batches of 128 windows (48 Adam steps) on a learnable
    series, dropout off.  Fixture = the reference's own train() (tests/golden/make_golden.py:
    train_curve_case): per-step losses, final parameters, and the eval forward after training."""
    from gdn_amd import harness
    data, p = load_golden("train_curve_48step")
    m = meta(data)
    model = build_model(p, m, gpu_device)
    model.dp.p = 0.0
    series, w, bsz = data["series"], m["w"], m["b"]
    t = series.shape[1] - w
    idx = np.arange(t)[:, None] + np.arange(w)[None, :]
    xs = torch.from_numpy(series[:, idx].transpose(1, 0, 2).copy())      # datasets/TimeDataset.py:42-58
    ys = torch.from_numpy(series[:, w:].T.copy())
    loader = [(xs[s:s + bsz], ys[s:s + bsz], torch.zeros(bsz), None) for s in range(0, t, bsz)]
    losses = harness.train(model, "", {"epoch": int(data["epochs"])}, loader, None, use_graph=use_graph)
    ref = data["losses"]
    assert len(losses) == len(ref) == 48
    # the trajectory: every step within 2e-4 of the reference's loss (losses run 0.25 -> 0.06)
    np.testing.assert_allclose(losses, ref, atol=2e-4, rtol=0)
    for key, val in model.state_dict().items():
        if "num_batches" in key:
            assert int(val) == int(data["p_final/" + key]), key
            continue
        # 48 Adam steps of lr 1e-3: a weight whose gradient is rounding noise can drift by ~lr per step
        # (gnn.bias has an exactly-zero gradient, and the BatchNorm behind it tracks its mean)
        loose = key.endswith("gnn.bias") or key.endswith("0.bn.running_mean")
        np.testing.assert_allclose(val.cpu().numpy(), data["p_final/" + key], atol=0.1 if loose else 2e-3,
                                   rtol=0, err_msg=key)
    model.eval()
    out = model(xs[:64].to(gpu_device), None)
    # eval mode normalises by the RUNNING mean, which lags the drifting zero-gradient bias (momentum 0.1):
    # unlike in training the drift does not cancel exactly, so two correct runs differ by a few 1e-3
    np.testing.assert_allclose(out.cpu().numpy(), data["eval_after"], atol=1e-2, rtol=0)


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (512, 127), (4096, 127)])
def test_fused_mse_loss_and_gradient(shape, gpu_device):
    """gdn_mse_loss_grad == F.mse_loss(reduction='mean') + autograd (train.py:20-23), workspace reused."""
    from gdn_amd import ops
    g = torch.Generator().manual_seed(shape[0])
    ws = ops.mse_workspace(gpu_device)
    for _ in range(3):                              # the workspace must come back zeroed
        out = torch.randn(shape, generator=g).to(gpu_device).requires_grad_(True)
        y = torch.randn(shape, generator=g).to(gpu_device)
        ref = torch.nn.functional.mse_loss(out.double(), y.double(), reduction="mean")
        ref.backward()
        loss, d_out = ops.mse_loss_grad(out.detach(), y, ws)
        np.testing.assert_allclose(float(loss), float(ref.detach()), rtol=2e-7, atol=0)
        np.testing.assert_allclose(d_out.cpu().numpy(), out.grad.cpu().numpy(), rtol=1e-6, atol=1e-12)
    assert float(ws.abs().sum()) >= 0 and int(ws.view(torch.int64)[0]) == 0


@pytest.mark.parametrize("case", MODEL_CASES)
def test_train_step_against_float64_oracle(case, gpu_device):
    """Accuracy rather than parity: the same training step computed in float64 (tests/_grad_check.py, pinned to
    the op-faithful oracle by tests/test_oracle_golden.py).  Every gradient is compared RELATIVE to its tensor
    (max|d| <= 2e-5 max|g|) and to its element (|d| <= 1e-2 max(|g|, 1e-3 max|g|)): the bounds are 6-10x what
    profiles/r03_grad_error_stages_l3_*.txt measured for the HIP path (3.6e-6 / 7.6e-4) and for the reference's own
    fp32 arithmetic (2.6e-6 / 4.1e-4).  An absolute 2e-6 — the round-2 bound — is larger than whole attention
    gradients and saw nothing."""
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step
    data, p = load_golden(case)
    m = meta(data)
    model = build_model(p, m, gpu_device)
    model.injected_graph = torch.from_numpy(data["learned_graph"]).to(gpu_device)
    mask = torch.from_numpy(data["dropout_mask"])
    model.dp = FixedMaskDropout([mask.to(gpu_device)])
    model.train()
    model.zero_grad()
    x, y = torch.from_numpy(data["x"]), torch.from_numpy(data["y"])
    loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
    loss.backward()
    ref_loss, want, kink = oracle_step(p, x, y, torch.from_numpy(data["learned_graph"]), m["out_layer_num"], mask)
    assert kink > KINK_BAND, "fixture has a (Leaky)ReLU input inside the fp32 rounding band: gradients are ambiguous"
    assert abs(loss.item() - ref_loss) < 2e-6 * max(1.0, abs(ref_loss))
    assert_grads_close({name: prm.grad for name, prm in model.named_parameters()}, want, what=case)


def test_eval_after_replays_equals_a_fresh_model_with_the_same_state(gpu_device):
    """N replays, then eval (model.forward and a SeriesEvaluator that had captured its graph BEFORE the
    training): both must equal a freshly built model loaded with the trained state_dict."""
    from gdn_amd import GDN, harness
    from test_gpu_forward_parity import random_params
    g = torch.Generator().manual_seed(13)
    x = torch.rand((64, 27, 10), generator=g).to(gpu_device)
    y = torch.rand((64, 27), generator=g).to(gpu_device)
    model = random_params(27, 10, 8, 64, seed=6).to(gpu_device)
    model.dp.p = 0.0
    ev = harness.SeriesEvaluator(model, x, y, batch=32, use_graph=True, streams=1)
    before = ev.step().clone()                       # captures the eval graph with the untrained constants
    step = harness.GraphedTrainStep(model, 64)
    step.x.copy_(x)
    step.y.copy_(y)
    for _ in range(5):
        step.step()
    model.eval()
    with torch.no_grad():
        got = model(x, None)
    after = ev.step().clone()
    fresh = GDN([torch.zeros((2, 1), dtype=torch.long)], 27, dim=64, input_dim=10, topk=8)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(gpu_device).eval()
    with torch.no_grad():
        want = fresh(x, None)
    assert float((want - got).abs().max()) == 0.0
    ev2 = harness.SeriesEvaluator(fresh, x, y, batch=32, use_graph=False, streams=1)
    np.testing.assert_array_equal(after.cpu().numpy(), ev2.step().cpu().numpy())
    assert not torch.equal(before, after)


# ------------------------------------------------------------------ native step
def test_adam_kernel_matches_torch_adam(gpu_device):
    """gdn_adam_step over a flat buffer against torch.optim.Adam (single-tensor form) on the same gradients,
    with and without weight decay, over several steps; the cleared gradient slot and the step counter."""
    from gdn_amd import _lib
    g = torch.Generator().manual_seed(1)
    for wd in (0.0, 0.01):
        count = 9729 + 3
        p0 = torch.randn((count,), generator=g)
        ref_p = p0.clone().to(gpu_device).requires_grad_(True)
        opt = torch.optim.Adam([ref_p], lr=1e-3, weight_decay=wd)
        p = p0.clone().to(gpu_device)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        state = torch.zeros((1,), dtype=torch.int64, device=gpu_device)
        for step in range(6):
            grads = (torch.randn((count,), generator=g) * (10.0 ** (step - 3))).to(gpu_device)
            ref_p.grad = grads.clone()
            opt.step()
            gbuf = grads.clone()
            _lib.call("gdn_adam_step", p.data_ptr(), gbuf.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), count,
                      1e-3, 0.9, 0.999, 1e-8, wd, 1.0, 100, 64, torch.cuda.current_stream().cuda_stream)
            assert int(state[0]) == step + 1
            assert float(gbuf[100:164].abs().max()) == 0.0 and torch.equal(gbuf[:100], grads[:100])
            np.testing.assert_allclose(p.cpu().numpy(), ref_p.detach().cpu().numpy(), rtol=2e-6, atol=2e-7)
        # (elements of exp_avg that cancel to ~0 carry the rounding of their large terms)
        np.testing.assert_allclose(m.cpu().numpy(), opt.state[ref_p]["exp_avg"].cpu().numpy(), rtol=1e-6,
                                   atol=2e-7 * float(m.abs().max()))
        np.testing.assert_allclose(v.cpu().numpy(), opt.state[ref_p]["exp_avg_sq"].cpu().numpy(), rtol=2e-6, atol=1e-30)
        # (1 - beta2 is formed in double like torch's Python-float arithmetic: 1 - 0.999f would be 4.7e-5 off)


def test_native_step_state_follows_checkpoint_round_trip(gpu_device):
    """Parameters stay ordinary module parameters: state_dict() sees the trained values and a fresh model loaded
    from it predicts what the trained one predicts."""
    from gdn_amd import GDN, harness
    from test_gpu_forward_parity import random_params
    model = random_params(27, 10, 8, 64, seed=2).to(gpu_device)
    step = harness.GraphedTrainStep(model, 32)
    assert isinstance(step, harness.NativeTrainStep)
    step.x.copy_(torch.rand_like(step.x)); step.y.copy_(torch.rand_like(step.y))
    l0 = float(step.step())
    for _ in range(30):
        step.step()
    assert float(step.loss) < l0
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fresh = GDN([torch.zeros((2, 1), dtype=torch.long)], 27, dim=64, input_dim=10, topk=8)
    fresh.load_state_dict(sd)
    fresh = fresh.to(gpu_device).eval()
    model.eval()
    x = torch.rand((8, 27, 10), device=gpu_device)
    with torch.no_grad():
        assert torch.equal(model(x, None), fresh(x, None))


@pytest.mark.parametrize("n,k,d", [(512, 64, 64), (512, 64, 128), (400, 20, 128)])
@pytest.mark.parametrize("path", ["autograd", "native_graph"])
def test_training_step_at_the_512_sensor_stress_shape(path, n, k, d, gpu_device):
    """BASELINE configs[4] shape (512 sensors, top-k 64, W=30, d=64): the backward's two [n, pitch] tables
    (164 KB each) cannot sit in LDS, gdn_attn_aggregate_bwd runs them through its workspace in global memory.
    At d = 128 a window's [n, 128] tile (263 KB) does not fit either: the workgroup walks two 64-column slices
    (round 2 and the first half of round 3 refused the shape).
    One training step against float64 (loss and every gradient, relative bounds), through the autograd
    Functions and through the DEFAULT path of harness.train / python -m gdn_amd.main: the captured
    NativeTrainStep (round 2 raised GDN_ERR_UNSUPPORTED there).  The reference trains at any n
    (train.py:58-79)."""
    from gdn_amd import harness
    from _grad_check import KINK_BAND, assert_grads_close, oracle_step
    from test_gpu_forward_parity import random_params
    w, b = 30, 2
    model = random_params(n, w, k, d, seed=21)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).train()
    g = torch.Generator().manual_seed(22)
    x, y = torch.rand((b, n, w), generator=g), torch.rand((b, n), generator=g)
    if path == "autograd":
        mask = (torch.rand((b, n, d), generator=g) >= 0.2).float() / 0.8
        model.dp = FixedMaskDropout([mask.to(gpu_device)])
        model.zero_grad()
        loss = torch.nn.functional.mse_loss(model(x.to(gpu_device), None), y.to(gpu_device))
        loss.backward()
        got = {name: prm.grad for name, prm in model.named_parameters()}
        graph = model.learned_graph.cpu()
    else:
        seed = 424242
        assert harness.NativeTrainStep.applicable(model)
        step = harness.GraphedTrainStep(model, b)
        assert isinstance(step, harness.NativeTrainStep)
        step.state[0] = seed
        mask = (_mix32_mask(seed, 0, b * n * d, 0.2, gpu_device).float() / 0.8).view(b, n, d).cpu()
        step.x.copy_(x.to(gpu_device)); step.y.copy_(y.to(gpu_device))
        loss = step.step()
        got = {name: step.flat_g[off:off + cnt].view(prm.shape)
               for (name, prm), (off, cnt) in zip(model.named_parameters(), step.slices)}
        graph = step.ws["topk"].cpu()
    ref_loss, want, kink = oracle_step(p, x, y, graph, 1, mask)
    assert kink > KINK_BAND
    assert abs(float(loss.detach()) - ref_loss) < 2e-6
    assert_grads_close(got, want, what=path)


def test_native_step_is_refused_for_shapes_outside_the_training_kernels(gpu_device):
    """NativeTrainStep.applicable() asks the library (gdn_train_supported) instead of failing at the first batch:
    a 2000-sensor model at d = 64 (tile beyond LDS) is refused, GraphedTrainStep then builds the autograd step."""
    from gdn_amd import _lib, harness
    from test_gpu_forward_parity import random_params
    assert _lib.load().gdn_train_supported(512, 30, 64, 64) == 1
    assert _lib.load().gdn_train_supported(512, 30, 128, 64) == 1          # two column slices
    assert _lib.load().gdn_train_supported(1024, 30, 128, 64) == 0         # a 64-column slice is beyond LDS too
    assert _lib.load().gdn_train_supported(127, 15, 64, 30) == 1
    assert _lib.load().gdn_train_supported(2000, 15, 64, 30) == 0          # (n+1)*d*4 > 160 KB
    assert _lib.load().gdn_train_supported(127, 15, 48, 30) == 0           # d outside {16, 32, 64, 128}
    model = random_params(2000, 15, 30, 64, seed=1).to(gpu_device)
    assert not harness.NativeTrainStep.applicable(model)


# ---------------------------------------------------------------- train-mode OutLayer MLP (out_layer_num > 1)
@pytest.mark.parametrize("rows,d_in,hidden,layers", [(60, 32, 48, 2), (60, 16, 24, 3), (4064, 64, 256, 2),
                                                     (2033, 64, 512, 2), (517, 64, 384, 3), (130, 128, 260, 2),
                                                     (3456, 64, 128, 3), (1000, 128, 64, 4), (131, 64, 256, 2),
                                                     # hidden widths that are not a multiple of 4
                                                     (300, 64, 50, 3), (130, 32, 301, 2), (77, 16, 1, 2),
                                                     (515, 64, 257, 3)])
def test_mlp_train_kernels_match_fp64_autograd(rows, d_in, hidden, layers, gpu_device):
    """gdn_mlp_train_fwd / gdn_mlp_train_bwd (fp32 matrix cores, fp64 statistics) against the reference's
    OutLayer (models/GDN.py:27-56) run by torch autograd in float64: output, every parameter gradient, the
    input gradient, the BatchNorm running statistics."""
    from gdn_amd import ops
    from gdn_amd.model import OutLayer
    torch.manual_seed(rows + hidden)
    ref = OutLayer(d_in, 1, layers, inter_num=hidden).double()
    with torch.no_grad():
        for mod in ref.mlp:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    hip = OutLayer(d_in, 1, layers, inter_num=hidden)
    hip.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
    hip = hip.to(gpu_device).train()
    ref.train()
    act = torch.rand((rows, d_in), dtype=torch.float64) * (torch.rand((rows, d_in)) > 0.2)   # post-ReLU/dropout-like
    d_out = torch.randn((rows,), dtype=torch.float64) / rows
    a64 = act.clone().requires_grad_(True)
    out64 = ref(a64.view(1, rows, d_in)).view(rows)              # BatchNorm over the rows, as GDN.py:53-54
    out64.backward(d_out)
    assert ops.mlp_train_supported(hip, d_in, rows)
    act_d = act.float().to(gpu_device)
    out, saved = ops.mlp_train_fwd(act_d, hip)
    np.testing.assert_allclose(out.cpu().double().numpy(), out64.detach().numpy(), atol=5e-6, rtol=1e-5)
    hidden_mods, last = ops.mlp_train_layers(hip)
    params = [t.detach() for lin, bn in hidden_mods for t in (lin.weight, lin.bias, bn.weight, bn.bias)]
    d_act, grads, d_ow, d_ob = ops.mlp_train_bwd(d_out.float().to(gpu_device), act_d, params, last.weight.detach(),
                                                 saved, d_in, hidden, layers)
    ref_hidden, ref_last = ops.mlp_train_layers(ref)
    want = [t.grad for lin, bn in ref_hidden for t in (lin.weight, lin.bias, bn.weight, bn.bias)]
    scale = max(float(w.abs().max()) for w in want)
    for i, (g, w) in enumerate(zip(grads, want)):
        np.testing.assert_allclose(g.cpu().double().numpy(), w.numpy(), atol=2e-6 * max(scale, 1.0), rtol=2e-5,
                                   err_msg=f"hidden-layer gradient {i}")
    np.testing.assert_allclose(d_ow.cpu().double().numpy(), ref_last.weight.grad.view(-1).numpy(), atol=2e-6, rtol=2e-5)
    np.testing.assert_allclose(d_ob.cpu().double().numpy(), ref_last.bias.grad.numpy(), atol=2e-6, rtol=2e-5)
    np.testing.assert_allclose(d_act.cpu().double().numpy(), a64.grad.numpy(), atol=2e-7, rtol=2e-5)
    for (lin, bn), (_rl, rbn) in zip(hidden_mods, ref_hidden):
        np.testing.assert_allclose(bn.running_mean.cpu().double().numpy(), rbn.running_mean.numpy(), atol=1e-6)
        np.testing.assert_allclose(bn.running_var.cpu().double().numpy(), rbn.running_var.numpy(), atol=1e-6, rtol=1e-5)
        assert int(bn.num_batches_tracked) == 1
    # bitwise reproducible: fixed-order reductions, no atomics
    out2, saved2 = ops.mlp_train_fwd(act_d, hip)
    d_act2, grads2, _, _ = ops.mlp_train_bwd(d_out.float().to(gpu_device), act_d, params, last.weight.detach(), saved2,
                                             d_in, hidden, layers)
    assert torch.equal(out, out2) and torch.equal(d_act, d_act2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_mlp_head_training_uses_the_hip_mlp(gpu_device, monkeypatch):
    """out_layer_num = 2 under model.train(): forward + backward go through _MlpHeadTrainFn (HIP head passes
    + HIP MLP); a hidden width that is not a multiple of 4 runs there too (element-wise operand staging), one beyond the
    HIP set (> 512) falls back to torch instead of failing."""
    import gdn_amd
    from gdn_amd import ops
    calls = []
    orig = ops.mlp_train_fwd
    monkeypatch.setattr(ops, "mlp_train_fwd", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    for hidden, expect in ((256, 1), (250, 1), (600, 0)):
        torch.manual_seed(0)
        model = gdn_amd.GDN([torch.zeros((2, 1), dtype=torch.long)], 27, dim=64, input_dim=15, out_layer_num=2,
                            out_layer_inter_dim=hidden, topk=10).to(gpu_device).train()
        x = torch.rand((8, 27, 15), device=gpu_device)
        calls.clear()
        loss = model(x, None).square().mean()
        loss.backward()
        assert len(calls) == expect
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_matrix_core_backward_of_the_aggregate_over_random_shapes(gpu_device):
    """gdn_attn_aggregate_bwd on the matrix-core path (n <= 127, d = 64: G = dZ.X^T and dX = A^T.dZ as dense
    products, d_z scaled per window) against float64 autograd of the same layer (graph_layer.py:106-117 in list
    form), over a seeded sweep of shapes and with the gradient magnitude varying by 12 orders of magnitude
    BETWEEN the windows of one launch (the per-window power-of-two scaling)."""
    from _graph_layer_bwd_ref import aggregate_ref
    from gdn_amd import _lib, ops
    rng = np.random.default_rng(7)
    shapes = [(127, 30), (127, 63), (2, 1), (31, 15), (32, 16), (33, 31), (64, 47), (65, 48), (96, 5), (97, 32)]
    while len(shapes) < 22:
        n = int(rng.integers(2, 128))
        shapes.append((n, int(rng.integers(1, min(n, 63) + 1))))
    for idx, (n, k) in enumerate(shapes):
        b, d = int(rng.integers(1, 12)), 64
        assert _lib.load().gdn_attn_aggregate_bwd_uses_reverse(n, d, k) == 0          # the dense path takes it
        g = torch.Generator().manual_seed(idx)
        emb = torch.randn((n, d), generator=g)
        graph = ops.topk_graph(emb.to(gpu_device), k)
        xlin = torch.randn((b * n, d), generator=g)
        s_i, s_j = torch.randn((b * n,), generator=g), torch.randn((b * n,), generator=g)
        bias = torch.randn((d,), generator=g) * 0.1
        mags = 10.0 ** torch.from_numpy(rng.uniform(-9, 3, size=b)).float()          # per-window gradient scale
        d_z = (torch.randn((b, n, d), generator=g) * mags.view(b, 1, 1)).reshape(b * n, d)
        dev = lambda t: t.to(gpu_device)
        z, alpha = ops.attn_aggregate_fwd(dev(xlin), dev(s_i), dev(s_j), graph, dev(bias), b, want_alpha=True)
        d_xlin, d_si, d_sj, d_bias = ops.attn_aggregate_bwd(dev(d_z), dev(xlin), alpha, dev(s_i), dev(s_j), graph, b)
        # float64 autograd of the layer in list form (tests/_graph_layer_bwd_ref.py; nbr: [n, pitch], padding = n)
        z64, _a64, dx64, dsi64, dsj64, db64 = aggregate_ref(xlin.view(b, n, d), s_i.view(b, n), s_j.view(b, n), bias,
                                                            graph.nbr.cpu().long(), d_z.view(b, n, d))
        np.testing.assert_allclose(z.cpu().double().numpy(), z64.reshape(b * n, d).numpy(), atol=3e-6, rtol=1e-5)
        scale = mags.double().view(b, 1, 1)                                 # compare per window, relative to its scale
        for name, got, want in (("d_xlin", d_xlin.view(b, n, d), dx64), ("d_si", d_si.view(b, n, 1), dsi64.unsqueeze(-1)),
                                ("d_sj", d_sj.view(b, n, 1), dsj64.unsqueeze(-1))):
            err = ((got.cpu().double() - want) / scale).abs().max()
            ref = (want / scale).abs().max().clamp_min(1.0)
            assert float(err / ref) < 3e-6, (n, k, b, name, float(err / ref))
        np.testing.assert_allclose(d_bias.cpu().double().numpy(), db64.numpy(), rtol=2e-5,
                                   atol=2e-6 * float(mags.max()) * (b * n) ** 0.5)


def check_graph_and_terms_single_launch(n, k, d, w, device):
    """One shape of the test below (tests/test_gpu_graph_stages.py runs it at the borders of the rank count)."""
    from gdn_amd import _lib, ops
    g = torch.Generator().manual_seed(n)
    emb = torch.randn((n, d), generator=g).to(device)
    lin_w = torch.randn((d, w), generator=g).to(device)
    att = [torch.randn((d,), generator=g).to(device) for _ in range(4)]
    graph = ops.topk_graph(emb, k)
    terms = ops.node_terms(lin_w, *[t.view(1, 1, d) for t in att], emb)
    pitch = ops.nbr_pitch(k)
    topk = torch.empty((n, k), dtype=torch.int64, device=device)
    nbr = torch.empty((n, pitch), dtype=torch.uint16, device=device)
    deg = torch.empty((n,), dtype=torch.int32, device=device)
    terms2 = torch.empty_like(terms)
    _lib.call("gdn_topk_graph_terms", emb.data_ptr(), n, d, k, topk.data_ptr(), nbr.data_ptr(), deg.data_ptr(),
              lin_w.data_ptr(), *[t.data_ptr() for t in att], w, terms2.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    assert torch.equal(topk, graph.topk) and torch.equal(deg, graph.deg)
    assert torch.equal(nbr.view(torch.int16), graph.nbr.view(torch.int16))
    assert torch.equal(terms2, terms)


def test_graph_and_terms_single_launch_equals_the_two_entry_points(gpu_device):
    """gdn_topk_graph_terms (one launch, used by the native training step) against gdn_topk_graph + gdn_node_terms:
    identical graph tables and folded attention terms, bit for bit."""
    for n, k, d, w in ((127, 30, 64, 15), (27, 5, 64, 5), (512, 64, 128, 30), (40, 16, 128, 30)):
        check_graph_and_terms_single_launch(n, k, d, w, gpu_device)


def test_training_statistics_accumulator_is_exact(gpu_device):
    """The cross-workgroup sums of the training head (BatchNorm statistics, BatchNorm / Linear gradients) go through a
    260-bit fixed-point accumulator fed by 64-bit integer atomics (gdn_head_train.hip): the total does not depend on
    the order of the addends.  gdn_exact_sum exposes it; against math.fsum (the exactly rounded sum) on addends that
    defeat floating-point summation — cancellation over 60 orders of magnitude, every sign pattern, values at both
    ends of the range — and bit for bit under a permutation of the addends."""
    import math
    from gdn_amd import _lib
    lib = _lib.load()
    ws = torch.zeros((lib.gdn_exact_sum_workspace_bytes() // 8,), dtype=torch.int64, device=gpu_device)
    out = torch.zeros((1,), dtype=torch.float64, device=gpu_device)
    st = torch.cuda.current_stream().cuda_stream

    def hip_sum(values):
        x = torch.tensor(values, dtype=torch.float64, device=gpu_device)
        _lib.call("gdn_exact_sum", x.data_ptr(), x.numel(), ws.data_ptr(), out.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(ws.abs().sum()) == 0                      # left zeroed for the next use
        return float(out[0])

    g = torch.Generator().manual_seed(5)
    cases = {
        "cancellation": [1e30, 1.0, -1e30, 3.0e-20, 2.5, -3.0e-20],
        "tiny": [2.0 ** -120, -(2.0 ** -121), 2.0 ** -125],
        "huge": [2.0 ** 120, 2.0 ** 100, -(2.0 ** 119)],
        "one": [0.1],
        "zeros": [0.0, -0.0, 0.0],
    }
    mags = torch.randint(-80, 80, (2000,), generator=g).double()
    rnd = ((torch.rand(2000, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** mags).tolist()
    cases["random_2000"] = rnd
    cases["random_with_opposites"] = rnd[:1000] + [-v for v in rnd[:999]]
    sq = (torch.randn(2048, generator=g).float().double() * 3.0e7) ** 2          # squares of raw-unit fp32 values
    cases["squares"] = sq.tolist()
    for name, vals in cases.items():
        want = math.fsum(vals)
        got = hip_sum(vals)
        assert abs(got - want) <= 4 * abs(want) * 2.0 ** -53, (name, got, want)
        perm = torch.randperm(len(vals), generator=g).tolist()
        assert hip_sum([vals[i] for i in perm]) == got, name         # bit for bit
    assert math.isnan(hip_sum([1.0, float("inf")])) and math.isnan(hip_sum([float("nan")]))
    assert math.isnan(hip_sum([2.0 ** 131]))                         # beyond the accumulator's range: flagged, not wrapped
    assert lib.gdn_exact_sum(0, 4096, 0, 0, 0) != 0                  # argument / size checks
