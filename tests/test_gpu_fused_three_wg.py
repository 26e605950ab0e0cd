"""The fused dense forward with fp32 storage computes the attention scalars s_i / s_j on the VALU from the staged
registers (no row-major x tile, no scalar-tile products), keeps the X^T fragments compact where rows 16 .. 31 do not
exist, and runs three workgroups per CU (gdn_forward_dense.hip, DCfg::XAGG / XHALF / WGS; a launch whose occupancy
query reports fewer fails, so every launch here checks it).  Every case is held against the float64 oracle at the
bar of tests/test_gpu_fused_reordered.py: 2e-7 of the output scale, planned and plan-less."""
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import random_params
from test_gpu_fused_reordered import _planned_launch_with_guard, assert_fp32_grade, f64_params, planned_and_plain

pytestmark = pytest.mark.gpu

EDGE_W = (1, 15, 16, 17, 30)
EDGE_N = (1, 32, 33, 96, 127)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("w", EDGE_W)
def test_tile_edges_in_w_and_n(w, n, gpu_device):
    k = min(20, n)
    model = random_params(n, w, k, 64, seed=91)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((19, n, w), generator=torch.Generator().manual_seed(92))
    assert_fp32_grade(model, p, x, k, gpu_device)


@pytest.mark.parametrize("n,w,d", [(31, 15, 64), (32, 16, 64), (63, 15, 64), (63, 17, 64),
                                   (31, 15, 128), (33, 16, 128), (63, 30, 128)])
def test_fully_connected_graphs(n, w, d, gpu_device):
    model = random_params(n, w, n, d, seed=93)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((11, n, w), generator=torch.Generator().manual_seed(94))
    assert_fp32_grade(model, p, x, n, gpu_device)


@pytest.mark.parametrize("n,w,k,d", [(127, 15, 30, 64), (127, 15, 30, 128), (96, 30, 20, 64)])
def test_attention_that_follows_the_window(n, w, k, d, gpu_device):
    """att_i / att_j four times their initial size: the part of a logit that depends on the window, a_i . x_i +
    a_j . x_j, then outweighs the embedding part c_i + c_j (asserted below on the float64 terms), so the softmax is
    decided by the scalars this kernel now computes as fp32 dot products.  Why four: the logits stay O(1), where an
    fp32 dot product of w <= 30 terms is good to a few 2^-24 and the 2e-7 bar is one fp32 arithmetic can hold;
    tests/test_cpu_fused_scalar_path_emulation.py holds the emulated chain to the same bar on the same model."""
    model = random_params(n, w, k, d, seed=81)
    with torch.no_grad():
        model.gnn_layers[0].gnn.att_i.mul_(4.0)
        model.gnn_layers[0].gnn.att_j.mul_(4.0)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    x = torch.rand((8, n, w), generator=torch.Generator().manual_seed(82))
    gnn, lin = model.gnn_layers[0].gnn, model.gnn_layers[0].gnn.lin.weight.detach().double()
    emb = model.embedding.weight.detach().double()
    from_x = sum(((x.double() @ (att.detach().double().reshape(-1) @ lin)).std() for att in (gnn.att_i, gnn.att_j)))
    from_emb = sum(((emb @ att.detach().double().reshape(-1)).std() for att in (gnn.att_em_i, gnn.att_em_j)))
    print(f"logit spread from the window {float(from_x):.3f}, from the embeddings {float(from_emb):.3f}")
    assert float(from_x) > float(from_emb)
    model = model.to(gpu_device).eval()
    assert_fp32_grade(model, p, x, k, gpu_device)


LIMIT = 7500.0          # 60000 / 2^3: the x limit of every plan (asserted below)
LIMIT_SHAPES = [(127, 15, 30, 64), (40, 20, 12, 128)]


def _near_limit_model(n, w, k, d, gpu_device, att_scale=1.0):
    model = random_params(n, w, k, d, seed=95)
    with torch.no_grad():
        model.gnn_layers[0].gnn.att_i.mul_(att_scale)
        model.gnn_layers[0].gnn.att_j.mul_(att_scale)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    with torch.no_grad():
        model(torch.rand((1, n, w)).to(gpu_device), None)
    assert model.operand_limit() == LIMIT
    return model, p


@pytest.mark.parametrize("n,w,k,d", LIMIT_SHAPES)
def test_inputs_just_below_the_x_limit(n, w, k, d, gpu_device):
    """Spikes: 41 entries of a batch of O(1) inputs sit at +-0.9999 of the x limit, the last column of the last sensor
    of the last window among them; the launch leaves its range flag down and is held to 2e-7 of the output scale
    like every other case of this file.
    The margin is thin by nature, not by accident: a spiked sensor's features are O(1e3) where the output is O(1e2),
    so fp32 arithmetic sits AT this bar.  On these two shapes the fp32 oracle is itself 1.6e-5 / 1.3e-5 from float64
    where 2e-7 of the output scale is 1.9e-5 / 9.8e-6; the numpy emulation of the kernel's chain 1.6e-5 (d = 64); the
    kernel measured 1.57e-5 / 8.1e-6, planned and plan-less alike."""
    model, p = _near_limit_model(n, w, k, d, gpu_device)
    b = 21
    g = torch.Generator().manual_seed(96)
    x = torch.rand((b, n, w), generator=g)
    idx = torch.randint(0, b * n * w, (40,), generator=g)
    x.view(-1)[idx] = 0.9999 * LIMIT * torch.where(torch.rand(40, generator=g) < 0.5, -1.0, 1.0)
    x[b - 1, n - 1, w - 1] = 0.9999 * LIMIT
    _out, guard = _planned_launch_with_guard(model, x.to(gpu_device))
    assert guard == [0, 0]
    assert_fp32_grade(model, p, x, k, gpu_device)


@pytest.mark.parametrize("n,w,k,d", LIMIT_SHAPES)
def test_attention_scalars_of_inputs_just_below_the_x_limit(n, w, k, d, gpu_device):
    """Beyond the issue's list: EVERY input up to 0.9999 of the limit, att_i / att_j divided by 4000 so that the
    logits are O(1) and depend on x through the fp32 dot products of phase X alone.  The bound is 4 x the fp32
    oracle's own deviation from float64 on the same inputs (no term in the output scale).  What it catches: the
    features are O(1e3), so a relative error e of a logit moves the output by about e x 1e3; scalars carried in one
    f16 term (e = 5e-4) or a coefficient column lost in the reduction would be three to four orders beyond it."""
    model, p = _near_limit_model(n, w, k, d, gpu_device, att_scale=1.0 / 4000.0)
    x = torch.rand((21, n, w), generator=torch.Generator().manual_seed(96)) * (0.999 * LIMIT)
    x[2, 3, 0] = -0.9999 * LIMIT
    out, guard = _planned_launch_with_guard(model, x.to(gpu_device))
    assert guard == [0, 0]
    graph = model.learned_graph.cpu()
    ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=graph)["out"]
    ref32 = gdn_oracle.forward(p, x, k, graph=graph)["out"].double()
    err, bound = float((out.cpu().double() - ref).abs().max()), 4.0 * float((ref32 - ref).abs().max())
    print(f"all inputs near the limit, logits O(1): err {err:.3e} bound {bound:.3e} "
          f"(2e-7 of the output scale: {2e-7 * max(1.0, float(ref.abs().max())):.3e})")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("n,w,k,d", LIMIT_SHAPES)
def test_a_value_at_or_above_the_x_limit_raises_the_range_flag(n, w, k, d, gpu_device):
    """The predicate runs on the staged registers: a value above the limit, one AT it in the last column of the last
    sensor of the last window, minus the limit in the first, and a NaN each raise the flag; the same batch without
    them leaves it down."""
    model, _p = _near_limit_model(n, w, k, d, gpu_device)
    b = 21
    below = torch.rand((b, n, w), generator=torch.Generator().manual_seed(96)) * (0.999 * LIMIT)
    _out, guard = _planned_launch_with_guard(model, below.to(gpu_device))
    assert guard == [0, 0]
    for where, value in (((5, n // 2, w // 2), 1.0001 * LIMIT), ((b - 1, n - 1, w - 1), LIMIT),
                         ((0, 0, 0), -LIMIT), ((3, n - 1, 0), float("nan"))):
        above = below.clone()
        above[where] = value
        _out, guard = _planned_launch_with_guard(model, above.to(gpu_device))
        assert guard[0] == 1, (where, value)


def test_lists_with_sentinel_slots(gpu_device):
    """k = 5 in a pitch of 16 and k = 17 in a pitch of 32: most slots of a list are the sentinel, whose s_j is
    -inf and whose image column stays zero."""
    for n, w, k, d in ((127, 15, 5, 64), (50, 15, 17, 64), (33, 12, 1, 128)):
        model = random_params(n, w, k, d, seed=97)
        p = {key: v.detach().clone() for key, v in model.state_dict().items()}
        model = model.to(gpu_device).eval()
        x = torch.rand((13, n, w), generator=torch.Generator().manual_seed(98))
        assert_fp32_grade(model, p, x, k, gpu_device)


@pytest.mark.parametrize("n,w,k,d", [(127, 15, 30, 64), (96, 16, 20, 64), (33, 17, 20, 128)])
def test_windows_series_and_keys_entries_bit_for_bit(n, w, k, d, gpu_device):
    t = 1100
    model = random_params(n, w, k, d, seed=99)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    raw = torch.rand((n, t + w), generator=torch.Generator().manual_seed(100))
    x = raw.unfold(1, w, 1)[:, :t].permute(1, 0, 2).contiguous()
    dev_raw, dev_x = raw.to(gpu_device), x.to(gpu_device)
    gt = dev_raw[:, w:].t().contiguous()
    with torch.no_grad():
        plain = model.forward_into(dev_x, torch.empty((t, n), device=gpu_device))
        series = model.forward_series(dev_raw, 0, t)
        tail = model.forward_series(dev_raw, 41, t - 41)
        assert model.fused_keys_supported(False)
        keys = torch.zeros((n, t), dtype=torch.float64, device=gpu_device)
        keyed = model.forward_into(dev_x, torch.empty((t, n), device=gpu_device), keys=(gt, keys.data_ptr(), t))
        keys_s = torch.zeros((n, t), dtype=torch.float64, device=gpu_device)
        keyed_s = model.forward_series(dev_raw, 0, t, keys=(gt, keys_s.data_ptr(), t))
    torch.cuda.synchronize()
    assert torch.equal(series, plain) and torch.equal(tail, plain[41:])
    assert torch.equal(keyed, plain) and torch.equal(keyed_s, plain)
    want = (plain.double() - gt.double()).abs().t()
    assert torch.equal(keys, want) and torch.equal(keys_s, want)
    ref = gdn_oracle.forward(f64_params(p), x.double(), k, graph=model.learned_graph.cpu())["out"]
    err = float((plain.cpu().double() - ref).abs().max())
    assert err <= 2e-7 * max(1.0, float(ref.abs().max())), err


def test_planned_and_plan_less_launches_agree(gpu_device):
    """Both compute their constants with the same code; only the order of a lane's list slots differs (the plan
    orders them by LDS bank), which reorders the softmax sums: the relation holds to the bar either launch is held
    to against float64."""
    for n, w, k, d in ((127, 15, 30, 64), (127, 17, 30, 64), (64, 15, 63, 128)):
        model = random_params(n, w, k, d, seed=101).to(gpu_device).eval()
        x = torch.rand((29, n, w), generator=torch.Generator().manual_seed(102))
        planned, plain = planned_and_plain(model, x, gpu_device)
        scale = max(1.0, float(planned.abs().max()))
        diff = float((planned - plain).abs().max())
        print(f"planned vs plan-less: {diff:.3e} of scale {scale:.3f}")
        assert diff <= 2 * 2e-7 * scale, (diff, scale)


@pytest.mark.parametrize("d", [64, 128])
def test_every_workgroup_runs_several_windows_and_the_last_round_is_ragged(d, gpu_device):
    """More windows than three rounds of the largest grid the kernel takes (3 workgroups on each of at most 256 CUs,
    768), and not a multiple of it: the last round leaves most workgroups without a window.  A sample of the
    windows (the first, the last, a stride in between) is held against float64; every window is held against the
    same window computed in a small launch, bit for bit (a window's result does not depend on its launch)."""
    n, w, k = 127, 15, 30
    b = 3 * 768 + 131
    model = random_params(n, w, k, d, seed=103)
    p = {key: v.detach().clone() for key, v in model.state_dict().items()}
    model = model.to(gpu_device).eval()
    x = torch.rand((b, n, w), generator=torch.Generator().manual_seed(104))
    dev_x = x.to(gpu_device)
    with torch.no_grad():
        out = model.forward_into(dev_x, torch.empty((b, n), device=gpu_device))
        parts = torch.cat([model.forward_into(dev_x[i:i + 97].contiguous(), torch.empty((min(97, b - i), n), device=gpu_device))
                           for i in range(0, b, 97)])
    torch.cuda.synchronize()
    assert torch.equal(out, parts)
    pick = torch.cat([torch.arange(0, b, 61), torch.tensor([b - 1])])
    ref = gdn_oracle.forward(f64_params(p), x[pick].double(), k, graph=model.learned_graph.cpu())["out"]
    err = float((out.cpu()[pick].double() - ref).abs().max())
    bound = 2e-7 * max(1.0, float(ref.abs().max()))
    print(f"ragged multi-round launch: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)
