"""The fused dense forward with fp32 storage at w <= 16 keeps X^T fragments in registers from the ahi pass of M to the
alo pass and reads lin', the A operand of P1, from LDS (gdn_forward_dense.hip, DCfg::XKEEP / DCfg::BLDS).  `GDN.forward`
is held against the float64 oracle at the bar of tests/test_gpu_fused_dead_rows.py (2e-7 of the output scale) on one
shape per wave count and list length of the family, plus w = 17 (two window k-steps: code the change does not touch,
still routed); batches of 3 and 769 (a workgroup runs several windows: the resident fragments are rewritten per
window).  One case runs the same input twice in one process and wants the same bits."""
import pytest
import torch

from oracle import gdn_oracle
from test_gpu_forward_parity import random_params

pytestmark = pytest.mark.gpu

# (n, k, w): bench shape NT 4 SL 16 | NT 3, all 16 columns | NT 2 SL 8 | NT 1 | WK = 2
CASES = [(127, 30, 15), (96, 30, 16), (33, 12, 5), (20, 6, 8), (127, 30, 17)]
BATCHES = (3, 769)
D = 64


def reference_case(n, k, w, seed, dev):
    """(model on the device, windows [max batch, n, w], float64 reference [max batch, n]): computed once per case."""
    model = random_params(n, w, k, D, seed=seed)
    p = {key: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone())
         for key, v in model.state_dict().items()}
    model = model.to(dev).eval()
    x = torch.rand((max(BATCHES), n, w), generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        model(x[:1].to(dev), None)                       # the model learns its graph
    ref = gdn_oracle.forward(p, x.double(), k, graph=model.learned_graph.cpu())["out"]
    return model, x, ref


@pytest.mark.parametrize("n,k,w", CASES, ids=lambda v: str(v))
def test_forward_against_float64(n, k, w, gpu_device):
    model, x, ref = reference_case(n, k, w, 271, gpu_device)
    dev_x = x.to(gpu_device)
    with torch.no_grad():
        for b in BATCHES:
            got = model(dev_x[:b], None)
            torch.cuda.synchronize()
            err = float((got.cpu().double() - ref[:b]).abs().max())
            bound = 2e-7 * max(1.0, float(ref[:b].abs().max()))
            print(f"n={n} k={k} w={w} b={b}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (n, k, w, b, err, bound)


def test_same_input_twice_same_bits(gpu_device):
    n, k, w = 127, 30, 15
    model = random_params(n, w, k, D, seed=273).to(gpu_device).eval()
    x = torch.rand((769, n, w), generator=torch.Generator().manual_seed(274)).to(gpu_device)
    with torch.no_grad():
        first = model(x, None).clone()
        again = model(x, None)
    torch.cuda.synchronize()
    assert torch.equal(first, again)
