"""DINOHead on the HIP path (dino/vision_transformer.py, _DINOHeadTrain) against a float64 torch twin built from nn.Linear /
nn.GELU / F.normalize / nn.utils.weight_norm (tests/dino_ref.py TwinHead): the logits, every parameter gradient and the gradient of
the input rows, in the three precisions. Needs an MI355X.

Error measure: max |g - g64| / max |g64| per tensor. Limits: tests/test_linear_probing_train_gpu.py's ladder (fp32 2e-5, bf16x3
2e-4, bf16 3e-2)."""
import functools

import pytest
import torch

from tests import dino_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 3e-2}
SMALL = dict(in_dim=128, hidden_dim=128, bottleneck_dim=64, out_dim=96)
CASES = {
    "small": dict(SMALL, rows=5, nlayers=3, norm_last_layer=True),
    "small_g": dict(SMALL, rows=5, nlayers=3, norm_last_layer=False),
    "small_1": dict(SMALL, rows=5, nlayers=1, norm_last_layer=False),
    "small_2": dict(SMALL, rows=5, nlayers=2, norm_last_layer=True),
    "vits": dict(in_dim=384, hidden_dim=2048, bottleneck_dim=256, out_dim=4096, rows=20, nlayers=3, norm_last_layer=False),
}


def _kw(name):
    return {k: v for k, v in CASES[name].items() if k != "rows"}


def _inputs(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(17)
    return torch.randn(c["rows"], c["in_dim"], generator=g), torch.randn(c["rows"], c["out_dim"], generator=g)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(state dict, logits64, {parameter name | "x": grad64}) of the twin."""
    twin = R.TwinHead(**_kw(name))
    sd = R.fill_head(twin, seed=23, g_spread=0.1)
    twin = twin.double()
    x, G = _inputs(name)
    x64 = x.double().requires_grad_(True)
    out = twin(x64)
    out.backward(G.double())
    grads = {n: p.grad.clone() for n, p in twin.named_parameters() if p.grad is not None}
    grads["x"] = x64.grad.clone()
    return sd, out.detach(), grads


def _head(name, precision, dev):
    sd, _, _ = _reference(name)
    head = VT.DINOHead(**_kw(name))
    head.load_state_dict(sd, strict=True)
    head.precision = precision
    return head.to(dev).train()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_match_float64(dev, name, precision):
    _, out64, grads64 = _reference(name)
    head = _head(name, precision, dev)
    x, G = _inputs(name)
    xd = x.to(dev).requires_grad_(True)
    out = head(xd)
    assert out.grad_fn is not None and out.shape == out64.shape
    errs = {"logits": R.rel(out, out64)}
    out.backward(G.to(dev))
    got = {n: p.grad for n, p in head.named_parameters()}
    got["x"] = xd.grad
    assert {n for n, g in got.items() if g is not None} == set(grads64)  # weight_g has a gradient exactly when it trains
    for n, g64 in grads64.items():
        assert got[n].shape == g64.shape
        errs[n] = R.rel(got[n], g64)
    print(name, precision, {k: f"{v:.2e}" for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    assert errs[worst] <= TOL[precision], f"{worst}: {errs[worst]:.3e} > {TOL[precision]:.0e} ({errs})"
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        out.backward(G.to(dev))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["small_g", "small_1", "vits"])
def test_eval_forward_equals_training_forward(dev, name, precision):
    head = _head(name, precision, dev)
    x = _inputs(name)[0].to(dev)
    trained = head(x)
    assert trained.grad_fn is not None
    with torch.no_grad():
        assert_same_bits(head(x), trained.detach(), "no_grad forward")
    head.eval()
    plain = head(x)
    assert plain.grad_fn is None
    assert_same_bits(plain, trained.detach(), "eval forward")
    assert_same_bits(head(x.reshape(1, -1, x.shape[1])).reshape(plain.shape), plain, "leading axes are folded into rows")


def test_frozen_head_builds_no_graph_and_updates_are_seen(dev):
    head = _head("small_g", "bf16x3", dev)
    x = _inputs("small_g")[0].to(dev)
    before = head(x).detach()
    with torch.no_grad():
        head.last_layer.weight_g.mul_(2.0)  # through autograd's counting: the cached last layer is rebuilt
    assert R.rel(head(x), before.double() * 2) <= 1e-6
    for p in head.parameters():
        p.requires_grad_(False)
    assert head(x.requires_grad_(True)).grad_fn is None
