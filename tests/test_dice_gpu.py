"""utils.DiceLoss on the HIP path (kernels_train.hip: dice_partial_kernel / dice_finish_kernel / dice_bwd_kernel) against the
reference's formula (utils.py:410-424) evaluated in float64. Needs an MI355X.

Error measure: max |v - v64| / max |v64| per tensor (the loss is a tensor of one element). Bound: the larger of 1e-6 and 4 x
the error that torch's own fp32 eager evaluation of the same formula (forward and autograd backward, on the same device and
the same inputs) shows against float64 — computed here, per case. Every figure is printed before it is asserted."""
import pytest
import torch

from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import utils as U

pytestmark = pytest.mark.gpu

SPAN = 4096  # elements one workgroup sums (dice_plan: counts up to 1024 spans)
COUNTS = [1, 3, 4, 255, 4097, 3 * 384 * 384, 3 * SPAN + 5]  # the last: odd, above a workgroup's span, ends mid-vector
TARGETS = ["binary", "soft", "zeros", "ones"]


def _formula(x, t, smooth=1):
    p = torch.sigmoid(x).reshape(-1)  # (the reference's view(-1), for non-contiguous inputs too)
    t = t.reshape(-1)
    inter = (p * t).sum()
    return 1 - (2. * inter + smooth) / (p.sum() + t.sum() + smooth)


def _inputs(count, kind, dev):
    g = torch.Generator().manual_seed(count * 7 + TARGETS.index(kind))
    x = (torch.randn(count, generator=g) * 6).clamp_(-30, 30)
    x[::5] = x[::5].sign() * 30 * torch.rand(x[::5].shape, generator=g)  # a fifth of the logits spread up to |x| = 30
    if count >= 4:
        x[0], x[-1] = 30.0, -30.0
    t = {"binary": lambda: (torch.rand(count, generator=g) < 0.4).float(), "soft": lambda: torch.rand(count, generator=g),
         "zeros": lambda: torch.zeros(count), "ones": lambda: torch.ones(count)}[kind]()
    return x.to(dev), t.to(dev)


def _rel(v, ref):
    return float((v.detach().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _with_grad(fn, x, t, dtype):
    leaf = x.detach().to(dtype).requires_grad_(True)
    loss = fn(leaf, t.to(dtype))
    loss.backward()
    return loss.detach(), leaf.grad


@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("count", COUNTS)
def test_loss_and_gradient_match_float64(dev, count, kind):
    x, t = _inputs(count, kind, dev)
    loss64, g64 = _with_grad(_formula, x, t, torch.float64)
    eager, geager = _with_grad(_formula, x, t, torch.float32)
    loss, grad = _with_grad(U.DiceLoss(), x, t, torch.float32)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == x.shape
    e_loss, e_grad = _rel(loss, loss64), _rel(grad, g64)
    y_loss, y_grad = _rel(eager, loss64), _rel(geager, g64)
    print(f"GPUTEST dice count={count} {kind}: loss {e_loss:.3e} (eager {y_loss:.3e}), dlogits {e_grad:.3e} (eager {y_grad:.3e})")
    assert e_loss <= max(1e-6, 4 * y_loss), f"loss {e_loss:.3e}, eager fp32 {y_loss:.3e}"
    assert e_grad <= max(1e-6, 4 * y_grad), f"dlogits {e_grad:.3e}, eager fp32 {y_grad:.3e}"


@pytest.mark.parametrize("count", [3, 4097, 3 * 384 * 384])
def test_same_bits_on_repeated_calls_and_under_no_grad(dev, count):
    x, t = _inputs(count, "binary", dev)
    first = _with_grad(U.DiceLoss(), x, t, torch.float32)
    for rep in range(4):  # five calls in all
        again = _with_grad(U.DiceLoss(), x, t, torch.float32)
        assert_same_bits(again[0], first[0], f"loss, call {rep + 2}")
        assert_same_bits(again[1], first[1], f"dlogits, call {rep + 2}")
    with torch.no_grad():  # finetune.py's evaluate()
        quiet = U.DiceLoss()(x, t)
    assert quiet.grad_fn is None and not quiet.requires_grad
    assert_same_bits(quiet, first[0], "loss under no_grad")


def test_other_dtypes_layouts_smooth_and_upstream_gradient(dev):
    """Non-contiguous and non-fp32 inputs are made contiguous fp32 first; the gradient comes back in the input's own dtype and
    shape; `smooth` and the upstream gradient are honoured."""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(2, 1, 24, 40, generator=g).to(dev)
    t = (torch.rand(2, 1, 40, 24, generator=g) < 0.5).to(dev)  # a bool mask
    x16 = base.to(torch.bfloat16).transpose(2, 3).requires_grad_(True)  # (2, 1, 40, 24), non-contiguous, bf16
    assert not x16.is_contiguous()
    loss = U.DiceLoss()(x16, t, smooth=0.5)
    (3.0 * loss).backward()
    x64 = x16.detach().double().requires_grad_(True)
    want = _formula(x64, t.double(), smooth=0.5)
    (3.0 * want).backward()
    assert loss.dtype == torch.float32 and x16.grad.dtype == torch.bfloat16 and x16.grad.shape == x16.shape
    assert _rel(loss, want.detach()) <= 1e-6
    assert _rel(x16.grad, x64.grad) <= 2 ** -8  # one rounding of the fp32 gradient to bf16
    with pytest.raises(ValueError, match="same, non-zero number of elements"):
        U.DiceLoss()(base, t[:1])
