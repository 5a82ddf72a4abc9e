"""model.build_unet on the HIP path against the float64 twin (tests/unet_twin.py).

The bound. The error of 23 stacked layers is not derived; it is measured per precision from an emulation that runs the twin on
the CPU in float32 with the input and weight of every MFMA convolution rounded the way that precision rounds its operands
(fp32: not at all; bf16x3: to a hi + lo bf16 pair; bf16: to bf16). The HIP result must lie within 4 x that emulation's
distance from float64 (the factor covers a different summation order over K up to 9216: a random-walk difference, not a
different rounding model). Distances are max |difference| / max |float64 logits|.

Measured on an MI355X (emulation distance / HIP distance):
  B=2 32x32: fp32 1.23e-6 / 3.30e-6, bf16x3 2.58e-5 / 3.02e-5, bf16 1.66e-2 / 1.75e-2
  B=1 48x32: fp32 1.46e-6 / 3.00e-6, bf16x3 2.66e-5 / 3.48e-5, bf16 1.64e-2 / 1.48e-2
B=3 16x16 (a 1 x 1 bottleneck grid) and B=1 16x48 (1 x 3) run under the same bound; the test prints their distances.
"""
import functools

import pytest
import torch

from tests.memcheck import assert_same_bits
from tests.unet_twin import ROUNDING, make_case
from vit_ocm_wmsegmentation_amd import model as M

pytestmark = pytest.mark.gpu

SHAPES = {"b2_32x32": (2, 32, 32), "b1_48x32": (1, 48, 32),
          "b3_16x16": (3, 16, 16),  # the smallest image forward accepts: the bottleneck is a 1 x 1 grid
          "b1_16x48": (1, 16, 48)}  # a 1 x 3 bottleneck, 2 x 6 and 4 x 12 grids above it
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def _case(shape_name, seed=21):
    """(x float64, eval-mode float64 twin, float64 logits, {precision: emulation distance}) — computed once, never modified."""
    B, H, W = SHAPES[shape_name]
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    twin = make_case(seed, x)
    with torch.no_grad():
        ref = twin(x)
        twin32 = make_case(seed, x).float()
        scale = float(ref.abs().max())
        emu = {p: float((twin32(x.float(), rnd).double() - ref).abs().max()) / scale for p, rnd in ROUNDING.items()}
    return x, twin, ref, emu


def _net(twin, dev, precision):
    net = M.build_unet()
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in twin.state_dict().items()}, strict=True)
    net.precision = precision
    return net.to(dev).eval()


def _emu_dist(twin, x, ref, precision):
    """Distance from float64 of the float32 emulation of `precision` (module docstring) for this twin."""
    sd = {k: v.float() if v.is_floating_point() else v for k, v in twin.state_dict().items()}
    t32 = type(twin)().eval()
    t32.load_state_dict(sd)
    with torch.no_grad():
        return float((t32(x.float(), ROUNDING[precision]).double() - ref).abs().max() / ref.abs().max())


def _dist(got, ref):
    return float((got.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("precision", sorted(ROUNDING))
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_logits_against_the_float64_twin(dev, shape_name, precision):
    x, twin, ref, emu = _case(shape_name)
    net = _net(twin, dev, precision)
    out = net(x.float().to(dev))
    assert out.shape == ref.shape and out.dtype == torch.float32 and out.device.type == "cuda"
    d = _dist(out, ref)
    msg = f"{shape_name} {precision}: HIP distance {d:.3e}, emulation distance {emu[precision]:.3e}, bound {FACTOR * emu[precision]:.3e}"
    print(msg)
    assert d <= FACTOR * emu[precision], msg
    assert_same_bits(out, net(x.float().to(dev)), "run to run", ("image", "channel", "y", "x"))


def test_batch_independence(dev):
    """An image's logits are the same bits alone and as image 1 of a batch of 3."""
    x, twin, _, _ = _case("b2_32x32")
    net = _net(twin, dev, "bf16x3")
    g = torch.Generator().manual_seed(2)
    batch = torch.randn(3, 3, 32, 32, generator=g).to(dev)
    alone = net(batch[1:2])
    assert_same_bits(alone[0], net(batch)[1], "image alone vs image 1 of 3", ("channel", "y", "x"))


def test_no_stale_operand_cache(dev):
    """After load_state_dict of other weights and after an in-place change of one running_var the output follows."""
    x, twin, ref, emu = _case("b2_32x32")
    xd = x.float().to(dev)
    net = _net(twin, dev, "fp32")
    out0 = net(xd)
    # other weights: the twin of another seed (its running statistics were taken on the same input)
    twin2 = make_case(22, x)
    with torch.no_grad():
        ref2 = twin2(x)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in twin2.state_dict().items()}, strict=True)
    out1 = net(xd)
    d1 = _dist(out1, ref2)
    b1 = FACTOR * _emu_dist(twin2, x, ref2, "fp32")
    assert d1 <= b1, f"after load_state_dict: distance {d1:.3e} from the new weights' float64 logits (bound {b1:.3e})"
    assert _dist(out1, ref) > 1e-2
    # one running_var in place, on the module and on a copy of the twin
    with torch.no_grad():
        net.d4.conv.bn2.running_var.mul_(4.0)
        twin3 = make_case(22, x)
        twin3.d4.conv.bn2.running_var.mul_(4.0)
        ref3 = twin3(x)
    out2 = net(xd)
    d2 = _dist(out2, ref3)
    b2 = FACTOR * _emu_dist(twin3, x, ref3, "fp32")
    assert d2 <= b2, f"after running_var.mul_: distance {d2:.3e} from the changed float64 logits (bound {b2:.3e})"
    assert _dist(out2, ref2) > 1e-2
    assert not torch.equal(out0, out1)


def test_pgt_evaluate_usage(dev):
    """PGT.py: model.eval(); with torch.no_grad(): torch.sigmoid(model(x)) > 0.5 -> a (B, 1, H, W) mask."""
    x, twin, ref, _ = _case("b1_48x32")
    net = _net(twin, dev, "bf16x3")
    net.train()
    net.eval()
    with torch.no_grad():
        mask = torch.sigmoid(net(x.float().to(dev))) > 0.5
    assert mask.shape == (1, 1, 48, 32) and mask.dtype == torch.bool
    want = torch.sigmoid(ref) > 0.5
    sure = (ref.abs() > 1e-2 * ref.abs().max())  # pixels whose sign no rounding flips
    assert torch.equal(mask.cpu()[sure], want[sure])


def test_training_mode_is_refused(dev):
    x, twin, _, _ = _case("b2_32x32")
    net = _net(twin, dev, "bf16x3").train()
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        net(x.float().to(dev))
    with pytest.raises(RuntimeError, match="HIP device"):
        net.eval()(x.float())
