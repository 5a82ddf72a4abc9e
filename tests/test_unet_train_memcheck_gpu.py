"""Memory behaviour of one training step of build_unet (tests/memcheck.py): every activation and gradient buffer of the forward
and the backward comes from NaN-poisoned, guard-banded memory through the module's allocator seam; every guard band stays intact,
the gradients are finite, and they are bit for bit the gradients of a plain run."""
import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from tests.test_unet_train_gpu import _case, _grads, _hip_step, _net

pytestmark = pytest.mark.gpu


def test_training_step_on_poisoned_buffers(dev):
    c = _case("b2_32x32")
    plain = _net(c, dev, "bf16x3")
    out0 = _hip_step(plain, c, dev).detach().clone()
    want = _grads(plain)
    held = []

    def poisoned(shape, device):
        n = 1
        for s in shape:
            n *= s
        gd = Guarded(n * 4, device, pattern="nan")
        held.append(gd)
        return gd.payload(torch.float32, tuple(shape))

    net = _net(c, dev, "bf16x3")
    net.__dict__["_alloc"] = poisoned
    out = _hip_step(net, c, dev)
    torch.cuda.synchronize()
    forward_buffers = 4 * 5 + 4 + 4 * 4 + 6  # per level y1, t, y2, [up | skip], pooled; the bottleneck's four; per decoder level
    #                                          y1, t, y2, z; the im2col operand of the six layers split-bf16 runs as a composition
    assert len(held) > forward_buffers  # and the backward's gradient buffers and im2col operands
    for i, gd in enumerate(held):
        assert gd.check() is None, f"buffer {i} of {len(held)}: {gd.check()}"
    got = _grads(net)
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    assert_same_bits(out.detach(), out0, "logits on poisoned buffers", ("image", "channel", "y", "x"))
    for k in want:
        assert_same_bits(got[k], want[k], f"{k}: poisoned buffers vs plain run")
    for (k, a), (_, b) in zip(net.named_buffers(), plain.named_buffers()):
        assert_same_bits(a, b, f"{k}: running statistics")
