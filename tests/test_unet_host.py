"""build_unet without a GPU: the module tree and state_dict of the reference's model.py:227-320, the round trip with the test
twin, the refusals that need no device, the layer description every walk of the network reads, and the twin itself against a
module-free restatement."""
import pytest
import torch

from tests.unet_twin import UNetTwin, make_case, restated_forward
from vit_ocm_wmsegmentation_amd import model as M

# convolution_block instances of model.py:280-300: state_dict prefix, in channels, out channels
BLOCKS = [("e1.conv", 3, 64), ("e2.conv", 64, 128), ("e3.conv", 128, 256), ("e4.conv", 256, 512), ("b", 512, 1024),
          ("d1.conv", 1024, 512), ("d2.conv", 512, 256), ("d3.conv", 256, 128), ("d4.conv", 128, 64)]
# ConvTranspose2d(in, out, 2, stride=2) of the decoder blocks: weight (in, out, 2, 2)
UPS = [("d1.up", 1024, 512), ("d2.up", 512, 256), ("d3.up", 256, 128), ("d4.up", 128, 64)]


def expected_state_dict_shapes():
    want = {}
    for p, cin, cout in BLOCKS:
        want[f"{p}.conv1.weight"] = (cout, cin, 3, 3)
        want[f"{p}.conv1.bias"] = (cout,)
        want[f"{p}.conv2.weight"] = (cout, cout, 3, 3)
        want[f"{p}.conv2.bias"] = (cout,)
        for bn in ("bn1", "bn2"):
            want[f"{p}.{bn}.weight"] = (cout,)
            want[f"{p}.{bn}.bias"] = (cout,)
            want[f"{p}.{bn}.running_mean"] = (cout,)
            want[f"{p}.{bn}.running_var"] = (cout,)
            want[f"{p}.{bn}.num_batches_tracked"] = ()
    for p, cin, cout in UPS:
        want[f"{p}.weight"] = (cin, cout, 2, 2)
        want[f"{p}.bias"] = (cout,)
    want["outputs.weight"] = (1, 64, 1, 1)
    want["outputs.bias"] = (1,)
    return want


def test_state_dict_keys_and_shapes():
    net = M.build_unet()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    want = expected_state_dict_shapes()
    assert len(want) == 9 * 14 + 4 * 2 + 2
    assert got == want, set(got) ^ set(want)
    # the submodule classes carry the reference's names (PGT.py / unet.py only construct build_unet, checkpoints only keys)
    assert type(net.e1).__name__ == "encoder_block" and type(net.d1).__name__ == "decoder_block"
    assert type(net.b).__name__ == "convolution_block" and isinstance(net.e1.pool, torch.nn.MaxPool2d)
    assert isinstance(net.e1.conv.relu, torch.nn.ReLU)


def test_state_dict_round_trip_with_the_twin():
    torch.manual_seed(3)
    net, twin = M.build_unet(), UNetTwin()
    twin.load_state_dict(net.state_dict(), strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k]), k
    torch.manual_seed(4)
    other = UNetTwin()
    net.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k


def test_precision_attribute():
    net = M.build_unet()
    assert net.precision == "bf16x3"
    net.precision = "fp32"
    assert net.precision == "fp32"
    with pytest.raises(ValueError):
        net.precision = "fp16"
    assert "_precision" not in net.state_dict()


def test_refusals_need_no_device():
    net = M.build_unet()
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)"):  # a fresh module is in training mode
        net(torch.zeros(1, 3, 32, 32))
    net.eval()
    with pytest.raises(RuntimeError, match="H=40, W=32"):
        net(torch.zeros(1, 3, 40, 32))
    with pytest.raises(RuntimeError, match="H=32, W=24"):
        net(torch.zeros(1, 3, 32, 24))
    with pytest.raises(RuntimeError, match=r"\(B, 3, H, W\)"):
        net(torch.zeros(1, 1, 32, 32))
    with pytest.raises(RuntimeError, match=r"\(B, 3, H, W\)"):
        net(torch.zeros(3, 32, 32))
    with pytest.raises(RuntimeError, match="HIP device"):  # a CPU tensor of a valid shape: no CPU fallback
        net(torch.zeros(1, 3, 32, 32))
    net.e2.conv.bn1.train()
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        net(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("H,W", [(32, 32), (48, 32)])
def test_plan_describes_the_module_tree(H, W):
    net = M.build_unet()
    steps = [s for _, stage in M._unet_plan(H, W) for s in stage]
    convs = [s for s in steps if s.op == "conv"]
    assert [s.key for s in convs] == [f"{p}.conv{i}" for p, _, _ in BLOCKS for i in (1, 2)]  # forward order
    assert len(convs) == 18
    level = {"e1": 0, "e2": 1, "e3": 2, "e4": 3, "b": 4, "d1": 3, "d2": 2, "d3": 1, "d4": 0}
    for s in convs:
        cv, bn = net.get_submodule(s.key), net.get_submodule(s.bn)
        assert isinstance(cv, torch.nn.Conv2d) and (s.C, s.O) == (cv.in_channels, cv.out_channels), s.key
        assert isinstance(bn, torch.nn.BatchNorm2d) and bn.num_features == s.O, s.key
        assert s.bn + ".running_var" in net.state_dict() and s.bn.rsplit(".", 1)[0] == s.key.rsplit(".", 1)[0]
        lvl = level[s.key.split(".")[0]]
        assert s.grid == (H >> lvl, W >> lvl), s.key
        assert s.src.buf == "x" or s.src.ld == s.C, s.key  # every source of a 3x3 layer is dense
    assert [(s.key, s.C, s.O) for s in steps if s.op == "up"] == [(p, cin, cout) for p, cin, cout in UPS]
    assert [s.key for s in steps if s.op == "pool"] == ["e1.pool", "e2.pool", "e3.pool", "e4.pool"]
    assert steps[-1].op == "head" and (steps[-1].key, steps[-1].C, steps[-1].src.ld) == ("outputs", 64, 64)
    # every buffer is written by an earlier step than any step that reads it; the image is given
    written, writers = {"x"}, {}
    for s in steps:
        assert s.src.buf in written, f"{s.key} reads {s.src.buf} before it is written"
        if s.dst is not None:
            written.add(s.dst.buf)
            writers.setdefault(s.dst.buf, []).append(s)
    # torch.cat([up, skip], 1): each half of a 2 O-wide buffer has exactly one writer, at columns 0 and O
    cats = {b: w for b, w in writers.items() if b.endswith(".cat")}
    assert sorted(cats) == ["e1.cat", "e2.cat", "e3.cat", "e4.cat"]
    for (buf, w), O in zip(sorted(cats.items()), (64, 128, 256, 512)):
        assert [(s.op, s.dst.col, s.dst.ld, s.O) for s in w] == [("conv", O, 2 * O, O), ("up", 0, 2 * O, O)], buf
        readers = [(s.op, s.src.col, s.src.ld) for s in steps if s.src.buf == buf]
        assert readers == [("pool", O, 2 * O), ("conv", 0, 2 * O)], buf
    for buf, w in writers.items():  # every other buffer is dense and has one writer
        if buf not in cats:
            assert len(w) == 1 and (w[0].dst.col, w[0].dst.ld) == (0, w[0].O), buf


def test_twin_agrees_with_the_restatement():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 16, 16, generator=gen, dtype=torch.float64)
    twin = make_case(5, x)
    with torch.no_grad():
        got, want = twin(x), restated_forward(twin.state_dict(), x)
    assert got.shape == (2, 1, 16, 16)
    scale = float(want.abs().max())
    assert scale > 1e-3
    assert float((got - want).abs().max()) <= 1e-12 * scale
