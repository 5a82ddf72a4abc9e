"""optimizer.AdamW / Adam / SGD on the device (kernels_optim.hip) against torch itself in float64 on the CPU: the same optimizer
class on .double() copies of the same parameters and gradients. Yardstick: torch's own fp32 CPU step (foreach=False) on the same
inputs. Error measure max |x - x64| / max |x64| per tensor; bound max(1e-6, 4 x the yardstick's error on that tensor), computed per
case (tests/optim_cases.py). Needs an MI355X."""
import copy
import types
from functools import partial

import pytest
import torch
import torch.nn as nn

from tests import optim_cases as OC
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import optimizer as OPT

pytestmark = pytest.mark.gpu

CONFIGS = {
    "adamw": ("AdamW", dict(lr=1e-3, weight_decay=0.05)),
    "adam": ("Adam", dict(lr=1e-3, weight_decay=0.0)),
    "adam_l2": ("Adam", dict(lr=1e-3, weight_decay=0.01)),
    "sgd_nesterov": ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)),
    "sgd_plain": ("SGD", dict(lr=1e-2, momentum=0.0)),
}
STEPS = 10


def _ours(cls):
    return getattr(OPT, cls)


def _run_ours(cls, kwargs, params, grads, dev, lrs=None, snap_at=(1,), kept=False, stream=None):
    """Our class on device copies. Gradients get new addresses on every step (the old ones are held alive while the new ones are
    allocated) unless `kept`, which copies into the first step's tensors."""
    ps = [nn.Parameter(p.to(dev)) for p in params]
    opt = _ours(cls)(ps, **kwargs)
    snaps, alive = {}, []
    for i, gs in enumerate(grads, 1):
        if lrs is not None:
            for grp in opt.param_groups:
                grp["lr"] = lrs[i - 1]
        for p, g in zip(ps, gs):
            if kept and p.grad is not None:
                p.grad.copy_(g)
            else:
                alive.append(p.grad)
                p.grad = g.to(dev)
        if stream is None:
            opt.step()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                opt.step()
            torch.cuda.current_stream().wait_stream(stream)
        if i in snap_at:
            snaps[i] = OC.snapshot(opt, ps)
    return snaps, opt, ps


@pytest.mark.parametrize("set_name", ["small", "chunks", "many", "empty", "2d"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_steps_match_float64(dev, config, set_name):
    cls, kwargs = CONFIGS[config]
    params, grads = OC.inputs(set_name, STEPS)
    at = (1, STEPS)
    ref = OC.run_cpu(cls, kwargs, params, grads, torch.float64, snap_at=at)
    yard = OC.run_cpu(cls, kwargs, params, grads, torch.float32, snap_at=at)
    got, opt, ps = _run_ours(cls, kwargs, params, grads, dev, snap_at=at)
    for s in at:
        OC.check_against_reference(got[s], ref[s], yard[s], f"{config}/{set_name} step {s}")
    for p in ps:  # torch's state: `step` a CPU fp32 scalar for the Adam rules, none for SGD
        st = opt.state.get(p, {})
        if cls == "SGD":
            assert "step" not in st
        else:
            assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == STEPS


@pytest.mark.parametrize("config", ["adamw", "sgd_nesterov"])
def test_unaligned_view_and_noncontiguous_grad(dev, config):
    """A parameter that is a view at element offset 1 of a larger buffer (not 16-byte aligned): stepped right, the buffer's other
    elements unchanged bit for bit. A 2-D parameter with a transposed (non-contiguous) gradient beside it."""
    cls, kwargs = CONFIGS[config]
    _, C = OC.limits()
    n = C + 6
    gen = torch.Generator().manual_seed(7)
    buf = torch.randn(n + 3, generator=gen)
    w = torch.randn(33, 17, generator=gen)
    grads = [[torch.randn(n, generator=gen) * 1e-3, torch.randn(17, 33, generator=gen).t()] for _ in range(3)]
    assert not grads[0][1].is_contiguous()
    params = [buf[1:1 + n], w]
    ref = OC.run_cpu(cls, kwargs, params, grads, torch.float64, snap_at=(3,))
    yard = OC.run_cpu(cls, kwargs, params, grads, torch.float32, snap_at=(3,))
    dbuf = buf.to(dev)
    ps = [nn.Parameter(dbuf[1:1 + n]), nn.Parameter(w.to(dev))]
    assert ps[0].data_ptr() % 16 == 4 and ps[0].data_ptr() == dbuf.data_ptr() + 4
    opt = _ours(cls)(ps, **kwargs)
    for gs in grads:
        ps[0].grad = gs[0].to(dev)
        ps[1].grad = gs[1].t().contiguous().to(dev).t()
        assert not ps[1].grad.is_contiguous()
        opt.step()
    OC.check_against_reference(OC.snapshot(opt, ps), ref[3], yard[3], f"{config}/view")
    assert_same_bits(dbuf[:1].cpu(), buf[:1], "element before the view")
    assert_same_bits(dbuf[1 + n:].cpu(), buf[1 + n:], "elements after the view")
    assert_same_bits(dbuf[1:1 + n], ps[0].detach(), "the view is the buffer")


def test_param_groups_and_lr_changes(dev):
    """Two groups with different lr / weight_decay, lr changed between steps through param_groups."""
    params, grads = OC.inputs("small", 4, seed=1)
    lrs = [(1e-3, 5e-3), (2e-3, 1e-3), (5e-4, 5e-4), (1e-3, 2e-3)]

    def run(cls_of, to, dtype, **extra):
        ps = [nn.Parameter(p.to(to, dtype).clone()) for p in params]
        opt = cls_of([dict(params=ps[:2], lr=1e-3, weight_decay=0.1), dict(params=ps[2:], lr=5e-3, weight_decay=0.0)],
                     betas=(0.8, 0.99), **extra)
        for gs, lr in zip(grads, lrs):
            opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr
            for p, g in zip(ps, gs):
                p.grad = g.to(to, dtype)
            opt.step()
        return OC.snapshot(opt, ps)

    OC.check_against_reference(run(OPT.AdamW, dev, torch.float32), run(torch.optim.AdamW, "cpu", torch.float64),
                               run(torch.optim.AdamW, "cpu", torch.float32, foreach=False), "groups")


@pytest.mark.parametrize("config", ["adamw", "sgd_nesterov"])
def test_grad_none_is_skipped(dev, config):
    """A parameter without a gradient is skipped: no state, no step counted, bits unchanged. When it gets a gradient later its
    step starts at 1 while the others' continue."""
    cls, kwargs = CONFIGS[config]
    params, grads = OC.inputs("small", 4, seed=2)
    late = 2  # index of the parameter whose first two gradients are None

    def run(cls_of, to, dtype, **extra):
        ps = [nn.Parameter(p.to(to, dtype).clone()) for p in params]
        opt = cls_of(ps, **kwargs, **extra)
        for i, gs in enumerate(grads):
            for j, (p, g) in enumerate(zip(ps, gs)):
                p.grad = None if (j == late and i < 2) else g.to(to, dtype)
            opt.step()
            if i == 1 and to != "cpu":
                assert len(opt.state.get(ps[late], {})) == 0
                assert_same_bits(ps[late].detach().cpu(), params[late], "the skipped parameter")
        return OC.snapshot(opt, ps), opt, ps

    got, opt, ps = run(_ours(cls), dev, torch.float32)
    ref = run(OC.torch_class(cls), "cpu", torch.float64)[0]
    yard = run(OC.torch_class(cls), "cpu", torch.float32, foreach=False)[0]
    OC.check_against_reference(got, ref, yard, f"{config}/grad None")
    if cls != "SGD":
        assert [float(opt.state[p]["step"]) for p in ps] == [2.0 if j == late else 4.0 for j in range(len(ps))]


def test_adam_l2_leaves_grad_bits(dev):
    cls, kwargs = CONFIGS["adam_l2"]
    params, grads = OC.inputs("chunks", 1, seed=3)
    ps = [nn.Parameter(p.to(dev)) for p in params]
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt = OPT.Adam(ps, **kwargs)
    versions = [p._version for p in ps]
    opt.step()
    for p, g, v in zip(ps, grads[0], versions):
        assert_same_bits(p.grad.cpu(), g, "p.grad after an Adam step with L2 decay")
        assert p._version > v  # the raw kernel write is made visible to every (data_ptr, _version) cache


@pytest.mark.parametrize("config", ["adamw", "sgd_nesterov"])
def test_kept_addresses_side_stream_and_repeatability(dev, config):
    cls, kwargs = CONFIGS[config]
    params, grads = OC.inputs("chunks", 3, seed=4)
    ref = OC.run_cpu(cls, kwargs, params, grads, torch.float64, snap_at=(3,))[3]
    yard = OC.run_cpu(cls, kwargs, params, grads, torch.float32, snap_at=(3,))[3]
    new = _run_ours(cls, kwargs, params, grads, dev, snap_at=(3,))[0][3]
    kept = _run_ours(cls, kwargs, params, grads, dev, snap_at=(3,), kept=True)[0][3]
    side = _run_ours(cls, kwargs, params, grads, dev, snap_at=(3,), stream=torch.cuda.Stream(device=dev))[0][3]
    OC.check_against_reference(new, ref, yard, f"{config}/new addresses")
    OC.check_against_reference(kept, ref, yard, f"{config}/kept addresses")
    OC.check_against_reference(side, ref, yard, f"{config}/side stream")
    for other, what in ((kept, "kept addresses"), (side, "side stream")):  # the same inputs give the same bits
        for i, (a, b) in enumerate(zip(new, other)):
            for k in a:
                assert_same_bits(a[k], b[k], f"{what}: tensor {i} {k}")


@pytest.mark.parametrize("how", ["assign", "delete"])
@pytest.mark.parametrize("config", ["adamw", "sgd_nesterov"])
def test_state_reset_by_hand_is_followed(dev, config, how):
    """`opt.state[p] = {}` and `del opt.state[p]` between steps restart that parameter's state, as they do in torch: the next step
    builds new moments and a new count in the dict that optimizer.state holds, not in the one it held before."""
    cls, kwargs = CONFIGS[config]
    params, grads = OC.inputs("small", 4, seed=6)
    victim = 4

    def run(cls_of, to, dtype, **extra):
        ps = [nn.Parameter(p.to(to, dtype).clone()) for p in params]
        opt = cls_of(ps, **kwargs, **extra)
        for i, gs in enumerate(grads):
            if i == 2:
                if how == "assign":
                    opt.state[ps[victim]] = {}
                else:
                    del opt.state[ps[victim]]
            for p, g in zip(ps, gs):
                p.grad = g.to(to, dtype)
            opt.step()
        return OC.snapshot(opt, ps), opt, ps

    got, opt, ps = run(_ours(cls), dev, torch.float32)
    ref = run(OC.torch_class(cls), "cpu", torch.float64)[0]
    yard = run(OC.torch_class(cls), "cpu", torch.float32, foreach=False)[0]
    OC.check_against_reference(got, ref, yard, f"{config}/state {how}")
    if cls != "SGD":
        assert [float(opt.state[p]["step"]) for p in ps] == [2.0 if j == victim else 4.0 for j in range(len(ps))]
        assert float(opt.state_dict()["state"][victim]["step"]) == 2.0


def _finetune_model(dev):
    from tests.helpers import CASES
    from vit_ocm_wmsegmentation_amd import model as M
    from vit_ocm_wmsegmentation_amd import synth
    c = CASES["tiny_p8"]
    # the fine-tuning encoder keeps the 224^2 position table and interpolates it (tests/test_finetune_train_gpu.py)
    sd = synth.synth_state_dict(c["dim"], c["depth"], c["patch"], seed=c["seed"], variant=c["variant"], img_size=224)
    enc = M.VisionTransformerForFinetune(patch_size=c["patch"], embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"],
                                         mlp_ratio=4, img_size=[c["img_size"]], qkv_bias=True,
                                         norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    assert not enc.load_state_dict(sd, strict=True).missing_keys
    enc.enable_finetune(True)
    return enc.to(dev)


def test_next_forward_sees_the_stepped_weights(dev):
    """The tiny_p8 VisionTransformer after one backward and one step: its output equals, bit for bit, the output of a fresh
    module loaded with its state_dict(). The package's operand caches key on (data_ptr, _version): without the version bump after
    the launch the stepped module would still run its previous weights."""
    from tests.helpers import CASES, case_inputs
    x = case_inputs(CASES["tiny_p8"])[0].to(dev)
    enc = _finetune_model(dev).train()
    opt = OPT.AdamW(enc.parameters(), lr=1e-2, weight_decay=0.05)
    with torch.no_grad():
        before = enc(x)  # the inference engine has uploaded the weights it will compare (data_ptr, _version) against
    enc(x).square().mean().backward()
    versions = {n: p._version for n, p in enc.named_parameters() if p.grad is not None}
    assert versions
    opt.step()
    for n, p in enc.named_parameters():
        if n in versions:
            assert p._version > versions[n], n
    with torch.no_grad():
        after = enc(x)
    fresh = _finetune_model(dev).train()
    fresh.load_state_dict(enc.state_dict())
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(after, before)
    assert_same_bits(after, want, "forward after step() vs a fresh module with the same state_dict")


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_state_dict_exchange(dev, direction):
    """3 steps in one class, state_dict() into the other, 1 more step each on the same gradient: both within the bound of the
    float64 twin's fourth step. The `step` entry is a CPU fp32 tensor on both sides."""
    kwargs = dict(lr=1e-3, weight_decay=0.05)
    params, grads = OC.inputs("small", 4, seed=5)
    ref = OC.run_cpu("AdamW", kwargs, params, grads, torch.float64, snap_at=(4,))[4]
    yard = OC.run_cpu("AdamW", kwargs, params, grads, torch.float32, snap_at=(4,))[4]
    first, second = (OPT.AdamW, torch.optim.AdamW) if direction == "ours_to_torch" else (torch.optim.AdamW, OPT.AdamW)
    ps_a = [nn.Parameter(p.to(dev)) for p in params]
    a = first(ps_a, **kwargs)
    for gs in grads[:3]:
        for p, g in zip(ps_a, gs):
            p.grad = g.to(dev)
        a.step()
    sd = copy.deepcopy(a.state_dict())  # load_state_dict keeps the tensors it is given: the two must not share moments
    for st in sd["state"].values():
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 3.0
    ps_b = [nn.Parameter(p.detach().clone()) for p in ps_a]
    b = second(ps_b, **kwargs)
    b.load_state_dict(sd)
    for opt, ps in ((a, ps_a), (b, ps_b)):
        for p, g in zip(ps, grads[3]):
            p.grad = g.to(dev)
        opt.step()
        name = "ours" if isinstance(opt, OPT.AdamW) else "torch"
        OC.check_against_reference(OC.snapshot(opt, ps), ref, yard, f"{direction}: {name} after the exchange")
        assert all(float(opt.state[p]["step"]) == 4.0 and opt.state[p]["step"].device.type == "cpu" for p in ps)


def test_mim_loop(dev):
    """One loop in the shape of mim.py on the smallest geometry of tests/test_mim_train_gpu.py: build_pretrain_optimizer,
    clip_grad_norm_ (config.py's CLIP_GRAD = 5.0), 3 steps with a changing lr. The loss falls, and the parameters stay within the
    bound of the same loop with torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ on the device (foreach=False). Yardstick, measured
    here: the difference between torch's foreach=True and foreach=False runs of that loop, times 4, floor 1e-6."""
    import logging

    from tests import test_mim_train_gpu as MT
    from vit_ocm_wmsegmentation_amd import utils as U
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(
        BASE_LR=1e-4, WEIGHT_DECAY=0.05, OPTIMIZER=types.SimpleNamespace(NAME="adamw", EPS=1e-8, BETAS=(0.9, 0.999), MOMENTUM=0.9)))
    lrs = [1e-4, 8e-5, 5e-5]
    logger = logging.getLogger("test_mim_loop")

    def loop(kind):
        mim, x, mask = MT._model("wrap_p8_64", "fp32", dev)
        if kind == "ours":
            opt = OPT.build_pretrain_optimizer(cfg, mim, logger)
            assert isinstance(opt, OPT.AdamW)
            clip = U.clip_grad_norm_
        else:
            groups = OPT.get_pretrain_param_groups(mim, logger, mim.no_weight_decay(), mim.no_weight_decay_keywords())
            opt = torch.optim.AdamW(groups, eps=1e-8, betas=(0.9, 0.999), lr=1e-4, weight_decay=0.05, foreach=kind == "foreach")
            clip = partial(torch.nn.utils.clip_grad_norm_, foreach=kind == "foreach")
        losses = []
        for lr in lrs + [None]:
            loss, _, _ = mim(x, mask)
            losses.append(float(loss.detach()))
            if lr is None:
                break
            for grp in opt.param_groups:
                grp["lr"] = lr
            opt.zero_grad()
            loss.backward()
            clip(mim.parameters(), 5.0)
            opt.step()
        return losses, {n: p.detach().double().cpu() for n, p in mim.named_parameters()}

    losses, ours = loop("ours")
    _, single = loop("single")
    _, foreach = loop("foreach")
    print("losses", losses)
    assert losses[-1] < losses[0], losses
    bad = []
    for n in single:
        e, ey = OC.rel_err(ours[n], single[n]), OC.rel_err(foreach[n], single[n])
        bound = max(OC.FLOOR, 4 * ey)
        print(f"mim loop {n}: err {e:.3e} yardstick {ey:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((n, e, bound))
    assert not bad, bad
