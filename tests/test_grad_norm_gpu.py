"""utils.grad_norm / clip_grad_norm_ / get_grad_norm on the device (kernels_optim.hip). The norm against sqrt of the float64 sum of
squares: relative error <= 1.2e-7, two fp32 roundings (the sums are float64, only the final cast rounds to fp32). Clipped gradients
against float64 within tests/optim_cases.py's bound (yardstick: torch.nn.utils.clip_grad_norm_ in fp32 on the CPU, foreach=False).
Needs an MI355X."""
import math

import pytest
import torch
import torch.nn as nn

from tests import optim_cases as OC
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import utils as U

pytestmark = pytest.mark.gpu

SETS = ["small", "chunks", "many", "empty", "2d"]
NORM_RTOL = 1.2e-7


def _params(set_name, dev, seed=0):
    params, grads = OC.inputs(set_name, 1, seed=seed)
    ps = [nn.Parameter(p.to(dev)) for p in params]
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    return ps, grads[0]


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


@pytest.mark.parametrize("set_name", SETS)
def test_norm_matches_float64_and_repeats(dev, set_name):
    ps, grads = _params(set_name, dev)
    want = _norm64(grads)
    calls = [U.grad_norm(ps) for _ in range(5)]
    first = calls[0]
    assert first.dim() == 0 and first.dtype == torch.float32 and first.device.type == "cuda"
    err = abs(float(first) - want) / want
    print(f"{set_name}: norm {float(first)!r} float64 {want!r} relative error {err:.3e}")
    assert err <= NORM_RTOL
    for c in calls[1:]:
        assert_same_bits(c, first, "the norm on a repeated call")
    for p, g in zip(ps, grads):
        assert_same_bits(p.grad.cpu(), g, "grad_norm leaves the gradients alone")
    assert U.get_grad_norm(ps) == float(first) and isinstance(U.get_grad_norm(ps), float)
    assert U.get_grad_norm(ps[0]) == float(U.grad_norm([ps[0]]))  # a single tensor, as the reference accepts


def test_unaligned_gradient_gives_the_same_bits(dev):
    """The same values at a 16-byte aligned address and at element offset 1 of a buffer."""
    _, C = OC.limits()
    g = torch.randn(2 * C + 7, generator=torch.Generator().manual_seed(3))
    a, b = nn.Parameter(torch.zeros_like(g).to(dev)), nn.Parameter(torch.zeros_like(g).to(dev))
    a.grad = g.to(dev)
    b.grad = torch.cat([torch.zeros(1), g]).to(dev)[1:]
    assert a.grad.data_ptr() % 16 == 0 and b.grad.data_ptr() % 16 == 4
    assert_same_bits(U.grad_norm([a]), U.grad_norm([b]), "aligned vs unaligned")


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("where", ["above", "below"])
def test_clip_matches_float64(dev, set_name, where):
    """max_norm below the norm: the gradients are scaled, within the bound of the float64 result. max_norm above it: torch's
    coefficient clamps to exactly 1.0 and the gradients keep their bits."""
    ps, grads = _params(set_name, dev, seed=1)
    norm = _norm64(grads)
    max_norm = 0.37 * norm if where == "above" else 2.5 * norm  # the NORM is above / below max_norm

    def cpu(dtype):
        qs = [nn.Parameter(g.to(dtype).clone()) for g in grads]
        for q, g in zip(qs, grads):
            q.grad = g.to(dtype).clone()
        n = torch.nn.utils.clip_grad_norm_(qs, max_norm, foreach=False)
        return [dict(g=q.grad.double()) for q in qs], float(n)

    ref, n64 = cpu(torch.float64)
    yard, _ = cpu(torch.float32)
    got_norm = U.clip_grad_norm_(ps, max_norm)
    assert got_norm.dim() == 0 and got_norm.dtype == torch.float32 and got_norm.device.type == "cuda"
    err = abs(float(got_norm) - n64) / n64
    print(f"{set_name}/{where}: returned norm relative error {err:.3e}")
    assert err <= NORM_RTOL
    OC.check_against_reference([dict(g=p.grad.double().cpu()) for p in ps], ref, yard, f"clip {set_name}/{where}")
    if where == "below":
        for p, g in zip(ps, grads):
            assert_same_bits(p.grad.cpu(), g, "gradients under a coefficient of exactly 1.0")
    else:
        assert any(not torch.equal(p.grad.cpu(), g) for p, g in zip(ps, grads))


@pytest.mark.parametrize("poison", ["inf", "nan"])
def test_nonfinite_gradients_do_what_torch_does(dev, poison):
    """One inf / nan element: the same NaN / zero pattern as torch.nn.utils.clip_grad_norm_ on the CPU for the same input."""
    ps, grads = _params("small", dev, seed=2)
    grads = [g.clone() for g in grads]
    grads[4][100] = float(poison)
    ps[4].grad = grads[4].to(dev)
    qs = [nn.Parameter(g.clone()) for g in grads]
    for q, g in zip(qs, grads):
        q.grad = g.clone()
    want_norm = torch.nn.utils.clip_grad_norm_(qs, 1.0, foreach=False)
    got_norm = U.clip_grad_norm_(ps, 1.0)
    assert torch.isnan(got_norm).item() == torch.isnan(want_norm).item()
    assert torch.isinf(got_norm).item() == torch.isinf(want_norm).item()
    for p, q in zip(ps, qs):
        got = p.grad.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(q.grad))
        assert torch.equal(got == 0, q.grad == 0)
    with pytest.raises(RuntimeError, match="non-finite"):
        U.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


def test_surface(dev):
    none = [nn.Parameter(torch.zeros(3, device=dev)) for _ in range(2)]
    assert float(U.grad_norm(none)) == 0.0 and float(U.clip_grad_norm_(none, 1.0)) == 0.0 and U.get_grad_norm(none) == 0.0
    ps, _ = _params("small", dev)
    for fn in (lambda: U.clip_grad_norm_(ps, 1.0, norm_type=1), lambda: U.grad_norm(ps, norm_type=1),
               lambda: U.get_grad_norm(ps, norm_type=1), lambda: U.clip_grad_norm_(ps, 1.0, norm_type=float("inf"))):
        with pytest.raises(ValueError):
            fn()
    versions = [p.grad._version for p in ps]
    U.clip_grad_norm_(ps, 1e-3)
    assert all(p.grad._version > v for p, v in zip(ps, versions))
    # a non-contiguous gradient is made contiguous and clipped, not refused
    w = nn.Parameter(torch.zeros(5, 9, device=dev))
    g = torch.randn(9, 5, generator=torch.Generator().manual_seed(1))
    w.grad = g.to(dev).t()
    n = U.clip_grad_norm_([w], 0.5)
    want = g.t().double() * (0.5 / (float(g.double().norm()) + 1e-6))
    assert abs(float(n) - float(g.double().norm())) <= NORM_RTOL * float(g.double().norm())
    assert OC.rel_err(w.grad, want) <= OC.FLOOR
    d = nn.Parameter(torch.zeros(3, device=dev, dtype=torch.float64))
    d.grad = torch.ones_like(d)
    with pytest.raises(TypeError):
        U.grad_norm(ps + [d])


@pytest.mark.parametrize("error_if_nonfinite", [False, True])
def test_generator_of_parameters_is_clipped(dev, error_if_nonfinite):
    """model.parameters() is a generator, and that is how every training script calls clip_grad_norm_: it is walked once, with
    and without error_if_nonfinite, and the gradients come out scaled."""
    ps, grads = _params("chunks", dev, seed=4)
    norm = _norm64(grads)
    got = U.clip_grad_norm_((p for p in ps), 0.25 * norm, error_if_nonfinite=error_if_nonfinite)
    assert got.device.type == "cuda" and abs(float(got) - norm) <= NORM_RTOL * norm
    for p, g in zip(ps, grads):
        want = g.double() * (0.25 * norm / (norm + 1e-6))
        assert OC.rel_err(p.grad, want) <= OC.FLOOR
    after = U.get_grad_norm(p for p in ps)
    assert abs(after - 0.25 * norm) <= 1e-6 * norm
    assert float(U.grad_norm(p for p in ps)) == after


def test_norm_of_a_noncontiguous_gradient(dev):
    """grad_norm / get_grad_norm take a non-contiguous gradient as torch does, and leave it as it is; so does the
    error_if_nonfinite path of clip_grad_norm_, which then clips a contiguous copy."""
    w = nn.Parameter(torch.zeros(5, 9, device=dev))
    g = torch.randn(9, 5, generator=torch.Generator().manual_seed(2))
    w.grad = g.to(dev).t()
    held = w.grad
    want = float(g.double().norm())
    assert abs(float(U.grad_norm([w])) - want) <= NORM_RTOL * want
    assert abs(U.get_grad_norm(w) - want) <= NORM_RTOL * want
    assert w.grad is held and not w.grad.is_contiguous()
    assert_same_bits(w.grad.cpu(), g.t(), "grad_norm leaves the gradient alone")
    n = U.clip_grad_norm_(iter([w]), 0.5, error_if_nonfinite=True)
    assert abs(float(n) - want) <= NORM_RTOL * want
    assert OC.rel_err(w.grad, g.t().double() * (0.5 / (want + 1e-6))) <= OC.FLOOR
