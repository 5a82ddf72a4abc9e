"""ocm_op_mim_l1_loss, ocm_op_swin_mask_tokens and its backward on the device, against the numpy restatement of
tests/swin_mim_ref.py and float64 sums. Needs an MI355X.

What is compared how:
  rec    bit-equal to ocm_op_pixel_shuffle;
  dlin   bit-equal to the restatement: every element is +scale, -scale or 0 with scale = (float)(1 / ((count + 1e-5) c)), so there
         is no rounding to allow for. Exact ties rec == x are planted inside and outside the mask;
  loss   within one fp32 ulp of the float64 value: the operator sums exact float64 differences and rounds once (half an ulp),
         the second half covers the float64 sum's own order;
  d_mask_token  the same bound against a float64 column sum (float64 partials, rounded once)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import swin_mim_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if v else float(np.finfo(np.float32).tiny)


def _inputs(B, hp, c, s, p, seed, kind):
    """lin, x, mask (numpy) with ties planted; kind: "random" (about 60 % masked), "all", "none"."""
    rng = np.random.default_rng(seed)
    S = hp * s
    lin = rng.standard_normal((B * hp * hp, c * s * s)).astype(np.float32)
    x = rng.standard_normal((B, c, S, S)).astype(np.float32)
    side = S // p
    mask = {"random": (rng.uniform(size=(B, side, side)) < 0.6), "all": np.ones((B, side, side), bool),
            "none": np.zeros((B, side, side), bool)}[kind].astype(np.uint8)
    if kind == "random":
        mask[0, 0, 0], mask[-1, -1, -1] = 3, 0  # any nonzero byte masks
    rec = R.shuffle(lin, B, hp, hp, c, s)
    x[0, 0, 0, 0] = rec[0, 0, 0, 0]  # a tie inside the mask (random, all) ...
    x[-1, -1, -1, -1] = rec[-1, -1, -1, -1]  # ... and one outside it (random, none)
    return lin, x, mask


def _run(lib, dev, lin, x, mask, B, hp, c, s, p, want=("rec", "dlin", "loss")):
    tl, tx, tm = (torch.from_numpy(a).to(dev) for a in (lin, x, mask))
    out = {"rec": torch.full(x.shape, float("nan"), device=dev), "dlin": torch.full(lin.shape, float("nan"), device=dev),
           "loss": torch.full((1,), float("nan"), device=dev)}
    nbytes = lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, c, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = {k: (out[k].data_ptr() if k in want else None) for k in out}
    rc = lib.ocm_op_mim_l1_loss(tl.data_ptr(), tx.data_ptr(), tm.data_ptr(), B, hp, hp, c, s, p, ptr["rec"], ptr["dlin"],
                                ptr["loss"], ws.data_ptr(), nbytes, _s())
    assert rc == 0, lib.ocm_last_error()
    torch.cuda.synchronize()
    return out, tl


def _check(lib, dev, B, hp, c, s, p, seed, kind):
    lin, x, mask = _inputs(B, hp, c, s, p, seed, kind)
    out, tl = _run(lib, dev, lin, x, mask, B, hp, c, s, p)
    rec, dlin, loss, scale = R.mim_l1_ref(lin, x, mask, B, hp, hp, c, s, p)
    what = f"mim_l1_loss B={B} hp={hp} c={c} s={s} p={p} mask {kind}"
    shuf = torch.empty_like(out["rec"])
    assert lib.ocm_op_pixel_shuffle(tl.data_ptr(), shuf.data_ptr(), B, hp, hp, c, s, _s()) == 0
    assert_same_bits(out["rec"], shuf, what + ": rec vs ocm_op_pixel_shuffle")
    assert_same_bits(out["rec"].cpu(), torch.from_numpy(rec), what + ": rec")
    assert_same_bits(out["dlin"].cpu(), torch.from_numpy(dlin), what + ": dlin")
    got = float(out["loss"][0])
    assert abs(got - loss) <= _ulp32(loss), (what, got, loss)
    if not mask.any():  # "none", and a one-entry random mask whose only byte is the planted zero
        assert got == 0.0 and not bool(out["dlin"].any())
    else:
        assert float(out["dlin"].abs().max()) == float(scale)
        assert mask[0, 0, 0] == 0 or float(out["dlin"][0, 0]) == 0.0  # the masked tie
    return got


@pytest.mark.parametrize("s,p", [(32, 4), (8, 4), (8, 8), (4, 4)])
def test_mim_l1_loss_grid(lib, dev, s, p):
    """c in {1, 3} x hp = wp in {1, 3, 6} x B in {1, 3}, random masks; all-true and all-false masks at the middle size."""
    seed = 1000 * s + p
    for c, hp, B in itertools.product((1, 3), (1, 3, 6), (1, 3)):
        seed += 1
        _check(lib, dev, B, hp, c, s, p, seed, "random")
    for kind in ("all", "none"):
        _check(lib, dev, 3, 3, 3, s, p, seed + 7, kind)


def test_mim_l1_loss_every_subset_of_outputs(lib, dev):
    """A null output is skipped and the others keep their bits; the skipped buffers are not touched."""
    B, hp, c, s, p = 2, 3, 3, 8, 4
    lin, x, mask = _inputs(B, hp, c, s, p, 77, "random")
    full, _ = _run(lib, dev, lin, x, mask, B, hp, c, s, p)
    names = ("rec", "dlin", "loss")
    for n in range(len(names) + 1):
        for want in itertools.combinations(names, n):
            out, _ = _run(lib, dev, lin, x, mask, B, hp, c, s, p, want)
            for k in names:
                if k in want:
                    assert_same_bits(out[k], full[k], f"{k} with outputs {want}")
                else:
                    assert bool(torch.isnan(out[k]).all()), f"{k} was written though null was passed ({want})"


def test_mim_l1_loss_many_partials_rerun(lib, dev):
    """B = 4, c = 3, S = 192, s = 32: 432 workgroup partials, more than the finalise workgroup's 256 lanes hold in one round;
    two runs give the same bits."""
    B, hp, c, s, p = 4, 6, 3, 32, 4
    assert (lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, c, s) - 256) // 8 > 256
    a = _check(lib, dev, B, hp, c, s, p, 5, "random")
    lin, x, mask = _inputs(B, hp, c, s, p, 5, "random")
    o1, _ = _run(lib, dev, lin, x, mask, B, hp, c, s, p)
    o2, _ = _run(lib, dev, lin, x, mask, B, hp, c, s, p)
    for k in o1:
        assert_same_bits(o1[k], o2[k], f"{k} run to run")
    assert float(o1["loss"][0]) == a


# ---- the mask-token select -----------------------------------------------------------------------------------------------
def _mask_rows(T, kind, rng):
    return {"random": rng.uniform(size=T) < 0.6, "all": np.ones(T, bool), "none": np.zeros(T, bool)}[kind].astype(np.uint8) * 5


@pytest.mark.parametrize("Cn", [32, 96, 128])
def test_swin_mask_tokens(lib, dev, Cn):
    """T = 1, 300 (not a multiple of the 256-row chunk nor of the workgroup), 2 * 48^2; random, all and no rows masked."""
    rng = np.random.default_rng(Cn)
    for T, kind in [(1, "all"), (1, "none"), (300, "random"), (300, "all"), (300, "none"), (2 * 48 * 48, "random")]:
        what = f"swin_mask_tokens T={T} C={Cn} mask {kind}"
        rows = torch.from_numpy(rng.standard_normal((T, Cn)).astype(np.float32)).to(dev)
        tok = torch.from_numpy(rng.standard_normal(Cn).astype(np.float32)).to(dev)
        mk = torch.from_numpy(_mask_rows(T, kind, rng)).to(dev)
        want = torch.where(mk.bool().unsqueeze(1), tok.unsqueeze(0).expand(T, Cn), rows)
        got = rows.clone()
        assert lib.ocm_op_swin_mask_tokens(got.data_ptr(), mk.data_ptr(), tok.data_ptr(), T, Cn, _s()) == 0, lib.ocm_last_error()
        assert_same_bits(got, want, what)
        # backward
        d = torch.from_numpy(rng.standard_normal((T, Cn)).astype(np.float32)).to(dev)
        nbytes = lib.ocm_swin_mask_tokens_backward_workspace_bytes(T, Cn)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        d_rows = torch.full((T, Cn), float("nan"), device=dev)
        d_tok = torch.full((Cn,), float("nan"), device=dev)
        rc = lib.ocm_op_swin_mask_tokens_backward(d.data_ptr(), mk.data_ptr(), d_rows.data_ptr(), d_tok.data_ptr(), T, Cn,
                                                  ws.data_ptr(), nbytes, _s())
        assert rc == 0, lib.ocm_last_error()
        assert_same_bits(d_rows, torch.where(mk.bool().unsqueeze(1), torch.zeros_like(d), d), what + ": d_rows")
        sel = d.double().cpu() * mk.bool().unsqueeze(1).cpu()
        ref = sel.sum(0)
        err = (d_tok.double().cpu() - ref).abs()
        ulp = torch.tensor([_ulp32(float(v)) for v in ref], dtype=torch.float64)
        assert bool((err <= ulp).all()), (what, float((err / ulp).max()))
        if kind == "none":
            assert not bool(d_tok.any())
        # in place, and each output alone: the same bits
        d2, t2 = d.clone(), torch.full((Cn,), float("nan"), device=dev)
        assert lib.ocm_op_swin_mask_tokens_backward(d2.data_ptr(), mk.data_ptr(), d2.data_ptr(), None, T, Cn, ws.data_ptr(),
                                                    nbytes, _s()) == 0
        assert lib.ocm_op_swin_mask_tokens_backward(d.data_ptr(), mk.data_ptr(), None, t2.data_ptr(), T, Cn, ws.data_ptr(),
                                                    nbytes, _s()) == 0
        assert_same_bits(d2, d_rows, what + ": d_rows in place")
        assert_same_bits(t2, d_tok, what + ": d_mask_token alone")


def test_refused_arguments_on_device_buffers(lib, dev):
    """OCM_EINVAL / OCM_ENOMEM with real buffers: nothing is launched, the outputs keep their fill."""
    B, hp, c, s, p = 1, 3, 1, 4, 4
    lin, x, mask = _inputs(B, hp, c, s, p, 3, "random")
    tl, tx, tm = (torch.from_numpy(a).to(dev) for a in (lin, x, mask))
    rec = torch.full(x.shape, float("nan"), device=dev)
    nbytes = lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, c, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(lin_=tl, x_=tx, m_=tm, B_=B, hp_=hp, c_=c, s_=s, p_=p, ws_=ws, n_=nbytes):
        return lib.ocm_op_mim_l1_loss(lin_.data_ptr() if lin_ is not None else None, x_.data_ptr() if x_ is not None else None,
                                      m_.data_ptr() if m_ is not None else None, B_, hp_, hp_, c_, s_, p_, rec.data_ptr(), None,
                                      None, ws_.data_ptr() if ws_ is not None else None, n_, _s())

    E, M = _lib.OCM_EINVAL, _lib.OCM_ENOMEM
    assert call(lin_=None) == E and call(x_=None) == E and call(m_=None) == E
    assert call(p_=5) == E and call(p_=8) == E and call(B_=0) == E and call(hp_=0) == E and call(c_=0) == E and call(s_=0) == E
    assert call(ws_=None) == M and call(n_=nbytes - 1) == M
    torch.cuda.synchronize()
    assert bool(torch.isnan(rec).all())
    assert call() == 0
    rows = torch.zeros(4, 32, device=dev)
    mk = torch.ones(4, dtype=torch.uint8, device=dev)
    assert lib.ocm_op_swin_mask_tokens(rows.data_ptr(), mk.data_ptr(), None, 4, 32, _s()) == E
    assert lib.ocm_op_swin_mask_tokens(rows.data_ptr(), mk.data_ptr(), rows.data_ptr(), 0, 32, _s()) == E
    assert lib.ocm_op_swin_mask_tokens(rows.data_ptr(), mk.data_ptr(), rows.data_ptr(), 4, 30, _s()) == E
    assert lib.ocm_op_swin_mask_tokens_backward(rows.data_ptr(), mk.data_ptr(), rows.data_ptr(), rows.data_ptr(), 4, 32, None, 0,
                                                _s()) == M
    torch.cuda.synchronize()
    assert not bool(rows.any())
