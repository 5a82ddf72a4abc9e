"""ocm_op_mim_l1_loss, ocm_op_swin_mask_tokens(_backward) and ocm_swin_forward_masked on poisoned workspaces and guard-banded
outputs (tests/memcheck.py; check_call of tests/test_memcheck_gpu.py): no store outside an output or the workspace, every output
element written, and the same bits whatever the workspace and the outputs held before. Shapes: the smallest of
tests/test_swin_mim_ops_gpu.py, and one whose token and pixel counts are off every block multiple. Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import swin_mim_ref as R
from tests.memcheck import PATTERNS
from tests.test_memcheck_gpu import _s, _spec, check_call
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW

pytestmark = pytest.mark.gpu
POISON = list(PATTERNS)


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("B,hp,c,s,p", [(1, 1, 1, 4, 4), (3, 3, 3, 8, 4), (1, 5, 1, 7, 5)])
def test_mim_l1_loss_guarded(lib, dev, B, hp, c, s, p, pattern):
    """(1, 5, 1, 7, 5): s = 7 takes the scalar kernel, 1225 pixels are no multiple of the workgroup, p = 5 is no power of two."""
    rng = np.random.default_rng(B * 100 + s)
    S = hp * s
    lin = torch.from_numpy(rng.standard_normal((B * hp * hp, c * s * s)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((B, c, S, S)).astype(np.float32)).to(dev)
    mask = torch.from_numpy((rng.uniform(size=(B, S // p, S // p)) < 0.6).astype(np.uint8)).to(dev)
    nbytes = lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, c, s)
    specs = {"rec": _spec((B, c, S, S)), "dlin": _spec(tuple(lin.shape)), "loss": _spec((1,))}
    out = check_call(lib, f"mim_l1_loss B={B} hp={hp} c={c} s={s} p={p} ws {pattern}",
                     lambda q, ws: lib.ocm_op_mim_l1_loss(lin.data_ptr(), x.data_ptr(), mask.data_ptr(), B, hp, hp, c, s, p,
                                                          q["rec"], q["dlin"], q["loss"], ws, nbytes, _s()),
                     specs, scratch_bytes=nbytes, pattern=pattern)
    rec, dlin, loss, _ = R.mim_l1_ref(lin.cpu().numpy(), x.cpu().numpy(), mask.cpu().numpy(), B, hp, hp, c, s, p)
    assert torch.equal(out["rec"].cpu(), torch.from_numpy(rec)) and torch.equal(out["dlin"].cpu(), torch.from_numpy(dlin))
    assert abs(float(out["loss"][0]) - loss) <= float(np.spacing(np.float32(loss)))


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("T,Cn", [(1, 32), (300, 96), (1031, 36)])
def test_swin_mask_tokens_guarded(lib, dev, T, Cn, pattern):
    """(1031, 36): rows off the 256-row chunk and the four row slices, columns off the 64-column workgroup."""
    rng = np.random.default_rng(T + Cn)
    rows = torch.from_numpy(rng.standard_normal((T, Cn)).astype(np.float32)).to(dev)
    tok = torch.from_numpy(rng.standard_normal(Cn).astype(np.float32)).to(dev)
    mask = torch.from_numpy((rng.uniform(size=T) < 0.6).astype(np.uint8)).to(dev)
    out = check_call(lib, f"swin_mask_tokens T={T} C={Cn}",
                     lambda q, ws: lib.ocm_op_swin_mask_tokens(q["rows"], mask.data_ptr(), tok.data_ptr(), T, Cn, _s()),
                     {"rows": _spec((T, Cn))}, inits={"rows": rows})
    assert torch.equal(out["rows"], torch.where(mask.bool().unsqueeze(1), tok.expand(T, Cn), rows))
    nbytes = lib.ocm_swin_mask_tokens_backward_workspace_bytes(T, Cn)
    out = check_call(lib, f"swin_mask_tokens_backward T={T} C={Cn} ws {pattern}",
                     lambda q, ws: lib.ocm_op_swin_mask_tokens_backward(rows.data_ptr(), mask.data_ptr(), q["d_rows"], q["d_tok"],
                                                                        T, Cn, ws, nbytes, _s()),
                     {"d_rows": _spec((T, Cn)), "d_tok": _spec((Cn,))}, scratch_bytes=nbytes, pattern=pattern)
    assert torch.equal(out["d_rows"], torch.where(mask.bool().unsqueeze(1), torch.zeros_like(rows), rows))
    ref = (rows.double() * mask.bool().unsqueeze(1)).sum(0)
    assert float((out["d_tok"].double() - ref).abs().max()) <= 1e-5


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("name,precision", [("gray56_w7", "bf16x3"), ("gray56_w7", "bf16"), ("t96_w6", "fp32")])
def test_swin_forward_masked_poisoned_workspace(lib, dev, name, precision, pattern):
    """B = 3 (token counts off the row tiles), a backbone engine with the mask token: pooled, last_hidden and hidden[0]."""
    cfg, sd, x, mask = R.case(name, batch=3)
    m = SW.SwinForMaskedImageModeling(SW.SwinConfig(**R.hf_kwargs(cfg)))
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).set_precision(precision).eval()
    eng = m._get_engine(dev)
    h, c, B = eng["h"], m.config, 3
    x = x.to(dev)
    mk = mask.to(dev).to(torch.uint8).contiguous()
    side = c.image_size // c.patch_size
    last = side >> (c.num_layers - 1)
    nbytes = lib.ocm_swin_workspace_bytes(h, B)
    specs = {"pooled": _spec((B, c.hidden_size)), "hidden": _spec((B, last * last, c.hidden_size)),
             "h0": _spec((B, side * side, c.embed_dim))}

    def call(q, ws):
        outs = _lib.OcmSwinOutputs()
        outs.hidden[0] = q["h0"]
        return lib.ocm_swin_forward_masked(h, x.data_ptr(), mk.data_ptr(), B, None, q["pooled"], q["hidden"], outs, ws, nbytes,
                                           _s())

    out = check_call(lib, f"ocm_swin_forward_masked {name} {precision} ws {pattern}", call, specs, scratch_bytes=nbytes,
                     pattern=pattern, plain=False)
    tok = sd["swin.embeddings.mask_token"].reshape(-1).to(dev)
    assert torch.equal(out["h0"][mask.to(dev)], tok.expand(int(mask.sum()), -1))
    got = m.swin(pixel_values=x, bool_masked_pos=mask.to(dev)).last_hidden_state
    assert torch.equal(out["hidden"], got)
