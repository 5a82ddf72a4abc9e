"""Host side of Swin SimMIM pre-training (no GPU): the float64 twin of tests/swin_mim_ref.py pinned on the installed
transformers' SwinForMaskedImageModeling (loss, reconstruction and every parameter gradient), the module's parameter names and
state_dict against transformers', the numpy restatement of ocm_op_mim_l1_loss against torch, the output's indexing, and what the
module and the C ABI refuse before any launch.

transformers forms the loss's denominator as `mask.sum() + 1e-5` in torch's DEFAULT dtype (the count is an integer tensor), so a
float64 model under the float32 default loses the 1e-5. The comparison therefore runs transformers with the default dtype set to
float64; the twin forms that sum in its own dtype. Its attention is "sdpa": transformers' eager path rounds the softmax to
float32 even in a double model (2.9e-8 on the reconstruction), which would hide a twin error below that."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import swin_mim_ref as R
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW


def _module(name, **extra):
    cfg, sd, x, mask = R.case(name)
    m = SW.SwinForMaskedImageModeling(SW.SwinConfig(**R.hf_kwargs(cfg, **extra)))
    msg = m.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return m, x, mask


@pytest.mark.parametrize("name", ["t96_w6", "gray56_w7"])
def test_twin_matches_live_transformers(name):
    tf = pytest.importorskip("transformers")
    cfg, sd, x, mask = R.case(name, dtype=torch.float64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        hf = tf.SwinForMaskedImageModeling(tf.SwinConfig(**R.hf_kwargs(cfg, drop_path_rate=0.0, attn_implementation="sdpa")))
        msg = hf.load_state_dict(sd, strict=True)
        assert not msg.missing_keys and not msg.unexpected_keys
        hf = hf.double().eval().requires_grad_(True)
        out = hf(pixel_values=x, bool_masked_pos=mask)
        out.loss.backward()
    finally:
        torch.set_default_dtype(old)
    prm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    mine = R.twin(prm, cfg, x, mask)
    mine["loss"].backward()

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))

    assert rel(mine["loss"].detach(), out.loss.detach()) <= 1e-10
    assert rel(mine["reconstruction"].detach(), out.reconstruction.detach()) <= 1e-10
    grads = dict(hf.named_parameters())
    assert set(grads) == set(prm)
    for k, p in prm.items():
        assert grads[k].grad is not None and p.grad is not None, k
        if k.endswith("k_proj.bias"):  # exactly zero in exact arithmetic: round-off on both sides
            scale = grads[k[:-len("bias")] + "weight"].grad.abs().max()
            assert float((p.grad - grads[k].grad).abs().max() / scale) <= 1e-10, k
        else:
            assert rel(p.grad, grads[k].grad) <= 1e-10, (k, rel(p.grad, grads[k].grad))


def test_parameter_names_and_state_dict_equal_transformers():
    tf = pytest.importorskip("transformers")
    cfg = R.CASES["t192_w6_s32"]["cfg"]
    hf = tf.SwinForMaskedImageModeling(tf.SwinConfig(**R.hf_kwargs(cfg)))
    m = SW.SwinForMaskedImageModeling(SW.SwinConfig(**R.hf_kwargs(cfg)))
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert {m._names[n] for n, _ in m.named_parameters()} == {n for n, _ in hf.named_parameters()}
    msg = m.load_state_dict(hf.state_dict(), strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    assert torch.equal(m.state_dict()["decoder.0.weight"], hf.state_dict()["decoder.0.weight"])
    assert float(SW.SwinForMaskedImageModeling(SW.SwinConfig(**R.hf_kwargs(cfg))).state_dict()[
        "swin.embeddings.mask_token"].abs().max()) == 0.0  # zeros, as transformers creates it
    # the backbone with a mask token: the view over the model's own parameters (a stand-alone SwinModel keeps refusing
    # use_mask_token=True, as tests/test_swin_outputs_host.py holds it to)
    hback = tf.SwinModel(tf.SwinConfig(**R.hf_kwargs(cfg)), add_pooling_layer=False, use_mask_token=True)
    view = m.swin
    assert set(view.state_dict()) == set(hback.state_dict()) and view.add_pooling_layer is False
    assert view.state_dict()["embeddings.mask_token"].data_ptr() == m.state_dict()["swin.embeddings.mask_token"].data_ptr()
    assert SW.SwinConfig().encoder_stride == 32 == tf.SwinConfig().encoder_stride


def test_numpy_restatement_against_torch():
    """mim_l1_ref against F.l1_loss, repeat_interleave and torch's abs backward in float64, with an exact tie inside and outside
    the mask, and an all-false mask."""
    rng = np.random.default_rng(5)
    for (s, p, c, hp, B) in [(8, 4, 3, 3, 2), (4, 4, 1, 2, 1), (8, 8, 3, 2, 2), (32, 4, 3, 1, 1)]:
        S = hp * s
        lin = rng.standard_normal((B * hp * hp, c * s * s)).astype(np.float32)
        x = rng.standard_normal((B, c, S, S)).astype(np.float32)
        mask = (rng.uniform(size=(B, S // p, S // p)) < 0.6).astype(np.uint8)
        mask[0, 0, 0], mask[0, -1, -1] = 1, 0
        rec0 = R.shuffle(lin, B, hp, hp, c, s)
        x[0, 0, 0, 0], x[0, 0, -1, -1] = rec0[0, 0, 0, 0], rec0[0, 0, -1, -1]  # ties: masked, unmasked
        for mk in (mask, np.zeros_like(mask)):
            rec, dlin, loss, scale = R.mim_l1_ref(lin, x, mk, B, hp, hp, c, s, p)
            tl = torch.from_numpy(lin).double().requires_grad_(True)
            trec = F.pixel_shuffle(tl.reshape(B, hp, hp, c * s * s).permute(0, 3, 1, 2), s)
            assert np.array_equal(trec.detach().numpy().astype(np.float32), rec)
            m = torch.from_numpy(mk).bool().repeat_interleave(p, 1).repeat_interleave(p, 2).unsqueeze(1)
            tloss = (F.l1_loss(torch.from_numpy(x).double(), trec, reduction="none") * m).sum() / (m.sum().double() + 1e-5) / c
            tloss.backward()
            assert abs(loss - float(tloss.detach())) <= 1e-14 * max(1.0, abs(loss))
            g = tl.grad.numpy()
            assert set(np.unique(dlin).tolist()) <= {0.0, float(scale), -float(scale)}
            assert np.array_equal(np.sign(g), np.sign(dlin))
            assert np.allclose(g, dlin.astype(np.float64), rtol=1e-6, atol=0)
            if not mk.any():
                assert loss == 0.0 and not dlin.any()
            else:
                assert dlin[0, 0] == 0.0  # the masked tie: sign(0) = 0


def test_output_indexing():
    loss, rec = torch.zeros(()), torch.zeros(1, 3, 8, 8)
    out = SW.SwinMaskedImageModelingOutput(loss=loss, reconstruction=rec, hidden_states=None, attentions=None,
                                           reshaped_hidden_states=None)
    assert out["loss"] is loss and out[0] is loss and out[1] is rec and out.to_tuple() == (loss, rec)
    out = SW.SwinMaskedImageModelingOutput(loss=None, reconstruction=rec, hidden_states=(rec,), attentions=None,
                                           reshaped_hidden_states=(rec,))
    assert out[0] is rec and out["loss"] is None and len(out.to_tuple()) == 3 and out["reconstruction"] is rec


def test_refusals_before_any_launch(monkeypatch):
    m, x, mask = _module("gray56_w7")
    m.train().requires_grad_(True)

    def no_launch():
        raise AssertionError("the library was called before the refusal")

    monkeypatch.setattr(_lib, "load", no_launch)
    with pytest.raises(RuntimeError, match="HIP"):
        m(pixel_values=x, bool_masked_pos=mask)
    with pytest.raises(RuntimeError, match="HIP"):
        m.eval()(pixel_values=x, bool_masked_pos=mask)
    cfg = R.CASES["gray56_w7"]["cfg"]
    with pytest.raises(ValueError, match="encoder_stride"):
        SW.SwinForMaskedImageModeling(SW.SwinConfig(**R.hf_kwargs(cfg, encoder_stride=16)))
    # the mask's dtype and the token are checked on the host (_patch_mask), after the device check of the pixels
    c = m.config
    xd = x  # stands for a device tensor: _patch_mask does not look at where it lives
    for bad in (mask.float(), mask.to(torch.uint8), mask.long()):
        with pytest.raises(ValueError, match="torch.bool"):
            SW._patch_mask(c, xd, bad, True)
    with pytest.raises(ValueError, match="mask token"):
        SW._patch_mask(c, xd, mask, False)
    with pytest.raises(ValueError, match="mask token"):  # on a model without the token, before the device check
        SW.SwinModel(c)(pixel_values=x, bool_masked_pos=mask)
    with pytest.raises(ValueError, match="bool_masked_pos"):
        SW._patch_mask(c, xd, mask[:, :-1], True)
    assert SW._patch_mask(c, xd, None, False) is None
    got = SW._patch_mask(c, xd, mask, True)
    assert got.dtype == torch.uint8 and torch.equal(got.bool(), mask)
    # the training checks are the classifier's, message for message
    with pytest.raises(NotImplementedError, match="gradient of the input"):
        SW._check_swin_trainable(c, x.clone().requires_grad_(True))
    c.hidden_dropout_prob = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        SW._check_swin_trainable(c, x)
    c.hidden_dropout_prob = 0.0
    wide = SW.SwinConfig(image_size=64, embed_dim=32, depths=(2,), num_heads=(1,), window_size=8, encoder_stride=4)
    with pytest.raises(NotImplementedError, match="windows of 2 to 7"):
        SW._check_swin_trainable(wide, x)
    padded = SW.SwinConfig(image_size=64, embed_dim=32, depths=(2,), num_heads=(1,), window_size=7, encoder_stride=4)
    with pytest.raises(NotImplementedError, match="padding"):
        SW._check_swin_trainable(padded, x)
    assert SW._check_swin_trainable(c, x) is None
    assert not hasattr(m, "enable_padded_training") and not hasattr(m, "enable_wide_window_training")


def test_abi_refuses_bad_arguments(lib):
    """OCM_EINVAL / OCM_ENOMEM before any launch (no device is touched: the pointers are never dereferenced)."""
    P, W = C.c_void_p(4096), C.c_void_p(8192)
    EINVAL, ENOMEM = _lib.OCM_EINVAL, _lib.OCM_ENOMEM
    need = lib.ocm_mim_l1_loss_workspace_bytes(2, 3, 3, 3, 8)
    assert need >= 8 and lib.ocm_mim_l1_loss_workspace_bytes(0, 3, 3, 3, 8) == 0

    def loss(lin=P, x=P, mask=P, B=2, hp=3, wp=3, c=3, s=8, p=4, ws=W, nbytes=need):
        return lib.ocm_op_mim_l1_loss(lin, x, mask, B, hp, wp, c, s, p, P, P, P, ws, nbytes, None)

    assert loss(lin=None) == EINVAL and loss(x=None) == EINVAL and loss(mask=None) == EINVAL
    for bad in (dict(B=0), dict(hp=0), dict(wp=0), dict(c=0), dict(s=0), dict(p=0), dict(p=5), dict(p=16), dict(hp=2)):
        assert loss(**bad) == EINVAL, bad
    assert loss(ws=None) == ENOMEM and loss(nbytes=need - 1) == ENOMEM and loss(nbytes=0) == ENOMEM
    assert loss(lin=C.c_void_p(4100)) == EINVAL  # s % 4 == 0: 16-byte pieces

    need = lib.ocm_swin_mask_tokens_backward_workspace_bytes(300, 96)
    assert need == 2 * 96 * 8 and lib.ocm_swin_mask_tokens_backward_workspace_bytes(0, 96) == 0
    assert lib.ocm_op_swin_mask_tokens(None, P, P, 4, 32, None) == EINVAL
    assert lib.ocm_op_swin_mask_tokens(P, None, P, 4, 32, None) == EINVAL
    assert lib.ocm_op_swin_mask_tokens(P, P, None, 4, 32, None) == EINVAL
    assert lib.ocm_op_swin_mask_tokens(P, P, P, 0, 32, None) == EINVAL
    assert lib.ocm_op_swin_mask_tokens(P, P, P, 4, 0, None) == EINVAL
    assert lib.ocm_op_swin_mask_tokens(P, P, P, 4, 30, None) == EINVAL
    bwd = lib.ocm_op_swin_mask_tokens_backward
    assert bwd(None, P, P, P, 300, 96, W, need, None) == EINVAL and bwd(P, None, P, P, 300, 96, W, need, None) == EINVAL
    assert bwd(P, P, P, P, 0, 96, W, need, None) == EINVAL and bwd(P, P, P, P, 300, 0, W, need, None) == EINVAL
    assert bwd(P, P, P, P, 300, 96, None, need, None) == ENOMEM and bwd(P, P, P, P, 300, 96, W, need - 1, None) == ENOMEM
    # the engine entry: a null handle
    assert lib.ocm_swin_forward_masked(None, P, P, 1, P, P, P, None, W, 1 << 20, None) == EINVAL
