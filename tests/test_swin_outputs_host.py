"""Host side of the Swin backbone outputs (no GPU): the float64 twin (tests/swin_outputs_ref.py) pinned on live transformers,
the conditioning of the test weights, ocm_swin_output_shape, and the parameter surface of SwinModel / `.swin`."""
import ctypes as C

import pytest
import torch

from tests import swin_outputs_ref as R
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd import swin as SW

_TWIN = {}


def twin(name, batch=2):
    """The float64 twin's outputs (with the conditioning variants) for a geometry, computed once."""
    if (name, batch) not in _TWIN:
        cfg, sd, x = R.case(name, torch.float64, batch)
        _TWIN[name, batch] = R.backbone_outputs(sd, cfg, x, variants=True)
    return _TWIN[name, batch]


def _c_config(cfg, precision=_lib.OCM_PREC_FP32, reserved=0):
    c = _lib.OcmSwinConfig(image_size=cfg["image_size"], patch_size=cfg["patch_size"], num_channels=cfg["num_channels"],
                           embed_dim=cfg["embed_dim"], num_stages=len(cfg["depths"]), window_size=cfg["window_size"],
                           num_labels=cfg["num_labels"], mlp_ratio=cfg["mlp_ratio"], ln_eps=cfg["layer_norm_eps"],
                           precision=precision, reserved=reserved)
    for i, (d, h) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        c.depths[i], c.num_heads[i] = d, h
    return c


def _shape(lib, cfg, batch, kind, index):
    dims = (C.c_int64 * 4)()
    _lib.check(lib.ocm_swin_output_shape(C.byref(_c_config(cfg)), batch, kind, index, dims))
    return tuple(dims)


def _hf_model(cfg, sd):
    """transformers' SwinForImageClassification in float64 with eager attention and a hook on every block's attention."""
    tf = pytest.importorskip("transformers")
    hc = tf.SwinConfig(image_size=cfg["image_size"], patch_size=cfg["patch_size"], num_channels=cfg["num_channels"],
                       embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                       window_size=cfg["window_size"], mlp_ratio=cfg["mlp_ratio"], layer_norm_eps=cfg["layer_norm_eps"],
                       num_labels=cfg["num_labels"], attn_implementation="eager")
    m = tf.SwinForImageClassification(hc)
    msg = m.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    m = m.double().eval()
    hooked = []
    for stage in m.swin.encoder.layers:
        for blk in stage.blocks:
            blk.attention.register_forward_hook(lambda mod, args, out: hooked.append(out[1]))
    return m, hooked


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_twin_matches_live_transformers(name):
    cfg, sd, x = R.case(name, torch.float64)
    m, hooked = _hf_model(cfg, sd)
    with torch.no_grad():
        out = m(pixel_values=x, output_hidden_states=True, output_attentions=True)
    want = twin(name)
    n_layers = sum(cfg["depths"])
    assert len(hooked) == n_layers and all(h is not None for h in hooked)
    for i, (got, ref) in enumerate(zip(hooked, want["attentions"])):
        assert got.shape == ref.shape, i
        err = float((got.double() - ref).abs().max())
        assert err <= 1e-6, (i, err)  # transformers' eager softmax is float32 even in a double model
    # what transformers itself returns as `attentions` (per stage in 5.x, per layer before) is among the hooked tensors
    assert all(any(a is h or torch.equal(a, h) for h in hooked) for a in out.attentions)
    assert len(out.hidden_states) == len(want["hidden_states"]) == len(cfg["depths"]) + 1
    for i, (got, ref) in enumerate(zip(out.hidden_states, want["hidden_states"])):
        assert got.shape == ref.shape, i
        err = float((got - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()), (i, err)
    for got, ref, hid in zip(out.reshaped_hidden_states, want["reshaped_hidden_states"], out.hidden_states):
        B, Cc, H, W = got.shape
        assert got.shape == ref.shape
        assert torch.equal(got, hid.transpose(1, 2).reshape(B, Cc, H, W))
    for ref, hid in zip(want["reshaped_hidden_states"], want["hidden_states"]):
        assert torch.equal(ref, hid.transpose(1, 2).reshape(ref.shape))
    assert float((out.logits - want["logits"]).abs().max()) <= 1e-5 * max(1.0, float(want["logits"].abs().max()))


@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_test_weights_are_conditioned(name, batch):
    """In every layer of every test geometry: zeroing the bias table moves some probability by >= 0.05, so does dropping the
    shift mask in the shifted layers, and no softmax row saturates — a wrong bias bin, head order or mask cannot hide inside a
    tolerance, and the -100 mask is not the only thing the rows show."""
    cfg = dict(synth.SWIN_TINY, **R.GEOMETRIES[name][0])
    want = twin(name, batch)
    shifted = 0
    for i, (p, v) in enumerate(zip(want["attentions"], want["variants"])):
        assert float((p - v["zero_bias"]).abs().max()) >= 0.05, i
        if v["shift"]:
            shifted += 1
            assert float((p - v["no_mask"]).abs().max()) >= 0.05, i
        else:
            assert torch.equal(p, v["no_mask"]), i
        assert float(p.max(-1).values.max()) <= 0.999, i
        assert float((p.sum(-1) - 1).abs().max()) <= 1e-12
    # g32w4: stage 1's grid equals the window, so only stage 0 shifts; g40w4 shifts (and pads) in both stages
    assert shifted == {"g32w4": 1, "g40w4": 2, "g56w7": 1, "g56w7c96": 1}[name]
    assert len(want["attentions"]) == sum(cfg["depths"])


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_output_shape_matches_twin(lib, name):
    cfg = dict(synth.SWIN_TINY, **R.GEOMETRIES[name][0])
    for batch in (2, 3):
        want = twin(name, batch)
        for i, (h, r) in enumerate(zip(want["hidden_states"], want["reshaped_hidden_states"])):
            assert _shape(lib, cfg, batch, _lib.OCM_SWIN_OUT_HIDDEN, i) == tuple(h.shape) + (1,)
            assert _shape(lib, cfg, batch, _lib.OCM_SWIN_OUT_RESHAPED, i) == tuple(r.shape)
        for i, a in enumerate(want["attentions"]):
            assert _shape(lib, cfg, batch, _lib.OCM_SWIN_OUT_ATTENTION, i) == tuple(a.shape)
    if name == "g40w4":  # padded window counts: 10 -> 12 (9 windows) and 5 -> 8 (4 windows) per image
        assert [tuple(a.shape)[0] for a in twin(name, 2)["attentions"]] == [18, 18, 8, 8]


def test_output_shape_swin_tiny_defaults_and_errors(lib):
    cfg, B = synth.SWIN_TINY, 5
    got = [_shape(lib, cfg, B, _lib.OCM_SWIN_OUT_ATTENTION, i) for i in range(12)]
    want = [(B * 64, 3, 49, 49)] * 2 + [(B * 16, 6, 49, 49)] * 2 + [(B * 4, 12, 49, 49)] * 6 + [(B, 24, 49, 49)] * 2
    assert got == want
    assert [_shape(lib, cfg, B, _lib.OCM_SWIN_OUT_HIDDEN, i) for i in range(5)] == [
        (B, 3136, 96, 1), (B, 784, 192, 1), (B, 196, 384, 1), (B, 49, 768, 1), (B, 49, 768, 1)]
    assert [_shape(lib, cfg, B, _lib.OCM_SWIN_OUT_RESHAPED, i) for i in range(5)] == [
        (B, 96, 56, 56), (B, 192, 28, 28), (B, 384, 14, 14), (B, 768, 7, 7), (B, 768, 7, 7)]
    # an odd grid is halved upwards by the patch merging: image 200 -> grids 50, 25, 13, 7; windows on the padded grids
    c200 = dict(cfg, image_size=200)
    assert _shape(lib, c200, 1, _lib.OCM_SWIN_OUT_RESHAPED, 2) == (1, 384, 13, 13)
    assert _shape(lib, c200, 1, _lib.OCM_SWIN_OUT_ATTENTION, 0) == (64, 3, 49, 49)   # 50 -> 56: 8 x 8 windows
    assert _shape(lib, c200, 1, _lib.OCM_SWIN_OUT_ATTENTION, 4) == (4, 12, 49, 49)   # 13 -> 14: 2 x 2 windows
    dims = (C.c_int64 * 4)()
    cc = _c_config(cfg)
    for kind, index in ((_lib.OCM_SWIN_OUT_HIDDEN, 5), (_lib.OCM_SWIN_OUT_HIDDEN, -1), (_lib.OCM_SWIN_OUT_ATTENTION, 12), (3, 0)):
        assert lib.ocm_swin_output_shape(C.byref(cc), 1, kind, index, dims) == _lib.OCM_EINVAL, (kind, index)
    assert lib.ocm_swin_output_shape(C.byref(cc), 0, 0, 0, dims) == _lib.OCM_EINVAL
    assert lib.ocm_swin_output_shape(None, 1, 0, 0, dims) == _lib.OCM_EINVAL
    assert lib.ocm_swin_output_shape(C.byref(_c_config(dict(cfg, image_size=96))), 1, 0, 0, dims) == _lib.OCM_EINVAL
    # a backbone configuration (no classifier) ignores num_labels; without the flag num_labels = 0 stays an error
    assert lib.ocm_swin_output_shape(C.byref(_c_config(dict(cfg, num_labels=0))), 1, 0, 0, dims) == _lib.OCM_EINVAL
    back = _c_config(dict(cfg, num_labels=0), reserved=_lib.OCM_SWIN_CFG_BACKBONE)
    assert lib.ocm_swin_output_shape(C.byref(back), 1, 0, 0, dims) == _lib.OCM_OK
    assert lib.ocm_swin_output_shape(C.byref(_c_config(cfg, reserved=2)), 1, 0, 0, dims) == _lib.OCM_EINVAL


def test_new_entry_points_reject_bad_arguments(lib):
    one = C.c_void_p(256)
    assert lib.ocm_swin_forward_ex(None, one, 1, one, None, None, None, one, 1 << 20, None) == _lib.OCM_EINVAL
    ok = dict(batch=1, height=4, width=4, window=4, shift=0, heads=1)

    def probs(precision=_lib.OCM_PREC_FP32, qkv=one, ld=96, out=one, table=one, scratch=one, **kw):
        a = dict(ok, **kw)
        return lib.ocm_op_swin_window_probs(precision, qkv, ld, out, table, scratch, a["batch"], a["height"], a["width"],
                                            a["window"], a["shift"], a["heads"], None)

    for bad in (dict(qkv=None), dict(out=None), dict(table=None), dict(scratch=None), dict(precision=7), dict(window=8),
                dict(window=1), dict(height=6), dict(width=0), dict(shift=4), dict(shift=-1), dict(heads=0), dict(batch=0),
                dict(ld=95), dict(ld=100, precision=_lib.OCM_PREC_BF16X3), dict(out=C.c_void_p(260))):
        assert probs(**bad) == _lib.OCM_EINVAL, bad
    for bad in ((None, one, 1, 4, 32), (one, None, 1, 4, 32), (one, one, 0, 4, 32), (one, one, 1, 0, 32), (one, one, 1, 4, 0),
                (one, one, 65536, 4, 32)):
        assert lib.ocm_op_swin_tokens_to_nchw(*bad, None) == _lib.OCM_EINVAL, bad


# ---- the parameter surface -------------------------------------------------------------------------------------------------
def _small_config(**kw):
    return SW.SwinConfig(**dict(dict(image_size=32, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=4, num_labels=5),
                                **kw))


def test_swin_model_keys_equal_transformers():
    tf = pytest.importorskip("transformers")
    over = dict(image_size=32, embed_dim=32, depths=[2, 2], num_heads=[1, 2], window_size=4)
    hf = tf.SwinModel(tf.SwinConfig(**over))
    ours = SW.SwinModel(_small_config())
    assert set(ours.state_dict()) == set(hf.state_dict())
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert not ours.load_state_dict(hf.state_dict(), strict=True).missing_keys
    cls_keys = set(SW.SwinForImageClassification(_small_config()).state_dict())
    assert {"swin." + k for k in ours.state_dict()} == {k for k in cls_keys if not k.startswith("classifier.")}
    assert len(ours.state_dict()) == 77 and len(cls_keys) == 79
    # Swin-T defaults as well
    assert set(SW.SwinModel(SW.SwinConfig()).state_dict()) == set(tf.SwinModel(tf.SwinConfig()).state_dict())


def test_swin_view_shares_parameters_and_leaves_the_owner_unchanged():
    m = SW.SwinForImageClassification(_small_config())
    keys, params, named = list(m.state_dict()), list(m.parameters()), [n for n, _ in m.named_parameters()]
    modules = list(m.modules())
    v = m.swin
    assert isinstance(v, SW.SwinModel)
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_parameters()] == named
    assert len(list(m.parameters())) == len(params) and all(a is b for a, b in zip(m.parameters(), params))
    assert list(m.modules()) == modules and "swin" not in m._modules and not list(m.children())
    own = {m._names[n]: p for n, p in m.named_parameters()}
    seen = {v._names[n]: p for n, p in v.named_parameters()}
    assert set(seen) == {k[len("swin."):] for k in own if k.startswith("swin.")}
    for k, p in seen.items():
        assert p is own["swin." + k]  # the same Parameter objects, hence the same storage
    with torch.no_grad():
        own["swin.layernorm.weight"].add_(1.0)
    assert torch.equal(v.state_dict()["layernorm.weight"], own["swin.layernorm.weight"])
    assert v.state_dict()["layernorm.weight"].data_ptr() == own["swin.layernorm.weight"].data_ptr()
    # a fine-tuned classifier's weights reach a stand-alone SwinModel through the view's state_dict
    alone = SW.SwinModel(_small_config())
    assert not alone.load_state_dict(v.state_dict(), strict=True).missing_keys
    assert v.training == m.training and m.eval().swin.training is False
    assert m.set_precision("fp32").swin._precision == "fp32"


def test_not_implemented_paths():
    cfg = _small_config()
    with pytest.raises(NotImplementedError):
        SW.SwinModel(cfg, use_mask_token=True)
    assert SW.SwinModel(cfg, add_pooling_layer=False).add_pooling_layer is False
    x = torch.zeros(1, 3, 32, 32)
    m = SW.SwinModel(cfg)
    with pytest.raises(NotImplementedError):
        m(x, bool_masked_pos=torch.zeros(1, 64, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        m(x, interpolate_pos_encoding=True)
    with pytest.raises(RuntimeError):  # no CPU fallback
        m.eval()(x)
    with pytest.raises(ValueError):
        SW._layer_list(cfg, [4])
    assert SW._layer_list(cfg, True) == [0, 1, 2, 3] and SW._layer_list(cfg, False) == [] and SW._layer_list(cfg, (3, 1)) == [1, 3]


@pytest.mark.gpu
def test_training_mode_refusals(dev):
    """What needs a device to be reached: the training-mode refusals come after the input's device check."""
    cfg = _small_config()
    x = torch.zeros(1, 3, 32, 32, device=dev)
    m = SW.SwinModel(cfg).to(dev).train().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m(x)
    c = SW.SwinForImageClassification(cfg).to(dev).train().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        c(pixel_values=x, output_attentions=True)
    out = c(pixel_values=x, output_hidden_states=True)
    assert out.hidden_states is None and out.reshaped_hidden_states is None and out.attentions is None
    assert out.last_hidden_state is not None
    with pytest.raises(NotImplementedError):
        c.swin(x)
