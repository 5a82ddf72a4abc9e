"""Memory behaviour of the shipped kernels: what they read from memory nobody wrote in this call, and what they write
outside their outputs. Needs an MI355X.

Every output sits in its own guard-banded buffer (tests/memcheck.py: 64 KiB guards on each side of an exactly sized
payload) and every workspace / scratch buffer is an exactly sized guarded payload filled with a byte pattern (`nan`,
`ones`, `zero`, `big`, `unit`). Each case asserts
  (a) the call returns OCM_OK;
  (b) no guard byte changed, of the workspace or of any output (a stray store within 64 KiB of a buffer; one that lands
      farther away is not seen here);
  (c) every output fully written: the call is made twice, on outputs pre-filled with `nan` and with `zero`, and the two
      results are the same bits (for floating-point outputs: no NaN left either);
  (d) the outputs do not depend on the workspace's previous contents: the same bits as the same call on a `zero`
      workspace.
Accuracy against the oracle is pinned by the other GPU modules; here a stand-alone operator is compared bit for bit with
the same call on plain exactly-sized allocations, which those modules check against their references.
"""
import ctypes as C
from functools import partial

import pytest
import torch

from tests.memcheck import Guarded, PATTERNS, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd.engine import Engine, to_operand

pytestmark = pytest.mark.gpu

POISON = list(PATTERNS)  # every case runs once per workspace pattern
ATTN_AXES = ("image", "head", "row", "col")
L = _lib


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(lib):
    return lib.ocm_last_error().decode(errors="replace")


def _once(lib, what, call, specs, fill, scratch, pattern, inits):
    """One call on freshly filled guarded outputs and scratch; returns {name: raw payload bytes (a copy)}."""
    outs = {}
    for name, (nbytes, _dtype, _shape) in specs.items():
        g = Guarded(nbytes, "cuda", fill)
        if name in inits:
            src = inits[name]
            g.payload(src.dtype, src.shape).copy_(src)
        outs[name] = g
    if scratch is not None:
        scratch.fill(pattern)
    torch.cuda.synchronize()
    rc = call({k: g.ptr for k, g in outs.items()}, scratch.ptr if scratch is not None else None)
    assert rc == 0, f"{what}: rc {rc} ({_err(lib)})"
    torch.cuda.synchronize()
    for name, g in outs.items():
        bad = g.check()
        assert bad is None, f"{what}: output {name!r}: {bad}"
    if scratch is not None:
        bad = scratch.check()
        assert bad is None, f"{what}: workspace (filled {pattern}): {bad}"
    return {k: g.payload().clone() for k, g in outs.items()}


def check_call(lib, what, call, specs, *, scratch_bytes=None, pattern="zero", inits=None, written=None, plain=True):
    """Run `call(ptrs, scratch_ptr)` under guards (module docstring (a)-(d)) and return the decoded outputs.

    specs: {name: (nbytes, dtype, shape)} of the outputs. inits: {name: tensor} copied into an output before each call
    (in-place operands). written: {name: fn(raw u8 payload) -> (bytes that must be written, bytes that must stay as
    filled)} for outputs the call writes only in part (padding columns, gap columns). plain: also run the call on
    exactly-sized torch.empty buffers and require the same bits."""
    inits, written = inits or {}, written or {}
    scratch = Guarded(scratch_bytes, "cuda", pattern) if scratch_bytes is not None else None
    a = _once(lib, what, call, specs, "nan", scratch, pattern, inits)
    b = _once(lib, what, call, specs, "zero", scratch, pattern, inits)
    for name in specs:
        ua, ub = a[name], b[name]
        if name in written:
            (ua, ka), (ub, kb) = written[name](ua), written[name](ub)
            if ka is not None:  # bytes the call must leave alone: still the fill (nan: bytes 0xC0 / 0x7F; zero: 0)
                assert bool(((ka == 0xC0) | (ka == 0x7F)).all()) and bool((kb == 0).all()), \
                    f"{what}: {name}: bytes outside the region the call writes were changed"
        assert_same_bits(ua, ub, f"{what}: {name} on outputs pre-filled with nan / zero (bytes)")
    outs = {}
    for name, (nbytes, dtype, shape) in specs.items():
        t = a[name].view(dtype).view(shape)
        if t.is_floating_point() and name not in written:
            nn_ = int(torch.isnan(t).sum())
            assert nn_ == 0, f"{what}: {name}: {nn_} NaN left (unwritten elements, or a poisoned read)"
        outs[name] = t
    if scratch is not None and pattern != "zero":
        z = _once(lib, what, call, specs, "nan", scratch, "zero", inits)
        for name in specs:
            assert_same_bits(a[name], z[name], f"{what}: {name}, workspace {pattern} vs zero (bytes)")
    if plain:
        bufs = {name: torch.empty(nbytes, dtype=torch.uint8, device="cuda") for name, (nbytes, _, _) in specs.items()}
        for name, src in inits.items():
            bufs[name].view(src.dtype).view(src.shape).copy_(src)
        sc = torch.empty(max(scratch_bytes or 0, 1) + 256, dtype=torch.uint8, device="cuda") if scratch is not None else None
        sp = (sc.data_ptr() + (-sc.data_ptr()) % 256) if sc is not None else None
        rc = call({k: t.data_ptr() for k, t in bufs.items()}, sp)
        assert rc == 0, f"{what}: plain call rc {rc} ({_err(lib)})"
        torch.cuda.synchronize()
        for name in specs:
            if name in written:
                assert_same_bits(written[name](a[name])[0], written[name](bufs[name])[0], f"{what}: {name} guarded vs plain")
            else:
                assert_same_bits(a[name], bufs[name], f"{what}: {name} guarded vs plain (bytes)")
    return outs


def _spec(shape, dtype=torch.float32):
    n = 1
    for d in shape:
        n *= d
    return (n * torch.empty((), dtype=dtype).element_size(), dtype, tuple(shape))


# ---------------------------------------------------------------------------------------------------------------------
# a. ocm_vit_forward through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _vit(kind, precision):
    """(module, engine) for a synthetic-weight ViT; `kind` = (embed_dim, depth, heads, patch, img)."""
    key = (kind, precision)
    if key not in _MODELS:
        import torch.nn as nn
        import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
        D, depth, H, p, img = kind
        model = vits.VisionTransformer(img_size=[img], patch_size=p, embed_dim=D, depth=depth, num_heads=H, mlp_ratio=4,
                                       qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), num_classes=0)
        model.load_state_dict(synth.synth_state_dict(D, depth, p, seed=3, variant="sharp" if D == 384 and H == 6 else "full",
                                                     img_size=img))
        model = model.eval().to("cuda").set_precision(precision)
        eng = model._engine(torch.device("cuda", 0))
        g = torch.Generator().manual_seed(5)
        eng.set_param("mask_token", (torch.randn(D, generator=g) * 0.02).cuda())
        _MODELS[key] = (model, eng)
    return _MODELS[key]


VITS16 = (384, 12, 6, 16, 224)
VITS8 = (384, 12, 6, 8, 384)
VITB16 = (768, 12, 12, 16, 384)
SIMMIM = (384, 2, 3, 16, 224)   # 3 heads of 128 channels (model.py's build_model encoder), two blocks
W48 = (192, 2, 4, 16, 224)      # 48-wide heads: the generic attention kernel and the qkv32 region

FLAGSETS = {
    "feat_attn_qkv": (L.OCM_OUT_FEAT | L.OCM_OUT_ATTN | L.OCM_OUT_QKV, 2),
    "last_attn": (L.OCM_LAST_ATTN_ONLY | L.OCM_OUT_ATTN, 1),
    "rows": (L.OCM_OUT_ROWS | L.OCM_LAST_ATTN_ONLY, 1),
    "fmap_tokens_mask": (L.OCM_OUT_FMAP | L.OCM_OUT_TOKENS, 1),
}


def _vit_specs(eng, B, n, hp, wp, flags, n_last, n_rows):
    D, H, hd = eng.D, eng.H, eng.hd
    s = {}
    if flags & L.OCM_OUT_FEAT:
        s["feat"] = _spec((n_last, B, n, D))
    if flags & L.OCM_OUT_ATTN:
        s["attn"] = _spec((n_last, B, H, n, n))
    if flags & L.OCM_OUT_QKV:
        s["qkv"] = _spec((n_last, 3, B, H, n, hd))
    if flags & L.OCM_OUT_TOKENS:
        s["tokens"] = _spec((B, n, D))
    if flags & L.OCM_OUT_ROWS:
        s["rows"] = _spec((B, H, n_rows, n - 1))
    if flags & L.OCM_OUT_FMAP:
        s["fmap"] = _spec((B, D, hp, wp))
    return s


def _vit_io(model, eng, x, flags, n_last):
    B, _, Ht, Wt = x.shape
    n = eng.n_tokens(Ht, Wt)
    pos = model._pos_for(n - 1, Ht, Wt, x.device)
    io = eng._io(x, (x.stride(0), x.stride(1), x.stride(2)), None, B, Ht, Wt, pos)
    io.flags, io.n_last = flags, n_last
    return io, n, pos


def _vit_call(lib, eng, io, keep):
    def call(p, ws):
        io.out_feat, io.out_attn, io.out_qkv = p.get("feat"), p.get("attn"), p.get("qkv")
        io.out_tokens, io.out_rows, io.out_fmap = p.get("tokens"), p.get("rows"), p.get("fmap")
        io.workspace, io.workspace_bytes = ws, keep["ws_bytes"]
        return lib.ocm_vit_forward(eng._h, C.byref(io))
    return call


def run_vit_forward(lib, kind, precision, B, flagset, pattern, options=()):
    model, eng = _vit(kind, precision)
    flags, n_last = FLAGSETS[flagset]
    img = kind[4]
    x = synth.synth_tiles(B, img, seed=11 + B).cuda()
    io, n, pos = _vit_io(model, eng, x, flags, n_last)
    hp = wp = img // kind[3]
    keep = {"x": x, "pos": pos}
    n_rows = 0
    if flags & L.OCM_OUT_ROWS:
        qr = torch.tensor([0, n - 1, n // 2], dtype=torch.int32, device="cuda")
        keep["qr"] = qr
        io.query_rows, io.n_rows = qr.data_ptr(), 3
        n_rows = 3
    if flagset == "fmap_tokens_mask":
        mask = synth.synth_patch_mask(B, hp, seed=B).to(torch.float32).reshape(B, -1).cuda()
        keep["mask"] = mask
        io.patch_mask = mask.data_ptr()
    keep["ws_bytes"] = lib.ocm_vit_workspace_bytes(eng._h, B, n)
    specs = _vit_specs(eng, B, n, hp, wp, flags, n_last, n_rows)
    what = f"ocm_vit_forward D{kind[0]} H{kind[2]} p{kind[3]} {img}^2 B={B} {precision} {flagset} options {options} ws {pattern}"
    try:
        for opt, val in options:
            L.check(lib.ocm_vit_set_option(eng._h, opt, val))
        return check_call(lib, what, _vit_call(lib, eng, io, keep), specs, scratch_bytes=keep["ws_bytes"], pattern=pattern,
                          plain=False)
    finally:
        for opt, _ in options:
            lib.ocm_vit_set_option(eng._h, opt, 0)


# (shape, precision, batch, flag sets, options). The comments name the dispatch branch each shape reaches, as ocm_gemm_plan reports
# it (csrc/gemm_plan.h; tests/test_gemm_plan_host.py asserts these rows: 197 x 384 x 1536 with a split-K workspace, 591 and 12 608
# rows at N = 384 / 1536, 15 002 rows at D = 768).
VIT_CASES = [
    # ViT-S/16 B = 1 (T = 197): split-K fc2 into w.part (T <= 512), the small-M DMA tiles, the folded LayerNorm (auto)
    (VITS16, "bf16x3", 1, ("feat_attn_qkv", "last_attn", "rows", "fmap_tokens_mask"), ()),
    (VITS16, "bf16x3", 1, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 1),)),
    (VITS16, "bf16x3", 1, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 2),)),
    (VITS16, "bf16x3", 1, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 1), (L.OCM_OPT_FUSE_LN, 1))),
    (VITS16, "bf16x3", 1, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 1), (L.OCM_OPT_FUSE_LN, 2))),
    # B = 3 (T = 591): past the split-K limit, fc2 on the plain GEMM
    (VITS16, "bf16x3", 3, ("feat_attn_qkv", "last_attn", "rows"), ()),
    # B = 64 (config 2, T = 12 608): 128 x 192 proj / fc2 with EpiResidStats' residual prefetch on the in-place x, the
    # 160-row fc1 tile with its half band, attn_fwd_x3_pp_kernel (V^T pad zeroing), the row-centring stats / shift slots
    (VITS16, "bf16x3", 64, ("feat_attn_qkv", "last_attn", "rows", "fmap_tokens_mask"), ()),
    (VITS16, "bf16x3", 64, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 2),)),
    (VITS16, "bf16x3", 64, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 1), (L.OCM_OPT_FUSE_LN, 1))),
    (VITS16, "bf16x3", 64, ("feat_attn_qkv",), ((L.OCM_OPT_FOLD_LN, 1), (L.OCM_OPT_FUSE_LN, 2))),
    # ViT-S/8 384^2 (N = 2305): the key-split attention into w.kpart at small B, streaming attention above 1024 tokens
    (VITS8, "bf16x3", 1, ("last_attn", "rows"), ()),
    (VITS8, "bf16x3", 2, ("feat_attn_qkv", "rows"), ()),
    # ViT-B/16 384^2 B = 26 (T = 15 002): the 256 x 256 tiles on the 16 x 16 MFMA (attn.qkv, mlp.fc1; proj / fc2 have 177 of them: 128 x 128)
    (VITB16, "bf16x3", 26, ("last_attn", "fmap_tokens_mask"), ()),
    # fp32 and single bf16: other element sizes, no folded LayerNorm
    (VITS16, "fp32", 1, ("feat_attn_qkv", "rows"), ()),
    (VITS16, "fp32", 64, ("feat_attn_qkv", "last_attn"), ()),
    (VITS16, "bf16", 1, ("feat_attn_qkv", "fmap_tokens_mask"), ()),
    (VITS16, "bf16", 64, ("feat_attn_qkv", "rows"), ()),
    # 128-wide heads (the SimMIM encoder) and 48-wide heads (generic attention on the fp32 qkv32 region)
    (SIMMIM, "bf16x3", 2, ("feat_attn_qkv", "rows", "fmap_tokens_mask"), ()),
    (W48, "bf16x3", 2, ("feat_attn_qkv", "last_attn", "rows"), ()),
    (W48, "fp32", 2, ("feat_attn_qkv", "rows"), ()),
]


def _case_id(c):
    kind, prec, B, fls, opts = c
    name = {VITS16: "vits16", VITS8: "vits8_384", VITB16: "vitb16_384", SIMMIM: "simmim_hd128", W48: "hd48"}[kind]
    o = "".join(f"-{'fold' if k == L.OCM_OPT_FOLD_LN else 'fuse'}{v}" for k, v in opts)
    return f"{name}-{prec}-B{B}{o}"


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("case", VIT_CASES, ids=_case_id)
def test_vit_forward_poisoned_workspace(lib, dev, case, pattern):
    kind, prec, B, flagsets, opts = case
    for fs in flagsets:
        run_vit_forward(lib, kind, prec, B, fs, pattern, opts)


@pytest.mark.parametrize("pattern", POISON)
def test_vit_forward_graph_replay_on_repoisoned_workspace(lib, dev, pattern):
    """OCM_USE_GRAPH at B = 1: capture, then replay with the same pointers after the workspace was poisoned again."""
    model, eng = _vit(VITS16, "bf16x3")
    x = synth.synth_tiles(1, 224, seed=12).cuda()
    flags = L.OCM_OUT_FEAT | L.OCM_OUT_ATTN | L.OCM_OUT_QKV
    io, n, pos = _vit_io(model, eng, x, flags | L.OCM_USE_GRAPH, 2)
    nbytes = lib.ocm_vit_workspace_bytes(eng._h, 1, n)
    specs = _vit_specs(eng, 1, n, 14, 14, flags, 2, 0)
    ref = run_vit_forward(lib, VITS16, "bf16x3", 1, "feat_attn_qkv", "zero")
    ws = Guarded(nbytes, "cuda", pattern)
    outs = {k: Guarded(nb, "cuda", "nan") for k, (nb, _, _) in specs.items()}
    io.out_feat, io.out_attn, io.out_qkv = outs["feat"].ptr, outs["attn"].ptr, outs["qkv"].ptr
    io.workspace, io.workspace_bytes = ws.ptr, nbytes
    r0, c0 = eng.graph_stats()
    for rep in range(2):
        ws.fill(pattern)
        for g in outs.values():
            g.fill("nan")
        torch.cuda.synchronize()
        rc = lib.ocm_vit_forward(eng._h, C.byref(io))
        assert rc == 0, _err(lib)
        torch.cuda.synchronize()
        assert ws.check() is None, f"graph call {rep}: workspace: {ws.check()}"
        for k, g in outs.items():
            assert g.check() is None, f"graph call {rep}: {k}: {g.check()}"
            assert_same_bits(g.payload(torch.float32, specs[k][2]), ref[k], f"graph call {rep} ({pattern}) {k} vs plain launches")
    r1, c1 = eng.graph_stats()
    # the second call replays (the first one too when an earlier case left a capture of the same pointers)
    assert (r1 - r0) + (c1 - c0) == 2 and r1 - r0 >= 1, (r0, c0, r1, c1)


# ---------------------------------------------------------------------------------------------------------------------
# b. the call sequence of test_config2_batch64_sampled_images, at module level, with a poisoned workspace per shape
# ---------------------------------------------------------------------------------------------------------------------
class _PoisonedWorkspaces:
    """Replacement for Engine.workspace: a new guarded workspace filled with `pattern` whenever the shape changes; the
    previous one's guards are checked when it is replaced. All of them stay alive until the test ends (captured graphs
    may point at them)."""

    def __init__(self, pattern):
        self.pattern, self.all, self.cur, self.problems = pattern, [], {}, []

    def check(self, key, g):
        torch.cuda.synchronize()
        bad = g.check()
        if bad:
            self.problems.append(f"workspace {key}: {bad}")

    def __call__(self, eng, batch, n):
        key = (batch, n)
        ent = self.cur.get(id(eng))
        if ent is None or ent[0] != key:
            if ent is not None:
                self.check(*ent)
            g = Guarded(eng.lib.ocm_vit_workspace_bytes(eng._h, batch, n), eng.device, self.pattern)
            self.all.append(g)
            self.cur[id(eng)] = ent = (key, g)
        return ent[1].ptr, ent[1].nbytes

    def rotate(self, pattern):
        """Check the current workspaces' guards; the next call of every engine takes a new one filled with `pattern`."""
        for key, g in self.cur.values():
            self.check(key, g)
        self.cur.clear()
        self.pattern = pattern

    def finish(self):
        self.rotate(self.pattern)
        assert not self.problems, "; ".join(self.problems)


@pytest.fixture
def poisoned(monkeypatch, request):
    pw = _PoisonedWorkspaces(request.param)
    monkeypatch.setattr(Engine, "workspace", lambda eng, batch, n: pw(eng, batch, n))
    yield pw
    pw.finish()


def _config2_model(variant):
    import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
    model = vits.vit_small(patch_size=16, num_classes=0)
    model.load_state_dict(synth.synth_arch_state_dict("vit_small", 16, seed=0, variant=variant))
    return model.eval().cuda()


@pytest.mark.parametrize("poisoned", POISON, indirect=True)
@pytest.mark.parametrize("variant", ["init", "sharp"])
def test_config2_sequence_on_poisoned_workspaces(dev, poisoned, variant):
    model = _config2_model(variant)
    x = synth.synth_tiles(64, 224, seed=1234).to(dev)
    attn = model.get_last_selfattention(x)
    rows = model.get_last_attention_rows(x)
    one = model.get_last_selfattention(x[31:32])
    feat, attns, qkvs = model.get_intermediate_feat(x, n=1)
    third = model.get_last_selfattention(x)
    torch.cuda.synchronize()
    for t, name in ((attn, "attn"), (rows, "rows"), (one, "one"), (feat[0], "feat"), (qkvs[0], "qkv")):
        assert not bool(torch.isnan(t).any()), f"{name}: NaN in the output"
    assert_same_bits(third, attn, f"{variant}/{poisoned.pattern}: third get_last_selfattention vs the first", ATTN_AXES)
    assert_same_bits(attns[0], third, f"{variant}/{poisoned.pattern}: get_intermediate_feat attns[0] vs the third "
                     "get_last_selfattention", ATTN_AXES)
    assert_same_bits(attns[0], attn, f"{variant}/{poisoned.pattern}: get_intermediate_feat attns[0] vs "
                     "get_last_selfattention", ATTN_AXES)


@pytest.mark.parametrize("poisoned", ["nan", "big", "unit"], indirect=True)
def test_every_block_on_poisoned_vs_zeroed_workspace(dev, poisoned):
    """get_intermediate_feat(n = depth) at B = 64: attn / qkv / feat of every block on a poisoned workspace and on a
    zeroed one; the message names the first block that differs."""
    model = _config2_model("sharp")
    x = synth.synth_tiles(64, 224, seed=1234).to(dev)
    got = model.get_intermediate_feat(x, n=12)
    pattern = poisoned.pattern
    poisoned.rotate("zero")  # the next call takes a fresh, zeroed workspace
    want = model.get_intermediate_feat(x, n=12)
    poisoned.rotate(pattern)
    for blk in range(12):
        for kind, axes in ((1, ATTN_AXES), (2, None), (0, ("image", "token", "channel"))):
            name = ("feat", "attn", "qkv")[kind]
            if not torch.equal(got[kind][blk], want[kind][blk]):
                assert_same_bits(got[kind][blk], want[kind][blk], f"first differing block: {blk}, {name} ({pattern} vs zero)",
                                 axes)


# ---------------------------------------------------------------------------------------------------------------------
# c. block-level entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("B", [1, 64])
def test_block_entry_points(lib, dev, B, pattern):
    model, eng = _vit(VITS16, "bf16x3")
    x = synth.synth_tiles(B, 224, seed=21).cuda()
    io, n, pos = _vit_io(model, eng, x, 0, 1)
    D, H = eng.D, eng.H
    tok = check_call(lib, f"ocm_vit_prepare_tokens B={B}", lambda p, ws: lib.ocm_vit_prepare_tokens(eng._h, C.byref(io), p["x"]),
                     {"x": _spec((B, n, D))})["x"].clone()
    ws_bytes = lib.ocm_vit_workspace_bytes(eng._h, B, n)
    for flags, outs in ((L.OCM_OUT_ATTN, ("x", "attn")), (L.OCM_OUT_ATTN | L.OCM_OUT_QKV, ("x", "attn", "qkv")),
                        (L.OCM_LAST_ATTN_ONLY | L.OCM_OUT_ATTN, ("x", "attn"))):
        specs = {"x": _spec((B, n, D)), "attn": _spec((B, H, n, n)), "qkv": _spec((3, B, H, n, 64))}
        specs = {k: specs[k] for k in outs}

        def call(p, ws, flags=flags):
            return lib.ocm_vit_block_forward(eng._h, 5, p["x"], B, n, flags, p.get("attn"), p.get("qkv"), ws, ws_bytes, _s())
        check_call(lib, f"ocm_vit_block_forward B={B} flags {flags} ws {pattern}", call, specs, scratch_bytes=ws_bytes,
                   pattern=pattern, inits={"x": tok})
    check_call(lib, f"ocm_vit_final_norm B={B}", lambda p, ws: lib.ocm_vit_final_norm(eng._h, tok.data_ptr(), p["y"], B * n, _s()),
               {"y": _spec((B, n, D))})


# ---------------------------------------------------------------------------------------------------------------------
# d. Swin
# ---------------------------------------------------------------------------------------------------------------------
def _swin(image_size, precision):
    """Swin-T at 224^2, the padded 120^2 miniature, or (a str) a SWIN_GEOMETRIES entry."""
    from tests.golden_cases import SWIN_CASES, SWIN_GEOMETRIES
    from vit_ocm_wmsegmentation_amd import swin as SW
    if isinstance(image_size, str):
        g = SWIN_GEOMETRIES[image_size]
        cfg = dict(synth.SWIN_TINY, **g["cfg"])
        sd = synth.synth_swin_state_dict(cfg, seed=g["seed"], qk_gain=g["qk_gain"])
    else:
        extra = SWIN_CASES["pad120"]["cfg"] if image_size == 120 else {}  # three stages: grids 30 / 15 / 8
        cfg = dict(synth.SWIN_TINY, **extra)
        sd = synth.synth_swin_state_dict(cfg, seed=21, qk_gain=6.0)
    model = SW.SwinForImageClassification(SW.SwinConfig(**{k: cfg[k] for k in (
        "image_size", "num_channels", "embed_dim", "depths", "num_heads", "window_size", "mlp_ratio", "layer_norm_eps",
        "num_labels")}))
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval().set_precision(precision)
    return model, model._get_engine(torch.device("cuda", 0))


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("image_size,precision,fuse", [(224, "bf16x3", 1), (224, "bf16x3", 0), (224, "bf16", 1),
                                                       (224, "fp32", 1), (120, "bf16x3", 1), (120, "fp32", 0),
                                                       ("B", "bf16", 1), ("B", "fp32", 1), ("C", "bf16", 1), ("C", "fp32", 1)])
def test_swin_forward_poisoned_workspace(lib, dev, image_size, precision, fuse, pattern):
    """224^2 B = 2 in every precision, the fused split-bf16 MLP / attention halves (OPT_FUSE_MLP 1) and the unfused
    launches (0), and the padded 120^2 geometry (grids 30 / 15 / 8: zero rows, odd-grid merging). SWIN_GEOMETRIES B and C at
    B = 3: the first geometries whose bf16 operands are K-padded (C = 32 -> 64, hidden 96 -> 128), so the engine's ctx / hid
    memsets and the zero columns of the LayerNorm rows carry the padding, whatever the workspace held before."""
    model, eng = _swin(image_size, precision)
    h = eng["h"]
    c = model.config
    B = 2 if isinstance(image_size, int) else 3
    side = c.image_size // c.patch_size
    for _ in range(c.num_layers - 1):
        side = (side + 1) // 2
    x = synth.synth_tiles(B, c.image_size, seed=71, channels=c.num_channels).cuda()
    nbytes = lib.ocm_swin_workspace_bytes(h, B)
    L.check(lib.ocm_swin_set_option(h, L.OCM_SWIN_OPT_FUSE_MLP, fuse))
    try:
        specs = {"logits": _spec((B, c.num_labels)), "pooled": _spec((B, c.hidden_size)),
                 "hidden": _spec((B, side * side, c.hidden_size))}
        check_call(lib, f"ocm_swin_forward {image_size}^2 {precision} fuse {fuse} ws {pattern}",
                   lambda p, ws: lib.ocm_swin_forward(h, x.data_ptr(), B, p["logits"], p["pooled"], p["hidden"], ws, nbytes, _s()),
                   specs, scratch_bytes=nbytes, pattern=pattern, plain=False)
    finally:
        lib.ocm_swin_set_option(h, L.OCM_SWIN_OPT_FUSE_MLP, 1)


def _pattern_fill(t, pattern):
    """Fill a tensor's (any strides; 4 bytes per element or a whole number of words per row) bytes with a pattern word."""
    w = PATTERNS[pattern]
    src = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    src.view(torch.uint8).view(-1, 4).copy_(torch.tensor([w - 2 ** 32 if w >= 2 ** 31 else w], dtype=torch.int32)
                                            .view(torch.uint8).to(t.device).expand(src.numel() * src.element_size() // 4, 4))
    t.copy_(src)
    return t


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp32"])
@pytest.mark.parametrize("H,W,ws,shift,heads", [(14, 14, 7, 3, 3), (8, 12, 4, 2, 2)])
def test_swin_window_attention_gap_columns(lib, dev, precision, H, W, ws, shift, heads, pattern):
    """ocm_op_swin_window_attention with ld > 3 * 32 * heads and ldc > 32 * heads: the input's gap columns hold the
    pattern (results must not depend on them), the output's gap columns must come back untouched, the scratch is
    poisoned."""
    B, C_ = 2, heads * 32
    ld, ldc = 3 * C_ + 64, C_ + 32
    rows = B * H * W
    g = torch.Generator().manual_seed(H + shift)
    qkv = torch.randn(rows, 3 * C_, generator=g).cuda()
    pc = L.PRECISIONS[precision]
    op = to_operand(qkv, pc)
    esz = op.element_size()
    src = _pattern_fill(torch.empty((rows, ld), dtype=op.dtype, device="cuda"), pattern)
    src[:, :3 * C_] = op
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    nbytes = heads * (4096 + ws ** 4) * 4

    def split(raw):
        r = raw.view(rows, ldc * esz)
        return r[:, :C_ * esz].contiguous(), r[:, C_ * esz:].contiguous()

    def call(p, sc):
        return lib.ocm_op_swin_window_attention(pc, src.data_ptr(), ld, p["ctx"], ldc, table.data_ptr(), sc, B, H, W, ws, shift,
                                                heads, _s())
    check_call(lib, f"swin window attention {precision} {H}x{W} ws{ws} shift{shift} scratch {pattern}", call,
               {"ctx": (rows * ldc * esz, op.dtype, (rows, ldc))}, scratch_bytes=nbytes, pattern=pattern,
               written={"ctx": lambda raw: (split(raw)[0], split(raw)[1])})


@pytest.mark.parametrize("pattern", POISON)
def test_swin_fused_ops_poisoned_scratch(lib, dev, pattern):
    """ocm_op_swin_attn_block (3 and 6 heads), ocm_op_swin_mlp and ocm_op_swin_lnqkv with guarded x / qkv."""
    pc = L.OCM_PREC_BF16X3
    g = torch.Generator().manual_seed(9)
    for heads, Hh, Ww, shift in ((3, 14, 14, 3), (6, 14, 14, 3)):
        Cn, B, ws = 32 * heads, 2, 7
        T = B * Hh * Ww
        x = (torch.randn(T, Cn, generator=g) * 2 + 0.3).cuda()
        gam, bet = (torch.randn(Cn, generator=g) * 0.2 + 1).cuda(), (torch.randn(Cn, generator=g) * 0.1).cuda()
        wqkv = to_operand((torch.randn(3 * Cn, Cn, generator=g) * Cn ** -0.5).cuda(), pc)
        bqkv = (torch.randn(3 * Cn, generator=g) * 0.1).cuda()
        wo = to_operand((torch.randn(Cn, Cn, generator=g) * Cn ** -0.5).cuda(), pc)
        bo = (torch.randn(Cn, generator=g) * 0.1).cuda()
        table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
        nbytes = (heads * 4096 + (T * Cn if heads in (4, 6) else 0)) * 4
        check_call(lib, f"swin attn_block heads {heads} scratch {pattern}",
                   lambda p, sc: lib.ocm_op_swin_attn_block(pc, p["x"], gam.data_ptr(), bet.data_ptr(), wqkv.data_ptr(),
                                                            bqkv.data_ptr(), wo.data_ptr(), bo.data_ptr(), table.data_ptr(), sc,
                                                            B, Hh, Ww, ws, shift, heads, 1e-5, _s()),
                   {"x": _spec((T, Cn))}, scratch_bytes=nbytes, pattern=pattern, inits={"x": x})
    for T, Cn in ((1000, 96), (33, 128)):
        x = (torch.randn(T, Cn, generator=g) * 2 + 0.3).cuda()
        gam, bet = (torch.randn(Cn, generator=g) * 0.2 + 1).cuda(), (torch.randn(Cn, generator=g) * 0.1).cuda()
        w1 = to_operand((torch.randn(4 * Cn, Cn, generator=g) * Cn ** -0.5).cuda(), pc)
        w2 = to_operand((torch.randn(Cn, 4 * Cn, generator=g) * (4 * Cn) ** -0.5).cuda(), pc)
        b1, b2 = (torch.randn(4 * Cn, generator=g) * 0.1).cuda(), (torch.randn(Cn, generator=g) * 0.1).cuda()
        check_call(lib, f"swin mlp T={T} C={Cn}",
                   lambda p, sc: lib.ocm_op_swin_mlp(pc, p["x"], gam.data_ptr(), bet.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                                     w2.data_ptr(), b2.data_ptr(), T, Cn, 4 * Cn, 1e-5, _s()),
                   {"x": _spec((T, Cn))}, inits={"x": x})
    for T, Cn in ((1000, 96), (37, 192)):
        x = (torch.randn(T, Cn, generator=g) * 2 + 0.3).cuda()
        gam, bet = (torch.randn(Cn, generator=g) * 0.2 + 1).cuda(), (torch.randn(Cn, generator=g) * 0.1).cuda()
        w = to_operand((torch.randn(3 * Cn, Cn, generator=g) * Cn ** -0.5).cuda(), pc)
        b = (torch.randn(3 * Cn, generator=g) * 0.1).cuda()
        check_call(lib, f"swin lnqkv T={T} C={Cn}",
                   lambda p, sc: lib.ocm_op_swin_lnqkv(pc, x.data_ptr(), gam.data_ptr(), bet.data_ptr(), w.data_ptr(),
                                                       b.data_ptr(), p["qkv"], T, Cn, 1e-5, _s()),
                   {"qkv": _spec((T, 3 * Cn), torch.int32)})


# ---------------------------------------------------------------------------------------------------------------------
# e. stand-alone operators of ocm_vit.h
# ---------------------------------------------------------------------------------------------------------------------
_ACT = {L.OCM_PREC_BF16: torch.bfloat16, L.OCM_PREC_FP32: torch.float32, L.OCM_PREC_BF16X3: torch.int32}

# the dispatch shapes listed above test_linear_x3 (tests/test_ops_x3_gpu.py), the M tails 12609 / 333 / 70 and N tails 96 / 288
LINEAR_SHAPES = [(1000, 384, 384), (12608, 1536, 384), (333, 384, 1536), (70, 96, 192), (12608, 384, 384), (64, 192, 64),
                 (32768, 1024, 768), (24576, 384, 1536), (6000, 288, 96), (6000, 96, 384), (5000, 576, 192),
                 (5000, 192, 768), (16384, 512, 384), (12609, 1536, 384), (20000, 1024, 384)]


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_guarded(lib, dev, M, N, K, precision):
    pc = L.PRECISIONS[precision]
    if pc == L.OCM_PREC_BF16:
        K = 64 * ((K + 63) // 64)  # single-bf16 operands need K % 64 == 0
    g = torch.Generator().manual_seed(M + N + K)
    a = to_operand(torch.randn(M, K, generator=g).cuda(), pc)
    w = to_operand((torch.randn(N, K, generator=g) * K ** -0.5).cuda(), pc)
    bias = torch.randn(N, generator=g).cuda()
    resid = torch.randn(M, N, generator=g).cuda()
    for epi in range(4):
        act = epi in (L.OCM_EPI_BIAS_GELU_BF16, L.OCM_EPI_BIAS_BF16)
        dt = _ACT[pc] if act else torch.float32
        inits = {"out": resid} if epi == L.OCM_EPI_BIAS_RESID_F32 else {}
        check_call(lib, f"linear {precision} M={M} N={N} K={K} epilogue {epi}",
                   lambda p, sc: lib.ocm_op_linear(pc, a.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                                   p["out"] if epi == L.OCM_EPI_BIAS_RESID_F32 else None, p["out"], M, N, K, epi,
                                                   _s()),
                   {"out": _spec((M, N), dt)}, inits=inits)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("M,D,K", [(12608, 384, 384), (12608, 384, 1536), (333, 256, 256), (8192, 128, 512)])
def test_linear_resid_ln_guarded(lib, dev, M, D, K, precision):
    pc = L.PRECISIONS[precision]
    g = torch.Generator().manual_seed(M + D + K)
    a = to_operand(torch.randn(M, K, generator=g).cuda(), pc)
    w = to_operand((torch.randn(D, K, generator=g) * K ** -0.5).cuda(), pc)
    bias, gam, bet = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
    resid = torch.randn(M, D, generator=g).cuda()
    check_call(lib, f"linear_resid_ln {precision} M={M} D={D} K={K}",
               lambda p, sc: lib.ocm_op_linear_resid_ln(pc, a.data_ptr(), w.data_ptr(), bias.data_ptr(), p["x"], p["x"],
                                                        gam.data_ptr(), bet.data_ptr(), p["xn"], M, D, K, 1e-6, _s()),
               {"x": _spec((M, D)), "xn": _spec((M, D), _ACT[pc])}, inits={"x": resid})


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("B,N,H,hd", [(2, 197, 6, 64), (1, 2305, 6, 64), (3, 50, 2, 128), (2, 37, 4, 48)])
def test_attention_chain_guarded(lib, dev, B, N, H, hd, precision):
    """qkv projection (q, k, V^T and the fp32 qkv tensor, each guarded) -> attention (ctx, lse) -> probabilities -> rows,
    and the generic kernel for 48-wide heads. The V^T padding columns are not written by contract (the attention multiplies
    them by exact zeros, so its callers zero them): they are checked as untouched and zeroed before the attention; the q / k
    padding rows are left poisoned."""
    pc = L.PRECISIONS[precision]
    D = H * hd
    g = torch.Generator().manual_seed(B * N + hd)
    a = to_operand(torch.randn(B * N, D, generator=g).cuda(), pc)
    w = to_operand((torch.randn(3 * D, D, generator=g) * D ** -0.5).cuda(), pc)
    bias = (torch.randn(3 * D, generator=g) * 0.1).cuda()
    scale = hd ** -0.5
    npad = lib.ocm_n_pad_prec(pc, N)
    et = _ACT[pc]
    esz = torch.empty((), dtype=et).element_size()
    tag = f"{precision} B={B} N={N} H={H} hd={hd}"
    if hd not in (64, 128):
        q32 = check_call(lib, f"qkv_proj_hd (fp32 only) {tag}",
                         lambda p, sc: lib.ocm_op_qkv_proj_hd(pc, a.data_ptr(), w.data_ptr(), bias.data_ptr(), None, None, None,
                                                              p["qkv"], B, N, H, hd, _s()),
                         {"qkv": _spec((3, B, H, N, hd))})["qkv"].clone()
        check_call(lib, f"attention_generic {tag}",
                   lambda p, sc: lib.ocm_op_attention_generic(pc, q32.data_ptr(), p["ctx"], p["attn"], B, N, H, hd, scale, _s()),
                   {"ctx": _spec((B * N, D), et), "attn": _spec((B, H, N, N))})
        return

    def vt_split(raw):  # [B*H][hd][npad]: columns >= N are padding the projection does not write
        r = raw.view(B * H * hd, npad * esz)
        if pc == L.OCM_PREC_BF16X3:  # pairs interleave 32 keys as [32 hi | 32 lo]: the whole 128-byte groups of keys < N
            return r[:, :(N // 32) * 128].contiguous(), None
        return r[:, :N * esz].contiguous(), r[:, N * esz:].contiguous()
    specs = {"q": _spec((B * H, npad, hd), et), "k": _spec((B * H, npad, hd), et), "vt": _spec((B * H, hd, npad), et),
             "qkv": _spec((3, B, H, N, hd))}

    def qk_split(raw):  # [B*H][npad][hd]: rows >= N are padding (written or not: not part of the contract)
        return raw.view(B * H, npad * hd * esz)[:, :N * hd * esz].contiguous(), None
    fn = lib.ocm_op_qkv_proj_hd
    o = check_call(lib, f"qkv_proj_hd {tag}",
                   lambda p, sc: fn(pc, a.data_ptr(), w.data_ptr(), bias.data_ptr(), p["q"], p["k"], p["vt"], p["qkv"], B, N, H,
                                    hd, _s()),
                   specs, written={"q": qk_split, "k": qk_split, "vt": vt_split})
    q, k, vt = o["q"].clone(), o["k"].clone(), o["vt"].clone()
    if pc == L.OCM_PREC_BF16X3:  # the callers' part of the contract: zero V^T padding (hi and lo halves of keys >= N)
        vt.view(torch.int16).view(B * H * hd, npad // 32, 2, 32)[:, -1, :, N % 32 or 32:] = 0
    else:
        vt.view(B * H, hd, npad)[:, :, N:] = 0
    if hd == 64:
        o64 = check_call(lib, f"qkv_proj {tag}",
                         lambda p, sc: lib.ocm_op_qkv_proj(pc, a.data_ptr(), w.data_ptr(), bias.data_ptr(), p["q"], p["k"], p["vt"],
                                                           p["qkv"], B, N, H, _s()),
                         specs, written={"q": qk_split, "k": qk_split, "vt": vt_split})
        assert_same_bits(o64["qkv"], o["qkv"], f"qkv_proj vs qkv_proj_hd {tag}")
    for t in (q, k):  # padding rows: whatever the projection left there, poisoned now
        _pattern_fill(t.view(B * H, npad, hd)[:, N:], "nan")
    out = check_call(lib, f"attention_hd {tag}",
                     lambda p, sc: lib.ocm_op_attention_hd(pc, q.data_ptr(), k.data_ptr(), vt.data_ptr(), p["ctx"], p["lse"], B,
                                                           N, H, hd, scale, _s()),
                     {"ctx": _spec((B, N, D), et), "lse": _spec((B * H, N))})
    lse = out["lse"].clone()
    check_call(lib, f"attention_probs_hd {tag}",
               lambda p, sc: lib.ocm_op_attention_probs_hd(pc, q.data_ptr(), k.data_ptr(), lse.data_ptr(), p["attn"], B, N, H, hd,
                                                           scale, _s()),
               {"attn": _spec((B, H, N, N))})
    if hd == 64:
        qr = torch.tensor([0, N - 1, N // 2], dtype=torch.int32, device="cuda")
        check_call(lib, f"attention_rows {tag}",
                   lambda p, sc: lib.ocm_op_attention_rows(pc, q.data_ptr(), k.data_ptr(), qr.data_ptr(), 3, p["rows"], B, N, H,
                                                           scale, _s()),
                   {"rows": _spec((B, H, 3, N - 1))})
        check_call(lib, f"attention {tag}",
                   lambda p, sc: lib.ocm_op_attention(pc, q.data_ptr(), k.data_ptr(), vt.data_ptr(), p["ctx"], p["lse"], B, N, H,
                                                      scale, _s()),
                   {"ctx": _spec((B, N, D), et), "lse": _spec((B * H, N))})
        check_call(lib, f"attention_probs {tag}",
                   lambda p, sc: lib.ocm_op_attention_probs(pc, q.data_ptr(), k.data_ptr(), lse.data_ptr(), p["attn"], B, N, H,
                                                            scale, _s()),
                   {"attn": _spec((B, H, N, N))})


@pytest.mark.parametrize("rows,dim", [(1000, 384), (7, 192), (513, 768), (65, 160)])
def test_layernorm_and_casts_guarded(lib, dev, rows, dim):
    g = torch.Generator().manual_seed(rows + dim)
    x = (torch.randn(rows, dim, generator=g) * 3 + 0.5).cuda()
    gam, bet = (torch.randn(dim, generator=g) * 0.1 + 1).cuda(), (torch.randn(dim, generator=g) * 0.1).cuda()
    for kind, dt in ((L.OCM_LN_F32, torch.float32), (L.OCM_LN_BF16, torch.bfloat16), (L.OCM_LN_SPLIT, torch.int32)):
        if kind == L.OCM_LN_SPLIT and dim % 32:
            continue
        check_call(lib, f"layernorm kind {kind} rows={rows} dim={dim}",
                   lambda p, sc: lib.ocm_op_layernorm(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), p["y"], kind, rows, dim, 1e-6,
                                                      _s()),
                   {"y": _spec((rows, dim), dt)})
    n = rows * dim
    check_call(lib, f"cast_bf16 {n}", lambda p, sc: lib.ocm_op_cast_bf16(x.data_ptr(), p["y"], n, _s()),
               {"y": _spec((n,), torch.bfloat16)})
    if n % 32 == 0:
        sp = check_call(lib, f"cast_split {n}", lambda p, sc: lib.ocm_op_cast_split(x.data_ptr(), p["y"], n, _s()),
                        {"y": _spec((n,), torch.int32)})["y"].clone()
        check_call(lib, f"merge_split {n}", lambda p, sc: lib.ocm_op_merge_split(sp.data_ptr(), p["y"], n, _s()),
                   {"y": _spec((n,))})


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
def test_im2col_and_pixel_shuffle_guarded(lib, dev, precision):
    pc = L.PRECISIONS[precision]
    B, h, w, Cc = 2, 14, 14, 64
    x = torch.randn(B, h * w, Cc, generator=torch.Generator().manual_seed(1)).cuda()
    for relu in (0, 1):
        check_call(lib, f"im2col3x3 {precision} relu {relu}",
                   lambda p, sc: lib.ocm_op_im2col3x3(pc, x.data_ptr(), p["y"], B, h, w, Cc, relu, _s()),
                   {"y": _spec((B * h * w, 9 * Cc), _ACT[pc])})
    s, c_out = 4, 3
    lin = torch.randn(B * h * w, s * s * c_out).cuda()
    check_call(lib, "pixel_shuffle", lambda p, sc: lib.ocm_op_pixel_shuffle(lin.data_ptr(), p["y"], B, h, w, c_out, s, _s()),
               {"y": _spec((B, c_out, h * s, w * s))})


def test_post_ops_guarded(lib, dev):
    g = torch.Generator().manual_seed(4)
    T, H, P = 5, 6, 48 * 48
    rows = (torch.rand(T, H, 1, P, generator=g) * 0.01).cuda()
    check_call(lib, "tile_postprocess", lambda p, sc: lib.ocm_op_tile_postprocess(rows.data_ptr(), p["y"], T, H, 1, P, _s()),
               {"y": _spec((T, P))})
    check_call(lib, "head_mean", lambda p, sc: lib.ocm_op_head_mean(rows.data_ptr(), p["y"], T, H, 1, P, _s()),
               {"y": _spec((T, P))})
    small = torch.rand(T, 48, 48, generator=g).cuda()
    check_call(lib, "bilinear_upsample", lambda p, sc: lib.ocm_op_bilinear_upsample(small.data_ptr(), p["y"], T, 48, 48, 8, _s()),
               {"y": _spec((T, 384, 384))})
    check_call(lib, "nearest_upsample", lambda p, sc: lib.ocm_op_nearest_upsample(small.data_ptr(), p["y"], T, 48, 48, 3, _s()),
               {"y": _spec((T, 144, 144))})
    big = torch.rand(T, 96, 96, generator=g).cuda()
    check_call(lib, "downscale_centre", lambda p, sc: lib.ocm_op_downscale_centre(big.data_ptr(), p["y"], T, 96, 96, 8, _s()),
               {"y": _spec((T, 12, 12))})
    for k in (3, 5):
        check_call(lib, f"median_filter {k}",
                   lambda p, sc: lib.ocm_op_median_filter(small.data_ptr(), p["y"], T, 48, 48, k, _s()), {"y": _spec((T, 48, 48))})
    for n, window, stride in ((3, 96, 32), (2, 384, 128)):
        crops = (torch.rand(n * n, window, window, generator=g) * 255).cuda()
        ramp = torch.linspace(1, 0, window - stride, dtype=torch.float64).cuda()
        S = window + (n - 1) * stride
        check_call(lib, f"stitch n={n}", lambda p, sc: lib.ocm_op_stitch(crops.data_ptr(), p["y"], ramp.data_ptr(), n, window,
                                                                         stride, _s()), {"y": _spec((S, S))})
        slab = torch.rand(3, S - 5, S + 3, generator=g).cuda()  # windows reaching past the slab: zero fill
        check_call(lib, f"stitch_image_u8 n={n}",
                   lambda p, sc: lib.ocm_op_stitch_image_u8(slab.data_ptr(), slab.stride(0), slab.stride(1), 3, S - 5, S + 3,
                                                            p["y"], ramp.data_ptr(), n, window, stride, p["hist"], _s()),
                   {"y": _spec((S, S), torch.uint8), "hist": _spec((256,), torch.int64)})
    attn = torch.rand(2, 3, 36, 36, generator=g).cuda()
    check_call(lib, "attention_map", lambda p, sc: lib.ocm_op_attention_map(attn.data_ptr(), p["y"], 1, 3, 36, 0, 5, 7, 8, _s()),
               {"y": _spec((3, 40, 56))})


@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("count", [4096, 4099, 1000 * 1000 + 7, 15])
def test_u8_ops_guarded(lib, dev, count, pattern):
    """u8 operators at counts that are and are not multiples of 16 (the vector tails); the 2048-byte scratch of
    normalize_u8 / weighted_u8 is poisoned; every hist256 is guarded."""
    g = torch.Generator().manual_seed(count)
    img = torch.rand(3, count, generator=g).cuda()
    heat = torch.rand(count, generator=g).cuda()
    u8 = (torch.rand(count, generator=g) * 255).to(torch.uint8).cuda()
    u8b = (torch.rand(count, generator=g) * 255).to(torch.uint8).cuda()
    h = _spec((256,), torch.int64)
    check_call(lib, f"normalize_u8 {count} scratch {pattern}",
               lambda p, sc: lib.ocm_op_normalize_u8(heat.data_ptr(), count, sc, p["y"], p["hist"], _s()),
               {"y": _spec((count,), torch.uint8), "hist": h}, scratch_bytes=2048, pattern=pattern)
    check_call(lib, f"weighted_u8 {count} scratch {pattern}",
               lambda p, sc: lib.ocm_op_weighted_u8(heat.data_ptr(), u8.data_ptr(), count, sc, p["r"], p["a"], p["hr"], p["ha"],
                                                    _s()),
               {"r": _spec((count,), torch.uint8), "a": _spec((count,), torch.uint8), "hr": h, "ha": h},
               scratch_bytes=2048, pattern=pattern)
    if pattern != "zero":
        return  # the operators below have no scratch: once is enough
    check_call(lib, f"histogram_u8 {count}", lambda p, sc: lib.ocm_op_histogram_u8(u8.data_ptr(), count, p["hist"], _s()),
               {"hist": h})
    check_call(lib, f"threshold_u8 {count}", lambda p, sc: lib.ocm_op_threshold_u8(u8.data_ptr(), p["y"], count, 100, _s()),
               {"y": _spec((count,), torch.uint8)})
    check_call(lib, f"blend_u8 {count}",
               lambda p, sc: lib.ocm_op_blend_u8(u8.data_ptr(), u8b.data_ptr(), count, 0.3, 1 - 0.3, p["y"], p["hist"], _s()),
               {"y": _spec((count,), torch.uint8), "hist": h})
    for chans in (1, 3):
        check_call(lib, f"image_to_gray_u8 {count} chans {chans}",
                   lambda p, sc: lib.ocm_op_image_to_gray_u8(img.data_ptr(), count, chans, count, p["y"], p["hist"], _s()),
                   {"y": _spec((count,), torch.uint8), "hist": h})


def test_guard_reports_a_byte_changed_by_torch(dev):
    """The guard helper's own sanity case on the device: a byte changed with torch (not by a kernel) is reported."""
    g = Guarded(4096, dev, "unit")
    assert g.check() is None
    g._buf.view(torch.uint8)[g.end + 100] = 0
    torch.cuda.synchronize()
    msg = g.check()
    print(f"\nGPUTEST guard sanity: {msg}")
    assert msg is not None and "back guard: 1 byte(s) changed at offsets 100 .. 100" in msg
