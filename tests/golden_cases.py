"""The golden-fixture cases: shared by oracle/make_golden.py (which writes tests/golden/<name>.npz from
the real reference) and by the tests (which regenerate weights/inputs from the same seeds).
  arch | (dim, depth, heads): model;  patch, img_size: constructor;  variant, seed: synth.synth_state_dict;
  inputs: [(batch, height, width, tile_seed)];  n: last-n blocks returned;  full: store complete tensors."""
CASES = {
    # name: dict(ctor=..., heads, patch, img_size, variant, seed, inputs=[(B, H, W, seed)], n)
    "tiny_p8": dict(dim=128, depth=2, heads=2, patch=8, img_size=32, variant="full", seed=1,
                    inputs=[(2, 32, 32, 11), (1, 48, 32, 12)], n=2, full=True),
    "vits16_full": dict(arch="vit_small", patch=16, img_size=224, variant="full", seed=0,
                        inputs=[(2, 224, 224, 1234)], n=1),
    "vits16_sharp": dict(arch="vit_small", patch=16, img_size=224, variant="sharp", seed=0,
                         inputs=[(2, 224, 224, 1234)], n=1),
    "vits16_peaked": dict(arch="vit_small", patch=16, img_size=224, variant="peaked", seed=0,
                          inputs=[(2, 224, 224, 1234)], n=1),
    "vits16_init": dict(arch="vit_small", patch=16, img_size=224, variant="init", seed=0,
                        inputs=[(1, 224, 224, 1234)], n=1),
    "vitt16_full": dict(arch="vit_tiny", patch=16, img_size=224, variant="full", seed=3,
                        inputs=[(1, 224, 224, 77)], n=1),
    "vits8_384_sharp": dict(arch="vit_small", patch=8, img_size=224, variant="sharp", seed=0,
                            inputs=[(1, 384, 384, 4321)], n=1),
    "vitb16_384_full": dict(arch="vit_base", patch=16, img_size=224, variant="full", seed=0,
                            inputs=[(1, 384, 384, 99)], n=1),
    # round 3: precision stress sets for the other two BASELINE geometries, qkv gain calibrated to attention max ~0.8
    # (the x8 of "peaked" saturates ViT-B's softmax at 1.0000 and leaves ViT-S/8's 2305-token softmax at 0.06)
    "vitb16_384_sharp": dict(arch="vit_base", patch=16, img_size=224, variant="qkv6.5", seed=0,
                             inputs=[(1, 384, 384, 99)], n=1),
    "vits8_384_peaked": dict(arch="vit_small", patch=8, img_size=224, variant="qkv10", seed=0,
                             inputs=[(1, 384, 384, 4321)], n=1),
    # ViT-B with the x8 gain: attention max 1.0000, CLS-row max 0.998. Ill-conditioned: the reference's own fp32
    # result moves by 5.5e-4 against float64 arithmetic (tools/precision_study.py). Kept as a documented
    # conditioning case with its own, looser bounds (tests/test_model_gpu.py), not as a 1e-3 case.
    "vitb16_384_saturated": dict(arch="vit_base", patch=16, img_size=224, variant="peaked", seed=0,
                                 inputs=[(1, 384, 384, 99)], n=1),
}


# Precision-stress sets (attention max >= 0.79): single-bf16 operands are off by 1e-2 .. 1 here, so that mode is not
# claimed on them; the default split-bf16 mode is held to the north star's 1e-3 on all but the saturated one.
STRESS = ("vits16_peaked", "vits8_384_peaked", "vitb16_384_sharp", "vitb16_384_saturated")
# Saturated softmax (max 1.0000): the fp32 reference itself is 5.5e-4 away from float64 arithmetic, i.e. ill-conditioned
# at the 1e-3 level. Bounds per mode (tests/test_model_gpu.py): split-bf16 3e-2, fp32 MFMA 3e-3.
SATURATED = ("vitb16_384_saturated",)


# scipy.ndimage.median_filter fixture (oracle/make_golden_median.py writes tests/golden/median.npz from scipy itself;
# the tests regenerate the inputs here without importing scipy)
MEDIAN_SIZES = (2, 3, 4, 5, 7)


def median_inputs(seed=17):
    import numpy as np
    rng = np.random.default_rng(seed)
    smooth = rng.random((2, 6, 5), dtype=np.float32)
    up = np.repeat(np.repeat(smooth, 4, axis=1), 4, axis=2)  # block-constant like a nearest-upsampled attention map
    noisy = rng.random((2, 24, 20), dtype=np.float32)
    noisy[0, 3:9, 2:7] = 0.5  # ties
    return np.concatenate([up, noisy], 0)


# The filter's edges (oracle/make_golden_median.py writes tests/golden/median_edges.npz, keys map<i>_size<k>): maps of height
# or width 1, windows wider than the map (size // 2 >= h: scipy's "reflect" runs through more than one period; >= 2h at
# (1, 1, 7) and (1, 2, 3)), the identity (size 1), eval.py's --median_filter 13 and the cap 15 with its even neighbour.
MEDIAN_EDGE_SIZES = (1, 2, 6, 13, 14, 15)
MEDIAN_EDGE_SHAPES = ((1, 1, 1), (1, 1, 7), (2, 5, 9), (1, 2, 3), (1, 3, 17))


def median_edge_inputs(seed=23):
    """One (T, h, w) float32 array per MEDIAN_EDGE_SHAPES entry: values in [0.125, 1.125) with planted ties (every third
    element is 0.5), no NaN and no negative zero — scipy's choice among equal values of different bits is not pinned."""
    import numpy as np
    rng = np.random.default_rng(seed)
    maps = []
    for shape in MEDIAN_EDGE_SHAPES:
        m = rng.random(shape, dtype=np.float32) + np.float32(0.125)
        m.reshape(-1)[2::3] = 0.5
        maps.append(m)
    return maps


# Post-processing geometries shared by the oracle's CPU pins (tests/test_oracle_golden.py) and the kernels' value tests
# (tests/test_post_shapes_gpu.py). The stitchers accept stride < window <= 3 * stride; (n, window, stride):
#   (3, 12, 4) the reference's 3:1;  (3, 12, 6) exactly two windows per pixel;  (4, 11, 5) (4, 13, 5) (5, 7, 3) (3, 10, 4)
#   strides that do not divide the window, with two- and three-window folds;  (3, 9, 8) a one-element ramp;
#   (2, 10, 7) window <= 2 * stride;  (1, 12, 4) a single window
STITCH_GEOMETRIES = ((3, 12, 4), (3, 12, 6), (4, 11, 5), (3, 9, 8), (2, 10, 7), (4, 13, 5), (5, 7, 3), (1, 12, 4), (3, 10, 4))
# uint8 slab stitcher, (H, W, stride, window); the window count per axis is len(range(0, side - 2 * stride, stride)).
# (21, 23, 4, 12) and (21, 22, 5, 13) have windows that reach past the slab (PIL crop's zero fill), the second of them
# at a stride that does not divide the window.
STITCH_U8_GEOMETRIES = ((20, 20, 4, 12), (21, 23, 4, 12), (30, 28, 6, 12), (26, 26, 8, 9), (25, 27, 7, 10), (19, 19, 5, 13),
                        (21, 22, 5, 13))
# bilinear upsample, (T, h, w, scale): non-square maps, scales with an inexact reciprocal (3, 5), one-pixel sides, the
# identity, and 147 456 outputs per map against the launch's 64 workgroups x 256 threads
BILINEAR_SHAPES = ((2, 5, 7, 3), (1, 1, 9, 8), (1, 9, 1, 2), (3, 4, 6, 1), (2, 48, 48, 8), (1, 13, 31, 5))


# model.py wrappers: encoder geometry + decoder stride; weights / masks from synth.py.
# img_size != 224 exercises the interpolated-position branch (model.py:38-39), 224 the native one.
WRAPPER_CASES = {
    "wrap_p8_64": dict(dim=128, depth=2, heads=2, patch=8, img_size=64, batch=2, seed=11, variant="full"),
    "wrap_p16_224": dict(dim=128, depth=2, heads=2, patch=16, img_size=224, batch=1, seed=12, variant="sharp"),
    # the reference's own build_model() encoder (model.py:93-103): depth 4, THREE heads of 128 channels
    "wrap_mim_hd128": dict(dim=384, depth=4, heads=3, patch=8, img_size=64, batch=2, seed=13, variant="sharp"),
}


# Swin: fixtures come from the installed transformers package (oracle/make_golden_swin.py).
# "tiny224" is the reference's configuration (SwinConfig defaults, num_labels=5, ADB/train.py:70-77);
# "small56" is a 2-stage miniature (image 56 -> 14x14 -> 7x7 grids) that exercises shift masks and the
# window-equals-grid clamp in seconds.
SWIN_CASES = {
    "tiny224": dict(batch=2, seed=21, qk_gain=6.0),
    "small56": dict(batch=3, seed=22, qk_gain=6.0, cfg=dict(image_size=56, depths=(2, 2), num_heads=(3, 6))),
    # transformers' padding paths: grids 30 -> 15 -> 8 (windows of 7: padded to 35 / 21 / 14; the odd 15 x 15 grid gets a row and
    # a column of zeros in the patch merging)
    "pad120": dict(batch=2, seed=23, qk_gain=6.0, cfg=dict(image_size=120, depths=(2, 2, 2), num_heads=(3, 6, 12))),
}


# Swin geometries off the Swin-T defaults (oracle/make_golden_swin.py writes tests/golden/swin_geom_<name>.npz;
# tests/test_swin_geometry_gpu.py runs them in every precision against the float64 oracle). Each entry reaches dispatch
# branches of libocm_vit.so's Swin engine that SWIN_CASES (window 7, embed_dim 96, mlp_ratio 4, eps 1e-5) never takes.
# "bf16" names the single-bf16 mode, whose GEMM K step of 64 pads K = 32 / 96 rows; split-bf16 and fp32 step by 32.
# Counts (batch x windows x heads) per stage are given where they leave partial workgroups (4 wavefronts in the bf16
# window attention, 3 in the split-bf16 one, 2 / 4 windows in the fused attention halves).
SWIN_GEOMETRIES = {
    # embed <1, 2>; grids 14 -> 7 padded to 15 / 10 for windows of 5 (shifted windows in stage 0); layernorm_after + fc1 +
    # GELU fused at C = 128, N = 256 (hidden != 4C, so no fused MLP); odd depth 3 (the last layer unshifted); generic pool
    # head at C = 128; config eps 1e-3 against the fixed 1e-5 of embedding / merging; window x head counts 54 and 48
    "A": dict(batch=3, seed=61, qk_gain=4.0, cfg=dict(image_size=56, embed_dim=64, num_channels=1, depths=(3, 1),
                                                      num_heads=(2, 4), window_size=5, mlp_ratio=2.0, layer_norm_eps=1e-3,
                                                      num_labels=7)),
    # embed <3, 1>; bf16: K padding of C = 32 (Kc 64: the ctx memset) and of M = 96 (Km 128: the hid memset); patch merging
    # LayerNorm widths 128 and 256; stage 2 grid 4 = window (no shift): fused attention half <4, 0, 8> on 3 windows (one
    # partial workgroup of 4) and layernorm_after + fc1 + GELU at C = 128, N = 384; one label
    "B": dict(batch=3, seed=62, qk_gain=5.0, cfg=dict(image_size=64, embed_dim=32, num_channels=3, depths=(2, 2, 1),
                                                      num_heads=(1, 2, 4), window_size=4, mlp_ratio=3.0, layer_norm_eps=1e-5,
                                                      num_labels=1)),
    # one stage (the pool head right after stage 0, no merging); embed <1, 3>; fused attention half <3, 0, 4> (o_proj fused)
    # at ws 6; layernorm_after + fc1 + GELU at C = 96, N = 96; bf16: Km != M (96 -> 128); eps 1e-6
    "C": dict(batch=3, seed=63, qk_gain=6.0, cfg=dict(image_size=48, embed_dim=96, num_channels=1, depths=(3,), num_heads=(3,),
                                                      window_size=6, mlp_ratio=1.0, layer_norm_eps=1e-6, num_labels=3)),
    # embed <3, 4>; grids 10 -> 5 padded to 12 / 6 for windows of 3 (shift 1 at both); pool head vec<1> (C = 256)
    "D": dict(batch=3, seed=64, qk_gain=4.0, cfg=dict(image_size=40, embed_dim=128, num_channels=3, depths=(2, 2),
                                                      num_heads=(4, 8), window_size=3, mlp_ratio=4.0, layer_norm_eps=1e-5,
                                                      num_labels=3)),
    # embed <3, 2>; windows of 2 in four stages (the last grid = window); fused MLP and fused attention half <4, 0, 8> at
    # C = 128; pool head vec<2> (C = 512)
    "E": dict(batch=3, seed=65, qk_gain=5.0, cfg=dict(image_size=64, embed_dim=64, num_channels=3, depths=(2, 2, 2, 2),
                                                      num_heads=(2, 4, 8, 16), window_size=2, mlp_ratio=4.0,
                                                      layer_norm_eps=1e-5, num_labels=4)),
    # embed <1, 4>; 32 heads in the last stage; pool head vec<4> (C = 1024) with 1000 labels (far more than its 8
    # wavefronts); batch 1: window x head counts 256, 128, 64, 32
    "F": dict(batch=1, seed=66, qk_gain=6.0, cfg=dict(image_size=64, embed_dim=128, num_channels=1, depths=(1, 1, 3, 1),
                                                      num_heads=(4, 8, 16, 32), window_size=2, mlp_ratio=4.0,
                                                      layer_norm_eps=1e-5, num_labels=1000)),
    # embed <1, 1>; odd grid 15 padded to 21 for windows of 7, merged (one zero row / column) to 8, padded to 14; generic
    # pool head at C = 64; batch 1: window x head counts 9 and 8
    "G": dict(batch=1, seed=67, qk_gain=4.0, cfg=dict(image_size=60, embed_dim=32, num_channels=1, depths=(2, 2), num_heads=(1, 2),
                                                      window_size=7, mlp_ratio=4.0, layer_norm_eps=1e-5, num_labels=2)),
    # grids 24 -> 12, multiples of the window 6 (no padding): fused attention halves <3, 0, 4, true> and <6, 0, 8, false>,
    # fused MLP at C = 96, layernorm_after + fc1 + GELU at C = 192
    "H": dict(batch=3, seed=68, qk_gain=5.0, cfg=dict(image_size=96, embed_dim=96, num_channels=3, depths=(1, 2), num_heads=(3, 6),
                                                      window_size=6, mlp_ratio=4.0, layer_norm_eps=1e-5, num_labels=5)),
}
