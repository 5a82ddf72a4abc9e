/*
 * ocm_swin.h — C ABI of the Swin forward (BASELINE.json config 5), part of libocm_vit.so.
 *
 * Replaces, for inference, what Allen_data_Backbone/train.py:70-85 of linum-uqam/ViT-OCM-WMSegmentation
 * builds: transformers' SwinForImageClassification(SwinConfig(num_labels=5)) — patch embedding, four stages
 * of (shifted-)window attention blocks with relative-position bias, patch merging, final LayerNorm, mean pool
 * and classifier (transformers/models/swin/modeling_swin.py). Parameter names are that model's state_dict
 * keys. Same conventions as ocm_vit.h: plain pointers and sizes, int return codes (OCM_OK / OCM_E*),
 * ocm_last_error() for the message, nothing synchronises the device, no CPU fallback.
 */
#ifndef OCM_SWIN_H
#define OCM_SWIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ocm_swin_config {
    int32_t image_size;   /* square input, multiple of patch_size * window_size * 2^(stages-1) (224)   */
    int32_t patch_size;   /* 4                                                                        */
    int32_t num_channels; /* 1 or 3                                                                   */
    int32_t embed_dim;    /* C0 (96): stage s has C0 * 2^s channels                                   */
    int32_t num_stages;   /* 1..4                                                                     */
    int32_t depths[4];    /* (2, 2, 6, 2)                                                             */
    int32_t num_heads[4]; /* (3, 6, 12, 24): channels / heads must be 32                              */
    int32_t window_size;  /* 7; 2 .. 12 in inference (12: the window12-384 checkpoints), 2 .. 7 in training */
    int32_t num_labels;   /* classifier outputs (5 in the reference), positive unless a backbone      */
    float mlp_ratio;      /* 4.0                                                                      */
    float ln_eps;         /* 1e-5                                                                     */
    int32_t precision;    /* OCM_PREC_BF16 / OCM_PREC_FP32 / OCM_PREC_BF16X3 (ocm_vit.h)              */
    int32_t reserved;     /* flag bits: 0, or OCM_SWIN_CFG_BACKBONE                                   */
} ocm_swin_config;

/* reserved = OCM_SWIN_CFG_BACKBONE: transformers' SwinModel, a backbone without classifier. num_labels is ignored (0 labels),
 * no classifier.* parameter exists or is waited for by ocm_swin_params_ready, and `logits` of the forward may be null.
 * (Without the flag num_labels = 0 stays an error, as before.) */
enum { OCM_SWIN_CFG_BACKBONE = 1 };

typedef struct ocm_swin ocm_swin_t;

int ocm_swin_create(const ocm_swin_config *cfg, ocm_swin_t **out);
void ocm_swin_destroy(ocm_swin_t *h);

/* Upload one parameter by its transformers state_dict key, e.g.
 *   swin.embeddings.patch_embeddings.projection.{weight,bias}, swin.embeddings.norm.{weight,bias},
 *   swin.encoder.layers.{s}.blocks.{b}.attention.{q,k,v,o}_proj.{weight,bias},
 *   swin.encoder.layers.{s}.blocks.{b}.attention.relative_position_bias.relative_position_bias_table,
 *   swin.encoder.layers.{s}.blocks.{b}.{layernorm_before,layernorm_after}.{weight,bias},
 *   swin.encoder.layers.{s}.blocks.{b}.mlp.{fc1,fc2}.{weight,bias},
 *   swin.encoder.layers.{s}.downsample.{reduction.weight,norm.weight,norm.bias},
 *   swin.layernorm.{weight,bias}, classifier.{weight,bias}
 * from a contiguous fp32 device buffer in the reference layout; the engine keeps its own packed copy.
 * swin.embeddings.mask_token (embed_dim floats: transformers' SwinForMaskedImageModeling) is optional:
 * ocm_swin_params_ready does not wait for it, and only ocm_swin_forward_masked with a mask reads it. */
int ocm_swin_set_param(ocm_swin_t *h, const char *name, const float *dev_src, size_t count, void *stream);
int ocm_swin_params_ready(const ocm_swin_t *h);

size_t ocm_swin_workspace_bytes(const ocm_swin_t *h, int32_t batch);

/* SwinForImageClassification.forward (modeling_swin.py:1029-1066) on pixel_values (B, C, S, S) fp32, contiguous.
 * logits: (B, num_labels); pooled (optional): (B, C_last) = pooler_output; last_hidden (optional):
 * (B, L_last, C_last) = last_hidden_state after the final LayerNorm. */
int ocm_swin_forward(ocm_swin_t *h, const float *pixel_values, int32_t batch, float *logits, float *pooled,
                     float *last_hidden, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the backbone outputs (transformers' SwinModel / SwinEncoder with output_hidden_states / output_attentions) ----
 * Every member of ocm_swin_outputs is optional: a null pointer skips that output. All buffers are fp32 device memory the
 * caller owns, sized by ocm_swin_output_shape, the attention buffers 16-byte aligned.
 *   hidden[i], i in [0, num_stages]: token-major (B, L_i, C_i). [0] is the embeddings output, [s + 1] stage s's output AFTER
 *     its patch merging, the last entry the last stage's output BEFORE the final LayerNorm (transformers' hidden_states).
 *     They are copies of the residual stream at the stage boundaries: asking for them changes nothing that is computed.
 *   reshaped[i]: the same values as (B, C_i, H_i, W_i) = hidden[i].transpose(1, 2).reshape(...) (reshaped_hidden_states).
 *   attentions: a HOST array of sum(depths) device pointers in global layer order (stage 0's blocks first), or null.
 *     attentions[l] receives layer l's softmax(q k^T / sqrt(32) + bias + shift mask) as (B * nW, heads, ws^2, ws^2), windows of
 *     the rolled grid in window_partition order, nW counted on the grid PADDED to the window (as transformers returns it with
 *     attn_implementation="eager"; one entry per layer, not per stage). A layer whose map is requested runs LayerNorm ->
 *     q | k | v GEMM -> window attention -> o_proj (the chain of OCM_SWIN_OPT_FUSE_MLP = 0 and of the padded geometries)
 *     followed by ocm_op_swin_window_probs on the q | k | v rows. So does every layer BEFORE the last requested one, so that
 *     a map holds the same bits whichever other maps are asked for; the layers after it stay on their fused kernels. In
 *     fp32 and bf16 that is the chain the plain call runs (same bits); in split-bf16 logits / pooled / last_hidden then
 *     agree with the plain call to fp32 rounding, as OCM_SWIN_OPT_FUSE_MLP = 0 does. ocm_swin_workspace_bytes covers both
 *     chains (the q | k | v and LayerNorm buffers are sized for every stage, fused or not). */
typedef struct ocm_swin_outputs {
    float *hidden[5];
    float *reshaped[5];
    float *const *attentions;
} ocm_swin_outputs;

/* ocm_swin_forward with the backbone outputs: `outputs` null (or all of its members null) is ocm_swin_forward, bit for bit.
 * On a backbone (OCM_SWIN_CFG_BACKBONE) logits may be null and is not written. ocm_swin_forward is this call with null. */
int ocm_swin_forward_ex(ocm_swin_t *h, const float *pixel_values, int32_t batch, float *logits, float *pooled,
                        float *last_hidden, const ocm_swin_outputs *outputs, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ocm_swin_forward_ex with SwinEmbeddings' bool_masked_pos: patch_mask (B, L_0) uint8 on the device, one byte per token of the
 * patch grid, or null. A token whose byte is nonzero is replaced by swin.embeddings.mask_token (ocm_op_swin_mask_tokens, a row
 * select, bit exact) after embeddings.norm and before hidden[0] is emitted; everything behind it is ocm_swin_forward_ex.
 * A null mask is ocm_swin_forward_ex bit for bit (which is this call with null); a mask without the parameter is OCM_EINVAL. */
int ocm_swin_forward_masked(ocm_swin_t *h, const float *pixel_values, const uint8_t *patch_mask, int32_t batch, float *logits,
                            float *pooled, float *last_hidden, const ocm_swin_outputs *outputs, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Shape of an output of ocm_swin_forward_ex for a configuration and batch: a host function, no device is touched (the
 * configuration is checked as ocm_swin_create checks it). kind OCM_SWIN_OUT_HIDDEN: index in [0, num_stages] -> dims
 * (B, L, C, 1); OCM_SWIN_OUT_RESHAPED: (B, C, H, W); OCM_SWIN_OUT_ATTENTION: index = global layer -> (B * nW, heads, ws^2, ws^2)
 * with nW = ceil(grid / ws)^2 (the padded grid; an odd grid is halved upwards by the patch merging). The window is
 * window_size in every stage (a grid smaller than the window is refused); where the grid equals the window the odd layers
 * run without a shift, which changes values, not shapes. */
enum { OCM_SWIN_OUT_HIDDEN = 0, OCM_SWIN_OUT_RESHAPED = 1, OCM_SWIN_OUT_ATTENTION = 2 };
int ocm_swin_output_shape(const ocm_swin_config *cfg, int32_t batch, int32_t kind, int32_t index, int64_t dims[4]);

/* Per-handle dispatch options. OCM_SWIN_OPT_FUSE_MLP (default 1): in split-bf16 precision the layers of the narrow stages
 * (96 or 128 channels) run their MLP half as ONE kernel (ocm_op_swin_mlp), those of up to 192 channels layernorm_before +
 * the q | k | v projection as one (ocm_op_swin_lnqkv), and those of 96 channels their whole attention half as one
 * (ocm_op_swin_attn_block); 0 runs LayerNorm kernels, GEMMs and the window-attention kernel. Results agree to fp32 rounding. */
enum { OCM_SWIN_OPT_FUSE_MLP = 0 };
int ocm_swin_set_option(ocm_swin_t *h, int32_t option, int32_t value);

/* layernorm_before + the q | k | v projections of one SwinLayer (modeling_swin.py:641, :430-432) in one kernel:
 * qkv (tokens, 3 * channels) split pairs = LayerNorm(x; gamma, beta, eps) W^T + bias, W (3 * channels, channels) split pairs
 * (rows: q | k | v), x (tokens, channels) fp32. OCM_PREC_BF16X3, channels 96, 128 or 192; anything else returns OCM_EINVAL. */
int ocm_op_swin_lnqkv(int32_t precision, const float *x, const float *gamma, const float *beta, const void *w,
                      const float *bias, void *qkv, int64_t tokens, int32_t channels, float eps, void *stream);

/* MLP half of one SwinLayer (modeling_swin.py:668-672: layernorm_after, SwinIntermediate, SwinOutput, residual) in one
 * kernel: x (tokens, channels) fp32, in place, x += W2 gelu(W1 LayerNorm(x; gamma, beta, eps) + b1) + b2. Built for
 * precision OCM_PREC_BF16X3 (w1 (hidden, channels) and w2 (channels, hidden) as split pairs, ocm_op_cast_split),
 * channels 96 or 128, hidden = 4 x channels; anything else returns OCM_EINVAL. */
int ocm_op_swin_mlp(int32_t precision, float *x, const float *gamma, const float *beta, const void *w1, const float *b1,
                    const void *w2, const float *b2, int64_t tokens, int32_t channels, int32_t hidden, float eps,
                    void *stream);

/* Attention half of one SwinLayer (modeling_swin.py:641-666: layernorm_before, SwinSelfAttention with the relative-position
 * bias and the shift mask, SwinSelfOutput, residual) in one kernel: x (batch * height * width, 32 * heads) fp32, in place,
 * x += Wo window_attention(q | k | v of LayerNorm(x; gamma, beta, eps)) + bo. wqkv (3 * C, C) (rows q | k | v) and wo (C, C)
 * as split pairs (ocm_op_cast_split); rel_table: (2*ws-1)^2 x heads fp32 device table; scratch: heads * 4096 floats of device
 * memory, plus batch * height * width * C floats with 4 or 6 heads. Built for OCM_PREC_BF16X3 and 3 heads (C = 96, stage 0 of
 * Swin-T: one kernel), 4 heads (C = 128) or 6 heads (C = 192, stage 1 of Swin-T): one kernel up to the context + the o_proj GEMM;
 * anything else — windows above 7 included — returns OCM_EINVAL. */
int ocm_op_swin_attn_block(int32_t precision, float *x, const float *gamma, const float *beta, const void *wqkv,
                           const float *bqkv, const void *wo, const float *bo, const float *rel_table, float *scratch,
                           int32_t batch, int32_t height, int32_t width, int32_t window, int32_t shift, int32_t heads, float eps,
                           void *stream);

/* Stand-alone (shifted-)window attention of one SwinLayer (modeling_swin.py:529-563 without the projections):
 * qkv (B*H*W, ld) holds q | k | v (heads*32 channels each) per token in E = bf16 / fp32 / split-bf16 pairs (`precision`; pairs: ld and ldc multiples of 32);
 * ctx (B*H*W, ldc) receives softmax(q k^T / sqrt(32) + bias + shift mask) v at the token's own row.
 * rel_table: (2*ws-1)^2 x heads fp32 device table; scratch: ocm_swin_window_scratch_floats(window, heads) floats of device
 * memory. Windows of 2 to 7 run one wavefront per (window, head) (two 32-query tiles, two 32-key halves); windows of 8 to 12
 * (64 .. 144 positions) one workgroup of ceil(ws^2 / 32) wavefronts per (window, head): K and V of the window staged in LDS once,
 * each wavefront 32 queries against every 32-key sub-tile, scores in registers, exact two-pass softmax, the head's bias table
 * in LDS; bf16 and pairs on the bf16 MFMA, fp32 on the exact-fp32 MFMA. Above 7, ld and ldc are whole 16-byte pieces (8 bf16 /
 * 4 fp32 elements / groups of 32 pairs) with ld >= 3 * 32 * heads and ldc >= 32 * heads; anything else returns OCM_EINVAL. */
int ocm_op_swin_window_attention(int32_t precision, const void *qkv, int32_t ld, void *ctx, int32_t ldc,
                                 const float *rel_table, float *scratch, int32_t batch, int32_t height, int32_t width,
                                 int32_t window, int32_t shift, int32_t heads, void *stream);

/* Scratch floats of ocm_op_swin_window_attention / ocm_op_swin_window_probs (a host function; 0 for a window outside [2, 12] or
 * heads <= 0). window <= 7: heads * (4096 + ws^4) — the bias permuted into the kernels' register order, heads * 4096 floats,
 * then the dense [head][ws^2][ws^2] table. window 8 .. 12: heads * 544 — [head][bin] = rel_table[bin][head] * log2(e) for the
 * (2*ws-1)^2 <= 529 bins, bin = (dy + ws - 1) * (2*ws - 1) + (dx + ws - 1) with (dy, dx) = query - key position, zeros behind.
 * The operators fill the scratch themselves on every call. */
size_t ocm_swin_window_scratch_floats(int32_t window, int32_t heads);

/* The probabilities of those windows as an output (transformers' per-layer `attentions`): the arguments and argument domain of
 * ocm_op_swin_window_attention (qkv rows with ld >= 3 * 32 * heads in whole 16-byte pieces, rel_table, the same scratch, all
 * three precisions), and probs (batch * nW, heads, ws^2, ws^2) fp32, 16-byte aligned = softmax(q k^T / sqrt(32) + bias + shift
 * mask), windows of the grid rolled by -shift in window_partition order, tokens row-major inside a window. Scores are computed
 * from the element format as the attention kernel of that precision computes them (bf16 and pairs on MFMA, three instructions
 * per product for pairs; fp32 by FMAs), the softmax is fp32; the -100 mask is additive as in transformers (masked entries are
 * ~4e-44 or 0). One workgroup per (window, head) stages its block in LDS and writes it linearly (windows of 8 to 12: each of
 * its wavefronts the 32 x ws^2 rows of its query tile, with the score path of the wide attention kernel); no atomics and a
 * fixed summation order: reruns give the same bits. */
int ocm_op_swin_window_probs(int32_t precision, const void *qkv, int32_t ld, float *probs, const float *rel_table,
                             float *scratch, int32_t batch, int32_t height, int32_t width, int32_t window, int32_t shift,
                             int32_t heads, void *stream);

/* x (batch, tokens, channels) fp32 token-major -> out (batch, channels, tokens): hidden.transpose(1, 2), i.e. the
 * (B, C, H, W) feature map of a stage (32 x 32 LDS tiles, coalesced on both sides; any positive sizes, batch <= 65535). */
int ocm_op_swin_tokens_to_nchw(const float *x, float *out, int32_t batch, int32_t tokens, int32_t channels, void *stream);

/* The LayerNorm of SwinPatchMerging (modeling_swin.py:309-326, before the reduction): x (batch, height, width, channels) fp32;
 * y (batch * ceil(height / 2) * ceil(width / 2), ldy) operand rows in the precision's element format (fp32, bf16 or split pairs)
 * = LayerNorm(x0 | x1 | x2 | x3; gamma, beta, 1e-5) of the 2 x 2 neighbourhood, an odd side padded with zeros, columns
 * [4 * channels, ldy) zero. channels a multiple of 32 up to 512; ldy >= 4 * channels, a multiple of 64 (bf16) or 32. */
int ocm_op_swin_merge_ln(int32_t precision, const float *x, const float *gamma, const float *beta, void *y, int32_t batch,
                         int32_t height, int32_t width, int32_t channels, int32_t ldy, void *stream);

/* ---- training (SwinForImageClassification fine-tuning, train.py's Trainer loop; kernels_swin_train.hip) ----
 * The training forward runs the stand-alone operators (ocm_op_layernorm, ocm_op_linear, ocm_op_swin_window_attention,
 * ocm_op_gelu, ocm_op_swin_merge_ln); its backward the ViT training operators of ocm_vit.h plus the entry points below.
 * Gradients are fp32; every sum runs in an order fixed by the shapes, without atomics, so reruns give the same bits.
 * Null pointers and bad shapes return OCM_EINVAL. */

/* Backward of ocm_op_swin_window_attention for 32-wide heads and windows of 2 to 7: qkv (B*H*W, 3 * 32 * heads) fp32 q | k | v
 * per token in row-major token order, dctx (B*H*W, 32 * heads) fp32, rel_table (2*ws-1)^2 x heads fp32
 *   -> dqkv (B*H*W, 3 * 32 * heads) fp32 in the q | k | v column order of q_proj / k_proj / v_proj (every element written)
 *      and dtable (2*ws-1)^2 x heads = the sum over images, windows and position pairs of dS in each relative-position bin.
 * S = q k^T / sqrt(32) + bias + shift mask (transformers' -100 additive mask) and P = softmax(S) are recomputed in fp32.
 * One workgroup owns a (window, head) pair; the table gradient is per-window partials plus a fixed-order column sum in the
 * workspace (ocm_swin_window_attention_backward_workspace_bytes). height and width multiples of window, 0 <= shift < window. */
size_t ocm_swin_window_attention_backward_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t window,
                                                          int32_t heads);
int ocm_op_swin_window_attention_backward(const float *qkv, const float *dctx, const float *rel_table, float *dqkv, float *dtable,
                                          int32_t batch, int32_t height, int32_t width, int32_t window, int32_t shift,
                                          int32_t heads, void *workspace, size_t workspace_bytes, void *stream);

/* The same backward for windows of 8 to 12 (ws^2 = 64 .. 144 positions; the window12-384 checkpoints): the arguments, outputs and
 * recomputation of ocm_op_swin_window_attention_backward, qkv / dctx / dqkv 16-byte aligned. One workgroup of ceil(ws^2 / 32)
 * wavefronts owns a (window, head) pair; all five products (S = q k^T, dP = dO v^T, dQ = dS k, dK = dS^T q, dV = P^T dO) run on
 * the exact-fp32 MFMA in every precision mode, padding key slots contribute exact zeros, no atomics, reruns give the same bits.
 * Workspace: (nwin + ceil(nwin / 64)) * (2*ws-1)^2 * heads * 4 bytes with nwin = batch * (height / ws) * (width / ws) — the
 * per-window bin partials and the first level of their fixed-order column sum; 0 for a window outside 8 .. 12 or a non-positive
 * size. OCM_EINVAL: a window outside 8 .. 12, a grid that is not a multiple of the window, shift >= window, null pointers, a
 * short workspace, more than 2^31 (window, head) pairs. */
size_t ocm_swin_window_attention_backward_wide_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t window,
                                                               int32_t heads);
int ocm_op_swin_window_attention_backward_wide(const float *qkv, const float *dctx, const float *rel_table, float *dqkv,
                                               float *dtable, int32_t batch, int32_t height, int32_t width, int32_t window,
                                               int32_t shift, int32_t heads, void *workspace, size_t workspace_bytes, void *stream);

/* SwinPatchMerging's 2 x 2 gather (modeling_swin.py:309-326) as fp32 rows, even height and width only:
 * y (batch * height/2 * width/2, 4 * channels) = x0 | x1 | x2 | x3 of x (batch, height, width, channels) fp32 — the merging
 * LayerNorm's input; and its inverse in gather form, dx (batch, height, width, channels) from dy of y's shape (bit exact). */
int ocm_op_swin_merge_gather(const float *x, float *y, int32_t batch, int32_t height, int32_t width, int32_t channels,
                             void *stream);
int ocm_op_swin_merge_scatter(const float *dy, float *dx, int32_t batch, int32_t height, int32_t width, int32_t channels,
                              void *stream);

/* ---- the padded geometries in training (SwinLayer.maybe_pad, SwinPatchMerging.maybe_pad). Byte-moving and bit exact: 16-byte
 * accesses (every pointer 16-byte aligned), one writer per output element, every output byte written. ----
 * ocm_op_swin_pad_rows: rows of row_bytes bytes (a positive multiple of 16) in any element format (fp32, bf16, split pairs),
 * src (batch, height, width, row) -> dst (batch, height_pad, width_pad, row), zeros at the positions right of and below the grid
 * (the kernel the engine runs on its padded geometries). ocm_op_swin_crop_rows: the inverse, src (batch, height_pad, width_pad,
 * row) -> dst (batch, height, width, row); each is the other's backward. height_pad >= height, width_pad >= width. */
int ocm_op_swin_pad_rows(const void *src, void *dst, int32_t batch, int32_t height, int32_t width, int32_t height_pad,
                         int32_t width_pad, size_t row_bytes, void *stream);
int ocm_op_swin_crop_rows(const void *src, void *dst, int32_t batch, int32_t height, int32_t width, int32_t height_pad,
                          int32_t width_pad, size_t row_bytes, void *stream);

/* ocm_op_swin_merge_gather / _scatter for any positive sides, channels a multiple of 4: y (batch * ceil(height / 2) *
 * ceil(width / 2), 4 * channels) = x0 | x1 | x2 | x3 with zeros where the 2 x 2 neighbourhood leaves the grid (an odd side is
 * padded by one zero row / column); the scatter is its transpose: every element of dx (batch, height, width, channels) is
 * written, and what dy holds at the appended positions is dropped. On even sides both give the bits of the pair above. */
int ocm_op_swin_merge_gather_pad(const float *x, float *y, int32_t batch, int32_t height, int32_t width, int32_t channels,
                                 void *stream);
int ocm_op_swin_merge_scatter_pad(const float *dy, float *dx, int32_t batch, int32_t height, int32_t width, int32_t channels,
                                  void *stream);

/* The pooled head: pooled (batch, channels) = the token mean of x (batch, tokens, channels) fp32, tokens summed in order;
 * its backward dx (batch, tokens, channels) = dpooled / tokens broadcast over the tokens. */
int ocm_op_swin_pool(const float *x, float *pooled, int32_t batch, int32_t tokens, int32_t channels, void *stream);
int ocm_op_swin_pool_backward(const float *dpooled, float *dx, int32_t batch, int32_t tokens, int32_t channels, void *stream);

/* Stochastic depth on the attention branch (SwinDropPath, modeling_swin.py:567): out = x + branch * scale[image] (out may alias
 * x), scale = mask / keep_prob per image, all (batch, tokens, channels) fp32 but scale (batch); and the branch's gradient
 * dbranch = dout * scale[image] (the residual passes dout unchanged). */
int ocm_op_swin_drop_path(const float *x, const float *branch, const float *scale, float *out, int32_t batch, int32_t tokens,
                          int32_t channels, void *stream);
int ocm_op_swin_drop_path_backward(const float *dout, const float *scale, float *dbranch, int32_t batch, int32_t tokens,
                                   int32_t channels, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OCM_SWIN_H */
