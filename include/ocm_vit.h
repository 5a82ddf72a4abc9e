/*
 * ocm_vit.h — C ABI of the MI355X (gfx950) ViT attention-map engine.
 *
 * The reference (linum-uqam/ViT-OCM-WMSegmentation) has NO native/FFI layer: its
 * boundary is the Python nn.Module surface of
 *   Self-supervised_segmentation/dino/vision_transformer.py
 * (SURVEY.md §8-b).  This header is therefore the ABI that the build's Python
 * mirror of that module binds through ctypes; every entry point names the
 * reference lines whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.
 *   - every pointer marked "dev" is a device (HBM) pointer owned by the caller
 *     unless stated otherwise; nothing here allocates caller-visible memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). No entry
 *     point synchronises the device; all work is enqueued on `stream`.
 *   - return value: 0 = OCM_OK, otherwise an OCM_E* code; ocm_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - thread-compatible: one ocm_vit_t per model, no globals besides the
 *     thread-local error string.
 */
#ifndef OCM_VIT_H
#define OCM_VIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCM_ABI_VERSION 20

enum {
    OCM_OK = 0,
    OCM_EINVAL = 1,     /* bad argument / unsupported shape (Python: ValueError)      */
    OCM_ESTATE = 2,     /* parameter missing, handle not ready (Python: RuntimeError) */
    OCM_EHIP = 3,       /* HIP runtime / launch failure (Python: RuntimeError)        */
    OCM_ENOMEM = 4,     /* workspace too small / allocation failure                    */
    OCM_ENAME = 5       /* unknown parameter name (Python: KeyError)                   */
};

/* Arithmetic of the contraction kernels. The residual stream, LayerNorm
 * statistics, softmax and all accumulators are fp32 in every mode. */
enum {
    OCM_PREC_BF16 = 0, /* bf16 operands, v_mfma_f32_32x32x16_bf16, fp32 accumulate (fast path)            */
    OCM_PREC_FP32 = 1, /* fp32 operands, v_mfma_f32_32x32x2_f32: exact fp32 products, 1/16 the MFMA rate;
                          matrices, activations, q/k/v and P stay fp32 end to end (reference-grade maps) */
    OCM_PREC_BF16X3 = 2 /* split-bf16: every operand is a pair x = hi + lo of bf16 numbers (2^-17 relative) and every
                          product runs as three v_mfma_f32_32x32x16_bf16 (hi*hi + hi*lo + lo*hi), fp32 accumulate:
                          attention maps within 1e-3 of the fp32 reference on every golden weight set whose softmax is
                          not saturated — the trained-like sets of all three geometries, attention max 0.79 .. 0.96,
                          where single bf16 reaches 6e-2 — at ~3x the MFMA work of OCM_PREC_BF16 instead of 16x
                          (on a saturated softmax, attention max 1.0000, fp32 arithmetic itself is 5e-4 from
                          float64 and this mode 2-5e-3: DESIGN.md section 5). Split tensors ("E = split pairs" below) keep 4 bytes per element: the
                          contraction axis is cut into groups of 32 elements stored as 128 bytes
                          [32 x bf16 hi | 32 x bf16 lo] (ocm_op_cast_split / ocm_op_merge_split convert). */
};

/* Hyper-parameters: VisionTransformer.__init__ (vision_transformer.py:137-165) and
 * the vit_tiny/small/base factories (:259-279). head_dim = embed_dim/num_heads = 64 (T/S/B) runs the MFMA attention
 * kernels; any other multiple of 8 (the SimMIM encoder of model.py:93-103: 3 heads of 128) runs the fp32 attention
 * of kernels_attn.hip::attn_generic_kernel. */
typedef struct ocm_vit_config {
    int32_t patch_size;   /* p: 8 or 16 (any multiple of 8 up to 32)                   */
    int32_t in_chans;     /* 3 (reference) or 1 (grayscale-folded patch embedding)     */
    int32_t embed_dim;    /* D, multiple of 64                                         */
    int32_t depth;        /* L                                                         */
    int32_t num_heads;    /* H; head_dim = D/H                                         */
    int32_t mlp_hidden;   /* int(D*mlp_ratio), multiple of 64                          */
    float ln_eps;         /* 1e-6 for the DINO factories (:262,268,277)                */
    float qk_scale;       /* head_dim^-0.5 unless qk_scale was given (:71)             */
    int32_t precision;    /* OCM_PREC_*                                                */
    int32_t reserved;
} ocm_vit_config;

typedef struct ocm_vit ocm_vit_t; /* opaque engine handle */

/* ---- library --------------------------------------------------------------- */
int ocm_abi_version(void);
const char *ocm_last_error(void);

/* ---- handle life cycle ----------------------------------------------------- */
int ocm_vit_create(const ocm_vit_config *cfg, ocm_vit_t **out);
void ocm_vit_destroy(ocm_vit_t *h);

/* Upload one parameter. `name` is the reference state_dict key:
 *   cls_token, patch_embed.proj.{weight,bias}, blocks.{i}.norm1.{weight,bias},
 *   blocks.{i}.attn.qkv.{weight,bias}, blocks.{i}.attn.proj.{weight,bias},
 *   blocks.{i}.norm2.{weight,bias}, blocks.{i}.mlp.fc1.{weight,bias},
 *   blocks.{i}.mlp.fc2.{weight,bias}, norm.{weight,bias}
 * and, optionally, mask_token (model.py:16; only needed when ocm_vit_io.patch_mask is used)
 * (`pos_embed` is passed per forward, see ocm_vit_io.pos_embed).
 * `dev_src` is a contiguous fp32 device buffer of `count` elements in the
 * reference's layout; the engine keeps its own packed (bf16 for matrices, fp32
 * for vectors) copy, so the source may be freed after the stream has run. */
int ocm_vit_set_param(ocm_vit_t *h, const char *name, const float *dev_src, size_t count,
                      void *stream);
/* Per-handle dispatch options (this handle only; no process-wide state). 0 is always "automatic".
 *   OCM_OPT_FUSE_LN  attn.proj / mlp.fc2 + residual fused with the LayerNorm that follows (one full-row kernel, bit
 *                    identical to the GEMM + LayerNorm pair): 0 = where it is faster (>= 8192 token rows and fewer than
 *                    512 tiles of 128 x 128 in the output), 1 = never, 2 = whenever the embedding width has the kernel
 *                    (ocm_linear_resid_ln_supported).
 *   OCM_OPT_FOLD_LN  (OCM_PREC_BF16X3 engines) LayerNorm folded into the GEMM that consumes it: the residual stream is
 *                    handed over un-normalised as split pairs with per-row sums, the consumer multiplies by W * gamma
 *                    and finishes rstd * (acc - mu * c) + d in its epilogue — no LayerNorm launches, no full-row tiles.
 *                    0 = where it is faster (forwards whose (T x D) output holds fewer than 512 tiles of 128 x 128; the
 *                    block-level entry points keep the LayerNorm kernels), 1 = never, 2 = in every ocm_vit_forward. */
enum { OCM_OPT_FUSE_LN = 0, OCM_OPT_FOLD_LN = 1, OCM_OPT_COUNT = 2 };
int ocm_vit_set_option(ocm_vit_t *h, int32_t option, int32_t value);
/* 0 when every parameter has been set, else OCM_ESTATE with the first missing
 * name in ocm_last_error(). */
int ocm_vit_params_ready(const ocm_vit_t *h);

/* ---- forward --------------------------------------------------------------- */
enum {
    OCM_OUT_FEAT = 1 << 0,      /* norm(x) of the last n blocks       (get_intermediate_feat :234)  */
    OCM_OUT_ATTN = 1 << 1,      /* softmax probabilities (B,H,N,N)    (Attention.forward :83-85)    */
    OCM_OUT_QKV = 1 << 2,       /* (3,B,H,N,64) fp32                  (Attention.forward :80)       */
    OCM_OUT_TOKENS = 1 << 3,    /* raw residual stream after the last block (no final norm)         */
    OCM_OUT_ROWS = 1 << 4,      /* selected query rows of the last block's attention, CLS column
                                   dropped: (B,H,n_rows,N-1)          (utils.py:229-233)            */
    OCM_LAST_ATTN_ONLY = 1 << 5,/* get_last_selfattention (:239-246): the last block stops after
                                   its attention probabilities; FEAT/TOKENS/QKV must not be set.    */
    OCM_OUT_FMAP = 1 << 6,      /* norm(x)[:, 1:] as a (B,D,hp,wp) feature map — what the encoders of
                                   model.py:48-53,134-139 return                                   */
    OCM_USE_GRAPH = 1 << 7      /* launch through a cached hipGraph: the forward's ~80 kernel launches are
                                   captured once and replayed with one hipGraphLaunch while shapes, flags
                                   and every pointer in the io block stay the same (the steady state of the
                                   reference's one-tile-per-call loops); otherwise the graph is re-captured
                                   and updated in place. Same results, less host time per call.        */
};

/* One batch of tiles through prepare_tokens + blocks [+ final norm].
 * Tiles are p-aligned windows of fp32 planar images resident in HBM:
 *   pixel(b, c, y, x) = image[ b*img_stride_b + c*img_stride_c
 *                              + (y0_b + y)*img_stride_y + (x0_b + x) ]
 * where (y0_b, x0_b) = tile_origins[2b], tile_origins[2b+1] when tile_origins is
 * non-NULL and (0,0) otherwise.  A contiguous (B,3,H,W) torch tensor is
 * {stride_b = 3HW, stride_c = HW, stride_y = W}; a sliding-window sweep over one
 * slab uses stride_b = 0 and per-tile origins (sw_processing.py:151-163).
 * Strides are in elements.  x origins, img_stride_y and the base pointer must
 * keep every patch row 16-byte aligned (x0 % 4 == 0, stride_y % 4 == 0). */
typedef struct ocm_vit_io {
    const float *image;          /* dev */
    int64_t img_stride_b, img_stride_c, img_stride_y;
    const int32_t *tile_origins; /* dev, [batch][2] = (y0, x0), or NULL */
    int32_t batch;               /* B                                               */
    int32_t tile_h, tile_w;      /* pixels, multiples of patch_size                 */
    const float *pos_embed;      /* dev, [N][D] fp32: row 0 = cls position, rows 1.. = (interpolated)
                                    patch positions for this tile shape (:176-196)  */
    int32_t flags;               /* OCM_OUT_* | OCM_LAST_ATTN_ONLY                  */
    int32_t n_last;              /* n of get_intermediate_feat / get_intermediate_layers (>=1) */
    float *out_feat;             /* dev, [n_last][B][N][D]            or NULL       */
    float *out_attn;             /* dev, [n_last][B][H][N][N]         or NULL       */
    float *out_qkv;              /* dev, [n_last][3][B][H][N][hd]     or NULL       */
    float *out_tokens;           /* dev, [B][N][D]                    or NULL       */
    const int32_t *query_rows;   /* dev, [n_rows] token indices (0 = CLS) or NULL   */
    int32_t n_rows;
    int32_t reserved;
    float *out_rows;             /* dev, [B][H][n_rows][N-1]          or NULL       */
    const float *patch_mask;     /* dev, [B][P] fp32 SimMIM mask w or NULL: patch rows become
                                    x*(1-w) + mask_token*w before cls/pos (model.py:28-33); needs the
                                    optional parameter "mask_token"                 */
    float *out_fmap;             /* dev, [B][D][hp][wp]               or NULL       */
    void *workspace;             /* dev, >= ocm_vit_workspace_bytes(h, batch, N)    */
    size_t workspace_bytes;
    void *stream;                /* hipStream_t                                     */
} ocm_vit_io;

/* Bytes of scratch HBM one forward of `batch` tiles with `n_tokens` = N needs. */
size_t ocm_vit_workspace_bytes(const ocm_vit_t *h, int32_t batch, int32_t n_tokens);

/* VisionTransformer.get_intermediate_feat / get_last_selfattention / forward_feats /
 * get_intermediate_layers (vision_transformer.py:211-256), selected by io->flags. */
int ocm_vit_forward(ocm_vit_t *h, const ocm_vit_io *io);

/* Counters of the OCM_USE_GRAPH path: forwards replayed from the cached graph / graph (re-)captures. */
int ocm_vit_graph_stats(const ocm_vit_t *h, uint64_t *replays, uint64_t *captures);

/* VisionTransformer.prepare_tokens (:198-209): patch embedding + cls + pos.
 * Uses image/strides/origins/batch/tile_*, pos_embed and stream of `io`;
 * writes x_out[B][N][D] fp32. */
int ocm_vit_prepare_tokens(ocm_vit_t *h, const ocm_vit_io *io, float *x_out);

/* Block.forward (:106-114) of block `index`, in place on x[B][N][D] fp32.
 * flags: OCM_OUT_ATTN / OCM_OUT_QKV fill out_attn (B,H,N,N) / out_qkv (3,B,H,N,64);
 * OCM_LAST_ATTN_ONLY returns after the probabilities (return_attention=True). */
int ocm_vit_block_forward(ocm_vit_t *h, int32_t index, float *x, int32_t batch, int32_t n_tokens,
                          int32_t flags, float *out_attn, float *out_qkv, void *workspace,
                          size_t workspace_bytes, void *stream);

/* self.norm (:158, :214, :221, :234): y = LayerNorm(x) over rows of D, fp32 out. */
int ocm_vit_final_norm(ocm_vit_t *h, const float *x, float *y, int64_t rows, void *stream);

/* ---- stand-alone operators (kernel-level parity tests; same kernels the engine uses) ---- */

/* nn.LayerNorm(D, eps) (:98,102,158). y is fp32, bf16 or split pairs (dim % 32 == 0) by `out_kind`. */
enum { OCM_LN_F32 = 0, OCM_LN_BF16 = 1, OCM_LN_SPLIT = 2 };
int ocm_op_layernorm(const float *x, const float *gamma, const float *beta, void *y,
                     int32_t out_kind, int64_t rows, int32_t dim, float eps, void *stream);

/* fp32 -> bf16 (round-to-nearest-even) of `count` elements. */
int ocm_op_cast_bf16(const float *src, void *dst_bf16, size_t count, void *stream);
/* fp32 -> split pairs and back (hi + lo in fp32); `count` % 32 == 0, dst of 4*count bytes. Rows whose length is a
 * multiple of 32 keep their row structure (row r starts at byte r * 4 * row_len). */
int ocm_op_cast_split(const float *src, void *dst_split, size_t count, void *stream);
int ocm_op_merge_split(const void *src_split, float *dst, size_t count, void *stream);

enum {
    OCM_EPI_BIAS_F32 = 0,       /* out fp32 [M][N] = acc + bias                                  */
    OCM_EPI_BIAS_RESID_F32 = 1, /* out fp32 [M][N] = resid + acc + bias   (proj/fc2 + skip :110) */
    OCM_EPI_BIAS_GELU_BF16 = 2, /* out bf16 [M][N] = gelu_erf(acc + bias) (fc1 + act :58-59)     */
    OCM_EPI_BIAS_BF16 = 3       /* out bf16 [M][N] = acc + bias                                  */
};
/* The stand-alone contraction operators take `precision` (OCM_PREC_*): operand / activation buffers
 * named E are bf16 for OCM_PREC_BF16, fp32 for OCM_PREC_FP32 and split pairs for OCM_PREC_BF16X3 (the *_BF16
 * epilogues then emit E). */

/* nn.Linear: out = epilogue(A[M][K] · W[N][K]^T + bias[N]); A, W of type E row-major,
 * K % 64 == 0 (bf16) or K % 32 == 0 (fp32, split pairs), N % 32 == 0. resid may alias out. */
int ocm_op_linear(int32_t precision, const void *a, const void *w, const float *bias, const float *resid,
                  void *out, int32_t M, int32_t N, int32_t K, int32_t epilogue, void *stream);

/* nn.Linear + residual with the NEXT LayerNorm's row sums (the engine's attn.proj / mlp.fc2 when that LayerNorm is folded into
 * its consumer): x[M][N] fp32 += A · W^T + bias in place; xs[M][N] of type E = x - shift[row]; stats[M][N / 64][2] fp32 = per row
 * (sum, sum of squares) of x - shift[row], carried by the first 64-column slot of every tile, zeros in the tile's other slots.
 * shift[M] (or NULL: nothing is subtracted) is WRITTEN: prev_shift[row] + (sum over slots of prev_stats[row][.][0]) / N, either
 * previous-site input may be NULL (then it counts as zero). N % 64 == 0, K as for ocm_op_linear. */
int ocm_op_linear_stats(int32_t precision, const void *a, const void *w, const float *bias, float *x, void *xs, float *stats,
                        float *shift, const float *prev_stats, const float *prev_shift, int32_t M, int32_t N, int32_t K,
                        void *stream);

/* nn.Linear + residual + LayerNorm in one kernel (Block.forward :107-111 with the NEXT normalisation folded in:
 *   x = resid + A[M][K] · W[D][K]^T + bias;   xn = LayerNorm(x; gamma, beta, eps) in the activation type E
 * exactly as ocm_op_linear (epilogue RESID_F32) followed by ocm_op_layernorm would produce them (bit for bit).
 * A workgroup owns whole rows, so D is one of 128 / 256 / 384 (ocm_linear_resid_ln_supported). resid may
 * alias x. The engine uses it for attn.proj -> norm2 and mlp.fc2 -> the next block's norm1 when M >= 8192. */
int ocm_linear_resid_ln_supported(int32_t D);
int ocm_op_linear_resid_ln(int32_t precision, const void *a, const void *w, const float *bias, const float *resid,
                           float *x, const float *gamma, const float *beta, void *xn, int32_t M, int32_t D, int32_t K,
                           float eps, void *stream);

/* Which kernel a GEMM-shaped operator launches for a shape: the library's own tile dispatch (csrc/gemm_plan.h), asked without
 * launching anything. Host only: no device is touched, so it also answers on a machine without a GPU. It makes the very call
 * the launchers make (a plan is a function of the shape alone).
 *   family     M, N, K of the GEMM                                    operators
 *   LINEAR     M, N, K; epilogue OCM_EPI_* (4: the ReLU epilogue)     ocm_op_linear, ocm_op_linear_relu, the engines' nn.Linear layers
 *   QKV        M = batch * n_tokens, N = 3 D, K = D (D % 64 == 0)     ocm_op_qkv_proj[_hd]
 *   LINEAR_LD  M, N, K (bf16 / fp32 only)                             the Swin engine's strided nn.Linear
 *   CONV       M = batch * h * w, N = O (4 O: the up-convolution),    ocm_op_conv3x3 (K = 9 C, flag CONV3X3), ocm_op_conv3x3_image (K = 27),
 *              K = the contraction length before padding              ocm_op_upconv2x2 (K = C)
 *   RESID_LN   M, N = D in {128, 256, 384}, K % 64 == 0               ocm_op_linear_resid_ln
 * `epilogue` is read for LINEAR only. flags: STATS_EPILOGUE = the residual epilogue that also produces the next LayerNorm's row
 * sums (ocm_op_linear_stats and the engine's folded-LayerNorm forward; its tiles are multiples of 64 wide), SPLITK_OFFERED = the caller holds a split-K
 * workspace (the engine below 512 rows), CONV3X3 = the A operand comes through the 3x3 loader. Arguments the operator itself
 * refuses return OCM_EINVAL. */
enum { OCM_GEMM_LINEAR = 0, OCM_GEMM_QKV = 1, OCM_GEMM_LINEAR_LD = 2, OCM_GEMM_CONV = 3, OCM_GEMM_RESID_LN = 4 };
enum { OCM_PLAN_STATS_EPILOGUE = 1, OCM_PLAN_SPLITK_OFFERED = 2, OCM_PLAN_CONV3X3 = 4 };
typedef struct ocm_gemm_plan_info {
    int32_t bm, bn;   /* tile rows x columns                                                        */
    int32_t waves;    /* wavefronts per workgroup                                                   */
    int32_t mfma16;   /* 1: v_mfma_f32_16x16x32_bf16, 0: the 32 x 32 MFMA shapes                    */
    int32_t lds_dma;  /* main loop: 0 register-staged, 1 LDS-DMA ring                               */
    int32_t stages;   /* LDS buffers of (bm + bn) * 128 bytes: ring depth; 2 on the register-staged loop */
    int32_t ksteps;   /* compile-time K-step count of the kernel, 0: the run-time loop              */
    int32_t splitk;   /* K slices, 1: none                                                          */
} ocm_gemm_plan_info;
int ocm_gemm_plan(int32_t family, int32_t precision, int32_t epilogue, int32_t M, int32_t N, int32_t K, uint32_t flags,
                  ocm_gemm_plan_info *plan);

/* Head-major packed projections the attention kernels consume:
 *   q, k : E [B*H][n_pad][64];  vt : E [B*H][64][n_pad],  n_pad = ocm_n_pad_prec(precision, N)
 * (N rounded up to 8, or to 32 for split pairs: the key axis of V^T is a contraction axis). ocm_n_pad(N) is the
 * bf16 / fp32 value. */
int32_t ocm_n_pad(int32_t n_tokens);
int32_t ocm_n_pad_prec(int32_t precision, int32_t n_tokens);

/* Attention.forward qkv projection (:80): A[B*N][D] bf16 · Wqkv[3D][D]^T + b -> q/k/vt
 * (and, when qkv_f32 != NULL, the fp32 (3,B,H,N,64) tensor the reference returns). */
int ocm_op_qkv_proj(int32_t precision, const void *a, const void *w, const float *bias, void *q, void *k,
                    void *vt, float *qkv_f32, int32_t batch, int32_t n_tokens, int32_t heads,
                    void *stream);

/* softmax(q k^T * scale) v (:83-87). ctx E [B][N][H*64] (or NULL);
 * lse2 fp32 [B*H][N] = log2-domain log-sum-exp of the scaled scores (or NULL). */
int ocm_op_attention(int32_t precision, const void *q, const void *k, const void *vt, void *ctx, float *lse2,
                     int32_t batch, int32_t n_tokens, int32_t heads, float scale, void *stream);

/* Attention probabilities (:83-84) from q, k and lse2: attn fp32 [B][H][N][N]. */
int ocm_op_attention_probs(int32_t precision, const void *q, const void *k, const float *lse2, float *attn,
                           int32_t batch, int32_t n_tokens, int32_t heads, float scale,
                           void *stream);

/* Selected rows of the probabilities with the CLS column dropped
 * (utils.py:232, attentions[0, :, query, 1:]): rows fp32 [B][H][n_rows][N-1]. */
int ocm_op_attention_rows(int32_t precision, const void *q, const void *k, const int32_t *query_rows,
                          int32_t n_rows, float *rows, int32_t batch, int32_t n_tokens, int32_t heads, float scale,
                          void *stream);

/* The qkv projection, attention and probabilities for heads of `head_dim` channels: 64 (identical to the entry points
 * above) or 128 — the encoder the reference's build_model() constructs (Self-supervised_segmentation/model.py:93-103:
 * embed_dim 384, 3 heads) — in every precision (split-bf16 since round 3, fp32 and single bf16 since round 4). q / k are then
 * [B*H][n_pad][128] and vt [B*H][128][n_pad] in the operand type, ctx [B][N][H*128]. Any other width returns OCM_EINVAL (an
 * engine handle runs such heads on its generic fp32 attention kernel) — except that ocm_op_qkv_proj_hd with q = k = vt = NULL
 * fills only qkv_f32, for any head_dim that is a multiple of 8 (the input of ocm_op_attention_generic). D = heads * head_dim must
 * be a multiple of 64 in every precision (the projection's 64-wide column tiles cover q | k | v exactly). */
int ocm_op_qkv_proj_hd(int32_t precision, const void *a, const void *w, const float *bias, void *q, void *k, void *vt,
                       float *qkv_f32, int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, void *stream);
int ocm_op_attention_hd(int32_t precision, const void *q, const void *k, const void *vt, void *ctx, float *lse2,
                        int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, float scale, void *stream);
int ocm_op_attention_probs_hd(int32_t precision, const void *q, const void *k, const float *lse2, float *attn,
                              int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, float scale, void *stream);

/* Which kernel ocm_op_attention[_hd / _ws] and an engine handle launch for a shape: the library's own dispatch (csrc/attn_plan.h),
 * asked without launching anything. Host only: no device is touched, so it also answers on a machine without a GPU. It makes
 * the very call the launcher makes. workspace_bytes: the key-slice workspace the caller would offer
 * (0: none, as ocm_op_attention and ocm_op_attention_hd). Arguments the operators refuse return OCM_EINVAL. */
enum {
    OCM_ATTN_BF16_WHOLE = 0,    /* single bf16: the whole key range of one (image, head) in LDS, N <= 256            */
    OCM_ATTN_BF16_STREAM = 1,   /* single bf16: streaming flash kernel                                               */
    OCM_ATTN_FP32_STREAM = 2,   /* fp32: streaming flash kernel                                                      */
    OCM_ATTN_X3_WAVE_SPLIT = 3, /* split-bf16: one 32-query tile per workgroup, its four waves split the keys        */
    OCM_ATTN_X3_PIPELINED = 4,  /* split-bf16: software-pipelined four-wave kernel                                   */
    OCM_ATTN_X3_DMA = 5,        /* split-bf16: LDS-DMA ring (eight waves above 1024 tokens; four for 128-wide heads) */
    OCM_ATTN_X3_DMA_KSPLIT = 6  /* ... with the key range cut into grid_z slices, then the merge kernel              */
};
typedef struct ocm_attention_plan_info {
    int32_t kernel;   /* OCM_ATTN_*                                                                  */
    int32_t waves;    /* wavefronts per workgroup                                                    */
    int32_t stages;   /* LDS buffers per operand (ring depth); 1: the whole sequence resident        */
    int32_t kslices;  /* key slices, 1: none                                                         */
    int32_t grid_x, grid_y, grid_z;
    int32_t lds_bytes;        /* dynamic LDS of the launch                                           */
    uint64_t workspace_need;  /* bytes of the offered workspace the plan writes (0 without a split)  */
} ocm_attention_plan_info;
int ocm_attention_plan(int32_t precision, int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, size_t workspace_bytes,
                       ocm_attention_plan_info *plan);

/* ocm_op_attention_hd with a key-slice workspace ("ws" = workspace, not the wave-split kernel): what an engine handle does for a
 * long sequence in few workgroups (split-bf16, 64-wide heads, more than 1024 tokens, at most 128 eight-wave workgroups). The key
 * range is then cut into up to four slices that leave unnormalised partial results in `workspace`, and a merge kernel combines
 * them. ocm_attention_workspace_bytes is what to offer (0: this shape never splits; also 0 for arguments the operator refuses).
 * workspace: device memory, 16-byte aligned, or NULL; a workspace smaller than ocm_attention_plan's workspace_need is left
 * untouched and the call runs exactly as ocm_op_attention_hd. */
size_t ocm_attention_workspace_bytes(int32_t precision, int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim);
int ocm_op_attention_ws(int32_t precision, const void *q, const void *k, const void *vt, void *ctx, float *lse2, int32_t batch,
                        int32_t n_tokens, int32_t heads, int32_t head_dim, float scale, void *workspace, size_t workspace_bytes,
                        void *stream);

/* Attention for heads of ANY width (head_dim a multiple of 4, up to 512; at most 8192 tokens; heads * head_dim a multiple of 32
 * for a split-bf16 ctx; batch * heads at most 65535, the launch's grid y, which holds for an engine handle with such heads
 * too) on the fp32 tensor
 * qkv_f32 [3][B][H][N][head_dim] that ocm_op_qkv_proj_hd writes: plain fp32 FMAs, one wavefront per query row — what an engine
 * handle runs for head widths the MFMA kernels are not built for, and what the free-standing Attention module
 * (dino/vision_transformer.py:66-90 accepts any dim / num_heads) calls for them. ctx (optional): [B][N][H*head_dim] in the
 * operand type of `precision`; attn (optional): fp32 [B][H][N][N]. */
int ocm_op_attention_generic(int32_t precision, const float *qkv_f32, void *ctx, float *attn, int32_t batch,
                             int32_t n_tokens, int32_t heads, int32_t head_dim, float scale, void *stream);

/* compute_attention (utils.py:229-235) on device: attn fp32 [B][H][N][N] ->
 * maps fp32 [H][hf*p][wf*p] = nearest-neighbour x p upsample of attn[b, :, query, 1:]. */
int ocm_op_attention_map(const float *attn, float *maps, int32_t b, int32_t heads,
                         int32_t n_tokens, int32_t query, int32_t hf, int32_t wf, int32_t p,
                         void *stream);

/* ---- in-library kernel timing (diagnostic; process-wide, single host thread) --------------------
 * While enabled, every launch of a kernel class selected in `class_mask` is bracketed by two
 * hipEvents recorded on the launch stream (no host synchronisation). ocm_prof_end() waits for the
 * recorded events, returns per-class launch counts and summed device milliseconds, and disables
 * profiling. bench.py uses it for the live per-kernel duration behind its `roofline` object. */
enum {
    OCM_K_PATCH = 0, /* patch-embedding gather + GEMM                 */
    OCM_K_LN = 1,    /* LayerNorm                                      */
    OCM_K_QKV = 2,   /* qkv projection GEMM                            */
    OCM_K_ATTN = 3,  /* flash attention (scores + softmax + P.V)       */
    OCM_K_PROBS = 4, /* attention-probability materialisation / rows   */
    OCM_K_PROJ = 5,  /* attn.proj GEMM + residual                      */
    OCM_K_FC1 = 6,   /* mlp.fc1 GEMM + GELU                            */
    OCM_K_FC2 = 7,   /* mlp.fc2 GEMM + residual                        */
    OCM_K_COUNT = 8
};
int ocm_prof_begin(uint32_t class_mask, int32_t max_launches);
int ocm_prof_end(double *ms_per_class /*[OCM_K_COUNT]*/, int64_t *launches_per_class /*[OCM_K_COUNT]*/);

/* ---- sliding-window post-processing on device (SURVEY §8-f "next" rows 1-2; sw_processing.py) ---- */
/* :245 + :253-254 — rows (T,H,n_rows,P) CLS-row maps (row 0 used) -> maps (T,P):
 * head mean (sequential fp32, as np.mean(axis=0)) then per-window (v - min) / (max - min) * 255. */
int ocm_op_tile_postprocess(const float *rows, float *maps, int32_t tiles, int32_t heads, int32_t n_rows,
                            int32_t pixels, void *stream);
/* :255-257 — cv2.resize(INTER_LINEAR) x`scale` of (T,h,w) float32 maps: half-pixel centres, replicate
 * border, fp32 (cv2 is an un-vendored dependency: parity unpinned). */
int ocm_op_bilinear_upsample(const float *src, float *dst, int32_t tiles, int32_t h, int32_t w, int32_t scale,
                             void *stream);
/* Nearest-neighbour x`rep` of (T,h,w) float32 maps (index replication: compute_attention's nearest upsample utils.py:233,
 * the block values of the //8 *8 resize chain sw_processing.py:255-257, the patch mask of model.py:71): dst (T,h*rep,w*rep). */
int ocm_op_nearest_upsample(const float *src, float *dst, int32_t tiles, int32_t h, int32_t w, int32_t rep, void *stream);
/* concat_crops :113-149 — n x n row-major float32 windows (n*n, window, window) -> (S,S),
 * S = window + (n-1)*stride; ramp = np.linspace(1, 0, window - stride) as float64 on device.
 * Bit-exact with the reference's sequential stitcher. stride < window <= 3*stride. */
int ocm_op_stitch(const float *crops, float *out, const double *ramp, int32_t n, int32_t window,
                  int32_t stride, void *stream);
/* threshold() :43-48 — min_max_normalize -> *255 -> astype(uint8) and the 256-bin histogram of the result.
 * scratch: >= 2048 bytes of device memory. */
int ocm_op_normalize_u8(const float *img, int64_t count, void *scratch, uint8_t *out, uint64_t *hist256,
                        void *stream);
/* cv2.threshold(img, 0, 255, THRESH_BINARY + THRESH_OTSU) :62 — host part: Otsu level of a histogram
 * (restates OpenCV's getThreshVal_Otsu_8u; parity unpinned), and the binary mask on device. */
int32_t ocm_otsu_threshold(const uint64_t *hist256_host, int64_t count);
int ocm_op_threshold_u8(const uint8_t *img, uint8_t *mask, int64_t count, int32_t thresh, void *stream);

/* sw_processing.py:224-227 — the stitched image of the windows, as the reference builds it for threshold():
 * concat_crops on the uint8 RGB windows (float64 blend, TRUNCATED into the uint8 overlap array at every fold), then
 * PIL .convert("L"). `image`: the float slab planes (x = u / 255 as ToTensor made them; 1 or 3 planes, strides in
 * elements), height x width pixels; windows that reach past the slab are zero-filled (PIL crop). out: (S,S) uint8,
 * S = window + (n-1)*stride; hist256 optional. */
int ocm_op_stitch_image_u8(const float *image, int64_t stride_c, int64_t stride_y, int32_t chans, int32_t height,
                           int32_t width, uint8_t *out, const double *ramp, int32_t n, int32_t window, int32_t stride,
                           uint64_t *hist256, void *stream);
/* sw_processing.py:42-48 — attention = min_max_normalize(heat); result = (img * attention / max(attention)).astype(uint8)
 * (float32 arithmetic, truncation) and att_u8 = (attention * 255).astype(uint8), with both 256-bin histograms.
 * scratch: >= 2048 bytes. */
int ocm_op_weighted_u8(const float *heat, const uint8_t *img, int64_t count, void *scratch, uint8_t *result,
                       uint8_t *att_u8, uint64_t *hist_result, uint64_t *hist_att, void *stream);

/* 256-bin histogram of a uint8 image (input of the Otsu levels when the image arrives as uint8). */
int ocm_op_histogram_u8(const uint8_t *img, int64_t count, uint64_t *hist256, void *stream);

/* eval.py:144,158 — scipy.ndimage.median_filter(map, size): size x size footprint, mode "reflect", upper median.
 * (T,h,w) fp32 -> (T,h,w); src != dst. Pinned against scipy (tests/golden/median.npz). */
int ocm_op_median_filter(const float *src, float *dst, int32_t tiles, int32_t h, int32_t w, int32_t size, void *stream);
/* eval.py:169, sw_processing.py:255 — cv2.resize(map, (w/f, h/f)) (INTER_LINEAR) for an integer factor: the two
 * centre pixels averaged per axis in float32 (cv2: parity unpinned). (T,h,w) -> (T,h/f,w/f). */
int ocm_op_downscale_centre(const float *src, float *dst, int32_t tiles, int32_t h, int32_t w, int32_t factor,
                            void *stream);

/* ---- eval.py's per-image mask chain (eval.py:126-171, utils.py:55-115 threshold()) ---- */
/* eval.py:142 — np.mean(attention_response, axis=0): rows (T,H,n_rows,P) -> maps (T,P), sequential fp32. */
int ocm_op_head_mean(const float *rows, float *maps, int32_t tiles, int32_t heads, int32_t n_rows,
                     int32_t pixels, void *stream);
/* eval.py:122,166 — transform(img).convert("L"): float planes (1 or 3, `stride_c` elements apart) ->
 * uint8 by mul(255).byte() and PIL's integer RGB->L weights; optional 256-bin histogram. */
int ocm_op_image_to_gray_u8(const float *image, int64_t stride_c, int32_t chans, int64_t count, uint8_t *out,
                            uint64_t *hist256, void *stream);
/* utils.py:76-81 — result = ((img / 2) * (1 - alpha) + (attention / 2) * alpha).astype(uint8) in float64;
 * `one_minus_alpha` is the host's own (1 - alpha) double. Optional histogram of the result. */
int ocm_op_blend_u8(const uint8_t *img, const uint8_t *att, int64_t count, double alpha, double one_minus_alpha,
                    uint8_t *out, uint64_t *hist256, void *stream);

/* ---- decoder head of model.py:60-66,147-152: Conv2d(D, s*s*C_out, 1) + PixelShuffle(s) ---- */
/* lin: (B*hp*wp, s*s*c_out) fp32 = the 1x1 conv evaluated token-major (ocm_op_linear on the normed patch
 * tokens); out: (B, c_out, hp*s, wp*s) with out[b][c][y*s+i][x*s+j] = lin[b*hp*wp + y*wp + x][c*s*s + i*s + j]. */
int ocm_op_pixel_shuffle(const float *lin, float *out, int32_t batch, int32_t hp, int32_t wp, int32_t c_out,
                         int32_t s, void *stream);

/* ---- two-layer decoder of model.py:154-166: Conv2d(3x3, padding 1) as im2col + ocm_op_linear ---- */
/* in: token-major fp32 [B][h*w][C] (C % 32 == 0); out: operand rows E [B*h*w][9*C], K index (ky*3 + kx)*C + c, zeros
 * outside the image; relu != 0 applies max(x, 0) on the way (the nn.ReLU in front of the second convolution). The
 * matching weight is the (O, C, 3, 3) kernel permuted to (O, 3, 3, C). */
int ocm_op_im2col3x3(int32_t precision, const float *in, void *out, int32_t batch, int32_t h, int32_t w,
                     int32_t channels, int32_t relu, void *stream);

/* ---- U-Net inference (model.py:227-320: build_unet; kernels_conv.hip) ----
 * Activations are fp32 and token-major (NHWC): row m = (b, y, x). Every activation argument has a leading dimension in floats
 * (>= its channel count, a multiple of 4), so an operator reads or writes a channel slice of a wider buffer:
 * torch.cat([up, skip], 1) is the up-convolution writing columns [0, O) and the encoder's second convolution writing columns
 * [O, 2 O) of one 2 O-wide buffer. Activation and weight pointers are 16-byte aligned. No atomics: the same inputs give the
 * same bits on every run. */

/* Conv2d(C, O, 3, padding=1): out[m][o] = act(bias[o] + sum_{ky,kx,c} in[(b, y+ky-1, x+kx-1)][c] * W[o][(ky*3+kx)*C + c]), zeros
 * outside the image, act = ReLU when relu != 0. W: operand copy (type E of `precision`) of the (O, C, 3, 3) kernel permuted to
 * (O, 3, 3, C), rows of 9 C elements (ocm_op_im2col3x3's K order). The rows of the 3x3 neighbourhood are gathered and converted
 * on the way into LDS: no 9 C-wide operand exists in memory. C % 32 == 0 (C <= 4096), O % 32 == 0. */
int ocm_op_conv3x3(int32_t precision, const float *in, int64_t ld_in, const void *w, const float *bias, float *out,
                   int64_t ld_out, int32_t batch, int32_t h, int32_t w_px, int32_t channels, int32_t out_channels, int32_t relu,
                   void *stream);
/* nn.Linear + ReLU into a column slice: out[m][0..N) = max(A[M][K] . W[N][K]^T + bias[N], 0) in fp32, rows ld_out floats apart;
 * A, W of type E as for ocm_op_linear (same shape rules, same tile dispatch). With ocm_op_im2col3x3 in front it is the 3x3
 * convolution as a composition: what build_unet runs where that measures faster than ocm_op_conv3x3 (few rows, long K). */
int ocm_op_linear_relu(int32_t precision, const void *a, const void *w, const float *bias, float *out, int64_t ld_out, int32_t M,
                       int32_t N, int32_t K, void *stream);
/* The same for a three-channel image read in place: pixel (b, c, y, x) = image[b*stride_b + c*stride_c + y*stride_y + x] (element
 * strides, any alignment). W: operand copy of the (O, 3, 3, 3) kernel permuted to (O, 3, 3, 3 = c), its 27 columns followed by zero
 * columns up to one K step: rows of 32 elements (fp32, split pairs) or 64 (bf16). */
int ocm_op_conv3x3_image(int32_t precision, const float *image, int64_t stride_b, int64_t stride_c, int64_t stride_y,
                         const void *w, const float *bias, float *out, int64_t ld_out, int32_t batch, int32_t h, int32_t w_px,
                         int32_t out_channels, int32_t relu, void *stream);
/* nn.MaxPool2d((2, 2)): out[(b, y, x)][c] = max over in[(b, 2y+i, 2x+j)][c], bit exact with torch (NaN propagates). h, w even,
 * C % 4 == 0. */
int ocm_op_maxpool2x2(const float *in, int64_t ld_in, float *out, int64_t ld_out, int32_t batch, int32_t h, int32_t w,
                      int32_t channels, void *stream);
/* nn.ConvTranspose2d(C, O, 2, stride=2): out[(b, 2y+i, 2x+j)][o] = bias[o] + sum_c in[(b, y, x)][c] * Wt[c][o][i][j]; h, w_px are
 * the INPUT grid. One GEMM with N = 4 O whose epilogue places the four O-wide groups at their pixels. W: operand copy of the
 * (C, O, 2, 2) kernel permuted to (2, 2, O, C): row (i*2 + j)*O + o, C elements. C % 32 == 0, O % 32 == 0, bias 16-byte aligned. */
int ocm_op_upconv2x2(int32_t precision, const float *in, int64_t ld_in, const void *w, const float *bias, float *out,
                     int64_t ld_out, int32_t batch, int32_t h, int32_t w_px, int32_t channels, int32_t out_channels, void *stream);
/* Conv2d(C, 1, 1) written as planes: out[b][0][p] = bias[0] + sum_c in[b*hw + p][c] * w[c] in fp32 (bias may be NULL), out
 * (B, 1, hw) contiguous. C % 4 == 0. */
int ocm_op_conv1x1_planes(const float *in, int64_t ld_in, const float *w, const float *bias, float *out, int32_t batch,
                          int64_t hw, int32_t channels, void *stream);

/* ---- training of the LinearProbing decoders on a frozen encoder (model.py:142-174; kernels_train.hip) ----
 * Token-major rows m = (image, y, x), M = B*hp*wp. Every reduction runs in a fixed order decided by the shapes alone (no
 * atomics): the same inputs give the same bits on every run. Statistics, sums and accumulators are fp32. Workspaces are
 * caller-allocated device memory of at least the queried size; their contents on entry do not matter. */

/* Weight (and bias) gradient of a token-major linear map Y = X W^T + b: dw[N][K] = sum_m dy[m][n] x[m][k] and, when db is
 * not NULL, db[N] = sum_m dy[m][n]. dy fp32 [M][N], x fp32 [M][K], row-major; the products run on the MFMA in `precision`
 * (the operands are rounded to bf16 / split pairs on the way into LDS; fp32 keeps exact products), fp32 accumulate. M is
 * split across workgroups and the partial slabs are added in slice order. N % 32 == 0, K % 32 == 0, any M >= 1.
 * For the decoders: conv1 (N = 4 s^2, K = 9 D, x = im2col of the patch tokens), conv2 (N = s^2, K = 9 * 4 s^2), the 1x1
 * head (N = s^2 * c_out, K = D, x = the normed patch tokens). */
size_t ocm_weight_grad_workspace_bytes(int32_t M, int32_t N, int32_t K);
int ocm_op_weight_grad(int32_t precision, const float *dy, const float *x, float *dw, float *db, int32_t M, int32_t N,
                       int32_t K, void *workspace, size_t workspace_bytes, void *stream);

/* Workspace of the per-channel reductions below for `rows` x `channels`. */
size_t ocm_channel_reduce_workspace_bytes(int64_t rows, int32_t channels);
/* BatchNorm2d batch statistics of a token-major fp32 [rows][channels] tensor: mean and the BIASED variance, two passes
 * (the second sums (x - mean)^2: no cancellation when a channel's mean is large against its spread). */
int ocm_op_batch_stats(const float *x, float *mean, float *var, int64_t rows, int32_t channels, void *workspace,
                       size_t workspace_bytes, void *stream);
/* ocm_op_im2col3x3 of z = max(y * scale[c] + shift[c], 0) (BatchNorm with scale = gamma * invstd, shift = beta - mean *
 * scale, then the ReLU): conv2's operand in the training-mode forward, in the operand type of `precision`. */
int ocm_op_bn_relu_im2col3x3(int32_t precision, const float *y, const float *scale, const float *shift, void *out,
                             int32_t batch, int32_t h, int32_t w, int32_t channels, void *stream);
/* Backward of z = ReLU(BatchNorm(y)) with batch statistics, all [rows][channels] fp32, channels % 4 == 0:
 *   u = dz * [y * scale + shift > 0],  xhat = (y - mean) * invstd
 *   dbeta = sum_m u,  dgamma = sum_m u * xhat,  dy = scale * (u - dbeta / rows - xhat * dgamma / rows). */
int ocm_op_bn_relu_backward(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale,
                            const float *shift, float *dy, float *dgamma, float *dbeta, int64_t rows, int32_t channels,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Inverse of ocm_op_pixel_shuffle: grad_lin[b*hp*wp + y*wp + x][c*s*s + i*s + j] = grad_out[b][c][y*s+i][x*s+j] (a gather,
 * bit exact). */
int ocm_op_pixel_shuffle_backward(const float *grad_out, float *grad_lin, int32_t batch, int32_t hp, int32_t wp,
                                  int32_t c_out, int32_t s, void *stream);

/* ---- masked image modelling on the decoder GEMM's rows (transformers' SwinForMaskedImageModeling; kernels_mim.hip) ----
 * SimMIM's masked L1 reconstruction loss straight from the 1x1 convolution evaluated token-major:
 *   lin  (batch*hp*wp, c*s*s) fp32, the layout ocm_op_pixel_shuffle reads;  x (batch, c, S, S) fp32 with S = hp*s = wp*s;
 *   mask (batch, S/p, S/p) uint8, nonzero = masked; p divides S (p < s, p = s and p > s are all served).
 * Outputs, each optional (null skips it):
 *   rec  (batch, c, S, S): rec[b][ch][y*s+i][xx*s+j] = lin[b*hp*wp + y*wp + xx][ch*s*s + i*s + j], the bits of ocm_op_pixel_shuffle;
 *   dlin (lin's shape): sign(rec - x) * m * scale with m the pixel's mask bit, sign(0) = 0 (torch's abs backward) and
 *        scale = (float)(1.0 / ((count + 1e-5) * c)) formed in double, count = p*p * (nonzero mask bytes) the masked pixels of
 *        one channel: every element is exactly +scale, -scale or 0 — the gradient of `loss` with respect to lin;
 *   loss (one float): (float)(sum |x - rec| * m / (count + 1e-5) / c), each |x - rec| exact in float64, summed as float64
 *        per-workgroup partials combined in a fixed order. count = 0 gives loss = 0 and dlin = 0.
 * Three stream-ordered launches (mask count, main pass, finalise; only the main pass when rec alone is asked for), no atomics,
 * nothing synchronises, reruns give the same bits. The workspace (ocm_mim_l1_loss_workspace_bytes, 8-byte aligned) needs no
 * initialisation; it is required even when no output needs it. With s % 4 == 0 the float pointers are 16-byte aligned.
 * OCM_EINVAL: null lin / x / mask, a non-positive size, p not dividing S, hp*s != wp*s, a misaligned pointer;
 * OCM_ENOMEM: a null or short workspace. */
size_t ocm_mim_l1_loss_workspace_bytes(int32_t batch, int32_t hp, int32_t wp, int32_t c, int32_t s);
int ocm_op_mim_l1_loss(const float *lin, const float *x, const uint8_t *mask, int32_t batch, int32_t hp, int32_t wp, int32_t c,
                       int32_t s, int32_t p, float *rec, float *dlin, float *loss, void *workspace, size_t workspace_bytes,
                       void *stream);

/* The mask-token step of SwinEmbeddings.forward, embeddings * (1 - w) + mask_token * w with a 0 / 1 w, as a row select:
 * rows (tokens, channels) fp32 in place — a row whose mask byte is nonzero becomes mask_token (channels floats) bit for bit,
 * the other rows are not touched. channels a multiple of 4, rows and mask_token 16-byte aligned.
 * Backward: d_rows (may alias d; optional) = d at the unmasked rows and zero at the masked ones; d_mask_token (channels floats;
 * optional) = the sum of d over the masked rows, float64 partials per 256 rows combined in row order and rounded once. Its
 * workspace (ocm_swin_mask_tokens_backward_workspace_bytes, 8-byte aligned) needs no initialisation; null or short: OCM_ENOMEM. */
int ocm_op_swin_mask_tokens(float *rows, const uint8_t *mask, const float *mask_token, int64_t tokens, int32_t channels,
                            void *stream);
size_t ocm_swin_mask_tokens_backward_workspace_bytes(int64_t tokens, int32_t channels);
int ocm_op_swin_mask_tokens_backward(const float *d, const uint8_t *mask, float *d_rows, float *d_mask_token, int64_t tokens,
                                     int32_t channels, void *workspace, size_t workspace_bytes, void *stream);

/* ---- training of build_unet (model.py:227-320; PGT.py's and unet.py's step; kernels_conv_train.hip) ----
 * The forward runs every convolution without its ReLU (ocm_op_conv3x3 with relu = 0, or ocm_op_im2col3x3 + ocm_op_linear),
 * ocm_op_batch_stats and ocm_op_bn_relu; the backward runs ocm_op_bn_relu_backward, ocm_op_weight_grad on an im2col operand,
 * the data gradient as ocm_op_conv3x3 with the flipped kernel, and the operators below. Token-major fp32 rows with leading
 * dimensions as for inference; one lane per four channels, 64-bit element indices, every output element written exactly once,
 * no atomics. Activation pointers are 16-byte aligned, leading dimensions multiples of 4. */

/* z[m][c] = max(y[m][c] * scale[c] + shift[c], 0): y dense [rows][channels], z rows ld_z floats apart. The pre-activation is the
 * expression whose sign ocm_op_bn_relu_backward tests: an element passes that gate exactly when z > 0. channels % 4 == 0. */
int ocm_op_bn_relu(const float *y, const float *scale, const float *shift, float *z, int64_t ld_z, int64_t rows, int32_t channels,
                   void *stream);
/* Backward of ocm_op_maxpool2x2 over z (the forward's input, (batch, h, w) rows): per window the scan of the forward is replayed
 * (a later value wins when it is greater or NaN) and the position it ends on gets dpool[(b, y/2, x/2)], the other three get 0;
 * when add is not NULL every position adds add[(b, y, x)] (the gradient a skip connection carries to the same tensor). */
int ocm_op_maxpool2x2_backward(const float *z, int64_t ld_z, const float *dpool, int64_t ld_dp, const float *add, int64_t ld_add,
                               float *dz, int64_t ld_dz, int32_t batch, int32_t h, int32_t w, int32_t channels, void *stream);
/* The output gradient of ocm_op_upconv2x2 as the rows of its GEMM: g[(b, y, x)][(i*2 + j)*O + o] = dout[(b, 2y+i, 2x+j)][o], a
 * bit-exact copy; h, w are the INPUT grid, g is dense (batch*h*w, 4 O). Then dIn = ocm_op_linear(g, W^T), dW = ocm_op_weight_grad(g,
 * in) and dbias = its db summed over the four groups. O % 4 == 0. */
int ocm_op_upconv2x2_gather(const float *dout, int64_t ld, float *g, int32_t batch, int32_t h, int32_t w, int32_t out_channels,
                            void *stream);
/* The fp32 rows ocm_op_conv3x3_image gathers: out[(b, y, x)][(ky*3 + kx)*3 + c] = image[b*stride_b + c*stride_c + (y+ky-1)*stride_y +
 * x+kx-1], zeros outside the image and in columns 27..31; out dense (batch*h*w, 32): the x of the first layer's weight gradient. */
int ocm_op_im2col3x3_image(const float *image, int64_t stride_b, int64_t stride_c, int64_t stride_y, float *out, int32_t batch,
                           int32_t h, int32_t w, void *stream);
/* Backward of ocm_op_conv1x1_planes: dlogits (B, 1, hw) contiguous; din[m][c] = dlogits[m] * w[c]; when dw is not NULL
 * dw[c] = sum_m dlogits[m] * in[m][c]; when db is not NULL db[0] = sum_m dlogits[m]. The sums run in a fixed order through the
 * workspace. C % 4 == 0, C <= 1024. */
size_t ocm_conv1x1_planes_backward_workspace_bytes(int64_t rows, int32_t channels);
int ocm_op_conv1x1_planes_backward(const float *dlogits, const float *in, int64_t ld_in, const float *w, float *din, int64_t ld_din,
                                   float *dw, float *db, int32_t batch, int64_t hw, int32_t channels, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ---- training of the ViT encoder (SimMIM pre-training, model.py:55-83; kernels_train.hip, kernels_train_attn.hip) ----
 * The forward runs the stand-alone operators above and keeps, per block, the LayerNorm inputs, qkv_f32, lse2, the context and the
 * fp32 fc1 pre-activation; the backward below plus ocm_op_linear (data gradients, transposed weights) and ocm_op_weight_grad
 * (weight and bias gradients). No atomics anywhere: the same inputs give the same bits on every run. Token-major rows
 * m = b*N + n, all gradients fp32. */

/* Attention backward for heads of head_dim = 64 or 128 (any other width: OCM_EINVAL), any N >= 1, batch * heads <= 65535:
 *   qkv_f32 [3][B][H][N][hd] (ocm_op_qkv_proj_hd), lse2 [B*H][N] (ocm_op_attention_hd), dctx [B][N][H*hd] = dO,
 *   delta [B*H][N] = rowsum(dO o O) (ocm_op_attention_backward_delta)
 *   -> dqkv fp32 [B*N][3*H*hd]: columns (which, head, channel) in qkv.weight's row order, every element written.
 * P = exp2(q.k * scale * log2e - lse2) is recomputed per tile, never stored. All products are fp32 on v_mfma_f32_32x32x2_f32 in
 * every set_precision mode (the operands are the fp32 projections; the mode only decided the forward's lse2). dK / dV come from a
 * key-block-major kernel, dQ from a query-block-major one: each output has one owner and one summation order. */
int ocm_op_attention_backward(const float *qkv_f32, const float *lse2, const float *dctx, const float *delta, float *dqkv,
                              int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, float scale, void *stream);
/* delta[b*H + h][n] = sum_d dctx[b][n][h*hd + d] * ctx[b][n][h*hd + d] with ctx in the operand type E of `precision` (what
 * ocm_op_attention_hd wrote), and, when ctx_f32 != NULL, ctx as fp32 [B*N][H*hd]. heads * head_dim % 32 == 0. */
int ocm_op_attention_backward_delta(int32_t precision, const void *ctx, const float *dctx, float *delta, float *ctx_f32,
                                    int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim, void *stream);

/* LayerNorm backward over rows of `dim` (statistics recomputed from x in two passes, so rows with a large mean stay accurate):
 *   dx = rstd (gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat)) + dres   (dres: the residual branch's gradient, or NULL;
 *   it may alias dx), dgamma = sum_m dy xhat, dbeta = sum_m dy (fixed-order column sums). All fp32 [rows][dim]. */
size_t ocm_layernorm_backward_workspace_bytes(int64_t rows, int32_t dim);
int ocm_op_layernorm_backward(const float *dy, const float *x, const float *gamma, const float *dres, float *dx, float *dgamma,
                              float *dbeta, int64_t rows, int32_t dim, float eps, void *workspace, size_t workspace_bytes,
                              void *stream);

/* Stochastic depth (DropPath, dino/vision_transformer.py:25-44) behind a branch whose GEMM ran with OCM_EPI_BIAS_F32 into
 * `branch`; scale [batch] fp32 holds 0 or 1 / keep per image, the image of a row is row / tokens (kernels_drop_path.hip).
 *   x_out[b][t][:] = x[b][t][:] + branch[b][t][:] * scale[b]   (fp32: the product rounded, then the sum; x_out may alias x or
 *   branch)
 *   y              = LayerNorm(x_out; gamma, beta, eps) in out_kind (OCM_LN_F32 / OCM_LN_BF16 / OCM_LN_SPLIT), bit for bit
 *   what ocm_op_layernorm makes of x_out.
 * Every dim ocm_op_layernorm accepts. Null pointers, batch or tokens <= 0, a bad dim or out_kind return OCM_EINVAL before any
 * launch. */
int ocm_op_drop_path_layernorm(const float *x, const float *branch, const float *scale, const float *gamma, const float *beta,
                               float *x_out, void *y, int32_t out_kind, int32_t batch, int32_t tokens, int32_t dim, float eps,
                               void *stream);
/* dbranch_f32 = dout * scale[image] (it may alias dout); dbranch_op (NULL for OCM_PREC_FP32) = the same values in the operand
 * type of `precision` (bf16, or split pairs with dim % 32 == 0), as ocm_op_cast_bf16 / ocm_op_cast_split would write them from
 * dbranch_f32. One pass; dim % 8 == 0. Refusals as above. */
int ocm_op_drop_path_backward(int32_t precision, const float *dout, const float *scale, float *dbranch_f32, void *dbranch_op,
                              int32_t batch, int32_t tokens, int32_t dim, void *stream);

/* nn.Dropout of the ViT training path without a stored mask (kernels_dropout.hip, csrc/philox.h). The mask of one site over a
 * tensor in row-major order of its unpadded shape, flat index f: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32), seed
 * the site's non-negative int64, and counter (g & 0xffffffff, g >> 32, 0, 0), g = f >> 2; element f reads output word f & 3 and
 * is kept iff word >= thresh. A kept element's factor is inv_keep, a dropped one's 0.0f; every operator applies it as one
 * rounded fp32 multiplication.
 * The three functions below run on the host and need no device. */
void ocm_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* thresh = (uint32) floor(p * 2^32 + 0.5) in double, inv_keep = (float)(1.0 / (1.0 - p)); OCM_EINVAL outside 0 < p < 1. */
int ocm_dropout_threshold(double p, uint32_t *thresh, float *inv_keep);
/* keep[i] = 1 where element first + i is kept, else 0, for i < count. */
int ocm_dropout_keep_host(int64_t seed, uint64_t first, uint64_t count, uint32_t thresh, uint8_t *keep);
/* The device operators read the seed as seeds[site] from DEVICE memory, so nothing is synchronised. fp32 pointers are 16-byte
 * aligned. Null pointers, a negative site, non-positive sizes, a bad dim, out_kind or precision return OCM_EINVAL before any
 * launch.
 * keep[i] = 1 / 0 for i < count: the mask itself, as the device generator forms it. */
int ocm_op_dropout_mask(const int64_t *seeds, int32_t site, size_t count, uint32_t thresh, uint8_t *keep, void *stream);
/* y = x * factor, fp32; y may alias x; count % 4 == 0. Its own backward. */
int ocm_op_dropout(const float *x, const int64_t *seeds, int32_t site, uint32_t thresh, float inv_keep, float *y, size_t count,
                   void *stream);
/* The sibling of ocm_op_drop_path_layernorm behind a dropped branch: d = branch * factor; with scale ([batch], or NULL)
 * d = d * scale[image]; x_out = x + d (each step rounded); y = LayerNorm(x_out) in out_kind, bit for bit what ocm_op_layernorm
 * makes of x_out. The flat index of the mask is row * dim + column. Same aliasing and widths as ocm_op_drop_path_layernorm. */
int ocm_op_dropout_layernorm(const float *x, const float *branch, const int64_t *seeds, int32_t site, uint32_t thresh,
                             float inv_keep, const float *scale, const float *gamma, const float *beta, float *x_out, void *y,
                             int32_t out_kind, int32_t batch, int32_t tokens, int32_t dim, float eps, void *stream);
/* The sibling of ocm_op_drop_path_backward: dbranch_f32 = (dout * factor) * scale[image] (scale may be NULL; dbranch_f32 may
 * alias dout), dbranch_op (NULL for OCM_PREC_FP32) the same values as ocm_op_cast_bf16 / ocm_op_cast_split would write them.
 * One pass; dim % 8 == 0. */
int ocm_op_dropout_backward(int32_t precision, const float *dout, const int64_t *seeds, int32_t site, uint32_t thresh,
                            float inv_keep, const float *scale, float *dbranch_f32, void *dbranch_op, int32_t batch,
                            int32_t tokens, int32_t dim, void *stream);
/* gelu(h) as ocm_op_gelu forms it in fp32, times the factor, then the operand cast of `precision` into out; out_f32 (optional)
 * the masked fp32 values. ocm_op_gelu's conditions on count. */
int ocm_op_gelu_dropout(int32_t precision, const float *h, const int64_t *seeds, int32_t site, uint32_t thresh, float inv_keep,
                        void *out, float *out_f32, size_t count, void *stream);
/* dh = (dg * factor) * gelu'(h), as ocm_op_gelu_backward forms it from the masked dg (dh may alias dg); g_f32 (optional) =
 * gelu(h) * factor, the masked activation of the forward. */
int ocm_op_gelu_dropout_backward(const float *dg, const float *h, const int64_t *seeds, int32_t site, uint32_t thresh,
                                 float inv_keep, float *dh, float *g_f32, size_t count, void *stream);

/* erf GELU (nn.GELU()) of `count` fp32 values: out in the operand type E of `precision` (count % 32 == 0 for split pairs, rows
 * whose length is a multiple of 32), out_f32 (optional) in fp32. */
int ocm_op_gelu(int32_t precision, const float *h, void *out, float *out_f32, size_t count, void *stream);
/* dh = dg * gelu'(h) (dh may alias dg); g_f32 (optional) = gelu(h). */
int ocm_op_gelu_backward(const float *dg, const float *h, float *dh, float *g_f32, size_t count, void *stream);

/* Patch rows of a contiguous fp32 image (B, C, H, W): cols [B*P][C*p*p], row b*P + py*wp + px, column c*p*p + ky*p + kx (the
 * (D, C, p, p) weight's K order): the input of the patch-embedding weight gradient. H, W multiples of p. */
int ocm_op_patch_unfold(const float *image, float *cols, int32_t batch, int32_t channels, int32_t height, int32_t width,
                        int32_t patch, void *stream);
/* Gradient dtok [B][N][D] of t = cat(cls, patch * (1 - w) + mask_token * w) + pos (model.py:28-41) split into
 *   dpatch [B*(N-1)][D] = (1 - w) dtok[:, 1:],  dmask_token [D] = sum over (b, p) of w dtok (only when mask != NULL),
 *   dpos [N][D] = sum_b dtok (row 0 is the cls token's gradient), images summed in order.
 * mask [B][N-1] fp32 or NULL (w = 0). */
size_t ocm_patch_embed_backward_workspace_bytes(int32_t batch, int32_t n_tokens, int32_t dim);
int ocm_op_patch_embed_backward(const float *dtok, const float *mask, float *dpatch, float *dmask_token, float *dpos,
                                int32_t batch, int32_t n_tokens, int32_t dim, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- sigmoid Dice loss (utils.py:410-424: finetune.py's loss; kernels_train.hip) ----
 * loss = 1 - (2 I + smooth) / (sum p + sum t + smooth) with p = sigmoid(logits), I = sum p t over `count` >= 1 fp32 elements.
 * One pass writes per-workgroup partial sums into the workspace, a finishing launch adds them in a fixed order (no atomics:
 * the same bits on every run) and writes sums_out[3] = (I, sum p, sum t) and loss_out[1] to device memory; nothing
 * synchronises with the host. 16-byte loads when both pointers are 16-byte aligned, a scalar tail for any count. */
size_t ocm_dice_loss_workspace_bytes(size_t count);
int ocm_op_dice_loss(const float *logits, const float *targets, float *loss_out, float *sums_out, size_t count, float smooth,
                     void *workspace, size_t workspace_bytes, void *stream);
/* dlogits = -g (2 t S - (2 I + smooth)) / S^2 * p (1 - p), S = sum p + sum t + smooth, g = grad_loss[0]; `sums` (what
 * ocm_op_dice_loss wrote) and grad_loss are device memory. Elementwise, every element of dlogits written. */
int ocm_op_dice_loss_backward(const float *logits, const float *targets, const float *sums, const float *grad_loss,
                              float *dlogits, size_t count, float smooth, void *stream);

/* ---- k-means feature clustering (eval.py --method k-means_feature_clustering, utils.py:171-197; kernels_cluster.hip) ----
 * X is the fp32 [S*S][dim] feature matrix, row y*S + x; dim % 4 == 0 and 4 <= dim <= 1024. Every reduction runs in a fixed
 * order (no atomics): the same inputs give the same bits. Null pointers, S < 1 or a bad dim return OCM_EINVAL. */
/* X = keys of the patch tokens of `image` in qkv (3, batch, heads, n_tokens, head_dim) fp32, channel order (head, hd),
 * bilinearly upsampled from the grid x grid token grid (n_tokens = grid^2 + 1, CLS first) to S x S with torch's
 * align_corners=False rule. head_dim % 4 == 0. */
int ocm_op_kmeans_features(const float *qkv, int32_t batch, int32_t heads, int32_t n_tokens, int32_t head_dim, int32_t image,
                           int32_t grid, int32_t S, float *X, void *stream);
/* In place: X = (X - mean) / std (torch.mean / unbiased torch.std per column, in fp32 arithmetic), then X -= X.mean(axis=0)
 * (sklearn KMeans.fit's centring). Statistics in fp64, two passes. stats [4][dim] fp64: mean, std, the fp32 centring mean
 * (as fp64; add it back to centres), and the biased variance of the final X per column (sklearn's _tolerance). */
size_t ocm_kmeans_zscore_workspace_bytes(int32_t S, int32_t dim);
int ocm_op_kmeans_zscore(float *X, int32_t S, int32_t dim, double *stats, void *workspace, size_t workspace_bytes,
                         void *stream);
/* dist [n_cand][S*S] fp64 = ||x - cand[k]||^2 accumulated in fp64; with `closest` [S*S] (or NULL) the running minimum
 * min(closest, dist) of k-means++. cand [n_cand][dim] fp32, 1 <= n_cand <= 64. */
int ocm_op_kmeans_dist(const float *X, int32_t S, int32_t dim, const float *cand, int32_t n_cand, const double *closest,
                       double *dist, void *stream);
/* One Lloyd step for two clusters: labels[r] = argmin_c ||x_r - centers[c]||^2 (fp64; a tie goes to cluster 0).
 * Unless assign_only: centers_new [2][dim] = fp32 of the fp64 cluster sums / counts, and sums [2][dim] fp64 (or NULL).
 * info [7] fp64: inertia sum ||x - centers[label]||^2, count0, count1, ||centers_new - centers||^2 per cluster (0 when
 * assign_only), 1 when any label differs from labels_old (1 when labels_old is NULL), the number of empty clusters
 * (centers_new of an empty cluster is 0: the caller treats a non-zero count as an error). */
size_t ocm_kmeans_lloyd_workspace_bytes(int32_t S, int32_t dim);
int ocm_op_kmeans_lloyd(const float *X, int32_t S, int32_t dim, const float *centers, const int32_t *labels_old,
                        int32_t *labels, float *centers_new, double *sums, double *info, int32_t assign_only, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---- region-queried attention: the query points of analyse_attention.py --region_query (:183-223; utils.py:237-281
 * yen_threshold / morphology_cleaning, data.py:216-233 get_ROIs; kernels_morph.hip) ----
 * Every operator works on `batch` independent (h, w) images (sides 1..32768, h * w <= 2^30: int32 pixel indices, batch <=
 * 65535). Masks are uint8, nonzero = foreground; masks written here hold 0 / 1. Refused arguments return OCM_EINVAL (a short
 * workspace OCM_ENOMEM) before any launch. All arithmetic is on integers: the same inputs give the same bits. */
/* mask = (level <= img) (utils.py:242) */
int ocm_op_mask_ge_u8(const uint8_t *img, uint8_t *mask, int64_t count, int32_t level, void *stream);
/* 8-connected components (skimage.measure.label(connectivity=2) / scipy.ndimage.label with the 3x3 structure): labels
 * [batch][h][w] int32, 0 on background and 1..n on foreground, numbered in raster order of each component's first pixel;
 * counts[b] = n. Union-find on pixel indices in `labels` itself: LDS pass per ocm_label8_tile() x ocm_label8_tile() tile,
 * tile-border pass with integer atomic minima, flatten, scan of the root flags. The workspace needs no initialisation. */
int32_t ocm_label8_tile(void);
size_t ocm_label8_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int ocm_op_label8(const uint8_t *mask, int32_t *labels, int32_t *counts, int32_t batch, int32_t h, int32_t w, void *workspace,
                  size_t workspace_bytes, void *stream);
/* Exact sums per label 1..max_regions of a label image (labels outside that range are ignored): area, sum of row and of
 * column indices as int64 [batch][max_regions], bbox int32 [batch][max_regions][4] = (min_row, min_col, max_row + 1,
 * max_col + 1) as skimage's regionprops gives it ((h, w, 0, 0) for a label without pixels). centroid = sum / area. */
int ocm_op_region_stats(const int32_t *labels, int32_t batch, int32_t h, int32_t w, int32_t max_regions, int64_t *area,
                        int64_t *sum_row, int64_t *sum_col, int32_t *bbox, void *stream);
/* skimage.morphology.remove_small_objects(mask, min_size, connectivity=2) of a boolean mask: out = 1 on the pixels of
 * 8-connected components of at least min_size pixels, else 0. out may be mask itself. */
size_t ocm_remove_small_objects_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int ocm_op_remove_small_objects(const uint8_t *mask, uint8_t *out, int32_t batch, int32_t h, int32_t w, int32_t min_size,
                                void *workspace, size_t workspace_bytes, void *stream);
/* scipy.ndimage.binary_dilation (op 0) / binary_erosion (op 1) with a size x size footprint (size odd, 1..7; bit
 * dy * size + dx of footprint_bits = footprint[dy][dx], centre size / 2) and border_value 0 / 1 for the pixels outside the
 * image. skimage's binary_closing(mask, disk(2)) is dilation with border 0, then erosion with border 1. src != dst. */
int ocm_op_binary_morph(const uint8_t *src, uint8_t *dst, int32_t batch, int32_t h, int32_t w, uint64_t footprint_bits,
                        int32_t size, int32_t op, int32_t border_value, void *stream);
/* analyse_attention.py:196-211 — rows (tiles, heads, n_rows, pixels) fp32 attention rows; for tile t the rows
 * sel[offsets[t] .. offsets[t+1]) (indices into n_rows, duplicates allowed, n_sel entries in all): the head mean of each
 * exactly as ocm_op_head_mean computes it, the maps added in that order in fp32 and divided by their number
 * (np.mean(list_of_maps, axis=0)). maps (tiles, pixels). An empty (or out-of-range) selection writes NaN. */
int ocm_op_query_mean(const float *rows, const int32_t *sel, const int32_t *offsets, float *maps, int32_t tiles, int32_t heads,
                      int32_t n_rows, int32_t pixels, int32_t n_sel, void *stream);

/* ---- ROI-guided SimMIM masks: mim.py --roi_masking (data.py:211-233, SimMIMTransform.__call__; kernels_roi.hip) ----
 * The two ends of the per-image chain threshold -> get_ROIs -> resize(order=0) -> mask * rois; the closing and the labelling
 * between them are ocm_op_binary_morph (twice) and ocm_op_label8 on the whole batch. Same conventions as the block above. */
/* binary = ToPILImage()(img).convert('L') > level: `batch` float32 images of `chans` (1 or 3) dense (h, w) planes, images
 * stride_b and planes stride_c elements apart; L is ocm_op_image_to_gray_u8's arithmetic bit for bit (mul(255) truncated, PIL's
 * integer RGB -> L weights; one plane is its own grey image). mask [batch][h][w] = 0 / 1; white[b] = the number of white pixels of
 * image b, an exact integer (the operator zeroes it itself, in stream order). level 0..255. */
int ocm_op_roi_threshold(const float *images, int64_t stride_b, int64_t stride_c, int32_t chans, int32_t batch, int32_t h,
                         int32_t w, int32_t level, uint8_t *mask, int32_t *white, void *stream);
/* labels [batch][h][w] int32 (ocm_op_label8 of the closed mask); row_idx [gh] / col_idx [gw] int32 device tables: grid cell (i, j)
 * samples labels[b][row_idx[i]][col_idx[j]] — scipy.ndimage.zoom(order=0, mode='mirror', grid_mode=True), which is what
 * skimage.transform.resize(order=0, anti_aliasing=False) calls; an entry outside the image reads as background. For image b:
 *   roi(i, j) = white[b] >= min_size && (label & 255) != 0
 *               (remove_small_objects reads the uint8 {0, 255} image as a label image: the white class goes as a whole, and only
 *               when it holds fewer than min_size pixels in total; rois.astype(np.uint8) of a float64 label wraps modulo 256)
 *   new(i, j) = masks[b][i][j] != 0 && roi(i, j)
 *   out[b] = new and used[b] = 1 when any cell of new is set, else out[b] = (masks[b] != 0) and used[b] = 0.
 * masks / out: [batch][gh][gw] elements of mask_bytes bytes (1: uint8 or bool, 8: int64), out holds 0 / 1; masks != out.
 * One workgroup per image. */
int ocm_op_roi_apply(const int32_t *labels, const int32_t *row_idx, const int32_t *col_idx, const int32_t *white,
                     int32_t min_size, const void *masks, int32_t mask_bytes, void *out, uint8_t *used, int32_t batch, int32_t h,
                     int32_t w, int32_t gh, int32_t gw, void *stream);

/* ---- Chan-Vese level sets: skimage.segmentation.chan_vese (0.19.x) as utils.py:199-225 calls it (eval.py's "chan-vese" /
 * "chan-vese_ours" methods; kernels_levelset.hip) ----
 * For each of `batch` independent images: image [batch][h][w] float64, already normalised as skimage does (img - min, then
 * / max when that is not 0); phi [batch][h][w] float64, the initial level set on entry and the final one on return;
 * mask[b][y][x] = phi > 0 (0 / 1); iters[b] = the number of iterations image b ran. The loop, all in float64:
 *   i = 0; phivar = DBL_MAX
 *   while phivar > tol and i < max_num_iter:
 *     c, e, w, s, n = phi at the pixel and its x+1, x-1, y+1, y-1 neighbours (edge-replicated); eta = 1e-16
 *     xp = e-c  xn = c-w  x0 = (e-w)/2  yp = s-c  yn = c-n  y0 = (s-n)/2
 *     C1 = 1/sqrt(eta+xp^2+y0^2)  C2 = 1/sqrt(eta+xn^2+y0^2)  C3 = 1/sqrt(eta+x0^2+yp^2)  C4 = 1/sqrt(eta+x0^2+yn^2)
 *     K = e C1 + w C2 + s C3 + n C4;  H = phi > 0 (the sharp Heaviside)
 *     c1 = sum(image H) / sum(H) when sum(H) != 0, else sum(image H); c2 the same with 1 - H
 *     D = -lambda1 (image-c1)^2 + lambda2 (image-c2)^2;  delta = 1 / (1 + phi^2)
 *     new = (phi + dt delta (mu K + D)) / (1 + mu dt delta (C1+C2+C3+C4))
 *     phivar = sqrt(mean((new - phi)^2)); phi = new; i += 1
 * Every term reads the old phi. One stream-ordered launch per iteration, no host synchronisation; the images of a batch stop
 * independently. Sums are per-workgroup partials added in a fixed order (no floating-point atomics): the same inputs give the
 * same bits. The kernels work on ocm_chan_vese_tile() x ocm_chan_vese_tile() tiles. The workspace needs no initialisation.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): batch outside 1..65535, a side outside
 * 1..32768 or h * w > 2^30, max_num_iter outside 0..10000, a non-finite or negative mu, dt or tol, a non-finite lambda, null
 * pointers. max_num_iter = 0 returns phi unchanged, its mask and iters = 0. */
int32_t ocm_chan_vese_tile(void);
size_t ocm_chan_vese_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int ocm_op_chan_vese(const double *image, double *phi, uint8_t *mask, int32_t *iters, int32_t batch, int32_t h, int32_t w,
                     double mu, double lambda1, double lambda2, double tol, int32_t max_num_iter, double dt, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- mask scores: what eval.py's validate loop reports per image (eval.py:204-221; utils.py:388-424 calculate_metrics and
 * DiceLoss; the six-score variant of PGT.py:247-275 / finetune.py:209; kernels_score.hip) ----
 * pred holds `batch` images of `count` elements back to back: a uint8 mask whose value is v / 255.0f (eval.py's output / 255)
 * when pred_is_u8 != 0, else fp32 used as is; target is fp32 of the same layout. The predicted class of an element is
 * value > 0.5f and its true class is target > 0.5f; a NaN compares false, so it is class 0.
 *   counts[b] = {tp, fp, fn, tn}, exact
 *   scores[b] = {jaccard tp / (tp + fp + fn), f1 2 tp / (2 tp + fp + fn), recall tp / (tp + fn), precision tp / (tp + fp),
 *                accuracy (tp + tn) / count, auc 0.5 (tp / (tp + fn) + tn / (tn + fp)), dice_loss} in float64
 * Each quotient is one IEEE float64 division of the integers; a zero denominator gives 0.0 (sklearn's zero_division="warn"
 * value: an all-zero pair scores 0, 0, 0, 0, 1). auc is the ROC-AUC of the 0/1 prediction and is NaN when the target holds one
 * class only (sklearn 1.7's value).
 *   dice_loss = 1 - (2 sum p t + smooth) / (sum p + sum t + smooth), p = sigmoid(value) in fp32 (the sigmoid of
 * ocm_op_dice_loss; the reference's DiceLoss applies it to eval.py's 0/1 mask as well), the three sums in float64. A NaN
 * element makes it NaN.
 * One pass writes per-workgroup partials into the workspace and a finishing launch per image adds them, both in a fixed order
 * (no atomics): the same inputs give the same bits, and an image scores to the same bits alone as within a batch, wherever it
 * starts. 16-byte loads for the images that start 16-byte aligned, element loads for the others. Nothing synchronises with the
 * host. The workspace (16-byte aligned) needs no initialisation; its size depends on the arguments alone, grows with count up
 * to a cap and is 0 for arguments the operator refuses.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): null pointers, batch outside 1..65535,
 * count 0 or above 2^36, a non-finite or negative smooth. */
size_t ocm_mask_scores_workspace_bytes(int32_t batch, size_t count);
int ocm_op_mask_scores(const void *pred, int32_t pred_is_u8, const float *target, int32_t batch, size_t count, float smooth,
                       int64_t *counts, double *scores, void *workspace, size_t workspace_bytes, void *stream);

/* ---- pixel k-means: cv2.kmeans as utils.py:118-169 calls it (eval.py's "k-means" / "k-means_ours" methods;
 * kernels_kmeans_px.hip) ----
 * The reference reshapes a gray uint8 image to N = H W / 3 samples of three consecutive pixels in raster order, runs
 * cv2.kmeans(Z, 2, None, (EPS + MAX_ITER, 10, 1.0), 10, KMEANS_RANDOM_CENTERS), paints res = np.uint8(centres)[labels] and takes
 * its Otsu mask. Restated from OpenCV 4.x modules/core/src/kmeans.cpp for K = 2, dims = 3; parity with a live cv2 unpinned
 * (cv2 is not installable here). A problem is one image of 3 N pixels; pixels holds `problems` of them back to back.
 *
 * ocm_cv_rng_uniform (host) is cv::RNG: state = (state & 0xffffffff) * 4164903690 + (state >> 32) mod 2^64, and a draw is
 * (float)(uint32)state * 2.3283064365386963e-10f. It writes n draws and advances *state; a state of 0 stands for 0xffffffff
 * (cv::RNG's seed 0, and a fresh process's state). cv2.kmeans draws attempts x 2 x 3 of them whatever the data are:
 * uniforms [problems][attempts][2][3] (device) is that stream, problem after problem.
 *
 * The loop, float32 unless stated, every operation rounded on its own (no fused multiply-add):
 *   lo[j], hi[j] = minimum and maximum of column j; d(x, c) = ((t0 t0 + t1 t1) + t2 t2), t = x - c
 *   for attempt a = 0 .. attempts - 1:
 *     c[k][j] = (u[a][k][j] * (1.f + margin * 2.f) - margin) * (hi[j] - lo[j]) + lo[j], margin = 1.f / 3
 *     iter = 0
 *     loop:
 *       if iter > 0:
 *         old = c; count[k], sum[k][j] = members and column sums of cluster k under the labels
 *         for every k with count[k] == 0: m = the cluster with the most members; b = sum[m] * (1.f / count[m]); among the
 *           members of m the sample with the largest d(x, b), the largest index on a tie, moves to k (its label, both counts,
 *           both sums)
 *         c[k][j] = sum[k][j] * (1.f / count[k]); shift = max over k of sum_j ((double)(c[k][j] - old[k][j]))^2
 *       else shift = +inf
 *       last = (++iter == max(max_iter, 2)) or shift <= eps * eps
 *       if last: compactness[a] = sum_i (double)d(x_i, c[label_i]), the labels not reassigned; stop
 *       label_i = 1 when d(x_i, c[1]) < d(x_i, c[0]), else 0 (a tie goes to 0)
 *   best = the first attempt with the smallest compactness (an attempt replaces the best only when strictly smaller)
 * The samples are integers 0..255, so the sums are exact integers: they are accumulated as integers and rounded to float32
 * once. That is OpenCV's sequential float32 sum bit for bit while 255 N < 2^24 (images up to 197 379 pixels, 384 x 384
 * included); beyond that OpenCV's own sum rounds along the way and this one stays exact. The compactness is a float64 sum in
 * one fixed order: the same inputs give the same bits, and a problem gives the same bits alone as within a batch, wherever it
 * starts.
 *
 * Outputs: labels [problems][N] (0 / 1) and centers [problems][2][3] of the best attempt; compactness and iters
 * [problems][attempts] (iters = the value of iter when the attempt stopped); best [problems]; mask [problems][3 N] =
 * res > level ? 255 : 0 with res[3 i + j] = (uint8)centers[label_i][j] (truncation) and level the Otsu level of res's
 * histogram by the statements of ocm_otsu_threshold (cv2.threshold(res, 0, 255, THRESH_BINARY + THRESH_OTSU)).
 * One workgroup runs one attempt's whole loop and a second launch finishes each problem: no atomics, no waiting between
 * workgroups, nothing synchronises with the host. 16-byte loads and stores for the problems that start 16-byte aligned,
 * element accesses for the others. The workspace (16-byte aligned) needs no initialisation; its size is 0 for arguments the
 * operator refuses.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): null pointers, problems outside
 * 1..65535, samples outside 2..2^24, attempts outside 1..32, max_iter outside 1..1000, a non-finite or negative eps, a
 * workspace that is not 16-byte aligned. */
int ocm_cv_rng_uniform(uint64_t *state, float *out, int64_t n);
size_t ocm_kmeans_px_workspace_bytes(int32_t problems, int64_t samples, int32_t attempts);
int ocm_op_kmeans_px(const uint8_t *pixels, int32_t problems, int64_t samples, const float *uniforms, int32_t attempts,
                     int32_t max_iter, double eps, uint8_t *labels, float *centers, double *compactness, int32_t *iters,
                     int32_t *best, uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Pillow's 8-bit resample: Image.resize, Image.crop(...).resize and ToTensor (sw_processing.py:217-231,
 * analyse_attention.py:102-120, data.py:18-122 and :189-215; kernels_resample.hip) ----
 * Restated from Pillow's libImaging (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the 8bpc passes; Geometry.c:
 * ImagingScaleAffine for NEAREST) and pinned on the live library by tests/test_resample_host.py. The filter values are
 * Pillow's: */
#define OCM_RESAMPLE_NEAREST 0
#define OCM_RESAMPLE_BILINEAR 2
#define OCM_RESAMPLE_BICUBIC 3
/* One axis' table (host, double arithmetic, no device): the source axis has in_size pixels, the box in0 .. in1 of it (rounded
 * to float32, as Pillow holds a box) becomes out_size pixels.
 *   scale = (in1 - in0) / out_size (the difference a float32), filterscale = max(scale, 1),
 *   support = filter support * filterscale (bilinear 1, bicubic 2 with a = -0.5), ksize = (int)ceil(support) * 2 + 1
 *   for xx in 0 .. out_size - 1: center = in0 + (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0);
 *     xmax = min((int)(center + support + 0.5), in_size) - xmin; w[x] = filter((x + xmin - center + 0.5) / filterscale), summed
 *     in index order and each divided by the sum when it is not 0; coeffs[xx][x] = (int)(+-0.5 + w[x] * 2^22), the sign of w[x];
 *     bounds[xx] = (xmin, xmax)
 * NEAREST is one tap of weight 2^22 (ksize 1) at ImagingScaleAffine's source index: xo = in0 + scale * 0.5, then xo += scale
 * per pixel, truncated; an index outside the axis leaves no tap (the pixel is 0).
 * bounds is [out_size][2], coeffs [out_size][ksize_padded] with the taps past a row's count zeroed; flip != 0 stores row xx
 * at out_size - 1 - xx (the resized axis mirrored: RandomHorizontalFlip / RandomVerticalFlip at no cost on the device). Taps
 * read outside the box, up to the ends of the axis, as Image.resize(box=) does; a crop (Image.crop(...).resize) is an axis of
 * its own: in_size = the rectangle's size, in0 = 0, in1 = in_size, with the rectangle's origin given to the operator.
 * ocm_resample_ksize returns ksize, or a negative OCM_E* code. Refused with OCM_EINVAL: an unknown filter, in_size < 1,
 * out_size < 1, in1 <= in0, a box outside 0 .. in_size, null pointers, ksize_padded < ksize. */
int32_t ocm_resample_ksize(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size);
int ocm_resample_table(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size, int32_t flip,
                       int32_t ksize_padded, int32_t *bounds, int32_t *coeffs);
/* The two passes for a batch (device, stream-ordered, nothing synchronises with the host). Horizontal first, into a uint8
 * intermediate in the workspace, then vertical from it — Pillow's order; the rounding between the passes is part of the result.
 * Each pass: acc = 2^21 + sum pixel * coeff in int32, clip(acc >> 22, 0, 255).
 * src: uint8, `batch` images of src_h x src_w pixels of `chans` (1 or 3) channels; pixel (b, y, x, c) is the byte at
 * b stride_b + y stride_y + x stride_x + c stride_c (HWC as decoded, planar CHW, a row pitch wider than the image, a stride
 * of 0 to repeat a plane). rects (device, [batch][4] = y0, x0, h, w; or null: the whole source) cuts image b's rectangle out
 * first: it is a source of its own, h x w pixels, and taps stop at its edges. The x tables are for in_size = w and the y
 * tables for in_size = h: [out][2] bounds and [out][ksize] coeffs shared by the batch (per_image 0), or one table per image,
 * [batch][out][...], padded to a common ksize (per_image 1: RandomResizedCrop's rectangles). tmp_rows is the number of
 * intermediate rows per image: at least the largest h (the src_h rows when rects is null).
 * Outputs, either or both: out_u8 (batch, out_h, out_w, chans) and out_f32 (batch, chans, out_h, out_w) = (float)u8 / 255.0f,
 * the IEEE float32 quotient (torchvision's ToTensor). Tables and rectangles are clamped on the device to the source and the
 * intermediate before use: wrong ones give wrong pixels, never an access outside the call's memory. The workspace (16-byte
 * aligned, ocm_resample_u8_workspace_bytes: 0 for arguments the operator refuses) needs no initialisation.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): null pointers, both outputs null, batch
 * outside 1..65535, chans other than 1 or 3, src_h outside 1..2^19, src_w outside 1..2^26, a negative stride, out_h outside
 * 1..65535, out_w * chans outside 1..2^26, a ksize < 1, tmp_rows outside 1..2^19 or (rects null) below src_h, a workspace that
 * is not 16-byte aligned. */
size_t ocm_resample_u8_workspace_bytes(int32_t batch, int32_t chans, int32_t tmp_rows, int32_t out_w);
int ocm_op_resample_u8(const uint8_t *src, int64_t stride_b, int64_t stride_y, int64_t stride_x, int64_t stride_c,
                       int32_t batch, int32_t chans, int32_t src_h, int32_t src_w, const int32_t *rects, int32_t tmp_rows,
                       const int32_t *xbounds, const int32_t *xcoeffs, int32_t xksize, const int32_t *ybounds,
                       const int32_t *ycoeffs, int32_t yksize, int32_t per_image, int32_t out_h, int32_t out_w, uint8_t *out_u8,
                       float *out_f32, void *workspace, size_t workspace_bytes, void *stream);

/* ---- DINO's augmentations per pixel: ColorJitter, RandomGrayscale, GaussianBlur, Solarization, ToTensor + Normalize
 * (dino/utils.py:36-68 and upstream main_dino.py's DataAugmentationDINO; kernels_augment.hip) ----
 * Restated from Pillow's libImaging (BoxBlur.c, Blend.c, Convert.c) and ImageEnhance / ImageOps, pinned on the live library by
 * tests/test_augment_host.py. Images are dense uint8 (batch, h, w, 3), 1..65535 images of up to 2^26 pixels; every per-image
 * choice is a table on the device, so one call serves a batch in which each image has its own parameters. Stream-ordered,
 * nothing synchronises with the host; float arithmetic is C's statements one by one (no fused multiply-add).
 *
 * ocm_op_color_u8: the point operations of one view, in that view's own order. out may be src. Per image:
 *   ops[4], factors[4]  four slots run in order, each OCM_COLOR_NONE or
 *     BRIGHTNESS / CONTRAST / SATURATION  ImageEnhance = Image.blend(degenerate, image, f): per byte in float32
 *       t = d + f * (x - d), truncated when 0 <= f <= 1, else clipped to 0..255 and truncated. d = 0 for brightness; the pixel's
 *       L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16 for saturation; int(mean(L) + 0.5) for contrast, the mean a double
 *       quotient of the exact integer sum of L over the image as it stands when that slot runs
 *     HUE  convert('HSV'), H += (int)factor modulo 256, convert('RGB') (Convert.c's float / double statements; round() puts
 *       halves away from zero); the factor holds the byte shift, torchvision's uint8(hue_factor * 255)
 *   flags[3]  grey != 0: L to all three channels (convert('L')); solarize != 0 with threshold: x < threshold ? x : 255 - x
 *             (ImageOps.solarize), after grey
 * The workspace (8-byte aligned, ocm_color_u8_workspace_bytes: 0 for a batch the operator refuses) holds one 64-bit sum per
 * image and slot; the operator zeroes it in stream order and the images add to it in integer atomics (exact in any order).
 * Factors are finite. Five launches: one per slot for the images whose slot is a contrast (the others leave at once), one to apply.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): null pointers, batch outside 1..65535, h or
 * w < 1, more than 2^26 pixels, a workspace that is not 8-byte aligned. */
#define OCM_COLOR_NONE 0
#define OCM_COLOR_BRIGHTNESS 1
#define OCM_COLOR_CONTRAST 2
#define OCM_COLOR_SATURATION 3
#define OCM_COLOR_HUE 4
size_t ocm_color_u8_workspace_bytes(int32_t batch);
int ocm_op_color_u8(const uint8_t *src, uint8_t *out, int32_t batch, int32_t h, int32_t w, const int32_t *ops,
                    const float *factors, const int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);
/* Image.filter(ImageFilter.GaussianBlur(radius)): three box-blur passes along the rows, then three along the columns, in 8.24
 * fixed point with the rounding to bytes after every pass.
 * ocm_gaussian_blur_table (host, no device) gives table[3] = r, ww, fw of one radius as BoxBlur.c forms them, in float variables:
 *   s2 = radius * radius / 3; L = sqrt(12.0 * s2 + 1.0); l = floor((L - 1.0) / 2.0);
 *   a = (2 l + 1)(l (l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)); fr = l + a;
 *   r = (int)fr; ww = (uint32)(2^24 / (2 fr + 1)); fw = (2^24 - (2 r + 1) ww) / 2
 * Radius 0 gives (0, 2^24, 0), the identity: "not blurred this time" shares the launch. Refused with OCM_EINVAL: a null table, a
 * radius that is NaN, negative or above 4096.
 * One pass of a line: out[x] = (ww * sum_{i=-r..r} in[clamp(x+i)] + fw * (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + 2^23) >> 24 in
 * uint32, the clamp to the line's ends on that pass's own input; r may exceed the line.
 * ocm_op_gaussian_blur_u8: table is device memory, [batch][3]. Two launches, one per axis: a workgroup holds whole lines in LDS
 * through the three passes, so an axis holds at most ocm_gaussian_blur_max_axis() = 1024 pixels. solarize (device, [batch], or
 * null) is a threshold per image applied after the blur, x < threshold ? x : 255 - x; 256 leaves the image as it is (upstream's
 * second global view solarizes after its blur). Outputs, either or both: out_u8 (batch, h, w, 3) and out_f32 (batch, 3, h, w) =
 * ((float)u8 / 255.0f - mean[c]) / std[c] as separate float32 operations (ToTensor, then Normalize's sub_().div_()); mean and std
 * are host arrays of three floats read during the call, both null for plain ToTensor. The workspace (ocm_gaussian_blur_u8_
 * workspace_bytes: 0 for arguments the operator refuses) needs no initialisation; out_u8 may be src.
 * Refused before any launch with OCM_EINVAL (a short or null workspace: OCM_ENOMEM): null src or table, both outputs null, one of
 * mean / std without the other, batch outside 1..65535, h or w outside 1..1024. */
int ocm_gaussian_blur_table(float radius, uint32_t *table);
int32_t ocm_gaussian_blur_max_axis(void);
size_t ocm_gaussian_blur_u8_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int ocm_op_gaussian_blur_u8(const uint8_t *src, int32_t batch, int32_t h, int32_t w, const uint32_t *table,
                            const int32_t *solarize, uint8_t *out_u8, float *out_f32, const float *mean, const float *std,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- the optimizer step, the gradient norm and its clipping (optimizer.py, utils.py:363 get_grad_norm, mim.py's and train.py's
 * clip_grad_norm_; kernels_optim.hip) ----
 * fp32 tensors, many per call: the host array `tensors` describes them, the operator cuts it into launches whose table of
 * pointers travels in the kernel arguments (no device copy of it, no allocation, nothing synchronises with the host). A
 * descriptor's pointers are device addresses of `count` contiguous floats each, 4-byte aligned; 16-byte loads and stores are
 * used for a tensor whose pointers are all 16-byte aligned, element accesses otherwise, and nothing past `count` elements is
 * touched. count == 0 is legal (its pointers are not looked at). An operator looks only at the pointers it uses; the others may
 * be null. */
typedef struct OcmOptimTensor {
    void *param; /* updated in place by the step */
    void *grad;  /* read by the step and the norm, scaled in place by the scale */
    void *m;     /* Adam / AdamW: exp_avg; SGD: momentum_buffer (unused with momentum == 0) */
    void *v;     /* Adam / AdamW: exp_avg_sq; SGD: unused */
    int64_t count;
} OcmOptimTensor;
#define OCM_OPTIM_ADAMW 0
#define OCM_OPTIM_ADAM 1
#define OCM_OPTIM_SGD 2
/* The values of one step, in double as torch's Python holds them; the operator forms the factors (1 - lr weight_decay,
 * 1 - beta1, 1 - beta2, 1 - dampening) in double and rounds each to float32 once. The caller forms the two that depend on the
 * step count: step_size = lr / (1 - beta1^step) and bias_correction2_sqrt = sqrt(1 - beta2^step).
 * The rules are torch's single-tensor ones, every operation rounded on its own:
 *   AdamW  p = p (1 - lr wd); m = m + (1 - beta1)(g - m); v = v beta2 + ((1 - beta2) g) g;
 *          p = p + (-step_size)(m / (sqrt(v) / bias_correction2_sqrt + eps))
 *   Adam   the same without the first statement and with g' = g + wd p for g (wd != 0; grad itself is not written)
 *   SGD    g' = g + wd p (wd != 0); with momentum != 0: m = g' when first_step, else m = m momentum + (1 - dampening) g';
 *          g' = g' + momentum m when nesterov, else m; then p = p + (-lr) g' */
typedef struct OcmOptimHyper {
    int32_t rule;       /* OCM_OPTIM_* */
    int32_t nesterov;   /* SGD */
    int32_t first_step; /* SGD: the momentum buffers hold nothing yet and are written from g' */
    int32_t reserved;
    double lr, beta1, beta2, eps, weight_decay, step_size, bias_correction2_sqrt, momentum, dampening;
} OcmOptimHyper;
/* The tensors one launch takes and the elements one workgroup takes (a multiple of 4). */
void ocm_optim_limits(int32_t *max_tensors, int32_t *chunk_elems);
/* One step of every tensor of the table under one set of values. Refused before any launch with OCM_EINVAL: a null table or
 * null hyper-parameters, n < 0, an unknown rule, non-finite values (bias_correction2_sqrt <= 0 for the Adam rules), a count
 * outside 0..2^36, a null or misaligned pointer the rule uses in a descriptor with count > 0. */
int ocm_op_optim_step(const OcmOptimTensor *tensors, int32_t n, const OcmOptimHyper *hyper, void *stream);
/* The 2-norm of all gradients of the table. One workgroup per chunk writes the float64 sum of the squares (each square formed in
 * float64) to the workspace, a last workgroup adds them: *sumsq = the total (float64), *norm = (float)sqrt(total), *coef =
 * min(max_norm / (norm + 1e-6f), 1) in float32 as torch.nn.utils.clip_grad_norm_ forms it (a NaN norm gives NaN, an infinite one
 * 0). All three are device addresses. Every sum has one fixed order and there are no atomics: equal gradients give equal bits on
 * every call, aligned or not. The workspace (8-byte aligned) needs no initialisation; its size depends on the counts alone and
 * is 0 for a table the operator refuses. Refused with OCM_EINVAL: as above (only grad is looked at), null outputs, a null, short
 * or misaligned workspace. */
size_t ocm_grad_norm_workspace_bytes(const OcmOptimTensor *tensors, int32_t n);
int ocm_op_grad_norm(const OcmOptimTensor *tensors, int32_t n, double max_norm, double *sumsq, float *norm, float *coef,
                     void *workspace, size_t workspace_bytes, void *stream);
/* grad = grad * *coef for every gradient of the table, the coefficient read from device memory by the kernel. */
int ocm_op_grad_scale(const OcmOptimTensor *tensors, int32_t n, const float *coef, void *stream);

/* param = param * m + grad * (1 - m) for every tensor of the table: the teacher's exponential moving average of DINO
 * (dino/utils.py ema_update; param = the teacher's tensor, grad = the student's), torch's p.mul_(m).add_((1 - m) * q): 1 - m is
 * formed in double and rounded to float once, then three separately rounded operations, no FMA. The launcher and limits of the
 * optimizer step: 16-byte accesses for a tensor whose two pointers are 16-byte aligned, element accesses otherwise, count == 0
 * legal. Refused with OCM_EINVAL: as ocm_op_optim_step (param and grad are looked at), a non-finite momentum. */
int ocm_op_ema_update(const OcmOptimTensor *tensors, int32_t n, double momentum, void *stream);

/* ---- DINO self-distillation (dino/vision_transformer.py DINOHead, dino/utils.py DINOLoss; kernels_dino.hip) ----
 * Row kernels over fp32 data: one workgroup per row (or per slice of 4096 columns of the loss), 16-byte loads and stores for a row
 * whose address is 16-byte aligned, element accesses otherwise and for the tail of any length. Every reduction runs in float64 in
 * an order fixed by the shapes alone (no atomics): equal inputs give equal bits. Every output element is written exactly once,
 * nothing synchronises with the host, and bad arguments (null or misaligned pointers, shapes outside the stated ranges) are
 * refused with OCM_EINVAL before any launch. */

/* F.normalize(x, p = 2, dim = -1) over `rows` rows of `dim` floats: norm[r] = max(|x[r]|_2, 1e-12), y = x / norm. rows >= 1,
 * dim >= 1. */
int ocm_op_l2_normalize(const float *x, float *y, float *norm, int64_t rows, int32_t dim, void *stream);
/* dx = (dy - y (y . dy)) / norm from the forward's y and norm; a row whose norm is the clamp (<= 1e-12) gets dx = dy / norm, the
 * gradient torch's graph gives through clamp_min. dx may alias dy. */
int ocm_op_l2_normalize_backward(const float *dy, const float *y, const float *norm, float *dx, int64_t rows, int32_t dim,
                                 void *stream);

/* nn.utils.weight_norm (dim = 0) of a Linear: w[n][:] = g[n] v[n][:] / |v[n]|_2 for v [N][K], g [N]; norm[n] = |v[n]|_2. */
int ocm_op_weight_norm(const float *v, const float *g, float *w, float *norm, int32_t N, int32_t K, void *stream);
/* From dw [N][K]: dg[n] = (dw[n] . v[n]) / norm[n], dv[n] = g[n] / norm[n] (dw[n] - v[n] (dw[n] . v[n]) / norm[n]^2). Either of
 * dg, dv may be NULL (not both). dv may alias dw. */
int ocm_op_weight_norm_backward(const float *dw, const float *v, const float *g, const float *norm, float *dg, float *dv, int32_t N,
                                int32_t K, void *stream);

/* The DINO loss. student [V*B][K] crop-major (crop v owns rows v*B .. v*B + B - 1), teacher [2*B][K], center [K];
 *   q[i,b,:] = softmax((teacher[i,b,:] - center) / teacher_temp), l[v,b,:] = log_softmax(student[v,b,:] / student_temp),
 *   loss = 1 / (2 (V - 1)) sum_i sum_{v != i} (1 / B) sum_b sum_k -q[i,b,k] l[v,b,k],
 * every softmax with its row maximum subtracted. Two passes over the logits: the row statistics (row_stats[(V + 2) * B][2]
 * float64: the maximum and the sum of exp(z - max) of every student row, then of every teacher row), then the 2 x V table of
 * q_i . S_v per image through the workspace, from which sum_k q l = (q . S_v) / student_temp - lse_v. loss_out[1] is device
 * memory. V >= 2, B >= 1, K >= 1, temperatures finite and > 0; K <= 65535 * 4096. row_stats 8-byte aligned. */
size_t ocm_dino_loss_workspace_bytes(int32_t B, int32_t V, int32_t K);
int ocm_op_dino_loss(const float *student, const float *teacher, const float *center, float student_temp, float teacher_temp,
                     int32_t B, int32_t V, int32_t K, float *loss_out, double *row_stats, void *workspace, size_t workspace_bytes,
                     void *stream);
/* One pass: dstudent[v,b,k] = grad_loss[0] / (2 (V - 1) B student_temp) (c_v p[v,b,k] - sum_{i != v} q[i,b,k]), p =
 * softmax(student / student_temp), c_v = 1 for v < 2 and 2 otherwise; grad_loss[1] is read from device memory, row_stats is
 * the forward's. No workspace. */
int ocm_op_dino_loss_backward(const float *grad_loss, const float *student, const float *teacher, const float *center,
                              float student_temp, float teacher_temp, int32_t B, int32_t V, int32_t K, const double *row_stats,
                              float *dstudent, void *stream);

/* The centre of the DINO loss, in two calls because a distributed run all-reduces batch_sum in between:
 *   OCM_DINO_CENTER_SUM     batch_sum[k] = ((teacher[0][k] + teacher[1][k]) + teacher[2][k]) + ... over `rows` rows, in fp32
 *                           (center, count, momentum unused)
 *   OCM_DINO_CENTER_UPDATE  center = center * m + (batch_sum / count) * (1 - m), count = rows * world size rounded to float,
 *                           1 - m formed in double and rounded once, each operation rounded on its own (teacher, rows unused) */
#define OCM_DINO_CENTER_SUM 0
#define OCM_DINO_CENTER_UPDATE 1
int ocm_op_dino_center(int32_t mode, const float *teacher, int64_t rows, int32_t K, float *batch_sum, float *center, double count,
                       double momentum, void *stream);

/* ---- sliding-window index math (host, integer; sw_processing.py:151-163) ---- */
/* Number of windows per axis: len(range(0, size - 2*stride, stride)). */
int32_t ocm_sw_count(int32_t size, int32_t stride);
/* Row-major (y0, x0) origins for an (height x width) image; returns the number of
 * windows written (<= cap) or a negative OCM_E* code. */
int32_t ocm_sw_origins(int32_t height, int32_t width, int32_t stride, int32_t *origins_yx,
                       int32_t cap);
/* Contiguous block partition of `n_tiles` over `world` ranks:
 * rank r owns [*begin, *end); every rank's padded share is ceil(n_tiles/world). */
int32_t ocm_sw_shard(int32_t n_tiles, int32_t world, int32_t rank, int32_t *begin, int32_t *end);

#ifdef __cplusplus
}
#endif
#endif /* OCM_VIT_H */
