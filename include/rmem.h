/* librmem_hip.so -- C ABI of the MI355X (gfx950) space-time memory-reading engine.
 *
 * The reference (Bardli/RMem_ocu) has no FFI: its hot path is nn.Modules calling
 * ATen/cuDNN kernels.  This header is the boundary one level below
 * the reference's Python inference API; each entry point names the reference call
 * site(s) whose vendor kernels it replaces (paths relative to aot_plus/).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work and never
 *     synchronise, so a caller may wrap any sequence of them in a hipGraph capture;
 *   - return value: 0 on success, negative on error (rmem_last_error_string() says why);
 *     no exception crosses the boundary; the only global mutable state is the
 *     thread-local error string and the opt-in launch timers (rmem_profile_* /
 *     rmem_gated_profile_*: process-wide, mutex-protected, off unless started);
 *   - "bf16" = IEEE bfloat16 stored as uint16; feature maps are NHWC with N = 1, which
 *     for the LSTT is the same memory as the reference's [L, B=1, C] token layout;
 *   - leading dimensions (ld*) are in elements.
 */
#ifndef RMEM_H_
#define RMEM_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMEM_ABI_VERSION 15

int rmem_abi_version(void);
const char* rmem_last_error_string(void);

/* ------------------------------------------------------------------ convolution / linear
 * Implicit-GEMM NHWC convolution, bf16 in, fp32 accumulate:
 *   y = act(conv(x, w) + bias (+ residual)),  optional y2 = bf16(conv(x, w) + bias).
 * Replaces: encoders/resnet.py:48-68, 179-195 (conv + FrozenBatchNorm2d folded into w/bias + ReLU
 * + residual), models/aot.py:25-29, 133 (encoder_projector), models/aot.py:68-74, 112 (id bank),
 * decoders/fpn.py:22-32 (ConvGN convs, adapters, conv_out), and every nn.Linear of
 * layers/transformer.py:487-512 and layers/attention.py:19-25 (a 1x1 conv with H = rows, W = 1).
 * w is [Cout][KH][KW][Cin] bf16; Cin must be a multiple of 8. */
typedef struct rmem_conv_desc {
  int H, W, Cin;      /* input feature map */
  int Ho, Wo, Cout;   /* output feature map (checked against the geometry) */
  int KH, KW, stride, pad;
  int ldo;            /* y row stride  (>= Cout) */
  int ldr;            /* residual row stride */
  int ld2;            /* y2 row stride */
  int relu;           /* activation after bias/residual: 0 none, 1 ReLU, 2 exact (erf) GELU, 3 SiLU (layers/attention.py:89) */
  int out_f32;        /* 1: y is fp32, 0: bf16 */
  int res_f32;        /* 1: residual is fp32, 0: bf16 */
  int ldx;            /* 1x1 stride-1 problems only: input row stride in elements (0 = Cin); lets a GEMM read a column
                         range of a wider activation buffer (the torch.split / torch.cat of transformer.py:1104-1124) */
  int batch;          /* images in x / y (0 or 1 = one): x is [batch][H][W][Cin], y [batch][Ho][Wo] rows of ldo; several
                         clips' frames go through the encoder as one launch per layer */
  int act_begin;      /* the activation applies to output channels >= act_begin (multiple of 8; 0 = all): one GEMM for
                         linear_QV, whose Q half is raw and whose V half goes through SiLU (transformer.py:1104-1110) */
  int res_up_h, res_up_w, res_up_align;
                      /* res_up_h > 0: `residual` is a LOWER-resolution bf16 map [batch][res_up_h][res_up_w] rows of ldr and is
                         bilinearly resized to (Ho, Wo) on the fly (rounded to bf16 like rmem_bilinear_nhwc, so both routes
                         are bit-identical): `F.interpolate(x, size) + adapter(shortcut)` of decoders/fpn.py:49-52, 57-60
                         without materialising the resized map.  Needs Cout % 8 == 0 and 16-byte aligned operands. */
} rmem_conv_desc;

/* Problems with few output tiles are cut along K (split-K) when a workspace of at least
 * rmem_conv_workspace_bytes(desc) bytes is supplied (fp32 slabs, summed in slice order: reproducible);
 * workspace may be NULL (no split-K). */
size_t rmem_conv_workspace_bytes(const rmem_conv_desc* desc);
int rmem_conv2d_nhwc(const rmem_conv_desc* desc, const void* x, const void* w, const float* bias,
                     const void* residual, void* y, void* y2, void* workspace, void* stream);

/* The launch plan of a convolution / linear problem: which kernel family, ring depth, split count and grid rmem_conv2d_nhwc,
 * rmem_conv1x1_dual_nhwc or rmem_linear_grouped give it.  A pure host function of the geometry (no pointer, no GPU): the three
 * entry points take their decision from the same function.  The same for both element types. */
enum rmem_gemm_family {
  RMEM_GEMM_GENERAL64 = 0, /* 64x64 tile, per-lane addresses (any Cin % 8 == 0); the only family that is split along K */
  RMEM_GEMM_SCALAR64 = 1,  /* 64x64, scalar k-walk (Cin % 64 == 0) */
  RMEM_GEMM_ROWRUN64 = 2,  /* 64x64, row-run (KW * Cin contiguous elements per filter row) */
  RMEM_GEMM_ONE128 = 3,    /* 128x128, scalar k-walk, every wave loads and multiplies */
  RMEM_GEMM_PC128 = 4,     /* 128x128, scalar k-walk, producer / consumer waves (512 threads) */
  RMEM_GEMM_ROWRUN128 = 5, /* 128x128, row-run */
  RMEM_GEMM_DUAL64 = 6,    /* rmem_conv1x1_dual_nhwc, 64x64 */
  RMEM_GEMM_DUAL128 = 7,   /* rmem_conv1x1_dual_nhwc, 128x128 */
  RMEM_GEMM_GROUPED = 8    /* rmem_linear_grouped, 64x64 (scalar k-walk when fast == 1, else per-lane addresses) */
};
enum rmem_gemm_entry { RMEM_GEMM_ENTRY_CONV2D = 0, RMEM_GEMM_ENTRY_DUAL = 1, RMEM_GEMM_ENTRY_GROUPED = 2 };
typedef struct rmem_gemm_plan {
  int family;           /* enum rmem_gemm_family */
  int tile;             /* output tile edge: 64 or 128 */
  int ring;             /* LDS ring depth of the k-loop: 1, 2 or 3 */
  int is1x1;            /* 1x1 stride-1 pad-0 problem (a plain GEMM) */
  int fast;             /* address form the geometry allows: 0 general, 1 scalar k-walk, 2 row-run */
  int splits;           /* > 1: split along K over grid_z, followed by the slab-summing epilogue kernel */
  int steps_per_split;  /* k-steps (of 64) per slice; all of them when splits == 1 */
  int xcd_ny;           /* > 0: 1-D grid in XCD-aware order, xcd_ny column tiles per row tile; 0: plain 2-D grid */
  int grid_x, grid_y, grid_z, threads;
} rmem_gemm_plan;
/* desc as for the entry point named by `entry` (enum rmem_gemm_entry); has_workspace: a split-K workspace would be passed
 * (rmem_conv2d_nhwc only); extra: Cin2 of rmem_conv1x1_dual_nhwc, n of rmem_linear_grouped, otherwise ignored.
 * Returns -1 for the geometry errors the entry point itself reports. */
int rmem_conv_plan(const rmem_conv_desc* desc, int has_workspace, int entry, int extra, rmem_gemm_plan* plan);

/* n <= 4 GEMMs of IDENTICAL shape (desc: 1x1, stride 1) with different operands as one launch: the per-layer linears of one
 * memory update (linear_QMem / linear_VMem / linear_V of layers/transformer.py:279-285 for the 3 LSTT layers) do not depend on
 * each other, and at M = HW = 1674 a launch costs more than its arithmetic.  bias / residual may be NULL or hold NULLs. */
int rmem_linear_grouped(const rmem_conv_desc* desc, int n, const void* const* x, const void* const* w,
                        const float* const* bias, const void* const* residual, void* const* y, void* stream);

/* y = act([x | x2 sampled at stride2] * w_cat^T + bias): the closing 1x1 convolution of a ResNet bottleneck and its (strided) 1x1
 * shortcut (encoders/resnet.py:48-68: `out = conv3(out); identity = downsample(x); out += identity; relu`) as ONE GEMM over
 * K = desc->Cin + Cin2, so the shortcut tensor is neither written nor re-read.  desc describes the dense 1x1 problem on x
 * (batch, H = Ho, W = Wo, Cin, Cout, relu, ldo; no residual); x2 is NHWC [batch][H2][W2][Cin2] with (H2 - 1) / stride2 + 1 == Ho;
 * w_cat is [Cout][Cin + Cin2] bf16 (both BN-folded weights side by side), bias the sum of both folded biases.
 * Cin and Cin2 must be multiples of 64. */
int rmem_conv1x1_dual_nhwc(const rmem_conv_desc* desc, const void* x, const void* x2, int H2, int W2, int Cin2, int stride2,
                           const void* w_cat, const float* bias, void* y, void* stream);

/* The tail of a ResNet bottleneck chained into the FIRST 1x1 convolution of the following block, one launch
 * (encoders/resnet.py:62-68 of block i, then :48-50 of block i + 1 -- or of the next layer's first block):
 *   y  = relu(b . w3^T + bias3 + res)      b [M][K1] (the 3x3 conv's output), w3 [Cout][K1], res / y [M][Cout], M = batch * Ho * Wo
 *   a2 = relu(y . w1^T + bias1)            w1 [N2][Cout], a2 [M][N2]; Cout = 256 with N2 = 64 or 128, or Cout = 512 with N2 = 128 or 256
 * y is stored (later blocks need it as their shortcut) but never read back: its 64-row tile stays in LDS, rounded as stored, as the
 * A operand of the second GEMM (Cout = 512: in two column chunks of 256, the second GEMM's accumulators persisting).  Dual form (x2 != NULL, res == NULL; the block with the strided 1x1 shortcut, as
 * rmem_conv1x1_dual_nhwc): y = relu([b | x2 sampled at stride2] . w3^T + bias3) with w3 [Cout][K1 + Cin2], x2 NHWC [batch][H2][W2][Cin2].
 * Bit-identical to rmem_conv2d_nhwc (or rmem_conv1x1_dual_nhwc) followed by rmem_conv2d_nhwc.  K1, Cin2 multiples of 64. */
typedef struct rmem_bneck_chain_desc { int batch, Ho, Wo, K1, Cout, N2, H2, W2, Cin2, stride2; } rmem_bneck_chain_desc;
int rmem_bneck_chain(const rmem_bneck_chain_desc* desc, const void* b, const void* x2, const void* w3, const float* bias3, const void* res,
                     void* y, const void* w1, const float* bias1, void* a2, void* stream);

/* A whole ResNet bottleneck with planes = 64 and stride 1 (layer 1) in one launch, NHWC (csrc/bneck_block.hip):
 *   a = relu(conv1x1(x; w1, bias1)), b = relu(conv3x3(a; w2, bias2)) with pad 1 (a is padded with zeros),
 *   Cin = 256, identity form:   y = relu(b . w3^T + bias3 + x), w3 [256][64];
 *   Cin = 64, projection form:  y = relu([b | x] . w3^T + bias3), w3 the packed [256][64 + 64] of rmem_conv1x1_dual_nhwc;
 *   N2 = 128 (identity form only), tail: a_next = relu(y . w1n^T + bias1n), w1n [128][256], y rounded as stored; N2 = 0: w1n,
 *   bias1n and a_next are NULL.
 * x [images][H][W][Cin], w1 [64][Cin], w2 [64][3][3][64], y [images][H][W][256], a_next [images][H][W][128].  It replaces the
 * launch list rmem_conv2d_nhwc (1x1) + rmem_conv3x3_direct + rmem_conv2d_nhwc with residual / rmem_conv1x1_dual_nhwc
 * (+ rmem_conv2d_nhwc for the tail), or the rmem_bneck_chain form of it (encoder_batch.py), and is bit-identical to both.
 * The environment variable RMEM_BNECK_ROWS forces the rows a workgroup walks down (tests); results do not depend on it. */
typedef struct rmem_bneck_block_desc { int images, H, W, Cin, N2; } rmem_bneck_block_desc;
int rmem_bneck_block64(const rmem_bneck_block_desc* desc, const void* x, const void* w1, const float* bias1, const void* w2, const float* bias2,
                       const void* w3, const float* bias3, void* y, const void* w1n, const float* bias1n, void* a_next, void* stream);

/* ------------------------------------------------------------------ memory-read attention
 * out[q, 32h:32h+32] = softmax_k( (Q[q,h]+pe_cur[h]) . (K[k,h]+pe_mem[slot(k),h]) / sqrt(32) ) V[k,h]
 * over the keys named by the chunk table, plus (optionally) the per-memory-frame probability mass
 * mass[q, t] = mean_h sum_{k in frame t} p[h, q, k].
 * Replaces: layers/attention.py:45-64 as called from layers/transformer.py:632-635 (long-term),
 * the K + temporal-PE materialisation of transformer.py:594-626, and the attention-weight recording of
 * transformer.py:636-643.  With chunks == NULL it is plain attention over one key frame of lk_single
 * keys split into nchunks ranges (transformer.py:569 self-attention, 657-662 short-term attention).
 * The output is pre-projection (attention.py:79 is a rmem_conv2d_nhwc call).
 * Head dim is fixed at 32; heads <= 8. */
typedef struct rmem_attn_chunk {
  int slot;       /* bank slot: keys at k_bank + slot * slot_stride */
  int key_begin;  /* first key (row) of the chunk inside the slot */
  int key_count;  /* >= 0; 0 = padding row (no keys, no mass): lets clips with shorter banks share a launch, rmem_mem_read_attn_clips */
  int pe_slot;    /* row of pe_mem added to these keys, or -1 */
  int t;          /* memory-frame index the chunk's probability mass is credited to */
  int reserved[3];
} rmem_attn_chunk;

size_t rmem_attn_workspace_bytes(int Lq, int heads, int nchunks);

int rmem_mem_read_attn(const void* q, int ldq,                     /* bf16 [Lq][ldq] */
                       const void* k_bank, const void* v_bank,     /* bf16, rows [Lk][ldkv] per slot */
                       long long slot_stride, int ldkv,
                       const rmem_attn_chunk* chunks, int nchunks, /* device table, or NULL */
                       int lk_single,                              /* keys when chunks == NULL; with a table: total keys
                                                                      named by it (used by rmem_profile_* only) */
                       const float* pe_cur,                        /* fp32 [C] or NULL */
                       const float* pe_mem,                        /* fp32 [4][C] or NULL */
                       int Lq, int heads,
                       void* out, int ldo,                         /* bf16 [Lq][ldo] */
                       float* attn_mass, int T,                    /* fp32 [Lq][T] or NULL */
                       void* workspace, void* stream);

/* The same for nclips independent clips of identical shape in ONE launch (clips of a group advance in lockstep): clip c's
 * queries / one-frame keys / outputs sit c * {q, kv, out}_clip_stride elements further, its chunk-table rows are
 * chunks[c * nchunks ...] (bank slots in them are global indexes into k_bank / v_bank), its mass is attn_mass + c * Lq * T,
 * the workspace is nclips times rmem_attn_workspace_bytes. */
int rmem_mem_read_attn_clips(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv,
                             const rmem_attn_chunk* chunks, int nchunks, int lk_single, const float* pe_cur, const float* pe_mem,
                             int Lq, int heads, void* out, int ldo, float* attn_mass, int T, int nclips,
                             long long q_clip_stride, long long kv_clip_stride, long long out_clip_stride,
                             void* workspace, void* stream);

/* The long-term memory read AND the short-term attention of an LSTT block (layers/transformer.py:632-635, 656-662) as ONE launch:
 * both use the same queries (curr_Q) and are independent of each other, so the short-term attention's workgroups ride behind the
 * memory read's as extra grid slices (every XCD gets its share of both) instead of a second launch that starts on an empty
 * GPU.  The memory read is exactly rmem_mem_read_attn_clips with a chunk table (out_long, attn_mass); the second attention
 * is softmax(Q K_short^T / sqrt(32)) V_short over lk_short keys of one frame per clip ([lk_short][ldkv] rows, clip c at
 * c * kv_short_clip_stride), no temporal embedding, written to out_short ([Lq][ldo] rows, clip c at c * out_short_clip_stride).
 * Results are bit-identical to the two separate launches. */
int rmem_lstt_attn_pair_clips(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv,
                              const rmem_attn_chunk* chunks, int nchunks, int lk_total, const float* pe_cur, const float* pe_mem,
                              int Lq, int heads, void* out_long, int ldo, float* attn_mass, int T, int nclips,
                              long long q_clip_stride, long long out_clip_stride,
                              const void* k_short, const void* v_short, int lk_short, long long kv_short_clip_stride,
                              void* out_short, long long out_short_clip_stride, void* workspace, void* stream);

/* The same launch with the merge of the key groups DEFERRED to the consumer of out_long.  At bench geometry the memory read
 * splits the keys into several groups (RMEM_ATTN_WGS) whose normalised partial outputs and (m, l) pairs a row-local pass then
 * merges into out_long; this form does not launch that pass when there is more than one group and fills *merge with what the
 * merge needs, for rmem_lstt_chain_b_merged to do it while it stages its rows (out_long is then neither written nor read).
 * With one group nothing changes: out_long is final and merge->ngroups = 1.  The mass output is as in the plain form. */
typedef struct rmem_attn_merge {
  int ngroups, heads, Lq, reserved;   /* key groups (<= 1: nothing was deferred), heads, queries per clip */
  const void* opart;                  /* partial outputs, normalised by their own sum: 16-bit [clip][group][head][8][Lq][4] */
  const float* mlg;                   /* (reference maximum, sum) of every partial: fp32 [clip][group][head][Lq][2] */
  long long opart_cs, mlg_cs;         /* clip strides of the two, in 4-byte units */
} rmem_attn_merge;
int rmem_lstt_attn_pair_clips_deferred(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv,
                                       const rmem_attn_chunk* chunks, int nchunks, int lk_total, const float* pe_cur, const float* pe_mem,
                                       int Lq, int heads, void* out_long, int ldo, float* attn_mass, int T, int nclips,
                                       long long q_clip_stride, long long out_clip_stride,
                                       const void* k_short, const void* v_short, int lk_short, long long kv_short_clip_stride,
                                       void* out_short, long long out_short_clip_stride, void* workspace,
                                       rmem_attn_merge* merge, void* stream);

/* Optional timing of the memory-read launches (chunks != NULL) with HIP events on the launch stream:
 * between start and stop every such launch outside a graph capture is bracketed by two events;
 * start() also calibrates what an event bracket costs around an empty kernel and stop() subtracts that per launch;
 * stop() synchronises on the events and returns the summed kernel time, the summed algorithmic FLOPs
 * (4 * Lq * keys * C per launch) and the launch count.  Used by bench.py's roofline leg. */
int rmem_profile_start(int max_launches);
int rmem_profile_stop(double* total_ms, double* total_flops, int* launches);

/* ------------------------------------------------------------------ normalisation / activation
 * LayerNorm over 256 channels of (a [+ b]); writes any of: bf16 y, fp32 y, bf16 (y + pos).
 * Replaces: layers/transformer.py:566-568 (norm1 and with_pos_embed), 574 (norm2), 659-660 (norm4 of a
 * sum), 683 (norm3), 250-259 (decoder_norms). */
int rmem_layernorm256(const void* a, int a_is_f32, int lda, const void* b, int b_is_f32, int ldb,
                      const float* gamma, const float* beta, float eps, int M,
                      void* y_bf16, int ldy, const float* pos, void* ypos_bf16, int ldyp,
                      float* y_f32, int ldyf, void* stream);

/* Two LayerNorm(256) of summed bf16 inputs with ONE weight set as one launch: y0 = LN(a0 + b0), y1 = LN(a1 + b1), all
 * [M][256] bf16 contiguous.  Replaces the two norm4 calls of layers/transformer.py:659-660. */
int rmem_layernorm256_pair(const void* a0, const void* b0, void* y0, const void* a1, const void* b1, void* y1,
                           const float* gamma, const float* beta, float eps, int M, void* stream);

/* ------------------------------------------------------------------ LSTT block chains (row-local sequences as ONE launch)
 * Between its three attentions an LSTT block (layers/transformer.py:553-692) is a sequence of row-local operations on the
 * [tokens][256] residual stream.  Each entry point below runs one such sequence for all rows of `clips` clips of L tokens
 * (rows are [clip][token], everything contiguous unless a leading dimension is given), a workgroup owning 32 or 64 consecutive
 * tokens of one clip (rmem_lstt_chain_rows) with the rows resident in LDS; results do not depend on that choice and are bit-identical to the same sequence of rmem_conv2d_nhwc /
 * rmem_layernorm256 / rmem_layernorm256_pair launches (same accumulation order, same points of rounding).
 * Weights are 16-bit [N][K] matrices (nn.Linear layout) re-packed once in FRAGMENT ORDER for NW = rmem_lstt_chain_waves()
 * waves per workgroup: [N / 256][NW][K / 32][16 / NW][64][8] = [column block][wave][k chunk][column tile j][lane][8 consecutive k],
 * element (n, k) with n = 256 nb + (256 / NW) wave + 16 j + (lane & 15), k = 32 kc + 8 (lane >> 4) + e
 * (rmem_ocu_amd/pack.py::pack_frag), so that a wave reads one MFMA B fragment as 1 KiB of contiguous memory.  Biases and
 * LayerNorm parameters are fp32; every pointer must be 16-byte aligned.
 *
 * chain A, after the self attention (transformer.py:571-576, 659-660):
 *   x += att . w_proj^T + b_proj;  curr_v = LN2(x);  curr_q = curr_v . w_q^T + b_q;
 *   k4 = LN4(short_k + curr_q);  v4 = LN4(short_v + curr_v) */
int rmem_lstt_chain_waves(void);      /* waves per workgroup the chain kernels were built for (4 or 8): the weight packing depends on it */
/* Rows per workgroup a chain launch over `clips` clips of L tokens takes on a device with `cus` compute units: 64 when the
 * 32-row grid, ceil(L / 32) * clips workgroups of one per CU, would need more than one round, else 32.  A pure function; the
 * launches apply it to the current device unless the environment sets RMEM_CHAIN_ROWS = 32 | 64 (read per call). */
int rmem_lstt_chain_rows(int L, int clips, int cus);
typedef struct rmem_chain_a_desc {
  int L, clips; float eps; int reserved;
  const void* att; float* x;
  const void* w_proj; const float* b_proj; const float* ln2_g; const float* ln2_b; void* curr_v;
  const void* w_q; const float* b_q; void* curr_q;
  const void* short_k; const void* short_v; const float* ln4_g; const float* ln4_b; void* k4; void* v4;
} rmem_chain_a_desc;
int rmem_lstt_chain_a(const rmem_chain_a_desc* d, void* stream);

/* chain B, after the long-term and the short-term attention (transformer.py:635, 662, 673-685):
 *   x += att_long . w_long^T + b_long;  tgt3 = att_short . w_short^T + b_short;  x += tgt3;  h1 = LN3(x) . w1^T + b1   ([rows][1024])
 * gn_partial (optional): per-32-row-block (sum, sum of squares) of h1 over each of the 32 GroupNorm groups of 32 channels,
 * fp32 [clips][32][gn_splits][2], entry `split` = the 32-row block whatever the workgroup's height (gn_splits >= ceil(L / 32); the caller keeps the unused
 * entries zero): with gn_splits = 64 the statistics rmem_gn_act_dwconv5x5_prestats_nhwc_images consumes (layers/basic.py:27-35). */
typedef struct rmem_chain_b_desc {
  int L, clips; float eps; int gn_splits;
  const void* att_long; const void* att_short; float* x;
  const void* w_long; const float* b_long; const void* w_short; const float* b_short; void* tgt3;
  const float* ln3_g; const float* ln3_b; const void* w1; const float* b1; void* h1; float* gn_partial;
} rmem_chain_b_desc;
int rmem_lstt_chain_b(const rmem_chain_b_desc* d, void* stream);
/* chain B behind rmem_lstt_attn_pair_clips_deferred: with merge->ngroups > 1 the rows of att_long are not read from d->att_long
 * but merged from the memory read's key groups while they are staged, per (row, head, 4 channels) exactly the merge pass's
 * sequence (maximum over the groups with l > 0, w = exp2(m - m_max) l, weighted sum in group order, times 1 / sum of w, one
 * rounding to 16 bits): bit-identical to the merge pass followed by rmem_lstt_chain_b.  merge->ngroups <= 1: rmem_lstt_chain_b.
 * *merge is read at the call (the deferred launch fills it just before), heads must be 8 and Lq = d->L. */
int rmem_lstt_chain_b_merged(const rmem_chain_b_desc* d, const rmem_attn_merge* merge, void* stream);

/* chain C, after GroupNorm + GELU + depth-wise 5x5 (transformer.py:685-687, 250-259; 565-569 of the NEXT block):
 *   h3 != NULL:     x += h3 . w2^T + b2  (h3 [rows][1024]);  dec_out[row * ld_dec + 0..255] = LN_dec(x)
 *   w_qkv != NULL:  qkv = LN1'(x) . w_qkv^T + b_qkv + pos_qk  ([rows][768]; pos_qk fp32 [rows][768]) of the next block
 * (h3 == NULL: the first block of the stack, x as the projector left it; w_qkv == NULL: the last block). */
typedef struct rmem_chain_c_desc {
  int L, clips; float eps; int ld_dec;
  float* x;
  const void* h3; const void* w2; const float* b2; const float* dec_g; const float* dec_b; void* dec_out;
  const float* ln1_g; const float* ln1_b; const void* w_qkv; const float* b_qkv; const float* pos_qk; void* qkv;
} rmem_chain_c_desc;
int rmem_lstt_chain_c(const rmem_chain_c_desc* d, void* stream);

/* LayerNorm over C in {128, 256, 512, 1024} channels; bf16 and/or fp32 output.  Replaces the nn.LayerNorm call sites of the
 * Swin-B encoder (encoders/swin/swin_transformer.py:266, 318, 354, 538, 704).  Rows move as 8 / 16-byte vectors: lda, ldy, ldyf
 * multiples of 4, a / y_f32 / gamma / beta 16-byte and y_bf16 8-byte aligned. */
int rmem_layernorm(const void* a, int a_is_f32, int lda, const float* gamma, const float* beta, float eps, int M, int C,
                   void* y_bf16, int ldy, float* y_f32, int ldyf, void* stream);

/* Swin patch merging without the linear: gather the 2x2 neighbourhood of every output token of an fp32 [H][W][C] map
 * (zero beyond an odd border), LayerNorm over 4C, bf16 [ceil(H/2)*ceil(W/2)][4C] (swin_transformer.py:336-355; the
 * reduction Linear at 356 is a rmem_conv2d_nhwc call).  C in {128, 256}. */
int rmem_patch_merge_ln(const float* x, int H, int W, int C, const float* gamma, const float* beta, float eps,
                        void* y_bf16, void* stream);
/* the same over a batch: x fp32 [images][H][W][C] -> y [images][ceil(H/2)*ceil(W/2)][4C] (encoder_batch.SwinBatchEncoder) */
int rmem_patch_merge_ln_images(const float* x, int images, int H, int W, int C, const float* gamma, const float* beta, float eps,
                               void* y_bf16, void* stream);

/* Swin (shifted-)window attention over a [H][W] token map, 7x7 windows, head dim 32: padding, cyclic shift, window
 * partition / reverse, relative-position bias and the shifted-window mask are index arithmetic inside the kernel.
 * qkv: bf16 [H*W][3C] (q | k | v); qkv_bias: fp32 [3C] (what a padded zero token projects to);
 * bias_mask_table: fp32 [4][heads][49][49] = (relative_position_bias + mask of window type t) * log2(e), type = 2 * (last
 * window row) + (last window column) (only type 0 is read when shift == 0); out: bf16 [H*W][C], pre-projection.
 * Replaces encoders/swin/swin_transformer.py:156-195 and the token plumbing of 263-305. */
int rmem_window_attn(const void* qkv, const float* qkv_bias, const float* bias_mask_table, void* out, int H, int W,
                     int C, int heads, int shift, void* stream);
/* the same over a batch of token maps: qkv [images][H*W][3C], out [images][H*W][C]; windows never cross images */
int rmem_window_attn_images(const void* qkv, const float* qkv_bias, const float* bias_mask_table, void* out, int images, int H, int W,
                            int C, int heads, int shift, void* stream);

/* y = a + b (bf16).  Replaces the `curr_v + curr_id_emb` adds of layers/transformer.py:279-285. */
int rmem_add16(const void* a, const void* b, void* y, long long n, void* stream);
/* n <= 8 such adds of equal length as one launch (the per-layer adds of one memory update are independent). */
int rmem_add16_grouped(int n, const void* const* a, const void* const* b, void* const* y, long long count, void* stream);

/* GroupNorm on NHWC bf16 with fused activation (0 none, 1 ReLU, 2 exact GELU).
 * Replaces: layers/basic.py:31-32 (GN(32)+GELU of the conv-FFN) and layers/basic.py:69-70 +
 * decoders/fpn.py:44-64 (GN(8)+ReLU of the FPN head). */
size_t rmem_groupnorm_workspace_bytes(int groups);
int rmem_groupnorm_nhwc(const void* x, int M, int C, int groups, const float* gamma, const float* beta,
                        float eps, int act, void* y, float* workspace, void* stream);

/* Same with an fp32 input: the final GroupNorm1D(512, 2 groups) over the concatenated residual streams of the DeAOT
 * stack (layers/transformer.py:755-758, 806-808; layers/basic.py:6-12). */
int rmem_groupnorm_f32_nhwc(const float* x, int M, int C, int groups, const float* gamma, const float* beta,
                            float eps, int act, void* y, float* workspace, void* stream);

/* Batched forms: x / y hold `images` maps back to back ([images][M][C]); statistics are per image.  workspace: images times
 * rmem_groupnorm_workspace_bytes(groups). */
int rmem_groupnorm_nhwc_images(const void* x, int images, int M, int C, int groups, const float* gamma, const float* beta,
                               float eps, int act, void* y, float* workspace, void* stream);
/* y[m][n] = bias[n] + sum_c w[n][c] * act(GroupNorm(x))[m][c], n < N <= 16, fp32 rows of ldy: the segmentation head's
 * `conv_out(relu(gn(x)))` (decoders/fpn.py:62-66) in one pass over x (the normalised 128-channel map is never written;
 * it is rounded to bf16 on chip exactly as rmem_groupnorm_nhwc would store it).  C must be 128; w is [N][128] bf16. */
int rmem_groupnorm_head_nhwc_images(const void* x, int images, int M, int C, int groups, const float* gamma, const float* beta,
                                    float eps, int act, const void* w, const float* bias, int N, float* y, int ldy,
                                    float* workspace, void* stream);
int rmem_gn_act_dwconv5x5_nhwc_images(const void* x, int images, int H, int W, int C, int groups, const float* gamma,
                                      const float* beta, float eps, int act, const float* w_t, void* y, float* workspace, void* stream);
int rmem_bilinear_nhwc_images(const void* x, void* y, int images, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);
/* rmem_gn_act_dwconv5x5_nhwc_images without its statistics launch: `stats` already holds, per image and group, the (sum, sum of
 * squares) of up to 64 row ranges -- fp32 [images][groups][64][2], unused entries zero -- written by the producer of x
 * (rmem_lstt_chain_b: gn_partial with gn_splits = 64, i.e. at most 2048 rows per image). */
int rmem_gn_act_dwconv5x5_prestats_nhwc_images(const void* x, int images, int H, int W, int C, int groups, const float* gamma,
                                               const float* beta, float eps, int act, const float* w_t, void* y, const float* stats,
                                               void* stream);

/* Depth-wise 5x5, pad 2, NHWC bf16; w_t is [25][C] fp32.  Replaces layers/basic.py:19-25, 33. */
int rmem_dwconv5x5_nhwc(const void* x, const float* w_t, void* y, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------ DeAOT gated propagation attention
 * Single head, d_att = 128, values DV wide (1024 in R50-DeAOTL):
 *   out[q, :] = ( softmax_k( (Q[q]+pe_cur) . (K[k]+pe_mem[slot(k)]) / sqrt(128) ) V[k, :] ) * U[q, :]
 * Replaces layers/attention.py:138-208 (GatedPropagation.forward through `outputs * U`; use_linear False) as called from
 * layers/transformer.py:1183-1184 (long-term attention over the restricted bank: the K + temporal-embedding
 * materialisation of 1141-1177 and the [V | ID_V] concatenation of 1179 happen by indexing; attn_mass is
 * record_attn_weight of 1185-1192) and from 1229 (self-attention, after the linear_QK / V / U GEMMs of attention.py:151-173).
 * The depth-wise 5x5 and the projection (attention.py:210-211) are rmem_dwconv5x5_nhwc / rmem_conv2d_nhwc calls.
 * chunks: the rmem_attn_chunk table (<= 64 rows, key_begin a multiple of 64) or NULL for ONE key frame of
 * keys_per_frame keys cut into nchunks ranges.  The gate U is given as two column ranges: u_a covers [0, usplit),
 * u_b covers [usplit, DV) or is NULL for all ones (layer 0, transformer.py:1117-1118).
 * out: bf16 [Lq][ldo]; attn_mass: fp32 [Lq][frames] or NULL. */
size_t rmem_gated_attn_workspace_bytes(int Lq, int DV, int frames, int keys_per_frame, int nchunks);
int rmem_gated_attn(const void* q, int ldq,                                        /* bf16 [Lq][ldq], 128 used */
                    const void* k_bank, long long k_slot_stride, int ldk,          /* bf16 rows of 128 */
                    const void* v_bank, long long v_slot_stride, int ldv,          /* bf16 rows of DV */
                    const rmem_attn_chunk* chunks, int nchunks, int frames, int keys_per_frame,
                    const float* pe_cur, const float* pe_mem,                      /* fp32 [128], [4][128] or NULL */
                    int Lq, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit,
                    void* out, int ldo, float* attn_mass,
                    const float* dw_w_t, int H, int W,   /* optional: out = dw_conv5x5(gated) (attention.py:210), weights [25][DV],
                                                            H * W == Lq; NULL: out = gated */
                    void* workspace, void* stream);
/* 15x15 local window flavour (layers/attention.py:281-349, use_linear False, one head): keys/values are the previous
 * frame's [H*W] tokens; a key contributes to a query iff |dy| <= 7 and |dx| <= 7 (the zero padding + 1e8 mask of
 * 299-303, 338); rel: fp32 [H*W][ldrel] = relative_emb_k(q) (attention.py:305, a rmem_conv2d_nhwc call with fp32 output),
 * column (dy+7)*15 + (dx+7).  Workspace: rmem_gated_attn_workspace_bytes(H*W, DV, 1, H*W, 8). */
int rmem_local_gated_attn(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel, int ldrel,
                          int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit,
                          void* out, int ldo, const float* dw_w_t, void* workspace, void* stream);

/* Both gated attentions for nclips independent clips of identical shape in ONE launch per kernel (clips of a group advance in
 * lockstep): q, the gates, out and (one-frame calls) k / v / rel are [clip][rows][ld] arrays, i.e. clip c sits rows * ld elements
 * further; the bank is addressed through GLOBAL slot indexes in the table, clip c's table rows are chunks[c * nchunks ...], its
 * mass attn_mass + c * Lq * frames; the workspace is nclips times rmem_gated_attn_workspace_bytes.  Results per clip are those
 * of the single-clip entry points (the split of the key stream into partial-sum slabs depends on the clip count: fp32 summation
 * order only). */
int rmem_gated_attn_clips(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank,
                          long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames, int keys_per_frame,
                          const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a, int ldua, const void* u_b, int ldub,
                          int usplit, void* out, int ldo, float* attn_mass, const float* dw_w_t, int H, int W, int nclips,
                          void* workspace, void* stream);
int rmem_local_gated_attn_clips(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel, int ldrel,
                                int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo,
                                const float* dw_w_t, int nclips, void* workspace, void* stream);
/* HIP-event timing of the k_gp_pv launches of rmem_gated_attn calls that carry a chunk table (bench.py's roofline leg) */
int rmem_gated_profile_start(void);
int rmem_gated_profile_stop(double* total_ms, double* total_flops, int* launches);
/* Memory-bank append for a group of clips: block c of src ([nclips][block_bytes], the new K or V entries of all clips) goes to
 * dst + slots_dev[c] * slot_bytes.  slots_dev is a device table, so one captured launch serves whatever slots the clips'
 * eviction policies have freed (layers/transformer.py:305-322 appends, 432-433 removes). */
int rmem_scatter_blocks(const void* src, void* dst, const int* slots_dev, int nclips, long long block_bytes, long long slot_bytes,
                        void* stream);
/* strided 2-D device copy (rows of row_bytes): the torch.cat / slice bookkeeping of transformer.py:840-872 */
int rmem_copy2d_async(void* dst, long long dst_pitch, const void* src, long long src_pitch, long long row_bytes, int rows, void* stream);

/* GroupNorm + activation + depth-wise 5x5 as two launches (statistics; normalise + activate + convolve through an LDS tile)
 * instead of three, bit-identical to rmem_groupnorm_nhwc followed by rmem_dwconv5x5_nhwc.  Replaces layers/basic.py:27-35
 * (GNActDWConv2d.forward).  C % 64 == 0, channels per group in {8, 16, 32, 64}. */
int rmem_gn_act_dwconv5x5_nhwc(const void* x, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps,
                               int act, const float* w_t, void* y, float* workspace, void* stream);

/* ------------------------------------------------------------------ layout / resampling */
/* fp32 [3][H][W] image -> bf16 [H][W][8] (channels 3..7 zero): input of encoders/resnet.py:179. */
int rmem_image_to_nhwc8(const float* img_chw, void* out, int H, int W, void* stream);
/* the `_images` forms of this section take `images` equally sized problems stored back to back (clip groups, encoder
 * look-ahead) as ONE launch; each image's result equals the single-image call. */
int rmem_image_to_nhwc8_images(const float* img_chw, void* out, int images, int H, int W, void* stream);
/* The same with the images named by a DEVICE table of `images` pointers (fp32 [3][H][W] each): the frames of several clips go into
 * one encoder batch from wherever the caller keeps them, without a staging copy (models/aot.py:116-134: the encoder's input). */
int rmem_image_ptrs_to_nhwc8(const float* const* img_ptrs, void* out, int images, int H, int W, void* stream);
/* ResNet stem without im2col traffic (encoders/resnet.py:131-135: conv1 7x7 stride 2 pad 3, bn1 folded, ReLU).
 * rmem_stem_padded_size: the frame layout the kernel reads -- NHWC with 4 channels (r, g, b, 0) inside a zero border: [images][Hp][Wp][4],
 *   pixel (y, x) at row y + 3, column x + 3; the caller zeroes the buffer ONCE, rmem_image_ptrs_to_nhwc4p writes only the interior.
 * rmem_stem7x7s2: y [images][Ho][Wo][64] = relu(conv + bias), Ho = (H - 1) / 2 + 1; w is [64][8][8][4] (ky, kx, c; zero where ky = 7,
 *   kx = 7 or c = 3), i.e. K = 256.  A persistent workgroup keeps the weights in registers and copies each 64-output window block
 *   (8 rows x 134 pixels) to LDS once; MFMA B fragments are read from it in place.  Same products as rmem_conv2d_nhwc on the 8-channel
 *   layout, summed in another order (fp32). */
int rmem_stem_padded_size(int H, int W, int* Hp, int* Wp);
int rmem_image_ptrs_to_nhwc4p(const float* const* img_ptrs, void* out_padded, int images, int H, int W, void* stream);
int rmem_stem7x7s2(const void* x_padded, int images, int H, int W, const void* w, const float* bias, void* y, void* stream);
/* The same followed by the 3x3 stride-2 pad-1 max-pool (encoders/resnet.py:136) in ONE pass: y_pooled [images][HP][WP][64], HP = (Ho - 1) / 2 + 1;
 * the half-resolution map is never written.  Bit-identical to rmem_stem7x7s2 + rmem_maxpool3x3s2_nhwc_images. */
int rmem_stem7x7s2_pool(const void* x_padded, int images, int H, int W, const void* w, const float* bias, void* y_pooled, void* stream);
/* 3x3 stride-1 pad-1 convolution with C input and C output channels (C = 64 or 128) + bias (+ ReLU), read in place from rows kept in
 * LDS with the weights in registers: the second conv of the ResNet layer-1 / layer-2 bottlenecks (encoders/resnet.py:52-56) and the
 * decoder's conv_4x (decoders/fpn.py:54-58).  x NHWC [images][H][W][C], w [C][3][3][C] (rmem_conv2d_nhwc's layout), y like x.
 * Bit-identical to rmem_conv2d_nhwc (same k order, same epilogue).  rmem_conv3x3_c64_direct = C 64 with ReLU. */
int rmem_conv3x3_direct(const void* x, int images, int H, int W, int C, const void* w, const float* bias, int relu, void* y, void* stream);
int rmem_conv3x3_c64_direct(const void* x, int images, int H, int W, const void* w, const float* bias, void* y, void* stream);
/* Frame ingest: decoded uint8 RGB [Hs][Ws][3] -> bicubic resize to the network size (OpenCV INTER_CUBIC semantics) ->
 * ImageNet normalise -> fp32 [3][Hd][Wd] (the engine API's input) and/or bf16 [Hd][Wd][8] (the encoder's input).
 * Replaces dataloaders/video_transforms.py:648-652 (cv2.resize) + 676-680 (normalise) on the host. */
int rmem_ingest_rgb8(const unsigned char* rgb_hwc, int Hs, int Ws, int Hd, int Wd, float* out_chw, void* out_nhwc8, void* stream);
/* ------------------------------------------------------------------ baseline JPEG decode (jpeg_host.cpp, jpeg.hip)
 * Compressed frames in, the exact uint8 RGB libjpeg-turbo (Pillow) produces out.  Supported: 8-bit baseline / extended Huffman,
 * one interleaved scan, grayscale or YCbCr at 4:4:4, 4:2:2 (h2v1) and 4:2:0 (h2v2), optional restart intervals, any size.
 * The host side (parse, pack) needs no GPU; the device side runs on the caller's stream with no host synchronisation. */
#define RMEM_JPEG_SUBSEQ_BITS 1024      /* one lane of the entropy decoder owns this many bits of a unit */

typedef struct rmem_jpeg_info {
  int width, height, components;
  int h_samp[3], v_samp[3], quant_id[3];   /* as written in SOF (components >= 1) */
  int restart_interval;                    /* MCUs per restart interval (DRI), 0 = none */
  int quant_mask;                          /* bit t set: quant[t] was defined by a DQT */
  unsigned short quant[4][64];             /* quantisation tables in natural (row-major) order */
  long long scan_begin, scan_end;          /* byte range of the entropy-coded segment in the file */
  long long packed_bound;                  /* upper bound of the bytes rmem_jpeg_pack appends for this file */
} rmem_jpeg_info;

/* Huffman decode table: a 9-bit lookup for short codes and the canonical-code slow path for lengths 10..16. */
typedef struct rmem_jpeg_huff {
  unsigned short lut[512];                 /* next 9 bits -> (code length << 8) | symbol; 0 = code longer than 9 bits */
  int maxcode[18];                         /* largest code of each length, -1 if none */
  int valoff[18];                          /* symbol index of a code of length l = code + valoff[l] */
  unsigned char vals[256];
} rmem_jpeg_huff;

/* Per-frame descriptor written by rmem_jpeg_pack (fixed size, copied to the device as an array).
 * A frame's chunk in the clip buffer is: (nunits + 1) x {uint32 bit offset, uint32 first subsequence} (the last entry closes the
 * list), zero padding to data_off, the entropy bytes without byte stuffing and RSTn markers, then >= 16 zero bytes.
 * A unit is a restart interval, or the whole scan without DRI; it starts on a byte boundary and is cut into
 * ceil(bits / RMEM_JPEG_SUBSEQ_BITS) subsequences. */
typedef struct rmem_jpeg_desc {
  long long offset;                        /* byte offset of the chunk in the clip buffer (16-byte aligned) */
  long long bytes;                         /* chunk length */
  int width, height, ncomp, hmax, vmax;
  int mcus_x, mcus_y, bpm;                 /* MCU grid and blocks per MCU (a one-component scan has 1x1-block MCUs) */
  int restart_mcus, nunits, nsub, total_blocks;
  int data_off, data_bits;                 /* entropy bytes: chunk offset and length in bits */
  int comp_h[3], comp_v[3];                /* sampling factors (1 for a one-component scan) */
  int comp_bw[3], comp_bh[3];              /* coefficient plane of a component in blocks (the MCU grid's, padded) */
  int comp_block0[3];                      /* first block of the component's plane in the [total_blocks][64] buffer */
  int comp_dw[3], comp_dh[3];              /* downsampled_width / height: ceil(width * h / hmax), ceil(height * v / vmax) */
  int mcu_comp[10], mcu_sub[10];           /* block b of an MCU: component, and index inside that component's h x v group */
  unsigned short quant[3][64];             /* per component, natural order */
  rmem_jpeg_huff dc[3], ac[3];             /* per component */
} rmem_jpeg_desc;

/* Sizes of a decode call, from rmem_jpeg_workspace_bytes; pass the struct to the device entry points unchanged except for
 * sync_rounds / flags. */
typedef struct rmem_jpeg_plan {
  int batch;                               /* frames per call at most */
  int max_width, max_height, max_sub, max_blocks, max_units;
  int sync_rounds;                         /* bounded cross-workgroup sync launches (default 8; 0 = none) */
  int flags;                               /* RMEM_JPEG_FORCE_FALLBACK: every unit goes to the sequential decoder (tests) */
  long long slot_bytes;                    /* workspace per frame */
  long long off_state, off_unit, off_dc, off_coef, off_plane, off_misc;   /* offsets inside a slot */
} rmem_jpeg_plan;
#define RMEM_JPEG_FORCE_FALLBACK 1
/* status word of a frame (0 = decoded) */
#define RMEM_JPEG_ST_COUNT   1                  /* a unit did not decode to its MCU count */
#define RMEM_JPEG_ST_CODE    2                  /* invalid Huffman code or coefficient index on the decode path */
#define RMEM_JPEG_ST_DESC    4                  /* descriptor outside the plan */

/* Headers only: 0, or non-zero with the reason in rmem_last_error_string() (progressive, arithmetic, 12-bit, multi-scan,
 * 4 components, unsupported sampling, truncated, ...).  No GPU needed. */
int rmem_jpeg_parse(const unsigned char* data, size_t n, rmem_jpeg_info* out);
/* Appends one frame's chunk to the caller's (pinned) buffer at the 16-byte aligned offset >= *used and advances *used;
 * fills *desc.  Fails if cap is too small (info.packed_bound bytes always suffice).  No GPU needed. */
int rmem_jpeg_pack(const unsigned char* data, size_t n, unsigned char* buf, size_t cap, size_t* used, rmem_jpeg_desc* desc);
/* Workspace for decoding up to `batch` frames at once of any of the ndesc host descriptors; fills *plan. */
size_t rmem_jpeg_workspace_bytes(const rmem_jpeg_desc* descs, int ndesc, int batch, rmem_jpeg_plan* plan);
/* Entropy decode of frames first .. first+n-1 of the device descriptor table: int16 coefficients [total_blocks][64] in natural
 * order with DC values (not differences) at workspace + i * plan->slot_bytes + plan->off_coef.  bits = clip buffer (device).
 * status[n] (device) receives the per-frame status word; stats (device, may be NULL) accumulates {sync launches that ran,
 * units sent to the sequential fallback}. */
int rmem_jpeg_entropy_decode(const unsigned char* bits, const rmem_jpeg_desc* descs, int first, int n, const rmem_jpeg_plan* plan,
                             void* workspace, int* status, int* stats, void* stream);
/* Dequantise + ISLOW IDCT + fancy upsampling + YCbCr->RGB of the coefficients left by rmem_jpeg_entropy_decode:
 * out[i] (device array of n device pointers) = uint8 [height][width][3]. */
int rmem_jpeg_coef_to_rgb(const rmem_jpeg_desc* descs, int first, int n, const rmem_jpeg_plan* plan, void* workspace,
                          unsigned char* const* out, void* stream);
/* Both of the above. */
int rmem_jpeg_decode_batch(const unsigned char* bits, const rmem_jpeg_desc* descs, int first, int n, const rmem_jpeg_plan* plan,
                           void* workspace, unsigned char* const* out, int* status, int* stats, void* stream);
/* 3x3 stride-2 pad-1 max-pool (encoders/resnet.py:105, 182). */
int rmem_maxpool3x3s2_nhwc(const void* x, void* y, int H, int W, int C, void* stream);
int rmem_maxpool3x3s2_nhwc_images(const void* x, void* y, int images, int H, int W, int C, void* stream);
/* bilinear resize, NHWC bf16 (decoders/fpn.py:49-52, 57-60). */
int rmem_bilinear_nhwc(const void* x, void* y, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);
/* logits fp32 NHWC [Hi][Wi][ldl]: ids > keep_max_id forced to -1e10, bilinear to (Ho, Wo); writes any of
 * NCHW fp32 logits, uint8 argmax labels, fp32 argmax labels (engines/aot_engine.py:450-463;
 * managers/evaluator.py:430-441). */
int rmem_logits_post(const float* logits_nhwc, int ldl, int num_classes, int keep_max_id, int Hi, int Wi,
                     int Ho, int Wo, int align_corners, float* out_nchw, unsigned char* label_u8,
                     float* label_f32, void* stream);
/* images > 1: labels only (out_nchw must be NULL) */
int rmem_logits_post_images(const float* logits_nhwc, int images, int ldl, int num_classes, int keep_max_id, int Hi, int Wi,
                            int Ho, int Wo, int align_corners, float* out_nchw, unsigned char* label_u8,
                            float* label_f32, void* stream);
/* Identity-bank embedding straight from a label map, without the one-hot tensor (models/aot.py:139-147 patch_wise_id_bank applied to
 * one_hot(mask), engines/aot_engine.py:208-232): label [images][Hs][Ws] (uint8, or fp32 with label_is_f32) is resized to the network
 * size H x W (nearest, as rmem_label_to_onehot16 does) into the INTERIOR of label_scratch_u8 [images][Hpd][Wpd] (rmem_label_id_embed_scratch_size:
 * a border of `pad` pixels all round and one more row below, which the caller fills with 255 ONCE and which is never written), then
 *   out[pos][0..255] = bias + sum over the KH x KW window of pos of w[:, ky, kx, label]      (stride, pad as the conv; labels >= num_classes: 0)
 * with w [256][KH][KW][16] (rmem_conv2d_nhwc's layout of the Cin-padded weight).  The one-hot MFMA operand is built in registers from
 * the label bytes.  Same products as rmem_label_to_onehot16 + rmem_conv2d_nhwc, summed in another order (fp32). */
int rmem_label_id_embed_scratch_size(int H, int W, int pad, int* Hpd, int* Wpd);
int rmem_label_id_embed(const void* label, int label_is_f32, int images, int Hs, int Ws, int H, int W, int KH, int KW, int stride, int pad,
                        int num_classes, const void* w, const float* bias, void* label_scratch_u8, void* out, void* stream);

/* label map (uint8 or fp32) -> nearest resize -> one-hot + ignore channel, bf16 [Hd][Wd][16]
 * (utils/image.py:69-74; engines/aot_engine.py:208-224; managers/evaluator.py:518-522). */
int rmem_label_to_onehot16(const void* label, int label_is_f32, int Hs, int Ws, int Hd, int Wd,
                           int num_classes, void* out, void* stream);
int rmem_label_to_onehot16_images(const void* label, int label_is_f32, int images, int Hs, int Ws, int Hd, int Wd,
                                  int num_classes, void* out, void* stream);
/* scores[t] = sum_q mass[q][t] * (1 - softmax(bilinear_ac(logits -> He x We))[0])
 * (engines/aot_engine.py:355-362 + layers/transformer.py:341-351, the device half of the eviction policy).
 * `scores` must hold 32 + 64 * 32 floats: the first T are the result, the rest is reduction scratch. */
int rmem_evict_scores(const float* logits_nhwc, int ldl, int num_classes, int keep_max_id, int Hi, int Wi,
                      int He, int We, const float* attn_mass, int T, float* scores, void* stream);

/* Asynchronous copy on `stream` (device<->device, or pinned host<->device): frame ingest into the fixed input
 * buffer, bank append of curr_K (layers/transformer.py:319), chunk-table upload, eviction-score readback.
 * Capturable into a hipGraph (memcpy node). */
int rmem_copy_async(void* dst, const void* src, size_t bytes, void* stream);

/* Clips with more than 10 objects run one engine per 10 objects (engines/aot_engine.py:604-673).
 * rmem_split_label: engine e's label map = ids start_id..end_id renumbered from 1, everything else 0 (separate_mask, 610-628).
 * rmem_soft_logit_aggregate: soft_logit_aggregation (650-673) -- per engine softmax over its num_classes channels, background =
 * product of the engines' background probabilities, then the engines' objs_per_engine foreground channels concatenated;
 * clamp to [1e-5, 1 - 1e-5] and logit.  logits_nchw: HOST array of n_engines device pointers to [num_classes][H][W] fp32;
 * out: [1 + n_engines * objs_per_engine][H][W] fp32. */
int rmem_split_label(const float* label, int start_id, int end_id, float* out, long long n, void* stream);
int rmem_soft_logit_aggregate(const float* const* logits_nchw, int n_engines, int num_classes, int objs_per_engine, int H, int W,
                              float* out_nchw, void* stream);

/* fp32 planes [planes][Hs][Ws] -> optionally mirrored along W (utils/image.py:109-113 flip_tensor(dim 3)) -> nearest-neighbour resize
 * (F.interpolate(mode='nearest') index rule: src = floor(dst * in / out)) to [planes][Hd][Wd]: the frames and label maps the
 * evaluator hands to its flipped-augmentation engines, in the reference's order flip, then resize (managers/evaluator.py:342-355,
 * 490-522). */
int rmem_resize_nearest_flip_f32(const float* src, int planes, int Hs, int Ws, float* dst, int Hd, int Wd, int flip_w, void* stream);

/* Test-time-augmentation merge: softmax of each augmentation's NCHW logits (read horizontally flipped where flips[a] != 0),
 * mean over the <= 8 augmentations (scales x flips), argmax; writes any of uint8 labels, fp32 labels, NCHW mean probabilities.
 * logits_nchw / flips are HOST arrays of n_aug entries.  Replaces managers/evaluator.py:427-441 (flip / multi-scale TTA). */
int rmem_tta_merge(const float* const* logits_nchw, const int* flips, int n_aug, int num_classes, int H, int W,
                   unsigned char* label_u8, float* label_f32, float* prob_nchw, void* stream);

/* Flip test-time augmentation inside a clip group, fused: logits fp32 [rows][Hi * Wi][16], rows = 2P, row p a clip and row P + p its
 * horizontally mirrored twin.  Per output pixel (y, x) of pair p: row p blended at (y, x) and row P + p at (y, Wo - 1 - x) (bilinear,
 * ids > keep_max_id forced to -1e10, as rmem_logits_post_images), softmax of each over the num_classes channels, mean, argmax (first
 * maximum) -- what rmem_logits_post + rmem_tta_merge compute for the pair, without the full-size fp32 maps.  label_u8 [rows][Ho][Wo]:
 * label_u8[p][y][x] = the merged label, label_u8[P + p][y][Wo - 1 - x] = the same value (the twin's row holds the mirror, what its
 * memory update takes).  Refused (non-zero, nothing launched): odd rows, num_classes > 16, keep_max_id >= num_classes, null
 * pointers, logits not 16-byte aligned. */
int rmem_logits_post_flip_pairs(const float* logits_nhwc16, int rows, int num_classes, int keep_max_id, int Hi, int Wi, int Ho, int Wo,
                                int align_corners, unsigned char* label_u8, void* stream);

/* Multi-scale (x flip) testing inside clip groups, fused: every scale runs a clip group of its own at its own network size, and the
 * groups meet here once per frame.  members / Hi / Wi / flips are HOST arrays of n_aug (1..8) entries in the evaluator's order (scale
 * outer, flip inner): member a is a device pointer to fp32 logits [clips][Hi[a] * Wi[a]][16], 16-byte aligned; the mirrored twins of
 * a flip group are its logits buffer advanced by `clips` rows.  Per output pixel (y, x) of clip p, for a = 0 .. n_aug - 1 in order:
 * member a blended at (y, x), or at (y, Wo - 1 - x) where flips[a] (bilinear, ids > keep_max_id forced to -1e10, as
 * rmem_logits_post_images), softmax over the num_classes channels, summed; * 1 / n_aug, argmax (first maximum) -- what rmem_logits_post
 * per member + rmem_tta_merge compute, without the full-size fp32 maps.  label_u8 [clips][Ho][Wo] gets the merged label; twin_u8
 * [clips][Ho][Wo], if given, the same value at (y, Wo - 1 - x) (row `clips` of a [2 * clips][Ho][Wo] buffer: what the mirrored
 * engines' memory updates take).  n_aug = 2, equal sizes, flips (0, 1) gives rmem_logits_post_flip_pairs bit for bit.  Refused
 * (non-zero, nothing launched): n_aug outside 1..8, num_classes > 16, keep_max_id >= num_classes, clips < 1, non-positive sizes, a
 * null member or label_u8, a member not 16-byte aligned. */
int rmem_logits_post_ms_merge(const float* const* members, const int* Hi, const int* Wi, const int* flips, int n_aug, int clips,
                              int num_classes, int keep_max_id, int Ho, int Wo, int align_corners, unsigned char* label_u8,
                              unsigned char* twin_u8, void* stream);

/* Label routing of a RAGGED clip group (clip_runner.RaggedGroupSlot): the rows of a group run clips of different lengths, so after
 * the decoder every row delivers its label map to another address, and a row may take a new object's overlay, continue from fed
 * labels, mirror into its flip twin or be idle.  One launch, driven by a device table of `rows` entries; rows_u8 [rows][Ho * Wo]
 * (the group's label rows, what the memory update reads) is rewritten in place.  Per row of mode 0, pred = the row on entry:
 *   x = feed ? feed : pred;   overlay: x = overlay > 0 ? overlay : x;   dst (if set) := feed ? pred : x;   row := x;
 *   twin >= 0: rows_u8[twin] := x mirrored along W (the twin's own entry has mode 2: its row is written by its primary only).
 * mode 1 (idle): row := 0, nothing is delivered, twin / feed / overlay / dst are not looked at.  dst, overlay and feed name Ho * Wo
 * bytes each and may not overlap rows_u8.  Rows start at any byte, so 4-byte accesses are used where every address of a row allows
 * them and single bytes otherwise.  Replaces the per-row torch.where / flip / copy of clip_runner.GroupSlot.step (evaluator.py:
 * 484-497).  Refused (non-zero, nothing launched): rows outside 1..65535, null rows_u8 / routes, non-positive Ho / Wo. */
typedef struct {
  unsigned char* dst;           /* this row's label map of this step goes here (Ho * Wo bytes), or NULL */
  const unsigned char* overlay; /* new object's map: its non-zero pixels replace the row's, or NULL */
  const unsigned char* feed;    /* labels to continue from instead of the prediction, or NULL */
  int twin;                     /* row that receives this row's final map mirrored along W, or -1 */
  int mode;                     /* 0 live, 1 idle (row := 0, nothing delivered), 2 written by its primary (skip) */
} rmem_label_route;
int rmem_route_labels(unsigned char* rows_u8, int rows, int Ho, int Wo, const rmem_label_route* routes, void* stream);

/* Label census of an annotation (or prediction) stack: which ids a frame holds, how large they are and where -- what the clip
 * protocol (protocol.py: ids, first appearance, squeeze_idx, new-object overlays) and box consumers are built from, and what
 * dataloaders/eval_datasets.py (VOSTest, np.unique per annotated frame) computes on the host.
 * Census of uint8 label maps.  labels [n][H][W], contiguous.  out int32 [n][256][5]: for frame f and label value v
 * area, xmin, ymin, xmax, ymax of the pixels equal to v; a value absent from the frame reads (0, W, H, -1, -1).
 * Every entry of out is written by the call: the caller initialises nothing, prior contents do not matter.
 * labels may start at any byte (16-byte loads are used between an unaligned head and tail).  Integer atomics only: the result
 * does not depend on the order of arrival and is bit-reproducible.  Refused (non-zero, nothing launched): null labels / out, n
 * outside 1..65535, non-positive H / W, H * W above 2^26. */
int rmem_label_census(const unsigned char* labels, int n, int H, int W, int* out, void* stream);

/* dst[f][p] = luts[(lut_per_frame ? f : 0) * 256 + src[f][p]] for p < pixels.  luts: device uint8 [n or 1][256].
 * dst == src (in place) is allowed; partial overlap is not looked for.  src and dst may start at any byte.  The squeeze of sparse
 * palette ids, and with one table per frame the first-frame label and the new-object overlays of a whole clip in one launch.
 * Refused (non-zero, nothing launched): null src / dst / luts, n outside 1..65535, pixels outside 1..2^26. */
int rmem_label_remap(const unsigned char* src, unsigned char* dst, int n, long long pixels, const unsigned char* luts,
                     int lut_per_frame, void* stream);

/* Pair census of two uint8 label stacks: per frame the joint histogram of (value in a, value in b) -- the table behind the IoU of
 * every predicted with every annotated object (pairs.py: pair_iou, track_iou, assign; evaluator.relabel_to_match,
 * identity_report), where rmem_mask_iou_counts / rmem_clip_score_counts compare id i with id i only.
 * a, b [n][H][W], contiguous; each may start at any byte, independently of the other.  out int32 [n][num_a + 2][num_b + 2]:
 * out[f][i][j] = number of pixels of frame f with min(a, num_a + 1) == i and min(b, num_b + 1) == j.  The last row and the last
 * column are "other": every value above num_a / num_b falls there (a void label of 255 when num_b < 255); no pixel is dropped, so
 * every frame's table sums to H * W.  Every entry of out is written by the call (zeroed on the stream first): prior contents do not
 * matter.  No state between calls, no workspace, no host sync.  Tables of up to rmem_label_pair_census_lds_bins() bins are kept in
 * LDS per workgroup and flushed with global integer adds, larger ones are added to in global memory directly.  Integer atomics
 * only: the result does not depend on the order of arrival and is bit-reproducible.  Refused (non-zero, nothing launched): null a /
 * b / out, n outside 1..65535, non-positive H / W, H * W above 2^26 (which keeps every count inside int32), num_a or num_b
 * outside 1..255. */
int rmem_label_pair_census(const unsigned char* a, const unsigned char* b, int n, int H, int W, int num_a, int num_b, int* out,
                           void* stream);
int rmem_label_pair_census_lds_bins(void);   /* host only */

/* Connected components of uint8 label stacks, their statistics and the clean-up rule built on them (components.py: fill small
 * holes, drop small specks, keep the largest piece of every object) -- the census above knows label VALUES, this knows their PIECES.
 * labels: uint8 [n][H][W], contiguous, device, may start at any byte.  Every value 0..255 is treated alike (0 too: its components
 * are the holes and the background; a void label of 255 is an ordinary value); frames are independent.  Two pixels of a frame are
 * in one component when they hold one value and a path of pixels of that value links them under `connectivity`: 4 = edge
 * neighbours, 8 = corner neighbours too.
 *   roots  int32 [n][H][W]: the flat index y * W + x of the component's FIRST PIXEL IN RASTER ORDER -- independent of scheduling,
 *          comparable bit for bit.  rmem_label_components writes every entry (prior contents do not matter).
 *   status int32 [1]: OR-ed into, never cleared (the caller zeroes it).  Every loop over parents is bounded (find: H * W steps,
 *          union: H * W + 64 rounds); bit 0 = a union, bit 1 = a find ran into its bound.  A set bit is a bug, not a condition.
 *   stats  int32 [n][H * W][4]: at a root's flat index (area, nb_min, nb_max, border), anywhere else (0, 256, -1, 0).  nb_min /
 *          nb_max: the smallest / largest value among the in-frame pixels adjacent (same connectivity) to a pixel of the
 *          component that hold another value; (256, -1) when the component is the whole frame.  border: 1 if a pixel of the
 *          component lies in row 0, row H - 1, column 0 or column W - 1.
 *   table  int32 [n][256][3]: per value (number of components, area of the largest, root of the largest -- the smallest root on
 *          equal areas); (0, 0, -1) for an absent value.
 * rmem_label_component_stats writes every entry of stats and table from labels and the roots of rmem_label_components with the
 * same connectivity.  rmem_label_clean is one pass, every decision taken from the components of src: a pixel of value v whose
 * component has (area, nb_min, nb_max, border) becomes
 *   v == 0, area <= max_hole_area, border == 0 and nb_min == nb_max: nb_min (a hole wholly inside one object);
 *   v != 0 and (area <= max_sprinkle_area, or keep_largest and the component's root is not table[f][v][2]): nb_min where
 *          nb_min == nb_max (a speck wholly inside one object, or on the background), else 0;
 *   and stays v otherwise.  Areas of 0 and keep_largest = 0 are the identity.  dst == src (in place) is allowed; partial overlap
 * is not looked for; src and dst may start at any byte.
 * The tile kernel works on tiles of th x tw pixels (rmem_label_components_tile); rmem_label_components_workspace_bytes is the bytes
 * of roots, stats and table for n frames (0 for refused geometry).  No state between calls, no host sync, integer atomics only:
 * bit-reproducible.  Refused (non-zero, nothing launched): a null pointer, n outside 1..65535, non-positive H / W, H * W above
 * 2^26, a connectivity other than 4 or 8, a negative area. */
int rmem_label_components_tile(int* th, int* tw);   /* host only */
long long rmem_label_components_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_components(const unsigned char* labels, int n, int H, int W, int connectivity, int* roots, int* status, void* stream);
int rmem_label_component_stats(const unsigned char* labels, const int* roots, int n, int H, int W, int connectivity, int* stats,
                               int* table, void* stream);
int rmem_label_clean(const unsigned char* src, unsigned char* dst, const int* roots, const int* stats, const int* table, int n, int H,
                     int W, int max_hole_area, int max_sprinkle_area, int keep_largest, void* stream);

/* Label pieces through time (tubes.py: label_tubes, lineage, piece_events, tube_table, clean_tubes) -- the components above know
 * the pieces of one frame, this knows which piece of frame f goes on in which piece of frame f + 1.
 * labels: uint8 [n][H][W], contiguous, device, may start at any byte; every value 0..255 is treated alike.  roots / stats: what
 * rmem_label_components / rmem_label_component_stats wrote for the WHOLE stack (their connectivity is the pieces').  Two pieces of
 * one value on consecutive frames are linked when a pixel (y, x) of the one and a pixel (y', x') of the other satisfy
 * (y', x') == (y, x) under temporal = 1, |y' - y| <= 1 and |x' - x| <= 1 under temporal = 9.  A tube is a connected set of pieces
 * under links: what scipy.ndimage.label gives for labels == v under the 3-D structure whose centre plane is the pieces'
 * connectivity and whose two outer planes hold the centre voxel (1) or the full 3 x 3 (9).  A tube is contiguous in time.
 * A voxel's global index is g = f * H * W + y * W + x; tubes cross any boundary a pass would draw, so every entry point takes the
 * stack whole: n in 1..65535, H * W <= 2^26, n * H * W <= 2^31 - 1.
 *   tubes  int32 [n][H][W]: the global index of the tube's FIRST VOXEL in frame-major raster order.  rmem_label_tubes writes every
 *          entry (three launches: parents from roots, links united with atomicMin in which the smaller index wins, flatten).
 *   status int32 [1]: OR-ed into, never cleared; bit 0 = a union, bit 1 = a find ran into its bound (n * H * W steps).  A bug, not
 *          a condition.
 *   links  int32 [n][H * W][4]: at a piece's root (prev_min, prev_max, next_min, next_max), the smallest and largest root among
 *          the linked pieces on frame f - 1 and on frame f + 1, (H * W, -1) where there is none; (H * W, -1, H * W, -1) anywhere
 *          else.  Equal min and max: exactly one neighbour in time.  rmem_label_tube_lineage writes every entry.
 *   events int32 [n][256][4]: per frame f and value v the number of pieces of v on f that are born (f >= 1, no predecessor), ended
 *          (f <= n - 2, no successor), splitting (several successors: next_max >= 0 and next_min != next_max) and merging (several
 *          predecessors).  rmem_label_tube_events writes every entry from the links of the same stack.
 *   rank   int32 [n][H][W]: at a tube's first voxel its position among all tubes in ascending id, -1 elsewhere; total int32 [1]:
 *          the number of tubes.  rmem_label_tube_index writes every entry of both (count, scan, write; the counts of the chunks
 *          pass through rank itself).
 *   table  int32 [rows][10]: row rank = (first = the tube id, value, voxels, pieces, f_first, f_last, nb_min, nb_max, border,
 *          peak_area): nb_min / nb_max the extrema of its pieces' nb_min / nb_max, (256, -1) if no piece has a neighbour; border 1
 *          if a piece touches its frame's edge; peak_area its largest piece.  rmem_label_tube_table writes every row below
 *          min(rows, total) completely and nothing else: a tube whose rank is >= rows is left out, rows = 0 launches nothing.
 * rmem_label_tube_clean is one pass, every decision from the pieces and tubes of src; table must hold every tube (rows >= total).
 * With life = f_last - f_first + 1 and closed = f_first >= 1 and f_last <= n - 2 (frame 0 is the given annotation; a tube alive on
 * the last frame has a life nobody has seen the end of) a voxel of value v becomes
 *   v != 0, closed, life < min_frames: its PIECE's nb_min where the piece's nb_min == nb_max, else 0 (rmem_label_clean's rule);
 *   v == 0, closed, life <= max_hole_frames, the tube's border == 0 and nb_min == nb_max: the tube's nb_min;
 *   and stays v otherwise.  min_frames <= 1 with max_hole_frames = 0 is the identity.  dst == src is allowed; both may start at
 * any byte.  rmem_label_tubes_workspace_bytes: the bytes of roots, stats, tubes and rank for the whole stack (28 per voxel), 0 for
 * refused geometry.  No state between calls, no host sync, everything on the caller's stream, integer atomics only:
 * bit-reproducible.  Refused (non-zero, nothing launched): a null pointer, n outside 1..65535, non-positive H / W, H * W above
 * 2^26, n * H * W above 2^31 - 1, a temporal other than 1 or 9, negative rows, min_frames or max_hole_frames. */
long long rmem_label_tubes_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_tubes(const unsigned char* labels, const int* roots, int n, int H, int W, int temporal, int* tubes, int* status,
                     void* stream);
int rmem_label_tube_lineage(const unsigned char* labels, const int* roots, int n, int H, int W, int temporal, int* links, void* stream);
int rmem_label_tube_events(const unsigned char* labels, const int* roots, const int* links, int n, int H, int W, int* events,
                           void* stream);
int rmem_label_tube_index(const int* tubes, int n, int H, int W, int* rank, int* total, void* stream);
int rmem_label_tube_table(const unsigned char* labels, const int* roots, const int* stats, const int* tubes, const int* rank, int n,
                          int H, int W, int rows, int* table, void* stream);
int rmem_label_tube_clean(const unsigned char* src, unsigned char* dst, const int* roots, const int* stats, const int* tubes,
                          const int* rank, const int* table, int n, int H, int W, int min_frames, int max_hole_frames, void* stream);

/* Exact Euclidean distance transform of uint8 label stacks and the peaks of a distance map (distance.py: label_edt, peaks,
 * hausdorff2, hausdorff; evaluator.surface_distance, next_clicks).  Squared distances between pixel centres as int32; integers
 * only, no float anywhere.  labels: uint8 [n][H][W], contiguous, device, may start at any byte; frames are independent; every
 * value 0..255 is treated alike (a void label of 255 is an ordinary value).
 *   value = -1  "other": dist2[f][y][x] = min |p - q|^2 over the pixels q of frame f with labels[q] != labels[p] -- the interior
 *               depth of every object, and for the background the distance to the nearest object.  border = 1: the outside of the
 *               frame counts as another value, min(y + 1, H - y, x + 1, W - x)^2 joins the minimum (what padding the frame with
 *               one ring of a value it does not hold does); border = 0: the outside counts as nothing.
 *   value 0..255 "to value": dist2 = min |p - q|^2 over q with labels[q] == value, 0 on the pixels of value.  border must be 0.
 * Where no q exists (a frame of one value without border; value absent from the frame) dist2 = 2^31 - 1.  H and W are at most
 * 16384, so every real distance is below 2^30.  rmem_label_edt writes every entry of dist2; prior contents of dist2 and of the
 * workspace do not matter.  workspace: rmem_label_edt_workspace_bytes(n, H, W) bytes (0 for refused geometry), 4-byte aligned:
 * the vertical distances of the column pass, 16 bits per pixel.  Two launches; the scan of the row pass is bounded by the root
 * of the result, and a frame without any site is filled without a scan.
 * rmem_label_edt_peaks: table int32 [n][256][2], table[f][v] = (the largest dist2 among the pixels of frame f with keys == v,
 * the flat index y * W + x of the FIRST such pixel in raster order that attains it), (-1, -1) for a value no pixel holds.  keys:
 * any uint8 stack [n][H][W] (the labels themselves, or the other stack of a pair), may start at any byte.  dist2 must not be
 * negative (rmem_label_edt writes none).  Every entry of table is written.  workspace: rmem_label_edt_peaks_workspace_bytes(n)
 * bytes (0 for n outside 1..65535), 8-byte aligned: one 64-bit key per frame and value.  Three launches.
 * No state between calls, no host sync, integer atomics only: both are bit-reproducible and independent of scheduling.  Refused
 * (non-zero, nothing launched): a null pointer, n outside 1..65535, non-positive H / W, H * W above 2^26, (rmem_label_edt) H or
 * W above 16384, value outside -1..255, border other than 0 / 1 or 1 with a value, a workspace too small or misaligned. */
long long rmem_label_edt_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_edt(const unsigned char* labels, int n, int H, int W, int value, int border, int* dist2, void* workspace,
                   long long workspace_bytes, void* stream);
long long rmem_label_edt_peaks_workspace_bytes(int n);   /* host only */
int rmem_label_edt_peaks(const int* dist2, const unsigned char* keys, int n, int H, int W, int* table, void* workspace,
                         long long workspace_bytes, void* stream);

/* Nearest-site feature transform of uint8 label stacks: which pixel the nearest site is, and the label there (distance.py:
 * nearest, grow; evaluator.expand_masks, fill_void, labels_from_seeds).  Integers only, no atomics: bit-reproducible and
 * independent of scheduling.  labels: uint8 [n][H][W], contiguous, device, may start at any byte; frames are independent.
 * site_bits, fill_bits: HOST arrays of 256 bits read during the call, bit (v & 31) of word v >> 5 = value v is in the set;
 * fill_bits NULL: every value.  A pixel is a SITE if its value is in site_bits; an empty set is legal (nothing has a site).
 * max_d2: -1 (no limit) or 0..2^30: a site farther than max_d2 (squared) does not count, d2 == max_d2 still does.
 * Per pixel p of frame f, each output int32 / uint8 [n][H][W] and each may be NULL (not all three):
 *   index[p]  the flat index y * W + x, within the frame, of the site nearest to p by squared Euclidean distance between pixel
 *             centres; AMONG EQUALLY NEAR SITES THE ONE WITH THE SMALLEST FLAT INDEX (the first in raster order); -1 where the
 *             frame holds no site within the limit.  A site maps to itself.
 *   dist2[p]  that squared distance, 2^31 - 1 where index is -1.
 *   taken[p]  labels[f][index[p]] if labels[p] is in fill_bits and index[p] >= 0, else labels[p].  taken must not overlap labels.
 * Every entry of every non-NULL output is written; prior contents of the outputs and of the workspace do not matter.  workspace:
 * rmem_label_nearest_workspace_bytes(n, H, W) bytes (0 for refused geometry), 4-byte aligned: the signed vertical offset to the
 * nearest site of every pixel's own column, 16 bits per pixel.  Two launches, no host sync, no state between calls: a column pass
 * in which the site above wins a tie against the site below, and a row pass that takes the minimum of (d2, index) over the
 * columns; its scan is bounded by the root of the result or of max_d2.  With index and dist2 NULL, pixels outside fill_bits are
 * copied without a scan.  Refused (non-zero, nothing launched): null labels, site_bits or workspace, all three outputs NULL,
 * taken == labels, n outside 1..65535, non-positive H / W, H * W above 2^26, H or W above 16384, max_d2 outside -1..2^30, a
 * workspace too small or misaligned. */
long long rmem_label_nearest_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_nearest(const unsigned char* labels, int n, int H, int W, const unsigned int site_bits[8],
                       const unsigned int fill_bits[8], int max_d2, int* index, int* dist2, unsigned char* taken, void* workspace,
                       long long workspace_bytes, void* stream);

/* Geodesic nearest-site transform of uint8 label stacks over uint8 frames: rmem_label_nearest's image-aware twin, the same sites
 * and the same three outputs under another metric (distance.py: geodesic_nearest, geodesic_grow; evaluator.
 * labels_from_seeds_geodesic, fill_void_geodesic, snap_masks).  Integers only, no float on the device: bit-reproducible and
 * independent of scheduling.
 * labels: uint8 [n][H][W]; image: uint8 [n][H][W][C], C = channels = 1 or 3, interleaved (the layout rmem_overlay_rgb8 takes);
 * both contiguous, device, may start at any byte, only read; frames are independent.  site_bits, fill_bits: HOST arrays of 256
 * bits as rmem_label_nearest takes them (fill_bits NULL: every value); an empty site set is legal.  spatial in 1..64, colour in
 * 0..64, max_cost -1 (no limit) or 0..2^30.  H and W at most 16384, H * W at most 2^26, n in 1..65535.
 * THE GRAPH: the 8-connected pixel grid of a frame; the edge between neighbours p and q costs
 *   w(p, q) = spatial * s + colour * sum over the channels c of |I_c(p) - I_c(q)|,   s = 5 for an axial step, 7 for a diagonal one
 * (the 5-7 chamfer; colour = 0 is the plain chamfer distance).  An edge costs at most 64 * 7 + 64 * 765 = 49408; the straight
 * chamfer path bounds every real cost by 16383 * 49408 < 2^30.
 * key(p) = the lexicographic minimum over the frame's sites s of (the cost of the cheapest path s -> p, the flat index of s); a
 * site's cost to itself is 0, so a site maps to itself.  Per pixel p of frame f, each output [n][H][W], each may be NULL (not all):
 *   index[p] (int32)  the flat index y * W + x of that site; -1 where no site is within max_cost (a cost == max_cost still counts).
 *   cost[p]  (int32)  its cost, 2^31 - 1 where index is -1.
 *   taken[p] (uint8)  labels[f][index[p]] if labels[p] is in fill_bits and index[p] >= 0, else labels[p].  Must not overlap labels.
 * The answer is unique: relaxing (cost, index) with the lexicographic minimum over the eight neighbours is a monotone system whose
 * fixed point, reached from "no key anywhere but (0, own index) on the sites", is key; it does not depend on the order of
 * relaxation, the tile or the number of rounds.  A candidate above max_cost is dropped where it arises (a prefix of a cheapest
 * path is no dearer than the path).
 * Three calls on one workspace of rmem_label_geodesic_workspace_bytes(n, H, W) bytes (0 for refused geometry), 16-byte aligned:
 * two planes of 64-bit keys (cost << 32 | index; 2^31 - 1 and all ones: no key) and two sets of one byte per tile:
 *   begin   writes plane 0 from labels and site_bits.  One launch.
 *   rounds  runs the rounds first_round .. first_round + count - 1, one launch each; round r reads plane r & 1 and writes the other.
 *           One workgroup per tile of th x tw pixels (rmem_label_geodesic_tile) and frame relaxes the tile inside LDS to the fixed
 *           point for its one-pixel halo, or for a bounded number of passes, and writes one byte: its core changed.  changed int32
 *           [n]: the number of tiles of frame f whose core changed in the call's LAST round (zeroed by the call, one integer atomic
 *           per such tile).  All zero: plane (first_round + count) & 1 holds key.  A tile whose own byte and whose eight neighbours'
 *           bytes of the round before are all 0 leaves at once, from round 1 on (RMEM_GEODESIC_SKIP=0 in the environment: never,
 *           for A/B runs).  The caller continues with first_round + count, with the same image, weights and limit, until changed
 *           is all zero: a call that reports a change lowered a key, and keys are bounded below.
 *   finish  unpacks plane rounds & 1 (rounds: how many rounds have run) into the outputs, applying fill_bits and max_cost.  One
 *           launch.  Before the fixed point the outputs are upper bounds of no further meaning.
 * Every entry of every non-NULL output is written; prior contents of outputs and workspace do not matter at begin.  No host
 * sync, no kernel waits for another workgroup.  Refused (non-zero, nothing launched): null labels (begin, finish), image or
 * changed (rounds), site_bits (begin) or workspace; all three outputs NULL; taken == labels; channels other than 1 or 3; spatial,
 * colour or max_cost out of range; n outside 1..65535, non-positive H / W, H * W above 2^26, H or W above 16384; negative
 * first_round or rounds, count below 1, first_round + count beyond 31 bits; a workspace too small or misaligned. */
int rmem_label_geodesic_tile(int* th, int* tw);   /* host only */
long long rmem_label_geodesic_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_geodesic_begin(const unsigned char* labels, int n, int H, int W, const unsigned int site_bits[8], void* workspace,
                              long long workspace_bytes, void* stream);
int rmem_label_geodesic_rounds(const unsigned char* image, int channels, int n, int H, int W, int spatial, int colour, int max_cost,
                               int first_round, int count, int* changed, void* workspace, long long workspace_bytes, void* stream);
int rmem_label_geodesic_finish(const unsigned char* labels, int n, int H, int W, const unsigned int fill_bits[8], int max_cost, int rounds,
                               int* index, int* cost, unsigned char* taken, const void* workspace, long long workspace_bytes,
                               void* stream);

/* Shape census of uint8 label stacks: raw moments, row extents and convex hulls (shapes.py: label_moments, row_extents,
 * convex_hulls, region_props; evaluator.object_shapes, object_centroids, rotated_boxes).  Integers only, integer atomics only:
 * bit-reproducible.  labels: uint8 [n][H][W], contiguous, device, may start at any byte and is only read.  x and y are a pixel's
 * column and row index.  H and W at most 16384 (and H * W at most 2^26): every sum stays below 2^55.
 * rmem_label_moments: one pass over the labels by image rows, two outputs, either may be NULL (not both).
 *   moments int64 [n][256][6] = (m00, m10, m01, m20, m11, m02) = (count, sum x, sum y, sum x^2, sum x y, sum y^2) of the pixels of
 *     frame f equal to value v; zeros for an absent value.  The call zeroes the table itself.
 *   extents int32 [n][num][H][2] = (xmin, xmax) of value v = 1..num (entry v - 1) on row y, (W, -1) on a row without it.  Values
 *     above num are counted in the moments and appear in no extent.  num is read only with extents.
 *   Every entry of both is written; prior contents do not matter.
 * The hull is that of the pixel SQUARES, in pixel-corner coordinates (rmem_label_polygons' system): corner level l, 0..H, lies
 * between rows l - 1 and l; its candidates are L[l] = min(xmin[l-1], xmin[l]) and R[l] = max(xmax[l-1], xmax[l]) + 1 over the rows
 * that hold the value.  The hull is the convex minorant of L and the concave majorant of R over the levels plus the top and the
 * bottom edge: at most 2 (h + 1) vertices for an object h rows high.
 * rmem_label_hull_count: extents as above for n frames; flags uint8 [n][num][H + 1]: bit 0 = level l is a vertex of the left chain,
 *   bit 1 = of the right chain; counts int32 [n * num]: the object's number of hull vertices, 0 for an absent one (else >= 4).
 *   Every entry of both is written.  One wave per object, one serial stack walk per chain (O(h)); turns are int32 cross products
 *   below 2^29; 4 H bytes of LDS.
 * rmem_label_hull_offsets: counts int32 [objects + 1]: the first `objects` entries become their exclusive prefix sums in place,
 *   the last one the total V.  One workgroup.
 * rmem_label_hull_write: extents and flags of n frames as rmem_label_hull_count left them, offsets int32 [n * num + 1] their part
 *   of the scanned counts; verts int32 [capacity][2] = (x, y) corners, object o's ring at verts[offsets[o] .. offsets[o + 1]):
 *   strictly convex vertices only, starting at the vertex with the smallest (y, x), the object on the right of the direction of
 *   travel with y down (east along the top edge first: rmem_label_polygons' outer rings, a positive shoelace sum).  A ring that
 *   would not fit `capacity` is not written.
 * Refused (non-zero, nothing launched): null pointers, n outside 1..65535, H or W outside 1..16384, H * W above 2^26, num outside
 * 1..255 (where it is read), objects outside 1..65535 * 255, capacity outside 1..2^31-1. */
int rmem_label_moments(const unsigned char* labels, int n, int H, int W, int num, long long* moments, int* extents, void* stream);
int rmem_label_hull_count(const int* extents, int n, int H, int W, int num, unsigned char* flags, int* counts, void* stream);
int rmem_label_hull_offsets(int* counts, int objects, void* stream);
int rmem_label_hull_write(const int* extents, const unsigned char* flags, int n, int H, int W, int num, const int* offsets, int* verts,
                          long long capacity, void* stream);

/* Surface distances of two label stacks: the surfaces, a distance transform evaluated on chosen pixels only, and the census that
 * reduces every object's surface-to-surface distances to a few integers (surface.py: label_surface, edt_at, surface_census,
 * surface_metrics; evaluator.surface_metrics).  Integers only, integer atomics only: bit-reproducible.  All stacks [n][H][W],
 * contiguous, device; uint8 stacks may start at any byte.  SENTINEL = 2^31 - 1.
 * rmem_label_surface: surface[p] = labels[p] where a 4-neighbour of p holds another value or lies outside the frame, else 0 (for
 * a value v: mask & ~binary_erosion(mask, cross, border_value=0), mask = labels == v).  One launch, every byte of surface is
 * written, nothing outside the frame is read.  A void label of 255 is an ordinary value.
 * rmem_label_edt_at: rmem_label_edt's to-value transform at the pixels with keys[p] == key alone: there samples[p] = min |p - q|^2
 * over q with labels[q] == value, SENTINEL where the frame holds none; every other entry of samples is left untouched.  value and
 * key in 0..255.  workspace: rmem_label_edt_workspace_bytes(n, H, W) bytes, 4-byte aligned.  Two launches: the column pass, and a
 * row pass that leaves a row without a key pixel before it reads anything else.
 * rmem_surface_census: keys_a / keys_b are surface stacks, samples_a / samples_b int32 stacks read only where the key is in
 * 1..num_objs: samples_a[p], key i, is the squared distance of p on the surface of object i of a to that surface of b (what
 * rmem_label_edt_at(keys_b, keys_a, .., i, i, samples_a, ..) writes), samples_b the mirror image.  Per frame f and object i the sets
 * 0 (a -> b), 1 (b -> a) and 2 (both pooled) of samples; a set holds sentinels only (the other surface is empty) or none.
 * table int64 [n][num_objs][3][9] = (count m, sum_fix = sum of floor(sqrt(d2 * 2^32)), max, lo, hi, within[0..3]): lo and hi are
 * the samples of rank r_lo = (m - 1) * q / 10000 and r_hi = min(r_lo + 1, m - 1) in ascending order (q in hundredths of a percent:
 * with frac = ((m - 1) * q % 10000) / 10000, sqrt(lo) + frac * (sqrt(hi) - sqrt(lo)) is the linear percentile of the distances);
 * within[t] counts the samples with d2 <= tol2[t], t < num_tol <= 4, 0 for unused t; tol2: HOST array, entries in 0..2^30 - 1.  An
 * empty set: (0, 0, -1, -1, -1, 0, 0, 0, 0); sentinels only: (m, 0, SENTINEL, SENTINEL, SENTINEL, 0, 0, 0, 0).  Every entry of
 * table is written.  workspace: rmem_surface_census_workspace_bytes(n, num_objs) bytes (0 for n or num_objs out of range), 8-byte
 * aligned; prior contents do not matter.  A memset and eight launches: an accumulate walk, a radix select of lo over three
 * 10-bit digits (a histogram walk and a pick each), an integer-min walk for hi, the table.  No state between calls, no host sync.
 * Refused (non-zero, nothing launched): a null pointer, n outside 1..65535, non-positive H / W, H * W above 2^26, H or W above
 * 16384, value / key outside 0..255, num_objs outside 1..255, num_tol outside 0..4, q outside 0..10000, a tol2 entry outside
 * 0..2^30 - 1, a workspace too small or misaligned. */
int rmem_label_surface(const unsigned char* labels, int n, int H, int W, unsigned char* surface, void* stream);
int rmem_label_edt_at(const unsigned char* labels, const unsigned char* keys, int n, int H, int W, int value, int key, int* samples,
                      void* workspace, long long workspace_bytes, void* stream);
long long rmem_surface_census_workspace_bytes(int n, int num_objs);   /* host only */
int rmem_surface_census(const int* samples_a, const unsigned char* keys_a, const int* samples_b, const unsigned char* keys_b, int n,
                        int H, int W, int num_objs, const int* tol2, int num_tol, int q, long long* table, void* workspace,
                        long long workspace_bytes, void* stream);

/* Label stacks thinned to skeletons (Guo and Hall 1989, algorithm A1; the rule of bwmorph's 'thin') and the list of a stack's
 * non-zero pixels (skeleton.py: thin, pixels, tile, table; evaluator.next_scribbles).  Bytes and integers only: bit-identical to a
 * host restatement.  labels: uint8 [n][H][W], contiguous, device, may start at any byte; frames are independent.
 * The rule.  Value 0 is background and never changes.  For a pixel p of value L != 0 the neighbour bit x_i is 1 iff that neighbour
 * lies inside the frame and holds L; x1..x8 = E, NE, N, NW, W, SW, S, SE (y grows downward), x9 = x1.  Pixels of other values count
 * as background for p: every value is thinned as if it were alone in the frame, a void label of 255 is an ordinary value.  p is
 * deleted (set to 0) in a sub-iteration iff  X_H = sum_{i=1..4} [x_{2i-1} = 0 and (x_{2i} = 1 or x_{2i+1} = 1)] = 1,
 * 2 <= min(n1, n2) <= 3 with n1 = sum_{k=1..4} (x_{2k-1} | x_{2k}), n2 = sum_{k=1..4} (x_{2k} | x_{2k+1}), and in an even
 * sub-iteration (x2 | x3 | !x8) & x1 = 0, in an odd one (x6 | x7 | !x4) & x5 = 0.  A sub-iteration is synchronous: every decision
 * is taken from the state before it.  With mask bit k = x_{k+1} each rule is a 256-entry table of 37 set entries.
 * rmem_label_thin applies the sub-iterations first, first + 1, .., first + count - 1 (sub-iteration s uses table s & 1) to labels
 * and writes every byte of out; out may be the same pointer as labels (otherwise labels is read only and the two must not
 * overlap).  lost int32 [n][2], every entry written: lost[f][0] = the pixels frame f lost during the call, lost[f][1] = those lost
 * in the call's last two sub-iterations (in the only one if count = 1): with count >= 2, lost[f][1] == 0 means that frame f is at
 * its fixed point.  workspace: rmem_label_thin_workspace_bytes(n, H, W) bytes (0 for refused geometry), 4-byte aligned, prior
 * contents do not matter: a second stack and two bytes per tile and frame.  A memset and ceil(count / k) launches of up to k
 * sub-iterations each on tiles of th x tw pixels with a halo of k (rmem_label_thin_tile), one device copy more where out ==
 * labels and that number is odd; a tile none of whose 3 x 3 tiles changed in the round before is skipped (RMEM_THIN_SKIP=0 in the
 * environment: never, for A/B runs).  rmem_label_thin_table: the table of a parity as 256 bits, bit m of byte m / 8 = mask m is
 * deleted; host only, the constant the kernels use.
 * rmem_label_pixels_count / _write: the non-zero pixels of a uint8 stack as a list in raster order, frame by frame.  count writes
 * totals int32 [n] = the non-zero pixels of every frame and leaves offsets in the workspace; write, on the same stack and workspace,
 * writes row i of entries int32 [total][4] = (frame, y, x, value) and, with samples (an int32 stack [n][H][W]; NULL with sampled
 * NULL: none), sampled[i] = samples at that pixel.  Rows at or beyond `capacity` are not written.  workspace:
 * rmem_label_pixels_workspace_bytes(n, H, W) bytes, 8-byte aligned.  Three launches and one.
 * No state between calls, no host sync, integer atomics only.  Refused (non-zero, nothing launched): a null pointer, n outside
 * 1..65535, non-positive H / W, H * W above 2^26, first < 0, count < 1, first + count above 2^31 - 1, parity other than 0 / 1,
 * capacity < 0, samples without sampled or the reverse, a workspace too small or misaligned. */
int rmem_label_thin_tile(int* th, int* tw, int* k);   /* host only */
int rmem_label_thin_table(int parity, unsigned char* out /* [32] */);   /* host only */
long long rmem_label_thin_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_thin(const unsigned char* labels, int n, int H, int W, int first, int count, unsigned char* out, int* lost,
                    void* workspace, long long workspace_bytes, void* stream);
long long rmem_label_pixels_workspace_bytes(int n, int H, int W);   /* host only */
int rmem_label_pixels_count(const unsigned char* stack, int n, int H, int W, int* totals, void* workspace, long long workspace_bytes,
                            void* stream);
int rmem_label_pixels_write(const unsigned char* stack, const int* samples, int n, int H, int W, long long capacity, int* entries,
                            int* sampled, const void* workspace, long long workspace_bytes, void* stream);

/* Label stacks traced into polygon rings: the outer contours and the holes of every object of every frame, the last way a run's
 * labels leave the device (polygons.py: trace, trace_label_stack; evaluator.polygon_results) -- what CVAT / Labelme tracks and
 * COCO `segmentation` lists are made of, and what labels.cpu() plus a sequential border follower per frame and object computes.
 * labels: uint8 [n][H][W], contiguous, device, may start at any byte.  Objects are the values 1..num_objs; 0 and every value above
 * num_objs are "not an object".  Frames are independent.  connectivity (4 or 8) is that of the objects.
 * Edges.  Vertices are pixel corners (x, y), 0 <= x <= W, 0 <= y <= H, y pointing down.  A pixel (y, x) of object v owns a
 * directed unit edge on each side whose neighbour does not hold v (a side on the frame's edge is such a side); the object lies on
 * the right of the direction of travel:
 *   side 0 top    (x, y)         -> (x + 1, y)      east        side 1 right  (x + 1, y)     -> (x + 1, y + 1)  south
 *   side 2 bottom (x + 1, y + 1) -> (x, y + 1)      west        side 3 left   (x, y + 1)     -> (x, y)          north
 * The edge id is (y * W + x) * 4 + side.
 * Successor.  For an edge of pixel (y, x), side s, A is the pixel ahead on the right and B the pixel ahead on the left of its end
 * vertex: s = 0: A (y, x + 1), B (y - 1, x + 1); s = 1: A (y + 1, x), B (y + 1, x + 1); s = 2: A (y, x - 1), B (y + 1, x - 1);
 * s = 3: A (y - 1, x), B (y - 1, x - 1).  a / b: A / B holds v (false outside the frame).  8: left turn if b, else straight if a,
 * else right turn.  4: right turn if not a, else straight if not b, else left turn.  Right turn: side (s + 1) % 4 of the same
 * pixel; straight: side s of A; left turn: side (s + 3) % 4 of B.  This is a permutation of a frame's edges; its cycles are the
 * rings.
 * Rings.  A ring's start edge is its smallest edge id.  Its vertices are the start corners of those of its edges whose heading
 * differs from their predecessor's, in walk order beginning at the start edge (which need not be a corner itself; for a hole it
 * usually is not).  area2 is the shoelace sum of (x_i * y_{i+1} - x_{i+1} * y_i): positive for an outer ring, negative for a
 * hole.  Collinear vertices never occur; a vertex can occur twice in one ring (the saddle between two diagonal pixels under 8).
 * Output, all device, in the order (frame, start edge):
 *   rings  int32 [max_edges / 4 + 1][8]: (frame, value, first vertex, vertex count, area2, start edge id, edge count, 0); a ring's
 *          vertices are contiguous, and ring r + 1 starts where ring r ends.
 *   verts  int32 [max_edges][2]: (x, y).
 *   counts int32 [4]: (edges E, rings R, vertices V, status).
 * Prior contents of the outputs do not matter; entries beyond R and V are not written.  E above max_edges: status =
 * RMEM_POLY_ST_CAPACITY, counts[0] is still the exact E (2^31 - 1 where it is larger), R = V = 0, nothing is written to rings or
 * verts.  Every loop is bounded; RMEM_POLY_ST_LINK (a successor was not found among its pixel's edges) and RMEM_POLY_ST_ORDER (a
 * ring position out of range) say that one ran out or an index went astray: a bug, never a condition.
 * workspace: rmem_label_polygons_workspace_bytes(n, H, W, max_edges) bytes of device memory, 16-byte aligned (0 for refused
 * arguments): 40 bytes per edge of capacity plus 4 per walk unit.  A walk unit is rmem_label_polygons_unit() pixels of one row.
 * No state between calls, no host sync, 15 + ceil(log2(min(max_edges, 4 H W))) launches on `stream`, integer arithmetic only:
 * bit-reproducible.  Refused (non-zero, nothing launched): a null pointer, n outside 1..65535, non-positive H / W, H * W above
 * 2^26, num_objs outside 1..255, a connectivity other than 4 or 8, max_edges below 4, a workspace smaller than the query says. */
#define RMEM_POLY_ST_CAPACITY 1
#define RMEM_POLY_ST_LINK 2
#define RMEM_POLY_ST_ORDER 4
int rmem_label_polygons_unit(void);   /* host only */
size_t rmem_label_polygons_workspace_bytes(int n, int H, int W, int max_edges);   /* host only */
int rmem_label_polygons(const unsigned char* labels, int n, int H, int W, int num_objs, int connectivity, int max_edges,
                        void* workspace, size_t workspace_bytes, int* rings, int* verts, int* counts, void* stream);

/* The rings of rmem_label_polygons simplified (Douglas-Peucker, exact): a traced ring is a pixel staircase with a vertex at every
 * corner; a person who corrects a track in a labelling tool wants tens of points per object (polygons.py: simplify,
 * trace_label_stack(tolerance=...); evaluator.polygon_results(tolerance=...)).  One call on `stream` behind the tracer, no host
 * sync: R and V are read on the device.
 * Input: rings [max_rings][8], verts [max_verts][2], counts [4] = (E, R, V, status) as rmem_label_polygons writes them.  Only the
 * columns 2 (first vertex) and 3 (vertex count) of a ring row and the vertices are interpreted: any table of that form is valid,
 * not only a traced one.  Coordinates lie in 0..32767, which keeps every product below 2^62.
 * Tolerance.  T = tolerance_16ths, 0..1024: 1/16 pixel steps, at most 64 pixels.
 * Rule for one ring p_0 .. p_{k-1}, p_k := p_0, k >= 1.  Anchors: vertex 0 and B, the vertex of 1..k-1 farthest from p_0 by squared
 * distance, the smallest index among equals (k = 1: the output is that one vertex).  Kept = {0, B} + DP(0, B) + DP(B, k).
 * DP(i, j): nothing when j - i < 2; else m = the vertex of i < m < j with the largest key(m), the smallest m among equals; if
 * key(m) > thr, m is kept and DP(i, m) and DP(m, j) follow.  key is the squared distance to the SEGMENT p_i p_j times L: with
 * a = p_j - p_i, L = |a|^2, b = p_m - p_i, t = a.b:  L = 0: key = |b|^2, thr = floor(T^2 / 256);  L > 0: thr = floor(T^2 L / 256)
 * and key = |b|^2 L if t <= 0, |p_m - p_j|^2 L if t >= L, (a x b)^2 otherwise.  64-bit integers, no division by data; a x b
 * needs 64 bits before it is squared; every key is below 2^62 and T^2 L below 2^51.  The segment, not the line: a ring can visit
 * a vertex twice, so p_i = p_j happens.
 * Output, all device, in the input's ring order:
 *   rings_out  [max_rings][8]: the input row with column 2 = the new first vertex, column 3 = the kept count, column 7 = the
 *              original vertex count; column 4 stays the TRACED area2 (the exact pixel area; its sign still tells hole from
 *              exterior), column 5 the start edge.
 *   verts_out  [max_verts][2]: the kept vertices in ring order, ring after ring, contiguous.
 *   counts_out [4]: (V of the input, R, V_out, status).
 * Rows beyond R and V_out are not written.  A non-zero input status is passed on with R = V_out = 0 and nothing written.
 * RMEM_SIMPLIFY_ST_TABLE: R outside 0..max_rings, V outside 0..max_verts, or the vertex counts of the rings sum to more than
 * max_verts (only when rings share vertices, which a traced table never does): (V, 0, 0, RMEM_SIMPLIFY_ST_TABLE), nothing written.
 * RMEM_SIMPLIFY_ST_RING: a ring row whose (first, count) is no range of 0..V with count >= 1, or a vertex of a ring outside
 * 0..32767: that ring is emitted with 0 vertices, the others are unaffected.  Every index read from device memory is checked
 * before use; every loop is bounded, a ring's refinement runs at most its vertex count of rounds.
 * Properties: the kept vertices are a subsequence of the ring with both anchors; every dropped vertex is within T / 16 of the
 * segment of its kept neighbours, so ring and simplification are within Hausdorff distance T / 16 of each other, and under the
 * even-odd fill below a pixel centre farther than that from every ring edge of its frame keeps its value.  Topology is NOT
 * preserved: a simplified ring may touch or cross itself or a neighbour (as OpenCV's approxPolyDP).  T = 0 drops exactly the
 * vertices on the segment between their kept neighbours.
 * 10 launches whatever the data, no workgroup waits for another: a ring of at most rmem_polygon_simplify_short_max() vertices
 * lives in one wave, a longer one in one workgroup -- one very long ring runs on one compute unit, for as many rounds as its
 * recursion is deep.  Both classes give the same bytes; integer maxima and minima only: bit-reproducible.
 * workspace: rmem_polygon_simplify_workspace_bytes(max_rings, max_verts) bytes, 16-byte aligned (0 for refused arguments): 32
 * bytes per vertex and 24 per ring of capacity (and 12 per 2048 rings); prior contents do not matter.  Refused (non-zero, nothing launched): a null
 * pointer, a capacity outside 1..2^31-1, tolerance_16ths outside 0..1024, a misaligned or too small workspace. */
#define RMEM_SIMPLIFY_ST_TABLE 8
#define RMEM_SIMPLIFY_ST_RING 16
int rmem_polygon_simplify_short_max(void);   /* host only */
size_t rmem_polygon_simplify_workspace_bytes(long long max_rings, long long max_verts);   /* host only, 0 for refused arguments */
int rmem_polygon_simplify(const int* rings, const int* verts, const int* counts, long long max_rings, long long max_verts,
                          int tolerance_16ths, void* workspace, size_t workspace_bytes, int* rings_out, int* verts_out,
                          int* counts_out, void* stream);

/* The inverse: annotation polygons filled into uint8 label maps labels[frames][H][W] (contiguous, device, may start at any byte),
 * the way polygon tracks (CVAT, Labelme, COCO `segmentation` lists) enter a run (polygons.py: PackedPolygons, fill_labels_into,
 * fill_label_stack; evaluator.labels_from_polygons).  One call on `stream`, no host sync, no state kept between calls; only the
 * vertices' edges cross to the device.
 * The rule.  A shape is a set of rings (an exterior, holes, several pieces, in any order and orientation; rings may self-intersect,
 * repeat vertices, have zero area or leave the frame), filled under the even-odd rule sampled at pixel centres, in exact integer
 * arithmetic on 1/256-pixel fixed point.  A vertex (x, y) -- x right, y down, pixel corners at integers, as rmem_label_polygons
 * emits them -- is X = rint(256 x), Y = rint(256 y) (ties to even), |x|, |y| <= 2^20.  The centre of pixel (y, x) is
 * (256 x + 128, 256 y + 128).  An edge (X0, Y0) -> (X1, Y1), oriented so that Y0 < Y1, crosses the sample row of y iff
 * Y0 <= 256 y + 128 < Y1; horizontal edges cross nothing.  A crossing toggles every pixel of that row from column c on, c the
 * smallest integer with (256 c + 128) * dY >= X0 * dY + (256 y + 128 - Y0) * dX, clamped to 0..W (dX = X1 - X0, dY = Y1 - Y0;
 * every term stays below 2^59).  A pixel belongs to the shape iff it was toggled an odd number of times.  So left and top edges
 * are inclusive, right and bottom ones exclusive, and shapes that share an edge neither overlap nor leave a gap; the rings of
 * rmem_label_polygons fill back to exactly the pixels they were traced from.  (Not pycocotools' frPoly, which upsamples the
 * outline five times and rounds in its own way: masks can differ from it in boundary pixels.)
 * A stack.  Frame f lists its shapes in painting order, each with a label value 1..255: label[shape] = value in listing order (the
 * later shape wins), 0 under no shape.  Every byte of the frames of the pass is written by the call.
 * Input, all device, built by the host:
 *   edge_xy     int32 [nedges][4], 16-byte aligned: (X0, Y0, X1, Y1) of every edge that crosses a sample row of the frame, in any
 *               orientation, listed shape by shape.
 *   edge_shape  int32 [nedges]: the edge's shape (index into shapes).
 *   edge_first  int32 [nedges + 1]: the exclusive prefix of the edges' crossing counts (an edge's count: the rows y in 0..H-1 it
 *               crosses); edge_first[nedges] is the total, at most 2^31 - 1.
 *   shapes      RmemPolyShape [nshapes]: frame (non-decreasing along the table), value, the box of the pixels whose centres the
 *               shape can cover, clipped to the frame (columns x0..x1-1, rows y0..y1-1; empty: the shape paints nothing and has no
 *               plane), and the word offset of its bit plane -- (y1 - y0) rows of ceil((x1 - x0) / 32) 32-bit words, bit i of a
 *               row = column x0 + i -- among the planes of the whole table.
 *   frame_shape int32 [frames + 1]: the first shape of every frame; frame_shape[frames] = nshapes.
 * pass (host): the frames the call fills and what belongs to them -- the shapes listed for those frames, their edges, the crossings
 * of those edges (cross0 = edge_first[edge0]), and the planes (plane0 = the first plane's offset, plane_words = their sum).  One
 * table can so be filled in several passes when the planes of all frames exceed the workspace the caller wants to spend.
 * workspace: rmem_polygon_fill_workspace_bytes(plane_words) bytes, 16-byte aligned (0 for refused arguments); the call clears the
 * pass's planes itself, a dirty workspace never shows.
 * status (device, int32 [nshapes]) is written for every shape of the pass, 0 = painted.  Every index read from device memory is
 * range-checked before it is used; a failed check sets a bit instead of making the access, and a shape with a non-zero status paints
 * nothing:
 *   ST_DESC    frame outside the pass or below the frame of the shape before, the shape outside its frame's range in frame_shape,
 *              value outside 1..255, a box outside the frame, a plane outside the pass's planes; also set when an edge names a
 *              shape outside the pass (on the pass's first or last shape, whichever is nearer to the name)
 *   ST_PREFIX  the crossing prefix disagrees with an edge (more crossings than the edge has rows, a decreasing prefix)
 *   ST_EDGE    an edge coordinate beyond 2^28, or a crossing in a row outside the shape's box
 * Edges without a crossing in the pass are never looked at.  5 launches per pass (a memset, the check, one thread per crossing,
 * one per plane row, one per 16 output bytes); the only atomics are integer XOR and OR: the bytes do not depend on the order of
 * arrival.  Every loop is bounded.
 * Refused (non-zero, nothing launched): null pointers, frames outside 1..65535, non-positive H / W, H * W above 2^26, nshapes
 * outside 1..65535*255, nedges outside 0..2^30, a pass whose frames, shapes or edges are no range of the tables', whose crossings
 * leave 0..2^31-1 or exist without edges, whose plane words leave 0..2^34; a misaligned workspace or edge_xy, a workspace smaller
 * than the query says.
 * Replaces a host rasteriser per frame and object (Pillow, pycocotools) and the upload of H * W bytes per frame. */
typedef struct RmemPolyShape {
  int frame;            /* 0..frames-1 */
  int value;            /* 1..255: the label the shape paints */
  int x0, y0, x1, y1;   /* the box, clipped to the frame */
  long long plane;      /* word offset of the shape's bit plane */
} RmemPolyShape;
typedef struct RmemPolyPass {
  int frame0, frames;
  int shape0, shapes;
  int edge0, edges;
  long long cross0, crossings;
  long long plane0, plane_words;
} RmemPolyPass;
#define RMEM_POLYFILL_ST_DESC 1
#define RMEM_POLYFILL_ST_PREFIX 2
#define RMEM_POLYFILL_ST_EDGE 4
size_t rmem_polygon_fill_workspace_bytes(long long plane_words);   /* host only, 0 for refused arguments */
int rmem_polygon_fill_labels(const int* edge_xy, const int* edge_shape, const int* edge_first, int nedges,
                             const RmemPolyShape* shapes /* device */, int nshapes, const int* frame_shape, int frames, int H, int W,
                             const RmemPolyPass* pass /* host */, void* workspace, size_t workspace_bytes,
                             unsigned char* labels /* device [frames][H][W] */, int* status /* device [nshapes] */, void* stream);

/* Strokes drawn into uint8 label maps labels[frames][H][W] (contiguous, device, may start at any byte): scribbles, clicks and
 * polylines, the way interactive rounds and DAVIS-interactive scribble files enter a run (strokes.py: PackedStrokes,
 * draw_labels_into, draw_label_stack; evaluator.seeds_from_scribbles, seeds_from_clicks, labels_from_scribbles).  One call on
 * `stream`, no host sync, no state kept between calls; only the strokes' segments cross to the device.
 * Coordinates are PIXEL-INDEX coordinates: the centre of pixel (y, x) is the point (x, y) -- what evaluator.next_clicks and
 * next_scribbles return and the DAVIS toolkit uses, NOT the corner convention of the polygon fill above.  Fixed point is 1/256
 * pixel: X = rint(256 x), Y = rint(256 y) in float64 (ties to even), |x|, |y| <= 2^20; pixel (py, px) is the point
 * P = (256 px, 256 py).
 * A stroke is a value 0..255 (0 erases), a radius r in 0..256 pixels, R = rint(256 r), and a polyline of at least one point (one
 * point: a click), given as segments A -> B; a lone point is the one segment A -> A.  A frame lists its strokes in painting order:
 * a pixel covered by several strokes takes the value of the last one, a pixel covered by none is 0, or keeps its byte when `over`
 * is not zero.
 * Round brush, R >= 1.  A stroke covers the pixels whose centre lies within R of any of its segments, so joins and caps are round
 * and a lone point covers a disc.  For a segment A -> B with d = B - A, w = P - A, t = w.d, L = d.d: if t <= 0 the pixel is
 * covered iff |w|^2 <= R^2; if t >= L iff |P - B|^2 <= R^2; otherwise iff (w x d)^2 <= R^2 L.  Integer arithmetic throughout: every
 * 64-bit term stays below 2^60, the two products of the last comparison are taken in 128 bits.
 * Hairline, R == 0: a digital line, 8-connected and independent of direction.  The host orients every segment by its major axis M
 * (x if |dX| >= |dY|, else y; m is the other one) so that dM > 0; a segment with d = 0 draws only its endpoint's pixel.  Drawn are
 * the pixel of each endpoint, rounded half up per axis, (X + 128) >> 8 with a floor shift, and for every integer k with
 * A_M <= 256 k <= B_M the pixel whose major index is k and whose minor index is floor((N + 128 dM) / (256 dM)),
 * N = A_m dM + (256 k - A_M) d_m: the exact minor coordinate rounded half up.  A path of integer vertices that are 8-neighbours
 * draws exactly its vertices' pixels.
 * Anything off the frame is clipped and is no error.  (Equality with the DAVIS toolkit's Bresenham and Bezier code is not claimed.)
 * Input, all device, built by the host:
 *   seg_xy       int32 [nsegs][4], 16-byte aligned: (AX, AY, BX, BY) of every segment that has work items, listed stroke by stroke.
 *   seg_stroke   int32 [nsegs]: the segment's stroke (index into strokes).
 *   seg_first    int32 [nsegs + 1]: the exclusive prefix of the segments' work items; seg_first[nsegs] is the total, at most
 *                2^31 - 1.  A segment's box is the pixels it can cover clipped to the frame -- columns ceil((minX - R) / 256) ..
 *                floor((maxX + R) / 256) for a round brush, (minX + 128) >> 8 .. (maxX + 128) >> 8 for a hairline, rows alike.  A
 *                segment with an empty box has no work items and is not listed.  Otherwise a round-brush segment has one work item
 *                per row of its box, a hairline two (its endpoints) plus one per k above with the major index inside the frame.
 *   strokes      RmemStroke [nstrokes]: frame (non-decreasing along the table), value, R, the union of the boxes of its segments
 *                (columns x0..x1-1, rows y0..y1-1; all zero when it has none) and slot, the place of its frame in `stroked`.
 *   frame_stroke int32 [frames + 1]: the first stroke of every frame; frame_stroke[frames] = nstrokes.
 *   stroked      int32 [nstroked]: the frames that list at least one stroke, ascending.
 * pass (host): the frames the call draws and what belongs to them -- the strokes listed for those frames, their segments, the work
 * items of those segments (item0 = seg_first[seg0]) and the stroked frames among them (slot0, slots).
 * workspace: rmem_stroke_workspace_bytes(slots, H, W) bytes, 16-byte aligned: one int32 owner map [H][W] per STROKED frame of the
 * pass (frames without strokes have none), cleared by the call itself: a dirty workspace never shows.  A covered pixel takes the
 * maximum of (the stroke's index within its frame) + 1 by an integer atomic; max commutes, the bytes do not depend on the order of
 * arrival.  Then, per 16 output bytes: where the owner is not zero the byte is the owning stroke's value; otherwise it is 0, or
 * untouched when `over` is not zero -- then frames without strokes are not touched at all, while without `over` they are zeroed.
 * status (device, int32 [nstrokes]) is written for every stroke of the pass, 0 = drawn.  Every index read from device memory is
 * range-checked before it is used, and a stroke with a non-zero status draws nothing, the others are intact:
 *   ST_DESC    frame outside the pass or below the frame of the stroke before, the stroke outside its frame's range in
 *              frame_stroke, value outside 0..255, R outside 0..65536, a box outside the frame, a slot outside the pass's or one
 *              whose entry in `stroked` is another frame; also set when a segment names a stroke outside the pass (on the pass's
 *              first or last stroke, whichever is nearer to the name)
 *   ST_PREFIX  the work-item prefix disagrees with a segment (its difference is not the segment's count, it decreases, or its ends
 *              are not the pass's item0 and item0 + items)
 *   ST_SEGMENT a coordinate beyond 2^28, a hairline segment with d != 0 and dM <= 0, or a segment whose box leaves its stroke's box
 * 5 launches per pass: a memset, one thread per stroke, one per segment (the checks above: all of them precede the first atomic,
 * because a maximum cannot be taken back), one per work item, one per 16 output bytes.  Every loop is bounded.
 * Refused (non-zero, nothing launched): null pointers, frames outside 1..65535, non-positive H / W, H * W above 2^26, nstrokes
 * outside 1..2^30, nsegs outside 0..2^30, nstroked outside 1..frames, a pass whose frames, strokes, segments or slots are no range
 * of the tables', whose items leave 0..2^31-1 or exist without segments and strokes, whose strokes exist without slots; a
 * misaligned workspace or seg_xy, a workspace smaller than the query says. */
typedef struct RmemStroke {
  int frame;            /* 0..frames-1 */
  int value;            /* 0..255: the label the stroke draws, 0 erases */
  int radius;           /* R = rint(256 r), 0..65536; 0: a hairline */
  int x0, y0, x1, y1;   /* the box, clipped to the frame */
  int slot;             /* stroked[slot] == frame */
} RmemStroke;
typedef struct RmemStrokePass {
  int frame0, frames;
  int stroke0, strokes;
  int seg0, segs;
  int slot0, slots;
  long long item0, items;
} RmemStrokePass;
#define RMEM_STROKE_ST_DESC 1
#define RMEM_STROKE_ST_PREFIX 2
#define RMEM_STROKE_ST_SEGMENT 4
size_t rmem_stroke_workspace_bytes(int stroked_frames, int H, int W);   /* host only, 0 for refused arguments */
int rmem_stroke_draw_labels(const int* seg_xy, const int* seg_stroke, const int* seg_first, int nsegs,
                            const RmemStroke* strokes /* device */, int nstrokes, const int* frame_stroke, const int* stroked,
                            int nstroked, int frames, int H, int W, const RmemStrokePass* pass /* host */, void* workspace,
                            size_t workspace_bytes, unsigned char* labels /* device [frames][H][W] */, int over,
                            int* status /* device [nstrokes] */, void* stream);

/* Region-similarity (Jaccard) counts per object id for one mask pair: counts[2*id] += |pred==id & gt==id|,
 * counts[2*id+1] += |pred==id | gt==id| over the n pixels whose ground truth is not `void_label`; the caller zeroes
 * counts (uint64 [2 * num_ids]).  Replaces evaluation/source/metrics.py:6-37 (db_eval_iou) per object. */
int rmem_mask_iou_counts(const unsigned char* pred, const unsigned char* gt, long long n, int num_ids, int void_label,
                         unsigned long long* counts, void* stream);

/* Clip scoring: boundary accuracy F and region similarity J counts for a whole stack of frames in one call, no host sync.
 * pred / gt: uint8 label stacks [frames][H][W] with ids 0..num_ids-1 (2 <= num_ids <= 32); gt may carry `void_label`, whose pixels
 * are cleared from both masks.  counts: uint64 [frames][num_ids][6], zeroed on the stream by the call, row of id 0 left zero:
 *   [0] n_fg      boundary pixels of pred == id        [1] n_gt      boundary pixels of gt == id
 *   [2] fg_match  pred boundary inside the gt boundary dilated by a disk of `radius` (dx^2 + dy^2 <= radius^2, zero padding)
 *   [3] gt_match  gt boundary inside the dilated pred boundary
 *   [4], [5]      J intersection and union, per frame what rmem_mask_iou_counts returns.
 * The boundary map is seg2bmap at the mask's own size (a pixel differs from its east, south or south-east neighbour; last row:
 * east only, last column: south only, bottom-right pixel: 0).  1 <= radius <= 63.  workspace: rmem_clip_score_workspace_bytes
 * bytes of device memory (the boundary bit planes), no state kept between calls.
 * Replaces evaluation/source/metrics.py db_eval_boundary / f_measure (seg2bmap + cv2.dilate with skimage's disk) per object and
 * frame, and a per-frame loop over db_eval_iou. */
size_t rmem_clip_score_workspace_bytes(int frames, int H, int W, int num_ids);   /* 0 on bad geometry */
/* The dilation radius f_measure uses: bound_th itself when bound_th >= 1 (it must be an integer), else
 * ceil(bound_th * sqrt(H^2 + W^2)); 0.008 gives 8 at 480x854 and 18 at 1080x1920.  -1 on a bad argument.  Host only. */
int rmem_boundary_radius(int H, int W, double bound_th);
int rmem_clip_score_counts(const unsigned char* pred, const unsigned char* gt, int frames, int H, int W, int num_ids,
                           int void_label, int radius, void* workspace, unsigned long long* counts, void* stream);

/* Pair boundary census: the boundary match counts of EVERY object of a with every object of b, per frame, in one call, no host
 * sync -- what the boundary accuracy F of every (predicted, annotated) pair is made of (pairs.py: pair_boundary_counts, pair_f,
 * pair_jf; evaluator.score_clip_objects, score_unsupervised_clip), where rmem_clip_score_counts compares id i with id i only and
 * stops at 31 objects.  a, b: uint8 label stacks [frames][H][W], contiguous, each may start at any byte; objects are 1..num_a and
 * 1..num_b (1 <= num <= 255), every other value is "no object".  With void = (b == void_label), A_i = (a == i) & ~void,
 * B_j = (b == j) & ~void, d = seg2bmap at the mask's own size (rmem_clip_score_counts' boundary map) and (+) r = dilation by the
 * disk dx^2 + dy^2 <= radius^2 with zero padding:
 *   bnd_a[f][i] = |dA_i|                        int32 [frames][num_a + 1]
 *   bnd_b[f][j] = |dB_j|                        int32 [frames][num_b + 1]
 *   match[f][i][j][0] = |dA_i & (dB_j (+) r)|   int32 [frames][num_a + 1][num_b + 1][2]
 *   match[f][i][j][1] = |dB_j & (dA_i (+) r)|
 * Index 0 (background) is a zero row and column, so ids index directly.  For num <= 31 the diagonal equals columns 0..3 of
 * rmem_clip_score_counts.  A void_label outside 0..255 means no void; one inside must lie above num_b.  All three outputs are
 * zeroed on the stream by the call: prior contents do not matter.
 * workspace: 8-byte aligned device memory of workspace_bytes bytes for the bit planes, per frame (num_a + num_b + 2) planes of
 * H * ceil(W / 64) 64-bit words (the ids of both sides and, per side, the OR of its boundaries);
 * rmem_pair_boundary_workspace_bytes(frames, ...) is what `frames` frames need (0 on bad arguments), 132 MB per 1080p frame at
 * 255 + 255 ids.  The call works in passes of min(frames, workspace_bytes / one frame's bytes) frames on the stream, clears a
 * pass's planes itself (a dirty workspace never shows) and keeps no state between calls.  Integer atomics only: the result does not
 * depend on the order of arrival and is bit-reproducible.
 * Refused (non-zero, nothing launched): a null pointer, num_a or num_b outside 1..255, radius outside 1..63 (the word-triple
 * dilation reaches one word to each side), frames outside 1..65535, non-positive H / W, H * W above 2^26 (which keeps every count
 * inside int32), H * ceil(W / 64) of 2^30 or more, a void_label in 0..num_b, a workspace smaller than one frame's planes or not
 * 8-byte aligned. */
size_t rmem_pair_boundary_workspace_bytes(int frames, int H, int W, int num_a, int num_b);   /* host only */
int rmem_pair_boundary_counts(const unsigned char* a, const unsigned char* b, int frames, int H, int W, int num_a, int num_b,
                              int void_label, int radius, void* workspace, size_t workspace_bytes, int* bnd_a, int* bnd_b,
                              int* match, void* stream);

/* Palette-PNG payloads: one zlib stream per uint8 label map [frames][H][W] (contiguous, device), in one call on `stream`, no host
 * sync.  lut: 256 device bytes applied to every label as it is read (save_mask's un-squeeze of object ids), or NULL.  The streams
 * are packed back to back: stream f is out[offsets[f] : offsets[f+1]), offsets (device, int64 [frames + 1]) starts at 0; out holds
 * frames * rmem_png_zlib_bound(H, W) bytes and is 4-byte aligned.  Whatever must be zero (the used part of out) is zeroed on the
 * stream inside the call; workspace: rmem_png_workspace_bytes bytes, 16-byte aligned, no state kept between calls.
 * The stream of one frame is fixed bit for bit:
 *   78 01; one DEFLATE block, BFINAL = 1, BTYPE = 01 (fixed Huffman codes, RFC 1951 3.2.6); the end-of-block code; zero bits up to
 *   the byte boundary; the Adler-32 of the filtered bytes, big-endian.
 *   Filtered bytes: per row the filter type 2 (Up), then the W bytes label[y][x] - label[y-1][x] (mod 256), row -1 all zero.
 *   Tokens: each row's W + 1 filtered bytes are cut into maximal runs of equal bytes (a run never crosses a row); a run of value v
 *   and length L is: literal v; rem = L - 1; while rem >= 3 one match of distance 1 and length t = min(rem, 258), rem -= t; then
 *   rem (0, 1 or 2) literals v.  Length 258 uses code 285.
 * No token costs more than 9 bits per byte it covers: rmem_png_zlib_bound = 2 + ceil((3 + 9 (W + 1) H + 7) / 8) + 4.
 * Wrapped into signature / IHDR (8 bit, colour type 3) / PLTE / IDAT / IEND on the host (rmem_ocu_amd/png.py; the chunk CRCs stay
 * there).  H * W <= 2^26, so that a frame's bit count fits 32 bits.
 * Replaces utils/image.py:90-106 (save_mask: Pillow's PNG encoder, one frame at a time on a host copy of the label map). */
size_t rmem_png_zlib_bound(int H, int W);                         /* host only, 0 on bad geometry */
/* uint32 [frames][H] x 3 (row bits, Adler-32 partials) + per frame its Adler-32 and byte size.  Host only, 0 on bad geometry. */
size_t rmem_png_workspace_bytes(int frames, int H, int W);
int rmem_png_encode_labels(const unsigned char* labels, int frames, int H, int W, const unsigned char* lut /* device, 256 bytes, or NULL */,
                           void* workspace, unsigned char* out, long long* offsets, void* stream);

/* Palette-PNG annotations: the inverse direction.  One zlib stream per frame (the concatenated IDAT payloads of a PNG file) in, uint8
 * label maps out[frames][H][W] (contiguous, device) out, in one call on `stream`, no host sync, no state kept between calls.
 * bits: the streams packed back to back by the host (rmem_ocu_amd/png.py PackedPngs) -- every stream starts on an 8-byte boundary of
 * an 8-byte aligned buffer and is followed by at least 8 zero bytes; descs[f] (device) says where stream f lies and how its samples
 * are stored.  Only the compressed bytes and the descriptors cross PCIe; the chunk walk and the chunk CRC-32s stay on the host.
 * Accepted: non-interlaced PNG of colour type 3 (indexed) at bit depth 1, 2, 4 or 8, or colour type 0 (grey) at bit depth 8; all
 *   frames of a call share H and W, depth and colour type are per frame.  zlib: CM = 8, CINFO <= 7, no preset dictionary.  DEFLATE:
 *   stored, fixed and dynamic blocks in any number and mix, distances up to 32768, lengths up to 258, overlapping copies.  All five
 *   row filters (the filter unit is one byte for every accepted format).  Samples below 8 bits are unpacked most significant bits
 *   first; a row's padding bits are ignored.
 * lut: 256 device bytes applied to every sample (palette index or grey value, e.g. 255 -> 1), or NULL.
 * status (device, int [frames]) is written for every frame by the call, 0 = decoded and its Adler-32 verified.  A frame whose
 * status is not zero is zero-filled in `out`: every byte of out is written by every call.  The first error ends a stream, so one
 * bit is set:
 *   ST_INPUT   the stream needs more bits than it has (reads beyond its end return zero and touch no memory)
 *   ST_SIZE    the inflated bytes would exceed, or end short of, H * (1 + ceil(W * depth / 8))
 *   ST_RANGE   a match reaches back before the first byte
 *   ST_CODE    block type 3, stored LEN != ~NLEN, HLIT > 286 or HDIST > 30, an over-subscribed or (other than zlib's single
 *              one-bit code) incomplete code, no end-of-block code, a repeat with no previous length or running over HLIT + HDIST,
 *              a bit pattern that is no code, literal/length symbol 286 / 287, distance symbol 30 / 31
 *   ST_HEADER  CM != 8, CINFO > 7, FCHECK wrong, FDICT set
 *   ST_ADLER   the Adler-32 of the inflated bytes differs from the trailer
 *   ST_FILTER  a row's filter type is above 4
 *   ST_DESC    a descriptor outside the accepted formats, or a misaligned offset
 * workspace: rmem_png_decode_workspace_bytes bytes, 16-byte aligned: the inflated (filtered) bytes of every frame, sized for depth 8.
 * Replaces dataloaders/eval_datasets.py (Image.open of an annotation file, np.array, one host-to-device copy of H * W bytes per
 * frame). */
typedef struct RmemPngDesc {
  long long offset;     /* of the stream in bits, a multiple of 8 */
  long long bytes;      /* of the stream (without the padding) */
  int bit_depth;        /* 1, 2, 4, 8 */
  int colour_type;      /* 3, or 0 with bit depth 8 */
} RmemPngDesc;
#define RMEM_PNG_ST_INPUT 1
#define RMEM_PNG_ST_SIZE 2
#define RMEM_PNG_ST_RANGE 4
#define RMEM_PNG_ST_CODE 8
#define RMEM_PNG_ST_HEADER 16
#define RMEM_PNG_ST_ADLER 32
#define RMEM_PNG_ST_FILTER 64
#define RMEM_PNG_ST_DESC 128
size_t rmem_png_decode_workspace_bytes(int frames, int H, int W);   /* host only, 0 on bad geometry (H * W <= 2^26) */
int rmem_png_decode_labels(const unsigned char* bits, const RmemPngDesc* descs /* device */, int frames, int H, int W,
                           const unsigned char* lut /* device, 256 bytes, or NULL */, void* workspace,
                           unsigned char* out /* device [frames][H][W] */, int* status /* device [frames] */, void* stream);

/* COCO run-length masks (maskApi.c's compressed RLE, the 'counts' of {'size': [H, W], 'counts': ...}), written from a uint8 label
 * stack labels[frames][H][W] (contiguous, device, may start at any byte): one string per (frame, id), id = 1..num_ids; pixels with
 * any other value belong to no mask.  One call on `stream`, no host sync, no state kept between calls; whatever must be zero is
 * zeroed on the stream inside the call.
 * The format: a binary mask is read column-major (position j = x * H + y); counts are the lengths of the alternating runs, zeros
 *   first (the first count is 0 when pixel (0, 0) is set), the last run always emitted (empty mask: [H*W], full: [0, H*W]).  Count
 *   i is x = counts[i], minus counts[i-2] when i > 2 (not >= 2); then repeat c = x & 0x1f, x >>= 5 (arithmetic), more = (c & 0x10)
 *   ? x != -1 : x != 0, c |= 0x20 when more, emit c + 48: characters 48..111, at most 6 per count since H * W <= 2^26.
 * The strings are packed back to back, frame-major: string (f, k) is out[offsets[f * num_ids + k - 1] : offsets[f * num_ids + k]);
 * offsets (device, int64 [frames * num_ids + 1]) starts at 0 and grows strictly (every string has at least one byte).  Sizes are
 * computed exactly before anything is written: offsets is always complete and exact.  When offsets[frames * num_ids] > capacity
 * (the bytes out holds) nothing is written to out and status[0] (device, int32) is RMEM_RLE_ST_CAPACITY; otherwise it is 0.
 * The bytes are reproducible: the only atomics are integer adds on counters that one thread owns.
 * workspace: rmem_rle_workspace_bytes bytes, 16-byte aligned: boundary counters per (frame, id, column, block of 128 rows), the
 * boundary positions (2 H W int32 per frame, the worst case) and per-string totals.
 * Refused (non-zero, nothing launched): null pointers, frames outside 1..65535, non-positive H / W, H * W above 2^26, num_ids
 * outside 1..255, capacity below 0, a misaligned workspace.
 * Replaces stack.cpu() and a host transpose plus run-length pass per frame and object (pycocotools' encode). */
#define RMEM_RLE_ST_CAPACITY 1
size_t rmem_rle_workspace_bytes(int frames, int H, int W, int num_ids);   /* host only, 0 on bad geometry */
int rmem_rle_encode_labels(const unsigned char* labels, int frames, int H, int W, int num_ids, void* workspace, unsigned char* out,
                           long long capacity, long long* offsets /* device, int64 [frames * num_ids + 1] */,
                           int* status /* device, int32 [1] */, void* stream);

/* The inverse: nstrings run-length strings in, uint8 label maps labels[frames][H][W] (contiguous, device) out, in one call on
 * `stream`, no host sync, no state kept between calls.  bits: total_bytes bytes on the device that hold the strings; descs[s]
 * (device) says where string s lies, which frame it belongs to and which label value (1..255) its mask paints.  Strings are listed
 * frame by frame (frames never decrease along descs) and their byte ranges do not overlap (each string's counts are kept in the
 * workspace at its own offset).  Every byte of labels is written by the call; pixels under no mask are 0; where masks of one frame
 * overlap, the string listed later wins (label[mask] = value in listing order).
 * Reading a string: 5 bits per character, little end first, continuation bit 0x20, sign extension from bit 0x10 of a count's last
 * character, counts[m-2] added once m > 2; the counts must be >= 0 and add up to H * W.
 * status (device, int32 [nstrings]) is written for every string, 0 = painted.  A string with a non-zero status paints nothing and is
 * never read or written out of range:
 *   ST_CHAR       a byte outside 48..111
 *   ST_TRUNCATED  the string ends inside a count (its last character has the continuation bit)
 *   ST_LONG       a count of more than 6 characters
 *   ST_NEGATIVE   a count below 0
 *   ST_SUM        the counts do not add up to H * W
 *   ST_DESC       frame outside 0..frames-1 or below the frame of the string before, value outside 1..255, or a range outside bits
 * CHAR, TRUNCATED and LONG end the reading of a string; NEGATIVE and SUM are looked for only in strings without them.
 * workspace: rmem_rle_decode_workspace_bytes bytes, 16-byte aligned: one int32 per byte of bits, 16 + 4 W bytes per string (the run
 * at the top of every column), 8 per frame.
 * Refused (non-zero, nothing launched): null pointers, total_bytes outside 0..2^31-1, nstrings outside 1..65535*255, frames outside
 * 1..65535, non-positive H / W, H * W above 2^26, a misaligned workspace.
 * Replaces pycocotools' decode per mask on the host and the upload of H * W bytes per frame. */
typedef struct RmemRleDesc {
  int frame;            /* 0..frames-1 */
  int value;            /* 1..255: the label the mask paints */
  long long offset;     /* of the string in bits */
  int length;           /* of the string in bytes */
} RmemRleDesc;
#define RMEM_RLE_ST_CHAR 1
#define RMEM_RLE_ST_TRUNCATED 2
#define RMEM_RLE_ST_LONG 4
#define RMEM_RLE_ST_NEGATIVE 8
#define RMEM_RLE_ST_SUM 16
#define RMEM_RLE_ST_DESC 32
size_t rmem_rle_decode_workspace_bytes(long long nstrings, long long total_bytes, int frames, int W);   /* host only, 0 on bad arguments */
int rmem_rle_decode_labels(const unsigned char* bits, long long total_bytes, const RmemRleDesc* descs /* device */, int nstrings, int frames,
                           int H, int W, void* workspace, unsigned char* labels /* device [frames][H][W] */,
                           int* status /* device [nstrings] */, void* stream);

/* Baseline-JPEG files written on the device: uint8 RGB frames rgb[frames][H][W][3] (contiguous, device) in, complete .jpg files
 * packed back to back out, in one call on `stream`, no host sync, no state kept between calls.  File f is
 * out[offsets[f] : offsets[f+1]) (offsets: device, int64 [frames + 1], starts at 0); out holds frames * rmem_jpeg_encode_bound(H, W)
 * bytes.  With labels (uint8 [frames][H][W], device) the overlay of rmem_overlay_rgb8 is applied to every pixel as it is read; the
 * overlaid frames are never written to memory.  The counterpart of rmem_jpeg_decode_batch; replaces a host copy of the frames, a
 * numpy blend and Pillow's Image.save per frame (the reference's demo / overlay script).
 * A file is SOI, APP0 (JFIF 1.01), two DQT, SOF0, four DHT, DRI (unless restart_rows is 0), SOS, the entropy-coded segment, EOI.
 * The segment is libjpeg-turbo's bit for bit (Pillow: Image.save(f, 'JPEG', quality=q, subsampling=2, optimize=False,
 * restart_marker_rows=restart_rows)):
 *   Colour (jccolor.c):  Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *                        Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *                        Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   Sampling: 4:2:0 only, Y 2x2, Cb and Cr 1x1.  Per component cw = ceil(W h / 2), ch = ceil(H v / 2), wib = ceil(cw / 8) and
 *     hib = ceil(ch / 8) real blocks; the MCU grid has ceil(W / 16) x ceil(H / 16) MCUs of Y00 Y01 Y10 Y11 Cb Cr.
 *   Edges: luma is replicated to the right up to 8 wib columns and downwards up to 8 hib rows.  Chroma at full resolution is
 *     replicated to the right up to 16 wib columns and downwards by at most one row (to an even height), then averaged (jcsample.c
 *     h2v2): (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... by output column; the averaged rows are replicated down to 8 hib.
 *   FDCT: jfdctint.c (ISLOW) on sample - 128, CONST_BITS 13, PASS1_BITS 2, rows first, then columns.
 *   Quantisation: d = 8 Q[k], q = (|c| + (d >> 1)) / d, sign restored.  Q: Annex K's luminance and chrominance tables scaled as
 *     jpeg_quality_scaling does (s = 5000 / quality below 50, else 200 - 2 quality; entry = (base s + 50) / 100 clamped to 1..255).
 *   Dummy blocks (jccoefct.c): luma blocks of the MCU grid to the right of wib or below hib are not transformed: their ACs are zero
 *     and their DC is the DC of the block before them in the MCU (which may itself be a dummy).
 *   Entropy coding: Annex K's four Huffman tables; the DC difference per component, the predictor reset at every restart interval;
 *     ZRL (0xF0) for every 16 zeros inside a run, EOB (0x00) when a block ends in zeros; an interval is padded to a byte with
 *     1-bits; every 0xFF data byte is followed by 0x00; RSTm with m = interval index mod 8 between intervals, none after the last.
 *   Restart interval: restart_rows MCU rows, DRI = restart_rows * ceil(W / 16) <= 65535; 0 = one interval per frame, no DRI segment.
 * rmem_jpeg_encode_header (host only): the header bytes (header may be NULL: *header_bytes alone is set) and the table blob the
 * device calls read (RMEM_JPEG_ENC_TABLE_BYTES bytes, copied to the device by the caller): the divisors 8 Q, code and length of
 * every Huffman symbol, restart_rows and the header itself.  It depends on (H, W, quality, restart_rows) alone.
 * rmem_jpeg_encode_bound (host only, 0 on bad geometry): the most bytes one file can take.  A block costs at most 22 + 63 * 26 bits
 * = 208 bytes (DC: an 11-bit code and 11 value bits; each AC: a 16-bit code and 10 value bits), every byte of the segment may be
 * 0xFF and be followed by 0x00, every interval pads to a byte and is followed by a 2-byte marker, at most one interval per MCU row:
 *   bound = RMEM_JPEG_ENC_HEADER_MAX + 2 * 208 * 6 * MCUs + 4 * ceil(H / 16) + 2.
 * workspace: rmem_jpeg_encode_workspace_bytes bytes (0 on bad geometry), 16-byte aligned: int16 coefficients in scan and zig-zag
 * order, bit counts, and the unstuffed bits of every interval at its worst-case distance (untouched memory beyond what is used).
 * Limits, refused with a reason before anything is launched: 1 <= H, W <= 65535, H * W <= 2^26, quality 1..100, frames <= 65535. */
#define RMEM_JPEG_ENC_HEADER_MAX 629
#define RMEM_JPEG_ENC_TABLE_BYTES 4096
int rmem_jpeg_encode_header(int H, int W, int quality, int restart_rows, unsigned char* header, int capacity, int* header_bytes,
                            void* tables /* host, RMEM_JPEG_ENC_TABLE_BYTES bytes, or NULL */);
size_t rmem_jpeg_encode_bound(int H, int W);
size_t rmem_jpeg_encode_workspace_bytes(int frames, int H, int W);
int rmem_jpeg_encode_rgb8(const unsigned char* rgb, const unsigned char* labels /* device, or NULL: no overlay */,
                          const unsigned char* palette /* device, 768 bytes; may be NULL without labels */, int alpha256, int frames,
                          int H, int W, const void* tables /* device: the blob of rmem_jpeg_encode_header for this H, W */,
                          void* workspace, unsigned char* out, long long* offsets, void* stream);
/* The overlay alone: out_rgb[frames][H][W][3].  For a pixel p with label l = labels[p] and m the largest label among its
 * 4-neighbours inside the image:  m > l: black (a one-pixel contour just outside every object; between two touching objects on the
 * side of the smaller id, as painting the objects in ascending id gives);  else l != 0:
 * out_c = (a rgb_c + (256 - a) palette[3 l + c] + 128) >> 8 with a = alpha256 in 0..256;  else the pixel unchanged.  Integer
 * arithmetic throughout; in the manner of the reference's demo overlay, which blends in floating point (no bit parity claimed). */
int rmem_overlay_rgb8(const unsigned char* rgb, const unsigned char* labels, const unsigned char* palette /* device, 768 bytes */,
                      int alpha256, int frames, int H, int W, unsigned char* out_rgb, void* stream);

/* ------------------------------------------------------------------ stream capture helpers
 * Thin wrappers over hipStreamBeginCapture / hipGraphInstantiate / hipGraphLaunch so the Python host
 * can replay one frame's launch sequence as a hipGraph. */
int rmem_graph_begin(void* stream);
int rmem_graph_end(void* stream, void** graph_exec_out);
int rmem_graph_launch(void* graph_exec, void* stream);
int rmem_graph_destroy(void* graph_exec);


/* ------------------------------------------------------------------ IEEE-half flavour
 * Every entry point above that takes 16-bit operands ("bf16" pointers: activations, weights, bank entries) exists a second time
 * with the suffix _f16: identical signature, layout and semantics, but the 16-bit element type is IEEE binary16 instead of
 * bfloat16 (accumulation, residual streams and all statistics stay fp32).  This is the operand type of the reference's --amp
 * path (tools/eval.py:45-47: torch.cuda.amp.autocast) and of BASELINE cfg 5; with 11 significant bits instead of 8 it is also the
 * flavour that reaches >= 0.999 mask IoU against the fp32 reference.  Differences: the memory-read kernel
 * always runs its online-softmax pass (P = exp2(S - m) must stay below 2^16), and values beyond +-65504 overflow, as under
 * autocast.  Element-type-agnostic entry points (workspace sizes, fp32 / uint8 post-processing, copies, graphs, timers) have no twin. */
int rmem_conv2d_nhwc_f16(const rmem_conv_desc* desc, const void* x, const void* w, const float* bias, const void* residual, void* y, void* y2, void* workspace, void* stream);
int rmem_mem_read_attn_f16(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv, const rmem_attn_chunk* chunks, int nchunks, int lk_single, const float* pe_cur, const float* pe_mem, int Lq, int heads, void* out, int ldo, float* attn_mass, int T, void* workspace, void* stream);
int rmem_mem_read_attn_clips_f16(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv, const rmem_attn_chunk* chunks, int nchunks, int lk_single, const float* pe_cur, const float* pe_mem, int Lq, int heads, void* out, int ldo, float* attn_mass, int T, int nclips, long long q_clip_stride, long long kv_clip_stride, long long out_clip_stride, void* workspace, void* stream);
int rmem_lstt_attn_pair_clips_f16(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv, const rmem_attn_chunk* chunks, int nchunks, int lk_total, const float* pe_cur, const float* pe_mem, int Lq, int heads, void* out_long, int ldo, float* attn_mass, int T, int nclips, long long q_clip_stride, long long out_clip_stride, const void* k_short, const void* v_short, int lk_short, long long kv_short_clip_stride, void* out_short, long long out_short_clip_stride, void* workspace, void* stream);
int rmem_lstt_attn_pair_clips_deferred_f16(const void* q, int ldq, const void* k_bank, const void* v_bank, long long slot_stride, int ldkv, const rmem_attn_chunk* chunks, int nchunks, int lk_total, const float* pe_cur, const float* pe_mem, int Lq, int heads, void* out_long, int ldo, float* attn_mass, int T, int nclips, long long q_clip_stride, long long out_clip_stride, const void* k_short, const void* v_short, int lk_short, long long kv_short_clip_stride, void* out_short, long long out_short_clip_stride, void* workspace, rmem_attn_merge* merge, void* stream);
int rmem_layernorm256_f16(const void* a, int a_is_f32, int lda, const void* b, int b_is_f32, int ldb, const float* gamma, const float* beta, float eps, int M, void* y_bf16, int ldy, const float* pos, void* ypos_bf16, int ldyp, float* y_f32, int ldyf, void* stream);
int rmem_layernorm_f16(const void* a, int a_is_f32, int lda, const float* gamma, const float* beta, float eps, int M, int C, void* y_bf16, int ldy, float* y_f32, int ldyf, void* stream);
int rmem_patch_merge_ln_f16(const float* x, int H, int W, int C, const float* gamma, const float* beta, float eps, void* y_bf16, void* stream);
int rmem_window_attn_f16(const void* qkv, const float* qkv_bias, const float* bias_mask_table, void* out, int H, int W, int C, int heads, int shift, void* stream);
int rmem_window_attn_images_f16(const void* qkv, const float* qkv_bias, const float* bias_mask_table, void* out, int images, int H, int W, int C, int heads, int shift, void* stream);
int rmem_patch_merge_ln_images_f16(const float* x, int images, int H, int W, int C, const float* gamma, const float* beta, float eps, void* y_bf16, void* stream);
int rmem_add16_f16(const void* a, const void* b, void* y, long long n, void* stream);
int rmem_add16_grouped_f16(int n, const void* const* a, const void* const* b, void* const* y, long long count, void* stream);
int rmem_lstt_chain_a_f16(const rmem_chain_a_desc* d, void* stream);
int rmem_lstt_chain_b_f16(const rmem_chain_b_desc* d, void* stream);
int rmem_lstt_chain_b_merged_f16(const rmem_chain_b_desc* d, const rmem_attn_merge* merge, void* stream);
int rmem_lstt_chain_c_f16(const rmem_chain_c_desc* d, void* stream);
int rmem_layernorm256_pair_f16(const void* a0, const void* b0, void* y0, const void* a1, const void* b1, void* y1, const float* gamma, const float* beta, float eps, int M, void* stream);
int rmem_bneck_block64_f16(const rmem_bneck_block_desc* desc, const void* x, const void* w1, const float* bias1, const void* w2, const float* bias2, const void* w3, const float* bias3, void* y, const void* w1n, const float* bias1n, void* a_next, void* stream);
int rmem_bneck_chain_f16(const rmem_bneck_chain_desc* desc, const void* b, const void* x2, const void* w3, const float* bias3, const void* res, void* y, const void* w1, const float* bias1, void* a2, void* stream);
int rmem_conv1x1_dual_nhwc_f16(const rmem_conv_desc* desc, const void* x, const void* x2, int H2, int W2, int Cin2, int stride2, const void* w_cat, const float* bias, void* y, void* stream);
int rmem_linear_grouped_f16(const rmem_conv_desc* desc, int n, const void* const* x, const void* const* w, const float* const* bias, const void* const* residual, void* const* y, void* stream);
int rmem_groupnorm_nhwc_f16(const void* x, int M, int C, int groups, const float* gamma, const float* beta, float eps, int act, void* y, float* workspace, void* stream);
int rmem_groupnorm_f32_nhwc_f16(const float* x, int M, int C, int groups, const float* gamma, const float* beta, float eps, int act, void* y, float* workspace, void* stream);
int rmem_groupnorm_nhwc_images_f16(const void* x, int images, int M, int C, int groups, const float* gamma, const float* beta, float eps, int act, void* y, float* workspace, void* stream);
int rmem_groupnorm_head_nhwc_images_f16(const void* x, int images, int M, int C, int groups, const float* gamma, const float* beta, float eps, int act, const void* w, const float* bias, int N, float* y, int ldy, float* workspace, void* stream);
int rmem_gn_act_dwconv5x5_nhwc_images_f16(const void* x, int images, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, int act, const float* w_t, void* y, float* workspace, void* stream);
int rmem_gn_act_dwconv5x5_prestats_nhwc_images_f16(const void* x, int images, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, int act, const float* w_t, void* y, const float* stats, void* stream);
int rmem_gn_act_dwconv5x5_nhwc_f16(const void* x, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps, int act, const float* w_t, void* y, float* workspace, void* stream);
int rmem_dwconv5x5_nhwc_f16(const void* x, const float* w_t, void* y, int H, int W, int C, void* stream);
int rmem_image_ptrs_to_nhwc4p_f16(const float* const* img_ptrs, void* out_padded, int images, int H, int W, void* stream);
int rmem_conv3x3_direct_f16(const void* x, int images, int H, int W, int C, const void* w, const float* bias, int relu, void* y, void* stream);
int rmem_conv3x3_c64_direct_f16(const void* x, int images, int H, int W, const void* w, const float* bias, void* y, void* stream);
int rmem_stem7x7s2_pool_f16(const void* x_padded, int images, int H, int W, const void* w, const float* bias, void* y_pooled, void* stream);
int rmem_stem7x7s2_f16(const void* x_padded, int images, int H, int W, const void* w, const float* bias, void* y, void* stream);
int rmem_image_ptrs_to_nhwc8_f16(const float* const* img_ptrs, void* out, int images, int H, int W, void* stream);
int rmem_image_to_nhwc8_f16(const float* img_chw, void* out, int H, int W, void* stream);
int rmem_image_to_nhwc8_images_f16(const float* img_chw, void* out, int images, int H, int W, void* stream);
int rmem_ingest_rgb8_f16(const unsigned char* rgb_hwc, int Hs, int Ws, int Hd, int Wd, float* out_chw, void* out_nhwc8, void* stream);
int rmem_maxpool3x3s2_nhwc_f16(const void* x, void* y, int H, int W, int C, void* stream);
int rmem_maxpool3x3s2_nhwc_images_f16(const void* x, void* y, int images, int H, int W, int C, void* stream);
int rmem_bilinear_nhwc_f16(const void* x, void* y, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);
int rmem_bilinear_nhwc_images_f16(const void* x, void* y, int images, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);
int rmem_label_id_embed_f16(const void* label, int label_is_f32, int images, int Hs, int Ws, int H, int W, int KH, int KW, int stride, int pad, int num_classes, const void* w, const float* bias, void* label_scratch_u8, void* out, void* stream);
int rmem_label_to_onehot16_f16(const void* label, int label_is_f32, int Hs, int Ws, int Hd, int Wd, int num_classes, void* out, void* stream);
int rmem_label_to_onehot16_images_f16(const void* label, int label_is_f32, int images, int Hs, int Ws, int Hd, int Wd, int num_classes, void* out, void* stream);
int rmem_gated_attn_f16(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank, long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames, int keys_per_frame, const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, float* attn_mass, const float* dw_w_t, int H, int W, void* workspace, void* stream);
int rmem_local_gated_attn_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel, int ldrel, int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, const float* dw_w_t, void* workspace, void* stream);
int rmem_gated_attn_clips_f16(const void* q, int ldq, const void* k_bank, long long k_slot_stride, int ldk, const void* v_bank, long long v_slot_stride, int ldv, const rmem_attn_chunk* chunks, int nchunks, int frames, int keys_per_frame, const float* pe_cur, const float* pe_mem, int Lq, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, float* attn_mass, const float* dw_w_t, int H, int W, int nclips, void* workspace, void* stream);
int rmem_local_gated_attn_clips_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* rel, int ldrel, int H, int W, int DV, const void* u_a, int ldua, const void* u_b, int ldub, int usplit, void* out, int ldo, const float* dw_w_t, int nclips, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RMEM_H_ */
