/* C ABI of libtransfuser_hip.so - the MI355X (gfx950) kernels of the TransFuser training hot path.
 *
 * The reference (autonomousvision/transfuser) has no FFI / plugin layer: its native work is done
 * by third-party wheels (cuDNN/cuBLAS through torch 1.11, mmcv, torch_scatter).  Each entry point
 * below names the reference call site(s) whose arithmetic it replaces (file:line relative to the
 * reference repo).  Conventions:
 *   - every function returns 0 on success, non-zero on error; tf_last_error() gives the text;
 *   - all pointers are device pointers borrowed for the duration of the call; nothing is
 *     allocated, freed or retained; launches are asynchronous on `stream` (a hipStream_t);
 *     no entry point synchronises the device, so all of them are hipGraph-capturable;
 *   - activations are NHWC ("channels-last") fp32; conv weights are (Cout, kh, kw, Cin/groups),
 *     i.e. the channels_last physical layout of a torch (Cout, Cin/g, kh, kw) parameter;
 *   - token / linear tensors are row-major (rows, features).
 */
#ifndef TRANSFUSER_HIP_H
#define TRANSFUSER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tf_version(void);
const char* tf_last_error(void);
/* Provenance of a shipped library: the first 16 hex digits of the sha256 over the sources it was compiled from (transfuser_amd/csrc/*.cpp,
 * *.h and this header, sorted by file name; written into the compile line by transfuser_amd/build.py).  The reference has no counterpart
 * (it ships no native code); the Python binding compares it with the sources beside the library (transfuser_amd/_lib.py:load). */
const char* tf_build_id(void);
/* Stream-K GEMM launches issued by this process so far (diagnostics / tests: a pinned stream-K plan silently falls back to the data-parallel
 * launch when the call carries no scratch or the tile count divides evenly). */
long tf_streamk_launches(void);
/* 16-byte epilogue of the register-staged GEMM engine (transposed accumulator; the reference's cuBLAS / cuDNN epilogues behind
 * transfuser.py:380,442,539-549 have no such knob).  TF_GEMM_EPI16=0 in the environment keeps every launch on the 4-byte epilogue.
 * tf_gemm_epi16(0 | 1) sets the switch, tf_gemm_epi16(-1) re-reads the environment; both return the value now in force (tests).
 * tf_gemm_epi16_launches(): launches configured with the 16-byte epilogue so far - a query, it changes no result: a call that is not
 * eligible (alignment, N % 4, atomic mode, tiling) silently takes the 4-byte epilogue and leaves the counter alone. */
int tf_gemm_epi16(int on);
long tf_gemm_epi16_launches(void);
/* Deterministic mode (the counterpart of torch.use_deterministic_algorithms, which the reference leaves off: train.py:115 only turns on
 * cudnn.benchmark).  Process-wide, read on the host at launch time like tf_set_precision - so a captured graph keeps the forms it was
 * captured with.  On: every reduction that by default ends in fp32 atomics (the k-split weight gradients of the MFMA engine, the grouped 3x3
 * weight gradient, LayerNorm dgamma / dbeta, the SE excitation backward, the small-M input gradient, the skinny weight gradient, the opt-in
 * atomic BatchNorm / column sums) takes a fixed-order form whose result is a pure function of its inputs and the GEMM plan; an entry without
 * such a form returns an error that names this flag instead of running atomics (tf_dwconv7_wgrad_f32; tf_layernorm_bwd_f32 /
 * tf_layernorm_bwd_drop_f32 when asked for dgamma / dbeta: use tf_layernorm_bwd_dw_f32).  Scratch for these forms is the caller's, per call:
 * tf_gemm_desc.splitk_ws (tf_gemm_splitk_ws_floats), tf_conv2d_wgrad_ws_f32, tf_se_excite_bwd_ws_floats, the reduction workspace.  Off
 * (default): every launch is exactly what it was.  tf_set_deterministic returns 0; tf_get_deterministic the flag. */
int tf_set_deterministic(int on);
int tf_get_deterministic(void);
/* Launches so far of kernel forms that combine partial results with float atomics (the engine's atomic k-split counts only when the launch
 * really runs with the atomic epilogue) - tests assert that it stands still under tf_set_deterministic(1) and moves without it. */
long tf_float_atomic_launches(void);
/* Launches so far of the ordered slab k-split of the MFMA engine: under tf_set_deterministic(1) a plan that would split K with the atomic
 * epilogue has slice s store its raw partial tile at splitk_ws + s * m * round_up(n, 4) and a fix-up kernel add the slices to C in slice order. */
long tf_slab_splitk_launches(void);

/* GEMM tiling plans.  The reference turns on cudnn.benchmark (train.py:115); the equivalent here: while tf_autotune(1)
 * is on (eager warm-up, NOT during graph capture - it synchronises), the first call of every distinct
 * (entry point, M, N, K, batch) times the candidate tilings with HIP events and caches the winner.  Plans can be
 * saved to / loaded from a text file (tf_plans_load returns the number of plans read). */
/* Compute precision of every MFMA-engine contraction (GEMMs and implicit-GEMM convolutions): 0 = exact fp32 MFMA (the reference's
 * arithmetic, config.py:55 trains fp32; default), 1 = operands rounded to bf16 (RNE) on the LDS->register path and multiplied on the bf16
 * MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulation, fp32 storage of activations / weights / gradients - the MI355X counterpart of
 * torch.autocast(bfloat16) with fp32 master weights (BASELINE configs[2]); 3 = the same with IEEE-half operands (v_mfma_f32_32x32x16_f16,
 * BASELINE configs[4]; pair it with a loss scale, tf_adamw_scaled_f32).  Tuned plans are kept per precision (3 shares the plans of 1). */
int tf_set_precision(int mode);
int tf_get_precision(void);
int tf_autotune(int enable);
/* The integer `splitk` of tf_force_plan / tf_force_dma and of the 10th field of a plan file (tf_plans_load / tf_plans_save) encodes how the
 * plan partitions K: 1 = no k-split; 2 .. 999999 = that many k-slices added into C with fp32 atomics (pure accumulations only; under
 * tf_set_deterministic(1) the same slices through the ordered slab split); 1000000 + S = two-pass split with S = 2..4 slices through
 * tf_gemm_desc.splitk_ws (LDS-DMA configurations only); 2000000 = stream-K (LDS-DMA configurations only; needs splitk_ws and sk_flags).  A call
 * that cannot take its plan's partition runs unsplit.  Inside the library the encoding exists in one decode / encode pair (csrc/api.cpp). */
int tf_force_plan(int bm, int bn, int bk, int splitk); /* tests: pin one tiling of the register-staged kernel (bm = 0 clears) */
int tf_force_dma(int kind, int splitk);                /* tests: pin LDS-DMA configuration `kind` (1..8, tf_gemm_dma.h) for every eligible call */
int tf_plans_count(void);
int tf_plans_clear(void);
int tf_plans_save(const char* path);
int tf_plans_load(const char* path);

/* ---- dense contractions (fp32 MFMA, LDS-tiled) --------------------------------------------- */

/* C[z] (op)= alpha * A[z] . B[z] (+bias[col]) (+res) (relu).  Replaces nn.Linear fwd/dgrad/wgrad
 * (transfuser.py:500-507,539-541; model.py:592-605), the attention score / context bmm
 * (transfuser.py:519-523) and every 1x1 convolution on NHWC maps (timm RegNetY conv1/conv3,
 * transfuser.py:92-109).
 *   a_trans = 0: A(i,k) = a[i*lda + k]   a_trans = 1: A(i,k) = a[k*lda + i]
 *   b_trans = 0: B(k,j) = b[j*ldb + k]  (torch Linear / conv weight [out][in])
 *   b_trans = 1: B(k,j) = b[k*ldb + j]
 *   batch z in [0,batch): offset = (z / inner) * s?_outer + (z % inner) * s?_inner
 *   accumulate: 0 store, 1 C += (split-K with fp32 atomics may be used)
 *   splitk_ws / splitk_ws_floats: optional caller-owned scratch (stream-ordered with this call).  When given, GEMMs whose output has too few
 *   tiles to fill the 256 CUs (e.g. the GPT-4 [1740 x 6048] . [6048 x 1512] MLP contraction: 168 tiles of 128 x 128) may run as a
 *   deterministic TWO-PASS split-K: S k-slices write partial tiles into the scratch, a fix-up kernel sums them in slice order and applies the
 *   epilogue (alpha, bias, residual, ReLU, mask, store / +=).  Needs S * m * round_up(n, 4) floats (S <= 4); NULL disables it.
 *   Under tf_set_deterministic(1) the same scratch carries the ordered slab k-split of the accumulating calls (any S: the slice count of the
 *   plan, lowered until S slices fit; without scratch the call runs unsplit) and the block partials of the skinny weight gradient. */
typedef struct {
    const float* a; const float* b; float* c; const float* bias; const float* res;
    int m, n, k;
    int a_trans, b_trans;
    int64_t lda, ldb, ldc, ldres;
    int batch, inner;
    int64_t sa_outer, sa_inner, sb_outer, sb_inner, sc_outer, sc_inner;
    float alpha; int relu; int accumulate;
    const float* mask; int64_t ldmask;   /* optional (batch == 1, store mode): c(i,j) is zeroed unless mask[i*ldmask + j] > 0 - the ReLU
                                          * mask of a backward GEMM (dX = (dY W) * [act > 0]) fused into the epilogue */
    float* splitk_ws; int64_t splitk_ws_floats;
    int* sk_flags;                       /* with splitk_ws: 2048 ints, ZERO on entry and left zero (caller-owned, persistent, one per stream): hand-over flags of the
                                          * stream-K plans - persistent workgroups split the (tile, k) space evenly when the tile count does not divide over the
                                          * resident slots (GPT-4: 672 tiles of 128 x 128 on 512 slots); NULL disables them */
    /* optional: train-mode BatchNorm statistics of the OUTPUT fused into the epilogue (timm ConvBnAct = bias-free conv + BatchNormAct2d,
     * transfuser.py:380,442; point_pillar.py:15-25 Linear + BatchNorm1d).  colstat: device buffer of >= 3 * n * ceil(m / 32) floats that
     * receives per-part Welford triples [part][{count, mean, M2}][n]; *colstat_nparts (HOST int, written before the call returns) = number
     * of parts written, 0 when the plan chosen for this call cannot produce them (the caller then reduces separately).  Needs batch == 1,
     * a_trans == 0, store mode, no residual / ReLU / mask.  Consumed by tf_bn_fwd_parts_f32. */
    float* colstat; int* colstat_nparts;
    /* nn.Dropout on the product before the residual is added (round 5; drop_seed NULL = off): c = res + dropout(alpha a b + bias), the
     * x + resid_drop(proj(...)) / x + mlp(...)[-1] of a transformer Block (transfuser.py:543-549) in the GEMM's own epilogue.  The mask is the one
     * tf_dropout_f32 / tf_dropout_add_f32 generate for (seed, site) over the contiguous (m, n) output, so the backward regenerates it with
     * tf_dropout_f32.  Needs batch 1, a plain store, ldc == n, a_trans == 0. */
    const uint32_t* drop_seed; uint32_t drop_site; float drop_p;
} tf_gemm_desc;
int tf_gemm_f32(const tf_gemm_desc* d, void* stream);
/* Floats of splitk_ws this call can use: 0 unless the cached (or about-to-be-tuned) plan of the call's shape is a two-pass split-K plan, so
 * the caller only allocates scratch for the few GEMMs that want it (the reference's addmm never needs caller scratch: torch's cuBLAS
 * workspace plays this role, transfuser.py:500-507,539-541). */
long tf_gemm_splitk_ws_floats(const tf_gemm_desc* d);   /* under tf_set_deterministic(1): also what the ordered slab k-split / the skinny weight gradient of this call want */
/* Pair launch: between tf_gemm_pair_begin() and tf_gemm_pair_end(stream) (same thread) up to TWO tf_gemm_f32 calls whose plan is a 64 x 64
 * register-staged tiling (batch 1, 16-byte aligned operands, no output statistics) are held back and issued by tf_gemm_pair_end: a weight
 * gradient ([tn]: a_trans && b_trans) + an input gradient ([nn]: b_trans) pair as ONE grid whose second problem's workgroups start as the first
 * one's retire; any other held call as its ordinary launch, in call order.  Calls that are not eligible launch immediately, as without the
 * bracket.  The two calls must be independent (neither reads what the other writes): the weight / input gradient of one layer, which torch
 * autograd issues back to back behind every Conv2d / Linear of the reference (transfuser.py:380,442,545-549).  tf_gemm_pair_count(0 | 1):
 * joint / single launches issued by tf_gemm_pair_end so far on this thread. */
int tf_gemm_pair_begin(void);
int tf_gemm_pair_end(void* stream);
long tf_gemm_pair_count(int singles);

/* 2-D convolution as implicit GEMM (im2col gather -> LDS -> MFMA): kernel 1x1 or 3x3, stride 1/2,
 * pad, groups.  Replaces cuDNN conv fwd/bwd of the RegNetY trunks (timm regnety_032 via
 * transfuser.py:380,442), Seg/Depth decoders (transfuser.py:221-237,256-272), CenterNet heads
 * (model.py:93-99) and pred_bev (model.py:581-585). */
typedef struct {
    int B, Hi, Wi, Cin, Ho, Wo, Cout, ksize, stride, pad, groups;
} tf_conv_geom;
int tf_conv2d_fwd_f32(const tf_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int relu, void* stream);
/* the same with the output's BatchNorm statistics fused into the epilogue (see tf_gemm_desc.colstat; colstat holds >= 3 * Cout * ceil(B Ho Wo / 32) floats) */
int tf_conv2d_fwd_colstat_f32(const tf_conv_geom* g, const float* x, const float* w, const float* bias, float* y, float* colstat, int* colstat_nparts,
                              void* stream);
int tf_conv2d_dgrad_f32(const tf_conv_geom* g, const float* dy, const float* w, float* dx, int accumulate, void* stream);
int tf_conv2d_wgrad_f32(const tf_conv_geom* g, const float* dy, const float* x, float* dw, int accumulate, void* stream);
/* tf_conv2d_wgrad_f32 with caller-owned scratch of ws_floats floats (tf_conv2d_wgrad_ws_floats(g); 0 / NULL allowed): under
 * tf_set_deterministic(1) the k-slices of the weight gradient go through it (ordered slab k-split) instead of fp32 atomics - without scratch
 * the call runs unsplit.  With the flag off it is tf_conv2d_wgrad_f32 and the query returns 0. */
int tf_conv2d_wgrad_ws_f32(const tf_conv_geom* g, const float* dy, const float* x, float* dw, int accumulate, float* ws, long ws_floats, void* stream);
long tf_conv2d_wgrad_ws_floats(const tf_conv_geom* g);

/* Direct LDS-tiled 3x3 / stride 1 / pad 1 convolutions for Cin, Cout <= 32 at large resolution (the last decoder layers,
 * transfuser.py:232-237,267-272, and their gradients): one read of the input instead of 9 im2col reads through L2.  NHWC activations,
 * weights (Cout, 3, 3, Cin) channels-last as everywhere.  dgrad/wgrad take the FORWARD conv's Cin / Cout.  wgrad needs
 * tf_conv3x3_small_wgrad_ws_floats() floats of scratch. */
int tf_conv3x3_small_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int relu, void* stream);
int tf_conv3x3_small_dgrad_f32(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout, int accumulate, void* stream);
long tf_conv3x3_small_wgrad_ws_floats(void);
int tf_conv3x3_small_wgrad_f32(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int accumulate, float* ws, void* stream);

/* ---- BatchNorm apply folded into its CONSUMERS (round 3; the conv2 -> BatchNormAct2d -> SEModule -> conv3 segment of every timm RegNetY
 * bottleneck, transfuser.py:380,442): z = max(x scale + shift, 0) is recomputed from the convolution output wherever it is needed - the SE
 * squeeze, the SE scale, the gate gradient, the BatchNorm backward's ReLU mask - and never written.  tf_bn_finalize_parts_f32 = the finalize half
 * of tf_bn_fwd_parts_f32 (coef_out = [scale | shift], 2 C floats owned by the caller: read again in the backward).  The *_parts entry points
 * leave / take [segment][chunk][C] chunk sums in the reduction workspace (nchunks is returned on the host); the excitation kernels finish them. */
int tf_bn_finalize_parts_f32(const float* parts, int nparts, int rows, int C, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float momentum, float eps, float* save_mean, float* save_invstd, float* coef_out, void* stream);
int tf_colsum_bnrelu_parts_f32(const float* x, const float* coef, int nseg, int rows_per_seg, int C, float* ws, int* nchunks, void* stream);
int tf_se_excite_fwd_parts_f32(const float* parts, int nchunks, float scale, const float* W1, const float* b1, const float* W2, const float* b2, int B, int C,
                               int Cr, float* s_out, float* g1, float* gate, float* bwd_scratch, void* stream);
int tf_se_scale_bn_fwd_f32(const float* x, const float* coef, const float* gate, float* y, int B, int HW, int C, void* stream);
int tf_se_gate_grad_parts_f32(const float* dy, const float* x, const float* coef, int B, int HW, int C, float* ws, int* nchunks, void* stream);
int tf_se_excite_bwd_parts_f32(const float* parts, int nchunks, const float* gate, const float* s, const float* g1, const float* W1, const float* W2, int B,
                               int C, int Cr, float* dW1, float* db1, float* dW2, float* db2, float* ds, float* scratch, int scratch_is_zero, void* stream);
int tf_bn_bwd_remask_f32(const float* dz, const float* x, const float* fwd_coef, int rows, int C, const float* gamma, const float* save_mean,
                         const float* save_invstd, float* dx, float* dgamma, float* dbeta, float* ws, void* stream);
/* tf_se_scale_bwd_x_f32 folded into tf_bn_bwd_remask_f32 (the BatchNorm in front of a timm SEModule, backward): the incoming gradient
 * dz = dy * sigmoid(gate[b][c]) + dmean[b][c] / HW is recomputed by the reduction and the apply pass instead of being written; x (B, HW, C). */
int tf_bn_bwd_remask_se_f32(const float* dy, const float* gate, const float* dmean, int B, int HW, int C, const float* x, const float* fcoef, const float* gamma,
                            const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta, float* ws, void* stream);

/* ---- ConvNeXt trunk pieces (timm 0.5.4 convnext_*: the re-labelling branch of ImageCNN / LidarEncoder, transfuser.py:395-416,457-471).
 * tf_dwconv7_fwd_f32: depthwise 7x7 / pad 3 (+ bias) on NHWC, weights (C, 7, 7) = the (C, 1, 7, 7) parameter; flip != 0 mirrors the taps = the
 * input gradient (bias ignored); accumulate: y += .  tf_dwconv7_wgrad_f32 ACCUMULATES dw (C, 7, 7) and dbias (optional).  GELU is the exact
 * (erf) form of nn.GELU.  tf_colscale_add_f32: y = res + gamma[c] x + beta[c] (each of gamma / beta / res optional): layer scale + shortcut,
 * conv bias.  tf_colsum_mul_f32: out[c] (+)= sum_r a[r][c] b[r][c] (layer-scale gradient). */
int tf_dwconv7_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, int flip, int accumulate, void* stream);
int tf_dwconv7_wgrad_f32(const float* dy, const float* x, float* dw, float* dbias, int B, int H, int W, int C, void* stream);   /* fp32 atomics over the row blocks, no fixed-order form: an error under tf_set_deterministic(1) */
int tf_gelu_fwd_f32(const float* x, float* y, int64_t n, void* stream);
int tf_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int tf_colscale_add_f32(const float* x, const float* gamma, const float* beta, const float* res, float* y, int64_t rows, int C, void* stream);
int tf_colsum_mul_f32(const float* a, const float* b, int rows, int C, float* out, int accumulate, float* ws, void* stream);
/* out_e[c] += sum_r x_e[r][c] for n <= 8 matrices with the same row count in ONE single-pass launch (no workspace, no finalize, bitwise
 * reproducible): the bias gradients of a transformer Block's four nn.Linear layers (transfuser.py:500-507,539-541).  C_e % 4 == 0, row strides
 * ld_e (floats) % 4 == 0, 16-byte aligned bases. */
int tf_colsum_multi_f32(int n, const float* const* xs, const int* Cs, const long* lds, float* const* outs, int rows, void* stream);

/* ---- 16-bit operand STORAGE path (BASELINE configs[2] "bf16", configs[4] "fp16 MFMA"; the reference trains fp32 only, config.py:55).
 * tf_cast16_f32: x (rows x cols fp32, row stride ldx) -> y16 (rows x cols, row stride ldy, pad columns zeroed) and / or y16t (cols x rows: the
 * TRANSPOSE, row stride ldyt % 8 == 0, rows zero-padded to a multiple of 8); dtype 1 = bf16, 2 = IEEE half, round to nearest even.
 * tf_gemm16_nt_f32: C (m x n fp32) (op)= alpha A16 (m x k) . B16 (n x k)^T with the fp32 epilogue of tf_gemm_f32 (bias, residual, ReLU, mask,
 * accumulate); k, lda, ldb % 8 == 0; dtype as above (+ 16 x kind pins LDS-DMA tile configuration kind = 1..8: tests / tuning).  With the transposed copies every contraction of a linear layer (transfuser.py:500-527,540-547:
 * y = x W^T, dx = dy W, dW = dy^T x) is such an NT product. */
int tf_cast16_f32(const float* x, int rows, int cols, int ldx, void* y16, int ldy, void* y16t, int ldyt, int dtype, void* stream);
/* The same copies of MANY matrices in one launch (round 5: every cached 16-bit linear weight after AdamW, train.py:316 optimizer.step()): a
 * DEVICE-resident table sorted by tile0 = the index of the item's first 64 x 64 tile in the launch (prefix sums of ceil(rows / 64) * ceil(cols / 64));
 * total_tiles = the sum.  Per item the rules of tf_cast16_f32 hold (the caller checks them: the table is device memory). */
typedef struct { const float* x; void* y16; void* y16t; int rows, cols, ldx, ldy, ldyt, tile0; } tf_cast16_item;
int tf_cast16_multi_f32(const tf_cast16_item* items_dev, int n_items, int total_tiles, int dtype, void* stream);
/* The four element-wise producers of a RegNetY Bottleneck's 1x1-convolution operands (timm Bottleneck behind transfuser.py:380,442) writing the 16-bit copies
 * themselves (round 5; 16-bit storage modes: conv1 / conv3 then run as tf_gemm16_nt_f32 products like the GPT linear layers).  y16 (rows x C, contiguous, may
 * be NULL) and y16t (C x rows8, row stride ldyt % 8 == 0, rows zero-padded to a multiple of 8, may be NULL) are bitwise tf_cast16_f32 of the fp32 kernel named
 * below; the fp32 output (y32 / dx32) may be NULL where only the 16-bit GEMMs read the result.  C % 4 == 0, every tensor 16-byte aligned, dtype 1 = bf16, 2 = half.
 *   tf_bn_apply16_f32      : y = x sc + sh (+ res) (ReLU), coef = [sc | sh] of tf_bn_finalize_parts_f32 - the apply pass of tf_bn_fwd_parts_f32 (block output)
 *   tf_se_scale_bn16_f32   : tf_se_scale_bn_fwd_f32 (conv3's input; x is (B, HW, C), gate (B, C))
 *   tf_bn_bwd16_f32        : tf_bn_bwd_f32 (the gradient entering conv3; + dres, dgamma / dbeta ACCUMULATED; ws of tf_workspace_bytes())
 *   tf_bn_bwd_remask16_f32 : tf_bn_bwd_remask_f32 (the gradient entering conv1) */
int tf_bn_apply16_f32(const float* x, const float* coef, const float* res, int relu, float* y32, int rows, int C, void* y16, void* y16t, int ldyt, int dtype, void* stream);
int tf_se_scale_bn16_f32(const float* x, const float* coef, const float* gate, int B, int HW, int C, void* y16, void* y16t, int ldyt, int dtype, void* stream);
int tf_bn_bwd16_f32(const float* dz, const float* z, const float* x, int rows, int C, const float* gamma, const float* save_mean, const float* save_invstd, float* dx32,
                    float* dres, float* dgamma, float* dbeta, float* ws, void* dx16, void* dx16t, int ldyt, int dtype, void* stream);
int tf_bn_bwd_remask16_f32(const float* dz, const float* x, const float* fcoef, int rows, int C, const float* gamma, const float* save_mean, const float* save_invstd,
                           float* dx32, float* dgamma, float* dbeta, float* ws, void* dx16, void* dx16t, int ldyt, int dtype, void* stream);
/* nn.LayerNorm whose outputs are ONLY those 16-bit copies (round 5): ln1 / ln2 of a Block in the 16-bit storage modes (transfuser.py:535-536,546-547),
 * == tf_cast16_f32(tf_layernorm_fwd_f32(x)) bitwise, without the fp32 tensor in between.  C % 4 == 0, C <= 2048, 16-byte aligned x / gamma / beta;
 * y16 (may be NULL): ldy % 4 == 0, 8-byte aligned; y16t (may be NULL): as tf_cast16_f32.  mean / rstd as tf_layernorm_fwd_f32 (kept for the backward). */
int tf_layernorm_fwd16_f32(const float* x, const float* gamma, const float* beta, void* y16, int ldy, void* y16t, int ldyt, float* mean, float* rstd,
                           int rows, int C, float eps, int dtype, void* stream);
int tf_gemm16_nt_f32(const void* a16, const void* b16, float* c, int m, int n, int k, int lda, int ldb, int ldc, const float* bias, const float* res, int ldres,
                     float alpha, int relu, int accumulate, const float* mask, int ldmask, int dtype, void* stream);
/* plain store + the BatchNorm statistics of the output (tf_gemm_desc.colstat semantics): the RegNetY 1x1 convolutions in the 16-bit storage modes */
int tf_gemm16_nt_colstat_f32(const void* a16, const void* b16, float* c, int m, int n, int k, int lda, int ldb, int ldc, int dtype, float* colstat,
                             int* colstat_nparts, void* stream);
/* dst[b][2 i][2 j][:] += src[b][i][j][:] (NHWC, C % 4 == 0): the scatter half of a 1x1 / stride-2 convolution's input gradient (the RegNet
 * downsample branches, timm Bottleneck via transfuser.py:380,442); the other half is a plain GEMM over the B Ho Wo output pixels. */
int tf_add_strided2_f32(const float* src, float* dst, int B, int Ho, int Wo, int C, int Hi, int Wi, void* stream);
/* im2col matrix of a dense 3x3 / stride 1 / pad 1 convolution on NHWC: cols (B H W, 9 C), K ordered like the (Cout, kh, kw, Cin) weight, zero padding.
 * For the few-row, deep-K convolutions at the head of the Seg / Depth decoders (transfuser.py:221-225, 256-260: 512 -> 128 at 8 x 22): the product then
 * runs as tf_gemm_f32 with its deterministic split-K (opt-in, ops: TF_IM2COL_GEMM=1). */
int tf_im2col3x3_f32(const float* x, float* cols, int B, int H, int W, int C, void* stream);

/* The same layer shape with a THIN output: Cin == 32, 1 <= Cout <= 7 (the decoders' last convolution, transfuser.py:237,272: 32 -> 7 / 32 -> 1
 * at 256 x 704).  The 9 taps are folded into the GEMM's N (forward) / K (dgrad) / M (wgrad) dimension, so the launches are bandwidth-bound like
 * the layer itself instead of costing a 32 -> 32 convolution.  dgrad: relu_mask (optional, same shape as dx) = the forward OUTPUT of the
 * preceding ReLU layer (this layer's input): dx is zeroed where it is <= 0, i.e. dx is already that layer's masked gradient.
 * wgrad: dbias (optional, Cout floats) is ALWAYS accumulated into; ws = tf_conv3x3_thin_wgrad_ws_floats() floats. */
int tf_conv3x3_thin_supported(int Cin, int Cout);
int tf_conv3x3_thin_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, void* stream);
int tf_conv3x3_thin_dgrad_f32(const float* dy, const float* w, const float* relu_mask, float* dx, int B, int H, int W, int Cin, int Cout, int accumulate,
                              void* stream);
long tf_conv3x3_thin_wgrad_ws_floats(void);
int tf_conv3x3_thin_wgrad_f32(const float* dy, const float* x, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout, int accumulate, float* ws,
                              void* stream);

/* Grouped 3x3 / stride 1 / pad 1 convolution with group width 24 (C / 24 groups of 24 -> 24 channels): the timm regnety_032 bottleneck
 * convolution (transfuser.py:380,442; timm 0.5.4 regnet.py Bottleneck.conv2) and its gradients as per-group direct kernels.  x, y, dy, dx:
 * NHWC (B, H, W, C); w / dw: (C, 3, 3, 24) = the channels-last storage of a (C, 24, 3, 3) parameter.  wgrad needs
 * tf_conv3x3_grouped_wgrad_ws_floats() floats of scratch.  Stride-2 grouped convolutions use tf_conv2d_*. */
int tf_conv3x3_grouped_fwd_f32(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, int relu, void* stream);
/* the same with the output's BatchNorm statistics: every block merges the Welford triples of the tiles it walks; colstat holds >= 3 * C *
 * tf_conv3x3_grouped_colstat_parts() floats, *colstat_nparts (host) receives the number of parts written */
int tf_conv3x3_grouped_colstat_parts(void);
int tf_conv3x3_grouped_fwd_colstat_f32(const float* x, const float* w, float* y, int B, int H, int W, int C, float* colstat, int* colstat_nparts, void* stream);
int tf_conv3x3_grouped_dgrad_f32(const float* dy, const float* w, float* dx, int B, int H, int W, int C, int accumulate, void* stream);
/* Input gradient of the STRIDE-2 (pad 1) grouped 3x3 convolution - the first block of every RegNetY stage - by sub-pixel decomposition: nine
 * tap products per dY pixel instead of nine masked taps per pixel of the 4x larger dX grid.  dy is (B, (Hi-1)/2+1, (Wi-1)/2+1, C), dx (B, Hi, Wi, C). */
int tf_conv3x3_grouped_s2_dgrad_f32(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int accumulate, void* stream);
long tf_conv3x3_grouped_wgrad_ws_floats(void);
int tf_conv3x3_grouped_wgrad_f32(const float* dy, const float* x, float* dw, int B, int H, int W, int C, int accumulate, float* ws, void* stream);
/* conv1 -> BatchNormAct2d -> grouped conv2 of a timm RegNetY Bottleneck (transfuser.py:380,442) with the BatchNorm apply folded into the CONSUMER:
 * x is the RAW output of conv1, in_coef = [scale | shift] (2 C floats, tf_bn_finalize_parts_f32) of its BatchNorm; the kernels stage
 * max(x scale + shift, 0) themselves (zero padding stays zero), so the normalised activation is never written to memory.  Forward = the
 * colstat forward above, weight gradient = tf_conv3x3_grouped_wgrad_f32 against that recomputed activation; the BatchNorm's own backward
 * recomputes its ReLU mask the same way (tf_bn_bwd_remask_f32). */
int tf_conv3x3_grouped_bnrelu_fwd_colstat_f32(const float* x, const float* in_coef, const float* w, float* y, int B, int H, int W, int C, float* colstat,
                                              int* colstat_nparts, void* stream);
int tf_conv3x3_grouped_bnrelu_wgrad_f32(const float* dy, const float* x, const float* in_coef, float* dw, int B, int H, int W, int C, int accumulate, float* ws,
                                        void* stream);
/* The STRIDE-2 grouped 3x3 convolution of the first block of every RegNetY stage (timm Bottleneck conv2 with stride 2) as direct kernels: forward
 * (Hi x Wi input -> ((Hi - 1) / 2 + 1) x ((Wi - 1) / 2 + 1) output; colstat / colstat_nparts optional: BatchNorm statistics of y as above; in_coef
 * optional: the producer's BatchNorm apply folded in) and weight gradient (ws as tf_conv3x3_grouped_wgrad_f32).  The input gradient is
 * tf_conv3x3_grouped_s2_dgrad_f32. */
int tf_conv3x3_grouped_s2_fwd_f32(const float* x, const float* in_coef, const float* w, float* y, int B, int Hi, int Wi, int C, float* colstat, int* colstat_nparts,
                                  void* stream);
int tf_conv3x3_grouped_s2_wgrad_f32(const float* dy, const float* x, const float* in_coef, float* dw, int B, int Hi, int Wi, int C, int accumulate, float* ws,
                                    void* stream);

/* Stem convolutions reading the NCHW model inputs directly (Cin <= 4, no bias, NHWC output):
 * channels [0,C0) from s0, [C0,C0+C1) from s1 - the torch.cat of model.py:741-742 is never
 * materialised; normalize != 0 folds normalize_imagenet (transfuser.py:419-428, K17) into the load.
 * Replaces features.conv1 / _model.conv1 (transfuser.py:136,140,475-478). */
int tf_stem_conv_fwd_f32(const tf_conv_geom* g, const float* s0, int C0, const float* s1, int C1, int normalize, const float* w, float* y, void* stream);
int tf_stem_conv_wgrad_f32(const tf_conv_geom* g, const float* dy, const float* s0, int C0, const float* s1, int C1, int normalize, float* dw,
                           int accumulate, void* stream);
/* tf_stem_conv_wgrad_f32 with caller scratch: the RegNet stems (ks^2 Cin <= 32, Cout = 32; transfuser.py:136-143) then run on direct kernels
 * (partial panels in ws + a deterministic reduce) instead of the im2col engine.  tf_stem_conv_wgrad_ws_floats: floats of scratch this geometry
 * wants (0 = the engine path, no scratch). */
long tf_stem_conv_wgrad_ws_floats(const tf_conv_geom* g, int C0, int C1);
int tf_stem_conv_wgrad_ws_f32(const tf_conv_geom* g, const float* dy, const float* s0, int C0, const float* s1, int C1, int normalize, float* dw,
                              int accumulate, float* ws, long ws_floats, void* stream);

/* ---- row-wise normalisation ------------------------------------------------------------------ */

/* nn.LayerNorm (transfuser.py:319,535-536).  bwd: dgamma/dbeta are ACCUMULATED (may be NULL). */
int tf_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int rows, int C, float eps, void* stream);
int tf_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, int dx_accumulate,
                         float* dgamma, float* dbeta, int rows, int C, void* stream);
/* tf_layernorm_bwd_f32 + a second output dropped = nn.Dropout(p)(dx) (dx = the finished, accumulated gradient) with the mask of
 * tf_dropout_f32(seed, site) over the contiguous (rows, C) tensor: the gradient entering the attention branch of a Block behind ln2's backward
 * (x_mid = x + resid_drop(proj(.)), transfuser.py:543-547) without a separate dropout launch (round 5).  dropped != dx. */
int tf_layernorm_bwd_drop_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, int dx_accumulate,
                              float* dgamma, float* dbeta, int rows, int C, float* dropped, const uint32_t* seed_dev, uint32_t site, float p, void* stream);
/* The parameter gradients of tf_layernorm_bwd_f32 alone, in fixed summation order: dgamma[c] += sum_rows dy xhat, dbeta[c] += sum_rows dy as
 * per-row-chunk partials in ws (the tf_workspace_bytes() reduction scratch every tf_bn_* / tf_colsum_* call takes) and a second stage that adds
 * the chunks in chunk order - bitwise reproducible, where the default form ends every 64-row block in fp32 atomics.  Under
 * tf_set_deterministic(1) the two entries above refuse dgamma / dbeta; call them with NULL and this entry beside them. */
int tf_layernorm_bwd_dw_f32(const float* dy, const float* x, const float* mean, const float* rstd, float* dgamma, float* dbeta, int rows, int C, float* ws,
                            void* stream);
/* F.softmax over attention rows (transfuser.py:520), in place; bwd turns dP into dS in place. */
int tf_softmax_fwd_f32(float* s, int rows, int n, int ld, void* stream);
int tf_softmax_bwd_f32(const float* p, float* dp, int rows, int n, int ld, void* stream);
/* softmax + attn_drop fused (transfuser.py:520-521): fwd writes the probabilities in place (kept for the backward) and the dropped
 * probabilities to sd; bwd takes the gradient w.r.t. the dropped probabilities.  Mask = tf_dropout_f32(site) over the flat (rows x ld) tensor. */
int tf_softmax_dropout_fwd_f32(float* s, float* sd, int rows, int n, int ld, const uint32_t* seed_dev, uint32_t site, float p, void* stream);
int tf_softmax_dropout_bwd_f32(const float* p, float* dp, int rows, int n, int ld, const uint32_t* seed_dev, uint32_t site, float pdrop, void* stream);

/* Fused self-attention of one GPT Block (SelfAttention.forward, transfuser.py:510-527): y = attn_drop(softmax(q k^T / sqrt(hs))) v for every
 * (sample, head), the (B, nh, T, T) scores never leave the CU.  qkv: (B*T, 3C) rows = [key | query | value] (transfuser.py:500-502), head h owns
 * columns h*hs .. (h+1)*hs of each third; y: (B*T, C) heads merged (transfuser.py:523); lse: (B*nh*T) row-wise log-sum-exp kept for the
 * backward, which RECOMPUTES the probabilities.  attn_drop mask = tf_dropout_f32's for the flat index ((b nh + h) T + i) Tp + j, Tp = T
 * rounded up to 4 (pdrop = 0: no dropout, seed_dev may be NULL).  bwd: dqkv (B*T, 3C) = gradients of [key | query | value]; dsum: (B*nh*T)
 * scratch.  Limits: T <= 1024, even hs <= 384 (tf_attention_supported); the model has T = 174, hs in {18, 54, 144, 378}.  T <= 192 (one column
 * chunk) runs the whole-row kernels; 192 < T <= 1024 (other anchor grids, transfuser.py:19-20,304) the column-chunked ones, dispatched inside
 * tf_attention_fwd_f32 and tf_attention_bwd_y_f32.  tf_attention_bwd_f32 (the two dependent launches without y) stays at T <= 192 and fails beyond. */
int tf_attention_supported(int T, int C, int nh);
int tf_attention_fwd_f32(const float* qkv, float* y, float* lse, int B, int T, int C, int nh, const uint32_t* seed_dev, uint32_t site, float pdrop,
                         void* stream);
int tf_attention_bwd_f32(const float* qkv, const float* dy, const float* lse, float* dqkv, float* dsum, int B, int T, int C, int nh,
                         const uint32_t* seed_dev, uint32_t site, float pdrop, void* stream);
/* The same gradients in two launches whose second one holds BOTH halves (round 6): y = tf_attention_fwd_f32's output; D_i = dY_i . Y_i (equal to
 * sum_j dP_ij P_ij, also under attention dropout) is formed first (written to dsum), then keys and queries run as one grid.  dy / y 8-byte aligned. */
int tf_attention_bwd_y_f32(const float* qkv, const float* dy, const float* y, const float* lse, float* dqkv, float* dsum, int B, int T, int C, int nh,
                           const uint32_t* seed_dev, uint32_t site, float pdrop, void* stream);

/* ---- per-channel reductions / BatchNorm / Squeeze-Excite ------------------------------------- */

/* scratch every reduction entry point needs (one buffer per stream is enough).  The buffer must be ZERO-INITIALISED once by its owner before
 * its first use: its last 16 KB hold the arrival counters of the fused reduce + finalize kernels (the block that draws a column tile's last
 * ticket sums the chunk partials in a fixed order and resets the counter, so the buffer stays valid for the next launch on that stream). */
long tf_workspace_bytes(void);
/* Train-mode BatchNorm forward whose batch statistics were gathered by the PRODUCING convolution's epilogue (tf_gemm_desc.colstat,
 * tf_conv2d_fwd_colstat_f32, tf_conv3x3_grouped_fwd_colstat_f32: per-part Welford triples [part][{count, mean, M2}][C]): merges the parts
 * (Chan's formula), updates the running statistics, writes save_mean / save_invstd and applies y = bn(x) (+res) (relu) - the moments pass
 * over x of tf_bn_fwd_f32 is gone (timm BatchNormAct2d behind every RegNetY convolution, transfuser.py:380,442). */
int tf_bn_fwd_parts_f32(const float* x, int rows, int C, const float* parts, int nparts, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps, const float* res, int relu, float* y, float* save_mean, float* save_invstd,
                        float* ws, void* stream);
/* timm BatchNormAct2d on NHWC (rows = B*H*W): y = bn(x) (+res) (relu); training uses batch statistics
 * and updates the running buffers (momentum, unbiased var).  bwd accumulates dgamma/dbeta.
 * zacc: optional tf_bn_zacc_floats(C) floats that the CALLER has zeroed (e.g. a slice of a scratch arena cleared once per step): the statistics are then
 * accumulated there with fp32 atomics (16 copies, added up in fp64) and folded into the normalise pass - 2 launches instead of 3.  NULL: partials in ws + a
 * finalize kernel (bit-reproducible summation order). */
int tf_bn_fwd_f32(const float* x, int rows, int C, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                  float eps, const float* res, int relu, float* y, float* save_mean, float* save_invstd, float* ws, int training, float* zacc,
                  void* stream);
int tf_bn_zacc_floats(int C);
int tf_bn_bwd_f32(const float* dz, const float* z, const float* x, int rows, int C, const float* gamma, const float* save_mean, const float* save_invstd,
                  float* dx, float* dres, float* dgamma, float* dbeta, float* ws, float* zacc, void* stream);
/* BatchNorm2d backward of a layer that normalised with FROZEN statistics (the module in eval() inside a training step: F.batch_norm(x, running_mean,
 * running_var, gamma, beta, training=False)); mean / invstd = what tf_bn_fwd_f32(training = 0) leaves in save_mean / save_invstd (running_mean,
 * 1 / sqrt(running_var + eps)).  With g = dz [z > 0] (z NULL: no ReLU): dx = g gamma invstd, dres = g (optional), dgamma += sum g (x - mean) invstd,
 * dbeta += sum g.  dgamma and dbeta are given together (then x, mean and ws = tf_workspace_bytes() are needed) or both NULL (frozen affine: one
 * element-wise pass, x is not read).  The column sums are chunk partials + a finalize launch in every mode: no float atomics. */
int tf_bn_bwd_frozen_f32(const float* dz, const float* z, const float* x, int rows, int C, const float* gamma, const float* mean, const float* invstd,
                         float* dx, float* dres, float* dgamma, float* dbeta, float* ws, void* stream);
/* out[seg][c] (+)= scale * sum_rows x (* [mask > 0]): SE squeeze / global average pool
 * (transfuser.py:203-205), bias gradients, pos_emb gradient. */
int tf_colsum_f32(const float* x, const float* mask, int nseg, int rows_per_seg, int C, float scale, float* out, int accumulate, float* ws, void* stream);
/* timm SEModule excite: y = x * sigmoid(gate[b][c]) and its two backward pieces. */
int tf_se_scale_fwd_f32(const float* x, const float* gate, float* y, int B, int HW, int C, void* stream);
int tf_se_scale_bwd_gate_f32(const float* dy, const float* x, const float* gate, float* dgate, int B, int HW, int C, float* ws, void* stream);
int tf_se_scale_bwd_x_f32(const float* dy, const float* gate, const float* dmean, float* dx, int B, int HW, int C, int accumulate, void* stream);

/* SE excitation MLP fused (timm SEModule.fc1 -> ReLU -> fc2 on the pooled (B, C) vector; B <= 16):
 *   fwd: g1 (B, Cr) = relu(s W1^T + b1), gate (B, C) = g1 W2^T + b2 (pre-sigmoid; tf_se_scale_fwd_f32 applies the sigmoid).
 *   bwd: given dgate (B, C): dW2 += dgate^T g1, db2 += sum_b dgate, dg1 = (dgate W2) * (g1 > 0), dW1 += dg1^T s, db1 += sum_b dg1,
 *        ds (B, C) = dg1 W1.  All parameter gradients are ACCUMULATED; scratch = B*Cr floats. */
int tf_se_excite_fwd_f32(const float* s, const float* W1, const float* b1, const float* W2, const float* b2, int B, int C, int Cr, float* g1,
                         float* gate, float* bwd_scratch /* optional (B, Cr): cleared here for tf_se_excite_bwd_f32(scratch_is_zero = 1) */, void* stream);
int tf_se_excite_bwd_f32(const float* dgate, const float* s, const float* g1, const float* W1, const float* W2, int B, int C, int Cr, float* dW1,
                         float* db1, float* dW2, float* db2, float* ds, float* scratch, int scratch_is_zero, void* stream);
/* Floats `scratch` of tf_se_excite_bwd_f32 / tf_se_excite_bwd_parts_f32 must hold: B * Cr, and under tf_set_deterministic(1)
 * ceil(C / 8) * B * Cr - the fc2 pass then writes one (B, Cr) slab of dg1 per block instead of adding into one with fp32 atomics, the fc1 pass
 * sums the slabs in block order and takes all Cr rows per column block (ds is stored, not added); scratch_is_zero is ignored in that mode. */
long tf_se_excite_bwd_ws_floats(int B, int C, int Cr);

/* ---- resampling ------------------------------------------------------------------------------ */

/* AdaptiveAvgPool2d((oh,ow)) of an NHWC map written straight into rows [tok_off, tok_off+oh*ow) of the
 * (B, T_total, C) token matrix, + pos_emb (+ per-sample vector): transfuser.py:150-151,346-357. */
int tf_pool_tokens_fwd_f32(const float* x, int B, int H, int W, int C, int oh, int ow, const float* pos, const float* bvec, float* tok, int T_total,
                           int tok_off, void* stream);
/* dx = (add ? add : 0) + pool^T(dtok): `add` carries the identity branch of x + up(gpt(x)) */
int tf_pool_tokens_bwd_f32(const float* dtok, int B, int H, int W, int C, int oh, int ow, int T_total, int tok_off, float* dx, const float* add, void* stream);

/* F.interpolate(mode='bilinear') with explicit element strides for input and output (any layout):
 * y = up(x) (+ add);  bwd is a gather (no atomics).  transfuser.py:103,154-157,241,243; model.py:760. */
typedef struct {
    int B, C, Hi, Wi, Ho, Wo;
    int64_t sb_i, sc_i, sh_i, sw_i;
    int64_t sb_o, sc_o, sh_o, sw_o;
    int align_corners;
} tf_bilinear_desc;
int tf_bilinear_fwd_f32(const tf_bilinear_desc* d, const float* x, float* y, const float* add, void* stream);
int tf_bilinear_bwd_f32(const tf_bilinear_desc* d, const float* dy, float* dx, int accumulate, void* stream);
/* 3x3 / stride 2 / pad 1 max pooling on NHWC maps: ``maxpool`` of the timm ResNet trunks, the reference's DEFAULT architectures
 * (transfuser.py:15,139,143: image 'resnet34', LiDAR 'resnet18').  idx: one byte per output element = the winning tap 0..8 (first maximum in
 * (kh, kw) order, as ATen); the backward gathers through it (no atomics).  Output (B, (Hi-1)/2+1, (Wi-1)/2+1, C). */
int tf_maxpool3x3s2_fwd_f32(const float* x, float* y, unsigned char* idx, int B, int Hi, int Wi, int C, void* stream);
int tf_maxpool3x3s2_bwd_f32(const float* dy, const unsigned char* idx, float* dx, int B, int Hi, int Wi, int C, void* stream);

/* G1 - geometric-fusion correspondence gather (geometric_fusion.py:134-137,147-150; and :173-176 ... :262-266 for the other
 * stages): out[b, i, :] = sum_k src[b, idx[b,i,k,1] * Ws + idx[b,i,k,0], :].  The reference indexes B x B and keeps the diagonal;
 * only the diagonal is computed here.  src (B, Hs*Ws, E) fp32, idx (B, n, K, 2) int64 (x, y) pairs, out (B, n, E).
 * bwd is the transposed gather in a fixed summation order (deterministic); accumulate != 0 adds into dsrc. */
int tf_gather_sum_fwd_f32(const float* src, const long long* idx, int B, int Hs, int Ws, int E, int n, int K, float* out, void* stream);
int tf_gather_sum_bwd_f32(const float* dout, const long long* idx, int B, int Hs, int Ws, int E, int n, int K, float* dsrc, int accumulate,
                          void* stream);

/* ---- losses ---------------------------------------------------------------------------------- */

/* F.cross_entropy(logits, target, weight=class_w) (model.py:763,783) over NHWC logits (rows, C <= 16):
 * loss = sum w_y nll / sum w_y; dlogits = w_y (softmax - onehot) (multiply by g * (*inv_wsum) later). */
int tf_ce_fwd_f32(const float* logits, const int64_t* target, const float* class_w, int64_t rows, int C, float* dlogits, float* loss, float* inv_wsum,
                  float* ws, void* stream);
/* mean |f(pred) - target| with f = identity / sigmoid (model.py:765,784); dpred un-scaled. */
int tf_l1_fwd_f32(const float* pred, const float* target, int64_t n, int use_sigmoid, float* dpred, float* loss, float* ws, void* stream);
/* x *= (*a_dev) * (*b_dev) * mult (device scalars optional) */
int tf_scale_dev_f32(float* x, int64_t n, const float* a_dev, const float* b_dev, float mult, void* stream);
/* LidarCenterNetHead.get_targets (model.py:285-374) in one launch, no host sync.
 * tgtf (B,fh,fw,8) = [heatmap, wh_w, wh_h, off_x, off_y, yaw_res, velocity, weight]; tgti (B,fh,fw,2) = [yaw_class, brake]; cnt[b] = #(heatmap == 1) */
int tf_centernet_targets_f32(const float* label, int B, int nbox, int fh, int fw, float ratio_w, float ratio_h, int num_dir_bins, float* tgtf,
                             int32_t* tgti, int32_t* cnt, void* stream);
/* LidarCenterNetHead.loss (model.py:150-248) with mmdet 2.25 semantics; pred (B,fh,fw,9+bins) =
 * [hm logit, wh(2), offset(2), yaw_class(bins), yaw_res, velocity, brake(2)]; losses[7] in the order
 * center_heatmap, wh, offset, yaw_class, yaw_res, velocity, brake. */
int tf_centernet_loss_fwd_f32(const float* pred, const float* tgtf, const int32_t* tgti, const int32_t* cnt, int B, int fh, int fw, int num_dir_bins,
                              float* losses, float* ws, void* stream);
int tf_centernet_loss_bwd_f32(const float* pred, const float* tgtf, const int32_t* tgti, const int32_t* cnt, const float* gup, int B, int fh, int fw,
                              int num_dir_bins, float* dpred, void* stream);

/* Inference decode of the CenterNet head (model.py:436-497 decode_heatmap with mmdet's get_local_maximum /
 * get_topk_from_heatmap / transpose_and_gather_feat): pred (B, fh, fw, 9 + bins) packed logits as in tf_centernet_loss_*,
 * out (B, k, 8) = [x, y, w, h (already x ratio), yaw, velocity, brake (0/1), score], sorted by decreasing score. */
int tf_centernet_decode_f32(const float* pred, int B, int fh, int fw, int num_dir_bins, int k, int kernel, float ratio, float* out, void* stream);

/* ---- elementwise / recurrent / optimiser / data ----------------------------------------------- */
int tf_relu_mask_f32(const float* dy, const float* y, float* out, int64_t n, void* stream);
int tf_sigmoid_f32(const float* x, float* y, int64_t n, void* stream);
int tf_axpby_f32(const float* a, const float* b, float* out, float alpha, float beta, int64_t n, void* stream);
/* total = sum_i weights[i] * terms[i][0] over 1..16 device scalars in separate allocations, added in index order, and its backward
 * dterms[i] = weights[i] * dtotal[0] (dtotal NULL = 1): the weighted sum of the 11 detailed losses of train.py:307-311 in one launch per direction.
 * terms / weights are HOST arrays read at call time (graph-capturable: they travel as kernel arguments). */
int tf_weighted_sum_f32(const float* const* terms, const float* weights, int n, float* out, void* stream);
int tf_weighted_sum_bwd_f32(const float* dtotal, const float* weights, int n, float* dterms, void* stream);
/* nn.Dropout with a counter-based RNG keyed by (*seed_dev, site, index); calling it on dy with the
 * same key is the backward (transfuser.py:311,504-505,542). */
int tf_dropout_f32(const float* x, float* y, int64_t n, const uint32_t* seed_dev, uint32_t site, float p, void* stream);
/* y = res + dropout(x) with the mask of tf_dropout_f32(site): x + resid_drop(...) of transfuser.py:543-544 in one pass (y may alias x or res) */
int tf_dropout_add_f32(const float* x, const float* res, float* y, int64_t n, const uint32_t* seed_dev, uint32_t site, float p, void* stream);
/* Waypoint decoder (model.py:611-646): pred_len x { GRUCell(4|2 -> 64), Linear(64,3), running sum } fused
 * into one launch per direction.  cache: tf_gru_waypoints_cache_floats(B, pred_len) floats kept for the
 * backward, which ACCUMULATES the parameter gradients and writes dz0 (grad of the join-MLP output). */
long tf_gru_waypoints_cache_floats(int B, int pred_len);
int tf_gru_waypoints_fwd_f32(const float* z0, const float* target_point, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                             const float* w_out, const float* b_out, int B, int hidden, int pred_len, int nin, float shift_x, float* wp, float* cache,
                             void* stream);
int tf_gru_waypoints_bwd_f32(const float* dwp, const float* cache, const float* w_ih, const float* w_hh, const float* w_out, int B, int hidden,
                             int pred_len, int nin, float* dz0, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* dw_out, float* db_out,
                             void* stream);
/* fp32 <-> bf16 (round to nearest even; y = x * scale on the way back): optional bf16 gradient buckets of the data-parallel all-reduce
 * (DistributedDataParallel's bucketed all-reduce, train.py:134, reduces fp32; halving the xGMI payload is an opt-in of this framework). */
int tf_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, void* stream);
int tf_cast_bf16_f32(const uint16_t* x, float* y, int64_t n, float scale, void* stream);
/* torch.optim.AdamW (train.py:142) over a flat arena in one launch; state_dev = {step, lr} floats
 * on the device (step is advanced by the call, so a captured hipGraph replays correctly). */
int tf_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps, float weight_decay,
                 void* stream);
/* The same update with the gradients multiplied by grad_scale on the way in (= 1 / loss scale of the fp16 mode; the loss scale seeds the backward). */
int tf_adamw_scaled_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps, float weight_decay,
                        float grad_scale, void* stream);
/* The same update under a DYNAMIC loss scale (fp16 mode; the reference trains fp32 - config.py:55 - and has no counterpart; semantics of
 * torch.cuda.amp.GradScaler): ls_state = {scale, clean steps, found_inf, growth interval} floats on the device.  The call (1) sets found_inf
 * when any of g_check[0 .. n_check) is Inf / NaN (pass the WHOLE reduced gradient arena here, also when p / g / m / v are a ZeRO-1 shard, so
 * every rank decides alike), (2) skips the step - parameters, moments and the step counter untouched - when it is set, else updates with the
 * gradients divided by scale, (3) halves the scale after an overflow / doubles it after `growth interval` clean steps and clears found_inf.
 * The next backward is seeded with ls_state[0].  No host synchronisation: hipGraph-capturable. */
int tf_adamw_dynscale_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                          float weight_decay, const float* g_check, int64_t n_check, float* ls_state, void* stream);
/* Global-norm gradient clipping in front of the AdamW step (torch.nn.utils.clip_grad_norm_; extends the loop of train.py:305-314, which has
 * none).  tf_grad_sumsq_f32 reads the 16-byte-aligned fp32 range g[0 .. n), n >= 1, once and stores P = tf_grad_sumsq_parts(n) <= 1024 partial
 * sums of squares into `partials` (caller scratch of P floats; the library allocates nothing).  P depends on n alone, every block writes one
 * plain store and nothing is combined with atomics: summing the partials in index order is a fixed-order sum, bitwise reproducible and legal
 * under tf_set_deterministic(1). */
int tf_grad_sumsq_parts(int64_t n);
int tf_grad_sumsq_f32(const float* g, int64_t n, float* partials, void* stream);
/* tf_adamw_scaled_f32 with the gradients clipped to `max_norm` on their way in (extends train.py:305-314 likewise): `partials` / `nparts` are
 * what tf_grad_sumsq_f32 left for the norm range g_norm[0 .. n_norm) - the WHOLE active gradient arena, also when p / g / m / v are a ZeRO-1
 * shard, as with g_check of tf_adamw_dynscale_f32.  Every block sums the partials in one fixed order, norm = gs * sqrt(sum),
 * coef = min(1, max_norm / (norm + 1e-6)) - clip_grad_norm_'s formula, with its non-finite behaviour - and updates with gs * coef; the pre-clip
 * norm (what clip_grad_norm_ returns) is stored to norm_out[0].  gs = grad_scale, or grad_scale / ls_state[0] with a (nullable) ls_state: the
 * step then runs under the dynamic loss scale exactly as tf_adamw_dynscale_f32 does (overflow check over g_norm, which only this case reads;
 * a skipped step writes nothing and does not count).  nparts must equal tf_grad_sumsq_parts(n_norm), max_norm > 0 (+inf never clips). */
int tf_adamw_clip_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps, float weight_decay,
                      float grad_scale, const float* g_norm, int64_t n_norm, const float* partials, int nparts, float max_norm, float* norm_out,
                      float* ls_state, void* stream);
/* AdamW parameter groups (torch.optim.AdamW's param_groups; extends train.py:142, which has one group).  The range is whole tiles of 64 floats
 * (n % 64 == 0, n >= 64); tile_group[t] (n / 64 bytes) names the group of floats [64 t, 64 t + 64) and table = [ngroups][{lr_mult, weight_decay,
 * frozen}] floats, both on the device, ngroups in 1..255 (an id >= ngroups reads the last row).  A group updates with lr = state_dev[1] * lr_mult
 * and its own decoupled weight decay; frozen != 0 skips the tile before any load: p, m, v are neither read nor written, g is not read.  Values
 * written to the table between two replays of a captured graph take effect without a recapture.  For a ZeRO-1 shard [lo, hi) pass
 * tile_group + lo / 64 with the shard's p / g / m / v.
 * tf_grad_sumsq_groups_f32 = tf_grad_sumsq_f32 without the frozen tiles (clip_grad_norm_ only sees parameters that have a gradient): the same
 * P = tf_grad_sumsq_parts(n) plain-store partials, no atomics, legal under tf_set_deterministic(1).
 * tf_adamw_groups_f32 = tf_adamw_scaled_f32 per group; with partials != NULL it clips like tf_adamw_clip_f32 (nparts = tf_grad_sumsq_parts(n_norm)
 * partials of the norm range, max_norm > 0, pre-clip norm to norm_out[0]); partials NULL: no clipping, nparts / n_norm / max_norm / norm_out
 * unused.  There is no dynamic-loss-scale form. */
int tf_grad_sumsq_groups_f32(const float* g, int64_t n, const uint8_t* tile_group, const float* table, int ngroups, float* partials, void* stream);
int tf_adamw_groups_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps, float grad_scale,
                        const uint8_t* tile_group, const float* table, int ngroups, const float* partials, int nparts, int64_t n_norm, float max_norm,
                        float* norm_out, void* stream);
/* Exponential moving average of the weights (timm's ModelEmaV2, with ModelEmaV3's optional warm-up; the reference keeps none - this sits beside
 * its optimizer and checkpoint code, train.py:142,204-210,381-384).  A pass of its own BEHIND the optimizer step, 12 B per parameter (p read,
 * e read, e written); the AdamW kernels are not involved.  Element-wise throughout: no atomics, no workspace, nothing allocated, capturable,
 * legal under tf_set_deterministic(1).
 * ema_state = {decay, num_updates, last_opt_step, coef} floats on the device, so a replayed graph advances it without the host.
 * tf_ema_tick_f32 (one thread; a launch of its own in front of the apply launches, which only read the state): with t = opt_state[0]
 * (FlatAdamW's {step, lr}) the step is a no-op, coef = 0, when t == last_opt_step - the optimizer skipped an overflowed fp16 step and did not
 * count it - or when t % every != 0; otherwise n = num_updates, d = warmup ? min(decay, (1 + n) / (10 + n)) : decay, coef = 1 - d,
 * num_updates = n + 1, last_opt_step = t.  opt_state NULL: every call updates (last_opt_step stays).  every >= 1.
 * tf_ema_apply_f32: e = fma(coef, p - e, e) over n floats, n % 4 == 0, both ranges 16-byte aligned and disjoint; returns at once when coef == 0.
 * tf_ema_apply_multi_f32: the same over a device table of (ema, live, count) entries of any alignment and count >= 1, one launch (the module
 * buffers outside the arena: BatchNorm running_mean / running_var), nentries >= 1.
 * tf_swap_f32 / tf_swap_multi_f32 exchange the contents of a / b (n % 4 == 0, 16-byte aligned) or of every (ema, live) pair of the table, in
 * place.  tf_swap_f32 refuses overlapping ranges; the ranges of a table live on the device and must be pairwise disjoint - ops.ema_table
 * refuses to build a table whose ranges overlap.  A refused call launches nothing. */
typedef struct { float* ema; float* live; int64_t count; } tf_ema_item;
int tf_ema_tick_f32(float* ema_state, const float* opt_state, int every, int warmup, void* stream);
int tf_ema_apply_f32(float* ema, const float* p, int64_t n, const float* ema_state, void* stream);
int tf_ema_apply_multi_f32(const tf_ema_item* table_dev, int nentries, const float* ema_state, void* stream);
int tf_swap_f32(float* a, float* b, int64_t n, void* stream);
int tf_swap_multi_f32(const tf_ema_item* table_dev, int nentries, void* stream);
/* lidar_to_histogram_features (data.py:446-470): points (B, max_points, stride>=3) f32 -> (B,2,256,256),
 * integer-exact; num_points may be NULL. */
int tf_lidar_hist_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, float* out, void* stream);
/* The same in two launches instead of three: `zero_ws` = tf_lidar_hist_ws_bytes(B) bytes (16-byte aligned) owned by the caller, ALL ZERO before the
 * first call; every call leaves it all zero again (the int32 cell counters live there instead of in `out`, the finishing pass clears them). */
long tf_lidar_hist_ws_bytes(int B);
int tf_lidar_hist_ws_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, void* zero_ws, float* out, void* stream);

/* ---- H2: PointPillars front-end (point_pillar.py:37-122, model.py:736-738) - integer-exact pillar ids without a sort ---------
 * The reference's torch.unique(dim=0, return_inverse=True) over (batch, x_idx, y_idx) rows == rank of the occupied cell in an
 * occupancy grid scanned in (b, x_idx, y_idx) order.  GX = nx + 1, GY = ny + 1 (an index may reach nx / ny when (x - min) rounds
 * up; the reference clamps it in scatter_points).  Call order (host reads the two scan totals N, P in between):
 *   tf_pillar_keys_f32  -> keys (B*Nmax; -1 = dropped), keep flags, occupancy grid (B*GX*GY)         [:70-83, first num_points]
 *   tf_exclusive_scan_i32 x2 -> pos = scan(keep) (+N), rank = scan(occ) (+P)                          [torch.unique, :88]
 *   tf_pillar_gather_f32 -> stable compaction pts4 (N,4), inv (N), per-pillar xyz sums + count (P,4) as int64 (coordinates in units of 2^-24 m:
 *                           integer atomics, so the sums do not depend on the order they land in - run-to-run reproducible), cellkey (P)
 *   tf_pillar_decorate_f32 -> 9 features per point (:54-67, quirk Q15 kept)
 *   [DynamicPointNet: Linear+BN1d+ReLU x2 through tf_gemm_f32 / tf_bn_*]
 *   tf_pillar_scatter_max_f32 -> pillar_feat (P,C) = scatter_max (:32), arg (P,C) = lowest row attaining it
 *   tf_pillar_canvas_f32 -> NHWC (B,H,W,C+Ce): scatter_points (:94-95, clamps, last duplicate wins) + rot90(-1) (model.py:738)
 *                           + the Ce extra NCHW channels (target-point image, model.py:741-742) appended un-rotated
 *   tf_pillar_canvas_bwd_f32 -> dz (N,C): the canvas gradient routed to each pillar's arg-max point. */
int tf_pillar_keys_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, float min_x, float max_x,
                       float min_y, float max_y, float pixels_per_meter, int GX, int GY, int32_t* keys, int32_t* keep, int32_t* occ, void* stream);
/* Both scans of the pillar index in two launches (point_pillar.py:85-91: what torch.unique(return_inverse) yields, without the sort): pos = exclusive
 * scan of [keys >= 0] (row of every kept point in the compacted cloud), rank = exclusive scan of the occupancy grid (sorted-unique pillar id of
 * every occupied cell), cellkey[rank] = cell, totals = {kept points, pillars}.  ws: (n_points + ncells) / 1024 + 2 ints.  tf_pillar_gather_f32 may
 * then be called with occ = NULL (the cell keys exist already). */
int tf_pillar_index_scan_i32(const int32_t* keys, int64_t n_points, const int32_t* occ, int64_t ncells, int32_t* pos, int32_t* rank, int32_t* cellkey,
                             int32_t* totals, int32_t* ws, void* stream);
int tf_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* total, int32_t* ws /* n/1024+1 ints */, void* stream);
int tf_pillar_gather_f32(const float* points, int point_stride, const int32_t* keys, const int32_t* pos, const int32_t* occ, const int32_t* rank,
                         int64_t n_all, int64_t ncells, int P, float* pts4, int32_t* inv, int64_t* sums, int32_t* cellkey, void* stream);
int tf_pillar_decorate_f32(const float* pts4, const int32_t* inv, const int64_t* sums, const int32_t* cellkey, int64_t N, int GX, int GY,
                           float pixels_per_meter, float min_x, float min_y, float* feat, void* stream);
/* Round 6: the same index in three launches, no fill, no global atomic (reference: the same lines of point_pillar.py:69-91 + decorate :54-67; results
 * identical to the sequence above - integer-exact pillar ids, the same fixed-point sums).  Cells carry a PADDED id b * CP + x_idx * GY + y_idx,
 * CP = tf_pillar_padded_cells(GX, GY) (each sample rounded up to whole LDS slabs; CP % 128 == 0; the order of the ids is torch.unique's row order).
 *   tf_pillar_mark_f32            keys (B*Nmax padded ids; -1 = dropped), bitmap (B*CP/32 ints, every word written), cellsums (B*CP x 4 int64; only the
 *                                 occupied cells' entries are written - and later read), blockcnt (B * cdiv(Nmax, 1024) kept-point counts)
 *   tf_pillar_rank_scan_i32       wordprefix (like bitmap), blockoff (like blockcnt), totals = {kept points N, pillars P} (device memory)
 *   tf_pillar_gather_decorate_f32 pts4 (N,4), inv (N), feat (N,9), cellkey (P; un-padded (b*GX + x_idx)*GY + y_idx); fill_tail = 1 (static shapes): the buffers
 *                                 have B*Nmax rows / cell_cap slots, rows >= N are written as zero and cell-key slots >= P as -1 by the same launch
 * No workspace survives a call; bitmap / wordprefix / cellsums 16-byte aligned; padded cells and points < 2^24. */
long tf_pillar_padded_cells(int GX, int GY);
int tf_pillar_mark_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, float min_x, float max_x, float min_y,
                       float max_y, float pixels_per_meter, int GX, int GY, int32_t* keys, int32_t* bitmap, int64_t* cellsums, int32_t* blockcnt, void* stream);
int tf_pillar_rank_scan_i32(const int32_t* bitmap, int64_t padded_cells, const int32_t* blockcnt, int nblocks, int32_t* wordprefix, int32_t* blockoff,
                            int32_t* totals, void* stream);
int tf_pillar_gather_decorate_f32(const float* points, int point_stride, const int32_t* keys, int B, int max_points, const int32_t* blockoff,
                                  const int32_t* wordprefix, const int32_t* bitmap, const int64_t* cellsums, const int32_t* totals, int GX, int GY,
                                  float pixels_per_meter, float min_x, float min_y, float* pts4, int32_t* inv, float* feat, int32_t* cellkey, int64_t cell_cap,
                                  int fill_tail, void* stream);
int tf_pillar_scatter_max_f32(const float* z, const int32_t* inv, int64_t N, int C, int P, float* pillar_feat, int32_t* arg, void* stream);
int tf_pillar_canvas_f32(const float* pillar_feat, const int32_t* cellkey, int P, int C, int B, int H, int W, int GX, int GY,
                         const float* extra_nchw, int Ce, int32_t* owner, float* out_nhwc, void* stream);
int tf_pillar_canvas_bwd_f32(const float* dout_nhwc, const int32_t* owner, const int32_t* cellkey, const int32_t* inv, const int32_t* arg,
                             int64_t N, int C, int Cs, int GX, int GY, int H, int W, float* dz, void* stream);
/* Static-shape mode of the front-end (round 5: --use_point_pillars under a captured hipGraph).  The kept-point / pillar counts stay on the DEVICE
 * (totals of tf_pillar_index_scan_i32): every buffer has its capacity (B * max_points rows, min(B * max_points, cells) pillars), the compacted cloud and
 * inv are zero-filled, unused cell-key slots hold -1 (tf_pillar_canvas_f32 skips them), and the point net's nn.BatchNorm1d (point_pillar.py:17-27), whose
 * row count is data dependent, runs as tf_bn_rows_dev_*: statistics over the first *nrows_dev rows only, rows beyond written as zero by both apply passes -
 * so Linear, scatter-max and the weight gradients can run over the whole capacity.  C <= 256 dividing 256; ws: tf_bn_rows_dev_ws_floats(C) floats. */
long tf_bn_rows_dev_ws_floats(int C);
int tf_bn_rows_dev_fwd_f32(const float* x, const int32_t* nrows_dev, int rows_cap, int C, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, float* ws, void* stream);
int tf_bn_rows_dev_bwd_f32(const float* dz, const float* z, const float* x, const int32_t* nrows_dev, int rows_cap, int C, const float* gamma,
                           const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta, float* ws, void* stream);

/* GPU-side batch preparation: the per-sample numpy work of team_code_transfuser/data.py after file decoding, batched.
 * tf_lidar_align_hist_f64: align (data.py:411-444: q = T (x, -y, z, 1), y' = -q1; T (B,16) row-major fp64) fused with the 2-bin height histogram
 *   (data.py:446-470) of the transformed cloud; optional aligned cloud output (B, max_points, 4) fp32 for PointPillars (data.py:247-251).
 * tf_image_prep_u8: centre crop with per-sample x shift of an HWC uint8 batch; mode 0 -> CHW float (crop_image_cv2, data.py:536-553), 1 -> get_depth
 *   (data.py:358-372), 2 -> crop_seg + class LUT (data.py:176-177).  tf_bev_prep_u8: decode_pil_to_npy + load_crop_bev_npy (data.py:844-856,586-612). */
int tf_lidar_align_hist_f64(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, const double* transforms, float* out,
                            float* aligned_or_null, void* stream);
int tf_lidar_align_hist_ws_f64(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, const double* transforms,
                               void* zero_ws, float* out, float* aligned_or_null, void* stream);      /* two launches, workspace as tf_lidar_hist_ws_f32 */

/* lidar_bev_cam_correspondences + correspondences_at_one_scale (team_code_transfuser/data.py:632-842; per sample at data.py:273 and
 * submission_agent.py:306) for a batch of raw clouds: points (B, max_points, point_stride >= 3) float32 in the CARLA frame (x left, y forward,
 * z up; y_negated != 0: the buffer holds the cloud as the loader keeps it, y already negated (data.py:170), and is read with y flipped back),
 * num_points (B) or NULL.  cam6 (HOST pointer) = {focal_x, focal_y, cos(-60 deg), sin(-60 deg), cos(60 deg), sin(60 deg)} as
 * data.py:688-712,741-747 evaluates them.  Outputs int32: bev_points (B, 8, 8, 5, 2) = image cells (x in [0, 22), y in [0, 5)) of up to five
 * points per BEV cell, cam_points (B, 22, 5, 5, 2) = BEV cells of up to five points per image cell, zero padded like the reference.  Cells with
 * more than five points: the reference draws random.sample(list, 5) from Python's global generator; here a counter-based draw keyed by
 * (seed, sample, list, cell, entry) with the same distribution.  ws: tf_lidar_cam_correspondences_ws_bytes(B, max_points) bytes, 16-byte aligned. */
long tf_lidar_cam_correspondences_ws_bytes(int B, int max_points);
int tf_lidar_cam_correspondences_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, int y_negated,
                                     const double* cam6, uint32_t seed, void* ws, int32_t* bev_points, int32_t* cam_points, void* stream);
int tf_image_prep_u8(const uint8_t* src, int B, int Hs, int Ws, int C, int crop_h, int crop_w, int start_y, const int32_t* start_x, int mode, const uint8_t* lut,
                     void* out, void* stream);
int tf_bev_prep_u8(const uint8_t* encoded, int B, int S, const float* degrees_or_null, int64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
