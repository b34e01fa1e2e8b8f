/*
 * dfd_hip.h -- C ABI of the MI355X-native EfficientNet-B0 frame-classifier hot path.
 *
 * libdfd_hip.so (built from deepfake-video-detection_amd/csrc for gfx950) exports exactly
 * the functions below.  Every argument is a plain pointer / size; device pointers are HIP
 * device memory owned by the caller (PyTorch's caching allocator in the Python binding);
 * `stream` is a hipStream_t passed as void*.  No function allocates device memory on the
 * launch path, synchronises, or aborts: every entry point returns 0 on success and -1 on
 * failure, with a message from dfd_last_error() (the Python layer raises RuntimeError,
 * which the reference's callers turn into error dicts, app.py:2320-2321, detector.py:134-141).
 *
 * The reference has no native code; each entry point names the reference
 * Python call site whose computation it replaces.
 */
#ifndef DFD_HIP_H
#define DFD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFD_API __attribute__((visibility("default")))

/* dtype codes for the activation storage of the trunk */
#define DFD_DTYPE_F32 0
#define DFD_DTYPE_BF16 1
#define DFD_DTYPE_F16 2 /* IEEE half storage, v_mfma_f32_16x16x32_f16 (train with dynamic loss scaling) */

/* tensor kinds reported by dfd_b0_tensor_info */
#define DFD_TENSOR_PARAM 0   /* trainable fp32 parameter (flat parameter buffer)      */
#define DFD_TENSOR_BNBUF 1   /* BatchNorm running_mean / running_var (flat BN buffer) */
#define DFD_TENSOR_COUNTER 2 /* BatchNorm num_batches_tracked (host-managed int64)   */

typedef struct dfd_b0_plan dfd_b0_plan;

/* Last error message of the calling thread ("" if none). */
DFD_API const char* dfd_last_error(void);
/* ABI version (major*100 + minor). */
DFD_API int dfd_version(void);

/* ---- EfficientNet-B0 trunk ------------------------------------------------------------
 * Replaces timm.create_model('efficientnet_b0') wrapped as
 * nn.Sequential(*list(backbone.children())[:-1])   (src/pretrained_detector.py:43-46)
 * and its call self.backbone(x_flat) -> (B*T, 1280)  (src/pretrained_detector.py:116). */

/* Number of trunk tensors, in timm state_dict order (names relative to the Sequential,
 * e.g. "2.1.0.conv_dw.weight"; the detector prefixes "backbone."). */
DFD_API int dfd_b0_tensor_count(void);
/* Name (NUL-terminated, truncated to cap), kind, rank and shape (up to 4 dims) of tensor idx. */
DFD_API int dfd_b0_tensor_info(int idx, char* name, int cap, int* kind, int* ndim, int64_t* shape4);

/* Shape-specialised plan for `frames` frames of height x width (dtype DFD_DTYPE_*). */
DFD_API int dfd_b0_plan_create(int frames, int height, int width, int dtype, dfd_b0_plan** out);
DFD_API void dfd_b0_plan_destroy(dfd_b0_plan* plan);
/* Bytes of device workspace one forward(+backward) needs (saved activations + scratch). */
DFD_API int64_t dfd_b0_workspace_bytes(const dfd_b0_plan* plan);
/* Bind element offsets of every tensor (params: into the fp32 parameter buffer; BN buffers:
 * into the fp32 BN buffer; counters ignored).  n must equal dfd_b0_tensor_count(). */
DFD_API int dfd_b0_bind(dfd_b0_plan* plan, const int64_t* offsets, int n);
/* Forward.  x: fp32 frames, element strides x_strides4 = {frame, channel, row, col} (any
 * layout; channels-last input is read in place).  training=1 uses batch statistics and
 * updates running stats with `momentum` (BatchNorm2d train semantics); 0 = eval.
 * features: fp32 [frames][1280].  The workspace keeps what backward needs. */
DFD_API int dfd_b0_forward(dfd_b0_plan* plan, void* stream, const float* x, const int64_t* x_strides4,
                           const float* params, float* bn_buffers, void* workspace, float* features,
                           int training, float momentum);
/* Backward of the same forward (same workspace).  Runs segments [seg_begin, seg_end) in
 * reverse network order: 0 = conv_head+bn2, 1..7 = blocks stage 6..0, 8 = stem.  Gradients
 * are written (accumulate=0) or added (accumulate=1) at the parameter offsets of `grads`. */
DFD_API int dfd_b0_backward(dfd_b0_plan* plan, void* stream, const float* x, const int64_t* x_strides4,
                            const float* dfeatures, const float* params, void* workspace, float* grads,
                            int training, int seg_begin, int seg_end, int accumulate);
/* Input-format variants.  x_format DFD_INPUT_F32: as above.  DFD_INPUT_U8: raw uint8 face crops
 * (the .npz `faces` arrays, data_prepare.py:278-281 / dataset.py:51-81) with the same element
 * strides (e.g. torch.from_numpy(faces).permute(0,3,1,2), app.py:2084), normalised inside the stem
 * as ((v / 255) - mean[c]) / std[c], norm6 = {mean[3], std[3]} -- exactly the fp32 operations of
 * `.float() / 255.0` + imagenet_normalize (app.py:1772-1780); mean 0 / std 1 is the /255-only
 * feed of src/train.py:59.  Both formats give bit-identical results for the same pixels.
 * Calls on one plan from several threads serialise their enqueue (per-plan lock). */
#define DFD_INPUT_F32 0
#define DFD_INPUT_U8 1
DFD_API int dfd_b0_forward_ex(dfd_b0_plan* plan, void* stream, const void* x, int x_format,
                              const int64_t* x_strides4, const float* norm6, const float* params,
                              float* bn_buffers, void* workspace, float* features, int training, float momentum);
DFD_API int dfd_b0_backward_ex(dfd_b0_plan* plan, void* stream, const void* x, int x_format,
                               const int64_t* x_strides4, const float* norm6, const float* dfeatures,
                               const float* params, void* workspace, float* grads, int training, int seg_begin,
                               int seg_end, int accumulate);
/* Per-plan kernel-selection override of a dfd_set_tuning key (INT64_MIN clears it); the
 * process-wide dfd_set_tuning values stay the defaults of plans that set nothing. */
DFD_API int dfd_b0_plan_set_tuning(dfd_b0_plan* plan, const char* key, int64_t value);
DFD_API int dfd_b0_segment_count(void);
/* Introspection of the activations a forward saved in the workspace (pre-BN conv outputs and
 * block outputs, NHWC [rows][cols] in the plan dtype): 0 = conv_stem, then per block
 * (conv_pw (IR only), conv_dw, conv_pwl/conv_pw, block output), last = conv_head.
 * Returns -1 past the end.  Used by the layer-by-layer parity tests. */
DFD_API int dfd_b0_saved_tensor(const dfd_b0_plan* plan, int idx, int64_t* byte_offset, int64_t* rows,
                                int64_t* cols);
/* Introspection of a backward's activation gradient (NHWC [rows][cols], plan dtype): the gradient
 * w.r.t. the INPUT of MBConv block `block` (1..nblocks-1, flat block order), or for block =
 * nblocks w.r.t. the last block's output (the conv_head input).  Valid right after the backward
 * segment that contains that block (the head segment for block = nblocks) and before the next
 * segment runs: the buffers are reused.  Used by the per-stage parity tests. */
DFD_API int dfd_b0_grad_tensor(const dfd_b0_plan* plan, int block, int64_t* byte_offset, int64_t* rows,
                               int64_t* cols);
/* The fused 7x7-stage MBConv forward (bf16 plans, tuning key "mbconv7"): the number of blocks the
 * forward runs as one launch each, and the workspace byte offset of the int32 abort flag those
 * launches raise if their grid-wide barriers found the grid not co-resident (the forward's output is
 * then invalid; the flag is cleared at the start of each training forward).  No reference
 * counterpart: the reference's forward is torch's eager timm module. */
DFD_API int dfd_b0_fused_info(const dfd_b0_plan* plan, int* nblocks, int64_t* abort_offset);
/* Sticky plan status (0 ok, 1 a device-side software barrier timed out -- the split SE excitation's
 * slice barrier, when another stream's kernels held the CUs its grid needed -- and that call's
 * outputs were invalid).  Set by the device in pinned host memory, so reading it needs no device
 * call (synchronise the stream first for a definitive answer).  While it is set, every
 * forward / backward call of the plan fails with dfd_last_error() explaining why; clear it to
 * run again.  Error convention of the reference's callers: app.py:2320-2321 turns the raised error
 * into an error dict. */
DFD_API int dfd_b0_plan_status(const dfd_b0_plan* plan, int* status);
DFD_API int dfd_b0_plan_clear_status(dfd_b0_plan* plan);
/* Test seam: `workgroups` 1024-thread workgroups, each holding a whole CU's LDS, that spin for
 * `microseconds` (wall clock, bounded) on `stream` -- occupies CUs so tests can run the plan next to
 * a kernel that denies it the device (tests/test_se_sync_gpu.py). */
DFD_API int dfd_test_occupy(void* stream, int workgroups, int64_t microseconds);
/* Test seam: `workgroups` (<= CUs) workgroups meet at the software group barrier the split SE excitation
 * uses (csrc/tail.h group_sync), expecting `expected` arrivals within `seconds`: expected > workgroups
 * can never complete, so every waiter must give up -- scratch (>= 3 + workgroups zeroed int32) receives
 * per-workgroup results (1 passed, 2 gave up) at [3 + i], and the barrier raises *host_word (pinned,
 * device-visible host memory), as it raises the plan status (tests/test_se_sync_gpu.py). */
DFD_API int dfd_test_group_sync(void* stream, int workgroups, int expected, double seconds, int* scratch,
                                int* host_word);
/* Test seam: the fp32 convolution launchers (csrc/k_conv.hip conv_forward / conv_dgrad / conv_wgrad) as
 * dfd_rn_train_conv_fwd / dfd_rn_conv_dgrad / dfd_rn_conv_wgrad take them, with a caller-given `fold`
 * (1: the ResNet-50 two-level sums, 0: CNNLSTMHybrid's templates) and, forward only, an optional conv
 * bias[Cout] added to y before the BN partials (NULL: none).  Buffers as for the dfd_rn_* entry points
 * (stats: dfd_rn_conv_stat_rows(N, Ho, Wo) * 2 * Cout floats).  No product path calls these
 * (tests/test_conv_kernels_gpu.py). */
DFD_API int dfd_test_conv_fwd(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin,
                              const float* w, const float* bias, int Cout, int kh, int kw, int stride, int pad,
                              int fold, float* wpack, float* y, float* stats);
DFD_API int dfd_test_conv_dgrad(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w, int Cout,
                                int kh, int kw, int stride, int pad, int fold, float* wpack, float* wpack_t,
                                float* dx);
DFD_API int dfd_test_conv_wgrad(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin,
                                const float* dy, int Cout, int kh, int kw, int stride, int pad, int fold, float* slab,
                                int64_t slab_floats, float* dw);
/* Test seam: the launchers of csrc/k_vit.hip one at a time, exactly as csrc/vit.cpp calls them
 * (tests/test_vit_kernels_gpu.py).  dtype 0 = fp32, 1 = bf16 storage of every `void*` operand.  The caller
 * sizes every buffer; no product path calls these.
 *  bgemm: C[b] (M x N) = alpha * op(A[b]) (M x K) * op(B[b]) (K x N); ta: A stored [k][m], tb: B stored [n][k];
 *         a4 / b4 / c4 = (ld, inner, s_outer, s_inner): batch b sits at (b / inner) * s_outer + (b % inner) *
 *         s_inner elements.  Columns >= N of C are not written.
 *  softmax: rows of n scores in a row pitch ld <= 256; columns [n, ld) of P and of dS are written as 0.
 *  ln_fwd / ln_bwd: C % 8 == 0, C <= 1024; ldx is the row pitch of X, dres and dX, ldy / ldd of Y / dY;
 *         out_f32 / dy_f32 (bf16 only): Y / dY are fp32 (the final norm over the CLS rows).  part: part_cap
 *         floats (>= 2 C), the number of workgroups is at most part_cap / (2 C).
 *  patch_gather: A[(image, patch)][c * 256 + ky * 16 + kx] from a (B, nodes, 3, H, W) fp32 batch with element
 *         strides x_strides5.
 *  tokens_fwd / tokens_bwd: X0[i][t] = (t == 0 ? cls : PE[i][t - 1]) + pos[t] and its backward.
 *  wcast: up to 8 segments src[i] fp32 [rows][cols] -> dst[i] [rows][cols] and / or dst_t[i] [cols][rows]
 *         (either may be NULL).
 *  colsum: out[n] = sum_m X[m][n], N % 8 == 0, at most part_cap / N row splits.
 *  gelu (bf16): mode 0: out = gelu(Z), Z := gelu'(Z); mode 1: out *= Z; n % 8 == 0. */
DFD_API int dfd_test_vit_bgemm(void* stream, int dtype, int ta, int tb, int batch, int M, int N, int K, float alpha,
                               const void* A, const int64_t* a4, const void* B, const int64_t* b4, void* C,
                               const int64_t* c4);
DFD_API int dfd_test_vit_softmax_fwd(void* stream, int dtype, const void* S, void* P, int64_t rows, int n, int ld);
DFD_API int dfd_test_vit_softmax_bwd(void* stream, int dtype, const void* P, const void* dP, void* dS, int64_t rows,
                                     int n, int ld, float scale);
DFD_API int dfd_test_vit_ln_fwd(void* stream, int dtype, int out_f32, const void* X, int64_t ldx, const float* g,
                                const float* b, void* Y, int64_t ldy, float* mean, float* rstd, int64_t rows, int C,
                                float eps);
DFD_API int dfd_test_vit_ln_bwd(void* stream, int dtype, int dy_f32, const void* X, int64_t ldx, const void* dY,
                                int64_t ldd, const float* g, const float* mean, const float* rstd, const void* dres,
                                void* dX, int64_t rows, int C, float* part, int64_t part_cap, float* dgamma,
                                float* dbeta, int accumulate);
DFD_API int dfd_test_vit_patch_gather(void* stream, int dtype, const float* x, const int64_t* x_strides5, int nodes,
                                      int H, int W, int images, void* A);
DFD_API int dfd_test_vit_tokens_fwd(void* stream, int dtype, const void* PE, const float* cls, const float* pos,
                                    int images, int ntok, int D, void* X0);
DFD_API int dfd_test_vit_tokens_bwd(void* stream, int dtype, const void* dX0, int images, int ntok, int D, void* dPE,
                                    float* dpos, float* dcls);
DFD_API int dfd_test_vit_wcast(void* stream, int dtype, int nseg, const float* const* src, void* const* dst,
                               void* const* dst_t, const int* rows, const int* cols);
DFD_API int dfd_test_vit_colsum(void* stream, int dtype, const void* X, int64_t M, int N, float* part,
                                int64_t part_cap, float* out, int accumulate);
DFD_API int dfd_test_vit_gelu(void* stream, void* Z, void* out, int64_t n, int mode);
/* Test seam: float offsets of H1, Y1 (post-ReLU), D1 (after dropout), Y2, G, C1 (post-ReLU), Dc (after dropout)
 * inside the work buffer of dfd_gcn_head_forward (declared below). */
DFD_API int dfd_test_gcn_head_offsets(int B, int N, int feat_dim, int hid, int out, int num_classes,
                                      int64_t* offsets7);
/* Tensor index range [*lo, *hi) whose gradients are final after segment `seg`. */
DFD_API int dfd_b0_segment_tensors(int seg, int* lo, int* hi);

/* Live timing of one launch site (HIP events recorded around it on the launch stream, at most n
 * times).  kind: 0 conv_pw fwd, 1 conv_dw fwd, 2 conv_pwl fwd, 3 conv_dw dgrad, 4 conv_dw wgrad,
 * 5 conv_pw dgrad, 6 conv_pw wgrad, 7 conv_pwl dgrad, 8 conv_pwl wgrad, 9 SE squeeze; (stage, idx) =
 * the MBConv block.  Events are created by arm (not on the launch path); read synchronises on them. */
DFD_API int dfd_b0_probe_arm(dfd_b0_plan* plan, int kind, int stage, int idx, int n);
DFD_API int dfd_b0_probe_read(dfd_b0_plan* plan, float* ms, int cap, int* count);
DFD_API int dfd_b0_probe_disarm(dfd_b0_plan* plan);

/* ---- detector head ---------------------------------------------------------------------
 * Replaces PretrainedBackboneDetector's temporal attention + classifier
 * (src/pretrained_detector.py:65-76 construction, :123-141 forward).
 * params8 / grads8: ta.0.weight, ta.0.bias, ta.2.weight, ta.2.bias, fc1.weight, fc1.bias,
 * fc2.weight, fc2.bias (fp32).  work: fp32 scratch of dfd_head_work_floats() elements that
 * must be kept between forward and backward.  Dropout (p) uses a counter hash of `seed`. */
DFD_API int64_t dfd_head_work_floats(int B, int T, int D, int H, int F1);
DFD_API int dfd_head_forward(void* stream, int B, int T, int D, int H, int F1, int NC, int use_attn,
                             const float* const* params8, const float* features, float* work, uint64_t seed,
                             float p, float* logits, float* frame_scores);
DFD_API int dfd_head_backward(void* stream, int B, int T, int D, int H, int F1, int NC, int use_attn,
                              const float* const* params8, const float* features, float* work, uint64_t seed,
                              float p, const float* frame_scores, const float* dlogits,
                              const float* dframe_scores, float* dfeatures, float* const* grads8);

/* ---- weighted cross entropy --------------------------------------------------------------
 * Replaces nn.CrossEntropyLoss(weight=class_weights) (src/ensemble_trainer.py:358,
 * src/train.py:337): mean of w[y]*nll over non-ignored rows, normalised by sum of w[y]. */
DFD_API int dfd_ce_forward(void* stream, const float* logits, const int64_t* labels, const float* weight, int B,
                           int NC, int64_t ignore_index, float* loss, float* wsum);
DFD_API int dfd_ce_backward(void* stream, const float* logits, const int64_t* labels, const float* weight, int B,
                            int NC, int64_t ignore_index, const float* wsum, const float* grad_out,
                            float* dlogits);

/* ---- focal / label-smoothed classification losses ----------------------------------------
 * Replaces the two criteria of ImprovedTrainer (src/train_improved.py): FocalLoss(gamma, weight,
 * label_smoothing) (:29-78, mode DFD_LOSS_FOCAL; `mean` is the plain mean over the B rows, there is no
 * ignore_index) and nn.CrossEntropyLoss(weight, label_smoothing) (:136-150, mode DFD_LOSS_CE; torch's
 * formula: `mean` divides by the sum of weight[label] over the rows that are not ignore_index, the
 * smoothing term weights every class).  logits (B, C) fp32, 1 <= C <= 1024, labels (B) int64, weight
 * (C) fp32 or NULL.  loss: one float for DFD_REDUCE_MEAN / _SUM, B floats for DFD_REDUCE_NONE.  work:
 * dfd_loss_work_floats(B, C) floats, written by the forward and read by the backward of the same call
 * arguments.  grad_out: the upstream gradient in device memory, one float or B floats alike (never read
 * by the host).  The result is the same bits on every run (fixed-order sums, no atomics).  A row
 * whose label is outside [0, C) (and is not ignore_index in CE mode) reads nothing through the label,
 * gets a NaN loss and a zero gradient.  0 < gamma < 1 with pt rounding to 1 is undefined (inf or NaN
 * gradients), as in the reference. */
#define DFD_LOSS_FOCAL 0
#define DFD_LOSS_CE 1
#define DFD_REDUCE_NONE 0
#define DFD_REDUCE_MEAN 1
#define DFD_REDUCE_SUM 2
DFD_API int64_t dfd_loss_work_floats(int B, int C);
DFD_API int dfd_loss_forward(void* stream, int mode, int reduction, const float* logits, const int64_t* labels,
                             const float* weight, int B, int C, double gamma, double label_smoothing,
                             int64_t ignore_index, float* work, float* loss);
DFD_API int dfd_loss_backward(void* stream, int mode, int reduction, const int64_t* labels, const float* weight,
                              int B, int C, double gamma, double label_smoothing, int64_t ignore_index,
                              const float* work, const float* grad_out, float* dlogits);

/* ---- device-side epoch metrics ------------------------------------------------------------
 * Replaces the per-step bookkeeping of EnsembleTrainer.train_epoch / validate (src/ensemble_trainer.py:
 * 203-211, 266-273: loss.item() and three .cpu() copies per step) and the reductions behind its metrics
 * (:276-329) for a binary classifier with 2 logits.  The caller owns the state: probs (capacity floats),
 * tags (capacity bytes), loss_sums (2 doubles: sum of loss, sum of loss * B), all device memory, and
 * counts the rows it has appended itself.  Neither call allocates, synchronises or copies.
 * dfd_metrics_append: rows offset .. offset + B - 1 get softmax(logits)[1] (fp32) and a tag byte
 * (DFD_METRICS_TAG_*: label, argmax prediction with ties to class 0, labelled); a label other than 0 / 1
 * (-1: unlabelled) is stored and skipped by the finalize.  loss: a device scalar added to loss_sums in
 * stream order, or NULL.  -1 for B <= 0, offset < 0, offset + B > capacity, a null pointer.
 * dfd_metrics_finalize: zeroes result (DFD_METRICS_RESULT_WORDS int64) on the stream and fills it from the
 * first N rows: [0] n_pos [1] n_neg [2] tn [3] fp [4] fn [5] tp [6] U2 = sum over (i positive, j negative)
 * of 2 [p_i > p_j] + [p_i == p_j] (AUC = U2 / (2 n_pos n_neg)) [8 + t] / [40 + t] true / false positives
 * of `prob >= thresholds[t]` in fp32.  thresholds: n_thresholds <= 32 HOST floats.  Integer reductions
 * only: the same bits on every run.  -1 for N < 0, more than 32 thresholds, a null pointer; N == 0 is
 * valid (all zero). */
#define DFD_METRICS_TAG_LABEL 1
#define DFD_METRICS_TAG_PRED 2
#define DFD_METRICS_TAG_VALID 4
#define DFD_METRICS_MAX_THRESHOLDS 32
#define DFD_METRICS_RESULT_WORDS 72
DFD_API int dfd_metrics_append(void* stream, const float* logits, const int64_t* labels, const float* loss, int B,
                               int64_t offset, int64_t capacity, float* probs, uint8_t* tags, double* loss_sums);
DFD_API int dfd_metrics_finalize(void* stream, const float* probs, const uint8_t* tags, int64_t N,
                                 const float* thresholds, int n_thresholds, int64_t* result);

/* ---- serving an ensemble --------------------------------------------------------------------
 * The combination of EnsembleDetector.forward (src/pretrained_detector.py:196-216) and the fp32 values of the
 * app's ensemble decision step (app.py:2090-2094, 2130-2143; the enhanced agent's softmaxes,
 * src/enhanced_decision_agent.py:115-138) for V videos in ONE launch: every member runs once, the host reads
 * one block back per batch.  All device memory, fp32, contiguous:
 *   member_logits (M, V, 2), member_scores (M, V, T), weights (M) the raw ensemble weights (softmax inside) or NULL
 *   logits (V, 2): average = sum over members / M; weighted = sum of logits * softmax(weights); voting = one-hot of
 *     the modal argmax (argmax and mode ties -> class 0, as torch.argmax / torch.mode)
 *   scores (V, T): the weighted sum (weighted) or the mean over members (average, voting)
 *   block (V, dfd_ensemble_decide_floats(M) = 5 + 2M): [0] softmax(logits)[fake_idx] [1] softmax(logits)[1 - fake_idx]
 *     [2] softmax(logits / temperature)[fake_idx] [3] modal argmax of the members [4] M
 *     [5 + m] softmax(member m)[fake_idx] [5 + M + m] softmax(member m / temperature)[fake_idx]
 * -1, with nothing launched, for M outside 1..DFD_ENSEMBLE_MAX_MEMBERS, C != 2, T outside 1..DFD_ENSEMBLE_MAX_FRAMES,
 * V < 1, an unknown method, fake_idx outside {0, 1}, temperature <= 0 or not finite, a null pointer, or
 * DFD_ENSEMBLE_WEIGHTED without weights.  Neither allocates, synchronises nor copies. */
#define DFD_ENSEMBLE_AVERAGE 0
#define DFD_ENSEMBLE_WEIGHTED 1
#define DFD_ENSEMBLE_VOTING 2
#define DFD_ENSEMBLE_MAX_MEMBERS 8
#define DFD_ENSEMBLE_MAX_FRAMES 64
DFD_API int64_t dfd_ensemble_decide_floats(int M);
DFD_API int dfd_ensemble_decide(void* stream, const float* member_logits, const float* member_scores,
                                const float* weights, int M, int64_t V, int C, int T, int method, int fake_idx,
                                float temperature, float* logits, float* scores, float* block);

/* ---- input pipeline ----------------------------------------------------------------------
 * Replaces the frame gather of collate_batch_cnn_lstm / collate_batch (src/train.py:38-61,
 * 62-100): out[s] = src[sel[s]] for s < nsel, frames of frame_bytes uint8 each (sel[s] < 0: an
 * all-zero frame), written as uint8 (out_f32 = 0) or as fp32 v / 255 (out_f32 = 1, the
 * reference's `.float() / 255.0`, bit-identical).  src / out are device pointers. */
DFD_API int dfd_collate_frames(void* stream, const uint8_t* src, const int64_t* sel, int64_t nsel,
                               int64_t frame_bytes, int out_f32, void* out);

/* Train-time augmentation / eval resize of uint8 NHWC face crops (VideoFacesDataset's transforms,
 * src/dataset.py:125-142): a deterministic function of the frame and its row of the two parameter
 * tables, which the HOST draws (deepfake_amd/augment.py).  The JPEG recompression of the train chain
 * is dfd_augment_frames_jpeg below.
 *   params_i32 [n][DFD_AUG_PI]: flags (DFD_AUG_*), crop box top, left, height, width, the four
 *     colour-jitter operations in application order (0 brightness, 1 contrast, 2 saturation, 3 hue),
 *     the hue shift in H code values (0..255), and the (h2, w2) of the downscale/upscale stage;
 *   params_f32 [n][DFD_AUG_PF]: brightness, contrast, saturation factors and the three blur taps.
 * src (n, src_h, src_w, 3), out (n, out_h, out_w, 3) and scratch are device pointers; the two tables
 * are HOST pointers: they are validated here (box inside the source, 1 <= h2 <= max(out_h, 8) and the
 * same for w2, the permutation a permutation, finite factors, blur only on frames of at least 2 x 2,
 * n <= 65535) and a bad table returns -1 before anything is enqueued.  One kernel launch per call. */
#define DFD_AUG_PI 12
#define DFD_AUG_PF 6
#define DFD_AUG_FLIP 1
#define DFD_AUG_JITTER 2
#define DFD_AUG_GRAY 4
#define DFD_AUG_DOWNUP 8
#define DFD_AUG_BLUR 16
DFD_API int64_t dfd_augment_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w);
/* 1: the working image of this shape stays in LDS; 0: it goes through the scratch; -1: bad shape */
DFD_API int dfd_augment_lds_resident(int src_h, int src_w, int out_h, int out_w);
DFD_API int dfd_augment_frames(void* stream, const uint8_t* src, int n, int src_h, int src_w,
                               const int32_t* params_i32, const float* params_f32, int out_h, int out_w,
                               uint8_t* out, void* scratch, int64_t scratch_bytes);
/* The same chain with the reference's JPEG recompression (_RandomJPEGCompression, src/dataset.py:83-105)
 * between the downscale/upscale and the blur, in the same single launch: quality[n] (HOST pointer) holds
 * 0 (stage off for that frame) or the quality 1..100; a frame with a quality comes out byte for byte as
 * Pillow's save(format='JPEG', quality=q, optimize=True) + open().convert('RGB') (libjpeg-turbo, baseline,
 * 4:2:0) returns it.  The tables follow dfd_augment_frames' rules (flag bits above DFD_AUG_BLUR stay
 * unknown: the quality is no flag); a quality outside 0..100 returns -1 before anything is enqueued.
 * The scratch also holds the qualities: size it with dfd_augment_jpeg_scratch_bytes. */
DFD_API int64_t dfd_augment_jpeg_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w);
DFD_API int dfd_augment_frames_jpeg(void* stream, const uint8_t* src, int n, int src_h, int src_w,
                                    const int32_t* params_i32, const float* params_f32, const int32_t* quality,
                                    int out_h, int out_w, uint8_t* out, void* scratch, int64_t scratch_bytes);

/* ---- ResNet-50 ensemble member, inference (src/pretrained_detector.py:37-40 -> torchvision
 * resnet50 children[:-1]; EnsembleDetector default ENSEMBLE_BACKBONES, app.py:661,1597).  NHWC
 * activations, dtype 0 = fp32, 1 = bf16.  Every convolution is dfd_rn_conv, an implicit-GEMM MFMA
 * kernel with the eval BatchNorm folded into weights + bias (conv1: dfd_rn_gemm over the stem
 * gather).  No library GEMM on this path. ---- */
/* NHWC x (N,H,W,C) -> rows [N*Ho*Wo][Kp], column (ky*kw + kx)*C + c, zero padding; C % 8 == 0 */
DFD_API int dfd_rn_im2col(void* stream, int dtype, const void* x, int N, int H, int W, int C, int kh, int kw,
                          int stride, int pad, int Kp, void* out);
/* conv1 7x7/2 pad 3 rows of the (N,3,H,W) frames (element strides4; DFD_INPUT_F32 or DFD_INPUT_U8 with
 * norm6 = mean[3], std[3]) -> [N*Ho*Wo][152] (147 taps + zero padding) */
DFD_API int dfd_rn_stem_im2col(void* stream, int dtype, const void* x, int input_fmt, const int64_t* strides4,
                               const float* norm6, int N, int H, int W, void* out);
/* conv1 + its folded BN + ReLU in one implicit-GEMM launch (bf16 only; the output map's sides multiples
 * of 16): the frames as for dfd_rn_stem_im2col, w [64][152] bf16 (the im2col column order), bias[64]
 * fp32, out NHWC (N, Ho, Wo, 64) bf16 -- the rows of dfd_rn_stem_im2col never reach HBM. */
DFD_API int dfd_rn_stem_conv(void* stream, int dtype, const void* x, int input_fmt, const int64_t* strides4,
                             const float* norm6, int N, int H, int W, const void* w, const float* bias, void* out);
/* C[M][N] = relu?(A[M][K] . B[N][K]^T + bias[N] (+ R[M][N])), fp32 accumulate (the MFMA kernel of
 * dfd_rn_conv on an explicit A; K % 8 == 0) */
DFD_API int dfd_rn_gemm(void* stream, int dtype, const void* A, const void* B, void* C, const void* R,
                        const float* bias, int relu, int64_t M, int N, int K);
/* One folded convolution + BN (+ identity) (+ ReLU) of torchvision's Bottleneck / downsample
 * (resnet.py:Bottleneck.forward): x NHWC (N,H,W,Cin) -> out NHWC (N,Ho,Wo,Cout),
 * out = relu?(conv(x, w) + bias (+ res)); w [Cout][kh*kw*Cin] (column (ky*kw + kx)*Cin + c);
 * Cin a power of two >= 8 unless kh = kw = stride = 1; kw 1 or 3.  bf16 with Cin % 64 == 0 and
 * Cout % 128 == 0 runs on the LDS-DMA NT GEMM of dfd_vgemm (1x1 stride 1: plain rows; 3x3 and strided:
 * per-tap implicit A gather) and rounds once (fp32 acc + bias + res, ReLU); the implicit-GEMM kernel
 * rounds acc + bias before adding res (bf16(bf16(acc + bias) + res)). */
DFD_API int dfd_rn_conv(void* stream, int dtype, const void* x, int N, int H, int W, int Cin, int kh, int kw,
                        int stride, int pad, const void* w, const float* bias, const void* res, int relu, int Cout,
                        void* out);
/* 3x3/2 pad 1 max pooling, NHWC, C % 8 == 0 */
DFD_API int dfd_rn_maxpool(void* stream, int dtype, const void* x, int N, int H, int W, int C, void* out);
/* global average pooling (N, HW, C) -> (N, C) fp32 */
DFD_API int dfd_rn_avgpool(void* stream, int dtype, const void* x, int N, int HW, int C, float* out);

/* ---- ResNet-50 ensemble member, TRAINING, fp32 (EnsembleTrainer.train_epoch trains every member:
 * src/ensemble_trainer.py:158-229; torchvision train-mode BatchNorm2d semantics).  NHWC fp32; the
 * convolutions are exact-fp32 implicit-GEMM MFMA kernels (no im2col buffer, no library GEMM). ---- */
/* BN-stat partial rows a training conv forward writes: stats needs rows * 2 * Cout floats */
DFD_API int64_t dfd_rn_conv_stat_rows(int N, int Ho, int Wo);
/* y (N,Ho,Wo,Cout) = conv(x, w) without bias, and the BN-stat partials of y's channels: per 64-row
 * tile of y, [sum][Cout] then [M2][Cout] (M2 = sum of squared deviations from the tile's own mean;
 * dfd_rn_bn_train_finalize merges the tiles in fp64); x read through element strides
 * xs4 = (n, y, x, c); w OIHW [Cout][Cin][kh][kw]; wpack >= Cout*Cin*kh*kw */
DFD_API int dfd_rn_train_conv_fwd(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin,
                                  const float* w, int Cout, int kh, int kw, int stride, int pad, float* wpack,
                                  float* y, float* stats);
/* batch mean / invstd / scale / shift of a train-mode BN from dfd_rn_train_conv_fwd's partials
 * (Chan's merge of the tiles' (count, mean, M2)); updates running_mean / running_var with momentum
 * (unbiased variance), like torch */
DFD_API int dfd_rn_bn_train_finalize(void* stream, const float* stats, int rows, int64_t count, int C,
                                     const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, float momentum, float eps, float* mean, float* invstd,
                                     float* scale, float* shift);
/* out = relu?((y - mean) * scale + beta (+ res)), (M, C), C % 4 == 0 -- torch's centred order of
 * operations (scale = gamma * invstd from dfd_rn_bn_train_finalize, beta = the BN bias) */
DFD_API int dfd_rn_bn_act(void* stream, const float* y, const float* mean, const float* scale, const float* beta,
                          const float* res, int relu, int64_t M, int C, float* out);
/* stem: out = maxpool3x3/2(relu((y - mean) * scale + beta)) with the argmax tap kept; and its backward
 * to the BN output gradient g (relu' included) */
DFD_API int dfd_rn_pool_train_fwd(void* stream, const float* y, const float* mean, const float* scale,
                                  const float* beta, int N, int H, int W, int C, float* out, uint8_t* argmax);
DFD_API int dfd_rn_pool_train_bwd(void* stream, const float* dout, const uint8_t* argmax, const float* y,
                                  const float* mean, const float* scale, const float* beta, int N, int H, int W, int C,
                                  float* g);
/* g = out > 0 ? dout : 0 (n % 4 == 0);  global-average-pool backward through the last ReLU:
 * g[n][p][c] = out > 0 ? dfeat[n][c] / HW : 0 */
DFD_API int dfd_rn_relu_bwd(void* stream, const float* dout, const float* out, int64_t n, float* g);
DFD_API int dfd_rn_gap_bwd(void* stream, const float* dfeat, const float* out, int N, int HW, int C, float* g);
/* train-mode BN backward from its output gradient g: dgamma, dbeta (written) and
 * dy = k1*g + k2*(y - mean) + k3 (centred);
 * stats >= 2048*2*C floats, coef >= 3*C floats (scratch) */
DFD_API int dfd_rn_bn_train_bwd(void* stream, const float* g, const float* y, int64_t M, int C, const float* mean,
                                const float* invstd, const float* scale, const float* shift, const float* gamma,
                                float* dgamma, float* dbeta, float* stats, float* coef, float* dy);
/* the same from the gradient da of the ReLU that follows the BN (its saved output relu_out): g =
 * (relu_out > 0) * da is folded into the reduction and the apply pass, never stored; C % 64; stats >= 512
 * rows x 2 x C floats */
DFD_API int dfd_rn_bn_train_bwd_relu(void* stream, const float* da, const float* relu_out, const float* y, int64_t M,
                                     int C, const float* mean, const float* invstd, const float* gamma,
                                     float* dgamma, float* dbeta, float* stats, float* coef, float* dy);
/* dx (N,H,W,Cin) = conv data gradient of dy (N,Ho,Wo,Cout), stride 1 or 2; wpack, wpack_t scratch of
 * Cout*Cin*kh*kw floats each */
DFD_API int dfd_rn_conv_dgrad(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w, int Cout,
                              int kh, int kw, int stride, int pad, float* wpack, float* wpack_t, float* dx);
/* the same with dx = data gradient + res (the bottleneck's identity / downsample path, (N,H,W,Cin)) added
 * in the epilogue; Cin, Cout % 64 (the shapes of the fp32 tile loops) */
DFD_API int dfd_rn_conv_dgrad_res(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w,
                                  int Cout, int kh, int kw, int stride, int pad, float* wpack, float* wpack_t,
                                  const float* res, float* dx);
/* the slab size (floats) dfd_rn_conv_wgrad uses in full for this shape (its pixel splits x |dw|; a
 * smaller slab runs fewer splits) */
DFD_API int64_t dfd_rn_conv_wgrad_slab_floats(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride,
                                              int pad);
/* dw OIHW (written) = weight gradient from x (strides xs4) and dy; slab: scratch of slab_floats */
DFD_API int dfd_rn_conv_wgrad(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin,
                              const float* dy, int Cout, int kh, int kw, int stride, int pad, float* slab,
                              int64_t slab_floats, float* dw);

/* ---- ResNet-50 ensemble member: bf16 TRAINING (k_rn16.hip) -----------------------------------
 * Replaces the same train-mode trunk as dfd_rn_train_* (torchvision resnet50 children()[:-1] under
 * EnsembleTrainer.train_epoch, src/ensemble_trainer.py:158-229, src/pretrained_detector.py:37-40) for
 * every bottleneck convolution (1x1 / 3x3, stride 1 / 2, pad (k-1)/2, Cin % 64, Cout % 64): bf16 NHWC
 * activations, v_mfma_f32_16x16x32_bf16 with fp32 accumulation, fp32 master weights packed per step,
 * BN statistics in fp32 partials merged in fp64.  conv1 + bn1 + relu + maxpool stay on dfd_rn_train_*.
 * w OIHW fp32 -> wf [Cout][k][k][Cin] bf16 (forward), wd [Cin][k][k][Cout] bf16 (data gradient, or null) */
DFD_API int dfd_rn16_pack_weights(void* stream, const float* w, int Cout, int Cin, int k, void* wf, void* wd);
/* every convolution of a step in one launch: table = n device rows of int64 {w (fp32 OIHW pointer), Cout, Cin, k*k,
 * wf offset, wd offset or -1} (offsets in bf16 elements of out); max_elems = the largest Cout*Cin*k*k */
DFD_API int dfd_rn16_pack_all(void* stream, const int64_t* table, int n, int64_t max_elems, void* out);
/* y = conv(x) NHWC bf16 (no bias); BN partial rows (sum, sum of squares) into stats (>= 2048*Cout floats),
 * *stat_rows rows, for dfd_rn16_bn_finalize */
DFD_API int dfd_rn16_conv_fwd(void* stream, const void* x, int N, int H, int W, int Cin, const void* wf, int Cout,
                              int k, int stride, int pad, void* y, float* stats, int* stat_rows);
/* train-mode BN of dfd_rn16_conv_fwd's output: batch mean / invstd, scale = gamma*invstd, shift, the running
 * buffers updated like torch (unbiased variance, momentum) */
DFD_API int dfd_rn16_bn_finalize(void* stream, const float* stats, int rows, int64_t count, int C, const float* gamma,
                                 const float* beta, float* running_mean, float* running_var, float momentum,
                                 float eps, float* mean, float* invstd, float* scale, float* shift);
/* out = relu?((y - mean) * scale + beta (+ res)), bf16 in / out */
DFD_API int dfd_rn16_bn_act(void* stream, const void* y, const float* mean, const float* scale, const float* beta,
                            const void* res, int relu, int64_t M, int C, void* out);
DFD_API int dfd_rn16_relu_bwd(void* stream, const void* dout, const void* out, int64_t n, void* g);
DFD_API int dfd_rn16_gap_bwd(void* stream, const float* dfeat, const void* out, int N, int HW, int C, void* g);
/* train-mode BN backward (centred), bf16 g / y / dy; dgamma, dbeta written; stats >= 2048*2*C, coef >= 3*C;
 * relu_out (or null; C % 64): the saved output of the ReLU after this BN, g is masked by it inline */
DFD_API int dfd_rn16_bn_train_bwd(void* stream, const void* g, const void* relu_out, const void* y, int64_t M, int C,
                                  const float* mean, const float* invstd, const float* scale, const float* shift,
                                  const float* gamma, float* dgamma, float* dbeta, float* stats, float* coef,
                                  void* dy);
/* dx [N][H][W][Cin] bf16 = transposed conv of dy [N][Ho][Wo][Cout] (+ res, same shape as dx) */
DFD_API int dfd_rn16_conv_dgrad(void* stream, const void* dy, int N, int H, int W, int Cin, const void* wd, int Cout,
                                int k, int stride, int pad, const void* res, void* dx);
DFD_API int64_t dfd_rn16_conv_wgrad_slab_floats(int N, int H, int W, int Cin, int Cout, int k, int stride, int pad);
/* dw OIHW fp32 (written) from x and dy (bf16 NHWC); slab: scratch of slab_floats */
DFD_API int dfd_rn16_conv_wgrad(void* stream, const void* x, int N, int H, int W, int Cin, const void* dy, int Cout,
                                int k, int stride, int pad, float* slab, int64_t slab_floats, float* dw);
/* n elements (n % 8 == 0): fp32 -> bf16 (to_bf16 = 1) or bf16 -> fp32 */
DFD_API int dfd_rn16_cast(void* stream, const void* src, int to_bf16, int64_t n, void* dst);

/* ---- optimizer ----------------------------------------------------------------------------
 * Replaces torch.nn.utils.clip_grad_norm_(params, max_norm) (src/ensemble_trainer.py:199) and
 * optim.AdamW / optim.Adam .step() (src/ensemble_trainer.py:146,200; src/train.py:323,126)
 * over one flat fp32 buffer.  out2[0] = total norm, out2[1] = clip coefficient.
 * scratch: >= 8192 bytes of device memory. */
DFD_API int dfd_grad_norm(void* stream, const float* grads, int64_t n, float max_norm, void* scratch, float* out2);
DFD_API int dfd_adam_step(void* stream, float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                          double grad_scale, int decoupled, const float* clip_out2);
/* Dynamic loss scaling for fp16 training (replaces torch.cuda.amp.GradScaler's scale / unscale_ /
 * step / update around the same step; no host synchronisation).  scaler_state: 4 device floats
 * [scale, growth tracker, found_inf, applied steps].  The gradient is the SCALED one (the loss was
 * multiplied by scale before backward).  dfd_grad_norm_scaled: as dfd_grad_norm, the norm unscaled
 * and found_inf = (norm not finite).  dfd_adam_step_scaled: as dfd_adam_step on grads / scale (written
 * back unscaled, and clipped with clip_out2), skipped entirely when found_inf; bias corrections from
 * applied steps + 1.  dfd_loss_scale_update: scale *= backoff on found_inf, else *= growth after
 * growth_interval finite steps in a row; counts the applied steps. */
DFD_API int dfd_grad_norm_scaled(void* stream, const float* grads, int64_t n, float max_norm, float* scaler_state,
                                 void* scratch, float* out2);
DFD_API int dfd_adam_step_scaled(void* stream, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                 int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 double grad_scale, int decoupled, const float* clip_out2, const float* scaler_state);
DFD_API int dfd_loss_scale_update(void* stream, float* scaler_state, double growth_factor, double backoff_factor,
                                  int growth_interval);

/* Kernel-selection knobs (process-wide; returns the previous value, -1 for an unknown key).
 * "stream_min_rows": bf16 1x1 convs with at least this many rows use the streaming kernel
 * (default 100000; 0 routes every covered shape there, a huge value routes none).
 * "fold_min_rows": IR blocks whose conv_pw has at least this many rows run its backward through
 * the BN-folded form (no materialised BN input gradient; default 100000).
 * "dw_bwd_fused": 1 (default) runs the depthwise input and weight gradients as one fused pass,
 * 0 as two kernels.
 * "gemm_tile": tile of the (non-streaming) 1x1-conv GEMM: 0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 32x64,
 * -1 (default) = chosen per shape. */
DFD_API int64_t dfd_set_tuning(const char* key, int64_t value);

/* ---- pointwise (1x1) convolution, the trunk's conv_pw / conv_pwl / conv_head kernels ----------
 * Replaces aten conv2d(kernel_size=1, bias=False) on NHWC activations as timm's MBConv blocks
 * run it inside self.backbone(x_flat) (src/pretrained_detector.py:116), with the producing
 * layer's BatchNorm+SiLU (+ squeeze-excite gate) applied to the input on the fly:
 *   C[M][N] = pro(A)[M][K] . W[N][K]^T (+ R[M][N])
 *   pro_mode 0: a = x;  1: a = silu(x*scale[k] + shift[k]);  2: the same times gate[m / rows_per_frame][k];
 *   4: a = x * gate[m / rows_per_frame][k] (x already activated).
 * dtype DFD_DTYPE_F32 (fp32 storage), DFD_DTYPE_BF16 or DFD_DTYPE_F16 (16-bit storage); fp32 accumulation; N, K
 * multiples of 8.  stats (optional, R must then be NULL): per-column partial sums of C and C^2 in
 * rows [*stat_rows][2][N] (room for 1024*2*N floats).  Used by the trunk and the kernel tests. */
DFD_API int dfd_pw_conv(void* stream, int dtype, const void* A, const void* W, void* C, const void* R, int64_t M,
                        int N, int K, int pro_mode, const float* scale, const float* shift, const float* gate,
                        int rows_per_frame, float* stats, int* stat_rows);
/* Weight gradient of the same conv: dW[N][K] (=, or += if accumulate) sum_m dY[m][n] * pro(X)[m][k],
 * fp32 output; slab: fp32 scratch of slab_floats >= N*K (deterministic split-M partials). */
DFD_API int dfd_pw_conv_wgrad(void* stream, int dtype, const void* dY, const void* X, int64_t M, int N, int K,
                              int pro_mode, const float* scale, const float* shift, const float* gate,
                              int rows_per_frame, float* slab, int64_t slab_floats, float* dW, int accumulate);

/* Fused multi-head attention (bf16, head dim 64, nt <= 256; test seam of the ViT trunk's attention,
 * timm Attention as run by ViTFeatureExtractor, src/models.py:88-107).  qkv: bf16 rows of nt tokens per
 * image, head h's q / k / v at columns h*64 / koff + h*64 / voff + h*64 (row stride ldq); O [rows][ldo]
 * bf16; lse [images*heads][nt] fp32.  backward = 0: O, lse from qkv.  backward = 1: dqkv (qkv's
 * layout, row stride lddq) from qkv, O, lse and dO [rows][lddo]. */
DFD_API int dfd_attention(void* stream, int backward, int images, int heads, int nt, float scale, const void* qkv,
                          int64_t ldq, int koff, int voff, void* O, int64_t ldo, float* lse, const void* dO,
                          int64_t lddo, void* dqkv, int64_t lddq);

/* The ViT trunk's large bf16 GEMMs (k_vgemm.hip; test / measurement seam): op 0 (NT):
 * C[M][N] (bf16) = A[M][K] . B[N][K]^T with the epilogue mask epi (applied in this order, fp32, one
 * rounding): 1 + bias[N] (fp32), 2 + R[M][N], 16 ReLU; 4 (GELU pair, with 1): with z the bf16-rounded
 * pre-activation, G = gelu(z) and C = gelu'(z) -- C does NOT keep the pre-activation; 8: C *= Z[M][N]
 * elementwise, Z being the derivative an epi-4 launch stored in its C (the MLP backward's x gelu').
 * Instantiated masks: 0, 1, 1|2, 1|4, 8, 1|16, 1|2|16.  K % 64 == 0 and N % 128 == 0, except that
 * N % 64 == 0 (the 64-wide tile) is accepted with the masks 0, 1, 1|2, 1|16, 1|2|16 only.  The
 * tile width (256, 128 or 64 columns) is chosen by shape; ops 4 / 5 / 7 force 256 (N % 256 == 0) /
 * 128 / 64.
 * op 1 (TN): C (fp32 [N][K]) = A^T . B for A [M][N], B [M][K] (bf16), split over M into slab
 * (>= dfd_vgemm_tn_slab_floats) and summed in a fixed order; N, K % 256 == 0; with G non-null also
 * G (fp32 [N]) = the column sums of A (a linear's bias gradient) from the same launch.  op 6: op 1 with
 * the split partials reduced inside the launch (the ViT backward's form: the splits of a 256 x 256 tile
 * meet at a group barrier and each sums its share of the tile's rows over all splits in split order;
 * used when the grid fits the device at once, else op 1's separate reductions); needs 2 x (N/256) x
 * (K/256) + 64 floats of slab beyond op 1's, taken from the slab's end.  ops 2 / 3: the same products
 * through hipBLASLt (measurement comparison only; op 2 takes epi 0..3). */
DFD_API int dfd_vgemm(void* stream, int op, const void* A, const void* B, void* C, const void* R, const float* bias,
                      const void* Z, void* G, int64_t M, int N, int K, int epi, float* slab, int64_t slab_floats);
DFD_API int64_t dfd_vgemm_tn_slab_floats(int64_t M, int N, int K);
/* hipBLASLt calls made so far in this process (only dfd_vgemm ops 2 / 3 make any) */
DFD_API int64_t dfd_blaslt_calls(void);

/* fp32 GEMM of the recurrent models' plain products (test seam): C[m][n] = beta*C + sum_k A(m,k) B(n,k)
 * (+ bias[n]); A(m,k) = ta ? A[k*lda+m] : A[m*lda+k], B(n,k) = tb ? B[k*ldb+n] : B[n*ldb+k].  The
 * kernels behind nn.Linear / nn.LSTM input projections and weight gradients of LogicRNNLSTM,
 * CNNLSTMHybrid and the GCN head (no reference counterpart: torch's own GEMMs there). */
DFD_API int dfd_sgemm(void* stream, int ta, int tb, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                      int M, int N, int K, float beta, const float* bias);

/* ---- LogicRNNLSTM (src/RNNModel.py:43-147), fp32 ----
 * Replaces LogicRNNLSTM.forward (RNNModel.py:81-133) and its autograd backward.
 * x: (B, T, IN) fp32 contiguous.  order: the reference's sort_idx of lengths.sort(0, descending=True)
 * (RNNModel.py:92-95; B int64) or NULL when lengths is None; lengths: the SORTED lengths (B int64)
 * or NULL.  The output stays in sorted order, exactly like the reference (it never un-sorts).
 * params / grads: 14*L + 8 fp32 pointers in named_parameters() order: per layer
 * {and,or,not,forget,input,cell,output}_gate.{weight,bias}, then attention.{0,2}.{weight,bias},
 * classifier.{0,3}.{weight,bias}.  y: (B) = sigmoid output.  p: dropout probability (0 in eval),
 * seed: counter-hash dropout seed (must match between forward and backward).
 * work: dfd_rnn_work_floats() floats kept from forward to backward; scratch: dfd_rnn_scratch_floats(). */
DFD_API int64_t dfd_rnn_work_floats(int B, int T, int IN, int H, int L);
DFD_API int64_t dfd_rnn_scratch_floats(int B, int T, int IN, int H, int L);
DFD_API int dfd_rnn_forward(void* stream, int B, int T, int IN, int H, int L, const float* x, const int64_t* order,
                            const int64_t* lengths, float* const* params, float* work, float* y, uint64_t seed,
                            float p);
/* dy: (B) gradient of y; writes (overwrites) every parameter gradient. */
DFD_API int dfd_rnn_backward(void* stream, int B, int T, int IN, int H, int L, const float* x, const int64_t* order,
                             const int64_t* lengths, float* const* params, float* work, float* scratch,
                             const float* dy, float* const* grads, uint64_t seed, float p);

/* ---- CNNLSTMHybrid (src/models.py:20-85), fp32 ----
 * Replaces CNNLSTMHybrid.forward (models.py:72-85) and its autograd backward: frame CNN
 * (4 conv+BN+ReLU, 3 maxpools, GAP), nn.LSTM(512, hidden, layers, dropout, batch_first),
 * attention pooling, classifier.  x: (B*T, 3, H, W) fp32 with element strides x_strides4
 * (n, c, h, w) -- channels-last strides are fine.  params / grads: 16 + 4*layers + 8 pointers in
 * named_parameters() order (cnn.{0,1,4,5,8,9,12,13}.{weight,bias}, lstm.{weight_ih,weight_hh,
 * bias_ih,bias_hh}_l{k}, attention.{0,2}.*, classifier.{0,3}.*); bn_running: 8 pointers
 * cnn.{1,5,9,13}.{running_mean,running_var} (updated in training, momentum as given, eps 1e-5).
 * logits: (B, num_classes).  work: dfd_cnnlstm_work_floats() kept from forward to backward. */
DFD_API int64_t dfd_cnnlstm_work_floats(int B, int T, int H, int W, int hidden, int layers, int num_classes);
DFD_API int64_t dfd_cnnlstm_scratch_floats(int B, int T, int H, int W, int hidden, int layers, int num_classes);
DFD_API int dfd_cnnlstm_forward(void* stream, int B, int T, int H, int W, int hidden, int layers, int num_classes,
                                const float* x, const int64_t* x_strides4, float* const* params,
                                float* const* bn_running, float* work, int training, float momentum, uint64_t seed,
                                float p, float* logits);
/* dlogits: (B, num_classes); writes (overwrites) every parameter gradient. */
DFD_API int dfd_cnnlstm_backward(void* stream, int B, int T, int H, int W, int hidden, int layers, int num_classes,
                                 const float* x, const int64_t* x_strides4, float* const* params, float* work,
                                 float* scratch, int training, uint64_t seed, float p, const float* dlogits,
                                 float* const* grads);

/* ---------------- DeepfakeModel: ViT-B/16 trunk + SimpleGCN head (C5) ----------------
 * Replaces ViTFeatureExtractor.forward (src/models.py:88-107: timm vit_base_patch16_224,
 * num_classes=0 -> CLS features after the final norm) and SimpleGCN + pooling + classifier
 * (src/models.py:199-219, 280-291), forward and backward (train.py:104-133 trains it).
 * dtype 0 = fp32 storage (parity), 1 = bf16 storage; fp32 accumulation.  depth 12 is the
 * reference's model (smaller depths only for tests).  Images: 224x224, fp32, element strides
 * x_strides5 = (b, n, c, h, w) of a (B, N, 3, H, W) tensor; images = B*N.
 * params: dfd_vit_param_count(depth) pointers in timm named_parameters() order (cls_token,
 * pos_embed, patch_embed.proj.{weight,bias}, blocks.{i}.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,
 * mlp.fc2}.{weight,bias}, norm.{weight,bias}).  feats: (images, 768) fp32.
 * work (dfd_vit_work_bytes) is kept from forward to backward; backward overwrites grads. */
DFD_API int dfd_vit_param_count(int depth);
DFD_API int64_t dfd_vit_work_bytes(int dtype, int depth, int images, int height, int width);
DFD_API int64_t dfd_vit_scratch_bytes(int dtype, int depth, int images, int height, int width);
DFD_API int dfd_vit_forward(void* stream, int dtype, int depth, int images, int nodes, int height, int width,
                            const float* x, const int64_t* x_strides5, const float* const* params, void* work,
                            float* feats);
/* dfd_vit_forward with keep_backward = 0: an inference forward -- the bf16 fc1 epilogue stores
 * gelu(pre) alone, not the GELU derivative the backward reads (12 x images*197 x 3072 bf16 fewer
 * bytes written); feats are bit-identical to dfd_vit_forward's.  dfd_vit_backward must not follow it.
 * keep_backward = 1 is dfd_vit_forward. */
DFD_API int dfd_vit_forward_ex(void* stream, int dtype, int depth, int images, int nodes, int height, int width,
                               const float* x, const int64_t* x_strides5, const float* const* params, void* work,
                               float* feats, int keep_backward);
DFD_API int dfd_vit_backward(void* stream, int dtype, int depth, int images, int height, int width,
                             const float* const* params, void* work, void* scratch, const float* dfeats,
                             float* const* grads);
/* GCN head: feats (B*N, feat_dim) -> H = A_norm @ feats -> relu(fc1) -> dropout(p) -> relu(fc2) ->
 * mean over N -> classifier Linear(out,64) / ReLU / Dropout(p) / Linear(64, classes).
 * params (8): gcn.fc1.{weight,bias}, gcn.fc2.{weight,bias}, classifier.0.*, classifier.3.*.
 * Dropout: the library's counter hash (streams 40, 41), p applied only when training. */
DFD_API int64_t dfd_gcn_head_work_floats(int B, int N, int feat_dim, int hid, int out, int num_classes);
DFD_API int64_t dfd_gcn_head_scratch_floats(int B, int N, int feat_dim, int hid, int out, int num_classes);
DFD_API int dfd_gcn_head_forward(void* stream, int B, int N, int feat_dim, int hid, int out, int num_classes,
                                 const float* feats, const float* a_norm, const float* const* params, float* work,
                                 int training, uint64_t seed, float p, float* logits);
DFD_API int dfd_gcn_head_backward(void* stream, int B, int N, int feat_dim, int hid, int out, int num_classes,
                                  const float* a_norm, const float* const* params, const float* work,
                                  float* scratch, int training, uint64_t seed, float p, const float* dlogits,
                                  float* const* grads, float* dfeats);

#ifdef __cplusplus
}
#endif
#endif /* DFD_HIP_H */
