/*
 * cotr_hip.h - C ABI of libcotr_hip.so: the MI355X (gfx950) implementation of COTR's
 * batched correspondence-query forward path.
 *
 * The reference (ubc-vision/COTR) has no FFI: its seam is the Python call
 *     COTR.forward(samples, queries) -> {'pred_corrs'}      (COTR/models/cotr_model.py:26-40)
 * made by SparseEngine.infer_batch (COTR/inference/sparse_engine.py:47-56),
 * FasterSparseEngine.infer_batch_grouped (:277-282), cotr_patch_flow_exhaustive
 * (COTR/inference/inference_helper.py:106-145) and cotr_corr_base (:186-204).
 * This header is what a binding for that seam binds to; cotr_amd/models (ctypes) is
 * the binding this repository ships, INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - plain C, no exceptions; every call returns COTR_OK (0) or a negative COTR_ERR_* and
 *    leaves a message retrievable with cotr_last_error().
 *  - all tensors are fp32, contiguous; `img`, `queries`, `out` are DEVICE pointers owned by
 *    the caller (torch tensors' data_ptr()); weight pointers may be host or device.
 *  - `stream` is a hipStream_t (NULL = the default stream).  All work is enqueued on it;
 *    nothing synchronises the device except cotr_load_weights / cotr_destroy / cotr_debug_tap.
 *  - packed weights and scratch live in memory owned by the handle (grow-only arenas).
 *  - one handle per device per caller thread; a handle is not thread-safe.  Handles on different
 *    devices may coexist in one process: every call makes its handle's device current for its
 *    duration and restores the caller's current device before returning; one-time kernel
 *    attributes and helper buffers are kept per device.
 *  - a NaN in the inputs/weights yields NaN outputs, never a trap: the reference's engines
 *    raise ValueError('NaN in prediction') themselves (sparse_engine.py:54-55).
 *
 * Model geometry is COTR's default and only published configuration
 * (COTR/options/options.py:41-51): resnet50 to layer3, hidden 256, 8 heads, FFN 1024,
 * lin_sine; the number of encoder/decoder layers is read from the weight names.
 */
#ifndef COTR_HIP_H
#define COTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden and linked with a version script made from this header (cotr_amd/build.py): the
 * functions declared here are its ONLY dynamic symbols. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define COTR_HIP_ABI_VERSION 2   /* 2: tuning knobs per handle (cotr_set_knob(h, ...)), the cotr_set_<knob>(int) functions are gone;
                                  cotr_train_attention_bwd takes a scratch argument; experiments live in libcotr_hip_exp.so */

#define COTR_OK 0
#define COTR_ERR_ARG (-1)    /* bad argument (null pointer, bad shape)                     */
#define COTR_ERR_HIP (-2)    /* a HIP runtime call failed; see cotr_last_error()            */
#define COTR_ERR_STATE (-3)  /* weights not loaded / decode without a matching encode       */
#define COTR_ERR_WEIGHTS (-4) /* a required tensor is missing or has the wrong element count */

typedef struct cotr_ctx* cotr_handle;
typedef void* cotr_stream; /* hipStream_t */

int cotr_abi_version(void);

/* Per-device context.  Replaces: model = build_model(opt).cuda()  (demo_single_pair.py:26-27) */
int cotr_create(cotr_handle* out, int device);
void cotr_destroy(cotr_handle h);
const char* cotr_last_error(cotr_handle h); /* h may be NULL: last error of cotr_create */

/* Load a state-dict: n tensors, names as in the reference's checkpoints
 * ('backbone.0.body.layer1.0.conv1.weight', 'transformer.encoder.layers.0.self_attn.in_proj_weight',
 * ...; full table: cotr_amd/models/spec.py).  Re-lays-out conv weights to [Cout][kh][kw][Cin],
 * folds the four FrozenBN buffers into (scale, bias) exactly as COTR/models/backbone.py:46-56
 * computes them, concatenates the decoder K/V projections.  Unknown names are ignored
 * (e.g. decoder norm1, never applied: COTR/models/transformer.py:173,185-201).
 * Replaces: utils.safe_load_weights(model, weights)  (COTR/utils/utils.py:164-193). */
int cotr_load_weights(cotr_handle h, const char* const* names, const float* const* ptrs,
                      const int64_t* numels, int n);

/* Query-independent half: backbone on both 256x256 halves, input_proj, 6 encoder layers and the
 * K/V projections of every decoder layer; result cached in the handle for cotr_decode.
 * img: [B,3,256,512] NCHW, ImageNet-normalised side-by-side pair.
 * Follows COTR/models/backbone.py:79-92,114-123, cotr_model.py:37, transformer.py:49-55,143-159,192-195. */
int cotr_encode(cotr_handle h, const float* img, int B, cotr_stream stream);

/* Backbone only: features [B,16,32,1024] (NHWC over the side-by-side pair = 512 token rows of 1024 channels per pair,
 * token h*32+w like flatten(2) of the reference's [B,1024,16,32]).  Replaces self.backbone(samples)[0][-1].tensors
 * (COTR/models/backbone.py:79-92) for callers that run the rest themselves: the training step with a frozen backbone
 * (train_cotr.py:54-55 with --lr_backbone=0, the reference's stage 1). */
int cotr_backbone(cotr_handle h, const float* img, int B, float* features, cotr_stream stream);
/* Same, stopping after `stage` = 1, 2 or 3 (layer1 [B,64,128,256], layer2 [B,32,64,512], layer3 [B,16,32,1024], NHWC over
 * the pair): the part of the backbone that stays frozen when the reference trains layer2/layer3 (--lr_backbone > 0 trains
 * only parameters whose name contains layer2/3/4, COTR/models/backbone.py:66-69; stages 2-3 of readme.md:50-52). */
int cotr_backbone_upto(cotr_handle h, const float* img, int B, int stage, float* features, cotr_stream stream);

/* Query-dependent half against the cached encode: lin_sine query encoding, 6 cross-attention
 * decoder layers, decoder.norm and the corr_embed MLP on the LAST layer only (the reference runs
 * them on all 6 and keeps [-1]: transformer.py:107-117, cotr_model.py:38-39).
 * queries, out: [B,Q,2]; may be called repeatedly per encode (cycle pass of
 * inference_helper.py:197-198, query chunks of :131-136).  Q == 0 is a no-op. */
int cotr_decode(cotr_handle h, const float* queries, int B, int Q, float* out, cotr_stream stream);

/* cotr_encode + cotr_decode: the drop-in for COTR.forward (cotr_model.py:26-40). */
int cotr_forward(cotr_handle h, const float* img, const float* queries, int B, int Q, float* out,
                 cotr_stream stream);

/* Bytes of device memory behind a call of that size (packed weights + encode cache + scratch). */
int cotr_workspace_bytes(cotr_handle h, int B, int Q, size_t* bytes);

/* Scratch from the CALLER's allocator ("torch allocates, passes in").  By default the encode cache and the two
 * scratch arenas are grow-only hipMalloc'ed memory owned by the handle; growing one (a larger batch arrives) costs a
 * hipFree + hipMalloc, i.e. a device synchronisation in the middle of the caller's stream.  With a workspace the handle
 * carves the three regions from [ws, ws + bytes) instead (256-byte aligned `ws`, device memory, e.g. a torch uint8 tensor
 * from the caching allocator) and never allocates or frees.  cotr_scratch_bytes(B, Q) is the size a call of that shape needs;
 * a call that does not fit returns COTR_ERR_ARG.  keep_encode != 0: a cached encode is carried over into the new workspace
 * (device copy on `stream`, so the old workspace must outlive the work enqueued so far; meant for a decode with more queries
 * than the workspace was sized for - same number of pairs); otherwise, and with ws == NULL (back to handle-owned memory), it
 * is dropped.  The packed weights (74 MB) and the 0.5 MB position table stay handle-owned. */
int cotr_scratch_bytes(cotr_handle h, int B, int Q, size_t* bytes);
int cotr_set_workspace(cotr_handle h, void* ws, size_t bytes, int keep_encode, cotr_stream stream);

/* How a (B, Q) call is cut into passes under the handle's knobs (knob batch_split): which = 0 the encode passes, 1 the decode passes;
 * sizes[0 .. min(return, cap)) = pairs per pass; returns the number of passes or < 0.  Pairs are independent, so a call computes each
 * pass exactly as a call on those pairs alone would (tests/test_parity_gpu.py). */
int cotr_batch_chunks(cotr_handle h, int B, int Q, int which, int* sizes, int cap);

/* ---- varlen: a different number of queries per pair in one call ------------------------------
 * B >= 1 pairs; pair b owns rows offsets[b] .. offsets[b+1] of the packed queries [N][2] and of out [N][2], N = offsets[B].
 * `offsets` is a HOST array of B + 1 ints: offsets[0] = 0, nondecreasing (a pair may have no rows).  It is read before the call
 * returns and may be freed or changed right after; calls with different offsets may be enqueued back to back on one stream.
 * The result of every row is that of a uniform call on its pair (no arithmetic couples two rows).  cotr_decode_varlen decodes
 * against the cached encode of exactly B pairs (COTR_ERR_STATE otherwise); cotr_forward_varlen is cotr_encode + cotr_decode_varlen.
 * Malformed offsets, B <= 0, or null queries / out with N > 0: COTR_ERR_ARG, with a message in cotr_last_error.
 * cotr_scratch_bytes_varlen: what cotr_set_workspace must be given for such a call (it never allocates device memory then).
 * The tile tables of a call are staged in pinned host memory of the handle (allocated at first use, grow-only) and wait on a
 * HIP event of the call 4 varlen calls back: a varlen call can NOT be captured in a HIP graph.  Knob side_stream is not used. */
int cotr_decode_varlen(cotr_handle h, const float* queries, const int* offsets, int B, float* out, cotr_stream stream);
int cotr_forward_varlen(cotr_handle h, const float* img, const float* queries, const int* offsets, int B, float* out,
                        cotr_stream stream);
int cotr_scratch_bytes_varlen(cotr_handle h, const int* offsets, int B, size_t* bytes);

/* ---- pairs: B pairs drawn from M distinct images, each image's backbone run once ----------------
 * images: device [M,3,256,256] fp32 NCHW, normalised as the reference does (one half of a side-by-side input).
 * pairs:  HOST int32 [B][2], (left image, right image) of pair b; read before the call returns; repeats, self-pairs (a, a) and
 *         unused images are allowed.
 * Each image's backbone and input_proj run once; each pair's encoder input is then assembled from its two images and the encoder
 * and decoder K/V run per pair.  Afterwards the encode cache holds B pairs: cotr_decode / cotr_decode_varlen follow as after
 * cotr_encode.  cotr_forward_pairs is cotr_encode_pairs + cotr_decode (queries, out [B,Q,2]).  Pair b's result is that of
 * cotr_forward on the side-by-side input [images[pairs[b][0]] | images[pairs[b][1]]].  An index outside [0, M), M <= 0, B <= 0
 * or a null pointer: COTR_ERR_ARG with a message in cotr_last_error, nothing enqueued.  cotr_scratch_bytes_pairs: what
 * cotr_set_workspace must be given for such a call.  The indices travel in kernel arguments: a pairs call has no host wait and
 * can be captured in a HIP graph.  Knob side_stream is not used. */
int cotr_encode_pairs(cotr_handle h, const float* images, int M, const int* pairs, int B, cotr_stream stream);
int cotr_forward_pairs(cotr_handle h, const float* images, int M, const int* pairs, const float* queries, int B, int Q, float* out,
                       cotr_stream stream);
int cotr_scratch_bytes_pairs(cotr_handle h, int M, int B, int Q, size_t* bytes);

/* ---- test / profiling hooks (not needed by a binding) ------------------------------------ */

/* Keep copies of scratch intermediates for cotr_debug_tap (off by default: costs D2D copies). */
int cotr_set_debug_taps(cotr_handle h, int enable);

/* Copy an intermediate of the LAST cotr_encode / cotr_decode to dst (device or host pointer).
 * always available: "memory" ([B*512,256]), "kv" ([B*512, L*512]), "pos" ([512,256]);
 * with debug taps on: "stem" "pool" "layer1" "layer2" "layer3" (NHWC side-by-side [B,H,2W,C] of the
 * last encode chunk), "src" ([B*512,256]), "query_pos" "hs" ([rows,256] of the last decode chunk).
 * Synchronises the stream. */
int cotr_debug_tap(cotr_handle h, const char* name, float* dst, size_t max_elems, size_t* n_elems,
                   cotr_stream stream);

/* HIP-event timings (ms) of the last cotr_encode + cotr_decode: enable = 1 per stage, 2 per kernel launch
 * (names carry the GEMM shape and launch configuration), 0 off. */
int cotr_set_profiling(cotr_handle h, int enable);
int cotr_get_profile(cotr_handle h, const char** names, float* ms, int max_entries, int* n_entries);

/* Single-kernel entry points used by tests/test_ops_gpu.py for op-level parity.
 * All pointers are device pointers. */
/* y[M,N] = epilogue(x[M,K] (+ x2[M % x2_row_mod, K]) . w[N,K]^T) ; any of scale/bias/residual may be NULL */
int cotr_op_linear(const float* x, const float* x2, int x2_row_mod, const float* w, const float* scale,
                   const float* bias, const float* residual, int relu, float* y, int M, int N, int K,
                   cotr_stream stream);
/* NHWC side-by-side conv + FrozenBN(scale,bias) (+residual) (+ReLU):
 * x [B,Hin,2*Win,Cin], w [Cout][k][k][Cin], y [B,Hout,2*Wout,Cout] */
int cotr_op_conv(const float* x, const float* w, const float* scale, const float* bias,
                 const float* residual, int relu, float* y, int B, int Hin, int Win, int Cin, int Cout,
                 int ksize, int stride, cotr_stream stream);
/* stem: img NCHW [B,3,256,512] -> y [B,128,256,64]; w [64][160] (k = c*49+ky*7+kx, zero padded) */
int cotr_op_stem(const float* img, const float* w, const float* scale, const float* bias, float* y, int B,
                 cotr_stream stream);
int cotr_op_maxpool(const float* x, float* y, int B, int Hin, int Win, int C, cotr_stream stream);
/* conv1 + FrozenBN + ReLU + maxpool fused (stem_pool.hip): img [B,3,256,512] NCHW, w [64][160] -> y [B,64,128,64] NHWC sbs */
int cotr_op_stem_pool(const float* img, const float* w, const float* scale, const float* bias, float* y, int B,
                      cotr_stream stream);
/* q [nb*nq, ldq] (pre-scaled), k/v [nb*512, ldkv]; 8 heads x 32; o [nb*nq, ldo] */
int cotr_op_attention(const float* q, int ldq, const float* k, const float* v, int ldkv, float* o, int ldo,
                      int nb, int nq, cotr_stream stream);
/* the same kernel with the q projection as prologue (wq != NULL: q = ((x + x2) . wq_h^T + bq_h) * qscale per head, `q`
 * unused; x or x2 may be NULL) and / or the output projection as epilogue (wo != NULL: per-head partial outputs
 * part[8][nb*nq][256], part[h] = O_h . wo[:, 32h:32h+32]^T; `o` may then be NULL) */
int cotr_op_attention_fused(const float* q, int ldq, const float* x, const float* x2, const float* wq, const float* bq,
                            float qscale, const float* k, const float* v, int ldkv, float* o, int ldo, const float* wo,
                            float* part, int nb, int nq, cotr_stream stream);
/* y = LayerNorm(sum_c parts[c] + bias + residual) over rows of 256; parts [np][rows][256]; residual may be NULL */
/* (always ln_reduce_kernel, pointwise.hip: the reference of the next two) */
int cotr_op_ln_reduce(const float* parts, int np, const float* bias, const float* residual, const float* w, const float* b,
                      float* y, int rows, cotr_stream stream);
/* the same as the forward path launches it: np 8 / 16 by ln_reduce1.hip (no serialised round trips; the same bits), any other np by
 * ln_reduce_kernel */
int cotr_op_ln_reduce1(const float* parts, int np, const float* bias, const float* residual, const float* w, const float* b,
                       float* y, int rows, cotr_stream stream);
/* ... followed by a second LayerNorm (post_w, post_b; both NULL = none), as the last decoder layer's launch applies decoder.norm:
 * form 0 = ln_reduce_kernel, form 1 = the forward path's choice */
int cotr_op_ln_reduce_post(const float* parts, int np, const float* bias, const float* residual, const float* w, const float* b,
                           const float* post_w, const float* post_b, float* y, int rows, int form, cotr_stream stream);
int cotr_op_layernorm(const float* x, const float* w, const float* b, float* y, int rows, cotr_stream stream);
/* fused FFN block y = LN(x + W2 relu(W1 x + b1) + b2) in two launches (ffn.hip + ln_reduce); scratch holds
 * cotr_op_ffn_chunks(M) * M * 256 floats */
int cotr_op_ffn_block(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_w,
                      const float* ln_b, float* scratch, float* y, int M, cotr_stream stream);
int cotr_op_ffn_chunks(int M);
/* the attention sub-layer in ONE launch for many rows (att_rows.hip: transformer.py:149-155 encoder, :192-198 decoder):
 * y = LayerNorm(residual + out_proj(MHA(q, k, v)) + bo), 8 heads of 32, 512 keys per pair; q [nb*nq][ldq] given pre-scaled by
 * 32^-0.5 (wq == NULL), or projected here: q = ((x + x2) . wq^T + bq) * qscale (x may be NULL: decoder layer 0).  residual may be
 * NULL; y must not alias residual / x / x2 / q */
int cotr_op_att_rows(const float* q, int ldq, const float* x, const float* x2, const float* wq, const float* bq, float qscale,
                     const float* k, const float* v, int ldkv, const float* wo, const float* bo, const float* residual,
                     const float* ln_w, const float* ln_b, float* y, int nb, int nq, cotr_stream stream);
/* the same block in ONE launch for many rows (ffn_rows.hip: transformer.py:156-158 / 199-201 [+ :110-111 with post_w / post_b, a
 * second LayerNorm of the result]); y must not alias x */
int cotr_op_ffn_rows(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_w,
                     const float* ln_b, const float* post_w, const float* post_b, float* y, int M, cotr_stream stream);
/* the same for a layer2 bottleneck (conv23m.hip): t1 [B,32 S,64 S,128] NHWC side-by-side (S = stride of the 3x3: 1 or 2), w2 [128][3][3][128],
 * w3 [512][128], residual / y [B,32,64,512] */
int cotr_op_conv23m(const float* t1, const float* w2, const float* s2, const float* b2, const float* w3, const float* s3, const float* b3,
                    const float* residual, float* y, int B, int stride, cotr_stream stream);
/* one or two 1x1 convolutions with K = 64 over the same x in ONE launch for many rows (expand.hip; layer1 block 0's downsample branch
 * and conv1 of torchvision's Bottleneck with COTR/models/backbone.py:46-56): y_s = [relu](FrozenBN_s(x . w_s^T)); x [M][64], M a multiple
 * of 128; w_s [n_s][64], y_s [M][n_s], n_s multiples of 64; n1 == 0: one set.  Shapes it is not written for are declined (-1) */
int cotr_op_expand(const float* x, int M, const float* w0, const float* s0, const float* b0, int relu0, float* y0, int n0, const float* w1,
                   const float* s1, const float* b1, int relu1, float* y1, int n1, cotr_stream stream);
/* conv2 (3x3, padding 1 per half) + FrozenBN + ReLU -> conv3 (1x1) + FrozenBN + identity + ReLU of a layer1 bottleneck in ONE launch
 * (conv23.hip; torchvision Bottleneck.forward with COTR/models/backbone.py:46-56): t1 [B,64,128,64] NHWC side-by-side, w2 [64][3][3][64],
 * w3 [256][64], residual / y [B,64,128,256] */
int cotr_op_conv23(const float* t1, const float* w2, const float* s2, const float* b2, const float* w3, const float* s3, const float* b3,
                   const float* residual, float* y, int B, cotr_stream stream);
/* lin_sine encoding of pts [n,2] -> y [n,256] (COTR/models/position_encoding.py:41-45) */
int cotr_op_posenc(const float* pts, float* y, int n, cotr_stream stream);


/* ---- training step ----------------------------------------------------------
 * The kernels the autograd tape of cotr_amd/training.py runs besides the GEMMs above; they replace, op for op, what
 * COTRTrainer.train_batch (COTR/trainers/cotr_trainer.py:118-150) has torch/cuDNN compute in COTR/models/transformer.py
 * with dropout active.  All device pointers, fp32, rows of 256 channels unless stated.  Dropout is counter-based
 * (keep = hash(seed, element index) >= p * 2^32): backward kernels recompute the mask from (seed, index), nothing is stored;
 * p == 0 makes every kernel exact (what the gradient goldens pin).  Reductions across workgroups go through `part` scratch and
 * are summed in a fixed order (no atomics: a step is bit-repeatable).  cotr_train_*_parts / _splits give the scratch sizes.
 * Alignment: a pointer the kernels access as float4 must be 16-byte aligned (with rows of 256 floats, or a row stride that is a
 * multiple of 4, every row then is); a pointer they access by scalar needs the 4-byte alignment of a float.  The "alignment of"
 * line under each prototype says which is which; tests/test_train_guard_gpu.py places every buffer at exactly that and no better.
 * No entry point checks it: a misaligned float4 pointer is undefined behaviour, not COTR_ERR_ARG. */
/* y[m] = x[m] + x2[m % mod] (mod == 0: row m): src + pos (transformer.py:147), tgt + query_pos (:192) */
int cotr_train_add_rowmod(const float* x, const float* x2, int mod, float* y, int rows, cotr_stream stream);
/* alignment of cotr_train_add_rowmod: x, x2, y 16-byte aligned */
/* y = LayerNorm(s), s = x + dropout(a) (x may be NULL); s_out (may be NULL) and stats [rows][2] = (mean, rstd) for the backward:
 * transformer.py:154-155,157-158 (encoder), :196-198,200-201 (decoder), :110-111 (decoder.norm with x NULL, p 0) */
int cotr_train_add_drop_ln_fwd(const float* x, const float* a, const float* w, const float* b, float* s_out, float* y, float* stats,
                               int rows, float p, uint32_t seed, cotr_stream stream);
/* alignment of cotr_train_add_drop_ln_fwd: x, a, w, b, s_out, y 16-byte aligned; stats 4-byte aligned */
int cotr_train_ln_bwd_parts(int rows);   /* like cotr_train_colsum_parts and cotr_train_head_bwd_parts: 0 for rows <= 0 */
/* ds = d loss / d s (= dx), da = ds * mask / (1-p) (may be NULL), dwb [512] = dgamma | dbeta; part: parts * 512 floats */
int cotr_train_ln_bwd(const float* dy, const float* s_in, const float* stats, const float* w, float* ds, float* da, float* part,
                      float* dwb, int rows, float p, uint32_t seed, cotr_stream stream);
/* alignment of cotr_train_ln_bwd: dy, s_in, w, ds, da 16-byte aligned; stats, part, dwb 4-byte aligned */
/* Captured (hipGraph) training steps: the seed argument of a dropout launch is baked into the graph, so every training kernel that
 * draws a mask XORs its seed with the word at `salt` (device memory, read at kernel start); the captured step advances that word
 * itself (any device-side add), so each replay draws fresh masks and forward / backward of one step agree.  NULL (default) = the
 * seeds alone.  The registration is per DEVICE (the current one) and process-wide: the autograd engine runs the backward kernels
 * that recompute a mask on its own worker thread, and they must see the salt the forward drew the mask with.
 * cotr_train_clear_dropout_salt unregisters `salt` only if it is still the registered word (COTR_ERR_STATE otherwise). */
int cotr_train_set_dropout_salt(const unsigned int* salt);
int cotr_train_clear_dropout_salt(const unsigned int* salt);
/* in place x *= mask / (1-p) (n % 4 == 0); backward of y = dropout(relu(h)): dx = y > 0 ? dy / (1-p) : 0 (p == 0: relu backward) */
int cotr_train_dropout_fwd(float* x, size_t n, float p, uint32_t seed, cotr_stream stream);
/* alignment of cotr_train_dropout_fwd: x 16-byte aligned */
int cotr_train_relu_drop_bwd(const float* dy, const float* y, float* dx, size_t n, float p, cotr_stream stream);
/* alignment of cotr_train_relu_drop_bwd: dy, y, dx 16-byte aligned */
/* out[N] = column sums of x [M][N] (bias gradients); part: parts(M) * N floats */
int cotr_train_colsum_parts(int M);
int cotr_train_colsum(const float* x, float* part, float* out, int M, int N, cotr_stream stream);
/* alignment of cotr_train_colsum: x, part 16-byte aligned (N % 4 == 0 keeps every row so); out 4-byte aligned */
/* dst [C][R] = src [R][C]^T (W^T once per optimiser step, for dX = dY . W on the GEMM kernels) */
int cotr_train_transpose(const float* src, float* dst, int R, int C, cotr_stream stream);
/* alignment of cotr_train_transpose: src, dst 4-byte aligned */
/* Convolution backward of the trainable backbone stages (layer2 / layer3, backbone.py:66-69) by explicit im2col over the NHWC
 * side-by-side activations [B][Hin][2*Win][Cin] (each half padded on its own, like the forward kernels):
 *   col [B*Hout*2*Wout][k*k*Cin] = im2col(x);  wgrad dW [Cout][k*k*Cin] = dz^T . col (cotr_train_gemm_tn);
 *   dgrad dcol = dz . W (GEMM), dx = col2im(dcol) (gather over the taps in a fixed order).
 * cotr_train_scale_rows: out[r][:] = w[r][:] * scale[r] (FrozenBN folded into the weights / unfolded from their gradient);
 * cotr_train_transpose_batched: per batch element dst[C][R] = src[R][C]^T (torch's [Cout][Cin][k*k] <-> packed [Cout][k*k][Cin]) */
int cotr_train_im2col(const float* x, float* col, int B, int Hin, int Win, int Cin, int ksize, int stride, cotr_stream stream);
/* alignment of cotr_train_im2col: x, col 16-byte aligned (Cin % 4 == 0) */
int cotr_train_col2im(const float* dcol, float* dx, int B, int Hin, int Win, int Cin, int ksize, int stride, cotr_stream stream);
/* alignment of cotr_train_col2im: dcol, dx 16-byte aligned (Cin % 4 == 0) */
int cotr_train_scale_rows(const float* w, const float* scale, float* out, int rows, int cols, cotr_stream stream);
/* alignment of cotr_train_scale_rows: w, out 16-byte aligned (cols % 4 == 0); scale 4-byte aligned */
int cotr_train_transpose_batched(const float* src, float* dst, int batch, int R, int C, cotr_stream stream);
/* alignment of cotr_train_transpose_batched: src, dst 4-byte aligned */
/* out [N][K] = A [M][N]^T . B [M][K] (dW = dY^T . X, both row-major, no transposed copies); N, K multiples of 64.
 * colsum != NULL: also colsum [N] = column sums of A (db) from the same pass over dY; it must be out + N*K (one buffer
 * [N*K + N]) so that one launch finishes both.  part: splits(M, N, K) * (N * K + N) floats */
int cotr_train_gemm_tn_splits(int M, int N, int K);
int cotr_train_gemm_tn(const float* A, const float* B, float* part, float* out, float* colsum, int M, int N, int K,
                       cotr_stream stream);
/* alignment of cotr_train_gemm_tn: A, B 16-byte aligned; part, out, colsum 4-byte aligned */
/* The partials of cotr_train_gemm_tn alone (part [splits][N*K (+ N with with_colsum)]): -> number of partials written (0 for
 * M == 0), < 0 = error.  The count can be SMALLER than cotr_train_gemm_tn_splits(M, N, K) - the rows of a split are rounded up to a
 * multiple of 32 (M = 4100, N = K = 256: 26 of 32) - and the partials past it are not written: sum only the count returned.  cotr_train_ln_bwd / cotr_train_head_bwd with dwb == NULL likewise leave their partials unsummed.
 * cotr_train_reduce_jobs finishes ALL partials of a backward pass in one launch and accumulates them into the gradient buffers
 * (cotr_amd/train_ops.py: GradSink - replaces one reduction launch per weight plus autograd's add_ into .grad):
 *   for each job, each source in order:  dst[perm(e)] += scale[e / row_len] * sum_{p < nparts, in order} part[p * pstride + e]
 * jobs / srcs / chunk_job live in DEVICE memory; one workgroup per 1024-element chunk: chunk0 = a job's first chunk
 * ((numel + 1023) / 1024 chunks per job), nchunks = their total, chunk_job[c] = index of the job chunk c belongs to; taps > 1: element e = (row, tap, c) of a packed [row][taps][cin] record goes to (row, c, tap) (conv weight
 * gradients back to torch's [Cout][Cin][k][k]); vec = 1 promises 16-byte aligned pointers and counts that are multiples of 4. */
typedef struct cotr_reduce_src {
  const float* part;
  unsigned long long pstride;
  unsigned nparts, pad_;
} cotr_reduce_src;
typedef struct cotr_reduce_job {
  float* dst;
  const float* scale;
  unsigned numel, first_src, n_src, chunk0;
  unsigned row_len, cin, taps, vec;
} cotr_reduce_job;
int cotr_train_gemm_tn_parts(const float* A, const float* B, float* part, int M, int N, int K, int with_colsum, cotr_stream stream);
/* alignment of cotr_train_gemm_tn_parts: A, B 16-byte aligned; part 4-byte aligned */
/* The same partials for the weight gradient of a convolution WITHOUT its im2col image (round 6): A = dz [B*Hout*2*Wout][Cout], the
 * second operand is gathered from x [B][Hin][2*Win][Cin] by the kernel (zeros where a tap leaves the half) - the bits of
 * cotr_train_im2col + cotr_train_gemm_tn_parts(dz, col, ..., 0).  part as for cotr_train_gemm_tn_parts with M = B*Hout*2*Wout,
 * N = Cout, K = ksize*ksize*Cin.  Returns the number of partials, or -1 where this form does not apply (Cin % 128 != 0, small
 * shapes): form the image and call cotr_train_gemm_tn_parts. */
int cotr_train_conv_wgrad_parts(const float* dz, const float* x, float* part, int B, int Hin, int Win, int Cin, int Cout, int ksize,
                                int stride, cotr_stream stream);
/* alignment of cotr_train_conv_wgrad_parts: dz, x 16-byte aligned; part 4-byte aligned */
/* out[i] = part[0][i] + part[1][i] + ... in split order (i < n; part [nparts][n]): what cotr_train_gemm_tn does after its partials */
int cotr_train_sum_parts(const float* part, int nparts, size_t n, float* out, cotr_stream stream);
/* alignment of cotr_train_sum_parts: part, out 4-byte aligned */
int cotr_train_reduce_jobs(const cotr_reduce_job* jobs, const cotr_reduce_src* srcs, const unsigned* chunk_job, int njobs, int nchunks,
                           cotr_stream stream);
/* alignment of cotr_train_reduce_jobs: jobs, srcs 8-byte aligned (they hold pointers), chunk_job 4-byte aligned; inside a job with vec = 1
 * dst and every part 16-byte aligned and numel, pstride, row_len, cin multiples of 4, with vec = 0 4-byte aligned; scale 4-byte aligned */
/* torch.optim.Adam's update (train_cotr.py:49-57: betas (0.9, 0.999), eps 1e-8, no weight decay / amsgrad) over EVERY trainable
 * parameter in one launch, on flat gradient / exp_avg / exp_avg_sq buffers of one layout (cotr_amd/training.py: FusedAdam on the
 * GradSink's buffer):  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;  p -= lr[group] / bc1 * m / (sqrt(v) / bc2_sqrt + eps).
 * jobs / chunk_job (device memory): one job per parameter, one workgroup per 1024 elements, as for cotr_train_reduce_jobs; lr = HOST
 * array of ngroups <= 8 rates.  step == NULL: bias_correction1 = 1 - b1^t and bias_correction2_sqrt = sqrt(1 - b2^t) as given
 * (torch computes them on the host in double precision); step != NULL: *step (device, float) = t, corrections computed in the kernel
 * (captured steps). */
typedef struct cotr_adam_job {
  float* p;
  unsigned long long off;
  unsigned numel, chunk0, group, vec;
} cotr_adam_job;
int cotr_train_adam(const cotr_adam_job* jobs, const unsigned* chunk_job, int nchunks, const float* g, float* m, float* v, const float* lr,
                    int ngroups, double beta1, double beta2, double eps, double bias_correction1, double bias_correction2_sqrt,
                    const float* step, cotr_stream stream);
/* alignment of cotr_train_adam: jobs 8-byte aligned, chunk_job and step 4-byte aligned, lr a host array; a job with vec = 1 needs p, g + off,
 * m + off, v + off 16-byte aligned (g, m, v 16-byte aligned and off a multiple of 4), with vec = 0 everything 4-byte aligned */
/* Every weight-shaped operand of a training step re-derived from the parameters in ONE launch (after the optimiser step): the W^T
 * slices of the dX GEMMs, the packed [Cout][k][k][Cin] convolution weights, the FrozenBN-scaled transposed convolution weights (one
 * fp32 multiply per element, as cotr_train_scale_rows makes).  A job is a batched strided transpose of 32 x 32 tiles:
 * dst[z*dz + c*dc + r] = src[z*sz + r*sr + c*sc] * (scale ? scale[r] : 1); tile_job[workgroup] = its job (device memory, like
 * cotr_train_reduce_jobs); tile0 = the job's first workgroup, tiles_r / tiles_c = ceil(R / 32) / ceil(C / 32). */
typedef struct cotr_perm_job {
  const float* src;
  float* dst;
  const float* scale;
  unsigned Z, R, C;
  unsigned sz, sr, sc, dz, dc;
  unsigned tile0, tiles_r, tiles_c, pad;
} cotr_perm_job;
int cotr_train_perm_jobs(const cotr_perm_job* jobs, const unsigned* tile_job, int njobs, int ntiles, cotr_stream stream);
/* alignment of cotr_train_perm_jobs: jobs 8-byte aligned, tile_job 4-byte aligned; src, dst, scale inside a job 4-byte aligned */
/* last corr_embed layer 256 -> 2 (position_encoding.py:23-26): y [nb][nq][2]; backward: dh [rows][256], dwb [514] = dW2 | db2 */
int cotr_train_head_fwd(const float* x, const float* w, const float* b, float* y, int nb, int nq, cotr_stream stream);
/* alignment of cotr_train_head_fwd: x, w 16-byte aligned; b, y 4-byte aligned */
int cotr_train_head_bwd_parts(int rows);
int cotr_train_head_bwd(const float* dy, const float* h, const float* w2, float* dh, float* part, float* dwb, int rows,
                        cotr_stream stream);
/* alignment of cotr_train_head_bwd: h, w2, dh 16-byte aligned; dy, part, dwb 4-byte aligned */
/* o = dropout(softmax(q k^T * qscale)) v per head (8 x 32; q [nb*nq][ldq], k [nb*512][ldk], v [nb*512][ldv]); lse [nb*nq][8]
 * (log2-domain log-sum-exp) for the backward */
int cotr_train_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, float* lse,
                             int nb, int nq, float qscale, float p, uint32_t seed, cotr_stream stream);
/* alignment of cotr_train_attention_fwd: q, k, v, o 16-byte aligned and every ld a multiple of 4; lse 4-byte aligned */
/* dq [nb*nq][lddq], dk [nb*512][lddk], dv [nb*512][lddv]; delta: nb*nq*8 floats of scratch; o / d_o share ldo.
 * scratch: cotr_train_attention_bwd_scratch(nb, nq) floats or NULL - room for the dQ partials of the one-pass backward when the keys
 * of a head are split over several workgroups (few pairs); without it that shape takes the two-kernel form */
int cotr_train_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                             const float* d_o, int ldo, const float* lse, float* delta, float* dq, int lddq, float* dk, int lddk,
                             float* dv, int lddv, int nb, int nq, float qscale, float p, uint32_t seed, float* scratch,
                             cotr_stream stream);
/* alignment of cotr_train_attention_bwd: q, k, v, o, d_o, dq, dk, dv, scratch 16-byte aligned and every ld a multiple of 4; lse, delta
 * 4-byte aligned */
size_t cotr_train_attention_bwd_scratch(int nb, int nq);

/* ---- engine-side input construction (one launch per zoom level) -------------
 * For each of n tasks: crop the square box (xa, ya, size_a) of image A and (xb, yb, size_b) of image B
 * (uint8 HWC RGB, DEVICE pointers; boxes int32 [n][6] on the device, inside the images), resize both to
 * 256x256 with Pillow's 8-bit BILINEAR resample (bit-exact), place them side by side, convert to float/255
 * and ImageNet-normalise: out float32 [n,3,256,512], directly consumable by cotr_encode.
 * Replaces per task: PIL resize x2 + two_images_side_by_side + to_tensor + normalize
 * (COTR/inference/refinement_task.py:105-120) and the H2D copy of sparse_engine.py:50.
 * max_size: the largest crop edge among the boxes, or any upper bound of it (the result does not depend on which); it sizes
 * the workgroup's LDS row window, whose 160 KB hold crops up to COTR_CROP_MAX_SIZE.  2 <= max_size <= COTR_CROP_MAX_SIZE,
 * otherwise COTR_ERR_ARG with nothing launched and `out` untouched; n == 0 returns COTR_OK and does nothing. */
#define COTR_CROP_MAX_SIZE 7936
int cotr_crop_resize_pairs(const uint8_t* img_a, int ha, int wa, const uint8_t* img_b, int hb, int wb,
                           const int32_t* boxes, int n, float* out, int max_size, cotr_stream stream);

/* ---- dense initial pass: post-processing on the device ---------------------------------------
 * Replaces the host round trip of COTR/inference/inference_helper.py:137-160 (cotr_patch_flow_exhaustive.one_pass
 * tail) and :61-75 (merge_flow_patches) + COTR/utils/utils.py:69-83 (float_image_resize).
 *
 * cotr_dense_cycle: pred [n_pairs,256,512,2] = the network's answer for the query grid (j/512, i/256) ->
 *   maps [n_pairs,256,512,3] = (x, y, cycle error): self-composition through bilinear grid_sample (zeros padding,
 *   align_corners=False), x re-centred per half (:140-142), then the 2x3 affine of that half applied in double
 *   (:157-158).  affine [n_pairs][2][6] doubles (device): [p][0] left half -> image b, [p][1] right half -> image a.
 * cotr_dense_merge: for one image (side 0 = a / left halves, 1 = b / right halves) resize each entry's 256x256x3
 *   half to its patch boxes[p] = (x, y, size) with Pillow's mode-'F' BILINEAR (bit-exact) and keep per pixel the
 *   entry with the lowest cycle error, later entries winning ties -> flow [H,W,2], conf [H,W] (100 where uncovered). */
int cotr_dense_cycle(const float* pred, int n_pairs, const double* affine, float* maps, cotr_stream stream);
int cotr_dense_merge(const float* maps, const int32_t* boxes, int n_pairs, int side, int H, int W, float* flow,
                     float* conf, cotr_stream stream);

/* src [Hs,Ws,C] float -> dst [Hd,Wd,C] with Pillow's mode-'F' BILINEAR resample, channel by channel, bit-exact:
 * utils.float_image_resize (COTR/utils/utils.py:69-83), used by SparseEngine's 'stretching' mode to bring the dense maps
 * of the squared images back to the image shape (sparse_engine.py:124-129). */
int cotr_resize_f32(const float* src, int Hs, int Ws, int C, float* dst, int Hd, int Wd, cotr_stream stream);

/* ---- triangulate_corr: rasterise a triangle mesh into a dense map (cotr_amd/csrc/triangulate.hip) --------------------
 * Replaces the vispy/OpenGL render of COTR/inference/inference_helper.py:293-308 (the Delaunay triangles of the
 * correspondences drawn into an H x W float framebuffer, B's normalised coordinates as vertex colours).
 *
 * cotr_raster_mesh: verts [n_verts,2] normalised A points (u, v), attrs [n_verts,2] float values, tris [n_tris,3] int32
 *   vertex indices, all DEVICE pointers -> out [H,W,2] (DEVICE, 8-byte aligned) = at the centre (j + 0.5, i + 0.5) px of
 *   pixel (i, j) the barycentric interpolation of attrs over the covering triangle, 0 where no triangle covers it;
 *   mask [H,W] (DEVICE, may be NULL) = 1 where covered.  Vertices are snapped to 1/256 px (X = rint(u*W*256),
 *   Y = rint(v*H*256)); coverage uses exact int64 edge functions with a tie rule that covers every sample of a proper
 *   triangulation exactly once; where triangles overlap the highest index wins (bit-identical from run to run).
 *   A triangle with an index outside [0, n_verts), a non-finite vertex, a snapped coordinate of magnitude >= 2^30
 *   (2^22 px) or zero snapped area is skipped.  1 <= H, W <= 16384; n_tris == 0 writes zeros.
 *   scratch: DEVICE, 16-byte aligned, at least cotr_raster_mesh_scratch_bytes(n_tris, H, W) bytes.  Stream-ordered,
 *   no host waits, capturable.
 * Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error() (these
 * calls have no handle; the message is per thread). */
int cotr_raster_mesh_scratch_bytes(int n_tris, int H, int W, size_t* bytes);
int cotr_raster_mesh(const float* verts, int n_verts, const float* attrs, const int32_t* tris, int n_tris, int H, int W,
                     float* out, uint8_t* mask, void* scratch, size_t scratch_bytes, cotr_stream stream);
const char* cotr_raster_last_error(void);

/* ---- delaunay: the triangles cotr_raster_mesh draws, made on the device (cotr_amd/csrc/delaunay.hip) -------------------
 * Replaces scipy.spatial.Delaunay(corr[:, :2]) of inference_helper.py:239,293-308 by an exact rule that is unique for
 * every input: points snapped to 2^-24, orientation in int64, the in-circle test in 128-bit integers,
 * cocircular points decided as if point i were lifted by an infinitesimal amount that is larger for a lower i.
 *
 * cotr_delaunay: verts [n,2] float32 normalised points (u, v), DEVICE -> tris [cotr_delaunay_max_tris(n), 3] int32 (DEVICE):
 *   the triangles, each counter-clockwise with its lowest index first, ordered by that index and then in the order of its
 *   walk; rows past the count are -1 (cotr_raster_mesh skips them: the whole capacity can be passed on, no count read
 *   back).  info: DEVICE int32[2] = {count, status}; status 0 = ok, 1 = a walk reached its bound of n steps (never seen).
 *   A point that is not finite, has |u| or |v| > 4, or snaps onto a valid point of lower index is in no triangle.
 *   0 <= n <= 65536.  The cost is quadratic in n.  scratch: DEVICE, 16-byte aligned, at least
 *   cotr_delaunay_scratch_bytes(n) bytes.  Stream-ordered, no host waits, no allocation, capturable; bit-identical from
 *   run to run.
 * cotr_delaunay_max_tris: 2 n, the capacity of tris in triangles (COTR_ERR_ARG for n outside [0, 65536]).
 * Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_delaunay_max_tris(int n);
int cotr_delaunay_scratch_bytes(int n, size_t* bytes);
int cotr_delaunay(const float* verts, int n, int32_t* tris, int32_t* info, void* scratch, size_t scratch_bytes,
                  cotr_stream stream);

/* ---- guided matching: nearest / mutual keypoints and fundamental-matrix RANSAC (cotr_amd/csrc/guided.hip) --------------
 * The host post-processing of demo_guided_matching.py:48-63 (scipy distance matrices + argmin, the mutual double loop,
 * cv2.findFundamentalMat(FM_RANSAC)) on the device.  Rules in DESIGN.md 3h.
 *
 * cotr_nearest_mutual: pred_ab [na,2], kp_b [nb,2], pred_ba [nb,2], kp_a [na,2], float64 DEVICE pointers (callers widen
 *   float32 keypoints exactly) -> idx_ab [na] int32 = argmin_j d(pred_ab[i], kp_b[j]), idx_ba [nb] int32 likewise, and
 *   mutual [na] uint8 = 1 iff idx_ba[idx_ab[i]] == i.  d = sqrt(dx*dx + dy*dy) with dx = k.x - p.x, dy = k.y - p.y in
 *   float64, no contraction, correctly rounded sqrt (bit-equal to scipy.spatial.distance_matrix); the lowest j wins ties
 *   and a NaN distance counts as the minimum (numpy's argmin).  1 <= na, nb <= 2^24.
 *   scratch: DEVICE, 16-byte aligned, at least cotr_nearest_mutual_scratch_bytes(na, nb) bytes.
 * cotr_ransac_fundamental: pts1 [n,2], pts2 [n,2] float64 DEVICE pointers (rounded to float32 first) -> F_out [9]
 *   (float64, row-major, p2^T F p1 = 0), mask_out [n] uint8 inliers of F_out, info_out [4] int32 = {found, best inlier
 *   count, sequential iterations run, chosen hypothesis slot (-1: none)}; F_out = 0 and mask_out = 0 when nothing is
 *   found.  Iteration it draws 7 distinct indices from splitmix64 counters of (seed, it, draw), solves the 7-point
 *   problem (up to 3 candidates, slots 3*it + k) and the candidates are counted in parallel; the sequential FM_RANSAC
 *   loop (adaptive iteration count with confidence) is then replayed on the counts.  An inlier has
 *   float(max(e1, e2)) <= float(threshold^2), e1 / e2 the squared distances to the epipolar lines.  15 <= n <= 2^24,
 *   1 <= max_iters <= 65536, threshold > 0 finite, 0 < confidence < 1.
 *   hyp_F [3*max_iters][9] float64, hyp_count [3*max_iters] int32 (-1: no candidate in the slot; its F is NaN),
 *   hyp_samples [max_iters][7] int32 (-1 past the indices drawn): optional DEVICE outputs (NULL: not written).
 *   scratch: DEVICE, 16-byte aligned, at least cotr_ransac_fundamental_scratch_bytes(n, max_iters) bytes.
 * Both calls are stream-ordered, with no host waits and no allocation (capturable).  Bad arguments are checked before
 * any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error() (the per-thread message slot of every
 * handle-less call). */
int cotr_nearest_mutual_scratch_bytes(int na, int nb, size_t* bytes);
int cotr_nearest_mutual(const double* pred_ab, const double* kp_b, const double* pred_ba, const double* kp_a, int na, int nb,
                        int32_t* idx_ab, int32_t* idx_ba, uint8_t* mutual, void* scratch, size_t scratch_bytes, cotr_stream stream);
int cotr_ransac_fundamental_scratch_bytes(int n, int max_iters, size_t* bytes);
int cotr_ransac_fundamental(const double* pts1, const double* pts2, int n, double threshold, double confidence, int max_iters,
                            uint64_t seed, double* F_out, uint8_t* mask_out, int32_t* info_out, double* hyp_F, int32_t* hyp_count,
                            int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- homography RANSAC with a least-squares refit on the inliers (cotr_amd/csrc/homography.hip) -------------------------
 * The structure of cv2.findHomography(pts1, pts2, cv2.RANSAC, threshold) on the device, by rules of the library's own
 * (no bit-compatibility with OpenCV is claimed).  H maps pts1 to pts2: [u, v, 1]^T ~ H [x, y, 1]^T.
 *
 * cotr_ransac_homography: pts1 [n,2], pts2 [n,2] float64 DEVICE pointers (rounded to float32 first) -> H_out [9] (float64,
 *   row-major; the refit on the inliers of the chosen candidate), mask_out [n] uint8 (the inliers of the chosen candidate:
 *   the RANSAC mask, as in cv2), info_out [8] int32 = {found, best inlier count, sequential iterations run, chosen slot
 *   (-1: none), Gauss-Newton steps kept, refit status (0: DLT + refinement, 1: DLT only, 2: none), 0, 0}; H_out = 0 and
 *   mask_out = 0 when nothing is found.  Iteration it draws 4 distinct indices with the sampler of
 *   cotr_ransac_fundamental, rejects degenerate samples (three points on a line in either set, or an orientation that is
 *   not kept), solves the Hartley-normalised 8x8 system by full-pivot elimination (slot it); the candidates are counted in
 *   parallel and the sequential RANSAC loop is replayed on the counts.  An inlier has
 *   float(dx^2 + dy^2) <= float(threshold^2), (dx, dy) = H(x, y) - (u, v).  The refit: Hartley normalisation of the
 *   inliers, the eigenvector of the smallest eigenvalue of the 9x9 DLT matrix (cyclic Jacobi), then refine_iters
 *   Gauss-Newton steps on the 8 free entries, each kept only while the squared error falls.  Every floating-point sum is
 *   taken in a fixed order (no atomics): the same input gives the same bits on any stream, with any scratch contents.
 *   4 <= n <= 2^24, 1 <= max_iters <= 65536, 0 <= refine_iters <= 64, threshold > 0 finite, 0 < confidence < 1.
 *   H_ransac [9] (the chosen candidate, 0 when nothing is found), hyp_H [max_iters][9] float64, hyp_count [max_iters]
 *   int32 (-1: no candidate in the slot; its H is NaN), hyp_samples [max_iters][4] int32 (-1 past the indices drawn):
 *   optional DEVICE outputs (NULL: not written).
 *   scratch: DEVICE, 16-byte aligned, at least cotr_ransac_homography_scratch_bytes(n, max_iters) bytes.
 * Stream-ordered, 4 + 2 * (refine_iters + 4) launches (10 with refine_iters = 0) whatever the data, no host waits and no allocation (capturable).
 * Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_ransac_homography_scratch_bytes(int n, int max_iters, size_t* bytes);
int cotr_ransac_homography(const double* pts1, const double* pts2, int n, double threshold, double confidence, int max_iters,
                           int refine_iters, uint64_t seed, double* H_out, uint8_t* mask_out, int32_t* info_out, double* H_ransac,
                           double* hyp_H, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes,
                           cotr_stream stream);

/* ---- essential-matrix RANSAC and the pose of an essential matrix (cotr_amd/csrc/essential.hip) --------------------------
 * The structure of cv2.findEssentialMat(pts1, pts2, K1, dist1, K2, dist2, cv2.RANSAC, prob, threshold) and
 * cv2.recoverPose(E, pts1, pts2, K1, ..., distanceThresh) on the device, by rules of the library's own (no
 * bit-compatibility with OpenCV is claimed).  x2h^T E x1h = 0 on camera-normalised points; x2 ~ R x1 + t.
 *
 * K1, K2: HOST pointers to 9 doubles each, row-major upper-triangular camera matrices (fx, skew, cx; 0, fy, cy; 0, 0, 1;
 *   only those five entries are read), finite, fx and fy not 0.  A pixel (u, v), rounded to float32, becomes
 *   y = (v - cy) / fy, x = (u - cx - skew y) / fx.
 * cotr_ransac_essential: pts1 [n,2], pts2 [n,2] float64 DEVICE pointers (rounded to float32 first) -> E_out [9] (float64,
 *   row-major, unit Frobenius norm, the first entry of largest magnitude positive: the chosen candidate, no refit),
 *   mask_out [n] uint8 (its inliers), info_out [8] int32 = {found, best inlier count, sequential iterations run, chosen
 *   slot (-1: none), 0, 0, 0, 0}; E_out = 0 and mask_out = 0 when nothing is found.  Iteration it draws 5 distinct indices
 *   with the sampler of cotr_ransac_fundamental and solves the five-point problem (0..10 real candidates, slots
 *   10 * it + k, in ascending order of the root): a 4-dimensional null space, the ten cubic constraints in 20 monomials,
 *   Gauss-Jordan elimination of the cubic monomials, the real eigenvalues of the 10 x 10 action matrix by Hessenberg
 *   reduction and shifted QR iteration, then 3 Gauss-Newton steps on every root.  The candidates are counted in parallel
 *   and the sequential RANSAC loop is replayed on the counts.  An inlier has float(Sampson error) <= float(thr^2) with
 *   thr = threshold / ((fx1 + fy1 + fx2 + fy2) / 4).  5 <= n <= 2^24, 1 <= max_iters <= 6553, threshold > 0 finite,
 *   0 < confidence < 1.
 *   hyp_E [10*max_iters][9] float64, hyp_count [10*max_iters] int32 (-1: no candidate in the slot; its E is NaN),
 *   hyp_samples [max_iters][5] int32 (-1 past the indices drawn): optional DEVICE outputs (NULL: not written).
 *   scratch: DEVICE, 16-byte aligned, at least cotr_ransac_essential_scratch_bytes(n, max_iters) bytes.
 * cotr_recover_pose: E [9] float64 DEVICE pointer, pts1, pts2 as above, mask_in [n] uint8 DEVICE (NULL: every point),
 *   found: DEVICE pointer to an int32 (NULL: taken as 1; 0: nothing to decompose, e.g. info_out of cotr_ransac_essential)
 *   -> R_out [9], t_out [3] float64 (unit length), mask_out [n] uint8 = mask_in and in front of both cameras under the
 *   chosen candidate, info_out [8] int32 = {points in front, chosen candidate (-1: none), the four counts, 0, 0}.  The
 *   candidates, in cv2's order: (R1, t), (R2, t), (R1, -t), (R2, -t) with R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2], U and V
 *   from cyclic Jacobi on E^T E.  A point is in front when its least-squares depths in both cameras lie in
 *   (0, distance_thresh).  The first candidate with the largest count is taken.  found = 0 or a non-finite E: R_out = 0,
 *   t_out = 0, mask_out = 0, info_out = {0, -1, 0, ...}.  5 <= n <= 2^24, distance_thresh > 0 finite.
 *   scratch: DEVICE, 16-byte aligned, at least cotr_recover_pose_scratch_bytes(n) bytes.
 * Stream-ordered, 5 and 3 launches whatever the data, no host waits and no allocation (capturable); integer atomics only:
 * the same input gives the same bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in
 * cotr_raster_last_error(). */
int cotr_ransac_essential_scratch_bytes(int n, int max_iters, size_t* bytes);
int cotr_ransac_essential(const double* pts1, const double* pts2, int n, const double* K1, const double* K2, double threshold,
                          double confidence, int max_iters, uint64_t seed, double* E_out, uint8_t* mask_out, int32_t* info_out,
                          double* hyp_E, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes,
                          cotr_stream stream);
int cotr_recover_pose_scratch_bytes(int n, size_t* bytes);
int cotr_recover_pose(const double* E, const double* pts1, const double* pts2, int n, const double* K1, const double* K2,
                      double distance_thresh, const uint8_t* mask_in, const int32_t* found, double* R_out, double* t_out,
                      uint8_t* mask_out, int32_t* info_out, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- the refit of a relative pose on its inliers (cotr_amd/csrc/essential.hip; rules in DESIGN.md 3h-5) ------------------
 * Undamped Gauss-Newton on the Sampson error over (R, unit t), with the inliers re-counted between rounds: what the
 * homography and PnP estimators end with, for the pose of cotr_ransac_essential + cotr_recover_pose.
 *
 * K1, K2, pts1, pts2, mask_in, found: as for cotr_recover_pose (K1, K2 on the HOST, the rest DEVICE pointers; mask_in NULL:
 *   every point; found NULL: 1).  R_in [9], t_in [3] float64 DEVICE: the pose to start from, e.g. R_out, t_out of
 *   cotr_recover_pose.  -> R_out [9], t_out [3] (unit length), E_out [9] = [t]x R at unit Frobenius norm with the first
 *   entry of largest magnitude positive, mask_out [n] uint8 (the mask the last round fitted on; must not overlap mask_in),
 *   info_out [8] int32 = {found, points in mask_out, rounds run, steps kept in total, steps kept in the last round, points
 *   skipped at the returned pose, 0, 0}.
 * The points are rounded to float32 and normalised by the rule above.  State: a rotation R, t = t_in / |t_in|,
 *   E = [t]x R.  Residual of a masked point: r = d / sqrt(g) with a = E x1h, b = E^T x2h, d = x2 a0 + y2 a1 + a2,
 *   g = a0^2 + a1^2 + b0^2 + b1^2 (r^2: the Sampson error); a point with g = 0 or a residual that is not finite adds
 *   nothing and is counted.  Five parameters: R <- exp([w]x) R and t <- (t + u b1 + v b2) / |...| with b1 = e_k x t
 *   normalised (k: the first index of smallest |t_k|) and b2 = t x b1; the Jacobian is exact.  A step solves
 *   J^T J delta = -J^T r by full-pivot elimination and is kept only if the summed squared error falls; the first step not
 *   kept, or a singular system, ends the round; no damping.  Round 1 fits on mask_in; each later round first takes as
 *   its mask the points with float(Sampson error) <= float(thr^2) under the current E (thr as for cotr_ransac_essential)
 *   whose least-squares depths under the current (R, t) lie in (0, distance_thresh), then fits again.  A round with fewer
 *   than 5 points in its mask takes no step.  refine_iters = 0 with rounds = 1: R_out = R_in and t_out = t_in / |t_in|
 *   bit for bit.  found = 0, a non-finite R_in or t_in, or t_in = 0: every output is 0.
 *   5 <= n <= 2^24, threshold > 0 finite, distance_thresh > 0 finite, 1 <= rounds <= 8, 0 <= refine_iters <= 64.
 *   scratch: DEVICE, 16-byte aligned, at least cotr_refine_pose_scratch_bytes(n) bytes.
 * Stream-ordered, 2 + rounds (1 + 2 (refine_iters + 1)) launches whatever the data, no host waits and no allocation
 * (capturable); integer atomics only, sums in a fixed order: the same input gives the same bits.  Bad arguments are
 * checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_refine_pose_scratch_bytes(int n, size_t* bytes);
int cotr_refine_pose(const double* R_in, const double* t_in, const double* pts1, const double* pts2, int n, const double* K1,
                     const double* K2, double threshold, double distance_thresh, int rounds, int refine_iters,
                     const uint8_t* mask_in, const int32_t* found, double* R_out, double* t_out, double* E_out, uint8_t* mask_out,
                     int32_t* info_out, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- absolute pose: P3P RANSAC with a refit, and the lift of pixels through a depth map (cotr_amd/csrc/pnp.hip) ----------
 * The structure of cv2.solvePnPRansac(object, image, K, None, flags=cv2.SOLVEPNP_P3P) on the device, by rules of the
 * library's own (no bit-compatibility with OpenCV is claimed).  x_cam = R X + t.
 *
 * K: HOST pointer to 9 doubles, a row-major upper-triangular camera matrix (fx, skew, cx; 0, fy, cy; 0, 0, 1; only those
 *   five entries are read), finite, fx and fy not 0.
 * cotr_lift_pixels: depth [H,W] float32, points [n,2] float64 (x, y) in pixels, c2w [16] float64 row-major or NULL: DEVICE
 *   pointers -> out [n,3] float64.  The depth z is read at (rint(x), rint(y)) (ties to even); a point whose rounded index
 *   lies outside the map, or whose depth is not finite and > 0, gets three NaN.  Otherwise yn = (y - cy) / fy,
 *   xn = (x - cx - skew yn) / fx, X = (xn z, yn z, z), and with c2w its rows 0..2 applied to (X, 1).  1 <= n <= 2^24,
 *   H W <= 2^28.  One launch.
 * cotr_ransac_pnp: object_points [n,3], image_points [n,2] float64 DEVICE pointers (the image points rounded to float32
 *   first) -> R_out [9] (row-major), t_out [3] float64, mask_out [n] uint8 (the RANSAC inliers of the chosen candidate;
 *   not re-evaluated after the refit), info_out [8] int32 = {found, best inlier count, sequential iterations run, chosen
 *   slot (-1: none), refit steps kept, 0, 0, 0}; R_out = 0, t_out = 0, mask_out = 0 when nothing is found.  Iteration it
 *   draws 4 distinct indices with the sampler of cotr_ransac_fundamental and solves P3P on the first three in sample order
 *   (Grunert's quartic in the depth ratio v = s2 / s0, its roots in (0, 1e8) in ascending order, three Newton steps on the
 *   three distance equations, three positive depths, the rigid motion of the two triangles; a solution must re-project the
 *   three points within 1e-9 px); of the solutions with the fourth point in front of the camera the one with the smallest
 *   squared reprojection error there is the candidate (the first of equal ones).  No candidate: a short draw, a NaN among
 *   the four points, the three object points on a line, no solution.  A candidate is 9 doubles: rows 1 and 2 of R, then
 *   t; row 3 is their cross product.  The candidates are counted in parallel and the sequential RANSAC loop is replayed
 *   on the counts.  An inlier lies in front of the camera (z > 0) with float(squared reprojection error) <=
 *   float(threshold^2); a NaN object point never is one.  refine_iters > 0: up to that many Gauss-Newton steps on the
 *   inliers (R <- exp([w]x) R, t <- t + dt), each kept only if the summed squared error falls and every inlier stays in
 *   front; the first step not kept ends the refinement.  4 <= n <= 2^24, 1 <= max_iters <= 65536, threshold > 0 finite,
 *   0 < confidence < 1, 0 <= refine_iters <= 64.
 *   hyp_pose [max_iters][9] float64, hyp_count [max_iters] int32 (-1: no candidate; its entries are NaN), hyp_samples
 *   [max_iters][4] int32 (-1 past the indices drawn): optional DEVICE outputs (NULL: not written).
 *   scratch: DEVICE, 16-byte aligned, at least cotr_ransac_pnp_scratch_bytes(n, max_iters) bytes.
 * Stream-ordered, 4 + 2 (refine_iters + 1) launches (4 with refine_iters = 0) whatever the data, no host waits and no
 * allocation (capturable); integer atomics only, sums in a fixed order: the same input gives the same bits.  Bad arguments
 * are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_lift_pixels(const float* depth, int H, int W, const double* K, const double* c2w, const double* points, int n, double* out,
                     cotr_stream stream);
int cotr_ransac_pnp_scratch_bytes(int n, int max_iters, size_t* bytes);
int cotr_ransac_pnp(const double* object_points, const double* image_points, int n, const double* K, double threshold,
                    double confidence, int max_iters, uint64_t seed, int refine_iters, double* R_out, double* t_out,
                    uint8_t* mask_out, int32_t* info_out, double* hyp_pose, int32_t* hyp_count, int32_t* hyp_samples,
                    void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- 3D-3D registration: rigid and similarity RANSAC with a closed-form refit (cotr_amd/csrc/rigid3d.hip) ----------------
 * Robust absolute orientation (Kabsch / Horn / Umeyama) of n corresponding 3D points, by rules of the library's own
 * (DESIGN.md 3h-8).  y = s R x + t.
 *
 * cotr_ransac_rigid3d: src [n,3], dst [n,3] float64 DEVICE pointers, taken as they are -> R_out [9] (row-major), t_out [3],
 *   scale_out [1] float64, mask_out [n] uint8, info_out [8] int32 = {found, best inlier count, sequential iterations run,
 *   chosen slot (-1: none), refit rounds run, points in mask_out, 0, 0}; every output is 0 when nothing is found.
 *   Iteration it draws 3 distinct indices with the sampler of cotr_ransac_fundamental and solves Horn's closed form on the
 *   three pairs: the centroids, the centred 3 x 3 cross-covariance, the symmetric 4 x 4 matrix N of the quaternion method,
 *   the eigenvector of its first largest eigenvalue by cyclic Jacobi -> R (a proper rotation by construction); with_scale =
 *   1: s = sum (R a').b' / sum |a'|^2, finite and > 0; with_scale = 0: s = 1 exactly; t = cb - s R ca.  No candidate: a
 *   short draw, a NaN among the six points, a sample on a line in src or in dst (|e1 x e2| <= 1e-12 |e1| |e2|), the two
 *   largest eigenvalues of N not separated (l1 - l2 <= 1e-12 l1).  A candidate is 9 doubles: rows 1 and 2 of s R, then t;
 *   s = |row 1| and row 3 = (row 1 x row 2) / s (with_scale = 0: s = 1, row 3 = row 1 x row 2).  The candidates are counted
 *   in parallel and the sequential RANSAC loop is replayed on the counts.  An inlier has float(|s R x + t - y|^2) <=
 *   float(threshold^2), the threshold in dst's units; a pair with a NaN never is one.  rounds = 0: the outputs are the
 *   chosen candidate bit for bit (R_out = s R / s) and mask_out its inliers.  rounds > 0: round 1 fits the closed form on
 *   the RANSAC mask (two passes: the centroids, then the centred moments); each later round first re-counts the inliers of
 *   the current model among all n points and fits on those.  A round whose mask holds fewer than 3 points or whose moments
 *   are degenerate is skipped: the model stays and no later round runs.  mask_out is the mask the last executed round
 *   fitted on.  3 <= n <= 2^24, 1 <= max_iters <= 65536, threshold > 0 finite with a finite non-zero float32 square,
 *   0 < confidence < 1, with_scale 0 or 1, 0 <= rounds <= 8.
 *   hyp_model [max_iters][9] float64, hyp_count [max_iters] int32 (-1: no candidate; its entries are NaN), hyp_samples
 *   [max_iters][3] int32 (-1 past the indices drawn): optional DEVICE outputs (NULL: not written).
 *   scratch: DEVICE, 16-byte aligned, at least cotr_ransac_rigid3d_scratch_bytes(n, max_iters) bytes.
 * Stream-ordered, 4 launches with rounds = 0 and 4 + 4 + 6 (rounds - 1) otherwise, whatever the data, no host waits and no
 * allocation (capturable); integer atomics only, sums in a fixed order: the same input gives the same bits.  Bad arguments
 * are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_ransac_rigid3d_scratch_bytes(int n, int max_iters, size_t* bytes);
int cotr_ransac_rigid3d(const double* src, const double* dst, int n, double threshold, double confidence, int max_iters,
                        uint64_t seed, int with_scale, int rounds, double* R_out, double* t_out, double* scale_out,
                        uint8_t* mask_out, int32_t* info_out, double* hyp_model, int32_t* hyp_count, int32_t* hyp_samples,
                        void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- dense registration of two depth maps: point-to-plane ICP (cotr_amd/csrc/icp.hip; rules in DESIGN.md 3h-9) -----------
 * Projective data association with a point-to-plane Gauss-Newton step, by rules of the library's own.  x_a = R x_b + t.
 *
 * cotr_icp_depth: depth_a [Ha,Wa], depth_b [Hb,Wb] float32 DEVICE; K_a, K_b HOST, 9 doubles each as in cotr_lift_pixels;
 *   R0 [9], t0 [3] float64 DEVICE, the start (they may be the outputs of cotr_ransac_rigid3d); c2w_a [16] float64 DEVICE or
 *   NULL: NULL, the poses are x_a = R x_b + t in A's camera frame; given, the start and the result map B's camera frame to
 *   the world frame, and the start is taken into A's camera frame with the rigid inverse (R_a^T, -R_a^T t_a) and the result
 *   back.  found: int32 DEVICE or NULL; found[0] == 0: every output is 0 (assoc_out -1) and the chain idles.  src_mask
 *   [Hb,Wb] uint8 DEVICE or NULL: only source pixels whose entry is not 0 may be used.
 *   Maps, of both captures: the vertex of pixel (x, y) is cotr_lift_pixels' point of (x, y) without c2w, NaN where the
 *   depth is not finite and > 0.  The normal of an interior pixel is (V(x+1,y) - V(x-1,y)) x (V(x,y+1) - V(x,y-1)) over
 *   its norm, negated when n . V > 0; it exists only when all five depths are valid, each of the four neighbours has
 *   |z_nb - z| <= edge z, and the norm is > 0.  Border pixels have none.
 *   One evaluation at (R, t), over the source pixels x % stride == 0 and y % stride == 0 of B in row-major order: a pixel
 *   makes a pair when, in this order, it has a normal and src_mask admits it; Y = R X_b + t has Y_z > 0; (rint u, rint v)
 *   (ties to even) of u = (fx xn + skew yn) + cx, v = fy yn + cy, xn = Y_x / Y_z, yn = Y_y / Y_z through K_a lies inside
 *   A; A has a normal n_a there; |Y - V_a|^2 <= max_dist^2; (R n_b) . n_a >= normal_cos.  Its residual is r = n_a . (Y -
 *   V_a), its Jacobian row over (w, dt) of R <- exp([w]x) R, t <- t + dt is ((R X_b) x n_a, n_a).  29 sums in a fixed
 *   order: the upper triangle of J^T J row-major (21), J^T r (6), sum r^2, the pairs.
 *   The chain stops and the pose stays when the pairs are fewer than 6 (stop reason 1), a sum is not finite (3), or the
 *   normal matrix is ill-conditioned (2): its eigenvalues by cyclic Jacobi, l_min <= cond_tol l_max.  Otherwise the step
 *   -V diag(1 / l) V^T (J^T r) is taken, every time: the pairs change with the pose, so no fall of an error is asked for.
 *   iters steps at most, iters + 1 evaluations; the last only evaluates.
 *   -> R_out [9] (row-major), t_out [3] float64; info_out [8] int32 = {ok: ran all its evaluations, steps taken, pairs at
 *   the returned pose, stop reason (0: ran all), source pixels that have a normal and are admitted by src_mask, pixels of
 *   A with a normal, 0, 0}; stats_out [2] float64 = {sum r^2, sqrt(sum r^2 / pairs)} at the returned pose.
 *   Optional DEVICE outputs (NULL: not written): hist_out [iters + 1][32] float64, the 29 sums of every evaluation, then
 *   l_min, l_max (0 where no step was solved for) and 0; rows after a stop are 0.  assoc_out [n_src] int32, n_src =
 *   ceil(Hb / stride) ceil(Wb / stride): for the evaluation at the returned pose, the pixel index of A paired with each
 *   source pixel, or -1.  maps_a_out [Ha Wa][6], maps_b_out [Hb Wb][6] float64: vertex, then normal, of every pixel.
 *   3 <= H, W and H W <= 2^28 on both sides, 1 <= stride <= 64, 0 <= iters <= 64, max_dist > 0 finite, -1 <= normal_cos
 *   <= 1, edge > 0 finite, 0 < cond_tol < 1.
 *   scratch: DEVICE, 16-byte aligned, at least cotr_icp_depth_scratch_bytes(Ha, Wa, Hb, Wb, stride) bytes.
 * Stream-ordered, 3 + 2 (iters + 1) launches whatever the data (a prologue, the two maps, iters + 1 pairs of accumulate and
 * finish; the last finish is the epilogue), no host waits and no allocation (capturable); integer atomics only, sums in a
 * fixed order: the same input gives the same bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the
 * message in cotr_raster_last_error(). */
int cotr_icp_depth_scratch_bytes(int Ha, int Wa, int Hb, int Wb, int stride, size_t* bytes);
int cotr_icp_depth(const float* depth_a, int Ha, int Wa, const double* K_a, const float* depth_b, int Hb, int Wb,
                   const double* K_b, const double* R0, const double* t0, const double* c2w_a, const int32_t* found,
                   const uint8_t* src_mask, double max_dist, double normal_cos, double edge, double cond_tol, int iters,
                   int stride, double* R_out, double* t_out, int32_t* info_out, double* stats_out, double* hist_out,
                   int32_t* assoc_out, double* maps_a_out, double* maps_b_out, void* scratch, size_t scratch_bytes,
                   cotr_stream stream);

/* ---- joint registration of n depth maps: multi-way point-to-plane ICP (cotr_amd/csrc/icp_multi.hip) -------
 * All free camera-to-world poses of n depth maps of one size are refined together, on every ordered pair (edge) of a graph of
 * views, with one normal system per step.  The rules are the library's own.  Neither call takes a scratch: all device state
 * lives in the outputs below.
 *
 * cotr_icp_maps: depths [n][H][W] float32 DEVICE; Ks HOST [n][9], each as K in cotr_lift_pixels; edge as in cotr_icp_depth.
 *   -> maps_out [n][H][W][6] float64 DEVICE: the vertex, then the normal, of every pixel by the rule of cotr_icp_depth (its
 *   maps_a_out, bit for bit), NaN where there is none; info_out [n][4] int32 = {pixels with a vertex, pixels with a normal,
 *   0, 0}.  1 <= n <= 32, 3 <= H, W, n H W <= 2^28, edge > 0 finite.  2 launches: a prologue, one thread a pixel.
 *
 * cotr_icp_multiview: maps [n][H][W][6] float64 DEVICE, what cotr_icp_maps writes; Ks HOST [n][9]; c2w0 [n][16] float64
 *   DEVICE, the start, row-major [R | t] camera-to-world (c2w_out may be c2w0); edges [E][2] int32 DEVICE = (a, b): A = view a
 *   is the target, B = view b the source; fixed_mask: bit v set, view v does not move; centre HOST [3], the point c the
 *   twists turn about (the mean of the camera centres keeps the system well scaled); found int32 DEVICE [n] or NULL.
 *   An edge is dead when an index is outside [0, n), a == b, found is 0 for either view, or an earlier edge names the same
 *   ordered pair.  A dead edge has no pairs, its rows of edge_out are 0 and its rows of assoc_out -1.
 *   One evaluation of a live edge at the working poses: R_ab[i][j] = (R_a[0][i] R_b[0][j] + R_a[1][i] R_b[1][j]) + R_a[2][i]
 *   R_b[2][j], d = t_b - t_a, t_ab[i] = (R_a[0][i] d[0] + R_a[1][i] d[1]) + R_a[2][i] d[2]; then the gates of cotr_icp_depth
 *   at R = R_ab, t = t_ab, in its order and with its arithmetic, through K_a, over the source pixels x % stride == 0 and y %
 *   stride == 0 of B in row-major order (usable: B has a normal there), and its residual r = n_a . (Y - V_a).  A pose is
 *   perturbed by a world-frame twist about c: R <- exp([w]x) R, t <- exp([w]x) (t - c) + c + dt.  With N[i] = (R_a[i][0]
 *   n_x + R_a[i][1] n_y) + R_a[i][2] n_z and Yc[i] = (((R_a[i][0] Y_x + R_a[i][1] Y_y) + R_a[i][2] Y_z) + t_a[i]) - c[i], the
 *   Jacobian row of r over (w, dt) of view b is J = (Yc x N, N) = (Yc_1 N_2 - Yc_2 N_1, Yc_2 N_0 - Yc_0 N_2, Yc_0 N_1 - Yc_1
 *   N_0, N), and over those of view a it is -J.  29 sums as in cotr_icp_depth: the upper triangle of J^T J row-major (21),
 *   J^T r (6), sum r^2, the pairs.
 *   The source rows are cut into 8 bands, band s = rows [floor(s Hs / 8), floor((s + 1) Hs / 8)) of the Hs = ceil(H / stride)
 *   source rows; one workgroup per (edge, band) adds its band's terms in a fixed order (per thread in row-major order, per
 *   wavefront, across wavefronts) -> edge_out[e][s][0..28], [29] = the band's usable source pixels, [30], [31] = 0.
 *   The step: a sum of an edge is that of its 8 bands in band order.  An edge with fewer than 6 pairs is dropped for the
 *   step; the others are kept.  A view is free when it is not in fixed_mask, is found and has a kept edge; the free views
 *   take slots in index order, 6 unknowns (w, dt) each.  The system: block (v, v) = the sum of J^T J over the kept edges that
 *   touch v, the other view w ascending and (v, w) before (w, v); block (a, b) = -(J^T J of (lo, hi) + J^T J of (hi, lo)), lo
 *   < hi the two views; the gradient of v: over w ascending, - J^T r of (v, w), then + J^T r of (w, v).  Cholesky by columns
 *   on the packed lower triangle (at most 186 unknowns) fails when a pivot is not finite or <= pivot_tol times that entry's
 *   original diagonal value; x solves system x = gradient, and every free view takes the twist (w, dt) = -x of its slot.
 *   The chain stops, and the poses stay, with stop reason 1: no free view or fewer than 6 pairs over the kept edges; 3: sum
 *   r^2 or an entry of the assembled system is not finite; 2: Cholesky failed.  The pivot rule detects a structurally
 *   singular system only (a component of views tied to each other and to no fixed view: ratio <= 2e-16); a geometric slide,
 *   such as views of two planes alone, passes it: the pairwise call has the eigenvalue test for that, and the per-edge sums of
 *   edge_out are there so that a caller can examine an edge's normal matrix.  Otherwise every step is taken.  iters steps at
 *   most, iters + 1 evaluations; the last only evaluates.
 *   -> c2w_out [n][16] float64: the working poses, returned; info_out [8] int32 = {ok: ran all its evaluations, steps taken,
 *   pairs over the kept edges at the returned poses, stop reason (0: ran all), live edges, edges kept at the last
 *   evaluation, free views, 0}; view_info_out [n][4] int32 = {free, pairs over its kept edges, kept edges, 0}; stats_out [2]
 *   float64 = {sum r^2 over the kept edges in edge order, sqrt(sum r^2 / pairs)}; edge_out [E][8][32] float64 (above), of
 *   the evaluation at the returned poses.  Optional DEVICE outputs (NULL: not written): hist_out [iters + 1][4] float64 =
 *   {sum r^2, pairs, smallest pivot over its original diagonal value (0 where no step was solved for), 0} of every
 *   evaluation, rows after a stop 0; assoc_out [E][n_src] int32, n_src = ceil(H / stride) ceil(W / stride): for the
 *   evaluation at the returned poses, the pixel of A paired with each source pixel, or -1.
 *   2 <= n <= 32, 3 <= H, W, n H W <= 2^28, 1 <= E <= n (n - 1), fixed_mask with a bit below n, 0 <= iters <= 64, 1 <= stride
 *   <= 64, max_dist > 0 finite, -1 <= normal_cos <= 1, 0 < pivot_tol < 1, centre finite.
 * Stream-ordered, 1 + 2 (iters + 1) launches whatever the data (a prologue, iters + 1 pairs of edge and solve kernel), no host
 * waits and no allocation (capturable); integer atomics only, sums in a fixed order: the same input gives the same bits.
 * Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_icp_maps(const float* depths, int n, int H, int W, const double* Ks, double edge, double* maps_out,
                  int32_t* info_out, cotr_stream stream);
int cotr_icp_multiview(const double* maps, int n, int H, int W, const double* Ks, const double* c2w0, const int32_t* edges,
                       int E, uint32_t fixed_mask, const double* centre, const int32_t* found, double max_dist,
                       double normal_cos, double pivot_tol, int iters, int stride, double* c2w_out, int32_t* info_out,
                       int32_t* view_info_out, double* stats_out, double* edge_out, double* hist_out, int32_t* assoc_out,
                       cotr_stream stream);

/* ---- a fused model of posed depth maps: TSDF integration and raycast (cotr_amd/csrc/tsdf.hip; rules in DESIGN.md 3h-11) ---
 * A truncated signed distance volume that averages registered depth maps, and the depth map of its zero crossing seen from
 * a pose: the map cotr_icp_depth tracks the next capture against.  The rules are the library's own.
 *
 * The volume: tsdf, weight float32 [Nz][Ny][Nx] DEVICE, x fastest, owned by the caller; a fresh volume has tsdf = 1 and
 *   weight = 0.  origin: HOST, 3 doubles, the world position of the centre of voxel (0, 0, 0); voxel > 0: the voxel's side.
 *   2 <= Nx, Ny, Nz and Nx Ny Nz <= 2^28.  Storage is float32; every intermediate below is float64, and no product is
 *   contracted into an FMA.
 * cotr_tsdf_integrate: depths [n][H][W] float32 DEVICE, 1 <= n <= 32, 1 <= H, W and H W <= 2^28; Ks HOST [n][9], each as K
 *   in cotr_lift_pixels; c2w [n][16] float64 DEVICE, row-major camera-to-world [R | t] (it may be built from the outputs of
 *   cotr_icp_depth without a host trip); found int32 DEVICE [n] or NULL: a capture whose entry is 0 is skipped; obs_weight
 *   HOST [n] or NULL (every w = 1): each finite and > 0; trunc > 0 finite; max_weight > 0.
 *   One thread owns a voxel and takes the captures in the order 0 .. n-1, so the result is the same bits as n calls of one
 *   capture each; the volume is read once and written once whatever n is.  Voxel (i, j, k), capture c:
 *   P = origin + voxel (i, j, k) (each origin_a + voxel * index); D = P - t; Y = R^T D, each component (R_0a D_0 + R_1a D_1)
 *   + R_2a D_2.  Skipped unless Y_z > 0.  xn = Y_x / Y_z, yn = Y_y / Y_z, u = (fx xn + skew yn) + cx, v = fy yn + cy (the rule
 *   of cotr_icp_depth); skipped unless (rint u, rint v) (ties to even) lies inside the map.  z: the depth there; skipped
 *   unless it is finite and > 0.  sdf = z - Y_z; skipped when sdf < -trunc.  d = min(1, sdf / trunc);
 *   tsdf <- float32((double(tsdf) double(weight) + d w) / (double(weight) + w)), then
 *   weight <- float32(min(double(weight) + w, max_weight)).
 *   -> info_out int32 [n][4] = {integrated (0 when found skipped it), voxels updated, voxels whose pixel held a valid
 *   depth, 0}.
 * cotr_tsdf_raycast: K HOST; c2w [16] float64 DEVICE; found int32 DEVICE [1] or NULL: found[0] == 0: every output is 0.
 *   1 <= H, W and H W <= 2^28; near >= 0, far > near, step > 0, all finite, S = ceil((far - near) / step) <= 65536.
 *   One thread owns a pixel (x, y).  yn = (y - cy) / fy, xn = (x - cx - skew yn) / fx (cotr_lift_pixels' rule at the pixel
 *   centre), m = sqrt((xn^2 + yn^2) + 1), the direction in the camera frame c = (xn / m, yn / m, 1 / m) and in the world
 *   d_a = (R_a0 c_0 + R_a1 c_1) + R_a2 c_2.  Sample k = 0 .. S lies at s_k = near + k step (a product, not a running sum),
 *   p = t + s_k d.  A sample at p: g = (p - origin) / voxel, i0 = floor(g); valid iff 0 <= i0 <= N - 2 on each axis and all 8
 *   corners i0 + {0, 1}^3 have weight > 0; its value f is the trilinear blend of their tsdf with fr = g - i0, every blend
 *   a + fr (b - a), along x, then y, then z.  The first k whose previous sample is valid with f_prev > 0 and whose own is
 *   valid with f <= 0 is a hit at s* = s_(k-1) + step (f_prev / (f_prev - f)).  A valid f_prev < 0 followed by a valid f > 0
 *   is a back face: the ray ends with no hit.  An invalid sample resets "previous".
 *   -> depth_out float32 [H][W] = s* c_2, 0 where there is no hit: a valid input of cotr_icp_depth, cotr_lift_pixels and
 *   cotr_tsdf_integrate.  normal_out float64 [H][W][3] DEVICE or NULL, in the camera frame: at p* = t + s* d the gradient
 *   G_a = f(p* + voxel e_a) - f(p* - voxel e_a) from six more samples, L = sqrt((G_0^2 + G_1^2) + G_2^2), n_a = ((R_0a G_0 +
 *   R_1a G_1) + R_2a G_2) / L; three NaN where there is no hit, one of the six samples is invalid or L is not > 0.
 *   info_out int32 [4] = {ok (found), pixels hit, rays ended at a back face, 0}.
 * Stream-ordered, 2 launches each whatever the data (a prologue that sets info_out, then the volume or the image), no host
 * waits and no allocation (capturable); integer atomics only: the same input gives the same bits.  Bad arguments are checked
 * before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_tsdf_integrate(float* tsdf, float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, double trunc,
                        const float* depths, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                        const double* obs_weight, double max_weight, int32_t* info_out, cotr_stream stream);
int cotr_tsdf_raycast(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel,
                      const double* K, const double* c2w, const int32_t* found, int H, int W, double near, double far,
                      double step, float* depth_out, double* normal_out, int32_t* info_out, cotr_stream stream);

/* ---- the colour of a TSDF volume: fuse images, colour points and depth maps (cotr_amd/csrc/tsdf.hip) ------
 * A third array beside tsdf and weight that averages the captures' 8-bit images near the surface, and its colour at points
 * (the vertices of cotr_tsdf_mesh) and at the pixels of a depth map (the map of cotr_tsdf_raycast).  The rules are the
 * library's own.
 *
 * The colour volume: color float32 [Nz][Ny][Nx][4] DEVICE = (r, g, b, colour weight), x fastest, owned by the caller, 16-byte
 *   aligned, all 0 when fresh; colours on the images' scale 0 .. 255.  Nx, Ny, Nz, origin, voxel: those of
 *   cotr_tsdf_integrate.  Storage is float32; every intermediate below is float64, and no product is contracted into an FMA.
 * cotr_tsdf_color_integrate: depths, n, H, W, Ks, c2w, found, obs_weight, trunc, max_weight as in cotr_tsdf_integrate; images
 *   uint8 [n][H][W][3] DEVICE.  tsdf and weight are neither read nor written: the depth call and the colour call may come in
 *   either order.  Voxel (i, j, k), capture c: Y, (u, v), the pixel (rint u, rint v) and its depth z by the expressions of
 *   cotr_tsdf_integrate in their order; skipped where that call skips before sdf.  sdf = z - Y_z; skipped when sdf < -trunc or
 *   sdf > trunc: only the band around the surface takes a colour, not the free space in front of it.  p: the three bytes of
 *   that pixel as doubles, Wc the stored colour weight:
 *   each channel <- float32((double(channel) double(Wc) + p w) / (double(Wc) + w)), then
 *   Wc <- float32(min(double(Wc) + w, max_weight)).
 *   One thread owns a voxel and takes the captures in the order 0 .. n-1: the same bits as n calls of one capture each.
 *   -> info_out int32 [n][4] = {integrated (0 when found skipped it), voxels coloured, voxels whose pixel held a valid
 *   depth (the third column of cotr_tsdf_integrate for the same capture), 0}.
 * The colour at a world point p: q_a = (p_a - origin_a) / voxel; p is in the box iff 0 <= q_a <= N_a - 1 on each axis (false
 *   for NaN; the faces belong to it, unlike a raycast sample, so that a mesh vertex on the last voxel layer has a colour).
 *   b_a = min(floor(q_a), N_a - 2), r_a = q_a - b_a; the corner b + (dx, dy, dz) has beta = (wx wy) wz with w = r for d = 1
 *   and 1 - r for d = 0, and counts iff its colour weight is > 0.  Over the corners that count, dx fastest, then dy, then dz,
 *   S and C_ch are the running sums of beta and beta c_ch from 0.  The point is valid iff it is in the box and S > 0; its
 *   channel is rint(C_ch / S) (ties to even) clamped to 0 .. 255: renormalised over the coloured corners, so that colour
 *   reaches the rim of what the cameras saw.
 * cotr_tsdf_color_points: points float64 [n][3] DEVICE in the world frame, 0 <= n <= 2^28 (points, rgb_out and valid_out may
 *   be NULL with n = 0); found int32 DEVICE [1] or NULL: found[0] == 0: every output is 0.  -> rgb_out uint8 [n][3] ((0, 0,
 *   0) at an invalid point), valid_out uint8 [n], info_out int32 [4] = {ok (found), valid points, 0, 0}.
 * cotr_tsdf_color_map: depth float32 [H][W] DEVICE (as cotr_tsdf_raycast writes it), K HOST, c2w [16] float64 DEVICE, found
 *   as above; 1 <= H, W and H W <= 2^28.  Pixel (x, y) with a depth z that is finite and > 0: yn = (y - cy) / fy, xn = (x - cx -
 *   skew yn) / fx (the raycast's ray), Y = (xn z, yn z, z), p_a = ((R_a0 Y_x + R_a1 Y_y) + R_a2 Y_z) + t_a, and the colour at
 *   p by the rule above.  -> rgb_out uint8 [H][W][3], (0, 0, 0) at every other pixel and where p is not valid; info_out int32
 *   [4] = {ok (found), pixels coloured, pixels with a depth, 0}.
 * Stream-ordered, 2 launches each whatever the data (1 for cotr_tsdf_color_points with n = 0), no scratch, no host waits and
 * no allocation (capturable); integer atomics only, and only for info_out: the same input gives the same bits.  Bad
 * arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_tsdf_color_integrate(float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, double trunc,
                              const float* depths, const uint8_t* images, int n, int H, int W, const double* Ks,
                              const double* c2w, const int32_t* found, const double* obs_weight, double max_weight,
                              int32_t* info_out, cotr_stream stream);
int cotr_tsdf_color_points(const float* color, int Nx, int Ny, int Nz, const double* origin, double voxel,
                           const double* points, int n, const int32_t* found, uint8_t* rgb_out, uint8_t* valid_out,
                           int32_t* info_out, cotr_stream stream);
int cotr_tsdf_color_map(const float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, const float* depth,
                        int H, int W, const double* K, const double* c2w, const int32_t* found, uint8_t* rgb_out,
                        int32_t* info_out, cotr_stream stream);

/* ---- the surface of a TSDF volume as an indexed triangle mesh (cotr_amd/csrc/tsdf.hip; rules in DESIGN.md 3h-12) ----------
 * Marching tetrahedra on the Kuhn split of every cell: no case table to trust, no ambiguous face, closed and consistently
 * oriented meshes by construction, about twice the triangles of marching cubes.  The rule is the library's own.
 *
 * The volume is the one of cotr_tsdf_integrate, here with 2 <= Nx, Ny, Nz and Nx Ny Nz <= 2^27 (12 triangles a cell in an
 *   int32).  A corner is inside iff tsdf <= 0 (the raycast's hit rule).  Cell c = (i, j, k), 0 <= i <= Nx - 2 and likewise j, k,
 *   is valid iff its 8 corners all have weight > 0.
 * Tetrahedra: cell c is split into T_0 .. T_5, one for each permutation p of the axes in lexicographic order (xyz, xzy, yxz,
 *   yzx, zxy, zyx): q0 = c, q1 = q0 + e_p1, q2 = q1 + e_p2, q3 = c + (1, 1, 1).  Every tetrahedron edge is (v, v + d) with d in
 *   {0, 1}^3 \ {0}, and every face diagonal runs from the face's low corner to its high corner, so neighbouring cells agree.
 * Vertices: edge (v, d) crosses iff exactly one end is inside and is live iff it crosses and some valid cell contains it.
 *   Each live edge carries one vertex: with fa, fb the float32 values at v and v + d as doubles, t = fa / (fa - fb); grid
 *   coordinate g_a = v_a + t where d_a = 1, else v_a; world coordinate p_a = origin_a + voxel * g_a.  Vertices are numbered in
 *   the order of (linear index of v with x fastest, dcode = dx + 2 dy + 4 dz).  Every vertex is referenced by a triangle.
 * Triangles: the valid cells in linear order, in each T_0 .. T_5.  S: the inside vertices among q0 .. q3; E_ab (a < b): the
 *   vertex on edge (q_a, q_b).  0 or 4 inside: nothing.  1 inside, {a}, or 3 inside with {a} outside: with b < c < d the
 *   others, (E_ab, E_ac, E_ad).  2 inside {a, b}, a < b, with {c, d} outside, c < d: (E_ac, E_ad, E_bd), then (E_ac, E_bd,
 *   E_bc).  Each triangle is written so, or with its second and third vertex swapped, whichever makes (B - A) x (C - A) point
 *   to the outside (tsdf > 0): that depends on the tetrahedron and S alone.  Triangles of no area (a corner value of exactly
 *   0) are kept: the counts are combinatorial.
 * Normals (normals_out not NULL): at the vertex's grid coordinates g, G_a = f(g + e_a) - f(g - e_a), f the trilinear value
 *   of cotr_tsdf_raycast with its validity (0 <= floor <= N - 2 on each axis, all 8 corners observed); n = G / sqrt((G_0^2 +
 *   G_1^2) + G_2^2), in the world frame; three NaN where one of the six samples is invalid or the length is not > 0.
 * cotr_tsdf_mesh: found int32 DEVICE [1] or NULL: found[0] == 0: every count is 0, every written row of tris_out is -1 and
 *   verts_out, normals_out are not touched.  verts_out float64 [cap_verts][3] DEVICE (NULL with cap_verts = 0); normals_out
 *   float64 [cap_verts][3] DEVICE or NULL; tris_out int32 [cap_tris][3] DEVICE (NULL with cap_tris = 0).  Capacities as in
 *   cotr_depth_corrs: a vertex or triangle beyond its capacity is counted, not written; the rows of tris_out past the count
 *   are -1; a triangle that refers to a vertex beyond cap_verts is written all the same.  Both capacities 0: the call only
 *   counts.  info_out int32 [4] DEVICE = {ok (found), vertices, triangles, valid cells}.  scratch: DEVICE, 16-byte aligned,
 *   cotr_tsdf_mesh_scratch_bytes(Nx, Ny, Nz) bytes (6 a voxel).
 * Stream-ordered; 4 launches, one more with a capacity above 0 and one more with cap_tris above 0, whatever the data; no
 * host waits and no allocation (capturable).  Every output position comes from a scan; integer atomics only, and only for
 * info_out: the same input gives the same bytes.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the
 * message in cotr_raster_last_error(). */
int cotr_tsdf_mesh_scratch_bytes(int Nx, int Ny, int Nz, size_t* bytes);
int cotr_tsdf_mesh(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel,
                   const int32_t* found, double* verts_out, int cap_verts, double* normals_out, int32_t* tris_out, int cap_tris,
                   int32_t* info_out, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- structure from known cameras: robust N-view triangulation (cotr_amd/csrc/structure.hip; rules in DESIGN.md 3h-6) ----
 * n correspondences seen in V posed views -> their 3D points, the views each point was fitted on, and the per-point
 * figures a reconstruction filters on.  The rules are the library's own.
 *
 * DEVICE pointers: points [V][n][2] float64 (x, y) in pixels, view-major, rounded to float32 first; visible [V][n] uint8
 *   or NULL (every view sees every point); cams [V][5] float64 (fx, fy, cx, cy, skew); poses [V][12] float64, the
 *   world-to-camera [R | t] row-major (x_cam = R X + t); found int32 or NULL: when found[0] is 0 every output is 0.
 * A view whose camera or pose has an entry that is not finite, a focal length of 0 or a centre c = -R^T t that is not
 *   finite sees no point.  Ray of a point in a view: d = R^T (x, y, 1) normalised, (x, y) by the rule of
 *   cotr_ransac_essential.  S: the visible views of the point whose rounded coordinates are finite, ascending; fewer than
 *   two: the point has too few views.
 * Ray least squares over a set of views: (sum I - d d^T) X = sum (I - d d^T) c, summed ascending, solved by cofactors; a
 *   determinant that is 0 or not finite, or a coordinate that is not finite: degenerate.
 * robust = 1: every pair i < j of S in lexicographic order is triangulated by that rule and counts the views of S with depth
 *   > 0 and float(squared reprojection error) <= float(threshold^2); the first pair with the largest count gives U, its
 *   inlier views; a count below 2: too few views.  robust = 0: U = S.
 * Fit: X = ray least squares over U, then up to refine_iters undamped Gauss-Newton steps on the summed squared pixel error
 *   over U (analytic Jacobian, the 3 x 3 system by cofactors); none unless every view of U has depth > 0 at the start; a
 *   step is kept only if the error falls and every view of U keeps depth > 0; the first step not kept, or a degenerate
 *   system, ends the fit.
 * rule = 1 (V = 2, robust = 0, refine_iters = 0 only): X = c_a + s d_a, the point of ray A nearest ray B,
 *   s = (d_a.w - (d_a.d_b)(d_b.w)) / (1 - (d_a.d_b)^2), w = c_b - c_a; a denominator of 0: degenerate.
 * -> X_out [n][3] float64 (NaN: not solved), used_out [V][n] uint8 (U; 0 when not solved), quality_out [n][5] float64 over
 *   U at X = {mean squared reprojection error, largest, smallest depth, largest depth, smallest cosine between two rays}
 *   (NaN when not solved), mask_out [n] uint8 = solved, every depth in (0, distance_thresh), every float(error) <=
 *   float(threshold^2) and the smallest cosine <= max_cos; info_out [8] int32 = {found, points in mask_out, points with too
 *   few views, degenerate points, solved points dropped by depth, by error (depth passed), by parallax (both passed), steps
 *   kept in total}.
 * 2 <= V <= 32, 1 <= n <= 2^24, threshold > 0 finite with a squared float32 that is finite and not 0, -1 <= max_cos <= 1,
 *   distance_thresh > 0 finite, 0 <= refine_iters <= 64, robust and rule 0 or 1.  points and scratch 16-byte aligned;
 *   scratch: DEVICE, at least cotr_triangulate_views_scratch_bytes(V, n) bytes.
 * Stream-ordered, 2 launches whatever the data, no host waits and no allocation (capturable); a thread per point sums in a
 * fixed order and the counters are integer atomics: the same input gives the same bits.  Bad arguments are checked before
 * any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_triangulate_views_scratch_bytes(int V, int n, size_t* bytes);
int cotr_triangulate_views(const double* points, const uint8_t* visible, const double* cams, const double* poses, int V, int n,
                           const int32_t* found, double threshold, double max_cos, double distance_thresh, int refine_iters,
                           int robust, int rule, double* X_out, uint8_t* used_out, double* quality_out, uint8_t* mask_out,
                           int32_t* info_out, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- bundle adjustment: poses and points refined together (cotr_amd/csrc/bundle.hip; rules in DESIGN.md 3h-7) ----
 * Levenberg-Marquardt on the summed squared pixel error over the poses of the views that are not fixed and the points, the
 * points eliminated by the Schur complement.  The intrinsics are not optimised.  The rules are the library's own.
 *
 * DEVICE pointers: points, visible, cams, poses_in (the world-to-camera poses to start from), found: as for
 *   cotr_triangulate_views, with its view validity and its projection (z, xn, yn, du, dv, e); X_in [n][3] float64, the
 *   points to start from.  fixed_views: HOST uint8 [V] (read before the call returns), not 0: the view's pose is held; NULL:
 *   view 0 alone.
 * Eligible observation (v, p): the view is valid, sees the point, both rounded coordinates are finite, X of p is finite.
 * The set of round 1: the eligible observations with z > 0 at the input state; of a later round: those with z in (0,
 *   distance_thresh) and float(e) <= float(threshold^2) at the current state.  A view that is not fixed with fewer than 4
 *   observations in the set is frozen for the round (its pose stays, its observations leave the set); after that a point
 *   with fewer than 2 observations is a landmark for the round (its X stays, its observations still constrain the views).
 *   No free view left, or no observation: the round takes no step.
 * Parameters: per free view R <- exp([w]x) R (Rodrigues, as cotr_ransac_pnp) and t <- t + dt; per point X <- X + dX;
 *   exact Jacobians Jc (2 x 6) and Jp (2 x 3) per observation.  An iteration at damping lambda: V_p = sum Jp^T Jp,
 *   g_p = sum Jp^T r, U_v = sum Jc^T Jc, g_v = sum Jc^T r, W_vp = Jc^T Jp; the diagonals of U_v and V_p times (1 + lambda);
 *   V_p* inverted by the cofactor rule of cotr_triangulate_views (a determinant that is 0 or not finite: a landmark for this
 *   iteration); S_vw = [v = w] U_v* - sum_p W_vp V_p*^-1 W_wp^T, b_v = g_v - sum_p W_vp V_p*^-1 g_p; S dc = b by Cholesky (a
 *   pivot <= 0 or not finite rejects the step); dX_p = V_p*^-1 (g_p - sum_v W_vp^T dc_v); the candidate is the state minus
 *   the steps and is kept only if its summed e over the set is strictly smaller (a NaN rejects) and every observation of
 *   the set keeps z > 0.  Kept: lambda <- max(lambda / 10, 1e-12); rejected: lambda <- 10 lambda.  A round starts at lambda0
 *   and ends after iters iterations or when lambda exceeds 1e12.
 * -> poses_out [V][12], X_out [n][3] float64 (views and points that never moved: the input bit for bit), used_out [V][n]
 *   uint8 (the last round's set), stats_out [4] float64 = {cost of round 1's set at the input state, cost of the last
 *   round's set at the output state, the last lambda, 0}, info_out [8] int32 = {found, observations in the last set, free
 *   views of the last round, views frozen, landmarks, steps kept in total, steps rejected in total, rounds run}; found[0] =
 *   0: every output is 0.
 * 2 <= V <= 32, 1 <= n <= 2^20, 1 <= rounds <= 8, 0 <= iters <= 64, 1e-12 <= lambda0 <= 1e12, threshold as for
 *   cotr_triangulate_views, distance_thresh > 0 finite, at least one view fixed and one not.  points and scratch 16-byte
 *   aligned; scratch: DEVICE, at least cotr_bundle_adjust_scratch_bytes(V, n) bytes (O(n + chunks V^2): the Jacobians are
 *   recomputed where needed, not stored).
 * Stream-ordered, 3 + rounds (3 + 5 iters) launches whatever the data (rejected iterations and those after a round's end
 * cost their launches and change nothing), no host waits and no allocation (capturable); integer atomics only, every
 * floating-point sum in a fixed order: the same input gives the same bits.  Bad arguments are checked before any HIP call:
 * COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_bundle_adjust_scratch_bytes(int V, int n, size_t* bytes);
int cotr_bundle_adjust(const double* points, const uint8_t* visible, const double* cams, const double* poses_in,
                       const double* X_in, const uint8_t* fixed_views, int V, int n, const int32_t* found, double threshold,
                       double distance_thresh, int rounds, int iters, double lambda0, double* poses_out, double* X_out,
                       uint8_t* used_out, double* stats_out, int32_t* info_out, void* scratch, size_t scratch_bytes,
                       cotr_stream stream);

/* ---- the poses of N views from pairwise results: rotation averaging and the position solve (cotr_amd/csrc/global_pose.hip;
 *      rules in DESIGN.md 3h-19) ----
 * The global step between the two-view poses and the bundle adjustment.  Poses are world-to-camera [R | t], the centre is
 * C = -R^T t.  The rules are the library's own.  Neither call takes a scratch.  Every intermediate is float64 and no product is
 * contracted into an FMA.
 *
 * cotr_average_rotations: DEVICE pointers: R_rel [E][9] float64 row-major, edges [E][2] int32 = (i, j): x_j ~ R_ij x_i + t_ij, so
 *   R_j = R_ij R_i (what cotr_recover_pose returns with i as view 1); weights [E] float64 or NULL (every edge 1); found [E] int32
 *   or NULL.  Repeated and reversed pairs are allowed and each counts.
 *   Dead edge: an index outside [0, n), i = j, found[e] = 0, a weight that is <= 0 or not finite, a matrix entry that is not
 *   finite.  The others are live.
 *   Start: R_root = I, located in round 0.  In round k = 1 .. n - 1 every view not yet located takes R_j = R_ij R_i (through an
 *   edge (j, i): R_j = R_ji^T R_i) from the live edge of largest weight that joins it to a view located before round k, the
 *   lowest edge index among equals.  A view never reached is not located: its rotation is NaN and its edges take no part.
 *   Step k = 0 .. iters - 1, sigma_k = max(sigma_end, sigma0 2^-k): per live edge between located views r_e = log(R_j^T (R_ij R_i))
 *   and w_e = weight_e / (1 + (|r_e| / sigma_k)^2)^2; log(M): a = the vector of (M - M^T) / 2, s = |a|, c = (trace - 1) / 2,
 *   theta = atan2(s, c), r = a theta / s where s > 1e-8, r = a below that with c > 0, else theta times the unit vector along the
 *   column of M + I with the largest diagonal entry.  The step minimises sum w_e |r_e + x_i - x_j|^2 over the located views
 *   other than the root (the root's x is 0) as ONE system of 3 F <= 93 unknowns, F the located views other than the root in
 *   index order: the weighted graph Laplacian (x) I_3, right-hand side -w_e r_e at i and +w_e r_e at j, each view's sums over its
 *   edges in ascending edge index by one thread; Cholesky by columns.  A pivot that is not finite, <= 0 or <= 1e-9 times its
 *   diagonal entry before the elimination (the relative rule of cotr_icp_multiview) stops the chain: stop reason 2, the
 *   rotations stay.  No located view other than the root: stop reason 1.  Then R_v <- R_v exp([x_v]x) by the Rodrigues rule of
 *   cotr_ransac_pnp.
 *   -> R_out [n][9] float64; edge_out [E][4] float64 = {|r_e| at the output (NaN for an edge that takes no part), w_e of the last
 *   step taken (weight_e when none was, 0 for an edge that takes no part), live, inlier: takes part and |r_e| <= edge_thresh};
 *   view_info_out [n][4] int32 = {located, the round it was located in (-1: never), its live edges, its inlier edges};
 *   info_out [8] int32 = {ok: at least two views located and no pivot refused, located views, live edges, inlier edges, steps
 *   taken, stop reason (0 ran all, 1, 2), 0, 0}; stats_out [2] float64 = {sum w_e |r_e|^2 at the output in edge order, the
 *   largest |r_e| over the inliers}.
 *   2 <= n <= 32, 1 <= E <= n (n - 1), 0 <= root < n, 0 <= iters <= 64, 0 < sigma_end <= sigma0 finite, edge_thresh > 0 finite
 *   (radians).  One launch of one workgroup whatever the data; all state in LDS.
 *
 * cotr_solve_positions: DEVICE pointers: points [V][n][2] float64 (16-byte aligned), visible [V][n] uint8 or NULL, cams [V][5] as
 *   for cotr_triangulate_views, with its pixel rounding and its ray; R [V][9] float64 (e.g. R_out above); located [V] int32 or
 *   NULL (every view); found int32 [1] or NULL.  A view is valid when its camera row is finite with focal lengths that are not
 *   0, its rotation is finite and its entry of located is not 0.  found[0] = 0, or a root that is not valid: every output is 0.
 *   Ray of observation (v, p): d = R_v^T r / |r|, r the ray of cotr_triangulate_views with R_v.  P = I - d d^T.  Model:
 *   P_vp (X_p - C_v) = 0 for every observation of the set, C_root = 0.
 *   The set of round 1: the observations of the valid views that visible admits and whose rounded coordinates are finite; of a
 *   later round: those of them with depth d . (X_p - C_v) > 0 and atan2(|d x (X_p - C_v)|, depth) <= threshold / sqrt(|fx fy|)
 *   at the previous round's X and C (a view not placed then has no centre and stays out).  A view other than the root with
 *   fewer than min_obs observations so counted leaves the set for the round; then a point with fewer than two views, or whose
 *   A_p = sum_v P_vp (views ascending, one thread) has a determinant that is 0 or not finite (the cofactor rule of
 *   cotr_triangulate_views), leaves it too.
 *   Reduced matrix over the placed views other than the root, in index order: S_vw = [v = w] sum_p P_vp - sum_p P_vp A_p^-1 P_wp,
 *   summed per thread, wavefront and chunk of 2048 points in the fixed order of cotr_bundle_adjust.  mu = 1e-12 times the largest
 *   diagonal entry of S; Cholesky of S + mu I (a pivot <= 0 or not finite: the call fails, ok = 0, C, the translations and X
 *   are NaN, the later rounds do nothing).  power_iters steps of inverse iteration x <- y / |y|, y = (S + mu I)^-1 x, from
 *   x_i = 1 + (i mod 3) / 2 + (i div 3) / 8, normalised; lambda0 = 1 / (x . y) - mu at the last step.  A second run from
 *   x_i = 1 + ((5 i) mod 7) / 4 - (i div 3) / 16, the start and every y deflated by the first run's vector, gives lambda1.
 *   X_p = A_p^-1 sum_v P_vp C_v.  Sign: turned round when more observations of the set have negative depth than positive.
 *   Scale: the root-mean-square distance of the other placed centres from the root is 1.
 *   -> C_out [V][3] float64 (NaN for a view not placed), poses_out [V][12] = [R | -R C], X_out [n][3] (NaN for a point that
 *   left the set), used_out [V][n] uint8 (the last round's set), stats_out [4] float64 = {lambda0, lambda1, the cost
 *   sum |P (X - C)|^2 of the last set at the output scale, 0}, info_out [8] int32 = {ok, observations in the last set, views
 *   placed (the root included), valid views dropped, points solved, positive depths, negative depths, rounds run}.
 *   The caller judges ambiguity from lambda1: tracks that do not tie a group of views to the root leave that group free to
 *   shift and scale, which shows as lambda1 ~ lambda0 ~ 0 while ok stays 1.  With V = 2 the solution is the baseline direction.
 *   work_out: DEVICE, at least cotr_solve_positions_work_doubles(V, n) float64, 8-byte aligned, an output whose content is the
 *   call's own: the view rows, the state and counters, the raw centres, A_p^-1 [n][6], the cost per 256 points and the block
 *   sums [V (V + 1) / 2][chunks][16].
 *   2 <= V <= 32, 1 <= n <= 2^20, 0 <= root < V, threshold > 0 finite (pixels), 1 <= rounds <= 8, min_obs >= 1,
 *   1 <= power_iters <= 64.  1 + 6 rounds launches whatever the data.
 * Both: stream-ordered, no host waits and no allocation (capturable); integer atomics only, every floating-point sum in a fixed
 * order: the same input gives the same bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in
 * cotr_raster_last_error(). */
int cotr_average_rotations(const double* R_rel, const int32_t* edges, const double* weights, const int32_t* found, int n, int E,
                           int root, int iters, double sigma0, double sigma_end, double edge_thresh, double* R_out,
                           double* edge_out, int32_t* view_info_out, int32_t* info_out, double* stats_out, cotr_stream stream);
int cotr_solve_positions_work_doubles(int V, int n, size_t* doubles);
int cotr_solve_positions(const double* points, const uint8_t* visible, const double* cams, const double* R,
                         const int32_t* located, int V, int n, const int32_t* found, int root, double threshold, int rounds,
                         int min_obs, int power_iters, double* C_out, double* poses_out, double* X_out, uint8_t* used_out,
                         double* stats_out, int32_t* info_out, double* work_out, cotr_stream stream);

/* ---- multi-view tracks from pairwise keypoint matches (cotr_amd/csrc/tracks.hip; rules in DESIGN.md 3h-21) ----
 * The step between the keypoint index pairs of cotr_nearest_mutual and the N-view calls above, which consume tracks: points
 * [V][n][2] and visible [V][n].  All arithmetic is on integers.  The call takes no scratch.
 *
 * cotr_build_tracks: a node is one keypoint of one view; nodes are numbered view by view: node g belongs to view v when
 *   offsets[v] <= g < offsets[v + 1], K = offsets[V].  DEVICE pointers: offsets [V + 1] int32, non-decreasing from 0 (a view
 *   may have no keypoints); matches [M][2] int32, global node ids; keep [M] uint8 or NULL (all ones; e.g. the two-view inlier
 *   masks); keypoints [K][2] float64 or NULL.
 *   Dead match: an id outside [0, K), both ids in one view (a = b included), or keep[m] = 0.  Repeated and reversed matches are
 *   allowed.  A node with at least one live match is touched; the others belong to nothing.
 *   Component: a connected component of the live matches over the touched nodes; its label is its smallest node id.
 *   Conflict: view v is in conflict in a component that holds two different nodes of v.  conflict = 0 ("drop"): a component
 *   with any view in conflict is not a track.  conflict = 1 ("views"): the views in conflict are taken out of it and the rest
 *   goes on.
 *   Track: a component that survives the conflict rule and has at least min_views views left.  Tracks are numbered in
 *   ascending label; track t < cap is written, tracks from cap on are only counted.
 *   -> track_of_node [K] int32: the track of each observation written (-1 for an untouched node, a node of a view in conflict,
 *   a node of a component that is no track, or a track >= cap); node_out [V][cap] int32: the keypoint index local to its view,
 *   or -1; visible_out [V][cap] uint8; points_out [V][cap][2] float64, NULL exactly when keypoints is NULL: the keypoint, or
 *   NaN where not visible; info_out [8] int32 = {tracks found (the cap not applied), tracks written, observations written,
 *   live matches, components, components with a view in conflict, components that survive the conflict rule but keep fewer
 *   than min_views views, views of the longest written track}.  Under conflict = 1 a component can count in both [5] and [6].
 *   Columns info[1] .. cap - 1 are written as empty (-1, 0, NaN), so a later call can take all cap columns at a fixed shape
 *   with no host wait.  With cap = 0 the three [V][cap] outputs are not touched and may be NULL, as may matches with M = 0.
 *   offsets cannot be checked on the host.  The view of node g is found by a binary search over entries 1 .. V - 1 that stays
 *   in [0, V) whatever the table holds: it is the largest v with offsets[v] <= g when the table is non-decreasing, and some
 *   view in range, the same on every call, when it is not.  Every rule above then holds with that assignment, every write
 *   stays inside the outputs, and node_out = g - offsets[view] is only meaningful for a table that is non-decreasing from 0.
 *   work_out: DEVICE, at least cotr_build_tracks_work_ints(K, M) int32, 4-byte aligned, an output whose content is the call's
 *   own, each region on its own 256 bytes from the start: the parents [K] (at the end the position of a root's track within
 *   its 256 nodes, or -1), the labels [K], the seen and the conflict masks [K] each, the touched flags [K] uint8, the block
 *   sums [ceil(K / 256)], 8 counters.
 *   2 <= V <= 32, 1 <= K <= 2^21, 0 <= M <= 2^24, 2 <= min_views <= V, 0 <= cap <= K / 2.  M = 0 is legal and yields no tracks.
 *   int32 pointers 4-byte, float64 pointers 8-byte aligned.
 * Stream-ordered, 7 launches whatever the data, no cooperative launch, no host waits and no allocation (capturable); integer
 * atomics only: the same input gives the same bits, whatever the order of the matches.  Bad arguments are checked before any
 * HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_build_tracks_work_ints(int K, int M, size_t* ints);
int cotr_build_tracks(const int32_t* offsets, const int32_t* matches, const uint8_t* keep, const double* keypoints, int V, int K,
                      int M, int min_views, int conflict, int cap, int32_t* track_of_node, int32_t* node_out,
                      uint8_t* visible_out, double* points_out, int32_t* info_out, int32_t* work_out, cotr_stream stream);

/* ---- keypoints of 8-bit grey images (cotr_amd/csrc/keypoints.hip; rules in DESIGN.md 3h-22) ----
 * The first link of the chain: what cotr_nearest_mutual, cotr_build_tracks and the engine's queries take as keypoints.  On an
 * 8-bit image the structure tensor is integer arithmetic and the selection a total order on (key, pixel index), so the result
 * is defined exactly, whatever order the workgroups run in.
 *
 * cotr_detect_keypoints: DEVICE pointers: images [n][H][W] uint8, grey; mask [n][H][W] uint8 or NULL (all ones).
 *   Gradients: Ix, Iy are the 3x3 Sobel responses with weights 1-2-1 (right minus left, below minus above), integers;
 *   a, b, c the sums of Ix Ix, Ix Iy, Iy Iy over the (2r+1)^2 box around the pixel, r = window_radius, in int64.  For r <= 4,
 *   a, c <= 81 * 1020^2, so every integer below fits int64.
 *   Key of a pixel, an int64 that orders pixels.  score = 1 (harris): key = 64 (a c - b b) - 3 (a + c)^2 (k = 3/64), and the
 *   score is S = (double)key.  score = 0 (min_eig): S = (double)(a + c) - sqrt((double)((a - c)^2 + 4 b b)), twice the smaller
 *   eigenvalue, every operation IEEE round-to-nearest, and key = the bit pattern of S, which keeps the order of S > 0.  In both
 *   S <= 0 gives key 0.  Key 0 also where the pixel is closer than max(border, r + 1) to an image edge (no support ever
 *   leaves the image) and where mask is 0.  The score map of the sub-pixel step is S where key > 0, and 0 elsewhere.
 *   Candidate: a pixel p with key(p) > 0, S(p) >= min_score, and for every other pixel q of the (2R+1)^2 window around it,
 *   R = nms_radius, pixels outside the image taken as key 0: key(q) < key(p), or key(q) == key(p) and q has the larger raster
 *   index y W + x.  No two candidates lie within Chebyshev distance R of each other, so an image has at most
 *   cap = ceil(H / (R+1)) * ceil(W / (R+1)) of them.
 *   Selection: Smax = the largest S among the image's candidates; a candidate survives when S >= quality * Smax (one double
 *   multiply); survivors are ordered by key descending, then raster index ascending; the first K = max_keypoints are written
 *   in that order, and rows from their count on as NaN / NaN / -1, so a later call can take all K rows at a fixed shape with
 *   no host wait.
 *   Sub-pixel position, per axis, from the score map at the pixel (S_0) and its two neighbours (S_m before, S_p behind):
 *   den = (S_m - S_0) + (S_p - S_0); off = den < 0 ? 0.5 * (S_m - S_p) / den : 0, clamped to [-0.5, 0.5];
 *   xy = (x + off_x, y + off_y).  Integer pixel indices are pixel coordinates, as for the engine's queries and cv2.
 *   -> xy_out [n][K][2] float64; score_out [n][K] float64 (S); pixel_out [n][K] int32 (the raster index); info_out [n][4]
 *   int32 = {candidates, survivors of the quality test, keypoints written, 0}.
 *   work_out: DEVICE, at least cotr_detect_keypoints_work_bytes(n, H, W, nms_radius) bytes, 8-byte aligned, an output whose
 *   content is the call's own and whose candidate order is not defined, each region on its own 256 bytes from the start:
 *   the candidates' keys [n][cap] int64, their positions [n][cap][2] float64, their pixels [n][cap] int32, the candidates
 *   per image [n] int32, the largest key per image [n] uint64.  The list cannot overflow.
 *   1 <= n <= 64, 1 <= window_radius <= 4, 1 <= nms_radius <= 8, border >= 0, 2 max(border, r + 1) + 1 <= H, W,
 *   H, W <= 2^20, n H W <= 2^28, 0 <= quality <= 1, min_score not NaN, 1 <= max_keypoints <= 65536.  float64 pointers 8-byte, int32
 *   pointers 4-byte aligned.
 * Stream-ordered, 3 launches whatever the data, no cooperative launch, no host waits and no allocation (capturable); integer
 * atomics only (the length of the candidate list, a 64-bit maximum of keys, the counts of info): the same input gives the same
 * bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_detect_keypoints_work_bytes(int n, int H, int W, int nms_radius, size_t* bytes);
int cotr_detect_keypoints(const uint8_t* images, const uint8_t* mask, int n, int H, int W, int score, int window_radius,
                          int nms_radius, int border, double quality, double min_score, int max_keypoints, double* xy_out,
                          double* score_out, int32_t* pixel_out, int32_t* info_out, void* work_out, cotr_stream stream);

/* ---- multi-view depth maps: a depth map from correspondence maps, and the cross-check of depth maps (cotr_amd/csrc/mvdepth.hip;
 *      rules in DESIGN.md 3h-16) ----
 * The step between dense correspondences and the TSDF stack: the correspondence maps of a reference view into its posed
 * neighbours become the reference's depth map, and a set of depth maps is checked against each other before it is fused.  The
 * rules are the library's own.  Neither call takes a scratch.  Every intermediate is float64, evaluated as bracketed below, and
 * no product is contracted into an FMA.
 *
 * cotr_corr_depth: V = K + 1 views, view 0 the reference, views 1 .. K its neighbours.  DEVICE pointers: corr [K][H][W][2]
 *   float32, 8-byte aligned: (u, v) = corr[k][y][x], the position in pixels of view k + 1 of what reference pixel (x, y) shows;
 *   valid [K][H][W] uint8 or NULL (every entry counts); cams [V][5] and poses [V][12] float64 as in cotr_triangulate_views
 *   (world-to-camera); found int32 [1] or NULL.
 *   Views: a view is valid, and has the centre c_j = -R^T t, by the rule of cotr_triangulate_views.  When the reference view is
 *   not valid or found[0] is 0, every output is empty: depth 0, views 0, err NaN, every counter 0.
 *   Reference ray of pixel (x, y): (xn, yn) by the rule of cotr_ransac_essential in view 0, r_i = (R_0i xn + R_1i yn) + R_2i, not
 *   normalised; X(s)_i = c_0i + s r_i, and the depth of X(s) in the reference camera is s itself.
 *   Candidate views: neighbour j sees the pixel when it is valid, its entry of valid is not 0 and both its coordinates are
 *   finite.  r_j: its ray, formed the same way from (u, v).  a = r.r, b = r.r_j, e = r_j.r_j, w = c_j - c_0 (every dot product
 *   (p_0 q_0 + p_1 q_1) + p_2 q_2).  j has parallax iff b / sqrt(a e) <= max_cos; its candidate is
 *   s_j = ((r.w) e - b (r_j.w)) / (a e - b b), degenerate when the denominator is 0 or not finite or s_j is not finite or <= 0.
 *   P: the views that see the pixel and have parallax; the others take no part.  No view of P with a candidate that is not
 *   degenerate: the pixel has no candidate.
 *   Vote: the candidates of P that are not degenerate, ascending in j; each counts the views of P in which X(s_j) has depth z > 0
 *   and float(squared reprojection error) <= float(threshold^2), by the projection of cotr_triangulate_views.  A candidate takes
 *   over only with a strictly larger count: the first with the largest count gives s and U, its inlier views.  |U| < min_views:
 *   the pixel has too few views.
 *   Refit: up to refine_iters scalar Gauss-Newton steps on E(s) = sum over U of the squared reprojection errors e_j, ascending
 *   in j.  With q = R_j r (q_i = (R_i0 r_0 + R_i1 r_1) + R_i2 r_2), (xn_j, yn_j, z) the projection of X(s) and (du, dv) its
 *   residual: a_j = (q_0 - xn_j q_2) / z, b_j = (q_1 - yn_j q_2) / z, ju = fx a_j + skew b_j, jv = fy b_j, A += ju ju + jv jv,
 *   g += ju du + jv dv; the proposal is s - g / A.  A step is kept only if A is finite and > 0, the new s is > 0, every view of U
 *   keeps z > 0 and E falls; the first step not kept ends the refit.
 *   Filters: the pixel is dropped by depth unless 0 < s < distance_thresh, and (depth passed) by error unless float(e_j) <=
 *   float(threshold^2) for every view of U at the final s.
 *   -> depth_out [H][W] float32 = float32(s), 0 where there is none; views_out [H][W] uint8 = |U|, 0 where there is no depth;
 *   err_out [H][W] float32 = float32(E / |U|), NaN where there is no depth; info_out [8] int32 = {found, pixels with a depth,
 *   pixels with too few views, without a candidate, dropped by depth, dropped by error, 0, steps kept in total}.
 *   2 <= V <= 32, 1 <= H, W and H W <= 2^28, threshold > 0 finite with a squared float32 that is finite and not 0, -1 <= max_cos
 *   <= 1, distance_thresh > 0 finite, 1 <= min_views <= 31, 0 <= refine_iters <= 64.
 *
 * cotr_depth_consistency: depths [n][H][W] float32 DEVICE, 2 <= n <= 32, 1 <= H, W and n H W <= 2^28; Ks HOST [n][9], each as K
 *   in cotr_lift_pixels; c2w [n][16] float64 DEVICE, row-major camera-to-world; found int32 DEVICE [n] or NULL, as in
 *   cotr_tsdf_integrate: a view whose entry is 0 is checked against nothing (its outputs and its row of info_out are 0) and no
 *   view is checked against it; pairs [n][n] uint8 DEVICE or NULL (everything): view i is checked against view j only where
 *   pairs[i][j] is not 0; the diagonal is not read.
 *   Pixel (x, y) of view i is valid when its depth z is finite and > 0.  Its vertex Y = (xn z, yn z, z) by cotr_lift_pixels'
 *   rule at the pixel centre, its world point P_a = ((R_a0 Y_x + R_a1 Y_y) + R_a2 Y_z) + t_a through c2w_i.  For every allowed
 *   j != i, ascending: P in view j, its depth Y_z and its pixel by the expressions of cotr_tsdf_integrate in their order; j is
 *   skipped unless Y_z > 0 and the pixel (rint u, rint v) (ties to even) lies inside the map and holds a valid depth d_j.  That
 *   pixel of j is lifted at d_j through c2w_j and projected into view i the same way (not rounded): (u', v') with depth z'.
 *   j is consistent iff z' > 0, (u' - x)^2 + (v' - y)^2 <= px_thresh^2 and |z' - z| <= rel_thresh z.  j is a violation iff it is
 *   not consistent and d_j > Y_z (1 + rel_thresh): view j sees through the point.  The pixel is kept iff consistent >= min_views
 *   and (max_violations < 0 or violations <= max_violations).
 *   -> depth_out [n][H][W] float32: a kept pixel float32((z + sum z') / (1 + consistent)), summed over the consistent views
 *   ascending, every other pixel 0; count_out [n][H][W] uint8 = consistent (0 at a pixel that is not valid); info_out [n][4]
 *   int32 = {evaluated (found), valid pixels in, pixels kept, pixels with enough consistent views dropped by violations}.
 *   px_thresh > 0 finite with a finite square, 0 < rel_thresh < 1, 0 <= min_views <= 31, -1 <= max_violations <= 31.
 * Both: no output may share a byte with another output or with an input (depth_out is not depths): COTR_ERR_ARG.
 * Stream-ordered, 2 launches each whatever the data (a prologue that sets info_out, then a thread a pixel), no scratch, no host
 * waits and no allocation (capturable); integer atomics only, and only for info_out; no floating-point sum crosses a thread:
 * the same input gives the same bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in
 * cotr_raster_last_error(). */
int cotr_corr_depth(const float* corr, const uint8_t* valid, const double* cams, const double* poses, int V, int H, int W,
                    const int32_t* found, double threshold, double max_cos, double distance_thresh, int min_views,
                    int refine_iters, float* depth_out, uint8_t* views_out, float* err_out, int32_t* info_out,
                    cotr_stream stream);
int cotr_depth_consistency(const float* depths, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                           const uint8_t* pairs, double px_thresh, double rel_thresh, int min_views, int max_violations,
                           float* depth_out, uint8_t* count_out, int32_t* info_out, cotr_stream stream);

/* ---- photometric refinement of a depth map: a plane sweep around the depth each pixel came with (cotr_amd/csrc/photodepth.hip;
 *      rules in DESIGN.md 3h-18) ----
 * The step behind cotr_corr_depth: the depth of a reference pixel is moved to where the patches of the posed neighbour images look
 * most like the reference's.  The rule is the library's own.  No scratch.  Every intermediate is float64, evaluated as bracketed
 * below, and no product is contracted into an FMA.
 *
 * cotr_photo_depth: V = K + 1 views, view 0 the reference, views 1 .. K its neighbours.  DEVICE pointers: grey [V][H][W] uint8, the
 *   views' images, all of one size; depth_in [H][W] float32, the reference's depth (a pixel whose entry is not finite and > 0 has
 *   none); cams [V][5] and poses [V][12] float64 and found int32 [1] or NULL as in cotr_corr_depth.
 *   Views: validity, centre c_0 and the ray r(x, y) of a reference pixel as in cotr_corr_depth.  When the reference view is not
 *   valid or found[0] is 0, every output is empty: depth 0, score NaN, views 0, every counter 0.
 *   Patch of pixel (x, y): the N = (2 R + 1)^2 taps (x + dx, y + dy), dy outer and dx inner, each ascending from -R to R; a_t the
 *   image of view 0 there.  Sa = sum a_t, Saa = sum a_t a_t in that order (every sum below likewise, starting from 0).  A pixel
 *   with a tap outside the image is rim; a pixel with Saa - Sa Sa / N < min_var N is flat (rim is tested first).
 *   Score of a valid neighbour j at the depth s: tap t is the world point X_i = c_0i + s r_i(x + dx, y + dy), whose depth in the
 *   reference camera is s: the patch is fronto-parallel.  (z, u, v): its depth and pixel in view j by the projection of
 *   cotr_triangulate_views (u = (fx xn + skew yn) + cx, v = fy yn + cy).  j scores only if every tap has z > 0, 0 <= u <= W - 1
 *   and 0 <= v <= H - 1.  b_t, the bilinear sample: x0 = max(min(floor u, W - 2), 0), x1 = min(x0 + 1, W - 1), au = u - x0, y0, y1,
 *   av likewise, g the image of view j; b_t = (1 - av) ((1 - au) g[y0][x0] + au g[y0][x1]) + av ((1 - au) g[y1][x0] + au g[y1][x1]).
 *   Sb = sum b_t, Sbb = sum b_t b_t, Sab = sum a_t b_t; j scores only if Sbb - Sb Sb / N >= min_var N, and its score is
 *   (Sab - Sa Sb / N) / sqrt((Saa - Sa Sa / N) (Sbb - Sb Sb / N)).
 *   f(s): the sum of the scores of the scoring neighbours, ascending in j, over their number n; it exists when n >= min_views.
 *   Sweep i = 0 .. sweeps - 1 around the centre c_i (c_0 = depth_in): h_i = rel_step / 2^i; the hypotheses s_k = c_i (1 + k h_i),
 *   k = -steps .. steps.  The winner k* is the k with the largest f that exists; among equal f the smallest |k|, then the
 *   negative one.  d = 0; when |k*| < steps, f- = f(s_(k*-1)) and f+ = f(s_(k*+1)) both exist and den = (f- - 2 f(s_k*)) + f+ < 0:
 *   d = 0.5 (f- - f+) / den, clipped to [-0.5, 0.5].  c_(i+1) = c_i (1 + (k* + d) h_i); a sweep in which no f exists leaves the
 *   centre where it is.
 *   Finish: a pixel with an input depth that is neither rim nor flat is refined iff an f existed in the last sweep, that sweep's
 *   f(s_k*) >= min_score and float32(c_sweeps) lies in (0, distance_thresh): depth_out = float32(c_sweeps), score_out =
 *   float32(f(s_k*)), views_out = n there.  Every other pixel: score NaN, views 0, and depth_out = depth_in when keep_input is 1
 *   and the pixel has an input depth, else 0.
 *   -> depth_out, score_out [H][W] float32, views_out [H][W] uint8, info_out [8] int32 = {found, pixels refined, without an input
 *   depth, rim, flat, without an f in the last sweep, below min_score, dropped by range} (each pixel in the first that applies).
 *   2 <= V <= 32, 1 <= H, W and H W <= 2^28, 1 <= radius <= 4, 1 <= steps <= 16, 1 <= sweeps <= 8, rel_step > 0 finite with
 *   steps rel_step < 1, min_var > 0 finite, -1 <= min_score <= 1, 1 <= min_views <= V - 1, distance_thresh > 0 finite, keep_input
 *   0 or 1.  No output may share a byte with another output or with an input (depth_out is not depth_in): COTR_ERR_ARG.
 * Stream-ordered, 2 launches whatever the data (a prologue that sets info_out, then a thread a pixel that runs every sweep), no
 * scratch, no host waits and no allocation (capturable); integer atomics only, and only for info_out; no floating-point sum
 * crosses a thread: the same input gives the same bits.  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the
 * message in cotr_raster_last_error(). */
int cotr_photo_depth(const uint8_t* grey, const float* depth_in, const double* cams, const double* poses, int V, int H, int W,
                     const int32_t* found, int radius, int steps, int sweeps, double rel_step, double min_var, double min_score,
                     int min_views, double distance_thresh, int keep_input, float* depth_out, float* score_out, uint8_t* views_out,
                     int32_t* info_out, cotr_stream stream);

/* ---- warps of 8-bit images: cv2.remap / cv2.warpPerspective, INTER_LINEAR, BORDER_CONSTANT 0 (cotr_amd/csrc/warp.hip) ----
 * The last host step of demo_single_pair.py:43 (image B warped by triangulate_corr's dense map) and of
 * demo_homography.py:46-49 (a picture pasted through four corners).  Rule in DESIGN.md 3i: OpenCV's 8-bit bilinear remap.
 *
 * cotr_warp_map: src [Hs,Ws,C] uint8, C in {1, 3, 4}; map [Hd,Wd,2] = (x, y) source positions in pixel INDICES (sample
 *   (j, i) is the centre of src[i, j]), float32 (8-byte aligned) or, with map_is_f64 != 0, float64 (16-byte aligned,
 *   rounded to float32 first) -> dst [Hd,Wd,C] uint8.  X = rint(x * 32) (ties to even), ix = X >> 5, fx = X & 31, Y alike;
 *   taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1), weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy; a tap outside
 *   the source reads 0; dst = (sum w p + 512) >> 10.  A non-finite coordinate or one of magnitude >= 2^26 puts all four
 *   taps outside.
 *   cover [Hd,Wd] uint8 (may be NULL) = 1 where a tap with a non-zero weight lies inside the source.
 *   background [Hd,Wd,C] uint8 (may be NULL): an uncovered pixel of dst takes the background's pixel instead of 0.
 * cotr_warp_perspective: the same with the positions from M, a HOST double[9] (row-major 3x3, destination -> source; read
 *   before the call returns): per destination pixel (x, y) in double, W = (m6 x + m7 y) + m8, W = W != 0 ? 32 / W : 0,
 *   X = rint(clamp(((m0 x + m1 y) + m2) W, INT_MIN, INT_MAX)), Y alike, products and sums in this order, not contracted.
 *   W == 0 or a NaN position puts all four taps outside.  M must be finite.
 * All image pointers are DEVICE pointers; 1 <= Hs, Ws, Hd, Wd <= 16384; dst must not overlap src or background.  One launch
 * each, stream-ordered, no host waits, no allocation (capturable).  Bad arguments are checked before any HIP call:
 * COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_warp_map(const uint8_t* src, int Hs, int Ws, int C, const void* map, int map_is_f64, int Hd, int Wd, uint8_t* dst,
                  uint8_t* cover, const uint8_t* background, cotr_stream stream);
int cotr_warp_perspective(const uint8_t* src, int Hs, int Ws, int C, const double* M, int Hd, int Wd, uint8_t* dst,
                          uint8_t* cover, const uint8_t* background, cotr_stream stream);

/* ---- training batches from depth and camera poses (cotr_amd/csrc/reproject.hip, cotr_amd/data.py) ------------------------
 * The geometry of COTR/datasets/cotr_dataset.py (get_corrs) and COTR/projector/pcd_projector.py on the device.  Rules in DESIGN.md 3j.
 *
 * cotr_depth_corrs: n items, each described by one row of three DEVICE tables (so items may differ in size):
 *   ptrs   [n][3] uint64: from_depth [Hf,Wf] float32, to_depth [Ht,Wt] float32, subset (int32 source pixel indices y * Wf + x,
 *          or 0: every pixel in row-major order) - DEVICE addresses
 *   shapes [n][5] int32:  Hf, Wf, Ht, Wt, n_src (the subset's length, or Hf * Wf)
 *   cams   [n][37] float64: Kinv_from 3x3 | c2w_from 4x4 | P_to = K_to . w2c_to[0:3] 3x4, row-major
 *   Per source pixel (x, y), z = from_depth[y, x], in double, products and sums in this order, not contracted:
 *     c = (Kinv . (x, y, 1)) z with a row (k0 x + k1 y) + k2; reject unless z > 0 and c.z > 0
 *     w = c2w . (c, 1) with a row ((m0 c.x + m1 c.y) + m2 c.z) + m3; reject if w.w == 0, then w.xyz /= w.w
 *     p = P_to . (w.xyz, 1), rows alike; reject unless p.z > 0
 *     u = p.x / p.z, v = p.y / p.z; reject unless 0 <= u < Wt - 1 and 0 <= v < Ht - 1
 *     keep iff |to_depth[floor(v), floor(u)] - p.z| < 0.5
 *   -> counts [n] int32 (DEVICE) and rows [n][cap][4] float64 (DEVICE, 16-byte aligned) = (x, y, u, v) of the kept pixels in
 *   SOURCE order (row-major, or the subset's order; a subset index outside the map is rejected).  Rows beyond cap are counted
 *   but not written; rows past the count are left alone.  max_src: a host upper bound of every n_src (it sizes the grid; an
 *   item's n_src is clamped to it).  The compaction is a scan (wave ballots, block totals, their scan, scatter): two runs
 *   return the same bytes.
 * cotr_depth_valid: the same compaction with the predicate from_depth > 0 (to_depth and cams are not read) ->
 *   indices [n][cap] int32 (4-byte aligned: written one index at a time) = y * Wf + x of the valid pixels in source order,
 *   counts [n].
 *   ptrs and cams 8-byte, shapes and counts 4-byte aligned.
 *   scratch for both: DEVICE, 16-byte aligned, at least cotr_depth_corrs_scratch(n, max_src) bytes (0 for arguments out of range).
 * cotr_crop_depth_nearest: for each of n items crop the box boxes[i] = (x, y, size) (int32 [n][3], DEVICE, inside the map) of the
 *   float32 depth map srcs[i] (uint64 [n] DEVICE addresses) of shapes[i] = (H, W) (int32 [n][2], DEVICE) and resize it to
 *   out x out -> dst [n][out][out] float32, bit-identical to PIL.Image.fromarray(depth[y:y+s, x:x+s]).resize((out, out), NEAREST)
 *   in mode 'F': source column of output column j is int(xo_j), xo_0 = a / 2, xo_(j+1) = xo_j + a, a = size / out in double (the
 *   accumulated sum of Pillow's ImagingScaleAffine), rows alike.  One launch.  1 <= out <= 4096.
 * 0 <= n <= 65535 (n == 0 does nothing), 1 <= max_src <= 2^28, n * cap <= 2^31.  Stream-ordered, no host waits, no allocation
 * (capturable).  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
size_t cotr_depth_corrs_scratch(int n, int max_src);
int cotr_depth_corrs(const uint64_t* ptrs, const int32_t* shapes, const double* cams, int n, int max_src, double* rows, int cap,
                     int32_t* counts, void* scratch, size_t scratch_bytes, cotr_stream stream);
int cotr_depth_valid(const uint64_t* ptrs, const int32_t* shapes, int n, int max_src, int32_t* indices, int cap, int32_t* counts,
                     void* scratch, size_t scratch_bytes, cotr_stream stream);
int cotr_crop_depth_nearest(const uint64_t* srcs, const int32_t* shapes, const int32_t* boxes, int n, float* dst, int out,
                            cotr_stream stream);

/* ---- rotation augmentation of captures: cv2.warpAffine about the centre (cotr_amd/csrc/rotate.hip, cotr_amd/data.py) -------
 * capture.rotate_capture of the reference (COTR/cameras/capture.py:128-132, 407-418) on the device: the image through
 * warpAffine(INTER_LINEAR), the depth through warpAffine(INTER_NEAREST), BORDER_CONSTANT 0.  Rule in DESIGN.md 3l.
 *
 * cotr_rotate_captures: n items, each described by one row of three DEVICE tables (so items may differ in size):
 *   ptrs   [n][4] uint64: image src [H,W,3] uint8, image dst [H,W,3] uint8, depth src [H,W] float32, depth dst [H,W] float32 -
 *          DEVICE addresses; an image or a depth half with a 0 address is absent and skipped
 *   shapes [n][2] int32:  H, W (an item with a side outside [1, 16384] is skipped)
 *   mats   [n][6] float64: m0..m5, destination -> source (what warpAffine holds after inverting the 2 x 3 matrix)
 *   Per destination pixel (x, y), in double, products and sums in this order, not contracted; rint = ties to even, saturated
 *   to int32:  ad = rint((m0 x) 1024), bd = rint((m3 x) 1024), X0 = rint(((m1 y) + m2) 1024), Y0 = rint(((m4 y) + m5) 1024)
 *     image: X = (X0 + 16 + ad) >> 5, Y = (Y0 + 16 + bd) >> 5 (arithmetic shifts): the source position in 1/32 px, then the
 *            8-bit bilinear of cotr_warp_map (ix = X >> 5, fx = X & 31, four taps, a tap outside reads 0, (sum + 512) >> 10)
 *     depth: X = (X0 + 512 + ad) >> 10, Y = (Y0 + 512 + bd) >> 10; dst = src[Y][X] if inside, else 0.0f; the 32 bits are
 *            copied (a NaN payload, -0.0 or a denormal arrives unchanged)
 *   The int32 sums do not overflow for a rotation about the centre of an item with sides <= 16384 (every term is below 2^26);
 *   for any other matrix they wrap, and every tap stays bounds-checked.
 *   max_h, max_w: host upper bounds of every H and W (they size the grid; pixels of an item beyond them are not written).
 *   A dst must not overlap any src of the call: the tables live on the device, so this is NOT checked here; the caller
 *   allocates the destinations (cotr_amd.data.rotate_captures does).
 * 1 <= n <= 65535, 1 <= max_h, max_w <= 16384; ptrs and mats 8-byte aligned.  One launch for the whole batch, images and depths
 * together; stream-ordered, no host waits, no allocation (capturable).  Bad arguments are checked before any HIP call:
 * COTR_ERR_ARG, with the message in cotr_raster_last_error(). */
int cotr_rotate_captures(const uint64_t* ptrs, const int32_t* shapes, const double* mats, int n, int max_h, int max_w,
                         cotr_stream stream);

/* ---- overlap of the captures of a scene (cotr_amd/csrc/overlap.hip, cotr_amd/scene.py) ------------------------------------
 * The per-scene "distance matrix" of scripts/prepare_nn_distance_mat.py (distance_between_two_caps) on the device: the world
 * points of capture d projected into capture q, and the intersection over union of the two depth supports.  Rule in DESIGN.md 3k.
 *
 * Captures are described by DEVICE tables, so the captures of one call may differ in size:
 *   caps   [n][2] uint64: depth [H,W] float32, xyz [H*W][3] float32 (the capture's world points; 0 where none are needed) -
 *          DEVICE addresses
 *   shapes [n][2] int32: H, W
 * cotr_world_points: cams [n][25] float64 = Kinv 3x3 | c2w 4x4, row-major.  Per pixel (x, y) in row-major order,
 *   z = depth[y, x], in double, products and sums in this order, not contracted:
 *     c = (Kinv . (x, y, 1)) z with a row (k0 x + k1 y) + k2; invalid unless z > 0 and c.z > 0
 *     w = c2w . (c, 1) with a row ((m0 c.x + m1 c.y) + m2 c.z) + m3; invalid if w.w == 0, then w.xyz /= w.w
 *   -> xyz[y W + x] = w.xyz rounded to float32, or three NaNs for an invalid pixel.  One launch.
 * cotr_overlap_pairs: proj [n_caps][12] float64 = P = K . w2c[0:3] of every capture, pairs [n_pairs][2] int32 = (q, d) capture
 *   indices (DEVICE).  Per pair, every world point X of d (float32, widened): p = P_q . (X, 1) with rows as above; kept iff
 *   p.z > 0 and, with u = p.x / p.z and v = p.y / p.z, 0 <= u < Wq - 1 and 0 <= v < Hq - 1; it lands on the canvas pixel
 *   (clip(rint(v), 0, Hq - 1), clip(rint(u), 0, Wq - 1)), ties to even.  canvas = p.z of the kept point with the LARGEST source
 *   index y Wd + x landing there (no depth test: the last writer in source order), 0 where none lands.  With qm = depth_q > 0
 *   and rm = canvas > 0: union = #(qm | rm), good = #(qm & rm & |depth_q - canvas| < 1.0)
 *   -> counts [n_pairs][2] int32 = (good, union) and ratio [n_pairs] float32 = float(good / union), 0 when union == 0 (DEVICE).
 *   A pair with an index outside [0, n_caps) scores (0, 0).  Integer atomics only: two runs return the same bytes.
 *   max_px: a host upper bound of every capture's H * W (it sizes the grid and the canvases; a larger capture counts as empty).
 *   scratch: DEVICE, 16-byte aligned, cotr_overlap_scratch(pairs_in_flight, max_px) bytes = pairs_in_flight canvases of max_px
 *   uint32 (each rounded up to 16 bytes); 0 for arguments out of range.  The pairs are processed in tiles of as many canvases
 *   as scratch_bytes holds (at least one): a memset and two launches per tile, one more launch for the ratios.
 * 0 <= n <= 65535, 1 <= n_caps <= 65535, 0 <= n_pairs <= 2^24, 1 <= max_px <= 2^28, 1 <= pairs_in_flight <= 65535.  Stream-ordered,
 * no host waits, no allocation (capturable).  Bad arguments are checked before any HIP call: COTR_ERR_ARG, with the message in
 * cotr_raster_last_error(). */
int cotr_world_points(const uint64_t* caps, const int32_t* shapes, const double* cams, int n, int max_px, cotr_stream stream);
size_t cotr_overlap_scratch(int pairs_in_flight, int max_px);
int cotr_overlap_pairs(const uint64_t* caps, const int32_t* shapes, const double* proj, int n_caps, const int32_t* pairs, int n_pairs,
                       int max_px, float* ratio, int32_t* counts, void* scratch, size_t scratch_bytes, cotr_stream stream);

/* ---- tuning knobs -------------------------------------------------------------------------------------------
 * Named integer switches that choose between launch schedules / kernel variants with the SAME results (bit-identical unless a
 * knob's line says otherwise).  They are not part of the drop-in boundary: a binding never needs them.  ONE SET PER HANDLE:
 * cotr_set_knob(h, ...) affects only that handle's cotr_encode / cotr_decode / cotr_forward / cotr_backbone calls (two handles, or
 * two threads, can differ); a new handle starts from the shipped defaults.  h == NULL addresses the process-wide set read by the
 * handle-less op-level entry points below (cotr_op_*, cotr_bench_*, cotr_train_*: tests and tools).  count / name enumerate the
 * knobs, get returns the current and the shipped default value, reset puts every knob of that set back to its default; a value
 * outside a knob's range is refused with COTR_ERR_ARG.
 *
 *   encode_chunk               pairs per backbone / encoder pass inside cotr_encode (1..128, default 64; 64 is +2-3 % over 32 from 64
 *                              pairs up, 128 is -20 %).  Scratch of a pass is ~66 MB per pair: set BEFORE sizing a caller-supplied
 *                              workspace (cotr_scratch_bytes uses the handle's value)
 *   attention_fusion_max_rows  up to this many rows (default 4096; 0 = never) the attention kernel also does the output projection
 *                              (per-head partials summed + bias + residual + LayerNorm by one ln_reduce launch) and, in the
 *                              decoder, the q projection of its own queries - above 1024 rows only where its grid of 32-row tiles x 8
 *                              heads fills whole rounds of the CUs to >= 90 % (round 6)
 *   ffn_fusion_max_rows        the fused FFN block (ffn.hip) for at most this many rows (default 4096; 0 = never; above 1024 rows
 *                              under the same fill rule), with at most
 *   ffn_fused_max_chunks       hidden-unit chunks = partial output slabs per row tile (2, 4, 8 or 16; default 16)
 *   ks3                        1 (default): K-deep small-M GEMMs the table gives to the two-stage LDS-DMA k-split run its three-stage form
 *   dual_conv                  1 (default): downsample + conv1 of a ResNet stage's entry block as one launch at few pairs
 *   fused_stem                 1 (default): conv1 + bn1 + relu + maxpool as one launch (stem_pool.hip)
 *   xcd_mapping                workgroup -> XCD mapping, a bit field (default 1): bits 0-1 GEMM / conv tiles (0 = column tiles over the
 *                              8 XCDs, 2 = row tiles, 1 = per launch by operand size); bit 2 fused FFN: hidden-unit chunks over XCDs;
 *                              bit 3 attention: heads over XCDs; bit 4 fused FFN: plain instead of write-through partial stores;
 *                              bit 5 att_rows: the plain (tile, pair) grid also where the pairs are a multiple of 8 (default there: all tiles of a
 *                              pair on ONE XCD - round 6: fabric traffic of the kernel / 2.5-3.7, its time -0 ... -3 %)
 *   attention_fused_splits     key splits of the fused attention: 0 (default = 4), 4, 8, 48 / 84 (encoder / decoder separately)
 *   conv_patch                 1 (default): layer3's 3x3 convolutions at few pairs load their input patch once
 *   pos_table_min_rows         token rows from which the encoder in-projections take pos . W^T from tables built at cotr_load_weights
 *                              (default 8192; >= 2^30 also turns the K/V projection's table off; +1 fp32 addition per output)
 *   attention_wide_min_rows    query rows of a launch from which the 64-query / resident-K/V attention kernels are used (default 4096)
 *   attention_wide_occupancy   wavefronts per SIMD of the 64-query kernel: 3 (default) or 2
 *   attention_splits           key splits of the plain attention kernel: 0 (automatic), 1, 2, 4, 8, 16
 *   attention_resident         1 (default): K_h / V_h resident in LDS for many rows (attention_res_kernel)
 *   conv1x1_dense              1 (default): a 1x1 stride-1 convolution is launched as the dense product of its pixel rows
 *   ws_flags                   wave-specialised large tiles (configurations 40 / 41): bit 0 priority for the MFMA wavefronts' loop,
 *                              bit 1 (default) for the loaders
 *   bottleneck_max_pairs       layer1's bottlenecks as ONE launch each (bottleneck.hip) up to this many pairs per pass (default 5)
 *   train_attention_form       training attention backward: 0 (default) = by shape, 1-3 = force the first / second / one-pass form
 *   att_rows_min_rows, ffn_rows_min_rows   query rows / rows from which the attention sub-layer / the FFN block run as ONE launch
 *                              (att_rows.hip / ffn_rows.hip; default 8192), and
 *   rows_min_fill              the least fill, in percent, of the last round of their 64-row tiles over the CUs (default 75)
 *   conv23_min_pairs, conv23m_min_pairs, expand_min_rows   layer1 / layer2 conv2 -> conv3 and layer1.0's downsample + conv1 as one
 *                              launch from this many pairs per pass / rows (defaults 5 / 16 / 65536; conv23 above bottleneck_max_pairs only;
 *                              conv23m not where its single round fills the CUs unevenly: 17 ... 27 pairs on 256 CUs)
 *   batch_split                1 (default): a batch is walked in the passes the measured time-against-pairs staircase prefers - encode
 *                              passes from a measured table (csrc/enc_split.inc, tools/batch_cost.py: 17 pairs = 16 + 1, 33 = 32 + 1),
 *                              decode passes where a prefix of the pairs fills the one-launch rows kernels and the whole does not;
 *                              0: passes of encode_chunk pairs / 32768 query rows only (cotr_batch_chunks reports the passes)
 *   side_stream                cotr_forward with few rows (B * Q <= 8192, one encode pass and one decode pass; otherwise off for that
 *                              call): bit 0 the query encoding, bit 1 the K/V projections of decoder layers 1-5 (with the pos table
 *                              only) run on a second stream owned by the handle, beside the chain; joined before the call returns
 *                              (default 0: measured, profiles/r6_ab_side_stream_*.txt)
 * libcotr_hip_exp.so (the experimental build, -DCOTR_EXPERIMENTAL) adds the knobs of the measured dead ends, all off by default:
 *   head_fusion_max_rows, ffn_preln, ffn_tail, coop_tail, coop_tail_spin, gemm_ln_min_rows, l2_warm  (cotr_amd/csrc/experimental/experimental.h)
 * and the RESEARCH path of docs/LABNOTES.md 3e (not a dead end; off by default, results as close to fp64 as the fp32 path but not its bits):
 *   split_f16                  0 (default) = off; 1 = the backbone + input_proj of a pass on packed split-f16 tensors (three f16 MFMAs per
 *                              fp32 product); 2 = also the projections / FFN blocks / corr_embed of the many-row (>= 8192 rows) transformer
 *                              path; 3 = also attention in both stacks.  |activations| must stay below 65504
 *   split_f16_min_pairs        the backbone pass takes that path only from this many pairs per pass (default 8) */
int cotr_knob_count(void);
const char* cotr_knob_name(int i);
int cotr_get_knob(cotr_handle h, const char* name, int* value, int* default_value);
int cotr_set_knob(cotr_handle h, const char* name, int value);
/* COTR_OK if cotr_set_knob would accept (name, value), COTR_ERR_ARG otherwise; changes no knob set */
int cotr_check_knob(const char* name, int value);
int cotr_reset_knobs(cotr_handle h);
/* 1 in libcotr_hip_exp.so, 0 in the product library */
int cotr_is_experimental(void);

/* ---- GEMM configuration tuning (tools/tune_gemm.py) and per-config tests ------------------- */
int cotr_gemm_num_configs(void);
/* one layer1 bottleneck from unpacked device weights (tests): x [B][64][128][cin] -> y [B][64][128][256]; cin = 64 with the
 * downsample branch (wd != NULL) or 256 without; w1 [64][cin], w2 [64][3][3][64], w3 [256][64], wd [256][64]; s* / b* FrozenBN
 * scale / bias per output channel */
int cotr_op_bottleneck(const float* x, float* y, int B, int cin, const float* w1, const float* w2, const float* w3, const float* wd,
                       const float* s1, const float* b1, const float* s2, const float* b2, const float* s3, const float* b3,
                       const float* sd, const float* bd, cotr_stream stream);
/* microseconds per launch of one shape under config `cfg` (-1: the library's own choice), measured
 * with HIP events around a captured graph of `iters` launches on a private stream */
int cotr_bench_linear(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int cfg,
                      int iters, float* us);
int cotr_bench_conv(const float* x, const float* w, const float* scale, const float* bias, float* y, int B, int Hin,
                    int Win, int Cin, int Cout, int ksize, int stride, int cfg, int iters, float* us);
int cotr_op_linear_cfg(const float* x, const float* w, const float* bias, const float* residual, int relu, float* y,
                       int M, int N, int K, int cfg, cotr_stream stream);
int cotr_op_conv_cfg(const float* x, const float* w, const float* scale, const float* bias, const float* residual,
                     int relu, float* y, int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int cfg,
                     cotr_stream stream);

/* phase timestamps of the fused FFN launches that follow into `times` (device, [workgroups][8] uint64, 100 MHz wall clock); NULL = off */
int cotr_debug_ffn_times(unsigned long long* times);
/* the same for the fused attention launches (cotr_op_attention_fused / the forward's small-row path) */
int cotr_debug_attention_times(unsigned long long* times);
/* the launch configuration the library picks for this convolution (tools) */
int cotr_gemm_pick_conv(int B, int Hin, int Win, int Cin, int Cout, int ksize, int stride);
/* the launch configuration the library picks for the dense product [M,K] x [N,K]^T with lda = K, ldc = ldr = N and aligned pointers;
 * flags bit 0: the x + pos prologue is present, bit 1: the residual is a row-periodic table.  Makes no HIP call (tests, tools) */
int cotr_gemm_pick_linear(int M, int N, int K, int flags);
/* workgroup tile (rows, columns) of launch configuration `cfg` and whether it has a dual-launch form (any pointer may be NULL);
 * COTR_ERR_ARG outside [0, cotr_gemm_num_configs()).  An index the library has no kernel for reports 0 x 0.  Makes no HIP call */
int cotr_gemm_config_info(int cfg, int* bm, int* bn, int* has_dual);
/* one convolution launch whose k-split kernel writes phase timestamps (100 MHz wall clock) of every workgroup to `times`
 * (device memory, [workgroups][8] uint64; slots 0..4 = entry, loads issued, first data usable, K loop done, stored) */
int cotr_debug_conv_times(const float* x, const float* w, const float* scale, const float* bias, float* y, int B, int Hin, int Win,
                          int Cin, int Cout, int ksize, int stride, int cfg, unsigned long long* times, cotr_stream stream);

/* two independent convolutions of the SAME input in one launch under config `cfg` (the dual-launch path of the entry blocks) */
int cotr_op_conv_dual_cfg(const float* x, const float* w0, const float* scale0, const float* bias0, int relu0, float* y0, int Cout0,
                          int ksize0, int stride0, const float* w1, const float* scale1, const float* bias1, int relu1, float* y1,
                          int Cout1, int ksize1, int stride1, int B, int Hin, int Win, int Cin, int cfg, cotr_stream stream);

/* ---- libcotr_hip_exp.so only (COTR_EXPERIMENTAL): op-level entry points of two measured dead ends ---- */
#ifdef COTR_EXPERIMENTAL
/* decoder tail: out[b][q][0..1] = corr_embed(LayerNorm(x)) for x [nb_pairs*nq, 256]; hs (optional) receives the normalised rows */
int cotr_op_dec_head(const float* x, const float* nw, const float* nb, const float* w0, const float* b0, const float* w1,
                     const float* b1, const float* w2, const float* b2, float* hs, float* out, int nb_pairs, int nq, int q_total,
                     cotr_stream stream);
/* y [M][256] = LayerNorm(x [M][K] . w [256][K]^T + bias + residual [M][256]) * ln_w + ln_b in one launch (op-level entry for the tests) */
int cotr_op_linear_ln(const float* x, const float* w, const float* bias, const float* residual, const float* ln_w, const float* ln_b,
                      float* y, int M, int K, cotr_stream stream);
/* RESEARCH (csrc/experimental/gemm_h2.h): y[i] = packed split-f16 form of x[i] (f16(x) | f16((x - f16(x)) * 2^11) << 16), n a multiple of 4,
 * 16-byte aligned, in place allowed.  cotr_op_linear / cotr_op_conv with the forced configurations 46 / 47 take BOTH operands (activations
 * and weights) in this form and return fp32; |x| must stay below 65504.  Not bit-identical to the fp32-MFMA path. */
int cotr_op_split_h2(const float* x, void* y, size_t n, cotr_stream stream);
int cotr_op_unsplit_h2(const void* x, float* y, size_t n, cotr_stream stream);   /* the inverse: exact */
/* flags of the following cotr_op_linear_cfg / cotr_op_conv_cfg calls of this thread on configurations 46 / 47: bit 0 = y is written packed,
 * bit 1 = the residual is packed (what a chain of such launches passes from one to the next); 0 restores fp32 residual / output */
int cotr_op_set_h2_flags(int flags);
/* RANGE SAFETY of the research path: a cotr_encode / cotr_decode / cotr_forward that ran with split_f16 on and packed an activation outside f16's
 * range (|x| >= 65504) is run again on the fp32-MFMA kernels before it returns; this counts those re-runs (process-wide) */
long cotr_h2_fallbacks(void);
/* cotr_op_attention on PACKED k / v (q fp32 or packed: q_packed; o fp32 or packed: out_packed), csrc/experimental/attention_h2.hip */
int cotr_op_attention_h2(const float* q, int ldq, int q_packed, const float* k, const float* v, int ldkv, float* o, int ldo, int out_packed,
                         int nb, int nq, cotr_stream stream);
#endif

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* COTR_HIP_H */
