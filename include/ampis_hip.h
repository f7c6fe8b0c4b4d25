/*
 * ampis_hip.h — C ABI of libampis_hip.so: the MI355X (gfx950) Mask R-CNN R50-FPN hot path that
 * rccohn/AMPIS reaches through detectron2.
 *
 * The reference has no FFI of its own; its boundary to this path is the detectron2 Python API
 * (SURVEY.md §8b). Each entry point below names the reference call site it replaces:
 *   - amp_infer*                 <- `predictor(img)` at colab/AMPIS Tutorial.ipynb cell 26/28 (DefaultPredictor.__call__),
 *                                   whose output is consumed by ampis/data_utils.py:275-278 (compress_pred)
 *   - amp_dets (RLE counts)      <- `RLE.encode(np.asfortranarray(x))` at ampis/data_utils.py:275
 *   - amp_rle_*                  <- pycocotools.mask calls at ampis/data_utils.py:275, ampis/analyze.py:108,158,315-321,
 *                                   ampis/structures.py:465-468,568,752
 *   - amp_model_* / amp_init     <- `DefaultPredictor(cfg)` (notebook cell 24) / `DefaultTrainer(cfg)` (cell 22,
 *                                   ampis/data_utils.py:135-160)
 * The per-kernel entry points (amp_conv2d_nhwc, amp_roi_align, amp_nms, ...) are the stages of that path
 *  and exist so the parity tests can check each stage against the CPU oracle.
 *
 * Conventions: plain C types only; every pointer is a DEVICE pointer unless its name ends in _h (host);
 * activations are fp32 NHWC, weights fp32 [Cout][KH][KW][Cin]; every function returns AMP_OK (0) or a
 * negative amp_status and leaves a message readable through amp_last_error(); handles are opaque, one per
 * HIP stream, thread-compatible but not thread-safe.
 */
#ifndef AMPIS_HIP_H
#define AMPIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum amp_status {
    AMP_OK = 0,
    AMP_ERR_ARG = -1,      /* bad argument / shape the kernels do not support */
    AMP_ERR_HIP = -2,      /* HIP runtime error (message has the call and hipGetErrorString) */
    AMP_ERR_NOMEM = -3,    /* workspace too small */
    AMP_ERR_STATE = -4     /* call out of order (e.g. infer before weights are loaded) */
} amp_status;

typedef struct amp_ctx amp_ctx;

/* Library / context -------------------------------------------------------------------------- */
const char* amp_last_error(void);
int  amp_version(void);
/* flags & AMP_STREAM_BORROW: launch on `hip_stream` (a hipStream_t; NULL = the legacy default stream) and never
 * destroy it; otherwise hip_stream is ignored and the context creates (and owns) a non-blocking HIP stream. */
#define AMP_STREAM_BORROW 1
int  amp_init(int device, void* hip_stream, int flags, amp_ctx** out);
void amp_destroy(amp_ctx* ctx);
int  amp_sync(amp_ctx* ctx);
void* amp_stream(amp_ctx* ctx);
/* HIP-event stopwatch on the context's stream: start records an event, stop records a second one, waits for it
 * and returns the elapsed milliseconds between the two (bench.py times kernels with this, not with torch events). */
int  amp_timer_start(amp_ctx* ctx);
int  amp_timer_stop(amp_ctx* ctx, float* ms_h);

/* Live profile of the dominant kernel: between begin and end every amp_conv2d_nhwc launch on this context is bracketed
 * by a HIP-event pair on the context's stream; end waits for the stream and sums duration and algorithmic FLOPs
 * (2*M*Cout*KH*KW*Cin) per slot: [0] = wide conv tiles (128x128 / 128x256), [1] = 128x64 conv tiles, [2] = the weight-gradient
 * MFMA kernel of amp_conv2d_wgrad (wgrad_f16x3_kernel / wgrad_mfma_kernel, without its row-table and reduce passes). */
typedef struct amp_prof_summary {
    long long launches[3];
    double ms[3];
    double flops[3];
    int truncated;            /* 1 when more launches happened than max_launches */
} amp_prof_summary;
int  amp_prof_begin(amp_ctx* ctx, int max_launches);
int  amp_prof_end(amp_ctx* ctx, amp_prof_summary* out);
/* between begin and end: stop / resume recording (the event pairs themselves cost ~5 us of idle GPU per launch: sample some steps) */
int  amp_prof_pause(amp_ctx* ctx, int paused);
/* After amp_prof_end: the recorded launches one by one, in launch order -- duration, algorithmic FLOPs and algorithmic BYTES (every
 * operand the launch must read and every value it must write, once: sampled input rows + weights + output + residual / mask), and the
 * GEMM shape M x N x K.  What a per-layer roofline needs: a short-K 1x1 layer is bounded by its bytes, not by the matrix pipe
 * (tools/layer_roofline.py).  *n_out = number of recorded launches (may exceed cap; the first cap are written). */
typedef struct amp_prof_launch {
    double ms, flops, bytes;
    int M, N, K;
    int slot;                 /* index into amp_prof_summary's arrays */
} amp_prof_launch;
int  amp_prof_launches(amp_ctx* ctx, amp_prof_launch* out, int cap, int* n_out);

/* Device memory helpers (so that hosts without torch can drive the library) ----------------- */
int amp_malloc(amp_ctx* ctx, size_t bytes, void** out);
int amp_free(amp_ctx* ctx, void* p);
int amp_memcpy_h2d(amp_ctx* ctx, void* dst, const void* src_h, size_t bytes);
int amp_memcpy_d2h(amp_ctx* ctx, void* dst_h, const void* src, size_t bytes);
int amp_memset(amp_ctx* ctx, void* dst, int value, size_t bytes);

/* Convolution arithmetic of this context (every conv / fc of the inference path and, in training, the forward and data-gradient
 * convolutions; weight gradients always run on the fp32 MFMA).
 * AMP_CONV_F32:   v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulation.
 * AMP_CONV_F16X3: fp32 in / fp32 out on the f16 matrix pipe: each operand is split x = hi + lo (two f16, 22 significant bits for
 *                 2^-25 < |x| < 65504), a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with exact products and fp32 accumulation;
 *                 error against an fp64 reference measured at or below the fp32-MFMA kernel's (tests/test_conv_modes_gpu.py).
 *                 An operand of magnitude >= 65504 leaves a non-finite accumulator, raises the range flag below, and
 *                 amp_model_infer re-runs the batch in AMP_CONV_F32.  Default; override with amp_set_conv_mode or AMP_CONV_MODE=f32|f16x3. */
enum { AMP_CONV_F32 = 0, AMP_CONV_F16X3 = 1 };
int amp_set_conv_mode(amp_ctx* ctx, int mode);
int amp_get_conv_mode(amp_ctx* ctx);
/* *flag_h = 1 when an AMP_CONV_F16X3 convolution since the last clear left a non-finite accumulator; synchronises the stream */
int amp_conv_range_flag(amp_ctx* ctx, int clear, int* flag_h);

/* w [rows][K] fp32 (K % 32 == 0) -> the AMP_CONV_F16X3 operand layout (same byte size); amp_conv2d_nhwc does this per call,
 * amp_model_finalize once per layer. */
int amp_split_weights(amp_ctx* ctx, const float* w, long long rows, int K, float* w_split);

/* Stage a7 (DefaultPredictor.__call__: ResizeShortestEdge): uint8 bilinear resize, bit-exact with PIL's Image.resize(BILINEAR)
 * (antialiased triangle filter, 22-bit fixed-point coefficients, horizontal then vertical pass).  src [H,W,3], dst [h,w,3] and
 * tmp (amp_resize_scratch_bytes) are device pointers. */
size_t amp_resize_scratch_bytes(int H, int W, int h, int w);
int amp_resize_bilinear_u8(amp_ctx* ctx, const unsigned char* src, int H, int W, unsigned char* dst, int h, int w, void* tmp);
/* Train-time input pipeline on the device (detectron2 DatasetMapper under ampis/data_utils.py:171-175: ResizeShortestEdge + RandomFlip, then
 * ImageList.from_tensors): the same resize written into the top-left h x w pixels of a frame slot whose rows are dst_pitch pixels apart,
 * mirrored left-right when flip != 0 (== numpy out[:, ::-1] of the resized image).  h == H and w == W: a (mirrored) copy, tmp may be null. */
int amp_resize_flip_u8(amp_ctx* ctx, const unsigned char* src, int H, int W, unsigned char* dst, int dst_pitch, int h, int w, int flip, void* tmp);
/* RandomCrop + ResizeShortestEdge + RandomFlip (INPUT.CROP, INPUT.RANDOM_FLIP "horizontal" | "vertical"): `src` points at the first pixel of
 * an H x W window of an uploaded image whose rows are src_pitch pixels apart (src_pitch >= W); the window is resized like above into the frame
 * slot.  flip bit 0 mirrors left-right, bit 1 up-down; both are applied where the last pass writes (no extra pass, no extra buffer).  With
 * src_pitch == W and flip in {0, 1} this is amp_resize_flip_u8, byte for byte. */
int amp_crop_resize_flip_u8(amp_ctx* ctx, const unsigned char* src, int src_pitch, int H, int W, unsigned char* dst, int dst_pitch, int h, int w,
                            int flip, void* tmp);

/* Stage a9/a10/a11/a14/a16: implicit-GEMM convolution on fp32 MFMA ------------------------- */
typedef struct amp_conv_desc {
    int B, H, W, Cin;         /* input  [B,H,W,Cin]  (Cin % 4 == 0) */
    int Cout;                 /* weight [Cout][KH][KW][Cin] */
    int KH, KW, stride, pad;
    int relu;                 /* 1: y = max(y, 0) after the affine and the residual */
    int res_mode;             /* 0 none; 1 res[B,Ho,Wo,Cout] added; 2 res[B,Ho/2,Wo/2,Cout] nearest-upsampled x2 then added (FPN top-down) */
    int out_mode;             /* 0 NHWC [B,Ho,Wo,Cout]; 1 ConvTranspose 2x2 s2 scatter: Cout = 4*C2 ordered (ky,kx,co) -> y[B,2Ho,2Wo,C2];
                                 2 stride-2 scatter: row (b,oy,ox) -> y[B,2Ho,2Wo,Cout] at (2oy,2ox), y pre-zeroed (dgrad of a strided 1x1) */
} amp_conv_desc;
/* y = act( conv(x, w) * scale[c] + shift[c] (+ res) ); scale may be NULL (= 1), shift may be NULL (= 0). */
int amp_conv2d_nhwc(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w,
                    const float* scale, const float* shift, const float* res, float* y);
/* Grouped convolution (detectron2 ResNeXt `conv2`, groups = RESNETS.NUM_GROUPS): Cin == Cout, Cin / groups in {8,16,32,64}.
 * w_win is the window layout [Cout][KH][KW][64] made by amp_group_expand_weights from grouped weights [Cout][KH][KW][Cin/groups]. */
int amp_group_expand_weights(amp_ctx* ctx, const float* w, int Cout, int KH, int KW, int cpg, float* w_win);
int amp_conv2d_grouped_nhwc(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w_win,
                            const float* scale, const float* shift, const float* res, float* y);
/* the same on split-format tensors (AMP_CONV_F16X3; fmt: AMP_FMT_* bits as in amp_conv2d_nhwc_fmt): the 64-channel window of an N tile
 * is 256 B of a split row as it is of an fp32 row, so a ResNeXt trunk stays in the format through its grouped layers */
int amp_conv2d_grouped_nhwc_fmt(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* w_win,
                                const float* scale, const float* shift, const float* res, float* y, int fmt);
/* Backward of the grouped convolution (training a ResNeXt backbone).  Weight gradient in the window layout (zero outside a channel's
 * group), times scale[co] when given (FrozenBN); fp32 MFMA, partial sums over row slices added in slice order.  scratch:
 * amp_grouped_wgrad_scratch_floats(d) floats.  Data gradient: the grouped forward convolution of dy with amp_group_dgrad_weights'
 * windows (transposed inside each 64-channel tile, taps flipped, times scale[co]); stride 1 (a stride-2 layer spreads dy over the even
 * positions of a zeroed map first). */
size_t amp_grouped_wgrad_scratch_floats(const amp_conv_desc* d);
int amp_conv2d_grouped_wgrad(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* dy, const float* scale,
                             float* scratch, float* grad_win);
/* The same with operands in the split hi|lo' row format (same bytes as fp32): fmt bit 0: x, bit 1: dy; decoded on the load (exact).  dy -- split
 * or fp32 -- may hold dy * 2^dy_shift (the scaled gradient chain of a training step): the reduce pass multiplies the sums by 2^-dy_shift. */
int amp_conv2d_grouped_wgrad_fmt(amp_ctx* ctx, const amp_conv_desc* d, int groups, const float* x, const float* dy, const float* scale,
                                 float* scratch, float* grad_win, int fmt, int dy_shift);
int amp_group_dgrad_weights(amp_ctx* ctx, const float* w_win, const float* scale, int C, int KH, int KW, float* wt_win);
/* same, with an optional mask tensor indexed like y: y = mask > 0 ? y : 0 (applied last; the ReLU backward of a data gradient) */
int amp_conv2d_nhwc_ex(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w, const float* scale, const float* shift,
                       const float* res, const float* mask, float* y);

/* The split operand format as a tensor format (AMP_CONV_F16X3 inference: the trunk's native activation format).  A [rows][C] fp32
 * tensor and its split form have the same byte size and the same row offsets; inside a row every 32 channels are 32 f16 `hi` halves
 * (64 B) followed by 32 f16 halves of lo' = (x - hi) * 2^11 (64 B).  amp_split_weights makes it from fp32 rows, amp_unsplit_rows
 * reads it back (hi + lo' * 2^-11, exact in fp32); a convolution can take its input and its residual in it and write its output in
 * it (fmt bits below), which changes the data path (both operands staged by LDS-DMA, no split in the kernel), not the arithmetic. */
enum { AMP_FMT_X_SPLIT = 1, AMP_FMT_Y_SPLIT = 2, AMP_FMT_RES_SPLIT = 4, AMP_FMT_MASK_SPLIT = 8 };
int amp_conv2d_nhwc_fmt(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* w, const float* scale, const float* shift,
                        const float* res, float* y, int fmt);
int amp_unsplit_rows(amp_ctx* ctx, const float* x_split, long long rows, int C, float* out);
/* The tail of a res2 bottleneck (detectron2 BottleneckBlock.forward, modeling/backbone/resnet.py: conv2 3x3 64 -> 64 + FrozenBN + ReLU, conv3 1x1
 * 64 -> C3 + FrozenBN, + shortcut, ReLU) in ONE launch, every tensor in the split row format and the weights pre-split (amp_split_weights): conv2's
 * output never reaches memory.  Bit-identical to the two amp_conv2d_nhwc_fmt calls it replaces.  AMP_ERR_STATE when it does not apply
 * (not AMP_CONV_F16X3, C3 % 64 != 0 or > 256, fewer than 512 tiles of 8 x 16 pixels). */
int amp_bottleneck64_tail(amp_ctx* ctx, int B, int H, int W, const float* x_split, const float* w2_split, const float* scale2, const float* shift2,
                          const float* w3_split, const float* scale3, const float* shift3, int C3, const float* res_split, float* y_split);

/* Stage a19: backward building blocks -------------------------------------------------------------------------------- */
/* dW[Cout][KH][KW][Cin] (= or +=) scale[n] * conv-wgrad(dy [B*Ho*Wo, Cout], x [B,H,W,Cin]); `d` describes the FORWARD conv.
 * Cin % 128 == 0, Cout % 4 == 0. scratch: amp_conv_wgrad_scratch_floats(d) floats. Deterministic (split-K slabs, fixed-order sum). */
size_t amp_conv_wgrad_scratch_floats(const amp_conv_desc* d);
int amp_conv2d_wgrad(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* dy, const float* scale, float* scratch,
                     float* grad, int accumulate);
/* same; in AMP_CONV_F16X3 mode dy (or x) is multiplied by 2^dy_shift (2^x_shift) before the f16 split and the result by the inverse
 * (exact): loss gradients of 1e-9..1e-4 need it to keep fp32-equivalent accuracy. At most one shift non-zero; ignored in AMP_CONV_F32.
 * |operand * 2^shift| >= 65504 raises amp_conv_range_flag(). amp_conv2d_wgrad == shifts 0. */
int amp_conv2d_wgrad_scaled(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* dy, const float* scale, float* scratch,
                            float* grad, int accumulate, int dy_shift, int x_shift);
/* The same with x in the split hi|lo' row format (AMP_FMT_X_SPLIT; written by amp_conv2d_nhwc_fmt / the native trunk): x_split = 1;
 * x_split & 2: dy is in that format as well and already multiplied by 2^dy_shift (what a data-gradient convolution with AMP_FMT_Y_SPLIT
 * on scaled split gradients writes);
 * bias_grad != NULL (AMP_CONV_F16X3 only): bias_grad[n] (= or +=) sum over the pixels of dy[.][n], summed on the side by the MFMA kernel
 * from the dy tiles it stages anyway (replaces a separate amp_colsum pass over dy). */
int amp_conv2d_wgrad_fmt(amp_ctx* ctx, const amp_conv_desc* d, const float* x, const float* dy, const float* scale, float* scratch,
                            float* grad, int accumulate, int dy_shift, int x_shift, int x_split, float* bias_grad, int bias_accumulate);
/* out[n] (= or +=) sum_m dy[m][n]; N % 4 == 0; scratch >= ceil(M/512)*N floats */
int amp_colsum(amp_ctx* ctx, const float* dy, int M, int N, float* scratch, float* out, int accumulate);
/* the same pass also writing dy * 2^shift in the split row format (N % 32 == 0): the dy operand of amp_conv2d_wgrad_fmt(x_split & 2) */
int amp_colsum_split(amp_ctx* ctx, const float* dy, int M, int N, float* scratch, float* out, int accumulate, float* dy_split, int shift);
/* the column sums alone of a dy that is already split rows of dy * 2^shift (read-only; the values summed are the 22-bit ones the split holds) */
int amp_colsum_of_split(amp_ctx* ctx, const float* dy_split, int M, int N, float* scratch, float* out, int accumulate, int shift);
/* wt[Cin][KH][KW][Cout] = flipped / transposed / scaled copy of w[Cout][KH][KW][Cin]: conv(dy, wt) is the data gradient */
int amp_dgrad_weights(amp_ctx* ctx, const float* w, const float* scale, int Cout, int KH, int KW, int Cin, float* wt);
/* the same tensor already in the AMP_CONV_F16X3 split row format (= amp_split_weights of amp_dgrad_weights' result, bit for bit, in one
 * pass; Cout % 32 == 0): what a training step of amp_model makes for all its layers in one launch.  Allocates two small tables per call. */
int amp_dgrad_weights_split(amp_ctx* ctx, const float* w, const float* scale, int Cout, int KH, int KW, int Cin, float* wt_split);
/* dfeat[level] += RoIAlign-backward(dout [R,P,P,C]).  C == 256: owner-computes, no atomics -- every 4x4 tile of a gradient map is
 * summed by one wave over the RoIs in index order: bitwise reproducible.  Other C: float atomics (reproducible to fp32 rounding).
 * _batched: B = number of images (maps are [B,h,w,C]); amp_roi_align_bwd derives it from batch_idx (one small read-back). */
int amp_roi_align_bwd(amp_ctx* ctx, float* const dfeat[4], const int fh[4], const int fw[4], const int stride[4], int C, const float* rois,
                      const int* batch_idx, int R, int P, const float* dout);
int amp_roi_align_bwd_batched(amp_ctx* ctx, float* const dfeat[4], const int fh[4], const int fw[4], const int stride[4], int C, const float* rois,
                              const int* batch_idx, int R, int P, const float* dout, int B);
int amp_upsample2_bwd(amp_ctx* ctx, const float* dfine, float* dcoarse, int B, int Hc, int Wc, int C);   /* dcoarse += 2x2 sums */
/* dcoarse = the 2x2 sums: what amp_upsample2_bwd leaves in a zero-filled dcoarse, bit for bit; dcoarse may be uninitialised (it is written,
 * never read).  The form a training step of amp_model runs. */
int amp_upsample2_bwd_init(amp_ctx* ctx, const float* dfine, float* dcoarse, int B, int Hc, int Wc, int C);
int amp_subsample2_bwd(amp_ctx* ctx, const float* dy, float* dx, int B, int H, int W, int C);           /* dx[::2, ::2] += dy */
int amp_relu_mask(amp_ctx* ctx, float* g, const float* act, size_t n);                                                         /* g = act > 0 ? g : 0 */
/* The same with the activation in the split hi|lo' row format ([.., C] rows, C % 32 == 0): the mask is decode(act_split) > 0, so it sees
 * what the split kept of the activation.  The floor: a positive activation down to 2^-35 still decodes positive (hi = 0, lo' = 2^-24, the
 * smallest f16 subnormal); 2^-36 and below splits to all zeros and is masked out like 0.  -0.0 is not positive. */
int amp_relu_mask_split(amp_ctx* ctx, float* g, const float* act_split, size_t n, int C);
/* Scaled split gradients (the backbone's backward pass on the ring kernel): out = split(2^shift * (act > 0 ? g : 0)), and the
 * stride-2 scatter-add back into an fp32 gradient: dx[b,2y,2x,:] += 2^-shift * decode(dy_split[b,y,x,:]). */
int amp_relu_mask_to_split(amp_ctx* ctx, const float* g, const float* act_split, float* out_split, size_t n, int C, int shift);
int amp_subsample2_bwd_split(amp_ctx* ctx, const float* dy_split, float* dx, int B, int H, int W, int C, int shift);
/* dx (fp32, same resolution) += decode(dy_split) * 2^-shift: a scaled split gradient joins an fp32 gradient map (ResNeXt first blocks, where
 * conv1's data gradient lives at the block's INPUT resolution). */
int amp_accumulate_split(amp_ctx* ctx, const float* dy_split, float* dx, long long rows, int C, int shift);
/* up[b, 2y, 2x, :] = src[b, y, x, :] as raw 16-byte chunks (split rows stay split rows), every other pixel of `up` zero: the input of the stride-1
 * data gradient of a stride-2 convolution whose gradient arrives in the split format.  up: [B, H, W, C], src: [B, ceil(H/2), ceil(W/2), C]. */
int amp_scatter2_rows(amp_ctx* ctx, const float* src, float* up, int B, int H, int W, int C);
/* dx[p][c] = act[p][c] > 0 ? sum_k dl[p][k] * w[k][c] : 0 over dl [npix][ld] (K <= ld), w [K][C]; the sum runs over k in index order from 0,
 * the product and the sum each rounded in fp32.  act == NULL: no mask. */
int amp_small_k_dgrad(amp_ctx* ctx, const float* dl, int ld, int K, const float* w, int C, const float* act, float* dx, size_t npix);
/* The same product for dl rows of 16 floats (K <= 16), C % 32 == 0 and act in the split row format, leaving dx * 2^shift as split rows (the
 * dy operand of the ring kernels) and colsum_out[c] (= or +=) the sum over the pixels of dx[.][c] (the bias gradient of the layer that
 * produced act); scratch: ceil(npix / 512) * C floats. */
int amp_small_k_dgrad_split(amp_ctx* ctx, const float* dl, int K, const float* w, int C, const float* act_split, float* dx_split, int npix,
                            int shift, float* scratch, float* colsum_out, int accumulate);
/* The same with dl rows of ld = 4, 8, 12 or 16 floats (K <= ld) and act as plain fp32 rows (the mask predictor behind the deconv, whose output
 * is fp32): dx is amp_small_k_dgrad's value, * 2^shift, as split rows; colsum_out = the deconv's bias gradient. */
int amp_small_k_dgrad_split_f32act(amp_ctx* ctx, const float* dl, int ld, int K, const float* w, int C, const float* act, float* dx_split, int npix,
                                   int shift, float* scratch, float* colsum_out, int accumulate);
/* ... and with act in the split row format again (a deconv output kept split: amp_conv2d_nhwc_fmt with out_mode 1 and AMP_FMT y split).
 * The dl columns k >= K: _f32act does not read their values (they may hold anything, NaN included).  The two variants with act in the split
 * format multiply them by a zero weight, so they must be FINITE (a NaN or inf there reaches every dx of the row).  The model zero-fills
 * them: it calls amp_mask_target_loss_fmt with K = Kp, which writes every column of the padded rows. */
int amp_small_k_dgrad_split_ld(amp_ctx* ctx, const float* dl, int ld, int K, const float* w, int C, const float* act_split, float* dx_split, int npix,
                               int shift, float* scratch, float* colsum_out, int accumulate);
int amp_colsum_finish(amp_ctx* ctx, const float* partial, int parts, int N, float* out, int accumulate);
int amp_deconv_grad_transpose(amp_ctx* ctx, const float* in, float* out, int Cin, int T, int C2, int accumulate);
/* torch.optim.SGD: g' = grad_scale*g + wd*p; v = mu*v + g'; p -= lr*v */
int amp_sgd_update(amp_ctx* ctx, float* p, const float* g, float* v, size_t n, float lr, float momentum, float weight_decay, float grad_scale);
/* The general step: what detectron2's build_optimizer adds to torch.optim.SGD (SOLVER.NESTEROV, BIAS_LR_FACTOR, WEIGHT_DECAY_BIAS,
 * CLIP_GRADIENTS).  Per element, every operation rounded on its own:
 *   gs = g * grad_scale
 *   gc = gs | min(max(gs, -c), c) (AMP_CLIP_VALUE) | gs * k (AMP_CLIP_NORM, per tensor: N = ||gs||_norm_type accumulated in fp64 and
 *        narrowed to fp32, k = min(c / (N + 1e-6), 1) in fp32 -- torch.nn.utils.clip_grad_norm_ on that tensor alone)
 *   g' = gc + wd_t * p;  v = mu * v + g';  u = nesterov ? g' + mu * v : v;  p -= lr_t * u
 * lr_t = lr * bias_lr_factor and wd_t = weight_decay_bias for bias tensors, lr and weight_decay for the others. */
enum { AMP_CLIP_NONE = 0, AMP_CLIP_VALUE = 1, AMP_CLIP_NORM = 2 };
typedef struct amp_sgd_opts {
    float lr, momentum, weight_decay, grad_scale;
    int nesterov;
    float bias_lr_factor, weight_decay_bias;
    int clip_type;
    float clip_value;
    float norm_type;                 /* 1, 2 or INFINITY (AMP_CLIP_NORM only) */
} amp_sgd_opts;
/* lr 0, momentum 0.9, weight_decay = weight_decay_bias = 1e-4, grad_scale 1, bias_lr_factor 1, no Nesterov, AMP_CLIP_NONE (clip_value 1, norm_type 2) */
int amp_sgd_opts_default(amp_sgd_opts* opts);
/* The step on a caller's arenas (device) and tensor table (host: offset in floats, a multiple of 4; n >= 1 floats; is_bias), so that the
 * stage can be tested without a model.  norms_h / coefs_h (host, [ntensors], or NULL): N and k of every tensor (0 and 1 without
 * AMP_CLIP_NORM).  Synchronises.  Refuses (AMP_ERR_ARG, naming the field) a norm_type other than 1, 2, INFINITY, clip_value <= 0 and
 * non-finite scalars. */
int amp_sgd_step_tensors(amp_ctx* ctx, float* p, const float* g, float* v, const unsigned long long* off_h, const unsigned long long* n_h,
                         const unsigned char* is_bias_h, int ntensors, const amp_sgd_opts* opts, float* norms_h, float* coefs_h);


/* Stage a8 / a9 / a10: memory-bound NHWC helpers --------------------------------------------- */
/* uint8 BGR [B,H,W,3] -> fp32 [B,Hp,Wp,4] = (x - mean) / std, zero padded (4th channel 0). img_hw: optional device [B][2]
 * valid (h,w) of each image inside the common HxW frame; pixels beyond it are 0 after normalisation (ImageList.from_tensors). */
int amp_preprocess(amp_ctx* ctx, const uint8_t* img_bgr, int B, int H, int W, int Hp, int Wp, const float mean[3],
                   const float std[3], const int* img_hw, float* out);
int amp_maxpool3x3s2(amp_ctx* ctx, const float* x, int B, int H, int W, int C, float* y);   /* k3 s2 p1 */
int amp_subsample2(amp_ctx* ctx, const float* x, int B, int H, int W, int C, float* y);     /* x[:, ::2, ::2] */

/* Stage a12: RPN candidate selection ----------------------------------------------------------- */
typedef struct amp_rpn_levels {
    int nlevels;               /* <= 5 */
    int A;                     /* anchors per location (3), 1..9 */
    int ld;                    /* row length of pred: A logits, then A*4 deltas, then padding (>= 5 A; the model uses 16 * ceil(5 A / 16)) */
    const float* pred[5];      /* per level [B, h*w, ld] */
    int h[5], w[5], stride[5], anchor_size[5];
    /* MODEL.ANCHOR_GENERATOR.{SIZES, ASPECT_RATIOS} per level (detectron2 DefaultAnchorGenerator, offset 0): cell anchors in the order
     * `for size: for ratio:`, n_sizes[l] * n_ratios[l] == A.  n_sizes[l] == 0 (a zero-initialised tail): the one size anchor_size[l]
     * with the ratios 0.5, 1, 2. */
    int n_sizes[5], n_ratios[5];
    double sizes[5][9], ratios[5][9];   /* double: the cell anchors are computed from the cfg's python floats */
} amp_rpn_levels;
/* Host only: the cell anchors of level l as the kernels use them, cell[a] = (x1, y1, x2, y2) around the origin, computed in double and
 * stored fp32 (generate_cell_anchors); *A_out = their number.  cap >= 9 rows is always enough. */
int amp_cell_anchors(const amp_rpn_levels* lv, int level, float* cell /* [cap][4] */, int cap, int* A_out);
/* per (image, level) top-k by logit, descending, ties by ascending anchor index. keys_scratch: [B*nlevels*max_n] u32. */
int amp_rpn_topk(amp_ctx* ctx, const amp_rpn_levels* lv, int B, int k, uint32_t* keys_scratch, int max_n, int* sel_idx,
                 float* sel_logit, int* sel_count);
/* decode + clip the selected anchors; sortkey = 0 for non-finite / empty boxes. boxes [B,cap,4], sortkey [B,cap]. */
int amp_rpn_decode(amp_ctx* ctx, const amp_rpn_levels* lv, int B, int k, const int* sel_idx, const float* sel_logit,
                   const int* sel_count, int img_h, int img_w, int cap, float* boxes, unsigned long long* sortkey,
                   int* anchor_id /* [B,cap] global anchor index of each candidate, or NULL */);
/* same with per-image sizes: img_hw = device int [B][2] (h, w) of each image inside the common frame (a batch of differently sized
 * images, detectron2 ImageList): every image's proposals are clipped to ITS size (find_top_rpn_proposals); NULL = img_h / img_w. */
int amp_rpn_decode_sized(amp_ctx* ctx, const amp_rpn_levels* lv, int B, int k, const int* sel_idx, const float* sel_logit,
                         const int* sel_count, int img_h, int img_w, const int* img_hw, int cap, float* boxes,
                         unsigned long long* sortkey, int* anchor_id);
/* per image: order `cap` (<= 16384) 64-bit sort words descending; gather boxes_in[b][pos] (box_stride entries per image);
 * outputs sorted boxes/scores/categories [B,cap], the number of valid entries [B], optionally the source positions. */
int amp_sort_gather(amp_ctx* ctx, int B, int cap, int box_stride, const unsigned long long* sortkey, const float* boxes_in,
                    float* boxes_out, float* score_out, int* cat_out, int* count_out, int* pos_out,
                    const int* payload_in /* [B,box_stride] or NULL */, int* payload_out /* [B,cap] or NULL */);
/* the same with a hint: n_used[b] (device, may exceed cap) = the sort words of image b are its first n_used[b] slots and the rest are 0
 * (the compacted candidate list of amp_box_candidates): only the smallest power of two that holds them is sorted. NULL: all cap slots. */
int amp_sort_gather_n(amp_ctx* ctx, int B, int cap, int box_stride, const unsigned long long* sortkey, const float* boxes_in,
                      float* boxes_out, float* score_out, int* cat_out, int* count_out, int* pos_out,
                      const int* payload_in, int* payload_out, const int* n_used);

/* Stages a12 / a15: batched greedy NMS on score-sorted boxes (cap <= 16384 per image) ---------- */
/* mask_scratch: [B*cap*ceil(cap/64)] u64. keep_idx [B,max_keep] (positions, ascending), keep_count [B]. */
int amp_nms(amp_ctx* ctx, int B, int cap, const float* boxes, const int* cats, const int* counts, float thresh,
            int max_keep, unsigned long long* mask_scratch, int* keep_idx, int* keep_count);

/* Stage a12, second half of find_top_rpn_proposals (detectron2 proposal_utils.py: batched_nms(boxes, scores, lvl, nms_thresh)[:post_nms_topk]):
 * the decoded candidates of amp_rpn_decode (level l of image b at [off, off + sel_count[b][l]) of its `cap` slots, each level in
 * descending order; sort word 0 = invalid) are suppressed PER LEVEL and the survivors of the L levels merged by sort word: the first
 * max_keep per image with boxes / logits / levels (/ payload_in[b][slot] -> payload_out), the remaining rows zero / -1 as
 * amp_gather_dets leaves them.  Identical to amp_sort_gather + amp_nms(cats = level) + amp_gather_dets on the same candidates.
 * scratch: amp_rpn_nms_scratch_words(B, L, k) u64. */
size_t amp_rpn_nms_scratch_words(int B, int L, int k);
int amp_rpn_nms_levels(amp_ctx* ctx, int B, int L, int k, int cap, const float* cand_boxes, const unsigned long long* cand_keys,
                       const int* sel_count, float thresh, int max_keep, unsigned long long* scratch, float* prop_boxes,
                       float* prop_scores, int* prop_lvl, int* prop_count, const int* payload_in /* [B,cap] or NULL */,
                       int* payload_out /* [B,max_keep] or NULL */);

/* Stages a13 / a16: RoIAlign (aligned, sampling_ratio 0) with FPN level assignment ------------- */
typedef struct amp_fpn_feats {
    const float* feat[4];      /* p2..p5, NHWC [B,h,w,C] */
    int h[4], w[4], stride[4];
    int C;
} amp_fpn_feats;
/* rois [R,4] (x1,y1,x2,y2 in image coordinates), batch_idx [R] or NULL, roi_count device int or NULL -> out [R,P,P,C]. */
int amp_roi_align(amp_ctx* ctx, const amp_fpn_feats* f, const float* rois, const int* batch_idx, const int* roi_count,
                  int R, int P, float* out, int* level_out);

/* same with the feature maps (AMP_FMT_X_SPLIT) and / or the pooled output (AMP_FMT_Y_SPLIT) in the split row format; C % 32 == 0 */
int amp_roi_align_fmt(amp_ctx* ctx, const amp_fpn_feats* f, const float* rois, const int* batch_idx, const int* roi_count,
                      int R, int P, float* out, int* level_out, int fmt);

/* Stage a15: box-head inference ------------------------------------------------------------------ */
int amp_box_candidates(amp_ctx* ctx, const float* pred, int ld, const float* proposals, const int* prop_count, int B,
                       int Rcap, int K, const float reg_weights[4], float score_thresh, int img_h, int img_w,
                       float* dense_boxes, unsigned long long* keys, int ccap, int* cand_count, int* overflow);
int amp_box_candidates_sized(amp_ctx* ctx, const float* pred, int ld, const float* proposals, const int* prop_count, int B,
                             int Rcap, int K, const float reg_weights[4], float score_thresh, int img_h, int img_w,
                             const int* img_hw /* device [B][2] or NULL, as in amp_rpn_decode_sized */,
                             float* dense_boxes, unsigned long long* keys, int ccap, int* cand_count, int* overflow);
int amp_gather_dets(amp_ctx* ctx, int B, int cap, int D, const float* sboxes, const float* sscores, const int* scats,
                    const int* keep_idx, const int* keep_count, float* det_boxes, float* det_scores, int* det_classes,
                    const int* payload_in /* [B,cap] or NULL */, int* payload_out /* [B,D] or NULL */);
/* [B][D] detections with device-side counts -> compact rows in image order (+ the image index of every row) for the mask branch */
int amp_compact_dets(amp_ctx* ctx, int B, int D, const int* det_count, const float* det_boxes, const float* det_scores, const int* det_classes,
                     float* boxes, float* scores, int* classes, int* batch);

/* Stages a16 / a17 / a3: mask probability, paste + threshold + RLE counts ----------------------- */
/* logits [N,28,28,K] (channels last), classes [N] -> prob [N,28,28] = sigmoid of channel classes[n].  A class outside [0, K) (the -1 that
 * amp_gather_dets leaves in unused rows) reads channel 0: the row is computed, never skipped, and nothing is read out of range. */
int amp_mask_prob(amp_ctx* ctx, const float* logits, const int* classes, int N, int K, float* prob);
/* the RPN head of one pyramid level in one kernel (AMP_CONV_F16X3; stage a11): x_split [B,H,W,256] (split rows) -> 3x3 conv + bias + ReLU ->
 * the 16 predictor rows (3 objectness logits, 12 anchor deltas, 1 zero row: w_pred [16][256], b_pred [16]) as a second product in the
 * epilogue -> pred [B*H*W][16]; the 256-channel hidden tensor is never written. B*H*W >= 24576. */
int amp_rpn_head_fused(amp_ctx* ctx, const float* x_split, int B, int H, int W, const float* w_conv, const float* b_conv, const float* w_pred,
                       const float* b_pred, float* pred);
/* the same for a head of ld = 16, 32 or 48 predictor rows (A <= 3, 6, 9 anchors per location: A logits, 4 A deltas, zero rows up to ld):
 * w_pred [ld][256], b_pred [ld], pred [B*H*W][ld] */
int amp_rpn_head_fused_ld(amp_ctx* ctx, const float* x_split, int B, int H, int W, const float* w_conv, const float* b_conv, const float* w_pred,
                          const float* b_pred, int ld, float* pred);
/* the tail of the mask head in one kernel (AMP_CONV_F16X3): x_split [N,14,14,256] (split rows) -> ConvTranspose2d 2x2 s2 (w_deconv
 * [(ky,kx,co)][256], bias [1024] = the 256 biases once per tap) -> ReLU -> predictor row of classes[n] (pred_w [K][256], pred_b [K]) ->
 * sigmoid -> prob [N,28,28]; the [N,28,28,256] activation is never written */
int amp_mask_deconv_predict(amp_ctx* ctx, const float* x_split, int N, const float* w_deconv, const float* bias, const float* pred_w,
                            const float* pred_b, const int* classes, int K, float* prob);
int amp_paste_rle(amp_ctx* ctx, const float* prob, const float* det_boxes, const int* det_batch, int N, const int* out_h,
                  const int* out_w, int max_out_hw, int in_h, int in_w, float threshold, float* out_boxes, int* valid,
                  unsigned int* pool, unsigned long long pool_cap, unsigned long long* pool_used, unsigned long long* rle_off,
                  int* rle_len, int* overflow);
/* same; in_hw = device int [B][2]: the network-input size of each image (detector_postprocess scales by output / image size) or NULL;
 * pos_scratch (+ capacity, device counter) = a second pool for the transition positions the run lengths are made from: `pool` then
 * holds the run lengths only, densely (half the bytes to read back); NULL = positions behind each mask's run lengths in `pool`. */
int amp_paste_rle_sized(amp_ctx* ctx, const float* prob, const float* det_boxes, const int* det_batch, int N, const int* out_h,
                        const int* out_w, int max_out_hw, int in_h, int in_w, const int* in_hw, float threshold, float* out_boxes,
                        int* valid, unsigned int* pool, unsigned long long pool_cap, unsigned long long* pool_used,
                        unsigned long long* rle_off, int* rle_len, int* overflow, unsigned int* pos_scratch,
                        unsigned long long pos_cap, unsigned long long* pos_used);

/* Stage a18: training-mode label assignment, seeded sampling and losses (+ their gradients w.r.t. the network outputs) ---- */
int amp_anchor_labels(amp_ctx* ctx, const amp_rpn_levels* lv, int B, const float* gt_boxes, const int* gt_off, int total_gt,
                      float iou_lo, float iou_hi, float* match_val, int* match_idx, unsigned int* gt_best, signed char* label);
int amp_rpn_sample_loss(amp_ctx* ctx, const amp_rpn_levels* lv, float* const dpred[5], int B, const float* gt_boxes,
                        const int* gt_off, const signed char* label, const int* match_idx, uint32_t* keys_scratch, int batch,
                        int num_pos_max /* int(batch * POSITIVE_FRACTION), in double */, unsigned int seed, int* sampled, int* counts,
                        float* partial);
int amp_roi_sample(amp_ctx* ctx, int B, const float* prop_boxes, const int* prop_count, int Pcap, const float* gt_boxes,
                   const int* gt_classes, const int* gt_off, int K, int batch, int num_fg_max /* int(batch * POSITIVE_FRACTION), in double */,
                   float iou_thresh, unsigned int seed,
                   uint32_t* keys_scratch, int* cls_scratch, int* gti_scratch, int ncap, float* rois, int* roi_cls, int* roi_gti,
                   int* counts, const int* prop_anchor /* [B,Pcap] stable ids for the sampling hash */, int num_anchors);
int amp_box_loss(amp_ctx* ctx, int B, int batch, int K, const float* pred, int ld, float* dpred, const float* rois, const int* roi_cls,
                 const int* roi_gti, const float* gt_boxes, const int* gt_off, const float reg_weights[4], int total_rois, float* partial);
/* The box regression losses of the RPN and the box head as detectron2 configures them (MODEL.RPN.{BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA,
 * LOSS_WEIGHT, BBOX_REG_LOSS_WEIGHT}, MODEL.ROI_BOX_HEAD.{BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA, BBOX_REG_LOSS_WEIGHT}).  Per sampled positive
 * anchor / foreground RoI, every operation rounded on its own, sums in a fixed order:
 *   AMP_BOXLOSS_SMOOTH_L1 (fvcore smooth_l1_loss, reduction sum), d = predicted delta - get_deltas(source, matched GT, box weights):
 *     beta < 1e-5:  |d|, gradient sign(d)                                  (the default, beta = 0: plain L1)
 *     otherwise:    0.5 d^2 / beta with gradient d / beta for |d| < beta,  |d| - 0.5 beta with gradient sign(d) elsewhere
 *   AMP_BOXLOSS_GIOU (fvcore giou_loss, reduction sum, eps = 1e-7) on box = apply_deltas(predicted deltas, source, box weights), where
 *     dw and dh are clamped at log(1000 / 16) after the division by their weight and a clamped delta gets gradient 0:
 *     I = intersection with the GT box (0 unless both extents are strictly positive), U = area(box) + area(GT) - I,
 *     C = area of the smallest enclosing box;  loss = 1 - I / (U + eps) + (C - U) / (C + eps);  the gradient reaches the four deltas
 *     through the corners of the box.
 * The box weights are (1, 1, 1, 1) for the RPN and amp_model_cfg.bbox_reg_weights for the box head.  Normalisers and weights:
 *   loss_rpn_cls = rpn_loss_weight * sum BCE / (rpn_batch * B)
 *   loss_rpn_loc = rpn_loss_weight * rpn_bbox_reg_loss_weight * sum / (rpn_batch * B)
 *   loss_box_reg = box_bbox_reg_loss_weight * sum / max(number of sampled RoIs, 1);   loss_cls and loss_mask carry no weight.
 * The weights multiply the reported losses and the gradients alike. */
enum { AMP_BOXLOSS_SMOOTH_L1 = 0, AMP_BOXLOSS_GIOU = 1 };
typedef struct amp_loss_opts {
    int rpn_loss_type;               /* AMP_BOXLOSS_* */
    float rpn_smooth_l1_beta;
    float rpn_loss_weight;
    float rpn_bbox_reg_loss_weight;
    int box_loss_type;               /* AMP_BOXLOSS_* */
    float box_smooth_l1_beta;
    float box_bbox_reg_loss_weight;
} amp_loss_opts;
/* AMP_BOXLOSS_SMOOTH_L1 with beta 0 on both heads, every weight 1: the losses of amp_rpn_sample_loss / amp_box_loss.  No device call. */
int amp_loss_opts_default(amp_loss_opts* opts);
/* amp_rpn_sample_loss / amp_box_loss with the options (the fields of the other head are validated and otherwise unused).  dpred carries
 * the loss weights; partial stays the unnormalised, UNWEIGHTED sums ([B][2]: classification, regression).  With amp_loss_opts_default
 * both run the arithmetic of the entry points above: the same bits in dpred and partial, the same launches.  Refuse (AMP_ERR_ARG, naming the
 * field) a non-finite or negative beta or weight and an unknown loss type. */
int amp_rpn_sample_loss_ex(amp_ctx* ctx, const amp_rpn_levels* lv, float* const dpred[5], int B, const float* gt_boxes,
                           const int* gt_off, const signed char* label, const int* match_idx, uint32_t* keys_scratch, int batch,
                           int num_pos_max, unsigned int seed, int* sampled, int* counts, float* partial, const amp_loss_opts* opts);
int amp_box_loss_ex(amp_ctx* ctx, int B, int batch, int K, const float* pred, int ld, float* dpred, const float* rois, const int* roi_cls,
                    const int* roi_gti, const float* gt_boxes, const int* gt_off, const float reg_weights[4], int total_rois, float* partial,
                    const amp_loss_opts* opts);
/* Sigmoid focal loss (fvcore sigmoid_focal_loss, reduction 'sum', times `scale`) over logits [N,K] with integer labels (label K =
 * background, negative = the row is ignored), forward and gradient in one pass: *loss_d = scale * sum, dlogits (optional) = scale *
 * d sum / d logits.  alpha < 0 switches the class weighting off.  partial: device scratch of partial_cap floats (<= 2048 used); sums run in a
 * fixed order (bitwise reproducible).  Not on the reference's Mask R-CNN path; the north star names it. */
int amp_sigmoid_focal_loss(amp_ctx* ctx, long long N, int K, const float* logits, const int* labels, float alpha, float gamma, float scale,
                           float* dlogits, float* partial, int partial_cap, float* loss_d);
/* Mask targets + mask BCE loss.  Polygon ground truth: detectron2 PolygonMasks.crop_and_resize = rasterize_polygons_within_box (every
 * polygon of the instance by pycocotools' rleFrPoly at 28 x 28, merged).  Bitmask ground truth (what `get_ddicts('binary'|'label'|'rle')`
 * emits, ampis/data_utils.py:394-433,482-525): BitMasks.crop_and_resize = roi_align(mask, scale 1, sampling_ratio 0, aligned) >= 0.5,
 * evaluated straight from the instance's COCO run lengths (amp_mask_targets_bitmask; scratch = nslots x slot_words words, a slot must
 * hold width x ceil(height / 32) words of the largest mask).  amp_mask_target_loss = one polygon per instance, no bitmasks. */
int amp_mask_target_loss(amp_ctx* ctx, int N, int K, const float* logits, float* dlogits, const float* rois, const int* cls,
                         const int* poly_id, const double* poly_xy, const int* poly_off, float* partial, unsigned char* target_out);
int amp_mask_targets_bitmask(amp_ctx* ctx, int N, const float* rois, const int* inst, const unsigned long long* rle_off,
                             const uint32_t* rle_counts, const int* rle_hw, unsigned int* scratch, size_t slot_words, int nslots,
                             unsigned char* target /* [N,28,28] */, int* overflow_flag);
int amp_mask_target_loss_fmt(amp_ctx* ctx, int N, int K, const float* logits, float* dlogits, const float* rois, const int* cls,
                             const int* inst, const double* poly_xy, const int* poly_off /* per polygon */,
                             const int* inst_poly_off /* [instances+1] or NULL: one polygon per instance */,
                             const unsigned long long* rle_off /* [instances+1] or NULL */, const unsigned char* target_in,
                             float* partial, unsigned char* target_out);

/* Host-side COCO RLE codec (all pointers HOST) --------------------------------------------------- */
int amp_rle_to_string(const uint32_t* cnts, int m, char* out, size_t cap, size_t* len);
/* n lists out of one pool (list i = pool[off[i] .. +len[i])) -> n strings back to back; string i = out[str_off[i] .. str_off[i+1]) */
int amp_rle_to_strings(const uint32_t* pool, const unsigned long long* off, const int* len, int n, char* out, size_t cap,
                       size_t* str_off /* [n+1] */);
/* Device op behind AMP_RLE_STRINGS (all pointers are device pointers): mask i = pool[off[i] .. off[i] + len[i]) -> its counts string at
 * str[str_off[i] .. str_off[i] + str_len[i]); *total = bytes needed (> cap: the tail was not written). maskApi.c rleToString, restated. */
int amp_rle_strings_device(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, char* str,
                           unsigned long long cap, unsigned long long* str_off, int* str_len, unsigned long long* total);
int amp_rle_from_string(const char* s, size_t len, uint32_t* cnts, int cap, int* m_out);
int amp_rle_encode(const uint8_t* mask_colmajor, int h, int w, uint32_t* cnts, int cap, int* m_out);
int amp_rle_decode(const uint32_t* cnts, int m, int h, int w, uint8_t* mask_colmajor);
int amp_rle_area(const uint32_t* cnts, int m, unsigned long long* area);
int amp_rle_iou(const uint32_t* dt, int md, const uint32_t* gt, int mg, int iscrowd, double* iou);
/* all-pairs IoU of two pools of run lists (pycocotools.mask.iou): out[d * ng + g]; bounding boxes are compared first (h = mask height) */
int amp_rle_iou_matrix(const uint32_t* dpool, const unsigned long long* doff, const int* dlen, int nd, const uint32_t* gpool,
                       const unsigned long long* goff, const int* glen, int ng, const unsigned char* iscrowd /* [ng] or NULL */, int h,
                       double* out);
/* Pixel classes of `npairs` mask pairs (a = apool run list pair_a[p], b = bpool run list pair_b[p]) in one call: |a AND b|, |a \ b|,
 * |b \ a|.  Replaces the per-match pycocotools.mask.merge(intersect=True) + area calls of det_seg_scores (ampis/analyze.py:315-321). */
int amp_rle_pair_overlap(const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                         const unsigned long long* boff, const int* blen, const int* pair_a, const int* pair_b, int npairs,
                         unsigned long long* inter, unsigned long long* only_a, unsigned long long* only_b);
/* mask_edge_distance (ampis/analyze.py:416-499) for `n` (ground truth, prediction) pairs in one call.  ALL POINTERS ARE HOST POINTERS.
 * Masks are run lists out of two pools (list i = pool[off[i] .. off[i] + len[i]), ng / np lists) over one h x w image, h, w <= 32768;
 * pair p = (pair_g[p], pair_p[p]), any pairs, repeats allowed; box[p] = {r1, r2, c1, c2}, the merged index box of the pair, applied as the
 * slice [r1:r2, c1:c2] (0 <= r1 <= r2, 0 <= c1 <= c2; an end beyond the image is the image's end).  Pixels outside the crop do not exist for
 * the pair.  fp_d2[fp_off[p] .. fp_off[p + 1]): for every crop pixel of pred & ~gt in row-major order, the minimum over the crop's gt pixels of
 * dr^2 + dc^2, exact; fn_d2 / fn_off: the same for gt & ~pred against pred.  A query whose target mask has no pixel in the crop gets
 * 0xffffffff.  fp_cap / fn_cap: capacity of fp_d2 / fn_d2 in values (the summed areas of the pairs' masks always suffice); a smaller one is
 * AMP_ERR_NOMEM with the need in the message and nothing written.  Every run list a pair names is checked on the host first (length > 0,
 * runs summing to h * w): a malformed list is AMP_ERR_ARG and never a device access.
 * ctx == NULL: computed on the host (mask_analysis_host.hip).  Otherwise on ctx's device and stream (edge_distance.hip): the function uploads, runs a
 * fixed number of launches whatever n is, downloads and returns with the results in host memory; the order and the bytes do not depend on
 * the device's scheduling. */
int amp_mask_edge_distance(amp_ctx* ctx, const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng,
                           const uint32_t* ppool, const unsigned long long* poff, const int* plen, int np, const int* pair_g,
                           const int* pair_p, const int* box, int n, int h, int w, uint32_t* fp_d2, unsigned long long fp_cap,
                           unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap, unsigned long long* fn_off);
/* Region properties (ampis/structures.py:474-514, skimage.measure.regionprops restated) of `n` masks in one call.  ALL POINTERS ARE HOST
 * POINTERS.  Mask i is the run list pool[off[i] .. off[i] + len[i]) over one h x w image, h, w <= 32768 and h * w <= 2^30.  A region is ALL set
 * pixels of a mask, holes and disconnected parts included; r = row, c = column of the full image.
 *   bbox[i] = {rmin, cmin, rmax + 1, cmax + 1}, {0, 0, 0, 0} for an empty mask;
 *   vals[i] = {N, sum r, sum c, sum r^2, sum r c, sum c^2, P1, P2, P3, convex area, 0, 0, 0}, exact (every sum < 2^60), all 0 for an empty mask.
 * P1, P2, P3 count the border pixels (mask minus its erosion by the 4-connected cross, outside the image = 0) by n4 / nd, the numbers of their
 * 4-neighbours / diagonal neighbours on the border: P1: n4 in {2, 3} and nd <= 2; P2: (n4, nd) in {(0, 2), (1, 3)}; P3: (1, 1), (1, 2) --
 * skimage's perimeter = P1 + P2 sqrt(2) + P3 (1 + sqrt(2)) / 2.  convex area = the pixel centres inside or on the convex hull of the four edge
 * midpoints (r -+ 1/2, c), (r, c -+ 1/2) of every pixel (convex_hull_image, offset_coordinates=True), decided in half-pixel integers.
 * Every run list is checked on the host first (length > 0, runs summing to h * w, the size limits): a malformed list is AMP_ERR_ARG, nothing
 * written and never a device access.  ctx == NULL: computed on the host (mask_analysis_host.hip).  Otherwise on ctx's device and stream
 * (region_props.hip): the function uploads, runs a fixed number of launches whatever n is, downloads and returns with the results in host
 * memory; integer arithmetic only, the bytes do not depend on the device's scheduling and equal the host's. */
int amp_mask_region_props(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                          long long* bbox /* [n][4] */, unsigned long long* vals /* [n][13] */);
/* All-pairs mask intersection inside groups (ampis/applications/powder.py:80-83: every satellite of an image against every particle).  ALL
 * POINTERS ARE HOST POINTERS.  Masks are run lists out of two pools (list i = pool[off[i] .. off[i] + len[i])).  Group g -- one image of
 * gh[g] x gw[g] pixels, 1 .. 32768 a side and at most 2^30 pixels -- owns the masks a_first[g] .. a_first[g + 1] of pool A and b_first[g] ..
 * b_first[g + 1] of pool B (a_first[0] = b_first[0] = 0, both non-decreasing); na_g, nb_g are their numbers.  The block of group g in `inter`
 * starts at the sum of na_k nb_k over the groups before it, is row-major [na_g][nb_g] and holds the exact pixel count of a_i AND b_j; pairs
 * across groups are never formed.  area_a / area_b receive the pixel count of every mask of pool A / B.  inter_cap: capacity of `inter` in
 * values.  ngroups == 0, groups without masks on one side and masks without a set pixel (a row or column of zeros) are valid.  Everything is
 * checked on the host first -- the image sizes, every run list non-empty and summing to its group's h * w, the order of a_first / b_first,
 * inter_cap -- and refused with AMP_ERR_ARG naming the offending index: nothing written and never a device access.
 * ctx == NULL: computed on the host (mask_analysis_host.hip).  Otherwise on ctx's device and stream (rle_overlap.hip): the function uploads, runs one
 * launch whatever the number of groups, downloads and returns with the results in host memory; integer arithmetic only, every output word
 * written once, the bytes do not depend on the device's scheduling and equal the host's. */
int amp_rle_overlap_groups(amp_ctx* ctx, const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                           const unsigned long long* boff, const int* blen, const int* a_first /* [ngroups + 1] */,
                           const int* b_first /* [ngroups + 1] */, const int* gh, const int* gw /* [ngroups] */, int ngroups, uint32_t* inter,
                           size_t inter_cap, unsigned long long* area_a, unsigned long long* area_b);
/* Segmentation class map (ampis/analyze.py:589-699, seg_perf_iset): the pixels of one h x w image classed by what the matched pairs say of
 * them.  ALL POINTERS ARE HOST POINTERS.  Masks are run lists out of two pools (list i = pool[off[i] .. off[i] + len[i])); for pair p, g is the
 * ground-truth mask pair_g[p] and q the predicted mask pair_p[p].  TP = OR_p (g & q), FN = OR_p (g & ~q), FP = OR_p (~g & q), and
 * code = TP + 2 FN + 4 FP.  mode 1 ('all'): K = 7 classes, class k - 1 is code == k.  mode 0 ('reduced'): K = 4, the classes are code == 1,
 * code == 2, code == 4 and code in {3, 5, 6, 7}.  Each class comes back as a COCO run list over the whole image (column-major, the first count is
 * the run of zeros and may be 0): class k is counts[counts_off[k] .. counts_off[k + 1]).  pixels[c] = the pixels of code c, all 8 codes in both
 * modes.  A mask or a pair may be named any number of times; n == 0 is valid (every class is the one run h * w); masks no pair names are never
 * read.  1 <= h, w <= 32768 and h * w <= 2^30.
 * Everything is checked on the host first -- mode, the image size, the pair indices, every NAMED run list non-empty and summing to h * w,
 * counts_cap -- and refused with AMP_ERR_ARG naming the offending index, or AMP_ERR_NOMEM naming the capacity needed: nothing written and never
 * a device access.  The capacity that is always enough, and the one that is asked for, is K x (1 + the sum of len - 1 over the distinct named
 * run lists): a class changes only where a named mask does.
 * ctx == NULL: computed on the host (mask_analysis_host.hip).  Otherwise on ctx's device and stream (seg_class_map.hip): the function uploads, runs five
 * launches whatever n is, downloads and returns with the results in host memory; integer arithmetic only, the bytes do not depend on the
 * device's scheduling and equal the host's.  Memory: three bit planes of the image and the result, nothing proportional to n x h x w. */
int amp_seg_class_map(amp_ctx* ctx, const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                      const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, int n, int h, int w,
                      int mode /* 0 reduced, 1 all */, uint32_t* counts, unsigned long long counts_cap,
                      unsigned long long* counts_off /* [K + 1] */, unsigned long long* pixels /* [8] */);
/* Instances of an annotation image as COCO run lists (ampis/data_utils.py:412-428, get_ddicts 'binary' / 'label': label the foreground, one dense
 * mask per instance, encode each).  ALL POINTERS ARE HOST POINTERS.  image: h x w, row-major as numpy holds it, 1 <= h, w and h * w <= 2^30.
 * kind AMP_LABEL_BINARY: uint8, nonzero is foreground; the instances are the connected components -- connectivity 1: 4 neighbours, 2: 8
 * neighbours -- numbered 1 .. K by the row-major position of their first pixel (scipy.ndimage.label, skimage.measure.label).
 * kind AMP_LABEL_IDS: int32 ids; one instance per distinct id in ascending order, disconnected parts included; zero_is_background != 0 skips id 0
 * (connectivity is checked and not used).  Per instance i, in instance order: ids[i] (the component number or the id), boxes[4 i ..] = {r0, c0,
 * r1, c1} the tight box with exclusive ends, areas[i], and the run list counts[counts_off[i] .. + counts_len[i]) over the whole image --
 * column-major, the first count is the run of zeros and may be 0 -- exactly what amp_rle_encode gives for the instance's dense mask.
 * labels (may be NULL): the int32 h x w image, row-major, of instance number i + 1 at the pixels of instance i and 0 elsewhere.
 * inst_cap: capacity of ids / boxes / areas / counts_off / counts_len in instances; counts_cap: of counts in values.  With valid arguments
 * need[0] = the instances and need[1] = the counts are always written; with a capacity below its need the call returns AMP_ERR_NOMEM naming
 * both and writes nothing else.  Arguments are checked on the host before any device work (AMP_ERR_ARG naming the argument, nothing written).
 * ctx == NULL: computed on the host (label_runs_host.hip: run-based union-find).  Otherwise on ctx's device and stream (label_runs.hip): upload, a
 * fixed list of launches whatever the image holds, download; integer arithmetic only, the bytes do not depend on the device's scheduling and
 * equal the host's. */
enum { AMP_LABEL_BINARY = 0, AMP_LABEL_IDS = 1 };
int amp_label_runs(amp_ctx* ctx, const void* image, int h, int w, int kind, int connectivity, int zero_is_background, int* ids, int* boxes,
                   unsigned int* areas, uint32_t* counts, unsigned long long* counts_off, int* counts_len, int inst_cap,
                   unsigned long long counts_cap, int* labels, unsigned long long* need /* [2] */);
/* Instance overlays of one image from run lists (detectron2 Visualizer.overlay_instances as ampis_amd/utils/visualizer.py draws it: per instance
 * draw_binary_mask, then draw_box), every instance in draw order in one call.  image / out: uint8, row-major h x w x 3; out == image is allowed.
 * Instance i = run list pool[off[i] : off[i] + len[i]] of the h x w image (pool == NULL: no masks), fill_tab [n][256][3]: channel c of a mask
 * pixel holding v becomes fill_tab[i][v][c] (the caller tabulates its blend, so the call is lookups only); an EDGE pixel -- a mask pixel with
 * a 4-neighbour outside the mask, or in the first or last row or column of the image -- becomes edge_rgb[i] instead (edge_rgb == NULL: no
 * edges).  boxes [n][4] = {x0, y0, x1, y1} (NULL: none), 0 <= x < w and 0 <= y < h, inverted boxes allowed: after its mask, instance i sets to
 * box_rgb[i] the union of rows [y0, min(y0 + lw, h)) and [max(y1 - lw + 1, 0), y1 + 1) x cols [x0, x1 + 1), and rows [y0, y1 + 1) x cols
 * [x0, min(x0 + lw, w)) and [max(x1 - lw + 1, 0), x1 + 1); a rectangle whose stop is <= its start is empty.  A mask without a pixel draws
 * nothing; its box is drawn.
 * Everything is checked on the host first -- NULL image / out, n < 0, lw < 1, h * w > 2^30, every run list non-empty and summing to h * w,
 * the box coordinates -- and refused with AMP_ERR_ARG naming the offender: nothing written and never a device access.
 * ctx == NULL: drawn on the host (mask_analysis_host.hip).  Otherwise on ctx's device and stream (render.hip): upload, ONE launch whatever n
 * is, download; lookups and integer arithmetic only, every byte written once by the workgroup that owns its tile: the bytes do not depend
 * on the device's scheduling and equal the host's. */
int amp_render_instances(amp_ctx* ctx, const uint8_t* image, int h, int w, const uint32_t* pool, const unsigned long long* off, const int* len,
                         int n, const uint8_t* fill_tab, const uint8_t* edge_rgb, const int* boxes, const uint8_t* box_rgb, int lw, uint8_t* out);
/* Nearest-neighbour resize (+ horizontal mirror when flip) of a mask in the run-length domain: the runs of
 * flip(PIL.Image.resize(decode(cnts), (nw, nh), NEAREST)) -- what detectron2's ResizeTransform.apply_segmentation + HFlipTransform do to a bitmask
 * annotation -- without decoding (Pillow's ImagingScaleAffine pixel correspondence, restated).  cap >= nh * nw + 1 is always enough. */
int amp_rle_resize_nearest(const uint32_t* cnts, int m, int h, int w, int nh, int nw, int flip, uint32_t* out, int cap, int* m_out);
/* The same for a crop: the runs of flips(PIL.Image.resize(decode(cnts)[y0:y0+ch, x0:x0+cw], (nw, nh), NEAREST)) -- CropTransform +
 * ResizeTransform + HFlip / VFlipTransform on a bitmask annotation.  flip bit 0 mirrors left-right, bit 1 up-down. */
int amp_rle_crop_resize_nearest(const uint32_t* cnts, int m, int h, int w, int y0, int x0, int ch, int cw, int nh, int nw, int flip,
                                uint32_t* out, int cap, int* m_out);
/* Sutherland-Hodgman clip of polygons against the rectangle [x0, x1] x [y0, y1] in float64 (the region CropTransform.apply_polygons keeps; the
 * vertex order is this routine's own).  Polygon j of the call is polygon sel[j] of the pool: xy[off[sel[j]] .. off[sel[j] + 1]) flat x,y values.
 * Results go back to back into out (cap doubles; 6 * input + 16 per polygon is always enough) with out_off[nsel + 1]; a result with fewer
 * than 3 vertices or zero area is empty.  Coordinates are NOT translated. */
int amp_polygon_clip_rect(const double* xy, const long long* off, const int* sel, int nsel, double x0, double y0, double x1, double y1,
                          double* out, long long cap, long long* out_off);
int amp_rle_merge2(const uint32_t* A, int ka, const uint32_t* B, int kb, int intersect, uint32_t* out, int cap, int* m_out);
/* polygon (k vertices, flat xy) -> runs of an h x w mask (pycocotools rleFrPoly / frPyObjects) */
int amp_rle_from_polygon(const double* xy, int k, int h, int w, uint32_t* cnts, int cap, int* m_out);
/* The polygon instances of one image as run lists in one call (VIA ground truth, detectron2 PolygonMasks): instance i holds polygons
 * inst_first[i] .. inst_first[i + 1] - 1, polygon p the flat x, y values xy[poly_off[p] .. poly_off[p + 1]).  All pointers are host pointers.
 * Per instance the call returns, byte for byte, the run list of today's composition -- amp_rle_from_polygon on each of its polygons, united in
 * order with amp_rle_merge2(intersect = 0), what rle.merge(rle.frPyObjects(polygons, h, w)) encodes; that composition is the definition,
 * pycocotools' painting across column ends for a polygon that leaves the image sideways included --: counts[counts_off[i] .. + counts_len[i]),
 * column-major, the first count the run of zeros (it may be 0); boxes[4 i ..] = {r0, c0, r1, c1} the tight box of that list with exclusive
 * ends (a run across a column end covers the first and the last row; zeros for an empty mask) and areas[i] its pixels.
 * Checked on the host before any device work (AMP_ERR_ARG naming the offender, nothing written): NULL pointers, n < 0, h, w < 1, h * w > 2^30,
 * offsets that do not ascend, a polygon with an odd number of values or without a vertex, an instance without a polygon, and THE ONE DEPARTURE
 * from amp_rle_from_polygon: a coordinate that is not finite or exceeds 10^6 in magnitude is refused, because the routine's (int) casts are
 * undefined there and differ between host and device.  With valid arguments need[0] = the counts of all instances is always written; with
 * counts_cap below it the call returns AMP_ERR_NOMEM and writes nothing else.
 * ctx == NULL: computed on the host (polygon_runs_host.hip: the two routines in a loop, buffers kept across polygons).  Otherwise on ctx's
 * device and stream (polygon_runs.hip): upload, a fixed list of launches whatever the instances, polygons or crossings, download; work is
 * spread over (edge, step) items, memory is linear in vertices + crossings + counts, the double arithmetic is the host's operation for
 * operation, and the bytes do not depend on the device's scheduling and equal the host's. */
int amp_polygons_to_rle(amp_ctx* ctx, const double* xy, const unsigned long long* poly_off /* [inst_first[n] + 1], in doubles */,
                        const int* inst_first /* [n + 1] */, int n, int h, int w, uint32_t* counts, unsigned long long counts_cap,
                        unsigned long long* counts_off /* [n] */, int* counts_len /* [n] */, int* boxes /* [n][4] */, unsigned int* areas /* [n] */,
                        unsigned long long* need /* [1] */);
/* The pieces of masks: connected components per mask for the n run lists pool[off[i] : off[i] + len[i]] of one h x w image size (1 <= h, w
 * <= 32768, h * w <= 2^30) in one call, the components a rule picks flipped, the results as canonical run lists -- what
 * skimage.morphology.remove_small_objects / remove_small_holes, scipy.ndimage.binary_fill_holes and regionprops' euler_number / filled_area
 * compute on one decoded array per mask.  ALL POINTERS ARE HOST POINTERS.  connectivity k: 1 or 2.
 *   colour 1  PARTS: the components of the ones, 4 neighbours for k = 1, 8 for k = 2.  Flipped (removed): with keep_largest every part but the
 *             one of largest area (among equals the one whose first pixel col * h + row is smallest), and then every part of area < threshold.
 *   colour 0  HOLES: the components of the zeros under the dual neighbourhood (4 neighbours for k = 2, 8 for k = 1) that lie inside the mask's
 *             tight box and have no pixel in its border rows or columns; zeros that reach further are the outside, as in binary_fill_holes.
 *             Flipped (filled): every hole of area < threshold; threshold = 0xffffffff fills all.  keep_largest must be 0.
 * stats [n][4] = {components, their pixels, the largest component's pixels, the pixels flipped}; an empty mask has no component.
 * out_pool == NULL: statistics only.  Otherwise mask i's result is out_pool[out_off[i] .. + out_len[i]), the lists back to back in mask order,
 * each what amp_rle_encode gives for the dense result (the first count is the run of zeros and may be 0; with nothing flipped, the canonical
 * form of the input).  With valid arguments need[0] = the counts of all results is always written; with out_cap below it the call returns
 * AMP_ERR_NOMEM and writes nothing else.  sum(len[i] + box width of mask i + 1) always suffices: a flip removes boundaries of the input
 * and adds them only at column ends inside the tight box.  Arguments are checked on the host before any device work (AMP_ERR_ARG naming the
 * offender, nothing written): the sizes, colour, connectivity, keep_largest, NULL pointers, every run list non-empty and summing to h * w.
 * ctx == NULL: computed on the host (mask_parts_host.hip).  Otherwise on ctx's device and stream (mask_parts.hip): upload, a fixed list of
 * launches whatever n is, download; integer arithmetic only, the bytes do not depend on the device's scheduling and equal the host's. */
int amp_mask_parts(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int colour,
                   int connectivity, unsigned int threshold, int keep_largest, unsigned long long* stats /* [n][4] */, uint32_t* out_pool,
                   unsigned long long out_cap, unsigned long long* out_off /* [n] */, int* out_len /* [n] */,
                   unsigned long long* need /* [1] */);
/* Overlap-free instances: which instance a pixel belongs to, for the n run lists pool[off[i] : off[i] + len[i]] of one h x w image (1 <= h, w
 * <= 32768, h * w <= 2^30) in one call -- what users compute with a loop of decoded masks, labels[mask_i] = i + 1 in reverse priority and
 * encode(labels == i + 1) per instance.  ALL POINTERS ARE HOST POINTERS.  The OWNER of a pixel is, among the instances that cover it, the one
 * with the smallest rank[i], among equal ranks the one with the smallest index; any rank values are valid, rank == NULL means index order; a
 * pixel nothing covers has no owner.
 *   labels (may be NULL): int32 h x w, row-major as numpy holds it: owner + 1, or 0 where there is no owner.
 *   counts (may be NULL: no list is emitted, counts_cap must be 0, counts_off / counts_len / need are not used): instance i's VISIBLE list
 *     -- the pixels it owns, over the whole image -- is counts[counts_off[i] .. + counts_len[i]), the lists back to back in instance order,
 *     each exactly what amp_rle_encode gives for the dense labels == i + 1 (column-major, the first count is the run of zeros and may be 0,
 *     runs joined across column ends); an instance that owns nothing is the single run h * w.
 *   stats [n][2] = {the area of the input mask, the pixels owned}; boxes [n][4] = {r0, c0, r1, c1} the tight box of the owned pixels with
 *     exclusive ends, zeros when nothing is owned; pixels [3] = the pixels covered by no instance, by exactly one, by two or more.
 * With valid arguments and counts != NULL need[0] = the counts of all visible lists is always written; with counts_cap below it the call
 * returns AMP_ERR_NOMEM naming both and writes nothing else.  counts_cap = 2 x the sum of len[i] always suffices: the owner changes only at
 * a position where some input mask changes, such a position is a boundary of at most two visible lists, and the one further count every
 * list has is paid by its mask's own.  Arguments are checked on the host before any device work (AMP_ERR_ARG naming the
 * offender, nothing written): the sizes, n < 0, NULL pointers that are not optional, counts_cap without counts, every run list non-empty
 * and summing to h * w.  n == 0 is valid: labels all zero, pixels = {h * w, 0, 0}.
 * ctx == NULL: computed on the host (flatten_host.hip: one sweep over the sorted run ends with the set of covering instances).  Otherwise
 * on ctx's device and stream (flatten.hip): upload, a fixed list of launches whatever n is, download; no dense mask per instance, integer
 * arithmetic only, the bytes do not depend on the device's scheduling and equal the host's. */
int amp_flatten_instances(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                          const uint32_t* rank /* [n] or NULL */, int* labels /* [h][w] or NULL */, uint32_t* counts,
                          unsigned long long counts_cap, unsigned long long* counts_off /* [n] */, int* counts_len /* [n] */,
                          unsigned long long* stats /* [n][2] */, int* boxes /* [n][4] */, unsigned long long* pixels /* [3] */,
                          unsigned long long* need /* [1] */);
/* Boundary rings: the polygons of the n run lists pool[off[i] : off[i] + len[i]] of one h x w image size (1 <= h, w <= 32768, h * w <= 2^30)
 * in one call -- the way back from amp_polygons_to_rle, what users get from a contour tracer on one decoded array per mask.  ALL POINTERS ARE
 * HOST POINTERS.  Pixel (r, c) is the square [c, c + 1] x [r, r + 1]; vertices are integer pixel corners (x, y), 0 <= x <= w, 0 <= y <= h, the
 * coordinates of amp_polygons_to_rle, no half-pixel shift.  A boundary edge is a unit pixel side with a one on one side and a zero (or the
 * outside of the image) on the other, directed with the one on its right hand, y down: outer boundaries run clockwise on screen.  Following
 * successors partitions the edges into closed rings; at a saddle vertex (ones on one diagonal, zeros on the other) the walk turns left on to
 * the diagonal pixel for connectivity 2 (ones 8-connected) and right for connectivity 1.  A ring is stored as its corners only -- a saddle
 * visited twice appears twice --, starting at its smallest corner by x, then y; the rings of a mask are ordered by that corner.
 *   ring_first [n + 1]: the rings of mask i are ring_first[i] .. ring_first[i + 1] - 1; an empty mask has none.
 *   per ring r: its corners are xy[2 * ring_off[r] .. 2 * (ring_off[r] + ring_len[r])) as int32 x, y pairs, the rings back to back;
 *     ring_area2[r] = sum(x_i * y_(i+1) - x_(i+1) * y_i), positive for the outer ring of a part (twice the pixels it encloses), negative
 *     for a hole ring; ring_length[r] = the crack length, the sum of the segment lengths.
 * With valid arguments need[0] = the vertices and need[1] = the rings of all masks are always written; with xy_cap (in vertices) or ring_cap
 * below them the call returns AMP_ERR_NOMEM and writes nothing else.  Four vertices and two rings per vertical piece of ones always suffice,
 * and the pieces of a mask are at most its runs of ones plus the columns of its tight box, so xy_cap = 4 * sum(len[i] / 2 + box width of mask
 * i) and ring_cap = half of that do: a piece (a maximal vertical run of ones within one column; a run of the list is cut only at the column
 * ends it crosses) has two horizontal boundary edges that start a vertical segment, its top and its bottom side; every vertical segment
 * follows exactly one such edge, has two corners, and a ring has at least two of them.  Arguments are checked on the host before
 * any device work (AMP_ERR_ARG naming the offender, nothing written): the sizes, n < 0, connectivity, NULL pointers, every run list
 * non-empty and summing to h * w.  n == 0 is valid.
 * ctx == NULL: computed on the host (contours_host.hip: a sequential walk of the successor function).  Otherwise on ctx's device and stream
 * (contours.hip): upload, a list of launches that depends only on the largest piece count of one mask, download; no dense mask, integer
 * arithmetic only, the bytes do not depend on the device's scheduling and equal the host's. */
int amp_mask_contours(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int connectivity,
                      unsigned long long* ring_first /* [n + 1] */, unsigned long long* ring_off, int* ring_len, long long* ring_area2,
                      long long* ring_length, unsigned long long ring_cap, int* xy, unsigned long long xy_cap,
                      unsigned long long* need /* [2] */);
/* Mask morphology on run lists: the n run lists pool[off[i] : off[i] + len[i]] of one h x w image size (1 <= h, w <= 32768, h * w <= 2^30)
 * dilated, eroded, opened, closed or reduced to a boundary band in one call, without a dense mask.  ALL POINTERS ARE HOST POINTERS.  The
 * structuring element is the set of offsets (dx, dy) with |dx| <= radius and |dy| <= hh(dx):
 *   AMP_MORPH_SQUARE   hh = radius                             Chebyshev distance, the 3 x 3 ones element iterated radius times;
 *   AMP_MORPH_DIAMOND  hh = radius - |dx|                      city-block distance, the 3 x 3 cross iterated radius times;
 *   AMP_MORPH_DISK     hh = isqrt(radius^2 - dx^2)             Euclidean distance, dx^2 + dy^2 <= radius^2.
 * A piece is a maximal vertical run of ones [s, e) of one column x; it sends to every output column x + dx inside the image
 *   dilation: the rows [max(s - hh, 0), min(e + hh, h)) with weight 1; a pixel is set where the weights covering it sum to at least 1;
 *   erosion:  the rows [s + hh, e - hh), empty ones dropped; with border_value 1 an end on the image's first row (s == 0) or behind its last
 *             (e == h) is not moved.  A pixel of column x is set where the cover equals K(x): 2 * radius + 1 with border_value 0 (the outside
 *             of the image is background, a mask erodes from the image's sides), the number of columns x - dx inside the image with
 *             border_value 1 (the outside counts as mask).
 *   AMP_MORPH_OPEN = dilation of the erosion, AMP_MORPH_CLOSE = erosion of the dilation, border_value used by the erosion; AMP_MORPH_BAND_IN =
 *   the mask minus its erosion, AMP_MORPH_BAND_OUT = its dilation minus the mask (the mask's own pieces enter with weight 2^32).
 * Mask i's result is the canonical run list of the dense result, what amp_rle_encode gives (the first count may be 0), at
 * out_pool[out_off[i] : out_off[i] + out_len[i]]; boxes[i] = its tight box {r0, c0, r1, c1}, ends exclusive, as amp_polygons_to_rle reports
 * it (zeros for an empty result), areas[i] its pixels.  radius == 0 gives the canonical form of the input (an empty mask for the bands).
 * With valid arguments need[0] = the counts of all results is always written; with out_cap below it the call returns AMP_ERR_NOMEM and writes
 * nothing else.  No closed form bounds the need: a result can have more runs than its input as well as fewer; call again with need[0].
 * Checked on the host before any device work (AMP_ERR_ARG naming the offender, nothing written): the sizes, n < 0, op, shape, border_value
 * (0 or 1), radius (0 .. 1024), NULL pointers, every run list non-empty and summing to h * w, and the events of the call: summed over the
 * pieces, 2 x the output columns inside the image (one more for a band) must stay below 2^31.  The second pass of an opening or closing is
 * held to the same limit on the events it really emits, once the first pass is known.  n == 0, empty masks, full masks and zero-length
 * runs are valid.
 * ctx == NULL: computed on the host (morphology_host.hip: a sweep per mask and output column).  Otherwise on ctx's device and stream
 * (morphology.hip): upload, a fixed list of launches whatever the masks hold (twice for an opening or closing, the intermediate stays on the
 * device), download; integer arithmetic only, the bytes do not depend on the device's scheduling and equal the host's. */
enum { AMP_MORPH_DILATE = 0, AMP_MORPH_ERODE = 1, AMP_MORPH_OPEN = 2, AMP_MORPH_CLOSE = 3, AMP_MORPH_BAND_IN = 4, AMP_MORPH_BAND_OUT = 5 };
enum { AMP_MORPH_SQUARE = 0, AMP_MORPH_DIAMOND = 1, AMP_MORPH_DISK = 2 };
#define AMP_MORPH_MAX_RADIUS 1024
int amp_mask_morphology(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, int op,
                        int shape, int radius, int border_value, uint32_t* out_pool, unsigned long long out_cap,
                        unsigned long long* out_off /* [n] */, int* out_len /* [n] */, long long* boxes /* [n][4] */,
                        unsigned long long* areas /* [n] */, unsigned long long* need /* [1] */);
/* Distance maps inside masks: for the n run lists pool[off[i] : off[i] + len[i]] of one h x w image size (1 <= h, w <= 32768, h * w <= 2^30)
 * the exact squared Euclidean distance d2(p) of every pixel p of mask i to the nearest pixel that is not in mask i -- what
 * scipy.ndimage.distance_transform_edt gives, squared --, its per-mask statistics and the erosion curve, in one call, without a dense mask.
 * ALL POINTERS ARE HOST POINTERS.  border_value 0: the pixels just outside the image are background as well, as if the mask were padded by
 * one zero on every side; 1: only pixels inside the image count (scipy on the undecorated array).  A mask with no background at all
 * (border_value 1 and the full image) has d2 = AMP_DIST_NONE on every pixel; every real value is below 2^31.
 * The masks are cut into pieces, maximal vertical runs of ones of one column (amp_mask_parts' items).  For a pixel at row r of piece [s, e)
 * of its own column the column distance is g = min(r - s + 1, e - r), where with border_value 1 a side that is the image's edge (s == 0 or
 * e == h) does not count; d2(p) = min over the columns c' of (c - c')^2 + g_c'(r)^2, with g_c'(r) = 0 where (r, c') is not in the mask and
 * columns -1 and w contributing (c - c')^2 with border_value 0.  The search walks outwards from the pixel's own column and stops as soon as
 * dx^2 reaches the best value so far, so it is exact and a pixel costs about as many steps as its distance.
 *   stats[i] = {d2_max, pos, sum_d2, area}: pos = col * h + row of the pixel that attains d2_max, among equals the smallest pos (the first in
 *              column-major order); zeros for an empty mask, {AMP_DIST_NONE, 0, 0, h * w} for the mask without background;
 *   boxes[i] = the tight box {r0, c0, r1, c1}, ends exclusive, zeros for an empty mask (amp_mask_morphology's layout);
 *   curve[i][r], r = 0 .. ncurve - 1 (ncurve 0 .. AMP_MORPH_MAX_RADIUS + 1; curve == NULL requires ncurve == 0) = the pixels of mask i with
 *              d2 > r^2: curve[i][0] is the area, and with border_value 0 curve[i][r] is the area of the erosion by the disk of radius r;
 *   map (or NULL, then map_cap must be 0 and map_off and need are not used): mask i's squared distances on its tight box, row-major, 0 outside
 *              the mask, at map[map_off[i] .. + (r1 - r0) * (c1 - c0)), the crops back to back in mask order.  need[0] = the sum of the box
 *              areas is always written when map != NULL and the arguments are valid; with map_cap below it the call returns AMP_ERR_NOMEM
 *              and writes nothing else.
 * Checked on the host before any device work (AMP_ERR_ARG naming the offender, nothing written): the sizes, n < 0, border_value, ncurve,
 * NULL pointers that are not optional, map_cap without map, every run list non-empty and summing to h * w.  n == 0, empty masks, full masks
 * and zero-length runs are valid.
 * ctx == NULL: computed on the host (mask_distance_host.hip).  Otherwise on ctx's device and stream (mask_distance.hip): upload, one memset
 * and one kernel whatever the masks hold, download; integer arithmetic and integer atomics only, the bytes do not depend on the device's
 * scheduling and equal the host's.  Both paths evaluate the one walk of mask_distance.h; its work grows with the distance found:
 * O(pixels x inscribed radius) in the worst case, and nothing is refused for that reason. */
#define AMP_DIST_NONE 0xffffffffu
int amp_mask_distance(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                      int border_value, unsigned long long* stats /* [n][4] */, long long* boxes /* [n][4] */,
                      unsigned long long* curve /* [n][ncurve] or NULL */, int ncurve, uint32_t* map /* or NULL */,
                      unsigned long long map_cap, unsigned long long* map_off /* [n] */, unsigned long long* need /* [1] */);
/* Grey levels under masks: for the n run lists pool[off[i] : off[i] + len[i]] of one h x w image size (1 <= h, w <= 32768, h * w <= 2^30) and
 * one image of that size -- C order [h][w][channels], channels 1 .. 4, uint8 (depth 8) or uint16 (depth 16) -- the exact statistics of the
 * image's values on the pixels of every mask, per channel, and on request a histogram, in one call, without a dense mask -- the integers
 * behind skimage's regionprops(..., intensity_image=img) columns.  ALL POINTERS ARE HOST POINTERS.
 *   vals[i][ch] = {N, sum v, sum v^2, sum r v, sum c v, min, max, 0} over the pixels (r, c) of mask i (row and column in the full image) with
 *              v = image[r][c][ch]; N is the mask's area; eight zeros for an empty mask.  Overlapping masks do not see each other.  Every
 *              sum fits 64 bits by the limits above: sum v^2 < 2^30 * 2^32, sum r v and sum c v < 2^30 * 2^15 * 2^16.
 *   hist_shift -1: no histogram; hist, hist_cap and need are not used.  Otherwise a pixel of value v counts in bin v >> hist_shift of
 *              nbins = 2^(depth - hist_shift) bins, 1 <= nbins <= 4096 (hist_shift 0 .. 8 at depth 8, 4 .. 16 at depth 16):
 *              hist[i][ch][b], [n][channels][nbins] words.  need[0] = n * channels * nbins is always written when the arguments are valid;
 *              with hist_cap below it the call returns AMP_ERR_NOMEM and writes nothing else.
 * Checked on the host before any device work (AMP_ERR_ARG, every message begins "amp_mask_intensity: ", nothing written): the sizes, n < 0,
 * channels, depth, hist_shift and the number of bins it asks for, NULL pointers (hist and need only with a histogram), every run list
 * non-empty and summing to h * w.  n == 0, empty masks, full masks and zero-length runs are valid.
 * ctx == NULL: computed on the host (mask_intensity_host.hip: the runs cut at the column ends, the image read at stride w * channels).
 * Otherwise on ctx's device and stream (mask_intensity.hip): upload, a fill, a tile transpose of the image into one column-major plane per
 * channel -- where every run is one contiguous range --, one segmented reduction whatever the masks hold, download; integer arithmetic and
 * integer atomics only, the bytes do not depend on the device's scheduling and equal the host's. */
#define AMP_INTENSITY_NVALS 8
int amp_mask_intensity(amp_ctx* ctx, const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w,
                       const void* image /* host, C order [h][w][channels], uint8 or uint16 */, int channels /* 1..4 */, int depth /* 8 | 16 */,
                       int hist_shift /* -1: no histogram; else bin = v >> hist_shift */, unsigned long long* vals /* [n][channels][8] */,
                       uint32_t* hist /* [n][channels][nbins] or NULL */, unsigned long long hist_cap /* words */,
                       unsigned long long* need /* [1]: words hist needs */);

/* The model: DefaultPredictor(cfg) / predictor(img) ---------------------------------------------- */
typedef struct amp_model amp_model;
typedef struct amp_model_cfg {
    int num_classes;                 /* MODEL.ROI_HEADS.NUM_CLASSES */
    float pixel_mean[3], pixel_std[3];
    int pre_nms_topk, post_nms_topk; /* MODEL.RPN.{PRE,POST}_NMS_TOPK_TEST */
    float rpn_nms_thresh;            /* MODEL.RPN.NMS_THRESH */
    float score_thresh, nms_thresh;  /* MODEL.ROI_HEADS.{SCORE,NMS}_THRESH_TEST */
    int detections_per_image;        /* TEST.DETECTIONS_PER_IMAGE */
    float bbox_reg_weights[4];
    float mask_threshold;
    int max_batch, max_h, max_w;     /* capacity: largest (padded) network input */
    int max_out_hw;                  /* capacity: largest side of an output (original) image */
    size_t rle_pool_counts;          /* capacity of the RLE run pool in uint32 (0 = default) */
    /* training-mode forward (amp_model_forward_losses); train_enable = 0 skips its workspace */
    int train_enable;
    int pre_nms_topk_train, post_nms_topk_train;   /* MODEL.RPN.{PRE,POST}_NMS_TOPK_TRAIN (2000 / 1000) */
    /* The positive caps are integers: detectron2 truncates batch * fraction in double, and a float product truncates differently (100 x 0.29f
     * gives 29, the double 28; 10 x 0.7f widened to double gives 6, the double 7).  The host computes them from the fraction it was given. */
    int rpn_batch;                   /* MODEL.RPN.BATCH_SIZE_PER_IMAGE (256), in [1, 512] */
    int rpn_pos_max;                 /* int(BATCH_SIZE_PER_IMAGE * MODEL.RPN.POSITIVE_FRACTION) computed in double (128), in [0, rpn_batch] */
    float rpn_iou_lo, rpn_iou_hi;    /* MODEL.RPN.IOU_THRESHOLDS (0.3, 0.7) */
    int roi_batch;                   /* MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE (512), in [1, 2048] */
    int roi_fg_max;                  /* int(BATCH_SIZE_PER_IMAGE * MODEL.ROI_HEADS.POSITIVE_FRACTION) computed in double (128), in [0, roi_batch] */
    float roi_iou;                   /* MODEL.ROI_HEADS.IOU_THRESHOLDS (0.5): one threshold */
    int max_gt;                      /* capacity: ground-truth instances per batch */
    int max_poly_doubles;            /* capacity: polygon coordinates (doubles) per batch */
    /* backbone variant (both train): MODEL.RESNETS.{DEPTH, NUM_GROUPS, WIDTH_PER_GROUP,
     * STRIDE_IN_1X1}.  R50-FPN = 50/1/64/1 (default, also when resnet_depth == 0); X101-32x8d-FPN = 101/32/8/0. */
    int resnet_depth, num_groups, width_per_group, stride_in_1x1;
} amp_model_cfg;
/* Ground truth of one batch (all pointers HOST): instances of image b are [gt_off[b], gt_off[b+1]).  The mask of an instance is
 * EITHER polygons (flat x0,y0,x1,y1,... in input-image pixels; polygon q = poly_xy[poly_off[q] .. poly_off[q+1]); the polygons of
 * instance i are [inst_poly_off[i], inst_poly_off[i+1]), or polygon i alone when inst_poly_off is NULL) -- detectron2's
 * INPUT.MASK_FORMAT = 'polygon' -- OR a bitmask given as COCO run lengths of the instance's full-image mask at network-input
 * resolution (column-major, first run counts zeros; runs of instance i = rle_counts[rle_off[i] .. rle_off[i+1]), size rle_hw[i]) --
 * MASK_FORMAT = 'bitmask'.  An instance with runs uses them; rle_off == NULL: polygons only. */
typedef struct amp_gt {
    int B;
    const int* gt_off;
    const float* boxes;              /* [total,4] XYXY */
    const int* classes;              /* [total] in [0, num_classes) */
    const int* poly_off;             /* [polygons+1], in doubles */
    const double* poly_xy;
    const int* inst_poly_off;        /* [total+1] or NULL */
    const unsigned long long* rle_off; /* [total+1] or NULL */
    const uint32_t* rle_counts;
    const int* rle_hw;               /* [total,2] */
} amp_gt;
/* Host view of the detections of the last amp_model_infer call; pointers stay valid until the next call. */
typedef struct amp_dets {
    int B, D;                        /* images, capacity per image (detections_per_image) */
    const int* n;                    /* [B] detections per image, sorted by descending score */
    const float* boxes;              /* [B,D,4] XYXY in output-image pixels */
    const float* scores;             /* [B,D] */
    const int* classes;              /* [B,D] */
    const unsigned long long* rle_off; /* [B,D] offset of the mask's run lengths in rle_counts */
    const int* rle_len;              /* [B,D] number of runs (column-major, first run counts zeros) */
    const uint32_t* rle_counts;      /* NULL under AMP_RLE_STRINGS */
    const int* out_h; const int* out_w; /* [B] mask size */
    /* amp_model_set_rle_output(m, AMP_RLE_STRINGS | AMP_RLE_BOTH): the masks as COCO compressed-RLE "counts" strings, encoded on the
     * device -- the bytes pycocotools' mask.encode()["counts"] holds, what compress_pred stores (ampis/data_utils.py:275). NULL otherwise. */
    const char* rle_str;             /* string of detection (b, i) = rle_str[rle_str_off[b*D+i] .. + rle_str_len[b*D+i]) (no terminator) */
    const unsigned long long* rle_str_off; /* [B,D] */
    const int* rle_str_len;          /* [B,D] */
} amp_dets;
enum { AMP_RLE_COUNTS = 0, AMP_RLE_STRINGS = 1, AMP_RLE_BOTH = 2 };
/* What amp_model_infer hands back for the masks (default AMP_RLE_COUNTS: uint32 run lengths). With AMP_RLE_STRINGS the run lengths
 * never leave the device: 3-4x fewer bytes over PCIe and no host-side encoding (replaces the pycocotools call of data_utils.py:275). */
int  amp_model_set_rle_output(amp_model* m, int mode);
int  amp_model_cfg_default(amp_model_cfg* cfg);
int  amp_model_create(amp_ctx* ctx, const amp_model_cfg* cfg, amp_model** out);
/* MODEL.ANCHOR_GENERATOR.{SIZES, ASPECT_RATIOS} of p2..p6 (the fields of the same names of amp_rpn_levels): A = n_sizes[l] * n_ratios[l] anchors
 * per location, the same on every level, 1 <= A <= 9; positive finite entries.  The RPN predictors then are
 * objectness_logits [A,256,1,1] / anchor_deltas [4A,256,1,1].  A zero-initialised struct = the anchors of amp_model_create. */
typedef struct amp_anchor_cfg {
    int n_sizes[5], n_ratios[5];
    double sizes[5][9], ratios[5][9];   /* double: the cell anchors are computed from the cfg's python floats */
} amp_anchor_cfg;
int  amp_model_create_anchors(amp_ctx* ctx, const amp_model_cfg* cfg, const amp_anchor_cfg* anchors /* NULL = amp_model_create */, amp_model** out);
void amp_model_destroy(amp_model* m);
size_t amp_model_workspace_bytes(amp_model* m);
int  amp_model_num_tensors(amp_model* m);
const char* amp_model_tensor_name(amp_model* m, int i);
/* data_h: host fp32 in the torch layout of detectron2's state_dict entry `name` (conv OIHW, linear [out,in]). */
int  amp_model_load_tensor(amp_model* m, const char* name, const float* data_h, const long long* shape, int ndim);
int  amp_model_finalize(amp_model* m);
/* imgs_bgr: uint8 [B,H,W,3], device pointer (imgs_on_host = 0) or host pointer (1). out_h_h/out_w_h: host [B] original
 * image sizes the boxes/masks are rescaled to (NULL = network input size). */
int  amp_model_infer(amp_model* m, const uint8_t* imgs_bgr, int imgs_on_host, int B, int H, int W, const int* out_h_h,
                     const int* out_w_h, amp_dets* out);
/* Training-mode forward (what `model(data)` returns to LossEvalHook, ampis/data_utils.py:111-122):
 * losses_h[5] = loss_cls, loss_box_reg, loss_mask, loss_rpn_cls, loss_rpn_loc. Sub-sampling is seeded (oracle/train.py). */
int  amp_model_forward_losses(amp_model* m, const uint8_t* imgs_bgr, int imgs_on_host, int B, int H, int W, const amp_gt* gt,
                              unsigned int seed, float losses_h[5]);
/* Same forward, then the backward pass: gradients of the summed losses w.r.t. every trainable tensor land in
 * the gradient arena (same offsets as the parameters; amp_model_grad_arena exposes it for the RCCL all-reduce of row a20). */
int  amp_model_forward_backward(amp_model* m, const uint8_t* imgs_bgr, int imgs_on_host, int B, int H, int W, const amp_gt* gt,
                                unsigned int seed, float losses_h[5]);
/* The regression losses and loss weights (amp_loss_opts above) of the following amp_model_forward_losses / amp_model_forward_backward
 * calls: the five reported losses and the gradients carry the weights.  Valid on a model created with train_enable, at any time between
 * steps; a new model holds amp_loss_opts_default.  Refuses (AMP_ERR_ARG, naming the field) what amp_rpn_sample_loss_ex refuses. */
int  amp_model_set_loss_opts(amp_model* m, const amp_loss_opts* opts);
int  amp_model_get_loss_opts(amp_model* m, amp_loss_opts* opts);
int  amp_model_grad_arena(amp_model* m, float** grads_dev, size_t* nfloats);
/* How many amp_model_infer batches / training steps of this model were run a second time in AMP_CONV_F32 because a split kernel raised the
 * range flag (amp_conv_range_flag) during the call.  A model call clears the context's flag on entry, in stream order: only its own kernels
 * decide, never a flag an earlier op-level call left behind. */
int  amp_model_f32_reruns(amp_model* m, int* count);
/* the SGD momentum buffers: one arena with the parameters' offsets (like amp_model_grad_arena).  The layout depends on the model
 * configuration only (classes, backbone), not on the capacity: a host can carry it over to a re-created model or into a checkpoint. */
int  amp_model_momentum_arena(amp_model* m, float** vel_dev, size_t* nfloats);
/* torch.optim.SGD step on every trainable tensor: g' = grad_scale*g + wd*p; v = mu*v + g'; p -= lr*v */
int  amp_model_sgd_step(amp_model* m, float lr, float momentum, float weight_decay, float grad_scale);
/* The general step (amp_sgd_opts above) on every trainable tensor; a tensor is an entry of detectron2's state_dict (the two halves of a
 * fused predictor clip separately) and a bias is a name ending in ".bias".  Options that ask for nothing beyond amp_model_sgd_step --
 * AMP_CLIP_NONE, no Nesterov, bias_lr_factor == 1, weight_decay_bias == weight_decay -- run amp_model_sgd_step's own kernel: the same
 * bits at the same cost.  Otherwise three launches (gradient statistics with AMP_CLIP_NORM only, the per-tensor table, the update), no
 * host round trip, bitwise reproducible.  With a communicator it runs after the exchange, on the summed gradients times grad_scale. */
int  amp_model_sgd_step_ex(amp_model* m, const amp_sgd_opts* opts);
/* N and k of the last amp_model_sgd_step_ex with AMP_CLIP_NORM, one per trainable tensor in amp_model_tensor_name order (host arrays of
 * capacity cap; synchronises).  Both arrays NULL: only *n_out, the number of trainable tensors. */
int  amp_model_clip_stats(amp_model* m, float* norms_h, float* coefs_h, int cap, int* n_out);
/* Current value (kind 0) / gradient (1) / SGD momentum (2) of one tensor, converted back to the torch layout of detectron2's
 * state_dict entry `name` (host). */
int  amp_model_get_tensor(amp_model* m, const char* name, int kind, float* out_h, size_t capacity_floats);
/* The inverse for the momentum: the buffer of `name` in torch layout -> the momentum arena (resuming a checkpoint that stores the
 * velocity under the parameters' names, independent of this build's arena layout). */
int  amp_model_set_momentum_tensor(amp_model* m, const char* name, const float* data_h, size_t nfloats);
/* Valid (h,w) of each image of the NEXT batches inside the common frame (host [B][2]); NULL = every image fills the frame. */
int  amp_model_set_image_sizes(amp_model* m, const int* hw_h, int B);
/* Device buffer of an intermediate stage of the last infer call (parity tests): dtype 0 f32, 1 i32, 2 u64. */
int  amp_model_get_tap(amp_model* m, const char* name, void** ptr, int* dtype, int* ndim, long long shape[5]);
/* Which path a training step takes (csrc/train_plan.h), host only: no context, no model, no GPU.  inputs: 36 integers (the step's shape and
 * state, then one layer for the per-layer rules), switches: the 16 A/B switches or NULL for the process's current state, out: 21 integers;
 * the order of all three is documented at the definition in csrc/model.hip and named in tests/test_train_plan.py. */
int  amp_debug_train_plan(const int* inputs, const int* switches, int* out);

/* Several batches in flight on one GPU (serving throughput) -------------------------------------------------------------
 * An amp_pipeline runs `depth` lanes -- models the caller created on contexts of their own (own stream, workspace and result buffers),
 * normally loaded with the same weights -- from one worker thread each, so that ONE calling thread keeps `depth` batches in flight:
 * the next batch's convolutions fill the chip while the previous batch sits in its latency-bound selection / NMS / paste kernels and
 * host read-backs (+9 % images/s at depth 2 on BASELINE configs[1]; splitting one call into micro-batches does not).
 * submit() returns at once with a ticket (lanes round-robin; at most `depth` uncollected tickets), wait(ticket) blocks until that
 * batch is done and hands out its amp_dets, valid until the lane's next submit.  Host images must stay alive until wait() returns.
 * Every batch runs the same kernels in the same order as amp_model_infer: results are bit-identical to the plain call. */
typedef struct amp_pipeline amp_pipeline;
int amp_pipeline_create(amp_model* const* models, int depth, amp_pipeline** out);
int amp_pipeline_submit(amp_pipeline* p, const uint8_t* imgs_bgr, int imgs_on_host, int B, int H, int W, const int* out_h_h,
                        const int* out_w_h, long long* ticket);
int amp_pipeline_wait(amp_pipeline* p, long long ticket, amp_dets* out);
int amp_pipeline_destroy(amp_pipeline* p);       /* waits for batches in flight; the models stay the caller's */

/* Multi-GPU exchange: RCCL over xGMI, one process and one communicator per GPU ---------------------------------------
 * Replaces what the reference gets from detectron2's launch()/DDP + NCCL: the gradient all-reduce under
 * `DefaultTrainer(cfg).train()` (ampis/data_utils.py:135, notebook cell 22) and `comm.synchronize()`
 * (ampis/data_utils.py:107).  librccl is dlopen'ed by the first amp_comm_* call; nothing here needs torch.
 * Rank 0 makes the id, the host hands its AMP_COMM_ID_BYTES bytes to every rank by any side channel (a file, a TCP store,
 * torch.distributed on gloo), every rank calls amp_comm_init.  Collectives run on a stream owned by the communicator and are
 * ordered against the context's stream by HIP events. */
#define AMP_COMM_ID_BYTES 128
int amp_comm_unique_id(unsigned char* id_h /* [AMP_COMM_ID_BYTES] */);
int amp_comm_init(amp_ctx* ctx, int rank, int world, const unsigned char* id_h);
int amp_comm_destroy(amp_ctx* ctx);                                   /* also done by amp_destroy */
int amp_comm_info(amp_ctx* ctx, int* rank, int* world /* 0: no communicator */, int* rccl_version);
/* every rank's stream work so far has completed on return (host-blocking) */
int amp_barrier(amp_ctx* ctx);
/* in-place all-reduce of a device buffer, ordered after the context's stream and complete before its later work */
enum { AMP_F32 = 0, AMP_F64 = 1, AMP_I32 = 2 };
enum { AMP_SUM = 0, AMP_MAX = 1 };
int amp_allreduce(amp_ctx* ctx, void* buf, size_t count, int dtype, int op);
/* timing of the last gradient exchange: exposed_ms = from the end of the backward pass (context stream) to the end of the last
 * bucket (communication stream), 0 when the exchange finished first; span_ms = first bucket ready -> last bucket reduced */
int amp_comm_stats(amp_ctx* ctx, float* exposed_ms, float* span_ms);
/* the context's stream waits (on the device) for every collective issued so far: call it before reading the gradient arena through
 * amp_model_grad_arena after an exchange (amp_model_sgd_step and amp_model_get_tensor do it themselves); no-op without a communicator */
int amp_comm_wait(amp_ctx* ctx);
/* per bucket of the last gradient exchange: microseconds on the communication stream from "inputs ready and stream free" to
 * "reduced" (with peers: includes waiting for the slowest rank to arrive); -1 for a bucket that was not exchanged */
int amp_comm_bucket_stats(amp_ctx* ctx, float us[/* AMP_GRAD_BUCKETS */ 7]);
/* in-place broadcast of `bytes` of device memory from rank `root`, ordered after the context's stream and complete before its
 * later work (ncclBroadcast on the communication stream) */
int amp_comm_broadcast(amp_ctx* ctx, void* buf, size_t bytes, int root);

/* The gradient arena is exchanged in AMP_GRAD_BUCKETS buckets, in the order the backward pass completes them:
 * 0 mask head, 1 box head, 2 RPN head, 3 FPN, 4 res5, 5 res4, 6 res3 (stem and res2 are frozen: -1).  Host-only helpers (no
 * device call), so that the plan can be checked -- and driven over gloo -- without a GPU. */
#define AMP_GRAD_BUCKETS 7
int amp_grad_bucket_of(const char* state_dict_name);
/* tensors (bucket[t], off[t], n[t]) -> per bucket, in issue order, the merged float ranges of the arena (ranges of one bucket
 * closer than max_gap floats are joined; the gap holds padding / frozen entries whose gradient is 0) */
int amp_plan_grad_buckets(int ntensors, const int* bucket, const size_t* off, const size_t* n, size_t max_gap, int cap,
                          int* out_bucket, size_t* out_off, size_t* out_n, int* out_count);
/* the plan of this model's arena: ranges in issue order (cap >= 64 is always enough) */
int amp_model_grad_buckets(amp_model* m, int cap, int* out_bucket, size_t* out_off, size_t* out_n, int* out_count);
/* mode 1 (default once the context has a communicator): amp_model_forward_backward hands every bucket to RCCL as soon as the
 * backward pass has completed it, so that the exchange overlaps the remaining weight- and data-gradient kernels, and
 * amp_model_sgd_step waits for the last bucket on the device.  mode 0: nothing is exchanged inside forward_backward; the host
 * calls amp_model_allreduce_grads (all buckets at once) or reduces amp_model_grad_arena itself. */
int amp_model_set_grad_overlap(amp_model* m, int mode);
int amp_model_allreduce_grads(amp_model* m);            /* refused when the current gradients were already exchanged */
/* 1 when every bucket of the current gradients has been handed to RCCL (by forward_backward or by amp_model_allreduce_grads) */
int amp_model_grads_exchanged(amp_model* m, int* exchanged);
/* rank `root`'s parameters (the whole arena: weights, biases, FrozenBN scale / shift) and SGD momentum to every rank: what torch
 * DDP's constructor does under DefaultTrainer (ampis/data_utils.py:135).  Call once after loading weights / resuming.
 *
 * amp_model_forward_backward on a communicator of more than one rank is a collective: every rank must call it for every step; a
 * rank whose step fails still completes the step's RCCL sequence, and then EVERY rank returns an error for that step (the failing
 * rank its own status, the others AMP_ERR_STATE) with the gradients discarded.
 * What that covers: failures that leave the HIP runtime usable -- bad arguments, capacity / out-of-memory refusals, the f16 range flag.
 * A HIP error is sticky: the failing rank can then no longer issue its remaining buckets or join the agreement, and its peers would wait
 * in a collective nobody joins.  RCCL has no timeout of its own, so on AMP_ERR_HIP the caller must end the job (the trainer does: it
 * raises, the launcher tears the group down); the library does not try to continue on a dead device. */
int amp_model_broadcast_params(amp_model* m, int root);

#ifdef __cplusplus
}
#endif
#endif /* AMPIS_HIP_H */
