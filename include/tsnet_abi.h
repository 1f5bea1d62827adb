/*
 * tsnet_abi.h -- C ABI of the MI355X-native TS-Net generator forward path.
 *
 * The reference (nihaomiao/WACV23_TSNet) has NO plugin / operator / FFI boundary: callers
 * drive a Python object.  This header therefore defines the boundary
 * a binding for that object would use; every entry point cites the reference interface it
 * replaces.  Plain C: pointers and sizes only, no torch types.  All device pointers are
 * contiguous fp32 buffers in the caller's HIP context; `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  Work is enqueued stream-ordered and asynchronously; the
 * library never synchronises the device inside tsnet_forward*.
 *
 * Threading: one host thread per handle; handles are independent (one per GPU / process).
 * Errors: 0 = ok, negative = failure; tsnet_last_error(h) returns a message owned by the handle
 *         (tsnet_last_error(NULL) returns the message of the last failed tsnet_create).
 *
 * Additions within TSNET_ABI_VERSION 5 (new entry points only; nothing that existed changed): tsnet_face_adapt_stats,
 * tsnet_face_adapt_apply, tsnet_smooth_keypoints -- the face loader's key-point preparation of a cross-identity pair; tsnet_bank_capacity,
 * tsnet_bank_put, tsnet_forward_bank -- the source bank; tsnet_op_flow_k_slots, tsnet_op_warp_k_slots, tsnet_op_add_stats_slots,
 * tsnet_op_fuse_tail_slots -- its kernels one at a time; tsnet_forward_u8, tsnet_set_sources_u8, tsnet_forward_target_u8, tsnet_bank_put_u8,
 * tsnet_forward_bank_u8, tsnet_op_pack_input_u8, tsnet_prepare_frames_u8 -- compact (byte) inputs; tsnet_paste_frames -- generated frames
 * back into the video frames; tsnet_prepare_frames_boxes, tsnet_prepare_frames_boxes_u8, tsnet_paste_frames_boxes -- the same with a box per frame;
 * tsnet_face_labels_boxes, tsnet_face_labels_boxes_u8 -- the face labels of a clip with a crop per frame, frames of different sizes in one pass;
 * tsnet_op_upconv2d -- the decoder's up-convolution as one operator; tsnet_op_conv2d_epi -- a convolution with its epilogue's statistics, addend,
 * published maximum, device-derived operand scale and bf16 storage, as the forward calls it; tsnet_op_patch_warp, tsnet_op_train_tail -- the
 * launches of tsnet_train_extras on the caller's tensors; tsnet_gaussian_box_params, tsnet_blur_mask -- feathered paste masks; tsnet_yuv_coeffs,
 * tsnet_rgb_to_yuv420, tsnet_yuv420_to_rgb -- frames in and out as YUV 4:2:0.
 */
#ifndef TSNET_ABI_H
#define TSNET_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSNET_ABI_VERSION 5      /* 5: tsnet_op_warp_k (round 6); added since, version unchanged: tsnet_face_adapt_stats, tsnet_face_adapt_apply, tsnet_smooth_keypoints, the source bank (tsnet_bank_*, tsnet_forward_bank, tsnet_op_*_slots), compact inputs (tsnet_*_u8), tsnet_op_upconv2d, tsnet_op_conv2d_epi, tsnet_op_patch_warp, tsnet_op_train_tail, tsnet_gaussian_box_params, tsnet_blur_mask, tsnet_yuv_coeffs, tsnet_rgb_to_yuv420, tsnet_yuv420_to_rgb; 4: tsnet_cfg.operand_mode = 2 (bf16 storage); tsnet_op_conv2d kernel = 3 (Winograd-along-x form); tsnet_op_flow_k, tsnet_flow_plan */
#define TSNET_MAX_SOURCES 8

enum {
    TSNET_OK = 0,
    TSNET_ERR_ARG = -1,     /* bad argument / shape / state */
    TSNET_ERR_WEIGHT = -2,  /* unknown, missing or mis-shaped parameter */
    TSNET_ERR_HIP = -3,     /* HIP runtime failure (message carries hipGetErrorString) */
    TSNET_ERR_NOMEM = -4
};

typedef struct tsnet_engine* tsnet_handle;

/* Constructor arguments of the reference model that shape the forward graph.
 * Replaces: TSNet.__init__ (model/TSNet.py:204-228), pose extras (model/TSNet_pose.py:214-215,276-280). */
typedef struct tsnet_cfg {
    int label_nc;        /* L: label channels (2 face, 25 pose) */
    int n_blocks;        /* decoder ResnetBlocks (0 quick-start, 4 demos) */
    int n_downsampling;  /* must be 3 with ngf=64 (FuseNet width is 2*ngf*2^n_down, TSNet.py:227) */
    int n_source;        /* K <= TSNET_MAX_SOURCES */
    int ngf;             /* 64 in every reference caller; a power of two >= 8 */
    int enc_blocks;      /* img_enc ResnetBlocks (Encoder default 9, TSNet.py:53) */
    int addcoords;       /* Encoder.coord_conv on/off (TSNet.py:89-90) */
    int pose_composite;  /* 1 = TSNet_pose use_mask epilogue (TSNet_pose.py:416-417); needs H=W=256 */
    float pose_mean[3];  /* BGR mean of the pose model (TSNet_pose.py:215) */
    int height, width;   /* input frame size (256x256 in the reference) */
    int max_batch;       /* largest B a forward will be called with (workspace is sized once) */
    int operand_mode;    /* 0 = fp32-class arithmetic (default: split operands, parity 1e-3 with the fp32 reference);
                          * 1 = bf16 operands (BASELINE.json configs[2] / [4]): every convolution input and weight is rounded to bf16,
                          *     one MFMA product, fp32 accumulate, fp32 InstanceNorm / softmax / RGB head.  Own tolerance.
                          * 2 = mode 1 + bf16 STORAGE of the large convolution-to-convolution activations (the encoders' 256^2 .. 64^2 maps,
                          *     the decoder's up-convolution outputs and upsampled inputs): statistics from the fp32 accumulators, the
                          *     stored tensor rounded once, widened exactly by its consumer.
                          * 3 = fp16 operands: every convolution input and weight is scaled by a power of two (the bounds and per-layer weight
                          *     scales of mode 0) and rounded to fp16 -- 11 significant bits against bf16's 8 -- one MFMA product at the cost of
                          *     mode 1's, fp32 accumulate and fp32 storage; everything else as in mode 1.  Own tolerance. */
} tsnet_cfg;

/* tsnet_op_conv2d / tsnet_op_conv2d_cat `nprod`: ONE product on one fp16 plane rne16(operand * 2^s) -- the arithmetic of operand_mode = 3 */
#define TSNET_NPROD_F16 16

/* ---- lifecycle ---------------------------------------------------------------------------
 * tsnet_create          <- TSNet(...) construction                       (model/TSNet.py:204-264)
 * tsnet_load_weights    <- net.load_state_dict(ckpt['img_enc'|...])      (demo/demo_face.py:126-129)
 *     `name` = "<net>.<state_dict key>", nets img_enc / lbl_enc / fuse_net / dec, e.g.
 *     "img_enc.model.13.conv_block.1.weight" (OIHW fp32) or "dec.map_conv.bias".
 *     `data` may be a host or a device pointer.  Unknown names -> TSNET_ERR_WEIGHT.
 * tsnet_finalize        <- networks.init_net's net.cuda()                (model/networks.py:116)
 *     checks that every parameter was loaded, re-packs weights into the kernels' K-major
 *     layout in HBM and allocates the workspace arena.  No allocation happens after it.
 */
int tsnet_abi_version(void);
int tsnet_create(const tsnet_cfg* cfg, tsnet_handle* out);
int tsnet_load_weights(tsnet_handle h, const char* name, const float* data, const int64_t* shape, int rank);
int tsnet_finalize(tsnet_handle h, void* stream);
void tsnet_destroy(tsnet_handle h);
const char* tsnet_last_error(tsnet_handle h);

/* Number of parameters the configuration expects and their names/shapes, so a binding can
 * validate a checkpoint before loading (key schema: SURVEY.md section 8-b). */
int tsnet_num_params(tsnet_handle h);
int tsnet_param_info(tsnet_handle h, int index, const char** name, int64_t shape_out[4], int* rank);

/* Packed-weight buffer (device) for replication across GPUs: rank 0 finalizes from a checkpoint,
 * other ranks finalize from zeros and receive this buffer by one RCCL broadcast
 * (SURVEY.md section 8-e).  The reference is single-GPU only; there is no reference call site. */
int tsnet_packed_weights(tsnet_handle h, void** dev_ptr, size_t* bytes);

/* ---- forward -----------------------------------------------------------------------------
 * tsnet_forward  <- TSNet.set_test_input(...) + TSNet.forward()  (model/TSNet.py:283-294, 309-407)
 *   src_img[i]  (B,3,H,W)  source frames exactly as the reference caller passes them, i.e. BEFORE
 *                          the /255 that set_test_input applies (TSNet.py:286)
 *   src_lbl[i]  (B,L,H,W)  src_bbox[i] (B,H,W)    i < n_source
 *   tar_lbl     (B,L,H,W)  tar_bbox    (B,H,W)
 *   out_rgb     (B,3,H,W)  = self.rec_tar_img     (TSNet.py:407; pose composite TSNet_pose.py:416-417)
 *   out_flow    NULL or (K,B,H/8,W/8,2) = self.warp_grid2d_list when return_flow (TSNet.py:369-370)
 */
int tsnet_forward(tsnet_handle h,
                  const float* const* src_img, const float* const* src_lbl, const float* const* src_bbox,
                  const float* tar_lbl, const float* tar_bbox,
                  float* out_rgb, float* out_flow, int B, void* stream);

/* Per-source divisor applied to the source IMAGES on load: 255 (default; the `/255.0` of set_test_input / set_train_input,
 * TSNet.py:267,286) or 1 for a source that is a previously generated frame already in [0,1] (`use_prev`, TSNet.py:269-276).
 * div: n host floats (n <= n_source; the rest reset to 255).  Drops the clip-mode source cache. */
int tsnet_set_source_divisors(tsnet_handle h, const float* div, int n);

/* Clip mode (caller pattern demo/demo_face.py:185-192: the same K
 * sources for every driving frame).  tsnet_set_sources runs img_enc once and caches its features;
 * tsnet_forward_target then costs only lbl_enc + both branches + decoder and returns the same
 * result as tsnet_forward on the same inputs. */
int tsnet_set_sources(tsnet_handle h, const float* const* src_img, const float* const* src_lbl,
                      const float* const* src_bbox, int B, void* stream);
int tsnet_forward_target(tsnet_handle h, const float* tar_lbl, const float* tar_bbox,
                         float* out_rgb, float* out_flow, int B, void* stream);

/* Clip mode with ONE source set for every driving frame (demo/demo_face.py:185-192): src_img[i] (1,3,H,W), src_lbl[i] (1,L,H,W),
 * src_bbox[i] (1,H,W).  Afterwards tsnet_forward_target accepts any B in 1..max_batch; frame b of its result has the bits of
 * tsnet_forward on (the same sources, driving frame b).  The cache holds K encoded images (tsnet_set_sources: K*B); it is replaced
 * or dropped by tsnet_forward, tsnet_set_sources and tsnet_set_source_divisors like the per-batch cache.  tsnet_train_extras after a
 * forward on a shared source set returns TSNET_ERR_ARG (its src_img are per batch element). */
int tsnet_set_sources_shared(tsnet_handle h, const float* const* src_img, const float* const* src_lbl,
                             const float* const* src_bbox, void* stream);

/* Source bank: the layout both clip modes are special cases of.  The source-side cache is seen as tsnet_bank_capacity(h) = n_source *
 * max_batch SLOTS of one encoded source each; every driving frame of a forward names the slots it reads.
 * tsnet_bank_put encodes `count` sources of batch 1 -- src_img[i] (1,3,H,W), src_lbl[i] (1,L,H,W), src_bbox[i] (1,H,W), i < count; div: `count`
 *   HOST floats, the image divisors (what tsnet_set_source_divisors is to the caches above), NULL = 255 -- into slots first_slot ..
 *   first_slot + count - 1, at 1 / n_source of a tsnet_set_sources per slot.  The first put after tsnet_forward, tsnet_set_sources*,
 *   tsnet_set_source_divisors (they write the same buffers and drop the bank), or after none, starts an empty bank; later puts add or
 *   replace slots and leave the others as they are.  tsnet_forward_target after a put is refused: the bank is no per-batch cache.
 * tsnet_forward_bank runs B driving frames, each on Kc sources (1 <= Kc <= n_source, the means divide by Kc): slots = Kc*B HOST ints, entry
 *   s*B + b the slot of source s of frame b, read before the call returns.  A slot may repeat within a frame and across frames.  Frame b of
 *   the result has the bits of tsnet_forward at B = 1 on (the sources it names, in that order; frame b); out_flow (Kc,B,H/8,W/8,2).
 *   TSNET_ERR_ARG, with a message naming the cause: a slot outside the bank or not filled (the slot is named), Kc or B out of range, no bank.
 *   Both are stream-ordered like the calls above; a put enqueued behind a forward cannot overtake its reads.  tsnet_train_extras after
 *   a bank forward returns TSNET_ERR_ARG; tsnet_stage_ptr("src_fea") then exposes every slot (capacity images, unfilled ones undefined). */
int tsnet_bank_capacity(tsnet_handle h);
int tsnet_bank_put(tsnet_handle h, int first_slot, int count, const float* const* src_img, const float* const* src_lbl,
                   const float* const* src_bbox, const float* div, void* stream);
int tsnet_forward_bank(tsnet_handle h, const int* slots, int Kc, const float* tar_lbl, const float* tar_bbox,
                       float* out_rgb, float* out_flow, int B, void* stream);

/* Compact inputs: the same five calls on the BYTES the wide tensors are made from, one byte per value instead of four.
 *   image  (B,3,H,W) bytes, planes B, G, R: the loader's resized frame BEFORE its `- IMG_MEAN` (tsnet_prepare_frames_u8 writes it);
 *   label  (B,H,W)   bytes, class indices (what the rasterisers emit; an index >= label_nc gives an all-zero pixel, as vl2ch's comparison does);
 *   bbox   (B,H,W)   bytes, widened as (float)byte: pass 0 / 1 for the masks the wide entries take.
 * mean_bgr: 3 HOST floats, required wherever images are passed.  The stems' packing kernel widens on load with the operations the wide form went
 * through -- (float)byte is exact, `- mean` and `/ div` are the loader's and the packing kernel's own two fp32 operations, one-hot is a comparison
 * -- so every result has the BITS of the sibling call on the widened tensors.  Everything else is the sibling's: the source divisors (`div` of
 * tsnet_bank_put_u8, tsnet_set_source_divisors for the others), the cache and bank state machine, stream ordering, error codes and messages
 * (plus: null mean_bgr; label_nc > 255).  The two forms mix freely across calls: sources put as floats and driving frames as bytes share one
 * cache, and vice versa.  tsnet_set_sources_u8: shared != 0 is tsnet_set_sources_shared (B must be 1).  The masks of compact driving frames are
 * widened into an arena buffer of max_batch*H*W floats sized at tsnet_finalize: still no allocation after it.  tsnet_train_extras is unchanged. */
int tsnet_forward_u8(tsnet_handle h, const uint8_t* const* src_img, const uint8_t* const* src_lbl, const uint8_t* const* src_bbox,
                     const uint8_t* tar_lbl, const uint8_t* tar_bbox, const float* mean_bgr,
                     float* out_rgb, float* out_flow, int B, void* stream);
int tsnet_set_sources_u8(tsnet_handle h, const uint8_t* const* src_img, const uint8_t* const* src_lbl, const uint8_t* const* src_bbox,
                         const float* mean_bgr, int B, int shared, void* stream);
int tsnet_forward_target_u8(tsnet_handle h, const uint8_t* tar_lbl, const uint8_t* tar_bbox,
                            float* out_rgb, float* out_flow, int B, void* stream);
int tsnet_bank_put_u8(tsnet_handle h, int first_slot, int count, const uint8_t* const* src_img, const uint8_t* const* src_lbl,
                      const uint8_t* const* src_bbox, const float* mean_bgr, const float* div, void* stream);
int tsnet_forward_bank_u8(tsnet_handle h, const int* slots, int Kc, const uint8_t* tar_lbl, const uint8_t* tar_bbox,
                          float* out_rgb, float* out_flow, int B, void* stream);

/* Training-mode extras of the forward (model/TSNet.py:327-331, 372-390, 402-405), computed
 * from the flows and features the LAST tsnet_forward / tsnet_forward_target left in the engine -- call it right after that
 * forward, same B, same source images.  src_img: n_source x (B,3,H,W) raw (the /255 of set_train_input is applied inside);
 * tar_img (B,3,H,W) raw.  warp_src_img (n_source,B,3,H,W): every source image warped patch-wise by its flow and
 * re-normalised to the target image's statistics (warp_src_img_list); losses: 2 device floats {loss_warp, loss_align}.
 * With cfg.pose_composite (the pose model, model/TSNet_pose.py:343-346, 386-404) the warped images get the fixed-background
 * composite before the L1 (:399-402) and losses[1] is 0: that model has no alignment loss. */
int tsnet_train_extras(tsnet_handle h, const float* const* src_img, const float* tar_img, int B,
                       float* warp_src_img, float* losses, void* stream);

/* Device copies of the stage tensors of the last forward, for stage-wise parity tests
 * (NHWC fp32).  name: "src_fea" (K*B,h,w,c; n = i*B+b -- K images after a forward on a shared source set, every slot after one on a source bank), "tar_fea" (B,h,w,c), "pg", "sg" (B,h,w,c),
 * "dec_map" (B,h,w,c), "dec_up<i>" (B, h<<(i+1), w<<(i+1), c>>(i+1)): RAW output of the i-th decoder
 * up-convolution, before its InstanceNorm + ReLU.  Returns the element count through *count. */
int tsnet_stage_ptr(tsnet_handle h, const char* name, const float** dev_ptr, size_t* count);

/* Algorithmic work of one forward at batch B (multiply-accumulates, SURVEY.md section 8-d closed form). */
double tsnet_forward_macs(tsnet_handle h, int B);

/* Per-kernel-class timing of the next forward(s): when enabled the engine brackets every launch
 * class with hipEvents on the caller's stream (used by bench.py for the roofline object).
 * tsnet_timing_read returns accumulated milliseconds and launch counts per class. */
#define TSNET_TIMING_CLASSES 9
enum { TSNET_T_CONV = 0, TSNET_T_STATS = 1, TSNET_T_ELEMWISE = 2, TSNET_T_FLOW = 3, TSNET_T_WARP = 4,
       TSNET_T_PACK = 5, TSNET_T_UPSAMPLE = 6, TSNET_T_OTHER = 7,
       TSNET_T_CONV_RES = 8 /* the 3x3 convolutions of the ResnetBlocks: the dominant kernel, timed apart from TSNET_T_CONV */ };
int tsnet_timing_enable(tsnet_handle h, int on);
int tsnet_timing_read(tsnet_handle h, double ms_out[TSNET_TIMING_CLASSES], int64_t launches_out[TSNET_TIMING_CLASSES], int reset);

/* ---- single operators (NHWC fp32 device tensors), exported for op-level parity tests ------
 * These run the very kernels tsnet_forward uses.
 *
 * tsnet_op_conv2d <- nn.Conv2d (+ preceding nn.ReflectionPad2d / zero padding)  (TSNet.py:27,42,66,70,139,147,193)
 *   x (N,H,W,Cin) fp32, Cin = 8 or a multiple of 16 (pad channels with zeros); w OIHW (Cout,Cin,k,k) host or device; bias (Cout) or NULL;
 *   y (N,Ho,Wo,Cout).  ksize 1, 3 or 7; pad_mode 0 = zero, 1 = reflect.  in_alpha / in_beta (N*Cin each) or NULL: the producer's
 *   nn.InstanceNorm2d (+ nn.ReLU when in_relu) applied while the operand tile is staged, x' = max(alpha*x + beta, 0); zero padding pads x'.
 *   bound = an upper bound of |operand| after that transform (it fixes the power-of-two operand scale of the fp16 x 2 split).
 *   nprod = 3 (lo*hi, hi*lo, hi*hi), 4 (+ lo*lo; 3x3 / stride-1 patch kernel only), 1 (bf16 operands, tsnet_cfg.operand_mode = 1; `bound`
 *   is not used) or TSNET_NPROD_F16 = 16 (one fp16 plane, tsnet_cfg.operand_mode = 3: `bound` fixes the operand scale as for nprod = 3; every
 *   kernel and tile of nprod = 1 except kernel = 3, and no deep schedule 12128).
 *   kernel: 0 = the kernel the forward runs this layer on at this frame size (patch kernels of conv_h2.hpp where the output splits into
 *   4 x 32 rectangles: 3x3 / stride 1, 3x3 / stride 2 / zero pad, 7x7 stem with 8 input channels; the general implicit GEMM of conv_h2r.hpp
 *   elsewhere), 1 = the general kernel, 2 = the patch kernel (error if the layer has none), 3 = the Winograd F(2,3)-along-x form of a
 *   3x3 / stride-1 / pad-1 layer on frames of whole 4 x 32 tiles (conv_w1.hpp: the kernel the forward runs its ResnetBlock / FuseNet / first
 *   up-convolution layers on; the op packs the transformed filters itself; `tile` = tiles per workgroup, 1, 2 or 3, 0 = the launcher's choice).
 *   tile: 0 = the launcher's choice; patch 3x3 / stride 1: 32, 64, 128 (4-row tiles), 2128 (2 rows x 128), 3128 (nprod = 1 / 16 only: 4 rows x 128
 *   with the four waves side by side, the one-product modes' own tile), 20032 / 20064 (two-K-group tiles); patch 3x3 / stride 2: 64, 128 (4 rows)
 *   or 2128 (2 rows x 128: the forward's shape; 12128: its deep schedule, what a launch of at most two workgroups per CU runs); general kernel: 64 or 128 (16-deep steps, conv_h2r.hpp), 3064 / 3128 (64-deep steps,
 *   conv_g64.hpp, 64 / 128 rows: where the layer allows, the forward's choice).
 *   All one-group tiles of one kernel produce identical bits, and so do the two two-group tiles among themselves (tested); the two-group
 *   tiles, and patch vs general kernels, sum K in another association / order: agreement to fp32 rounding.  Any other kernel or tile value,
 *   or a code the layer's kernel has no tile for, returns TSNET_ERR_ARG (csrc/conv_plan.hpp decode_tile_code, plan_conv).
 * tsnet_op_upconv2d <- nn.Upsample(scale_factor=2, bilinear, align_corners=False) + nn.ReflectionPad2d(1) + nn.Conv2d(3 x 3) (TSNet.py:145-147), as the
 *   decoder runs its up-convolutions: x (N,H,W,Cin) is the LOW-resolution map, y (N,2H,2W,Cout); the other arguments are tsnet_op_conv2d's, for a
 *   3 x 3 / stride-1 / pad-1 layer with reflection padding and nprod = 3; in_alpha / in_beta / in_relu apply to x (NULL: the raw map, no ReLU).
 *   kernel: 0 = the fused form (conv_h2.hpp: the patch kernel forms the upsampled patch from a low-resolution patch while it stages it; the
 *   upsampled tensor never exists), 1 = tsnet_op_upsample2x into a scratch tensor, then tsnet_op_conv2d with the same tile -- the same bits
 *   (tested).  tile: 0, 64 or 128.  2H and 2W must split into 4 x 32 tiles.  Zero padding, another kernel size or stride, nprod != 3, or a
 *   frame / tile the fused form is not built for return TSNET_ERR_ARG on BOTH routes, with nothing launched.
 * tsnet_op_conv2d_epi <- tsnet_op_conv2d with the epilogue's optional parts (struct tsnet_conv_epi, documented at its declaration below): the addend
 *   of a split convolution, the fp64 InstanceNorm partials and alpha / beta on either finalize route, max |y| per image, the operand scale derived
 *   on the device from a published max |x|, bf16 storage of x / y.  With every part off it is tsnet_op_conv2d; with any of them on, y has the
 *   bits tsnet_op_conv2d gives on the same kernel and tile (plus the addend: one fp32 addition).
 * tsnet_op_conv2d_cat <- the same on torch.cat((x, x2), channel axis) formed on load (dec.map_conv on cat(pg, sg), TSNet.py:163):
 *   x (N,H,W,C1), x2 (x2_nmod,H,W,C2) read at image n % x2_nmod; C1 a multiple of 16.  No input transform.
 * tsnet_op_head <- the decoder's RGB head: ReflectionPad2d(3) + Conv2d(C -> 3, 7x7) + bias + Tanh (TSNet.py:151-152) on relu(alpha*x+beta),
 *   with the pose model's fixed-background composite (TSNet_pose.py:416-417: columns outside [64,192) <- bg) when composite != 0.
 *   x (N,H,W,C) NHWC, w (3,C,7,7), bias (3), bg 3 host floats or NULL; y (N,3,H,W) NCHW.  composite: bit 0 = the composite; bits 8.. = tile
 *   rows of the kernel to force (8, 16, 32; 0 = the launcher's choice by the number of workgroups: every choice gives the same bits).
 *   Bits 1-7 set, other tile rows, or forced rows with C not a multiple of 16 (the narrow head has no row tiles) return TSNET_ERR_ARG.
 * tsnet_op_instnorm_stats <- nn.InstanceNorm2d statistics (TSNet.py:53; eps 1e-5, biased variance):
 *   alpha = 1/sqrt(var+eps), beta = -mean*alpha, each (N*C).
 * tsnet_op_norm_act   : y = alpha*x+beta (relu optional) ; if resid != NULL y += resid  (ResnetBlock tail, TSNet.py:48)
 * tsnet_op_upsample2x <- nn.Upsample(scale_factor=2, bilinear, align_corners=False) (TSNet.py:145), with the
 *   producer's InstanceNorm+ReLU fused on load when alpha/beta != NULL.
 * tsnet_op_flow       <- transformation branch up to the flow field (TSNet.py:319-323,339-365):
 *   tar_fea (B,h,w,C), src_fea (B,h,w,C) un-normalised NHWC; bboxes (B,H,W); flow (B,h,w,2).
 * tsnet_op_flow_k     <- the same for K sources per driving frame, as the model's loop over sources runs it (TSNet.py:336-366): tar_fea /
 *   tar_bbox hold B images, src_fea / src_bbox / flow K*B images (image k*B + b = source k of batch element b), 1 <= K <= 8.  Maps of
 *   >= 2048 positions (configs[4]: 64 x 64) run flow_kernel_p -- a workgroup keeps its 64 target positions for all K sources.  variant: 0 =
 *   as the forward runs it; 1 = flow_kernel whatever the plan says; 2 = flow_kernel_p without its exp pass (tools library only).  repeat > 1
 *   launches the flow kernel that many times (identical results); ms_out (nullable) receives the average time of launches 2 .. repeat by
 *   HIP events (tools/flow_bench.py), 0 when repeat <= 1.
 * tsnet_op_warp       <- F.grid_sample(bilinear, zeros, align_corners=False) (TSNet.py:366) on NHWC.
 * tsnet_op_warp_k     <- the same for K sources per driving frame fused with the mean over sources (TSNet.py:366, 392/400), as the forward
 *   runs it: src_fea / flow hold K*B images (image k*B + b), out (B,h,w,C).  repeat > 1 launches the kernel that many times; ms_out
 *   (nullable) receives the average time of launches 2 .. repeat by HIP events -- the kernel ALONE (tools/warp_bench.py).
 * tsnet_op_warp_k_shared <- tsnet_op_warp_k with the forward's source-batch extent SB (B, or 1 in clip mode: one source set shared by the
 *   batch): src_fea holds K*SB images and (source k, driving frame b) reads image k*SB + b % SB; SB must divide B.  No timing arguments.
 * tsnet_op_add_stats  <- FuseNet's join (TSNet.py:195-197 split at the concat): y[n] = x[n / add_nmod * x_sb + n % add_nmod % x_sb] +
 *   add[n % add_nmod] (one fp32 addition per element) with the InstanceNorm statistics of y as tsnet_op_instnorm_stats gives them.
 *   x (N / add_nmod * x_sb, HW, C), add (add_nmod, HW, C), y (N, HW, C), alpha / beta (N*C); add_nmod divides N, x_sb divides add_nmod.
 * tsnet_op_finalize_stats <- stage 2 of the statistics alone: part (N, S, C, 2) DEVICE doubles, (sum, sum of squares) per (image, partial,
 *   channel) over HW positions in all -> alpha, beta (N*C) by the kernel the forward picks for S (in_finalize for S <= 8, in_finalize2
 *   above: what a convolution epilogue's S = tiles per image, up to 1024, goes through).
 * tsnet_op_fuse_tail  <- FuseNet's tail (TSNet.py:198-200, :400): zbar[b] = mean over k of cat(src_fea[k*SB + b % SB], tar_fea[b]) +
 *   (y2[k*B + b] * alpha + beta).  src_fea (K*SB, P, C1), tar_fea (B, P, C1), y2 (K*B, P, 2*C1), alpha / beta (K*B * 2*C1), zbar (B, P, 2*C1);
 *   1 <= K <= 8, SB divides B, C1 a multiple of 4.
 * tsnet_op_pack_input <- the stems' input assembly (set_test_input's /255 + torch.cat + coord_conv, TSNet.py:286,312,107-125): img / lbl are
 *   HOST arrays of S device pointers, img[s] (B,3,H,W) and lbl[s] (B,L,H,W) NCHW; out (S*B, H, W, Cp) NHWC holds [img / img_div[s] | lbl |
 *   xx yy rr (coords != 0: tsnet_coord_table) | zeros], image s*B + b.  nimg = 3, or 0 for the label-only form (img, img_div not read);
 *   img_div: S HOST floats (255, or 1 for a frame already in [0,1]).  Cp = 8 or a multiple of 16, at least the real channel count.
 *   amax (S*B): zeroed, then max |out| per image as float bits -- what fixes the stem's operand scale.
 * tsnet_op_pack_input_u8 <- the same assembly from compact inputs, as the tsnet_*_u8 forward entries run it: img[s] (B,3,H,W) bytes, lbl[s] (B,H,W)
 *   class-index bytes, out[.., c] = (float(byte) - mean_bgr[c]) / img_div[s] for the image channels and byte == j ? 1 : 0 for label channel j;
 *   mean_bgr: 3 HOST floats (nimg = 3).  bbox: NULL, or S device pointers to (B,H,W) mask bytes, widened to bbox_out (S*B,H,W) floats by the same
 *   launch.  The checks of tsnet_op_pack_input, and L <= 255.  out and amax carry the bits tsnet_op_pack_input gives on the widened tensors.
 * tsnet_op_upsample2x_st <- tsnet_op_upsample2x in the bf16 storage mode (tsnet_cfg.operand_mode = 2): x_bf16 / y_bf16 != 0: x / y hold bf16
 *   (widened exactly on load; the fp32 result rounded to nearest even on store).
 * tsnet_op_flow_k_slots, tsnet_op_warp_k_slots, tsnet_op_add_stats_slots, tsnet_op_fuse_tail_slots <- tsnet_op_flow_k, tsnet_op_warp_k_shared,
 *   tsnet_op_add_stats, tsnet_op_fuse_tail as a source-bank forward runs them: the source-side tensor (src_fea and, for the flow, src_bbox; x of
 *   add_stats) holds n_src images, and slots -- HOST ints, one per (source k, frame b) pair, entry k*B + b (add_stats: one per image n) -- names
 *   the image each pair reads, in place of the siblings' SB / x_sb expression.  Everything else as the sibling; a slot outside 0 .. n_src - 1
 *   returns TSNET_ERR_ARG.
 * tsnet_op_patch_warp <- the patch warp of tsnet_train_extras alone (F.unfold + F.grid_sample + F.fold, TSNet.py:373-379): src_img K HOST-listed
 *   device pointers to (B,3,H,W) raw images, div K HOST floats (255, or 1 for a frame already in [0,1]), flow (K*B, h*w, 2) with image s*B + b,
 *   out (K,B,3,H,W).  1 <= K <= 8; h divides H, w divides W, H/h = W/w.
 * tsnet_op_train_tail <- everything tsnet_train_extras does after the patch warp (TSNet.py:329-330, 381-390, 403-405), by the same launches: x
 *   (K*B,3,H*W) is re-normalised IN PLACE to the per-channel mean / unbiased std of tar_img / 255 (tar_img (B,3,H,W) raw; frame n takes target
 *   n % B), columns outside [fore_x0, fore_x1) then replaced by bg (3 HOST floats) when fore_x1 > fore_x0 (TSNet_pose.py:399-400);
 *   losses[0] = sum over sources of 10 * mean |x - tar_img / 255|, losses[1] = 1 - mean cosine similarity of the rows of pg and sg ((B*P, C), C a
 *   multiple of 4, 16-byte aligned), or 0 with pg = sg = NULL (the pose form: no cosine launch).  gen_mean, gen_std (K*B*3) and ref_mean, ref_std
 *   (B*3): NULL, or device floats that receive the statistics the image was re-normalised with.  The reductions' partials live in a scratch
 *   buffer of the call, filled with NaN first.
 * The entry points from tsnet_op_warp_k_shared on check their arguments on the host and return TSNET_ERR_ARG, with a message and nothing
 * launched, for a null tensor, a channel count that is not a multiple of 4, K outside 1..8, an extent that does not divide, a bad Cp, S < 1
 * or HW < 1; they return after the stream has drained.
 */
int tsnet_op_conv2d(const float* x, int N, int H, int W, int Cin,
                    const float* w_oihw, const float* bias, int Cout, int ksize, int stride, int pad, int pad_mode,
                    const float* in_alpha, const float* in_beta, int in_relu, float bound, int nprod, int kernel, int tile,
                    float* y, void* stream);
int tsnet_op_upconv2d(const float* x, int N, int H, int W, int Cin,
                      const float* w_oihw, const float* bias, int Cout, int ksize, int stride, int pad, int pad_mode,
                      const float* in_alpha, const float* in_beta, int in_relu, float bound, int nprod, int kernel, int tile,
                      float* y, void* stream);
/* tsnet_op_conv2d_epi: tsnet_op_conv2d as the forward calls it -- with what the convolutions' shared epilogue (csrc/conv_common.hpp conv_epilogue)
 * does beside storing y.  Every pointer of the struct is a DEVICE pointer unless it says host; a null pointer switches its part off.  The plan
 * is made first and every scratch size is checked against it before anything is launched; the call returns after the stream has drained. */
#define TSNET_CONV_EPI_INFO 8
typedef struct tsnet_conv_epi {
    int stats;                     /* 0 = no statistics; 1 = fp64 partials per (tile, channel), then the finalize launch (in_finalize2); 2 = the arrival
                                    * counters offered as the forward offers them: up to 32 tiles per image the last-arriving workgroup of an (image,
                                    * channel tile) writes alpha / beta itself, above that the finalize launch runs as for 1 */
    int repeat;                    /* >= 1 launches back to back on the same buffers; before EACH the op fills `part` with 0xFF bytes (every double a
                                    * NaN) and zeroes amax_out, on the stream */
    double* part;                  /* (N * tpi, Cout, 2): sum and sum of squares of y over the tile's positions; tpi = tiles per image of the plan */
    long long part_capacity;       /* doubles `part` holds; N * tpi * Cout * 2 are needed */
    float* alpha; float* beta;     /* out, (N * Cout) each: 1 / sqrt(var + 1e-5), -mean * alpha (tsnet_op_instnorm_stats' definition) */
    int* counters;                 /* stats = 2: 65536 ints, ZERO on entry; the finalizing workgroups leave them zero */
    int* counters_nonzero_out;     /* HOST int: counters that are not zero after the last launch has drained */
    const float* addend;           /* (add_nmod, Ho, Wo, Cout): y += addend[image % add_nmod], one fp32 addition (the shared half of a split convolution) */
    int add_nmod;                  /* must divide N */
    unsigned int* amax_out;        /* (N): float bits of max |y| of each image */
    const unsigned int* in_amax;   /* (N): float bits of max |x| per image; the operand scale of image n is derived on the device from */
    float bound_add;               /*      in_amax[n] + bound_add, and `bound` is not used (nprod = 1 has no scale: ignored) */
    int x_bf16, y_bf16;            /* bf16 storage (nprod = 1): x / y hold bf16 -- widened exactly on load; the fp32 value rounded to nearest even on
                                    * store, the statistics and amax_out still taken from the fp32 values */
    int* info_out;                 /* HOST, TSNET_CONV_EPI_INFO ints: the plan -- kernel family (csrc/conv_plan.hpp ConvFamily: 0 H2R, 1 G64, 2 H2, 3 H2S,
                                    * 4 H2S32, 5 H2D, 6 W1), tiles per image, 1 if alpha / beta were written in the kernel, conv_w1's tiles per workgroup,
                                    * 1 if its chunks may cross images, the tile's rows (patch families: rows of a rows x 32 pixel rectangle, tiles in
                                    * row-major order inside an image; general kernels: consecutive output positions of an image), its width in
                                    * channels, channel tiles */
} tsnet_conv_epi;
/* TSNET_ERR_ARG with a message, nothing of the convolution launched and y / part / alpha / beta untouched: what tsnet_op_conv2d refuses; part_capacity
 * below N * tpi * Cout * 2; stats = 2 with more than 65536 (image, 32-channel group) pairs; stats != 0 without part, alpha or beta, stats = 2 without
 * counters; add_nmod that does not divide N; repeat < 1; bf16 storage with nprod != 1; x_bf16 on a layer that runs the Winograd form or a 7 x 7 stem
 * kernel (no bf16 load is built there). */
int tsnet_op_conv2d_epi(const float* x, int N, int H, int W, int Cin,
                        const float* w_oihw, const float* bias, int Cout, int ksize, int stride, int pad, int pad_mode,
                        const float* in_alpha, const float* in_beta, int in_relu, float bound, int nprod, int kernel, int tile,
                        float* y, const tsnet_conv_epi* epi, void* stream);
int tsnet_op_conv2d_cat(const float* x, const float* x2, int N, int H, int W, int C1, int C2, int x2_nmod,
                        const float* w_oihw, const float* bias, int Cout, int ksize, int stride, int pad, int pad_mode,
                        float bound, int nprod, float* y, void* stream);
int tsnet_op_head(const float* x, int N, int H, int W, int C, const float* in_alpha, const float* in_beta,
                  const float* w_oihw, const float* bias, int composite, const float* bg, float* y, void* stream);
int tsnet_op_instnorm_stats(const float* x, int N, int HW, int C, float* alpha, float* beta, void* stream);
int tsnet_op_norm_act(const float* x, const float* alpha, const float* beta, int relu, const float* resid,
                      int N, int HW, int C, float* y, void* stream);
int tsnet_op_upsample2x(const float* x, const float* alpha, const float* beta, int relu,
                        int N, int H, int W, int C, float* y, void* stream);
int tsnet_op_flow(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                  int B, int h, int w, int C, int H, int W, float* flow, void* stream);
int tsnet_op_flow_k(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                    int B, int K, int h, int w, int C, int H, int W, float* flow, int variant, int repeat, float* ms_out, void* stream);
/* Which kernel tsnet_op_flow / tsnet_op_flow_k / the forward run on B driving frames of h x w positions, C channels: 0 = flow_kernel (a
 * workgroup per (source, batch element, 64 targets)); G >= 1 = flow_kernel_p with G workgroups per target tile (csrc/flow_warp.hpp); -1 bad
 * arguments.  Host logic only. */
int tsnet_flow_plan(int B, int h, int w, int C);
int tsnet_op_warp(const float* src_fea, const float* flow, int B, int h, int w, int C, float* out, void* stream);
int tsnet_op_warp_k(const float* src_fea, const float* flow, int B, int K, int h, int w, int C, float* out, int repeat, float* ms_out, void* stream);
int tsnet_op_warp_k_shared(const float* src_fea, const float* flow, int B, int K, int SB, int h, int w, int C, float* out, void* stream);
int tsnet_op_add_stats(const float* x, const float* add, int add_nmod, int x_sb, int N, int HW, int C,
                       float* y, float* alpha, float* beta, void* stream);
int tsnet_op_finalize_stats(const double* part, int N, int S, int C, int HW, float* alpha, float* beta, void* stream);
int tsnet_op_fuse_tail(const float* src_fea, const float* tar_fea, const float* y2, const float* alpha, const float* beta,
                       int B, int K, int SB, int P, int C1, float* zbar, void* stream);
int tsnet_op_flow_k_slots(const float* tar_fea, const float* src_fea, const float* tar_bbox, const float* src_bbox,
                          int B, int K, int h, int w, int C, int H, int W, float* flow, int variant, int repeat, float* ms_out,
                          const int* slots, int n_src, void* stream);
int tsnet_op_warp_k_slots(const float* src_fea, const float* flow, int B, int K, int h, int w, int C, float* out,
                          const int* slots, int n_src, void* stream);
int tsnet_op_add_stats_slots(const float* x, const float* add, int add_nmod, int N, int HW, int C,
                             float* y, float* alpha, float* beta, const int* slots, int n_src, void* stream);
int tsnet_op_fuse_tail_slots(const float* src_fea, const float* tar_fea, const float* y2, const float* alpha, const float* beta,
                             int B, int K, int P, int C1, float* zbar, const int* slots, int n_src, void* stream);
int tsnet_op_pack_input(const float* const* img, const float* const* lbl, int S, int B, int H, int W, int L, int nimg, int Cp, int coords,
                        const float* img_div, float* out, unsigned int* amax, void* stream);
int tsnet_op_pack_input_u8(const uint8_t* const* img, const uint8_t* const* lbl, const uint8_t* const* bbox, int S, int B, int H, int W, int L,
                           int nimg, int Cp, int coords, const float* img_div, const float* mean_bgr, float* out, float* bbox_out,
                           unsigned int* amax, void* stream);
int tsnet_op_upsample2x_st(const float* x, const float* alpha, const float* beta, int relu,
                           int N, int H, int W, int C, int x_bf16, int y_bf16, float* y, void* stream);
int tsnet_op_patch_warp(const float* const* src_img, const float* div, const float* flow, int K, int B, int H, int W, int h, int w, float* out,
                        void* stream);
int tsnet_op_train_tail(float* x, const float* tar_img, const float* pg, const float* sg, int K, int B, int H, int W, int P, int C,
                        int fore_x0, int fore_x1, const float* bg, float* gen_mean, float* gen_std, float* ref_mean, float* ref_std,
                        float* losses, void* stream);
const char* tsnet_op_last_error(void);

/* ---- demo post-processing (demo/demo_face.py:96-105,180-198 = demo/demo_pose.py:98-107,
 * 186-203).  The reference does this per frame on the host with numpy + cv2; these entry points keep the frame on the
 * device and hand back packed uint8 RGB.
 * tsnet_frame_stats      <- x.view(B,C,-1) / div, then .mean(dim=2) and .std(dim=2) (unbiased): mean, std are (B*C) floats.
 *                           div = 255 for the reference image (:180), 1 for a generated frame (:195-196).
 * tsnet_demo_postprocess <- ((rec - gen_mean) / gen_std) * ref_std + ref_mean (:197-198), then sample_img (:96-105):
 *                           + img_mean_over_255, clip to [0,1], * 255, BGR -> RGB, and the .astype('uint8') of :222.
 *                           rec (B,3,H,W) fp32; gen_mean / gen_std (B*3); ref_mean / ref_std (3) device floats;
 *                           img_mean_over_255: 3 HOST floats (IMG_MEAN / 255); out_rgb (B,H,W,3) bytes. */
int tsnet_frame_stats(const float* x, int B, int C, int HW, float div, float* mean, float* std_unbiased, void* stream);
int tsnet_demo_postprocess(const float* rec, int B, int H, int W, const float* gen_mean, const float* gen_std,
                           const float* ref_mean, const float* ref_std, const float* img_mean_over_255,
                           unsigned char* out_rgb, void* stream);

/* Input rasterisation, one call per clip.
 * tsnet_fit_face_curves <- utils/keypoint2img.py interp_points (:319-354) up to the fitted curve, HOST code: for each of the 34 pieces of
 *                      FaceDatasetTest.part_list (dataset/dataset_video_face.py:271-280, 473-477) the axis choice and scipy.optimize.curve_fit's
 *                      Levenberg-Marquardt fit (MINPACK lmdif from p0 = ones), reproduced bit for bit (csrc/lmfit.hpp).  keypoints: (F,68,2)
 *                      HOST doubles, (x, y) already relative to the crop (read_keypoints, :497-505); curves: (F,34,8) HOST doubles
 *                      {kind, a, b, c, u_first, u_last, 0, 0}, kind 0 = nothing drawn (|a| > 1), bit 1 = curve is x(y), bit 2 = quadratic.
 * tsnet_raster_face <- FaceDatasetTest.get_face_image + get_bbox_image (:466-495; interp_points' sampling + draw_edge, keypoint2img.py:298-316,
 *                      335-354).  keypoints (F,68,2) and curves (F,34,8): DEVICE doubles; edges / bbox: (F,h,w) device bytes, 0 / 255,
 *                      either may be NULL (edges needs curves, bbox needs keypoints).
 * tsnet_vl2ch       <- utils/misc.py vl2ch (:50-67): labels (B,HW) class indices as floats -> out (B,num_classes,HW) one-hot floats. */
int tsnet_fit_face_curves(const double* keypoints, int F, double* curves);
int tsnet_raster_face(const double* keypoints, const double* curves, int F, int h, int w, int bw, unsigned char* edges, unsigned char* bbox, void* stream);
int tsnet_vl2ch(const float* labels, int B, int HW, int num_classes, float* out, void* stream);

/* Key-point preparation of a cross-identity face pair (dataset/dataset_video_face.py FaceDatasetTest.__getitem__ :335, :355-379), HOST code on
 * HOST doubles, once per clip, between reading the landmarks and tsnet_fit_face_curves (csrc/face_adapt.hpp).  Every operation is the
 * reference's, in its order: the results carry the bits of its float64 arrays.
 * tsnet_face_adapt_stats <- normalize_faces(is_ref=True) (:411-441) on the SUBJECT clip.  kp (F,68,2), (x, y) relative to the clip's crop;
 *                      stats: 77 doubles = ref_dist_x[38] | ref_dist_y[38] | width.  Per landmark group of :418-424, ref_dist_x is the mean over all
 *                      frames and the group's points of |point - group centroid|, ref_dist_y the same mean of |group centroid - face centre|
 *                      (landmark 8 of the frame; counted once per point), each + 1e-3; width = max x - min x of the FIRST frame.
 * tsnet_face_adapt_apply <- normalize_faces(is_ref=False) (:411-454) on the DRIVING clip, in place.  img_scale = stats width / (max x - min x of
 *                      the driving clip's first frame); per group sx = ref_dist_x / mean_dist_x / img_scale, sy likewise with the driving clip's
 *                      own means; every point becomes (p - c) * sx + (c - fc) * sy + fc (c the group's centroid in that frame, fc the frame's
 *                      face centre before any point moved).  TSNET_ERR_ARG: F < 1, a driving (or subject) width that is zero or not finite,
 *                      key points or statistics that are not finite.
 * tsnet_smooth_keypoints <- the five-frame moving average of :357-379 over the frames of in (F,P,2), per point and coordinate, through the running
 *                      sum c: out[0] = in[0], out[1] = c[2] / 3, out[2] = c[4] / 5, out[i] = (c[i+2] - c[i-3]) / 5 for 3 <= i <= F-3,
 *                      out[F-2] = (c[F-1] - c[F-4]) / 3, out[F-1] = in[F-1].  out may be in.  TSNET_ERR_ARG: F < 5 (the reference cannot run), P < 1. */
int tsnet_face_adapt_stats(const double* kp, int F, double* stats);
int tsnet_face_adapt_apply(const double* stats, double* kp, int F);
int tsnet_smooth_keypoints(const double* in, int F, int P, double* out);

/* Pose clips (dataset/dataset_video_pose.py PoseDatasetTestVideo.get_image / get_smooth_lbl :489-536, test mode).
 * tsnet_fit_pose_curves <- interp_points (utils/keypoint2img_posenorm.py:490-516) of every stroke of connect_keypoints (:265-311), HOST code as
 *                      tsnet_fit_face_curves: pts (F,137,2) HOST doubles, flags as below; curves (F,118,8) HOST doubles (24 limb strokes, 40 finger
 *                      segments, 54 face pieces; kind 0 = dropped by the flags or a missing point).
 * tsnet_raster_pose <- utils/keypoint2img_posenorm.py connect_keypoints (:265-311; draw_edge :469-487, interp_points' sampling) followed by
 *                      crop_person_region (:538-552) and utils/misc.py im2vl (:27-47).  pts: (F,137,2) device doubles in frame coordinates =
 *                      the four arrays connect_keypoints takes, concatenated (pose 25 | face 70 | left hand 21 | right hand 21), invalid points
 *                      zero (extract_valid_keypoints, :242-262); curves (F,118,8) device doubles from tsnet_fit_pose_curves.  The skeleton is drawn on the h x w frame; labels (F, win_y1-win_y0,
 *                      win_x1-win_x0) receives the CLASS INDEX (0..24) of every pixel of the window [win_x0,win_x1) x [win_y0,win_y1) -- what
 *                      im2vl makes of the cropped colour image.  labels must be 4-byte aligned and its allocation a multiple of 4 bytes.
 *                      flags: 1 = basic_point_only, 2 = remove_face_labels.  Stroke widths are the test-mode ones (isTrain = False).
 * tsnet_label_bbox  <- PoseDatasetTestVideo.get_bbox_image (:590-607): box of the non-zero label pixels grown by h/16, w/16; 0 / 255 bytes.
 * tsnet_resize_pad  <- Image.resize(size, NEAREST) + resize_square (:425-432, :471-477): out[f, pad_top+y, pad_left+x] = in[f, ytab[y], xtab[x]],
 *                      zero elsewhere; out (F,OH,OW) floats (binarise: != 0 -> 1, the `bbox != 0` of :441, :448).  ytab / xtab: device ints, the
 *                      source row / column of every output row / column (wacv23_tsnet_amd/raster.py computes them in PIL's order). */
/* tsnet_resize_label <- np.asarray(img_as_bool(skimage.transform.resize(map, (OH, OW)))) of the face loader (dataset/dataset_video_face.py:104-106,
 *                      316-317, 397-398; scikit-image 0.18.3): in (F,h,w) device bytes (0 / 255), out (F,OH,OW) device floats 0 / 1.  Restated from
 *                      the published algorithm of that version (oracle/skimage_resize.py) -- PARITY UNPINNED: scikit-image is not available to
 *                      check it against.  wts_rows / wts_cols: HOST doubles, the anti-aliasing Gaussian of an axis that shrinks, centre first:
 *                      w[j] = exp(-0.5 j^2 / sigma^2) / sum, j = 0..lw, sigma = (in / out - 1) / 2, lw = int(4 sigma + 0.5)
 *                      (scipy.ndimage.gaussian_filter1d); lw = -1 (or sigma = 0): no pass along that axis.  Synchronises the stream. */
int tsnet_resize_label(const unsigned char* in, int F, int h, int w, int OH, int OW, const double* wts_rows, int lw_rows,
                       const double* wts_cols, int lw_cols, float* out, void* stream);
int tsnet_fit_pose_curves(const double* pts, int F, int flags, double* curves);
int tsnet_raster_pose(const double* pts, const double* curves, int F, int h, int w, int win_x0, int win_y0, int win_x1, int win_y1, int flags,
                      unsigned char* labels, void* stream);
int tsnet_label_bbox(const unsigned char* labels, int F, int h, int w, unsigned char* bbox, void* stream);
int tsnet_resize_pad(const unsigned char* in, int F, int h, int w, const int* ytab, const int* xtab, int oh, int ow,
                     int pad_top, int pad_left, int OH, int OW, int binarise, float* out, void* stream);

/* Micro-benchmark of one convolution shape on synthetic (non-zero) data: average milliseconds per launch over `iters` back-to-back
 * launches, hipEvent-timed on `stream`.  variant: -1 = the layer's own kernel and tile; else bits 0-11 tile code (tsnet_op_conv2d; with
 * bit 15 tiles per workgroup), bit 12 general kernel, bit 13 bf16 operands, bit 14 patch kernel, bit 15 Winograd form, bits 16-20 ablation
 * mask, bit 21 cold weights, bits 22-27 experiment mask (tools build), bits 28-30 XCD grid (0 the launcher's, 1 linear, 2..5 grids of
 * 1, 2, 4, 8 columns) -- csrc/conv_plan.hpp decode_bench_variant.  Diagnostic only. */
int tsnet_bench_conv(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int pad_mode, int norm,
                     int variant, int iters, float* ms_out, void* stream);

/* Launch counters since the last reset: out[0] = patch convolution kernels (conv_h2.hpp), out[1] = general convolution kernel
 * (conv_h2r.hpp), out[2] = RGB head; out[3] = tile code (rows * 1000 + width) of the last ResnetBlock-class patch convolution launched
 * (bench.py labels the roofline kernel with it).  Diagnostic. */
void tsnet_debug_counters(int64_t out[4], int reset);

/* Host-side constant tables, exported so CPU tests can pin them against torch:
 * tsnet_linspace <- torch.linspace(-1,1,n) as used by get_grid (TSNet.py:301-302);
 * tsnet_coord_table <- Encoder.coord_conv channels (xx,yy,rr) at (H,W), layout (H,W,3) (TSNet.py:107-122). */
void tsnet_linspace(int n, float* out);
void tsnet_coord_table(int H, int W, float* out);

/* Frame loading: the image side of the reference's loaders (dataset/dataset_video_face.py:318-329, 391-401: self.crop, Image.resize to 256 x 256,
 * RGB -> BGR, - mean; dataset/dataset_video_pose.py:346, 412-417, 450-457: crop, Image.resize to 128 x 256, resize_square, RGB -> BGR, - mean).
 * Image.resize's default filter is bicubic; Pillow's 8-bit resampler is integer arithmetic on coefficient tables, reproduced here byte for byte.
 * tsnet_bicubic_taps    -> the row stride of an axis' coefficient table, 2 * ceil(2 * max(n_in / n_out, 1)) + 1; negative on bad sizes.
 * tsnet_bicubic_table   <- libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc for one axis, HOST code: first[n_out], count[n_out] (the
 *                          window of every output index inside the n_in input pixels) and coef[n_out * taps] (22 fractional bits, unused taps 0).
 * tsnet_prepare_frames  <- frame.crop((x0, y0, x1, y1)).resize((ow, oh)), centred in an OH x OW canvas at (pad_top, pad_left) whose other pixels are
 *                          byte 0, channels reversed, minus mean_bgr.  frames: (F,h,w,3) device bytes, RGB interleaved; the box may leave the frame
 *                          (Image.crop: those pixels read 0).  The x tables are those of (x1 - x0 -> ow), the y tables of (y1 - y0 -> oh): DEVICE
 *                          ints; an axis that keeps its size is skipped and its tables are not read (may be NULL).  mean_bgr: 3 HOST floats.
 *                          out: (F,3,OH,OW) device floats, planes B, G, R.  One kernel on `stream`: no allocation, no synchronisation.
 *                          TSNET_ERR_ARG (nothing written): empty box, taps that are not those of the size ratio, padding that does not fit.
 * tsnet_prepare_frames_u8 <- the same kernel storing the resized BYTE: out (F,3,OH,OW) device bytes, no mean -- the compact image the tsnet_*_u8 entries
 *                          take; (float)out - mean_bgr is tsnet_prepare_frames' output, bit for bit. */
int tsnet_bicubic_taps(int n_in, int n_out);
int tsnet_bicubic_table(int n_in, int n_out, int* first, int* count, int* coef);
int tsnet_prepare_frames(const unsigned char* frames, int F, int h, int w, int x0, int y0, int x1, int y1,
                         const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                         const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                         int oh, int ow, int pad_top, int pad_left, int OH, int OW, const float* mean_bgr, float* out, void* stream);
int tsnet_prepare_frames_u8(const unsigned char* frames, int F, int h, int w, int x0, int y0, int x1, int y1,
                            const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                            const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                            int oh, int ow, int pad_top, int pad_left, int OH, int OW, unsigned char* out, void* stream);

/* The way back of tsnet_prepare_frames: the generated frames resized to the crop box they came from and put back into the full frames.  Per frame
 * f, in Pillow's terms (default bicubic filter, 8 bits per channel):
 *     g = Image.fromarray(gen[f]).crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
 *     m = None if mask is None else Image.fromarray(mask[f], "L").crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
 *     frame_f.paste(g, (x0, y0), m)               # in place
 * reproduced byte for byte, with these three behaviours of Pillow:
 *   - crop, then resize: the resampling window clamps to the source rectangle (sx0, sy0, sx1, sy1), never to the rest of gen;
 *   - clipped paste: the box may leave the frame; exactly box ∩ frame is written, destination pixel (X, Y) gets resized pixel (X - x0, Y - y0);
 *     a box entirely outside the frame writes nothing, launches nothing and returns 0;
 *   - masked paste (paste_mask_L), per byte with a = frame, b = resized gen, m = resized mask: t = b * m + a * (255 - m) + 128,
 *     out = (t + (t >> 8)) >> 8 (a at m = 0, b at m = 255).  The mask is one channel and goes through the same tables and rounding as a
 *     colour channel: the horizontal pass first, rounded to bytes, then the vertical pass.
 * gen: (F,GH,GW,3) device bytes, RGB interleaved (what tsnet_demo_postprocess writes); mask: (F,GH,GW) device bytes or NULL (plain paste);
 * frames: (F,h,w,3) device bytes, RGB interleaved, written in place.  gen and mask must NOT overlap frames (not checked).  The x tables are those
 * of (sx1 - sx0 -> x1 - x0), the y tables of (sy1 - sy0 -> y1 - y0): DEVICE ints from tsnet_bicubic_table; an axis that keeps its size is
 * skipped, its tables are not read (may be NULL) and its taps are not looked at.  One kernel on `stream` over box ∩ frame: no allocation, no
 * synchronisation.
 * TSNET_ERR_ARG (message in tsnet_op_last_error, nothing written): F < 1; gen or frames NULL; an empty box; a source rectangle that is empty or not
 * inside GH x GW; taps that are not tsnet_bicubic_taps of the axis' size pair; a missing table of an axis that is not skipped; a vertical
 * reduction too steep for the kernel's 112-row buffer (about 256 -> 9 rows and beyond). */
int tsnet_paste_frames(const unsigned char* gen, const unsigned char* mask, int F, int GH, int GW, int sx0, int sy0, int sx1, int sy1,
                       const int* xfirst, const int* xcount, const int* xcoef, int xtaps,
                       const int* yfirst, const int* ycount, const int* ycoef, int ytaps,
                       unsigned char* frames, int h, int w, int x0, int y0, int x1, int y1, void* stream);

/* A box per frame: the reference's FaceDatasetTest(fix_crop_pos=False) crops every frame by the box of its own landmarks
 * (dataset/dataset_video_face.py:303-308, 317-320, 348-353, 390-393).  The three entries are the siblings of tsnet_prepare_frames,
 * tsnet_prepare_frames_u8 and tsnet_paste_frames with the same semantics per frame -- frame f of a call has the bytes of the single-box entry
 * called on frame f alone with box f -- and with the box, and so the coefficient tables, belonging to the frame.  Fixed per call: the output
 * geometry of the prepare (oh, ow, pad_top, pad_left, OH, OW) and the source rectangle of the paste.
 *   boxes: (F, 8) ints, row f = {x0, y0, x1, y1, xoff, xtaps, yoff, ytaps}.  xoff / yoff: the offset, in ints, of that axis' table inside `pool`,
 *          where a table lies as first[n_out] | count[n_out] | coef[n_out * taps] (tsnet_bicubic_table's three outputs one after the other);
 *          xtaps / ytaps its row stride.  An axis that keeps its size is skipped: its offset (-1 by convention) and taps are not looked at.
 *          For the prepare the x table is that of (x1 - x0 -> ow), the y table of (y1 - y0 -> oh); for the paste those of
 *          (sx1 - sx0 -> x1 - x0) and (sy1 - sy0 -> y1 - y0).
 *   boxes_host / boxes_dev: the same (F, 8) ints twice.  The HOST copy is validated and sizes the grid; the DEVICE copy, which the caller
 *          uploaded, is what the kernel reads.  The device copy is trusted as the tables are: the kernel range-checks what it takes from it
 *          (pool offsets against pool_len, frame reads and paste stores against h, w), so a device copy that differs gives wrong pixels, never
 *          an access outside the tensors.
 *   pool, pool_len: DEVICE ints and their number; may be NULL / 0 when every axis of every frame is skipped.
 * One kernel on `stream` for all F frames: no allocation, no synchronisation.  The tile height is one per launch, the smallest any frame of the
 * call needs (integer arithmetic: the tile shape changes no byte).  The paste's grid covers the largest box ∩ frame of the call; a frame whose
 * box lies outside is left as it is while the others are pasted, and when every box is outside nothing is launched and 0 returned.
 * TSNET_ERR_ARG, all checked on the host copy before anything is launched, so that nothing is written for ANY frame; the message names the frame
 * ("... frame 3: ..."): an empty box, or one beyond the single-box entry's bounds; taps that are not tsnet_bicubic_taps of that frame's size
 * pair; an offset of -1 on an axis that does not keep its size; a table that ends beyond the pool; a vertical reduction too steep for the
 * 112-row buffer.  Without a frame to name: F < 1, a NULL tensor or descriptor, and the per-call geometry errors of the single-box entries. */
int tsnet_prepare_frames_boxes(const unsigned char* frames, int F, int h, int w, const int* boxes_host, const int* boxes_dev,
                               const int* pool, int pool_len, int oh, int ow, int pad_top, int pad_left, int OH, int OW,
                               const float* mean_bgr, float* out, void* stream);
int tsnet_prepare_frames_boxes_u8(const unsigned char* frames, int F, int h, int w, const int* boxes_host, const int* boxes_dev,
                                  const int* pool, int pool_len, int oh, int ow, int pad_top, int pad_left, int OH, int OW,
                                  unsigned char* out, void* stream);
int tsnet_paste_frames_boxes(const unsigned char* gen, const unsigned char* mask, int F, int GH, int GW, int sx0, int sy0, int sx1, int sy1,
                             const int* boxes_host, const int* boxes_dev, const int* pool, int pool_len,
                             unsigned char* frames, int h, int w, void* stream);

/* The face labels of a clip with a crop per frame in one pass over frames of different sizes: what tsnet_raster_face followed by
 * tsnet_resize_label (once for the edge map, once for the mask) give for frame f alone at its own crop's size, for all F frames at once --
 * the same operations per pixel in the same order, so frame f has the bits of the single-size entries.  tsnet_face_labels_boxes writes
 * float32 outputs, tsnet_face_labels_boxes_u8 bytes; both hold 0 / 1.
 *   keypoints (F,68,2) DEVICE doubles, relative to each frame's crop; curves (F,34,8) DEVICE doubles from tsnet_fit_face_curves on those points.
 *   labels, masks: (F,OH,OW) DEVICE, the class map (the resized edge map) and the resized bounding-box mask.  Either may be NULL, as in
 *          tsnet_raster_face; keypoints are needed by the mask only, curves by the class map only.
 *   bw: the brush, one per call (the reference computes it once per clip).
 *   desc: (F, 8) ints, row f = {h, w, off, lw_rows, woff_rows, lw_cols, woff_cols, 0}.  h, w: the frame's crop.  off: the byte offset of the
 *          frame's region of 4 h w bytes in the workspace.  lw_*: the half width of that axis' anti-aliasing Gaussian, -1 when the axis does
 *          not shrink (h <= OH, w <= OW: no pass), else int(4 sigma + 0.5) with sigma = (in / out - 1) / 2; woff_*: the offset, in doubles, of
 *          its lw + 1 weights (centre first, scipy's gaussian_filter1d) inside `pool`.  lw = 0 is the single weight 1.0: the pass is skipped.
 *   desc_host / desc_dev: the same (F, 8) ints twice, the convention of tsnet_prepare_frames_boxes.  The HOST copy is validated and sizes the
 *          grids; the kernels read the DEVICE copy and range-check what they take from it against workspace_len, pool_len and OH, OW: a device
 *          copy that differs gives wrong pixels (an unusable row an all-zero frame), never an access outside the tensors.
 *   pool, pool_len: DEVICE doubles and their number; may be NULL / 0 when no axis of any frame has lw >= 0.
 *   workspace, workspace_len: DEVICE bytes, 4-byte aligned, the caller's; contents need not be initialised and are not kept between calls.
 *          [0, 16 F): the 2F {min, max} int pairs of the images; frame f's region at off_f: edge map A | mask A | edge map B | mask B of
 *          h w bytes each (the rasteriser draws into A, the two Gaussian passes go A -> B -> A).  Regions may lie anywhere behind the pairs.
 * At most six kernels on `stream` whatever F and however many sizes (fill, edges, rows pass, columns pass, min / max, resize; a pass that no
 * frame takes is not launched): no allocation, no memset, no copy, no synchronisation.
 * TSNET_ERR_ARG, all checked on the host copy before anything is enqueued, so that nothing is written for ANY frame.  Without a frame to name:
 * F < 1 or 2 F > 65535 (the grid's y); both outputs NULL, or a NULL input that an output needs, NULL descriptors or workspace; bw < 1;
 * OH or OW < 1; a workspace that is misaligned or shorter than the pairs.  Naming the frame ("... frame 3: ..."): h or w < 1 (or > 32767);
 * lw outside -1 .. 63; lw >= 0 on an axis that does not shrink, or lw that is not int(4 sigma + 0.5) of that size pair; a half-kernel that
 * ends beyond the pool; a region that overlaps the pairs or another frame's region, or ends beyond the workspace. */
int tsnet_face_labels_boxes(const double* keypoints, const double* curves, int F, const int* desc_host, const int* desc_dev,
                            const double* pool, int pool_len, int bw, void* workspace, long long workspace_len, int OH, int OW,
                            float* labels, float* masks, void* stream);
int tsnet_face_labels_boxes_u8(const double* keypoints, const double* curves, int F, const int* desc_host, const int* desc_dev,
                               const double* pool, int pool_len, int bw, void* workspace, long long workspace_len, int OH, int OW,
                               unsigned char* labels, unsigned char* masks, void* stream);

/* Feathered paste masks: Image.filter(ImageFilter.GaussianBlur(r)) of Pillow on "L" images, byte for byte (csrc/mask_blur.hpp).  Pillow's
 * Gaussian blur is three passes of an extended box blur per axis in 32-bit integers, each pass rounded to bytes, rows first, then columns.
 *
 * tsnet_gaussian_box_params: HOST only.  The constants of one axis for a blur radius: with s2 = radius^2 / passes, L = sqrt(12 s2 + 1),
 * l = floor((L - 1) / 2), a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)) and R = l + a, all in FLOAT arithmetic (doubles only inside
 * sqrt and floor, as C promotes them; double arithmetic throughout gives other bytes, e.g. at radius 1 and 0.3):
 *     *box_radius = (int)R;  *ww = (unsigned)((float)(1 << 24) / (R * 2 + 1));  *fw = ((1 << 24) - (2 * box_radius + 1) * ww) / 2
 * One pass along a line in[0 .. n), clamp replicating the end pixels:
 *     out[x] = (acc * ww + far * fw + (1 << 23)) >> 24,  acc = sum of in[clamp(x + d)] over |d| <= box_radius,
 *     far = in[clamp(x - box_radius - 1)] + in[clamp(x + box_radius + 1)].
 * Pillow's GaussianBlur has passes = 3.  A pixel farther than 3 (box_radius + 1) from every non-zero pixel is exactly 0 after the three passes.
 * TSNET_ERR_ARG: a negative or non-finite radius (or one whose box radius is beyond 1e9), passes < 1, a NULL output.
 *
 * tsnet_blur_mask: out = GaussianBlur((radius_x, radius_y)) of every frame of `in`, (F,H,W) DEVICE bytes.  An axis whose radius is 0 is
 * skipped; both 0 is a copy.
 *   in == NULL: the source is the indicator of rect = HOST ints {x0, y0, x1, y1}, inside the image and not empty -- 255 inside, 0 outside, the
 *          same for all F frames; no input is read.  With an input, rect is not looked at (may be NULL).
 *   flags: bit 0 -- every non-zero input byte counts as 255 (0 / 1 masks go in as they are); bits 8-15 -- route selector, 0 = the library's
 *          choice, 1 = the rows kernel then the columns kernel (the only route there is); every other bit must be 0.
 *   tmp:   F * H * W DEVICE bytes of the caller's, the rows' result on its way to the columns; contents are not kept.
 *   out:   (F,H,W) DEVICE bytes; it must be neither in nor tmp (overlaps beyond the first byte are not checked).
 * At most two kernels on `stream` (one when an axis is skipped): no allocation, no memset, no synchronisation.
 * TSNET_ERR_ARG (message in tsnet_op_last_error; every refusal comes before the first launch, nothing is written): out or tmp NULL; in and rect
 * both NULL; F, H or W < 1 (or F > 65535); H or W over 512, the longest line the kernels' tile holds (kMbMaxSide, named in the message); a
 * radius that is negative, not a number or over 4096; an empty rectangle or one not inside the image; unknown flag bits or route; out == in or
 * out == tmp. */
int tsnet_gaussian_box_params(float radius, int passes, int* box_radius, unsigned* ww, unsigned* fw);
int tsnet_blur_mask(const unsigned char* in, int F, int H, int W, const int* rect, float radius_x, float radius_y, int flags,
                    unsigned char* out, unsigned char* tmp, void* stream);

/* Video in and out as YUV 4:2:0 (csrc/yuv_frames.hpp): packed RGB bytes <-> planar 8-bit Y'CbCr with the chroma planes at half size in both
 * directions, 1.5 bytes per pixel.  The contract is INTEGER arithmetic; tests/yuv_cases.py restates it in numpy and the tests hold equality.
 * A conversion is fixed by a standard -- 601: BT.601, Kr = 0.299, Kb = 0.114; 709: BT.709, Kr = 0.2126, Kb = 0.0722; Kg = 1 - Kr - Kb -- and
 * a range: full (JFIF, ITU-T T.871): sy = sc = 1, Y offset 0; limited: sy = 219/255, sc = 224/255, Y offset 16.  The chroma offset is 128.
 *
 * tsnet_yuv_coeffs: HOST only, computed in double.  The rows of the real matrix are Y = sy (Kr, Kg, Kb), Cb = sc (-Kr, -Kg, 1 - Kb) /
 * (2 (1 - Kb)), Cr = sc (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)); every entry times 65536, rounded to nearest; then the GREEN entry of each row is
 * corrected so that the Y row sums to round(65536 sy) and the chroma rows to 0: a grey pixel has chroma exactly 128.
 *   fwd[12]: the rows Y, Cb, Cr as {cR, cG, cB, offset}.
 *   inv[6]:  {iy, rv, gu, gv, bu, oy}: iy = round(65536 / sy), rv = round(65536 * 2 (1 - Kr) / sc), bu = round(65536 * 2 (1 - Kb) / sc),
 *            gu = -round(65536 Kb 2 (1 - Kb) / (Kg sc)), gv = -round(65536 Kr 2 (1 - Kr) / (Kg sc)), oy = the Y offset.
 * (601 full: Y row 19595, 38470, 7471 -- libjpeg's.)  TSNET_ERR_ARG: a standard other than 601 or 709, a NULL table.
 *
 * Layouts.  A frame of h x w pixels is h w + 2 ch cw bytes with ch = (h + 1) / 2, cw = (w + 1) / 2; frames are contiguous (no stride, no pitch).
 *   0 = I420: the Y plane, then the Cb plane, then the Cr plane (a Y4M frame's payload);
 *   1 = NV12: the Y plane, then ch rows of cw interleaved (Cb, Cr) pairs (hardware encoders and decoders).
 *
 * tsnet_rgb_to_yuv420: rgb (F,h,w,3) DEVICE bytes -> yuv, F frames, DEVICE; fwd: 12 HOST ints.
 *   Y[y][x] = clamp((cR R + cG G + cB B + (off << 16) + 32768) >> 16, 0, 255) with the Y row;
 *   the chroma sample (j, i) covers the n = 4, 2 or 1 pixels of the 2 x 2 block at (2j, 2i) that lie inside the frame; with S the sum over them of
 *   cR R + cG G + cB B (that plane's row): C = clamp((S (4 / n) + (off << 18) + (1 << 17)) >> 18, 0, 255) -- one rounding of the block's mean
 *   chroma, centred (JPEG) siting.  >> is arithmetic.
 * tsnet_yuv420_to_rgb: the inverse; inv: 6 HOST ints.  The chroma of pixel (y, x) is the sample at (y >> 1, x >> 1), replicated; with
 *   t = (Y - oy) iy, u = Cb - 128, v = Cr - 128:  R = clamp((t + rv v + 32768) >> 16), G = clamp((t + gu u + gv v + 32768) >> 16),
 *   B = clamp((t + bu u + 32768) >> 16).
 * Each is ONE kernel on `stream` for all F frames: no allocation, no memset, no synchronisation.  A lane moves a block of 8 x 2 pixels with 8- or
 * 4-byte accesses where the block is whole and its rows are aligned, byte by byte on ragged edges and unaligned rows; the bytes are the same.
 * TSNET_ERR_ARG (message in tsnet_op_last_error starting with the entry's name less "tsnet_"; every refusal comes before the launch, nothing is
 * written): a NULL tensor or table; F, h or w < 1; F over 65535 (kYuvMaxFrames, the grid); a frame over 2^31 - 1 RGB bytes (h w 3, the 32-bit
 * index inside a frame); a layout other than 0 or 1; yuv == rgb (overlaps beyond the first byte are not checked); a forward table with a row
 * whose sum of |c| is over 1 << 17 (kYuvRowSumMax) or an inverse table with an entry over 1 << 21 in size (kYuvInvCoefMax) -- beyond them the
 * sums may overflow 32 bits; a table offset outside 0 .. 255. */
int tsnet_yuv_coeffs(int standard, int full_range, int* fwd, int* inv);
int tsnet_rgb_to_yuv420(const unsigned char* rgb, int F, int h, int w, const int* fwd, int layout, unsigned char* yuv, void* stream);
int tsnet_yuv420_to_rgb(const unsigned char* yuv, int F, int h, int w, const int* inv, int layout, unsigned char* rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSNET_ABI_H */
