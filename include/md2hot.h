/*
 * md2hot.h — C ABI of the MI355X (gfx950) monodepth2 photometric hot path.
 *
 * One fused operator replaces the body of
 *   Trainer.generate_images_pred   /root/reference/trainer.py:341-391
 *   Trainer.compute_losses         /root/reference/trainer.py:407-496
 *   (+ compute_reprojection_loss   trainer.py:393-405, and the layers.py
 *    primitives they call: disp_to_depth 16-25, BackprojectDepth 139-168,
 *    Project3D 171-193, get_smooth_loss 202-215, SSIM 218-248)
 * and the autograd backward of all of it (dL/ddisp_s for every scale and
 * dL/dcam_T_cam for every source frame).
 *
 * The reference exposes no FFI: its boundary is the two Python methods above.
 * This header is what the Python host side (monodepth2_amd/_lib.py, ctypes)
 * binds; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every tensor is fp32 (disparities: fp32 or bf16, md2_desc.disp_dtype),
 *    contiguous NCHW, device memory owned by the caller
 *    (PyTorch's caching allocator).  The library never allocates outside
 *    md2_aug_plan_create: scratch lives in `workspace` (md2_workspace_bytes) and
 *    must be the SAME buffer for a forward and its backward (the forward leaves
 *    per-image statistics there).
 *  - Work is enqueued on `stream` (a hipStream_t); no host synchronisation, no
 *    device malloc, so every call except md2_aug_run (host-staged parameters) is
 *    hipGraph-capturable.
 *  - Return 0 on success, a negative code otherwise; md2_last_error() then
 *    describes the failure (thread-local).  Nothing in the library aborts.
 *  - Results are deterministic: every reduction is a fixed-order tree.
 */
#ifndef MD2HOT_H
#define MD2HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MD2_ABI_VERSION 24
#define MD2_MAX_SCALES 4
#define MD2_MAX_SRC 3

#define MD2_OK 0
#define MD2_ERR_ARG (-1)
#define MD2_ERR_HIP (-2)

/* opt.* switches of the reference (options.py:104-118) */
#define MD2_NO_SSIM          (1u << 0) /* --no_ssim             trainer.py:399-403      */
#define MD2_AVG_REPROJECTION (1u << 1) /* --avg_reprojection    trainer.py:441-442,461  */
#define MD2_NO_AUTOMASK      (1u << 2) /* --disable_automasking trainer.py:432,466,480  */
#define MD2_V1_MULTISCALE    (1u << 3) /* --v1_multiscale       trainer.py:347-352,417  */
#define MD2_T_PER_SCALE      (1u << 4) /* a cam_T_cam per scale (posecnn, trainer.py:366-375) */
#define MD2_PREDICTIVE_MASK  (1u << 5) /* --predictive_mask     trainer.py:447-459 (needs NO_AUTOMASK) */

/* md2_desc.disp_dtype: the disparities (and the gradients written for them) as fp32,
 * or bf16 as the depth decoder emits them under bf16 autocast (config C5), read as is */
#define MD2_DTYPE_F32  0u
#define MD2_DTYPE_BF16 1u

typedef struct md2_desc {
    int32_t batch;               /* B: images per rank (opt.batch_size)                  */
    int32_t height, width;       /* opt.height / opt.width (full resolution)             */
    int32_t num_src;             /* S = len(frame_ids) - 1, 1..3                          */
    int32_t num_scales;          /* len(opt.scales) (scales are 0..num_scales-1), 1..4   */
    uint32_t flags;              /* MD2_* above                                          */
    float min_depth, max_depth;  /* opt.min_depth / opt.max_depth                        */
    float disparity_smoothness;  /* opt.disparity_smoothness                             */
    uint32_t disp_dtype;         /* MD2_DTYPE_*: element type of disp[] and grad_disp[]  */
    uint64_t seed;               /* tie-break noise seed when tensors.noise == NULL      */
} md2_desc;

/*
 * Operands.  "loss resolution" of scale s is (H, W) normally and
 * (H>>s, W>>s) with MD2_V1_MULTISCALE (trainer.py:347-352).
 */
typedef struct md2_tensors {
    /* outputs[("disp", s)]: (B,1,H>>s,W>>s) */
    const float* disp[MD2_MAX_SCALES];
    /* inputs[("color", frame, s)]: (B,3,H>>s,W>>s); frame 0 = target (frame_ids[0]),
     * frames 1..S = frame_ids[1:].  Targets are read at every scale (smoothness,
     * trainer.py:423,488); sources only at the loss resolution of each scale. */
    const float* color[MD2_MAX_SCALES][1 + MD2_MAX_SRC];
    /* inputs[("K", s)] / inputs[("inv_K", s)]: (B,4,4); only [0] unless V1_MULTISCALE */
    const float* K[MD2_MAX_SCALES];
    const float* inv_K[MD2_MAX_SCALES];
    /* cam_T_cam per source frame, stacked: (S,B,4,4); with MD2_T_PER_SCALE
     * (num_scales,S,B,4,4).  The stereo frame passes inputs["stereo_T"]. */
    const float* T;
    /* Optional unit-normal tie-break noise (trainer.py:468), per scale packed
     * back to back, scale s shaped (B, C, h_s, w_s) with C = S (or 1 with
     * AVG_REPROJECTION) at the loss resolution.  NULL: drawn in-kernel from seed. */
    const float* noise;
    /* Optional device-side uint64 mixed into desc.seed at run time, so a captured
     * hipGraph draws fresh noise on every replay (the caller increments it). */
    const uint64_t* seed_ptr;
    /* MD2_PREDICTIVE_MASK: outputs["predictive_mask"][("disp", s)] upsampled to the
     * loss resolution (trainer.py:449-453), per scale packed back to back, scale s
     * shaped (B, S, h_s, w_s).  Multiplies each frame's reprojection loss. */
    const float* mask;
    /* Optional (ABI 20): the source frames' scale-0 colours as 8-bit RGBx dwords,
     * (S, B, H, W) uint32, byte c of a pixel = k with color[0][1+f][b][c][y][x] == k/255
     * exactly — what the loader's to_tensor makes of 8-bit images (mono_dataset.py:
     * 199-200), e.g. written by md2_aug_run2 as it decodes them.  NULL: the forward
     * packs them from the fp32 planes itself and checks every colour (pack_src8).  The
     * forward and the backward must see the same value. */
    const uint32_t* src8;
} md2_tensors;

int md2_abi_version(void);
const char* md2_last_error(void);
/* Hash of the sources the library was built from (monodepth2_amd/build.py
 * source_hash(): every .hip source, the headers, the flags and the target), so the
 * Python binding can refuse a prebuilt library that is stale for the tree. */
const char* md2_build_id(void);

/* Scratch needed by one forward + backward pair (bytes, 256-B aligned). */
size_t md2_workspace_bytes(const md2_desc* desc);

/* Bytes of the per-pixel selection map the forward writes (one uint8 per
 * loss-resolution pixel per scale, scales packed back to back). */
size_t md2_select_bytes(const md2_desc* desc);

/*
 * Forward.  Writes loss_out[0..num_scales-1] = losses["loss/s"] and
 * loss_out[num_scales] = losses["loss"] (trainer.py:492-495), and select_out:
 * per pixel the argmin index into torch.cat((identity, reprojection), 1)
 * (trainer.py:471-478); identity_selection = select > (C-1) (trainer.py:481).
 */
int md2_photometric_fwd(const md2_desc* desc, const md2_tensors* t,
                        float* loss_out, uint8_t* select_out,
                        void* workspace, void* stream);

/*
 * Backward.  grad_loss: device (num_scales+1) upstream gradients of loss_out.
 * Writes (overwrites) grad_disp[s] shaped like disp[s], and grad_T shaped like
 * T, and with MD2_PREDICTIVE_MASK grad_mask shaped like tensors.mask (dL/dmask
 * through trainer.py:455; the BCE term of 457-459 is the caller's).  select and
 * workspace must come from the matching forward.
 */
int md2_photometric_bwd(const md2_desc* desc, const md2_tensors* t,
                        const float* grad_loss, const uint8_t* select,
                        float* const* grad_disp, float* grad_T, float* grad_mask,
                        void* workspace, void* stream);

/*
 * Materialise what generate_images_pred stores in `outputs` (trainer.py:356,
 * 382, 384-387) for logging / evaluation steps.  Any pointer may be NULL.
 *   depth_out[s]          (B,1,h_s,w_s)           outputs[("depth", 0, s)]
 *   sample_out[s*S + f]   (B,h_s,w_s,2)           outputs[("sample", frame, s)]
 *   color_out[s*S + f]    (B,3,h_s,w_s)           outputs[("color", frame, s)]
 */
int md2_generate_images(const md2_desc* desc, const md2_tensors* t,
                        float* const* depth_out, float* const* sample_out,
                        float* const* color_out, void* stream);

/*
 * The tie-break noise the forward draws in-kernel when tensors.noise is NULL
 * (trainer.py:468, unit normal before the 1e-5 scale), for scale s: writes
 * (B, C, h_s, w_s) with C = S (or 1 with AVG_REPROJECTION) at the loss resolution.
 * seed_ptr: the same optional device seed the forward takes.  Lets tests hand the exact draw of a
 * seeded forward to the CPU oracle.
 */
int md2_tiebreak_noise(const md2_desc* desc, const uint64_t* seed_ptr, int scale,
                       float* out, void* stream);

/*
 * Optional kernel timing for benchmarks: between md2_timing_begin and
 * md2_timing_end every launch of the photometric kernels (the forward's three
 * launches — identity, reprojection, combine — as one interval, and the backward
 * photo kernel; they dominate the hot path) is launched with hipExtLaunchKernelGGL,
 * which stamps a start/stop hipEvent pair on the kernel dispatches themselves (v1_multiscale's per-scale launches are not timed).
 * md2_timing_end waits
 * for the last event and returns the summed durations (ms) and launch counts.
 * Not for use under graph capture (events are recorded eagerly).
 */
int md2_timing_begin(int max_launches);
int md2_timing_end(double* fwd_ms, int* n_fwd, double* bwd_ms, int* n_bwd);
/* After md2_timing_end: the summed durations of whole md2_photometric_fwd calls (first
 * kernel's start to the finalize kernel's end) and md2_photometric_bwd calls (photo_bwd
 * start to grad_T end) in that window — every kernel of the hot path, for its roofline.
 * Each whole call takes a slot of max_launches besides its kernel slot. */
int md2_timing_calls(double* fwd_ms, int* n_fwd, double* bwd_ms, int* n_bwd);

/*
 * DepthDecoder block fusion: the input of every decoder
 * conv — ReflectionPad2d(1) (layers.py:127-135) of [ELU(previous conv output)
 * (layers.py:113-118), nearest x2 upsampled (layers.py:196-199), concatenated with
 * the encoder skip feature (networks/depth_decoder.py:55-58)] — in one pass, and its
 * adjoint in one pass.  x: (B,C,h,w); skip: (B,Cs,H,W) with (H,W) = (2h,2w) if
 * MD2_PAD_UPSAMPLE else (h,w); out: (B,C+Cs,H+2,W+2).  With MD2_PAD_ELU x is the
 * pre-activation and the backward needs it again.  Returns MD2_OK / MD2_ERR_*.
 */
#define MD2_PAD_ELU      (1u << 0)
#define MD2_PAD_UPSAMPLE (1u << 1)
#define MD2_PAD_NHWC     (1u << 2)   /* x, skip, out (and their grads) channels_last */
#define MD2_PAD_BF16     (1u << 3)   /* bf16 tensors (needs NHWC, channels multiples of 4) */

typedef struct md2_pad_desc {
    int32_t batch, channels, height, width; /* of x */
    int32_t skip_channels;                  /* 0: no skip tensor */
    uint32_t flags;                         /* MD2_PAD_* */
} md2_pad_desc;

/* bias (nullable, (C,) fp32): the bias of the conv that produced x, added here
 * before the ELU so the conv runs without one (no separate bias-add pass); the
 * backward then also returns grad_bias = the fixed-order sum of grad_x over
 * (B, h, w), with `workspace` of md2_decoder_pad_workspace_bytes.  NHWC with
 * channels a multiple of 4 dividing 1024 (every DepthDecoder width), else MD2_ERR_ARG. */
size_t md2_decoder_pad_workspace_bytes(const md2_pad_desc* desc);
int md2_decoder_pad_fwd(const md2_pad_desc* desc, const float* x, const float* skip, const float* bias,
                        float* out, void* stream);
int md2_decoder_pad_bwd(const md2_pad_desc* desc, const float* x, const float* bias, const float* grad_out,
                        float* grad_x, float* grad_skip, float* grad_bias, void* workspace, void* stream);
/* md2_decoder_pad_bwd of grad_out + grad_out2 (NULL = none; same shape and layout as
 * grad_out, MD2_PAD_NHWC with channel counts multiple of 4 only): the padded input of
 * upconv(i,1)'s output feeds both dispconv(i) and upconv(i-1,0) (depth_decoder.py:56-64),
 * so its two gradients are summed as they are read instead of by a separate add.
 * (ABI 19) */
int md2_decoder_pad_bwd2(const md2_pad_desc* desc, const float* x, const float* bias, const float* grad_out,
                         const float* grad_out2, float* grad_x, float* grad_skip, float* grad_bias, void* workspace,
                         void* stream);

/*
 * DepthDecoder disparity heads (networks/depth_decoder.py:63-64, layers.py:121-136):
 * disp = sigmoid(Conv2d(C, 1, 3)(padded) + bias) on the reflection-padded NHWC fp32
 * input that md2_decoder_pad_fwd builds, padded = (B, h+2, w+2, C); disp (B,1,h,w).
 * weight is the (1,C,3,3) parameter in its own memory format (MD2_HEAD_WEIGHT_CL:
 * channels_last, i.e. [ky][kx][c]; else [c][ky][kx]); grad_weight is written in the
 * same format.  The backward takes the forward's disp (sigmoid backward from its
 * output, as torch) and returns grad_padded (B,h+2,w+2,C) plus grad_weight /
 * grad_bias as fixed-order sums (deterministic), with `workspace` of
 * md2_disp_head_workspace_bytes.  C a multiple of 4 dividing 1024, C <= 256.
 * Replaces the dispconv Conv3x3 + nn.Sigmoid of the reference decoder.
 */
#define MD2_HEAD_WEIGHT_CL (1u << 0)
/* ABI 23: padded / grad_padded are bf16 (uint16 storage behind the float pointers; config
 * C5's bf16 decoder), widened exactly / rounded to nearest even; weight, bias, disp and
 * the gradients of the parameters stay fp32 */
#define MD2_HEAD_BF16 (1u << 1)

typedef struct md2_head_desc {
    int32_t batch, channels, height, width; /* of the unpadded output */
    uint32_t flags;                         /* MD2_HEAD_* */
} md2_head_desc;

size_t md2_disp_head_workspace_bytes(const md2_head_desc* desc);
int md2_disp_head_fwd(const md2_head_desc* desc, const float* padded, const float* weight, const float* bias,
                      float* disp, void* stream);
int md2_disp_head_bwd(const md2_head_desc* desc, const float* padded, const float* weight, const float* disp,
                      const float* grad_disp, float* grad_padded, float* grad_weight, float* grad_bias,
                      void* workspace, void* stream);

/*
 * Weight gradient of the ResNet stem convolution (conv1 of networks/resnet_encoder.py
 * via torchvision ResNet: Conv2d(C, 64, 7, stride 2, padding 3, bias=False)), whose
 * input is data (the normalised frames), so the input gradient is never needed.
 * x (batch, height, width, channels) NHWC fp32, channels 3 / 6 / 9 (one, two or three
 * frames); grad_y (batch, Ho, Wo, 64) NHWC with Ho = (height-1)/2+1, Wo likewise;
 * grad_weight (64, channels, 7, 7) written (not accumulated) in the weight's memory
 * format (MD2_STEM_WEIGHT_CL: channels_last [co][ky][kx][ci]; else [co][ci][ky][kx]).
 * Deterministic (fixed-order sums); workspace of md2_stem_wgrad_workspace_bytes.
 * Replaces MIOpen's backward-weights convolution for this layer.
 */
#define MD2_STEM_WEIGHT_CL (1u << 0)
/* ABI 23: bf16 operands (uint16 storage behind the float pointers; config C5's bf16
 * autocast stem), channels 3 / 6: md2_stem_wgrad's x and grad_y (grad_weight stays
 * fp32); md2_stem_fwd's x and y (the fp32 weight rounded to bf16, fp32 accumulation,
 * y rounded to nearest even) */
#define MD2_STEM_BF16 (1u << 1)
/* md2_stem_wgrad / md2_stem_wgrad_bn, fp32, channels 3 / 6: this call runs the form that
 * prefetches the next chunk behind the MFMAs (what MD2_STEM_PF32=1 selects for every
 * call); same sums, bit for bit */
#define MD2_STEM_PREFETCH (1u << 2)

typedef struct md2_stem_desc {
    int32_t batch, channels, height, width; /* of the input */
    uint32_t flags;                         /* MD2_STEM_* */
} md2_stem_desc;

size_t md2_stem_wgrad_workspace_bytes(const md2_stem_desc* desc);
int md2_stem_wgrad(const md2_stem_desc* desc, const float* x, const float* grad_y, float* grad_weight,
                   void* workspace, void* stream);

/*
 * Forward of the same convolution: y (batch, Ho, Wo, 64) NHWC fp32 = conv(x, weight),
 * stride 2, padding 3, on split-bf16 MFMA (f32-class), channels 3 / 6.  weight
 * (64, channels, 7, 7) in the memory format MD2_STEM_WEIGHT_CL names.  No workspace.
 * Replaces MIOpen's forward convolution for this layer (torchvision conv1 forward,
 * networks/resnet_encoder.py:93).
 */
int md2_stem_fwd(const md2_stem_desc* desc, const float* x, const float* weight, float* y, void* stream);

/*
 * Conv bias (+ ReLU) epilogue on NHWC fp32 activations (networks/pose_decoder.py:43-54:
 * relu(conv(x) + b) and the last conv's bias), the convolution itself running
 * bias-free on MIOpen.  x / y / grad (pixels, channels) row-major = channels_last.
 * fwd: y = [relu](x + bias).
 * bwd: grad_x = grad_y · [y > 0] (MD2_BIAS_ACT_RELU only; without it grad_x is unused
 * and may be NULL) and grad_bias = Σ_pixels of that, in a fixed order, with `workspace`
 * of md2_bias_act_workspace_bytes.  channels a multiple of 4.
 */
#define MD2_BIAS_ACT_RELU (1u << 0)

typedef struct md2_bias_act_desc {
    int64_t pixels;
    int32_t channels;
    uint32_t flags; /* MD2_BIAS_ACT_* */
} md2_bias_act_desc;

int md2_bias_act_fwd(const md2_bias_act_desc* desc, const float* x, const float* bias, float* y, void* stream);
size_t md2_bias_act_workspace_bytes(const md2_bias_act_desc* desc);
int md2_bias_act_bwd(const md2_bias_act_desc* desc, const float* y, const float* grad_y, float* grad_x,
                     float* grad_bias, void* workspace, void* stream);

/*
 * The encoders' input (networks/resnet_encoder.py:93 normalisation, trainer.py:280-290
 * frame-pair concatenation) in one pass: src[g * slots + k] is a (batch,3,H,W) NCHW
 * fp32 frame tensor; out is (groups*batch, H, W, 3*slots) = a channels_last
 * (groups*batch, 3*slots, H, W) tensor with out = (src - mean) * (1.f / std) per channel
 * (torch's fp32 arithmetic for a division by a scalar).
 * groups * slots <= 8.  Returns MD2_OK / MD2_ERR_*.
 */
int md2_encoder_input(int groups, int batch, int slots, int height, int width, const float* const* src, float mean,
                      float std_, float* out, void* stream);

/*
 * The optimizer step (torch.optim.Adam as the reference's trainer.py:102-104, 209;
 * no weight decay / amsgrad) in one launch per 256 parameters over a device table of
 * chunks.  Every chunk is a contiguous run of n fp32 elements of one parameter with
 * its gradient and its two moment buffers in the same layout; `step` is the 1-based
 * step count the bias corrections use.  Returns MD2_OK / MD2_ERR_*.
 */
typedef struct md2_adam_chunk {
    float* p;         /* parameter elements [off, off + n) */
    float* m;         /* exp_avg, same elements */
    float* v;         /* exp_avg_sq, same elements */
    int64_t off;      /* element offset into the parameter's gradient */
    int64_t n;
    int32_t param;    /* index into grads[] */
    int32_t reserved;
} md2_adam_chunk;

/* table: device array of chunks ordered by param; chunk_start (host, nparams + 1):
 * first chunk of each parameter; grads (host, nparams): this step's gradient base
 * pointers (same layout as their parameters). */
int md2_adam_step(const md2_adam_chunk* table, const int* chunk_start, int nparams, const float* const* grads,
                  double lr, double beta1, double beta2, double eps, int step, void* stream);
/* The same step with the step counter and lr on the device (hipGraph-capturable, the
 * `capturable=True` form of torch.optim.Adam): *step (fp32, the value torch keeps in
 * state["step"]) is incremented first, the bias corrections are formed in double from
 * it and *lr (fp64, the param group's lr tensor that StepLR fills); `hyper` is 2 fp32
 * of device scratch. */
int md2_adam_step_dev(const md2_adam_chunk* table, const int* chunk_start, int nparams, const float* const* grads,
                      const double* lr, double beta1, double beta2, double eps, float* step, float* hyper,
                      void* stream);
/* The capturable step in parts (ABI v21): md2_adam_hyper advances *step and writes the
 * two factors to `hyper` (md2_adam_step_dev's first launch); md2_adam_apply_dev updates
 * the parameters [k_begin, k_end) of the table with them.  Calls over disjoint ranges,
 * each on a stream ordered after md2_adam_hyper and after its parameters' gradients,
 * cover the step once (the trainer runs the pose network's parameters on the pose
 * stream as soon as its backward is done).  grads is indexed like chunk_start. */
int md2_adam_hyper(const double* lr, double beta1, double beta2, float* step, float* hyper, void* stream);
int md2_adam_apply_dev(const md2_adam_chunk* table, const int* chunk_start, int k_begin, int k_end,
                       const float* const* grads, double beta1, double beta2, double eps, const float* hyper,
                       void* stream);

/*
 * Fused pose producer: transformation_from_parameters
 * (layers.py:28-45, with rot_from_axisangle 64-103 and get_translation_matrix
 * 48-61) for every (frame, image) of a step in one launch, and its adjoint.
 * axisangle, translation: (frames, batch, 3); T / grad_T: (frames, batch, 4, 4);
 * bit f of invert_mask selects invert=True for frame f (trainer.py:294-295).
 */
int md2_pose_fwd(int32_t frames, int32_t batch, uint32_t invert_mask, const float* axisangle,
                 const float* translation, float* T, void* stream);
int md2_pose_bwd(int32_t frames, int32_t batch, uint32_t invert_mask, const float* axisangle,
                 const float* translation, const float* grad_T, float* grad_axisangle,
                 float* grad_translation, void* stream);

/*
 * GPU input pipeline: what MonoDataset.__getitem__ does to
 * the decoded frames of a batch (datasets/mono_dataset.py:136-200 with
 * kitti_dataset.py:58-63) — horizontal flip, the cascaded Resize(ANTIALIAS) pyramid
 * (mono_dataset.py:80-84, 96-101), ToTensor and the per-item ColorJitter
 * (mono_dataset.py:66-78, 175-181, 103-108) — bit-exact with the PIL arithmetic the
 * reference runs on the CPU workers.  The per-item random decisions are drawn by the
 * caller (same draws, same order as the reference) and passed in `items`.
 */
typedef struct md2_aug_desc {
    int32_t items;                 /* batch size B */
    int32_t frames;                /* frames per item F (frame_ids, incl. "s") */
    int32_t in_height, in_width;   /* decoded frame size (scale -1) */
    int32_t height, width;         /* scale-0 size; scale s is (height>>s, width>>s) */
    int32_t num_scales;            /* 1..4 */
    int32_t reserved;
} md2_aug_desc;

#define MD2_AUG_BRIGHTNESS 0
#define MD2_AUG_CONTRAST   1
#define MD2_AUG_SATURATION 2
#define MD2_AUG_HUE        3

typedef struct md2_aug_item {
    uint8_t flip;        /* do_flip (mono_dataset.py:137): frames flipped left-right */
    uint8_t color_aug;   /* do_color_aug (mono_dataset.py:136) */
    uint8_t hue_shift;   /* np.uint8(hue_factor * 255), wrapped as numpy 1.x does */
    uint8_t reserved;
    uint8_t order[4];    /* MD2_AUG_* in application order (ColorJitter's shuffle) */
    float brightness, contrast, saturation;   /* the get_params factors */
} md2_aug_item;

typedef struct md2_aug_plan md2_aug_plan;

/* Builds the LANCZOS tables (host, double, as PIL) and allocates the uint8 pyramid
 * scratch on the current device.  NULL on error (see md2_last_error). */
md2_aug_plan* md2_aug_plan_create(const md2_aug_desc* desc);
void md2_aug_plan_destroy(md2_aug_plan* plan);

/*
 * frames: device uint8 (F, B, in_height, in_width, 3), frame-major (frame f of item b
 * at index f*B + b); items: HOST md2_aug_item[B], staged through a pinned ring owned by
 * the plan and uploaded on `stream` (the call does not wait for the GPU; a plan is not
 * thread-safe);
 * color[s] / color_aug[s]: device float32 (F, B, 3, height>>s, width>>s), i.e.
 * inputs[("color", frame_ids[f], s)][b] and inputs[("color_aug", ...)][b].
 */
int md2_aug_run(md2_aug_plan* plan, const uint8_t* frames, const md2_aug_item* items,
                float* const* color, float* const* color_aug, void* stream);
/* ... and (ABI 20) src8, device uint32 (F-1, B, height, width) or NULL: frames 1..F-1
 * (the photometric sources, frame_ids[1:]) at scale 0 as RGBx dwords, byte c = the
 * 8-bit colour whose k/255 is color[0] — md2_tensors.src8, so the hot path's forward
 * does not re-pack them from the fp32 planes. */
int md2_aug_run2(md2_aug_plan* plan, const uint8_t* frames, const md2_aug_item* items,
                 float* const* color, float* const* color_aug, uint32_t* src8, void* stream);

/*
 * Mixed decoded sizes in one batch (ABI 24, new symbols): KITTI raw has four frame
 * sizes by recording date and a shuffled batch mixes them (each item is resized on its
 * own, mono_dataset.py:96-101).  sizes: num_sizes (1..16) pairs (in_height, in_width),
 * the plan's size classes; desc->in_height / in_width are ignored.  One set of scale-0
 * LANCZOS tables per class (host, double, as PIL); levels 1.. are built once; scratch
 * is sized for the largest class.  A mixed plan runs through md2_aug_run_mixed only.
 */
md2_aug_plan* md2_aug_plan_create_mixed(const md2_aug_desc* desc, const int32_t* sizes, int num_sizes);
/*
 * frames_base: ONE device uint8 buffer of total_bytes holding frame f of item b as a
 * tight (h_c, w_c, 3) image at byte frame_offset[f*B + b] (its allocation must reach
 * total_bytes rounded up to 4: rows are fetched as aligned dwords);
 * frame_offset: HOST uint64[F*B], every entry a multiple of 16; item_class: HOST
 * int32[B] indexing `sizes` (all frames of an item share a class: one drive).  Both
 * travel with `items` through the plan's pinned ring in one upload: no synchronisation
 * and no allocation per call.  Outputs are md2_aug_run2's, and for every item bit-equal
 * to a single-size plan run on that item alone (the contrast mean is per image).
 * Scale 0 is one launch per class present (two-pass classes: h, v and their contrast
 * sums).  MD2_ERR_ARG, before any launch: a NULL argument, a class out of range, a
 * misaligned offset, offset + h_c*w_c*3 > total_bytes, a non-permutation order.
 * Overlapping frames are not refused: frames are only read.
 */
int md2_aug_run_mixed(md2_aug_plan* plan, const uint8_t* frames_base, uint64_t total_bytes,
                      const int32_t* item_class, const uint64_t* frame_offset, const md2_aug_item* items,
                      float* const* color, float* const* color_aug, uint32_t* src8, void* stream);

/*
 * Training-mode BatchNorm2d (+ residual add) (+ ReLU) on channels_last activations:
 * relu(bn(x)) and relu(bn(x) + identity) of the ResNet encoders' blocks
 * (torchvision BasicBlock / Bottleneck behind networks/resnet_encoder.py:62-98).
 * x, y, residual and their gradients: (pixels = N*H*W, channels) fp32, or bf16 with
 * MD2_BN_BF16 (NHWC; fp32 arithmetic and statistics);
 * channels a multiple of 4 with channels/4 dividing, or a multiple of, 256.
 * Forward writes y, the batch mean and 1/sqrt(var + eps) (save_*), and updates the
 * running statistics when running_mean/var are given (momentum, unbiased variance,
 * as nn.BatchNorm2d).  workspace: md2_bn_workspace_bytes, no initialisation needed;
 * a backward must not share its workspace with another call in flight.  Three
 * launches each way; deterministic.
 */
#define MD2_BN_RELU     (1u << 0)
#define MD2_BN_RESIDUAL (1u << 1)
#define MD2_BN_BF16     (1u << 2)   /* x, residual, y and their gradients are bf16 (params, stats fp32) */

typedef struct md2_bn_desc {
    int64_t pixels;   /* N*H*W over all groups */
    int32_t channels;
    uint32_t flags;   /* MD2_BN_* */
    float eps, momentum;
    /* groups > 1: the N images form `groups` equal consecutive chunks, each normalised
     * with its own batch statistics, running statistics updated chunk by chunk in
     * order — exactly `groups` separate BatchNorm calls (the pose encoder runs both
     * frame pairs as one batch this way).  save_mean / save_invstd: (groups, C). */
    int32_t groups;
    int32_t reserved;
} md2_bn_desc;

size_t md2_bn_workspace_bytes(const md2_bn_desc* desc);
int md2_bn_fwd(const md2_bn_desc* desc, const void* x, const float* gamma, const float* beta,
               const void* residual, float* running_mean, float* running_var, void* y,
               float* save_mean, float* save_invstd, void* workspace, void* stream);
/* grad_residual = d(loss)/d(residual) (with MD2_BN_RESIDUAL); y is needed with MD2_BN_RELU. */
int md2_bn_bwd(const md2_bn_desc* desc, const void* x, const void* y, const void* grad_y,
               const float* gamma, const float* save_mean, const float* save_invstd,
               void* grad_x, void* grad_residual, float* grad_gamma, float* grad_beta,
               void* workspace, void* stream);
/* md2_bn_bwd with the output gradient given as up to three tensors summed on load
 * (grad_y + grad_y2 + grad_y3; grad_y2 / grad_y3 may be NULL): the output's other
 * consumers (the next block's shortcut, the decoder skip) hand their gradients here
 * instead of autograd adding them in separate passes. */
int md2_bn_bwd_multi(const md2_bn_desc* desc, const void* x, const void* y, const void* grad_y,
                     const void* grad_y2, const void* grad_y3, const float* gamma, const float* save_mean,
                     const float* save_invstd, void* grad_x, void* grad_residual, float* grad_gamma,
                     float* grad_beta, void* workspace, void* stream);
/* ABI 15: the ReLU mask instead of y.  md2_bn_fwd_mask = md2_bn_fwd that also writes
 * relu_mask (MD2_BN_RELU only; NULL = none): one byte per element quad of y, bit i set
 * when element 4q + i of y (as stored: bf16 after rounding) is > 0 — pixels*channels/4
 * bytes.  md2_bn_bwd_mask = md2_bn_bwd_multi gated by that mask instead of reading y
 * (1/16 of y's bytes in fp32): same results, bit for bit. */
int md2_bn_fwd_mask(const md2_bn_desc* desc, const void* x, const float* gamma, const float* beta,
                    const void* residual, float* running_mean, float* running_var, void* y, uint8_t* relu_mask,
                    float* save_mean, float* save_invstd, void* workspace, void* stream);
int md2_bn_bwd_mask(const md2_bn_desc* desc, const void* x, const uint8_t* relu_mask, const void* grad_y,
                    const void* grad_y2, const void* grad_y3, const float* gamma, const float* save_mean,
                    const float* save_invstd, void* grad_x, void* grad_residual, float* grad_gamma,
                    float* grad_beta, void* workspace, void* stream);

/*
 * The ResNet stem's MaxPool2d(3, stride 2, padding 1) on channels_last activations
 * (x: (batch, height, width, channels), channels a multiple of 4; fp32, or bf16 with
 * MD2_POOL_BF16).  idx: one byte per output value, the winning window position 0..8
 * (first maximum in scan order; NaN propagates, as ATen), uint32-packed per 4
 * channels: batch * ho * wo * channels / 4 words.  The backward gathers (no atomics).
 */
#define MD2_POOL_BF16 (1u << 0)

typedef struct md2_pool_desc {
    int32_t batch, channels, height, width;
    uint32_t flags;
    int32_t reserved;
} md2_pool_desc;

int md2_maxpool3s2_fwd(const md2_pool_desc* desc, const void* x, void* y, uint32_t* idx, void* stream);
int md2_maxpool3s2_bwd(const md2_pool_desc* desc, const uint32_t* idx, const void* grad_y, void* grad_x,
                       void* stream);
/* grad_x = the pool's adjoint of grad_y + grad_add (same shape and layout as x; NULL
 * = none): the stem activation also feeds the DepthDecoder skip (resnet_encoder.py:96
 * features[0]), so its two gradients are summed in the gather instead of a separate
 * add pass. */
int md2_maxpool3s2_bwd_add(const md2_pool_desc* desc, const uint32_t* idx, const void* grad_y, const void* grad_add,
                           void* grad_x, void* stream);
/* ... and grad_y2 (NULL = none) a second gradient of the pooled map y, same shape and
 * layout as grad_y, summed into it on load: y feeds both the first BasicBlock's conv1 and
 * its identity shortcut (torchvision BasicBlock.forward, `identity = x`), so autograd
 * would otherwise add the two gradients in a separate pass. (ABI 19) */
int md2_maxpool3s2_bwd_multi(const md2_pool_desc* desc, const uint32_t* idx, const void* grad_y, const void* grad_y2,
                             const void* grad_add, void* grad_x, void* stream);

/*
 * fp32 convolutions as implicit GEMMs on f32 MFMA (csrc/conv.hip): the ResNet
 * encoders' 3x3 / 1x1 convolutions (networks/resnet_encoder.py, torchvision
 * BasicBlock/Bottleneck) and the DepthDecoder's 3x3 convolutions on reflection-padded
 * inputs (networks/depth_decoder.py:50-65 via layers.py:106-136 Conv3x3; the padding
 * is md2_decoder_pad_fwd's, so pad = 0), forward and backward, replacing MIOpen.
 * x (batch, height, width, in_channels) NHWC fp32; weight (out_channels, kernel_h,
 * kernel_w, in_channels) = a channels_last Conv2d weight; y (batch, Ho, Wo,
 * out_channels) NHWC with Ho = (height + 2 pad - kernel_h) / stride + 1.  No bias.
 * Channel counts multiples of 4, pad < kernel, every tensor < 2^29 elements.  Zero
 * padding outside the image.  Deterministic (a K split sums its partials in order);
 * workspace of md2_conv_workspace_bytes (0 = none needed).
 */
#define MD2_CONV_NO_SPLIT  (1u << 1) /* no K split (tests)              */
#define MD2_CONV_TILE_N32  (1u << 2) /* force the 128 x 32 tile (tests) */
#define MD2_CONV_TILE_N64  (1u << 3) /* force the 128 x 64 tile         */
#define MD2_CONV_TILE_N128 (1u << 4) /* force the 128 x 128 tile        */
#define MD2_CONV_X6        (1u << 5) /* split-bf16 (3 planes, 6 products) f32-class MFMA path */
#define MD2_CONV_BM256     (1u << 6) /* x6 forward / input grad: 256 x 128 tiles (N > 64)     */
#define MD2_CONV_PRESPLIT  (1u << 7) /* x6: `weight` holds md2_conv_split_weights planes      */
#define MD2_CONV_PATCH     (1u << 8) /* x6 3x3 stride 1: fwd / dgrad (GEMM channels % 32) with
                                        the input patch of a pixel rectangle staged once for
                                        all nine taps (conv_x6p_kernel); the weight gradient
                                        with three input rows per 32-pixel segment staged
                                        once for the nine taps (conv_x6pw_kernel)           */
#define MD2_CONV_S2_ONE    (1u << 9) /* x6 stride-2 input gradient: the four parity classes
                                        in one launch, no K split                           */
#define MD2_CONV_WS        (1u << 10) /* x6 forward / stride-1 input gradient, 128-wide tiles: the
                                         warp-specialised kernel (4 MFMA + 4 staging waves) */
#define MD2_CONV_BF16      (1u << 11) /* ABI 22: a bf16 autocast convolution (config C5): x, y,
                                         grad_y, grad_x are bf16 NHWC; `weight` of md2_conv_fwd /
                                         md2_conv_dgrad is ONE bf16 plane of
                                         md2_conv_bf16_weights; grad_weight stays fp32, holding
                                         bf16-rounded values (the autocast cast's backward).
                                         f32 accumulation, output rounded to nearest even,
                                         deterministic (fixed-order K split).  fwd: in_channels
                                         % 8; dgrad: stride 1, out_channels % 8 */

typedef struct md2_conv_desc {
    int32_t batch, height, width, in_channels; /* input */
    int32_t out_channels, kernel_h, kernel_w, stride, pad;
    uint32_t flags;                            /* MD2_CONV_* */
} md2_conv_desc;

size_t md2_conv_workspace_bytes(const md2_conv_desc* desc);
/* The split-bf16 weight planes of md2_conv_fwd / md2_conv_dgrad with MD2_CONV_X6 in
 * one pass: planes_fwd [3][Co][KH*KW][Ci] bf16 and (nullable) planes_dgrad
 * [3][Ci][KH*KW][Co] (taps flipped); pass them as `weight` with MD2_CONV_PRESPLIT.
 * Channels must be multiples of 8. */
int md2_conv_split_weights(const md2_conv_desc* desc, const float* weight, void* planes_fwd, void* planes_dgrad,
                           void* stream);
/* Every conv weight of a training step split in ONE launch (the per-convolution
 * md2_conv_split_weights launches of the forward, ~80 tiny kernels per step, become one
 * ~10k-block grid): `table` is a DEVICE array of `n` entries; entry e covers grid blocks
 * [block0, block0 + ceil(ci/32) * ceil(co/32) * kt) in ascending order, and
 * `total_blocks` is the last entry's end.  Same planes as md2_conv_split_weights
 * (planes_dgrad nullable per entry).  Graph-capturable (no host sync). */
typedef struct md2_wsplit_entry {
    const float* weight;        /* (co, kt, ci) channels_last conv weight        */
    void* planes_fwd;           /* [3][co][kt][ci] bf16                           */
    void* planes_dgrad;         /* [3][ci][kt][co] bf16, taps flipped, or NULL    */
    int32_t co, kt, ci;         /* out channels, kernel_h * kernel_w, in channels */
    int32_t block0;             /* first grid block of this entry                 */
    void* planes_col;           /* [3][kt][ci][co] bf16 (taps not flipped), or NULL: the
                                   weight as the 1x1 GEMM operand of a strided input
                                   gradient's column form (md2_conv_col2im; ABI 19) */
} md2_wsplit_entry;
int md2_conv_split_weights_multi(const md2_wsplit_entry* table, int n, int total_blocks, void* stream);
/* MD2_CONV_BF16 operands (ABI 22): the fp32 weight rounded to bf16 (nearest even) in the
 * forward layout w_fwd [Co][KH*KW][Ci] and (nullable) the input gradient's w_dgrad
 * [Ci][KH*KW][Co] with the taps flipped — what autocast's bf16 cast of the weight feeds a
 * bf16 convolution, in the two GEMM layouts.  The _multi form converts a whole table of
 * weights in one launch (md2_wsplit_entry: planes_fwd / planes_dgrad receive the one
 * plane each, planes_col unused). */
int md2_conv_bf16_weights(const md2_conv_desc* desc, const float* weight, void* w_fwd, void* w_dgrad, void* stream);
int md2_conv_bf16_weights_multi(const md2_wsplit_entry* table, int n, int total_blocks, void* stream);
int md2_conv_fwd(const md2_conv_desc* desc, const float* x, const float* weight, float* y, void* workspace,
                 void* stream);
/* grad_x (batch, height, width, in_channels) from grad_y (batch, Ho, Wo, out_channels):
 * stride 1 (a "full" convolution with the flipped, transposed weight), or stride 2 with
 * MD2_CONV_X6 and >= 32 out_channels (four output-parity classes, each a stride-1 GEMM
 * over its taps, scattered into grad_x) */
int md2_conv_dgrad(const md2_conv_desc* desc, const float* grad_y, const float* weight, float* grad_x,
                   void* workspace, void* stream);
/* The gather half of a strided input gradient computed as one GEMM: cols (batch, Ho, Wo,
 * kernel_h, kernel_w, in_channels) — grad_y times the weight as [out][(kh, kw, ci)], a 1x1
 * md2_conv_fwd with kernel_h*kernel_w*in_channels outputs — summed into grad_x (batch,
 * height, width, in_channels): each pixel gathers its taps in (kh, kw) order, written
 * (not accumulated).  in_channels % 4; replaces the parity-class launches of a stride-2
 * md2_conv_dgrad (MIOpen's backward-data convolution, networks/resnet_encoder.py). */
int md2_conv_col2im(const md2_conv_desc* desc, const float* cols, float* grad_x, void* stream);
/* grad_weight (out_channels, kernel_h, kernel_w, in_channels) = channels_last layout */
int md2_conv_wgrad(const md2_conv_desc* desc, const float* x, const float* grad_y, float* grad_weight,
                   void* workspace, void* stream);
/* Direct 3x3 stride-1 convolution on the f32 VALU (csrc/direct.hip) for the
 * DepthDecoder's 16-output-channel layers (networks/depth_decoder.py:50-65:
 * upconv(0,0) 32->16, upconv(0,1) 16->16) and their input gradients: y (batch, Ho, Wo,
 * out_channels) = x (batch, height, width, in_channels) correlated with
 * wk [9][in_channels][out_channels] (tap-major; for the input gradient: the flipped
 * weight with its channel roles swapped, pad = 2 - the forward's pad), zero padding
 * `pad` (0..2), Ho = height + 2 pad - 2.  (in, out) channels (16,16), (32,16) or
 * (16,32); kernel 3x3, stride 1; desc flags unused.  One thread per output pixel,
 * exact f32 FMA chains. */
int md2_conv_direct(const md2_conv_desc* desc, const float* x, const float* wk, float* y, void* stream);
/* Weight gradient of the same layers on the f32 VALU: grad_weight (out_channels, 3, 3,
 * in_channels) = sum over output pixels of grad_y x the input's tap; (in, out) channels
 * (16,16) or (32,16), stride 1, pad 0..2.  Per-block partial rows in `workspace`
 * (md2_conv_wgrad_direct_workspace_bytes), summed in block order (deterministic). */
size_t md2_conv_wgrad_direct_workspace_bytes(const md2_conv_desc* desc);
int md2_conv_wgrad_direct(const md2_conv_desc* desc, const float* x, const float* grad_y, float* grad_weight,
                          void* workspace, void* stream);

/*
 * KITTI depth evaluation (ABI 24, csrc/eval.hip): the per-image body of the reference's
 * evaluate_depth.py:181-214 (resize the disparity to the ground-truth map, mask, median
 * scaling, clamp, compute_errors 27-45, batch_post_process_disparity 48-56) and of
 * Trainer.compute_depth_losses (trainer.py:498-526) as one chain of launches on `stream`:
 * no boolean indexing, no host-side median, nothing returns to the host.
 *
 * disp (B,1,height,width): the network's sigmoid output (disp_to_depth's scaling with
 * min_depth / max_depth, layers.py:16-25, happens here); disp_flipped: the same for the
 * horizontally flipped images (MD2_EVAL_POST_PROCESS; else may be NULL); gt
 * (B,gt_height,gt_width), 0 = no measurement.  Per ground-truth pixel:
 *   default              pred = scale_factor / bilinear(scaled disparity)   (evaluate_depth.py)
 *   MD2_EVAL_RESIZE_DEPTH pred = scale_factor * clamp(bilinear(1 / scaled disparity),
 *                                eval_min, eval_max)                (compute_depth_losses)
 * bilinear = half-pixel centres, src = (dst + 0.5) * in / out - 0.5, negative coordinates
 * clamped to 0, the upper neighbour clamped to the edge (F.interpolate, align_corners=
 * False).  A pixel is valid when gt > 0 (MD2_EVAL_GT_RANGE: eval_min < gt < eval_max) and
 * it lies in the crop rectangle [crop_y0, crop_y1) x [crop_x0, crop_x1).  A population is
 * the valid pixels of one image, or of the whole batch with MD2_EVAL_POOL_BATCH.  With
 * MD2_EVAL_MEDIAN_SCALE pred *= median(gt) / median(pred) over the population, the
 * medians being exact order statistics of the fp32 values (four 8-bit radix passes over
 * their bit patterns): the element at (n-1)/2 with MD2_EVAL_MEDIAN_LOWER (torch.median),
 * else the mean of the elements at (n-1)/2 and n/2 (np.median).  Then pred is clamped to
 * [eval_min, eval_max] and the seven metrics are reduced: fixed per-block trees, the block
 * partials summed in block order, all in fp64; the threshold counts are integers.
 * disp_to_depth is torch's fp32 product and sum; the arithmetic between it and the fp32
 * pred (post-processing, resize, inversion) is fp64, rounded once.  min_depth 1 with
 * max_depth INFINITY makes that scaling the identity (disp already scaled).
 *
 * out: P x 10 floats, P = B (or 1 with POOL_BATCH): abs_rel, sq_rel, rmse, rmse_log, a1,
 * a2, a3, the median ratio applied (1 without MEDIAN_SCALE), the valid-pixel count, 0
 * (reserved).  A population without a valid pixel gets count 0 and NaN in the first eight.
 * workspace: the size the function below returns, no initialisation needed; after the call its
 * first B * gt_height * gt_width floats hold pred before the median scaling (bit pattern
 * 0xFFFFFFFF at invalid pixels).  Deterministic, hipGraph-capturable.
 */
#define MD2_EVAL_POST_PROCESS (1u << 0)
#define MD2_EVAL_RESIZE_DEPTH (1u << 1)
#define MD2_EVAL_GT_RANGE     (1u << 2)
#define MD2_EVAL_MEDIAN_SCALE (1u << 3)
#define MD2_EVAL_MEDIAN_LOWER (1u << 4)
#define MD2_EVAL_POOL_BATCH   (1u << 5)
#define MD2_EVAL_OUT 10   /* floats per population */

typedef struct md2_eval_desc {
    int32_t batch;                  /* B */
    int32_t height, width;          /* of disp (the network's scale-0 map) */
    int32_t gt_height, gt_width;    /* of gt */
    int32_t crop_y0, crop_y1, crop_x0, crop_x1; /* within the gt map; the whole map = no crop */
    uint32_t flags;                 /* MD2_EVAL_* */
    double min_depth, max_depth;    /* opt.min_depth / opt.max_depth of disp_to_depth, as the
                                       Python doubles (offset 40): lo = fp32(1 / max_depth) and
                                       range = fp32(1 / min_depth - 1 / max_depth) are then the
                                       fp32 scalars torch multiplies and adds for any value */
    float eval_min, eval_max;       /* MIN_DEPTH / MAX_DEPTH of the evaluation (1e-3, 80) */
    double scale_factor;            /* opt.pred_depth_scale_factor (5.4 for stereo); a double (at
                                       offset 56) because it multiplies every prediction: the
                                       fp32 of 5.4 alone is off by 1.8e-8; offset 64, the struct is 72 bytes */
} md2_eval_desc;

/* 0 (and md2_last_error) for a desc md2_depth_eval would refuse */
size_t md2_depth_eval_workspace_bytes(const md2_eval_desc* desc);
int md2_depth_eval(const md2_eval_desc* desc, const float* disp, const float* disp_flipped, const float* gt,
                   float* out, void* workspace, void* stream);

/*
 * KITTI velodyne scans -> sparse ground-truth depth maps (csrc/velo.hip): the reference's
 * kitti_utils.generate_depth_map (kitti_utils.py:46-98), which export_gt_depth.py and
 * KITTIRAWDataset.get_depth run per frame in numpy and a Python loop, for a batch of
 * frames of one image size as a fixed chain of launches on `stream` (memset, scatter,
 * resolve).  Added under ABI 24 without raising MD2_ABI_VERSION: the additions are new
 * symbols only, no existing struct or function changed, and md2_build_id already refuses
 * a library built from other sources.
 *
 * points: fp32 (total_points, 4) rows x, y, z, reflectance, the frames' .bin contents
 * concatenated (the fourth value is ignored); offsets: int64 (B + 1), frame b owns the
 * rows offsets[b] .. offsets[b+1]; P: fp64 (B, 3, 4), P_rect_0{cam} @ R_rect_00 (4x4) @
 * velo2cam (4x4) per frame; depth: fp32 (B, height, width), written completely (0 = no
 * measurement).  All on the device.  Per frame, with the point order being the row order:
 *   - a point is kept if x >= 0;
 *   - q = P . (x, y, z, 1) in fp64, ((P0*x + P1*y) + P2*z) + P3 uncontracted;
 *     u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1 (half to even); it is valid if
 *     0 <= u < width and 0 <= v < height, compared in fp64 (NaN, infinite and q2 == 0
 *     points fail the comparisons); its depth is q2, or x with MD2_VELO_VEL_DEPTH;
 *   - every pixel first takes the depth of its last valid point;
 *   - valid points are grouped by the reference's sub2ind key v * (width - 1) + u - 1,
 *     which (v, width-1) and (v+1, 0) share; the pixel of a group's first point takes the
 *     minimum depth of the group.  So a pixel with several points gets their minimum, and
 *     of a wrapped pair one pixel gets the minimum over both while the other keeps its
 *     last-written value;
 *   - negative depths become 0; the map is rounded to fp32 (exact with VEL_DEPTH).
 * Refused (MD2_ERR_ARG): NULL operands, non-positive sizes, width < 2 (the key
 * degenerates), batch > 65535, batch * height * width or total_points at or above 2^31.
 * The offsets cannot be checked without a synchronisation: 0 = offsets[0] <= ... <=
 * offsets[B] = total_points is the caller's contract (rows outside [0, total_points) are
 * never read, the maps of a broken table are meaningless).
 * workspace: the size the function below returns, no initialisation needed, 16 bytes per
 * pixel.  Integer atomics only: bitwise repeatable for any arrival order, any number of
 * points per pixel.  hipGraph-capturable, no allocation, no host synchronisation.
 */
#define MD2_VELO_VEL_DEPTH (1u << 0)   /* the depth of a point is its own x (export_gt_depth.py:49) */

typedef struct md2_velo_desc {
    int32_t batch;                  /* B frames */
    int32_t height, width;          /* of every map of the call (S_rect_02 reversed) */
    uint32_t flags;                 /* MD2_VELO_* */
    int64_t total_points;           /* rows of points (offset 16) */
    int32_t reserved[2];            /* 0; the struct is 32 bytes */
} md2_velo_desc;

/* 0 (and md2_last_error) for a desc md2_velo_project would refuse */
size_t md2_velo_project_workspace_bytes(const md2_velo_desc* desc);
int md2_velo_project(const md2_velo_desc* desc, const float* points, const int64_t* offsets, const double* P,
                     float* depth, void* workspace, void* stream);

/*
 * KITTI odometry pose evaluation (csrc/traj.hip): the reference's evaluate_pose.py:104-125
 * — local ground-truth poses, 5-frame snippets, scale-aligned absolute trajectory error
 * (ATE), mean and standard deviation — for a batch of sequences as a fixed chain of three
 * launches on `stream` (local poses, errors, statistics), every step in fp64.  New
 * symbols under ABI 24, no version bump (as md2_velo_project).
 *
 * Sequence s owns the frames offsets[s] .. offsets[s+1] (M_s of them) of gt, fp64
 * (total_frames, 3, 4) KITTI pose rows; its M_s - 1 predicted transforms start at row
 * offsets[s] - s of pred, fp32 (total_frames - S, 4, 4), what the reference stores in
 * poses.npy (transformation_from_parameters(axisangle[:, 0], translation[:, 0]), not
 * inverted); its errors start at the same row of ates, fp64 (total_frames - S); stats is
 * fp64 (S, 2): mean, population standard deviation.  All on the device.
 *   - G_i is the 3x4 block over [0,0,0,1]; L_i = inv(inv(G_{i-1}) . G_i), i = 1..M_s-1,
 *     literally: two inverses and a product.  The inverse is the general affine one,
 *     cofactors of the 3x3 over det = (a00*c00 + a01*c01) + a02*c02, then
 *     -((i0*t0 + i1*t1) + i2*t2) per row — not [R^T | -R^T t], which is 1e-7..1e-6 off on
 *     KITTI's seven-digit rotations far from the origin;
 *   - a product is ((a0*b0 + a1*b1) + a2*b2) + a3*b3 per element, the bottom row of the
 *     right factor included ([0,0,0,1] for L, the stored row of a prediction);
 *   - snippet i (0 <= i < M_s - 1) chains n = min(track_length - 1, M_s - 1 - i)
 *     transforms from C = I, C = C . T_k, a point being C[:3, 3] after each, the first
 *     (0,0,0): n + 1 points from L and n + 1 from pred (fp32 promoted to fp64);
 *   - offset = gt[0] - pred[0], pred += offset; num = sum gt*pred, den = sum pred*pred
 *     (points in order, x, y, z within a point, from 0.0); scale = num / den;
 *     ate = sqrt(sum (pred*scale - gt)^2) / (n + 1).  All-zero predicted points give
 *     0/0 = nan, as in the reference;
 *   - mean = sum(ates) / (M_s-1), std = sqrt(sum((a - mean)^2) / (M_s-1)); both sums have
 *     a fixed shape: 256 lanes, lane j adds elements j, j+256, ... in rising order from
 *     0.0, then strides 128, 64, ..., 1 fold lane j+stride into lane j.
 * No contraction anywhere, no float atomics: bitwise repeatable, independent of the
 * launch geometry.  hipGraph-capturable, no allocation, no host synchronisation.
 * Refused (MD2_ERR_ARG): NULL desc or operand, sequences < 1 or > 65535, track_length
 * outside 2..16, non-zero flags, total_frames < 2 * sequences or >= 2^31, a workspace
 * not 256-byte aligned.  The offsets cannot be checked without a synchronisation:
 * 0 = offsets[0] <= ... <= offsets[S] = total_frames with at least two frames per
 * sequence is the caller's contract.  A sequence found shorter than two frames (or whose
 * rows would leave the operands) gets nan in its stats row and nothing else is written
 * for it.  workspace: the size the query returns (the local poses), no initialisation.
 */
typedef struct md2_pose_ate_desc {
    int32_t sequences;              /* S >= 1 */
    int32_t track_length;           /* points per snippet, 2..16; the reference uses 5 */
    uint32_t flags;                 /* none defined yet: non-zero is refused */
    int32_t reserved0;
    int64_t total_frames;           /* sum of ground-truth frames over all sequences (offset 16) */
    int64_t reserved;               /* 0; the struct is 32 bytes */
} md2_pose_ate_desc;

/* 0 (and md2_last_error) for a desc md2_pose_ate would refuse */
size_t md2_pose_ate_workspace_bytes(const md2_pose_ate_desc* desc);
int md2_pose_ate(const md2_pose_ate_desc* desc, const float* pred, const double* gt, const int64_t* offsets,
                 double* ates, double* stats, void* workspace, void* stream);

/*
 * Disparity -> colour picture (csrc/viz.hip): the tail of the reference's test_simple.py
 * (136-155) — bilinear resize to the original image size, np.percentile(., 95) and .min(),
 * matplotlib's Normalize and `magma`, uint8 — for a batch of equally sized maps as a fixed
 * chain of launches on `stream` (memset, resize, four radix-select passes, finalise,
 * colourise).  New symbols under ABI 24, no version bump (as md2_pose_ate).
 *
 * disp: fp32 (B, 1, in_height, in_width) contiguous; rgb: uint8 (B, H, W, 3), row stride
 * 3 * W bytes; resized (optional, may be NULL): fp32 (B, H, W); stats (optional): fp32
 * (B, 2), vmin and vmax per image.  All on the device; statistics are per image.
 *   - resize, fp32, F.interpolate(bilinear, align_corners=False): s = f32(in) / f32(out),
 *     src = max(s * (dst + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = min(i0 + 1, in - 1),
 *     l1 = src - i0, l0 = 1 - l1, r = hy0 * (wx0*a + wx1*b) + hy1 * (wx0*c + wx1*d); at
 *     equal sizes r is the input (a -0 becomes +0, a NaN or infinity spreads to the
 *     neighbours whose zero weight multiplies it);
 *   - with n = H * W and a[0..n-1] the sorted map: q = f32(percentile) / 100f,
 *     vi = f32(n-1) * q; vi >= n-1: vmax = a[n-1]; else lo = floor(vi), g = vi - lo,
 *     d = a[lo+1] - a[lo], vmax = g >= 0.5 ? a[lo+1] - d * (1 - g) : a[lo] + d * g, all
 *     fp32 (numpy's `linear` method on an fp32 array); vmin = min(r), -0 below +0;
 *   - vmin == vmax: t = 0; else u = f32(f64(r) - f64(vmin)),
 *     t = f32(f64(u) / (f64(vmax) - f64(vmin))); x = t * 256f; index 0 if x < 0 or x is
 *     NaN, 255 if x >= 256, else (int)x; the pixel is entry `index` of matplotlib's magma
 *     table as (uint8)(channel * 255);
 *   - a map that holds a NaN after the resize: every pixel (0, 0, 0), vmin = vmax = NaN.
 *     Infinities index inside the table; what they select is unspecified.
 * No contraction, integer atomics only: bitwise repeatable.  hipGraph-capturable, no
 * allocation, no host synchronisation.
 * Refused (MD2_ERR_ARG): NULL desc, disp, rgb or workspace, a non-positive size, batch >
 * 65535, out_height * out_width > 2^24 (f32(n-1) must be exact), in_height * in_width >=
 * 2^31, a percentile outside 0..100, non-zero flags, a workspace not 256-byte aligned.
 * workspace: the size the query returns (the resized maps, histograms, partials), no
 * initialisation needed.
 */
typedef struct md2_viz_desc {
    int32_t batch;                  /* B images, 1..65535 */
    int32_t in_height, in_width;    /* of disp */
    int32_t out_height, out_width;  /* H, W of the picture */
    int32_t percentile;             /* 0..100; the reference uses 95 */
    uint32_t flags;                 /* none defined yet: non-zero is refused */
    int32_t reserved;               /* 0; the struct is 32 bytes */
} md2_viz_desc;

/* 0 (and md2_last_error) for a desc md2_disp_colorize would refuse */
size_t md2_disp_colorize_workspace_bytes(const md2_viz_desc* desc);
int md2_disp_colorize(const md2_viz_desc* desc, const float* disp, uint8_t* rgb, float* resized, float* stats,
                      void* workspace, void* stream);

/*
 * The ResNet stem's BatchNorm elementwise passes folded into their neighbours
 * (csrc/bnorm.hip, csrc/stem.hip; networks/resnet_encoder.py:62-98 conv1 -> bn1 -> relu ->
 * maxpool).  New symbols under ABI 24, no version bump (as md2_disp_colorize).  Every
 * output is bit for bit what the unfused launches give; all calls are hipGraph-capturable
 * (no allocation, no host synchronisation).
 *
 * md2_bn_pool_fwd = md2_bn_fwd_mask (statistics and finaliser launches unchanged) whose
 * apply pass also is md2_maxpool3s2_fwd: it reads x once and writes the pooled map
 * (batch, height/2, width/2, channels), the pool's idx words, relu_mask, and y only when y
 * is not NULL (a caller that uses the pooled map alone never materialises y).
 * desc->pixels = batch * height * width.  Takes fp32, MD2_BN_RELU alone, even height and
 * width, batch * height / 2 <= 65535 (md2_bn_pool_fwd_supported: 1 / 0); anything else is
 * refused and runs as the two calls.
 *
 * md2_bn_bwd_reduce_mask = md2_bn_bwd_mask without its last launch: grad_gamma,
 * grad_beta, and the three dx coefficient rows coef[3][groups][channels] (γ·invstd,
 * Σg'/N, Σg'x̂/N·invstd) left in the workspace at byte offset md2_bn_coef_offset(desc).
 * md2_stem_wgrad_bn = md2_stem_wgrad whose grad_y is that BatchNorm's missing dx, formed
 * on load from grad (the gradient of relu(bn(z))), z, relu_mask, save_mean and coef in
 * md2_bn_bwd_mask's expressions — dx is never written.  It must follow its
 * md2_bn_bwd_reduce_mask on the same stream with no other BatchNorm call on that
 * workspace in between.  fp32, channels 3 / 6 (md2_stem_wgrad_bn_supported: 1 / 0).
 */
int md2_bn_pool_fwd_supported(const md2_bn_desc* desc, int height, int width);
int md2_bn_pool_fwd(const md2_bn_desc* desc, int height, int width, const float* x, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, float* y, uint8_t* relu_mask,
                    float* pooled, uint32_t* idx, float* save_mean, float* save_invstd, void* workspace,
                    void* stream);
int md2_bn_bwd_reduce_mask(const md2_bn_desc* desc, const void* x, const uint8_t* relu_mask, const void* grad_y,
                           const float* gamma, const float* save_mean, const float* save_invstd, float* grad_gamma,
                           float* grad_beta, void* workspace, void* stream);
size_t md2_bn_coef_offset(const md2_bn_desc* desc);
int md2_stem_wgrad_bn_supported(const md2_stem_desc* desc);
int md2_stem_wgrad_bn(const md2_stem_desc* desc, const float* x, const float* grad, const float* z,
                      const uint8_t* relu_mask, const float* save_mean, const float* coef, int bn_groups,
                      float* grad_weight, void* workspace, void* stream);

/*
 * 16-bit depth maps for the KITTI depth-prediction benchmark (csrc/eval.hip): the
 * reference's export loop, evaluate_depth.py:148-163 — cv2.resize of the scaled disparity
 * to 1216 x 352, depth = 5.4 / disp, clip to [0, 80], uint16(depth * 256), per image on the
 * host — for a batch in one launch on `stream`.  New symbols under ABI 24, no version bump
 * (as md2_disp_colorize).
 *
 * disp (B,1,in_height,in_width): the network's sigmoid output; disp_flipped: the same for
 * the horizontally flipped images (MD2_DEPTH16_POST_PROCESS; else may be NULL); out:
 * uint16 (B,out_height,out_width) contiguous, 2-byte aligned, written completely.  Per
 * output pixel, with md2_depth_eval's own device functions:
 *   - the four neighbours' scaled disparities, fp32 product then fp32 sum (disp_to_depth
 *     with min_depth / max_depth; 1 and INFINITY make it the identity), blended in fp64
 *     with batch_post_process_disparity's masks when asked;
 *   - r = the half-pixel bilinear weights of md2_depth_eval applied in fp64, with
 *     in_height / out_height and in_width / out_width;
 *   - v = scale_factor / r, v = min(max(v, 0), clip_max); out = (uint16)(v * quant),
 *     truncated toward zero.
 * Where the reference leaves the result to numpy's undefined float-to-integer casts this
 * build defines it: r == +0 gives clip_max * quant, r < 0 (and -0) gives 0, NaN gives 0.
 * No workspace, no atomics: bitwise repeatable, hipGraph-capturable.
 * Refused (MD2_ERR_ARG): NULL desc, disp or out (or disp_flipped with the flag), a
 * non-positive size, batch > 65535, batch * in_height * in_width or batch * out_height *
 * out_width at or above 2^31, unknown flag bits, a non-zero reserved field, min_depth /
 * max_depth not 0 < min < max, a scale_factor, clip_max or quant that is not positive and
 * finite, clip_max * quant > 65535, an odd `out` address.
 */
#define MD2_DEPTH16_POST_PROCESS (1u << 0)

typedef struct md2_depth16_desc {
    int32_t batch;                  /* B images, 1..65535 */
    int32_t in_height, in_width;    /* of disp */
    int32_t out_height, out_width;  /* of out; the benchmark's maps are 352 x 1216 */
    uint32_t flags;                 /* MD2_DEPTH16_* */
    double min_depth, max_depth;    /* of disp_to_depth, Python doubles as in md2_eval_desc; offset 24 */
    double scale_factor;            /* the reference's STEREO_SCALE_FACTOR, 5.4 (offset 40) */
    double clip_max;                /* MAX_DEPTH, 80 */
    double quant;                   /* counts per metre, 256 */
    int64_t reserved;               /* 0; the struct is 72 bytes */
} md2_depth16_desc;

/* MD2_OK, or MD2_ERR_ARG (and md2_last_error) for a desc md2_depth_export16 would refuse:
 * the op has no workspace query to ask, and a caller sizes `out` from the desc */
int md2_depth_export16_check(const md2_depth16_desc* desc);
int md2_depth_export16(const md2_depth16_desc* desc, const float* disp, const float* disp_flipped, uint16_t* out,
                       void* stream);

/*
 * Baseline JPEG frames decoded on the device (csrc/jpeg.hip) for training from disk: the
 * host parses the headers (monodepth2_amd/jpeg_ops.py) and uploads the entropy-coded
 * segments with the byte stuffing removed; Huffman decoding, dequantisation, the inverse
 * DCT, chroma upsampling and the colour conversion run here and write the tight (h, w, 3)
 * frames md2_aug_run_mixed reads.  Every byte is what libjpeg's accurate-integer path (the
 * one Pillow uses) gives for the file: jidctint's islow transform, the fancy upsamplers on
 * the cropped component planes with plain replication when the cropped chroma plane is at
 * most two samples wide, and the 16-bit fixed-point YCbCr -> RGB tables.  Integer
 * arithmetic only.  New symbols under ABI 24, no version bump (as md2_depth_export16).
 *
 * streams: device bytes; image i's unstuffed segment is stream_bytes bytes at
 * stream_offset (a multiple of 4; whole 32-bit words are fetched, so the range is rounded
 * up to 4 and must stay inside streams_bytes; what lies behind the last byte is masked).
 * images: HOST array of n, staged through a pinned ring owned by the plan and uploaded on
 * `stream` (the call does not wait for the GPU; a plan is not thread-safe and its calls
 * belong on one stream, since they share its workspace).  bank: DEVICE tables the images
 * index per component: quant, num_quant x 64 uint16 in natural (row-major) order, 16-byte
 * aligned; huff, num_huff x 272 bytes, the 16 code counts by length then 256 symbol values,
 * as a DHT segment lists them.  out: device bytes; frame i is written at out_offset (a
 * multiple of 16), nothing else of out is touched.  status: device uint32[n], written by
 * the call: 0, or MD2_JPEG_ST_* bits when the stream did not decode to exactly the image's
 * blocks (the frame is then unspecified; the other frames of the batch are unaffected).
 *
 * A fixed chain of launches for the whole batch (memset, entropy, DC scan, inverse DCT,
 * colour), hipGraph-unfriendly only in the descriptor upload.  Entropy decoding is parallel
 * within an image without restart markers: the stream is cut into 128-byte subsequences
 * whose entry states converge by a fixed-point iteration to those of the sequential decode
 * (csrc/jpeg.hip), so the result does not depend on scheduling: two runs are bit-equal.
 * Refused (MD2_ERR_ARG) before anything is launched: NULL arguments, n < 1 or n > 4096 or
 * above the plan's, a height or width outside 1..8192, an unknown sampling class, a stream
 * above 2^28 bytes, a table index outside the bank, a misaligned offset, a stream or frame
 * that leaves its buffer, a batch that needs more workspace than the plan owns.
 * Overlapping frames are not refused.  md2_jpeg_check runs the same checks alone.
 */
#define MD2_JPEG_444 0   /* sampling factors 1x1, 1x1, 1x1 */
#define MD2_JPEG_422 1   /* 2x1, 1x1, 1x1 */
#define MD2_JPEG_420 2   /* 2x2, 1x1, 1x1 */

#define MD2_JPEG_ST_BLOCKS (1u << 0)   /* the stream holds fewer or more blocks than the image */
#define MD2_JPEG_ST_CODE   (1u << 1)   /* a bit pattern that is no Huffman code */
#define MD2_JPEG_ST_END    (1u << 2)   /* a symbol reaches past the end of the stream */
#define MD2_JPEG_ST_INDEX  (1u << 3)   /* md2_jpeg_run_indexed: the index does not fit the stream */

typedef struct md2_jpeg_image {
    uint64_t stream_offset;         /* bytes into streams, a multiple of 4 */
    uint64_t out_offset;            /* bytes into out, a multiple of 16 */
    uint32_t stream_bytes;          /* of the unstuffed entropy-coded segment */
    int32_t height, width;          /* 1..8192 */
    int32_t sampling;               /* MD2_JPEG_444 / 422 / 420 */
    uint8_t quant[3];               /* per component: index into bank.quant */
    uint8_t dc[3], ac[3];           /* per component: indices into bank.huff */
    uint8_t reserved[7];            /* 0; the struct is 48 bytes */
} md2_jpeg_image;

typedef struct md2_jpeg_bank {
    const void* quant;
    const void* huff;
    int32_t num_quant, num_huff;    /* 1..256 each */
} md2_jpeg_bank;

typedef struct md2_jpeg_plan md2_jpeg_plan;

/* Device scratch a batch needs (coefficients, sample planes, subsequence states): 0 (and
 * md2_last_error) for a batch md2_jpeg_run would refuse on its geometry. */
size_t md2_jpeg_workspace_bytes(const md2_jpeg_image* images, int n);
int md2_jpeg_check(const md2_jpeg_image* images, int n, int num_quant, int num_huff, uint64_t streams_bytes,
                   uint64_t out_bytes);
/* Allocates the workspace on the current device and the pinned descriptor ring for up to
 * max_images images.  NULL on error. */
md2_jpeg_plan* md2_jpeg_plan_create(int max_images, size_t workspace_bytes);
void md2_jpeg_plan_destroy(md2_jpeg_plan* plan);
int md2_jpeg_run(md2_jpeg_plan* plan, const uint8_t* streams, uint64_t streams_bytes, const md2_jpeg_image* images,
                 int n, const md2_jpeg_bank* bank, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream);

/*
 * Decoding from a stored synchronisation index (csrc/jpeg.hip; monodepth2_amd/pack.py keeps
 * the index beside each stream).  The entry states md2_jpeg_run's entropy kernel finds by
 * fixed-point iteration are a property of the file, so they are computed once
 * (md2_jpeg_index) and every later decode (md2_jpeg_run_indexed) starts each 1024-bit
 * subsequence of every image from its stored state, one thread per subsequence, workgroups
 * over (image, group of subsequences): no rounds, no barrier after the Huffman tables are
 * built, the whole batch spread over the GPU.  New symbols under ABI 24, no version bump
 * (as md2_jpeg_run).
 *
 * An image's index, for nsub = max(ceil(8 * stream_bytes / 1024), 1) subsequences: nsub
 * uint64 entry states (bit << 16 | block_in_mcu << 8 | zigzag: the decoder's state at the
 * first symbol that starts at or after bit 1024 i), then nsub uint32 first_block values
 * (the blocks completed before that state), zero padded to a multiple of 16 bytes:
 * md2_jpeg_index_bytes(stream_bytes), 12 bytes per 128 stream bytes.  md2_jpeg_image stays as
 * it is; where each image's index lies travels as a parallel HOST array index_offsets[n]
 * (multiples of 16).
 *
 * md2_jpeg_index: images, streams, bank, status and plan as for md2_jpeg_run (out_offset is
 * not used; the plan needs md2_jpeg_workspace_bytes of the batch); runs the synchronisation
 * alone, writes no frame, and writes image i's index at index + index_offsets[i] (`index`: DEVICE
 * bytes, 16-byte aligned, index_bytes long).  status: 0, or MD2_JPEG_ST_BLOCKS when the
 * stream does not hold exactly the image's blocks.
 *
 * md2_jpeg_run_indexed: as md2_jpeg_run, with image i's index read from streams +
 * index_offsets[i] (streams 16-byte aligned).  The chain is memset, the indexed entropy
 * kernel, then md2_jpeg_run's DC scan, inverse DCT and colour kernels; with its true index a
 * stream that holds exactly its image's blocks gives md2_jpeg_run's bytes and status 0 (one
 * that does not reports MD2_JPEG_ST_INDEX beside md2_jpeg_run's bits: a short stream and a
 * wrong last count cannot be told apart).  The index is not trusted: every
 * subsequence checks its entry state's range, its exit state against the next entry and its
 * block count against the next first_block (the last against the image's blocks); a
 * mismatch sets MD2_JPEG_ST_INDEX in the image's status word, the frame is then unspecified
 * and the other frames of the batch are unaffected.  Whatever the index says, reads stay
 * inside streams and writes inside the image's own coefficient planes.  Refused
 * (MD2_ERR_ARG) before anything is launched: what md2_jpeg_run refuses, NULL index_offsets,
 * an index offset that is no multiple of 16, an index that leaves streams_bytes.
 * md2_jpeg_check_indexed runs those checks alone.
 */
size_t md2_jpeg_index_bytes(uint32_t stream_bytes);
int md2_jpeg_index(md2_jpeg_plan* plan, const uint8_t* streams, uint64_t streams_bytes, const md2_jpeg_image* images,
                   const uint64_t* index_offsets, int n, const md2_jpeg_bank* bank, uint8_t* index,
                   uint64_t index_bytes, uint32_t* status, void* stream);
int md2_jpeg_check_indexed(const md2_jpeg_image* images, const uint64_t* index_offsets, int n, int num_quant,
                           int num_huff, uint64_t streams_bytes, uint64_t out_bytes);
int md2_jpeg_run_indexed(md2_jpeg_plan* plan, const uint8_t* streams, uint64_t streams_bytes,
                         const md2_jpeg_image* images, const uint64_t* index_offsets, int n,
                         const md2_jpeg_bank* bank, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream);

/*
 * Baseline JPEG encoding on the device (csrc/jpegenc.hip): the other half of md2_jpeg_run.
 * Tight (h, w, 3) uint8 RGB frames of mixed sizes -> the entropy-coded segment of each,
 * UNSTUFFED (no FF 00; what md2_jpeg_image.stream_bytes describes and a pack record holds),
 * the last partial byte filled with 1-bits.  Every byte is what libjpeg's default integer
 * path (the one Pillow uses) writes for the frame at the same tables and sampling: 16-bit
 * fixed-point RGB -> YCbCr, box downsampling with the alternating bias (no smoothing), edges
 * by repetition, jfdctint's islow forward transform, quantisation by 8 q rounding half away
 * from zero, one interleaved scan without restart markers, the four standard Huffman tables
 * of ITU-T T.81 Annex K (compiled in; there are no optimised tables).  The host writes the
 * file around the segment (monodepth2_amd/jpeg_ops.py).  Integer arithmetic only; the only
 * atomics are integer ORs on the words two neighbouring blocks share: two runs are
 * bit-equal.  New symbols under ABI 24, no version bump (as md2_jpeg_index).
 *
 * in: device bytes; frame i is height * width * 3 bytes at in_offset.  images: HOST array of
 * n, read for the checks and the launch sizes only; dev_images: a DEVICE copy of the same
 * array (8-byte aligned), which the kernels read, so the caller uploads it with the frames
 * and the call stages nothing.  quant: DEVICE bank of num_quant tables of 64 uint16 in
 * natural (row-major) order, the layout of md2_jpeg_bank.quant; an image names its luma and
 * its chroma table.  out: device bytes, 16-byte aligned; image i owns out_capacity bytes at
 * out_offset (a multiple of 16).  Whole 32-bit words take the OR, so a range is rounded up
 * to 4 bytes for the bounds check against out_bytes (rounded up likewise); the bytes of that
 * last word beyond the capacity are OR-ed with zeros and keep their value.  workspace:
 * device bytes, 256-byte aligned, md2_jpeg_encode_workspace_bytes of the batch, no
 * initialisation needed.  stream_bytes, status: device uint32[n], written by the call:
 * the stream's length (also when it does not fit, so the caller can size a second call) and
 * 0 or MD2_JPEGENC_ST_SPACE.  A stream that does not fit its capacity writes nothing of its
 * range; no byte outside an image's range is written in either case and the other images of
 * the batch are unaffected.  Bit offsets are 64-bit, so no batch is too long.
 *
 * A fixed chain of launches on `stream` (setup, dct + quantise, bit count, per-image scan,
 * zero, emit): no allocation, no host synchronisation, hipGraph-capturable.  Refused
 * (MD2_ERR_ARG) before anything is launched: NULL arguments, n outside 1..4096, a height or
 * width outside 1..8192, an unknown sampling class, num_quant outside 1..256, a table index
 * outside the bank, a frame that leaves in_bytes, an out_offset that is no multiple of 16,
 * an output range that leaves out_bytes, misaligned buffers, a workspace that is too small.
 * md2_jpeg_encode_check runs the checks that need no pointer alone (host only, launches
 * nothing).  md2_jpeg_encode_bound: a capacity no stream of that geometry exceeds (a block
 * is at most 20 + 63 * 26 = 1658 bits: 208 bytes per block, dummy blocks included), 0 (and
 * md2_last_error) for a geometry the encoder refuses.
 */
#define MD2_JPEGENC_ST_SPACE (1u << 0)   /* the stream does not fit out_capacity */

typedef struct md2_jpegenc_image {
    uint64_t in_offset;             /* bytes into in: the tight (height, width, 3) frame */
    uint64_t out_offset;            /* bytes into out, a multiple of 16 */
    uint32_t out_capacity;          /* bytes of the output range */
    int32_t height, width;          /* 1..8192 */
    int32_t sampling;               /* MD2_JPEG_444 / 422 / 420 */
    uint8_t quant[2];               /* luma, chroma: indices into the quant bank */
    uint8_t reserved[6];            /* 0; the struct is 40 bytes */
} md2_jpegenc_image;

size_t md2_jpeg_encode_bound(int height, int width, int sampling);
size_t md2_jpeg_encode_workspace_bytes(const md2_jpegenc_image* images, int n);
int md2_jpeg_encode_check(const md2_jpegenc_image* images, int n, int num_quant, uint64_t in_bytes,
                          uint64_t out_bytes);
int md2_jpeg_encode(const uint8_t* in, uint64_t in_bytes, const md2_jpegenc_image* images,
                    const md2_jpegenc_image* dev_images, int n, const uint16_t* quant, int num_quant, uint8_t* out,
                    uint64_t out_bytes, void* workspace, size_t workspace_bytes, uint32_t* stream_bytes,
                    uint32_t* status, void* stream);

/*
 * 8-bit RGB PNG frames decoded on the device (csrc/png.hip): the last host-side decoder on
 * the way from a KITTI tree to the training step.  The host reads the chunks, checks their
 * CRCs and the zlib header (monodepth2_amd/png_ops.py) and uploads, per file, the
 * concatenated IDAT payload without its 2-byte zlib header: the raw deflate stream followed
 * by the 4 bytes of the Adler-32 trailer.  The device inflates it (RFC 1951: stored, fixed
 * and dynamic blocks, every stream zlib's inflate accepts) into the caller's workspace and
 * then undoes the five scanline filters (bpp = 3) into the tight (height, width, 3) frame,
 * every byte what Pillow's Image.open(path).convert("RGB") gives; the same pass forms the
 * Adler-32 of the scanlines and compares it with the trailer.  Integer arithmetic only, no
 * atomics: two runs are bit-equal.  New symbols under ABI 24, no version bump (as
 * md2_jpeg_encode).
 *
 * streams: device bytes, 16-byte aligned; image i's stream is stream_bytes bytes at
 * stream_offset (a multiple of 16).  images: HOST array of n, read for the checks and the
 * launch sizes only; dev_images: a DEVICE copy of it (8-byte aligned), which the kernels
 * read, so the caller uploads it with the streams and the call stages nothing.  workspace:
 * device bytes, 16-byte aligned, md2_png_workspace_bytes of the batch (the inflated
 * scanlines, height * (1 + 3 width) bytes per image rounded up to 16), no initialisation
 * needed.  out: device bytes; frame i is written at out_offset (a multiple of 16) and no
 * other byte of out is.  status: device uint32[n], written by the call: 0, or
 * MD2_PNG_ST_* bits.  Decoding stops at the image's last byte, so stream bytes after a
 * complete image set no bit (Pillow ignores them too).  With a bit of the inflate stage set
 * (BLOCK, CODE, END, DIST) the frame is not written at all; with FILTER or ADLER alone it is
 * written (a row with a bad filter byte as if its filter were None).  A corrupt stream writes
 * nothing outside its own workspace range and its own status word, and the other images of
 * the batch are unaffected.
 *
 * Two launches on `stream` (inflate: one wave per stream; unfilter + Adler-32: one wave per
 * image), no allocation, no host synchronisation, hipGraph-capturable.  Refused
 * (MD2_ERR_ARG) before anything is launched: n outside 0..4096, NULL arguments, a height or
 * width outside 1..8192, a stream_offset or out_offset that is no multiple of 16, a stream
 * that leaves streams_bytes, a frame that leaves out_bytes, misaligned buffers, a workspace
 * that is too small.  md2_png_check runs the checks that need no pointer alone (host only,
 * launches nothing).  md2_png_workspace_bytes: 0 (and md2_last_error) for a geometry the
 * decoder refuses.
 */
#define MD2_PNG_ST_BLOCK  (1u << 0)  /* block type 3, or a stored block whose LEN and NLEN disagree */
#define MD2_PNG_ST_CODE   (1u << 1)  /* a code-length set zlib's inflate refuses, a bit pattern that is no code,
                                        literal/length symbols 286/287, distance symbols 30/31 */
#define MD2_PNG_ST_END    (1u << 2)  /* the stream ends before the image is complete */
#define MD2_PNG_ST_DIST   (1u << 3)  /* a distance reaching before the first output byte */
#define MD2_PNG_ST_FILTER (1u << 4)  /* a row's filter byte above 4 */
#define MD2_PNG_ST_ADLER  (1u << 5)  /* the trailer is not the Adler-32 of the h * (1 + 3w) raw bytes */

typedef struct md2_png_image {
    int32_t height, width;          /* 1..8192 */
    uint64_t out_offset;            /* bytes into out, a multiple of 16: the tight (height, width, 3) frame */
    uint64_t stream_offset;         /* bytes into streams, a multiple of 16 */
    uint32_t stream_bytes;          /* the deflate stream and the 4 trailer bytes */
    uint32_t reserved;              /* 0; the struct is 32 bytes */
} md2_png_image;

size_t md2_png_workspace_bytes(const md2_png_image* images, int n);
int md2_png_check(const md2_png_image* images, int n, uint64_t streams_bytes, uint64_t out_bytes);
int md2_png_run(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                const md2_png_image* dev_images, int n, uint8_t* workspace, size_t workspace_bytes, uint8_t* out,
                uint64_t out_bytes, uint32_t* status, void* stream);

/*
 * The indexed PNG decoder (csrc/png.hip): md2_png_run decodes a stream serially, so a call
 * lasts as long as one stream.  Where a stream's symbols start is a property of the file: it
 * is found once (md2_png_index, when a frame pack is built) and stored beside the stream;
 * md2_png_run_indexed then inflates all segments of all streams at the same time.  New
 * symbols under ABI 24, no version bump.
 *
 * The index of a stream cuts its output, the height * (1 + 3 width) scanline bytes, into
 * consecutive segments for one value of segment_bytes, S: a power of two in 1024..32768.
 * Walking the stream as md2_png_run does, a boundary candidate is a block header, the start
 * of a literal/length symbol (the end-of-block symbol included) in a fixed or dynamic block,
 * and every byte of a stored block.  Segment 0 starts at bit 0 and output 0; a new segment
 * starts at the first candidate at which the current one has produced at least S bytes, so
 * every segment but the last holds S..S + 257 bytes and there are at most raw_bytes / S + 1.
 * No segment starts at the image's end.  The layout (little-endian, fixed per geometry and S):
 *
 *   bytes 0..15   u32 count (segments; 0: the stream did not inflate, nothing decodes from
 *                 this index), u32 segment_bytes, 8 zero bytes
 *   then          raw_bytes / S + 1 entries of 24 bytes, the first `count` in use, the rest 0:
 *                   u64 header_bit   bit offset of the 3-bit header of the block the segment starts in
 *                   u64 symbol_bit   bit offset of the segment's first symbol (a stored block:
 *                                    of its first byte; at a block's start: header_bit)
 *                   u32 out_pos      output position of the segment's first byte
 *                   u32 0
 *   zeros up to a multiple of 16: md2_png_index_bytes(height, width, segment_bytes) in all
 *   (0 and md2_last_error for a geometry or an S the decoder refuses).
 *
 * md2_png_index: streams, images and dev_images as for md2_png_run (out_offset is not used);
 * makes the index alone with md2_png_run's serial walk (one wave per stream, no byte of the
 * frame is produced) and writes image i's index at index + index_offsets[i] (`index`: DEVICE
 * bytes, 16-byte aligned, index_bytes long; index_offsets: HOST array of n multiples of 16,
 * dev_index_offsets a DEVICE copy of it, 8-byte aligned, as dev_images is of images).
 * status: the bits of md2_png_run's inflate stage (BLOCK, CODE, END, DIST); a stream with a
 * bit set gets count 0.  FILTER and ADLER are not looked at.
 *
 * md2_png_run_indexed: md2_png_run's contract, with image i's index read from streams +
 * index_offsets[i] (where a pack record's bytes put it: behind the stream) and a workspace of
 * md2_png_indexed_workspace_bytes (the scanlines as for md2_png_run, a 16-bit symbol per
 * scanline byte, a status word per segment; 16-byte aligned, no initialisation needed).
 * Three launches on `stream`, ordered by their boundaries alone (no workgroup waits for
 * another's memory), no allocation, no host synchronisation, hipGraph-capturable:
 *   segments  one wave per (image, segment), the grid as wide as the batch's largest
 *             capacity: re-reads the block header at header_bit, rebuilds its tables, seeks to
 *             symbol_bit and decodes up to the next entry's out_pos (the last: the image's
 *             end) into 16-bit symbols held in LDS (S + 257 positions): b for a known byte,
 *             0x8000 | k for "the byte k + 1 before this segment's start" (k in 0..32767: every
 *             legal distance); a copy from inside the segment copies symbols
 *   resolve   one workgroup per image: ORs the segments' status words into the image's;
 *             if that is 0, turns symbols into bytes segment after segment behind its own
 *             barrier, so a reference through several segments finds a final byte
 *   unfilter  md2_png_run's second launch, unchanged
 * The index is not trusted.  Every wave checks its entry (bits inside the stream, header_bit
 * <= symbol_bit, out_pos ascending, inside the image and at most S + 257 before the next,
 * entry 0 at bit 0 and output 0, count within capacity, the stored S the call's) and its exit against
 * the next entry (exactly on out_pos, the same symbol_bit, in the same block), and that it
 * met no candidate S or more bytes into its range (a boundary the index lacks); a mismatch
 * sets MD2_PNG_ST_INDEX in the image's status word, a distance reaching before byte 0
 * MD2_PNG_ST_DIST.  Whatever the index says, a wave writes only the symbols of its own output
 * range and its own status word, and reads stay inside streams.  With an inflate-stage bit
 * or INDEX set the frame is not written, and the other images are unaffected.  With its true
 * index a stream gives md2_png_run's bytes and status exactly.
 *
 * Refused (MD2_ERR_ARG) before anything is launched: what md2_png_run refuses, NULL
 * index_offsets or dev_index_offsets, an index offset that is no multiple of 16, an index that
 * leaves streams_bytes, a segment_bytes that is no power of two in 1024..32768.
 * md2_png_check_indexed runs the checks that need no device pointer alone (host only).
 */
#define MD2_PNG_ST_INDEX  (1u << 6)  /* the index does not fit the stream (md2_png_run_indexed) */

size_t md2_png_index_bytes(int height, int width, int segment_bytes);
size_t md2_png_indexed_workspace_bytes(const md2_png_image* images, int n, int segment_bytes);
int md2_png_index(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                  const md2_png_image* dev_images, int n, int segment_bytes, uint8_t* index, uint64_t index_bytes,
                  const uint64_t* index_offsets, const uint64_t* dev_index_offsets, uint32_t* status, void* stream);
int md2_png_check_indexed(const md2_png_image* images, const uint64_t* index_offsets, int n, int segment_bytes,
                          uint64_t streams_bytes, uint64_t out_bytes);
int md2_png_run_indexed(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                        const md2_png_image* dev_images, const uint64_t* index_offsets,
                        const uint64_t* dev_index_offsets, int n, int segment_bytes, uint8_t* workspace,
                        size_t workspace_bytes, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream);

/*
 * PNG encoding on the device (csrc/pngenc.hip): the other half of md2_png_run.  Tight
 * (height, width, 3) uint8 RGB frames (MD2_PNGENC_RGB8: colour type 2, depth 8) and (height,
 * width) 16-bit grey maps in host byte order (MD2_PNGENC_GRAY16: colour type 0, depth 16,
 * written big-endian; int16 storage holds the uint16 bit patterns, as md2_depth_export16
 * leaves them), of mixed sizes and kinds -> the complete zlib stream of each file's IDAT chunk
 * (2-byte header, deflate blocks, Adler-32).  The host writes the signature, IHDR, IDAT, IEND
 * and their CRCs around it (monodepth2_amd/png_ops.py).  The bytes follow the format rules of
 * DESIGN.md §6n (per-row filter choice, segments of segment_bytes filtered bytes that are
 * compressed independently, one deflate block each and an empty stored block behind every
 * segment but the last, the candidate and parse rule, the code construction); they are not
 * zlib's bytes, and every stream is one zlib's inflate accepts.  Integer arithmetic only;
 * the atomics are integer (LDS max/add, OR on a wave's own zeroed words): two runs are
 * bit-equal.  New symbols under ABI 24, no version bump (as md2_jpeg_encode).
 *
 * in: device bytes, 2-byte aligned; frame i is height * width * 3 (RGB8) or * 2 (GRAY16)
 * bytes at in_offset (GRAY16: a multiple of 2).  images: HOST array of n, read for the checks
 * and the launch sizes only; dev_images: a DEVICE copy of the same array (8-byte aligned),
 * which the kernels read.  workspace: device bytes, 256-byte aligned,
 * md2_png_encode_workspace_bytes of the batch, no initialisation needed; image i's range
 * starts at ws_offset, which must be the sum of md2_png_encode_workspace_bytes(&images[k], 1)
 * over k < i.  out: device bytes; image i owns out_capacity bytes at out_offset (any
 * alignment).  stream_bytes, status: device uint32[n], written by the call: the stream's
 * length (also when it does not fit, so the caller can size a second call) and 0 or
 * MD2_PNGENC_ST_SPACE.  A stream that does not fit its capacity writes nothing of its range;
 * no byte outside an image's range is written in either case and the other images of the
 * batch are unaffected.
 *
 * Three launches on `stream` (filter + row sums: one wave per row; deflate: one wave per
 * segment; pack: one block per image), no allocation, no host synchronisation,
 * hipGraph-capturable.  Refused (MD2_ERR_ARG) before anything is launched: NULL arguments, n
 * outside 1..4096, a height or width outside 1..8192, an unknown kind, a segment_bytes that is
 * no power of two in 1024..32768, a frame that leaves in_bytes, an odd in_offset of a 16-bit
 * frame, an output range that leaves out_bytes, a ws_offset that is not the running sum, a
 * non-zero reserved word, misaligned buffers, a workspace that is too small.
 * md2_png_encode_check runs the checks that need no pointer alone (host only, launches
 * nothing).  md2_png_encode_bound: a capacity no stream of that geometry exceeds (every
 * segment stored, n + 5, and flushed, 5; header 2 and trailer 4: total + 10 * segments + 6),
 * 0 (and md2_last_error) for a geometry the encoder refuses.
 */
#define MD2_PNGENC_RGB8   0
#define MD2_PNGENC_GRAY16 1
#define MD2_PNGENC_ST_SPACE (1u << 0)   /* the stream does not fit out_capacity */

typedef struct md2_pngenc_image {
    uint64_t in_offset;             /* bytes into in: the tight frame */
    uint64_t out_offset;            /* bytes into out */
    uint64_t ws_offset;             /* bytes into workspace: the running sum of the images before */
    uint32_t out_capacity;          /* bytes of the output range */
    int32_t height, width;          /* 1..8192 */
    int32_t kind;                   /* MD2_PNGENC_RGB8 / MD2_PNGENC_GRAY16 */
    int32_t segment_bytes;          /* S: a power of two in 1024..32768 */
    uint32_t reserved;              /* 0; the struct is 48 bytes */
} md2_pngenc_image;

size_t md2_png_encode_bound(int height, int width, int kind, int segment_bytes);
size_t md2_png_encode_workspace_bytes(const md2_pngenc_image* images, int n);
int md2_png_encode_check(const md2_pngenc_image* images, int n, uint64_t in_bytes, uint64_t out_bytes);
int md2_png_encode(const uint8_t* in, uint64_t in_bytes, const md2_pngenc_image* images,
                   const md2_pngenc_image* dev_images, int n, void* workspace, size_t workspace_bytes, uint8_t* out,
                   uint64_t out_bytes, uint32_t* stream_bytes, uint32_t* status, void* stream);

/*
 * The training log's pictures (csrc/md2hot.hip): what the reference's Trainer.log writes at
 * a log step (trainer.py:540-572, with normalize_image, utils.py:22-28) for the first
 * `items` images of the batch, as one uint8 contact sheet (items, sheet_h, sheet_w, 3) filled
 * on the device in two launches on `stream`: per-(item, scale) disparity minimum and maximum
 * (one block each; its other blocks clear the sheet), then one table-driven launch that
 * writes every tile.  New symbols under ABI 24, no version bump (as md2_jpeg_run).
 *
 * A tile is a rectangle of the sheet of item `item`; tiles are disjoint, everything outside
 * them is written 0 (the caller does not clear the sheet).  Kinds, with (h_s, w_s) =
 * (height >> s, width >> s):
 *   MD2_LOG_COLOR  src: fp32 (3, h_s, w_s) planes, inputs[("color", frame, s)][item]; R, G, B.
 *   MD2_LOG_WARP   outputs[("color", frame, 0)][item] (trainer.py:384-387) for source frame
 *                  `frame` (1..S), scale 0 only, computed here from tensors->disp[0], color[0],
 *                  K[0], inv_K[0] and T (the scale-0 T with MD2_T_PER_SCALE) with
 *                  md2_generate_images's own device functions: bit-equal to quantising its
 *                  color_out.  src: color[0][frame] + item * 3 * height * width.
 *   MD2_LOG_DISP   normalize_image(outputs[("disp", s)][item]); src: that map, (h_s, w_s),
 *                  fp32 or bf16 by desc.hot.disp_dtype (bf16 is widened exactly), and
 *                  tensors->disp[s] must be the batch it belongs to (the statistics are
 *                  taken from there).  With mi, ma the map's minimum and maximum:
 *                  d = fp32(fp64(ma) - fp64(mi)), or 1e5 when ma == mi; v = (x - mi) / d,
 *                  an fp32 subtraction and a correctly rounded fp32 division.  A map that
 *                  holds a NaN has mi = ma = NaN and every byte 0.  Grey.
 *   MD2_LOG_MAP    src: an fp32 (h, w) map written as grey, (h, w) = (h_s, w_s) (a predictive
 *                  mask, trainer.py:562-567) or (height, width) (identity_selection at the
 *                  loss resolution, trainer.py:569-572).
 * Every value becomes a byte as the reference's image writer makes one of a float image:
 * uint8(clip(fp32(x) * 255f, 0, 255)), one fp32 product then truncation; NaN gives 0.  So
 * x = fp32(k / 255) gives k for every k.  Grey tiles repeat the byte in the three channels.
 * Tiles whose x and w are multiples of 4 pixels (and sheet_w too) store whole dwords.
 *
 * tiles: DEVICE array of desc->num_tiles entries in ascending block0, entry e owning grid
 * blocks [block0, block0 + md2_log_panel_tile_blocks(e)); it must be a copy of a host table
 * that md2_log_panel_check accepted.  workspace: md2_log_panel_workspace_bytes, 256-byte
 * aligned, no initialisation needed; after the call its first items * num_scales * 2 floats
 * hold mi, ma per (item, scale).  sheet: 16-byte aligned.  Integer and fp32 arithmetic, no
 * atomics: bitwise repeatable.  hipGraph-capturable, no allocation, no host synchronisation.
 *
 * md2_log_panel_check (host only, touches no device) answers MD2_ERR_ARG for: a NULL desc or
 * table, non-positive sizes, num_scales outside 1..4, num_src outside 1..3, a scale whose
 * map would be empty, items outside 1..MD2_LOG_MAX_ITEMS or above batch, num_tiles outside
 * 1..MD2_LOG_MAX_TILES, a sheet of 2^31 bytes or more, an unknown kind, an item, scale or
 * frame (0..S; warp: 1..S) out of range, a warp tile at a scale other than 0 or in a frame
 * smaller than 2 x 2, a size that does not match kind, scale and desc, a tile that leaves the
 * sheet or overlaps another tile of its item, a NULL src, a block0 that is not the running
 * sum of md2_log_panel_tile_blocks.  tensors may be NULL when the table holds no warp tile;
 * with one, T, disp[0], K[0], inv_K[0] and color[0][1..S] must be set.
 */
#define MD2_LOG_COLOR 0
#define MD2_LOG_WARP  1
#define MD2_LOG_DISP  2
#define MD2_LOG_MAP   3
#define MD2_LOG_MAX_ITEMS 4
#define MD2_LOG_MAX_TILES 1024

typedef struct md2_log_tile {
    int32_t kind;                   /* MD2_LOG_* */
    int32_t item;                   /* image of the batch, 0..items-1 */
    int32_t scale;                  /* 0..num_scales-1 */
    int32_t frame;                  /* 0 = target, 1..S = frame_ids[1:] */
    int32_t y, x, h, w;             /* rectangle in the item's sheet, pixels */
    const void* src;                /* see the kinds above (offset 32) */
    int32_t block0;                 /* first grid block of this tile */
    int32_t reserved;               /* 0; the struct is 48 bytes */
} md2_log_tile;

typedef struct md2_log_desc {
    md2_desc hot;                   /* the step's hot-path descriptor (48 bytes) */
    int32_t items;                  /* n = min(4, batch) */
    int32_t sheet_h, sheet_w;
    int32_t num_tiles;              /* the struct is 64 bytes */
} md2_log_desc;

/* grid blocks of one tile: ceil(h * ceil(w / 4) / 256), one thread per 4-pixel run of a row */
int md2_log_panel_tile_blocks(const md2_log_tile* tile);
int md2_log_panel_check(const md2_log_desc* desc, const md2_log_tile* tiles_host, const md2_tensors* tensors);
/* 0 (and md2_last_error) for a desc md2_log_panel would refuse */
size_t md2_log_panel_workspace_bytes(const md2_log_desc* desc);
int md2_log_panel(const md2_log_desc* desc, const md2_tensors* tensors, const md2_log_tile* tiles,
                  int total_blocks, uint8_t* sheet, void* workspace, void* stream);

/*
 * Depth maps -> point cloud (csrc/points.hip): the reference's disp_to_depth
 * (layers.py:16-25) and BackprojectDepth (layers.py:139-168) per pixel in fp32, for a batch
 * of equally sized maps at the original image size, with the pixels that are invalid or
 * out of range dropped, the survivors compacted in (image, row, column) order over the whole
 * batch and packed as the 15-byte vertex records of a binary little-endian PLY file: the
 * first 15 * offsets[B] bytes of `vertices` are the file's body.  Three launches on
 * `stream` (count per block, scan of the block counts, emit).  New symbols under ABI 24, no
 * version bump (as md2_disp_colorize).
 *
 * map: fp32 (B, H, W); rgb: uint8 (B, H, W, 3); inv_K: fp32 (B, 4, 4) row-major, only rows
 * and columns 0..2 are read; T: fp32 (B, 4, 4), rows 0..2 are read, required with
 * MD2_POINTS_WORLD and NULL without it; vertices: `capacity` records of 15 bytes, any
 * alignment; offsets: uint32 [B + 1].  All on the device.  Per pixel (b, y, x) with d the
 * map's value, every product and sum one fp32 operation in this order (no contraction):
 *   1. sd = disp_b + disp_a * d
 *   2. depth = 1.0f / sd; with MD2_POINTS_DEPTH_INPUT depth = d (disp_a, disp_b ignored)
 *   3. z = depth_scale * depth
 *   4. r_i = (k[i][0] * (float)x + k[i][1] * (float)y) + k[i][2], i = 0..2, k = inv_K[b]; x
 *      and y are the integer pixel indices (no half-pixel offset, the reference's meshgrid)
 *   5. P_i = z * r_i
 *   6. with MD2_POINTS_WORLD: Q_i = ((t[i][0]*P_0 + t[i][1]*P_1) + t[i][2]*P_2) + t[i][3],
 *      t = T[b], and the record holds Q, else P.
 * A pixel is kept when y % stride == 0 and x % stride == 0, near <= z <= far (both ends
 * inclusive, z in the camera frame, before T) and the three stored coordinates are finite;
 * a NaN fails the comparisons by itself.  A record: x, y, z as little-endian float32, then
 * red, green, blue (the pixel's bytes).  offsets[0] = 0, offsets[b + 1] = the records of
 * images 0..b.  Exactly bytes 0 .. 15 * offsets[B] of `vertices` are written, each once; no
 * byte after them is touched.
 * No atomics, a record's slot comes from the scan: the order is fixed and the output
 * bitwise repeatable.  hipGraph-capturable, no allocation, no host synchronisation.
 * Refused (MD2_ERR_ARG) before any launch: a NULL desc, map, rgb, inv_K, vertices, offsets
 * or workspace; T without MD2_POINTS_WORLD or the flag without T; a non-positive batch,
 * height, width or stride; batch > 65535; batch * ceil(height / stride) * ceil(width /
 * stride) >= 2^31; capacity below that product (so no record can land outside `vertices`
 * whatever the map holds); near or far not finite, near <= 0 or near > far (a sparse map's
 * zeros are never points); a depth_scale that is not positive and finite; unknown flag bits
 * or non-zero reserved words; a workspace not 256-byte aligned.  What cannot be checked:
 * that map, rgb, inv_K, T, vertices, offsets and the workspace are as large as the desc
 * and `capacity` say.
 * workspace: the size the query returns (one word per block), no initialisation needed.
 */
#define MD2_POINTS_DEPTH_INPUT (1u << 0)   /* the map holds depth, not the network's disparity */
#define MD2_POINTS_WORLD (1u << 1)         /* apply T: records in the world frame */

typedef struct md2_points_desc {
    int32_t batch;                  /* B images, 1..65535 */
    int32_t height, width;          /* of map and rgb */
    int32_t stride;                 /* every stride-th row and column; 1: every pixel */
    float disp_a, disp_b;           /* f32(1/min_depth - 1/max_depth), f32(1/max_depth) (offset 16) */
    float depth_scale;              /* 1, or the reference's STEREO_SCALE_FACTOR (offset 24) */
    float near, far;                /* the kept range of z, inclusive (offset 28) */
    uint32_t flags;                 /* MD2_POINTS_* (offset 36) */
    uint32_t reserved[2];           /* 0; the struct is 48 bytes */
} md2_points_desc;

/* 0 (and md2_last_error) for a desc md2_depth_points would refuse */
size_t md2_depth_points_workspace_bytes(const md2_points_desc* desc);
int md2_depth_points(const md2_points_desc* desc, const float* map, const uint8_t* rgb, const float* inv_K,
                     const float* T, uint8_t* vertices, size_t capacity, uint32_t* offsets, void* workspace,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD2HOT_H */
