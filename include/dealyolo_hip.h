/* libdealyolo_hip.so -- C ABI of the MI355X (gfx950) DEAL-YOLO hot path.
 *
 * The reference (adityaX1412/Experiment-YOLO, an Ultralytics-YOLOv8 fork) has NO native code and no FFI on this
 * path: every operator below replaces a *sequence of ATen calls* issued by the reference's Python modules.  Each
 * entry therefore cites the reference Python interface (file:line under /root/reference/ultralytics) whose
 * arithmetic it takes over; INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless named host_*;
 *   - activations are NHWC fp16 ("f16"), addressed as (pointer, ld) where ld is the pixel stride in ELEMENTS, so a
 *     channel slice of a wider buffer (Concat / chunk) is just an offset pointer with the parent's ld;
 *     channel counts and ld are multiples of 8, pointers 16-byte aligned;
 *   - every function enqueues work on `stream` and returns immediately: no allocation, no synchronisation, no
 *     global state; workspaces are caller-owned;  return value: DY_OK (0) or a negative DY_ERR_* code.
 */
#ifndef DEALYOLO_HIP_H
#define DEALYOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define DY_OK 0
#define DY_ERR_ARG (-1)
#define DY_ERR_LAUNCH (-2)
#define DY_ERR_ALIGN (-3)
#define DY_ERR_CAPACITY (-4) /* more items than a kernel's fixed table holds; nothing was launched */

/* A channel CONCATENATION that is never materialised: the tensor's channels [c_end[s-1], c_end[s]) live in segment s, an fp16 NHWC
 * tensor (or channel slice) of its own pixel stride.  C2f's ``torch.cat(y, 1)`` (nn/modules/block.py:222-226), SPPF's and the model's
 * Concat layers (nn/modules/conv.py:338-348) feed 1x1 convolutions only; those read their input, write their input gradient and read
 * their weight-gradient operand through this table, so every concat member stays a contiguous tensor for the kernels that touch it
 * alone (BatchNorm apply / backward reduce, the 3x3 convs of a Bottleneck) instead of a strided slice of a wide buffer. */
#define DY_MAX_SEGS 8
typedef struct DySegs {
  int nseg;                      /* 1..DY_MAX_SEGS */
  int c_end[DY_MAX_SEGS];        /* exclusive end channel of segment s in the concatenated tensor (multiples of 8, increasing) */
  int ld[DY_MAX_SEGS];           /* pixel stride of segment s in elements */
  int acc[DY_MAX_SEGS];          /* as an OUTPUT: 1 = add to what the segment holds (gradient fan-in), 0 = store.  As the INPUT of
                                    dy_conv1x1_forward_segs: 2 = the segment is nn.Upsample(None, 2, 'nearest') of a (n, h/2, w/2) tensor
                                    (ptr / ld are that tensor's): pixel (y, x) reads (y >> 1, x >> 1), the up-sampled copy in front
                                    of the reference's Concat (the head of every cfg/models YAML) is never written */
  const void* ptr[DY_MAX_SEGS];  /* first channel of segment s */
} DySegs;
int dy_segs_bytes(void); /* sizeof(DySegs) in the library (bindings check their layout) */

/* conv epilogue flags */
#define DY_EPI_STATS 1   /* write per-workgroup sum / sum-of-squares partials of the (fp16-rounded) output */
#define DY_EPI_BIAS 2    /* add bias[cout] */
#define DY_EPI_SILU 4    /* apply SiLU */
#define DY_EPI_F32OUT 8  /* y is fp32 (Detect's final 1x1 convs feed the loss in fp32) */
#define DY_EPI_ACCUM 16  /* y += result (gradient fan-in) */
#define DY_EPI_STATS_ACC 32 /* with DY_EPI_STATS: `partials` is a double accumulator [DY_BN_COPIES][2][round16(cout)], zeroed by the
                             * caller, that every workgroup ADDS its sums into (copy = workgroup index % DY_BN_COPIES); consumed by
                             * dy_bn_act_apply_acc -- no dy_bn_finalize launch */
#define DY_BN_COPIES 16

#define DY_ACT_NONE 0
#define DY_ACT_SILU 1
#define DY_ACT_LEAKY 2 /* LeakyReLU(0.1), ScalSeq */

int dy_abi_version(void);

/* ---- Conv.forward / forward_fuse, nn/modules/conv.py:41-59; nn.Conv2d heads nn/modules/head.py:38-42;
 *      LDConv.p_conv nn/modules/conv.py:356; input-gradient half of aten::convolution_backward. ------------------ */
int dy_conv_geometry(int cin, int cout, int ks, int stride, int* cin_p, int* cout_p, int* cc, int* nch, int* mt,
                     int* ngroups, int* ksteps, int* packed_elems);
/* fp32 OIHW master weights -> fp16 MFMA-packed; scale: optional per-Cout factor (BN folding, utils/torch_utils.py:171-198);
 * transposed=1 builds the (Cout->Cin, flipped taps) pack consumed by the stride-1 input-gradient pass. */
int dy_pack_weights(const float* w, const float* scale, void* out, int cout, int cin, int ks, int stride,
                    int transposed, hipStream_t stream);
/* every pack of a model in ONE launch: fill host descriptors (dy_pack_desc_bytes() each, first_block = running sum of the
 * returned block counts), copy them to the device once, then call dy_pack_weights_batched every step. */
int dy_pack_desc_bytes(void);
int dy_pack_desc_fill(void* desc, const float* w, const float* scale, void* out, int cout, int cin, int ks, int stride,
                      int transposed, int ld_taps, int ld_cphys, int first_block);
int dy_pack_weights_batched(const void* descs_device, int n, int total_blocks, hipStream_t stream);
/* y[n,ho,wo,:cout] = conv(x)[...]; x: (n,h,w,cin) with cin a multiple of 8 (zero-padded channels).
 * dil=2: x is read as a zero-dilated map of size (2h,2w) -- the input gradient of a stride-2 conv; out_h/out_w (>0)
 * then give the extent of the forward input (2h or 2h-1), otherwise pass 0 to derive the output extent.
 * partials: [num_partials][2][cout_p] floats, required with DY_EPI_STATS. */
/* size limit: the input is addressed with 32-bit byte offsets -- n*h*w*ldx*2 (1x1) or h*w*ldx*2 (3x3, per image) < 2 GiB, else DY_ERR_ARG */
int dy_conv_forward(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy, float* partials,
                    int n, int h, int w, int cin, int cout, int ks, int stride, int dil, int out_h, int out_w, int epi,
                    int* num_partials, hipStream_t stream);
int dy_conv_num_partials(int n, int h, int w, int cin, int cout, int ks, int stride, int dil);
/* Input gradient of a stride-1 conv (the dgrad half of aten::convolution_backward: dy (n,h,w,cin) x transposed pack -> dx (n,h,w,cout))
 * that is the ONLY writer of dx = the gradient w.r.t. the activated output of a Conv (nn/modules/conv.py:49-55): the first pass of that
 * Conv's BatchNorm backward (sums of g = dx * silu'(raw*scale+shift) and g*xhat over the pixels, dy_bn_act_bwd_reduce_acc) runs in
 * the epilogue on the values being stored and is added into acc [DY_BN_COPIES][2][C].  C == cout; dy_conv_red_supported(cin, cout, ks)
 * tells whether the geometry has this form (else DY_ERR_ARG). */
/* Conv.forward_fuse followed by Bottleneck's shortcut add (nn/modules/conv.py:57-59, nn/modules/block.py:333-335) in one launch:
 * y = fp16(fp16(SiLU(conv(x) + bias)) + res), the bits of dy_conv_forward(DY_EPI_BIAS | DY_EPI_SILU) followed by dy_add.  3x3 stride-1
 * convolutions the ping-pong kernel takes (dy_conv_res_supported); res: fp16 (N, Ho, Wo, ldres). */
int dy_conv_res_supported(int cin, int cout, int ks, int stride);
int dy_conv_forward_res(const void* x, int ldx, const void* w_packed, const float* bias, const void* res, int ldres, void* y, int ldy,
                        int n, int h, int w, int cin, int cout, int ks, int stride, hipStream_t stream);
int dy_conv_red_supported(int cin, int cout, int ks);
int dy_conv_input_grad_red(const void* dy, int lddy, const void* w_packed_t, void* dx, int lddx, int n, int h, int w, int cin, int cout,
                           int ks, const void* raw, int ldraw, const float* coef, double* acc, int C, hipStream_t stream);
/* host-side: the kernel instantiation dy_conv_forward launches for this geometry, spelled as rocprofv3 prints it */
int dy_conv_kernel_name(int cin, int cout, int ks, int stride, char* out, int cap);
/* ... for a launch with this output width, dilation and epilogue: maps exactly 40 pixels wide run 3x3 stride-1 convs of 32-channel
 * chunks on full-width tiles (conv_mfma_pp_kernel's last template argument), which rocprofv3 lists as a kernel of their own */
int dy_conv_kernel_name_at(int cin, int cout, int ks, int stride, int out_w, int dil, int epi, char* out, int cap);

/* ---- weight-gradient half of aten::convolution_backward for the same modules. dw: fp32 OIHW (cout,cin,ks,ks). -- */
int dy_wgrad_workspace(int n, int h, int w, int cin, int cout, int ks, int stride, int* nslabs, long* slab_elems);
/* host-side: the kernel instantiation dy_conv_wgrad launches for this geometry, spelled as rocprofv3 prints it.  The 3x3 block of
 * 64 x 64 channels exists with eight waves per workgroup (conv_wgrad_kernel<3, 1, 4, 4, BNF>, the default) and with four
 * (the instantiation BNF + 16): DY_WGRAD_WIDE=0 / 1, read at every call, picks; same slabs, same bits. */
int dy_wgrad_kernel_name(int cin, int cout, int ks, int stride, char* out, int cap);
/* the same for a given map: on small maps a workgroup owns a smaller (ci, co) channel block, so that fewer fp32 weight slabs exist */
int dy_wgrad_kernel_name_at(int n, int h, int w, int cin, int cout, int ks, int stride, char* out, int cap);
int dy_conv_wgrad(const void* x, int ldx, const void* dy, int lddy, float* slabs, float* dw, int n, int h, int w,
                  int cin, int cout, int ks, int stride, int accumulate, hipStream_t stream);
/* Weight gradient of a Conv (conv + BatchNorm + SiLU, nn/modules/conv.py:49-55) from the gradient w.r.t. its ACTIVATED output
 * (autograd: silu_backward + native_batch_norm_backward + the weight half of convolution_backward in one kernel): the
 * BatchNorm / SiLU backward apply pass runs on the dY operand while it is staged -- coef [4][cout] from the forward, acc
 * [DY_BN_COPIES][2][cout] from dy_bn_act_bwd_reduce_acc -- and d(raw conv output) is written to draw (N,Ho,Wo,ldraw; the geometry
 * of raw) for the input-gradient pass; dgamma / dbeta (may be NULL) receive the BatchNorm parameter gradients.  cout % 16 == 0. */
int dy_conv_wgrad_bn(const void* x, int ldx, const void* dy, int lddy, const void* raw, int ldraw, void* draw, const float* coef,
                     const double* acc, float* dgamma, float* dbeta, float count, float* slabs, float* dw, int n, int h, int w,
                     int cin, int cout, int ks, int stride, int accumulate, hipStream_t stream);
int dy_conv_wgrad_ld_bn(const void* x, int ldx, const void* dy, int lddy, const void* raw, int ldraw, void* draw,
                        const float* coef, const double* acc, float* dgamma, float* dbeta, float count, float* slabs, float* dw,
                        int n, int h, int w, int cout, int ld_cin, int ld_taps, int ld_cphys, int accumulate, hipStream_t stream);
/* 1x1 convolutions over a never-materialised concatenation (DySegs above): forward (dy_conv_forward with xs in place of (x, ldx); epi as
 * there), input gradient (every 8-channel piece of W^T dy stored in / added to its segment) and weight gradient with the BatchNorm backward
 * apply inside (dy_conv_wgrad_bn with xs in place of (x, ldx)).  dy_conv1x1_segs_supported: a Cin chunk exists that no segment boundary
 * cuts (the geometry's own, or 32 where that is 64: same packed weights) and the ping-pong kernel takes the shape. */
int dy_conv1x1_segs_supported(int cin, int cout, const DySegs* xs);
int dy_conv1x1_segs_kernel_name(int cin, int cout, const DySegs* xs, char* out, int cap); /* as dy_conv_kernel_name, for dy_conv1x1_forward_segs */
/* host-side: the kernel a 1x1 launch really runs, spelled as rocprofv3 prints it -- Conv.forward of a k = 1 Conv (nn/modules/conv.py:49-55)
 * or its input gradient through dy_conv_forward (xs = ys = NULL), dy_conv1x1_forward_segs (xs) or dy_conv1x1_input_grad_segs (ys: cin =
 * channels of dy, cout = channels of the concatenation, epi 0).  conv1x1_stream_kernel<k-steps, MT, PP> (csrc/conv1x1_stream.hip; PP = true for launches with BatchNorm sums) where the
 * selection rule takes it -- fp16 store, DY_EPI_ACCUM or DY_EPI_STATS | DY_EPI_STATS_ACC, Cin <= 128; environment DY_CONV1X1_STREAM:
 * 0 = never, force = every supported launch, unset = the measured rule -- else what dy_conv_kernel_name / dy_conv1x1_segs_kernel_name
 * return, which keep naming the ping-pong instantiation of the geometry.  Decided from the geometry alone: an output whose pixel stride
 * is not a multiple of 8 or whose base is not 16-byte aligned also stays on the ping-pong kernel, which this function cannot see. */
int dy_conv1x1_kernel_name_live(int cin, int cout, int n, int h, int w, int epi, const DySegs* xs, const DySegs* ys, char* out, int cap);
int dy_conv1x1_forward_segs(const DySegs* xs, const void* w_packed, const float* bias, void* y, int ldy, float* partials, int n, int h,
                            int w, int cin, int cout, int epi, hipStream_t stream);
int dy_conv1x1_input_grad_segs(const void* dy, int lddy, const void* w_packed_t, const DySegs* dxs, int n, int h, int w, int cin, int cout,
                               hipStream_t stream);
int dy_conv1x1_wgrad_bn_segs(const DySegs* xs, const void* dy, int lddy, const void* raw, int ldraw, void* draw, const float* coef,
                             const double* acc, float* dgamma, float* dbeta, float count, float* slabs, float* dw, int n, int h, int w,
                             int cin, int cout, int accumulate, hipStream_t stream);
/* C2f's ``cv1(x).chunk(2, 1)`` (nn/modules/block.py:223) with each half a tensor of its own ("two planes": channels [0, csplit) at one
 * base, [csplit, C) at another): the BatchNorm apply that writes them (dy_bn_act_apply_acc, no residual), the backward reduce that
 * reads their gradients (dy_bn_act_bwd_reduce_acc, no shortcut gradient) and the 1x1 weight gradient with the BatchNorm backward
 * inside whose dY operand they are (dy_conv_wgrad_bn; xs != NULL: dy_conv1x1_wgrad_bn_segs).  The weight gradient wants both planes
 * in one allocation, dy2 >= dy + n*h*w*lddy, same pixel stride. */
int dy_bn_act_apply_acc_split(const void* x, int ldx, void* y, int ldy, void* y2, int ldy2, int csplit, const double* acc,
                              const float* gamma, const float* beta, float* running_mean, float* running_var, float* coef, long npix,
                              int C, int act, float count, float eps, float momentum, hipStream_t stream);
int dy_bn_act_bwd_reduce_acc_split(const void* dy, int lddy, const void* dy2, int lddy2, int csplit, const void* x, int ldx,
                                   const float* coef, double* acc, long npix, int C, int act, hipStream_t stream);
int dy_conv1x1_wgrad_bn_planes(const DySegs* xs, const void* x, int ldx, const void* dy, const void* dy2, int lddy, int csplit,
                               const void* raw, int ldraw, void* draw, const float* coef, const double* acc, float* dgamma,
                               float* dbeta, float count, float* slabs, float* dw, int n, int h, int w, int cin, int cout,
                               int accumulate, hipStream_t stream);
/* Weight gradient AND input gradient of a 1x1 Conv + BatchNorm + SiLU in one launch: the fused counterparts of dy_conv_wgrad_bn (ks 1),
 * dy_conv1x1_wgrad_bn_segs and dy_conv1x1_wgrad_bn_planes.  d(raw) is formed while dY is staged, as there, but is never written out:
 * the workgroup multiplies its LDS tile by the rows of w_packed_t (dy_pack_weights, transposed = 1) that belong to its Cin chunk and
 * stores dX = W^T d(raw) itself -- into (dx, lddx), stored or (dx_accumulate) added to what it holds, or piece by piece into the
 * members of dxs (dy_conv1x1_input_grad_segs' table: c_end as in xs, acc 1 = add).  Every dX element is the MFMA chain of the
 * two-launch form (dy_conv_forward over w_packed_t / dy_conv1x1_input_grad_segs) and has its bits.  Exists where one workgroup's
 * block holds every output channel of the layer -- cout a multiple of 16 up to 64 that the map's weight-gradient geometry does not
 * split, cin a multiple of 8: dy_conv1x1_wgrad_dgrad_supported (host-side, no GPU needed); anything else is DY_ERR_ARG.
 * dy_wgrad_dgrad_kernel_name: the instantiation such a launch runs, as rocprofv3 prints it (segs != 0: the xs / dxs form). */
int dy_conv1x1_wgrad_dgrad_supported(int n, int h, int w, int cin, int cout);
int dy_wgrad_dgrad_kernel_name(int n, int h, int w, int cin, int cout, int segs, char* out, int cap);
int dy_conv1x1_wgrad_dgrad_bn(const void* x, int ldx, const void* dy, int lddy, const void* raw, int ldraw, const float* coef,
                              const double* acc, float* dgamma, float* dbeta, float count, float* slabs, float* dw,
                              const void* w_packed_t, void* dx, int lddx, int dx_accumulate, int n, int h, int w, int cin, int cout,
                              int accumulate, hipStream_t stream);
int dy_conv1x1_wgrad_dgrad_bn_segs(const DySegs* xs, const void* dy, int lddy, const void* raw, int ldraw, const float* coef,
                                   const double* acc, float* dgamma, float* dbeta, float count, float* slabs, float* dw,
                                   const void* w_packed_t, const DySegs* dxs, int n, int h, int w, int cin, int cout, int accumulate,
                                   hipStream_t stream);
int dy_conv1x1_wgrad_dgrad_bn_planes(const DySegs* xs, const void* x, int ldx, const void* dy, const void* dy2, int lddy, int csplit,
                                     const void* raw, int ldraw, const float* coef, const double* acc, float* dgamma, float* dbeta,
                                     float count, float* slabs, float* dw, const void* w_packed_t, void* dx, int lddx,
                                     int dx_accumulate, const DySegs* dxs, int n, int h, int w, int cin, int cout, int accumulate,
                                     hipStream_t stream);
/* The input gradient ALONE of a 1x1 Conv + BatchNorm + SiLU whose weight, gamma and beta are frozen: reference nn/modules/conv.py:41-59
 * under autograd with requires_grad=False parameters (engine/trainer.py:662-682, freeze=...), where BatchNorm stays in training mode, so
 * the batch-statistics backward is still live but no parameter gradient exists.  d(raw) is formed from (dy, raw, coef, acc) while dY is
 * staged and multiplied by w_packed_t into dX exactly as in dy_conv1x1_wgrad_dgrad_bn* -- same MFMA chains, same bits -- with NO X
 * operand: nothing of the layer input is read, no slab, dgamma or dbeta is written.  One entry for the three operand conventions:
 * dy2 != NULL = dY in two planes split at channel csplit (else csplit = 0); dxs != NULL = dX stored / added per member of a
 * concatenation (c_end up to cin, acc 1 = add; dx unused), else (dx, lddx) stored or (dx_accumulate) added to.  Supported exactly where
 * dy_conv1x1_wgrad_dgrad_supported is (dy_conv1x1_dgrad_bn_supported repeats it); dy_dgrad_only_kernel_name spells the instantiation
 * (BNF 13, segs != 0: 15) as rocprofv3 prints it. */
int dy_conv1x1_dgrad_bn_supported(int n, int h, int w, int cin, int cout);
int dy_dgrad_only_kernel_name(int n, int h, int w, int cin, int cout, int segs, char* out, int cap);
int dy_conv1x1_dgrad_bn(const void* dy, const void* dy2, int lddy, int csplit, const void* raw, int ldraw, const float* coef,
                        const double* acc, float count, const void* w_packed_t, void* dx, int lddx, int dx_accumulate,
                        const DySegs* dxs, int n, int h, int w, int cin, int cout, hipStream_t stream);
/* The stem Conv(3 -> 16, k 3, s 2, p 1) of the model YAMLs (nn/modules/conv.py:41-55 as model.0) read straight from the image
 * batch the trainer hands the model (models/yolo/detect/train.py:57-59: fp32 NCHW, img * mul): no import pass, no padded copy.
 * dy_stem_forward writes the raw conv output (N,Ho,Wo,ldraw) fp16 and ADDS the BatchNorm sums into acc [DY_BN_COPIES][2][16]
 * (then dy_bn_act_apply_acc as for any Conv).  dy_stem_wgrad_bn: weight gradient with the BatchNorm / SiLU backward apply inside
 * (as dy_conv_wgrad_bn; no d(raw) output -- the image needs no gradient): slabs [dy_stem_grid()][9][16][16] fp32 for
 * dy_wgrad_reduce_batched (descriptor: cin 3, cout 16, ks 3, stride 2).
 * The three launches run software-pipelined kernels with 16-byte image loads where w % 4 == 0 and the image base is 16-byte aligned
 * (dy_stem_pipelined: 1), the plain kernels otherwise or under DY_STEM_V1=1 (read at every call); the results are the same bits. */
int dy_stem_grid(int n, int h, int w);
int dy_stem_pipelined(const float* img_nchw, int w);
int dy_stem_forward(const float* img_nchw, const float* weight, void* raw, int ldraw, double* acc, int n, int h, int w, float mul,
                    hipStream_t stream);
/* The same stem in eval mode (Conv.forward_fuse, nn/modules/conv.py:57-59; get_FPS.py:49 fuses the model before timing it):
 * y = act(conv(img * mul) + bias) as fp16 NHWC, no statistics.  bias NULL: none (un-fused eval: BatchNorm with running statistics follows
 * as its own pass); silu 0: no activation. */
int dy_stem_forward_eval(const float* img_nchw, const float* weight, const float* bias, void* y, int ldy, int n, int h, int w, float mul,
                         int silu, hipStream_t stream);
int dy_stem_wgrad_bn(const float* img_nchw, const void* dy, int lddy, const void* raw, int ldraw, const float* coef,
                     const double* acc, float* dgamma, float* dbeta, float count, float* slabs, int n, int h, int w, float mul,
                     hipStream_t stream);
/* Weight gradient of a conv with bias (Detect's final nn.Conv2d nn/modules/head.py:38-42, LDConv.p_conv nn/modules/conv.py:356) that also
 * takes the bias gradient -- the sum of dY over the pixels -- from the dY granules it stages: added into bias_acc
 * [DY_BN_COPIES][round8(cout)] (fp64, zeroed by the caller), finished by dy_wgrad_reduce_batched for descriptors marked with
 * dy_wgrad_reduce_desc_bias(desc, bias_acc, dbias, round8(cout)).  Not for 48- / 96-channel outputs (DY_ERR_ARG). */
int dy_conv_wgrad_bias(const void* x, int ldx, const void* dy, int lddy, double* bias_acc, float* slabs, float* dw, int n, int h, int w,
                       int cin, int cout, int ks, int stride, int accumulate, hipStream_t stream);
int dy_wgrad_reduce_desc_bias(void* desc, const double* bias_acc, float* dbias, int c);
/* dw == NULL in dy_conv_wgrad / dy_conv_wgrad_ld defers the slab reduction: the caller keeps that layer's slabs alive, fills one
 * descriptor per layer (host side, sizeof = dy_wgrad_reduce_desc_bytes(); returns the layer's block count, first_block = the
 * exclusive prefix sum of those counts) and reduces every layer of the backward pass in ONE launch. */
int dy_wgrad_reduce_desc_bytes(void);
int dy_wgrad_reduce_desc_fill(void* desc, const float* slabs, int nslabs, float* dw, int cin, int cout, int ks, int stride,
                              int accumulate, int ld_taps, int ld_cphys, int ld_cin, int first_block);
int dy_wgrad_reduce_batched(const void* descs_device, int n, int total_blocks, hipStream_t stream);

/* ---- LDConv, nn/modules/conv.py:350-503: sampling (offset -> 4-corner bilinear gather, :366-410, :456-489) writes
 *      x_off[pix][n*C + c]; the (N,1) column conv (:354) then is a 1x1 conv with K = N*C whose weights are packed /
 *      whose weight gradient is unpacked by the *_ld variants (master layout (cout, cin, N, 1)). ------------------- */
int dy_ldconv_sample(const void* x, int ldx, const float* off, int ldoff, const int* pn, void* xo, int ldxo, int n, int H,
                     int W, int h, int w, int C, int Np, int stride, hipStream_t stream);
/* dx32: (n,H,W,C) fp32 scatter accumulator, zeroed by the caller (NULL: skip); doff: fp16 (n,h,w,lddoff), ch [0,2Np) */
int dy_ldconv_sample_backward(const void* x, int ldx, const float* off, int ldoff, const int* pn, const void* dxo,
                              int lddxo, float* dx32, void* doff, int lddoff, int n, int H, int W, int h, int w, int C,
                              int Np, int stride, hipStream_t stream);
/* The same backward with the input gradient computed by a deterministic gather and written (accumulate=0) or added
 * (accumulate=1) straight into the fp16 gradient map dx (n,H,W,lddx).  Samples whose offsets stay within rmax pixels
 * (1..16) are gathered, with the candidate radius shrunk to the largest |offset| of the layer, measured on the device into
 * scratch (>= 4 bytes); the far ones go through fp32 atomics into dx32 (n*H*W*C floats, caller-owned, need not be
 * zeroed, untouched when the layer has no far sample) and are folded in by the gather -- no host decision anywhere. */
int dy_ldconv_sample_backward_gather(const void* x, int ldx, const float* off, int ldoff, const int* pn, const void* dxo,
                                     int lddxo, void* dx, int lddx, int accumulate, float* dx32, void* doff, int lddoff,
                                     void* scratch, int rmax, int n, int H, int W, int h, int w, int C, int Np, int stride,
                                     hipStream_t stream);
int dy_f32_to_f16_add(const float* src, void* dst, int ld, long npix, int C, int accumulate, hipStream_t stream);
int dy_pack_weights_ld(const float* w, void* out, int cout, int cin, int ld_taps, int ld_cphys, int transposed,
                       hipStream_t stream);
int dy_conv_wgrad_ld(const void* x, int ldx, const void* dy, int lddy, float* slabs, float* dw, int n, int h, int w,
                     int cout, int ld_cin, int ld_taps, int ld_cphys, int accumulate, hipStream_t stream);

/* ---- nn.BatchNorm2d / BatchNorm3d (training statistics) + SiLU / LeakyReLU, nn/modules/conv.py:49-55,
 *      nn/extra_modules/block.py:3440-3441, utils/torch_utils.py:347-349, and their autograd backward. ------------- */
/* coef: [4][C] = scale, shift, mean, invstd.  Up to three weighted partial sets (ScalSeq: three resolutions). */
int dy_bn_finalize(const float* p0, int n0, float w0, const float* p1, int n1, float w1, const float* p2, int n2,
                   float w2, const float* gamma, const float* beta, float* running_mean, float* running_var,
                   float* coef, int C, float count, float eps, float momentum, int update_running, hipStream_t stream);
int dy_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                    float* coef, int C, float eps, hipStream_t stream);
/* y = act(x*scale+shift) (+ res) */
int dy_bn_act_apply(const void* x, int ldx, const void* res, int ldr, void* y, int ldy, const float* coef, long npix,
                    int C, int act, hipStream_t stream);
/* The same three passes WITHOUT the finalize launches (nn/modules/conv.py:49-55 and its autograd backward, as above): the
 * statistics travel in fp64 accumulators acc[DY_BN_COPIES][2][C] that the producer adds into (dy_conv_forward with
 * DY_EPI_STATS | DY_EPI_STATS_ACC; dy_bn_act_bwd_reduce_acc) and the consumer sums in its prologue; block 0 of the consumer leaves
 * coef [4][C] + the running statistics (forward) / dgamma, dbeta (backward) behind.  The caller zeroes acc before the producer. */
int dy_bn_act_apply_acc(const void* x, int ldx, const void* res, int ldr, void* y, int ldy, const double* acc,
                        const float* gamma, const float* beta, float* running_mean, float* running_var, float* coef,
                        long npix, int C, int act, float count, float eps, float momentum, hipStream_t stream);
/* res_grad (may be NULL): gradient of a residual operand added after the activation (Bottleneck shortcut, nn/modules/block.py:333-335)
 * -- it equals dy, and is stored (res_accumulate 0) or added (1) while dy streams through, instead of by a pass of its own */
int dy_bn_act_bwd_reduce_acc(const void* dy, int lddy, const void* x, int ldx, const float* coef, double* acc, long npix,
                             int C, int act, void* res_grad, int ldrg, int res_accumulate, hipStream_t stream);
/* The accumulator forms of the forward apply / backward reduce (SiLU, no residual / shortcut operand) for SEVERAL tensors in one launch
 * (n <= dy_bn_group_max(); array arguments have n entries): independent Convs of one stage, whose passes would otherwise queue behind
 * each other although the small ones cannot fill the chip. */
int dy_bn_group_max(void);
int dy_bn_act_apply_acc_group(int n, const void* const* x, const int* ldx, void* const* y, const int* ldy, const double* const* acc,
                              const float* const* gamma, const float* const* beta, float* const* running_mean, float* const* running_var,
                              float* const* coef, const long* npix, const int* C, const float* count, const float* eps,
                              const float* momentum, hipStream_t stream);
int dy_bn_act_bwd_reduce_acc_group(int n, const void* const* dy, const int* lddy, const void* const* x, const int* ldx,
                                   const float* const* coef, double* const* acc, const long* npix, const int* C, hipStream_t stream);
/* dy_bn_act_bwd_reduce_acc for a gradient that has ROWS (what dy_conv1x1_rows_backward passes down: zero at every background anchor):
 * the sums visit the foreground pixels of `assigned` (B = n images, A anchors each, this tensor's pixel (b, r) is anchor a0 + r) only */
int dy_bn_act_bwd_reduce_rows(const void* dy, int lddy, const void* x, int ldx, const float* coef, double* acc, int n, int hw, int C,
                              int act, const int* assigned, int A, int a0, hipStream_t stream);
int dy_bn_act_bwd_apply_acc(const void* dy, int lddy, const void* x, int ldx, void* dx, int lddx, const float* coef,
                            const double* acc, float* dgamma, float* dbeta, long npix, int C, int act, float count,
                            hipStream_t stream);
int dy_bn_act_bwd_reduce(const void* dy, int lddy, const void* x, int ldx, const float* coef, float* partials,
                         int max_partials, long npix, int C, int act, int* nparts, hipStream_t stream);
/* bwdcoef: [2][C] = mean(g), mean(g*xhat); dgamma/dbeta fp32 (may be NULL) */
int dy_bn_bwd_finalize(const float* partials, int nparts, float* dgamma, float* dbeta, float* bwdcoef, int C,
                       float count, int accumulate, hipStream_t stream);
int dy_bn_act_bwd_apply(const void* dy, int lddy, const void* x, int ldx, void* dx, int lddx, const float* coef,
                        const float* bwdcoef, long npix, int C, int act, int frozen_stats, hipStream_t stream);

/* ---- the same passes for ANY channel count C >= 1 (Detect's class branch is max(ch[0], min(nc, 100)) wide, nn/modules/head.py:36).
 * Tensors keep a pixel stride that is a multiple of 8 and >= round8(C); lanes c in [C, round8(C)) of the last 8-channel granule are
 * PAD lanes.  A pad lane that is READ (the raw conv output: dy_conv_forward masks its fp16 stores at channel granularity, so those
 * lanes may hold anything) never reaches a result; a pad lane that is WRITTEN (y, dx) gets +0.0, so the convolution that reads the
 * tensor next multiplies exact zeros; per-channel vectors (gamma, beta, running statistics, coef [4][C], bwdcoef [2][C], dgamma,
 * dbeta) are C long and never indexed at c >= C.  Same pixel-to-lane mapping and arithmetic as the entry points above at width
 * round8(C): the real channels carry the same bits, and for C % 8 == 0 so does everything. */
/* dy_bn_finalize for one partial set whose rows are ldp >= C floats apart ([nparts][2][ldp]: dy_conv_forward's DY_EPI_STATS rows are
 * round16(cout) wide); with update_running, *num_batches_tracked (int64, may be NULL) is incremented once, as nn.BatchNorm's training
 * forward does (the entry points above leave that counter to their caller) */
int dy_bn_finalize_ld(const float* part, int nparts, int ldp, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float* coef, int C, float count, float eps, float momentum, int update_running,
                      long long* num_batches_tracked, hipStream_t stream);
int dy_bn_act_apply_c(const void* x, int ldx, const void* res, int ldr, void* y, int ldy, const float* coef, long npix, int C,
                      int act, hipStream_t stream);
/* partials: [*nparts][2][round8(C)], columns c >= C never written */
int dy_bn_act_bwd_reduce_c(const void* dy, int lddy, const void* x, int ldx, const float* coef, float* partials, int max_partials,
                           long npix, int C, int act, int* nparts, hipStream_t stream);
int dy_bn_bwd_finalize_ld(const float* partials, int nparts, int ldp, float* dgamma, float* dbeta, float* bwdcoef, int C,
                          float count, int accumulate, hipStream_t stream);
int dy_bn_act_bwd_apply_c(const void* dy, int lddy, const void* x, int ldx, void* dx, int lddx, const float* coef,
                          const float* bwdcoef, long npix, int C, int act, int frozen_stats, hipStream_t stream);
/* dst[0, n) = src, dst[n, n_pad) = 0: the bias of a fused Conv whose width is not a multiple of 8, so that its convolution can run over
 * round8(cout) rows (zero weight rows) and store SiLU(0) = +0.0 in the pad lanes */
int dy_pad_f32(const float* src, int n, float* dst, int n_pad, hipStream_t stream);

/* ---- data movement: image import (models/yolo/detect/train.py:57-59), nn.Upsample(2,'nearest') (model YAMLs),
 *      SPPF's MaxPool2d(5,1,2) chain nn/modules/block.py:166-171, Add nn/extra_modules/block.py:3483-3484,
 *      Concat nn/modules/conv.py:338-348, ScalSeq tail nn/extra_modules/block.py:3437-3443. -------------------------- */
int dy_import_image(const float* x_nchw, void* y, int n, int c, int h, int w, int cp, float mul, hipStream_t stream);
/* The loader's batch: uint8 NHWC RGB (n,h,w,3), 4-byte aligned -> fp16 NHWC with channels zero-padded to cp, value u8/255
 * (models/yolo/detect/train.py:59 `batch["img"].float() / 255`).  flip: NULL, or n bytes -- bit 0 mirrors image i left-right,
 * bit 1 up-down while converting (RandomFlip, data/augment.py:651-683; the loader then ships unflipped pixels).  index: NULL,
 * or n ints -- batch slot i reads image index[i] of x, a pool of decoded images resident in HBM (no per-step host copy).
 * hsv: NULL, or n x 3 floats -- RandomHSV's hue / saturation / value gains of image i (data/augment.py:605-624). */
int dy_import_image_u8(const void* x, void* y, int n, int h, int w, int cp, const void* flip, const int* index,
                       const float* hsv, hipStream_t stream);
/* Mosaic (data/augment.py:208-241) + random affine / perspective (cv2.warpAffine | warpPerspective of RandomPerspective :384-435,
 * border 114) + MixUp (:326-345) + flips, composed from an HBM-resident pool of letterboxed s x s uint8 images straight into the
 * fp16 NHWC stem input.  slots: n x 2 records (dy_warp_slot_bytes() bytes per sample: the sample, then its MixUp partner) of
 * 48 words = { float minv[6] (output pixel -> canvas, rows 0-1 of the inverse map); int canvas_w, canvas_h, xc, yc, flip, npatch;
 * int patch[4][7] = pool index, destination x1,y1,x2,y2 on the canvas, source x,y; float hsv[3] (RandomHSV gains, 0 = off);
 * float pinv[3] (row 2 of the inverse map; 0,0,1 when affine); double mix_r (MixUp ratio of this image; < 0: no partner) },
 * built on the host from the random draws. */
int dy_warp_import_u8(const void* pool, const void* slots, void* y, int n, int s, int cp, hipStream_t stream);
int dy_warp_slot_bytes(void);
int dy_add(const void* a, int lda, const void* b, int ldb, const void* c, int ldc, void* y, int ldy, long npix, int C,
           hipStream_t stream);
int dy_upsample2x(const void* x, int ldx, void* y, int ldy, int n, int h, int w, int C, int backward, int accumulate,
                  hipStream_t stream);
/* SPDConv's space-to-depth, nn/extra_modules/block.py:2504-2507 (``torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2],
 * x[..., 1::2, 1::2]], 1)`` in front of its 3x3 Conv): y[n, i, j, (a + 2b) C + k] = x[n, 2i + a, 2j + b, k] with a the row and b the
 * column parity.  x: (n, h, w, C) at pixel stride ldx; y: (n, h/2, w/2, 4C) at pixel stride ldy; either may be a channel slice of a
 * wider tensor, and no other channel is touched.  backward = 0: y <- x.  backward = 1: y holds dY and x receives dX (accumulate = 1:
 * is added to, one fp16 addition per element).  DY_ERR_ARG for a null pointer or an odd / < 2 map side, DY_ERR_ALIGN when C, ldx or
 * ldy is no multiple of 8 or a pointer is not 16-byte aligned; nothing is launched then. */
int dy_space_to_depth(void* x, int ldx, void* y, int ldy, int n, int h, int w, int C, int backward, int accumulate,
                      hipStream_t stream);
/* DySample's sampling stage, nn/extra_modules/block.py:3856-3879 (style 'lp', no dyscope: ``offset(x) * 0.25 + init_pos``, the grid of
 * ``sample`` :3860-3870 and ``F.grid_sample(bilinear, align_corners=False, padding_mode='border')`` per channel group :3871-3872).
 * x: fp16 (n, H, W, C) at pixel stride ldx; off: the RAW fp32 output of the 1x1 offset convolution, (n, H, W, 2 G s^2) at ldoff,
 * channel d G s^2 + g s^2 + i s + j = coordinate d (0 = x, 1 = y) of group g at sub-position (row i, column j); y: fp16
 * (n, sH, sW, C) at ldy.  Output pixel (s h + i, s w + j) of group g (channels [g C/G, (g+1) C/G)) is the bilinear sample of x at
 * (clamp(w + 0.25 o_x + t[j], 0, W-1), clamp(h + 0.25 o_y + t[i], 0, H-1)), t[k] = (k - (s-1)/2) / s -- init_pos in closed form, no
 * buffer is read.  x and y may be channel slices of wider tensors; no other channel is touched.
 * dy_dysample_supported: s in {2, 4}, G >= 1, C a multiple of 8 G (host-side, no GPU needed).  DY_ERR_ARG for anything else, a
 * null pointer or a pitch below its channel count; DY_ERR_ALIGN when ldx / ldy is no multiple of 8 or x / y is not 16-byte
 * aligned; nothing is launched then. */
int dy_dysample_supported(int C, int G, int s);
int dy_dysample(const void* x, int ldx, const float* off, int ldoff, void* y, int ldy, int n, int H, int W, int C, int G, int s,
                hipStream_t stream);
/* Backward of dy_dysample (autograd through :3878 and grid_sample's backward).  dy: fp16 gradient of y at lddy.
 * doff (fp16, (n, H, W, lddoff), channels [0, 2 G s^2), lddoff a multiple of 8): the gradient w.r.t. the RAW convolution output --
 * 0.25 * sum over the group's channels of dy * d(value)/d(coordinate), zero where the unclamped position is at or beyond 0 / size-1
 * (grid_sample's border rule) -- written, not accumulated.  NULL: skipped.
 * dx (fp16, (n, H, W, C) at lddx): the sampler's input gradient, written (accumulate = 0) or added (1), by the contract of
 * dy_ldconv_sample_backward_gather: a deterministic gather over the base pixels within R <= rmax (1..16) of an input pixel, R from
 * the largest |0.25 o| of the layer measured on the device into scratch (>= 4 bytes); samples with |0.25 o| > rmax - 1 go through
 * fp32 atomics into dx32 (n*H*W*C floats, caller-owned, need not be zeroed, untouched when the layer has none) and are folded in
 * by the gather -- no host decision anywhere; without far samples two calls on the same inputs give the same bits.  NULL: skipped
 * (dx32 / scratch are not needed then).  The offset convolution's own input gradient is the caller's. */
int dy_dysample_backward(const void* x, int ldx, const float* off, int ldoff, const void* dy, int lddy, void* dx, int lddx,
                         int accumulate, float* dx32, void* doff, int lddoff, void* scratch, int rmax, int n, int H, int W, int C,
                         int G, int s, hipStream_t stream);
/* CARAFE's reassembly stage, nn/extra_modules/block.py:3926-3935 (pixel_shuffle, softmax over the 25 kernel taps, nearest
 * up-sampling, Unfold(5, dilation 2, padding 4) and the einsum), for k_up = 5 and scale = 2.
 * x: fp16 (n, H, W, C) at pixel stride ldx; logits: the encoder's fp16 output (:3924-3925), 100 logical channels at ldl >= 104;
 * y: fp16 (n, 2H, 2W, C) at ldy.  Y[c, 2h+i, 2w+j] = sum_{a,b} p[5a+b] x[c, h+a-2, w+b-2] with p = softmax over k = 0..24 of
 * logits[4k + 2i + j, h, w] (maximum subtracted) and x = 0 outside the map.  x and y may be channel slices of wider tensors; no
 * other channel is touched.  dy_carafe_supported: k_up == 5, scale == 2, C >= 8 a multiple of 8 (host-side, no GPU needed).
 * DY_ERR_ARG for anything else, a null pointer, n / H / W < 1, a pitch below its width or a map whose 4 n H W reaches 2^31;
 * DY_ERR_ALIGN when a pitch is no multiple of 8 or a pointer is not 16-byte aligned; nothing is launched then. */
int dy_carafe_supported(int C, int k_up, int scale);
int dy_carafe(const void* x, int ldx, const void* logits, int ldl, void* y, int ldy, int n, int H, int W, int C, hipStream_t stream);
/* Backward of dy_carafe (autograd through :3926-3935).  dy: fp16 gradient of y at lddy.  The softmax weights are recomputed from
 * the logits, not kept.  dlogits (fp16 (n, H, W, 104) at lddl >= 104, required): p_k (g_k - sum_m p_m g_m) with
 * g_k = sum_c dy[c, 2h+i, 2w+j] x[c, h+a-2, w+b-2] in the channel order of logits; lanes 100..103 are written as zeros.
 * dx (fp16 (n, H, W, C) at lddx): written (accumulate = 0) or added to (1); a gather over the <= 25 base pixels x 4 sub-pixels that
 * read an input pixel.  NULL: that half is skipped.  Fixed summation order, no atomics: two calls give the same bits.  Refusals as
 * dy_carafe. */
int dy_carafe_backward(const void* x, int ldx, const void* logits, int ldl, const void* dy, int lddy, void* dx, int lddx,
                       int accumulate, void* dlogits, int lddl, int n, int H, int W, int C, hipStream_t stream);
/* ---- Depthwise convolution with channel multiplier m = c2 / c1 (reference nn/modules/conv.py:106-111 DWConv: Conv with
 * g = math.gcd(c1, c2); :113-122 DSConv: DWConv(c1, c1, 3) then Conv(c1, c2, 1); nn.Conv2d(groups = c1), no bias, 'same' padding k / 2;
 * BatchNorm folded by nn/tasks.py:178).  x: fp16 (n, H, W, C1) at ldx; the output (n, Ho, Wo, C1 m) with Ho = (H + 2 (k / 2) - k) / s + 1;
 * w: the fp32 MASTER weights (C1 m, 1, k, k) -- there is no pack; output channel o reads input channel o / m.
 * dy_dwconv_supported (host-side, no GPU needed): C1 >= 8 a multiple of 8, m in {1, 2}, k in {3, 5}, s in {1, 2}.  Every entry below:
 * DY_ERR_ARG for anything else, a null pointer, n / H / W < 1, a pitch below its width; DY_ERR_ALIGN when a pitch is no multiple of 8
 * or a pointer is not 16-byte aligned; nothing is launched then.  x, y and the gradients may be channel slices (pitch > width).  No
 * allocation, no synchronisation, fixed summation orders and no atomics: two calls give the same bits (csrc/dwconv.hip lists the orders). */
int dy_dwconv_supported(int C1, int m, int k, int s);
/* rows of statistics partials dy_dwconv_forward writes / slabs dy_dwconv_wgrad needs for this geometry (host-side) */
int dy_dwconv_num_partials(int n, int H, int W, int C1, int m, int k, int s);
int dy_dwconv_wgrad_slabs(int n, int H, int W, int C1, int m, int k, int s);
/* epi: 0 = raw fp16 output; DY_EPI_STATS = raw output + per-channel sum / sum of squares of the STORED values as rows
 * partials[dy_dwconv_num_partials][2][C1 m] (what dy_bn_finalize / dy_bn_finalize_ld with ldp = C1 m take); DY_EPI_BIAS
 * (| DY_EPI_SILU) = act(fp16(conv) + bias[c]) in one launch (Conv.forward_fuse, nn/modules/conv.py:57-59). */
int dy_dwconv_forward(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, float* partials, int n, int H,
                      int W, int C1, int m, int k, int s, int epi, hipStream_t stream);
/* dX of the convolution (autograd of nn/modules/conv.py:52), a gather: every input pixel sums the taps that reach it (stride 2: those
 * of its parity class) and, for m = 2, both output channels of its group, in fp32.  draw: d(raw output) fp16 at lddy; dx (n, H, W, C1)
 * at lddx stored (accumulate = 0) or added to (1); NULL: no launch, DY_OK. */
int dy_dwconv_input_grad(const void* draw, int lddy, const float* w, void* dx, int lddx, int accumulate, int n, int H, int W, int C1,
                         int m, int k, int s, hipStream_t stream);
/* dW[o][ky][kx] = sum over (n, y, x) of draw[n, y, x, o] x[n, y s + ky - k / 2, x s + kx - k / 2, o / m] in two launches: per-workgroup
 * fp32 slabs[dy_dwconv_wgrad_slabs][C1 m k k], then their ordered reduction into dw (fp32 (C1 m, 1, k, k): stored, or added to). */
int dy_dwconv_wgrad(const void* x, int ldx, const void* draw, int lddy, float* slabs, float* dw, int accumulate, int n, int H, int W,
                    int C1, int m, int k, int s, hipStream_t stream);
/* ---- The pooled front of ADown, the YOLOv9 down-sampler (reference nn/extra_modules/block.py:4685-4698: :4693
 * ``avg_pool2d(x, 2, 1, 0, False, True)``, :4694 ``x.chunk(2, 1)``, :4696 ``max_pool2d(x2, 3, 2, 1)``; the two Convs behind it run as
 * any Conv).  x: fp16 (n, H, W, C) at ldx, C a multiple of 16, H, W >= 2; Ho = H / 2, Wo = W / 2, c = C / 2.  ONE launch writes
 * a (n, 2Ho, 2Wo, c) at lda: the averages of the first c channels -- fp32 ((x00 + x01) + x10) + x11, times 0.25, one fp16 rounding --
 * with the row / column past the (H-1) x (W-1) averaged map (an even side has exactly one) written as ZERO on every launch, so that the
 * 3x3 s2 p1 convolution behind it reads a stored zero where the reference reads padding; p (n, Ho, Wo, c) at ldp: the 3x3 s2 p1 max
 * over the fp16 averages of the last c channels, out-of-range taps skipped; argmax (NULL in inference): the winning tap 3 ky + kx, one
 * uint8 per element of p (dense, pitch c), the FIRST maximum in row-major (ky, kx) order as ATen has it.
 * DY_ERR_ARG: a null pointer (argmax excepted in the forward), n < 1, H < 2, W < 2, a pitch below its width; DY_ERR_ALIGN: C % 16, a
 * pitch that is no multiple of 8, a pointer off a 16-byte boundary; nothing is launched then.  Every operand may be a channel slice
 * of a wider tensor: no other channel is touched.  No allocation, no synchronisation, no atomics. */
int dy_adown_pool(const void* x, int ldx, void* a, int lda, void* p, int ldp, void* argmax, int n, int H, int W, int C,
                  hipStream_t stream);
/* Autograd of the three lines above, a gather over the pixels of x.  First half: dx = 0.25 x the sum of the <= 4 entries of da whose
 * average read the pixel (the border of da is never read).  Second half: 0.25 x the sum, over those averages, of the dp of the <= 4
 * windows whose argmax names that average.  fp32 sums in a fixed order (csrc/adown.hip), one fp16 rounding; accumulate = 1 adds to dx
 * (one fp32 addition of the stored value, then the one rounding).  Two calls give the same bits. */
int dy_adown_pool_backward(const void* da, int ldda, const void* dp, int lddp, const void* argmax, void* dx, int lddx, int accumulate,
                           int n, int H, int W, int C, hipStream_t stream);
/* ---- Fusion in 'bifpn' mode, BiFPN's fast normalised fusion (reference nn/extra_modules/block.py:453-490: :486
 * ``fusion_weight = self.relu(self.fusion_weight.clone())``, :487 ``fusion_weight / torch.sum(fusion_weight, dim=0)``, :488 the
 * weighted sum of the stacked operands; built by nn/tasks.py:922-925).  nops = 2 or 3 operands x_i: fp16 (n, H, W, C) at ld_i, C a
 * multiple of 8; half_i != 0: the operand is STORED at half resolution, (n, H/2, W/2, C) (an nn.Upsample(None, 2, 'nearest') that
 * was not executed; H and W even), and pixel (h, w) reads (h/2, w/2).  p: the fp32 parameter (nops values) in DEVICE memory, read by
 * the launch: w = max(p, 0), s = (w0 + w1) + w2, f = w / s; NO epsilon (the reference sets self.epsilon = 1e-4 at :463 and never
 * uses it): all weights <= 0 give NaN, as the reference's 0 / 0.  y = fp16((f0 x0 + f1 x1) + f2 x2), fp32 arithmetic, one rounding.
 * Unused operand slots (x2 with nops = 2) are ignored.  DY_ERR_ARG: a null pointer, nops outside 2..3, n, H, W < 1, a pitch below C,
 * an odd H or W with a half-resolution operand; DY_ERR_ALIGN: C % 8, a pitch % 8, a pointer off a 16-byte boundary (p, ws, gw: 4);
 * nothing is launched then.  No allocation, no synchronisation, no atomics in any of the entries. */
int dy_fusion_forward(const void* x0, int ld0, int half0, const void* x1, int ld1, int half1, const void* x2, int ld2, int half2,
                      const float* p, void* y, int ldy, int nops, int n, int H, int W, int C, hipStream_t stream);
/* Autograd of :486-488 in one pass over dy and the operands.  dx_i (null: the operand needs no gradient) = fp16(f_i dy), at FULL
 * resolution at lddx_i also for a half-resolution operand (nn.Upsample's backward folds it); acc_i = 1: fp16(stored + f_i dy), one
 * fp32 addition.  ws: fp32 [nops][dy_fusion_num_partials(n H W, C)], caller-provided: workgroup b stores its part of
 * g_i = <dy, x_i> at ws[i * parts + b] (running fp32 sums per work item, xor-shuffle tree, the four waves in order: csrc/fusion.hip).
 * ws = NULL: the frozen variant -- no operand is read (the x_i may be null), no dot product, the same dx bits. */
int dy_fusion_backward(const void* dy, int lddy, const void* x0, int ld0, int half0, void* dx0, int lddx0, int acc0, const void* x1,
                       int ld1, int half1, void* dx1, int lddx1, int acc1, const void* x2, int ld2, int half2, void* dx2, int lddx2,
                       int acc2, const float* p, float* ws, int nops, int n, int H, int W, int C, hipStream_t stream);
/* One workgroup: g_i = the nparts partials of ws summed in a fixed order in fp64 (as the BatchNorm statistics are), rounded to fp32;
 * then in fp32 t = (f0 g0 + f1 g1) + f2 g2 and dL/dp_j = p_j > 0 ? (g_j - t) / s : 0, stored to gw[j] (accumulate = 0) or added to it
 * (accumulate = 1, the convention of dy_bn_bwd_finalize's bias gradients).  gw: fusion_weight's slice of the flat gradient buffer. */
int dy_fusion_wgrad_finish(const float* ws, int nparts, const float* p, float* gw, int nops, int accumulate, hipStream_t stream);
/* Workgroups (= partials per dot product) of dy_fusion_backward for a map of npix pixels x C channels; < 0: DY_ERR_ARG. */
int dy_fusion_num_partials(long npix, int C);
/* ---- SimAM, parameter-free attention (reference nn/extra_modules/attention.py:53-77: :72 ``n = w * h - 1``, :74 the squared
 * deviation from the plane mean, :75 ``/ (4 * (sum / n + e_lambda)) + 0.5``, :77 ``x * sigmoid(y)``; built by nn/tasks.py:969-970).
 * Per image and channel over the M = H W values of the plane: mu = mean(x), d = x - mu, S = sum(d^2), D = 4 (S / (M - 1) + e_lambda),
 * y = x sigmoid(d^2 / D + 0.5).  x, y: fp16 (n, H, W, C) at ldx / ldy, C a multiple of 8 (an operand may be a channel slice of a
 * wider tensor; nothing outside its C channels is read or written).  Two launches: plane sums of x and x^2 through fp64
 * accumulators (exact for fp16 inputs, so a mean far above the spread needs no second pass), one fp64 partial per
 * (image, pixel run, sum, channel) in ws; then every workgroup folds its image's partials in a fixed order and applies.  stats: fp32
 * [n][2][C], written here -- mu and 1 / D per (image, channel) -- and read by dy_simam_backward.  ws: fp64
 * [n][dy_simam_num_partials(H W, C)][2][C], caller-provided scratch.  All other arithmetic is fp32 (csrc/simam.hip states it), one
 * fp16 rounding of y.  A plane of ONE pixel gives 0 / 0: its y is NaN, as the reference's; nothing guards it.  DY_ERR_ARG: a null
 * pointer, n, H, W < 1, C < 8 or not a multiple of 8, a pitch below C; DY_ERR_ALIGN: a pitch % 8, a pointer off a 16-byte boundary
 * (ws: 8); nothing is launched then.  No allocation, no synchronisation, no atomics: two calls give the same bits. */
int dy_simam_forward(const void* x, int ldx, void* y, int ldy, float* stats, double* ws, float e_lambda, int n, int H, int W, int C,
                     hipStream_t stream);
/* Autograd of :72-77 through the plane's mean and variance.  With g = dy, a recomputed from x and stats (never stored),
 * q = g x a (1 - a), T = sum(q d^2), U = sum(q d) over the plane:  dx = g a + (2 d / D) (q - 4 T / ((M - 1) D)) - 2 U / (M D).
 * Two launches as the forward: T and U through fp64 accumulators into ws (same size as the forward's), then the fold and dx,
 * stored (accumulate = 0) or added to what is there (accumulate = 1: one fp32 addition of the stored value, then the one
 * rounding).  Reads dy and x twice: 4 reads + 1 write (+ 1 read when accumulating) of the map. */
int dy_simam_backward(const void* dy, int lddy, const void* x, int ldx, const float* stats, void* dx, int lddx, int accumulate,
                      double* ws, int n, int H, int W, int C, hipStream_t stream);
/* Pixel runs (= fp64 partials per plane sum) per image of the two entries above for planes of M = H W pixels x C channels;
 * < 0: DY_ERR_ARG. */
int dy_simam_num_partials(long M, int C);
/* ---- GSConv's channel shuffle (reference nn/extra_modules/block.py:896-908: ``x2 = cat(x1, cv2(x1))``, then the reshape / permute /
 * reshape / cat chain, which is exactly ``cat(x2[:, 0::2], x2[:, 1::2])``: every even channel of x2, then every odd one).  x1, d: fp16
 * (n, H, W, c_) at ld1 / ldd, the two halves of x2, which is never built; y: fp16 (n, H, W, 2 c_) at ldy; y[j] = x2[2 j],
 * y[c_ + j] = x2[2 j + 1].  c_ a multiple of 8.  One work item per (pixel, 8 output channels): the two 16-byte granules of x2 that hold them are loaded,
 * one 16-byte granule is stored; consecutive lanes store consecutive granules.
 * DY_ERR_ARG: a null pointer, n / H / W < 1, c_ < 8, a pitch below its width (c_, c_, 2 c_); DY_ERR_ALIGN: c_ % 8, a pitch that is no
 * multiple of 8, a pointer off a 16-byte boundary; nothing is launched then.  Every operand may be a channel slice of a wider tensor:
 * no other channel is touched.  No allocation, no synchronisation, no atomics; 64-bit offsets. */
int dy_gs_shuffle_forward(const void* x1, int ld1, const void* d, int ldd, void* y, int ldy, int n, int H, int W, int c_,
                          hipStream_t stream);
/* Its autograd, the inverse interleave: the gradient of x2[2 j] is dy[j], of x2[2 j + 1] dy[c_ + j]; the first c_ channels of that go to
 * dx1, the rest to dd.  A destination whose flag (acc1 / accd) is set receives fp16(old + v), one fp32 addition; otherwise it is
 * stored.  A null destination is skipped (its pitch is not looked at); both null: DY_OK, nothing launched.  Errors as above (dy is
 * required).  Two calls give the same bits. */
int dy_gs_shuffle_backward(const void* dy, int ldy, void* dx1, int ld1, int acc1, void* dd, int ldd, int accd, int n, int H, int W,
                           int c_, hipStream_t stream);
int dy_maxpool5(const void* x, int ldx, void* y, int ldy, void* argmax, int n, int h, int w, int C, hipStream_t stream);
int dy_maxpool5_backward(const void* dy, int lddy, const void* argmax, void* dx, int lddx, int n, int h, int w, int C,
                         int accumulate, hipStream_t stream);
/* SPPF's three chained pools (nn/modules/block.py:166-171) in one launch when a whole map fits in LDS.  cat: [n*h*w][ld] fp16, slice 0
 * (C channels) = cv1's output, slices 1..3 receive y1..y3; argK: [n*h*w][C] uint8 arg-max of pool K (as dy_maxpool5 writes it; may be
 * NULL in forward when no backward follows).  dy_sppf_pool3_supported: channels per workgroup (16 / 8) or 0 = use dy_maxpool5.
 * Backward: gcat holds the gradients of the four slices (from cv2's input gradient); on return slice 0 holds (accK: is added to)
 * the gradient of cv1's output; the gradients of y1 / y2 are consumed inside the kernel and not written back. */
int dy_sppf_pool3_supported(int h, int w, int C);
int dy_sppf_pool3(void* cat, int ld, int C, void* arg0, void* arg1, void* arg2, int n, int h, int w, hipStream_t stream);
int dy_sppf_pool3_backward(void* gcat, int ld, int C, const void* arg0, const void* arg1, const void* arg2, int n, int h, int w,
                           int acc0, int acc1, int acc2, hipStream_t stream);
int dy_scalseq_tail(const void* r0, int ld0, const void* r1, int ld1, const void* r2, int ld2, const void* res,
                    int ldres, void* y, int ldy, const float* coef, int n, int h, int w, int C, hipStream_t stream);
/* mode 0: BN3d backward partial sums for `level`; mode 1: dr_level */
int dy_scalseq_tail_backward(const void* r0, int ld0, const void* r1, int ld1, const void* r2, int ld2, const void* dy,
                             int lddy, void* dr, int lddr, const float* coef, const float* bwdcoef, float* partials,
                             int max_partials, int n, int h, int w, int C, int level, int mode, int* nparts,
                             hipStream_t stream);
/* all three levels in one pass (mode 0: BN partial sums [nparts][2][C]; mode 1: dr0/dr1/dr2 at full, 1/2, 1/4 resolution) */
int dy_scalseq_tail_backward_all(const void* r0, int ld0, const void* r1, int ld1, const void* r2, int ld2,
                                 const void* dy, int lddy, void* dr0, int lddr0, void* dr1, int lddr1, void* dr2,
                                 int lddr2, const float* coef, const float* bwdcoef, float* partials, int max_partials,
                                 int n, int h, int w, int C, int mode, int* nparts, hipStream_t stream);
/* The streaming kernel behind dy_scalseq_tail_backward_all runs a resident grid whose workgroups walk the nparts "virtual blocks" in turn.
 * This caps that physical grid (0 = default, four workgroups per CU) so that a test reaches several virtual blocks per workgroup on a
 * small shape; results do not depend on it.  Returns the previous cap.  Environment DY_TENSOR_OPS_V1=1 (read at every call) makes
 * dy_scalseq_tail_backward_all and dy_sppf_pool3 launch the kernels their current ones replaced (same bits). */
int dy_scalseq_bwd_grid_cap(int cap);
/* Zoom_cat fine branch nn/extra_modules/block.py:3406-3412: 2x2 max + 2x2 mean to half resolution (h, w = output extent) */
int dy_zoom_pool(const void* x, int ldx, void* y, int ldy, int n, int h, int w, int C, hipStream_t stream);
int dy_zoom_pool_backward(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int n, int h, int w, int C,
                          int accumulate, hipStream_t stream);
int dy_copy_slice(const void* x, int ldx, void* y, int ldy, long npix, int C, hipStream_t stream);
int dy_fill_zero(void* p, size_t bytes, hipStream_t stream);

/* ---- v8DetectionLoss.__call__ utils/loss.py:356-457 + TaskAlignedAssigner utils/tal.py:39-258 + BboxLoss
 *      utils/loss.py:202-250 + bbox_iou / wasserstein_loss / WiseIouLoss utils/metrics.py:75-126,540-565,591-645,
 *      forward AND backward (gradients w.r.t. the head logits are written as fp16 * gscale). ------------------------ */
typedef struct DyLossArgs {
  int nl, B, nc, ncp, nmax;      /* levels (<=4), batch, classes, classes padded to 8, gt capacity per image */
  const float* box[4];           /* (B,H,W,64) fp32 DFL logits per level */
  const float* cls[4];           /* (B,H,W,ncp) fp32 class logits per level */
  void* dbox[4];                 /* (B,H,W,64) fp16 out */
  void* dcls[4];                 /* (B,H,W,ncp) fp16 out */
  int H[4], W[4];
  float stride[4];
  const float* t_batch_idx;      /* (n,) targets as the dataloader emits them, data/dataset.py:207-224 */
  const float* t_cls;            /* (n,) */
  const float* t_boxes;          /* (n,4) normalised xywh */
  int n_targets;
  const int* n_targets_dev;      /* optional device copy of n_targets (read instead of n_targets when non-NULL, so a
                                    captured hipGraph sees per-step counts) */
  float img_w, img_h;
  float hyp_box, hyp_cls, hyp_dfl; /* cfg/default.yaml box/cls/dfl gains */
  int use_wiou, use_nwd;         /* BboxLoss.use_wiseiou / nwd_loss toggles, utils/loss.py:194,197 */
  float iou_ratio;
  const float* gscale;           /* device scalar: loss scale folded into every gradient */
  float* scalars;                /* 16 persistent floats: [1] target_scores_sum [3] #fg [4] WIoU iou_mean (init 1)
                                    [5..7] loss_items box,cls,dfl [8] loss.sum()*B [9] error flag */
  void* workspace;               /* dy_loss_workspace_bytes(B, A, nmax) bytes */
  int dbox_rows_only;            /* non-zero: dbox is written at foreground anchors only and NOT zeroed elsewhere -- for a consumer that
                                    reads it through the assignment (dy_conv1x1_rows_backward); 0: every row is defined */
  int box_from_input;            /* non-zero: box[] is not read.  pred_box in the workspace was written by dy_head_box_decode, and the DFL
                                    logits of foreground anchors are recomputed from the final box convolution's operands: */
  const void* box_in[4];         /* its input (B,H,W,box_in_ld) fp16, 64 channels */
  int box_in_ld[4];
  const float* box_w[4];         /* its fp32 weight (64,64) and bias (64) */
  const float* box_b[4];
  const float* box_in_coef[4];   /* NULL, or the BatchNorm coefficient table [4][64] of the Conv that produced box_in when box_in is that
                                    Conv's RAW output (no apply launch ran): BatchNorm + SiLU are applied where the rows are read */
  /* ---- extended box loss (abi v2).  All zero: the four legacy modes above (use_wiou / use_nwd), unchanged. ---- */
  int box_family;                /* DY_BOX_FAMILY_*: 0 legacy, 1 WiseIouLoss, 2 bbox_iou family; non-zero overrides use_wiou */
  int box_ltype;                 /* DY_BOX_* loss type */
  int box_fm;                    /* DY_BOX_FM_*: Wise focusing mechanism (family 1 only) */
  int box_modifier;              /* DY_BOX_MOD_*: the plain, Inner or Focaler IoU term */
  float inner_ratio;             /* get_inner_iou ratio, utils/metrics.py:186 (call sites: 0.7, utils/loss.py:207,213) */
  float focaler_d, focaler_u;    /* Focaler-IoU interval, utils/metrics.py:375,618 (call sites: 0.0, 0.95) */
  float shape_scale;             /* ShapeIoU scale, utils/metrics.py:153,685 (call site: 0.0, utils/loss.py:208) */
  float piou_lambda;             /* PIoU2 Lambda, utils/metrics.py:179,722 (default 1.3) */
} DyLossArgs;
/* box_family codes */
#define DY_BOX_FAMILY_LEGACY 0 /* BboxLoss.forward as shipped, utils/loss.py:206-218: CIoU or WIoU v3 per use_wiou */
#define DY_BOX_FAMILY_WISE 1   /* WiseIouLoss(ltype, monotonous, inner_iou, focaler_iou), utils/metrics.py:567-741, utils/loss.py:207-210 */
#define DY_BOX_FAMILY_BBOX 2   /* (1 - bbox_*iou(...)) * weight, utils/metrics.py:75-538, utils/loss.py:212-218 */
/* box_ltype codes: WiseIouLoss._<ltype> (family 1) / the bbox_iou flag or bbox_*mpdiou (family 2) */
#define DY_BOX_IOU 0      /* _IoU metrics.py:640 | bbox_iou() metrics.py:184 */
#define DY_BOX_WIOU 1     /* _WIoU metrics.py:643 (family 1 only) */
#define DY_BOX_EIOU 2     /* _EIoU metrics.py:647 | EIoU=True metrics.py:127-132 */
#define DY_BOX_GIOU 3     /* _GIoU metrics.py:652 | GIoU=True metrics.py:182-183 */
#define DY_BOX_DIOU 4     /* _DIoU metrics.py:655 | DIoU=True metrics.py:181 */
#define DY_BOX_CIOU 5     /* _CIoU metrics.py:658 | CIoU=True metrics.py:122-126 */
#define DY_BOX_SIOU 6     /* _SIoU metrics.py:665 | SIoU=True metrics.py:133-150 */
#define DY_BOX_SHAPEIOU 7 /* _ShapeIoU metrics.py:685 | ShapeIoU=True metrics.py:151-167 */
#define DY_BOX_PIOU 8     /* _PIoU metrics.py:708 | PIoU=True metrics.py:168-176 */
#define DY_BOX_PIOU2 9    /* _PIoU2 metrics.py:722 | PIoU2=True metrics.py:177-180 */
#define DY_BOX_MPDIOU 10  /* _MPDIoU metrics.py:680 | bbox_mpdiou / bbox_inner_mpdiou / bbox_focaler_mpdiou metrics.py:446-538;
                             mpdiou_hw = (img_h^2 + img_w^2) / stride^2 per level, utils/loss.py:445 */
/* box_fm codes (WiseIouLoss monotonous, metrics.py:568-572, _scaled_loss metrics.py:629-638) */
#define DY_BOX_FM_V1 1 /* monotonous=None: no focusing */
#define DY_BOX_FM_V2 2 /* monotonous=True: loss * sqrt(beta) */
#define DY_BOX_FM_V3 3 /* monotonous=False: loss * beta / (delta * alpha^(beta - delta)) */
/* box_modifier codes */
#define DY_BOX_MOD_PLAIN 0   /* inter / union */
#define DY_BOX_MOD_INNER 1   /* get_inner_iou metrics.py:186-218 (bbox_inner_iou metrics.py:220, inner_iou=True metrics.py:618) */
#define DY_BOX_MOD_FOCALER 2 /* clamp((iou - d) / (u - d), 0, 1) (bbox_focaler_iou metrics.py:333, focaler_iou=True metrics.py:618) */
int dy_loss_args_bytes(void); /* sizeof(DyLossArgs) in the library: bindings compare it with their own layout */
size_t dy_loss_workspace_bytes(int B, int A, int nmax);
/* byte offsets of pred_box (B,A,4 f32, grid units), assigned gt index (B,A i32, -1 = background) and target score
 * (B,A f32) inside the workspace after a call -- used by the parity tests */
int dy_loss_workspace_layout(int B, int A, int nmax, size_t* off_pred_box, size_t* off_asg_gt, size_t* off_tscore);
int dy_detection_loss(const DyLossArgs* args, hipStream_t stream);
/* Backward of Detect's final box convolution (nn/modules/head.py:38-40, Conv2d(c2, 4*reg_max, 1) with bias) from a gradient that has
 * ROWS: utils/loss.py:436-445 gives box / DFL terms to foreground anchors only, every other row of d(box logits) is zero.
 * assigned: the loss's per-anchor gt index (B, A) int32, -1 = background (workspace + off_asg_gt of dy_loss_workspace_layout);
 * this level's pixel (b, r) is anchor a0 + r.  Weight gradient: dy_conv1x1_rows_slabs(n, h, w) fp32 slabs [64][64] for
 * dy_wgrad_reduce_batched (descriptor: cin 64, cout 64, ks 1); bias gradient: fp64 sums into bias_acc [DY_BN_COPIES][64] (finished by
 * dy_wgrad_reduce_desc_bias); input gradient dx (may be NULL): W^T dy on foreground pixels, zeros (or untouched when dx_accumulate)
 * elsewhere.  Rows of dy whose anchor is background are never read.  Supported: cin == cout == 64. */
/* Forward of the same convolution fused with the loss's bbox_decode (utils/loss.py:347-354): pred_box (B, A, 4) in grid units, the
 * buffer at off_pred_box of the loss workspace; no logits are written (DyLossArgs.box_from_input). */
/* x_coef (both entries; may be NULL): x is the RAW output of the Conv below and x_coef its coefficient table [4][64] (scale, shift,
 * mean, invstd as dy_bn_act_apply_acc leaves them): BatchNorm + SiLU are applied on load -- what nn/modules/conv.py:49-55 computes,
 * without the launch and the tensor in between. */
int dy_head_box_decode(const void* x, int ldx, const float* x_coef, const float* weight, const float* bias, float* pred_box, int A, int a0,
                       int n, int h, int w, int cin, int cout, hipStream_t stream);
/* Detect's final CLASS convolution (nn/modules/head.py:41-42, Conv2d(c3, nc, 1) with bias) for nc <= 8, cin 32 or 64, as stand-alone
 * kernels.  Forward: logits (npix, 8) fp32, channels >= nc written as 0.  x_coef as above (RAW input + the coefficient table of the
 * Conv in front, or NULL for an activated input).  Backward, one walk: weight gradient as dy_cls_head_slabs() fp32 slabs [16][cin] for
 * dy_wgrad_reduce_batched, bias gradient as fp64 sums in bias_acc [DY_BN_COPIES][8], input gradient dx = W^T dy (stored, or added
 * when dx_accumulate; may be NULL).  dy: (npix, 8) fp16. */
int dy_cls_head_supported(int cin, int nc);
int dy_cls_head_slabs(void);
int dy_cls_head_forward(const void* x, int ldx, const float* x_coef, const float* weight, const float* bias, float* logits, long npix,
                        int cin, int nc, hipStream_t stream);
int dy_cls_head_backward(const void* x, int ldx, const float* x_coef, const void* dy, const float* weight, void* dx, int lddx,
                         int dx_accumulate, float* slabs, double* bias_acc, long npix, int cin, int nc, hipStream_t stream);
/* The four head entries for SEVERAL detection levels in one launch each (nl <= 4; array arguments have nl entries; the same kernels,
 * blockIdx picks the level): the small levels' latency-bound workgroups run beside the large level's instead of after it. */
int dy_head_box_decode_levels(int nl, const void* const* x, const int* ldx, const float* const* x_coef, const float* const* weight,
                              const float* const* bias, float* pred_box, int A, const int* a0, int n, const int* h, const int* w, int cin,
                              int cout, hipStream_t stream);
int dy_conv1x1_rows_backward_levels(int nl, const void* const* x, const int* ldx, const float* const* x_coef, const void* const* dy,
                                    const int* lddy, const int* assigned, int A, const int* a0, const float* const* weight, void* const* dx,
                                    const int* lddx, const int* dx_accumulate, float* const* slabs, double* const* bias_acc, int n,
                                    const int* h, const int* w, int cin, int cout, hipStream_t stream);
int dy_cls_head_forward_levels(int nl, const void* const* x, const int* ldx, const float* const* x_coef, const float* const* weight,
                               const float* const* bias, float* const* logits, const long* npix, int cin, int nc, hipStream_t stream);
int dy_cls_head_backward_levels(int nl, const void* const* x, const int* ldx, const float* const* x_coef, const void* const* dy,
                                const float* const* weight, void* const* dx, const int* lddx, const int* dx_accumulate, float* const* slabs,
                                double* const* bias_acc, const long* npix, int cin, int nc, hipStream_t stream);
int dy_conv1x1_rows_supported(int cin, int cout);
int dy_conv1x1_rows_slabs(int n, int h, int w);
int dy_conv1x1_rows_backward(const void* x, int ldx, const float* x_coef, const void* dy, int lddy, const int* assigned, int A, int a0,
                             const float* weight, void* dx, int lddx, int dx_accumulate, float* slabs, double* bias_acc, int n,
                             int h, int w, int cin, int cout, hipStream_t stream);
/* TaskAlignedAssigner.forward utils/tal.py:39-88 as a call of its own (topk 10, alpha 0.5, beta 6.0: what v8DetectionLoss builds,
 * utils/loss.py:311): scores[l] (B,H,W,ncp) class PROBABILITIES (pd_scores re-laid per level), pd_boxes_grid (B,A,4) xyxy in grid
 * units (pd_bboxes / stride), gt_labels (B,n) int32, gt_bboxes (B,n,4) xyxy pixels, mask_gt (B,n) int32.  Out: asg_gt (B,A) int32,
 * the assigned gt slot or -1 (fg_mask / target_gt_idx), tscore (B,A) = the normalised alignment metric at the assigned class
 * (target_scores).  workspace: dy_loss_workspace_bytes(B, A, n) bytes. */
int dy_tal_assign(const float* const* scores, const int* H, const int* W, const float* stride, int nl, int B, int nc, int ncp,
                  int n, const float* pd_boxes_grid, const int* gt_labels, const float* gt_bboxes, const int* mask_gt, int* asg_gt,
                  float* tscore, void* workspace, hipStream_t stream);

/* ---- Detect inference decode nn/modules/head.py:50-74 (+ DFL nn/modules/block.py:52-55, dist2bbox utils/tal.py:310-318)
 *      -> y (B, 4+nc, A) fp32 [xywh pixels, sigmoid class scores] ------------------------------------------------- */
/* The whole inference tail of Detect in ONE launch (nn/modules/head.py:50-74 `_inference` with its two final convs head.py:38-42):
 * per level l the box conv Conv2d(64, 64, 1) over x_box[l] and the class conv Conv2d(cin_cls, nc, 1) over x_cls[l] (fp16 NHWC, the
 * activated outputs of cv2[l][1] / cv3[l][1]; fp32 master weights (cout, cin) + bias), DFL expectation, dist2bbox(xywh) * stride and
 * sigmoid, written straight as y (B, 4+nc, A): no fp32 logits are written or re-read.  Same bits as dy_conv_forward (fp32 out + bias)
 * followed by dy_decode_predictions.  dy_head_infer_supported: 64 -> 64 box conv, nc <= 80, cin_cls a multiple of 16 up to 128. */
int dy_head_infer_supported(int cin_box, int cout_box, int cin_cls, int nc);
int dy_head_infer_levels(int nl, const void* const* x_box, const int* ld_box, const float* const* w_box, const float* const* b_box,
                         const void* const* x_cls, const int* ld_cls, const float* const* w_cls, const float* const* b_cls, const int* h,
                         const int* w, const float* stride, int n, int cin_cls, int nc, float* y, hipStream_t stream);
/* The same launch, which also writes the logits it computes on the way: per level box_logits[l] (B,H,W,64) and cls_logits[l]
 * (B,H,W,ncp) fp32, ncp = nc rounded up to 8 with channels [nc, ncp) exact zeros; 16-byte aligned.  Bit for bit what dy_conv_forward
 * (fp32 out + bias) writes over the same activations, and y bit for bit dy_head_infer_levels': a validation inside training hands the
 * logits to the loss without re-reading the activations.  Same supported shapes and error codes. */
int dy_head_infer_levels_logits(int nl, const void* const* x_box, const int* ld_box, const float* const* w_box, const float* const* b_box,
                                const void* const* x_cls, const int* ld_cls, const float* const* w_cls, const float* const* b_cls,
                                const int* h, const int* w, const float* stride, int n, int cin_cls, int nc, float* y,
                                float* const* box_logits, float* const* cls_logits, hipStream_t stream);
int dy_decode_predictions(const float* const* box, const float* const* cls, const int* H, const int* W,
                          const float* stride, int nl, int B, int nc, int ncp, float* y, hipStream_t stream);
/* ---- ops.non_max_suppression utils/ops.py:292-427: candidate extraction (:344-392, order-preserving) ... */
int dy_nms_candidates(const float* pred, int B, int nc, int A, float conf, int multi_label, const int* classes,
                      int n_classes, float* cbox, float* cscore, float* ccls, int* ccount, int cap, hipStream_t stream);
/* ---- ... the candidate cap utils/ops.py:395-396 ``x = x[x[:, 4].argsort(descending=True)[:max_nms]]``: per image with more than
 *      max_nms candidates the max_nms most confident ones in descending confidence (ties in candidate order: the reference's
 *      unstable argsort leaves them unspecified); other images are copied through.  Outputs (B,max_nms,4) / (B,max_nms); count is
 *      clamped in place.  workspace: dy_nms_presort_workspace(B, max_nms) bytes. */
size_t dy_nms_presort_workspace(int B, int max_nms);
int dy_nms_presort(const float* cbox, const float* cscore, const float* ccls, int* count, int B, int cap, int max_nms, float* obox,
                   float* oscore, float* ocls, void* workspace, hipStream_t stream);
/* ---- ... and ops.soft_nms utils/ops.py:260-290 with bbox_iou_for_nms :162-199 (sequential semantics kept; scores are
 *      decayed in place; keep/nkeep receive the kept candidate indices per image) ---------------------------------- */
int dy_soft_nms(const float* boxes, float* scores, const float* cls, const int* count, int* order_a, int* order_b,
                int* keep, int* nkeep, int B, int cap, float iou_thr, float sigma, float score_thr, float class_offset,
                hipStream_t stream);

/* ---- BaseTrainer.optimizer_step engine/trainer.py:949-957 + build_optimizer groups :1146-1174 + ModelEMA.update
 *      utils/torch_utils.py:447-458 + GradScaler policy, over flat fp32 buffers.  mode: 0 SGD-nesterov, 1 Adam, 2 AdamW,
 *      3 RMSprop, 4 RAdam, 5 Adamax, 6 NAdam (betas = (momentum, 0.999) as build_optimizer :1159-1164 sets them). -------------- */
int dy_optimizer_step(float* params, const float* grads, float* mom, float* adam_v, float* ema, long n, long g0_end,
                      long g1_end, const unsigned char* frozen, const float* buffers, float* ema_buffers,
                      long n_buffers, const float* hyper, float* state, float* partials, int mode, hipStream_t stream);
/* The same step over a flat buffer of SIX segments [bucket A: bias | decayed | norm][bucket B: bias | decayed | norm] (seg_ends: the ends
 * of the first five, host array): each data-parallel gradient bucket is then ONE contiguous slice that RCCL reduces in place -- DDP's
 * reducer works on contiguous buckets too (engine/trainer.py:694-695).  Segment k takes the hyper-parameters of group k % 3. */
int dy_optimizer_step_seg(float* params, const float* grads, float* mom, float* adam_v, float* ema, long n, const long* seg_ends,
                          const unsigned char* frozen, const float* buffers, float* ema_buffers, long n_buffers, const float* hyper,
                          float* state, float* partials, int mode, hipStream_t stream);
/* hyper (16 device floats read by dy_optimizer_step: lr per group, momentum, weight decay per group, EMA decay, max grad norm,
 * beta2, eps) set from 16 HOST floats that are copied at enqueue time (kernel arguments): safe however far the host runs ahead. */
int dy_set_hyper(float* hyper_dev, const float* host_values16, hipStream_t stream);
int dy_axpy_f32(float* y, const float* x, float a, long n, hipStream_t stream);

/* ---- optimizer='SOAP': the reference trainer's SOAP class (engine/trainer.py:54-473, built by build_optimizer :1156-1165) over the
 *      flat fp32 buffers, one table-driven launch per kind of work (csrc/soap.hip; the host side is ultralytics/hip/soap.py).
 * One table entry per TRAINABLE tensor (a frozen tensor has none), in device memory.  Entries hold offsets, not pointers: the gradient
 * base differs between the step's gradient buffer and the accumulation buffer.  All Gram matrices of the model live in one pool and
 * all eigenbases in another of the same layout, grouped by matrix size n so that the n x n matrices form one (count_n, n, n) tensor.
 * The *_blk columns give the first workgroup of the entry in each launch (the host sums the tile counts); a workgroup finds its entry
 * by binary search, so no launch count depends on the number of tensors. */
#define DY_SOAP_MAX_DIMS 5
typedef struct DySoapDesc {
  long off;                         /* first element in the flat parameter layout (params, grads, m, v, scratch) */
  long numel;
  long pool_off[DY_SOAP_MAX_DIMS];  /* per dimension: first float of its n x n Gram matrix / eigenbasis in the pools */
  int group;                        /* optimizer group 0 bias, 1 decayed weights, 2 norm weights */
  int ndim;                         /* 1..DY_SOAP_MAX_DIMS */
  int shape[DY_SOAP_MAX_DIMS];      /* unused dimensions 1 */
  int has_q[DY_SOAP_MAX_DIMS];      /* 1: the dimension keeps a Gram matrix and a basis; 0: none (a 1-D tensor, a dimension above
                                       max_precond_dim): it passes through every rotation */
  int ord_off[DY_SOAP_MAX_DIMS];    /* per dimension: first int of its order vector (n ints) in the order pool of a QR refresh */
  int rot_blk[DY_SOAP_MAX_DIMS];    /* first workgroup in dimension k's dy_soap_rotate launch: 32 x 32 output tiles,
                                       ceil(n / 32) * ceil(numel / n / 32) of them, or ceil(numel / 1024) where it passes through */
  int gram_blk[DY_SOAP_MAX_DIMS];   /* first workgroup of (entry, k) in the dy_soap_gram launch: 1 where n <= 8, else ceil(n / 32)^2;
                                       a dimension without a Gram matrix takes none */
  int ew_blk;                       /* first workgroup in the element-wise launches: ceil(numel / 1024) each */
  int reserved;
} DySoapDesc;
int dy_soap_desc_bytes(void); /* sizeof(DySoapDesc) in the library (bindings check their layout) */
/* The first two launches of dy_optimizer_step on their own (GradScaler.unscale_ + clip_grad_norm_, engine/trainer.py:949-953):
 * state[2] found_inf, state[3] the unscaled norm, state[4] the clip coefficient.  Every SOAP entry below reads found_inf on the device
 * and leaves its outputs untouched when it is set; the unscale x clip factor is (1 / state[0]) * state[4]. */
int dy_grad_norm(const float* grads, long n, const float* hyper, float* state, float* partials, hipStream_t stream);
/* SOAP.project / project_back (engine/trainer.py:283-309, :352-378) for dimension `dim` of every tensor: viewed as (A, n, B) around
 * it, dst[a, j, b] = sum_i src[a, i, b] * Q[i, j] (back: Q[j, i]); a tensor without a basis there is copied.  Applied for dim = 0 ..
 * max ndim - 1 this is the reference's chain of tensordots (only the summation order inside a dot product differs).  scaled: src is
 * the raw gradient, multiplied by the unscale x clip factor as it is read.  dst != src. */
int dy_soap_rotate(float* dst, const float* src, const DySoapDesc* table, int n_tensors, int n_blocks, const float* basis, int dim,
                   int back, int scaled, const float* state, hipStream_t stream);
/* SOAP.update_preconditioner's Gram update (engine/trainer.py:311-350, the lerp_ of :320-341): GG <- GG + (1 - beta2) *
 * (G_(k) G_(k)^T - GG) for every (tensor, dimension) that keeps one, G_(k) the mode-k unfolding of the unscaled, clipped gradient.
 * Each output tile is summed by one workgroup in a fixed order. */
int dy_soap_gram(float* gram, const float* grads, const DySoapDesc* table, int n_tensors, int n_blocks, float one_minus_beta2,
                 const float* state, hipStream_t stream);
/* SOAP.step's moments in the eigenbasis (engine/trainer.py:152-255, :210-213): m <- beta1 m + (1 - beta1) gp, v <- beta2 v +
 * (1 - beta2) gp^2, upd = m / (sqrt(v) + eps) over every table entry; gp and upd may be the same buffer. */
int dy_soap_adam(float* m, float* v, const float* gp, float* upd, const DySoapDesc* table, int n_tensors, int n_blocks, float beta1,
                 float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* state, hipStream_t stream);
/* ... and its parameter update (:221-247): p <- p - size3[group] * upd, then p <- p - decay3[group] * p where decay3[group] > 0
 * (decay = lr * weight_decay).  size3 / decay3: three HOST floats each, copied at enqueue time (kernel arguments, as dy_set_hyper). */
int dy_soap_apply(float* params, const float* upd, const DySoapDesc* table, int n_tensors, int n_blocks, const float* size3,
                  const float* decay3, const float* state, hipStream_t stream);
/* get_orthogonal_matrix_QR's exp_avg_sq.index_select(dim, sort_idx) (engine/trainer.py:416-473, :457) for dimension `dim` of every
 * tensor: dst[a, j, b] = src[a, order[j], b]; a tensor without a basis there is copied.  dst != src. */
int dy_soap_permute_v(float* dst, const float* src, const DySoapDesc* table, int n_tensors, int n_blocks, const int* order, int dim,
                      const float* state, hipStream_t stream);

/* ---- validation: the per-batch half of DetectionValidator.update_metrics in ONE launch --
 *      _prepare_batch/_prepare_pred (models/yolo/detect/val.py:93-115: xywh2xyxy * imgsz, scale_boxes + clip_boxes),
 *      box_iou (utils/metrics.py:53-73) and BaseValidator.match_predictions (engine/validator.py:217-257, numpy path).
 *      preds (Ntot,6) x1 y1 x2 y2 conf cls packed over the batch, pred_off (B+1); targets as the collate function gives
 *      them (batch_idx, cls, xywh normalised); geom (B,5) = gain, padw, padh, ori_h, ori_w per image; iouv (niou <= 16);
 *      tp (Ntot,niou) uint8; predn (Ntot,6) native-space predictions or NULL; *status |= 1 if an image has > 1024 labels. */
int dy_match_predictions(const float* preds, const int* pred_off, const float* t_batch_idx, const float* t_cls,
                         const float* t_boxes, int n_targets, const float* geom, const float* iouv, int niou, int B,
                         int img_h, int img_w, unsigned char* tp, float* predn, int* status, hipStream_t stream);
/* utils/metrics.py:53-73 box_iou: (n,4) x (m,4) xyxy fp32 -> (n,m) */
int dy_box_iou(const float* box1, int n, const float* box2, int m, float* out, hipStream_t stream);

/* ---- two-stage ("double") inference, double_inference.py:98-305 ----------------------------------------------------
 * crop + resize + letterbox of K rectangles of one HBM-resident uint8 HWC image into a (K,S,S,3) batch
 * (prepare_cropped_image_cv2 :129-149; rects x1,y1,x2,y2 with exclusive x2/y2; geom new_w,new_h,pad_x,pad_y per crop). */
int dy_crop_letterbox_u8(const void* img, int H, int W, const int* rects, const int* geom, int K, int S, void* out,
                         hipStream_t stream);
/* per first-stage detection: map its crop's second-stage rows back (scale_boxes_vectorized :152-161) and pick the
 * replacement of process_refined_boxes_optimized :263-303.  dets: packed (x1,y1,x2,y2,conf,cls) rows, offsets (K+1),
 * orig (K,6), scale (K,3) ratio,pad_x,pad_y; out (K,6), found (K). */
int dy_refine_select(const float* dets, const int* offsets, const float* orig, const int* rects, const float* scale, int K,
                     float img_w, float img_h, float* out, int* found, hipStream_t stream);
/* greedy per-class NMS in descending score order, suppress IoU > iou_thr (torchvision_nms :164-203); n <= 2048; keep: n bytes */
int dy_nms_hard(const float* boxes, const float* scores, const float* labels, int n, float iou_thr, void* keep,
                hipStream_t stream);

/* ---- two-stage inference over a chunk of N images, double_inference.py main :509-562 (process_image_optimized :404-449 per image,
 *      calculate_metrics_optimized :306-333 for the counts): the three kernels above for many images per launch.
 * dy_crop_letterbox_u8 for K crops of N images of different sizes in one launch (the per-image open / crop / resize / pad of
 * perform_batch_double_inference :206-226).  pool: the uint8 HWC images back to back; img_off (N) int64 byte offsets, any alignment;
 * img_hw (N,2) height, width; crop_img (K) the image of each crop; rects / geom / out as dy_crop_letterbox_u8.  Every crop holds the
 * bits dy_crop_letterbox_u8 writes for its image alone.  The caller guarantees 0 <= crop_img[k] < N and rects inside their image. */
int dy_crop_letterbox_u8_multi(const void* pool, const long* img_off, const int* img_hw, const int* crop_img, const int* rects,
                               const int* geom, int K, int S, void* out, hipStream_t stream);
/* dy_refine_select with the bounds filter of process_refined_boxes_optimized (:277-280: x2 <= img_w, y2 <= img_h) taken from the
 * crop's own image: crop_img (K), img_hw (N,2) height, width. */
int dy_refine_select_multi(const float* dets, const int* offsets, const float* orig, const int* rects, const float* scale,
                           const int* crop_img, const int* img_hw, int K, float* out, int* found, hipStream_t stream);
/* The rest of process_image_optimized (:430-444) and calculate_metrics_optimized (:306-333) for N images in one launch, one workgroup
 * per image.  rows (M,6) x1 y1 x2 y2 conf cls: the first-stage detections of the chunk with row_off (N+1), in/out; refined (K,6) and
 * found (K) from dy_refine_select_multi with crop_off (N+1); crop_row (K) indexes rows and ascends within an image; labels (L,5) fp32
 * cls x1 y1 x2 y2 in native pixels (load_ground_truth :492-506) with lab_off (N+1).
 *  1. apply: aligned != 0, a found refinement k replaces rows[crop_row[k]]; aligned == 0, the script's zip (:431): the j-th FOUND
 *     refinement of an image replaces rows[crop_row[crop_off[b] + j]].
 *  2. dy_nms_hard on the image's rows after step 1 -> keep (M) bytes.  nms_iou < 0 skips the sweep (every row kept).
 *  3. the kept rows in stored order each take, among the unmatched labels of their class, the one of largest IoU (calculate_iou_tensor,
 *     fp32) if it is >= match_iou and > 0; ties to the first label.  counts (N,3) int32 = tp, fp, fn.
 * *status |= 1 and nothing is written for an image with more than 2048 rows or 1024 labels. */
int dy_two_stage_merge(float* rows, const int* row_off, const float* refined, const int* found, const int* crop_row,
                       const int* crop_off, int aligned, float nms_iou, const float* labels, const int* lab_off, float match_iou,
                       int N, void* keep, int* counts, int* status, hipStream_t stream);

/* ---- test-time augmentation, reference nn/tasks.py:335-371 (DetectionModel._predict_augment / _descale_pred / _clip_augmented) and
 *      utils/torch_utils.py:355-366 (scale_img); the pass geometry is host arithmetic (ultralytics/hip/tta.py).
 * scale_img of one pass in one launch: x (B, 3, H, W) fp32 NCHW -> out (B, 3, Hp, Wp) fp32 NCHW = x flipped (flip 0: none,
 * 2: up-down, 3: left-right), resized into the top-left Ho x Wo with F.interpolate(mode='bilinear', align_corners=False) index
 * arithmetic (sizes given, no scale factor), the rest filled with (float)0.447.  Ho <= Hp, Wo <= Wp; Ho == H and Wo == W copies. */
int dy_scale_img(const float* x, int B, int H, int W, int flip, int Ho, int Wo, int Hp, int Wp, float* out, hipStream_t stream);
/* _descale_pred + _clip_augmented + torch.cat(y, -1) of n_pass (<= 4) passes in one launch: pass k's output y_ptrs[k] (B, no, A[k])
 * contributes its columns [col_lo[k], col_hi[k]) to out (B, no, sum_k (col_hi[k] - col_lo[k])), rows 0-3 divided by scale[k] (the
 * correctly rounded quotient), then x = W - x for flip[k] == 3, y = H - y for flip[k] == 2; (H, W) is the original input size.
 * Host arrays y_ptrs .. flip; out must not overlap any y. */
int dy_tta_merge(int n_pass, const float* const* y_ptrs, const int* A, const int* col_lo, const int* col_hi, const float* scale,
                 const int* flip, int B, int no, int H, int W, float* out, hipStream_t stream);

/* ---- paired bootstrap of the validation statistics, reference testandcox.py:150-227 (30 resamples of the test split, one full
 *      ``model.val`` per resample and model) with ultralytics/utils/metrics.py compute_ap (:1109-1139) / ap_per_class (:1142-1230):
 *      AP of every (resample, class, IoU threshold) from ONE validation pass in one launch, one workgroup per (resample, class).
 * Per model, prepared once: the D detections sorted by (class, confidence descending, stable) -- tp_bits[d] bit j = true positive at
 * IoU threshold j of the validator's ten, det_img[d] = image index -- cls_off (nc + 1) = the class segments of that order, lab_cnt
 * (n_img, nc) = labels per image and class.  Per call: mult (S, n_img) uint16 = how often image i occurs in resample s.
 * ap (S, nc, 10) fp64 = what compute_ap returns for the list in which every detection of image i appears mult[s, i] times (recall =
 * tpc / (n_l + 1e-16), sentinels (0, 1) / (1, 0), right-to-left envelope, np.interp on linspace(0, 1, 101), trapezoid); 0 where the
 * class has no label or no detection in the resample.  nl (S, nc) = sum_i mult[s, i] * lab_cnt[i, c].  No workspace: nothing of size
 * D or S x D is written.  The weighted detections of one class and resample must stay below 2^31 (callers check on the host). */
int dy_bootstrap_ap(const unsigned short* tp_bits, const int* det_img, const int* cls_off, const int* lab_cnt,
                    const unsigned short* mult, int D, int n_img, int nc, int S, double* ap, int* nl, hipStream_t stream);

/* ---- detection confusion matrix, reference ultralytics/utils/metrics.py:935-986 (ConfusionMatrix.process_batch; box_iou :53-73), as
 *      the reference validator fills it per labelled image (models/yolo/detect/val.py:136-152), for a whole batch in ONE launch, one
 *      workgroup per image.  predn (n_preds,6) native-space x1 y1 x2 y2 conf cls with pred_off (B+1): what dy_match_predictions writes;
 *      targets and geom as dy_match_predictions takes them (same native-space formulas).  geom NULL: t_boxes are native xyxy already.
 *      pred_off NULL / t_batch_idx NULL (B == 1 only): the one image owns all n_preds detections / all n_targets labels.
 * Rule: detections with conf > conf_thr each choose the label of largest IoU among IoU > iou_thres (any class); a label keeps the
 * chooser of largest IoU.  matrix (nc+1,nc+1) int32, [predicted, true], index nc = background, is ADDED to (caller zeroes it): a
 * label with a winner -> [cls(winner), cls(label)], without -> [nc, cls(label)]; only if the image has a matched pair (the
 * reference's ``if n:``, :983), every other kept detection -> [cls(det), nc].  An image without labels adds nothing when
 * skip_unlabelled (the validator), else its kept detections -> [cls, nc] (:945-951).  Exact IoU ties, undefined in the reference
 * (unstable argsort), go to the lower label index, then the lower detection index.
 * *status |= 1 if an image has > 1024 labels, |= 2 if a class lies outside [0, nc) (that entry is not counted). */
int dy_confusion_matrix(const float* predn, const int* pred_off, int n_preds, const float* t_batch_idx, const float* t_cls,
                        const float* t_boxes, int n_targets, const float* geom, int B, int img_h, int img_w, int nc, float conf_thr,
                        float iou_thres, int skip_unlabelled, int* matrix, int* status, hipStream_t stream);
/* ---- false-positive count, reference gt_fails.py:35-84 (count_fp with load_labels :9-16, yolo_to_xyxy :18-23, iou :25-33), for a
 *      batch of images in one launch, one wave per image.  dets (Ntot,6) native pixels with det_off (B+1); labels (Ltot,5) fp64 rows
 *      cls xc yc w h in file order with lab_off (B+1); wh (B,2) image width, height.  Detections with conf >= conf_thr, in stored
 *      order, each take the FIRST unused label of the same class with inter / (area_a + area_b - inter + 1e-6) >= iou_thr (labels
 *      xc*w -+ bw*w/2, unclipped); fp[b] = detections that found none.  The script's mix of float32 and float64 is replaced by fp64
 *      arithmetic on the fp32 detections: equal away from the threshold.  *status |= 1 if an image has > 1024 labels. */
int dy_count_fp(const float* dets, const int* det_off, const double* labels, const int* lab_off, const int* wh, int B, float conf_thr,
                double iou_thr, int* fp, int* status, hipStream_t stream);

/* ---- sliced (tiled) inference for frames much larger than the model input (ultralytics/utils/tiled.py): the frame is cut into
 *      overlapping S x S tiles, optionally plus one letterboxed view of the whole frame; every record goes through the model at S x S
 *      and the detections of all records are merged per frame.
 * dy_tile_gather_f32: K records of N images into out (K,3,S,S) fp32 planar -- the input tensor of the forward itself.  pool / img_off /
 * img_hw / rects / geom as dy_crop_letterbox_u8_multi; tile_img (K) the image of each record, < 0 = a pad canvas (all 114; its rect and
 * geom are not read).  Every value is lut[u] with u the byte dy_crop_letterbox_u8_multi writes for that pixel and channel; lut (256)
 * device floats, the caller's byte -> float conversion (u / 255 as the caller's framework rounds it).  A thread writes four pixels of a
 * row per plane as one 16-byte store when S % 4 == 0 and out is 16-byte aligned, single floats otherwise.  The caller guarantees
 * tile_img[k] < N and rects inside their image. */
int dy_tile_gather_f32(const void* pool, const long* img_off, const int* img_hw, const int* tile_img, const int* rects, const int* geom,
                       const float* lut, int K, int S, float* out, hipStream_t stream);
/* dy_tile_merge: N images in one launch, one workgroup per image.  rows (M,6) x1 y1 x2 y2 score label in the coordinates of their
 * record's canvas, packed image-major with row_off (N+1); row_tile (M) indexes tiles (Kt,6) = x1, y1, pad_x, pad_y, r, 1/r of the
 * record (fp32; 1/r the correctly rounded reciprocal); img_hw (N,2) height, width.
 *  1. out (M,6): every coordinate v -> (v - pad) / r + origin in fp32, each operation rounded once (the quotient is the correctly
 *     rounded one; r == 1 gives v + origin exactly), x clipped to [0, W], y to [0, H].  A row whose clipped width or height is <= 0 (or
 *     whose score is NaN) is written but takes no further part.
 *  2. per image the remaining rows in descending score, ties to the lower row index; walking that order, a surviving row is kept and
 *     removes every later surviving row of the same label (any label when agnostic) whose metric with it is > thr.  metric 0: IoU
 *     (0 for an empty intersection or a non-positive area, no epsilon); 1: the same intersection over the smaller of the two areas.
 *  order (M): the kept row indices (into rows) of image i in that order from order[row_off[i]]; nkeep (N) their number.
 * max_rows: the largest row count of an image (the host knows it; row_off is device memory): above DY_TILE_MERGE_MAX_ROWS the call
 * returns DY_ERR_CAPACITY and launches nothing -- never a truncated result.  *status |= 1 if an image nevertheless exceeds the
 * capacity (it gets nkeep 0), |= 2 if a row_tile lies outside [0, Kt) (that row is copied through and dropped). */
#define DY_TILE_MERGE_MAX_ROWS 8192
int dy_tile_merge(const float* rows, const int* row_off, const int* row_tile, const float* tiles, const int* img_hw, int N, int Kt,
                  int max_rows, float thr, int metric, int agnostic, float* out, int* order, int* nkeep, int* status,
                  hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
