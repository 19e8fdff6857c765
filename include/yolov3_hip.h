/*
 * yolov3_hip.h -- C ABI of libyolov3_hip.so: the MI355X (gfx950) YOLOv3 inference hot path.
 *
 * The reference (nrsyed/pytorch-yolov3) has no FFI layer: its hot path is the Python
 * call chain Darknet.forward -> YOLOLayer.forward -> inference() tail -> non_max_suppression.
 * Each entry point below replaces the arithmetic of one of those call sites; the Python
 * package pytorch-yolov3_amd/yolov3 keeps the reference's signatures and binds these
 * symbols with ctypes.  Citations are into /root/reference.
 *
 * Conventions
 *   - plain C types only; every pointer named d_* is a DEVICE address (hipMalloc'd by the
 *     caller, e.g. torch tensor .data_ptr()); the library never allocates or frees caller-visible memory and never
 *     synchronises the device.  One exception, for callers that do not pass y3_op.d_weight_frag: a plan then makes and owns a
 *     private fragment-order copy of the weights of every layer it gives to the direct-weights strip kernel (hipMalloc at
 *     y3_plan_create on the device that owns d_weight, one stream synchronisation there, hipFree at y3_plan_destroy);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - every function returns 0 on success, a negative Y3_ERR_* code otherwise, and
 *     y3_last_error() then returns a human-readable message (thread-local);
 *   - activations are NHWC ("pixel-major"): element (b, y, x, c) of a tensor with pixel
 *     stride ld lives at ((b*H + y)*W + x)*ld + c;  ld >= C, and ld*sizeof(elem) as well
 *     as every channel-slice offset are multiples of 16 bytes on the MFMA path;
 *   - one plan / one stream per GPU; entry points are not re-entrant per plan.
 */
#ifndef YOLOV3_HIP_H
#define YOLOV3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y3_ABI_VERSION 6

/* error codes */
#define Y3_OK 0
#define Y3_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define Y3_ERR_HIP (-2)       /* a HIP runtime call failed        */
#define Y3_ERR_NODEVICE (-3)  /* no gfx950 device visible         */

/* element types of activations / weights */
#define Y3_F32 0
#define Y3_BF16 1
#define Y3_F16 2   /* IEEE half storage, float32 accumulation: every kernel of the bf16 mode instantiated on
                      v_mfma_f32_16x16x32_f16 (same rate, same bytes, 11 instead of 8 significand bits) */
#define Y3_F64 3   /* float64: box coordinates handed to y3_nms_float / y3_cxywh_to_tlbr_float only (no network runs in it) */

/* op kinds of a plan (one per Darknet block that does work) */
#define Y3_OP_CONV 1      /* conv -> (BN as per-channel scale/bias) -> LeakyReLU -> (+residual)  darknet.py:236-264, :376-379 */
#define Y3_OP_MAXPOOL 2   /* darknet.py:16-29 (zero-pad right/bottom quirk when stride==1): stride 1 takes the window
                             [y, y+k) x [x, x+k) and counts out-of-range taps as 0.0; other strides pool unpadded,
                             out = (in - k) / stride + 1.  With Y3_F_POOL_DARKNET: Darknet's own rule instead, with
                             p = y3_op.pad: out = (in + p - k) / stride + 1, window origin o * stride - p / 2, taps
                             outside the image ignored (size k odd, stride 1, p = k - 1: the centred "same" pool)  */
#define Y3_OP_UPSAMPLE 3  /* nearest, integer factor: darknet.py:299-305                        */
#define Y3_OP_ADD 4       /* unfused shortcut: darknet.py:376-379                               */
#define Y3_OP_COPY 5      /* unfused route slice copy: darknet.py:369-375                       */
#define Y3_OP_YOLO 6      /* YOLOLayer.forward + head concat + wh/net size: darknet.py:48-122, :389-399 */
#define Y3_OP_REORG 7     /* Darknet's [reorg] (YOLOv2's pass-through layer), factor s = y3_op.stride: (C, H, W) per frame ->
                             (C*s*s, H/s, W/s).  Needs H % s == 0 and W % s == 0.  Two forms, both stated on the frame's NCHW
                             arrays (the kernel works on the NHWC tensors with their pixel strides in_ld / out_ld):
                               default -- Darknet's original layer (later Darknet: "reorg_old"), what the published yolov2
                               weights were trained with.  Needs C % (s*s) == 0.  With oc = C / (s*s), for k < C, j < H, i < W:
                                 c2 = k % oc, off = k / oc, w2 = i*s + off % s, h2 = j*s + off / s
                                 out_flat[i + W*(j + H*k)] = in_flat[w2 + (W*s)*(h2 + (H*s)*c2)]
                               with both arrays C*H*W floats long and out_flat then read as (C*s*s, H/s, W/s): a fixed
                               permutation of the frame's elements that is NOT a space-to-depth;
                               Y3_F_REORG_3D -- the space-to-depth of later Darknet ([reorg3d]): for k < C*s*s, g = k / C:
                                 out[k][j][i] = in[k % C][j*s + g / s][i*s + g % s].
                             A move of storage elements: bit-exact in every dtype.  in_c = C, out_c = C*s*s, out_h = H/s,
                             out_w = W/s.  y3_capabilities() reports Y3_CAP_REORG                                        */
/* The attention blocks of Darknet (csrc/attention.hip, libyolov3_hip_attn.so; y3_capabilities() reports Y3_CAP_ATTENTION).  All three
 * read and write NHWC tensors of the op's dtype with their pixel strides, take no flag at all (none of y3_op.flags: the op never
 * reads the plan's input and never stores float32 from 16-bit storage), and have a 16-byte form (8 elements of 16-bit storage,
 * 4 of float32 per thread) and an element form, taken where in_c, a pixel stride or a base address is off the 16-byte grain;
 * both forms give the same bits.  d_in, in_h, in_w, in_c, in_ld describe `prev`, the output of the block in front; d_res and
 * res_ld describe `src`, the block the cfg's `from` names (as in Y3_OP_ADD); out_* the output.  in_c == out_c.             */
#define Y3_OP_AVGPOOL 8   /* [avgpool]: global average pool, (C, H, W) -> (C, 1, 1); out_h = out_w = 1.  With P = in_h * in_w:
                               out[b][c] = round_to_storage(S / float32(P))
                             with the correctly rounded float32 division and S the float32 sum of prev[b][.][.][c] in ONE order,
                             a function of P only (not of batch, channel count, strides, the form that runs, the grid or
                             y3_set_tuning("device_cus", n)); pixels p = y * W + x:
                               32 partial sums s[0..31] start at +0.0f; s[r] adds pixels r, r + 32, r + 64, ... in increasing order;
                               then s[r] += s[r + 16] for r < 16, s[r] += s[r + 8] for r < 8, and so on with 4, 2, 1;  S = s[0].
                             (numpy float32: s = zeros(32); for p in range(P): s[p % 32] += x[p]; then for h in 16, 8, 4, 2, 1:
                             s[:h] += s[h:2*h].)  No atomics.  A sum of integer-valued inputs below 2^24 is exact in any order.  */
#define Y3_OP_SCALE_CHANNELS 9 /* [scale_channels]: out[b][y][x][c] = round_to_storage(float32(src[b][y][x][c]) * float32(prev[b][c])):
                             prev is (C, 1, 1) (in_h = in_w = 1), out has src's shape.  The float32 product of two bf16 values,
                             and of two fp16 values, is exact, so in both 16-bit modes the result is the exact product rounded
                             once (nearest even); in float32 it is the IEEE product.  Zeros keep their sign, 0 * inf and NaN
                             operands give NaN.  float32 denormal products are KEPT (not flushed), as add_kernel's denormal sums
                             are: the kernels are compiled with IEEE denormal handling for float32, hipcc's default on gfx950.  */
#define Y3_OP_SAM 10      /* [sam]: out = round_to_storage(float32(src) * float32(prev)) element by element, prev of src's shape
                             (in_h == out_h, in_w == out_w); the arithmetic of Y3_OP_SCALE_CHANNELS                         */

/* y3_op.flags */
#define Y3_F_LEAKY 1u          /* LeakyReLU(0.1) after scale/bias                        */
#define Y3_F_RESIDUAL 2u       /* add d_res (same dtype as output) after the activation  */
#define Y3_F_OUT_F32 4u        /* store float32 regardless of dtype (detection-head convs) */
#define Y3_F_IN_NCHW_F32 8u    /* conv input is the network input, float32 (B,C,H,W) in [0,1]  (inference.py:332-335) */
#define Y3_F_IN_NHWC_U8BGR 16u /* conv input is uint8 (B,H,W,3) BGR frames; kernel applies BGR->RGB and /255.0 (inference.py:332-333) */
#define Y3_F_PLAN_INPUT 32u    /* d_in is supplied at y3_plan_run time                  */
#define Y3_F_FUSE_NEXT 64u     /* plan hint: this conv's output is read by the NEXT op only, so the executor may run
                                  both as one kernel (stem + stride-2 conv) and never materialise d_out      */
#define Y3_F_MISH 128u         /* mish, x * tanh(softplus(x)), after scale/bias instead of LeakyReLU (YOLOv4's backbone);
                                  exclusive with Y3_F_LEAKY; Y3_F_RESIDUAL still adds after it.  Kernels that do not
                                  implement it decline the op; y3_capabilities() reports Y3_CAP_MISH             */
#define Y3_F_LOGISTIC 256u     /* logistic, 1 / (1 + e^-x), after scale/bias (the detection-head convs of new_coords networks:
                                  Scaled-YOLOv4); exclusive with Y3_F_LEAKY and Y3_F_MISH; Y3_F_RESIDUAL still adds after it.
                                  Exactly 1 above x ~ 17, exactly 0 below x ~ -88.7; y3_capabilities() reports Y3_CAP_LOGISTIC */
#define Y3_F_NEW_COORDS 512u   /* Y3_OP_YOLO: Darknet's new_coords=1 decode of a head whose conv ends in Y3_F_LOGISTIC: the inputs are
                                  probabilities already, so centre = (sxy(t) + cell) / grid, size = t * t * 4 * anchor / net,
                                  prob = objectness * max_c t_c (no exp, no soft-max); y3_capabilities() reports Y3_CAP_NEW_COORDS */
#define Y3_F_POOL_DARKNET 1024u /* Y3_OP_MAXPOOL: Darknet's pooling rule.  y3_op.pad carries the cfg's `padding` p (Darknet's default:
                                  ksize - 1); out_h = (in_h + p - ksize) / stride + 1, likewise out_w; output (i, j) is the max
                                  over n, m in [0, ksize) of in[i * stride + n - p / 2][j * stride + m - p / 2], taking only taps
                                  inside the image (integer p / 2).  An op some window of which would hold no tap is refused.
                                  Without the flag `pad` is ignored on pools; the flag on any other op kind is an error.  Max of
                                  stored values is exact, so results are bit-exact in every dtype for NaN-free inputs.  NaN taps:
                                  the single-pool kernels (every dtype) and the float32 pyramid ignore them (fmaxf; a window whose
                                  taps are all NaN gives -inf from the former); the 16-bit pyramid compares with
                                  `a >= b ? a : b`, so whether a NaN survives depends on where it sits in the window -- the same
                                  as without the flag.  y3_capabilities() reports Y3_CAP_POOL_DARKNET                         */
#define Y3_F_SCORES_DARKNET 2048u /* Y3_OP_YOLO: Darknet's class scores instead of the reference's soft-max.  Score and class only, the
                                  box is untouched.  In float32, one rounding per operation:
                                    obj = 1 / (1 + expf(-t4)),  p_c = 1 / (1 + expf(-t_c))         (Darknet's logistic_activate)
                                    prob = p_best * obj,  cls = the first index c with p_c == max_c p_c
                                  (the arg-max on the computed p_c, not on the logits: distinct logits above ~17 all give 1.0f and
                                  the first wins).  16-bit networks compute the class terms with the hardware exp2, as they do the
                                  soft-max's.  With Y3_F_NEW_COORDS the inputs are probabilities already and that decode is Darknet's:
                                  the flag is accepted there and changes nothing, bit for bit.  On any other op kind it is an
                                  error.  y3_capabilities() reports Y3_CAP_SCORES_DARKNET                                    */
#define Y3_F_REORG_3D 4096u    /* Y3_OP_REORG: the [reorg3d] form (see Y3_OP_REORG); on any other op kind it is an error      */

/*
 * One unit of work.  POD, 8-byte aligned, zero-initialise unused fields.
 * Weight layouts (prepared on the host by yolov3/darknet.py:load_weights):
 *   igemm path  : d_weight[co][ (ky*ks + kx)*Cin + ci ]  row stride k_ld elements (zero padded),
 *                 rows padded with zeros up to a multiple of 128; dtype = op dtype
 *   small-Cin   : (Cin <= 4) d_weight as float32 [ (ky*ks+kx)*Cin + ci ][ co ] with row stride = cout_pad
 *   direct path : same as igemm layout
 * d_scale/d_bias: float32 per output channel (BN folded to y = conv*scale + bias; scale=1 for
 * convs with a bias and no BN), padded like the weight rows.
 */
typedef struct y3_op {
  int32_t kind;
  int32_t dtype;
  uint32_t flags;
  int32_t batch;
  int32_t in_h, in_w, in_c, in_ld;
  int32_t out_h, out_w, out_c, out_ld;
  int32_t ksize, stride, pad;     /* conv / maxpool / upsample factor in `stride`; pad: conv, and maxpool with Y3_F_POOL_DARKNET */
  int32_t res_ld;
  int32_t k_ld;                   /* weight row stride (elements)                  */
  int32_t cout_pad;               /* padded rows of weight / length of scale, bias */
  const void *d_in;
  void *d_out;
  const void *d_res;
  const void *d_weight;
  const float *d_scale;
  const float *d_bias;
  /* Y3_OP_YOLO: d_in is the float32 head tensor (B,h,w,ld) with channel = anchor*n_attr + attr.
   * Y3_OP_CONV: `groups` shares n_anchor's four bytes (only YOLO ops read n_anchor).  0 and 1 both mean an ordinary conv.
   * With groups > 1 the op still has in_c input and out_c output channels in all; output channel co belongs to group
   * g = co / (out_c / groups) and reads input channels [g * in_c / groups, (g + 1) * in_c / groups).  Weight layouts: see
   * y3_conv_path (answers 4 and 5).  y3_capabilities() reports Y3_CAP_GROUPED_CONV                                        */
  union {
    int32_t n_anchor;
    int32_t groups;
  };
  int32_t n_attr;
  float anchor_w[8], anchor_h[8]; /* pixels, already selected by `mask` (darknet.py:44) */
  int32_t row_offset, rows_total; /* this head's first row / total rows M of the concatenated output */
  float net_w, net_h;             /* cfg [net] width/height (darknet.py:395-399)          */
  float *d_bbox;                  /* (B, rows_total, 4) cx,cy in [0,1], w,h / net size     */
  float *d_prob;                  /* (B, rows_total)                                       */
  int64_t *d_cls;                 /* (B, rows_total)                                       */
  int32_t block_idx;              /* Darknet block this op implements (diagnostics)        */
  /* Y3_OP_YOLO: Darknet's [yolo] scale_x_y s, box centre = (sigmoid(t) * s - (s - 1) / 2 + cell) / grid; 0 means 1 (the
   * YOLOv3 decode, bit for bit).  Was `int32_t reserved` (always 0) before Y3_CAP_SCALE_X_Y.                          */
  float scale_x_y;
  /* ABI 6: the conv's weights in MFMA-fragment order (y3_conv_make_fragment_weights), y3_conv_fragment_weight_bytes() bytes,
   * for the layers the direct-weights strip kernel takes; shared by every plan of the network.  NULL: a plan that needs the
   * copy makes a private one (see the conventions above).                                                              */
  const void *d_weight_frag;
} y3_op;

typedef struct y3_plan y3_plan;

/*
 * y3_options.auto_mask: per-layer kernel choice of the MFMA convolutions, one bit per rule (profiles/ holds the A/B tables
 * behind every default).  Results do not depend on it: all MFMA conv kernels sum a layer in the same K order (channel chunk
 * outermost, filter tap innermost), so a layer's output is bit-identical whichever of them runs.
 */
#define Y3_AM_HALO_WIDE 0x0001u      /* halo-reuse kernel for 3x3 stride-1 layers (Cin, Cout >= 128) with rows of more than 64 px */
#define Y3_AM_IGEMM3_MID 0x0002u     /* wave-specialised implicit GEMM for such layers with rows of 33..64 px (if not HALO_MID)   */
#define Y3_AM_HALO_NARROW 0x0004u    /* halo-reuse kernel for rows of <= 32 px                                                     */
#define Y3_AM_IGEMM3_1X1_DEEP 0x0008u /* wave-specialised implicit GEMM for 1x1 layers with Cin >= 1024                            */
#define Y3_AM_HALO_MID 0x0010u       /* halo-reuse kernel for rows of 33..64 px                                                    */
#define Y3_AM_IGEMM3_NARROW 0x0020u  /* wave-specialised implicit GEMM for rows of <= 32 px (if not HALO_NARROW)                   */
#define Y3_AM_IGEMM3_1X1_BM64 0x0040u /* 64-pixel tiles of it for bf16 1x1 layers with Cin >= 256 (A/B only)                       */
#define Y3_AM_PATCH_WIDE 0x0080u     /* 2-D patch kernel (8 x 32 output tiles) for 3x3 stride-1 layers with rows wider than 128 px */
#define Y3_AM_HALO_TILE256 0x0200u   /* halo kernel with 256-pixel tiles only: the THROUGHPUT choice of callers that keep several  */
                                     /* batches in flight on their own streams (default: 192-pixel tiles where they shorten one forward) */
#define Y3_AM_NO_BN_SHRINK 0x0400u   /* A/B: implicit-GEMM channel tiles by Cout only (no narrower tiles on small grids)           */
#define Y3_AM_NO_SMALL_GRID 0x0800u  /* A/B: no small-grid / stride-2 rerouting (the round-1 selection)                            */
#define Y3_AM_NO_WRES 0x1000u        /* A/B: never the weights-resident persistent 1x1 kernel                                      */
#define Y3_AM_HALO_DW 0x4000u        /* direct-weights strip kernel (192 x 256 tiles, weight fragments straight from global memory) */
                                     /* for 3x3 layers whose tile count fills the chip better that way (round 5)                   */
#define Y3_AM_HALO_DW_ALWAYS 0x8000u /* tests / A-B: that kernel wherever it fits                                                  */
#define Y3_AM_1X1_DW 0x10000u        /* direct-weights 1x1 kernel (whole activation tile in LDS, weight fragments straight from global */
                                     /* memory) for the short-K bottleneck layers whose map x batch gives every CU one tile (round 6) */
#define Y3_AM_SMALL_DW 0x20000u       /* small-grid direct-weights kernel (48-pixel x 32..256-channel tiles, whole halo in LDS) for 1x1 and   */
                                     /* 3x3 layers whose map x batch fits the chip in ONE round of such tiles: one frame at a time (round 6)  */
#define Y3_AM_SMALL_DW_ALWAYS 0x40000u /* tests / A-B: that kernel wherever its shape constraints hold, whatever the grid                       */
#define Y3_AM_SMALL_DW_WIDE 0x80000u  /* ... and for grids a little over one round where it measured faster than what the layer ran on: 3x3 layers  */
                                     /* up to 1.5 rounds of its widest tiles; 1x1 layers with ONE channel tile per pixel tile (128+ channels) up   */
                                     /* to 8 rounds, after the weights-resident kernel has had its say (batches of 3-8; two layers at batch 16)   */
#define Y3_AM_WRES_ALWAYS 0x2000u    /* tests: that kernel on every layer it supports, whatever the map size                       */
#define Y3_AM_DEFAULT (Y3_AM_HALO_WIDE | Y3_AM_HALO_NARROW | Y3_AM_IGEMM3_1X1_DEEP | Y3_AM_HALO_MID | Y3_AM_PATCH_WIDE | Y3_AM_HALO_DW | Y3_AM_1X1_DW | Y3_AM_SMALL_DW | Y3_AM_SMALL_DW_WIDE)   /* 0xb409d */
#define Y3_AM_IGEMM_ONLY 0u          /* LDS-DMA implicit GEMM (igemm_version) everywhere                                           */

/*
 * Kernel-selection options of ONE plan (fixed when the plan is created).  y3_options_default() fills in the
 * library's defaults -- the measured-best choices, profiles/ -- as modified by y3_set_tuning().
 *   auto_mask        Y3_AM_* bits, default Y3_AM_DEFAULT
 *   unused0          (was halo_persistent: the persistent strip kernels measured slower twice and were removed,
 *                    profiles/r03b_persistent_halo_wsq_investigation.txt; ignored)
 *   igemm_version    1 register-staged, 2 LDS-DMA double-buffered [default], 3 wave-specialised
 *   igemm_ns         LDS stages of version 3 (3 or 4; less means 3);  igemm_bm  64 = 64-pixel tiles for version 3 (bf16)
 *   use_graph        1: y3_plan_run replays a captured hipGraph (one launch per forward) on non-default streams;
 *                    0 [default]: every kernel is launched individually (measured 1 % faster at batch 16)
 *   fuse_stem        1 [default]: conv pairs flagged Y3_F_FUSE_NEXT run as one kernel where one exists; 2: same, with the
 *                    phase-by-phase form of the fused stem kernel (same bits, slower: A/B and tests); 0: never fused
 *   fuse_head        1 [default]: detection-head conv + YOLO decode in one launch (16-bit networks), on the direct-weights 1x1 kernel
 *                    where the head conv has 256 / 512 / 1024 input channels (it reads the fragment-order copy of the weights:
 *                    y3_op.d_weight_frag or a private copy; 48-pixel tiles), else on the tiled kernel; 2: the tiled kernel only; 3 / 4:
 *                    the direct-weights kernel with 48- / 96-pixel tiles wherever the shape allows (same bits all four: A/B and tests);
 *                    0: two launches
 *   fuse_spp         1 [default]: three stride-1 max-pools (5 / 9 / 13) of one tensor in one launch, when all three pool by the
 *                    same rule (all with Y3_F_POOL_DARKNET and pad = ksize - 1, or none with it); 0: three launches, same bits
 *   decode_lanes     4 [default]: four lanes per box in the bf16 decode; 1: sequential class loop everywhere
 *   fuse_block       0 [default]: off.  1: a 1x1 conv (-> 128 channels) + the 3x3 conv that is its only reader (+ the
 *                    shortcut add) run as ONE kernel with the 128-channel tensor kept in LDS (csrc/conv_block.hip), where map
 *                    and batch give enough workgroups to fill the chip (yolov3@608: the 76^2 blocks from batch 12 on); 2:
 *                    wherever the kernel supports the pair (tests).  Same bits either way; measured level with the two
 *                    launches (profiles/r04_block_fused_AB.txt), which is why it is not the default.
 *                    3: the same pairs under the rule of 1 on the DIRECT-WEIGHTS form of the kernel (csrc/conv_block_dw.hip,
 *                    libyolov3_hip_block.so), which reads the fragment-order copies of both convs' weights: it takes a pair only
 *                    when both ops carry y3_op.d_weight_frag (y3_conv_fragment_weight_bytes answers by shape for such ops); a
 *                    pair without them runs as two launches -- no private copies for fused steps.  Same bits; 8 % faster
 *                    than the two launches at yolov3@608 batch 16 (profiles/block_dw_AB.txt): what yolov3.Pipeline asks for
 *                    when batches overlap.  4: the same kernel wherever it supports the pair (tests only).
 */
typedef struct y3_options {
  int32_t auto_mask, unused0, igemm_version, igemm_ns, igemm_bm;
  int32_t use_graph, fuse_stem, fuse_head, fuse_spp, decode_lanes;
  int32_t fuse_block;
  int32_t reserved[5];
} y3_options;

/* library / device ------------------------------------------------------------------- */
int y3_abi_version(void);
/* what this build computes beyond ABI 6 as first released (the version number and y3_op's size stay put: every addition
 * keeps zero-initialised callers working).  Callers check it before they rely on a feature, so that a stale library is
 * refused instead of running, say, mish as linear.                                                                   */
#define Y3_CAP_MISH 1u         /* Y3_F_MISH on conv ops                      */
#define Y3_CAP_SCALE_X_Y 2u    /* y3_op.scale_x_y on YOLO ops                */
#define Y3_CAP_LOGISTIC 4u     /* Y3_F_LOGISTIC on conv ops                  */
#define Y3_CAP_NEW_COORDS 8u   /* Y3_F_NEW_COORDS on YOLO ops                */
#define Y3_CAP_LETTERBOX 16u   /* y3_letterbox_geometry, y3_letterbox_u8, y3_detect_letterbox */
#define Y3_CAP_POOL_DARKNET 32u /* Y3_F_POOL_DARKNET and y3_op.pad on max-pool ops */
#define Y3_CAP_NMS_DARKNET 64u /* y3_detect_darknet, y3_nms_darknet and their workspace queries */
#define Y3_CAP_SCORES_DARKNET 128u /* Y3_F_SCORES_DARKNET on YOLO ops      */
#define Y3_CAP_MULTI_LABEL 256u /* y3_expand_labels and its workspace query   */
#define Y3_CAP_PREPROCESS_DARKNET 512u /* y3_preprocess_darknet_f32            */
#define Y3_CAP_REORG 1024u     /* Y3_OP_REORG and Y3_F_REORG_3D              */
#define Y3_CAP_LAUNCH_LOG 2048u /* y3_debug_launch_log_begin, y3_debug_launch_log_end */
#define Y3_CAP_PLAN_OP_DIMS 4096u /* y3_plan_op_dims and y3_set_tuning("device_cus", n) */
#define Y3_CAP_TILES 8192u     /* y3_tiles_u8, y3_detect_tiled and its workspace query */
#define Y3_CAP_GROUPED_CONV 16384u /* y3_op.groups on conv ops, y3_conv_path answers 4 and 5, y3_set_tuning("grouped_generic", v) */
#define Y3_CAP_ATTENTION 32768u /* Y3_OP_AVGPOOL, Y3_OP_SCALE_CHANNELS and Y3_OP_SAM */
#define Y3_CAP_TILE_MERGE 65536u /* y3_merge_tiled and its workspace query   */
uint32_t y3_capabilities(void);
const char *y3_last_error(void);
/* number of visible HIP devices whose arch is gfx950 (0 on a CPU-only machine) */
int y3_device_count(void);

/* plan executor: replaces the block loop of Darknet.forward (darknet.py:366-399) -------- */
/* copies `ops` (host array); `d_zero` = >= 256 bytes of zeroed device memory that outlives the plan */
int y3_plan_create(const y3_op *ops, int n_ops, const void *d_zero, y3_plan **out_plan);
/* same with explicit options (NULL = the current defaults); the plan keeps its own copy */
int y3_plan_create_ex(const y3_op *ops, int n_ops, const void *d_zero, const y3_options *options, y3_plan **out_plan);
void y3_options_default(y3_options *options);
void y3_plan_destroy(y3_plan *plan);
/* launches every op on `stream` (with the "use_graph" knob: from the second call on, on a non-default stream, as one
 * captured hipGraph per distinct d_input); `d_input` feeds ops flagged Y3_F_PLAN_INPUT */
int y3_plan_run(y3_plan *plan, const void *d_input, void *stream);
/* same, bracketing every op with HIP events; after the call ms_per_op[i] holds op i's device
 * time in milliseconds (synchronises the stream; for bench.py / profiling only)              */
int y3_plan_run_timed(y3_plan *plan, const void *d_input, void *stream, float *ms_per_op);
/* same run, but every kernel is launched with a start / stop event pair bound to its DISPATCH (hipExtLaunchKernel):
 * kernel_ms_per_op[i] is the device time of op i's kernel(s) from begin to end -- what rocprofv3's kernel trace reports --
 * without the dispatch / barrier-packet handling between two stream events that y3_plan_run_timed's figure includes
 * (~5 us per launch on an MI355X).  Synchronises the stream; for bench.py / profiling only.                       */
int y3_plan_run_profiled(y3_plan *plan, const void *d_input, void *stream, float *kernel_ms_per_op);
/* name of the kernel an op dispatches to, e.g. "conv_igemm_bf16_128x128" (static string)     */
const char *y3_plan_op_kernel(const y3_plan *plan, int op_index);
/* the launch an op's step recorded when the plan was created: out[0] workgroups, out[1] threads per workgroup, out[2] bytes of
 * dynamic LDS; three zeros for an op that an earlier step launches (a fused group's second op, the SPP pyramid's second and
 * third pool).  Tests and tools: the launchers launch exactly these.                                                   */
int y3_plan_op_dims(const y3_plan *plan, int op_index, int64_t out[3]);
/* algorithmic FLOPs (2*k*k*Cin*Cout*Hout*Wout*B for convs, divided by `groups` for a grouped one, else 0) and compulsory
 * bytes (a grouped conv's weights count k*k*(Cin/groups)*Cout elements)                                              */
double y3_plan_op_flops(const y3_plan *plan, int op_index);
double y3_plan_op_bytes(const y3_plan *plan, int op_index);

/* kernel family a Y3_OP_CONV op dispatches to: 0 = MFMA implicit GEMM (weights [cout_pad][k_ld] in
 * the op dtype), 1 = 3-channel stem (weights float32 [27][cout_pad]), 2 = direct fallback (same
 * layout as 0), 3 = MFMA stem for uint8 BGR frames -> bf16 (weights bf16 [32][32], k = ky*9 + kx*3 +
 * byte-channel, zero padded; scale/bias 32 floats); -1 if `op` is not a conv.  The host lays weights
 * out accordingly.
 * A conv with groups > 1 is asked about before anything else and gets one of two answers of its own:
 *   4 = grouped (csrc/conv_grouped.hip: conv_grouped_*): weights [cout_pad][k_ld] in the op dtype, row = output channel,
 *       k = (ky*ksize + kx) * (in_c / groups) + c with c the channel inside the group: layout 0 with the group's channel
 *       count.  k_ld >= ksize*ksize*(in_c / groups), cout_pad >= out_c; scale / bias have cout_pad entries.
 *   5 = depthwise (conv_dwise_*): groups == in_c == out_c with in_c, in_ld, out_ld (and res_ld) multiples of 8 and d_in, d_out,
 *       d_res, d_weight, d_scale, d_bias (those that are set) 16-byte aligned; a depthwise op off that grain is answered 4.  Weights
 *       [ksize*ksize][k_ld] in the op dtype, tap-major with the channel innermost; k_ld = cout_pad = c_pad =
 *       round_up(out_c, 8) (a larger multiple of 8 as k_ld is accepted); scale / bias have c_pad entries.
 * Both kernels take float32, bf16 and fp16, any ksize / stride / pad that give the op's output size, every activation
 * and Y3_F_RESIDUAL.  They sum a value in float32 from 0 in the order ky outermost, kx next, channel of the group
 * innermost, every product rounded before it is added (no fused multiply-add); taps outside the image add nothing.  So a
 * depthwise op gives the same bits on either -- for finite weights: the depthwise kernel adds the zero products of the columns
 * outside the image where the grouped kernel skips the tap, and 0 * inf is NaN (a damaged weights file).  Under y3_set_tuning("grouped_generic", 1) the answer is 4 for every grouped
 * op.  Plan creation refuses, with Y3_ERR_INVALID and the block's number: groups < 0; in_c or out_c no multiple of groups;
 * groups > 1 with Y3_F_IN_NCHW_F32, Y3_F_IN_NHWC_U8BGR, Y3_F_PLAN_INPUT or Y3_F_OUT_F32 (a grouped stem or head conv);
 * k_ld / cout_pad below the layout's.  No fused group takes a grouped op.                                              */
int y3_conv_path(const y3_op *op);

/* Fragment-order weights of the direct-weights strip kernel (csrc/conv_halo.hip: 1-KiB blocks of 16 output channels x 32
 * K-elements in the MFMA operand layout).  y3_conv_fragment_weight_bytes: size of the copy if a plan created with `options`
 * (NULL = the current defaults) runs `op` on that kernel, else 0 -- the host makes ONE copy per layer and device with
 * y3_conv_make_fragment_weights (reads op->d_weight, [cout_pad][k_ld]; stream-ordered on `stream`) and passes it to every
 * plan in y3_op.d_weight_frag.  No reference counterpart (a layout of the parameters darknet.py:415-476 loads).          */
size_t y3_conv_fragment_weight_bytes(const y3_op *op, const y3_options *options);
int y3_conv_make_fragment_weights(const y3_op *op, void *d_dst, void *stream);

/* A/B measurements only (tools/conv_bench.py, bench.py --tuning): changes ONE field of the process-wide DEFAULT
 * options by name ("auto_mask", "igemm_version", "igemm_ns", "igemm_bm", "use_graph", "fuse_stem",
 * "fuse_head", "fuse_spp", "decode_lanes", "fuse_block").  Plans created afterwards without explicit options pick it up; existing
 * plans keep the options they were created with.
 * One key is no option field: "device_cus".  0 [default] asks the device for its compute-unit count, as ever; 1 .. 4096 is the
 * count every chooser gets instead, for every device, until it is set back to 0 (any other value: Y3_ERR_INVALID).  The count
 * sizes persistent grids, picks tile shapes and moves ops between kernels, all at plan creation: a plan keeps what it was
 * created with.  It is how the tests make, on an unpartitioned MI355X, the plans that a DPX / QPX / CPX compute partition
 * (128 / 64 / 32 CUs) gets; a grid of 32 workgroups computes the same values on either.  Not a speed knob.
 * Another is "grouped_generic".  0 [default]: a depthwise conv on the 8-channel grain runs conv_dwise_*.  1: every grouped
 * conv runs conv_grouped_* and y3_conv_path answers 4 for it (other values: Y3_ERR_INVALID).  Process-wide like "device_cus",
 * because y3_conv_path has no options argument; the host must lay the weights out under the value the plan is created
 * under.  Same bits either way: tests and A/B runs.                                                                   */
int y3_set_tuning(const char *key, int value);

/* Launch log (tests and tools only; host code, the kernels are the same): between the two calls every kernel the CALLING
 * THREAD launches through this library is recorded by its code-object symbol name, the mangled name the `.name` field of the
 * AMDGPU metadata holds (e.g. _Z16conv_dw48_kernelIDF16bLi3ELi2ELi2ELi1EEv...), in launch order, one name per line.  A replayed
 * hipGraph (use_graph) launches nothing through the library and logs nothing.  y3_debug_launch_log_begin fails when the thread
 * has a log already.  y3_debug_launch_log_end copies the NUL-terminated text into `names` and ends the log; *needed (may be
 * NULL) receives the bytes the text takes, NUL included.  With names == NULL or capacity < *needed it returns Y3_ERR_INVALID
 * and the log stays open -- the size query -- so the caller asks, allocates and calls again.  A launch whose name the runtime
 * could not give is logged as "?" and makes the ending call return Y3_ERR_INVALID after it has copied the text.       */
int y3_debug_launch_log_begin(void);
int y3_debug_launch_log_end(char *names, size_t capacity, size_t *needed);

/* single op (unit tests): same dispatch as inside a plan */
int y3_op_run(const y3_op *op, const void *d_input, const void *d_zero, void *stream);

/* detection tail: replaces inference.py:342-366 (threshold, scale, int cast, cxywh_to_tlbr,
 * per-class non_max_suppression, gather) for a whole batch, on device ---------------------- */
size_t y3_detect_workspace_bytes(int batch, int rows);
/*
 * d_bbox (batch,rows,4) f32, d_prob (batch,rows) f32, d_cls (batch,rows) i64: Darknet.forward outputs.
 * d_orig_hw (batch,2) int32: original frame height,width (inference.py:351-352).
 * Outputs, capacity `rows` per frame, detections ordered by (class asc, score desc, row desc):
 *   d_det_count (batch) int32; d_det_tlbr (batch,rows,4) int64; d_det_prob (batch,rows) f32;
 *   d_det_cls (batch,rows) int64; d_det_row (batch,rows) int32 = row index into the `rows` predictions.
 */
int y3_detect(const float *d_bbox, const float *d_prob, const int64_t *d_cls, int batch, int rows,
              const int32_t *d_orig_hw, float prob_thresh, double iou_thresh, void *d_workspace,
              size_t workspace_bytes, int32_t *d_det_count, int64_t *d_det_tlbr, float *d_det_prob,
              int64_t *d_det_cls, int32_t *d_det_row, void *stream);

/* the same with Darknet's letterbox box correction (correct_yolo_boxes(..., letter=1)) for frames that went through
 * y3_letterbox_u8 into a (net_h, net_w) network.  Per frame, with {new_h, new_w} = the y3_letterbox_geometry of its
 * d_orig_hw entry (computed on the device), every candidate's relative box is corrected before the * orig_w / * orig_h
 * product:
 *   deltaw = (float)(net_w - new_w),  ratiow = (float)new_w / net_w                                  (float32)
 *   x' = (float)(((double)x - (double)deltaw / 2.0 / (double)net_w) / (double)ratiow),  w' = w * (1.0f / ratiow)
 * and likewise y, h with net_h, new_h.  The image is shifted by the INTEGER top / left while the boxes are corrected by
 * delta / 2, which may end in .5 -- Darknet's mismatch, kept.  A net-sized frame's correction is the identity: the output
 * then equals y3_detect's bit for bit.  net_h, net_w > 0.                                                           */
int y3_detect_letterbox(const float *d_bbox, const float *d_prob, const int64_t *d_cls, int batch, int rows,
                        const int32_t *d_orig_hw, float prob_thresh, double iou_thresh, void *d_workspace,
                        size_t workspace_bytes, int32_t *d_det_count, int64_t *d_det_tlbr, float *d_det_prob,
                        int64_t *d_det_cls, int32_t *d_det_row, int net_h, int net_w, void *stream);

/* the same for frames that were run as TILES: windows of the frame cut out at full resolution (y3_tiles_u8 below), each one
 * network input of its own.  Not in the reference.  d_bbox (batch * tiles, rows, 4), d_prob and d_cls (batch * tiles, rows) are
 * the forward outputs of frame b's tiles, contiguous: tiles b * tiles .. b * tiles + tiles - 1.  A frame's candidates are all rows
 * of all its tiles; row r of tile t is the combined row t * rows + r, which is what d_det_row reports.  d_geom is a DEVICE array
 * of batch * tiles y3_tile_geom, one per tile in the same order; with g the entry of its tile, a candidate (x, y, w, h) becomes
 *   cx = (int64)(x * g.sx) + g.ox,  cy = (int64)(y * g.sy) + g.oy,  bw = (int64)(w * g.sx),  bh = (int64)(h * g.sy)
 * (float32 products truncated toward zero; the offset is added after the truncation), corners = centre -/+ (size >> 1), and
 * from there on everything is y3_detect's on the union: >= prob_thresh, per-class suppression on the integer corners with +1
 * areas and strict >, order (class asc, score desc, combined row desc).  A window cut 1:1 at (y0, x0) of the frame carries
 * {net_w, net_h, x0, y0}; the whole frame stretched to the network carries {src_w, src_h, 0, 0}.  With tiles = 1 and
 * {orig_w, orig_h, 0, 0} the outputs equal y3_detect's bit for bit.  Outputs have capacity tiles * rows per frame:
 * d_det_count (batch); d_det_tlbr (batch, tiles * rows, 4); d_det_prob, d_det_cls, d_det_row (batch, tiles * rows).
 * tiles * rows must fit an int32.  The same kernel as y3_detect, one launch.  Darknet's suppression kinds, the letterbox
 * correction and multi-label virtual rows have no tiled form.  An object cut by a tile border yields partial boxes that the
 * suppression does not merge, unless y3_merge_tiled (below) runs after it: otherwise overlapping windows (and a stretched
 * overview for large objects) are the caller's guard.                                                                   */
typedef struct {
  float sx, sy;      /* pixels per unit of the tile's relative x / y */
  int32_t ox, oy;    /* the tile's origin in the frame, pixels        */
} y3_tile_geom;
size_t y3_detect_tiled_workspace_bytes(int batch, int tiles, int rows);
int y3_detect_tiled(const float *d_bbox, const float *d_prob, const int64_t *d_cls, int batch, int tiles, int rows,
                    const y3_tile_geom *d_geom, float prob_thresh, double iou_thresh, void *d_workspace, size_t workspace_bytes,
                    int32_t *d_det_count, int64_t *d_det_tlbr, float *d_det_prob, int64_t *d_det_cls, int32_t *d_det_row,
                    void *stream);

/* Seam merging, an opt-in second pass over the output of y3_detect_tiled (csrc/tile_merge.hip, libyolov3_hip_tilemerge.so;
 * y3_capabilities() reports Y3_CAP_TILE_MERGE).  Not in the reference.  y3_detect_tiled itself is unchanged: a caller that does
 * not call this function gets what it always got.  An object cut by a tile border comes out of y3_detect_tiled as partial boxes:
 * the IoU of a part with the whole, or of two parts, is small, so the suppression keeps them all.  This pass matches boxes of
 * DIFFERENT tiles by intersection over the smaller area (IoS), which is near 1 for a part against its whole, and merges the
 * matches into their union box.  Everything is integers plus one float64 division: there is no tolerance anywhere.
 *   Input: one frame's `count` detections in the canonical order (class ascending, score descending, combined row descending),
 *   each with int64 corners (x1, y1, x2, y2), a float32 score, an int64 class and an int32 combined row.  The tile of a
 *   detection is row / tile_rows; the overview is a tile like any other.
 *   Measures: w = x2 - x1 + 1, h = y2 - y1 + 1, area = w * h in int64 (the +1 pixel convention of y3_detect).  A box with w <= 0
 *   or h <= 0 is degenerate: it never matches, is never matched, and passes through unchanged.  For two non-degenerate boxes
 *   iw = min(ax2, bx2) - max(ax1, bx1) + 1 clamped at 0, ih likewise in y, inter = iw * ih, and
 *     a matches b  iff  (double)inter / (double)min(area_a, area_b) > thr          (true float64 division, strict comparison)
 *   Greedy pass, in the canonical order, classes independent: a detection that nothing has absorbed is a keeper.  Keeper i
 *   absorbs every later detection j that has i's class, is not absorbed yet, comes from a different tile than i, and whose
 *   ORIGINAL box i's ORIGINAL box matches.  The first keeper in order that matches a detection takes it; an absorbed detection
 *   absorbs nobody; matching never uses a grown box.
 *   The different-tile condition: within one tile the network saw both boxes in one view and the IoU suppression has already
 *   ruled -- a small box inside a larger one of its class in the same window is two objects; across tiles it is a part and a whole.
 *   Output: the keepers, in the input's order (so still canonical).  A keeper's box is the union of its own box and the original
 *   boxes of everything it absorbed (min of the x1 / y1, max of the x2 / y2); score, class and row are its own; members = 1 + the
 *   number of detections it absorbed.  Slots past the new count are not written.
 * thr = 1.0 never matches, and neither does anything when capacity == tile_rows (one tile): the output is then the input bit for bit,
 * all members 1.  The five inputs are y3_detect_tiled's outputs for `batch` frames of `capacity` (= tiles * rows) slots each and
 * are only read; tile_rows = rows, a divisor of capacity; thr is finite, 0 <= thr <= 1.  The outputs have the inputs' shapes, plus
 * d_out_members (batch, capacity) int32, which may be null; no output (nor the workspace) may overlap an input.  A frame whose count is 0
 * writes count 0 and nothing else; a count past `capacity` is read as `capacity`.  One launch of one 1024-thread workgroup per frame,
 * no host synchronisation; boxes may lie anywhere in int64 as long as their areas do (those within +-16000 take a 32-bit test
 * that decides the same).                                                                                                */
size_t y3_merge_tiled_workspace_bytes(int batch, int capacity);
int y3_merge_tiled(const int32_t *d_det_count, const int64_t *d_det_tlbr, const float *d_det_prob, const int64_t *d_det_cls,
                   const int32_t *d_det_row, int batch, int capacity, int tile_rows, double thr, void *d_workspace,
                   size_t workspace_bytes, int32_t *d_out_count, int64_t *d_out_tlbr, float *d_out_prob, int64_t *d_out_cls,
                   int32_t *d_out_row, int32_t *d_out_members, void *stream);

/* Darknet's suppression rule (src/box.c: box_iou, box_diou, box_diounms; do_nms_sort, diounms_sort) instead of the
 * reference's.  Not in the reference.  ONLY the decision which candidates survive changes: thresholding, candidate order
 * (class ascending, score descending, higher row first), "a suppressed box suppresses nobody", independent classes and
 * everything a kept detection carries are y3_detect's, so the detections are a subset of y3_detect's at iou_thresh = 1.0 with
 * identical rows.  The rule works on the float32 centre / size boxes (x, y, w, h) of d_bbox as the network emitted them --
 * with net_h, net_w > 0 on the letterbox-corrected values of y3_detect_letterbox, before the * orig_w / * orig_h product --
 * in float32, one rounding per operation, except pow:
 *   overlap(x1,w1,x2,w2) = min(x1 + w1/2, x2 + w2/2) - max(x1 - w1/2, x2 - w2/2)     min(p,q) = p < q ? p : q, max likewise
 *   I   = (ow < 0 || oh < 0) ? 0 : ow * oh                 ow, oh = overlap in x, in y
 *   U   = a.w*a.h + b.w*b.h - I
 *   iou = (I == 0 || U == 0) ? 0 : I / U
 *   cw  = max(a.x + a.w/2, b.x + b.w/2) - min(a.x - a.w/2, b.x - b.w/2)    ch likewise in y
 *   c   = cw*cw + ch*ch          d = (a.x-b.x)*(a.x-b.x) + (a.y-b.y)*(a.y-b.y)
 *   Y3_NMS_IOU     m = iou                                  (what a cfg without nms_kind gets)
 *   Y3_NMS_GREEDY  m = (c == 0) ? iou : iou - d / c         (nms_kind=greedynms)
 *   Y3_NMS_DIOU    m = (c == 0) ? iou : iou - (float)pow((double)(d / c), (double)beta_nms)    (nms_kind=diounms)
 *   a suppresses b  iff  m > (float)iou_thresh
 * NaN compares false everywhere: a NaN measure suppresses nothing.  beta_nms must be finite and > 0 (whatever the kind).
 * net_h = net_w = 0: the frames were not letterboxed.  Workspace: y3_detect_darknet_workspace_bytes (larger than
 * y3_detect's: it also holds the candidates' float boxes).                                                          */
#define Y3_NMS_IOU 0
#define Y3_NMS_GREEDY 1
#define Y3_NMS_DIOU 2
size_t y3_detect_darknet_workspace_bytes(int batch, int rows);
int y3_detect_darknet(const float *d_bbox, const float *d_prob, const int64_t *d_cls, int batch, int rows,
                      const int32_t *d_orig_hw, float prob_thresh, double iou_thresh, void *d_workspace,
                      size_t workspace_bytes, int32_t *d_det_count, int64_t *d_det_tlbr, float *d_det_prob,
                      int64_t *d_det_cls, int32_t *d_det_row, int net_h, int net_w, int nms_kind, float beta_nms,
                      void *stream);
/* the same rule on caller-provided boxes: d_xywh (n,4) float32 centre / size (16-byte aligned), d_prob (n) f32, d_cls (n)
 * int64 or NULL (class-agnostic); d_keep (n) int64 receives the kept indices ordered by (class asc, score desc, index
 * desc); d_keep_count (1) int32.                                                                                     */
size_t y3_nms_darknet_workspace_bytes(int n);
int y3_nms_darknet(const float *d_xywh, const float *d_prob, const int64_t *d_cls, int n, float thresh, int nms_kind,
                   float beta_nms, void *d_workspace, size_t workspace_bytes, int64_t *d_keep, int32_t *d_keep_count,
                   void *stream);

/* Darknet's multi-label candidates (get_yolo_detections): every class of a box whose score passes the threshold becomes a
 * candidate of its own, where Darknet.forward's outputs carry the arg-max class only.  Not in the reference.
 * A y3_head_view is one detection head's float32 conv output (B, h, w, ld), channel = anchor * n_attr + attr, exactly what the
 * head's Y3_OP_YOLO op reads; prediction row = row_offset + anchor * h * w + y * w + x as in the decode.  new_coords != 0: the
 * stored values are probabilities already (a head decoded with Y3_F_NEW_COORDS) and are used as they are.  `heads` is a HOST
 * array (1..8 views whose row ranges lie inside [0, rows_total) and do not overlap); it travels as kernel arguments, so it may be
 * reused as soon as the call returns.  Per frame f and row, in float32 with one rounding per operation (the sequential form of
 * Y3_F_SCORES_DARKNET):
 *   obj = 1 / (1 + expf(-t4));   if obj > thresh:   for every class c:   p_c = 1 / (1 + expf(-t_c)),  s_c = obj * p_c;
 *                                                                        if s_c > thresh: emit label (row, c, s_c)
 * Both comparisons are strict and a NaN compares false.  Labels are written as VIRTUAL ROWS in ascending (row, c) order -- the
 * order does not depend on scheduling --:
 *   d_vbbox (batch, cap, 4) f32 = d_bbox[f, row] bit for bit;  d_vprob (batch, cap) f32 = s_c;  d_vcls (batch, cap) i64 = c;
 *   d_vrow (batch, cap) i32 = row;  slots k >= count: a box of zeros, vprob -1, vcls 0, vrow -1.
 * d_vcount (batch) i32 is the TRUE label count of the frame even when it exceeds `cap`; only the first `cap` labels in that
 * order are then written.  d_bbox (batch, rows_total, 4) f32 is the decode's output; it and d_vbbox are 16-byte aligned.
 * thresh must be finite and >= 0, cap >= 1.  The virtual rows are what y3_detect / y3_detect_letterbox / y3_detect_darknet
 * take as (d_bbox, d_prob, d_cls) with rows = cap and the same prob_thresh: every label is > thresh, so their >= keeps all of
 * them and drops the padding, and their canonical order (class ascending, score descending, higher row first) holds on the
 * real rows as well, because virtual rows ascend with them.  d_det_row then indexes virtual rows: map it through d_vrow.
 * Two launches (count, then place and write); allocates nothing and never synchronises.  Workspace:
 * y3_expand_labels_workspace_bytes (one counter per 64 rows and frame).                                              */
typedef struct {
  const float *d_head;
  int32_t h, w, ld, n_anchor, n_attr, row_offset, new_coords;
} y3_head_view;
size_t y3_expand_labels_workspace_bytes(int batch, int rows_total, int cap);
int y3_expand_labels(const y3_head_view *heads, int n_heads, const float *d_bbox, int batch, int rows_total, float thresh,
                     int cap, void *d_ws, size_t ws_bytes, float *d_vbbox, float *d_vprob, int64_t *d_vcls, int32_t *d_vrow,
                     int32_t *d_vcount, void *stream);

/* non_max_suppression (inference.py:161-266) on caller-provided integer boxes -------------- */
size_t y3_nms_workspace_bytes(int n);
/*
 * d_tlbr (n,4) int64, d_prob (n) f32, d_cls (n) int64 or NULL (class-agnostic).
 * d_keep (n) int64 receives the kept indices ordered by (class asc, score desc, index desc);
 * d_keep_count (1) int32.
 */
int y3_nms(const int64_t *d_tlbr, const float *d_prob, const int64_t *d_cls, int n, double iou_thresh,
           void *d_workspace, size_t workspace_bytes, int64_t *d_keep, int32_t *d_keep_count,
           void *stream);

/* the same on FLOATING-POINT boxes: the reference's non_max_suppression takes any numeric dtype (inference.py:161-217;
 * its own inference() only passes integers) and numpy then computes areas, intersections, IoU and the comparison with the
 * threshold in the array's dtype.  d_tlbr (n,4) float32 (box_dtype Y3_F32) or float64 (Y3_F64), d_prob (n) float64
 * (exact for float32 / float64 scores), d_cls (n) int64 or NULL; outputs and order as y3_nms. */
size_t y3_nms_float_workspace_bytes(int n);
int y3_nms_float(const void *d_tlbr, int box_dtype, const double *d_prob, const int64_t *d_cls, int n, double iou_thresh,
                 void *d_workspace, size_t workspace_bytes, int64_t *d_keep, int32_t *d_keep_count, void *stream);

/* cxywh_to_tlbr (inference.py:269-283) on int64 rows of `cols` >= 4 columns ---------------- */
int y3_cxywh_to_tlbr(const int64_t *d_xywh, int64_t *d_tlbr, int n, int cols, void *stream);
/* ... and on float32 / float64 rows (dtype Y3_F32 / Y3_F64): tl = c - floor(wh / 2), br = c + floor(wh / 2), numpy's `//` */
int y3_cxywh_to_tlbr_float(const void *d_xywh, void *d_tlbr, int n, int cols, int dtype, void *stream);

/* frame resize on device (replaces the host cv2.resize of inference.py:320-326): uint8
 * (src_h,src_w,3) -> (dst_h,dst_w,3) with OpenCV's 8-bit INTER_LINEAR arithmetic: per channel
 *   top = S[ylo][xlo]*ax0 + S[ylo][xhi]*ax1,  bot = the same on row yhi   (int, 11-bit coefficients)
 *   out = (((ay0 * (top >> 4)) >> 16) + ((ay1 * (bot >> 4)) >> 16) + 2) >> 2
 * d_ytab (dst_h,4) / d_xtab (dst_w,4) int32 rows = {lo index, hi index, weight_lo, weight_hi}: OpenCV's yofs / ibeta
 * and xofs / ialpha tables, computed on the host (yolov3/preprocess.py:axis_table). */
int y3_resize_bilinear_u8(const uint8_t *d_src, int src_h, int src_w, uint8_t *d_dst, int dst_h, int dst_w,
                          const int32_t *d_ytab, const int32_t *d_xtab, void *stream);

/* Darknet letterboxing (letterbox_image): the frame keeps its aspect ratio inside the network input and the rest is
 * filled.  Not in the reference, which stretches every frame (cv2.resize).
 * y3_letterbox_geometry: out = {new_h, new_w, top, left} of a (src_h, src_w) frame in a (net_h, net_w) network:
 *   if (float)net_w / src_w < (float)net_h / src_h:  new_w = net_w, new_h = src_h * net_w / src_w   (int64, truncated)
 *   else:                                             new_h = net_h, new_w = src_w * net_h / src_h
 *   new_h, new_w clamped to >= 1;  top = (net_h - new_h) / 2,  left = (net_w - new_w) / 2.
 * Host function: the device side of y3_letterbox_u8 / y3_detect_letterbox uses the same definition.             */
int y3_letterbox_geometry(int src_h, int src_w, int net_h, int net_w, int32_t out[4]);
/* One frame of a letterboxed batch: d_src uint8 (src_h, src_w, 3) on the device; d_ytab (new_h, 4) / d_xtab (new_w, 4)
 * the y3_resize_bilinear_u8 tap tables of a (src_h, src_w) -> (new_h, new_w) resize, {new_h, new_w} from
 * y3_letterbox_geometry (the kernel trusts their indices: tables of another size read out of bounds).            */
typedef struct {
  const uint8_t *d_src;
  int32_t src_h, src_w;
  const int32_t *d_ytab, *d_xtab;
} y3_letterbox_frame;
/* d_dst (batch, net_h, net_w, 3) uint8: frame i resized to (new_h, new_w) with y3_resize_bilinear_u8's arithmetic and
 * pasted at (top, left) on a canvas of the byte `fill` (0..255; Darknet fills with 0.5 in float, which a uint8 frame
 * read as v / 255 cannot hold -- 128 is the usual choice).  `frames` is a HOST array of `batch` descriptors: they travel
 * as kernel arguments (a fixed number per launch, several launches on `stream` for bigger batches), so the array may
 * be reused as soon as the call returns.  Frames of different sizes share one call.                              */
int y3_letterbox_u8(const y3_letterbox_frame *frames, int batch, uint8_t *d_dst, int net_h, int net_w, int fill,
                    void *stream);

/* Tiles: net-sized windows of larger frames, cut out 1:1 on the device.  Not in the reference.  d_dst (n_tiles, net_h, net_w, 3)
 * uint8: pixel (y, x) of tile i is pixel (y0 + y, x0 + x) of its frame d_src (src_h, src_w, 3) where that lies inside the frame,
 * else the byte `fill` (0..255).  0 <= y0 < src_h and 0 <= x0 < src_w.  Tiles of different frames may share a call.  `tiles` is
 * a HOST array: the descriptors travel as kernel arguments (32 per launch, several launches on `stream` for more), so the array
 * may be reused as soon as the call returns.  The kernel of y3_letterbox_u8, which copies where a frame has no tap tables.  */
typedef struct {
  const uint8_t *d_src;
  int32_t src_h, src_w, y0, x0;
} y3_tile;
int y3_tiles_u8(const y3_tile *tiles, int n_tiles, uint8_t *d_dst, int net_h, int net_w, int fill, void *stream);

/* Darknet's own preprocessing (load_image -> letterbox_image / resize_image): uint8 BGR frames of any size -> the float32
 * network input, bit for bit what `darknet detector test` / `map` feed the network.  Not in the reference, which resizes the
 * 8-bit frame (cv2.resize) and divides by 255 afterwards; y3_letterbox_u8 above differs from Darknet in the resize arithmetic
 * and in the pad value (a byte), this entry point in neither.  All arithmetic is float32, one rounding per operation (no fused
 * multiply-add).  Per frame (h, w) and channel, with p(r, c) = (float)byte / 255.0f of the frame's pixel (equal to Darknet's
 * (float)(byte / 255.) for every byte):
 *   target (H, W) = {new_h, new_w} of y3_letterbox_geometry when `letterbox`, else (net_h, net_w)   (no dsize quirk here)
 *   (h, w) == (H, W): out = p.   Otherwise   w_scale = (float)(w - 1) / (float)(W - 1),  h_scale likewise, and
 *   part(r, c) = p(r, w - 1)                                        if c == W - 1 or w == 1, else
 *              = (1 - dx) * p(r, ix) + dx * p(r, ix + 1)            sx = (float)c * w_scale, ix = (int)sx, dx = sx - (float)ix
 *   out(r, c)  = (1 - dy) * part(iy, c)  [+ dy * part(iy + 1, c)  unless r == H - 1 or h == 1]
 *                                                                   sy = (float)r * h_scale, iy = (int)sy, dy = sy - (float)iy
 * dy is NOT forced to 0 on the last row: where (H - 1) * h_scale rounds to just below h - 1, that row is (1 - dy) * part(h - 2)
 * with dy just below 1 -- Darknet's quirk, kept.  An axis with h == 1 (w == 1) takes scale 0 (Darknet's 0 / 0 for 1 -> 1 is
 * never used for a pixel that matters).  A target of ONE row / column from a longer source divides by zero in Darknet and is
 * refused here (Y3_ERR_INVALID) -- with `letterbox` that is a frame more than net-size times longer than wide, or the reverse.
 * d_dst (batch, 3, net_h, net_w) float32, planar R, G, B from the BGR frame; with `letterbox` the canvas is 0.5f and the resized
 * frame lies at (top, left); 4-byte aligned (16-byte alignment and net_w % 4 == 0 give 16-byte stores).  `frames` is a HOST
 * array of `batch` descriptors, d_src uint8 (src_h, src_w, 3) on the device: they travel as kernel arguments (64 per launch,
 * so one launch for any usual batch), and the array may be reused as soon as the call returns.  Frames of different sizes share
 * one call.  All sizes must be below 2^24.  Darknet.forward (Y3_F_IN_NCHW_F32) takes d_dst as it is.                       */
typedef struct {
  const uint8_t *d_src;
  int32_t src_h, src_w;
} y3_darknet_frame;
int y3_preprocess_darknet_f32(const y3_darknet_frame *frames, int batch, float *d_dst, int net_h, int net_w, int letterbox,
                              void *stream);

/* frames in / detections out without a copy engine: what yolov3/pipeline.py (the loop bench.py times and detect_in_frames
 * runs) uses in place of the `.to(device)` / `.cpu()` transfers around Darknet.forward (inference.py:335, :338-340).  A small
 * grid of `blocks` workgroups (<= 0: 32) moves `nbytes` bytes with 16-byte accesses.  `src` or `dst` may be PINNED (registered)
 * host memory, which the GPU addresses directly over PCIe; both must be 16-byte aligned, and a pointer the runtime does not
 * know (pageable host memory) is rejected with Y3_ERR_INVALID.  Unlike hipMemcpyAsync it needs no copy-engine hand-over on
 * the stream, so batches in flight on other streams keep the chip (measured: profiles/r03c_pcie_inclusive.txt). */
int y3_copy_bytes(const void *src, void *dst, size_t nbytes, int blocks, void *stream);

/* padded fixed-size detection records for the multi-GPU all-gather (no reference counterpart:
 * the reference is single device).  Record = 8 x int32: x1,y1,x2,y2 (int64 corners saturated to int32), score bits, class, row, and the
 * frame's TRUE detection count (0 in padding records: the field doubles as the valid flag; a count
 * above kmax means the frame was truncated to its kmax best-ordered detections).
 * d_records (batch, kmax, 8) int32; d_rec_count (batch) int32 also receives the true counts, may be NULL. */
int y3_pack_records(const int32_t *d_det_count, const int64_t *d_det_tlbr, const float *d_det_prob,
                    const int64_t *d_det_cls, const int32_t *d_det_row, int batch, int rows, int kmax,
                    int32_t *d_records, int32_t *d_rec_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLOV3_HIP_H */
