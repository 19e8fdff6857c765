// C-ABI glue: error string, device query, op dispatch and the plan executor that replaces the
// block loop of Darknet.forward (/root/reference/yolov3/darknet.py:366-399).
#include <stdarg.h>
#include <string.h>

#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "common.h"

static_assert(sizeof(y3_op) == 248, "y3_op layout is part of the ABI (ctypes mirror in yolov3/_hip.py)");

namespace {
thread_local char g_err[512] = "";
}

// Default options (y3_options_default / y3_set_tuning); the auto_mask bits are named in include/yolov3_hip.h (Y3_AM_*).
static y3_options g_y3_defaults = {/*auto_mask*/ (int32_t)Y3_AM_DEFAULT, /*unused0*/ 0, /*igemm_version*/ 2, /*igemm_ns*/ 2,
                                   /*igemm_bm*/ 0, /*use_graph*/ 0, /*fuse_stem*/ 1, /*fuse_head*/ 1, /*fuse_spp*/ 1,
                                   /*decode_lanes*/ 4, /*fuse_block*/ 0, {0, 0, 0, 0, 0}};
static thread_local Y3LaunchHooks tl_y3_hooks = {nullptr, nullptr};
Y3LaunchHooks *y3_launch_hooks() { return &tl_y3_hooks; }
// The launch log of one thread: newline-separated symbol names in launch order.  A launch whose name the runtime cannot
// give is recorded as "?" and makes y3_debug_launch_log_end fail: a census must never miss a kernel quietly.
struct Y3LaunchLog {
  std::string names;
  bool unnamed = false;
};
void y3_launch_log_append(Y3LaunchLog *log, const void *host_function, hipStream_t stream) {
  const char *name = hipKernelNameRefByPtr(host_function, stream);
  if (!name || !*name) {
    hipFunction_t f = nullptr;
    if (hipGetFuncBySymbol(&f, host_function) == hipSuccess && f) name = hipKernelNameRef(f);
    else (void)hipGetLastError();
  }
  if (!name || !*name) {
    name = "?";
    log->unnamed = true;
  }
  log->names += name;
  log->names += '\n';
}
// y3_set_tuning("debug", v): exists in DIAGNOSTIC builds only (`make variant FLAGS=-DY3_DEBUG_KEY ...`, `make stamps`); the product
// library rejects the key, so a benchmark line can never come from kernels that skip work
#if defined(Y3_DEBUG_KEY) || defined(Y3_STAMPS)
#define Y3_HAS_DEBUG_KEY 1
static int g_y3_debug = 0;
int y3_debug_flags() { return g_y3_debug; }
#else
int y3_debug_flags() { return 0; }
#endif

// y3_set_tuning("device_cus", n): 0 asks the device; 1 .. 4096 is the count every chooser gets for every device (the plans of a
// compute partition of 128, 64 or 32 CUs, made and run on an unpartitioned device).  Read here and nowhere else.
static std::atomic<int> g_y3_device_cus{0};
// y3_set_tuning("grouped_generic", v): 1 sends every grouped conv to conv_grouped_* (y3_conv_path answers 4); process-wide,
// because y3_conv_path has no options to read it from.  Read by conv_path and nowhere else.
static std::atomic<int> g_y3_grouped_generic{0};
int y3_grouped_generic() { return g_y3_grouped_generic.load(std::memory_order_relaxed); }
// CU count of the current device (256 on an MI355X; 256 as well when no device is visible: dry runs on a CPU box)
int y3_device_cus() {
  const int forced = g_y3_device_cus.load(std::memory_order_relaxed);
  if (forced > 0) return forced;
  static std::atomic<int> cus[32];                 // (zero-initialised; concurrent first calls store the same value)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) { (void)hipGetLastError(); return 256; }
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
void y3_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

struct y3_plan {
  std::vector<y3_op> ops;
  std::vector<y3_step> steps;   // per op: what it launches, decided at creation (fuse into_prev: launched by an earlier step)
  std::vector<char> frag_own;   // per op: the plan made (and frees) steps[i].frag_w; callers of ABI 6 pass a shared copy in the op
  const void *d_zero;
  std::vector<hipEvent_t> events;
  std::vector<hipEvent_t> kstart, kstop;   // y3_plan_run_profiled: event pairs bound to the dispatches (two per op)
  // hipGraph replay (one graph launch per forward instead of ~80 kernel launches): executable graphs keyed by the
  // input pointer they were captured with; the first run of a plan is always eager (one-time function attributes)
  struct GraphEntry { const void *input; hipGraphExec_t exec; };
  std::vector<GraphEntry> graphs;
  bool warmed = false, graph_ok = true;
  y3_options opt;           // fixed at creation
};

namespace {

bool y3_is_attention(const y3_op &op) { return op.kind == Y3_OP_AVGPOOL || op.kind == Y3_OP_SCALE_CHANNELS || op.kind == Y3_OP_SAM; }

// 0 = MFMA implicit GEMM, 1 = 3-channel stem kernel (VALU), 2 = direct fallback, 3 = MFMA stem (uint8 -> bf16),
// 4 = grouped, 5 = depthwise (a grouped op is asked about first: no other family's chooser ever sees one)
int conv_path(const y3_op &op) {
  if (op.groups > 1) return !y3_grouped_generic() && y3_conv_dwise_fits(op) ? 5 : 4;
  const bool net_input = op.flags & (Y3_F_IN_NCHW_F32 | Y3_F_IN_NHWC_U8BGR);
  if (y3_conv_stem_mfma_supported(op)) return 3;
  if (net_input && op.in_c == 3 && op.ksize == 3 && !(op.flags & Y3_F_RESIDUAL)) return 1;
  if (!net_input && y3_conv_igemm_supported(op)) return 0;
  return 2;
}

// The conv chooser: what a conv op runs under options `o`.  The rules are asked in this order and are not independent (the
// SMALL_DW_WIDE 1x1 rule, for one, is asked only after the weights-resident kernel's).
int choose_conv(const y3_op &op, const y3_options &o, y3_step &st) {
  const uint32_t acts = op.flags & (Y3_F_LEAKY | Y3_F_MISH | Y3_F_LOGISTIC);
  Y3_REQUIRE((acts & (acts - 1)) == 0, "conv block %d: Y3_F_LEAKY, Y3_F_MISH and Y3_F_LOGISTIC are exclusive", op.block_idx);
  Y3_REQUIRE(op.out_h == (op.in_h + 2 * op.pad - op.ksize) / op.stride + 1 &&
                 op.out_w == (op.in_w + 2 * op.pad - op.ksize) / op.stride + 1,
             "conv block %d: output size mismatch", op.block_idx);
  switch (conv_path(op)) {
    case 1: return y3_choose_conv_small(op, st);
    case 2: return y3_choose_conv_direct(op, st);
    case 3: return y3_choose_conv_stem_mfma(op, st);
    case 4: return y3_choose_conv_grouped(op, st);
    case 5: return y3_choose_conv_dwise(op, st);
    default: break;
  }
  const unsigned am = (unsigned)o.auto_mask;
  if (!am) return y3_choose_conv_igemm(op, o, st);
  const int w = op.in_w;
  const bool k3 = op.ksize == 3 && op.stride == 1 && op.in_c >= 128 && op.out_c >= 128 && !(op.flags & Y3_F_OUT_F32);
  const bool halo_ok = k3 && y3_conv_halo_ws_fits(op);
  bool want_halo = false, want_ws = false;
  if (k3 && w > 64) want_halo = am & Y3_AM_HALO_WIDE;
  else if (k3 && w > 32) { want_halo = am & Y3_AM_HALO_MID; want_ws = am & Y3_AM_IGEMM3_MID; }
  else if (k3) { want_halo = am & Y3_AM_HALO_NARROW; want_ws = am & Y3_AM_IGEMM3_NARROW; }
  else if (op.ksize == 1 && op.in_c >= 1024 && op.out_c >= 128 && !(op.flags & Y3_F_OUT_F32))
    // (not below 64 tiles of 128 x 128: yolov3-tiny's 1024 -> 256 at 13^2 x 8 frames is 22 of them; the LDS-DMA
    // version with narrower channel tiles has four times the workgroups)
    want_ws = (am & Y3_AM_IGEMM3_1X1_DEEP) &&
              ((am & Y3_AM_NO_SMALL_GRID) || (long long)y3_ceil_div(op.batch * op.out_h * op.out_w, 128) * y3_ceil_div(op.out_c, 128) >= y3_device_cus() / 4);
  if ((am & Y3_AM_1X1_DW) && y3_conv1x1_dw_pays(op)) return y3_choose_conv1x1_dw(op, st);
  // small grids (one frame at a time, small batches): 48-pixel tiles that fill the chip in one round (conv_dw48.hip)
  const bool small_dw = (am & (Y3_AM_SMALL_DW | Y3_AM_SMALL_DW_ALWAYS)) && !(am & Y3_AM_NO_SMALL_GRID);
  if (small_dw && (y3_conv_dw48_fits(op, o) || (op.ksize == 3 && y3_conv_dw48_fits_wide(op, o)))) return y3_choose_conv_dw48(op, o, st);
  if (!(am & Y3_AM_NO_WRES) && y3_conv1x1_wres_supported(op) && ((am & Y3_AM_WRES_ALWAYS) || y3_conv1x1_wres_pays(op)))
    return y3_choose_conv1x1_wres(op, st);
  // 1x1 layers on grids of a few rounds, where the weights-resident kernel does not pay
  if (small_dw && op.ksize == 1 && y3_conv_dw48_fits_wide(op, o)) return y3_choose_conv_dw48(op, o, st);
  if ((am & Y3_AM_IGEMM3_1X1_BM64) && op.ksize == 1 && op.in_c >= 256 && op.out_c >= 128 && !(op.flags & Y3_F_OUT_F32) &&
      y3_is16(op.dtype))
    return y3_choose_conv_igemm(op, o, st, 3, 3, 64);
  if ((am & Y3_AM_PATCH_WIDE) && op.ksize == 3 && op.stride == 1 && w > 128 && op.out_c >= 128 && y3_conv_patch_fits(op))
    return y3_choose_conv_patch(op, st);
  // Small grids (small maps x small batches): a halo tile is 192+ pixels x 128 channels, and below ~3/4 of a
  // tile per CU most of the chip idles through its long K loop; the 128 x 128 implicit GEMMs have more, shorter
  // workgroups.  tools/conv_bench.py at batch 1 / 4 / 8 (profiles/r02f_convbench_small_batches.txt): 512 -> 1024
  // at 19^2 x 8 frames (128 tiles) 615 TFLOP/s on the halo kernel, 722 on the wave-specialised implicit GEMM;
  // in float32 (yolov3-tiny's 13^2 layers at batch 8) 66 against 93 on the LDS-DMA implicit GEMM.
  // (Which kernel runs changes speed only: every MFMA conv kernel sums in the same K order.)
  const long long halo_tiles = (long long)y3_ceil_div(op.batch * op.in_h * op.in_w, 192) * (op.out_c / 128);
  const bool small_grid = !(am & Y3_AM_NO_SMALL_GRID) && k3 && halo_tiles < (3 * y3_device_cus()) / 4;
  // direct-weights strip kernel (192 x 256 tiles) where its tile count fills the chip better (csrc/conv_halo.hip)
  if (k3 && !small_grid && halo_ok && (((am & Y3_AM_HALO_DW) && y3_conv_halo_dw_pays(op, o)) ||
                                       ((am & Y3_AM_HALO_DW_ALWAYS) && y3_conv_halo_dw_fits(op))))
    return y3_choose_conv_halo_dw(op, st);
  if (small_grid && y3_is16(op.dtype)) return y3_choose_conv_igemm(op, o, st, 3, 3);
  if (want_halo && halo_ok && !small_grid) return y3_choose_conv_halo(op, o, st);
  if (want_ws) return y3_choose_conv_igemm(op, o, st, 3, 3);
  // 3x3 stride-2 layer with 256 input channels (76^2 -> 38^2): 865 against 762 TFLOP/s on the wave-specialised
  // implicit GEMM at batch 16; the other stride-2 layers measured faster on the LDS-DMA version
  // (64 input channels -- 304^2 -> 152^2 -- at one or two frames: 9.6 against 12.3 us at one frame, level at four, 109 against
  // 97 at sixteen: profiles/r06_conv_dw48.txt)
  if (!(am & Y3_AM_NO_SMALL_GRID) && op.ksize == 3 && op.stride == 2 && op.out_c >= 128 && y3_is16(op.dtype) && !(op.flags & Y3_F_OUT_F32) &&
      ((op.in_c == 256 && (long long)op.batch * op.out_h * op.out_w >= 16384) ||
       (op.in_c == 64 && (long long)op.batch * op.out_h * op.out_w <= 49152)))
    return y3_choose_conv_igemm(op, o, st, 3, 3);
  return y3_choose_conv_igemm(op, o, st);
}

// flags that belong to one op kind only (checked for every op of a plan, the ones a fused step absorbs included)
int check_flags(const y3_op &op) {
  Y3_REQUIRE(!(op.flags & Y3_F_POOL_DARKNET) || op.kind == Y3_OP_MAXPOOL,
             "op for block %d: Y3_F_POOL_DARKNET on an op of kind %d (max-pool ops only)", op.block_idx, op.kind);
  Y3_REQUIRE(!(op.flags & Y3_F_SCORES_DARKNET) || op.kind == Y3_OP_YOLO,
             "op for block %d: Y3_F_SCORES_DARKNET on an op of kind %d (YOLO ops only)", op.block_idx, op.kind);
  Y3_REQUIRE(!(op.flags & Y3_F_REORG_3D) || op.kind == Y3_OP_REORG,
             "op for block %d: Y3_F_REORG_3D on an op of kind %d (reorg ops only)", op.block_idx, op.kind);
  // the attention ops take no flag: none of the conv-only ones (activations, residual, float32 store, network input, fusion
  // hint) and none of the pool-only ones
  if (y3_is_attention(op))
    Y3_REQUIRE(op.flags == 0, "op for block %d: flags 0x%x on an attention op of kind %d (avgpool, scale_channels and sam ops take none)",
               op.block_idx, op.flags, op.kind);
  return Y3_OK;
}

// y3_op.groups of a conv op (it shares its bytes with n_anchor, which only YOLO ops read): checked for every op of a plan
// before any chooser sees it
int check_groups(const y3_op &op) {
  if (op.kind != Y3_OP_CONV) return Y3_OK;
  const int g = op.groups;
  Y3_REQUIRE(g >= 0, "conv block %d: groups=%d", op.block_idx, g);
  if (g <= 1) return Y3_OK;
  Y3_REQUIRE(op.in_c % g == 0 && op.out_c % g == 0, "conv block %d: groups=%d does not divide %d input and %d output channels",
             op.block_idx, g, op.in_c, op.out_c);
  Y3_REQUIRE(!(op.flags & (Y3_F_IN_NCHW_F32 | Y3_F_IN_NHWC_U8BGR | Y3_F_PLAN_INPUT)),
             "conv block %d: a grouped conv (groups=%d) cannot read the network input", op.block_idx, g);
  Y3_REQUIRE(!(op.flags & Y3_F_OUT_F32), "conv block %d: a grouped conv (groups=%d) cannot store float32 from 16-bit storage (a detection-head conv)",
             op.block_idx, g);
  if (conv_path(op) == 5)
    Y3_REQUIRE(op.k_ld >= (op.out_c + 7) / 8 * 8 && op.cout_pad >= (op.out_c + 7) / 8 * 8,
               "conv block %d: depthwise weights [%d][c_pad] need k_ld and cout_pad >= %d (k_ld %d, cout_pad %d)", op.block_idx,
               op.ksize * op.ksize, (op.out_c + 7) / 8 * 8, op.k_ld, op.cout_pad);
  else
    Y3_REQUIRE((long long)op.k_ld >= (long long)op.ksize * op.ksize * (op.in_c / g) && op.cout_pad >= op.out_c,
               "conv block %d: grouped weights need k_ld >= %lld and cout_pad >= %d (k_ld %d, cout_pad %d)", op.block_idx,
               (long long)op.ksize * op.ksize * (op.in_c / g), op.out_c, op.k_ld, op.cout_pad);
  return Y3_OK;
}

// The size limits of every op kind (checked for every op of a plan, the ones a fused step absorbs included, before any chooser
// sees it).  Byte addresses are 64-bit in every kernel, but the tiled kernels keep the PIXEL index of a tile in an int or a
// uint32_t (`m = m0 + ...`, the magic-number divisions by __umulhi: common.h y3_fast_div, exact below 2^31), a tile reaches up
// to 256 pixels past the tensor's last pixel, and the choosers themselves form batch x height x width in int.  So both pixel
// counts stay one widest tile below 2^31; and the grid of the smallest tile any kernel has (16 pixels x 32 channels bounds
// them all from above) stays an int.  The table is in DESIGN.md section 1.
constexpr long long kY3MaxPixels = (1ll << 31) - 1 - 256;
int check_size(const y3_op &op) {
  const long long in_px = (long long)op.batch * op.in_h * op.in_w, out_px = (long long)op.batch * op.out_h * op.out_w;
  Y3_REQUIRE(in_px <= kY3MaxPixels, "op for block %d: %lld input pixels (%d x %d x %d); the limit is %lld (2^31 less one 256-pixel tile)",
             op.block_idx, in_px, op.batch, op.in_h, op.in_w, kY3MaxPixels);
  Y3_REQUIRE(out_px <= kY3MaxPixels, "op for block %d: %lld output pixels (%d x %d x %d); the limit is %lld (2^31 less one 256-pixel tile)",
             op.block_idx, out_px, op.batch, op.out_h, op.out_w, kY3MaxPixels);
  const long long tiles = (out_px / 16 + 1) * (op.out_c / 32 + 1);
  Y3_REQUIRE(tiles < (1ll << 31), "op for block %d: %lld output pixels x %d channels need %lld tiles of 16 x 32; the limit is 2^31 - 1",
             op.block_idx, out_px, op.out_c, tiles);
  return Y3_OK;
}

// grid x block of what a step launches (the grid and block its chooser recorded, which its launcher launches): fewer than 2^32
int check_launch(const y3_op &op, const y3_step &st) {
  const long long threads = st.dims.grid * st.dims.block;
  Y3_REQUIRE(threads <= kY3MaxThreads, "op for block %d: %s would be a launch of %lld threads; the limit is %lld (2^32 less one workgroup)",
             op.block_idx, st.name, threads, kY3MaxThreads);
  return Y3_OK;
}

// what one op runs on its own under options `o` (the op has passed check_flags and check_size)
int choose_op(const y3_op &op, const y3_options &o, y3_step &st) {
  Y3_REQUIRE(op.dtype == Y3_F32 || op.dtype == Y3_BF16 || op.dtype == Y3_F16, "op for block %d: unknown dtype %d", op.block_idx, op.dtype);
  Y3_REQUIRE(op.batch > 0 && op.in_h > 0 && op.in_w > 0 && op.in_c > 0, "op for block %d: empty input shape", op.block_idx);
  switch (op.kind) {
    case Y3_OP_CONV: return choose_conv(op, o, st);
    case Y3_OP_MAXPOOL: case Y3_OP_UPSAMPLE: case Y3_OP_ADD: case Y3_OP_COPY: return y3_choose_layer(op, st);
    case Y3_OP_REORG: return y3_choose_reorg(op, st);
    case Y3_OP_YOLO: return y3_choose_yolo(op, o, st);
    case Y3_OP_AVGPOOL: case Y3_OP_SCALE_CHANNELS: case Y3_OP_SAM: return y3_choose_attention(op, st);
    default: break;
  }
  y3_set_error("op for block %d: unknown kind %d", op.block_idx, op.kind);
  return Y3_ERR_INVALID;
}

// Every single-op conv kernel computes the op's activation code (common.h: y3_act); the fused conv groups hard-wire
// LeakyReLU and their choosers decline mish and logistic ops; the fused head kernels compute linear and logistic (the
// head conv of a new_coords network).  Checked once more per step, so that a chooser that forgot would be an error here and
// never a conv run as linear or leaky.
int check_activation(const y3_op *ops, int n, const y3_step &st) {
  for (int k = 0; k < n; ++k) {
    if (ops[k].kind != Y3_OP_CONV) continue;
    Y3_REQUIRE(!(ops[k].flags & Y3_F_MISH) || st.fuse == y3_fuse::none,
               "conv block %d: mish op given to %s, which does not compute mish", ops[k].block_idx, st.name);
    Y3_REQUIRE(!(ops[k].flags & Y3_F_LOGISTIC) || st.fuse == y3_fuse::none || st.fuse == y3_fuse::head_decode,
               "conv block %d: logistic op given to %s, which does not compute logistic", ops[k].block_idx, st.name);
  }
  return Y3_OK;
}

// the pointers an op launched on its own reads and writes; `in` is the plan input where the op reads that
int check_pointers(const y3_op &op, const void *in) {
  Y3_REQUIRE(in != nullptr, "op for block %d has no input pointer", op.block_idx);
  Y3_REQUIRE(op.d_out != nullptr || op.kind == Y3_OP_YOLO, "op for block %d has no output pointer", op.block_idx);
  Y3_REQUIRE(op.kind != Y3_OP_CONV || (op.d_weight && op.d_scale && op.d_bias), "conv block %d: missing parameters", op.block_idx);
  Y3_REQUIRE(op.kind != Y3_OP_YOLO || (op.d_bbox && op.d_prob && op.d_cls), "yolo block %d: missing output pointers", op.block_idx);
  Y3_REQUIRE((op.kind != Y3_OP_SCALE_CHANNELS && op.kind != Y3_OP_SAM) || op.d_res, "op for block %d has no source pointer (d_res)", op.block_idx);
  return Y3_OK;
}

// one step of a plan, as decided at plan creation
int run_op(y3_plan *plan, size_t i, const void *d_input, hipStream_t s) {
  const y3_step &st = plan->steps[i];
  if (st.fuse == y3_fuse::into_prev) return Y3_OK;
  const y3_op &op = plan->ops[i];
  const void *in = (op.flags & Y3_F_PLAN_INPUT) ? d_input : op.d_in;
  if (st.fuse == y3_fuse::none) {
    const int rc = check_pointers(op, in);
    if (rc != Y3_OK) return rc;
  }
  Y3_REQUIRE(in != nullptr, "op for block %d has no input pointer", op.block_idx);
  return st.launch(&plan->ops[i], st, in, plan->d_zero, s);
}

// Private fragment-order copies of the weights of the steps that read them, for callers that pass no y3_op.d_weight_frag: made on
// the device that OWNS the weights -- not on whichever device happens to be current (a network on cuda:1 compiled
// while device 0 is current put the copy on GPU 0) -- and on one non-blocking stream of its own, so that neither the legacy null
// stream's implicit synchronisation nor a stream capture in progress elsewhere in the process is touched.  (A plan runs on one
// stream: its weights are on one device.)
int make_private_fragment_weights(y3_plan *p) {
  int prev = -1, rc = Y3_OK;
  Y3_HIP_CHECK(hipGetDevice(&prev));
  hipStream_t s = nullptr;
  hipError_t e = hipSuccess;
  auto fail = [&](const char *what, int block) {
    y3_set_error("y3_plan_create: fragment-order weights of block %d: %s failed: %s", block, what, hipGetErrorString(e));
    rc = Y3_ERR_HIP;
  };
  for (size_t i = 0; i < p->ops.size() && rc == Y3_OK; ++i) {
    y3_step &st = p->steps[i];
    const y3_op &op = p->ops[i];
    if (!st.frag || st.frag_w) continue;
    if (!s) {
      int owner = prev;
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, op.d_weight) == hipSuccess && attr.device >= 0) owner = attr.device;
      else (void)hipGetLastError();
      if ((e = hipSetDevice(owner)) != hipSuccess) { fail("hipSetDevice", op.block_idx); break; }
      if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) { s = nullptr; fail("hipStreamCreateWithFlags", op.block_idx); break; }
    }
    void *w = nullptr;
    if ((e = hipMalloc(&w, y3_conv_halo_dw_weight_bytes(op))) != hipSuccess) { fail("hipMalloc", op.block_idx); break; }
    st.frag_w = w;
    p->frag_own[i] = 1;
    rc = y3_conv_halo_dw_make_weights(op, w, s);
  }
  if (s) {
    if ((e = hipStreamSynchronize(s)) != hipSuccess && rc == Y3_OK) fail("hipStreamSynchronize", -1);
    (void)hipStreamDestroy(s);
  }
  (void)hipSetDevice(prev);
  return rc;
}

}  // namespace

extern "C" {

int y3_abi_version(void) { return Y3_ABI_VERSION; }

uint32_t y3_capabilities(void) {
  return Y3_CAP_MISH | Y3_CAP_SCALE_X_Y | Y3_CAP_LOGISTIC | Y3_CAP_NEW_COORDS | Y3_CAP_LETTERBOX | Y3_CAP_POOL_DARKNET |
         Y3_CAP_NMS_DARKNET | Y3_CAP_SCORES_DARKNET | Y3_CAP_MULTI_LABEL | Y3_CAP_PREPROCESS_DARKNET | Y3_CAP_REORG |
         Y3_CAP_LAUNCH_LOG | Y3_CAP_PLAN_OP_DIMS | Y3_CAP_TILES | Y3_CAP_GROUPED_CONV | Y3_CAP_ATTENTION |
         Y3_CAP_TILE_MERGE;
}

int y3_debug_launch_log_begin(void) {
  Y3_REQUIRE(!tl_y3_hooks.log, "y3_debug_launch_log_begin: this thread has a launch log already");
  tl_y3_hooks.log = new (std::nothrow) Y3LaunchLog;
  Y3_REQUIRE(tl_y3_hooks.log, "y3_debug_launch_log_begin: out of memory");
  return Y3_OK;
}

int y3_debug_launch_log_end(char *names, size_t capacity, size_t *needed) {
  Y3LaunchLog *log = tl_y3_hooks.log;
  Y3_REQUIRE(log, "y3_debug_launch_log_end: this thread has no launch log");
  const size_t n = log->names.size() + 1;
  if (needed) *needed = n;
  // too small a buffer is the size query: the log stays open (and goes on recording) until a call that can take it
  Y3_REQUIRE(names && capacity >= n, "y3_debug_launch_log_end: the log needs %zu bytes, the buffer has %zu", n, capacity);
  memcpy(names, log->names.c_str(), n);
  const bool unnamed = log->unnamed;
  tl_y3_hooks.log = nullptr;
  delete log;
  Y3_REQUIRE(!unnamed, "y3_debug_launch_log_end: the runtime gave no name for a launched kernel (logged as \"?\")");
  return Y3_OK;
}

const char *y3_last_error(void) { return g_err; }

int y3_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

// which kernel family a conv op will use: 0 igemm, 1 stem, 2 direct (the host side lays the
// weights out accordingly before creating the plan)
int y3_conv_path(const y3_op *op) {
  if (!op || op->kind != Y3_OP_CONV) return -1;
  return conv_path(*op);
}

size_t y3_conv_fragment_weight_bytes(const y3_op *op, const y3_options *options) {
  if (!op || op->kind != Y3_OP_CONV || conv_path(*op) != 0) return 0;
  const y3_options &o = options ? *options : g_y3_defaults;
  y3_step st;
  // (a detection-head conv is chosen for together with the YOLO op behind it, at plan creation: asked about by its shape here)
  if (o.fuse_head && y3_conv_head_dw_fits(*op, o)) return y3_conv_halo_dw_weight_bytes(*op);
  if (check_flags(*op) != Y3_OK || check_groups(*op) != Y3_OK || check_size(*op) != Y3_OK) return 0;
  // (so is a member of a 1x1 -> 3x3 pair that fuse_block = 3 / 4 runs on the direct-weights block kernel)
  if (y3_conv_block_dw_member(*op, o)) return y3_conv_halo_dw_weight_bytes(*op);
  return choose_op(*op, o, st) == Y3_OK && st.frag ? y3_conv_halo_dw_weight_bytes(*op) : 0;
}

// the fragment-order layout needs 16-bit weights of the implicit-GEMM layout in whole 32 x 32 blocks
int y3_conv_make_fragment_weights(const y3_op *op, void *d_dst, void *stream) {
  Y3_REQUIRE(op && d_dst && op->d_weight, "y3_conv_make_fragment_weights: bad arguments");
  Y3_REQUIRE(op->kind == Y3_OP_CONV && conv_path(*op) == 0 && y3_is16(op->dtype) && op->cout_pad % 32 == 0 && op->k_ld % 32 == 0,
             "conv block %d: weights without a fragment-order layout", op->block_idx);
  return y3_conv_halo_dw_make_weights(*op, d_dst, static_cast<hipStream_t>(stream));
}

void y3_options_default(y3_options *options) {
  if (options) *options = g_y3_defaults;
}

int y3_plan_create(const y3_op *ops, int n_ops, const void *d_zero, y3_plan **out_plan) {
  return y3_plan_create_ex(ops, n_ops, d_zero, nullptr, out_plan);
}

int y3_plan_create_ex(const y3_op *ops, int n_ops, const void *d_zero, const y3_options *options, y3_plan **out_plan) {
  Y3_REQUIRE(ops && n_ops > 0 && out_plan, "y3_plan_create: bad arguments");
  Y3_REQUIRE(d_zero, "y3_plan_create: d_zero (zeroed device page) is required");
  y3_plan *p = new (std::nothrow) y3_plan;
  Y3_REQUIRE(p, "y3_plan_create: out of host memory");
  p->opt = options ? *options : g_y3_defaults;
  const y3_options &o = p->opt;
  p->ops.assign(ops, ops + n_ops);
  p->steps.assign(n_ops, y3_step());
  p->frag_own.assign(n_ops, 0);
  p->d_zero = d_zero;
  const y3_op *q = p->ops.data();
  bool private_frag = false;
  for (int i = 0; i < n_ops; ++i) {
    y3_step &st = p->steps[i];
    int rc = check_flags(q[i]);
    if (rc == Y3_OK) rc = check_groups(q[i]);
    if (rc == Y3_OK) rc = check_size(q[i]);
    if (rc != Y3_OK) {
      y3_plan_destroy(p);
      return rc;
    }
    if (st.fuse == y3_fuse::into_prev) { st.name = "(fused into the previous op)"; continue; }
    if (i + 2 < n_ops && o.fuse_spp && y3_choose_maxpool_spp(q[i], q[i + 1], q[i + 2], st)) {
      st.fuse = y3_fuse::spp;           // SPP pyramid: pool 5 / 9 / 13 of one tensor in one launch
    } else if (i + 1 < n_ops && (q[i].flags & Y3_F_FUSE_NEXT) && q[i].kind == Y3_OP_CONV &&
               y3_choose_conv_fused_stem_s2(q[i], q[i + 1], o, st)) {
      st.fuse = y3_fuse::stem_pair;
    } else if (i + 1 < n_ops && (q[i].flags & Y3_F_FUSE_NEXT) && y3_choose_conv_fused_resblock(q[i], q[i + 1], o, st)) {
      st.fuse = y3_fuse::resblock;      // whole residual block in one kernel
    } else if (i + 1 < n_ops && (q[i].flags & Y3_F_FUSE_NEXT) && y3_choose_conv_block_fused(q[i], q[i + 1], o, st)) {
      st.fuse = y3_fuse::block;         // 1x1 -> 3x3 (+ shortcut) with the 128-channel tensor in LDS
    } else if (i + 1 < n_ops && y3_choose_conv_head_decode(q[i], q[i + 1], o, st)) {
      st.fuse = y3_fuse::head_decode;   // head conv + YOLO decode (the float32 logits never leave the CU)
    } else {
      rc = choose_op(q[i], o, st);
    }
    const int absorbed = st.fuse == y3_fuse::none ? 0 : (st.fuse == y3_fuse::spp ? 2 : 1);
    if (rc == Y3_OK) rc = check_activation(q + i, absorbed + 1, st);
    if (rc == Y3_OK) rc = check_launch(q[i], st);
    if (rc != Y3_OK) {
      y3_plan_destroy(p);
      return rc;
    }
    for (int k = 1; k <= absorbed; ++k) p->steps[i + k].fuse = y3_fuse::into_prev;
    // a kernel that reads its weights in MFMA-fragment order: the caller's shared copy (y3_op.d_weight_frag, ABI 6), or --
    // callers that pass none -- a private copy that the plan makes below and frees when it is destroyed
    if (st.frag) st.frag_w = q[i].d_weight_frag;
    private_frag |= st.frag && !st.frag_w;
  }
  if (private_frag) {
    const int rc = make_private_fragment_weights(p);
    if (rc != Y3_OK) {
      y3_plan_destroy(p);
      return rc;
    }
  }
  *out_plan = p;
  return Y3_OK;
}

void y3_plan_destroy(y3_plan *plan) {
  if (!plan) return;
  for (hipEvent_t e : plan->events) (void)hipEventDestroy(e);
  for (hipEvent_t e : plan->kstart) (void)hipEventDestroy(e);
  for (hipEvent_t e : plan->kstop) (void)hipEventDestroy(e);
  for (auto &g : plan->graphs) (void)hipGraphExecDestroy(g.exec);
  for (size_t i = 0; i < plan->steps.size(); ++i)
    if (plan->frag_own[i]) (void)hipFree(const_cast<void *>(plan->steps[i].frag_w));
  delete plan;
}

static int plan_run_eager(y3_plan *plan, const void *d_input, hipStream_t s) {
  for (size_t i = 0; i < plan->ops.size(); ++i) {
    const int rc = run_op(plan, i, d_input, s);
    if (rc != Y3_OK) return rc;
  }
  return Y3_OK;
}

int y3_plan_run(y3_plan *plan, const void *d_input, void *stream) {
  Y3_REQUIRE(plan, "y3_plan_run: null plan");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // graphs need a capturable (non-default) stream; the plan's pointers and options never change, only d_input may
  if (!plan->opt.use_graph || !plan->graph_ok || s == nullptr || !plan->warmed) {
    plan->warmed = true;
    return plan_run_eager(plan, d_input, s);
  }
  for (auto &g : plan->graphs)
    if (g.input == d_input) {
      Y3_HIP_CHECK(hipGraphLaunch(g.exec, s));
      return Y3_OK;
    }
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    plan->graph_ok = false;
    return plan_run_eager(plan, d_input, s);
  }
  const int rc = plan_run_eager(plan, d_input, s);
  const hipError_t e_end = hipStreamEndCapture(s, &graph);
  if (rc != Y3_OK || e_end != hipSuccess || graph == nullptr ||
      hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
    plan->graph_ok = false;                       // capture not possible here: stay eager from now on
    return rc != Y3_OK ? rc : plan_run_eager(plan, d_input, s);
  }
  (void)hipGraphDestroy(graph);
  if (plan->graphs.size() >= 8) {                 // callers cycle through a few input buffers at most
    (void)hipGraphExecDestroy(plan->graphs.front().exec);
    plan->graphs.erase(plan->graphs.begin());
  }
  plan->graphs.push_back({d_input, exec});
  Y3_HIP_CHECK(hipGraphLaunch(exec, s));
  return Y3_OK;
}

int y3_plan_run_timed(y3_plan *plan, const void *d_input, void *stream, float *ms_per_op) {
  Y3_REQUIRE(plan && ms_per_op, "y3_plan_run_timed: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = plan->ops.size();
  while (plan->events.size() < n + 1) {
    hipEvent_t e;
    Y3_HIP_CHECK(hipEventCreate(&e));
    plan->events.push_back(e);
  }
  Y3_HIP_CHECK(hipEventRecord(plan->events[0], s));
  for (size_t i = 0; i < n; ++i) {
    const int rc = run_op(plan, i, d_input, s);
    if (rc != Y3_OK) return rc;
    Y3_HIP_CHECK(hipEventRecord(plan->events[i + 1], s));
  }
  Y3_HIP_CHECK(hipEventSynchronize(plan->events[n]));
  for (size_t i = 0; i < n; ++i) Y3_HIP_CHECK(hipEventElapsedTime(&ms_per_op[i], plan->events[i], plan->events[i + 1]));
  return Y3_OK;
}

int y3_plan_run_profiled(y3_plan *plan, const void *d_input, void *stream, float *kernel_ms_per_op) {
  Y3_REQUIRE(plan && kernel_ms_per_op, "y3_plan_run_profiled: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = plan->ops.size(), cap = 2 * n;       // (an op is one launch today; room for two)
  while (plan->kstart.size() < cap) {
    hipEvent_t a, b;
    Y3_HIP_CHECK(hipEventCreate(&a));
    plan->kstart.push_back(a);
    Y3_HIP_CHECK(hipEventCreate(&b));
    plan->kstop.push_back(b);
  }
  Y3KernelTimer timer = {plan->kstart.data(), plan->kstop.data(), 0, (int)cap};
  std::vector<int> first(n + 1, 0);
  int rc = Y3_OK;
  tl_y3_hooks.timer = &timer;
  for (size_t i = 0; i < n && rc == Y3_OK; ++i) {
    first[i] = timer.n;
    rc = run_op(plan, i, d_input, s);
  }
  first[n] = timer.n;
  tl_y3_hooks.timer = nullptr;
  if (rc != Y3_OK) return rc;
  Y3_HIP_CHECK(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i) {
    float sum = 0.f;
    for (int k = first[i]; k < first[i + 1]; ++k) {
      float ms = 0.f;
      Y3_HIP_CHECK(hipEventElapsedTime(&ms, plan->kstart[k], plan->kstop[k]));
      sum += ms;
    }
    kernel_ms_per_op[i] = sum;
  }
  return Y3_OK;
}

const char *y3_plan_op_kernel(const y3_plan *plan, int op_index) {
  if (!plan || op_index < 0 || (size_t)op_index >= plan->ops.size()) return "";
  return plan->steps[op_index].name;
}

int y3_plan_op_dims(const y3_plan *plan, int op_index, int64_t out[3]) {
  Y3_REQUIRE(plan && out && op_index >= 0 && (size_t)op_index < plan->ops.size(), "y3_plan_op_dims: bad arguments");
  const y3_step &st = plan->steps[op_index];
  const bool launched = st.fuse != y3_fuse::into_prev;
  out[0] = launched ? (int64_t)st.dims.grid : 0;
  out[1] = launched ? (int64_t)st.dims.block : 0;
  out[2] = launched ? (int64_t)st.dims.lds : 0;
  return Y3_OK;
}

double y3_plan_op_flops(const y3_plan *plan, int op_index) {
  if (!plan || op_index < 0 || (size_t)op_index >= plan->ops.size()) return 0.0;
  auto conv_flops = [](const y3_op &o) {
    return o.kind != Y3_OP_CONV ? 0.0 : 2.0 * o.ksize * o.ksize * o.in_c * (double)o.out_c * o.out_h * o.out_w * o.batch /
                                            (o.groups > 1 ? o.groups : 1);
  };
  const y3_op *q = &plan->ops[op_index];
  switch (plan->steps[op_index].fuse) {
    case y3_fuse::into_prev: return 0.0;
    case y3_fuse::stem_pair: case y3_fuse::resblock: case y3_fuse::block: return conv_flops(q[0]) + conv_flops(q[1]);
    default: return conv_flops(q[0]);   // (head_decode: the decode has no conv FLOPs)
  }
}

double y3_plan_op_bytes(const y3_plan *plan, int op_index) {
  if (!plan || op_index < 0 || (size_t)op_index >= plan->ops.size()) return 0.0;
  const y3_op &a = plan->ops[op_index];
  switch (plan->steps[op_index].fuse) {
    case y3_fuse::into_prev: return 0.0;
    case y3_fuse::stem_pair: {   // frames in, second conv's output out, both weight sets; nothing in between
      const y3_op &b = plan->ops[op_index + 1];
      return (double)a.batch * a.in_h * a.in_w * a.in_c + (double)b.batch * b.out_h * b.out_w * b.out_c * 2.0 +
             27.0 * a.out_c * 2.0 + 9.0 * b.in_c * b.out_c * 2.0;
    }
    case y3_fuse::head_decode: {   // activations + weights in, 28 bytes per box out
      const y3_op &b = plan->ops[op_index + 1];
      return ((double)a.batch * a.in_h * a.in_w * a.in_c + (double)a.in_c * a.out_c) * 2.0 +
             (double)b.batch * b.in_h * b.in_w * b.n_anchor * 28.0;
    }
    case y3_fuse::spp:   // the tensor in once, three pooled tensors out
      return 4.0 * a.batch * a.in_h * a.in_w * a.in_c * y3_elem_size(a.dtype);
    case y3_fuse::resblock: case y3_fuse::block: {   // x in (once), z out, both weight sets
      const y3_op &b = plan->ops[op_index + 1];
      return ((double)a.batch * a.in_h * a.in_w * a.in_c + (double)b.batch * b.out_h * b.out_w * b.out_c) * 2.0 +
             ((double)a.in_c * a.out_c + 9.0 * b.in_c * b.out_c) * 2.0;
    }
    case y3_fuse::none: break;
  }
  const y3_op &o = plan->ops[op_index];
  const double es = y3_elem_size(o.dtype);
  const double in_px = (double)o.batch * o.in_h * o.in_w, out_px = (double)o.batch * o.out_h * o.out_w;
  switch (o.kind) {
    case Y3_OP_CONV: {
      double in_es = es;
      if (o.flags & Y3_F_IN_NCHW_F32) in_es = 4;
      if (o.flags & Y3_F_IN_NHWC_U8BGR) in_es = 1;
      const double out_es = (o.flags & Y3_F_OUT_F32) ? 4 : es;
      double b = in_px * o.in_c * in_es + out_px * o.out_c * out_es +
                 (double)o.ksize * o.ksize * o.in_c * o.out_c * es / (o.groups > 1 ? o.groups : 1);
      if (o.flags & Y3_F_RESIDUAL) b += out_px * o.out_c * es;
      return b;
    }
    case Y3_OP_ADD: case Y3_OP_SAM: return 3.0 * out_px * o.out_c * es;
    case Y3_OP_SCALE_CHANNELS: return (2.0 * out_px + in_px) * o.out_c * es;   // src in, out, and the (C, 1, 1) scales
    case Y3_OP_YOLO: return in_px * o.n_anchor * (o.n_attr * 4.0 + 28.0);
    default: return (in_px * o.in_c + out_px * o.out_c) * es;
  }
}

int y3_set_tuning(const char *key, int value) {
  if (!key) return Y3_ERR_INVALID;
  struct { const char *name; int32_t *field; } fields[] = {
      {"auto_mask", &g_y3_defaults.auto_mask},
      {"igemm_version", &g_y3_defaults.igemm_version}, {"igemm_ns", &g_y3_defaults.igemm_ns},
      {"igemm_bm", &g_y3_defaults.igemm_bm}, {"use_graph", &g_y3_defaults.use_graph},
      {"fuse_stem", &g_y3_defaults.fuse_stem}, {"fuse_head", &g_y3_defaults.fuse_head},
      {"fuse_spp", &g_y3_defaults.fuse_spp}, {"decode_lanes", &g_y3_defaults.decode_lanes},
      {"fuse_block", &g_y3_defaults.fuse_block}};
  for (auto &f : fields)
    if (!strcmp(key, f.name)) { *f.field = value; return Y3_OK; }
  if (!strcmp(key, "device_cus")) {
    Y3_REQUIRE(value >= 0 && value <= 4096, "y3_set_tuning: device_cus %d (0 asks the device; 1 .. 4096 is the count to plan for)", value);
    g_y3_device_cus.store(value, std::memory_order_relaxed);
    return Y3_OK;
  }
  if (!strcmp(key, "grouped_generic")) {
    Y3_REQUIRE(value == 0 || value == 1, "y3_set_tuning: grouped_generic %d (0: conv_dwise where it fits; 1: conv_grouped for every grouped op)", value);
    g_y3_grouped_generic.store(value, std::memory_order_relaxed);
    return Y3_OK;
  }
#ifdef Y3_HAS_DEBUG_KEY
  if (!strcmp(key, "debug")) { g_y3_debug = value; return Y3_OK; }
#endif
  y3_set_error("y3_set_tuning: unknown key %s", key);
  return Y3_ERR_INVALID;
}

// one op on its own, chosen under the defaults in force now; a kernel that reads fragment-order weights and gets no shared copy
// (y3_op.d_weight_frag) makes one here, stream-ordered, and frees it after the launch
int y3_op_run(const y3_op *op, const void *d_input, const void *d_zero, void *stream) {
  Y3_REQUIRE(op, "y3_op_run: null op");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const void *in = (op->flags & Y3_F_PLAN_INPUT) ? d_input : op->d_in;
  int rc = check_pointers(*op, in);
  y3_step st;
  if (rc == Y3_OK) rc = check_flags(*op);
  if (rc == Y3_OK) rc = check_groups(*op);
  if (rc == Y3_OK) rc = check_size(*op);
  if (rc == Y3_OK) rc = choose_op(*op, g_y3_defaults, st);
  if (rc == Y3_OK) rc = check_launch(*op, st);
  if (rc != Y3_OK) return rc;
  st.frag_w = op->d_weight_frag;
  if (!st.frag || st.frag_w) return st.launch(op, st, in, d_zero, s);
  void *tmp = nullptr;
  Y3_HIP_CHECK(hipMallocAsync(&tmp, y3_conv_halo_dw_weight_bytes(*op), s));
  st.frag_w = tmp;
  rc = y3_conv_halo_dw_make_weights(*op, tmp, s);
  if (rc == Y3_OK) rc = st.launch(op, st, in, d_zero, s);
  (void)hipFreeAsync(tmp, s);
  return rc;
}

}  // extern "C"
