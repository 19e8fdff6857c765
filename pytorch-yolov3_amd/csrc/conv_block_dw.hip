// The fused 1x1 -> 3x3 (+ shortcut) block of the 128-channel bottleneck stage (conv_block.hip: geometry, phases, K order,
// swizzles and write-out are that kernel's) with DIRECT WEIGHTS: both convs take their weight fragments straight from the
// fragment-order copies of their weights (y3_conv_halo_dw_make_weights; the plan's shared copies, y3_op.d_weight_frag) into
// registers by inline-asm global_load_dwordx4, as conv_halo_dw_kernel / conv1x1_dw_kernel / conv_dw48_kernel do.  No weight
// slots in LDS, no LDS-DMA of weights, and
//   phase B  no barrier inside a 128-channel pass: conv_halo_dw_kernel's K-step (6 x 4 accumulator tiles, 48 MFMAs per wave, three
//            rotating register sets of four fragments, loads one K-step ahead, counted waits that name their registers) on the mid
//            image; no border masks (the mid image's rows never wrap, rows outside the frame are zero).  The old kernel paid one
//            barrier and a three-slot ring with one step of lead per K-step (2250 cycles for 1536 of MFMA).
//   phase A  x still streams through LDS in 32-channel sub-chunks (kNB buffers of 28 KiB, LDS-DMA kLX = kNB - 1 sub-steps ahead, one
//            barrier per sub-chunk); the 1x1's fragments run ONE sub-step ahead in two alternating register sets.  vmcnt retires
//            in order, so a sub-step issues its weight loads BEFORE its x pieces: the wait for the fragments of sub-step j then
//            leaves the youngest sub-chunk of x in flight.
// Nothing that writes a register another load may still be filling sits under a branch: a tie ("+v") in one of several branches
// makes the compiler COPY the registers into the branch -- before the wait, i.e. possibly before the data has landed.  So the
// counted waits that depend on a run-time count are plain waits, followed by ONE unconditional tie; every register-destination
// load is issued unconditionally (past the end: a valid address again); and both passes drain their run-ahead loads before the
// write-out, whose branches they would otherwise cross in flight.
// LDS: kNB x 28 KiB.  kNB = 4 (112 KiB, exactly the mid image) returns all 48 KiB of the old ring to whatever else runs on the
// CU; kNB = 5 (140 KiB: a fifth x buffer, x four sub-steps ahead) measured level per launch and 0.2 % behind end to end -- phase A
// is bound by HBM, not by its lead (profiles/block_dw_AB.txt) -- so four it is (-DY3_BLOCK_DW_XBUF=5 builds the other).
// Same K order (chunk outermost, tap innermost, K-halves in order) and the same epilogue arithmetic as the two separate
// launches and as conv_block_fused_kernel: same bits.  Selected by y3_options.fuse_block = 3 (4: wherever supported, tests);
// lives in libyolov3_hip_block.so so that the device code of libyolov3_hip.so stays what it was (csrc/Makefile).
#include "common.h"
#include "conv_device.h"

#ifndef Y3_BLOCK_DW_XBUF
#define Y3_BLOCK_DW_XBUF 4
#endif

namespace {

constexpr int kHaloRows = 448;                  // patch rows a workgroup can hold (28 fragments)
constexpr int kPlane = kHaloRows * 128;         // one mid plane (64 channels): 57344 bytes
constexpr int kNT = 512;
constexpr int kMA = 7;                          // phase A: fragments per wave (4 pixel groups x 7 = 28)
constexpr int kMB = 6;                          // phase B: fragments per wave (4 pixel groups x 6 = 24 -> 384 pixels)
constexpr int kMH = kMB / 2;
constexpr int kSub = kHaloRows * 64;            // one 32-channel sub-chunk of the x patch: 28672 bytes
constexpr int kNB = Y3_BLOCK_DW_XBUF;           // x buffers of phase A
constexpr int kLX = kNB - 1;                    // sub-steps the x sub-chunks run ahead
constexpr int kBlockDwLds = kNB * kSub;
static_assert(kNB == 4 || kNB == 5, "four or five x buffers");
static_assert(kBlockDwLds >= 2 * kPlane && kBlockDwLds <= 160 * 1024, "the x buffers of phase A hold the mid image of phase B");

struct BlockDwArgs {
  const char *x;      // 1x1 input (B, H, W, x_ld); also the shortcut operand when `res`
  int H, W, x_ld, ns; // ns = Cin / 64 channel chunks of the 1x1
  const char *w1; int kb1; const float *sc1, *bi1;   // 1x1: fragment-order copy, kb1 = k_ld / 32 blocks per channel block
  const char *w3; int kb3; const float *sc3, *bi3;   // 3x3: fragment-order copy, k = tap * 128 + ci
  char *out; int out_ld, npass;                      // npass = Cout / 128
  int res;            // 1: add x (shortcut)
  int leaky1, leaky3;
  int TW, TH, tiles_x, tiles_y;
  uint32_t inv_pw, inv_tw;   // n / d == (n * inv) >> 16 for n < 512 (d = TW + 2, TW)
};

__device__ __forceinline__ uint32_t lane32(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// y3_wait_vmcnt_for over the six shortcut registers of a half of the write-out (and a compiler barrier for memory accesses)
template <int N>
__device__ __forceinline__ void wait_vmcnt_for6(u32x4 (&r)[6]) {
  asm volatile("s_waitcnt vmcnt(%6)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]) : "n"(N) : "memory");
}

// ... and the tie alone, after plain waits that sit under branches
__device__ __forceinline__ void tie6(u32x4 (&r)[6]) {
  asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]) :: "memory");
}

template <int V>
using IntC = std::integral_constant<int, V>;

template <typename T>
__global__ __launch_bounds__(kNT) void conv_block_dw_kernel(BlockDwArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int pg = wave >> 1, cg = wave & 1;            // pixel group (4), channel group (2 x 64 channels)

  int tile = y3_xcd_remap(blockIdx.x, gridDim.x);
  const int tx = tile % p.tiles_x;
  tile /= p.tiles_x;
  const int ty = tile % p.tiles_y, b = tile / p.tiles_y;
  const int oy0 = ty * p.TH, ox0 = tx * p.TW;
  const int PW = p.TW + 2;
  const int nhalo = PW * (p.TH + 2), npx = p.TW * p.TH;

  // ---- x loader of phase A (conv_block_fused_kernel's): 32-channel sub-chunks, 64-byte LDS rows; a pass of the 512 threads
  // fills 128 rows, thread t -> row t >> 2 of the pass, 16-byte piece (t & 3) ^ ((row >> 1) & 3) of the row's 64 bytes ----
  const int arow = tid >> 2, apc16 = ((tid & 3) ^ ((tid >> 3) & 3)) << 4;
  constexpr int kAX = 4;                              // passes per x sub-chunk (the last one: rows 384..447, waves 0-3 only)
  const int n_ax = wave < 4 ? kAX : kAX - 1;
  uint32_t xoff[kAX];
#pragma unroll
  for (int i = 0; i < kAX; ++i) {
    int row = i * 128 + arow;
    row = row < nhalo ? row : nhalo - 1;              // rows past the patch: any valid address (their mid rows are unused)
    const int hr = (int)(((uint32_t)row * p.inv_pw) >> 16), hc = row - hr * PW;
    int gy = oy0 - 1 + hr, gx = ox0 - 1 + hc;         // pixels outside the frame: clamped (their mid rows are forced to zero)
    gy = gy < 0 ? 0 : (gy >= p.H ? p.H - 1 : gy);
    gx = gx < 0 ? 0 : (gx >= p.W ? p.W - 1 : gx);
    xoff[i] = (uint32_t)((b * p.H + gy) * p.W + gx) * (uint32_t)(p.x_ld * 2) + (uint32_t)apc16;
  }
  auto issue_x = [&](int j) {                         // sub-chunk j -> buffer j % kNB
    const char *base = p.x + j * 64;
    char *dst = smem + (j % kNB) * kSub + wave * 1024;
#pragma unroll
    for (int i = 0; i < kAX - 1; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void *)(base + lane32(xoff[i])), (lds_void *)(dst + i * (kNT * 16)), 16, 0, 0);
    if (wave < 4)
      __builtin_amdgcn_global_load_lds((gbl_void *)(base + lane32(xoff[kAX - 1])), (lds_void *)(dst + (kAX - 1) * (kNT * 16)), 16, 0, 0);
  };

  // ---- weight fragments: block (channel block cb, K block kb) of a fragment-order copy sits at ((cb * KB + kb) << 10), the
  // lane's 16 bytes at lane * 16 (conv_halo.hip weights_to_fragment_order_kernel; row fr of block cb = channel y3_pair_perm(cb * 16 + fr)) ----
  const uint32_t f_voff = (uint32_t)lane * 16u;
  const char *a_base[4], *b_base[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    a_base[ni] = p.w1 + (((long long)(cg * 4 + ni) * p.kb1) << 10);
    b_base[ni] = p.w3 + (((long long)(cg * 4 + ni) * p.kb3) << 10);
  }
  auto load_wa = [&](u32x4 (&w)[4], int j) {          // 1x1, K block j = sub-chunk j
    const uint32_t voff = f_voff + ((uint32_t)j << 10);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(w[ni]) : "v"(voff), "s"(a_base[ni]));
  };
  auto load_w0 = [&](u32x4 (&w)[4], uint32_t voff) {  // 3x3, K-half 0 / 1 of a K-step
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(w[ni]) : "v"(voff), "s"(b_base[ni]));
  };
  auto load_w1 = [&](u32x4 (&w)[4], uint32_t voff) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(w[ni]) : "v"(voff), "s"(b_base[ni]));
  };
  // K-step (pass np, chunk c, tap) of the 3x3: K blocks tap * 4 + c * 2 (+ 1) of channel blocks np * 8 + cg * 4 + ni
  auto w3_voff = [&](int np, int c, int tap) {
    return f_voff + ((uint32_t)(np * 8 * p.kb3 + tap * 4 + c * 2) << 10);   // < 2^31: chooser
  };

  Y3_STAMP_DECL

  // L2 warm-up of the 3x3's weights (conv_block_fused_kernel's, on the fragment-order copy): every workgroup of the chip reads
  // the same 16 KiB in the same K-step, each once per launch, one K-step ahead; the workgroups of an XCD share a pass's 2304 lines.
  uint32_t sink = 0;   // destination of the warm-up loads: stays allocated until they have returned (tied into the wait below)
  auto warm_l2 = [&](int np_w) {
    const int per_xcd = (gridDim.x + 7) >> 3, mine = blockIdx.x >> 3;
    const int lines = 8 * 288;                                   // 8 channel blocks x 36 K blocks of 1 KiB
    const int share = (lines + per_xcd - 1) / per_xcd;
    for (int l = mine * share + tid; l < (mine + 1) * share && l < lines; l += kNT) {
      const int row = l / 288, seg = l - row * 288;
      const uint32_t off = ((uint32_t)((np_w * 8 + row) * p.kb3) << 10) + (uint32_t)seg * 128u;
      asm volatile("global_load_dword %0, %1, %2" : "+v"(sink) : "v"(off), "s"(p.w3) : "memory");
    }
  };

  // ---- phase A: mid = leaky(bn(conv1x1(x))) over the patch ----
  const int pA = pg * kMA * 16 + fr;                  // patch row of fragment 0; fragment mi is 16 mi rows further
  const int aswz = (fq ^ ((fr >> 1) & 3)) << 4;
  const int a_rd = pA * 64 + aswz;                    // + mi * 1024
  // where this lane's results go in the mid image, and whether the pixel lies inside the frame
  int midw[kMA];
  uint32_t inside = 0;
#pragma unroll
  for (int mi = 0; mi < kMA; ++mi) {
    const int pr = pA + mi * 16;
    const int hr = (int)(((uint32_t)pr * p.inv_pw) >> 16), hc = pr - hr * PW;
    const int key = (p.TW * hr + hc) & 7;
    midw[mi] = cg * kPlane + pr * 128 + ((fq ^ key) << 4);
    const bool in = pr < nhalo && (unsigned)(oy0 - 1 + hr) < (unsigned)p.H && (unsigned)(ox0 - 1 + hc) < (unsigned)p.W;
    inside |= (in ? 1u : 0u) << mi;
  }
  u32x4 wf[3][4];                                     // phase B's weight register sets
  {
    f32x4 acc[kMA][4];
#pragma unroll
    for (int mi = 0; mi < kMA; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsub = 2 * p.ns;                        // even, >= 6: chooser
    u32x4 wa[2][4];
    // Sub-step s issues, after its barrier, the fragments of sub-step s + 1 and THEN the x pieces of sub-chunk s + kLX; the
    // prologue is sub-steps -kLX .. -1 of that rule.
    y3_static_for<kLX - 1>([&](auto ic) { issue_x(decltype(ic)::value); });
    load_wa(wa[0], 0);
    issue_x(kLX - 1);
    auto step_a = [&](auto sc, int j) {
      constexpr int S = decltype(sc)::value;          // j & 1
      // younger than the fragments of sub-step j: the pieces of sub-chunk j - 1 + kLX (4 in waves 0-3, 3 in waves 4-7), if it exists.
      // (x(j) is older.)  Plain waits under the branches, then the one tie.
      if (j - 1 + kLX < nsub) {
        if (n_ax == kAX) y3_wait_vmcnt<kAX>();
        else y3_wait_vmcnt<kAX - 1>();
      } else {
        y3_wait_vmcnt<0>();
      }
      asm volatile("" : "+v"(wa[S][0]), "+v"(wa[S][1]), "+v"(wa[S][2]), "+v"(wa[S][3]));
      __builtin_amdgcn_s_barrier();                   // sub-chunk j is in LDS; everyone is done with sub-step j - 1
      Y3_STAMP(0);
      load_wa(wa[S ^ 1], j + 1 < nsub ? j + 1 : j);   // into the set of sub-step j - 1 (past the end: this step's again, unused)
      if (j + kLX < nsub) issue_x(j + kLX);           // into the buffer of sub-step j - 1
      const char *xb = smem + (j % kNB) * kSub;
      u32x4 xf[kMA];
#pragma unroll
      for (int mi = 0; mi < kMA; ++mi) xf[mi] = *reinterpret_cast<const u32x4 *>(xb + a_rd + mi * 1024);
#pragma unroll
      for (int mi = 0; mi < kMA; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = y3_mfma16<T>(wa[S][ni], xf[mi], acc[mi][ni]);
      wait_lgkm0();
      Y3_STAMP(1);
    };
#pragma unroll 1
    for (int j = 0; j < nsub; j += 2) {
      step_a(IntC<0>{}, j);
      step_a(IntC<1>{}, j + 1);
    }
    y3_wait_vmcnt_for<0>(wa[0]);                      // the last sub-step's run-ahead load (nobody uses it) has landed
    __builtin_amdgcn_s_barrier();                     // every read of the x buffers is done
    for (int npw = 0; npw < p.npass; ++npw) warm_l2(npw);
    // K-step 0 of phase B: both K-halves (their latency, and the warm-up's, runs under the mid image's write)
    load_w0(wf[0], w3_voff(0, 0, 0));
    load_w1(wf[2], w3_voff(0, 0, 0));
    // scale / bias / leaky -> storage type -> mid image (over the x buffers)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ch0 = (cg * 2 + k) * 32 + fq * 8;     // this lane's eight channels of fragment pair k
      const f32x4 sl = *reinterpret_cast<const f32x4 *>(p.sc1 + ch0), sh = *reinterpret_cast<const f32x4 *>(p.sc1 + ch0 + 4);
      const f32x4 bl = *reinterpret_cast<const f32x4 *>(p.bi1 + ch0), bh = *reinterpret_cast<const f32x4 *>(p.bi1 + ch0 + 4);
#pragma unroll
      for (int mi = 0; mi < kMA; ++mi) {
        float v[8];
        y3_bn_act8(v, acc[mi][2 * k], acc[mi][2 * k + 1], sl, sh, bl, bh, p.leaky1 ? Y3_ACT_LEAKY : Y3_ACT_LINEAR);
        u32x4 ov = y3_pack8<T>(v);
        if (!((inside >> mi) & 1u)) ov = u32x4{0u, 0u, 0u, 0u};   // the 3x3's zero padding
        *reinterpret_cast<u32x4 *>(smem + (midw[mi] ^ (k * 64))) = ov;
      }
    }
  }

  // ---- phase B: 3x3 from the mid image ----
  int p0b[kMB];        // byte offset of the mid row of tap (0, 0) of this lane's pixel of fragment mi
#pragma unroll
  for (int mi = 0; mi < kMB; ++mi) {
    const int q = (pg * kMB + mi) * 16 + fr;
    const int qc = q < npx ? q : npx - 1;
    const int r = (int)(((uint32_t)qc * p.inv_tw) >> 16), c = qc - r * p.TW;
    p0b[mi] = (r * PW + c) * 128;
  }
  // (b * H + oy) * W + ox of that pixel (of the tile's first pixel if it is not stored): recomputed at every write-out, from the
  // lane's fr behind an empty asm of that write-out -- else these, and the offsets made of them, are computed before the K loop
  // and kept (spilled) through it
  auto out_px = [&](int mi, int frv, bool &ok) {
    const int q = (pg * kMB + mi) * 16 + frv;
    const int qc = q < npx ? q : npx - 1;
    const int r = (int)(((uint32_t)qc * p.inv_tw) >> 16), c = qc - r * p.TW;
    const int oy = oy0 + r, ox = ox0 + c;
    ok = q < npx && oy < p.H && ox < p.W;
    return ok ? (b * p.H + oy) * p.W + ox : (b * p.H + oy0) * p.W + ox0;
  };
  f32x4 acc[kMB][4];
  u32x4 xf[kMB];
  // K-half 0 of tap (ky, kx) of mid plane c, relative to p0b: tap shift, plane, swizzle key (the output raster index mod 8);
  // K-half 1 is the same ^ 64
  // (frv: the lane's fr behind an empty asm of the K-step that uses it -- computed from fr itself the offsets of all nine taps,
  // and their sums with p0b, are loop invariants that the compiler hoists out of the K loop and then spills)
  auto tap_off = [&](int c, auto tapc, int frv) {
    constexpr int tap = decltype(tapc)::value, ky = tap / 3, kx = tap % 3;
    return ((fq ^ ((frv + p.TW * ky + kx) & 7)) << 4) + (ky * PW + kx) * 128 + c * kPlane;
  };
  auto read_half = [&](int lo, int toff) {
#pragma unroll
    for (int mi = 0; mi < kMH; ++mi) xf[lo + mi] = *reinterpret_cast<const u32x4 *>(smem + (p0b[lo + mi] + toff));
  };
  auto mma_half = [&](int lo, const u32x4 (&w)[4]) {
#pragma unroll
    for (int mi = 0; mi < kMH; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[lo + mi][ni] = y3_mfma16<T>(w[ni], xf[lo + mi], acc[lo + mi][ni]);
  };
  // One K-step (64 channels of one tap): conv_halo_dw_kernel's.  The step with S = tap % 3 multiplies K-half 0 with wf[S] and K-half 1
  // with wf[(S + 2) % 3]; the next step's K-half 0 is loaded into wf[(S + 1) % 3] at the top, its K-half 1 into wf[S] once this
  // step's K-half 0 MFMAs are issued (18 steps per pass: the rotation is the same in every pass).  VMEM order per step: 4 loads,
  // 4 loads.  A pass's last step loads the next pass's first step (after the last pass: K-step 0 of pass 0 again, a valid
  // address); both sets are waited for, by name, before the write-out.
  auto kstep = [&](auto tapc, int np, int c) {
    constexpr int tap = decltype(tapc)::value, S = tap % 3, tap_n = tap == 8 ? 0 : tap + 1;
    int c_n = c, np_n = np;
    if constexpr (tap == 8) {
      if (c == 1) { c_n = 0; np_n = np + 1 < p.npass ? np + 1 : 0; }
      else c_n = 1;
    }
    const uint32_t voff_n = w3_voff(np_n, c_n, tap_n);
    const int frv = (int)lane32((uint32_t)fr);
    const int toff = tap_off(c, tapc, frv);
    load_w0(wf[(S + 1) % 3], voff_n);
    y3_wait_vmcnt_for<8>(wf[S]);                      // younger for certain: 4 loads of the previous step + 4 of this one
    mma_half(0, wf[S]);
    read_half(0, toff ^ 64);
    mma_half(kMH, wf[S]);
    read_half(kMH, toff ^ 64);
    __builtin_amdgcn_sched_barrier(0);
    load_w1(wf[S], voff_n);
    y3_wait_vmcnt_for<8>(wf[(S + 2) % 3]);            // younger for certain: 4 + 4 loads of this step
    mma_half(0, wf[(S + 2) % 3]);
    if (tap == 8 && c == 1) {
      mma_half(kMH, wf[(S + 2) % 3]);                 // end of a pass: the write-out wants the fragment registers
    } else {
      const int toff_n = tap_off(c_n, IntC<tap_n>{}, frv);
      read_half(0, toff_n);
      mma_half(kMH, wf[(S + 2) % 3]);
      read_half(kMH, toff_n);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // write-out of output channels np * 128 .. + 127 straight from the accumulators (one copy of the code per kind of block, so
  // that the shortcut registers are defined and used in the same branch)
  auto write_out = [&](auto with_res, int np) {
    constexpr bool RES = decltype(with_res)::value;
    int pxo[kMB];
    uint32_t stored = 0;
    const int frv = (int)lane32((uint32_t)fr);
#pragma unroll
    for (int mi = 0; mi < kMB; ++mi) {
      bool ok;
      pxo[mi] = out_px(mi, frv, ok);
      stored |= (ok ? 1u : 0u) << mi;
    }
    f32x4 sl[2], sh[2], bl[2], bh[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ch0 = np * 128 + (cg * 2 + k) * 32 + fq * 8;
      sl[k] = *reinterpret_cast<const f32x4 *>(p.sc3 + ch0); sh[k] = *reinterpret_cast<const f32x4 *>(p.sc3 + ch0 + 4);
      bl[k] = *reinterpret_cast<const f32x4 *>(p.bi3 + ch0); bh[k] = *reinterpret_cast<const f32x4 *>(p.bi3 + ch0 + 4);
    }
    u32x4 rv[2][kMB];
    if constexpr (RES) {
      // shortcut operand (from x): both halves go out at once
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int mi = 0; mi < kMB; ++mi) {
          const uint32_t ro = (uint32_t)(pxo[mi] * p.x_ld + np * 128 + (cg * 2 + k) * 32 + fq * 8) * 2u;   // < 2^32: chooser
          asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(rv[k][mi]) : "v"(ro), "s"(p.x) : "memory");
        }
      // younger than half 0 for certain: the six loads of half 1
      wait_vmcnt_for6<6>(rv[0]);
    }
    auto half = [&](int k, int mi) {
      float v[8];
      y3_bn_act8(v, acc[mi][2 * k], acc[mi][2 * k + 1], sl[k], sh[k], bl[k], bh[k], p.leaky3 ? Y3_ACT_LEAKY : Y3_ACT_LINEAR);
      if constexpr (RES) y3_add8<T>(v, rv[k][mi]);
      return y3_pack8<T>(v);
    };
    auto store = [&](int k, int mi, const u32x4 &ov) {
      const int ch0 = np * 128 + (cg * 2 + k) * 32 + fq * 8;
      if ((stored >> mi) & 1u) *reinterpret_cast<u32x4 *>(p.out + lane32((uint32_t)(pxo[mi] * p.out_ld + ch0) * 2u)) = ov;
    };
#pragma unroll
    for (int mi = 0; mi < kMB; ++mi) store(0, mi, half(0, mi));
    if constexpr (RES) {
      // Younger than half 1 for certain: the stores of half 0 that this wave issued.  They are predicated per lane and a store none
      // of whose lanes is live may be skipped, so the count is taken from the mask: one store per fragment with a live lane (a
      // store issued all the same only makes the wait stricter).
      int ns = 0;
#pragma unroll
      for (int mi = 0; mi < kMB; ++mi) ns += __builtin_amdgcn_ballot_w64((stored >> mi) & 1u) != 0ull ? 1 : 0;
      if (ns == 0) y3_wait_vmcnt<0>();                // (plain waits under the branches, then the one tie: see the file header)
      else if (ns == 1) y3_wait_vmcnt<1>();
      else if (ns == 2) y3_wait_vmcnt<2>();
      else if (ns == 3) y3_wait_vmcnt<3>();
      else if (ns == 4) y3_wait_vmcnt<4>();
      else if (ns == 5) y3_wait_vmcnt<5>();
      else y3_wait_vmcnt<6>();
      tie6(rv[1]);
    }
#pragma unroll
    for (int mi = 0; mi < kMB; ++mi) store(1, mi, half(1, mi));
  };

  // the younger wave of each SIMD loses every issue arbitration to its older partner: a static priority evens the pair out
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  Y3_STAMP(2);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink) :: "memory");
  y3_wait_vmcnt_for<0>(wf[0]);
  y3_wait_vmcnt_for<0>(wf[2]);
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();                       // mid image complete
  Y3_STAMP(3);
#pragma unroll 1
  for (int np = 0; np < p.npass; ++np) {
#pragma unroll
    for (int mi = 0; mi < kMB; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const int toff0 = tap_off(0, IntC<0>{}, (int)lane32((uint32_t)fr));
      read_half(0, toff0);
      read_half(kMH, toff0);
    }
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
      kstep(IntC<0>{}, np, c); kstep(IntC<1>{}, np, c); kstep(IntC<2>{}, np, c);
      kstep(IntC<3>{}, np, c); kstep(IntC<4>{}, np, c); kstep(IntC<5>{}, np, c);
      kstep(IntC<6>{}, np, c); kstep(IntC<7>{}, np, c); kstep(IntC<8>{}, np, c);
    }
    // The run-ahead loads of the next pass's first step (wf[0]: K-half 0, wf[2]: K-half 1; tap 8 has S = 2) -- after the last
    // pass: of a step nobody runs -- land before the write-out: its branches must not be crossed by registers in flight, and after
    // the last pass nothing else would keep the registers allocated until then (the comment after conv_halo_dw_kernel's K loop,
    // profiles/r05s_halo_dw.txt).
    y3_wait_vmcnt_for<0>(wf[0]);
    y3_wait_vmcnt_for<0>(wf[2]);
    Y3_STAMP(5);
    if (p.res) write_out(std::true_type{}, np);
    else write_out(std::false_type{}, np);
    Y3_STAMP(6);
  }
  __builtin_amdgcn_s_setprio(0);
  Y3_STAMP_COUNT();
}

// Geometry of the kernel on tw x th rectangles (conv_block.hip choose_tile): one workgroup of kNT threads per rectangle
struct BlockDwGeom { int tiles_x, tiles_y; long long grid; };
BlockDwGeom block_dw_geom(const y3_op &op0, int tw, int th) {
  BlockDwGeom g;
  g.tiles_x = y3_ceil_div(op0.in_w, tw);
  g.tiles_y = y3_ceil_div(op0.in_h, th);
  g.grid = (long long)g.tiles_x * g.tiles_y * op0.batch;
  return g;
}

int launch_block_dw(const y3_op *ops, const y3_step &st, const void *, const void *, hipStream_t s) {
  const y3_op &op0 = ops[0], &op1 = ops[1];
  const BlockDwGeom g = block_dw_geom(op0, st.tw, st.th);
  BlockDwArgs a;
  a.x = static_cast<const char *>(op0.d_in);
  a.H = op0.in_h; a.W = op0.in_w; a.x_ld = op0.in_ld; a.ns = op0.in_c / 64;
  a.w1 = static_cast<const char *>(op0.d_weight_frag); a.kb1 = op0.k_ld / 32; a.sc1 = op0.d_scale; a.bi1 = op0.d_bias;
  a.w3 = static_cast<const char *>(op1.d_weight_frag); a.kb3 = op1.k_ld / 32; a.sc3 = op1.d_scale; a.bi3 = op1.d_bias;
  a.out = static_cast<char *>(op1.d_out); a.out_ld = op1.out_ld; a.npass = op1.out_c / 128;
  a.res = (op1.flags & Y3_F_RESIDUAL) ? 1 : 0;
  a.leaky1 = (op0.flags & Y3_F_LEAKY) ? 1 : 0;
  a.leaky3 = (op1.flags & Y3_F_LEAKY) ? 1 : 0;
  a.TW = st.tw;
  a.TH = st.th;
  a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y;
  a.inv_pw = (65536u + (uint32_t)(a.TW + 2) - 1u) / (uint32_t)(a.TW + 2);
  a.inv_tw = (65536u + (uint32_t)a.TW - 1u) / (uint32_t)a.TW;
  return y3_by_dtype16(op0.dtype, [&](auto tag) {
    return y3_launch<conv_block_dw_kernel<decltype(tag)>>(st.dims, s, a);
  });
}

}  // namespace

// What the direct-weights kernel needs beyond y3_choose_conv_block_fused's conditions: both convs carry the caller's
// fragment-order copy (no private copies for fused steps: a pair without them runs as two launches), whole 32 x 32 blocks
bool y3_conv_block_dw_fits(const y3_op &op0, const y3_op &op1) {
  if (!op0.d_weight_frag || !op1.d_weight_frag) return false;
  return op0.k_ld % 32 == 0 && op1.k_ld % 32 == 0 && op0.cout_pad % 32 == 0 && op1.cout_pad % 32 == 0;
}

// fills the step for a pair that y3_choose_conv_block_fused accepted on tw x th rectangles
void y3_choose_conv_block_dw(const y3_op &op0, int tw, int th, y3_step &st) {
  st.tw = tw;
  st.th = th;
  st.launch = launch_block_dw;
  st.dims = {block_dw_geom(op0, tw, th).grid, kNT, kBlockDwLds};
  st.name = Y3_KNAME(op0.dtype, "conv_block_dw_", "_x128");
}

Y3_STAMP_READER(y3_debug_stamps_block_dw)
