// Which kernel runs a forward conv (hiseg_conv2d_fwd and its planners; include/hiseg.h).
//
// Nine kernel families sit beside the generic implicit GEMM of conv_igemm.hip, one file each; all share one host
// interface (conv_common.h): family_try(a, s, variant) launches and returns 1, declines the layer with 0, or fails
// with < 0.  This file holds
//   conv_args        the one place a ConvArgs is filled from a descriptor
//   kFamilies        the families in routing order, each with the variant numbers it owns (a forced variant)
//   auto_candidates  the ordered (family, variant) list of the automatic choice (variant 0), with the measurements
//                    that put each entry where it is
//   conv_one_range   the single loop that tries the candidates and falls back to the generic kernel
//   conv_in_ranges   image ranges for operands of >= 2 GiB and for the pointwise kernel's SE-gate table
//   conv2d_impl      argument validation and the fused-statistics form, in front of those
// A new family: declare its *_try in conv_common.h, add its HISEG_CONV_PATH_* id (include/hiseg.h), one kFamilies
// row with its variant numbers, and -- if the automatic choice should use it -- one line in auto_candidates at the
// place its measurements justify.
#include <atomic>
#include <climits>
#include <cstdlib>
#include "conv_common.h"

using namespace hiseg;

// Which kernel took each forward conv (hiseg_conv2d_path_stats, hiseg_conv2d_last_path; include/hiseg.h): conv2d_impl
// notes the family and the variant number it passed to the *_try that launched -- for the generic kernel, the Cout
// tile of its launch -- so a test can tell a forced variant that ran from one that declined the layer.
static std::atomic<long long> g_conv_paths[HISEG_CONV_PATH_FAMILIES];
static thread_local int g_conv_last = -1;

static void conv_note_path(int family, int variant) {
  g_conv_paths[family].fetch_add(1);
  g_conv_last = family * 10000 + variant;
}

extern "C" int hiseg_conv2d_last_path(void) { return g_conv_last; }

extern "C" int hiseg_conv2d_path_stats(long long* counts, int n, int reset) {
  for (int i = 0; i < HISEG_CONV_PATH_FAMILIES; ++i) {
    // (reset: one exchange, so a launch counted on another thread between a load and a store is not lost)
    const long long c = reset ? g_conv_paths[i].exchange(0) : g_conv_paths[i].load();
    if (counts && i < n) counts[i] = c;
  }
  return HISEG_CONV_PATH_FAMILIES;
}

// ---------------------------------------------------------------------------------------- ConvArgs
// Every field of a ConvArgs, from the descriptor alone.  The entry points keep their own guards in front of it (dtype,
// N > 0, M < 2^31, K_pad a whole number of K blocks, a_up): M is 0 when the pixel count passes 2^31, a_up <= 0 reads
// as 1.
static ConvArgs conv_args(const hiseg_conv2d_desc& d) {
  ConvArgs a;
  a.d = d;
  const long long M = (long long)d.N * d.Ho * d.Wo;
  a.M = M < (1ll << 31) ? (int)M : 0;
  a.Cin = d.Ca + d.Cb;
  a.nK = d.K_pad / (d.dtype == HISEG_BF16 ? 64 : 32);
  const int up = d.a_up > 0 ? d.a_up : 1;
  a.Hs = d.H / up;
  a.Ws = d.W / up;
  a.kper = a.nK;
  a.ins_vec = d.in_scale != nullptr && ((uintptr_t)d.in_scale & 15) == 0 && (d.Ca & 3) == 0;
  a.ws = static_cast<float*>(d.workspace);
  return a;
}

// ---------------------------------------------------------------------------------------- toggles
// HISEG_CONV_HWC64=0 (read per call; A/B timing): the 64-Cout layers on conv_hwr (variant 100) instead of conv_hwc 107
static bool hwc64_mode() {
  const char* e = getenv("HISEG_CONV_HWC64");
  return !(e && atoi(e) == 0);
}

// HISEG_CONV_HWC_R3=0 (read per call; A/B timing): the 128-Cout layers on variant 104 (two halo buffers) instead of 108
static bool hwc_r3_mode() {
  const char* e = getenv("HISEG_CONV_HWC_R3");
  return !(e && atoi(e) == 0);
}

// HISEG_CONV_HWC_MTW=0|1 (read per call; A/B timing): the multi-tile conv_hwc forms (109 for 128-multiple Cout, 102 for
// the 64-Cout layers) instead of 108 / 107
#ifndef HISEG_CONV_HWC_MT_DEFAULT
#define HISEG_CONV_HWC_MT_DEFAULT(bco) false
#endif
static bool hwc_mt_mode(const char* e, int bco) {   // e: getenv("HISEG_CONV_HWC_MTW"), one read per call for both tiles
  if (e) return atoi(e) != 0;
  return HISEG_CONV_HWC_MT_DEFAULT(bco);
}

// ---------------------------------------------------------------------------------------- planners
// Workspace bytes the automatic choice uses for this layer (split-K generic kernel), 0 when it needs none.
extern "C" long long hiseg_conv2d_workspace_bytes(const hiseg_conv2d_desc* d) {
  if (d == nullptr || d->dtype != HISEG_BF16 || d->convT || d->N <= 0) return 0;
  const long long M = (long long)d->N * d->Ho * d->Wo;
  if (M >= (1ll << 31) || d->K_pad % 64) return 0;
  const ConvArgs a = conv_args(*d);
  if (conv_pw_applies(a)) return 0;
  // an SE-gated 1x1 layer whose gate table exceeds the pointwise kernel's LDS runs in image ranges on that kernel
  // (conv_in_ranges), never on the split-K path
  if (d->in_scale && d->KH == 1 && d->KW == 1 && conv_pw_gate_images(a) > 0) return 0;
  return splitk_bytes(a, splitk_plan(a));
}

extern "C" int hiseg_conv2d_stats_tiles(const hiseg_conv2d_desc* d) {
  if (d == nullptr || d->dtype != HISEG_BF16 || d->convT || d->N <= 0) return 0;
  const long long M = (long long)d->N * d->Ho * d->Wo;
  if (M >= (1ll << 31)) return 0;
  return conv_hwc_stats_tiles(conv_args(*d));
}

// The fused operands of rounds 7, 8 and 10 -- whether any is set, and in a combination some kernel has: px_scale
// alone (the pointwise kernel); head2_out, with or without res_gate; a_gate alone (the 3x3 halo kernel); raw_src
// alone (the halo-tiled direct kernel's stem form).
static bool has_fused_operands(const hiseg_conv2d_desc* d) {
  return d->px_scale || d->head2_out || d->a_gate || d->res_gate || d->raw_src;
}
static bool fused_operands_ok(const hiseg_conv2d_desc* d) {
  if (!has_fused_operands(d)) return false;
  if (d->raw_src) return !d->px_scale && !d->head2_out && !d->a_gate && !d->res_gate;
  if (d->px_scale) return !d->head2_out && !d->a_gate && !d->res_gate;
  if (d->a_gate) return !d->head2_out && !d->res_gate;
  return d->head2_out != nullptr;   // (res_gate rides with head2_out only)
}

extern "C" int hiseg_conv2d_fused_ok(const hiseg_conv2d_desc* d) {
  if (d == nullptr || d->dtype != HISEG_BF16 || d->N <= 0 || !fused_operands_ok(d) || d->stats_partial ||
      d->bnb_partial || d->a_up != 1 || d->K_pad % 64)
    return 0;
  const long long M = (long long)d->N * d->Ho * d->Wo;
  if (M >= (1ll << 31)) return 0;
  const ConvArgs a = conv_args(*d);
  if (d->raw_src) {
    // one launch only: the images (12 B per pixel; 16 as the range split of conv_in_ranges counts the 8-channel bf16
    // view they stand for) and the output under 2 GiB, and none of the epilogue operands the stem does not have
    const long long lim = (1ll << 31) - (1ll << 20);
    if (d->residual || d->mul || d->out2 || (long long)d->N * d->H * d->W * 16 > lim ||
        M * d->o_cstride * 2 > lim)
      return 0;
    return conv_small_raw_applies(a) ? 1 : 0;
  }
  return d->px_scale ? (conv_pw_applies(a) ? 1 : 0) : (conv_hwc_fused_variant(a, hwc_r3_mode()) ? 1 : 0);
}

// ---------------------------------------------------------------------------------------- families
struct VariantRange {
  int lo = 1, hi = 0;   // inclusive; the default is empty
  bool has(int v) const { return lo <= v && v <= hi; }
};

struct ConvFamily {
  int path;   // HISEG_CONV_PATH_*
  int (*try_launch)(const ConvArgs&, hipStream_t, int);
  VariantRange owns[3];   // the forced variants routed to it (first row that owns the number)
};

// In routing order.  The numbers a family owns include the timing-only ones of a DIAG build; its *_try declines those
// it does not know.  conv_small catches every number from 50 up that no row before it owns.  0..49 are the ring
// kernel's own configurations (0 never arrives here: it is the automatic choice); a negative variant has no row and
// runs the generic kernel.
enum { F_ROWS, F_PW, F_HWR, F_HWC, F_HWT, F_HW, F_WIDE, F_FAST, F_SMALL, F_COUNT };
static const ConvFamily kFamilies[F_COUNT] = {
    {HISEG_CONV_PATH_ROWS, conv_rows_try, {{98, 98}}},
    {HISEG_CONV_PATH_PW, conv_pw_try, {{90, 90}, {190, 221}}},
    {HISEG_CONV_PATH_HWR, conv_hwr_try, {{92, 97}, {100, 101}, {110, 141}}},
    {HISEG_CONV_PATH_HWC, conv_hwc_try, {{102, 102}, {104, 109}, {150, 4299}}},
    {HISEG_CONV_PATH_HWT, conv_hwt_try, {{103, 103}}},
    {HISEG_CONV_PATH_HW, conv_hw_try, {{80, 89}}},
    {HISEG_CONV_PATH_WIDE, conv_wide_try, {{70, 79}}},
    {HISEG_CONV_PATH_FAST, conv_fast_try, {{60, 69}, {0, 49}}},
    {HISEG_CONV_PATH_SMALL, conv_small_try, {{50, INT_MAX}}},
};

static const ConvFamily* forced_family(int variant) {
  for (const ConvFamily& f : kFamilies)
    for (const VariantRange& r : f.owns)
      if (r.has(variant)) return &f;
  return nullptr;
}

struct ConvCandidate {
  const ConvFamily* family;
  int variant;
};
constexpr int kMaxCandidates = 16;

// Launches the candidate if its kernel takes the layer, and notes the path.  > 0: launched, 0: declined, < 0: error.
static int conv_take(const ConvCandidate& c, const ConvArgs& a, hipStream_t s) {
  const int r = c.family->try_launch(a, s, c.variant);
  if (r > 0) conv_note_path(c.family->path, c.variant);
  return r;
}

// The variants a release library accepts: the automatic choice, the generic kernel and every configuration
// tests/test_gpu_parity.py checks bit for bit.  Timing-only, stamp and experimental kernels exist only in a
// -DHISEG_DIAG build (Makefile DIAG=1).
static bool release_variant(int v) {
  return v == -1 || v == 0 || (v >= 1 && v <= 8) || v == 50 || v == 51 || v == 52 || v == 54 || v == 58 ||
         (v >= 60 && v <= 69) || v == 70 || v == 71 || v == 72 || v == 74 || v == 80 || v == 82 || v == 84 || v == 86 ||
         v == 88 || v == 89 || v == 90 || (v >= 92 && v <= 101) || v == 103 || v == 102 || (v >= 104 && v <= 109);
}

// ---------------------------------------------------------------------------------------- automatic choice
// Automatic choice (variant 0) = the fastest measured configuration per layer class (tools/conv_bench.py), as an
// ordered list: the first candidate whose kernel takes the layer runs it, and every kernel declines what it does not
// cover.  The order is the behaviour.  Returns the number of candidates written to c[kMaxCandidates].
static int auto_candidates(const ConvArgs& a, ConvCandidate* c) {
  const hiseg_conv2d_desc& d = a.d;
  int n = 0;
  auto add = [&](int family, int variant) { c[n++] = {&kFamilies[family], variant}; };
  // HISEG_CONV_WAVES=4 restores the 4-wave tiles (A/B timing only)
  static const bool four_waves = [] { const char* e = getenv("HISEG_CONV_WAVES"); return e && atoi(e) == 4; }();
  // HISEG_CONV_HALO=0 keeps the tap-major kernels (A/B timing only)
  static const bool halo = [] { const char* e = getenv("HISEG_CONV_HALO"); return !(e && atoi(e) == 0); }();
  // 1x1 layers and the ConvTranspose GEMM with 256-multiple GEMM columns: the persistent pointwise kernel
  // (conv_pw.hip, variant 90: weights resident in LDS, activations streamed into MFMA registers;
  // tools/conv_bench.py: 0.205 vs 0.308 ms on 256->256 @64x48 x256 ROIs, 0.21 vs 0.34 ms on the 256+8
  // combiner, 0.16 vs 0.24 ms on 128->256; bit-identical)
  if (d.KH == 1 && d.KW == 1) add(F_PW, 90);
  // narrow 3x3 layers (16 / 32 output channels: the full-image UNet's last decoder blocks and head): the
  // row-streaming kernel (conv_rows.hip, variant 98: weights in registers, input rows streamed through an LDS
  // ring; bit-identical to conv_small)
  if (d.KH == 3 && d.KW == 3 && d.Cout_pad <= 32) {
    add(F_ROWS, 98);
    // (sources far apart in memory: conv_rows takes them through one buffer resource each, VERDICT r3 weak #1.)
    // A layer of its form it still declines (an output alignment it does not store) takes conv_small, whose
    // accumulation order is conv_rows' (bit-identical)
    if (conv_rows_form(a)) add(F_SMALL, 0);
  }
  if (halo && !four_waves) {
    if (d.weight_frag != nullptr) {
      // 3x3 layers with weights also packed in MFMA fragment order (hiseg.ops.frag_pack) and 128-multiple Cout: the
      // register-streamed-weight halo kernel (conv_hwr.hip: one barrier per 32-channel slice) in its B-reuse,
      // MFMA-priority configuration (variant 97; tools/conv_bench.py, profiles/r3_conv_bench_hwr*.json: 0.732 vs
      // 0.793 ms (variant 86) on 256->256 @64x48 x256 ROIs, 0.879 vs 0.930 ms on 128->128 @128x96, 0.364 vs 0.408 ms
      // on 128->256; bit-identical to variant 86)
      // Round 5: the Cout-split form of the same kernel (conv_hwc.hip, variant 104: each wave 32 Cout x all 256 pixels
      // of the tile -- half the weight-fragment loads, each halo row's B fragment reused across the 3 ky taps;
      // tools/conv_bench.py, profiles/r5_conv_hwc.txt: 256->256 @64x48 x256 ROIs 0.736 -> 0.678 ms, 128->128 @128x96
      // 0.875 -> 0.799, 128->256 0.369 -> 0.345; bit-identical to variant 97 / 86)
      // Round 6: variant 108, the same kernel with a ring of three halo buffers (slice sl + 2's halo in flight during
      // slice sl; 72 KiB of LDS, two workgroups per CU): bit-identical, 256->256 @64x48 x256 ROIs 0.709 -> 0.701 ms,
      // 128->128 @128x96 0.829 -> 0.814, 128->256 0.364 -> 0.351 (tools/conv_bench.py, profiles/r6_conv_hwc_r3.txt)
      // Round 6: variants 109 / 102, multi-tile workgroups (conv_hwc_mt_kernel: the next tile's first halo slice lands
      // during the last slice, two-half epilogue; bit-identical; HISEG_CONV_HWC_MTW=0|1 overrides the default)
      const char* mtw = getenv("HISEG_CONV_HWC_MTW");
      if (d.Cout % 128 == 0) {
        if (hwc_mt_mode(mtw, 128)) add(F_HWC, 109);
        add(F_HWC, hwc_r3_mode() ? 108 : 104);
        add(F_HWR, 97);
      }
      // 64-multiple Cout (the EnhancedUNet's 64-channel layers, the smp decoder's 64-channel block): conv_hwc on
      // 64-Cout x 16 x 32-pixel tiles (variant 107, round 5), else conv_hwr's (variant 100).  (A 128-multiple Cout is
      // one too: these follow when all three above declined.)
      if (d.Cout % 64 == 0) {
        if (hwc64_mode()) {
          if (hwc_mt_mode(mtw, 64)) add(F_HWC, 102);
          add(F_HWC, 107);
        }
        add(F_HWR, 100);
      }
    }
    // 3x3 single-source layers with 128-multiple Cout: the halo-tiled kernel, BCO 128 with B-fragment reuse
    // across ky (conv_hw.hip, variant 86: two workgroups per CU; tools/conv_bench.py: 0.85 vs 1.02 ms (wide
    // kernel) on the 256->256 @64x48 x256 ROI class, 1.01 vs 1.37 ms on 128->128 @128x96, 0.44 vs 0.54 ms on
    // 128->256; channel-major K order, within bf16 rounding); 64-multiple Cout: its BCO-64 configuration (variant
    // 89: 0.104 vs 0.140 ms on the 64->64 residual class, 0.26 vs 0.43 ms on 256->64)
    // (BCO 64 for every Cout that is not a 128 multiple: full 64 tiles plus a partial last tile)
    add(F_HW, d.Cout % 128 ? 89 : 86);
  }
  // 256-output-channel 3x3 layers: the wide-tile kernel (conv_wide.hip: 256x256 workgroup tile, 128x128 wave
  // tiles, LDS epilogue; tools/conv_bench.py: 0.99 vs 1.23 ms on the 256->256 3x3 @64x48 x256 ROI class,
  // 0.58 vs 0.66 ms on 128->256, bit-identical).  It declines what it does not cover.
  if (d.Cout % 256 == 0 && d.KH * d.KW > 1 && !four_waves) add(F_WIDE, 70);
  // LDS-DMA ring kernel, 128x128 tiles for Cout >= 128, 64x128 for 64:
  // 61 = 128x128 ring, 8 waves as 4 (Cout) x 2 (pixel) with 32x64 wave tiles, LDS full-row epilogue;
  // 68 = the same wave grid on 64x128 tiles (tools/conv_bench.py: +1..4 % / +7..9 % over the 4-wave
  // 66 / 67, which had beaten the register epilogue by 4..17 %; all bit-identical)
  add(F_FAST, four_waves ? ((d.Cout_pad % 128 == 0) ? 66 : 67) : ((d.Cout_pad % 128 == 0) ? 61 : 68));
  add(F_SMALL, 0);   // narrow / ragged layers: halo-tiled direct kernel
  return n;
}

// ---------------------------------------------------------------------------------------- dispatch
// the generic kernel, noted as generic / generic split-K with the Cout tile it launched
static int launch_generic(const ConvArgs& a, hipStream_t s, int splits = 1) {
  int bco = 0;
  const int r = conv_generic_launch(a, s, splits, &bco);
  if (r == HISEG_OK) conv_note_path(splits > 1 ? HISEG_CONV_PATH_GENERIC_SPLITK : HISEG_CONV_PATH_GENERIC, bco);
  return r;
}

// One launch of a validated descriptor whose every operand spans < 2 GiB (conv_in_ranges).
static int conv_one_range(const hiseg_conv2d_desc* d, hipStream_t s, int variant) {
  const long long M = (long long)d->N * d->Ho * d->Wo;
  HISEG_REQUIRE(M < (1ll << 31), HISEG_ERR_BAD_SHAPE, "conv2d: too many pixels");
  ConvArgs a = conv_args(*d);
  // The fused operands of round 7 exist in one kernel each, and no other kernel may take the layer and silently
  // ignore them: the caller asks hiseg_conv2d_fused_ok first.
  if (d->raw_src) {   // the stem on the raw images: conv_small's staging form, a path of its own
    const int r = conv_small_try(a, s, 0);
    HISEG_REQUIRE(r != 0, HISEG_ERR_BAD_ARG, "conv2d: no kernel takes this layer with raw_src (hiseg_conv2d_fused_ok)");
    if (r > 0) conv_note_path(HISEG_CONV_PATH_STEM_RAW, 1);
    return r < 0 ? r : HISEG_OK;
  }
  if (has_fused_operands(d)) {
    const ConvCandidate fc = d->px_scale ? ConvCandidate{&kFamilies[F_PW], 90}
                                         : ConvCandidate{&kFamilies[F_HWC], variant ? variant : hwc_r3_mode() ? 108 : 104};
    const int r = conv_take(fc, a, s);
    HISEG_REQUIRE(r != 0, HISEG_ERR_BAD_ARG,
                  "conv2d: no kernel takes this layer with px_scale / head2_out / a_gate / res_gate "
                  "(hiseg_conv2d_fused_ok)");
    return r < 0 ? r : HISEG_OK;
  }
  if (variant == 99 || variant == 0) {
    // split-K generic kernel for small-grid, long-K 1x1 layers (variant 99 forces it when the plan splits)
    const int sp = splitk_plan(a);
    if (sp > 1 && d->workspace != nullptr && d->workspace_bytes >= splitk_bytes(a, sp) &&
        !(variant == 0 && conv_pw_applies(a))) {
      a.kper = (a.nK + sp - 1) / sp;
      return launch_generic(a, s, (a.nK + a.kper - 1) / a.kper);
    }
    HISEG_REQUIRE(variant == 0, HISEG_ERR_BAD_ARG, "conv2d: variant 99 (split-K) does not apply to this layer / workspace");
  }
  // the automatic choice's list, or the one family that owns a forced variant; whatever they decline, and a negative
  // variant, runs the generic kernel
  ConvCandidate cand[kMaxCandidates];
  int n = 0;
  if (variant == 0) {
    n = auto_candidates(a, cand);
  } else if (const ConvFamily* f = forced_family(variant)) {
    cand[n++] = {f, variant};
  }
  for (int i = 0; i < n; ++i) {
    const int r = conv_take(cand[i], a, s);
    if (r != 0) return r < 0 ? r : HISEG_OK;
  }
  return launch_generic(a, s);
}

// Operands of >= 2 GiB: the LDS-DMA kernels address through 32-bit buffer offsets, so the launch is split
// into image ranges whose every operand spans < 2 GiB (NHWC images are contiguous blocks; the conv never
// mixes images), each range a launch of its own on the same stream.
static int conv_in_ranges(const hiseg_conv2d_desc* d, hipStream_t s, int variant) {
  const long long ea = d->dtype == HISEG_BF16 ? 2 : 4, eo = d->out_dtype == HISEG_BF16 ? 2 : 4;
  const long long in_px = (long long)(d->H / d->a_up) * (d->W / d->a_up);
  const long long out_px = (long long)d->Ho * d->Wo * (d->convT ? 4 : 1);
  long long per = in_px * d->a_cstride * ea;
  auto upd = [&](long long v) { if (v > per) per = v; };
  if (d->srcB) upd((long long)d->H * d->W * d->b_cstride * ea);
  if (d->residual) upd(out_px * d->r_cstride * ea);
  if (d->mul) upd(out_px * d->m_cstride * ea);
  upd(out_px * d->o_cstride * eo);
  if (d->out2) upd(out_px * d->o2_cstride * ea);
  const long long lim = (1ll << 31) - (1ll << 20);
  int step = 0;
  if (per * d->N > lim) {
    HISEG_REQUIRE(per <= lim, HISEG_ERR_BAD_SHAPE, "conv2d: one image's operand exceeds 2 GiB");
    step = (int)(lim / per);
  }
  if (variant == 0 && d->in_scale && d->dtype == HISEG_BF16 && d->KH == 1 && d->KW == 1) {
    // an SE-gated 1x1 layer the pointwise kernel takes at up to `g` images per launch (its LDS gate table):
    // image ranges of g, whatever the batch (batch-invariant numerics, conv_pw_gate_images).  A range of <= g
    // images asks for no further split, so one level of ranges is all there is.
    const int g = conv_pw_gate_images(conv_args(*d));
    if (g > 0 && (step == 0 || g < step)) step = g;
  }
  if (step <= 0 || step >= d->N) return conv_one_range(d, s, variant);
  for (int n0 = 0; n0 < d->N; n0 += step) {
    hiseg_conv2d_desc c = *d;
    c.N = d->N - n0 < step ? d->N - n0 : step;
    auto at = [&](const void* p, long long bytes_per_image) {
      return p ? (const void*)((const char*)p + bytes_per_image * n0) : p;
    };
    c.srcA = at(d->srcA, in_px * d->a_cstride * ea);
    c.srcB = at(d->srcB, (long long)d->H * d->W * d->b_cstride * ea);
    c.residual = at(d->residual, out_px * d->r_cstride * ea);
    c.mul = at(d->mul, out_px * d->m_cstride * ea);
    c.out = const_cast<void*>(at(d->out, out_px * d->o_cstride * eo));
    c.out2 = const_cast<void*>(at(d->out2, out_px * d->o2_cstride * ea));
    if (d->in_scale) c.in_scale = d->in_scale + (long long)n0 * d->Ca;   // per-image SE gate [N][Ca]
    if (d->px_scale) c.px_scale = d->px_scale + n0 * in_px;              // per-pixel scale of source A
    if (d->head2_out) c.head2_out = d->head2_out + 2 * n0 * out_px;      // [pixels][2]
    if (d->a_gate) c.a_gate = d->a_gate + (long long)n0 * d->Ca;         // per-image channel gates [N][Ca]
    if (d->res_gate) c.res_gate = d->res_gate + (long long)n0 * d->Cout;   // [N][Cout]
    if (d->raw_src) c.raw_src = d->raw_src + 3 * n0 * in_px;             // f32 [N][3][H][W]
    const int r = conv_one_range(&c, s, variant);
    if (r) return r;
  }
  return HISEG_OK;
}

static int conv2d_impl(const hiseg_conv2d_desc* d, hiseg_stream_t stream, int variant) {
  HISEG_REQUIRE(d != nullptr, HISEG_ERR_BAD_ARG, "conv2d: null descriptor");
  HISEG_REQUIRE(d->dtype == HISEG_F32 || d->dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "conv2d: dtype %d", d->dtype);
  HISEG_REQUIRE(d->out_dtype == HISEG_F32 || d->out_dtype == HISEG_BF16, HISEG_ERR_BAD_DTYPE, "conv2d: out_dtype %d", d->out_dtype);
  HISEG_REQUIRE((d->srcA || d->raw_src) && d->weight && d->scale && d->shift && (d->out || d->head2_out),
                HISEG_ERR_BAD_ARG, "conv2d: null pointer");
#ifdef HISEG_DIAG
  const bool fused_variant = variant == 0 || (variant == 148 && d->a_gate);   // (148: the gated form, for timing)
#else
  const bool fused_variant = variant == 0;
#endif
  HISEG_REQUIRE(!has_fused_operands(d) ||
                    (fused_variant && !d->stats_partial && !d->bnb_partial && fused_operands_ok(d)),
                HISEG_ERR_BAD_ARG,
                "conv2d: px_scale / head2_out / a_gate / res_gate / raw_src go with the automatic choice alone: "
                "px_scale, a_gate or raw_src by itself, res_gate only beside head2_out");
  HISEG_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0, HISEG_ERR_BAD_SHAPE, "conv2d: empty grid");
  HISEG_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, HISEG_ERR_BAD_SHAPE, "conv2d: bad window");
  HISEG_REQUIRE(d->a_up == 1 || d->a_up == 2, HISEG_ERR_BAD_SHAPE, "conv2d: a_up must be 1 or 2");
  HISEG_REQUIRE(d->a_up == 1 || (d->H % 2 == 0 && d->W % 2 == 0), HISEG_ERR_BAD_SHAPE, "conv2d: upsampled grid must be even");
  HISEG_REQUIRE(d->Cb == 0 || d->srcB, HISEG_ERR_BAD_ARG, "conv2d: Cb > 0 needs srcB");
  HISEG_REQUIRE(d->Cout > 0 && d->Cout_pad >= d->Cout && d->Cout_pad % 16 == 0, HISEG_ERR_BAD_SHAPE,
                "conv2d: Cout %d Cout_pad %d (must be multiple of 16)", d->Cout, d->Cout_pad);
  const int kch = d->dtype == HISEG_BF16 ? 8 : 4;
  const int bk = 8 * kch;
  const int Cin = d->Ca + d->Cb;
  HISEG_REQUIRE(d->Ca > 0 && d->Ca % kch == 0 && d->Cb % kch == 0 && d->a_cstride % kch == 0 &&
                    d->a_coff % kch == 0 && (d->Cb == 0 || (d->b_cstride % kch == 0 && d->b_coff % kch == 0)),
                HISEG_ERR_BAD_SHAPE, "conv2d: input channels/strides must be multiples of %d", kch);
  HISEG_REQUIRE(d->K_pad % bk == 0 && d->K_pad >= d->KH * d->KW * Cin, HISEG_ERR_BAD_SHAPE,
                "conv2d: K_pad %d must be a multiple of %d and >= %d", d->K_pad, bk, d->KH * d->KW * Cin);
  HISEG_REQUIRE(al16(d->srcA) && al16(d->srcB) && al16(d->weight), HISEG_ERR_BAD_SHAPE, "conv2d: operands must be 16-B aligned");
  HISEG_REQUIRE(!d->convT || (d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->Cout % 16 == 0 &&
                              d->Ho == d->H && d->Wo == d->W),
                HISEG_ERR_BAD_SHAPE, "conv2d: convT requires a 1x1 GEMM with Cout = 4*C, C %% 4 == 0");
  hipStream_t s = (hipStream_t)stream;
  // BatchNorm statistics fused into the epilogue: only the halo kernel's fused-statistics form computes them, and no
  // fallback may silently skip them (the caller would finalize garbage)
  if (d->stats_partial || d->bnb_partial) {   // (also the fused BatchNorm-backward reduction of a data gradient)
    HISEG_REQUIRE(variant == 0 || variant == 104 || variant == 107, HISEG_ERR_BAD_ARG,
                  "conv2d: stats_partial / bnb_partial with variant %d", variant);
    HISEG_REQUIRE(al16(d->out) && al16(d->scale) && al16(d->shift), HISEG_ERR_BAD_SHAPE, "conv2d: alignment");
    // (>= 2^31 pixels: M reads 0 and conv_hwc_stats_tiles refuses the layer by its own pixel limit)
    const ConvArgs a = conv_args(*d);
    HISEG_REQUIRE(conv_hwc_stats_tiles(a) > 0, HISEG_ERR_BAD_ARG,
                  "conv2d: stats_partial / bnb_partial set but the layer has no fused kernel (hiseg_conv2d_stats_tiles)");
    const int r = conv_take({&kFamilies[F_HWC], d->Cout % 128 == 0 ? 104 : 107}, a, s);
    HISEG_REQUIRE(r != 0, HISEG_ERR_BAD_ARG, "conv2d: the fused-statistics kernel declined the layer");
    return r < 0 ? r : HISEG_OK;
  }
  return conv_in_ranges(d, s, variant);
}

// ---------------------------------------------------------------------------------------- fused ResidualBlock
// Two layers in one launch (conv_resblock.hip).  Not a candidate of the automatic choice: the caller holds both
// descriptors, asks hiseg_resblock_fused_ok and otherwise launches the layers one by one.
extern "C" int hiseg_resblock_fused_ok(const hiseg_conv2d_desc* d1, const hiseg_conv2d_desc* d2) {
  return d1 != nullptr && d2 != nullptr && conv_resblock_applies(*d1, *d2) ? 1 : 0;
}

extern "C" int hiseg_resblock_fwd(const hiseg_conv2d_desc* d1, const hiseg_conv2d_desc* d2, hiseg_stream_t stream) {
  HISEG_REQUIRE(d1 != nullptr && d2 != nullptr, HISEG_ERR_BAD_ARG, "resblock: null descriptor");
  HISEG_REQUIRE(conv_resblock_applies(*d1, *d2), HISEG_ERR_BAD_ARG,
                "resblock: the pair of layers has no fused kernel (hiseg_resblock_fused_ok)");
  const int r = conv_resblock_launch(*d1, *d2, (hipStream_t)stream);
  if (r == HISEG_OK) conv_note_path(HISEG_CONV_PATH_RESBLOCK, 1);
  return r;
}

extern "C" int hiseg_conv2d_fwd(const hiseg_conv2d_desc* d, hiseg_stream_t stream) {
  return conv2d_impl(d, stream, 0);
}

extern "C" int hiseg_conv2d_fwd_variant(const hiseg_conv2d_desc* d, int variant, hiseg_stream_t stream) {
#ifndef HISEG_DIAG
  HISEG_REQUIRE(release_variant(variant), HISEG_ERR_BAD_ARG,
                "conv2d: variant %d is not a release variant (diagnostic kernels need a DIAG=1 build)", variant);
#endif
  return conv2d_impl(d, stream, variant);
}
