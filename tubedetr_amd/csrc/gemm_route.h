// Which kernel a td_conv_gemm / td_linear_ex call runs on: the route table of DESIGN.md as a pure function of the call's
// descriptor, the epilogue's flags, the dtype, the CU count and the dispatch knobs.  Host-only plain C++ - no HIP call, no
// getenv, no statics - so that the table is asserted on a machine without a GPU (tests/test_gemm_routes_cpu.py through
// td_conv_gemm_route / td_linear_ex_route).  gemm_conv.hip launches what these functions return (launch_route).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/tubedetr_hip.h"

#ifndef TD_REQUIRE  // built alone, without td_common.h: the three things this header takes from it
namespace td {
void set_error(const char* fmt, ...);
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
}  // namespace td
#define TD_REQUIRE(cond, ...)           \
  do {                                  \
    if (!(cond)) {                      \
      td::set_error(__VA_ARGS__);       \
      return TD_ERR_INVALID;            \
    }                                   \
  } while (0)
#endif

namespace td {

// the A/B knobs of the dispatch (table at the end of INTEGRATION.md), read from the environment once per process (gemm_knobs())
struct GemmKnobs {
  int pw_persist = 1;          // TD_PW_PERSIST (2: not with a ReLU mask; 3: forward geometry only)
  int pw_persist_min = 4;      // TD_PW_PERSIST_MIN
  int pw_persist_dropout = 1;  // TD_PW_PERSIST_DROPOUT (0 = dropout epilogues on the tiled kernel)
  int conv_tap_uniform = 1;    // TD_CONV_TAP_UNIFORM
  int conv_big = 1;            // TD_CONV_BIG
  int conv_big_min_wg = 160;   // TD_CONV_BIG_MIN_WG
  int conv_tap_inner = 1;      // TD_CONV_TAP_INNER
  int conv_big_persist = 1;    // TD_CONV_BIG_PERSIST (0 = one workgroup per tile)
  int conv_deep = 1;           // TD_CONV_DEEP
  int dgrad_s2_parity = 1;     // TD_DGRAD_S2_PARITY (0 = one gather over all 9 taps)
  int wgrad_blocks = 256, wgrad_wide = 1, wgrad_wide_min_m = 4096, wgrad_split_stages = 0;  // TD_WGRAD_* (wgrad_plan.h)
};

// a launch that uses a subset of the column blocks (filter taps) of a larger weight matrix
struct WeightSubset {
  int w_ld;          // row stride of the matrix in elements
  int ntap;          // taps of this launch, in its own (r', s') order
  int wtap[4];       // their tap indices in the matrix
  size_t w_bytes;    // addressable bytes from the pointer handed in
};

// what the planner reads of a td_epilogue (pointers only tested for null)
struct EpiFlags {
  bool res, msk, sigmoid, drop;
  float alpha;
};
inline EpiFlags epi_flags(const td_epilogue* e) {
  EpiFlags f = {false, false, false, false, 1.f};
  if (e) f = {e->residual != nullptr, e->mask_src != nullptr, e->sigmoid != 0, e->dropout_p > 0.f, e->alpha != 0.f ? e->alpha : 1.f};
  return f;
}

// one launch: the public record (kernel, family, tile, stages, walk, grid, block, the profiler's row) and what only the launcher needs
struct GemmRoute : td_gemm_route {
  bool res, msk;                            // template arguments of the persistent instance (both) and of conv_gemm_big8_kernel (res)
  int nkt, MTp, Pp;                         // persistent instance: K tiles, row tiles, workgroups per XCD
  int tap_inner;                            // 256-row tiles: GemmParams::tap_inner
  uint32_t src_bytes, src2_bytes, w_bytes;  // buffer-descriptor ranges of the operands
  double bytes;                             // the profiler's algorithmic HBM bytes, by the route's own formula
  const char* label;                        // check_launch's
};

inline int validate(const td_conv_desc* d, int dtype, const char* who) {
  const int vec = dtype == TD_BF16 ? 8 : 4;
  TD_REQUIRE(dtype == TD_F32 || dtype == TD_BF16, "%s: bad dtype %d", who, dtype);
  TD_REQUIRE(d->C % vec == 0, "%s: source channels C=%d must be a multiple of %d (pad them)", who, d->C, vec);
  TD_REQUIRE(d->N > 0 && d->Hs > 0 && d->Ws > 0 && d->Ho > 0 && d->Wo > 0 && d->R > 0 && d->S > 0 && d->stride > 0,
             "%s: bad geometry", who);
  TD_REQUIRE((double)d->N * d->Hs * d->Ws * d->C < 2147483647.0, "%s: source tensor exceeds 2^31 elements", who);
  TD_REQUIRE(!d->aniso || (d->mode == 0 && d->stride_w >= 1 && d->pad_w >= 0 && d->out_sp <= 1), "%s: anisotropic stride / padding is a forward-only geometry", who);
  return TD_OK;
}

// tile shape of the tiled kernel: 128x64 for <=64 output channels; 64x128 when 128x128 would leave the 256 CUs under-filled,
// and for the short-K, HBM-bound 1x1 layers (3 workgroups / CU: more loads in flight per CU)
inline void tiled_shape(GemmRoute& r) {
  const bool narrow = r.N <= 64;
  const int tiles128 = cdiv(r.M, 128) * cdiv(r.N, 128);
  const bool small_m = !narrow && (tiles128 < 512 || r.K <= 512);
  r.kernel = TD_GEMM_KERNEL_TILED;
  r.family = narrow ? TD_PROF_GEMM_128x64 : (small_m ? TD_PROF_GEMM_64x128 : TD_PROF_GEMM_128x128);
  r.bm = small_m ? 64 : 128;
  r.bn = narrow ? 64 : 128;
  r.stages = 2;
  r.grid = 8 * cdiv(cdiv(r.M, r.bm), 8) * cdiv(r.N, r.bn);
  r.block = 256;
}

// one td_conv_gemm launch (of the whole call, or of one parity class with its WeightSubset): first match wins
inline int plan_conv_launch(const td_conv_desc* d, const EpiFlags& f, int dtype, int n_cu, const GemmKnobs& kn, const WeightSubset* sub, GemmRoute& r) {
  int rc = validate(d, dtype, "td_conv_gemm");
  if (rc) return rc;
  memset(&r, 0, sizeof(r));
  const int M = d->N * d->Ho * d->Wo, K = d->R * d->S * d->C, out_sp = d->out_sp < 1 ? 1 : d->out_sp;
  const double es = dtype == TD_BF16 ? 2.0 : 4.0;
  const double src_elems = (double)d->N * d->Hs * d->Ws * d->C, sb = src_elems * es, wb = (double)d->Nc * K * es;
  TD_REQUIRE(sb < 4294967000.0 && wb < 4294967000.0, "td_conv_gemm: operand exceeds the 4 GiB buffer-descriptor range");
  TD_REQUIRE(d->ldc >= d->Nc, "td_conv_gemm: ldc < Nc");
  r.src_bytes = (uint32_t)sb;
  r.w_bytes = sub ? (uint32_t)sub->w_bytes : (uint32_t)wb;
  r.dtype = dtype; r.M = M; r.N = d->Nc; r.K = K; r.R = d->R; r.stride = d->stride; r.mode = d->mode;
  r.res = f.res;
  r.msk = f.msk;
  const bool use_wtap = sub && sub->ntap > 1;
  const double out_bytes = (double)M * d->Nc * es;
  {
    // persistent weight-stationary instance (see pw_resident2_kernel): bf16 pointwise layers with short K and many rows
    // dense rows, or the strided 1x1 of a downsample branch in forward geometry (the kernel derives the source pixel per row)
    const bool pw0 = d->R == 1 && d->S == 1 && d->pad == 0 && out_sp == 1 && !d->aniso &&
                     ((d->stride == 1 && d->Hs == d->Ho && d->Ws == d->Wo) ||
                      (d->stride > 1 && d->mode == 0 && (d->Ho - 1) * d->stride < d->Hs && (d->Wo - 1) * d->stride < d->Ws));
    const int NTp = d->Nc / 128, Pp = 2 * n_cu / 8;
    const bool shape_ok = pw0 && !sub && dtype == TD_BF16 && K % 64 == 0 && K <= 256 && d->Nc % 128 == 0 &&
                          (NTp == 1 || NTp == 2 || NTp == 4 || NTp == 8 || NTp == 16) && Pp >= NTp && d->ldc % 8 == 0 && !f.sigmoid &&
                          f.alpha == 1.f && n_cu % 8 == 0 && (!f.drop || kn.pw_persist_dropout) && (double)M * d->ldc < 2147483000.0;
    const int MTp = cdiv(M, 64);
    const int groups = shape_ok ? 8 * (Pp / NTp) : 1;
    if (kn.pw_persist && shape_ok && MTp >= kn.pw_persist_min * groups && !(kn.pw_persist == 2 && f.msk) && !(kn.pw_persist == 3 && d->mode != 0)) {
      r.kernel = TD_GEMM_KERNEL_PERSISTENT;
      r.family = TD_PROF_PW_RESIDENT;
      r.bm = 64; r.bn = 128;
      r.walk = TD_GEMM_WALK_POINTWISE;
      r.nkt = K / 64; r.MTp = MTp; r.Pp = Pp;
      r.grid = 2 * n_cu;  // two resident workgroups per CU (64 KiB of LDS each)
      r.block = 256;
      r.bytes = ((double)M * K + (double)d->Nc * K) * es + out_bytes * (1 + f.res + f.msk);
      r.label = "td_conv_gemm(pw_resident)";
      return TD_OK;
    }
  }
  const bool pw = d->R == 1 && d->S == 1 && d->stride == 1 && d->pad == 0 && out_sp == 1 && d->Hs == d->Ho && d->Ws == d->Wo;
  // tap-uniform addressing (see conv_gemm_kernel): spatial convs whose channel count is a multiple of the K tile
  // (a strided 1x1 - the downsample branch of a stage's first block - is the one-tap case of the same addressing)
  const int bk = dtype == TD_BF16 ? 64 : 32;
  const bool tu = (kn.conv_tap_uniform || use_wtap) && !pw && !d->aniso && (d->R * d->S > 1 || (d->stride > 1 && d->mode == 0)) && d->R * d->S <= 32 && d->C % bk == 0 &&
                  (out_sp == 1 || d->mode == 0) && (d->mode == 0 || d->stride == 1);
  // a tap -> column-block map (WeightSubset: the parity classes of a stride-2 input gradient) is honoured by the tap-uniform K walk only
  TD_REQUIRE(tu || !use_wtap, "td_conv_gemm: a weight-column subset needs the tap-uniform addressing (C %% %d == 0, at most 32 taps)", bk);
  r.walk = pw ? TD_GEMM_WALK_POINTWISE : (tu ? TD_GEMM_WALK_TAP_UNIFORM : TD_GEMM_WALK_GATHER);
  {
    // 256-row tiles (conv_gemm_big8_kernel / conv_gemm_big8n_kernel): MFMA-bound bf16 layers with enough workgroups to matter
    const int bnb = d->Nc % 256 == 0 ? 256 : 128;
    const int wgs = cdiv(M, 256) * (d->Nc / bnb);
    if (kn.conv_big && dtype == TD_BF16 && (pw || tu) && out_sp == 1 && !use_wtap && !sub && d->Nc % 128 == 0 && K % 64 == 0 && K >= 512 && d->ldc % 8 == 0 && !f.sigmoid &&
        !f.drop && wgs >= kn.conv_big_min_wg && (double)M * d->ldc < 2147483000.0 &&  // (rows past M leave through an out-of-range offset: the tensor must end below it)
        K <= 64 * 154 && M < (1 << 24)) {  // (the K table's 160 entries; rows decoded with float reciprocals.  Anything larger runs on 128 x 128 tiles)
      r.kernel = bnb == 256 ? TD_GEMM_KERNEL_BIG8 : TD_GEMM_KERNEL_BIG8N;
      r.family = tu ? TD_PROF_GEMM_256 : TD_PROF_GEMM_256_PW;
      r.bm = 256; r.bn = bnb;
      r.tap_inner = tu && kn.conv_tap_inner && d->R * d->S > 1;
      r.grid = 8 * cdiv(cdiv(M, 256), 8) * (d->Nc / bnb);
      if (bnb == 256 && kn.conv_big_persist && n_cu % 8 == 0 && (unsigned)n_cu < r.grid) r.grid = n_cu;  // 256 wide: persistent, one workgroup per CU
      r.block = 512;
      r.bytes = (src_elems + (double)d->Nc * K) * es + out_bytes * (1 + f.res + f.msk);
      r.label = "td_conv_gemm(256-row tiles)";
      return TD_OK;
    }
  }
  tiled_shape(r);
  // under-filled launch (at most two 64x128 workgroups per CU anyway) with a long K loop: the third stage costs nothing
  // in occupancy and halves the exposed DMA round trips
  if (dtype == TD_BF16 && kn.conv_deep && r.bm == 64 && (int)r.grid <= 2 * 256 && K >= 1024) r.stages = 3;  // measured: +6 % at K >= 1024, neutral-to-negative at K = 256
  // algorithmic HBM bytes: every operand / result tensor once (the gathered source counted as the tensor it is read from)
  const double rows_out = d->out_sp > 1 ? (double)d->N * d->out_H * d->out_W : (double)M;
  r.bytes = (src_elems + (double)d->Nc * K) * es + out_bytes + rows_out * d->Nc * es * (f.res + f.msk);
  r.label = "td_conv_gemm";
  return TD_OK;
}

// Input gradient of a 3x3 / stride 2 / pad 1 convolution (the second conv of a stage's first block), by output parity.  dx pixel
// (2a + ph, 2b + pw) only receives taps r with ph + 1 - r even: 1 tap per axis for an even coordinate, 2 for an odd one - 9 taps
// over 4 pixels.  Walked as ONE gather over all 9 taps per output pixel (the generic input-gradient path) three quarters of the
// MFMAs multiply zero rows: 4.0 ms per 16-clip step for the three such layers.  Here each parity class is a dense stride-1
// FORWARD-geometry convolution over g with a 1x1 / 1x2 / 2x1 / 2x2 filter whose taps are column blocks of the same w_dgrad matrix
// (no re-packed weights: the tap-uniform K walk takes a tap -> column-block map), written with output stride 2 at offset (ph, pw).
inline bool conv_splits_by_parity(const td_conv_desc* d, const td_epilogue* e, int dtype, const GemmKnobs& kn) {
  return kn.dgrad_s2_parity && dtype == TD_BF16 && d->mode == 1 && d->stride == 2 && d->R == 3 && d->S == 3 && d->pad == 1 && !d->aniso && d->out_sp <= 1 &&
         d->Ho == 2 * d->Hs && d->Wo == 2 * d->Ws && d->C % 64 == 0 && d->ldc >= d->Nc && !(e && (e->dropout_p > 0.f || e->sigmoid));
}
struct ParityClass {
  td_conv_desc d;
  WeightSubset sub;
  size_t w_off, out_off;  // byte offsets of the class's weight pointer, and of its output / residual / mask pointers
};
inline ParityClass parity_class(const td_conv_desc* d, int ph, int pw) {
  const int Hg = d->Hs, Wg = d->Ws, Co = d->C, H = d->Ho, W = d->Wo;
  const size_t es = 2, wbytes = (size_t)d->Nc * 9 * Co * es;
  // axis taps in the sub-filter's own order r' = 0, 1 (source offset + r'): even coordinate: r = 1; odd: r' = 0 <-> r = 2, r' = 1 <-> r = 0
  const int nr = ph ? 2 : 1, ns = pw ? 2 : 1;
  const int rmap[2] = {ph ? 2 : 1, 0}, smap[2] = {pw ? 2 : 1, 0};
  ParityClass c;
  memset(&c, 0, sizeof(c));
  c.d = {d->N, Hg, Wg, Co, Hg, Wg, nr, ns, 1, 0, 0, d->Nc, d->ldc, 2, H, W};
  c.sub.w_ld = 9 * Co;
  c.sub.ntap = nr * ns;
  for (int r = 0; r < nr; ++r)
    for (int s_ = 0; s_ < ns; ++s_) c.sub.wtap[r * ns + s_] = rmap[r] * 3 + smap[s_];
  c.out_off = ((size_t)ph * W + pw) * d->ldc * es;
  if (c.sub.ntap == 1) {  // one tap: its column block by pointer offset (a 1x1 launch has no tap walk)
    c.w_off = (size_t)c.sub.wtap[0] * Co * es;
    c.sub.wtap[0] = 0;
  }
  c.sub.w_bytes = wbytes - c.w_off;
  return c;
}

// td_linear_ex: the tiled kernel's GX instances on the same tile rule
inline int plan_linear_ex(const td_linear_ex_desc* x, bool has_a2, const EpiFlags& f, int dtype, GemmRoute& r) {
  TD_REQUIRE(dtype == TD_F32 || dtype == TD_BF16, "td_linear_ex: bad dtype %d", dtype);
  const int vec = dtype == TD_BF16 ? 8 : 4, bk = dtype == TD_BF16 ? 64 : 32;
  const int es = dtype == TD_BF16 ? 2 : 4;
  const int K2 = has_a2 ? x->K2 : 0;
  TD_REQUIRE(x->M >= 1 && x->N >= 1 && x->K1 >= vec && K2 >= 0, "td_linear_ex: bad sizes");
  TD_REQUIRE(x->K1 % vec == 0 && K2 % vec == 0 && x->lda1 % vec == 0 && (!has_a2 || x->lda2 % vec == 0), "td_linear_ex: K1 / K2 / lda must be multiples of %d", vec);
  TD_REQUIRE(!has_a2 || x->K1 % bk == 0, "td_linear_ex: with a second source K1=%d must be a multiple of the K tile (%d)", x->K1, bk);
  TD_REQUIRE(x->lda1 >= x->K1 && (!has_a2 || x->lda2 >= K2) && x->ldc >= x->N, "td_linear_ex: row stride smaller than the row");
  TD_REQUIRE(x->rows1 >= 1 && (!has_a2 || x->rows2 >= 1) && (x->a1_map || x->rows1 >= x->M) && (!has_a2 || x->a2_map || x->rows2 >= x->M),
             "td_linear_ex: source has fewer rows than M and no row map");
  const bool w_shared = has_a2 && x->w_shared;
  TD_REQUIRE(!w_shared || K2 == x->K1, "td_linear_ex: a shared weight needs K2 == K1");
  memset(&r, 0, sizeof(r));
  r.dtype = dtype; r.M = x->M; r.N = x->N; r.K = x->K1 + K2; r.R = 1; r.stride = 1; r.mode = 2;
  const double b1 = (double)x->rows1 * x->lda1 * es, b2 = has_a2 ? (double)x->rows2 * x->lda2 * es : 16.0, wb = (double)x->N * (w_shared ? x->K1 : r.K) * es;
  TD_REQUIRE(b1 < 4294967000.0 && b2 < 4294967000.0 && wb < 4294967000.0, "td_linear_ex: operand exceeds the 4 GiB buffer-descriptor range");
  r.src_bytes = (uint32_t)b1;
  r.src2_bytes = (uint32_t)b2;
  r.w_bytes = (uint32_t)wb;
  r.res = f.res;
  r.msk = f.msk;
  tiled_shape(r);
  r.walk = TD_GEMM_WALK_GX;
  r.bytes = ((double)r.M * r.K + (double)r.N * r.K + (double)r.M * r.N * (1 + f.res + f.msk)) * es;  // every gathered row counted once per use
  r.label = "td_linear_ex";
  return TD_OK;
}

}  // namespace td
