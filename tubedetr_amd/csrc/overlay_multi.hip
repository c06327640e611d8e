// K labelled tubes and a moment timeline drawn into decoded frames in one pass: td_tube_overlay_multi (include/tubedetr_hip.h
// has the rule).
//
// The structure is td_tube_overlay's (overlay.hip): a workgroup owns a tile of kTileRows luma rows x tile_w luma columns of one
// frame and walks its byte rows, a lane owns an aligned run of 16 bytes (load_run / store_run), the heat layer's tables are
// built once per tile in LDS, and a run that no layer reaches goes from the load to the store untouched.  What is new is that a
// frame carries up to 4 K + 2 more layers - K outlines, K tag plates, K glyph layers, the timeline's bar, K segments and the
// cursor.  Every one of them is a RECTANGLE of one colour: the outline is a rectangle with a rectangular hole, a segment is a
// rectangle because "i(x) lies in the span" is an interval of columns, and all but the glyphs have one alpha.  So:
//   * per tile, ONCE: lane s of the first wave builds candidate layer s (its own box and span: the K loads run side by side),
//     drops it when it misses the tile, lies wholly in its hole or has alpha 0, and a ballot packs the survivors in rule order
//     into a layer list in LDS.  A 720p frame has 45 tiles; most hold none or a few of the layers;
//   * per run: the heat / dim pass of the overlay, then the list.  A layer costs a run two interval tests (its rectangle, its
//     hole) on a record that every lane reads from the same LDS address - a broadcast, no bank conflict - and only a run that it
//     reaches unpacks its 16 bytes.  The layers are applied one after the other to the run's bytes, which is the rule's order
//     for every byte; the run's registers are indexed by unrolled constants only (no scratch);
//   * a glyph layer reads its alpha bitmap from global memory (K x 32 x 256 bytes at most, shared by all frames: it lives in
//     the caches), only for pixels inside the plate; the division by tag_scale is a multiplication by a host-made reciprocal.
// The column table holds the heat layer's tap and fraction only, at the overlay's bank-spreading slots (col_slot).
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kTileRows = 16;      // luma rows per workgroup (even)
constexpr int kMaxTileCols = 2048; // luma columns per workgroup (the column table's size)
constexpr int kMaxMap = 256;
constexpr int kMaxTubes = 8;
constexpr int kMaxLayers = 4 * kMaxTubes + 2;
constexpr int kMaxTagH = 32, kMaxTagW = 256, kMaxTagScale = 8, kMaxLaneH = 64, kMaxTimelineRows = 1 << 20;

struct MultiParams {
  const unsigned char* src[3];
  unsigned char* dst[3];
  long long sstride, dstride;
  int spitch[3], dpitch[3];
  int fmt, T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  const unsigned char* heat;
  const unsigned char* tags;
  int n_tube, K, mh, mw, th, heat_alpha, dim_alpha;
  int tag_h, tag_w, tag_scale, tag_inv, tag_alpha;  // tag_inv = ceil(2^16 / tag_scale): d / tag_scale = (d tag_inv) >> 16 for d < 8192
  int lane_h, bar_alpha, seg_alpha;
  uint32_t tube_c[kMaxTubes], heat_c, dim_c, text_c, bar_c, cursor_c;  // byte k = component k
  int joint;                                                           // I420: the U and V destination rows agree modulo kRun
  int tile_w, ntx, nty, block_begin;
};

// a layer of the list: the pixels of [x0, x1) x [y0, y1) that are not in the hole [hx0, hx1) x [hy0, hy1) get alpha `a` - or, for
// a glyph layer (glyph >= 0: the offset of tube k's bitmap in `tags`), the bitmap's alpha at ((y - py0) / scale, (x - px0) / scale)
enum { kX0, kY0, kX1, kY1, kHx0, kHy0, kHx1, kHy1, kAlpha, kColor, kGlyph, kPx0, kPy0, kLayerInts = 16 };

// the slots of the candidate layers, in the rule's order: box k, then plate k and glyph k, then the bar, segment k, the cursor
constexpr int kSlotTag = kMaxTubes, kSlotBar = 3 * kMaxTubes, kSlotSeg = kSlotBar + 1, kSlotCursor = kSlotSeg + kMaxTubes;
static_assert(kSlotCursor + 1 == kMaxLayers && kMaxLayers <= 64, "one candidate per lane of the first wave");

struct Frame {  // what is uniform over a tile
  uint32_t a_dim;
  int heat_on, heat_alpha, mw, n_lay;
  uint32_t heat_c, dim_c;
};

// heat alpha of luma pixel (row rl, column xl) of the tile
__device__ __forceinline__ uint32_t heat_alpha_at(const Frame& f, const uint32_t* col, const unsigned short* vb, int rl, int xl) {
  const uint32_t ce = col[col_slot(xl)];
  const int ix = ce & 255, fx = (ce >> 8) & 255, ix1 = min(ix + 1, f.mw - 1);
  const unsigned short* v = vb + rl * f.mw;
  const uint32_t h = ((256u - fx) * v[ix] + (uint32_t)fx * v[ix1] + 32768u) >> 16;
  return (h * (uint32_t)f.heat_alpha + 127u) / 255u;
}

struct Layer {  // a list entry in registers
  int x0, y0, x1, y1, hx0, hy0, hx1, hy1, glyph, px0, py0;
  uint32_t a, c;
};

}  // namespace

__global__ __launch_bounds__(kThreads) void tube_overlay_multi_kernel(const MultiParams* __restrict__ tab, int n_jobs) {
  __shared__ uint32_t col[kMaxTileCols + kMaxTileCols / 16];
  __shared__ unsigned short vb[kTileRows * kMaxMap];
  __shared__ int lay[kMaxLayers][kLayerInts];
  __shared__ int frame_lds[2];  // the list's length, the dim layer's alpha
  const int tid = threadIdx.x, b = blockIdx.x;
  const MultiParams& p = tab[find_job(tab, n_jobs, b)];
  const int sh = p.sh, sw = p.sw, K = p.K, n_tube = p.n_tube;
  int local = b - p.block_begin;
  const int tx = local % p.ntx; local /= p.ntx;
  const int ty = local % p.nty;
  const int t = local / p.nty;
  const int xb = tx * p.tile_w, xe = min(xb + p.tile_w, sw);  // the tile's luma columns and rows
  const int yb = ty * kTileRows, ye = min(yb + kTileRows, sh);

  // ---- what the frame asks for
  const int r = tube_row(p.frame_map, t);
  const bool live = r >= 0 && r < n_tube;
  const gcbyte_ptr tags = (gcbyte_ptr)p.tags;
  const int tag_w = p.tag_w, tag_inv = p.tag_inv;

  // ---- the layer list (the first wave; every branch on tid < 64 is uniform over it)
  if (tid < 64) {
    const int s = tid;
    int e[kLayerInts];
#pragma unroll
    for (int i = 0; i < kLayerInts; i++) e[i] = 0;
    e[kGlyph] = -1;
    bool on = false, in_span = false;
    if (live && s < kMaxLayers) {
      const bool is_box = s < kSlotTag, is_tag = s >= kSlotTag && s < kSlotBar, is_seg = s >= kSlotSeg && s < kSlotCursor;
      const int k = is_box ? s : is_tag ? (s - kSlotTag) >> 1 : is_seg ? s - kSlotSeg : 0;
      if (k < K) {
        in_span = row_in_span(p.span, k, r);
        const int strip = sh - K * p.lane_h;  // the timeline's first row
        if (is_box || is_tag) {
          int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
          if (p.boxes && in_span && (is_box || tags) && rounded_box(p.boxes, (long long)r * K + k, x0, y0, x1, y1)) {
            on = true;
            if (is_box) {
              const int th = p.th;
              e[kX0] = x0; e[kY0] = y0; e[kX1] = x1; e[kY1] = y1;
              e[kHx0] = x0 + th; e[kHy0] = y0 + th; e[kHx1] = x1 - th; e[kHy1] = y1 - th;
              e[kAlpha] = 256; e[kColor] = (int)p.tube_c[k];
            } else {
              const int pw = tag_w * p.tag_scale, ph = p.tag_h * p.tag_scale, py0 = y0 - ph >= 0 ? y0 - ph : y0;
              e[kX0] = e[kPx0] = x0; e[kY0] = e[kPy0] = py0; e[kX1] = x0 + pw; e[kY1] = py0 + ph;
              if (s & 1) { e[kGlyph] = k * p.tag_h * tag_w; e[kAlpha] = 256; e[kColor] = (int)p.text_c; }  // (kSlotTag is even: odd slots are glyphs)
              else { e[kAlpha] = p.tag_alpha; e[kColor] = (int)p.tube_c[k]; }
            }
          }
        } else if (p.lane_h > 0) {
          on = true;
          e[kX0] = 0; e[kX1] = sw; e[kY0] = strip; e[kY1] = sh;
          if (s == kSlotBar) { e[kAlpha] = p.bar_alpha; e[kColor] = (int)p.bar_c; }
          else if (is_seg) {
            // i(x) = floor(x n_tube / sw) lies in [s0, s1]  <=>  x lies in [ceil(s0 sw / n_tube), ceil((s1 + 1) sw / n_tube))
            long long s0 = 0, s1 = n_tube - 1;
            if (p.span) {
              s0 = max(((const TD_GLOBAL long long*)p.span)[2 * k], 0LL);
              s1 = min(((const TD_GLOBAL long long*)p.span)[2 * k + 1], (long long)n_tube - 1);
            }
            on = s0 <= s1;
            e[kX0] = (int)((s0 * sw + n_tube - 1) / n_tube); e[kX1] = (int)(((s1 + 1) * sw + n_tube - 1) / n_tube);
            e[kY0] = sh - (K - k) * p.lane_h; e[kY1] = e[kY0] + p.lane_h;
            e[kAlpha] = p.seg_alpha; e[kColor] = (int)p.tube_c[k];
          } else {
            e[kX0] = (int)(((long long)r * sw) / n_tube); e[kX1] = max((int)(((long long)(r + 1) * sw) / n_tube), e[kX0] + 1);
            e[kAlpha] = 256; e[kColor] = (int)p.cursor_c;
          }
        }
      }
    }
    // dim: the span is given and r lies outside every tube's span (the box slots of the K tubes looked)
    const bool any_span = __ballot(in_span && s < kSlotTag) != 0ull;
    // the layer takes part in this tile: it meets it, the tile is not wholly inside its hole, and its alpha can change a byte
    on = on && e[kX0] < xe && e[kX1] > xb && e[kY0] < ye && e[kY1] > yb && !(xb >= e[kHx0] && xe <= e[kHx1] && yb >= e[kHy0] && ye <= e[kHy1]) &&
         (e[kAlpha] != 0 || e[kGlyph] >= 0);
    const unsigned long long mask = __ballot(on);
    if (on) {
      const int at = __popcll(mask & ((1ull << s) - 1ull));
#pragma unroll
      for (int i = 0; i < kLayerInts; i++) lay[at][i] = e[i];
    }
    if (s == 0) {
      frame_lds[0] = __popcll(mask);
      frame_lds[1] = (live && p.span && !any_span) ? p.dim_alpha : 0;
    }
  }

  // ---- the heat layer's tables
  Frame f;
  f.heat_on = live && p.heat != nullptr;
  f.heat_alpha = p.heat_alpha; f.mw = p.mw;
  f.heat_c = p.heat_c; f.dim_c = p.dim_c;
  if (f.heat_on) {
    for (int xl = tid; xl < xe - xb; xl += kThreads) {
      const int g = map_coord(xb + xl, p.mw, sw);
      col[col_slot(xl)] = (uint32_t)(g >> 8) | ((uint32_t)(g & 255) << 8);
    }
    gcbyte_ptr q = (gcbyte_ptr)p.heat + (long long)r * p.mh * p.mw;
    for (int i = tid; i < (ye - yb) * p.mw; i += kThreads) {
      const int rl = i / p.mw, j = i - rl * p.mw;
      const int g = map_coord(yb + rl, p.mh, sh), iy = g >> 8, fy = g & 255, iy1 = min(iy + 1, p.mh - 1);
      vb[rl * p.mw + j] = (unsigned short)((256 - fy) * (int)q[iy * p.mw + j] + fy * (int)q[iy1 * p.mw + j]);
    }
  }
  __syncthreads();
  f.n_lay = frame_lds[0];
  f.a_dim = (uint32_t)frame_lds[1];

  // alpha of luma pixel (y, x) under layer L
  auto alpha_at = [&](const Layer& L, int y, int x) -> uint32_t {
    if (!(x >= L.x0 && x < L.x1 && y >= L.y0 && y < L.y1) || (x >= L.hx0 && x < L.hx1 && y >= L.hy0 && y < L.hy1)) return 0u;
    if (L.glyph < 0) return L.a;
    const uint32_t m = tags[L.glyph + (((y - L.py0) * tag_inv) >> 16) * tag_w + (((x - L.px0) * tag_inv) >> 16)];
    return (256u * m + 127u) / 255u;
  };

  // ---- the byte rows of the tile.  n_rows rows from plane row y_first on, bytes [blo, bhi) of each; sb: the row of that plane is
  // walked with sa's (same bytes, same alignment of the destination); comp: the colour component of a kChroma row
  const long long soff = (long long)t * p.sstride, doff = (long long)t * p.dstride;
  auto walk = [&](const int kind, const int n_rows, const int y_first, const int blo, const int bhi, const unsigned char* sa, unsigned char* da, const int spa, const int dpa,
                  const int comp, const unsigned char* sb, unsigned char* db, const int spb, const int dpb) {
    const int len = bhi - blo;
    // runs per row: exact when every row of the plane has the alignment of the first, else the most a row can have
    const int n_run = (dpa & (kRun - 1)) ? (len + 2 * (kRun - 1)) / kRun : ((int)((uintptr_t)(da + doff + (long long)y_first * dpa + blo) & (kRun - 1)) + len + kRun - 1) / kRun;
    for (int idx = tid; idx < n_rows * n_run; idx += kThreads) {
      const int ri = idx / n_run, d = idx - ri * n_run, y = y_first + ri;
      const unsigned char* srow = sa + soff + (long long)y * spa;
      unsigned char* drow = da + doff + (long long)y * dpa;
      const int o0 = blo - (int)((uintptr_t)(drow + blo) & (kRun - 1)) + kRun * d;  // byte offset in the row of the run's first byte
      if (o0 >= bhi) continue;
      const int v0 = max(o0, blo), v1 = min(o0 + kRun, bhi);
      uint32_t out_a[4], out_b[4] = {0, 0, 0, 0};
      load_run(srow, o0, v0, v1, out_a);
      if (sb) load_run(sb + soff + (long long)y * spb, o0, v0, v1, out_b);

      // one layer over the run's bytes from offset o0 on; alpha(y, x): the layer's alpha of a luma pixel
      auto apply = [&](const int o0, const uint32_t c, auto alpha) {
        int last_cx = -1;
        uint32_t a = 0;
#pragma unroll
        for (int j = 0; j < kRun; j++) {
          const int o = min(max(o0 + j, blo), bhi - 1);  // a byte outside the tile computes its neighbour's value and is dropped
          int ch = comp;
          if (kind == kRgb || kind == kLuma) {
            int x = o;
            if (kind == kRgb) { x = o / 3; ch = o - 3 * x; }
            a = alpha(y, x);
          } else {
            int cx = o;
            if (kind == kPairs) { cx = o >> 1; ch = 1 + (o & 1); }
            if (cx != last_cx) {  // the mean over the luma pixels of the block that exist
              last_cx = cx;
              const int ly = 2 * y, lx = 2 * cx;
              const int ny = ly + 1 < sh ? 2 : 1, nx = lx + 1 < sw ? 2 : 1, lg = (ny - 1) + (nx - 1);  // n = ny nx = 1 << lg
              uint32_t sum = 0;
#pragma unroll
              for (int dy = 0; dy < 2; dy++)
#pragma unroll
                for (int dx = 0; dx < 2; dx++)
                  if (dy < ny && dx < nx) sum += alpha(ly + dy, lx + dx);
              a = (sum + ((1u << lg) >> 1)) >> lg;  // (sum + n / 2) / n
            }
          }
          // the byte is replaced where it stands (new - old, shifted, added modulo 2^32: no carry leaves the byte): no second set of registers
          const uint32_t va = (out_a[j >> 2] >> (8 * (j & 3))) & 255u;
          out_a[j >> 2] += (blend(va, (c >> (8 * ch)) & 255u, a) - va) << (8 * (j & 3));
          if (sb) {
            const uint32_t vc = (out_b[j >> 2] >> (8 * (j & 3))) & 255u;
            out_b[j >> 2] += (blend(vc, (c >> 16) & 255u, a) - vc) << (8 * (j & 3));
          }
        }
      };

      if (f.a_dim) apply(o0, f.dim_c, [&](int, int) { return f.a_dim; });
      if (f.heat_on) apply(o0, f.heat_c, [&](int ya, int xa) { return heat_alpha_at(f, col, vb, ya - yb, xa - xb); });
      if (f.n_lay) {
        // the run's luma columns [c_lo, c_hi) (a superset) and rows [r_lo, r_hi)
        int c_lo, c_hi, r_lo = y, r_hi = y + 1;
        if (kind == kRgb) { c_lo = v0 / 3; c_hi = (v1 - 1) / 3 + 1; }
        else if (kind == kLuma) { c_lo = v0; c_hi = v1; }
        else {
          if (kind == kChroma) { c_lo = 2 * v0; c_hi = 2 * v1; } else { c_lo = v0 & ~1; c_hi = (v1 + 1) & ~1; }
          r_lo = 2 * y; r_hi = 2 * y + 2;
        }
        for (int li = 0; li < f.n_lay; li++) {
          int e[kLayerInts];  // the record is the same for every lane: it goes to scalar registers
#pragma unroll
          for (int i = 0; i <= kPy0; i++) e[i] = __builtin_amdgcn_readfirstlane(lay[li][i]);
          // can the layer reach this run?  it meets the layer's rectangle and does not lie wholly in its hole
          if (!(c_lo < e[kX1] && c_hi > e[kX0] && r_lo < e[kY1] && r_hi > e[kY0])) continue;
          if (c_lo >= e[kHx0] && c_hi <= e[kHx1] && r_lo >= e[kHy0] && r_hi <= e[kHy1]) continue;
          Layer L;
          L.x0 = e[kX0]; L.y0 = e[kY0]; L.x1 = e[kX1]; L.y1 = e[kY1];
          L.hx0 = e[kHx0]; L.hy0 = e[kHy0]; L.hx1 = e[kHx1]; L.hy1 = e[kHy1];
          L.a = (uint32_t)e[kAlpha]; L.c = (uint32_t)e[kColor]; L.glyph = e[kGlyph]; L.px0 = e[kPx0]; L.py0 = e[kPy0];
          // the 16 bytes' coordinates do not depend on the layer: hoisted out of this loop they would occupy some 100 registers for
          // the whole walk (3 waves per SIMD instead of 5); an offset the compiler cannot see through keeps them inside
          int o0_here = o0;
          asm volatile("" : "+v"(o0_here));
          apply(o0_here, L.c, [&](int ya, int xa) { return alpha_at(L, ya, xa); });
        }
      }
      store_run(drow, o0, v0, v1, out_a);
      if (sb) store_run(db + doff + (long long)y * dpb, o0, v0, v1, out_b);
    }
  };

  const int cyb = yb >> 1, cye = (ye + 1) >> 1, cxb = xb >> 1, cxe = (xe + 1) >> 1;  // the tile's chroma rows and columns
  if (p.fmt == TD_SRC_RGB24) {
    walk(kRgb, ye - yb, yb, 3 * xb, 3 * xe, p.src[0], p.dst[0], p.spitch[0], p.dpitch[0], 0, nullptr, nullptr, 0, 0);
  } else {
    walk(kLuma, ye - yb, yb, xb, xe, p.src[0], p.dst[0], p.spitch[0], p.dpitch[0], 0, nullptr, nullptr, 0, 0);
    if (p.fmt == TD_SRC_NV12) {
      walk(kPairs, cye - cyb, cyb, 2 * cxb, 2 * cxe, p.src[1], p.dst[1], p.spitch[1], p.dpitch[1], 1, nullptr, nullptr, 0, 0);
    } else if (p.joint) {
      walk(kChroma, cye - cyb, cyb, cxb, cxe, p.src[1], p.dst[1], p.spitch[1], p.dpitch[1], 1, p.src[2], p.dst[2], p.spitch[2], p.dpitch[2]);
    } else {
      walk(kChroma, cye - cyb, cyb, cxb, cxe, p.src[1], p.dst[1], p.spitch[1], p.dpitch[1], 1, nullptr, nullptr, 0, 0);
      walk(kChroma, cye - cyb, cyb, cxb, cxe, p.src[2], p.dst[2], p.spitch[2], p.dpitch[2], 2, nullptr, nullptr, 0, 0);
    }
  }
}

}  // namespace td

using namespace td;

extern "C" size_t td_tube_overlay_multi_table_bytes(int n_jobs) { return table_bytes<MultiParams>(n_jobs); }

extern "C" int td_tube_overlay_multi(const td_overlay_multi_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_overlay_multi";
  if (int rc = check_workspace<MultiParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  MultiParams* host = (MultiParams*)table_host;
  int n = 0;
  long long blocks = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_overlay_multi_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSide, "%s: job %d: sh x sw = %d x %d outside 1..%d", who, i, j.sh, j.sw, kMaxSide);
    TD_REQUIRE(j.n_tube >= 0, "%s: job %d: negative n_tube %d", who, i, j.n_tube);
    TD_REQUIRE(j.K >= 1 && j.K <= kMaxTubes, "%s: job %d: K = %d outside 1..%d", who, i, j.K, kMaxTubes);
    TD_REQUIRE(!j.boxes || j.thickness >= 1, "%s: job %d: thickness %d is below 1", who, i, j.thickness);
    TD_REQUIRE(j.heat_alpha >= 0 && j.heat_alpha <= 256, "%s: job %d: heat_alpha %d outside [0, 256]", who, i, j.heat_alpha);
    TD_REQUIRE(j.dim_alpha >= 0 && j.dim_alpha <= 256, "%s: job %d: dim_alpha %d outside [0, 256]", who, i, j.dim_alpha);
    TD_REQUIRE(j.tag_alpha >= 0 && j.tag_alpha <= 256, "%s: job %d: tag_alpha %d outside [0, 256]", who, i, j.tag_alpha);
    TD_REQUIRE(j.bar_alpha >= 0 && j.bar_alpha <= 256, "%s: job %d: bar_alpha %d outside [0, 256]", who, i, j.bar_alpha);
    TD_REQUIRE(j.seg_alpha >= 0 && j.seg_alpha <= 256, "%s: job %d: seg_alpha %d outside [0, 256]", who, i, j.seg_alpha);
    TD_REQUIRE(!j.heat || (j.mh >= 1 && j.mw >= 1 && j.mh <= kMaxMap && j.mw <= kMaxMap), "%s: job %d: token grid mh x mw = %d x %d outside 1..%d", who, i, j.mh, j.mw, kMaxMap);
    if (j.tags) {
      TD_REQUIRE(j.boxes, "%s: job %d: tags without boxes", who, i);
      TD_REQUIRE(j.tag_h >= 1 && j.tag_h <= kMaxTagH, "%s: job %d: tag_h %d outside 1..%d", who, i, j.tag_h, kMaxTagH);
      TD_REQUIRE(j.tag_w >= 1 && j.tag_w <= kMaxTagW, "%s: job %d: tag_w %d outside 1..%d", who, i, j.tag_w, kMaxTagW);
      TD_REQUIRE(j.tag_scale >= 1 && j.tag_scale <= kMaxTagScale, "%s: job %d: tag_scale %d outside 1..%d", who, i, j.tag_scale, kMaxTagScale);
    }
    TD_REQUIRE(j.lane_h >= 0 && j.lane_h <= kMaxLaneH, "%s: job %d: lane_h %d outside 0..%d", who, i, j.lane_h, kMaxLaneH);
    if (j.lane_h > 0) {
      TD_REQUIRE(j.n_tube >= 1 && j.n_tube <= kMaxTimelineRows, "%s: job %d: a timeline (lane_h > 0) needs n_tube in 1..%d, not %d", who, i, kMaxTimelineRows, j.n_tube);
      TD_REQUIRE(j.K * j.lane_h <= j.sh, "%s: job %d: K lane_h = %d x %d rows do not fit sh = %d", who, i, j.K, j.lane_h, j.sh);
    }
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet sets[2] = {{"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride},
                              {"dst", {j.dst0, j.dst1, j.dst2}, {j.dst_pitch0, j.dst_pitch1, j.dst_pitch2}, j.dst_frame_stride}};
    const PlaneSet &sp = sets[0], &dp = sets[1];
    if (int rc = check_planes(who, i, g, sets, 2)) return rc;
    if (j.T == 0) continue;
    for (int k = 0; k < g.n_planes; k++)
      if (int rc = check_inplace_or_apart(who, i, g, sp, dp, j.T, k)) return rc;
    MultiParams p{};
    for (int k = 0; k < g.n_planes; k++) {
      p.src[k] = (const unsigned char*)sp.p[k]; p.dst[k] = (unsigned char*)dp.p[k];
      p.spitch[k] = sp.pitch[k]; p.dpitch[k] = dp.pitch[k];
    }
    p.sstride = j.src_frame_stride; p.dstride = j.dst_frame_stride;
    p.fmt = j.fmt; p.T = j.T; p.sh = j.sh; p.sw = j.sw;
    p.boxes = j.boxes; p.span = j.span; p.frame_map = j.frame_map; p.heat = j.heat; p.tags = j.tags;
    p.n_tube = j.n_tube; p.K = j.K; p.mh = j.mh; p.mw = j.mw; p.heat_alpha = j.heat_alpha; p.dim_alpha = j.dim_alpha;
    p.th = std::min(j.thickness, 1 << 22);  // fills every box the rounding can make; x0 + th stays in int32
    if (j.tags) {
      p.tag_h = j.tag_h; p.tag_w = j.tag_w; p.tag_scale = j.tag_scale; p.tag_alpha = j.tag_alpha;
      p.tag_inv = (65536 + j.tag_scale - 1) / j.tag_scale;  // exact for d < 65536 / 8: a plate is at most 256 x 8 = 2048 pixels wide
    }
    p.lane_h = j.lane_h; p.bar_alpha = j.bar_alpha; p.seg_alpha = j.seg_alpha;
    for (int k = 0; k < kMaxTubes; k++) p.tube_c[k] = pack3(j.tube_color[k]);
    p.heat_c = pack3(j.heat_color); p.dim_c = pack3(j.dim_color); p.text_c = pack3(j.tag_text_color); p.bar_c = pack3(j.bar_color); p.cursor_c = pack3(j.cursor_color);
    // U and V rows in one walk: every pair of destination rows (row y of frame t of both planes) has the same alignment
    p.joint = j.fmt == TD_SRC_I420 && (((uintptr_t)dp.p[1] ^ (uintptr_t)dp.p[2]) & (kRun - 1)) == 0 && ((dp.pitch[1] ^ dp.pitch[2]) & (kRun - 1)) == 0;
    p.ntx = cdiv(j.sw, kMaxTileCols);
    p.tile_w = (cdiv(j.sw, p.ntx) + 31) & ~31;  // equal tiles of whole 2 x 2 blocks; their chroma rows split at multiples of 16 bytes
    p.ntx = cdiv(j.sw, p.tile_w);
    p.nty = cdiv(j.sh, kTileRows);
    if (int rc = add_blocks(who, blocks, (long long)j.T * p.ntx * p.nty, p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_overlay_multi_kernel, blocks, 0, host, table_dev, n, stream, who);
}
