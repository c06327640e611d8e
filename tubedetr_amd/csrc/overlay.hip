// Grounded tubes drawn into decoded frames: td_tube_overlay (include/tubedetr_hip.h has the rule).
//
// Pure data movement: every source byte is read once, every destination byte written once.  The alpha of a layer is a
// function of the pixel's POSITION only (span, attention map, box), never of a pixel value, so the planes of a frame do not
// depend on each other: a workgroup owns a tile of kTileRows luma rows x tile_w luma columns of one frame (both even, so the
// tile owns whole 2 x 2 chroma blocks) and walks the byte rows of that tile - the Y rows, then the chroma rows under them.
// A chroma byte computes the mean alpha of its block from the same tables as the luma bytes; it has one writer.
//   * per tile, ONCE, into LDS: per column the map tap and fraction (the only integer division per column) and the two
//     box-column bits; per row the two box-row bits and, with a map, the row's VERTICALLY blended map row
//     vb[j] = (256 - fy) q[iy][j] + fy q[iy + 1][j] (the rule's h regrouped, exact: (256 - fx) vb[ix] + fx vb[ix + 1] is the
//     same integer as the header's form, below 2^24), so a luma byte costs one table dword, two 16-bit LDS reads and two multiplies;
//   * a lane owns an ALIGNED run of 16 bytes of a destination row (the rows of the tile are spread over the whole workgroup):
//     one 16-byte load when the source row has the same alignment (in place, equal pitches), 4 dwords when it agrees modulo 4,
//     bytes else; one 16-byte store (load_run / store_run in frame_jobs.h, which is also why the in-place case has no hazard);
//   * the outline touches few runs: a run whose columns and rows miss it (two interval tests) skips the box layer, and with
//     no other layer on the frame its 16 bytes go from the load to the store untouched;
//   * the U and V rows of an I420 frame are walked together when their destination rows agree modulo 16 (the host checks:
//     any tightly packed frame whose chroma plane is a multiple of 16 bytes), and the two bytes of an NV12 pair share one
//     evaluation: a block's alphas are computed once for both components;
//   * the blend (v (256 - a) + c a + 128) >> 8 cannot leave [0, 255], so there is no clamp here and nothing for the
//     compiler to fuse into a packed shift-and-clamp (see shift_clamp_u8 in resample_dev.h before adding one).
// The table's pointers are loaded from memory: they are declared global so that loads and stores are global_*, not flat_*
// (which would also take the LDS path the tables need).  The job search, the byte runs, the steps of the box rule, the blend and the
// heat layer's map coordinate (shared with overlay_multi.hip) and the host's plane checks and launch are the family's: frame_jobs.h.
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kTileRows = 16;      // luma rows per workgroup (even)
constexpr int kMaxTileCols = 2048; // luma columns per workgroup (the column table's size)
constexpr int kMaxMap = 256;

struct OverlayParams {
  const unsigned char* src[3];
  unsigned char* dst[3];
  long long sstride, dstride;
  int spitch[3], dpitch[3];
  int fmt, T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  const unsigned char* heat;
  int n_tube, mh, mw, th, heat_alpha, dim_alpha;
  uint32_t box_c, heat_c, dim_c;  // byte k = component k
  int joint;                      // I420: the U and V destination rows agree modulo kRun
  int tile_w, ntx, nty, block_begin;
};

// column entry: bits 0-7 map column ix, 8-15 fraction fx, 16 inside [x0, x1), 17 inside [x0 + th, x1 - th)
// row entry: bit 16, 17 alike for rows
constexpr uint32_t kOuter = 1u << 16, kInner = 1u << 17;
struct Frame {  // what is uniform over a tile
  uint32_t a_dim;
  int heat_on, box_on, heat_alpha, mw;
  int x0, x1, th;  // the box's columns (box_on)
  uint32_t box_c, heat_c, dim_c;
};

// heat and box alpha of luma pixel (row rl, column xl) of the tile; `boxed`: the box layer can reach this run
__device__ __forceinline__ void alphas(const Frame& f, const uint32_t* col, const uint32_t* row, const unsigned short* vb, bool boxed, int rl, int xl, uint32_t& a_heat,
                                       uint32_t& a_box) {
  a_heat = 0; a_box = 0;
  if (!f.heat_on && !boxed) return;
  const uint32_t ce = col[col_slot(xl)];
  if (f.heat_on) {
    const int ix = ce & 255, fx = (ce >> 8) & 255, ix1 = min(ix + 1, f.mw - 1);
    const unsigned short* v = vb + rl * f.mw;
    const uint32_t h = ((256u - fx) * v[ix] + (uint32_t)fx * v[ix1] + 32768u) >> 16;
    a_heat = (h * (uint32_t)f.heat_alpha + 127u) / 255u;
  }
  if (boxed) {
    const uint32_t both = ce & row[rl];
    a_box = ((both & kOuter) && !(both & kInner)) ? 256u : 0u;
  }
}

__device__ __forceinline__ uint32_t layers(const Frame& f, bool boxed, uint32_t v, int ch, uint32_t a_heat, uint32_t a_box) {
  if (f.a_dim) v = blend(v, (f.dim_c >> (8 * ch)) & 255u, f.a_dim);
  if (f.heat_on) v = blend(v, (f.heat_c >> (8 * ch)) & 255u, a_heat);
  if (boxed) v = blend(v, (f.box_c >> (8 * ch)) & 255u, a_box);
  return v;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void tube_overlay_kernel(const OverlayParams* __restrict__ tab, int n_jobs) {
  __shared__ uint32_t col[kMaxTileCols + kMaxTileCols / 16];
  __shared__ uint32_t row[kTileRows];
  __shared__ unsigned short vb[kTileRows * kMaxMap];
  const int tid = threadIdx.x, b = blockIdx.x;
  const OverlayParams p = tab[find_job(tab, n_jobs, b)];
  int local = b - p.block_begin;
  const int tx = local % p.ntx; local /= p.ntx;
  const int ty = local % p.nty;
  const int t = local / p.nty;
  const int xb = tx * p.tile_w, xe = min(xb + p.tile_w, p.sw);  // the tile's luma columns and rows
  const int yb = ty * kTileRows, ye = min(yb + kTileRows, p.sh);

  // ---- what the frame asks for (uniform)
  const int r = tube_row(p.frame_map, t);
  const bool live = r >= 0 && r < p.n_tube;
  const bool in_span = row_in_span(p.span, 0, r);
  Frame f;
  f.a_dim = (live && p.span && !in_span) ? (uint32_t)p.dim_alpha : 0u;
  f.heat_on = live && p.heat != nullptr;
  f.heat_alpha = p.heat_alpha; f.mw = p.mw; f.th = p.th;
  f.box_c = p.box_c; f.heat_c = p.heat_c; f.dim_c = p.dim_c;
  f.x0 = f.x1 = 0;
  int y0 = 0, y1 = 0;
  f.box_on = live && p.boxes && in_span && rounded_box(p.boxes, r, f.x0, y0, f.x1, y1);

  // ---- the tile's tables
  if (f.heat_on || f.box_on) {
    for (int xl = tid; xl < xe - xb; xl += kThreads) {
      const int x = xb + xl;
      uint32_t e = 0;
      if (f.heat_on) { const int g = map_coord(x, p.mw, p.sw); e = (uint32_t)(g >> 8) | ((uint32_t)(g & 255) << 8); }
      if (f.box_on) e |= (x >= f.x0 && x < f.x1 ? kOuter : 0u) | (x >= f.x0 + p.th && x < f.x1 - p.th ? kInner : 0u);
      col[col_slot(xl)] = e;
    }
    if (tid < ye - yb) {
      const int y = yb + tid;
      row[tid] = f.box_on ? ((y >= y0 && y < y1 ? kOuter : 0u) | (y >= y0 + p.th && y < y1 - p.th ? kInner : 0u)) : 0u;
    }
    if (f.heat_on) {
      gcbyte_ptr q = (gcbyte_ptr)p.heat + (long long)r * p.mh * p.mw;
      for (int i = tid; i < (ye - yb) * p.mw; i += kThreads) {
        const int rl = i / p.mw, j = i - rl * p.mw;
        const int g = map_coord(yb + rl, p.mh, p.sh), iy = g >> 8, fy = g & 255, iy1 = min(iy + 1, p.mh - 1);
        vb[rl * p.mw + j] = (unsigned short)((256 - fy) * (int)q[iy * p.mw + j] + fy * (int)q[iy1 * p.mw + j]);
      }
    }
  }
  __syncthreads();

  // ---- the byte rows of the tile.  n_rows rows from plane row y_first on, bytes [blo, bhi) of each; plane_b >= 0: the row of that
  // plane is walked with plane_a's (same bytes, same alignment of the destination); comp: the colour component of a kChroma row
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
      uint32_t in_a[4], in_b[4] = {0, 0, 0, 0};
      load_run(srow, o0, v0, v1, in_a);
      if (sb) load_run(sb + soff + (long long)y * spb, o0, v0, v1, in_b);
      // can the outline reach this run?  its luma columns [c_lo, c_hi) (a superset) and rows against the box: a row strictly between the
      // two horizontal bars meets only the two vertical bars
      bool boxed = false;
      if (f.box_on) {
        int c_lo, c_hi;
        uint32_t re0, re1 = 0;
        if (kind == kRgb) { c_lo = v0 / 3; c_hi = (v1 - 1) / 3 + 1; re0 = row[y - yb]; }
        else if (kind == kLuma) { c_lo = v0; c_hi = v1; re0 = row[y - yb]; }
        else {
          if (kind == kChroma) { c_lo = 2 * v0; c_hi = 2 * v1; } else { c_lo = v0 & ~1; c_hi = (v1 + 1) & ~1; }
          re0 = row[2 * y - yb];
          if (2 * y + 1 < ye) re1 = row[2 * y + 1 - yb];
        }
        const bool outer = (re0 | re1) & kOuter;
        const bool bar = ((re0 & kOuter) && !(re0 & kInner)) || ((re1 & kOuter) && !(re1 & kInner));
        boxed = outer && c_lo < f.x1 && c_hi > f.x0 && (bar || c_lo < f.x0 + f.th || c_hi > f.x1 - f.th);
      }
      uint32_t out_a[4] = {in_a[0], in_a[1], in_a[2], in_a[3]}, out_b[4] = {in_b[0], in_b[1], in_b[2], in_b[3]};
      if (f.a_dim || f.heat_on || boxed) {
        out_a[0] = out_a[1] = out_a[2] = out_a[3] = 0;
        out_b[0] = out_b[1] = out_b[2] = out_b[3] = 0;
        int last_cx = -1;
        uint32_t a_heat = 0, a_box = 0;
#pragma unroll
        for (int j = 0; j < kRun; j++) {
          const int o = min(max(o0 + j, blo), bhi - 1);  // a byte outside the tile computes its neighbour's value and is dropped
          const uint32_t va = (in_a[j >> 2] >> (8 * (j & 3))) & 255u;
          int ch = comp;
          if (kind == kRgb || kind == kLuma) {
            int x = o;
            if (kind == kRgb) { x = o / 3; ch = o - 3 * x; }
            alphas(f, col, row, vb, boxed, y - yb, x - xb, a_heat, a_box);
          } else {
            int cx = o;
            if (kind == kPairs) { cx = o >> 1; ch = 1 + (o & 1); }
            if (cx != last_cx) {  // the mean over the luma pixels of the block that exist
              last_cx = cx;
              const int ly = 2 * y, lx = 2 * cx;
              const int ny = ly + 1 < p.sh ? 2 : 1, nx = lx + 1 < p.sw ? 2 : 1, lg = (ny - 1) + (nx - 1);  // n = ny nx = 1 << lg
              uint32_t sum_h = 0, sum_b = 0;
#pragma unroll
              for (int dy = 0; dy < 2; dy++)
#pragma unroll
                for (int dx = 0; dx < 2; dx++)
                  if (dy < ny && dx < nx) {
                    uint32_t ah, ab;
                    alphas(f, col, row, vb, boxed, ly + dy - yb, lx + dx - xb, ah, ab);
                    sum_h += ah; sum_b += ab;
                  }
              a_heat = (sum_h + ((1u << lg) >> 1)) >> lg;  // (sum + n / 2) / n
              a_box = (sum_b + ((1u << lg) >> 1)) >> lg;
            }
          }
          out_a[j >> 2] |= layers(f, boxed, va, ch, a_heat, a_box) << (8 * (j & 3));
          if (sb) out_b[j >> 2] |= layers(f, boxed, (in_b[j >> 2] >> (8 * (j & 3))) & 255u, 2, a_heat, a_box) << (8 * (j & 3));
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

extern "C" size_t td_tube_overlay_table_bytes(int n_jobs) { return table_bytes<OverlayParams>(n_jobs); }

extern "C" int td_tube_overlay(const td_overlay_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_overlay";
  if (int rc = check_workspace<OverlayParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  OverlayParams* host = (OverlayParams*)table_host;
  int n = 0;
  long long blocks = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_overlay_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSide, "%s: job %d: sh x sw = %d x %d outside 1..%d", who, i, j.sh, j.sw, kMaxSide);
    TD_REQUIRE(j.n_tube >= 0, "%s: job %d: negative n_tube %d", who, i, j.n_tube);
    TD_REQUIRE(!j.boxes || j.thickness >= 1, "%s: job %d: thickness %d is below 1", who, i, j.thickness);
    TD_REQUIRE(j.heat_alpha >= 0 && j.heat_alpha <= 256, "%s: job %d: heat_alpha %d outside [0, 256]", who, i, j.heat_alpha);
    TD_REQUIRE(j.dim_alpha >= 0 && j.dim_alpha <= 256, "%s: job %d: dim_alpha %d outside [0, 256]", who, i, j.dim_alpha);
    TD_REQUIRE(!j.heat || (j.mh >= 1 && j.mw >= 1 && j.mh <= kMaxMap && j.mw <= kMaxMap), "%s: job %d: token grid mh x mw = %d x %d outside 1..%d", who, i, j.mh, j.mw, kMaxMap);
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet sets[2] = {{"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride},
                              {"dst", {j.dst0, j.dst1, j.dst2}, {j.dst_pitch0, j.dst_pitch1, j.dst_pitch2}, j.dst_frame_stride}};
    const PlaneSet &sp = sets[0], &dp = sets[1];
    if (int rc = check_planes(who, i, g, sets, 2)) return rc;
    if (j.T == 0) continue;
    for (int k = 0; k < g.n_planes; k++)
      if (int rc = check_inplace_or_apart(who, i, g, sp, dp, j.T, k)) return rc;
    OverlayParams p{};
    for (int k = 0; k < g.n_planes; k++) {
      p.src[k] = (const unsigned char*)sp.p[k]; p.dst[k] = (unsigned char*)dp.p[k];
      p.spitch[k] = sp.pitch[k]; p.dpitch[k] = dp.pitch[k];
    }
    p.sstride = j.src_frame_stride; p.dstride = j.dst_frame_stride;
    p.fmt = j.fmt; p.T = j.T; p.sh = j.sh; p.sw = j.sw;
    p.boxes = j.boxes; p.span = j.span; p.frame_map = j.frame_map; p.heat = j.heat;
    p.n_tube = j.n_tube; p.mh = j.mh; p.mw = j.mw; p.heat_alpha = j.heat_alpha; p.dim_alpha = j.dim_alpha;
    p.th = std::min(j.thickness, 1 << 22);  // fills every box the rounding can make; x0 + th stays in int32
    p.box_c = pack3(j.box_color); p.heat_c = pack3(j.heat_color); p.dim_c = pack3(j.dim_color);
    // U and V rows in one walk: every pair of destination rows (row y of frame t of both planes) has the same alignment
    p.joint = j.fmt == TD_SRC_I420 && (((uintptr_t)dp.p[1] ^ (uintptr_t)dp.p[2]) & (kRun - 1)) == 0 && ((dp.pitch[1] ^ dp.pitch[2]) & (kRun - 1)) == 0;
    p.ntx = cdiv(j.sw, kMaxTileCols);
    p.tile_w = (cdiv(j.sw, p.ntx) + 31) & ~31;  // equal tiles of whole 2 x 2 blocks; their chroma rows split at multiples of 16 bytes
    p.ntx = cdiv(j.sw, p.tile_w);
    p.nty = cdiv(j.sh, kTileRows);
    if (int rc = add_blocks(who, blocks, (long long)j.T * p.ntx * p.nty, p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_overlay_kernel, blocks, 0, host, table_dev, n, stream, who);
}
