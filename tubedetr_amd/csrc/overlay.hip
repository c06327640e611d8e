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
//     bytes else; one 16-byte store.  Only the first / last run of a tile's row, which it shares with the row padding or
//     with the neighbour tile, is loaded and stored by bytes - so the in-place case has no hazard: no lane reads or writes
//     a byte that another lane writes;
//   * the outline touches few runs: a run whose columns and rows miss it (two interval tests) skips the box layer, and with
//     no other layer on the frame its 16 bytes go from the load to the store untouched;
//   * the U and V rows of an I420 frame are walked together when their destination rows agree modulo 16 (the host checks:
//     any tightly packed frame whose chroma plane is a multiple of 16 bytes), and the two bytes of an NV12 pair share one
//     evaluation: a block's alphas are computed once for both components;
//   * the blend (v (256 - a) + c a + 128) >> 8 cannot leave [0, 255], so there is no clamp here and nothing for the
//     compiler to fuse into a packed shift-and-clamp (see shift_clamp_u8 in augment.hip before adding one).
// The table's pointers are loaded from memory: they are declared global so that loads and stores are global_*, not flat_*
// (which would also take the LDS path the tables need).
#include <algorithm>
#include <cmath>

#include "td_common.h"

namespace td {

namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 16;      // luma rows per workgroup (even)
constexpr int kMaxTileCols = 2048; // luma columns per workgroup (the column table's size)
constexpr int kMaxSide = 16384;    // (2 y + 1) * 256 * 128 stays below 2^30
constexpr int kMaxMap = 256;
constexpr int kRun = 16;           // bytes of a row per lane

#define TD_GLOBAL __attribute__((address_space(1)))
typedef const TD_GLOBAL unsigned char* gcbyte_ptr;
typedef TD_GLOBAL unsigned char* gbyte_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

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
// where column xl of the tile lives in the column table: the lanes of a wave read columns 16 apart (a luma run; 32 for an I420 chroma
// run), which would all fall into 4 (2) of the 64 LDS banks; one spare slot per 16 columns makes the lane stride 17 (34) dwords
__device__ __forceinline__ int col_slot(int xl) { return xl + (xl >> 4); }

// kind of a byte row
enum { kRgb = 0,      // 3 bytes per pixel
       kLuma = 1,     // 1 byte per pixel
       kChroma = 2,   // 1 byte per 2 x 2 block (I420: U, V, or both rows together)
       kPairs = 3 };  // 2 bytes per block (NV12)

__device__ __forceinline__ uint32_t blend(uint32_t v, uint32_t c, uint32_t a) { return (v * (256u - a) + c * a + 128u) >> 8; }

// g = clamp(((2 v + 1) m 128) / n - 128, 0, 256 (m - 1))
__device__ __forceinline__ int map_coord(int v, int m, int n) { return min(max(((2 * v + 1) * m * 128) / n - 128, 0), 256 * (m - 1)); }

__device__ __forceinline__ int round_coord(float v) { return (int)floorf(fminf(fmaxf(v, -1048576.f), 1048576.f) + 0.5f); }

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

// bytes [o0, o0 + 16) of a row, of which [v0, v1) belong to the tile: no other byte is touched
__device__ __forceinline__ void load_run(const unsigned char* rowp, int o0, int v0, int v1, uint32_t in[4]) {
  const unsigned char* a = rowp + o0;
  const bool full = v0 == o0 && v1 == o0 + kRun;
  if (full && ((uintptr_t)a & 15) == 0) {
    const u32x4 v = *(const TD_GLOBAL u32x4*)a;
    in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
  } else if (full && ((uintptr_t)a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = ((const TD_GLOBAL uint32_t*)a)[k];
  } else {
    in[0] = in[1] = in[2] = in[3] = 0;
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (o0 + j >= v0 && o0 + j < v1) in[j >> 2] |= (uint32_t)((gcbyte_ptr)a)[j] << (8 * (j & 3));
  }
}

// rowp + o0 is 16-byte aligned
__device__ __forceinline__ void store_run(unsigned char* rowp, int o0, int v0, int v1, const uint32_t out[4]) {
  unsigned char* a = rowp + o0;
  if (v0 == o0 && v1 == o0 + kRun) {
    u32x4 v;
    v.x = out[0]; v.y = out[1]; v.z = out[2]; v.w = out[3];
    *(TD_GLOBAL u32x4*)a = v;
  } else {
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (o0 + j >= v0 && o0 + j < v1) ((gbyte_ptr)a)[j] = (unsigned char)(out[j >> 2] >> (8 * (j & 3)));
  }
}

}  // namespace

__global__ __launch_bounds__(kThreads) void tube_overlay_kernel(const OverlayParams* __restrict__ tab, int n_jobs) {
  __shared__ uint32_t col[kMaxTileCols + kMaxTileCols / 16];
  __shared__ uint32_t row[kTileRows];
  __shared__ unsigned short vb[kTileRows * kMaxMap];
  const int tid = threadIdx.x, b = blockIdx.x;
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {  // last job whose first block is <= b (uniform: scalar loads)
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= b) lo = mid; else hi = mid - 1;
  }
  const OverlayParams p = tab[lo];
  int local = b - p.block_begin;
  const int tx = local % p.ntx; local /= p.ntx;
  const int ty = local % p.nty;
  const int t = local / p.nty;
  const int xb = tx * p.tile_w, xe = min(xb + p.tile_w, p.sw);  // the tile's luma columns and rows
  const int yb = ty * kTileRows, ye = min(yb + kTileRows, p.sh);

  // ---- what the frame asks for (uniform)
  const int r = p.frame_map ? ((const TD_GLOBAL int*)p.frame_map)[t] : t;
  const bool live = r >= 0 && r < p.n_tube;
  bool in_span = true;
  if (p.span) { const long long s0 = ((const TD_GLOBAL long long*)p.span)[0], s1 = ((const TD_GLOBAL long long*)p.span)[1]; in_span = r >= s0 && r <= s1; }
  Frame f;
  f.a_dim = (live && p.span && !in_span) ? (uint32_t)p.dim_alpha : 0u;
  f.heat_on = live && p.heat != nullptr;
  f.heat_alpha = p.heat_alpha; f.mw = p.mw; f.th = p.th;
  f.box_c = p.box_c; f.heat_c = p.heat_c; f.dim_c = p.dim_c;
  f.x0 = f.x1 = 0;
  int y0 = 0, y1 = 0;
  f.box_on = 0;
  if (live && p.boxes && in_span) {
    const TD_GLOBAL float* bx = (const TD_GLOBAL float*)p.boxes + 4 * (long long)r;
    const float c0 = bx[0], c1 = bx[1], c2 = bx[2], c3 = bx[3];
    if (isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3)) {
      f.x0 = round_coord(c0); y0 = round_coord(c1); f.x1 = round_coord(c2); y1 = round_coord(c3);
      f.box_on = f.x1 > f.x0 && y1 > y0;
    }
  }

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

namespace {

struct Plane { const unsigned char* p; long long bytes; };

size_t overlay_table_bytes(int n_jobs) { return (((size_t)n_jobs * sizeof(OverlayParams)) + 255) & ~(size_t)255; }

uint32_t pack3(const unsigned char c[3]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

}  // namespace

}  // namespace td

using namespace td;

extern "C" size_t td_tube_overlay_table_bytes(int n_jobs) { return n_jobs > 0 ? overlay_table_bytes(n_jobs) : 0; }

extern "C" int td_tube_overlay(const td_overlay_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_overlay";
  TD_REQUIRE(jobs && n_jobs > 0 && n_jobs <= 65536, "%s: no jobs (or more than 65536)", who);
  TD_REQUIRE(table_host && table_dev && table_bytes >= td_tube_overlay_table_bytes(n_jobs),
             "%s: job-table workspace missing or smaller than td_tube_overlay_table_bytes(%d)", who, n_jobs);
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
    const int n_planes = j.fmt == TD_SRC_RGB24 ? 1 : j.fmt == TD_SRC_NV12 ? 2 : 3;
    const int cw = (j.sw + 1) / 2, ch = (j.sh + 1) / 2;
    const int row_bytes[3] = {j.fmt == TD_SRC_RGB24 ? 3 * j.sw : j.sw, j.fmt == TD_SRC_NV12 ? 2 * cw : cw, cw};
    const int rows[3] = {j.sh, ch, ch};
    const void* sp[3] = {j.src0, j.src1, j.src2};
    void* dp[3] = {j.dst0, j.dst1, j.dst2};
    const int spitch[3] = {j.src_pitch0, j.src_pitch1, j.src_pitch2}, dpitch[3] = {j.dst_pitch0, j.dst_pitch1, j.dst_pitch2};
    for (int k = 0; k < n_planes; k++) {
      TD_REQUIRE(sp[k], "%s: job %d: src%d is null", who, i, k);
      TD_REQUIRE(dp[k], "%s: job %d: dst%d is null", who, i, k);
      TD_REQUIRE(spitch[k] >= row_bytes[k], "%s: job %d: src_pitch%d = %d is below its row of %d bytes", who, i, k, spitch[k], row_bytes[k]);
      TD_REQUIRE(dpitch[k] >= row_bytes[k], "%s: job %d: dst_pitch%d = %d is below its row of %d bytes", who, i, k, dpitch[k], row_bytes[k]);
      TD_REQUIRE(j.src_frame_stride >= (long long)spitch[k] * (rows[k] - 1) + row_bytes[k],
                 "%s: job %d: src_frame_stride %lld is smaller than plane %d needs (%d rows of pitch %d)", who, i, j.src_frame_stride, k, rows[k], spitch[k]);
      TD_REQUIRE(j.dst_frame_stride >= (long long)dpitch[k] * (rows[k] - 1) + row_bytes[k],
                 "%s: job %d: dst_frame_stride %lld is smaller than plane %d needs (%d rows of pitch %d)", who, i, j.dst_frame_stride, k, rows[k], dpitch[k]);
    }
    if (j.T == 0) continue;
    // a destination plane is its source plane, or touches no source plane (byte ranges from the first row of frame 0 to the last row of frame T - 1)
    Plane s[3], d[3];
    for (int k = 0; k < n_planes; k++) {
      s[k] = Plane{(const unsigned char*)sp[k], (long long)(j.T - 1) * j.src_frame_stride + (long long)spitch[k] * (rows[k] - 1) + row_bytes[k]};
      d[k] = Plane{(const unsigned char*)dp[k], (long long)(j.T - 1) * j.dst_frame_stride + (long long)dpitch[k] * (rows[k] - 1) + row_bytes[k]};
    }
    for (int k = 0; k < n_planes; k++) {
      if (dp[k] == sp[k] && dpitch[k] == spitch[k] && j.dst_frame_stride == j.src_frame_stride) continue;  // in place
      for (int m = 0; m < n_planes; m++)
        TD_REQUIRE(d[k].p + d[k].bytes <= s[m].p || s[m].p + s[m].bytes <= d[k].p,
                   "%s: job %d: dst%d overlaps src%d without being the same plane (pointer, pitch and frame stride)", who, i, k, m);
    }
    OverlayParams p{};
    for (int k = 0; k < n_planes; k++) {
      p.src[k] = (const unsigned char*)sp[k]; p.dst[k] = (unsigned char*)dp[k];
      p.spitch[k] = spitch[k]; p.dpitch[k] = dpitch[k];
    }
    p.sstride = j.src_frame_stride; p.dstride = j.dst_frame_stride;
    p.fmt = j.fmt; p.T = j.T; p.sh = j.sh; p.sw = j.sw;
    p.boxes = j.boxes; p.span = j.span; p.frame_map = j.frame_map; p.heat = j.heat;
    p.n_tube = j.n_tube; p.mh = j.mh; p.mw = j.mw; p.heat_alpha = j.heat_alpha; p.dim_alpha = j.dim_alpha;
    p.th = std::min(j.thickness, 1 << 22);  // fills every box the rounding can make; x0 + th stays in int32
    p.box_c = pack3(j.box_color); p.heat_c = pack3(j.heat_color); p.dim_c = pack3(j.dim_color);
    // U and V rows in one walk: every pair of destination rows (row y of frame t of both planes) has the same alignment
    p.joint = j.fmt == TD_SRC_I420 && (((uintptr_t)dp[1] ^ (uintptr_t)dp[2]) & (kRun - 1)) == 0 && ((dpitch[1] ^ dpitch[2]) & (kRun - 1)) == 0;
    p.ntx = cdiv(j.sw, kMaxTileCols);
    p.tile_w = (cdiv(j.sw, p.ntx) + 31) & ~31;  // equal tiles of whole 2 x 2 blocks; their chroma rows split at multiples of 16 bytes
    p.ntx = cdiv(j.sw, p.tile_w);
    p.nty = cdiv(j.sh, kTileRows);
    p.block_begin = (int)blocks;
    blocks += (long long)j.T * p.ntx * p.nty;
    TD_REQUIRE(blocks < (1LL << 31), "%s: too many workgroups", who);
    host[n++] = p;
  }
  if (n == 0) return TD_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(table_dev, host, (size_t)n * sizeof(OverlayParams), hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("%s: job table upload failed", who);
    return TD_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(tube_overlay_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, (const OverlayParams*)table_dev, n);
  return check_launch(who);
}
