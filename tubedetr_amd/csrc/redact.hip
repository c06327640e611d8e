// Grounded tubes redacted in decoded frames: td_tube_redact (include/tubedetr_hip.h has the rule).
//
// The selection of a byte is a function of its POSITION only (the frame's up-to-eight snapped rectangles, XOR invert), and the
// planes of a frame do not depend on each other, so a PLANE is the unit here: it has rows x cols samples of C interleaved
// channels (rgb24: 3; the UV plane of NV12: 2; else 1), and sample (i, j) asks luma pixel (s i, s j), s = 1 or 2.  A
// workgroup owns a tile of one plane of one frame:
//   FILL    64 rows x 1024 samples;
//   MOSAIC  whole cells: 1 to 8 cell rows (64 rows where 8 or fewer make them) x max(1, 256 / cp) cells, cp = the plane's cell
//           side (cp = 1, the chroma of cell 2, is the identity: a copy);
//   BLUR    64 rows x (256 - 2 rp) samples, rp = the plane's radius: the 256 lanes are the tile's columns plus the halo.
//   * per tile, ONCE: lanes 0..7 evaluate the frame's rectangles (steps 1 - 6 of the rule) into LDS; every lane then builds the
//     tile's column and row bit tables from them (bit k: inside rectangle k), so a byte's selection is one AND;
//   * a tile that no rectangle reaches (and invert = 0) is a copy, and IN PLACE its workgroup returns without touching memory;
//   * the write is td_tube_overlay's (load_run / store_run in frame_jobs.h): a lane owns an ALIGNED run of 16 bytes of a
//     destination row, loaded with one 16-byte load when the source row has the same alignment, 4 dwords when it agrees modulo 4,
//     bytes else; only the first / last run of a tile's row is handled by bytes, so no lane reads or writes a byte that another
//     workgroup writes.  Two interval tests per
//     rectangle that reaches the row say whether a run lies inside one (selected throughout) or outside all (not at all); only a
//     run that straddles an edge asks the tables byte by byte.  A run without a selected byte goes from the load to the store
//     untouched; in place it is not touched at all; a FILL run selected throughout is not loaded;
//   * MOSAIC needs no pixel storage: a lane walks one byte column of the tile's selected cells downwards (coalesced across the
//     lanes, the loads of a column independent of each other) and leaves a 16-bit sum per cell row; then one lane per (cell,
//     channel) adds cp column sums and divides; the write takes the constant from an LDS table, once per run when the run lies
//     in one cell.  All reads of a tile come before its first write (a barrier), and a tile is whole cells: in place is safe;
//   * BLUR keeps, per lane, the sum of its column over rows [y - rp, y + rp] and slides it down the tile (one sample added, one
//     subtracted per output row, loaded a batch of 4 rows ahead); the horizontal window is a difference of two entries of the
//     row's prefix sum over the 256 lanes (wave scans joined through LDS; the 4 rows x C channels of a batch are independent
//     chains between one set of barriers), so neither direction costs more at a larger radius, except for the halo.  Batches
//     of the tile that no rectangle reaches skip all of it and are copied.
// No atomics, no scratch; everything is plain C++ and vector stores.  The table's pointers are loaded from memory: they are
// declared global so that loads and stores are global_*, not flat_*.  Steps 1 - 5 of the rule, the job search, the byte runs and
// the host's plane checks and launch are the family's: frame_jobs.h.
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kMaxRects = 8;
constexpr int kCols = 256;          // samples per tile row: MOSAIC, BLUR (with the halo)
constexpr int kFillRows = 64, kFillCols = 1024;
constexpr int kBlurRows = 64, kBlurBatch = 4;
constexpr int kMosaicCellRows = 8;  // cell rows per MOSAIC tile, at most
constexpr int kMaxTileRows = 256;   // one cell row of cell 256
constexpr int kValBytes = kMosaicCellRows * 128 * 3;  // cp >= 2: at most 128 cells per cell row, 3 channels

struct RedactParams {
  const unsigned char* src[3];
  unsigned char* dst[3];
  long long sstride, dstride;
  int spitch[3], dpitch[3];
  int fmt, T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  int n_tube, K, mode, invert, margin_num, margin_den, cell, radius;
  uint32_t color;  // byte k = component k
  int n_planes;
  int inplace[3];
  int tw[3], th[3], ntx[3], nty[3];  // per plane: tile columns (BLUR: without the halo) and rows, tiles per row and per column
  int pbegin[3];                     // first workgroup of the plane within the job
  int block_begin;
};

union ModeTables {
  struct {
    unsigned short colsum[kMosaicCellRows * 3 * kCols];  // [cell row][byte column] summed over the cell's rows
    unsigned char val[kValBytes];                         // [cell row][cell][channel]
  } mosaic;
  struct {
    uint32_t pre[kBlurBatch][3][kCols];        // per row of the batch and channel, prefix sums of the lanes' column sums
    unsigned char stage[kBlurBatch][3 * kCols];  // the blurred bytes of the batch's rows of the tile
  } blur;
};

enum { kCopy = 0, kFill = 1, kMosaic = 2, kBlur = 3 };  // where a selected byte's value comes from

}  // namespace

__global__ __launch_bounds__(kThreads) void tube_redact_kernel(const RedactParams* __restrict__ tab, int n_jobs) {
  __shared__ int rect[kMaxRects][4];               // X0, X1, Y0, Y1 in luma pixels; an absent rectangle is all zeros
  __shared__ unsigned char colbits[kFillCols];     // bit k: the sample's column is inside rectangle k
  __shared__ unsigned char rowbits[kMaxTileRows];
  __shared__ unsigned char colcell[kCols];         // MOSAIC: the cell (within the tile) of a sample column
  __shared__ ModeTables tables;                    // MOSAIC and BLUR never meet in a workgroup: their tables share the space
  __shared__ uint32_t wtot[kBlurBatch][kThreads / 64][3];
  __shared__ unsigned char batch_on[kBlurRows / kBlurBatch];
  auto& colsum = tables.mosaic.colsum;
  auto& val = tables.mosaic.val;
  auto& pre = tables.blur.pre;
  auto& stage = tables.blur.stage;
  const int tid = threadIdx.x, b = blockIdx.x;
  const RedactParams* p = tab + find_job(tab, n_jobs, b);
  int local = b - p->block_begin;
  int pl = 0;
  if (p->n_planes > 1 && local >= p->pbegin[1]) pl = 1;
  if (p->n_planes > 2 && local >= p->pbegin[2]) pl = 2;
  local -= p->pbegin[pl];
  const int ntx = p->ntx[pl], nty = p->nty[pl], tw = p->tw[pl], th = p->th[pl];
  const int tx = local % ntx; local /= ntx;
  const int ty = local % nty;
  const int t = local / nty;
  const int fmt = p->fmt, mode = p->mode, inv = p->invert, sh = p->sh, sw = p->sw;
  const int s = pl ? 2 : 1;                                              // luma pixels per sample
  const int rows = pl ? (sh + 1) >> 1 : sh, cols = pl ? (sw + 1) >> 1 : sw;
  const int C = fmt == TD_SRC_RGB24 ? 3 : (fmt == TD_SRC_NV12 && pl) ? 2 : 1;
  const int par = mode == TD_REDACT_MOSAIC ? (pl ? p->cell >> 1 : p->cell) : (pl ? (p->radius + 1) >> 1 : p->radius);  // cp or rp
  const bool inplace = p->inplace[pl] != 0;
  const uint32_t color = p->color;
  const int xb = tx * tw, xe = min(xb + tw, cols);  // the tile's samples
  const int yb = ty * th, ye = min(yb + th, rows);

  // ---- the frame's rectangles (steps 1 - 6), one per lane
  const int r = tube_row(p->frame_map, t);
  if (tid < kMaxRects) {
    int X0 = 0, X1 = 0, Y0 = 0, Y1 = 0;
    int x0, y0, x1, y1, wx0, wy0, cw, ch;
    if (tid < p->K && r >= 0 && r < p->n_tube && row_in_span(p->span, tid, r) && rounded_box(p->boxes, (long long)r * p->K + tid, x0, y0, x1, y1) &&
        grow_and_clamp(x0, y0, x1, y1, p->margin_num, p->margin_den, sh, sw, wx0, wy0, cw, ch)) {
      const int wx1 = wx0 + cw, wy1 = wy0 + ch;
      if (mode == TD_REDACT_MOSAIC) {  // step 6: whole cells, whole 2 x 2 blocks
        const int cell = p->cell;
        X0 = (wx0 / cell) * cell; X1 = min(((wx1 + cell - 1) / cell) * cell, sw);
        Y0 = (wy0 / cell) * cell; Y1 = min(((wy1 + cell - 1) / cell) * cell, sh);
      } else {
        X0 = wx0 & ~1; X1 = min(wx1 + (wx1 & 1), sw);
        Y0 = wy0 & ~1; Y1 = min(wy1 + (wy1 & 1), sh);
      }
    }
    rect[tid][0] = X0; rect[tid][1] = X1; rect[tid][2] = Y0; rect[tid][3] = Y1;
  }
  __syncthreads();

  // ---- which rectangles can reach the tile's columns / rows (supersets), and what the tile has to do
  uint32_t kcols = 0, krows = 0;
#pragma unroll
  for (int k = 0; k < kMaxRects; k++) {
    const int X0 = rect[k][0], X1 = rect[k][1], Y0 = rect[k][2], Y1 = rect[k][3];
    if (X1 > X0) {
      if (s * xb < X1 && s * (xe - 1) >= X0) kcols |= 1u << k;
      if (s * yb < Y1 && s * (ye - 1) >= Y0) krows |= 1u << k;
    }
  }
  int vmode = mode == TD_REDACT_FILL ? kFill : mode == TD_REDACT_MOSAIC ? kMosaic : kBlur;
  if (!(inv || (kcols & krows)) || (mode == TD_REDACT_MOSAIC && par == 1)) vmode = kCopy;
  if (vmode == kCopy && inplace) return;  // uniform
  if (vmode != kCopy) {
    for (int xl = tid; xl < xe - xb; xl += kThreads) {
      const int lx = s * (xb + xl);
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < kMaxRects; k++) bits |= (lx >= rect[k][0] && lx < rect[k][1]) ? 1u << k : 0u;
      colbits[xl] = (unsigned char)bits;
      if (vmode == kMosaic) colcell[xl] = (unsigned char)(xl / par);
    }
    for (int yl = tid; yl < ye - yb; yl += kThreads) {
      const int ly = s * (yb + yl);
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < kMaxRects; k++) bits |= (ly >= rect[k][2] && ly < rect[k][3]) ? 1u << k : 0u;
      rowbits[yl] = (unsigned char)bits;
    }
  }
  __syncthreads();

  const unsigned char* splane = p->src[pl] + (long long)t * p->sstride;
  unsigned char* dplane = p->dst[pl] + (long long)t * p->dstride;
  const int sp = p->spitch[pl], dp = p->dpitch[pl];
  const int blo = C * xb, bhi = C * xe, len = bhi - blo;  // the tile's bytes of a row
  const int ncc = vmode == kMosaic ? (xe - xb + par - 1) / par : 0;  // cells per cell row of the tile

  // ---- rows [y_first, y_first + n_rows) of the tile.  quiet_only: skip the rows that a rectangle reaches (BLUR writes them one by one)
  auto write_rows = [&](const int y_first, const int n_rows, const bool quiet_only) {
    // runs per row: exact when every row of the plane has the alignment of the first, else the most a row can have
    const int n_run = (dp & (kRun - 1)) ? (len + 2 * (kRun - 1)) / kRun : ((int)((uintptr_t)(dplane + (long long)y_first * dp + blo) & (kRun - 1)) + len + kRun - 1) / kRun;
    for (int idx = tid; idx < n_rows * n_run; idx += kThreads) {
      const int ri = idx / n_run, d = idx - ri * n_run, y = y_first + ri;
      const uint32_t rb = vmode == kCopy ? 0u : rowbits[y - yb];
      if (quiet_only && batch_on[(y - yb) / kBlurBatch]) continue;
      const unsigned char* srow = splane + (long long)y * sp;
      unsigned char* drow = dplane + (long long)y * dp;
      const int o0 = blo - (int)((uintptr_t)(drow + blo) & (kRun - 1)) + kRun * d;  // byte offset in the row of the run's first byte
      if (o0 >= bhi) continue;
      const int v0 = max(o0, blo), v1 = min(o0 + kRun, bhi);
      const uint32_t valid = (0xffffu >> (o0 + kRun - v1)) & (0xffffu << (v0 - o0));  // bit j: byte o0 + j belongs to the tile
      uint32_t m = 0;                                                                  // bit j: byte o0 + j is selected
      if (vmode != kCopy) {
        // the run against the columns of the rectangles that reach this row: inside one of them, outside all of them, or mixed
        const int l_lo = s * (C == 3 ? v0 / 3 : v0 >> (C - 1)), l_hi = s * (C == 3 ? (v1 - 1) / 3 : (v1 - 1) >> (C - 1));  // first and last luma column asked
        bool all = false, some = false;
        for (uint32_t act = rb & kcols; act; act &= act - 1) {
          const int k = __ffs(act) - 1;
          const int X0 = rect[k][0], X1 = rect[k][1];
          if (l_lo >= X0 && l_hi < X1) all = true;
          else if (l_hi >= X0 && l_lo < X1) some = true;
        }
        if (all || !some) {
          m = (all != (inv != 0)) ? valid : 0u;
        } else {
#pragma unroll
          for (int j = 0; j < kRun; j++) {
            const int o = o0 + j;
            if (o >= v0 && o < v1) {
              const int x = C == 3 ? o / 3 : o >> (C - 1);
              if ((((uint32_t)colbits[x - xb] & rb) != 0) != (inv != 0)) m |= 1u << j;
            }
          }
        }
      }
      if (m == 0 && inplace) continue;
      uint32_t in[4] = {0, 0, 0, 0};
      if (!(vmode == kFill && m == valid)) load_run(srow, o0, v0, v1, in);
      uint32_t out[4] = {in[0], in[1], in[2], in[3]};
      if (m) {
        const int crow = vmode == kMosaic ? ((y - yb) / par) * ncc : 0;
        // one value per channel for the whole run (FILL; MOSAIC when its selected bytes lie in one cell): byte c of `vals`
        bool uniform = vmode == kFill;
        uint32_t vals = color >> (8 * pl);
        if (vmode == kMosaic) {
          const int of = o0 + __ffs(m) - 1, ol = o0 + 31 - __clz(m);
          const int cf = colcell[(C == 3 ? of / 3 : of >> (C - 1)) - xb], cl = colcell[(C == 3 ? ol / 3 : ol >> (C - 1)) - xb];
          uniform = cf == cl;
          if (uniform) {
            const int vi = (crow + cf) * C;
            vals = val[vi];
            if (C > 1) vals |= (uint32_t)val[vi + 1] << 8;
            if (C > 2) vals |= (uint32_t)val[vi + 2] << 16;
          }
        }
        if (uniform) {
          int ch = C == 3 ? (o0 + 48) % 3 : (o0 & (C - 1));  // o0 >= -15
#pragma unroll
          for (int j = 0; j < kRun; j++) {
            if (m & (1u << j)) out[j >> 2] = (out[j >> 2] & ~(255u << (8 * (j & 3)))) | (((vals >> (8 * ch)) & 255u) << (8 * (j & 3)));
            ch = ch + 1 == C ? 0 : ch + 1;
          }
        } else {
#pragma unroll
          for (int j = 0; j < kRun; j++) {
            if (m & (1u << j)) {
              const int o = o0 + j;
              const int x = C == 3 ? o / 3 : o >> (C - 1), ch = o - C * x;
              const uint32_t v = vmode == kMosaic ? val[(crow + colcell[x - xb]) * C + ch] : stage[(y - yb) & (kBlurBatch - 1)][o - blo];
              out[j >> 2] = (out[j >> 2] & ~(255u << (8 * (j & 3)))) | (v << (8 * (j & 3)));
            }
          }
        }
      }
      store_run(drow, o0, v0, v1, out);
    }
  };

  if (vmode == kCopy || vmode == kFill) {
    write_rows(yb, ye - yb, false);
  } else if (vmode == kMosaic) {
    // ---- every selected cell of the tile: sum, then the constant.  A lane walks its byte column down the tile (the loads of a
    // column do not depend on each other: many in flight) and leaves one sum per cell row; at most 256 x 255 fits 16 bits
    const int ncr = (ye - yb + par - 1) / par;
    for (int bc = tid; bc < len; bc += kThreads) {
      const uint32_t cb = colbits[C == 3 ? bc / 3 : bc >> (C - 1)];
      gcbyte_ptr a = (gcbyte_ptr)splane + (long long)yb * sp + blo + bc;
      uint32_t acc = 0;
      int left = par, cr = 0;
      for (int y = yb; y < ye; y += 8, a += 8 * (long long)sp) {  // 8 rows in flight
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (y + k < ye && (((cb & (uint32_t)rowbits[y + k - yb]) != 0) != (inv != 0))) ? a[(long long)k * sp] : 0u;
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (y + k < ye) {
            acc += v[k];
            if (--left == 0 || y + k == ye - 1) {
              colsum[cr * len + bc] = (unsigned short)acc;
              acc = 0; left = par; cr++;
            }
          }
      }
    }
    __syncthreads();
    for (int i = tid; i < ncr * ncc * C; i += kThreads) {  // i = (cell row * ncc + cell) * C + channel
      const int cell_i = i / C, ch = i - cell_i * C, cr = cell_i / ncc, cc = cell_i - cr * ncc;
      const int x0c = cc * par, x1c = min(x0c + par, xe - xb), y0c = yb + cr * par, y1c = min(y0c + par, ye);
      const int cs = cr * len + ch;
      uint32_t sum = 0;
      for (int xl = x0c; xl < x1c; xl++) sum += colsum[cs + xl * C];
      const uint32_t n = (uint32_t)((y1c - y0c) * (x1c - x0c));
      val[i] = (unsigned char)((sum + n / 2) / n);
    }
    __syncthreads();  // the values are complete, and every read of the tile's source is behind us
    write_rows(yb, ye - yb, false);
  } else {
    // ---- BLUR: lane = column xc of the plane (the tile's columns and rp more on both sides); kBlurBatch rows per round of barriers
    const int rp = par;
    const int xc = xb - rp + tid;
    const bool col_live = xc >= 0 && xc < cols && xc < xe + rp;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < kBlurRows / kBlurBatch) {  // does a rectangle reach a row of the batch?
      bool on = false;
      for (int i = 0; i < kBlurBatch; i++) {
        const int yl = kBlurBatch * tid + i;
        if (yb + yl < ye) on = on || inv || ((uint32_t)rowbits[yl] & kcols);
      }
      batch_on[tid] = on;
    }
    __syncthreads();
    write_rows(yb, ye - yb, true);  // the batches that no rectangle reaches
    uint32_t sums[3] = {0, 0, 0};   // column xc over rows [y - rp, y + rp] of the plane
    if (col_live) {
      const int ya = max(yb - rp, 0), yz = min(yb + rp, rows - 1);
      gcbyte_ptr a = (gcbyte_ptr)splane + (long long)ya * sp + (long long)xc * C;
#pragma unroll 8
      for (int y = ya; y <= yz; y++, a += sp) {
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < C) sums[c] += a[c];
      }
    }
    for (int y0 = yb; y0 < ye; y0 += kBlurBatch) {
      // step[i]: what turns the column's window of row y0 + i into that of row y0 + i + 1 (the sample that enters minus the one that
      // leaves), loaded for the whole batch at once: the latency hides behind the batch's work
      uint32_t step[kBlurBatch][3];
#pragma unroll
      for (int i = 0; i < kBlurBatch; i++) {
        const int ya = y0 + i + 1 + rp, ys = y0 + i - rp;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          uint32_t e = 0, l = 0;
          if (c < C && col_live) {
            if (ya < rows) e = ((gcbyte_ptr)splane + (long long)ya * sp + (long long)xc * C)[c];
            if (ys >= 0 && ys < rows) l = ((gcbyte_ptr)splane + (long long)ys * sp + (long long)xc * C)[c];
          }
          step[i][c] = e - l;
        }
      }
      const int nb = min(kBlurBatch, ye - y0);
      if (batch_on[(y0 - yb) / kBlurBatch]) {  // uniform
        uint32_t inc[kBlurBatch][3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          uint32_t rs = sums[c];
#pragma unroll
          for (int i = 0; i < kBlurBatch; i++) {  // the scans of the batch's rows and channels are independent chains
            uint32_t v = rs;
            if (c < C) {
#pragma unroll
              for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = __shfl_up(v, d, 64);
                if (lane >= d) v += u;
              }
              if (lane == 63) wtot[i][wave][c] = v;
            }
            inc[i][c] = v;
            rs += step[i][c];
          }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kBlurBatch; i++)
#pragma unroll
          for (int c = 0; c < 3; c++)
            if (c < C) {
              uint32_t off = 0;
#pragma unroll
              for (int w = 0; w < kThreads / 64 - 1; w++)
                if (w < wave) off += wtot[i][w][c];
              pre[i][c][tid] = inc[i][c] + off;
            }
        __syncthreads();
        if (tid >= rp && tid < rp + (xe - xb)) {
          const int nx = min(xc + rp, cols - 1) - max(xc - rp, 0) + 1;
#pragma unroll
          for (int i = 0; i < kBlurBatch; i++)
            if (i < nb) {
              const int y = y0 + i, ny = min(y + rp, rows - 1) - max(y - rp, 0) + 1;
              const uint32_t n = (uint32_t)(nx * ny);
#pragma unroll
              for (int c = 0; c < 3; c++)
                if (c < C) {
                  const uint32_t sum = pre[i][c][tid + rp] - (tid - rp - 1 >= 0 ? pre[i][c][tid - rp - 1] : 0u);
                  stage[i][(xc - xb) * C + c] = (unsigned char)((sum + n / 2) / n);
                }
            }
        }
        __syncthreads();
        write_rows(y0, nb, false);
      }
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < kBlurBatch; i++) sums[c] += step[i][c];  // slide to row y0 + kBlurBatch
    }
  }
}

}  // namespace td

using namespace td;

extern "C" size_t td_tube_redact_table_bytes(int n_jobs) { return table_bytes<RedactParams>(n_jobs); }

extern "C" int td_tube_redact(const td_redact_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_redact";
  if (int rc = check_workspace<RedactParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  RedactParams* host = (RedactParams*)table_host;
  int n = 0;
  long long blocks = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_redact_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.mode == TD_REDACT_FILL || j.mode == TD_REDACT_MOSAIC || j.mode == TD_REDACT_BLUR, "%s: job %d: unknown mode %d", who, i, j.mode);
    TD_REQUIRE(j.invert == 0 || j.invert == 1, "%s: job %d: invert %d is not 0 or 1", who, i, j.invert);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSide, "%s: job %d: sh x sw = %d x %d outside 1..%d", who, i, j.sh, j.sw, kMaxSide);
    TD_REQUIRE(j.n_tube >= 1, "%s: job %d: n_tube = %d is below 1", who, i, j.n_tube);
    TD_REQUIRE(j.K >= 1 && j.K <= kMaxRects, "%s: job %d: K = %d outside 1..%d", who, i, j.K, kMaxRects);
    TD_REQUIRE(j.margin_den >= 1 && j.margin_den <= kMaxMarginDen, "%s: job %d: margin_den = %d outside 1..%d", who, i, j.margin_den, kMaxMarginDen);
    TD_REQUIRE(j.margin_num >= 0 && j.margin_num <= 4 * j.margin_den, "%s: job %d: margin_num = %d outside 0..4 margin_den = %d", who, i, j.margin_num, 4 * j.margin_den);
    TD_REQUIRE(j.mode != TD_REDACT_MOSAIC || (j.cell >= 2 && j.cell <= 256 && (j.cell & 1) == 0), "%s: job %d: cell = %d is not an even number in 2..256", who, i, j.cell);
    TD_REQUIRE(j.mode != TD_REDACT_BLUR || (j.radius >= 1 && j.radius <= 64), "%s: job %d: radius = %d outside 1..64", who, i, j.radius);
    TD_REQUIRE(j.boxes, "%s: job %d: boxes is null", who, i);
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet sets[2] = {{"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride},
                              {"dst", {j.dst0, j.dst1, j.dst2}, {j.dst_pitch0, j.dst_pitch1, j.dst_pitch2}, j.dst_frame_stride}};
    const PlaneSet &sp = sets[0], &dp = sets[1];
    if (int rc = check_planes(who, i, g, sets, 2)) return rc;
    RedactParams p{};
    for (int k = 0; k < g.n_planes; k++) {  // in place is refused for BLUR, whatever the frame count
      bool inplace;
      if (int rc = check_inplace_or_apart(who, i, g, sp, dp, j.T, k, &inplace)) return rc;
      TD_REQUIRE(!inplace || j.mode != TD_REDACT_BLUR, "%s: job %d: dst%d is its source plane: TD_REDACT_BLUR cannot run in place (it reads neighbours that are already rewritten)", who, i, k);
      p.inplace[k] = inplace;
    }
    if (j.T == 0) continue;
    for (int k = 0; k < g.n_planes; k++) {
      p.src[k] = (const unsigned char*)sp.p[k]; p.dst[k] = (unsigned char*)dp.p[k];
      p.spitch[k] = sp.pitch[k]; p.dpitch[k] = dp.pitch[k];
    }
    p.sstride = j.src_frame_stride; p.dstride = j.dst_frame_stride;
    p.fmt = j.fmt; p.T = j.T; p.sh = j.sh; p.sw = j.sw;
    p.boxes = j.boxes; p.span = j.span; p.frame_map = j.frame_map;
    p.n_tube = j.n_tube; p.K = j.K; p.mode = j.mode; p.invert = j.invert;
    p.margin_num = j.margin_num; p.margin_den = j.margin_den;
    p.cell = j.mode == TD_REDACT_MOSAIC ? j.cell : 2; p.radius = j.mode == TD_REDACT_BLUR ? j.radius : 1;
    p.color = (uint32_t)j.color[0] | ((uint32_t)j.color[1] << 8) | ((uint32_t)j.color[2] << 16);
    p.n_planes = g.n_planes;
    long long job_blocks = 0;
    for (int k = 0; k < g.n_planes; k++) {
      if (j.mode == TD_REDACT_MOSAIC && (k ? p.cell / 2 : p.cell) >= 2) {
        const int cp = k ? p.cell / 2 : p.cell;  // whole cells: about kBlurRows rows, at most kCols samples
        p.th[k] = cp * std::min(kMosaicCellRows, std::max(1, kBlurRows / cp));
        p.tw[k] = cp * std::max(1, kCols / cp);
      } else if (j.mode == TD_REDACT_BLUR) {
        const int rp = k ? (p.radius + 1) / 2 : p.radius;
        p.th[k] = kBlurRows;
        p.tw[k] = kCols - 2 * rp;
      } else {
        p.th[k] = kFillRows;
        p.tw[k] = kFillCols;
      }
      p.ntx[k] = cdiv(g.cols[k], p.tw[k]);
      p.nty[k] = cdiv(g.rows[k], p.th[k]);
      p.pbegin[k] = (int)job_blocks;
      job_blocks += (long long)j.T * p.ntx[k] * p.nty[k];
    }
    if (int rc = add_blocks(who, blocks, job_blocks, p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_redact_kernel, blocks, 0, host, table_dev, n, stream, who);
}
