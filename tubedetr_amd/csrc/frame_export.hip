// Rendered frames exported on the device - cut to the frames wanted, downscaled, converted to another pixel format and padded:
// td_frame_export (include/tubedetr_hip.h has the rule: area resize A, yuv -> rgb B, rgb -> yuv C).
//
// A workgroup owns kTilesPerGroup tiles of kBand rows x kTile columns of ONE destination frame (padding included) of one job, one
// after the other.  For a tile it streams the
// source rows that its tile covers through the LDS, up to kMaxGroup rows per barrier pair, and every lane owns one output column:
//   * per source row the lane sums its columns' samples, weighted by their overlap with the column (yuv -> rgb24 converts each
//     sample on the way: B), and adds the row's sum, weighted by the row's overlap, to the accumulators of the output row(s) that
//     the source row touches - at most two, because nothing is enlarged.  A finished output row is rounded, divided and put
//     into the tile's picture in the LDS.  An axis that keeps its size runs with n = m = 1 (the same quotient: all of its
//     weights share the factor n), so a same-size job never leaves 8 bits and has no bound on sh sw;
//   * rgb24 -> yuv then makes the Y bytes and the chroma bytes from the tile's rgb picture in the LDS (C); yuv -> yuv runs the
//     row stream twice, for Y and for the chroma planes (their own ratio), straight into the Y and chroma pictures;
//   * at the end the lanes write the tile's rows of every destination plane as aligned 16-byte runs (frame_jobs.h), a byte of
//     the picture from the LDS, any other byte from `pad`; a blank frame and a tile beside or below the picture skip the stream.
// Tiles that meet inside a 16-byte run, or inside a source sample that two columns / two bands share, each touch only their own
// bytes of it; a shared source row or column is read by both.  LDS per workgroup: the tile's pictures (768 kBand + 256 kBand +
// 128 kBand bytes) and the staged rows (at most 16 KiB, or one row).  No helper moved to frame_jobs.h: stage_bytes and
// write_rows are used here only.
#include <algorithm>

#include "resample_dev.h"

namespace td {

namespace {

constexpr int kTile = 256;  // picture columns of a tile = lanes
constexpr int kBand = 8;    // destination rows of a tile (even: chroma rows are whole)
constexpr int kMaxGroup = 8;
constexpr int kStageBudget = 16 * 1024;
constexpr int kTilesPerGroup = 16;  // tiles of one frame per workgroup, one after the other: a tile alone is too little work for a launch slot
constexpr int kPictureBytes = kBand * (3 * kTile + kTile + kTile / 2);

struct Ratio { int ny, my, nx, mx, shift; uint32_t D; };  // per axis n -> m, (1, 1) for an axis that keeps its size; shift >= 0: D = 1 << shift

struct ExportParams {
  const unsigned char* src[3];
  unsigned char* dst[3];
  long long src_frame_stride, dst_frame_stride;
  const int* take;
  unsigned char* valid;
  int src_pitch[3], dst_pitch[3];
  int src_fmt, dst_fmt;
  int T, To, sh, sw, oh, ow, dh, dw;
  int yo, cy, crv, cgu, cgv, cbu;  // B
  int fwd[9], y_off;               // C: rows Y, U, V; y_off = 2^20 offset + 2^19
  uint32_t pad;
  Ratio luma, chroma;              // rgb24 and Y; the chroma planes of a yuv -> yuv job
  int group, slot_bytes, off_c1, off_c2;  // staged rows per barrier pair; bytes of one staged row; where its chroma rows start
  int nbands, ntiles, chunks, block_begin;  // chunks: workgroups per frame
};

__device__ __forceinline__ int overlap(int j, int i, int n, int m) { return max(0, min((j + 1) * n, (i + 1) * m) - max(j * n, i * m)); }

// bytes [gp, gp + nbytes) of the row [lo, hi) -> lds, by aligned dwords: byte k lands at lds[(gp & 3) + k]
__device__ __forceinline__ void stage_bytes(unsigned char* lds, const unsigned char* gp, int nbytes, const unsigned char* lo, const unsigned char* hi, int tid) {
  const int o = (int)((uintptr_t)gp & 3);
  const int nd = (o + nbytes + 3) >> 2;
  for (int d = tid; d < nd; d += kThreads) ((uint32_t*)lds)[d] = load_dword_guarded(gp - o + 4 * d, lo, hi);
}

__device__ __forceinline__ uint32_t rounded_quotient(uint32_t S, const Ratio& r) {
  if (r.shift >= 0) return (S + (r.D >> 1)) >> r.shift;
  return (S + (r.D >> 1)) / r.D;
}

enum { kFromRgb = 0,     // rgb24 -> rgb picture
       kFromYuv = 1,     // I420 / NV12 -> rgb picture (B on every sample)
       kPlanes = 2 };    // one byte plane -> one byte plane: Y, or U and V side by side (lanes 0..127 and 128..255)

// Stage A for output rows [j0, j1) and the tile's columns from c0 on; this lane's column is x (live: it lies in the picture).
// `which` (kPlanes, chroma): 0 = U, 1 = V.  out: where this lane's sample of row j0 goes; the next row lies out_pitch further.
template <int MODE>
__device__ __forceinline__ void resize_pass(const ExportParams& p, const Ratio& r, long long fsrc, bool chroma, int n_cols, int c0, int c1, int j0, int j1, int x, bool live,
                                            int which, unsigned char* stage, unsigned char* out, int out_pitch, int tid) {
  constexpr int NC = MODE == kPlanes ? 1 : 3;
  const int sa = (c0 * r.nx) / r.mx, sb = min(n_cols, (c1 * r.nx + r.mx - 1) / r.mx);  // the tile's source columns
  const int xa = (x * r.nx) / r.mx, xb = min(sb, ((x + 1) * r.nx + r.mx - 1) / r.mx);  // this lane's
  const int lo = x * r.nx, hi = lo + r.nx;
  const int ia = (j0 * r.ny) / r.my, ib = (j1 * r.ny + r.my - 1) / r.my;
  const bool nv12 = p.src_fmt == TD_SRC_NV12;
  uint32_t acc[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) acc[c] = 0;
  int j = j0;
  for (int ig = ia; ig < ib; ig += p.group) {
    const int n_g = min(p.group, ib - ig);
    __syncthreads();  // the rows staged before are consumed
    for (int g = 0; g < n_g; g++) {
      const int i = ig + g;
      unsigned char* slot = stage + (size_t)g * p.slot_bytes;
      if (MODE == kFromRgb) {
        const unsigned char* row = p.src[0] + fsrc + (long long)i * p.src_pitch[0];
        stage_bytes(slot, row + 3 * sa, 3 * (sb - sa), row, row + 3 * p.sw, tid);
      } else if (MODE == kFromYuv || !chroma) {
        const unsigned char* row = p.src[0] + fsrc + (long long)i * p.src_pitch[0];
        stage_bytes(slot, row + sa, sb - sa, row, row + p.sw, tid);
      }
      if (MODE == kFromYuv ? (g == 0 || !(i & 1)) : (MODE == kPlanes && chroma)) {
        // chroma row and columns: of the 2 x 2 blocks of the staged luma (kFromYuv), or the plane's own (kPlanes)
        const int ci = MODE == kFromYuv ? i >> 1 : i, ca = MODE == kFromYuv ? sa >> 1 : sa, cb = MODE == kFromYuv ? ((sb - 1) >> 1) + 1 : sb;
        const int cw = (p.sw + 1) >> 1;
        if (nv12) {
          const unsigned char* row = p.src[1] + fsrc + (long long)ci * p.src_pitch[1];
          stage_bytes(slot + p.off_c1, row + 2 * ca, 2 * (cb - ca), row, row + 2 * cw, tid);
        } else {
          const unsigned char* row1 = p.src[1] + fsrc + (long long)ci * p.src_pitch[1];
          const unsigned char* row2 = p.src[2] + fsrc + (long long)ci * p.src_pitch[2];
          stage_bytes(slot + p.off_c1, row1 + ca, cb - ca, row1, row1 + cw, tid);
          stage_bytes(slot + p.off_c2, row2 + ca, cb - ca, row2, row2 + cw, tid);
        }
      }
    }
    __syncthreads();
    for (int g = 0; g < n_g; g++) {
      const int i = ig + g;
      uint32_t H[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) H[c] = 0;
      if (live) {
        const unsigned char* slot = stage + (size_t)g * p.slot_bytes;
        if (MODE == kFromRgb) {
          const unsigned char* s = slot + ((uintptr_t)(p.src[0] + fsrc + (long long)i * p.src_pitch[0] + 3 * sa) & 3);
          for (int k = xa; k < xb; k++) {
            const uint32_t w = (uint32_t)(min(hi, (k + 1) * r.mx) - max(lo, k * r.mx));
#pragma unroll
            for (int c = 0; c < 3; c++) H[c] += w * s[3 * (k - sa) + c];
          }
        } else if (MODE == kFromYuv) {
          const unsigned char* cslot = stage + (size_t)((i & 1) && g > 0 ? g - 1 : g) * p.slot_bytes;
          const int ci = i >> 1, ca = sa >> 1;
          const unsigned char* sy = slot + ((uintptr_t)(p.src[0] + fsrc + (long long)i * p.src_pitch[0] + sa) & 3);
          const unsigned char *su, *sv;
          int cstep;
          if (nv12) {
            su = cslot + p.off_c1 + ((uintptr_t)(p.src[1] + fsrc + (long long)ci * p.src_pitch[1] + 2 * ca) & 3);
            sv = su + 1;
            cstep = 2;
          } else {
            su = cslot + p.off_c1 + ((uintptr_t)(p.src[1] + fsrc + (long long)ci * p.src_pitch[1] + ca) & 3);
            sv = cslot + p.off_c2 + ((uintptr_t)(p.src[2] + fsrc + (long long)ci * p.src_pitch[2] + ca) & 3);
            cstep = 1;
          }
          const int base = 32768 - p.cy * p.yo;
          for (int k = xa; k < xb; k++) {
            const uint32_t w = (uint32_t)(min(hi, (k + 1) * r.mx) - max(lo, k * r.mx));
            const int yy = __mul24(p.cy, (int)sy[k - sa]) + base;
            const int d = (int)su[cstep * ((k >> 1) - ca)] - 128, e = (int)sv[cstep * ((k >> 1) - ca)] - 128;
            H[0] += w * shift_clamp_u8(yy + __mul24(p.crv, e));
            H[1] += w * shift_clamp_u8(yy - __mul24(p.cgu, d) - __mul24(p.cgv, e));
            H[2] += w * shift_clamp_u8(yy + __mul24(p.cbu, d));
          }
        } else {
          const unsigned char* s;
          int step = 1;
          if (!chroma) s = slot + ((uintptr_t)(p.src[0] + fsrc + (long long)i * p.src_pitch[0] + sa) & 3);
          else if (nv12) {
            s = slot + p.off_c1 + ((uintptr_t)(p.src[1] + fsrc + (long long)i * p.src_pitch[1] + 2 * sa) & 3) + which;
            step = 2;
          } else {
            const unsigned char* row = which ? p.src[2] + fsrc + (long long)i * p.src_pitch[2] : p.src[1] + fsrc + (long long)i * p.src_pitch[1];
            s = slot + (which ? p.off_c2 : p.off_c1) + ((uintptr_t)(row + sa) & 3);
          }
          for (int k = xa; k < xb; k++) {
            const uint32_t w = (uint32_t)(min(hi, (k + 1) * r.mx) - max(lo, k * r.mx));
            H[0] += w * s[step * (k - sa)];
          }
        }
      }
      // the output row(s) that source row i touches: uniform over the workgroup
      const uint32_t wy = (uint32_t)overlap(j, i, r.ny, r.my);
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] += wy * H[c];
      if ((i + 1) * r.my >= (j + 1) * r.ny) {  // row j ends inside source row i
        if (live) {
#pragma unroll
          for (int c = 0; c < NC; c++) out[(j - j0) * out_pitch + c] = (unsigned char)rounded_quotient(acc[c], r);
        }
        j++;
        const uint32_t wn = j < j1 ? (uint32_t)overlap(j, i, r.ny, r.my) : 0u;
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = wn * H[c];
      }
    }
  }
}

// Rows [r0, r1) of a destination plane, bytes [b0, b1) of each: byte b of row r comes from lds[(r - r0) * lds_pitch + b - b0] when
// r < vr and b < vb (the picture), else it is the pad byte of component c0 + b % per.
__device__ __forceinline__ void write_rows(unsigned char* plane, int pitch, int r0, int r1, int b0, int b1, int vr, int vb, const unsigned char* lds, int lds_pitch, uint32_t pad,
                                           int per, int c0, int tid) {
  if (b1 <= b0) return;
  const int runs = ((b1 - b0) >> 4) + 2;
  const int inv = (65536 + runs - 1) / runs;  // idx / runs = (idx * inv) >> 16 while idx * runs < 65536: a tile has at most kBand * 50 runs
  for (int idx = tid; idx < (r1 - r0) * runs; idx += kThreads) {
    const int rr = (idx * inv) >> 16, k = idx - rr * runs;
    unsigned char* rowp = plane + (long long)(r0 + rr) * pitch;
    const int o0 = b0 - (int)((uintptr_t)(rowp + b0) & 15) + kRun * k;
    if (o0 >= b1) continue;
    const int v0 = max(o0, b0), v1 = min(o0 + kRun, b1);
    const bool row_in = r0 + rr < vr;
    const unsigned char* s = lds + rr * lds_pitch;
    uint32_t out[4] = {0, 0, 0, 0};
    if (row_in && v0 == o0 && v1 == o0 + kRun && v1 <= vb) {  // a whole run of the picture: no byte needs a decision
      __builtin_memcpy(out, s + (o0 - b0), kRun);
    } else {
#pragma unroll
      for (int q = 0; q < kRun; q++) {
        const int b = o0 + q;
        if (b >= v0 && b < v1) {
          const uint32_t v = row_in && b < vb ? (uint32_t)s[b - b0] : (pad >> (8 * (c0 + (per == 3 ? b % 3 : per == 2 ? (b & 1) : 0)))) & 0xffu;
          out[q >> 2] |= v << (8 * (q & 3));
        }
      }
    }
    store_run(rowp, o0, v0, v1, out);
  }
}

}  // namespace

// one tile (band, tile) of output frame fi; every lane of the workgroup comes through here, so the barriers inside are uniform
__device__ __forceinline__ void export_tile(const ExportParams& p, unsigned char* smem, int fi, int band, int tile, int tid) {
  const int y0 = band * kBand, y1 = min(y0 + kBand, p.dh), x0 = tile * kTile, x1 = min(x0 + kTile, p.dw);

  unsigned char* rgb = smem;                   // [kBand][3 kTile]
  unsigned char* lum = rgb + kBand * 3 * kTile;  // [kBand][kTile]
  unsigned char* chr = lum + kBand * kTile;      // [kBand / 2][kTile]: I420: U in [0, 128), V in [128, 256); NV12: pairs
  unsigned char* stage = chr + (kBand / 2) * kTile;

  int s = p.take ? ((const TD_GLOBAL int*)p.take)[fi] : fi;
  s = __builtin_amdgcn_readfirstlane(s);
  const bool blank = s < 0 || s >= p.T;
  if (p.valid && band == 0 && tile == 0 && tid == 0) ((gbyte_ptr)p.valid)[fi] = blank ? 0 : 1;
  const bool inside = !blank && y0 < p.oh && x0 < p.ow;
  const int py1 = min(y1, p.oh), px1 = min(x1, p.ow);  // the picture's part of the tile
  const bool src_rgb = p.src_fmt == TD_SRC_RGB24, dst_rgb = p.dst_fmt == TD_SRC_RGB24, dst_nv12 = p.dst_fmt == TD_SRC_NV12;

  if (inside) {
    const long long fsrc = (long long)s * p.src_frame_stride;
    if (src_rgb || dst_rgb) {
      const int x = x0 + tid;
      if (src_rgb) resize_pass<kFromRgb>(p, p.luma, fsrc, false, p.sw, x0, px1, y0, py1, x, x < px1, 0, stage, rgb + 3 * tid, 3 * kTile, tid);
      else resize_pass<kFromYuv>(p, p.luma, fsrc, false, p.sw, x0, px1, y0, py1, x, x < px1, 0, stage, rgb + 3 * tid, 3 * kTile, tid);
      if (!dst_rgb) {  // C on the tile's rgb picture
        __syncthreads();
        for (int idx = tid; idx < (py1 - y0) * (kTile / 4); idx += kThreads) {  // 4 pixels per lane: 3 dwords in, 1 out (a pixel beyond px1 is never read back)
          const int rr = idx / (kTile / 4), xl = 4 * (idx - rr * (kTile / 4));
          if (x0 + xl < px1) {
            const uint32_t* q = (const uint32_t*)(rgb + rr * 3 * kTile + 3 * xl);
            const uint32_t w[3] = {q[0], q[1], q[2]};
            uint32_t packed = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const int c[3] = {(int)((w[(3 * e) >> 2] >> (8 * ((3 * e) & 3))) & 0xff), (int)((w[(3 * e + 1) >> 2] >> (8 * ((3 * e + 1) & 3))) & 0xff),
                                (int)((w[(3 * e + 2) >> 2] >> (8 * ((3 * e + 2) & 3))) & 0xff)};
              const int a = p.fwd[0] * c[0] + p.fwd[1] * c[1] + p.fwd[2] * c[2] + p.y_off;
              packed |= (uint32_t)(min(max(a, 0), (256 << 20) - 1) >> 20) << (8 * e);
            }
            *(uint32_t*)(lum + rr * kTile + xl) = packed;
          }
        }
        const int cr0 = y0 >> 1, cr1 = (py1 + 1) >> 1, cc0 = x0 >> 1, cc1 = (px1 + 1) >> 1;
        for (int idx = tid; idx < (cr1 - cr0) * (kTile / 2); idx += kThreads) {
          const int rr = idx / (kTile / 2), xl = idx - rr * (kTile / 2);
          if (cc0 + xl < cc1) {
            const int yy = 2 * rr, xx = 2 * xl;  // in the tile
            const int nyb = y0 + yy + 1 < py1 ? 2 : 1, nxb = x0 + xx + 1 < px1 ? 2 : 1;
            int Rs = 0, Gs = 0, Bs = 0;
            for (int dy = 0; dy < nyb; dy++)
              for (int dx = 0; dx < nxb; dx++) {
                const unsigned char* q = rgb + (yy + dy) * 3 * kTile + 3 * (xx + dx);
                Rs += q[0]; Gs += q[1]; Bs += q[2];
              }
            const int lg = (nyb >> 1) + (nxb >> 1);  // log2 of the block's pixels
            const int off = ((128 << 20) + (1 << 19)) << lg, top = (256 << (20 + lg)) - 1;
            const int u = min(max(p.fwd[3] * Rs + p.fwd[4] * Gs + p.fwd[5] * Bs + off, 0), top) >> (20 + lg);
            const int v = min(max(p.fwd[6] * Rs + p.fwd[7] * Gs + p.fwd[8] * Bs + off, 0), top) >> (20 + lg);
            if (dst_nv12) { chr[rr * kTile + 2 * xl] = (unsigned char)u; chr[rr * kTile + 2 * xl + 1] = (unsigned char)v; }
            else { chr[rr * kTile + xl] = (unsigned char)u; chr[rr * kTile + kTile / 2 + xl] = (unsigned char)v; }
          }
        }
      }
    } else {  // yuv -> yuv: the Y plane, then U and V with the chroma planes' own ratio
      resize_pass<kPlanes>(p, p.luma, fsrc, false, p.sw, x0, px1, y0, py1, x0 + tid, x0 + tid < px1, 0, stage, lum + tid, kTile, tid);
      const int which = tid >> 7, xl = tid & 127;
      const int cr0 = y0 >> 1, cr1 = (py1 + 1) >> 1, cc0 = x0 >> 1, cc1 = (px1 + 1) >> 1;
      unsigned char* out = dst_nv12 ? chr + 2 * xl + which : chr + which * (kTile / 2) + xl;
      resize_pass<kPlanes>(p, p.chroma, fsrc, true, (p.sw + 1) >> 1, cc0, cc1, cr0, cr1, cc0 + xl, cc0 + xl < cc1, which, stage, out, kTile, tid);
    }
  }
  __syncthreads();

  // ---- the tile's rows of every destination plane
  const long long fdst = (long long)fi * p.dst_frame_stride;
  const int vr = inside ? py1 : 0;
  if (dst_rgb) {
    write_rows(p.dst[0] + fdst, p.dst_pitch[0], y0, y1, 3 * x0, 3 * x1, vr, 3 * px1, rgb, 3 * kTile, p.pad, 3, 0, tid);
  } else {
    write_rows(p.dst[0] + fdst, p.dst_pitch[0], y0, y1, x0, x1, vr, px1, lum, kTile, p.pad, 1, 0, tid);
    const int cr0 = y0 >> 1, cr1 = (y1 + 1) >> 1, cc0 = x0 >> 1, cc1 = (x1 + 1) >> 1;
    const int cvr = inside ? (py1 + 1) >> 1 : 0, cvb = (px1 + 1) >> 1;
    if (dst_nv12) {
      write_rows(p.dst[1] + fdst, p.dst_pitch[1], cr0, cr1, 2 * cc0, 2 * cc1, cvr, 2 * cvb, chr, kTile, p.pad, 2, 1, tid);
    } else {
      write_rows(p.dst[1] + fdst, p.dst_pitch[1], cr0, cr1, cc0, cc1, cvr, cvb, chr, kTile, p.pad, 1, 1, tid);
      write_rows(p.dst[2] + fdst, p.dst_pitch[2], cr0, cr1, cc0, cc1, cvr, cvb, chr + kTile / 2, kTile, p.pad, 1, 2, tid);
    }
  }
}

__global__ __launch_bounds__(kThreads) void frame_export_kernel(const ExportParams* __restrict__ tab, int n_jobs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const ExportParams p = tab[find_job(tab, n_jobs, b)];
  const int local = b - p.block_begin;
  const int fi = local / p.chunks, first = (local - fi * p.chunks) * kTilesPerGroup, n_tiles = p.nbands * p.ntiles;
  for (int it = first; it < min(first + kTilesPerGroup, n_tiles); it++) {  // tiles side by side first: they share source rows
    export_tile(p, smem, fi, it / p.ntiles, it % p.ntiles, tid);
    __syncthreads();  // the next tile rewrites the pictures
  }
}

namespace {

constexpr int kMaxCols = 8192;
constexpr long long kMaxResizePixels = 1LL << 24;

// round(2^20 x) of the forward matrix (render.color_in_space; the header gives x by Kr, Kb and the range): rows Y, U, V
const int kFwdCoef[2][2][9] = {
    {{269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897}, {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}},  // BT.601
    {{191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230}, {222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074}},   // BT.709
};

Ratio make_ratio(int ny, int my, int nx, int mx) {
  Ratio r{};
  r.ny = ny == my ? 1 : ny; r.my = ny == my ? 1 : my;
  r.nx = nx == mx ? 1 : nx; r.mx = nx == mx ? 1 : mx;
  r.D = (uint32_t)r.ny * (uint32_t)r.nx;
  r.shift = -1;
  for (int s = 0; s < 32; s++)
    if (r.D == (1u << s)) r.shift = s;
  return r;
}

// source columns that a tile of `tile` output columns can cover
int tile_span(int n, int m, int tile) { return (int)std::min<long long>(n, ((long long)tile * n + m - 1) / m + 1); }

int align16(int v) { return (v + 15) & ~15; }

bool is_fmt(int f) { return f == TD_SRC_RGB24 || f == TD_SRC_I420 || f == TD_SRC_NV12; }

}  // namespace

}  // namespace td

using namespace td;

extern "C" size_t td_frame_export_table_bytes(int n_jobs) { return table_bytes<ExportParams>(n_jobs); }

extern "C" int td_frame_export(const td_export_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_frame_export";
  if (int rc = check_workspace<ExportParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  ExportParams* host = (ExportParams*)table_host;
  int n = 0;
  long long blocks = 0;
  size_t lds = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_export_job& j = jobs[i];
    TD_REQUIRE(is_fmt(j.src_fmt), "%s: job %d: unknown src_fmt %d", who, i, j.src_fmt);
    TD_REQUIRE(is_fmt(j.dst_fmt), "%s: job %d: unknown dst_fmt %d", who, i, j.dst_fmt);
    const bool any_yuv = j.src_fmt != TD_SRC_RGB24 || j.dst_fmt != TD_SRC_RGB24;
    TD_REQUIRE(!any_yuv || j.matrix == TD_MATRIX_BT601 || j.matrix == TD_MATRIX_BT709, "%s: job %d: unknown matrix %d", who, i, j.matrix);
    TD_REQUIRE(!any_yuv || j.full_range == 0 || j.full_range == 1, "%s: job %d: full_range %d is not 0 or 1", who, i, j.full_range);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.To >= 0, "%s: job %d: negative frame count To = %d", who, i, j.To);
    TD_REQUIRE(j.take || j.To == j.T, "%s: job %d: To = %d differs from T = %d and take is null", who, i, j.To, j.T);
    TD_REQUIRE(j.sh > 0 && j.sh <= kMaxSide, "%s: job %d: sh = %d outside 1..%d", who, i, j.sh, kMaxSide);
    TD_REQUIRE(j.sw > 0 && j.sw <= kMaxCols, "%s: job %d: sw = %d outside 1..%d (the LDS stages whole rows of a narrow picture)", who, i, j.sw, kMaxCols);
    TD_REQUIRE(j.oh > 0 && j.oh <= j.sh, "%s: job %d: oh = %d outside 1..sh = %d (no enlargement)", who, i, j.oh, j.sh);
    TD_REQUIRE(j.ow > 0 && j.ow <= j.sw, "%s: job %d: ow = %d outside 1..sw = %d (no enlargement)", who, i, j.ow, j.sw);
    const bool resize = j.oh != j.sh || j.ow != j.sw;
    TD_REQUIRE(!resize || (long long)j.sh * j.sw <= kMaxResizePixels, "%s: job %d: sh * sw = %lld is above 2^24, the bound of a job that resizes", who, i, (long long)j.sh * j.sw);
    TD_REQUIRE(j.dh >= j.oh && j.dh <= kMaxSide, "%s: job %d: dh = %d outside oh = %d .. %d", who, i, j.dh, j.oh, kMaxSide);
    TD_REQUIRE(j.dw >= j.ow && j.dw <= kMaxSide, "%s: job %d: dw = %d outside ow = %d .. %d", who, i, j.dw, j.ow, kMaxSide);
    const PlaneGeom gs = plane_geom(j.src_fmt, j.sh, j.sw), gd = plane_geom(j.dst_fmt, j.dh, j.dw);
    const PlaneSet src{"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride};
    const PlaneSet dst{"dst", {j.dst0, j.dst1, j.dst2}, {j.dst_pitch0, j.dst_pitch1, j.dst_pitch2}, j.dst_frame_stride};
    if (int rc = check_planes(who, i, gs, &src, 1)) return rc;
    if (int rc = check_planes(who, i, gd, &dst, 1)) return rc;
    if (j.To == 0) continue;
    if (j.T > 0) {  // no export in place: the To destination frames touch none of the T source frames
      for (int k = 0; k < gd.n_planes; k++) {
        const unsigned char* d0 = (const unsigned char*)dst.p[k];
        for (int m = 0; m < gs.n_planes; m++)
          TD_REQUIRE(d0 + plane_extent(gd, k, dst.pitch[k], dst.frame_stride, j.To) <= src.p[m] ||
                         (const unsigned char*)src.p[m] + plane_extent(gs, m, src.pitch[m], src.frame_stride, j.T) <= d0,
                     "%s: job %d: dst%d overlaps src%d (an export is never in place)", who, i, k, m);
      }
    }
    ExportParams p{};
    for (int k = 0; k < 3; k++) {
      p.src[k] = (const unsigned char*)src.p[k]; p.src_pitch[k] = src.pitch[k];
      p.dst[k] = (unsigned char*)dst.p[k]; p.dst_pitch[k] = dst.pitch[k];
    }
    p.src_frame_stride = j.src_frame_stride; p.dst_frame_stride = j.dst_frame_stride;
    p.take = j.take; p.valid = j.valid;
    p.src_fmt = j.src_fmt; p.dst_fmt = j.dst_fmt;
    p.T = j.T; p.To = j.To; p.sh = j.sh; p.sw = j.sw; p.oh = j.oh; p.ow = j.ow; p.dh = j.dh; p.dw = j.dw;
    if (any_yuv) {
      const int* k = kYuvCoef[j.matrix][j.full_range];
      p.yo = k[0]; p.cy = k[1]; p.crv = k[2]; p.cgu = k[3]; p.cgv = k[4]; p.cbu = k[5];
      for (int q = 0; q < 9; q++) p.fwd[q] = kFwdCoef[j.matrix][j.full_range][q];
      p.y_off = ((j.full_range ? 0 : 16) << 20) + (1 << 19);
    }
    p.pad = pack3(j.pad);
    p.luma = make_ratio(j.sh, j.oh, j.sw, j.ow);
    p.chroma = make_ratio((j.sh + 1) / 2, (j.oh + 1) / 2, (j.sw + 1) / 2, (j.ow + 1) / 2);
    // a staged row: the tile's source columns, from an address rounded down to a dword (+ 3), per plane
    const int span = tile_span(j.sw, j.ow, kTile);
    if (j.src_fmt == TD_SRC_RGB24) p.slot_bytes = align16(3 * span + 8);
    else {
      const int cspan = std::max(span / 2 + 2, tile_span((j.sw + 1) / 2, (j.ow + 1) / 2, kTile / 2));
      p.off_c1 = align16(span + 8);
      p.off_c2 = p.off_c1 + align16(2 * cspan + 8);
      p.slot_bytes = p.off_c2 + align16(2 * cspan + 8);
    }
    p.group = std::min(kMaxGroup, std::max(1, kStageBudget / p.slot_bytes));
    const size_t need = (size_t)kPictureBytes + (size_t)p.group * p.slot_bytes;
    TD_REQUIRE(need <= kMaxLds, "%s: job %d needs %zu bytes of LDS: sw = %d is too large for ow = %d", who, i, need, j.sw, j.ow);
    lds = std::max(lds, need);
    p.nbands = cdiv(j.dh, kBand); p.ntiles = cdiv(j.dw, kTile);
    p.chunks = cdiv(p.nbands * p.ntiles, kTilesPerGroup);
    if (int rc = add_blocks(who, blocks, (long long)j.To * p.chunks, p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(frame_export_kernel, blocks, lds, host, table_dev, n, stream, who);
}
