// Device code shared by the bilinear resampling kernels: td_clip_resample / td_clip_resample_src (augment.hip) and
// td_tube_crop (tube_crop.hip).  The crop's pixels are DEFINED as what td_clip_resample writes for the same window, so the
// three places where a bit could differ - the tap coordinates, the yuv -> rgb staging conversion and the order of the three
// fmaf of the blend - exist once, here, and both translation units instantiate them.  What these kernels share with the other
// job-table kernels (addressing, the tube rule, plane checks, the launch) is in frame_jobs.h.
//
// The yuv functions are templates over the job record P; they read P's fields
//   src, plane1, plane2 (plane pointers of frame 0), src_frame_stride, pitch, pitch1, pitch2, src_bytes, bytes1, bytes2 (extents),
//   fmt, cmin (first staged source column), nd (staged Y dwords of a row), slot_bytes, yo, cy, crv, cgu, cgv, cbu.
#pragma once
#include "frame_jobs.h"

namespace td {

constexpr int kMaxBand = 4;        // output rows per workgroup
constexpr int kStageDepth = 4;     // staged dwords per lane and source row held in registers (rows of up to 1365 pixels take the fast path)
constexpr int kYuvDepth = 2;       // the same for Y dwords of an I420 / NV12 row (rows of up to 2045 pixels): a staged Y dword brings up to 4 chroma dwords along
constexpr int kFrameChunk = 4;     // frames per workgroup (amortises the column table)
constexpr int kMaxSrcCols = 8192;  // 3 * (column - cmin) fits the table's 16-bit offsets
constexpr size_t kMaxLds = 64 * 1024;

struct ColEntry { unsigned short off0, off1; float w; };
struct RowEntry { int y0, y1; float w; int pad; };

// source index pair + weight of output index v of a virtual resize of n_src samples to n_dst (exact integers)
__device__ __forceinline__ void tap(int v, int n_src, int n_dst, int& i0, int& i1, float& w) {
  const int num = (2 * v + 1) * n_src - n_dst, den = 2 * n_dst;
  int q = 0, r = 0;
  if (num > 0) { q = num / den; r = num - q * den; }
  i0 = q;
  i1 = min(q + 1, n_src - 1);
  w = (float)r / (float)den;  // r < den <= 2^15: both exact in fp32, the quotient correctly rounded
}

// one output byte from the four taps of channel c: staged rows r0 (upper) and r1 (lower), column entry ce, row weight wy
__device__ __forceinline__ uint32_t blend_taps(const ColEntry ce, const unsigned char* r0, const unsigned char* r1, float wy, int c) {
  const float p00 = (float)r0[ce.off0 + c], p01 = (float)r0[ce.off1 + c], p10 = (float)r1[ce.off0 + c], p11 = (float)r1[ce.off1 + c];
  const float top = fmaf(ce.w, p01 - p00, p00), bot = fmaf(ce.w, p11 - p10, p10);
  return (uint32_t)(fmaf(wy, bot - top, top) + 0.5f);
}

// 4 bytes at the dword-aligned address a; bytes outside [lo, hi) read as 0 and are never touched
__device__ __forceinline__ uint32_t load_dword_guarded(const unsigned char* a, const unsigned char* lo, const unsigned char* hi) {
  if (a >= lo && a + 4 <= hi) return *(const TD_GLOBAL uint32_t*)a;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (a + j >= lo && a + j < hi) v |= (uint32_t)((gcbyte_ptr)a)[j] << (8 * j);
  return v;
}

// clamp(acc >> 16) to [0, 255], written as a clamp of the accumulator BEFORE the shift (the same integer for every acc).
// The shift-then-clamp form is selected as v_ashr_pk_u8_i32 for pairs of channels, and the bytes packed next to its result
// came back ORed with the unclamped second value on the MI355X (hipcc roc-7.2.0): do not "simplify" this back.
__device__ __forceinline__ uint32_t shift_clamp_u8(int acc) { return (uint32_t)min(max(acc, 0), 0xffffff) >> 16; }

// 4 bytes from the unaligned address a + (sh >> 3) of the aligned dword pair (lo at a, hi at a + 4)
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh); }

// where the staged Y dword d of source row srow and its chroma samples live: y is dword-aligned and holds columns x0 .. x0 + 3
// (x0 may start before column 0 or end past the row: those pixels are converted from whatever the guards let through and never
// read); c1 / c2 are the addresses of chroma sample x0 >> 1 (NV12: c1 is its (U, V) pair)
struct YuvAddr { const unsigned char *y, *c1, *c2; int x0, o; };
template <typename P>
__device__ __forceinline__ YuvAddr yuv_addr(const P& p, int t, int srow, int d) {
  const long long f = (long long)t * p.src_frame_stride;
  const unsigned char* rp = p.src + f + (long long)srow * p.pitch + p.cmin;
  YuvAddr a;
  a.o = (int)((uintptr_t)rp & 3);
  a.y = rp - a.o + 4 * d;
  a.x0 = p.cmin - a.o + 4 * d;
  const int cx = a.x0 >> 1, crow = srow >> 1;
  if (p.fmt == TD_SRC_NV12) {
    a.c1 = p.plane1 + f + (long long)crow * p.pitch1 + 2 * cx;
    a.c2 = nullptr;
  } else {
    a.c1 = p.plane1 + f + (long long)crow * p.pitch1 + cx;
    a.c2 = p.plane2 + f + (long long)crow * p.pitch2 + cx;
  }
  return a;
}

// the aligned dwords that hold a Y dword's chroma: I420 c[0..1] = U, c[2..3] = V (3 samples from any alignment span at most 2 dwords),
// NV12 c[0..2] (3 pairs span at most 3)
template <typename P>
__device__ __forceinline__ void load_yuv(const P& p, const YuvAddr& a, uint32_t& y, uint32_t c[4]) {
  y = load_dword_guarded(a.y, p.src, p.src + p.src_bytes);
  const unsigned char* b1 = a.c1 - ((uintptr_t)a.c1 & 3);
  c[0] = load_dword_guarded(b1, p.plane1, p.plane1 + p.bytes1);
  c[1] = load_dword_guarded(b1 + 4, p.plane1, p.plane1 + p.bytes1);
  if (p.fmt == TD_SRC_NV12) {
    c[2] = load_dword_guarded(b1 + 8, p.plane1, p.plane1 + p.bytes1);
    c[3] = 0;
  } else {
    const unsigned char* b2 = a.c2 - ((uintptr_t)a.c2 & 3);
    c[2] = load_dword_guarded(b2, p.plane2, p.plane2 + p.bytes2);
    c[3] = load_dword_guarded(b2 + 4, p.plane2, p.plane2 + p.bytes2);
  }
}

// the header's integer rule on the 4 pixels of a Y dword -> their 12 rgb bytes.  The accumulators are the header's, term by term
// regrouped (exact in int32): cy (Y - yo) + crv (V - 128) + 32768 = cy Y + (crv V + bias_r), the bracket once per chroma sample.
// Every factor is below 2^24: 24-bit multiplies (full rate; the 32-bit ones are not).
template <typename P>
__device__ __forceinline__ void yuv_to_rgb4(const P& p, const YuvAddr& a, uint32_t y, const uint32_t c[4], uint32_t out[3]) {
  uint32_t u, v;  // byte i = sample (x0 >> 1) + i
  if (p.fmt == TD_SRC_NV12) {
    const int sh = 8 * (int)((uintptr_t)a.c1 & 3);
    const uint32_t w0 = funnel(c[0], c[1], sh), w1 = funnel(c[1], c[2], sh);  // U0 V0 U1 V1 | U2 V2 . .
    u = (w0 & 0xff) | ((w0 >> 8) & 0xff00) | ((w1 & 0xff) << 16);
    v = ((w0 >> 8) & 0xff) | ((w0 >> 16) & 0xff00) | ((w1 & 0xff00) << 8);
  } else {
    u = funnel(c[0], c[1], 8 * (int)((uintptr_t)a.c1 & 3));
    v = funnel(c[2], c[3], 8 * (int)((uintptr_t)a.c2 & 3));
  }
  const int base = 32768 - p.cy * p.yo;  // uniform: scalar arithmetic
  const int bias_r = base - 128 * p.crv, bias_g = base + 128 * (p.cgu + p.cgv), bias_b = base - 128 * p.cbu;
  int cr[3], cg[3], cb[3];  // the chroma part of the three accumulators, per chroma sample
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int uu = (int)((u >> (8 * i)) & 0xff), vv = (int)((v >> (8 * i)) & 0xff);
    cr[i] = __mul24(p.crv, vv) + bias_r;
    cg[i] = bias_g - __mul24(p.cgu, uu) - __mul24(p.cgv, vv);
    cb[i] = __mul24(p.cbu, uu) + bias_b;
  }
  const bool odd = a.x0 & 1;  // column x0 + j uses sample (x0 + j) >> 1 = (x0 >> 1) + ((j + odd) >> 1): 0, 0 | 1, 1, 1 | 2
  out[0] = out[1] = out[2] = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int yy = __mul24(p.cy, (int)((y >> (8 * j)) & 0xff));
    int r, g, b;
    if (j == 0 || j == 2) { r = cr[j >> 1]; g = cg[j >> 1]; b = cb[j >> 1]; }
    else { r = odd ? cr[(j + 1) >> 1] : cr[j >> 1]; g = odd ? cg[(j + 1) >> 1] : cg[j >> 1]; b = odd ? cb[(j + 1) >> 1] : cb[j >> 1]; }
    const uint32_t px[3] = {shift_clamp_u8(yy + r), shift_clamp_u8(yy + g), shift_clamp_u8(yy + b)};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) out[(3 * j + ch) >> 2] |= px[ch] << (8 * ((3 * j + ch) & 3));
  }
}

// staging of an I420 / NV12 band: as the rgb24 staging of the kernels, with the conversion between the loads and the LDS writes
template <typename P>
__device__ __forceinline__ void stage_yuv(const P& p, const RowEntry* row, int* slot_off, unsigned char* slots, int t, int n_live, int tid) {
  const int nd = p.nd;
  if (nd <= kYuvDepth * kThreads) {
    uint32_t y[2 * kMaxBand][kYuvDepth], c[2 * kMaxBand][kYuvDepth][4];
#pragma unroll
    for (int s = 0; s < 2 * kMaxBand; s++) {
      if (s < 2 * n_live) {
        const int srow = (s & 1) ? row[s >> 1].y1 : row[s >> 1].y0;
#pragma unroll
        for (int k = 0; k < kYuvDepth; k++) {
          const int d = tid + k * kThreads;
          if (d < nd) load_yuv(p, yuv_addr(p, t, srow, d), y[s][k], c[s][k]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 2 * kMaxBand; s++) {
      if (s < 2 * n_live) {
        const int srow = (s & 1) ? row[s >> 1].y1 : row[s >> 1].y0;
        uint32_t* dst_lds = (uint32_t*)(slots + (size_t)s * p.slot_bytes);
#pragma unroll
        for (int k = 0; k < kYuvDepth; k++) {
          const int d = tid + k * kThreads;
          if (d < nd) {
            const YuvAddr a = yuv_addr(p, t, srow, d);
            uint32_t out[3];
            yuv_to_rgb4(p, a, y[s][k], c[s][k], out);
            dst_lds[3 * d] = out[0]; dst_lds[3 * d + 1] = out[1]; dst_lds[3 * d + 2] = out[2];
            if (d == 0) slot_off[s] = 3 * a.o;
          }
        }
      }
    }
  } else {
    for (int s = 0; s < 2 * n_live; s++) {
      const int srow = (s & 1) ? row[s >> 1].y1 : row[s >> 1].y0;
      uint32_t* dst_lds = (uint32_t*)(slots + (size_t)s * p.slot_bytes);
      for (int d = tid; d < nd; d += kThreads) {
        const YuvAddr a = yuv_addr(p, t, srow, d);
        uint32_t y, c[4], out[3];
        load_yuv(p, a, y, c);
        yuv_to_rgb4(p, a, y, c, out);
        dst_lds[3 * d] = out[0]; dst_lds[3 * d + 1] = out[1]; dst_lds[3 * d + 2] = out[2];
        if (d == 0) slot_off[s] = 3 * a.o;
      }
    }
  }
}

// round(65536 x) of the textbook values (include/tubedetr_hip.h): [matrix][full_range] = {yo, cy, crv, cgu, cgv, cbu}
static const int kYuvCoef[2][2][6] = {
    {{16, 76309, 104597, 25675, 53279, 132201}, {0, 65536, 91881, 22553, 46802, 116130}},   // BT.601
    {{16, 76309, 117489, 13975, 34925, 138438}, {0, 65536, 103206, 12276, 30679, 121609}},  // BT.709
};

}  // namespace td
