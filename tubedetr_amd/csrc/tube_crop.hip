// Grounded tubes cropped out of decoded frames: td_tube_crop (include/tubedetr_hip.h has the rule).
//
// clip_resample_kernel (augment.hip) with the window read ON THE DEVICE, per frame, from the tube's box.  The work split is
// the same - a workgroup owns a band of R output rows of a chunk of kFrameChunk frames of one job - and so are the taps, the
// yuv staging conversion and the blend (resample_dev.h): the bytes are td_clip_resample's by construction.  What differs:
//   * the host knows no window, so the grid and the LDS are sized from oh, ow, T and from sw as the widest row a window can
//     stage; R is the largest band whose 2R staged rows of sw pixels fit the LDS budget beside the column table;
//   * per frame every lane evaluates the rule (tube row, span, rounding, margin, clamp, keep_aspect size) from the same few
//     dwords - uniform work, a few dozen instructions, two integer divisions - and the six results go through readfirstlane,
//     so that everything derived from them (loop bounds, addresses of staged rows) is scalar; then the workgroup rebuilds the
//     column table (rw entries) and its band's row entries for that frame.  That costs one tap() per output column and frame
//     where clip_resample_kernel pays one per kFrameChunk frames: ow / 256 integer divisions per lane and frame;
//   * only columns [wx0, wx1) of the band's source rows are staged: cmin = wx0 and the dword count follow the frame;
//   * an empty frame (rh = rw = 0) stages nothing and runs the producing half with no byte inside: zeros, mask 1.
// The band is one contiguous byte range of each of the frame's three planes and of its mask plane, so a lane produces an
// ALIGNED destination dword whatever ow is and wherever the frame starts (3 oh ow need not be a multiple of 4); only a
// band's first / last partial dword falls back to byte stores.  valid[t] and windows[t] are written by the workgroup of
// band 0.  LDS: the column table is read at consecutive entries by consecutive lanes (8-byte entries: conflict-free per
// half wave); the taps are byte reads of the staged rows at strides of the resampling ratio, as in clip_resample_kernel.
// Steps 1 - 5 of the rule, the job search and the host's plane checks and launch are the family's: frame_jobs.h.
#include <algorithm>

#include "resample_dev.h"

namespace td {

namespace {

struct CropParams {
  const unsigned char* src;     // rgb24 pixels, or Y
  const unsigned char* plane1;  // U (I420), interleaved UV (NV12)
  const unsigned char* plane2;  // V (I420)
  long long src_frame_stride;
  long long src_bytes, bytes1, bytes2;  // extents of the job's planes: no load touches a byte outside them
  int pitch, pitch1, pitch2;
  int fmt;
  int yo, cy, crv, cgu, cgv, cbu;
  int T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  int n_tube;
  int oh, ow, margin_num, margin_den, keep_aspect;
  unsigned char* dst;
  unsigned char* mask;
  unsigned char* valid;
  int* windows;
  int slot_bytes;  // LDS bytes of one staged source row of sw pixels
  int R, nbands, block_begin;
  int cmin, nd;    // per frame, set by the kernel in its own copy: first staged column (wx0), staged Y dwords of a row
};

struct Window { int wy0, wx0, ch, cw, rh, rw; };  // all zero: the frame is empty

// the header's rule, steps 1 - 6, for frame t (uniform over the workgroup)
__device__ __forceinline__ Window frame_window(const CropParams& p, int t) {
  Window w{0, 0, 0, 0, 0, 0};
  const int r = tube_row(p.frame_map, t);
  int x0, y0, x1, y1, wx0, wy0, cw, ch;
  if (r >= 0 && r < p.n_tube && row_in_span(p.span, 0, r) && rounded_box(p.boxes, r, x0, y0, x1, y1) &&
      grow_and_clamp(x0, y0, x1, y1, p.margin_num, p.margin_den, p.sh, p.sw, wx0, wy0, cw, ch)) {
    int rh = p.oh, rw = p.ow;
    if (p.keep_aspect) {  // step 6
      if ((long long)cw * p.oh >= (long long)ch * p.ow) rh = (int)min((long long)p.oh, max(1LL, (2LL * ch * p.ow + cw) / (2LL * cw)));
      else rw = (int)min((long long)p.ow, max(1LL, (2LL * cw * p.oh + ch) / (2LL * ch)));
    }
    w = Window{wy0, wx0, ch, cw, rh, rw};
  }
  w.wy0 = __builtin_amdgcn_readfirstlane(w.wy0); w.wx0 = __builtin_amdgcn_readfirstlane(w.wx0);
  w.ch = __builtin_amdgcn_readfirstlane(w.ch); w.cw = __builtin_amdgcn_readfirstlane(w.cw);
  w.rh = __builtin_amdgcn_readfirstlane(w.rh); w.rw = __builtin_amdgcn_readfirstlane(w.rw);
  return w;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void tube_crop_kernel(const CropParams* __restrict__ tab, int n_jobs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, b = blockIdx.x;
  CropParams p = tab[find_job(tab, n_jobs, b)];
  const int local = b - p.block_begin;
  const int band = local % p.nbands, chunk = local / p.nbands;
  const int yb = band * p.R;
  const int Rb = min(p.R, p.oh - yb);

  ColEntry* col = (ColEntry*)smem;                                     // [ow]
  RowEntry* row = (RowEntry*)(smem + (size_t)p.ow * sizeof(ColEntry));  // [kMaxBand]
  int* slot_off = (int*)(row + kMaxBand);                              // [2 * kMaxBand] row address & 3 of the staged rows
  unsigned char* slots = (unsigned char*)(slot_off + 2 * kMaxBand);    // [2 * R][slot_bytes], 8-byte aligned (dword writes, byte reads)

  const unsigned char* src_end = p.src + p.src_bytes;
  const int t_end = min(p.T, (chunk + 1) * kFrameChunk);
  const int L = p.ow;  // bytes of one destination row
  const int seg_len = Rb * L;
  for (int t = chunk * kFrameChunk; t < t_end; t++) {
    // ---- the frame's window and its tables
    const Window w = frame_window(p, t);
    for (int x = tid; x < w.rw; x += kThreads) {
      int x0, x1;
      float wt;
      tap(x, w.cw, w.rw, x0, x1, wt);
      col[x] = ColEntry{(unsigned short)(3 * x0), (unsigned short)(3 * x1), wt};
    }
    if (tid < Rb) {
      RowEntry e{0, 0, 0.f, 0};
      if (yb + tid < w.rh) {
        tap(yb + tid, w.ch, w.rh, e.y0, e.y1, e.w);
        e.y0 += w.wy0; e.y1 += w.wy0;
      }
      row[tid] = e;
    }
    if (band == 0 && tid == 0) {
      if (p.valid) ((gbyte_ptr)p.valid)[t] = w.rh > 0 ? 1 : 0;
      if (p.windows) {
        TD_GLOBAL int* wp = (TD_GLOBAL int*)p.windows + 6 * (long long)t;
        wp[0] = w.wy0; wp[1] = w.wx0; wp[2] = w.ch; wp[3] = w.cw; wp[4] = w.rh; wp[5] = w.rw;
      }
    }
    __syncthreads();

    // ---- stage columns [wx0, wx0 + cw) of the band's source rows
    const int n_live = min(Rb, w.rh - yb);  // rows of the band that carry pixels (<= 0: padding only)
    p.cmin = w.wx0;
    if (p.fmt != TD_SRC_RGB24) {
      p.nd = (w.cw + 3 + 3) >> 2;  // + 3: the Y row is staged from its address rounded down to a dword
      stage_yuv(p, row, slot_off, slots, t, n_live, tid);
    } else {
      const unsigned char* fsrc = p.src + (long long)t * p.src_frame_stride;
      const int nd = (3 * w.cw + 3 + 3) >> 2;  // + 3: the row is staged from its address rounded down to a dword
      if (nd <= kStageDepth * kThreads) {
        // all loads of the band in flight together (a load-then-LDS-write loop would pay one memory latency per source row)
        uint32_t v[2 * kMaxBand][kStageDepth];
#pragma unroll
        for (int s = 0; s < 2 * kMaxBand; s++) {
          if (s < 2 * n_live) {
            const int srow = (s & 1) ? row[s >> 1].y1 : row[s >> 1].y0;
            const unsigned char* rp = fsrc + (long long)srow * p.pitch + 3 * p.cmin;
            const int o = (int)((uintptr_t)rp & 3);
            if (tid == 0) slot_off[s] = o;
#pragma unroll
            for (int k = 0; k < kStageDepth; k++) {
              const int d = tid + k * kThreads;
              if (d < nd) v[s][k] = load_dword_guarded(rp - o + 4 * d, p.src, src_end);
            }
          }
        }
#pragma unroll
        for (int s = 0; s < 2 * kMaxBand; s++) {
          if (s < 2 * n_live) {
            uint32_t* dst_lds = (uint32_t*)(slots + (size_t)s * p.slot_bytes);
#pragma unroll
            for (int k = 0; k < kStageDepth; k++) {
              const int d = tid + k * kThreads;
              if (d < nd) dst_lds[d] = v[s][k];
            }
          }
        }
      } else {
        for (int s = 0; s < 2 * n_live; s++) {
          const int srow = (s & 1) ? row[s >> 1].y1 : row[s >> 1].y0;
          const unsigned char* rp = fsrc + (long long)srow * p.pitch + 3 * p.cmin;
          const int o = (int)((uintptr_t)rp & 3);
          uint32_t* dst_lds = (uint32_t*)(slots + (size_t)s * p.slot_bytes);
          for (int d = tid; d < nd; d += kThreads) dst_lds[d] = load_dword_guarded(rp - o + 4 * d, p.src, src_end);
          if (tid == 0) slot_off[s] = o;
        }
      }
    }
    __syncthreads();

    // ---- produce the band, one aligned destination dword per lane and step: three colour planes, then the mask
    const int n_planes = p.mask ? 4 : 3;
    for (int pl = 0; pl < n_planes; pl++) {
      unsigned char* base;
      if (pl < 3) base = p.dst + (((long long)t * 3 + pl) * p.oh + yb) * p.ow;
      else base = p.mask + ((long long)t * p.oh + yb) * p.ow;
      const int head = (int)((uintptr_t)base & 3);
      const int ndw = (head + seg_len + 3) >> 2;
      for (int d = tid; d < ndw; d += kThreads) {
        const int f0 = 4 * d - head;
        uint32_t packed = 0;
        int r_cur = -1;  // row whose weight and staged-row pointers are held (a dword rarely straddles two rows)
        float wy = 0.f;
        const unsigned char *r0 = nullptr, *r1 = nullptr;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int f = f0 + j;
          const int r = (f >= L) + (f >= 2 * L) + (f >= 3 * L);  // kMaxBand = 4
          const int x = f - r * L;
          const bool inside = f >= 0 && f < seg_len && x < w.rw && yb + r < w.rh;
          uint32_t v = 0;
          if (pl == 3) v = (f >= 0 && f < seg_len && !inside) ? 1u : 0u;
          else if (inside) {
            if (r != r_cur) {
              r_cur = r;
              wy = row[r].w;
              r0 = slots + (size_t)(2 * r) * p.slot_bytes + slot_off[2 * r];
              r1 = slots + (size_t)(2 * r + 1) * p.slot_bytes + slot_off[2 * r + 1];
            }
            v = blend_taps(col[x], r0, r1, wy, pl);
          }
          packed |= v << (8 * j);
        }
        unsigned char* a = base - head + 4 * d;
        if (f0 >= 0 && f0 + 4 <= seg_len) *(TD_GLOBAL uint32_t*)a = packed;
        else {
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (f0 + j >= 0 && f0 + j < seg_len) ((gbyte_ptr)a)[j] = (unsigned char)(packed >> (8 * j));
        }
      }
    }
    __syncthreads();  // the next frame rewrites the tables and the slots
  }
}

namespace {

constexpr int kMaxOut = 4096;

}  // namespace

}  // namespace td

using namespace td;

extern "C" size_t td_tube_crop_table_bytes(int n_jobs) { return table_bytes<CropParams>(n_jobs); }

extern "C" int td_tube_crop(const td_crop_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_crop";
  if (int rc = check_workspace<CropParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  CropParams* host = (CropParams*)table_host;
  int n = 0;
  long long blocks = 0;
  size_t lds = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_crop_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.matrix == TD_MATRIX_BT601 || j.matrix == TD_MATRIX_BT709, "%s: job %d: unknown matrix %d", who, i, j.matrix);
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.full_range == 0 || j.full_range == 1, "%s: job %d: full_range %d is not 0 or 1", who, i, j.full_range);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sh <= kMaxSide, "%s: job %d: sh = %d outside 1..%d", who, i, j.sh, kMaxSide);
    TD_REQUIRE(j.sw > 0 && j.sw <= kMaxSrcCols, "%s: job %d: sw = %d outside 1..%d (a window can be the whole row)", who, i, j.sw, kMaxSrcCols);
    TD_REQUIRE(j.oh > 0 && j.oh <= kMaxOut, "%s: job %d: oh = %d outside 1..%d", who, i, j.oh, kMaxOut);
    TD_REQUIRE(j.ow > 0 && j.ow <= kMaxOut, "%s: job %d: ow = %d outside 1..%d", who, i, j.ow, kMaxOut);
    TD_REQUIRE(j.n_tube >= 1, "%s: job %d: n_tube = %d is below 1", who, i, j.n_tube);
    TD_REQUIRE(j.margin_den >= 1 && j.margin_den <= kMaxMarginDen, "%s: job %d: margin_den = %d outside 1..%d", who, i, j.margin_den, kMaxMarginDen);
    TD_REQUIRE(j.margin_num >= 0 && j.margin_num <= 4 * j.margin_den, "%s: job %d: margin_num = %d outside 0..4 margin_den = %d", who, i, j.margin_num, 4 * j.margin_den);
    TD_REQUIRE(j.keep_aspect == 0 || j.keep_aspect == 1, "%s: job %d: keep_aspect %d is not 0 or 1", who, i, j.keep_aspect);
    TD_REQUIRE(j.boxes, "%s: job %d: boxes is null", who, i);
    TD_REQUIRE(j.dst, "%s: job %d: dst is null", who, i);
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet src{"", {j.plane0, j.plane1, j.plane2}, {j.pitch0, j.pitch1, j.pitch2}, j.frame_stride};
    if (int rc = check_planes(who, i, g, &src, 1)) return rc;
    if (j.T == 0) continue;
    CropParams p{};
    p.src = (const unsigned char*)j.plane0; p.pitch = j.pitch0; p.src_bytes = plane_extent(g, 0, j.pitch0, j.frame_stride, j.T);
    if (g.n_planes > 1) { p.plane1 = (const unsigned char*)j.plane1; p.pitch1 = j.pitch1; p.bytes1 = plane_extent(g, 1, j.pitch1, j.frame_stride, j.T); }
    if (g.n_planes > 2) { p.plane2 = (const unsigned char*)j.plane2; p.pitch2 = j.pitch2; p.bytes2 = plane_extent(g, 2, j.pitch2, j.frame_stride, j.T); }
    p.src_frame_stride = j.frame_stride;
    p.fmt = j.fmt;
    if (j.fmt != TD_SRC_RGB24) {
      const int* k = kYuvCoef[j.matrix][j.full_range];
      p.yo = k[0]; p.cy = k[1]; p.crv = k[2]; p.cgu = k[3]; p.cgv = k[4]; p.cbu = k[5];
    }
    p.T = j.T; p.sh = j.sh; p.sw = j.sw;
    p.boxes = j.boxes; p.span = j.span; p.frame_map = j.frame_map; p.n_tube = j.n_tube;
    p.oh = j.oh; p.ow = j.ow; p.margin_num = j.margin_num; p.margin_den = j.margin_den; p.keep_aspect = j.keep_aspect;
    p.dst = (unsigned char*)j.dst; p.mask = (unsigned char*)j.mask; p.valid = (unsigned char*)j.valid; p.windows = j.windows;
    // the widest row a window can stage: all sw columns, from an address rounded down to a dword (+ 3)
    p.slot_bytes = j.fmt == TD_SRC_RGB24 ? (3 * j.sw + 3 + 15) & ~15 : (12 * ((j.sw + 3 + 3) >> 2) + 15) & ~15;
    const size_t fixed = (((size_t)j.ow * sizeof(ColEntry) + kMaxBand * sizeof(RowEntry) + 2 * kMaxBand * sizeof(int)) + 15) & ~(size_t)15;
    p.R = kMaxBand;
    while (p.R > 1 && fixed + 2 * (size_t)p.R * p.slot_bytes > kMaxLds) p.R >>= 1;
    const size_t need = fixed + 2 * (size_t)p.R * p.slot_bytes;
    TD_REQUIRE(need <= kMaxLds, "%s: job %d needs %zu bytes of LDS: sw = %d and ow = %d are too large together", who, i, need, j.sw, j.ow);
    lds = std::max(lds, need);
    p.nbands = cdiv(j.oh, p.R);
    if (int rc = add_blocks(who, blocks, (long long)p.nbands * cdiv(j.T, kFrameChunk), p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_crop_kernel, blocks, lds, host, table_dev, n, stream, who);
}
