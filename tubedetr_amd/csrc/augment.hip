// Device-side clip augmentation: td_clip_resample (include/tubedetr_hip.h).
//
// Pure data movement: every source byte of the window is read once from HBM (rows that two output rows share come
// from L2), every output byte written once.  One workgroup owns a BAND of R consecutive output rows of one job for a
// chunk of its frames:
//   * the per-column (byte offset, byte offset, weight) triples and the per-row (row, row, weight) triples are the same for
//     every frame and channel of the job: they are computed ONCE per workgroup into LDS, from exact integer coordinates
//     ((2x + 1) sw - rw over 2 rw); the only integer divisions of the kernel are those, one per column / row;
//   * per frame, the 2R source rows of the band are staged into LDS with aligned dword loads (rgb24 rows are not
//     dword-aligned: each row is staged from its address rounded down, the remainder is kept per row) - all loads of the
//     band are issued before the first LDS write, so a band pays one memory latency per frame, not one per row - and the
//     four taps of an output byte are LDS byte reads;
//   * the band is ONE contiguous byte range of every destination plane (full-width rows), so a lane produces the four
//     bytes of an ALIGNED destination dword whatever W is, finds each byte's row by compares and stores 4 bytes; only a
//     band's first / last partial dword falls back to byte stores (its other bytes belong to the neighbour band).
//
// td_clip_resample_src adds the source format (I420 / NV12 beside rgb24): the same kernel, instantiated on a job record that
// carries the planes.  Only the staging step differs: a lane takes the 4 pixels of one ALIGNED Y dword and their 2 or 3
// chroma samples (aligned dwords again, funnel-shifted to the sample), converts them by the header's integer rule and
// writes the 12 rgb bytes into the slot - so the slots hold what the rgb24 staging would have put there from the
// converted frame, and the tables and the producing half are shared: bit equality with the rgb24 path by construction.
// Every plane has its own extent guard.  The 3 dword stores of a lane go to dwords 3d, 3d + 1, 3d + 2: a stride of 3
// dwords over the lanes, coprime with the 32 banks of a store, so each of the three is conflict-free.
// tap(), the yuv staging and the blend live in resample_dev.h: td_tube_crop (tube_crop.hip) is defined by this kernel's bytes and shares them;
// the job search, the plane geometry and the table upload + launch are every job-table kernel's: frame_jobs.h.
#include <algorithm>
#include <type_traits>

#include "resample_dev.h"

namespace td {

struct ResampleParams {
  const unsigned char* src;
  unsigned char* dst;
  unsigned char* mask;
  long long src_frame_stride;
  long long src_bytes;  // extent of the job's source from `src`: no load touches a byte outside it
  int pitch, T, sh, sw, flip, rh, rw, wy, wx, wh, ww;
  int planar, frame_off, H, W;  // planar = 0: H = wh, W = ww
  int cmin;                     // first (flipped) source column any output column of the window reads
  int slot_bytes;               // LDS bytes of one staged source row
  int R, nbands, block_begin;
};

// td_clip_resample_src: the job record + the source format.  RGB24: the base describes the job, as in td_clip_resample.
// I420 / NV12: src / pitch / src_bytes are the Y plane's; a slot holds 12 bytes per staged Y dword.
struct SrcParams : ResampleParams {
  const unsigned char* plane1;  // U (I420), interleaved UV (NV12)
  const unsigned char* plane2;  // V (I420)
  long long bytes1, bytes2;     // extents of the job's chroma planes from plane1 / plane2
  int pitch1, pitch2;
  int fmt;
  int nd;                       // staged Y dwords of one source row
  int yo, cy, crv, cgu, cgv, cbu;
};

// P = ResampleParams: rgb24 sources only (td_clip_resample); P = SrcParams: the job says (td_clip_resample_src)
template <typename P>
__global__ __launch_bounds__(kThreads) void clip_resample_kernel(const P* __restrict__ tab, int n_jobs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const P p = tab[find_job(tab, n_jobs, b)];
  const int local = b - p.block_begin;
  const int band = local % p.nbands, chunk = local / p.nbands;
  const int yb = band * p.R;
  const int rows_total = p.planar ? p.H : p.wh;
  const int Rb = min(p.R, rows_total - yb);

  ColEntry* col = (ColEntry*)smem;                                    // [W]
  RowEntry* row = (RowEntry*)(smem + (size_t)p.W * sizeof(ColEntry));  // [kMaxBand]
  int* slot_off = (int*)(row + kMaxBand);                             // [2 * kMaxBand] row address & 3 of the staged rows
  unsigned char* slots = (unsigned char*)(slot_off + 2 * kMaxBand);   // [2 * R][slot_bytes], 8-byte aligned (dword writes, byte reads)

  for (int x = tid; x < p.ww; x += kThreads) {
    int x0, x1;
    float w;
    tap(p.wx + x, p.sw, p.rw, x0, x1, w);
    if (p.flip) { x0 = p.sw - 1 - x0; x1 = p.sw - 1 - x1; }
    col[x] = ColEntry{(unsigned short)(3 * (x0 - p.cmin)), (unsigned short)(3 * (x1 - p.cmin)), w};
  }
  if (tid < Rb) {
    RowEntry e{0, 0, 0.f, 0};
    if (yb + tid < p.wh) tap(p.wy + yb + tid, p.sh, p.rh, e.y0, e.y1, e.w);
    row[tid] = e;
  }
  __syncthreads();

  const unsigned char* src_end = p.src + p.src_bytes;
  const int t_end = min(p.T, (chunk + 1) * kFrameChunk);
  const int L = p.planar ? p.W : 3 * p.ww;  // bytes of one destination row
  const int seg_len = Rb * L;
  const int n_live = min(Rb, p.wh - yb);    // rows of the band that carry pixels (<= 0: padding only)
  for (int t = chunk * kFrameChunk; t < t_end; t++) {
    const unsigned char* fsrc = p.src + (long long)t * p.src_frame_stride;
    // ---- stage the band's source rows
    const int nd = p.slot_bytes >> 2;
    bool yuv = false;
    if constexpr (std::is_same<P, SrcParams>::value) yuv = p.fmt != TD_SRC_RGB24;
    if (yuv) {
      if constexpr (std::is_same<P, SrcParams>::value) stage_yuv(p, row, slot_off, slots, t, n_live, tid);
    } else if (nd <= kStageDepth * kThreads) {
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
    __syncthreads();
    // ---- produce the band, one aligned destination dword per lane and step
    const int n_planes = p.planar ? 4 : 1;
    for (int pl = 0; pl < n_planes; pl++) {
      unsigned char* base;
      if (!p.planar) base = p.dst + ((long long)t * p.wh + yb) * L;
      else if (pl < 3) base = p.dst + (((long long)(p.frame_off + t) * 3 + pl) * p.H + yb) * p.W;
      else base = p.mask + ((long long)(p.frame_off + t) * p.H + yb) * p.W;
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
          const int bx = f - r * L;
          int x = bx, c = pl;
          if (!p.planar) { x = bx / 3; c = bx - 3 * x; }
          const bool inside = f >= 0 && f < seg_len && x < p.ww && yb + r < p.wh;
          uint32_t v = 0;
          if (pl == 3) v = (f >= 0 && f < seg_len && !inside) ? 1u : 0u;
          else if (inside) {
            if (r != r_cur) {
              r_cur = r;
              wy = row[r].w;
              r0 = slots + (size_t)(2 * r) * p.slot_bytes + slot_off[2 * r];
              r1 = slots + (size_t)(2 * r + 1) * p.slot_bytes + slot_off[2 * r + 1];
            }
            v = blend_taps(col[x], r0, r1, wy, c);
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
    __syncthreads();  // the next frame's staging overwrites the slots
  }
}

static void set_format(ResampleParams&, const td_resample_src_job&, int) {}
static void set_format(SrcParams& p, const td_resample_src_job& j, int ncols) {
  p.fmt = j.fmt;
  if (j.fmt == TD_SRC_RGB24) return;
  const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
  p.src_bytes = plane_extent(g, 0, j.pitch0, j.frame_stride, j.T);
  p.plane1 = (const unsigned char*)j.plane1; p.pitch1 = j.pitch1; p.bytes1 = plane_extent(g, 1, j.pitch1, j.frame_stride, j.T);
  if (j.fmt == TD_SRC_I420) { p.plane2 = (const unsigned char*)j.plane2; p.pitch2 = j.pitch2; p.bytes2 = plane_extent(g, 2, j.pitch2, j.frame_stride, j.T); }
  p.nd = (ncols + 3 + 3) >> 2;  // + 3: the Y row is staged from its address rounded down to a dword
  p.slot_bytes = (12 * p.nd + 15) & ~15;
  const int* k = kYuvCoef[j.matrix][j.full_range];
  p.yo = k[0]; p.cy = k[1]; p.crv = k[2]; p.cgu = k[3]; p.cgv = k[4]; p.cbu = k[5];
}

// validation + job table + launch of both entry points; `legacy`: the jobs came through td_clip_resample (its messages)
static const td_resample_src_job& widen(const td_resample_src_job& j) { return j; }
static td_resample_src_job widen(const td_resample_job& j) {  // the same job in the wider record, format rgb24
  td_resample_src_job s{};
  s.plane0 = j.src; s.frame_stride = j.src_frame_stride; s.pitch0 = j.src_pitch;
  s.fmt = TD_SRC_RGB24; s.T = j.T; s.sh = j.sh; s.sw = j.sw; s.flip = j.flip; s.rh = j.rh; s.rw = j.rw;
  s.wy = j.wy; s.wx = j.wx; s.wh = j.wh; s.ww = j.ww;
  s.dst = j.dst; s.planar = j.planar; s.frame_off = j.frame_off; s.H = j.H; s.W = j.W; s.mask = j.mask;
  return s;
}

template <typename P, typename J>
static int enqueue(const char* who, bool legacy, const J* jobs, int n_jobs, void* table_host, void* table_dev, td_stream_t stream) {
  P* host = (P*)table_host;
  int n = 0;
  long long blocks = 0;
  size_t lds = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_resample_src_job j = widen(jobs[i]);
    TD_REQUIRE(j.T >= 0, "%s: job %d has a negative frame count T = %d", who, i, j.T);
    if (legacy) {
      TD_REQUIRE(j.plane0 && j.dst, "%s: job %d has a null source or destination", who, i);
    } else {
      TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown source format %d", who, i, j.fmt);
      TD_REQUIRE(j.fmt == TD_SRC_RGB24 || ((j.matrix == TD_MATRIX_BT601 || j.matrix == TD_MATRIX_BT709) && (j.full_range == 0 || j.full_range == 1)),
                 "%s: job %d: unknown colour matrix %d (or full_range %d is not 0 or 1)", who, i, j.matrix, j.full_range);
      TD_REQUIRE(j.plane0, "%s: job %d: plane 0 is null", who, i);
      TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.plane1, "%s: job %d: plane 1 is null", who, i);
      TD_REQUIRE(j.fmt != TD_SRC_I420 || j.plane2, "%s: job %d: plane 2 is null", who, i);
      TD_REQUIRE(j.dst, "%s: job %d has a null destination", who, i);
    }
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.rh > 0 && j.rw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSrcCols && j.rh <= kMaxSide && j.rw <= kMaxSide,
               "%s: job %d: sizes %d x %d -> %d x %d outside 1..%d (source rows up to %d pixels)", who, i, j.sh, j.sw, j.rh, j.rw, kMaxSide, kMaxSrcCols);
    TD_REQUIRE(j.wy >= 0 && j.wx >= 0 && j.wh > 0 && j.ww > 0 && j.wy + (long long)j.wh <= j.rh && j.wx + (long long)j.ww <= j.rw,
               "%s: job %d: window (%d, %d, %d, %d) outside the resized image %d x %d", who, i, j.wy, j.wx, j.wh, j.ww, j.rh, j.rw);
    if (legacy) {
      TD_REQUIRE(j.pitch0 >= 3 * j.sw && j.frame_stride >= (long long)j.pitch0 * (j.sh - 1) + 3 * j.sw,
                 "%s: job %d: row pitch %d / frame stride %lld too small for %d x %d rgb24", who, i, j.pitch0, j.frame_stride, j.sh, j.sw);
    } else {
      const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);  // this entry point's own wording and order: all pitches, then all strides
      const int pitch[3] = {j.pitch0, j.pitch1, j.pitch2};
      for (int k = 0; k < g.n_planes; k++)
        TD_REQUIRE(pitch[k] >= g.row_bytes[k], "%s: job %d: pitch %d of plane %d is below its row of %d bytes", who, i, pitch[k], k, g.row_bytes[k]);
      for (int k = 0; k < g.n_planes; k++)
        TD_REQUIRE(j.frame_stride >= plane_extent(g, k, pitch[k]),
                   "%s: job %d: frame stride %lld is smaller than plane %d needs (%d rows of pitch %d)", who, i, j.frame_stride, k, g.rows[k], pitch[k]);
    }
    TD_REQUIRE(j.flip == 0 || j.flip == 1, "%s: job %d: flip must be 0 or 1", who, i);
    if (j.planar)
      TD_REQUIRE(j.mask && j.H >= j.wh && j.W >= j.ww && j.H <= kMaxSide && j.W <= kMaxSide && j.frame_off >= 0,
                 "%s: job %d: planar destination needs a mask, frame_off >= 0 and H x W = %d x %d >= the window %d x %d", who, i, j.H, j.W, j.wh, j.ww);
    if (j.T == 0) continue;
    P p{};
    p.src = (const unsigned char*)j.plane0; p.dst = (unsigned char*)j.dst; p.mask = (unsigned char*)j.mask;
    p.src_frame_stride = j.frame_stride;
    p.src_bytes = (long long)(j.T - 1) * j.frame_stride + (long long)(j.sh - 1) * j.pitch0 + 3LL * j.sw;
    p.pitch = j.pitch0; p.T = j.T; p.sh = j.sh; p.sw = j.sw; p.flip = j.flip; p.rh = j.rh; p.rw = j.rw;
    p.wy = j.wy; p.wx = j.wx; p.wh = j.wh; p.ww = j.ww;
    p.planar = j.planar ? 1 : 0; p.frame_off = j.frame_off;
    p.H = j.planar ? j.H : j.wh; p.W = j.planar ? j.W : j.ww;
    // source columns the window reads: first tap of its first column .. second tap of its last (same integers as the kernel's tap())
    auto first_tap = [&](int v) { const long long num = (2LL * v + 1) * j.sw - j.rw; return num > 0 ? (int)(num / (2LL * j.rw)) : 0; };
    const int c_lo = first_tap(j.wx), c_hi = std::min(first_tap(j.wx + j.ww - 1) + 1, j.sw - 1);
    p.cmin = j.flip ? j.sw - 1 - c_hi : c_lo;
    const int ncols = c_hi - c_lo + 1;
    p.slot_bytes = (3 * ncols + 3 + 15) & ~15;  // + 3: the row is staged from its address rounded down to a dword
    set_format(p, j, ncols);                    // I420 / NV12: the Y plane's extent, the chroma planes, 12 bytes per staged Y dword
    const size_t fixed = (((size_t)p.W * sizeof(ColEntry) + kMaxBand * sizeof(RowEntry) + 2 * kMaxBand * sizeof(int)) + 15) & ~(size_t)15;
    p.R = kMaxBand;
    while (p.R > 1 && fixed + 2 * (size_t)p.R * p.slot_bytes > kMaxLds) p.R >>= 1;
    const size_t need = fixed + 2 * (size_t)p.R * p.slot_bytes;
    TD_REQUIRE(need <= kMaxLds, "%s: job %d needs %zu bytes of LDS (destination row of %d pixels, %d source columns)", who, i, need, p.W, ncols);
    lds = std::max(lds, need);
    p.nbands = cdiv(p.H, p.R);
    if (int rc = add_blocks(who, blocks, (long long)p.nbands * cdiv(p.T, kFrameChunk), p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(clip_resample_kernel<P>, blocks, lds, host, table_dev, n, stream, who);
}

}  // namespace td

using namespace td;

extern "C" size_t td_clip_resample_table_bytes(int n_jobs) { return table_bytes<ResampleParams>(n_jobs); }

extern "C" int td_clip_resample(const td_resample_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes_, td_stream_t stream) {
  if (int rc = check_workspace<ResampleParams>("td_clip_resample", jobs, n_jobs, table_host, table_dev, table_bytes_)) return rc;
  return enqueue<ResampleParams>("td_clip_resample", true, jobs, n_jobs, table_host, table_dev, stream);
}

extern "C" size_t td_clip_resample_src_table_bytes(int n_jobs) { return table_bytes<SrcParams>(n_jobs); }

extern "C" int td_clip_resample_src(const td_resample_src_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes_, td_stream_t stream) {
  if (int rc = check_workspace<SrcParams>("td_clip_resample_src", jobs, n_jobs, table_host, table_dev, table_bytes_)) return rc;
  return enqueue<SrcParams>("td_clip_resample_src", false, jobs, n_jobs, table_host, table_dev, stream);
}
