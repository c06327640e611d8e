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
#include <algorithm>

#include "td_common.h"

namespace td {

constexpr int kThreads = 256;
constexpr int kMaxBand = 4;        // output rows per workgroup
constexpr int kStageDepth = 4;     // staged dwords per lane and source row held in registers (rows of up to 1365 pixels take the fast path)
constexpr int kFrameChunk = 4;     // frames per workgroup (amortises the column table)
constexpr int kMaxSide = 16384;    // (2x + 1) * sw stays below 2^30
constexpr int kMaxSrcCols = 8192;  // 3 * (column - cmin) fits the table's 16-bit offsets
constexpr size_t kMaxLds = 64 * 1024;

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

// the table's pointers are loaded from memory, so the compiler cannot see that they are global: say so (global_load / global_store
// instead of flat ones, which also occupy the LDS path that the taps need)
#define TD_GLOBAL __attribute__((address_space(1)))
typedef const TD_GLOBAL unsigned char* gcbyte_ptr;
typedef TD_GLOBAL unsigned char* gbyte_ptr;

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

// 4 bytes at the dword-aligned address a; bytes outside [lo, hi) read as 0 and are never touched
__device__ __forceinline__ uint32_t load_dword_guarded(const unsigned char* a, const unsigned char* lo, const unsigned char* hi) {
  if (a >= lo && a + 4 <= hi) return *(const TD_GLOBAL uint32_t*)a;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (a + j >= lo && a + j < hi) v |= (uint32_t)((gcbyte_ptr)a)[j] << (8 * j);
  return v;
}

__global__ __launch_bounds__(kThreads) void clip_resample_kernel(const ResampleParams* __restrict__ tab, int n_jobs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, b = blockIdx.x;
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {  // last job whose first block is <= b (uniform: scalar loads)
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= b) lo = mid; else hi = mid - 1;
  }
  const ResampleParams p = tab[lo];
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
            const ColEntry ce = col[x];
            const float p00 = (float)r0[ce.off0 + c], p01 = (float)r0[ce.off1 + c], p10 = (float)r1[ce.off0 + c], p11 = (float)r1[ce.off1 + c];
            const float top = fmaf(ce.w, p01 - p00, p00), bot = fmaf(ce.w, p11 - p10, p10);
            v = (uint32_t)(fmaf(wy, bot - top, top) + 0.5f);
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

static size_t table_bytes(int n_jobs) { return (((size_t)n_jobs * sizeof(ResampleParams)) + 255) & ~(size_t)255; }

}  // namespace td

using namespace td;

extern "C" size_t td_clip_resample_table_bytes(int n_jobs) { return n_jobs > 0 ? table_bytes(n_jobs) : 0; }

extern "C" int td_clip_resample(const td_resample_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes_, td_stream_t stream) {
  TD_REQUIRE(jobs && n_jobs > 0 && n_jobs <= 65536, "td_clip_resample: no jobs (or more than 65536)");
  TD_REQUIRE(table_host && table_dev && table_bytes_ >= td_clip_resample_table_bytes(n_jobs),
             "td_clip_resample: job-table workspace missing or smaller than td_clip_resample_table_bytes(%d)", n_jobs);
  ResampleParams* host = (ResampleParams*)table_host;
  int n = 0;
  long long blocks = 0;
  size_t lds = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_resample_job& j = jobs[i];
    TD_REQUIRE(j.T >= 0, "td_clip_resample: job %d has a negative frame count T = %d", i, j.T);
    TD_REQUIRE(j.src && j.dst, "td_clip_resample: job %d has a null source or destination", i);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.rh > 0 && j.rw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSrcCols && j.rh <= kMaxSide && j.rw <= kMaxSide,
               "td_clip_resample: job %d: sizes %d x %d -> %d x %d outside 1..%d (source rows up to %d pixels)", i, j.sh, j.sw, j.rh, j.rw, kMaxSide, kMaxSrcCols);
    TD_REQUIRE(j.wy >= 0 && j.wx >= 0 && j.wh > 0 && j.ww > 0 && j.wy + (long long)j.wh <= j.rh && j.wx + (long long)j.ww <= j.rw,
               "td_clip_resample: job %d: window (%d, %d, %d, %d) outside the resized image %d x %d", i, j.wy, j.wx, j.wh, j.ww, j.rh, j.rw);
    TD_REQUIRE(j.src_pitch >= 3 * j.sw && j.src_frame_stride >= (long long)j.src_pitch * (j.sh - 1) + 3 * j.sw,
               "td_clip_resample: job %d: row pitch %d / frame stride %lld too small for %d x %d rgb24", i, j.src_pitch, j.src_frame_stride, j.sh, j.sw);
    TD_REQUIRE(j.flip == 0 || j.flip == 1, "td_clip_resample: job %d: flip must be 0 or 1", i);
    if (j.planar)
      TD_REQUIRE(j.mask && j.H >= j.wh && j.W >= j.ww && j.H <= kMaxSide && j.W <= kMaxSide && j.frame_off >= 0,
                 "td_clip_resample: job %d: planar destination needs a mask, frame_off >= 0 and H x W = %d x %d >= the window %d x %d", i, j.H, j.W, j.wh, j.ww);
    if (j.T == 0) continue;
    ResampleParams p{};
    p.src = (const unsigned char*)j.src; p.dst = (unsigned char*)j.dst; p.mask = (unsigned char*)j.mask;
    p.src_frame_stride = j.src_frame_stride;
    p.src_bytes = (long long)(j.T - 1) * j.src_frame_stride + (long long)(j.sh - 1) * j.src_pitch + 3LL * j.sw;
    p.pitch = j.src_pitch; p.T = j.T; p.sh = j.sh; p.sw = j.sw; p.flip = j.flip; p.rh = j.rh; p.rw = j.rw;
    p.wy = j.wy; p.wx = j.wx; p.wh = j.wh; p.ww = j.ww;
    p.planar = j.planar ? 1 : 0; p.frame_off = j.frame_off;
    p.H = j.planar ? j.H : j.wh; p.W = j.planar ? j.W : j.ww;
    // source columns the window reads: first tap of its first column .. second tap of its last (same integers as the kernel's tap())
    auto first_tap = [&](int v) { const long long num = (2LL * v + 1) * j.sw - j.rw; return num > 0 ? (int)(num / (2LL * j.rw)) : 0; };
    const int c_lo = first_tap(j.wx), c_hi = std::min(first_tap(j.wx + j.ww - 1) + 1, j.sw - 1);
    p.cmin = j.flip ? j.sw - 1 - c_hi : c_lo;
    const int ncols = c_hi - c_lo + 1;
    p.slot_bytes = (3 * ncols + 3 + 15) & ~15;  // + 3: the row is staged from its address rounded down to a dword
    const size_t fixed = (((size_t)p.W * sizeof(ColEntry) + kMaxBand * sizeof(RowEntry) + 2 * kMaxBand * sizeof(int)) + 15) & ~(size_t)15;
    p.R = kMaxBand;
    while (p.R > 1 && fixed + 2 * (size_t)p.R * p.slot_bytes > kMaxLds) p.R >>= 1;
    const size_t need = fixed + 2 * (size_t)p.R * p.slot_bytes;
    TD_REQUIRE(need <= kMaxLds, "td_clip_resample: job %d needs %zu bytes of LDS (destination row of %d pixels, %d source columns)", i, need, p.W, ncols);
    lds = std::max(lds, need);
    p.nbands = cdiv(p.H, p.R);
    p.block_begin = (int)blocks;
    blocks += (long long)p.nbands * cdiv(p.T, kFrameChunk);
    TD_REQUIRE(blocks < (1LL << 31), "td_clip_resample: too many workgroups");
    host[n++] = p;
  }
  if (n == 0) return TD_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(table_dev, host, (size_t)n * sizeof(ResampleParams), hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("td_clip_resample: job table upload failed");
    return TD_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(clip_resample_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, st, (const ResampleParams*)table_dev, n);
  return check_launch("td_clip_resample");
}
