// td_replica_maps: every index vector of one durations pattern (ragged clip counts included) in ONE launch, from a device table of
// b records (duration, first_clip, clips).  All of them are closed forms of (video, frame-in-video, token): a clip's frames are a
// contiguous frame range (owner is non-decreasing and every clip owns at least one frame), so the CSR lists of the backward's
// segment sums need neither a sort nor a prefix scan over clips.  One thread per (frame, token) and per (clip, token); the table
// (plus each video's first valid frame: a serial sum by one thread of every workgroup, which is why b is bounded by 256 - a step holds
// tens of videos) sits in LDS; plain vector stores only.
#include "td_common.h"

using namespace td;

namespace {

constexpr int kMaxVideos = 256;

struct MapsOut {
  td_replica_maps_out o;
};

__global__ __launch_bounds__(256) void replica_maps_kernel(const int* __restrict__ table, int b, int t, int k, int hw, int L, int n, MapsOut P) {
  extern __shared__ int lds[];  // [b] duration | [b] first_clip | [b] clips | [b] first valid frame (packed frame numbering)
  int* dur = lds;
  int* first = lds + b;
  int* cnt = lds + 2 * b;
  int* vbase = lds + 3 * b;
  for (int i = threadIdx.x; i < b; i += blockDim.x) {
    dur[i] = table[3 * i];
    first[i] = table[3 * i + 1];
    cnt[i] = table[3 * i + 2];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < b; ++i) {
      vbase[i] = acc;
      acc += dur[i];
    }
  }
  __syncthreads();
  const td_replica_maps_out& o = P.o;
  const int S = hw + L, F = b * t;
  const long long frame_items = (long long)F * S, clip_items = (long long)n * S;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < frame_items) {
    const int f = (int)(e / S), s = (int)(e - (long long)f * S);
    const int i = f / t, j = f - i * t;
    const int ci = cnt[i];
    const int lc = min(j / k, ci - 1);   // a time-padded frame takes its video's last clip
    const int c = first[i] + lc;
    if (s == 0) {
      if (o.owner) o.owner[f] = c;
      if (o.vid_of_frame) o.vid_of_frame[f] = i;
      if (o.query_mask) o.query_mask[f] = (j >= dur[i] && j > 0) ? 1 : 0;
      if (j < dur[i]) {
        if (o.frame_dest) o.frame_dest[vbase[i] + j] = f;
        if (o.clip_of) o.clip_of[vbase[i] + j] = c;
      }
    }
    if (o.all_src) {
      const int f0 = i * t + lc * k;                           // first frame of clip c
      const int count = lc < ci - 1 ? k : t - (ci - 1) * k;    // its frames (the last clip also owns the time padding)
      const int q = f - f0;
      const int frow = f * S + s, crow = c * S + s;
      o.all_src[frow] = crow;
      o.seg_all_idx[S * f0 + s * count + q] = frow;
      if (s < hw) {
        o.vis_src[f * hw + s] = crow;
        o.vis_dst[f * hw + s] = frow;
        o.seg_vis_idx[hw * f0 + s * count + q] = frow;
      } else {
        const int l = s - hw;
        o.txt_src[f * L + l] = crow;
        o.txt_dst[f * L + l] = frow;
        o.seg_txt_idx[L * f0 + l * count + q] = frow;
      }
    }
  } else if (e < frame_items + clip_items) {
    const long long r = e - frame_items;
    const int c = (int)(r / S), s = (int)(r - (long long)c * S);
    int lo = 0, hi = b - 1;  // video of clip c: the last record whose first clip is <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    if (s == 0 && o.vid_of_clip) o.vid_of_clip[c] = i;
    if (o.all_src) {
      const int ci = cnt[i], lc = c - first[i];
      const int f0 = i * t + lc * k;
      const int count = lc < ci - 1 ? k : t - (ci - 1) * k;
      o.seg_all_ptr[c * S + s] = S * f0 + s * count;
      if (s < hw) {
        o.iota_vis[c * hw + s] = c * hw + s;
        o.clip_vis[c * hw + s] = c * S + s;
        o.seg_vis_ptr[c * hw + s] = hw * f0 + s * count;
      } else {
        const int l = s - hw;
        o.clip_txt[c * L + l] = c * S + s;
        o.seg_txt_ptr[c * L + l] = L * f0 + l * count;
      }
      if (r == 0) {  // the CSR lists' closing entries
        o.seg_all_ptr[n * S] = F * S;
        o.seg_vis_ptr[n * hw] = F * hw;
        o.seg_txt_ptr[n * L] = F * L;
      }
    }
  }
}

}  // namespace

extern "C" int td_replica_maps(const int* table, int b, int t, int k, int hw, int L, int n_clips, const td_replica_maps_out* out, td_stream_t stream) {
  TD_REQUIRE(table && out, "td_replica_maps: null pointer");
  TD_REQUIRE(b >= 1 && b <= kMaxVideos && t >= 1 && k >= 1 && n_clips >= b, "td_replica_maps: b=%d (1..%d), t=%d, k=%d, n_clips=%d out of range", b, kMaxVideos, t, k, n_clips);
  TD_REQUIRE(hw >= 1 && L >= 0, "td_replica_maps: hw=%d, L=%d out of range", hw, L);
  const td_replica_maps_out& o = *out;
  const int n_maps = !!o.vis_src + !!o.vis_dst + !!o.txt_src + !!o.txt_dst + !!o.all_src + !!o.iota_vis + !!o.clip_vis + !!o.clip_txt + !!o.seg_vis_idx +
                     !!o.seg_vis_ptr + !!o.seg_txt_idx + !!o.seg_txt_ptr + !!o.seg_all_idx + !!o.seg_all_ptr;
  TD_REQUIRE(n_maps == 0 || L >= 1, "td_replica_maps: the replication maps need at least one text token (L=%d)", L);
  TD_REQUIRE(n_maps == 0 || n_maps == 14, "td_replica_maps: the 14 replication maps are written together (all of their pointers, or none)");
  const long long F = (long long)b * t, S = hw + L;
  TD_REQUIRE(F * S < (1ll << 31), "td_replica_maps: %lld frames of %lld rows exceed 32-bit row indices", F, S);
  const long long items = (F + n_clips) * S;
  MapsOut P;
  P.o = o;
  hipStream_t st = (hipStream_t)stream;
  replica_maps_kernel<<<(unsigned)((items + 255) / 256), 256, (size_t)4 * b * sizeof(int), st>>>(table, b, t, k, hw, L, n_clips, P);
  return check_launch("td_replica_maps");
}
