// How a td_conv_wgrad / td_conv_wgrad_batch call is laid out on the device: kernel, tile class, reduction splits, work-item length, owning
// XCD and first slot of every job, the XCD index and grid of every launch, which outputs the library zero-fills - a pure function of the job
// array (pointers only tested for NULL), the dtype, the CU count, the deterministic flag and the TD_WGRAD_* knobs.  Host-only plain C++ - no
// HIP call, no getenv, no statics - so that the plan is asserted on a machine without a GPU (tests/test_wgrad_plan_cpu.py through
// td_conv_wgrad_batch_plan).  Every argument check of the two calls is made here, before anything is enqueued.  conv_wgrad.hip launches what
// these functions return.
#pragma once
#include <algorithm>
#include <vector>

#include "gemm_route.h"

namespace td {

// one job: the public record and what only the launcher needs
struct WgradJobPlan : td_wgrad_plan_job {
  int M, K;                     // reduction rows, columns of the im2col operand (R * S * C)
  uint32_t g_bytes, src_bytes;  // buffer-descriptor ranges of the operands
};

// the checks and the geometry every weight gradient shares; tn x tk = the 128 x 128 tile grid
inline int wgrad_geometry(const td_conv_desc* d, int ldg, int dtype, const char* who, WgradJobPlan& q) {
  int rc = validate(d, dtype, who);
  if (rc) return rc;
  const int vec = dtype == TD_BF16 ? 8 : 4;
  TD_REQUIRE(d->mode == 0 && !d->aniso, "%s: isotropic forward geometry expected", who);
  TD_REQUIRE(d->Nc % vec == 0 && ldg % vec == 0, "%s: Nc=%d / ldg=%d must be multiples of %d", who, d->Nc, ldg, vec);
  memset(&q, 0, sizeof(q));
  q.M = d->N * d->Ho * d->Wo;
  q.K = d->R * d->S * d->C;
  const double es = dtype == TD_BF16 ? 2.0 : 4.0;
  const double gb = (double)q.M * ldg * es, sb = (double)d->N * d->Hs * d->Ws * d->C * es;
  TD_REQUIRE(gb < 4294967000.0 && sb < 4294967000.0, "%s: operand exceeds the 4 GiB buffer-descriptor range", who);
  q.g_bytes = (uint32_t)gb;
  q.src_bytes = (uint32_t)sb;
  q.tn = cdiv(d->Nc, 128);
  q.tk = cdiv(q.K, 128);
  q.kernel = (d->R * d->S == 1 && d->stride == 1 && d->pad == 0) ? TD_WGRAD_KERNEL_POINTWISE : TD_WGRAD_KERNEL_GENERAL;
  return TD_OK;
}

// `splits` wanted -> rows per split (whole stages of 64 / 32 rows) and the splits that leaves
inline void wgrad_set_splits(WgradJobPlan& q, int splits, int dtype, bool det) {
  const int mk = dtype == TD_BF16 ? 64 : 32;
  if (splits < 1) splits = 1;
  if (det) splits = 1;  // one workgroup per output tile walks the whole reduction: no atomics between splits, a fixed summation order
  q.mper = cdiv(cdiv(q.M, splits), mk) * mk;
  q.splits = cdiv(q.M, q.mper);
}

// td_conv_wgrad / td_conv_wgrad_bias: one launch of grid (tn, tk, splits); splits < 1 = chosen here
inline int plan_wgrad_single(const td_conv_desc* d, int ldg, int dtype, int splits, bool det, const GemmKnobs& kn, WgradJobPlan& q) {
  int rc = wgrad_geometry(d, ldg, dtype, "td_conv_wgrad", q);
  if (rc) return rc;
  if (splits < 1) {
    // about one workgroup per CU (TD_WGRAD_BLOCKS, default 256), at least 8 reduction stages per split.
    // measured: 192-256 workgroups beat 512-1536 (fewer fp32 atomics per output tile)
    splits = kn.wgrad_blocks / (q.tn * q.tk);  // four stages take one workgroup per CU: never a second round
    splits = std::min(splits, cdiv(q.M, 8 * (dtype == TD_BF16 ? 64 : 32)));
  }
  wgrad_set_splits(q, splits, dtype, det);
  return TD_OK;
}

// td_conv_wgrad_batch.  Jobs flagged `accumulate` add to what the overwriting jobs of the same call wrote: they are a second phase behind
// them.  A phase is up to three launches, one per kernel (general geometry, pointwise, wide tiles), each over a table of its jobs that is
// ordered by owning XCD.  plan[i] belongs to jobs[i]; `launches` has room for 6.
inline int plan_wgrad_batch(const td_wgrad_job* jobs, int n_jobs, int dtype, int n_cu, bool det, const GemmKnobs& kn, WgradJobPlan* plan,
                            td_wgrad_plan_launch* launches, int* n_launches) {
  const int mk = dtype == TD_BF16 ? 64 : 32;
  std::vector<int> order;
  std::vector<double> cost(n_jobs);
  order.reserve(n_jobs);
  int nl = 0;
  for (int phase = 0; phase < 2; ++phase) {
    auto in_phase = [&](int i) { return (jobs[i].accumulate != 0) == (phase != 0); };
    // stages (64 / 32 reduction rows) per work item: total work of the phase in 256 x 256 tile-stages / (3.4 items per CU).  The tiles
    // of all jobs fill the chip; a job is split only to bound the longest work item.  Every split pays an fp32-atomic epilogue (65 536
    // atomics per 256 x 256 tile, 36-byte strided for the 3x3 layers: ~30 % of a 192-stage item), an unsplit trunk leaves 3 000-stage
    // items next to 190-stage ones: measured over the trunk's 93 jobs at 8 clips 8.5 ms at 192 stages per item, 7.1 ms at 512 .. 1024,
    // 10.4 ms unsplit.  Within 192 .. 2048 stages: 512 at 4 clips, ~1000 at 8 (in the network: 80.5 clips/s at 512, 81.1 at 1024).
    double units = 0;
    int members = 0;
    for (int i = 0; i < n_jobs; ++i) {
      if (!in_phase(i)) continue;
      const td_conv_desc& d = jobs[i].d;
      units += (double)cdiv(d.Nc, 128) * cdiv(d.R * d.S * d.C, 128) / 4.0 * cdiv(d.N * d.Ho * d.Wo, mk);
      ++members;
    }
    if (!members) continue;
    const int item_stages = kn.wgrad_split_stages > 0 ? kn.wgrad_split_stages : (int)std::min(2048.0, std::max(192.0, units / (3.4 * n_cu)));
    for (int i = 0; i < n_jobs; ++i) {
      if (!in_phase(i)) continue;
      const td_wgrad_job& j = jobs[i];
      WgradJobPlan& q = plan[i];
      TD_REQUIRE(j.g && j.src && j.dW, "td_conv_wgrad_batch: job %d has a null pointer", i);
      int rc = wgrad_geometry(&j.d, j.ldg, dtype, "td_conv_wgrad_batch", q);
      if (rc) return rc;
      wgrad_set_splits(q, cdiv(q.M, std::max(1, item_stages) * mk), dtype, det);
      TD_REQUIRE(j.ci_real >= 1 && j.ci_real <= j.d.C, "td_conv_wgrad_batch: job %d: ci_real=%d out of range", i, j.ci_real);
      TD_REQUIRE(!phase || !j.dbias, "td_conv_wgrad_batch: job %d: an accumulating job cannot carry a bias gradient", i);
      q.phase = phase;
      q.out_mode = (q.splits == 1 && !phase) ? 2 : 1;  // plain stores when nobody else touches the tile, else fp32 atomics ...
      q.fill_dw = q.splits > 1 && !phase && !j.prezeroed;  // ... into zeros: the caller's, or a fill enqueued ahead of the launches
      q.fill_dbias = q.fill_dw && j.dbias;
      // wide tiles: bf16, many reduction rows, whole 128-column sub-tiles (see wgrad_wide_body), no fused bias gradient
      const bool wide = kn.wgrad_wide && dtype == TD_BF16 && q.M >= kn.wgrad_wide_min_m && j.d.Nc % 128 == 0 && j.d.C % 128 == 0 && !j.dbias &&
                        j.d.R * j.d.S <= 255 && (j.d.Nc % 256 == 0 || q.K >= 256);
      if (wide) {
        const int gs = j.d.Nc % 256 == 0 ? 2 : 1, xs = q.K >= 256 ? 2 : 1;
        q.cls = (gs - 1) | ((xs - 1) << 1) | (q.kernel == TD_WGRAD_KERNEL_POINTWISE ? 4 : 0);
        q.tn = j.d.Nc / (gs * 128);
        q.tk = cdiv(q.K, xs * 128);
        q.kernel = TD_WGRAD_KERNEL_WIDE;
      }
    }
    for (int k = 0; k < 3; ++k) {
      // one XCD per job, longest job first onto the least loaded XCD; inside an XCD the long work items come first so that the tail
      // of the launch is made of short ones
      auto member = [&](int i) { return in_phase(i) && plan[i].kernel == k; };
      td_wgrad_plan_launch L;
      memset(&L, 0, sizeof(L));
      order.clear();
      for (int i = 0; i < n_jobs; ++i) {
        if (!member(i)) continue;
        const WgradJobPlan& q = plan[i];
        const td_wgrad_job& j = jobs[i];
        order.push_back(i);
        cost[i] = (double)q.tn * q.tk * q.splits * (double)q.mper * ((k == TD_WGRAD_KERNEL_POINTWISE || (q.cls & 4)) ? 1.0 : 1.5) *
                  (k == TD_WGRAD_KERNEL_WIDE && (q.cls & 3) != 3 ? 0.6 : 1.0);  // half-size wide tiles: half the MFMAs, same DMA count
        L.flops += 2.0 * q.M * j.d.Nc * q.K;
        L.bytes += ((double)q.M * j.ldg + (double)j.d.N * j.d.Hs * j.d.Ws * j.d.C) * (dtype == TD_BF16 ? 2.0 : 4.0) +
                   (double)j.d.Nc * j.ci_real * j.d.R * j.d.S * 4.0;
      }
      if (order.empty()) continue;
      L.phase = phase;
      L.kernel = k;
      L.n_jobs = (int)order.size();
      L.item_stages = item_stages;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
      double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i : order) {
        int best = 0;
        for (int x = 1; x < 8; ++x)
          if (load[x] < load[best]) best = x;
        plan[i].xcd = best;
        load[best] += cost[i];
      }
      int pos = 0;
      long long max_slots = 0;
      for (int x = 0; x < 8; ++x) {
        L.start[x] = pos;
        order.clear();  // (from here on: the jobs of XCD x, in job order)
        for (int i = 0; i < n_jobs; ++i)
          if (member(i) && plan[i].xcd == x) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
          return (double)plan[a].mper * jobs[a].d.R * jobs[a].d.S > (double)plan[b].mper * jobs[b].d.R * jobs[b].d.S;
        });
        long long slots = 0;
        for (int i : order) {
          WgradJobPlan& q = plan[i];
          q.first = (int)slots;
          q.launch = nl;
          q.pos = pos++;
          slots += (long long)q.tn * q.tk * q.splits;
        }
        TD_REQUIRE(slots < 200000000LL, "td_conv_wgrad_batch: too many work items");
        L.slots[x] = (int)slots;
        max_slots = std::max(max_slots, slots);
      }
      L.start[8] = pos;
      L.grid = (unsigned)(8 * max_slots);
      L.block = k == TD_WGRAD_KERNEL_WIDE ? 1024 : 256;
      launches[nl++] = L;
    }
  }
  *n_launches = nl;
  return TD_OK;
}

}  // namespace td
