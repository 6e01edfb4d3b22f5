// The cut of a frame into batches and passes (render_frame's reserve_workspace; included by rtx_hip.hip): plain arithmetic on the frame's sizes. Nothing here touches
// the device, so rt_frame_plan() runs it in tests at the shapes it was tuned for (2^29 paths per pass), which no GPU test can afford.
// A batch is a range of owned pixels whose sampler tables (2 * dims u16 per sample) are built at once; it is rendered in passes of pass_samples consecutive samples of
// all its pixels, ~2^pass_log2 paths per pass. `cap` bounds the paths of any pass of any batch: it is how far the kernels may index the workspace.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
// (after rtx_kernels.h and include/rtx_hip.h: RT_QSHARDS and the RT_ERR_* codes)

struct FramePlanIn {
  unsigned long long owned_pixels;  // a rank may own no rows
  unsigned spp, dims;               // spp: a power of two
  int pass_log2, batch_log2;        // RTX_PASS_LOG2 less the halvings of the allocation retry loop, RTX_BATCH_LOG2
  bool lead_on;                     // RTX_LEAD_BATCH, or 1024 spp
  bool fixed;                       // a frame whose resident sampler tables are built: the cut they were laid out by
  unsigned long long fixed_batch_pixels, fixed_lead_pixels;
  unsigned n_cu;
};
struct FramePlan {
  unsigned long long batch_pixels = 0, lead_pixels = 0, cap = 0;
  unsigned pass_samples = 0, shard_cap = 0;
  size_t n_slots = 0;  // slots of a sharded queue (>= cap: bounce 0 of a fully traced pass uses slot = path id)
  bool multi_batch = false;
};
// The Whitted integrator's pending stack of a pass of `cap` paths (rtx_whitted_launch.h): four 16-byte records per level and path, max_depth - 1 levels, dense.
static inline unsigned long long whitted_stack_bytes(int max_depth, unsigned long long cap) { return 64ull * (unsigned long long)(max_depth > 1 ? max_depth - 1 : 0) * cap; }
// Must the pass be halved for the stack to stay within `budget` bytes? Never below the smallest pass frame_plan_cut makes (2^14 paths: 15 MiB of stack at depth 16).
static inline bool whitted_pass_too_large(int max_depth, unsigned long long cap, int pass_log2, unsigned long long budget) {
  return whitted_stack_bytes(max_depth, cap) > budget && pass_log2 > 14;
}
// The direct-lighting integrator's array tables (rtx_direct_launch.h): 2 * max_depth * n_lights (0,2) tables per pixel under strategy "all" (0), none under "one";
// a table is spp u16 permutation entries and two u32 scrambles.
static inline unsigned direct_n_arrays(int max_depth, int n_lights, int strategy) { return strategy == 0 ? 2u * (unsigned)max_depth * (unsigned)n_lights : 0u; }
static inline unsigned long long direct_table_bytes_per_pixel(unsigned n_arrays, unsigned spp) { return (unsigned long long)n_arrays * ((unsigned long long)spp * 2ull + 8ull); }
// The pixels of a batch: `pixels` halved while the batch's array tables exceed `budget` bytes, never below one workgroup's pixels (64).
static inline unsigned long long direct_chunk_pixels(unsigned n_arrays, unsigned spp, unsigned long long pixels, unsigned long long budget) {
  unsigned long long c = pixels;
  while (c > 64ull && c * direct_table_bytes_per_pixel(n_arrays, spp) > budget) c = std::max<unsigned long long>(64ull, (c + 1ull) / 2ull);
  return c;
}
struct FrameBatch { unsigned long long first, pixels; unsigned pass_samples; };  // owned pixels [first, first + pixels); a short batch: more samples per pass, same paths

static int frame_plan_cut(const FramePlanIn& in, FramePlan& p, const char*& why) {
  if (in.pass_log2 < 14) { why = "not enough free device memory for the smallest pass (2^14 paths)"; return RT_ERR_OOM; }
  const unsigned long long target_paths = 1ull << in.pass_log2, table_bytes_per_pixel = 2ull * in.dims * in.spp * 2ull;
  p.batch_pixels = std::max<unsigned long long>(1, std::min<unsigned long long>(in.owned_pixels, std::min(1ull << in.batch_log2, target_paths)));
  while (p.batch_pixels > 4096 && p.batch_pixels * table_bytes_per_pixel > (16ull << 30)) p.batch_pixels >>= 1;  // <= 16 GiB of tables per buffer
  // A short LEADING batch (RTX_LEAD_BATCH; on at 1024 spp since the end of round 4): the first batch's sampler tables are the only ones no path kernel runs over, so a
  // first batch of an eighth of the others lets the path kernels start early. Measured alone it gained nothing (the NEXT batch's tables are then built under that
  // short batch's kernels on the low-priority stream, where they take 3 - 4x their time alone: S1 883 -> 881 ms, S3 328 -> 353); together with the parallel replay
  // of the shuffles at 1024 spp it does (S1 679.5 -> 667.5 ms, S4 5280 -> 5242).
  p.lead_pixels = 0;
  if (in.lead_on && in.owned_pixels >= (1ull << 16) && in.owned_pixels * in.spp >= (1ull << 27)) p.lead_pixels = std::max<unsigned long long>(1ull << 15, (p.batch_pixels / 8) & ~4095ull);
  if (p.lead_pixels >= in.owned_pixels || p.lead_pixels >= p.batch_pixels) p.lead_pixels = 0;
  // a shard without a leading batch that fits one batch (a 256 x 256 window; 1/8 of a frame on an 8-GPU run) is still cut in two, so that the second half's
  // sampler tables are built under the first half's path kernels; only worth it when there is enough work to hide them under (the rule used to test
  // lead_on instead of lead_pixels, so 2^15 <= owned_pixels < 2^16 at 1024 spp rendered as one batch)
  if (p.lead_pixels == 0 && in.owned_pixels <= p.batch_pixels && in.owned_pixels >= (1ull << 15) && in.owned_pixels * in.spp >= (1ull << 27)) p.batch_pixels = (in.owned_pixels + 1) / 2;
  if (in.fixed) { p.batch_pixels = in.fixed_batch_pixels; p.lead_pixels = in.fixed_lead_pixels; }
  p.pass_samples = (unsigned)std::max<unsigned long long>(1, target_paths / p.batch_pixels);
  if (p.pass_samples > in.spp) p.pass_samples = in.spp;
  p.cap = p.batch_pixels * p.pass_samples;
  if (p.cap > 0x7fffffffull) { why = "pass too large"; return RT_ERR_INVALID; }
  // a shard receives the appends of the blocks with blockIdx % RT_QSHARDS == shard; a grid-stride loop hands
  // each block at most ceil(n / (grid * 256)) iterations, so cap / RT_QSHARDS plus one iteration per block bounds it
  p.shard_cap = (unsigned)(p.cap / RT_QSHARDS) + 256u * (in.n_cu * 8u / RT_QSHARDS + 1u) + 256u;
  p.n_slots = (size_t)p.shard_cap * RT_QSHARDS;
  p.multi_batch = in.owned_pixels > p.batch_pixels || p.lead_pixels > 0;
  return RT_OK;
}

static std::vector<FrameBatch> frame_plan_batches(const FramePlanIn& in, const FramePlan& p) {
  std::vector<FrameBatch> batches;
  for (unsigned long long first = 0; first < in.owned_pixels;) {
    const unsigned long long npx = (first == 0 && p.lead_pixels) ? p.lead_pixels : std::min(p.batch_pixels, in.owned_pixels - first);
    batches.push_back({first, npx, (unsigned)std::min<unsigned long long>(in.spp, std::max<unsigned long long>(p.pass_samples, p.cap / npx))});
    first += npx;
  }
  return batches;
}
