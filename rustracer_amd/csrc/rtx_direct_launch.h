// rtx_direct_launch.h - the direct-lighting integrator (rtx_direct.hip: k_sampler_array_tables, k_direct_vertex, k_direct_probe, k_direct_info): what the frame loop hands
// its kernels. Included after rtx_kernels.h.
#pragma once
namespace rtx {
// One round of one step of the depth-first walk (run_direct, rtx_hip.hip): run_whitted's step - the closest-hit launch has left the node's hit at the sample's slot -, then
// n_rounds launches of k_direct_vertex. Under RT_DIRECT_ALL round r < n_lights runs estimate_direct for light r of the list; under RT_DIRECT_ONE the single round runs it
// for the light the sample picks. A round leaves at most one shadow record per sample (the light half: the any-hit launch after the round adds a clear record's term into
// lacc[path]) and at most one PROBE record (the BSDF half of a non-delta light: the BSDF-sampled ray, its path, its light and f |cos| weight / pdf times the throughput;
// the closest-hit launch over the probe queue and k_direct_probe then add term * le). Both are resolved before the next round runs: the additions come in the contract's
// order and never race. Round 0 also adds beta * Le; the LAST round draws the reflection and moves the sample on, as k_whitted_vertex does.
//   wst    [path id] (get_2d() draws after the camera sample, li invocations, get_1d() draws, vertices that reached uniform_sample_all_light)
//   stack, levels, stack_cap, rdiff: WhittedArgs'
//   arr    the batch's array tables as a Tables view (dims = 0: table_2d(arr, pix, a, s) is array a), n_arrays = 2 * max_depth * n_lights of them (RT_DIRECT_ALL)
struct DirectArgs {
  unsigned round, n_rounds, step;
  int n_lights, max_depth, strategy;
  uint4* wst; float4* stack; unsigned levels; size_t stack_cap;
  RayDiffSrc rdiff;
  Tables arr; unsigned n_arrays;
};
void rtx_launch_direct_vertex(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const DirectArgs& a);
// after a round's closest-hit launch over the probe queue (ps.q_mis, counter block 2 of ps.cnt_out; records ps.mi.o / d / hit / a): lacc[path] += term * le
void rtx_launch_direct_probe(bool general, unsigned grid, hipStream_t stream, const DScene& d, const PassState& ps);
// after the last step: info[[window pixel][sample of the call]] = (li invocations, get_2d() draws, get_1d() draws, array vertices), with k_sample_store's indexing
void rtx_launch_direct_info(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const DirectArgs& a, int wx0, int wy0, int ww, uint4* info);
// ZeroTwoSequence::start_pixel continued past the 2 * dims tables: the n_arrays array tables of the batch's n_pixels pixels (fp.chunk_first names the first), one lane per
// pixel. scrambles [2 a + {0, 1}][pixel], perms [a][sample][pixel]: K0's layout with dims = 0. Returns hipSuccess or the launch's error.
hipError_t rtx_launch_sampler_array_tables(hipStream_t stream, const FrameParams& fp, unsigned n_pixels, unsigned spp, unsigned dims, unsigned n_arrays, unsigned* scrambles,
                                           unsigned short* perms);
void rtx_direct_set_ewa_lut(const float* lut128);  // kEwaLut of that translation unit
}
