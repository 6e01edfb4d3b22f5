// rtx_whitted_launch.h - the Whitted integrator (rtx_whitted.hip: k_whitted_vertex, k_whitted_info): what the frame loop hands its kernels.
// Included after rtx_kernels.h.
#pragma once
namespace rtx {
#define RT_WHITTED_STACK_PLANES 4  // 16-byte records per pending entry: (o | b2), (d | prim), (b0, b1, -, -), (beta | -)
// One round of one step of the depth-first walk (run_whitted, rtx_hip.hip). A step advances every active camera sample by ONE node of its own tree: the closest-hit
// launch has left the node's hit at the sample's slot, then n_rounds = max(n_lights, 1) launches of k_whitted_vertex - round r < n_lights produces light r's term as
// one shadow record per sample (the any-hit launch between two rounds adds a clear record's term into lacc[path]: one record per path and round, no float atomics, the
// additions in list order), round 0 also adds beta * Le, and the LAST round draws the reflection and moves the sample on: down into the reflected ray, across to the
// transmitted one, or up to the pending transmission of the nearest ancestor.
//   wst    [path id] (get_2d() draws consumed after the camera sample, li invocations, -, -): the draw index of a node depends on the subtrees before it
//   stack  the pending vertices, planar: plane p of level l of path i at stack[(p * levels + l) * stack_cap + i] - a wave's accesses to one level are contiguous
//          runs. levels = max_depth - 1: a vertex at depth d (< max_depth - 1) waits at level d while its reflection subtree is walked.
//   rdiff  the caller's ray records where they carry differentials (RT_FLAG_RAY_DIFFERENTIALS on a scene that reads them), else rays == NULL: a camera frame
//          rebuilds the camera ray's from the film position, as the shade kernels do. Depth 0 only: specular children carry none.
struct WhittedArgs {
  unsigned round, n_rounds, step;  // step 0: the camera rays - depth 0, nothing pending, no draws yet (the records raygen wrote say nothing else)
  int n_lights, max_depth;
  uint4* wst; float4* stack; unsigned levels; size_t stack_cap;
  RayDiffSrc rdiff;
};
void rtx_launch_whitted_vertex(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const WhittedArgs& a);
// after the last step: info[[window pixel][sample of the call]] = (li invocations, draws) of every traced sample, with k_sample_store's indexing
void rtx_launch_whitted_info(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const WhittedArgs& a, int wx0, int wy0, int ww, uint2* info);
void rtx_whitted_set_ewa_lut(const float* lut128);  // kEwaLut of that translation unit
}
