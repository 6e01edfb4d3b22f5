// rtx_ao_launch.h - the ambient-occlusion and normal integrators (rtx_ao.hip: k_ao_rays, k_ao_fold, k_ao_finish): what the frame loop hands its kernels.
// Included after rtx_kernels.h.
#pragma once
namespace rtx {
// One round of AmbientOcclusion::li's loop (integrator/ao.rs:41-51) over the entries of bounce 0's queue: `round` is k, the k-th get_2d() of every hit path.
// flag: 0x80000000 - the any-hit epilogue adds a clear ray's (1, 0, 0) into lacc[path] (TraceIO::direct_add); 0 - the launch leaves one byte per record in
// PassState::occ_sh and k_ao_fold adds (the calls that hand the rays out). aux: [path id] (|d . n|, t, status, 0), written in round 0, or NULL (a frame: nothing reads it).
// rays_out: NULL, or the caller's [pixel_index][ray_ns][n_ao][2] float4 records - (o | t_max), (d | occluded, set by k_ao_fold) - of samples [ray_s0, ray_s0 + ray_ns).
struct AoArgs { unsigned round, n_ao; float max_distance; unsigned flag; float4* aux; float4* rays_out; unsigned ray_s0, ray_ns; };
void rtx_launch_ao_rays(bool general, unsigned grid, hipStream_t stream, const DScene& d, const FrameParams& fp, const PassState& ps, const AoArgs& a);
// after the round's any-hit launch of a call that hands its rays out: lacc[path].x += 1 for every clear record of the round's queue, the record's answer into rays_out
void rtx_launch_ao_fold(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const AoArgs& a);
// after the last round: ao = float32(n_clear) / float32(n_ao) per path. out NULL (a frame): lacc[path] = (ao, ao, ao | flags), Spectrum::grey(ao) for the film kernel;
// else out[[window pixel][sample of the call]] = (ao, |d . n|, t, status) with k_sample_store's indexing (ps.spp = the call's samples per pixel, ps.s0 relative to its first)
void rtx_launch_ao_finish(unsigned grid, hipStream_t stream, const FrameParams& fp, const PassState& ps, const AoArgs& a, int wx0, int wy0, int ww, float4* out);
}
