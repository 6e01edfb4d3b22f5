/* rtx_hip.h — C ABI of the MI355X (gfx950) wavefront path-tracing backend.
 *
 * This is the drop-in boundary for ONE path of abusch/rustracer: the call
 *     renderer::render(scene, integrator, camera, num_threads, sampler, 16)
 * made once per WorldEnd (rustracer-core/src/api.rs:1003-1010, implemented in
 * rustracer-core/src/renderer.rs:22-143). A host (Rust in the reference; the C++ layer of
 * include/rtx_host.h here) keeps scene parsing, the SAH BVH build and the Film; it flattens
 * BVH nodes, triangles, material/texture tables and the light list into the plain arrays below
 * and hands them over. Plain pointers and sizes only; nothing here knows about torch.
 *
 * `rc/` = rustracer-core/src/ of the reference.
 */
#ifndef RTX_HIP_H
#define RTX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_INVALID (-1)   /* bad argument / inconsistent description            */
#define RT_ERR_NO_DEVICE (-2) /* no usable gfx950 device; there is NO CPU fallback. rt_scene_create / rt_multi_create check the whole description first: a faulty
                                 one is refused with RT_ERR_INVALID / RT_ERR_UNSUPPORTED and the same message on any machine, a valid one gets this code */
#define RT_ERR_HIP (-3)       /* a HIP call failed; see rt_last_error()             */
#define RT_ERR_OOM (-4)
#define RT_ERR_UNSUPPORTED (-5) /* input the reference accepts and this backend does not  */

/* -- flattened BVH node, 32 B: replaces LinearBVHNode (rc/bvh/mod.rs:582-598) ------------ */
typedef struct rt_bvh_node {
  float bmin[3];
  float bmax[3];
  uint32_t offset;  /* leaf: first primitive (leaf order); interior: second child index */
  uint16_t n_prims; /* 0 => interior                                                    */
  uint8_t axis;     /* interior: split axis                                             */
  uint8_t pad;
} rt_bvh_node;

/* -- per-triangle metadata: replaces GeometricPrimitive{shape,material,area_light}
 *    (rc/primitive.rs:34-76) and Triangle{reverse_orientation,swaps_handedness}
 *    (rc/shapes/mesh.rs:175-180) ---------------------------------------------------------- */
#define RT_TRI_FLIP 1u   /* reverse_orientation ^ transform_swaps_handedness */
#define RT_TRI_HAS_N 2u  /* mesh.n is Some                                   */
#define RT_TRI_HAS_UV 4u /* mesh.uv is Some (else default uvs, mesh.rs:201-211) */
#define RT_TRI_HAS_S 8u  /* mesh.s is Some                                   */
#define RT_TRI_HAS_ALPHA 16u        /* mesh.alpha_mask is Some: tri_alpha[2 i] is its float texture (rc/shapes/mesh.rs:38,134-144)          */
#define RT_TRI_HAS_SHADOW_ALPHA 32u /* mesh.shadow_alpha_mask is Some: tri_alpha[2 i + 1] (mesh.rs:39,146-156); shadow rays only (:577-581) */
#define RT_PRIM_SPHERE 64u /* this primitive is an analytic sphere (rc/shapes/sphere.rs), not a triangle: its tri_p slot holds the world bounding
                              box (p0 = min, p1 = max) and, as the bits of p2.x, its index into rt_scene_desc::spheres                          */
#define RT_PRIM_INSTANCE 128u /* this primitive is an object instance (TransformedPrimitive, rc/primitive.rs:79-118): its tri_p slot holds the world
                                 bounding box (p0 = min, p1 = max) and, as the bits of p2.x, its index into rt_scene_desc::instances              */
typedef struct rt_tri_meta {
  int32_t material; /* index into materials[]                 */
  int32_t light;    /* index into lights[] (area light) or -1 */
  uint32_t flags;
  uint32_t source_index; /* triangle index before BVH re-ordering (diagnostics) */
} rt_tri_meta;

/* -- Shape "sphere": replaces Sphere (rc/shapes/sphere.rs:15-68). o2w / w2o: the object-to-world matrix and its inverse, row-major 4x4
 *    (Transform{m, m_inv}: the inverse as the host computed it - a Gauss-Jordan inverse in f32 need not have an exact last row, and
 *    Transform * Point divides by w whenever w != 1, transform.rs:264-286); z_min .. phi_max as Sphere::new leaves them. -------------------- */
typedef struct rt_sphere {
  float o2w[16], w2o[16];
  float radius, z_min, z_max, theta_min, theta_max, phi_max;
  int32_t reverse_orientation, swaps_handedness;
  /* the same record carries the reference's two other quadrics: kind 1 = Disk (rc/shapes/disk.rs: height, radius, inner_radius, phi_max),
   * kind 2 = Cylinder (rc/shapes/cylinder.rs: radius, z_min, z_max, phi_max); kind 0 = Sphere */
  int32_t kind;
  float height, inner_radius;
} rt_sphere;

/* -- ObjectInstance: replaces TransformedPrimitive{primitive, primitive_to_world} (rc/primitive.rs:79-118, rc/api.rs:1053-1090). The object is what
 *    object_instance wraps: the BVH aggregate over the object's primitives - n_nodes nodes from nodes[node_base], child / primitive offsets relative to
 *    the object's own first node / first primitive - or, for an object of exactly one primitive, that primitive itself (n_nodes = 0). Its n_prims
 *    primitives (triangles in OBJECT space, leaf order) sit in the tri_* arrays from prim_base on, after the n_top_prims primitives of the top level.
 *    A hit inside instance k carries the id n_top_prims + (n_prims of instances 0 .. k-1) + its leaf-order index in the object (rt_trace_closest):
 *    ids below n_top_prims name top-level primitives, as before. ------------------------------------------------------------------------------ */
typedef struct rt_instance {
  float o2w[16], w2o[16]; /* primitive_to_world and its inverse as the host holds them, row-major */
  uint32_t node_base, n_nodes, prim_base, n_prims;
} rt_instance;

/* -- textures: replaces dyn Texture<T> (rc/texture/{constant,scale,mix,imagemap,checkerboard,uv,fbm}.rs) --
 * checkerboard (2D): tex1, tex2, mapping, amount = AAMethod (0 none, 1 closedform); uv: mapping;
 * fbm: value[0] = omega, amount = octaves (texture space = world space).
 * RT_TEX_CHECKER_PLANAR: a checkerboard under PlanarMapping2D (rc/texture/mod.rs:63-85): tex1, tex2, amount as for RT_TEX_CHECKER; `image` names a word block
 *   (an rt_image with n_levels == 0) whose first 8 words are v1.xyz, v2.xyz, udelta, vdelta (f32); mapping[] is unused.
 * RT_TEX_FBM_MAPPED: fbm under IdentityMapping3D (rc/texture/mod.rs:92-115): value[0] = omega, amount = octaves as for RT_TEX_FBM; `image` names a word
 *   block whose first 16 words are the row-major 4 x 4 matrix applied to the hit point and its differentials - the CTM at the Texture directive itself, which
 *   the reference stores as its world_to_texture.
 * Scale, mix and checkerboards nest to any depth, and a mix amount may be any float texture. The graph must be acyclic. A graph's value slots (the combinator
 * values alive at once while it is evaluated, heavier operands first) are held in registers and bounded by RT_TEX_SLOTS: every tree of at most 120
 * combinators fits (the smallest tree that needs 9 values at once has 121, with three-operand mixes), a graph that shares a sub-graph keeps its value until
 * its last reader, and rt_scene_create refuses a graph that needs more than RT_TEX_SLOTS - or, as an alpha mask, more than RT_TEX_MASK_SLOTS (every tree of
 * at most 12 combinators fits) - naming the texture and its requirement. This falls short of "every graph of 64 combinators": a graph that shares many
 * sub-graphs can need more than 8 values with fewer combinators. */
enum { RT_TEX_CONST = 0, RT_TEX_SCALE = 1, RT_TEX_MIX = 2, RT_TEX_IMAGE = 3, RT_TEX_CHECKER = 4, RT_TEX_UV = 5, RT_TEX_FBM = 6, RT_TEX_CHECKER_PLANAR = 7,
       RT_TEX_FBM_MAPPED = 8 };
#define RT_TEX_SLOTS 8
#define RT_TEX_MASK_SLOTS 4 /* ... of the graph of an alpha / shadow-alpha mask (evaluated inside the traversal kernels) */
typedef struct rt_texture {
  int32_t kind;
  float value[3];             /* constant; float textures use value[0]                 */
  int32_t tex1, tex2, amount; /* scale / mix / checkerboard operands (see above)       */
  int32_t image;              /* imagemap: index into images[]                         */
  float mapping[4];           /* UVMapping2D su sv du dv (rc/texture/mod.rs:38-61)      */
} rt_texture;

/* -- MIP pyramid built by the host: replaces MIPMap<Spectrum> (rc/mipmap.rs:46-53) ---------
 * An image with n_levels == 0 is a block of packed 32-bit words instead: the word block of an RT_TEX_CHECKER_PLANAR / RT_TEX_FBM_MAPPED texture that names it,
 * or else a Fourier BSDF table (FourierBSDFTable, rc/bsdf/fourier.rs:281-371) that an RT_MAT_FOURIER material names:
 * `texels` points to 3 * n_texels packed 32-bit words (zero-padded to a whole texel) - the header {nMu, mMax, nChannels, nCoeffs as u32, eta as f32},
 * then mu[nMu] (f32, strictly ascending), cdf[nMu * nMu] (f32), offset_and_length[2 * nMu * nMu] (u32) and a[nCoeffs] (f32), as a .bsdf file lists them.
 * rt_scene_create / rt_multi_create refuse with RT_ERR_INVALID (as every fault of a description: before any device is touched) a table whose sizes do not add up, with nMu outside [2, 8192],
 * nChannels not 1 or 3, mu not ascending, a cell longer than mMax or whose coefficients run past nCoeffs, more than 2^28 table words in the scene, a Fourier
 * material whose slot M1 names a MIP pyramid, and an image texture or infinite light that names a table. width / height / offset / trilinear / wrap are unused.
 * They refuse as well (RT_ERR_INVALID) a word block shorter than its texture's words, a mapped texture that names a MIP
 * pyramid, a Fourier material, image texture or infinite light that names a word block, a texture graph with a cycle and an operand out of range. */
enum { RT_WRAP_REPEAT = 0, RT_WRAP_BLACK = 1, RT_WRAP_CLAMP = 2 };
#define RT_MAX_MIP_LEVELS 16
typedef struct rt_image {
  int32_t n_levels;
  int32_t width[RT_MAX_MIP_LEVELS], height[RT_MAX_MIP_LEVELS];
  uint64_t offset[RT_MAX_MIP_LEVELS]; /* texel offset of each level inside `texels` (RGB f32) */
  const float* texels;                /* all levels, row-major, 3 floats per texel            */
  uint64_t n_texels;
  int32_t trilinear;
  float max_anisotropy;
  int32_t wrap;
} rt_image;

/* -- materials: replaces dyn Material (rc/material/*.rs) ----------------------------------- */
enum { RT_MAT_MATTE = 0, RT_MAT_PLASTIC, RT_MAT_METAL, RT_MAT_MIRROR, RT_MAT_GLASS, RT_MAT_UBER, RT_MAT_SUBSTRATE, RT_MAT_MIX, RT_MAT_TRANSLUCENT,
       RT_MAT_DISNEY /* rc/material/disney.rs; slots: KD color, KS metallic, ETA eta, ROUGHNESS roughness, KR speculartint, UROUGH anisotropic,
                        KT sheen, SIGMA sheentint, VROUGH clearcoat, K clearcoatgloss, OPACITY spectrans, REFLECT scatterdistance,
                        TRANSMIT flatness, AMOUNT difftrans, M1 = thin (0 / 1, not an id) */,
       RT_MAT_FOURIER /* rc/material/fourier.rs; M1 = index into images[] of its Fourier BSDF table (n_levels == 0, see rt_image; not a texture id);
                         bump as for the other kinds; the other slots are -1 */ };
enum { RT_SLOT_KD = 0, RT_SLOT_KS, RT_SLOT_KR, RT_SLOT_KT, RT_SLOT_SIGMA, RT_SLOT_ROUGHNESS, RT_SLOT_UROUGH, RT_SLOT_VROUGH,
       RT_SLOT_ETA, RT_SLOT_K, RT_SLOT_OPACITY, RT_SLOT_REFLECT, RT_SLOT_TRANSMIT, RT_SLOT_AMOUNT, RT_SLOT_M1, RT_SLOT_M2, RT_N_SLOTS };
typedef struct rt_material {
  int32_t kind;
  int32_t slot[RT_N_SLOTS]; /* texture ids (material ids for M1/M2); -1 = absent */
  int32_t remap_roughness;
  int32_t bump;             /* "bumpmap" float texture id or -1 (material::bump, rc/material/mod.rs:50-92); ignored by mix */
} rt_material;

/* -- lights: replaces dyn Light (rc/light/{diffuse,point,distant,infinite}.rs) ------------- */
enum { RT_LIGHT_DIFFUSE_AREA = 0, RT_LIGHT_POINT = 1, RT_LIGHT_DISTANT = 2, RT_LIGHT_INFINITE = 3 };
typedef struct rt_light {
  int32_t kind;
  int32_t prim;      /* area: emitting triangle, LEAF-ORDER index          */
  float rgb[3];      /* area: L_emit; point: I; distant: L                 */
  int32_t two_sided;
  float vec[3];      /* point: position; distant: normalised direction     */
  float area;        /* area: Shape::area()                                */
  float world_radius; /* distant / infinite: scene bounding-sphere radius  */
  int32_t image;     /* infinite: Lmap pyramid                             */
  float l2w[12], w2l[12]; /* infinite: 3x4 light<->world                   */
  /* infinite: Distribution2D over (2*w) x (2*h) (rc/light/infinite.rs:80-101), host-built */
  int32_t dist_nu, dist_nv;
  const float* dist_func;     /* nv*nu                */
  const float* dist_cdf;      /* nv*(nu+1)            */
  const float* dist_func_int; /* nv                   */
  const float* marg_func;     /* nv                   */
  const float* marg_cdf;      /* nv+1                 */
  float marg_func_int;
} rt_light;

/* -- the flattened scene handed over at WorldEnd -------------------------------------------- */
typedef struct rt_scene_desc {
  uint32_t n_nodes;
  const rt_bvh_node* nodes; /* pre-order, left child = i+1 (rc/bvh/mod.rs:314-358)          */
  uint32_t n_tris;          /* primitives in leaf order: triangles, and spheres where tri_meta[i].flags has RT_PRIM_SPHERE      */
  const float* tri_p;       /* n_tris*9, world space, LEAF ORDER (p0 p1 p2)                  */
  const float* tri_n;       /* n_tris*9 or NULL                                              */
  const float* tri_uv;      /* n_tris*6 or NULL                                              */
  const float* tri_s;       /* n_tris*9 or NULL                                              */
  const rt_tri_meta* tri_meta;
  const int32_t* tri_alpha; /* n_tris*2 {alpha, shadowalpha} float-texture ids, read where the RT_TRI_HAS_*ALPHA flags are set; NULL if no
                               mesh carries a mask. A hit whose mask evaluates to 0 is no hit (Triangle::intersect mesh.rs:353-370,
                               intersect_p :534-582) - in BVH traversal and in Shape::pdf_wi's re-intersection alike */
  uint32_t n_spheres; const rt_sphere* spheres; /* the analytic spheres among the n_tris primitives (RT_PRIM_SPHERE); an area light's `prim` may name one */
  uint32_t n_textures; const rt_texture* textures;
  uint32_t n_images; const rt_image* images;
  uint32_t n_materials; const rt_material* materials;
  uint32_t n_lights; const rt_light* lights; /* order = Scene::lights (rc/scene.rs:24)       */
  /* object instances (two-level traversal). With n_instances > 0: nodes[0 .. n_top_nodes) is the top-level tree and tri_*[0 .. n_top_prims) its
   * primitives (some of them RT_PRIM_INSTANCE); the objects' trees and primitives follow in the same arrays (n_nodes, n_tris count everything).
   * Without instances the three fields are 0 / NULL. */
  uint32_t n_instances; const rt_instance* instances;
  uint32_t n_top_nodes, n_top_prims;
  /* Emitters that are no lights: lights[n_lights .. n_lights + n_unlisted_lights) are DiffuseAreaLight records (rgb, two_sided) a primitive's `light`
   * may name although Scene::lights does not hold them - a shape with an AreaLightSource inside an ObjectBegin block keeps its area light (it glows when a
   * camera ray or a specular bounce hits it) while the light itself never reaches the scene's list (rc/api.rs:954-964): it is never sampled, has no entry in
   * the light distribution, and a BSDF-sampled ray that reaches it contributes nothing (no sampled light is this one, rc/integrator/mod.rs:293-307). */
  uint32_t n_unlisted_lights;
} rt_scene_desc;

/* -- what renderer::render receives through &dyn Camera / Film / Sampler / Integrator ------- */
typedef struct rt_camera {        /* PerspectiveCamera (rc/camera.rs:18-27)        */
  float raster_to_camera[16];     /* 4x4 projective                                */
  float camera_to_world[16];
  float dx_camera[3], dy_camera[3];
  float lens_radius, focal_distance;
} rt_camera;
typedef struct rt_film_desc {     /* Film (rc/film.rs:45-55)                       */
  int32_t cropped_pixel_bounds[4]; /* x0 y0 x1 y1                                  */
  int32_t sample_bounds[4];        /* Film::get_sample_bounds, x0 y0 x1 y1         */
  float filter_radius[2];
  float filter_table[256];         /* 16x16, film.rs:16-17,92-102                  */
  float max_sample_luminance;
} rt_film_desc;
typedef struct rt_sampler_desc {  /* ZeroTwoSequence (rc/sampler/zerotwosequence.rs) */
  int32_t spp;                    /* rounded up to a power of two by the callee    */
  int32_t dimensions;             /* "dimensions", default 4                       */
} rt_sampler_desc;
typedef struct rt_path_desc {     /* PathIntegrator (rc/integrator/path.rs:25-31)  */
  int32_t max_depth;
  float rr_threshold;
  int32_t light_strategy;         /* 0 "spatial" (voxel CDF, rc/lightdistrib.rs), 1 "uniform" */
  int32_t pixel_bounds[4];        /* x0 y0 x1 y1                                    */
} rt_path_desc;
/* Film sharding for multi-GPU: this call renders the bands r of the sample rows with r % world_size == rank; pixels of
 * other rows stay zero in the output. A band is RT_SHARD_ROWS(H, world_size) rows high: 4 rows on a sharded frame (round 6; rounds 4 - 5 cut the reference's 16-row
 * tile rows, or 8 rows where those did not divide over the ranks). What a rank's rows cost depends on what they show, and the slowest rank sets the frame time: on the
 * headline scene the 8-way split's slowest rank took 1.037 of the mean with 16-row bands, 1.022 with 8, 1.013 with 4 (profiles/r06_shard_band_sweep.txt), and 1080 rows
 * are 270 bands - 34 or 33 per rank of 8. Which samples a device renders changes nothing in the film: every pixel's sampler is keyed by the pixel (pixel-keyed mode). */
typedef struct rt_shard { int32_t rank, world_size; } rt_shard;
#define RT_SHARD_ROWS(H, world_size) ((world_size) > 1 ? 4 : 16)

typedef struct rt_stats {
  uint64_t camera_rays;
  uint64_t rays_closest, rays_shadow, rays_mis;  /* ray casts by class            */
  uint64_t nodes_closest, nodes_shadow, nodes_mis; /* BVH node visits (0 unless counting is on) */
  uint64_t tris_closest, tris_shadow, tris_mis;    /* triangle tests                */
  uint64_t paths_scrubbed;                       /* NaN / negative / inf samples set to black (renderer.rs:115-126) */
  double ms_total;                               /* rt_render wall time, device-synchronised */
  double ms_sampler, ms_raygen, ms_trace_closest, ms_trace_any, ms_trace_mis, ms_shade, ms_resolve, ms_film, ms_lightdist; /* HIP-event times */
  uint64_t launches_trace_closest;               /* number of trace_closest launches (path + MIS) */
  uint64_t n_passes;
  /* path vertices by the shade front-end that served them: constant-Kd matte under area lights, Lambert under any light,
   * two-lobe materials (matte with sigma, plastic, metal, mirror), everything else */
  uint64_t vertices_lambert_const, vertices_lambert, vertices_two_lobe, vertices_generic;
  /* ms_shade split (RT_FLAG_TIME_KERNELS): the shade launches of each front-end, the queue binning, the miss bin */
  double ms_shade_lambert_const, ms_shade_lambert, ms_shade_two_lobe, ms_shade_generic, ms_shade_bin, ms_shade_miss;
  /* measurement builds only (make ABLATE=1; zero otherwise): wave cycles per section of the shade kernel, [front-end 0..3][section 0..7] =
   * state + interaction, emission + differentials, material, light pick, light-sampling half, BSDF-sampling half, continuation + stores, loop tail */
  uint64_t shade_section_cycles[32];
  /* BSDF-sampled MIS rays toward an infinite light are traced for occlusion only (their own launch of the any-hit kernel): of rays_mis / nodes_mis /
   * tris_mis, the part that belongs to those rays, and of ms_trace_mis the time of their launches. nodes_ / tris_mis_any are filled by frames rendered with
   * RT_FLAG_COUNT_TRAVERSAL | RT_FLAG_COUNT_AS_RENDERED (plain RT_FLAG_COUNT_TRAVERSAL walks every MIS ray as the reference does: closest hit). */
  uint64_t rays_mis_any, nodes_mis_any, tris_mis_any;
  double ms_trace_mis_any;
  /* rt_multi_render, `total` only: wall time from the moment the last device finished its chunks to the merged frame being in place (the additions on
   * devices[0] and the final copy); per-device wall times are per_device[k].ms_total */
  double ms_gather;
  /* of rays_mis: BSDF-sampled rays toward a sphere light that miss the sphere's world box and were therefore not cast (Sphere::pdf_wi is non-zero for any
   * direction, sphere.rs:310-334; such a ray's term is zero whatever it hits). Zero on frames that count the reference's walk. */
  uint64_t rays_mis_not_cast;
  /* of rays_closest: path rays that follow a NON-specular bounce at the depth limit and were therefore not cast. PathIntegrator::li traces the next ray
   * before it tests the depth (path.rs:100-137) and reads the hit only to add emitted light after a specular bounce: after any other bounce the ray at
   * bounces == max_depth is never read. The film is the one the cast rays give; zero on frames that count the reference's walk. */
  uint64_t rays_tail_not_cast;
  /* launches per stage of this frame, as issued (round 5; launches_trace_closest above = launches_trace_path + launches_trace_mis): the closest-hit launches of
   * the path rays, the any-hit launches of the shadow rays, the closest-hit launches of the BSDF-sampled MIS rays, the any-hit launches of the MIS rays toward
   * an infinite light, and the k_shade launches of all front-ends together (binning and the miss bin not counted). What a per-launch average divides by. */
  uint64_t launches_trace_path, launches_trace_shadow, launches_trace_mis, launches_trace_mis_any, launches_shade;
  /* of rays_shadow: segments whose voxel / light pair the shadow sets mark EMPTY (rt_shadow_sets) - unoccluded for certain, answered by k_shade without a
   * walk. Zero on frames that count the reference's walk and where RTX_SHADOW_SETS=0. */
  uint64_t rays_shadow_not_cast;
} rt_stats;

#define RT_FLAG_COUNT_TRAVERSAL 1u /* fill nodes_ and tris_ counters (slower)                  */
#define RT_FLAG_FILM_ON_DEVICE 2u  /* film_xyzw is a device pointer (HBM-resident output)      */
#define RT_FLAG_TIME_KERNELS 4u    /* fill the per-kernel ms_ fields with HIP events           */
#define RT_FLAG_COUNT_AS_RENDERED 8u /* with RT_FLAG_COUNT_TRAVERSAL: count the walks an uncounted frame runs (occlusion-only MIS rays walk as
                                        intersect_p does) instead of the reference's (every MIS ray a closest-hit walk): what a roofline figure divides by
                                        the time of */
#define RT_FLAG_REF_STREAM 16u /* round 6: the frame with the REFERENCE'S sampler stream - one PCG32 stream per 16 x 16 tile, consumed by the tile's pixels and samples in order
                                (rc/renderer.rs:83-84) - instead of the pixel-keyed one: one lane per tile walks the reference's loop (slow by construction; for the configuration
                                the reference itself runs). The film then equals the oracle's SAMPLER_REF mode sample for sample: weights exact, radiance inside the image gate.
                                Single device, plain-triangle scenes; stats: camera_rays and the three ray counts. */
#define RT_FLAG_FRAME_STATS 32u /* rt_frame_begin only (other entry points ignore it): the frame keeps per-pixel luminance moments and accepts rt_frame_advance_adaptive */
#define RT_FLAG_FRAME_FEATURES 64u /* rt_frame_begin / rt_multi_frame_begin only (other entry points ignore it): the frame keeps per-pixel sums of its samples' first-hit features
                                      (albedo, normal, depth, coverage), read with RT_FRAME_FEATURES */
#define RT_FLAG_RAY_DIFFERENTIALS 128u /* rt_render_rays, rt_frame_advance_rays, rt_frame_advance_rays_adaptive, rt_camera_rays (other entry points ignore it): a ray record is
                                          RT_RAY_DIFF_FLOATS floats - the eight of rt_render_rays, then the ray's differentials rx_o.xyz, ry_o.xyz, rx_d.xyz, ry_d.xyz */

typedef struct rt_scene rt_scene;

/* Uploads the flattened scene (copies every array; the caller may free its own afterwards).
 * device < 0 => the current HIP device. Replaces Scene::new + BVH ownership (rc/scene.rs:29-49). */
int rt_scene_create(const rt_scene_desc* desc, int device, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

/* BVH::new (rc/bvh/mod.rs:80-135) on the device, for callers that want the tree in milliseconds rather than the best
 * tree: a linear BVH (63-bit Morton order of the centroids, one radix sort, boxes fitted bottom-up), leaves of up to
 * max_prims_per_node triangles, written in the layout flatten_bvh gives (rc/bvh/mod.rs:314-358: pre-order, first child
 * = i + 1, `offset` = second child, `axis` = the axis the children are ordered along). The SAH tree of the host layer
 * traces faster and is what parity on node / triangle counts refers to; closest hits do not depend on the builder.
 * tri_p: n_tris x 9 floats, world space, host memory. nodes: room for 2 * n_tris - 1 records. ordered: n_tris source
 * triangle indices in leaf order. RT_ERR_UNSUPPORTED if the tree needs more than the 64-entry traversal stack. */
int rt_bvh_build(const float* tri_p, uint32_t n_tris, int32_t max_prims_per_node, rt_bvh_node* nodes, uint32_t* n_nodes, int32_t* ordered,
                 float* ms_device /* may be NULL */);

/* MIPMap::new (rc/mipmap.rs:75-187) on the device: the Lanczos zoom of a non-power-of-two image (taps computed by the caller: first
 * source texel + 4 weights per output texel and axis; NULL and px = width, py = height for power-of-two images) and the box-filtered
 * levels. lvl_w / lvl_h / lvl_off: level geometry (texel offsets into texels_out, which receives every level). Host pointers. */
int rt_mip_build(const float* rgb, int32_t width, int32_t height, int32_t px, int32_t py, const int32_t* s_first, const float* s_wts, const int32_t* t_first,
                 const float* t_wts, int32_t wrap, int32_t n_levels, const int32_t* lvl_w, const int32_t* lvl_h, const uint64_t* lvl_off, float* texels_out);
/* The sampling tables of InfiniteAreaLight::new (rc/light/infinite.rs:78-101) on the device: func = luminance of the filtered map
 * lookup * sin(theta) at width x height (twice the map's resolution), one Distribution1D per row (rc/distribution1d.rs:11-42) and the
 * marginal one over the row integrals. mode / il / delta: MIPMap::lookup's level choice for the constant filter width (0: level 0,
 * 1: the last level's texel, 2: levels il and il + 1 blended by delta); sin_theta: height values. All pointers are host memory. */
int rt_env_distribution(const rt_image* image, int32_t width, int32_t height, int32_t mode, int32_t il, float delta, const float* sin_theta,
                        float* func, float* cdf, float* func_int, float* marg_cdf, float* marg_func_int);

/* Renders one frame: the body of renderer::render (rc/renderer.rs:22-143) — preprocess (light
 * distribution), per-pixel sampler tables, camera rays, PathIntegrator::li for every sample,
 * radiance scrubbing and Film::add_sample/merge. Blocking; calls on one rt_scene from several threads are safe and take turns (they share the
 * scene's workspace), calls on different rt_scene objects run concurrently. The light distribution is built by the first frame that needs it
 * and kept (the scene is immutable). film_xyzw: W*H*4 floats over the
 * cropped pixel bounds, (X, Y, Z, filter_weight_sum) per pixel as Film's Pixel (film.rs:38-43).
 * `stream` is a hipStream_t (NULL = the null stream). */
int rt_render(rt_scene* scene, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler,
              const rt_path_desc* path, const rt_shard* shard, uint32_t flags, void* stream, float* film_xyzw, rt_stats* stats);

/* Several GPUs of one node from one process (north_star: "partition the film across the 8 GPUs of one node"). The reference's
 * render loop hands 16 x 16 tiles to worker threads from a shared queue and merges finished tiles into the film (rc/renderer.rs:47-71,
 * rc/film.rs:177-194); here the workers are GPUs. rt_multi_create replicates the scene on every listed device (a device may be listed more than
 * once). rt_multi_render cuts the frame into n_devices * chunks_per_device chunks of interleaved bands of RT_SHARD_ROWS rows, lets one host thread per
 * device pull chunks from a shared counter (chunks_per_device = 1: the static split; > 1: the dynamic queue for frames whose rows differ in
 * cost), and sends only the film rows a chunk can have touched to devices[0] over xGMI (hipMemcpyPeerAsync), where they are summed in chunk
 * order - the gather that replaces Film::merge_film_tile. No collective while paths are traced. film_xyzw: host memory, or memory of
 * devices[0] with RT_FLAG_FILM_ON_DEVICE. total / per_device (n_devices entries) may be NULL; total->ms_total is the wall time of the call.
 * One process per GPU (torch.distributed / RCCL harness) uses rt_render with rt_shard instead. */
typedef struct rt_multi rt_multi;
int rt_multi_create(const rt_scene_desc* desc, const int32_t* devices, int32_t n_devices, rt_multi** out);
void rt_multi_destroy(rt_multi* multi);
int rt_multi_render(rt_multi* multi, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                    int32_t chunks_per_device, uint32_t flags, float* film_xyzw, rt_stats* total, rt_stats* per_device);

/* Kernel-level entry points used by the parity tests.
 * rays: n*8 floats (o.xyz, t_max, d.xyz, unused). closest: hits n*4 floats (t, prim as int bits
 * or -1, b0, b1) — BVH::intersect (rc/bvh/mod.rs:366-433). any: hits n uint32 0/1 —
 * BVH::intersect_p (:435-501). counters (optional): {node visits, triangle tests}; with counters the kernels
 * that walk the tree one node per step (the reference's visit sequence) run, without them the kernels rt_render
 * uses (same hits). Host pointers. */
int rt_trace_closest(rt_scene* scene, const float* rays, uint64_t n, float* hits, uint64_t counters[2]);
int rt_trace_any(rt_scene* scene, const float* rays, uint64_t n, uint32_t* occluded, uint64_t counters[2]);
/* Same kernels on device-resident buffers, timed with HIP events on `stream` (bench): returns the
 * average milliseconds per launch over `reps` launches in *ms_per_launch. */
int rt_trace_closest_device(rt_scene* scene, const void* d_rays, uint64_t n, void* d_hits, int reps, void* stream, float* ms_per_launch);

/* ZeroTwoSequence::start_pixel in the pixel-keyed mode: for pixels
 * [pixel0, pixel0+n_pixels) returns the 12 scramble words and the post-shuffle sample index
 * permutation of each of the 2*dimensions tables. scrambles: n_pixels*3*dimensions u32
 * (1D dims first, then 2D pairs); perms: n_pixels*2*dimensions*spp u16. Host pointers. */
int rt_sampler_tables(int32_t spp, int32_t dimensions, uint64_t pixel0, uint64_t n_pixels, uint32_t* scrambles, uint16_t* perms);
/* Same result from the single-kernel statement of the algorithm (one lane walks a pixel's whole RNG stream in
 * order). Not used by rt_render; it is the on-device cross-check of the segmented sampler over large pixel ranges. */
int rt_sampler_tables_plain(int32_t spp, int32_t dimensions, uint64_t pixel0, uint64_t n_pixels, uint32_t* scrambles, uint16_t* perms);

/* offset_ray_origin (rc/geometry/mod.rs:203-220) with its next_float_up / next_float_down steps (rc/lib.rs:227-262) on n points: p, p_error, normal and
 * direction w as n x 3 floats each, out n x 3. The device function every spawned ray goes through (Interaction::spawn_ray / spawn_ray_to, rc/interaction.rs:
 * 56-74), exposed for the parity tests (zeros of both signs, infinities, denormals, NaN). Host pointers. */
int rt_offset_ray_origin(const float* p, const float* p_error, const float* n, const float* w, uint64_t count, float* out);

/* FourierBSDF::f, ::pdf and ::sample_f (rc/bsdf/fourier.rs:45-278) of RT_MAT_FOURIER material `material` of the scene, run by the device lobe functions of
 * the shade kernel on n queries in the shading frame (TransportMode::RADIANCE, no bump map, no mix): wo, wi n x 3 floats, u n x 2 (sample_f's u[0], u[1]).
 * out: n x 11 floats - f(wo, wi) rgb, pdf(wo, wi), then sample_f(wo, u): f rgb, wi xyz, pdf. Host pointers. For the parity tests. */
int rt_fourier_eval(rt_scene* scene, int32_t material, uint64_t n, const float* wo, const float* wi, const float* u, float* out);

/* Texture::evaluate (rc/texture/*.rs) of texture `texture` of the scene on n records, run by the device evaluator the shade kernels call. records: n x 15
 * floats in the order u v dudx dvdx dudy dvdy p.xyz dpdx.xyz dpdy.xyz; rgb_out: n x 3 (a float texture: its value three times). Host pointers. For the
 * parity tests. */
int rt_texture_eval(rt_scene* scene, int32_t texture, uint64_t n, const float* records, float* rgb_out);

/* The Bsdf a material builds, on n queries: Material::compute_scattering_functions (TransportMode::Radiance, allow_multiple_lobes = true as path.rs:145
 * passes it) of material `material` at a surface point, then Bsdf::f(wo, wi, ALL), Bsdf::pdf(wo, wi, ALL) and Bsdf::sample_f(wo, u, ALL)
 * (rc/bsdf/mod.rs:94-251) - run by the front-end structs of the shade kernels themselves (textures, bump maps, mix materials and Fourier tables apply).
 * wo, wi: n x 3 floats, WORLD space, as the integrator passes them; u: n x 2. out: n x RT_BSDF_OUT_FLOATS -
 *   f rgb, pdf, then of sample_f: f rgb, wi xyz (world), pdf, the sampled lobe's type flags (BxDFType bits, as a float), and the number of lobes of the Bsdf.
 * surface: NULL = the canonical hit for every query (p = 0, n = shading n = +z, dpdu = shading dpdu = +x, dpdv = shading dpdv = +y, uv = (0.5, 0.5), every
 * differential zero), or n x RT_BSDF_SURFACE_FLOATS floats of SurfaceInteraction in the order
 *   p.xyz, n.xyz (geometric), shading n.xyz, dpdu.xyz, dpdv.xyz, shading dpdu.xyz, shading dpdv.xyz, dndu.xyz, dndv.xyz, u v, dudx dvdx dudy dvdy,
 *   dpdx.xyz, dpdy.xyz, flip
 * flip != 0: the primitive's reverse_orientation ^ transform_swaps_handedness (read by bump maps only: set_shading_geometry, interaction.rs:218-242).
 * dndu / dndv are carried for completeness and read as zero: every bump-mapped primitive of the backend is a triangle, whose dndu / dndv are zero
 * (mesh.rs:372-382). The first axis of Bsdf::new's frame is normalize(shading dpdu), as the per-triangle shade records hold it.
 * front_end: which front-end of the shade kernels builds and evaluates the Bsdf. RT_BSDF_FRONT_AUTO - the one rt_render sends a camera-ray vertex of this
 * material to (the constant-texture forms where a frame uses them); RT_BSDF_FRONT_GENERIC - the tagged-lobe aggregate, valid for every material;
 * RT_BSDF_FRONT_LAMBERT / _TWO_LOBE / _TWO_LOBE_WIDE - the register-resident front-ends, refused with RT_ERR_INVALID for a material whose class they do not
 * serve. One lane per query; host pointers. n up to 2^31 - 1 queries per call. */
enum { RT_BSDF_FRONT_AUTO = 0, RT_BSDF_FRONT_GENERIC = 1, RT_BSDF_FRONT_LAMBERT = 2, RT_BSDF_FRONT_TWO_LOBE = 3, RT_BSDF_FRONT_TWO_LOBE_WIDE = 4 };
#define RT_BSDF_SURFACE_FLOATS 40
#define RT_BSDF_OUT_FLOATS 13
int rt_bsdf_eval(rt_scene* scene, int32_t material, int32_t front_end, uint64_t n, const float* surface, const float* wo, const float* wi, const float* u,
                 float* out);

/* The light half of the shade stage, on n queries: what estimate_direct's light-sampling half (rc/integrator/mod.rs:222-262) runs at a vertex, per query and
 * without a surface - the light pick of uniform_sample_one_light (mod.rs:186-220), Light::sample_li, Light::pdf_li, Light::le and
 * VisibilityTester::unoccluded (light/mod.rs:52-55) - run by the device functions the shade kernels call. Host pointers; one lane per query.
 * ref: n x RT_LIGHT_REF_FLOATS floats p.xyz, n.xyz, p_error.xyz - the fields of the reference Interaction that lights read. n may be zero (a point in free
 *   space) and so may p_error; Sphere::sample_si and the shadow segment offset their origins with them (spawn_ray_to_interaction, interaction.rs:69-74).
 * u: n x 3 floats u_pick, u_light.x, u_light.y.
 * light >= 0: that entry of the scene's light list for every query; the reported pick pdf is 1 and u_pick is not read. light == RT_LIGHT_PICK: chosen per query
 *   as uniform_sample_one_light does - light_strategy 0: the spatial distribution looked up at p (rc/lightdistrib.rs), 1: uniform; uniform whenever the scene
 *   has one light (path.rs:89). The tables are built on first use and kept (those of rt_light_distribution and of rt_render). The spatial tables hold the voxels
 *   that can contain a surface point (all voxels once rt_light_distribution has been called): a p whose voxel has no table gives light -1, pick pdf 0 and zeros
 *   in the rest of its record; so does a pick of pdf 0 (a voxel no light reaches), with the picked index in float 0.
 * wi: n x 3 floats, world space, used as given (not normalised), or NULL.
 * out: n x RT_LIGHT_OUT_FLOATS floats per query -
 *   0 light index (as a float) | 1 discrete pick pdf | 2-4 Li rgb | 5-7 wi of the sample | 8 pdf of the sample | 9-11 p1.p, the far end of the visibility
 *   segment | 12-14 p1.n | 15 visibility: 1 unoccluded, 0 occluded, -1 not traced | 16 Light::pdf_li(ref, wi query) | 17-19 Light::le along wi query (only an
 *   infinite light has one). Floats 16-19 are zero when wi is NULL.
 * flags: RT_LIGHT_EVAL_VISIBILITY - for the records with pdf > 0 and a non-black Li the segment spawn_ray_to_interaction(ref, p1) is traced by the scene's any-hit
 *   launch, the route of rt_trace_any (Scene::intersect_p: shadow-alpha masks, quadrics and instances apply; the shadow sets, keyed to surface points, do not).
 *   RT_LIGHT_EVAL_GENERAL - the GENERAL instantiation of the light functions (quadric and masked emitters); without it the one the scene's shade kernels use.
 * Refused with RT_ERR_INVALID and a message before any device work, `out` untouched: a NULL scene, ref, u or out; n == 0; n > RT_LIGHT_EVAL_MAX (device buffers
 *   are sized by n: 176 bytes per query, one pass, no chunks); a light that is neither RT_LIGHT_PICK nor an index of the light list; a scene without lights; a
 *   light_strategy other than 0 / 1 (checked whether or not the pick reads it); unknown flag bits. */
#define RT_LIGHT_PICK (-1)
#define RT_LIGHT_REF_FLOATS 9
#define RT_LIGHT_OUT_FLOATS 20
#define RT_LIGHT_EVAL_VISIBILITY 1u
#define RT_LIGHT_EVAL_GENERAL 2u
#define RT_LIGHT_EVAL_MAX (1u << 24)
int rt_light_eval(rt_scene* scene, int32_t light, int32_t light_strategy, uint64_t n, const float* ref, const float* u, const float* wi /* may be NULL */,
                  uint32_t flags, float* out);

/* The radiance of every sample of a pixel window: the frame of rt_render (same batches, passes, kernels and queues) for the pixels of path->pixel_bounds
 * intersected with the film's sample bounds, handed back unfiltered. radiance: n_pixels x spp x 4 floats, pixels row-major in that window, sample index s =
 * the pixel-keyed sampler's index: L rgb exactly as PathIntegrator::li returned it - before the renderer's scrubbing and the max_sample_luminance clamp -
 * and 1.0 in the fourth float where renderer.rs:115-126 scrubs the sample (NaN, negative or infinite luminance), else 0.0. p_film (may be NULL): n_pixels x
 * spp x 2, the samples' film positions. spp is rounded up to a power of two as in rt_render and sizes the outputs. A window of more than
 * RT_SAMPLES_MAX (2^27) samples - 2 GiB of radiance and 1 GiB of film positions - is refused with RT_ERR_INVALID before any device work; so are an empty
 * window, RT_FLAG_REF_STREAM and a NULL radiance. RT_FLAG_FILM_ON_DEVICE: both outputs are device pointers. RT_FLAG_COUNT_TRAVERSAL and RT_FLAG_TIME_KERNELS
 * as in rt_render (ms_film: the kernel that moves the samples out). Single device. */
#define RT_SAMPLES_MAX 134217728
int rt_render_samples(rt_scene* scene, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                      uint32_t flags, void* stream, float* radiance, float* p_film, rt_stats* stats);

/* First-hit features of every sample of a pixel window: what a denoiser takes as guide images, per camera sample, from the vertex the camera ray reaches - the values the
 * frame loop has in hand at bounce 0. Window, sample indexing and refusals are rt_render_samples': the pixels of path->pixel_bounds intersected with the film's sample bounds,
 * features: n_pixels x spp x RT_FEATURE_FLOATS floats, pixels row-major in that window, sample index s = the pixel-keyed sampler's index (spp rounded up to a power of two).
 * Per sample, in this order:
 *   o.xyz, d.xyz   the camera ray as ray generation wrote it (PerspectiveCamera::generate_ray_differential + Ray::transform);
 *   prim, b0, b1   its closest hit in rt_trace_closest's numbering (prim as int bits; a hit inside an object instance is n_top_prims + ...); prim = -1 marks a miss;
 *   depth          length(p - o), p the point of the SurfaceInteraction the shade kernels build at the hit (Triangle / Sphere::intersect, SurfaceInteraction::transform
 *                  for a hit inside an instance) - by the same device functions;
 *   normal.xyz     that interaction's SHADING normal: the interpolated vertex normal where the mesh has normals, else the geometric normal, a quadric's own; world space,
 *                  unit length, negated where dot(n, d) > 0 so that it faces the ray origin. It is the interaction BEFORE Material::compute_scattering_functions:
 *                  BUMP MAPS ARE NOT APPLIED;
 *   albedo.rgb     the factor PathIntegrator::li multiplies beta by at the camera vertex (path.rs:172-196): f * |wi . ns| / pdf of the continuation's Bsdf::sample_f
 *                  draw - the throughput the shade kernel stores for the path's next vertex, beta having entered as 1. A one-sample estimate of the directional
 *                  albedo for every material (Kd for a Lambertian surface up to rounding, Kr for a mirror); zero where sample_f returns black or pdf <= 0 and where
 *                  max_depth == 0 (no Bsdf is built).
 * A miss has prim = -1 and b0, b1, depth, normal and albedo zero (its ray is still reported).
 * Each pass ends after the camera vertices are shaded: nothing past them is traced. RT_FLAG_REF_STREAM, an empty window and a NULL output are refused with RT_ERR_INVALID,
 * and so is, before any device work, a window of more than RT_FEATURE_SAMPLES_MAX (2^25) samples - 2 GiB of features. RT_FLAG_FILM_ON_DEVICE: `features` is a device
 * pointer. Single device. Under RT_FLAG_TIME_KERNELS the feature kernels' time is part of ms_film, here and in a feature frame's steps. */
#define RT_FEATURE_FLOATS 16
#define RT_FEATURE_SAMPLES_MAX 33554432
int rt_render_sample_features(rt_scene* scene, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                              uint32_t flags, void* stream, float* features);

/* Path-traced radiance along caller-supplied rays: PathIntegrator::li(ray, ..) on a batch, with rt_render's kernels, queues and sampler - for the cameras this backend
 * has no struct for (orthographic, environment, fisheye, a realistic lens), light probes, lightmap texels, sensor positions.
 *   rays      [height][width][n_samples][8] floats: o.xyz, t_max, d.xyz, unused - rt_trace_closest's record. d is used as given (not normalised), as Ray::d is.
 *   radiance  [height][width][n_samples][4] floats: L rgb exactly as PathIntegrator::li returns it (rt_render_samples' record), and a fourth float: 0.0 a normal sample,
 *             1.0 where renderer.rs:115-126 would scrub it, 2.0 a ray that was not traced.
 * The batch is a VIRTUAL FILM whose sample bounds are [0, width) x [0, height): ray (x, y, sl) is sample s = sample0 + sl of the pixel with pixel_index = y * width + x. It
 * draws from that pixel's sampler tables at index s and from the keyed RNG stream pixel_index * spp + s + 2^32, the dimension counters starting where get_camera_sample
 * leaves them (cur_1d = 1, cur_2d = 2: what a camera would have consumed is unused). sampler->spp, rounded up to a power of two, sizes the tables, and
 * [sample0, sample0 + n_samples) must lie inside [0, spp): a job of more than RT_RAYS_MAX rays is cut by sample range, and the calls together are the one call, bit for bit.
 * So the camera rays rt_render_sample_features reports of a film with a box filter of radius 0.5, fed back in with t_max = inf, give the radiance rt_render_samples reports.
 * Without RT_FLAG_RAY_DIFFERENTIALS the rays carry no differentials (Ray { differential: None }): every derivative of the first vertex is zero, as at every later vertex
 * (interaction.rs:245-314), and image maps are looked up at zero filter width.
 * RT_FLAG_RAY_DIFFERENTIALS: a record is RT_RAY_DIFF_FLOATS (20) floats - the eight above, then rx_o.xyz, ry_o.xyz, rx_d.xyz, ry_d.xyz: Ray::differential's rx_origin,
 * ry_origin, rx_direction, ry_direction (ray.rs) in world space, USED AS GIVEN - the caller applies scale_differentials (1 / sqrt(spp) in the reference's renderer) itself.
 * They enter compute_differential (interaction.rs:245-314) at the first vertex only; later vertices have none, as in PathIntegrator::li. So MIP maps are filtered,
 * closed-form checkerboards antialiased, fbm octaves clamped and bump maps given footprints as in a camera frame: rt_camera_rays' records of a film with a box filter of
 * radius 0.5 give the radiance rt_render_samples reports on a textured scene too. A record whose twelve differential floats are zero behaves exactly as a ray without
 * differentials (compute_differential returns early on the division by zero), and on a scene that reads none (RT_QUERY_NEEDS_DIFFERENTIALS == 0) the fields are never read:
 * the result is the unflagged call's, bit for bit. The flag costs 48 more bytes per ray of upload and three 16-byte loads per camera vertex.
 * A ray whose t_max is not > 0 (zero, negative, NaN) is SKIPPED: radiance (0, 0, 0, 2.0), nothing consumed, not counted in stats->camera_rays. One scan of the rays on the
 * device decides the route of the call: none skipped - the route of a frame whose pixel_bounds crop nothing, else that of a cropped one. Same radiance either way.
 * path: max_depth, rr_threshold and light_strategy as in rt_render (the light distribution is built by the first call that needs it); pixel_bounds is ignored.
 * flags: RT_FLAG_FILM_ON_DEVICE - rays AND radiance are device pointers; RT_FLAG_RAY_DIFFERENTIALS - records of 20 floats; RT_FLAG_COUNT_TRAVERSAL / _TIME_KERNELS / _COUNT_AS_RENDERED as in rt_render_samples (ms_raygen: the
 * scan and the kernel that reads the rays). Refused with RT_ERR_INVALID before any device work: a NULL scene, rays, sampler, path or radiance; width, height or
 * n_samples <= 0; sample0 < 0 or sample0 + n_samples > the rounded spp; width * height * n_samples > RT_RAYS_MAX; spp > 16384; dimensions outside [2, 8];
 * RT_FLAG_REF_STREAM. Single device. */
#define RT_RAYS_MAX 134217728   /* 2^27 rays per call: 4 GiB of rays, 2 GiB of radiance */
int rt_render_rays(rt_scene* scene, const float* rays, int32_t width, int32_t height, int32_t sample0, int32_t n_samples,
                   const rt_sampler_desc* sampler, const rt_path_desc* path, uint32_t flags, void* stream,
                   float* radiance, rt_stats* stats /* may be NULL */);

/* The perspective camera's rays, as a camera frame generates them - what k_raygen and bounce 0's shade kernels compute - for samples [sample0, sample0 + n_samples) of every
 * pixel of the film's sample bounds (W x H pixels, pixel_index = row * W + column): for a caller who bends them (lens distortion, a stereo offset, a rolling shutter) and
 * feeds them to rt_render_rays or a ray frame, and as the exact source of the camera's differentials.
 *   rays    [H][W][n_samples][8] floats - o.xyz, t_max = inf, d.xyz, 0 - or [..][RT_RAY_DIFF_FLOATS] with RT_FLAG_RAY_DIFFERENTIALS: then rx_o, ry_o, rx_d, ry_d as
 *           PerspectiveCamera::generate_ray_differential leaves them after scale_differentials(1 / sqrt(spp)), spp rounded up to a power of two;
 *   p_film  [H][W][n_samples][2] floats, or NULL: the film position of each sample (pixel + the pixel-keyed sampler's 2D#0; the lens sample is 2D#1).
 * The first 8 floats of a record are the same with and without the flag, and calls over sample ranges that add up to a range give that range's call. With
 * RT_FLAG_FILM_ON_DEVICE both outputs are device pointers; any other flag bit is refused. Refused with RT_ERR_INVALID and a message before any device work: a NULL scene,
 * camera, film, sampler or rays; an empty film; n_samples <= 0, sample0 < 0 or sample0 + n_samples > the rounded spp; more than RT_RAYS_MAX rays; spp > 16384;
 * dimensions outside [2, 8]. Single device. */
#define RT_RAY_DIFF_FLOATS 20
int rt_camera_rays(rt_scene* scene, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler,
                   int32_t sample0, int32_t n_samples, uint32_t flags, void* stream, float* rays, float* p_film /* may be NULL */);

/* Progressive frames: the frame of rt_render rendered in steps, with the film readable between them. The reference's CLI offers "display image as it is
 * rendered" (-p / --display); it has no checkpoint or resume. The pixel-keyed sampler makes sample s of pixel p the same whichever call renders it, so a frame
 * can stop after any number of samples per pixel and go on later.
 * rt_frame_begin copies camera, film, sampler and path, builds the light distribution as a first rt_render would, and allocates the frame's own state on the
 *   scene's device: the film sums (one float4 per cropped pixel), each pixel's own sum (one float4 per owned pixel of the shard), the filter table and - if
 *   owned_pixels * (2 * dims * spp * 2 + 3 * dims * 4) bytes fit table_budget_bytes (0: the smaller of 32 GiB and a quarter of the free device memory) - the
 *   sampler tables of the whole shard, built once by the first step. Otherwise every step rebuilds each batch's tables as rt_render does; the film is the same
 *   byte for byte. Path-state workspace stays the scene's. Refused with RT_ERR_INVALID before any device work: RT_FLAG_REF_STREAM, spp > 16384, dimensions
 *   outside [2, 8], a bad shard, an empty film, a NULL out. flags: RT_FLAG_COUNT_TRAVERSAL / _TIME_KERNELS / _COUNT_AS_RENDERED act per step as in rt_render.
 * rt_frame_advance renders samples [done, min(done + n_samples, spp)) of every owned pixel (spp rounded up to a power of two) with the kernels, queues and routes
 *   of rt_render; stats are those of the step. n_samples <= 0: RT_ERR_INVALID; a finished frame: RT_OK, zeroed stats, no device work. A pixel's own sum receives
 *   its samples in index order whatever the steps are: the finished frame is rt_render's (bit for bit where the filter reaches no further than the pixel and a pixel
 *   receives at most one edge splat; else up to the order of the float additions, which rt_render does not fix either).
 * rt_frame_read resolves the film as it stands (zeros before the first step) without changing the frame. RT_FRAME_XYZW: W*H float4 (X, Y, Z, filter weight
 *   sum), what rt_render hands back (scale ignored); RT_FRAME_RGB: W*H*3 floats, Film::write_image's pixel (rc/film.rs:196-234: XYZ -> RGB, / weight where
 *   it is not zero, max(0, .), * scale); RT_FRAME_RGB8: W*H*3 bytes, that pixel through write_image_png's sRGB quantisation (rc/imageio.rs:52-63; NaN -> 0).
 *   out: host memory, or device memory with RT_FLAG_FILM_ON_DEVICE in `flags`.
 * rt_frame_query: RT_FRAME_SAMPLES_DONE, RT_FRAME_SPP (rounded), RT_FRAME_TABLES_RESIDENT (0 / 1), RT_FRAME_STATE_BYTES (device bytes the frame holds).
 * Any number of frames may live on one scene; their steps and rt_render calls on that scene take turns on the scene's mutex and change no byte of each other.
 * A FRAME MUST BE ENDED BEFORE ITS SCENE IS DESTROYED. rt_frame_end(NULL) is a no-op. One device per rt_frame; rt_shard is honoured (rows of other ranks read as zero) - rt_multi_frame_* below
 * spans the devices of an rt_multi with one rt_frame each and merges their films on the device.
 *
 * Frame statistics and adaptive steps (opt-in: a frame begun without RT_FLAG_FRAME_STATS launches exactly the kernels described above).
 * RT_FLAG_FRAME_STATS gives the frame one more plane, 32 B per owned pixel, zero at begin and counted in RT_FRAME_STATE_BYTES: {double sum_y, double sum_y2,
 *   uint32 n, padding}. The frame's film kernel then adds, for every sample of the pixel that was traced (inside pixel_bounds and the sample rows, and taken by
 *   the pixel), in sample-index order: y = luminance (float32: 0.212671 r + 0.715160 g + 0.072169 b, left to right, no contraction) of the value the film splats
 *   - after the renderer's scrubbing (a scrubbed sample counts as 0) and the max_sample_luminance clamp -, n += 1, sum_y += (double)y, sum_y2 += (double)y *
 *   (double)y. One lane owns a pixel's entry: no atomics, and the sums are those of a sequential loop. The film itself is unchanged by the flag, byte for byte.
 * rt_frame_read(RT_FRAME_STATS): W*H*3 doubles over the cropped pixel bounds, (n, sum_y, sum_y2) per pixel; zeros in rows of other ranks and before the first
 *   step; scale ignored; RT_ERR_INVALID on a frame begun without the flag.
 * rt_frame_advance_adaptive offers sample indices [done, min(done + n_samples, spp)) as rt_frame_advance does - afterwards `done` is that end - but a pixel takes
 *   them only if it is ACTIVE. Activity is decided once per call, before any path work, from the plane as it stands, in IEEE double arithmetic:
 *       active = inside pixel_bounds and the sample bounds and (n < max(min_samples, 2) or se > threshold * max(mean, floor_y))
 *       mean = sum_y / n,  var = max(0, sum_y2 - sum_y * mean) / (n - 1),  se = sqrt(var / n)
 *   An inactive pixel's samples are never traced (they cost one ray-generation lane and one film-kernel read). When no pixel is active no path kernel is
 *   launched, `done` still advances and the stats are zero. RT_ERR_INVALID before any device work: a NULL frame, a frame without RT_FLAG_FRAME_STATS,
 *   n_samples <= 0, min_samples < 0, a NaN or negative threshold or floor_y (+inf is legal: no pixel past min_samples is active). A finished frame: RT_OK, zeroed
 *   stats. rt_frame_advance on a stats frame works as before - every pixel takes the samples - and updates the moments.
 *   A FRAME THAT USED ADAPTIVE STEPS IS NO LONGER rt_render'S FRAME. Each pixel is still sum(w L) / sum(w) over the samples taken - the pixel-keyed sampler
 *   shuffles a pixel's sample order at random, so any subset of its indices is as good a sample set as a prefix - and a wide filter splats the taken samples as
 *   before; but which pixels go on sampling depends on their own estimates, which gives the small bias every variance-driven sampler has (a pixel whose early
 *   samples happen to agree stops early). RT_FRAME_SAMPLES_DONE then means "sample indices offered", not "samples every pixel holds".
 * rt_frame_query, further: RT_FRAME_SAMPLES_TAKEN - the sum of camera_rays over the frame's steps (kept on the host); RT_FRAME_ACTIVE_PIXELS - the number of
 *   active pixels of the last adaptive step, 0 before one has run.
 *
 * First-hit feature planes (opt-in: a frame begun without RT_FLAG_FRAME_FEATURES launches exactly the kernels described above, and its film and rt_stats are untouched).
 * RT_FLAG_FRAME_FEATURES gives the frame one more plane, 64 B per owned pixel, zero at begin and counted in RT_FRAME_STATE_BYTES: double sums of albedo rgb, normal xyz and
 *   depth - the per-sample values of rt_render_sample_features -, uint32 n (samples taken) and uint32 hits (of them, camera rays that hit a surface). Once per pass one
 *   lane per pixel adds the pixel's samples in sample-index order: no atomics, the sums of a sequential loop. Only samples that were traced count: inside pixel_bounds and
 *   the shard's rows, and of a pixel that is active in an adaptive step. THE PLANES ARE UNFILTERED: a pixel's entry holds its own samples only, whatever the film's filter.
 *   The flag combines freely with RT_FLAG_FRAME_STATS; film and statistics plane are the same bytes with and without it. One difference in rt_stats: a feature frame of
 *   max_depth == 1 casts the continuation rays of its camera vertices, which a frame without the flag leaves out (nothing reads them; the albedo is their stored throughput) -
 *   rays_tail_not_cast and the rays actually cast differ there, as they do under RTX_DEAD_TAIL=0, and the film does not.
 * rt_frame_read(RT_FRAME_FEATURES): W*H*8 float32 over the cropped pixel bounds - albedo.rgb = (float)(sum / n), normal.xyz = (float)(sum / n) (not renormalised: misses
 *   add zero), depth = (float)(sum / hits) or 0 when hits == 0, coverage = (float)((double)hits / n); IEEE double divisions. Zeros where n == 0, in rows of other ranks and
 *   before the first step; scale ignored; RT_ERR_INVALID on a frame begun without the flag.
 *
 * rt_frame_read(RT_FRAME_SUMS): W*H float4 over the cropped pixel bounds - the frame's sums as it holds them, before any colour arithmetic: (sum of w * L).rgb and the filter
 *   weight sum, film sum + the pixel's own sum as in every other read-out (RT_FRAME_XYZW is these through the float32 RGB -> XYZ matrix, with the same fourth value). For a
 *   caller that wants sum / weight in the radiance's own RGB - RT_FRAME_RGB is Film::write_image's pixel and goes RGB -> XYZ -> RGB, two float32 matrices that multiply to the
 *   identity only within 1e-6. scale ignored. rt_frame_read only: rt_multi_frame_read refuses it as an unknown read-out. */
enum { RT_FRAME_XYZW = 0, RT_FRAME_RGB = 1, RT_FRAME_RGB8 = 2, RT_FRAME_STATS = 3, RT_FRAME_FEATURES = 4, RT_FRAME_SUMS = 5 };
enum { RT_FRAME_SAMPLES_DONE = 0, RT_FRAME_SPP = 1, RT_FRAME_TABLES_RESIDENT = 2, RT_FRAME_STATE_BYTES = 3, RT_FRAME_SAMPLES_TAKEN = 4, RT_FRAME_ACTIVE_PIXELS = 5 };
typedef struct rt_frame rt_frame;
int rt_frame_begin(rt_scene* scene, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                   const rt_shard* shard /* may be NULL */, uint32_t flags, uint64_t table_budget_bytes, rt_frame** out);
int rt_frame_advance(rt_frame* frame, int32_t n_samples, void* stream, rt_stats* stats /* of this step, may be NULL */);
int rt_frame_advance_adaptive(rt_frame* frame, int32_t n_samples, float threshold, float floor_y, int32_t min_samples, void* stream, rt_stats* stats /* of this step, may be NULL */);
int rt_frame_read(rt_frame* frame, int32_t what, float scale, uint32_t flags, void* stream, void* out);
int rt_frame_query(rt_frame* frame, int32_t what, uint64_t* value);
void rt_frame_end(rt_frame* frame);

/* Ray frames: a progressive frame whose steps take their rays, and the film positions their samples are splatted at, from the caller - the film stage of rt_frame_* for
 * the cameras rt_render_rays serves (orthographic, environment, fisheye, a realistic lens), lightmap bakes and light probes. Nothing per sample travels back to the host.
 * rt_frame_begin_rays opens a frame over rt_render_rays' VIRTUAL FILM: sample bounds = cropped pixel bounds = [0, width) x [0, height), pixel_index = y * width + x, so a
 *   ray frame and rt_render_rays draw the same sampler values for the same ray. Of `film` only filter_radius, filter_table and max_sample_luminance are read (both bounds
 *   arrays are ignored); NULL: a box filter of radius 0.5, a table of ones, no clamp. path->pixel_bounds is ignored, as in rt_render_rays. rt_shard is honoured: rays of
 *   rows a rank does not own are never read. flags: RT_FLAG_FRAME_STATS / _FRAME_FEATURES as in rt_frame_begin; RT_FLAG_COUNT_TRAVERSAL / _TIME_KERNELS /
 *   _COUNT_AS_RENDERED act per step. Refused with RT_ERR_INVALID before any device work: a NULL out, scene, sampler or path; width or height <= 0; width * height >
 *   RT_RAYS_MAX; spp > 16384; dimensions outside [2, 8]; a bad shard; a filter radius > 8 or not > 0; RT_FLAG_REF_STREAM.
 * rt_frame_advance_rays renders samples [done, done + n_samples) of every owned pixel:
 *   rays    [height][width][n_samples][8] floats, rt_render_rays' record, for exactly those samples - [..][RT_RAY_DIFF_FLOATS] with RT_FLAG_RAY_DIFFERENTIALS;
 *   p_film  [height][width][n_samples][2] floats: the raster position each sample is splatted at (FilmTile::add_sample), or NULL: the pixel centre (x + 0.5, y + 0.5).
 *   The position is used as given. A sample whose position lies in its own pixel goes into the pixel's own sum in sample-index order, as in rt_frame_advance: with the
 *   camera's rays and positions the film is the camera frame's, bit for bit. A position elsewhere is legal; what it adds to other pixels - like every tap of a wide
 *   filter outside the sample's pixel - reaches the film through float atomics, so those sums are fixed only up to the order of the additions.
 *   A ray whose t_max is not > 0 (zero, negative, NaN) is SKIPPED, as in rt_render_rays: not traced, not splatted, not counted in the moments' n, the feature plane's n or
 *   camera_rays - the way to mask pixels (outside a fisheye circle, say). The one scan of the step's rays that picks the route of its passes is rt_render_rays'.
 *   flags: RT_FLAG_FILM_ON_DEVICE - rays and p_film are device pointers; RT_FLAG_RAY_DIFFERENTIALS - the records carry the rays' differentials, with rt_render_rays'
 *   semantics: with rt_camera_rays' records and positions a textured scene's film, statistics and feature planes are the camera frame's, bit for bit; any other bit is RT_ERR_INVALID. RT_ERR_INVALID before any device work: a NULL frame or rays;
 *   a frame begun with rt_frame_begin; n_samples <= 0; done + n_samples > spp (rounded) - the caller's array fixes the count, so it is refused, not clamped;
 *   width * height * n_samples > RT_RAYS_MAX. A finished frame: RT_OK, zeroed stats. rt_frame_advance / _advance_adaptive on a ray frame are RT_ERR_INVALID as well.
 * rt_frame_advance_rays_adaptive: rt_frame_advance_adaptive's decision - per pixel, from the moments plane as it stands, before any path work - with the caller's rays:
 *   the rays of an inactive pixel are passed over like skipped rays (and not read). Needs RT_FLAG_FRAME_STATS; threshold, floor_y and min_samples as there.
 *   RT_FRAME_ACTIVE_PIXELS and RT_FRAME_SAMPLES_TAKEN behave as for a camera frame.
 * rt_frame_read, rt_frame_query and rt_frame_end work unchanged on a ray frame. The rays of a step without RT_FLAG_RAY_DIFFERENTIALS carry no differentials (see
 * rt_render_rays); the flag is per step. Single device per frame. */
int rt_frame_begin_rays(rt_scene* scene, int32_t width, int32_t height, const rt_film_desc* film /* may be NULL */, const rt_sampler_desc* sampler, const rt_path_desc* path,
                        const rt_shard* shard /* may be NULL */, uint32_t flags, uint64_t table_budget_bytes, rt_frame** out);
int rt_frame_advance_rays(rt_frame* frame, const float* rays, const float* p_film /* may be NULL */, int32_t n_samples, uint32_t flags, void* stream,
                          rt_stats* stats /* of this step, may be NULL */);
int rt_frame_advance_rays_adaptive(rt_frame* frame, const float* rays, const float* p_film /* may be NULL */, int32_t n_samples, float threshold, float floor_y,
                                   int32_t min_samples, uint32_t flags, void* stream, rt_stats* stats /* of this step, may be NULL */);

/* Camera models: pbrt-v3's orthographic and environment (lat-long) cameras generated ON THE DEVICE from the pixel-keyed sampler - the first users of rt_render_rays and
 * ray frames no longer compute their rays on the host, upload them, or bring a jitter of their own. A model is `int32_t model` plus `const float camera[RT_CAMERA_MODEL_FLOATS]`:
 *   camera[0..15]  camera_to_world, row-major 4 x 4 (points as columns; the last row is not read): o_w = M o, d_w = normalize(M3x3 d), no origin nudge
 *   camera[16..19] screen_window x0, x1, y0, y1 of the plane z = 0 of camera space (orthographic; the environment camera reads none)
 *   camera[20]     lens_radius (orthographic: pbrt-v3's thin lens; the environment camera has none: must be 0)
 *   camera[21]     focal_distance (read where lens_radius > 0)
 *   camera[22..23] reserved, must be 0
 * The film is the VIRTUAL FILM of rt_render_rays and ray frames, W x H = the extent of film->cropped_pixel_bounds - the film's full resolution: a model has no crop window, so
 * the bounds must start at (0, 0); film->sample_bounds is ignored - and sample bounds = cropped pixel bounds = [0, W) x [0, H), pixel_index = y * W + x.
 * The camera sample of (pixel, sample) is the perspective frame's: p_film = (x, y) + 2D#0 of the pixel's tables, p_lens = 2D#1 where lens_radius > 0, the keyed RNG stream
 * and the dimension counters where get_camera_sample leaves them - so dimension 2D#0 keeps its (0,2)-sequence stratification, and a shard generates its own rows' rays.
 *   RT_CAMERA_ORTHOGRAPHIC: p_cam = (x0 + p_film.x / W (x1 - x0), y1 - p_film.y / H (y1 - y0), 0), d = (0, 0, 1); with a lens pl = lens_radius * concentric_sample_disk(p_lens),
 *     the ray leaves (pl.x, pl.y, 0) toward p_cam + focal_distance / d.z * d. Differentials: rx_o = o + ((x1 - x0) / W, 0, 0), ry_o = o + (0, -(y1 - y0) / H, 0), rx_d = ry_d = d;
 *     with a lens rx_o = ry_o = o and rx_d = normalize(p_cam + dx + (0, 0, ft) - o), ft = focal_distance / d.z of the main ray, ry_d likewise.
 *   RT_CAMERA_ENVIRONMENT: theta = pi p_film.y / H, phi = 2 pi p_film.x / W, o = 0, d = (sin theta cos phi, cos theta, sin theta sin phi); the differentials are the same
 *     generator at p_film + (1, 0) and p_film + (0, 1).
 *   In world space the differentials are pulled toward the main ray by 1 / sqrt(spp) (spp rounded up to a power of two), as rt_camera_rays' are. t_max = inf.
 * rt_camera_model_rays: rt_camera_rays for a model - same record layouts ([H][W][n_samples][8 | RT_RAY_DIFF_FLOATS], p_film [H][W][n_samples][2] or NULL), flags
 *   (RT_FLAG_FILM_ON_DEVICE, RT_FLAG_RAY_DIFFERENTIALS; any other bit is refused) and limits (RT_RAYS_MAX). p_film equals rt_camera_rays' of a film with these bounds, byte for byte.
 * rt_frame_begin_model: a progressive frame whose steps generate the model's rays on the device - no ray, film position or sample crosses the host bus. Of `film`
 *   filter_radius, filter_table and max_sample_luminance are read as in rt_frame_begin_rays (a radius in (0, 8]); path->pixel_bounds is ignored. flags: RT_FLAG_FRAME_STATS /
 *   _FRAME_FEATURES / _COUNT_TRAVERSAL / _TIME_KERNELS / _COUNT_AS_RENDERED as in rt_frame_begin, and RT_FLAG_RAY_DIFFERENTIALS: bounce 0 is shaded with the model's
 *   differentials on a scene that reads them (without the flag, or on a scene that reads none, none are generated). rt_frame_advance, rt_frame_advance_adaptive,
 *   rt_frame_read, rt_frame_query and rt_frame_end work on the frame; rt_frame_advance_rays* refuse it. A step stages its records in a buffer the frame owns
 *   (counted in RT_FRAME_STATE_BYTES; 40 or 88 bytes per pixel and sample of the step) and then runs the step of a ray frame on it; a step of more than RT_RAYS_MAX rays
 *   is cut by sample range internally. THE FRAME IS THE RAY FRAME OF ITS OWN RAYS: rt_frame_advance_rays with rt_camera_model_rays' records and positions of the same
 *   sample ranges gives the same sums, statistics and feature planes byte for byte. ms_raygen of a step: generation and k_raygen_rays_film.
 * rt_render_model: rt_render's one-call form - begin, one step of spp samples, rt_frame_read(RT_FRAME_XYZW), end: film_xyzw [H][W][4] (device memory with
 *   RT_FLAG_FILM_ON_DEVICE), the bytes of the finished model frame.
 * Refused with RT_ERR_INVALID and a message that names the field, before any device work: an unknown model; a screen_window that is empty or not finite (orthographic);
 *   lens_radius < 0 or not finite; focal_distance not > 0 while lens_radius > 0; a non-zero lens_radius on the environment camera; a camera_to_world entry that is not
 *   finite; non-zero reserved floats; cropped_pixel_bounds that do not start at (0, 0) or are empty; and what rt_camera_rays / rt_frame_begin_rays refuse. Single device. */
#define RT_CAMERA_ORTHOGRAPHIC 1
#define RT_CAMERA_ENVIRONMENT 2
#define RT_CAMERA_MODEL_FLOATS 24
int rt_camera_model_rays(rt_scene* scene, int32_t model, const float camera[RT_CAMERA_MODEL_FLOATS], const rt_film_desc* film, const rt_sampler_desc* sampler,
                         int32_t sample0, int32_t n_samples, uint32_t flags, void* stream, float* rays, float* p_film /* may be NULL */);
int rt_frame_begin_model(rt_scene* scene, int32_t model, const float camera[RT_CAMERA_MODEL_FLOATS], const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                         const rt_shard* shard /* may be NULL */, uint32_t flags, uint64_t table_budget_bytes, rt_frame** out);
int rt_render_model(rt_scene* scene, int32_t model, const float camera[RT_CAMERA_MODEL_FLOATS], const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                    const rt_shard* shard /* may be NULL */, uint32_t flags, void* stream, float* film_xyzw, rt_stats* stats /* may be NULL */);

/* Progressive and adaptive frames across the workers of an rt_multi: the frame of rt_frame_* spread over the devices of rt_multi_create, read as ONE film.
 * rt_multi_frame_begin opens one rt_frame per worker k on the multi's replica k with rt_shard{k, n_devices} - the static split into interleaved bands of
 *   RT_SHARD_ROWS rows: a pixel's own sum, its sampler tables and its moments live on one device for the life of the frame, so the chunk queue of rt_multi_render
 *   does not apply. It refuses what rt_frame_begin refuses, before any device work and with rt_frame_begin's messages, and a NULL multi; if one worker's begin
 *   fails, the frames already opened are ended and the first error is returned. table_budget_bytes is per worker (0: rt_frame_begin's default). flags:
 *   RT_FLAG_FRAME_STATS / _FRAME_FEATURES / _COUNT_TRAVERSAL / _TIME_KERNELS / _COUNT_AS_RENDERED pass through. A worker with nothing to trace - it owns no row (fewer bands than workers), or
 *   none of its rows lies inside pixel_bounds - is legal: its steps launch nothing and its step stats are zero.
 * rt_multi_frame_advance / _advance_adaptive: one host thread per worker runs rt_frame_advance (_adaptive) on its own frame and stream, all at once. per_device
 *   (n_devices entries, may be NULL): worker k's step stats; total (may be NULL): their sum, with ms_total the wall time of the call. An adaptive step decides
 *   each pixel from its owner's plane - a per-pixel decision, so the one a single-device frame makes. Every RT_ERR_INVALID case of the single-device calls is
 *   refused before any thread starts; a finished frame: RT_OK, zeroed stats. If a step fails on a worker the first error is returned once every worker has
 *   stopped, and the frame is BROKEN (the workers' sample counts may differ): every later call except rt_multi_frame_end answers RT_ERR_INVALID and says so.
 * rt_multi_frame_read yields the merged frame on devices[0]: worker k forms c_k[i] = film_acc_k[i] + own_k[i] where it owns pixel i's row, else film_acc_k[i]
 *   (float32 RGB sums, before any colour conversion) for the film rows it can have touched - its bands widened by the filter's reach -, only those rows travel to
 *   devices[0] (hipMemcpyPeerAsync), and one kernel there adds c_0[i] + c_1[i] + ... left to right in worker order over the workers whose rows hold i and reads
 *   the sum out with rt_frame_read's arithmetic. what / scale as in rt_frame_read; RT_FRAME_STATS takes each pixel's (n, sum_y, sum_y2) from its owner, nothing
 *   is added, and RT_FRAME_FEATURES likewise takes each pixel's feature sums from its owner's plane. out: host memory, or memory of devices[0] with RT_FLAG_FILM_ON_DEVICE in `flags`. The frame owns every buffer of the read: an rt_multi_render on the
 *   same rt_multi between two steps disturbs nothing.
 * rt_multi_frame_query: RT_FRAME_SAMPLES_DONE, RT_FRAME_SPP as for one frame; RT_FRAME_TABLES_RESIDENT: 1 only if resident on every worker that owns pixels;
 *   RT_FRAME_STATE_BYTES (the workers' frames and the buffers of the read), RT_FRAME_SAMPLES_TAKEN, RT_FRAME_ACTIVE_PIXELS: sums over the workers.
 * A MULTI FRAME MUST BE ENDED BEFORE rt_multi_destroy. rt_multi_frame_end(NULL) is a no-op. Thread safety is rt_multi_render's: calls on one rt_multi - its
 *   frames' calls and rt_multi_render alike - from one thread at a time.
 * What equals what. One worker: every read-out is the rt_frame's, bit for bit, for any filter. Several workers, at every step: the statistics plane is bit-equal
 *   to a single-device frame's after the same calls, and so are RT_FRAME_ACTIVE_PIXELS, RT_FRAME_SAMPLES_TAKEN and which pixels took which samples; the film is
 *   bit-equal where the filter reaches no further than the pixel and a pixel receives at most one edge splat (the caveat of rt_frame_advance), otherwise equal up
 *   to the order of the float additions, which neither rt_render nor rt_multi_render fixes. */
typedef struct rt_multi_frame rt_multi_frame;
int rt_multi_frame_begin(rt_multi* multi, const rt_camera* camera, const rt_film_desc* film, const rt_sampler_desc* sampler, const rt_path_desc* path,
                         uint32_t flags, uint64_t table_budget_bytes, rt_multi_frame** out);
int rt_multi_frame_advance(rt_multi_frame* frame, int32_t n_samples, rt_stats* total /* may be NULL */, rt_stats* per_device /* n_devices entries, may be NULL */);
int rt_multi_frame_advance_adaptive(rt_multi_frame* frame, int32_t n_samples, float threshold, float floor_y, int32_t min_samples, rt_stats* total, rt_stats* per_device);
int rt_multi_frame_read(rt_multi_frame* frame, int32_t what, float scale, uint32_t flags, void* out);
int rt_multi_frame_query(rt_multi_frame* frame, int32_t what, uint64_t* value);
void rt_multi_frame_end(rt_multi_frame* frame);

/* Dense voxel light distribution of SpatialLightDistribution (rc/lightdistrib.rs:101-179):
 * n_voxels[3]; func: nvox*n_lights, cdf: nvox*(n_lights+1), func_int: nvox (host pointers, may be NULL
 * to query n_voxels only). */
int rt_light_distribution(rt_scene* scene, int32_t n_voxels[3], float* func, float* cdf, float* func_int);

/* What rt_scene_create decided about a scene (measurement / tests): RT_QUERY_LDS_RESIDENT - 1 if the traversal kernels keep the whole tree and its
 * primitives in LDS (k_trace; the roofline of such a scene's traversal is VALU issue, its HBM bytes are ray records only), else 0. < 0: bad argument. */
enum { RT_QUERY_LDS_RESIDENT = 0, RT_QUERY_LDS_NODES_TESTED = 1 /* LDS-resident scenes: the nodes the stackless walks test (<= n_nodes: interior nodes whose test rarely fails are passed over) */,
       RT_QUERY_LDS_OCCLUSION = 2 /* 1 if the scene is too large for RT_QUERY_LDS_RESIDENT but fits ONE workgroup's 160 KB per CU (<= 2816 nodes, <= 1408 plain triangles): occlusion rays walk an LDS copy of it, closest-hit rays its bounds and link tables;
                                      RT_QUERY_LDS_NODES_TESTED then counts the occlusion walk's nodes */,
       RT_QUERY_SHADOW_PAIRS = 3 /* shadow sets (rt_shadow_sets): voxel / light pairs of the voxels a surface reaches; 0 where the scene has none */,
       RT_QUERY_SHADOW_EMPTY = 4 /* ... of them EMPTY: no shadow segment of the pair can be occluded */,
       RT_QUERY_BSDF_LAUNCHED = 5 /* the kernel the scene's last rt_bsdf_eval launched: 1 + 2 * mode + const_tex (mode 0 generic, 3 Lambert, 5 two-lobe, 6 two-lobe wide;
                                     const_tex 1: its constant-texture form), 0 before the first call */,
       RT_QUERY_NEEDS_DIFFERENTIALS = 6 /* 1 if some texture or bump map of the scene reads ray differentials (image maps, closed-form checkerboards, fbm): the shade kernels
                                           then regenerate the camera ray's at bounce 0 in the frames of a camera, and load the caller's from the ray records in a call or ray-frame step with
                                           RT_FLAG_RAY_DIFFERENTIALS; without the flag caller-supplied rays have none */,
       RT_QUERY_LDS_SPEC = 7 /* the form of the closest-hit link walk of an LDS-resident scene of plain triangles (RTX_LDS_SPEC, read by rt_scene_create; 0: leaf holders wait,
                                1: they keep walking up to the next leaf), 0 for every other scene */ };
int rt_scene_query(rt_scene* scene, int32_t what);
/* The tables rt_scene_create hands the stackless LDS walks of a small (<= 256 nodes, <= 128 primitives) or mid-size (<= 2816 / 1408) scene, computed on the host alone - no
 * device is touched (tests, offline inspection). link_kept / link_full: 9 * n_nodes + 9 words each (rows 0 - 7: closest hit by direction octant, their 8 start nodes,
 * row 8: occlusion rays, its start node; a word = (first tested node inside the node's subtree << 16) | first tested node after it, a leaf's word = bit 31 | its primitive
 * range | the same low half) over the nodes the calibration kept / over all nodes. stats (27 doubles, may be NULL): per set of calibration rays 0 - 8 the number of rays, their
 * simulated node tests with every node tested, and with the kept ones. mid != 0: the mid-size packing of a leaf's primitive range. RT_ERR_INVALID when capacity_words is short. */
int rt_link_tables(const rt_scene_desc* desc, int32_t mid, uint32_t* link_kept, uint32_t* link_full, uint64_t capacity_words, double* stats);
/* The shadow sets rt_scene_create builds for an LDS-resident plain-triangle scene of two triangle lights (host only, no device): per voxel of the light
 * distribution's grid (n_voxels, x fastest) and light, one word - RT_SHADOW_EMPTY (1): no shadow segment from a surface point of the voxel to the light
 * can be occluded; 0: walk. words: 2 per voxel (capacity_words >= 2 * voxels), or NULL; stats[0] = pairs of voxels a surface reaches and lights, stats[1] = of
 * them EMPTY. RT_ERR_INVALID for any other scene. */
int rt_shadow_sets(const rt_scene_desc* desc, uint32_t* words, uint64_t capacity_words, int32_t n_voxels[3], uint64_t* stats);
/* sizeof() of an ABI struct by its C name ("rt_stats", "rt_scene_desc", ...), or -1: lets a binding in another language check its mirror of the
 * header against the library it actually loaded (rustracer_amd/host.py does at load time; tests/test_abi_cpu.py checks every struct). */
int rt_sizeof(const char* struct_name);
/* The byte offsets at which the shade kernels' vertex bodies read their arguments in the kernarg segment (RT_SHADE_KARGS): out[0..2] = the scene
 * record, the frame parameters and the pass state (the same in k_shade, k_shade_split and k_shade_rays), out[3] = k_shade_split's hit-mask pointer, out[4] =
 * k_shade_rays' ray-differential source. tests/test_shade_kargs_cpu.py holds them to the argument metadata of the built code object. */
void rt_shade_karg_offsets(uint32_t out[5]);

const char* rt_last_error(void);
/* 1 if a gfx950 device is visible to this process, else 0 (never falls back to a CPU path). */
int rt_device_available(void);
const char* rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RTX_HIP_H */
