/*
 * mrt.h -- C-ABI of the MI355X ray engine (libmrt.so).
 *
 * Drop-in boundary for the hot path of bitfrozen/rendering-algorithms-raytracer
 * ("Miro"): per-pixel ray generation -> QBVH traversal -> Moller-Trumbore ->
 * Lambert/Blinn shade + shadow rays.  Plain C types only (no torch / HIP types in
 * the signatures; streams are passed as void*).  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *  - Return value: 0 (MRT_OK) or a negative MRT_ERR_* code; mrt_last_error()
 *    gives a thread-local message.  No C++ exception crosses this ABI
 *    (reference: bool returns + printf, src/TriangleMeshLoad.cpp:53-57).
 *  - Ownership: the library copies every input array; the caller keeps its
 *    buffers.  The scene owns its device memory; mrt_scene_destroy frees all
 *    (reference: Scene never frees Objects, src/Scene.h:17-21).
 *  - Frames are W*H, row 0 = bottom (reference src/Image.cpp:78-87,137-154).
 *  - Numerics are the reference's x86 SSE contract:
 *    hit t/a/b/prim and float RGB are bit-identical to the CPU restatement.
 */
#ifndef MRT_H
#define MRT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRT_ABI_VERSION 10

enum {
    MRT_OK = 0,
    MRT_ERR_INVALID = -1,   /* bad argument / handle                              */
    MRT_ERR_IO = -2,        /* file could not be read / parsed                    */
    MRT_ERR_HIP = -3,       /* HIP runtime failure (device, alloc, launch)        */
    MRT_ERR_BUILD = -4,     /* BVH build failed (degenerate input)                */
    MRT_ERR_NOT_BUILT = -5, /* scene used before mrt_scene_build_bvh              */
    MRT_ERR_OVERFLOW = -6,  /* traversal stack overflow detected on the device    */
    MRT_ERR_NO_DEVICE = -7  /* no HIP device visible                              */
};

enum { MRT_LAMBERT = 0, MRT_BLINN = 1 };                 /* src/Lambert.h, src/Blinn.h */
enum { MRT_POINT_LIGHT = 0, MRT_RECT_LIGHT = 1, MRT_DOME_LIGHT = 2 }; /* src/Light.h:9 lightType_t */

typedef struct mrt_scene mrt_scene;

/* Material as data (replaces virtual Material::shade, src/Material.h:18). */
typedef struct {
    int32_t type;            /* MRT_LAMBERT | MRT_BLINN                               */
    float kd[3], ka[3], ks[3];
    float spec_exp, spec_amt;/* Blinn m_specExp / m_specAmt (src/Blinn.h:59-61)       */
    float le[3];             /* Blinn m_Le, setLightEmittedColor (src/Blinn.h:45,64):
                                added to every Blinn shade() result (src/Blinn.cpp:335) */
    float emitted;           /* Blinn m_lightEmitted, setLightEmittedIntensity
                                (src/Blinn.h:44,63): with path tracing, a GI ray that
                                reaches this surface returns emitted * le
                                (src/Blinn.cpp:46-51).  Both 0 = not an emitter
                                (the Blinn ctor forces 0, src/Blinn.cpp:28-29)     */
} mrt_material;

/* Light as data (replaces virtual Light::sampleLight, src/Light.h:35). */
typedef struct {
    int32_t type;            /* MRT_POINT_LIGHT | MRT_RECT_LIGHT | MRT_DOME_LIGHT      */
    float pos[3];            /* PointLight::setPosition                                */
    float v1[3], v2[3], v3[3];/* RectangleLight::setVertices                           */
    float power;             /* Light::setPower (area scaling applied internally);
                                DomeLight::setPower = m_Gain                           */
    int32_t samples;         /* Light::setSamples                                      */
    float noise_threshold;   /* Light::setNoiseThreshold (default 0.001)               */
    int32_t cast_shadows;    /* Light::setCastShadows (a dome light always casts)      */
    int32_t texture;         /* MRT_DOME_LIGHT: DomeLight::setTexture, a texture id of
                                mrt_scene_add_texture (-1 for the other lights)        */
    int32_t transparent_shadows; /* 1 = Light::setFastShadows(false) (src/Light.h:24).
                                Point light: its walk (src/PointLight.cpp:49-70) starts
                                with sampleHit.t = distance and loops while t < distance,
                                so it never traces -- the light casts no shadow, as the
                                reference.  Rectangle / dome lights: the transparency
                                walk of src/RectangleLight.cpp:93-116 / src/DomeLight.cpp:
                                123-145 (closest-hit rays through every hit, attenuated
                                by refractAmt at front faces; ABI 9), rendered by the
                                fused kernels.  0 (zero-initialised) = m_fastShadows
                                true, the reference default (ABI 7)                   */
} mrt_light;

/* Camera (src/Camera.h:26-45): eye, lookAt, up, vertical FOV in degrees, and
 * the lens of Camera::eyeRayAdaptive (src/Camera.cpp:153-174; ABI 5):
 * aperture < 0.001 (epsilon) is a pinhole; otherwise rays start on a
 * rejection-sampled disc of radius aperture and pass through the point at
 * distance focus_plane along the pinhole direction (setAperture / setFocusPlane,
 * reference defaults 0 and 1).  shutter_speed scales getTimeSample's
 * time = 1 - r^3 * shutter_speed (src/Camera.h:44-46, default 0.001), the ray
 * time of motion-blurred objects. */
typedef struct {
    float eye[3], look_at[3], up[3];
    float fov_deg;
    float aperture, focus_plane, shutter_speed;
} mrt_camera;

/* Raw triangle mesh (TriangleMesh arrays, src/TriangleMesh.h:36-47).  The
 * reference keeps vertices and normals as 16-byte Vector3 (src/Vector3.h:19,
 * x y z + pad): pass vert_stride = normal_stride = 4 to hand those arrays over
 * without repacking; 0 (or 3) = packed x y z. */
typedef struct {
    const float* verts;      /* nv*vert_stride floats                                   */
    const float* normals;    /* nn*normal_stride floats                                 */
    const uint32_t* vidx;    /* nt*3 vertex indices (TupleI3 m_vertexIndices)           */
    const uint32_t* nidx;    /* nt*3 normal indices (TupleI3 m_normalIndices)           */
    int32_t nv, nn, nt;
    int32_t vert_stride, normal_stride;  /* floats per vertex / normal: 0 or 3 packed, 4 Vector3 */
} mrt_mesh;

typedef struct {             /* HitInfo (src/Ray.h:185-200)                            */
    float t, a, b;
    int32_t prim;            /* global object id in scene order, -1 = miss (or, for an
                                any-hit query, 1 = occluded); mrt_scene_prim_object
                                maps it to (mesh, triangle, instance) = HitInfo::obj  */
    int32_t inst;            /* HitInfo::m_proxy: ProxyObject instance of the hit,
                                -1 = a world triangle (or a miss)                      */
} mrt_hit;

typedef struct {
    int32_t nodes, leaves, prims;       /* QBVH nodes / 4-triangle leaf packets / tris */
    int32_t bin_nodes, bin_leaves;      /* binary BVH before the 4-wide collapse       */
    int32_t max_depth;
    double build_ms;
    uint64_t device_bytes;              /* node + leaf + shading arrays in HBM         */
} mrt_bvh_info;

typedef struct {
    int32_t width, height;   /* frame size                                              */
    int32_t device;          /* HIP device ordinal                                      */
    int32_t count_visits;    /* 1: instrumented launch (node/leaf visit counters)       */
    int32_t want_rgb8;       /* 1: also write tone-mapped 8-bit RGB (Image::Map)        */
    int32_t want_hits;       /* 1: also write primary mrt_hit per pixel (debug/parity)  */
    uint32_t seed;           /* stochastic configs only (counter RNG stream)            */
    /* mrt_render only: render on several HIP devices of this process.  The 32x32
     * buckets of src/Scene.cpp:90-95 are dealt bucket b -> devices[b mod n] (a
     * device may appear more than once), each device renders its share from its
     * own scene replica, and the tiles are gathered into the caller's frame.  The
     * result is bit-identical to a one-device render.  NULL / 0 = `device` only. */
    const int32_t* devices;
    int32_t n_devices;
} mrt_render_opts;

typedef struct {
    uint64_t primary_rays, shadow_rays;
    uint64_t node_visits, leaf_visits;   /* all rays; valid when count_visits was set   */
    uint64_t primary_node_visits, primary_leaf_visits; /* primary-ray launch share     */
    uint64_t primary_hits;               /* primary rays that hit geometry               */
    uint64_t primary_wave_steps;         /* count mode: sum over tiles of the max node
                                            visits of a lane (x64 = issued lane-steps)   */
    uint64_t primary_uniform_visits;     /* count mode: primary node visits made in wave
                                            steps where all active lanes were on one node */
    float kernel_ms;                     /* device time of the last frame (all launches)*/
    float primary_ms, shade_ms;          /* per launch: primary rays / shade + shadows  */
    int32_t max_stack;                   /* deepest traversal stack seen (count mode)   */
    /* count mode, per launch of the persistent render kernels (device wall clock):
     * span = first wave start -> last wave end, ramp = spread of wave starts,
     * tail = spread of wave ends (time the launch runs below full occupancy)   */
    float primary_span_us, primary_ramp_us, primary_tail_us;
    float shade_span_us, shade_ramp_us, shade_tail_us;
    uint64_t secondary_rays;             /* Blinn reflection / refraction / GI rays traced */
    /* count mode, wavefront shadow_kernel: wave loop steps and node visits (lane
     * utilisation = shadow_node_visits / (64 * shadow_wave_steps)) */
    uint64_t shadow_wave_steps, shadow_node_visits;
    /* 1: the frame ran as ONE launch (frame1_kernel: camera rays, closest hits,
     * shading and shadow rays fused; one point light, one path); primary_ms is
     * then the whole frame and shade_ms ~0 (ABI 7) */
    int32_t fused;
    /* 1: the frame's shading ran the wavefront chain engine (secondary rays,
     * dispersive splits, path tracing; with adaptive supersampling as passes
     * over it) rather than one fused kernel (ABI 7) */
    int32_t chain;
    /* chain engine: the per-stream chunk budget its last frame was cut to (bytes,
     * at most the mrt_set_tuning("chain_mb") cap, 80% of the free memory and the
     * stream's share of 80% of the device) and the chunks it ran (ABI 8) */
    uint64_t chain_budget_bytes;
    uint32_t chain_chunks;
    /* chunks whose level counts outgrew the capacities estimated from earlier chunks
     * on the stream (mrt_set_tuning "chain_est"): their units were rendered again by
     * the fused chain shading -- same frame, slower (ABI 9) */
    int32_t chain_fallbacks;
} mrt_stats;

const char* mrt_last_error(void);
int mrt_abi_version(void);
/* Number of visible HIP devices (0 when none); never initialises a context. */
int mrt_device_count(void);

/* ---- scene construction: Scene::addObject/addLight/preCalc (src/Scene.h:17-28) */
mrt_scene* mrt_scene_create(void);
void mrt_scene_destroy(mrt_scene* s);
/* returns material id >= 0 */
int mrt_scene_add_material(mrt_scene* s, const mrt_material* m);
/* returns light id >= 0 */
int mrt_scene_add_light(mrt_scene* s, const mrt_light* l);
/* TriangleMesh::load(file, ctm) + makeMeshObjs (src/TriangleMeshLoad.cpp:50-214).
 * ctm16: row-major 4x4 or NULL (identity).  Returns mesh id >= 0. */
int mrt_scene_add_obj(mrt_scene* s, const char* path, const float* ctm16, int material);
/* Raw mesh (TriangleMesh::createSingleTriangle + setV1..3 / setN1..3, src/TriangleMesh.cpp:11-42). */
int mrt_scene_add_mesh(mrt_scene* s, const mrt_mesh* mesh, int material);
int mrt_scene_mesh_info(const mrt_scene* s, int mesh, int32_t* nv, int32_t* nn, int32_t* nt);
int mrt_scene_mesh_export(const mrt_scene* s, int mesh, float* verts, float* normals,
                          uint32_t* vidx, uint32_t* nidx);
/* TriangleMesh m_texCoords / m_texCoordIndices of a mesh added with
 * mrt_scene_add_mesh (OBJ files load their vt lines): n_texcoords (u, v) pairs
 * and 3 indices per triangle.  HitInfo::getAllInfos interpolates (u, v) and the
 * tangent frame TriangleMesh::preCalc derives (src/Ray.cpp:33-47,
 * src/TriangleMesh.cpp:105-148); without texture coordinates (u, v) = (a, b). */
int mrt_scene_mesh_set_texcoords(mrt_scene* s, int mesh, const float* uv, int32_t n_texcoords, const uint32_t* tidx);
int mrt_scene_mesh_texcoords(const mrt_scene* s, int mesh, int32_t* n_texcoords, float* uv, uint32_t* tidx);
/* MBObject(material, mesh, mesh_t2, i) for every triangle of `mesh`
 * (src/MBObject.cpp:7-11, src/MBObject.h): verts2 = m_mesh_t2's vertices,
 * n_vertices x 3 floats, same topology.  A ray of time t meets
 * t*verts2 + (1-t)*verts; shading uses the time-0 mesh.  World meshes only
 * (instanced BLAS meshes stay static, as in the reference). */
int mrt_scene_set_mesh_motion(mrt_scene* s, int mesh, const float* verts2);
/* Scene::setBGColor (src/Scene.h:37) */
int mrt_scene_set_background(mrt_scene* s, const float rgb[3]);
/* Scene::m_numPaths (src/Scene.h:61): shade() calls per primary hit */
int mrt_scene_set_num_paths(mrt_scene* s, int num_paths);
/* Blinn::setReflectAmt / Material::setRefractAmt / Blinn::setIor (src/Blinn.h:38-41,
 * src/Material.h:32; Blinn ctor defaults 0, 0, 1.5, src/Blinn.h:11-22): reflection and refraction rays of Blinn::shade (src/Blinn.cpp:238-330),
 * Fresnel-weighted Russian roulette, at most 5 bounces, IOR history per ray.
 * No effect on Lambert materials. */
int mrt_scene_set_material_optics(mrt_scene* s, int material, float reflect_amt, float refract_amt, float ior);
/* (ior is m_ior[1]: it also replaces the middle IOR of mrt_scene_set_material_dispersion,
 * as the reference keeps one m_ior[3] array.) */
/* Material::m_disperse + Blinn::setIor(ior, i) for i = 0..2 (src/Material.h:45,
 * src/Blinn.h:38,59; ABI 6).  `ior` replaces all three m_ior; ior[1] is also the
 * optics IOR above (the non-dispersive refraction reads m_ior[1], src/Blinn.cpp:183).
 * With disperse set, a ray that is not itself a refraction ray and refracts at
 * this material splits into three refraction rays through ior[0], ior[1], ior[2],
 * each child's colour masked to its channel (src/Blinn.cpp:169-173,275-301). */
int mrt_scene_set_material_dispersion(mrt_scene* s, int material, int disperse, const float ior[3]);
/* Blinn::setReflectGloss (src/Blinn.h:42; default 1): below 1 the reflection
 * vector is blended with a cosine-distributed sample
 * (Material::getCosineDistributedSamples, src/Material.cpp:14-41; src/Blinn.cpp:166-171). */
int mrt_scene_set_material_gloss(mrt_scene* s, int material, float gloss);
/* Material::setTranslucency (src/Material.h:30; default 0): above 0.01 a Blinn
 * material also samples every light from the back side (-normal) and adds
 * translucency * light * kd (src/Blinn.cpp:224-236), as the reference's leaf
 * materials do (src/main.cpp:253, src/Assignment3.h:70). */
int mrt_scene_set_material_translucency(mrt_scene* s, int material, float translucency);
/* Blinn::setLightEmittedIntensity / setLightEmittedColor after the material was
 * added (same fields as mrt_material.emitted / le). */
int mrt_scene_set_material_emission(mrt_scene* s, int material, float emitted, const float le[3]);
/* Material::setSampleEnv (src/Material.h:27; default true): a path-tracing GI ray
 * that misses takes the environment colour only when both this flag and the
 * scene's (mrt_scene_set_path_trace) are set (src/Blinn.cpp:70-73). */
int mrt_scene_set_material_sample_env(mrt_scene* s, int material, int sample_env);
/* Scene::m_pathTrace / m_maxBounces / setSampleEnv (src/Scene.h:40,48,57-64;
 * defaults false, 10; the reference never initialises m_sampleLightFromEnv, read
 * here as false): Blinn::calculatePathTracing (src/Blinn.cpp:39-89) adds one
 * cosine-distributed GI ray per direct-lighting shade() while the ray's GI bounce
 * count is below max_bounces - 1, and samples the lights directly at the last
 * bounce.  1 <= max_bounces <= 64. */
int mrt_scene_set_path_trace(mrt_scene* s, int enable, int max_bounces, int sample_env);
/* Scene::setMinSubdivs / setMaxSubdivs / setNoise (src/Scene.h:42-55; defaults
 * 1, 1, 0.01 at src/Scene.cpp:20-22): adaptive supersampling of
 * Scene::adaptiveSampleScene (src/Scene.cpp:252-293).  With both counts 1 a
 * frame is one ray per pixel; otherwise levels 2.. of n x n jittered sub-samples
 * run until the gamma-space change is below noise (at least up to min_subdivs,
 * at most max_subdivs).  1 <= min_subdivs <= max_subdivs <= 16. */
int mrt_scene_set_subdivs(mrt_scene* s, int min_subdivs, int max_subdivs, float noise_threshold);
/* ---- images and image-based lighting -------------------------------------
 * HDRLoader::load (src/hdrloader.cpp:29-97, via RawImage::loadImage/loadHDR,
 * src/RawImage.cpp:16-32): mrt_hdr_info reads the header, mrt_hdr_load decodes
 * into caller memory, width*height*3 floats, row 0 = the top (first) scanline. */
int mrt_hdr_info(const char* path, int32_t* width, int32_t* height);
int mrt_hdr_load(const char* path, float* rgb, int32_t width, int32_t height);
/* new RawImage(w, h, data, HDR) + new Texture(image) (src/RawImage.cpp:9-14,
 * src/Texture.h:13): copies width*height*3 floats (row 0 = top).  Returns the
 * texture id (<= 16 per scene). */
int mrt_scene_add_texture(mrt_scene* s, const float* rgb, int32_t width, int32_t height);
/* RawImage::loadImage (src/RawImage.cpp:16-188) by extension: .tga (uncompressed
 * 8/24/32-bit, rows flipped, colour through Image::gamma_to_linear, alpha / 255,
 * B/R swapped), .ppm (P6, bytes / 255) or .hdr.  type: MRT_TEX_HDR (3 floats per
 * texel), MRT_TEX_GRAY (1), MRT_TEX_RGB (3), MRT_TEX_RGBA (4); data holds
 * width*height*channels floats in RawImage m_rawData order (ABI 5). */
enum { MRT_TEX_HDR = 0, MRT_TEX_GRAY = 1, MRT_TEX_RGB = 3, MRT_TEX_RGBA = 4 };
int mrt_image_info(const char* path, int32_t* width, int32_t* height, int32_t* type);
int mrt_image_load(const char* path, float* data, int32_t width, int32_t height);
/* new RawImage(w, h, data, type) + new Texture(image) for any RawImage type
 * (Texture::getPixel per type, src/Texture.cpp:100-125).  Returns the texture id. */
int mrt_scene_add_texture_typed(mrt_scene* s, const float* data, int32_t width, int32_t height, int32_t type);
/* Material::setColorMap / setNormalMap / setSpecularMap / setReflectMap /
 * setRefractMap / setAlphaMap (src/Material.h:20-25): maps[6] texture ids in that
 * order, -1 = none.  Lambert uses the colour map (src/Lambert.cpp:32-36); Blinn all
 * of them (src/Blinn.cpp:114-142); an alpha map makes intersect4 skip a
 * triangle whose alpha at the hit is below 0.5 (src/BVH.cpp:1397-1445), for
 * closest-hit and shadow rays.  Alpha maps apply to world (non-instanced) meshes. */
int mrt_scene_set_material_maps(mrt_scene* s, int material, const int32_t maps[6]);
/* Scene::setEnvMap + Scene::setEnvExposure (src/Scene.h:23-24): primary rays
 * that miss return the lat-long lookup x exposure instead of the background
 * (src/Scene.cpp:236-239).  texture = -1 clears. */
int mrt_scene_set_env_map(mrt_scene* s, int32_t texture, float exposure);
/* Material::setEnvMap + m_envExposure (src/Material.h:19,41-42; ABI 9): a Blinn
 * material's missed reflection / refraction / path-tracing GI rays take this map
 * x exposure instead of the scene's (Material::getEnvironmentColor,
 * src/Material.cpp:44-64).  An RGB / HDR texture id, or -1 = the scene's. */
int mrt_scene_set_material_env_map(mrt_scene* s, int material, int32_t texture, float exposure);
/* Importance tables of dome light `light` (DomeLight::setTexture,
 * src/DomeLight.cpp:8-78), for inspection: cdf_u[nu+1], func_u[nu],
 * cdf_v[nu*(nv+1)], func_v[nu*nv], func_int[nu+1] (column integrals, then the u
 * integral), cos_u/sin_u[nu+1], cos_v/sin_v[nv+1]. */
int mrt_scene_dome_info(const mrt_scene* s, int32_t light, int32_t* nu, int32_t* nv);
int mrt_scene_dome_export(const mrt_scene* s, int32_t light, float* cdf_u, float* func_u, float* cdf_v,
                          float* func_v, float* func_int, float* cos_u, float* sin_u, float* cos_v, float* sin_v);

/* ---- instancing: ProxyObject (src/ProxyObject.cpp:5-95,131-167) -----------
 * mrt_scene_make_blas builds a proxy BVH from meshes already added
 * (ProxyObject::setupMultiProxy: the meshes in order, each mesh's triangles last
 * to first, then BVH::build); those meshes leave the world object list.  Returns
 * the BLAS id.  mrt_scene_add_instance adds one ProxyObject (row-major 4x4
 * m_transform; ProxyMatrix derives the inverse and inverse transpose); it joins
 * the world objects in call order with the world meshes.  Hit ids (mrt_hit.prim):
 * world objects 0..n-1 (mrt_bvh_info.prims = n; a proxy's own slot never hits),
 * then instance i's BLAS objects at n + (BLAS sizes of the instances before i) +
 * BLAS object index.  blas_info/export give a BLAS's canonical QBVH arrays
 * (same layout as mrt_scene_bvh_export). */
int mrt_scene_make_blas(mrt_scene* s, const int32_t* meshes, int32_t n_meshes);
int mrt_scene_add_instance(mrt_scene* s, int32_t blas, const float* m16);
int mrt_scene_blas_info(const mrt_scene* s, int32_t blas, int32_t* nodes, int32_t* leaves, int32_t* prims);
int mrt_scene_blas_export(const mrt_scene* s, int32_t blas, float* node_boxes, int32_t* node_child,
                          float* leaf_tris, int32_t* leaf_prims);

/* Scene::preCalc -> BVH::build (src/Scene.cpp:62-79, src/BVH.cpp:457-575):
 * binned SAH, 4-wide collapse, host-side; then uploads to the device lazily. */
int mrt_scene_build_bvh(mrt_scene* s);
int mrt_scene_bvh_info(const mrt_scene* s, mrt_bvh_info* info);
/* HitInfo::obj / m_proxy of a hit id (mrt_hit.prim): the Object's mesh id and
 * triangle index (Object::m_mesh / m_index, src/Object.h:49-77) and the
 * ProxyObject instance (-1 = a world triangle).  Valid after mrt_scene_build_bvh. */
int mrt_scene_prim_object(const mrt_scene* s, int32_t prim, int32_t* mesh, int32_t* tri, int32_t* inst);
/* Canonical QBVH arrays: node_boxes[24*nodes] (minX4 minY4 minZ4 maxX4 maxY4 maxZ4),
 * node_child[4*nodes] (>=0 inner node, ~leaf for a leaf slot, INT32_MIN empty),
 * leaf_tris[36*leaves] (Ax4 Ay4 Az4 e0x4 e0y4 e0z4 e1x4 e1y4 e1z4),
 * leaf_prims[4*leaves] (-1 empty).  (QBVH_Node / TriCache4, src/BVH.h:37-109) */
int mrt_scene_bvh_export(const mrt_scene* s, float* node_boxes, int32_t* node_child,
                         float* leaf_tris, int32_t* leaf_prims);
/* Replace the built hierarchy with given canonical arrays (identical-BVH tests). */
int mrt_scene_bvh_import(mrt_scene* s, int32_t nodes, int32_t leaves, const float* node_boxes,
                         const int32_t* node_child, const float* leaf_tris, const int32_t* leaf_prims);
/* Copy the scene to device `device` (done implicitly by render/trace). */
int mrt_scene_upload(mrt_scene* s, int device);

/* ---- geometry that moves between frames: refit (no reference counterpart: the
 * reference rebuilds).  Replace the vertices (nv*3 floats, packed) and, when not NULL,
 * the normals (nn*3) of world mesh `mesh`, same counts and topology, then refit the
 * world hierarchy on every uploaded replica of the scene: the tree keeps its topology,
 * the leaf triangles are recomputed from the vertices and every box from its children
 * (std::min / std::max merges in lane and slot order, so the result is exact and stated
 * bit for bit; DESIGN.md "Refit").  Tree quality degrades under large deformation:
 * mrt_scene_rebuild_bvh (below) gives the world hierarchy a new topology on the device, and
 * mrt_scene_bvh_cost measures when; mrt_scene_build_bvh remains the way to the best tree.
 * *refit_ms (nullable): device time of the refit kernels on the current device.
 * Scope:
 *  - world (non-instanced) meshes without mrt_scene_set_mesh_motion.  A mesh of a BLAS
 *    or a motion-blurred mesh returns MRT_ERR_INVALID (a BLAS refit moves the instance
 *    box and the world tree above it; an MBObject lane's box needs both vertex sets).
 *    Scenes that hold instances or motion-blurred meshes beside the updated mesh are
 *    fine: a ProxyObject lane keeps the box it has now (the build's, or the one
 *    mrt_scene_update_instances gave it since), an MBObject lane the build's.
 *  - a scene whose hierarchy came from mrt_scene_bvh_import (it may share nodes between
 *    parents) returns MRT_ERR_INVALID; an unbuilt scene MRT_ERR_NOT_BUILT.
 *  - arguments are checked before any device call; every vertex and normal must be
 *    finite, else MRT_ERR_INVALID with the first bad index in mrt_last_error.
 *  - a scene that is built but not uploaded (or due for a re-upload) is refitted on the
 *    host: the same arithmetic.
 *  - a mesh with texture coordinates gets its tangent frames recomputed on the host
 *    (TriangleMesh::preCalc) and uploaded.
 * After an update of an uploaded scene mrt_scene_bvh_export returns the arrays the
 * device holds, read back and converted to the canonical layout.
 * mrt_scene_deform_mesh (below) takes the two kinds of mesh refused here. */
int mrt_scene_update_mesh(mrt_scene* s, int mesh, const float* verts,
                          const float* normals, float* refit_ms);
/* The same with device pointers, enqueued on `stream`, never synchronising (the first
 * refit of a replica allocates and uploads its schedule).  Acts on the scene's current
 * device; the vertices never visit the host, and are not checked: they must be finite.
 * It needs the scene uploaded to exactly one device (else MRT_ERR_INVALID) and refuses
 * a mesh with texture coordinates (its tangent accumulation is order-dependent and
 * stays on the host).  The host copy is left stale: mrt_scene_bvh_export,
 * mrt_scene_mesh_export, a re-upload after a scene change and an upload to a second
 * device first read the device state back, synchronising. */
int mrt_scene_update_mesh_async(mrt_scene* s, int mesh, const float* d_verts,
                                const float* d_normals, void* stream);

/* ---- instances that move between frames: ProxyMatrix::set (src/ProxyMatrix.cpp:17-22)
 * for instances of a built scene, followed by a refit where the reference rebuilds.
 * m16s holds n row-major 4x4 m_transform matrices for the instances ids[0 .. n)
 * (ids == NULL: instances 0 .. n-1).  Per instance m_transform, m_inverse, m_invTranspose
 * and the ProxyObject::getAABB box are recomputed exactly as mrt_scene_add_instance does,
 * then the world hierarchy is refitted on every uploaded replica as mrt_scene_update_mesh
 * does: the topology, the BLAS arrays and every hit id stay.  On the device one kernel
 * restates the host arithmetic bit for bit (DESIGN.md "Instance refit").
 * *refit_ms (nullable): device time of the kernels on the current device.  n == 0: MRT_OK.
 *  - every argument is checked before any device call and before any change: a batch is
 *    all or nothing.  MRT_ERR_INVALID for a null scene or null matrices, a hierarchy from
 *    mrt_scene_bvh_import, an id out of range or repeated in the batch (the id is in
 *    mrt_last_error), a matrix with an entry that is not finite, and a matrix whose
 *    computed inverse or box is not finite, which covers a singular one (mrt_last_error
 *    names its position in the batch); MRT_ERR_NOT_BUILT for an unbuilt scene.
 *  - a scene that is built but not uploaded (or due for a re-upload) is updated and
 *    refitted on the host: the same arithmetic.
 * New vertices for a mesh of a BLAS or a motion-blurred mesh: mrt_scene_deform_mesh.
 * Out of scope: adding or removing instances, changing an instance's BLAS, any
 * automatic rebuild (tree quality degrades as instances travel: mrt_scene_rebuild_bvh
 * below), and the shim. */
int mrt_scene_update_instances(mrt_scene* s, const int32_t* ids, int32_t n,
                               const float* m16s, float* refit_ms);
/* The same for the contiguous range [first, first + n) with the matrices on the device,
 * enqueued on `stream`, never synchronising (the first refit of a replica allocates and
 * uploads its schedule).  The range is checked on the host; the matrices are not checked:
 * they must be finite and invertible.  It needs the scene uploaded to exactly one device
 * (else MRT_ERR_INVALID).  The host copy is left stale: mrt_scene_bvh_export,
 * mrt_scene_instance_info, a host refit, a re-upload after a scene change and an upload
 * to a second device first read the device state back, synchronising. */
int mrt_scene_update_instances_async(mrt_scene* s, int32_t first, int32_t n,
                                     const float* d_m16s, void* stream);
/* What an instance holds now: its BLAS id, m_transform, m_inverse, m_invTranspose
 * (row-major 4x4 each) and its ProxyObject::getAABB box (min xyz, max xyz); every output
 * is nullable.  After an async update it reads the device state back (synchronises). */
int mrt_scene_instance_count(const mrt_scene* s);
int mrt_scene_instance_info(const mrt_scene* s, int32_t inst, int32_t* blas, float m16[16],
                            float inv16[16], float inv_t16[16], float box6[6]);

/* ---- any mesh deformed in place: same counts, same triangles, new positions (DESIGN.md
 * "Deform").  verts (nv*3) and, when not NULL, normals (nn*3) replace the mesh's own; the
 * kind of mesh decides the rest:
 *  - a plain world mesh: exactly mrt_scene_update_mesh (verts2 must be NULL).
 *  - a mesh of a BLAS (verts2 must be NULL: a BLAS mesh's motion vertices are inert, only
 *    world meshes make MBObjects): that BLAS is refitted in place (leaf triangles A, B-A,
 *    C-A, packet boxes merged in lane order from the empty box, node boxes per height,
 *    deepest first: mrt_scene_blas_export states the result), then the
 *    ProxyObject::getAABB box of every instance of that BLAS is recomputed from the new
 *    root and the instance's current m_transform (mrt_scene_add_instance's arithmetic;
 *    m_inverse and m_invTranspose stay), then the world hierarchy is refitted.  Hit ids,
 *    child words, leaf prims, every other BLAS and the boxes of its instances stay.
 *  - a motion-blurred world mesh (mrt_scene_set_mesh_motion): verts2 (nv*3, time 1) is
 *    required beside verts (time 0); each of its MBObject boxes becomes the union of the
 *    triangle's box at both times (later update_mesh / update_instances calls keep it),
 *    then the world hierarchy is refitted.
 * Everything is checked before any device call and before any change.  MRT_ERR_INVALID
 * for a null scene or null verts, a bad mesh id, verts2 given for a mesh without motion
 * vertices or missing for one with them, a vertex, motion vertex or normal that is not
 * finite (the first bad index is in mrt_last_error) and a hierarchy from
 * mrt_scene_bvh_import; MRT_ERR_NOT_BUILT for an unbuilt scene.  A scene that is built but
 * not uploaded (or due for a re-upload) is deformed on the host: the same arithmetic.  A
 * mesh with texture coordinates gets its tangent frames recomputed on the host.
 * *refit_ms (nullable): device time of the kernels on the current device.
 * Out of scope: motion-blurred meshes inside a BLAS, topology changes, any rebuild
 * heuristic, and the shim. */
int mrt_scene_deform_mesh(mrt_scene* s, int mesh, const float* verts, const float* verts2,
                          const float* normals, float* refit_ms);
/* The same with device pointers, enqueued on `stream`, never synchronising (the first refit
 * of a replica allocates and uploads its schedule).  Only the id and the kind of mesh are
 * checked; the arrays must be finite.  It needs the scene uploaded to exactly one device
 * and refuses a mesh with texture coordinates.  The host copy is left stale:
 * mrt_scene_bvh_export, mrt_scene_blas_export, mrt_scene_mesh_export,
 * mrt_scene_instance_info, mrt_scene_add_instance, mrt_scene_update_instances, a host refit,
 * a re-upload and an upload to a second device first read the device state back. */
int mrt_scene_deform_mesh_async(mrt_scene* s, int mesh, const float* d_verts, const float* d_verts2,
                                const float* d_normals, void* stream);

/* ---- the world hierarchy rebuilt on the device (no reference counterpart: Scene::preCalc ->
 * BVH::build on the host is what the reference does between frames; DESIGN.md "Rebuild").
 * A new topology for the WORLD hierarchy from the lanes its packets hold now -- plain
 * triangles, ProxyObject lanes and MBObject lanes -- with no re-upload: a lane's box is the
 * one a refit gives it; its key is the 30-bit Morton code of the box centre in the root box
 * over its current position (4 * packet + lane); the sorted lanes fill packets four at a
 * time, triangle data and prim words moved as they are; a binary radix tree over the packet
 * keys (Karras 2012) is cut into 4-wide nodes, two bit levels per node.  Hit ids, BLASes,
 * instance records, PrimShade records, vertices and every other array stay.  The result is a
 * function of the input alone and is stated by mrt_scene_bvh_export (nodes numbered breadth
 * first).  The tree is a Morton tree: worse than mrt_scene_build_bvh's on the geometry that
 * one was built for.  Against a refitted tree it is expected to win where objects have changed
 * places under the world tree (64 instances with permuted positions: the frame 26% faster)
 * and measured slower where one mesh of large triangles deforms (DESIGN.md "Rebuild" has both
 * tables): mrt_scene_bvh_cost and a timed frame decide.
 * Conventions of mrt_scene_update_mesh / _async: everything is checked before any device call
 * and before any change (MRT_ERR_NOT_BUILT for an unbuilt scene, MRT_ERR_INVALID for a null
 * scene or a hierarchy from mrt_scene_bvh_import, MRT_ERR_OVERFLOW when the node array the
 * rebuilt tree may need would pass 4 GiB); the synchronous form acts on every uploaded
 * replica and reports in *rebuild_ms (nullable) the device time on the current one; a scene
 * that is built but not uploaded (or due for a re-upload) is rebuilt on the host by the same
 * rule.  The first rebuild of a replica allocates its scratch and, where the new tree may
 * need more nodes than the world's range holds, grows the node array once.  A rebuilt replica
 * does not take the LDS top-node walk (lds_nodes) until it is uploaded again.
 * mrt_scene_bvh_info reports the new nodes and leaves; bin_*, max_depth and build_ms stay the
 * host build's. */
int mrt_scene_rebuild_bvh(mrt_scene* s, float* rebuild_ms);
/* The same enqueued on `stream`, never synchronising after the first rebuild of a replica.
 * That first one allocates and, where the node array has to grow, waits for the device once
 * (hipDeviceSynchronize) and copies the nodes into the larger array before it enqueues: call
 * it once outside a stream capture and outside a latency-critical frame.  It needs the scene uploaded to exactly one device (else MRT_ERR_INVALID).  The
 * node count and the topology are then known on the device alone: mrt_scene_bvh_export,
 * mrt_scene_bvh_info, mrt_scene_bvh_cost, the next refit of any kind, a re-upload and an upload
 * to a second device first read them back, synchronising once; renders and ray queries need
 * nothing from the host. */
int mrt_scene_rebuild_bvh_async(mrt_scene* s, void* stream);
/* The measure a caller decides with, in double on the host over the canonical arrays (read
 * back first after a device refit or rebuild): the sum over every used node slot of
 * area(slot box) / area(root box), an inner slot once and a leaf slot once per lane of its
 * packet; the root box is the merge of node 0's used slots; a zero root area gives 0. */
int mrt_scene_bvh_cost(const mrt_scene* s, double* cost);

/* ---- relighting in place: lights, a material's base record and the texels of a texture
 * change on the replicas without a re-upload (the setters above mark the scene for one).
 * Conventions of mrt_scene_update_mesh / _async: every argument is checked, with its own
 * text in mrt_last_error, before any device call and before any change; the synchronous
 * forms update every uploaded replica (they wait for the device first); the async forms
 * need the scene uploaded to exactly one device, enqueue on `stream` and never synchronise
 * (the first texture update of a replica allocates its scratch); a scene that is not
 * uploaded (or due for a re-upload) is updated on the host; ordering against launches in
 * flight on other streams is the caller's.
 *
 * mrt_scene_update_lights: Light::setPosition / setVertices / setPower / setSamples /
 * setNoiseThreshold / setCastShadows (src/Light.h:20-29, src/PointLight.h, src/RectangleLight.h,
 * src/DomeLight.h:52) on the lights that exist.  lights[n] replaces the parameters of the
 * scene's n lights, converted as mrt_scene_add_light converts them; n must be the scene's
 * light count, and every light keeps its type, its texture (dome) and its
 * transparent_shadows (MRT_ERR_INVALID names the light and the field).  Both forms take a
 * host pointer: the records travel as a kernel argument, so the update is stream-ordered. */
int mrt_scene_update_lights(mrt_scene* s, const mrt_light* lights, int32_t n);
int mrt_scene_update_lights_async(mrt_scene* s, const mrt_light* lights, int32_t n, void* stream);
/* Lambert::setKd / setKa, Blinn::setKd / setKa / setKs / setSpecExp / setSpecAmt /
 * setLightEmittedColor / setLightEmittedIntensity (src/Lambert.h:15-16, src/Blinn.h:30-45) on
 * an existing material: the mrt_material fields (what mrt_scene_add_material set) and the
 * derived emitter flag; the type must not change.  Optics, maps, environment map, gloss,
 * translucency and dispersion stay as their setters left them. */
int mrt_scene_update_material(mrt_scene* s, int material, const mrt_material* m);
int mrt_scene_update_material_async(mrt_scene* s, int material, const mrt_material* m, void* stream);
/* RawImage texels replaced (src/RawImage.h:21 m_rawData), same width, height and type:
 * W*H*channels floats.  Environment maps and material maps read the new texels where the old
 * ones were.  For every dome light of this texture DomeLight::setTexture
 * (src/DomeLight.cpp:8-78) runs again, on the device, to the bits of the host build.  The
 * update commits or does nothing: a texture whose Distribution1D integral is not positive
 * and finite is refused as by mrt_scene_add_light (MRT_ERR_INVALID), texels and tables
 * staying as they were.  *update_ms (nullable): device time on the current device.
 * The async form reads d_data (device memory) on `stream`; a refused update is counted on
 * the device instead.  Afterwards the host copy is stale (the tables after either form, the
 * texels after the async one): mrt_scene_dome_export, mrt_scene_dome_export_derived,
 * mrt_scene_add_light, a re-upload and an upload to a second device first read it back. */
int mrt_scene_update_texture(mrt_scene* s, int32_t texture, const float* data, float* update_ms);
int mrt_scene_update_texture_async(mrt_scene* s, int32_t texture, const float* d_data, void* stream);
/* *rejected: async texture updates refused since the last call (one device word is read and
 * cleared; the caller has synchronised the streams it used); 0 for a scene not uploaded. */
int mrt_scene_texture_update_status(mrt_scene* s, int32_t* rejected);
/* The derived tables of the device sampler mrt_scene_dome_export leaves out (DomeLight has no
 * counterpart): rad[(nu+1)*(nv+1)*4], guide_u[nu+1], guide_v[nu*(nv+1)]. */
int mrt_scene_dome_export_derived(const mrt_scene* s, int32_t light, float* rad, int32_t* guide_u,
                                  int32_t* guide_v);
/* How many times this scene has been uploaded to a device (one per replica made); no
 * reference counterpart: a probe for tests. */
int mrt_scene_upload_count(const mrt_scene* s);

/* ---- frame entry: Scene::raytraceImage(Camera*, Image*) (src/Scene.cpp:85-217).
 * Synchronous, host buffers: rgb (W*H*3 floats, before Map) and rgb8 (W*H*3,
 * after Image::Map; nullable); hits (W*H, nullable).  1 spp primary + shadow. */
int mrt_render(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts,
               float* rgb, uint8_t* rgb8, mrt_hit* hits);

/* ---- bucketed device render for multi-GPU tiling (src/Scene.cpp:90-174 buckets).
 * Renders the 32x32 buckets listed in d_buckets (device int32 ids, row-major
 * bucket grid) into d_tiles: n_buckets * 32*32*3 floats, bucket-major, pixels
 * row-major inside a bucket (pixels outside the frame left untouched).
 * Everything is enqueued on `stream` (hipStream_t, NULL = default); returns
 * without synchronising.  Device pointers come from the caller (e.g. torch). */
int mrt_render_buckets_async(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts,
                             const int32_t* d_buckets, int32_t n_buckets, float* d_tiles,
                             void* stream);
/* Scatter bucket tiles into a W*H*3 float frame (and optional W*H*3 rgb8). */
int mrt_unpack_buckets_async(const int32_t* d_buckets, int32_t n_buckets, const float* d_tiles,
                             int32_t width, int32_t height, float* d_frame, uint8_t* d_frame8,
                             const mrt_scene* s_for_lut, void* stream);
/* ---- batched bucket render: several frames (cameras) in one launch pair.
 * Same bucket loop (src/Scene.cpp:90-174) over a batch of n_cams <= 16 frames of
 * one size (e.g. a camera path, or one frame's buckets dealt across GPUs).
 * d_items: device int32 ids, id = frame * buckets_per_frame + bucket, with
 * buckets_per_frame = ceil(W/32) * ceil(H/32); an id whose frame is >= n_cams
 * renders with the last camera.  Frame f uses RNG seed (opts->seed or the
 * default) + f, so it equals an mrt_render of camera f with that seed.
 * Outputs (either may be NULL, not both), slot-major like mrt_render_buckets_async:
 * d_tiles n_items*1024*3 floats; d_tiles8 n_items*1024*3 bytes (Image::Map). */
int mrt_render_batch_async(mrt_scene* s, const mrt_camera* cams, int32_t n_cams, const mrt_render_opts* opts,
                           const int32_t* d_items, int32_t n_items, float* d_tiles, uint8_t* d_tiles8,
                           void* stream);
/* Scatter batch tiles into n_frames consecutive W*H frames (frame f at offset
 * f*W*H*3).  d_frames needs d_tiles; d_frames8 copies d_tiles8 or, when it is
 * NULL, maps d_tiles through the scene's gamma LUT.  Items of frames >= n_frames
 * are skipped. */
int mrt_unpack_batch_async(const int32_t* d_items, int32_t n_items, const float* d_tiles, const uint8_t* d_tiles8,
                           int32_t width, int32_t height, int32_t n_frames, float* d_frames, uint8_t* d_frames8,
                           const mrt_scene* s_for_lut, void* stream);
/* ---- the batch render written straight into frames (ABI 10): the same items and
 * launches as mrt_render_batch_async, but each pixel goes to its place in n_cams
 * consecutive W*H frames (frame f at offset f*W*H*3 of d_frames / d_frames8, either
 * may be NULL, not both); pixels outside the frame and items of frames >= n_cams
 * write nothing.  With the frames of another process mapped by mrt_ipc_open, every
 * rank of the multi-GPU split writes its buckets into rank 0's frame directly: the
 * frame is complete when every rank's launch is (a stream-ordered barrier), with no
 * gather and no unpack (src/Scene.cpp:90-174's bucket loop, one image for all). */
int mrt_render_batch_frames_async(mrt_scene* s, const mrt_camera* cams, int32_t n_cams, const mrt_render_opts* opts,
                                  const int32_t* d_items, int32_t n_items, float* d_frames, uint8_t* d_frames8,
                                  void* stream);
/* Device memory shared between processes (hipIpcGetMemHandle / hipIpcOpenMemHandle):
 * mrt_ipc_export describes the allocation holding d_ptr (any pointer into a device
 * allocation, e.g. a torch tensor's data) and d_ptr's offset in it; mrt_ipc_open maps
 * it in this process for `device` (peer access enabled) and returns the same byte;
 * mrt_ipc_close unmaps a pointer mrt_ipc_open returned.  The handle is plain bytes
 * (send it to the other ranks over any channel). */
typedef struct {
    uint8_t handle[64];
    uint64_t offset, size;
} mrt_ipc_handle;
int mrt_ipc_export(const void* d_ptr, mrt_ipc_handle* out);
int mrt_ipc_open(const mrt_ipc_handle* h, int device, void** d_ptr);
int mrt_ipc_close(void* d_ptr);
/* Whole frame straight into device buffers (N = 1 fast path, no tiles). */
int mrt_render_frame_async(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts,
                           float* d_rgb, uint8_t* d_rgb8, void* stream);

/* ---- batched ray query: Scene::trace / BVH::intersect (src/Scene.cpp:295-298,
 * src/BVH.cpp:1112-1178).  o,d: n*3 floats; tmin,tmax: n floats.  any_hit=1
 * stops at the first accepted triangle (shadow rays; occlusion result is
 * identical to the reference's closest-hit shadow traversal). */
int mrt_trace(mrt_scene* s, const float* o, const float* d, const float* tmin, const float* tmax,
              size_t n, int any_hit, mrt_hit* out);
int mrt_trace_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_tmin,
                    const float* d_tmax, size_t n, int any_hit, mrt_hit* d_out, void* stream);

/* Scene::trace (src/Scene.cpp:295-298) for rays with a time, Ray(o, d, time) (src/Ray.h:71):
 * where an MBObject's triangle is (src/MBObject.cpp).  time: n floats, or NULL = mrt_trace
 * exactly (the same kernel, the same bytes out).  With the rays of mrt_camera_rays, tmin =
 * 0.001 and tmax = 1e12 (epsilon and MIRO_TMAX, src/Miro.h:35,56) the closest hits are the
 * hit records of mrt_sample_rays, byte for byte.  Conventions of mrt_sample_rays: argument
 * checks before any device call, n = 0 is MRT_OK, n at most 2^28, the async form takes device
 * pointers, enqueues on `stream` and never synchronises. */
int mrt_trace_rays(mrt_scene* s, const float* o, const float* d, const float* time, const float* tmin,
                   const float* tmax, size_t n, int any_hit, mrt_hit* out);
int mrt_trace_rays_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, const float* d_tmin,
                         const float* d_tmax, size_t n, int any_hit, mrt_hit* d_out, void* stream);

/* ---- batched radiance query: Scene::sampleScene (src/Scene.cpp:219-243) for n caller
 * rays.  o, d: n*3 floats (d is used as given, as Ray(o, d) does: not normalised); time:
 * n floats or NULL (= 0, the Ray ctor default; the MBObject time of src/MBObject.cpp).
 * rgb: n*3 floats (before Image::Map); hits: n primary hit records or NULL.  Ray i draws
 * from the RNG stream of "pixel" i, eye-ray sample 0, of `seed` (0 = the default seed, as
 * mrt_render_opts.seed).  row_width is a coherence hint only: > 0 says the batch is an
 * image of rows of that many rays (waves then take 8x8 blocks of it); 0 = a list (a wave
 * takes 64 consecutive rays).  Results never depend on it.  The scene's subdivision
 * setting is ignored: one sampleScene per ray.  n is at most 2^28.  Runs on the scene's
 * current device (device 0 before any upload), like mrt_trace.
 * The synchronous form copies in and out; the async form takes device pointers, enqueues
 * on `stream` and never synchronises.  Both fill mrt_scene_last_stats like a frame
 * (primary_rays = n) and report MRT_ERR_OVERFLOW the same way (the async form from
 * mrt_scene_last_stats).  On the rays of mrt_camera_rays(cam, W, H, seed) the result is
 * the float frame and the hit records of mrt_render(cam, W x H, seed), bit for bit. */
int mrt_sample_rays(mrt_scene* s, const float* o, const float* d, const float* time, size_t n,
                    int32_t row_width, uint32_t seed, int32_t count_visits,
                    float* rgb, mrt_hit* hits);
int mrt_sample_rays_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time,
                          size_t n, int32_t row_width, uint32_t seed, int32_t count_visits,
                          float* d_rgb, mrt_hit* d_hits, void* stream);
/* ---- shade caller-supplied hits: the hit branch and the miss branch of Scene::sampleScene
 * (src/Scene.cpp:224-241) -- m_numPaths Material::shade calls (src/Material.h:18) on the hit,
 * the environment map or background of the ray's direction on a miss -- for n caller (ray,
 * hit) pairs: mrt_sample_rays with its primary rays replaced by the caller's hit records.
 * o, d, time, row_width, seed, count_visits, rgb as for mrt_sample_rays; ray i draws from
 * the RNG stream of "pixel" i.  On the rays of mrt_camera_rays and the closest hits
 * mrt_trace_rays(o, d, time, 0.001, 1e12) finds for them, rgb and the ray counts of
 * mrt_scene_last_stats (shadow_rays, secondary_rays, primary_hits) equal those of
 * mrt_sample_rays, bit for bit.
 * Hit records: t, a, b and prim as mrt_trace / mrt_trace_rays (closest hit) / mrt_sample_rays
 * / mrt_render write them; prim == -1 is a miss; inst is ignored (the id names the
 * instance).  An any-hit result (any_hit = 1: prim = 1 is an occlusion flag, not an id) is
 * NOT a hit record.  The records are not trusted.  Invalid: prim < -1, prim at or above the
 * scene's hit-id count (the world objects plus every instance's BLAS objects), prim a
 * ProxyObject's own world slot (which never hits), t, a or b not finite, |a| or |b| above
 * 2^24.  The synchronous entry checks the host array before touching a device and returns
 * MRT_ERR_INVALID, the first bad index in mrt_last_error.  The async entry checks on the
 * device, before anything is indexed: an invalid record is shaded as a miss, and
 * mrt_scene_last_stats then returns MRT_ERR_INVALID (the count in mrt_last_error), the way
 * MRT_ERR_OVERFLOW is reported. */
int mrt_shade_hits(mrt_scene* s, const float* o, const float* d, const float* time, const mrt_hit* hits, size_t n,
                   int32_t row_width, uint32_t seed, int32_t count_visits, float* rgb);
int mrt_shade_hits_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, const mrt_hit* d_hits,
                         size_t n, int32_t row_width, uint32_t seed, int32_t count_visits, float* d_rgb, void* stream);

/* ---- the surface a hit names: Ray::getPoint (src/Ray.h) + HitInfo::getAllInfos
 * (src/Ray.cpp:5-49), batched.  p = o + t * d; n / geo_n the interpolated and the geometric
 * normal (through an instance's inverse transpose, src/Ray.cpp:27-31); (u, v) the
 * interpolated texture coordinates with the tangent frame tan / bitan whenever the mesh has
 * texture coordinates, else (u, v) = (a, b) and tan = bitan = 0; material the material id;
 * mesh, tri, inst = HitInfo::obj / m_proxy as mrt_scene_prim_object gives them.  What
 * Material::shade does to N afterwards (the Blinn flip, normal maps) is not applied.  Hit
 * records and their validation as for mrt_shade_hits; a miss or an invalid record writes
 * zeros and material = mesh = tri = inst = -1. */
typedef struct {
    float p[3], n[3], geo_n[3], tan[3], bitan[3], u, v;
    int32_t material, mesh, tri, inst;
} mrt_surface;
int mrt_hit_surfaces(mrt_scene* s, const float* o, const float* d, const mrt_hit* hits, size_t n, mrt_surface* out);
int mrt_hit_surfaces_async(mrt_scene* s, const float* d_o, const float* d_d, const mrt_hit* d_hits, size_t n,
                           mrt_surface* d_out, void* stream);

/* ---- sample the lights at caller points: Light::sampleLight (src/Light.h:35;
 * src/PointLight.cpp:8-81, src/RectangleLight.cpp:42-136, src/DomeLight.cpp:80-160) for n
 * caller points, every light of the scene in scene order -- what Material::shade asks of the
 * lights, without a ray, a hit or a material.  from, normal: n*3 floats, used as given
 * (nothing is normalised); rvec: n*3 floats, the reflection vector of the specular term, or
 * NULL = the zero vector, which Lambert::shade passes; time: n floats or NULL (= 0), the
 * shadow rays' time (where an MBObject's triangle is).  secondary is the isSecondary argument:
 * with it set a dome light takes one sample.
 * per_light (nullable): n * n_lights * 4 floats, for point i and light l {E.r, E.g, E.b,
 * outSpec} at (i * n_lights + l) * 4.  e (nullable; e and per_light may not both be NULL):
 * n*3 floats, the float sum of E over the lights, added in light order starting from 0 --
 * what Lambert::shade accumulates with kd = 1 and ka = 0 (src/Lambert.cpp:42-50).  A scene
 * without lights writes zeros.
 * Point i draws from the RNG stream of "pixel" i, eye-ray sample 0, path 0, of `seed` (0 =
 * the default seed), the draws numbered from the first draw of chain level 0 plus
 * first_draw: 0 is where the light loop of Lambert::shade starts, 1 where that of
 * Blinn::shade starts, after its roulette draw (src/Blinn.cpp:195).  The lights consume draws
 * in order, as in a frame.  So on the points and normals mrt_hit_surfaces gives for a
 * camera's rays, `e` is the float RGB mrt_shade_hits gives a white Lambert surface there (one
 * path), bit for bit, with the same shadow_rays.
 * Shadows are the frame's: alpha-mapped, motion-blurred and instanced occluders, and the
 * transparency walk of a rectangle / dome light with transparent_shadows.  Inputs are not
 * checked for finiteness.  Conventions of mrt_sample_rays: argument checks before any device
 * call, n = 0 is MRT_OK, n at most 2^28, the scene's current device; the synchronous form
 * copies in and out, the async form takes device pointers, enqueues on `stream` and never
 * synchronises.  mrt_scene_last_stats: shadow_rays (every trace counts), kernel_ms,
 * node_visits / leaf_visits with count_visits, primary_rays = 0; MRT_ERR_OVERFLOW as for
 * mrt_sample_rays. */
int mrt_sample_lights(mrt_scene* s, const float* from, const float* normal, const float* rvec,
                      const float* time, size_t n, uint32_t seed, uint32_t first_draw,
                      int32_t secondary, int32_t count_visits, float* e, float* per_light);
int mrt_sample_lights_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                            const float* d_time, size_t n, uint32_t seed, uint32_t first_draw,
                            int32_t secondary, int32_t count_visits, float* d_e, float* d_per_light,
                            void* stream);

/* ---- the samples behind mrt_sample_lights: what each light's loop took at each point, one
 * record per sample, and the same query through wavefront passes (gen / bin / trace /
 * resolve over the point list) instead of one fused kernel. */
typedef struct {   /* one sample a light took at a point; 32 bytes */
    float dir[3];  /* point -> light sample, as the light's loop holds it when it asks for the shadow answer */
    float dist;    /* the distance the loop computed (point, rectangle); 1e12 for a dome sample */
    float e[3];    /* what this sample adds to the light's sum at vis = 1 */
    float vis;     /* the shadow answer: 1 visible, 0 occluded or rejected */
} mrt_light_sample;

/* The most samples each light can take at a point (a built scene; no device is touched):
 * per_light[l] (nullable, n_lights entries) = 1 for a point light, max(1, samples) for a
 * rectangle light and for a dome light, 1 for a dome light with `secondary` set; *total
 * (nullable) = their sum M, the row stride of mrt_light_samples' records. */
int mrt_scene_light_sample_cap(const mrt_scene* s, int32_t secondary, int32_t* per_light, int32_t* total);

/* mrt_sample_lights with per-sample records.  from, normal, rvec, time, n, seed, first_draw,
 * secondary, count_visits, e and per_light are mrt_sample_lights' (the same RNG stream per
 * point, the same draw numbering, the same bits in e and per_light); e and per_light may both
 * be NULL here, but at least one of samples, counts, e, per_light is required.
 * counts (nullable): n * n_lights int32, the samples light l took at point i (the loop's
 * `done`): 0 for a point light facing away, and for a dome call whose every draw was rejected.
 * samples (nullable): n * M records, M from mrt_scene_light_sample_cap.  Point i's samples
 * start at row i * M, in light order, then sample order, compact; rows past the sum of the
 * point's counts are not written.
 *   point light      dir = the normalised L, dist = distance, e = A * nDotL in all three
 *                    channels; with cast_shadows 0, vis = 1 and no ray
 *   rectangle light  dir = the normalised rd, dist = dist, e = E in all three channels (no
 *                    cosine: the reference's rectangle light has none).  A sample whose nDotL
 *                    is at most 0.001 is still a sample (the loop counts it): vis = 0, dist = 0,
 *                    dir = rd as it stands (not normalised), e = the loop's E (stale falloff)
 *   dome light       dir = dir, dist = 1e12, e = m_Gain * image / pdf; a rejected
 *                    below-horizon draw is no sample (it consumes its two draws)
 * A light's {E, outSpec} is the loop's own sum over its records: acc += e * vis in order,
 * times 1 / count (a point light: e * vis).
 * Refused (MRT_ERR_INVALID, before any device call): a scene with a transparent_shadows
 * light (the wavefront shadow answer is one bit), M above 64, n * M at or above 2^32.
 * Otherwise the conventions and statistics of mrt_sample_lights: shadow_rays counts the
 * traces, kernel_ms, node_visits / leaf_visits with count_visits, primary_rays = 0,
 * MRT_ERR_OVERFLOW.  A scene without lights (M = 0) writes zeros to e and nothing else.
 * Inputs are not checked for finiteness; with finite inputs and light parameters every
 * output is deterministic and independent of the tuning's schedules. */
int mrt_light_samples(mrt_scene* s, const float* from, const float* normal, const float* rvec,
                      const float* time, size_t n, uint32_t seed, uint32_t first_draw,
                      int32_t secondary, int32_t count_visits,
                      mrt_light_sample* samples, int32_t* counts, float* e, float* per_light);
int mrt_light_samples_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                            const float* d_time, size_t n, uint32_t seed, uint32_t first_draw,
                            int32_t secondary, int32_t count_visits,
                            mrt_light_sample* d_samples, int32_t* d_counts, float* d_e, float* d_per_light,
                            void* stream);

/* Camera::eyeRayAdaptive(x, y, .5, .5, .5, .5) (src/Camera.cpp:116-174) for every pixel of
 * a width x height frame, on the host (no device is touched): the rays mrt_render traces
 * at 1 spp with this seed, index y*width + x, lens and getTimeSample time included.
 * o, d: width*height*3 floats; time: width*height floats. */
int mrt_camera_rays(const mrt_camera* cam, int32_t width, int32_t height, uint32_t seed,
                    float* o, float* d, float* time);

/* The walk of the scene's last one-light frame on its current device: *lds_nodes = 1
 * when it ran the LDS top-node walk (tuning "lds_nodes"), 0 when not, -1 before any;
 * *walk_exits = the walk loop's form of the frame / primary kernels, 1 (one exit: a
 * stack overflow empties the stack and leaves at the pop test; the default) or 2 (a
 * second exit on overflow; tuning "walk_exit" 0).  Both forms give the same bits. */
int mrt_scene_walk_info(const mrt_scene* s, int32_t* lds_nodes, int32_t* walk_exits);

/* The size limit of mrt_scene_upload: 1 when a device hierarchy of n_nodes nodes (128 B
 * each) and n_leaves leaf packets (160 B each; the world's and every BLAS's together) has
 * both arrays end within 4 GiB, else 0.  The walks address nodes and leaf triangles by
 * 32-bit byte offsets; mrt_scene_upload refuses a larger scene with MRT_ERR_OVERFLOW. */
int mrt_walk_arrays_fit(uint64_t n_nodes, uint64_t n_leaves);

/* Counters of the last render on this scene (ray counts, visits, kernel time). */
int mrt_scene_last_stats(const mrt_scene* s, mrt_stats* out);

/* Performance A/B switches (no effect on results; defaults in brackets).  Each key is
 * either selected by a default path or exercised by the GPU tests (round 6 removed the
 * rest, with their kernel instantiations; their A/B records stay in profiles/):
 * "fast_box" 0/[1] (hardware min/max slab test when its finiteness precondition holds),
 * "scalar_nodes" 0..[7] (bit 0 scalar fetch of wave-uniform nodes, bit 1 of wave-uniform
 * triangles, bit 2 octant-ordered box test), "walk_exit" 0/[1] (the frame / primary
 * kernels' walk loop: two exits, one exit), "walk_latch" 0/[1] (the frame kernel's
 * camera-ray walk: nested latches, one latch), "lds_nodes" [0]/1 (the frame kernel's LDS
 * top-node walk), "sched" 0..3 [2] (tile schedule: static grid-stride, static XCD bands,
 * dynamic interleaved, dynamic banded; see TileSched), "fused" 0/[1] (one-launch frame
 * kernel for one point light), "shade1" 0/[1] (specialised shading kernel for one point
 * light and one path), "frame1_waves" 1/5/6/[7]/8 and "primary_waves" 0/6/[7]/8 and
 * "primary_inst_waves" 1/4/[5]/6 (occupancy targets), "wavefront" 0/[1] (gen / shadow /
 * resolve passes instead of the fused shading kernel), "shadow_sched" [-1]..2 (wavefront
 * shadow rays: auto, grid-stride, XCD bands, bands + lane refill), "near_first" [-1]..1
 * (any-hit walks descend into the nearest hit child first), "dome_replay" 0/[1] (the
 * dome-light resolve pass sums the recorded samples), "bin" [-1] / 0..7 (ray binning
 * before tracing: bit 0 the wavefront shadow pass, bit 1 the chain levels' closest-hit
 * entries, bit 2 their shadow rays; -1 auto), "bin_dbits" 0..6 [2] / "bin_obits" 0..4 [2]
 * (binning key: direction and origin cells per axis as powers of two, 2 dbits + 3 obits
 * <= 12), "bin_inst" [0]..2 (instance-major shadow-ray bin keys), "chain" 0/[1] (the
 * wavefront chain engine for secondary rays), "chain_bands" [-1]..1 (XCD-banded chain
 * trace queue; -1: on for binned levels), "chain_est" 0/[1] / "chain_est_pct" [125] /
 * "chain_mb" [8192] (chain level capacities and scratch budget), "chain_shadow_step"
 * [0]/1 and "chain_shadow_refill" [0]/1 (instanced chain levels' shadow walks),
 * "adapt_refill" 0..64 [32] (adaptive pixel refill), "batch_tpw" 1..64 [2] (tiles per
 * wave a bucket batch smaller than the persistent grid is launched for), "wave_log"
 * [0]/1 (timing-only wave log, diagnostics).  Process-wide. */
int mrt_set_tuning(const char* key, int value);
/* The value a tuning key holds now (its default until set).  MRT_ERR_INVALID for a null
 * or unknown key or a null value. */
int mrt_get_tuning(const char* key, int* value);

/* Diagnostics: per-wave records of the last count-mode render (count_visits = 1)
 * for launch 0 (primary rays) or 1 (shading + shadow rays): 60 x uint64 per wave
 * {start, end (device wall clock ticks), tiles processed, node visits, then for the
 * wave's first 28 tiles: tile id << 40 | low 40 bits of the tick it started, then
 * for the same tiles the ticks their dequeue (tile-queue atomics) took}.
 * Returns the number of waves copied (<= max_waves). */
int mrt_debug_wave_log(const mrt_scene* s, int launch, uint64_t* out, int32_t max_waves);
/* Device wall-clock rate (kHz) of the scene's device, for the ticks above. */
int mrt_device_wall_clock_khz(const mrt_scene* s);

/* Numerics probes (x86 RCPSS/RSQRTSS emulation + one Newton step, SSE.h:67-101). */
/* The device's acosf(x) (fn 0) / atan2f(y, x) (fn 1) / sinf(x) (fn 3) / cosf(x) (fn 4) /
 * powf(x, y) (fn 5) over n host inputs (a kernel on the current device; glibc's code
 * restated, csrc/mrt_libm.h), or its rcp_nr(x) (fn 2: the RCPSS emulation and Newton step
 * of every triangle test; y unused). */
int mrt_debug_libm(int fn, const float* x, const float* y, size_t n, float* out);
/* Ray-binning probe: the three launches of csrc/mrt_bin.hip (keys + per-block counts, the
 * scan of the bins, the scatter) on host arrays, without a scene: every field of the
 * renderer's own binning call comes from the caller.  items = n, or with has_n_dev
 * min(n, min(cap1, n_dev * mul1 - sub) * mul2); slot i < items is valid iff nrays is null
 * or i % m < nrays[i / m].  The key of a valid slot: direction cell (dbits per axis, major)
 * and Morton code of the origin's cell (o - lo) * inv (obits per axis, minor); with hits
 * (dbits = obits = 2) a slot whose pixel's hit id (the bits of hits[4 * (i / m) + 3]) is at
 * or above n_world gets 1 << 11 | inst_class << 4 | direction cell of the last instance
 * whose hit_base is at or below it, or with inst_cell 1 << 11 | BLAS bit << 10 | Morton code
 * of its object-space cell << 4 | direction cell.  On return keys[i], i < items, holds the
 * key or 0xFFFF (invalid slot), hist[b], b < 2^bits, the number of valid slots with key <=
 * b, hist[2^bits] their total and perm[0 .. total) the valid slots in key order (bits: 12
 * with hits, else 2 dbits + 3 obits).  keys and perm are copied to the device before the
 * launches, so what they held past items / past total comes back as it was.
 * Refused (MRT_ERR_INVALID, before any device call): a null probe, o, d, keys, hist or perm,
 * m < 1, grid outside 1..1024, n at or above 2^31, inst_cell without inst_inv, hits
 * without hit_base / inst_class, an inst_class value above 127; the binning's own refusals
 * (key widths, instance tables) are returned as they are. */
typedef struct mrt_bin_probe {
    const float* o;             /* n x 4 floats: ray origins (w unused) */
    const float* d;             /* n x 4 floats: ray directions */
    uint32_t n;
    int32_t has_n_dev;          /* 1: n_dev is placed on the device as the batch's count */
    uint32_t n_dev;
    uint32_t mul1, sub, cap1, mul2;
    const uint8_t* nrays;       /* ceil(n / m) ray counts, or null */
    uint32_t m;
    float lo[3], inv[3];
    int32_t dbits, obits;
    int32_t grid;               /* workgroups of the count and scatter passes */
    const float* hits;          /* ceil(n / m) x 4 floats (t, a, b, hit id bits), or null */
    const int32_t* hit_base;    /* n_inst, ascending */
    const uint16_t* inst_class; /* n_inst, each 0..127 */
    int32_t n_inst, n_world;
    const float* inst_cell;     /* 2 n_inst x 4 floats, or null */
    const float* inst_inv;      /* n_inst x 12 floats: world-to-object matrices, 3 rows of 4 */
    uint16_t* keys;             /* n, in / out */
    uint32_t* hist;             /* 4097 words, out: the first 2^bits + 1 are written */
    uint32_t* perm;             /* n, in / out */
} mrt_bin_probe;
int mrt_debug_bin_rays(const mrt_bin_probe* p);
/* Ownership probe: the device allocations, pinned allocations, events and streams the library's
 * replicas, stream contexts and staging buffers hold in this process now.  It returns to its
 * earlier value when what was created since has been destroyed (mrt_scene_destroy). */
int64_t mrt_debug_live_resources(void);
float mrt_rcp_nr(float x);
float mrt_rsqrt_nr(float x);

#ifdef __cplusplus
}
#endif
#endif /* MRT_H */
