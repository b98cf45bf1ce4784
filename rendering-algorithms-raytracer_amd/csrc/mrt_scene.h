// mrt_scene.h -- internal scene object behind the opaque mrt_scene handle.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mrt.h"
#include "mrt_math.h"
#include "mrt_types.h"

namespace mrt {

// Packed x86 approximation tables (host copies; uploaded to the device).
const uint16_t* host_rcp_table();
const uint16_t* host_rsqrt_table();
const uint8_t* host_gamma_lut();  // 32769 entries, Image::generateGammaTables
const float* host_gamma_float_lut();  // Image::linear_to_gammaF, 32769 entries

struct Mesh {
    std::vector<v3> verts, normals;
    std::vector<uint32_t> vidx, nidx;
    int material = 0;
    // TriangleMesh m_texCoords (u, v pairs) / m_texCoordIndices (empty: none), and
    // the per-normal tangent frame TriangleMesh::preCalc derives from them
    std::vector<float> uv;
    std::vector<uint32_t> tidx;
    std::vector<v3> tan, btan;
    // MBObject m_mesh_t2 vertices (motion blur, src/MBObject.cpp): empty = static
    std::vector<v3> verts2;
    int32_t nt() const { return (int32_t)(vidx.size() / 3); }
};

// RawImage types (src/RawImage.h ImageType): floats per texel 3 (HDR), 1, 3, 4
enum { kTexHDR = 0, kTexGray = 1, kTexRGB = 3, kTexRGBA = 4 };
inline int tex_channels(int type) { return type == kTexGray ? 1 : type == kTexRGBA ? 4 : 3; }

struct Texture {                // RawImage (src/RawImage.h): W*H*channels floats (m_rawData order)
    std::vector<float> rgb;
    int32_t W = 0, H = 0;
    int32_t type = kTexHDR;
};

struct DomeTables {             // DomeLight::setTexture (src/DomeLight.cpp:8-78)
    int32_t tex = -1, nu = 0, nv = 0;
    std::vector<float> func_u, cdf_u, func_v, cdf_v, int_v, inv_int_v, cos_u, sin_u, cos_v, sin_v;
    float int_u = 0.f, inv_int_u = 0.f;
    // derived lookup tables of the device sampler (not reference state):
    // rad = the lat-long lookup of every table direction (iu, iv) in 0..nu x 0..nv,
    // 4 floats per cell; guide_u / guide_v = CDF guide tables (guide_table)
    std::vector<float> rad;
    std::vector<int32_t> guide_u, guide_v;
};

// A ProxyObject's BVH (ProxyObject::setupMultiProxy, src/ProxyObject.cpp:149-167):
// objects are the meshes in order, each mesh's triangles last to first.
struct Blas {
    std::vector<int32_t> meshes;
    std::vector<int32_t> obj_mesh, obj_tri;
    std::vector<QNode> nodes;
    std::vector<QLeaf> leaves;
};

// ProxyObject + ProxyMatrix (src/ProxyObject.cpp:5-12, src/ProxyMatrix.cpp:3-8)
struct Instance {
    float m[16], inv[16], inv_t[16];  // m_transform, m_inverse, m_invTranspose (row-major)
    float box[6];                     // ProxyObject::getAABB: min xyz, max xyz
    int32_t blas;
    int32_t hit_base;                 // hit id of its BLAS object 0 (set by build_qbvh)
};

struct DeviceState;  // defined in mrt_device.h

struct Scene {
    std::vector<Mesh> meshes;
    std::vector<DevMaterial> materials;
    std::vector<DevLight> lights;
    std::vector<mrt_light> light_args;   // what mrt_scene_add_light was given, per light (mrt_scene_update_lights compares)
    std::vector<Texture> textures;
    std::vector<DomeTables> domes;
    int32_t env_tex = -1;           // Scene::m_envMap (-1: background colour)
    float env_exposure = 1.f;       // Scene::m_envExposure
    float bg[3] = {0.f, 0.f, 0.f};
    int num_paths = 1;
    // Scene::m_pathTrace / m_maxBounces / m_sampleLightFromEnv (src/Scene.cpp:17-19)
    bool path_trace = false;
    int max_bounces = 10;
    bool sample_env = false;
    // Scene::m_minSubdivs / m_maxSubdivs / m_noiseThreshold (src/Scene.cpp:20-22)
    int min_subdivs = 1, max_subdivs = 1;
    float noise_threshold = 0.01f;
    // world object groups in add order: mesh id (>= 0) or ~instance id
    std::vector<int32_t> groups;
    std::vector<int32_t> mesh_blas;   // per mesh: owning BLAS, -1 = world geometry
    std::vector<Blas> blas;
    std::vector<Instance> instances;

    int32_t push_mesh(Mesh&& m) {
        meshes.push_back(std::move(m));
        mesh_blas.push_back(-1);
        groups.push_back((int32_t)meshes.size() - 1);
        built = false;
        dev_dirty = true;
        return (int32_t)meshes.size() - 1;
    }

    // objects in scene order (makeMeshObjs): global prim id -> (mesh, tri)
    std::vector<int32_t> obj_mesh, obj_tri, obj_inst;  // obj_inst >= 0: a ProxyObject
    // QBVH
    std::vector<QNode> nodes;
    std::vector<QLeaf> leaves;
    mrt_bvh_info info{};
    bool built = false;
    bool imported = false;   // nodes / leaves came from mrt_scene_bvh_import (may be a DAG: no refit)

    // mrt_scene_update_mesh on an uploaded scene refits on the device only: the replicas'
    // node boxes and leaf triangles are then ahead of nodes / leaves (host_bvh_stale), and
    // after the async form the vertices and normals of host_mesh_stale's meshes too.
    // sync_host (mrt_refit.hip) reads them back before anything reads the host copy.
    // After mrt_scene_update_instances_async the matrices, inverses and boxes of `instances`
    // are behind the replica's too (host_inst_stale).
    bool host_bvh_stale = false;
    // After mrt_scene_rebuild_bvh_async the world's node count, child words and packets are
    // behind the replica's as well (the synchronous form reads them back itself): sync_host
    // renumbers them breadth first and every replica's refit schedule is made again.
    bool host_topo_stale = false;
    std::vector<int32_t> host_mesh_stale;
    bool host_inst_stale = false;
    // After mrt_scene_deform_mesh on an uploaded scene the nodes and leaves of these BLASes
    // are behind the replica's (and with them the boxes of their instances: host_inst_stale).
    std::vector<int32_t> host_blas_stale;
    // After mrt_scene_update_texture on an uploaded scene the DomeTables of these domes (indices
    // into `domes`) are behind the replica's, which its kernels rebuilt (mrt_relight.hip), and
    // after the async form the texels of these textures too.
    std::vector<int32_t> host_dome_stale, host_tex_stale;
    bool host_stale() const {
        return host_bvh_stale || !host_mesh_stale.empty() || host_inst_stale || !host_blas_stale.empty() ||
               !host_dome_stale.empty() || !host_tex_stale.empty();
    }
    int upload_count = 0;   // upload_scene calls (mrt_scene_upload_count)

    // device replicas (one per HIP device used, mrt_render_opts.devices); `dev` is
    // the one the last call used.  dev_dirty: the host scene changed, every
    // replica is re-uploaded on its next use.
    std::vector<DeviceState*> devs;
    DeviceState* dev = nullptr;
    bool dev_dirty = true;
    mrt_stats last{};
    // the last call was a multi-device mrt_render: `last` already holds the summed
    // counters of its shares (last_rc: MRT_ERR_OVERFLOW if a share overflowed)
    bool stats_final = false;
    int last_rc = 0;
};

// host_build.cpp
int load_obj(const char* path, const float* ctm16, Mesh& out, std::string& err);
int build_qbvh(Scene& s, std::string& err);
int make_blas(Scene& s, const int32_t* meshes, int n_meshes, std::string& err);
int add_instance(Scene& s, int32_t blas, const float* m16, std::string& err);
// m, inv, inv_t and box of I from the row-major 4x4 m16 and the root of BLAS I.blas
// (add_instance's arithmetic; mrt_scene_update_instances uses it for a built scene)
void instance_set_matrix(const Scene& s, Instance& I, const float* m16);
// Its box half: ProxyObject::getAABB of BLAS root r under the row-major 4x4 m16 (min xyz, max xyz)
void instance_box(const QNode& r, const float* m16, float box[6]);
// The refit on the host: the world leaf triangles from the meshes' vertices (make_leaf),
// then every box bottom-up, topology kept (the arithmetic of mrt_refit.hip's kernels).
void refit_host(Scene& s);
// The same for BLAS b from its meshes' vertices, then Instance::box of every instance of b
// from the refitted root and the instance's m_transform (mrt_scene_deform_mesh).
void refit_blas_host(Scene& s, int32_t b);
// The box the build gave world object o when it is a ProxyObject or an MBObject lane
// (Builder::tri_aabb): min xyz, max xyz.  False for a plain triangle.
bool fixed_lane_box(const Scene& s, int32_t o, float box[6]);
// mrt_scene_rebuild_bvh on the host: a new topology for the world hierarchy from the lanes its
// packets hold now (mrt_rebuild.hip's kernels apply the same rule); every
// replica is re-uploaded on its next use.
void rebuild_host(Scene& s);
// mrt_scene_bvh_cost over the canonical arrays (the caller has run sync_host)
double bvh_cost_host(const Scene& s);
// mrt_refit.hip: bring a stale host copy up to date from the device (synchronises); a
// no-op when nothing is stale
// (meshes_only: the vertices and normals, and the instances, an async update left there, not
// the hierarchy)
int sync_host(Scene& s, bool meshes_only = false);
// host_api.cpp: the argument checks of mrt_scene_update_instances (m16s == nullptr: the async
// form, whose matrices are on the device; ids == nullptr: first .. first + n - 1).  out: the
// instances of the batch with their new matrices, inverses and boxes, nothing changed yet
int instances_check(const Scene& s, const int32_t* ids, int32_t first, int32_t n, const float* m16s,
                    std::vector<Instance>* out);
// host_api.cpp: the argument checks of mrt_scene_update_mesh (verts == nullptr: the async
// form, whose arrays are on the device), and the new arrays into the host mesh
int refit_check(const Scene& s, int mesh, const float* verts, const float* normals);
void refit_set_mesh(Mesh& m, const float* verts, const float* normals);
// host_api.cpp: the argument checks of mrt_scene_deform_mesh (verts == nullptr: the async form,
// which passes has_verts2 for its device pointer).  kind: kDeformWorld, kDeformBlas or kDeformMotion.
enum { kDeformWorld = 0, kDeformBlas = 1, kDeformMotion = 2 };
int deform_check(const Scene& s, int mesh, const float* verts, const float* verts2, bool has_verts2,
                 const float* normals, int* kind);
void deform_set_motion(Mesh& m, const float* verts2);
// host_api.cpp: the mrt_light -> DevLight conversion of mrt_scene_add_light (the rectangle light's
// setPower area scaling, the samples < 1 clamp, the point-light cast_shadows rule); dome: the
// light's DomeTables index (-1: not a dome light)
DevLight make_light(const mrt_light& l, int32_t dome);
// host_api.cpp: the mrt_material fields into d (what mrt_scene_add_material sets of them: kd, ka,
// ks, spec_exp, spec_amt, le, emitted and the derived emitter; a Lambert emits nothing)
void set_material_base(DevMaterial& d, const mrt_material& m);
// host_api.cpp: the argument checks of mrt_scene_update_lights / _material / _texture, each
// refusal with its own text and before any device call
int lights_check(const Scene& s, const mrt_light* lights, int32_t n);
int material_check(const Scene& s, int material, const mrt_material* m);
int texture_check(const Scene& s, int32_t texture, const float* data);
// the domes (indices into Scene::domes) that texture `texture` feeds
std::vector<int32_t> domes_of_texture(const Scene& s, int32_t texture);
// mrt_scene_update_texture on the host copy: new texels, build_dome for every dome the texture
// feeds; on a refusal the old texels are back and nothing changed
int update_texture_host(Scene& s, int32_t texture, const float* data);
// host_texture.cpp
// sin(theta) of row i's centre, i = 0 .. nv - 1: build_dome's weights (they depend on nv only)
void dome_sin_theta(int nv, std::vector<float>& out);
int load_hdr(const char* path, int& W, int& H, std::vector<float>* rgb, std::string& err);
int build_dome(const Texture& t, DomeTables& d, std::string& err);
// RawImage::loadImage (TGA / PPM / HDR by extension); data == nullptr: size + type only
int load_image(const char* path, int& W, int& H, int& type, std::vector<float>* data, std::string& err);
// TriangleMesh::preCalc's tangent frame (src/TriangleMesh.cpp:105-148)
void mesh_tangents(Mesh& m);

void set_error(const std::string& msg);

}  // namespace mrt

struct mrt_scene {
    mrt::Scene impl;
};
