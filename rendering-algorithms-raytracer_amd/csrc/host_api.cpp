// host_api.cpp -- the CPU-only part of libmrt's C-ABI: scene construction and
// queries, the image loaders, the numerics probes and the tuning table.  Plain C++:
// nothing here calls HIP (the entries that touch device state are in mrt_device.hip).
#include <math.h>
#include <string.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "mrt_device.h"
#include "mrt_scene.h"

namespace mrt {

static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }

Tuning g_tune;

// One row per tuning key: its field and the values mrt_set_tuning accepts.
struct TuneRow {
    const char* key;
    int Tuning::*field;
    enum Form { kFlag, kRange, kSet } form;   // any value, stored as 0 / 1 | v[0]..v[1] | one of v[0 .. n)
    int v[5];
    int n;
};
static const TuneRow kTuneRows[] = {
    {"fast_box", &Tuning::fast_box, TuneRow::kFlag, {}, 0},
    {"primary_waves", &Tuning::primary_waves, TuneRow::kSet, {0, 1, 6, 7, 8}, 5},
    {"scalar_nodes", &Tuning::scalar_nodes, TuneRow::kRange, {0, 7}, 2},   // bit 0 nodes, bit 1 triangles (1 = round 3's nodes only), bit 2 octant box test
    {"batch_tpw", &Tuning::batch_tpw, TuneRow::kRange, {1, 64}, 2},
    {"wave_log", &Tuning::wave_log, TuneRow::kFlag, {}, 0},
    {"shade1", &Tuning::shade1, TuneRow::kFlag, {}, 0},
    {"wavefront", &Tuning::wavefront, TuneRow::kFlag, {}, 0},
    {"chain", &Tuning::chain, TuneRow::kFlag, {}, 0},
    {"chain_mb", &Tuning::chain_mb, TuneRow::kRange, {1, 1 << 20}, 2},
    {"shadow_sched", &Tuning::shadow_sched, TuneRow::kRange, {-1, 2}, 2},
    {"primary_inst_waves", &Tuning::primary_inst_waves, TuneRow::kSet, {1, 4, 5, 6}, 4},
    {"adapt_refill", &Tuning::adapt_refill, TuneRow::kRange, {0, 64}, 2},
    {"chain_shadow_step", &Tuning::chain_shadow_step, TuneRow::kFlag, {}, 0},
    {"near_first", &Tuning::near_first, TuneRow::kRange, {-1, 1}, 2},
    {"fused", &Tuning::fused, TuneRow::kFlag, {}, 0},
    {"chain_est", &Tuning::chain_est, TuneRow::kFlag, {}, 0},
    {"chain_est_pct", &Tuning::chain_est_pct, TuneRow::kRange, {1, 100000}, 2},
    {"chain_shadow_refill", &Tuning::chain_shadow_refill, TuneRow::kFlag, {}, 0},
    {"bin_inst", &Tuning::bin_inst, TuneRow::kRange, {0, 2}, 2},
    {"chain_bands", &Tuning::chain_bands, TuneRow::kRange, {-1, 1}, 2},
    {"dome_replay", &Tuning::dome_replay, TuneRow::kFlag, {}, 0},
    {"bin", &Tuning::bin, TuneRow::kRange, {-1, 7}, 2},   // -1: auto
    {"bin_dbits", &Tuning::bin_dbits, TuneRow::kRange, {0, 6}, 2},   // the pair is checked when a batch is binned (2 dbits + 3 obits = 1..12)
    {"bin_obits", &Tuning::bin_obits, TuneRow::kRange, {0, 4}, 2},
    {"walk_latch", &Tuning::walk_latch, TuneRow::kRange, {0, 1}, 2},
    {"walk_exit", &Tuning::walk_exit, TuneRow::kRange, {0, 1}, 2},
    {"lds_nodes", &Tuning::lds_nodes, TuneRow::kRange, {0, 1}, 2},
    {"frame1_waves", &Tuning::frame1_waves, TuneRow::kSet, {1, 5, 6, 7, 8}, 5},
    {"sched", &Tuning::sched, TuneRow::kRange, {0, 3}, 2},
};

static const TuneRow* tune_row(const char* key) {
    if (!key) { set_error("null key"); return nullptr; }
    for (const TuneRow& r : kTuneRows)
        if (strcmp(r.key, key) == 0) return &r;
    set_error(std::string("unknown tuning key ") + key);
    return nullptr;
}

// What refit_check and deform_check share, `name` being the entry's in its messages: a built
// scene and a mesh of it before the entry's own refusals ...
static int mesh_check(const Scene& S, int mesh, const std::string& name) {
    if (!S.built) { set_error(name + ": scene not built"); return MRT_ERR_NOT_BUILT; }
    if (mesh < 0 || mesh >= (int)S.meshes.size()) { set_error(name + ": bad mesh id"); return MRT_ERR_INVALID; }
    return MRT_OK;
}
// ... and after them a hierarchy of the build and finite arrays (verts == nullptr: the async
// forms, whose arrays are on the device)
static int arrays_check(const Scene& S, const Mesh& m, const std::string& name, const float* verts, const float* verts2,
                        const float* normals) {
    if (S.imported) {
        set_error(name + ": the hierarchy was imported (mrt_scene_bvh_import) and need not be a tree: rebuild it");
        return MRT_ERR_INVALID;
    }
    auto finite = [&](const float* p, size_t n, const char* what) {
        for (size_t i = 0; i < 3 * n; i++)
            if (!std::isfinite(p[i])) {
                set_error(name + ": " + what + " " + std::to_string(i / 3) + " is not finite");
                return false;
            }
        return true;
    };
    if (verts && !finite(verts, m.verts.size(), "vertex")) return MRT_ERR_INVALID;
    if (verts && verts2 && !finite(verts2, m.verts.size(), "motion vertex")) return MRT_ERR_INVALID;
    if (verts && normals && !finite(normals, m.normals.size(), "normal")) return MRT_ERR_INVALID;
    return MRT_OK;
}

// mrt_scene_update_mesh / _async (mrt_refit.hip): which scenes and meshes a refit takes
int refit_check(const Scene& S, int mesh, const float* verts, const float* normals) {
    if (const int rc = mesh_check(S, mesh, "update_mesh")) return rc;
    const Mesh& m = S.meshes[(size_t)mesh];
    if (S.mesh_blas[(size_t)mesh] >= 0) {
        set_error("update_mesh: the mesh belongs to a BLAS (an instanced mesh is not refitted: its instance boxes would move)");
        return MRT_ERR_INVALID;
    }
    if (!m.verts2.empty()) {
        set_error("update_mesh: the mesh has motion vertices (mrt_scene_set_mesh_motion): an MBObject's box needs both sets");
        return MRT_ERR_INVALID;
    }
    return arrays_check(S, m, "update_mesh", verts, nullptr, normals);
}

void refit_set_mesh(Mesh& m, const float* verts, const float* normals) {
    for (size_t i = 0; i < m.verts.size(); i++) m.verts[i] = mk(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2]);
    if (normals)
        for (size_t i = 0; i < m.normals.size(); i++) m.normals[i] = mk(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
    mesh_tangents(m);   // TriangleMesh::preCalc of a texture-mapped mesh
}

// mrt_scene_deform_mesh / _async (mrt_refit.hip): which scenes, meshes and arrays it takes
int deform_check(const Scene& S, int mesh, const float* verts, const float* verts2, bool has_verts2, const float* normals,
                 int* kind) {
    if (const int rc = mesh_check(S, mesh, "deform_mesh")) return rc;
    const Mesh& m = S.meshes[(size_t)mesh];
    const bool in_blas = S.mesh_blas[(size_t)mesh] >= 0;
    if (in_blas && has_verts2) {
        set_error("deform_mesh: motion vertices given for a mesh of a BLAS (a BLAS mesh's motion vertices are inert: only world meshes make MBObjects)");
        return MRT_ERR_INVALID;
    }
    if (!in_blas && m.verts2.empty() && has_verts2) {
        set_error("deform_mesh: motion vertices given for a mesh without them (mrt_scene_set_mesh_motion)");
        return MRT_ERR_INVALID;
    }
    if (!in_blas && !m.verts2.empty() && !has_verts2) {
        set_error("deform_mesh: the mesh has motion vertices (mrt_scene_set_mesh_motion): give both sets, an MBObject's box needs them");
        return MRT_ERR_INVALID;
    }
    if (const int rc = arrays_check(S, m, "deform_mesh", verts, verts2, normals)) return rc;
    *kind = in_blas ? kDeformBlas : has_verts2 ? kDeformMotion : kDeformWorld;
    return MRT_OK;
}

void deform_set_motion(Mesh& m, const float* verts2) {
    for (size_t i = 0; i < m.verts2.size(); i++) m.verts2[i] = mk(verts2[3 * i], verts2[3 * i + 1], verts2[3 * i + 2]);
}

// mrt_scene_update_instances / _async (mrt_refit.hip): which scenes, ids and matrices it takes
int instances_check(const Scene& S, const int32_t* ids, int32_t first, int32_t n, const float* m16s,
                    std::vector<Instance>* out) {
    if (!S.built) { set_error("update_instances: scene not built"); return MRT_ERR_NOT_BUILT; }
    if (S.imported) {
        set_error("update_instances: the hierarchy was imported (mrt_scene_bvh_import) and need not be a tree: rebuild it");
        return MRT_ERR_INVALID;
    }
    const int64_t ni = (int64_t)S.instances.size();
    if (n < 0) { set_error("update_instances: negative count"); return MRT_ERR_INVALID; }
    if (!ids && (first < 0 || (int64_t)first + n > ni)) {
        set_error("update_instances: instance id " + std::to_string(first < 0 ? (int64_t)first : ni) + " out of range (the scene has " +
                  std::to_string(ni) + " instances)");
        return MRT_ERR_INVALID;
    }
    std::vector<char> seen(ids ? (size_t)ni : 0, 0);
    for (int32_t k = 0; ids && k < n; k++) {
        if (ids[k] < 0 || ids[k] >= ni) {
            set_error("update_instances: instance id " + std::to_string(ids[k]) + " out of range (the scene has " + std::to_string(ni) +
                      " instances)");
            return MRT_ERR_INVALID;
        }
        if (seen[(size_t)ids[k]]++) {
            set_error("update_instances: instance id " + std::to_string(ids[k]) + " repeated in the batch");
            return MRT_ERR_INVALID;
        }
    }
    if (!m16s) return MRT_OK;
    if (out) out->clear();
    for (int32_t k = 0; k < n; k++) {
        const float* m = m16s + 16 * (size_t)k;
        const int32_t id = ids ? ids[k] : first + k;
        const std::string which = "update_instances: matrix " + std::to_string(k) + " (instance " + std::to_string(id) + ")";
        for (int j = 0; j < 16; j++)
            if (!std::isfinite(m[j])) { set_error(which + " has an entry that is not finite"); return MRT_ERR_INVALID; }
        Instance I = S.instances[(size_t)id];
        instance_set_matrix(S, I, m);
        bool ok = true;
        for (int j = 0; j < 16; j++) ok = ok && std::isfinite(I.inv[j]);
        for (int j = 0; j < 6; j++) ok = ok && std::isfinite(I.box[j]);
        if (!ok) { set_error(which + " is singular or nearly so: its inverse or box is not finite"); return MRT_ERR_INVALID; }
        if (out) out->push_back(I);
    }
    return MRT_OK;
}

// mrt_scene_add_light / mrt_scene_update_lights: Light as the kernels read it.
// Light::setFastShadows(false): a point light's "full method" (src/PointLight.cpp:49-70)
// sets sampleHit.t = distance and then loops while sampleHit.t < distance: it never
// traces, so the light casts no shadow -- exactly cast_shadows = 0.  The rectangle and
// dome lights walk through refractive hits (src/RectangleLight.cpp:93-116,
// src/DomeLight.cpp:123-145; Shader::transmit).
DevLight make_light(const mrt_light& l, int32_t dome) {
    DevLight d;
    memset(&d, 0, sizeof d);
    d.dome = dome;
    d.type = l.type;
    memcpy(d.pos, l.pos, 12); memcpy(d.v1, l.v1, 12); memcpy(d.v2, l.v2, 12); memcpy(d.v3, l.v3, 12);
    d.samples = l.samples < 1 ? 1 : l.samples;
    d.noise = l.noise_threshold;
    d.cast_shadows = l.cast_shadows && !(l.transparent_shadows && l.type == MRT_POINT_LIGHT);
    d.transparent = l.transparent_shadows && l.type != MRT_POINT_LIGHT ? 1 : 0;
    d.power = l.power;
    if (l.type == MRT_RECT_LIGHT) {
        // RectangleLight::setPower (src/RectangleLight.cpp:14-40)
        const uint16_t* RS = host_rsqrt_table();
        v3 v1 = mk(l.v1[0], l.v1[1], l.v1[2]);
        v3 e0 = sub(mk(l.v2[0], l.v2[1], l.v2[2]), v1), e1 = sub(mk(l.v3[0], l.v3[1], l.v3[2]), v1);
        float recip = 1.0f, sq;
        if (fabsf(dot(e0, e1)) < 0.001f) sq = dot(e0, e0) * dot(e1, e1);
        else { v3 c = cross(e0, e1); sq = dot(c, c); }
        if (sq > 0.001f) recip = rsqrt_nr(sq, RS);
        d.power = l.power * recip;
    }
    return d;
}

void set_material_base(DevMaterial& d, const mrt_material& m) {
    memcpy(d.kd, m.kd, 12); memcpy(d.ka, m.ka, 12); memcpy(d.ks, m.ks, 12);
    d.spec_exp = m.spec_exp; d.spec_amt = m.spec_amt;
    memcpy(d.le, m.le, 12);
    d.emitted = m.emitted;
    d.emitter = (d.emitted > 0.0f || (d.le[0] + d.le[1]) + d.le[2] > 0.0f) ? 1 : 0;   // src/Blinn.cpp:47
    if (d.type != MRT_BLINN) { d.le[0] = d.le[1] = d.le[2] = 0.f; d.emitted = 0.f; d.emitter = 0; }
}

// mrt_scene_update_lights / _async (mrt_relight.hip): n lights that keep what shapes the replica
int lights_check(const Scene& S, const mrt_light* lights, int32_t n) {
    if (!lights) { set_error("update_lights: null lights"); return MRT_ERR_INVALID; }
    if (n < 0 || (size_t)n != S.lights.size()) {
        set_error("update_lights: " + std::to_string(n) + " lights given, the scene has " + std::to_string(S.lights.size()) +
                  " (the count is fixed: add lights with mrt_scene_add_light)");
        return MRT_ERR_INVALID;
    }
    for (int32_t i = 0; i < n; i++) {
        const mrt_light& a = S.light_args[(size_t)i];
        const mrt_light& b = lights[i];
        const char* field = nullptr;
        if (b.type != a.type) field = "type";
        else if (a.type == MRT_DOME_LIGHT && b.texture != a.texture) field = "texture";
        else if ((b.transparent_shadows != 0) != (a.transparent_shadows != 0)) field = "transparent_shadows";
        if (field) {
            set_error("update_lights: light " + std::to_string(i) + " changes its " + field +
                      " (it decides which kernels the scene runs: mrt_scene_add_light on a new scene)");
            return MRT_ERR_INVALID;
        }
    }
    return MRT_OK;
}

// mrt_scene_update_material / _async (mrt_relight.hip)
int material_check(const Scene& S, int material, const mrt_material* m) {
    if (!m) { set_error("update_material: null material"); return MRT_ERR_INVALID; }
    if (material < 0 || material >= (int)S.materials.size()) {
        set_error("update_material: bad material id " + std::to_string(material) + " (the scene has " +
                  std::to_string(S.materials.size()) + " materials)");
        return MRT_ERR_INVALID;
    }
    if (m->type != S.materials[(size_t)material].type) {
        set_error("update_material: material " + std::to_string(material) + " changes its type (Lambert / Blinn is fixed)");
        return MRT_ERR_INVALID;
    }
    return MRT_OK;
}

// mrt_scene_update_texture / _async (mrt_relight.hip)
int texture_check(const Scene& S, int32_t texture, const float* data) {
    if (!data) { set_error("update_texture: null texels"); return MRT_ERR_INVALID; }
    if (texture < 0 || texture >= (int32_t)S.textures.size()) {
        set_error("update_texture: bad texture id " + std::to_string(texture) + " (the scene has " +
                  std::to_string(S.textures.size()) + " textures)");
        return MRT_ERR_INVALID;
    }
    return MRT_OK;
}

std::vector<int32_t> domes_of_texture(const Scene& S, int32_t texture) {
    std::vector<int32_t> out;
    for (size_t i = 0; i < S.domes.size(); i++)
        if (S.domes[i].tex == texture) out.push_back((int32_t)i);
    return out;
}

int update_texture_host(Scene& S, int32_t texture, const float* data) {
    Texture& T = S.textures[(size_t)texture];
    std::vector<float> old(data, data + T.rgb.size());
    old.swap(T.rgb);
    const std::vector<int32_t> ids = domes_of_texture(S, texture);
    std::vector<DomeTables> built(ids.size());
    for (size_t k = 0; k < ids.size(); k++) {
        std::string err;
        const int rc = build_dome(T, built[k], err);
        if (rc) {
            old.swap(T.rgb);
            set_error("update_texture: " + err);
            return rc;
        }
        built[k].tex = texture;
    }
    for (size_t k = 0; k < ids.size(); k++) S.domes[(size_t)ids[k]] = std::move(built[k]);
    return MRT_OK;
}

}  // namespace mrt

using namespace mrt;

extern "C" {

const char* mrt_last_error(void) { return g_err.c_str(); }
int mrt_abi_version(void) { return MRT_ABI_VERSION; }

mrt_scene* mrt_scene_create(void) { return new (std::nothrow) mrt_scene(); }

int mrt_scene_add_material(mrt_scene* s, const mrt_material* m) {
    if (!s || !m || (m->type != MRT_LAMBERT && m->type != MRT_BLINN)) { set_error("bad material"); return MRT_ERR_INVALID; }
    if (s->impl.materials.size() >= (size_t)kMaxMaterials) { set_error("too many materials"); return MRT_ERR_INVALID; }
    DevMaterial d;
    d.type = m->type;
    set_material_base(d, *m);
    d.reflect = 0.f; d.refract = 0.f; d.ior = 1.5f; d.gloss = 1.f;   // Blinn defaults (src/Blinn.h:11-22)
    d.disperse = 0; d.ior3[0] = d.ior3[1] = d.ior3[2] = 1.5f;
    d.translucency = 0.f;
    d.sample_env = 1;                                                 // Material::Material, src/Material.cpp:6
    d.env = -1;                                                       // m_envMap NULL, m_envExposure 1 (:4)
    d.env_exposure = 1.f;
    for (int k = 0; k < 6; k++) d.maps[k] = -1;                       // no maps (src/Material.cpp:4-5)
    s->impl.materials.push_back(d);
    s->impl.dev_dirty = true;
    return (int)s->impl.materials.size() - 1;
}

int mrt_scene_add_light(mrt_scene* s, const mrt_light* l) {
    if (!s || !l || (l->type != MRT_POINT_LIGHT && l->type != MRT_RECT_LIGHT && l->type != MRT_DOME_LIGHT)) {
        set_error("bad light");
        return MRT_ERR_INVALID;
    }
    if (s->impl.lights.size() >= (size_t)kMaxLights) { set_error("too many lights"); return MRT_ERR_INVALID; }
    int32_t dome = -1;
    if (l->type == MRT_DOME_LIGHT) {
        // DomeLight::setTexture (src/DomeLight.cpp:8-78): tables built now, on the host
        if (l->texture < 0 || l->texture >= (int32_t)s->impl.textures.size() ||
            tex_channels(s->impl.textures[l->texture].type) != 3) {
            set_error("dome light needs an RGB / HDR texture id from mrt_scene_add_texture");
            return MRT_ERR_INVALID;
        }
        if (const int rc = sync_host(s->impl)) return rc;   // the texels an async texture update left on the device
        DomeTables t;
        std::string err;
        const int rc = build_dome(s->impl.textures[l->texture], t, err);
        if (rc) { set_error(err); return rc; }
        t.tex = l->texture;
        dome = (int32_t)s->impl.domes.size();
        s->impl.domes.push_back(std::move(t));
    }
    s->impl.lights.push_back(make_light(*l, dome));
    s->impl.light_args.push_back(*l);
    s->impl.dev_dirty = true;
    return (int)s->impl.lights.size() - 1;
}

int mrt_scene_make_blas(mrt_scene* s, const int32_t* meshes, int32_t n_meshes) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    std::string err;
    const int rc = make_blas(s->impl, meshes, n_meshes, err);
    if (rc < 0) set_error(err);
    return rc;
}

int mrt_scene_add_instance(mrt_scene* s, int32_t blas, const float* m16) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    if (const int rc = sync_host(s->impl)) return rc;   // the box comes from the BLAS root: a device deform may be ahead
    std::string err;
    const int rc = add_instance(s->impl, blas, m16, err);
    if (rc < 0) set_error(err);
    return rc;
}

int mrt_scene_blas_info(const mrt_scene* s, int32_t blas, int32_t* nodes, int32_t* leaves, int32_t* prims) {
    if (!s || !nodes || !leaves || !prims || blas < 0 || blas >= (int32_t)s->impl.blas.size()) {
        set_error("bad BLAS id / argument");
        return MRT_ERR_INVALID;
    }
    const Blas& B = s->impl.blas[blas];
    *nodes = (int32_t)B.nodes.size();
    *leaves = (int32_t)B.leaves.size();
    *prims = (int32_t)B.obj_mesh.size();
    return MRT_OK;
}

int mrt_scene_blas_export(const mrt_scene* s, int32_t blas, float* node_boxes, int32_t* node_child, float* leaf_tris,
                          int32_t* leaf_prims) {
    if (!s || !node_boxes || !node_child || !leaf_tris || !leaf_prims || blas < 0 ||
        blas >= (int32_t)s->impl.blas.size()) {
        set_error("bad BLAS id / argument");
        return MRT_ERR_INVALID;
    }
    // after a device deform of one of its meshes: the arrays the device holds, read back
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    const Blas& B = s->impl.blas[blas];
    for (size_t i = 0; i < B.nodes.size(); i++) {
        memcpy(node_boxes + 24 * i, B.nodes[i].box, 24 * sizeof(float));
        memcpy(node_child + 4 * i, B.nodes[i].child, 4 * sizeof(int32_t));
    }
    for (size_t i = 0; i < B.leaves.size(); i++) {
        memcpy(leaf_tris + 36 * i, B.leaves[i].t, 36 * sizeof(float));
        memcpy(leaf_prims + 4 * i, B.leaves[i].prim, 4 * sizeof(int32_t));
    }
    return MRT_OK;
}

int mrt_hdr_info(const char* path, int32_t* width, int32_t* height) {
    if (!path || !width || !height) { set_error("bad argument"); return MRT_ERR_INVALID; }
    int W = 0, H = 0;
    std::string err;
    const int rc = load_hdr(path, W, H, nullptr, err);
    if (rc) { set_error(err); return rc; }
    *width = W;
    *height = H;
    return MRT_OK;
}

int mrt_hdr_load(const char* path, float* rgb, int32_t width, int32_t height) {
    if (!path || !rgb) { set_error("bad argument"); return MRT_ERR_INVALID; }
    int W = 0, H = 0;
    std::string err;
    std::vector<float> buf;
    const int rc = load_hdr(path, W, H, &buf, err);
    if (rc) { set_error(err); return rc; }
    if (W != width || H != height) { set_error("HDR size differs from width x height (see mrt_hdr_info)"); return MRT_ERR_INVALID; }
    memcpy(rgb, buf.data(), buf.size() * sizeof(float));
    return MRT_OK;
}

int mrt_image_info(const char* path, int32_t* width, int32_t* height, int32_t* type) {
    if (!path || !width || !height || !type) { set_error("bad argument"); return MRT_ERR_INVALID; }
    int W = 0, H = 0, T = 0;
    std::string err;
    const int rc = load_image(path, W, H, T, nullptr, err);
    if (rc) { set_error(err); return rc; }
    *width = W;
    *height = H;
    *type = T;
    return MRT_OK;
}

int mrt_image_load(const char* path, float* data, int32_t width, int32_t height) {
    if (!path || !data) { set_error("bad argument"); return MRT_ERR_INVALID; }
    int W = 0, H = 0, T = 0;
    std::string err;
    std::vector<float> buf;
    const int rc = load_image(path, W, H, T, &buf, err);
    if (rc) { set_error(err); return rc; }
    if (W != width || H != height) { set_error("image size differs from width x height (see mrt_image_info)"); return MRT_ERR_INVALID; }
    memcpy(data, buf.data(), buf.size() * sizeof(float));
    return MRT_OK;
}

int mrt_scene_add_texture_typed(mrt_scene* s, const float* data, int32_t width, int32_t height, int32_t type) {
    if (!s || !data || width <= 0 || height <= 0 || (int64_t)width * height > (int64_t(1) << 28) ||
        (type != kTexHDR && type != kTexGray && type != kTexRGB && type != kTexRGBA)) {
        set_error("bad texture");
        return MRT_ERR_INVALID;
    }
    if (s->impl.textures.size() >= (size_t)kMaxTextures) { set_error("too many textures"); return MRT_ERR_INVALID; }
    Texture t;
    t.W = width;
    t.H = height;
    t.type = type;
    t.rgb.assign(data, data + (size_t)width * height * tex_channels(type));
    s->impl.textures.push_back(std::move(t));
    s->impl.dev_dirty = true;
    return (int)s->impl.textures.size() - 1;
}

int mrt_scene_set_material_maps(mrt_scene* s, int material, const int32_t maps[6]) {
    if (!s || !maps || material < 0 || material >= (int)s->impl.materials.size()) { set_error("bad material"); return MRT_ERR_INVALID; }
    for (int k = 0; k < 6; k++)
        if (maps[k] < -1 || maps[k] >= (int32_t)s->impl.textures.size()) { set_error("bad texture id"); return MRT_ERR_INVALID; }
    for (int k = 0; k < 6; k++) s->impl.materials[material].maps[k] = maps[k];
    s->impl.built = false;   // alpha maps change which leaf packets need the alpha test
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_add_texture(mrt_scene* s, const float* rgb, int32_t width, int32_t height) {
    if (!s || !rgb || width <= 0 || height <= 0 || (int64_t)width * height > (int64_t(1) << 28)) {
        set_error("bad texture");
        return MRT_ERR_INVALID;
    }
    if (s->impl.textures.size() >= (size_t)kMaxTextures) { set_error("too many textures"); return MRT_ERR_INVALID; }
    Texture t;
    t.W = width;
    t.H = height;
    t.rgb.assign(rgb, rgb + (size_t)width * height * 3);
    s->impl.textures.push_back(std::move(t));
    s->impl.dev_dirty = true;
    return (int)s->impl.textures.size() - 1;
}

int mrt_scene_set_material_env_map(mrt_scene* s, int material, int32_t texture, float exposure) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size()) { set_error("bad material id"); return MRT_ERR_INVALID; }
    if (texture < -1 || texture >= (int32_t)s->impl.textures.size() ||
        (texture >= 0 && tex_channels(s->impl.textures[texture].type) != 3)) {
        set_error("bad texture id (an environment map needs an RGB / HDR texture)");
        return MRT_ERR_INVALID;
    }
    DevMaterial& m = s->impl.materials[(size_t)material];
    m.env = texture;
    m.env_exposure = exposure;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_env_map(mrt_scene* s, int32_t texture, float exposure) {
    if (!s || texture < -1 || texture >= (int32_t)s->impl.textures.size() ||
        (texture >= 0 && tex_channels(s->impl.textures[texture].type) != 3)) {
        set_error("bad texture id (the environment map needs an RGB / HDR texture)");
        return MRT_ERR_INVALID;
    }
    s->impl.env_tex = texture;
    s->impl.env_exposure = exposure;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

static const DomeTables* dome_of(const mrt_scene* s, int32_t light) {
    if (!s || light < 0 || light >= (int32_t)s->impl.lights.size() || s->impl.lights[light].dome < 0) return nullptr;
    return &s->impl.domes[s->impl.lights[light].dome];
}

int mrt_scene_dome_info(const mrt_scene* s, int32_t light, int32_t* nu, int32_t* nv) {
    const DomeTables* t = dome_of(s, light);
    if (!t || !nu || !nv) { set_error("not a dome light"); return MRT_ERR_INVALID; }
    *nu = t->nu;
    *nv = t->nv;
    return MRT_OK;
}

int mrt_scene_dome_export(const mrt_scene* s, int32_t light, float* cdf_u, float* func_u, float* cdf_v,
                          float* func_v, float* func_int, float* cos_u, float* sin_u, float* cos_v, float* sin_v) {
    const DomeTables* t = dome_of(s, light);
    if (!t || !cdf_u || !func_u || !cdf_v || !func_v || !func_int || !cos_u || !sin_u || !cos_v || !sin_v) {
        set_error("not a dome light / bad argument");
        return MRT_ERR_INVALID;
    }
    // after a device texture update: the tables the device built, read back
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    auto put = [](const std::vector<float>& v, float* dst) { memcpy(dst, v.data(), v.size() * sizeof(float)); };
    put(t->cdf_u, cdf_u); put(t->func_u, func_u); put(t->cdf_v, cdf_v); put(t->func_v, func_v);
    put(t->int_v, func_int);
    func_int[t->nu] = t->int_u;
    put(t->cos_u, cos_u); put(t->sin_u, sin_u); put(t->cos_v, cos_v); put(t->sin_v, sin_v);
    return MRT_OK;
}

int mrt_scene_dome_export_derived(const mrt_scene* s, int32_t light, float* rad, int32_t* guide_u, int32_t* guide_v) {
    const DomeTables* t = dome_of(s, light);
    if (!t || !rad || !guide_u || !guide_v) { set_error("not a dome light / bad argument"); return MRT_ERR_INVALID; }
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    memcpy(rad, t->rad.data(), t->rad.size() * sizeof(float));
    memcpy(guide_u, t->guide_u.data(), t->guide_u.size() * sizeof(int32_t));
    memcpy(guide_v, t->guide_v.data(), t->guide_v.size() * sizeof(int32_t));
    return MRT_OK;
}

int mrt_scene_upload_count(const mrt_scene* s) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    return s->impl.upload_count;
}

int mrt_scene_add_obj(mrt_scene* s, const char* path, const float* ctm16, int material) {
    if (!s || !path) { set_error("bad argument"); return MRT_ERR_INVALID; }
    Mesh m;
    std::string err;
    int rc = load_obj(path, ctm16, m, err);
    if (rc != MRT_OK) { set_error(err); return rc; }
    m.material = material;
    s->impl.push_mesh(std::move(m));
    s->impl.built = false;
    return (int)s->impl.meshes.size() - 1;
}

int mrt_scene_add_mesh(mrt_scene* s, const mrt_mesh* mesh, int material) {
    if (!s || !mesh || mesh->nv < 0 || mesh->nn < 0 || mesh->nt < 0) { set_error("bad mesh"); return MRT_ERR_INVALID; }
    const int vs = mesh->vert_stride ? mesh->vert_stride : 3, ns = mesh->normal_stride ? mesh->normal_stride : 3;
    if (vs < 3 || ns < 3 || (mesh->nv && !mesh->verts) || (mesh->nn && !mesh->normals) ||
        (mesh->nt && (!mesh->vidx || !mesh->nidx))) {
        set_error("bad mesh: null array or stride < 3"); return MRT_ERR_INVALID;
    }
    Mesh m;
    m.material = material;
    for (int i = 0; i < mesh->nv; i++) {
        const float* v = mesh->verts + (size_t)vs * i;
        m.verts.push_back(mk(v[0], v[1], v[2]));
    }
    for (int i = 0; i < mesh->nn; i++) {
        const float* v = mesh->normals + (size_t)ns * i;
        m.normals.push_back(mk(v[0], v[1], v[2]));
    }
    m.vidx.assign(mesh->vidx, mesh->vidx + 3 * (size_t)mesh->nt);
    m.nidx.assign(mesh->nidx, mesh->nidx + 3 * (size_t)mesh->nt);
    for (size_t i = 0; i < m.vidx.size(); i++)
        if (m.vidx[i] >= (uint32_t)mesh->nv || m.nidx[i] >= (uint32_t)mesh->nn) { set_error("mesh index out of range"); return MRT_ERR_INVALID; }
    s->impl.push_mesh(std::move(m));
    s->impl.built = false;
    return (int)s->impl.meshes.size() - 1;
}

int mrt_scene_mesh_info(const mrt_scene* s, int mesh, int32_t* nv, int32_t* nn, int32_t* nt) {
    if (!s || mesh < 0 || mesh >= (int)s->impl.meshes.size()) { set_error("bad mesh id"); return MRT_ERR_INVALID; }
    const Mesh& m = s->impl.meshes[mesh];
    *nv = (int32_t)m.verts.size(); *nn = (int32_t)m.normals.size(); *nt = m.nt();
    return MRT_OK;
}

int mrt_scene_mesh_export(const mrt_scene* s, int mesh, float* verts, float* normals, uint32_t* vidx, uint32_t* nidx) {
    if (!s || mesh < 0 || mesh >= (int)s->impl.meshes.size()) { set_error("bad mesh id"); return MRT_ERR_INVALID; }
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;   // vertices an async update left on the device
    const Mesh& m = s->impl.meshes[mesh];
    for (size_t i = 0; i < m.verts.size(); i++) { verts[3*i] = m.verts[i].x; verts[3*i+1] = m.verts[i].y; verts[3*i+2] = m.verts[i].z; }
    for (size_t i = 0; i < m.normals.size(); i++) { normals[3*i] = m.normals[i].x; normals[3*i+1] = m.normals[i].y; normals[3*i+2] = m.normals[i].z; }
    memcpy(vidx, m.vidx.data(), m.vidx.size() * 4);
    memcpy(nidx, m.nidx.data(), m.nidx.size() * 4);
    return MRT_OK;
}

int mrt_scene_mesh_set_texcoords(mrt_scene* s, int mesh, const float* uv, int32_t n_texcoords, const uint32_t* tidx) {
    if (!s || mesh < 0 || mesh >= (int)s->impl.meshes.size() || !uv || !tidx || n_texcoords <= 0) {
        set_error("bad texcoords");
        return MRT_ERR_INVALID;
    }
    Mesh& m = s->impl.meshes[mesh];
    for (size_t i = 0; i < m.vidx.size(); i++)
        if (tidx[i] >= (uint32_t)n_texcoords) { set_error("texture-coordinate index out of range"); return MRT_ERR_INVALID; }
    m.uv.assign(uv, uv + 2 * (size_t)n_texcoords);
    m.tidx.assign(tidx, tidx + m.vidx.size());
    s->impl.built = false;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_mesh_motion(mrt_scene* s, int mesh, const float* verts2) {
    if (!s || mesh < 0 || mesh >= (int)s->impl.meshes.size() || !verts2) { set_error("bad mesh id"); return MRT_ERR_INVALID; }
    if (const int rc = sync_host(s->impl)) return rc;   // an async deform's vertex sets come back first, not over these
    Mesh& m = s->impl.meshes[mesh];
    m.verts2.resize(m.verts.size());
    for (size_t i = 0; i < m.verts.size(); i++) m.verts2[i] = v3{verts2[3*i], verts2[3*i+1], verts2[3*i+2]};
    s->impl.built = false;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_mesh_texcoords(const mrt_scene* s, int mesh, int32_t* n_texcoords, float* uv, uint32_t* tidx) {
    if (!s || mesh < 0 || mesh >= (int)s->impl.meshes.size() || !n_texcoords) { set_error("bad mesh id"); return MRT_ERR_INVALID; }
    const Mesh& m = s->impl.meshes[mesh];
    *n_texcoords = m.tidx.empty() ? 0 : (int32_t)(m.uv.size() / 2);
    if (*n_texcoords && uv) memcpy(uv, m.uv.data(), m.uv.size() * sizeof(float));
    if (*n_texcoords && tidx) memcpy(tidx, m.tidx.data(), m.tidx.size() * sizeof(uint32_t));
    return MRT_OK;
}

int mrt_scene_set_background(mrt_scene* s, const float rgb[3]) {
    if (!s || !rgb) { set_error("bad argument"); return MRT_ERR_INVALID; }
    memcpy(s->impl.bg, rgb, 12);
    return MRT_OK;
}

int mrt_scene_set_num_paths(mrt_scene* s, int num_paths) {
    if (!s || num_paths < 1 || num_paths > 1024) { set_error("bad num_paths (1..1024)"); return MRT_ERR_INVALID; }
    s->impl.num_paths = num_paths;
    return MRT_OK;
}

int mrt_scene_set_material_emission(mrt_scene* s, int material, float emitted, const float le[3]) {
    if (!s || !le || material < 0 || material >= (int)s->impl.materials.size()) {
        set_error("bad material / emission"); return MRT_ERR_INVALID;
    }
    DevMaterial& m = s->impl.materials[(size_t)material];
    if (m.type != MRT_BLINN) { set_error("only Blinn materials emit (src/Blinn.h:44-45)"); return MRT_ERR_INVALID; }
    memcpy(m.le, le, 12);
    m.emitted = emitted;
    m.emitter = (m.emitted > 0.0f || (m.le[0] + m.le[1]) + m.le[2] > 0.0f) ? 1 : 0;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_material_sample_env(mrt_scene* s, int material, int sample_env) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size()) { set_error("bad material"); return MRT_ERR_INVALID; }
    s->impl.materials[(size_t)material].sample_env = sample_env ? 1 : 0;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_path_trace(mrt_scene* s, int enable, int max_bounces, int sample_env) {
    if (!s || max_bounces < 1 || max_bounces > 64) { set_error("bad path trace settings (1 <= max_bounces <= 64)"); return MRT_ERR_INVALID; }
    s->impl.path_trace = enable != 0;
    s->impl.max_bounces = max_bounces;
    s->impl.sample_env = sample_env != 0;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_prim_object(const mrt_scene* s, int32_t prim, int32_t* mesh, int32_t* tri, int32_t* inst) {
    if (!s || !mesh || !tri || !inst) { set_error("bad argument"); return MRT_ERR_INVALID; }
    const Scene& S = s->impl;
    if (!S.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    if (prim < 0) { set_error("prim id out of range"); return MRT_ERR_INVALID; }
    if ((size_t)prim < S.obj_mesh.size()) {   // a world object (a ProxyObject's own slot never hits)
        *mesh = S.obj_mesh[prim]; *tri = S.obj_tri[prim]; *inst = S.obj_inst[prim];
        return MRT_OK;
    }
    int lo = 0, hi = (int)S.instances.size() - 1;   // the last instance with hit_base <= prim
    if (hi < 0) { set_error("prim id out of range"); return MRT_ERR_INVALID; }
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (S.instances[mid].hit_base <= prim) lo = mid; else hi = mid - 1;
    }
    const Blas& B = S.blas[S.instances[lo].blas];
    const int64_t k = (int64_t)prim - S.instances[lo].hit_base;
    if (k < 0 || k >= (int64_t)B.obj_mesh.size()) { set_error("prim id out of range"); return MRT_ERR_INVALID; }
    *mesh = B.obj_mesh[k]; *tri = B.obj_tri[k]; *inst = lo;
    return MRT_OK;
}

int mrt_scene_set_material_optics(mrt_scene* s, int material, float reflect_amt, float refract_amt, float ior) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size() || !(reflect_amt >= 0.f) ||
        !(refract_amt >= 0.f) || !(ior > 0.f)) {
        set_error("bad material optics: need a valid material, reflect / refract >= 0 and ior > 0");
        return MRT_ERR_INVALID;
    }
    DevMaterial& m = s->impl.materials[(size_t)material];
    m.reflect = reflect_amt;
    m.refract = refract_amt;
    m.ior = ior;
    m.ior3[1] = ior;   // one m_ior[3] in the reference: m_ior[1] is both the optics and the middle dispersion IOR
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_material_dispersion(mrt_scene* s, int material, int disperse, const float ior[3]) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size() || !ior || !(ior[0] > 0.f) ||
        !(ior[1] > 0.f) || !(ior[2] > 0.f)) {
        set_error("bad dispersion: need a valid material and three IORs > 0");
        return MRT_ERR_INVALID;
    }
    DevMaterial& m = s->impl.materials[(size_t)material];
    m.disperse = disperse ? 1 : 0;
    for (int i = 0; i < 3; i++) m.ior3[i] = ior[i];
    m.ior = ior[1];   // m_ior[1]: the IOR of the non-dispersive refraction
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_material_translucency(mrt_scene* s, int material, float translucency) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size() || !(translucency >= 0.f)) {
        set_error("bad translucency: need a valid material and translucency >= 0");
        return MRT_ERR_INVALID;
    }
    s->impl.materials[(size_t)material].translucency = translucency;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_material_gloss(mrt_scene* s, int material, float gloss) {
    if (!s || material < 0 || material >= (int)s->impl.materials.size() || !(gloss >= 0.f && gloss <= 1.f)) {
        set_error("bad gloss: need a valid material and 0 <= gloss <= 1");
        return MRT_ERR_INVALID;
    }
    s->impl.materials[(size_t)material].gloss = gloss;
    s->impl.dev_dirty = true;
    return MRT_OK;
}

int mrt_scene_set_subdivs(mrt_scene* s, int min_subdivs, int max_subdivs, float noise_threshold) {
    if (!s || min_subdivs < 1 || max_subdivs < min_subdivs || max_subdivs > 16 || !(noise_threshold >= 0.f)) {
        set_error("bad subdivs: need 1 <= min <= max <= 16 and noise >= 0");
        return MRT_ERR_INVALID;
    }
    s->impl.min_subdivs = min_subdivs;
    s->impl.max_subdivs = max_subdivs;
    s->impl.noise_threshold = noise_threshold;
    return MRT_OK;
}

int mrt_scene_build_bvh(mrt_scene* s) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    for (auto& m : s->impl.meshes)
        if (m.material < 0 || m.material >= (int)s->impl.materials.size()) { set_error("mesh references unknown material"); return MRT_ERR_INVALID; }
    if (const int rc = sync_host(s->impl)) return rc;   // the build reads the host vertices
    std::string err;
    int rc = build_qbvh(s->impl, err);
    if (rc != MRT_OK) set_error(err);
    return rc;
}

int mrt_scene_bvh_info(const mrt_scene* s, mrt_bvh_info* info) {
    if (!s || !info) { set_error("bad argument"); return MRT_ERR_INVALID; }
    if (!s->impl.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    // after an async rebuild: the node and packet counts the device holds, read back
    if (s->impl.host_topo_stale)
        if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    *info = s->impl.info;
    return MRT_OK;
}

int mrt_scene_bvh_cost(const mrt_scene* s, double* cost) {
    if (!s || !cost) { set_error("bad argument"); return MRT_ERR_INVALID; }
    if (!s->impl.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    // after a device refit or rebuild: the arrays the device holds, read back
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    *cost = bvh_cost_host(s->impl);
    return MRT_OK;
}

int mrt_scene_bvh_export(const mrt_scene* s, float* node_boxes, int32_t* node_child, float* leaf_tris, int32_t* leaf_prims) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    if (!s->impl.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    // after a device refit: the arrays the device holds, read back and converted
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl)) return rc;
    for (size_t i = 0; i < s->impl.nodes.size(); i++) {
        memcpy(node_boxes + 24 * i, s->impl.nodes[i].box, 96);
        memcpy(node_child + 4 * i, s->impl.nodes[i].child, 16);
    }
    for (size_t i = 0; i < s->impl.leaves.size(); i++) {
        memcpy(leaf_tris + 36 * i, s->impl.leaves[i].t, 144);
        memcpy(leaf_prims + 4 * i, s->impl.leaves[i].prim, 16);
    }
    return MRT_OK;
}

int mrt_scene_instance_count(const mrt_scene* s) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    return (int)s->impl.instances.size();
}

int mrt_scene_instance_info(const mrt_scene* s, int32_t inst, int32_t* blas, float m16[16], float inv16[16], float inv_t16[16],
                            float box6[6]) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    if (inst < 0 || (size_t)inst >= s->impl.instances.size()) { set_error("bad instance id"); return MRT_ERR_INVALID; }
    // after an async update: the matrices and the box the device holds, read back
    if (const int rc = sync_host(const_cast<mrt_scene*>(s)->impl, true)) return rc;
    const Instance& I = s->impl.instances[(size_t)inst];
    if (blas) *blas = I.blas;
    if (m16) memcpy(m16, I.m, sizeof I.m);
    if (inv16) memcpy(inv16, I.inv, sizeof I.inv);
    if (inv_t16) memcpy(inv_t16, I.inv_t, sizeof I.inv_t);
    if (box6) memcpy(box6, I.box, sizeof I.box);
    return MRT_OK;
}

int mrt_scene_bvh_import(mrt_scene* s, int32_t nodes, int32_t leaves, const float* node_boxes, const int32_t* node_child,
                         const float* leaf_tris, const int32_t* leaf_prims) {
    if (!s || nodes < 1 || leaves < 0) { set_error("bad argument"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (!S.built) { set_error("build the scene first (prim ids come from it)"); return MRT_ERR_NOT_BUILT; }
    if (const int rc = sync_host(S)) return rc;
    std::vector<QNode> N((size_t)nodes);
    std::vector<QLeaf> L((size_t)leaves);
    for (int i = 0; i < nodes; i++) {
        memset(&N[i], 0, sizeof(QNode));
        memcpy(N[i].box, node_boxes + 24 * (size_t)i, 96);
        memcpy(N[i].child, node_child + 4 * (size_t)i, 16);
        for (int k = 0; k < 4; k++) {
            int32_t c = N[i].child[k];
            if (c == kEmptySlot) continue;
            if ((c >= 0 && c >= nodes) || (c < 0 && ~c >= leaves)) { set_error("child index out of range"); return MRT_ERR_INVALID; }
        }
    }
    for (int i = 0; i < leaves; i++) {
        memcpy(L[i].t, leaf_tris + 36 * (size_t)i, 144);
        memcpy(L[i].prim, leaf_prims + 4 * (size_t)i, 16);
        for (int k = 0; k < 4; k++)
            if (L[i].prim[k] >= S.info.prims) { set_error("prim id out of range"); return MRT_ERR_INVALID; }
    }
    S.nodes.swap(N);
    S.leaves.swap(L);
    S.info.nodes = nodes;
    S.info.leaves = leaves;
    S.imported = true;
    S.dev_dirty = true;
    return MRT_OK;
}

int mrt_set_tuning(const char* key, int value) {
    const TuneRow* r = tune_row(key);
    if (!r) return MRT_ERR_INVALID;
    bool ok = r->form == TuneRow::kFlag || (r->form == TuneRow::kRange && value >= r->v[0] && value <= r->v[1]);
    for (int i = 0; r->form == TuneRow::kSet && i < r->n; i++) ok |= value == r->v[i];
    if (!ok) {
        std::string m = std::string(r->key) + " must be ";
        if (r->form == TuneRow::kRange) m += std::to_string(r->v[0]) + ".." + std::to_string(r->v[1]);
        for (int i = 0; r->form == TuneRow::kSet && i < r->n; i++)
            m += (i == 0 ? "one of " : i + 1 < r->n ? ", " : " or ") + std::to_string(r->v[i]);
        set_error(m);
        return MRT_ERR_INVALID;
    }
    g_tune.*r->field = r->form == TuneRow::kFlag ? (value ? 1 : 0) : value;
    return MRT_OK;
}

int mrt_get_tuning(const char* key, int* value) {
    const TuneRow* r = tune_row(key);
    if (!r) return MRT_ERR_INVALID;
    if (!value) { set_error("bad argument"); return MRT_ERR_INVALID; }
    *value = g_tune.*r->field;
    return MRT_OK;
}

int mrt_walk_arrays_fit(uint64_t n_nodes, uint64_t n_leaves) { return walk_arrays_fit(n_nodes, n_leaves) ? 1 : 0; }

float mrt_rcp_nr(float x) { return rcp_nr(x, host_rcp_table()); }
float mrt_rsqrt_nr(float x) { return rsqrt_nr(x, host_rsqrt_table()); }

}  // extern "C"
