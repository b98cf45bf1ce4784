// host_image.cpp -- build_image: a built Scene's device arrays and everything derived from
// them, on the host (plain C++, no HIP call).  It decides what every kernel reads;
// upload_scene (mrt_upload.hip) only copies it.
#include <string.h>

#include <algorithm>
#include <cmath>

#include "mrt_image.h"

namespace mrt {

// union of the root's used slot boxes (finite values only, per axis)
void root_box(const QNode& root, float lo3[3], float hi3[3]) {
    for (int a = 0; a < 3; a++) lo3[a] = hi3[a] = 0.f;
    bool any[3] = {false, false, false};
    for (int i = 0; i < 4; i++) {
        if (root.child[i] == kEmptySlot) continue;
        for (int a = 0; a < 3; a++) {
            const float lo = root.box[a * 4 + i], hi = root.box[12 + a * 4 + i];
            if (!std::isfinite(lo) || !std::isfinite(hi)) continue;
            lo3[a] = any[a] ? std::min(lo3[a], lo) : lo;
            hi3[a] = any[a] ? std::max(hi3[a], hi) : hi;
            any[a] = true;
        }
    }
}

namespace {

// world triangles the walks must check lane by lane: alpha-mapped materials, MBObject lanes
struct Special {
    const Scene& s;
    std::vector<char> alpha_mat;
    explicit Special(const Scene& sc) : s(sc), alpha_mat(sc.materials.size(), 0) {
        for (size_t m = 0; m < s.materials.size(); m++) alpha_mat[m] = s.materials[m].maps[kMapAlpha] >= 0;
    }
    bool world_mesh(int32_t p) const { return p >= 0 && (size_t)p < s.obj_mesh.size() && s.obj_mesh[p] >= 0; }
    bool alpha_obj(int32_t p) const { return world_mesh(p) && alpha_mat[(size_t)s.meshes[s.obj_mesh[p]].material]; }
    // MBObject world triangles (meshes with time-1 vertices)
    bool mb_obj(int32_t p) const {
        return world_mesh(p) && (s.obj_inst.empty() || s.obj_inst[(size_t)p] < 0) && !s.meshes[s.obj_mesh[p]].verts2.empty();
    }
};

// shading arrays: the meshes concatenated; texture coordinates of texture-mapped meshes
// ((u, v) pairs, per-normal tangent frames: TriangleMesh::preCalc, host_texture.cpp);
// PrimShade and uv records of the world objects (a ProxyObject's own slot stays zero), then
// of each BLAS's objects
void shading_records(const Scene& s, DeviceImage& g) {
    const size_t nm = s.meshes.size();
    g.vbase.resize(nm);
    g.nbase.resize(nm);
    for (size_t m = 0; m < nm; m++) {
        g.vbase[m] = (uint32_t)g.V.size();
        g.nbase[m] = (uint32_t)g.N.size();
        for (auto& p : s.meshes[m].verts) g.V.push_back(F4{p.x, p.y, p.z, 1.f});
        for (auto& p : s.meshes[m].normals) g.N.push_back(F4{p.x, p.y, p.z, 0.f});
    }
    g.any_uv = false;
    for (const Mesh& m : s.meshes) g.any_uv |= !m.tidx.empty();
    std::vector<uint32_t> ubase(nm, 0);
    if (g.any_uv) {
        g.TN.assign(g.N.size(), F4{0.f, 0.f, 0.f, 0.f});
        g.BTN.assign(g.N.size(), F4{0.f, 0.f, 0.f, 0.f});
        for (size_t m = 0; m < nm; m++) {
            const Mesh& M = s.meshes[m];
            ubase[m] = (uint32_t)g.UV.size();
            if (M.tidx.empty()) continue;
            for (size_t i = 0; i + 1 < M.uv.size(); i += 2) g.UV.push_back(F2{M.uv[i], M.uv[i + 1]});
            for (size_t i = 0; i < M.tan.size(); i++) {
                g.TN[g.nbase[m] + i] = F4{M.tan[i].x, M.tan[i].y, M.tan[i].z, 0.f};
                g.BTN[g.nbase[m] + i] = F4{M.btan[i].x, M.btan[i].y, M.btan[i].z, 0.f};
            }
        }
    }
    auto records = [&](const std::vector<int32_t>& obj_mesh, const std::vector<int32_t>& obj_tri) {
        for (size_t i = 0; i < obj_mesh.size(); i++) {
            const int32_t mesh = obj_mesh[i];
            const size_t t = (size_t)obj_tri[i];
            PrimShade p{};
            U4 u{0u, 0u, 0u, 0u};
            if (mesh < 0) {   // a ProxyObject's own world slot: never a hit (hit_record_usable refuses it by this mark)
                p.pad = 1u;
            } else {
                const Mesh& m = s.meshes[mesh];
                for (int k = 0; k < 3; k++) {
                    p.v[k] = g.vbase[mesh] + m.vidx[3 * t + k];
                    p.n[k] = g.nbase[mesh] + m.nidx[3 * t + k];
                }
                p.mat = (uint32_t)m.material;
                if (!m.tidx.empty()) u = U4{ubase[mesh] + m.tidx[3 * t], ubase[mesh] + m.tidx[3 * t + 1], ubase[mesh] + m.tidx[3 * t + 2], 1u};
            }
            g.PS.push_back(p);
            if (g.any_uv) g.PUV.push_back(u);
        }
    };
    records(s.obj_mesh, s.obj_tri);
    g.blas.assign(s.blas.size(), ImageInfo::BlasRange());
    for (size_t b = 0; b < s.blas.size(); b++) {
        g.blas[b].tree.shade_base = (int32_t)g.PS.size();
        records(s.blas[b].obj_mesh, s.blas[b].obj_tri);
    }
}

// One hierarchy appended to DN / DL, indices offset; returns its root.  Leaf slots carry
// their packet's object count, a ProxyObject bit and a check bit (leaf_child); a ProxyObject
// lane's prim is -2 - instance.  The world passes its obj_inst, a BLAS itself.
int32_t append(const Special& sp, DeviceImage& g, const std::vector<QNode>& nodes, const std::vector<QLeaf>& leaves,
               const std::vector<int32_t>* oi, const Blas* B) {
    const Scene& s = sp.s;
    const int32_t nb = (int32_t)g.DN.size(), lb = (int32_t)g.DL.size();
    auto proxy_of = [&](int32_t p) { return (oi && p >= 0 && (size_t)p < oi->size()) ? (*oi)[p] : -1; };
    for (QNode q : nodes) {
        for (int k = 0; k < 4; k++) {
            const int32_t c = q.child[k];
            if (c == kEmptySlot) continue;
            if (c >= 0) { q.child[k] = c + nb; continue; }
            const QLeaf& L = leaves[(size_t)~c];
            int cnt = 0;
            bool proxy = false, alpha = false;
            for (int j = 0; j < 4; j++)
                if (L.prim[j] >= 0) {  // zero-filled lanes below cnt are rejected by det = 0
                    cnt = j + 1;
                    proxy |= proxy_of(L.prim[j]) >= 0;
                    alpha |= oi != nullptr && proxy_of(L.prim[j]) < 0 &&
                             (sp.alpha_obj(L.prim[j]) || sp.mb_obj(L.prim[j]));   // world: alpha / motion blur
                    alpha |= B != nullptr && (size_t)L.prim[j] < B->obj_mesh.size() &&
                             sp.alpha_mat[(size_t)s.meshes[B->obj_mesh[(size_t)L.prim[j]]].material];   // BLAS: alpha
                }
            g.has_alpha |= alpha;
            q.child[k] = leaf_child((uint32_t)(~c + lb), cnt < 1 ? 1 : cnt, proxy, alpha);
        }
        g.DN.push_back(q);
    }
    for (const QLeaf& L : leaves) {
        DLeaf D{};
        for (int k = 0; k < 4; k++) {
            for (int c = 0; c < 9; c++) D.tri[k][c] = L.t[4 * c + k];
            const int32_t pi = proxy_of(L.prim[k]);
            D.prim[k] = pi >= 0 ? -2 - pi : L.prim[k];
        }
        g.DL.push_back(D);
    }
    return nb;
}

// The world hierarchy's first kLdsNodes nodes in breadth-first order get device numbers
// 0 .. kLdsNodes - 1 (frame1_kernel<LN> stages them in LDS).  Device node numbers are
// internal: the visit order follows the child slots, not the numbers.  BLAS nodes keep theirs.
void lds_renumber(DeviceImage& g, size_t nw) {
    std::vector<QNode>& DN = g.DN;
    g.lds_ok = nw >= (size_t)kLdsNodes;
    if (!g.lds_ok) return;
    // (an imported hierarchy may share a node between parents: each is numbered once)
    std::vector<int32_t> bfs{0};
    std::vector<int32_t> perm(DN.size(), -1);
    perm[0] = 0;
    for (size_t q = 0; q < bfs.size() && bfs.size() < (size_t)kLdsNodes; q++)
        for (int k = 0; k < 4 && bfs.size() < (size_t)kLdsNodes; k++) {
            const int32_t ch = DN[(size_t)bfs[q]].child[k];
            if (ch >= 0 && (size_t)ch < nw && perm[(size_t)ch] < 0) {
                perm[(size_t)ch] = (int32_t)bfs.size();
                bfs.push_back(ch);
            }
        }
    g.lds_ok = bfs.size() == (size_t)kLdsNodes;
    int32_t next = (int32_t)bfs.size();
    for (size_t i = 0; i < nw; i++)
        if (perm[i] < 0) perm[i] = next++;
    for (size_t i = nw; i < DN.size(); i++) perm[i] = (int32_t)i;
    std::vector<QNode> R(DN.size());
    for (size_t i = 0; i < DN.size(); i++) {
        QNode q = DN[i];
        for (int k = 0; k < 4; k++)
            if (q.child[k] >= 0) q.child[k] = perm[(size_t)q.child[k]];
        R[(size_t)perm[i]] = q;
    }
    DN.swap(R);
    for (ImageInfo::BlasRange& b : g.blas) b.tree.node_base = (uint32_t)perm[b.tree.node_base];
    g.node_perm.assign(perm.begin(), perm.begin() + (ptrdiff_t)nw);
}

// DevInstance records and the instance-major ray-bin keys (mrt_bin.h): hit bases, instances
// ranked by BLAS then index, and object-space cells: each instance's BLAS root box (its
// finite child boxes), 4 cells per axis
void instance_tables(const Scene& s, DeviceImage& g) {
    std::vector<DevInstance>& DI = g.DI;
    DI.resize(s.instances.size());
    for (size_t i = 0; i < DI.size(); i++) {
        const Instance& I = s.instances[i];
        memcpy(DI[i].inv, I.inv, sizeof DI[i].inv);
        memcpy(DI[i].inv_t, I.inv_t, sizeof DI[i].inv_t);  // rows 0-2
        DI[i].root = (int32_t)g.blas[(size_t)I.blas].tree.node_base;
        DI[i].hit_base = I.hit_base;
        DI[i].shade_base = g.blas[(size_t)I.blas].tree.shade_base;
        DI[i].pad = 0;
    }
    g.n_insts = (int)DI.size();
    g.hit_base.resize(DI.size());
    std::vector<uint32_t> order(DI.size());
    for (size_t i = 0; i < DI.size(); i++) { g.hit_base[i] = DI[i].hit_base; order[i] = (uint32_t)i; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return DI[a].root < DI[b].root; });
    g.cls.resize(DI.size());
    for (size_t r = 0; r < order.size(); r++) g.cls[order[r]] = (uint16_t)std::min<size_t>(127, r * 128 / order.size());
    g.cell.resize(2 * DI.size());
    for (size_t i = 0; i < DI.size(); i++) {
        float lo3[3], hi3[3];
        root_box(g.DN[(size_t)DI[i].root], lo3, hi3);
        auto sc = [&](int a) { return hi3[a] > lo3[a] ? 4.0f / (hi3[a] - lo3[a]) : 0.0f; };
        g.cell[2 * i] = F4{lo3[0], lo3[1], lo3[2], (float)(s.instances[i].blas & 1)};
        g.cell[2 * i + 1] = F4{sc(0), sc(1), sc(2), 0.f};
    }
}

// what the launches ask of a scene: its boxes, lights and materials
void scene_flags(const Scene& s, DeviceImage& g) {
    g.has_maps = false;
    for (const DevMaterial& m : s.materials) {
        const int32_t* mp = m.maps;
        g.has_maps |= mp[kMapColor] >= 0 || mp[kMapNormal] >= 0 || mp[kMapSpecular] >= 0 || mp[kMapReflect] >= 0 ||
                      mp[kMapRefract] >= 0;
    }
    g.special = g.n_insts > 0 || g.has_alpha || g.has_mb;
    g.boxes_finite = true;
    g.boxes_ordered = true;
    for (const QNode& q : g.DN) {
        for (int k = 0; k < 24; k++) g.boxes_finite &= std::isfinite(q.box[k]);
        for (int i = 0; i < 4; i++)
            if (q.child[i] != kEmptySlot)
                for (int a = 0; a < 3; a++) g.boxes_ordered &= q.box[a * 4 + i] <= q.box[12 + a * 4 + i];
    }
    if (!g.DN.empty()) root_box(g.DN[0], g.bb_lo, g.bb_hi);
    shading_flags(s, g);
}

}  // namespace

// what the launches ask of a scene's lights and materials (scene_flags at upload;
// mrt_scene_update_lights / _material on every replica's ImageInfo afterwards)
void shading_flags(const Scene& s, ImageInfo& g) {
    g.point_only = true;
    g.dome = false;
    // transparent shadows: the walk is compiled into the fused chain kernels only (it
    // needs a closest-hit traversal in the shading, which would cost the direct
    // kernels occupancy), and they shade a scene without secondary rays identically
    g.transparent = false;
    for (const DevLight& l : s.lights) {
        g.point_only &= (l.type == MRT_POINT_LIGHT);
        g.dome |= l.type == MRT_DOME_LIGHT;
        g.transparent |= l.transparent != 0;
    }
    g.recursive = 0;
    g.pow_spec = false;
    g.disperse = false;
    for (const DevMaterial& m : s.materials) {
        if (m.type != MRT_BLINN) continue;
        if (m.reflect > 0.f || m.refract > 0.f || m.gloss < 1.f || m.translucency > 0.01f) g.recursive = 1;
        g.pow_spec |= m.spec_exp != 1.0f;
        g.disperse |= m.disperse && (m.reflect > 0.f || m.refract > 0.f);
    }
    if (s.path_trace) g.recursive = 2;
    if (g.transparent && !g.recursive) g.recursive = 1;
}

namespace {

// mrt_scene_info.device_bytes: every array upload_scene copies (an empty one counts 0)
size_t image_bytes(const Scene& s, const DeviceImage& g) {
    auto sz = [](const auto&... v) { return (size_t(0) + ... + (v.size() * sizeof(v[0]))); };
    size_t n = sz(g.DN, g.DI, g.hit_base, g.cls, g.cell, g.DL, g.PS, g.V, g.N, s.materials, s.lights, g.tab, g.PUV, g.UV, g.TN,
                  g.BTN, g.V2, g.PF) +
               32769 * (1 + sizeof(float)) +   // the gamma tables
               s.domes.size() * sizeof(DevDome) + s.textures.size() * sizeof(DevTexture);
    for (const Texture& t : s.textures) n += sz(t.rgb);
    for (const DomeTables& t : s.domes)
        n += sz(t.cdf_u, t.func_u, t.cdf_v, t.func_v, t.inv_int_v, t.cos_u, t.sin_u, t.cos_v, t.sin_v, t.rad, t.guide_u, t.guide_v);
    return n;
}

}  // namespace

int build_image(const Scene& s, DeviceImage& g, std::string& err) {
    shading_records(s, g);
    const Special sp(s);
    g.PF.assign(s.obj_mesh.size(), 0);
    g.has_mb = false;
    for (size_t i = 0; i < g.PF.size(); i++)
        if (sp.mb_obj((int32_t)i)) { g.PF[i] = 1; g.has_mb = true; }
    g.tab.resize(4096);
    memcpy(g.tab.data(), host_rcp_table(), 4096);
    memcpy(g.tab.data() + 2048, host_rsqrt_table(), 4096);
    // device node / leaf arrays: the world hierarchy, then each BLAS
    size_t n_leaves = s.leaves.size();
    for (const Blas& B : s.blas) n_leaves += B.leaves.size();
    if (n_leaves >= (size_t(1) << 27)) { err = "too many leaf packets"; return MRT_ERR_OVERFLOW; }
    g.has_alpha = false;
    append(sp, g, s.nodes, s.leaves, &s.obj_inst, nullptr);
    for (size_t b = 0; b < s.blas.size(); b++) {
        RefitTree& T = g.blas[b].tree;
        T.leaf_base = (uint32_t)g.DL.size();
        T.node_base = (uint32_t)append(sp, g, s.blas[b].nodes, s.blas[b].leaves, nullptr, &s.blas[b]);
        T.n_nodes = (uint32_t)s.blas[b].nodes.size();
        T.n_leaves = (uint32_t)s.blas[b].leaves.size();
    }
    g.n_leaves_all = (uint32_t)g.DL.size();
    lds_renumber(g, s.nodes.size());
    g.world.n_nodes = (uint32_t)s.nodes.size();
    g.world.n_leaves = (uint32_t)s.leaves.size();
    g.world.fixed_lanes = true;
    for (QNode& q : g.DN) q.pad[0] = slot_kinds(q.child);   // the walks read the slot kinds (node_kinds)
    if (!walk_arrays_fit(g.DN.size(), g.DL.size())) {   // 32-bit byte offsets in the walks (node_at / tri_at)
        err = "scene too large: its node or leaf array passes 4 GiB";
        return MRT_ERR_OVERFLOW;
    }
    instance_tables(s, g);
    g.n_world = (int)s.obj_mesh.size();
    if (g.has_mb) {   // time-1 vertices parallel to V (copies of V for static meshes)
        g.V2 = g.V;
        for (size_t m = 0; m < s.meshes.size(); m++)
            for (size_t i = 0; i < s.meshes[m].verts2.size(); i++) {
                const v3& p = s.meshes[m].verts2[i];
                g.V2[g.vbase[m] + i] = F4{p.x, p.y, p.z, 1.f};
            }
    } else {
        g.PF.clear();   // copied for motion-blur scenes only
    }
    scene_flags(s, g);
    g.bytes = image_bytes(s, g);
    return MRT_OK;
}

}  // namespace mrt
