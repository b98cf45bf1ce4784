// mrt_upload.hip -- a scene's device replicas and their per-stream contexts: created,
// uploaded and freed here (HIP runtime calls only: this file holds no kernel).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "mrt_device.h"
#include "mrt_kernels.h"
#include "mrt_shader.h"

namespace mrt {

static void free_ctx(StreamCtx* c) {
    void* ptrs[] = {c->gstack, c->ctr, c->wave_log, c->hitbuf, c->rays, c->occl, c->nrays, c->lvl, c->chain,
                    c->adapt, c->bin_keys, c->bin_perm, c->bin_hist, c->ray_e, c->lrec};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (c->est_dev) (void)hipFree(c->est_dev);
    if (c->est_pinned) (void)hipHostFree(c->est_pinned);
    if (c->est_ev) (void)hipEventDestroy(c->est_ev);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->evm) (void)hipEventDestroy(c->evm);
    delete c;
}

static void free_device(DeviceState* d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();   // no launch may still use the scratch below
    for (StreamCtx* c : d->ctxs) free_ctx(c);
    for (hipStream_t st : d->share_streams) (void)hipStreamDestroy(st);
    if (d->gather_stream) (void)hipStreamDestroy(d->gather_stream);
    for (ShareBuf* b : d->share_bufs) {
        if (b->items) (void)hipFree(b->items);
        if (b->tiles) (void)hipFree(b->tiles);
        if (b->done) (void)hipEventDestroy(b->done);
        delete b;
    }
    if (d->g_tiles) (void)hipFree(d->g_tiles);
    if (d->g_items) (void)hipFree(d->g_items);
    if (d->refit_stage) (void)hipFree(d->refit_stage);
    if (d->refit_ev0) (void)hipEventDestroy(d->refit_ev0);
    if (d->refit_ev1) (void)hipEventDestroy(d->refit_ev1);
    void* ptrs[] = {d->nodes, d->leaves, d->prims, d->verts, d->normals, d->mats, d->lights, d->domes, d->insts,
                    d->inst_hit_base, d->inst_class, d->inst_cell, d->tables,
                    d->gamma, d->gammaF, d->d_rgb, d->d_rgb8, d->texs, d->puv, d->uvs, d->tans, d->btans,
                    d->pflags, d->verts2};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (void* p : d->bufs)
        if (p) (void)hipFree(p);
    delete d;
}

// Scratch context of `stream` (created on first use, at most kMaxStreamCtx).
int get_ctx(DeviceState& d, hipStream_t stream, StreamCtx*& out) {
    std::lock_guard<std::mutex> g(d.mu);
    for (StreamCtx* c : d.ctxs)
        if (c->stream == stream) { out = c; return MRT_OK; }
    if ((int)d.ctxs.size() >= kMaxStreamCtx) { set_error("too many streams on one scene (max 16)"); return MRT_ERR_INVALID; }
    StreamCtx* c = new StreamCtx();
    c->stream = stream;
    d.ctxs.push_back(c);   // owned by d from here (freed with it even if an allocation below fails)
    HIP_OK(hipMalloc((void**)&c->gstack, (size_t)kGlobalStack * d.gthreads * sizeof(int32_t)));
    HIP_OK(hipMalloc((void**)&c->ctr, kCtrBytes));
    HIP_OK(hipMalloc((void**)&c->wave_log, (size_t)2 * d.grid * (kWG / 64) * kLogWords * sizeof(unsigned long long)));
    HIP_OK(hipEventCreate(&c->ev0));
    HIP_OK(hipEventCreate(&c->ev1));
    HIP_OK(hipEventCreate(&c->evm));
    out = c;
    return MRT_OK;
}

template <typename T>
static int upload(T*& dst, const void* src, size_t bytes, size_t& total) {
    HIP_OK(hipMalloc((void**)&dst, bytes ? bytes : 16));
    if (bytes) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    total += bytes;
    return MRT_OK;
}

static int upload_scene(Scene& s, DeviceState& d, int device);

void free_replicas(Scene& s) {
    for (DeviceState* d : s.devs) free_device(d);
    s.devs.clear();
    s.dev = nullptr;
}

// The scene's replica on `device` (uploaded on first use; all replicas are
// dropped when the host scene changed) becomes s.dev.
int ensure_device(Scene& s, int device) {
    if (!s.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    if (s.dev_dirty) {
        if (const int rc = sync_host(s)) return rc;   // a device refit is ahead of the host copy the re-upload reads
        free_replicas(s);
        s.dev_dirty = false;
    }
    for (DeviceState* d : s.devs)
        if (d->device == device) { s.dev = d; return MRT_OK; }
    if (const int rc = sync_host(s)) return rc;   // a second device is uploaded from the host copy
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device"); return MRT_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) { set_error("bad device ordinal"); return MRT_ERR_INVALID; }
    if (s.lights.size() > (size_t)kMaxLights) { set_error("too many lights"); return MRT_ERR_INVALID; }
    DeviceState* d = new DeviceState();
    const int rc = upload_scene(s, *d, device);
    if (rc) { free_device(d); return rc; }
    s.devs.push_back(d);
    s.dev = d;
    return MRT_OK;
}

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

static int upload_scene(Scene& s, DeviceState& d, int device) {
    d.device = device;
    HIP_OK(hipSetDevice(device));
    // shading arrays: concatenate meshes
    std::vector<float4> V, N;
    std::vector<uint32_t> vbase(s.meshes.size()), nbase(s.meshes.size());
    for (size_t m = 0; m < s.meshes.size(); m++) {
        vbase[m] = (uint32_t)V.size();
        nbase[m] = (uint32_t)N.size();
        for (auto& p : s.meshes[m].verts) V.push_back(make_float4(p.x, p.y, p.z, 1.f));
        for (auto& p : s.meshes[m].normals) N.push_back(make_float4(p.x, p.y, p.z, 0.f));
    }
    // PrimShade: the world objects (a ProxyObject's own slot stays zero), then each BLAS's objects
    auto shade_rec = [&](int32_t mesh, int32_t tri) {
        PrimShade p{};
        if (mesh < 0) {   // a ProxyObject's own world slot: never a hit (hit_record_usable refuses it by this mark)
            p.pad = 1u;
            return p;
        }
        const Mesh& m = s.meshes[mesh];
        const size_t t = (size_t)tri;
        for (int k = 0; k < 3; k++) {
            p.v[k] = vbase[mesh] + m.vidx[3 * t + k];
            p.n[k] = nbase[mesh] + m.nidx[3 * t + k];
        }
        p.mat = (uint32_t)m.material;
        return p;
    };
    // texture coordinates of texture-mapped meshes: (u, v) pairs, per-prim indices,
    // per-normal tangent frames (TriangleMesh::preCalc, host_texture.cpp)
    bool any_uv = false;
    for (const Mesh& m : s.meshes) any_uv |= !m.tidx.empty();
    std::vector<float2> UV;
    std::vector<float4> TN, BTN;
    std::vector<uint32_t> ubase(s.meshes.size(), 0);
    if (any_uv) {
        TN.assign(N.size(), make_float4(0.f, 0.f, 0.f, 0.f));
        BTN.assign(N.size(), make_float4(0.f, 0.f, 0.f, 0.f));
        for (size_t m = 0; m < s.meshes.size(); m++) {
            const Mesh& M = s.meshes[m];
            ubase[m] = (uint32_t)UV.size();
            if (M.tidx.empty()) continue;
            for (size_t i = 0; i + 1 < M.uv.size(); i += 2) UV.push_back(make_float2(M.uv[i], M.uv[i + 1]));
            for (size_t i = 0; i < M.tan.size(); i++) {
                TN[nbase[m] + i] = make_float4(M.tan[i].x, M.tan[i].y, M.tan[i].z, 0.f);
                BTN[nbase[m] + i] = make_float4(M.btan[i].x, M.btan[i].y, M.btan[i].z, 0.f);
            }
        }
    }
    auto uv_rec = [&](int32_t mesh, int32_t tri) {
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (mesh < 0 || s.meshes[mesh].tidx.empty()) return u;
        const uint32_t* t = &s.meshes[mesh].tidx[3 * (size_t)tri];
        return make_uint4(ubase[mesh] + t[0], ubase[mesh] + t[1], ubase[mesh] + t[2], 1u);
    };
    std::vector<PrimShade> PS;
    std::vector<uint4> PUV;
    for (size_t i = 0; i < s.obj_mesh.size(); i++) {
        PS.push_back(shade_rec(s.obj_mesh[i], s.obj_tri[i]));
        if (any_uv) PUV.push_back(uv_rec(s.obj_mesh[i], s.obj_tri[i]));
    }
    std::vector<int32_t> shade_base(s.blas.size());
    for (size_t b = 0; b < s.blas.size(); b++) {
        shade_base[b] = (int32_t)PS.size();
        for (size_t i = 0; i < s.blas[b].obj_mesh.size(); i++) {
            PS.push_back(shade_rec(s.blas[b].obj_mesh[i], s.blas[b].obj_tri[i]));
            if (any_uv) PUV.push_back(uv_rec(s.blas[b].obj_mesh[i], s.blas[b].obj_tri[i]));
        }
    }
    // materials with maps; world leaf packets holding alpha-mapped triangles
    d.has_maps = false;
    std::vector<char> alpha_mat(s.materials.size(), 0);
    for (size_t m = 0; m < s.materials.size(); m++) {
        const int32_t* mp = s.materials[m].maps;
        d.has_maps |= mp[kMapColor] >= 0 || mp[kMapNormal] >= 0 || mp[kMapSpecular] >= 0 || mp[kMapReflect] >= 0 ||
                      mp[kMapRefract] >= 0;
        alpha_mat[m] = mp[kMapAlpha] >= 0;
    }
    auto alpha_obj = [&](int32_t p) {
        return p >= 0 && (size_t)p < s.obj_mesh.size() && s.obj_mesh[p] >= 0 &&
               alpha_mat[(size_t)s.meshes[s.obj_mesh[p]].material];
    };
    // MBObject world triangles (meshes with time-1 vertices)
    auto mb_obj = [&](int32_t p) {
        return p >= 0 && (size_t)p < s.obj_mesh.size() && s.obj_mesh[p] >= 0 &&
               (s.obj_inst.empty() || s.obj_inst[(size_t)p] < 0) && !s.meshes[s.obj_mesh[p]].verts2.empty();
    };
    std::vector<uint8_t> PF(s.obj_mesh.size(), 0);
    d.has_mb = false;
    for (size_t i = 0; i < PF.size(); i++)
        if (mb_obj((int32_t)i)) { PF[i] = 1; d.has_mb = true; }
    d.has_alpha = false;
    std::vector<uint16_t> tab(4096);
    memcpy(tab.data(), host_rcp_table(), 4096);
    memcpy(tab.data() + 2048, host_rsqrt_table(), 4096);
    size_t total = 0;
    int rc;
    // device node / leaf arrays: the world hierarchy, then each BLAS (indices
    // offset).  Leaf slots carry their packet's object count and a ProxyObject
    // bit (leaf_child); a ProxyObject lane's prim is -2 - instance.
    size_t n_leaves = s.leaves.size();
    for (const Blas& B : s.blas) n_leaves += B.leaves.size();
    if (n_leaves >= (size_t(1) << 27)) { set_error("too many leaf packets"); return MRT_ERR_OVERFLOW; }
    std::vector<QNode> DN;
    std::vector<DLeaf> DL;
    auto append = [&](const std::vector<QNode>& nodes, const std::vector<QLeaf>& leaves,
                      const std::vector<int32_t>* oi, const Blas* B) -> int32_t {
        const int32_t nb = (int32_t)DN.size(), lb = (int32_t)DL.size();
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
                                 (alpha_obj(L.prim[j]) || mb_obj(L.prim[j]));   // world: alpha / motion blur
                        alpha |= B != nullptr && (size_t)L.prim[j] < B->obj_mesh.size() &&
                                 alpha_mat[(size_t)s.meshes[B->obj_mesh[(size_t)L.prim[j]]].material];   // BLAS: alpha
                    }
                d.has_alpha |= alpha;
                q.child[k] = leaf_child((uint32_t)(~c + lb), cnt < 1 ? 1 : cnt, proxy, alpha);
            }
            DN.push_back(q);
        }
        for (const QLeaf& L : leaves) {
            DLeaf D{};
            for (int k = 0; k < 4; k++) {
                for (int c = 0; c < 9; c++) D.tri[k][c] = L.t[4 * c + k];
                const int32_t pi = proxy_of(L.prim[k]);
                D.prim[k] = pi >= 0 ? -2 - pi : L.prim[k];
            }
            DL.push_back(D);
        }
        return nb;
    };
    append(s.nodes, s.leaves, &s.obj_inst, nullptr);
    std::vector<int32_t> blas_root(s.blas.size());
    d.blas.assign(s.blas.size(), DeviceState::BlasRange());
    for (size_t b = 0; b < s.blas.size(); b++) {
        d.blas[b].tree.leaf_base = (uint32_t)DL.size();
        blas_root[b] = append(s.blas[b].nodes, s.blas[b].leaves, nullptr, &s.blas[b]);
        d.blas[b].tree.n_nodes = (uint32_t)s.blas[b].nodes.size();
        d.blas[b].tree.n_leaves = (uint32_t)s.blas[b].leaves.size();
        d.blas[b].tree.shade_base = shade_base[b];
    }
    d.n_leaves_all = (uint32_t)DL.size();
    // The world hierarchy's first kLdsNodes nodes in breadth-first order get device
    // numbers 0 .. kLdsNodes - 1 (frame1_kernel<LN> stages them in LDS).  Device node
    // numbers are internal: the visit order follows the child slots, not the numbers.
    const size_t nw = s.nodes.size();
    d.lds_ok = nw >= (size_t)kLdsNodes;
    if (d.lds_ok) {
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
        d.lds_ok = bfs.size() == (size_t)kLdsNodes;
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
        for (int32_t& br : blas_root) br = perm[(size_t)br];
        d.node_perm.assign(perm.begin(), perm.begin() + (ptrdiff_t)nw);
    }
    for (size_t b = 0; b < s.blas.size(); b++) d.blas[b].tree.node_base = (uint32_t)blas_root[b];   // BLAS nodes keep their numbers
    d.world.n_nodes = (uint32_t)nw;
    d.world.n_leaves = (uint32_t)s.leaves.size();
    d.world.fixed_lanes = true;
    d.vbase = vbase;
    d.nbase = nbase;
    for (QNode& q : DN) q.pad[0] = slot_kinds(q.child);   // the walks read the slot kinds (node_kinds)
    if (!walk_arrays_fit(DN.size(), DL.size())) {   // 32-bit byte offsets in the walks (node_at / tri_at)
        set_error("scene too large: its node or leaf array passes 4 GiB");
        return MRT_ERR_OVERFLOW;
    }
    if ((rc = upload(d.nodes, DN.data(), DN.size() * sizeof(QNode), total))) return rc;
    std::vector<DevInstance> DI(s.instances.size());
    for (size_t i = 0; i < DI.size(); i++) {
        const Instance& I = s.instances[i];
        memcpy(DI[i].inv, I.inv, sizeof DI[i].inv);
        memcpy(DI[i].inv_t, I.inv_t, sizeof DI[i].inv_t);  // rows 0-2
        DI[i].root = blas_root[I.blas];
        DI[i].hit_base = I.hit_base;
        DI[i].shade_base = shade_base[I.blas];
        DI[i].pad = 0;
    }
    if ((rc = upload(d.insts, DI.data(), DI.size() * sizeof(DevInstance), total))) return rc;
    d.n_insts = (int)DI.size();
    {   // instance-major ray-bin keys (mrt_bin.h): hit bases, and instances ranked by BLAS then index
        std::vector<int32_t> hb(DI.size());
        std::vector<uint32_t> order(DI.size());
        for (size_t i = 0; i < DI.size(); i++) { hb[i] = DI[i].hit_base; order[i] = (uint32_t)i; }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return DI[a].root < DI[b].root; });
        std::vector<uint16_t> cls(DI.size());
        for (size_t r = 0; r < order.size(); r++) cls[order[r]] = (uint16_t)std::min<size_t>(127, r * 128 / order.size());
        if ((rc = upload(d.inst_hit_base, hb.data(), hb.size() * sizeof(int32_t), total))) return rc;
        if ((rc = upload(d.inst_class, cls.data(), cls.size() * sizeof(uint16_t), total))) return rc;
        // object-space cells: each instance's BLAS root box (its finite child boxes), 4 cells per axis
        std::vector<float4> cell(2 * DI.size());
        for (size_t i = 0; i < DI.size(); i++) {
            const QNode& R = DN[(size_t)DI[i].root];
            float lo3[3] = {0, 0, 0}, hi3[3] = {0, 0, 0};
            bool any3[3] = {false, false, false};
            for (int k = 0; k < 4; k++) {
                if (R.child[k] == kEmptySlot) continue;
                for (int a = 0; a < 3; a++) {
                    const float l = R.box[a * 4 + k], h = R.box[12 + a * 4 + k];
                    if (!std::isfinite(l) || !std::isfinite(h)) continue;
                    lo3[a] = any3[a] ? std::min(lo3[a], l) : l;
                    hi3[a] = any3[a] ? std::max(hi3[a], h) : h;
                    any3[a] = true;
                }
            }
            auto sc = [&](int a) { return hi3[a] > lo3[a] ? 4.0f / (hi3[a] - lo3[a]) : 0.0f; };
            cell[2 * i] = make_float4(lo3[0], lo3[1], lo3[2], (float)(s.instances[i].blas & 1));
            cell[2 * i + 1] = make_float4(sc(0), sc(1), sc(2), 0.f);
        }
        if ((rc = upload(d.inst_cell, cell.data(), cell.size() * sizeof(float4), total))) return rc;
    }
    d.n_world = (int)s.obj_mesh.size();
    if ((rc = upload(d.leaves, DL.data(), DL.size() * sizeof(DLeaf), total))) return rc;
    if ((rc = upload(d.prims, PS.data(), PS.size() * sizeof(PrimShade), total))) return rc;
    if ((rc = upload(d.verts, V.data(), V.size() * sizeof(float4), total))) return rc;
    if ((rc = upload(d.normals, N.data(), N.size() * sizeof(float4), total))) return rc;
    if ((rc = upload(d.mats, s.materials.data(), s.materials.size() * sizeof(DevMaterial), total))) return rc;
    if ((rc = upload(d.lights, s.lights.data(), s.lights.size() * sizeof(DevLight), total))) return rc;
    if ((rc = upload(d.tables, tab.data(), tab.size() * sizeof(uint16_t), total))) return rc;
    if ((rc = upload(d.gamma, host_gamma_lut(), 32769, total))) return rc;
    if ((rc = upload(d.gammaF, host_gamma_float_lut(), 32769 * sizeof(float), total))) return rc;
    // textures, then each dome light's tables (DomeLight::setTexture products)
    auto upload_floats = [&](const std::vector<float>& v, const float*& dst) -> int {
        float* p = nullptr;
        const int r = upload(p, v.data(), v.size() * sizeof(float), total);
        d.bufs.push_back(p);
        dst = p;
        return r;
    };
    std::vector<const float*> dtex(s.textures.size(), nullptr);
    for (size_t i = 0; i < s.textures.size(); i++)
        if ((rc = upload_floats(s.textures[i].rgb, dtex[i]))) return rc;
    std::vector<DevDome> DD(s.domes.size());
    for (size_t i = 0; i < s.domes.size(); i++) {
        const DomeTables& t = s.domes[i];
        DevDome& g = DD[i];
        if ((rc = upload_floats(t.cdf_u, g.cdf_u)) || (rc = upload_floats(t.func_u, g.func_u)) ||
            (rc = upload_floats(t.cdf_v, g.cdf_v)) || (rc = upload_floats(t.func_v, g.func_v)) ||
            (rc = upload_floats(t.inv_int_v, g.inv_int_v)) || (rc = upload_floats(t.cos_u, g.cos_u)) ||
            (rc = upload_floats(t.sin_u, g.sin_u)) || (rc = upload_floats(t.cos_v, g.cos_v)) ||
            (rc = upload_floats(t.sin_v, g.sin_v)))
            return rc;
        float *rad = nullptr, *gu = nullptr, *gv = nullptr;
        if ((rc = upload(rad, t.rad.data(), t.rad.size() * sizeof(float), total)) ||
            (rc = upload(gu, t.guide_u.data(), t.guide_u.size() * sizeof(int32_t), total)) ||
            (rc = upload(gv, t.guide_v.data(), t.guide_v.size() * sizeof(int32_t), total)))
            return rc;
        for (float* p : {rad, gu, gv}) d.bufs.push_back(p);
        g.rad = rad;
        g.guide_u = reinterpret_cast<const int32_t*>(gu);
        g.guide_v = reinterpret_cast<const int32_t*>(gv);
        g.tex = dtex[t.tex];
        g.inv_int_u = t.inv_int_u;
        g.nu = t.nu;
        g.nv = t.nv;
    }
    if ((rc = upload(d.domes, DD.data(), DD.size() * sizeof(DevDome), total))) return rc;
    d.env = s.env_tex >= 0 ? dtex[s.env_tex] : nullptr;
    std::vector<DevTexture> DT(s.textures.size());
    for (size_t i = 0; i < DT.size(); i++) DT[i] = DevTexture{dtex[i], s.textures[i].W, s.textures[i].H, s.textures[i].type, 0};
    if ((rc = upload(d.texs, DT.data(), DT.size() * sizeof(DevTexture), total))) return rc;
    if (any_uv) {
        if ((rc = upload(d.puv, PUV.data(), PUV.size() * sizeof(uint4), total))) return rc;
        if ((rc = upload(d.uvs, UV.data(), UV.size() * sizeof(float2), total))) return rc;
        if ((rc = upload(d.tans, TN.data(), TN.size() * sizeof(float4), total))) return rc;
        if ((rc = upload(d.btans, BTN.data(), BTN.size() * sizeof(float4), total))) return rc;
    }
    if (d.has_mb) {
        std::vector<float4> V2 = V;
        for (size_t m = 0; m < s.meshes.size(); m++)
            for (size_t i = 0; i < s.meshes[m].verts2.size(); i++) {
                const v3& p = s.meshes[m].verts2[i];
                V2[vbase[m] + i] = make_float4(p.x, p.y, p.z, 1.f);
            }
        if ((rc = upload(d.verts2, V2.data(), V2.size() * sizeof(float4), total))) return rc;
        if ((rc = upload(d.pflags, PF.data(), PF.size(), total))) return rc;
    }
    d.special = d.n_insts > 0 || d.has_alpha || d.has_mb;
    d.bytes = total;
    // persistent grid: resident workgroups on every CU
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    d.cus = prop.multiProcessorCount;
    if (hipDeviceGetAttribute(&d.wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) d.wall_khz = 0;
    d.grid = d.cus * kMaxBlocksPerCU;
    d.boxes_finite = true;
    d.boxes_ordered = true;
    for (const QNode& q : DN) {
        for (int k = 0; k < 24; k++) d.boxes_finite &= std::isfinite(q.box[k]);
        for (int i = 0; i < 4; i++)
            if (q.child[i] != kEmptySlot)
                for (int a = 0; a < 3; a++) d.boxes_ordered &= q.box[a * 4 + i] <= q.box[12 + a * 4 + i];
    }
    if (!DN.empty()) root_box(DN[0], d.bb_lo, d.bb_hi);
    d.point_only = true;
    d.dome = false;
    for (const DevLight& l : s.lights) {
        d.point_only &= (l.type == MRT_POINT_LIGHT);
        d.dome |= l.type == MRT_DOME_LIGHT;
    }
    d.recursive = 0;
    for (const DevMaterial& m : s.materials)
        if (m.type == MRT_BLINN && (m.reflect > 0.f || m.refract > 0.f || m.gloss < 1.f || m.translucency > 0.01f)) d.recursive = 1;
    if (s.path_trace) d.recursive = 2;
    d.disperse = false;
    // transparent shadows: the walk is compiled into the fused chain kernels only (it
    // needs a closest-hit traversal in the shading, which would cost the direct
    // kernels occupancy), and they shade a scene without secondary rays identically
    d.transparent = false;
    for (const DevLight& l : s.lights) d.transparent |= l.transparent != 0;
    if (d.transparent && !d.recursive) d.recursive = 1;
    d.pow_spec = false;
    for (const DevMaterial& m : s.materials) d.pow_spec |= m.type == MRT_BLINN && m.spec_exp != 1.0f;
    for (const DevMaterial& m : s.materials)
        d.disperse |= m.type == MRT_BLINN && m.disperse && (m.reflect > 0.f || m.refract > 0.f);
    d.gthreads = (uint32_t)d.grid * kWG;
    s.info.device_bytes = total;
    return MRT_OK;
}

}  // namespace mrt
