// mrt_upload.hip -- DevOwner (every device allocation, event and stream of csrc), and a
// scene's device replicas and their per-stream contexts: created, uploaded from the host
// image (host_image.cpp) and freed here (HIP runtime calls only: this file holds no kernel).
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

// ---- DevOwner: the one place that creates and frees device resources
static std::atomic<int64_t> g_live{0};   // every owner's resources in this process
int64_t DevOwner::live() { return g_live.load(); }

void DevOwner::keep(void* h, void (*destroy)(void*), bool memory) {
    if (!h) return;   // (a zero-byte allocation is null: nothing to free)
    held.push_back(Held{h, destroy, memory});
    g_live++;
}

int DevOwner::memory(void*& p, size_t bytes, bool pinned) {
    if (pinned) {
        HIP_OK(hipHostMalloc(&p, bytes));
        keep(p, [](void* q) { (void)hipHostFree(q); }, true);
    } else {
        HIP_OK(hipMalloc(&p, bytes));
        keep(p, [](void* q) { (void)hipFree(q); }, true);
    }
    return MRT_OK;
}

int DevOwner::event(hipEvent_t& ev, unsigned flags) {
    HIP_OK(hipEventCreateWithFlags(&ev, flags));
    keep(ev, [](void* e) { (void)hipEventDestroy(static_cast<hipEvent_t>(e)); }, false);
    return MRT_OK;
}

int DevOwner::stream(hipStream_t& st) {
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    keep(st, [](void* s) { (void)hipStreamDestroy(static_cast<hipStream_t>(s)); }, false);
    return MRT_OK;
}

void DevOwner::release(void* p) {
    const auto it = std::find_if(held.begin(), held.end(), [&](const Held& r) { return r.memory && r.h == p; });
    if (it == held.end()) return;
    it->destroy(p);
    g_live--;
    held.erase(it);
}

void DevOwner::free_all() {
    for (const bool memory : {false, true})   // events and streams first
        for (const Held& r : held)
            if (r.memory == memory) { r.destroy(r.h); g_live--; }
    held.clear();
}

int reserve(DevOwner& own, const hipStream_t* drain, std::initializer_list<GrowBuf> bufs, std::initializer_list<GrowCap> caps) {
    bool enough = true, live = false;
    for (const GrowCap& k : caps) enough &= k.need <= *k.cap;
    if (enough) return MRT_OK;
    for (const GrowBuf& b : bufs) live |= *b.ptr != nullptr;
    if (live && drain) HIP_OK(hipStreamSynchronize(*drain));
    for (const GrowBuf& b : bufs) {
        own.release(*b.ptr);
        *b.ptr = nullptr;
    }
    for (const GrowCap& k : caps) *k.cap = 0;
    for (const GrowBuf& b : bufs)
        if (const int rc = own.alloc(*b.ptr, b.bytes)) return rc;
    for (const GrowCap& k : caps) *k.cap = k.need;
    return MRT_OK;
}

// no launch may still use what the owners hold: the caller has synchronised the device
static void free_device(DeviceState* d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    for (StreamCtx* c : d->ctxs) delete c;
    for (ShareBuf* b : d->share_bufs) delete b;
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
    int rc;
    if ((rc = c->own.alloc(c->gstack, (size_t)kGlobalStack * d.gthreads * sizeof(int32_t))) ||
        (rc = c->own.alloc(c->ctr, kCtrBytes)) ||
        (rc = c->own.alloc(c->wave_log, (size_t)2 * d.grid * (kWG / 64) * kLogWords * sizeof(unsigned long long))) ||
        (rc = c->own.event(c->ev0)) || (rc = c->own.event(c->ev1)) || (rc = c->own.event(c->evm)))
        return rc;
    out = c;
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

// The replica of a built scene: its host image (build_image) copied array by array, then the
// device's properties.
static int upload_scene(Scene& s, DeviceState& d, int device) {
    d.device = device;
    s.upload_count++;
    HIP_OK(hipSetDevice(device));
    DeviceImage g;
    std::string err;
    int rc;
    if ((rc = build_image(s, g, err))) { set_error(err); return rc; }
    DevOwner& o = d.own;
    auto up = [&](auto*& dst, const auto& v) { return o.upload(dst, v.data(), v.size() * sizeof(v[0])); };
    if ((rc = up(d.nodes, g.DN)) || (rc = up(d.insts, g.DI)) || (rc = up(d.inst_hit_base, g.hit_base)) ||
        (rc = up(d.inst_class, g.cls)) || (rc = up(d.inst_cell, g.cell)) || (rc = up(d.leaves, g.DL)) ||
        (rc = up(d.prims, g.PS)) || (rc = up(d.verts, g.V)) || (rc = up(d.normals, g.N)) || (rc = up(d.mats, s.materials)) ||
        (rc = up(d.lights, s.lights)) || (rc = up(d.tables, g.tab)) || (rc = o.upload(d.gamma, host_gamma_lut(), 32769)) ||
        (rc = o.upload(d.gammaF, host_gamma_float_lut(), 32769 * sizeof(float))))
        return rc;
    // textures, then each dome light's tables (DomeLight::setTexture products)
    std::vector<const float*> dtex(s.textures.size(), nullptr);
    for (size_t i = 0; i < s.textures.size(); i++)
        if ((rc = up(dtex[i], s.textures[i].rgb))) return rc;
    std::vector<DevDome> DD(s.domes.size());
    for (size_t i = 0; i < s.domes.size(); i++) {
        const DomeTables& t = s.domes[i];
        DevDome& q = DD[i];
        if ((rc = up(q.cdf_u, t.cdf_u)) || (rc = up(q.func_u, t.func_u)) || (rc = up(q.cdf_v, t.cdf_v)) ||
            (rc = up(q.func_v, t.func_v)) || (rc = up(q.inv_int_v, t.inv_int_v)) || (rc = up(q.cos_u, t.cos_u)) ||
            (rc = up(q.sin_u, t.sin_u)) || (rc = up(q.cos_v, t.cos_v)) || (rc = up(q.sin_v, t.sin_v)) ||
            (rc = up(q.rad, t.rad)) || (rc = up(q.guide_u, t.guide_u)) || (rc = up(q.guide_v, t.guide_v)))
            return rc;
        q.tex = dtex[t.tex];
        q.inv_int_u = t.inv_int_u;
        q.nu = t.nu;
        q.nv = t.nv;
    }
    if ((rc = up(d.domes, DD))) return rc;
    d.env = s.env_tex >= 0 ? dtex[s.env_tex] : nullptr;
    std::vector<DevTexture> DT(s.textures.size());
    for (size_t i = 0; i < DT.size(); i++) DT[i] = DevTexture{dtex[i], s.textures[i].W, s.textures[i].H, s.textures[i].type, 0};
    if ((rc = up(d.texs, DT))) return rc;
    d.dome_recs = DD;   // mrt_relight.hip writes through these pointers
    d.tex_recs = DT;
    if (g.any_uv && ((rc = up(d.puv, g.PUV)) || (rc = up(d.uvs, g.UV)) || (rc = up(d.tans, g.TN)) || (rc = up(d.btans, g.BTN))))
        return rc;
    if (g.has_mb && ((rc = up(d.verts2, g.V2)) || (rc = up(d.pflags, g.PF)))) return rc;
    static_cast<ImageInfo&>(d) = std::move(static_cast<ImageInfo&>(g));
    // persistent grid: resident workgroups on every CU
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    d.cus = prop.multiProcessorCount;
    if (hipDeviceGetAttribute(&d.wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) d.wall_khz = 0;
    d.grid = d.cus * kMaxBlocksPerCU;
    d.gthreads = (uint32_t)d.grid * kWG;
    s.info.device_bytes = d.bytes;
    return MRT_OK;
}

}  // namespace mrt

extern "C" int64_t mrt_debug_live_resources(void) { return mrt::DevOwner::live(); }
