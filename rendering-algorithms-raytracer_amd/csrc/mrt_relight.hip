// mrt_relight.hip -- relighting in place: new light records, a material's base record and the
// texels of a texture on the replicas, without a re-upload.
//
// Lights and materials arrive as a kernel argument and one small kernel stores them, so the
// update is ordered on the caller's stream and needs no staging buffer.  New texels are copied
// over the replica's; when the texture feeds a dome light, DomeLight::setTexture
// (src/DomeLight.cpp:8-78) runs again here, to the bits of build_dome (host_texture.cpp):
//   dome_scan_kernel    per column u the texel averages x sin(theta) and the running sum
//                       cdf[i] = cdf[i-1] + f[i-1] / nv (a recurrence: one lane per column,
//                       64 columns per block, rows staged in LDS and written out transposed)
//   dome_guide_kernel   per column cdf[i] / int_v[u] and its guide table (guide_table's merge)
//   dome_row_kernel     the same over the column integrals, one chain on one lane; decides
//                       whether int_u is positive and finite
//   dome_rad_kernel     the lat-long lookup of every table direction, one lane per cell
//   dome_commit_kernel  scratch tables over the live ones, only when int_u passed
//   tex_commit_kernel   the caller's texels over the live ones, only when int_u passed;
//                       otherwise one device word counts the refusal
// The builds read the caller's texels and write scratch, so a refused update changes nothing.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mrt_device.h"
#include "mrt_pick.h"
#include "mrt_texture.h"

namespace mrt {

// kMaxLights DevLight records, or one DevMaterial, by value (under 1 KB of kernel argument)
struct RelightWords {
    uint32_t w[kMaxLights * sizeof(DevLight) / 4];
};
static_assert(sizeof(DevLight) % 4 == 0 && sizeof(DevMaterial) % 4 == 0, "records are whole words");
static_assert(sizeof(DevMaterial) <= sizeof(RelightWords) && sizeof(RelightWords) < 1024, "a kernel argument under 1 KB");

// One dome build: the caller's texels, the size, the scratch tables and the live ones.
struct DomeBuild {
    const float* src;        // the caller's texels (nu x nv x 3 for a dome texture)
    float* tex;              // the replica's
    uint32_t n_tex;          // floats
    int32_t nu, nv;
    const float* sin_theta;  // nv (dome_sin_theta)
    const float *cos_u, *sin_u, *cos_v, *sin_v;   // the live angle tables: they depend on the size only
    float *s_rad, *s_func_v, *s_cdf_v, *s_inv_int_v, *s_int_v, *s_func_u, *s_cdf_u, *s_scal;   // scratch; s_scal: int_u, 1 / int_u
    int32_t *s_guide_u, *s_guide_v;
    float *rad, *func_v, *cdf_v, *inv_int_v, *func_u, *cdf_u, *ints;   // live; ints: int_v[nu], then int_u
    int32_t *guide_u, *guide_v;
    DevDome* rec;            // its record on the device (inv_int_u)
    uint32_t* status;        // DeviceState::relight_status
    int32_t count;           // an async update: a refusal is counted in status[0]
    int32_t gated;           // tex_commit_kernel: copy only when status[1] (the texture feeds a dome)
};

namespace {

constexpr int kTile = 64;                 // columns of a block = lanes of its one wave = rows of v per LDS tile
constexpr int kTileStride = kTile + 1;    // padded: lane c walking row r and lane r walking column c both hit 64 banks
constexpr int kCopyWG = 256;

// rows r0 .. r0 + rows - 1 of the tile's columns to dst[(u0 + c) * stride + off + row]: one store
// instruction per column covers `rows` consecutive floats
__device__ inline void tile_store(float* __restrict__ dst, const float* t, int u0, int nu, size_t stride, size_t off, int r0,
                                  int rows) {
    const int lane = (int)threadIdx.x;
    for (int c = 0; c < kTile && u0 + c < nu; c++)
        if (lane < rows) dst[(size_t)(u0 + c) * stride + off + (size_t)(r0 + lane)] = t[c * kTileStride + lane];
}
__device__ inline void tile_load(float* t, const float* __restrict__ src, int u0, int nu, size_t stride, size_t off, int r0,
                                 int rows) {
    const int lane = (int)threadIdx.x;
    for (int c = 0; c < kTile && u0 + c < nu; c++)
        if (lane < rows) t[c * kTileStride + lane] = src[(size_t)(u0 + c) * stride + off + (size_t)(r0 + lane)];
}

// build_dome's img and col, and step_cdf's first loop, for column u = the lane's: the texture is
// row-major with u along a row, so the wave's texel reads at one v are consecutive
__global__ __launch_bounds__(kTile) void dome_scan_kernel(DomeBuild B) {
    __shared__ float tf[kTile * kTileStride], tc[kTile * kTileStride];
    const int lane = (int)threadIdx.x, u0 = (int)blockIdx.x * kTile, u = u0 + lane;
    const int nu = B.nu, nv = B.nv;
    const bool live = u < nu;
    const float up = (float)u / (float)nu;
    float cdf = 0.f;
    for (int r0 = 0; r0 < nv; r0 += kTile) {
        const int rows = nv - r0 < kTile ? nv - r0 : kTile;
        if (live) {
#pragma unroll 4
            for (int r = 0; r < rows; r++) {   // the lookups do not depend on the running sum: several in flight
                const int v = r0 + r;
                const float vp = (float)v / (float)nv;
                const v3 L = tex_lookup3(B.src, nu, nv, up, vp);
                const float img = ((L.x + L.y) + L.z) * 0.333333f;   // Vector3::average
                const float f = img * B.sin_theta[v];
                cdf = cdf + f / (float)nv;
                tf[lane * kTileStride + r] = f;
                tc[lane * kTileStride + r] = cdf;
            }
        }
        __syncthreads();
        tile_store(B.s_func_v, tf, u0, nu, (size_t)nv, 0, r0, rows);
        tile_store(B.s_cdf_v, tc, u0, nu, (size_t)nv + 1, 1, r0, rows);
        __syncthreads();
    }
    if (live) {
        B.s_cdf_v[(size_t)u * ((size_t)nv + 1)] = 0.f;
        B.s_int_v[u] = cdf;
        B.s_inv_int_v[u] = 1.f / cdf;
    }
}

// step_cdf's second loop and guide_table for column u = the lane's.  guide_table's merge with
// the loops exchanged: entry i of bucket k closes every open bucket b <= k (g[b] = the first i
// whose bucket reaches b, which is what the merge leaves, ordered CDF or not: a black column's
// entries are 0/0 and x/0, bucket 0 by trunc_i32).
__global__ __launch_bounds__(kTile) void dome_guide_kernel(DomeBuild B) {
    __shared__ float tc[kTile * kTileStride];
    const int lane = (int)threadIdx.x, u0 = (int)blockIdx.x * kTile, u = u0 + lane;
    const int nu = B.nu, nv = B.nv;
    const bool live = u < nu;
    const float c = live ? B.s_int_v[u] : 1.f;
    int32_t* g = B.s_guide_v + (size_t)(live ? u : 0) * ((size_t)nv + 1);
    int b = 1;   // cdf[0] = 0 is in bucket 0
    if (live) g[0] = 0;
    for (int r0 = 0; r0 < nv; r0 += kTile) {
        const int rows = nv - r0 < kTile ? nv - r0 : kTile;
        tile_load(tc, B.s_cdf_v, u0, nu, (size_t)nv + 1, 1, r0, rows);
        __syncthreads();
        if (live)
            for (int r = 0; r < rows; r++) {
                const float x = tc[lane * kTileStride + r] / c;
                tc[lane * kTileStride + r] = x;
                const int k = guide_bucket(x, nv);   // <= nv - 1
                while (b <= k) g[b++] = r0 + r + 1;
            }
        __syncthreads();
        tile_store(B.s_cdf_v, tc, u0, nu, (size_t)nv + 1, 1, r0, rows);
        __syncthreads();
    }
    if (live)
        while (b <= nv) g[b++] = nv + 1;
}

// step_cdf and guide_table over the column integrals: one chain of nu additions on lane 0 (the
// divisions before it and after it are the wave's); then the int_u test of build_dome
__global__ __launch_bounds__(kTile) void dome_row_kernel(DomeBuild B) {
    __shared__ float q[kTile];
    __shared__ int bk[kTile];
    __shared__ float total;
    const int lane = (int)threadIdx.x, nu = B.nu;
    float run = 0.f;
    if (lane == 0) B.s_cdf_u[0] = 0.f;
    for (int base = 0; base < nu; base += kTile) {
        const int i = base + lane, m = nu - base < kTile ? nu - base : kTile;
        if (i < nu) {
            const float f = B.s_int_v[i];
            B.s_func_u[i] = f;
            q[lane] = f / (float)nu;
        }
        __syncthreads();
        if (lane == 0)
            for (int k = 0; k < m; k++) {
                run = run + q[k];
                q[k] = run;
            }
        __syncthreads();
        if (i < nu) B.s_cdf_u[i + 1] = q[lane];
        __syncthreads();
    }
    if (lane == 0) total = run;
    __syncthreads();
    const float c = total;
    int b = 1;
    if (lane == 0) {
        B.s_scal[0] = c;
        B.s_scal[1] = 1.f / c;
        B.status[1] = (c > 0.f && c <= 3.402823466e+38f) ? 1u : 0u;   // positive and finite
        B.s_guide_u[0] = 0;
    }
    for (int base = 0; base < nu; base += kTile) {
        const int i = base + lane, m = nu - base < kTile ? nu - base : kTile;
        if (i < nu) {   // (the lane that wrote s_cdf_u[i + 1] above)
            const float x = B.s_cdf_u[i + 1] / c;
            B.s_cdf_u[i + 1] = x;
            bk[lane] = guide_bucket(x, nu);
        }
        __syncthreads();
        if (lane == 0)
            for (int k = 0; k < m; k++)
                while (b <= bk[k]) B.s_guide_u[b++] = base + k + 1;
        __syncthreads();
    }
    if (lane == 0)
        while (b <= nu) B.s_guide_u[b++] = nu + 1;
}

// build_dome's rad: Texture::getLookupXYZ3 of table direction (iu, iv), row iv
__global__ __launch_bounds__(kCopyWG) void dome_rad_kernel(DomeBuild B) {
    const int nu = B.nu, nv = B.nv;
    const size_t n = ((size_t)nu + 1) * ((size_t)nv + 1);
    const size_t i = (size_t)blockIdx.x * kCopyWG + threadIdx.x;
    if (i >= n) return;
    const int iv = (int)(i / ((size_t)nu + 1)), iu = (int)(i % ((size_t)nu + 1));
    const float cosT = B.cos_v[iv], sinT = B.sin_v[iv], sinP = B.sin_u[iu], cosP = B.cos_u[iu];
    const v3 L = tex_lookup_dir(B.src, nu, nv, -sinT * cosP, -cosT, -sinT * sinP);
    reinterpret_cast<float4*>(B.s_rad)[i] = make_float4(L.x, L.y, L.z, 0.f);
}

template <typename T>
__device__ inline void copy_words(T* __restrict__ dst, const T* __restrict__ src, size_t n) {
    const size_t step = (size_t)gridDim.x * kCopyWG;
    for (size_t i = (size_t)blockIdx.x * kCopyWG + threadIdx.x; i < n; i += step) dst[i] = src[i];
}

__global__ __launch_bounds__(kCopyWG) void dome_commit_kernel(DomeBuild B) {
    if (!B.status[1]) return;
    const size_t nu = (size_t)B.nu, nv = (size_t)B.nv;
    copy_words(reinterpret_cast<float4*>(B.rad), reinterpret_cast<const float4*>(B.s_rad), (nu + 1) * (nv + 1));
    copy_words(B.func_v, (const float*)B.s_func_v, nu * nv);
    copy_words(B.cdf_v, (const float*)B.s_cdf_v, nu * (nv + 1));
    copy_words(B.guide_v, (const int32_t*)B.s_guide_v, nu * (nv + 1));
    copy_words(B.inv_int_v, (const float*)B.s_inv_int_v, nu);
    copy_words(B.ints, (const float*)B.s_int_v, nu);
    copy_words(B.func_u, (const float*)B.s_func_u, nu);
    copy_words(B.cdf_u, (const float*)B.s_cdf_u, nu + 1);
    copy_words(B.guide_u, (const int32_t*)B.s_guide_u, nu + 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        B.ints[nu] = B.s_scal[0];
        B.rec->inv_int_u = B.s_scal[1];
    }
}

__global__ __launch_bounds__(kCopyWG) void tex_commit_kernel(DomeBuild B) {
    if (B.gated && !B.status[1]) {
        if (B.count && blockIdx.x == 0 && threadIdx.x == 0) B.status[0] = B.status[0] + 1u;
        return;
    }
    copy_words(B.tex, B.src, (size_t)B.n_tex);
}

__global__ __launch_bounds__(kTile) void relight_store_kernel(unsigned* __restrict__ dst, RelightWords W, int n) {
    for (int i = (int)threadIdx.x; i < n; i += kTile) dst[i] = W.w[i];
}

}  // namespace

DomeFn pick_dome_scan() { return dome_scan_kernel; }
DomeFn pick_dome_guide() { return dome_guide_kernel; }
DomeFn pick_dome_row() { return dome_row_kernel; }
DomeFn pick_dome_rad() { return dome_rad_kernel; }
DomeFn pick_dome_commit() { return dome_commit_kernel; }
DomeFn pick_tex_commit() { return tex_commit_kernel; }
RelightFn pick_relight_store() { return relight_store_kernel; }

namespace {

const char* const kNoRadiance = "update_texture: dome texture has no positive radiance (zero Distribution1D integral)";

// the scratch tables of one build, in floats: rad first (float4 stores), the rest in DomeBuild's order
struct TabLayout {
    size_t rad, func_v, cdf_v, guide_v, inv_int_v, int_v, func_u, cdf_u, guide_u, scal, total;
    TabLayout(size_t nu, size_t nv) {
        size_t at = 0;
        auto take = [&](size_t n) { const size_t a = at; at += (n + 3) & ~size_t(3); return a; };
        rad = take(4 * (nu + 1) * (nv + 1));
        func_v = take(nu * nv);
        cdf_v = take(nu * (nv + 1));
        guide_v = take(nu * (nv + 1));
        inv_int_v = take(nu);
        int_v = take(nu);
        func_u = take(nu);
        cdf_u = take(nu + 1);
        guide_u = take(nu + 1);
        scal = take(4);
        total = at;
    }
};

// What the first texture update of replica d makes: per dome sin(theta) and the integrals
// mrt_scene_dome_export returns (from the host copy, which is current), the scratch tables sized
// by the largest dome, the status words and the timing events.
int prepare(Scene& S, DeviceState& d) {
    if (d.relight_ready) return MRT_OK;
    int rc;
    if ((rc = sync_host(S))) return rc;
    HIP_OK(hipSetDevice(d.device));
    size_t need = 0;
    d.relight_sin.assign(S.domes.size(), nullptr);
    d.relight_int.assign(S.domes.size(), nullptr);
    for (size_t k = 0; k < S.domes.size(); k++) {
        const DomeTables& T = S.domes[k];
        need = std::max(need, TabLayout((size_t)T.nu, (size_t)T.nv).total);
        std::vector<float> st, in(T.int_v);
        dome_sin_theta(T.nv, st);
        in.push_back(T.int_u);
        if ((rc = d.own.upload(d.relight_sin[k], st.data(), st.size() * sizeof(float))) ||
            (rc = d.own.upload(d.relight_int[k], in.data(), in.size() * sizeof(float))))
            return rc;
    }
    if ((rc = reserve(d.own, nullptr, {{(void**)&d.relight_tab, need * sizeof(float)}}, {{&d.relight_tab_cap, need}}))) return rc;
    if ((rc = d.own.alloc(d.relight_status, 2 * sizeof(uint32_t)))) return rc;
    HIP_OK(hipMemset(d.relight_status, 0, 2 * sizeof(uint32_t)));
    if ((rc = d.own.event(d.relight_ev0)) || (rc = d.own.event(d.relight_ev1))) return rc;
    d.relight_ready = true;
    return MRT_OK;
}

inline int blocks_of(size_t n, int wg, int cap) {
    const size_t b = (n + (size_t)wg - 1) / (size_t)wg;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)cap));
}

// New texels for texture `texture` of replica d from device memory `src`, on `stream`: every
// dome of the texture built into scratch and committed when its integral passes, then the texels.
int enqueue_texture(const Scene& S, DeviceState& d, int32_t texture, const float* src, bool count, hipStream_t stream) {
    const DevTexture& T = d.tex_recs[(size_t)texture];
    const std::vector<int32_t> ids = domes_of_texture(S, texture);
    DomeBuild B{};
    B.src = src;
    B.tex = const_cast<float*>(T.data);
    B.n_tex = (uint32_t)((size_t)T.W * T.H * tex_channels(T.type));
    B.status = d.relight_status;
    B.count = count ? 1 : 0;
    B.gated = ids.empty() ? 0 : 1;
    const int copy_cap = d.cus > 0 ? d.cus * 8 : 1024;
    for (int32_t k : ids) {
        const DevDome& R = d.dome_recs[(size_t)k];
        const size_t nu = (size_t)R.nu, nv = (size_t)R.nv;
        const TabLayout L(nu, nv);
        float* t = d.relight_tab;
        B.nu = R.nu;
        B.nv = R.nv;
        B.sin_theta = d.relight_sin[(size_t)k];
        B.cos_u = R.cos_u; B.sin_u = R.sin_u; B.cos_v = R.cos_v; B.sin_v = R.sin_v;
        B.s_rad = t + L.rad; B.s_func_v = t + L.func_v; B.s_cdf_v = t + L.cdf_v; B.s_inv_int_v = t + L.inv_int_v;
        B.s_int_v = t + L.int_v; B.s_func_u = t + L.func_u; B.s_cdf_u = t + L.cdf_u; B.s_scal = t + L.scal;
        B.s_guide_u = reinterpret_cast<int32_t*>(t + L.guide_u);
        B.s_guide_v = reinterpret_cast<int32_t*>(t + L.guide_v);
        B.rad = const_cast<float*>(R.rad); B.func_v = const_cast<float*>(R.func_v); B.cdf_v = const_cast<float*>(R.cdf_v);
        B.inv_int_v = const_cast<float*>(R.inv_int_v); B.func_u = const_cast<float*>(R.func_u);
        B.cdf_u = const_cast<float*>(R.cdf_u); B.ints = d.relight_int[(size_t)k];
        B.guide_u = const_cast<int32_t*>(R.guide_u); B.guide_v = const_cast<int32_t*>(R.guide_v);
        B.rec = d.domes + k;
        const int col_blocks = (int)((nu + kTile - 1) / kTile);
        const size_t cells = (nu + 1) * (nv + 1);
        hipLaunchKernelGGL(pick_dome_scan(), dim3(col_blocks), dim3(kTile), 0, stream, B);
        hipLaunchKernelGGL(pick_dome_guide(), dim3(col_blocks), dim3(kTile), 0, stream, B);
        hipLaunchKernelGGL(pick_dome_row(), dim3(1), dim3(kTile), 0, stream, B);
        hipLaunchKernelGGL(pick_dome_rad(), dim3((unsigned)((cells + kCopyWG - 1) / kCopyWG)), dim3(kCopyWG), 0, stream, B);
        hipLaunchKernelGGL(pick_dome_commit(), dim3(blocks_of(cells, kCopyWG, copy_cap)), dim3(kCopyWG), 0, stream, B);
    }
    hipLaunchKernelGGL(pick_tex_commit(), dim3(blocks_of(B.n_tex, kCopyWG, copy_cap)), dim3(kCopyWG), 0, stream, B);
    HIP_OK(hipGetLastError());
    return MRT_OK;
}

// the async entries: the scene on exactly one device, which becomes the current one
int async_one_replica(Scene& S, const char* name) {
    if (S.dev_dirty || S.devs.size() != 1 || !S.dev) {
        set_error(std::string(name) + "_async needs the scene uploaded to exactly one device (mrt_scene_upload)");
        return MRT_ERR_INVALID;
    }
    HIP_OK(hipSetDevice(S.dev->device));
    return MRT_OK;
}

// n words to `dst` of every replica (the async form: of the one replica, on `stream`), where
// dst = at(replica); then its launch flags follow the host copy (shading_flags)
template <typename At>
int store_records(Scene& S, const void* rec, size_t bytes, bool async, hipStream_t stream, const char* name, At at) {
    const bool on_device = !S.dev_dirty && !S.devs.empty();
    if (async) {
        if (const int rc = async_one_replica(S, name)) return rc;
    } else if (!on_device) {
        return MRT_OK;   // the host copy is the scene: the next upload reads it
    }
    RelightWords W{};
    memcpy(W.w, rec, bytes);
    DeviceState* cur = S.dev ? S.dev : S.devs[0];
    for (DeviceState* d : S.devs) {
        HIP_OK(hipSetDevice(d->device));
        if (!async) HIP_OK(hipDeviceSynchronize());   // no frame in flight may read the records while they change
        hipLaunchKernelGGL(pick_relight_store(), dim3(1), dim3(kTile), 0, async ? stream : nullptr, at(*d), W, (int)(bytes / 4));
        HIP_OK(hipGetLastError());
        if (!async) HIP_OK(hipStreamSynchronize(nullptr));
        shading_flags(S, *d);
    }
    HIP_OK(hipSetDevice(cur->device));
    return MRT_OK;
}

int update_lights(mrt_scene* s, const mrt_light* lights, int32_t n, bool async, hipStream_t stream) {
    if (!s) { set_error("update_lights: null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (const int rc = lights_check(S, lights, n)) return rc;
    if (async && (S.dev_dirty || S.devs.size() != 1 || !S.dev)) return async_one_replica(S, "update_lights");   // before any change
    if (n == 0) return MRT_OK;
    for (int32_t i = 0; i < n; i++) {
        S.lights[(size_t)i] = make_light(lights[i], S.lights[(size_t)i].dome);
        S.light_args[(size_t)i] = lights[i];
    }
    return store_records(S, S.lights.data(), (size_t)n * sizeof(DevLight), async, stream, "update_lights",
                         [](DeviceState& d) { return reinterpret_cast<unsigned*>(d.lights); });
}

int update_material(mrt_scene* s, int material, const mrt_material* m, bool async, hipStream_t stream) {
    if (!s) { set_error("update_material: null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (const int rc = material_check(S, material, m)) return rc;
    if (async && (S.dev_dirty || S.devs.size() != 1 || !S.dev)) return async_one_replica(S, "update_material");
    DevMaterial& D = S.materials[(size_t)material];
    set_material_base(D, *m);
    return store_records(S, &D, sizeof D, async, stream, "update_material",
                         [&](DeviceState& d) { return reinterpret_cast<unsigned*>(d.mats + material); });
}

void mark(std::vector<int32_t>& list, int32_t id) {
    if (std::find(list.begin(), list.end(), id) == list.end()) list.push_back(id);
}

}  // namespace

int relight_read_back(Scene& s, DeviceState& d) {
    for (int32_t t : s.host_tex_stale) {
        if ((size_t)t >= d.tex_recs.size() || (size_t)t >= s.textures.size()) continue;
        std::vector<float>& v = s.textures[(size_t)t].rgb;
        if (!v.empty()) HIP_OK(hipMemcpy(v.data(), d.tex_recs[(size_t)t].data, v.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    s.host_tex_stale.clear();
    for (int32_t k : s.host_dome_stale) {
        if ((size_t)k >= d.dome_recs.size() || (size_t)k >= d.relight_int.size() || (size_t)k >= s.domes.size()) continue;
        DomeTables& T = s.domes[(size_t)k];
        const DevDome& R = d.dome_recs[(size_t)k];
        auto get = [&](auto& v, const void* src) -> int {
            if (!v.empty()) HIP_OK(hipMemcpy(v.data(), src, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost));
            return MRT_OK;
        };
        int rc;
        if ((rc = get(T.cdf_u, R.cdf_u)) || (rc = get(T.func_u, R.func_u)) || (rc = get(T.cdf_v, R.cdf_v)) ||
            (rc = get(T.func_v, R.func_v)) || (rc = get(T.inv_int_v, R.inv_int_v)) || (rc = get(T.rad, R.rad)) ||
            (rc = get(T.guide_u, R.guide_u)) || (rc = get(T.guide_v, R.guide_v)) || (rc = get(T.int_v, d.relight_int[(size_t)k])))
            return rc;
        DevDome rec;
        HIP_OK(hipMemcpy(&T.int_u, d.relight_int[(size_t)k] + T.int_v.size(), sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(&rec, d.domes + k, sizeof rec, hipMemcpyDeviceToHost));
        T.inv_int_u = rec.inv_int_u;
    }
    s.host_dome_stale.clear();
    return MRT_OK;
}

}  // namespace mrt

using namespace mrt;

extern "C" {

int mrt_scene_update_lights(mrt_scene* s, const mrt_light* lights, int32_t n) { return update_lights(s, lights, n, false, nullptr); }
int mrt_scene_update_lights_async(mrt_scene* s, const mrt_light* lights, int32_t n, void* stream) {
    return update_lights(s, lights, n, true, (hipStream_t)stream);
}

int mrt_scene_update_material(mrt_scene* s, int material, const mrt_material* m) {
    return update_material(s, material, m, false, nullptr);
}
int mrt_scene_update_material_async(mrt_scene* s, int material, const mrt_material* m, void* stream) {
    return update_material(s, material, m, true, (hipStream_t)stream);
}

int mrt_scene_update_texture(mrt_scene* s, int32_t texture, const float* data, float* update_ms) {
    if (update_ms) *update_ms = 0.f;
    if (!s) { set_error("update_texture: null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    int rc;
    if ((rc = texture_check(S, texture, data))) return rc;   // arguments first: no device call before
    const bool on_device = !S.dev_dirty && !S.devs.empty();
    if (!on_device) {   // not uploaded (or a re-upload is due anyway): build_dome on the host
        if ((rc = sync_host(S))) return rc;
        return update_texture_host(S, texture, data);
    }
    Texture& T = S.textures[(size_t)texture];
    const std::vector<int32_t> ids = domes_of_texture(S, texture);
    DeviceState* cur = S.dev ? S.dev : S.devs[0];
    for (DeviceState* d : S.devs) {
        if ((rc = prepare(S, *d))) return rc;
        HIP_OK(hipSetDevice(d->device));
        HIP_OK(hipDeviceSynchronize());   // no frame in flight may read the texels while they change
        const size_t bytes = T.rgb.size() * sizeof(float);
        if ((rc = reserve(d->own, nullptr, {{(void**)&d->relight_stage, bytes}}, {{&d->relight_stage_cap, T.rgb.size()}}))) return rc;
        HIP_OK(hipMemcpy(d->relight_stage, data, bytes, hipMemcpyHostToDevice));
        HIP_OK(hipEventRecord(d->relight_ev0, nullptr));
        if ((rc = enqueue_texture(S, *d, texture, d->relight_stage, false, nullptr))) return rc;
        HIP_OK(hipEventRecord(d->relight_ev1, nullptr));
        HIP_OK(hipEventSynchronize(d->relight_ev1));
        if (d == cur && update_ms) HIP_OK(hipEventElapsedTime(update_ms, d->relight_ev0, d->relight_ev1));
        if (!ids.empty()) {
            uint32_t passed = 0;
            HIP_OK(hipMemcpy(&passed, d->relight_status + 1, sizeof passed, hipMemcpyDeviceToHost));
            if (!passed) {   // every replica refuses alike: nothing was committed anywhere
                HIP_OK(hipSetDevice(cur->device));
                set_error(kNoRadiance);
                return MRT_ERR_INVALID;
            }
        }
    }
    HIP_OK(hipSetDevice(cur->device));
    T.rgb.assign(data, data + T.rgb.size());
    S.host_tex_stale.erase(std::remove(S.host_tex_stale.begin(), S.host_tex_stale.end(), texture), S.host_tex_stale.end());
    for (int32_t k : ids) mark(S.host_dome_stale, k);
    return MRT_OK;
}

int mrt_scene_update_texture_async(mrt_scene* s, int32_t texture, const float* d_data, void* stream) {
    if (!s) { set_error("update_texture: null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    int rc;
    if ((rc = texture_check(S, texture, d_data))) return rc;
    if ((rc = async_one_replica(S, "update_texture"))) return rc;
    if ((rc = prepare(S, *S.dev))) return rc;
    if ((rc = enqueue_texture(S, *S.dev, texture, d_data, true, (hipStream_t)stream))) return rc;
    mark(S.host_tex_stale, texture);
    for (int32_t k : domes_of_texture(S, texture)) mark(S.host_dome_stale, k);
    return MRT_OK;
}

int mrt_scene_texture_update_status(mrt_scene* s, int32_t* rejected) {
    if (!s || !rejected) { set_error("texture_update_status: null argument"); return MRT_ERR_INVALID; }
    *rejected = 0;
    Scene& S = s->impl;
    DeviceState* d = S.dev ? S.dev : (S.devs.empty() ? nullptr : S.devs[0]);
    if (!d || !d->relight_ready) return MRT_OK;
    HIP_OK(hipSetDevice(d->device));
    uint32_t n = 0;
    HIP_OK(hipMemcpy(&n, d->relight_status, sizeof n, hipMemcpyDeviceToHost));
    if (n) HIP_OK(hipMemset(d->relight_status, 0, sizeof n));
    *rejected = (int32_t)n;
    return MRT_OK;
}

}  // extern "C"
