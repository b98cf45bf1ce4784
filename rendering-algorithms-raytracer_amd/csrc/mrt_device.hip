// mrt_device.hip -- kernels, launch logic and the device side of libmrt's C-ABI
// (MI355X / gfx950).  The CPU-only entries are in host_api.cpp, the scene upload, the
// per-stream contexts and the owner of all device memory in mrt_upload.hip, their shared
// state in mrt_device.h.
//
// Render kernel: persistent workgroups of 4 waves; a wave renders one 8x8
// pixel tile per step (one lane per pixel), so a wave's rays are coherent.
// Per lane: camera ray (Camera::eyeRayAdaptive, src/Camera.cpp:116-157) ->
// closest-hit traversal -> Lambert/Blinn shading (src/Lambert.cpp:19-53,
// src/Blinn.cpp:91-237) with PointLight / RectangleLight shadow rays traced
// any-hit (same occlusion boolean as the reference's closest-hit shadow rays)
// -> float RGB (+ Image::Map 8-bit).  The rcp/rsqrt tables (8 KB) and the
// traversal stacks live in LDS.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "mrt_bin.h"
#include "mrt_device.h"
#include "mrt_kernels.h"
#include "mrt_scene.h"
#include "mrt_texture.h"
#include "mrt_shader.h"

namespace mrt {

// Kernel 2b: every wavefront shadow ray of the frame, any-hit (the occlusion
// answer of Shader::occluded).  Slots past a pixel's ray count are skipped.
//   sched 0: grid-stride, one ray per lane per iteration.
//   sched 1: XCD bands -- the ray slots are cut into 8 contiguous bands (slot
//            order is pixel order, so a band is a band of the image) and
//            workgroup b, which runs on XCD b mod 8, takes 64-slot chunks of band
//            b mod 8 from that band's counter, then steals from the others: the
//            rays one XCD traces touch the geometry of one image band, so its
//            4 MB L2 holds that band's share of the hierarchy.
//   sched 2: sched 1 + lane refill: a lane whose ray is done (an any-hit ray
//            ends at its first accepted triangle) or whose slot is empty takes
//            a new slot as soon as `refill_min` lanes of its wave are idle;
//            traversal runs one node visit per wave step (anyhit_step; in
//            special-leaf scenes anyhit_step_inst, which defers ProxyObject
//            lanes onto the stack), so the wave no longer waits for its longest
//            ray.
// Every ray is traced with traverse()'s box and triangle tests (the same
// visit order, except the deferred instance walks of sched 2, which an
// any-hit answer does not depend on), so the answers are identical under
// every schedule.
static constexpr int kShadowChunk = 64;
// REFILL: sched 2 (its own kernel, so the chunked schedules' nested traversal
// does not set its register budget); CHECK: the lane-refill step of a
// special-leaf scene handles alpha-mapped / motion-blurred lanes.
template <bool COUNT, bool FAST, bool INST, bool REFILL, bool CHECK, int MINW = 1>
__global__ void __launch_bounds__(kWG, MINW) shadow_kernel(RenderParams P, size_t n_rays, int sched, int refill_min) {
    __shared__ uint16_t s_tab[2048];
    __shared__ int32_t s_stack[kLdsStack * kWG];
    load_tables(P.tables, s_tab, 1024);
    const int tid = threadIdx.x, lane = tid & 63;
    Trav T{P.nodes, P.fast_box != 0, P.scalar_nodes, P.leaves, s_tab, s_stack + tid,
           P.gstack + (blockIdx.x * kWG + tid), P.gstride};
    T.inst = P.insts;
    trav_alpha(T, P);
    TravStats st;
    unsigned long long wave_steps = 0;
    if (P.ch_ovf && *P.ch_ovf) return;   // a chain chunk past its estimated capacity (redone by its fallback)
    // chain levels: the entry count is on the device (n_rays is the capacity)
    if (P.sh_count) {
        const size_t nd = (size_t)*P.sh_count * (size_t)P.max_shadow;
        if (nd < n_rays) n_rays = nd;
    }
    // binned order (mrt_bin.h): position c traces slot perm[c]; the list holds valid slots only
    const uint32_t* perm = P.sh_perm;
    if (perm) n_rays = *P.sh_perm_n;
    // slot e = pixel slot * max_shadow + j (n_rays < 2^32, checked on the host: 32-bit division)
    const uint32_t m = (uint32_t)P.max_shadow, nr32 = (uint32_t)n_rays;
    auto valid = [&](size_t e64) {
        if (perm) return e64 < n_rays;
        // m through an empty asm: the division's reciprocal is formed here, per dequeue, instead of
        // once before the loop and held across the walk (it was the kernel's one spilled value)
        uint32_t mm = m;
        asm volatile("" : "+s"(mm));
        const uint32_t e = (uint32_t)e64, px = e / mm;
        return e64 < n_rays && e < nr32 && e - px * m < (uint32_t)P.nrays[px];
    };
    auto slot_at = [&](size_t c) -> size_t { return perm ? (size_t)perm[c] : c; };
    auto trace_one = [&](size_t e) __attribute__((always_inline)) {   // (inlined: see chain_trace_kernel)
        const float4 o = P.ray_o[e], d = P.ray_d[e];
        const DRay r = make_ray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), d.w);
        DHit h{o.w, 0.f, 0.f, -1};
        const uint32_t n0 = st.nodes;
        constexpr uint32_t ANYHIT = W_ANY | walk_opt(W_COUNT, COUNT) | walk_opt(W_FAST, FAST) | walk_opt(W_INST, INST) |
                                    walk_opt(W_NOCHECK, !CHECK) | walk_opt(W_XONE, !INST);
        P.occl[e] = traverse<ANYHIT>(T, r, 0.001f, h, st) ? 1 : 0;
        return st.nodes - n0;
    };
    // per-XCD band of ray slots and its chunk counter (own 128-B line)
    const int home = blockIdx.x & 7;
    auto band_lo = [&](int k) { return n_rays * (size_t)k / 8; };
    int band = home, probes = 0;
    // wave-level dequeue of `want` consecutive slots of the current band (or
    // the next band with slots left); returns the first slot (lane 0's atomic,
    // broadcast) and the end of its band, or exhausted
    auto dequeue = [&](uint32_t want, size_t& first, size_t& end) {
        unsigned long long got = ~0ull, hi = 0;
        if (lane == 0) {
            while (probes < 8) {
                const size_t lo = band_lo(band), bend = band_lo(band + 1);
                const unsigned long long v = atomicAdd(reinterpret_cast<unsigned long long*>(P.queue + band * 32),
                                                       (unsigned long long)want);
                if (lo + v < bend) { got = lo + v; hi = bend; break; }
                band = (band + 1) & 7;
                probes++;
            }
        }
        got = __shfl(got, 0);
        hi = __shfl(hi, 0);
        first = (size_t)got;
        end = (size_t)hi;
        return got != ~0ull;
    };
    if constexpr (!REFILL) {
        if (sched == 0) {
            for (size_t e0 = (size_t)blockIdx.x * kWG + (tid & ~63); e0 < n_rays; e0 += (size_t)gridDim.x * kWG) {
                const size_t e = e0 + lane;
                uint32_t v = valid(e) ? trace_one(slot_at(e)) : 0u;
                if (COUNT) {
                    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
                    wave_steps += v;
                }
            }
        } else {   // XCD bands: wave-uniform chunks, one ray per lane
            size_t first, end;
            while (dequeue(kShadowChunk, first, end)) {
                const size_t e = first + lane;
                uint32_t v = (e < end && valid(e)) ? trace_one(slot_at(e)) : 0u;
                if (COUNT) {
                    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
                    wave_steps += v;
                }
            }
        }
    } else {   // lane refill
        bool exhausted = false;   // wave-uniform
        bool active = false;
        uint32_t e = 0;   // the lane's ray slot (n_rays < 2^32, checked on the host): one VGPR, not two
        float tmax = 0.f;
        AnyState as{};
        for (;;) {
            const unsigned long long idle = __ballot(!active);
            const int nidle = __popcll(idle);
            if (!exhausted && (nidle >= refill_min || nidle == 64)) {
                size_t first, end;
                if (!dequeue((uint32_t)nidle, first, end)) {
                    exhausted = true;
                } else if (!active) {
                    const size_t c = first + (size_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                    if (c < end && valid(c)) {
                        e = (uint32_t)slot_at(c);
                        const float4 o = P.ray_o[e], d = P.ray_d[e];
                        as.q = make_ray(mk(o.x, o.y, o.z), mk(d.x, d.y, d.z), d.w);
                        tmax = o.w;
                        as.cur = 0;
                        as.sp = 0;
                        as.aoff = -1;
                        active = true;
                    }
                }
            }
            if (__ballot(active) == 0) {
                if (exhausted) break;
                continue;
            }
            if (COUNT) wave_steps++;
            if (active) {
                bool hit = false;
                bool done;
                if constexpr (INST) done = anyhit_step_inst<COUNT, FAST, CHECK>(T, 0.001f, tmax, as, P.ray_o, P.ray_d, e, hit, st);
                else done = (FAST && as.q.finite) ? anyhit_step<COUNT, true>(T, as.q, 0.001f, tmax, as.cur, as.sp, hit, st)
                                                  : anyhit_step<COUNT, false>(T, as.q, 0.001f, tmax, as.cur, as.sp, hit, st);
                if (done) {
                    P.occl[e] = hit ? 1 : 0;
                    active = false;
                }
            }
        }
    }
    if (COUNT) {
        unsigned long long nv = st.nodes, lv = st.leaves;
        for (int off = 32; off > 0; off >>= 1) {
            nv += __shfl_down(nv, off);
            lv += __shfl_down(lv, off);
        }
        if (lane == 0) {
            atomicAdd(&P.ctr[CTR_NODES], nv);
            atomicAdd(&P.ctr[CTR_LEAVES], lv);
            atomicAdd(&P.ctr[CTR_NODES_S], nv);
            atomicAdd(&P.ctr[CTR_WAVE_STEPS_S], wave_steps);
        }
    }
    if (st.overflow) atomicOr(&P.ctr[CTR_OVERFLOW], 1ull);
}


// Numerics probe (mrt_debug_libm): the device's acosf / atan2f / sinf / cosf / powf
// (mrt_libm.h) and rcp_nr (RCPSS emulation + Newton step, mrt_math.h; table from global
// memory).
__global__ void __launch_bounds__(256) libm_kernel(int fn, const float* x, const float* y, size_t n, float* out,
                                                   const uint16_t* rcpT) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = fn == 0 ? fd_acosf(x[i]) : fn == 1 ? fd_atan2f(y[i], x[i]) : fn == 2 ? rcp_nr(x[i], rcpT)
               : fn == 3 ? gl_sinf(x[i]) : fn == 4 ? gl_cosf(x[i]) : gl_powf(x[i], y[i]);
}

// Batched Scene::trace: one lane per query ray.  TIMED: the rays carry a time
// (mrt_trace_rays: Ray(o, d, time), where an MBObject lane's triangle is); without one
// they are Ray(o, d), time 0 (src/Ray.h:71).
template <bool ANY, bool INST, bool TIMED>
__device__ __forceinline__ void trace_rays(uint16_t* s_tab, int32_t* s_stack, const QNode* nodes, const DLeaf* leaves,
                                           const uint16_t* tables, int32_t* gstack, uint32_t gstride, const float* o,
                                           const float* d, const float* time, const float* tmin, const float* tmax,
                                           size_t n, mrt_hit* out, unsigned long long* ctr, int fast_box,
                                           const DevInstance* insts, const Trav& alpha) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += kWG) reinterpret_cast<uint32_t*>(s_tab)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    __syncthreads();
    const uint32_t gtid = blockIdx.x * kWG + tid;
    Trav T{nodes, fast_box != 0, false, leaves, s_tab, s_stack + tid, gstack + gtid, gstride};
    T.inst = insts;
    T.ovf = ctr + CTR_OVERFLOW;
    T.aprims = alpha.aprims; T.apuv = alpha.apuv; T.auv = alpha.auv; T.amats = alpha.amats; T.atex = alpha.atex;
    T.pflags = alpha.pflags; T.verts = alpha.verts; T.verts2 = alpha.verts2;
    TravStats st;
    for (size_t i = (size_t)blockIdx.x * kWG + tid; i < n; i += (size_t)gridDim.x * kWG) {
        DRay r = make_ray(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
        if constexpr (TIMED) r.time = time[i];
        DHit h{tmax[i], 0.f, 0.f, -1};
        bool hit = traverse<walk_opt(W_ANY, ANY) | walk_opt(W_INST, INST)>(T, r, tmin[i], h, st);
        mrt_hit res;
        res.t = h.t; res.a = h.a; res.b = h.b; res.prim = hit ? (ANY ? 0 : h.prim) : -1;
        res.inst = (hit && !ANY) ? h.inst : -1;
        if (ANY && hit) res.prim = 1;  // any-hit: occluded flag only
        out[i] = res;
    }
    if (st.overflow) atomicOr(&ctr[CTR_OVERFLOW], 1ull);
}
template <bool ANY, bool INST = false>
__global__ void __launch_bounds__(kWG) trace_kernel(const QNode* nodes, const DLeaf* leaves, const uint16_t* tables,
                                                    int32_t* gstack, uint32_t gstride, const float* o, const float* d,
                                                    const float* tmin, const float* tmax, size_t n, mrt_hit* out,
                                                    unsigned long long* ctr, int fast_box,
                                                    const DevInstance* insts, Trav alpha) {
    __shared__ uint16_t s_tab[2048];
    __shared__ int32_t s_stack[kLdsStack * kWG];
    trace_rays<ANY, INST, false>(s_tab, s_stack, nodes, leaves, tables, gstack, gstride, o, d, nullptr, tmin, tmax, n, out,
                                 ctr, fast_box, insts, alpha);
}
// mrt_trace_rays with a time array: a kernel of its own, so trace_kernel keeps its code
template <bool ANY, bool INST>
__global__ void __launch_bounds__(kWG) trace_timed_kernel(const QNode* nodes, const DLeaf* leaves, const uint16_t* tables,
                                                          int32_t* gstack, uint32_t gstride, const float* o, const float* d,
                                                          const float* time, const float* tmin, const float* tmax, size_t n,
                                                          mrt_hit* out, unsigned long long* ctr, int fast_box,
                                                          const DevInstance* insts, Trav alpha) {
    __shared__ uint16_t s_tab[2048];
    __shared__ int32_t s_stack[kLdsStack * kWG];
    trace_rays<ANY, INST, true>(s_tab, s_stack, nodes, leaves, tables, gstack, gstride, o, d, time, tmin, tmax, n, out, ctr,
                                fast_box, insts, alpha);
}

// Device hit records (t, a, b, prim bits) -> mrt_hit (mrt_sample_rays_async): m_proxy from
// the id, as to_hit() does on the host -- the last instance whose hit_base <= id.
__global__ void __launch_bounds__(256) hit_records_kernel(const float4* rec, size_t n, const DevInstance* insts,
                                                          int32_t n_insts, int32_t n_world, mrt_hit* out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float4 v = rec[i];
        mrt_hit h;
        h.t = v.x; h.a = v.y; h.b = v.z;
        h.prim = __float_as_int(v.w);
        h.inst = -1;
        if (h.prim >= n_world && n_insts > 0) {
            int lo = 0, hi = n_insts - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (insts[mid].hit_base <= h.prim) lo = mid; else hi = mid - 1;
            }
            h.inst = lo;
        }
        out[i] = h;
    }
}

// A caller's record as the kernels may use it: hit_record_class, and a ProxyObject's own
// world slot (PrimShade::pad, set on upload) refused too.  prims is read only for an id the
// comparisons have placed in [0, n_world).
__device__ __forceinline__ bool hit_record_usable(const mrt_hit& h, int32_t n_world, int32_t n_ids, const PrimShade* prims,
                                                  bool& invalid) {
    int k = hit_record_class(h.t, h.a, h.b, h.prim, n_ids);
    if (k > 0 && h.prim < n_world && prims[h.prim].pad != 0u) k = -1;
    invalid = k < 0;
    return k > 0;
}

// mrt_hit -> device hit records (t, a, b, prim bits) in the stream's hitbuf, in the place of
// the primary launch (mrt_shade_hits): the inverse of hit_records_kernel.  A miss and an
// invalid record become the walks' miss record; hits and invalid records are counted.
__global__ void __launch_bounds__(256) hit_supply_kernel(const mrt_hit* in, size_t n, int32_t n_world, int32_t n_ids,
                                                         const PrimShade* prims, float4* rec, unsigned long long* ctr) {
    unsigned long long nh = 0, nbad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const mrt_hit h = in[i];
        bool bad;
        const bool ok = hit_record_usable(h, n_world, n_ids, prims, bad);
        rec[i] = ok ? make_float4(h.t, h.a, h.b, __int_as_float(h.prim)) : make_float4(1e12f, 0.f, 0.f, __int_as_float(-1));
        nh += ok ? 1u : 0u;
        nbad += bad ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        nh += __shfl_down(nh, off);
        nbad += __shfl_down(nbad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nh) atomicAdd(&ctr[CTR_HITS], nh);
        if (nbad) atomicAdd(&ctr[CTR_INVALID], nbad);
    }
}

// Ray::getPoint + HitInfo::getAllInfos (src/Ray.cpp:5-49) per (ray, hit) pair: the shader's
// own normals() and texcoords(), the frame always asked for.  No shading-side change of N.
__global__ void __launch_bounds__(kWG) surface_kernel(RenderParams P, const float* o, const float* d, const mrt_hit* hits,
                                                      size_t n, int32_t n_ids, const SurfaceGroup* groups, int32_t n_groups,
                                                      mrt_surface* out) {
    const uint16_t* rsqT = P.tables + 2048;
    Trav T{};
    TravStats st;
    unsigned long long nbad = 0;
    for (size_t i = (size_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (size_t)gridDim.x * kWG) {
        const mrt_hit h = hits[i];
        bool bad;
        const bool ok = hit_record_usable(h, P.n_world, n_ids, P.prims, bad);
        nbad += bad ? 1u : 0u;
        mrt_surface s{};
        s.material = s.mesh = s.tri = s.inst = -1;
        if (ok) {
            Shader<false, false, true> S{P, T, P.tables, rsqT, st, 0u, 0u, 0u, 0, 0u};
            const DHit dh{h.t, h.a, h.b, h.prim};
            v3 N, geoN, tn, bt;
            uint32_t mat;
            float u, v;
            S.normals(dh, N, geoN, mat);
            S.texcoords(dh, true, u, v, tn, bt);
            int inst = -1;
            if (h.prim >= P.n_world) S.inst_shade_index(h.prim, &inst);
            int lo = 0, hi = n_groups - 1;   // the last run that starts at or before the record
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (groups[mid].start <= S.psi) lo = mid; else hi = mid - 1;
            }
            const SurfaceGroup g = groups[lo];
            for (int k = 0; k < 3; k++) s.p[k] = o[3 * i + k] + h.t * d[3 * i + k];   // Ray::getPoint
            s.n[0] = N.x; s.n[1] = N.y; s.n[2] = N.z;
            s.geo_n[0] = geoN.x; s.geo_n[1] = geoN.y; s.geo_n[2] = geoN.z;
            s.tan[0] = tn.x; s.tan[1] = tn.y; s.tan[2] = tn.z;
            s.bitan[0] = bt.x; s.bitan[1] = bt.y; s.bitan[2] = bt.z;
            s.u = u; s.v = v;
            s.material = (int32_t)mat;
            s.mesh = g.mesh;
            s.tri = g.tri0 + (S.psi - g.start) * g.step;
            s.inst = inst;
        }
        out[i] = s;
    }
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_down(nbad, off);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&P.ctr[CTR_INVALID], nbad);
}

// Bucket tiles -> frames.  Item id = frame * buckets_per_frame + bucket; frame f
// of the output starts at f * W * H pixels.  Float tiles (nullable) go to
// `frames`; 8-bit pixels come from tiles8 when given, else from the LUT.
// One 256-thread workgroup per item (a 32x32 tile), a thread per 4 consecutive
// pixels of a tile row: 48 B of float RGB as three 16-B loads and stores and 12 B
// of 8-bit RGB as three dword stores when the frame width is a multiple of 4
// and the buffers are 16-B / 4-B aligned (every 4-pixel group then is too);
// otherwise, and for groups the frame's right edge cuts, pixel by pixel.
__global__ void __launch_bounds__(256) unpack_kernel(const int32_t* items, int32_t n_items, const float* tiles,
                                                     const uint8_t* tiles8, int32_t W, int32_t H, int32_t buckets_x,
                                                     int32_t buckets_per_frame, int32_t n_frames, float* frames,
                                                     uint8_t* frames8, const uint8_t* gamma) {
    const int bslot = blockIdx.x;
    if (bslot >= n_items) return;
    const uint32_t id = (uint32_t)items[bslot];
    const uint32_t f = id / (uint32_t)buckets_per_frame, b = id % (uint32_t)buckets_per_frame;
    const int row = threadIdx.x >> 3, px = (threadIdx.x & 7) * 4;
    const int x = (int)(b % buckets_x) * 32 + px, y = (int)(b / buckets_x) * 32 + row;
    if (f >= (uint32_t)n_frames || x >= W || y >= H) return;  // ids outside the batch are ignored
    const size_t i = (size_t)bslot * 1024 + (size_t)(row * 32 + px);   // first pixel of the group in the tiles
    const size_t q = (size_t)f * W * H + (size_t)y * W + x;            // ... and in the frames
    const bool aligned = (((uintptr_t)tiles | (uintptr_t)frames) & 15) == 0 && (((uintptr_t)tiles8 | (uintptr_t)frames8) & 3) == 0;
    if ((W & 3) == 0 && aligned) {   // x + 3 < W: the whole group, aligned
        float v[12];
        if (tiles) {
            const float4* t4 = reinterpret_cast<const float4*>(tiles + 3 * i);
            const float4 a = t4[0], c = t4[1], d = t4[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y;
            v[6] = c.z; v[7] = c.w; v[8] = d.x; v[9] = d.y; v[10] = d.z; v[11] = d.w;
            if (frames) {
                float4* o4 = reinterpret_cast<float4*>(frames + 3 * q);
                o4[0] = a; o4[1] = c; o4[2] = d;
            }
        }
        if (frames8) {
            uint32_t w[3];
            if (tiles8) {
                const uint32_t* t = reinterpret_cast<const uint32_t*>(tiles8 + 3 * i);
                w[0] = t[0]; w[1] = t[1]; w[2] = t[2];
            } else {
                uint32_t c8[12];
#pragma unroll
                for (int k = 0; k < 12; k++) c8[k] = map8(gamma, v[k]);
#pragma unroll
                for (int k = 0; k < 3; k++)
                    w[k] = c8[4 * k] | c8[4 * k + 1] << 8 | c8[4 * k + 2] << 16 | c8[4 * k + 3] << 24;
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(frames8 + 3 * q);
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        }
        return;
    }
    for (int k = 0; k < 4 && x + k < W; k++) {
        const size_t ik = i + k, qk = q + k;
        if (tiles && frames) {
            frames[3 * qk] = tiles[3 * ik]; frames[3 * qk + 1] = tiles[3 * ik + 1]; frames[3 * qk + 2] = tiles[3 * ik + 2];
        }
        if (frames8) {
            if (tiles8) {
                frames8[3 * qk] = tiles8[3 * ik]; frames8[3 * qk + 1] = tiles8[3 * ik + 1];
                frames8[3 * qk + 2] = tiles8[3 * ik + 2];
            } else {
                frames8[3 * qk] = map8(gamma, tiles[3 * ik]); frames8[3 * qk + 1] = map8(gamma, tiles[3 * ik + 1]);
                frames8[3 * qk + 2] = map8(gamma, tiles[3 * ik + 2]);
            }
        }
    }
}

static constexpr int kRefillMin = 40;   // lane refill: idle lanes of a wave that trigger a dequeue
static constexpr int kBinBlocks = 4;   // binning launches: workgroups per CU (each reserves its range of every bin atomically)

static int host_camera(const mrt_camera* c, int W, int H, CamParams& out) {
    if (!c || W <= 0 || H <= 0) { set_error("bad camera/frame"); return MRT_ERR_INVALID; }
    const uint16_t* RS = host_rsqrt_table();
    // Camera::setEye/setLookAt/setUp (src/Camera.h:82-124), eyeRayAdaptive basis
    v3 eye = mk(c->eye[0], c->eye[1], c->eye[2]);
    v3 viewDir = normalized(sub(mk(c->look_at[0], c->look_at[1], c->look_at[2]), eye), RS);
    v3 up = normalized(mk(c->up[0], c->up[1], c->up[2]), RS);
    v3 w = normalized(neg(viewDir), RS);
    v3 u = normalized(cross(up, w), RS);
    v3 v = cross(w, u);
    float aspect = (float)W / (float)H;
    const float DegToRad = 3.1415926f / 180.0f, Half = DegToRad / 2.0f;
    float top = tanf(c->fov_deg * Half);
    float right = aspect * top;
    out.eye[0] = eye.x; out.eye[1] = eye.y; out.eye[2] = eye.z;
    out.u[0] = u.x; out.u[1] = u.y; out.u[2] = u.z;
    out.v[0] = v.x; out.v[1] = v.y; out.v[2] = v.z;
    out.w[0] = w.x; out.w[1] = w.y; out.w[2] = w.z;
    out.top = top; out.right = right; out.bottom = -top; out.left = -right;
    out.W = W; out.H = H;
    out.aperture = c->aperture;
    out.focus = c->focus_plane;
    out.shutter = c->shutter_speed;
    return MRT_OK;
}

static void fill_params(const Scene& s, RenderParams& P) {
    const DeviceState& d = *s.dev;
    P.nodes = d.nodes; P.leaves = d.leaves; P.prims = d.prims; P.verts = d.verts; P.normals = d.normals;
    P.mats = d.mats; P.lights = d.lights; P.tables = d.tables; P.gamma = d.gamma;
    P.gammaF = d.gammaF;
    P.min_subdivs = s.min_subdivs;
    P.max_subdivs = s.max_subdivs;
    P.noise = s.noise_threshold;
    P.domes = d.domes;
    P.insts = d.insts;
    P.texs = d.texs;
    P.puv = d.puv;
    P.uvs = d.uvs;
    P.tans = d.tans;
    P.btans = d.btans;
    P.has_maps = d.has_maps ? 1 : 0;
    P.pflags = d.pflags;
    P.verts2 = d.verts2;
    P.has_mb = d.has_mb ? 1 : 0;
    P.n_insts = d.n_insts;
    P.n_world = d.n_world;
    P.env = d.env;
    P.env_w = d.env ? s.textures[s.env_tex].W : 0;
    P.env_h = d.env ? s.textures[s.env_tex].H : 0;
    P.env_exposure = s.env_exposure;
    P.gstride = d.gthreads;
    P.bg[0] = s.bg[0]; P.bg[1] = s.bg[1]; P.bg[2] = s.bg[2];
    P.n_lights = (int32_t)s.lights.size();
    P.num_paths = s.num_paths;
    P.path_trace = s.path_trace ? 1 : 0;
    P.max_bounces = s.max_bounces;
    P.sample_env = s.sample_env ? 1 : 0;
    P.mat_env = 0;
    for (const DevMaterial& m : s.materials) P.mat_env |= m.env >= 0 ? 1 : 0;
}

// The scene's hit ids (mrt_hit.prim of a hit) are [0, hit_id_count): the world objects, then
// every instance's BLAS objects in instance order (build_qbvh sets hit_base that way).
static int32_t hit_id_count(const Scene& s) {
    int64_t n = (int64_t)s.obj_mesh.size();
    if (!s.instances.empty()) {
        const Instance& I = s.instances.back();
        n = (int64_t)I.hit_base + (int64_t)s.blas[(size_t)I.blas].obj_mesh.size();
    }
    return (int32_t)std::min<int64_t>(n, INT32_MAX);
}

// The first record of a caller's host array that mrt_shade_hits / mrt_hit_surfaces refuse
// (the device's test, hit_record_usable, on the host scene), or n: before any device call.
static size_t first_bad_hit(const Scene& s, const mrt_hit* hits, size_t n, const char*& why) {
    const int32_t n_ids = hit_id_count(s), n_world = (int32_t)s.obj_mesh.size();
    for (size_t i = 0; i < n; i++) {
        const mrt_hit& h = hits[i];
        const int k = hit_record_class(h.t, h.a, h.b, h.prim, n_ids);
        if (k < 0) {
            why = (h.prim < -1 || h.prim >= n_ids) ? "prim outside the scene's hit ids" : "t, a or b not finite or out of range";
            return i;
        }
        if (k > 0 && h.prim < n_world && !s.obj_inst.empty() && s.obj_inst[(size_t)h.prim] >= 0) {
            why = "prim is a ProxyObject's own slot, which never hits";
            return i;
        }
    }
    return n;
}

// chain levels of the REC kernels: reflection / refraction bounces (< 5) plus
// the GI bounces (giBounces < m_maxBounces - 1)
static int chain_levels(const Scene& s) { return 6 + (s.path_trace ? s.max_bounces : 0); }
// words of a level record: reflect / refract 3; GI 12 + 3 per light; a
// dispersive split in the fused engine 26 + the IOR history (Shader::level)
static constexpr int kDispWords = 26 + kIorCap;
static int level_words(const Scene& s) {
    const int w = s.path_trace ? 12 + 3 * (int)s.lights.size() : 3;
    return s.dev && s.dev->disperse ? std::max(w, kDispWords) : w;
}

// Scratch groups of a stream context (reserve, mrt_device.h): its stream's last launch may still read them.
static int ensure_levels(StreamCtx& c, size_t floats) {
    return reserve(c.own, &c.stream, {{(void**)&c.lvl, floats * sizeof(float)}}, {{&c.lvl_cap, floats}});
}

static inline int fast_box(const DeviceState& d) { return (g_tune.fast_box && d.boxes_finite) ? 1 : 0; }

// wavefront shadow-ray buffers of a stream context
static int ensure_rays(StreamCtx& c, size_t slots, size_t per_slot) {
    const size_t n = slots * per_slot;
    return reserve(c.own, &c.stream, {{(void**)&c.rays, 2 * n * sizeof(float4)}, {(void**)&c.occl, n}, {(void**)&c.nrays, slots}},
                   {{&c.ray_cap, n}, {&c.nrays_cap, slots}});
}

// Dome-light replay scratch of a stream: n ray slots, calls call records.
static int ensure_replay(StreamCtx& c, size_t n, size_t calls) {
    return reserve(c.own, &c.stream, {{(void**)&c.ray_e, n * sizeof(float4)}, {(void**)&c.lrec, calls * sizeof(uint32_t)}},
                   {{&c.ray_e_cap, n}, {&c.lrec_cap, calls}});
}

// The binning switches in effect for a scene (tuning "bin", or the auto choice).
static int bin_mode(const DeviceState& d) {
    if (g_tune.bin >= 0) return g_tune.bin;
    return (d.recursive == 2 ? 6 : 0) | (d.n_insts > 0 && d.dome ? 5 : 0) | (d.disperse ? 4 : 0);
}

// Ray-binning scratch of a stream (mrt_bin.h) for batches of up to n rays.
static constexpr size_t kBinHist = (size_t(1) << kBinBits) + 64;   // bins + the valid count, padded
static int ensure_bin(StreamCtx& c, size_t n) {
    return reserve(c.own, &c.stream,
                   {{(void**)&c.bin_keys, n * sizeof(uint16_t)}, {(void**)&c.bin_perm, 2 * n * sizeof(uint32_t)},
                    {(void**)&c.bin_hist, 2 * kBinHist * sizeof(uint32_t)}},
                   {{&c.bin_cap, n}});
}

// Binning of a ray batch o[i] / d[i], i < n (host bound), into permutation
// `which` of the stream's scratch; keys from the scene box and the tuning
// knobs.  The caller sets the validity / device-count fields, then bins.
static BinArgs bin_args(const DeviceState& d, const StreamCtx& c, int which, const float4* o, const float4* dd, size_t n) {
    BinArgs A{};
    A.o = o; A.d = dd; A.n = (uint32_t)n;
    A.mul1 = 1; A.cap1 = 0xFFFFFFFFu; A.mul2 = 1; A.m = 1;
    A.dbits = g_tune.bin_dbits; A.obits = g_tune.bin_obits;
    for (int a = 0; a < 3; a++) {
        const float ext = d.bb_hi[a] - d.bb_lo[a];
        A.lo[a] = d.bb_lo[a];
        A.inv[a] = ext > 0.f ? (float)(1 << A.obits) / ext : 0.f;
    }
    A.keys = c.bin_keys;
    A.hist = c.bin_hist + (size_t)which * kBinHist;
    A.perm = c.bin_perm + (size_t)which * c.bin_cap;
    return A;
}
static const uint32_t* bin_total(const BinArgs& A) {
    return A.hist + (size_t(1) << (A.hits ? kBinBits : 2 * A.dbits + 3 * A.obits));
}
static int bin_grid(const DeviceState& d, size_t n) {   // fewer blocks: fewer per-bin global atomics
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)d.cus * (size_t)kBinBlocks, (n + 255) / 256));
}

static int ensure_slots(StreamCtx& c, size_t slots) {
    return reserve(c.own, &c.stream, {{(void**)&c.hitbuf, slots * sizeof(float4)}}, {{&c.hit_slots, slots}});
}

// Resident workgroups per CU of one kernel instantiation (occupancy API, cached).
// An over-estimate only queues blocks behind the resident ones: the tile
// schedule (sched 2/3) keeps late blocks useful.
static int blocks_per_cu(KernelFn f, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<const void*, size_t>, int> cache;
    std::lock_guard<std::mutex> g(mu);
    const auto key = std::make_pair(reinterpret_cast<const void*>(f), lds);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(f), kWG, lds) != hipSuccess) n = 1;
    n = std::max(1, std::min(n, kMaxBlocksPerCU));
    cache[key] = n;
    return n;
}

template <int W, bool I, bool CHK = true, bool X = false>
static KernelFn primary_fn(bool c, bool f) {
    return with_bools([](auto C, auto F) -> KernelFn { return primary_kernel<C(), W, F(), I, CHK, X>; }, c, f);
}
// check: the special-leaf scene has alpha-mapped or motion-blurred lanes; scenes with
// instances only take the variants without those tests (no noinline calls: C5's nested
// instance walk at 5 waves spills 28 B instead of 256 B per lane)
// xone: the one-exit walk loop (non-instanced scenes; the instanced walk keeps its exits:
// C5's primary launch measured 36% slower with one)
KernelFn pick_primary(int w, int inst_waves, bool c, bool f, bool inst, bool check, bool xone) {
    if (inst && !check) return with_ints<4, 6, 1, 5>(inst_waves, [&](auto W) { return primary_fn<W(), true, false>(c, f); });
    // special-leaf scenes (instances: nested BLAS walks); 4 waves: 128 VGPRs, the nested instance walk without spills
    if (inst) return with_ints<4, 5, 6, 1>(inst_waves, [&](auto W) { return primary_fn<W(), true>(c, f); });
    if (xone) return with_ints<6, 7, 8, 1>(w, [&](auto W) { return primary_fn<W(), false, true, true>(c, f); });
    return with_ints<6, 7, 8, 1>(w, [&](auto W) { return primary_fn<W(), false>(c, f); });
}
// kGen / kResolve: no traversal, FAST unused; special-leaf scenes take POINT_ONLY = false
// bound: the dome-light resolve pass at 4 waves (~240 VGPRs unbounded)
template <int MODE>
static KernelFn shade_mode_fn(bool c, bool po, bool inst, bool bound) {
    if (!c && MODE == kResolve && bound)
        // special-leaf scenes at 3 waves: 168 VGPRs and no scratch (152 B / 40 spills at 4 waves);
        // C5's resolve pass -0.7% (profiles/r06_c5_resolve_waves_ab.txt)
        return with_bools([](auto I, auto PO) -> KernelFn {
            return shade_kernel<false, PO() && !I(), false, I(), MODE, 0, I() ? 3 : 4>;
        }, inst, po);
    return with_bools([](auto I, auto PO, auto C) -> KernelFn { return shade_kernel<C(), PO() && !I(), false, I(), MODE>; }, inst, po, c);
}
// MINW: launch-bounds occupancy target of the timed (COUNT = false) variants
template <bool INST, bool REFILL, bool CHECK, int MINW = 1>
static ShadowFn shadow_fn(bool c, bool f) {
    return with_bools([](auto C, auto F) -> ShadowFn { return shadow_kernel<C(), F(), INST, REFILL, CHECK, C() ? 1 : MINW>; }, c, f);
}
// check: the scene has alpha-mapped or motion-blurred lanes (child-word bit 3), which the
// refill step must test as such
ShadowFn pick_shadow(bool c, bool f, bool inst, bool refill, bool check) {
    if (!refill) return inst ? shadow_fn<true, false, true>(c, f) : shadow_fn<false, false, false, 8>(c, f);
    if (!inst) return shadow_fn<false, true, false, 8>(c, f);
    return check ? shadow_fn<true, true, true>(c, f) : shadow_fn<true, true, false, 8>(c, f);
}
// shadow rays per pixel at most: num_paths x (1 per point light, m_numSamples per area / dome light)
static int max_shadow_rays(const Scene& s) {
    int per_path = 0;
    for (const DevLight& l : s.lights) per_path += l.type == MRT_POINT_LIGHT ? 1 : std::max(1, l.samples);
    return s.num_paths * per_path;
}

KernelFn pick_shade(bool c, bool po, bool f, bool inst, int rec) {
    if (rec) return pick_shade_rec(c, po, f, inst, rec);
    return shade_fn<0>(c, po, f, inst);
}
// the wavefront shadow passes 2a (gen) / 2c (resolve)
KernelFn pick_shade_mode(bool resolve, bool c, bool po, bool inst, bool bound) {
    if (!resolve) return shade_mode_fn<kGen>(c, po, inst, bound);
    return shade_mode_fn<kResolve>(c, po, inst, bound);
}

// The wavefront chain engine (mrt_chain.hip) for the shading of a REC scene:
// per chunk of work units (eye rays), level 0 of every path (gen, shadow rays,
// resolve), then per level compact / trace / gen / shadow rays / resolve, the
// per-level folds and the per-unit finish.  P holds the primary launch's
// parameters (hits, outputs, cameras, work items, or an adaptive pass's units);
// the chunks are sized so the per-level arrays fit g_tune.chain_mb.
static constexpr int kMaxChainLevels = 63;   // < the 64 level counts (level L's count stays 0)
// shadow rays one chain level of one path traces at most: every light's
// samples for the direct term, again for translucency, again for the last GI
// bounce (0: more than the u8 ray count holds -> fused kernel)
static int chain_shadow_rays(const Scene& s) {
    int per = 0;
    for (const DevLight& l : s.lights) per += l.type == MRT_POINT_LIGHT ? 1 : std::max(1, l.samples);
    bool tr = false;
    for (const DevMaterial& m : s.materials) tr |= m.type == MRT_BLINN && m.translucency > 0.01f;
    const int m = per * (1 + (tr ? 1 : 0) + (s.path_trace ? 1 : 0));
    return m <= 255 ? std::max(1, m) : 0;
}
// Entries of chain level k per path at most: one child per level, except a
// dispersive split's three (src/Blinn.cpp:275-301).  Split children are
// refraction rays, which do not split again, so splits are at least two levels
// apart: 3^ceil(k/2).  (Dispersion with path tracing -- GI levels without a
// bounce bound on splits -- stays on the fused kernel.)
static uint64_t level_mult(const Scene& s, int k) {
    uint64_t m = 1;
    if (s.dev->disperse)
        for (int i = 0; i < (k + 1) / 2; i++) m *= 3;
    return m;
}
// (Transparent shadows: the walk's answer is an attenuation, not the one bit the
// wavefront shadow passes carry -- such scenes shade in the fused kernels.)
static bool use_chain(const Scene& s) {
    return s.dev->recursive && g_tune.chain && chain_levels(s) <= kMaxChainLevels && chain_shadow_rays(s) > 0 &&
           !(s.dev->disperse && s.path_trace) && !s.dev->transparent;
}
// One chunk of the engine over units [Q.unit_base, Q.unit_base + Q.n_units) of
// Q's pass (the chunk layout -- ch_lofs, arrays -- is set by the caller).
static int chain_chunk(Scene& s, StreamCtx& c, RenderParams& Q, bool count, hipStream_t stream, size_t ctl,
                       unsigned int* queues) {
    DeviceState& d = *s.dev;
    const int L = Q.ch_levels;
    const bool inst = d.special;
    const bool rays = Q.mode == 2;   // a ray batch: the kernels' ray-mode instantiations
    const KernelFn g0 = pick_chain0(false, d.point_only, inst, d.recursive, rays),
                   r0 = pick_chain0(true, d.point_only, inst, d.recursive, rays);
    const KernelFn gk = pick_chain_shade(false, d.point_only, inst, d.recursive, rays),
                   rk = pick_chain_shade(true, d.point_only, inst, d.recursive, rays);
    const KernelFn kc = pick_chain_compact(), kt = pick_chain_trace(count, Q.fast_box != 0, inst,
                                                                           g_tune.chain_shadow_step ? (d.has_alpha || d.has_mb ? 2 : 1) : 0,
                                                                           rays),
                   kf = pick_chain_finish(rays), kd = pick_chain_fold();
    auto go = [&](KernelFn f, int g) -> int {
        void* args[] = {&Q};
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(f), dim3(std::max(1, g)), dim3(kWG), args, 0, stream));
        return MRT_OK;
    };
    auto full = [&](KernelFn f) { return std::min(d.grid, d.cus * blocks_per_cu(f, 0)); };
    const int ug = (int)std::min<uint64_t>((uint64_t)full(r0), ((uint64_t)Q.n_units + kWG - 1) / kWG);
    int rc;
    // ray binning before each trace launch (g_tune.bin bits 1 / 2): level k's closest-hit entries
    // and level k - 1's shadow rays, each in its own permutation
    const uint32_t m = (uint32_t)Q.max_shadow;
    auto lcap_h = [&](int k) { return (size_t)Q.ch_lofs[k + 1] - Q.ch_lofs[k]; };
    const int bm = bin_mode(d);
    if (bm & 6) {
        size_t need = 1;
        for (int k = 0; k < L; k++) need = std::max(need, std::max(lcap_h(k), lcap_h(k) * m));
        if ((rc = ensure_bin(c, need))) return rc;
    }
    // instanced scenes: the levels' shadow rays on the lane-refill kernel (their own launch)
    const bool refill_sh = inst && g_tune.chain_shadow_refill;
    const ShadowFn ksh = refill_sh ? pick_shadow(count, Q.fast_box != 0, true, true, d.has_alpha || d.has_mb) : nullptr;
    int gsh = refill_sh ? std::max(8, std::min(d.grid, d.cus * blocks_per_cu(reinterpret_cast<KernelFn>(ksh), 0))) & ~7 : 0;
    auto trace = [&](int k) -> int {   // Q.ch_level == k
        if ((bm & 2) && k < L) {
            const size_t lo = Q.ch_lofs[k], cap = lcap_h(k);
            BinArgs A = bin_args(d, c, 1, Q.ch_ray + 2 * lo, Q.ch_ray + 2 * lo + cap, cap);
            A.n_dev = Q.ch_cnt + k;
            int r2;
            if ((r2 = bin_rays(A, bin_grid(d, cap), stream))) return r2;
            Q.tr_perm = A.perm;
        }
        if (bm & 4) {
            const size_t lo = Q.ch_lofs[k - 1], nb = lcap_h(k - 1) * m;
            BinArgs B = bin_args(d, c, 0, Q.ray_o + lo * m, Q.ray_d + lo * m, nb);
            B.nrays = Q.nrays + lo;
            B.m = m;
            if (k - 1 > 0) {
                B.n_dev = Q.ch_cnt + (k - 1);
                B.mul2 = m;
            } else if (Q.unit_cnt) {   // adaptive pass: chunk_units on the device
                B.n_dev = Q.unit_cnt;
                B.mul1 = Q.adapt_n > 1 ? (uint32_t)(Q.adapt_n * Q.adapt_n) : 1u;
                B.sub = Q.unit_base;
                B.cap1 = Q.n_units;
                B.mul2 = (uint32_t)Q.num_paths * m;
            } else {
                const uint32_t units = Q.units_total > Q.unit_base ? std::min(Q.n_units, Q.units_total - Q.unit_base) : 0u;
                B.n = (uint32_t)std::min<uint64_t>(nb, (uint64_t)units * (uint64_t)Q.num_paths * m);
            }
            int r2;
            if ((r2 = bin_rays(B, bin_grid(d, nb), stream))) return r2;
            Q.sh_perm = B.perm;
            Q.sh_perm_n = bin_total(B);
        }
        int r3 = MRT_OK;
        if (refill_sh) {
            // instanced scenes: level k - 1's shadow rays on the lane-refill any-hit kernel
            // (shadow_kernel sched 2: a finished lane takes the next ray, proxy lanes deferred
            // onto the stack), the entries' closest hits in chain_trace below.  Same rays,
            // same answers; level 0's ray counts of units past the chunk are zeroed at its start.
            RenderParams S = Q;
            const size_t sbase = (size_t)Q.ch_lofs[k - 1] * m;
            S.ray_o = Q.ray_o + sbase;
            S.ray_d = Q.ray_d + sbase;
            S.occl = Q.occl + sbase;
            S.nrays = Q.nrays + Q.ch_lofs[k - 1];
            S.sh_count = k - 1 > 0 ? Q.ch_cnt + (k - 1) : nullptr;
            S.near_first = 0;
            S.queue = queues + (size_t)(L + 2 + k) * 256;
            size_t n_rays = lcap_h(k - 1) * m;
            int sched = 2, refill = kRefillMin;
            void* sargs[] = {&S, &n_rays, &sched, &refill};
            r3 = MRT_OK;
            if (hipLaunchKernel(reinterpret_cast<const void*>(ksh), dim3(gsh), dim3(kWG), sargs, 0, stream) != hipSuccess) {
                set_error("chain shadow launch"); r3 = MRT_ERR_HIP;
            }
            Q.ch_skip_shadow = 1;
        }
        if (r3 == MRT_OK) r3 = go(kt, full(kt));
        Q.ch_skip_shadow = 0;
        Q.tr_perm = nullptr;
        Q.sh_perm = nullptr;
        Q.sh_perm_n = nullptr;
        return r3;
    };
    HIP_OK(hipMemsetAsync(Q.ch_cnt, 0, ctl, stream));
    if (refill_sh) HIP_OK(hipMemsetAsync(Q.nrays + Q.ch_lofs[0], 0, lcap_h(0), stream));   // level 0: only live units' counts
    Q.queue = queues;
    if (Q.uhits) {   // adaptive pass: the chunk's eye rays and their closest hits (counted in the frame's
                     // statistics: they run before any level can outgrow its capacity)
        const KernelFn ke = pick_unit_eye(count, Q.fast_box != 0, inst);
        unsigned long long* cc = Q.ctr;
        Q.ctr = Q.ctr_out;
        rc = go(ke, (int)std::min<uint64_t>((uint64_t)full(ke), ((uint64_t)Q.n_units + kWG - 1) / kWG));
        Q.ctr = cc;
        if (rc) return rc;
    }
    Q.ch_level = 0;
    if ((rc = go(g0, ug))) return rc;                 // level 0: shadow rays + children
    for (int k = 0; k + 1 < L; k++) {
        Q.ch_level = k;
        if ((rc = go(kc, full(kc)))) return rc;        // children of level k -> entries of level k + 1
        Q.ch_level = k + 1;
        if ((rc = trace(k + 1))) return rc;            // their closest hits + level k's shadow rays
        if ((rc = go(gk, full(gk)))) return rc;        // level k + 1: shadow rays + children
    }
    Q.ch_level = L;
    if ((rc = trace(L))) return rc;                    // the last level's shadow rays
    Q.queue = queues + 256;
    if ((rc = go(r0, ug))) return rc;                  // resolve level 0, then levels 1 .. L - 1
    if ((rc = go(rk, full(rk)))) return rc;
    for (int k = L - 2; k >= 0; k--) {                 // fold the values up, deepest level first
        Q.ch_level = k;
        if ((rc = go(kd, full(kd)))) return rc;
    }
    if ((rc = go(kf, ug))) return rc;                  // per unit: paths averaged, pixel / unit colour
    // the chunk's statistics and capacity counts; a chunk that outgrew a level: its units again,
    // fused (counted in the frame's statistics directly)
    void* margs[] = {&Q};
    HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(pick_chain_merge()), dim3(1), dim3(64), margs, 0, stream));
    const KernelFn kfb = pick_chain_fallback(d.point_only, inst, d.recursive, count, rays);
    unsigned long long* cc = Q.ctr;
    Q.ctr = Q.ctr_out;
    rc = go(kfb, std::min(full(kfb), ug));
    Q.ctr = cc;
    return rc;
}

// The chain engine over a pass of `units_max` units (at most; the adaptive
// passes' counts live on the device): the scratch layout for `per_chunk`
// units, then the chunks.
static constexpr int kEstPasses = 17;   // capacity estimates: pass index 0 (no supersampling), 1 .. 16
static int launch_chain(Scene& s, StreamCtx& c, const RenderParams& P0, bool count, hipStream_t stream,
                        uint64_t units_max, int unit_align) {
    DeviceState& d = *s.dev;
    const int L = chain_levels(s), W = level_words(s), m = chain_shadow_rays(s), split = d.disperse ? 3 : 1;
    const uint64_t np = (uint64_t)P0.num_paths;
    // Level capacities in entries per path x 65536.  Worst case: level k holds 3^ceil(k/2)
    // entries per path where dispersive splits can occur, else one.  With chain_est, a level
    // this stream has seen (this pass index) gets the largest count per path any chunk needed
    // x chain_est_pct + 1/32: a chunk that outgrows it sets ch_ovf, its remaining launches
    // return at once and chain_fallback renders its units with the fused chain shading --
    // the same frame, at the fused kernel's speed for that chunk only.
    const int pi = std::min(P0.adapt_n, kEstPasses - 1);
    if (g_tune.chain_est && !c.est_dev) {
        int rc;
        if ((rc = c.own.alloc(c.est_dev, kEstPasses * 64 * sizeof(uint32_t)))) return rc;
        HIP_OK(hipMemsetAsync(c.est_dev, 0, kEstPasses * 64 * sizeof(uint32_t), stream));
        if ((rc = c.own.pinned(c.est_pinned, kEstPasses * 64 * sizeof(uint32_t))) ||
            (rc = c.own.event(c.est_ev, hipEventDisableTiming)))
            return rc;
        c.est.assign(kEstPasses * 64, 0u);
    }
    if (c.est_pending && hipEventQuery(c.est_ev) == hipSuccess) {   // the last copy has landed: no wait
        std::copy(c.est_pinned, c.est_pinned + kEstPasses * 64, c.est.begin());
        c.est_pending = false;
    }
    std::vector<uint64_t> capr(L);
    uint64_t capr_sum = 0, capr_max = 0;
    for (int k = 0; k < L; k++) {
        const uint64_t worst = level_mult(s, k) << 16;
        uint64_t r = worst;
        const uint32_t e = g_tune.chain_est && k > 0 ? c.est[(size_t)pi * 64 + k] : 0u;
        if (e != 0u && e != 0xFFFFFFFFu) r = std::min(worst, (uint64_t)(e - 1) * (uint64_t)g_tune.chain_est_pct / 100 + 2048);
        capr[k] = r;
        capr_sum += r;
        capr_max = std::max(capr_max, r);
    }
    // per path over all levels: ray + ior 2 x 32 B, hit 16, value 16, record 4 W, child map 4 split,
    // shadow rays m x (32 B + occlusion byte) + ray count; sparse spawn slots 65 B x split x the widest level
    const uint64_t entry_bytes = 32 + 32 + 16 + 16 + 4 * (uint64_t)W + 4 * (uint64_t)split + (uint64_t)m * 33 + 1;
    const uint64_t path_bytes = (capr_sum * entry_bytes + capr_max * (uint64_t)split * 65 + 65535) >> 16;
    const uint64_t unit_bytes = np * path_bytes + (P0.adapt_n ? 16 : 0);
    uint64_t budget = (uint64_t)g_tune.chain_mb << 20;
    size_t mem_free = 0, mem_total = 0;   // this stream's current chunk can be reused: count it as free
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) {
        budget = std::min<uint64_t>(budget, ((uint64_t)mem_free + c.chain_bytes) / 5 * 4);
        // every stream of this scene may hold a chunk at once: each gets at most its share of 80% of the
        // device (frames in flight on 4 streams cannot claim the whole device between them)
        size_t live = 1;
        {
            std::lock_guard<std::mutex> g(d.mu);
            live = std::max<size_t>(1, d.ctxs.size());
        }
        budget = std::min<uint64_t>(budget, (uint64_t)mem_total / 5 * 4 / live);
    }
    c.chain_budget = budget;
    uint64_t per = std::max<uint64_t>(1, budget / unit_bytes);
    per = std::max<uint64_t>(unit_align, per / unit_align * unit_align);
    per = std::min<uint64_t>(per, (units_max + unit_align - 1) / unit_align * unit_align);
    const uint64_t paths = per * np;
    std::vector<uint64_t> lcap(L);
    uint64_t entries = 0, lmax = 0;
    for (int k = 0; k < L; k++) {
        // whole 64-entry groups: every array's level slice stays aligned (the u64 statistics
        // after the maps need 8-byte alignment) and a wave's 64 entries share a group
        lcap[k] = k == 0 ? paths : std::max<uint64_t>(64, (((paths * capr[k] + 65535) >> 16) + 63) / 64 * 64);
        entries += lcap[k];
        lmax = std::max(lmax, lcap[k]);
    }
    const uint64_t spcap = lmax * (uint64_t)split;
    if (entries * (uint64_t)m >= (uint64_t(1) << 32) || spcap >= (uint64_t(1) << 32)) {
        set_error("chain chunk too large"); return MRT_ERR_INVALID;
    }
    int rc;
    if ((rc = ensure_rays(c, entries, (size_t)m))) return rc;   // every level keeps its shadow rays
    // layout: ray | ior (2 per entry) | hit | val | spawn (4 per slot) | uhits (float4), rec (float),
    // map (u32), control (counts, trace + resolve + chain shadow-launch queues, the chunk's
    // statistics, its overflow flag), flag (u8)
    const size_t ctl_q = 256 + (size_t)(2 * L + 3) * 1024;
    const size_t ctl = ctl_q + 256 + 64;
    const uint64_t n4 = 2 * entries + 2 * entries + entries + entries + 4 * spcap + (P0.adapt_n ? per : 0);
    const uint64_t bytes = n4 * 16 + entries * (uint64_t)W * 4 + entries * (uint64_t)split * 4 + ctl + spcap;
    if ((rc = reserve(c.own, &c.stream, {{&c.chain, (size_t)bytes}}, {{&c.chain_bytes, (size_t)bytes}}))) return rc;
    RenderParams Q = P0;
    float4* f4 = static_cast<float4*>(c.chain);
    Q.ch_ray = f4; f4 += 2 * entries;
    Q.ch_ior = f4; f4 += 2 * entries;
    Q.ch_hit = f4; f4 += entries;
    Q.ch_val = f4; f4 += entries;
    Q.ch_sp = f4; f4 += 4 * spcap;
    Q.uhits = P0.adapt_n ? f4 : nullptr; f4 += P0.adapt_n ? per : 0;
    Q.ch_rec = reinterpret_cast<float*>(f4);
    Q.ch_map = reinterpret_cast<uint32_t*>(Q.ch_rec + entries * (uint64_t)W);
    Q.ch_cnt = Q.ch_map + entries * (uint64_t)split;           // 64 counts, then L + 2 queues
    unsigned int* queues = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(Q.ch_cnt) + 256);
    Q.ctr_out = P0.ctr;
    Q.ctr = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(Q.ch_cnt) + ctl_q);
    Q.ch_ovf = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(Q.ch_cnt) + ctl_q + 256);
    Q.ch_est = g_tune.chain_est ? c.est_dev + (size_t)pi * 64 : nullptr;
    if (reinterpret_cast<uintptr_t>(Q.ctr) % 8 != 0) { set_error("chain layout misaligned"); return MRT_ERR_INVALID; }
    Q.ch_flag = reinterpret_cast<uint8_t*>(Q.ch_cnt) + ctl;
    Q.ch_spcap = (uint32_t)spcap;
    Q.ch_split = split;
    Q.ch_levels = L;
    uint64_t off = 0;
    for (int k = 0; k <= L; k++) {
        Q.ch_lofs[k] = (uint32_t)off;
        if (k < L) off += lcap[k];
    }
    Q.lvl_words = W;
    Q.ch_bands = g_tune.chain_bands > 0 || (g_tune.chain_bands < 0 && (bin_mode(d) & 6));
    Q.wave_log = nullptr;
    Q.ray_o = c.rays;
    Q.ray_d = c.rays + entries * (uint64_t)m;
    Q.occl = c.occl;
    Q.nrays = c.nrays;
    Q.max_shadow = m;
    Q.n_units = (uint32_t)per;
    c.chain_chunks += (uint32_t)((units_max + per - 1) / per);
    for (uint64_t b = 0; b < units_max; b += per) {
        Q.unit_base = (uint32_t)b;
        if ((rc = chain_chunk(s, c, Q, count, stream, ctl, queues))) return rc;
    }
    if (g_tune.chain_est) {   // this pass's estimates to the host, read by a later frame once they have landed
        HIP_OK(hipMemcpyAsync(c.est_pinned, c.est_dev, kEstPasses * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipEventRecord(c.est_ev, stream));
        c.est_pending = true;
    }
    return MRT_OK;
}

// Adaptive supersampling of a REC scene on the chain engine: passes n = 1 ..
// max_subdivs over the pixels still refining (each pass: the units' eye rays,
// the chain engine, then adapt_combine's running mean + stop test, which lists
// the next pass's pixels or writes the pixel).
static int launch_chain_adaptive(Scene& s, StreamCtx& c, RenderParams& P, bool count, hipStream_t stream) {
    DeviceState& d = *s.dev;
    const uint64_t lanes = (uint64_t)P.n_tiles * 64;   // pixels of the frame / batch (work-item lanes)
    const int maxs = std::max(P.min_subdivs, P.max_subdivs);
    // per stream: running means, two pixel lists + counts, unit colours of the largest pass
    const uint64_t ucol_n = lanes * (uint64_t)maxs * (uint64_t)maxs;
    const uint64_t bytes = lanes * 16 + 2 * lanes * 4 + 256 + ucol_n * 16;
    int cur = 0, rc;
    if ((rc = reserve(c.own, &c.stream, {{&c.adapt, (size_t)bytes}}, {{&c.adapt_bytes, (size_t)bytes}}))) return rc;
    float4* res = static_cast<float4*>(c.adapt);
    float4* ucol = res + lanes;
    uint32_t* lists = reinterpret_cast<uint32_t*>(ucol + ucol_n);
    uint32_t* cnts = lists + 2 * lanes;   // 2 counts (own 256 B)
    P.adapt_res = res;
    P.ucol = ucol;
    const KernelFn kcomb = pick_adapt_combine();
    for (int n = 1; n <= maxs; n++) {
        const int nxt = cur ^ 1;
        P.adapt_n = n;
        P.units = n == 1 ? nullptr : lists + (size_t)cur * lanes;
        P.unit_cnt = n == 1 ? nullptr : cnts + cur;
        P.units_total = (uint32_t)lanes;
        P.next_units = lists + (size_t)nxt * lanes;
        P.next_cnt = cnts + nxt;
        HIP_OK(hipMemsetAsync(cnts + nxt, 0, 4, stream));
        if ((rc = launch_chain(s, c, P, count, stream, lanes * (uint64_t)n * (uint64_t)n, 64))) return rc;
        void* args[] = {&P};
        const int g = std::min<int>(d.grid, (int)((lanes + kWG - 1) / kWG));
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(kcomb), dim3(std::max(1, g)), dim3(kWG), args, 0, stream));
        cur = nxt;
    }
    return MRT_OK;
}

// The bracket of a query that is not a render (trace_async, hit_surfaces_async): the stream's
// context with `ctr_bytes` of its counters cleared and ev0 recorded; then the caller's launch;
// then end_launch.
static int begin_query(Scene& s, DeviceState& d, hipStream_t stream, size_t ctr_bytes, bool supplied, StreamCtx*& c) {
    if (const int rc = get_ctx(d, stream, c)) return rc;
    s.stats_final = false;
    HIP_OK(hipMemsetAsync(c->ctr, 0, ctr_bytes, stream));
    c->last_was_render = false;
    c->supplied = supplied;
    HIP_OK(hipEventRecord(c->ev0, stream));
    return MRT_OK;
}
// after the last launch of a render or a query: its launch error, ev1, and c is what the statistics read
static int end_launch(DeviceState& d, StreamCtx& c, hipStream_t stream) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c.ev1, stream));
    d.last = &c;
    return MRT_OK;
}

// Two launches on `stream`: primary rays -> hit records, then shading with
// shadow rays.  Events bracket both (kernel_ms covers the whole frame).  With
// adaptive supersampling (subdivs > 1) one fused launch (kernel 3) instead.
// supplied (ray mode only, mrt_shade_hits): the caller's hit records, one per ray -- the
// primary launch is replaced by their conversion into the stream's hitbuf.
static int launch_render(Scene& s, RenderParams& P, size_t slots, bool count, hipStream_t stream, bool want_hits,
                         const mrt_hit* supplied = nullptr) {
    DeviceState& d = *s.dev;
    StreamCtx* cp = nullptr;
    int rc = get_ctx(d, stream, cp);
    if (rc) return rc;
    StreamCtx& c = *cp;
    s.stats_final = false;
    c.supplied = supplied != nullptr;
    if ((rc = ensure_slots(c, slots))) return rc;
    if (d.recursive) {
        P.lvl_words = level_words(s);
        if ((rc = ensure_levels(c, (size_t)d.gthreads * chain_levels(s) * P.lvl_words))) return rc;
        P.lvl = c.lvl;
    }
    P.hits = c.hitbuf;
    P.gstack = c.gstack;
    P.ctr = c.ctr;
    P.fast_box = fast_box(d);
    P.sched = g_tune.sched;
    P.cus = d.cus;
    P.scalar_nodes = g_tune.scalar_nodes & (d.boxes_ordered ? 7 : 3);
    P.near_first = g_tune.near_first > 0 ? 1 : 0;
    c.chain_chunks = 0;
    c.chain_budget = 0;
    const bool inst = d.special;   // instances or alpha maps: the special-leaf kernels
    const bool adaptive = P.min_subdivs > 1 || P.max_subdivs > 1;
    const bool one = g_tune.shade1 && d.point_only && P.n_lights == 1 && P.num_paths == 1 && !P.env && !inst && !d.recursive &&
                     !d.has_maps;
    const size_t log_stride = (size_t)d.grid * (kWG / 64) * kLogWords;
    const bool logw = count || g_tune.wave_log;   // wave log: count mode, or timing-only on the timed kernels
    HIP_OK(hipMemsetAsync(c.ctr, 0, kCtrBytes, stream));
    unsigned int* qbase = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c.ctr) + CTR_N * sizeof(unsigned long long));
    P.queue = qbase;
    // workgroups: at most one per 4 tiles (a tile per wave); bucket batches (P.mode 1) may ask for
    // g_tune.batch_tpw tiles per wave, so a small share's waves take several tiles each
    const int tpw = P.mode == 1 ? g_tune.batch_tpw : 1;
    const int items = (int)(((int64_t)P.n_tiles + 4 * tpw - 1) / (4 * tpw));
    if (logw) HIP_OK(hipMemsetAsync(c.wave_log, 0, 2 * log_stride * sizeof(unsigned long long), stream));
    int which = 0;
    auto launch = [&](KernelFn f) -> int {
        const int g = std::max(1, std::min(std::min(d.grid, d.cus * blocks_per_cu(f, 0)), items));
        P.wave_log = logw && which < 2 ? c.wave_log + which * log_stride : nullptr;  // primary + first shade
        P.n_waves = g * (kWG / 64);
        if (logw && which < 2) c.log_waves[which] = g * (kWG / 64);
        which++;
        void* args[] = {&P};
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(f), dim3(g), dim3(kWG), args, 0, stream));
        return MRT_OK;
    };
    // every path ends here, after its last launch (and its evm record)
    auto done = [&]() -> int {
        c.last_was_render = true;
        if (const int r = end_launch(d, c, stream)) return r;
        s.last = mrt_stats{};
        return MRT_OK;
    };
    HIP_OK(hipEventRecord(c.ev0, stream));
    const bool fb = P.fast_box != 0;
    c.chain_used = false;
    if (adaptive) {
        HIP_OK(hipEventRecord(c.evm, stream));   // primary_ms = 0: one launch
        P.refill_min = g_tune.adapt_refill;
        if (use_chain(s)) {     // secondary rays: passes over the chain engine
            c.chain_used = true;
            if ((rc = launch_chain_adaptive(s, c, P, count, stream))) return rc;
        } else if ((rc = launch(pick_adaptive(count, d.point_only, fb, inst, d.recursive)))) {
            return rc;
        }
        return done();
    }
    c.fused = one && g_tune.fused && P.mode != 2;   // a ray batch: the two-launch path (frame1_kernel makes its own rays)
    if (c.fused) {   // one launch: camera rays, closest hits, shading, shadow rays
        if (!want_hits) P.hits = nullptr;
        // LDS top-node walk (tuning "lds_nodes"; both walks give the same bits)
        const bool ln = fb && d.lds_ok && g_tune.lds_nodes > 0;
        d.lds_pick = ln ? 1 : 0;
        const int walk = ln ? 2 : g_tune.walk_exit == 0 ? 0 : g_tune.walk_latch ? 3 : 1;
        if ((rc = launch(pick_frame1(g_tune.frame1_waves, count, fb, d.pow_spec, walk)))) return rc;
        HIP_OK(hipEventRecord(c.evm, stream));
        return done();
    }
    const bool chk = d.has_alpha || d.has_mb;
    const bool rays = P.mode == 2;   // a ray batch: the kernels' ray-mode instantiations
    if (supplied) {   // the caller's hits into hitbuf: no primary rays
        const int g = (int)std::max<size_t>(1, std::min<size_t>((slots + 255) / 256, (size_t)d.cus * 8));
        hipLaunchKernelGGL(hit_supply_kernel, dim3(g), dim3(256), 0, stream, supplied, slots, (int32_t)d.n_world,
                           hit_id_count(s), d.prims, c.hitbuf, c.ctr);
        HIP_OK(hipGetLastError());
        which = 1;   // the wave log's primary record stays empty
    } else if ((rc = launch(rays ? pick_primary_rays(count, fb, inst, chk, g_tune.walk_exit == 1)
                                 : pick_primary(g_tune.primary_waves, g_tune.primary_inst_waves, count, fb, inst, chk,
                                                g_tune.walk_exit == 1)))) {
        return rc;
    }
    HIP_OK(hipEventRecord(c.evm, stream));
    P.queue = qbase + 8 * 32;
    const int max_sh = max_shadow_rays(s);
    // secondary rays and their shadow rays depend on hits along the path: fused kernel
    const bool wave = !one && g_tune.wavefront && max_sh > 0 && max_sh <= kMaxWaveShadow && !d.recursive && !d.transparent;
    if (use_chain(s)) {
        c.chain_used = true;
        P.units = nullptr;
        P.unit_cnt = nullptr;
        P.adapt_n = 0;
        P.units_total = (uint32_t)P.n_tiles * 64u;
        if ((rc = launch_chain(s, c, P, count, stream, (uint64_t)P.n_tiles * 64, 64))) return rc;
    } else if (one || !wave) {
        if ((rc = launch(one    ? pick_shade1(count, fb, d.pow_spec, rays)
                         : rays ? pick_shade_rays(count, d.point_only, fb, inst, d.recursive)
                                : pick_shade(count, d.point_only, fb, inst, d.recursive))))
            return rc;
    } else {
        if ((rc = ensure_rays(c, slots, (size_t)max_sh))) return rc;
        P.ray_o = c.rays;
        P.ray_d = c.rays + slots * (size_t)max_sh;
        P.occl = c.occl;
        P.nrays = c.nrays;
        P.max_shadow = max_sh;
        int ndome = 0;
        for (const DevLight& l : s.lights) ndome += l.type == MRT_DOME_LIGHT ? 1 : 0;
        const bool dome = ndome > 0;
        if (dome && g_tune.dome_replay) {   // 2a records the dome samples, 2c replays them
            P.lcalls = P.num_paths * ndome;
            if ((rc = ensure_replay(c, slots * (size_t)max_sh, slots * (size_t)P.lcalls))) return rc;
            P.ray_e = c.ray_e;
            P.lrec = c.lrec;
        }
        if ((rc = launch(rays ? pick_shade_mode_rays(false, count, d.point_only, inst)
                              : pick_shade_mode(false, count, d.point_only, inst, false))))
            return rc;
        // lane refill for dome-light (incoherent) rays: D1 -7%, C5 -13% shade pass; coherent
        // area-light rays keep the bands (C4: refill +9%)
        int sched = g_tune.shadow_sched >= 0 ? g_tune.shadow_sched : (dome ? 2 : 1), refill = kRefillMin;
        ShadowFn sf = pick_shadow(count, fb, inst, sched == 2, d.has_alpha || d.has_mb);
        int g = std::max(1, std::min(d.grid, d.cus * blocks_per_cu(reinterpret_cast<KernelFn>(sf), 0)));
        if (sched && (g & 7)) g &= ~7;          // XCD bands need a whole number of workgroups per XCD
        if (g < 8) {                            // too few workgroups for the bands: grid-stride
            sched = 0;
            sf = pick_shadow(count, fb, inst, false, d.has_alpha || d.has_mb);
        }
        size_t n_rays = slots * (size_t)max_sh;
        if (n_rays >= (size_t(1) << 32)) { set_error("too many wavefront shadow-ray slots (2^32)"); return MRT_ERR_INVALID; }
        P.near_first = g_tune.near_first >= 0 ? g_tune.near_first : (sched == 2 || inst ? 0 : 1);
        if (bin_mode(d) & 1) {   // the rays in binned order (valid slots only)
            if ((rc = ensure_bin(c, n_rays))) return rc;
            BinArgs A = bin_args(d, c, 0, P.ray_o, P.ray_d, n_rays);
            A.nrays = P.nrays;
            A.m = (uint32_t)max_sh;
            if (g_tune.bin_inst && d.n_insts > 0 && A.dbits == 2 && A.obits == 2) {   // instance-major keys
                A.hits = P.hits;
                A.hit_base = d.inst_hit_base;
                A.inst_class = d.inst_class;
                A.inst_cell = g_tune.bin_inst == 2 ? d.inst_cell : nullptr;   // 2: object-space cells
                A.insts = d.insts;
                A.n_inst = d.n_insts;
                A.n_world = d.n_world;
            }
            if ((rc = bin_rays(A, bin_grid(d, n_rays), stream))) return rc;
            P.sh_perm = A.perm;
            P.sh_perm_n = bin_total(A);
        }
        void* args[] = {&P, &n_rays, &sched, &refill};
        P.wave_log = nullptr;
        P.queue = qbase + 24 * 32;
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(sf), dim3(g), dim3(kWG), args, 0, stream));
        P.sh_perm = nullptr;
        P.sh_perm_n = nullptr;
        P.queue = qbase + 16 * 32;
        // dome-light resolve passes run faster at 4 waves (D1 -4%, C5 -1.2 ms), the rect-light one not (C4 +2%)
        if ((rc = launch(rays ? pick_shade_mode_rays(true, count, d.point_only, inst)
                              : pick_shade_mode(true, count, d.point_only, inst, dome))))
            return rc;
        P.ray_e = nullptr;
        P.lrec = nullptr;
        P.lcalls = 0;
    }
    return done();
}

}  // namespace mrt

using namespace mrt;

// ================================================================== C ABI (device side; the rest: host_api.cpp)
// What the entries share:
//   current_replica   the scene's current replica (device 0 before the first upload), made current
//   ray_args_check    the argument checks of the caller-ray entries, before any device call
//   Staged            the device copies of a synchronous entry's host arrays: a DevOwner, freed when it returns
//   begin_query / end_launch (above launch_render)   the bracket of a launch that is not a render
//   frame_params, seed_or_default, ensure_frame      one-camera frame setup
// A synchronous entry is: checks, current_replica, stage in, its async body, copy out, its own
// closing status.
static int current_replica(Scene& S, DeviceState*& d) {
    const int dev = S.dev ? S.dev->device : 0;
    if (const int rc = ensure_device(S, dev)) return rc;
    HIP_OK(hipSetDevice(dev));
    d = S.dev;
    return MRT_OK;
}

static constexpr size_t kMaxRayBatch = size_t(1) << 28;
static bool any_null(std::initializer_list<const void*> a) { return std::find(a.begin(), a.end(), nullptr) != a.end(); }
// `need`: the arrays an entry requires when n > 0, `what` names them ("null <what> array");
// row_width: 0 from an entry that has none
static int ray_args_check(const mrt_scene* s, size_t n, int32_t row_width, std::initializer_list<const void*> need,
                          const char* what) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    if (n && any_null(need)) { set_error(std::string("null ") + what + " array"); return MRT_ERR_INVALID; }
    if (row_width < 0) { set_error("row_width must be >= 0"); return MRT_ERR_INVALID; }
    if (n > kMaxRayBatch) { set_error("at most 2^28 rays per batch"); return MRT_ERR_INVALID; }
    if (!s->impl.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    return MRT_OK;
}

// One allocation per array per call; after a failure (rc) every further call does nothing.
struct Staged : DevOwner {
    int rc = MRT_OK;
    template <typename T> T* out(size_t bytes) {
        T* p = nullptr;
        if (rc == MRT_OK) rc = alloc(p, bytes);
        return p;
    }
    template <typename T> T* in(const T* host, size_t bytes) {   // a null host array stays null
        T* p = host ? out<T>(bytes) : nullptr;
        if (p) rc = copy(p, host, bytes, hipMemcpyHostToDevice);
        return p;
    }
    int back(void* host, const void* dev, size_t bytes) { return copy(host, dev, bytes, hipMemcpyDeviceToHost); }
private:
    static int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        HIP_OK(hipMemcpy(dst, src, bytes, kind)); return MRT_OK;
    }
};

static uint32_t seed_or_default(uint32_t seed) { return seed ? seed : 0x5EEDu; }

// the parameters of a one-camera frame: tiles of 8x8 pixels
static int frame_params(const Scene& S, const mrt_camera* cam, const mrt_render_opts* opts, RenderParams& P) {
    fill_params(S, P);
    if (const int rc = host_camera(cam, opts->width, opts->height, P.cam[0])) return rc;
    P.seed = seed_or_default(opts->seed);
    P.mode = 0;
    P.tiles_x = (opts->width + 7) / 8;
    P.n_tiles = P.tiles_x * ((opts->height + 7) / 8);
    return MRT_OK;
}

// the replica's frame buffers of the synchronous renders hold px pixels; drain: what may still read the old ones
static int ensure_frame(DeviceState& d, size_t px, const hipStream_t* drain) {
    return reserve(d.own, drain, {{(void**)&d.d_rgb, px * 12}, {(void**)&d.d_rgb8, px * 3}}, {{&d.frame_px, px}});
}

extern "C" {

int mrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mrt_scene_destroy(mrt_scene* s) {
    if (!s) return;
    free_replicas(s->impl);
    delete s;
}

int mrt_scene_upload(mrt_scene* s, int device) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    return ensure_device(s->impl, device);
}

int mrt_render_frame_async(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts, float* d_rgb,
                           uint8_t* d_rgb8, void* stream) {
    if (!s || !cam || !opts || !d_rgb) { set_error("bad argument"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    int rc = ensure_device(S, opts->device);
    if (rc) return rc;
    HIP_OK(hipSetDevice(opts->device));
    RenderParams P{};
    if ((rc = frame_params(S, cam, opts, P))) return rc;
    P.out_rgb = d_rgb;
    P.out_rgb8 = d_rgb8;
    rc = launch_render(S, P, (size_t)opts->width * opts->height, opts->count_visits != 0, (hipStream_t)stream,
                       opts->want_hits != 0);
    S.last.primary_rays = (uint64_t)opts->width * opts->height;
    return rc;
}

static int render_batch(mrt_scene* s, const mrt_camera* cams, int32_t n_cams, const mrt_render_opts* opts,
                        const int32_t* d_items, int32_t n_items, float* d_out, uint8_t* d_out8, void* stream,
                        bool frame_out) {
    if (!s || !cams || !opts || n_items < 0 || (n_items && !d_items) || (!d_out && !d_out8)) {
        set_error("bad argument"); return MRT_ERR_INVALID;
    }
    if (n_cams < 1 || n_cams > kMaxBatch) { set_error("n_cams must be 1..16"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    int rc = ensure_device(S, opts->device);
    if (rc) return rc;
    HIP_OK(hipSetDevice(opts->device));
    RenderParams P{};
    fill_params(S, P);
    for (int f = 0; f < n_cams; f++)
        if ((rc = host_camera(cams + f, opts->width, opts->height, P.cam[f]))) return rc;
    P.seed = seed_or_default(opts->seed);
    P.mode = 1;
    P.frame_out = frame_out ? 1 : 0;
    P.buckets = d_items;
    P.buckets_x = (opts->width + 31) / 32;
    P.buckets_per_frame = P.buckets_x * ((opts->height + 31) / 32);
    P.n_cams = n_cams;
    P.n_tiles = n_items * 16;
    P.out_rgb = d_out;
    P.out_rgb8 = d_out8;
    if (n_items == 0) return MRT_OK;
    rc = launch_render(S, P, (size_t)n_items * 1024, opts->count_visits != 0, (hipStream_t)stream, opts->want_hits != 0);
    S.last.primary_rays = 0;
    return rc;
}

int mrt_render_batch_async(mrt_scene* s, const mrt_camera* cams, int32_t n_cams, const mrt_render_opts* opts,
                           const int32_t* d_items, int32_t n_items, float* d_tiles, uint8_t* d_tiles8, void* stream) {
    return render_batch(s, cams, n_cams, opts, d_items, n_items, d_tiles, d_tiles8, stream, false);
}

int mrt_render_batch_frames_async(mrt_scene* s, const mrt_camera* cams, int32_t n_cams, const mrt_render_opts* opts,
                                  const int32_t* d_items, int32_t n_items, float* d_frames, uint8_t* d_frames8,
                                  void* stream) {
    return render_batch(s, cams, n_cams, opts, d_items, n_items, d_frames, d_frames8, stream, true);
}

// ---- device memory shared between processes (the multi-GPU split's frame assembly)
int mrt_ipc_export(const void* d_ptr, mrt_ipc_handle* out) {
    if (!d_ptr || !out) { set_error("bad argument"); return MRT_ERR_INVALID; }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    HIP_OK(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_ptr));
    hipIpcMemHandle_t h;
    HIP_OK(hipIpcGetMemHandle(&h, (void*)base));
    static_assert(sizeof(h) <= sizeof(out->handle), "hipIpcMemHandle_t does not fit mrt_ipc_handle");
    memset(out, 0, sizeof(*out));
    memcpy(out->handle, &h, sizeof(h));
    out->offset = (uint64_t)((const char*)d_ptr - (const char*)base);
    out->size = (uint64_t)size;
    return MRT_OK;
}

static std::mutex g_ipc_mu;
static std::vector<std::pair<void*, void*>> g_ipc_maps;   // (pointer handed out, mapping base)

int mrt_ipc_open(const mrt_ipc_handle* h, int device, void** d_ptr) {
    if (!h || !d_ptr || h->offset > h->size) { set_error("bad argument"); return MRT_ERR_INVALID; }
    HIP_OK(hipSetDevice(device));
    hipIpcMemHandle_t hh;
    memcpy(&hh, h->handle, sizeof(hh));
    void* base = nullptr;
    HIP_OK(hipIpcOpenMemHandle(&base, hh, hipIpcMemLazyEnablePeerAccess));
    *d_ptr = (char*)base + h->offset;
    std::lock_guard<std::mutex> g(g_ipc_mu);
    g_ipc_maps.emplace_back(*d_ptr, base);
    return MRT_OK;
}

int mrt_ipc_close(void* d_ptr) {
    void* base = nullptr;
    {
        std::lock_guard<std::mutex> g(g_ipc_mu);
        for (size_t i = 0; i < g_ipc_maps.size(); i++)
            if (g_ipc_maps[i].first == d_ptr) {
                base = g_ipc_maps[i].second;
                g_ipc_maps.erase(g_ipc_maps.begin() + (long)i);
                break;
            }
    }
    if (!base) { set_error("not a pointer from mrt_ipc_open"); return MRT_ERR_INVALID; }
    HIP_OK(hipIpcCloseMemHandle(base));
    return MRT_OK;
}

int mrt_render_buckets_async(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts, const int32_t* d_buckets,
                             int32_t n_buckets, float* d_tiles, void* stream) {
    if (!d_tiles) { set_error("bad argument"); return MRT_ERR_INVALID; }
    return mrt_render_batch_async(s, cam, 1, opts, d_buckets, n_buckets, d_tiles, nullptr, stream);
}

int mrt_unpack_batch_async(const int32_t* d_items, int32_t n_items, const float* d_tiles, const uint8_t* d_tiles8,
                           int32_t width, int32_t height, int32_t n_frames, float* d_frames, uint8_t* d_frames8,
                           const mrt_scene* s_for_lut, void* stream) {
    if ((n_items && !d_items) || n_items < 0 || width <= 0 || height <= 0 || n_frames < 1 || (!d_frames && !d_frames8)) {
        set_error("bad argument"); return MRT_ERR_INVALID;
    }
    if (d_frames && !d_tiles) { set_error("float frames need float tiles"); return MRT_ERR_INVALID; }
    if (d_frames8 && !d_tiles8 && !d_tiles) { set_error("rgb8 frames need tiles"); return MRT_ERR_INVALID; }
    const bool need_lut = d_frames8 && !d_tiles8;
    if (need_lut && (!s_for_lut || !s_for_lut->impl.dev)) { set_error("rgb8 needs an uploaded scene for the LUT"); return MRT_ERR_INVALID; }
    if (n_items == 0) return MRT_OK;
    const uint8_t* lut = need_lut ? s_for_lut->impl.dev->gamma : nullptr;
    const int bx = (width + 31) / 32, bpf = bx * ((height + 31) / 32);
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream, d_items,
                       n_items, d_tiles, d_tiles8, width, height, bx, bpf, n_frames, d_frames, d_frames8, lut);
    HIP_OK(hipGetLastError());
    return MRT_OK;
}

int mrt_unpack_buckets_async(const int32_t* d_buckets, int32_t n_buckets, const float* d_tiles, int32_t width,
                             int32_t height, float* d_frame, uint8_t* d_frame8, const mrt_scene* s_for_lut, void* stream) {
    if (!d_tiles || !d_frame) { set_error("bad argument"); return MRT_ERR_INVALID; }
    return mrt_unpack_batch_async(d_buckets, n_buckets, d_tiles, nullptr, width, height, 1, d_frame, d_frame8,
                                  s_for_lut, stream);
}

// HitInfo of a device hit record (t, a, b, prim bits): m_proxy from the id
static mrt_hit to_hit(const Scene& S, const float4& v) {
    mrt_hit h;
    h.t = v.x; h.a = v.y; h.b = v.z;
    h.prim = __builtin_bit_cast(int32_t, v.w);
    h.inst = -1;
    if (h.prim >= (int32_t)S.obj_mesh.size() && !S.instances.empty()) {
        int lo = 0, hi = (int)S.instances.size() - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (S.instances[mid].hit_base <= h.prim) lo = mid; else hi = mid - 1;
        }
        h.inst = lo;
    }
    return h;
}

// mrt_render over several devices: bucket b of the frame's 32x32 grid
// (src/Scene.cpp:90-95) -> share b mod n, share k rendered on devices[k] from
// that device's scene replica (own stream, persistent item / tile buffers).  The
// frame is assembled on the caller's device: every share's float tiles are
// copied into one gather buffer there (a peer copy over xGMI from another
// device, a device copy from the same one), the caller's stream waits for them
// and one unpack launch scatters them into the frame (+ Image::Map 8-bit), which
// is copied to the caller's host buffers once.  Each pixel is a pure function of
// (scene, camera, pixel, seed), so the frame is bit-identical to a one-device
// render.  Hit records (want_hits, debug / parity) still come back per share.
static int ensure_buf(DevOwner& own, void** p, size_t& cap, size_t bytes, hipStream_t drain) {
    return reserve(own, &drain, {{p, bytes}}, {{&cap, bytes}});
}
static int render_shared(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts, float* rgb, uint8_t* rgb8,
                         mrt_hit* hits) {
    Scene& S = s->impl;
    const int n = opts->n_devices, W = opts->width, H = opts->height;
    const int bx = (W + 31) / 32, bpf = bx * ((H + 31) / 32);
    const size_t tile_f = 1024 * 3;   // floats per 32x32 bucket tile
    int rc;
    // the caller's device: gather buffer, item list, frame, its own stream
    if ((rc = ensure_device(S, opts->device))) return rc;
    DeviceState& dc = *S.dev;
    HIP_OK(hipSetDevice(dc.device));
    if (!dc.gather_stream && (rc = dc.own.stream(dc.gather_stream))) return rc;
    const hipStream_t gs = dc.gather_stream;
    const size_t px = (size_t)W * H;
    if ((rc = ensure_frame(dc, px, &gs)) ||
        (rc = ensure_buf(dc.own, (void**)&dc.g_tiles, dc.g_tiles_cap, (size_t)bpf * tile_f * sizeof(float), gs)) ||
        (rc = ensure_buf(dc.own, (void**)&dc.g_items, dc.g_items_cap, (size_t)bpf * sizeof(int32_t), gs)))
        return rc;
    struct Share {
        int device = -1;
        DeviceState* d = nullptr;
        hipStream_t stream = nullptr;
        ShareBuf* buf = nullptr;
        size_t first = 0, ni = 0;   // its items' offset in the gathered list
        std::vector<float4> hitrec;
    };
    std::vector<Share> sh((size_t)n);
    std::vector<int32_t> all;   // the gathered item list: share 0's buckets, then share 1's, ...
    all.reserve((size_t)bpf);
    for (int k = 0; k < n; k++) {
        sh[k].first = all.size();
        for (int b = k; b < bpf; b += n) all.push_back(b);
        sh[k].ni = all.size() - sh[k].first;
    }
    HIP_OK(hipMemcpyAsync(dc.g_items, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, gs));
    rc = MRT_OK;
    for (int k = 0; k < n && rc == MRT_OK; k++) {
        Share& q = sh[k];
        q.device = opts->devices[k];
        if ((rc = ensure_device(S, q.device))) break;
        q.d = S.dev;
        int slot = 0;
        for (int j = 0; j < k; j++) slot += sh[j].device == q.device;
        if (hipSetDevice(q.device) != hipSuccess) { set_error("hipSetDevice"); rc = MRT_ERR_HIP; break; }
        while ((int)q.d->share_streams.size() <= slot) {
            hipStream_t st = nullptr;
            if (q.d->own.stream(st) != MRT_OK) { set_error("stream"); rc = MRT_ERR_HIP; break; }
            q.d->share_streams.push_back(st);
        }
        if (rc) break;
        while ((int)q.d->share_bufs.size() <= slot) q.d->share_bufs.push_back(new ShareBuf());
        q.stream = q.d->share_streams[slot];
        q.buf = q.d->share_bufs[slot];
        if (!q.buf->done && q.d->own.event(q.buf->done, hipEventDisableTiming) != MRT_OK) {
            set_error("event"); rc = MRT_ERR_HIP; break;
        }
        if (q.ni == 0) continue;
        const size_t tb = q.ni * tile_f * sizeof(float);
        if ((rc = ensure_buf(q.d->own, (void**)&q.buf->items, q.buf->items_cap, q.ni * sizeof(int32_t), q.stream)) ||
            (rc = ensure_buf(q.d->own, (void**)&q.buf->tiles, q.buf->tiles_cap, tb, q.stream)))
            break;
        if (hipMemcpyAsync(q.buf->items, all.data() + q.first, q.ni * sizeof(int32_t), hipMemcpyHostToDevice, q.stream) !=
            hipSuccess) {
            set_error("hipMemcpyAsync"); rc = MRT_ERR_HIP; break;
        }
        mrt_render_opts o = *opts;
        o.device = q.device; o.devices = nullptr; o.n_devices = 0;
        o.want_hits = hits ? 1 : 0;
        if ((rc = mrt_render_batch_async(s, cam, 1, &o, q.buf->items, (int32_t)q.ni, q.buf->tiles, nullptr, q.stream))) break;
        // the share's tiles into the caller's gather buffer: over xGMI from a peer, a device copy on the same device
        float* dst = dc.g_tiles + q.first * tile_f;
        hipError_t e;
        if (q.device == dc.device) {
            e = hipMemcpyAsync(dst, q.buf->tiles, tb, hipMemcpyDeviceToDevice, q.stream);
        } else {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, q.device, dc.device) == hipSuccess && can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(dc.device, 0);
                if (pe == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            }
            e = hipMemcpyPeerAsync(dst, dc.device, q.buf->tiles, q.device, tb, q.stream);
        }
        if (e != hipSuccess || hipEventRecord(q.buf->done, q.stream) != hipSuccess) {
            set_error(std::string("share tile copy: ") + hipGetErrorString(e)); rc = MRT_ERR_HIP; break;
        }
    }
    // the caller's stream: wait for every share's tiles, one unpack, one copy back
    if (rc == MRT_OK) {
        HIP_OK(hipSetDevice(dc.device));
        for (Share& q : sh)
            if (q.ni) HIP_OK(hipStreamWaitEvent(gs, q.buf->done, 0));
        hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)bpf), dim3(256), 0, gs, dc.g_items,
                           (int32_t)bpf, dc.g_tiles, (const uint8_t*)nullptr, W, H, bx, bpf, 1, dc.d_rgb,
                           rgb8 ? dc.d_rgb8 : nullptr, dc.gamma);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(rgb, dc.d_rgb, px * 12, hipMemcpyDeviceToHost, gs));
        if (rgb8) HIP_OK(hipMemcpyAsync(rgb8, dc.d_rgb8, px * 3, hipMemcpyDeviceToHost, gs));
    }
    mrt_stats total{};
    for (int k = 0; k < n && rc == MRT_OK; k++) {
        Share& q = sh[k];
        if (q.ni == 0) continue;
        if (hipSetDevice(q.device) != hipSuccess) { set_error("hipSetDevice"); rc = MRT_ERR_HIP; break; }
        StreamCtx* c = nullptr;
        if ((rc = get_ctx(*q.d, q.stream, c))) break;
        if (hits) {   // debug / parity: the share's hit records to the host
            q.hitrec.resize(q.ni * 1024);
            if (hipMemcpyAsync(q.hitrec.data(), c->hitbuf, q.ni * 1024 * sizeof(float4), hipMemcpyDeviceToHost, q.stream) !=
                hipSuccess) {
                set_error("hipMemcpyAsync"); rc = MRT_ERR_HIP; break;
            }
        }
        if (hipStreamSynchronize(q.stream) != hipSuccess) { set_error("hipStreamSynchronize"); rc = MRT_ERR_HIP; break; }
        // this share's counters (the share's own stream context)
        q.d->last = c;
        S.dev = q.d;
        mrt_stats st{};
        const int src = mrt_scene_last_stats(s, &st);
        if (src && src != MRT_ERR_OVERFLOW) { rc = src; break; }
        total.shadow_rays += st.shadow_rays; total.secondary_rays += st.secondary_rays;
        total.node_visits += st.node_visits; total.leaf_visits += st.leaf_visits;
        total.primary_node_visits += st.primary_node_visits; total.primary_leaf_visits += st.primary_leaf_visits;
        total.primary_hits += st.primary_hits; total.primary_wave_steps += st.primary_wave_steps;
        total.primary_uniform_visits += st.primary_uniform_visits;
        total.kernel_ms = std::max(total.kernel_ms, st.kernel_ms);
        total.fused = st.fused;
        total.chain = st.chain;
        total.max_stack = std::max(total.max_stack, st.max_stack);
        if (src == MRT_ERR_OVERFLOW) rc = src;
        if (hits)
            for (size_t i = 0; i < q.ni; i++) {
                const int b = all[q.first + i], x0 = (b % bx) * 32, y0 = (b / bx) * 32;
                for (int ly = 0; ly < 32 && y0 + ly < H; ly++)
                    for (int lx = 0; lx < 32 && x0 + lx < W; lx++)
                        hits[(size_t)(y0 + ly) * W + x0 + lx] = to_hit(S, q.hitrec[i * 1024 + ly * 32 + lx]);
            }
    }
    // every share and the assembly are done before the caller's buffers are returned
    for (Share& q : sh) {
        if (q.device >= 0) (void)hipSetDevice(q.device);
        if (q.stream) (void)hipStreamSynchronize(q.stream);
    }
    (void)hipSetDevice(dc.device);
    if (hipStreamSynchronize(gs) != hipSuccess && rc == MRT_OK) { set_error("frame assembly"); rc = MRT_ERR_HIP; }
    // the scene's current replica goes back to the caller's device (mrt_trace /
    // mrt_trace_async launch on S.dev->device), not the last share's
    for (DeviceState* d : S.devs)
        if (d->device == opts->device) S.dev = d;
    if (rc && rc != MRT_ERR_OVERFLOW) return rc;
    total.primary_rays = (uint64_t)W * H;
    S.last = total;
    S.stats_final = true;
    S.last_rc = rc;
    if (rc) set_error("traversal stack overflow");
    return rc;
}

int mrt_render(mrt_scene* s, const mrt_camera* cam, const mrt_render_opts* opts, float* rgb, uint8_t* rgb8, mrt_hit* hits) {
    if (!s || !cam || !opts || !rgb || opts->width <= 0 || opts->height <= 0) { set_error("bad argument"); return MRT_ERR_INVALID; }
    if (opts->n_devices < 0 || (opts->n_devices > 0 && !opts->devices)) { set_error("bad device list"); return MRT_ERR_INVALID; }
    if (opts->n_devices > 1 || (opts->n_devices == 1 && opts->devices[0] != opts->device)) {
        if (opts->n_devices > 64) { set_error("at most 64 bucket shares"); return MRT_ERR_INVALID; }
        return render_shared(s, cam, opts, rgb, rgb8, hits);
    }
    Scene& S = s->impl;
    int rc = ensure_device(S, opts->device);
    if (rc) return rc;
    HIP_OK(hipSetDevice(opts->device));
    DeviceState& d = *S.dev;
    size_t px = (size_t)opts->width * opts->height;
    if ((rc = ensure_frame(d, px, nullptr))) return rc;
    RenderParams P{};
    if ((rc = frame_params(S, cam, opts, P))) return rc;
    P.out_rgb = d.d_rgb;
    P.out_rgb8 = d.d_rgb8;
    if ((rc = launch_render(S, P, px, opts->count_visits != 0, nullptr, hits != nullptr || opts->want_hits))) return rc;
    HIP_OK(hipMemcpy(rgb, d.d_rgb, px * 12, hipMemcpyDeviceToHost));
    if (rgb8) HIP_OK(hipMemcpy(rgb8, d.d_rgb8, px * 3, hipMemcpyDeviceToHost));
    if (hits) {
        std::vector<float4> rec(px);
        HIP_OK(hipMemcpy(rec.data(), d.last->hitbuf, px * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < px; i++) hits[i] = to_hit(S, rec[i]);
    }
    S.last.primary_rays = px;
    mrt_stats tmp;
    if ((rc = mrt_scene_last_stats(s, &tmp))) return rc;
    return MRT_OK;
}

// ---- Scene::sampleScene for caller rays (ray mode of the render dispatch, P.mode == 2), and its
// hit / miss branch for caller (ray, hit) pairs (mrt_shade_hits)
// the ray mode of the render dispatch on device arrays (checked by the caller, n > 0);
// d_supplied: the caller's hit records in the primary launch's place (mrt_shade_hits)
static int ray_batch_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, size_t n,
                           int32_t row_width, uint32_t seed, int32_t count_visits, float* d_rgb, mrt_hit* d_hits,
                           const mrt_hit* d_supplied, void* stream) {
    int rc;
    Scene& S = s->impl;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(S, dp))) return rc;
    RenderParams P{};
    fill_params(S, P);
    P.min_subdivs = P.max_subdivs = 1;   // one sampleScene per ray
    P.seed = seed_or_default(seed);
    P.mode = 2;
    P.rays_o = d_o;
    P.rays_d = d_d;
    P.rays_t = d_time;
    P.n_rays = (uint32_t)n;
    // work items: 8x8 blocks of the ray image (a row at least as long as the batch is one row), or 64 rays in a row
    const size_t w = std::min<size_t>((size_t)row_width, n);
    P.ray_w = (int32_t)w;
    P.tiles_x = w ? (int32_t)((w + 7) / 8) : 1;
    P.n_tiles = w ? (int32_t)((size_t)P.tiles_x * (((n + w - 1) / w + 7) / 8)) : (int32_t)((n + 63) / 64);
    P.out_rgb = d_rgb;
    if ((rc = launch_render(S, P, n, count_visits != 0, (hipStream_t)stream, d_hits != nullptr, d_supplied))) return rc;
    S.last.primary_rays = (uint64_t)n;
    if (d_hits) {
        const DeviceState& d = *dp;
        const int g = (int)std::min<size_t>((n + 255) / 256, (size_t)d.cus * 8);
        hipLaunchKernelGGL(hit_records_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, d.last->hitbuf, n, d.insts,
                           (int32_t)d.n_insts, (int32_t)d.n_world, d_hits);
        HIP_OK(hipGetLastError());
    }
    return MRT_OK;
}

// the same on host arrays (checked by the caller, n > 0): hits out (nullable), or supplied in
static int ray_batch_sync(mrt_scene* s, const float* o, const float* d, const float* time, size_t n, int32_t row_width,
                          uint32_t seed, int32_t count_visits, float* rgb, mrt_hit* hits, const mrt_hit* supplied) {
    int rc;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(s->impl, dp))) return rc;
    Staged st;
    const float *bo = st.in(o, n * 12), *bd = st.in(d, n * 12);
    const mrt_hit* bs = st.in(supplied, n * sizeof(mrt_hit));
    const float* bt = st.in(time, n * 4);
    float* brgb = st.out<float>(n * 12);
    mrt_hit* bh = hits ? st.out<mrt_hit>(n * sizeof(mrt_hit)) : nullptr;
    if (st.rc) return st.rc;
    if ((rc = ray_batch_async(s, bo, bd, bt, n, row_width, seed, count_visits, brgb, bh, bs, nullptr))) return rc;
    if ((rc = st.back(rgb, brgb, n * 12))) return rc;
    if (hits && (rc = st.back(hits, bh, n * sizeof(mrt_hit)))) return rc;
    mrt_stats tmp;
    return mrt_scene_last_stats(s, &tmp);   // the counters; MRT_ERR_OVERFLOW
}

int mrt_sample_rays_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, size_t n,
                          int32_t row_width, uint32_t seed, int32_t count_visits, float* d_rgb, mrt_hit* d_hits,
                          void* stream) {
    const int rc = ray_args_check(s, n, row_width, {d_o, d_d, d_rgb}, "ray / output");
    if (rc || n == 0) return rc;
    return ray_batch_async(s, d_o, d_d, d_time, n, row_width, seed, count_visits, d_rgb, d_hits, nullptr, stream);
}

int mrt_sample_rays(mrt_scene* s, const float* o, const float* d, const float* time, size_t n, int32_t row_width,
                    uint32_t seed, int32_t count_visits, float* rgb, mrt_hit* hits) {
    const int rc = ray_args_check(s, n, row_width, {o, d, rgb}, "ray / output");
    if (rc || n == 0) return rc;
    return ray_batch_sync(s, o, d, time, n, row_width, seed, count_visits, rgb, hits, nullptr);
}

// the synchronous entries refuse a bad record of the host array, naming the first
static int host_hits_check(const mrt_scene* s, const mrt_hit* hits, size_t n) {
    const char* why = "";
    const size_t bad = first_bad_hit(s->impl, hits, n, why);
    if (bad == n) return MRT_OK;
    set_error("hit record " + std::to_string(bad) + ": " + why);
    return MRT_ERR_INVALID;
}

int mrt_shade_hits_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, const mrt_hit* d_hits,
                         size_t n, int32_t row_width, uint32_t seed, int32_t count_visits, float* d_rgb, void* stream) {
    const int rc = ray_args_check(s, n, row_width, {d_o, d_d, d_hits, d_rgb}, "ray / hit / output");
    if (rc || n == 0) return rc;
    return ray_batch_async(s, d_o, d_d, d_time, n, row_width, seed, count_visits, d_rgb, nullptr, d_hits, stream);
}

int mrt_shade_hits(mrt_scene* s, const float* o, const float* d, const float* time, const mrt_hit* hits, size_t n,
                   int32_t row_width, uint32_t seed, int32_t count_visits, float* rgb) {
    int rc = ray_args_check(s, n, row_width, {o, d, hits, rgb}, "ray / hit / output");
    if (rc || n == 0) return rc;
    if ((rc = host_hits_check(s, hits, n))) return rc;
    return ray_batch_sync(s, o, d, time, n, row_width, seed, count_visits, rgb, nullptr, hits);
}

// ---- Ray::getPoint + HitInfo::getAllInfos for caller (ray, hit) pairs (mrt_hit_surfaces)
// the replica's SurfaceGroup table, built on first use
static int surface_groups(const Scene& S, DeviceState& d) {
    std::lock_guard<std::mutex> g(d.mu);
    if (d.sgroups) return MRT_OK;
    std::vector<SurfaceGroup> G;
    int32_t at = 0;
    auto runs = [&](const std::vector<int32_t>& mesh, const std::vector<int32_t>& tri) {
        for (size_t i = 0; i < mesh.size(); i++, at++) {
            bool extends = false;   // the run so far (of this array: i > 0) goes on with this record
            if (i > 0 && G.back().mesh == mesh[i]) {
                SurfaceGroup& b = G.back();
                const int32_t k = at - b.start, step = tri[i] - tri[i - 1];
                if (k == 1 && (step == 1 || step == -1)) {   // its second record sets the direction
                    b.step = step;
                    extends = true;
                } else if (k > 1 && step == b.step) {
                    extends = true;
                }
            }
            if (!extends) G.push_back(SurfaceGroup{at, mesh[i], tri[i], 1});
        }
    };
    runs(S.obj_mesh, S.obj_tri);
    for (const Blas& b : S.blas) runs(b.obj_mesh, b.obj_tri);   // the PrimShade order of build_image
    SurfaceGroup* p = nullptr;   // (an empty table is 16 bytes, one record's size, as every empty upload)
    if (const int rc = d.own.upload(p, G.data(), G.size() * sizeof(SurfaceGroup))) return rc;
    d.n_sgroups = (int)G.size();
    d.sgroups = p;
    return MRT_OK;
}

// on device arrays (checked by the caller, n > 0)
static int hit_surfaces_async(mrt_scene* s, const float* d_o, const float* d_d, const mrt_hit* d_hits, size_t n,
                              mrt_surface* d_out, hipStream_t stream) {
    int rc;
    Scene& S = s->impl;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(S, dp))) return rc;
    DeviceState& d = *dp;
    if ((rc = surface_groups(S, d))) return rc;
    StreamCtx* c = nullptr;
    if ((rc = begin_query(S, d, stream, kCtrBytes, true, c))) return rc;
    RenderParams P{};
    fill_params(S, P);
    P.ctr = c->ctr;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)d.grid, (n + kWG - 1) / kWG));
    hipLaunchKernelGGL(surface_kernel, dim3(grid), dim3(kWG), 0, stream, P, d_o, d_d, d_hits, n, hit_id_count(S),
                       (const SurfaceGroup*)d.sgroups, (int32_t)d.n_sgroups, d_out);
    if ((rc = end_launch(d, *c, stream))) return rc;
    S.last = mrt_stats{};
    return MRT_OK;
}

int mrt_hit_surfaces_async(mrt_scene* s, const float* d_o, const float* d_d, const mrt_hit* d_hits, size_t n,
                           mrt_surface* d_out, void* stream) {
    const int rc = ray_args_check(s, n, 0, {d_o, d_d, d_hits, d_out}, "ray / hit / output");
    if (rc || n == 0) return rc;
    return hit_surfaces_async(s, d_o, d_d, d_hits, n, d_out, (hipStream_t)stream);
}

int mrt_hit_surfaces(mrt_scene* s, const float* o, const float* d, const mrt_hit* hits, size_t n, mrt_surface* out) {
    int rc = ray_args_check(s, n, 0, {o, d, hits, out}, "ray / hit / output");
    if (rc || n == 0) return rc;
    if ((rc = host_hits_check(s, hits, n))) return rc;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(s->impl, dp))) return rc;
    Staged st;
    const float *bo = st.in(o, n * 12), *bd = st.in(d, n * 12);
    const mrt_hit* bh = st.in(hits, n * sizeof(mrt_hit));
    mrt_surface* bs = st.out<mrt_surface>(n * sizeof(mrt_surface));
    if (st.rc) return st.rc;
    if ((rc = hit_surfaces_async(s, bo, bd, bh, n, bs, nullptr))) return rc;
    return st.back(out, bs, n * sizeof(mrt_surface));   // no counters: the host check has refused every bad record
}

// ---- Light::sampleLight for caller points (mrt_sample_lights): light_points_kernel, mrt_lights.hip
// on device arrays (checked by the caller, n > 0)
static int sample_lights_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                               const float* d_time, size_t n, uint32_t seed, uint32_t first_draw, int32_t secondary,
                               int32_t count_visits, float* d_e, float* d_per_light, hipStream_t stream) {
    int rc;
    Scene& S = s->impl;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(S, dp))) return rc;
    DeviceState& d = *dp;
    StreamCtx* c = nullptr;
    if ((rc = begin_query(S, d, stream, kCtrBytes, false, c))) return rc;
    RenderParams P{};
    fill_params(S, P);
    P.seed = seed_or_default(seed);
    P.gstack = c->gstack;
    P.ctr = c->ctr;
    P.fast_box = fast_box(d);
    P.cus = d.cus;
    P.scalar_nodes = g_tune.scalar_nodes & (d.boxes_ordered ? 7 : 3);
    P.near_first = g_tune.near_first > 0 ? 1 : 0;   // the fused kernels' setting
    // the band counters of the shadow launch, cleared with the statistics
    P.queue = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c->ctr) + CTR_N * sizeof(unsigned long long)) + 24 * 32;
    LightQuery Q{d_from, d_normal, d_rvec, d_time, d_e, d_per_light, (uint32_t)n, first_draw, secondary};
    const LightFn f = pick_light_points(count_visits != 0, P.fast_box != 0, d.special, d.has_alpha || d.has_mb, d.transparent);
    // a chunk per wave; a whole number of workgroups per XCD once there are 8
    const size_t blocks = (n + kWG - 1) / kWG;
    int g = (int)std::max<size_t>(1, std::min<size_t>(blocks, (size_t)std::min(d.grid, d.cus * blocks_per_cu(reinterpret_cast<KernelFn>(f), 0))));
    if (g > 8) g &= ~7;
    void* args[] = {&P, &Q};
    HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(f), dim3(g), dim3(kWG), args, 0, stream));
    if ((rc = end_launch(d, *c, stream))) return rc;
    S.last = mrt_stats{};
    return MRT_OK;
}

static int sample_lights_check(const mrt_scene* s, const void* from, const void* normal, size_t n, const void* e,
                               const void* per_light) {
    if (const int rc = ray_args_check(s, n, 0, {from, normal}, "point / normal")) return rc;
    if (n && !e && !per_light) { set_error("null output arrays: e and per_light"); return MRT_ERR_INVALID; }
    return MRT_OK;
}

int mrt_sample_lights_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                            const float* d_time, size_t n, uint32_t seed, uint32_t first_draw, int32_t secondary,
                            int32_t count_visits, float* d_e, float* d_per_light, void* stream) {
    const int rc = sample_lights_check(s, d_from, d_normal, n, d_e, d_per_light);
    if (rc || n == 0) return rc;
    return sample_lights_async(s, d_from, d_normal, d_rvec, d_time, n, seed, first_draw, secondary, count_visits, d_e,
                               d_per_light, (hipStream_t)stream);
}

int mrt_sample_lights(mrt_scene* s, const float* from, const float* normal, const float* rvec, const float* time, size_t n,
                      uint32_t seed, uint32_t first_draw, int32_t secondary, int32_t count_visits, float* e,
                      float* per_light) {
    int rc = sample_lights_check(s, from, normal, n, e, per_light);
    if (rc || n == 0) return rc;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(s->impl, dp))) return rc;
    const size_t pl_bytes = n * s->impl.lights.size() * 16;
    Staged st;
    const float *bf = st.in(from, n * 12), *bn = st.in(normal, n * 12), *br = st.in(rvec, n * 12), *bt = st.in(time, n * 4);
    float* be = e ? st.out<float>(n * 12) : nullptr;
    float* bp = per_light ? st.out<float>(std::max<size_t>(pl_bytes, 16)) : nullptr;   // (a scene without lights: nothing is written)
    if (st.rc) return st.rc;
    if ((rc = sample_lights_async(s, bf, bn, br, bt, n, seed, first_draw, secondary, count_visits, be, bp, nullptr))) return rc;
    if (e && (rc = st.back(e, be, n * 12))) return rc;
    if (per_light && pl_bytes && (rc = st.back(per_light, bp, pl_bytes))) return rc;
    mrt_stats tmp;
    return mrt_scene_last_stats(s, &tmp);   // the counters; MRT_ERR_OVERFLOW
}

// ---- mrt_light_samples: the same query through the frame's wavefront shadow passes over the
// point list -- gen (light_gen_kernel), bin, trace (shadow_kernel), resolve (light_resolve_kernel)
static int light_sample_cap(const Scene& S, bool secondary, int32_t* per_light) {
    int64_t total = 0;
    for (size_t l = 0; l < S.lights.size(); l++) {
        const DevLight& L = S.lights[l];
        const int32_t cap = L.type == MRT_POINT_LIGHT || (L.type == MRT_DOME_LIGHT && secondary) ? 1 : std::max(1, L.samples);
        if (per_light) per_light[l] = cap;
        total += cap;
    }
    return (int)std::min<int64_t>(total, INT32_MAX);
}

int mrt_scene_light_sample_cap(const mrt_scene* s, int32_t secondary, int32_t* per_light, int32_t* total) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    if (!s->impl.built) { set_error("scene not built"); return MRT_ERR_NOT_BUILT; }
    const int m = light_sample_cap(s->impl, secondary != 0, per_light);
    if (total) *total = m;
    return MRT_OK;
}

// scratch of a stream for n * m sample rows and n * n_lights counts; the records' own group
static int ensure_light_samples(StreamCtx& c, size_t rows, size_t counts, bool records) {
    if (const int rc = reserve(c.own, &c.stream, {{(void**)&c.ls_aux, rows * sizeof(float)}, {(void**)&c.ls_counts, counts * sizeof(int32_t)}},
                               {{&c.ls_aux_cap, rows}, {&c.ls_counts_cap, counts}}))
        return rc;
    if (!records) return MRT_OK;
    return reserve(c.own, &c.stream, {{&c.ls_rec, rows * sizeof(mrt_light_sample)}}, {{&c.ls_rec_cap, rows}});
}

// on device arrays (checked by the caller, n > 0)
static int light_samples_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                               const float* d_time, size_t n, uint32_t seed, uint32_t first_draw, int32_t secondary,
                               int32_t count_visits, mrt_light_sample* d_samples, int32_t* d_counts, float* d_e,
                               float* d_per_light, hipStream_t stream) {
    int rc;
    Scene& S = s->impl;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(S, dp))) return rc;
    DeviceState& d = *dp;
    StreamCtx* cp = nullptr;
    if ((rc = begin_query(S, d, stream, kCtrBytes, false, cp))) return rc;
    StreamCtx& c = *cp;
    const int m = light_sample_cap(S, secondary != 0, nullptr);
    if (m == 0) {   // no lights: a zero sum, nothing else
        if (d_e) HIP_OK(hipMemsetAsync(d_e, 0, n * 12, stream));
    } else {
        const size_t n_rays = n * (size_t)m, n_lights = S.lights.size();
        const bool count = count_visits != 0;
        if ((rc = ensure_rays(c, n, (size_t)m))) return rc;
        if ((rc = ensure_light_samples(c, n_rays, n * n_lights, d_samples == nullptr))) return rc;
        RenderParams P{};
        fill_params(S, P);
        P.seed = seed_or_default(seed);
        P.gstack = c.gstack;
        P.ctr = c.ctr;
        P.fast_box = fast_box(d);
        P.cus = d.cus;
        P.scalar_nodes = g_tune.scalar_nodes & (d.boxes_ordered ? 7 : 3);
        P.ray_o = c.rays;
        P.ray_d = c.rays + n_rays;
        P.occl = c.occl;
        P.nrays = c.nrays;
        P.max_shadow = m;
        LightSamples G{};
        G.q = LightQuery{d_from, d_normal, d_rvec, d_time, d_e, d_per_light, (uint32_t)n, first_draw, secondary};
        G.rec = d_samples ? d_samples : static_cast<mrt_light_sample*>(c.ls_rec);
        G.aux = c.ls_aux;
        G.counts = d_counts ? d_counts : c.ls_counts;
        G.m = m;
        G.write_vis = d_samples ? 1 : 0;
        const int blocks = (int)((n + kWG - 1) / kWG);   // n <= 2^28
        void* pass_args[] = {&P, &G};
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(pick_light_gen()), dim3(blocks), dim3(kWG), pass_args, 0, stream));
        // the frame's shadow launch (launch_render): schedule, grid, walk order, bins
        const bool inst = d.special, chk = d.has_alpha || d.has_mb, fb = P.fast_box != 0;
        bool dome = false;
        for (const DevLight& l : S.lights) dome |= l.type == MRT_DOME_LIGHT;
        int sched = g_tune.shadow_sched >= 0 ? g_tune.shadow_sched : (dome ? 2 : 1), refill = kRefillMin;
        ShadowFn sf = pick_shadow(count, fb, inst, sched == 2, chk);
        int g = std::max(1, std::min(d.grid, d.cus * blocks_per_cu(reinterpret_cast<KernelFn>(sf), 0)));
        if (sched && (g & 7)) g &= ~7;
        if (g < 8) {
            sched = 0;
            sf = pick_shadow(count, fb, inst, false, chk);
        }
        P.near_first = g_tune.near_first >= 0 ? g_tune.near_first : (sched == 2 || inst ? 0 : 1);
        if (bin_mode(d) & 1) {   // (no instance-major keys: a point list has no primary hits)
            if ((rc = ensure_bin(c, n_rays))) return rc;
            BinArgs A = bin_args(d, c, 0, P.ray_o, P.ray_d, n_rays);
            A.nrays = P.nrays;
            A.m = (uint32_t)m;
            if ((rc = bin_rays(A, bin_grid(d, n_rays), stream))) return rc;
            P.sh_perm = A.perm;
            P.sh_perm_n = bin_total(A);
        }
        // the band counters of the shadow launch, cleared with the statistics
        P.queue = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c.ctr) + CTR_N * sizeof(unsigned long long)) + 24 * 32;
        size_t nr = n_rays;
        void* args[] = {&P, &nr, &sched, &refill};
        HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(sf), dim3(g), dim3(kWG), args, 0, stream));
        P.sh_perm = nullptr;
        P.sh_perm_n = nullptr;
        if (d_samples || d_e || d_per_light)   // (counts alone: nothing is left to write)
            HIP_OK(hipLaunchKernel(reinterpret_cast<const void*>(pick_light_resolve()), dim3(blocks), dim3(kWG), pass_args, 0, stream));
    }
    if ((rc = end_launch(d, c, stream))) return rc;
    S.last = mrt_stats{};
    return MRT_OK;
}

// every refusal, before any device call
static int light_samples_check(const mrt_scene* s, const void* from, const void* normal, size_t n, const void* samples,
                               const void* counts, const void* e, const void* per_light, int32_t secondary) {
    if (const int rc = ray_args_check(s, n, 0, {from, normal}, "point / normal")) return rc;
    if (n && !samples && !counts && !e && !per_light) {
        set_error("null output arrays: samples, counts, e and per_light");
        return MRT_ERR_INVALID;
    }
    for (const DevLight& l : s->impl.lights)
        if (l.transparent) {
            set_error("a light with transparent shadows: the wavefront shadow answer is one bit (use mrt_sample_lights)");
            return MRT_ERR_INVALID;
        }
    const int m = light_sample_cap(s->impl, secondary != 0, nullptr);
    if (m > kMaxWaveShadow) {
        set_error("more than 64 light samples per point (mrt_scene_light_sample_cap)");
        return MRT_ERR_INVALID;
    }
    if ((uint64_t)n * (uint64_t)m >= (uint64_t(1) << 32)) {
        set_error("too many light-sample rows: n * M reaches 2^32");
        return MRT_ERR_INVALID;
    }
    return MRT_OK;
}

int mrt_light_samples_async(mrt_scene* s, const float* d_from, const float* d_normal, const float* d_rvec,
                            const float* d_time, size_t n, uint32_t seed, uint32_t first_draw, int32_t secondary,
                            int32_t count_visits, mrt_light_sample* d_samples, int32_t* d_counts, float* d_e,
                            float* d_per_light, void* stream) {
    const int rc = light_samples_check(s, d_from, d_normal, n, d_samples, d_counts, d_e, d_per_light, secondary);
    if (rc || n == 0) return rc;
    return light_samples_async(s, d_from, d_normal, d_rvec, d_time, n, seed, first_draw, secondary, count_visits, d_samples,
                               d_counts, d_e, d_per_light, (hipStream_t)stream);
}

int mrt_light_samples(mrt_scene* s, const float* from, const float* normal, const float* rvec, const float* time, size_t n,
                      uint32_t seed, uint32_t first_draw, int32_t secondary, int32_t count_visits, mrt_light_sample* samples,
                      int32_t* counts, float* e, float* per_light) {
    int rc = light_samples_check(s, from, normal, n, samples, counts, e, per_light, secondary);
    if (rc || n == 0) return rc;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(s->impl, dp))) return rc;
    const size_t n_lights = s->impl.lights.size();
    const size_t rec_bytes = n * (size_t)light_sample_cap(s->impl, secondary != 0, nullptr) * sizeof(mrt_light_sample);
    const size_t cnt_bytes = n * n_lights * 4, pl_bytes = n * n_lights * 16;
    Staged st;
    const float *bf = st.in(from, n * 12), *bn = st.in(normal, n * 12), *br = st.in(rvec, n * 12), *bt = st.in(time, n * 4);
    // the records go in as well: the rows past a point's count keep what the caller put there
    mrt_light_sample* bs = samples && rec_bytes ? st.in(samples, rec_bytes) : nullptr;
    int32_t* bc = counts ? st.out<int32_t>(std::max<size_t>(cnt_bytes, 16)) : nullptr;
    float* be = e ? st.out<float>(n * 12) : nullptr;
    float* bp = per_light ? st.out<float>(std::max<size_t>(pl_bytes, 16)) : nullptr;
    if (st.rc) return st.rc;
    if ((rc = light_samples_async(s, bf, bn, br, bt, n, seed, first_draw, secondary, count_visits, bs, bc, be, bp, nullptr)))
        return rc;
    if (samples && rec_bytes && (rc = st.back(samples, bs, rec_bytes))) return rc;
    if (counts && cnt_bytes && (rc = st.back(counts, bc, cnt_bytes))) return rc;
    if (e && (rc = st.back(e, be, n * 12))) return rc;
    if (per_light && pl_bytes && (rc = st.back(per_light, bp, pl_bytes))) return rc;
    mrt_stats tmp;
    return mrt_scene_last_stats(s, &tmp);   // the counters; MRT_ERR_OVERFLOW
}

int mrt_camera_rays(const mrt_camera* cam, int32_t width, int32_t height, uint32_t seed, float* o, float* d, float* time) {
    if (!cam || !o || !d || !time) { set_error("bad argument"); return MRT_ERR_INVALID; }
    CamParams C;
    int rc = host_camera(cam, width, height, C);   // (rejects a non-positive size)
    if (rc) return rc;
    const uint16_t* RS = host_rsqrt_table();
    const uint32_t sd = seed_or_default(seed);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const EyeRay er = camera_ray(C, sd, x, y, RS);   // the device's eye_ray(), compiled for the host
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            o[3 * i] = er.o.x; o[3 * i + 1] = er.o.y; o[3 * i + 2] = er.o.z;
            d[3 * i] = er.d.x; d[3 * i + 1] = er.d.y; d[3 * i + 2] = er.d.z;
            time[i] = er.time;
        }
    return MRT_OK;
}

int mrt_scene_walk_info(const mrt_scene* cs, int32_t* lds_nodes, int32_t* walk_exits) {
    if (!cs) { set_error("bad argument"); return MRT_ERR_INVALID; }
    const Scene& S = cs->impl;
    const DeviceState* d = S.dev;
    if (lds_nodes) *lds_nodes = d ? (int32_t)d->lds_pick.load() : -1;
    if (walk_exits) {
        *walk_exits = g_tune.walk_exit ? 1 : 2;
    }
    return MRT_OK;
}

int mrt_scene_last_stats(const mrt_scene* cs, mrt_stats* out) {
    if (!cs || !out) { set_error("bad argument"); return MRT_ERR_INVALID; }
    mrt_scene* s = const_cast<mrt_scene*>(cs);
    Scene& S = s->impl;
    if (S.stats_final) {   // multi-device mrt_render: the shares' counters, summed
        *out = S.last;
        if (S.last_rc) set_error("traversal stack overflow");
        return S.last_rc;
    }
    if (!S.dev) { set_error("nothing rendered"); return MRT_ERR_INVALID; }
    DeviceState& d = *S.dev;
    if (!d.last) { set_error("nothing rendered"); return MRT_ERR_INVALID; }
    const StreamCtx& x = *d.last;
    HIP_OK(hipSetDevice(d.device));
    HIP_OK(hipEventSynchronize(x.ev1));
    unsigned long long c[CTR_N];
    HIP_OK(hipMemcpy(c, x.ctr, sizeof c, hipMemcpyDeviceToHost));
    unsigned long long invalid = 0;   // a launch on the caller's hit records: those it refused
    if (x.supplied) HIP_OK(hipMemcpy(&invalid, x.ctr + CTR_INVALID, sizeof invalid, hipMemcpyDeviceToHost));
    float ms = 0.f, ms1 = 0.f, ms2 = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, x.ev0, x.ev1));
    if (x.last_was_render) {
        HIP_OK(hipEventElapsedTime(&ms1, x.ev0, x.evm));
        HIP_OK(hipEventElapsedTime(&ms2, x.evm, x.ev1));
    }
    S.last.primary_ms = ms1;
    S.last.shade_ms = ms2;
    S.last.primary_node_visits = c[CTR_NODES_P];
    S.last.primary_leaf_visits = c[CTR_LEAVES_P];
    S.last.shadow_rays = c[CTR_SHADOW];
    S.last.primary_hits = c[CTR_HITS];
    if (c[CTR_RAYS_P]) S.last.primary_rays = c[CTR_RAYS_P];
    S.last.secondary_rays = c[CTR_SECONDARY];   // adaptive supersampling: eye rays traced
    S.last.primary_wave_steps = c[CTR_WAVE_STEPS_P];
    S.last.primary_uniform_visits = c[CTR_UNIFORM_P];
    S.last.node_visits = c[CTR_NODES];
    S.last.leaf_visits = c[CTR_LEAVES];
    S.last.max_stack = (int32_t)c[CTR_MAXSP];
    S.last.shadow_wave_steps = c[CTR_WAVE_STEPS_S];
    S.last.shadow_node_visits = c[CTR_NODES_S];
    if (x.last_was_render && c[CTR_TP + 3]) {   // count mode: wave ramp / tail (wall clock)
        const double us = d.wall_khz > 0 ? 1e3 / d.wall_khz : 0.0;
        for (int k = 0; k < 2; k++) {
            // the fused frame kernel is one launch: its span is the primary record's
            const unsigned long long* t = c + ((k && !x.fused) ? CTR_TS : CTR_TP);
            const double s0 = (double)~t[0], s1 = (double)t[1], e0 = (double)~t[2], e1 = (double)t[3];
            float* o = k ? &S.last.shade_span_us : &S.last.primary_span_us;
            o[0] = (float)((e1 - s0) * us);   // first wave start -> last wave end
            o[1] = (float)((s1 - s0) * us);   // ramp: first -> last wave start
            o[2] = (float)((e1 - e0) * us);   // tail: first -> last wave end
        }
    }
    S.last.kernel_ms = ms;
    S.last.fused = x.last_was_render && x.fused ? 1 : 0;
    S.last.chain = x.last_was_render && x.chain_used ? 1 : 0;
    S.last.chain_budget_bytes = x.chain_budget;
    S.last.chain_chunks = x.chain_chunks;
    S.last.chain_fallbacks = (int32_t)c[CTR_FALLBACK];
    *out = S.last;
    if (c[CTR_OVERFLOW]) { set_error("traversal stack overflow"); return MRT_ERR_OVERFLOW; }
    if (invalid) {
        set_error(std::to_string(invalid) + " invalid hit record(s): treated as misses");
        return MRT_ERR_INVALID;
    }
    return MRT_OK;
}

// mrt_trace_async / mrt_trace_rays_async: d_time == nullptr is Ray(o, d), trace_kernel
static int trace_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, const float* d_tmin,
                       const float* d_tmax, size_t n, int any_hit, mrt_hit* d_out, hipStream_t stream) {
    int rc;
    Scene& S = s->impl;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(S, dp)) || n == 0) return rc;
    DeviceState& d = *dp;
    StreamCtx* cp = nullptr;
    if ((rc = begin_query(S, d, stream, CTR_N * sizeof(unsigned long long), false, cp))) return rc;
    StreamCtx& c = *cp;
    int grid = (int)std::min<size_t>((size_t)d.grid, (n + kWG - 1) / kWG);
    Trav alpha{};
    alpha.aprims = d.prims; alpha.apuv = d.puv; alpha.auv = d.uvs; alpha.amats = d.mats; alpha.atex = d.texs;
    alpha.pflags = d.pflags; alpha.verts = d.verts; alpha.verts2 = d.verts2;
    if (d_time) {
        auto kern = any_hit ? (d.special ? trace_timed_kernel<true, true> : trace_timed_kernel<true, false>)
                            : (d.special ? trace_timed_kernel<false, true> : trace_timed_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kWG), 0, stream, d.nodes, d.leaves, d.tables, c.gstack, d.gthreads,
                           d_o, d_d, d_time, d_tmin, d_tmax, n, d_out, c.ctr, fast_box(d), d.insts, alpha);
    } else {
        auto kern = any_hit ? (d.special ? trace_kernel<true, true> : trace_kernel<true, false>)
                            : (d.special ? trace_kernel<false, true> : trace_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kWG), 0, stream, d.nodes, d.leaves, d.tables, c.gstack, d.gthreads,
                           d_o, d_d, d_tmin, d_tmax, n, d_out, c.ctr, fast_box(d), d.insts, alpha);
    }
    return end_launch(d, c, stream);
}

// mrt_trace / mrt_trace_rays: host arrays in and out (time nullable)
static int trace_sync(mrt_scene* s, const float* o, const float* d, const float* time, const float* tmin,
                      const float* tmax, size_t n, int any_hit, mrt_hit* out) {
    int rc;
    DeviceState* dp = nullptr;
    if ((rc = current_replica(s->impl, dp)) || n == 0) return rc;
    Staged st;
    const float *bo = st.in(o, n * 12), *bd = st.in(d, n * 12), *bt = st.in(time, n * 4);
    const float *bmin = st.in(tmin, n * 4), *bmax = st.in(tmax, n * 4);
    mrt_hit* bout = st.out<mrt_hit>(n * sizeof(mrt_hit));
    if (st.rc) return st.rc;
    if ((rc = trace_async(s, bo, bd, bt, bmin, bmax, n, any_hit, bout, nullptr))) return rc;
    if ((rc = st.back(out, bout, n * sizeof(mrt_hit)))) return rc;
    unsigned long long c[CTR_N];   // only the overflow flag: a trace leaves the scene's last statistics alone
    if ((rc = st.back(c, dp->last->ctr, sizeof c))) return rc;
    if (c[CTR_OVERFLOW]) { set_error("traversal stack overflow"); return MRT_ERR_OVERFLOW; }
    return MRT_OK;
}

// The older pair keeps its own checks: one message, no batch cap, and "not built" comes from the
// replica, so n == 0 asks for it too.
static int trace_args_check(const mrt_scene* s, size_t n, std::initializer_list<const void*> need) {
    if (!s || (n && any_null(need))) { set_error("bad argument"); return MRT_ERR_INVALID; }
    return MRT_OK;
}

int mrt_trace_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_tmin, const float* d_tmax, size_t n,
                    int any_hit, mrt_hit* d_out, void* stream) {
    if (const int rc = trace_args_check(s, n, {d_o, d_d, d_tmin, d_tmax, d_out})) return rc;
    return trace_async(s, d_o, d_d, nullptr, d_tmin, d_tmax, n, any_hit, d_out, (hipStream_t)stream);
}

int mrt_trace(mrt_scene* s, const float* o, const float* d, const float* tmin, const float* tmax, size_t n, int any_hit,
              mrt_hit* out) {
    if (const int rc = trace_args_check(s, n, {o, d, tmin, tmax, out})) return rc;
    return trace_sync(s, o, d, nullptr, tmin, tmax, n, any_hit, out);
}

// ---- Scene::trace for rays with a time (mrt_trace_rays)
int mrt_trace_rays_async(mrt_scene* s, const float* d_o, const float* d_d, const float* d_time, const float* d_tmin,
                         const float* d_tmax, size_t n, int any_hit, mrt_hit* d_out, void* stream) {
    const int rc = ray_args_check(s, n, 0, {d_o, d_d, d_tmin, d_tmax, d_out}, "ray / bound / output");
    if (rc || n == 0) return rc;
    return trace_async(s, d_o, d_d, d_time, d_tmin, d_tmax, n, any_hit, d_out, (hipStream_t)stream);
}

int mrt_trace_rays(mrt_scene* s, const float* o, const float* d, const float* time, const float* tmin, const float* tmax,
                   size_t n, int any_hit, mrt_hit* out) {
    const int rc = ray_args_check(s, n, 0, {o, d, tmin, tmax, out}, "ray / bound / output");
    if (rc || n == 0) return rc;
    return trace_sync(s, o, d, time, tmin, tmax, n, any_hit, out);
}

int mrt_debug_wave_log(const mrt_scene* cs, int launch, uint64_t* out, int32_t max_waves) {
    if (!cs || !out || launch < 0 || launch > 1 || max_waves < 0) { set_error("bad argument"); return MRT_ERR_INVALID; }
    const Scene& S = cs->impl;
    if (!S.dev) { set_error("nothing rendered"); return MRT_ERR_INVALID; }
    const DeviceState& d = *S.dev;
    HIP_OK(hipSetDevice(d.device));
    if (!d.last) { set_error("nothing rendered"); return MRT_ERR_INVALID; }
    HIP_OK(hipEventSynchronize(d.last->ev1));
    const int n = std::min(max_waves, d.last->log_waves[launch]);
    const size_t log_stride = (size_t)d.grid * (kWG / 64) * kLogWords;
    if (n > 0)
        HIP_OK(hipMemcpy(out, d.last->wave_log + launch * log_stride, (size_t)n * kLogWords * sizeof(uint64_t),
                         hipMemcpyDeviceToHost));
    return n;
}

int mrt_device_wall_clock_khz(const mrt_scene* cs) {
    if (!cs || !cs->impl.dev) { set_error("scene not on a device"); return MRT_ERR_INVALID; }
    return cs->impl.dev->wall_khz;
}

int mrt_debug_libm(int fn, const float* x, const float* y, size_t n, float* out) {
    if (fn < 0 || fn > 5 || !x || !out || ((fn == 1 || fn == 5) && !y)) { set_error("bad libm probe arguments"); return MRT_ERR_INVALID; }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_error("no HIP device"); return MRT_ERR_NO_DEVICE; }
    if (n == 0) return MRT_OK;
    const size_t b = n * sizeof(float);
    Staged st;
    const float* dx = st.in(x, b);
    const float* dy = fn == 1 || fn == 5 ? st.in(y, b) : st.out<float>(b);   // (the kernel's argument; read by 1 and 5 only)
    const uint16_t* dt = st.in(host_rcp_table(), 2048 * sizeof(uint16_t));
    float* dout = st.out<float>(b);
    if (st.rc) return st.rc;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(libm_kernel, dim3(blocks), dim3(256), 0, 0, fn, dx, dy, n, dout, dt);
    HIP_OK(hipGetLastError());
    return st.back(out, dout, b);
}

// bin_rays (mrt_bin.hip) as the renderer calls it, on the caller's arrays: no kernel of its own
int mrt_debug_bin_rays(const mrt_bin_probe* p) {
    const auto refuse = [](const char* m) { set_error(m); return MRT_ERR_INVALID; };
    if (!p || !p->o || !p->d || !p->keys || !p->hist || !p->perm) return refuse("null ray-bin probe array");
    if (p->m < 1) return refuse("ray-bin probe: m must be at least 1");
    if (p->grid < 1 || p->grid > 1024) return refuse("ray-bin probe: grid must be 1..1024");
    if (p->n >= 0x80000000u) return refuse("ray-bin probe: fewer than 2^31 rays");
    if (p->inst_cell && !p->inst_inv) return refuse("ray-bin probe: inst_cell needs the instance matrices");
    if (p->hits && (!p->hit_base || !p->inst_class || p->n_inst < 1)) return refuse("ray-bin probe: hits need the instance tables");
    if (p->hits)   // (a larger class would carry the key past the bins)
        for (int32_t i = 0; i < p->n_inst; i++)
            if (p->inst_class[i] > 127) return refuse("ray-bin probe: inst_class above 127");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_error("no HIP device"); return MRT_ERR_NO_DEVICE; }
    const size_t n = p->n, px = (n + p->m - 1) / p->m, ni = p->hits ? (size_t)p->n_inst : 0;
    Staged st;
    // an empty array takes one element and no copy
    const auto in = [&](const auto* host, size_t count) {
        return count ? st.in(host, count * sizeof *host) : st.out<std::remove_cv_t<std::remove_pointer_t<decltype(host)>>>(sizeof *host);
    };
    BinArgs A{};
    A.o = (const float4*)in(p->o, 4 * n);
    A.d = (const float4*)in(p->d, 4 * n);
    A.n = p->n;
    A.n_dev = p->has_n_dev ? in(&p->n_dev, 1) : nullptr;
    A.mul1 = p->mul1; A.sub = p->sub; A.cap1 = p->cap1; A.mul2 = p->mul2;
    A.nrays = p->nrays ? in(p->nrays, px) : nullptr;
    A.m = p->m;
    for (int a = 0; a < 3; a++) { A.lo[a] = p->lo[a]; A.inv[a] = p->inv[a]; }
    A.dbits = p->dbits; A.obits = p->obits;
    std::vector<DevInstance> DI;
    if (p->hits) {
        A.hits = (const float4*)in(p->hits, 4 * px);
        A.hit_base = in(p->hit_base, ni);
        A.inst_class = in(p->inst_class, ni);
        A.n_inst = p->n_inst; A.n_world = p->n_world;
        if (p->inst_cell) {
            DI.resize(ni);
            for (size_t i = 0; i < ni; i++) {
                memset(&DI[i], 0, sizeof(DevInstance));
                memcpy(DI[i].inv, p->inst_inv + 12 * i, 12 * sizeof(float));
                DI[i].inv[15] = 1.f;
            }
            A.inst_cell = (const float4*)in(p->inst_cell, 8 * ni);
            A.insts = in(DI.data(), ni);
        }
    }
    A.keys = const_cast<uint16_t*>(in((const uint16_t*)p->keys, n));
    A.perm = const_cast<uint32_t*>(in((const uint32_t*)p->perm, n));
    A.hist = st.out<uint32_t>(kBinHist * sizeof(uint32_t));
    if (st.rc) return st.rc;
    if (const int rc = bin_rays(A, p->grid, 0)) return rc;
    HIP_OK(hipStreamSynchronize(0));
    const int bits = A.hits ? kBinBits : 2 * A.dbits + 3 * A.obits;
    int rc = st.back(p->hist, A.hist, ((size_t(1) << bits) + 1) * sizeof(uint32_t));
    if (!rc && n) rc = st.back(p->keys, A.keys, n * sizeof(uint16_t));
    if (!rc && n) rc = st.back(p->perm, A.perm, n * sizeof(uint32_t));
    return rc;
}

}  // extern "C"
