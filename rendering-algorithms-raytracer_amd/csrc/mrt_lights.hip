// mrt_lights.hip -- Light::sampleLight (src/Light.h:35) for caller points: the kernel of
// mrt_sample_lights.  The work item is a point with a normal, not a pixel or a hit; every
// light of the scene is sampled there by the shader's own sample_light -- point_light,
// rect_light, dome_light, the any-hit shadow walks, the transparency walk -- with the draws
// numbered as Material::shade numbers them.  A translation unit of its own: no existing
// instantiation changes and the library's kernels compile in parallel.
#include "mrt_shader.h"

namespace mrt {

static constexpr int kLightChunk = 64;   // a wave's work item: 64 consecutive points

// One lane per point, persistent workgroups.  The schedule is shadow_kernel's XCD bands: the
// points are cut into 8 contiguous bands and workgroup b takes 64-point chunks of band b mod 8
// from that band's counter (P.queue, 128 B apart), then steals from the others.  Chosen over a
// grid-stride loop because a point's cost varies by orders of magnitude -- nothing for a
// point that faces away from every light, a light's whole sample count of walks for one that
// does not -- so equal shares of points are not equal shares of work; and callers list
// points in surface order (texels, vertices, a camera's hits), so a band is a region of the
// scene and one XCD's L2 holds that region's share of the hierarchy.
// CHECK: the special-leaf scene has alpha-mapped or motion-blurred lanes (false: instances only)
// XP: a rectangle / dome light has transparent shadows: Shader REC = 1, which compiles
//     Shader::transmit into light_vis (nothing else of REC is reached from sample_light)
template <bool COUNT, bool FAST, bool INST, bool CHECK, bool XP>
__global__ void __launch_bounds__(kWG) light_points_kernel(RenderParams P, LightQuery Q) {
    __shared__ uint16_t s_tab[2048];
    __shared__ int32_t s_stack[kLdsStack * kWG];
    load_tables(P.tables, s_tab, 1024);
    const uint16_t* rcpT = s_tab;           // per triangle test: LDS
    const uint16_t* rsqT = P.tables + 2048; // a few per sample: global (L1-resident)
    const int tid = threadIdx.x, lane = tid & 63;
    Trav T{P.nodes, P.fast_box != 0, P.scalar_nodes, P.leaves, rcpT, s_stack + tid, P.gstack + (blockIdx.x * kWG + tid), P.gstride};
    T.inst = P.insts;
    trav_alpha(T, P);
    TravStats st;
    uint32_t shadow_total = 0;
    const size_t n = Q.n;
    auto band_lo = [&](int k) { return n * (size_t)k / 8; };
    int band = blockIdx.x & 7, probes = 0;
    // wave-level dequeue of a chunk of the current band (or of the next band with points left):
    // lane 0's atomic, broadcast; false: every band is exhausted
    auto dequeue = [&](size_t& first, size_t& end) {
        unsigned long long got = ~0ull, hi = 0;
        if (lane == 0) {
            while (probes < 8) {
                const size_t lo = band_lo(band), bend = band_lo(band + 1);
                const unsigned long long v = atomicAdd(reinterpret_cast<unsigned long long*>(P.queue + band * 32),
                                                       (unsigned long long)kLightChunk);
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
    size_t first, end;
    while (dequeue(first, end)) {
        const size_t i = first + (size_t)lane;
        if (i < end) {   // (a band's last chunk is cut at the band's end)
            const float* f = Q.from + 3 * i;
            const float* nn = Q.normal + 3 * i;
            const v3 from = mk(f[0], f[1], f[2]), normal = mk(nn[0], nn[1], nn[2]);
            v3 rVec = mk(0, 0, 0);
            if (Q.rvec) rVec = mk(Q.rvec[3 * i], Q.rvec[3 * i + 1], Q.rvec[3 * i + 2]);
            Shader<false, FAST, INST, kFused, XP ? 1 : 0, CHECK> S{P, T, rcpT, rsqT, st, (uint32_t)i, 0u, P.seed, 0, 0u};
            S.skey = 0u;
            S.dim = level_key(0) + Q.first_draw;
            S.time = S.shadow_time = Q.time ? Q.time[i] : 0.f;
            v3 sum = mk(0, 0, 0);
            for (int l = 0; l < P.n_lights; l++) {
                float spec = 0.f;
                const v3 E = S.template sample_light<COUNT>(l, from, normal, rVec, spec, Q.secondary != 0);
                sum = add(sum, E);
                if (Q.per_light) {
                    float* o = Q.per_light + ((size_t)i * (size_t)P.n_lights + (size_t)l) * 4;
                    o[0] = E.x; o[1] = E.y; o[2] = E.z; o[3] = spec;
                }
            }
            if (Q.e) {
                float* o = Q.e + 3 * i;
                o[0] = sum.x; o[1] = sum.y; o[2] = sum.z;
            }
            shadow_total += S.shadow_rays;
        }
    }
    // the shadow-ray count, the visit counters (count mode) and the overflow flag
    flush_stats<COUNT, false, false>(P, st, shadow_total, lane, 0, 0);
}

template <bool INST, bool CHECK>
static LightFn light_points_fn(bool c, bool f, bool xp) {
    return with_bools([](auto C, auto F, auto X) -> LightFn { return light_points_kernel<C(), F(), INST, CHECK, X()>; }, c, f, xp);
}
// plain scenes have no special lanes to check (their walks never read the switch)
LightFn pick_light_points(bool c, bool f, bool inst, bool check, bool xp) {
    if (!inst) return light_points_fn<false, true>(c, f, xp);
    return check ? light_points_fn<true, true>(c, f, xp) : light_points_fn<true, false>(c, f, xp);
}

}  // namespace mrt
