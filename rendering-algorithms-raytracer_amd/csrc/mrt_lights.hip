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

// ---------------------------------------------------------------- mrt_light_samples: gen / resolve
// The same query through wavefront passes: light_gen_kernel runs the three light loops once per
// point and writes every sample's record and every shadow ray; the rays are binned and traced
// by shadow_kernel (mrt_device.hip), as a frame's are; light_resolve_kernel sums each light's
// records with the answers.  Neither kernel walks the hierarchy: no LDS, no stack columns.
//
// The loops are restated here, not instantiated from Shader: a record needs the sample's E,
// direction and distance where Shader's loops hold them, and no existing kernel changes.  The
// operations and their order are Shader::point_light / rect_light / dome_light's
// (mrt_shader.h), which are the reference's:
//   point      src/PointLight.cpp:18-36 (L, nDotL, the SSE reciprocals), :38-48 (the fast shadow
//              ray, sampleHit.t = distance), :72, :80-81 (cosine, outSpec, E)
//   rectangle  src/RectangleLight.cpp:53-133: :56-59 (the draws, e2 capped, randDir), :61-80,
//              :82-92 (sampleHit.t = distance - epsilon), :119-122 (a sample that cannot be
//              hit still counts), :124-131 (E from the possibly stale falloff, the cut-off,
//              the sums), :135-136
//   dome       src/DomeLight.cpp:89-157: :93-105 (the draws, the table direction), :106 (a draw
//              below the horizon is redrawn uncounted; Shader's kDomeMaxRejects bound), :108-118
//              (pdf, image sample, sampleHit.t = MIRO_TMAX), :148-155, :159-160
// Transparent shadows (the `else` branches at PointLight.cpp:49, RectangleLight.cpp:93,
// DomeLight.cpp:123) are refused on the host.

// What PointLight::sampleLight forms before its shadow ray (src/PointLight.cpp:18-36, and the
// factors of :80-81), shared by gen and resolve so that both hold the same bits.  false: the
// light cannot be hit (nDotL <= 0), no sample.
struct PointTerms { v3 L; float distance, nDotL, A, rdl; };
__device__ __forceinline__ bool point_terms(const DevLight& l, v3 from, v3 normal, v3 rVec, const uint16_t* rcpT,
                                            const uint16_t* rsqT, PointTerms& t) {
    v3 L = sub(mk(l.pos[0], l.pos[1], l.pos[2]), from);
    float nDotL = dot(normal, L);
    if (!(nDotL > 0.0f)) return false;
    float falloff = dot(L, L);
    const float distanceRecip = rsqrt_nr(falloff, rsqT);
    falloff = rcp_nr(falloff, rcpT);
    t.distance = rcp_nr(distanceRecip, rcpT);
    t.L = scale(L, distanceRecip);
    nDotL *= distanceRecip;
    t.nDotL = nDotL;
    t.A = (l.power * falloff) * (0.25f / 3.1415926f);
    t.rdl = std_max(0.f, dot(rVec, t.L));
    return true;
}

struct LightPoint { v3 from, normal, rVec; float time; };
__device__ __forceinline__ LightPoint load_light_point(const LightQuery& Q, size_t i) {
    LightPoint p;
    p.from = mk(Q.from[3 * i], Q.from[3 * i + 1], Q.from[3 * i + 2]);
    p.normal = mk(Q.normal[3 * i], Q.normal[3 * i + 1], Q.normal[3 * i + 2]);
    p.rVec = mk(0, 0, 0);
    if (Q.rvec) p.rVec = mk(Q.rvec[3 * i], Q.rvec[3 * i + 1], Q.rvec[3 * i + 2]);
    p.time = Q.time ? Q.time[i] : 0.f;
    return p;
}

// Gen: one lane per point.  Draws exactly as Shader::sample_light does ("pixel" i, skey 0, from
// level_key(0) + first_draw).  Sample rows and ray slots are bounded by m on the host: a point
// light takes at most 1, a rectangle light max(1, samples), a dome light max(1, numSamples).
__global__ void __launch_bounds__(kWG) light_gen_kernel(RenderParams P, LightSamples G) {
    const LightQuery& Q = G.q;
    const uint16_t* rcpT = P.tables;          // a few per sample: global (L1-resident)
    const uint16_t* rsqT = P.tables + 2048;
    const size_t i = (size_t)blockIdx.x * kWG + threadIdx.x;
    uint32_t nray = 0;
    if (i < Q.n) {
        const LightPoint pt = load_light_point(Q, i);
        const v3 from = pt.from, normal = pt.normal, rVec = pt.rVec;
        const uint32_t pixel = (uint32_t)i;
        uint32_t dim = level_key(0) + Q.first_draw;
        const size_t row0 = i * (size_t)G.m;
        uint32_t ns = 0;
        auto next_rand = [&]() { return rng(pixel, 0u, dim++, P.seed); };
        // the sample's record; traced: its shadow ray into the point's next slot
        auto put = [&](v3 dir, float dist, v3 e, float aux, float vis, bool traced, float tMax) {
            mrt_light_sample r;
            r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
            r.dist = dist;
            r.e[0] = e.x; r.e[1] = e.y; r.e[2] = e.z;
            r.vis = traced ? kVisPending : vis;
            G.rec[row0 + ns] = r;
            G.aux[row0 + ns] = aux;
            ns++;
            if (traced) {
                P.ray_o[row0 + nray] = make_float4(from.x, from.y, from.z, tMax);
                P.ray_d[row0 + nray] = make_float4(dir.x, dir.y, dir.z, pt.time);
                nray++;
            }
        };
        for (int li = 0; li < P.n_lights; li++) {
            const DevLight& l = P.lights[li];
            int done = 0;
            if (l.type == MRT_POINT_LIGHT) {
                PointTerms t;
                if (point_terms(l, from, normal, rVec, rcpT, rsqT, t)) {
                    const float e = t.A * t.nDotL;   // A * (1 * nDotL): the light's E at vis = 1
                    put(t.L, t.distance, mk(e, e, e), t.rdl, 1.0f, l.cast_shadows != 0, t.distance);
                    done = 1;
                }
            } else if (l.type == MRT_DOME_LIGHT) {
                const DevDome& D = P.domes[l.dome];
                const int numSamples = Q.secondary ? 1 : l.samples;
                int rejects = 0;
                bool cut = false;
                do {
                    const float e1 = next_rand();
                    const float e2 = next_rand();
                    float pdf0, pdf1;
                    const float fu = dist_sample_guided(D.cdf_u, D.func_u, D.guide_u, D.nu, D.inv_int_u, e1, pdf0);
                    const int iu = (int)fu;
                    const int u = iu == D.nu ? iu - 1 : iu;
                    const size_t cv = (size_t)u * (D.nv + 1);
                    const float fv = dist_sample_guided(D.cdf_v + cv, D.func_v + (size_t)u * D.nv, D.guide_v + cv, D.nv,
                                                        D.inv_int_v[u], e2, pdf1);
                    const int iv = (int)fv;
                    const float cosT = D.cos_v[iv], sinT = D.sin_v[iv], sinP = D.sin_u[iu], cosP = D.cos_u[iu];
                    const v3 dir = mk(-sinT * cosP, -cosT, -sinT * sinP);
                    if (dot(normal, dir) < 0.0f) {
                        if (++rejects >= Shader<false, false>::kDomeMaxRejects) break;
                        continue;
                    }
                    const float pdf = (pdf0 * pdf1) / (kTwoPI2 * sinT);
                    const float4 rc = reinterpret_cast<const float4*>(D.rad)[(size_t)iv * (D.nu + 1) + iu];
                    const v3 img = mk(rc.x, rc.y, rc.z);
                    const float inv = 1.0f / pdf;
                    const v3 E = scale(scale(img, l.power), inv);
                    put(dir, 1e12f, E, dot(rVec, dir), 1.0f, true, 1e12f);   // a dome light always traces
                    done++;
                    const float recip = 1.0f / (float)done;
                    const v3 Es = scale(E, recip);
                    cut = (((Es.x + Es.y) + Es.z) * 0.333333f) < l.noise;
                } while (done < numSamples && !cut);
            } else {
                const v3 v1 = mk(l.v1[0], l.v1[1], l.v1[2]), v2 = mk(l.v2[0], l.v2[1], l.v2[2]), w3 = mk(l.v3[0], l.v3[1], l.v3[2]);
                float falloff = 1.0f;
                bool cut = false;
                do {
                    const float e1 = next_rand();
                    float e2 = next_rand();
                    e2 = ((double)e2 > 0.99) ? (float)0.99 : e2;
                    v3 rd = sub(add(add(v1, scale(sub(v2, v1), e1)), scale(sub(w3, v1), e2)), from);
                    const float nDotL = dot(normal, rd);
                    float dist = 0.0f, vis = 0.0f;   // a sample that cannot be hit: counted, never visible
                    bool traced = false;
                    if (nDotL > 0.001f) {
                        falloff = dot(rd, rd);
                        const float dr = rsqrt_nr(falloff, rsqT);
                        falloff = rcp_nr(falloff, rcpT);
                        dist = rcp_nr(dr, rcpT);
                        rd = scale(rd, dr);
                        vis = 1.0f;
                        traced = l.cast_shadows != 0;
                    }
                    const float E = (l.power * falloff) * (0.25f / 3.1415926f);
                    put(rd, dist, mk(E, E, E), std_max(0.f, dot(rVec, rd)), vis, traced, dist - 0.001f);
                    done++;
                    const float recip = 1.0f / (float)done;
                    const float Es = E * recip;
                    cut = ((Es + Es + Es) * 0.333333f) < l.noise;
                } while (done < l.samples && !cut);
            }
            G.counts[i * (size_t)P.n_lights + (size_t)li] = done;
        }
        P.nrays[i] = (uint8_t)nray;
    }
    // the traces of this query (every lane takes part in the wave's sum)
    TravStats st;
    flush_stats<false, false, false>(P, st, nray, threadIdx.x & 63, 0, 0);
}

// Resolve: one lane per point; its samples in order, a running ray index.  A pending vis
// becomes the trace's answer; each light's {E, outSpec} is formed with its loop's own sums
// (acc = add(acc, scale(E, att)), tmpSpec += factor * att, then 1.0f / (float)done -- the
// last recip the loop formed), a point light's from point_terms (attenuate = vis * nDotL);
// e is their sum in light order from 0.
__global__ void __launch_bounds__(kWG) light_resolve_kernel(RenderParams P, LightSamples G) {
    const LightQuery& Q = G.q;
    const size_t i = (size_t)blockIdx.x * kWG + threadIdx.x;
    if (i >= Q.n) return;
    const size_t row0 = i * (size_t)G.m;
    uint32_t s = 0, r = 0;
    auto answer = [&]() {   // the next sample's vis (stored into the caller's record where it was pending)
        float vis = G.rec[row0 + s].vis;
        if (vis == kVisPending) {
            vis = P.occl[row0 + r++] != 0 ? 0.0f : 1.0f;
            if (G.write_vis) G.rec[row0 + s].vis = vis;
        }
        return vis;
    };
    v3 sum = mk(0, 0, 0);
    for (int li = 0; li < P.n_lights; li++) {
        const DevLight& l = P.lights[li];
        const int done = G.counts[i * (size_t)P.n_lights + (size_t)li];
        v3 E = mk(0, 0, 0);
        float spec = 0.f;
        if (l.type == MRT_POINT_LIGHT) {
            if (done) {
                const float vis = answer();
                if (Q.e || Q.per_light) {
                    const LightPoint pt = load_light_point(Q, i);
                    PointTerms t;
                    point_terms(l, pt.from, pt.normal, pt.rVec, P.tables, P.tables + 2048, t);
                    float attenuate = vis;
                    attenuate *= t.nDotL;
                    spec = t.rdl * attenuate;
                    const float e = t.A * attenuate;
                    E = mk(e, e, e);
                }
                s++;
            }
        } else {
            v3 acc = mk(0, 0, 0);
            float tmpSpec = 0.f;
            for (int j = 0; j < done; j++) {
                const float att = answer();
                const mrt_light_sample& rec = G.rec[row0 + s];
                acc = add(acc, scale(mk(rec.e[0], rec.e[1], rec.e[2]), att));
                tmpSpec += G.aux[row0 + s] * att;
                s++;
            }
            const float recip = done ? 1.0f / (float)done : 1.0f;
            spec = tmpSpec * recip;
            E = scale(acc, recip);
        }
        sum = add(sum, E);
        if (Q.per_light) {
            float* o = Q.per_light + (i * (size_t)P.n_lights + (size_t)li) * 4;
            o[0] = E.x; o[1] = E.y; o[2] = E.z; o[3] = spec;
        }
    }
    if (Q.e) {
        float* o = Q.e + 3 * i;
        o[0] = sum.x; o[1] = sum.y; o[2] = sum.z;
    }
}

LightPassFn pick_light_gen() { return light_gen_kernel; }
LightPassFn pick_light_resolve() { return light_resolve_kernel; }

}  // namespace mrt
