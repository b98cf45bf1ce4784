// mrt_pick.h -- which kernel instantiation a launch runs.  Every kernel family is a
// template over compile-time switches; a pick function maps a launch's run-time
// arguments to one instantiation.  The picks are pure functions with external linkage,
// so tests/native/kernel_picks.cpp can call each over its whole domain without a GPU
// ("Kernel variants").
#pragma once
#include <cstddef>
#include <type_traits>

namespace mrt {

struct RenderParams;
using KernelFn = void (*)(RenderParams);
using ShadowFn = void (*)(RenderParams, size_t, int, int);
struct LightQuery;
using LightFn = void (*)(RenderParams, LightQuery);
struct LightSamples;
using LightPassFn = void (*)(RenderParams, LightSamples);

// Run-time bools to compile-time constants: with_bools(f, a, b) calls f(A, B) with
// std::true_type / std::false_type values, so a generic lambda names the instantiation
// once --  with_bools([](auto C, auto F) -> KernelFn { return k<C(), F()>; }, c, f)  --
// and every combination is instantiated, the first bool varying slowest.
template <class F>
static auto with_bools(F f) { return f(); }
template <class F, class... Bs>
static auto with_bools(F f, bool b, Bs... rest) {
    return b ? with_bools([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...)
             : with_bools([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}
// The integer counterpart, for occupancy targets and walk forms: with_ints<6, 7, 8, 1>(w, f)
// calls f(std::integral_constant<int, V>) for the listed V equal to w, else for the last one.
template <int V, int... Vs, class F>
static auto with_ints(int w, F f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else return w == V ? f(std::integral_constant<int, V>{}) : with_ints<Vs...>(w, f);
}

// c: count mode (visit statistics); f: the hierarchy's boxes are finite (FAST walks);
// po: point lights only; inst: a special-leaf scene (instances, alpha maps, motion blur);
// rec: Shader REC (0 direct, 1 reflection / refraction chains, 2 + path tracing);
// rays: the ray-mode instantiations (the work units are a caller's rays)

// mrt_device.hip: the primary kernel at an occupancy target (w; inst_waves for special-leaf
// scenes), the fused shading kernel, the wavefront shadow passes 2a / 2c and 2b
KernelFn pick_primary(int w, int inst_waves, bool c, bool f, bool inst, bool check, bool xone);
KernelFn pick_shade(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_shade_mode(bool resolve, bool c, bool po, bool inst, bool bound);
ShadowFn pick_shadow(bool c, bool f, bool inst, bool refill, bool check);
// mrt_frame.hip: the one-point-light frame / shade kernels at an occupancy target w;
// pow: a Blinn material with specExp != 1
KernelFn pick_frame1(int w, bool c, bool f, bool pow, int walk);
KernelFn pick_shade1(bool c, bool f, bool pow, bool rays = false);
// mrt_rec.hip: the fused chain kernels (rec 1, 2) and the adaptive supersampling kernels (any rec)
KernelFn pick_shade_rec(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_adaptive(bool c, bool po, bool f, bool inst, int rec);
// mrt_chain.hip: the wavefront chain engine
KernelFn pick_chain0(bool resolve, bool po, bool inst, int rec, bool rays = false);
KernelFn pick_chain_shade(bool resolve, bool po, bool inst, int rec, bool rays = false);
KernelFn pick_chain_trace(bool c, bool f, bool inst, int step, bool rays = false);
KernelFn pick_chain_compact();
KernelFn pick_chain_merge();
KernelFn pick_chain_fallback(bool po, bool inst, int rec, bool count, bool rays = false);
KernelFn pick_chain_finish(bool rays = false);
KernelFn pick_chain_fold();
KernelFn pick_unit_eye(bool c, bool f, bool inst);
KernelFn pick_adapt_combine();
// mrt_rays.hip: the ray-mode instantiations of the primary / shading kernels
KernelFn pick_primary_rays(bool c, bool f, bool inst, bool check, bool xone);
KernelFn pick_shade_rays(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_shade_mode_rays(bool resolve, bool c, bool po, bool inst);
// mrt_lights.hip: Light::sampleLight at caller points (mrt_sample_lights).  check: the special-leaf
// scene has alpha-mapped or motion-blurred lanes; xp: a rectangle / dome light with transparent
// shadows (the transparency walk, compiled into these variants only)
LightFn pick_light_points(bool c, bool f, bool inst, bool check, bool xp);
// mrt_lights.hip: the gen and resolve passes of mrt_light_samples (one lane per point, no
// traversal: one instantiation each; the trace between them is pick_shadow's)
LightPassFn pick_light_gen();
LightPassFn pick_light_resolve();
// mrt_relight.hip: the device build of a dome light's tables after mrt_scene_update_texture (one
// instantiation each) -- the column scans, the column normalisation with its guide tables, the
// row scan with the int_u test, the rad cells, the gated commits of the tables and the texels --
// and the store of light / material records that arrive as a kernel argument
struct DomeBuild;
using DomeFn = void (*)(DomeBuild);
struct RelightWords;
using RelightFn = void (*)(unsigned*, RelightWords, int);
DomeFn pick_dome_scan();
DomeFn pick_dome_guide();
DomeFn pick_dome_row();
DomeFn pick_dome_rad();
DomeFn pick_dome_commit();
DomeFn pick_tex_commit();
RelightFn pick_relight_store();

}  // namespace mrt
