// Which kernel instantiation each pick function (csrc/mrt_pick.h) returns, over its whole
// argument domain: one line per call -- the function, the arguments, the mangled symbol of
// the returned kernel (dladdr on the host-side kernel handle).  Plain C++ linked against
// libmrt.so; calls no HIP function and needs no GPU.  tests/test_kernel_picks.py compares
// the output with tests/golden/kernel_picks.txt, recorded from the parent of the commit
// that last changed a pick.
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include <initializer_list>
#include <utility>
#include <vector>

namespace mrt {
struct RenderParams;
using KernelFn = void (*)(RenderParams);
using ShadowFn = void (*)(RenderParams, size_t, int, int);
KernelFn pick_primary(int w, int inst_waves, bool c, bool f, bool inst, bool check, bool xone);
KernelFn pick_shade(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_shade_mode(bool resolve, bool c, bool po, bool inst, bool bound);
ShadowFn pick_shadow(bool c, bool f, bool inst, bool refill, bool check);
KernelFn pick_frame1(int w, bool c, bool f, bool pow, int walk);
KernelFn pick_shade1(bool c, bool f, bool pow, bool rays);
KernelFn pick_shade_rec(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_adaptive(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_chain0(bool resolve, bool po, bool inst, int rec, bool rays);
KernelFn pick_chain_shade(bool resolve, bool po, bool inst, int rec, bool rays);
KernelFn pick_chain_trace(bool c, bool f, bool inst, int step, bool rays);
KernelFn pick_chain_compact();
KernelFn pick_chain_merge();
KernelFn pick_chain_fallback(bool po, bool inst, int rec, bool count, bool rays);
KernelFn pick_chain_finish(bool rays);
KernelFn pick_chain_fold();
KernelFn pick_unit_eye(bool c, bool f, bool inst);
KernelFn pick_adapt_combine();
KernelFn pick_primary_rays(bool c, bool f, bool inst, bool check, bool xone);
KernelFn pick_shade_rays(bool c, bool po, bool f, bool inst, int rec);
KernelFn pick_shade_mode_rays(bool resolve, bool c, bool po, bool inst);
}  // namespace mrt
using namespace mrt;

using Dom = std::vector<int>;
static const Dom B{0, 1};   // a bool, both ways

template <class R, class... A, size_t... I>
static R call(R (*fn)(A...), const int* v, std::index_sequence<I...>) { return fn(static_cast<A>(v[I])...); }

// fn over the cross product of its arguments' domains, the last argument varying fastest
template <class R, class... A>
static void sweep(const char* name, R (*fn)(A...), std::initializer_list<Dom> doms) {
    const std::vector<Dom> d(doms);
    std::vector<size_t> at(d.size(), 0);
    while (true) {
        int v[8] = {0};
        for (size_t i = 0; i < d.size(); i++) v[i] = d[i][at[i]];
        const R r = call(fn, v, std::index_sequence_for<A...>{});
        Dl_info info{};
        const bool ok = dladdr(reinterpret_cast<void*>(r), &info) && info.dli_sname && info.dli_saddr == reinterpret_cast<void*>(r);
        printf("%s(", name);
        for (size_t i = 0; i < d.size(); i++) printf("%s%d", i ? ", " : "", v[i]);
        printf(") -> %s\n", ok ? info.dli_sname : "?");
        size_t i = d.size();
        while (i > 0 && ++at[i - 1] == d[i - 1].size()) at[--i] = 0;
        if (i == 0) break;
    }
}

int main() {
    const Dom rec{0, 1, 2}, chain_rec{1, 2}, step{0, 1, 2};
    // each occupancy / walk table's listed values and one it does not list (the default's case)
    const Dom primary_w{1, 5, 6, 7, 8}, inst_w{1, 4, 5, 6, 7}, frame_w{1, 4, 5, 6, 7, 8}, walk{0, 1, 2, 3, 4};
    sweep("pick_primary", pick_primary, {primary_w, inst_w, B, B, B, B, B});
    sweep("pick_shade", pick_shade, {B, B, B, B, rec});
    sweep("pick_shade_mode", pick_shade_mode, {B, B, B, B, B});
    sweep("pick_shadow", pick_shadow, {B, B, B, B, B});
    sweep("pick_frame1", pick_frame1, {frame_w, B, B, B, walk});
    sweep("pick_shade1", pick_shade1, {B, B, B, B});
    sweep("pick_shade_rec", pick_shade_rec, {B, B, B, B, rec});
    sweep("pick_adaptive", pick_adaptive, {B, B, B, B, rec});
    sweep("pick_chain0", pick_chain0, {B, B, B, chain_rec, B});
    sweep("pick_chain_shade", pick_chain_shade, {B, B, B, chain_rec, B});
    sweep("pick_chain_trace", pick_chain_trace, {B, B, B, step, B});
    sweep("pick_chain_compact", pick_chain_compact, {});
    sweep("pick_chain_merge", pick_chain_merge, {});
    sweep("pick_chain_fallback", pick_chain_fallback, {B, B, chain_rec, B, B});
    sweep("pick_chain_finish", pick_chain_finish, {B});
    sweep("pick_chain_fold", pick_chain_fold, {});
    sweep("pick_unit_eye", pick_unit_eye, {B, B, B});
    sweep("pick_adapt_combine", pick_adapt_combine, {});
    sweep("pick_primary_rays", pick_primary_rays, {B, B, B, B, B});
    sweep("pick_shade_rays", pick_shade_rays, {B, B, B, B, rec});
    sweep("pick_shade_mode_rays", pick_shade_mode_rays, {B, B, B, B});
    return 0;
}
