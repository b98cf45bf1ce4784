// mrt_rec.hip -- instantiations of the fused chain kernels (Shader REC 1 / 2:
// Blinn reflection / refraction chains and path tracing traced inline) and of
// the adaptive supersampling kernels.  A translation unit of its own so the
// library's kernels compile in parallel (the shading code is mrt_shader.h).
#include "mrt_shader.h"

namespace mrt {

KernelFn pick_shade_rec(bool c, bool po, bool f, bool inst, int rec) {
    return with_ints<2, 1>(rec, [&](auto REC) { return shade_fn<REC()>(c, po, f, inst); });
}

// (special-leaf scenes take POINT_ONLY = false, as shade_fn)
template <int REC>
static KernelFn adaptive_fn(bool c, bool po, bool f, bool inst) {
    return with_bools([](auto I, auto PO, auto C, auto F) -> KernelFn {
        return adaptive_kernel<C(), PO() && !I(), F(), I(), REC>;
    }, inst, po, c, f);
}
// direct-lighting adaptive kernels (timed variants) at an occupancy target:
// unbounded, the compiler gives them all 256 VGPRs (one wave per SIMD)
template <int W>
static KernelFn adapt_direct(bool po, bool f, bool inst) {
    return with_bools([](auto I, auto PO, auto F) -> KernelFn {
        return adaptive_kernel<false, PO() && !I(), F(), I(), 0, W>;
    }, inst, po, f);
}

KernelFn pick_adaptive(bool c, bool po, bool f, bool inst, int rec) {
    if (rec == 0 && !c) return adapt_direct<6>(po, f, inst);   // 4 / 5 waves measured 6% / 1% slower on A3
    // (REC 1 / 2 kernels bounded to 2 or 3 waves still end at one: no variants)
    return with_ints<2, 1, 0>(rec, [&](auto REC) { return adaptive_fn<REC()>(c, po, f, inst); });
}

}  // namespace mrt
