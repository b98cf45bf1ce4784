// mrt_rays.hip -- the ray-mode (RAYS) instantiations of the primary and shading
// kernels: Scene::sampleScene for caller rays (mrt_sample_rays).  The same kernels as
// a camera frame's two-launch / wavefront / fused-chain paths with the unit's ray
// loaded from the caller's arrays (item_pixel<true>, source_ray<true>) instead of made
// by the camera.  A translation unit of its own: the camera-frame instantiations are
// untouched and the library's kernels compile in parallel.  (The chain engine's are in
// mrt_chain.hip, shade1_kernel's in mrt_frame.hip, beside their kernels.)
#include "mrt_shader.h"

namespace mrt {

// The primary kernel at the default occupancy targets of a camera frame (7 waves; 5 for
// special-leaf scenes): the targets are a tuning matter, every variant gives the same bits.
template <int W, bool I, bool CHK, bool X>
static KernelFn primary_rays_fn(bool c, bool f) {
    return with_bools([](auto C, auto F) -> KernelFn { return primary_kernel<C(), W, F(), I, CHK, X, true>; }, c, f);
}
KernelFn pick_primary_rays(bool c, bool f, bool inst, bool check, bool xone) {
    if (inst) return check ? primary_rays_fn<5, true, true, false>(c, f) : primary_rays_fn<5, true, false, false>(c, f);
    return xone ? primary_rays_fn<7, false, true, true>(c, f) : primary_rays_fn<7, false, true, false>(c, f);
}

// fused shading (direct lighting, or rec 1 / 2: the chains traced inline)
KernelFn pick_shade_rays(bool c, bool po, bool f, bool inst, int rec) {
    return with_ints<2, 1, 0>(rec, [&](auto REC) { return shade_fn<REC(), true>(c, po, f, inst); });
}

// wavefront shadow passes 2a (gen) / 2c (resolve): no traversal, FAST unused
template <int MODE>
static KernelFn shade_mode_rays_fn(bool c, bool po, bool inst) {
    return with_bools([](auto I, auto PO, auto C) -> KernelFn {
        return shade_kernel<C(), PO() && !I(), false, I(), MODE, 0, 1, true>;
    }, inst, po, c);
}
KernelFn pick_shade_mode_rays(bool resolve, bool c, bool po, bool inst) {
    return resolve ? shade_mode_rays_fn<kResolve>(c, po, inst) : shade_mode_rays_fn<kGen>(c, po, inst);
}

}  // namespace mrt
