// mrt_refit_dev.h -- internal: the box arithmetic the refit kernels (mrt_refit.hip) and the
// rebuild kernels (mrt_rebuild.hip) share.  Every box is a min / max merge in a fixed order
// (mrt_math.h std_min / std_max, as Builder::tri_aabb and merge).
#pragma once
#include <hip/hip_runtime.h>

#include "mrt_types.h"

namespace mrt {
namespace {

struct DBox {
    float lo[3], hi[3];
};
__device__ __forceinline__ DBox d_empty_box() {   // empty_box(): +-MIRO_TMAX
    return DBox{{1e12f, 1e12f, 1e12f}, {-1e12f, -1e12f, -1e12f}};
}
__device__ __forceinline__ DBox d_merge(const DBox& a, const DBox& b) {
    DBox r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = std_min(a.lo[k], b.lo[k]);
        r.hi[k] = std_max(a.hi[k], b.hi[k]);
    }
    return r;
}
// slot k of a node (SoA: min xyz, max xyz, four slots each) as a box, and back
__device__ __forceinline__ DBox d_slot_box(const QNode& q, int k) {
    return DBox{{q.box[0 + k], q.box[4 + k], q.box[8 + k]}, {q.box[12 + k], q.box[16 + k], q.box[20 + k]}};
}
__device__ __forceinline__ void d_store_slot(QNode& q, int k, const DBox& b) {
    q.box[0 + k] = b.lo[0]; q.box[4 + k] = b.lo[1]; q.box[8 + k] = b.lo[2];
    q.box[12 + k] = b.hi[0]; q.box[16 + k] = b.hi[1]; q.box[20 + k] = b.hi[2];
}
// box i of the float4 pairs (min xyz, max xyz) in lbox and fixed, and back
template <typename I>
__device__ __forceinline__ DBox d_load_box(const float4* p, I i) {
    const float4 lo = p[2 * i], hi = p[2 * i + 1];
    return DBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
}
template <typename I>
__device__ __forceinline__ void d_store_box(float4* p, I i, const DBox& b) {
    p[2 * (size_t)i] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.f);
    p[2 * (size_t)i + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.f);
}
// Builder::box3 of a triangle's vertices
__device__ __forceinline__ DBox d_tri_box(const float4 A, const float4 B, const float4 C) {
    return DBox{{std_min(A.x, std_min(B.x, C.x)), std_min(A.y, std_min(B.y, C.y)), std_min(A.z, std_min(B.z, C.z))},
                {std_max(A.x, std_max(B.x, C.x)), std_max(A.y, std_max(B.y, C.y)), std_max(A.z, std_max(B.z, C.z))}};
}

}  // namespace
}  // namespace mrt
