// mrt_refit.hip -- mrt_scene_update_mesh: new vertices for a world mesh, same topology, and
// the world hierarchy refitted on the device: a scatter of the vertices into the mesh's
// slice, one leaf kernel (triangles A, B-A, C-A and one box per packet) and one node kernel
// launch per height, deepest first.  Every box is a min / max merge in a fixed order
// (mrt_math.h std_min / std_max, as Builder::tri_aabb and merge): the result is stated bit
// for bit by refit_host (host_build.cpp) and by tests/test_refit.py's numpy restatement.
// mrt_scene_update_instances: new matrices for ProxyObject instances; one kernel restates
// add_instance's arithmetic per instance (inverse, inverse transpose, box), then the same
// leaf and node kernels.
// mrt_scene_deform_mesh: new vertices for any mesh.  A mesh of a BLAS: the same leaf and node
// kernels over that BLAS's range, one kernel that recomputes the box of each of its instances
// from the refitted root, then the world tree.  A motion-blurred world mesh: both vertex sets,
// one kernel that recomputes the union box of each of its MBObject lanes, then the world tree.
// One pipeline serves them all: a RefitTree (mrt_image.h) is the world or a BLAS, with one
// height_schedule, enqueue_tree and read_tree for either; enqueue_mesh is the launch sequence
// of every mesh entry, refit_replicas the per-replica loop of every synchronous entry and
// async_ready what every async entry asks of the scene.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mrt_device.h"
#include "mrt_kernels.h"
#include "mrt_refit_dev.h"

namespace mrt {

namespace {

constexpr int kRefitWG = 256;

// n packed (x, y, z) -> float4 (x, y, z, w) at dst (and dst2: the time-1 copy of a static mesh)
__global__ __launch_bounds__(kRefitWG) void refit_scatter_kernel(float4* __restrict__ dst, float4* __restrict__ dst2,
                                                                 const float* __restrict__ src, uint32_t n, float w) {
    const uint32_t i = blockIdx.x * kRefitWG + threadIdx.x;
    if (i >= n) return;
    const float* p = src + (size_t)i * 3;
    const float4 v = make_float4(p[0], p[1], p[2], w);
    dst[i] = v;
    if (dst2) dst2[i] = v;
}

// One lane per packet lane of the world DLeaf range (n_lanes = 4 x packets, so the four
// lanes of a packet are in one wave and all inside or all outside the range).
__global__ __launch_bounds__(kRefitWG) void refit_leaf_kernel(DLeaf* __restrict__ leaves, uint32_t n_lanes,
                                                              const PrimShade* __restrict__ prims,
                                                              const float4* __restrict__ verts,
                                                              const uint8_t* __restrict__ pflags,
                                                              const int32_t* __restrict__ mbslot,
                                                              const float4* __restrict__ fixed, int n_insts,
                                                              float4* __restrict__ lbox) {
    const uint32_t g = blockIdx.x * kRefitWG + threadIdx.x;
    const bool in = g < n_lanes;
    const uint32_t leaf = g >> 2, k = g & 3u;
    DBox b = d_empty_box();
    int used = 0;
    if (in) {
        const int32_t prim = leaves[leaf].prim[k];
        int fx = -1;   // a ProxyObject lane: its instance's box now; an MBObject lane: its box of the build
        if (prim <= -2) fx = -2 - prim;
        else if (prim >= 0 && pflags && (pflags[prim] & 1u)) fx = n_insts + mbslot[prim];
        if (fx >= 0) {
            b = d_load_box(fixed, fx);
            used = 1;
        } else if (prim >= 0) {
            const PrimShade ps = prims[prim];
            const float4 A = verts[ps.v[0]], B = verts[ps.v[1]], C = verts[ps.v[2]];
            float* t = leaves[leaf].tri[k];   // make_leaf: A, B - A, C - A
            t[0] = A.x; t[1] = A.y; t[2] = A.z;
            t[3] = B.x - A.x; t[4] = B.y - A.y; t[5] = B.z - A.z;
            t[6] = C.x - A.x; t[7] = C.y - A.y; t[8] = C.z - A.z;
            b = d_tri_box(A, B, C);
            used = 1;
        }
    }
    // the packet's box: its used lanes merged in lane order from the empty box
    DBox acc = d_empty_box();
    for (int j = 0; j < 4; j++) {
        DBox o;
        for (int a = 0; a < 3; a++) {
            o.lo[a] = __shfl(b.lo[a], j, 4);
            o.hi[a] = __shfl(b.hi[a], j, 4);
        }
        if (__shfl(used, j, 4)) acc = d_merge(acc, o);
    }
    if (in && k == 0) d_store_box(lbox, leaf, acc);
}

// One lane per slot of the n nodes of one height (order[0 .. n)): a leaf slot takes its
// packet's box, an inner slot the merge of that child's used slots in slot order (the
// child is of a smaller height: an earlier launch wrote it).  Empty slots, the child words
// and the slot kinds are not touched.
__global__ __launch_bounds__(kRefitWG) void refit_node_kernel(QNode* __restrict__ nodes,
                                                              const int32_t* __restrict__ order, uint32_t n,
                                                              const float4* __restrict__ lbox) {
    const uint32_t g = blockIdx.x * kRefitWG + threadIdx.x;
    if (g >= 4u * n) return;
    const uint32_t k = g & 3u;
    QNode* q = nodes + order[g >> 2];
    const int32_t c = q->child[k];
    if (c == kEmptySlot) return;
    DBox b;
    if (c < 0) {
        b = d_load_box(lbox, (size_t)(~(uint32_t)c >> 4));   // leaf_child
    } else {
        const QNode* ch = nodes + c;
        b = d_empty_box();
        for (int j = 0; j < 4; j++)
            if (ch->child[j] != kEmptySlot) b = d_merge(b, d_slot_box(*ch, j));
    }
    d_store_slot(*q, (int)k, b);
}

// Matrix4x4::invert as inverse() of host_build.cpp states it, operation for operation: the 18
// 2x2 terms, the 16 3x3 sums, det, 1 / det in double (a correctly rounded f64 divide, then
// one rounding to float) and the signed cofactors times it.
__device__ void d_inverse(const float (&a)[4][4], float (&R)[4][4]) {
    auto t2 = [](float p, float q, float r, float s) { return p * q - r * s; };
    const float T34_12 = t2(a[2][0], a[3][1], a[2][1], a[3][0]), T34_13 = t2(a[2][0], a[3][2], a[2][2], a[3][0]);
    const float T34_14 = t2(a[2][0], a[3][3], a[2][3], a[3][0]), T34_23 = t2(a[2][1], a[3][2], a[2][2], a[3][1]);
    const float T34_24 = t2(a[2][1], a[3][3], a[2][3], a[3][1]), T34_34 = t2(a[2][2], a[3][3], a[2][3], a[3][2]);
    const float T24_12 = t2(a[1][0], a[3][1], a[1][1], a[3][0]), T24_13 = t2(a[1][0], a[3][2], a[1][2], a[3][0]);
    const float T24_14 = t2(a[1][0], a[3][3], a[1][3], a[3][0]), T24_23 = t2(a[1][1], a[3][2], a[1][2], a[3][1]);
    const float T24_24 = t2(a[1][1], a[3][3], a[1][3], a[3][1]), T24_34 = t2(a[1][2], a[3][3], a[1][3], a[3][2]);
    const float T23_12 = t2(a[1][0], a[2][1], a[1][1], a[2][0]), T23_13 = t2(a[1][0], a[2][2], a[1][2], a[2][0]);
    const float T23_14 = t2(a[1][0], a[2][3], a[1][3], a[2][0]), T23_23 = t2(a[1][1], a[2][2], a[1][2], a[2][1]);
    const float T23_24 = t2(a[1][1], a[2][3], a[1][3], a[2][1]), T23_34 = t2(a[1][2], a[2][3], a[1][3], a[2][2]);
    auto s3 = [](float p, float q, float r, float s, float u, float v) { return p * q - r * s + u * v; };
    const float sd[4][4] = {
        {s3(a[1][1], T34_34, a[1][2], T34_24, a[1][3], T34_23), s3(a[1][0], T34_34, a[1][2], T34_14, a[1][3], T34_13),
         s3(a[1][0], T34_24, a[1][1], T34_14, a[1][3], T34_12), s3(a[1][0], T34_23, a[1][1], T34_13, a[1][2], T34_12)},
        {s3(a[0][1], T34_34, a[0][2], T34_24, a[0][3], T34_23), s3(a[0][0], T34_34, a[0][2], T34_14, a[0][3], T34_13),
         s3(a[0][0], T34_24, a[0][1], T34_14, a[0][3], T34_12), s3(a[0][0], T34_23, a[0][1], T34_13, a[0][2], T34_12)},
        {s3(a[0][1], T24_34, a[0][2], T24_24, a[0][3], T24_23), s3(a[0][0], T24_34, a[0][2], T24_14, a[0][3], T24_13),
         s3(a[0][0], T24_24, a[0][1], T24_14, a[0][3], T24_12), s3(a[0][0], T24_23, a[0][1], T24_13, a[0][2], T24_12)},
        {s3(a[0][1], T23_34, a[0][2], T23_24, a[0][3], T23_23), s3(a[0][0], T23_34, a[0][2], T23_14, a[0][3], T23_13),
         s3(a[0][0], T23_24, a[0][1], T23_14, a[0][3], T23_12), s3(a[0][0], T23_23, a[0][1], T23_13, a[0][2], T23_12)}};
    const float det = a[0][0] * sd[0][0] - a[0][1] * sd[0][1] + a[0][2] * sd[0][2] - a[0][3] * sd[0][3];
    const float di = (float)(1.0 / (double)det);
    // R(r,c) = (-1)^(r+c) * sd[c][r] * di
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) R[r][c] = (((r + c) & 1) ? -sd[c][r] : sd[c][r]) * di;
}

// DPPS 0xFF on (x, y, z, 1): (p0 + p1) + (p2 + p3)
__device__ __forceinline__ float d_dp4(const float (&row)[4], float x, float y, float z) {
    const float p0 = row[0] * x, p1 = row[1] * y, p2 = row[2] * z, p3 = row[3] * 1.0f;
    return (p0 + p1) + (p2 + p3);
}

// ProxyObject::getAABB as add_instance states it: the BLAS root's four slot boxes merged from
// the empty box (unused zero boxes included), the corners A..F, bbMin, bbMax through
// multiplyAndDivideByW (xform_point: rcp_nr of the w dot, three multiplies), grown in order.
__device__ DBox d_instance_box(const float (&m)[4][4], const QNode& r, const uint16_t* __restrict__ rcpT) {
    DBox t = d_empty_box();
    for (int k = 0; k < 4; k++)
        t = d_merge(t, d_slot_box(r, k));
    const float* lo = t.lo;
    const float* hi = t.hi;
    const float P[8][3] = {{lo[0], lo[1], hi[2]}, {lo[0], hi[1], lo[2]}, {hi[0], lo[1], lo[2]}, {lo[0], hi[1], hi[2]},
                           {hi[0], hi[1], lo[2]}, {hi[0], lo[1], hi[2]}, {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
    DBox nb = d_empty_box();
    for (int j = 0; j < 8; j++) {
        const float x = P[j][0], y = P[j][1], z = P[j][2];
        const float w = rcp_nr(d_dp4(m[3], x, y, z), rcpT);
        const float q[3] = {w * d_dp4(m[0], x, y, z), w * d_dp4(m[1], x, y, z), w * d_dp4(m[2], x, y, z)};
        nb = d_merge(nb, DBox{{q[0], q[1], q[2]}, {q[0], q[1], q[2]}});
    }
    return nb;
}

// instance i's box from its matrix and its BLAS root, into the fixed boxes the leaf kernel reads
__device__ __forceinline__ void d_fix_instance_box(float4* __restrict__ fixed, size_t i, const float (&m)[4][4],
                                                   const QNode& root, const uint16_t* __restrict__ rcpT) {
    d_store_box(fixed, i, d_instance_box(m, root, rcpT));
}

// ProxyMatrix::set for n instances, one lane each: lane g takes the row-major 4x4 at
// m16s + 16 g for instance ids[g] (ids == nullptr: first + g; the host checked the ids) and
// writes its inverse and inverse transpose into insts, the matrix into inst_m and its box
// into the fixed boxes the leaf kernel reads.  The RCPSS table comes from global memory:
// eight lookups per lane do not pay for staging 4 KB in LDS.
__global__ __launch_bounds__(kRefitWG) void refit_instance_kernel(DevInstance* __restrict__ insts, float* __restrict__ inst_m,
                                                                  float4* __restrict__ fixed,
                                                                  const QNode* __restrict__ nodes,
                                                                  const uint16_t* __restrict__ rcpT,
                                                                  const float* __restrict__ m16s,
                                                                  const int32_t* __restrict__ ids, int32_t first, uint32_t n) {
    const uint32_t g = blockIdx.x * kRefitWG + threadIdx.x;
    if (g >= n) return;
    const size_t i = (size_t)(ids ? ids[g] : first + (int32_t)g);
    float m[4][4], inv[4][4];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) m[r][c] = m16s[(size_t)g * 16 + 4 * r + c];
    d_inverse(m, inv);
    DevInstance& I = insts[i];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            I.inv[4 * r + c] = inv[r][c];
            if (r < 3) I.inv_t[4 * r + c] = inv[c][r];
            inst_m[i * 16 + 4 * r + c] = m[r][c];
        }
    d_fix_instance_box(fixed, i, m, nodes[I.root], rcpT);
}

// The box half alone for the n instances ids[0 .. n) of one BLAS whose root was just refitted:
// lane g reads instance ids[g]'s m_transform from inst_m and writes its box.  inv, inv_t and
// the matrix stay.  The RCPSS table comes from global memory, as in refit_instance_kernel.
__global__ __launch_bounds__(kRefitWG) void refit_instance_box_kernel(float4* __restrict__ fixed,
                                                                      const DevInstance* __restrict__ insts,
                                                                      const float* __restrict__ inst_m,
                                                                      const QNode* __restrict__ nodes,
                                                                      const uint16_t* __restrict__ rcpT,
                                                                      const int32_t* __restrict__ ids, uint32_t n) {
    const uint32_t g = blockIdx.x * kRefitWG + threadIdx.x;
    if (g >= n) return;
    const size_t i = (size_t)ids[g];
    float m[4][4];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) m[r][c] = inst_m[i * 16 + 4 * r + c];
    d_fix_instance_box(fixed, i, m, nodes[insts[i].root], rcpT);
}

// MBObject::getAABB for the n world prims first .. first + n - 1 (one motion-blurred mesh), one
// lane each: box3 of the time-0 vertices merged with box3 of the time-1 vertices
// (fixed_lane_box), into the prim's fixed box.
__global__ __launch_bounds__(kRefitWG) void refit_motion_box_kernel(float4* __restrict__ fixed, int n_insts,
                                                                    const int32_t* __restrict__ mbslot,
                                                                    const uint8_t* __restrict__ pflags,
                                                                    const PrimShade* __restrict__ prims,
                                                                    const float4* __restrict__ verts,
                                                                    const float4* __restrict__ verts2, uint32_t first,
                                                                    uint32_t n) {
    const uint32_t g = blockIdx.x * kRefitWG + threadIdx.x;
    if (g >= n) return;
    const size_t p = (size_t)first + g;
    if (!(pflags[p] & 1u)) return;
    const int32_t slot = mbslot[p];
    if (slot < 0) return;
    const PrimShade ps = prims[p];
    auto box3 = [&](const float4* __restrict__ v) { return d_tri_box(v[ps.v[0]], v[ps.v[1]], v[ps.v[2]]); };
    const DBox b = d_merge(box3(verts), box3(verts2));
    const size_t f = (size_t)n_insts + (size_t)slot;
    d_store_box(fixed, f, b);
}

// The height schedule of tree T (`what` in the messages) from its canonical nodes N and n_leaves
// packets: T.off by height and, appended to `order`, the nodes sorted by height in device
// numbers (perm[i]; perm empty: T.node_base + i).  Every child has a larger canonical number
// than its parent (qbuild).
int height_schedule(const std::vector<QNode>& N, size_t n_leaves, const std::vector<int32_t>& perm, const char* what,
                    RefitTree& T, std::vector<int32_t>& order) {
    const size_t n = N.size();
    if (n != T.n_nodes || n_leaves != T.n_leaves) { set_error("refit: replica out of date"); return MRT_ERR_INVALID; }
    std::vector<int32_t> height(n, 0);
    int32_t top = 0;
    for (size_t i = n; i-- > 0;) {
        int32_t h = 0;
        for (int k = 0; k < 4; k++) {
            const int32_t c = N[i].child[k];
            if (c < 0) continue;
            if ((size_t)c <= i || (size_t)c >= n) { set_error(std::string("refit: ") + what + " is not a tree in build order"); return MRT_ERR_INVALID; }
            h = std::max(h, height[(size_t)c] + 1);
        }
        height[i] = h;
        top = std::max(top, h);
    }
    T.off.assign((size_t)top + 2, 0);
    for (size_t i = 0; i < n; i++) T.off[(size_t)height[i] + 1]++;
    for (size_t h = 0; h + 1 < T.off.size(); h++) T.off[h + 1] += T.off[h];
    const size_t first = order.size();
    order.resize(first + n);
    std::vector<uint32_t> at(T.off.begin(), T.off.end() - 1);
    for (size_t i = 0; i < n; i++) order[first + at[(size_t)height[i]]++] = perm.empty() ? (int32_t)(T.node_base + i) : perm[i];
    return MRT_OK;
}

// The height schedules of replica d: the world's nodes by height, then each BLAS's (BLAS nodes
// are not permuted), uploaded as refit_order (an earlier list is released: the caller has
// synchronised the device if one was in use).
int make_schedule(const Scene& s, DeviceState& d) {
    int rc;
    std::vector<int32_t> order;
    if ((rc = height_schedule(s.nodes, s.leaves.size(), d.node_perm, "the hierarchy", d.world, order))) return rc;
    if (d.blas.size() != s.blas.size() || d.n_leaves_all < d.world.n_leaves) { set_error("refit: replica out of date"); return MRT_ERR_INVALID; }
    for (size_t b = 0; b < s.blas.size(); b++)
        if ((rc = height_schedule(s.blas[b].nodes, s.blas[b].leaves.size(), {}, "a BLAS hierarchy", d.blas[b].tree, order))) return rc;
    d.own.release(d.refit_order);
    d.refit_order = nullptr;
    if ((rc = d.own.upload(d.refit_order, order.data(), order.size() * sizeof(int32_t)))) return rc;
    d.world.order = d.refit_order;   // each tree's part of the one list
    const int32_t* at = d.refit_order + d.world.n_nodes;
    for (DeviceState::BlasRange& R : d.blas) {
        R.tree.order = at;
        at += R.tree.n_nodes;
    }
    d.sched_stale = false;
    return MRT_OK;
}

// What the refit of replica d needs beyond the upload, made once: the node lists by height in
// device numbers (made again after a rebuild, which alone changes a topology while the replica
// lives), the packet box scratch and the fixed boxes of ProxyObject / MBObject lanes.  The
// current device is d's.
int prepare(const Scene& s, DeviceState& d) {
    if (d.refit_ready) return d.sched_stale ? make_schedule(s, d) : MRT_OK;
    int rc;
    if ((rc = make_schedule(s, d))) return rc;
    // fixed boxes: instance i at i, then the MBObject lanes
    std::vector<float4> fixed;
    auto push_box = [&](const float* b) {
        fixed.push_back(make_float4(b[0], b[1], b[2], 0.f));
        fixed.push_back(make_float4(b[3], b[4], b[5], 0.f));
    };
    for (const Instance& I : s.instances) push_box(I.box);
    std::vector<int32_t> mbslot;
    if (d.has_mb) {
        mbslot.assign(s.obj_mesh.size(), -1);
        int32_t next = 0;
        for (size_t o = 0; o < s.obj_mesh.size(); o++) {
            float b[6];
            if (s.obj_inst[o] >= 0 || !fixed_lane_box(s, (int32_t)o, b)) continue;
            mbslot[o] = next++;
            push_box(b);
        }
    }
    std::vector<float> inst_m(16 * s.instances.size());   // m_transform: the device keeps inv / inv_t only
    for (size_t i = 0; i < s.instances.size(); i++) memcpy(&inst_m[16 * i], s.instances[i].m, 16 * sizeof(float));
    // each BLAS: the ids of its instances
    std::vector<int32_t> binsts;
    for (size_t b = 0; b < s.blas.size(); b++) {
        DeviceState::BlasRange& R = d.blas[b];
        R.inst_at = (uint32_t)binsts.size();
        for (size_t i = 0; i < s.instances.size(); i++)
            if (s.instances[i].blas == (int32_t)b) binsts.push_back((int32_t)i);
        R.n_inst = (uint32_t)binsts.size() - R.inst_at;
    }
    if ((rc = d.own.upload(d.refit_fixed, fixed.data(), fixed.size() * sizeof(float4))) ||
        (rc = d.own.upload(d.refit_mbslot, mbslot.data(), mbslot.size() * sizeof(int32_t))) ||
        (rc = d.own.upload(d.refit_inst_m, inst_m.data(), inst_m.size() * sizeof(float))) ||
        (rc = d.own.upload(d.refit_blas_insts, binsts.data(), binsts.size() * sizeof(int32_t))))
        return rc;
    d.mesh_prim0.assign(s.meshes.size(), -1);   // first prim of each world mesh
    for (size_t o = s.obj_mesh.size(); o-- > 0;)
        if (s.obj_mesh[o] >= 0) d.mesh_prim0[(size_t)s.obj_mesh[o]] = (int32_t)o;
    // the packet boxes of the world and of every BLAS, by device packet number (the child words' own)
    if ((rc = d.own.alloc(d.refit_lbox, std::max<size_t>(1, d.n_leaves_all) * 2 * sizeof(float4))) ||
        (rc = d.own.event(d.refit_ev0)) || (rc = d.own.event(d.refit_ev1)))
        return rc;
    d.refit_ready = true;
    return MRT_OK;
}

inline dim3 blocks(size_t n) { return dim3((unsigned)((n + kRefitWG - 1) / kRefitWG)); }

// Enqueue on `stream`: tree T refitted to the vertices (and, the world, the fixed boxes) the
// device holds now: the leaf kernel over its packets, then the node kernels, deepest height first.
void enqueue_tree(DeviceState& d, const RefitTree& T, hipStream_t stream) {
    const uint32_t n_lanes = 4u * T.n_leaves;
    if (n_lanes)
        hipLaunchKernelGGL(refit_leaf_kernel, blocks(n_lanes), dim3(kRefitWG), 0, stream, d.leaves + T.leaf_base, n_lanes,
                           (const PrimShade*)(d.prims + T.shade_base), (const float4*)d.verts,
                           (const uint8_t*)(T.fixed_lanes && d.has_mb ? d.pflags : nullptr),
                           (const int32_t*)(T.fixed_lanes ? d.refit_mbslot : nullptr), (const float4*)d.refit_fixed,
                           d.n_insts, d.refit_lbox + 2 * (size_t)T.leaf_base);
    for (size_t h = 0; h + 1 < T.off.size(); h++) {
        const uint32_t n = T.off[h + 1] - T.off[h];
        if (!n) continue;
        hipLaunchKernelGGL(refit_node_kernel, blocks((size_t)4 * n), dim3(kRefitWG), 0, stream, d.nodes, T.order + T.off[h],
                           n, (const float4*)d.refit_lbox);
    }
}

// the world tree, last in every entry's sequence: a launch that failed shows here
int enqueue_world(DeviceState& d, hipStream_t stream) {
    enqueue_tree(d, d.world, stream);
    HIP_OK(hipGetLastError());
    return MRT_OK;
}

// Enqueue on `stream`: n matrices (device, row-major 4x4 each) for the instances d_ids[0 .. n)
// (nullptr: first .. first + n - 1), then the tree.  The ids are in [0, d.n_insts).
int enqueue_instances(DeviceState& d, const float* d_m16s, const int32_t* d_ids, int32_t first, uint32_t n,
                      hipStream_t stream) {
    if (n)
        hipLaunchKernelGGL(refit_instance_kernel, blocks(n), dim3(kRefitWG), 0, stream, d.insts, d.refit_inst_m,
                           d.refit_fixed, (const QNode*)d.nodes, (const uint16_t*)d.tables, d_m16s, d_ids, first, n);
    return enqueue_world(d, stream);
}

// Enqueue on `stream` for mesh m of `kind` (deform_check; blas: the mesh's BLAS): nv vertices
// (kDeformMotion: and the time-1 set) and nn normals (d_normals == nullptr: kept) scattered
// from packed device arrays into the mesh's slices; then, for a mesh of a BLAS, that BLAS's
// tree and the boxes of its instances, for a motion-blurred mesh the boxes of its nt MBObject
// lanes; then the world tree.
int enqueue_mesh(DeviceState& d, int m, int kind, int blas, const float* d_verts, const float* d_verts2, uint32_t nv,
                 const float* d_normals, uint32_t nn, uint32_t nt, hipStream_t stream) {
    auto scatter = [&](float4* dst, float4* dst2, const float* src, uint32_t n, float w) {
        if (n) hipLaunchKernelGGL(refit_scatter_kernel, blocks(n), dim3(kRefitWG), 0, stream, dst, dst2, src, n, w);
    };
    const bool motion = kind == kDeformMotion && d.has_mb;
    const size_t vb = d.vbase[(size_t)m];
    // a static mesh's time-1 copy follows; a motion-blurred one has its own set
    scatter(d.verts + vb, d.has_mb && kind != kDeformMotion ? d.verts2 + vb : nullptr, d_verts, nv, 1.f);
    if (motion) scatter(d.verts2 + vb, nullptr, d_verts2, nv, 1.f);
    if (d_normals) scatter(d.normals + d.nbase[(size_t)m], nullptr, d_normals, nn, 0.f);
    if (kind == kDeformBlas) {
        const DeviceState::BlasRange& R = d.blas[(size_t)blas];
        enqueue_tree(d, R.tree, stream);
        if (R.n_inst)
            hipLaunchKernelGGL(refit_instance_box_kernel, blocks(R.n_inst), dim3(kRefitWG), 0, stream, d.refit_fixed,
                               (const DevInstance*)d.insts, (const float*)d.refit_inst_m, (const QNode*)d.nodes,
                               (const uint16_t*)d.tables, (const int32_t*)(d.refit_blas_insts + R.inst_at), R.n_inst);
    } else if (motion && nt && d.mesh_prim0[(size_t)m] >= 0) {
        hipLaunchKernelGGL(refit_motion_box_kernel, blocks(nt), dim3(kRefitWG), 0, stream, d.refit_fixed, d.n_insts,
                           (const int32_t*)d.refit_mbslot, (const uint8_t*)d.pflags, (const PrimShade*)d.prims,
                           (const float4*)d.verts, (const float4*)d.verts2, (uint32_t)d.mesh_prim0[(size_t)m], nt);
    }
    return enqueue_world(d, stream);
}

// the synchronous entries' staging buffer on replica d holds `need` floats (they synchronise before they return: no drain)
int stage_reserve(DeviceState& d, size_t need) {
    return reserve(d.own, nullptr, {{(void**)&d.refit_stage, need * sizeof(float)}}, {{&d.refit_stage_cap, need}});
}

// id joins a stale list (Scene::host_mesh_stale, host_blas_stale) once
void mark_stale(std::vector<int32_t>& list, int32_t id) {
    if (std::find(list.begin(), list.end(), id) == list.end()) list.push_back(id);
}

// after a device deform of a mesh of BLAS b: its host nodes and leaves, and the boxes of its
// instances, are behind the replica's
void mark_blas_stale(Scene& S, int32_t b) {
    mark_stale(S.host_blas_stale, b);
    S.host_inst_stale = true;
}

// Tree T's host copy from replica d: the boxes of nodes N (perm: canonical -> device numbers;
// empty: the same) and the triangles of packets L (DLeaf AoS to the canonical SoA).
int read_tree(const DeviceState& d, const RefitTree& T, const std::vector<int32_t>& perm, std::vector<QNode>& N,
              std::vector<QLeaf>& L) {
    // a rebuilt world tree (mrt_rebuild.hip) lies in the world's node range of the upload and in the tail past the image's nodes
    const bool tail = &T == &d.world && d.rebuild_ready;
    const size_t head = tail ? d.rb_world_nodes : T.n_nodes, extra = tail ? d.rb_extra : 0;
    std::vector<QNode> DN(head + extra);
    std::vector<DLeaf> DL(T.n_leaves);
    if (head) HIP_OK(hipMemcpy(DN.data(), d.nodes + T.node_base, head * sizeof(QNode), hipMemcpyDeviceToHost));
    if (extra) HIP_OK(hipMemcpy(DN.data() + head, d.nodes + d.rb_tail, extra * sizeof(QNode), hipMemcpyDeviceToHost));
    if (!DL.empty()) HIP_OK(hipMemcpy(DL.data(), d.leaves + T.leaf_base, DL.size() * sizeof(DLeaf), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N.size(); i++) {
        size_t at = perm.empty() ? i : (size_t)perm[i];
        if (at >= head) at = extra && at >= d.rb_tail ? head + (at - d.rb_tail) : DN.size();
        if (at >= DN.size()) continue;
        memcpy(N[i].box, DN[at].box, sizeof N[i].box);
    }
    for (size_t i = 0; i < L.size() && i < DL.size(); i++)
        for (int k = 0; k < 4; k++)
            for (int c = 0; c < 9; c++) L[i].t[4 * c + k] = DL[i].tri[k][c];
    return MRT_OK;
}

}  // namespace

// The host copy from replica s.dev (or the first one): node boxes and leaf triangles in
// canonical numbers and layout, the vertices and normals of the meshes and the matrices and
// boxes of the instances an async update left on the device, and from them the binning boxes
// of every replica.
int sync_host(Scene& s, bool meshes_only) {
    if (s.host_topo_stale) meshes_only = false;   // after an async rebuild every refit needs the new topology first
    if (meshes_only ? s.host_mesh_stale.empty() && !s.host_inst_stale : !s.host_stale()) return MRT_OK;
    DeviceState* d = s.dev ? s.dev : (s.devs.empty() ? nullptr : s.devs[0]);
    if (!d) { set_error("refit: the device copy that is ahead of the host is gone"); return MRT_ERR_INVALID; }
    int cur = -1;
    (void)hipGetDevice(&cur);
    HIP_OK(hipSetDevice(d->device));
    HIP_OK(hipDeviceSynchronize());
    int rc;
    if (s.host_topo_stale) {   // a device rebuild: the topology, and with it the boxes and the triangles
        if ((rc = rebuild_read_back(s, *d))) return rc;
    } else if (s.host_bvh_stale && !meshes_only && (rc = read_tree(*d, d->world, d->node_perm, s.nodes, s.leaves))) {
        return rc;
    }
    if (!meshes_only && (rc = relight_read_back(s, *d))) return rc;   // texels and dome tables of a device texture update
    std::vector<float4> buf;
    auto read3 = [&](std::vector<v3>& dst, const float4* src) -> int {
        buf.resize(dst.size());
        if (!dst.empty()) HIP_OK(hipMemcpy(buf.data(), src, dst.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < dst.size(); i++) dst[i] = mk(buf[i].x, buf[i].y, buf[i].z);
        return MRT_OK;
    };
    for (int32_t m : s.host_mesh_stale) {
        Mesh& M = s.meshes[(size_t)m];
        if ((rc = read3(M.verts, d->verts + d->vbase[(size_t)m]))) return rc;
        if ((rc = read3(M.normals, d->normals + d->nbase[(size_t)m]))) return rc;
        if (!M.verts2.empty() && M.verts2.size() == M.verts.size() && d->verts2 && s.mesh_blas[(size_t)m] < 0)   // an async deform's time-1 set
            if ((rc = read3(M.verts2, d->verts2 + d->vbase[(size_t)m]))) return rc;
    }
    s.host_mesh_stale.clear();
    if (s.host_inst_stale && d->refit_ready && d->n_insts == (int)s.instances.size()) {
        // m_transform from the replica's copy, m_inverse and rows 0-2 of m_invTranspose from
        // DevInstance (row 3 of the transpose is column 3 of the inverse), the box from the fixed boxes
        const size_t ni = s.instances.size();
        std::vector<DevInstance> DI(ni);
        std::vector<float> M(16 * ni);
        std::vector<float4> FB(2 * ni);
        HIP_OK(hipMemcpy(DI.data(), d->insts, ni * sizeof(DevInstance), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(M.data(), d->refit_inst_m, M.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(FB.data(), d->refit_fixed, FB.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ni; i++) {
            Instance& I = s.instances[i];
            memcpy(I.m, &M[16 * i], sizeof I.m);
            memcpy(I.inv, DI[i].inv, sizeof I.inv);
            memcpy(I.inv_t, DI[i].inv_t, sizeof DI[i].inv_t);
            for (int c = 0; c < 4; c++) I.inv_t[12 + c] = I.inv[4 * c + 3];
            I.box[0] = FB[2 * i].x; I.box[1] = FB[2 * i].y; I.box[2] = FB[2 * i].z;
            I.box[3] = FB[2 * i + 1].x; I.box[4] = FB[2 * i + 1].y; I.box[5] = FB[2 * i + 1].z;
        }
    }
    s.host_inst_stale = false;
    if (!meshes_only) {   // the BLASes a deform refitted: boxes and triangles (BLAS nodes keep their order on the device)
        for (int32_t b : s.host_blas_stale) {
            if ((size_t)b >= d->blas.size() || (size_t)b >= s.blas.size()) continue;
            Blas& B = s.blas[(size_t)b];
            if ((rc = read_tree(*d, d->blas[(size_t)b].tree, {}, B.nodes, B.leaves))) return rc;
        }
        s.host_blas_stale.clear();
    }
    if (!meshes_only) s.host_bvh_stale = false;
    if (!meshes_only && !s.nodes.empty())
        for (DeviceState* r : s.devs) root_box(s.nodes[0], r->bb_lo, r->bb_hi);
    if (cur >= 0) (void)hipSetDevice(cur);
    return MRT_OK;
}

namespace {

// The device half of a synchronous entry, replica by replica: wait for the device (no frame
// in flight may read the arrays while they change), prepare, fill(d) copies the entry's
// arrays into a stage of stage_floats floats, enqueue(d) runs between the replica's event
// pair (refit_ms: the current replica's), and the binning box follows the refitted root.
template <typename Fill, typename Enqueue>
int refit_replicas(Scene& S, size_t stage_floats, float* refit_ms, Fill fill, Enqueue enqueue) {
    int rc;
    DeviceState* cur = S.dev ? S.dev : S.devs[0];
    for (DeviceState* d : S.devs) {
        HIP_OK(hipSetDevice(d->device));
        HIP_OK(hipDeviceSynchronize());
        if ((rc = prepare(S, *d))) return rc;
        if ((rc = stage_reserve(*d, stage_floats))) return rc;
        if ((rc = fill(*d))) return rc;
        HIP_OK(hipEventRecord(d->refit_ev0, nullptr));
        if ((rc = enqueue(*d))) return rc;
        HIP_OK(hipEventRecord(d->refit_ev1, nullptr));
        HIP_OK(hipEventSynchronize(d->refit_ev1));
        if (d == cur && refit_ms) HIP_OK(hipEventElapsedTime(refit_ms, d->refit_ev0, d->refit_ev1));
        QNode root;
        HIP_OK(hipMemcpy(&root, d->nodes, sizeof root, hipMemcpyDeviceToHost));
        root_box(root, d->bb_lo, d->bb_hi);
    }
    S.host_bvh_stale = true;   // mrt_scene_bvh_export reads the device's arrays back
    HIP_OK(hipSetDevice(cur->device));
    return MRT_OK;
}

// The synchronous entries after their argument checks: mesh `mesh` of `kind` (deform_check;
// mrt_scene_update_mesh: kDeformWorld) takes verts (verts2: kDeformMotion) and normals.
int update_sync(Scene& S, int mesh, int kind, const float* verts, const float* verts2, const float* normals, float* refit_ms) {
    int rc;
    Mesh& M = S.meshes[(size_t)mesh];
    const int32_t blas = S.mesh_blas[(size_t)mesh];
    auto set_host = [&] {
        refit_set_mesh(M, verts, normals);
        if (kind == kDeformMotion) deform_set_motion(M, verts2);
    };
    const bool on_device = !S.dev_dirty && !S.devs.empty();
    if (!on_device) {   // built, not uploaded (or a re-upload is due anyway): the same arithmetic on the host
        if ((rc = sync_host(S))) return rc;
        set_host();
        if (kind == kDeformBlas) refit_blas_host(S, blas);   // the BLAS, then the boxes of its instances
        refit_host(S);
        return MRT_OK;
    }
    if ((rc = sync_host(S, true))) return rc;   // the host mesh is current from here (the hierarchy stays on the device)
    set_host();
    const uint32_t nv = (uint32_t)M.verts.size(), nn = normals ? (uint32_t)M.normals.size() : 0u;
    const uint32_t nv2 = kind == kDeformMotion ? nv : 0u;
    const size_t at_n = (size_t)nv * 3, at_v2 = ((size_t)nv + nn) * 3;   // the stage: vertices, normals, time-1 vertices
    auto fill = [&](DeviceState& d) -> int {
        if (nv) HIP_OK(hipMemcpy(d.refit_stage, verts, (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice));
        if (nn) HIP_OK(hipMemcpy(d.refit_stage + at_n, normals, (size_t)nn * 3 * sizeof(float), hipMemcpyHostToDevice));
        if (nv2) HIP_OK(hipMemcpy(d.refit_stage + at_v2, verts2, (size_t)nv2 * 3 * sizeof(float), hipMemcpyHostToDevice));
        if (!M.tidx.empty() && d.tans && !M.tan.empty()) {   // the tangent frames of the new vertices (mesh_tangents)
            std::vector<float4> T(M.tan.size()), B(M.btan.size());
            for (size_t i = 0; i < T.size(); i++) T[i] = make_float4(M.tan[i].x, M.tan[i].y, M.tan[i].z, 0.f);
            for (size_t i = 0; i < B.size(); i++) B[i] = make_float4(M.btan[i].x, M.btan[i].y, M.btan[i].z, 0.f);
            HIP_OK(hipMemcpy(d.tans + d.nbase[(size_t)mesh], T.data(), T.size() * sizeof(float4), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(d.btans + d.nbase[(size_t)mesh], B.data(), B.size() * sizeof(float4), hipMemcpyHostToDevice));
        }
        return MRT_OK;
    };
    auto enqueue = [&](DeviceState& d) -> int {
        return enqueue_mesh(d, mesh, kind, blas, d.refit_stage, d.refit_stage + at_v2, nv, nn ? d.refit_stage + at_n : nullptr, nn,
                            (uint32_t)M.nt(), nullptr);
    };
    if ((rc = refit_replicas(S, at_v2 + (size_t)nv2 * 3, refit_ms, fill, enqueue))) return rc;
    if (kind == kDeformBlas) mark_blas_stale(S, blas);
    return MRT_OK;
}

// What an async entry (`name`: "update_mesh", ...) needs beyond its argument checks: no
// tangent frames to recompute (M: the mesh it moves, or nullptr) and the scene on exactly
// one device, which becomes the current one and is prepared.
int async_ready(Scene& S, const Mesh* M, const std::string& name) {
    if (M && !M->tidx.empty()) {
        set_error(name + "_async: the mesh has texture coordinates (its tangent frames are recomputed on the host: use mrt_scene_" +
                  name + ")");
        return MRT_ERR_INVALID;
    }
    if (S.dev_dirty || S.devs.size() != 1 || !S.dev) {
        set_error(name + "_async needs the scene uploaded to exactly one device (mrt_scene_upload)");
        return MRT_ERR_INVALID;
    }
    HIP_OK(hipSetDevice(S.dev->device));
    if (S.host_topo_stale)   // an async rebuild: the schedule needs the topology it left on the device
        if (const int rc = sync_host(S)) return rc;
    return prepare(S, *S.dev);
}

// The async mesh entries after their argument checks: enqueue and mark the host copy stale.
int mesh_async(Scene& S, int mesh, int kind, const std::string& name, const float* d_verts, const float* d_verts2,
               const float* d_normals, hipStream_t stream) {
    if (!d_verts) { set_error(name + ": null vertices"); return MRT_ERR_INVALID; }
    const Mesh& M = S.meshes[(size_t)mesh];
    int rc;
    if ((rc = async_ready(S, &M, name))) return rc;
    const int32_t blas = S.mesh_blas[(size_t)mesh];
    if ((rc = enqueue_mesh(*S.dev, mesh, kind, blas, d_verts, d_verts2, (uint32_t)M.verts.size(), d_normals,
                           (uint32_t)M.normals.size(), (uint32_t)M.nt(), stream)))
        return rc;
    S.host_bvh_stale = true;
    if (kind == kDeformBlas) mark_blas_stale(S, blas);
    mark_stale(S.host_mesh_stale, mesh);
    return MRT_OK;
}

}  // namespace

int refit_prepare(const Scene& s, DeviceState& d) { return prepare(s, d); }

}  // namespace mrt

using namespace mrt;

extern "C" {

int mrt_scene_update_mesh(mrt_scene* s, int mesh, const float* verts, const float* normals, float* refit_ms) {
    if (refit_ms) *refit_ms = 0.f;
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (!verts) { set_error("update_mesh: null vertices"); return MRT_ERR_INVALID; }
    const int rc = refit_check(S, mesh, verts, normals);   // arguments first: no device call before
    if (rc) return rc;
    return update_sync(S, mesh, kDeformWorld, verts, nullptr, normals, refit_ms);
}

int mrt_scene_deform_mesh(mrt_scene* s, int mesh, const float* verts, const float* verts2, const float* normals,
                          float* refit_ms) {
    if (refit_ms) *refit_ms = 0.f;
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (!verts) { set_error("deform_mesh: null vertices"); return MRT_ERR_INVALID; }
    int kind = kDeformWorld;
    const int rc = deform_check(S, mesh, verts, verts2, verts2 != nullptr, normals, &kind);   // arguments first
    if (rc) return rc;
    return update_sync(S, mesh, kind, verts, verts2, normals, refit_ms);
}

int mrt_scene_deform_mesh_async(mrt_scene* s, int mesh, const float* d_verts, const float* d_verts2, const float* d_normals,
                                void* stream) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    int kind = kDeformWorld;
    int rc = deform_check(S, mesh, nullptr, nullptr, d_verts2 != nullptr, nullptr, &kind);   // ids and kinds: the arrays are on the device
    if (rc) return rc;
    if (kind == kDeformWorld) return mrt_scene_update_mesh_async(s, mesh, d_verts, d_normals, stream);
    return mesh_async(S, mesh, kind, "deform_mesh", d_verts, d_verts2, d_normals, (hipStream_t)stream);
}

int mrt_scene_update_mesh_async(mrt_scene* s, int mesh, const float* d_verts, const float* d_normals, void* stream) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    const int rc = refit_check(S, mesh, nullptr, nullptr);
    if (rc) return rc;
    return mesh_async(S, mesh, kDeformWorld, "update_mesh", d_verts, nullptr, d_normals, (hipStream_t)stream);
}

int mrt_scene_update_instances(mrt_scene* s, const int32_t* ids, int32_t n, const float* m16s, float* refit_ms) {
    if (refit_ms) *refit_ms = 0.f;
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (!m16s) { set_error("update_instances: null matrices"); return MRT_ERR_INVALID; }
    std::vector<Instance> NI;   // arguments first: no device call and no change before
    int rc;
    if (!S.host_blas_stale.empty() && (rc = sync_host(S))) return rc;   // the boxes come from the BLAS roots: a device deform is ahead
    rc = instances_check(S, ids, 0, n, m16s, &NI);
    if (rc) return rc;
    if (n == 0) return MRT_OK;
    auto apply = [&] {
        for (int32_t k = 0; k < n; k++) S.instances[(size_t)(ids ? ids[k] : k)] = NI[(size_t)k];
    };
    const bool on_device = !S.dev_dirty && !S.devs.empty();
    if (!on_device) {   // built, not uploaded (or a re-upload is due anyway): the host refit reads Instance::box
        if ((rc = sync_host(S))) return rc;
        apply();
        refit_host(S);
        return MRT_OK;
    }
    if ((rc = sync_host(S, true))) return rc;   // the host instances are current from here (the hierarchy stays on the device)
    auto d_ids = [&](DeviceState& d) { return ids ? (int32_t*)(d.refit_stage + (size_t)n * 16) : nullptr; };   // after the matrices
    auto fill = [&](DeviceState& d) -> int {
        HIP_OK(hipMemcpy(d.refit_stage, m16s, (size_t)n * 16 * sizeof(float), hipMemcpyHostToDevice));
        if (ids) HIP_OK(hipMemcpy(d_ids(d), ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        return MRT_OK;
    };
    auto enqueue = [&](DeviceState& d) -> int { return enqueue_instances(d, d.refit_stage, d_ids(d), 0, (uint32_t)n, nullptr); };
    if ((rc = refit_replicas(S, (size_t)n * 17, refit_ms, fill, enqueue))) return rc;   // n matrices, then n ids
    apply();
    return MRT_OK;
}

int mrt_scene_update_instances_async(mrt_scene* s, int32_t first, int32_t n, const float* d_m16s, void* stream) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    Scene& S = s->impl;
    if (!d_m16s) { set_error("update_instances: null matrices"); return MRT_ERR_INVALID; }
    int rc = instances_check(S, nullptr, first, n, nullptr, nullptr);   // the range: the kernel trusts its ids
    if (rc) return rc;
    if (n == 0) return MRT_OK;
    if ((rc = async_ready(S, nullptr, "update_instances"))) return rc;
    if ((rc = enqueue_instances(*S.dev, d_m16s, nullptr, first, (uint32_t)n, (hipStream_t)stream))) return rc;
    S.host_bvh_stale = true;
    S.host_inst_stale = true;
    return MRT_OK;
}

}  // extern "C"
