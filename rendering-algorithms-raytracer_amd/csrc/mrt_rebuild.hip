// mrt_rebuild.hip -- mrt_scene_rebuild_bvh: a new topology for the world hierarchy, made on the
// device from the lanes its packets hold now (rebuild_host, host_build.cpp, is
// the same rule on the host and tests/test_rebuild.py restates it in numpy).  One sequence of
// launches on the caller's stream, each sized by what the host knows (the world's lanes n, its
// packets P = ceil(n / 4), the packet capacity of the upload) and none handing data between
// workgroups: a key per lane (the Morton code of its box centre in the root box, over its
// position), rocPRIM's radix sort, the packets gathered in sorted order with their boxes, a
// min / max segment tree over the packet boxes level by level, the binary radix tree over the
// packet keys (Karras 2012, one thread per node), an exclusive scan that numbers the binary
// nodes that root a 4-wide node, and one thread per such node that writes it.  Hit ids,
// BLASes, instances, PrimShade records and vertices stay as they are.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "mrt_device.h"
#include "mrt_kernels.h"
#include "mrt_rebuild.h"
#include "mrt_refit_dev.h"

namespace mrt {

namespace {

constexpr int kRebuildWG = 256;
constexpr uint64_t kNoKey = ~uint64_t(0);   // an empty lane: sorts last

inline dim3 blocks(size_t n) { return dim3((unsigned)((n + kRebuildWG - 1) / kRebuildWG)); }

// root_box (host_image.cpp) of a device node: the union of its used slots' finite values per axis
__device__ __forceinline__ void d_root_box(const QNode& q, float lo3[3], float hi3[3]) {
    for (int a = 0; a < 3; a++) {
        lo3[a] = hi3[a] = 0.f;
        bool any = false;
        for (int i = 0; i < 4; i++) {
            if (q.child[i] == kEmptySlot) continue;
            const float lo = q.box[a * 4 + i], hi = q.box[12 + a * 4 + i];
            if (!isfinite(lo) || !isfinite(hi)) continue;
            lo3[a] = any ? std_min(lo3[a], lo) : lo;
            hi3[a] = any ? std_max(hi3[a], hi) : hi;
            any = true;
        }
    }
}

// One lane per packet lane of the world's packet capacity: the box refit_leaf_kernel gives the
// lane (box3 of its triangle's vertices; a ProxyObject / MBObject lane its fixed box) and its
// key.  Lanes past the packets in use and empty lanes get the all-ones key.
__global__ __launch_bounds__(kRebuildWG) void rebuild_key_kernel(const DLeaf* __restrict__ leaves, uint32_t n_cap, uint32_t n_cur,
                                                                 const QNode* __restrict__ nodes,
                                                                 const PrimShade* __restrict__ prims,
                                                                 const float4* __restrict__ verts,
                                                                 const uint8_t* __restrict__ pflags,
                                                                 const int32_t* __restrict__ mbslot,
                                                                 const float4* __restrict__ fixed, int n_insts,
                                                                 uint64_t* __restrict__ keys, float4* __restrict__ lane_box) {
    const uint32_t g = blockIdx.x * kRebuildWG + threadIdx.x;
    if (g >= n_cap) return;
    uint64_t key = kNoKey;
    const int32_t prim = g < n_cur ? leaves[g >> 2].prim[g & 3u] : -1;
    if (prim != -1) {
        int fx = -1;
        if (prim <= -2) fx = -2 - prim;
        else if (pflags && (pflags[prim] & 1u)) fx = n_insts + mbslot[prim];
        DBox b;
        if (fx >= 0) {
            b = d_load_box(fixed, fx);
        } else {
            const PrimShade ps = prims[prim];
            b = d_tri_box(verts[ps.v[0]], verts[ps.v[1]], verts[ps.v[2]]);
        }
        float rlo[3], rhi[3];
        d_root_box(nodes[0], rlo, rhi);
        key = rb_key(b.lo, b.hi, rlo, rhi, g);
        d_store_box(lane_box, g, b);
    }
    keys[g] = key;
}

// One lane per lane of the P new packets: sorted lane i goes to lane i & 3 of packet i >> 2,
// its triangle data and prim word as they are; lanes past the n sorted ones are zero with
// prim -1.  The packet's box (its lanes merged in lane order from the empty box) becomes leaf
// P + p of the segment tree; its key is its first lane's; its word holds the low four bits
// append (host_image.cpp) would give its child word: count - 1, proxy, check.
__global__ __launch_bounds__(kRebuildWG) void rebuild_pack_kernel(const DLeaf* __restrict__ leaves, DLeaf* __restrict__ out,
                                                                  uint32_t P, uint32_t n, uint32_t n_cap,
                                                                  const uint64_t* __restrict__ sorted,
                                                                  const float4* __restrict__ lane_box,
                                                                  const PrimShade* __restrict__ prims,
                                                                  const DevMaterial* __restrict__ mats,
                                                                  const uint8_t* __restrict__ pflags,
                                                                  float4* __restrict__ seg, uint64_t* __restrict__ pkey,
                                                                  uint32_t* __restrict__ pword) {
    const uint32_t i = blockIdx.x * kRebuildWG + threadIdx.x;
    const bool in = i < 4u * P;   // the four lanes of a packet are in one wave and all inside or all outside
    const uint32_t p = i >> 2, k = i & 3u;
    DBox b = d_empty_box();
    uint64_t key = kNoKey;
    uint32_t bits = 0;   // bit 0 used, bit 2 a ProxyObject lane, bit 3 an alpha-mapped or motion-blurred triangle
    if (in) {
        if (i < n) key = sorted[i];
        const uint32_t src = (uint32_t)key;
        const bool used = key != kNoKey && src < n_cap;
        int32_t prim = -1;
        float t[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (used) {
            const DLeaf& L = leaves[src >> 2];
            prim = L.prim[src & 3u];
            for (int c = 0; c < 9; c++) t[c] = L.tri[src & 3u][c];
            b = d_load_box(lane_box, src);
            bits = 1u;
            if (prim <= -2) bits |= 4u;
            else if (prim >= 0 && ((pflags && (pflags[prim] & 1u)) || mats[prims[prim].mat].maps[kMapAlpha] >= 0)) bits |= 8u;
        }
        for (int c = 0; c < 9; c++) out[p].tri[k][c] = t[c];
        out[p].prim[k] = prim;
    }
    DBox acc = d_empty_box();
    uint32_t count = 0, flags = 0;
    for (int j = 0; j < 4; j++) {
        DBox o;
        for (int a = 0; a < 3; a++) {
            o.lo[a] = __shfl(b.lo[a], j, 4);
            o.hi[a] = __shfl(b.hi[a], j, 4);
        }
        const uint32_t ob = __shfl(bits, j, 4);
        if (ob & 1u) {
            acc = d_merge(acc, o);
            count = (uint32_t)j + 1u;
        }
        flags |= ob & 12u;
    }
    if (in && k == 0) {
        d_store_box(seg, (size_t)P + p, acc);
        pkey[p] = key;
        pword[p] = flags | ((count < 1u ? 1u : count) - 1u);
    }
}

// Segment-tree nodes lo .. hi - 1 (one level: their children 2 i and 2 i + 1 are of a level an
// earlier launch wrote, or packets)
__global__ __launch_bounds__(kRebuildWG) void rebuild_seg_kernel(float4* __restrict__ seg, uint32_t lo, uint32_t hi) {
    const uint32_t i = lo + blockIdx.x * kRebuildWG + threadIdx.x;
    if (i >= hi) return;
    d_store_box(seg, i, d_merge(d_load_box(seg, 2 * (size_t)i), d_load_box(seg, 2 * (size_t)i + 1)));
}
// The levels below node 2^(top + 1) in one workgroup, deepest first, a barrier between two levels
__global__ __launch_bounds__(kRebuildWG) void rebuild_seg_top_kernel(float4* __restrict__ seg, uint32_t P, int top) {
    for (int k = top; k >= 0; k--) {
        const uint32_t i = (1u << k) + threadIdx.x;
        if (threadIdx.x < (1u << k) && i < P)
            d_store_box(seg, i, d_merge(d_load_box(seg, 2 * (size_t)i), d_load_box(seg, 2 * (size_t)i + 1)));
        __syncthreads();
    }
}
// the merge of packet boxes first .. last
__device__ DBox d_range_box(const float4* __restrict__ seg, uint32_t P, uint32_t first, uint32_t last) {
    DBox r = d_empty_box();
    for (uint32_t l = first + P, e = last + P + 1; l < e; l >>= 1, e >>= 1) {
        if (l & 1u) r = d_merge(r, d_load_box(seg, l++));
        if (e & 1u) r = d_merge(r, d_load_box(seg, --e));
    }
    return r;
}

// One thread per binary node of the radix tree over the P packet keys: its range and children,
// and for each child that is a binary node whether it roots a 4-wide node (its digit is larger
// than this node's).  Node 0 is the root.
__global__ __launch_bounds__(kRebuildWG) void rebuild_karras_kernel(const uint64_t* __restrict__ pkey, uint32_t P,
                                                                    int32_t* __restrict__ bin, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * kRebuildWG + threadIdx.x;
    const uint32_t nb = P - 1;
    if (i >= nb) return;
    int64_t first, last, g;
    rb_karras(pkey, (int64_t)P, (int64_t)i, first, last, g);
    const int32_t l = rb_left(first, g), r = rb_right(last, g);
    bin[i] = (int32_t)first;
    bin[nb + i] = (int32_t)last;
    bin[2 * (size_t)nb + i] = l;
    bin[3 * (size_t)nb + i] = r;
    const int dg = rb_digit(pkey, first, last);
    if (l >= 0) flag[l] = dg < rb_digit(pkey, first, g) ? 1u : 0u;
    if (r >= 0) flag[r] = dg < rb_digit(pkey, g + 1, last) ? 1u : 0u;
    if (i == 0) flag[0] = 1u;
}

// dense node j as a device node number
__device__ __forceinline__ int32_t d_node_at(uint32_t j, uint32_t world_nodes, uint32_t tail) {
    return (int32_t)(j < world_nodes ? j : tail + (j - world_nodes));
}

// One thread per binary node that roots a 4-wide node: its children in key order, a leaf
// slot's box its packet's, an inner slot's the merge of the packet boxes of that child's
// range; the device child words and the slot kinds as build_image makes them.  P == 1: the
// root alone with the packet in slot 0.
__global__ __launch_bounds__(kRebuildWG) void rebuild_emit_kernel(QNode* __restrict__ nodes, uint32_t P, uint32_t leaf_base,
                                                                  uint32_t world_nodes, uint32_t tail,
                                                                  const uint64_t* __restrict__ pkey,
                                                                  const uint32_t* __restrict__ pword,
                                                                  const int32_t* __restrict__ bin,
                                                                  const uint32_t* __restrict__ flag,
                                                                  const uint32_t* __restrict__ num,
                                                                  const float4* __restrict__ seg, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * kRebuildWG + threadIdx.x;
    const uint32_t nb = P > 1 ? P - 1 : 1;
    if (i >= nb) return;
    int32_t kid[4];
    int nk;
    uint32_t j = 0;
    if (P == 1) {
        kid[0] = ~0;
        nk = 1;
        count[0] = 1u;
    } else {
        if (i == nb - 1) count[0] = num[i] + flag[i];
        if (!flag[i]) return;
        j = num[i];
        nk = rb_children(pkey, bin, bin + nb, bin + 2 * (size_t)nb, bin + 3 * (size_t)nb, (int32_t)i, kid);
    }
    QNode q;
    for (int k = 0; k < 24; k++) q.box[k] = 0.f;
    for (int k = 0; k < 4; k++) {
        q.child[k] = kEmptySlot;
        q.pad[k] = 0u;
    }
    for (int k = 0; k < nk; k++) {
        const int32_t c = kid[k];
        if (c < 0) {
            const uint32_t p = (uint32_t)~c, w = pword[p];
            q.child[k] = leaf_child(leaf_base + p, (int)(w & 3u) + 1, (w & 4u) != 0, (w & 8u) != 0);
            d_store_slot(q, k, d_load_box(seg, (size_t)P + p));
        } else {
            q.child[k] = d_node_at(num[c], world_nodes, tail);
            d_store_slot(q, k, d_range_box(seg, P, (uint32_t)bin[c], (uint32_t)bin[nb + c]));
        }
    }
    q.pad[0] = slot_kinds(q.child);
    nodes[d_node_at(j, world_nodes, tail)] = q;
}

uint32_t world_packets(const DeviceState& d) { return ((uint32_t)d.n_world + 3u) / 4u; }

// What a rebuild of replica d would add to its node array (extra nodes past the image's), and
// MRT_ERR_OVERFLOW when the walks could not address it: host arithmetic only
int grown_nodes(const DeviceState& d, uint32_t& total, uint32_t& extra) {
    if (d.rebuild_ready) { total = d.rb_tail; extra = d.rb_extra; return MRT_OK; }
    total = d.world.n_nodes;
    for (const DeviceState::BlasRange& R : d.blas) total += R.tree.n_nodes;
    const uint32_t P = world_packets(d);
    extra = P - 1 > d.world.n_nodes ? P - 1 - d.world.n_nodes : 0u;
    if (P < 1 || P > d.world.n_leaves) { set_error("rebuild_bvh: replica out of date"); return MRT_ERR_INVALID; }
    if (!walk_arrays_fit((uint64_t)total + extra, d.n_leaves_all)) {
        set_error("rebuild_bvh: the node array the rebuilt hierarchy may need passes 4 GiB");
        return MRT_ERR_OVERFLOW;
    }
    return MRT_OK;
}

// rocPRIM's scratch for a sort of n_keys keys and a scan of n_flags flags (sizes only: no launch)
int temp_bytes(uint32_t n_keys, uint32_t n_flags, size_t& bytes) {
    size_t a = 0, b = 0;
    uint64_t* k = nullptr;
    uint32_t* f = nullptr;
    HIP_OK(rocprim::radix_sort_keys(nullptr, a, k, k, n_keys, 0, 64, nullptr));
    if (n_flags) HIP_OK(rocprim::exclusive_scan(nullptr, b, f, f, 0u, n_flags, rocprim::plus<uint32_t>(), nullptr));
    bytes = std::max<size_t>(16, std::max(a, b));
    return MRT_OK;
}

// What the rebuild of replica d needs beyond the refit's, made once: the node array grown to
// hold P - 1 world nodes (the old nodes copied; BLAS nodes and node 0 keep their numbers) and
// the scratch of every launch.  The current device is d's and refit_prepare has run.
int prepare(DeviceState& d) {
    if (d.rebuild_ready) return MRT_OK;
    int rc;
    uint32_t total, extra;
    if ((rc = grown_nodes(d, total, extra))) return rc;
    const uint32_t P = world_packets(d), cap = d.world.n_leaves, nb = P > 1 ? P - 1 : 1;
    size_t tb;
    if ((rc = temp_bytes(4u * cap, P > 1 ? P - 1 : 0, tb))) return rc;
    if ((rc = d.own.alloc(d.rb_keys, (size_t)2 * 4 * cap * sizeof(uint64_t))) ||
        (rc = d.own.alloc(d.rb_lane_box, (size_t)4 * cap * 2 * sizeof(float4))) ||
        (rc = d.own.alloc(d.rb_leaves, (size_t)P * sizeof(DLeaf))) ||
        (rc = d.own.alloc(d.rb_seg, (size_t)2 * P * 2 * sizeof(float4))) ||
        (rc = d.own.alloc(d.rb_pkey, (size_t)P * sizeof(uint64_t))) ||
        (rc = d.own.alloc(d.rb_pword, (size_t)P * sizeof(uint32_t))) ||
        (rc = d.own.alloc(d.rb_bin, (size_t)4 * nb * sizeof(int32_t))) ||
        (rc = d.own.alloc(d.rb_flag, (size_t)2 * nb * sizeof(uint32_t))) ||
        (rc = d.own.alloc(d.rb_count, 16)) || (rc = d.own.alloc(d.rb_temp, tb)))
        return rc;
    d.rb_temp_bytes = tb;
    if (extra) {   // no launch may read the old array while it is replaced
        HIP_OK(hipDeviceSynchronize());
        QNode* grown = nullptr;
        if ((rc = d.own.alloc(grown, ((size_t)total + extra) * sizeof(QNode)))) return rc;
        HIP_OK(hipMemcpy(grown, d.nodes, (size_t)total * sizeof(QNode), hipMemcpyDeviceToDevice));
        HIP_OK(hipMemset(grown + total, 0, (size_t)extra * sizeof(QNode)));
        d.own.release(d.nodes);
        d.nodes = grown;
    }
    d.rb_world_nodes = d.world.n_nodes;
    d.rb_tail = total;
    d.rb_extra = extra;
    d.rb_cap_leaves = cap;
    d.rb_cur_leaves = cap;
    d.rebuild_ready = true;
    return MRT_OK;
}

// Enqueue on `stream`: the world hierarchy of replica d rebuilt from the lanes, vertices and
// fixed boxes the device holds now.
int enqueue(DeviceState& d, hipStream_t stream) {
    const uint32_t n = (uint32_t)d.n_world, P = world_packets(d), n_cap = 4u * d.rb_cap_leaves, nb = P - 1;
    uint64_t* keys = d.rb_keys;
    uint64_t* sorted = d.rb_keys + n_cap;
    const RefitTree& T = d.world;
    hipLaunchKernelGGL(rebuild_key_kernel, blocks(n_cap), dim3(kRebuildWG), 0, stream, (const DLeaf*)(d.leaves + T.leaf_base),
                       n_cap, 4u * d.rb_cur_leaves, (const QNode*)d.nodes, (const PrimShade*)(d.prims + T.shade_base),
                       (const float4*)d.verts, (const uint8_t*)(d.has_mb ? d.pflags : nullptr), (const int32_t*)d.refit_mbslot,
                       (const float4*)d.refit_fixed, d.n_insts, keys, d.rb_lane_box);
    size_t tb = d.rb_temp_bytes;
    HIP_OK(rocprim::radix_sort_keys(d.rb_temp, tb, keys, sorted, n_cap, 0, 64, stream));
    hipLaunchKernelGGL(rebuild_pack_kernel, blocks((size_t)4 * P), dim3(kRebuildWG), 0, stream,
                       (const DLeaf*)(d.leaves + T.leaf_base), d.rb_leaves, P, n, n_cap, (const uint64_t*)sorted,
                       (const float4*)d.rb_lane_box, (const PrimShade*)(d.prims + T.shade_base), (const DevMaterial*)d.mats,
                       (const uint8_t*)(d.has_mb ? d.pflags : nullptr), d.rb_seg, d.rb_pkey, d.rb_pword);
    HIP_OK(hipMemcpyAsync(d.leaves + T.leaf_base, d.rb_leaves, (size_t)P * sizeof(DLeaf), hipMemcpyDeviceToDevice, stream));
    uint32_t* flag = d.rb_flag;
    uint32_t* num = d.rb_flag + (P > 1 ? nb : 1);
    if (P > 1) {
        // segment-tree levels [2^k, 2^(k + 1)) below P, deepest first; the levels under node 256 in one workgroup
        int k = 0;
        while ((2u << k) < P) k++;   // the level of node P - 1
        for (; k >= 8; k--) {
            const uint32_t lo = 1u << k, hi = std::min(P, 2u << k);
            hipLaunchKernelGGL(rebuild_seg_kernel, blocks(hi - lo), dim3(kRebuildWG), 0, stream, d.rb_seg, lo, hi);
        }
        hipLaunchKernelGGL(rebuild_seg_top_kernel, dim3(1), dim3(kRebuildWG), 0, stream, d.rb_seg, P, k);
        hipLaunchKernelGGL(rebuild_karras_kernel, blocks(nb), dim3(kRebuildWG), 0, stream, (const uint64_t*)d.rb_pkey, P, d.rb_bin,
                           flag);
        tb = d.rb_temp_bytes;
        HIP_OK(rocprim::exclusive_scan(d.rb_temp, tb, flag, num, 0u, nb, rocprim::plus<uint32_t>(), stream));
    }
    hipLaunchKernelGGL(rebuild_emit_kernel, blocks(P > 1 ? nb : 1), dim3(kRebuildWG), 0, stream, d.nodes, P, T.leaf_base,
                       d.rb_world_nodes, d.rb_tail, (const uint64_t*)d.rb_pkey, (const uint32_t*)d.rb_pword,
                       (const int32_t*)d.rb_bin, (const uint32_t*)flag, (const uint32_t*)num, (const float4*)d.rb_seg, d.rb_count);
    HIP_OK(hipGetLastError());
    d.rb_cur_leaves = P;
    d.lds_ok = false;   // node numbers 0 .. 63 are no longer the tree's breadth-first head: the LDS top-node walk falls back
    return MRT_OK;
}

int scene_check(const mrt_scene* s) {
    if (!s) { set_error("null scene"); return MRT_ERR_INVALID; }
    const Scene& S = s->impl;
    if (!S.built) { set_error("rebuild_bvh: scene not built"); return MRT_ERR_NOT_BUILT; }
    if (S.imported) {
        set_error("rebuild_bvh: the hierarchy was imported (mrt_scene_bvh_import) and need not be a tree: mrt_scene_build_bvh");
        return MRT_ERR_INVALID;
    }
    return MRT_OK;
}

}  // namespace

// The canonical arrays from replica d after a device rebuild: nodes numbered breadth first from
// node 0, slots in order (every child gets a larger number than its parent); a leaf word ~p; a
// ProxyObject lane -2 - instance its world object id.  Every replica of the scene ran the same
// launches, so the dense node numbers and the counts are theirs too; device numbers are not
// (a replica uploaded after an earlier rebuild has another world range and tail), so each
// replica's permutation goes through its own layout.  Their schedules are made again.
int rebuild_read_back(Scene& s, DeviceState& d) {
    if (!d.rebuild_ready) { set_error("rebuild_bvh: the replica that was rebuilt is gone"); return MRT_ERR_INVALID; }
    uint32_t M = 0;
    HIP_OK(hipMemcpy(&M, d.rb_count, sizeof M, hipMemcpyDeviceToHost));
    const uint32_t W = d.rb_world_nodes, P = world_packets(d);
    if (M < 1 || M > W + d.rb_extra) { set_error("rebuild_bvh: bad node count on the device"); return MRT_ERR_INVALID; }
    std::vector<QNode> DN((size_t)W + d.rb_extra);
    HIP_OK(hipMemcpy(DN.data(), d.nodes, (size_t)W * sizeof(QNode), hipMemcpyDeviceToHost));
    if (d.rb_extra) HIP_OK(hipMemcpy(DN.data() + W, d.nodes + d.rb_tail, (size_t)d.rb_extra * sizeof(QNode), hipMemcpyDeviceToHost));
    std::vector<DLeaf> DL(P);
    HIP_OK(hipMemcpy(DL.data(), d.leaves + d.world.leaf_base, (size_t)P * sizeof(DLeaf), hipMemcpyDeviceToHost));
    auto slot_of = [&](int32_t dev) -> int64_t {   // where device node `dev` lies in DN, -1: not a world node
        if (dev >= 0 && (uint32_t)dev < W) return dev;
        if ((uint32_t)dev >= d.rb_tail && (uint32_t)dev < d.rb_tail + d.rb_extra) return (int64_t)W + ((uint32_t)dev - d.rb_tail);
        return -1;
    };
    std::vector<int32_t> perm{0};
    std::vector<QNode> N;
    for (size_t q = 0; q < perm.size(); q++) {
        const QNode& D = DN[(size_t)slot_of(perm[q])];
        QNode c;
        memset(&c, 0, sizeof c);
        memcpy(c.box, D.box, sizeof c.box);
        for (int k = 0; k < 4; k++) {
            const int32_t w = D.child[k];
            c.child[k] = w;
            if (w == kEmptySlot) continue;
            if (w < 0) {
                const uint32_t packet = (~(uint32_t)w >> 4) - d.world.leaf_base;
                if (packet >= P) { set_error("rebuild_bvh: bad packet number on the device"); return MRT_ERR_INVALID; }
                c.child[k] = ~(int32_t)packet;
                continue;
            }
            if (slot_of(w) < 0 || perm.size() >= M) { set_error("rebuild_bvh: bad node number on the device"); return MRT_ERR_INVALID; }
            c.child[k] = (int32_t)perm.size();
            perm.push_back(w);
        }
        N.push_back(c);
    }
    if (perm.size() != M) { set_error("rebuild_bvh: the device's node count and its tree differ"); return MRT_ERR_INVALID; }
    std::vector<int32_t> inst_obj(s.instances.size(), -1);
    for (size_t o = 0; o < s.obj_inst.size(); o++)
        if (s.obj_inst[o] >= 0) inst_obj[(size_t)s.obj_inst[o]] = (int32_t)o;
    std::vector<QLeaf> L(P);
    for (uint32_t p = 0; p < P; p++)
        for (int k = 0; k < 4; k++) {
            for (int c = 0; c < 9; c++) L[p].t[4 * c + k] = DL[p].tri[k][c];
            const int32_t pr = DL[p].prim[k];
            if (pr <= -2 && (size_t)(-2 - pr) >= inst_obj.size()) { set_error("rebuild_bvh: bad lane on the device"); return MRT_ERR_INVALID; }
            L[p].prim[k] = pr <= -2 ? inst_obj[(size_t)(-2 - pr)] : pr;
        }
    for (DeviceState* r : s.devs) {
        if (!r->rebuild_ready) { set_error("rebuild_bvh: a replica of the scene was not rebuilt"); return MRT_ERR_INVALID; }
        r->node_perm.resize(perm.size());
        for (size_t i = 0; i < perm.size(); i++) {
            const uint32_t j = (uint32_t)slot_of(perm[i]);   // the dense number: d's world range, then its tail
            if (j >= r->rb_world_nodes + r->rb_extra) { set_error("rebuild_bvh: replicas differ in their node counts"); return MRT_ERR_INVALID; }
            r->node_perm[i] = (int32_t)(j < r->rb_world_nodes ? j : r->rb_tail + (j - r->rb_world_nodes));
        }
        r->world.n_nodes = M;
        r->world.n_leaves = P;
        r->sched_stale = true;
        r->lds_ok = false;
    }
    s.nodes.swap(N);
    s.leaves.swap(L);
    s.info.nodes = (int32_t)M;
    s.info.leaves = (int32_t)P;
    s.host_topo_stale = false;
    return MRT_OK;
}

}  // namespace mrt

using namespace mrt;

extern "C" {

int mrt_scene_rebuild_bvh(mrt_scene* s, float* rebuild_ms) {
    if (rebuild_ms) *rebuild_ms = 0.f;
    int rc;
    if ((rc = scene_check(s))) return rc;   // arguments first: no device call before
    Scene& S = s->impl;
    if (S.dev_dirty || S.devs.empty()) {   // built, not uploaded (or a re-upload is due anyway): the same rule on the host
        if ((rc = sync_host(S))) return rc;
        rebuild_host(S);
        return MRT_OK;
    }
    if (S.host_topo_stale && (rc = sync_host(S))) return rc;   // an async rebuild: the counts the checks below read
    for (DeviceState* d : S.devs) {   // every replica can hold the rebuilt tree, or nothing changes
        uint32_t total, extra;
        if ((rc = grown_nodes(*d, total, extra))) return rc;
    }
    DeviceState* cur = S.dev ? S.dev : S.devs[0];
    for (DeviceState* d : S.devs) {   // every allocation before the first launch: a failure here leaves every tree as it was
        HIP_OK(hipSetDevice(d->device));
        HIP_OK(hipDeviceSynchronize());   // no frame in flight may read the arrays while they change
        if ((rc = refit_prepare(S, *d)) || (rc = prepare(*d))) {
            (void)hipSetDevice(cur->device);
            return rc;
        }
    }
    if ((rc = sync_host(S, true))) return rc;   // the host meshes and instances are current: what the failure path below refits from
    auto launch = [&](DeviceState* d) -> int {
        HIP_OK(hipSetDevice(d->device));
        HIP_OK(hipEventRecord(d->refit_ev0, nullptr));
        if (const int e = enqueue(*d, nullptr)) return e;
        HIP_OK(hipEventRecord(d->refit_ev1, nullptr));
        HIP_OK(hipEventSynchronize(d->refit_ev1));
        if (d == cur && rebuild_ms) HIP_OK(hipEventElapsedTime(rebuild_ms, d->refit_ev0, d->refit_ev1));
        return MRT_OK;
    };
    for (DeviceState* d : S.devs)
        if ((rc = launch(d))) {
            // some replicas are rebuilt and some are not: the host keeps the topology it has, refitted to
            // the geometry of now (the arithmetic of the device refit), and every replica is uploaded again
            S.host_bvh_stale = false;
            refit_host(S);
            S.dev_dirty = true;
            (void)hipSetDevice(cur->device);
            return rc;
        }
    HIP_OK(hipSetDevice(cur->device));
    // the counts and the topology are known on the device alone: read them now
    S.host_topo_stale = true;
    S.host_bvh_stale = true;
    return sync_host(S);
}

int mrt_scene_rebuild_bvh_async(mrt_scene* s, void* stream) {
    int rc;
    if ((rc = scene_check(s))) return rc;
    Scene& S = s->impl;
    if (S.dev_dirty || S.devs.size() != 1 || !S.dev) {
        set_error("rebuild_bvh_async needs the scene uploaded to exactly one device (mrt_scene_upload)");
        return MRT_ERR_INVALID;
    }
    DeviceState& d = *S.dev;
    uint32_t total, extra;
    if ((rc = grown_nodes(d, total, extra))) return rc;
    HIP_OK(hipSetDevice(d.device));
    // the first rebuild of a replica allocates (and makes the refit's fixed boxes); later ones only enqueue
    if (!d.refit_ready && (rc = refit_prepare(S, d))) return rc;
    if ((rc = prepare(d)) || (rc = enqueue(d, (hipStream_t)stream))) return rc;
    S.host_topo_stale = true;
    S.host_bvh_stale = true;
    return MRT_OK;
}

}  // extern "C"
