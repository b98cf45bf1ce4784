// mrt_image.h -- internal: the host image of a device replica.  build_image (host_image.cpp,
// plain C++: no HIP call) makes every array upload_scene copies and everything derived from
// them; upload_scene (mrt_upload.hip) copies the arrays and keeps the ImageInfo part.
#pragma once
#include "mrt_scene.h"

namespace mrt {

// float4 / float2 / uint4 as the device reads them
struct F4 { float x, y, z, w; };
struct F2 { float x, y; };
struct U4 { uint32_t x, y, z, w; };

// The walks address a lane's node and leaf triangle as a 32-bit byte offset from the array's
// base (node_at / tri_at, mrt_kernels.h), so a device node array (128 B per node) and leaf
// array (160 B per packet) must each end within 4 GiB.  build_image refuses a scene past that
// (MRT_ERR_OVERFLOW; mrt_walk_arrays_fit, host_api.cpp, is the same test on the C-ABI).
inline bool walk_arrays_fit(uint64_t n_nodes, uint64_t n_leaves) {
    return n_nodes <= (uint64_t(1) << 32) / 128 && n_leaves <= (uint64_t(1) << 32) / 160;
}

// One tree the refit walks, the world's or a BLAS's: where it lies in the replica's arrays (the
// image), and the schedule the first refit makes: its nodes in device numbers sorted by height.
struct RefitTree {
    uint32_t node_base = 0, n_nodes = 0;    // node_base is the root (BLAS nodes are not permuted; the world's are: node_perm)
    uint32_t leaf_base = 0, n_leaves = 0;   // DLeaf packets leaf_base .. leaf_base + n_leaves - 1
    int32_t shade_base = 0;                 // PrimShade of its object 0
    bool fixed_lanes = false;               // the world: ProxyObject / MBObject lanes take their boxes from refit_fixed
    const int32_t* order = nullptr;         // its part of DeviceState::refit_order
    std::vector<uint32_t> off;              //   height h holds order[off[h] .. off[h + 1])
};

// What a replica keeps of its image once the arrays are on the device (DeviceState derives from it).
struct ImageInfo {
    int n_insts = 0, n_world = 0;
    bool has_maps = false, has_alpha = false;
    bool has_mb = false;          // a motion-blurred world mesh (pflags, verts2)
    bool special = false;         // instances, alpha maps or motion blur: leaf packets with special lanes (INST kernels)
    bool boxes_finite = false;
    bool boxes_ordered = false;   // every used slot box has lo <= hi per axis (octant-ordered box test)
    bool lds_ok = false;          // the world hierarchy has kLdsNodes nodes for the LDS top-node walk (renumbered)
    float bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};   // world root box (ray-binning origin cells)
    bool point_only = false;
    bool dome = false;            // a dome light (incoherent shadow rays)
    int recursive = 0;            // chain shading (Shader REC): 1 reflection / refraction, 2 + path tracing
    bool disperse = false;        // a dispersive Blinn material with secondary rays: the fused (tree) engine
    bool transparent = false;     // a rect / dome light with transparent shadows: fused kernels only
    bool pow_spec = false;        // a Blinn material with specExp != 1 (frame1 / shade1 kernels with pow)
    size_t bytes = 0;             // mrt_scene_info.device_bytes: the arrays of upload_scene
    // refit (mrt_refit.hip): per mesh the first float4 of its slice of verts / normals, the
    // world hierarchy and its canonical -> device node numbers (the LDS breadth-first
    // permutation; empty = identity)
    std::vector<uint32_t> vbase, nbase;
    std::vector<int32_t> node_perm;
    RefitTree world;                      // nodes, packets and PrimShade records from 0
    // mrt_scene_deform_mesh: where each BLAS lies in nodes / leaves / prims (its child words hold
    // device node and packet numbers), and what the first refit adds: its tree's schedule and
    // the ids of its instances
    struct BlasRange {
        RefitTree tree;
        uint32_t inst_at = 0, n_inst = 0;      // refit_blas_insts[inst_at .. inst_at + n_inst): its instances, ascending
    };
    std::vector<BlasRange> blas;
    uint32_t n_leaves_all = 0;             // packets of the world and every BLAS (refit_lbox holds them all)
};

// The arrays, named as in DESIGN.md §4; textures and dome tables are copied from the Scene itself.
struct DeviceImage : ImageInfo {
    std::vector<F4> V, N, V2;          // vertices, normals, time-1 vertices (has_mb)
    std::vector<PrimShade> PS;         // world objects, then each BLAS's
    bool any_uv = false;               // texture-mapped meshes: per prim uv indices, (u, v) pairs, per normal tangent / bitangent
    std::vector<U4> PUV;
    std::vector<F2> UV;
    std::vector<F4> TN, BTN;
    std::vector<uint8_t> PF;           // per world prim bit 0 = MBObject lane (has_mb)
    std::vector<QNode> DN;             // the world hierarchy, then each BLAS's
    std::vector<DLeaf> DL;
    std::vector<DevInstance> DI;
    std::vector<int32_t> hit_base;     // instance-major ray-bin keys (mrt_bin.h): hit bases, 7-bit classes (rank by BLAS,
    std::vector<uint16_t> cls;         //   then index), object-space cells: BLAS box lo + BLAS bit, 4 / extent
    std::vector<F4> cell;
    std::vector<uint16_t> tab;         // the x86 rcp / rsqrt approximation tables
};

int build_image(const Scene& s, DeviceImage& img, std::string& err);   // MRT_OK, or MRT_ERR_OVERFLOW with err
void root_box(const QNode& root, float lo[3], float hi[3]);            // union of the root's used slot boxes (finite values)
// point_only, dome, transparent, recursive, pow_spec and disperse of g from s.lights, s.materials and s.path_trace
void shading_flags(const Scene& s, ImageInfo& g);

}  // namespace mrt
